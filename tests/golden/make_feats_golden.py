#!/usr/bin/env python
"""Generate tests/golden/feats.npz and feats_signatures.json from the LIVE reference's feat_deltas /
FeatureDeltas and mean_var_norm / MeanVarianceNormalization.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference/src python tests/golden/make_feats_golden.py

Every array is DATA: inputs this script draws and what the reference returned for them.  Case k of a
family stores its inputs and outputs under ``<family>_<k>_<name>`` and its arguments as a JSON string
under ``<family>_<k>_kw``; error cases store the reference's exception type name.
"""
import inspect
import itertools
import json
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("PDT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))

import pydrobert.torch.functional as RF  # noqa: E402
import pydrobert.torch.modules as RM  # noqa: E402

warnings.simplefilter("ignore")
rng = np.random.default_rng(0x5EED0FEA)
out = {}


def put(key, v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    out[key] = np.asarray(v)


def upstream(shape, dtype):
    """The fixed upstream gradient of every case (tests/test_feats_*.py restate it)."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


def deltas():
    k = 0
    for dt, order, width, mode in itertools.product(("float32", "float64"), range(4), (1, 2, 3),
                                                    ("replicate", "reflect", "circular", "constant")):
        if dt == "float64" and width != 1:
            continue
        P = width * order
        Ts = sorted({1, 2, max(P, 1), P + 1, 37})
        for T in Ts:
            if (mode == "reflect" and P >= T) or (mode == "circular" and P > T):
                continue
            # one placement per case, cycling through every (dim, time_dim, concatenate) of a 4-D x
            conc = bool(k % 2)
            Dd = 4 if conc else 5
            td = (k // 2) % 4
            dim = (k // 8) % Dd - (Dd if (k // 3) % 2 else 0)
            shape = [2, 2, 2, 2]
            shape[td] = T
            x = torch.from_numpy(rng.standard_normal(shape)).to(getattr(torch, dt))
            x.requires_grad_(True)
            kw = dict(dim=dim, time_dim=td, concatenate=conc, order=order, width=width, pad_mode=mode,
                      value=0.75 if mode == "constant" else 0.0)
            y = RF.feat_deltas(x, **kw)
            g = upstream(tuple(y.shape), x.dtype)
            (gx,) = torch.autograd.grad(y, x, g)
            pre = "deltas_{}_".format(k)
            put(pre + "kw", json.dumps(kw))
            put(pre + "x", x)
            put(pre + "y", y)
            put(pre + "gx", gx)
            k += 1
    put("deltas_n", k)
    for order, width in itertools.product(range(4), (1, 2, 3)):
        put("filters_{}_{}".format(order, width), RM.FeatureDeltas(order=order, width=width).filters)


def mvn():
    k = 0
    for dim, stats in itertools.product(range(-3, 3), ("computed", "mean", "std", "both")):
        shape = (4, 5, 6)
        x = torch.from_numpy(rng.standard_normal(shape) * 3 + 2)
        X = shape[dim]
        sl = [slice(None)] * 3
        sl[dim] = 1
        x[tuple(sl)] = 4.5  # a constant feature: std 0, the clamp engages
        x.requires_grad_(True)
        mean = torch.from_numpy(rng.standard_normal(X)).requires_grad_(True) if stats in ("mean", "both") else None
        std = (torch.from_numpy(rng.random(X) + 0.5)).requires_grad_(True) if stats in ("std", "both") else None
        y = RF.mean_var_norm(x, dim, mean, std)
        g = upstream(shape, torch.float64)
        ins = [t for t in (x, mean, std) if t is not None]
        grads = torch.autograd.grad(y, ins, g)
        pre = "mvn_{}_".format(k)
        put(pre + "kw", json.dumps(dict(dim=dim, stats=stats)))
        put(pre + "x", x)
        put(pre + "y", y)
        put(pre + "gx", grads[0])
        if mean is not None:
            put(pre + "mean", mean)
            put(pre + "gmean", grads[1])
        if std is not None:
            put(pre + "std", std)
            put(pre + "gstd", grads[-1])
        k += 1
    put("mvn_n", k)
    # accumulate over chunks (float64: the reference's sums are then the exact float64 ones), store both ways
    chunks = [torch.from_numpy(rng.standard_normal((int(rng.integers(3, 9)), 7, 5)) * 2 - 1) for _ in range(6)]
    for bessel in (False, True):
        m = RM.MeanVarianceNormalization(dim=1)
        for c in chunks:
            m.accumulate(c)
        put("acc_count", m.count)
        put("acc_sum", m.sum)
        put("acc_sumsq", m.sumsq)
        put("acc_keys_accumulated", json.dumps(sorted(m.state_dict())))
        m.store(bessel=bessel)
        put("acc_mean_b{}".format(int(bessel)), m.mean)
        put("acc_std_b{}".format(int(bessel)), m.std)
        put("acc_keys_stored", json.dumps(sorted(m.state_dict())))
    for i, c in enumerate(chunks):
        put("acc_chunk_{}".format(i), c)
    put("acc_keys_new", json.dumps(sorted(RM.MeanVarianceNormalization().state_dict())))
    put("deltas_keys_new", json.dumps(sorted(RM.FeatureDeltas().state_dict())))


def errors():
    cases = {
        "time_dim_range": lambda: RF.feat_deltas(torch.randn(2, 5, 3), time_dim=3),
        "dim_range": lambda: RF.feat_deltas(torch.randn(2, 5, 3), dim=3),
        "dim_range_stack": lambda: RF.feat_deltas(torch.randn(2, 5, 3), dim=4, concatenate=False),
        "order_negative": lambda: RF.feat_deltas(torch.randn(2, 5, 3), order=-1),
        "width_zero": lambda: RF.feat_deltas(torch.randn(2, 5, 3), width=0),
        "reflect_too_short": lambda: RF.feat_deltas(torch.randn(2, 4, 3), pad_mode="reflect"),
        "circular_too_short": lambda: RF.feat_deltas(torch.randn(2, 3, 3), pad_mode="circular"),
        "empty_time": lambda: RF.feat_deltas(torch.randn(2, 0, 3)),
        "mvn_dim_range": lambda: RF.mean_var_norm(torch.randn(2, 5, 3), 3),
        "mvn_dim_range_neg": lambda: RF.mean_var_norm(torch.randn(2, 5, 3), -4),
        "store_one_sample": lambda: _store_after(1),
        "store_nothing": lambda: RM.MeanVarianceNormalization().store(),
        "ctor_order": lambda: RM.FeatureDeltas(order=-1),
        "ctor_pad_mode": lambda: RM.FeatureDeltas(pad_mode="zeros"),
        "ctor_mean_ndim": lambda: RM.MeanVarianceNormalization(mean=torch.zeros(2, 2)),
        "ctor_mean_std_len": lambda: RM.MeanVarianceNormalization(mean=torch.zeros(2), std=torch.ones(3)),
        "ctor_eps": lambda: RM.MeanVarianceNormalization(eps=-1.0),
    }
    names = {}
    for key, fn in cases.items():
        try:
            fn()
            names[key] = "none"
        except Exception as e:  # noqa: BLE001
            names[key] = type(e).__name__
    put("errors", json.dumps(names))


def _store_after(n):
    m = RM.MeanVarianceNormalization()
    m.accumulate(torch.randn(n, 3))
    m.store()


def params(fn):
    fn = getattr(fn, "__wrapped__", fn)
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name, repr(p.default)
             if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def signatures():
    sig = {"functional": {n: params(getattr(RF, n)) for n in ("feat_deltas", "mean_var_norm")}, "modules": {}}
    for n in ("FeatureDeltas", "MeanVarianceNormalization"):
        cls = getattr(RM, n)
        sig["modules"][n] = {"__init__": params(cls.__init__), "forward": params(cls.forward)}
    with open(os.path.join(HERE, "feats_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


torch.manual_seed(0)
deltas()
mvn()
errors()
signatures()
np.savez_compressed(os.path.join(HERE, "feats.npz"), **out)
print("wrote feats.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "feats.npz")), "bytes")
