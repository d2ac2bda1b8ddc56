"""What tests/test_distributions_cpu.py and tests/test_distributions_gpu.py share: the golden file, the
substitution of recorded noise for ``torch.rand`` / ``torch.rand_like``, and the check of one golden case of
a relaxed distribution on one device.

Continuous results are held to tests/_distributions_ref.py -- float64, clamping at the eps of the dtype under
test -- within the bound the golden maker measured and stored (``tol_<family>_<output>_<dtype>``, in units of
eps (1 + |value|); gradients are taken with respect to the distribution's own logits / probs, and the yardstick
is evaluated at the values those tensors have in the distribution under test).  Discrete results are compared exactly, and always
computed from the golden ``z`` / ``zcond``, never from the code's own, ulp-different ones.
"""
import contextlib
import functools
import json
import os

import numpy as np
import torch

import _distributions_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = {"gumbel": "GumbelOneHotCategorical", "bernoulli": "LogisticBernoulli"}


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(os.path.join(HERE, "golden", "distributions.npz"))


@functools.lru_cache(maxsize=None)
def cases():
    return json.loads(str(gold()["cases"]))


@functools.lru_cache(maxsize=None)
def signatures():
    with open(os.path.join(HERE, "golden", "distributions_signatures.json")) as f:
        return json.load(f)


def tolerance(family, output, dtype):
    return float(gold()["tol_{}_{}_{}".format(family, output, dtype)])


@contextlib.contextmanager
def noise(*tensors):
    """torch.rand and torch.rand_like return ``tensors`` in order (on the device and in the dtype asked for)."""
    queue = list(tensors)
    saved = torch.rand, torch.rand_like

    def pop(shape, dtype, device):
        t = queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.to(device=device, dtype=dtype).clone()

    torch.rand = lambda shape, **kw: pop(shape, kw.get("dtype", torch.float32), kw.get("device", "cpu"))
    torch.rand_like = lambda t, **kw: pop(t.shape, t.dtype, t.device)
    try:
        yield
        assert not queue
    finally:
        torch.rand, torch.rand_like = saved


def tensors(k):
    """The recorded arrays of case ``k`` as CPU tensors in the case's dtype (inputs from the float32 twin)."""
    g, case = gold(), cases()[k]
    dtype = getattr(torch, case["dtype"])
    rec = {}
    for name in ("param", "u", "v"):
        src = k if case["dtype"] == "float32" else k - 1
        rec[name] = torch.from_numpy(g["case_{}_{}".format(src, name)]).to(dtype)
    for name in ("z", "b", "zcond", "log_prob", "tlog_prob", "clog_prob") + tuple("g_" + n for n in ref.CONTINUOUS):
        rec[name] = torch.from_numpy(g["case_{}_{}".format(k, name)]).to(dtype)
    return case, dtype, rec


def reference(k, at=None):
    """tests/_distributions_ref.py on the recorded inputs of case ``k``: outputs, and gradients evaluated at the
    logits / probs ``at`` of the distribution under test."""
    case, dtype, rec = tensors(k)
    eps = float(torch.finfo(dtype).eps)
    return ref.evaluate(case["family"], ref.f64(rec["param"]), case["probs"], *ref.f64(rec["u"], rec["v"]), eps,
                        *ref.f64(rec["z"], rec["b"], rec["zcond"]), at=at)


def build(family, param, from_probs, **kw):
    from pydrobert_amd import distributions as D

    return getattr(D, NAMES[family])(**{"probs" if from_probs else "logits": param}, **kw)


def check_case(k, device, report=None):
    """Every method of the distribution of case ``k`` on ``device``; returns ``{output: units}``."""
    case, dtype, rec = tensors(k)
    family, eps = case["family"], float(torch.finfo(dtype).eps)
    on = {name: t.to(device) for name, t in rec.items()}
    param = on["param"].clone().requires_grad_(True)
    dist = build(family, param, case["probs"])
    want, want_g = reference(k, dict(logits=ref.f64(dist.logits).cpu(), probs=ref.f64(dist.probs).cpu()))
    with noise(rec["u"]):
        z = dist.rsample(tuple(case["sample"]))
    assert z.dtype == dtype and z.device.type == device.type and z.shape == rec["z"].shape
    assert torch.equal(dist.threshold(on["z"]), on["b"])
    with noise(rec["v"]):
        zcond = dist.csample(on["b"])
    assert torch.equal(dist.threshold(zcond), on["b"])  # (of the code's own zcond: csample's contract)
    assert torch.equal(dist.threshold(on["zcond"]), on["b"])
    got = dict(z=z, zcond=zcond, log_prob=dist.log_prob(on["z"]), tlog_prob=dist.tlog_prob(on["b"]),
               clog_prob=dist.clog_prob(on["zcond"], on["b"]))
    assert torch.isfinite(got["clog_prob"]).all()
    figures = {}
    for name in ref.CONTINUOUS:
        assert got[name].dtype == dtype and got[name].shape == rec[name].shape, name
        figures[name] = ref.units(got[name], want[name], eps)
        (g,) = torch.autograd.grad(got[name], getattr(dist, ref.WRT[name]),
                                   ref.upstream(got[name].shape, dtype).to(device), retain_graph=True)
        figures["g_" + name] = ref.units(g, want_g["g_" + name], eps)
    if report is not None:
        report(k, case, figures)
    for name, d in figures.items():
        assert d <= tolerance(family, name, case["dtype"]), (k, case, name, d, tolerance(family, name, case["dtype"]))
    return figures


def lookup_lm(device):
    """The n-gram model stored in the golden file, on ``device``, and ``(V, sos, eos, T)``."""
    from pydrobert_amd.modules import LookupLanguageModel

    g = gold()
    V, sos, N, eos, T = (int(x) for x in g["seq_cfg"])
    dicts = []
    for n in range(N):
        d = {}
        for key, val in zip(g["seq_keys{}".format(n)], g["seq_vals{}".format(n)]):
            key = int(key[0]) if n == 0 else tuple(int(x) for x in key)
            d[key] = float(val[0]) if n == N - 1 else (float(val[0]), float(val[1]))
        dicts.append(d)
    return LookupLanguageModel(V, sos, dicts).to(device), (V, sos, eos, T)
