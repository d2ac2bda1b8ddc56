#!/usr/bin/env python
"""Generate tests/golden/rl_comb.npz and rl_comb_signatures.json from the LIVE reference's
time_distributed_return / TimeDistributedReturn and its combinatorics functions.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference/src python tests/golden/make_rl_comb_golden.py

Every array is DATA: inputs this script draws and what the reference returned for them.  Case k of a
family stores its inputs and outputs under ``<family>_<k>_<name>`` and its arguments as a JSON string
under ``<family>_<k>_kw``; error cases store the reference's exception type name.

The reference's return is a product with a matrix of power ratios, so each return case is first held
against a float64 recurrence: it is kept only if it lies within (T + 8) eps A[t] of it,
A[t] = sum_{t' >= t} |gamma|^(t' - t) |r[t']| (the cases that do not are listed in ``return_dropped``).
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
rng = np.random.default_rng(0x5EED0C0B)
out = {}


def put(key, v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    out[key] = np.asarray(v)


def upstream(shape, dtype):
    """The fixed upstream gradient of every case (tests/test_rl_comb_*.py restate it)."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


def recurrence(r, gamma, reverse=False):
    """float64 (T, N): R[t] = r[t] + gamma R[t + 1] (reverse: R[t - 1])."""
    T = r.shape[0]
    R = np.zeros_like(r)
    acc = np.zeros_like(r[0])
    for s in range(T):
        t = s if reverse else T - 1 - s
        acc = r[t] + gamma * acc
        R[t] = acc
    return R


def returns():
    k, dropped = 0, []
    for dt, bf, gamma, T, N in itertools.product(("float32", "float64"), (False, True),
                                                 (0.0, 0.5, 0.9, 1.0, -0.5, 1.5), (1, 2, 7, 64), (1, 3)):
        dtype = getattr(torch, dt)
        x = torch.from_numpy(rng.standard_normal((T, N))).to(dtype)  # time-major; transposed for batch_first
        r = (x.T.contiguous() if bf else x.clone()).requires_grad_(True)
        R = RF.time_distributed_return(r, gamma, bf)
        g = upstream(tuple(R.shape), dtype)
        (gr,) = torch.autograd.grad(R, r, g)
        eps = float(torch.finfo(dtype).eps)
        x64 = x.double().numpy()
        ok = True
        # the output against the recurrence, the gradient against the recurrence's adjoint
        g64 = (g.T if bf else g).double().numpy()
        for got, src, rev in ((R, x64, False), (gr, g64, True)):
            got = (got.detach().T if bf else got.detach()).double().numpy()
            A = recurrence(np.abs(src), abs(gamma), rev)
            ok = ok and bool((np.abs(got - recurrence(src, gamma, rev)) <= (T + 8) * eps * A).all())
        if not ok:
            dropped.append([dt, bf, gamma, T, N])
            continue
        pre = "return_{}_".format(k)
        put(pre + "kw", json.dumps(dict(gamma=gamma, batch_first=bf)))
        put(pre + "r", r)
        put(pre + "R", R)
        put(pre + "gr", gr)
        k += 1
    put("return_n", k)
    put("return_dropped", json.dumps(dropped))


def combinatorics():
    count = torch.arange(67).view(1, 67).expand(67, 67)
    length = torch.arange(67).view(67, 1).expand(67, 67)
    put("binom_small", RF.binomial_coefficient(length[:21], count[:21]))  # max length 20: factorials
    put("binom_large", RF.binomial_coefficient(length, count))  # above 20: the recursion
    k = 0
    for L, V in [(L, V) for L in range(5) for V in range(1, 5)] + [(10, 2)]:
        put("vocab_{}_kw".format(k), json.dumps(dict(length=L, vocab_size=V)))
        put("vocab_{}_out".format(k), RF.enumerate_vocab_sequences(L, V))
        k += 1
    put("vocab_n", k)
    put("vocab_float", RF.enumerate_vocab_sequences(3, 3, dtype=torch.float32))
    put("binary_4", RF.enumerate_binary_sequences(4))
    k = 0
    for L in range(11):
        for c in range(L + 2):
            put("card_{}_kw".format(k), json.dumps(dict(length=L, count=c)))
            put("card_{}_out".format(k), RF.enumerate_binary_sequences_with_cardinality(L, c))
            k += 1
    put("card_n", k)
    # tensor form: (3, 1) x (4,), with length 0 and counts above their length; the valid region only
    length = torch.tensor([[0], [3], [5]])
    count = torch.tensor([0, 1, 2, 4])
    support, binom = RF.enumerate_binary_sequences_with_cardinality(length, count)
    put("cardt_length", length)
    put("cardt_count", count)
    put("cardt_binom", binom)
    put("cardt_shape", np.array(support.shape))
    for i, j in itertools.product(range(3), range(4)):
        put("cardt_valid_{}_{}".format(i, j), support[i, j, : int(binom[i, j]), : int(length[i, 0])])


def errors():
    t = torch.tensor
    cases = {
        "return_1d": lambda: RF.time_distributed_return(torch.randn(5), 0.5),
        "return_3d": lambda: RF.time_distributed_return(torch.randn(5, 2, 2), 0.5),
        "ctor_gamma": lambda: RM.TimeDistributedReturn("a", False),
        "ctor_batch_first": lambda: RM.TimeDistributedReturn(0.5, 1),
        "vocab_length_negative": lambda: RF.enumerate_vocab_sequences(-1, 2),
        "vocab_size_zero": lambda: RF.enumerate_vocab_sequences(2, 0),
        "binary_length_negative": lambda: RF.enumerate_binary_sequences(-1),
        "binom_length_negative": lambda: RF.binomial_coefficient(t([-1, 2]), t([0, 1])),
        "binom_count_negative": lambda: RF.binomial_coefficient(t([1, 2]), t([0, -1])),
        "card_mixed": lambda: RF.enumerate_binary_sequences_with_cardinality(3, t(1)),
        "card_mixed_other": lambda: RF.enumerate_binary_sequences_with_cardinality(t(3), 1),
        "card_length_negative": lambda: RF.enumerate_binary_sequences_with_cardinality(-1, 0),
        "srswor_given_exceeds": lambda: RF.simple_random_sampling_without_replacement(t([3, 2]), t([1, 3])),
        "srswor_out_size_small": lambda: RF.simple_random_sampling_without_replacement(t([3, 5]), t([1, 2]), 4),
    }
    names = {}
    for key, fn in cases.items():
        try:
            fn()
            names[key] = "none"
        except Exception as e:  # noqa: BLE001
            names[key] = type(e).__name__
    put("errors", json.dumps(names))


def params(fn):
    while hasattr(fn, "__wrapped__"):
        fn = fn.__wrapped__
    fn = getattr(fn, "__original_fn", fn)
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name, repr(p.default)
             if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


FUNCTIONS = ("time_distributed_return", "binomial_coefficient", "enumerate_vocab_sequences",
             "enumerate_binary_sequences", "enumerate_binary_sequences_with_cardinality",
             "simple_random_sampling_without_replacement")


def signatures():
    sig = {"functional": {n: params(getattr(RF, n)) for n in FUNCTIONS}, "modules": {}}
    cls = RM.TimeDistributedReturn
    sig["modules"]["TimeDistributedReturn"] = {"__init__": params(cls.__init__), "forward": params(cls.forward)}
    sig["functional_all"] = sorted(RF.__all__)
    sig["modules_all"] = sorted(RM.__all__)
    with open(os.path.join(HERE, "rl_comb_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


torch.manual_seed(0)
returns()
combinatorics()
errors()
signatures()
np.savez_compressed(os.path.join(HERE, "rl_comb.npz"), **out)
print("wrote rl_comb.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "rl_comb.npz")), "bytes")
print("return cases kept:", int(out["return_n"]), "dropped:", str(out["return_dropped"]))
print("errors:", str(out["errors"]))
