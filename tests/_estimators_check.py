"""What tests/test_estimators_cpu.py and tests/test_estimators_gpu.py share: the golden file and the run of one
golden case through this package's estimators on one device.

Results are held to tests/_estimators_ref.py's float64 yardstick within the bound the golden maker measured and
stored (``tol_<estimator>_<output>_<dtype>``, in units of eps (1 + |value|)), or compared with the recorded
values directly (``exact``), where the torch bodies run the reference's own operations on the CPU.
"""
import functools
import json
import os
import types

import numpy as np
import torch

import _estimators_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
# the estimators whose CPU path is the reference's own operations in the reference's order
EXACT_ON_CPU = ("direct", "reparam", "is", "enumerate")
# (M, B, layout of f) of the kernels' parity tests; tests/test_estimators_cpu.py proves they meet every form
PARITY_SHAPES = [
    (1, 1, "dense"), (2, 65, "dense"), (7, 257, "dense"), (63, 257, "dense"), (7, 3, "transposed"),
    (64, 64, "dense"), (65, 65, "dense"), (1025, 257, "dense"), (64, 1, "dense"), (65, 3, "dense"), (1025, 3, "dense"),
    (65, 65, "transposed"), (1025, 64, "transposed"), (64, 16384, "dense"),
]


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(os.path.join(HERE, "golden", "estimators.npz"))


@functools.lru_cache(maxsize=None)
def cases():
    return json.loads(str(gold()["cases"]))


@functools.lru_cache(maxsize=None)
def signatures():
    with open(os.path.join(HERE, "golden", "estimators_signatures.json")) as f:
        return json.load(f)


def tolerance(est, output, dtype):
    return float(gold()["tol_{}_{}_{}".format(est, output, dtype)])


def namespace():
    from pydrobert_amd import distributions, estimators, modules

    return types.SimpleNamespace(E=estimators, D=distributions, M=modules)


def tensors(k):
    """(case, inputs of case ``k`` as CPU tensors in its dtype, recorded outputs)."""
    g, case = gold(), cases()[k]
    dtype = getattr(torch, case["dtype"])
    src = k if case["dtype"] == "float32" else k - 1  # (the inputs are the float32 twin's, widened)
    T, rec = {}, {}
    for name in ("logits", "theta", "w", "w2", "qlogits", "rows", "u", "nv"):
        key = "case_{}_{}".format(src, name)
        if key in g.files:
            t = torch.from_numpy(g[key])
            T[name] = t if t.dtype == torch.int64 or (name == "u" and case["est"] == "imh") else t.to(dtype)
    own = "case_{}_".format(k)
    if own + "b" in g.files:
        T["b"] = torch.from_numpy(g[own + "b"]).to(dtype)
    rec["v"] = torch.from_numpy(g[own + "v"])
    for name in ref.GRADS:
        if own + "g_" + name in g.files:
            rec["g_" + name] = torch.from_numpy(g[own + "g_" + name])
    return case, T, rec


def check_case(k, device, exact=False, report=None):
    """Case ``k`` through this package's estimators on ``device``; returns ``{output: units}``."""
    case, T, rec = tensors(k)
    dtype = getattr(torch, case["dtype"])
    eps = float(torch.finfo(dtype).eps)
    v, grads = ref.drive(namespace(), case, {name: t.to(device) for name, t in T.items()})
    assert v.dtype == dtype and v.device.type == torch.device(device).type and v.shape == rec["v"].shape, (k, case)
    got = {"v": v, **{"g_" + n: g for n, g in grads.items()}}
    assert set(got) == set(rec), (k, case, sorted(got), sorted(rec))
    if exact:
        for name in got:
            assert torch.equal(got[name].detach().cpu(), rec[name]), (k, case, name)
        return {}
    want, want_g = ref.yardstick(case, T)
    want = {"v": want, **{"g_" + n: g for n, g in want_g.items()}}
    figures = {name: ref.units(got[name], want[name], eps) for name in got}
    if report is not None:
        report(k, case, figures)
    for name, d in figures.items():
        tol = tolerance(case["est"], name, case["dtype"])
        assert d <= tol, (k, case, name, d, tol)
    return figures
