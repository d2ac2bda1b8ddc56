"""No GPU: the backward of relaxed sampling as an operator of its own -- its C ABI (declarations, argument checks
that return before any launch, the host-only plan), and ``pydrobert_amd::relaxed_backward`` on CPU tensors, where
it takes the torch bodies.

Every call of a launcher below ends in an argument check or an empty size: the pointers are made-up numbers.
"""
import os
import re

import pytest
import torch

import _distributions_check as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pdt_relaxed_backward_parts", "pdt_relaxed_backward_workspace_bytes", "pdt_relaxed_gumbel_backward",
         "pdt_relaxed_bernoulli_backward")
RSAMPLE, THRESHOLD, TLOG_PROB, CSAMPLE, LOG_PROB, CLOG_PROB = range(6)
DIFFERENTIABLE = (RSAMPLE, TLOG_PROB, CSAMPLE, LOG_PROB, CLOG_PROB)
PTR = 4096  # (never dereferenced)


def test_symbols_declared_with_matching_arity():
    from pydrobert_amd import _cabi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdt_amd.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for n in NAMES:
        assert n in _cabi.SIGNATURES and hasattr(lib, n), n
        declared = re.search(r"\b" + n + r"\s*\(([^)]*)\)\s*;", header)
        assert declared, n
        assert len(declared.group(1).split(",")) == len(_cabi.SIGNATURES[n][1]), n
    assert lib.pdt_amd_abi_version() == _cabi.ABI_VERSION == 14


def _call(fn, op=LOG_PROB, dtype=0, g=PTR, param=PTR, B=2, in1=PTR, in2=PTR, R=6, V=5, gp=PTR, gx=0, ws=PTR):
    return fn(op, dtype, g, param, B, V, 1, in1, in2, R, V, gp, gx, ws, 0)


@pytest.mark.parametrize("name", NAMES[2:])
def test_argument_validation_before_any_launch(name):
    from pydrobert_amd import _cabi

    lib = _cabi.lib()
    fn = getattr(lib, name)
    OK, ARG = _cabi.PDT_OK, _cabi.PDT_E_ARG
    for op in (-1, 6, THRESHOLD):
        assert _call(fn, op=op) == ARG
    for dtype in (-1, 2):
        assert _call(fn, dtype=dtype) == ARG
    for op in DIFFERENTIABLE:
        for missing in ("g", "in1", "param"):
            assert _call(fn, op=op, **{missing: 0}) == ARG, (op, missing)
        assert _call(fn, op=op, gp=0, gx=0) == ARG  # nothing asked for
        assert _call(fn, op=op, R=7) == ARG  # R % B != 0
        assert _call(fn, op=op, B=0) == ARG
        assert _call(fn, op=op, R=0) == OK and _call(fn, op=op, V=0) == OK  # nothing to do
        if op in (CSAMPLE, CLOG_PROB):
            assert _call(fn, op=op, in2=0) == ARG
        if op not in (LOG_PROB, CLOG_PROB):  # no gradient of the first data argument
            assert _call(fn, op=op, gx=PTR) == ARG and _call(fn, op=op, gx=PTR, gp=0) == ARG
    # a shape whose plan has parts needs the workspace
    assert lib.pdt_relaxed_backward_parts(64, 1, 5) > 1
    assert _call(fn, R=64, B=1, ws=0) == ARG
    assert _call(fn, V=2 ** 31) == _cabi.PDT_E_TOO_LONG


def test_plan_and_workspace_spot_values():
    from pydrobert_amd import _cabi

    lib = _cabi.lib()
    parts, ws = lib.pdt_relaxed_backward_parts, lib.pdt_relaxed_backward_workspace_bytes
    # empty or ill-formed sizes
    assert [parts(0, 1, 5), parts(6, 0, 5), parts(6, 2, 0), parts(7, 2, 5), parts(-2, 2, 5)] == [0] * 5
    # one sample row per parameter row, or fewer than eight: the base form
    assert [parts(3, 3, 5), parts(6, 3, 5), parts(7, 1, 65), parts(7, 1, 1), parts(21, 3, 65)] == [1] * 5
    # B = 1: a part per sample row, up to the 4096 waves that fill the device
    assert [parts(8, 1, 5), parts(8, 1, 65), parts(9, 1, 5), parts(64, 1, 5), parts(4096, 1, 5)] == [8, 8, 9, 64, 4096]
    # the parts never leave one empty: 10 ** 6 rows in 4096 parts are 245 each, and 4082 parts of 245 hold them
    assert parts(10 ** 6, 1, 5) == 4082 and parts(4097, 1, 5) == 2049
    # the timed shapes: 32 parameter rows of 64 samples, a part per sample row
    assert parts(64 * 32, 32, 512) == 64 and parts(64 * 32, 32, 32) == 64
    # enough parameter rows: groups of 8 lanes, 8 to a wave -- 4096 waves from 32761 rows on
    assert parts(16 * 32761, 32761, 5) == 1 and parts(16 * 32760, 32760, 5) == 2
    # rows beyond 512 columns are several units: 1500 columns are 3 waves
    assert parts(16 * 1366, 1366, 1500) == 1 and parts(16 * 1365, 1365, 1500) == 2
    for dtype in (0, 1):
        assert ws(dtype, 6, 3, 5) == 0 and ws(dtype, 0, 1, 5) == 0
        assert ws(dtype, 8, 1, 5) == 8 * 1 * 5 * 8
        assert ws(dtype, 64 * 32, 32, 512) == 64 * 32 * 512 * 8
    assert ws(2, 8, 1, 5) == _cabi.PDT_E_ARG


def _inputs(family, op, dtype=torch.double, sample=(2,), lead=(2,), V=3, seed=3):
    """(param, x1, x2) of a method, on the CPU: the parameter ``lead + (V,)``, the data ``sample +`` that."""
    from pydrobert_amd import _relaxed as X

    gen = torch.Generator().manual_seed(seed)
    fam = X.GUMBEL if family == "gumbel" else X.BERNOULLI
    logits = 2 * torch.randn(lead + (V,), dtype=dtype, generator=gen)
    if family == "gumbel":
        logits = logits.log_softmax(-1)
    probs = logits.exp() if family == "gumbel" else logits.sigmoid()
    shape = sample + lead + (V,)
    u, v = (torch.rand(shape, dtype=dtype, generator=gen) * 0.96 + 0.02 for _ in range(2))
    z = X._TORCH[fam](X.RSAMPLE, logits, u, None)
    b = X._TORCH[fam](X.THRESHOLD, None, z, None)
    zcond = X._TORCH[fam](X.CSAMPLE, probs, b, v)
    return fam, {RSAMPLE: (logits, u, None), TLOG_PROB: (logits, b, None), CSAMPLE: (probs, b, v),
                 LOG_PROB: (logits, z, None), CLOG_PROB: (logits, zcond, b)}[op]


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
@pytest.mark.parametrize("op", DIFFERENTIABLE)
def test_op_on_cpu_tensors_is_autograd_through_the_torch_forward(family, op):
    from pydrobert_amd import _relaxed as X

    fam, (param, x1, x2) = _inputs(family, op)
    leaf, x1_leaf = param.clone().requires_grad_(True), x1.clone().requires_grad_(op in (LOG_PROB, CLOG_PROB))
    out = X._TORCH[fam](op, leaf, x1_leaf, x2)
    g = torch.cos(torch.arange(out.numel(), dtype=out.dtype) * 0.7).reshape(out.shape)
    wrt = [leaf] + ([x1_leaf] if x1_leaf.requires_grad else [])
    want = torch.autograd.grad(out, wrt, g)
    for bits in (1, 2, 3) if len(wrt) == 2 else (1,):
        got = torch.ops.pydrobert_amd.relaxed_backward(fam, op, bits, g, param, x1, x2)
        assert got[0].shape == (param.shape if bits & 1 else (0,)) and got[1].shape == (x1.shape if bits & 2 else (0,))
        if bits & 1:
            assert torch.allclose(got[0], want[0], rtol=1e-12, atol=1e-12)
        if bits & 2:
            assert torch.allclose(got[1], want[1], rtol=1e-12, atol=1e-12)
    with pytest.raises(RuntimeError):
        torch.ops.pydrobert_amd.relaxed_backward(fam, op, 0, g, param, x1, x2)
    if len(wrt) == 1:
        with pytest.raises(RuntimeError):
            torch.ops.pydrobert_amd.relaxed_backward(fam, op, 2, g, param, x1, x2)


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
def test_fake_shapes_for_every_want(family):
    from torch._subclasses.fake_tensor import FakeTensorMode

    for op in DIFFERENTIABLE:
        fam, (param, x1, x2) = _inputs(family, op, sample=(4,), lead=(1, 2))
        x1 = x1.expand(4, 3, 2, 3)  # (the data may broadcast over a size-1 dimension of the parameter)
        x2 = None if x2 is None else x2.expand(4, 3, 2, 3)
        g = torch.ones(x1.shape[:-1] if family == "gumbel" and op in (TLOG_PROB, LOG_PROB, CLOG_PROB) else x1.shape,
                       dtype=x1.dtype)
        for bits in (1, 2, 3) if op in (LOG_PROB, CLOG_PROB) else (1,):
            real = torch.ops.pydrobert_amd.relaxed_backward(fam, op, bits, g, param, x1, x2)
            with FakeTensorMode() as mode:
                fake = torch.ops.pydrobert_amd.relaxed_backward(
                    fam, op, bits, *(None if t is None else mode.from_tensor(t) for t in (g, param, x1, x2)))
            for r, f in zip(real, fake):
                assert r.shape == f.shape and r.dtype == f.dtype
            assert real[0].shape == (param.shape if bits & 1 else (0,))
            assert real[1].shape == (x1.shape if bits & 2 else (0,))


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
def test_gradcheck_of_the_operators_registered_derivative(family):
    """The second derivative: the operator is differentiable in g, the parameter and the relaxed sample."""
    from torch.autograd import gradcheck

    for op in DIFFERENTIABLE:
        fam, (param, x1, x2) = _inputs(family, op, sample=(2,), lead=(), V=3)
        reduces = family == "gumbel" and op in (TLOG_PROB, LOG_PROB, CLOG_PROB)
        g = torch.cos(torch.arange(x1[..., 0].numel() if reduces else x1.numel(), dtype=x1.dtype) * 0.7)
        g = g.reshape(x1.shape[:-1] if reduces else x1.shape).requires_grad_(True)
        param = param.clone().requires_grad_(True)
        bits = 3 if op in (LOG_PROB, CLOG_PROB) else 1
        x1 = x1.clone().requires_grad_(bits == 3)

        def fn(g_, p_, x_):
            outs = torch.ops.pydrobert_amd.relaxed_backward(fam, op, bits, g_, p_, x_, x2)
            return outs if bits == 3 else outs[0]

        assert gradcheck(fn, (g, param, x1)), (family, op)


def test_public_methods_take_the_operator():
    """The distributions' backward goes through the new operator, once per method."""
    from torch.utils._python_dispatch import TorchDispatchMode

    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    logits = torch.randn(2, 3, dtype=torch.double).requires_grad_(True)
    dist = C.build("gumbel", logits, False)
    z = dist.rsample([4]).detach()
    out = dist.log_prob(z).sum()
    with Record():
        torch.autograd.grad(out, logits)
    assert sum("relaxed_backward" in name for name in seen) == 1, seen
