"""CPU: the plan of the fused ConcatSoftAttention score restated in Python against the library's own report, the
form every named case claims, the C ABI's descriptor errors and zero-size returns, the module's CPU route, and the
measured float32 bounds of tests/_concat_ref.py recomputed and held to the rule exactly."""
import os
import re

import pytest
import torch

import _concat_ref as R
import _wide as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def _plan(lib, desc, dt):
    out = torch.full((5,), -7, dtype=torch.int64)
    rc = lib.pdt_concat_score_plan(desc.data_ptr(), dt, out.data_ptr())
    return rc, dict(zip(("rt", "hchunks", "fpw", "chunks", "ws"), out.tolist()))


def _operands(name):
    """meta tensors of a case's operator call: (wq, wk, v, dim)."""
    c = R.CASES[name]
    dtype = torch.float32 if c["dtype"] == "float32" else torch.float64
    S, _, _ = R.geometry(c)
    q1 = list(c["q"])
    q1.insert(c["dim"], 1)
    wq = torch.empty(q1 + [c["H"]], dtype=dtype, device="meta")
    wk = R.as_seen(name, torch.empty(list(c["k"]) + [c["H"]], dtype=dtype, device="meta"), S)
    return wq, wk, torch.empty(c["H"], dtype=dtype, device="meta"), c["dim"]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_plan_of_equals_the_library_and_cases_reach_their_forms(lib, name):
    from pydrobert_amd import _attn

    c = R.CASES[name]
    wq, wk, v, dim = _operands(name)
    plan = _attn._ConcatPlan(wq, wk, v, dim)
    S, G, M = R.geometry(c)
    assert (plan.S, plan.R, plan.M, plan.T, plan.H) == (S, G * M, M, S[dim], c["H"])
    dt = 0 if c["dtype"] == "float32" else 1
    rc, got = _plan(lib, plan.desc, dt)
    want = R.plan_of(G, M, S[dim], c["H"], 8 if dt else 4)
    assert rc == 0 and got == want, (got, want)
    assert {k: got[k] for k in c["form"]} == c["form"], (name, got)
    assert lib.pdt_concat_score_workspace_bytes(plan.desc.data_ptr(), dt, 1) == want["ws"]
    assert lib.pdt_concat_score_workspace_bytes(plan.desc.data_ptr(), dt, 0) == 0


def test_every_form_is_reached_by_some_case():
    forms = [c["form"] for c in R.CASES.values()]
    assert {f["fpw"] for f in forms} == {4, 8, 16, 32}
    assert {f["hchunks"] for f in forms} == {1, 2} and {f["chunks"] for f in forms} >= {1, 2, 3}
    assert {f["rt"] for f in forms} >= {1, 2, 3, 8}
    lds = [c for c in R.CASES.values() if c["test"] == "lds"]
    assert all(c["form"]["rt"] < min(8, R.geometry(c)[2]) for c in lds)  # fewer rows than the group by LDS alone
    assert any(c["dtype"] == "float64" and c["H"] == 4096 for c in lds)
    # a combine of several chunks against a direct write, at otherwise equal shapes
    assert R.CASES["T32_decode"]["form"]["chunks"] == 1 and R.CASES["T33_decode"]["form"]["chunks"] == 2
    # the decode and training shapes of profiles/tools/time_attn.py
    assert R.plan_of(128, 8, 512, 1000, 4) == dict(rt=8, hchunks=1, fpw=32, chunks=16, ws=(2048 + 16384) * 4000)
    assert R.plan_of(256, 1, 512, 1000, 4)["fpw"] == 32


def test_descriptor_errors_and_zero_sizes(lib):
    from pydrobert_amd import _attn, _cabi

    wq, wk, v, dim = _operands("M9")
    good = _attn._ConcatPlan(wq, wk, v, dim).desc
    assert _plan(lib, good, 0)[0] == _cabi.PDT_OK
    assert lib.pdt_concat_score_plan(0, 0, good.data_ptr()) == _cabi.PDT_E_ARG
    assert lib.pdt_concat_score_plan(good.data_ptr(), 0, 0) == _cabi.PDT_E_ARG
    assert _plan(lib, good, 2)[0] == _cabi.PDT_E_ARG  # no such dtype
    assert lib.pdt_concat_score_workspace_bytes(good.data_ptr(), 0, 2) == -1  # no such kind
    base = 7 + _attn._MAX_DIMS
    for index, value in (
        (0, 9), (0, -1),  # more row dims than PDT_ATTN_MAX_DIMS, fewer than none
        (1, 17), (2, 3), (3, 5),  # R, G, M that do not multiply
        (4, -1), (5, -1),  # negative T, H
        (7, 3),  # sizes whose product is not R
        (base + 1 * (_attn._MAX_DIMS + 2) + 1, 65),  # wk strided along the group
        (base + 6 * (_attn._MAX_DIMS + 2) + 1, 65),  # grad_wk strided along the group
    ):  # fmt: skip
        bad = good.clone()
        bad[index] = value
        assert _plan(lib, bad, 0)[0] == _cabi.PDT_E_ARG, (index, value)
        assert lib.pdt_concat_score_workspace_bytes(bad.data_ptr(), 0, 1) == -1
        assert lib.pdt_concat_score(bad.data_ptr(), 0, 8, 8, 8, 8, 0) == _cabi.PDT_E_ARG
        assert lib.pdt_concat_score_backward(bad.data_ptr(), 0, 8, 8, 8, 8, 8, 8, 8, 8, 1 << 40, 0) == _cabi.PDT_E_ARG
    # null pointers and a short workspace with work to do: refused before any launch
    assert lib.pdt_concat_score(good.data_ptr(), 0, 0, 8, 8, 8, 0) == _cabi.PDT_E_ARG
    assert lib.pdt_concat_score(good.data_ptr(), 0, 8, 8, 8, 0, 0) == _cabi.PDT_E_ARG
    assert lib.pdt_concat_score_backward(good.data_ptr(), 0, 8, 8, 8, 8, 8, 8, 0, 8, 1 << 40, 0) == _cabi.PDT_E_ARG
    assert lib.pdt_concat_score_backward(good.data_ptr(), 0, 8, 8, 8, 8, 8, 8, 8, 8, 8, 0) == _cabi.PDT_E_ARG
    assert lib.pdt_concat_score_backward(good.data_ptr(), 0, 8, 8, 8, 8, 8, 8, 8, 0, 1 << 40, 0) == _cabi.PDT_E_ARG
    # grids beyond 2^31 - 1 workgroups
    huge = good.clone()
    huge[1], huge[2], huge[7], huge[4] = 9 << 40, 1 << 40, 1 << 40, 1 << 20
    assert _plan(lib, huge, 0)[0] == _cabi.PDT_E_TOO_LONG
    # R == 0, T == 0, H == 0: OK without a launch (null pointers are not even looked at), an all-zero plan
    for index in (1, 4, 5):
        empty = good.clone()
        empty[index] = 0
        if index == 1:
            empty[2], empty[7] = 0, 0
        rc, plan = _plan(lib, empty, 1)
        assert rc == _cabi.PDT_OK and set(plan.values()) == {0}, plan
        assert lib.pdt_concat_score(empty.data_ptr(), 1, 0, 0, 0, 0, 0) == _cabi.PDT_OK
        assert lib.pdt_concat_score_backward(empty.data_ptr(), 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == _cabi.PDT_OK
        assert lib.pdt_concat_score_workspace_bytes(empty.data_ptr(), 1, 1) == 0


def test_entry_points_declared_and_bound(lib):
    from pydrobert_amd import _cabi

    header = open(os.path.join(ROOT, "include", "pdt_amd.h")).read()
    for n in ("pdt_concat_score", "pdt_concat_score_backward", "pdt_concat_score_workspace_bytes",
              "pdt_concat_score_plan"):  # fmt: skip
        assert n in _cabi.SIGNATURES and re.search(r"\b" + n + r"\s*\(", header) and hasattr(lib, n)
    assert lib.pdt_amd_abi_version() == _cabi.ABI_VERSION


def test_operators_registered_with_fake_implementations():
    from pydrobert_amd import _attn  # noqa: F401

    wq, wk, v, dim = _operands("xfmr")
    e = torch.ops.pydrobert_amd.concat_score(wq, wk, v, dim)
    assert list(e.shape) == R.geometry(R.CASES["xfmr"])[0] and e.dtype == torch.float32
    grads = torch.ops.pydrobert_amd.concat_score_backward(e, wq, wk, v, dim)
    assert [g.shape for g in grads] == [wq.shape, wk.shape, v.shape]
    for bad_dim in (-1, 2):
        with pytest.raises(RuntimeError):
            torch.ops.pydrobert_amd.concat_score(wq, wk, v, bad_dim)
    with pytest.raises(RuntimeError):
        torch.ops.pydrobert_amd.concat_score(wq.expand(40, -1, -1, -1), wk, v, dim)  # wq spans the attended axis
    with pytest.raises(RuntimeError, match="ROCm"):
        torch.ops.pydrobert_amd.concat_score(torch.zeros(1, 2, 3), torch.zeros(4, 2, 3), torch.zeros(3), 0)


@pytest.mark.parametrize("qs,ks,shape,R,M", [
    ((1, 0, 3, 7), (5, 0, 1, 7), [5, 0, 3], 0, 3),  # an empty batch
    ((1, 2, 0, 7), (5, 2, 1, 7), [5, 2, 0], 0, 0),  # no beams
    ((1, 2, 3, 7), (0, 2, 1, 7), [0, 2, 3], 6, 3),  # no frames
    ((1, 2, 3, 0), (5, 2, 1, 0), [5, 2, 3], 6, 3),  # no hidden units
])  # fmt: skip
def test_zero_size_shapes_in_the_plan_and_the_fake_operators(qs, ks, shape, R, M):
    """A dim of size 0 is a row dim, so R is 0 with it (and the operators return before any launch); the fake
    implementations give the shapes the operators give."""
    from pydrobert_amd import _attn

    wq, wk = torch.empty(qs, device="meta"), torch.empty(ks, device="meta")
    v = torch.empty(qs[-1], device="meta")
    plan = _attn._ConcatPlan(wq, wk, v, 0)
    assert (plan.S, plan.R, plan.M, plan.T, plan.H) == (shape, R, M, shape[0], qs[-1])
    assert plan.R == 0 or plan.T == 0 or plan.H == 0
    e = torch.ops.pydrobert_amd.concat_score(wq, wk, v, 0)
    assert list(e.shape) == shape
    grads = torch.ops.pydrobert_amd.concat_score_backward(e, wq, wk, v, 0)
    assert [g.shape for g in grads] == [wq.shape, wk.shape, v.shape]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16])
def test_cpu_route_is_the_torch_body_bit_for_bit(dtype):
    from pydrobert_amd import _attn
    from pydrobert_amd import modules as M

    torch.manual_seed(3)
    m = M.ConcatSoftAttention(5, 6, 0, True, 7).to(dtype)
    q, k = torch.randn(3, 2, 5, dtype=dtype), torch.randn(9, 3, 1, 6, dtype=dtype)
    wq = torch.nn.functional.linear(q.unsqueeze(0), m.weight[:, :5], m.bias)
    wk = torch.nn.functional.linear(k, m.weight[:, 5:], None)
    want = _attn._concat_score_torch(wq, wk, m.v)
    assert torch.equal(m.score(q, k), want) and want.shape == (9, 3, 2)
    assert torch.equal(want, torch.nn.functional.linear(torch.tanh(wq + wk), m.v.unsqueeze(0), None).squeeze(-1))
    assert not _attn._concat_hip_route(wq, wk, m.v, 0)
    assert torch.equal(torch.jit.script(m).score(q, k), want)


def test_formulas_agree_with_autograd():
    """The written-out gradients of tests/_concat_ref.py are the derivative of its score."""
    for name in ("xfmr_f64", "expanded_f64", "M17_f64"):
        got = R.run_case(name, lambda wq, wk, v, dim: R.score_ref(wq, wk, v), torch.float64, "cpu")
        for n, ref in R.expected(name).items():
            assert torch.allclose(got[n], ref, rtol=1e-12, atol=1e-12), (name, n)


@pytest.mark.parametrize("name", sorted(n for n, c in R.CASES.items() if c["dtype"] == "float32"))
def test_measured_tolerances_follow_the_rule(name):
    """Every float32 bound is the rule's and nothing else: the suite's where 8 x err32 is not above it, otherwise
    8 x err32 rounded up to two digits, err32 the error of the float32 formula on the case's inputs, recomputed here
    (``_concat_ref.formula32`` writes out every operation, so the figure does not depend on the machine).  Every
    bound is under 1 % of the median |reference| of its tensor."""
    c = R.CASES[name]
    refs = R.expected(name)
    assert set(c["tol"]) <= set(refs)
    err32 = R.formula32_error(name)
    for n, ref in refs.items():
        suite, atol = R.bound(name, n)
        print("{} {}: err32 {:.3e}, 8 x err32 {:.3e}, bound {:.1e}".format(name, n, err32[n], 8 * err32[n], atol))
        assert atol == R.measured_bound(err32[n], suite), (n, err32[n], atol)
        assert (n in c["tol"]) == (atol != suite), n  # (no entry that merely repeats the suite's bound)
        mag = ref.abs()[ref != 0]
        assert atol < 0.01 * float(mag.median()), (n, atol, float(mag.median()))


def test_measured_bound_is_the_rule():
    assert R.measured_bound(1.0e-6, 2e-5) == 2e-5 and R.measured_bound(2.5e-6, 2e-5) == 2e-5
    assert R.measured_bound(2.51e-6, 2e-5) == 2.1e-5 and R.measured_bound(5.0e-6, 2e-5) == 4.0e-5
    assert R.measured_bound(1.2501e-5, 1e-4) == 1.1e-4 and R.measured_bound(2.09e-5, 1e-4) == 1.7e-4


def test_formula32_is_float32_arithmetic_in_a_written_order():
    """The tree sum against a sequential float64 sum, and its order: a float32 tree of [1, 2^-24, 2^-24, 1] is 2
    (each half rounds its small term away), where any order that added the two small terms first would give 2 + 2^-22."""
    x = torch.tensor([1.0, 2.0 ** -24, 2.0 ** -24, 1.0])
    assert float(R._tree_sum(x, 0)) == 2.0
    y = torch.randn(7, 1001, dtype=torch.float64)
    assert torch.allclose(R._tree_sum(y, 1), y.sum(1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(R._tree_sum_to(y.view(7, 7, 143), (1, 7, 1)), y.view(7, 7, 143).sum((0, 2), keepdim=True))
    w, b = torch.randn(5, 3, dtype=torch.float64), torch.randn(5, dtype=torch.float64)
    q = torch.randn(4, 2, 3, dtype=torch.float64)
    assert torch.allclose(R._linear32(q, w, b), torch.nn.functional.linear(q, w, b), rtol=1e-13, atol=1e-13)
    for name in ("xfmr", "expanded", "batch_first"):
        got, ref = R.formula32(name), R.expected(name)
        for n in R.TENSORS:
            assert got[n].dtype == torch.float32 and got[n].shape == ref[n].shape
            assert torch.allclose(got[n].double(), ref[n], rtol=1e-4, atol=1e-4), (name, n)


def test_float64_cases_keep_the_suite_bound():
    for name, c in R.CASES.items():
        if c["dtype"] == "float64":
            assert not c["tol"], name


def test_wide_layout():
    """The view of the offsets test: wk (T, N, 1, H) with batch element 1 beyond 2^32 elements, every wrapped
    offset on a decoy and inside the buffer (tests/_wide.py, check_layout)."""
    w = R.WIDE
    shape = (w["T"], w["N"], 1, w["H"])
    strides, A = W.wide_strides(shape, w["wide_dim"])
    W.check_layout(shape, strides, w["wide_dim"], W.MIN_NUMEL)
    view = W.wide_view(torch.empty(W.MIN_NUMEL, dtype=torch.float32, device="meta"), torch.empty(shape), w["wide_dim"])
    assert view.stride(1) == W.WRAP + A and view.shape == shape
