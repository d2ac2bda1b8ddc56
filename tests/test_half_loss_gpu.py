"""GPU: float16 / bfloat16 logits through hard_optimal_completion_distillation_loss give, bit for bit, the loss
the float32 route gives on ``x.float()`` and -- in ``x.dtype`` -- its gradient cast with ``.to(x.dtype)``, in
every row form of csrc/ocd_loss.hip and every layout; and neither pass makes a float32 copy of the logits.
Every comparison with the float32 route is one of bit patterns.  One test holds the half route to the float64
set form of tests/_loss_ref.py instead, so that a defect shared by both routes cannot hide."""
import numpy as np
import pytest
import torch

import _half_logits as hl
import _half_loss as hlo
import _loss_ref as LR

pytestmark = pytest.mark.gpu

DTYPES = sorted(hl.HALF_DTYPES)
_INT_OF = {2: torch.int16, 4: torch.int32}


@pytest.fixture(scope="module")
def lib():
    from pydrobert_amd import _cabi

    return _cabi.lib()


def _bits(t):
    t = t.detach().contiguous()
    return t.view(_INT_OF[t.element_size()])


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = _bits(got), _bits(want)
    assert torch.equal(a, b), "{}: {} of {} elements differ".format(what, int((a != b).sum()), a.numel())


def _tok(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _loss(x, ref, hyp, reduction, **kw):
    from pydrobert_amd import functional as F

    return F.hard_optimal_completion_distillation_loss(x, ref, hyp, reduction=reduction, warn=False, **kw)


def _rows_op(x, ref, hyp, weight=None, eos=None, include_eos=True, batch_first=False, ignore_index=-2):
    """(loss, count, bitmask, class_tokens) of the operator behind the loss."""
    return torch.ops.pydrobert_amd.ocd_loss_rows(
        x, ref, hyp, eos, include_eos, batch_first, 1.0, 1.0, 1.0, weight, ignore_index, False
    )


def _compare(base, view, ref, hyp, what, reductions=("none", "mean", "sum"), seed=0, **kw):
    """The loss on the half view ``view(base)`` against the float32 route on ``view(base).float()``: loss bits,
    and the bits of the gradient that reaches ``base`` against the float32 gradient, cast to the half type and
    scattered through the same view into zeros.  Returns (loss, gradient of the view) of ``"none"``."""
    assert base.dtype in hl.HALF_DTYPES.values()
    out = None
    for red in reductions:
        bh = base.detach().requires_grad_(True)
        xh = view(bh)
        xf = view(base).detach().float().contiguous().requires_grad_(True)
        assert xf.dtype == torch.float32 and xf.is_contiguous()
        lh, lf = _loss(xh, ref, hyp, red, **kw), _loss(xf, ref, hyp, red, **kw)
        assert lh.dtype == torch.float32
        _same_bits(lh, lf, "{} {} loss".format(what, red))
        g = torch.Generator().manual_seed(seed + 1)
        gw = torch.randn(tuple(lh.shape), generator=g).to(lh.device)  # (float32 upstream gradient)
        (lh * gw).sum().backward()
        (lf * gw).sum().backward()
        assert bh.grad.dtype == base.dtype and xf.grad.dtype == torch.float32
        want = torch.zeros_like(base)
        view(want).copy_(xf.grad.to(base.dtype))
        _same_bits(bh.grad, want, "{} {} gradient".format(what, red))
        if red == "none":
            out = (lh.detach(), view(bh.grad), xf.grad, gw)
    return out


def _identity(b):
    return b


# ---- 1. row forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_first", [False, True], ids=["tnv", "ntv"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [64, 65, 512, 513, 1024, 1025, 2500])
def test_row_forms_match_float32(device, V, dtype, batch_first):
    """Rows in 8 registers per lane (V <= 512), in 16 (V <= 1024; staged in LDS up to here) and streamed
    (beyond, where a target's gradient element is stored twice), at their edges, with the tokens on both sides
    of every chunk boundary as targets, a class weight and a random upstream gradient."""
    import oracle

    rng = np.random.default_rng(V)
    H, N, R = 9, 3, 11
    forced = hlo.forced_tokens(V)
    ref = rng.integers(0, V, (R, N))
    for n in range(N):
        ref[: len(forced), n] = np.roll(forced, n)
    hyp = rng.integers(0, V, (H, N))
    tgt = oracle.optimal_completion(ref, hyp, padding=-2, exclude_last=True)
    assert set(forced) <= set(tgt.flatten().tolist())
    w = torch.from_numpy(rng.uniform(0.5, 2, V).astype(np.float32)).to(device)
    shape = (N, H, V) if batch_first else (H, N, V)
    x = hl.planted(shape, hl.HALF_DTYPES[dtype], seed=V + 7, device=device)
    if batch_first:
        ref, hyp = ref.T, hyp.T
    ref, hyp = _tok(ref, device), _tok(hyp, device)
    what = "V={} {} bf={}".format(V, dtype, batch_first)
    _, _, gf, gw = _compare(x, _identity, ref, hyp, what, seed=V, weight=w, batch_first=batch_first)
    # the backward operator itself hands back the half type (no float32 gradient behind it)
    _, _, bitmask, class_tokens = _rows_op(x, ref, hyp, weight=w, batch_first=batch_first)
    direct = torch.ops.pydrobert_amd.ocd_loss_rows_backward(
        x, bitmask, class_tokens, w, -2, batch_first, gw.t() if batch_first else gw
    )
    assert direct.dtype == x.dtype
    _same_bits(direct, gf.to(x.dtype), what + " backward op")
    assert float(gf.abs().max()) > 0


# ---- 2. layouts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["offset", "padded", "every_other", "vocab_outermost"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [65, 1100])
def test_layouts_match_float32(device, V, dtype, layout):
    """Rows that start on 2-byte boundaries, padded rows, a class stride of 2 and the class axis outermost in
    memory, in a staged and in the streamed form: the gradient that reaches the underlying tensor."""
    rng = np.random.default_rng(V)
    H, N, R = 5, 3, 7
    ref = rng.integers(0, V, (R, N))
    ref[:3, 0] = (0, 64, V - 1)
    hyp = rng.integers(0, V, (H, N))
    x = hl.planted((H, N, V), hl.HALF_DTYPES[dtype], seed=V + 11, device=device)
    if layout == "offset":
        base = hl.lay_out(x, "offset")._base

        def view(b):
            return b[1:].view(H, N, V)

        assert view(base).data_ptr() % 4 == 2 and V % 2 == (1 if V == 65 else 0)
    elif layout == "padded":
        base = hl.lay_out(x, "padded")._base

        def view(b):
            return b[..., :V]

        assert view(base).stride(1) == V + 3
    elif layout == "every_other":
        base = torch.zeros((H, N, 2 * V), dtype=x.dtype, device=device)
        base[..., ::2] = x

        def view(b):
            return b[..., ::2]

        assert view(base).stride(2) == 2
    else:
        base = x.permute(2, 0, 1).contiguous()

        def view(b):
            return b.permute(1, 2, 0)

        assert view(base).stride(2) == H * N
    assert torch.equal(view(base), x) and (layout == "offset" or not view(base).is_contiguous())
    _compare(base, view, _tok(ref, device), _tok(hyp, device), "V={} {} {}".format(V, dtype, layout), seed=V)


# ---- 3. empty sets and an ignored class ----------------------------------------------------------------
@pytest.mark.parametrize("include_eos", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_sets_and_ignored_class(device, dtype, include_eos):
    """``ignore_index`` is a class (3) and hypotheses end early: rows with no target give loss 0 and gradient
    rows whose 16-bit patterns are all zero (+0, as the float32 route's cast gives).  The patterns are read
    under an upstream gradient of ones: a row's elements are ``g * 0 * softmax``, so under a NEGATIVE upstream
    ``g`` the float32 kernel writes -0 there and the half route, which has its bits, does too -- that case is
    covered by the bit comparison under the random upstream gradient, where the rows are asserted to be zeros
    of either sign."""
    import oracle

    rng = np.random.default_rng(24)
    V, eos, H, N, R = 7, 0, 8, 3, 6
    ref = rng.integers(0, V, (R, N))
    hyp = rng.integers(0, V, (H, N))
    w = torch.from_numpy(rng.uniform(0.5, 2, V).astype(np.float32)).to(device)
    tgt = oracle.optimal_completion(ref, hyp, padding=3, exclude_last=True, eos=eos, include_eos=include_eos)
    n_targets = torch.from_numpy((tgt != 3).sum(2))
    assert bool(((n_targets == 0).any(0) & (n_targets > 0).any(0)).all())
    x = hl.planted((H, N, V), hl.HALF_DTYPES[dtype], seed=24, device=device)
    ref, hyp = _tok(ref, device), _tok(hyp, device)
    kw = dict(eos=eos, include_eos=include_eos, ignore_index=3)
    la, ga, _, _ = _compare(x, _identity, ref, hyp, "empty {} {}".format(dtype, include_eos), weight=w, **kw)
    count = _rows_op(x, ref, hyp, weight=w, **kw)[1]
    assert count.dtype == torch.int32 and torch.equal(count.cpu().long(), n_targets.long())
    empty = (count == 0).cpu()
    assert empty.any() and not _bits(la).cpu()[empty].any()
    assert ga.dtype == x.dtype and not ga.cpu()[empty].any()
    leaf = x.detach().requires_grad_(True)
    _loss(leaf, ref, hyp, "none", weight=w, **kw).sum().backward()
    assert leaf.grad.dtype == x.dtype and not _bits(leaf.grad).cpu()[empty].any()
    assert _bits(leaf.grad).cpu()[~empty].any()


# ---- 4. -inf outside the sets --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [300, 1100])
def test_masked_vocabulary(device, V, dtype):
    """A third of each row's logits outside the set at -inf: finite loss and gradient with the float32 route's
    bits, gradient exactly 0 where the logit is -inf."""
    rng = np.random.default_rng(V)
    H, N, R = 6, 2, 8
    ref = rng.integers(0, V, (R, N))
    hyp = rng.integers(0, V, (H, N))
    M, _ = LR.oracle_multiplicity(ref, hyp, V)
    masked = torch.from_numpy((rng.random((H, N, V)) < 1 / 3) & (M.numpy() == 0))
    assert int(masked.view(H * N, V).sum(1).min()) > V // 4
    x = hl.planted((H, N, V), hl.HALF_DTYPES[dtype], seed=V + 13).masked_fill(masked, float("-inf")).to(device)
    la, ga, gf, _ = _compare(x, _identity, _tok(ref, device), _tok(hyp, device), "masked V={} {}".format(V, dtype), seed=V)
    assert torch.isfinite(la).all() and torch.isfinite(ga.float()).all() and torch.isfinite(gf).all()
    assert not ga.cpu()[masked].any() and float(ga.float().abs().max()) > 0


# ---- 5. bitmask words ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", [32, 33, 65])
def test_bitmask_words(device, R, dtype):
    """Class bitmasks of exactly one word, one class more, and three words: the reference tokens are distinct
    and the last prefix of utterance 0 has every one of them as a target."""
    rng = np.random.default_rng(R)
    V, H, N = 80, R, 2
    ref = np.stack([rng.permutation(V - 1)[:R] for _ in range(N)], 1)
    hyp = rng.integers(0, V, (H, N))
    hyp[:, 0] = V - 1
    x = hl.planted((H, N, V), hl.HALF_DTYPES[dtype], seed=R, device=device)
    ref, hyp = _tok(ref, device), _tok(hyp, device)
    _compare(x, _identity, ref, hyp, "R={} {}".format(R, dtype), seed=R)
    assert _rows_op(x, ref, hyp)[1][:, 0].tolist() == list(range(1, R + 1))


def test_wide_bitmask(device):
    """Both 64-word blocks of ``for_each_target`` in the streamed form: 2100 distinct reference tokens, a
    hypothesis of 2080 copies of a token outside them, so that prefix h has the h + 1 targets ref[0..h]."""
    rng = np.random.default_rng(2200)
    V, R, H = 2200, 2100, 2080
    ref = rng.permutation(V - 1)[:R].reshape(R, 1)
    hyp = np.full((H, 1), V - 1)
    g = torch.Generator().manual_seed(2200)
    x = (torch.randn((H, 1, V), generator=g) * 3.0).to(torch.bfloat16).to(device)
    w = torch.from_numpy(rng.uniform(0.5, 2, V).astype(np.float32)).to(device)
    ref, hyp = _tok(ref, device), _tok(hyp, device)
    _compare(x, _identity, ref, hyp, "wide bitmask", reductions=("none",), weight=w)
    assert _rows_op(x, ref, hyp, weight=w)[1][:, 0].tolist() == list(range(1, H + 1))


# ---- 6. independent of the float32 route ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [513, 1100])
def test_against_the_float64_set_form(device, V, dtype):
    """The half route held to the float64 set form on the logits as the type holds them, within the bound of
    tests/test_losses_gpu.py::test_hocd_input_types: LOSS_TOL for the loss; GRAD_TOL plus half a unit of the
    output type's rounding for the gradient."""
    from pydrobert_amd import functional as F

    rng = np.random.default_rng(V)
    H, N, R = 6, 3, 9
    ref = rng.integers(0, V, (R, N))
    ref[:3, 0] = (0, 512, 64)
    hyp = rng.integers(0, V, (H, N))
    dt = hl.HALF_DTYPES[dtype]
    x = hl.planted((H, N, V), dt, seed=V + 17, device=device).requires_grad_(True)
    w = rng.uniform(0.5, 2, V).astype(np.float32)
    M, _ = LR.oracle_multiplicity(ref, hyp, V)
    x64 = x.detach().cpu().double().requires_grad_(True)
    le, _ = LR.set_loss(x64, M, w)
    gw = torch.randn(le.shape, dtype=torch.double).float().double()
    (ge,) = torch.autograd.grad((le * gw).sum(), x64)
    la = F.hard_optimal_completion_distillation_loss(
        x, _tok(ref, device), _tok(hyp, device), weight=torch.from_numpy(w).to(device), reduction="none", warn=False
    )
    (ga,) = torch.autograd.grad((la * gw.float().to(device)).sum(), x)
    assert ga.dtype == dt and la.dtype == torch.float32
    ok, worst = LR.close(la, le, LR.LOSS_TOL)
    print("V={} {}: loss excess ratio {:.3g}".format(V, dtype, worst))
    assert ok, worst
    bound = LR.GRAD_TOL[1] + LR.GRAD_TOL[0] * ge.abs()
    bound = bound + 0.5 * float(torch.finfo(dt).eps) * (ge.abs() + bound)
    excess = float(((ga.cpu().double() - ge).abs() / bound).max())
    print("V={} {}: gradient excess ratio {:.3g}".format(V, dtype, excess))
    assert excess <= 1.0, excess


# ---- 7. the copies are gone ----------------------------------------------------------------------------
def _growth(fn):
    """Growth of max_memory_allocated across ``fn()`` (its outputs are kept alive until it is read)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return peak - base


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_float32_copy_of_the_logits(lib, device, dtype):
    """Peak memory of the forward and of the backward operator on half logits stays within 1 MiB (the
    allocator's rounding) of a fixed allowance -- the forward's small outputs and the mask workspace; the
    backward's gradient in the half type -- and each allowance is below the size of the float32 copy."""
    H, N, V, R = (hlo.NOCOPY[k] for k in ("H", "N", "V", "R"))
    dt = hl.HALF_DTYPES[dtype]
    g = torch.Generator().manual_seed(12)
    x = (torch.randn((H, N, V), generator=g) * 3.0).to(dt).to(device)
    ref = torch.randint(0, V, (R, N), generator=g).to(device)
    hyp = torch.randint(0, V, (H, N), generator=g).to(device)
    go = torch.randn((H, N), generator=g).to(device)
    copy_bytes = x.numel() * 4
    assert copy_bytes == 8_192_000
    _, _, bitmask, class_tokens = _rows_op(x, ref, hyp)
    allow = {
        "ocd_loss_rows": hlo.forward_allowance(lib, H, N, V, R),
        "ocd_loss_rows_backward": hlo.backward_allowance(H, N, V, x.element_size()),
    }
    calls = {
        "ocd_loss_rows": lambda: _rows_op(x, ref, hyp),
        "ocd_loss_rows_backward": lambda: torch.ops.pydrobert_amd.ocd_loss_rows_backward(
            x, bitmask, class_tokens, None, -2, False, go
        ),
    }
    for name, fn in calls.items():
        fn()  # (first call: anything the library or the allocator sets up once)
        grown = _growth(fn)
        print("{} {}: peak growth {} B, allowance {} B, float32 copy {} B".format(name, dtype, grown, allow[name], copy_bytes))
        assert allow[name] + hl.MIB < copy_bytes, name  # (not vacuous: the copy alone would break the bound)
        assert grown <= allow[name] + hl.MIB, (name, grown, allow[name])
    assert calls["ocd_loss_rows_backward"]().dtype == dt


# ---- 8. operator registration --------------------------------------------------------------------------
def test_opcheck_with_bfloat16_logits(device):
    """Schema, fake kernel and autograd registration of ``ocd_loss_rows`` hold for bfloat16 logits (the checks
    tests/test_jit_gpu.py runs on float32 ones, at its shape)."""
    from torch.library import opcheck

    T, N, V = 10, 4, 6
    g = torch.Generator().manual_seed(20)
    ref = torch.randint(0, V, (T, N), generator=g).to(device)
    hyp = torch.randint(0, V, (T, N), generator=g).to(device)
    logits = hl.planted((T, N, V), torch.bfloat16, seed=20, device=device).requires_grad_(True)
    opcheck(
        torch.ops.pydrobert_amd.ocd_loss_rows.default,
        (logits, ref, hyp, None, True, False, 1.0, 1.0, 1.0, None, -2, False),
        test_utils=("test_schema", "test_faketensor", "test_autograd_registration"),
    )
