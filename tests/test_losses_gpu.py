"""GPU: fused optimal-completion distillation loss and minimum-error-rate loss vs the oracle
and the golden vectors (forward and gradient)."""
import os

import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import modules as M

import _loss_ref as LR

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def test_hocd_random_vs_oracle_and_autograd(device):
    rng = np.random.default_rng(17)
    for it in range(30):
        N, R, H, V = int(rng.integers(1, 6)), int(rng.integers(1, 40)), int(rng.integers(1, 30)), int(rng.integers(3, 50))
        bf = bool(rng.integers(0, 2))
        eos = None if rng.random() < 0.4 else int(rng.integers(0, V))
        ref = rng.integers(0, V, (N, R) if bf else (R, N))
        hyp = rng.integers(0, V, (N, H) if bf else (H, N))
        logits = rng.normal(size=hyp.shape + (V,)).astype(np.float32)
        w = None if rng.random() < 0.5 else rng.uniform(0.5, 2, V).astype(np.float32)
        for red in ("mean", "sum", "none"):
            exp = oracle.hard_optimal_completion_distillation_loss(
                logits, ref, hyp, eos=eos, batch_first=bf, weight=w, reduction=red)
            x = T(logits, device).requires_grad_(True)
            act = F.hard_optimal_completion_distillation_loss(
                x, T(ref, device), T(hyp, device), eos=eos, batch_first=bf,
                weight=None if w is None else T(w, device), reduction=red, warn=False)
            assert act.shape == exp.shape
            assert np.allclose(act.detach().cpu().numpy(), exp, rtol=1e-5, atol=1e-6), (it, red)
            # gradient against torch autograd through cross_entropy on the oracle's targets
            opt = torch.from_numpy(oracle.optimal_completion(ref, hyp, eos=eos, batch_first=bf, padding=-2, exclude_last=True))
            xc = torch.from_numpy(logits).double().requires_grad_(True)
            C = opt.shape[-1]
            ce = torch.nn.functional.cross_entropy(
                xc.unsqueeze(2).expand(-1, -1, C, -1).reshape(-1, V), opt.flatten(),
                weight=None if w is None else torch.from_numpy(w).double(), ignore_index=-2, reduction="none",
            ).view_as(opt) if C else torch.zeros(opt.shape, dtype=torch.double)
            pad = opt == -2
            l = ce.masked_fill(pad, 0.0).sum(2) / (~pad).sum(2).clamp_min(1)
            gw = torch.randn(l.shape, dtype=torch.double)
            (ge,) = torch.autograd.grad((l * gw).sum(), xc, allow_unused=True)
            lo = F.hard_optimal_completion_distillation_loss(
                x, T(ref, device), T(hyp, device), eos=eos, batch_first=bf,
                weight=None if w is None else T(w, device), reduction="none", warn=False)
            (ga,) = torch.autograd.grad((lo * gw.float().to(device)).sum(), x)
            ge = torch.zeros_like(xc) if ge is None else ge
            assert torch.allclose(ga.cpu().double(), ge, rtol=1e-4, atol=1e-5), (it, (ga.cpu().double() - ge).abs().max())


def test_hocd_long_reference(device):
    """A reference beyond 2048 tokens: class bitmasks wider than 64 words through the loss."""
    rng = np.random.default_rng(23)
    N, R, H, V = 2, 2600, 21, 700
    ref = rng.integers(0, V, (R, N))
    hyp = rng.integers(0, V, (H, N))
    logits = rng.normal(size=(H, N, V)).astype(np.float32)
    exp = oracle.hard_optimal_completion_distillation_loss(logits, ref, hyp, reduction="none")
    x = T(logits, device).requires_grad_(True)
    act = F.hard_optimal_completion_distillation_loss(x, T(ref, device), T(hyp, device), reduction="none", warn=False)
    assert np.allclose(act.detach().cpu().numpy(), exp, rtol=1e-5, atol=1e-6)
    (g,) = torch.autograd.grad(act.sum(), x, retain_graph=True)
    assert torch.isfinite(g).all() and float(g.abs().sum()) > 0
    # the whole gradient, under a random upstream gradient, against the float64 set form
    Mx, _ = LR.oracle_multiplicity(ref, hyp, V)
    x64 = torch.from_numpy(logits).double().requires_grad_(True)
    le, _ = LR.set_loss(x64, Mx)
    gw = torch.randn(le.shape, dtype=torch.double)
    (ge,) = torch.autograd.grad((le * gw).sum(), x64)
    (ga,) = torch.autograd.grad((act * gw.float().to(device)).sum(), x)
    ok, worst = LR.close(ga, ge, LR.GRAD_TOL)
    assert ok, worst


def hocd_check(device, logits, ref, hyp, *, weight=None, M=None, oracle_reductions=True, seed=0, **kw):
    """The kernels' ``"none"`` loss and its gradient under a random upstream gradient against the float64
    set form (tests/_loss_ref.py) of the oracle's completion sets -- or of ``M`` where the caller has them
    in closed form -- and the ``"mean"`` / ``"sum"`` values against the oracle.  ``logits``: float32 numpy,
    ``hyp.shape + (V,)``; ``kw``: eos, include_eos, batch_first, ignore_index.  Returns what it compared."""
    V = logits.shape[-1]
    bf = kw.get("batch_first", False)
    if M is None:
        M, _ = LR.oracle_multiplicity(ref, hyp, V, kw.get("eos"), kw.get("include_eos", True), bf, kw.get("ignore_index", -2))
    x64 = torch.from_numpy(logits).double().requires_grad_(True)
    le, count = LR.set_loss(x64, M, weight)
    gw = torch.from_numpy(np.random.default_rng(seed).normal(size=tuple(le.shape)))
    (ge,) = torch.autograd.grad((le * gw).sum(), x64)
    wd = None if weight is None else T(weight, device)
    x = T(logits, device).requires_grad_(True)
    la = F.hard_optimal_completion_distillation_loss(x, T(ref, device), T(hyp, device), weight=wd, reduction="none", warn=False, **kw)
    (ga,) = torch.autograd.grad((la * gw.float().to(device)).sum(), x)
    ok, worst = LR.close(la, le, LR.loss_tol(V))
    assert ok, ("none", worst)
    ok, worst = LR.close(ga, ge, LR.GRAD_TOL)
    assert ok, ("gradient", worst)
    for red in ("mean", "sum"):
        if oracle_reductions:
            exp = oracle.hard_optimal_completion_distillation_loss(logits, ref, hyp, weight=weight, reduction=red, **kw)
        else:
            exp = LR.reduce(le, count, red, bf).detach()
        act = F.hard_optimal_completion_distillation_loss(x, T(ref, device), T(hyp, device), weight=wd, reduction=red, warn=False, **kw)
        ok, worst = LR.close(act, exp, LR.loss_tol(V))
        assert ok, (red, worst)
    return la.detach().cpu(), ga.cpu(), le.detach(), ge, count


def forced_tokens(V):
    """Both sides of every register-chunk (64) and staging (512, 1024) boundary of csrc/row_reduce.hpp."""
    return sorted({t for t in (0, 63, 64, 511, 512, 1023, 1024, V - 1) if t < V})


@pytest.mark.parametrize("batch_first", [False, True])
@pytest.mark.parametrize("V", [64, 65, 256, 512, 513, 1024, 1025, 2500])
def test_hocd_row_forms(device, V, batch_first):
    """Rows in 8 registers per lane (V <= 512), in 16 (<= 1024, staged in LDS up to here) and streamed
    (beyond), forward and backward, with the tokens on both sides of every chunk boundary as targets."""
    rng = np.random.default_rng(V)
    H, N, R = 9, 3, 11
    forced = forced_tokens(V)
    ref = rng.integers(0, V, (R, N))
    for n in range(N):  # the forced tokens lead the reference (in another order per utterance): prefix h of a
        ref[: len(forced), n] = np.roll(forced, n)  # hypothesis that matches nothing is completed by ref[0..h]
    hyp = rng.integers(0, V, (H, N))
    logits = rng.normal(size=(H, N, V)).astype(np.float32) * 3
    w = rng.uniform(0.5, 2, V).astype(np.float32)
    tgt = oracle.optimal_completion(ref, hyp, padding=-2, exclude_last=True)
    assert set(forced) <= set(tgt.flatten().tolist())
    if batch_first:
        ref, hyp, logits = ref.T.copy(), hyp.T.copy(), np.ascontiguousarray(logits.transpose(1, 0, 2))
    hocd_check(device, logits, ref, hyp, weight=w, batch_first=batch_first, seed=V)


@pytest.mark.parametrize("R", [32, 33, 64, 65])
def test_hocd_bitmask_words(device, R):
    """Class bitmasks of exactly one and two words and one class more: the reference tokens are distinct,
    so that the classes are R, and the last prefix of utterance 0 has every one of them as a target."""
    rng = np.random.default_rng(R)
    V, H, N = 80, R, 2
    ref = np.stack([rng.permutation(V - 1)[:R] for _ in range(N)], 1)
    hyp = rng.integers(0, V, (H, N))
    hyp[:, 0] = V - 1  # not in ref: the sets of utterance 0 are {ref[0..h]}
    logits = rng.normal(size=(H, N, V)).astype(np.float32)
    count = hocd_check(device, logits, ref, hyp, seed=R)[4]
    assert count[:, 0].tolist() == list(range(1, R + 1))


def test_hocd_wide_bitmask(device):
    """Both 64-word blocks of ``for_each_target``: 2100 distinct reference tokens, a hypothesis of 2080
    copies of a token outside them.  The completion set of prefix h is ``{ref[0..h]}`` (checked against the
    oracle at R = 70, H = 66 in tests/test_oracle_golden.py), so the multiplicities come from the closed
    form; the last row holds 51 classes of rank 2048 and above.  Loss and the full gradient."""
    rng = np.random.default_rng(2200)
    V, R, H = 2200, 2100, 2080
    ref = rng.permutation(V - 1)[:R].reshape(R, 1)
    hyp = np.full((H, 1), V - 1)
    logits = rng.normal(size=(H, 1, V)).astype(np.float32)
    w = rng.uniform(0.5, 2, V).astype(np.float32)
    M = LR.prefix_set_multiplicity(ref[:, 0], H, V)
    rank = np.searchsorted(np.sort(ref[:, 0]), ref[:H, 0])  # class index of each target of the last row
    assert int((rank >= 2048).sum()) == 51
    count = hocd_check(device, logits, ref, hyp, weight=w, M=M, oracle_reductions=False)[4]
    assert count[:, 0].tolist() == list(range(1, H + 1))


@pytest.mark.parametrize("include_eos", [True, False])
def test_hocd_empty_sets_and_ignored_class(device, include_eos):
    """``ignore_index`` is a class (3) and hypotheses end early: rows with no target give loss 0, gradient
    exactly 0, and stay out of the per-utterance denominator of ``"mean"``."""
    rng = np.random.default_rng(24)
    V, eos, H, N, R = 7, 0, 8, 3, 6
    ref = rng.integers(0, V, (R, N))
    hyp = rng.integers(0, V, (H, N))
    logits = rng.normal(size=(H, N, V)).astype(np.float32)
    w = rng.uniform(0.5, 2, V).astype(np.float32)
    kw = dict(eos=eos, include_eos=include_eos, ignore_index=3)
    tgt = oracle.optimal_completion(ref, hyp, padding=3, exclude_last=True, eos=eos, include_eos=include_eos)
    n_targets = (tgt != 3).sum(2)
    assert ((n_targets == 0).any(0) & (n_targets > 0).any(0)).all()
    la, ga, _, _, count = hocd_check(device, logits, ref, hyp, weight=w, **kw)
    assert np.array_equal(count.numpy(), n_targets)
    assert not la[count == 0].any() and not ga[count == 0].any()


@pytest.mark.parametrize("layout", ["every_other", "vocab_outermost"])
@pytest.mark.parametrize("V", [65, 1100])
def test_hocd_strided_logits(device, V, layout):
    """Logits whose class axis has stride 2, and stride H N (the class axis outermost in memory): the
    gradient that reaches the underlying tensor is the float64 one, scattered the same way."""
    rng = np.random.default_rng(V)
    H, N, R = 5, 3, 7
    ref = rng.integers(0, V, (R, N))
    ref[:3, 0] = (0, 64, V - 1)
    hyp = rng.integers(0, V, (H, N))
    base = rng.normal(size=(H, N, 2 * V) if layout == "every_other" else (V, H, N)).astype(np.float32) * 3
    view = (lambda b: b[..., ::2]) if layout == "every_other" else (lambda b: b.permute(1, 2, 0))
    M, _ = LR.oracle_multiplicity(ref, hyp, V)
    b64 = torch.from_numpy(base).double().requires_grad_(True)
    le, _ = LR.set_loss(view(b64), M)
    gw = torch.randn(le.shape, dtype=torch.double)
    (le * gw).sum().backward()
    b = T(base, device).requires_grad_(True)
    x = view(b)
    assert not x.is_contiguous() and x.stride(2) == (2 if layout == "every_other" else H * N)
    la = F.hard_optimal_completion_distillation_loss(x, T(ref, device), T(hyp, device), reduction="none", warn=False)
    (la * gw.float().to(device)).sum().backward()
    ok, worst = LR.close(la, le, LR.loss_tol(V))
    assert ok, worst
    ok, worst = LR.close(b.grad, b64.grad, LR.GRAD_TOL)
    assert ok, worst
    for red in ("mean", "sum"):
        exp = oracle.hard_optimal_completion_distillation_loss(view(torch.from_numpy(base)).numpy(), ref, hyp, reduction=red)
        act = F.hard_optimal_completion_distillation_loss(x, T(ref, device), T(hyp, device), reduction=red, warn=False)
        ok, worst = LR.close(act, exp, LR.loss_tol(V))
        assert ok, (red, worst)


@pytest.mark.parametrize("V", [300, 1100])
def test_hocd_extreme_logits(device, V):
    """A masked vocabulary (a third of each row's logits outside the set at -inf): finite loss and gradient,
    gradient exactly 0 where the logit is -inf.  Whole rows shifted by +-80: the same loss."""
    rng = np.random.default_rng(V)
    H, N, R = 6, 2, 8
    ref = rng.integers(0, V, (R, N))
    hyp = rng.integers(0, V, (H, N))
    logits = rng.normal(size=(H, N, V)).astype(np.float32) * 3
    M, _ = LR.oracle_multiplicity(ref, hyp, V)
    masked = (rng.random((H, N, V)) < 1 / 3) & (M.numpy() == 0)
    x_masked = np.where(masked, -np.inf, logits).astype(np.float32)
    with np.errstate(all="ignore"):
        la, ga, le, ge, _ = hocd_check(device, x_masked, ref, hyp, seed=V)
    assert torch.isfinite(la).all() and torch.isfinite(ga).all() and torch.isfinite(le).all() and torch.isfinite(ge).all()
    assert masked.reshape(H * N, V).sum(1).min() > V // 4 and not ga[torch.from_numpy(masked)].any()
    shift = np.where(rng.random((H, N, 1)) < 0.5, np.float32(80), np.float32(-80))
    shift[0, 0], shift[0, 1] = 80, -80
    l0 = hocd_check(device, logits, ref, hyp, seed=V)[2]
    la = hocd_check(device, logits + shift, ref, hyp, seed=V)[0]  # (against the shifted, rounded inputs)
    ok, worst = LR.close(la, l0, LR.loss_tol(V))
    assert ok, worst


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_hocd_input_types(device, dtype):
    """float16 / bfloat16 / float64 logits at V = 513: the kernels compute in float32; the gradient comes
    back in the type of the logits, within the float32 bound plus -- for the 16-bit types -- half a unit of
    the output's rounding (the bound form of tests/test_rl_comb_gpu.py), of the float64 reference evaluated
    on the logits as that type holds them."""
    rng = np.random.default_rng(513)
    V, H, N, R = 513, 6, 3, 9
    ref = rng.integers(0, V, (R, N))
    ref[:3, 0] = (0, 512, 64)
    hyp = rng.integers(0, V, (H, N))
    x = (torch.from_numpy(rng.normal(size=(H, N, V))) * 3).to(dtype).to(device).requires_grad_(True)
    w = rng.uniform(0.5, 2, V).astype(np.float32)
    M, _ = LR.oracle_multiplicity(ref, hyp, V)
    x64 = x.detach().cpu().double().requires_grad_(True)
    le, _ = LR.set_loss(x64, M, w)
    gw = torch.randn(le.shape, dtype=torch.double).float().double()
    (ge,) = torch.autograd.grad((le * gw).sum(), x64)
    la = F.hard_optimal_completion_distillation_loss(x, T(ref, device), T(hyp, device), weight=T(w, device), reduction="none", warn=False)
    (ga,) = torch.autograd.grad((la * gw.to(la.dtype).to(device)).sum(), x)
    assert ga.dtype == dtype
    ok, worst = LR.close(la, le, LR.loss_tol(V))
    assert ok, worst
    bound = LR.GRAD_TOL[1] + LR.GRAD_TOL[0] * ge.abs()
    if dtype != torch.float64:
        bound = bound + 0.5 * float(torch.finfo(dtype).eps) * (ge.abs() + bound)
    excess = ((ga.cpu().double() - ge).abs() / bound).max()
    assert float(excess) <= 1.0, float(excess)


@pytest.mark.parametrize("V", [98304, 131072, 262144])
def test_hocd_large_vocabulary(device, V):
    """Vocabularies up to and beyond 98304 classes, where the backward pass's LDS membership map used to
    refuse the launch after the forward pass had run: forward and gradient."""
    rng = np.random.default_rng(V)
    H, N, R = 1, 2, 3
    ref = rng.integers(0, V, (R, N))
    ref[0] = (V - 1, 98304 if V > 98304 else 0)
    hyp = rng.integers(0, V, (H, N))
    logits = rng.normal(size=(H, N, V)).astype(np.float32) * 3
    ge = hocd_check(device, logits, ref, hyp, seed=V)[3]
    assert int((ge.abs() > 100 * LR.GRAD_TOL[1]).sum()) > 100  # the comparison is not all absolute tolerance


def test_hocd_vocabulary_bound_names_V(device):
    """The one bound on V (32-bit row indices), raised before anything is launched or allocated."""
    V = 2**31
    logits = torch.zeros(1, device=device).expand(1, 1, V)
    tok = torch.zeros(1, 1, dtype=torch.long, device=device)
    with pytest.raises(RuntimeError, match="V = {} classes".format(V)):
        F.hard_optimal_completion_distillation_loss(logits, tok, tok, warn=False)


def test_loss_goldens(device):
    g = np.load(os.path.join(G, "losses.npz"))
    ref, hyp, w = T(g["ref"], device), T(g["hyp"], device), T(g["weight"], device)
    for tag, kw in {"a": dict(eos=0), "b": dict(eos=None, weight=w), "c": dict(eos=0, include_eos=False, weight=w)}.items():
        for red in ("mean", "sum", "none"):
            x = T(g["logits"], device).requires_grad_(True)
            mod = M.HardOptimalCompletionDistillationLoss(reduction=red, ignore_index=-2, **kw).to(device)
            loss = mod(x, ref, hyp, warn=False)
            (gr,) = torch.autograd.grad(loss.sum(), x)
            assert np.allclose(loss.detach().cpu().numpy(), g["hocd_{}_{}".format(tag, red)], rtol=1e-5, atol=1e-6)
            assert np.allclose(gr.cpu().numpy(), g["hocd_{}_{}_grad".format(tag, red)], rtol=1e-4, atol=1e-6)
    lp = T(g["mer_lp"], device).requires_grad_(True)
    for red in ("mean", "none"):
        for sub_avg in (True, False):
            loss = M.MinimumErrorRateLoss(eos=0, sub_avg=sub_avg, reduction=red)(lp, ref, T(g["mer_hyp"], device), warn=False)
            assert np.allclose(loss.detach().cpu().numpy(), g["mer_{}_{}".format(red, int(sub_avg))], rtol=1e-5, atol=1e-7)
    (gl,) = torch.autograd.grad(loss.sum(), lp)
    assert torch.isfinite(gl).all()


def test_loss_errors(device):
    logits = torch.zeros(3, 2, 4, device=device)
    tok = torch.zeros(3, 2, dtype=torch.long, device=device)
    with pytest.raises(RuntimeError, match="3 dimensional"):
        F.hard_optimal_completion_distillation_loss(logits[0], tok, tok)
    with pytest.raises(RuntimeError, match="must match hyp shape"):
        F.hard_optimal_completion_distillation_loss(logits, tok, tok[:2])
    with pytest.raises(RuntimeError, match="must be a class idx"):
        F.hard_optimal_completion_distillation_loss(logits, tok, tok, eos=9)
    with pytest.raises(RuntimeError, match="not class indices"):
        F.hard_optimal_completion_distillation_loss(logits, tok + 7, tok)
    with pytest.raises(RuntimeError, match="at least two samples"):
        F.minimum_error_rate_loss(torch.zeros(2, 1, device=device), tok, tok.unsqueeze(-1))
    with pytest.raises(ValueError):
        M.MinimumErrorRateLoss(reduction="avg")
