"""GPU: random_walk_advance and RandomWalk on the HIP kernels (csrc/random_walk.hip).

The sampling rule is restated here in numpy float64: for a row x and a uniform u, with w = exp(x - max x)
and Z = sum w, the token is the smallest v with w_v > 0 whose running prefix sum of w exceeds u Z, else the
largest v with w_v > 0.  Uniforms are placed well inside a token's interval so that float32 rounding cannot
move the draw."""
import math
from typing import Dict, Tuple

import numpy as np
import pytest
import torch

from pydrobert_amd import functional as F
from pydrobert_amd import modules as M
from pydrobert_amd import switches
from pydrobert_amd._lm import SequentialLanguageModel

from _lm_fixtures import random_dicts
from _toy_lm import CounterLM, ScriptableBigramLM
from _walk_plan import _choose, rule, u_inside  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rows(rng, N, V):
    """Rows of every kind: plain, unnormalised, with -inf entries, one-hot."""
    x = rng.normal(size=(N, V)) * 2.0
    kind = np.arange(N) % 4
    x[kind == 1] += 40.0
    holes = (rng.random((N, V)) < 0.4) & (kind == 2)[:, None]
    holes[holes.all(1), 0] = False
    x[holes] = -np.inf
    for n in np.nonzero(kind == 3)[0]:
        x[n] = -np.inf
        x[n, rng.integers(V)] = 0.0
    return x.astype(np.float32)


def _expected_y(y_prev, lens, tok):
    S, N = y_prev.shape
    if S == 0:
        return tok[None]
    if lens is None or lens.max() >= S:
        y = np.concatenate([y_prev, tok[None]], 0)
    else:
        y = y_prev.copy()
    if lens is not None:
        y[lens, np.arange(N)] = tok
    return y


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000, 5000])
def test_advance_is_token_exact(V):
    rng = np.random.default_rng(V)
    N = 512 if V == 5000 else 4096
    x = _rows(rng, N, V)
    tok, u = _choose(rng, x)
    for n in range(0, N, 97):
        assert rule(x[n], u[n]) == tok[n]
    lpp = torch.from_numpy(rng.normal(size=N).astype(np.float32)).to(DEV)
    S = 5
    y_prev = rng.integers(0, max(V, 2), (S, N))
    for layout in ("contiguous", "transposed"):
        lpt = torch.from_numpy(x).to(DEV)
        if layout == "transposed":
            lpt = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV).t()
            assert V == 1 or not lpt.is_contiguous()
        cases = [(0, None), (S, None), (S, rng.integers(0, S + 1, N)), (S, rng.integers(0, S, N))]
        for s, lens in cases:
            yp = torch.from_numpy(y_prev[:s]).to(DEV)
            ln = None if lens is None else torch.from_numpy(lens).to(DEV)
            y, lp = torch.ops.pydrobert_amd.random_walk_advance(lpt, torch.from_numpy(u).to(DEV), lpp, yp, ln)
            exp = _expected_y(y_prev[:s], None if lens is None else lens, tok)
            assert y.shape == exp.shape, (s, lens is None)
            assert np.array_equal(y.cpu().numpy(), exp)
            t = torch.from_numpy(tok).to(DEV).unsqueeze(1)
            assert torch.equal(lp, lpp + lpt.gather(1, t).squeeze(1))


@pytest.mark.parametrize("V", [1, 64, 65, 5000])
def test_advance_ends_of_the_unit_interval(V):
    """u = 0 draws the first token with mass, u = 1 - 2^-24 the last (a row whose last token with mass is
    dominant, so that the rounding of Z cannot matter)."""
    rng = np.random.default_rng(3 + V)
    N = 256
    x = _rows(rng, N, V)
    first = np.array([np.nonzero(np.isfinite(r))[0][0] for r in x])
    last = np.array([np.nonzero(np.isfinite(r))[0][-1] for r in x])
    x[np.arange(N), last] = x.max(1) + 8.0
    lpt = torch.from_numpy(x).to(DEV)
    z = torch.zeros(N, device=DEV)
    y0 = torch.empty((0, N), dtype=torch.long, device=DEV)
    y, _ = torch.ops.pydrobert_amd.random_walk_advance(lpt, z, z, y0, None)
    assert np.array_equal(y[0].cpu().numpy(), first)
    y, _ = torch.ops.pydrobert_amd.random_walk_advance(lpt, z + (1.0 - 2.0**-24), z, y0, None)
    assert np.array_equal(y[0].cpu().numpy(), last)
    for n in range(N):
        assert rule(x[n], 0.0) == first[n] and rule(x[n], 1.0 - 2.0**-24) == last[n]


@pytest.mark.parametrize("bad", ["-inf", "nan", "+inf"])
def test_rows_without_mass_raise(bad):
    N, V = 8, 100
    x = torch.randn(N, V, device=DEV)
    if bad == "-inf":
        x[3] = -math.inf
    else:
        x[3, 17] = float(bad)
    z = torch.zeros(N, device=DEV)
    y0 = torch.empty((0, N), dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):
        torch.ops.pydrobert_amd.random_walk_advance(x, torch.rand(N, device=DEV), z, y0, None)
    # ... and the device is fine afterwards
    y, _ = torch.ops.pydrobert_amd.random_walk_advance(x[:3], torch.rand(3, device=DEV), z[:3], y0[:, :3], None)
    assert y.shape == (1, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16])
def test_advance_gradient_and_dtypes(dtype):
    N, V = 64, 300
    gen = torch.Generator(DEV).manual_seed(2)
    lpt = torch.randn((N, V), device=DEV, generator=gen).log_softmax(-1).to(dtype).requires_grad_(True)
    lpp = torch.randn((N,), device=DEV, generator=gen).to(dtype).requires_grad_(True)
    u = torch.rand((N,), device=DEV, generator=gen)
    y_prev = torch.randint(0, V, (4, N), device=DEV, generator=gen)
    lens = torch.randint(0, 4, (N,), device=DEV, generator=gen)
    y, lp = torch.ops.pydrobert_amd.random_walk_advance(lpt, u, lpp, y_prev, lens)
    assert lp.dtype == (lpp + lpt[:, 0]).dtype and y.dtype == torch.long and y.shape == (4, N)
    tok = y.gather(0, lens.unsqueeze(0)).squeeze(0)
    exp = lpp.float() + lpt.float().gather(1, tok.unsqueeze(1)).squeeze(1)
    tol = {torch.float16: 1e-2, torch.bfloat16: 5e-2}.get(dtype, 1e-5)
    assert torch.allclose(lp.float(), exp, atol=tol, rtol=tol)
    g = torch.randn((N,), device=DEV, generator=gen)
    ga = torch.autograd.grad((lp.float() * g).sum(), (lpt, lpp))
    ref = lpp + lpt.gather(1, tok.unsqueeze(1)).squeeze(1)
    ge = torch.autograd.grad((ref.float() * g).sum(), (lpt, lpp))
    for a, e in zip(ga, ge):
        assert a.dtype == e.dtype and torch.equal(a, e)


def test_advance_distribution_chi_square():
    torch.manual_seed(11)
    V, D = 50, 1 << 16
    row = torch.randn(V, device=DEV) * 1.5
    row[7] = -math.inf
    torch.manual_seed(12)
    y, lp = F.random_walk_advance(row.expand(D, V), torch.zeros(D, device=DEV),
                                  torch.empty((0, D), dtype=torch.long, device=DEV))  # fmt: skip
    counts = torch.bincount(y[0], minlength=V).double().cpu()
    p = row.double().softmax(0).cpu()
    assert counts[7] == 0
    keep = p > 0
    chi2 = float(((counts[keep] - D * p[keep]) ** 2 / (D * p[keep])).sum())
    assert chi2 < 90.0, chi2  # (48 degrees of freedom: the 99.9th percentile is 84)
    assert torch.equal(lp, row[y[0]])
    # the uniforms: one torch.rand((N,)) on the device per call
    torch.manual_seed(12)
    u = torch.rand(D, device=DEV)
    y2, _ = torch.ops.pydrobert_amd.random_walk_advance(row.expand(D, V), u, torch.zeros(D, device=DEV), y[:0], None)
    assert torch.equal(y, y2)


def _rng_after(seed, N, T, max_iters):
    """The device generator's state after a walk of T iterations: one torch.rand((C, N)) per chunk begun
    (C = 64, doubling up to 4096, cut off at max_iters)."""
    torch.manual_seed(seed)
    t, C = 0, 64
    while t < T:
        c = min(C, max_iters - t)
        torch.rand((c, N), device=DEV)
        t, C = t + c, min(2 * C, 4096)
    return torch.cuda.get_rng_state(DEV)


def _bigram_lm(V, seed, order=2):
    rng = np.random.default_rng(seed)
    return M.LookupLanguageModel(V, V, random_dicts(rng, V, order, 0.6, sos=V)).to(DEV)


def _model_lp(lm, y, lens):
    """Sum along each path of the model's log-softmax (the reference's per-iteration calls)."""
    T, N = y.shape
    total = torch.zeros(N, dtype=torch.float64, device=DEV)
    for t in range(T):
        lp_t, _ = lm.calc_idx_log_probs(y[:t], dict(), torch.tensor(t, device=DEV))
        step = lp_t.double().log_softmax(-1).gather(1, y[t].unsqueeze(1)).squeeze(1)
        total += torch.where(t < lens, step, torch.zeros_like(step))
    return total


@pytest.mark.parametrize("table", [1, 0])
def test_walk_frequencies_follow_the_model(table):
    V, N = 8, 16384
    lm = _bigram_lm(V, 4)
    walk = M.RandomWalk(lm, eos=0).to(DEV)
    torch.manual_seed(12)
    with switches.override(PDT_WALK_TABLE=table):
        y, lens, lp = walk(None, N, 12)
    first, _ = lm.calc_idx_log_probs(y[:0], dict(), torch.tensor(0, device=DEV))
    p0 = first[0].double().softmax(0).cpu()
    f0 = torch.bincount(y[0], minlength=V).double().cpu() / N
    assert (f0 - p0).abs().max() < 0.015
    # transitions a -> b out of live positions
    a, b = y[:-1], y[1:]
    live = (torch.arange(1, y.size(0), device=DEV).unsqueeze(1) < lens.unsqueeze(0)).flatten()
    pairs = (a.flatten() * V + b.flatten())[live]
    counts = torch.bincount(pairs, minlength=V * V).view(V, V).double().cpu()
    for c in range(1, V):
        if counts[c].sum() < 3000:
            continue
        p, _ = lm.calc_idx_log_probs(torch.full((1, 1), c, device=DEV), dict(), torch.tensor(1, device=DEV))
        exp = p[0].double().softmax(0).cpu()
        assert (counts[c] / counts[c].sum() - exp).abs().max() < 0.03, c
    assert (_model_lp(lm, y, lens) - lp.double()).abs().max() < 1e-5


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("eos", [None, 3])
def test_table_and_per_iteration_routes_agree(order, eos):
    V = 40 if order == 2 else 12
    lm = _bigram_lm(V, 5 + order, order)
    walk = M.RandomWalk(lm, eos=eos).to(DEV)
    for max_iters in [0, 1, 63, 64, 65, 300, None]:
        if max_iters is None and eos is None:
            continue
        out = []
        for table in (1, 0):
            torch.manual_seed(20)
            with switches.override(PDT_WALK_TABLE=table):
                out.append(walk(None, 96, max_iters) + (torch.cuda.get_rng_state(),))
        for a, b in zip(*out):
            assert a.dtype == b.dtype and torch.equal(a, b), max_iters
        y, lens, _, _ = out[0]
        if eos is not None and y.size(0):
            T = int(lens.max())
            assert y.size(0) == (T if max_iters is None else min(T, max_iters))
            rows = torch.arange(y.size(0), device=DEV).unsqueeze(1)
            assert bool((y[rows >= lens.unsqueeze(0)] == eos).all())
    torch.manual_seed(21)
    exp = walk(None, 32, 80)
    scripted = torch.jit.script(walk)
    torch.manual_seed(21)
    act = scripted(None, 32, 80)
    for a, b in zip(exp, act):
        assert torch.equal(a, b)


class _SpinningLM(SequentialLanguageModel):
    """Deterministic: the next token is the previous one plus one (mod V), starting after prev["init"]."""

    def calc_idx_log_probs(
        self, hist: torch.Tensor, prev: Dict[str, torch.Tensor], idx: torch.Tensor
    ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        last = prev["init"][0] if int(idx) == 0 else hist[int(idx) - 1]
        nxt = (last + 1) % self.vocab_size
        return torch.nn.functional.one_hot(nxt, self.vocab_size).float().log() - 1.0, prev


def test_reference_behaviour_batch_is_per_row():
    N, V = 64, 12
    walk = M.RandomWalk(_SpinningLM(V), eos=V - 1).to(DEV)
    start = torch.randint(0, V, (1, N), device=DEV)
    start[0, 0] = V - 2
    torch.manual_seed(15)
    y, lens, lp = walk({"init": start}, N)
    assert torch.equal(torch.cuda.get_rng_state(DEV), _rng_after(15, N, y.size(0), 1 << 30))
    assert y.shape[1:] == lens.shape == lp.shape == (N,)
    assert int(lens[0]) == 1 and bool((lp == 0).all())
    for n in range(0, N, 5):
        L = int(lens[n])
        assert L == (V - 2 - int(start[0, n])) % V + 1
        assert bool((y[L - 1 :, n] == V - 1).all())
        yn, ln, lpn = walk({"init": start[:, n : n + 1]})
        assert yn.shape == (L,) and ln.shape == lpn.shape == () and int(ln) == L and float(lpn) == 0.0
        assert torch.equal(yn, y[:L, n])


class _StationaryLM(SequentialLanguageModel):
    def __init__(self, V):
        super().__init__(V)
        self.logits = torch.nn.Parameter(torch.randn(V, V))

    def calc_idx_log_probs(self, hist, prev, idx):
        last = hist.new_zeros(hist.size(1)) if int(idx) == 0 else hist[int(idx) - 1]
        return self.logits.index_select(0, last), prev


def test_reference_behaviour_stationary_walk_with_gradients():
    torch.manual_seed(13)
    V, N, T = 4, 256, 300
    lm = _StationaryLM(V).to(DEV)
    P = lm.logits.detach().double().softmax(-1)
    pi = torch.linalg.matrix_power(P, 256)[0]
    y, lens, lp = M.RandomWalk(lm).to(DEV)(None, N, T)
    assert y.shape == (T, N) and bool((lens == T).all())
    state = torch.cuda.get_rng_state(DEV)
    assert torch.equal(state, _rng_after(13, N, T, T))
    assert abs(float(y[30:].double().mean()) - float((pi * torch.arange(V, device=DEV)).sum())) < 0.02
    prev = torch.cat([torch.zeros_like(y[:1]), y[:-1]])
    exp = lm.logits.log_softmax(-1)[prev].gather(2, y.unsqueeze(2)).squeeze(2).sum(0)
    assert torch.allclose(lp, exp, rtol=1e-4, atol=1e-3)
    g_act = torch.autograd.grad(lp.sum(), lm.logits)[0]
    g_exp = torch.autograd.grad(exp.sum(), lm.logits)[0]
    assert torch.allclose(g_act, g_exp, rtol=1e-4, atol=1e-4)


def test_reference_behaviour_squeeze_zero_iterations_and_no_eos():
    lm = ScriptableBigramLM(torch.randn(6, 5, device=DEV).log_softmax(-1))
    torch.manual_seed(16)
    y, lens, lp = M.RandomWalk(lm, eos=0).to(DEV)(None, None, 7)
    assert y.dim() == 1 and lens.shape == lp.shape == () and y.size(0) == int(lens) <= 7
    assert torch.equal(torch.cuda.get_rng_state(DEV), _rng_after(16, 1, y.size(0), 7))
    y, lens, lp = M.RandomWalk(lm, eos=0).to(DEV)(None, 9, 0)
    assert y.shape == (0, 9) and bool((lens == 0).all()) and bool((lp == 0).all())
    y, lens, lp = M.RandomWalk(lm).to(DEV)(None, 9, 11)
    assert y.shape == (11, 9) and bool((lens == 11).all())
    with pytest.raises(RuntimeError):
        M.RandomWalk(lm).to(DEV)(None, 9)


def test_model_is_called_as_often_as_under_the_reference():
    V, N = 6, 200
    table = torch.randn(V + 1, V, device=DEV)
    table[:, 2] += 1.5
    lm = CounterLM(table)
    calls = []
    inner = lm.calc_idx_log_probs
    lm.calc_idx_log_probs = lambda h, p, i: (calls.append(int(i)), inner(h, p, i))[1]
    torch.manual_seed(14)
    y, lens, lp = M.RandomWalk(lm, eos=2).to(DEV)(None, N)
    T = int(lens.max())
    assert y.size(0) == T and calls == list(range(T))
    assert torch.equal(torch.cuda.get_rng_state(DEV), _rng_after(14, N, T, 1 << 30))


def test_unbounded_walk_memory_follows_the_iterations_run():
    lm = _bigram_lm(30, 9)
    walk = M.RandomWalk(lm, eos=1).to(DEV)
    for table in (1, 0):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        with switches.override(PDT_WALK_TABLE=table):
            y, lens, lp = walk(None, 1000)
        assert y.size(0) == int(lens.max())
        assert torch.cuda.max_memory_allocated(DEV) - base < (64 << 20)
