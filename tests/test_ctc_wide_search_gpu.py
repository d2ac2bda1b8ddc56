"""GPU: the CTC prefix search for beams of 33 to 128 prefixes in one launch (csrc/ctc_search_wide.hip),
through ``F.ctc_prefix_search``, ``torch.ops.pydrobert_amd.ctc_prefix_search``, ``M.CTCPrefixSearch`` and
the C ABI, against the oracle.

Near ties.  The oracle's own beam order changes under a few-ulp change of the softmax for a few
utterances (two candidates of the 33rd .. 128th rank whose masses agree to the last bits).  Such an
utterance is found ON THE CPU -- the oracle is run on the logits times (1 + u * 4e-7), u ~ U(-1, 1), three
times, and an utterance whose y or y_lens differ in any run is marked -- and is left out of the exact
comparison only: it must still hold no NaN, and its finite probabilities, sorted, must be within 1e-4
relative of the oracle's.  The number of marked utterances is capped: at most 1 in a case of up to 5
utterances, 6 of 300, and 1 % of all of them (checked on the CPU with the committed oracle: 13 of 1884).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import _cabi
from pydrobert_amd import functional as F
from pydrobert_amd import modules as M

pytestmark = pytest.mark.gpu
RTOL = 1e-5
SCALE = 8.0  # keeps every beam mass a normal float32 at these depths
CASES = [(40, 33), (64, 64), (80, 65), (150, 100), (300, 128), (127, 128)]
SHAPES = [(1, 2), (9, 3), (33, 4), (70, 5), (3, 300)]


def _peaky_logits(rng, T, N, V, scale=6.0):
    lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
    peak = rng.integers(0, V + 1, (T, N))
    np.put_along_axis(lg, peak[..., None], np.take_along_axis(lg, peak[..., None], 2) + scale, 2)
    return lg


def _near_tied(lg, K, lens, exp):
    """(N,) bool: utterances whose oracle beam changes under a few-ulp change of the logits."""
    marked = np.zeros(lg.shape[1], bool)
    for seed in (0, 1, 2):
        u = np.random.default_rng(seed).uniform(-1.0, 1.0, lg.shape)
        y, yl, _ = oracle.ctc_prefix_search((lg * (1.0 + u * 4e-7)).astype(np.float32), K, lens)
        marked |= (y != exp[0]).any((0, 2)) | (yl != exp[1]).any(1)
    return marked


def _check_search(act, exp, what, marked=None):
    y, yl, yp = (x.cpu().numpy() for x in act)
    ey, eyl, eyp = exp
    assert y.shape == ey.shape and yl.shape == eyl.shape and yp.shape == eyp.shape, what
    assert not np.isnan(yp).any(), what
    keep = np.ones(yp.shape[0], bool) if marked is None else ~marked
    for n in np.flatnonzero(~keep):  # near-tied: the same masses, possibly in another order
        a, e = np.sort(yp[n][np.isfinite(yp[n])]), np.sort(eyp[n][np.isfinite(eyp[n])])
        assert a.shape == e.shape and np.allclose(a, e, rtol=1e-4, atol=0.0), (what, n)
    y, yl, yp, ey, eyl, eyp = y[:, keep], yl[keep], yp[keep], ey[:, keep], eyl[keep], eyp[keep]
    fin = np.isfinite(eyp)
    assert np.array_equal(np.isfinite(yp), fin), what
    assert np.array_equal(yl[fin], eyl[fin]), (what, np.argwhere(yl != eyl)[:5])
    assert np.array_equal(y, ey), (what, np.argwhere(y != ey)[:5])
    assert np.allclose(yp[fin], eyp[fin], rtol=RTOL, atol=0.0), (what, np.abs(yp[fin] - eyp[fin]).max())


@functools.lru_cache(maxsize=None)
def _case(V, K):
    """The inputs of one width, their oracle results and their near-tied utterances: computed once."""
    rng = np.random.default_rng(7000 + V + K)
    out = []
    for it, (T, N) in enumerate(SHAPES):
        lg = _peaky_logits(rng, T, N, V, scale=SCALE)
        lens = None if it % 2 == 0 else rng.integers(0, T + 1, N)
        exp = oracle.ctc_prefix_search(lg, K, lens)
        marked = _near_tied(lg, K, lens, exp)
        for a in (lg, exp[0], exp[1], exp[2], marked) + (() if lens is None else (lens,)):
            a.setflags(write=False)
        out.append((lg, lens, exp, marked))
    return out


def _dev(a, device):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(device)


# ---- 1. against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", CASES)
def test_wide_search_against_the_oracle(device, V, K):
    for it, ((T, N), (lg, lens, exp, marked)) in enumerate(zip(SHAPES, _case(V, K))):
        assert marked.sum() <= (1 if N <= 5 else 6), (V, K, T, N, int(marked.sum()))
        tl, tt = _dev(lg, device), _dev(lens, device)
        _check_search(F.ctc_prefix_search(tl, K, tt), exp, (V, K, T, N), marked)
        _check_search(torch.ops.pydrobert_amd.ctc_prefix_search(tl, K, tt), exp, (V, K, T, N, "op"), marked)
        if it == 1:
            _check_search(M.CTCPrefixSearch(K)(tl, tt), exp, (V, K, T, N, "module"), marked)


def test_near_tied_utterances_are_few():
    total = sum(lg.shape[1] for V, K in CASES for lg, _, _, _ in _case(V, K))
    marked = sum(int(m.sum()) for V, K in CASES for _, _, _, m in _case(V, K))
    assert total == 6 * 314 and marked <= total // 100, (marked, total)


# ---- 2. the widths the op refused ------------------------------------------------------------------
def test_op_and_scripted_function_take_width_64(device):
    lg, lens, exp, marked = _case(64, 64)[1]
    tl, tt = _dev(lg, device), _dev(lens, device)
    _check_search(torch.ops.pydrobert_amd.ctc_prefix_search(tl, 64, tt), exp, "op", marked)

    def search(x: torch.Tensor, n: torch.Tensor):
        return F.ctc_prefix_search(x, 64, n)

    _check_search(torch.jit.script(search)(tl, tt), exp, "scripted", marked)
    plain = oracle.ctc_prefix_search(lg, 64)
    mk = _near_tied(lg, 64, None, plain)
    assert mk.sum() <= 1
    _check_search(torch.ops.pydrobert_amd.ctc_prefix_search(tl, 64, None), plain, "op, no lens", mk)

    def search_all(x: torch.Tensor):
        return F.ctc_prefix_search(x, 64)

    _check_search(torch.jit.script(search_all)(tl), plain, "scripted, no lens", mk)


# ---- 3. the same answers as the narrow kernels ------------------------------------------------------
def _wide_cabi(tl, tt, K):
    T, N, V = tl.shape[0], tl.shape[1], tl.shape[2] - 1
    S = T if tt is None else max(0, min(T, int(tt.max().item())))
    L = _cabi.lib()
    device = tl.device
    y = torch.empty((S, N, K), device=device, dtype=torch.long)
    yl = torch.empty((N, K), device=device, dtype=torch.long)
    yp = torch.empty((N, K), device=device, dtype=torch.float)
    ws = torch.empty((int(L.pdt_ctc_prefix_search_wide_workspace_bytes(T, N, V, K)),), device=device, dtype=torch.uint8)
    rc = L.pdt_ctc_prefix_search_wide(
        _cabi.ptr(tl), T, N, V, tl.stride(0), tl.stride(1), tl.stride(2), _cabi.ptr(tt), K, S,
        _cabi.ptr(y), _cabi.ptr(yl), _cabi.ptr(yp), _cabi.ptr(ws), _cabi.stream_ptr(device),
    )  # fmt: skip
    _cabi.check(rc, "pdt_ctc_prefix_search_wide")
    torch.cuda.synchronize(device)
    return y, yl, yp


@pytest.mark.parametrize("K", [16, 32])
def test_wide_kernel_gives_the_narrow_kernels_beams(device, K):
    rng = np.random.default_rng(300 + K)
    T, N, V = 30, 8, 70
    lg = _peaky_logits(rng, T, N, V, scale=SCALE)
    lens = rng.integers(0, T + 1, N)
    tl, tt = _dev(lg, device), _dev(lens, device)
    ey, eyl, eyp = (x.cpu().numpy() for x in F.ctc_prefix_search(tl, K, tt))
    y, yl, yp = (x.cpu().numpy() for x in _wide_cabi(tl, tt, K))
    assert np.array_equal(y, ey) and np.array_equal(yl, eyl)
    assert np.allclose(yp, eyp, rtol=RTOL, atol=0.0), np.abs(yp - eyp).max()


# ---- 4. strides and dtypes --------------------------------------------------------------------------
def test_wide_search_strides_and_dtypes(device):
    lg, lens, exp, marked = _case(64, 64)[1]
    T, N, V, K = 9, 3, 64, 64
    tt = _dev(lens, device)
    wide = torch.zeros((T, N, 2 * (V + 1)), device=device)
    wide[:, :, ::2] = _dev(lg, device)
    t = wide[:, :, ::2]
    assert t.stride(2) == 2
    _check_search(F.ctc_prefix_search(t, K, tt), exp, "strided vocabulary axis", marked)
    t = _dev(lg.transpose(1, 0, 2), device).transpose(0, 1)
    assert not t.is_contiguous() and t.shape == (T, N, V + 1)
    _check_search(F.ctc_prefix_search(t, K, tt), exp, "batch-major", marked)
    y, yl, yp = F.ctc_prefix_search(_dev(lg, device).double(), K, tt)
    assert yp.dtype == torch.double
    _check_search((y, yl, yp), exp, "float64", marked)
    half = lg.astype(np.float16)
    exp16 = oracle.ctc_prefix_search(half.astype(np.float32), K, lens)
    mk16 = _near_tied(half.astype(np.float32), K, lens, exp16)
    assert mk16.sum() <= 1
    y, yl, yp = F.ctc_prefix_search(_dev(half, device), K, tt)
    assert yp.dtype == torch.half
    # (the probabilities come back rounded to float16: the beams are compared, the masses to its precision)
    y, yl, yp = y.cpu().numpy()[:, ~mk16], yl.cpu().numpy()[~mk16], yp.float().cpu().numpy()[~mk16]
    fin = np.isfinite(exp16[2][~mk16])
    assert np.array_equal(y, exp16[0][:, ~mk16]) and np.array_equal(yl[fin], exp16[1][~mk16][fin])
    assert np.allclose(yp[fin], exp16[2][~mk16][fin], rtol=2e-3, atol=1e-7)


# ---- 5. more room in the beam than there are prefixes -----------------------------------------------
@pytest.mark.parametrize("K,V,T,N", [(64, 2, 5, 3), (128, 3, 4, 2)])
def test_wide_search_beam_wider_than_the_prefixes(device, K, V, T, N):
    """Every reachable prefix fits the beam, so the search is exact: the probabilities are those of a
    brute-force enumeration of the alignments; what is left of the beam is absent."""
    rng = np.random.default_rng(9 + K)
    lg = _peaky_logits(rng, T, N, V, scale=2.0)
    y, yl, yp = (x.cpu().numpy() for x in F.ctc_prefix_search(_dev(lg, device), K))
    assert not np.isnan(yp).any()
    p = np.exp(lg - lg.max(2, keepdims=True)).astype(np.float64)
    p /= p.sum(2, keepdims=True)
    for n in range(N):
        tot = {}
        for path in itertools.product(range(V + 1), repeat=T):
            pr = np.prod([p[t, n, c] for t, c in enumerate(path)])
            out, prev = [], None
            for c in path:
                if c != V and c != prev:
                    out.append(c)
                prev = c
            tot[tuple(out)] = tot.get(tuple(out), 0.0) + pr
        assert len(tot) <= K
        seen = set()
        for k in range(K):
            if not np.isfinite(yp[n, k]):
                assert yp[n, k] == -np.inf and yl[n, k] == 0 and not y[:, n, k].any()
                continue
            pref = tuple(y[: yl[n, k], n, k].tolist())
            assert pref not in seen
            seen.add(pref)
            want = tot.get(pref, 0.0)  # unreachable prefixes may fill a wide beam with mass 0
            assert abs(want - yp[n, k]) <= 1e-5 * want + 1e-9, (pref, want, yp[n, k])
            assert not y[yl[n, k] :, n, k].any()
        assert set(tot) <= seen


# ---- 6. a re-created intermediate prefix ------------------------------------------------------------
def _recreated_prefix_logits():
    """One utterance, V = 36, width 33, tokens a b c = 0 1 2, thirty fillers d_i = 3 .. 32, written as
    log-probabilities frame by frame:

      1. a.                         beam: a
      2. blank, b with 0.005.       a (0.995), ab (0.005)
      3. c 0.9, blank 0.05, the fillers share 0.05.
                                    ac, a, abc, a d_i x 30 -- 33 entries; ab (2.5e-4) is DROPPED, its
                                    extension abc (4.5e-3) and its prefix a stay
      4. b.                         a + b RE-CREATES ab while abc + b = abcb is in the beam: ab is a strict
                                    prefix of abcb, whose source abc is two tokens longer than ab's source
                                    a -- the token that follows ab inside abcb is in no table and is read
                                    off the trie (c)
      5. c 0.6, blank 0.4.          ab + c re-creates abc; whether it is a prefix of abcb (kept through the
                                    blank) is decided by the token found in frame 4, and the token that
                                    follows it there (b) takes a second walk
      6. b 0.55, blank 0.45.        abc + b IS abcb: its mass merges into that entry -- only if frames 4
                                    and 5 related the two; else the beam holds abcb twice
      7. a 0.7, blank 0.3.
    """
    V, a, b, c = 36, 0, 1, 2
    fillers = np.arange(3, 33)
    w = 0.97 ** np.arange(30)
    w /= w.sum()
    frames = [
        {a: 1.0},
        {b: 0.005, V: 0.995},
        dict([(c, 0.9), (V, 0.05)] + [(int(d), 0.05 * wi) for d, wi in zip(fillers, w)]),
        {b: 1.0},
        {c: 0.6, V: 0.4},
        {b: 0.55, V: 0.45},
        {a: 0.7, V: 0.3},
    ]
    p = np.empty((len(frames), 1, V + 1))
    for t, f in enumerate(frames):
        p[t, 0] = 1e-12 * (1.0 + 0.05 * np.arange(V + 1))  # everything else: tiny and distinct
        for v, q in f.items():
            p[t, 0, v] = q
    return np.log(p).astype(np.float32)


def _frames_that_walk(lg, K):
    """Replay on the CPU, frame by frame on the oracle's step function: the frames in which a new entry x,
    an extension, is a strict prefix of a new entry y whose source is at least two tokens longer than
    x's source -- where the kernel's next-token table cannot answer and the trie is walked."""
    T, N, V = lg.shape[0], lg.shape[1], lg.shape[2] - 1
    e = np.exp(lg - lg.max(2, keepdims=True))
    probs = (e / e.sum(2, keepdims=True)).astype(np.float32)
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y, last, lens = np.zeros((0, N, 1), np.int64), np.zeros((N, 1), np.int64), np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    hits = []
    for t in range(T):
        Kp = nb.shape[1]
        ext = np.ascontiguousarray(np.broadcast_to(probs[t, :, None, :V], (N, Kp, V)))
        y2, last2, lens2, (nb2, b2), isp2, src, non = oracle.ctc_prefix_search_advance(
            (ext, probs[t, :, :V], probs[t, :, V]), K, (nb, b), y, last, lens, isp
        )
        for n in range(N):
            ok = np.isfinite(nb2[n] + b2[n])
            sl = lens[n][src[n]]
            walk = (ok & ~non[n])[:, None] & ok[None, :] & isp2[n] & (lens2[n][:, None] < lens2[n][None, :])
            walk &= sl[None, :] > sl[:, None] + 1
            if walk.any():
                hits.append(t)
        y, last, lens, nb, b, isp = y2, last2, lens2, nb2, b2, isp2
    return hits


def test_recreated_intermediate_prefix_walks_the_trie(device):
    lg, K = _recreated_prefix_logits(), 33
    hits = _frames_that_walk(lg, K)
    assert 3 in hits and 4 in hits, hits  # frames 4 and 5 of the docstring
    exp = oracle.ctc_prefix_search(lg, K)
    assert not _near_tied(lg, K, None, exp).any()
    # the merge of frame 6 happened: abcb once, with abc's mass in it
    prefixes = [tuple(exp[0][: exp[1][0, k], 0, k]) for k in range(K)]
    assert len(set(prefixes)) == K
    _check_search(F.ctc_prefix_search(_dev(lg, device), K), exp, "re-created prefix")
    # several utterances side by side, the walk in one of them only
    rng = np.random.default_rng(5)
    both = np.concatenate([_peaky_logits(rng, 7, 1, 36, scale=SCALE), lg, _peaky_logits(rng, 7, 1, 36, scale=SCALE)], 1)
    exp = oracle.ctc_prefix_search(both, K)
    _check_search(F.ctc_prefix_search(_dev(both, device), K), exp, "re-created prefix, batch", _near_tied(both, K, None, exp))


# ---- 7. edges -------------------------------------------------------------------------------------
def test_wide_search_edges(device):
    K, V = 64, 64
    # no frame at all
    y, yl, yp = F.ctc_prefix_search(torch.zeros((0, 3, V + 1), device=device), K)
    assert y.shape == (0, 3, K) and not yl.any()
    assert (yp[:, 0] == 1).all() and (yp[:, 1:] == -float("inf")).all()
    # an utterance without frames among others
    rng = np.random.default_rng(77)
    lg = _peaky_logits(rng, 9, 4, V, scale=SCALE)
    lens = np.array([9, 0, 4, 0])
    exp = oracle.ctc_prefix_search(lg, K, lens)
    act = F.ctc_prefix_search(_dev(lg, device), K, _dev(lens, device))
    _check_search(act, exp, "lens = 0 among others", _near_tied(lg, K, lens, exp))
    yl, yp = act[1].cpu().numpy(), act[2].cpu().numpy()
    assert not yl[1].any() and yp[1, 0] == 1 and (yp[1, 1:] == -np.inf).all() and not act[0][:, 1].any()
    # no utterance
    y, yl, yp = F.ctc_prefix_search(torch.zeros((5, 0, V + 1), device=device), K)
    assert y.shape == (5, 0, K) and yl.shape == (0, K) and yp.shape == (0, K)
    y, yl, yp = F.ctc_prefix_search(torch.zeros((5, 0, V + 1), device=device), K, torch.zeros((0,), dtype=torch.long, device=device))
    assert y.shape == (0, 0, K)
    # S smaller than T: lens caps the rows of y
    lens = np.array([3, 5, 1, 4])
    exp = oracle.ctc_prefix_search(lg, K, lens)
    act = F.ctc_prefix_search(_dev(lg, device), K, _dev(lens, device))
    assert act[0].shape == (5, 4, K)
    _check_search(act, exp, "S < T", _near_tied(lg, K, lens, exp))
    # all lens 0: no row of y
    act = F.ctc_prefix_search(_dev(lg, device), K, torch.zeros((4,), dtype=torch.long, device=device))
    assert act[0].shape == (0, 4, K) and (act[2][:, 0] == 1).all() and (act[2][:, 1:] == -float("inf")).all()
    # beyond 128 the op still refuses ...
    with pytest.raises(RuntimeError, match="at most 128"):
        torch.ops.pydrobert_amd.ctc_prefix_search(_dev(lg, device), 129, None)


def test_width_129_still_runs_frame_by_frame(device):
    rng = np.random.default_rng(129)
    lg = _peaky_logits(rng, 9, 2, 150, scale=SCALE)
    exp = oracle.ctc_prefix_search(lg, 129)
    marked = _near_tied(lg, 129, None, exp)
    assert marked.sum() <= 1
    _check_search(F.ctc_prefix_search(_dev(lg, device), 129), exp, "F", marked)
    _check_search(M.CTCPrefixSearch(129)(_dev(lg, device)), exp, "module", marked)


# ---- 8. gradients keep their route ---------------------------------------------------------------------
def test_logits_that_require_grad_go_frame_by_frame(device, monkeypatch):
    rng = np.random.default_rng(8)
    lg = _dev(_peaky_logits(rng, 5, 2, 70, scale=SCALE), device).requires_grad_(True)
    calls = []
    stepwise = M.CTCPrefixSearch._frame_by_frame
    monkeypatch.setattr(M.CTCPrefixSearch, "_frame_by_frame", lambda self, *a: calls.append(1) or stepwise(self, *a))
    y, yl, yp = F.ctc_prefix_search(lg, 64)
    assert calls == [1] and yp.requires_grad
    yp[torch.isfinite(yp)].sum().backward()
    assert lg.grad is not None and torch.isfinite(lg.grad).all() and lg.grad.abs().sum() > 0
    ey, eyl, eyp = (x.cpu().numpy() for x in F.ctc_prefix_search(lg.detach(), 64))  # the one-launch search
    assert calls == [1]
    assert np.array_equal(y.cpu().numpy(), ey) and np.array_equal(yl.cpu().numpy(), eyl)
    assert np.allclose(yp.detach().cpu().numpy(), eyp, rtol=RTOL, atol=0.0)


# ---- rows beyond the LDS ----------------------------------------------------------------------------
def test_wide_search_rows_in_the_workspace(device):
    """A row of 20 001 probabilities does not fit the LDS next to the beam's state: it is kept in the
    utterance's row of the workspace."""
    rng = np.random.default_rng(20001)
    V, K = 20000, 33
    lg = _peaky_logits(rng, 3, 2, V, scale=12.0)
    lens = np.array([3, 2])
    exp = oracle.ctc_prefix_search(lg, K, lens)
    marked = _near_tied(lg, K, lens, exp)
    assert marked.sum() <= 1
    _check_search(F.ctc_prefix_search(_dev(lg, device), K, _dev(lens, device)), exp, "workspace rows", marked)
