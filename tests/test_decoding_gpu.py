"""GPU parity of the beam-search kernels vs the oracle (tie-free inputs).

Token sequences, lengths and source indices must match exactly; probabilities within 1e-5
relative (north star tolerance for float outputs).
"""
import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import modules as M

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def _peaky_logits(rng, T, N, V, scale=6.0):
    lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
    peak = rng.integers(0, V + 1, (T, N))
    np.put_along_axis(lg, peak[..., None], np.take_along_axis(lg, peak[..., None], 2) + scale, 2)
    return lg


def _check_search(act, exp, what):
    y, yl, yp = (x.cpu().numpy() for x in act)
    ey, eyl, eyp = exp
    assert y.shape == ey.shape and yl.shape == eyl.shape and yp.shape == eyp.shape, what
    fin = np.isfinite(eyp)
    assert np.array_equal(np.isfinite(yp), fin), what
    assert np.array_equal(yl[fin], eyl[fin]), (what, np.argwhere(yl != eyl)[:5])
    assert np.array_equal(y, ey), (what, np.argwhere(y != ey)[:5])
    assert np.allclose(yp[fin], eyp[fin], rtol=RTOL, atol=0.0), (what, np.abs(yp[fin] - eyp[fin]).max())


@pytest.mark.parametrize("V", [2, 5, 12, 70, 300])
@pytest.mark.parametrize("K", [1, 2, 4, 16, 32])
def test_ctc_prefix_search_random(device, V, K):
    if K > V + 1:
        # the reference itself breaks here: padded beam entries carry b = -inf * 0 = NaN into the
        # next frame (_decoding.py:875) and NaN wins every later topk.  See test_ctc_wide_beam.
        pytest.skip("reference yields NaN when width exceeds the number of valid paths")
    rng = np.random.default_rng(1000 * V + K)
    for it, (T, N) in enumerate([(1, 3), (7, 5), (30, 8), (64, 4)]):
        lg = _peaky_logits(rng, T, N, V, scale=4.0 if V < 20 else 8.0)
        lens = None if it % 2 == 0 else rng.integers(0, T + 1, N)
        exp = oracle.ctc_prefix_search(lg, K, lens)
        act = F.ctc_prefix_search(torch.from_numpy(lg).to(device), K,
                                  None if lens is None else torch.from_numpy(lens).to(device))  # fmt: skip
        _check_search(act, exp, (V, K, T, N))


def _ctc_plan(V, K):
    """(status, (producers, ring slots, utterances per workgroup, where a row is held, register chunks))
    the library picks for rows of V tokens (host arithmetic only: include/pdt_amd.h)."""
    import ctypes

    from pydrobert_amd import _cabi

    out = (ctypes.c_int32 * 5)()
    rc = _cabi.lib().pdt_ctc_prefix_search_plan(V, K, out)
    return rc, tuple(out)


def _plan_boundaries(K, hi=17000):
    """Every V at which the launch configuration changes, found from the library's own answer."""
    edges, lo = [], 1
    while True:
        cur = _ctc_plan(lo, K)
        if _ctc_plan(hi, K) == cur:
            return edges
        a, b = lo, hi  # plan(a) == cur != plan(b): bisect the first change
        while b - a > 1:
            m = (a + b) // 2
            if _ctc_plan(m, K) == cur:
                a = m
            else:
                b = m
        edges.append(b)
        lo = b


def _long_row_cases():
    """(V, K, PDT_CTC_ROWREG): a few fixed row lengths and one V on each side of every change of
    configuration -- with the long rows in the producers' registers (the default: a change is also
    every new register-chunk count of ctc_rowreg.hip) and with that form switched off (the LDS /
    workspace rows of ctc_search.hip, which also serve strided logits)."""
    from pydrobert_amd import switches

    cases = []
    for rowreg in (1, 0):
        with switches.override(PDT_CTC_ROWREG=rowreg):
            mine = [(513, 16), (700, 8), (1200, 32), (4600, 16), (9000, 4), (11000, 16), (15000, 8), (40000, 16)]
            for K in (16, 32):
                for edge in _plan_boundaries(K, hi=20000):
                    mine += [(edge - 1, K), (edge, K)]  # one V on each side of every change
        cases += [(V, K, rowreg) for V, K in sorted(set(mine))]
    return cases


@pytest.mark.parametrize("V,K,rowreg", _long_row_cases())
def test_ctc_prefix_search_long_rows(device, V, K, rowreg, switch):
    """Vocabularies beyond 511.  Default: the row of a frame stays in the registers of the producer
    wave that read it, up to 16 447 tokens (ctc_rowreg.hip, instantiations by register-chunk count).
    PDT_CTC_ROWREG=0: three producer waves around an LDS ring of rows (four slots, then three),
    finally rows that stay in the HBM workspace because no LDS ring holds them.  One V on each side of
    every change of configuration, ragged lens shorter than the number of producers included."""
    switch("PDT_CTC_ROWREG", rowreg)
    rng = np.random.default_rng(7000 + V)
    for it, (T, N) in enumerate([(2, 3), (25, 5), (61, 2)] if V < 10000 else [(2, 3), (23, 3)]):
        lg = _peaky_logits(rng, T, N, V, scale=11.0 if V < 10000 else 13.0)
        lens = None if it == 1 else rng.integers(0, T + 1, N)
        exp = oracle.ctc_prefix_search(lg, K, lens)
        act = F.ctc_prefix_search(torch.from_numpy(lg).to(device), K,
                                  None if lens is None else torch.from_numpy(lens).to(device))  # fmt: skip
        _check_search(act, exp, (V, K, T, N, _ctc_plan(V, K)))


@pytest.mark.parametrize("rowreg", [1, 0])
def test_ctc_prefix_search_workspace_rows_long_input(device, rowreg, switch):
    """Rows in the workspace (V beyond the three-slot LDS ring; PDT_CTC_ROWREG=0) or in registers with
    a ring of lists (the default) and an input long enough that the checkpoint table of the output
    walk, at 32-frame spacing, would not fit the LDS it overlays in either form: the spacing has to
    come from the layout the plan really uses."""
    V, K, T, N = 10400, 32, 4300, 1
    switch("PDT_CTC_ROWREG", rowreg)
    rc, plan = _ctc_plan(V, K)
    assert rc == 0 and plan[3] == (3 if rowreg else 2), plan
    rng = np.random.default_rng(424242)
    lg = _peaky_logits(rng, T, N, V, scale=19.0)  # p_peak ~ 0.9999: masses survive 4300 frames
    tl = torch.from_numpy(lg).to(device)
    act = F.ctc_prefix_search(tl, K)
    # (the C oracle needs minutes at this size: the check is the frame-by-frame route -- dense
    # histories, no trie, no checkpoints, itself pinned to the oracle by the tests above -- and
    # the best path, which at this peakiness is the collapsed arg-max sequence)
    exp = tuple(x.cpu().numpy() for x in M.CTCPrefixSearch(K)._frame_by_frame(tl, None, {}))
    assert exp[1].max() > 4100  # prefixes nearly as long as the input: the walk crosses every checkpoint
    y, yl, yp = (x.cpu().numpy() for x in act)
    assert np.array_equal(yl, exp[1]) and np.array_equal(y, exp[0])
    # (a product of 4300 per-frame factors, each within an ulp or two of torch's softmax: the
    # tokens are the point here, the masses only have to agree to the accumulated rounding)
    assert np.allclose(yp, exp[2], rtol=5e-3, atol=0.0), np.abs(yp / exp[2] - 1).max()
    best = lg[:, 0].argmax(1)
    keep = np.concatenate([[True], best[1:] != best[:-1]]) & (best != V)
    assert yl[0, 0] == keep.sum() and np.array_equal(y[: yl[0, 0], 0, 0], best[keep])


def test_ctc_plan_covers_every_vocabulary():
    """Every row length has a configuration (rows beyond the LDS: plan[3] == 2, the workspace)."""
    for V in (1, 64, 65, 511, 512, 5000, 16000, 16200, 100000, 1 << 20):
        rc, plan = _ctc_plan(V, 16)
        assert rc == 0 and plan[0] >= 1, (V, rc, plan)
    assert _ctc_plan(1 << 20, 16)[1][3] == 2 and _ctc_plan(256, 16)[1][3] == 1 and _ctc_plan(5000, 16)[1][3:] == (3, 80)
    assert _ctc_plan(16447, 16)[1][3:] == (3, 256) and _ctc_plan(16448, 16)[1][3] == 2


def test_ctc_prefix_search_golden_shape(device):
    """SURVEY G-D2 shape: T=30, N=8, V=12, K=4, peaky logits, ragged lens."""
    rng = np.random.default_rng(0x5EED0003)
    lg = _peaky_logits(rng, 30, 8, 12)
    lens = rng.integers(10, 31, 8)
    exp = oracle.ctc_prefix_search(lg, 4, lens)
    mod = M.CTCPrefixSearch(4)
    act = mod(torch.from_numpy(lg).to(device), torch.from_numpy(lens).to(device))
    _check_search(act, exp, "golden")


def test_ctc_prefix_search_long(device):
    """Longer searches with related beams (trie walks, re-created prefixes); lengths chosen so
    float32 prefix masses do not underflow to 0 (after which everything is a tie)."""
    rng = np.random.default_rng(5)
    for T, V, K, scale in [(60, 7, 8, 3.0), (40, 3, 4, 1.0), (300, 40, 16, 9.0), (90, 11, 12, 4.0)]:
        lg = _peaky_logits(rng, T, 6, V, scale=scale)
        exp = oracle.ctc_prefix_search(lg, K)
        assert exp[2].min() > 0.0
        act = F.ctc_prefix_search(torch.from_numpy(lg).to(device), K)
        _check_search(act, exp, ("long", T, V, K))


def test_ctc_prefix_search_many_checkpoints(device):
    """Long utterances: the output walk goes through many checkpoints, and with a small ring
    (small V) the checkpoint spacing doubles until the table fits; ragged lengths end between
    checkpoints.  Very peaky frames keep the float32 masses away from 0."""
    rng = np.random.default_rng(77)
    for T, V, K, N in [(1200, 4, 6, 4), (700, 30, 16, 3), (333, 2, 3, 5)]:
        lg = _peaky_logits(rng, T, N, V, scale=14.0)
        lens = rng.integers(T // 3, T + 1, N)
        lens[0] = T
        exp = oracle.ctc_prefix_search(lg, K, lens)
        assert exp[2][:, 0].min() > 0.0
        act = F.ctc_prefix_search(torch.from_numpy(lg).to(device), K, torch.from_numpy(lens).to(device))
        _check_search(act, exp, ("checkpoints", T, V, K))


def test_ctc_prefix_search_masked_tokens(device):
    """-inf logits (masked vocabulary entries) and rows with a huge dynamic range: the
    threshold guess of the short lists sees a -inf / overflowing row mean and must fall back to
    the complete selection."""
    rng = np.random.default_rng(99)
    for T, V, K in [(40, 70, 8), (33, 300, 16)]:
        lg = _peaky_logits(rng, T, 5, V, scale=9.0)
        dead = rng.random((T, 5, V + 1)) < 0.3
        dead[np.arange(T)[:, None], np.arange(5)[None], lg.argmax(2)] = False  # keep the peak
        lg[dead] = -np.inf
        lg[T // 2] *= 1e30  # finite, but the row sum overflows
        exp = oracle.ctc_prefix_search(lg, K)
        act = F.ctc_prefix_search(torch.from_numpy(lg).to(device), K)
        _check_search(act, exp, ("masked", T, V, K))


def test_ctc_wide_beam(device):
    """width > V + 1: the kernel treats padded entries as absent (documented superset of the
    reference, which degenerates to NaN).  Checks: no NaN, valid prefixes are distinct, their
    probabilities are the exact CTC prefix probabilities of a brute-force enumeration."""
    rng = np.random.default_rng(9)
    T, N, V, K = 4, 3, 2, 16
    lg = _peaky_logits(rng, T, N, V, scale=2.0)
    y, yl, yp = (x.cpu().numpy() for x in F.ctc_prefix_search(torch.from_numpy(lg).to(device), K))
    assert not np.isnan(yp).any()
    p = np.exp(lg - lg.max(2, keepdims=True))
    p /= p.sum(2, keepdims=True)
    import itertools

    for n in range(N):
        # brute force: sum over all alignments of length T
        tot = {}
        for path in itertools.product(range(V + 1), repeat=T):
            pr = np.prod([p[t, n, c] for t, c in enumerate(path)])
            out, prev = [], None
            for c in path:
                if c != V and c != prev:
                    out.append(c)
                prev = c
            tot[tuple(out)] = tot.get(tuple(out), 0.0) + pr
        seen = set()
        for k in range(K):
            if not np.isfinite(yp[n, k]):
                continue
            pref = tuple(y[: yl[n, k], n, k].tolist())
            assert pref not in seen
            seen.add(pref)
            want = tot.get(pref, 0.0)  # unreachable prefixes may fill a wide beam with mass 0
            assert abs(want - yp[n, k]) <= 1e-5 * want + 1e-9, (pref, want, yp[n, k])
        # every reachable prefix fits in the beam here, so all of them must be present
        assert set(tot) <= seen or len(seen) == K


@pytest.mark.parametrize("V,K", [(40, 33), (64, 64), (150, 100)])
def test_ctc_prefix_search_wider_than_the_kernel_holds(device, V, K):
    """More than 32 prefixes: frame by frame on the plain step kernel (csrc/advance_wide.hip), through
    the same entry points."""
    rng = np.random.default_rng(V + K)
    for it, (T, N) in enumerate([(1, 2), (9, 3), (25, 4)]):
        lg = _peaky_logits(rng, T, N, V, scale=3.0)
        lens = None if it % 2 == 0 else rng.integers(0, T + 1, N)
        exp = oracle.ctc_prefix_search(lg, K, lens)
        tl = None if lens is None else torch.from_numpy(lens).to(device)
        _check_search(F.ctc_prefix_search(torch.from_numpy(lg).to(device), K, tl), exp, (V, K, T, N))
        if it == 1:
            _check_search(M.CTCPrefixSearch(K)(torch.from_numpy(lg).to(device), tl), exp, (V, K, T, N, "module"))


def test_ctc_default_shape_instances_match_the_general_kernels(device):
    """ctc_search.hip has instantiations with the beam width 16 and the vocabulary size 256 (and with
    them the LDS layout and contiguous rows) as compile-time constants.  The same values through the
    general kernels -- a vocabulary axis with a stride (run-time strides: the width-16 instance), and
    widths 15 / 17 around the default against the oracle -- give the same bits / the oracle's
    answers; ragged lengths, several hundred frames (checkpoints, underflow guard), V = 256 .. 258."""
    rng = np.random.default_rng(123)
    T, N = 300, 37
    for V in (256, 257, 258):
        lg = _peaky_logits(rng, T, N, V, scale=6.0)
        lens = rng.integers(0, T + 1, N)
        tl = torch.from_numpy(lens).to(device)
        dense = torch.from_numpy(lg).to(device)
        wide = torch.zeros((T, N, 2 * (V + 1)), device=device)
        wide[:, :, ::2] = dense
        a = F.ctc_prefix_search(dense, 16, tl)
        b = F.ctc_prefix_search(wide[:, :, ::2], 16, tl)
        for x, y in zip(a, b):
            assert torch.equal(x, y), V
        exp = oracle.ctc_prefix_search(lg[:60, :8], 16, np.minimum(lens[:8], 60))
        _check_search(F.ctc_prefix_search(dense[:60, :8].contiguous(), 16, tl[:8].clamp(max=60)), exp, (V, 16))
        for K in (15, 17):
            exp = oracle.ctc_prefix_search(lg[:60, :8], K, np.minimum(lens[:8], 60))
            _check_search(F.ctc_prefix_search(dense[:60, :8].contiguous(), K, tl[:8].clamp(max=60)), exp, (V, K))


def test_two_frames_per_producer_pass_same_bits_as_one(device, switch):
    """V = 256, W = 16 (the BASELINE shape): the producer of ``ctc_search_kernel<1,4,true,false,16,256,true>``
    takes two frames per pass, one per half wave (PDT_CTC_PAIR, round 5).  Same bits as the one-frame form
    -- the normaliser is summed in that form's association -- on: odd and tiny frame counts (the upper
    half repeats the last frame), ragged lengths incl. 0 and 1, flat rows (every pass misses the
    short-list window), exact ties (few distinct logits: the (value, token) re-sort of a half), rows
    with -inf logits (the clamped exp instead of the tame one), duplicated rows.  And against the oracle."""
    rng = np.random.default_rng(505)
    V, K = 256, 16
    for it, (T, N, scale) in enumerate([(1, 5, 12.0), (2, 5, 12.0), (3, 9, 12.0), (65, 40, 12.0), (130, 33, 6.0), (64, 24, 0.0),
                                        (97, 16, 12.0), (96, 16, 12.0), (40, 12, 9.0)]):
        lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
        np.put_along_axis(lg, rng.integers(0, V + 1, (T, N, 1)), scale, 2)
        if it == 6:
            lg = np.round(lg * 2) / 2  # exact ties everywhere
        if it == 7:
            lg[:, :, rng.integers(0, V, 60)] = -np.inf  # masked vocabulary: rows that are not tame
        if it == 8:
            lg[1::2] = lg[0::2][: lg[1::2].shape[0]]  # every frame twice
        x = torch.from_numpy(lg).to(device)
        lens = rng.integers(0, T + 1, N)
        lens[:3] = [0, min(1, T), T]
        for ln in (None, torch.from_numpy(lens).to(device)):
            outs = []
            for pair in (1, 0):
                switch("PDT_CTC_PAIR", pair)
                outs.append(F.ctc_prefix_search(x, K, ln))
            for p, q in zip(*outs):
                assert torch.equal(p, q), (it, T, N, scale, ln is not None)
        if it in (3, 4):  # (tie-free inputs: the oracle's beams)
            switch("PDT_CTC_PAIR", 1)
            exp = oracle.ctc_prefix_search(lg, K, lens)
            _check_search(F.ctc_prefix_search(x, K, torch.from_numpy(lens).to(device)), exp, (it, "oracle"))


def test_lean_tier_extras_match_the_full_tiers(device, switch):
    """A frame whose winners include one prefix's third-and-deeper list entries, or two candidates
    that agree in the upper 26 bits of their masses, is decided beside the lean tier (ctc_frame.hpp:
    mid tier / exact re-ranking) -- with PDT_CTC_LEAN_EXTRA=0 by the full tiers.  Same bits on inputs
    built to hit both all the time: few distinct logit values (exact ties everywhere), duplicated
    logits (two tokens equal in a quarter of the rows -- the prefixes they start carry equal masses
    from then on), values on a coarse grid (near ties), blank-dominated rows (dense is-prefix relations:
    the pair-parallel update against the per-descendant loops); short rows (both instances) and register rows."""
    rng = np.random.default_rng(99)
    for it in range(32):
        V = int(rng.choice([256, 256, 300, 1000, 40])); W = int(rng.choice([16, 16, 8, 32, 5]))
        T = int(rng.choice([40, 120, 300])); N = int(rng.integers(2, 24))
        kind = it % 4
        lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
        peak = rng.integers(0, V + 1, (T, N, 1))
        if kind == 3:  # blank-dominated rows: short prefixes, dense is-prefix relations (the pair-parallel update)
            peak = np.where(rng.random((T, N, 1)) < 0.9, V, peak)
        np.put_along_axis(lg, peak, float(rng.choice([6.0, 9.0, 12.0])), 2)
        if kind == 0:
            lg = np.round(lg * 2) / 2
        elif kind == 1:
            for _ in range(T * N // 4):
                t, n = rng.integers(0, T), rng.integers(0, N)
                a, b = rng.integers(0, V, 2)
                lg[t, n, b] = lg[t, n, a]
        else:
            lg = np.round(lg * 4096) / 4096
        lens = torch.from_numpy(rng.integers(T // 2, T + 1, N)).to(device)
        x = torch.from_numpy(lg).to(device)
        outs = []
        for extra in (1, 0):
            switch("PDT_CTC_LEAN_EXTRA", extra)
            outs.append(F.ctc_prefix_search(x, W, lens))
        for p, q in zip(*outs):
            assert torch.equal(p, q), (it, V, W, T, N, kind)
    # narrow beams on few distinct values / masked rows: a tied pair at ranks (K - 1, K) whose bucket goes
    # on at rank K + 1 (a fuzz of 1 500 cases found the pairwise fix wrong there; profiles/tools/fuzz_tiers.py)
    for it in range(30):
        V = int(rng.choice([40, 64, 256])); W = int(rng.choice([2, 3, 5])); T = int(rng.choice([64, 300])); N = 40
        lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
        np.put_along_axis(lg, rng.integers(0, V + 1, (T, N, 1)), float(rng.choice([4.0, 8.0])), 2)
        if it % 2 == 0:
            lg = np.round(lg * 2) / 2
        else:
            lg[:, :, rng.integers(0, V, V // 4)] = -np.inf
        x = torch.from_numpy(lg).to(device)
        outs = []
        for extra in (1, 0):
            switch("PDT_CTC_LEAN_EXTRA", extra)
            outs.append(F.ctc_prefix_search(x, W))
        for p, q in zip(*outs):
            assert torch.equal(p, q), ("narrow", it, V, W, T)


def test_ctc_default_shape_with_many_frames(device):
    """V = 256, width 16 with so many frames that the checkpoints of the output walk are spaced wider
    than 32 frames (the constant-shape instance holds 32 as a constant, so the launcher must pick the
    width-16 instance instead): against the oracle and, through a strided vocabulary axis, against the
    general kernel."""
    rng = np.random.default_rng(321)
    T, N, V = 2100, 3, 256
    lg = _peaky_logits(rng, T, N, V, scale=12.0)  # (peaky enough for float32 masses to last 2100 frames)
    lens = np.array([2100, 1500, 1793])
    tl = torch.from_numpy(lens).to(device)
    dense = torch.from_numpy(lg).to(device)
    a = F.ctc_prefix_search(dense, 16, tl)
    _check_search(a, oracle.ctc_prefix_search(lg, 16, lens), "many frames")
    wide = torch.zeros((T, N, 2 * (V + 1)), device=device)
    wide[:, :, ::2] = dense
    b = F.ctc_prefix_search(wide[:, :, ::2], 16, tl)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_ctc_strided_logits_and_errors(device):
    rng = np.random.default_rng(6)
    lg = _peaky_logits(rng, 12, 4, 9)
    t = torch.from_numpy(np.ascontiguousarray(lg.transpose(1, 0, 2))).to(device).transpose(0, 1)
    assert not t.is_contiguous()
    _check_search(F.ctc_prefix_search(t, 3), oracle.ctc_prefix_search(lg, 3), "strided")
    # long rows: batch-major storage keeps the rows contiguous (the register form), a vocabulary axis
    # with a stride does not (the LDS rows take it)
    lg = _peaky_logits(rng, 9, 3, 700, scale=10.0)
    exp = oracle.ctc_prefix_search(lg, 5)
    t = torch.from_numpy(np.ascontiguousarray(lg.transpose(1, 0, 2))).to(device).transpose(0, 1)
    _check_search(F.ctc_prefix_search(t, 5), exp, "batch-major long rows")
    wide = torch.zeros((9, 3, 2 * 701), device=device)
    wide[:, :, ::2] = torch.from_numpy(lg).to(device)
    t = wide[:, :, ::2]
    assert t.stride(2) == 2
    _check_search(F.ctc_prefix_search(t, 5), exp, "strided vocabulary axis")
    with pytest.raises(RuntimeError, match="3 dimensional"):
        F.ctc_prefix_search(t[0], 3)
    with pytest.raises(RuntimeError, match="lens must be 1"):
        F.ctc_prefix_search(t, 3, torch.zeros((4, 1), dtype=torch.long, device=device))
    with pytest.raises(ValueError):
        M.CTCPrefixSearch(0)


# ---------------------------------------------------------------------------------------
# step functions
# ---------------------------------------------------------------------------------------
def _cmp_ctc_step(act, exp, what):
    (y, last, lens, (nb, b), isp, src, non) = [
        tuple(z.cpu().numpy() for z in x) if isinstance(x, tuple) else x.cpu().numpy() for x in act
    ]
    (ey, elast, elens, (enb, eb), eisp, esrc, enon) = exp
    assert y.shape == ey.shape, what
    assert np.array_equal(lens, elens), (what, lens, elens)
    assert np.array_equal(src, esrc), (what, src, esrc)
    assert np.array_equal(non, enon), what
    assert np.array_equal(last, elast), what
    assert np.array_equal(isp, eisp), (what, np.argwhere(isp != eisp)[:5])
    valid = np.isfinite(enb)
    assert np.array_equal(np.isfinite(nb), valid), what
    assert np.allclose(nb[valid], enb[valid], rtol=RTOL, atol=0), what
    assert np.allclose(b[valid], eb[valid], rtol=RTOL, atol=0), what
    S1, N, W = ey.shape
    for n in range(N):
        for k in range(W):
            assert np.array_equal(y[: elens[n, k], n, k], ey[: elens[n, k], n, k]), (what, n, k)


@pytest.mark.parametrize(
    "V,W",
    [(3, 2), (4, 5), (9, 4), (30, 8), (100, 16), (300, 32), (12, 7), (40, 13), (60, 27), (33, 31),
     (50, 33), (39, 40), (70, 64), (200, 70), (1000, 100)],  # (beyond 32: the plain workgroup form)
)  # fmt: skip
def test_ctc_prefix_search_advance_teacher_forced(device, V, W):
    """Run the oracle's search with per-prefix (LM-like) extension probabilities and, at every
    frame, feed the oracle's state to the kernel and compare all seven outputs.  Widths that do
    not divide 64 over 20+ frames make the history copy end on every possible partial wave."""
    rng = np.random.default_rng(V * 100 + W)
    N, T = 3, 12 if W in (2, 4, 8, 16, 32) else 22
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y = np.zeros((0, N, 1), np.int64)
    last = lens = np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    for t in range(T):
        Kp = nb.shape[1]
        p = np.exp(rng.normal(size=(N, V + 1)) * 1.5).astype(np.float32)
        p /= p.sum(1, keepdims=True)
        nonext, blank = np.ascontiguousarray(p[:, :V]), np.ascontiguousarray(p[:, V])
        lm = np.exp(rng.normal(size=(N, Kp, V)) * 0.7).astype(np.float32)
        lm /= lm.sum(2, keepdims=True)
        ext = (lm ** 0.5 * nonext[:, None]).astype(np.float32)
        exp = oracle.ctc_prefix_search_advance((ext, nonext, blank), W, (nb, b), y, last, lens, isp)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        act = F.ctc_prefix_search_advance(
            (tt(ext), tt(nonext), tt(blank)), W, (tt(nb), tt(b)), tt(y), tt(last), tt(lens), tt(isp)
        )
        _cmp_ctc_step(act, exp, (V, W, t))
        y, last, lens, (nb, b), isp = exp[0], exp[1], exp[2], exp[3], exp[4]


def test_ctc_prefix_search_advance_broadcast_ext(device):
    """No-LM form: ext_probs_t is an expand()ed view of nonext_probs_t (stride 0)."""
    rng = np.random.default_rng(77)
    N, V, W = 4, 6, 4
    p = rng.dirichlet(np.ones(V + 1), N).astype(np.float32)
    nonext, blank = torch.from_numpy(p[:, :V].copy()).to(device), torch.from_numpy(p[:, V].copy()).to(device)
    z = lambda *s: torch.zeros(s, dtype=torch.long, device=device)  # noqa: E731
    act = F.ctc_prefix_search_advance(
        (nonext.unsqueeze(1).expand(N, 1, V), nonext, blank), W,
        (torch.zeros(N, 1, device=device), torch.ones(N, 1, device=device)),
        z(0, N, 1), z(N, 1), z(N, 1), torch.ones(N, 1, 1, dtype=torch.bool, device=device),
    )  # fmt: skip
    exp = oracle.ctc_prefix_search_advance(
        (p[:, None, :V].copy(), p[:, :V].copy(), p[:, V].copy()), W,
        (np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)),
        np.zeros((0, N, 1), np.int64), np.zeros((N, 1), np.int64), np.zeros((N, 1), np.int64),
        np.ones((N, 1, 1), bool),
    )  # fmt: skip
    _cmp_ctc_step(act, exp, "broadcast")


@pytest.mark.parametrize("V,W", [(5, 3), (64, 8), (65, 16), (300, 7), (1000, 16), (1024, 32), (1025, 4)])
def test_ctc_step_forms_the_extension_probabilities_itself(device, V, W):
    """pdt_ctc_prefix_search_advance_lm (round 5): the language model's scores go into the step, which mixes
    them with the frame's probabilities as fusion_ext does and never writes the result -- every output of
    fusion_ext + ctc_prefix_search_advance, to the bit, over a run of frames whose state is the kernel's
    own; both mixtures.  V = 1025 is past the kernel's rows: the operator makes the two calls itself.
    Also here: prefixes that share one expand()ed row of extension probabilities share one list
    (PDT_STEP_FLAT) -- same outputs as with a row each."""
    from pydrobert_amd import _step as D

    g = torch.Generator(device=device).manual_seed(V * 31 + W)
    N, T = 5, 14
    for valid_mixture in (False, True):
        nb, b = torch.zeros((N, 1), device=device), torch.ones((N, 1), device=device)
        y = torch.zeros((0, N, 1), dtype=torch.long, device=device)
        last = lens = torch.zeros((N, 1), dtype=torch.long, device=device)
        isp = torch.ones((N, 1, 1), dtype=torch.bool, device=device)
        for t in range(T):
            Kp = nb.shape[1]
            p = (torch.randn((N, V + 1), device=device, generator=g) * 1.5).softmax(1)
            nonext, blank = p[:, :V], p[:, V]
            lm = torch.randn((N, Kp, V), device=device, generator=g) * 2.0
            if t % 4 == 3:
                lm[:, :, ::3] = float("-inf")  # masked tokens
            ext = torch.ops.pydrobert_amd.fusion_ext(lm.reshape(N * Kp, V), nonext, blank, 0.3, valid_mixture)
            two = torch.ops.pydrobert_amd.ctc_prefix_search_advance(ext, nonext, blank, W, nb, b, y, last, lens, isp)
            one = D._ctc_step_with_lm_scores(lm, 0.3, valid_mixture, nonext, blank, W, nb, b, y, last, lens, isp)
            via_op = torch.ops.pydrobert_amd.ctc_prefix_search_advance_lm(
                lm, 0.3, valid_mixture, nonext, blank, W, nb, b, y, last, lens, isp
            )
            for i, (u, v, w) in enumerate(zip(one, two, via_op)):
                valid = slice(None)
                if i == 0:  # rows of y beyond the lengths are unspecified
                    m = torch.arange(u.shape[0], device=device).view(-1, 1, 1) < two[2].unsqueeze(0)
                    u, v, w = u * m, v * m, w * m
                assert torch.equal(u[valid], v[valid]) and torch.equal(u[valid], w[valid]), (V, W, valid_mixture, t, i)
            # the no-LM form of the same frame: one shared row against a row each
            shared = F.ctc_prefix_search_advance((nonext.unsqueeze(1).expand(N, Kp, V), nonext, blank), W, (nb, b), y, last, lens, isp)
            each = F.ctc_prefix_search_advance((nonext.unsqueeze(1).expand(N, Kp, V).contiguous(), nonext, blank), W, (nb, b), y, last, lens, isp)
            flat = lambda o: [o[0] * (torch.arange(o[0].shape[0], device=device).view(-1, 1, 1) < o[2].unsqueeze(0)), o[1], o[2], o[3][0], o[3][1], o[4], o[5], o[6]]  # noqa: E731
            for i, (u, v) in enumerate(zip(flat(shared), flat(each))):
                assert torch.equal(u, v), ("shared", V, W, t, i)
            y, last, lens, nb, b, isp = two[0], two[1], two[2], two[3], two[4], two[5]


def _ctc_state(rng, N, V, Kp):
    """A beam of Kp prefixes per batch element: the oracle's first frame from the empty prefix."""
    p = rng.dirichlet(np.ones(V + 1), N).astype(np.float32)
    nonext, blank = np.ascontiguousarray(p[:, :V]), np.ascontiguousarray(p[:, V])
    out = oracle.ctc_prefix_search_advance(
        (nonext[:, None].copy(), nonext, blank), Kp, (np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)),
        np.zeros((0, N, 1), np.int64), np.zeros((N, 1), np.int64), np.zeros((N, 1), np.int64), np.ones((N, 1, 1), bool),
    )  # fmt: skip
    return out[0], out[1], out[2], out[3], out[4]


def _ctc_frame_inputs(rng, N, V, Kp):
    p = np.exp(rng.normal(size=(N, V + 1)) * 1.5).astype(np.float32)
    p /= p.sum(1, keepdims=True)
    nonext, blank = np.ascontiguousarray(p[:, :V]), np.ascontiguousarray(p[:, V])
    lm = np.exp(rng.normal(size=(N, Kp, V)) * 0.7).astype(np.float32)
    lm /= lm.sum(2, keepdims=True)
    return (lm ** 0.5 * nonext[:, None]).astype(np.float32), nonext, blank


@pytest.mark.parametrize("Kp", [3, 9, 17])
def test_ctc_prefix_search_advance_waves_per_element(device, Kp):
    """The waves of a workgroup take the K' prefixes in turn, a power of two <= min(K', 8) of them: K' = 3
    (two waves, an odd prefix left over), 9 (eight waves, one prefix in a second round) and 17 (eight waves,
    three rounds, the last with one) at N = 2, V = 70, two frames each against the oracle.  (K' = 1, 2 and 8
    are what test_ctc_prefix_search_advance_teacher_forced's widths 2 and 8 already run.)"""
    rng = np.random.default_rng(9000 + Kp)
    N, V = 2, 70
    y, last, lens, (nb, b), isp = _ctc_state(rng, N, V, Kp)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    for t in range(2):
        assert nb.shape[1] == Kp
        ext, nonext, blank = _ctc_frame_inputs(rng, N, V, Kp)
        exp = oracle.ctc_prefix_search_advance((ext, nonext, blank), Kp, (nb, b), y, last, lens, isp)
        act = F.ctc_prefix_search_advance(
            (tt(ext), tt(nonext), tt(blank)), Kp, (tt(nb), tt(b)), tt(y), tt(last), tt(lens), tt(isp)
        )
        _cmp_ctc_step(act, exp, (Kp, t))
        y, last, lens, (nb, b), isp = exp[0], exp[1], exp[2], exp[3], exp[4]


@pytest.mark.parametrize("Kp", [2, 9, 17])
def test_ctc_step_with_lm_scores_waves_per_element(device, Kp):
    """The step that mixes the language model's scores itself runs at most four waves per element: K' = 2
    (two waves), 9 and 17 (four waves, three and five rounds, the last with one prefix) at N = 2, V = 70, both
    mixtures, against the oracle's step on fusion_ext's extension probabilities.  (K' = 1, 3 and 8 are what
    test_ctc_step_forms_the_extension_probabilities_itself's widths already run.)"""
    from pydrobert_amd import _step as D

    rng = np.random.default_rng(9100 + Kp)
    N, V = 2, 70
    y, last, lens, (nb, b), isp = _ctc_state(rng, N, V, Kp)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    for valid_mixture in (False, True):
        _, nonext, blank = _ctc_frame_inputs(rng, N, V, Kp)
        lm = torch.from_numpy((rng.normal(size=(N, Kp, V)) * 2.0).astype(np.float32)).to(device)
        ext = torch.ops.pydrobert_amd.fusion_ext(lm.reshape(N * Kp, V), tt(nonext), tt(blank), 0.3, valid_mixture)
        exp = oracle.ctc_prefix_search_advance((ext.cpu().numpy(), nonext, blank), Kp, (nb, b), y, last, lens, isp)
        o = D._ctc_step_with_lm_scores(
            lm, 0.3, valid_mixture, tt(nonext), tt(blank), Kp, tt(nb), tt(b), tt(y), tt(last), tt(lens), tt(isp)
        )
        _cmp_ctc_step((o[0], o[1], o[2], (o[3], o[4]), o[5], o[6], o[7]), exp, (Kp, valid_mixture))


def test_ctc_prefix_search_advance_row_beyond_64k_of_lds(device):
    """ctc_advance_kernel<false> keeps the frame's row of V + 1 probabilities in LDS: at V = 16 400, width 2
    that is 65 616 bytes of row + 1 056 (K' = 1) or 1 568 (K' = 2) of frame scratch + 512 per wave = 67 184
    bytes in the first frame and 68 208 in the next two -- above the 64 KiB a kernel gets without asking.
    N = 1, three frames, against the oracle."""
    rng = np.random.default_rng(16400)
    N, V, W = 1, 16400, 2
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y = np.zeros((0, N, 1), np.int64)
    last = lens = np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    for t in range(3):
        ext, nonext, blank = _ctc_frame_inputs(rng, N, V, nb.shape[1])
        exp = oracle.ctc_prefix_search_advance((ext, nonext, blank), W, (nb, b), y, last, lens, isp)
        act = F.ctc_prefix_search_advance(
            (tt(ext), tt(nonext), tt(blank)), W, (tt(nb), tt(b)), tt(y), tt(last), tt(lens), tt(isp)
        )
        _cmp_ctc_step(act, exp, t)
        y, last, lens, (nb, b), isp = exp[0], exp[1], exp[2], exp[3], exp[4]


def test_ctc_prefix_search_advance_wide_beyond_64k_of_lds(device):
    """ctc_advance_wide_kernel's LDS is 16 K + 9 280 + 56 K' + 16 width bytes, K = min(width, K' (V + 1)): a beam
    of K' = 40 prefixes (V = 70) widened to 1 700 takes 27 200 + 9 280 + 2 240 + 27 200 = 65 920 bytes -- above the
    64 KiB a kernel gets without asking.  N = 1, against the oracle."""
    rng = np.random.default_rng(1700)
    N, V, Kp, W = 1, 70, 40, 1700
    y, last, lens, (nb, b), isp = _ctc_state(rng, N, V, Kp)
    ext, nonext, blank = _ctc_frame_inputs(rng, N, V, Kp)
    exp = oracle.ctc_prefix_search_advance((ext, nonext, blank), W, (nb, b), y, last, lens, isp)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    act = F.ctc_prefix_search_advance(
        (tt(ext), tt(nonext), tt(blank)), W, (tt(nb), tt(b)), tt(y), tt(last), tt(lens), tt(isp)
    )
    _cmp_ctc_step(act, exp, "wide")


@pytest.mark.parametrize("with_lens", [False, True])
def test_beam_search_advance_random(device, with_lens):
    rng = np.random.default_rng(31 + with_lens)
    for it in range(40):
        N, Kp, V = int(rng.integers(1, 5)), int(rng.integers(1, 9)), int(rng.integers(2, 90))
        W, S = int(rng.integers(1, 20)), int(rng.integers(0, 6))
        lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
        lpp = rng.normal(size=(N, Kp)).astype(np.float32)
        yp = rng.integers(0, V, (S, N, Kp))
        ypl = rng.integers(0, S + 1, (N, Kp)) if with_lens else None
        exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
        tt = lambda a: None if a is None else torch.from_numpy(a).to(device)  # noqa: E731
        act = [x.cpu().numpy() for x in F.beam_search_advance(tt(lpt), W, tt(lpp), tt(yp), tt(ypl))]
        K = min(W, Kp * V)
        assert act[0].shape == exp[0].shape, (it, act[0].shape, exp[0].shape)
        assert np.array_equal(act[1], exp[1]) and np.array_equal(act[3], exp[3]), it
        assert np.array_equal(act[2], exp[2]), it  # float adds are the same single operation
        assert np.array_equal(act[0][..., :K], exp[0][..., :K]), it


def test_beam_search_advance_without_growth(device):
    """All paths shorter than the history (y keeps its S rows, reference :133-137) with widths
    that leave a partial wave in the copy loop: the appended token must land at row lens."""
    rng = np.random.default_rng(41)
    for it in range(60):
        N, Kp, V = int(rng.integers(1, 4)), int(rng.integers(1, 12)), int(rng.integers(20, 70))
        W, S = int(rng.integers(9, 40)), int(rng.integers(2, 10))
        lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
        lpp = rng.normal(size=(N, Kp)).astype(np.float32)
        yp = rng.integers(0, V, (S, N, Kp))
        ypl = rng.integers(0, S, (N, Kp))  # strictly shorter than S
        exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
        tt = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        act = [x.cpu().numpy() for x in F.beam_search_advance(tt(lpt), W, tt(lpp), tt(yp), tt(ypl))]
        K = min(W, Kp * V)
        assert act[0].shape == exp[0].shape == (S, N, W), (it, act[0].shape, exp[0].shape)
        assert np.array_equal(act[1], exp[1]) and np.array_equal(act[3], exp[3]), it
        valid = np.arange(S)[:, None, None] < exp[1][None]
        valid[..., K:] = False
        assert np.array_equal(np.where(valid, act[0], 0), np.where(valid, exp[0], 0)), it


def _flat_case(rng, kind):
    N, Kp = int(rng.integers(1, 4)), int(rng.integers(1, 17))
    V = int(rng.integers(65, min(1100, 64 * (256 // Kp)) + 1))
    W, S = int(rng.integers(1, 40)), int(rng.integers(0, 5))
    lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
    lpp = rng.normal(size=(N, Kp)).astype(np.float32)
    if kind == 1:  # finished beams: a row is -inf but for one token (the same lane in every row)
        done = rng.random((N, Kp)) < 0.7
        if rng.random() < 0.5:
            done[0] = True  # ... every beam of an element
        eos = int(rng.integers(0, V))
        row = np.full(V, -np.inf, np.float32)
        row[eos] = 0.0
        lpt[done] = row
    elif kind == 2:  # exact ties everywhere
        lpt = np.round(lpt * 2) / 2
        lpp = np.round(lpp * 2) / 2
    elif kind == 3:  # the best candidates crowd one lane: more survivors than the list holds
        lane = int(rng.integers(0, 64))
        lpt[:, :, lane::64] += 30.0
    elif kind == 4:  # -inf nearly everywhere: fewer finite candidates than the width
        keep = rng.random(lpt.shape) < 3.0 / lpt[0].size
        lpt = np.where(keep, lpt, -np.inf).astype(np.float32)
    yp = rng.integers(0, V, (S, N, Kp))
    ypl = rng.integers(0, S + 1, (N, Kp)) if rng.random() < 0.5 else None
    return lpt, W, lpp, yp, ypl


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_beam_search_advance_flat_selection(device, switch, kind):
    """Rows of more than 64 tokens that fit the registers of a workgroup: the K winners come from ONE
    selection over all K' * V candidates (beam_advance_flat_kernel, round 5) -- against the oracle, and
    bit for bit against the sorted-list-per-prefix form (PDT_STEP_FLAT=0), contiguous and strided rows."""
    rng = np.random.default_rng(500 + kind)
    tt = lambda a: None if a is None else torch.from_numpy(a).to(device)  # noqa: E731
    for it in range(30):
        lpt, W, lpp, yp, ypl = _flat_case(rng, kind)
        exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
        lpt_d = tt(lpt)
        if it % 3 == 2:  # token stride 2
            wide = torch.zeros(lpt.shape[:2] + (2 * lpt.shape[2],), device=device)
            wide[..., ::2] = lpt_d
            lpt_d = wide[..., ::2]
        outs = []
        for flat in (1, 0):
            switch("PDT_STEP_FLAT", flat)
            outs.append([x.cpu().numpy() for x in F.beam_search_advance(lpt_d, W, tt(lpp), tt(yp), tt(ypl))])
        act, lists = outs
        K = min(W, lpt.shape[1] * lpt.shape[2])
        for a, b in zip(act, lists):
            assert np.array_equal(a, b), (kind, it)
        assert act[0].shape == exp[0].shape, (kind, it, act[0].shape, exp[0].shape)
        assert np.array_equal(act[2], exp[2]), (kind, it)
        # (-inf candidates tie: the kernels take the lowest flat index, the oracle's stable sort as well)
        assert np.array_equal(act[1], exp[1]) and np.array_equal(act[3], exp[3]), (kind, it)
        assert np.array_equal(act[0][..., :K], exp[0][..., :K]), (kind, it)


def test_beam_search_advance_wider_than_a_wave(device):
    """Widths and beam counts above 64 take the plain workgroup form: same answers, ties to the
    lowest flat index k * V + v (quantised values make exact ties common)."""
    rng = np.random.default_rng(77)
    shapes = [(2, 1, 200, 65), (2, 70, 9, 70), (1, 100, 37, 100), (3, 65, 3, 300), (2, 5, 300, 128), (1, 128, 130, 96)]
    for it, (N, Kp, V, W) in enumerate(shapes):
        for with_lens in (False, True):
            S = int(rng.integers(0, 5))
            lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
            lpp = rng.normal(size=(N, Kp)).astype(np.float32)
            if it % 2:
                lpt, lpp = np.round(lpt * 2) / 2, np.round(lpp * 2) / 2
            yp = rng.integers(0, V, (S, N, Kp))
            ypl = rng.integers(0, S + 1, (N, Kp)) if with_lens else None
            exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
            tt = lambda a: None if a is None else torch.from_numpy(a).to(device)  # noqa: E731
            act = [x.cpu().numpy() for x in F.beam_search_advance(tt(lpt), W, tt(lpp), tt(yp), tt(ypl))]
            K = min(W, Kp * V)
            assert act[0].shape == exp[0].shape, (it, act[0].shape, exp[0].shape)
            assert np.array_equal(act[1], exp[1]) and np.array_equal(act[3], exp[3]), (it, with_lens)
            assert np.array_equal(act[2], exp[2]), (it, with_lens)
            valid = np.arange(exp[0].shape[0])[:, None, None] < exp[1][None]
            valid[..., K:] = False
            assert np.array_equal(np.where(valid, act[0], 0), np.where(valid, exp[0], 0)), (it, with_lens)


def _cmp_beam_step(act, exp, K, what):
    act = [x.cpu().numpy() for x in act]
    assert act[0].shape == exp[0].shape, (what, act[0].shape, exp[0].shape)
    assert np.array_equal(act[1], exp[1]) and np.array_equal(act[3], exp[3]), what
    assert np.array_equal(act[2], exp[2]), what  # float adds are the same single operation
    valid = np.arange(exp[0].shape[0])[:, None, None] < exp[1][None]
    valid[..., K:] = False
    assert np.array_equal(np.where(valid, act[0], 0), np.where(valid, exp[0], 0)), what


@pytest.mark.parametrize("Kp", [1, 2, 3, 8, 9, 17])
def test_beam_search_advance_waves_per_element(device, Kp):
    """The list form's waves take the K' prefixes in turn, a power of two <= min(K', 8) of them: one wave,
    two, two with a prefix left over, eight, eight with one prefix in a second round, eight with three rounds
    -- N = 2, V = 70, with lengths, against the oracle.  Rows with a token stride of 2 take the list form; the
    same values in contiguous rows (the flat form, eight waves whatever K') must give the same."""
    rng = np.random.default_rng(9200 + Kp)
    N, V, W, S = 2, 70, 11, 4
    lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
    lpp = rng.normal(size=(N, Kp)).astype(np.float32)
    yp = rng.integers(0, V, (S, N, Kp))
    ypl = rng.integers(0, S + 1, (N, Kp))
    exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
    tt = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    strided = torch.zeros((N, Kp, 2 * V), device=device)
    strided[..., ::2] = tt(lpt)
    for rows in (strided[..., ::2], tt(lpt)):
        act = F.beam_search_advance(rows, W, tt(lpp), tt(yp), tt(ypl))
        _cmp_beam_step(act, exp, min(W, Kp * V), (Kp, rows.stride()))


def test_beam_search_advance_wide_beyond_64k_of_lds(device):
    """beam_advance_wide_kernel's LDS is 16 K + 9 280 + 12 width bytes, K = min(width, K' V): width 2 048 over
    K' V = 3 x 700 candidates takes 32 768 + 9 280 + 24 576 = 66 624 bytes -- above the 64 KiB a kernel gets
    without asking.  N = 1, against the oracle."""
    rng = np.random.default_rng(2048)
    N, Kp, V, W, S = 1, 3, 700, 2048, 2
    lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
    lpp = rng.normal(size=(N, Kp)).astype(np.float32)
    yp = rng.integers(0, V, (S, N, Kp))
    ypl = rng.integers(0, S + 1, (N, Kp))
    exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
    tt = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    act = F.beam_search_advance(tt(lpt), W, tt(lpp), tt(yp), tt(ypl))
    _cmp_beam_step(act, exp, W, "wide")


def test_beam_search_advance_errors(device):
    lpt = torch.zeros(2, 3, 4, device=device)
    with pytest.raises(RuntimeError, match="3 dimensional"):
        F.beam_search_advance(lpt[0], 2, torch.zeros(2, 3, device=device), torch.zeros(0, 2, 3, dtype=torch.long, device=device))
    with pytest.raises(RuntimeError, match="width"):
        F.beam_search_advance(lpt, 0, torch.zeros(2, 3, device=device), torch.zeros(0, 2, 3, dtype=torch.long, device=device))
    with pytest.raises(RuntimeError, match="Invalid lengths"):
        F.beam_search_advance(lpt, 2, torch.zeros(2, 3, device=device),
                              torch.zeros(0, 2, 3, dtype=torch.long, device=device),
                              torch.ones(2, 3, dtype=torch.long, device=device))  # fmt: skip


def test_host_report_left_armed_is_waited_for_before_it_is_armed_again(device, monkeypatch):
    """The words in pinned host memory a kernel reports to: a launch whose report was never read -- an exception
    between the launch and its wait, or inside the wait -- may still store to them, so arming them again first
    synchronises the device; a report that was read is armed again without one.  Then beam_search_advance with
    lengths reads its own verdict."""
    from pydrobert_amd import _cabi

    _cabi.host_report(device).disarm()  # (whatever an earlier test left)
    syncs = []
    sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda d=None: (syncs.append(d), sync(d))[1])
    N, Kp, V, W, S = 4, 3, 6, 5, 4
    reach = torch.full((N, Kp), S, dtype=torch.long, device=device)  # (a verdict of "y grows")
    report = _cabi.host_report(device)
    rc = _cabi.lib().pdt_lens_reach(_cabi.ptr(reach), Kp, 1, N, Kp, S, report.ptr, _cabi.stream_ptr(device))
    assert rc == _cabi.PDT_OK and not syncs
    report = _cabi.host_report(device)  # (armed again, its launch's report never read)
    assert syncs == [device] and not report.words.any()
    rc = _cabi.lib().pdt_lens_reach(_cabi.ptr(reach), Kp, 1, N, Kp, S, report.ptr, _cabi.stream_ptr(device))
    assert rc == _cabi.PDT_OK

    def interrupted():  # (as a KeyboardInterrupt would, without ending the session)
        raise RuntimeError("interrupted")

    with monkeypatch.context() as m:
        m.setattr(_cabi.time, "perf_counter", interrupted)
        with pytest.raises(RuntimeError, match="interrupted"):
            report.wait()
    report = _cabi.host_report(device)  # (armed again, its wait interrupted)
    assert syncs == [device, device] and not report.words.any()
    report.disarm()
    rng = np.random.default_rng(78)
    lpt = np.log(rng.dirichlet(np.ones(V), (N, Kp))).astype(np.float32)
    lpp = rng.normal(size=(N, Kp)).astype(np.float32)
    yp = rng.integers(0, V, (S, N, Kp))
    ypl = rng.integers(0, S, (N, Kp))  # (no path as long as the history: y does not grow)
    exp = oracle.beam_search_advance(lpt, W, lpp, yp, ypl)
    tt = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    act = [x.cpu().numpy() for x in F.beam_search_advance(tt(lpt), W, tt(lpp), tt(yp), tt(ypl))]
    assert act[0].shape == exp[0].shape == (S, N, W)
    assert np.array_equal(act[1], exp[1]) and np.array_equal(act[2], exp[2]) and np.array_equal(act[3], exp[3])
    valid = np.arange(S)[:, None, None] < exp[1][None]
    assert np.array_equal(np.where(valid, act[0], 0), np.where(valid, exp[0], 0))
    assert syncs == [device, device]


# ---------------------------------------------------------------------------------------
# gradients of the decoding outputs (the reference keeps them in its autograd graph)
# ---------------------------------------------------------------------------------------
def test_beam_search_advance_gradients(device):
    """log_probs_next carries gradients to log_probs_prev and log_probs_t exactly like the
    reference's graph (_decoding.py:121-131: sum, then top-k VALUES)."""
    rng = np.random.default_rng(3)
    for N, Kp, V, W in [(3, 4, 9, 5), (2, 1, 6, 6), (4, 7, 30, 16), (2, 3, 2, 8), (2, 70, 11, 80), (2, 3, 90, 66)]:  # (the last two: wider than a wave)
        lpt = torch.from_numpy(rng.normal(size=(N, Kp, V)).astype(np.float32)).log_softmax(-1)
        lpp = torch.from_numpy(rng.normal(size=(N, Kp)).astype(np.float32))
        yp = torch.from_numpy(rng.integers(0, V, (2, N, Kp)))
        g = torch.from_numpy(rng.normal(size=(N, W)).astype(np.float32))
        a, b = lpt.clone().requires_grad_(True), lpp.clone().requires_grad_(True)
        K = min(W, Kp * V)
        vals = (b.unsqueeze(2) + a).flatten(1).topk(K, 1)[0]
        (vals * g[:, :K]).sum().backward()
        a2, b2 = lpt.to(device).requires_grad_(True), lpp.to(device).requires_grad_(True)
        out = F.beam_search_advance(a2, W, b2, yp.to(device))
        assert out[2].requires_grad and not out[0].requires_grad
        torch.where(torch.isfinite(out[2]), out[2] * g.to(device), torch.zeros_like(out[2])).sum().backward()
        assert torch.allclose(a2.grad.cpu(), a.grad, atol=1e-6) and torch.allclose(b2.grad.cpu(), b.grad, atol=1e-6)


def test_ctc_prefix_search_advance_gradients(device):
    """(nb, b) of the step function are differentiable w.r.t. all five probability inputs;
    compared with autograd through the torch restatement of the reference's dense graph
    (oracle/torch_cpu.py), teacher-forced over several frames so that merges occur."""
    from oracle import torch_cpu as tc

    rng = np.random.default_rng(5)
    for V, W in [(4, 3), (6, 5), (3, 6), (9, 4), (40, 34)]:  # (34 prefixes: the plain workgroup form of the step)
        N = 3
        nb, b = torch.zeros(N, 1), torch.ones(N, 1)
        y = torch.zeros((0, N, 1), dtype=torch.long)
        last = lens = torch.zeros((N, 1), dtype=torch.long)
        isp = torch.ones((N, 1, 1), dtype=torch.bool)
        for t in range(7):
            Kp = nb.shape[1]
            p = torch.from_numpy(rng.random((N, V + 1)).astype(np.float32)).softmax(1)
            lm = torch.from_numpy(rng.random((N, Kp, V)).astype(np.float32))
            leaves = [(lm * p[:, None, :V]).contiguous(), p[:, :V].contiguous(), p[:, V].contiguous(), nb.clone(), b.clone()]
            gn, gb = torch.from_numpy(rng.normal(size=(N, W)).astype(np.float32)), torch.from_numpy(rng.normal(size=(N, W)).astype(np.float32))

            def loss(nb2, b2, gn, gb):
                ok = torch.isfinite(nb2)
                z = torch.zeros_like(nb2)
                return (torch.where(ok, nb2, z) * gn).sum() + (torch.where(ok, b2, z) * gb).sum()

            cpu = [x.clone().requires_grad_(True) for x in leaves]
            exp = tc.ctc_advance(cpu[0], cpu[1], cpu[2], W, cpu[3], cpu[4], y, last, lens, isp)
            loss(exp[3], exp[4], gn, gb).backward()
            dev = [x.to(device).requires_grad_(True) for x in leaves]
            act = F.ctc_prefix_search_advance(
                (dev[0], dev[1], dev[2]), W, (dev[3], dev[4]), y.to(device), last.to(device), lens.to(device), isp.to(device)
            )
            loss(act[3][0], act[3][1], gn.to(device), gb.to(device)).backward()
            assert torch.equal(act[2].cpu(), exp[2])  # same beam, so the same graph
            for name, c, d in zip(("ext", "nonext", "blank", "nb", "b"), cpu, dev):
                ok = torch.isfinite(c.grad)  # (-inf masses of absent prefixes make the dense graph's own gradient NaN)
                assert torch.isfinite(d.grad).all(), (name, V, W, t)
                assert torch.allclose(d.grad.cpu()[ok], c.grad[ok], rtol=1e-4, atol=1e-6), (name, V, W, t)
            y, last, lens, nb, b, isp = exp[0], exp[1], exp[2], exp[3].detach(), exp[4].detach(), exp[5]


def test_ctc_prefix_search_module_gradients(device):
    """CTCPrefixSearch probabilities are differentiable w.r.t. the logits (reference
    _decoding.py:1093, :1188): with requires_grad the Module runs frame by frame; same beams as the
    one-kernel search, gradients equal to those of the dense torch graph."""
    from oracle import torch_cpu as tc

    rng = np.random.default_rng(8)
    T, N, V, K = 12, 4, 7, 5
    lg = torch.from_numpy(_peaky_logits(rng, T, N, V, scale=3.0))
    w = torch.from_numpy(rng.normal(size=(N, K)).astype(np.float32))
    a = lg.clone().requires_grad_(True)
    ey, eyl, eyp = tc.ctc_prefix_search(a, K)
    (eyp * w).sum().backward()
    a2 = lg.to(device).requires_grad_(True)
    y, yl, yp = M.CTCPrefixSearch(K)(a2)
    assert yp.requires_grad
    fy, fyl, fyp = F.ctc_prefix_search(lg.to(device), K)
    assert torch.equal(yl, fyl) and torch.allclose(yp, fyp, rtol=1e-5)
    inside = torch.arange(T, device=device).view(-1, 1, 1) < yl.unsqueeze(0)
    assert torch.equal(y * inside, fy * inside) and torch.equal(yl.cpu(), eyl)
    (yp * w.to(device)).sum().backward()
    assert torch.allclose(a2.grad.cpu(), a.grad, rtol=1e-3, atol=1e-7), (a2.grad.cpu() - a.grad).abs().max()
    # ragged lengths take the same route
    lens = torch.tensor([12, 5, 0, 9])
    a3 = lg.to(device).requires_grad_(True)
    y3, yl3, yp3 = M.CTCPrefixSearch(K)(a3, lens.to(device))
    f3 = F.ctc_prefix_search(lg.to(device), K, lens.to(device))
    ok = torch.isfinite(f3[2])
    assert torch.equal(yl3[ok], f3[1][ok]) and torch.allclose(yp3[ok], f3[2][ok], rtol=1e-5)
    yp3[ok].sum().backward()
    assert torch.isfinite(a3.grad).all() and float(a3.grad[5:, 1].abs().max()) == 0.0  # frames past the length


def test_beam_search_trains_through_its_log_probs(device):
    """The MER recipe of the reference (_string.py:1573-1584): an n-best list out of BeamSearch,
    its log-probabilities into minimum_error_rate_loss, gradients into the language model."""
    from _toy_lm import BigramLM

    V, K, N = 6, 4, 3
    torch.manual_seed(2)
    table = torch.randn(V + 1, V).to(device).requires_grad_(True)

    class TrainableBigram(BigramLM):
        def __init__(self, t):
            torch.nn.Module.__init__(self)
            self.vocab_size = t.shape[1]
            self.table = t

    def run(tbl):
        search = M.BeamSearch(TrainableBigram(tbl.log_softmax(-1)), K).to(device)
        y, yl, lp = search(dict(), N, 5)
        return y, lp

    y, lp = run(table)
    assert lp.requires_grad
    ref = torch.randint(0, V, (5, N), device=device)
    loss = F.minimum_error_rate_loss(lp, ref, y, warn=False)
    (g,) = torch.autograd.grad(loss, table)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    # a directional finite difference of the loss with the beams held fixed by a tiny step
    d = torch.randn_like(table)
    eps = 1e-3
    lp_p, lp_m = run(table.detach() + eps * d)[1], run(table.detach() - eps * d)[1]
    fd = (F.minimum_error_rate_loss(lp_p, ref, y, warn=False) - F.minimum_error_rate_loss(lp_m, ref, y, warn=False)) / (2 * eps)
    assert abs(float(fd) - float((g * d).sum())) < 5e-2 * max(1.0, abs(float(fd))), (float(fd), float((g * d).sum()))


# ---------------------------------------------------------------------------------------
# exact ties: the lowest flat candidate index wins, in the kernels and in the oracle alike
# ---------------------------------------------------------------------------------------
def test_beam_search_advance_exact_ties(device):
    """Candidates whose float32 SUMS are equal although their log_probs_t differ (the rounding of
    log_probs_prev + log_probs_t merges them), equal log_probs_t inside one beam, and equal sums
    across beams: flat index k * V + v decides."""
    # (a) one beam, prev = 2^20: the ulp there is 1/8, so 0.01, 0.02 and 0.03 all round away
    lpt = torch.tensor([[[0.03, 0.01, -5.0, 0.02, -9.0, 0.03]]])
    lpp = torch.tensor([[1048576.0]])
    assert len({float(lpp[0, 0] + x) for x in lpt[0, 0, [0, 1, 3, 5]]}) == 1  # the sums do tie
    y = torch.zeros((0, 1, 1), dtype=torch.long)
    exp = oracle.beam_search_advance(lpt.numpy(), 4, lpp.numpy(), y.numpy())
    act = F.beam_search_advance(lpt.to(device), 4, lpp.to(device), y.to(device))
    assert act[0][0, 0].tolist() == exp[0][0, 0].tolist() == [0, 1, 3, 5]
    # (b) random cases built from few distinct values: ties everywhere, inside and across beams
    rng = np.random.default_rng(12)
    for it in range(200):
        N, Kp, V = int(rng.integers(1, 4)), int(rng.integers(1, 6)), int(rng.integers(2, 40))
        W = int(rng.integers(1, 12))
        lpt = rng.choice(np.array([-1.0, -1.5, -2.0, -3.0], np.float32), (N, Kp, V))
        lpp = rng.choice(np.array([0.0, -0.5, -1.0, 1e6], np.float32), (N, Kp))
        yp = rng.integers(0, V, (2, N, Kp))
        exp = oracle.beam_search_advance(lpt, W, lpp, yp)
        act = [x.cpu().numpy() for x in F.beam_search_advance(*(torch.from_numpy(a).to(device) for a in (lpt,)), W,
                                                               torch.from_numpy(lpp).to(device), torch.from_numpy(yp).to(device))]  # fmt: skip
        K = min(W, Kp * V)
        assert np.array_equal(act[3], exp[3]) and np.array_equal(act[2], exp[2]), it
        assert np.array_equal(act[0][..., :K], exp[0][..., :K]), it


def test_ctc_prefix_search_exact_ties(device):
    """Tokens with IDENTICAL logits give extensions of one prefix identical masses; the list is
    ordered (value, then token), so the lower token wins -- the oracle's flat index order.  The
    keys of such candidates collide in the lean tier's rounded 32-bit sort, which must hand the
    frame to the exact tiers instead of guessing."""
    rng = np.random.default_rng(4)
    for V, K, T in [(6, 4, 1), (20, 8, 1), (70, 16, 1), (300, 16, 1), (12, 5, 2)]:
        lg = rng.normal(size=(T, 3, V + 1)).astype(np.float32)
        lg[0, :, 1::2] = lg[0, :, : V + 1 : 2][:, : lg[0, :, 1::2].shape[1]]  # pairs (2i, 2i + 1) share a logit
        exp = oracle.ctc_prefix_search(lg[:1], K)
        act = F.ctc_prefix_search(torch.from_numpy(lg[:1]).to(device), K)
        _check_search(act, exp, ("ties", V, K))


_NEAR_TIE_CASE = {}


def _near_tie_case():
    """2048 utterances of moderately peaky logits and the oracle's beams (computed once)."""
    if not _NEAR_TIE_CASE:
        from concurrent.futures import ThreadPoolExecutor

        rng = np.random.default_rng(123)
        T, N, V, K = 120, 2048, 40, 8
        lg = _peaky_logits(rng, T, N, V, scale=5.0)

        def one(i):
            return oracle.ctc_prefix_search(np.ascontiguousarray(lg[:, i : i + 64]), K)

        with ThreadPoolExecutor(16) as ex:
            parts = list(ex.map(one, range(0, N, 64)))
        _NEAR_TIE_CASE.update(
            lg=lg, K=K, ey=np.concatenate([p[0] for p in parts], 1),
            eyl=np.concatenate([p[1] for p in parts]), eyp=np.concatenate([p[2] for p in parts]),
        )
    c = _NEAR_TIE_CASE
    return c["lg"], c["K"], c["ey"], c["eyl"], c["eyp"]


def _disagreeing(y, yl, ey, eyl):
    return [n for n in range(y.shape[1]) if not (np.array_equal(yl[n], eyl[n]) and np.array_equal(y[:, n], ey[:, n]))]


def test_ctc_prefix_search_near_ties_are_the_only_disagreements(device):
    """Probabilities are p * (1 / sum) with a guard-free exp: within an ulp or two of the
    reference's quotient.  That can swap two beam entries whose masses agree to ~1e-6 (measured by
    the fuzz scripts: ~4 utterances in 100 000).  Bound it: wherever the beams of kernel and oracle
    differ, they hold the same prefixes up to entries whose probabilities are within 1e-5 of a
    neighbour's, and the sorted probabilities agree to 1e-5 everywhere."""
    lg, K, ey, eyl, eyp = _near_tie_case()
    N = lg.shape[1]
    y, yl, yp = (x.cpu().numpy() for x in F.ctc_prefix_search(torch.from_numpy(lg).to(device), K))
    assert np.allclose(yp, eyp, rtol=1e-5, atol=0.0)  # sorted masses agree whatever the order of near-equal entries
    bad = _disagreeing(y, yl, ey, eyl)
    assert len(bad) <= 4, len(bad)  # a handful in 2048 at most
    for n in bad:
        mine = {tuple(y[: yl[n, k], n, k].tolist()) for k in range(K)}
        theirs = {tuple(ey[: eyl[n, k], n, k].tolist()) for k in range(K)}
        gap = np.abs(eyp[n, 1:] / eyp[n, :-1] - 1.0).min()
        # same prefixes in another order, or the K-th / (K+1)-th candidates were near-equal
        assert mine == theirs or gap < 1e-5, (n, gap)


def test_ctc_prefix_search_exact_division_switch(device, switch):
    """PDT_CTC_EXACT_DIV=1 makes the search form every probability as the IEEE quotient e / sum (what
    the reference's softmax does) instead of e * (1 / sum).  Same beams up to near ties either way;
    with the quotient the masses sit no further from the oracle's and no more utterances disagree --
    the switch a caller uses to tell the reciprocal's disagreements from real ones."""
    lg, K, ey, eyl, eyp = _near_tie_case()
    tl = torch.from_numpy(lg).to(device)
    res = {}
    for mode in ("0", "1"):
        switch("PDT_CTC_EXACT_DIV", mode)
        y, yl, yp = (x.cpu().numpy() for x in F.ctc_prefix_search(tl, K))
        assert np.allclose(yp, eyp, rtol=1e-5, atol=0.0)
        res[mode] = (len(_disagreeing(y, yl, ey, eyl)), float(np.abs(yp / eyp - 1.0).max()))
    assert res["1"][0] <= res["0"][0] and res["1"][0] <= 4, res
    assert res["1"][1] <= res["0"][1] * 1.5 + 1e-7, res


def _ulps(a, b):
    """Distance in float32 ulps between positive floats."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_why_near_ties_cannot_be_bit_exact_the_softmaxes_side_by_side(device, switch):
    """After ONE frame the beam of a search as wide as the row holds the frame's probabilities
    themselves (every token a prefix of length one, the empty prefix the blank): the kernel's softmax
    can be read off its output and put beside the reference's.  Measured on 4096 rows of 32 elements
    (MI355X, torch 2.10): the kernel's e * (1 / sum) equals torch's softmax on this device in 45 % of
    the elements, is 1 ulp off in 41 %, 2-4 ulps in 14 %; with PDT_CTC_EXACT_DIV=1 (e / sum) 55 % / 34 %
    / 12 %; against torch's softmax on the CPU -- what the reference's CPU path and tests/golden hold --
    up to 6 ulps either way.  And torch's OWN softmax on the device and on the CPU agree in only 67.5 %
    of the elements (up to 5 ulps apart).  So the last few ulps of a probability are not defined by the
    reference, two masses closer than that can come out in either order, and no arithmetic in the
    kernel can make the residual of test_ctc_prefix_search_near_ties... zero: that test bounds it
    instead (same prefixes, sorted masses to 1e-5).  Asserted here: the kernel within 8 ulps of both,
    the reference's two softmaxes not bit-equal, the quotient no further off than the reciprocal."""
    rng = np.random.default_rng(77)
    V, N = 31, 4096
    lg = (rng.normal(size=(1, N, V + 1)) * 3).astype(np.float32)
    tl = torch.from_numpy(lg).to(device)
    ref_dev = np.sort(tl.softmax(2)[0].cpu().numpy(), 1)[:, ::-1]
    ref_cpu = np.sort(torch.from_numpy(lg).softmax(2)[0].numpy(), 1)[:, ::-1]
    seen = {}
    for mode in (0, 1):
        switch("PDT_CTC_EXACT_DIV", mode)
        yp = F.ctc_prefix_search(tl, V + 1)[2].cpu().numpy()
        d_dev, d_cpu = _ulps(yp, np.ascontiguousarray(ref_dev)), _ulps(yp, np.ascontiguousarray(ref_cpu))
        seen[mode] = (int(d_dev.max()), float((d_dev == 0).mean()), int(d_cpu.max()), float((d_cpu == 0).mean()))
        assert d_dev.max() <= 8 and d_cpu.max() <= 8, seen
    own = _ulps(np.ascontiguousarray(ref_dev), np.ascontiguousarray(ref_cpu))
    # the reference's softmax against itself, device against host: identical bits would make the
    # argument above moot -- they are not
    assert own.max() >= 1 and (own == 0).mean() < 1.0, (int(own.max()), float((own == 0).mean()))
    # the quotient is no further from either than the reciprocal form
    assert seen[1][0] <= seen[0][0] + 1 and seen[1][2] <= seen[0][2] + 1, seen


@pytest.mark.parametrize("finish_all", [False, True])
def test_beam_search_fused_iterations_equal_the_step_by_step_loop(device, finish_all, switch):
    """BeamSearch with every iteration in one kernel (csrc/beam_step.hip; the number of unfinished
    batch elements read every eighth iteration) against the loop of reference-shaped torch ops around
    beam_search_advance (PDT_BEAM_FUSED=0): same paths, lengths and padding, log-probabilities to 1e-5;
    searches that end by eos at iterations that are no multiple of eight, by max_iters, at once.  The
    model has no state, so the batch elements of one search are copies of each other and finish at the
    same iteration; elements that finish apart are tests/test_beam_forms_gpu.py's mixed batches."""
    from _toy_lm import BigramLM

    class PositionalBigramLM(BigramLM):
        """Bigram scores plus a per-position offset: two orders of the same transitions no longer
        add up to the same log-probability (with the plain bigram table such paths tie up to the
        rounding of the sums and the two loops may order them differently)."""

        def __init__(self, table, pos):
            super().__init__(table)
            self.register_buffer("pos", pos)

        def calc_idx_log_probs(self, hist, prev, idx):
            lp, prev = super().calc_idx_log_probs(hist, prev, idx)
            return lp + self.pos[idx.clamp(max=self.pos.shape[0] - 1)], prev

    rng = np.random.default_rng(2024 + int(finish_all))
    for V, W, N, iters, eos_bias in [(9, 4, 5, 30, 1.5), (30, 8, 3, 21, 2.5), (6, 5, 7, 8, 0.0), (12, 3, 2, 0, 0.0),
                                     (40, 16, 33, 50, 3.0), (5, 8, 4, 12, 1.0)]:
        table = rng.normal(size=(V + 1, V)).astype(np.float32)
        table[:, 1] += eos_bias  # eos = 1 wins often enough to end paths at different iterations
        pos = rng.normal(size=(64, V)).astype(np.float32)
        lm = PositionalBigramLM(torch.from_numpy(table).to(device), torch.from_numpy(pos).to(device))
        for eos in (1, None):
            mod = M.BeamSearch(lm, W, eos, finish_all, -5).to(device)
            switch("PDT_BEAM_FUSED", "0")
            switch("PDT_CHECK_INVARIANTS", "1")  # (the loop's "y grows every iteration" is checked)
            ey, eyl, elp = mod(None, N, iters)
            switch("PDT_BEAM_FUSED", "1")
            y, yl, lp = mod(None, N, iters)
            what = (V, W, N, iters, eos, finish_all)
            assert y.shape == ey.shape and torch.equal(yl, eyl), (what, y.shape, ey.shape)
            assert torch.allclose(lp, elp, rtol=1e-5, atol=1e-6), what
            S = y.shape[0]
            mask = torch.arange(S, device=device).view(S, 1, 1) < eyl.unsqueeze(0)
            assert torch.equal(torch.where(mask, y, ey), ey), what  # tokens within the lengths
            if eos is not None and S:
                # padding of finished elements: identical wherever the step-by-step loop wrote pad_value
                assert torch.equal((y == -5).all(2), (ey == -5).all(2)), what
    # batch_size None (no batch dimension) and the hook: a subclass that overrides it keeps the loop
    mod = M.BeamSearch(lm, 3, 1).to(device)
    y, yl, lp = mod(None, None, 6)
    assert y.dim() == 2 and yl.shape == (3,) and lp.shape == (3,)

    class Hooked(M.BeamSearch):
        def update_log_probs_for_step(self, log_probs_prev, log_probs_t, y_prev, y_prev_lens, eos_mask):
            self.calls = getattr(self, "calls", 0) + 1
            return log_probs_prev, log_probs_t

    hooked = Hooked(lm, 3, 1).to(device)
    hy, hyl, hlp = hooked(None, 2, 5)
    assert hooked.calls >= 1 and hy.shape[1:] == (2, 3)
