"""Two steady frames at once (csrc/ctc_frame.hpp: ctc_two_steady_frames).  The two-frames-per-pass instance
of the CTC search (V = 256, K = 16, contiguous rows) decides an even-aligned pair of frames (t, t + 1) in one
go -- frame t in lanes 0-15, frame t + 1 in lanes 16-31 on the beam frame t would leave -- when the beam is
full, holds no strict-prefix relation and both frames pass the steady tier's test; otherwise nothing is
committed and both frames go through ctc_frame as before.  PDT_CTC_TWOFRAME=0 switches the pair path off
inside the same kernel instance, so every case runs the same launch twice: the outputs must be the same bits,
and the default setting must give the oracle's answer under the rules of test_decoding_gpu.py.

All cases use V = 256, K = 16 and contiguous rows: no other instance has the path.

The CPU side (no GPU needed) restates the steady tier's test on the oracle's step function, frame by frame
(as test_ctc_steady_lanes_gpu.py does), and asserts that the inputs reach what they were chosen for: the
bench-like headline case holds qualifying pairs, one of them ending on a checkpoint, and a pair whose first
frame is steady and whose second is not; each doctored utterance has its property in its frame.  The three
doctored utterances:

  * `second`: frame D + 1 (D even) has two tokens that nearly share the peak, so the best prefixes' second
    entries beat the K-th first entry: frame D is steady, frame D + 1 is not -- the speculation on row 1 is
    thrown away and nothing of frame D may have been committed;
  * `relation`: frame D - 1 gives the blank half of the mass, so parents stay next to their children: the
    even frame D starts with strict-prefix pairs in the beam, and the pair is refused at entry;
  * `bound`: test_ctc_steady_lanes_gpu.py's `short` construction moved one frame on, so that the frame that is
    steady with the bound of a short list's hidden second entry among its challengers is the odd frame 3.  A
    short list holds at least eight entries, so only a prefix whose children took its other entries can be
    left with one: such a beam has relations, and the pair (2, 3) must be refused at entry whatever frame 3
    looks like by itself.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import switches
from test_ctc_steady_gpu import _logits
from test_decoding_gpu import _check_search

V, K = 256, 16
# (T, N, ragged).  T = 70 crosses the checkpoints at 32 and 64, so the pairs (30, 31) and (62, 63) end on one,
# and N = 5 leaves the last workgroup an idle utterance; T = 69 has an odd tail; T = 1, 2, 3: no pair, one
# pair, one pair and a tail; ragged lengths: 0, odd and even ones
SHAPES = {
    "t70": (70, 5, False),
    "t69": (69, 5, False),
    "ragged": (70, 5, True),
    "t1": (1, 5, False),
    "t2": (2, 5, False),
    "t3": (3, 5, False),
}
RAGGED_LENS = np.array([0, 69, 70, 33, 24])
INPUTS = ["bench", "runs", "blank", "tied", "flat", "two_classes", "peak4", "doctored"]
BENCH_SEED = 3
SECOND, RELATION, BOUND = 1, 2, 3  # the doctored utterances
D = 30  # the doctored (even) frame of `second` and `relation`: the pair (30, 31) would end on a checkpoint
SHORT_MIN = 8  # the shortest list a producer hands over (csrc/ctc_ring.hpp)
CKPT = 32


def _seed(shape, kind):
    return BENCH_SEED if kind == "bench" else 4000 + 100 * list(SHAPES).index(shape) + INPUTS.index(kind)


@functools.lru_cache(maxsize=None)
def _doctored(T, N):
    """Bench-like rows; utterances SECOND, RELATION and BOUND as the module's text describes (T >= 32)."""
    rng = np.random.default_rng(777)
    lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
    peak = rng.integers(0, V + 1, (T, N, 1))
    first = K + 4
    for n in (SECOND, RELATION, BOUND):
        # peaks among the tokens K + 4 .. V - 1, never the blank and never the previous frame's: the bench's
        # distribution at its steadiest
        pk = first + peak[:, n, 0] % (V - first)
        for t in range(1, T):
            if pk[t] == pk[t - 1]:
                pk[t] = first + (pk[t] - first + 1) % (V - first)
        peak[:, n, 0] = pk
    np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 12.0, 2)
    u, w = 1, 2  # two tokens no peak of a doctored utterance uses

    def put(t, n, probs, scale=1.0):
        r = (scale * rng.normal(size=V + 1)).astype(np.float32)
        for c, q in probs.items():
            r[c] = np.float32(12.0 + np.log(q))
        lg[t, n] = r

    # second: two tokens nearly share the peak of frame D + 1
    r = rng.normal(size=V + 1).astype(np.float32)
    pk1 = int(peak[D + 1, SECOND, 0])
    r[pk1] += 12.0
    r[u] = r[pk1] - 0.25
    lg[D + 1, SECOND] = r
    # relation: the blank takes half of frame D - 1, a token the other half
    put(D - 1, RELATION, {V: 0.5, w: 0.495})
    # bound: the empty prefix and its K - 1 one-token children; two frames of blank; then the children's tokens
    # again, e^-3.5 below one new token, over a third of the usual noise
    a0 = 3
    put(0, BOUND, {V: 0.5, **{a0 + i: 0.03 * float(np.exp(-0.01 * i)) for i in range(K - 1)}})
    put(1, BOUND, {V: 0.997})
    put(2, BOUND, {V: 0.997})
    r = (0.3 * rng.normal(size=V + 1)).astype(np.float32)
    r[a0 : a0 + K - 1] = 8.5
    r[u] = 12.0
    lg[3, BOUND] = r
    lg.setflags(write=False)
    return lg


@functools.lru_cache(maxsize=None)
def _input(shape, kind):
    T, N, _ = SHAPES[shape]
    if kind == "doctored":
        return _doctored(max(T, 32), N)[:T]
    lg = _logits(kind, V, T, N, _seed(shape, kind))
    lg.setflags(write=False)
    return lg


def _lens(shape):
    return RAGGED_LENS if SHAPES[shape][2] else None


@functools.lru_cache(maxsize=None)
def _expected(shape, kind, cap):
    lg, lens = _input(shape, kind), _lens(shape)
    if cap is None:
        return oracle.ctc_prefix_search(lg, K, lens)
    T, N, _ = SHAPES[shape]
    lens_c = np.full(N, min(cap, T)) if lens is None else np.minimum(lens, cap)
    return oracle.ctc_prefix_search(lg[:cap], K, lens_c)


@functools.lru_cache(maxsize=None)
def _frames_cpu(shape, kind):
    """Frame by frame through the oracle's step function, the steady tier's four keys restated on the state in
    front of each frame (test_ctc_steady_lanes_gpu.py has the same model).  Returns per utterance a dict
    t -> flags for the frames that start with a full beam: 'steady' (every term of the test holds),
    'relation' (some prefix of the beam is a strict prefix of another), 'short' (a list of the shortest length
    a producer hands over would hide a prefix's second available entry)."""
    lg = _input(shape, kind)
    T, N, _ = lg.shape
    e = np.exp(lg - lg.max(2, keepdims=True))
    probs = (e / e.sum(2, keepdims=True)).astype(np.float32)
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y = np.zeros((0, N, 1), np.int64)
    y_lens = y_last = np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    out = [{} for _ in range(N)]
    f32 = np.float32
    for t in range(T):
        nonext, blank = np.ascontiguousarray(probs[t, :, :V]), np.ascontiguousarray(probs[t, :, V])
        Kp = nb.shape[1]
        full = (Kp == K) & ((nb + b) > 0).all(1)
        verdicts = {}
        for n in np.nonzero(full)[0]:
            p, pb = nonext[n], blank[n]
            order = np.lexsort((np.arange(V), -p))
            M = min(V, 2 * K)
            lens_n, last_n = y_lens[n], y_last[n]
            pref = [tuple(y[: lens_n[k], n, k]) for k in range(K)]
            tot = nb[n] + b[n]
            key0, key1, key2, key3 = (np.zeros(K, f32) for _ in range(4))
            flags = set()
            for k in range(K):
                lk = min(max(int(last_n[k]), 0), V - 1) if lens_n[k] else 0
                kids = {c[-1] for c in pref if len(c) == len(pref[k]) + 1 and c[:-1] == pref[k]}
                par = [q for q in range(K) if lens_n[k] and len(pref[q]) + 1 == len(pref[k]) and pref[k][:-1] == pref[q]]
                if any(len(c) > len(pref[k]) and c[: len(pref[k])] == pref[k] for c in pref):
                    flags.add("relation")
                av = [v for v in order[:M] if v != lk and v not in kids]
                if len([v for v in order[:SHORT_MIN] if v != lk and v not in kids]) < 2:
                    flags.add("short")
                key0[k], key1[k] = tot[k] * p[av[0]], tot[k] * p[av[1]]
                key2[k] = f32(0) if lk in kids else b[n, k] * p[lk]
                add = f32(0)
                for q in par:
                    lq = min(max(int(last_n[q]), 0), V - 1) if lens_n[q] else 0
                    add += ((f32(0) if lk == lq else nb[n, q]) + b[n, q]) * p[lk]
                key3[k] = (nb[n, k] * p[lk] + add) + tot[k] * pb
            kth = key0[K - 1]
            if not ((key0[:-1] < key0[1:]).any() or max(key1.max(), key2.max(), key3.max()) >= kth
                    or kth.view(np.uint32) + 1 <= 64):
                flags.add("steady")
            verdicts[n] = flags
            out[n][t] = frozenset(flags)
        ext = np.ascontiguousarray(np.broadcast_to(nonext[:, None, :], (N, Kp, V)))
        y, y_last, y_lens, (nb, b), isp, src, kept = oracle.ctc_prefix_search_advance(
            (ext, nonext, blank), K, (nb, b), y, y_last, y_lens, isp
        )
        for n, flags in verdicts.items():  # the model against the oracle's own step
            if "steady" in flags:
                assert (src[n] == np.arange(K)).all() and not kept[n].any(), (shape, kind, t, n)
    return out


def _qualifies(fr, t):
    """The even-aligned pair (t, t + 1) is one the pair path commits."""
    return (t % 2 == 0 and "steady" in fr.get(t, ()) and "relation" not in fr.get(t, ())
            and "steady" in fr.get(t + 1, ()))


def _check_entries_with_mass(act, exp, what):
    """_check_search on the beam entries that carry mass.  With two live classes an utterance of T <= 3 frames
    has fewer than K prefixes of positive mass (at most 2, 4 and 7 of them); the rest of its beam is whatever
    the top-k makes of candidates that all have mass 0, ties the reference leaves unspecified (ctc_search.hip:
    the tie policy).  The beam is sorted by mass, so the entries with mass are each utterance's first columns:
    those are held against the oracle by its rules, and the others must carry no mass here either."""
    y, yl, yp = (x.cpu() for x in act)
    ey, eyl, eyp = exp
    assert y.shape == ey.shape and yl.shape == eyl.shape and yp.shape == eyp.shape, what
    for n in range(eyp.shape[0]):
        kc = int((eyp[n] > 0).sum())
        assert kc > 0 and (eyp[n, :kc] > 0).all() and not (yp[n, kc:] > 0).any(), (what, n)
        _check_search((y[:, n : n + 1, :kc], yl[n : n + 1, :kc], yp[n : n + 1, :kc]),
                      (ey[:, n : n + 1, :kc], eyl[n : n + 1, :kc], eyp[n : n + 1, :kc]), (what, n))


def _run_both(x, lens):
    outs = []
    for two in (1, 0):
        with switches.override(PDT_CTC_TWOFRAME=two):
            outs.append(F.ctc_prefix_search(x, K, lens))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pairs_same_bits_and_the_oracles_answer(device, shape, kind):
    T, N, _ = SHAPES[shape]
    lg, lens = _input(shape, kind), _lens(shape)
    x = torch.from_numpy(np.ascontiguousarray(lg)).to(device)
    tl = None if lens is None else torch.from_numpy(lens).to(device)
    on, off = _run_both(x, tl)
    for name, p, q in zip(("y", "y_lens", "y_probs"), on, off):
        assert torch.equal(p, q), (shape, kind, name)
    # The oracle, under test_decoding_gpu's rules.  Unpeaked rows (flat, peak4) lose mass fast -- float32 masses
    # are denormal and then 0 well before frame 70, where the reference's top-k orders nothing but ties -- so
    # those two inputs are compared over their first 16 frames, as in test_ctc_steady_gpu.py
    if kind in ("flat", "peak4"):
        cap = 16
        lens_c = np.full(N, min(cap, T)) if lens is None else np.minimum(lens, cap)
        act = F.ctc_prefix_search(x[:cap].contiguous(), K, torch.from_numpy(lens_c).to(device))
        _check_search(act, _expected(shape, kind, cap), (shape, kind))
    elif kind == "two_classes" and T <= 3:
        _check_entries_with_mass(on, _expected(shape, kind, None), (shape, kind))
    else:
        _check_search(on, _expected(shape, kind, None), (shape, kind))


def test_the_bench_input_holds_the_pairs_the_path_is_for():
    """A case that never reaches the path proves nothing.  The headline case must hold a qualifying pair, one
    that ends on a checkpoint, and a pair whose first frame is steady and whose second is not."""
    for shape in ("t70", "t69"):
        T, N, _ = SHAPES[shape]
        frames = _frames_cpu(shape, "bench")
        pairs = [(n, t) for n in range(N) for t in range(0, T - 1, 2) if _qualifies(frames[n], t)]
        on_ckpt = [(n, t) for n, t in pairs if (t + 2) % CKPT == 0]
        first_only = [(n, t) for n in range(N) for t in range(0, T - 1, 2)
                      if "steady" in frames[n].get(t, ()) and "relation" not in frames[n].get(t, ())
                      and t + 1 in frames[n] and "steady" not in frames[n][t + 1]]
        print(shape, "qualifying pairs", len(pairs), "of", N * (T // 2), "| ending on a checkpoint", on_ckpt,
              "| first steady, second not", first_only)
        assert len(pairs) >= N * (T // 2) // 2, (shape, len(pairs))
        assert on_ckpt, shape
        assert first_only, shape
    # one pair at T = 2 and T = 3 can qualify only if frame 0 starts with a full beam: it does not (one
    # prefix), so those shapes check the loop's bounds, not the path
    assert not any(_frames_cpu("t3", "bench")[n].get(0) for n in range(5))


@pytest.mark.parametrize("shape", ["t70", "t69", "ragged"])
def test_every_doctored_utterance_has_its_property_in_its_frame(shape):
    frames = _frames_cpu(shape, "doctored")
    sec, rel, bnd = frames[SECOND], frames[RELATION], frames[BOUND]
    print(shape, "second:", D, sorted(sec[D]), D + 1, sorted(sec[D + 1]), "| relation:", D, sorted(rel[D]),
          "| bound:", 2, sorted(bnd[2]), 3, sorted(bnd[3]))
    assert "steady" in sec[D] and "relation" not in sec[D] and "steady" not in sec[D + 1]
    assert "relation" in rel[D]
    assert {"steady", "short", "relation"} <= bnd[3] and "relation" in bnd[2]
    # ... and beside their doctored frames they are the bench's distribution at its steadiest
    T = SHAPES[shape][0]
    for fr in (sec, rel):
        assert sum(_qualifies(fr, t) for t in range(0, T - 1, 2)) >= T // 4
