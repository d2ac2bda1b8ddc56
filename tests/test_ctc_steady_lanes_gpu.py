"""The steady tier of the CTC search (csrc/ctc_frame.hpp), decided in the beam's own 16 lanes in front
of the lean tier's 64-lane layout.

Lane k forms the four candidates of prefix k from its own registers -- key0 / key1, the masses of its
first two AVAILABLE list entries (the frame's tokens by descending probability, without the prefix's own
last token and without the tokens that lead to a child of the prefix that is in the beam already); key2,
the last-token stream b * p[last]; key3, the non-extension -- and the frame is steady when lanes 0 .. K-1
hold a real key0 each, the key0 do not increase with the lane, and key0[K-1] is strictly above every
key1, key2 and key3 (test_ctc_steady_ties_gpu.py has the rule and why ties inside the beam pass).  What
moving the test in front of the layout newly risks is that one of these per-lane values is not what the
layout would have held, so here one utterance per input is doctored so that ONE term of the test fails in
a known frame -- a kernel with that term wrong gives another verdict there, and the two settings differ:

  order     the key0 out of lane order, nothing else: lane 0 may not take its own last token, and its
            second-best token puts it below lane 1
  row1      a second entry (key1) above the K-th key0 ...
  row1_eq   ... and exactly AT it: all K masses equal and two classes share the peak logit
  stream1   the last-token stream (key2) above the K-th key0, nothing else
  stream2   the non-extensions (key3) above the K-th key0, nothing else
  hole      a steady frame in which parents sit beside their children by the frame's second-best token:
            their second available entry is not the list's second
  short     a steady frame in which a prefix has ONE list entry left, so that where the producer hands
            over a short list (V > 64, lists in LDS) its second entry is hidden and key1 is the upper
            bound with its + 1

order, stream1, stream2, hole and short are built on a FLAT beam in the utterance's first frames (K
prefixes one per cent apart): on the bench's own distribution the masses span four orders of magnitude,
and whatever disturbs a frame lets the best prefixes' second entries pass the K-th key0 as well, so no
term but key1 can fail alone there.  row1 and row1_eq are on the bench's distribution.

The bound of `short` cannot be made the ONLY failing term: a prefix loses list entries only to its own
last token and to its children in the beam, every child's non-extension takes the parent's mass times the
child's token (the merge), and the bound is the parent's mass times the list's LAST probability -- so
whenever the bound reaches the K-th key0, a child's key3 does too.  The input therefore has the bound in
play under the K-th key0, in a frame the tier decides.  That the kernel forms the bound in that frame, and
in no other, was read off the -DPDT_STATS build (counter 17: 1 for the headline, ragged and V = 300
inputs, whose lists come short; the other two shapes get complete lists and no bound).

Every case runs the same launch with PDT_CTC_STEADY=1 and 0 -- the outputs must be the same bits -- and,
on the tie-free inputs, the default setting against the oracle under the rules of test_decoding_gpu.py.

The CPU side (no GPU needed) restates the four keys on the oracle's step function, frame by frame, and
asserts for every shape that the reason's term is the only one that fails in its frame (hole, short: that
the frame is steady and has the feature), and that the bench-like utterances beside it reach the tier in
more than half of their full-beam frames.  An input that does not exercise its reason fails that test.
The model's verdict is also checked against the oracle's own step: a frame the model calls steady must
leave the beam extended in place.  (The model reads the oracle's float32 probabilities; the kernel's
differ from them in the last place, which moves no doctored frame: the narrowest margin is the one per
cent between neighbouring prefixes, and the equality case is equal by construction -- equal masses times
equal probabilities -- in any rounding.)  The model knows nothing of the length of a short list, which the
producer chooses by a threshold it adapts from frame to frame: its `short` flag says that a list of the
shortest length the producer may hand over would hide a prefix's second entry.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import switches
from test_decoding_gpu import _check_search

# (V, K, T, N, ragged): shapes of test_ctc_steady_gpu.py -- the benchmarked instance (T = 70 crosses the
# checkpoints at 32 and 64, N = 5 leaves the last workgroup an idle utterance), the same with ragged
# lengths, the width-16 instance, the general short-row instance with a narrower beam (its frame 0 has
# K' = 1 < K), rows in registers
SHAPES = {
    "headline": (256, 16, 70, 5, False),
    "ragged": (256, 16, 70, 5, True),
    "v300": (300, 16, 70, 5, False),
    "v40k8": (40, 8, 70, 5, False),
    "rowreg": (1000, 16, 40, 3, False),
}
REASONS = ["order", "row1", "row1_eq", "stream1", "stream2", "hole", "short"]
TIED = ("row1_eq",)  # inputs with exact ties: compared between the two settings only
DOC = 1  # the doctored utterance
FLAT = ("order", "stream1", "stream2", "hole")  # reasons isolated on a flat beam, in the utterance's first frames
SHORT_MIN = 8  # the shortest list a producer hands over (csrc/ctc_ring.hpp)


def _doc_frames(T):
    """The frames doctored for a reason: two places, so that a ragged length still leaves one."""
    return [T // 4 + 2, T // 2 + 4]


@functools.lru_cache(maxsize=None)
def _logits(kind, shape):
    V, K, T, N, _ = SHAPES[shape]
    rng = np.random.default_rng(9000 + 100 * list(SHAPES).index(shape) + REASONS.index(kind))
    lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
    peak = rng.integers(0, V + 1, (T, N, 1))
    # utterance DOC: peaks among the tokens K + 4 .. V - 1, never the blank and never the previous
    # frame's, so outside the doctored frames it is the bench's distribution at its steadiest
    first = K + 4
    pk = first + peak[:, DOC, 0] % (V - first)
    for t in range(1, T):
        if pk[t] == pk[t - 1]:
            pk[t] = first + (pk[t] - first + 1) % (V - first)
    peak[:, DOC, 0] = pk
    np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 12.0, 2)
    u, w = 1, 2  # two tokens no peak of DOC uses

    def row():
        return rng.normal(size=V + 1).astype(np.float32)

    def put(t, probs):
        """Frame t of DOC: N(0, 1) noise with the classes of `probs` at logit 12 + log(probability) -- next to
        them the noise is 0.3 % of the row, so they come out at these shares of it."""
        r = row()
        for c, q in probs.items():
            r[c] = np.float32(12.0 + np.log(q))
        lg[t, DOC] = r

    if kind in FLAT:
        # A FLAT beam, on which one term of the test can fail by itself.  (On the bench's distribution the
        # beam's masses span four orders of magnitude, and whatever disturbs a frame lets the best
        # prefixes' second entries pass the K-th first entry as well.)  Frame 0: K tokens a_0 .. a_{K-1} one
        # per cent apart, everything else noise -- the beam is (a_0) .. (a_{K-1}) in this order, mass t_i,
        # t_0 / t_{K-1} = e^{0.01 (K - 1)}, all distinct.
        a0 = 3
        r = row()
        r[a0 : a0 + K] = 12.0 - 0.01 * np.arange(K, dtype=np.float32)
        lg[0, DOC] = r
        low = a0 + K - 1  # the token of the lowest prefix
        if kind == "stream2":
            # frame 1: blank 0.6, one token 0.39 -- every first entry 0.39 t_k in order, every second entry
            # and stream 1 next to nothing, every non-extension 0.6 t_k: key3 alone is at or above the K-th key0
            put(1, {V: 0.6, u: 0.39})
        elif kind in ("order", "stream1"):
            # frame 1: blank 0.55 and the LOWEST prefix's own token 0.35: all K prefixes stay (0.55 t_k; the best
            # extension is 0.35 t_0 < 0.55 t_{K-2}), the lowest one with 0.9 t_{K-1}, of it 0.35 in nb and 0.55 in b
            # -- it is lane 0 now, the others follow in their order.
            put(1, {V: 0.55, low: 0.35})
            if kind == "order":
                # frame 2: that token again at c, a token e at 0.5 c.  Lane 0 may not take its own last token:
                # key0 = 0.5 c 0.9 t_{K-1}, below lane 1's c 0.55 t_0 -- out of order.  Everything else holds: the
                # second entries are 0.5 c 0.55 t_k, lane 0's stream 1 is c 0.55 t_{K-1} and its non-extension
                # c 0.35 t_{K-1}, all below the K-th key0 = c 0.55 t_{K-2} (stream 1 by the one per cent of frame 0)
                put(2, {low: 0.66, u: 0.33})
            else:
                # frame 2: the blank -- lane 0's mass is all in b now; frame 3: its token at c, e at 0.78 c.  Lane 0's
                # key0 = 0.78 c 0.9 t_{K-1} stays above lane 1's c 0.55 t_0, the second entries 0.78 c 0.55 t_k stay
                # below the K-th key0 = c 0.55 t_{K-2}, lane 0's non-extension is the blank's share -- and its
                # stream 1, c 0.9 t_{K-1}, is above the K-th key0: key2 alone
                put(2, {V: 0.997})
                put(3, {low: 0.56, u: 0.56 * 0.78})
        elif kind == "hole":
            # frame 1: blank 0.5, token w half the beam's spread below it (and off every tie) -- the stays 0.5 t_k
            # and the extensions by w interleave, so the beam holds parents P next to their children P + w;
            # frame 2: a peak with w second (0.04): a
            # parent's second available entry is not the list's second, its child takes the parent's share of w
            # into its non-extension, and nothing of that comes near the K-th key0 -- a steady frame, decided on
            # the parents' real entries
            put(1, {V: 0.5, w: 0.5 * float(np.exp(-0.005 * (K - 1) - 0.0005))})
            put(2, {int(pk[2]): 0.95, w: 0.04})
    # (the second doctored place uses other offsets than the first: with the same ones, "the blank here and the
    # peak there" and its mirror image would be two prefixes of equal mass but for rounding, and the oracle's
    # order of such a pair is not the kernel's to reproduce -- INTEGRATION.md, "Near ties")
    for i, t0 in enumerate(_doc_frames(T)):
        d = np.float32(0.4 * i)
        if kind == "row1":
            # two tokens nearly share the peak: the best prefixes' second entries beat the K-th first entry
            r = row()
            r[pk[t0]] += 12.0
            r[u] = r[pk[t0]] - 0.25 - d / 2
            lg[t0, DOC] = r
    if kind == "short":
        # A prefix with ONE list entry left.  Frame 0: blank 0.5 and K - 1 tokens one per cent apart share the
        # rest -- the beam is the empty prefix and its K - 1 one-token children; frame 1: the blank, all stay;
        # frame 2: those K - 1 tokens again, e^-3.5 below one new token u, over noise of a third of the usual
        # spread, so that the threshold the producer carries over from frame 1's noise falls between the noise and
        # the K tokens and the short list is exactly these K.  The empty prefix has u alone available: its second
        # entry is hidden, key1 is the bound 0.5 p[last entry] + 1.  It stays under the K-th key0 (0.03 p[u]), as
        # do the children's non-extensions (the parent's 0.5 times their token): a steady frame with the bound in it.
        a0 = 3
        put(0, {V: 0.5, **{a0 + i: 0.03 * float(np.exp(-0.01 * i)) for i in range(K - 1)}})
        put(1, {V: 0.997})
        r = (0.3 * rng.normal(size=V + 1)).astype(np.float32)
        r[a0 : a0 + K - 1] = 8.5
        r[u] = 12.0
        lg[2, DOC] = r
    if kind == "row1_eq":
        # frame 0: K + 1 classes share the top logit -- all K beam masses are equal; frame 1: two classes
        # share the peak -- every key0 and every key1 is the same number (the `edge` input of
        # test_ctc_steady_ties_gpu.py)
        r = row()
        r[: K + 1] = 12.0
        lg[0, DOC] = r
        r = row()
        r[[first + 1, first + 4]] = 12.0
        lg[1, DOC] = r
    lg.setflags(write=False)
    return lg


def _lens(shape):
    V, K, T, N, ragged = SHAPES[shape]
    if not ragged:
        return None
    lens = np.random.default_rng(78).integers(0, T + 1, N)
    lens[DOC] = T - 3  # (the doctored utterance keeps nearly all of its frames)
    return lens


@functools.lru_cache(maxsize=None)
def _expected(kind, shape):
    return oracle.ctc_prefix_search(_logits(kind, shape), SHAPES[shape][1], _lens(shape))


@functools.lru_cache(maxsize=None)
def _frames_cpu(kind, shape):
    """Frame by frame through the oracle's step function, the steady tier's four keys restated on the
    state in front of each frame.  Returns per utterance a list of (t, flags) for the frames that start
    with a full beam; flags: the conditions that FAIL ('order', 'row1', 'row1_eq', 'stream1', 'stream2',
    'tiny': the K-th mass in the lowest bucket), the features 'hole' and 'short', and 'steady' when none
    fails."""
    lg = _logits(kind, shape)
    V, K, T, N, _ = SHAPES[shape]
    e = np.exp(lg - lg.max(2, keepdims=True))
    probs = (e / e.sum(2, keepdims=True)).astype(np.float32)
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y = np.zeros((0, N, 1), np.int64)
    y_lens = y_last = np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    out = [[] for _ in range(N)]
    f32 = np.float32
    for t in range(T):
        nonext, blank = np.ascontiguousarray(probs[t, :, :V]), np.ascontiguousarray(probs[t, :, V])
        Kp = nb.shape[1]
        full = (Kp == K) & ((nb + b) > 0).all(1)
        verdicts = {}
        for n in np.nonzero(full)[0]:
            p, pb = nonext[n], blank[n]
            order = np.lexsort((np.arange(V), -p))  # by descending probability, lowest token first
            M = min(V, 2 * K)
            lens_n, last_n = y_lens[n], y_last[n]
            pref = [tuple(y[: lens_n[k], n, k]) for k in range(K)]
            tot = nb[n] + b[n]
            key0, key1, key2, key3 = (np.zeros(K, f32) for _ in range(4))
            flags = set()
            for k in range(K):
                lk = min(max(int(last_n[k]), 0), V - 1) if lens_n[k] else 0
                kids = {c[-1] for c in pref if len(c) == len(pref[k]) + 1 and c[:-1] == pref[k]}
                par = [q for q in range(K)
                       if lens_n[k] and len(pref[q]) + 1 == len(pref[k]) and pref[k][:-1] == pref[q]]
                av = [v for v in order[:M] if v != lk and v not in kids]
                plain = [v for v in order[:M] if v != lk]
                if av[:2] != plain[:2]:
                    flags.add("hole")
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
            if (key0[:-1] < key0[1:]).any():
                flags.add("order")
            if key1.max() >= kth:
                flags.add("row1")
            if key1.max() == kth:
                flags.add("row1_eq")
            if key2.max() >= kth:
                flags.add("stream1")
            if key3.max() >= kth:
                flags.add("stream2")
            if kth.view(np.uint32) + 1 <= 64:
                flags.add("tiny")
            if not flags & {"order", "row1", "stream1", "stream2", "tiny"}:
                flags.add("steady")
            verdicts[n] = flags
            out[n].append((t, frozenset(flags)))
        ext = np.ascontiguousarray(np.broadcast_to(nonext[:, None, :], (N, Kp, V)))
        y, y_last, y_lens, (nb, b), isp, src, kept = oracle.ctc_prefix_search_advance(
            (ext, nonext, blank), K, (nb, b), y, y_last, y_lens, isp
        )
        for n, flags in verdicts.items():  # the model against the oracle's own step
            if "steady" in flags:
                assert (src[n] == np.arange(K)).all() and not kept[n].any(), (kind, shape, t, n)
    return out


def _run_both(x, K, lens):
    outs = []
    for steady in (1, 0):
        with switches.override(PDT_CTC_STEADY=steady):
            outs.append(F.ctc_prefix_search(x, K, lens))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", REASONS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_reason_at_a_time_same_bits_and_the_oracles_answer(device, shape, kind):
    V, K, T, N, ragged = SHAPES[shape]
    lg, lens = _logits(kind, shape), _lens(shape)
    x = torch.from_numpy(lg).to(device)
    tl = None if lens is None else torch.from_numpy(lens).to(device)
    on, off = _run_both(x, K, tl)
    for name, p, q in zip(("y", "y_lens", "y_probs"), on, off):
        assert torch.equal(p, q), (shape, kind, name)
    if kind not in TIED:
        _check_search(on, _expected(kind, shape), (shape, kind))


# where each reason must show: the frame itself for the flat-beam inputs, offsets from a doctored frame t0 otherwise
FRAME = {"order": 2, "stream1": 3, "stream2": 1, "hole": 2, "short": 2}
WHERE = {"row1": (0,)}
TERMS = {"order", "row1", "stream1", "stream2", "tiny"}  # the conditions of the test, by the flag of their failure


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_reason_occurs_alone_and_the_other_utterances_reach_the_tier(shape):
    """The counts that make the GPU comparisons mean something, on the CPU model (see the module's text):
    every reason has a frame in which ITS term of the test is the only one that fails."""
    V, K, T, N, _ = SHAPES[shape]
    for kind in REASONS:
        frames = _frames_cpu(kind, shape)
        doc = dict(frames[DOC])
        if kind == "row1_eq":
            hits = [t for t, f in frames[DOC] if "row1_eq" in f]
        elif kind in FRAME:
            hits = [FRAME[kind]] if kind in doc.get(FRAME[kind], ()) else []
        else:
            hits = [t0 + dt for t0 in _doc_frames(T) for dt in WHERE[kind] if kind in doc.get(t0 + dt, ())]
        others = [f for n in range(N) if n != DOC for _, f in frames[n]]
        steady = sum("steady" in f for f in others)
        print(shape, kind, "full-beam frames of the doctored utterance", len(doc), "with the reason",
              [(t, sorted(doc[t])) for t in hits], "| others: steady", steady, "of", len(others))
        assert len(doc) >= T - 6, (shape, kind, len(doc))
        assert hits, (shape, kind)
        if kind in ("hole", "short"):  # these fail nothing by themselves: the tier decides such a frame, on the
            # prefix's real entries (hole) or with the hidden entry's bound among the challengers (short)
            assert any("steady" in doc[t] for t in hits), (shape, kind, [sorted(doc[t]) for t in hits])
        elif kind == "row1_eq":  # (equal masses: the second entries AT the K-th key, nothing else in the way)
            assert any(doc[t] & TERMS == {"row1"} for t in hits), (shape, kind, [sorted(doc[t]) for t in hits])
        else:
            assert any(doc[t] & TERMS == {kind} for t in hits), (shape, kind, [sorted(doc[t]) for t in hits])
        assert 2 * steady > len(others), (shape, kind, steady, len(others))
