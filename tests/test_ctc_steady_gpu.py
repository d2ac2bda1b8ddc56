"""The steady tier of the CTC search (csrc/ctc_frame.hpp): a frame whose K best extensions are the beam's
own row of "best available extension" candidates, already in rank order and strictly above everything
else, is decided without the lean tier's 64-key sort.  PDT_CTC_STEADY=0 switches the tier off without
changing the kernel instance, so every case runs the same launch twice: the outputs must be the same
bits, and the default setting must give the oracle's answer under the rules of test_decoding_gpu.py.

The tier is compiled into the shared-list searches (ctc_search.hip: the constant-shape instance, the
width-16 and general short-row instances; ctc_rowreg.hip: rows in registers) -- not into the step
functions or the bigram-table search, which is why there are no cases for those here.
"""
import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import switches
from test_decoding_gpu import _check_search

pytestmark = pytest.mark.gpu

# (V, K, T, N, ragged): the benchmarked instance (T = 70 crosses the 32-frame checkpoints at 32 and 64 and is
# odd-sized for a producer that takes two frames per pass; N = 5 leaves the last workgroup an idle
# utterance), the same with ragged lengths, the width-16 and the general short-row instances, register rows
SHAPES = {
    "headline": (256, 16, 70, 5, False),
    "ragged": (256, 16, 70, 5, True),
    "v300": (300, 16, 70, 5, False),
    "v40k8": (40, 8, 70, 5, False),
    "rowreg": (1000, 16, 40, 3, False),
}
INPUTS = ["bench", "runs", "blank", "tied", "flat", "two_classes", "peak4"]
# utterance of input "tied" whose two best prefixes carry equal masses from frame 0 on
TIED = 1


def _logits(kind, V, T, N, seed):
    rng = np.random.default_rng(seed)
    lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
    peak = rng.integers(0, V + 1, (T, N, 1))
    if kind == "bench":  # bench.py's distribution: N(0, 1) + 12 on a uniformly drawn class, blank included
        np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 12.0, 2)
    elif kind == "peak4":  # challengers win often: steady and lean frames alternate
        np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 4.0, 2)
    elif kind == "runs":  # the peak repeated for 2-4 frames: the last-token stream and the non-extension win
        t = 0
        while t < T:
            r = int(rng.integers(2, 5))
            peak[t : t + r] = peak[t]
            t += r
        np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 12.0, 2)
    elif kind == "blank":  # blank peaks in 80 % of the frames
        peak = np.where(rng.random((T, N, 1)) < 0.8, V, peak)
        np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 12.0, 2)
    elif kind == "tied":
        # utterance TIED: classes 3 and 7 share the peak logit of frame 0, and no later peak is either of them
        # or the blank, so prefixes (3) and (7) and their descendants carry equal masses in every frame
        peak[:, TIED] = 8 + peak[:, TIED] % (V - 8)
        np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 12.0, 2)
        lg[0, TIED, :] = rng.normal(size=V + 1).astype(np.float32)
        lg[0, TIED, 3] = lg[0, TIED, 7] = 12.0
    elif kind == "flat":
        pass
    elif kind == "two_classes":
        # all but two classes masked: fewer than K candidates with any mass.  Utterance 0: one token and the
        # blank (its t + 1 prefixes fill the beam only after K frames), the others two tokens each
        keep = np.zeros((N, V + 1), bool)
        for n in range(N):
            c = rng.choice(V, 2, replace=False)
            keep[n, c[0]] = True
            keep[n, V if n == 0 else c[1]] = True
        lg[:, ~keep] = -np.inf
    else:
        raise ValueError(kind)
    return lg


def _bucket(mass):
    """The rounded key of the lean tier's sort: float32 bits + 1, rounded up to a multiple of 64."""
    key = np.asarray(mass, np.float32).view(np.uint32).astype(np.int64) + 1
    return (key + 63) >> 6


def _steady_frames_cpu(lg, K):
    """Frame by frame through the oracle's step function.  Returns (full, steady): per utterance, the
    frames that start with a full beam (K prefixes with mass), and those of them in which the new beam is
    the old one extended in place -- next_src == arange(K), no winner a non-extension -- with the new
    masses in strictly descending buckets of the rounded sort (what the tier asks for)."""
    T, N, V1 = lg.shape
    V = V1 - 1
    e = np.exp(lg - lg.max(2, keepdims=True))
    probs = (e / e.sum(2, keepdims=True)).astype(np.float32)
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y = np.zeros((0, N, 1), np.int64)
    y_lens = y_last = np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    full, steady = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(T):
        nonext, blank = np.ascontiguousarray(probs[t, :, :V]), np.ascontiguousarray(probs[t, :, V])
        Kp = nb.shape[1]
        ext = np.ascontiguousarray(np.broadcast_to(nonext[:, None, :], (N, Kp, V)))
        had_full = (Kp == K) & ((nb + b) > 0).all(1)
        y, y_last, y_lens, (nb, b), isp, src, kept = oracle.ctc_prefix_search_advance(
            (ext, nonext, blank), K, (nb, b), y, y_last, y_lens, isp
        )
        bk = _bucket(nb + b)
        ok = (src == np.arange(K)[None]).all(1) & ~kept.any(1) & (bk[:, :-1] > bk[:, 1:]).all(1)
        full += had_full
        steady += had_full & ok
    return full, steady


def _run_both(x, K, lens):
    outs = []
    for steady in (1, 0):
        with switches.override(PDT_CTC_STEADY=steady):
            outs.append(F.ctc_prefix_search(x, K, lens))
    return outs


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_steady_tier_same_bits_and_the_oracles_answer(device, shape, kind):
    V, K, T, N, ragged = SHAPES[shape]
    seed = 1000 * list(SHAPES).index(shape) + INPUTS.index(kind)
    lg = _logits(kind, V, T, N, seed)
    lens = np.random.default_rng(seed + 77).integers(0, T + 1, N) if ragged else None
    x = torch.from_numpy(lg).to(device)
    tl = None if lens is None else torch.from_numpy(lens).to(device)
    on, off = _run_both(x, K, tl)
    for name, p, q in zip(("y", "y_lens", "y_probs"), on, off):
        assert torch.equal(p, q), (shape, kind, name)
    # The oracle, under test_decoding_gpu's rules (tokens and lengths exact, probabilities within its RTOL).
    # Unpeaked rows lose mass fast: the best class of a flat N(0, 1) row of 257 has p ~ 0.04 and a peak of
    # + 4 there p ~ 0.11 (0.03 among 1001), so float32 masses are denormal and then 0 well before frame 70,
    # where the reference's top-k orders nothing but ties (ctc_search.hip: the consumer's underflow exit).
    # The comparison of those two inputs therefore stops after 16 frames (masses of 1e-25 and above);
    # everything else is compared in full.
    if kind in ("flat", "peak4"):
        cap = 16
        lens_c = np.full(N, cap) if lens is None else np.minimum(lens, cap)
        act = F.ctc_prefix_search(x[:cap].contiguous(), K, torch.from_numpy(lens_c).to(device))
        _check_search(act, oracle.ctc_prefix_search(lg[:cap], K, lens_c), (shape, kind))
    else:
        _check_search(on, oracle.ctc_prefix_search(lg, K, lens), (shape, kind))


def test_the_inputs_reach_the_steady_tier_and_the_tied_utterance_never_does():
    """A case that never enters the tier proves nothing: on the bench's distribution at the headline
    shape, at least half of the frames that start with a full beam must be order-preserving (a CPU run
    of the reference over T = 512 gives 0.66 for frames 0-31 and 0.88 for 32-63, so ~0.77 is expected
    at T = 70; 0.5 leaves room for the seed).  And the utterance built to carry two equal masses must
    have no such frame: its buckets tie in every one, so the tier may never decide it."""
    V, K, T, _, _ = SHAPES["headline"]
    full, steady = _steady_frames_cpu(_logits("bench", V, T, 8, INPUTS.index("bench")), K)
    print("bench input: full-beam frames", full.tolist(), "order-preserving", steady.tolist())
    assert full.sum() >= 8 * (T - 2)
    assert steady.sum() >= 0.5 * full.sum(), (steady.sum(), full.sum())
    full, steady = _steady_frames_cpu(_logits("tied", V, T, 5, INPUTS.index("tied")), K)
    print("tied input: full-beam frames", full.tolist(), "order-preserving", steady.tolist())
    assert full[TIED] >= T - 2 and steady[TIED] == 0, (full.tolist(), steady.tolist())
    assert steady.sum() > 0  # (the other utterances of that input do reach it)
