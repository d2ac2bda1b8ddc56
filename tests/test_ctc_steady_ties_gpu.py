"""The steady tier of the CTC search (csrc/ctc_frame.hpp) on tied and nearly tied beams.

The tier decides a frame without the lean tier's sort when the beam's own row of "best available
extension" candidates stays where it is.  Since it compares EXACT keys the rule is: lanes 0 .. K-1 hold
real candidates, their keys do not increase in lane order (equal keys allowed), the K-th key is strictly
above every key of the other rows, and it lies above the lowest bucket of the rounded sort (underflowed
masses).  Equal or nearly equal masses inside the beam are in place all the same, because the lean
tier's re-rank orders by exact key and then by the lowest flat candidate index, which grows with the
lane for these candidates; an equal key in another row may have the lower index, so equality there
must send the frame to the sort.  (test_ctc_steady_gpu.py was written for the earlier rule, strictly
descending 64-ulp buckets, under which a tied pair never reached the tier; its CPU model still counts
those frames.)

Every case runs the same launch with PDT_CTC_STEADY=1 and 0 -- the outputs must be the same bits -- and
the default setting against the oracle under the rules of test_decoding_gpu.py.  All inputs are the
bench's distribution with utterance DOC doctored.
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F
from pydrobert_amd import switches
from test_decoding_gpu import _check_search

pytestmark = pytest.mark.gpu

# (V, K, T, N, ragged): the benchmarked instance (T = 70 crosses the checkpoints at 32 and 64, N = 5 leaves
# the last workgroup an idle utterance), the same with ragged lengths, the general short-row instance
# with a narrower beam, rows in registers
SHAPES = {
    "headline": (256, 16, 70, 5, False),
    "ragged": (256, 16, 70, 5, True),
    "v40k8": (40, 8, 70, 5, False),
    "rowreg": (1000, 16, 40, 3, False),
}
INPUTS = ["exact_tie", "near_tie", "run_of_three", "edge", "zero_masses"]
DOC = 1  # the doctored utterance
NEAR_ULPS = 1  # distance of the two peak logits of "near_tie", in float32 ulps of 12.0


@functools.lru_cache(maxsize=None)
def _logits(kind, shape):
    V, K, T, N, _ = SHAPES[shape]
    rng = np.random.default_rng(7000 + 100 * list(SHAPES).index(shape) + INPUTS.index(kind))
    lg = rng.normal(size=(T, N, V + 1)).astype(np.float32)
    peak = rng.integers(0, V + 1, (T, N, 1))
    # utterance DOC: the tied classes are among 0 .. K, and no later peak is one of them or the blank, so
    # the prefixes that start with them and their descendants are extended by the same token, in place, in
    # (nearly) every frame
    first = K + 1
    peak[:, DOC] = first + peak[:, DOC] % (V - first)
    np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + 12.0, 2)
    row0 = rng.normal(size=V + 1).astype(np.float32)
    if kind == "exact_tie":  # two classes share the peak logit of frame 0
        row0[[3, 7]] = 12.0
        lg[0, DOC] = row0
    elif kind == "near_tie":  # the same, NEAR_ULPS apart: unequal masses inside one 64-ulp bucket
        row0[3] = 12.0
        row0[7] = (np.float32(12.0).view(np.uint32) - np.uint32(NEAR_ULPS)).view(np.float32)
        lg[0, DOC] = row0
    elif kind == "run_of_three":
        row0[[2, 3, 7]] = 12.0
        lg[0, DOC] = row0
    elif kind == "edge":
        # frame 0: K + 1 classes share the top logit -- all K beam masses are equal; frame 1: two classes
        # share the peak -- every key of row 0 (best token) and row 1 (second token) is equal, and the
        # right answer gives the lowest prefixes both tokens, not every prefix its first
        row0[: K + 1] = 12.0
        lg[0, DOC] = row0
        row1 = rng.normal(size=V + 1).astype(np.float32)
        row1[[first + 1, first + 4]] = 12.0
        lg[1, DOC] = row1
    elif kind == "zero_masses":  # unpeaked rows: the masses reach 0 (V = 256: before frame 40) and tie there
        lg[:, DOC] = rng.normal(size=(T, V + 1)).astype(np.float32)
    else:
        raise ValueError(kind)
    lg.setflags(write=False)
    return lg


def _lens(shape):
    V, K, T, N, ragged = SHAPES[shape]
    if not ragged:
        return None
    lens = np.random.default_rng(77).integers(0, T + 1, N)
    lens[DOC] = T - 3  # (the doctored utterance keeps nearly all of its frames)
    return lens


@functools.lru_cache(maxsize=None)
def _expected(kind, shape, cap):
    lg, lens = _logits(kind, shape), _lens(shape)
    N = lg.shape[1]
    if cap is not None:
        lens = np.full(N, cap) if lens is None else np.minimum(lens, cap)
        lg = lg[:cap]
    return oracle.ctc_prefix_search(lg, SHAPES[shape][1], lens), lens


def _bucket(mass):
    """The rounded key of the lean tier's sort: float32 bits + 1, rounded up to a multiple of 64."""
    key = np.asarray(mass, np.float32).view(np.uint32).astype(np.int64) + 1
    return (key + 63) >> 6


def _tied_frames_cpu(lg, K):
    """Frame by frame through the oracle's step function.  Returns (full, tied): per utterance, the frames
    that start with a full beam, and those of them in which the new beam is the old one extended in place
    -- next_src == arange(K), no winner a non-extension -- with two or more of the K new masses in one
    bucket of the rounded sort: the frames the tier leaves to the sort under a strict-bucket rule and
    decides under the exact-key rule."""
    T, N, V1 = lg.shape
    V = V1 - 1
    e = np.exp(lg - lg.max(2, keepdims=True))
    probs = (e / e.sum(2, keepdims=True)).astype(np.float32)
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y = np.zeros((0, N, 1), np.int64)
    y_lens = y_last = np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    full, tied = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(T):
        nonext, blank = np.ascontiguousarray(probs[t, :, :V]), np.ascontiguousarray(probs[t, :, V])
        Kp = nb.shape[1]
        ext = np.ascontiguousarray(np.broadcast_to(nonext[:, None, :], (N, Kp, V)))
        had_full = (Kp == K) & ((nb + b) > 0).all(1)
        y, y_last, y_lens, (nb, b), isp, src, kept = oracle.ctc_prefix_search_advance(
            (ext, nonext, blank), K, (nb, b), y, y_last, y_lens, isp
        )
        bk = _bucket(nb + b)
        ok = (src == np.arange(K)[None]).all(1) & ~kept.any(1) & (bk[:, :-1] == bk[:, 1:]).any(1)
        full += had_full
        tied += had_full & ok
    return full, tied


def _run_both(x, K, lens):
    outs = []
    for steady in (1, 0):
        with switches.override(PDT_CTC_STEADY=steady):
            outs.append(F.ctc_prefix_search(x, K, lens))
    return outs


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tied_beams_same_bits_and_the_oracles_answer(device, shape, kind):
    V, K, T, N, ragged = SHAPES[shape]
    lg, lens = _logits(kind, shape), _lens(shape)
    x = torch.from_numpy(lg).to(device)
    tl = None if lens is None else torch.from_numpy(lens).to(device)
    on, off = _run_both(x, K, tl)
    for name, p, q in zip(("y", "y_lens", "y_probs"), on, off):
        assert torch.equal(p, q), (shape, kind, name)
    # The oracle, under test_decoding_gpu's rules.  The unpeaked utterance loses its masses to denormals
    # and then to 0, where the reference's top-k orders nothing but ties: as in test_ctc_steady_gpu.py
    # that input is compared over its first 16 frames, everything else in full.
    if kind == "zero_masses":
        exp, lens_c = _expected(kind, shape, 16)
        act = F.ctc_prefix_search(x[:16].contiguous(), K, torch.from_numpy(lens_c).to(device))
        _check_search(act, exp, (shape, kind))
    else:
        _check_search(on, _expected(kind, shape, None)[0], (shape, kind))


@pytest.mark.parametrize("shape", ["headline", "v40k8", "rowreg"])
def test_the_tied_inputs_are_in_place_with_a_bucket_tie(shape):
    """A tied utterance that is not in place, or whose near tie falls into two buckets, proves nothing
    about the tier: by the CPU model at least half of the doctored utterance's full-beam frames are the
    old beam extended in place with a tie among the new masses' buckets, for the exact and for the near
    tie (and for the other doctored inputs the counts are printed)."""
    V, K, T, N, _ = SHAPES[shape]
    for kind in INPUTS:
        full, tied = _tied_frames_cpu(_logits(kind, shape), K)
        print(shape, kind, "full-beam frames", full.tolist(), "in place with a bucket tie", tied.tolist())
        if kind in ("exact_tie", "near_tie"):
            assert full[DOC] >= T - 4, (shape, kind, full.tolist())
            assert 2 * tied[DOC] >= full[DOC], (shape, kind, tied.tolist(), full.tolist())
