"""Pacing of the CTC search's producer waves (csrc/ctc_ring.hpp: pace_prio; csrc/ctc_search.hip).  A producer of
the one-producer forms takes its `s_setprio` level from its own frame counter -- 2, 1, 0 and round again, one
step per band of 64 frames -- so that a producer that is ahead of the launch issues after those behind it; it
polls at level 0 and takes its band's level again after a wait.  Priorities order issue slots: they cannot
change a result.  PDT_CTC_PACE=0 switches the pacing off inside the same kernel instance, so every case runs
the same launch under both settings: the outputs must be the same bits, and the default setting must give the
oracle's answer under the rules of test_decoding_gpu.py.

The cases are the forms of the two producer loops:

  * the two-frames-per-pass instance (V = 256, K = 16, contiguous float32 rows) at T = 70, N = 5 -- the last
    workgroup has an idle utterance; frame 64 starts the second band -- on inputs whose producer is rarely
    ahead and never waits (`bench`, `tied`: short lists, cheap frames on both sides), or always ahead, waiting
    in every pass (`blank`, `flat`: the consumer's full tiers); an odd tail and the loop's bounds (T = 69, 1, 2,
    3); ragged lengths, where the partners of a workgroup finish far apart;
  * T = 48, N = 1200: 600 workgroups, more than two per CU -- the smallest shape at which waves of different
    age share a SIMD, which is where the levels decide anything.  The two settings are compared on every
    utterance, the first 8 against the oracle;
  * the one-frame producer loop: a general instance (V = 40, K = 8) and the constant-shape instance with
    PDT_CTC_PAIR=0;
  * T = 200 (N = 2) in both loops: the levels 2, 1, 0 and the step back to 2 at frame 192;
  * float16 rows: the element-typed instances of the same loops.  The kernel computes in float32 on the widened
    rows and rounds the probabilities once at the end, so tokens and lengths are held against the oracle on the
    widened rows, the probabilities against the float32 route rounded to float16 (as test_half_logits_gpu.py).

`flat` rows are unpeaked: their float32 masses reach 0 before frame 70, where the reference's top-k orders
nothing but ties, so that input meets the oracle over its first 16 frames, as in test_ctc_twoframe_gpu.py; the
two settings are compared over all 70.

Every test is one ordinary call per setting.
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

pytestmark = pytest.mark.gpu

RAGGED_LENS = np.array([0, 69, 70, 33, 24])
FLAT_CAP = 16
# name -> (V, K, T, N, input, ragged, PDT_CTC_PAIR)
CASES = {
    "t70_bench": (256, 16, 70, 5, "bench", False, 1),
    "t70_blank": (256, 16, 70, 5, "blank", False, 1),
    "t70_tied": (256, 16, 70, 5, "tied", False, 1),
    "t70_flat": (256, 16, 70, 5, "flat", False, 1),
    "t69_bench": (256, 16, 69, 5, "bench", False, 1),
    "t1_bench": (256, 16, 1, 5, "bench", False, 1),
    "t2_bench": (256, 16, 2, 5, "bench", False, 1),
    "t3_bench": (256, 16, 3, 5, "bench", False, 1),
    "ragged_bench": (256, 16, 70, 5, "bench", True, 1),
    "one_frame_v40": (40, 8, 40, 6, "bench", False, 1),
    "one_frame_v256": (256, 16, 33, 4, "bench", False, 0),
    # every level and the step back up to the first (frames 64, 128, 192), in both producer loops
    "t200_bench": (256, 16, 200, 2, "bench", False, 1),
    "one_frame_t200": (40, 8, 200, 2, "bench", False, 1),
}


@functools.lru_cache(maxsize=None)
def _input(name):
    V, K, T, N, kind, _, _ = CASES[name]
    lg = _logits(kind, V, T, N, 1500 + list(CASES).index(name))
    lg.setflags(write=False)
    return lg


def _run_both(x, K, lens):
    outs = []
    for pace in (1, 0):
        with switches.override(PDT_CTC_PACE=pace):
            outs.append(F.ctc_prefix_search(x, K, lens))
    return outs


def _same_bits(on, off, what):
    for name, p, q in zip(("y", "y_lens", "y_probs"), on, off):
        assert torch.equal(p, q), (what, name)


def test_pacing_is_on_by_default():
    assert switches.get("PDT_CTC_PACE") == 1


@pytest.mark.parametrize("name", list(CASES))
def test_paced_and_unpaced_same_bits_and_the_oracles_answer(device, name):
    V, K, T, N, kind, ragged, pair = CASES[name]
    lg = _input(name)
    lens = RAGGED_LENS if ragged else None
    x = torch.from_numpy(np.ascontiguousarray(lg)).to(device)
    tl = None if lens is None else torch.from_numpy(lens).to(device)
    with switches.override(PDT_CTC_PAIR=pair):
        on, off = _run_both(x, K, tl)
        _same_bits(on, off, name)
        if kind == "flat":
            lens_c = np.full(N, FLAT_CAP)
            act = F.ctc_prefix_search(x[:FLAT_CAP].contiguous(), K, torch.from_numpy(lens_c).to(device))
            _check_search(act, oracle.ctc_prefix_search(lg[:FLAT_CAP], K, lens_c), name)
        else:
            _check_search(on, oracle.ctc_prefix_search(lg, K, lens), name)


def test_more_than_two_workgroups_per_cu(device):
    V, K, T, N, first = 256, 16, 48, 1200, 8
    lg = _logits("bench", V, T, N, 1599)
    x = torch.from_numpy(lg).to(device)
    on, off = _run_both(x, K, None)
    _same_bits(on, off, "n1200")
    head = tuple(o[..., :first, :] if o.dim() == 3 else o[:first] for o in on)
    _check_search(head, oracle.ctc_prefix_search(np.ascontiguousarray(lg[:, :first]), K), "n1200")


def test_more_workgroups_than_the_device_holds(device):
    """Only a launch whose whole grid is resident is paced (csrc/ctc_search.hip: launch_ctc_search_p).  2100
    workgroups are more than 256 CUs hold at eight each, so the default setting takes the unpaced path of the
    same instance here: same bits as PDT_CTC_PACE=0, and the oracle's answer on the first and last utterances."""
    V, K, T, N, edge = 256, 16, 6, 4200, 4
    lg = _logits("bench", V, T, N, 1597)
    x = torch.from_numpy(lg).to(device)
    on, off = _run_both(x, K, None)
    _same_bits(on, off, "n4200")
    for sel in (slice(0, edge), slice(N - edge, N)):
        part = tuple(o[:, sel] if o.dim() == 3 else o[sel] for o in on)
        _check_search(part, oracle.ctc_prefix_search(np.ascontiguousarray(lg[:, sel]), K), ("n4200", sel))


def test_float16_rows(device):
    V, K, T, N = 256, 16, 33, 4
    lg = _logits("bench", V, T, N, 1598).astype(np.float16)
    x = torch.from_numpy(lg).to(device)
    on, off = _run_both(x, K, None)
    _same_bits(on, off, "float16")
    wide = F.ctc_prefix_search(x.float(), K)
    assert on[2].dtype == torch.float16 and torch.equal(on[2], wide[2].to(torch.float16))
    _check_search((on[0], on[1], wide[2]), oracle.ctc_prefix_search(lg.astype(np.float32), K), "float16")
