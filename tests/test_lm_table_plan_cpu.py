"""CPU: the host plans of the two one-call CTC searches with an n-gram model, swept without a launch.

csrc/ctc_lm_table.hip decides its LDS layout, checkpoint spacing and kernel instance in one host function
(pdt_ctc_lm_table_search_plan; pdt_ctc_lm_table_search_workspace_bytes goes through it).  The spacing used
to come from a loop that doubled it until the output walk's checkpoint table fitted the row ring -- and never
ended when the ring of a tiny vocabulary was narrower than ONE row of that table (12 * ((V + 4) & ~3) <
8 * W: V = 3 at width 8, V = 7 at 16, V = 19 at 32).  Here every call must return; every shape whose loop
ended keeps the spacing, count, instance and workspace it had (the old arithmetic, restated below); the rest
get a ring with room for one row and a single checkpoint.

csrc/ctc_lm_step.hip: the largest vocabulary whose rows fit a workgroup's LDS, per width
(pdt_ctc_lookup_lm_search_lds_bytes), against the plan's arithmetic restated; none reaches the 32 768 tokens
from which a history slot would need more than 16 bits."""
import ctypes
import os

import pytest

EDGES = [511, 512, 1023, 1024, 2047, 2048, 3071, 3072, 5119]
FRAMES = [0, 1, 31, 32, 33, 1000, 2**24 - 1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def _plan(lib, T, V, W):
    out = (ctypes.c_int32 * 6)()
    rc = lib.pdt_ctc_lm_table_search_plan(T, V, W, out)
    return rc, tuple(out)


def _old_plan(T, V, W):
    """(shift, checkpoints, chunks of the instance, constant width) as the launch computed them before the plan
    was one function; None where its loop did not end."""
    ring = 12 * ((V + 4) & ~3)
    if ring < 8 * W:
        return None
    sh = 5
    while ((T >> sh) + 1) * W * 8 > ring:
        sh += 1
    chunks = (V + 1 + 63) // 64
    nr = next(n for n in (8, 16, 32, 48, 80) if chunks <= n)
    return sh, (T >> sh) + 1, nr, 16 if W == 16 else 0


def test_table_search_plan_returns_for_every_shape_and_keeps_what_ended(lib):
    from pydrobert_amd import _cabi

    never_ended = set()
    for V in list(range(1, 101)) + EDGES:
        for W in range(1, 33):
            for T in FRAMES:
                rc, plan = _plan(lib, T, V, W)
                assert rc == _cabi.PDT_OK, (T, V, W, rc)
                shift, count, nr, wc, ring, lds = plan
                # the output walk's table fits the ring it overlays; the checkpoints fit the workspace
                assert 5 <= shift <= 24 and count == (T >> shift) + 1 and count * W * 8 <= ring, (T, V, W, plan)
                assert count <= T // 32 + 1 and ring >= 12 * ((V + 4) & ~3) and lds <= 160 * 1024, (T, V, W, plan)
                old = _old_plan(T, V, W)
                if old is None:
                    never_ended.add((V, W))
                    assert count == 1 and ring == (8 * W + 15) & ~15, (T, V, W, plan)
                    assert shift == max(5, T.bit_length()), (T, V, W, plan)  # the smallest that leaves one row
                else:
                    assert plan[:4] == old and ring == 12 * ((V + 4) & ~3), (T, V, W, plan, old)
                for N in (0, 1, 5):
                    ws = lib.pdt_ctc_lm_table_search_workspace_bytes(T, N, V, W)
                    assert ws == (((T + T // 32 + 1) * N * W * 8 + 255) & ~255) + 16, (T, N, V, W, ws)
    # the shapes of the report, and their neighbours that always ended
    assert {(3, 8), (7, 16), (19, 32), (2, 32)} <= never_ended
    assert not {(4, 8), (8, 16), (20, 32)} & never_ended
    assert all(V < 20 for V, _ in never_ended)


def test_table_search_plan_refuses_what_the_search_does_not_take(lib):
    from pydrobert_amd import _cabi

    size = lib.pdt_ctc_lm_table_search_workspace_bytes
    for T, V, W, rc in [(12, 5120, 8, _cabi.PDT_E_TOO_LONG), (12, 100, 33, _cabi.PDT_E_TOO_LONG),
                        (2**24, 100, 1, _cabi.PDT_E_TOO_LONG), (2**27, 100, 32, _cabi.PDT_E_TOO_LONG),
                        (-1, 100, 8, _cabi.PDT_E_ARG), (12, 0, 8, _cabi.PDT_E_ARG), (12, 100, 0, _cabi.PDT_E_ARG)]:
        assert _plan(lib, T, V, W)[0] == rc, (T, V, W)
        assert size(T, 4, V, W) == 0, (T, V, W)
    assert size(12, -1, 100, 8) == 0
    assert lib.pdt_ctc_lm_table_search_plan(12, 100, 8, None) == _cabi.PDT_E_ARG
    # the launch itself gives the same answers before anything touches a device (made-up non-null pointers)
    def search(T, V, W):
        return lib.pdt_ctc_lm_table_search(1, T, 2, V, 1, 1, 1, 0, W, T, 1, 1, V + 1, V, V, V + 1, 1, 0.3, 0, 1, 1, 1, 1, 0)

    assert search(12, 5120, 8) == _cabi.PDT_E_TOO_LONG
    assert search(12, 100, 33) == _cabi.PDT_E_TOO_LONG
    assert search(2**24, 100, 1) == _cabi.PDT_E_TOO_LONG


def _old_search_lds(V, W):
    """plan_lm_frame of csrc/ctc_lm_step.hip for the widest frame (K' = W), restated: 0 when the rows do
    not fit 160 KB with one wave per element."""
    frame_lds = 64 * 8 + W * 64 * 8 + W * 4 + 2 * W * 4  # FrameLds::bytes(V, W, W, dense)
    frame = (((V + 4) & ~3) * 4 + ((frame_lds + 15) & ~15) + 15) & ~15
    row = (V + 3) & ~3

    def lds(nw):
        return frame + nw * 64 * 8 + ((W * W + 3) & ~3) * 4 + nw * row * 4 + W * 16 * 4 + W * 8

    nw = 1
    while nw < 8 and nw * 2 <= W:
        nw *= 2
    while nw > 1 and lds(nw) > 40 * 1024:
        nw >>= 1
    return lds(nw) if lds(nw) <= 160 * 1024 else 0


def test_search_route_capacity(lib):
    fits = lib.pdt_ctc_lookup_lm_search_lds_bytes
    largest = {}
    for W in range(1, 33):
        lo, hi = 1, 32767
        while lo < hi:  # (the LDS grows with V: 8 bytes a token, rounded to 16)
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if fits(mid, W) > 0 else (lo, mid - 1)
        largest[W] = lo
        for V in (1, 2, 100, 1000, 5119, lo - 2, lo - 1, lo, lo + 1, lo + 2, lo + 3, lo + 4, 20480, 20481, 32767):
            assert fits(V, W) == _old_search_lds(V, W), (V, W)
            assert (fits(V, W) > 0) == (V <= lo), (V, W)
    assert (largest[1], largest[4], largest[32]) == (20272, 20044, 17455), largest
    assert max(largest.values()) == largest[1] < 20480 < 32767  # two rows of V floats alone are 8 V bytes of 160 KB
    for V, W in [(0, 4), (100, 0), (100, 33), (32768, 1), (1 << 40, 4)]:
        assert fits(V, W) == 0, (V, W)
    # the launch refuses what the plan does not admit, before anything touches a device
    from pydrobert_amd import _cabi

    def search(V, W):
        return lib.pdt_ctc_lookup_lm_search(1, 1, 1, 1, 0, 3, 2, V, W, 1, 1, 1, 1, 1, 1, 1, 2, V + 2, V, 0.3, 0, 1, 1, 1, 1, 1, 1 << 40, 0)

    assert search(32768, 1) == _cabi.PDT_E_TOO_LONG
    assert search(100, 33) == _cabi.PDT_E_TOO_LONG
