"""What the cases of tests/test_fill_forms_gpu.py (tests/_fill_forms.py) reach, asserted without a GPU: the geometry of
csrc/fill_after_eos.hip is restated here in literals, and the shapes and planted positions must land in every
tier, wave, slot, sub-block and pass of it.  An edit of the shape lists that drops one of these fails here."""
import numpy as np
import pytest

import _fill_forms as ff

# columns kernel: L -> (waves, passes, rows of the last pass).  Every tier at both ends; one, two and three passes
# at 16 waves, each but the last at both ends, and a third pass that is partly full.
COLS_GEOMETRY = {
    2: (1, 1, 2), 8: (1, 1, 8),
    9: (2, 1, 9), 16: (2, 1, 16),
    17: (4, 1, 17), 32: (4, 1, 32),
    33: (8, 1, 33), 64: (8, 1, 64),
    65: (16, 1, 65), 128: (16, 1, 128),
    129: (16, 2, 1), 256: (16, 2, 128),
    257: (16, 3, 1), 300: (16, 3, 44),
}  # fmt: skip
# rows kernel: L -> (passes, sub-blocks of the last pass, positions of its last sub-block)
ROWS_GEOMETRY = {
    1: (1, 1, 1), 63: (1, 1, 63), 64: (1, 1, 64), 65: (1, 2, 1),
    511: (1, 8, 63), 512: (1, 8, 64), 513: (2, 1, 1),
    1024: (2, 8, 64), 1025: (3, 1, 1), 1500: (3, 8, 28),
}  # fmt: skip


def test_the_shape_lists_are_the_geometry_restated():
    got = {}
    for L in ff.COLS_L:
        nw = ff.cols_waves(L)
        passes = -(-L // (8 * nw))
        got[L] = (nw, passes, L - (passes - 1) * 8 * nw)
    assert got == COLS_GEOMETRY
    got = {}
    for L in ff.ROWS_L:
        passes = -(-L // 512)
        rest = L - (passes - 1) * 512
        blocks = -(-rest // 64)
        got[L] = (passes, blocks, rest - (blocks - 1) * 64)
    assert got == ROWS_GEOMETRY
    # four sequences to a workgroup: part of one, all of one, one more, and a third workgroup
    assert ff.ROWS_PER_GROUP == 4 and ff.COLS_PER_GROUP == 64 and ff.ROWS_PASS == 8 * ff.SUB_BLOCK == 512
    assert [(-(-o // 4), o % 4) for o in ff.ROWS_OUTER] == [(1, 1), (1, 3), (1, 0), (2, 1), (3, 1)]
    # 64 columns to a workgroup: outer * inner below, at and above a multiple of 64, one to seven workgroups
    cols = sorted({o * i for o in ff.COLS_OUTER for i in ff.COLS_INNER})
    assert cols == [2, 6, 63, 64, 65, 130, 189, 192, 195, 390]
    assert {c % 64 for c in cols} >= {63, 0, 1, 2} and {-(-c // 64) for c in cols} >= {1, 2, 3, 4, 7}
    assert ff.cols_waves(8) == 1 and ff.cols_waves(9) == 2 and ff.cols_waves(128) == 16 and ff.cols_waves(10**6) == 16
    assert ff.cols_place(300, 299) == (2, 11, 2) and ff.cols_place(9, 8) == (0, 0, 4) and ff.rows_place(1499) == (2, 7, 27)


@pytest.mark.parametrize("L", ff.ROWS_L)
def test_rows_cases_plant_every_fixed_position_in_every_wave(L):
    want = {p for p in (ff.NONE, 0, 63, 64, 511, 512, L - 1) if p < L}
    for outer in ff.ROWS_OUTER:
        rounds = ff.rows_rounds(L, outer)
        fixed, interior = np.stack(rounds[:-1]), rounds[-1]
        for i in range(outer):
            assert set(fixed[:, i].tolist()) == want, (L, outer, i)
        assert interior.shape == (outer,)
        assert L <= 2 or ((interior > 0) & (interior < L - 1)).all()
    for case in ff.rows_cases(L):
        tok = ff.build_tokens(case.first, L)
        assert tok.shape == (case.outer, L, 1) and np.array_equal(ff.first_eos(tok, ff.EOS), case.first)


def test_rows_cases_reach_every_sub_block_a_later_pass_and_the_carry():
    places, carried, later_first, none_long = set(), 0, 0, 0
    for L in ff.ROWS_L:
        for case in ff.rows_cases(L):
            tok = ff.build_tokens(case.first, L)[:, :, 0]
            for o, p in enumerate(case.first[:, 0]):
                if p == ff.NONE:
                    none_long += L > 1024 and not (tok[o] == ff.EOS).any()
                    continue
                places.add(ff.rows_place(int(p)))
                # the first eos in one pass and positions to fill in a later one, with no eos of their own there
                # before some position (sparse sequences: none at all): only the carried flag fills those
                nxt = (p // 512 + 1) * 512
                if nxt < L and not (tok[o, nxt : nxt + 64] == ff.EOS).any():
                    carried += 1
                # a later eos in an earlier sub-block of a later pass than the first eos's own
                if p % 512 >= 64 and nxt < L and tok[o, nxt] == ff.EOS:
                    later_first += 1
    assert {(p, b) for p, b, _ in places} >= {(0, b) for b in range(8)} | {(1, b) for b in range(8)} | {(2, 0), (2, 7)}
    lanes = {(b, l) for _, b, l in places}
    assert {(0, 0), (0, 63), (1, 0), (7, 63)} <= lanes  # positions 0, 63, 64, 511 (and 512: pass 1, lane 0)
    assert (1, 0, 0) in places and (0, 7, 63) in places
    assert carried >= 20 and later_first >= 20 and none_long >= 5, (carried, later_first, none_long)


@pytest.mark.parametrize("L", ff.COLS_L)
def test_columns_cases_give_every_column_a_position(L):
    for case in ff.cols_cases(L):
        first = case.first.reshape(-1)
        assert first[0] == ff.NONE and (first.size < 2 or first[1] == 0) and (first.size < 3 or first[2] == L - 1)
        assert ((first >= ff.NONE) & (first < L)).all()
        # a permutation of the rows dealt over the columns, four of which the fixed positions then replace
        assert len(set(first.tolist())) >= min(L, first.size) - 4, (L, case.inner, case.outer)
        tok = ff.build_tokens(case.first, L)
        assert np.array_equal(ff.first_eos(tok, ff.EOS), case.first)


def test_columns_cases_reach_every_tier_wave_slot_and_pass():
    waves, slots, tiers = {}, {}, set()
    other_wave_later_pass, early_exit, late_eos_before = 0, 0, 0
    for L in ff.COLS_L:
        nw = ff.cols_waves(L)
        tiers.add(nw)
        for case in ff.cols_cases(L):
            tok = ff.build_tokens(case.first, L)
            for (o, i), p in np.ndenumerate(case.first):
                if p == ff.NONE:
                    continue
                ps, w, q = ff.cols_place(L, int(p))
                waves.setdefault(nw, set()).add(w)
                slots.setdefault(nw, set()).add(q)
                other_wave_later_pass += ps > 0 and w > 0
                # wave 0 stops searching after the pass in which it found an eos, which is later than the first
                early_exit += ps == 0 and w > 0 and (tok[o, 8 * nw :: nw, i] == ff.EOS).any() and 8 * nw < L
                nxt = (ps + 1) * 8 * nw
                late_eos_before += nxt < L and tok[o, nxt, i] == ff.EOS and w > 0
    assert tiers == {1, 2, 4, 8, 16}
    for nw in tiers:
        assert waves[nw] == set(range(nw)), (nw, waves[nw])
        assert slots[nw] == set(range(8)), (nw, slots[nw])
    assert other_wave_later_pass >= 50 and early_exit >= 50 and late_eos_before >= 50
    passes = {ff.cols_place(L, L - 1)[0] for L in ff.COLS_L}
    assert passes == {0, 1, 2}


def test_dtype_sweep_and_single_shapes_reach_both_kernels_and_a_later_pass():
    assert set(ff.DTYPES) == {"bool", "uint8", "int16", "float16", "bfloat16", "int32", "float32", "int64", "float64"}
    assert {ff.width_of(d) for d in ff.DTYPES} == {1, 2, 4, 8}
    assert any(f != f for f, _ in ff.FILLS["float32"]) and any(str(f) == "-0.0" for f, _ in ff.FILLS["bfloat16"])
    for name in ("float16", "bfloat16", "float32", "float64"):
        assert {str(f) for f, _ in ff.FILLS[name]} >= {"-0.0", "nan"}
    for name in ("int16", "int32", "int64"):
        assert all(f < 0 for f, _ in ff.FILLS[name])
    assert ff.FILLS["bool"] == [(1.0, 1)]
    assert all(o * L > 0 and L in ff.ROWS_L for o, L in ff.DTYPE_ROWS) and max(L for _, L in ff.DTYPE_ROWS) > 1024
    assert {ff.cols_waves(L) for _, L, _ in ff.DTYPE_COLS} == {2, 16} and max(L for _, L, _ in ff.DTYPE_COLS) > 256
    assert ff.LONG_ROWS[1] > 512 and ff.cols_waves(ff.LONG_COLS[1]) == 16
    for shape in ff.DTYPE_ROWS + ff.DTYPE_COLS + [ff.LONG_ROWS, ff.LONG_COLS]:
        later = 0
        for case in ff.shape_cases(shape):
            plen = ff.pass_length(case.L, case.inner)
            later += int((case.first >= plen).sum())
        assert later > 0 or case.L <= plen, shape
    # the ends of int64 are in the alphabet of their test, and the int64 fill is a number a float holds
    assert ff.INT64_ENDS[:2] == (2**63 - 1, -(2**63)) and int(ff.FILLS["int64"][0][0]) == ff.FILLS["int64"][0][1]
