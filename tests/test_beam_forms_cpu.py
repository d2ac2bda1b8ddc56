"""Conditions on the inputs of tests/test_beam_forms_gpu.py (tests/_beam_forms.py), none of which needs a GPU:
no case is near-tied, every eos case stops where it should, every mixed batch is mixed, the forms the case
table names are the forms the launchers' own plan functions report, and the tables of the two fallbacks of the
flat selection send it there."""
import ctypes
import os

import numpy as np
import pytest

import _beam_forms as forms
import oracle
from pydrobert_amd import _cabi

NAMES = [c.name for c in forms.CASES]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def _step_plan(lib, Kp, V, W, has_rows, stride=1):
    waves = ctypes.c_int32(-1)
    form = lib.pdt_beam_search_step_plan(Kp, V, W, has_rows, stride, ctypes.byref(waves))
    return "flat" if form == 1 else ("list%d" % waves.value if form == 0 else form)


def _table_plan(lib, V, W, U=None):
    form = lib.pdt_beam_search_table_plan(V + 1 if U is None else U, V, W, 1)
    return {0: "rows16", 1: "chunks", _cabi.PDT_E_UNSUPPORTED: None}[form]


@pytest.mark.parametrize("name", NAMES)
def test_no_case_is_near_tied_and_every_case_decodes(name):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    y, lens, lp = data.exp
    assert not data.marked, name  # (another salt in tests/_beam_forms.py, never a looser comparison)
    assert not np.isnan(lp).any() and y.shape[0] <= case.iters
    assert lp.shape == ((case.W,) if case.N is None else (case.N, case.W))
    assert np.isfinite(lp[..., 0]).all(), name


def test_eos_cases_stop_inside_their_iterations():
    plain = [c for c in forms.CASES if c.kind == "lookup" and c.eos is not None and not c.fin and c.iters > 1]
    inside = 0
    for case in plain:
        S = forms.case_data(case.name).exp[0].shape[0]
        inside += 2 <= S < case.iters
    assert 2 * inside >= len(plain), (inside, len(plain))
    for case in forms.CASES:
        if case.kind == "lookup" and case.fin:
            y, lens, _ = forms.case_data(case.name).exp
            S = y.shape[0]
            assert 2 <= S <= case.iters, (case.name, S)
            # a path ended before the last iteration: one that has not ended is S tokens long (a beam of one path
            # ends with its only path, in the last iteration)
            assert case.W == 1 or lens.min() < S, (case.name, S, lens.min())


@pytest.mark.parametrize("name", NAMES)
def test_padding_rows_of_the_oracle_are_where_first_pad_says(name):
    """first_pad's argument, checked on the oracle's own y.  Where pad_value is also a token the oracle runs again
    with one that is not: nothing but the padding rows depends on it."""
    case, data = forms.BY_NAME[name], forms.case_data(name)
    exp = data.exp
    if case.pad >= 0:
        case = case._replace(pad=-7)
        exp = forms.run_oracle(case, forms.oracle_lm(case, data.model))
        assert all(np.array_equal(a, b) for a, b in zip(exp[1:], data.exp[1:])) and forms.same(exp, data.exp)
        assert np.array_equal(forms.first_pad(case, exp), data.pad_rows)
    y = exp[0] if case.N is not None else exp[0][:, None]
    for n, t in enumerate(data.pad_rows):
        padded = (y[:, n] == case.pad).all(1)
        first = int(np.argmax(padded)) if padded.any() else -1
        assert first == (t if 0 <= t < y.shape[0] else -1), (name, n, first, t)
        assert not (y[:, n] == case.pad).any(1)[: t if t >= 0 else None].any(), (name, n)


@pytest.mark.parametrize("name", forms.MIXED)
def test_mixed_batches_are_mixed(name):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    pads = data.pad_rows.tolist()
    assert pads == forms.MIXED_FOUND[name], (name, pads)  # (what the case table says these cases reach)
    assert len(set(pads)) >= 3, (name, pads)
    if not case.fin:
        assert -1 in pads and len(set(pads) - {-1}) >= 2, (name, pads)
    else:
        assert max(pads) >= 2, (name, pads)
    # every element alone is the oracle's element of the batch
    for n in range(case.N):
        alone = oracle.beam_search(forms.StartRowLM(data.model, [case.V + n]), case.W, case.eos, case.fin, case.pad, None,
                                   1, case.iters)
        S = alone[0].shape[0]
        assert S <= data.exp[0].shape[0]
        assert np.array_equal(alone[1][0], data.exp[1][n]) and np.array_equal(alone[2][0], data.exp[2][n]), (name, n)
        assert forms.same((alone[0], alone[1]), (data.exp[0][:S, n : n + 1], data.exp[1][n : n + 1])), (name, n)


def test_plans_report_the_forms_the_case_table_names(lib):
    reached = set()
    for case in forms.CASES:
        V, W = case.V, case.W
        step, dense = _step_plan(lib, W, V, W, 1), _step_plan(lib, W, V, W, 0)
        first = _step_plan(lib, 1, V, W, 1)
        search = _table_plan(lib, V, W, V + case.N if case.kind == "mixed" else None)
        assert (step, dense, search) == (case.step, case.dense, case.search), (case.name, step, dense, search)
        assert first == ("flat" if V > 64 else "list1"), (case.name, first)
        assert _step_plan(lib, 1, V, W, 0) == "list1"
        reached |= {step, dense, first, "search:%s" % search}
    assert reached == {"list1", "list2", "list4", "list8", "flat", "search:rows16", "search:chunks", "search:None"}, reached
    # both refusals, and both sides of 256 = 8 waves x 32 chunk registers
    assert _step_plan(lib, 65, 65, 65, 1) == _cabi.PDT_E_TOO_LONG and _step_plan(lib, 0, 65, 4, 1) == _cabi.PDT_E_ARG
    assert lib.pdt_beam_search_table_plan(66, 65, 65, 1) == _cabi.PDT_E_UNSUPPORTED
    assert lib.pdt_beam_search_table_plan(0, 65, 4, 1) == _cabi.PDT_E_ARG
    assert _step_plan(lib, 16, 1024, 16, 1) == "flat" and _step_plan(lib, 16, 1025, 16, 1) == "list8"
    assert _step_plan(lib, 4, 4095, 4, 1) == "flat" and _step_plan(lib, 5, 4095, 5, 1) == "list4"
    assert _step_plan(lib, 64, 64, 64, 1) == "list8" and _step_plan(lib, 64, 65, 64, 1) == "flat"
    assert _step_plan(lib, 16, 1024, 16, 1, 2) == "list8"  # (a strided table: never flat)
    assert _table_plan(lib, 1024, 16) == "rows16" and _table_plan(lib, 1025, 16) is None and _table_plan(lib, 1025, 15) == "chunks"
    assert _table_plan(lib, 65, 16) == "rows16" and _table_plan(lib, 65, 17) == "chunks" and _table_plan(lib, 64, 8) is None
    assert _table_plan(lib, 4095, 4) == "chunks" and _table_plan(lib, 4095, 5) is None
    assert lib.pdt_beam_search_table_plan(65, 65, 16, 1) == 0  # as many rows as tokens (sos inside the vocabulary)
    assert lib.pdt_beam_search_table_plan(64, 65, 16, 1) == _cabi.PDT_E_UNSUPPORTED  # fewer rows than tokens


def _softmax_rows(table):
    return oracle._search._log_softmax(table)


def _ended_continuations(case, exp):
    """(N, W) bool: entries without a score that an ended path left by taking a token other than eos -- ended
    (their last token is eos) with that other token in the row behind their end."""
    y, lens, lp = exp
    out = np.zeros(lp.shape, bool)
    for n, k in np.argwhere(np.isneginf(lp)):
        end = int(lens[n, k])
        out[n, k] = 0 < end < y.shape[0] and y[end - 1, n, k] == case.eos and y[end, n, k] != case.eos
    return out


@pytest.mark.parametrize("name", [n for n in forms.RAW if forms.BY_NAME[n].kind in ("sparse_fin", "sparse_end")])
def test_sparse_tables_with_eos_keep_continuations_of_ended_paths_in_the_beam(name):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    for iters in (2, 3):
        short, exp = forms.short_data(name, iters)
        assert _ended_continuations(short, exp).any(1).all(), (name, iters)
    if case.kind == "sparse_end":
        # two finite paths, both ended; the rest of the beam continues the first ended one: finished at iteration 2
        y, lens, lp = data.exp
        assert y.shape[0] == 2 and data.pad_rows.tolist() == [2] * case.N
        assert (np.isfinite(lp).sum(1) == 2).all() and (_ended_continuations(case, data.exp).sum(1) == case.W - 2).all()
    else:
        assert data.exp[0].shape[0] == case.iters == 3


@pytest.mark.parametrize("name", [n for n in forms.RAW if n.split("_")[0] in ("sparse", "uniform") and forms.BY_NAME[n].eos is None])
def test_fallback_tables_send_the_flat_selection_to_its_fallbacks(name):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    y, lens, lp = data.exp
    ls = _softmax_rows(data.model)
    K = min(case.W, 64)
    if case.kind == "sparse":
        # the first iteration has 2 finite candidates, the second 4, the third 8 (fewer than K while 2^t < K):
        # entries without a finite score fill the beam in flat order
        assert np.isfinite(ls).sum(1).max() == 2 and K > 8
        first = ls[case.V]
        exp0 = sorted(np.flatnonzero(np.isfinite(first)), key=lambda v: -first[v]) + [v for v in range(case.V) if not np.isfinite(first[v])]
        got = oracle.beam_search(oracle.TableLM(data.model), case.W, None, False, case.pad, None, 1, 1)
        assert got[0][0, 0].tolist() == [int(v) for v in exp0[:K]] and np.isfinite(got[2][0]).sum() == 2
        for t, finite in ((2, 4), (3, 8)):
            got = oracle.beam_search(oracle.TableLM(data.model), case.W, None, False, case.pad, None, 1, t)
            assert np.isfinite(got[2][0]).sum() == finite, (name, t)
        assert np.isfinite(lp).sum(1).max() == min(K, 2 ** case.iters)
    else:
        # more than 64 candidates equal the maximum in every iteration: each row has V - 1 equal entries and
        # every prefix the same score
        assert case.V - 1 > 64
        for r in range(case.V + 1):
            assert (ls[r] == ls[r].max()).sum() == case.V - 1 and ls[r].max() == ls[0].max()
        assert (lp == lp[0, 0]).all() and np.isfinite(lp).all()
