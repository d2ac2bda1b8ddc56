"""CTCPrefixSearch with an n-gram LookupLanguageModel in the loop at every form its kernels take, each route
of the package ("table" = csrc/ctc_lm_table.hip, "search" = csrc/ctc_lm_step.hip from one call, "three" =
the host's frame loop; tests/test_lm_search_gpu.py) against oracle.ctc_prefix_search_lm around
oracle.NGramLM.  The inputs, their oracle results and their near-tied utterances are tests/_lm_forms.py's.

What the cases reach (host dispatch arithmetic: pdt_ctc_lm_table_search_plan, asserted below; the tiers of
the list selection from reading make_list in csrc/ctc_lm_table.hip):
  * the instance sweep: every ctc_lm_table_kernel<NR, WC>, NR in {8, 16, 32, 48, 80} with the width a
    constant (16) and generic, on both sides of every chunk-count edge; V <= 64 takes the plain sort, larger
    V the cheap threshold when K + K' <= 32 (K <= 16) and the 64-key sort above; V = 5120 leaves the route;
  * tiny vocabularies: the ring narrower than one row of the output walk's table (the host loop that
    looked for a checkpoint spacing did not end for them), beams wider than the prefixes that exist;
  * orders three and four on the table route (ctx_mod > 1), sos inside and outside the vocabulary;
  * checkpoints 64 to 512 frames apart (blank-dominated inputs of 200 and 300 frames);
  * exact ties (pairs of tokens with one logit and one score: the rounded 32-bit sort hands over to the pair
    sort; the lower token wins) and heavy ties (more than 64 survivors at the threshold: the chunked merge);
  * batch-major and vocabulary-strided logits, a batch that is no multiple of 8 (xcd_remap);
  * the largest vocabulary the search route's LDS plan admits, and the next one, which goes frame by frame.

Tokens and lengths exact; probabilities to rtol 1e-5, from 200 frames on as log-probabilities
(_drift.check_log_probs).  A near-tied utterance (tests/_lm_forms.py) is left out of the exact comparison
only: no NaN, and its sorted finite masses within 1e-4 of the oracle's.  At most 1 utterance of a case and 2 %
of all are near-tied, and every finite oracle mass is at least 1e-30 -- asserted on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _drift
import _lm_forms as forms
from pydrobert_amd import _cabi, _decoding
from pydrobert_amd import modules as M

gpu = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-5
ROUTES = {"table": dict(PDT_CTC_LM_TABLE=1, PDT_CTC_LM_FUSED=1),
          "search": dict(PDT_CTC_LM_TABLE=0, PDT_CTC_LM_FUSED=1),
          "three": dict(PDT_CTC_LM_TABLE=0, PDT_CTC_LM_FUSED=0)}
NAMES = [c.name for c in forms.CASES]


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as g

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


# ---- the inputs, on the CPU ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_inputs_keep_their_masses_and_few_near_ties(name):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    for vm in (0, 1):
        y, yl, yp = data.exp[vm]
        assert yp.shape == (case.N, case.K) and not np.isnan(yp).any()
        fin = np.isfinite(yp)
        assert fin[:, 0].all() and (yp[fin] != 0).all(), (name, vm)
        assert yp[fin].min() >= forms.MASS_FLOOR, (name, vm, yp[fin].min())
        assert data.marked[vm].sum() <= 1, (name, vm, int(data.marked[vm].sum()))
    if case.T >= 8:
        assert data.exp[0][1].max() >= 3  # (the search decodes something)


def test_near_tied_utterances_are_few():
    total = sum(2 * c.N for c in forms.CASES)
    marked = sum(int(m.sum()) for c in forms.CASES for m in forms.case_data(c.name).marked)
    assert total == 456 and marked * 50 <= total, (marked, total)


def test_instance_sweep_reaches_every_table_kernel_instance(lib):
    """From the host's dispatch arithmetic (pdt_ctc_lm_table_search_plan): (NR, constant width) of every pair."""
    reached = {}
    for V, K in forms.INSTANCES:
        plan = _decoding._lm_table_plan(12, V, K)
        reached.setdefault((plan[2], plan[3]), []).append((V, K))
    assert set(reached) == {(nr, wc) for nr in (8, 16, 32, 48, 80) for wc in (16, 0)}, reached
    assert _decoding._lm_table_plan(8, 5120, 8) is None
    # both sides of every edge of the chunk count
    nr_of = {V: _decoding._lm_table_plan(12, V, K)[2] for V, K in forms.INSTANCES}
    assert [nr_of[V] for V in (511, 512, 1023, 1024, 2047, 2048, 3071, 3072, 5119)] == [8, 16, 16, 32, 32, 48, 48, 80, 80]


def test_long_inputs_space_their_checkpoints_apart(lib):
    for name, (lo, hi) in forms.CKPT_SHIFTS.items():
        case = forms.BY_NAME[name]
        assert int(forms.case_data(name).lens.max()) == case.T
        shift = _decoding._lm_table_plan(case.T, case.V, case.K)[0]
        assert shift >= lo and (hi is None or shift <= hi), (name, shift)
    for case in forms.CASES:  # every other case of the table route keeps the spacing of 32 frames
        if case.table and case.name not in forms.CKPT_SHIFTS:
            assert _decoding._lm_table_plan(case.T, case.V, case.K)[0] == 5, case.name


def test_capacity_cases_sit_on_the_search_routes_boundary(lib):
    fits = lib.pdt_ctc_lookup_lm_search_lds_bytes
    assert fits(forms.SEARCH_MAX_V_W4, 4) > 0 and fits(forms.SEARCH_MAX_V_W4 + 1, 4) == 0
    for case in forms.CASES:
        assert (fits(case.V, case.K) > 0) == case.search, case.name
        assert (_decoding._lm_table_plan(case.T, case.V, case.K) is not None) == case.table, case.name


def test_oracle_against_brute_force_while_every_prefix_fits_the_beam():
    """Width 32 over two tokens: the beam is wider than its candidates for four frames, where the reference
    returns NaN (oracle/_search.py keeps the entries without a mass absent instead).  Up to there every
    prefix fits the beam, so the search is exact: the oracle's masses are those of the enumeration."""
    lg, lens, dicts, sos, exact = forms.exact_data()
    olm = forms.oracle.NGramLM(forms.EXACT.V, sos, dicts)
    for vm in (False, True):
        y, yl, yp = forms.oracle.ctc_prefix_search_lm(lg, forms.EXACT.K, lens, olm, forms.BETA, vm)
        for n in range(forms.EXACT.N):
            assert 2 ** (int(lens[n]) + 1) - 1 <= forms.EXACT.K and min(exact[vm][n].values()) > 0  # (prefixes in all; those with an alignment)
            assert forms.same_prefix_masses(y[:, n], yl[n], yp[n], exact[vm][n]), (vm, n)


# ---- every route against the oracle -------------------------------------------------------------------
def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)  # (a copy: the inputs are read-only)


@functools.lru_cache(maxsize=None)
def _model(name):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    return M.LookupLanguageModel(case.V, data.sos, [d.copy() for d in data.dicts]).to(DEV)


def _logits(case, lg):
    if case.layout == "batch_major":
        t = _t(lg.transpose(1, 0, 2)).transpose(0, 1)
        assert not t.is_contiguous() and t.stride(1) > t.stride(0)
    elif case.layout == "stride2":
        wide = torch.zeros((case.T, case.N, 2 * (case.V + 1)), device=DEV)
        wide[:, :, ::2] = _t(lg)
        t = wide[:, :, ::2]
        assert t.stride(2) == 2
    else:
        t = _t(lg)
    assert t.shape == lg.shape
    return t


def _search_and_its_route(search, logits, lens):
    """``search(logits, lens)`` and which of the module's routes served it."""
    ran = []
    for method in ("_lm_table_search", "_lookup_lm_search"):
        def spy(*args, _inner=getattr(search, method), _name=method, **kwargs):
            ran.append(_name)
            return _inner(*args, **kwargs)

        setattr(search, method, spy)
    with torch.no_grad():
        out = search(logits, lens)
    assert len(ran) <= 1, ran
    return tuple(x.cpu().numpy() for x in out), (ran[0] if ran else "frame loop")


def _expected_route(case, route):
    if route == "three":
        return "frame loop"
    if route == "table" and case.table:
        return "_lm_table_search"
    return "_lookup_lm_search" if case.search else "frame loop"


def _check(act, exp, marked, what, as_logs):
    y, yl, yp = act
    ey, eyl, eyp = exp
    assert y.shape == ey.shape and yl.shape == eyl.shape and yp.shape == eyp.shape, what
    assert not np.isnan(yp).any(), what
    for n in np.flatnonzero(marked):  # near-tied: the same masses, possibly in another order
        a, e = np.sort(yp[n][np.isfinite(yp[n])]), np.sort(eyp[n][np.isfinite(eyp[n])])
        assert a.shape == e.shape and np.allclose(a, e, rtol=1e-4, atol=0.0), (what, n)
    keep = ~marked
    y, yl, yp, ey, eyl, eyp = y[:, keep], yl[keep], yp[keep], ey[:, keep], eyl[keep], eyp[keep]
    fin = np.isfinite(eyp)
    assert np.array_equal(np.isfinite(yp), fin), what
    assert np.array_equal(yl, eyl), (what, np.argwhere(yl != eyl)[:5])
    inside = np.arange(y.shape[0])[:, None, None] < yl[None]
    assert np.array_equal(np.where(inside, y, 0), ey), (what, np.argwhere(np.where(inside, y, 0) != ey)[:5])
    if as_logs:
        assert fin.all(), what
        _drift.check_log_probs(yp, eyp, "LM forms {}, route {}, valid_mixture={}".format(*what))
    else:
        err = np.abs(yp[fin] / eyp[fin] - 1.0).max()
        print("max relative error", what, err)
        assert np.allclose(yp[fin], eyp[fin], rtol=RTOL, atol=0.0), (what, err)


@gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", NAMES)
def test_every_form_against_the_oracle(name, route, switch):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    for sw, value in ROUTES[route].items():
        switch(sw, value)
    lm = _model(name)
    logits, lens = _logits(case, data.lg), _t(data.lens)
    for vm in (False, True):
        search = M.CTCPrefixSearch(case.K, forms.BETA, lm, valid_mixture=vm)
        act, ran = _search_and_its_route(search, logits, lens)
        assert ran == _expected_route(case, route), (name, route, ran)
        _check(act, data.exp[vm], data.marked[vm], (name, route, vm), case.T >= forms.LONG_T)


@gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_wide_beam_over_two_tokens_against_brute_force(route, switch):
    """The first frames of the widest beam over the smallest vocabulary, where every prefix still fits it:
    each route returns the enumeration's masses (tests/_lm_forms.py: brute_force), whatever the order."""
    case = forms.EXACT
    lg, lens, dicts, sos, exact = forms.exact_data()
    for sw, value in ROUTES[route].items():
        switch(sw, value)
    lm = M.LookupLanguageModel(case.V, sos, [d.copy() for d in dicts]).to(DEV)
    for vm in (False, True):
        search = M.CTCPrefixSearch(case.K, forms.BETA, lm, valid_mixture=vm)
        (y, yl, yp), ran = _search_and_its_route(search, _t(lg), _t(lens))
        assert ran == _expected_route(case, route), (route, ran)
        for n in range(case.N):
            assert forms.same_prefix_masses(y[:, n], yl[n], yp[n], exact[vm][n]), (route, vm, n, yp[n], yl[n])
