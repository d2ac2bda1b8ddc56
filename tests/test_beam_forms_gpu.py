"""BeamSearch at every form its kernels take, each route of the package against oracle.beam_search: the inputs,
their oracle results and the forms they are meant to reach are tests/_beam_forms.py's (conditions on them:
tests/test_beam_forms_cpu.py).

Routes (tests/test_lm_search_gpu.py: BEAM_ROUTES): "search" = every iteration in one launch
(beam_search_table_kernel, both instances, and beam_search_walk_kernel), "table" = an iteration per launch over
the model's dense table (beam_step_flat_kernel; beam_step_kernel where the flat form does not take the shape),
"table_list" = the same with PDT_STEP_FLAT=0 (beam_step_kernel at every shape), "fused" = an iteration per launch
around the model's forward (beam_step_kernel), "loop" = the reference-shaped loop around beam_search_advance.
Which entry point served a search is asserted, from what was called.

  * lookup cases: a bigram LookupLanguageModel at both sides of every dispatch boundary, without eos, with eos,
    with eos and finish_all_paths; 257 and 600 iterations (the walk's tiles), one iteration, no batch dimension;
  * raw tables under the table routes: fewer finite candidates than the beam is wide (the -inf fill in flat
    order; with eos and finish_all_paths: an ended path's tokens other than eos among them, and the entries
    they make stay ended), every candidate tied (more than 64 survivors: the chunked merge), a third of every
    row -inf;
  * mixed batches: every element starts from a row of its own, so the elements finish at different iterations and
    some never -- the dense routes through a model with per-element start rows, the table step driven through
    the C ABI with per-element rows; every element again alone, to the bit.

Paths inside the lengths and the lengths exactly, log-probabilities to rtol 1e-5 / atol 1e-6 with -inf equal as
-inf, and every row from an element's first padding row on equal to pad_value."""
import json
import os

import numpy as np
import pytest
import torch

import _beam_forms as forms
import _drift
import _lm_forms
from _toy_lm import StartRowBigramLM
from pydrobert_amd import _cabi
from pydrobert_amd import modules as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROUTES = {"search": dict(PDT_BEAM_FUSED=1, PDT_BEAM_TABLE=1, PDT_BEAM_SEARCH=1, PDT_STEP_FLAT=1),
          "table": dict(PDT_BEAM_FUSED=1, PDT_BEAM_TABLE=1, PDT_BEAM_SEARCH=0, PDT_STEP_FLAT=1),
          "table_list": dict(PDT_BEAM_FUSED=1, PDT_BEAM_TABLE=1, PDT_BEAM_SEARCH=0, PDT_STEP_FLAT=0),
          "fused": dict(PDT_BEAM_FUSED=1, PDT_BEAM_TABLE=0, PDT_STEP_FLAT=1),
          "loop": dict(PDT_BEAM_FUSED=0, PDT_STEP_FLAT=1)}
_DRIFT = os.path.join(os.path.dirname(_drift._OUT), "beam_forms_drift.json")  # beside tests/_drift.py's own record


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)  # (a copy: the inputs are read-only)


def _np(out):
    return tuple(x.cpu().numpy() for x in out)


def _check(act, exp, case, pad_rows, what):
    """-> the largest |difference| of the finite log-probabilities."""
    y, lens, lp = act
    ey, elens, elp = exp
    assert y.shape == ey.shape and lens.shape == elens.shape and lp.shape == elp.shape, (what, y.shape, ey.shape)
    assert np.array_equal(lens, elens), (what, np.argwhere(lens != elens)[:5])
    assert forms.same((y, lens), (ey, elens)), what
    assert not np.isnan(lp).any() and np.array_equal(np.isneginf(lp), np.isneginf(elp)), what
    fin = np.isfinite(elp)
    err = float(np.abs(lp[fin] - elp[fin]).max()) if fin.any() else 0.0
    print("max |d log p|", what, err)
    assert np.allclose(lp, elp, rtol=forms.RTOL, atol=forms.ATOL), (what, err)
    yb = y if case.N is not None else y[:, None]
    for n, t in enumerate(pad_rows):  # from the iteration that found the element finished on: pad_value, every entry
        if t >= 0:
            assert (yb[t:, n] == case.pad).all(), (what, n, t)
    return err


def _record(config, err):
    try:
        os.makedirs(os.path.dirname(_DRIFT), exist_ok=True)
        rec = json.load(open(_DRIFT)) if os.path.exists(_DRIFT) else {}
        rec[config] = {"max_abs_dlogp": err}
        json.dump(rec, open(_DRIFT, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


class _Calls:
    """Which of BeamSearch's entry points a search went through: K' of every pdt_beam_search_step_table and
    pdt_beam_search_step call, whether pdt_beam_search_table took the shape, and the pdt_beam_search_advance
    calls of the step-by-step loop."""

    def __init__(self, monkeypatch):
        self.table_steps, self.dense_steps, self.one_launch, self.advances = [], [], [], []
        L = _cabi.lib()
        inner = {name: getattr(L, name) for name in ("pdt_beam_search_step_table", "pdt_beam_search_step", "pdt_beam_search_table",
                                                     "pdt_beam_search_advance")}

        def advance(*args):
            self.advances.append(1)
            return inner["pdt_beam_search_advance"](*args)

        def step_table(*args):
            self.table_steps.append(int(args[7]))
            return inner["pdt_beam_search_step_table"](*args)

        def step(*args):
            self.dense_steps.append(int(args[5]))
            return inner["pdt_beam_search_step"](*args)

        def table(*args):
            rc = inner["pdt_beam_search_table"](*args)
            self.one_launch.append(rc)
            return rc

        monkeypatch.setattr(L, "pdt_beam_search_step_table", step_table)
        monkeypatch.setattr(L, "pdt_beam_search_step", step)
        monkeypatch.setattr(L, "pdt_beam_search_table", table)
        monkeypatch.setattr(L, "pdt_beam_search_advance", advance)

    def clear(self):
        del self.table_steps[:], self.dense_steps[:], self.one_launch[:], self.advances[:]

    def served(self):
        if self.one_launch == [_cabi.PDT_OK]:
            assert not self.table_steps and not self.dense_steps and not self.advances
            return "search"
        assert sum(bool(c) for c in (self.table_steps, self.dense_steps, self.advances)) == 1, "one route, and a known one"
        for steps in (self.table_steps, self.dense_steps):
            assert steps[:1] in ([], [1]) and all(k == steps[-1] for k in steps[1:])  # K' = 1, then the width
        return "table" if self.table_steps else ("fused" if self.dense_steps else "loop")  # (loop: its advances were seen)


def _expected(case, route):
    if route == "search":
        return "search" if case.search is not None else "table"
    return "table" if route == "table_list" else route


def _run(search, case, route, switch, calls):
    for name, value in ROUTES[route].items():
        switch(name, value)
    calls.clear()
    with torch.no_grad():
        out = _np(search(dict(), case.N, case.iters))
    ran = calls.served()
    assert ran == _expected(case, route), (case.name, route, ran, calls.one_launch)
    if route == "search":
        assert calls.one_launch == [_cabi.PDT_OK if case.search is not None else _cabi.PDT_E_UNSUPPORTED], calls.one_launch
    return out


@pytest.mark.parametrize("name", forms.LOOKUP)
def test_lookup_model_every_route_against_the_oracle(name, switch, monkeypatch):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    calls = _Calls(monkeypatch)
    lm = M.LookupLanguageModel(case.V, case.V, [d.copy() for d in data.model]).to(DEV)
    search = M.BeamSearch(lm, case.W, case.eos, case.fin, case.pad).to(DEV)
    for route in ROUTES:
        if route == "table_list" and case.step != "flat":
            continue  # (the table step is the list form already)
        act = _run(search, case, route, switch, calls)
        err = _check(act, data.exp, case, data.pad_rows, (name, route))
        if case.iters > 256:
            _record("{} route {}".format(name, route), err)


def _row_stats(table):
    stats = torch.empty((table.size(0), 2), device=table.device)
    rc = _cabi.lib().pdt_row_log_softmax_stats(_cabi.ptr(table), table.stride(0), table.stride(1), table.size(0), table.size(1),
                                               _cabi.ptr(stats), _cabi.stream_ptr(table.device))
    assert rc == _cabi.PDT_OK
    return stats


@pytest.mark.parametrize("name", forms.RAW)
def test_raw_tables_under_the_table_routes_against_the_oracle(name, switch, monkeypatch):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    calls = _Calls(monkeypatch)
    V = case.V
    dicts = _lm_forms.ngram_dicts(forms.LmSpec(V, 2, False, "peaky", 1), np.random.default_rng(0))
    search = M.BeamSearch(M.LookupLanguageModel(V, V, dicts).to(DEV), case.W, case.eos, case.fin, case.pad).to(DEV)
    table = _t(data.model)
    dense = (table, _row_stats(table), V, V + 1)
    monkeypatch.setattr(search, "_bigram_table", lambda device: dense)
    for route in ("search", "table", "table_list"):
        act = _run(search, case, route, switch, calls)
        _check(act, data.exp, case, data.pad_rows, (name, route))
        if case.kind.startswith("sparse"):  # while entries without a score are still in the beam: which ones, in which order
            for iters in (1, 2, 3):
                short, exp = forms.short_data(name, iters)
                assert np.isneginf(exp[2]).any()
                _check(_run(search, short, route, switch, calls), exp, short, forms.first_pad(short, exp), (name, route, iters))


def _alone_equals_batch(alone, batch, n, case, what):
    """An element searched alone: the bits it has in the batch, which pads it from its own last row on."""
    (y1, l1, p1), (y, lens, lp) = alone, batch
    S = y1.shape[0]
    assert S <= y.shape[0], what
    assert np.array_equal(l1[0], lens[n]) and np.array_equal(p1[0].view(np.uint32), lp[n].view(np.uint32)), what
    assert np.array_equal(y1[:, 0], y[:S, n]) and (y[S:, n] == case.pad).all(), what


@pytest.mark.parametrize("route", ["fused", "loop"])
@pytest.mark.parametrize("name", forms.MIXED)
def test_mixed_batch_on_the_dense_routes(name, route, switch, monkeypatch):
    case, data = forms.BY_NAME[name], forms.case_data(name)
    calls = _Calls(monkeypatch)
    table = _t(data.model)
    starts = torch.arange(case.V, case.V + case.N, device=DEV)
    search = M.BeamSearch(StartRowBigramLM(table, starts), case.W, case.eos, case.fin, case.pad).to(DEV)
    act = _run(search, case, route, switch, calls)
    _check(act, data.exp, case, data.pad_rows, (name, route))
    for n in range(case.N):
        one = M.BeamSearch(StartRowBigramLM(table, starts[n : n + 1]), case.W, case.eos, case.fin, case.pad).to(DEV)
        with torch.no_grad():
            alone = _np(one(dict(), 1, case.iters))
        _alone_equals_batch(alone, act, n, case, (name, route, n))


def _drive_table_step(table, stats, starts, case):
    """pdt_beam_search_step_table for ``case.iters`` iterations, element n starting from row ``starts[n]`` and
    every prefix following the row of its last token, as BeamSearch's host loop drives it -- which cannot give
    the elements rows of their own.  -> (y with pad_value from pad_from on, lens, log-probs, active, pad_from)."""
    L, dev = _cabi.lib(), table.device
    N, W, V, T = starts.numel(), case.W, case.V, case.iters
    y = torch.empty((0, N, 1), dtype=torch.long, device=dev)
    lp = torch.zeros((N, 1), device=dev)
    lens = torch.zeros((N, 1), dtype=torch.long, device=dev)
    active = torch.zeros((T,), dtype=torch.int32, device=dev)
    pad_from = torch.full((N,), 2147483647, dtype=torch.int32, device=dev)
    stream, Kp = _cabi.stream_ptr(dev), 1
    for t in range(T):
        rows = starts.view(N, 1).contiguous() if t == 0 else y[t - 1]
        assert rows.is_contiguous() and rows.shape == (N, Kp)
        y_new = torch.empty((t + 1, N, W), dtype=torch.long, device=dev)
        lens_new = torch.empty((N, W), dtype=torch.long, device=dev)
        lp_new = torch.empty((N, W), device=dev)
        src = torch.empty((N, W), dtype=torch.long, device=dev)
        rc = L.pdt_beam_search_step_table(
            table.data_ptr(), table.stride(0), table.stride(1), table.size(0), stats.data_ptr(), rows.data_ptr(), N, Kp, V, W,
            lp.data_ptr(), lp.stride(0), lp.stride(1), y.data_ptr(), t, y.stride(0), y.stride(1), y.stride(2),
            lens.data_ptr(), lens.stride(0), lens.stride(1), int(case.eos is not None), int(case.eos or 0), int(case.fin),
            case.pad, y_new.data_ptr(), lens_new.data_ptr(), lp_new.data_ptr(), src.data_ptr(),
            active.data_ptr() + 4 * t, pad_from.data_ptr(), stream)  # fmt: skip
        assert rc == _cabi.PDT_OK, (t, rc)
        y, lens, lp, Kp = y_new, lens_new, lp_new, W
    idx = torch.arange(T, device=dev).view(-1, 1, 1)
    y = torch.where(idx >= pad_from.view(1, N, 1), y.new_full((), case.pad), y)
    return _np((y, lens, lp)), active.cpu().numpy(), pad_from.cpu().numpy()


@pytest.mark.parametrize("flat", [1, 0])
@pytest.mark.parametrize("name", forms.MIXED)
def test_mixed_batch_on_the_table_step(name, flat, switch):
    """The table step with a row of its own per element, in both kernels (PDT_STEP_FLAT; tests/_beam_forms.py names
    the one a shape takes): the oracle's result, extended by the padding of the iterations run past its end."""
    case, data = forms.BY_NAME[name], forms.case_data(name)
    switch("PDT_STEP_FLAT", flat)
    table = _t(data.model)
    stats = _row_stats(table)
    starts = torch.arange(case.V, case.V + case.N, device=DEV)
    (y, lens, lp), active, pad_from = _drive_table_step(table, stats, starts, case)
    S = data.exp[0].shape[0]
    _check((y[:S], lens, lp), data.exp, case, data.pad_rows, (name, flat))
    assert (y[S:] == case.pad).all(), name
    # the iterations that started with an unfinished element: those of the oracle's loop
    assert active.tolist() == [1] * S + [0] * (case.iters - S), (name, active.tolist())
    # an element found finished at iteration t is padded from row t on
    found = np.where(pad_from == 2147483647, -1, pad_from)
    assert np.array_equal(found, data.pad_rows), (name, found, data.pad_rows)
    for n in range(case.N):
        alone, _, pf = _drive_table_step(table, stats, starts[n : n + 1], case)
        assert pf[0] == pad_from[n]
        _alone_equals_batch(alone, (y, lens, lp), n, case, (name, flat, n))
