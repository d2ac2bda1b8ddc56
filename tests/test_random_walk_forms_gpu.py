"""GPU: pydrobert_amd::random_walk_step, pdt_random_walk_table and RandomWalk.forward held to planned walks
(tests/_walk_plan.py): every token, length, flag, context row and report word equals the plan, and every
log-probability lies within the float32 error bound derived there of the float64 sum along the planned path.  The
plans themselves are checked without a GPU in tests/test_walk_plan_cpu.py."""
import itertools

import numpy as np
import pytest
import torch

import _walk_plan as wp
from _lm_fixtures import random_dicts
from pydrobert_amd import _cabi, _walk
from pydrobert_amd import modules as M
from pydrobert_amd import switches

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

LAYOUTS = ("contiguous", "transposed", "every_other_column")
DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)
STEP_V = (1, 2, 64, 65, 512, 513, 1100)
STEP_N = (1, 3, 4, 5, 257)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ratio(lp32, plan_lp, bound, what):
    """Assert |lp - plan| <= bound wherever the bound is positive (equality where it is zero: no step taken);
    returns the largest ratio."""
    err = np.abs(lp32.astype(np.float64) - plan_lp)
    assert (err[bound == 0] == 0).all(), what
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ---- random_walk_step ------------------------------------------------------------------------------------------


def _scores(x32, layout, dtype, poison):
    """``x32`` (N, V) as a device tensor of ``dtype`` in ``layout``; the rows ``poison`` hold NaN and -inf."""
    x = x32.copy()
    x[poison[0::2]] = np.nan
    x[poison[1::2]] = -np.inf
    t = _dev(x).to(dtype)
    if layout == "transposed":
        t = _dev(x.T).to(dtype).t()
    elif layout == "every_other_column":
        buf = torch.full((x.shape[0], 2 * x.shape[1]), float("nan"), device=DEV, dtype=dtype)
        buf[:, ::2] = t
        t = buf[:, ::2]
    assert t.shape == x.shape
    return t


def _eos_kinds(V):
    return sorted({None, 0, V - 1, V // 2}, key=lambda e: -1 if e is None else e)


def _round_to(x32, dtype):
    """The float32 values of ``x32`` after a round trip through ``dtype`` (what the kernel reads)."""
    return torch.from_numpy(x32).to(dtype).float().numpy()


@pytest.mark.parametrize("V", STEP_V)
def test_step_follows_the_plan(V):
    """Two iterations of every (N, eos) with the layouts and dtypes dealt in turn (every V meets all twelve pairs):
    y[t], lens, ended, log_probs, the returned count and ctl against the plan; walks that come ended emit eos and
    keep their state to the bit, and their score rows, which are poisoned, are not read."""
    pairs = list(itertools.product(LAYOUTS, DTYPES))
    k, worst = 0, 0.0
    for N in STEP_N:
        for eos in _eos_kinds(V):
            layout, dtype = pairs[k % len(pairs)]
            k += 1
            rng = np.random.default_rng([V, N, k])
            T = 4
            y = torch.full((T, N), -7, dtype=torch.long, device=DEV)
            ended0 = rng.random(N) < 0.3
            lens0 = rng.integers(0, 9, N)
            lp0 = rng.normal(size=N).astype(np.float32)
            lens, ended, lp = _dev(lens0), _dev(ended0), _dev(lp0)
            ctl = torch.zeros(4, dtype=torch.int32, device=DEV)
            state = (ended0 & (eos is not None), lens0.copy(), lp0.astype(np.float64), np.zeros(N))
            for t in (2, 0):
                was_ended, lens_b, lp_b, bound = state
                x32 = _round_to(wp.rows_of_every_kind(rng, N, V), dtype)
                rows = wp.Rows(x32)
                plan = wp.plan_walk(rng, rows, lambda r, tok: r, np.arange(N), 1, eos,
                                    np.where(rng.random(N) < 0.4, 0, wp.NEVER), was_ended, lens_b, lp_b)  # fmt: skip
                sc = _scores(x32, layout, dtype, np.nonzero(was_ended)[0])
                lp_before = lp.clone()
                before = y.clone()
                live = torch.ops.pydrobert_amd.random_walk_step(sc, _dev(plan.u[0]), y, t, lens, ended, lp, ctl, eos)
                what = (V, N, eos, layout, dtype, t)
                got = y.cpu().numpy()
                assert np.array_equal(got[t], plan.y[0]), what
                before[t] = y[t]
                assert torch.equal(before, y), what  # (the other rows of y are untouched)
                assert np.array_equal(lens.cpu().numpy(), plan.lens), what
                assert np.array_equal(ended.cpu().numpy(), plan.ended), what
                assert live == plan.live and not ctl.any(), what
                if eos is not None:
                    assert (got[t][was_ended] == eos).all() and np.array_equal(plan.lens[was_ended], lens_b[was_ended])
                    assert torch.equal(lp[_dev(was_ended)].view(torch.int32), lp_before[_dev(was_ended)].view(torch.int32))
                else:
                    assert live == N and np.array_equal(plan.lens, lens_b + 1) and not plan.ended.any()
                bound = bound + plan.bound  # (plan.bound is this iteration's; the state's error comes with it)
                state = (plan.ended, plan.lens, plan.lp, bound)
                worst = max(worst, _ratio(lp.cpu().numpy(), plan.lp, bound, what))
    print("random_walk_step V=%d: largest lp error / bound = %.3f" % (V, worst))


def test_step_row_without_mass_raises_and_the_next_call_works():
    N, V = 6, 70
    rng = np.random.default_rng(5)
    x32 = wp.rows_of_every_kind(rng, N, V)
    rows = wp.Rows(x32)
    bad = x32.copy()
    bad[4] = -np.inf
    y = torch.full((2, N), -7, dtype=torch.long, device=DEV)
    ended0 = np.array([False, True, False, False, False, False])
    lens, ended, lp = _dev(np.zeros(N, np.int64)), _dev(ended0), _dev(np.zeros(N, np.float32))
    ctl = torch.zeros(4, dtype=torch.int32, device=DEV)
    plan = wp.plan_walk(rng, rows, lambda r, tok: r, np.arange(N), 1, 3, np.full(N, wp.NEVER), ended0)
    with pytest.raises(RuntimeError, match="no positive finite mass"):
        torch.ops.pydrobert_amd.random_walk_step(_dev(bad), _dev(plan.u[0]), y, 0, lens, ended, lp, ctl, 3)
    torch.cuda.synchronize()
    assert not ctl.any()
    # an ended walk's row without mass is not read, so it does not raise
    bad = x32.copy()
    bad[1] = -np.inf
    lens, ended, lp = _dev(np.zeros(N, np.int64)), _dev(ended0), _dev(np.zeros(N, np.float32))
    live = torch.ops.pydrobert_amd.random_walk_step(_dev(bad), _dev(plan.u[0]), y, 1, lens, ended, lp, ctl, 3)
    assert live == plan.live and np.array_equal(y[1].cpu().numpy(), plan.y[0]) and not ctl.any()
    assert np.array_equal(lens.cpu().numpy(), plan.lens)
    _ratio(lp.cpu().numpy(), plan.lp, plan.bound, "after the error")


# ---- pdt_random_walk_table -------------------------------------------------------------------------------------


class _Table:
    """A hand-made table on the device as RandomWalk._table_walk holds one: rows of stride ``V + pad`` (the
    padding poisoned with NaN), statistics from pdt_row_log_softmax_stats."""

    def __init__(self, case, pad):
        self.case, self.x32 = case, wp.make_table(case)
        self.rows = wp.Rows(self.x32)
        buf = torch.full((case.R, case.V + pad), float("nan"), device=DEV)
        buf[:, : case.V] = _dev(self.x32)
        self.table = buf[:, : case.V]
        assert self.table.stride() == (case.V + pad, 1)
        self.stats = torch.empty((case.R, 2), device=DEV)
        rc = _cabi.lib().pdt_row_log_softmax_stats(_cabi.ptr(self.table), self.table.stride(0), 1, case.R, case.V,
                                                   _cabi.ptr(self.stats), _cabi.stream_ptr(DEV))  # fmt: skip
        _cabi.check(rc, "pdt_row_log_softmax_stats")

    def launch(self, u, y, ctx, lens, ended, lp, ctl, eos):
        """One launch as RandomWalk._table_walk makes it; returns the report (bits, live, longest)."""
        c = self.case
        C, N = u.shape
        assert y.shape == (C, N) and y.is_contiguous() and u.is_contiguous()
        return _walk._walk_launch(
            DEV,
            lambda host: _cabi.lib().pdt_random_walk_table(
                _cabi.ptr(self.table), self.table.stride(0), c.R, c.U, c.V, _cabi.ptr(self.stats), _cabi.ptr(u), N, C,
                int(eos is not None), int(eos or 0), _cabi.ptr(y), _cabi.ptr(ctx), _cabi.ptr(lens), _cabi.ptr(ended),
                _cabi.ptr(lp), _cabi.ptr(ctl), host, _cabi.stream_ptr(DEV),
            ),
            "random walk table test",
        )  # fmt: skip


def _fresh(start):
    N = len(start)
    return (_dev(np.asarray(start, np.int64)), torch.zeros(N, dtype=torch.long, device=DEV),
            torch.zeros(N, dtype=torch.bool, device=DEV), torch.zeros(N, device=DEV),
            torch.zeros(4, dtype=torch.int32, device=DEV))  # fmt: skip


def _assert_state(plan, y, ctx, lens, ended, lp, report, what, eos):
    assert np.array_equal(y.cpu().numpy(), plan.y), what
    assert np.array_equal(lens.cpu().numpy(), plan.lens) and np.array_equal(ended.cpu().numpy(), plan.ended), what
    assert np.array_equal(ctx.cpu().numpy(), plan.ctx), what
    bits, live, longest = report
    assert (bits, live, longest) == (1, plan.live, plan.longest), what
    if eos is not None:  # after a walk's end: eos
        steps = np.arange(plan.y.shape[0])[:, None]
        assert (y.cpu().numpy()[steps >= plan.lens[None]] == eos).all(), what
    return _ratio(lp.cpu().numpy(), plan.lp, plan.bound, what)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("case", wp.TABLES, ids=[c.name for c in wp.TABLES])
def test_table_follows_the_plan(case, pad):
    """Every (C, N): the paths, the frozen state of ended walks, the final context row (the rotation, for the
    trigram table), the report; then the incoming ``ended`` with and without eos."""
    tb = _Table(case, pad)
    update = wp.table_update(case.U, case.R)
    worst = 0.0
    for C, N in itertools.product(wp.TABLE_C, wp.TABLE_N):
        rng = np.random.default_rng([9, C, N, pad])
        start = wp.start_rows(case, N)
        for eos in (case.eos, None):
            plan = wp.plan_walk(rng, tb.rows, update, start, C, eos, wp.end_steps(N))
            ctx, lens, ended, lp, ctl = _fresh(start)
            y = torch.full((C, N), -7, dtype=torch.long, device=DEV)
            report = tb.launch(_dev(plan.u), y, ctx, lens, ended, lp, ctl, eos)
            worst = max(worst, _assert_state(plan, y, ctx, lens, ended, lp, report, (case.name, C, N, eos), eos))
            assert not ctl.any()
    # walks that come ended: frozen with eos (the state keeps its bits), ignored without
    N, C = 9, 5
    start = wp.start_rows(case, N)
    ended0 = np.arange(N) % 2 == 1
    lens0, lp0 = np.arange(N) + 3, np.linspace(-9, -1, N).astype(np.float32)
    for eos in (case.eos, None):
        rng = np.random.default_rng([10, pad])
        plan = wp.plan_walk(rng, tb.rows, update, start, C, eos, np.full(N, wp.NEVER), ended0, lens0, lp0)
        ctx, _, _, _, ctl = _fresh(start)
        lens, ended, lp = _dev(lens0), _dev(ended0), _dev(lp0)
        y = torch.full((C, N), -7, dtype=torch.long, device=DEV)
        report = tb.launch(_dev(plan.u), y, ctx, lens, ended, lp, ctl, eos)
        got_lp = lp.cpu().numpy()
        if eos is None:
            assert plan.live == N and (plan.lens == lens0 + C).all() and not plan.ended.any()
            _assert_state(plan, y, ctx, lens, ended, lp, report, (case.name, "ended ignored"), eos)
        else:
            assert (plan.y[:, ended0] == eos).all() and np.array_equal(plan.ctx[ended0], start[ended0])
            assert np.array_equal(got_lp[ended0].view(np.int32), lp0[ended0].view(np.int32))
            _assert_state(plan, y, ctx, lens, ended, lp, report, (case.name, "ended kept"), eos)
    print("pdt_random_walk_table %s pad=%d: largest lp error / bound = %.3f" % (case.name, pad, worst))


@pytest.mark.parametrize("case", wp.TABLES, ids=[c.name for c in wp.TABLES])
def test_table_state_is_carried_between_launches(case):
    """130 iterations in one launch, and in launches of 64 and 66 with the state carried on the device: every
    output has the same bits, and both are the plan."""
    tb = _Table(case, 0)
    total, first, second = wp.SPLIT
    N = 130
    start = wp.start_rows(case, N)
    plan = wp.plan_walk(np.random.default_rng(11), tb.rows, wp.table_update(case.U, case.R), start, total, case.eos,
                        wp.end_steps(N))  # fmt: skip
    assert {"step0", "mid", "last_of_chunk", "first_of_next"} <= wp.end_kinds_met(plan, case.eos)
    u = _dev(plan.u)
    one = _fresh(start)
    y1 = torch.full((total, N), -7, dtype=torch.long, device=DEV)
    report1 = tb.launch(u, y1, *one, case.eos)
    two = _fresh(start)
    y2 = torch.full((total, N), -7, dtype=torch.long, device=DEV)
    mid = tb.launch(u[:first].contiguous(), y2[:first], *two, case.eos)
    # the state between the launches, from the plan: walks that ended in the first 64 iterations, the others' rows
    done = plan.ended & (plan.lens <= first)
    head_lens = np.minimum(plan.lens, first)
    assert 0 < done.sum() < N and mid == (1, int((~done).sum()), int(head_lens.max()))
    assert np.array_equal(two[2].cpu().numpy(), done) and np.array_equal(two[1].cpu().numpy(), head_lens)
    assert np.array_equal(two[0].cpu().numpy(), np.where(done, plan.ctx, plan.rows_at[first]))
    report2 = tb.launch(u[first:].contiguous(), y2[first:], *two, case.eos)
    assert report1 == report2 == (1, plan.live, plan.longest)
    assert torch.equal(y1, y2)
    for a, b in zip(one, two):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float else a, b.view(torch.int32) if b.dtype == torch.float else b)
    ratio = _assert_state(plan, y1, *one[:4], report1, (case.name, "split"), case.eos)
    print("pdt_random_walk_table %s 64+66: largest lp error / bound = %.3f" % (case.name, ratio))


def test_table_start_row_out_of_range_raises_and_the_others_walk_on():
    case = wp.TABLES[4]
    tb = _Table(case, 3)
    N, C = 7, 20
    start = wp.start_rows(case, N)
    plan = wp.plan_walk(np.random.default_rng(12), tb.rows, wp.table_update(case.U, case.R), start, C, case.eos,
                        wp.end_steps(N, 8))  # fmt: skip
    for bad_row in (case.R, -1):
        bad = start.copy()
        bad[[2, 5]] = bad_row
        ctx, lens, ended, lp, ctl = _fresh(bad)
        y = torch.full((C, N), -7, dtype=torch.long, device=DEV)
        with pytest.raises(RuntimeError, match="no positive finite mass"):
            tb.launch(_dev(plan.u), y, ctx, lens, ended, lp, ctl, case.eos)
        torch.cuda.synchronize()
        ok = np.array([n not in (2, 5) for n in range(N)])
        assert not ctl.any()
        assert np.array_equal(y.cpu().numpy()[:, ok], plan.y[:, ok]) and (y.cpu().numpy()[:, ~ok] == case.eos).all()
        assert np.array_equal(lens.cpu().numpy()[ok], plan.lens[ok]) and (lens.cpu().numpy()[~ok] == 0).all()
        assert np.array_equal(ctx.cpu().numpy()[ok], plan.ctx[ok]) and np.array_equal(ended.cpu().numpy()[ok], plan.ended[ok])
        assert (lp.cpu().numpy()[~ok] == 0).all()
        _ratio(lp.cpu().numpy()[ok], plan.lp[ok], plan.bound[ok], "beside a bad start row")
    # and the next launch on the same ctl reports as usual
    ctx, lens, ended, lp, _ = _fresh(start)
    report = tb.launch(_dev(plan.u), y, ctx, lens, ended, lp, ctl, case.eos)
    _assert_state(plan, y, ctx, lens, ended, lp, report, "after the error", case.eos)


@pytest.mark.parametrize("V", [1, 5, 64, 65, 300, 512, 513, 1100])
def test_row_statistics(V):
    """pdt_row_log_softmax_stats: the maximum is exact, the log-sum-exp within the derived bound."""
    x32 = wp.rows_of_every_kind(np.random.default_rng(V), 40, V)
    rows = wp.Rows(x32)
    worst = 0.0
    for pad in (0, 3):
        buf = torch.full((40, V + pad), float("nan"), device=DEV)
        buf[:, :V] = _dev(x32)
        stats = torch.empty((40, 2), device=DEV)
        rc = _cabi.lib().pdt_row_log_softmax_stats(_cabi.ptr(buf), V + pad, 1, 40, V, _cabi.ptr(stats), _cabi.stream_ptr(DEV))
        _cabi.check(rc, "pdt_row_log_softmax_stats")
        got = stats.cpu().numpy().astype(np.float64)
        assert np.array_equal(got[:, 0], rows.mx)
        ratio = np.abs(got[:, 1] - rows.lse) / rows.lse_bound
        assert ratio.max() <= 1.0, (V, pad, ratio.max())
        worst = max(worst, float(ratio.max()))
    print("pdt_row_log_softmax_stats V=%d: largest lse error / bound = %.3f" % (V, worst))


# ---- RandomWalk.forward ----------------------------------------------------------------------------------------


class _HookedWalk(M.RandomWalk):
    """An identity hook of its own: the random_walk_advance route."""

    def update_log_probs_for_step(self, log_probs_prev, log_probs_t, y_prev, y_prev_lens, eos_mask):
        return log_probs_prev, log_probs_t


def _model_rows(lm, V):
    """The bigram model's row for every context (row V: the start), from the model itself."""
    with torch.no_grad():
        first, _ = lm.calc_idx_log_probs(torch.empty((0, 1), dtype=torch.long, device=DEV), dict(), torch.tensor(0, device=DEV))
        hist = torch.arange(V, device=DEV).unsqueeze(0)
        rest, _ = lm.calc_idx_log_probs(hist, dict(), torch.tensor(1, device=DEV))
    return torch.cat([rest, first], 0).float().cpu().numpy()


FORWARD_ENDS = {
    "all_end": ("step0", "mid", "last_of_chunk", "first_of_next", "late"),
    "some_never": wp.END_KINDS,
    "no_eos": None,
}


@pytest.mark.parametrize("ends", list(FORWARD_ENDS))
def test_forward_follows_the_plan_on_every_route(ends, monkeypatch):
    """N = 96, max_iters = 200 (chunks at 0, 64 and 192), torch.rand((C, N)) on the device served from the plan
    in the chunk schedule: the table route, the per-iteration route and the random_walk_advance route each return
    the planned y and lens; the first two the planned log-probabilities within the bound."""
    V, N, max_iters = 40, 96, 200
    eos = None if ends == "no_eos" else 3
    lm = M.LookupLanguageModel(V, V, random_dicts(np.random.default_rng(31), V, 2, 0.6, sos=V)).to(DEV)
    rows = wp.Rows(_model_rows(lm, V))
    at = {"step0": 0, "mid": 31, "last_of_chunk": 63, "first_of_next": 64, "late": 100, "never": wp.NEVER}
    when = None if eos is None else np.array([at[FORWARD_ENDS[ends][n % 5]] for n in range(N)])
    plan = wp.plan_walk(np.random.default_rng(32), rows, lambda r, tok: tok, np.full(N, V), max_iters, eos, when)
    T = max_iters if eos is None else min(max_iters, plan.longest)
    if ends == "all_end":
        assert 100 < T < 192 and plan.live == 0
    else:
        assert T == max_iters and plan.live > 0
    assert eos is None or wp.end_kinds_met(plan, eos) >= {"step0", "mid", "last_of_chunk", "first_of_next"}
    u_dev = _dev(plan.u)
    real_rand = torch.rand
    served = []

    def planned_rand(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        device = kw.get("device")
        if len(shape) == 2 and shape[1] == N and device is not None and torch.device(device).type == "cuda":
            t = sum(served)
            assert shape[0] == _walk._walk_chunk(t, max_iters), (shape, t)
            served.append(shape[0])
            return u_dev[t : t + shape[0]].clone()
        return real_rand(*size, **kw)

    monkeypatch.setattr(torch, "rand", planned_rand)
    chunks = [c for _, c in wp.forward_chunks(max_iters)]
    routes = (("table", M.RandomWalk, 1), ("per-iteration", M.RandomWalk, 0), ("advance", _HookedWalk, 1))
    for name, cls, table in routes:
        walk = cls(lm, eos=eos).to(DEV)
        del served[:]
        with switches.override(PDT_WALK_TABLE=table):
            y, lens, lp = walk(None, N, max_iters)
        what = (ends, name)
        begun = sum(1 for t0, _ in wp.forward_chunks(max_iters) if t0 < T)
        assert served == chunks[:begun], (what, served)
        assert y.shape == (T, N) and np.array_equal(y.cpu().numpy(), plan.y[:T]), what
        assert np.array_equal(lens.cpu().numpy(), plan.lens), what
        if name != "advance":
            ratio = _ratio(lp.cpu().numpy(), plan.lp, plan.bound, what)
            print("RandomWalk.forward %s %s: largest lp error / bound = %.3f" % (ends, name, ratio))
        else:  # (torch's log_softmax, not walk_lp_add: the tolerance of test_random_walk_gpu.py for this route)
            assert np.allclose(lp.cpu().numpy(), plan.lp, rtol=1e-4, atol=1e-3), what
