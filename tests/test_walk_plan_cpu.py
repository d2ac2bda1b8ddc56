"""The plans of tests/test_random_walk_forms_gpu.py (tests/_walk_plan.py), checked without a GPU: for every planned
(row, uniform) the float64 rule returns the planned token, with u Z at least 1e-4 Z inside the token's interval; the
planned ends are of all five kinds; the state the plan reports is the state its path implies."""
import numpy as np
import pytest

import _walk_plan as wp


def _check(plan, rows, eos, update, start):
    steps, N = plan.y.shape
    r = np.asarray(start, np.int64).copy()
    ended = np.zeros(N, bool)
    lens = np.zeros(N, np.int64)
    lp = np.zeros(N)
    for t in range(steps):
        live = np.nonzero(~ended)[0]
        assert np.array_equal(plan.rows_at[t, live], r[live]) and (plan.rows_at[t, ended] == -1).all()
        if eos is not None:
            assert (plan.y[t, ended] == eos).all()
        tok = plan.y[t, live]
        assert np.array_equal(rows.rule(r[live], plan.u[t, live]), tok), t
        assert (rows.margin(r[live], tok, plan.u[t, live]) >= 1e-4).all(), t
        assert rows.ok[r[live], tok].all()
        for n in live[:: max(1, live.size // 3)]:  # ... and the rule as it is written for one row
            assert wp.rule(rows.x[r[n]], float(plan.u[t, n])) == plan.y[t, n]
        lp[live] += rows.lsm[r[live], tok]
        lens[live] += 1
        r[live] = update(r[live], tok)
        if eos is not None:
            ended[live] = tok == eos
    assert np.array_equal(plan.ctx, r) and np.array_equal(plan.lens, lens) and np.array_equal(plan.ended, ended)
    assert np.allclose(plan.lp, lp, rtol=1e-12, atol=0) and plan.live == int((~ended).sum())
    assert plan.longest == int(lens.max()) and (plan.u >= 0).all() and (plan.u < 1).all()
    assert (plan.bound[lens > 0] > 0).all() and np.isfinite(plan.bound).all()


@pytest.mark.parametrize("case", wp.TABLES, ids=[c.name for c in wp.TABLES])
def test_table_plans_draw_what_they_plan_and_end_in_every_way(case):
    rows = wp.Rows(wp.make_table(case))
    update = wp.table_update(case.U, case.R)
    met = set()
    for N in wp.TABLE_N:
        for C in (wp.TABLE_C[-1], wp.SPLIT[0]):
            rng = np.random.default_rng([7, N, C])
            start = wp.start_rows(case, N)
            plan = wp.plan_walk(rng, rows, update, start, C, case.eos, wp.end_steps(N))
            _check(plan, rows, case.eos, update, start)
            met |= wp.end_kinds_met(plan, case.eos)
            none = wp.plan_walk(rng, rows, update, start, 70, None)
            _check(none, rows, None, update, start)
            assert (none.lens == 70).all() and none.live == N and not none.ended.any()
    assert met == set(wp.END_KINDS), met
    if case.name.startswith("trigram"):  # the rotation is not the bigram's "row = last token"
        assert case.R == case.U**2 and (plan.ctx != plan.y[plan.lens - 1, np.arange(plan.y.shape[1])]).any()


def test_planned_ends_move_on_where_eos_lacks_the_mass():
    case = wp.TABLES[1]
    x = wp.make_table(case)
    x[:, case.eos] = -np.inf  # eos without mass everywhere but after token 7
    x[7, case.eos] = x[7].max()
    rows = wp.Rows(x)
    update = wp.table_update(case.U, case.R)
    plan = wp.plan_walk(np.random.default_rng(1), rows, update, wp.start_rows(case, 40), 400, case.eos, wp.end_steps(40))
    _check(plan, rows, case.eos, update, wp.start_rows(case, 40))
    for n in np.nonzero(plan.ended)[0]:
        L = int(plan.lens[n])
        assert L >= 2 and plan.y[L - 2, n] == 7 and plan.y[L - 1, n] == case.eos and (plan.y[:L - 1, n] != case.eos).all()


def test_end_steps_and_chunks():
    assert wp.end_steps(7).tolist() == [0, 31, 63, 64, wp.NEVER, 0, 31]
    assert wp.forward_chunks(200) == [(0, 64), (64, 128), (192, 8)] and wp.forward_chunks(64) == [(0, 64)]
    assert wp.forward_chunks(65) == [(0, 64), (64, 1)] and wp.forward_chunks(0) == []
    assert wp.SPLIT[0] == wp.SPLIT[1] + wp.SPLIT[2] and wp.SPLIT[1] == 64
    # the table kernel's sizes: one walk, a full workgroup, one more, many workgroups; iteration counts on both sides
    # of the chunk of 64 that the end kinds are planned around
    assert wp.TABLE_N == (1, 4, 5, 130) and wp.TABLE_C == (1, 2, 63, 64, 65, 200)
    assert [(c.U, c.V, c.R) for c in wp.TABLES] == [(6, 5, 6), (65, 64, 65), (66, 65, 66), (301, 300, 301), (7, 6, 49)]


@pytest.mark.parametrize("V", [1, 2, 64, 65, 513, 1100])
def test_rows_of_every_kind_and_their_bounds(V):
    rng = np.random.default_rng(V)
    x = wp.rows_of_every_kind(rng, 20, V)
    rows = wp.Rows(x)
    assert rows.ok.any(1).all() and np.allclose(np.exp(rows.lsm).sum(1), 1.0, rtol=1e-12)
    if V > 2:
        assert (np.isneginf(x).sum(1) == V - 1).sum() == 4  # the one-hot rows
        assert x[1].max() > 30 and x[4].max() < -30
    # a token and uniform chosen the old way are what the vectorised rule finds
    tok, u = wp._choose(rng, x)
    assert np.array_equal(rows.rule(np.arange(20), u), tok)
    # the bound of lse is never less than its two fixed terms: one roundoff per level of additions, expf's 3 ulp
    depth = -(-V // 64) + 6
    assert (rows.lse_bound >= (depth + 6) * wp.U32).all() and (rows.lse_bound < 1e-4).all()
    # ... and a float32 evaluation with the kernel's depth of additions (a lane's terms in turn, then six levels)
    # stays inside it
    for r in range(20):
        xr = x[r]
        mx = xr.max()
        e = np.exp((xr - mx).astype(np.float32)).astype(np.float32)
        lanes = np.zeros(64, np.float32)
        for v in range(V):
            lanes[v % 64] = np.float32(lanes[v % 64] + e[v])
        while lanes.size > 1:
            lanes = (lanes[0::2] + lanes[1::2]).astype(np.float32)
        lse32 = np.log(lanes[0]).astype(np.float32)
        assert abs(float(lse32) - rows.lse[r]) <= rows.lse_bound[r]
