"""Planned random walks: the tokens a walk draws are chosen first, then the uniforms that force them.

The sampling rule of csrc/row_sample.hpp is restated in numpy float64 (``rule``): for a row x and a uniform u,
with w = exp(x - max x) and Z = sum w, the token is the smallest v with w_v > 0 whose running prefix sum of w
exceeds u Z, else the largest v with w_v > 0.  A planned token holds at least 5e-4 of its row's mass and its
uniform lies in the middle 60 % of the token's interval, at least 1e-4 Z from both ends, so that float32 rounding
cannot move the draw.  ``plan_walk`` plans whole walks over a table of rows: per walk the step at which it draws
eos, the context row after every token, the float64 log-probability of the path and a bound on the error of the
kernels' float32 one.  Conditions on the plans that need no GPU: tests/test_walk_plan_cpu.py.

The bound (``Rows.step_bound``, ``Rows.lse_bound``), derived from the code.  u = 2^-24 is float32's unit
roundoff and g(n) = n u / (1 - n u).

* ``walk_lp_add`` (row_sample.hpp) forms ``lp + ((x_tok - mx) - lse)``: three float32 roundings, of results of the
  magnitudes |x_tok - mx|, |(x_tok - mx) - lse| and |lp'|.  x_tok and mx (a maximum: exact) are float32 numbers, so
  one step adds at most u (|x_tok - mx| + |(x_tok - mx) - lse| + |lp'|) (1 + 3 u) to the error, plus the error of
  lse, which passes through the two subtractions unchanged.
* ``lse = logf(s)``, s the float32 sum of e_v = expf(x_v - mx) (``row_log_softmax_stats``).  x_v - mx is rounded:
  an absolute error of u |x_v - mx| in the argument, a relative one of the same size in e_v.  expf and logf are
  the device library's, which is built to OpenCL's accuracy requirement of 3 ulp, 6 u relative.  A lane adds its
  ceil(V / 64) terms one after the other and the wave's six levels of additions follow, so a term passes through at
  most D = ceil(V / 64) + 6 additions: all terms are positive, and the sum's relative error is at most g(D).  So
  s = S (1 + e), |e| <= E = g(D) + 6 u + u sum_v w_v |x_v - mx| / S (and second-order terms: times 1 + 2^-10),
  |log s - log S| <= E / (1 - E), and logf adds 6 u |lse|.

A walk's bound is the sum over its steps.  The largest error-to-bound ratios the GPU tests have measured are
recorded in DESIGN.md; one above 1 means this derivation or the kernel is wrong.
"""
from collections import namedtuple

import numpy as np

U32 = 2.0**-24
MIN_MASS = 5e-4
FRAC = (0.2, 0.8)
LIB_ULP = 3  # OpenCL's bound for exp and log in single precision


def rule(x, u):
    x = np.asarray(x, np.float64)
    w = np.exp(x - x.max())
    P = np.cumsum(w)
    hit = np.nonzero((P > u * P[-1]) & (w > 0))[0]
    return int(hit[0]) if hit.size else int(np.nonzero(w > 0)[0][-1])


def u_inside(x, tok, frac):
    """A uniform whose draw from row x is token ``tok``: ``frac`` of the way through its interval."""
    x = np.asarray(x, np.float64)
    w = np.exp(x - x.max())
    return (w[:tok].sum() + frac * w[tok]) / w.sum()


def _choose(rng, x):
    """(token, u) per row: a token of at least 5e-4 of the row's mass, u in its middle 60%."""
    toks, us = [], []
    for row in x:
        w = np.exp(row.astype(np.float64) - row.max())
        ok = np.nonzero(w / w.sum() >= 5e-4)[0]
        k = int(rng.choice(ok))
        toks.append(k)
        us.append(u_inside(row, k, rng.uniform(0.2, 0.8)))
    return np.array(toks), np.array(us, np.float32)


def rows_of_every_kind(rng, R, V):
    """(R, V) float32 rows: plain, unnormalised by +40 and by -40, with -inf entries, one-hot (the kinds of
    test_random_walk_gpu._rows and the shift downwards)."""
    x = rng.normal(size=(R, V)) * 2.0
    kind = np.arange(R) % 5
    x[kind == 1] += 40.0
    x[kind == 4] -= 40.0
    holes = (rng.random((R, V)) < 0.4) & (kind == 2)[:, None]
    holes[holes.all(1), 0] = False
    x[holes] = -np.inf
    for n in np.nonzero(kind == 3)[0]:
        x[n] = -np.inf
        x[n, rng.integers(V)] = 0.0
    return x.astype(np.float32)


class Rows:
    """Float32 rows (R, V), each with positive finite mass, in float64: the rule's weights and prefix sums, the
    tokens that may be planned, log_softmax, and the error bounds of the module docstring."""

    def __init__(self, x):
        x = np.asarray(x)
        assert x.dtype == np.float32 and x.ndim == 2
        self.x = x.astype(np.float64)
        self.R, self.V = x.shape
        self.mx = self.x.max(1)
        assert np.isfinite(self.mx).all() and not np.isnan(self.x).any()
        d = self.x - self.mx[:, None]
        self.w = np.exp(d)
        self.P = np.cumsum(self.w, 1)
        self.Z = self.P[:, -1]
        self.ok = self.w / self.Z[:, None] >= MIN_MASS
        self.lse = np.log(self.Z)
        with np.errstate(invalid="ignore"):
            self.lsm = d - self.lse[:, None]
            wd = np.where(self.w > 0, self.w * np.abs(d), 0.0).sum(1) / self.Z
        depth = -(-self.V // 64) + 6
        E = (depth * U32 / (1 - depth * U32) + 2 * LIB_ULP * U32 + U32 * wd) * (1 + 2.0**-10)
        self.lse_bound = E / (1 - E) + 2 * LIB_ULP * U32 * np.abs(self.lse)

    def step_bound(self, r, tok, lp_after):
        """The error one step (token ``tok`` of row ``r``, the path's log-probability ``lp_after`` behind it) can
        add to a walk's float32 log-probability."""
        a = np.abs(self.x[r, tok] - self.mx[r])
        b = np.abs(self.lsm[r, tok])
        return U32 * (a + b + np.abs(lp_after)) * (1 + 3 * U32) + self.lse_bound[r]

    def draw(self, rng, r, eos=None, want_eos=None):
        """Plan one token for each walk standing at row ``r[n]``: eos where ``want_eos[n]`` and eos holds the mass
        (or where nothing else does), else a token other than eos; then the float32 uniform that draws it."""
        r = np.asarray(r)
        n = r.shape[0]
        cand = self.ok[r].copy()
        took_eos = np.zeros(n, bool)
        if eos is not None:
            has = cand[:, eos].copy()
            cand[:, eos] = False
            took_eos = has & (np.asarray(want_eos, bool) | ~cand.any(1))
            cand[took_eos] = False
            cand[took_eos, eos] = True
        assert cand.any(1).all()
        # the k-th candidate of each row, k uniform
        k = np.floor(rng.random(n) * cand.sum(1)).astype(np.int64)
        tok = (np.cumsum(cand, 1) > k[:, None]).argmax(1)
        assert cand[np.arange(n), tok].all()
        frac = rng.uniform(FRAC[0], FRAC[1], n)
        w = self.w[r, tok]
        u = ((self.P[r, tok] - w) + frac * w) / self.Z[r]
        return tok, u.astype(np.float32)

    def rule(self, r, u):
        """``rule`` for every (row r[n], uniform u[n]) at once."""
        r = np.asarray(r)
        u = np.asarray(u, np.float64)
        w = self.w[r]
        hit = (self.P[r] > (u * self.Z[r])[:, None]) & (w > 0)
        last = self.V - 1 - (w[:, ::-1] > 0).argmax(1)
        return np.where(hit.any(1), hit.argmax(1), last)

    def margin(self, r, tok, u):
        """How far u Z lies inside the token's interval, in units of Z (the smaller of the two distances)."""
        u = np.asarray(u, np.float64)
        hi = self.P[r, tok]
        lo = hi - self.w[r, tok]
        t = u * self.Z[r]
        return np.minimum(t - lo, hi - t) / self.Z[r]


END_KINDS = ("step0", "mid", "last_of_chunk", "first_of_next", "never")
NEVER = 1 << 30


def end_steps(n_walks, chunk=64, kinds=END_KINDS):
    """The step at which each walk is to draw eos, the five kinds dealt in turn: step 0, the middle of the first
    chunk, its last step, the first step of the next chunk, never."""
    at = {"step0": 0, "mid": chunk // 2 - 1, "last_of_chunk": chunk - 1, "first_of_next": chunk, "never": NEVER}
    return np.array([at[kinds[n % len(kinds)]] for n in range(n_walks)], np.int64)


Plan = namedtuple("Plan", "y u rows_at ctx lens ended lp bound live longest")


def table_update(U, R):
    """The context rotation of pdt_random_walk_table: r' = (r U + token) mod R."""
    return lambda r, tok: (r * U + tok) % R


def plan_walk(rng, rows, update, start, steps, eos=None, ends=None, ended=None, lens=None, lp=None):
    """``steps`` iterations of len(start) walks over ``rows`` (a Rows), walk n starting at row ``start[n]`` and
    moving to ``update(row, token)`` after each token.  With ``eos``, walk n draws eos at step ``ends[n]`` or, where
    eos lacks the mass in that context, at the next step where it has it; from then on its tokens are eos and its
    state is frozen.  ``ended`` / ``lens`` / ``lp``: the state the walks come with (default: fresh).

    Returns Plan(y (steps, N), u (steps, N) float32, rows_at (steps, N): the row each token was drawn from (-1:
    the walk had ended), ctx (N,) the final rows, lens, ended, lp (float64), bound, live, longest)."""
    start = np.asarray(start, np.int64)
    N = start.shape[0]
    r = start.copy()
    ended = np.zeros(N, bool) if ended is None or eos is None else np.asarray(ended, bool).copy()
    lens = np.zeros(N, np.int64) if lens is None else np.asarray(lens, np.int64).copy()
    lp = np.zeros(N, np.float64) if lp is None else np.asarray(lp, np.float64).copy()
    ends = np.full(N, NEVER, np.int64) if ends is None else np.asarray(ends, np.int64)
    bound = np.zeros(N, np.float64)
    y = np.zeros((steps, N), np.int64)
    u = rng.random((steps, N)).astype(np.float32)  # (an ended walk's uniform is never used: any value)
    rows_at = np.full((steps, N), -1, np.int64)
    for t in range(steps):
        y[t] = 0 if eos is None else eos
        live = np.nonzero(~ended)[0]
        if live.size == 0:
            continue
        tok, ut = rows.draw(rng, r[live], eos, None if eos is None else t >= ends[live])
        y[t, live], u[t, live], rows_at[t, live] = tok, ut, r[live]
        lp[live] += rows.lsm[r[live], tok]
        bound[live] += rows.step_bound(r[live], tok, lp[live])
        lens[live] += 1
        r[live] = update(r[live], tok)
        if eos is not None:
            ended[live] = tok == eos
    return Plan(y, u, rows_at, r, lens, ended, lp, bound, int((~ended).sum()), int(lens.max()) if N else 0)


def end_kinds_met(plan, eos, chunk=64):
    """Which of END_KINDS the plan's walks ended in, from where each walk's eos was drawn."""
    met = set()
    for n in range(plan.y.shape[1]):
        if not plan.ended[n]:
            met.add("never")
            continue
        t = int(plan.lens[n]) - 1
        assert plan.y[t, n] == eos
        if t == 0:
            met.add("step0")
        elif t % chunk == chunk - 1:
            met.add("last_of_chunk")
        elif t % chunk == 0:
            met.add("first_of_next")
        else:
            met.add("mid")
    return met


# ---- the hand-made tables of the table kernel's test -----------------------------------------------------------

TableCase = namedtuple("TableCase", "name R U V eos")
TABLES = (
    TableCase("bigram5", 6, 6, 5, 3),
    TableCase("bigram64", 65, 65, 64, 3),
    TableCase("bigram65", 66, 66, 65, 64),
    TableCase("bigram300", 301, 301, 300, 0),
    TableCase("trigram6", 49, 7, 6, 3),
)
TABLE_C = (1, 2, 63, 64, 65, 200)
TABLE_N = (1, 4, 5, 130)
SPLIT = (130, 64, 66)  # one launch of 130 iterations against launches of 64 and 66


def make_table(case, seed=0):
    """The case's (R, V) float32 rows: rows_of_every_kind, then every row is given a second token with mass (so
    that no walk is caught in a chain of one-hot rows) and eos the row's largest score -- but in every seventh row,
    where eos is -inf and a planned end has to move on to a later step."""
    rng = np.random.default_rng([5, seed, case.R, case.V])
    x = rows_of_every_kind(rng, case.R, case.V)
    top = x.max(1)
    for r in range(case.R):
        other = (r + 1) % case.V
        other = other if other != case.eos else (other + 1) % case.V
        if not np.isfinite(x[r, other]):
            x[r, other] = top[r] - 1.0
        x[r, case.eos] = -np.inf if r % 7 == 5 else top[r]
    return x


def start_rows(case, N):
    """Every walk its own start row, the last row (a bigram model's sos) first."""
    return (case.R - 1 - 5 * np.arange(N)) % case.R


def forward_chunks(max_iters):
    """The (start, length) of RandomWalk's chunks: 64, 128, ... cut off at max_iters."""
    out, t = [], 0
    while t < max_iters:
        c = min(min(t + 64, 4096), max_iters - t)
        out.append((t, c))
        t += c
    return out
