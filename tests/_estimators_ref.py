"""What the estimator tests and tests/golden/make_estimators_golden.py share.

* :func:`reduce64`: the yardstick of the fused reductions -- each formula of ``include/pdt_amd.h`` ("Sample-axis
  reductions") restated in float64 torch with autograd, the clamp bounds rounded to the dtype under test.
* :func:`imh_loop`: the accept / reject chain as a Python loop over scalars.
* the golden cases: deterministic estimator runs.  :func:`drive` builds and runs the estimator of a case from a
  namespace (the reference's, when the golden maker runs; this package's in the tests), :func:`yardstick` restates
  the whole case in float64.  A replay proposal hands out recorded rows in order, however many a call asks for;
  :func:`noise` substitutes recorded uniforms for ``torch.rand`` / ``torch.rand_like``.

Deviations are in units of eps (1 + |value|), eps the dtype's under test.
"""
import contextlib
import math

import numpy as np
import torch

EPS_NINF = math.log(1.1754943508222875e-38) / 2
EPS_INF = math.log(3.4028234663852886e38) / 2
MEAN, SCORE, WEIGHTED = 0, 1, 2
W_LOGM, W_SELF, W_NONE = 0, 1, 2
GRADS = ("logits", "theta", "log_temp", "eta")


def f64(*ts):
    out = tuple(None if t is None else t.detach().to("cpu", torch.float64) for t in ts)
    return out[0] if len(out) == 1 else out


def rounded(x: float, dtype) -> float:
    """The Python scalar ``x`` as an operation on a ``dtype`` tensor sees it."""
    return float(torch.tensor(x, dtype=torch.float64).to(dtype))


def units(got, want, eps) -> float:
    got, want = f64(got), f64(want)
    if got.shape != want.shape:
        return math.inf
    fin = torch.isfinite(want)
    same = torch.isfinite(got) == fin
    odd = ~fin & ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    if not bool(same.all()) or bool(odd.any()):
        return math.inf
    if not bool(fin.any()):
        return 0.0
    return float(((got - want).abs() / (eps * (1 + want.abs())))[fin].max())


def upstream(shape, dtype=torch.float64):
    n = int(torch.Size(shape).numel())
    return torch.cos(0.7 * torch.arange(n, dtype=torch.float64)).reshape(shape).to(dtype)


# ---- the yardstick of the reductions ------------------------------------------------------------------------------
def _sum0(x):
    """``x.sum(0)`` with the value of an exactly rounded sum (math.fsum down every column) where that is finite."""
    s = x.sum(0)
    cols = x.detach().reshape(x.size(0), -1).t().tolist()
    exact = torch.tensor([math.fsum(c) if all(map(math.isfinite, c)) else math.nan for c in cols], dtype=torch.float64).reshape(s.shape)
    return s + torch.where(torch.isnan(exact), torch.zeros_like(s), exact - s.detach())


def _lse(x):
    m = x.max(0, keepdim=True)[0]
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return _sum0((x - m).exp()).log() + m.squeeze(0)


def reduce64(kind, is_log, mode, dtype, f, a=None, cz=None, c=None, lp=None, lq=None):
    """float64 inputs of shape ``(M,) + batch`` (``c``: ``batch``) -> the reduction over the sample axis."""
    M = f.size(0)
    if kind == MEAN:
        return _lse(f) - math.log(M) if is_log else _sum0(f) / M
    if kind == WEIGHTED:
        if mode == W_NONE:
            ell = lp
        else:
            d = lp - lq.detach()
            ell = d - _lse(d) if mode == W_SELF else d - math.log(M)
        return _lse(f + ell) if is_log else _sum0(f * ell.exp())
    lo, hi = rounded(EPS_NINF, dtype), rounded(EPS_INF, dtype)
    w = f
    if is_log:
        big = torch.finfo(dtype)
        x = f.max(0, keepdim=True)[0].clamp(big.min / 2, big.max / 2)
        e = lambda t: (t - x).clamp(lo, hi).exp()  # noqa: E731
        w = e(f)
        a = None if a is None else e(a)
        c = None if c is None else e(c.unsqueeze(0))
        cz = None if cz is None else e(cz)
    if a is not None:
        w = w - a
    if c is not None:
        w = w + c
    el = w if cz is None else w + cz
    mu = _sum0(el) / M
    score = (w.detach() * lp).sum(0) / M
    if is_log:
        mu = mu.clamp_min(rounded(math.exp(EPS_NINF), dtype))
        score = score / mu.detach()
        return mu.log() + x.squeeze(0) + (score - score.detach())
    return mu + (score - score.detach())


def imh_loop(ratio, ratio0, log_u):
    """(idx, last, last_idx) of the chain over ``(M, B)`` CPU tensors, a scalar at a time in their own dtype."""
    r, u = ratio.numpy(), log_u.numpy()
    M, B = r.shape
    idx = torch.empty((M, B), dtype=torch.int32)
    last, cur = ratio0.clone(), torch.full((B,), -1, dtype=torch.int32)
    ix, la, cu = idx.numpy(), last.numpy(), cur.numpy()
    with np.errstate(invalid="ignore"):
        for b in range(B):
            for n in range(M):
                if (r[n, b] - la[b]) > u[n, b]:  # (one subtraction and one comparison in the data's dtype)
                    la[b], cu[b] = r[n, b], n
                ix[n, b] = cu[b]
    return idx, last, cur


# ---- deterministic proposals --------------------------------------------------------------------------------------
@contextlib.contextmanager
def noise(*tensors):
    """torch.rand and torch.rand_like return ``tensors`` in order (on the device and in the dtype asked for)."""
    queue = list(tensors)
    saved = torch.rand, torch.rand_like

    def pop(shape, dtype, device):
        t = queue.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.to(device=device, dtype=dtype or torch.float32).clone()

    torch.rand = lambda *shape, **kw: pop(shape[0] if len(shape) == 1 and not isinstance(shape[0], int) else shape,
                                          kw.get("dtype"), kw.get("device") or "cpu")
    torch.rand_like = lambda t, **kw: pop(t.shape, t.dtype, t.device)
    try:
        yield
        assert not queue
    finally:
        torch.rand, torch.rand_like = saved


class ReplayCategorical(torch.distributions.Distribution):
    """``sample`` hands out the recorded rows (class indices) in order; ``log_prob`` is the categorical's."""

    arg_constraints = {}
    has_rsample = False

    def __init__(self, logits, rows):
        self.logits, self.rows, self.at = logits.log_softmax(-1), rows, 0
        super().__init__(logits.shape[:-1], validate_args=False)

    def sample(self, sample_shape=torch.Size()):
        n = int(torch.Size(sample_shape).numel())
        out, self.at = self.rows[self.at : self.at + n], self.at + n
        assert out.size(0) == n
        return out

    def log_prob(self, value):
        return self.logits.expand(value.shape + self.logits.shape[-1:]).gather(-1, value.unsqueeze(-1)).squeeze(-1)


class ReplayNormal(torch.distributions.Distribution):
    """``rsample`` is ``loc`` plus the recorded rows, in order."""

    arg_constraints = {}
    has_rsample = True

    def __init__(self, loc, rows):
        self.loc, self.rows, self.at = loc, rows, 0
        super().__init__(loc.shape, validate_args=False)

    def rsample(self, sample_shape=torch.Size()):
        n = int(torch.Size(sample_shape).numel())
        out, self.at = self.rows[self.at : self.at + n], self.at + n
        return self.loc + out


def table_func(theta, w):
    return lambda b: theta * w[b]


def onehot_func(theta, w):
    return lambda x: theta * (x * w).sum(-1)


def square_func(theta, w):
    return lambda x: theta * (x - w) ** 2


def smooth_func(theta):
    return lambda z: theta * torch.sin(z) + 0.1 * z


CV_SCALE, START_TEMP, START_ETA = 0.7, 0.5, 0.8


def leaves(case, T):
    """The tensors a case differentiates with respect to, fresh leaves."""
    return {k: T[k].clone().requires_grad_(True) for k in ("logits", "theta")}


def drive(ns, case, T):
    """Run the estimator of ``case`` from namespace ``ns`` (attributes E, D, M: the estimators, distributions and
    modules namespaces) on the tensors ``T``.  Returns (v, {name: gradient})."""
    E, est, M, is_log = ns.E, case["est"], case["M"], case["is_log"]
    L = leaves(case, T)
    logits, theta = L["logits"], L["theta"]
    extra = []
    if est == "direct":
        prop = ReplayCategorical(logits, T["rows"])
        kw = {}
        if case["cv"]:
            kw = dict(cv=lambda b: CV_SCALE * T["w2"][b], cv_mean=CV_SCALE * (logits.softmax(-1) * T["w2"]).sum(-1))
        run = E.DirectEstimator(prop, table_func(theta, T["w"]), M, is_log=is_log, **kw)
    elif est == "reparam":
        run = E.ReparameterizationEstimator(ReplayNormal(logits, T["rows"]), smooth_func(theta), M, is_log)
    elif est == "st":
        run = E.StraightThroughEstimator(ns.D.LogisticBernoulli(logits=logits), square_func(theta, T["w"]), M, is_log)
        extra = [T["u"]]
    elif est == "is":
        prop = ReplayCategorical(T["qlogits"], T["rows"])
        density = torch.distributions.Categorical(logits=logits)
        run = E.ImportanceSamplingEstimator(prop, table_func(theta, T["w"]), M, density, case["self_normalize"], is_log)
    elif est == "imh":
        prop = ReplayCategorical(T["qlogits"], T["rows"])
        density = torch.distributions.Categorical(logits=logits)
        run = E.IndependentMetropolisHastingsEstimator(
            prop, table_func(theta, T["w"]), M, density, case["burn_in"], is_log=is_log)
        extra = [T["u"]]
    elif est == "enumerate":
        run = E.EnumerateEstimator(torch.distributions.Categorical(logits=logits), table_func(theta, T["w"]), is_log)
    else:  # relax
        if case["family"] == "gumbel":
            prop, func = ns.D.GumbelOneHotCategorical(logits=logits), onehot_func(theta, T["w"])
            cv = ns.M.GumbelOneHotCategoricalRebarControlVariate(func, START_TEMP, START_ETA)
        else:
            prop, func = ns.D.LogisticBernoulli(logits=logits), square_func(theta, T["w"])
            cv = ns.M.LogisticBernoulliRebarControlVariate(func, START_TEMP, START_ETA)
        cv = cv.to(device=logits.device, dtype=logits.dtype)
        L["log_temp"], L["eta"] = cv.log_temp, cv.eta
        kw = dict(proposal_params=(logits,), cv_params=(cv.log_temp, cv.eta)) if case["varmin"] else {}
        run = E.RelaxEstimator(prop, func, M, cv, is_log=is_log, **kw)
        extra = [T["u"], T["nv"]]
    with noise(*extra):
        v = run()
    grads = {}
    if est != "imh":
        names = list(L)
        gs = torch.autograd.grad(v, [L[n] for n in names], upstream(v.shape, v.dtype).to(v.device), allow_unused=True)
        grads = {n: (torch.zeros_like(L[n]) if g is None else g) for n, g in zip(names, gs)}
    return v, grads


def _cat_lp(logits, rows):
    lsm = logits.log_softmax(-1)
    return lsm.expand(rows.shape + lsm.shape[-1:]).gather(-1, rows.unsqueeze(-1)).squeeze(-1)


def yardstick(case, T):
    """The case in float64: (v, {name: gradient}).  ``T`` holds CPU tensors in the dtype under test."""
    est, M, is_log = case["est"], case["M"], case["is_log"]
    dtype = getattr(torch, case["dtype"])
    eps = float(torch.finfo(dtype).eps)
    D = {k: (t if t.dtype in (torch.int64, torch.uint8) else f64(t)) for k, t in T.items()}
    L = {k: D[k].clone().requires_grad_(True) for k in ("logits", "theta")}
    logits, theta, w = L["logits"], L["theta"], D.get("w")
    if est == "direct":
        rows = D["rows"]
        a = c = None
        if case["cv"]:
            a, c = CV_SCALE * D["w2"][rows], CV_SCALE * (logits.softmax(-1) * D["w2"]).sum(-1)
        v = reduce64(SCORE, is_log, 0, dtype, theta * w[rows], a=a, c=c, lp=_cat_lp(logits, rows))
        v = v.unsqueeze(0) if is_log else v
    elif est == "reparam":
        v = reduce64(MEAN, is_log, 0, dtype, smooth_func(theta)(logits + D["rows"]))
    elif est == "st":
        u = D["u"]
        z = logits + u.log() - (-u).log1p()
        b = D["b"] + z - z.detach()
        v = reduce64(MEAN, is_log, 0, dtype, square_func(theta, w)(b))
    elif est in ("is", "imh"):
        rows = D["rows"]
        lp, lq = _cat_lp(logits, rows), _cat_lp(D["qlogits"], rows)
        f = theta * w[rows]
        if est == "is":
            v = reduce64(WEIGHTED, is_log, W_SELF if case["self_normalize"] else W_LOGM, dtype, f, lp=lp, lq=lq)
        else:
            ratio = (lp - lq).detach()
            batch = ratio.shape[1:]
            idx, _, _ = imh_loop(ratio[1:].reshape(M, -1), ratio[0].reshape(-1), f64(T["u"].log()).reshape(M, -1))
            chain = f.detach().reshape(M + 1, -1).gather(0, idx[case["burn_in"] :].long() + 1)
            v = reduce64(MEAN, is_log, 0, dtype, chain).reshape(batch)
    elif est == "enumerate":
        V = logits.size(-1)
        rows = torch.arange(V).reshape((V,) + (1,) * (logits.dim() - 1)).expand((V,) + logits.shape[:-1])
        v = reduce64(WEIGHTED, is_log, W_NONE, dtype, theta * w[rows], lp=_cat_lp(logits, rows))
    else:
        u, nv, b = D["u"], D["nv"], D["b"]
        # (the control variates initialise their parameters in float32, whatever they are cast to afterwards)
        L["log_temp"] = torch.full((1,), START_TEMP, dtype=torch.float32).log().double().requires_grad_(True)
        L["eta"] = torch.full((1,), START_ETA, dtype=torch.float32).double().requires_grad_(True)
        if case["family"] == "gumbel":
            func = onehot_func(theta, w)
            ln = logits.log_softmax(-1)
            z = ln - (-u.log()).log()
            log_v, probs = nv.log(), ln.exp()
            hot = -(-log_v).log() * b
            rest = -(-log_v / probs - (log_v * b).sum(-1, keepdim=True)).log()
            zcond = hot + torch.min(hot.sum(-1, keepdim=True) - eps, rest) * (1 - b)
            lp = (ln * b).sum(-1)
            cv = lambda x: L["eta"] * func((x / L["log_temp"].exp()).softmax(-1))  # noqa: E731
        else:
            func = square_func(theta, w)
            z = logits + u.log() - (-u).log1p()
            p = logits.sigmoid()
            t = nv / ((1 - nv) * ((1 - b) * p + b * (1 - p))) + 1
            zcond = (2 * b - 1) * t.log() + b * eps
            lp = b * logits - torch.nn.functional.softplus(logits)
            cv = lambda x: L["eta"] * func((x / L["log_temp"].exp()).sigmoid())  # noqa: E731
        fb, cvz, cvzcond = func(b), cv(z), cv(zcond)
        v = reduce64(SCORE, is_log, 0, dtype, fb, a=cvzcond, cz=cvz, lp=lp)
        if case["varmin"]:
            assert not is_log
            v_ = ((fb - cvzcond) * lp + cvz).sum(0) / M
            (gp,) = torch.autograd.grad(v_, logits, torch.ones_like(v_), create_graph=True)
            attached = torch.autograd.grad(gp.norm(2), (L["log_temp"], L["eta"]), retain_graph=True)
    if est == "imh":
        return v, {}
    names = list(L)
    gs = torch.autograd.grad(v, [L[n] for n in names], upstream(v.shape), allow_unused=True)
    grads = {n: (torch.zeros_like(L[n]) if g is None else g) for n, g in zip(names, gs)}
    if est == "relax" and case["varmin"]:
        grads["log_temp"], grads["eta"] = attached
    return v, grads
