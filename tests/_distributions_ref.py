"""The formulas of the relaxed distributions, stated once in float64 torch ops: the yardstick of
tests/test_distributions_*.py and of tests/golden/make_distributions_golden.py.

Every function takes float64 tensors (``f64`` converts) and is differentiable as often as wanted.  ``eps`` is
the machine epsilon of the dtype UNDER TEST, not of float64: the distributions clamp probabilities and noise
to ``[eps, 1 - eps]`` of their own dtype and add or subtract that ``eps``, so a float32 result has to be held
against a float64 evaluation that clamps where float32 does.

Shapes: parameters ``batch + (V,)`` (Gumbel) or ``batch`` (logistic), data ``sample + `` that; broadcasting is
torch's.  ``units`` is the measure of every comparison: |a - b| in multiples of ``eps * (1 + |b|)``.
"""
import math

import torch


def f64(*ts):
    out = tuple(None if t is None else t.detach().double() for t in ts)
    return out[0] if len(out) == 1 else out


def units(got, want, eps):
    """max |got - want| / (eps (1 + |want|)) over the finite entries of ``want``; infinities must agree."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin], want[~fin])
    if not fin.any():
        return 0.0
    return float(((got[fin] - want[fin]).abs() / (eps * (1 + want[fin].abs()))).max())


def clamp(x, eps):
    return x.clamp(eps, 1 - eps)


def one_hot_argmax(z):
    return torch.nn.functional.one_hot(z.argmax(-1), z.shape[-1]).to(z)


# ---- Gumbel / one-hot categorical -------------------------------------------------------------------------------
def gumbel_logits(param, from_probs, eps):
    """The normalised logits of a distribution built from ``param`` (logits, or probs)."""
    if from_probs:
        return clamp(param / param.sum(-1, keepdim=True), eps).log()
    return param.log_softmax(-1)


def gumbel_probs(param, from_probs):
    return param / param.sum(-1, keepdim=True) if from_probs else param.softmax(-1)


def gumbel_rsample(logits, u, eps):
    return logits - torch.log(-torch.log(clamp(u, eps)))


def gumbel_tlog_prob(logits, b):
    return torch.where(b != 0, logits.expand_as(b), logits.new_zeros(())).sum(-1)


def gumbel_guard(probs, b, v, eps):
    """Where off the hot index the free value lies above z_k - eps, so that the min guard decides."""
    lv = torch.log(clamp(v, eps))
    lvk = (lv * b).sum(-1, keepdim=True)
    free = -torch.log(-lv / clamp(probs, eps) - lvk)
    return (free > -torch.log(-lvk) - eps) & (b == 0)


def gumbel_csample(probs, b, v, eps):
    lv = torch.log(clamp(v, eps))
    lvk = (lv * b).sum(-1, keepdim=True)
    zk = -torch.log(-lvk)
    free = -torch.log(-lv / clamp(probs, eps) - lvk)
    return torch.where(b != 0, zk.expand_as(free), torch.minimum(zk - eps, free))


def gumbel_log_prob(logits, z):
    g = logits - z
    return (g - g.exp()).sum(-1)


def gumbel_clog_prob(logits, zcond, b):
    hit = (one_hot_argmax(zcond) == b).all(-1)
    zk = (zcond * b).sum(-1, keepdim=True)
    g = logits - zcond
    off = g - g.exp() + (logits - zk).exp()
    lp = torch.where(b != 0, -zk - (-zk).exp(), off).sum(-1)
    return torch.where(hit, lp, lp.new_full((), -math.inf))


# ---- logistic / Bernoulli --------------------------------------------------------------------------------------
def bernoulli_logits(param, from_probs, eps):
    if from_probs:
        p = clamp(param, eps)
        return p.log() - (-p).log1p()
    return param


def bernoulli_probs(param, from_probs):
    return param if from_probs else param.sigmoid()


def bernoulli_rsample(logits, u, eps):
    u = clamp(u, eps)
    return logits + u.log() - (-u).log1p()


def bernoulli_threshold(z):
    return (z >= 0).to(z)


def bernoulli_tlog_prob(logits, b):
    return b * logits - torch.nn.functional.softplus(logits)


def bernoulli_csample(probs, b, v, eps):
    v, p = clamp(v, eps), clamp(probs, eps)
    q = torch.where(b != 0, 1 - p, p)
    mag = torch.log1p(v / ((1 - v) * q))
    return torch.where(b != 0, mag + eps, -mag)


def bernoulli_log_prob(logits, z):
    d = logits - z
    return d - 2 * torch.nn.functional.softplus(d)


def bernoulli_clog_prob(logits, zcond, b):
    sp = torch.nn.functional.softplus
    lp = -zcond + (1 - b) * logits + sp(logits) - 2 * sp(logits - zcond)
    return torch.where(bernoulli_threshold(zcond) == b, lp, lp.new_full((), -math.inf))


FAMILY = {
    "gumbel": dict(
        logits=gumbel_logits, probs=gumbel_probs, rsample=gumbel_rsample, threshold=one_hot_argmax,
        tlog_prob=gumbel_tlog_prob, csample=gumbel_csample, log_prob=gumbel_log_prob, clog_prob=gumbel_clog_prob,
    ),
    "bernoulli": dict(
        logits=bernoulli_logits, probs=bernoulli_probs, rsample=bernoulli_rsample, threshold=bernoulli_threshold,
        tlog_prob=bernoulli_tlog_prob, csample=bernoulli_csample, log_prob=bernoulli_log_prob,
        clog_prob=bernoulli_clog_prob,
    ),
}


CONTINUOUS = ("z", "zcond", "log_prob", "tlog_prob", "clog_prob")
WRT = dict(z="logits", zcond="probs", log_prob="logits", tlog_prob="logits", clog_prob="logits")


def upstream(shape, dtype=torch.float64):
    n = 1
    for s in shape:
        n *= s
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(tuple(shape)).to(dtype)


def exact_sum_to_size(t, shape):
    """``t.sum_to_size(shape)`` over the leading (sample) dimensions by compensated (Neumaier) summation: the
    yardstick of a sum must not carry a summation error of the size it is to judge."""
    rows = t.reshape((-1,) + tuple(shape))
    total, comp = torch.zeros(shape, dtype=t.dtype), torch.zeros(shape, dtype=t.dtype)
    for x in rows:
        s = total + x
        comp = comp + torch.where(total.abs() >= x.abs(), (total - s) + x, (x - s) + total)
        total = s
    return total + comp


def evaluate(family, param, from_probs, u, v, eps, z_in=None, b=None, zcond_in=None, grads=True, at=None):
    """One case from float64 inputs: ``(outs, grads)``.

    ``outs``: ``z, b, zcond, log_prob, tlog_prob, clog_prob``.  ``z_in``, ``b`` and ``zcond_in`` are what the
    methods downstream of a draw are given -- the recorded values of the code under test, so that every method
    is judged on the inputs it really had; left out, each method is fed the exact result of the one before.

    ``grads["g_<out>"]``: d <out, cos(0.7 n)> / d (the distribution's own ``logits``, or its ``probs`` for
    ``zcond``: ``WRT``), the tensor the method reads.  ``at = dict(logits=, probs=)`` gives the values of those
    tensors in the distribution under test (float64 copies): the gradient is a function of them, and torch's
    normalisation in front of them rounds differently from device to device, which is no property of the
    method.  Left out, they are computed from ``param``.
    """
    f = FAMILY[family]
    logits0, probs0 = f["logits"](param, from_probs, eps).detach(), f["probs"](param, from_probs).detach()
    z = f["rsample"](logits0, u, eps)
    z_in = z if z_in is None else z_in
    b = f["threshold"](z_in) if b is None else b
    zc = f["csample"](probs0, b, v, eps)
    zcond_in = zc if zcond_in is None else zcond_in
    outs = dict(z=z, b=b, zcond=zc, log_prob=f["log_prob"](logits0, z_in), tlog_prob=f["tlog_prob"](logits0, b),
                clog_prob=f["clog_prob"](logits0, zcond_in, b))
    g = {}
    if grads:
        at = dict(logits=logits0, probs=probs0) if at is None else at
        # (a copy per sample row, so that the terms of the sum over the rows come out one by one)
        leaf = {k: x.detach().expand(u.shape).clone().requires_grad_(True) for k, x in at.items()}
        again = dict(z=f["rsample"](leaf["logits"], u, eps), zcond=f["csample"](leaf["probs"], b, v, eps),
                     log_prob=f["log_prob"](leaf["logits"], z_in), tlog_prob=f["tlog_prob"](leaf["logits"], b),
                     clog_prob=f["clog_prob"](leaf["logits"], zcond_in, b))
        for k in CONTINUOUS:
            (t,) = torch.autograd.grad(again[k], leaf[WRT[k]], upstream(again[k].shape))
            g["g_" + k] = exact_sum_to_size(t, at[WRT[k]].shape)
    return outs, g
