"""Estimators of expectations on MI355X (reference _estimators.py, _enumerate_estimator.py, _mc.py:27-738).

The reference's estimators are chains of small ATen operations on ``(M,) + batch_shape`` tensors (``M`` the
number of samples): a clamp, exp, max, mean, log or softmax along the sample axis, walked back by autograd.  Here
every estimator calls ``proposal`` and ``func`` exactly as the reference does and then ONE fused operator,
:func:`mc_reduce`: one launch of ``csrc/mc_reduce.hip`` forward, one backward, on float32 / float64 ROCm tensors.
CPU tensors and other dtypes take :func:`mc_reduce_torch`, the reference's formula line for line.  The accept /
reject loop of independent Metropolis-Hastings is one launch of ``csrc/imh_chain.hip`` per chunk of proposals.

Gradients.  The backward kernel is an operator of its own whose derivative is that of the torch body, so the
fused operators can be differentiated twice (``gradgradcheck``, ``create_graph=True``); the result of that
second differentiation is not differentiable again.  The variance-minimising block of :class:`RelaxEstimator`
needs second derivatives of everything in front of the reduction and stays composed of torch operations.

One value differs between the two paths.  Where the mean of a log-space SCORE falls below ``exp(EPS_NINF)`` (a
control variate above ``func``: a negative average), the reference's ``log(mean) + deriv - deriv.detach() + max``
loses ``log(floor)`` = -43.7 to a ``deriv`` of the order of 1e19 and returns ``max``; so does the torch body.  The
kernel's score term is exactly 0 and it returns ``log(floor) + max``.  The gradients agree.
"""
import abc
import math
from typing import Callable, Optional, Sequence, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck, config
from ._relaxed import ConditionalStraightThrough, Density, StraightThrough

__all__ = [
    "DirectEstimator",
    "EnumerateEstimator",
    "Estimator",
    "FunctionOnSample",
    "ImportanceSamplingEstimator",
    "IndependentMetropolisHastingsEstimator",
    "MonteCarloEstimator",
    "RelaxEstimator",
    "ReparameterizationEstimator",
    "StraightThroughEstimator",
]

FunctionOnSample = Callable[[torch.Tensor], torch.Tensor]

MEAN, SCORE, WEIGHTED = 0, 1, 2
W_LOGM, W_SELF, W_NONE = 0, 1, 2  # kappa of WEIGHTED: log M, the column's logsumexp, none (no lq)
FORM_COLUMNS, FORM_WAVE = 0, 1  # pdt_mc_reduce_plan
_DTYPES = {torch.float32: 0, torch.float64: 1}
_STATS = 5

# The proposals of one chunk of the IMH chain, and the chain gathered from them, stay under this many bytes each.
IMH_CHUNK_BYTES = 64 << 20


# ---- torch bodies: the reference's formulas, line for line ----------------------------------------------------------
def _shift_exp(x: torch.Tensor, lmax: torch.Tensor) -> torch.Tensor:
    return (x - lmax).clamp(config.EPS_NINF, config.EPS_INF).exp()


def mc_reduce_torch(kind: int, is_log: bool, mode: int, f, a=None, cz=None, c=None, lp=None, lq=None) -> torch.Tensor:
    """Reduce ``(M,) + batch_shape`` inputs over the sample axis to ``batch_shape`` in torch operations (the
    table of ``include/pdt_amd.h``, "Sample-axis reductions")."""
    if kind == MEAN:  # _mc.py:233, 301
        return f.logsumexp(0) - math.log(f.size(0)) if is_log else f.mean(0)
    if kind == WEIGHTED:  # _mc.py:394-404, _enumerate_estimator.py:72-77
        if mode == W_NONE:
            llr = lp
        else:
            lq = lq.detach() + 0 * lq.sum()
            llr = (lp - lq).log_softmax(0) if mode == W_SELF else lp - lq - math.log(f.size(0))
        return (f + llr).logsumexp(0) if is_log else (f * llr.exp()).sum(0)
    # SCORE: _mc.py:148-173 (no cz), 523-530 and 556-564 (cz)
    fb = f
    if is_log:
        fb_lmax = fb.max(0, keepdim=True)[0].clamp(torch.finfo(fb.dtype).min / 2, torch.finfo(fb.dtype).max / 2)
        fb = _shift_exp(fb, fb_lmax)
        if a is not None:
            a = _shift_exp(a, fb_lmax)
        if c is not None:
            c = _shift_exp(c.unsqueeze(0), fb_lmax)
        if cz is not None:
            cz = _shift_exp(cz, fb_lmax)
    if a is not None:
        fb = fb - a
    if c is not None:
        fb = fb + c
    if cz is None:
        deriv = (fb.detach() * lp).mean(0)
        fb = fb.mean(0)
    else:
        deriv = fb.detach() * lp
        fb = (fb + cz).mean(0)
    if is_log:
        fb = fb.clamp_min(math.exp(config.EPS_NINF))
        deriv = deriv / fb.detach()
        v = fb.log() + deriv - deriv.detach() + fb_lmax
        v = v.squeeze(0) if cz is None else v
    else:
        v = fb + deriv - deriv.detach()
    return v if cz is None else v.mean(0)


def imh_chain_torch(ratio: torch.Tensor, ratio0: torch.Tensor, log_u: torch.Tensor):
    """The scan of ``csrc/imh_chain.hip`` in torch operations, one step of the chain per iteration."""
    M = ratio.size(0)
    last = ratio0.clone()
    cur = torch.full(ratio0.shape, -1, dtype=torch.int32, device=ratio.device)
    idx = torch.empty(ratio.shape, dtype=torch.int32, device=ratio.device)
    for n in range(M):
        accept = (ratio[n] - last) > log_u[n]
        last = torch.where(accept, ratio[n], last)
        cur = torch.where(accept, torch.full_like(cur, n), cur)
        idx[n] = cur
    return idx, last, cur


# ---- the fused operators ------------------------------------------------------------------------------------------
def _columns(t: Optional[torch.Tensor], lead: int):
    """``t`` of shape ``lead dims + batch_shape`` as columns through element strides: (tensor to keep alive, s_m,
    s_b).  ``lead`` is 1 for the ``(M,) + batch_shape`` inputs and 0 for cv_mean, which every sample reads
    (s_m = 0).  A batch shape whose dimensions do not collapse onto one stride gets a dense copy."""
    if t is None:
        return None, 0, 0
    dims = [(n, s) for n, s in zip(t.shape[lead:], t.stride()[lead:]) if n != 1]
    if any(x[1] != y[0] * y[1] for x, y in zip(dims, dims[1:])):
        t = t.contiguous()
        return _columns(t, lead)
    return t, (t.stride(0) if lead and t.size(0) != 1 else 0), (dims[-1][1] if dims else 0)


def _pointers(tensors):
    return (_cabi._P * len(tensors))(*[_cabi.ptr(t) or None for t in tensors])


def _call_kernel(backward: bool, kind, is_log, mode, inputs, M, B, extra):
    keep, strides = [], []
    for i, t in enumerate(inputs):
        t, s_m, s_b = _columns(t, 0 if i == 3 else 1)
        keep.append(t)
        strides += [s_m, s_b]
    f = keep[0]
    lib = _cabi.lib()
    device = f.device
    with _cabi.on_device(device):
        head = (kind, int(is_log), mode, _DTYPES[f.dtype], M, B, _pointers(keep), (_cabi._I64 * 12)(*strides))
        if backward:
            g, stats, grads = extra
            rc = lib.pdt_mc_reduce_backward(*head, _cabi.ptr(g), _cabi.ptr(stats), _pointers(grads), _cabi.stream_ptr(device))
        else:
            out, stats = extra
            rc = lib.pdt_mc_reduce(*head, _cabi.ptr(out), _cabi.ptr(stats), _cabi.stream_ptr(device))
    _cabi.check(rc, "pdt_mc_reduce_backward" if backward else "pdt_mc_reduce")


@custom_op("pydrobert_amd::mc_reduce", mutates_args=())
def _mc_reduce_op(
    kind: int, is_log: bool, mode: int, f: torch.Tensor, a: Optional[torch.Tensor], cz: Optional[torch.Tensor],
    c: Optional[torch.Tensor], lp: Optional[torch.Tensor], lq: Optional[torch.Tensor],
) -> Tuple[torch.Tensor, torch.Tensor]:  # fmt: skip
    """(the reduction of shape ``batch_shape``, the (5, B) float64 column statistics its backward reads).  ``c`` has
    the shape ``batch_shape``, the other inputs ``(M,) + batch_shape``; float32 / float64 on one ROCm device."""
    inputs = [None if t is None else t.detach() for t in (f, a, cz, c, lp, lq)]
    device = _cabi.require_hip(*inputs)
    M, B = f.size(0), f[0].numel()
    out = torch.empty(f.shape[1:], dtype=f.dtype, device=device)
    stats = torch.empty((_STATS, B), dtype=torch.float64, device=device)
    if B:
        _call_kernel(False, kind, is_log, mode, inputs, M, B, (out, stats))
    return out, stats


@_mc_reduce_op.register_fake
def _(kind, is_log, mode, f, a, cz, c, lp, lq):
    return f.new_empty(f.shape[1:]), f.new_empty((_STATS, f[0].numel()), dtype=torch.float64)


@custom_op("pydrobert_amd::mc_reduce_backward", mutates_args=())
def _mc_reduce_backward_op(
    kind: int, is_log: bool, mode: int, want: int, g: torch.Tensor, stats: torch.Tensor, f: torch.Tensor,
    a: Optional[torch.Tensor], cz: Optional[torch.Tensor], c: Optional[torch.Tensor], lp: Optional[torch.Tensor],
    lq: Optional[torch.Tensor],
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:  # fmt: skip
    """The gradients of (f, a, cz, c, lp, lq) for the gradient ``g`` of the reduction: bit i of ``want`` asks for
    input i, the others come back empty."""
    inputs = [None if t is None else t.detach() for t in (f, a, cz, c, lp, lq)]
    device = _cabi.require_hip(g, stats, *inputs)
    M, B = f.size(0), f[0].numel()
    grads = [
        torch.empty(t.shape if (want >> i) & 1 else (0,), dtype=f.dtype, device=device) if t is not None
        else torch.empty((0,), dtype=f.dtype, device=device)
        for i, t in enumerate(inputs)
    ]  # fmt: skip
    if B:
        wanted = [x if x.numel() else None for x in grads]
        _call_kernel(True, kind, is_log, mode, inputs, M, B, (g.detach().contiguous(), stats, wanted))
    return tuple(grads)


@_mc_reduce_backward_op.register_fake
def _(kind, is_log, mode, want, g, stats, f, a, cz, c, lp, lq):
    return tuple(
        f.new_empty(t.shape if t is not None and (want >> i) & 1 else (0,)) for i, t in enumerate((f, a, cz, c, lp, lq))
    )


def _reduce_setup_context(ctx, inputs, output):
    ctx.kind, ctx.is_log, ctx.mode = inputs[:3]
    ctx.save_for_backward(output[1], *inputs[3:])
    ctx.mark_non_differentiable(output[1])


def _reduce_backward(ctx, g, _g_stats):
    stats, *inputs = ctx.saved_tensors
    want = sum(1 << i for i in range(6) if ctx.needs_input_grad[3 + i] and inputs[i] is not None)
    args = (ctx.kind, ctx.is_log, ctx.mode, want, g, stats) + tuple(inputs)
    if _cabi.plain_call(*args[4:]):  # (an ordinary backward: nothing to record, nothing for the dispatcher to do)
        grads = _mc_reduce_backward_op._init_fn(*args)
    else:
        grads = torch.ops.pydrobert_amd.mc_reduce_backward(*args)
    return (None, None, None) + tuple(d if (want >> i) & 1 else None for i, d in enumerate(grads))


register_autograd("pydrobert_amd::mc_reduce", _reduce_backward, setup_context=_reduce_setup_context)


def _backward_setup_context(ctx, inputs, output):
    ctx.kind, ctx.is_log, ctx.mode, ctx.want = inputs[:4]
    ctx.save_for_backward(inputs[4], *inputs[6:])


def _backward_backward(ctx, *gg):
    """The derivative of the backward operator: the torch body's, in differentiable torch operations."""
    g, *inputs = ctx.saved_tensors
    with torch.enable_grad():
        gd = g.detach().requires_grad_()
        xd = [None if x is None else x.detach().requires_grad_() for x in inputs]
        v = mc_reduce_torch(ctx.kind, ctx.is_log, ctx.mode, *xd)
        asked = [i for i in range(6) if (ctx.want >> i) & 1]
        first = torch.autograd.grad(v, [xd[i] for i in asked], gd, create_graph=True, allow_unused=True)
        outs, gouts = [], []
        for i, d in zip(asked, first):
            if d is not None and d.requires_grad and gg[i] is not None:
                outs.append(d)
                gouts.append(gg[i])
        targets = [gd] + [x for x in xd if x is not None]
        second = torch.autograd.grad(outs, targets, gouts, allow_unused=True) if outs else [None] * len(targets)
    second = list(second)
    g_g = second.pop(0)
    g_inputs = [None if x is None else second.pop(0) for x in xd]
    return (None, None, None, None, g_g, None) + tuple(g_inputs)


register_autograd("pydrobert_amd::mc_reduce_backward", _backward_backward, setup_context=_backward_setup_context)


def _on_kernel(*tensors) -> bool:
    f = tensors[0]
    if f.device.type != "cuda" or f.dtype not in _DTYPES or f.dim() < 1 or f.numel() == 0:
        return False
    return all(t is None or (t.dtype == f.dtype and t.device == f.device) for t in tensors)


def mc_reduce(kind: int, is_log: bool, f, a=None, cz=None, c=None, lp=None, lq=None, mode: int = W_LOGM) -> torch.Tensor:
    """Operation ``kind`` over the sample axis of ``(M,) + batch_shape`` inputs (``c``: broadcast to
    ``batch_shape``): the fused kernels on float32 / float64 ROCm tensors, :func:`mc_reduce_torch` otherwise."""
    batch = f.shape[1:]
    if c is not None and c.dim() == f.dim() and c.size(0) == 1:
        c = c.squeeze(0)
    if not _on_kernel(f, a, cz, c, lp, lq) or (c is not None and c.dim() > len(batch)):
        return mc_reduce_torch(kind, is_log, mode, f, a, cz, c, lp, lq)
    others = tuple(None if t is None else t.expand(f.shape) for t in (a, cz))
    c = None if c is None else c.expand(batch)
    lp, lq = (None if t is None else t.expand(f.shape) for t in (lp, lq))
    args = (kind, is_log, mode, f) + others + (c, lp, lq)
    if not torch.jit.is_tracing() and _cabi.plain_call(*args[3:]):
        return _mc_reduce_op._init_fn(*args)[0]
    return torch.ops.pydrobert_amd.mc_reduce(*args)[0]


@custom_op("pydrobert_amd::imh_chain", mutates_args=())
def _imh_chain_op(ratio: torch.Tensor, ratio0: torch.Tensor, log_u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``ratio`` and ``log_u`` (M, B), ``ratio0`` (B,) -> (idx (M, B) int32, the final ratio (B,), the final index
    (B,) int32); float32 / float64 on one ROCm device."""
    device = _cabi.require_hip(ratio, ratio0, log_u)
    M, B = ratio.shape
    idx = torch.empty((M, B), dtype=torch.int32, device=device)
    last = torch.empty((B,), dtype=ratio.dtype, device=device)
    last_idx = torch.empty((B,), dtype=torch.int32, device=device)
    if B:
        with _cabi.on_device(device):
            rc = _cabi.lib().pdt_imh_chain(
                _DTYPES[ratio.dtype], _cabi.ptr(ratio), ratio.stride(0), ratio.stride(1), _cabi.ptr(ratio0),
                ratio0.stride(0), _cabi.ptr(log_u), log_u.stride(0), log_u.stride(1), M, B, _cabi.ptr(idx),
                _cabi.ptr(last), _cabi.ptr(last_idx), _cabi.stream_ptr(device),
            )  # fmt: skip
        _cabi.check(rc, "pdt_imh_chain")
    return idx, last, last_idx


@_imh_chain_op.register_fake
def _(ratio, ratio0, log_u):
    M, B = ratio.shape
    return (
        ratio.new_empty((M, B), dtype=torch.int32),
        ratio.new_empty((B,)),
        ratio.new_empty((B,), dtype=torch.int32),
    )


def imh_chain(ratio: torch.Tensor, ratio0: torch.Tensor, log_u: torch.Tensor):
    """The accept / reject scan over ``ratio`` of shape ``(M,) + batch_shape`` from ``ratio0`` of shape
    ``batch_shape``: (idx, the final ratio, the final index), ``idx[n]`` the proposal the chain stands on after
    step n, -1 for the sample carried in.  One launch on float32 / float64 ROCm tensors."""
    dtype = torch.promote_types(ratio.dtype, log_u.dtype)
    ratio, ratio0, log_u = ratio.to(dtype), ratio0.to(dtype), log_u.to(dtype)
    if ratio.device.type != "cuda" or dtype not in _DTYPES or ratio.numel() == 0:
        return imh_chain_torch(ratio, ratio0, log_u)
    M, batch = ratio.size(0), ratio.shape[1:]
    flat = (ratio.reshape(M, -1), ratio0.reshape(-1), log_u.reshape(M, -1))
    if not torch.jit.is_tracing() and _cabi.plain_call(*flat):
        idx, last, last_idx = _imh_chain_op._init_fn(*flat)
    else:
        idx, last, last_idx = torch.ops.pydrobert_amd.imh_chain(*flat)
    return idx.reshape(ratio.shape), last.reshape(batch), last_idx.reshape(batch)


# ---- the estimators -----------------------------------------------------------------------------------------------
class Estimator(metaclass=abc.ABCMeta):
    r"""Computes an estimate :math:`v \approx \mathbb{E}_{b \sim P}[f(b)]` (reference _estimators.py:28-113).

    ``proposal`` is the distribution the samples are drawn from, ``func`` maps samples of shape ``(num_samples,) +
    proposal.batch_shape + proposal.event_shape`` to values of shape ``(num_samples,) + proposal.batch_shape``.
    With ``is_log``, ``func`` is :math:`\log f` and the result an estimate of :math:`\log v`.  Calling the
    instance returns the estimate, of shape ``proposal.batch_shape``."""

    def __init__(
        self,
        proposal: torch.distributions.distribution.Distribution,
        func: FunctionOnSample,
        is_log: bool = False,
    ):
        proposal = argcheck.is_a(proposal, torch.distributions.distribution.Distribution, "proposal")
        is_log = argcheck.is_bool(is_log, "is_log")
        super().__init__()
        self.proposal, self.func, self.is_log = proposal, func, is_log

    @abc.abstractmethod
    def __call__(self) -> torch.Tensor:
        raise NotImplementedError


class EnumerateEstimator(Estimator):
    r"""The expectation, exactly, by enumerating the support of ``proposal``: :math:`\sum_b P(b) f(b)` (reference
    _enumerate_estimator.py:20-77).  One WEIGHTED reduction over the support."""

    def __init__(
        self,
        proposal: torch.distributions.distribution.Distribution,
        func: FunctionOnSample,
        is_log: bool = False,
    ) -> None:
        if not proposal.has_enumerate_support:
            raise ValueError(
                "proposal must be able to enumerate its support " "(proposal.has_enumerate_support == True)"
            )
        super().__init__(proposal, func, is_log)

    def __call__(self) -> torch.Tensor:
        b = self.proposal.enumerate_support()
        log_pb = self.proposal.log_prob(b)
        fb = self.func(b)
        return mc_reduce(WEIGHTED, self.is_log, fb, lp=log_pb, mode=W_NONE)


class MonteCarloEstimator(Estimator, metaclass=abc.ABCMeta):
    """An estimator that draws ``mc_samples`` samples from ``proposal`` (reference _mc.py:27-79).  In log space
    the estimate of :math:`\\log v` is the log of the estimate of :math:`v`: biased, a lower bound."""

    def __init__(
        self,
        proposal: torch.distributions.Distribution,
        func: FunctionOnSample,
        mc_samples: int,
        is_log: bool = False,
    ) -> None:
        proposal = argcheck.is_a(proposal, torch.distributions.Distribution, "proposal")
        mc_samples = argcheck.is_posi(mc_samples, "mc_samples")
        is_log = argcheck.is_bool(is_log, "is_log")
        super().__init__(proposal, func, is_log)
        self.mc_samples = mc_samples


class DirectEstimator(MonteCarloEstimator):
    r"""The sample average of ``func`` over draws from ``proposal``, with the REINFORCE gradient and an optional
    control variate ``cv`` of mean ``cv_mean`` (reference _mc.py:82-173).  One SCORE reduction.  As in the
    reference, the result in log space has shape ``(1,) + batch_shape``."""

    def __init__(
        self,
        proposal: torch.distributions.Distribution,
        func: FunctionOnSample,
        mc_samples: int,
        cv: Optional[FunctionOnSample] = None,
        cv_mean: Optional[torch.Tensor] = None,
        is_log: bool = False,
    ):
        cv_mean = argcheck.is_tensor(cv_mean, "cv_mean", True)
        super().__init__(proposal, func, mc_samples, is_log)
        self.cv, self.cv_mean = cv, cv_mean

    def __call__(self) -> torch.Tensor:
        b = self.proposal.sample([self.mc_samples])
        fb = self.func(b)
        cvb = c = None
        if self.cv is not None:
            c = self.cv_mean
            if c is None:  # (where the reference fails: on None.unsqueeze in log space, on fb - cvb + None out of it)
                raise (AttributeError if self.is_log else TypeError)("cv_mean must be given together with cv")
            cvb = self.cv(b)
        log_pb = self.proposal.log_prob(b)
        v = mc_reduce(SCORE, self.is_log, fb, a=cvb, c=c, lp=log_pb)
        return v.unsqueeze(0) if self.is_log else v


class ReparameterizationEstimator(MonteCarloEstimator):
    """The sample average over ``proposal.rsample``, differentiated through the samples (reference
    _mc.py:176-233).  One MEAN reduction."""

    def __init__(
        self,
        proposal: torch.distributions.Distribution,
        func: FunctionOnSample,
        mc_samples: int,
        is_log: bool = False,
    ) -> None:
        if not proposal.has_rsample:
            raise ValueError("proposal must implement rsample")
        super().__init__(proposal, func, mc_samples, is_log)

    def __call__(self) -> torch.Tensor:
        z = self.proposal.rsample([self.mc_samples])
        fz = self.func(z)
        return mc_reduce(MEAN, self.is_log, fz)


class StraightThroughEstimator(MonteCarloEstimator):
    """The sample average over thresholded relaxed samples, whose gradient passes straight through the threshold
    (reference _mc.py:236-301).  ``proposal`` is a :class:`pydrobert_amd.distributions.StraightThrough`.  One
    MEAN reduction."""

    def __init__(
        self,
        proposal: StraightThrough,
        func: FunctionOnSample,
        mc_samples: int,
        is_log: bool = False,
    ) -> None:
        proposal = argcheck.is_a(proposal, StraightThrough, "proposal")
        super().__init__(proposal, func, mc_samples, is_log)

    def __call__(self) -> torch.Tensor:
        z = self.proposal.rsample([self.mc_samples])
        b = self.proposal.threshold(z, True)
        fb = self.func(b)
        return mc_reduce(MEAN, self.is_log, fb)


class ImportanceSamplingEstimator(MonteCarloEstimator):
    """Samples from ``proposal`` Q weighted by the likelihood ratio of ``density`` P over Q, optionally
    self-normalised (reference _mc.py:304-404).  The proposal's parameters get a zero gradient.  One WEIGHTED
    reduction."""

    def __init__(
        self,
        proposal: torch.distributions.Distribution,
        func: FunctionOnSample,
        mc_samples: int,
        density: Density,
        self_normalize: bool = False,
        is_log: bool = False,
    ) -> None:
        self_normalize = argcheck.is_bool(self_normalize, "self_normalize")
        super().__init__(proposal, func, mc_samples, is_log)
        self.density = density
        self.self_normalize = self_normalize

    def __call__(self) -> torch.Tensor:
        b = self.proposal.sample([self.mc_samples])
        lpb = self.density.log_prob(b)
        lqb = self.proposal.log_prob(b)
        fb = self.func(b)
        return mc_reduce(WEIGHTED, self.is_log, fb, lp=lpb, lq=lqb, mode=W_SELF if self.self_normalize else W_LOGM)


class RelaxEstimator(MonteCarloEstimator):
    """RELAX [grathwohl2017]: the sample average of ``func(b) - cv(zcond) + cv(z)`` over a
    :class:`pydrobert_amd.distributions.ConditionalStraightThrough` proposal (reference _mc.py:407-564).  With
    ``proposal_params`` and ``cv_params`` the control variate's parameters get the gradient that minimises the
    variance of the proposal parameters' gradient estimates; that block needs second derivatives and is composed
    of torch operations.  The estimate itself is one SCORE reduction."""

    def __init__(
        self,
        proposal: ConditionalStraightThrough,
        func: FunctionOnSample,
        mc_samples: int,
        cv: FunctionOnSample,
        proposal_params: Sequence[torch.Tensor] = tuple(),
        cv_params: Sequence[torch.Tensor] = tuple(),
        is_log: bool = False,
    ) -> None:
        proposal = argcheck.is_a(proposal, ConditionalStraightThrough, "proposal")
        proposal_params = tuple(proposal_params)
        cv_params = tuple(cv_params)
        if (len(proposal_params) > 0) != (len(cv_params) > 0):
            raise ValueError("either both proposal_params and cv_params must be specified or neither")
        super().__init__(proposal, func, mc_samples, is_log)
        self.cv, self.proposal_params, self.cv_params = cv, proposal_params, cv_params

    def __call__(self) -> torch.Tensor:
        z = self.proposal.rsample([self.mc_samples])
        b = self.proposal.threshold(z)
        zcond = self.proposal.csample(b)
        log_pb = self.proposal.tlog_prob(b)
        fb = self.func(b)
        cvz = self.cv(z)
        cvzcond = self.cv(zcond)
        if self.cv_params:
            fb_, cvz_, cvzcond_ = fb, cvz, cvzcond
            if self.is_log:
                fb_lmax = fb.max(0, keepdim=True)[0].clamp(torch.finfo(fb.dtype).min / 2, torch.finfo(fb.dtype).max / 2)
                fb_, cvz_, cvzcond_ = (_shift_exp(x, fb_lmax) for x in (fb, cvz, cvzcond))
            v_ = ((fb_ - cvzcond_) * log_pb + cvz_).mean(0)
            if self.is_log:
                v_ = v_.log() + fb_lmax
            gs_proposal = torch.autograd.grad(
                v_, self.proposal_params, torch.ones_like(v_), create_graph=True, retain_graph=True
            )
            gs_cv = [0.0] * len(self.cv_params)
            for gp in gs_proposal:
                gp = gp.norm(2)
                gs_cv = [x + y for (x, y) in zip(gs_cv, torch.autograd.grad(gp, self.cv_params, retain_graph=True))]
            for gc, c in zip(gs_cv, self.cv_params):
                _attach_grad(c, gc.detach())
        return mc_reduce(SCORE, self.is_log, fb, a=cvzcond, cz=cvz, lp=log_pb)


def _event_index(index: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """``index`` over ``(n,) + batch_shape`` as a gather index into ``like``'s ``(*,) + batch_shape + event_shape``."""
    extra = like.dim() - index.dim()
    return index.reshape(index.shape + (1,) * extra).expand(index.shape + like.shape[index.dim():])


class IndependentMetropolisHastingsEstimator(MonteCarloEstimator):
    """Independent Metropolis-Hastings: a chain over proposals from ``proposal`` Q accepted by the ratio of
    ``density`` P over Q, averaged after ``burn_in`` steps (reference _mc.py:567-738).  No gradient.

    The random draws come in the reference's order (the initial sample, the uniforms, the proposals), but the
    proposals are drawn, scored and evaluated a chunk at a time (:data:`IMH_CHUNK_BYTES`): the accept / reject
    loop is one scan, ``func`` is called once per chunk on the gathered chain.  Two departures from the
    reference: a rejected proposal outside the support of ``density`` (ratio ``-inf``) leaves the chain's ratio
    as it was (the reference's blend turns it into NaN, after which nothing is accepted), and ``initial_sample``
    is validated against ``proposal`` (the reference reads an attribute it has not set yet and raises)."""

    def __init__(
        self,
        proposal: torch.distributions.Distribution,
        func: FunctionOnSample,
        mc_samples: int,
        density: Density,
        burn_in: int = 0,
        initial_sample: Optional[torch.Tensor] = None,
        initial_sample_tries: int = 1000,
        is_log: bool = False,
    ) -> None:
        burn_in = argcheck.is_nonnegi(burn_in, "burn_in")
        mc_samples = argcheck.is_posi(mc_samples, "mc_samples")
        argcheck.is_lt(burn_in, mc_samples, "burn_in", "mc_samples")
        if initial_sample is not None:
            proposal = argcheck.is_a(proposal, torch.distributions.Distribution, "proposal")
            sample_shape = proposal.batch_shape + proposal.event_shape
            if initial_sample.shape == sample_shape:
                initial_sample = initial_sample.unsqueeze(0)
            elif initial_sample.shape != (1,) + sample_shape:
                raise ValueError(
                    f"Expected initial_sample to have shape {(1,) + sample_shape} or " f"{sample_shape} "
                )
            if not torch.isfinite(density.log_prob(initial_sample)).all():
                raise ValueError("all values in initial_sample must lie in the support of density")
        elif initial_sample_tries < 1:
            raise ValueError("initial_sample_tries must be positive when initial_sample is None")
        super().__init__(proposal, func, mc_samples, is_log)
        self.density, self.initial_sample = density, initial_sample
        self.initial_sample_tries, self.burn_in = initial_sample_tries, burn_in

    def find_initial_sample(self, tries: Optional[int] = None) -> torch.Tensor:
        """Find an initial sample by randomly sampling from the proposal"""
        if tries is None:
            tries = self.initial_sample_tries
        if tries < 1:
            raise ValueError("tries must be positive")
        with torch.no_grad():
            sample = self.proposal.sample([1])
            keep = torch.isfinite(self.density.log_prob(sample))
            if keep.all():
                return sample
            for _ in range(tries - 1):
                cur_sample = self.proposal.sample([1])
                while keep.dim() < cur_sample.dim():
                    keep = keep.unsqueeze(-1)  # event dims
                sample = torch.where(keep, sample, cur_sample)
                keep = torch.isfinite(self.density.log_prob(sample))
                if keep.all():
                    return sample
            raise RuntimeError(
                f"Unable to find initial sample in {tries} draws. "
                f"Either specify initial_sample on instantiation or increase "
                f"initial_sample_tries."
            )

    def __call__(self) -> torch.Tensor:
        with torch.no_grad():
            if self.initial_sample is None:
                last_sample = self.find_initial_sample()
            else:
                last_sample = self.initial_sample
            M, num_kept = self.mc_samples, self.mc_samples - self.burn_in
            last_ratio = self.density.log_prob(last_sample) - self.proposal.log_prob(last_sample)
            uniform_draws = torch.rand((M,) + self.proposal.batch_shape, device=last_sample.device).log()
            steps = max(1, IMH_CHUNK_BYTES // max(1, last_sample.numel() * last_sample.element_size()))
            v, n0 = None, 0
            while n0 < M:
                m = min(steps, M - n0)
                cur_sample = self.proposal.sample([m])
                cur_ratio = self.density.log_prob(cur_sample) - self.proposal.log_prob(cur_sample)
                idx, ratio, last_idx = imh_chain(cur_ratio, last_ratio[0], uniform_draws[n0 : n0 + m])
                pool = torch.cat([last_sample, cur_sample], 0)  # (row 0: the sample carried in, idx -1)
                first = max(self.burn_in - n0, 0)
                if first < m:
                    chain = pool.gather(0, _event_index(idx[first:].long() + 1, pool))
                    part = mc_reduce(MEAN, self.is_log, self.func(chain))
                    if m - first != num_kept:  # one of several chunks: back to the sum, for the mean over all
                        scale = (m - first) / num_kept
                        part = part + math.log(scale) if self.is_log else part * scale
                    if v is None:
                        v = part
                    else:
                        v = torch.logaddexp(v, part) if self.is_log else v + part
                last_sample = pool.gather(0, _event_index(last_idx.long().unsqueeze(0) + 1, pool))
                last_ratio = ratio.unsqueeze(0)
                n0 += m
            return v


def _attach_grad(x: torch.Tensor, g: torch.Tensor):
    def hook(grad):
        hook.__handle.remove()
        hook.__handle = None  # dies if this hook is called again
        return hook.__grad

    hook.__grad = g
    hook.__handle = x.register_hook(hook)
