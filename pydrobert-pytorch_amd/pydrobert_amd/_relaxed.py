"""Relaxed sampling on MI355X (reference _straight_through.py, _mc.py:751-840): the Gumbel / one-hot categorical
and logistic / Bernoulli relaxations behind REBAR and RELAX, and the REBAR control variates.

Every method of the two distributions is ONE launch of ``csrc/relaxed.hip`` on float32 / float64 ROCm tensors
(the reference chains six to fifteen elementwise passes and up to two row reductions).  The uniform noise is
drawn here with ``torch.rand`` / ``torch.rand_like`` and handed to the kernels as data, so ``torch.manual_seed``
governs every draw, and on the CPU a seed reproduces the reference's stream.  Other dtypes, CPU tensors, and a
discrete sample ``b`` that itself wants a gradient take torch bodies that restate the reference's formulas.

Gradients.  The backward of every method is an operator of its own, ``pydrobert_amd::relaxed_backward``: one
launch of the backward kernels of ``csrc/relaxed.hip`` (the Jacobians are diagonal) that writes the gradient of
the relaxed sample, where the method has one, and the gradient of the parameter ALREADY summed over the sample
rows, in float64 and in one fixed order; a second small launch adds partial sums where few parameter rows have
many samples.  What is left to the host is a ``sum_to_size`` only where the parameter's shape still differs (a
size-1 dimension inside it, a stride-0 row, a scalar).  The operator's derivative is that of the torch bodies
``_gumbel_backward`` / ``_bernoulli_backward`` -- which CPU tensors and other dtypes also take inside it -- so a
method can be differentiated twice (``gradgradcheck``, ``create_graph=True``): in the incoming gradient, which
RELAX needs, and in the parameters and relaxed samples; the result of that second differentiation is not
differentiable again.  ``rsample`` alone stays with torch on the host side: its Jacobian is the identity, and
``sum_to_size`` of the incoming gradient is one launch from C++.  ``threshold`` is computed without gradient, as in
the reference.  An input with no derivative here (the noise) raises rather than receive a silent zero.
"""
import abc
import functools
import math
import warnings
from typing import Optional, Sequence, Tuple

import torch
from torch.distributions import constraints
from torch.distributions.utils import clamp_probs, lazy_property, logits_to_probs, probs_to_logits
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck

__all__ = [
    "ConditionalStraightThrough",
    "Density",
    "GumbelOneHotCategorical",
    "GumbelOneHotCategoricalRebarControlVariate",
    "LogisticBernoulli",
    "LogisticBernoulliRebarControlVariate",
    "StraightThrough",
]

GUMBEL, BERNOULLI = 0, 1
RSAMPLE, THRESHOLD, TLOG_PROB, CSAMPLE, LOG_PROB, CLOG_PROB = range(6)
_REDUCES = (TLOG_PROB, LOG_PROB, CLOG_PROB)  # Gumbel methods whose result drops the event dimension
_DTYPES = {torch.float32: 0, torch.float64: 1}
_EULER = 0.57721566490153286060


def _eps(t: torch.Tensor) -> float:
    return torch.finfo(t.dtype).eps


def _one_hot_argmax(z: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.one_hot(z.argmax(-1), z.size(-1)).to(z)


# ---- torch bodies: the reference's formulas, broadcasting as it does ----------------------------------------------
def _gumbel_torch(op: int, param, x1, x2):
    if op == RSAMPLE:
        return param - (-clamp_probs(x1).log()).log()
    if op == THRESHOLD:
        return _one_hot_argmax(x1)
    if op == TLOG_PROB:
        hot = x1 != 0
        return torch.where(hot, param.expand_as(x1), param.new_zeros(())).sum(-1)
    if op == CSAMPLE:
        b, log_v = x1, clamp_probs(x2).log()
        hot = -(-log_v).log() * b
        z_k = hot.sum(-1, keepdim=True)
        rest = -(-log_v / clamp_probs(param) - (log_v * b).sum(-1, keepdim=True)).log()
        return hot + torch.min(z_k - _eps(b), rest) * (1 - b)
    if op == LOG_PROB:
        g = param - x1
        return (g - g.exp()).sum(-1)
    zcond, b = x1, x2
    miss = (_one_hot_argmax(zcond) != b).any(-1)
    rest = 1 - b
    logits = param * rest
    g = logits - zcond
    z_k = (zcond * b).sum(-1, keepdim=True)
    lp = (g - g.exp() + (logits - z_k).exp() * rest).sum(-1)
    return lp.masked_fill(miss, -math.inf)


def _bernoulli_torch(op: int, param, x1, x2):
    if op == RSAMPLE:
        u = clamp_probs(x1)
        return param + u.log() - (-u).log1p()
    if op == THRESHOLD:
        return (x1 >= 0.0).to(x1)
    if op == TLOG_PROB:
        logits, b = torch.broadcast_tensors(param, x1)
        return -torch.nn.functional.binary_cross_entropy_with_logits(logits, b, reduction="none")
    if op == CSAMPLE:
        b, v, p = x1, clamp_probs(x2), clamp_probs(param)
        t = v / ((1 - v) * ((1 - b) * p + b * (1 - p))) + 1
        return (2 * b - 1) * t.log() + b * _eps(b)
    if op == LOG_PROB:
        d = param - x1
        return d - 2 * d.exp().log1p()
    zcond, b = x1, x2
    miss = (zcond >= 0.0).to(zcond) != b
    lp = -zcond + (1 - b) * param + param.exp().log1p() - 2 * (param - zcond).exp().log1p()
    return lp.masked_fill(miss, -math.inf)


_TORCH = (_gumbel_torch, _bernoulli_torch)


def _param_rows(param: torch.Tensor):
    """``param``, already expanded to the trailing dimensions of the data, as (B, V) rows through element strides
    ``(B, p_sr, p_sv)``, and the tensor to keep alive.  No copy when its leading dimensions collapse onto one
    stride: broadcast ones (stride 0) IN FRONT are dropped, since sample row r reads parameter row r mod B.  A
    broadcast dimension between others does not fit that rule: a dense copy then."""
    if param.dim() == 0:
        return param, 1, 0, 0
    dims = [(n, s) for n, s in zip(param.shape[:-1], param.stride()[:-1]) if n != 1]
    while dims and dims[0][1] == 0:
        dims.pop(0)
    if any(a[1] != b[0] * b[1] for a, b in zip(dims, dims[1:])):
        param = param.contiguous()
        return (param,) + _param_rows(param)[1:]
    B = 1
    for n, _ in dims:
        B *= n
    return param, B, (dims[-1][1] if dims else 0), param.stride(-1)


def _on_kernel(param, x1, x2) -> bool:
    dt = x1.dtype
    if x1.device.type != "cuda" or dt not in _DTYPES:
        return False
    return all(t is None or (t.dtype == dt and t.device == x1.device) for t in (param, x2))


@custom_op("pydrobert_amd::relaxed", mutates_args=())
def _relaxed_op(
    family: int, op: int, param: Optional[torch.Tensor], x1: torch.Tensor, x2: Optional[torch.Tensor]
) -> torch.Tensor:
    """Method ``op`` of relaxation ``family`` (the table of ``include/pdt_amd.h``, "Relaxed sampling").  The data
    arguments have the shape ``sample_shape + param.shape``, already broadcast."""
    param = None if param is None else param.detach()
    x1, x2 = x1.detach(), None if x2 is None else x2.detach()
    if not _on_kernel(param, x1, x2):
        out = _TORCH[family](op, param, x1, x2)
        return torch.empty(out.shape, dtype=out.dtype, device=out.device).copy_(out)
    device = _cabi.require_hip(param, x1, x2)
    x1 = x1.contiguous()
    x2 = None if x2 is None else x2.contiguous()
    if param is not None and param.dim():
        # a data argument may broadcast over a size-1 dimension of the parameter: the kernel's rows are those of
        # the data, so the parameter takes the data's trailing shape as a stride-0 view
        param = param.expand(x1.shape[x1.dim() - param.dim():])
    rows_of = x1 if param is None else param  # (a row is the parameter's last dimension: a scalar's rows hold 1)
    V = rows_of.shape[-1] if rows_of.dim() else 1
    reduces = family == GUMBEL and op in _REDUCES
    out = torch.empty(x1.shape[:-1] if reduces else x1.shape, dtype=x1.dtype, device=device)
    if x1.numel() == 0:
        return out
    keep, B, p_sr, p_sv = (None, 1, 0, 1) if param is None else _param_rows(param)
    lib = _cabi.lib()
    fn = lib.pdt_relaxed_gumbel if family == GUMBEL else lib.pdt_relaxed_bernoulli
    with _cabi.on_device(device):
        rc = fn(
            op, _DTYPES[x1.dtype], _cabi.ptr(keep), B, p_sr, p_sv, _cabi.ptr(x1), _cabi.ptr(x2), x1.numel() // V, V,
            _cabi.ptr(out), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_relaxed_gumbel" if family == GUMBEL else "pdt_relaxed_bernoulli")
    return out


@_relaxed_op.register_fake
def _(family, op, param, x1, x2):
    reduces = family == GUMBEL and op in _REDUCES
    return x1.new_empty(x1.shape[:-1] if reduces else x1.shape)


def _relaxed_setup_context(ctx, inputs, output):
    ctx.family, ctx.op, param, x1, x2 = inputs
    ctx.save_for_backward(param, x1, x2)


def _gumbel_backward(op: int, g, param, x1, x2):
    """(grad param, grad x1, grad x2) in differentiable torch ops; ``False`` marks an input without one."""
    if op == RSAMPLE:
        return g, False, None
    if op == TLOG_PROB:
        return g.unsqueeze(-1) * (x1 != 0).to(g), False, None
    if op == LOG_PROB:
        t = g.unsqueeze(-1) * (1 - (param - x1).exp())
        return t, -t, None
    eps = _eps(x1)
    if op == CSAMPLE:
        # z_j = -log w_j off the hot index, w_j = -log v_j / p_j - log v_k: dz_j/dp_j = -log v_j / (p_j^2 w_j),
        # zero on the hot index, where the min guard holds z_j at z_k - eps, and where p_j is clamped
        b, log_v = x1, clamp_probs(x2).log()
        p = clamp_probs(param)
        log_vk = (log_v * b).sum(-1, keepdim=True)
        w = -log_v / p - log_vk
        z_k = (-(-log_v).log() * b).sum(-1, keepdim=True)  # (as the forward: 0 for a row without a hot element)
        free = ((-w.log()) <= (z_k - eps)) & (param >= eps) & (param <= 1 - eps)
        return g * (-log_v / (p * p * w)) * (1 - b) * free.to(g), False, False
    zcond, b = x1, x2  # CLOG_PROB: rows whose b is not the threshold of zcond are -inf, constant
    rest = 1 - b
    logits = param * rest
    z_k = (zcond * b).sum(-1, keepdim=True)
    a = 1 - (logits - zcond).exp()
    e = (logits - z_k).exp() * rest
    hit = ~(_one_hot_argmax(zcond) != b).any(-1, keepdim=True)
    g = torch.where(hit, g.unsqueeze(-1), g.new_zeros(()))
    return g * rest * (a + e), g * (-a - b * e.sum(-1, keepdim=True)), False


def _bernoulli_backward(op: int, g, param, x1, x2):
    if op == RSAMPLE:
        return g, False, None
    if op == TLOG_PROB:
        return g * (x1 - param.sigmoid()), False, None
    if op == LOG_PROB:
        t = g * (1 - 2 * (param - x1).sigmoid())
        return t, -t, None
    if op == CSAMPLE:
        eps = _eps(x1)
        b, v, p = x1, clamp_probs(x2), clamp_probs(param)
        q = (1 - b) * p + b * (1 - p)
        t = v / ((1 - v) * q) + 1
        free = (param >= eps) & (param <= 1 - eps)
        return g * (2 * b - 1) ** 2 * v / ((1 - v) * q * q * t) * free.to(g), False, False
    zcond, b = x1, x2
    s = (param - zcond).sigmoid()
    g = torch.where((zcond >= 0.0).to(zcond) == b, g, g.new_zeros(()))
    return g * ((1 - b) + param.sigmoid() - 2 * s), g * (2 * s - 1), False


_BACKWARD = (_gumbel_backward, _bernoulli_backward)
_HAS_X1_GRAD = (LOG_PROB, CLOG_PROB)  # z of log_prob, zcond of clog_prob


def _grad_rows(param: torch.Tensor, expanded: torch.Tensor):
    """:func:`_param_rows` for the backward: ``expanded`` is ``param`` over the trailing dimensions of the data.
    Returns (tensor to keep alive, B, p_sr, p_sv, shape) where ``shape`` is what the kernel's (B, V) rows are
    viewed as, broadcastable to ``param.shape``.  Only a leading dimension the parameter itself has with size 1
    is left to the sum over the sample rows: one it has with stride 0 (an expanded view handed in as the
    parameter) gets a gradient per position, read through that stride."""
    if expanded.dim() == 0:
        return expanded, 1, 0, 0, ()
    lead = range(expanded.dim() - 1)
    kept = [i for i in lead if expanded.size(i) != 1]
    while kept and param.size(kept[0]) == 1:
        kept.pop(0)
    dims = [(expanded.size(i), expanded.stride(i)) for i in kept]
    if any(a[1] != b[0] * b[1] for a, b in zip(dims, dims[1:])):
        expanded = expanded.contiguous()
        dims = [(expanded.size(i), expanded.stride(i)) for i in kept]
    B = 1
    for n, _ in dims:
        B *= n
    shape = tuple(expanded.size(i) if i in kept else 1 for i in lead) + (expanded.size(-1),)
    return expanded, B, (dims[-1][1] if dims else 0), expanded.stride(-1), shape


def _fresh(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return torch.empty(t.shape, dtype=dtype, device=t.device).copy_(t)


@functools.lru_cache(maxsize=256)
def _workspace_words(code: int, R: int, B: int, V: int) -> int:
    """float64 words of the parts form's workspace (0: the base form); a pure function of the sizes."""
    return _cabi.lib().pdt_relaxed_backward_workspace_bytes(code, R, B, V) // 8


def _backward_body(family: int, op: int, want: int, g, param, x1, x2):
    """What ``pydrobert_amd::relaxed_backward`` computes, on tensors that carry no gradient: (the gradient of
    ``param`` in its own shape, that of ``x1``), ``None`` where ``want`` does not ask.  This is the host's share of
    every backward (the call is bound by it, not by the kernels), so the common case -- a dense parameter of the
    data's trailing shape -- takes no view, no row arithmetic and no placeholder."""
    dtype = x1.dtype
    if not _on_kernel(param, x1, x2) or g.dtype != dtype or g.device != x1.device:
        d_param, d_x1, _ = _BACKWARD[family](op, g, param, x1, x2)
        return (
            _fresh(d_param.sum_to_size(param.shape), d_param.dtype) if want & 1 else None,
            _fresh(d_x1, d_x1.dtype) if want & 2 else None,
        )
    device = x1.device
    if x1.numel() == 0:
        return (
            torch.zeros(param.shape, dtype=dtype, device=device) if want & 1 else None,
            torch.empty(x1.shape, dtype=dtype, device=device) if want & 2 else None,
        )
    g, x1 = g.contiguous(), x1.contiguous()
    x2 = None if x2 is None else x2.contiguous()
    nd = param.dim()
    if nd and param.shape == x1.shape[x1.dim() - nd:] and param.is_contiguous():
        V = param.shape[-1]
        keep, B, p_sr, p_sv, shape = param, param.numel() // V, V, 1, None
    else:
        expanded = param.expand(x1.shape[x1.dim() - nd:]) if nd else param
        V = expanded.shape[-1] if nd else 1
        keep, B, p_sr, p_sv, shape = _grad_rows(param, expanded)
    rows = torch.empty(param.shape if shape is None else (B, V), dtype=dtype, device=device) if want & 1 else None
    d_x1 = torch.empty(x1.shape, dtype=dtype, device=device) if want & 2 else None
    R = x1.numel() // V
    code = _DTYPES[dtype]
    words = _workspace_words(code, R, B, V)
    ws = torch.empty((words,), dtype=torch.float64, device=device) if words else None
    lib = _cabi.lib()
    fn = lib.pdt_relaxed_gumbel_backward if family == GUMBEL else lib.pdt_relaxed_bernoulli_backward
    with _cabi.on_device(device):
        rc = fn(
            op, code, g.data_ptr(), keep.data_ptr(), B, p_sr, p_sv, x1.data_ptr(), _cabi.ptr(x2), R, V,
            _cabi.ptr(rows), _cabi.ptr(d_x1), _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
    if rc:
        _cabi.check(rc, "pdt_relaxed_gumbel_backward" if family == GUMBEL else "pdt_relaxed_bernoulli_backward")
    if rows is not None and shape is not None:
        # (a size-1 dimension inside the parameter, a stride-0 row, the dense copy of a broadcast dimension between
        # others, a scalar: what is left to add up after the kernel's sum over the sample rows)
        rows = rows.view(shape)
        rows = rows if rows.shape == param.shape else rows.sum_to_size(param.shape)
    return rows, d_x1


@custom_op("pydrobert_amd::relaxed_backward", mutates_args=())
def _relaxed_backward_op(
    family: int, op: int, want: int, g: torch.Tensor, param: torch.Tensor, x1: torch.Tensor, x2: Optional[torch.Tensor]
) -> Tuple[torch.Tensor, torch.Tensor]:  # fmt: skip
    """The gradients of method ``op`` of relaxation ``family`` for the gradient ``g`` of its result: (that of
    ``param``, in ``param``'s own shape, summed over the sample rows; that of ``x1``).  Bit 0 of ``want`` asks for
    the first and bit 1 for the second; one not asked for comes back empty.  One launch of ``csrc/relaxed.hip``
    (two where the sample rows are cut into parts) on float32 / float64 ROCm tensors, the torch bodies otherwise."""
    if op == THRESHOLD or not want & 3 or (want & 2 and op not in _HAS_X1_GRAD):
        raise RuntimeError("pydrobert_amd::relaxed_backward: method {} has no such derivative".format(op))
    d_param, d_x1 = _backward_body(
        family, op, want, g.detach(), param.detach(), x1.detach(), None if x2 is None else x2.detach()
    )
    like = d_x1 if d_param is None else d_param
    return (
        torch.empty((0,), dtype=like.dtype, device=like.device) if d_param is None else d_param,
        torch.empty((0,), dtype=like.dtype, device=like.device) if d_x1 is None else d_x1,
    )


@_relaxed_backward_op.register_fake
def _(family, op, want, g, param, x1, x2):
    dtype = g.dtype
    for t in (param, x1, x2):
        dtype = dtype if t is None else torch.promote_types(dtype, t.dtype)
    return (
        param.new_empty(param.shape if want & 1 else (0,), dtype=dtype),
        x1.new_empty(x1.shape if want & 2 else (0,), dtype=dtype),
    )


def _relaxed_backward(ctx, g):
    param, x1, x2 = ctx.saved_tensors
    if ctx.op == THRESHOLD:
        return None, None, None, None, None
    has = (True, ctx.op in _HAS_X1_GRAD, False)
    for i in range(3):
        if ctx.needs_input_grad[2 + i] and not has[i]:
            raise NotImplementedError(
                "pydrobert_amd::relaxed: method {} has no derivative with respect to its {} argument".format(
                    ctx.op, ("parameter", "first data", "second data")[i]
                )
            )
    want = int(ctx.needs_input_grad[2]) | int(ctx.needs_input_grad[3]) << 1
    if not want:
        return None, None, None, None, None
    if ctx.op == RSAMPLE:
        # the Jacobian is the identity: nothing to compute, and torch's own reduction onto the parameter is one
        # launch from C++ (5 us a call against the 12 us and more of any launch through this layer: DESIGN.md 4.11)
        return None, None, g.sum_to_size(param.shape), None, None
    if _cabi.plain_call(g, param, x1, x2):  # (an ordinary backward: nothing to record, nothing for the dispatcher)
        d_param, d_x1 = _backward_body(ctx.family, ctx.op, want, g, param, x1, x2)
    else:
        d_param, d_x1 = torch.ops.pydrobert_amd.relaxed_backward(ctx.family, ctx.op, want, g, param, x1, x2)
    return None, None, d_param if want & 1 else None, d_x1 if want & 2 else None, None


register_autograd("pydrobert_amd::relaxed", _relaxed_backward, setup_context=_relaxed_setup_context)


def _backward_setup_context(ctx, inputs, output):
    ctx.family, ctx.op, ctx.want = inputs[:3]
    ctx.save_for_backward(*inputs[3:])


def _backward_backward(ctx, gg_param, gg_x1):
    """The derivative of the backward operator: the torch body's, in differentiable torch operations."""
    g, param, x1, x2 = ctx.saved_tensors
    with torch.enable_grad():
        leaves = [t.detach().requires_grad_() for t in (g, param, x1)]
        d_param, d_x1, _ = _BACKWARD[ctx.family](ctx.op, *leaves, x2)
        outs, gouts = [], []
        if ctx.want & 1 and gg_param is not None:
            outs.append(d_param.sum_to_size(param.shape))
            gouts.append(gg_param)
        if ctx.want & 2 and gg_x1 is not None:
            outs.append(d_x1)
            gouts.append(gg_x1)
        targets = [t for i, t in enumerate(leaves) if ctx.needs_input_grad[3 + i]]
        live = [(d, gd) for d, gd in zip(outs, gouts) if d.requires_grad]
        second = iter(
            torch.autograd.grad([d for d, _ in live], targets, [gd for _, gd in live], allow_unused=True)
            if live and targets else [None] * len(targets)
        )  # fmt: skip
    return (None, None, None) + tuple(next(second) if ctx.needs_input_grad[3 + i] else None for i in range(3)) + (None,)


register_autograd("pydrobert_amd::relaxed_backward", _backward_backward, setup_context=_backward_setup_context)


def _relaxed(family: int, op: int, param, x1, x2=None) -> torch.Tensor:
    if not torch.jit.is_tracing() and _cabi.plain_call(param, x1, x2):
        return _relaxed_op._init_fn(family, op, param, x1, x2)
    return torch.ops.pydrobert_amd.relaxed(family, op, param, x1, x2)


def _wants_grad(t: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and t.requires_grad


def _check_methods(C, *methods):
    # (collections.abc's rule: every method defined, and not set to None, somewhere along the MRO)
    for method in methods:
        for B in C.__mro__:
            if method in B.__dict__:
                if B.__dict__[method] is None:
                    return NotImplemented
                break
        else:
            return NotImplemented
    return True


class StraightThrough(torch.distributions.distribution.Distribution, metaclass=abc.ABCMeta):
    """Interface of distributions that allow a straight-through estimate (reference _straight_through.py:46-153):
    a relaxed draw :func:`rsample`, its discretisation :func:`threshold`, and the log probability of the
    discrete value :func:`tlog_prob`.  Any ``Distribution`` subclass with ``has_rsample`` and those three
    methods counts as a subclass."""

    has_rsample = True

    @abc.abstractmethod
    def rsample(self, sample_shape: Sequence = torch.Size()) -> torch.Tensor:
        ...

    @abc.abstractmethod
    def threshold(self, z: torch.Tensor, straight_through: bool = False) -> torch.Tensor:
        """The discrete sample ``b`` of the relaxed sample ``z``; with ``straight_through`` the gradient of ``z``
        is attached to it."""
        ...

    @abc.abstractmethod
    def tlog_prob(self, b: torch.Tensor) -> torch.Tensor:
        """The log probability of the discrete sample ``b``, of shape ``sample_shape + batch_shape``."""
        ...

    def _validate_thresholded_sample(self, value: torch.Tensor):
        """``Distribution._validate_sample`` for an argument that is a discrete sample."""
        if not isinstance(value, torch.Tensor):
            raise ValueError("The b argument must be a Tensor")
        event_dim_start = len(value.size()) - len(self.event_shape)
        if value.size()[event_dim_start:] != self.event_shape:
            raise ValueError(
                "The right-most size of b must match event_shape:{} vs {}.".format(value.size(), self.event_shape)
            )
        actual_shape = value.size()
        expected_shape = self.batch_shape + self.event_shape
        for i, j in zip(reversed(actual_shape), reversed(expected_shape)):
            if i != 1 and j != 1 and i != j:
                raise ValueError(
                    "Value is not broadcastable with batch_shape+event_shape: {} vs {}.".format(
                        actual_shape, expected_shape
                    )
                )
        try:
            support = self.thresholded_support
        except NotImplementedError:
            warnings.warn(
                "{} does not define `thresholded_support` to enable sample validation. Please initialize the "
                "distribution with `validate_args=False` to turn off validation.".format(self.__class__)
            )
            return
        assert support is not None
        if not support.check(value).all():
            raise ValueError(
                "Expected b argument ({} of shape {}) to be within the support ({}) of the distribution {}, but "
                "found invalid values:\n{}".format(type(value).__name__, tuple(value.shape), repr(support), repr(self), value)
            )

    @classmethod
    def __subclasshook__(cls, C) -> bool:
        if cls is StraightThrough:
            if not issubclass(C, torch.distributions.distribution.Distribution) or not C.has_rsample:
                return NotImplemented
            return _check_methods(C, "rsample", "threshold", "tlog_prob")
        return NotImplemented


class ConditionalStraightThrough(StraightThrough, metaclass=abc.ABCMeta):
    """A :class:`StraightThrough` that can also draw a relaxed sample given its discrete image, :func:`csample`,
    and score it, :func:`clog_prob` (reference _straight_through.py:156-223)."""

    @abc.abstractmethod
    def csample(self, b: torch.Tensor) -> torch.Tensor:
        """A relaxed sample ``zcond`` with ``threshold(zcond) == b``."""
        ...

    @abc.abstractmethod
    def clog_prob(self, zcond: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """``log P(zcond | b)``, of shape ``sample_shape + batch_shape``: the density of ``zcond`` over ``P(b)``
        where ``threshold(zcond) == b``, ``-inf`` elsewhere."""
        ...

    @classmethod
    def __subclasshook__(cls, C) -> bool:
        if cls is ConditionalStraightThrough:
            if StraightThrough.__subclasshook__(C) is NotImplemented:
                return NotImplemented
            return _check_methods(C, "csample", "clog_prob")
        return NotImplemented


class Density(metaclass=abc.ABCMeta):
    """Interface of a density: anything with a :func:`log_prob` (reference _straight_through.py:226-248)."""

    @abc.abstractmethod
    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        ...

    @classmethod
    def __subclasshook__(cls, C) -> bool:
        if cls is Density:
            return _check_methods(C, "log_prob")
        return NotImplemented


class _Relaxed(ConditionalStraightThrough):
    """What the two relaxations share: the parameter they were built from, and the route to the kernels."""

    _family = GUMBEL
    has_enumerate_support = False
    has_rsample = True

    def _new(self, *args, **kwargs):
        return self._param.new(*args, **kwargs)

    def _data(self, param: torch.Tensor, *values: torch.Tensor):
        """The data arguments broadcast to ``sample_shape + param.shape`` (expanded on the host)."""
        shape = torch.broadcast_shapes(param.shape, *(v.shape for v in values))
        return tuple(v.expand(shape) for v in values)

    def _call(self, op: int, param: Optional[torch.Tensor], x1: torch.Tensor, x2: Optional[torch.Tensor] = None):
        return _relaxed(self._family, op, param, x1, x2)

    def rsample(self, sample_shape: Sequence = torch.Size()) -> torch.Tensor:
        logits = self.logits
        u = torch.rand(self._extended_shape(sample_shape), device=logits.device, dtype=logits.dtype)
        return self._call(RSAMPLE, logits, u)

    def log_prob(self, z: torch.Tensor) -> torch.Tensor:
        if self._validate_args:
            self._validate_sample(z)
        logits = self.logits
        return self._call(LOG_PROB, logits, *self._data(logits, z))

    def threshold(self, z: torch.Tensor, straight_through: bool = False) -> torch.Tensor:
        if self._validate_args:
            self._validate_sample(z)
        with torch.no_grad():
            b = self._call(THRESHOLD, None, z)
        if straight_through:
            b = b + z - z.detach()
        return b

    def csample(self, b: torch.Tensor) -> torch.Tensor:
        if self._validate_args:
            self._validate_thresholded_sample(b)
        v = torch.rand_like(b)
        probs = self.probs
        if _wants_grad(b):
            return _TORCH[self._family](CSAMPLE, probs, b, v)
        return self._call(CSAMPLE, probs, *self._data(probs, b, v))

    def clog_prob(self, zcond: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        if self._validate_args:
            self._validate_sample(zcond)
            self._validate_thresholded_sample(b)
        logits = self.logits
        if _wants_grad(b):
            return _TORCH[self._family](CLOG_PROB, logits, zcond, b)
        return self._call(CLOG_PROB, logits, *self._data(logits, zcond, b))

    @property
    def variance(self) -> torch.Tensor:
        return self.stddev.pow(2)

    def _constant(self, value: float, shape) -> torch.Tensor:
        return torch.tensor(value, device=self._param.device, dtype=self._param.dtype).expand(shape)


class LogisticBernoulli(_Relaxed):
    r"""A logistic distribution whose samples threshold to Bernoulli ones (reference
    _straight_through.py:251-412; [tucker2017]).

    The statistics and :func:`rsample` / :func:`log_prob` are those of the relaxed (logistic) variable
    :math:`z = logits + \log u - \log(1 - u)`; :func:`threshold` gives :math:`b = [z \ge 0]`, and
    :func:`csample` draws :math:`z` given :math:`b`.  On a ROCm device every method is one elementwise launch.
    """

    arg_constraints = {"probs": constraints.unit_interval, "logits": constraints.real}
    support = constraints.real
    thresholded_support = constraints.boolean
    _family = BERNOULLI

    def __init__(
        self,
        probs: Optional[torch.Tensor] = None,
        logits: Optional[torch.Tensor] = None,
        validate_args: Optional[bool] = None,
    ):
        if (probs is None) is (logits is None):
            raise ValueError("Either probs or logits must be specified, not both")
        if probs is not None:
            self._param = self.probs = argcheck.is_tensor(probs, "probs")
        else:
            self._param = self.logits = argcheck.is_tensor(logits, "logits")
        super().__init__(self._param.shape, validate_args=validate_args)

    @lazy_property
    def logits(self) -> torch.Tensor:
        return probs_to_logits(self.probs, is_binary=True)

    @lazy_property
    def probs(self) -> torch.Tensor:
        return logits_to_probs(self.logits, is_binary=True)

    def expand(self, batch_shape, _instance=None):
        new = self._get_checked_instance(LogisticBernoulli, _instance)
        batch_shape = torch.Size(batch_shape)
        if "probs" in self.__dict__:
            new._param = new.probs = self.probs.expand(batch_shape)
        if "logits" in self.__dict__:
            new._param = new.logits = self.logits.expand(batch_shape)
        super(LogisticBernoulli, new).__init__(batch_shape, validate_args=False)
        new._validate_args = self._validate_args
        return new

    def tlog_prob(self, b: torch.Tensor) -> torch.Tensor:
        if self._validate_args:
            self._validate_thresholded_sample(b)
        logits = self.logits
        if _wants_grad(b):
            return _bernoulli_torch(TLOG_PROB, logits, b, None)
        return self._call(TLOG_PROB, logits, *self._data(logits, b))

    @property
    def mean(self) -> torch.Tensor:
        return self.logits

    @property
    def stddev(self) -> torch.Tensor:
        return self._constant(math.pi / math.sqrt(3), self.batch_shape)

    def entropy(self) -> torch.Tensor:
        return self._constant(2, self.batch_shape)


class GumbelOneHotCategorical(_Relaxed):
    r"""Independent Gumbel variables, normalised over the last dimension, whose arg-max is a one-hot categorical
    sample (reference _straight_through.py:415-598; [tucker2017]).

    The statistics and :func:`rsample` / :func:`log_prob` are those of the relaxed variable
    :math:`z = logits - \log(-\log u)`; :func:`threshold` gives the one-hot of the row's arg-max (the lowest
    index of a tie; ``-0`` and ``+0`` tie; a NaN is the maximum), and :func:`csample` draws :math:`z` given
    :math:`b`.  On a ROCm device every method is one launch that reads each row once.

    :func:`tlog_prob` is the sum of the logits where ``b`` is nonzero.  Wherever the reference returns, that is
    its value; for a ``b`` that is not one-hot, with validation off, the reference fails on a ``view`` and the
    sum is returned here.  :func:`csample` takes the first nonzero of a row of ``b`` as the hot index.
    """

    arg_constraints = {"probs": constraints.simplex, "logits": constraints.real_vector}
    support = constraints.real_vector
    thresholded_support = constraints.one_hot
    _family = GUMBEL

    def __init__(
        self,
        logits: Optional[torch.Tensor] = None,
        probs: Optional[torch.Tensor] = None,
        validate_args: Optional[bool] = None,
    ):
        if (probs is None) is (logits is None):
            raise ValueError("Either probs or logits must be specified, not both")
        if probs is not None:
            probs = argcheck.is_tensor(probs, "probs")
            if probs.dim() < 1:
                raise ValueError("probs must be at least 1 dimensional")
            self._param = self.probs = probs / probs.sum(-1, keepdim=True)
        else:
            logits = argcheck.is_tensor(logits, "logits")
            if logits.dim() < 1:
                raise ValueError("logits must be at least 1 dimensional")
            self._param = self.logits = logits.log_softmax(-1)
        shape = self._param.shape
        super().__init__(shape[:-1], shape[-1:], validate_args=validate_args)

    @lazy_property
    def logits(self) -> torch.Tensor:
        return probs_to_logits(self.probs)

    @lazy_property
    def probs(self) -> torch.Tensor:
        logits = self.logits
        if logits.device.type == "cuda" and logits.dtype == torch.float64:
            # the logits are normalised, so exp gives the probabilities; torch's device softmax of a float64 row
            # beyond 1024 elements is only good to float32 (profiles/softmax_f64.json: 1e-6 relative at V = 1500)
            return logits.exp()
        return logits_to_probs(logits)

    def expand(self, batch_shape, _instance=None):
        new = self._get_checked_instance(GumbelOneHotCategorical, _instance)
        batch_shape = torch.Size(batch_shape)
        param_shape = batch_shape + self.event_shape
        if "probs" in self.__dict__:
            new._param = new.probs = self.probs.expand(param_shape)
        if "logits" in self.__dict__:
            new._param = new.logits = self.logits.expand(param_shape)
        super(GumbelOneHotCategorical, new).__init__(batch_shape, self.event_shape, validate_args=False)
        new._validate_args = self._validate_args
        return new

    def tlog_prob(self, b: torch.Tensor) -> torch.Tensor:
        if self._validate_args:
            self._validate_thresholded_sample(b)
        logits = self.logits
        return self._call(TLOG_PROB, logits, *self._data(logits, b.detach()))

    @property
    def mean(self) -> torch.Tensor:
        return self.logits + _EULER

    @property
    def stddev(self) -> torch.Tensor:
        return self._constant(math.pi / math.sqrt(6), self._extended_shape())

    def entropy(self) -> torch.Tensor:
        return self._constant(self.event_shape[0] * (1 + _EULER), self.batch_shape)


class _RebarControlVariate(torch.nn.Module):
    """``eta * func(sigma(z / exp(log_temp)))`` (reference _mc.py:751-840): REBAR [tucker2017] as the control
    variate of RELAX [grathwohl2017].  ``func`` must accept relaxed samples.  ``log_temp`` starts at
    ``log(start_temp)`` and ``eta`` at ``start_eta``.  Plain torch ops: traceable (not scriptable), and
    differentiable as often as ``func`` is in ``z``, ``log_temp`` and ``eta``."""

    __constants__ = ("func", "start_temp", "start_eta")

    def __init__(self, func, start_temp: float = 0.1, start_eta: float = 1.0) -> None:
        start_temp = argcheck.is_posf(start_temp, "start_temp")
        start_eta = argcheck.is_float(start_eta, "start_eta")
        super().__init__()
        self.func, self.start_temp, self.start_eta = func, start_temp, start_eta
        self.log_temp = torch.nn.Parameter(torch.empty(1))
        self.eta = torch.nn.Parameter(torch.empty(1))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        self.log_temp.data.fill_(self.start_temp).log_()
        self.eta.data.fill_(self.start_eta)

    def extra_repr(self) -> str:
        return "start_temp={},start_eta={}".format(self.start_temp, self.start_eta)


class LogisticBernoulliRebarControlVariate(_RebarControlVariate):
    __doc__ = "REBAR control variate for :class:`LogisticBernoulli`: sigma is the sigmoid; ``z`` is ``(*)``.\n\n" + (
        _RebarControlVariate.__doc__
    )

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        return self.eta * self.func((z / self.log_temp.exp()).sigmoid())


class GumbelOneHotCategoricalRebarControlVariate(_RebarControlVariate):
    __doc__ = (
        "REBAR control variate for :class:`GumbelOneHotCategorical`: sigma is the softmax over the last "
        "dimension; ``z`` is ``(*, V)``.\n\n" + _RebarControlVariate.__doc__
    )

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        return self.eta * self.func((z / self.log_temp.exp()).softmax(-1))
