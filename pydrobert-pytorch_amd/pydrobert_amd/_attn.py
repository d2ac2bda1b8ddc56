"""Soft attention on MI355X (reference _attn.py:26-603): the five attention modules with the reference's
signatures, parameters, initialisation order and error types.

On a ROCm device (float32 / float64 / float16 / bfloat16) the scores, the masked softmax and the weighted sum of
values run as one HIP pass (``csrc/attn.hip``) that reads every key and value row once per group of rows sharing them, where the
reference materialises two products at the full broadcast shape.  Dot-product and generalized dot-product
attention make one operator call, ``pydrobert_amd::dot_attention``: the generalized form transforms the query
(``query @ weight``) instead of every key, and drops ``query . bias``, which is constant along ``dim`` and
cancels in the softmax.  ``ConcatSoftAttention`` applies the two halves of its ``W`` in torch and sums
``v . tanh`` in ``pydrobert_amd::concat_score`` (``csrc/concat_score.hip``), which builds no hidden-sized
tensor; a subclass with its own ``score`` computes it with torch.  Either score then goes to
``pydrobert_amd::attention_pool`` for the masked softmax and the weighted sum.
float16 / bfloat16 operands are read and written as they are (the ``_elem`` entry points: no float32 copy of any
operand), computed in float32 and rounded once where a result is stored; ``lse`` is float32 for them.
CPU tensors, other dtypes and operands of mixed dtypes run the reference's formulas in torch.

Deviation: a masked frame contributes exactly 0 on the HIP path, where the reference multiplies it by 0 (a
non-finite key or value in a masked frame gives NaN there and not here).
"""
import abc
from typing import List, Optional, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck

__all__ = [
    "ConcatSoftAttention",
    "DotProductSoftAttention",
    "GeneralizedDotProductSoftAttention",
    "GlobalSoftAttention",
    "MultiHeadedAttention",
]

_MAX_DIMS = 8  # PDT_ATTN_MAX_DIMS
_SLOTS = 8  # query / score, key, value, mask, out, grad query / score, grad key, grad value
_DESC_LEN = 7 + _MAX_DIMS + _SLOTS * (_MAX_DIMS + 2)
_SQ, _SK, _SV, _SM, _SO, _SGQ, _SGK, _SGV = range(_SLOTS)
_KIND_DOT, _KIND_DOT_BWD, _KIND_POOL, _KIND_POOL_BWD = 0, 1, 2, 3


def _bshape(a: List[int], b: List[int]) -> List[int]:
    """Broadcast two shapes (RuntimeError if they do not), scriptable."""
    n = max(len(a), len(b))
    out: List[int] = []
    for i in range(n):
        x = a[i - n + len(a)] if i - n + len(a) >= 0 else 1
        y = b[i - n + len(b)] if i - n + len(b) >= 0 else 1
        if x != y and x != 1 and y != 1:
            raise RuntimeError("shapes {} and {} do not broadcast".format(a, b))
        out.append(y if x == 1 else x)
    return out


def _prod(sizes: List[int]) -> int:
    p = 1
    for s in sizes:
        p *= s
    return p


def _check_input(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    mask: Optional[torch.Tensor],
    query_size: int,
    key_size: int,
    dim: int,
    runtime: bool,
) -> None:
    """The reference's check_input: ValueError for GlobalSoftAttention, RuntimeError (``runtime``) for
    MultiHeadedAttention; broadcast failures are RuntimeErrors in both."""
    key_dim = key.dim()
    msg = ""
    if query.dim() != key_dim - 1:
        msg = "query must have one fewer dimension than key"
    elif key_dim != value.dim():
        msg = "key must have same number of dimensions as value"
    elif query.shape[-1] != query_size:
        msg = "Last dimension of query must match query_size"
    elif key.shape[-1] != key_size:
        msg = "Last dimension of key must match key_size"
    elif dim > key_dim - 2 or key_dim == -1 or dim < -key_dim + 1:
        msg = "dim must be in the range [{}, {}] and not -1".format(-key_dim + 1, key_dim - 2)
    if msg != "":
        if runtime:
            raise RuntimeError(msg)
        raise ValueError(msg)
    e_shape = _bshape(list(query.unsqueeze(dim).shape[:-1]), list(key.shape[:-1]))
    if mask is not None:
        _bshape(e_shape, list(mask.shape))
    _bshape(e_shape + [1], list(value.shape))


def _softmax_pool(e: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor], dim: int) -> torch.Tensor:
    """The reference's formula (_attn.py:219-223), for CPU tensors and other dtypes."""
    if mask is not None:
        e = e.masked_fill(~mask, -float("inf"))
    a = torch.nn.functional.softmax(e, dim)
    return (a.unsqueeze(-1) * value).sum(dim)


def _hip_route(e_shape: List[int], value: torch.Tensor, mask: Optional[torch.Tensor], dim: int,
               tensors: List[torch.Tensor], width: int) -> bool:  # fmt: skip
    """True when the kernels compute what the reference's formula does: ROCm float32 / float64 / float16 /
    bfloat16 tensors of one dtype, a non-negative ``dim`` (with a negative one the reference's softmax and sum see
    different axes), a bool mask that adds no dimension, a softmax axis as long as the summed one and at most eight row dims;
    and one row of the tiles the kernels keep in LDS (``width`` features: D + Dv, or Dv for a given score)
    fits their 56 KiB (the half types' tiles are float32)."""
    dt = tensors[0].dtype
    if dt != torch.float32 and dt != torch.float64 and dt != torch.float16 and dt != torch.bfloat16:
        return False
    if width * (8 if dt == torch.float64 else 4) > 57344:  # (kAttnLdsBytes)
        return False
    for t in tensors:
        if not t.is_cuda or t.dtype != dt:
            return False
    if dim < 0:
        return False
    n = len(e_shape)
    soft = e_shape
    if mask is not None:
        if not mask.is_cuda or mask.dtype != torch.bool or mask.dim() > n:
            return False
        soft = _bshape(soft, list(mask.shape))
    full = _bshape(soft, list(value.shape[:-1]))
    if len(full) != n or soft[dim] != full[dim]:
        return False
    rows = 0
    for i in range(n):
        if i != dim and full[i] > 1:
            rows += 1
    return rows <= 8  # (PDT_ATTN_MAX_DIMS)


# ----------------------------------------------------------------------------------------------------------
# operators


_HALF = (torch.float16, torch.bfloat16)


def _dtype_code(x: torch.Tensor, *others, mask=None, half=False) -> int:
    """The kernels' code of the operands' one dtype: 0 float32, 1 float64 and, with ``half`` (the attention
    operators, whose ``_elem`` entry points take them), 2 float16, 3 bfloat16."""
    if x.dtype not in (torch.float32, torch.float64) + (_HALF if half else ()):
        raise TypeError("the attention kernels take {} tensors, got {}".format(
            "float32, float64, float16 or bfloat16" if half else "float32 or float64", x.dtype))  # fmt: skip
    for t in others:
        if t.dtype != x.dtype:
            raise TypeError("attention operands of different dtypes: {} and {}".format(x.dtype, t.dtype))
    if mask is not None and mask.dtype != torch.bool:
        raise RuntimeError("the attention mask must be a bool tensor, got {}".format(mask.dtype))
    return {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}[x.dtype]


def _entry(name: str, dt: int):
    """The entry point of an attention call: float16 / bfloat16 (codes 2, 3) go to the ``_elem`` sibling."""
    return getattr(_cabi.lib(), name + "_elem" if dt >= 2 else name)


def _lse_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.float32 if dtype in _HALF else dtype


def _sum_to(g: torch.Tensor, shape) -> torch.Tensor:
    """``g.sum_to_size(shape)``: what broadcast an input had beyond the group.  A half gradient that is reduced
    is summed in float32 and rounded once; one of the input's shape is returned as it is."""
    if list(g.shape) == list(shape):
        return g
    if g.dtype in _HALF:
        return g.float().sum_to_size(shape).to(g.dtype)
    return g.sum_to_size(shape)


def _full_shape(e_shape, value, mask):
    s = list(e_shape)
    if mask is not None:
        s = _bshape(s, list(mask.shape))
    return _bshape(s, list(value.shape[:-1]))


def _expand(x: torch.Tensor, shape: List[int]) -> torch.Tensor:
    return x.view([1] * (len(shape) - x.dim()) + list(x.shape)).expand(shape)


class _Plan:
    """Everything a kernel call needs about shapes: the full shape S (rows and T), the descriptor, and the
    contiguous layouts the kernels write (out / grad_query in S's row order; grad_key / grad_value with the
    group's dims at 1; grad_score at S)."""

    def __init__(self, S, d, D, Dv, operands, shared, pool):
        n = len(S)
        self.S, self.d, self.T = S, d, S[d]
        self.out_shape = S[:d] + S[d + 1:] + [Dv]
        rows = [i for i in range(n) if i != d and S[i] > 1]
        if len(rows) > _MAX_DIMS:
            raise RuntimeError("attention over more than {} broadcast row dims".format(_MAX_DIMS))
        # the group: dims where the caller's key and value have size 1 (not merely stride 0: a key the caller
        # expanded has a gradient per slice, which autograd's expand then sums)
        group = [i for i in rows if all(t.shape[i] == 1 for t in shared)]
        outer = [i for i in rows if i not in group]
        self.order = outer + group
        self.R = _prod(self.out_shape[:-1])
        self.M = _prod([S[i] for i in group])
        self.G = _prod([S[i] for i in outer])
        self.shared_shape = [1 if i in group else S[i] for i in range(n)]
        desc = [0] * _DESC_LEN
        desc[0:7] = [len(self.order), self.R, self.G, self.M, self.T, 0 if pool else D, Dv]
        for j, i in enumerate(self.order):
            desc[7 + j] = S[i]
        out_st = _contig_strides(self.out_shape)
        gq_st = _contig_strides(self.out_shape[:-1] + [D])
        ge_st = _contig_strides(S)
        for slot in range(_SLOTS):
            base = 7 + _MAX_DIMS + slot * (_MAX_DIMS + 2)
            if slot in (_SQ, _SK, _SV, _SM):
                t = operands[slot]
                if t is None:
                    continue
                st = list(t.stride())
                row_st = [st[i] for i in range(n)]
                ts, fs = st[d], (st[n] if slot != _SM and not (pool and slot == _SQ) else 0)
            elif slot == _SO or (slot == _SGQ and not pool):
                st = out_st if slot == _SO else gq_st
                row_st = [st[i if i < d else i - 1] if i != d else 0 for i in range(n)]
                ts, fs = 0, st[-1]
            elif slot == _SGQ:  # grad score, at S
                row_st, ts, fs = [ge_st[i] for i in range(n)], ge_st[d], 0
            else:
                width = D if slot == _SGK else Dv
                if slot == _SGK and pool:
                    continue
                st = _contig_strides(self.shared_shape + [width])
                row_st = [0 if i in group else st[i] for i in range(n)]
                ts, fs = st[d], 1
            for j, i in enumerate(self.order):
                desc[base + j] = row_st[i]
            desc[base + _MAX_DIMS] = ts
            desc[base + _MAX_DIMS + 1] = fs
        self.desc = torch.tensor(desc, dtype=torch.int64)


def _contig_strides(shape: List[int]) -> List[int]:
    st = [1] * len(shape)
    for i in range(len(shape) - 2, -1, -1):
        st[i] = st[i + 1] * max(shape[i + 1], 1)
    return st


def _workspace(plan: _Plan, dt: int, kind: int, device) -> torch.Tensor:
    nbytes = _entry("pdt_attn_workspace_bytes", dt)(plan.desc.data_ptr(), dt, kind)
    if nbytes < 0:
        raise RuntimeError("pdt_attn_workspace_bytes: invalid descriptor")
    return torch.empty((max(1, nbytes),), device=device, dtype=torch.uint8)


def _saved(out: torch.Tensor, lse: torch.Tensor, plan: _Plan, dtype: torch.dtype):
    """The forward's results as the backward kernels read them: ``out`` contiguous at the plan's shape in the
    operands' dtype, ``lse`` (2, rows) in float32 for half operands (a wrong size would be read out of bounds)."""
    if list(out.shape) != plan.out_shape or out.dtype != dtype:
        raise RuntimeError("attention backward: out must be the forward's output, {} of {}; got {} of {}".format(
            plan.out_shape, dtype, list(out.shape), out.dtype))  # fmt: skip
    if list(lse.shape) != [2, plan.R] or lse.dtype != _lse_dtype(dtype):
        raise RuntimeError("attention backward: lse must be the forward's, {} of {}; got {} of {}".format(
            [2, plan.R], _lse_dtype(dtype), list(lse.shape), lse.dtype))  # fmt: skip
    return out.detach().contiguous(), lse.detach().contiguous()


def _dot_geometry(query, key, value, mask, dim):
    if dim < 0 or dim > key.dim() - 2:
        raise RuntimeError("dot_attention takes a dim in [0, {}], got {}".format(key.dim() - 2, dim))
    q1 = query.unsqueeze(dim)
    e_shape = _bshape(list(q1.shape[:-1]), list(key.shape[:-1]))
    return q1, _full_shape(e_shape, value, mask)


def _dot_plan(query, key, value, mask, dim):
    q1, S = _dot_geometry(query, key, value, mask, dim)
    D, Dv = query.shape[-1], value.shape[-1]
    ops = [
        q1.expand(S + [D]), key.expand(S + [D]), value.expand(S + [Dv]),
        None if mask is None else _expand(mask, S),
    ]  # fmt: skip
    return _Plan(S, dim, D, Dv, ops, [key, value], False), ops


@custom_op("pydrobert_amd::dot_attention", mutates_args=())
def _dot_attention_op(
    query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor], dim: int,
    scale: float,
) -> Tuple[torch.Tensor, torch.Tensor]:  # fmt: skip
    """(out, lse): softmax over ``dim`` of ``scale * query . key`` (masked frames at -inf), then the weighted
    sum of ``value`` over ``dim``; lse is (2, rows), the per-row maximum and log of the sum of exp(score - maximum)
    that the backward reads, in the kernel's row order (kept apart: their sum would round away the second next
    to a large |score|)."""
    device = _cabi.require_hip(query, key, value, mask)
    dt = _dtype_code(query, key, value, mask=mask, half=True)
    plan, ops = _dot_plan(query, key, value, mask, dim)
    out = torch.empty(plan.out_shape, device=device, dtype=query.dtype)
    lse = torch.empty((2, plan.R), device=device, dtype=_lse_dtype(query.dtype))
    if plan.R == 0:
        return out, lse
    if plan.T == 0:
        return out.zero_(), lse.fill_(-float("inf"))
    ws = _workspace(plan, dt, _KIND_DOT, device)
    scale_c = _cabi.ctypes.c_double(scale)
    with _cabi.on_device(device):
        rc = _entry("pdt_attn_dot", dt)(
            plan.desc.data_ptr(), dt, ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), _cabi.ptr(ops[3]),
            _cabi.ctypes.addressof(scale_c), out.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(),
            _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_attn_dot")
    return out, lse


@_dot_attention_op.register_fake
def _(query, key, value, mask, dim, scale):
    _, S = _dot_geometry(query, key, value, mask, dim)
    out_shape = S[:dim] + S[dim + 1:] + [value.shape[-1]]
    return query.new_empty(out_shape), query.new_empty((2, _prod(out_shape[:-1])), dtype=_lse_dtype(query.dtype))


@custom_op("pydrobert_amd::dot_attention_backward", mutates_args=())
def _dot_attention_backward_op(
    grad_out: torch.Tensor, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
    mask: Optional[torch.Tensor], out: torch.Tensor, lse: torch.Tensor, dim: int, scale: float,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:  # fmt: skip
    """(grad_query, grad_key, grad_value) in the inputs' shapes.  The kernels sum grad_key / grad_value over
    the group; what other broadcast an input had is summed here."""
    device = _cabi.require_hip(grad_out, query, key, value, mask, out, lse)
    dt = _dtype_code(query, key, value, mask=mask, half=True)
    plan, ops = _dot_plan(query, key, value, mask, dim)
    D, Dv = query.shape[-1], value.shape[-1]
    if plan.R == 0 or plan.T == 0:
        return torch.zeros_like(query), torch.zeros_like(key), torch.zeros_like(value)
    g = grad_out.detach().to(query.dtype).contiguous()
    if list(g.shape) != plan.out_shape:
        raise RuntimeError("attention backward: grad_out of shape {}, out has {}".format(list(g.shape), plan.out_shape))
    out_c, lse_c = _saved(out, lse, plan, query.dtype)
    gq = torch.empty(plan.out_shape[:-1] + [D], device=device, dtype=query.dtype)
    gk = torch.empty(plan.shared_shape + [D], device=device, dtype=query.dtype)
    gv = torch.empty(plan.shared_shape + [Dv], device=device, dtype=query.dtype)
    ws = _workspace(plan, dt, _KIND_DOT_BWD, device)
    scale_c = _cabi.ctypes.c_double(scale)
    with _cabi.on_device(device):
        rc = _entry("pdt_attn_dot_backward", dt)(
            plan.desc.data_ptr(), dt, ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), _cabi.ptr(ops[3]),
            _cabi.ctypes.addressof(scale_c), out_c.data_ptr(), lse_c.data_ptr(), g.data_ptr(), gq.data_ptr(),
            gk.data_ptr(), gv.data_ptr(), ws.data_ptr(), ws.numel(), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_attn_dot_backward")
    q1_shape = list(query.unsqueeze(dim).shape)
    gq = _sum_to(gq.unsqueeze(dim), q1_shape).squeeze(dim)
    return gq.reshape(query.shape), _sum_to(gk, key.shape), _sum_to(gv, value.shape)


@_dot_attention_backward_op.register_fake
def _(grad_out, query, key, value, mask, out, lse, dim, scale):
    return torch.empty_like(query), torch.empty_like(key), torch.empty_like(value)


def _pool_geometry(score, value, mask, dim):
    if dim < 0 or dim > score.dim() - 1 or score.dim() != value.dim() - 1:
        raise RuntimeError("attention_pool takes a score of value's dims minus one and dim in [0, {}]".format(
            value.dim() - 2))  # fmt: skip
    return _full_shape(list(score.shape), value, mask)


def _pool_plan(score, value, mask, dim):
    S = _pool_geometry(score, value, mask, dim)
    Dv = value.shape[-1]
    ops = [score.expand(S), None, value.expand(S + [Dv]), None if mask is None else _expand(mask, S)]
    return _Plan(S, dim, 0, Dv, ops, [value], True), ops


@custom_op("pydrobert_amd::attention_pool", mutates_args=())
def _attention_pool_op(
    score: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor], dim: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, lse): the masked softmax of ``score`` over ``dim`` and the weighted sum of ``value``."""
    device = _cabi.require_hip(score, value, mask)
    dt = _dtype_code(score, value, mask=mask, half=True)
    plan, ops = _pool_plan(score, value, mask, dim)
    out = torch.empty(plan.out_shape, device=device, dtype=score.dtype)
    lse = torch.empty((2, plan.R), device=device, dtype=_lse_dtype(score.dtype))
    if plan.R == 0:
        return out, lse
    if plan.T == 0:
        return out.zero_(), lse.fill_(-float("inf"))
    ws = _workspace(plan, dt, _KIND_POOL, device)
    with _cabi.on_device(device):
        rc = _entry("pdt_attn_pool", dt)(
            plan.desc.data_ptr(), dt, ops[0].data_ptr(), ops[2].data_ptr(), _cabi.ptr(ops[3]), out.data_ptr(),
            lse.data_ptr(), ws.data_ptr(), ws.numel(), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_attn_pool")
    return out, lse


@_attention_pool_op.register_fake
def _(score, value, mask, dim):
    S = _pool_geometry(score, value, mask, dim)
    out_shape = S[:dim] + S[dim + 1:] + [value.shape[-1]]
    return score.new_empty(out_shape), score.new_empty((2, _prod(out_shape[:-1])), dtype=_lse_dtype(score.dtype))


@custom_op("pydrobert_amd::attention_pool_backward", mutates_args=())
def _attention_pool_backward_op(
    grad_out: torch.Tensor, score: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor],
    out: torch.Tensor, lse: torch.Tensor, dim: int,
) -> Tuple[torch.Tensor, torch.Tensor]:  # fmt: skip
    """(grad_score, grad_value) in the inputs' shapes."""
    device = _cabi.require_hip(grad_out, score, value, mask, out, lse)
    dt = _dtype_code(score, value, mask=mask, half=True)
    plan, ops = _pool_plan(score, value, mask, dim)
    if plan.R == 0 or plan.T == 0:
        return torch.zeros_like(score), torch.zeros_like(value)
    g = grad_out.detach().to(score.dtype).contiguous()
    if list(g.shape) != plan.out_shape:
        raise RuntimeError("attention backward: grad_out of shape {}, out has {}".format(list(g.shape), plan.out_shape))
    out_c, lse_c = _saved(out, lse, plan, score.dtype)
    ge = torch.empty(plan.S, device=device, dtype=score.dtype)
    gv = torch.empty(plan.shared_shape + [value.shape[-1]], device=device, dtype=score.dtype)
    ws = _workspace(plan, dt, _KIND_POOL_BWD, device)
    with _cabi.on_device(device):
        rc = _entry("pdt_attn_pool_backward", dt)(
            plan.desc.data_ptr(), dt, ops[0].data_ptr(), ops[2].data_ptr(), _cabi.ptr(ops[3]), out_c.data_ptr(),
            lse_c.data_ptr(), g.data_ptr(), ge.data_ptr(), gv.data_ptr(), ws.data_ptr(), ws.numel(),
            _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_attn_pool_backward")
    return _sum_to(ge, score.shape), _sum_to(gv, value.shape)


@_attention_pool_backward_op.register_fake
def _(grad_out, score, value, mask, out, lse, dim):
    return torch.empty_like(score), torch.empty_like(value)


def _dot_setup_context(ctx, inputs, output):
    query, key, value, mask, dim, scale = inputs
    out, lse = output
    ctx.save_for_backward(query, key, value, mask, out, lse)
    ctx.cfg = (dim, scale)
    ctx.mark_non_differentiable(lse)


def _dot_backward(ctx, grad_out, grad_lse):
    query, key, value, mask, out, lse = ctx.saved_tensors
    dim, scale = ctx.cfg
    gq, gk, gv = torch.ops.pydrobert_amd.dot_attention_backward(grad_out, query, key, value, mask, out, lse, dim, scale)
    need = ctx.needs_input_grad
    return gq if need[0] else None, gk if need[1] else None, gv if need[2] else None, None, None, None


def _pool_setup_context(ctx, inputs, output):
    score, value, mask, dim = inputs
    out, lse = output
    ctx.save_for_backward(score, value, mask, out, lse)
    ctx.dim = dim
    ctx.mark_non_differentiable(lse)


def _pool_backward(ctx, grad_out, grad_lse):
    score, value, mask, out, lse = ctx.saved_tensors
    ge, gv = torch.ops.pydrobert_amd.attention_pool_backward(grad_out, score, value, mask, out, lse, ctx.dim)
    need = ctx.needs_input_grad
    return ge if need[0] else None, gv if need[1] else None, None, None


def _no_double_backward(ctx, *grads):
    raise RuntimeError(
        "pydrobert_amd attention: double backward is not supported (the backward kernels are not differentiable)"
    )


def _setup_nothing(ctx, inputs, output):
    pass


register_autograd("pydrobert_amd::dot_attention", _dot_backward, setup_context=_dot_setup_context)
register_autograd("pydrobert_amd::attention_pool", _pool_backward, setup_context=_pool_setup_context)
register_autograd("pydrobert_amd::dot_attention_backward", _no_double_backward, setup_context=_setup_nothing)
register_autograd("pydrobert_amd::attention_pool_backward", _no_double_backward, setup_context=_setup_nothing)


def dot_attention(
    query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor], dim: int,
    scale: float,
) -> torch.Tensor:  # fmt: skip
    """The fused dot-product attention of ROCm tensors (``pydrobert_amd::dot_attention``'s output)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(query, key, value, mask):
            return _dot_attention_op._init_fn(query, key, value, mask, dim, scale)[0]
    return torch.ops.pydrobert_amd.dot_attention(query, key, value, mask, dim, scale)[0]


def attention_pool(score: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor], dim: int) -> torch.Tensor:
    """The masked softmax of ``score`` over ``dim`` and the weighted sum of ``value``, on ROCm tensors."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(score, value, mask):
            return _attention_pool_op._init_fn(score, value, mask, dim)[0]
    return torch.ops.pydrobert_amd.attention_pool(score, value, mask, dim)[0]


# ----------------------------------------------------------------------------------------------------------
# the fused ConcatSoftAttention score (csrc/concat_score.hip)

_CA, _CB, _CGE, _CE, _CGA, _CGB = 0, 1, 3, 4, 5, 6  # the descriptor slots the concat kernels read


def _concat_geometry(wq: torch.Tensor, wk: torch.Tensor, v: torch.Tensor, dim: int) -> List[int]:
    n = wk.dim() - 1
    if wq.dim() != wk.dim() or n < 1 or dim < 0 or dim > n - 1 or wq.shape[dim] != 1:
        raise RuntimeError(
            "concat_score takes wq and wk of the same number of dims, a dim in [0, {}] and wq of size 1 "
            "along it".format(n - 1)
        )
    if v.dim() != 1 or wq.shape[-1] != v.shape[0] or wk.shape[-1] != v.shape[0]:
        raise RuntimeError("concat_score: the last dimension of wq and wk must be v's size")
    return _bshape(list(wq.shape[:-1]), list(wk.shape[:-1]))


class _ConcatPlan:
    """The rows x T x H reduction of a concat_score call (the row / group rule of _Plan: the row dims where
    ``wk`` has size 1 form the group and go innermost), its descriptor, and the contiguous layouts the kernels
    write: e at S, grad_wq at S with ``dim`` at 1, grad_wk with the group's dims at 1."""

    def __init__(self, wq, wk, v, dim, grad_e=None):
        S = _concat_geometry(wq, wk, v, dim)
        n, H = len(S), v.shape[0]
        self.S, self.T, self.H = S, S[dim], H
        rows = [i for i in range(n) if i != dim and S[i] != 1]  # (a dim of size 0 is a row dim: R is then 0)
        if len(rows) > _MAX_DIMS:
            raise RuntimeError("concat_score over more than {} broadcast row dims".format(_MAX_DIMS))
        group = [i for i in rows if wk.shape[i] == 1]
        order = [i for i in rows if i not in group] + group
        self.R = _prod([S[i] for i in rows])
        self.M = _prod([S[i] for i in group])
        self.ga_shape = [1 if i == dim else S[i] for i in range(n)] + [H]
        self.gb_shape = [1 if i in group else S[i] for i in range(n)] + [H]
        desc = [0] * _DESC_LEN
        desc[0:7] = [len(order), self.R, self.R // max(self.M, 1), self.M, self.T, H, v.stride(0)]
        for j, i in enumerate(order):
            desc[7 + j] = S[i]
        a_st, b_st = list(wq.expand(S + [H]).stride()), list(wk.expand(S + [H]).stride())
        strides = {
            _CA: a_st, _CB: b_st, _CE: _contig_strides(S) + [0], _CGA: _contig_strides(self.ga_shape),
            _CGB: [0 if i in group else st for i, st in enumerate(_contig_strides(self.gb_shape))],
        }  # fmt: skip
        if grad_e is not None:
            strides[_CGE] = list(grad_e.stride()) + [0]
        for slot, st in strides.items():
            base = 7 + _MAX_DIMS + slot * (_MAX_DIMS + 2)
            for j, i in enumerate(order):
                desc[base + j] = st[i]
            desc[base + _MAX_DIMS] = st[dim]
            desc[base + _MAX_DIMS + 1] = st[n]
        self.desc = torch.tensor(desc, dtype=torch.int64)


def _concat_backward_torch(grad_e: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, v: torch.Tensor):
    """The three gradients of v . tanh(wq + wk) in differentiable torch operations."""
    th = torch.tanh(wq + wk)
    ge = grad_e.unsqueeze(-1)
    g = ge * v * (1 - th * th)
    return g.sum_to_size(wq.shape), g.sum_to_size(wk.shape), (ge * th).reshape(-1, v.shape[0]).sum(0)


@custom_op("pydrobert_amd::concat_score", mutates_args=())
def _concat_score_op(wq: torch.Tensor, wk: torch.Tensor, v: torch.Tensor, dim: int) -> torch.Tensor:
    """e = sum_h v[h] tanh(wq + wk)[..., h] at the broadcast of ``wq`` (size 1 along ``dim``) and ``wk``, without
    the hidden-sized intermediate."""
    device = _cabi.require_hip(wq, wk, v)
    dt = _dtype_code(wq, wk, v)
    plan = _ConcatPlan(wq, wk, v, dim)
    if plan.H == 0:  # (the sum over no hidden units)
        return torch.zeros(plan.S, device=device, dtype=wq.dtype)
    e = torch.empty(plan.S, device=device, dtype=wq.dtype)
    if plan.R == 0 or plan.T == 0:  # (an empty score: a batch dim or the attended axis of size 0)
        return e
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_concat_score(
            plan.desc.data_ptr(), dt, wq.data_ptr(), wk.data_ptr(), v.data_ptr(), e.data_ptr(),
            _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_concat_score")
    return e


@_concat_score_op.register_fake
def _(wq, wk, v, dim):
    return wq.new_empty(_concat_geometry(wq, wk, v, dim))


@custom_op("pydrobert_amd::concat_score_backward", mutates_args=())
def _concat_score_backward_op(
    grad_e: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, v: torch.Tensor, dim: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(grad_wq, grad_wk, grad_v) in the inputs' shapes, tanh recomputed.  The kernels sum grad_wk over the
    group; what other broadcast ``wq`` had is summed here."""
    device = _cabi.require_hip(grad_e, wq, wk, v)
    dt = _dtype_code(wq, wk, v)
    g = grad_e.detach().to(wq.dtype)
    plan = _ConcatPlan(wq, wk, v, dim, g.expand(_concat_geometry(wq, wk, v, dim)))
    if plan.R == 0 or plan.T == 0 or plan.H == 0:
        return torch.zeros_like(wq), torch.zeros_like(wk), torch.zeros_like(v)
    nbytes = _cabi.lib().pdt_concat_score_workspace_bytes(plan.desc.data_ptr(), dt, 1)
    if nbytes < 0:
        raise RuntimeError("pdt_concat_score_workspace_bytes: invalid descriptor")
    ws = torch.empty((max(1, nbytes),), device=device, dtype=torch.uint8)
    ga = torch.empty(plan.ga_shape, device=device, dtype=wq.dtype)
    gb = torch.empty(plan.gb_shape, device=device, dtype=wq.dtype)
    gv = torch.empty((plan.H,), device=device, dtype=wq.dtype)
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_concat_score_backward(
            plan.desc.data_ptr(), dt, wq.data_ptr(), wk.data_ptr(), v.data_ptr(), g.data_ptr(), ga.data_ptr(),
            gb.data_ptr(), gv.data_ptr(), ws.data_ptr(), ws.numel(), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_concat_score_backward")
    return ga.sum_to_size(wq.shape), gb.sum_to_size(wk.shape), gv


@_concat_score_backward_op.register_fake
def _(grad_e, wq, wk, v, dim):
    return torch.empty_like(wq), torch.empty_like(wk), torch.empty_like(v)


def _concat_setup_context(ctx, inputs, output):
    wq, wk, v, dim = inputs
    ctx.save_for_backward(wq, wk, v)
    ctx.dim = dim


def _concat_backward(ctx, grad_e):
    wq, wk, v = ctx.saved_tensors
    ga, gb, gv = torch.ops.pydrobert_amd.concat_score_backward(grad_e, wq, wk, v, ctx.dim)
    need = ctx.needs_input_grad
    return ga if need[0] else None, gb if need[1] else None, gv if need[2] else None, None


def _concat_backward_setup_context(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:4])


def _concat_backward_backward(ctx, gg_wq, gg_wk, gg_v):
    """The derivative of the backward operator: the torch body's, in differentiable torch operations."""
    saved = ctx.saved_tensors
    with torch.enable_grad():
        leaves = [t.detach().requires_grad_() for t in saved]
        outs = _concat_backward_torch(*leaves)
        live = [(o, gg) for o, gg in zip(outs, (gg_wq, gg_wk, gg_v)) if gg is not None and o.requires_grad]
        targets = [t for i, t in enumerate(leaves) if ctx.needs_input_grad[i]]
        second = iter(
            torch.autograd.grad([o for o, _ in live], targets, [gg for _, gg in live], allow_unused=True)
            if live and targets else [None] * len(targets)
        )  # fmt: skip
    return tuple(next(second) if ctx.needs_input_grad[i] else None for i in range(4)) + (None,)


register_autograd("pydrobert_amd::concat_score", _concat_backward, setup_context=_concat_setup_context)
register_autograd(
    "pydrobert_amd::concat_score_backward", _concat_backward_backward, setup_context=_concat_backward_setup_context
)


def concat_score(wq: torch.Tensor, wk: torch.Tensor, v: torch.Tensor, dim: int) -> torch.Tensor:
    """The fused additive score of ROCm tensors (``pydrobert_amd::concat_score``)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(wq, wk, v):
            return _concat_score_op._init_fn(wq, wk, v, dim)
    return torch.ops.pydrobert_amd.concat_score(wq, wk, v, dim)


def _concat_hip_route(wq: torch.Tensor, wk: torch.Tensor, v: torch.Tensor, dim: int) -> bool:
    """True when the kernels compute what the torch body does: float32 / float64 tensors of one dtype on one ROCm
    device, a non-negative ``dim`` along which ``wq`` has size 1, and at most eight row dims."""
    dt = wq.dtype
    if dt != torch.float32 and dt != torch.float64:
        return False
    if not wq.is_cuda or wk.device != wq.device or v.device != wq.device or wk.dtype != dt or v.dtype != dt:
        return False
    n = wk.dim() - 1
    if wq.dim() != wk.dim() or dim < 0 or dim > n - 1 or wq.size(dim) != 1:
        return False
    if v.dim() != 1 or wq.size(-1) != v.size(0) or wk.size(-1) != v.size(0):
        return False
    rows = 0
    for i in range(n):
        if i != dim and (wq.size(i) != 1 or wk.size(i) != 1):
            rows += 1
    return rows <= 8  # (PDT_ATTN_MAX_DIMS)


# ----------------------------------------------------------------------------------------------------------
# modules

class GlobalSoftAttention(torch.nn.Module, metaclass=abc.ABCMeta):
    r"""Parent class for soft attention over a whole input sequence (reference _attn.py:26-226)

    ``e = score(query, key)`` is computed by the subclass; the output is the sum over ``dim`` of
    ``softmax(e masked to -inf where mask is False, dim)[..., None] * value``.

    Parameters
    ----------
    query_size
        The size of the last dimension of `query`.
    key_size
        The size of the last dimension of `key`.
    dim
        The sequence dimension of `key`.

    Call Parameters
    ---------------
    query : torch.Tensor
        ``(A*, query_size)``; ``(A*)`` broadcasts with ``(B*, C*)``.
    key : torch.Tensor
        ``(B*, T, C*, key_size)``.
    value : torch.Tensor
        ``(B*, T, C*, D*)``.
    mask : Optional[torch.Tensor]
        Boolean ``(B*, T, C*)``; :obj:`False` frames are excluded.

    Returns
    -------
    out : torch.Tensor
        ``(E*, D*)``, ``(E*)`` the broadcast of ``(A*)`` with ``(B*, C*)``.  A row whose mask is all
        :obj:`False` is NaN; ``T = 0`` gives zeros.
    """

    __constants__ = ["query_size", "key_size", "dim"]

    query_size: int
    key_size: int
    dim: int
    _fused: torch.jit.Final[bool]

    def __init__(self, query_size: int, key_size: int, dim: int = 0):
        query_size = argcheck.is_posi(query_size, name="query_size")
        key_size = argcheck.is_posi(key_size, name="key_size")
        dim = argcheck.is_int(dim, name="dim")
        super().__init__()
        self.query_size, self.key_size, self.dim = query_size, key_size, dim
        # the fused route serves the two dot-product scores as written here, not a subclass's own score
        score = type(self).score
        self._fused = score is DotProductSoftAttention.score or score is GeneralizedDotProductSoftAttention.score

    @abc.abstractmethod
    def score(self, query: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
        """The score ``e`` of shape ``(E*, T, F*)`` from `query` ``(A*, query_size)`` and `key`
        ``(B*, T, C*, key_size)``; implemented by subclasses."""
        ...

    def check_input(
        self,
        query: torch.Tensor,
        key: torch.Tensor,
        value: torch.Tensor,
        mask: Optional[torch.Tensor] = None,
    ) -> None:
        """Raise if the input is malformed (ValueError; RuntimeError if shapes do not broadcast)"""
        _check_input(query, key, value, mask, self.query_size, self.key_size, self.dim, False)

    def _fused_query(self, query: torch.Tensor) -> Tuple[torch.Tensor, float]:
        return query, 1.0

    def forward(
        self,
        query: torch.Tensor,
        key: torch.Tensor,
        value: torch.Tensor,
        mask: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        self.check_input(query, key, value, mask)
        return self._attend(query, key, value, mask)

    def _attend(
        self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask: Optional[torch.Tensor]
    ) -> torch.Tensor:
        if self._fused:
            e_shape = _bshape(list(query.unsqueeze(self.dim).shape[:-1]), list(key.shape[:-1]))
            if _hip_route(e_shape, value, mask, self.dim, [query, key, value], key.shape[-1] + value.shape[-1]):
                q, scale = self._fused_query(query)
                return dot_attention(q, key, value, mask, self.dim, scale)
        e = self.score(query, key)
        if _hip_route(list(e.shape), value, mask, self.dim, [e, value], value.shape[-1]):
            return attention_pool(e, value, mask, self.dim)
        return _softmax_pool(e, value, mask, self.dim)

    def extra_repr(self) -> str:
        return "query_size={}, key_size={}, dim={}".format(self.query_size, self.key_size, self.dim)

    def reset_parameters(self) -> None:
        pass


class DotProductSoftAttention(GlobalSoftAttention):
    r"""Global soft attention with the dot-product score (reference _attn.py:229-283)

    ``e = scale_factor * sum_i query_i key_i`` over the last dimension of `query` and `key`.

    Parameters
    ----------
    size
        The size of the last dimension of both `query` and `key`.
    dim
    scale_factor
        Multiplies every score; ``1 / sqrt(size)`` gives scaled dot-product attention.
    """

    __constants__ = "query_size", "key_size", "dim", "scale_factor"

    scale_factor: float

    def __init__(self, size: int, dim: int = 0, scale_factor: float = 1.0):
        scale_factor = argcheck.is_float(scale_factor, name="scale_factor")
        super().__init__(size, size, dim)
        self.scale_factor = scale_factor

    def score(self, query: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
        query = query.unsqueeze(self.dim)
        return (query * key).sum(-1) * self.scale_factor

    def _fused_query(self, query: torch.Tensor) -> Tuple[torch.Tensor, float]:
        return query, self.scale_factor

    def extra_repr(self) -> str:
        return super().extra_repr() + f", scale_factor={self.scale_factor}"


class GeneralizedDotProductSoftAttention(GlobalSoftAttention):
    r"""Dot-product attention with a learned matrix between query and key (reference _attn.py:286-341)

    ``e = sum_q query_q (sum_k W_qk key_k + b_q)``.  On the fused route the query is transformed instead,
    ``(query W) . key``, and ``query . b`` -- constant along `dim` -- is dropped; `bias` stays in the graph
    with a zero gradient (the reference's is zero up to rounding).

    Parameters
    ----------
    query_size
    key_size
    dim
    bias
        Whether to add a bias term ``b``: ``W key + b``.
    """

    def __init__(self, query_size: int, key_size: int, dim: int = 0, bias: bool = False):
        bias = argcheck.is_bool(bias, "bias")
        super().__init__(query_size, key_size, dim)
        self.weight = torch.nn.parameter.Parameter(torch.empty(query_size, key_size))
        if bias:
            self.bias = torch.nn.parameter.Parameter(torch.empty(query_size))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def score(self, query: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
        Wkey = torch.nn.functional.linear(key, self.weight, self.bias)
        query = query.unsqueeze(self.dim)
        return (query * Wkey).sum(-1)

    def _fused_query(self, query: torch.Tensor) -> Tuple[torch.Tensor, float]:
        q = torch.matmul(query, self.weight)
        bias = self.bias
        if bias is not None:
            q = q + bias.sum() * 0.0  # (q . b cancels in the softmax: b's gradient is 0)
        return q, 1.0

    reset_parameters = torch.jit.unused(torch.nn.Linear.reset_parameters)


def _concat_score_torch(wq: torch.Tensor, wk: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """v . tanh(wq + wk) in torch, at the full broadcast shape times the hidden size: CPU tensors, other dtypes."""
    return torch.nn.functional.linear(torch.tanh(wq + wk), v.unsqueeze(0), None).squeeze(-1)


def _concat_score(
    query: torch.Tensor, key: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], v: torch.Tensor,
    dim: int,
) -> torch.Tensor:  # fmt: skip
    """v . tanh(W [query, key] + b) with the query and key halves of W applied before broadcasting, so no
    expanded concatenation is built (the reference's _attn.py:344-361 expands both); on ROCm tensors the sum
    over the hidden units runs in ``pydrobert_amd::concat_score`` and no hidden-sized tensor is built either."""
    Dq = query.size(-1)
    wq = torch.nn.functional.linear(query.unsqueeze(dim), weight[:, :Dq], bias)
    wk = torch.nn.functional.linear(key, weight[:, Dq:], None)
    if _concat_hip_route(wq, wk, v, dim):
        return concat_score(wq, wk, v, dim)
    return _concat_score_torch(wq, wk, v)


class ConcatSoftAttention(GlobalSoftAttention):
    r"""Attention whose score is an MLP of the concatenated query and key (reference _attn.py:365-441)

    ``e = sum_i v_i tanh(sum_c W_ic [query, key]_c + b_i)``, ``W`` of shape ``(hidden_size, query_size +
    key_size)`` and ``v`` of shape ``(hidden_size,)``.

    Parameters
    ----------
    query_size
    key_size
    dim
    bias
        Whether to add the bias term ``b``.
    hidden_size
    """

    def __init__(self, query_size: int, key_size: int, dim: int = 0, bias: bool = False, hidden_size: int = 1000):
        hidden_size = argcheck.is_posi(hidden_size, name="hidden_size")
        bias = argcheck.is_bool(bias, name="bias")
        super().__init__(query_size, key_size, dim)
        self.weight = torch.nn.parameter.Parameter(torch.empty(hidden_size, query_size + key_size))
        if bias:
            self.bias = torch.nn.parameter.Parameter(torch.empty(hidden_size))
        else:
            self.register_parameter("bias", None)
        self.v = torch.nn.parameter.Parameter(torch.empty(hidden_size))
        self.reset_parameters()

    def score(self, query: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
        return _concat_score(query, key, self.weight, self.bias, self.v, self.dim)

    def reset_parameters(self) -> None:
        torch.nn.Linear.reset_parameters(self)
        torch.nn.init.normal_(self.v)

    def extra_repr(self) -> str:
        return super().extra_repr() + f", hidden_size={self.v.size(0)}"


def _unflatten(x: torch.Tensor, dim: int, shape: List[int]) -> torch.Tensor:
    ndim = x.dim()
    dim = (dim + ndim) % ndim
    full = list(x.shape)
    return x.view(full[:dim] + shape + full[dim + 1:])


class MultiHeadedAttention(GlobalSoftAttention):
    r"""Attention over several heads, concatenated and projected (reference _attn.py:444-603)

    ``head_h = single_head_attention(W^Q_h query, W^K_h key, W^V_h value, mask)``, the heads concatenated on
    the last dimension and projected by ``W^C``.  The head axis is one more broadcast dimension of the single
    head's call, so it takes that module's route.

    Quirk kept from the reference: ``WK`` and ``WV`` take their bias flag from `bias_WQ`, not from `bias_WK`
    and `bias_WV` (state dicts depend on it).

    Parameters
    ----------
    query_size
    key_size
    value_size
    num_heads
    single_head_attention
        The :class:`GlobalSoftAttention` of one head; its ``dim`` (which must not be negative),
        ``query_size`` and ``key_size`` give the sequence dimension and the head sizes.
    out_size
        Defaults to `value_size`.
    d_v
        Defaults to ``max(1, value_size // num_heads)``.
    bias_WQ
    bias_WK
    bias_WV
    bias_WC
    """

    __constants__ = ("query_size", "key_size", "dim", "value_size", "num_heads", "out_size", "d_v")

    value_size: int
    num_heads: int
    out_size: int
    d_v: int

    def __init__(
        self,
        query_size: int,
        key_size: int,
        value_size: int,
        num_heads: int,
        single_head_attention: GlobalSoftAttention,
        out_size: Optional[int] = None,
        d_v: Optional[int] = None,
        bias_WQ: bool = False,
        bias_WK: bool = False,
        bias_WV: bool = False,
        bias_WC: bool = False,
    ):
        value_size = argcheck.is_posi(value_size, "value_size")
        out_size = value_size if out_size is None else argcheck.is_posi(out_size, "out_size")
        num_heads = argcheck.is_posi(num_heads, "num_heads")
        if single_head_attention.dim < 0:
            raise ValueError("Negative dimensions are ambiguous for multi-headed attention")
        d_v = max(1, value_size // num_heads) if d_v is None else argcheck.is_posi(d_v, "d_v")
        bias_WQ = argcheck.is_bool(bias_WQ, "bias_WQ")
        bias_WK = argcheck.is_bool(bias_WQ, "bias_WK")  # (sic: the reference's quirk)
        bias_WV = argcheck.is_bool(bias_WQ, "bias_WV")  # (sic)
        bias_WC = argcheck.is_bool(bias_WC, "bias_WC")
        super().__init__(query_size, key_size, dim=single_head_attention.dim)
        self.value_size, self.out_size, self.num_heads = value_size, out_size, num_heads
        self.single_head_attention = single_head_attention
        self.d_q = single_head_attention.query_size
        self.d_k = single_head_attention.key_size
        self.d_v = d_v
        self.WQ = torch.nn.Linear(query_size, num_heads * self.d_q, bias=bias_WQ)
        self.WK = torch.nn.Linear(key_size, num_heads * self.d_k, bias=bias_WK)
        self.WV = torch.nn.Linear(value_size, num_heads * d_v, bias=bias_WV)
        self.WC = torch.nn.Linear(d_v * num_heads, out_size, bias=bias_WC)
        single_head_attention.reset_parameters()

    def check_input(
        self,
        query: torch.Tensor,
        key: torch.Tensor,
        value: torch.Tensor,
        mask: Optional[torch.Tensor] = None,
    ) -> None:
        """Raise RuntimeError if the input is malformed"""
        _check_input(query, key, value, mask, self.query_size, self.key_size, self.dim, True)
        if value.size(-1) != self.value_size:
            raise RuntimeError("Last dimension of value must match value_size")

    @torch.jit.unused
    def score(self, query: torch.Tensor, key: torch.Tensor) -> None:
        raise NotImplementedError("In MultiHeadedAttention, score() is handled by single_head_attention")

    def forward(
        self,
        query: torch.Tensor,
        key: torch.Tensor,
        value: torch.Tensor,
        mask: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        if not torch.jit.is_scripting():
            self.check_input(query, key, value, mask)
        query_heads = _unflatten(self.WQ(query), -1, [self.num_heads, self.d_q])
        key_heads = _unflatten(self.WK(key), -1, [self.num_heads, self.d_k])
        value_heads = _unflatten(self.WV(value), -1, [self.num_heads, self.d_v])
        if mask is not None:
            mask = mask.unsqueeze(-2)
        cat = self.single_head_attention(query_heads, key_heads, value_heads, mask)
        return self.WC(cat.flatten(-2))

    def reset_parameters(self) -> None:
        self.WQ.reset_parameters()
        self.WK.reset_parameters()
        self.WV.reset_parameters()
        self.WC.reset_parameters()
        self.single_head_attention.reset_parameters()

    def extra_repr(self) -> str:
        s = super().extra_repr()
        s += ", value_size={}, out_size={}, num_heads={}".format(self.value_size, self.out_size, self.num_heads)
        return s
