"""CTC greedy search and the joint log-probability of token sequences on MI355X
(``csrc/seq_ops.hip``): ``ctc_greedy_search``, ``sequence_log_probs`` and their Modules.
"""
import math
from typing import Any, Optional, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck
from ._step import _i64, _logits_elem

__all__ = ["CTCGreedySearch", "SequenceLogProbabilities", "ctc_greedy_search", "sequence_log_probs"]


@custom_op("pydrobert_amd::ctc_greedy_search", mutates_args=())
def _ctc_greedy_search_op(
    logits: torch.Tensor,
    in_lens: Optional[torch.Tensor],
    blank_idx: int,
    batch_first: bool,
    is_probs: bool,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if logits.dim() != 3:
        raise RuntimeError("logits must be 3-dimensional")
    V = logits.size(2)
    if blank_idx < -V or blank_idx > (V - 1):
        raise RuntimeError(
            "Blank index out of range (expected to be in the range of [-{},{}], but got {})".format(
                V, V - 1, blank_idx
            )
        )
    blank_idx = (blank_idx + V) % V
    device = _cabi.require_hip(logits, in_lens)
    x, elem = _logits_elem(logits)  # (float16 / bfloat16: read as they are, no float32 copy)
    if batch_first:
        N, T = x.shape[:2]
        st, sn = x.stride(1), x.stride(0)
    else:
        T, N = x.shape[:2]
        st, sn = x.stride(0), x.stride(1)
    lens = None if in_lens is None else _i64(in_lens).contiguous()
    with torch.cuda.device(device):
        max_ = torch.empty((N,), device=device, dtype=torch.float)
        paths = torch.empty((N, T) if batch_first else (T, N), device=device, dtype=torch.long)
        out_lens = torch.empty((N,), device=device, dtype=torch.long)
        pst, psn = (paths.stride(1), paths.stride(0)) if batch_first else (paths.stride(0), paths.stride(1))
        args = (
            _cabi.ptr(x), T, N, V, st, sn, x.stride(2), _cabi.ptr(lens), blank_idx, int(is_probs),
            _cabi.ptr(max_), _cabi.ptr(paths), pst, psn, _cabi.ptr(out_lens), _cabi.stream_ptr(device),
        )  # fmt: skip
        L = _cabi.lib()
        rc = L.pdt_ctc_greedy_search_elem(*args, elem) if elem else L.pdt_ctc_greedy_search(*args)
    _cabi.check(rc, "pdt_ctc_greedy_search")
    return max_.to(logits.dtype), paths, out_lens


@_ctc_greedy_search_op.register_fake
def _(logits, in_lens, blank_idx, batch_first, is_probs):
    N = logits.shape[0] if batch_first else logits.shape[1]
    return (
        logits.new_empty((N,)),
        logits.new_empty(logits.shape[:2], dtype=torch.long),
        logits.new_empty((N,), dtype=torch.long),
    )


def _ctc_greedy_setup(ctx, inputs, output):
    logits, in_lens, _, batch_first, is_probs = inputs
    ctx.save_for_backward(logits, in_lens)
    ctx.cfg = (batch_first, is_probs)


def _ctc_greedy_backward(ctx, g_max, g_paths, g_lens):
    """``max_`` is the sum (product) over the valid frames of the best class's log-probability
    (probability): differentiable in the reference (_decoding.py:526-553).  The frames' maxima
    are recomputed with device ops and differentiated by autograd."""
    logits, in_lens = ctx.saved_tensors
    batch_first, is_probs = ctx.cfg
    with torch.enable_grad():
        x = logits.detach().requires_grad_(True)
        y = x if is_probs else x.log_softmax(2)
        if not batch_first:
            y = y.transpose(0, 1)
        best = y.max(2)[0]  # (N, T)
        if in_lens is not None:
            valid = torch.arange(best.size(1), device=best.device).unsqueeze(0) < in_lens.unsqueeze(1)
            best = best.masked_fill(~valid, 1.0 if is_probs else 0.0)
        total = best.prod(1) if is_probs else best.sum(1)
        (g,) = torch.autograd.grad(total, x, g_max.to(total.dtype))
    return g, None, None, None, None


register_autograd("pydrobert_amd::ctc_greedy_search", _ctc_greedy_backward, setup_context=_ctc_greedy_setup)


def ctc_greedy_search(
    logits: torch.Tensor,
    in_lens: Optional[torch.Tensor] = None,
    blank_idx: int = -1,
    batch_first: bool = False,
    is_probs: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Functional version of :class:`CTCGreedySearch` (reference _decoding.py:507-558):
    returns ``(max_, paths, out_lens)``.  One pass over the logits."""
    return torch.ops.pydrobert_amd.ctc_greedy_search(logits, in_lens, blank_idx, batch_first, is_probs)


def _slp_dims(hyp: torch.Tensor, dim: int) -> Tuple[int, int, int, int]:
    hyp_dim = hyp.dim()
    if dim < -hyp_dim or dim > hyp_dim - 1:
        raise RuntimeError(
            "Dimension out of range (expected to be in range of [{}, {}], but got {})".format(
                -hyp_dim, hyp_dim - 1, dim
            )
        )
    dim = (hyp_dim + dim) % hyp_dim
    shape = tuple(hyp.shape)
    return dim, int(math.prod(shape[:dim])), shape[dim], int(math.prod(shape[dim + 1 :]))


@custom_op("pydrobert_amd::sequence_log_probs", mutates_args=())
def _sequence_log_probs_op(
    logits: torch.Tensor, hyp: torch.Tensor, dim: int, eos: Optional[int]
) -> torch.Tensor:
    """Fused log-softmax + gather + masked sum over ``dim`` (csrc/seq_ops.hip)."""
    dim, A, S, B = _slp_dims(hyp, dim)
    if logits.shape[:-1] != hyp.shape:
        raise RuntimeError("logits must have shape hyp.shape + (num_classes,)")
    device = _cabi.require_hip(logits, hyp)
    x, elem = _logits_elem(logits)
    x = x.contiguous()  # (in its own dtype)
    h = _i64(hyp).contiguous()
    with torch.cuda.device(device):
        out = torch.empty((A, B), device=device, dtype=torch.float)
        args = (
            _cabi.ptr(x), _cabi.ptr(h), A, S, B, x.shape[-1], int(eos is not None),
            int(eos) if eos is not None else 0, _cabi.ptr(out), _cabi.stream_ptr(device),
        )  # fmt: skip
        L = _cabi.lib()
        rc = L.pdt_sequence_log_probs_forward_elem(*args, elem) if elem else L.pdt_sequence_log_probs_forward(*args)
    _cabi.check(rc, "pdt_sequence_log_probs_forward")
    shape = tuple(hyp.shape)
    return out.view(shape[:dim] + shape[dim + 1 :]).to(logits.dtype)


@_sequence_log_probs_op.register_fake
def _(logits, hyp, dim, eos):
    d = dim % hyp.dim()
    return logits.new_empty(tuple(hyp.shape[:d]) + tuple(hyp.shape[d + 1 :]))


@custom_op("pydrobert_amd::sequence_log_probs_backward", mutates_args=())
def _sequence_log_probs_backward_op(
    logits: torch.Tensor, hyp: torch.Tensor, dim: int, eos: Optional[int], grad_out: torch.Tensor
) -> torch.Tensor:
    dim, A, S, B = _slp_dims(hyp, dim)
    device = logits.device
    x, elem = _logits_elem(logits)
    x = x.contiguous()
    h = _i64(hyp).contiguous()
    g = grad_out.detach().float().contiguous()
    with torch.cuda.device(device):
        grad = torch.empty_like(x)  # (the logits' dtype: the kernel rounds each element as .to(dtype) would)
        args = (
            _cabi.ptr(x), _cabi.ptr(h), A, S, B, x.shape[-1], int(eos is not None),
            int(eos) if eos is not None else 0, _cabi.ptr(g), _cabi.ptr(grad),
            _cabi.stream_ptr(device),
        )  # fmt: skip
        L = _cabi.lib()
        rc = L.pdt_sequence_log_probs_backward_elem(*args, elem) if elem else L.pdt_sequence_log_probs_backward(*args)
    _cabi.check(rc, "pdt_sequence_log_probs_backward")
    return grad.view(logits.shape).to(logits.dtype)


@_sequence_log_probs_backward_op.register_fake
def _(logits, hyp, dim, eos, grad_out):
    return torch.empty_like(logits)


def _slp_setup_context(ctx, inputs, output):
    logits, hyp, dim, eos = inputs
    ctx.save_for_backward(logits, hyp)
    ctx.cfg = (dim, eos)


def _slp_backward(ctx, grad_out):
    logits, hyp = ctx.saved_tensors
    dim, eos = ctx.cfg
    grad = torch.ops.pydrobert_amd.sequence_log_probs_backward(logits, hyp, dim, eos, grad_out)
    return grad, None, None, None


register_autograd(
    "pydrobert_amd::sequence_log_probs", _slp_backward, setup_context=_slp_setup_context
)


def _sequence_log_probs_ps(
    logits: Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]],
    hyp: torch.Tensor,
    dim: int,
) -> torch.Tensor:
    # padded view + out-of-range tokens beyond each length: same kernel, same masking rule
    if dim < -2 or dim > 1:
        raise RuntimeError(
            "Dimension out of range (expected to be in range of [-2, 1], but got {})".format(dim)
        )
    data, batch_sizes, unsorted = logits[0], logits[1], logits[3]
    S = batch_sizes.size(0)
    padded, lens = torch._pad_packed_sequence(data, batch_sizes, False, 0.0, S)  # (S, N, V)
    if unsorted is not None:
        padded, lens = padded.index_select(1, unsorted), lens.index_select(0, unsorted.cpu())
    h = hyp if dim % 2 == 0 else hyp.t()
    h = h[:S]
    beyond = torch.arange(S, device=h.device).unsqueeze(1) >= lens.to(h.device).unsqueeze(0)
    return torch.ops.pydrobert_amd.sequence_log_probs(padded, h.masked_fill(beyond, -1), 0, None)


def sequence_log_probs(
    logits: Any, hyp: torch.Tensor, dim: int = 0, eos: Optional[int] = None
) -> torch.Tensor:
    """Functional version of :class:`SequenceLogProbabilities` (reference
    _decoding.py:1516-1633): joint log-probability of the token sequences ``hyp`` under
    ``logits`` (a tensor of shape ``hyp.shape + (V,)`` or a ``PackedSequence``).  Fused
    log-softmax + gather + masked sum; differentiable w.r.t. ``logits``."""
    if isinstance(logits, torch.Tensor):
        return torch.ops.pydrobert_amd.sequence_log_probs(logits, hyp, dim, eos)
    elif torch.jit.isinstance(
        logits, Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]
    ):
        return _sequence_log_probs_ps(logits, hyp, dim)
    raise RuntimeError("logits must be either a Tensor or PackedSequence")


class CTCGreedySearch(torch.nn.Module):
    """CTC greedy search (reference _decoding.py:561-635)."""

    __constants__ = "blank_idx", "batch_first", "is_probs"

    def __init__(self, blank_idx: int = -1, batch_first: bool = False, is_probs: bool = False):
        blank_idx = argcheck.is_int(blank_idx, "blank_idx")
        batch_first = argcheck.is_bool(batch_first, "batch_first")
        is_probs = argcheck.is_bool(is_probs, "is_probs")
        super().__init__()
        self.blank_idx, self.batch_first, self.is_probs = blank_idx, batch_first, is_probs

    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)

    def forward(
        self, logits: torch.Tensor, in_lens: Optional[torch.Tensor] = None
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return ctc_greedy_search(logits, in_lens, self.blank_idx, self.batch_first, self.is_probs)


class SequenceLogProbabilities(torch.nn.Module):
    """Calculate joint log probability of sequences (reference _decoding.py:1636-1720)."""

    __constants__ = "dim", "eos"

    def __init__(self, dim: int = 0, eos: Optional[int] = None):
        dim = argcheck.is_int(dim, "dim")
        eos = argcheck.is_int(eos, "eos", True)
        super().__init__()
        self.dim, self.eos = dim, eos

    def extra_repr(self) -> str:
        s = "dim={}".format(self.dim)
        if self.eos is not None:
            s += ", eos={}".format(self.eos)
        return s

    def forward(self, logits: Any, hyp: torch.Tensor) -> torch.Tensor:
        return sequence_log_probs(logits, hyp, self.dim, self.eos)
