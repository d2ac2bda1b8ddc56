"""Variable-length padding on MI355X (reference _pad.py:108-149, Module :152-238); the
movement behind :class:`RandomShift`.  One HIP pass (``csrc/pad_variable.hip``) instead of
the reference's masks + masked_scatter chain.

``pad_masked_sequence`` and ``chunk_by_slices`` (reference _pad.py:257-548) run on the row
compaction and the indexed copy of ``csrc/seq_chunk.hip``; CPU tensors (data-loader workers)
take a torch body written from the same rules."""
from typing import Optional, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck, config

__all__ = ["ChunkBySlices", "PadMaskedSequence", "PadVariable", "chunk_by_slices", "pad_masked_sequence", "pad_variable"]

_PAD_MODES = {"constant": 0, "reflect": 1, "replicate": 2}


@custom_op("pydrobert_amd::pad_variable", mutates_args=())
def _pad_variable_op(
    x: torch.Tensor, lens: torch.Tensor, pad: torch.Tensor, mode: str, value: float
) -> torch.Tensor:
    if x.dim() < 2:
        raise ValueError("Expected x to be at least two dimensional")
    shape = x.shape
    N, T = shape[0], shape[1]
    if lens.shape != (N,):
        raise ValueError(
            "For x of shape {}, lens should have shape ({},) but got {}".format(tuple(shape), N, tuple(lens.shape))
        )
    if pad.shape != (2, N):
        raise ValueError(
            "For x of shape {}, pad should have shape (2, {}), but got {}".format(tuple(shape), N, tuple(pad.shape))
        )
    if mode not in _PAD_MODES:
        raise ValueError("mode must be one of 'constant', 'reflect', 'replicate', got '{}'".format(mode))
    device = _cabi.require_hip(x, lens, pad)
    xc = x.detach().contiguous()
    ln = lens.detach().long().contiguous()
    pd = pad.detach().long().contiguous()
    F = 1
    for d in shape[2:]:
        F *= d
    with torch.cuda.device(device):
        # one read-back, like the reference's new_lens.max().item() (:128); the same trip
        # carries the two data checks of _get_padding_buffers (:52-56, :82-83)
        new_lens = ln + pd.sum(0)
        stats = torch.stack([
            new_lens.max() if N else ln.new_zeros(()),
            ((pd >= ln.unsqueeze(0)).any() if N else ln.new_zeros((), dtype=torch.bool)).long(),
            ((ln < 1).any() if N else ln.new_zeros((), dtype=torch.bool)).long(),
        ]).tolist()  # fmt: skip
        Tp, pad_ge_len, len_lt_1 = int(stats[0]), bool(stats[1]), bool(stats[2])
        if mode == "reflect" and pad_ge_len:
            raise NotImplementedError(
                "For reflect padding, all padding lengths must be less than the sequence length"
            )
        if mode == "replicate" and len_lt_1:
            raise RuntimeError("For replicate padding, all lens must be > 0")
        out = torch.empty((N, Tp) + tuple(shape[2:]), device=device, dtype=x.dtype)
        fill = torch.full((1,), value, device=device, dtype=x.dtype)
        rc = _cabi.lib().pdt_pad_variable(
            _cabi.ptr(xc) if xc.numel() else None, N, T, F, xc.element_size(), _cabi.ptr(ln),
            _cabi.ptr(pd), _PAD_MODES[mode], _cabi.ptr(fill), Tp,
            _cabi.ptr(out) if out.numel() else None, _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_pad_variable")
    return out


@_pad_variable_op.register_fake
def _(x, lens, pad, mode, value):
    Tp = torch.library.get_ctx().new_dynamic_size()
    return x.new_empty((x.shape[0], Tp) + tuple(x.shape[2:]))


@custom_op("pydrobert_amd::pad_variable_backward", mutates_args=())
def _pad_variable_backward_op(
    grad_out: torch.Tensor, lens: torch.Tensor, pad: torch.Tensor, mode: str, T: int
) -> torch.Tensor:
    device = _cabi.require_hip(grad_out, lens, pad)
    ct = torch.float64 if grad_out.dtype == torch.float64 else torch.float32
    g = grad_out.detach().to(ct).contiguous()
    N, Tp = g.shape[0], g.shape[1]
    F = 1
    for d in g.shape[2:]:
        F *= d
    ln, pd = lens.detach().long().contiguous(), pad.detach().long().contiguous()
    with torch.cuda.device(device):
        grad = torch.empty((N, T) + tuple(g.shape[2:]), device=device, dtype=ct)
        rc = _cabi.lib().pdt_pad_variable_backward(
            _cabi.ptr(g) if g.numel() else None, int(ct == torch.float64), N, T, F, _cabi.ptr(ln), _cabi.ptr(pd),
            _PAD_MODES[mode], Tp, _cabi.ptr(grad) if grad.numel() else None, _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_pad_variable_backward")
    return grad.to(grad_out.dtype)


@_pad_variable_backward_op.register_fake
def _(grad_out, lens, pad, mode, T):
    return grad_out.new_empty((grad_out.shape[0], T) + tuple(grad_out.shape[2:]))


def _pad_setup_context(ctx, inputs, output):
    x, lens, pad, mode, _ = inputs
    ctx.save_for_backward(lens, pad)
    ctx.cfg = (mode, x.shape[1])


def _pad_backward(ctx, grad_out):
    lens, pad = ctx.saved_tensors
    mode, T = ctx.cfg
    g = torch.ops.pydrobert_amd.pad_variable_backward(grad_out, lens, pad, mode, T)
    return g, None, None, None, None


register_autograd("pydrobert_amd::pad_variable", _pad_backward, setup_context=_pad_setup_context)


def pad_variable(
    x: torch.Tensor,
    lens: torch.Tensor,
    pad: torch.Tensor,
    mode: str = "constant",
    value: float = config.DEFT_PAD_VALUE,
) -> torch.Tensor:
    """Functional version of :class:`PadVariable` (reference _pad.py:108-149)."""
    return torch.ops.pydrobert_amd.pad_variable(x, lens, pad, mode, value)


class PadVariable(torch.nn.Module):
    """Pad variable-length input by a variable amount on each side (reference _pad.py:152-238)."""

    __constants__ = ("mode", "value")

    def __init__(self, mode: str = "constant", value: float = config.DEFT_PAD_VALUE):
        mode = argcheck.is_in(mode, tuple(_PAD_MODES), "mode")
        value = argcheck.is_float(value, "value")
        super().__init__()
        self.mode, self.value = mode, value

    def extra_repr(self) -> str:
        s = "mode={}".format(self.mode)
        if self.mode == "constant":
            s += ", value={}".format(self.value)
        return s

    def forward(self, x: torch.Tensor, lens: torch.Tensor, pad: torch.Tensor) -> torch.Tensor:
        return pad_variable(x, lens, pad, self.mode, self.value)


# ----------------------------------------------------------------------------------------------------------
# pad_masked_sequence / chunk_by_slices (csrc/seq_chunk.hip)


def _fill_like(x: torch.Tensor, value: float) -> torch.Tensor:
    return torch.full((1,), value, device=x.device, dtype=x.dtype)


def _rows(x: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """x with its trailing dims (2 ..) dense -- a copy only if they are not -- and their size F; the first
    two dims keep whatever strides they have (the kernels take them)."""
    F, dense = 1, True
    for d in range(x.dim() - 1, 1, -1):
        if x.shape[d] != 1 and x.stride(d) != F:
            dense = False
        F *= x.shape[d]
    return (x if dense else x.contiguous()), F


def _words(xc: torch.Tensor, F: int, s0: int, s1: int, out: torch.Tensor, value: float):
    """(word bytes, F, the two strides, the fill) as the copy kernels take them: in 16-byte words when
    every row of F elements, both strides and both pointers are multiples of 16 bytes (one access moves
    16 bytes per lane), else in elements."""
    es = xc.element_size()
    k = 16 // es
    if F % k == 0 and s0 % k == 0 and s1 % k == 0 and xc.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0:
        return 16, F // k, s0 // k, s1 // k, torch.full((k,), value, device=xc.device, dtype=xc.dtype)
    return es, F, s0, s1, _fill_like(xc, value)


def _pad_masked_checks(x: torch.Tensor, mask: torch.Tensor) -> None:
    if x.dim() < 2:
        raise RuntimeError("expected x to be at least two-dimensional, got {}".format(x.dim()))
    if mask.dim() != 2:
        raise RuntimeError("expected mask to be two-dimensional, got {}".format(mask.dim()))
    if mask.dtype != torch.bool:
        raise RuntimeError("expected mask to be a bool tensor, got {}".format(mask.dtype))
    if tuple(mask.shape) != tuple(x.shape[:2]):
        raise RuntimeError(
            "expected mask to have shape {}, got {}".format(tuple(x.shape[:2]), tuple(mask.shape))
        )


def _pad_masked_torch(x, mask, batch_first, padding_value):
    """Torch body (CPU tensors, and the device restatement the timing tool compares with): a stable sort
    of the dropped flags is the left-packing order."""
    if not batch_first:
        x, mask = x.transpose(0, 1), mask.transpose(0, 1)
    T = x.shape[1]
    lens = mask.sum(1)
    order = torch.argsort((~mask).to(torch.uint8), dim=1, stable=True)
    tail = torch.arange(T, device=x.device) >= lens.unsqueeze(1)
    shape = tuple(mask.shape) + (1,) * (x.dim() - 2)
    out = torch.where(tail.view(shape), _fill_like(x, padding_value), x.gather(1, order.view(shape).expand_as(x)))
    if not batch_first:
        out = out.transpose(0, 1)
    return out.contiguous(), lens


def _pad_masked_adjoint_torch(grad_out, mask, batch_first):
    if not batch_first:
        grad_out, mask = grad_out.transpose(0, 1), mask.transpose(0, 1)
    rank = (mask.long().cumsum(1) - 1).clamp_min(0)
    shape = tuple(mask.shape) + (1,) * (grad_out.dim() - 2)
    g = torch.where(mask.view(shape), grad_out.gather(1, rank.view(shape).expand_as(grad_out)),
                    grad_out.new_zeros(1))  # fmt: skip
    if not batch_first:
        g = g.transpose(0, 1)
    return g.contiguous()


def _pad_masked_hip(x, mask, batch_first, value, adjoint):
    """Forward (the src map: output step j reads the j-th kept step) or adjoint (the rank map: input step
    t reads the output step it went to, zeros if dropped) -- one compaction over the mask in place, one
    indexed copy.  Returns (out, lens)."""
    device = _cabi.require_hip(x, mask)
    nd, td = (0, 1) if batch_first else (1, 0)
    N, T = x.shape[nd], x.shape[td]
    xc, F = _rows(x)
    out = torch.empty(x.shape, device=device, dtype=x.dtype)
    lens = torch.zeros((N,), device=device, dtype=torch.long)
    if N * T == 0:
        return out, lens
    index = torch.empty(x.shape[:2], device=device, dtype=torch.int32)
    lib = _cabi.lib()
    with _cabi.on_device(device):
        stream = _cabi.stream_ptr(device)
        rc = lib.pdt_compact_mask(
            _cabi.ptr(mask), N, T, mask.stride(nd), mask.stride(td), None if adjoint else _cabi.ptr(index),
            _cabi.ptr(index) if adjoint else None, index.stride(nd), index.stride(td), _cabi.ptr(lens), stream,
        )  # fmt: skip
        _cabi.check(rc, "pdt_compact_mask")
        if F:
            wb, Fw, s_n, s_t, fill = _words(xc, F, xc.stride(nd), xc.stride(td), out, value)
            rc = lib.pdt_gather_steps(
                _cabi.ptr(xc), N, T, Fw, wb, s_n, s_t, _cabi.ptr(index),
                index.stride(nd), index.stride(td), T, int(not batch_first), _cabi.ptr(fill), _cabi.ptr(out), stream,
            )  # fmt: skip
            _cabi.check(rc, "pdt_gather_steps")
    return out, lens


@custom_op("pydrobert_amd::pad_masked_sequence", mutates_args=())
def _pad_masked_sequence_op(
    x: torch.Tensor, mask: torch.Tensor, batch_first: bool, padding_value: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    _pad_masked_checks(x, mask)
    x, mask = x.detach(), mask.detach()
    if x.device.type == "cpu":
        return _pad_masked_torch(x, mask, batch_first, padding_value)
    return _pad_masked_hip(x, mask, batch_first, padding_value, False)


@_pad_masked_sequence_op.register_fake
def _(x, mask, batch_first, padding_value):
    return x.new_empty(x.shape), mask.new_empty((x.shape[0 if batch_first else 1],), dtype=torch.long)


@custom_op("pydrobert_amd::pad_masked_sequence_backward", mutates_args=())
def _pad_masked_sequence_backward_op(grad_out: torch.Tensor, mask: torch.Tensor, batch_first: bool) -> torch.Tensor:
    # the ranks are recomputed from the mask (one byte per step) rather than saved
    grad_out, mask = grad_out.detach(), mask.detach()
    if grad_out.device.type == "cpu":
        return _pad_masked_adjoint_torch(grad_out, mask, batch_first)
    return _pad_masked_hip(grad_out, mask, batch_first, 0.0, True)[0]


@_pad_masked_sequence_backward_op.register_fake
def _(grad_out, mask, batch_first):
    return grad_out.new_empty(grad_out.shape)


def _pad_masked_setup_context(ctx, inputs, output):
    _, mask, batch_first, _ = inputs
    ctx.save_for_backward(mask)
    ctx.batch_first = batch_first


def _pad_masked_backward(ctx, grad_out, grad_lens):
    (mask,) = ctx.saved_tensors
    g = torch.ops.pydrobert_amd.pad_masked_sequence_backward(grad_out, mask, ctx.batch_first)
    return g, None, None, None


register_autograd(
    "pydrobert_amd::pad_masked_sequence", _pad_masked_backward, setup_context=_pad_masked_setup_context
)


def pad_masked_sequence(
    x: torch.Tensor,
    mask: torch.Tensor,
    batch_first: bool = False,
    padding_value: float = config.DEFT_PAD_VALUE,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Functional version of :class:`PadMaskedSequence` (reference _pad.py:257-279)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(x, mask):
            return _pad_masked_sequence_op._init_fn(x, mask, batch_first, padding_value)
    return torch.ops.pydrobert_amd.pad_masked_sequence(x, mask, batch_first, padding_value)


class PadMaskedSequence(torch.nn.Module):
    """Keep the steps of each sequence where ``mask`` is true, left-packed, and right-pad the rest with
    ``padding_value`` (reference _pad.py:282-369).  Returns ``(x_, lens)``, ``x_`` shaped like ``x``."""

    __constants__ = ("batch_first", "padding_value")
    batch_first: bool
    padding_value: float

    def __init__(self, batch_first: bool = False, padding_value: float = config.DEFT_PAD_VALUE):
        batch_first = argcheck.is_bool(batch_first, "batch_first")
        padding_value = argcheck.is_float(padding_value, "padding_value")
        super().__init__()
        self.batch_first, self.padding_value = batch_first, padding_value

    def extra_repr(self) -> str:
        return "batch_first={}, padding_value={}".format(self.batch_first, self.padding_value)

    def forward(self, x: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return pad_masked_sequence(x, mask, self.batch_first, self.padding_value)


def _chunk_index(slices, lens, T: int, Tp: int, mode: str):
    """(source step, valid) of every chunk step, (N, Tp) each: the rule the kernel applies."""
    start, end, ln = slices[:, 0:1], slices[:, 1:2], lens.unsqueeze(1)
    t = torch.arange(Tp, device=slices.device).unsqueeze(0)
    s = start + t
    if mode == "reflect":
        s = torch.where(s < 0, -s, torch.where(s >= ln, 2 * (ln - 1) - s, s))
    elif mode == "replicate":
        s = torch.minimum(s, ln - 1).clamp_min(0)
    valid = (t < end - start) & (s >= 0) & (s < ln) & (s < T)
    return s.clamp(0, max(T - 1, 0)), valid


def _chunk_torch(x, slices, lens, mode, value, Tp):
    N, T = x.shape[0], x.shape[1]
    idx, valid = _chunk_index(slices, lens, T, Tp, mode)
    shape = (N, Tp) + (1,) * (x.dim() - 2)
    idx = idx.view(shape).expand((N, Tp) + tuple(x.shape[2:]))
    return torch.where(valid.view(shape), x.gather(1, idx), _fill_like(x, value))


def _chunk_adjoint_torch(grad_out, slices, lens, mode, T):
    N, Tp = grad_out.shape[0], grad_out.shape[1]
    idx, valid = _chunk_index(slices, lens, T, Tp, mode)
    shape = (N, Tp) + (1,) * (grad_out.dim() - 2)
    g = grad_out * valid.view(shape).to(grad_out.dtype)
    grad_x = grad_out.new_zeros((N, T) + tuple(grad_out.shape[2:]))
    return grad_x.scatter_add_(1, idx.view(shape).expand_as(g), g)


def _chunk_lens(x, lens) -> torch.Tensor:
    N, T = x.shape[0], x.shape[1]
    if lens is None:
        return torch.full((N,), T, dtype=torch.long, device=x.device)
    return lens.detach().long().contiguous()


@custom_op("pydrobert_amd::chunk_by_slices", mutates_args=())
def _chunk_by_slices_op(
    x: torch.Tensor, slices: torch.Tensor, lens: Optional[torch.Tensor], mode: str, value: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    if x.dim() < 2:
        raise RuntimeError("Expected x to be at least 2-dimensional; got {}".format(x.dim()))
    N, T = x.shape[0], x.shape[1]
    if not N * T:
        return x.new_empty(x.shape), slices.new_zeros((N,))
    if lens is not None and tuple(lens.shape) != (N,):
        raise RuntimeError("Expected lens to be of shape ({},); got {}".format(N, tuple(lens.shape)))
    if tuple(slices.shape) != (N, 2):
        raise RuntimeError("Expected slices to be of shape ({}, 2); got {}".format(N, tuple(slices.shape)))
    if mode not in _PAD_MODES:
        raise ValueError("mode must be one of 'constant', 'reflect', 'replicate', got '{}'".format(mode))
    x = x.detach()
    sl = slices.detach().long().contiguous()
    ln = _chunk_lens(x, lens) if lens is not None or x.device.type == "cpu" else None  # (None: the kernels take T)
    if x.device.type != "cpu":
        _cabi.require_hip(x, sl, ln)
    # one read-back, like the reference's Tp (:414-416); the same trip carries the two data checks of
    # _get_padding_buffers (:57, :84)
    if x.device.type == "cpu":
        # (left pad, chunk length, right pad) per row, the pads zero for an empty slice (:406-409)
        start, end = sl[:, 0], sl[:, 1]
        span = end - start
        pads = torch.stack([-start, span, end - ln]).clamp_min(0).masked_fill((span <= 0).unsqueeze(0), 0)
        stats = torch.stack([pads.max(), (pads[::2] - ln).max(), ln.min()]).tolist()
        chunk_lens = pads[1]
    else:  # the same three numbers and the chunk lengths from one small launch
        report = torch.empty((3,), dtype=torch.long, device=x.device)
        chunk_lens = torch.empty((N,), dtype=torch.long, device=x.device)
        with _cabi.on_device(x.device):
            rc = _cabi.lib().pdt_chunk_stats(
                _cabi.ptr(sl), None if lens is None else _cabi.ptr(ln), N, T, _cabi.ptr(chunk_lens),
                _cabi.ptr(report), _cabi.stream_ptr(x.device),
            )  # fmt: skip
        _cabi.check(rc, "pdt_chunk_stats")
        stats = report.tolist()
    Tp, pad_ge_len, len_lt_1 = int(stats[0]), stats[1] >= 0, stats[2] < 1
    if mode == "reflect" and pad_ge_len:
        raise NotImplementedError("For reflect padding, all padding lengths must be less than the sequence length")
    if mode == "replicate" and len_lt_1:
        raise RuntimeError("For replicate padding, all lens must be > 0")
    chunk_lens = chunk_lens.to(slices.dtype)
    if x.device.type == "cpu":
        return _chunk_torch(x, sl, ln, mode, value, Tp), chunk_lens
    device = x.device
    xc, F = _rows(x)
    out = torch.empty((N, Tp) + tuple(x.shape[2:]), device=device, dtype=x.dtype)
    if out.numel():
        wb, Fw, s_n, s_t, fill = _words(xc, F, xc.stride(0), xc.stride(1), out, value)
        with _cabi.on_device(device):
            rc = _cabi.lib().pdt_chunk_by_slices(
                _cabi.ptr(xc), N, T, Fw, wb, s_n, s_t, _cabi.ptr(sl),
                None if lens is None else _cabi.ptr(ln), _PAD_MODES[mode], _cabi.ptr(fill), Tp, _cabi.ptr(out),
                _cabi.stream_ptr(device),
            )  # fmt: skip
        _cabi.check(rc, "pdt_chunk_by_slices")
    return out, chunk_lens


@_chunk_by_slices_op.register_fake
def _(x, slices, lens, mode, value):
    N = x.shape[0]
    if isinstance(N, int) and isinstance(x.shape[1], int) and not N * x.shape[1]:
        return x.new_empty(x.shape), slices.new_empty((N,))
    Tp = torch.library.get_ctx().new_dynamic_size()
    return x.new_empty((N, Tp) + tuple(x.shape[2:])), slices.new_empty((N,))


@custom_op("pydrobert_amd::chunk_by_slices_backward", mutates_args=())
def _chunk_by_slices_backward_op(
    grad_out: torch.Tensor, slices: torch.Tensor, lens: Optional[torch.Tensor], mode: str, T: int
) -> torch.Tensor:
    g = grad_out.detach()
    sl = slices.detach().long().contiguous()
    N, Tp = g.shape[0], g.shape[1]
    if g.device.type == "cpu":
        ln = torch.full((N,), T, dtype=torch.long) if lens is None else lens.detach().long()
        return _chunk_adjoint_torch(g, sl, ln, mode, T)
    device = _cabi.require_hip(g, sl, lens)
    ct = torch.float64 if g.dtype == torch.float64 else torch.float32
    g = g.to(ct).contiguous()
    ln = None if lens is None else lens.detach().long().contiguous()
    F = 1
    for d in g.shape[2:]:
        F *= d
    grad = torch.empty((N, T) + tuple(g.shape[2:]), device=device, dtype=ct)
    if grad.numel():
        with _cabi.on_device(device):
            rc = _cabi.lib().pdt_chunk_by_slices_backward(
                _cabi.ptr(g) if g.numel() else None, int(ct == torch.float64), N, T, F, _cabi.ptr(sl), _cabi.ptr(ln),
                _PAD_MODES[mode], Tp, _cabi.ptr(grad), _cabi.stream_ptr(device),
            )  # fmt: skip
        _cabi.check(rc, "pdt_chunk_by_slices_backward")
    return grad.to(grad_out.dtype)


@_chunk_by_slices_backward_op.register_fake
def _(grad_out, slices, lens, mode, T):
    return grad_out.new_empty((grad_out.shape[0], T) + tuple(grad_out.shape[2:]))


def _chunk_setup_context(ctx, inputs, output):
    x, slices, lens, mode, _ = inputs
    ctx.save_for_backward(slices, lens)
    ctx.cfg = (mode, x.shape[1], x.shape[0] * x.shape[1] == 0)


def _chunk_backward(ctx, grad_out, grad_lens):
    slices, lens = ctx.saved_tensors
    mode, T, is_empty = ctx.cfg
    if is_empty:
        return torch.zeros_like(grad_out), None, None, None, None
    g = torch.ops.pydrobert_amd.chunk_by_slices_backward(grad_out, slices, lens, mode, T)
    return g, None, None, None, None


register_autograd("pydrobert_amd::chunk_by_slices", _chunk_backward, setup_context=_chunk_setup_context)


def chunk_by_slices(
    x: torch.Tensor,
    slices: torch.Tensor,
    lens: Optional[torch.Tensor] = None,
    mode: str = "constant",
    value: float = config.DEFT_PAD_VALUE,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Functional version of :class:`ChunkBySlices` (reference _pad.py:383-463)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(x, slices, lens):
            return _chunk_by_slices_op._init_fn(x, slices, lens, mode, value)
    return torch.ops.pydrobert_amd.chunk_by_slices(x, slices, lens, mode, value)


class ChunkBySlices(torch.nn.Module):
    """Cut ``x[n, start:end]`` per row, padding where the slice leaves the sequence (reference
    _pad.py:466-548).  Returns ``(chunked, chunked_lens)``; steps of ``chunked[n]`` at or beyond
    ``chunked_lens[n]`` hold ``value`` in every mode."""

    __constants__ = ("mode", "value")
    mode: str
    value: float

    def __init__(self, mode: str = "constant", value: float = config.DEFT_PAD_VALUE) -> None:
        mode = argcheck.is_in(mode, tuple(_PAD_MODES), "mode")
        value = argcheck.is_float(value, "value")
        super().__init__()
        self.mode, self.value = mode, value

    def extra_repr(self) -> str:
        s = "mode={}".format(self.mode)
        if self.mode == "constant":
            s += ", value={}".format(self.value)
        return s

    def forward(
        self, x: torch.Tensor, slices: torch.Tensor, lens: Optional[torch.Tensor] = None
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        return chunk_by_slices(x, slices, lens, self.mode, self.value)
