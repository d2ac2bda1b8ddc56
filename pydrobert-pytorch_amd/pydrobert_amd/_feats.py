"""Feature deltas and mean/variance normalisation on MI355X (reference _feats.py:29-415): the two
operators of the feature front end ahead of SpecAugment.

On a ROCm device every pass is HIP (``csrc/feats.hip``): the deltas in one pass that writes the final
layout, the statistics as a fixed-order float64 reduction, the normalisation and both backward passes
elementwise.  No host read in any forward, backward or ``accumulate``.  CPU tensors (data-loader
workers) take a torch body written from the same formulas.

``slice_spect_data`` and ``chunk_token_sequences_by_slices`` (reference _feats.py:417-930) run on the row
compaction of ``csrc/seq_chunk.hip``, with the same split between HIP and the torch body.
"""
from typing import List, Optional, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck, config

__all__ = [
    "ChunkTokenSequencesBySlices",
    "FeatureDeltas",
    "MeanVarianceNormalization",
    "SliceSpectData",
    "chunk_token_sequences_by_slices",
    "feat_deltas",
    "mean_var_norm",
    "slice_spect_data",
]

_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
_PAD_MODES = {"replicate": 0, "reflect": 1, "circular": 2, "constant": 3}
_MVN_STATS, _MVN_ACCUM, _MVN_GRAD = 0, 1, 2


def _dtype_code(x: torch.Tensor) -> int:
    if x.dtype not in _DTYPES:
        raise TypeError("expected a floating-point tensor (float16/bfloat16/float32/float64), got {}".format(x.dtype))
    return _DTYPES[x.dtype]


def _compute_dtype(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def _prod(sizes) -> int:
    p = 1
    for s in sizes:
        p *= int(s)
    return p


# ----------------------------------------------------------------------------------------------------------
# deltas


def _check_order_width(order: int, width: int) -> None:
    if order < 0 or width < 1:
        raise RuntimeError(
            "feature deltas need order >= 0 and width >= 1 (order={}, width={})".format(order, width)
        )


def _feat_delta_filters(order: int, width: int) -> torch.Tensor:
    """The (order + 1, 1 + 2P) composite taps in float32, P = width * order.  Row 0 picks the centre
    sample; row u is row u - 1 cross-correlated with the slope kernel k[i] = (width - i) / sum_j j^2,
    i = 0 .. 2 * width, the row zero-padded by ``width`` on each side first.

    The correlation is spelt out, one slope tap after the other with each partial sum rounded to float32
    (the product of two float32 numbers is exact in float64): conv1d rounds differently from one CPU's
    vector units to another's, and these are the reference's filters bit for bit on all of them."""
    _check_order_width(order, width)
    K = 1 + 2 * width * order
    slope = torch.linspace(width, -width, 2 * width + 1, dtype=torch.float32)
    slope = (slope / slope.pow(2).sum()).double()
    taps = torch.zeros((order + 1, K), dtype=torch.float32)
    taps[0, K // 2] = 1.0
    for u in range(1, order + 1):
        padded = torch.nn.functional.pad(taps[u - 1], (width, width)).double()
        acc = torch.zeros(K, dtype=torch.float64)
        for i in range(2 * width + 1):
            acc = (acc + slope[i] * padded[i:i + K]).float().double()
        taps[u] = acc.float()
    return taps


_TAPS = {}


def _taps(filters: Optional[torch.Tensor], order: int, width: int, x: torch.Tensor) -> torch.Tensor:
    """The filters on x's device in the kernels' compute type.  Built ones are cached per (order, width,
    dtype, device): copied once from pinned memory without blocking the host, with an event the stream of
    every later call waits on (the copy may have been queued on another stream)."""
    ct = _compute_dtype(x.dtype)
    if filters is not None:
        return filters.detach().to(device=x.device, dtype=ct).contiguous()
    key = (order, width, ct, x.device)
    entry = _TAPS.get(key)
    if entry is None:
        host = _feat_delta_filters(order, width).to(ct).pin_memory()
        with torch.cuda.device(x.device):
            dev = host.to(x.device, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record()
        entry = _TAPS[key] = (host, dev, ready)
    torch.cuda.current_stream(x.device).wait_event(entry[2])
    return entry[1]


def _delta_geometry(shape: List[int], dim: int, time_dim: int, concatenate: bool) -> Tuple[int, int]:
    """(time axis, axis the order axis is inserted before), both normalised; the reference's errors."""
    D = len(shape)
    if time_dim < -D or time_dim >= D:
        raise RuntimeError("time_dim {} is outside [{}, {}] for a {}-D input".format(time_dim, -D, D - 1, D))
    time_dim = (time_dim + D) % D
    Dd = D if concatenate else D + 1
    if dim < -Dd or dim >= Dd:
        raise RuntimeError("dim {} is outside [{}, {}] (the output has {} dims)".format(dim, -Dd, Dd - 1, Dd))
    return time_dim, (dim + Dd) % Dd


def _delta_out_shape(shape: List[int], k: int, U: int, concatenate: bool) -> List[int]:
    out = list(shape)
    if concatenate:
        out[k] = out[k] * U
    else:
        out.insert(k, U)
    return out


def _delta_checks(shape, filters, dim, time_dim, concatenate, order, width, pad_mode, value=0.0):
    if filters is None:
        _check_order_width(order, width)  # (the reference builds them first: its errors come first)
    else:
        assert tuple(filters.shape) == (order + 1, 1 + (2 * width) * order)
    t, k = _delta_geometry(list(shape), dim, time_dim, concatenate)
    if pad_mode not in _PAD_MODES:
        raise NotImplementedError("Unrecognised padding mode {}".format(pad_mode))
    if pad_mode != "constant" and value != 0:  # (torch.nn.functional.pad's own check)
        raise RuntimeError("pad_mode '{}' takes no fill value (got value={})".format(pad_mode, value))
    T, P = shape[t], width * order
    if T == 0:
        raise RuntimeError("feat_deltas: the time axis is empty")
    if pad_mode == "reflect" and P >= T:
        raise RuntimeError("reflect padding of {} samples needs more than {} time steps".format(P, T))
    if pad_mode == "circular" and P > T:
        raise RuntimeError("circular padding of {} samples wraps more than once around {} time steps".format(P, T))
    return t, k


def _padded_index(T: int, P: int, mode: str) -> Optional[torch.Tensor]:
    j = torch.arange(-P, T + P)
    if mode == "replicate":
        return j.clamp(0, T - 1)
    if mode == "reflect":
        return torch.where(j < 0, -j, torch.where(j >= T, 2 * (T - 1) - j, j))
    if mode == "circular":
        return j.remainder(T)
    return None


def _feat_deltas_torch(x, filters, t, k, concatenate, order, width, pad_mode, value):
    """Torch body (CPU tensors, and the device restatement the timing tool compares with)."""
    T, P, U = x.shape[t], width * order, order + 1
    f = filters.to(x)
    idx = _padded_index(T, P, pad_mode)
    xt = x.movedim(t, -1)
    if idx is None:
        xp = torch.nn.functional.pad(xt, (P, P), "constant", value)
    else:
        xp = xt.index_select(-1, idx.to(x.device))
    win = xp.unfold(-1, 1 + 2 * P, 1)  # (..., T, K)
    out = torch.einsum("...tk,uk->...ut", win, f)  # (..., U, T)
    out = out.movedim(-1, t).movedim(-1, k)  # T back in place, then U before x's axis k
    if concatenate:
        out = out.flatten(k, k + 1)
    return out.contiguous()


def _feat_deltas_adjoint_torch(grad_out, filters, x_shape, t, k, concatenate, order, width, pad_mode):
    """Torch body of the adjoint: a full correlation with the flipped taps over the padded axis, whose
    padding is then folded back onto the samples it copied (dropped for constant padding)."""
    T, P, U = x_shape[t], width * order, order + 1
    f = filters.to(grad_out).flip(-1)
    g = grad_out.unflatten(k, (U, x_shape[k])) if concatenate else grad_out
    g = g.movedim(k, -1).movedim(t, -1)  # (..., U, T)
    gp = torch.nn.functional.pad(g, (2 * P, 2 * P))
    gxp = torch.einsum("...utk,uk->...t", gp.unfold(-1, 1 + 2 * P, 1), f)  # (..., T + 2P)
    idx = _padded_index(T, P, pad_mode)
    if idx is None:
        gx = gxp[..., P:P + T]
    else:
        gx = gxp.new_zeros(gxp.shape[:-1] + (T,)).index_add_(-1, idx, gxp)
    return gx.movedim(-1, t).contiguous()


def _collapse(shape, strides, lo, hi):
    """Element stride of dims [lo, hi) as one axis, or None if they do not collapse."""
    st = expect = None
    for d in range(hi - 1, lo - 1, -1):
        if shape[d] == 1:
            continue
        if st is not None and strides[d] != expect:
            return None
        if st is None:
            st = strides[d]
        expect = strides[d] * shape[d]
    return 0 if st is None else st


def _delta_groups(shape, t, k):
    """(A, B, T, C, D) sizes, their dim ranges and whether the order axis sits before D."""
    D = len(shape)
    if k <= t:
        ranges = ((0, k), (k, t), (t, t + 1), (t + 1, t + 1), (t + 1, D))
    else:
        ranges = ((0, t), (t, t), (t, t + 1), (t + 1, k), (k, D))
    return [_prod(shape[lo:hi]) for lo, hi in ranges], ranges, k > t


def _feat_deltas_hip(x, taps, t, k, concatenate, U, P, pad_mode, value):
    device = _cabi.require_hip(x)
    dt = _dtype_code(x)
    shape = list(x.shape)
    sizes, ranges, u_inner = _delta_groups(shape, t, k)
    strides = [_collapse(shape, list(x.stride()), lo, hi) for lo, hi in ranges]
    if any(s is None for s in strides):
        x = x.contiguous()
        strides = [_collapse(shape, list(x.stride()), lo, hi) for lo, hi in ranges]
    out = torch.empty(_delta_out_shape(shape, k, U, concatenate), device=device, dtype=x.dtype)
    fill = None
    if pad_mode == "constant":
        fill = torch.full((1,), value, device=device, dtype=x.dtype).to(taps.dtype)
    A, B, T, C, D = sizes
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_feat_deltas(
            _cabi.ptr(x) if x.numel() else None, dt, A, B, T, C, D, *strides, _cabi.ptr(taps), U, P,
            _PAD_MODES[pad_mode], _cabi.ptr(fill), int(u_inner), _cabi.ptr(out) if out.numel() else None,
            _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_feat_deltas")
    return out


@custom_op("pydrobert_amd::feat_deltas", mutates_args=())
def _feat_deltas_op(
    x: torch.Tensor, filters: Optional[torch.Tensor], dim: int, time_dim: int, concatenate: bool,
    order: int, width: int, pad_mode: str, value: float,
) -> torch.Tensor:  # fmt: skip
    t, k = _delta_checks(x.shape, filters, dim, time_dim, concatenate, order, width, pad_mode, value)
    _dtype_code(x)
    if x.device.type == "cpu":
        f = _feat_delta_filters(order, width) if filters is None else filters
        return _feat_deltas_torch(x.detach(), f.detach(), t, k, concatenate, order, width, pad_mode, value)
    return _feat_deltas_hip(x.detach(), _taps(filters, order, width, x), t, k, concatenate, order + 1,
                            width * order, pad_mode, value)  # fmt: skip


@_feat_deltas_op.register_fake
def _(x, filters, dim, time_dim, concatenate, order, width, pad_mode, value):
    t, k = _delta_geometry(list(x.shape), dim, time_dim, concatenate)
    return x.new_empty(_delta_out_shape(list(x.shape), k, order + 1, concatenate))


@custom_op("pydrobert_amd::feat_deltas_backward", mutates_args=())
def _feat_deltas_backward_op(
    grad_out: torch.Tensor, filters: Optional[torch.Tensor], x_shape: List[int], dim: int, time_dim: int,
    concatenate: bool, order: int, width: int, pad_mode: str,
) -> torch.Tensor:  # fmt: skip
    t, k = _delta_checks(x_shape, filters, dim, time_dim, concatenate, order, width, pad_mode)
    if grad_out.device.type == "cpu":
        f = (_feat_delta_filters(order, width) if filters is None else filters).detach()
        return _feat_deltas_adjoint_torch(grad_out.detach(), f, x_shape, t, k, concatenate, order, width, pad_mode)
    device = _cabi.require_hip(grad_out)
    dt = _dtype_code(grad_out)
    g = grad_out.detach().contiguous()
    taps = _taps(filters, order, width, g)
    sizes, _, u_inner = _delta_groups(list(x_shape), t, k)
    A, B, T, C, D = sizes
    grad_x = torch.empty(x_shape, device=device, dtype=g.dtype)
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_feat_deltas_backward(
            _cabi.ptr(g) if g.numel() else None, dt, A, B, T, C, D, _cabi.ptr(taps), order + 1, width * order,
            _PAD_MODES[pad_mode], int(u_inner), _cabi.ptr(grad_x) if grad_x.numel() else None,
            _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_feat_deltas_backward")
    return grad_x


@_feat_deltas_backward_op.register_fake
def _(grad_out, filters, x_shape, dim, time_dim, concatenate, order, width, pad_mode):
    return grad_out.new_empty(x_shape)


def _deltas_setup_context(ctx, inputs, output):
    x, filters, dim, time_dim, concatenate, order, width, pad_mode, _ = inputs
    ctx.filters = filters
    ctx.cfg = (list(x.shape), dim, time_dim, concatenate, order, width, pad_mode)


def _deltas_backward(ctx, grad_out):
    shape, dim, time_dim, concatenate, order, width, pad_mode = ctx.cfg
    g = torch.ops.pydrobert_amd.feat_deltas_backward(
        grad_out, ctx.filters, shape, dim, time_dim, concatenate, order, width, pad_mode
    )
    return g, None, None, None, None, None, None, None, None


def _deltas_backward_setup_context(ctx, inputs, output):
    _, filters, _, dim, time_dim, concatenate, order, width, pad_mode = inputs
    ctx.filters = filters
    ctx.cfg = (dim, time_dim, concatenate, order, width, pad_mode)


def _deltas_backward_backward(ctx, gg):
    # the adjoint of the adjoint: the forward op, the constant padding contributing nothing
    dim, time_dim, concatenate, order, width, pad_mode = ctx.cfg
    g = torch.ops.pydrobert_amd.feat_deltas(gg, ctx.filters, dim, time_dim, concatenate, order, width, pad_mode, 0.0)
    return g, None, None, None, None, None, None, None, None


register_autograd("pydrobert_amd::feat_deltas", _deltas_backward, setup_context=_deltas_setup_context)
register_autograd(
    "pydrobert_amd::feat_deltas_backward", _deltas_backward_backward, setup_context=_deltas_backward_setup_context
)


def feat_deltas(
    x: torch.Tensor,
    dim: int = -1,
    time_dim: int = -2,
    concatenate: bool = True,
    order: int = 2,
    width: int = 2,
    pad_mode: str = "replicate",
    value: float = config.DEFT_PAD_VALUE,
    _filters: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Functional version of :class:`FeatureDeltas` (reference _feats.py:216-286)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(x, _filters):
            return _feat_deltas_op._init_fn(x, _filters, dim, time_dim, concatenate, order, width, pad_mode, value)
    return torch.ops.pydrobert_amd.feat_deltas(x, _filters, dim, time_dim, concatenate, order, width, pad_mode, value)


class FeatureDeltas(torch.nn.Module):
    """Compute deltas of features along ``time_dim``, stacked or concatenated at ``dim`` (reference
    _feats.py:289-415).  Order ``u`` is the order ``u - 1`` deltas correlated with ``w / sum(w'^2)`` over
    ``w`` in ``[-width, width]``; the edges are padded by ``pad_mode``."""

    __constants__ = ["dim", "time_dim", "concatenate", "order", "width", "pad_mode", "value"]
    dim: int
    time_dim: int
    order: int
    width: int
    pad_mode: str
    value: float
    filters: torch.Tensor

    def __init__(
        self,
        dim: int = -1,
        time_dim: int = -2,
        concatenate: bool = True,
        order: int = 2,
        width: int = 2,
        pad_mode: str = "replicate",
        value: float = config.DEFT_PAD_VALUE,
    ):
        checked = dict(
            dim=argcheck.is_int(dim, "dim"),
            time_dim=argcheck.is_int(time_dim, "time_dim"),
            concatenate=argcheck.is_bool(concatenate, "concatenate"),
            order=argcheck.is_nonnegi(order, "order"),
            pad_mode=argcheck.is_in(pad_mode, tuple(_PAD_MODES), "pad_mode"),
        )
        super().__init__()
        for name, val in checked.items():
            setattr(self, name, val)
        self.width = width
        self.value = value
        # built here so that a bad width raises at construction, as the functional form does per call
        self.register_buffer("filters", _feat_delta_filters(checked["order"], width))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        cfg = (self.dim, self.time_dim, self.concatenate, self.order, self.width, self.pad_mode, self.value)
        return feat_deltas(x, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], cfg[6], self.filters)

    def extra_repr(self) -> str:
        names = ("dim", "time_dim", "concatenate", "order", "width", "pad_mode", "value")
        return ", ".join("{}={}".format(n, getattr(self, n)) for n in names)


# ----------------------------------------------------------------------------------------------------------
# mean / variance


def _mvn_dim(x: torch.Tensor, dim: int) -> int:
    D = x.dim()
    if dim < -D or dim > D - 1:
        raise IndexError("dim {} is outside [{}, {}] for a {}-D input".format(dim, -D, D - 1, D))
    return (dim + D) % D


def _mvn_axes(x: torch.Tensor, dim: int) -> Tuple[int, int, int]:
    return _prod(x.shape[:dim]), int(x.shape[dim]), _prod(x.shape[dim + 1:])


def _vec(v: Optional[torch.Tensor], X: int, device, what: str) -> Optional[torch.Tensor]:
    if v is None:
        return None
    if v.numel() != X:
        raise RuntimeError("{} has {} elements, expected {}".format(what, v.numel(), X))
    return v.detach().reshape(X).to(device).contiguous()  # (the kernels index it densely)


def _mvn_stats(x3: torch.Tensor, mode: int, out0, out1, count=None, g=None, m=None):
    """pdt_mvn_stats on a contiguous (A, X, B) view (out0 / out1 / count float64, on the stream)."""
    device = x3.device
    A, X, B = x3.shape
    lib = _cabi.lib()
    ws = torch.empty((max(1, lib.pdt_mvn_stats_workspace_bytes(A, X, B)),), device=device, dtype=torch.uint8)
    with _cabi.on_device(device):
        rc = lib.pdt_mvn_stats(
            _cabi.ptr(x3), _cabi.ptr(g), _cabi.ptr(m), _dtype_code(x3), A, X, B, mode, _cabi.ptr(out0),
            _cabi.ptr(out1), _cabi.ptr(count), _cabi.ptr(ws), ws.numel(), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_mvn_stats")


def _mvn_torch_stats(x3: torch.Tensor) -> torch.Tensor:
    """(2, X) float64: mean and population std per index of a (A, X, B) tensor (CPU body)."""
    xd = x3.transpose(0, 1).reshape(x3.shape[1], -1).double()
    mean = xd.mean(1)
    return torch.stack([mean, (xd - mean.unsqueeze(1)).square().mean(1).sqrt()])


@custom_op("pydrobert_amd::mean_var_norm", mutates_args=())
def _mean_var_norm_op(
    x: torch.Tensor, dim: int, mean: Optional[torch.Tensor], std: Optional[torch.Tensor], eps: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, stats): stats (2, X) float64 -- the mean and population std of x per index -- when either is
    computed, else (0, X)."""
    dim = _mvn_dim(x, dim)
    dt = _dtype_code(x)
    A, X, B = _mvn_axes(x, dim)
    mean, std = _vec(mean, X, x.device, "mean"), _vec(std, X, x.device, "std")
    x3 = x.detach().contiguous().view(A, X, B)
    need = mean is None or std is None
    stats = x3.new_empty((2 if need else 0, X), dtype=torch.float64)
    if need:
        if A * B == 0:
            stats.fill_(float("nan"))
        elif x.device.type == "cpu":
            stats.copy_(_mvn_torch_stats(x3))
        else:
            _cabi.require_hip(x)
            _mvn_stats(x3, _MVN_STATS, stats[0], stats[1])
    m = (stats[0] if mean is None else mean).to(x.dtype)
    s = (stats[1] if std is None else std).to(x.dtype).clamp_min(eps)
    if x.device.type == "cpu":
        y = ((x3 - m.view(1, X, 1)) / s.view(1, X, 1)).to(x.dtype)
    else:
        y = torch.empty_like(x3)
        with _cabi.on_device(x.device):
            rc = _cabi.lib().pdt_mvn_apply(
                _cabi.ptr(x3) if x3.numel() else None, dt, A, X, B, _cabi.ptr(m), _cabi.ptr(s),
                _cabi.ptr(y) if y.numel() else None, _cabi.stream_ptr(x.device),
            )  # fmt: skip
        _cabi.check(rc, "pdt_mvn_apply")
    return y.view(x.shape), stats


@_mean_var_norm_op.register_fake
def _(x, dim, mean, std, eps):
    dim = _mvn_dim(x, dim)
    X = x.shape[dim]
    need = mean is None or std is None
    return x.new_empty(x.shape), x.new_empty((2 if need else 0, X), dtype=torch.float64)


@custom_op("pydrobert_amd::mean_var_norm_backward", mutates_args=())
def _mean_var_norm_backward_op(
    grad_y: torch.Tensor, x: torch.Tensor, dim: int, mean: Optional[torch.Tensor], std: Optional[torch.Tensor],
    stats: torch.Tensor, eps: float,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:  # fmt: skip
    """(grad_x, grad_mean, grad_std), the last two float64 (X,) (zeros where the statistic was computed)."""
    dim = _mvn_dim(x, dim)
    dt = _dtype_code(x)
    A, X, B = _mvn_axes(x, dim)
    mean, std = _vec(mean, X, x.device, "mean"), _vec(std, X, x.device, "std")
    x3 = x.detach().contiguous().view(A, X, B)
    g3 = grad_y.detach().to(x.dtype).contiguous().view(A, X, B)
    n = float(A * B)
    m = (stats[0] if mean is None else mean).to(x.dtype)
    sigma = stats[1] if std is None else std
    s = sigma.to(x.dtype).clamp_min(eps).double()
    mask = sigma.to(x.dtype) >= eps  # (clamp_min passes the gradient where its input reaches the bound)
    # per-index sum g and sum g * c, c = x - m in x's dtype
    if x.device.type == "cpu":
        c3 = x3 - m.view(1, X, 1)
        sums = torch.stack([g3.double().sum((0, 2)), (g3.double() * c3.double()).sum((0, 2))])
    else:
        _cabi.require_hip(grad_y, x)
        sums = x3.new_empty((2, X), dtype=torch.float64)
        if A * B:
            _mvn_stats(x3, _MVN_GRAD, sums[0], sums[1], g=g3, m=m)
        else:
            sums.zero_()
    G1, G2 = sums[0], sums[1]
    dLds = -G2 / s.square()
    alpha = torch.zeros_like(s)
    beta = torch.zeros_like(s)
    if std is None:  # y depends on x through std: d std / d c_j = (c_j - mean(c)) / (n std)
        sig = stats[1]
        beta = torch.where(mask & (sig > 0), dLds / (n * sig), beta)
        alpha = alpha - beta * (stats[0] - m.double())
    if mean is None:  # ... and through the mean: minus the mean of d L / d c
        alpha = alpha - G1 / (n * s)
    coef = torch.stack([1.0 / s, alpha, beta]).to(_compute_dtype(x.dtype)).contiguous()
    if x.device.type == "cpu":
        c3 = x3 - m.view(1, X, 1)
        ct = coef.dtype
        gx = (g3.to(ct) * coef[0].view(1, X, 1) + coef[1].view(1, X, 1) + coef[2].view(1, X, 1) * c3.to(ct)).to(x.dtype)
    else:
        gx = torch.empty_like(x3)
        with _cabi.on_device(x.device):
            rc = _cabi.lib().pdt_mvn_backward(
                _cabi.ptr(g3) if g3.numel() else None, _cabi.ptr(x3) if x3.numel() else None, dt, A, X, B,
                _cabi.ptr(m), _cabi.ptr(coef), _cabi.ptr(gx) if gx.numel() else None, _cabi.stream_ptr(x.device),
            )  # fmt: skip
        _cabi.check(rc, "pdt_mvn_backward")
    grad_mean = -G1 / s if mean is not None else torch.zeros_like(s)
    grad_std = torch.where(mask, dLds, torch.zeros_like(s)) if std is not None else torch.zeros_like(s)
    return gx.view(x.shape), grad_mean, grad_std


@_mean_var_norm_backward_op.register_fake
def _(grad_y, x, dim, mean, std, stats, eps):
    dim = _mvn_dim(x, dim)
    X = x.shape[dim]
    return x.new_empty(x.shape), x.new_empty((X,), dtype=torch.float64), x.new_empty((X,), dtype=torch.float64)


def _mvn_setup_context(ctx, inputs, output):
    x, dim, mean, std, eps = inputs
    ctx.save_for_backward(x, mean, std, output[1])
    ctx.cfg = (dim, eps)
    ctx.mark_non_differentiable(output[1])


def _mvn_backward(ctx, grad_y, grad_stats):
    x, mean, std, stats = ctx.saved_tensors
    dim, eps = ctx.cfg
    gx, gm, gs = torch.ops.pydrobert_amd.mean_var_norm_backward(grad_y, x, dim, mean, std, stats, eps)
    gm = gm.view(mean.shape).to(mean.dtype) if mean is not None and ctx.needs_input_grad[2] else None
    gs = gs.view(std.shape).to(std.dtype) if std is not None and ctx.needs_input_grad[3] else None
    return gx if ctx.needs_input_grad[0] else None, None, gm, gs, None


register_autograd("pydrobert_amd::mean_var_norm", _mvn_backward, setup_context=_mvn_setup_context)


@custom_op("pydrobert_amd::mvn_accumulate", mutates_args=("count", "sum_", "sumsq"))
def _mvn_accumulate_op(x: torch.Tensor, dim: int, count: torch.Tensor, sum_: torch.Tensor, sumsq: torch.Tensor) -> None:
    """count += samples per index, sum_ += sum x, sumsq += sum x^2 (float64 buffers, in place)."""
    dim = _mvn_dim(x, dim)
    _dtype_code(x)
    A, X, B = _mvn_axes(x, dim)
    if sum_.shape != (X,) or sumsq.shape != (X,) or count.numel() != 1:
        raise RuntimeError("accumulated statistics have shape {}, expected ({},)".format(tuple(sum_.shape), X))
    x3 = x.detach().contiguous().view(A, X, B)
    if x.device.type == "cpu":
        xd = x3.double()
        count += A * B
        sum_ += xd.sum((0, 2))
        sumsq += xd.square().sum((0, 2))
        return
    _cabi.require_hip(x, count, sum_, sumsq)
    if count.dtype != torch.float64 or sum_.dtype != torch.float64 or sumsq.dtype != torch.float64:
        raise RuntimeError("accumulated statistics must be float64")
    if not (count.is_contiguous() and sum_.is_contiguous() and sumsq.is_contiguous()):
        raise RuntimeError("accumulated statistics must be contiguous")
    if A * B and X:
        _mvn_stats(x3, _MVN_ACCUM, sum_, sumsq, count=count)


@_mvn_accumulate_op.register_fake
def _(x, dim, count, sum_, sumsq):
    return None


def mean_var_norm(
    x: torch.Tensor,
    dim: int = -1,
    mean: Optional[torch.Tensor] = None,
    std: Optional[torch.Tensor] = None,
    eps: float = config.TINY,
) -> torch.Tensor:
    """Functional version of :class:`MeanVarianceNormalization` (reference _feats.py:29-52)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(x, mean, std):
            return _mean_var_norm_op._init_fn(x, dim, mean, std, eps)[0]
    return torch.ops.pydrobert_amd.mean_var_norm(x, dim, mean, std, eps)[0]


class MeanVarianceNormalization(torch.nn.Module):
    """Normalise features by mean and standard deviation per index of ``dim`` (reference
    _feats.py:55-213): given, computed from ``x``, or estimated with :func:`accumulate` and
    :func:`store`.  ``accumulate`` sums in float64 (the reference sums in ``x``'s dtype first)."""

    __constants__ = ["dim", "eps"]
    dim: int
    eps: float
    mean: Optional[torch.Tensor]
    std: Optional[torch.Tensor]
    count: Optional[torch.Tensor]
    sum: Optional[torch.Tensor]
    sumsq: Optional[torch.Tensor]

    def __init__(
        self,
        dim: int = -1,
        mean: Optional[torch.Tensor] = None,
        std: Optional[torch.Tensor] = None,
        eps: float = config.TINY,
    ):
        dim = argcheck.is_int(dim, "dim")
        given = {"mean": mean, "std": std}
        for name, stat in given.items():
            if stat is None:
                continue
            if not isinstance(stat, torch.Tensor) or stat.dim() != 1 or stat.numel() == 0:
                raise ValueError("{} must be a non-empty vector (a 1-D tensor), got {!r}".format(name, stat))
        if mean is not None and std is not None and mean.numel() != std.numel():
            raise ValueError("mean has {} elements but std has {}".format(mean.numel(), std.numel()))
        eps = argcheck.is_nonnegf(eps, "eps")
        super().__init__()
        self.dim = dim
        self.eps = eps
        for name in ("mean", "std"):
            self.register_buffer(name, given[name])
        for name in ("sum", "sumsq", "count"):  # the accumulated statistics, created by accumulate()
            self.register_buffer(name, None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return mean_var_norm(x, self.dim, self.mean, self.std, self.eps)

    @torch.jit.export
    def accumulate(self, x: torch.Tensor) -> None:
        """Add the sample count, sum and sum of squares of ``x`` per index of ``dim`` to float64 buffers."""
        n, s1, s2 = self.count, self.sum, self.sumsq
        if n is None or s1 is None or s2 is None:
            width = x.size(self.dim)
            n = torch.zeros(1, dtype=torch.float64, device=x.device)
            s1 = torch.zeros(width, dtype=torch.float64, device=x.device)
            s2 = torch.zeros(width, dtype=torch.float64, device=x.device)
            self.count = n
            self.sum = s1
            self.sumsq = s2
        torch.ops.pydrobert_amd.mvn_accumulate(x, self.dim, n, s1, s2)

    def extra_repr(self) -> str:
        return "dim={}, eps={:e}".format(self.dim, self.eps)

    @torch.jit.export
    def store(self, delete_stats: bool = True, bessel: bool = False) -> None:
        """Replace ``mean`` / ``std`` by the estimates from what :func:`accumulate` gathered: the sample mean
        and the population (or with ``bessel`` the unbiased) standard deviation.  Raises
        :class:`RuntimeError` below two accumulated samples."""
        n, s1, s2 = self.count, self.sum, self.sumsq
        if n is None or s1 is None or s2 is None:
            raise RuntimeError("store() needs at least two accumulated samples; none were accumulated")
        if bool(n < 2):  # (one host read, on the (1,) count)
            raise RuntimeError("store() needs at least two accumulated samples")
        avg = s1 / n
        second = s2 / n - avg * avg  # E[x^2] - E[x]^2
        if bessel:
            second = second * (n / (n - 1))
        self.mean = avg
        self.std = second.sqrt()
        if delete_stats:
            self.sum = None
            self.sumsq = None
            self.count = None


# ----------------------------------------------------------------------------------------------------------
# slices of spectral data and of token sequences (csrc/seq_chunk.hip)

_POLICIES = ("fixed", "ali", "ref")
_WINDOW_TYPES = ("symmetric", "causal", "future")


def _fixed_geometry(T: int, window_type: str, valid_only: bool, lobe_size: int) -> Tuple[int, int, int, int, int]:
    """(TT, a0, shift, width, m0) of policy 'fixed' (reference _feats.py:459-484): candidate k < TT is
    [a0 + k shift, a0 + k shift + width) and counts for a row whose length exceeds m0 + k shift."""
    shift = lobe_size + 1
    if window_type == "symmetric":
        width = 2 * lobe_size + 1
        if valid_only:
            return -(-max(T - width + 1, 0) // shift), 0, shift, width, width - 1
        half = shift // 2
        return (T + half) // shift, half - lobe_size, shift, width, half
    if valid_only:
        return -(-max(T - lobe_size, 0) // shift), 0, shift, shift, shift - 1
    if window_type == "causal":
        return -(-T // shift), -lobe_size, shift, shift, 0
    return -(-T // shift), 0, shift, shift, 0


def _lobes(window_type: str, lobe_size: int) -> Tuple[int, int]:
    left = lobe_size if window_type in ("symmetric", "causal") else 0
    right = lobe_size if window_type in ("symmetric", "future") else 0
    return left, right


def _slice_checks(input, in_lens, other_lens, policy, window_type, lobe_size):
    N = input.shape[0]
    if lobe_size < 0:
        raise RuntimeError("Expected non-negative lobe_size, got {}".format(lobe_size))
    if window_type not in _WINDOW_TYPES:
        raise RuntimeError(
            "expected window_type to be one of 'symmetric', 'casual', or 'future' got '{}'".format(window_type)
        )
    if policy not in _POLICIES:
        raise RuntimeError("Expected policy to be one of 'fixed', 'ali', or 'ref'; got '{}'".format(policy))
    if policy == "ali" and input.dim() != 2:
        raise RuntimeError("expected tensor of dimension 2 with policy 'ali'")
    if policy == "ref":
        if input.dim() != 3:
            raise RuntimeError("Expected input to be 3-dimensional, got {}".format(input.dim()))
        if input.shape[2] != 3:
            raise RuntimeError("Expected 3rd dimension of input to be of size 3, got {}".format(input.shape[2]))
        if other_lens is not None and tuple(other_lens.shape) != (N,):
            raise RuntimeError("Expected other_lens to have shape ({},); got {}".format(N, tuple(other_lens.shape)))
    if in_lens is not None and tuple(in_lens.shape) != (N,):
        raise RuntimeError("Expected in_lens to be of shape ({},); got {}".format(N, tuple(in_lens.shape)))


def _labels(x: torch.Tensor) -> torch.Tensor:
    """Alignment labels as contiguous int64 that are equal exactly where the labels are."""
    if x.is_floating_point():
        x = (x.double() + 0.0).view(torch.int64)  # (-0.0 + 0.0 is +0.0: equal values, equal bits)
    return x.long().contiguous()


def _slice_spect_torch(input, in_lens, other_lens, policy, window_type, valid_only, lobe_size):
    """Torch body (CPU tensors, and the device restatement the timing tool compares with)."""
    N, T = input.shape[0], input.shape[1]
    device = input.device
    rows = torch.arange(N, device=device)
    left, right = _lobes(window_type, lobe_size)
    if policy == "fixed":
        TT, a0, shift, width, m0 = _fixed_geometry(T, window_type, valid_only, lobe_size)
        k = torch.arange(TT, device=device) * shift
        slices = torch.stack([a0 + k, a0 + k + width], 1).expand(N, TT, 2).flatten(0, 1)
        sources = rows.view(N, 1).expand(N, TT).flatten()
        if in_lens is not None:
            keep = (in_lens.view(N, 1) > m0 + k).flatten()
            slices, sources = slices[keep], sources[keep]
        return slices.contiguous(), sources.contiguous()
    lens = torch.full((N,), T, device=device) if in_lens is None else in_lens.long().clamp_max(T)
    steps = torch.arange(T, device=device)
    if policy == "ref":
        starts, ends = input[..., 1].long(), input[..., 2].long()
        if other_lens is None:  # the end of the row's last triple
            other_lens = ends[rows, (lens - 1).clamp_min(0)].masked_fill(lens == 0, 0)
        keep = (lens.view(N, 1) > steps) & (starts >= 0) & (ends >= 0)
        starts, ends, other = starts - left, ends + right, other_lens.view(N, 1)
        keep = keep & ((starts >= 0) & (ends <= other) if valid_only else (ends > 0) & (starts < other))
        keep = keep & (starts < ends)
        return torch.stack([starts[keep], ends[keep]], 1), rows.view(N, 1).expand(N, T)[keep]
    # ali: runs of equal labels within the row's length, then the closed form of the reference's lobe loop
    x = _labels(input)
    first = torch.cat([torch.ones((N, 1), dtype=torch.bool, device=device), x[:, 1:] != x[:, :-1]], 1)
    first = first & (steps < lens.view(N, 1))
    K = first.sum(1)
    where = first.nonzero()
    src, st = where[:, 0], where[:, 1]
    NN = src.numel()
    base = K.cumsum(0) - K
    k = torch.arange(NN, device=device) - base[src]
    last_of_row = k == K[src] - 1
    en = torch.where(last_of_row, lens[src], torch.cat([st[1:], st.new_zeros(1)]))
    if valid_only:
        keep = k + left + right < K[src]
        i = torch.arange(NN, device=device)[keep]
        return torch.stack([st[i], en[i + left + right]], 1), src[keep]
    lo = base[src] + (k - left).clamp_min(0)
    hi = base[src] + torch.minimum(k + right, K[src] - 1)
    return torch.stack([st[lo], en[hi]], 1), src


def _row_offsets(counts: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(exclusive scan of the row counts, their total): the one host read of a flat list's size."""
    ends = counts.cumsum(0)
    return (ends - counts).contiguous(), int(ends[-1].item())


def _slice_spect_hip(input, in_lens, other_lens, policy, window_type, valid_only, lobe_size):
    device = _cabi.require_hip(input, in_lens, other_lens)
    N, T = input.shape[0], input.shape[1]
    lib = _cabi.lib()
    left, right = _lobes(window_type, lobe_size)
    ln = None if in_lens is None else in_lens.long().contiguous()

    def empty(n):
        return (torch.empty((n, 2), dtype=torch.long, device=device), torch.empty((n,), dtype=torch.long, device=device))

    with _cabi.on_device(device):
        stream = _cabi.stream_ptr(device)
        counts = torch.zeros((N,), dtype=torch.long, device=device)
        if policy == "fixed":
            TT, a0, shift, width, m0 = _fixed_geometry(T, window_type, valid_only, lobe_size)
            if N * TT == 0:
                return empty(0)

            def run(base, emit, slices, sources):
                rc = lib.pdt_slice_fixed(N, TT, _cabi.ptr(ln), a0, shift, width, m0, _cabi.ptr(base), emit,
                                         _cabi.ptr(slices), _cabi.ptr(sources), _cabi.ptr(counts), stream)  # fmt: skip
                _cabi.check(rc, "pdt_slice_fixed")

            if ln is None:  # every candidate counts: the size is known, no host read
                slices, sources = empty(N * TT)
                run(None, 1, slices, sources)
                return slices, sources
        elif policy == "ref":
            if N == 0:
                return empty(0)
            x = input.long().contiguous()
            ol = None if other_lens is None else other_lens.long().contiguous()

            def run(base, emit, slices, sources):
                rc = lib.pdt_slice_ref(_cabi.ptr(x), N, T, _cabi.ptr(ln), _cabi.ptr(ol), left, right, int(valid_only),
                                       _cabi.ptr(base), emit, _cabi.ptr(slices), _cabi.ptr(sources), _cabi.ptr(counts),
                                       stream)  # fmt: skip
                _cabi.check(rc, "pdt_slice_ref")

        else:
            if N == 0:
                return empty(0)
            x = _labels(input)
            seg = torch.empty((N, T), dtype=torch.int32, device=device)
            rc = lib.pdt_slice_ali_segments(_cabi.ptr(x), N, T, _cabi.ptr(ln), _cabi.ptr(seg), _cabi.ptr(counts), stream)
            _cabi.check(rc, "pdt_slice_ali_segments")
            cnt = (counts - (left + right)).clamp_min(0) if valid_only else counts
            base, total = _row_offsets(cnt)
            slices, sources = empty(total)
            if total:
                rc = lib.pdt_slice_ali_emit(_cabi.ptr(seg), N, T, _cabi.ptr(ln), _cabi.ptr(counts), _cabi.ptr(cnt),
                                            _cabi.ptr(base), left, right, int(valid_only), _cabi.ptr(slices),
                                            _cabi.ptr(sources), stream)  # fmt: skip
                _cabi.check(rc, "pdt_slice_ali_emit")
            return slices, sources
        # a run that counts, the one host read, a run that writes each row at its offset
        run(None, 0, None, None)
        base, total = _row_offsets(counts)
        slices, sources = empty(total)
        if total:
            run(base, 1, slices, sources)
        return slices, sources


@custom_op("pydrobert_amd::slice_spect_data", mutates_args=())
def _slice_spect_data_op(
    input: torch.Tensor, in_lens: Optional[torch.Tensor], other_lens: Optional[torch.Tensor], policy: str,
    window_type: str, valid_only: bool, lobe_size: int,
) -> Tuple[torch.Tensor, torch.Tensor]:  # fmt: skip
    if input.dim() < 2:
        raise RuntimeError("Expected input to be at least 2-dimensional; got {}".format(input.dim()))
    if not input.shape[1]:
        return (torch.empty((0, 2), dtype=torch.long, device=input.device),
                torch.empty((0,), dtype=torch.long, device=input.device))  # fmt: skip
    _slice_checks(input, in_lens, other_lens, policy, window_type, lobe_size)
    args = (input.detach(), None if in_lens is None else in_lens.detach(),
            None if other_lens is None else other_lens.detach(), policy, window_type, valid_only, lobe_size)  # fmt: skip
    if input.device.type == "cpu":
        return _slice_spect_torch(*args)
    return _slice_spect_hip(*args)


@_slice_spect_data_op.register_fake
def _(input, in_lens, other_lens, policy, window_type, valid_only, lobe_size):
    n = torch.library.get_ctx().new_dynamic_size()
    return input.new_empty((n, 2), dtype=torch.long), input.new_empty((n,), dtype=torch.long)


def slice_spect_data(
    input: torch.Tensor,
    in_lens: Optional[torch.Tensor] = None,
    other_lens: Optional[torch.Tensor] = None,
    policy: str = "fixed",
    window_type: str = "symmetric",
    valid_only: bool = True,
    lobe_size: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Functional version of :class:`SliceSpectData` (reference _feats.py:430-588)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(input, in_lens, other_lens):
            return _slice_spect_data_op._init_fn(input, in_lens, other_lens, policy, window_type, valid_only, lobe_size)
    return torch.ops.pydrobert_amd.slice_spect_data(
        input, in_lens, other_lens, policy, window_type, valid_only, lobe_size
    )


class SliceSpectData(torch.nn.Module):
    """Determine slices of feature chunks by policy ``fixed`` (windows of fixed size and shift), ``ali``
    (runs of equal alignment labels) or ``ref`` (segments of token triples), each widened by ``lobe_size``
    according to ``window_type`` (reference _feats.py:591-787).  Returns ``(slices, sources)``: ``(M, 2)``
    start / end pairs and the batch row each came from, rows in order."""

    __constants__ = ("policy", "window_type", "valid_only", "lobe_size")
    policy: str
    window_type: str
    valid_only: bool
    lobe_size: int

    def __init__(
        self,
        policy: str = "fixed",
        window_type: str = "symmetric",
        valid_only: bool = True,
        lobe_size: int = 0,
    ) -> None:
        policy = argcheck.is_in(policy, _POLICIES, "policy")
        window_type = argcheck.is_in(window_type, _WINDOW_TYPES, "window_type")
        valid_only = argcheck.is_bool(valid_only, "valid_only")
        lobe_size = argcheck.is_nonnegi(lobe_size, "lobe_size")
        super().__init__()
        self.policy, self.window_type, self.lobe_size = policy, window_type, lobe_size
        self.valid_only = valid_only

    def extra_repr(self) -> str:
        return "policy={}, window_type={}, lobe_size={}, valid_only={}".format(
            self.policy, self.window_type, self.lobe_size, self.valid_only
        )

    def forward(
        self,
        input: torch.Tensor,
        in_lens: Optional[torch.Tensor] = None,
        other_lens: Optional[torch.Tensor] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        return slice_spect_data(
            input, in_lens, other_lens, self.policy, self.window_type, self.valid_only, self.lobe_size
        )


def _chunk_tokens_torch(refs, slices, ref_lens, partial, retain):
    N, R = refs.shape[0], refs.shape[1]
    steps = torch.arange(R, device=refs.device)
    rs, re, ss, se = refs[..., 1], refs[..., 2], slices[:, 0:1], slices[:, 1:2]
    keep = (rs >= 0) & (re >= 0) & (re >= rs)
    if ref_lens is not None:
        keep = keep & (ref_lens.unsqueeze(1) > steps)
    keep = keep & ((ss < re) & (se > rs) if partial else (ss <= rs) & (se >= re))
    lens = keep.long().sum(1)
    order = torch.argsort((~keep).to(torch.uint8), dim=1, stable=True)
    out = refs.gather(1, order.unsqueeze(2).expand(N, R, 3))
    if not retain:  # (the reference adds the slice start, _feats.py:836)
        out = torch.cat([out[..., :1], out[..., 1:] + slices[:, 0].view(N, 1, 1)], 2)
    return out.masked_fill((steps >= lens.unsqueeze(1)).unsqueeze(2), 0), lens


@custom_op("pydrobert_amd::chunk_token_sequences_by_slices", mutates_args=())
def _chunk_tokens_op(
    refs: torch.Tensor, slices: torch.Tensor, ref_lens: Optional[torch.Tensor], partial: bool, retain: bool
) -> Tuple[torch.Tensor, torch.Tensor]:
    if refs.dim() == 2:
        return refs.new_empty((0, refs.shape[1])), slices.new_empty((0,))
    if refs.dim() != 3 or refs.shape[2] != 3:
        raise RuntimeError(
            "Expected refs to be 2-dimensional or 3-dimensional with final dimension size 3. "
            "Got shape '{}'".format(tuple(refs.shape))
        )
    N, R = refs.shape[0], refs.shape[1]
    if tuple(slices.shape) != (N, 2):
        raise RuntimeError("Expected slices to be a tensor of shape ({}, 2), got {}".format(N, tuple(slices.shape)))
    if ref_lens is not None and tuple(ref_lens.shape) != (N,):
        raise RuntimeError("Expected ref_lens to be a tensor of shape ({},), got {}".format(N, tuple(ref_lens.shape)))
    if refs.is_floating_point() or refs.dtype == torch.bool:
        raise RuntimeError("Expected refs to be an integer tensor, got {}".format(refs.dtype))
    if refs.device.type == "cpu":
        out, lens = _chunk_tokens_torch(refs.detach(), slices.detach().to(refs.dtype), ref_lens, partial, retain)
        return out.contiguous(), lens
    device = _cabi.require_hip(refs, slices, ref_lens)
    rf = refs.detach().long().contiguous()
    sl = slices.detach().long().contiguous()
    rl = None if ref_lens is None else ref_lens.detach().long().contiguous()
    out = torch.empty((N, R, 3), dtype=torch.long, device=device)
    lens = torch.zeros((N,), dtype=torch.long, device=device)
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_chunk_tokens(
            _cabi.ptr(rf) if R else None, N, R, _cabi.ptr(sl), _cabi.ptr(rl), int(partial), int(retain),
            _cabi.ptr(out) if R else None, _cabi.ptr(lens), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_chunk_tokens")
    return out.to(refs.dtype), lens


@_chunk_tokens_op.register_fake
def _(refs, slices, ref_lens, partial, retain):
    if refs.dim() == 2:
        return refs.new_empty((0, refs.shape[1])), slices.new_empty((0,))
    return refs.new_empty(refs.shape), slices.new_empty((refs.shape[0],), dtype=torch.long)


def chunk_token_sequences_by_slices(
    refs: torch.Tensor,
    slices: torch.Tensor,
    ref_lens: Optional[torch.Tensor] = None,
    partial: bool = False,
    retain: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Functional version of :class:`ChunkTokenSequencesBySlices` (reference _feats.py:790-837)."""
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(refs, slices, ref_lens):
            return _chunk_tokens_op._init_fn(refs, slices, ref_lens, partial, retain)
    return torch.ops.pydrobert_amd.chunk_token_sequences_by_slices(refs, slices, ref_lens, partial, retain)


class ChunkTokenSequencesBySlices(torch.nn.Module):
    """Keep the ``(tok, start, end)`` triples of each row that fall in the row's slice -- within it, or with
    ``partial`` overlapping it -- left-packed (reference _feats.py:840-930).  Returns ``(chunked,
    chunked_lens)``; triples at or beyond ``chunked_lens[n]`` are zeros."""

    __constants__ = ("partial", "retain")
    partial: bool
    retain: bool

    def __init__(self, partial: bool = False, retain: bool = False) -> None:
        partial = argcheck.is_bool(partial, "partial")
        retain = argcheck.is_bool(retain, "retain")
        super().__init__()
        self.partial, self.retain = partial, retain

    def extra_repr(self) -> str:
        return ", ".join(name for name in ("partial", "retain") if getattr(self, name))

    def forward(
        self, ref: torch.Tensor, slices: torch.Tensor, ref_lens: Optional[torch.Tensor] = None
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        return chunk_token_sequences_by_slices(ref, slices, ref_lens, self.partial, self.retain)
