"""Discounted returns on MI355X (reference _rl.py:24-96): the step that turns the per-token rewards of a
sampled batch into what each token is credited with.

The reference multiplies by a ``(T, T)`` matrix of ``gamma**i / gamma**j``; here it is the scan
``R[t] = r[t] + gamma * R[t + 1]`` (``csrc/returns.hip``): O(T), finite for every ``gamma`` and ``T``.  The
adjoint is the same scan run the other way, so backward -- and double backward -- is the forward op with
``reverse`` flipped.  No host read.  CPU tensors (rewards shaped in data-loader workers) take a torch body
that runs the recurrence.
"""
import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck
from ._feats import _dtype_code

__all__ = ["TimeDistributedReturn", "time_distributed_return"]


def _return_torch(r: torch.Tensor, gamma: float, time_dim: int, reverse: bool) -> torch.Tensor:
    """Torch body: the recurrence over the frames, accumulated as the kernels do (float32, or float64)."""
    ct = torch.float64 if r.dtype == torch.float64 else torch.float32
    x = r.movedim(time_dim, 0).to(ct)
    T = x.shape[0]
    out = torch.empty_like(x)
    acc = torch.zeros_like(x[0]) if T else None
    for s in range(T):
        t = s if reverse else T - 1 - s
        acc = x[t] + gamma * acc
        out[t] = acc
    return torch.empty_like(r).copy_(out.movedim(0, time_dim))


@custom_op("pydrobert_amd::time_distributed_return", mutates_args=())
def _return_op(r: torch.Tensor, gamma: float, batch_first: bool, reverse: bool) -> torch.Tensor:
    if r.dim() != 2:
        raise RuntimeError("r must be 2 dimensional")
    dt = _dtype_code(r)
    r = r.detach()
    td = 1 if batch_first else 0
    if r.device.type == "cpu":
        return _return_torch(r, gamma, td, reverse)
    device = _cabi.require_hip(r)
    R = torch.empty_like(r)  # (r's own axis order when r is dense: both sides of the kernel coalesce)
    T, N = r.shape[td], r.shape[1 - td]
    if T * N == 0:
        return R
    lib = _cabi.lib()
    R_st, R_sn = R.stride(td), R.stride(1 - td)
    nbytes = lib.pdt_time_distributed_return_workspace_bytes(T, N, dt, R_st, R_sn)
    ws = torch.empty((nbytes,), device=device, dtype=torch.uint8) if nbytes > 0 else None
    g = _cabi.ctypes.c_double(gamma)
    with _cabi.on_device(device):
        rc = lib.pdt_time_distributed_return(
            _cabi.ptr(r), dt, T, N, r.stride(td), r.stride(1 - td), _cabi.ctypes.addressof(g), int(reverse),
            _cabi.ptr(R), R_st, R_sn, _cabi.ptr(ws), max(nbytes, 0), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_time_distributed_return")
    return R


@_return_op.register_fake
def _(r, gamma, batch_first, reverse):
    return torch.empty_like(r)


def _return_setup_context(ctx, inputs, output):
    _, ctx.gamma, ctx.batch_first, ctx.reverse = inputs


def _return_backward(ctx, grad_R):
    g = torch.ops.pydrobert_amd.time_distributed_return(grad_R, ctx.gamma, ctx.batch_first, not ctx.reverse)
    return g, None, None, None


register_autograd("pydrobert_amd::time_distributed_return", _return_backward, setup_context=_return_setup_context)


def time_distributed_return(r: torch.Tensor, gamma: float, batch_first: bool = False) -> torch.Tensor:
    """Functional version of :class:`TimeDistributedReturn` (reference _rl.py:24-41)."""
    if r.dim() != 2:
        raise RuntimeError("r must be 2 dimensional")
    if gamma == 0.0:
        return r
    if not torch.jit.is_scripting():
        if not torch.jit.is_tracing() and _cabi.plain_call(r):
            return _return_op._init_fn(r, gamma, batch_first, False)
    return torch.ops.pydrobert_amd.time_distributed_return(r, gamma, batch_first, False)


class TimeDistributedReturn(torch.nn.Module):
    r"""Accumulate future local rewards at every time step (reference _rl.py:44-96):
    :math:`R_t = \sum_{t' \ge t} \gamma^{t' - t} r_{t'}` for ``r`` of shape ``(T, N)``, or ``(N, T)`` with
    ``batch_first``.  ``gamma`` gets no gradient; ``gamma == 0`` returns ``r`` itself."""

    __constants__ = ["gamma", "batch_first"]
    gamma: float
    batch_first: bool

    def __init__(self, gamma: float, batch_first: bool):
        gamma = argcheck.is_float(gamma, "gamma")
        batch_first = argcheck.is_bool(batch_first, "batch_first")
        super().__init__()
        self.gamma, self.batch_first = gamma, batch_first

    def extra_repr(self) -> str:
        return "gamma={},batch_first={}".format(self.gamma, self.batch_first)

    def forward(self, r: torch.Tensor) -> torch.Tensor:
        return time_distributed_return(r, self.gamma, self.batch_first)
