"""SpecAugment, polyharmonic splines and image warps on MI355X.

Host-side mirror of the reference's ``_img.py`` for the operators on the hot path
(``polyharmonic_spline``, ``warp_1d_grid``, ``dense_image_warp``, ``sparse_image_warp``,
``spec_augment*`` and their Modules).  Kernels: ``csrc/spline.hip``, ``csrc/spec_augment.hip``, ``csrc/image_warp.hip`` through the C ABI
(``include/pdt_amd.h``).  ``spec_augment_apply_parameters`` and the image warps are
differentiable with respect to the features / image (bilinear scatter in the backward pass); the image
warps also with respect to the flow / the control points, and the spline with respect to points, values
and queries (``dense_image_warp_flow_backward``, ``sparse_image_warp_points_backward``,
``spline_eval_adjoint``: HIP kernels; the torch bodies they replaced stay as ``_dense_flow_grad_torch``,
``_sparse_points_grad_torch`` and ``_spline_eval_adjoint_torch`` for the sizes the kernels refuse and for
profiles/tools/time_warp_grads.py -- there is no run-time switch).
"""
import functools
import math
from typing import Any, List, Optional, Tuple

import warnings

import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck
from ._pad import pad_variable

__all__ = [
    "DenseImageWarp",
    "PolyharmonicSpline",
    "RandomShift",
    "SparseImageWarp",
    "SpecAugment",
    "Warp1DGrid",
    "dense_image_warp",
    "polyharmonic_spline",
    "random_shift",
    "sparse_image_warp",
    "spec_augment",
    "spec_augment_apply_parameters",
    "spec_augment_draw_parameters",
    "warp_1d_grid",
]

_MODES = {"bilinear": 0, "nearest": 1}
_PADDINGS = {"zeros": 0, "border": 1, "reflection": 2}
_INDEXINGS = ("hw", "wh")
SpecAugmentParams = Tuple[
    torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
    torch.Tensor, torch.Tensor,
]  # fmt: skip


_NARROWING_WARNED = False


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """float32 contiguous view / copy of ``t`` for the kernels.  Splines, 1-D grids and SpecAugment's
    resampling compute in float32 (the spline systems are solved in float64 inside); a float64
    argument there is narrowed and the result cast back, said out loud once per process.  (The
    reference itself keeps spline points, flows and 1-D grids in float32, _img.py:142-143, :283, :420,
    and RAISES for float64 spline values / SpecAugment warps -- a dtype mismatch inside
    ``linalg.solve`` / ``grid_sample``; its one float64 computation, sampling a float64 image, is
    float64 here too: ``_pixels``.)"""
    global _NARROWING_WARNED
    t = t.detach()
    if t.dtype != torch.float:
        if t.dtype == torch.double and not _NARROWING_WARNED:
            _NARROWING_WARNED = True
            warnings.warn(
                "pydrobert_amd: float64 input to an image operator is computed in float32 on the GPU "
                "and cast back (the reference computes in float64); this warning is shown once"
            )
        t = t.float()
    return t.contiguous()


def _pixels(t: torch.Tensor) -> Tuple[torch.Tensor, str]:
    """(contiguous pixels, entry-point suffix) for the gathers: a float64 image is sampled in float64
    (``pdt_*_f64``: the reference forms the grid and samples it in the image's type, _img.py:423-436;
    flows and spline points are float32 there whatever the image's type); anything else in float32."""
    if t.dtype == torch.double:
        return t.detach().contiguous(), "_f64"
    return _f32c(t), ""


@custom_op("pydrobert_amd::polyharmonic_spline", mutates_args=())
def _polyharmonic_spline_op(
    train_points: torch.Tensor,
    train_values: torch.Tensor,
    query_points: torch.Tensor,
    order: int,
    regularization_weight: float,
) -> torch.Tensor:
    if train_points.dim() != 3 or train_values.dim() != 3 or query_points.dim() != 3:
        raise RuntimeError("train_points, train_values and query_points must be 3 dimensional")
    N, T, I = train_points.shape
    O, Q = train_values.shape[2], query_points.shape[1]
    if train_values.shape[:2] != (N, T) or query_points.shape[0] != N or query_points.shape[2] != I:
        raise RuntimeError("train_points, train_values and query_points have inconsistent shapes")
    device = _cabi.require_hip(train_points, train_values, query_points)
    c, f, x = _f32c(train_points), _f32c(train_values), _f32c(query_points)
    L = _cabi.lib()
    with torch.cuda.device(device):
        out = torch.empty((N, Q, O), device=device, dtype=torch.float)
        ws = torch.empty((int(L.pdt_spline_workspace_bytes(N, T, I, O)),), device=device, dtype=torch.uint8)
        rc = L.pdt_polyharmonic_spline(
            _cabi.ptr(c), _cabi.ptr(f), _cabi.ptr(x), N, T, I, O, Q, int(order),
            float(regularization_weight), _cabi.ptr(out), _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_polyharmonic_spline")
    return out.to(train_values.dtype)


@_polyharmonic_spline_op.register_fake
def _(train_points, train_values, query_points, order, regularization_weight):
    return train_values.new_empty(
        (train_points.shape[0], query_points.shape[1], train_values.shape[2])
    )


def _spline_solve(c: torch.Tensor, f: torch.Tensor, tail: Optional[torch.Tensor], order: int, reg: float):
    """(N, T+I+1, O) float64 solution of the spline's bordered system for right-hand side
    [f; tail] (include/pdt_amd.h: pdt_spline_solve)."""
    N, T, I = c.shape
    O = f.shape[2]
    device = c.device
    L = _cabi.lib()
    with torch.cuda.device(device):
        sol = torch.empty((N, T + I + 1, O), device=device, dtype=torch.double)
        ws = torch.empty((int(L.pdt_spline_workspace_bytes(N, T, I, O)),), device=device, dtype=torch.uint8)
        rc = L.pdt_spline_solve(
            _cabi.ptr(c), _cabi.ptr(f), _cabi.ptr(tail), N, T, I, O, int(order), float(reg),
            _cabi.ptr(sol), _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_spline_solve")
    return sol


def _phi_and_slope(r: torch.Tensor, order: int):
    """phi(r) and phi'(r) / r (zero where r = 0: the direction vector vanishes there)."""
    eps = float(torch.finfo(torch.float).eps)
    pos = r > 0
    safe = torch.where(pos, r, torch.ones_like(r))
    if order % 2:
        phi = r**order
        slope = order * safe ** (order - 2)
    else:
        lg = torch.log(safe.clamp(min=eps))
        phi = r**order * lg
        inner = torch.where(safe > eps, order * lg + 1.0, torch.full_like(lg, order * math.log(eps)))
        slope = safe ** (order - 2) * inner
    return phi, torch.where(pos, slope, torch.zeros_like(slope))


def _spline_eval_adjoint_torch(G: torch.Tensor, c: torch.Tensor, sol: torch.Tensor, x: torch.Tensor, order: int,
                               need_gx: bool):  # fmt: skip
    """The query-sized sums of the spline's backward as elementwise torch ops in float64 over (N, Q, T, I):
    the shapes csrc/spline.hip's reduction refuses (I or O above 4), and the other contestant of
    profiles/tools/time_warp_grads.py.  Returns what ``_spline_eval_adjoint`` returns."""
    d = torch.double
    T, I = c.shape[1], c.shape[2]
    G, cd, xd = G.to(d), c.to(d), x.to(d)
    w, v = sol[:, :T], sol[:, T:]
    dxc = xd.unsqueeze(2) - cd.unsqueeze(1)  # (N, Q, T, I)
    phi_xc, slope_xc = _phi_and_slope(dxc.norm(dim=3), order)
    x1 = torch.cat([xd, torch.ones_like(xd[..., :1])], 2)
    g_sol = torch.cat([phi_xc.transpose(1, 2) @ G, x1.transpose(1, 2) @ G], 1)  # (N, T+I+1, O)
    g_phi = (G @ w.transpose(1, 2)) * slope_xc  # (N, Q, T): dL/dPhi * phi'/r
    g_c = -(g_phi.unsqueeze(3) * dxc).sum(1)
    g_x = (g_phi.unsqueeze(3) * dxc).sum(2) + G @ v[:, :I].transpose(1, 2) if need_gx else None
    return g_sol, g_c, g_x


def _pixel_lattice(N: int, H: int, W: int, device) -> torch.Tensor:
    """(N, H*W, 2) float queries (x = w, y = h) of an H x W image, row-major."""
    hh, ww = torch.meshgrid(
        torch.arange(H, dtype=torch.float, device=device), torch.arange(W, dtype=torch.float, device=device),
        indexing="ij",
    )  # fmt: skip
    return torch.stack([ww.flatten(), hh.flatten()], 1).unsqueeze(0).expand(N, H * W, 2)


@custom_op("pydrobert_amd::spline_eval_adjoint", mutates_args=())
def _spline_eval_adjoint_op(
    grad_out: torch.Tensor,
    train_points: torch.Tensor,
    solution: torch.Tensor,
    query_points: Optional[torch.Tensor],
    height: int,
    width: int,
    order: int,
    need_query_grad: bool,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The query-sized half of the spline's backward (csrc/spline.hip: pdt_spline_eval_adjoint), float64:
    ``(rhs (N, T+I+1, O), grad_points (N, T, I), grad_query (N, Q, I))`` for ``grad_out`` (N, Q, O), the
    centres ``train_points`` and the float64 ``solution`` (N, T+I+1, O) of the spline.  ``query_points``
    None: the pixel lattice of a ``height x width`` image.  ``grad_query`` has zero elements unless
    ``need_query_grad``.  I, O <= 4."""
    device = _cabi.require_hip(grad_out, train_points, solution, query_points)
    G, c = _f32c(grad_out), _f32c(train_points)
    x = None if query_points is None else _f32c(query_points)
    sol = solution.detach().contiguous()
    if sol.dtype != torch.double:
        raise RuntimeError("solution must be float64")
    N, T, I = c.shape
    Q, O = G.shape[1], G.shape[2]
    if sol.shape != (N, T + I + 1, O) or G.shape[0] != N or (x is not None and x.shape != (N, Q, I)):
        raise RuntimeError("grad_out, train_points, solution and query_points have inconsistent shapes")
    if need_query_grad and x is None:
        raise RuntimeError("the pixel lattice has no gradient")
    L = _cabi.lib()
    plan = (_cabi._I64 * 6)()
    _cabi.check(min(L.pdt_spline_eval_adjoint_plan(N, T, I, O, Q, plan), 0), "pdt_spline_eval_adjoint_plan")
    with torch.cuda.device(device):
        rhs = torch.empty((N, T + I + 1, O), device=device, dtype=torch.double)
        g_c = torch.empty((N, T, I), device=device, dtype=torch.double)
        g_x = torch.empty((N, Q, I) if need_query_grad else (0,), device=device, dtype=torch.double)
        ws = torch.empty((int(plan[2]),), device=device, dtype=torch.uint8)
        rc = L.pdt_spline_eval_adjoint(
            _cabi.ptr(G), _cabi.ptr(c), _cabi.ptr(sol), _cabi.ptr(x), N, T, I, O, Q, int(height), int(width),
            int(order), _cabi.ptr(rhs), _cabi.ptr(g_c), _cabi.ptr(g_x) if need_query_grad else None,
            _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_spline_eval_adjoint")
    return rhs, g_c, g_x


@_spline_eval_adjoint_op.register_fake
def _(grad_out, train_points, solution, query_points, height, width, order, need_query_grad):
    N, T, I = train_points.shape
    Q, O = grad_out.shape[1], grad_out.shape[2]
    d = torch.double
    return (
        grad_out.new_empty((N, T + I + 1, O), dtype=d),
        grad_out.new_empty((N, T, I), dtype=d),
        grad_out.new_empty((N, Q, I) if need_query_grad else (0,), dtype=d),
    )


_SPLINE_ADJOINT_MAX_DIM = 4  # csrc/spline.hip: kAdjMaxDim


def _spline_eval_adjoint(G, c, sol, x, H: int, W: int, order: int, need_gx: bool):
    """(g_sol, g_c, g_x): the adjoint system's right-hand side, the evaluation's share of the centres'
    gradient and the queries' gradient (None unless ``need_gx``), float64.  ``x`` None: the H x W pixel
    lattice.  The HIP reduction where it serves the sizes (I, O <= 4), the torch sums beyond."""
    if c.shape[2] <= _SPLINE_ADJOINT_MAX_DIM and G.shape[2] <= _SPLINE_ADJOINT_MAX_DIM:
        g_sol, g_c, g_x = torch.ops.pydrobert_amd.spline_eval_adjoint(G, c, sol, x, H, W, order, need_gx)
        return g_sol, g_c, (g_x if need_gx else None)
    if x is None:
        x = _pixel_lattice(c.shape[0], H, W, c.device)
    return _spline_eval_adjoint_torch(G, c, sol, x, order, need_gx)


def _spline_system_adjoint(c: torch.Tensor, sol: torch.Tensor, g_sol: torch.Tensor, order: int, reg: float):
    """(g_c, g_f) through the spline's system for the right-hand side ``g_sol`` of its adjoint: one solve
    (the matrix is symmetric), then dL/dM = -lam sol^T chained into the centres -- small torch ops over
    (N, T, T)."""
    T, I = c.shape[1], c.shape[2]
    cd = c.to(torch.double)
    w, v = sol[:, :T], sol[:, T:]
    lam = _spline_solve(c, g_sol[:, :T].float().contiguous(), g_sol[:, T:].float().contiguous(), order, reg)
    lam_w, lam_v = lam[:, :T], lam[:, T:]
    dcc = cd.unsqueeze(2) - cd.unsqueeze(1)  # (N, T, T, I)
    _, slope_cc = _phi_and_slope(dcc.norm(dim=3), order)
    g_A = -(lam_w @ w.transpose(1, 2))
    g_A = (g_A + g_A.transpose(1, 2)) * slope_cc
    g_c = (g_A.unsqueeze(3) * dcc).sum(2)
    g_B = -(lam_w @ v.transpose(1, 2) + w @ lam_v.transpose(1, 2))  # (N, T, I+1)
    return g_c + g_B[..., :I], lam_w


@custom_op("pydrobert_amd::polyharmonic_spline_backward", mutates_args=())
def _polyharmonic_spline_backward_op(
    grad_out: torch.Tensor,
    train_points: torch.Tensor,
    train_values: torch.Tensor,
    query_points: torch.Tensor,
    order: int,
    regularization_weight: float,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Gradients of the spline with respect to (train_points, train_values, query_points).

    With M the symmetric bordered matrix, [w; v] = M^-1 [f; 0] and out = Phi(x, c) w + [x 1] v:
    the adjoint system M lam = [Phi^T G; [x 1]^T G] is solved by the same kernel (float64), the
    rest are the chain rules of phi(|x - c|) and phi(|c_i - c_j|) -- elementwise / matmul device
    ops over (N, Q, T) and (N, T, T)."""
    _cabi.require_hip(grad_out, train_points, train_values, query_points)
    c, f, x = _f32c(train_points), _f32c(train_values), _f32c(query_points)
    sol = _spline_solve(c, f, None, order, regularization_weight)  # (N, T+I+1, O)
    g_sol, g_c, g_x = _spline_eval_adjoint(grad_out.detach(), c, sol, x, 0, 0, order, True)
    g_sys, g_f = _spline_system_adjoint(c, sol, g_sol, order, regularization_weight)
    g_c = g_c + g_sys
    return g_c.to(train_points.dtype), g_f.to(train_values.dtype), g_x.to(query_points.dtype)


@_polyharmonic_spline_backward_op.register_fake
def _(grad_out, train_points, train_values, query_points, order, regularization_weight):
    return (torch.empty_like(train_points), torch.empty_like(train_values), torch.empty_like(query_points))


def _spline_setup_context(ctx, inputs, output):
    train_points, train_values, query_points, order, reg = inputs
    ctx.save_for_backward(train_points, train_values, query_points)
    ctx.cfg = (order, reg)


def _spline_backward(ctx, grad_out):
    c, f, x = ctx.saved_tensors
    g_c, g_f, g_x = torch.ops.pydrobert_amd.polyharmonic_spline_backward(grad_out, c, f, x, ctx.cfg[0], ctx.cfg[1])
    return g_c, g_f, g_x, None, None


register_autograd(
    "pydrobert_amd::polyharmonic_spline", _spline_backward, setup_context=_spline_setup_context
)


def polyharmonic_spline(
    train_points: torch.Tensor,
    train_values: torch.Tensor,
    query_points: torch.Tensor,
    order: int,
    regularization_weight: float = 0.0,
    full_matrix: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`PolyharmonicSpline` (reference _img.py:133-150).

    ``full_matrix`` is accepted for signature parity: the bordered system is solved exactly in
    float64, which both of the reference's float32 evaluation orders approximate.
    """
    return torch.ops.pydrobert_amd.polyharmonic_spline(
        train_points, train_values, query_points, order, regularization_weight
    )


@custom_op("pydrobert_amd::warp_1d_grid", mutates_args=())
def _warp_1d_grid_op(
    src: torch.Tensor,
    flow: torch.Tensor,
    lengths: torch.Tensor,
    max_length: Optional[int],
    interpolation_order: int,
) -> torch.Tensor:
    device = _cabi.require_hip(src, flow, lengths)
    N = src.shape[0]
    if max_length is None:
        T = int(math.ceil(lengths.max().item())) if lengths.numel() else 0  # :279
    else:
        T = max_length
    s, fl, ln = _f32c(src), _f32c(flow), _f32c(lengths)
    with torch.cuda.device(device):
        grid = torch.empty((N, T), device=device, dtype=torch.float)
        rc = _cabi.lib().pdt_warp_1d_grid(
            _cabi.ptr(s), _cabi.ptr(fl), _cabi.ptr(ln), N, T, int(interpolation_order),
            _cabi.ptr(grid), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_warp_1d_grid")
    return grid


@_warp_1d_grid_op.register_fake
def _(src, flow, lengths, max_length, interpolation_order):
    T = torch.library.get_ctx().new_dynamic_size() if max_length is None else max_length
    return src.new_empty((src.shape[0], T), dtype=torch.float)


def _warp_1d_grid_setup(ctx, inputs, output):
    src, flow, lengths, _, order = inputs
    ctx.save_for_backward(src, flow, lengths)
    ctx.T, ctx.order = output.shape[1], order


def _warp_1d_grid_backward(ctx, grad):
    """The grid is a three-knot spline whose knots are affine (clamped) in src and flow
    (_img.py:284-302): chain the knots' torch formulas into the spline's own backward."""
    src, flow, lengths = ctx.saved_tensors
    T, N = ctx.T, src.shape[0]
    if T == 0 or N == 0:
        return torch.zeros_like(src), torch.zeros_like(flow), None, None, None
    with torch.enable_grad():
        s0, f0 = src.detach().float().requires_grad_(True), flow.detach().float().requires_grad_(True)
        ln = lengths.detach().float()
        eps = float(torch.finfo(torch.float).eps)
        s = torch.min(s0, ln - 1).clamp_min(0)
        d = torch.min(s + f0, ln - 1).clamp_min(0)
        s, d = (2.0 * s + 1.0) / T - 1.0, (2.0 * d + 1.0) / T - 1.0
        lo = torch.full_like(ln, 1.0 / T - 1.0 - eps)
        up = (2.0 * ln - 1.0) / T - 1.0 + eps
        t = ((2.0 * torch.arange(T, device=src.device) + 1.0) / T - 1.0).expand(N, T)
        grid = torch.ops.pydrobert_amd.polyharmonic_spline(
            torch.stack([lo, d, up], 1).unsqueeze(-1), torch.stack([lo, s, up], 1).unsqueeze(-1),
            t.unsqueeze(-1), ctx.order, 0.0,
        ).squeeze(-1)  # fmt: skip
        g_s, g_f = torch.autograd.grad(grid, [s0, f0], grad.float())
    return g_s.to(src.dtype), g_f.to(flow.dtype), None, None, None


register_autograd("pydrobert_amd::warp_1d_grid", _warp_1d_grid_backward, setup_context=_warp_1d_grid_setup)


def warp_1d_grid(
    src: torch.Tensor,
    flow: torch.Tensor,
    lengths: torch.Tensor,
    max_length: Optional[int] = None,
    interpolation_order: int = 1,
) -> torch.Tensor:
    """Functional version of :class:`Warp1DGrid` (reference _img.py:268-303)."""
    return torch.ops.pydrobert_amd.warp_1d_grid(src, flow, lengths, max_length, interpolation_order)


@custom_op("pydrobert_amd::dense_image_warp", mutates_args=())
def _dense_image_warp_op(
    image: torch.Tensor, flow: torch.Tensor, indexing: str, mode: str, padding_mode: str
) -> torch.Tensor:
    """dense_image_warp with a gradient for the image (bilinear taps are linear in it)."""
    if indexing not in _INDEXINGS:
        raise ValueError("Invalid indexing! must be one of 'wh' or 'hw'")
    if image.dim() != 4 or flow.dim() != 4:
        raise RuntimeError("image and flow must be 4 dimensional")
    N, C, H, W = image.shape
    if flow.shape != (N, H, W, 2):
        raise RuntimeError("expected flow to have shape {}, got {}".format((N, H, W, 2), tuple(flow.shape)))
    device = _cabi.require_hip(image, flow)
    (img, sfx), fl = _pixels(image), _f32c(flow)
    with torch.cuda.device(device):
        out = torch.empty_like(img)
        rc = getattr(_cabi.lib(), "pdt_dense_image_warp" + sfx)(
            _cabi.ptr(img), _cabi.ptr(fl), N, C, H, W, int(indexing == "hw"), _MODES[mode],
            _PADDINGS[padding_mode], _cabi.ptr(out), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_dense_image_warp")
    return out.to(image.dtype)


@_dense_image_warp_op.register_fake
def _(image, flow, indexing, mode, padding_mode):
    return image.new_empty(image.shape)


@custom_op("pydrobert_amd::dense_image_warp_backward", mutates_args=())
def _dense_image_warp_backward_op(
    grad_out: torch.Tensor, flow: torch.Tensor, indexing: str, mode: str, padding_mode: str
) -> torch.Tensor:
    """Adjoint of the gather with respect to the image (csrc/image_warp.hip, BACKWARD)."""
    device = _cabi.require_hip(grad_out, flow)
    (g, sfx), fl = _pixels(grad_out), _f32c(flow)
    N, C, H, W = g.shape
    with torch.cuda.device(device):
        grad = torch.empty_like(g)
        rc = getattr(_cabi.lib(), "pdt_dense_image_warp_backward" + sfx)(
            _cabi.ptr(g), _cabi.ptr(fl), N, C, H, W, int(indexing == "hw"), _MODES[mode],
            _PADDINGS[padding_mode], _cabi.ptr(grad), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_dense_image_warp_backward")
    return grad.to(grad_out.dtype)


@_dense_image_warp_backward_op.register_fake
def _(grad_out, flow, indexing, mode, padding_mode):
    return grad_out.new_empty(grad_out.shape)


def _sampling_grid_from_flow(flow: torch.Tensor, indexing: str, H: int, W: int) -> torch.Tensor:
    """grid_sample's normalised (x, y) grid for ``output[h, w] = image[h - flow_h, w - flow_w]``
    (the algebra of reference _img.py:400-433)."""
    hh, ww = torch.meshgrid(
        torch.arange(H, dtype=torch.float, device=flow.device),
        torch.arange(W, dtype=torch.float, device=flow.device), indexing="ij",
    )  # fmt: skip
    xy = torch.stack((ww, hh), 2).unsqueeze(0)
    fl = flow.flip(-1) if indexing == "hw" else flow
    size = torch.tensor([W, H], dtype=torch.float, device=flow.device)
    return (2 * xy - 2 * fl + 1.0) / size - 1.0


def _dense_setup_context(ctx, inputs, output):
    image, flow, indexing, mode, padding_mode = inputs
    ctx.needs_flow = flow.requires_grad
    if ctx.needs_flow:
        ctx.save_for_backward(flow, image)
    else:
        ctx.save_for_backward(flow)
    ctx.cfg = (indexing, mode, padding_mode)


def _dense_backward(ctx, grad_out):
    flow = ctx.saved_tensors[0]
    indexing, mode, padding_mode = ctx.cfg
    g = None
    if ctx.needs_input_grad[0]:
        g = torch.ops.pydrobert_amd.dense_image_warp_backward(grad_out, flow, indexing, mode, padding_mode)
    g_flow = None
    if ctx.needs_flow and ctx.needs_input_grad[1]:
        # the derivative of the bilinear taps with respect to the sampling position (csrc/image_warp.hip,
        # WARP_POSITION): what the reference's graph differentiates through grid_sample's grid (:436)
        g_flow = torch.ops.pydrobert_amd.dense_image_warp_flow_backward(
            grad_out, ctx.saved_tensors[1], flow, indexing, mode, padding_mode
        )
    return g, g_flow, None, None, None


def _dense_flow_grad_torch(grad_out, image, flow, indexing, mode, padding_mode):
    """The flow's gradient through torch's own grid_sample adjoint on the device, in float32 whatever the
    image's type: not on any operator's path -- the other contestant of profiles/tools/time_warp_grads.py."""
    with torch.enable_grad():
        fl = flow.detach().float().requires_grad_(True)
        grid = _sampling_grid_from_flow(fl, indexing, image.shape[2], image.shape[3])
        out = torch.nn.functional.grid_sample(
            image.detach().float(), grid, mode=mode, padding_mode=padding_mode, align_corners=False
        )
        (g_flow,) = torch.autograd.grad(out, fl, grad_out.float())
    return g_flow.to(flow.dtype)


@custom_op("pydrobert_amd::dense_image_warp_flow_backward", mutates_args=())
def _dense_image_warp_flow_backward_op(
    grad_out: torch.Tensor, image: torch.Tensor, flow: torch.Tensor, indexing: str, mode: str, padding_mode: str
) -> torch.Tensor:
    """Gradient of ``dense_image_warp`` with respect to the flow (csrc/image_warp.hip, WARP_POSITION), in
    the image's type from the grid on, like the forward."""
    device = _cabi.require_hip(grad_out, image, flow)
    N, C, H, W = image.shape
    if mode == "nearest":  # (piecewise constant in the flow: no launch)
        return torch.zeros_like(flow)
    (img, sfx), fl = _pixels(image), _f32c(flow)
    g = grad_out.detach().to(img.dtype).contiguous()
    with torch.cuda.device(device):
        grad = torch.empty((N, H, W, 2), device=device, dtype=torch.float)
        rc = getattr(_cabi.lib(), "pdt_dense_image_warp_flow_backward" + sfx)(
            _cabi.ptr(g), _cabi.ptr(img), _cabi.ptr(fl), N, C, H, W, int(indexing == "hw"), _MODES[mode],
            _PADDINGS[padding_mode], _cabi.ptr(grad), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_dense_image_warp_flow_backward")
    return grad.to(flow.dtype)


@_dense_image_warp_flow_backward_op.register_fake
def _(grad_out, image, flow, indexing, mode, padding_mode):
    return flow.new_empty(flow.shape)


def _no_double_backward(ctx, *grads):
    raise RuntimeError(
        "pydrobert_amd image warps: double backward is not supported (the gradient kernels are not differentiable)"
    )


def _setup_nothing(ctx, inputs, output):
    pass


register_autograd(
    "pydrobert_amd::dense_image_warp", _dense_backward, setup_context=_dense_setup_context
)
register_autograd("pydrobert_amd::dense_image_warp_flow_backward", _no_double_backward, setup_context=_setup_nothing)
register_autograd("pydrobert_amd::spline_eval_adjoint", _no_double_backward, setup_context=_setup_nothing)


def dense_image_warp(
    image: torch.Tensor,
    flow: torch.Tensor,
    indexing: str = "hw",
    mode: str = "bilinear",
    padding_mode: str = "border",
) -> torch.Tensor:
    """Functional version of :class:`DenseImageWarp` (reference _img.py:393-439):
    ``output[n, c, h, w] = image[n, c, h - flow[n, h, w, 0], w - flow[n, h, w, 1]]``."""
    return torch.ops.pydrobert_amd.dense_image_warp(image, flow, indexing, mode, padding_mode)


@functools.lru_cache(maxsize=16)
def _pinned_points_const(k: int, W: int, H: int, device: torch.device) -> torch.Tensor:
    """(4 k, 2) boundary points for one image size -- constants of (k, W, H): built once per device
    instead of with a dozen small launches in every call (read only; never modified in place)."""
    return _pinned_points(k, W, H, 1, device)[0].contiguous()


@functools.lru_cache(maxsize=16)
def _wh_const(W: int, H: int, device: torch.device) -> torch.Tensor:
    """[W, H] as a device constant (a host-to-device copy per call otherwise)."""
    return torch.tensor([W, H], dtype=torch.float, device=device)


def _pinned_points(k: int, W: int, H: int, N: int, device) -> torch.Tensor:
    # reference _img.py:244-265, points in (x=w, y=h) order
    r = torch.linspace(0.0, 1.0, k + 1, device=device)
    wr, hr = (W - 1) * r, (H - 1) * r
    z = torch.zeros_like(r)
    pts = torch.cat(
        [
            torch.stack([wr, z], 1),
            torch.stack([z[1:-1], hr[1:-1]], 1),
            torch.stack([wr, torch.full_like(r, H - 1.0)], 1),
            torch.stack([torch.full_like(r, W - 1.0)[1:-1], hr[1:-1]], 1),
        ],
        0,
    )
    return pts.unsqueeze(0).expand(N, -1, -1)


def _sparse_prepare(image, source_points, dest_points, indexing, pinned_boundary_points,
                    include_flow):  # fmt: skip
    """(device, points, values, M') in the C ABI's conventions: (x=w, y=h) order, pinned
    boundary points appended, values = dest - source (flow form) or the normalised source grid."""
    if indexing not in _INDEXINGS:
        raise ValueError("Invalid indexing! must be one of 'wh' or 'hw'")
    if image.dim() != 4:
        raise RuntimeError("image must be 4 dimensional")
    device = _cabi.require_hip(image, source_points, dest_points)
    N, C, H, W = image.shape
    src, dst = source_points.detach().float(), dest_points.detach().float()
    if indexing == "hw":
        src, dst = src.flip(-1), dst.flip(-1)
    if src.shape[1] == 0:
        return device, None, None, 0
    if pinned_boundary_points > 0:
        pp = _pinned_points_const(pinned_boundary_points, W, H, device).unsqueeze(0).expand(N, -1, -1)
        src, dst = torch.cat([src, pp], 1), torch.cat([dst, pp], 1)
    Mp = src.shape[1]
    if include_flow:
        vals = dst - src  # :561-562
    else:
        vals = (2.0 * src + 1.0) / _wh_const(W, H, device) - 1.0  # :633
    return device, dst.contiguous(), vals.contiguous(), Mp


@custom_op("pydrobert_amd::sparse_image_warp", mutates_args=())
def _sparse_image_warp_op(
    image: torch.Tensor,
    source_points: torch.Tensor,
    dest_points: torch.Tensor,
    indexing: str,
    field_interpolation_order: int,
    field_regularization_weight: float,
    pinned_boundary_points: int,
    dense_interpolation_mode: str,
    dense_padding_mode: str,
    include_flow: bool,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(warped, flow); ``flow`` is an empty tensor unless ``include_flow``.  Differentiable
    with respect to ``image``."""
    device, pts, vals, Mp = _sparse_prepare(
        image, source_points, dest_points, indexing, pinned_boundary_points, include_flow
    )
    N, C, H, W = image.shape
    if Mp == 0:  # :543-548
        return image.clone(), torch.zeros(
            (N, H, W, 2) if include_flow else (0,), dtype=torch.float, device=device
        )
    img, sfx = _pixels(image)
    L = _cabi.lib()
    with torch.cuda.device(device):
        out = torch.empty_like(img)
        flow = torch.empty((N, H, W, 2) if include_flow else (0,), device=device, dtype=torch.float)
        ws = torch.empty((int(L.pdt_spline_workspace_bytes(N, Mp, 2, 2)),), device=device, dtype=torch.uint8)
        rc = getattr(L, "pdt_sparse_image_warp" + sfx)(
            _cabi.ptr(img), _cabi.ptr(pts), _cabi.ptr(vals), N, C, H, W, Mp,
            int(field_interpolation_order), float(field_regularization_weight),
            int(not include_flow), _MODES[dense_interpolation_mode], _PADDINGS[dense_padding_mode],
            _cabi.ptr(out), _cabi.ptr(flow) if include_flow else None, int(indexing == "hw"),
            _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_sparse_image_warp")
    return out.to(image.dtype), flow


@custom_op("pydrobert_amd::sparse_image_warp_backward", mutates_args=())
def _sparse_image_warp_backward_op(
    grad_out: torch.Tensor,
    source_points: torch.Tensor,
    dest_points: torch.Tensor,
    indexing: str,
    field_interpolation_order: int,
    field_regularization_weight: float,
    pinned_boundary_points: int,
    dense_interpolation_mode: str,
    dense_padding_mode: str,
    include_flow: bool,
) -> torch.Tensor:
    """Adjoint of ``sparse_image_warp`` with respect to the image."""
    device, pts, vals, Mp = _sparse_prepare(
        grad_out, source_points, dest_points, indexing, pinned_boundary_points, include_flow
    )
    if Mp == 0:
        return grad_out.clone()
    g, sfx = _pixels(grad_out)
    N, C, H, W = g.shape
    L = _cabi.lib()
    with torch.cuda.device(device):
        grad = torch.empty_like(g)
        ws = torch.empty((int(L.pdt_spline_workspace_bytes(N, Mp, 2, 2)),), device=device, dtype=torch.uint8)
        rc = getattr(L, "pdt_sparse_image_warp_backward" + sfx)(
            _cabi.ptr(g), _cabi.ptr(pts), _cabi.ptr(vals), N, C, H, W, Mp,
            int(field_interpolation_order), float(field_regularization_weight),
            int(not include_flow), _MODES[dense_interpolation_mode], _PADDINGS[dense_padding_mode],
            _cabi.ptr(grad), _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_sparse_image_warp_backward")
    return grad.to(grad_out.dtype)


@_sparse_image_warp_backward_op.register_fake
def _(grad_out, source_points, dest_points, indexing, field_interpolation_order,
      field_regularization_weight, pinned_boundary_points, dense_interpolation_mode,
      dense_padding_mode, include_flow):  # fmt: skip
    return grad_out.new_empty(grad_out.shape)


def _sparse_setup_context(ctx, inputs, output):
    ctx.points_need_grad = inputs[1].requires_grad or inputs[2].requires_grad
    if ctx.points_need_grad:
        ctx.save_for_backward(inputs[1], inputs[2], inputs[0])
    else:
        ctx.save_for_backward(inputs[1], inputs[2])
    ctx.cfg = tuple(inputs[3:])


def _sparse_backward(ctx, grad_warped, grad_flow):
    source_points, dest_points = ctx.saved_tensors[:2]
    g = None
    if ctx.needs_input_grad[0]:
        g = torch.ops.pydrobert_amd.sparse_image_warp_backward(
            grad_warped, source_points, dest_points, *ctx.cfg
        )
    g_src = g_dst = None
    if ctx.points_need_grad and source_points.shape[1]:
        # control points: the gather's position derivative chained into the spline's adjoint, as the
        # reference's graph does (_img.py:561-585, :633-655)
        include_flow = ctx.cfg[-1]
        g_src, g_dst = torch.ops.pydrobert_amd.sparse_image_warp_points_backward(
            grad_warped, grad_flow if include_flow else None, ctx.saved_tensors[2], source_points, dest_points,
            *ctx.cfg
        )
    return (g, g_src, g_dst) + (None,) * 7


def _sparse_points_grad_torch(grad_warped, grad_flow, image, source_points, dest_points, indexing, order, reg,
                              pinned, mode, padding, include_flow):  # fmt: skip
    """The control points' gradients by autograd through the spline at every pixel and torch's grid_sample
    on the device (float32): not on any operator's path -- the other contestant of
    profiles/tools/time_warp_grads.py.  Its spline backward takes the torch sums over (N, H*W, T, 2)."""
    N, C, H, W = image.shape
    with torch.enable_grad():
        s0 = source_points.detach().float().requires_grad_(True)
        d0 = dest_points.detach().float().requires_grad_(True)
        src, dst = (s0.flip(-1), d0.flip(-1)) if indexing == "hw" else (s0, d0)
        if pinned > 0:
            pp = _pinned_points(pinned, W, H, N, image.device)
            src, dst = torch.cat([src, pp], 1), torch.cat([dst, pp], 1)
        query = _pixel_lattice(N, H, W, image.device)
        size = torch.tensor([W, H], dtype=torch.float, device=image.device)
        vals = dst - src if include_flow else (2.0 * src + 1.0) / size - 1.0
        c, f = dst.detach().contiguous(), vals.detach().contiguous()
        sol = _spline_solve(c, f, None, order, reg)
        out = torch.ops.pydrobert_amd.polyharmonic_spline(c, f, query, order, reg).view(N, H, W, 2)
        out.requires_grad_(True)
        outs, grads = [], []
        if include_flow:
            grid = _sampling_grid_from_flow(out, "wh", H, W)
            if grad_flow is not None:
                outs.append(out.flip(-1) if indexing == "hw" else out)
                grads.append(grad_flow.float())
        else:
            grid = out
        warped = torch.nn.functional.grid_sample(
            image.detach().float(), grid, mode=mode, padding_mode=padding, align_corners=False
        )
        outs.append(warped)
        grads.append(grad_warped.float())
        (G,) = torch.autograd.grad(outs, [out], grads)
        g_sol, g_c, _ = _spline_eval_adjoint_torch(G.reshape(N, H * W, 2), c, sol, query, order, False)
        g_sys, g_f = _spline_system_adjoint(c, sol, g_sol, order, reg)
        g_src, g_dst = torch.autograd.grad([dst, vals], [s0, d0], [(g_c + g_sys).float(), g_f.float()],
                                           allow_unused=True)  # fmt: skip
    g_src = torch.zeros_like(source_points) if g_src is None else g_src.to(source_points.dtype)
    g_dst = torch.zeros_like(dest_points) if g_dst is None else g_dst.to(dest_points.dtype)
    return g_src, g_dst


@custom_op("pydrobert_amd::sparse_image_warp_points_backward", mutates_args=())
def _sparse_image_warp_points_backward_op(
    grad_warped: torch.Tensor,
    grad_flow: Optional[torch.Tensor],
    image: torch.Tensor,
    source_points: torch.Tensor,
    dest_points: torch.Tensor,
    indexing: str,
    field_interpolation_order: int,
    field_regularization_weight: float,
    pinned_boundary_points: int,
    dense_interpolation_mode: str,
    dense_padding_mode: str,
    include_flow: bool,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gradients of ``sparse_image_warp`` with respect to ``(source_points, dest_points)``: one solve, the
    position-gradient kernel (csrc/image_warp.hip, WARP_POSITION; ``grad_flow``, the gradient of the
    returned flow, is added there), the spline evaluation's adjoint over the pixel lattice
    (csrc/spline.hip: pdt_spline_eval_adjoint), one adjoint solve, the (T, T) system terms, and the chain
    back through the spline's values, the pinned points (no gradient) and ``indexing``."""
    order, reg = int(field_interpolation_order), float(field_regularization_weight)
    device, pts, vals, Mp = _sparse_prepare(
        image, source_points, dest_points, indexing, pinned_boundary_points, include_flow
    )
    M = source_points.shape[1]
    if Mp == 0:
        return torch.zeros_like(source_points), torch.zeros_like(dest_points)
    N, C, H, W = image.shape
    if grad_flow is not None and not include_flow:
        raise RuntimeError("grad_flow needs include_flow")
    if dense_interpolation_mode == "nearest" and grad_flow is None:  # (no sample moves with its position)
        return torch.zeros_like(source_points), torch.zeros_like(dest_points)
    img, sfx = _pixels(image)
    g = grad_warped.detach().to(img.dtype).contiguous()
    gf = None if grad_flow is None else _f32c(grad_flow)
    L = _cabi.lib()
    sol = _spline_solve(pts, vals, None, order, reg)  # (N, Mp + 3, 2)
    with torch.cuda.device(device):
        G = torch.empty((N, H, W, 2), device=device, dtype=torch.float)
        ws = torch.empty((int(L.pdt_spline_workspace_bytes(N, Mp, 2, 2)),), device=device, dtype=torch.uint8)
        rc = getattr(L, "pdt_sparse_image_warp_position_backward" + sfx)(
            _cabi.ptr(g), _cabi.ptr(img), _cabi.ptr(pts), _cabi.ptr(sol), N, C, H, W, Mp, order,
            int(not include_flow), _MODES[dense_interpolation_mode], _PADDINGS[dense_padding_mode],
            _cabi.ptr(gf), int(indexing == "hw"), _cabi.ptr(G), _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_sparse_image_warp_position_backward")
    g_sol, g_c, _ = _spline_eval_adjoint(G.view(N, H * W, 2), pts, sol, None, H, W, order, False)
    g_sys, g_f = _spline_system_adjoint(pts, sol, g_sol, order, reg)
    g_c = (g_c + g_sys)[:, :M]  # (the pinned points are constants)
    g_f = g_f[:, :M]
    if include_flow:  # values = dst - src
        g_src, g_dst = -g_f, g_c + g_f
    else:  # values = (2 src + 1) / size - 1
        g_src, g_dst = g_f * (2.0 / _wh_const(W, H, device).double()), g_c
    if indexing == "hw":
        g_src, g_dst = g_src.flip(-1), g_dst.flip(-1)
    return g_src.to(source_points.dtype).contiguous(), g_dst.to(dest_points.dtype).contiguous()


@_sparse_image_warp_points_backward_op.register_fake
def _(grad_warped, grad_flow, image, source_points, dest_points, indexing, field_interpolation_order,
      field_regularization_weight, pinned_boundary_points, dense_interpolation_mode, dense_padding_mode,
      include_flow):  # fmt: skip
    return torch.empty_like(source_points), torch.empty_like(dest_points)


register_autograd(
    "pydrobert_amd::sparse_image_warp", _sparse_backward, setup_context=_sparse_setup_context
)
register_autograd(
    "pydrobert_amd::sparse_image_warp_points_backward", _no_double_backward, setup_context=_setup_nothing
)


@_sparse_image_warp_op.register_fake
def _(image, source_points, dest_points, indexing, field_interpolation_order,
      field_regularization_weight, pinned_boundary_points, dense_interpolation_mode,
      dense_padding_mode, include_flow):  # fmt: skip
    N, _, H, W = image.shape
    return (
        image.new_empty(image.shape),
        image.new_empty((N, H, W, 2) if include_flow else (0,), dtype=torch.float),
    )


def sparse_image_warp(
    image: torch.Tensor,
    source_points: torch.Tensor,
    dest_points: torch.Tensor,
    indexing: str = "hw",
    field_interpolation_order: int = 2,
    field_regularization_weight: float = 0.0,
    field_full_matrix: bool = True,
    pinned_boundary_points: int = 0,
    dense_interpolation_mode: str = "bilinear",
    dense_padding_mode: str = "border",
    include_flow: bool = True,
) -> Any:
    """Functional version of :class:`SparseImageWarp` (reference _img.py:520-714).

    The spline over the control points is evaluated per pixel inside the gather kernel; the
    dense flow field is only written when ``include_flow``.
    """
    warped, flow = torch.ops.pydrobert_amd.sparse_image_warp(
        image, source_points, dest_points, indexing, field_interpolation_order,
        field_regularization_weight, pinned_boundary_points, dense_interpolation_mode,
        dense_padding_mode, include_flow,
    )  # fmt: skip
    if include_flow:
        return warped, flow
    else:
        return warped


def _spec_augment_check_shapes(feats: torch.Tensor, lengths: Optional[torch.Tensor] = None):
    # reference _img.py:1020-1036 (what the host can decide)
    if feats.dim() != 3:
        raise RuntimeError("Expected feats to have three dimensions, got {}".format(feats.dim()))
    N = feats.size(0)
    if lengths is not None:
        if lengths.dim() != 1:
            raise RuntimeError("Expected lengths to be one dimensional, got {}".format(lengths.dim()))
        if lengths.size(0) != N:
            raise RuntimeError(
                "Batch dimension of feats ({}) and lengths ({}) do not match".format(N, lengths.size(0))
            )


def _spec_augment_lengths_ok(feats: torch.Tensor, lengths: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The data-dependent part of the reference's input check (_img.py:1037-1041), LAUNCHED here and read
    by ``_spec_augment_raise_unless`` after the operator's own kernels have been launched: the host's
    wait for the verdict then overlaps the work instead of standing in front of it (0.34 -> 0.29 ms per
    ``apply_parameters`` at N=2048 x 1000 x 80).  Safe because no kernel of the path indexes with a
    length: out-of-range lengths only move clamped knots, and the result is dropped when this raises."""
    if lengths is None:
        return None
    ok = torch.all((lengths <= feats.size(1)) & (lengths > 0))
    if not lengths.is_cuda:  # (nothing to overlap: the verdict is there; host tensors are refused further on)
        _spec_augment_raise_unless(ok, feats.size(1))
        return None
    return ok


def _spec_augment_raise_unless(ok: Optional[torch.Tensor], T: int):
    if ok is not None and not bool(ok):
        raise RuntimeError("values of lengths must be between (1, {})".format(T))


def _spec_augment_check_input(feats: torch.Tensor, lengths: Optional[torch.Tensor] = None):
    # reference _img.py:1020-1041
    _spec_augment_check_shapes(feats, lengths)
    _spec_augment_raise_unless(_spec_augment_lengths_ok(feats, lengths), feats.size(1))


def _lens_long(lengths: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """``lengths`` as the kernels read them: contiguous int64, detached (or None)."""
    if lengths is None:
        return None
    lens = lengths.detach()
    if lens.dtype != torch.long or not lens.is_contiguous():
        lens = lens.long().contiguous()
    return lens


def _full_lengths(N: int, T: int, device: torch.device) -> torch.Tensor:
    """The lengths of a batch given without any: every utterance spans the whole axis."""
    return torch.full((N,), T, dtype=torch.long, device=device)


def _masks_enabled(max_time_mask: int, max_time_mask_proportion: float, num_time_mask: int,
                   num_time_mask_proportion: float, max_freq_mask: int, num_freq_mask: int) -> Tuple[bool, bool]:  # fmt: skip
    """``(tm, fm)``: does the configuration draw time / frequency masks at all (reference _img.py:1099, :1127)."""
    tm = max_time_mask != 0 and max_time_mask_proportion != 0.0 and num_time_mask != 0 and num_time_mask_proportion != 0.0
    fm = max_freq_mask != 0 and num_freq_mask != 0
    return tm, fm


def _mask_counts(t_0: Optional[torch.Tensor], f_0: Optional[torch.Tensor]) -> Tuple[int, int]:
    """``(mt, mf)``: masks per utterance along time and frequency (None: no masks)."""
    return (0 if t_0 is None else t_0.shape[1]), (0 if f_0 is None else f_0.shape[1])


@custom_op("pydrobert_amd::spec_augment_draw", mutates_args=())
def _spec_augment_draw_op(
    uniforms: torch.Tensor,
    lengths: Optional[torch.Tensor],
    T: int,
    F: int,
    max_time_warp: float,
    max_freq_warp: float,
    max_time_mask: int,
    max_freq_mask: int,
    max_time_mask_proportion: float,
    num_time_mask: int,
    num_time_mask_proportion: float,
    num_freq_mask: int,
    is_double: bool,
) -> List[torch.Tensor]:
    """Every SpecAugment parameter from one ``(N, R)`` tensor of uniform draws, in ONE kernel
    (csrc/spec_augment.hip: spec_augment_draw_kernel; reference _img.py:1082-1137, which spends ~35 tiny
    launches on it).  Returns ``[w_0, w, v_0, v, t_0, t, f_0, f]``; groups the configuration disables
    come back with zero elements."""
    device = _cabi.require_hip(uniforms, lengths)
    N = uniforms.size(0)
    u = uniforms.detach()
    if u.dtype != torch.float or not u.is_contiguous():
        u = u.float().contiguous()
    tw, fw = max_time_warp != 0.0, max_freq_warp != 0.0
    tm, fm = _masks_enabled(max_time_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion,
                            max_freq_mask, num_freq_mask)
    lens = _lens_long(lengths)
    with torch.cuda.device(device):
        fl = [torch.empty((N if on else 0,), device=device, dtype=torch.float) for on in (tw, tw, fw, fw)]
        tt = [torch.empty((N, num_time_mask) if tm else (0,), device=device, dtype=torch.long) for _ in range(2)]
        ff = [torch.empty((N, num_freq_mask) if fm else (0,), device=device, dtype=torch.long) for _ in range(2)]
        rc = _cabi.lib().pdt_spec_augment_draw(
            _cabi.ptr(u), N, u.size(1), _cabi.ptr(lens), T, F, float(max_time_warp), float(max_freq_warp),
            int(max_time_mask), int(max_freq_mask), float(max_time_mask_proportion), int(num_time_mask),
            float(num_time_mask_proportion), int(num_freq_mask), int(is_double),
            _cabi.ptr(fl[0]), _cabi.ptr(fl[1]), _cabi.ptr(fl[2]), _cabi.ptr(fl[3]),
            _cabi.ptr(tt[0]), _cabi.ptr(tt[1]), _cabi.ptr(ff[0]), _cabi.ptr(ff[1]), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_spec_augment_draw")
    return fl + tt + ff


@_spec_augment_draw_op.register_fake
def _(uniforms, lengths, T, F, max_time_warp, max_freq_warp, max_time_mask, max_freq_mask,
      max_time_mask_proportion, num_time_mask, num_time_mask_proportion, num_freq_mask, is_double):  # fmt: skip
    N = uniforms.shape[0]
    tw, fw = max_time_warp != 0.0, max_freq_warp != 0.0
    tm, fm = _masks_enabled(max_time_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion,
                            max_freq_mask, num_freq_mask)
    fl = [uniforms.new_empty((N if on else 0,), dtype=torch.float) for on in (tw, tw, fw, fw)]
    tt = [uniforms.new_empty((N, num_time_mask) if tm else (0,), dtype=torch.long) for _ in range(2)]
    ff = [uniforms.new_empty((N, num_freq_mask) if fm else (0,), dtype=torch.long) for _ in range(2)]
    return fl + tt + ff


def spec_augment_draw_parameters(
    feats: torch.Tensor,
    max_time_warp: float,
    max_freq_warp: float,
    max_time_mask: int,
    max_freq_mask: int,
    max_time_mask_proportion: float,
    num_time_mask: int,
    num_time_mask_proportion: float,
    num_freq_mask: int,
    lengths: Optional[torch.Tensor] = None,
) -> SpecAugmentParams:
    """Functional version of :func:`SpecAugment.draw_parameters` (reference _img.py:1056-1139).

    ONE ``torch.rand`` call on ``feats.device`` (a column per draw, in the reference's order w_0, w,
    v_0, v, t, t_0, f, f_0) and one kernel that turns every uniform into its parameter with the
    reference's float32 expressions -- instead of six ``rand`` calls and ~30 tensor ops (0.2-0.5 ms of
    launches at N = 2048).  Disabled groups return ``torch.empty(0)`` pairs like the reference's.
    """
    return _spec_augment_draw(
        feats, max_time_warp, max_freq_warp, max_time_mask, max_freq_mask, max_time_mask_proportion, num_time_mask,
        num_time_mask_proportion, num_freq_mask, lengths, True,
    )  # fmt: skip


def _spec_augment_draw(
    feats: torch.Tensor,
    max_time_warp: float,
    max_freq_warp: float,
    max_time_mask: int,
    max_freq_mask: int,
    max_time_mask_proportion: float,
    num_time_mask: int,
    num_time_mask_proportion: float,
    num_freq_mask: int,
    lengths: Optional[torch.Tensor],
    check: bool,
) -> SpecAugmentParams:
    ok: Optional[torch.Tensor] = None
    if check:
        _spec_augment_check_shapes(feats, lengths)
        ok = _spec_augment_lengths_ok(feats, lengths)
    N, T, F = feats.size(0), feats.size(1), feats.size(2)
    device = feats.device
    tw, fw = max_time_warp != 0.0, max_freq_warp != 0.0
    tm, fm = _masks_enabled(max_time_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion,
                            max_freq_mask, num_freq_mask)
    R = 2 * int(tw) + 2 * int(fw) + (2 * num_time_mask if tm else 0) + (2 * num_freq_mask if fm else 0)
    none = torch.empty(0)  # a disabled group: the reference's ``torch.empty(0)`` pair (_img.py:1093-1139)
    if R == 0 or N == 0:  # nothing is drawn: no kernel (and no device) is needed
        if N == 0 and R > 0:
            z, zl = feats.new_empty((0,), dtype=torch.float), feats.new_empty((0, 0), dtype=torch.long)
            _spec_augment_raise_unless(ok, T)
            return (z if tw else none, z if tw else none, z if fw else none, z if fw else none,
                    zl.new_empty((0, num_time_mask)) if tm else none, zl.new_empty((0, num_time_mask)) if tm else none,
                    zl.new_empty((0, num_freq_mask)) if fm else none, zl.new_empty((0, num_freq_mask)) if fm else none)  # fmt: skip
        _spec_augment_raise_unless(ok, T)
        return none, none, none, none, none, none, none, none
    uniforms = torch.rand((N, R), device=device)
    lens = None if lengths is None else lengths.to(device)
    out = torch.ops.pydrobert_amd.spec_augment_draw(
        uniforms, lens, T, F, max_time_warp, max_freq_warp, max_time_mask, max_freq_mask, max_time_mask_proportion,
        num_time_mask, num_time_mask_proportion, num_freq_mask, feats.dtype == torch.double,
    )  # fmt: skip
    _spec_augment_raise_unless(ok, T)
    return (out[0] if tw else none, out[1] if tw else none, out[2] if fw else none, out[3] if fw else none,
            out[4] if tm else none, out[5] if tm else none, out[6] if fm else none, out[7] if fm else none)  # fmt: skip


# float16 / bfloat16 features go to the kernels as they are (include/pdt_amd.h: the ``_elem`` entry points'
# element codes); the arithmetic is float32 and a result is rounded once where it is stored
_HALF_ELEM = {torch.float16: 2, torch.bfloat16: 3}


def _spec_feats(feats: torch.Tensor) -> Tuple[torch.Tensor, Optional[int]]:
    """``(x, elem)``: the detached features the application kernels read, with their own strides -- float16 /
    bfloat16 untouched with their element code, float32 untouched with None (the entry points without the
    suffix), anything else as float32."""
    x = feats.detach()
    elem = _HALF_ELEM.get(x.dtype)
    if elem is None and x.dtype != torch.float:
        x = x.float()
    return x, elem


def _has(a: Optional[torch.Tensor], b: Optional[torch.Tensor]) -> bool:
    return a is not None and a.numel() > 0 and b is not None and b.numel() > 0


@custom_op("pydrobert_amd::spec_augment_apply", mutates_args=())
def _spec_augment_apply_op(
    feats: torch.Tensor,
    tgrid: Optional[torch.Tensor],
    fgrid: Optional[torch.Tensor],
    t_0: Optional[torch.Tensor],
    t: Optional[torch.Tensor],
    f_0: Optional[torch.Tensor],
    f: Optional[torch.Tensor],
) -> torch.Tensor:
    """Time / frequency resampling through the 1-D grids, then band masks: ONE pass over
    ``feats`` (csrc/spec_augment.hip)."""
    device = _cabi.require_hip(feats, tgrid, fgrid, t_0, t, f_0, f)
    N, T, F = feats.shape
    x, elem = _spec_feats(feats)
    mt, mf = _mask_counts(t_0, f_0)
    with torch.cuda.device(device):
        out = torch.empty((N, T, F), device=device, dtype=x.dtype)
        args = (
            _cabi.ptr(x), N, T, F, x.stride(0), x.stride(1), x.stride(2),
            _cabi.ptr(tgrid), _cabi.ptr(fgrid), _cabi.ptr(t_0), _cabi.ptr(t), mt,
            _cabi.ptr(f_0), _cabi.ptr(f), mf, _cabi.ptr(out), _cabi.stream_ptr(device),
        )  # fmt: skip
        if elem is None:
            rc = _cabi.lib().pdt_spec_augment_apply(*args)
        else:
            rc = _cabi.lib().pdt_spec_augment_apply_elem(*args, elem)
    _cabi.check(rc, "pdt_spec_augment_apply")
    return out.to(feats.dtype)


@_spec_augment_apply_op.register_fake
def _(feats, tgrid, fgrid, t_0, t, f_0, f):
    return feats.new_empty(feats.shape)


@custom_op("pydrobert_amd::spec_augment_apply_backward", mutates_args=())
def _spec_augment_apply_backward_op(
    grad_out: torch.Tensor,
    tgrid: Optional[torch.Tensor],
    fgrid: Optional[torch.Tensor],
    t_0: Optional[torch.Tensor],
    t: Optional[torch.Tensor],
    f_0: Optional[torch.Tensor],
    f: Optional[torch.Tensor],
) -> torch.Tensor:
    """Adjoint of ``spec_augment_apply`` with respect to the features (masked positions carry
    no gradient; the others scatter theirs to their taps)."""
    device = _cabi.require_hip(grad_out, tgrid, fgrid, t_0, t, f_0, f)
    elem = _HALF_ELEM.get(grad_out.dtype)
    g = _f32c(grad_out) if elem is None else grad_out.detach().contiguous()
    N, T, F = g.shape
    mt, mf = _mask_counts(t_0, f_0)
    L = _cabi.lib()
    with torch.cuda.device(device):
        grad = torch.empty_like(g)
        args = (
            _cabi.ptr(g), N, T, F, _cabi.ptr(tgrid), _cabi.ptr(fgrid), _cabi.ptr(t_0),
            _cabi.ptr(t), mt, _cabi.ptr(f_0), _cabi.ptr(f), mf, _cabi.ptr(grad),
            _cabi.stream_ptr(device),
        )  # fmt: skip
        if elem is None:
            rc = L.pdt_spec_augment_apply_backward(*args)
        else:
            # (sums of several taps are float32: the scatter form accumulates in a workspace and rounds once)
            ws = None
            if (tgrid is not None or fgrid is not None) and g.numel() and L.pdt_spec_augment_apply_form(
                N, T, F, T * F, F, 1, g.data_ptr(), grad.data_ptr(), int(tgrid is not None), int(fgrid is not None),
                1, elem,
            ) == 0:  # fmt: skip
                ws = torch.empty((N, T, F), device=device, dtype=torch.float)
            rc = L.pdt_spec_augment_apply_backward_elem(*args, elem, _cabi.ptr(ws), 0 if ws is None else 4 * ws.numel())
    _cabi.check(rc, "pdt_spec_augment_apply_backward")
    return grad.to(grad_out.dtype)


@_spec_augment_apply_backward_op.register_fake
def _(grad_out, tgrid, fgrid, t_0, t, f_0, f):
    return grad_out.new_empty(grad_out.shape)


def _launch_apply_warp(device, x, src, flow, lens, order, t_0, t, mt, f_0, f, mf, check_lengths) -> Optional[torch.Tensor]:
    """One launch of ``pdt_spec_augment_apply_warp`` (``_elem`` for half features) on ``x``: the result, or None for a
    layout the one-pass kernel does not take (the caller goes through the grid).

    ``check_lengths``: the reference's "values of lengths must be between (1, T)" (_img.py:1037-1041)
    decided by the kernel that reads the lengths -- a word in pinned host memory, looked at once the
    stream has drained -- instead of four small kernels, a copy and a synchronisation in front of it."""
    N, T, F = x.shape
    report = _cabi.host_report(device) if (check_lengths and lens is not None) else None
    with torch.cuda.device(device):
        out = torch.empty((N, T, F), device=device, dtype=x.dtype)
        args = (
            _cabi.ptr(x), N, T, F, x.stride(0), x.stride(1), x.stride(2), _cabi.ptr(src), _cabi.ptr(flow),
            _cabi.ptr(lens), int(order), _cabi.ptr(t_0), _cabi.ptr(t), mt, _cabi.ptr(f_0), _cabi.ptr(f), mf,
            _cabi.ptr(out), 0 if report is None else report.ptr, _cabi.stream_ptr(device),
        )  # fmt: skip
        if x.dtype == torch.float:
            rc = _cabi.lib().pdt_spec_augment_apply_warp(*args)
        else:
            rc = _cabi.lib().pdt_spec_augment_apply_warp_elem(*args, _HALF_ELEM[x.dtype])
    if report is not None and (rc or not (N and T and F)):
        report.disarm()  # (no kernel was launched)
    if rc == _cabi.PDT_E_UNSUPPORTED:
        return None
    _cabi.check(rc, "pdt_spec_augment_apply_warp")
    if report is not None and N and T and F:
        torch.cuda.current_stream(device).synchronize()
        if report.read() != 0:
            raise RuntimeError("values of lengths must be between (1, {})".format(T))
    return out


@custom_op("pydrobert_amd::spec_augment_apply_warp", mutates_args=())
def _spec_augment_apply_warp_op(
    feats: torch.Tensor,
    w_0: torch.Tensor,
    w: torch.Tensor,
    lengths: Optional[torch.Tensor],
    interpolation_order: int,
    t_0: Optional[torch.Tensor],
    t: Optional[torch.Tensor],
    f_0: Optional[torch.Tensor],
    f: Optional[torch.Tensor],
    check_lengths: bool = False,
) -> torch.Tensor:
    """``spec_augment_apply`` with the time warp given by its parameters ``(w_0, w, lengths)``: the
    three-knot spline of ``warp_1d_grid`` is solved in closed form inside the one pass over ``feats``
    (csrc/img_sample.hpp: warp_1d_spline) -- one launch, no ``(N, T)`` grid, one operator instead of two.
    Layouts the one-pass kernel does not take go through the grid as before."""
    device = _cabi.require_hip(feats, w_0, w, lengths, t_0, t, f_0, f)
    N, T, F = feats.shape
    x, _ = _spec_feats(feats)
    src, flow = _f32c(w_0), _f32c(w)
    lens = _lens_long(lengths)
    mt, mf = _mask_counts(t_0, f_0)
    out = _launch_apply_warp(device, x, src, flow, lens, interpolation_order, t_0, t, mt, f_0, f, mf, check_lengths)
    if out is None:
        if check_lengths and lens is not None:
            _spec_augment_raise_unless(torch.all((lens <= T) & (lens > 0)), T)
        ln = lens if lens is not None else _full_lengths(N, T, device)
        tgrid = torch.ops.pydrobert_amd.warp_1d_grid(src, flow, ln, T, interpolation_order)
        return torch.ops.pydrobert_amd.spec_augment_apply(feats, tgrid, None, t_0, t, f_0, f)
    return out.to(feats.dtype)


@_spec_augment_apply_warp_op.register_fake
def _(feats, w_0, w, lengths, interpolation_order, t_0, t, f_0, f, check_lengths=False):
    return feats.new_empty(feats.shape)


def _spec_warp_setup_context(ctx, inputs, output):
    ctx.args = tuple(inputs[1:])
    ctx.T = inputs[0].shape[1]


def _spec_warp_backward(ctx, grad_out):
    # (the adjoint reads the grid: formed here, where a gradient is actually asked for)
    w_0, w, lengths, order, t_0, t, f_0, f = ctx.args[:8]
    ln = lengths if lengths is not None else _full_lengths(w_0.shape[0], ctx.T, w_0.device)
    tgrid = torch.ops.pydrobert_amd.warp_1d_grid(w_0.detach(), w.detach(), ln, ctx.T, order)
    g = torch.ops.pydrobert_amd.spec_augment_apply_backward(grad_out, tgrid, None, t_0, t, f_0, f)
    return g, None, None, None, None, None, None, None, None, None


register_autograd(
    "pydrobert_amd::spec_augment_apply_warp", _spec_warp_backward, setup_context=_spec_warp_setup_context
)


@custom_op("pydrobert_amd::spec_augment_forward", mutates_args=())
def _spec_augment_forward_op(
    feats: torch.Tensor,
    uniforms: torch.Tensor,
    lengths: Optional[torch.Tensor],
    max_time_warp: float,
    max_time_mask: int,
    max_freq_mask: int,
    max_time_mask_proportion: float,
    num_time_mask: int,
    num_time_mask_proportion: float,
    num_freq_mask: int,
    interpolation_order: int,
) -> List[torch.Tensor]:
    """``SpecAugment.forward`` in training mode with a time warp and no frequency warp -- the usual
    configuration -- behind ONE operator: the draw kernel and the one-pass application are launched back
    to back (no tensors cross the dispatcher in between), and the lengths are judged by the application's
    kernel.  Same numbers as ``apply_parameters(draw_parameters())`` on the same uniforms.  Returns
    ``[out, w_0, w, t_0, t, f_0, f]`` (the parameters for the adjoint; disabled masks: zero elements)."""
    device = _cabi.require_hip(feats, uniforms, lengths)
    N, T, F = feats.shape
    x, _ = _spec_feats(feats)
    u = uniforms.detach()
    if u.dtype != torch.float or not u.is_contiguous():
        u = u.float().contiguous()
    tm, fm = _masks_enabled(max_time_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion,
                            max_freq_mask, num_freq_mask)
    lens = _lens_long(lengths)
    L = _cabi.lib()
    with torch.cuda.device(device):
        stream = _cabi.stream_ptr(device)
        w_0, w = (torch.empty((N,), device=device, dtype=torch.float) for _ in range(2))
        t_0, t = (torch.empty((N, num_time_mask) if tm else (0,), device=device, dtype=torch.long) for _ in range(2))
        f_0, f = (torch.empty((N, num_freq_mask) if fm else (0,), device=device, dtype=torch.long) for _ in range(2))
        rc = L.pdt_spec_augment_draw(
            _cabi.ptr(u), N, u.size(1), _cabi.ptr(lens), T, F, float(max_time_warp), 0.0,
            int(max_time_mask), int(max_freq_mask), float(max_time_mask_proportion), int(num_time_mask),
            float(num_time_mask_proportion), int(num_freq_mask), int(feats.dtype == torch.double),
            _cabi.ptr(w_0), _cabi.ptr(w), 0, 0, _cabi.ptr(t_0) if tm else 0, _cabi.ptr(t) if tm else 0,
            _cabi.ptr(f_0) if fm else 0, _cabi.ptr(f) if fm else 0, stream,
        )  # fmt: skip
        _cabi.check(rc, "pdt_spec_augment_draw")
    out = _launch_apply_warp(
        device, x, w_0, w, lens, interpolation_order, t_0 if tm else None, t if tm else None,
        num_time_mask if tm else 0, f_0 if fm else None, f if fm else None, num_freq_mask if fm else 0, True,
    )  # fmt: skip
    if out is None:  # (a layout the one-pass kernel does not take: through the grid)
        out = _spec_augment_apply(feats, (w_0, w, torch.empty(0), torch.empty(0), t_0, t, f_0, f), interpolation_order,
                                  lengths, True)
        return [out, w_0, w, t_0, t, f_0, f]
    return [out.to(feats.dtype), w_0, w, t_0, t, f_0, f]


@_spec_augment_forward_op.register_fake
def _(feats, uniforms, lengths, max_time_warp, max_time_mask, max_freq_mask, max_time_mask_proportion, num_time_mask,
      num_time_mask_proportion, num_freq_mask, interpolation_order):  # fmt: skip
    N = feats.shape[0]
    tm, fm = _masks_enabled(max_time_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion,
                            max_freq_mask, num_freq_mask)
    fl = [feats.new_empty((N,), dtype=torch.float) for _ in range(2)]
    tt = [feats.new_empty((N, num_time_mask) if tm else (0,), dtype=torch.long) for _ in range(2)]
    ff = [feats.new_empty((N, num_freq_mask) if fm else (0,), dtype=torch.long) for _ in range(2)]
    return [feats.new_empty(feats.shape)] + fl + tt + ff


def _spec_forward_setup_context(ctx, inputs, output):
    ctx.lengths, ctx.order, ctx.T = inputs[2], inputs[10], inputs[0].shape[1]
    ctx.params = tuple(output[1:])


def _spec_forward_backward(ctx, grads):
    grad_out = grads[0]  # (a List[Tensor] output: one list of gradients; the parameters carry none)
    w_0, w, t_0, t, f_0, f = ctx.params
    ln = ctx.lengths if ctx.lengths is not None else _full_lengths(w_0.shape[0], ctx.T, w_0.device)
    tgrid = torch.ops.pydrobert_amd.warp_1d_grid(w_0, w, ln, ctx.T, ctx.order)
    g = torch.ops.pydrobert_amd.spec_augment_apply_backward(
        grad_out, tgrid, None, t_0 if t_0.numel() else None, t if t.numel() else None,
        f_0 if f_0.numel() else None, f if f.numel() else None)
    return (g,) + (None,) * 10


register_autograd(
    "pydrobert_amd::spec_augment_forward", _spec_forward_backward, setup_context=_spec_forward_setup_context
)


def _spec_setup_context(ctx, inputs, output):
    ctx.grids = tuple(inputs[1:])


def _spec_backward(ctx, grad_out):
    g = torch.ops.pydrobert_amd.spec_augment_apply_backward(grad_out, *ctx.grids)
    return g, None, None, None, None, None, None


register_autograd(
    "pydrobert_amd::spec_augment_apply", _spec_backward, setup_context=_spec_setup_context
)


def spec_augment_apply_parameters(
    feats: torch.Tensor,
    params: SpecAugmentParams,
    interpolation_order: int,
    lengths: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Functional version of :func:`SpecAugment.apply_parameters` (reference
    _img.py:1142-1211): time / frequency warp by bilinear resampling, then band masks, as ONE
    pass over ``feats`` -- ONE launch when only time is warped (the common setting): the 1-D grid's spline is
    solved and evaluated inside it."""
    return _spec_augment_apply(feats, params, interpolation_order, lengths, True)


def _spec_augment_apply(
    feats: torch.Tensor,
    params: SpecAugmentParams,
    interpolation_order: int,
    lengths: Optional[torch.Tensor],
    check: bool,
) -> torch.Tensor:
    ok: Optional[torch.Tensor] = None
    w_0, w, v_0, v, t_0, t, f_0, f = params
    fused = _has(w_0, w) and not _has(v_0, v) and feats.is_cuda
    if check:
        _spec_augment_check_shapes(feats, lengths)
        if not fused:  # (the one-launch route hears about the lengths from its kernel)
            ok = _spec_augment_lengths_ok(feats, lengths)
    device = feats.device
    N, T, F = feats.size(0), feats.size(1), feats.size(2)
    lens_dev: Optional[torch.Tensor] = None if lengths is None else lengths.to(device)
    tgrid: Optional[torch.Tensor] = None
    fgrid: Optional[torch.Tensor] = None
    t0_: Optional[torch.Tensor] = None
    t_: Optional[torch.Tensor] = None
    f0_: Optional[torch.Tensor] = None
    f_: Optional[torch.Tensor] = None
    if _has(t_0, t):
        t0_, t_ = t_0.to(device).long().contiguous(), t.to(device).long().contiguous()
    if _has(f_0, f):
        f0_, f_ = f_0.to(device).long().contiguous(), f.to(device).long().contiguous()
    if fused:
        return torch.ops.pydrobert_amd.spec_augment_apply_warp(
            feats, w_0.to(device), w.to(device), lens_dev, interpolation_order, t0_, t_, f0_, f_, check
        )
    lengths_ = lens_dev if lens_dev is not None else _full_lengths(N, T, device)
    if _has(w_0, w):
        tgrid = warp_1d_grid(w_0.to(device), w.to(device), lengths_, T, interpolation_order)
    if _has(v_0, v):
        fgrid = warp_1d_grid(
            v_0.to(device), v.to(device), _full_lengths(N, F, device), F, interpolation_order
        )
    if tgrid is None and fgrid is None and t0_ is None and f0_ is None:
        _spec_augment_raise_unless(ok, T)
        return feats
    out = torch.ops.pydrobert_amd.spec_augment_apply(feats, tgrid, fgrid, t0_, t_, f0_, f_)
    _spec_augment_raise_unless(ok, T)
    return out


def spec_augment(
    feats: torch.Tensor,
    max_time_warp: float,
    max_freq_warp: float,
    max_time_mask: int,
    max_freq_mask: int,
    max_time_mask_proportion: float,
    num_time_mask: int,
    num_time_mask_proportion: float,
    num_freq_mask: int,
    interpolation_order: int,
    lengths: Optional[torch.Tensor] = None,
    training: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`SpecAugment` (reference _img.py:1214-1245)."""
    _spec_augment_check_shapes(feats, lengths)
    if not training:
        _spec_augment_raise_unless(_spec_augment_lengths_ok(feats, lengths), feats.size(1))
        return feats
    if not feats.is_cuda:  # (host tensors are refused further on; the reference's order of errors)
        _spec_augment_raise_unless(_spec_augment_lengths_ok(feats, lengths), feats.size(1))
    tm, fm = _masks_enabled(max_time_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion,
                            max_freq_mask, num_freq_mask)
    if feats.is_cuda and max_time_warp != 0.0 and max_freq_warp == 0.0 and feats.size(0) > 0:
        # the usual configuration: both halves behind one operator (csrc: the draw kernel, then the one-pass
        # application that solves the time warp's spline itself and judges the lengths)
        R = 2 + (2 * num_time_mask if tm else 0) + (2 * num_freq_mask if fm else 0)
        uniforms = torch.rand((feats.size(0), R), device=feats.device)
        return torch.ops.pydrobert_amd.spec_augment_forward(
            feats, uniforms, None if lengths is None else lengths.to(feats.device), max_time_warp, max_time_mask,
            max_freq_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion, num_freq_mask,
            interpolation_order,
        )[0]  # fmt: skip
    # ONE verdict on the lengths for both halves, read after their launches: the draw goes unchecked
    # (no kernel of it indexes with a length), the application checks -- in its own kernel when the time
    # warp runs in one launch, with the deferred reduction otherwise
    params = _spec_augment_draw(
        feats, max_time_warp, max_freq_warp, max_time_mask, max_freq_mask,
        max_time_mask_proportion, num_time_mask, num_time_mask_proportion, num_freq_mask, lengths, False,
    )  # fmt: skip
    return _spec_augment_apply(feats, params, interpolation_order, lengths, True)


# ---------------------------------------------------------------------------------------
class _ReprMixin:
    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)


class PolyharmonicSpline(_ReprMixin, torch.nn.Module):
    """Guess a surface with a polyharmonic spline (reference _img.py:153-241)."""

    __constants__ = "order", "regularization_weight", "full_matrix"

    def __init__(self, order: int, regularization_weight: float = 0.0, full_matrix: bool = True):
        order = argcheck.is_posi(order, "order")
        regularization_weight = argcheck.is_float(regularization_weight, "regularization_weight")
        full_matrix = argcheck.is_bool(full_matrix, "full_matrix")
        super().__init__()
        self.order, self.regularization_weight, self.full_matrix = order, regularization_weight, full_matrix

    def forward(
        self, train_points: torch.Tensor, train_values: torch.Tensor, query_points: torch.Tensor
    ) -> torch.Tensor:
        return polyharmonic_spline(
            train_points, train_values, query_points, self.order, self.regularization_weight,
            self.full_matrix,
        )  # fmt: skip


class Warp1DGrid(torch.nn.Module):
    """Interpolate grid values for a 1-D warp (reference _img.py:306-379)."""

    __constants__ = "max_length", "interpolation_order"

    def __init__(self, max_length: Optional[int] = None, interpolation_order: int = 1):
        if max_length is not None:
            max_length = argcheck.is_nonnegi(max_length, "max_length")
        interpolation_order = argcheck.is_posi(interpolation_order, "interpolation_order")
        super().__init__()
        self.max_length, self.interpolation_order = max_length, interpolation_order

    def extra_repr(self) -> str:
        s = "interpolation_order={}".format(self.interpolation_order)
        if self.max_length is not None:
            s = "max_length={}, ".format(self.max_length) + s
        return s

    def forward(self, src: torch.Tensor, flow: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        return warp_1d_grid(src, flow, lengths, self.max_length, self.interpolation_order)


class DenseImageWarp(_ReprMixin, torch.nn.Module):
    """Warp an input image with per-pixel flow vectors (reference _img.py:442-517)."""

    __constants__ = "indexing", "mode", "padding_mode"

    def __init__(self, indexing: str = "hw", mode: str = "bilinear", padding_mode: str = "border"):
        indexing = argcheck.is_in(indexing, _INDEXINGS, "indexing")
        mode = argcheck.is_in(mode, tuple(_MODES), "mode")
        padding_mode = argcheck.is_in(padding_mode, tuple(_PADDINGS), "padding_mode")
        super().__init__()
        self.indexing, self.mode, self.padding_mode = indexing, mode, padding_mode

    def forward(self, image: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
        return dense_image_warp(image, flow, self.indexing, self.mode, self.padding_mode)


class SparseImageWarp(_ReprMixin, torch.nn.Module):
    """Warp an image by specifying mappings between few control points (reference
    _img.py:717-880)."""

    __constants__ = (
        "indexing", "field_interpolation_order", "field_regularization_weight",
        "field_full_matrix", "pinned_boundary_points", "dense_interpolation_mode",
        "dense_padding_mode", "include_flow",
    )  # fmt: skip

    def __init__(
        self,
        indexing: str = "hw",
        field_interpolation_order: int = 2,
        field_regularization_weight: float = 0.0,
        field_full_matrix: bool = True,
        pinned_boundary_points: int = 0,
        dense_interpolation_mode: str = "bilinear",
        dense_padding_mode: str = "border",
        include_flow: bool = True,
    ):
        indexing = argcheck.is_in(indexing, _INDEXINGS, "indexing")
        field_interpolation_order = argcheck.is_posi(field_interpolation_order, "field_interpolation_order")
        field_regularization_weight = argcheck.is_float(field_regularization_weight, "field_regularization_weight")
        field_full_matrix = argcheck.is_bool(field_full_matrix, "field_full_matrix")
        pinned_boundary_points = argcheck.is_nonnegi(pinned_boundary_points, "pinned_boundary_points")
        dense_interpolation_mode = argcheck.is_in(dense_interpolation_mode, tuple(_MODES), "dense_interpolation_mode")
        dense_padding_mode = argcheck.is_in(dense_padding_mode, tuple(_PADDINGS), "dense_padding_mode")
        include_flow = argcheck.is_bool(include_flow, "include_flow")
        super().__init__()
        self.indexing = indexing
        self.field_interpolation_order = field_interpolation_order
        self.field_regularization_weight = field_regularization_weight
        self.field_full_matrix = field_full_matrix
        self.pinned_boundary_points = pinned_boundary_points
        self.dense_interpolation_mode = dense_interpolation_mode
        self.dense_padding_mode = dense_padding_mode
        self.include_flow = include_flow

    def forward(
        self, image: torch.Tensor, source_points: torch.Tensor, dest_points: torch.Tensor
    ) -> Any:
        return sparse_image_warp(
            image, source_points, dest_points, self.indexing, self.field_interpolation_order,
            self.field_regularization_weight, self.field_full_matrix, self.pinned_boundary_points,
            self.dense_interpolation_mode, self.dense_padding_mode, self.include_flow,
        )  # fmt: skip


class SpecAugment(torch.nn.Module):
    """Warp and mask the time / frequency axes of filter-bank features (reference
    _img.py:1248-1536).  Identity in eval mode."""

    __constants__ = (
        "max_time_warp", "max_freq_warp", "max_time_mask", "max_freq_mask",
        "max_time_mask_proportion", "num_time_mask", "num_time_mask_proportion", "num_freq_mask",
        "interpolation_order",
    )  # fmt: skip

    def __init__(
        self,
        max_time_warp: float = 80.0,
        max_freq_warp: float = 0.0,
        max_time_mask: int = 100,
        max_freq_mask: int = 27,
        max_time_mask_proportion: float = 0.04,
        num_time_mask: int = 20,
        num_time_mask_proportion: float = 0.04,
        num_freq_mask: int = 2,
        interpolation_order: int = 1,
    ):
        max_time_warp = argcheck.is_nonnegf(max_time_warp, "max_time_warp")
        max_freq_warp = argcheck.is_nonnegf(max_freq_warp, "max_freq_warp")
        max_time_mask = argcheck.is_nonnegi(max_time_mask, "max_time_mask")
        max_freq_mask = argcheck.is_nonnegi(max_freq_mask, "max_freq_mask")
        max_time_mask_proportion = argcheck.is_closed01(max_time_mask_proportion, "max_time_mask_proportion")
        num_time_mask = argcheck.is_nonnegi(num_time_mask, "num_time_mask")
        num_time_mask_proportion = argcheck.is_closed01(num_time_mask_proportion, "num_time_mask_proportion")
        num_freq_mask = argcheck.is_nonnegi(num_freq_mask, "num_freq_mask")
        interpolation_order = argcheck.is_posi(interpolation_order, "interpolation_order")
        super().__init__()
        self.max_time_warp, self.max_freq_warp = max_time_warp, max_freq_warp
        self.max_time_mask, self.max_freq_mask = max_time_mask, max_freq_mask
        self.max_time_mask_proportion = max_time_mask_proportion
        self.num_time_mask, self.num_time_mask_proportion = num_time_mask, num_time_mask_proportion
        self.num_freq_mask, self.interpolation_order = num_freq_mask, interpolation_order

    def extra_repr(self) -> str:
        s = "warp_t={},max_f={},num_f={},max_t={},max_t_p={:.2f},num_t={}".format(
            self.max_time_warp, self.max_freq_mask, self.num_freq_mask, self.max_time_mask,
            self.max_time_mask_proportion, self.num_time_mask,
        )  # fmt: skip
        if self.max_freq_warp:
            s += ",warp_f={}".format(self.max_freq_warp)
        return s

    @torch.jit.export
    def draw_parameters(
        self, feats: torch.Tensor, lengths: Optional[torch.Tensor] = None
    ) -> SpecAugmentParams:
        return spec_augment_draw_parameters(
            feats, self.max_time_warp, self.max_freq_warp, self.max_time_mask, self.max_freq_mask,
            self.max_time_mask_proportion, self.num_time_mask, self.num_time_mask_proportion,
            self.num_freq_mask, lengths,
        )  # fmt: skip

    @torch.jit.export
    def apply_parameters(
        self, feats: torch.Tensor, params: SpecAugmentParams, lengths: Optional[torch.Tensor] = None
    ) -> torch.Tensor:
        return spec_augment_apply_parameters(feats, params, self.interpolation_order, lengths)

    @torch.jit.export
    def reset_parameters(self) -> None:
        pass

    def forward(self, feats: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        if lengths is None:
            lengths = _full_lengths(feats.size(0), feats.size(1), feats.device)
        if not self.training:
            return feats
        if not torch.jit.is_scripting():
            # a subclass with its own draw / apply is served through them, as the reference's forward does
            # (_img.py:1520-1536); otherwise both halves run behind ONE verdict on the lengths
            cls = type(self)
            if cls.draw_parameters is not SpecAugment.draw_parameters or cls.apply_parameters is not SpecAugment.apply_parameters:
                params = self.draw_parameters(feats, lengths)
                return self.apply_parameters(feats, params, lengths)
        return spec_augment(
            feats, self.max_time_warp, self.max_freq_warp, self.max_time_mask, self.max_freq_mask,
            self.max_time_mask_proportion, self.num_time_mask, self.num_time_mask_proportion, self.num_freq_mask,
            self.interpolation_order, lengths, True,
        )  # fmt: skip


def random_shift(
    input: torch.Tensor,
    in_lens: torch.Tensor,
    prop: Tuple[float, float],
    mode: str,
    value: float,
    training: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Functional version of :class:`RandomShift` (reference _img.py:883-908): the draws use
    torch's generator on ``in_lens``' device, the movement is one ``pad_variable`` pass."""
    if input.dim() < 2:
        raise RuntimeError("input must be at least 2 dimensional")
    if in_lens.dim() != 1 or in_lens.size(0) != input.size(0):
        raise RuntimeError(
            "For input of shape {}, expected in_lens to be of shape ({}), got {}".format(
                input.shape, input.size(0), in_lens.shape
            )
        )
    if training:
        in_lens_ = in_lens.float()
        pad = torch.stack([prop[0] * in_lens_, prop[1] * in_lens_])
        pad *= torch.rand_like(pad)
        pad = pad.long()
        out_lens = in_lens + pad.sum(0)
        return pad_variable(input, in_lens, pad, mode, value), out_lens
    else:
        return input, in_lens


class RandomShift(torch.nn.Module):
    """Pad to the left and right of each sequence by a random amount (reference
    _img.py:911-1017).  Identity in eval mode."""

    __constants__ = ("prop", "mode", "value")

    def __init__(self, prop, mode: str = "reflect", value: float = 0.0):
        try:
            prop = (argcheck.is_float(prop, "prop"), float(prop))
        except (TypeError, ValueError):
            prop = tuple(prop)
        if len(prop) != 2:
            raise ValueError("prop must be a single or pair of floating points, got '{}'".format(prop))
        prop = (float(prop[0]), float(prop[1]))
        if prop[0] < 0.0 or prop[1] < 0.0:
            raise ValueError("prop values must be non-negative")
        mode = argcheck.is_in(mode, ("reflect", "constant", "replicate"), "mode")
        if mode == "reflect" and (prop[0] > 1.0 or prop[1] > 1.0):
            raise NotImplementedError("if 'mode' is 'reflect', values in 'prop' must be <= 1")
        value = argcheck.is_float(value, "value")
        super().__init__()
        self.mode, self.prop, self.value = mode, prop, value

    def extra_repr(self) -> str:
        return "prop={}, mode={}, value={}".format(self.prop, self.mode, self.value)

    def reset_parameters(self) -> None:
        pass

    def forward(self, input: torch.Tensor, in_lens: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return random_shift(input, in_lens, self.prop, self.mode, self.value, self.training)
