"""Shared by tests/test_warp_grads_cpu.py (which pins everything here without a GPU) and
tests/test_warp_grads_gpu.py: the float64 yardstick for the gradients of the image warps with respect to
where they sample -- the reference's own graph (spline -> grid -> ``grid_sample``) differentiated by
autograd on the CPU --, the fixed inputs of the GPU tests, the pixels next to a kink that a comparison
leaves out, the float32 bound of the flow's gradient, and the spline evaluation's adjoint as float64 torch
sums.

numpy and torch float64 on the CPU only; nothing here imports the package under test.  Cases, control
points and position tolerances come from tests/_img_ref.py.

A *kink* is where the warped image is not differentiable in the sampling position: an integer source
coordinate (the bilinear taps change), a clip limit, a reflection point.  Every implementation picks its own
subgradient there, so a pixel within ``DELTA`` of one on either axis is left out of the comparison."""
import math

import numpy as np
import torch

import _img_ref as R
from oracle import _img as _o

DELTA = 1e-3  # px
MAX_EXCLUDED = 0.01
EPS32 = float(np.finfo(np.float32).eps)

DENSE_SHAPES = ((2, 3, 47, 45), (1, 1, 1, 5))  # 2115 pixels: a full workgroup of 2048 and a partial one; a size-1 axis
SPARSE_SHAPE = (2, 2, 33, 29)
MEMORY_SHAPE = (4, 1, 256, 80)


# ---------------------------------------------------------------------------------------------------
# dense: fixed inputs, kinks, reference, bound
# ---------------------------------------------------------------------------------------------------
def dense_input(shape, dtype=np.float32):
    """(image, flow, grad_out): N(0, 1) pixels and output gradients; flows of a fifth of the image's size
    (at least two pixels), so that about a third of the samples leave the image."""
    N, C, H, W = shape
    rng = np.random.default_rng(1000 + H * W)
    image = rng.normal(size=shape).astype(dtype)
    flow = (rng.normal(size=(N, H, W, 2)) * np.maximum(np.array([H, W]) * 0.22, 2.0)).astype(np.float32)
    return image, flow, rng.normal(size=shape).astype(dtype)


def dense_flow(flow, indexing):
    """The fixed flow (generated in "hw" order) given in ``indexing``'s order: the same geometry."""
    return flow if indexing == "hw" else np.ascontiguousarray(flow[..., ::-1])


def near_kink(pos, H, W, padding, delta=DELTA):
    """(N, H', W') bool: the un-padded position (x, y) is within ``delta`` of a kink on either axis.
    Per axis: the coordinate after reflection (reflection padding; otherwise the coordinate itself) is within
    ``delta`` of an integer -- where the taps change, and the clip limits 0 and size - 1 are integers -- or,
    for reflection padding, of a reflection point (-0.5 or size - 0.5)."""
    out = np.zeros(pos.shape[:-1], bool)
    for axis, size in ((0, W), (1, H)):
        x = pos[..., axis]
        if padding == "reflection":
            r = _o._reflect(x, -1, 2 * size - 1)
            out |= (np.abs(r + 0.5) < delta) | (np.abs(r - (size - 0.5)) < delta)
            x = r
        out |= np.abs(x - np.round(x)) < delta
    return out


def outside_share(pos, H, W):
    """The share of samples whose position lies outside [0, size - 1] on either axis."""
    x, y = pos[..., 0], pos[..., 1]
    return float(np.mean((x < 0) | (x > W - 1) | (y < 0) | (y > H - 1)))


def dense_positions(flow, indexing, H, W, image_dtype=np.float64):
    return R.positions(R.dense_grid(flow, indexing, H, W, image_dtype), H, W)


def dense_flow_grad(image, flow, grad_out, indexing, mode, padding):
    """(grad_flow, grad_image) of sum(dense_image_warp(image, flow) * grad_out) in float64 by autograd."""
    N, C, H, W = image.shape
    img = torch.from_numpy(np.asarray(image, np.float64)).requires_grad_(True)
    fl = torch.from_numpy(np.asarray(flow, np.float32).astype(np.float64)).requires_grad_(True)
    hh, ww = torch.meshgrid(torch.arange(H, dtype=torch.double), torch.arange(W, dtype=torch.double), indexing="ij")
    xy = torch.stack((ww, hh), 2).unsqueeze(0)
    f = fl.flip(-1) if indexing == "hw" else fl
    grid = (2 * xy - 2 * f + 1.0) / torch.tensor([W, H], dtype=torch.double) - 1.0
    out = torch.nn.functional.grid_sample(img, grid, mode=mode, padding_mode=padding, align_corners=False)
    g_flow, g_img = torch.autograd.grad(out, [fl, img], torch.from_numpy(np.asarray(grad_out, np.float64)))
    return g_flow.numpy(), g_img.numpy()


def tap_stats(image, pos, H, W, padding):
    """(mixed, total), each (N, C, H', W'): per sample and channel the mixed difference t11 - t10 - t01 + t00
    of the four bilinear taps at the padded position (taps outside the image are 0) -- how fast a position
    gradient's component changes with the other coordinate -- and the sum of their magnitudes."""
    img = np.asarray(image, np.float64)
    p = R.pad_positions(pos, H, W, padding)
    x0, y0 = np.floor(p[..., 0]).astype(np.int64), np.floor(p[..., 1]).astype(np.int64)
    n = np.arange(img.shape[0])[:, None, None]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = img[n, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]  # (N, H', W', C)
        return np.moveaxis(np.where(ok[..., None], v, 0.0), -1, 1)

    t00, t01, t10, t11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    return t11 - t10 - t01 + t00, np.abs(t00) + np.abs(t01) + np.abs(t10) + np.abs(t11)


def dense_flow_grad_tol(image, pos, grad_out, H, W, padding):
    """(N, H, W, 1) bound on a float32 flow gradient's error, built the way ``_img_ref.value_tol`` builds the
    forward's.  A component of dL/d(ix, iy) is linear in the other coordinate with slope = the taps' mixed
    difference, so a position off by ``pos_tol_dense`` moves it by at most pos_tol x max_c |mixed_c| x
    sum_c |g_c|; the arithmetic adds roundings of eps32 each, relative to sum_c |g_c| x the taps' magnitudes:
    two products per term, 4 C accumulations and the last factor, 4 C + 3 in all."""
    C = np.asarray(image).shape[1]
    mixed, total = tap_stats(image, pos, H, W, padding)
    gsum = np.abs(np.asarray(grad_out, np.float64)).sum(1)
    tol = R.pos_tol_dense(H, W) * np.abs(mixed).max(1) * gsum + (4 * C + 3) * EPS32 * gsum * total.max(1)
    return tol[..., None]


# ---------------------------------------------------------------------------------------------------
# sparse: the reference's graph
# ---------------------------------------------------------------------------------------------------
def _torch_phi(r, k):
    return r**k if k % 2 else r**k * torch.log(r.clamp(min=EPS32))


class _Solve(torch.autograd.Function):
    """X = A^-1 B with numpy's LAPACK and the adjoint written out (g_B = A^-T g, g_A = -g_B X^T).  Not
    ``torch.linalg.solve``: for systems of a few hundred unknowns torch's threaded LAPACK does not return once
    ``torch.set_num_threads`` has been changed earlier in the process, which the benchmark's CPU baseline does
    when the suite runs as a whole."""

    @staticmethod
    def forward(ctx, A, B):
        X = torch.from_numpy(np.linalg.solve(A.detach().numpy(), B.detach().numpy()))
        ctx.save_for_backward(A, X)
        return X

    @staticmethod
    def backward(ctx, g):
        A, X = ctx.saved_tensors
        g_B = torch.from_numpy(np.linalg.solve(A.detach().transpose(1, 2).contiguous().numpy(), g.contiguous().numpy()))
        return -g_B @ X.transpose(1, 2), g_B


def torch_spline(c, f, x, k, reg=0.0):
    """The reference's spline as a float64 torch graph (_img.py:67-130), as tests/test_img_gpu.py writes it."""
    N, T, I = c.shape
    cdist = lambda a, b: torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist")  # noqa: E731
    A = _torch_phi(cdist(c, c), k) + reg * torch.eye(T, dtype=c.dtype)
    B = torch.cat([c, torch.ones_like(c[..., :1])], 2)
    M_ = torch.cat([torch.cat([A, B], 2), torch.cat([B.transpose(1, 2), c.new_zeros(N, I + 1, I + 1)], 2)], 1)
    sol = _Solve.apply(M_, torch.cat([f, f.new_zeros(N, I + 1, f.shape[2])], 1))
    return _torch_phi(cdist(x, c), k) @ sol[:, :T] + torch.cat([x, torch.ones_like(x[..., :1])], 2) @ sol[:, T:]


def sparse_warp_graph(image, src, dst, indexing, order, pinned, include_flow, reg, mode, padding):
    """(warped, flow or None) of sparse_image_warp as a float64 torch graph of the tensors ``src``, ``dst``."""
    N, C, H, W = image.shape
    s, d = (src.flip(-1), dst.flip(-1)) if indexing == "hw" else (src, dst)
    if pinned > 0:
        pp = torch.from_numpy(_o._pinned_points(pinned, W, H, N))
        s, d = torch.cat([s, pp], 1), torch.cat([d, pp], 1)
    hh, ww = torch.meshgrid(torch.arange(H, dtype=torch.double), torch.arange(W, dtype=torch.double), indexing="ij")
    xy = torch.stack((ww, hh), 2).unsqueeze(0)
    query = xy.reshape(1, H * W, 2).expand(N, H * W, 2)
    size = torch.tensor([W, H], dtype=torch.double)
    flow = None
    if include_flow:
        fxy = torch_spline(d, d - s, query, order, reg).view(N, H, W, 2)
        grid = (2 * xy - 2 * fxy + 1) / size - 1
        flow = fxy.flip(-1) if indexing == "hw" else fxy
    else:
        grid = torch_spline(d, (2 * s + 1) / size - 1, query, order, reg).view(N, H, W, 2)
    img = torch.from_numpy(np.asarray(image, np.float64))
    return torch.nn.functional.grid_sample(img, grid, mode=mode, padding_mode=padding, align_corners=False), flow


def sparse_points_grad(image, src, dst, grad_warped, grad_flow=None, indexing="hw", order=2, pinned=0,
                       include_flow=True, reg=0.0, mode="bilinear", padding="border"):
    """(grad_source, grad_dest) of sum(warped * grad_warped) [+ sum(flow * grad_flow)], float64 autograd."""
    s = torch.from_numpy(np.asarray(src, np.float32).astype(np.float64)).requires_grad_(True)
    d = torch.from_numpy(np.asarray(dst, np.float32).astype(np.float64)).requires_grad_(True)
    warped, flow = sparse_warp_graph(image, s, d, indexing, order, pinned, include_flow, reg, mode, padding)
    loss = (warped * torch.from_numpy(np.asarray(grad_warped, np.float64))).sum()
    if grad_flow is not None:
        loss = loss + (flow * torch.from_numpy(np.asarray(grad_flow, np.float64))).sum()
    g_s, g_d = torch.autograd.grad(loss, [s, d])
    return g_s.numpy(), g_d.numpy()


class SparseGradCase:
    """One sparse warp of the GPU file: its settings and fixed inputs ("hw" order, tests/_img_ref.py's
    control points: samples leave the image on every side), and the float64 gradients, computed once."""

    def __init__(self, name, order, include_flow, pinned, indexing, reg, padding="border", pts=4, scattered=False,
                 flow_grad=False, shape=SPARSE_SHAPE):
        self.name, self.order, self.include_flow, self.pinned = name, order, include_flow, pinned
        self.indexing, self.reg, self.padding, self.pts, self.flow_grad = indexing, reg, padding, pts, flow_grad
        self.shape = shape
        N, C, H, W = shape
        seed = 7 * order + 3 * pinned + int(include_flow)
        if scattered:
            self.src, self.dst = R.scattered_points(N, pts, H, W, 500 + seed)
        else:
            self.src, self.dst = R.control_points(N, pts, H, W, 400 + seed, R.BANDS_SCALE)
        rng = np.random.default_rng(600 + seed)
        self.image = rng.normal(size=shape).astype(np.float32)
        self.grad_warped = rng.normal(size=shape).astype(np.float32)
        self.grad_flow = rng.normal(size=(N, H, W, 2)).astype(np.float32) if flow_grad else None
        self._ref = None

    def __repr__(self):
        return self.name

    @property
    def Mp(self):
        return self.pts + 4 * self.pinned

    def points(self):
        return R.for_indexing(self.src, self.dst, self.indexing)

    def kwargs(self):
        return dict(indexing=self.indexing, field_interpolation_order=self.order,
                    field_regularization_weight=self.reg, pinned_boundary_points=self.pinned,
                    dense_padding_mode=self.padding, include_flow=self.include_flow)  # fmt: skip

    def expected(self):
        if self._ref is None:
            s, d = self.points()
            self._ref = sparse_points_grad(self.image, s, d, self.grad_warped, self.grad_flow, self.indexing,
                                           self.order, self.pinned, self.include_flow, self.reg, "bilinear",
                                           self.padding)  # fmt: skip
        return self._ref


def _sparse_cases():
    """Orders 1-4 x include_flow both ways, with pinned 0 / 1 / 2, both indexings, regularisation 0 / 0.05 and
    the three paddings going round, so that every value of each occurs with every order."""
    out = []
    k = 0
    for order in (1, 2, 3, 4):
        for include_flow in (True, False):
            for pinned in (0, 1, 2):
                indexing = R.INDEXINGS[k % 2]
                reg = 0.05 if (k // 2) % 2 else 0.0
                padding = R.PADDINGS[k % 3]
                out.append(SparseGradCase("o%d-%s-p%d-%s-r%g-%s" % (order, "flow" if include_flow else "grid", pinned,
                                                                    indexing, reg, padding),
                                          order, include_flow, pinned, indexing, reg, padding))  # fmt: skip
                k += 1
    out.append(SparseGradCase("flow-gradient-hw", 2, True, 1, "hw", 0.0, flow_grad=True))
    out.append(SparseGradCase("flow-gradient-wh", 3, True, 0, "wh", 0.0, flow_grad=True))
    return out


SPARSE_CASES = _sparse_cases()


MANY_SHAPE = (2, 1, 96, 80)
MANY_POS_ERR = 1e-3  # px


def many_centres_case(pts):
    """``pts`` scattered control points (+ 4 pinned): more spline rows than a workgroup of the evaluation's
    adjoint holds once ``pts`` passes what its plan says.  Order 1 on a 96 x 80 image, the centres about five
    pixels apart: a float32 evaluation of such a spline -- the reference's own, _img_ref.pos_tol_sparse --
    stays within MANY_POS_ERR of the float64 one (tests/test_warp_grads_cpu.py asserts it).  With r^2 log r
    over 250 centres on SPARSE_SHAPE it is off by 1e-2 px, and the adjoint solve of that ill-conditioned
    system (condition number 3e9) turns the noise into tens of per cent of the points' gradient, in the
    reference's float32 as in any other.

    The image is smooth (one period over more than the image) and the padding "zeros".  A centre among 250
    gathers its gradient from the thirty pixels around it, so ONE sample that a float32 position puts on the
    other side of a kink (an integer coordinate, a clip limit: about 60 of the 15 360 samples lie within 1e-3 px
    of one) moves that gradient by the jump of the image's slope there over those thirty: tens of per cent on
    N(0, 1) pixels -- in the reference's own float32 evaluation, see above --, below 1e-3 on this image, where
    adjacent slopes differ by 2 pi / 128 of their size and nothing is clipped."""
    case = SparseGradCase("many-%d" % pts, 1, True, 1, "hw", 0.0, "zeros", pts=pts, scattered=True, shape=MANY_SHAPE)
    N, C, H, W = MANY_SHAPE
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    ph = 1.3 * np.arange(N * C, dtype=np.float64).reshape(N, C, 1, 1)
    case.image = (np.sin(x * (2 * np.pi / 128.0) + ph) * np.cos(y * (2 * np.pi / 160.0) - ph)).astype(np.float32)
    return case


# ---------------------------------------------------------------------------------------------------
# the spline evaluation's adjoint as float64 torch sums
# ---------------------------------------------------------------------------------------------------
def phi_and_slope(r, order):
    """phi(r) and phi'(r) / r (zero where r = 0), float64: the formulas of the package's spline backward."""
    pos = r > 0
    safe = torch.where(pos, r, torch.ones_like(r))
    if order % 2:
        phi = r**order
        slope = order * safe ** (order - 2)
    else:
        lg = torch.log(safe.clamp(min=EPS32))
        phi = r**order * lg
        inner = torch.where(safe > EPS32, order * lg + 1.0, torch.full_like(lg, order * math.log(EPS32)))
        slope = safe ** (order - 2) * inner
    return phi, torch.where(pos, slope, torch.zeros_like(slope))


def eval_adjoint(G, c, sol, x, order):
    """(rhs (N, T+I+1, O), g_c (N, T, I), g_x (N, Q, I)) from float64 copies of the arrays."""
    G, c, sol, x = (torch.from_numpy(np.asarray(a)).double() for a in (G, c, sol, x))
    T, I = c.shape[1], c.shape[2]
    w, v = sol[:, :T], sol[:, T:]
    dxc = x.unsqueeze(2) - c.unsqueeze(1)
    phi, slope = phi_and_slope(dxc.norm(dim=3), order)
    x1 = torch.cat([x, torch.ones_like(x[..., :1])], 2)
    rhs = torch.cat([phi.transpose(1, 2) @ G, x1.transpose(1, 2) @ G], 1)
    g_phi = (G @ w.transpose(1, 2)) * slope
    g_c = -(g_phi.unsqueeze(3) * dxc).sum(1)
    g_x = (g_phi.unsqueeze(3) * dxc).sum(2) + G @ v[:, :I].transpose(1, 2)
    return rhs.numpy(), g_c.numpy(), g_x.numpy()


ADJOINT_QS = (1, 63, 65, 5003)  # below, at and past a wave; several workgroups with a ragged last one (T = 7)


def _plan_field(lib, N, T, I, O, Q, field):
    import ctypes

    p = (ctypes.c_int64 * 6)()
    assert lib.pdt_spline_eval_adjoint_plan(N, T, I, O, Q, p) >= 0
    return p[field]


def _last_true(ok, hi):
    """The largest T in [1, hi) with ok(T), for a predicate that holds up to a boundary."""
    lo = 1
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def form_boundary(lib, I, O, Q):
    """The largest T whose rows one workgroup of the evaluation's adjoint holds (form 0), from the plan."""
    return _last_true(lambda T: _plan_field(lib, 1, T, I, O, Q, 0) == 0, 1 << 16)


def lds_boundary(lib, I, O):
    """The largest T at which the queries' gradient stages solution and centres in LDS, from the plan."""
    return _last_true(lambda T: _plan_field(lib, 1, T, I, O, 65, 3) == 1, 1 << 20)


def lattice(N, H, W):
    """(N, H*W, 2) float32 pixel lattice (x = w, y = h), row-major."""
    h, w = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    return np.stack([w.ravel(), h.ravel()], 1)[None].repeat(N, 0)


def adjoint_case(T, I, O, Q, N, seed, coincide=True):
    """(G, c, sol, x): centres on a jittered grid, random "solution" and output gradient; with ``coincide``
    query 0 sits exactly on centre 0 (r = 0) and, where there is a second query, query 1 within float32
    eps of centre 1 (0 < r < eps: centre 1 is moved next to the origin, where float32 resolves 5e-8)."""
    rng = np.random.default_rng(seed)
    c = R.jittered_grid(rng, N, T, I)
    x = rng.uniform(-3, 3, (N, Q, I)).astype(np.float32)
    if coincide and Q >= 1:
        x[:, 0] = c[:, 0]
    if coincide and Q >= 2 and T >= 2:
        c[:, 1] = 1e-3
        x[:, 1] = c[:, 1]
        x[:, 1, 0] += np.float32(5e-8)
        assert ((x[:, 1, 0] - c[:, 1, 0]) > 0).all() and ((x[:, 1, 0] - c[:, 1, 0]) < EPS32).all()
    sol = rng.normal(size=(N, T + I + 1, O))
    G = rng.normal(size=(N, Q, O)).astype(np.float32)
    return G, c, sol, x
