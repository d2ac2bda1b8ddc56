"""Shared by the CPU suite (tests/test_img_cpu.py, which pins everything here) and the GPU suite
(tests/test_img_gpu.py): where a dense or sparse image warp samples its image, in float64, how far a
float32 evaluation of the same spline lands from there, how rough an image is under its padding rule --
the three numbers a warp's tolerance is made of -- and the shapes and cases of the GPU tests, so that the
conditions a case must meet (samples outside the image on every side, at most 1 % of nearest samples on a
rounding boundary, a tolerance that a tap one pixel off cannot meet) are checked without a GPU.

numpy and torch float64 only, on ``oracle``; nothing here imports the package under test.

A *grid* is ``grid_sample``'s normalised ``(N, R, W, 2)`` array (x, y in the last axis), holding exactly the
values ``oracle.grid_sample`` would read (float32-representable for a float32 image: the reference forms
the grid in the image's type); a *position* is its un-normalised pixel coordinate BEFORE the padding rule.
``rows`` selects output rows, so a very large image is checked on a few of them."""
import numpy as np

import oracle
from oracle import _img as _o

PADDINGS = ("border", "zeros", "reflection")
MODES = ("bilinear", "nearest")
INDEXINGS = ("hw", "wh")
POS_FLOOR = 2e-5  # px: the least position tolerance of a sparse warp
VALUE_FLOOR = 1e-5


# ---------------------------------------------------------------------------------------------------
# positions
# ---------------------------------------------------------------------------------------------------
def _as_grid_dtype(grid, image_dtype):
    """The values grid_sample reads: a float32 image has a float32 grid (oracle/_img.py grid_sample)."""
    if np.dtype(image_dtype) == np.float64:
        return grid.astype(np.float64)
    return grid.astype(np.float32).astype(np.float64)


def positions(grid, H, W):
    """(x, y) pixel positions of a normalised grid, float64, before padding (align_corners=False)."""
    g = np.asarray(grid, np.float64)
    return np.stack([((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2], -1)


def pad_positions(pos, H, W, padding):
    """The positions after grid_sample's padding rule (zeros: unchanged; taps outside drop out)."""
    x, y = pos[..., 0], pos[..., 1]
    if padding == "border":
        x, y = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    elif padding == "reflection":
        x = np.clip(_o._reflect(x, -1, 2 * W - 1), 0, W - 1)
        y = np.clip(_o._reflect(y, -1, 2 * H - 1), 0, H - 1)
    return np.stack([x, y], -1)


def _rows(H, rows):
    return np.arange(H) if rows is None else np.asarray(rows, dtype=np.int64)


def dense_grid(flow, indexing, H, W, image_dtype=np.float32, rows=None):
    """The grid of ``dense_image_warp`` (oracle/_img.py dense_image_warp) on the selected rows.
    ``flow``: (N, R, W, 2), the rows of the flow that belong to ``rows``."""
    r = _rows(H, rows).astype(np.float64)
    flow = np.asarray(flow, np.float32).astype(np.float64)
    assert flow.shape[1:] == (r.size, W, 2)
    h, w = np.meshgrid(r, np.arange(W, dtype=np.float64), indexing="ij")
    hw = np.stack([w, h], 2)[None]
    if indexing == "hw":
        flow = flow[..., ::-1]
    grid = (2 * hw - 2 * flow + 1.0) / np.array([W, H], np.float64) - 1.0
    return _as_grid_dtype(grid, image_dtype)


def _control_points(src, dst, indexing, pinned, H, W):
    """(dst, src) in (x, y) order with the pinned boundary points appended, float64 of the float32 points."""
    src = np.asarray(src, np.float32).astype(np.float64)
    dst = np.asarray(dst, np.float32).astype(np.float64)
    if indexing == "hw":
        src, dst = src[..., ::-1], dst[..., ::-1]
    if pinned > 0:
        pp = _o._pinned_points(pinned, W, H, src.shape[0])
        src, dst = np.concatenate([src, pp], 1), np.concatenate([dst, pp], 1)
    return dst, src


def _queries(N, H, W, rows):
    h, w = np.meshgrid(_rows(H, rows).astype(np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([w.ravel(), h.ravel()], 1)[None].repeat(N, 0)


def sparse_grid(src, dst, indexing, H, W, order, pinned=0, include_flow=False, reg=0.0, image_dtype=np.float32,
                rows=None):
    """(grid, flow): the grid of ``sparse_image_warp`` on the selected rows, built on
    ``oracle.polyharmonic_spline`` exactly as ``oracle.sparse_image_warp`` builds it (the spline's float32
    output first: the reference's grid / flow is a float32 tensor), and the flow it returns (``indexing``'s
    order; None in the no-flow form)."""
    d, s = _control_points(src, dst, indexing, pinned, H, W)
    N, R = d.shape[0], _rows(H, rows).size
    q = _queries(N, H, W, rows)
    if include_flow:
        flow = oracle.polyharmonic_spline(d, d - s, q, order, reg).reshape(N, R, W, 2)
        grid = dense_grid(flow, "wh", H, W, image_dtype, rows)
        return grid, np.ascontiguousarray(flow[..., ::-1] if indexing == "hw" else flow)
    vals = (2.0 * s + 1.0) / np.array([W, H], np.float64) - 1.0
    grid = oracle.polyharmonic_spline(d, vals, q, order, reg).reshape(N, R, W, 2)
    return _as_grid_dtype(grid, image_dtype), None


# ---------------------------------------------------------------------------------------------------
# the spline's own float32 error
# ---------------------------------------------------------------------------------------------------
def spline_solution(c, f, order, reg=0.0):
    """(w (N,T,O), v (N,I+1,O)): the float64 solution oracle.polyharmonic_spline solves for (the same
    statements; the oracle does not return it)."""
    c, f = np.asarray(c, np.float64), np.asarray(f, np.float64)
    N, T, I = c.shape
    A = _o._phi(_o._cdist(c, c), order)
    if reg > 0.0:
        A = A + np.eye(T)[None] * reg
    B = np.concatenate([c, np.ones((N, T, 1))], 2)
    lhs = np.concatenate([np.concatenate([A, B], 2), np.concatenate([B.transpose(0, 2, 1), np.zeros((N, I + 1, I + 1))], 2)], 1)
    wv = np.linalg.solve(lhs, np.concatenate([f, np.zeros((N, I + 1, f.shape[2]))], 1))
    return wv[:, :T], wv[:, T:]


def spline_eval(c, w, v, x, order, dtype=np.float64):
    """The spline at x in ``dtype`` arithmetic with a plain left-to-right sum over the centres (float32: how
    the reference's float32 matmul and the kernels' centre loops accumulate, up to their fused roundings)."""
    dt = np.dtype(dtype).type
    c, w, v, x = (np.asarray(a).astype(dtype) for a in (c, w, v, x))
    I = c.shape[2]
    acc = np.broadcast_to(v[:, None, I], (x.shape[0], x.shape[1], w.shape[2])).astype(dtype)
    for k in range(I):
        acc = (acc + x[:, :, k, None] * v[:, None, k]).astype(dtype)
    eps = dt(np.finfo(np.float32).eps)
    for t in range(c.shape[1]):
        d = x - c[:, None, t]
        r = np.sqrt((d * d).sum(-1, dtype=dtype)).astype(dtype)
        p = r**order if order % 2 else (r**order) * np.log(np.maximum(r, eps))
        acc = (acc + p.astype(dtype)[..., None] * w[:, None, t]).astype(dtype)
    return acc


def _sparse_positions_in(dtype, src, dst, indexing, H, W, order, pinned, include_flow, reg):
    dt = np.dtype(dtype).type
    d, s = _control_points(src, dst, indexing, pinned, H, W)
    N = d.shape[0]
    q = _queries(N, H, W, None)
    size = np.array([W, H], np.float64)
    vals = d - s if include_flow else (2.0 * s + 1.0) / size - 1.0
    w, v = spline_solution(d, vals, order, reg)
    val = spline_eval(d, w, v, q, order, dtype)
    if include_flow:  # the grid formula in the same arithmetic (oracle/_img.py dense_image_warp)
        val = ((dt(2) * q.astype(dtype) - dt(2) * val + dt(1)) / size.astype(dtype) - dt(1)).astype(dtype)
    g = val.astype(np.float64)
    return positions(g.reshape(N, H, W, 2), H, W)


def pos_tol_sparse(src, dst, indexing, H, W, order, pinned=0, include_flow=False, reg=0.0):
    """The float32 position error of the operation itself, from the reference alone: the float64 solution
    of the spline evaluated at every pixel in float32 with a plain left-to-right sum, against its float64
    evaluation; the largest distance in pixels.  A test's position tolerance is ``pos_tol(this)``."""
    p32 = _sparse_positions_in(np.float32, src, dst, indexing, H, W, order, pinned, include_flow, reg)
    p64 = _sparse_positions_in(np.float64, src, dst, indexing, H, W, order, pinned, include_flow, reg)
    return float(np.sqrt(((p32 - p64) ** 2).sum(-1)).max())


def pos_tol(measured):
    """4 x the measured float32 error (the kernels' fused multiply-adds, v_log_f32 and the table's
    pre-scaled weights against the plain sum), at least 2e-5 px."""
    return max(4.0 * measured, POS_FLOOR)


def pos_tol_dense(H, W):
    """The grid formula makes about four float32 roundings at magnitude <= 2, scaled by size / 2: 4 * 2^-24 *
    max(H, W), with a margin of 2."""
    return 8.0 * 2.0**-24 * max(H, W)


# ---------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------
def _extended(image, padding):
    img = np.asarray(image, np.float64)
    if padding == "zeros":
        img = np.pad(img, [(0, 0)] * (img.ndim - 2) + [(1, 1), (1, 1)])
    return img


def lipschitz(image, padding):
    """The largest difference between horizontally or vertically adjacent pixels of the image extended by
    its padding rule: a ring of zeros for "zeros" (edge magnitudes count), the image itself for "border"
    and "reflection" (both repeat pixels of the image)."""
    img = _extended(image, padding)
    return float(max(np.abs(np.diff(img, axis=-1)).max(initial=0.0), np.abs(np.diff(img, axis=-2)).max(initial=0.0)))


def median_step(image):
    """The median difference of adjacent pixels: what a tap one pixel off changes a sample by."""
    img = np.asarray(image, np.float64)
    return float(np.median(np.concatenate([np.abs(np.diff(img, axis=-1)).ravel(), np.abs(np.diff(img, axis=-2)).ravel()])))


def value_tol(ptol, image, padding):
    return VALUE_FLOOR + ptol * lipschitz(image, padding)


def sensitive(tol, image):
    """The sensitivity condition of every comparison: the tolerance is at most a tenth of the median step."""
    return tol <= 0.1 * median_step(image)


def outside_shares(pos, H, W):
    """The share of samples beyond the image (past the half-pixel where reflection folds and zeros padding
    has dropped at least half a sample's weight) on the left, right, top and bottom."""
    x, y = pos[..., 0], pos[..., 1]
    return tuple(float(np.mean(m)) for m in (x < -0.5, x > W - 0.5, y < -0.5, y > H - 0.5))


def off_boundary(pos, H, W, padding, ptol):
    """Nearest mode: True where the padded position is further than ``ptol`` from a rounding boundary (a
    half-integer) in both axes, so that every correct evaluation picks the same pixel."""
    p = pad_positions(pos, H, W, padding)
    frac = np.abs(p - np.floor(p) - 0.5)
    return (frac > ptol).all(-1)


def tap_pixels(pos, H, W, padding, ptol):
    """(lo, hi, weight_bound): per sample and axis the integer range [lo, hi] of pixels a bilinear tap may
    read with the position anywhere within ``ptol`` of ``pos`` (after padding), shape (..., 2) each."""
    p = pad_positions(pos, H, W, padding)
    return np.floor(p - ptol).astype(np.int64), np.floor(p + ptol).astype(np.int64) + 1


# ---------------------------------------------------------------------------------------------------
# the cases of the GPU tests
# ---------------------------------------------------------------------------------------------------
SHAPE_BANDS = (2, 2, 37, 29)  # ten bands of four rows, the last with one real row; 290 lanes: two workgroups
SHAPE_TWO_WG = (2, 2, 50, 45)  # 2250 pixels: image_warp_kernel's second workgroup has 202, its last pass partial
SHAPE_BIG = (1, 1, 2049, 4096)  # 2^23 + 4096 pixels: the integer-division branch
BIG_ROWS = (0, 1, 1023, 1024, 2047, 2048)
MIN_OUTSIDE = 0.02
MAX_BOUNDARY_SHARE = 0.01


def image(shape, seed, dtype=np.float32):
    """N(0, 1) pixels: both signs, median step ~ 0.95."""
    return np.random.default_rng(seed).normal(size=shape).astype(dtype)


def smooth_image(H, W):
    """A low-frequency pattern of both signs with adjacent pixels ~ 1e-3 apart (the 2^23-pixel case: the
    value tolerance stays near 1e-5)."""
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    return (np.sin(x * (2 * np.pi / 1536.0)) * np.cos(y * (2 * np.pi / 1024.0)) * 0.25).astype(np.float32)[None, None]


def control_points(N, Mp, H, W, seed, scale=1.0, spread=0.3):
    """(src, dst) in "hw" order, float32, (N, Mp, 2).  The first four destinations sit ``spread`` of the size
    inside the image, one on each quadrant's diagonal (rotated per image); their sources lie ``scale`` x half
    the size further OUT along that diagonal (plus jitter), so that samples leave the image on every side.
    Further points (up to five) sit at and around the centre, well apart from the four and from each other,
    and move by about a pixel."""
    rng = np.random.default_rng(seed)
    quad = np.array([[-1, -1], [1, 1], [-1, 1], [1, -1]], np.float64)
    inner = np.array([[0, 0], [0.5, 0], [-0.5, 0], [0, 0.5], [0, -0.5]], np.float64)
    assert Mp <= 4 + len(inner)
    k = (np.arange(Mp)[None, :] + np.arange(N)[:, None]) % 4
    first = (np.arange(Mp) < 4)[None, :, None]
    quad = np.where(first, quad[k], inner[np.maximum(np.arange(Mp) - 4, 0)][None])
    centre = np.array([(H - 1) / 2.0, (W - 1) / 2.0])
    half = np.array([H / 2.0, W / 2.0])
    dst = centre + quad * half * (1 - 2 * spread) + rng.uniform(-1.5, 1.5, (N, Mp, 2))
    src = dst + np.where(first, quad * half * scale, 0.0) + rng.normal(size=(N, Mp, 2))
    return src.astype(np.float32), dst.astype(np.float32)


def for_indexing(src, dst, indexing):
    """The same geometry given in ``indexing``'s order."""
    if indexing == "hw":
        return src, dst
    return np.ascontiguousarray(src[..., ::-1]), np.ascontiguousarray(dst[..., ::-1])


# (M', control points, pinned): the 24 instances are order x padding x M' in {7, 8}; 4 and 5 unpinned use the
# MC = 8 kernels with zero-weight filler centres
BANDS_M = {7: (3, 1), 8: (4, 1), 4: (4, 0), 5: (5, 0)}
BANDS_SCALE = 0.6
FOLD_SCALE = 5.0  # displacements of 2.5 image sizes: reflect_coord folds at least twice


def bands_case(Mp, seed=0, scale=BANDS_SCALE, shape=SHAPE_BANDS):
    """(image, src, dst, pinned) of the bands-kernel tests at M' spline centres, "hw" order."""
    N, C, H, W = shape
    pts, pinned = BANDS_M[Mp]
    src, dst = control_points(N, pts, H, W, 100 + Mp + seed, scale)
    return image(shape, 200 + Mp + seed), src, dst, pinned


def jittered_grid(rng, N, T, I, lo=-3.0, hi=3.0):
    """T centres per batch element on a jittered grid in [lo, hi]^I, shuffled: no two nearly coincide (a
    cell is (hi - lo) / side wide and the jitter stays within its middle half)."""
    side = int(np.ceil(T ** (1.0 / I)))
    cells = np.stack(np.meshgrid(*([np.arange(side)] * I), indexing="ij"), -1).reshape(-1, I)
    out = np.empty((N, T, I), np.float32)
    step = (hi - lo) / side
    for n in range(N):
        pick = cells[rng.permutation(len(cells))[:T]]
        out[n] = lo + (pick + 0.5 + rng.uniform(-0.25, 0.25, (T, I))) * step
    return out


def spline_case(T, I, O, Q, N, order, seed):
    rng = np.random.default_rng(seed)
    c = jittered_grid(rng, N, T, I)
    f = rng.normal(size=(N, T, O)).astype(np.float32)
    x = rng.uniform(-3, 3, (N, Q, I)).astype(np.float32)
    return c, f, x


def spline_bound(c, f, x, order, seed=0):
    """(expected, bound, noise): the oracle's spline, and the tolerance derived from the reference alone --
    the same problem solved by the oracle twice, with the centres in two different orders (the same
    mathematics, another elimination order); ``noise`` is the largest difference of the two outputs, the
    bound 10 x that with a floor of 2^-23 max|expected|."""
    exp = oracle.polyharmonic_spline(c, f, x, order)
    perm = np.random.default_rng(seed).permutation(c.shape[1])
    again = oracle.polyharmonic_spline(np.ascontiguousarray(c[:, perm]), np.ascontiguousarray(f[:, perm]), x, order)
    noise = float(np.abs(exp.astype(np.float64) - again).max())
    bound = max(10.0 * noise, 2.0**-23 * float(np.abs(exp).max()))
    return exp, bound, noise


def scattered_points(N, pts, H, W, seed):
    """(src, dst), "hw" order: ``pts`` destinations on a jittered grid over the image (no two nearly
    coincide), each moved by about a pixel."""
    rng = np.random.default_rng(seed)
    unit = (jittered_grid(rng, N, pts, 2, 0.0, 1.0)).astype(np.float64)
    dst = unit * np.array([H - 1.0, W - 1.0])
    src = dst + rng.normal(size=dst.shape)
    return src.astype(np.float32), dst.astype(np.float32)


class SparseCase:
    """One sparse warp of the GPU suite: its inputs ("hw" order) and what the CPU suite checks of it."""

    def __init__(self, name, shape, pts, pinned, order, include_flow=False, mode="bilinear", dtype=np.float32,
                 scale=BANDS_SCALE, seed=0, scattered=False, outside=True):
        self.name, self.shape, self.pts, self.pinned, self.order = name, shape, pts, pinned, order
        self.include_flow, self.mode, self.dtype, self.outside = include_flow, mode, dtype, outside
        N, C, H, W = shape
        self.Mp = pts + 4 * pinned
        if scattered:
            self.src, self.dst = scattered_points(N, pts, H, W, 300 + seed)
        else:
            self.src, self.dst = control_points(N, pts, H, W, 100 + self.Mp + seed, scale)
        self.image = image(shape, 200 + self.Mp + seed, dtype)
        self._ref = {}

    def __repr__(self):
        return self.name

    def points(self, indexing):
        return for_indexing(self.src, self.dst, indexing)

    def measured(self):
        """pos_tol_sparse of the case (the same for both indexings: the same geometry)."""
        if "m" not in self._ref:
            N, C, H, W = self.shape
            self._ref["m"] = pos_tol_sparse(self.src, self.dst, "hw", H, W, self.order, self.pinned, self.include_flow)
        return self._ref["m"]

    def ptol(self):
        return pos_tol(self.measured())

    def grid(self, indexing):
        """(grid, flow) as the oracle forms them, computed once."""
        if indexing not in self._ref:
            N, C, H, W = self.shape
            s, d = self.points(indexing)
            self._ref[indexing] = sparse_grid(s, d, indexing, H, W, self.order, self.pinned, self.include_flow,
                                              image_dtype=self.dtype)
        return self._ref[indexing]

    def expected(self, indexing, padding, img=None):
        key = (indexing, padding)
        if img is not None:
            return oracle.grid_sample(img, self.grid(indexing)[0], self.mode, padding)
        if key not in self._ref:
            self._ref[key] = oracle.grid_sample(self.image, self.grid(indexing)[0], self.mode, padding)
        return self._ref[key]


def _cases():
    out = {}

    def add(*a, **k):
        c = SparseCase(*a, **k)
        out[c.name] = c

    for order in (1, 2, 3, 4):
        for Mp in (7, 8, 4, 5):
            pts, pinned = BANDS_M[Mp]
            add("bands-o%d-m%d" % (order, Mp), SHAPE_BANDS, pts, pinned, order)
    add("bands-fold", SHAPE_BANDS, 4, 0, 2, scale=FOLD_SCALE, seed=1)
    add("edge-h5", (2, 2, 5, 7), 4, 0, 2)
    add("edge-h3", (2, 2, 3, 7), 4, 0, 2)
    add("general-flow-m7", SHAPE_TWO_WG, 3, 1, 2, include_flow=True)
    add("general-m12", SHAPE_TWO_WG, 8, 1, 2)
    add("general-nearest-m7", SHAPE_TWO_WG, 3, 1, 2, mode="nearest")
    add("general-o4-m9", SHAPE_TWO_WG, 5, 1, 4)
    add("general-f64-m7", SHAPE_TWO_WG, 3, 1, 2, dtype=np.float64)
    add("many-m138", SHAPE_BANDS, 130, 2, 2, include_flow=True, scattered=True, outside=False)
    add("many-m140", SHAPE_BANDS, 132, 2, 2, include_flow=True, scattered=True, outside=False)
    return out


SPARSE_CASES = _cases()


def dense_case(shape=SHAPE_TWO_WG, dtype=np.float32, seed=5):
    """(image, flow): N(0, 1) pixels, flows of about six pixels (samples leave the image on every side)."""
    rng = np.random.default_rng(seed)
    N, C, H, W = shape
    return rng.normal(size=shape).astype(dtype), (rng.normal(size=(N, H, W, 2)) * 6).astype(np.float32)


def big_flow(seed=8):
    """The 2^23-pixel case's flow, a few pixels in size (the whole (1, H, W, 2) array)."""
    N, C, H, W = SHAPE_BIG
    return (np.random.default_rng(seed).normal(size=(N, H, W, 2)) * 3).astype(np.float32)


def adjoint_reference(grid, g, H, W, mode, padding):
    """The adjoint of grid_sample with respect to the image, float64 autograd through torch's own
    grid_sample on the CPU: grid (N, R, W', 2) float64, g (N, C, R, W') -> (N, C, H, W)."""
    import torch

    x = torch.zeros((g.shape[0], g.shape[1], H, W), dtype=torch.double, requires_grad=True)
    y = torch.nn.functional.grid_sample(x, torch.from_numpy(np.ascontiguousarray(grid)), mode=mode, padding_mode=padding,
                                        align_corners=False)
    (gx,) = torch.autograd.grad(y, x, torch.from_numpy(np.ascontiguousarray(g)).double())
    return gx.numpy()


def adjoint_mass(pos, g, H, W, padding, ptol):
    """(N, H, W): per image pixel, the sum over channels' largest |g| of the samples whose taps may touch it
    (position anywhere within ``ptol``): a tap's weight moves by at most ``ptol`` per axis, so the adjoint
    of a correct kernel differs from the reference by at most 2 ptol x this, whatever the weights."""
    lo, hi = tap_pixels(pos, H, W, padding, ptol)
    ga = np.abs(np.asarray(g, np.float64)).max(1)  # (N, R, W')
    out = np.zeros((pos.shape[0], H, W))
    n = np.broadcast_to(np.arange(pos.shape[0])[:, None, None], ga.shape)
    for dy in range(int((hi[..., 1] - lo[..., 1]).max()) + 1):
        for dx in range(int((hi[..., 0] - lo[..., 0]).max()) + 1):
            yy, xx = lo[..., 1] + dy, lo[..., 0] + dx
            ok = (yy <= hi[..., 1]) & (xx <= hi[..., 0]) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            np.add.at(out, (n[ok], yy[ok], xx[ok]), ga[ok])
    return out
