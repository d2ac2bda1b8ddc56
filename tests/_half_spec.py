"""Shared by tests/test_half_spec_cpu.py and tests/test_half_spec_gpu.py: the forward and backward cases of
SpecAugment on float16 / bfloat16 features, their inputs, bit patterns, and the constructions whose exactness the
CPU test proves in numpy float32.

A case's features live in a base buffer and are seen through ``(offset, strides)`` in elements, so that the CPU
test can ask ``pdt_spec_augment_apply_form`` about the very layout the GPU test runs.  ``fwd`` / ``bwd`` are the
forms WRITTEN DOWN here from the kernels' conditions (csrc/spec_augment.hip: rows_layout_ok), not computed:
forward 0 the general kernel, 1 the rows kernel; backward "gather" (rows), "scatter" (atomics into float32
sums), "one" (scatter kernel with no grid: one writer per element)."""
import numpy as np
import torch

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ELEM = {"float32": 0, "float16": 2, "bfloat16": 3}
ESIZE = {0: 4, 2: 2, 3: 2}
BASE_ADDR = 0x7F0000000000  # an allocation's address for the plan query (allocators align to 256 bytes or more)


def _contig(N, T, F):
    return 0, (T * F, F, 1)


def _offset1(N, T, F):
    return 1, (T * F, F, 1)


def _stride2(N, T, F):
    return 0, (2 * T * F, 2 * F, 2)


def _transposed(N, T, F):  # a (T, N, F) buffer seen as (N, T, F)
    return 0, (F, N * F, 1)


LAYOUTS = {"contig": _contig, "offset1": _offset1, "stride2": _stride2, "transposed": _transposed}

# Forward cases.  tw / fw: a time / frequency warp; masks: band masks; ``fused``: does apply_parameters take the
# one-launch route (a time warp and no frequency warp) -- it then runs the rows kernel where fwd == 1 and falls
# back through the grid to the general kernel where fwd == 0.
FWD_CASES = {
    # two row tiles, the second partial; three 4-element columns (the index split's fix-up); a time mask across
    # the tile boundary, a frequency mask that splits a 4-element column; lengths on and next to the boundary
    "rows-two-tiles": dict(N=3, T=300, F=12, layout="contig", tw=True, fw=False, masks=True, order=2,
                           lens=[300, 257, 256], fwd=1),
    "rows-F256": dict(N=2, T=20, F=256, layout="contig", tw=True, fw=False, masks=True, order=1, lens=[20, 13], fwd=1),
    "general-F260": dict(N=2, T=20, F=260, layout="contig", tw=True, fw=False, masks=True, order=1, lens=[20, 13],
                         fwd=0),
    "general-freq-warp": dict(N=6, T=50, F=10, layout="contig", tw=True, fw=True, masks=True, order=3,
                              lens=[50, 37, 20, 25, 44, 31], fwd=0),
    "general-offset1-F8": dict(N=3, T=40, F=8, layout="offset1", tw=True, fw=False, masks=True, order=1,
                               lens=[40, 33, 21], fwd=0),
    "general-stride2": dict(N=3, T=40, F=8, layout="stride2", tw=True, fw=False, masks=True, order=2,
                            lens=[40, 33, 21], fwd=0),
    "rows-transposed": dict(N=3, T=40, F=12, layout="transposed", tw=True, fw=False, masks=True, order=1,
                            lens=[40, 33, 21], fwd=1),
    "general-odd-F7": dict(N=3, T=40, F=7, layout="contig", tw=True, fw=False, masks=True, order=1,
                           lens=[40, 33, 21], fwd=0),
    "rows-tiny-lengths": dict(N=4, T=90, F=12, layout="contig", tw=True, fw=False, masks=True, order=1,
                              lens=[1, 2, 3, 90], fwd=1),
    "rows-masks-only": dict(N=3, T=40, F=8, layout="contig", tw=False, fw=False, masks=True, order=1,
                            lens=[40, 33, 21], fwd=1),
}

# Backward cases (the operator's tensors are contiguous).  grid: "time" / "freq" / "both" / None; ``exact``: the
# dyadic construction below (sums independent of their order); ``monotone``: a sorted random time grid or an
# arbitrary one (gather only).
BWD_CASES = {
    "gather-monotone-700x8": dict(N=3, T=700, F=8, grid="time", monotone=True, bwd="gather"),
    "gather-arbitrary-700x8": dict(N=3, T=700, F=8, grid="time", monotone=False, bwd="gather"),
    "gather-monotone-300x12": dict(N=3, T=300, F=12, grid="time", monotone=True, bwd="gather"),
    "gather-arbitrary-300x12": dict(N=3, T=300, F=12, grid="time", monotone=False, bwd="gather"),
    "gather-no-grid": dict(N=3, T=40, F=8, grid=None, bwd="gather"),
    "scatter-exact-both": dict(N=2, T=64, F=16, grid="both", exact=True, bwd="scatter"),
    "scatter-exact-freq": dict(N=2, T=64, F=16, grid="freq", exact=True, bwd="scatter"),
    # a time grid alone on a layout the rows kernel refuses: 12 T + 1296 bytes of LDS above 64 KiB
    "scatter-exact-long-T": dict(N=1, T=8192, F=16, grid="time", exact=True, bwd="scatter"),
    "scatter-random-both": dict(N=2, T=64, F=16, grid="both", exact=False, bwd="scatter"),
    "scatter-random-odd-F": dict(N=3, T=50, F=10, grid="both", exact=False, bwd="scatter"),
    "one-to-one": dict(N=3, T=40, F=6, grid=None, bwd="one"),
}
EXACT_BWD = [n for n, c in BWD_CASES.items() if c.get("exact")]
RANDOM_SCATTER = [n for n, c in BWD_CASES.items() if c["bwd"] == "scatter" and not c.get("exact")]
BIT_BWD = [n for n, c in BWD_CASES.items() if c["bwd"] != "scatter" or c.get("exact")]


def layout_of(c):
    """``(offset, strides, base_numel)`` of a forward case, in elements."""
    off, st = LAYOUTS[c["layout"]](c["N"], c["T"], c["F"])
    last = off + (c["N"] - 1) * st[0] + (c["T"] - 1) * st[1] + (c["F"] - 1) * st[2]
    return off, st, last + 1


def form_query(lib, c, elem, has_time_grid, has_freq_grid):
    """pdt_spec_augment_apply_form for a forward case's layout at ``BASE_ADDR`` (the output: contiguous, aligned)."""
    off, st, _ = layout_of(c)
    return lib.pdt_spec_augment_apply_form(
        c["N"], c["T"], c["F"], st[0], st[1], st[2], BASE_ADDR + off * ESIZE.get(elem, 2), BASE_ADDR + (1 << 30),
        int(has_time_grid), int(has_freq_grid), 0, elem)  # fmt: skip


def bwd_form_query(lib, c, elem):
    T, F = c["T"], c["F"]
    return lib.pdt_spec_augment_apply_form(
        c["N"], T, F, T * F, F, 1, BASE_ADDR, BASE_ADDR + (1 << 30), int(c["grid"] in ("time", "both")),
        int(c["grid"] in ("freq", "both")), 1, elem)  # fmt: skip


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.numel() == 0:
        return True
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def ulp_of(ref):
    """The spacing of ``ref``'s dtype at ``|ref|`` (float32 tensor): next value up minus the value, from the bits."""
    a = ref.abs().contiguous()
    up = (a.view(torch.int16) + 1).view(ref.dtype)
    return up.float() - a.float()


# ---- forward inputs ---------------------------------------------------------------------------------------
def fwd_numpy(name):
    """The case's float32 features (N, T, F), parameters (the eight of SpecAugmentParams as numpy, empty where
    disabled) and lengths.  Warp targets stay away from the ends (tests/test_img_gpu.py: _draw)."""
    c = FWD_CASES[name]
    N, T, F = c["N"], c["T"], c["F"]
    rng = np.random.default_rng(sorted(FWD_CASES).index(name) + 500)
    feats = rng.uniform(-0.5, 0.5, size=(N, T, F)).astype(np.float32)
    lens = np.asarray(c["lens"], np.int64)
    z = np.zeros(0, np.float32)
    zl = np.zeros(0, np.int64)
    w_0 = w = v_0 = v = z
    t_0 = t = f_0 = f = zl
    if name == "rows-two-tiles":
        w_0, w = np.array([150.0, 120.5, 100.25], np.float32), np.array([4.0, -2.5, 3.25], np.float32)
        t_0, t = np.array([[250, 10], [40, 250], [250, 255]]), np.array([[11, 5], [3, 11], [11, 1]])
        f_0, f = np.array([[3], [3], [3]]), np.array([[3], [3], [3]])
        return feats, (w_0, w, v_0, v, t_0, t, f_0, f), lens
    if c["tw"]:
        W = np.maximum(np.minimum(lens / 2 - 1, 8.0), 0.0)
        w_0 = (rng.uniform(size=N) * (lens - 2 * W) + W).astype(np.float32)
        w = (rng.uniform(size=N) * W - W / 2).astype(np.float32)
    if c["fw"]:
        v_0 = (rng.uniform(size=N) * (F - 4) + 2).astype(np.float32)
        v = (rng.uniform(size=N) * 2 - 1).astype(np.float32)
    if c["masks"]:
        t = rng.integers(0, 6, (N, 2))
        t_0 = (rng.uniform(size=(N, 2)) * np.maximum(lens[:, None] - t, 0)).astype(np.int64)
        f = rng.integers(1, 4, (N, 1))
        f_0 = (rng.uniform(size=(N, 1)) * (F - f)).astype(np.int64)
    return feats, (w_0, w, v_0, v, t_0, t, f_0, f), lens


def strided(values, c, dtype, device):
    """``values`` (N, T, F) cast to ``dtype`` behind the case's layout: a view of a fresh base buffer."""
    off, st, numel = layout_of(c)
    base = torch.zeros(numel, dtype=dtype, device=device)
    view = base.as_strided((c["N"], c["T"], c["F"]), st, off)
    view.copy_(values.to(device=device, dtype=dtype))
    return view


def widened(x, c):
    """The float32 features of the reference: ``x``'s values, widened exactly, behind the same layout (offset and
    strides in elements), so that the float32 operator takes the kernel form the half one does."""
    return strided(x, c, torch.float32, x.device)


def fwd_tensors(name, dtype, device):
    """``(feats view in dtype, params on the device, lengths on the device, order)``."""
    c = FWD_CASES[name]
    feats, params, lens = fwd_numpy(name)
    x = strided(torch.from_numpy(feats), c, dtype, device)
    return x, tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in params), \
        torch.from_numpy(lens).to(device), c["order"]  # fmt: skip


# ---- backward inputs --------------------------------------------------------------------------------------
def dyadic_grid(rng, rows, size):
    """(rows, size) float32 grid values ``(2 p + 1) / size - 1`` with p a multiple of 1/8 in [0, size - 1], size a
    power of two: float32 holds each exactly and unnormalize gives p back exactly (the CPU test proves both).
    The p crowd into a quarter of the axis, so several outputs sample one source element."""
    p = rng.integers(0, 8 * (size // 4) + 1, (rows, size)).astype(np.float64) / 8.0 + (size // 4)
    p = np.minimum(p, size - 1)
    return ((2.0 * p + 1.0) / size - 1.0).astype(np.float32), p


def bwd_numpy(name):
    """``(grad_out float32 (N,T,F), tgrid or None, fgrid or None, t_0, t, f_0, f)`` of a backward case.  Exact
    cases: dyadic grids and grad_out in multiples of 2^-6 within [-2, 2] (both half types hold those exactly)."""
    c = BWD_CASES[name]
    N, T, F = c["N"], c["T"], c["F"]
    rng = np.random.default_rng(sorted(BWD_CASES).index(name) + 900)
    tg = fg = None
    if c.get("exact"):
        g = (rng.integers(-128, 129, (N, T, F)) / 64.0).astype(np.float32)
        if c["grid"] in ("time", "both"):
            tg = dyadic_grid(rng, N, T)[0]
        if c["grid"] in ("freq", "both"):
            fg = dyadic_grid(rng, N, F)[0]
    else:
        g = rng.normal(size=(N, T, F)).astype(np.float32)
        if c["grid"] in ("time", "both"):
            tg = (rng.uniform(size=(N, T)) * 2.4 - 1.2).astype(np.float32)  # some samples clip at both borders
            if c.get("monotone"):
                tg = np.sort(tg, 1)
        if c["grid"] in ("freq", "both"):
            fg = (rng.uniform(size=(N, F)) * 2.4 - 1.2).astype(np.float32)
    if (T, F) == (700, 8):
        t_0, t = np.array([[5, 300], [0, 650], [100, 100]]), np.array([[10, 40], [3, 50], [0, 7]])
        f_0, f = np.array([[1], [6], [0]]), np.array([[2], [2], [0]])
    elif (T, F) == (300, 12):
        t_0, t = np.array([[5, 250], [0, 255], [100, 100]]), np.array([[10, 11], [3, 40], [0, 7]])
        f_0, f = np.array([[3], [10], [0]]), np.array([[3], [2], [0]])
    else:
        t = rng.integers(0, 5, (N, 2))
        t_0 = rng.integers(0, T - 5, (N, 2))
        f = rng.integers(0, 3, (N, 1))
        f_0 = rng.integers(0, F - 3, (N, 1))
    return g, tg, fg, t_0.astype(np.int64), t.astype(np.int64), f_0.astype(np.int64), f.astype(np.int64)


def bwd_tensors(name, dtype, device):
    g, *rest = bwd_numpy(name)
    return (torch.from_numpy(g).to(device=device, dtype=dtype),) + tuple(
        None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in rest)


# img_sample.hpp's coordinate arithmetic in numpy float32, operation by operation
def unnormalize32(g, size):
    one, half = np.float32(1), np.float32(0.5)
    return ((g.astype(np.float32) + one) * np.float32(size) - one) * half


def clip_coord32(x, size):
    return np.minimum(np.float32(size - 1), np.maximum(x, np.float32(0)))


def taps32(g, size):
    """``(y0, w0, w1)`` as the kernels form them from a grid value: floor, iy - y0f, (y0f + 1) - iy."""
    i = clip_coord32(unnormalize32(g, size), size)
    y0f = np.floor(i)
    return y0f.astype(np.int64), (y0f + np.float32(1)) - i, i - y0f


# ---- planted values ---------------------------------------------------------------------------------------
PLANT_T, PLANT_F = 16, 8


def halfway_grid(N):
    """A time grid (N, PLANT_T) with every output row t halfway between source rows y0 = min(t, T - 2) and
    y0 + 1: g = (2 y0 + 2) / T - 1, so iy = y0 + 1/2 and w1 == w0 == 1/2 exactly (T a power of two)."""
    y0 = np.minimum(np.arange(PLANT_T), PLANT_T - 2).astype(np.float64)
    g = ((2.0 * y0 + 2.0) / PLANT_T - 1.0).astype(np.float32)
    return np.broadcast_to(g, (N, PLANT_T)).copy(), y0.astype(np.int64)


# bfloat16 bit patterns of neighbouring values whose mean lies exactly between two bfloat16 numbers: the mean of
# (0x3F80, 0x3F81) must round DOWN to the even 0x3F80, that of (0x3F81, 0x3F82) UP to the even 0x3F82
BF16_TIES = ((0x3F80, 0x3F81, 0x3F80), (0x3F81, 0x3F82, 0x3F82), (0xC07F, 0xC080, 0xC080))


def bf16_to_f32(bits):
    return np.array([bits << 16], np.uint32).view(np.float32)[0]


def planted(dtype):
    """float32 features (2, PLANT_T, PLANT_F) whose values ``dtype`` holds exactly, for the halfway grid (output
    row t = mean of rows y0 and y0 + 1): rows 0-1 +inf / -inf and row 2 NaN (under the time mask [0, 3)); row 5
    NaN in the open; rows 8, 9 the largest finite value; rows 10-12 float16 subnormals 2^-24, 2^-23, 3 * 2^-24;
    rows 13-14 the bfloat16 ties in columns 1-3; column 0 (under the frequency mask) NaN and inf alternating.
    (Column 0, because the general kernel reads column f + 1 for output column f, with weight 0 on an unwarped
    axis, like grid_sample: garbage in column 0 is read for the masked column 0 alone.)"""
    rng = np.random.default_rng(4242)
    x = (rng.integers(-64, 65, (2, PLANT_T, PLANT_F)) / 32.0).astype(np.float32)
    x[:, 0], x[:, 1], x[:, 2] = np.inf, -np.inf, np.nan
    x[:, 5] = np.nan
    x[:, 8:10] = torch.finfo(dtype).max
    x[:, 10], x[:, 11], x[:, 12] = 2.0 ** -24, 2.0 ** -23, 3 * 2.0 ** -24
    for col, (a, b, _) in enumerate(BF16_TIES):
        x[:, 13, col + 1], x[:, 14, col + 1] = bf16_to_f32(a), bf16_to_f32(b)
    x[:, 0::2, 0], x[:, 1::2, 0] = np.nan, np.inf
    t_0, t = np.array([[0], [0]], np.int64), np.array([[3], [3]], np.int64)
    f_0, f = np.array([[0], [0]], np.int64), np.array([[1], [1]], np.int64)
    return x, t_0, t, f_0, f
