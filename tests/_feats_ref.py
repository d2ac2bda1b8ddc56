"""References of their own for the feature front end: feature deltas and mean/variance normalisation in
plain numpy float64, written from the operators' definitions and sharing no code with the package.  Float64
torch restatements of the same two formulas give the gradients through autograd.  tests/test_feats_cpu.py pins
all of them to the reference's goldens and to the package's CPU bodies; the GPU suite compares the kernels
with them."""
import numpy as np
import torch

NP_PAD = {"replicate": "edge", "reflect": "reflect", "circular": "wrap", "constant": "constant"}
TINY = 1.1754943508222875e-38


def _axes(ndim, time_dim, dim, concatenate):
    t = time_dim % ndim
    k = dim % (ndim if concatenate else ndim + 1)
    return t, k


def deltas_ref(x, taps, time_dim=-2, dim=-1, concatenate=True, pad_mode="replicate", value=0.0):
    """y[u, t] = sum_k taps[u, k] * xp[t + k] along the time axis, xp = x padded by P = (K - 1) / 2 on both
    sides; the U orders stacked before axis ``dim`` of the output, or merged into axis ``dim`` of x, order
    major."""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    U, K = taps.shape
    P = (K - 1) // 2
    t, k = _axes(x.ndim, time_dim, dim, concatenate)
    T = x.shape[t]
    xt = np.moveaxis(x, t, 0)
    width = [(P, P)] + [(0, 0)] * (x.ndim - 1)
    if pad_mode == "constant":
        xp = np.pad(xt, width, "constant", constant_values=value)
    else:
        xp = np.pad(xt, width, NP_PAD[pad_mode])
    y = np.zeros((U,) + xt.shape)
    for kk in range(K):
        win = xp[kk:kk + T]
        for u in range(U):
            if taps[u, kk] != 0.0:
                y[u] += taps[u, kk] * win
    y = np.moveaxis(y, 1, t + 1)  # (U, *x.shape)
    y = np.moveaxis(y, 0, k)  # the order axis just before x's axis k
    if concatenate:
        shape = list(x.shape)
        shape[k] *= U
        y = y.reshape(shape)
    return np.ascontiguousarray(y)


def _padded_steps(T, P, pad_mode):
    """Which step of x each padded position copies (-1: the constant), from np.pad itself."""
    if pad_mode == "constant":
        return np.pad(np.arange(T), P, "constant", constant_values=-1)
    return np.pad(np.arange(T), P, NP_PAD[pad_mode])


def deltas_torch(x, taps, time_dim=-2, dim=-1, concatenate=True, pad_mode="replicate", value=0.0):
    """The same formula as a float64 torch graph, one matrix product per time step: y[:, t] = taps @
    xp[t : t + K]."""
    x = x.double()
    taps = taps.detach().double().to(x.device)
    U, K = taps.shape
    P = (K - 1) // 2
    t, k = _axes(x.dim(), time_dim, dim, concatenate)
    T = x.shape[t]
    xt = x.movedim(t, 0)
    rest = xt.shape[1:]
    xt = xt.reshape(T, -1)
    steps = torch.from_numpy(_padded_steps(T, P, pad_mode)).to(x.device)
    xp = xt.index_select(0, steps.clamp_min(0))
    if pad_mode == "constant":
        xp = torch.where((steps >= 0).unsqueeze(1), xp, xp.new_full((), value))
    y = torch.stack([taps @ xp[s:s + K] for s in range(T)], 1)  # (U, T, rest)
    y = y.reshape((U, T) + tuple(rest)).movedim(1, t + 1).movedim(0, k)
    if concatenate:
        y = y.flatten(k, k + 1)
    return y.contiguous()


def _moments(x, dim):
    axes = tuple(d for d in range(x.ndim) if d != dim % x.ndim)
    mean = x.mean(axes)
    shape = [1] * x.ndim
    shape[dim % x.ndim] = -1
    std = np.sqrt(np.square(x - mean.reshape(shape)).mean(axes))
    return mean, std, shape


def mvn_ref(x, dim=-1, mean=None, std=None, eps=TINY):
    """(y, mean, std): y = (x - mean) / max(std, eps) per index of ``dim``; the statistics not given are the
    mean and the population standard deviation of x over every other axis (two passes, float64)."""
    x = np.asarray(x, dtype=np.float64)
    m, s, shape = _moments(x, dim)
    m = m if mean is None else np.asarray(mean, dtype=np.float64).reshape(-1)
    s = s if std is None else np.asarray(std, dtype=np.float64).reshape(-1)
    y = (x - m.reshape(shape)) / np.maximum(s, eps).reshape(shape)
    return y, m, s


def mvn_ref_rounded(x, dim=-1, mean=None, std=None, eps=TINY):
    """mvn_ref for a torch tensor of a narrow dtype, rounding to that dtype where the operator does: the
    mean, the standard deviation (before the clamp) and the difference x - mean.  The quotient is left in
    float64.  Returns (y, mean, std), numpy float64."""
    dtype = x.dtype

    def rnd(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).double().numpy()

    xd = x.detach().cpu().double().numpy()
    m, s, shape = _moments(xd, dim)
    m = m if mean is None else mean.detach().cpu().double().numpy().reshape(-1)
    s = s if std is None else std.detach().cpu().double().numpy().reshape(-1)
    c = rnd(xd - rnd(m).reshape(shape))
    y = c / np.maximum(rnd(s), eps).reshape(shape)
    return y, m, s


def mvn_torch(x, dim=-1, mean=None, std=None, eps=TINY):
    """The same formula as a float64 torch graph (gradients reach x and the given statistics)."""
    x = x.double()
    dims = [d for d in range(x.dim()) if d != dim % x.dim()]
    shape = [1] * x.dim()
    shape[dim % x.dim()] = -1
    m = x.mean(dims) if mean is None else mean.double().reshape(-1)
    # (torch.std: the population formula, and a zero gradient where the deviation is zero and the clamp holds)
    s = x.std(dims, unbiased=False) if std is None else std.double().reshape(-1)
    return (x - m.view(shape)) / s.clamp_min(eps).view(shape)


def ulps(act, exp, dtype):
    """Largest distance of ``act`` (a tensor of ``dtype``) from the float64 array ``exp`` rounded to
    ``dtype``, in units of eps * max(|exp|, 1): the suite's 16-bit measure."""
    e = torch.from_numpy(np.ascontiguousarray(exp)).to(dtype).double()
    unit = e.abs().clamp_min(1.0) * torch.finfo(dtype).eps
    return ((act.detach().cpu().double() - e).abs() / unit).max().item()


# ----------------------------------------------------------------------------------------------------------
# the shapes the CPU pins and the GPU suite share

MODES = ("replicate", "reflect", "circular", "constant")
EDGE = ("replicate", "constant")  # (reflect and circular need P <= T)

# (id, x shape, dtype, feat_deltas arguments, pad modes)
DELTA_CASES = [
    ("vec-2coltiles", (2, 40, 260), "float32", dict(order=2, width=2), MODES),
    ("scalar-2coltiles", (2, 150, 70), "float32", dict(order=2, width=2), MODES),
    ("c-across-coltile", (2, 40, 5, 60), "float32", dict(order=2, width=2, time_dim=1, dim=3), MODES),
    ("order-axis-0-cat", (2, 40, 260), "float32", dict(order=2, width=2, dim=0, concatenate=True), MODES),
    ("order-axis-0-stack", (2, 40, 260), "float32", dict(order=2, width=2, dim=0, concatenate=False), MODES),
    ("order-axis-1-cat", (2, 40, 260), "float32", dict(order=2, width=2, dim=1, concatenate=True), MODES),
    ("order-axis-1-stack", (2, 40, 260), "float32", dict(order=2, width=2, dim=1, concatenate=False), MODES),
    ("order-axis-last-stack", (2, 40, 260), "float32", dict(order=2, width=2, dim=-1, concatenate=False), MODES),
    ("float64-2x2tiles", (2, 40, 130), "float64", dict(order=2, width=2), MODES),
    ("float16-2x3tiles", (2, 20, 520), "float16", dict(order=2, width=2), MODES),
    ("bfloat16-2x3tiles", (2, 20, 520), "bfloat16", dict(order=2, width=2), MODES),
    ("shrink-mild", (1, 64, 256), "float32", dict(order=2, width=20), MODES),
    ("shrink-deep", (1, 320, 256), "float32", dict(order=3, width=100), MODES),
    ("lds-last-f32-vec", (1, 6, 4), "float32", dict(order=1, width=2047), EDGE),
    ("direct-first-f32-vec", (1, 6, 4), "float32", dict(order=1, width=2048), EDGE),
    ("lds-last-f32-scalar", (1, 5, 3), "float32", dict(order=1, width=8191), EDGE),
    ("direct-first-f32-scalar", (1, 5, 3), "float32", dict(order=1, width=8192), EDGE),
    ("lds-last-f64", (1, 6, 2), "float64", dict(order=1, width=2047), EDGE),
    ("direct-first-f64", (1, 6, 2), "float64", dict(order=1, width=2048), EDGE),
    ("lds-last-f16", (1, 6, 8), "float16", dict(order=1, width=1023), EDGE),
    ("direct-first-f16", (1, 6, 8), "float16", dict(order=1, width=1024), EDGE),
    ("circular-P-eq-T", (2, 12, 8), "float32", dict(order=3, width=4), ("circular",)),
    ("reflect-P-eq-T-1", (2, 13, 8), "float32", dict(order=3, width=4), MODES),
]

# (x shape, dim) in float32
MVN_CASES = [
    ((300, 300), -1),
    ((40, 257), -1),
    ((500, 255), -1),
    ((1000, 80), -1),
    ((20000, 1), -1),
    ((37, 3, 301), 1),
    ((5000, 4, 3), 1),
    ((6, 9000), 0),
    ((3, 5, 300), 1),
    ((10, 6), -1),
    ((4, 9), -1),
]
# (x shape, dim) in float16 and bfloat16
MVN_CASES_16 = [((16, 3), -1), ((8, 12), -1), ((37, 3, 301), 1), ((1000, 80), -1)]

# The largest distance, in ulps (see ulps()), of the package's CPU body from mvn_ref_rounded over MVN_CASES_16
# with the inputs of mvn_input(), measured: 0.0 in float16 and 0.0 in bfloat16 (33411 and 80000 elements at the
# two large shapes) -- with the mean, the deviation and the difference rounded alike, the float32 quotient
# rounds to the same 16-bit number as the float64 one.  test_feats_cpu.py asserts the figure; the GPU suite
# allows one ulp more, for the kernel's own float32 division.
MVN_16BIT_CPU_ULPS = 0.0


def delta_input(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(1234 + seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(getattr(torch, dtype) if isinstance(dtype, str) else dtype)


def mvn_input(shape, dtype, seed=0):
    """randn * 3 + 1: means away from zero."""
    g = torch.Generator().manual_seed(4321 + seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * 3 + 1).to(dtype)


def upstream(shape, dtype):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)
