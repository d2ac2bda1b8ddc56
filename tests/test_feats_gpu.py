"""GPU: feat_deltas / FeatureDeltas and mean_var_norm / MeanVarianceNormalization on the HIP path
(csrc/feats.hip) -- the reference's goldens, the C4 shape, sweeps against a float64 restatement on the
device, gradcheck, statistics robustness, determinism, accumulate, 16-bit dtypes, traceability and no
host synchronisation; then every tile and launch form of the kernels against the references of
tests/_feats_ref.py (numpy float64, and float64 torch graphs for the gradients)."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
MODES = ("replicate", "reflect", "circular", "constant")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "feats.npz"))


def upstream(shape, dtype, device=DEV):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(device=device, dtype=dtype)


def ref_deltas(x, **kw):
    """float64 restatement: the package's torch body (checked against the reference's goldens on the CPU)."""
    from pydrobert_amd import _feats

    kw = dict(dict(dim=-1, time_dim=-2, concatenate=True, order=2, width=2, pad_mode="replicate", value=0.0), **kw)
    t, k = _feats._delta_geometry(list(x.shape), kw["dim"], kw["time_dim"], kw["concatenate"])
    f = _feats._feat_delta_filters(kw["order"], kw["width"]).to(x.device)
    return _feats._feat_deltas_torch(x.double(), f, t, k, kw["concatenate"], kw["order"], kw["width"],
                                     kw["pad_mode"], kw["value"])  # fmt: skip


def ref_mvn(x, dim=-1):
    xd = x.double()
    dims = [d for d in range(x.dim()) if d != dim % x.dim()]
    mean = xd.mean(dims, keepdim=True)
    std = (xd - mean).square().mean(dims, keepdim=True).sqrt()
    return (xd - mean) / std.clamp_min(1.1754943508222875e-38)


def test_goldens_outputs_and_gradients(gold):
    from pydrobert_amd import functional as F

    for k in range(int(gold["deltas_n"])):
        pre = "deltas_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        x = torch.from_numpy(gold[pre + "x"]).to(DEV).requires_grad_(True)
        tol = 1e-5 if x.dtype == torch.float32 else 1e-12
        y = F.feat_deltas(x, **kw)
        assert y.shape == gold[pre + "y"].shape, kw
        assert np.abs(y.detach().cpu().numpy() - gold[pre + "y"]).max() <= tol, kw
        (gx,) = torch.autograd.grad(y, x, upstream(tuple(y.shape), x.dtype))
        assert np.abs(gx.cpu().numpy() - gold[pre + "gx"]).max() <= tol * max(1.0, np.abs(gold[pre + "gx"]).max()), kw
    for k in range(int(gold["mvn_n"])):
        pre = "mvn_{}_".format(k)
        kw = json.loads(str(gold[pre + "kw"]))
        x = torch.from_numpy(gold[pre + "x"]).to(DEV).requires_grad_(True)
        mean = torch.from_numpy(gold[pre + "mean"]).to(DEV).requires_grad_(True) if pre + "mean" in gold else None
        std = torch.from_numpy(gold[pre + "std"]).to(DEV).requires_grad_(True) if pre + "std" in gold else None
        y = F.mean_var_norm(x, kw["dim"], mean, std)
        assert np.allclose(y.detach().cpu().numpy(), gold[pre + "y"], rtol=1e-5, atol=1e-5), kw
        ins = [t for t in (x, mean, std) if t is not None]
        grads = torch.autograd.grad(y, ins, upstream(tuple(x.shape), x.dtype))
        assert np.allclose(grads[0].cpu().numpy(), gold[pre + "gx"], rtol=1e-5, atol=1e-5), kw
        if mean is not None:
            assert np.allclose(grads[1].cpu().numpy(), gold[pre + "gmean"], rtol=1e-5, atol=1e-5), kw
        if std is not None:
            assert np.allclose(grads[-1].cpu().numpy(), gold[pre + "gstd"], rtol=1e-5, atol=1e-5), kw


def test_goldens_accumulate_store(gold):
    from pydrobert_amd import modules as M

    chunks = [torch.from_numpy(gold["acc_chunk_{}".format(i)]).to(DEV) for i in range(6)]
    for bessel in (False, True):
        m = M.MeanVarianceNormalization(dim=1)
        for c in chunks:
            m.accumulate(c)
        for name in ("count", "sum", "sumsq"):
            assert np.allclose(getattr(m, name).cpu().numpy(), gold["acc_" + name], rtol=1e-12, atol=0), name
        m.store(bessel=bessel)
        assert np.allclose(m.mean.cpu().numpy(), gold["acc_mean_b{}".format(int(bessel))], rtol=1e-12, atol=0)
        assert np.allclose(m.std.cpu().numpy(), gold["acc_std_b{}".format(int(bessel))], rtol=1e-12, atol=0)


def test_full_size_c4():
    from pydrobert_amd import functional as F

    x = torch.randn(2048, 1000, 80, device=DEV)
    y = F.feat_deltas(x)
    assert y.shape == (2048, 1000, 240)
    for n0 in (0, 1024, 2047):  # (the float64 restatement of the whole tensor would not fit beside it)
        exp = ref_deltas(x[n0:n0 + 1])
        assert (y[n0:n0 + 1].double() - exp).abs().max().item() < 1e-5
    del y
    z = F.mean_var_norm(x, -1)
    xd = x.double()
    mean = xd.mean((0, 1))
    std = xd.var((0, 1), unbiased=False).sqrt()
    for n0 in (0, 2047):
        exp = (xd[n0] - mean) / std
        assert (z[n0].double() - exp).abs().max().item() < 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_sweep_against_float64(mode):
    from pydrobert_amd import functional as F

    for order, width in itertools.product(range(4), (1, 2, 3)):
        P = order * width
        T = max(P + 1, 9)
        base = torch.randn(3, T, 5, 4, device=DEV)
        for td, dim, conc in ((1, 0, True), (1, 1, False), (1, 2, True), (1, 3, False), (1, 4, False), (1, -1, True),
                              (2, 0, False), (2, 1, True), (2, 3, True), (2, -1, False), (0, 2, True)):
            x = base.movedim(1, td).contiguous() if td != 1 else base
            kw = dict(dim=dim, time_dim=td, concatenate=conc, order=order, width=width, pad_mode=mode,
                      value=-0.5 if mode == "constant" else 0.0)
            y = F.feat_deltas(x, **kw)
            exp = ref_deltas(x, **kw)
            assert y.shape == exp.shape and (y.double() - exp).abs().max().item() < 1e-5, kw
        # non-contiguous inputs: a transposed view and a stepped slice
        kw = dict(order=order, width=width, pad_mode=mode, value=0.25 if mode == "constant" else 0.0)
        xt = torch.randn(5, T, 3, device=DEV).transpose(0, 2)  # (3, T, 5), time stride 5
        assert (F.feat_deltas(xt, **kw).double() - ref_deltas(xt, **kw)).abs().max().item() < 1e-5
        xs = torch.randn(3, T, 16, device=DEV)[:, :, ::2]
        assert (F.feat_deltas(xs, **kw).double() - ref_deltas(xs, **kw)).abs().max().item() < 1e-5
    for dim in range(-3, 3):
        x = torch.randn(6, 7, 9, device=DEV) * 3 + 1
        assert (torch.ops.pydrobert_amd.mean_var_norm(x, dim, None, None, 1e-38)[0].double() - ref_mvn(x, dim)).abs().max() < 1e-5
        xt = x.transpose(0, 2)
        assert (F.mean_var_norm(xt, dim).double() - ref_mvn(xt, dim)).abs().max() < 1e-5


def test_gradcheck_float64():
    from pydrobert_amd import functional as F

    x = torch.randn(2, 7, 3, device=DEV, dtype=torch.float64, requires_grad=True)
    for mode in MODES:
        def fn(x, mode=mode):
            return F.feat_deltas(x, order=2, width=1, pad_mode=mode, value=0.3 if mode == "constant" else 0.0)

        assert torch.autograd.gradcheck(fn, (x,))
        assert torch.autograd.gradgradcheck(fn, (x,))
    xs = torch.randn(4, 3, 5, device=DEV, dtype=torch.float64) * 2 + 1
    x = xs.clone().requires_grad_(True)
    xs[:, 1] = 0.5 + 0.01 * torch.randn(4, 5, device=DEV, dtype=torch.float64)
    xc = xs.requires_grad_(True)  # the clamp case: a feature whose std stays below eps
    mean = torch.randn(3, device=DEV, dtype=torch.float64, requires_grad=True)
    std = (torch.rand(3, device=DEV, dtype=torch.float64) + 0.5).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: F.mean_var_norm(x, 1), (x,))
    assert torch.autograd.gradcheck(lambda x, m, s: F.mean_var_norm(x, 1, m, s), (x, mean, std))
    assert torch.autograd.gradcheck(lambda x, m: F.mean_var_norm(x, 1, m), (x, mean))
    assert torch.autograd.gradcheck(lambda x, s: F.mean_var_norm(x, 1, None, s), (x, std))
    assert torch.autograd.gradcheck(lambda x: F.mean_var_norm(x, 1, eps=0.5), (xc,))
    assert torch.autograd.gradcheck(lambda x, m: F.mean_var_norm(x, 1, m, eps=0.5), (xc, mean))
    x2 = torch.randn(5, 4, 6, device=DEV, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: F.mean_var_norm(x, 0), (x2,))


def test_statistics_robust_to_large_mean():
    from pydrobert_amd import modules as M

    rng = np.random.default_rng(5)
    xn = (rng.standard_normal((4000, 16)) * 0.5 + 1e4 * 0.5 * np.sign(rng.standard_normal(16))).astype(np.float32)
    x = torch.from_numpy(xn).to(DEV)
    stats = torch.ops.pydrobert_amd.mean_var_norm(x, -1, None, None, 1e-38)[1].cpu().numpy()
    exp = xn.astype(np.float64).std(0)
    assert np.abs(stats[1] / exp - 1).max() < 1e-9
    assert np.abs(stats[0] / xn.astype(np.float64).mean(0) - 1).max() < 1e-12


def test_determinism_and_streams():
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    x = torch.randn(64, 300, 80, device=DEV)

    def run():
        m = M.MeanVarianceNormalization()
        m.accumulate(x)
        m.accumulate(x[:7])
        out = torch.ops.pydrobert_amd.mean_var_norm(x, -1, None, None, 1e-38)
        return [F.feat_deltas(x), out[0], out[1], m.count, m.sum, m.sumsq, F.mean_var_norm(x, 1)]

    a = run()
    b = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = run()
    torch.cuda.current_stream().wait_stream(s)
    for p, q, r in zip(a, b, c):
        assert torch.equal(p, q) and torch.equal(p, r)


def test_accumulate_100_chunks_and_store():
    from pydrobert_amd import modules as M

    rng = np.random.default_rng(11)
    chunks = [(rng.standard_normal((int(rng.integers(1, 50)), 20, 40)) * 3 + 7).astype(np.float32) for _ in range(100)]
    m = M.MeanVarianceNormalization(dim=-1)
    for c in chunks:
        m.accumulate(torch.from_numpy(c).to(DEV))
    allx = np.concatenate([c.reshape(-1, 40) for c in chunks]).astype(np.float64)
    assert m.count.item() == allx.shape[0]
    assert np.allclose(m.sum.cpu().numpy(), allx.sum(0), rtol=1e-12, atol=0)
    assert np.allclose(m.sumsq.cpu().numpy(), np.square(allx).sum(0), rtol=1e-12, atol=0)
    m.store(delete_stats=False)
    assert np.allclose(m.mean.cpu().numpy(), allx.mean(0), rtol=1e-12, atol=0)
    assert np.allclose(m.std.cpu().numpy(), allx.std(0), rtol=1e-9, atol=0)
    m.store(bessel=True)
    assert np.allclose(m.std.cpu().numpy(), allx.std(0, ddof=1), rtol=1e-9, atol=0)
    assert m.count is None
    m2 = M.MeanVarianceNormalization()
    m2.accumulate(torch.randn(1, 5, device=DEV))
    with pytest.raises(RuntimeError):
        m2.store()


def _ulps(a, b, dtype):
    eps = torch.finfo(dtype).eps
    scale = b.abs().clamp_min(torch.finfo(dtype).tiny)
    return ((a.double() - b.double()).abs() / (scale.double() * eps)).max().item()


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16, torch.float64))
def test_dtypes(dtype):
    from pydrobert_amd import functional as F

    x = torch.randn(4, 50, 24, device=DEV).to(dtype)
    y = F.feat_deltas(x)
    exp = ref_deltas(x.double())
    assert y.dtype == dtype
    if dtype == torch.float64:
        assert (y - exp).abs().max().item() < 1e-12
    else:
        # 2 ulps of the float64 restatement rounded to the dtype, or an absolute ulp near zero
        d = (y.double() - exp.to(dtype).double()).abs()
        ulp = exp.to(dtype).double().abs().clamp_min(1.0) * torch.finfo(dtype).eps
        assert (d <= 2 * ulp).all()
    z = F.mean_var_norm(x, -1)
    assert z.dtype == dtype
    expz = ref_mvn(x.double() if dtype == torch.float64 else x, -1)
    if dtype == torch.float64:
        assert (z - expz).abs().max().item() < 1e-12
    else:
        d = (z.double() - expz.to(dtype).double()).abs()
        ulp = expz.to(dtype).double().abs().clamp_min(1.0) * torch.finfo(dtype).eps
        assert (d <= 2 * ulp).all()


def test_traceable_on_device():
    from pydrobert_amd import modules as M

    x = torch.randn(3, 20, 8, device=DEV)
    for mod in (M.FeatureDeltas().to(DEV), M.FeatureDeltas(1, 1, False, 1, 3, "reflect").to(DEV),
                M.MeanVarianceNormalization(-1).to(DEV)):
        exp = mod(x)
        assert torch.allclose(torch.jit.script(mod)(x), exp)
        assert torch.allclose(torch.jit.trace(mod, x)(x), exp)
        assert torch.allclose(torch.compile(mod, backend="eager")(x), exp)
    sm = torch.jit.script(M.MeanVarianceNormalization())
    sm.accumulate(x)
    sm.accumulate(x)
    sm.store()
    assert sm.mean.device == x.device and sm(x).shape == x.shape


def test_no_host_synchronisation():
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    x = torch.randn(8, 100, 40, device=DEV, requires_grad=True)
    m = M.MeanVarianceNormalization()
    m.accumulate(x.detach())
    mod = M.FeatureDeltas(pad_mode="constant", value=1.0).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = F.mean_var_norm(mod(x), -1) + F.feat_deltas(x, order=3, width=1, pad_mode="circular").sum()
        y.backward(torch.ones_like(y))
        m.accumulate(x.detach())
        F.mean_var_norm(x.detach(), -1, m.sum, m.sumsq)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_given_statistics_strided():
    """A given mean / std that are strided views (columns of one (X, 2) tensor) read element by element."""
    from pydrobert_amd import functional as F

    x = torch.randn(5, 6, 7, dtype=torch.float64) * 2 + 1
    both = torch.stack([torch.randn(7, dtype=torch.float64), torch.rand(7, dtype=torch.float64) + 0.5], 1)
    g = upstream((5, 6, 7), torch.float64, device="cpu")
    res = []
    for dev in ("cpu", DEV):
        xs = x.to(dev).requires_grad_(True)
        st = both.to(dev).requires_grad_(True)
        mean, std = st[:, 0], st[:, 1]
        assert mean.stride() == (2,) and std.stride() == (2,)
        outs = [F.mean_var_norm(xs, -1, mean), F.mean_var_norm(xs, -1, None, std), F.mean_var_norm(xs, -1, mean, std)]
        y = torch.stack(outs)
        grads = torch.autograd.grad(y, (xs, st), torch.stack([g, g, g]).to(dev))
        res.append([t.detach().cpu() for t in (y,) + grads])
    for a, b in zip(*res):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
def test_wide_halo_without_lds(dtype):
    """1 + 2P rows of one column vector beyond 64 KiB of LDS: the kernel without a tile."""
    from pydrobert_amd import functional as F

    kw = dict(order=2, width=1100)  # P = 2200
    x = torch.randn(2, 50, 4, device=DEV, dtype=dtype, requires_grad=True)
    y = F.feat_deltas(x, **kw)
    exp = ref_deltas(x.detach(), **kw)
    assert (y.double() - exp).abs().max().item() < (1e-5 if dtype == torch.float32 else 1e-12)
    (gx,) = torch.autograd.grad(y, x, upstream(tuple(y.shape), dtype))
    xc = x.detach().cpu().requires_grad_(True)
    (gc,) = torch.autograd.grad(F.feat_deltas(xc, **kw), xc, upstream(tuple(y.shape), dtype, device="cpu"))
    assert (gx.cpu().double() - gc.double()).abs().max().item() < (1e-4 if dtype == torch.float32 else 1e-12)


def test_cached_taps_filled_on_another_stream():
    """The built taps are copied on the stream of the first call; a later call on another stream waits."""
    from pydrobert_amd import _feats
    from pydrobert_amd import functional as F

    x = torch.randn(4, 40, 16, device=DEV)
    for key in [k for k in _feats._TAPS if k[:2] == (3, 3)]:
        del _feats._TAPS[key]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.feat_deltas(x, order=3, width=3)
    y = F.feat_deltas(x, order=3, width=3)
    torch.cuda.synchronize()
    assert (y.double() - ref_deltas(x, order=3, width=3)).abs().max().item() < 1e-5


# ----------------------------------------------------------------------------------------------------------
# every tile and launch form, against the references of tests/_feats_ref.py (numpy float64 for the values,
# autograd through float64 torch restatements for the gradients; pinned to the goldens and to the CPU bodies
# in tests/test_feats_cpu.py).  The plan named with each case is what pdt_feat_deltas / mvn_splits choose for
# it: EC columns x TT time rows per tile, column tiles x time tiles per (a, b) row.

import _feats_ref as R  # noqa: E402


def _close(act, exp, dtype, scale=1.0):
    """The suite's bounds against a float64 reference: 1e-5 absolute in float32, 1e-12 in float64, 2 ulps of
    the reference rounded to a 16-bit dtype (an absolute ulp below 1); ``scale`` widens them for gradients."""
    act = act.detach().cpu()
    exp = torch.as_tensor(np.ascontiguousarray(exp)) if not torch.is_tensor(exp) else exp.detach().cpu()
    assert act.dtype == dtype and act.shape == exp.shape, (act.dtype, act.shape, exp.shape)
    if dtype in (torch.float16, torch.bfloat16):
        e = exp.to(dtype).double()
        d = (act.double() - e).abs() / (e.abs().clamp_min(1.0) * torch.finfo(dtype).eps * scale)
        return d.max().item() <= 2.0
    return (act.double() - exp.double()).abs().max().item() <= (1e-5 if dtype == torch.float32 else 1e-12) * scale


def _check_deltas(x, kw, mode, taps=None, grad_out=None, module=None):
    """Forward and gradient of one feat_deltas call on the device against the references.  ``x`` may be any
    view; ``taps`` (float64, CPU) are passed as the caller's own filters, else the built ones are used."""
    from pydrobert_amd import _feats
    from pydrobert_amd import functional as F

    dtype = x.dtype
    value = -0.5 if mode == "constant" else 0.0
    geo = dict(dim=kw.get("dim", -1), time_dim=kw.get("time_dim", -2), concatenate=kw.get("concatenate", True),
               pad_mode=mode, value=value)
    ref_taps = _feats._feat_delta_filters(kw["order"], kw["width"]).double() if taps is None else taps
    xg = x.detach().requires_grad_(True)
    if module is not None:
        y = module(xg)
    else:
        y = F.feat_deltas(xg, order=kw["order"], width=kw["width"], _filters=None if taps is None else taps.to(DEV), **geo)
    xc = x.detach().cpu().double().requires_grad_(True)
    exp = R.deltas_ref(xc.detach().numpy(), ref_taps.numpy(), **geo)
    assert _close(y, exp, dtype), (kw, mode)
    g = R.upstream(tuple(y.shape), dtype) if grad_out is None else grad_out
    (gx,) = torch.autograd.grad(y, xg, g.to(DEV))
    (ge,) = torch.autograd.grad(R.deltas_torch(xc, ref_taps, **geo), xc, g.double())
    assert _close(gx, ge, dtype, max(1.0, ge.abs().max().item())), (kw, mode)


_DELTA_PARAMS = [pytest.param(c, m, id="{}-{}".format(c[0], m)) for c in R.DELTA_CASES for m in c[4]]


@pytest.mark.parametrize("case,mode", _DELTA_PARAMS)
def test_deltas_every_tile_form(case, mode):
    """float32 vector form (EC 256): (2, 40, 260) is TT 16, 2 column tiles (the last one vector wide) x 3 time
    tiles (the last partial), with the order axis in each place; (2, 40, 5, 60) has C = 5 rows of D = 60
    across the column tiles.  Scalar form (EC 64): (2, 150, 70) is TT 64, 2 x 3 tiles, the last 6 columns
    wide.  float64 (2, 40, 130): EC 128, TT 32, 2 x 2.  16-bit (2, 20, 520): EC 512, TT 8, 2 x 3.  The shrink
    loop: P = 40 gives TT 16 -> 8, EC 256 -> 128, 2 x 8 tiles; P = 300 gives EC 16, TT 8, 16 x 40 tiles.  The
    last P of the tile form launches with 65520 (float32 vector), 65532 (float32 scalar), 65520 (float64)
    and 65504 (float16) bytes of LDS, and P + 1 is the first of the kernel without LDS.  Circular with
    P == T and reflect with P == T - 1 are the widest halos those modes accept."""
    name, shape, dtype, kw, _ = case
    _check_deltas(R.delta_input(shape, dtype).to(DEV), kw, mode)


@pytest.mark.parametrize("mode", MODES)
def test_deltas_strided_c_across_column_tile(mode):
    """(2, 40, 5, 60) as a transposed view of (2, 5, 40, 60): the C axis has a stride of its own
    (xs_c = 2400, not D), read through by the vector form."""
    base = R.delta_input((2, 5, 40, 60), "float32").to(DEV)
    x = base.transpose(1, 2)
    assert not x.is_contiguous()
    _check_deltas(x, dict(order=2, width=2, time_dim=1, dim=3), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,order,width", [((2, 40, 260), 2, 2), ((3, 9, 5), 2, 2), ((3, 9, 5), 3, 1)],
                         ids=("vec-2coltiles", "small", "small-order3"))
def test_deltas_filters_of_the_callers_own(shape, order, width, mode):
    """Random (U, K) taps -- neither symmetric nor antisymmetric, so a wrong tap index in the forward or the
    adjoint changes a value -- through ``_filters`` and through a module whose ``filters`` buffer is
    overwritten."""
    from pydrobert_amd import modules as M

    g = torch.Generator().manual_seed(order * 100 + width)
    taps = torch.randn(order + 1, 1 + 2 * order * width, generator=g, dtype=torch.float64)
    x = R.delta_input(shape, "float32").to(DEV)
    kw = dict(order=order, width=width)
    _check_deltas(x, kw, mode, taps=taps.float().double())
    mod = M.FeatureDeltas(order=order, width=width, pad_mode=mode, value=-0.5 if mode == "constant" else 0.0).to(DEV)
    mod.filters.copy_(taps)
    _check_deltas(x, kw, mode, taps=mod.filters.detach().cpu().double(), module=mod)


@pytest.mark.parametrize("mode", MODES)
def test_deltas_expanded_and_offset_inputs(mode):
    """A batch expanded with stride 0; x[..., 1:] of a 16-byte aligned base, whose rows start 4 bytes past an
    aligned address; and a view whose pointer alone is off.  The vector form must be refused for both."""
    kw = dict(order=2, width=2)
    x = R.delta_input((1, 40, 260), "float32").to(DEV).expand(3, 40, 260)
    assert x.stride(0) == 0
    _check_deltas(x, kw, mode)
    base = R.delta_input((2, 40, 261), "float32").to(DEV)
    assert base.data_ptr() % 16 == 0
    _check_deltas(base[..., 1:], kw, mode)  # D = 260, but rows 261 apart
    flat = R.delta_input((2 * 40 * 264 + 4,), "float32").to(DEV)
    off = flat[1:].as_strided((2, 40, 260), (40 * 264, 264, 1))
    assert off.data_ptr() % 16 == 4  # D and every stride a multiple of 4 elements: only the pointer is off
    _check_deltas(off, kw, mode)


@pytest.mark.parametrize("mode", MODES)
def test_deltas_gradient_through_sum(mode):
    """y.sum() hands the adjoint an expanded grad_out (every stride 0), made contiguous ahead of the kernel.
    Random taps: rows of built ones sum to 0 or 1, which would leave little to compare."""
    from pydrobert_amd import functional as F

    taps = torch.randn(3, 9, generator=torch.Generator().manual_seed(7)).double()
    x = R.delta_input((2, 40, 260), "float32").to(DEV).requires_grad_(True)
    value = -0.5 if mode == "constant" else 0.0
    F.feat_deltas(x, pad_mode=mode, value=value, _filters=taps.to(DEV)).sum().backward()
    xc = x.detach().cpu().double().requires_grad_(True)
    R.deltas_torch(xc, taps, pad_mode=mode, value=value).sum().backward()
    assert _close(x.grad, xc.grad, torch.float32, max(1.0, xc.grad.abs().max().item()))


def _mvn_tols(dtype):
    return dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1e-12, atol=1e-12)


def _check_mvn(x, dim):
    """y, the float64 statistics, the gradients in the four given / computed forms, and accumulate (twice) +
    store of one input on the device.  16-bit y: within MVN_16BIT_CPU_ULPS + 1 ulps of mvn_ref_rounded (see
    tests/_feats_ref.py); 16-bit gradients: within 2 ulps of the package's CPU body, which states the same
    formula in torch with the same roundings of the mean and of x - mean (a float64 graph rounds neither)."""
    from pydrobert_amd import modules as M

    dtype, shape = x.dtype, tuple(x.shape)
    narrow = dtype in (torch.float16, torch.bfloat16)
    X = shape[dim]
    xg = x.to(DEV)
    xn = x.double().numpy()
    y, stats = torch.ops.pydrobert_amd.mean_var_norm(xg, dim, None, None, R.TINY)
    exp, m, s = R.mvn_ref(xn, dim)
    assert y.dtype == dtype and stats.dtype == torch.float64
    st = stats.cpu().numpy()
    assert (np.abs(st[0] - m) <= 1e-12 * np.maximum(1.0, np.abs(m))).all(), (shape, dim)
    assert np.abs(st[1] / s - 1).max() <= 1e-9, (shape, dim)
    if narrow:
        worst = R.ulps(y, R.mvn_ref_rounded(x, dim)[0], dtype)
        print("mvn {} {} dim {}: {} ulps from mvn_ref_rounded".format(dtype, shape, dim, worst))
        assert worst <= R.MVN_16BIT_CPU_ULPS + 1.0, (shape, dim, worst)
    else:
        assert np.allclose(y.cpu().numpy(), exp, **_mvn_tols(dtype)), (shape, dim)
    # gradients
    cdt = torch.float32 if narrow else dtype
    given_m = R.mvn_input((X,), cdt, seed=1)
    given_s = R.mvn_input((X,), cdt, seed=2).abs() + 0.5
    g = R.upstream(shape, dtype)
    for mean, std in ((None, None), (given_m, None), (None, given_s), (given_m, given_s)):
        ins = [t.to(DEV).requires_grad_(True) if t is not None else None for t in (x, mean, std)]
        yg = torch.ops.pydrobert_amd.mean_var_norm(ins[0], dim, ins[1], ins[2], R.TINY)[0]
        act = torch.autograd.grad(yg, [t for t in ins if t is not None], g.to(DEV))
        ins = [t.clone().requires_grad_(True) if t is not None else None for t in (x, mean, std)]
        if narrow:
            yc = torch.ops.pydrobert_amd.mean_var_norm(ins[0], dim, ins[1], ins[2], R.TINY)[0]
            assert R.ulps(yg, yc.detach().double().numpy(), dtype) <= 1.0, (shape, dim)
            ref = torch.autograd.grad(yc, [t for t in ins if t is not None], g)
            assert R.ulps(act[0], ref[0].double().numpy(), dtype) <= 2.0, (shape, dim)
            for a, b in zip(act[1:], ref[1:]):
                assert np.allclose(a.cpu().numpy(), b.numpy(), rtol=1e-5, atol=1e-5), (shape, dim)
        else:
            yr = R.mvn_torch(ins[0], dim, ins[1], ins[2])
            assert np.allclose(yg.detach().cpu().numpy(), yr.detach().numpy(), **_mvn_tols(dtype)), (shape, dim)
            ref = torch.autograd.grad(yr, [t for t in ins if t is not None], g.double())
            for a, b in zip(act, ref):
                assert np.allclose(a.cpu().numpy(), b.numpy(), **_mvn_tols(dtype)), (shape, dim, mean is None, std is None)
    # accumulate twice, store
    x2 = R.mvn_input(shape, dtype, seed=3)
    mod = M.MeanVarianceNormalization(dim=dim)
    mod.accumulate(xg)
    mod.accumulate(x2.to(DEV))
    both = np.moveaxis(np.stack([xn, x2.double().numpy()]), dim % len(shape) + 1, -1).reshape(-1, X)
    assert mod.count.item() == both.shape[0]
    assert np.allclose(mod.sum.cpu().numpy(), both.sum(0), rtol=1e-12, atol=0), (shape, dim)
    assert np.allclose(mod.sumsq.cpu().numpy(), np.square(both).sum(0), rtol=1e-12, atol=0), (shape, dim)
    mod.store()
    em = both.mean(0)
    assert (np.abs(mod.mean.cpu().numpy() - em) <= 1e-12 * np.maximum(1.0, np.abs(em))).all(), (shape, dim)
    assert np.abs(mod.std.cpu().numpy() / both.std(0) - 1).max() <= 1e-9, (shape, dim)


@pytest.mark.parametrize("shape,dim", R.MVN_CASES, ids=str)
def test_mvn_every_launch_form(shape, dim):
    """B == 1 (mvn_partial_cols): (300, 300) is two column tiles with RP 1, 10 splits of 30 rows (the
    unrolled sweep plus a remainder); (40, 257) has one column in the second tile, (500, 255) one idle lane;
    (1000, 80) is RP 3 with 16 idle lanes, 11 splits; (20000, 1) is X = 1, RP 256, 3 splits.  B > 1
    (mvn_partial_inner): (37, 3, 301) is B > 256 (da = 0), 2 splits, the second starting mid-row (m0 = 5569:
    ia 18, ib 151); (5000, 4, 3) is da 85, db 1, 2 splits; (6, 9000) dim 0 is A = 1, 2 splits; (3, 5, 300)
    is B > 256 in one split, ib wrapping.  (10, 6) and (4, 9): X % 4 != 0 with a total that is a multiple
    of 4, the index wrapping inside a 16-byte vector of the apply kernel."""
    _check_mvn(R.mvn_input(shape, torch.float32), dim)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=str)
@pytest.mark.parametrize("shape,dim", R.MVN_CASES_16, ids=str)
def test_mvn_every_launch_form_16bit(shape, dim, dtype):
    """(16, 3): X < V = 8, the index wrapping twice inside one vector; (8, 12): X % 8 != 0; the split forms
    of (37, 3, 301) dim 1 and (1000, 80) dim -1 in the 16-bit types."""
    _check_mvn(R.mvn_input(shape, dtype), dim)


def test_mvn_misaligned_rows_take_the_scalar_apply():
    """x[1:] of (11, 6) float32 is contiguous, 60 elements, but starts 24 bytes into its allocation."""
    x = R.mvn_input((11, 6), torch.float32).to(DEV)[1:]
    assert x.is_contiguous() and x.data_ptr() % 16 == 8 and x.numel() % 4 == 0
    y, stats = torch.ops.pydrobert_amd.mean_var_norm(x, -1, None, None, R.TINY)
    exp, m, s = R.mvn_ref(x.cpu().double().numpy(), -1)
    assert np.allclose(y.cpu().numpy(), exp, rtol=1e-5, atol=1e-5)
    assert np.abs(stats[1].cpu().numpy() / s - 1).max() <= 1e-9
    xg = x.detach().requires_grad_(True)
    g = R.upstream((10, 6), torch.float32)
    (gx,) = torch.autograd.grad(torch.ops.pydrobert_amd.mean_var_norm(xg, -1, None, None, R.TINY)[0], xg, g.to(DEV))
    xc = x.detach().cpu().requires_grad_(True)
    (ge,) = torch.autograd.grad(R.mvn_torch(xc, -1), xc, g.double())
    assert np.allclose(gx.cpu().numpy(), ge.numpy(), rtol=1e-5, atol=1e-5)
