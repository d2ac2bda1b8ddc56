"""GPU: SpecAugment on float16 / bfloat16 features.  A half call is the float32 call on the exactly widened
features with each result rounded once where it is stored, so every route is held to the BIT against the float32
operators of this package on the widened features (``feats.float()``'s values behind ``feats``' own layout, so
that both calls take the same kernel form; ``grad_out.float()``), the result ``.to(dtype)``: the explicit
grid, the fused warp and ``SpecAugment.forward`` for every forward case of tests/_half_spec.py (each kernel form,
layouts on 2-byte boundaries, strided and transposed views, tiny lengths, masks only); planted infinities, NaNs,
largest finite values, subnormals and bfloat16 ties; the gather adjoint for any grid; the scatter adjoint on
inputs whose sums are exact, and within one ulp of the dtype on random ones; the one-to-one adjoint; the gradient
through the module.  No float32 copy of the features or of the gradient is made."""
import functools

import numpy as np
import pytest
import torch

import _half_spec as hs
from pydrobert_amd import functional as F
from pydrobert_amd import modules as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTNAMES = list(hs.DTYPES)
ops = torch.ops.pydrobert_amd


def _opt(m):
    return m if m.numel() else None


def _grids(x, params, lens, order):
    """The explicit-grid route's arguments from a case's parameters: float32 grids (None where not warped) and
    int64 masks (None where there are none)."""
    w_0, w, v_0, v, t_0, t, f_0, f = params
    N, T, Fq = x.shape
    tg = F.warp_1d_grid(w_0, w, lens, T, order) if w_0.numel() else None
    fg = F.warp_1d_grid(v_0, v, torch.full((N,), Fq, device=x.device), Fq, order) if v_0.numel() else None
    return tg, fg, _opt(t_0), _opt(t), _opt(f_0), _opt(f)


def _module(c):
    return M.SpecAugment(
        max_time_warp=8.0 if c["tw"] else 0.0, max_freq_warp=1.0 if c["fw"] else 0.0, max_time_mask=6,
        max_freq_mask=3, max_time_mask_proportion=0.5, num_time_mask=2, num_time_mask_proportion=0.5,
        num_freq_mask=1, interpolation_order=c["order"]).to(DEV)  # fmt: skip


@functools.lru_cache(maxsize=None)
def fwd_reference(name):
    """{dtname: (grid route, parameter route, module route)}: the float32 operators' results on the case's
    features as the half dtype holds them, widened, each rounded to that dtype.  Cached: treat as read-only."""
    c = hs.FWD_CASES[name]
    out = {}
    for dtname, dt in hs.DTYPES.items():
        x, params, lens, order = hs.fwd_tensors(name, dt, DEV)
        xf = hs.widened(x, c)
        assert xf.stride() == x.stride() and torch.equal(xf, x.float())
        a = ops.spec_augment_apply(xf, *_grids(xf, params, lens, order))
        b = F.spec_augment_apply_parameters(xf, params, order, lens)
        torch.manual_seed(1234)
        m = _module(c)(xf, lens)
        out[dtname] = tuple(r.to(dt) for r in (a, b, m))
    return out


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", sorted(hs.FWD_CASES))
def test_forward_to_the_bit(name, dtname):
    """The three routes of a case give, in the features' dtype, the bit patterns of the float32 operators' results
    rounded once; the features keep their strides on the way to the kernel (the plan query's form for the very
    tensor is the table's); masked bands are +0."""
    from pydrobert_amd import _cabi

    c, dt = hs.FWD_CASES[name], hs.DTYPES[dtname]
    x, params, lens, order = hs.fwd_tensors(name, dt, DEV)
    st = hs.layout_of(c)[1]
    assert x.stride() == st and x.dtype == dt
    form = _cabi.lib().pdt_spec_augment_apply_form(
        c["N"], c["T"], c["F"], st[0], st[1], st[2], x.data_ptr(), 0, int(c["tw"]), int(c["fw"]), 0, hs.ELEM[dtname])
    assert form == c["fwd"], (name, form)
    ref_a, ref_b, ref_m = fwd_reference(name)[dtname]
    act_a = ops.spec_augment_apply(x, *_grids(x, params, lens, order))
    act_b = F.spec_augment_apply_parameters(x, params, order, lens)
    torch.manual_seed(1234)
    act_m = _module(c)(x, lens)
    for route, act, ref in (("grid", act_a, ref_a), ("parameters", act_b, ref_b), ("module", act_m, ref_m)):
        assert act.dtype == dt and act.shape == x.shape and act.is_contiguous(), route
        assert hs.same_bits(act, ref), (name, route)
    t_0, t, f_0, f = (p.cpu().numpy() for p in params[4:])
    bits = act_b.view(torch.int16).cpu().numpy()
    for n in range(c["N"]):
        for m in range(t.shape[1]):
            assert (bits[n, t_0[n, m] : t_0[n, m] + t[n, m]] == 0).all()
        for m in range(f.shape[1]):
            assert (bits[n, :, f_0[n, m] : f_0[n, m] + f[n, m]] == 0).all()
    if not c["tw"]:  # masks only: an exact copy of the kept bits
        keep = bits != 0
        assert (bits[keep] == x.contiguous().view(torch.int16).cpu().numpy()[keep]).all() and keep.mean() > 0.5


@pytest.mark.parametrize("dtname", DTNAMES)
def test_empty_batches_and_bad_lengths(dtname):
    """N = 0 and T = 0 give empty results of the features' dtype on every route; lengths outside [1, T] raise the
    reference's error for half features exactly as for float32, from the fused route and from the grid route."""
    dt = hs.DTYPES[dtname]
    e = torch.empty(0)
    for shape in ((0, 20, 8), (3, 0, 8)):
        x = torch.zeros(shape, dtype=dt, device=DEV)
        N = shape[0]
        lens = torch.full((N,), max(shape[1], 1), device=DEV)
        params = (torch.full((N,), 3.0, device=DEV), torch.ones(N, device=DEV), e, e,
                  torch.zeros(N, 1, dtype=torch.long, device=DEV), torch.ones(N, 1, dtype=torch.long, device=DEV), e, e)
        out = ops.spec_augment_apply(x, None, None, params[4], params[5], None, None)
        assert out.dtype == dt and out.shape == x.shape
        if shape[1]:
            out = F.spec_augment_apply_parameters(x, params, 1, lens)
            assert out.dtype == dt and out.shape == x.shape
        g = ops.spec_augment_apply_backward(x, None, None, params[4], params[5], None, None)
        assert g.dtype == dt and g.shape == x.shape
    N, T, Fq = 3, 20, 8
    params = (torch.full((N,), 8.0, device=DEV), torch.ones(N, device=DEV), e, e, e, e, e, e)
    sa = M.SpecAugment(max_time_warp=4.0).to(DEV)
    for d in (dt, torch.float32):
        for Fx in (Fq, 7):  # (the rows kernel judges the lengths itself; the general kernel's route asks the host)
            x = torch.randn(N, T, Fx, device=DEV).to(d)
            for bad in (torch.tensor([20, 21, 5], device=DEV), torch.tensor([20, 0, 5], device=DEV)):
                with pytest.raises(RuntimeError, match=r"values of lengths must be between \(1, 20\)"):
                    F.spec_augment_apply_parameters(x, params, 1, bad)
                with pytest.raises(RuntimeError, match=r"values of lengths must be between \(1, 20\)"):
                    sa(x, bad)


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("layout", ["contig", "offset1"])
def test_planted_values(layout, dtname):
    """Non-finite values under a mask give exactly +0 (selected, never multiplied); a NaN in the open reaches the
    two output rows whose taps read it and no other; two neighbouring rows of the largest finite value blend to
    it; float16 subnormals and the bfloat16 ties round to nearest even -- on the rows kernel (contiguous) and on
    the general kernel (rows on 2-byte boundaries), to the bit of the float32 operator's rounded result."""
    dt = hs.DTYPES[dtname]
    xs, t_0, t, f_0, f = hs.planted(dt)
    c = dict(N=2, T=hs.PLANT_T, F=hs.PLANT_F, layout=layout)
    x = hs.strided(torch.from_numpy(xs), c, dt, DEV)
    grid = torch.from_numpy(hs.halfway_grid(2)[0]).to(DEV)
    masks = tuple(torch.from_numpy(m).to(DEV) for m in (t_0, t, f_0, f))
    act = ops.spec_augment_apply(x, grid, None, *masks)
    ref = ops.spec_augment_apply(hs.widened(x, c), grid, None, *masks).to(dt)
    assert act.dtype == dt and hs.same_bits(act, ref)
    bits = act.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF
    a = act.float().cpu().numpy()
    assert (bits[:, 0:3] == 0).all() and (bits[:, :, 0] == 0).all()  # +0 under the masks, not -0, not NaN
    nan = np.isnan(a)
    assert nan[:, 4:6, 1:].all() and nan.sum() == 2 * 2 * 7
    assert (a[:, 8, 1:] == float(torch.finfo(dt).max)).all()
    if dt == torch.float16:
        assert (a[:, 10, 1:] == 2.0 ** -23).all() and (a[:, 11, 1:] == 2.0 ** -23).all()
    else:
        assert (a[:, 10, 1:] == 1.5 * 2.0 ** -24).all() and (a[:, 11, 1:] == 2.5 * 2.0 ** -24).all()
        for col, (_, _, even) in enumerate(hs.BF16_TIES):
            assert (bits[:, 13, col + 1] == even).all(), (col, hex(bits[0, 13, col + 1]))


def _backward(g, rest):
    return ops.spec_augment_apply_backward(g, *rest)


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", hs.BIT_BWD)
def test_backward_to_the_bit(name, dtname):
    """Gather (monotone and arbitrary grids, two tiles, no grid), one-to-one, and the scatter on the dyadic inputs
    whose float32 sums are exact in any order (tests/test_half_spec_cpu.py): the gradient has the bit patterns of
    the float32 operator's on ``grad_out.float()``, rounded once.  The same call twice gives the same bits."""
    dt = hs.DTYPES[dtname]
    g, *rest = hs.bwd_tensors(name, dt, DEV)
    act = _backward(g, rest)
    ref = _backward(g.float(), rest)
    assert act.dtype == dt and ref.dtype == torch.float32 and act.shape == g.shape
    assert hs.same_bits(act, ref.to(dt)), name
    assert hs.same_bits(act, _backward(g, rest)), name
    assert bool(act.float().abs().sum() > 0)


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", hs.RANDOM_SCATTER)
def test_scatter_backward_within_one_ulp(name, dtname):
    """Random grids and gradients on the scatter form: the order of the float32 atomic additions is not fixed, so
    the half call's sums and the reference's may differ by float32 roundings, far below a half ulp of the dtype,
    before each is rounded once: |act - ref| <= ulp(|ref|)."""
    dt = hs.DTYPES[dtname]
    g, *rest = hs.bwd_tensors(name, dt, DEV)
    act = _backward(g, rest)
    ref = _backward(g.float(), rest).to(dt)
    assert act.dtype == dt
    err, ulp = (act.float() - ref.float()).abs(), hs.ulp_of(ref)
    print(name, dtname, "max |act - ref| / ulp:", float((err / ulp).max()), "differing:", int((err > 0).sum()))
    assert bool((err <= ulp).all()), float((err / ulp).max())


@pytest.mark.parametrize("dtname", DTNAMES)
def test_gradient_through_the_module(dtname):
    """torch.autograd.grad through SpecAugment.forward on half features is, bit for bit, the gradient through the
    float32 module on the widened features rounded to the dtype (same seed, so the same parameters)."""
    dt = hs.DTYPES[dtname]
    N, T, Fq = 4, 120, 16
    torch.manual_seed(5)
    feats = torch.randn(N, T, Fq, device=DEV).to(dt)
    lens = torch.tensor([120, 90, 77, 31], device=DEV)
    g = torch.randn(N, T, Fq, device=DEV).to(dt)
    sa = M.SpecAugment(max_time_warp=12.0, max_time_mask=10, max_time_mask_proportion=0.5, num_time_mask=2,
                       num_time_mask_proportion=0.5, max_freq_mask=4, num_freq_mask=1).to(DEV)  # fmt: skip
    xh = feats.clone().requires_grad_(True)
    torch.manual_seed(77)
    yh = sa(xh, lens)
    (gh,) = torch.autograd.grad(yh, xh, g)
    xf = feats.float().requires_grad_(True)
    torch.manual_seed(77)
    yf = sa(xf, lens)
    (gf,) = torch.autograd.grad(yf, xf, g.float())
    assert yh.dtype == dt and gh.dtype == dt
    assert hs.same_bits(yh.detach(), yf.detach().to(dt)) and hs.same_bits(gh, gf.to(dt))
    assert bool((gh == 0).any()) and bool((gh != 0).any())


def _growth(fn):
    """Peak growth of allocated device memory across one call of ``fn`` (after a warm-up call), and its result."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


@pytest.mark.parametrize("dtname", DTNAMES)
def test_no_float32_copy(dtname):
    """One ``spec_augment_apply_parameters`` call with a time warp and masks on (8, 512, 80) half features grows
    the allocated memory by at most 1.5 times the output's N T F 2 bytes (the output itself, the parameters and
    allocator rounding; a widened copy, a float32 result and its narrowing would need 5 times), and so does the
    rows-route backward for its ``grad``."""
    dt = hs.DTYPES[dtname]
    N, T, Fq = 8, 512, 80
    bound = 1.5 * N * T * Fq * 2
    torch.manual_seed(3)
    x = torch.randn(N, T, Fq, device=DEV).to(dt)
    lens = torch.randint(T // 2, T + 1, (N,), device=DEV)
    e = torch.empty(0)
    params = (lens.float() / 2, torch.full((N,), 5.0, device=DEV), e, e,
              torch.randint(0, 200, (N, 2), device=DEV), torch.randint(0, 30, (N, 2), device=DEV),
              torch.randint(0, 60, (N, 2), device=DEV), torch.randint(0, 10, (N, 2), device=DEV))  # fmt: skip
    grew, out = _growth(lambda: F.spec_augment_apply_parameters(x, params, 1, lens))
    print(dtname, "forward growth", grew, "bound", bound)
    assert out.dtype == dt and grew <= bound, (grew, bound)
    tgrid = F.warp_1d_grid(params[0], params[1], lens, T, 1)
    g = torch.randn(N, T, Fq, device=DEV).to(dt)
    grew, grad = _growth(lambda: ops.spec_augment_apply_backward(g, tgrid, None, *params[4:]))
    print(dtname, "backward growth", grew, "bound", bound)
    assert grad.dtype == dt and grew <= bound, (grew, bound)


@pytest.mark.parametrize("dtname", DTNAMES)
def test_opcheck_with_half_features(dtname):
    """Schemas, fake kernels (the features' dtype and shape) and autograd registrations of the four operators hold
    for half features, one case per operator."""
    from torch.library import opcheck

    dt = hs.DTYPES[dtname]
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    x, params, lens, order = hs.fwd_tensors("rows-two-tiles", dt, DEV)
    grids = _grids(x, params, lens, order)
    xr = x.clone().requires_grad_(True)
    opcheck(ops.spec_augment_apply.default, (xr,) + grids, test_utils=utils)
    opcheck(ops.spec_augment_apply_warp.default,
            (xr, params[0], params[1], lens, order) + grids[2:] + (True,), test_utils=utils)  # fmt: skip
    opcheck(ops.spec_augment_apply_backward.default, (x,) + grids, test_utils=("test_schema", "test_faketensor"))
    u = torch.rand(x.shape[0], 2 + 4 + 2, device=DEV)
    opcheck(ops.spec_augment_forward.default, (xr, u, lens, 8.0, 6, 3, 0.5, 2, 0.5, 1, order), test_utils=utils)
