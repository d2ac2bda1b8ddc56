"""GPU: the gradients of the image warps with respect to where they sample -- dense_image_warp's flow
(csrc/image_warp.hip, WARP_POSITION), sparse_image_warp's control points (the same kernel chained into
csrc/spline.hip's pdt_spline_eval_adjoint) and the spline evaluation's adjoint alone -- against the float64
yardstick of tests/_warp_grad_ref.py, whose inputs and conditions tests/test_warp_grads_cpu.py pins without
a GPU."""
import numpy as np
import pytest
import torch

import _img_ref as R
import _warp_grad_ref as G
from pydrobert_amd import functional as F

pytestmark = pytest.mark.gpu


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---------------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------------
_DENSE_REF = {}


def _dense_ref(shape, dtype, indexing, padding):
    """The float64 gradients of one dense case, computed once."""
    key = (shape, np.dtype(dtype).name, indexing, padding)
    if key not in _DENSE_REF:
        image, flow, g = G.dense_input(shape, dtype)
        _DENSE_REF[key] = G.dense_flow_grad(image, G.dense_flow(flow, indexing), g, indexing, "bilinear", padding)
    return _DENSE_REF[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("indexing", R.INDEXINGS)
@pytest.mark.parametrize("padding", R.PADDINGS)
@pytest.mark.parametrize("shape", G.DENSE_SHAPES, ids=["two-wg", "h1"])
def test_dense_flow_gradient(device, shape, padding, indexing, dtype):
    """Every pixel further than DELTA from a kink against float64 autograd through grid_sample.  float32: within
    pos_tol_dense x the taps' mixed difference x sum_c |g_c| plus (4 C + 3) eps32 x sum_c |g_c| x the taps'
    magnitudes (_warp_grad_ref.dense_flow_grad_tol).  float64: within 1e-12 x max(1, sum_c |g_c| x the taps'
    magnitudes) -- the image's type from the grid on, where the torch route this replaces narrowed to float32.
    The image's gradient of the same backward call is the image-adjoint operator's, to the rounding of its
    unordered atomics here and to the bit in test_dense_image_gradient_is_unchanged."""
    N, C, H, W = shape
    image, flow, g = G.dense_input(shape, dtype)
    flow = G.dense_flow(flow, indexing)
    exp, _ = _dense_ref(shape, dtype, indexing, padding)
    pos = G.dense_positions(flow, indexing, H, W, dtype)
    keep = ~G.near_kink(pos, H, W, padding)
    assert keep.mean() >= 1 - G.MAX_EXCLUDED
    img, fl = _t(image, device).requires_grad_(True), _t(flow, device).requires_grad_(True)
    out = F.dense_image_warp(img, fl, indexing, "bilinear", padding)
    g_img, g_fl = torch.autograd.grad(out, [img, fl], _t(g, device))
    assert g_fl.dtype == torch.float and g_fl.shape == (N, H, W, 2)
    if dtype == np.float64:
        _, total = G.tap_stats(image, pos, H, W, padding)
        tol = 1e-12 * np.maximum(1.0, np.abs(g.astype(np.float64)).sum(1) * total.max(1))[..., None]
        # the result leaves the kernel as float32, like the flow: compare what float32 holds of the reference
        exp_cmp = exp.astype(np.float32).astype(np.float64)
    else:
        tol = G.dense_flow_grad_tol(image, pos, g, H, W, padding)
        exp_cmp = exp
    err = np.abs(g_fl.cpu().numpy().astype(np.float64) - exp_cmp)
    worst = (err / np.maximum(tol, 1e-300))[keep].max()  # (all four taps outside: 0 within 0)
    print(shape, padding, indexing, np.dtype(dtype).name, "worst error / tolerance %.3g, largest error %.3g" % (worst, err[keep].max()))
    assert worst <= 1.0, (padding, indexing, worst)
    direct = torch.ops.pydrobert_amd.dense_image_warp_backward(_t(g, device), fl.detach(), indexing, "bilinear", padding)
    # (the adjoint's atomics are not ordered: the same operator, the same arguments, sums in any order)
    assert g_img.dtype == direct.dtype and torch.allclose(g_img, direct, rtol=0, atol=1e-5 if dtype == np.float32 else 1e-12)


def test_dense_image_gradient_is_unchanged(device):
    """The image gradient of a backward call that also asks for the flow's is ``torch.equal`` to
    ``dense_image_warp_backward`` called directly.  The adjoint adds with unordered float atomics, so the
    bits are only defined where no pixel's sum has more than two terms (a + b = b + a): one row of pixels
    (border padding: a single row of taps), every sample 0.4 px right of its pixel -- a pixel receives from
    its own sample and from its left neighbour's.  (test_dense_flow_gradient compares the full-size case
    to the atomics' rounding.)"""
    N, C, H, W = 2, 2, 1, 7
    flow = np.zeros((N, H, W, 2), np.float32)
    flow[..., 1] = -0.4  # ("hw": component 1 is w; the source is w - flow)
    image, g = R.image((N, C, H, W), 31), R.image((N, C, H, W), 32)
    img, fl = _t(image, device).requires_grad_(True), _t(flow, device).requires_grad_(True)
    out = F.dense_image_warp(img, fl, "hw", "bilinear", "border")
    g_img, g_fl = torch.autograd.grad(out, [img, fl], _t(g, device))
    direct = torch.ops.pydrobert_amd.dense_image_warp_backward(_t(g, device), fl.detach(), "hw", "bilinear", "border")
    assert torch.equal(g_img, direct) and g_fl.shape == fl.shape and g_fl.abs().sum() > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_dense_nearest_has_a_zero_flow_gradient(device, dtype):
    shape = G.DENSE_SHAPES[0]
    image, flow, g = G.dense_input(shape, dtype)
    img, fl = _t(image, device).requires_grad_(True), _t(flow, device).requires_grad_(True)
    out = F.dense_image_warp(img, fl, "hw", "nearest", "border")
    g_img, g_fl = torch.autograd.grad(out, [img, fl], _t(g, device))
    assert g_fl.shape == fl.shape and g_fl.dtype == fl.dtype and not g_fl.any()
    assert g_img.abs().sum() > 0


def test_double_backward_fails_loudly(device):
    image, flow, g = G.dense_input(G.DENSE_SHAPES[1])
    img, fl = _t(image, device), _t(flow, device).requires_grad_(True)
    out = F.dense_image_warp(img, fl, "hw", "bilinear", "border")
    (g_fl,) = torch.autograd.grad(out, fl, _t(g, device), create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        g_fl.sum().backward()


# ---------------------------------------------------------------------------------------------------
# sparse
# ---------------------------------------------------------------------------------------------------
def _sparse_point_grads(case, device):
    s, d = case.points()
    s2, d2 = _t(s, device).requires_grad_(True), _t(d, device).requires_grad_(True)
    res = F.sparse_image_warp(_t(case.image, device), s2, d2, **case.kwargs())
    outs, grads = [res[0] if case.include_flow else res], [_t(case.grad_warped, device)]
    if case.grad_flow is not None:
        outs.append(res[1])
        grads.append(_t(case.grad_flow, device))
    return torch.autograd.grad(outs, [s2, d2], grads)


def _check_sparse(case, device):
    """max |difference| / max |reference| < 5e-3 for both point sets: the project's measure for these
    gradients (tests/test_img_gpu.py: test_warps_gradients_wrt_flow_and_points)."""
    exp = case.expected()
    act = _sparse_point_grads(case, device)
    for name, a, e in zip(("source", "dest"), act, exp):
        assert a.shape == e.shape and a.dtype == torch.float
        err = np.abs(a.cpu().numpy().astype(np.float64) - e).max() / np.abs(e).max()
        print(case.name, name, "relative error %.3g" % err)
        assert err < 5e-3, (case.name, name, float(err))


@pytest.mark.parametrize("case", G.SPARSE_CASES, ids=repr)
def test_sparse_point_gradients(device, case):
    _check_sparse(case, device)


def test_sparse_point_gradients_past_the_row_boundary(device):
    """Enough scattered centres that the spline's rows no longer fit one workgroup of the evaluation's
    adjoint (its plan says where that is): the row-tiled form, and the form just below it."""
    from pydrobert_amd import _cabi

    N, C, H, W = G.MANY_SHAPE
    last = G.form_boundary(_cabi.lib(), 2, 2, H * W)  # the largest T of form 0
    for Mp in (last, last + 1):
        case = G.many_centres_case(Mp - 4)
        assert case.Mp == Mp
        _check_sparse(case, device)


def test_sparse_float64_image_and_nearest(device):
    """A float64 image: the position gradient in float64 (the points' gradients stay float32, like the
    points); nearest mode: zero gradients for the points unless the flow carries one."""
    case = G.SPARSE_CASES[2]
    s, d = case.points()
    exp = case.expected()
    s2, d2 = _t(s, device).requires_grad_(True), _t(d, device).requires_grad_(True)
    res = F.sparse_image_warp(_t(case.image.astype(np.float64), device), s2, d2, **case.kwargs())
    warped = res[0] if case.include_flow else res
    assert warped.dtype == torch.double
    act = torch.autograd.grad(warped, [s2, d2], _t(case.grad_warped.astype(np.float64), device))
    for a, e in zip(act, exp):
        assert np.abs(a.cpu().numpy() - e).max() / np.abs(e).max() < 5e-3
    kw = dict(case.kwargs(), dense_interpolation_mode="nearest")
    res = F.sparse_image_warp(_t(case.image, device), s2, d2, **kw)
    warped = res[0] if case.include_flow else res
    g_s, g_d = torch.autograd.grad(warped, [s2, d2], _t(case.grad_warped, device))
    assert not g_s.any() and not g_d.any()


# ---------------------------------------------------------------------------------------------------
# the spline evaluation's adjoint alone
# ---------------------------------------------------------------------------------------------------
def _adjoint(G_, c, sol, x, order, device, need_gx=True):
    return torch.ops.pydrobert_amd.spline_eval_adjoint(_t(G_, device), _t(c, device), _t(sol, device),
                                                       None if x is None else _t(x, device), 0, 0, order, need_gx)  # fmt: skip


def _check_adjoint(act, exp, what):
    for name, a, e in zip(("rhs", "g_c", "g_x"), act, exp):
        a = a.cpu().numpy()
        assert a.shape == e.shape and a.dtype == np.float64, (what, name)
        err = np.abs(a - e).max() / np.abs(e).max()
        assert err < 1e-3, (what, name, float(err))  # the bound of test_polyharmonic_spline_gradients


@pytest.mark.parametrize("O", [1, 3])
@pytest.mark.parametrize("I", [1, 2, 3])
def test_spline_eval_adjoint(device, I, O):
    """Against the float64 torch sums at 1e-3 relative, for Q below, at and past a wave and over several
    workgroups with a ragged last one, with a query on a centre (r = 0) and one within eps of a centre, every
    order; two runs give the same bits."""
    T, N = 7, 2
    for Q in G.ADJOINT_QS:
        for order in (1, 2, 3, 4):
            G_, c, sol, x = G.adjoint_case(T, I, O, Q, N, 50 + Q + order)
            act = _adjoint(G_, c, sol, x, order, device)
            _check_adjoint(act, G.eval_adjoint(G_, c, sol, x, order), (I, O, Q, order))
            again = _adjoint(G_, c, sol, x, order, device)
            assert all(torch.equal(a, b) for a, b in zip(act, again)), (I, O, Q, order)


def test_spline_eval_adjoint_forms_and_lattice(device):
    """The row-tiled form on both sides of its boundary, the queries' gradient on both sides of its LDS cap
    (boundaries from the plan), and the pixel lattice in place of explicit queries: the same bits."""
    from pydrobert_amd import _cabi

    lib = _cabi.lib()
    last = G.form_boundary(lib, 2, 2, 300)
    for T in (last, last + 1, 2 * last + 7):
        G_, c, sol, x = G.adjoint_case(T, 2, 2, 300, 2, 70 + T)
        _check_adjoint(_adjoint(G_, c, sol, x, 2, device), G.eval_adjoint(G_, c, sol, x, 2), ("rows", T))
    cap = G.lds_boundary(lib, 3, 3)
    for T in (cap, cap + 1):
        G_, c, sol, x = G.adjoint_case(T, 3, 3, 65, 1, 80 + T)
        _check_adjoint(_adjoint(G_, c, sol, x, 3, device), G.eval_adjoint(G_, c, sol, x, 3), ("lds", T))
    N, H, W = 2, 33, 29
    G_, c, sol, _ = G.adjoint_case(8, 2, 2, H * W, N, 90, coincide=False)
    x = G.lattice(N, H, W)
    explicit = _adjoint(G_, c, sol, x, 2, device, need_gx=False)
    implied = torch.ops.pydrobert_amd.spline_eval_adjoint(_t(G_, device), _t(c, device), _t(sol, device), None, H, W,
                                                          2, False)  # fmt: skip
    assert torch.equal(explicit[0], implied[0]) and torch.equal(explicit[1], implied[1])
    assert implied[2].numel() == 0


def test_spline_gradients_beyond_four_dimensions(device):
    """I = 5: the kernel answers PDT_E_UNSUPPORTED, the spline's backward takes the torch sums and still
    matches float64 autograd through the reference's graph."""
    from pydrobert_amd import _cabi

    N, T, I, O, Q = 2, 9, 5, 2, 11
    assert _cabi.lib().pdt_spline_eval_adjoint_plan(N, T, I, O, Q, None) == _cabi.PDT_E_UNSUPPORTED
    rng = np.random.default_rng(45)
    c = (rng.uniform(size=(N, T, I)) * 4).astype(np.float32)
    f = rng.normal(size=(N, T, O)).astype(np.float32)
    x = (rng.uniform(size=(N, Q, I)) * 4).astype(np.float32)
    Gm = rng.normal(size=(N, Q, O)).astype(np.float32)
    ref = [torch.from_numpy(a).double().requires_grad_(True) for a in (c, f, x)]
    (G.torch_spline(*ref, 2) * torch.from_numpy(Gm).double()).sum().backward()
    dev = [_t(a, device).requires_grad_(True) for a in (c, f, x)]
    (F.polyharmonic_spline(*dev, 2) * _t(Gm, device)).sum().backward()
    for name, a, b in zip("cfx", dev, ref):
        err = (a.grad.cpu().double() - b.grad).abs().max() / b.grad.abs().max()
        assert err < 1e-3, (name, float(err))


# ---------------------------------------------------------------------------------------------------
# memory: the point of the change
# ---------------------------------------------------------------------------------------------------
def test_points_backward_allocates_less_than_one_dxc(device):
    """N = 4 images of 256 x 80 with one pinned point per edge (T = 3 + 4 = 7): allocated memory grows across
    the backward with respect to the points by less than N H W T I 8 bytes = 9.2 MB, the size of ONE of the
    (N, Q, T, I) float64 tensors the torch sums form."""
    N, C, H, W = G.MEMORY_SHAPE
    src, dst = R.control_points(N, 3, H, W, 77, R.BANDS_SCALE)
    image = _t(R.image(G.MEMORY_SHAPE, 78), device)
    w = _t(R.image(G.MEMORY_SHAPE, 79), device)
    s2, d2 = _t(src, device).requires_grad_(True), _t(dst, device).requires_grad_(True)

    def run():
        warped = F.sparse_image_warp(image, s2, d2, pinned_boundary_points=1, include_flow=False)
        loss = (warped * w).sum()
        torch.cuda.synchronize(device)
        torch.cuda.reset_peak_memory_stats(device)
        before = torch.cuda.memory_allocated(device)
        grads = torch.autograd.grad(loss, [s2, d2])
        torch.cuda.synchronize(device)
        return torch.cuda.max_memory_allocated(device) - before, grads

    run()  # (the first call loads code objects and fills caches of constants)
    growth, grads = run()
    one_dxc = N * H * W * 7 * 2 * 8
    print("growth across the backward: %d bytes (one dxc: %d)" % (growth, one_dxc))
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)
    assert growth < one_dxc, (growth, one_dxc)
