"""CPU: the gradients of the image warps with respect to flow / control points (csrc/image_warp.hip
WARP_POSITION, csrc/spline.hip pdt_spline_eval_adjoint) as far as they go without a GPU -- the operators and
entry points exist, every argument guard answers before any launch, the plan names every form for the
shapes tests/test_warp_grads_gpu.py uses -- and the yardstick of that file (tests/_warp_grad_ref.py): the
conditions its fixed inputs must meet, and the reference against a finite difference."""
import ctypes

import numpy as np
import pytest
import torch

import _img_ref as R
import _warp_grad_ref as G

ENTRY_POINTS = (
    "pdt_dense_image_warp_flow_backward",
    "pdt_dense_image_warp_flow_backward_f64",
    "pdt_sparse_image_warp_position_backward",
    "pdt_sparse_image_warp_position_backward_f64",
    "pdt_spline_eval_adjoint",
    "pdt_spline_eval_adjoint_plan",
)
OPERATORS = ("dense_image_warp_flow_backward", "sparse_image_warp_points_backward", "spline_eval_adjoint")


@pytest.fixture(scope="module")
def lib():
    import os

    import __graft_entry__ as g
    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def _plan(lib, N, T, I, O, Q):
    p = (ctypes.c_int64 * 6)()
    rc = lib.pdt_spline_eval_adjoint_plan(N, T, I, O, Q, p)
    return rc, list(p)


def test_operators_and_entry_points_exist(lib):
    from pydrobert_amd import _cabi, _img  # noqa: F401

    for name in ENTRY_POINTS:
        assert name in _cabi.SIGNATURES and hasattr(lib, name), name
    for name in OPERATORS:
        assert hasattr(torch.ops.pydrobert_amd, name), name
    # the torch bodies the kernels replaced stay, as named private functions
    for name in ("_dense_flow_grad_torch", "_sparse_points_grad_torch", "_spline_eval_adjoint_torch"):
        assert callable(getattr(_img, name)), name


def test_operators_have_fake_kernels():
    """Shapes and dtypes without a device (what torch.compile / make_fx trace)."""
    import pydrobert_amd  # noqa: F401

    ops = torch.ops.pydrobert_amd
    with torch._subclasses.FakeTensorMode():
        img, flow = torch.empty(2, 3, 5, 7), torch.empty(2, 5, 7, 2)
        g = ops.dense_image_warp_flow_backward(img, img, flow, "hw", "bilinear", "border")
        assert g.shape == flow.shape and g.dtype == flow.dtype
        s = torch.empty(2, 4, 2)
        gs, gd = ops.sparse_image_warp_points_backward(img, None, img, s, s, "hw", 2, 0.0, 1, "bilinear", "border",
                                                       False)  # fmt: skip
        assert gs.shape == s.shape and gd.shape == s.shape
        rhs, gc, gx = ops.spline_eval_adjoint(torch.empty(2, 35, 3), s, torch.empty(2, 7, 3, dtype=torch.double), None,
                                              5, 7, 2, False)  # fmt: skip
        assert rhs.shape == (2, 7, 3) and gc.shape == (2, 4, 2) and gx.numel() == 0 and rhs.dtype == torch.double


def test_argument_guards_answer_before_any_launch(lib):
    """The forward entry points' limits and checks, PDT_E_UNSUPPORTED beyond I, O = 4: none of these calls
    reaches a launch, so they are safe without a GPU (null pointers throughout)."""
    from pydrobert_amd import _cabi

    OK, ARG, LONG, UNSUP = _cabi.PDT_OK, _cabi.PDT_E_ARG, _cabi.PDT_E_TOO_LONG, _cabi.PDT_E_UNSUPPORTED
    one = ctypes.c_void_p(64)  # (a non-null pointer that is never dereferenced)
    for sfx in ("", "_f64"):
        dense = getattr(lib, "pdt_dense_image_warp_flow_backward" + sfx)
        assert dense(0, 0, 0, 0, 1, 4, 4, 0, 0, 0, 0, 0) == OK  # N == 0
        assert dense(0, 0, 0, 1, 1, 4, 0, 0, 0, 0, 0, 0) == OK  # W == 0
        assert dense(0, 0, 0, 1, 1, 4, 4, 0, 5, 0, 0, 0) == ARG  # bad mode
        assert dense(0, 0, 0, 1, 1, 4, 4, 0, 0, 3, 0, 0) == ARG  # bad padding
        assert dense(0, 0, 0, -1, 1, 4, 4, 0, 0, 0, 0, 0) == ARG  # negative size
        assert dense(0, 0, 0, 1, 1, 4, 4, 0, 0, 0, 0, 0) == ARG  # null grad_flow
        assert dense(0, 0, 0, 1, 1, 4, 4, 0, 0, 0, one, 0) == ARG  # null inputs
        assert dense(one, one, one, 1, 1, 1 << 16, 1 << 15, 0, 0, 0, one, 0) == LONG  # 2^31 pixels
        assert dense(one, one, one, 65536, 1, 4, 4, 0, 0, 0, one, 0) == LONG
        sparse = getattr(lib, "pdt_sparse_image_warp_position_backward" + sfx)
        assert sparse(0, 0, 0, 0, 0, 1, 4, 4, 3, 2, 0, 0, 0, 0, 0, 0, 0, 0) == OK  # N == 0
        assert sparse(0, 0, 0, 0, 1, 1, 4, 4, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0) == ARG  # M < 1
        assert sparse(0, 0, 0, 0, 1, 1, 4, 4, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0) == ARG  # order < 1
        assert sparse(0, 0, 0, 0, 1, 1, 4, 4, 3, 2, 0, 2, 0, 0, 0, 0, 0, 0) == ARG  # bad mode
        assert sparse(0, 0, 0, 0, 1, 1, 4, 4, 3, 2, 0, 0, 0, 0, 0, 0, 0, 0) == ARG  # null pointers
        assert sparse(one, one, one, one, 1, 1, 4, 4, 3, 2, 0, 0, 0, 0, 0, one, 0, 0) == ARG  # null workspace
        assert sparse(one, one, one, one, 1, 1, 4, 4, 3, 2, 1, 0, 0, one, 0, one, one, 0) == ARG  # grad_flow, no flow
        assert sparse(one, one, one, one, 1, 1, 1 << 16, 1 << 15, 3, 2, 0, 0, 0, 0, 0, one, one, 0) == LONG
        assert sparse(one, one, one, one, 65536, 1, 4, 4, 3, 2, 0, 0, 0, 0, 0, one, one, 0) == LONG
    adj = lib.pdt_spline_eval_adjoint
    assert adj(0, 0, 0, 0, 0, 3, 2, 2, 5, 0, 0, 2, 0, 0, 0, 0, 0) == ARG  # x null, H * W != Q
    assert adj(0, 0, 0, one, 0, 3, 2, 2, 5, 0, 0, 2, 0, 0, 0, 0, 0) == OK  # N == 0
    assert adj(0, 0, 0, one, 1, 0, 2, 2, 5, 0, 0, 2, 0, 0, 0, 0, 0) == ARG  # T < 1
    assert adj(0, 0, 0, one, 1, 3, 2, 2, 5, 0, 0, 0, 0, 0, 0, 0, 0) == ARG  # order < 1
    assert adj(0, 0, 0, one, 1, 3, 2, 2, 5, 0, 0, 2, 0, 0, 0, 0, 0) == ARG  # null pointers
    assert adj(one, one, one, 0, 1, 3, 3, 2, 6, 2, 3, 2, one, one, 0, one, 0) == ARG  # the lattice needs I == 2
    assert adj(one, one, one, 0, 1, 3, 2, 2, 6, 2, 3, 2, one, one, one, one, 0) == ARG  # the lattice has no gradient
    assert adj(one, one, one, one, 1, 3, 5, 2, 5, 0, 0, 2, one, one, 0, one, 0) == UNSUP  # I = 5
    assert adj(one, one, one, one, 1, 3, 2, 5, 5, 0, 0, 2, one, one, 0, one, 0) == UNSUP  # O = 5
    assert adj(one, one, one, one, 65536, 3, 2, 2, 5, 0, 0, 2, one, one, 0, one, 0) == LONG
    assert adj(one, one, one, one, 1, 3, 2, 2, 1 << 31, 0, 0, 2, one, one, 0, one, 0) == LONG
    assert _plan(lib, 1, 3, 5, 2, 5)[0] == UNSUP and _plan(lib, 1, 0, 2, 2, 5)[0] == ARG
    assert _plan(lib, 65536, 3, 2, 2, 5)[0] == LONG
    assert lib.pdt_spline_eval_adjoint_plan(1, 3, 2, 2, 5, None) == 0  # (the plan array is optional)


def test_plan_names_every_form(lib):
    """Form 0 (all T + I + 1 rows in a workgroup of 256 lanes, 256 // rows slices of q) up to 256 rows, form 1
    (row tiles, one slice) beyond; the workgroups and the workspace follow; the queries' gradient stages in
    LDS up to the spline kernels' cap.  For the shapes of tests/test_warp_grads_gpu.py."""
    N, C, H, W = G.SPARSE_SHAPE
    for Mp in (4, 8, 12):  # the sparse cases: 36, 23 and 17 slices
        form, p = _plan(lib, N, Mp, 2, 2, H * W)
        assert form == 0 and p[0] == 0 and p[4] == 256 // (Mp + 3) and p[3] == 1, (Mp, p)
        assert p[1] >= 1 and p[1] * p[5] >= H * W > (p[1] - 1) * p[5] and p[5] % p[4] == 0
        assert p[2] >= N * p[1] * ((Mp + 3) * 2 + Mp * 2) * 8
    # the C4 shape the issue is about: 25 slices of 7 + 3 rows, 50 workgroups of 1600 queries per image
    form, p = _plan(lib, 2048, 7, 2, 2, 80000)
    assert form == 0 and p[4] == 25 and p[5] == 1600 and p[1] == 50, p
    assert p[2] < 2048 * 80000 * 7 * 2 * 8 // 500  # (a five-hundredth of one (N, Q, T, I) float64 tensor)
    # the row boundary, whatever it is: the last T of form 0 and the first of form 1
    T = 1
    while _plan(lib, N, T + 1, 2, 2, H * W)[0] == 0:
        T += 1
        assert T < 4096
    assert T == G.form_boundary(lib, 2, 2, H * W) == 253  # 256 rows = T + I + 1
    form, p = _plan(lib, N, T + 1, 2, 2, H * W)
    assert form == 1 and p[4] == 1 and p[1] == 2 * -(-H * W // p[5]), p  # two row tiles per chunk of q
    # a workgroup never asks for more partials than kAdjMaxChunks x tiles
    form, p = _plan(lib, 1, 7, 2, 2, 1 << 30)
    assert form == 0 and p[1] == 128, p
    # the spline-alone cases
    for I in (1, 2, 3):
        for O in (1, 3):
            for Q in G.ADJOINT_QS:
                form, p = _plan(lib, 2, 7, I, O, Q)
                assert form == 0 and p[3] == 1 and p[1] * p[5] >= Q, (I, O, Q, p)
            assert _plan(lib, 2, 7, I, O, G.ADJOINT_QS[-1])[1][1] > 2  # several workgroups, a ragged last one
            assert G.ADJOINT_QS[-1] % _plan(lib, 2, 7, I, O, G.ADJOINT_QS[-1])[1][5] != 0
    # the LDS cap of the queries' gradient: staged up to it, global memory beyond
    T = G.lds_boundary(lib, 3, 3)
    assert _plan(lib, 1, T, 3, 3, 65)[1][3] == 1 and _plan(lib, 1, T + 1, 3, 3, 65)[1][3] == 0
    assert (T + 4) * 3 * 8 + T * 3 * 4 <= 160 * 1024 - 64 < (T + 5) * 3 * 8 + (T + 1) * 3 * 4


@pytest.mark.parametrize("shape", G.DENSE_SHAPES)
def test_dense_inputs_meet_their_conditions(shape):
    """At most 1 % of the pixels of each fixed dense input lie within DELTA of a kink (a condition on the
    seeds, asserted on the reference alone: about 4 DELTA = 0.4 % is expected), for every padding and both
    image types; on the large shape about a third of the samples leave the image."""
    N, C, H, W = shape
    image, flow, g = G.dense_input(shape)
    for dtype in (np.float32, np.float64):
        pos = G.dense_positions(flow, "hw", H, W, dtype)
        for padding in R.PADDINGS:
            share = float(G.near_kink(pos, H, W, padding).mean())
            assert share <= G.MAX_EXCLUDED, (shape, padding, share)
    if H * W > 100:
        assert 0.25 <= G.outside_share(pos, H, W) <= 0.45, G.outside_share(pos, H, W)
        assert G.near_kink(pos, H, W, "zeros").any()  # (the exclusion is exercised)
    # both indexings are the same geometry
    assert np.array_equal(G.dense_positions(G.dense_flow(flow, "wh"), "wh", H, W), G.dense_positions(flow, "hw", H, W))
    # the bound is far below the gradients it judges
    tol = G.dense_flow_grad_tol(image, pos, g, H, W, "border")
    ref, _ = G.dense_flow_grad(image, flow, g, "hw", "bilinear", "border")
    assert np.median(tol) < 1e-3 * np.abs(ref).max()


@pytest.mark.parametrize("padding", R.PADDINGS)
def test_reference_agrees_with_a_finite_difference(padding):
    """The yardstick itself: float64 autograd through grid_sample against a central difference of the
    float64 forward, on a small dense case (pixels next to a kink left out) and a small sparse one."""
    shape = (1, 2, 6, 5)
    N, C, H, W = shape
    rng = np.random.default_rng(3)
    image, g = rng.normal(size=shape), rng.normal(size=shape)
    flow = (rng.normal(size=(N, H, W, 2)) * 2.5).astype(np.float32)
    ref, _ = G.dense_flow_grad(image, flow, g, "hw", "bilinear", padding)
    keep = ~G.near_kink(G.dense_positions(flow, "hw", H, W), H, W, padding, 1e-2)
    assert keep.mean() > 0.8
    h = 1e-4  # (no kink within 1e-2: the forward is bilinear between flow +- h)
    for k in range(2):
        d = np.zeros(flow.shape)
        d[..., k] = h
        # (every pixel's flow moves at once: output pixel p depends on flow[p] alone)
        up = forward_f64(image, flow.astype(np.float64) + d, g, padding)
        dn = forward_f64(image, flow.astype(np.float64) - d, g, padding)
        fd = (up - dn) / (2 * h)
        err = np.abs(fd - ref[..., k])[keep]
        assert err.max() < 1e-6 * max(1.0, np.abs(ref).max()), (padding, k, err.max())


def forward_f64(image, flow64, g, padding):
    """(N, H, W): sum over the channels of grad_out x the float64 dense warp at a float64 flow ("hw")."""
    N, C, H, W = image.shape
    h, w = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    grid = (2 * np.stack([w, h], 2)[None] - 2 * flow64[..., ::-1] + 1.0) / np.array([W, H], np.float64) - 1.0
    return (R.oracle.grid_sample(image, grid, "bilinear", padding) * g).sum(1)


def test_sparse_reference_agrees_with_a_finite_difference():
    shape = (1, 1, 7, 6)
    rng = np.random.default_rng(4)
    image, g = rng.normal(size=shape), rng.normal(size=shape)
    src, dst = R.control_points(1, 4, 7, 6, 11, 0.3)
    for include_flow, pinned, indexing in ((True, 1, "hw"), (False, 0, "wh")):
        gf = rng.normal(size=(1, 7, 6, 2)) if include_flow else None
        g_s, g_d = G.sparse_points_grad(image, src, dst, g, gf, indexing, 2, pinned, include_flow, 0.0, "bilinear", "border")
        assert np.isfinite(g_s).all() and np.isfinite(g_d).all()

        def loss(s, d):
            with torch.no_grad():
                w, fl = G.sparse_warp_graph(image, torch.from_numpy(s), torch.from_numpy(d), indexing, 2, pinned,
                                            include_flow, 0.0, "bilinear", "border")  # fmt: skip
                out = (w * torch.from_numpy(g)).sum()
                return float(out + (fl * torch.from_numpy(gf)).sum()) if include_flow else float(out)

        s64, d64 = src.astype(np.float64), dst.astype(np.float64)
        h = 1e-6
        for which, ref in ((0, g_s), (1, g_d)):
            for idx in ((0, 0, 0), (0, 2, 1), (0, 3, 0)):
                e = np.zeros(src.shape)
                e[idx] = h
                args = lambda sign: (s64 + sign * e, d64) if which == 0 else (s64, d64 + sign * e)  # noqa: E731
                fd = (loss(*args(1)) - loss(*args(-1))) / (2 * h)
                assert abs(fd - ref[idx]) < 1e-4 * max(1.0, np.abs(ref).max()), (include_flow, which, idx, fd, ref[idx])


def test_sparse_cases_cover_the_settings():
    cases = G.SPARSE_CASES
    for order in (1, 2, 3, 4):
        mine = [c for c in cases if c.order == order]
        assert {c.include_flow for c in mine} == {True, False} and {c.pinned for c in mine} == {0, 1, 2}
        assert {c.indexing for c in mine} == {"hw", "wh"} and {c.reg for c in mine} >= {0.0, 0.05}
    assert {c.padding for c in cases} == set(R.PADDINGS)
    assert sum(c.flow_grad for c in cases) == 2 and len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.pts == 4 and c.shape == G.SPARSE_SHAPE


def test_many_centres_cases_are_well_posed_in_float32(lib):
    """The cases on both sides of the row boundary (from the plan): the reference's own float32 evaluation
    of their splines stays within MANY_POS_ERR px of the float64 one, and the gradients are finite."""
    N, C, H, W = G.MANY_SHAPE
    last = G.form_boundary(lib, 2, 2, H * W)
    for Mp in (last, last + 1):
        case = G.many_centres_case(Mp - 4)
        assert case.Mp == Mp and _plan(lib, N, Mp, 2, 2, H * W)[0] == int(Mp > last)
        err = R.pos_tol_sparse(case.src, case.dst, "hw", H, W, case.order, case.pinned, case.include_flow, case.reg)
        assert err <= G.MANY_POS_ERR, (Mp, err)
        assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in case.expected())


def test_eval_adjoint_reference_is_the_spline_backward():
    """The float64 torch sums agree with autograd through the reference's spline graph (rhs and g_x directly;
    g_c through the full chain is the GPU file's business)."""
    T, I, O, Q, N = 5, 2, 3, 9, 2
    Gm, c, sol, x = G.adjoint_case(T, I, O, Q, N, 12, coincide=False)
    rhs, g_c, g_x = G.eval_adjoint(Gm, c, sol, x, 2)
    ct, xt = torch.from_numpy(c).double().requires_grad_(True), torch.from_numpy(x).double().requires_grad_(True)
    st = torch.from_numpy(sol).requires_grad_(True)
    cd = torch.cdist(xt, ct, compute_mode="donot_use_mm_for_euclid_dist")
    out = G._torch_phi(cd, 2) @ st[:, :T] + torch.cat([xt, torch.ones_like(xt[..., :1])], 2) @ st[:, T:]
    e_c, e_x, e_s = torch.autograd.grad(out, [ct, xt, st], torch.from_numpy(Gm).double())
    assert np.allclose(rhs, e_s.numpy(), rtol=1e-10, atol=1e-10)
    assert np.allclose(g_c, e_c.numpy(), rtol=1e-10, atol=1e-10)
    assert np.allclose(g_x, e_x.numpy(), rtol=1e-10, atol=1e-10)
