"""Pins tests/_img_ref.py, the reference side of tests/test_img_gpu.py, without a GPU: the oracle's
``grid_sample`` against torch's own in float64, the position helpers against the oracle's warps, and the
conditions every shape of the GPU tests must meet -- samples outside the image on all four sides, at most
1 % of nearest samples on a rounding boundary, and a tolerance that a tap one pixel off cannot meet."""
import numpy as np
import pytest
import torch

import oracle
import _img_ref as R


def _torch_sample(img, grid, mode, padding):
    return torch.nn.functional.grid_sample(
        torch.from_numpy(img), torch.from_numpy(grid), mode=mode, padding_mode=padding, align_corners=False
    ).numpy()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("padding", R.PADDINGS)
def test_oracle_grid_sample_is_torchs(mode, padding):
    """float64 image and grid, so torch samples in float64 too.  Random positions up to four image sizes
    outside (the reflection folds more than once), and every integer and half-pixel position from two sizes
    before the image to two sizes after it, in both axes.  Nearest mode: positions within 1e-9 of a rounding
    boundary are left out (the grid's round trip through its normalised form decides them)."""
    rng = np.random.default_rng(1)
    N, C, H, W = 2, 3, 7, 5
    img = rng.normal(size=(N, C, H, W))
    px = rng.uniform(-4 * W, 5 * W, (N, 40, 30))
    py = rng.uniform(-4 * H, 5 * H, (N, 40, 30))
    hx = np.arange(-4 * W, 6 * W + 1) / 2.0  # integers and halves
    hy = np.arange(-4 * H, 6 * H + 1) / 2.0
    gx, gy = np.meshgrid(hx, hy, indexing="xy")
    for x, y in ((px, py), (np.broadcast_to(gx, (N,) + gx.shape), np.broadcast_to(gy, (N,) + gy.shape))):
        grid = np.stack([(2 * x + 1) / W - 1, (2 * y + 1) / H - 1], -1)
        exp = _torch_sample(img, grid, mode, padding)
        act = oracle.grid_sample(img, grid, mode, padding)
        if mode == "nearest":
            ok = R.off_boundary(R.positions(grid, H, W), H, W, padding, 1e-9)
            assert ok.mean() > 0.2  # (the lattice: a quarter is integer in both axes)
            bad = np.abs(exp - act).max(1) > 1e-12
            assert not (bad & ok).any()
            continue
        assert np.abs(exp - act).max() < 1e-12, (mode, padding)


def test_reflection_folds_more_than_once():
    """The positions above do what their comment says."""
    x = np.array([-12.3, 17.9, 3.2])
    folded = R.pad_positions(np.stack([x, x], -1), 5, 5, "reflection")[..., 0]
    # period 10 around [-0.5, 4.5]: -12.3 -> 1.3 after two folds, 17.9 -> 1.1 after three, 3.2 stays
    assert np.allclose(folded, [1.3, 1.1, 3.2])


@pytest.mark.parametrize("name", sorted(R.SPARSE_CASES))
def test_sparse_positions_reproduce_the_oracle(name):
    """Sampling the image at the helper's grid IS oracle.sparse_image_warp, and its flow is the oracle's."""
    c = R.SPARSE_CASES[name]
    for indexing in R.INDEXINGS:
        s, d = c.points(indexing)
        for padding in R.PADDINGS:
            exp = oracle.sparse_image_warp(c.image, s, d, indexing, c.order, pinned_boundary_points=c.pinned,
                                           dense_interpolation_mode=c.mode, dense_padding_mode=padding,
                                           include_flow=c.include_flow)
            if c.include_flow:
                assert np.array_equal(exp[1], c.grid(indexing)[1])
                exp = exp[0]
            assert exp.dtype == c.dtype and np.array_equal(exp, c.expected(indexing, padding))
    # a subset of rows is the same rows of the whole
    N, C, H, W = c.shape
    rows = [0, H - 1]
    g, f = R.sparse_grid(*c.points("hw"), "hw", H, W, c.order, c.pinned, c.include_flow, image_dtype=c.dtype, rows=rows)
    assert np.array_equal(g, c.grid("hw")[0][:, rows])
    assert f is None or np.array_equal(f, c.grid("hw")[1][:, rows])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dense_positions_reproduce_the_oracle(dtype):
    img, flow = R.dense_case(dtype=dtype)
    N, C, H, W = img.shape
    rows = [0, 3, H - 1]
    for indexing in R.INDEXINGS:
        grid = R.dense_grid(flow, indexing, H, W, dtype)
        assert np.array_equal(R.dense_grid(flow[:, rows], indexing, H, W, dtype, rows=rows), grid[:, rows])
        for mode in R.MODES:
            for padding in R.PADDINGS:
                exp = oracle.dense_image_warp(img, flow, indexing, mode, padding)
                assert np.array_equal(exp, oracle.grid_sample(img, grid, mode, padding))


def test_spline_solution_is_the_oracles():
    """spline_solution + spline_eval in float64 = oracle.polyharmonic_spline up to its float32 cast."""
    c, f, x = R.spline_case(20, 2, 3, 50, 2, 2, 0)
    for order in (1, 2, 3, 4):
        exp = oracle.polyharmonic_spline(c, f, x, order)
        act = R.spline_eval(c, *R.spline_solution(c, f, order), x, order)
        assert np.array_equal(act.astype(np.float32), exp) or np.abs(act - exp).max() <= 2.0**-23 * np.abs(exp).max()


def test_lipschitz_counts_the_padding():
    img = np.array([[[[3.0, 1.0], [-2.0, 0.5]]]])
    assert R.lipschitz(img, "border") == 5.0 and R.lipschitz(img, "reflection") == 5.0  # 3 -> -2
    assert R.lipschitz(img[..., :1, :] * 3, "zeros") == 9.0  # the edge magnitude of 9 against the ring of zeros
    assert R.median_step(img) == 2.25  # steps 2, 2.5, 5, 0.5


# ---------------------------------------------------------------------------------------------------
# the conditions of the GPU tests' shapes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SPARSE_CASES))
def test_sparse_cases_meet_their_conditions(name):
    """Sensitivity under every padding (the tolerance is at most a tenth of the median pixel step); where the
    case is to leave the image, at least 2 % of the samples beyond each of the four sides; nearest mode: at
    most 1 % of the samples within the tolerance of a rounding boundary.  Measured pos_tol_sparse here: 3.5e-6
    to 4.8e-4 px for the cases of up to 12 centres, 3.2e-3 / 3.7e-3 px for 138 / 140 centres."""
    c = R.SPARSE_CASES[name]
    N, C, H, W = c.shape
    m = c.measured()
    assert 1e-7 < m < 5e-3, m
    pos = R.positions(c.grid("hw")[0], H, W)
    assert np.array_equal(pos, R.positions(c.grid("wh")[0], H, W))  # the same geometry in both indexings
    for padding in R.PADDINGS:
        tol = R.value_tol(c.ptol(), c.image, padding)
        assert R.sensitive(tol, c.image), (padding, tol, R.median_step(c.image))
        if c.mode == "nearest":
            assert 1.0 - R.off_boundary(pos, H, W, padding, c.ptol()).mean() <= R.MAX_BOUNDARY_SHARE
    if c.outside:
        assert min(R.outside_shares(pos, H, W)) >= R.MIN_OUTSIDE, R.outside_shares(pos, H, W)
    assert (c.image > 0).any() and (c.image < 0).any()


def test_fold_case_folds_twice():
    c = R.SPARSE_CASES["bands-fold"]
    N, C, H, W = c.shape
    pos = R.positions(c.grid("hw")[0], H, W)
    x, y = pos[..., 0], pos[..., 1]
    # beyond one whole image past either edge: reflect_coord's flips reach 2
    assert np.mean((x < -0.5 - W) | (x > 2 * W - 0.5)) > 0.2 and np.mean((y < -0.5 - H) | (y > 2 * H - 0.5)) > 0.2


def test_band_and_workgroup_arithmetic():
    """What the shapes are chosen for (csrc/image_warp.hip: four rows per band, 256 lanes and 2048 pixels
    per workgroup, the division branch from 2^23 pixels)."""
    N, C, H, W = R.SHAPE_BANDS
    bands = -(-H // 4)
    assert bands == 10 and H - 4 * (bands - 1) == 1 and bands * W == 290 and 290 - 256 == 34
    assert (-(-5 // 4), 5 - 4) == (2, 1) and -(-3 // 4) == 1
    N, C, H, W = R.SHAPE_TWO_WG
    assert H * W == 2250 and H * W - 2048 == 202 and 202 % 256 != 0
    N, C, H, W = R.SHAPE_BIG
    assert H * W >= 2**23 and max(R.BIG_ROWS) == H - 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dense_case_meets_its_conditions(dtype):
    img, flow = R.dense_case(dtype=dtype)
    N, C, H, W = img.shape
    ptol = R.pos_tol_dense(H, W)
    pos = R.positions(R.dense_grid(flow, "hw", H, W, dtype), H, W)
    assert min(R.outside_shares(pos, H, W)) >= R.MIN_OUTSIDE
    for padding in R.PADDINGS:
        assert R.sensitive(R.value_tol(ptol, img, padding), img)
        assert 1.0 - R.off_boundary(pos, H, W, padding, ptol).mean() <= R.MAX_BOUNDARY_SHARE


def test_big_case_meets_its_conditions():
    """The smooth image keeps the value tolerance near 1e-5 at a position tolerance of 2e-3 px, still a
    tenth of its median step."""
    N, C, H, W = R.SHAPE_BIG
    img = R.smooth_image(H, W)
    assert img.shape == R.SHAPE_BIG and (img > 0).any() and (img < 0).any()
    ptol = R.pos_tol_dense(H, W)
    tol = R.value_tol(ptol, img, "border")
    assert tol < 1.5e-5 and R.sensitive(tol, img), (tol, R.median_step(img))


def test_spline_cases_are_well_conditioned():
    """The bounds the regime tests use, from the oracle alone (spline_bound): the conditioning noise of
    the solver cases is at most a few float32 ulps of the output, so the bound is a tight one."""
    for T in (86, 87, 139, 140):
        for order in (1, 2, 3):
            c, f, x = R.spline_case(T, 2, 2, 300, 2, order, T)
            d = c[:, :, None] - c[:, None]
            r = np.sqrt((d * d).sum(-1)) + np.eye(T) * 9
            assert r.min() > 0.1  # no two centres nearly coincide
            exp, bound, noise = R.spline_bound(c, f, x, order)
            assert bound <= 1e-4 * max(1.0, np.abs(exp).max()), (T, order, bound, noise)
    for T in (125, 126, 315, 316):
        c, f, x = R.spline_case(T, 1, 64, 20, 2, 1, T)
        exp, bound, noise = R.spline_bound(c, f, x, 1)
        assert bound <= 1e-4 * max(1.0, np.abs(exp).max()), (T, bound, noise)
