"""CPU: the entry points through which SpecAugment's application kernels read and write float16 / bfloat16
features as they are (include/pdt_amd.h: pdt_spec_augment_apply*_elem, pdt_spec_augment_apply_form,
pdt_spec_augment_backward_workspace_bytes) exist in the header, the ctypes table and the library, judge the element
code and the pointers before any device work, and plan every case of tests/_half_spec.py as its table says; the
table reaches every form; and the constructions the GPU test's bit-equalities rest on -- dyadic grids whose
scatter sums do not depend on their order, blends that lie exactly halfway between two bfloat16 numbers -- hold
in numpy float32."""
import os
import re

import numpy as np
import pytest
import torch

import _half_spec as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdt_amd.h")
SIBLINGS = ("pdt_spec_augment_apply", "pdt_spec_augment_apply_warp", "pdt_spec_augment_apply_backward")
ELEMS = (0, 2, 3)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def test_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for sibling in SIBLINGS:
        name = sibling + "_elem"
        assert name in _cabi.SIGNATURES, name + " is not in the ctypes table"
        assert hasattr(lib, name), "libpdt_amd.so does not export " + name
        own, sib = _cabi.SIGNATURES[name], _cabi.SIGNATURES[sibling]
        extra = 3 if sibling.endswith("backward") else 1  # (int elem [, void *workspace, int64_t workspace_bytes])
        assert own[0] == sib[0] and own[1][:-extra] == sib[1], name
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, name + " is not declared in pdt_amd.h"
        assert re.match(r"\s*const void \*", m.group(1)) and "int elem" in m.group(1), name
        m = re.search(r"\b" + sibling + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert re.match(r"\s*const float \*", m.group(1)) and "elem" not in m.group(1), sibling  # (unchanged)
    for name in ("pdt_spec_augment_apply_form", "pdt_spec_augment_backward_workspace_bytes"):
        assert name in _cabi.SIGNATURES and hasattr(lib, name) and re.search(r"\b" + name + r"\s*\(", src), name
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14


def _calls(lib):
    """name -> f(N, elem, p): each _elem entry point on a (N, 5, 8) problem with one mask band each way and every
    pointer ``p`` (0: null; otherwise a made-up address, never dereferenced: every call here returns before a
    launch)."""
    return {
        "apply": lambda N, e, p: lib.pdt_spec_augment_apply_elem(p, N, 5, 8, 40, 8, 1, p, 0, p, p, 1, p, p, 1, p, 0, e),
        "warp": lambda N, e, p: lib.pdt_spec_augment_apply_warp_elem(
            p, N, 5, 8, 40, 8, 1, p, p, p, 1, p, p, 1, p, p, 1, p, 0, 0, e),
        "backward": lambda N, e, p: lib.pdt_spec_augment_apply_backward_elem(
            p, N, 5, 8, p, p, p, p, 1, p, p, 1, p, 0, e, p, 4 * N * 5 * 8),
    }  # fmt: skip


def test_element_codes_and_pointers_are_judged_without_a_device(lib):
    """Element code 1 (float64) is PDT_E_UNSUPPORTED and any other code but 0, 2, 3 PDT_E_ARG, whatever the rest;
    null pointers with work to do are PDT_E_ARG for every element type; no utterances is PDT_OK; negative sizes
    PDT_E_ARG; a half scatter with a grid and no (or a short) workspace is PDT_E_ARG."""
    from pydrobert_amd import _cabi

    OK, ARG, UNSUP = _cabi.PDT_OK, _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    addr = hs.BASE_ADDR
    for name, call in _calls(lib).items():
        for N in (0, 3):
            for p in (0, addr):
                assert call(N, 1, p) == UNSUP, name
                assert call(N, 7, p) == ARG and call(N, -1, p) == ARG, name
        for e in ELEMS:
            assert call(3, e, 0) == ARG, (name, e)
            assert call(0, e, 0) == OK and call(0, e, addr) == OK, (name, e)
            assert call(-1, e, addr) == ARG, (name, e)
    # the frequency grid sends the adjoint to the scatter form: a half type needs its float32 sums
    for e in (2, 3):
        for ws, nbytes in ((0, 0), (0, 4 * 3 * 5 * 8), (addr, 4 * 3 * 5 * 8 - 1)):
            assert lib.pdt_spec_augment_apply_backward_elem(
                addr, 3, 5, 8, addr, addr, 0, 0, 0, 0, 0, 0, addr, 0, e, ws, nbytes) == ARG, (e, ws, nbytes)
    # the fused warp refuses what the rows kernel does not take, before any launch: odd F, and rows on 2-byte
    # boundaries for a half type (4-byte ones for float32)
    for e in ELEMS:
        assert lib.pdt_spec_augment_apply_warp_elem(
            addr, 3, 5, 7, 35, 7, 1, addr, addr, 0, 1, 0, 0, 0, 0, 0, 0, addr, 0, 0, e) == UNSUP
        assert lib.pdt_spec_augment_apply_warp_elem(
            addr + hs.ESIZE[e], 3, 5, 8, 40, 8, 1, addr, addr, 0, 1, 0, 0, 0, 0, 0, 0, addr, 0, 0, e) == UNSUP


@pytest.mark.parametrize("name", sorted(hs.FWD_CASES))
def test_forward_form_of_every_case(lib, name):
    """pdt_spec_augment_apply_form gives the table's form for the case's layout, for float32 and both half types
    (an element size each), with the case's grids on the explicit-grid route and with none on the fused-warp
    route, which takes the rows kernel exactly where the table says 1."""
    c = hs.FWD_CASES[name]
    for e in ELEMS:
        assert hs.form_query(lib, c, e, c["tw"], c["fw"]) == c["fwd"], (name, e)
        if c["tw"] and not c["fw"]:
            assert hs.form_query(lib, c, e, False, False) == c["fwd"], (name, e)
    assert hs.form_query(lib, c, 1, c["tw"], c["fw"]) == -3 and hs.form_query(lib, c, 5, c["tw"], c["fw"]) == -1


def test_form_follows_the_element_size(lib):
    """Rows and base pointers must be aligned to 4 elements: an offset of 2 elements is 8 bytes for float32 and 4
    for a half type -- general for both; 4 elements is rows for both; 8 bytes past a 16-byte boundary is rows for
    a half type alone.  A frequency grid, F above 256, F % 4 != 0 and strides that are no multiple of 4 are
    general for every element type; the form with eight elements per lane does not exist."""
    q = lib.pdt_spec_augment_apply_form
    A = hs.BASE_ADDR
    for e in ELEMS:
        es = hs.ESIZE[e]
        assert q(2, 10, 8, 80, 8, 1, A, A, 1, 0, 0, e) == 1
        assert q(2, 10, 8, 80, 8, 1, A + 2 * es, A, 1, 0, 0, e) == 0
        assert q(2, 10, 8, 80, 8, 1, A, A + 2 * es, 1, 0, 0, e) == 0
        assert q(2, 10, 8, 80, 8, 1, A + 4 * es, A, 1, 0, 0, e) == 1
        assert q(2, 10, 8, 80, 8, 1, A + 8, A, 1, 0, 0, e) == (1 if es == 2 else 0)
        assert q(2, 10, 8, 80, 8, 1, A, A, 1, 1, 0, e) == 0
        assert q(2, 10, 8, 82, 8, 1, A, A, 1, 0, 0, e) == 0 and q(2, 10, 8, 90, 9, 1, A, A, 1, 0, 0, e) == 0
        assert q(2, 10, 8, 160, 16, 2, A, A, 1, 0, 0, e) == 0
        assert q(2, 10, 256, 2560, 256, 1, A, A, 1, 0, 0, e) == 1 and q(2, 10, 260, 2600, 260, 1, A, A, 1, 0, 0, e) == 0
        for F in (8, 16, 64, 256):
            assert q(2048, 1000, F, 1000 * F, F, 1, A, A, 1, 0, 0, e) == 1  # (never 2)
        # the adjoint: contiguous whatever strides are passed; three words of LDS per frame
        assert q(2, 5353, 8, 1, 1, 7, A, A, 1, 0, 1, e) == 1 and q(2, 5354, 8, 5354 * 8, 8, 1, A, A, 1, 0, 1, e) == 0
        assert q(-1, 10, 8, 80, 8, 1, A, A, 1, 0, 0, e) == -1 and q(1, 1 << 20, 1 << 11, 1 << 31, 1 << 11, 1, A, A, 0, 0, 0, e) == -2


def test_case_table_reaches_every_form(lib):
    """General, rows, rows behind the fused warp, the fused warp's fallback; gather, scatter (by a frequency grid
    and by a refused layout) and one-to-one backward -- each is in the table, and the plan query agrees with the
    table's backward form for every element type."""
    F = hs.FWD_CASES
    assert {c["fwd"] for c in F.values()} == {0, 1}
    assert any(c["fwd"] == 1 and c["tw"] and not c["fw"] for c in F.values())  # rows behind the fused warp
    assert any(c["fwd"] == 0 and c["tw"] and not c["fw"] for c in F.values())  # its fallback: the half general kernel
    assert any(c["fwd"] == 1 and not c["tw"] for c in F.values())  # rows, no grid
    assert any(c["fw"] for c in F.values())
    assert {c["layout"] for c in F.values()} == set(hs.LAYOUTS)
    B = hs.BWD_CASES
    assert {c["bwd"] for c in B.values()} == {"gather", "scatter", "one"}
    assert any(c["bwd"] == "scatter" and c["grid"] == "time" for c in B.values())
    for name, c in B.items():
        for e in ELEMS:
            assert hs.bwd_form_query(lib, c, e) == (1 if c["bwd"] == "gather" else 0), (name, e)


def test_backward_workspace_bytes(lib):
    """0 for float32 whatever the route; 0 for the rows (gather) and one-to-one routes; 4 N T F for a half scatter
    with a grid; -1 for element codes that are not 0, 2, 3 and for negative sizes."""
    q = lib.pdt_spec_augment_backward_workspace_bytes
    for name, c in hs.BWD_CASES.items():
        N, T, F = c["N"], c["T"], c["F"]
        has = {None: 0, "time": 1, "freq": 2, "both": 3}[c["grid"]]
        assert q(N, T, F, has, 0) == 0, name
        for e in (2, 3):
            assert q(N, T, F, has, e) == (4 * N * T * F if c["bwd"] == "scatter" else 0), (name, e)
    assert q(2, 64, 16, 3, 1) == -1 and q(2, 64, 16, 3, 7) == -1 and q(-2, 64, 16, 3, 2) == -1
    assert q(0, 64, 16, 3, 2) == 0


@pytest.mark.parametrize("name", hs.EXACT_BWD)
def test_dyadic_scatter_sums_do_not_depend_on_their_order(name):
    """The exact scatter cases, restated in numpy float32 (img_sample.hpp: unnormalize, clip_coord): every grid
    value gives its p back exactly, so every tap weight is a multiple of 1/8 and a product of two of 1/64;
    grad_out is multiples of 2^-6 within [-2, 2] that both half types hold; so every contribution is a multiple
    of 2^-12, and the sum of the magnitudes that reach one source element stays below 2^11 -- any partial sum in
    any order is a multiple of 2^-12 below 2^11, which float32's 24 bits hold exactly.  Some source element
    receives three contributions or more (there is an order to vary)."""
    c = hs.BWD_CASES[name]
    N, T, F = c["N"], c["T"], c["F"]
    g, tg, fg, t_0, t, f_0, f = hs.bwd_numpy(name)
    assert np.array_equal(g * 64, np.round(g * 64)) and np.abs(g).max() <= 2
    for dt in hs.DTYPES.values():
        assert np.array_equal(torch.from_numpy(g).to(dt).float().numpy(), g)
    ident = lambda n, size: np.broadcast_to(  # noqa: E731  (the kernels' identity grid of an unwarped axis)
        (np.float32(2) * np.arange(size, dtype=np.float32) + np.float32(1)) / np.float32(size) - np.float32(1), (n, size))
    y0, wy0, wy1 = hs.taps32(tg if tg is not None else ident(N, T), T)
    x0, wx0, wx1 = hs.taps32(fg if fg is not None else ident(N, F), F)
    for w in (wy0, wy1, wx0, wx1):
        assert w.dtype == np.float32 and np.array_equal(w * 8, np.round(w * 8)) and w.min() >= 0 and w.max() <= 1
    assert np.array_equal(wy0 + wy1, np.ones_like(wy0)) and np.array_equal(wx0 + wx1, np.ones_like(wx0))
    if tg is None:
        assert np.array_equal(y0, np.broadcast_to(np.arange(T), (N, T))) and not wy1.any()
    if fg is None:
        assert np.array_equal(x0, np.broadcast_to(np.arange(F), (N, F))) and not wx1.any()
    count = np.zeros((N, T, F), np.int64)
    mag = np.zeros((N, T, F), np.float64)
    ar_t, ar_f = np.arange(T)[None, :, None], np.arange(F)[None, :, None]
    keep_t = ~((ar_t >= t_0[:, None, :]) & (ar_t < (t_0 + t)[:, None, :])).any(2)
    keep_f = ~((ar_f >= f_0[:, None, :]) & (ar_f < (f_0 + f)[:, None, :])).any(2)
    keep = keep_t[:, :, None] & keep_f[:, None, :]
    nn = np.broadcast_to(np.arange(N)[:, None, None], (N, T, F))
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            w = wy[:, :, None].astype(np.float64) * wx[:, None, :]
            yy = np.broadcast_to(np.minimum(y0 + dy, T - 1)[:, :, None], (N, T, F))
            xx = np.broadcast_to(np.minimum(x0 + dx, F - 1)[:, None, :], (N, T, F))
            sel = keep & (w != 0)
            np.add.at(count, (nn[sel], yy[sel], xx[sel]), 1)
            np.add.at(mag, (nn[sel], yy[sel], xx[sel]), (np.abs(g) * w)[sel])
    assert count.max() >= 3, count.max()
    assert mag.max() < 2 ** 11, mag.max()


def test_halfway_construction():
    """The planted-value case in numpy float32: the grid puts every output row exactly halfway between two source
    rows (w0 == w1 == 1/2), the bfloat16 ties' means have float32 patterns ending in 0x8000 (exactly between two
    bfloat16 numbers, the lower one odd or even as the table says), the means of the float16 subnormals lie
    halfway between two float16 numbers, and every planted value is held exactly by the dtype it is planted
    for."""
    grid, y0_exp = hs.halfway_grid(2)
    y0, w0, w1 = hs.taps32(grid, hs.PLANT_T)
    assert np.array_equal(y0, np.broadcast_to(y0_exp, y0.shape))
    assert (w0 == np.float32(0.5)).all() and (w1 == np.float32(0.5)).all()
    # the kernels form w0 as (y0 + 1) - (y0 + w1) in the rows kernel: the same half
    assert ((y0.astype(np.float32) + np.float32(1)) - (y0.astype(np.float32) + w1) == np.float32(0.5)).all()
    half = np.float32(0.5)
    for a, b, even in hs.BF16_TIES:
        mean = hs.bf16_to_f32(a) * half + hs.bf16_to_f32(b) * half
        bits = int(np.array([mean], np.float32).view(np.uint32)[0])
        assert bits & 0xFFFF == 0x8000 and bits >> 16 == min(a, b), hex(bits)
        assert even & 1 == 0 and even in (a, b)
        assert int(torch.tensor([float(mean)]).to(torch.bfloat16).view(torch.int16).item()) & 0xFFFF == even
    for lo, hi, exp in ((2.0 ** -24, 2.0 ** -23, 2.0 ** -23), (2.0 ** -23, 3 * 2.0 ** -24, 2.0 ** -23)):
        mean = np.float32(lo) * half + np.float32(hi) * half
        assert float(mean) * 2.0 ** 24 % 1 == 0.5  # (between two float16 subnormals)
        assert float(torch.tensor([float(mean)]).to(torch.float16).item()) == exp
    for dt in hs.DTYPES.values():
        x = hs.planted(dt)[0]
        back = torch.from_numpy(x).to(dt).float().numpy()
        assert np.array_equal(np.isnan(back), np.isnan(x)) and np.array_equal(back[~np.isnan(x)], x[~np.isnan(x)])
        assert (x[:, 8:10, 1:] == torch.finfo(dt).max).all()


def test_ulp_helper_and_memory_allowance():
    """ulp_of is the dtype's spacing (2^-10 / 2^-7 at 1, the smallest subnormal at 0); the no-copy allowance, 1.5
    times the output's bytes, is below the output plus ONE float32 tensor of the features' shape."""
    for dt, at_one, at_zero in ((torch.float16, 2.0 ** -10, 2.0 ** -24), (torch.bfloat16, 2.0 ** -7, 2.0 ** -133)):
        u = hs.ulp_of(torch.tensor([1.0, -1.0, 0.0, 1.5], dtype=dt))
        assert u.tolist() == [at_one, at_one, at_zero, at_one]
    n = 8 * 512 * 80
    assert 1.5 * n * 2 < n * 2 + n * 4
