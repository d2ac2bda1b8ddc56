"""GPU: fill_after_eos in every launch form of csrc/fill_after_eos.hip, with the first eos planted where the
kernels' ballots, carries and minima have to find it (tests/_fill_forms.py; the coverage the cases give is asserted
without a GPU in tests/test_fill_forms_cpu.py).  The expected output is the oracle's (oracle.fill_after_eos);
values are compared as raw bits."""
import numpy as np
import pytest
import torch

import _fill_forms as ff
import oracle
from pydrobert_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

BITS_TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _typed(vbits, name):
    """The numpy words on the device as a tensor of dtype ``name``."""
    return torch.from_numpy(vbits).to(DEV).view(getattr(torch, name))


def _bits(t):
    return t.contiguous().view(BITS_TORCH[t.element_size()]).cpu().numpy()


def _check_positions(case, tok, eos=ff.EOS):
    assert np.array_equal(ff.first_eos(tok, eos), case.first), case


def _run_case(case, dtype="int64", fills=None, seed=0):
    """One case through the operator with a value tensor of ``dtype`` and every fill of ``fills``."""
    tok = ff.build_tokens(case.first, case.L, seed=seed)
    _check_positions(case, tok)
    shape = tok.shape if case.kernel == "cols" else tok.shape[:2]
    tk = torch.from_numpy(tok.reshape(shape)).to(DEV)
    vbits = ff.value_bits(shape, dtype, seed)
    val = _typed(vbits, dtype)
    for fill, fill_bits in ff.FILLS[dtype] if fills is None else fills:
        act = F.fill_after_eos(tk, ff.EOS, 1, fill, val)
        exp = ff.expected_bits(tok, ff.EOS, vbits.reshape(tok.shape), fill_bits).reshape(shape)
        assert act.dtype == val.dtype and act.shape == val.shape
        got = _bits(act).astype(exp.dtype)  # (uint8 words of a bool tensor compare as uint8)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (case.kernel, case.outer, case.L, case.inner, dtype, fill, bad[:4].tolist(),
                               case.first.reshape(-1)[:8].tolist())  # fmt: skip
    return tok, tk


@pytest.mark.parametrize("L", ff.ROWS_L)
def test_rows_kernel_finds_the_first_eos_wherever_it_is(L):
    """inner == 1: no eos, eos at 0, at lanes 63 and 64, at 511 and 512 (the last position of a pass and the
    first of the next), at L - 1 and at a random interior position, in every wave of a workgroup; the default
    call (value None, fill = eos) and an int64 value with a negative fill."""
    for case in ff.rows_cases(L):
        tok, tk = _run_case(case)
        assert np.array_equal(F.fill_after_eos(tk, ff.EOS, 1).cpu().numpy(), oracle.fill_after_eos(tok[:, :, 0], ff.EOS, 1))
        assert np.array_equal(F.fill_after_eos(tk, ff.EOS, -1, 9.0).cpu().numpy(), oracle.fill_after_eos(tok[:, :, 0], ff.EOS, 1, 9.0))


@pytest.mark.parametrize("L", ff.COLS_L)
def test_columns_kernel_finds_the_first_eos_in_every_tier(L):
    """inner > 1: every tier of waves at both ends, one to three passes at 16 waves, outer * inner below, at and
    above multiples of 64, every column its own position."""
    for case in ff.cols_cases(L):
        tok, tk = _run_case(case)
        assert np.array_equal(F.fill_after_eos(tk, ff.EOS, 1).cpu().numpy(), oracle.fill_after_eos(tok, ff.EOS, 1))
        if case.outer == 1:  # the same launch reached through dim 0 of a matrix
            assert np.array_equal(F.fill_after_eos(tk[0], ff.EOS, 0).cpu().numpy(), oracle.fill_after_eos(tok[0], ff.EOS, 0))


@pytest.mark.parametrize("dtype", ff.DTYPES)
def test_every_word_width_and_fill_pattern_on_both_kernels(dtype):
    """Values move as opaque words of 1, 2, 4 and 8 bytes: every bit pattern of the value comes through, and the
    fill's bits (a negative integer, -0.0, NaN, True) are the ones torch's conversion of the scalar gives."""
    for shape in ff.DTYPE_ROWS + ff.DTYPE_COLS:
        for case in ff.shape_cases(shape):
            _run_case(case, dtype, seed=1)
    # the bits this test expects of the fill are torch's own
    for fill, fill_bits in ff.FILLS[dtype]:
        one = torch.full((1,), fill, dtype=getattr(torch, dtype))
        assert int(_bits(one).astype(ff.WIDTHS[ff.width_of(dtype)][0])[0]) == fill_bits, (dtype, fill)


@pytest.mark.parametrize("shape", [ff.LONG_ROWS, ff.LONG_COLS], ids=["rows", "cols"])
def test_tokens_of_other_dtypes_and_transposed_views(shape):
    """Tokens that are not int64 compare against eos as ``tokens == eos`` does; tokens and value that are
    transposed views are walked along the dimension the caller names."""
    for case in ff.shape_cases(shape):
        tok = ff.build_tokens(case.first, case.L, seed=2)
        sq = tok if case.kernel == "cols" else tok[:, :, 0]
        vbits = ff.value_bits(sq.shape, "float32", 2)
        exp = ff.expected_bits(sq, ff.EOS, vbits, -7)
        for tdt in (torch.int32, torch.uint8, torch.int16, torch.float32, torch.float64):
            tk = torch.from_numpy(sq).to(DEV).to(tdt)
            assert np.array_equal(_bits(F.fill_after_eos(tk, ff.EOS, 1, -7.0, _typed(vbits, "int32"))), exp), tdt
            d = F.fill_after_eos(tk, ff.EOS, 1)
            assert d.dtype == tdt and np.array_equal(d.cpu().numpy(), oracle.fill_after_eos(sq.astype(d.cpu().numpy().dtype), ff.EOS, 1))
        # the walked dimension moved to the front of a transposed view: the contiguous memory is (L, ...)
        perm = (1, 0) if sq.ndim == 2 else (1, 0, 2)
        tt = torch.from_numpy(np.ascontiguousarray(sq.transpose(perm))).to(DEV).permute(perm)
        vt = _typed(np.ascontiguousarray(vbits.transpose(perm)), "int32").permute(perm)
        assert not tt.is_contiguous() and not vt.is_contiguous() and tt.shape == sq.shape
        assert np.array_equal(_bits(F.fill_after_eos(tt, ff.EOS, 1, -7.0, vt)), exp)
        assert np.array_equal(_bits(F.fill_after_eos(tt, ff.EOS, 1, -7.0, _typed(vbits, "int32"))), exp)
        if sq.ndim == 2:
            # ... and walked along dimension 0 of the transposed matrix: the columns kernel at this L
            exp_t = ff.expected_bits(sq, ff.EOS, vbits, -7).T
            act = F.fill_after_eos(tt.t(), ff.EOS, 0, -7.0, _typed(np.ascontiguousarray(vbits.T), "int32"))
            assert np.array_equal(_bits(act), exp_t)


@pytest.mark.parametrize("shape", [ff.LONG_ROWS, ff.LONG_COLS, (3, 9, 65)], ids=["rows", "cols16", "cols2"])
@pytest.mark.parametrize("eos", ff.INT64_ENDS[:2], ids=["max", "min"])
def test_eos_at_the_ends_of_int64(shape, eos):
    """Both ends of int64 are tokens, each the eos once: the lanes beyond L, which the kernels pad with eos + 1,
    are never taken for an eos, and eos itself is compared in all 64 bits."""
    for case in ff.shape_cases(shape):
        tok = ff.build_tokens(case.first, case.L, eos, ff.INT64_ENDS, seed=3)
        assert (tok == 2**63 - 1).any() and (tok == -(2**63)).any() or case.L < 3
        _check_positions(case, tok, eos)
        sq = tok if case.kernel == "cols" else tok[:, :, 0]
        tk = torch.from_numpy(sq).to(DEV)
        vbits = ff.value_bits(sq.shape, "int64", 3)
        act = F.fill_after_eos(tk, eos, 1, -1.0, _typed(vbits, "int64"))
        assert np.array_equal(_bits(act), ff.expected_bits(sq, eos, vbits, -1))
        act = F.fill_after_eos(tk, eos, 1, -1.0)
        assert np.array_equal(_bits(act), ff.expected_bits(sq, eos, sq, -1))
        # the default fill is eos itself, also where a double does not hold it (2^63 - 1)
        assert np.array_equal(_bits(F.fill_after_eos(tk, eos, 1)), ff.expected_bits(sq, eos, sq, eos))
        assert np.array_equal(F.fill_after_eos(tk, eos, 1).cpu().numpy(), oracle.fill_after_eos(sq, eos, 1))


@pytest.mark.parametrize("shape", [ff.LONG_ROWS, ff.LONG_COLS], ids=["rows", "cols"])
def test_gradient_is_the_keep_mask(shape):
    """The gradient with respect to ``value`` is exactly the oracle's keep-mask: a rows shape of more than one
    pass, a columns shape at 16 waves."""
    for case in ff.shape_cases(shape):
        tok = ff.build_tokens(case.first, case.L, seed=4)
        sq = tok if case.kernel == "cols" else tok[:, :, 0]
        tk = torch.from_numpy(sq).to(DEV)
        v = torch.randn(sq.shape, device=DEV, requires_grad=True)
        out = F.fill_after_eos(tk, ff.EOS, 1, 0.25, v)
        g = torch.randn(sq.shape, device=DEV)
        (gv,) = torch.autograd.grad((out * g).sum(), v)
        keep = torch.from_numpy(ff.keep_mask(sq, ff.EOS)).to(DEV)
        assert torch.equal(gv, torch.where(keep, g, torch.zeros_like(g)))
        (g1,) = torch.autograd.grad(F.fill_after_eos(tk, ff.EOS, 1, 0.25, v).sum(), v)
        assert torch.equal(g1, keep.float())
