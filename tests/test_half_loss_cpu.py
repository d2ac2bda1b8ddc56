"""CPU: the entry points through which the hard optimal-completion distillation loss reads float16 / bfloat16
logits as they are (include/pdt_amd.h: pdt_ocd_loss_forward_elem, pdt_ocd_loss_backward_elem) exist in the
header, the ctypes table and the library; they validate the element code and the pointers before anything
touches a GPU; and the memory allowances of the GPU no-copy test are below the float32 copy they rule out."""
import ctypes
import os
import re

import pytest

import _half_loss as hlo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdt_amd.h")

ELEM_ENTRIES = ("pdt_ocd_loss_forward_elem", "pdt_ocd_loss_backward_elem")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def test_elem_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ELEM_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), name + " is not declared in pdt_amd.h"
        assert name in _cabi.SIGNATURES, name + " is not in the ctypes table"
        assert hasattr(lib, name), "libpdt_amd.so does not export " + name
        sibling = name[: -len("_elem")]
        res, args = _cabi.SIGNATURES[name]
        sres, sargs = _cabi.SIGNATURES[sibling]
        assert res is sres and args == sargs + [ctypes.c_int], name  # the sibling's arguments + `int elem`
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert "const void *logits" in m.group(1) and m.group(1).rstrip().endswith("int elem"), name
        # the float32 sibling keeps its declaration
        m = re.search(r"\b" + sibling + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert "const float *logits" in m.group(1) and m.group(1).rstrip().endswith("void *stream"), sibling
    m = re.search(r"\bpdt_ocd_loss_backward_elem\s*\((.*?)\)\s*;", src, flags=re.S)
    assert "void *grad_logits" in m.group(1) and "float *grad_logits" not in m.group(1)
    m = re.search(r"\bpdt_ocd_loss_backward\s*\((.*?)\)\s*;", src, flags=re.S)
    assert "float *grad_logits" in m.group(1)


def test_abi_version_is_still_14(lib):
    from pydrobert_amd import _cabi

    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14


def _calls(lib):
    """name -> f(logits, elem, H, N): each _elem entry point with made-up non-null pointers for everything but
    the logits (never dereferenced: every call here returns before a launch).  V = 5, R = 3."""
    return {
        "pdt_ocd_loss_forward_elem": lambda lg, e, H=2, N=2: lib.pdt_ocd_loss_forward_elem(
            lg, H, N, 5, 10, 5, 1, 1, 1, 3, 0, -2, 1, 1, 0, 0, e),
        "pdt_ocd_loss_backward_elem": lambda lg, e, H=2, N=2: lib.pdt_ocd_loss_backward_elem(
            lg, H, N, 5, 10, 5, 1, 1, 1, 3, 0, -2, 1, 1, 0, e),
    }  # fmt: skip


def test_elem_codes_and_null_logits_without_gpu(lib):
    from pydrobert_amd import _cabi

    for name, call in _calls(lib).items():
        assert call(1, 1) == _cabi.PDT_E_UNSUPPORTED, name  # float64: no kernel
        for bad in (7, -1, 4):
            assert call(1, bad) == _cabi.PDT_E_ARG, (name, bad)
        for elem in (0, 2, 3):
            assert call(0, elem) == _cabi.PDT_E_ARG, (name, elem)  # null logits with H, N > 0
            assert call(0, elem, H=0) == _cabi.PDT_OK, (name, elem)  # nothing to do
            assert call(0, elem, N=0) == _cabi.PDT_OK, (name, elem)
            assert call(1, elem, H=0) == _cabi.PDT_OK and call(1, elem, N=0) == _cabi.PDT_OK, (name, elem)
        # the element code is looked at before the sizes say there is nothing to do
        assert call(0, 1, H=0) == _cabi.PDT_E_UNSUPPORTED and call(0, 9, N=0) == _cabi.PDT_E_ARG, name
    # the float32 entry points: same answers as before
    assert lib.pdt_ocd_loss_forward(0, 2, 2, 5, 10, 5, 1, 1, 1, 3, 0, -2, 1, 1, 0, 0) == _cabi.PDT_E_ARG
    assert lib.pdt_ocd_loss_backward(0, 2, 2, 5, 10, 5, 1, 1, 1, 3, 0, -2, 1, 1, 0) == _cabi.PDT_E_ARG
    assert lib.pdt_ocd_loss_forward(1, 2, 2, 5, 10, 5, 1, 0, 1, 3, 0, -2, 1, 1, 0, 0) == _cabi.PDT_E_ARG  # no bitmask
    assert lib.pdt_ocd_loss_backward(1, 2, 2, 5, 10, 5, 1, 1, 1, 3, 0, -2, 1, 0, 0) == _cabi.PDT_E_ARG  # no gradient
    assert lib.pdt_ocd_loss_forward(0, 0, 2, 5, 10, 5, 1, 0, 0, 3, 0, -2, 0, 0, 0, 0) == _cabi.PDT_OK
    assert lib.pdt_ocd_loss_backward(0, 2, 0, 5, 10, 5, 1, 0, 0, 3, 0, -2, 0, 0, 0) == _cabi.PDT_OK
    assert lib.pdt_ocd_loss_forward(1, 2, 2, 0, 10, 5, 1, 1, 1, 3, 0, -2, 1, 1, 0, 0) == _cabi.PDT_E_ARG  # V < 1
    assert lib.pdt_ocd_loss_forward(1, 2, 2, 1 << 30, 10, 5, 1, 1, 1, 3, 0, -2, 1, 1, 0, 0) == _cabi.PDT_E_TOO_LONG


def test_nocopy_allowances_are_below_the_float32_copy(lib):
    """The sizes the GPU test of the same name relies on: what each operator may allocate on half logits,
    plus the allocator's rounding, stays below the float32 copy of the logits that the parent route made."""
    H, N, V, R = (hlo.NOCOPY[k] for k in ("H", "N", "V", "R"))
    copy_bytes = H * N * V * 4
    assert copy_bytes == 8_192_000
    fwd = hlo.forward_allowance(lib, H, N, V, R)
    assert lib.pdt_oc_mask_words(R) == 1
    fixed = H * N * 4 + N * R * 8 + 12 + H * N * 4 + H * N * 4  # bitmask, class tokens, status, loss, count
    assert fwd == fixed + lib.pdt_oc_mask_workspace_bytes(R, H, N) and fwd >= fixed == 13_836
    assert fwd + hlo.MIB < copy_bytes
    for elem_size in (2,):  # float16 and bfloat16
        bwd = hlo.backward_allowance(H, N, V, elem_size)
        assert bwd == 4_096_000 + H * N * 4
        assert bwd + hlo.MIB < copy_bytes
