"""CPU: the entry points that read float16 / bfloat16 logits as they are (include/pdt_amd.h, "_elem") exist in
the header, the ctypes table and the library; they validate the element code and the pointers before anything
touches a GPU; the case table of tests/_half_logits.py reaches every kernel form it names; and the ABI version
is the one the rest of the suite pins."""
import ctypes
import os
import re

import pytest

from _half_logits import CTC_CASES, NOCOPY, STRIDED_VOCAB, case_vocab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdt_amd.h")

ELEM_ENTRIES = (
    "pdt_ctc_prefix_search_elem",
    "pdt_ctc_prefix_search_wide_elem",
    "pdt_ctc_greedy_search_elem",
    "pdt_sequence_log_probs_forward_elem",
    "pdt_sequence_log_probs_backward_elem",
)


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
    for name in ELEM_ENTRIES + ("pdt_ctc_prefix_search_wide_plan",):
        assert re.search(r"\b" + name + r"\s*\(", src), name + " is not declared in pdt_amd.h"
        assert name in _cabi.SIGNATURES, name + " is not in the ctypes table"
        assert hasattr(lib, name), "libpdt_amd.so does not export " + name
    for name in ELEM_ENTRIES:
        sibling = name[: -len("_elem")]
        res, args = _cabi.SIGNATURES[name]
        sres, sargs = _cabi.SIGNATURES[sibling]
        assert res is sres and args == sargs + [ctypes.c_int], name  # the sibling's arguments + `int elem`
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert "const void *logits" in m.group(1) and m.group(1).rstrip().endswith("int elem"), name
    m = re.search(r"\bpdt_sequence_log_probs_backward_elem\s*\((.*?)\)\s*;", src, flags=re.S)
    assert "void *grad_logits" in m.group(1) and "float *grad_logits" not in m.group(1)


def test_abi_version_is_still_14(lib):
    from pydrobert_amd import _cabi

    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14


def _calls(lib):
    """name -> f(logits, elem): each _elem entry point with a non-empty problem and made-up non-null pointers
    for everything but the logits (never dereferenced: every call here returns before a launch)."""
    return {
        "pdt_ctc_prefix_search_elem": lambda lg, e: lib.pdt_ctc_prefix_search_elem(
            lg, 5, 2, 40, 82, 41, 1, 0, 4, 5, 1, 1, 1, 1, 0, e),
        "pdt_ctc_prefix_search_wide_elem": lambda lg, e: lib.pdt_ctc_prefix_search_wide_elem(
            lg, 5, 2, 40, 82, 41, 1, 0, 64, 5, 1, 1, 1, 1, 0, e),
        "pdt_ctc_greedy_search_elem": lambda lg, e: lib.pdt_ctc_greedy_search_elem(
            lg, 5, 2, 41, 82, 41, 1, 0, 40, 0, 1, 1, 2, 1, 1, 0, e),
        "pdt_sequence_log_probs_forward_elem": lambda lg, e: lib.pdt_sequence_log_probs_forward_elem(
            lg, 1, 1, 5, 2, 41, 0, 0, 1, 0, e),
        "pdt_sequence_log_probs_backward_elem": lambda lg, e: lib.pdt_sequence_log_probs_backward_elem(
            lg, 1, 1, 5, 2, 41, 0, 0, 1, 1, 0, e),
    }  # fmt: skip


def test_elem_codes_and_null_logits_without_gpu(lib):
    from pydrobert_amd import _cabi

    for name, call in _calls(lib).items():
        assert call(1, 1) == _cabi.PDT_E_UNSUPPORTED, name  # float64: no kernel
        for bad in (7, -1, 4):
            assert call(1, bad) == _cabi.PDT_E_ARG, (name, bad)
        for elem in (0, 2, 3):  # null logits with T > 0 (S > 0), every element type the kernels read
            assert call(0, elem) == _cabi.PDT_E_ARG, (name, elem)
    # an empty batch is nothing to do for every element type the kernels read
    for elem in (0, 2, 3):
        assert lib.pdt_ctc_prefix_search_elem(0, 5, 0, 40, 1, 1, 1, 0, 4, 5, 0, 0, 0, 0, 0, elem) == _cabi.PDT_OK
        assert lib.pdt_ctc_prefix_search_wide_elem(0, 5, 0, 40, 1, 1, 1, 0, 64, 5, 0, 0, 0, 0, 0, elem) == _cabi.PDT_OK
        assert lib.pdt_ctc_greedy_search_elem(0, 5, 0, 41, 1, 1, 1, 0, 40, 0, 0, 0, 1, 1, 0, 0, elem) == _cabi.PDT_OK
        assert lib.pdt_sequence_log_probs_forward_elem(0, 0, 0, 5, 2, 41, 0, 0, 0, 0, elem) == _cabi.PDT_OK
        assert lib.pdt_sequence_log_probs_backward_elem(0, 0, 0, 5, 2, 41, 0, 0, 0, 0, 0, elem) == _cabi.PDT_OK
    # the float32 entry points are untouched: same answers as before
    assert lib.pdt_ctc_prefix_search(0, 5, 2, 40, 82, 41, 1, 0, 4, 5, 1, 1, 1, 1, 0) == _cabi.PDT_E_ARG
    assert lib.pdt_sequence_log_probs_forward(0, 1, 1, 5, 2, 41, 0, 0, 1, 0) == _cabi.PDT_E_ARG


def test_wide_plan_query(lib):
    from pydrobert_amd import _cabi

    plan = (ctypes.c_int32 * 2)()
    assert lib.pdt_ctc_prefix_search_wide_plan(40, 64, None) == _cabi.PDT_E_ARG
    assert lib.pdt_ctc_prefix_search_wide_plan(0, 64, plan) == _cabi.PDT_E_ARG
    assert lib.pdt_ctc_prefix_search_wide_plan(40, 0, plan) == _cabi.PDT_E_ARG
    assert lib.pdt_ctc_prefix_search_wide_plan(40, 129, plan) == _cabi.PDT_E_TOO_LONG
    assert lib.pdt_ctc_prefix_search_wide_plan(40, 64, plan) == _cabi.PDT_OK and list(plan) == [1, 1]
    assert lib.pdt_ctc_prefix_search_wide_plan(40, 65, plan) == _cabi.PDT_OK and list(plan) == [1, 0]
    assert lib.pdt_ctc_prefix_search_wide_plan(40000, 65, plan) == _cabi.PDT_OK and list(plan) == [0, 0]


def test_case_table_reaches_every_form(lib):
    """Through the plan queries: each CTC case is served by the form its name claims.  A strided vocabulary
    never takes the rows-in-registers form, so those cases are looked up with that form switched off -- the plan
    that then answers is the one the launcher falls through to."""
    from pydrobert_amd import _cabi, switches

    plan5 = (ctypes.c_int32 * 5)()
    plan2 = (ctypes.c_int32 * 2)()
    seen = set()
    for name, case in CTC_CASES.items():
        V, W, form = case_vocab(lib, name), case["W"], case["form"]
        if form[0] == "wide":
            assert 32 < W <= 128, name
            assert lib.pdt_ctc_prefix_search_wide_plan(V, W, plan2) == _cabi.PDT_OK, name
            assert tuple(plan2) == form[1:], (name, V, tuple(plan2))
            if case["V"] is None:  # the first V past the bound: the one before it still has its row in LDS
                assert lib.pdt_ctc_prefix_search_wide_plan(V - 1, W, plan2) == _cabi.PDT_OK and plan2[0] == 1, name
            seen.add(form)
            continue
        assert W <= 32, name
        if name in STRIDED_VOCAB:
            assert case["layout"] == "transposed", name
            assert lib.pdt_ctc_prefix_search_plan(V, W, plan5) == _cabi.PDT_OK and plan5[3] == 3, name  # (rowreg, were it contiguous)
            with switches.override(PDT_CTC_ROWREG=0):
                assert lib.pdt_ctc_prefix_search_plan(V, W, plan5) == _cabi.PDT_OK, name
        else:
            assert lib.pdt_ctc_prefix_search_plan(V, W, plan5) == _cabi.PDT_OK, name
        got = (plan5[0], plan5[3], plan5[4])
        assert got == form[1:], (name, got)
        seen.add(("narrow", plan5[0], plan5[3], plan5[4], V // 64 == 4, W == 16, V == 256))
    # the named instances inside the one-producer form: NT = 4, with and without the width-16 instance, V = 256
    assert ("narrow", 1, 1, 0, False, False, False) in seen  # general
    assert ("narrow", 1, 1, 0, True, False, False) in seen  # four chunks
    assert ("narrow", 1, 1, 0, True, True, False) in seen  # four chunks, width 16
    assert ("narrow", 1, 1, 0, True, True, True) in seen  # the headline shape
    for chunks in (8, 16, 24, 80):
        assert any(s[:4] == ("narrow", 3, 3, chunks) for s in seen), chunks
    assert any(s[:3] == ("narrow", 3, 0) for s in seen) and any(s[:3] == ("narrow", 3, 2) for s in seen)
    assert {("wide", 1, 1), ("wide", 1, 0), ("wide", 0, 1), ("wide", 0, 0)} <= seen
    # rem = V mod 64 of the two rowreg edge cases
    assert CTC_CASES["rowreg_rem0_nr8"]["V"] % 64 == 0 and CTC_CASES["rowreg_rem63_nr16"]["V"] % 64 == 63
    # beyond the rowreg range: more than 256 chunks of 64
    assert CTC_CASES["workspace_rows"]["V"] // 64 > 256


def test_nocopy_allowance_is_below_the_float32_copy(lib):
    """The sizes the GPU test of the same name relies on: outputs + the workspace the query reports stay far
    below the float32 copy of the logits that the half-precision route no longer makes."""
    T, N, V, W = NOCOPY["T"], NOCOPY["N"], NOCOPY["V"], NOCOPY["W"]
    copy_bytes = T * N * (V + 1) * 4
    assert copy_bytes == 8_192_000
    ws = lib.pdt_ctc_prefix_search_workspace_bytes(T, N, V, W)
    trie = (T + T // 32 + 1) * N * W * 8
    assert trie == 34_304 and trie <= ws <= trie + 1024  # (rows of 2000 stay in registers: no rows in the workspace)
    outputs = T * N * W * 8 + N * W * 8 + N * W * 4 + N * W * 2
    assert ws + outputs + (1 << 20) < copy_bytes
    assert T * N * (V + 1) * 2 + (1 << 20) < copy_bytes  # the backward's gradient in the half type
