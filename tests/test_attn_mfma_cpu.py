"""CPU: the entry points of the matrix-core attention forward (include/pdt_amd.h: pdt_attn_dot_mfma_plan,
pdt_attn_dot_mfma_elem) exist in the header, the ctypes table and the library; the plan admits exactly the shapes
of its gate and none of the float32 cases of tests/_attn_ref.py (so the bit contract of tests/test_half_attn_*
is out of its reach); the launching entry point refuses everything it must before anything touches a GPU."""
import ctypes
import os
import re

import pytest

import _attn_mfma as M
import _attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdt_amd.h")
GOOD = dict(G=2, M=64, T=100, D=64, Dv=64)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


def test_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi, switches

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("pdt_attn_dot_mfma_plan", "pdt_attn_dot_mfma_elem"):
        assert name in _cabi.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(\s*const int64_t \*desc,\s*int elem,", src), name
    assert _cabi.SIGNATURES["pdt_attn_dot_mfma_elem"] == _cabi.SIGNATURES["pdt_attn_dot_elem"]
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14
    assert "PDT_ATTN_MFMA" in switches.names() and switches.get("PDT_ATTN_MFMA") == 1


@pytest.mark.parametrize("elem", [2, 3])
def test_no_float32_case_of_the_suite_qualifies(lib, elem):
    for name, c in R.CASES.items():
        if c["dtype"] != "float32" or c["route"] != "dot":
            continue
        G, m = R.plan_shape(c)
        assert M.plan(lib, M.desc(G, m, c["T"], max(1, c["D"]), c["Dv"]), elem) == (0, [0] * 7), name


@pytest.mark.parametrize("change", [
    dict(M=63), dict(D=48 + 8), dict(Dv=144), dict(D=16), dict(fs=2), dict(kv_ts=4), dict(q_row=68),
])  # fmt: skip
def test_plan_refuses_what_the_gate_excludes(lib, change):
    from pydrobert_amd import _cabi, switches

    assert M.plan(lib, M.desc(**GOOD), 2)[0] == 1
    assert M.plan(lib, M.desc(**dict(GOOD, **change)), 2) == (0, [0] * 7)
    assert M.plan(lib, M.desc(**GOOD), 0)[0] == 0  # float32
    assert M.plan(lib, M.desc(**GOOD), 1)[0] == _cabi.PDT_E_UNSUPPORTED
    assert M.plan(lib, M.desc(**GOOD), 7)[0] == _cabi.PDT_E_ARG
    bad = M.desc(**GOOD)
    bad[1] += 1  # R != G * M
    assert M.plan(lib, bad, 2)[0] == _cabi.PDT_E_ARG
    with switches.override(PDT_ATTN_MFMA=0):
        assert M.plan(lib, M.desc(**GOOD), 2) == (0, [0] * 7)


@pytest.mark.parametrize("name", list(M.CASES))
def test_plan_of_the_gpu_cases(lib, name):
    """rows per workgroup, rows per wave, frames per key block, then the spans, workspace and LDS each case is
    named for: a row tail where M is no multiple of 64, a key tail where T is none."""
    c = M.CASES[name]
    G, m, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    for elem in (2, 3):
        ok, p = M.plan(lib, M.desc(G, m, T, D, Dv), elem)
        assert ok == 1 and p[:3] == [64, 16, 64]
        blocks = -(-T // 64)
        assert p[3] == c["splits"] and p[4] == 64 * -(-blocks // c["splits"])
        assert p[5] == (0 if c["splits"] == 1 else c["splits"] * G * m * (Dv + 2) * 4)
        assert p[6] == 2 * (64 * (D + 8) + Dv * 72) <= 36 * 1024
    assert (M.CASES["tails-length"]["M"] % 64, M.CASES["tails-length"]["T"] % 64) == (36, 6)


def test_entry_point_refuses_before_any_launch(lib):
    from pydrobert_amd import _cabi

    ARG, UNSUP = _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    scale = ctypes.c_double(1.0)
    sp = ctypes.addressof(scale)
    good, split = M.desc(**GOOD), M.desc(1, 64, 300, 64, 64)
    call = lambda d, e, p=16, s=sp, w=1 << 30, q=None: lib.pdt_attn_dot_mfma_elem(  # noqa: E731
        d, e, p if q is None else q, p, p, 0, s, p, p, p, w, 0)
    assert call(good, 0) == UNSUP and call(good, 1) == UNSUP and call(good, 5) == ARG
    for e in (2, 3):
        assert call(good, e, s=None) == ARG  # no scale
        assert call(M.desc(**dict(GOOD, M=63)), e) == UNSUP
        assert call(M.desc(**dict(GOOD, fs=2)), e) == UNSUP
        assert call(good, e, p=0) == ARG  # null pointers
        assert call(good, e, q=18) == ARG  # a query two bytes off
        need = M.plan(lib, split, e)[1][5]
        assert need > 0 and call(split, e, w=need - 1) == ARG
