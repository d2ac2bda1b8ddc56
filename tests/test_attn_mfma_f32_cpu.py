"""CPU: the entry points of the float32 matrix-core attention forward (include/pdt_amd.h:
pdt_attn_dot_mfma_f32_plan, pdt_attn_dot_mfma_f32) exist in the header, the ctypes table and the library; the plan
admits exactly the shapes of its gate and none of the float32 cases of tests/_attn_ref.py (so the bit contract of
tests/test_half_attn_* is out of its reach); the launching entry point refuses everything it must before anything
touches a GPU."""
import ctypes
import re

import pytest

import _attn_mfma_f32 as M
import _attn_ref as R
from test_attn_mfma_cpu import GOOD, HEADER, lib  # noqa: F401 (the library fixture, built on demand)


def test_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi, switches

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("pdt_attn_dot_mfma_f32_plan", "pdt_attn_dot_mfma_f32"):
        assert name in _cabi.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(\s*const int64_t \*desc,", src), name
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14
    assert "PDT_ATTN_MFMA_F32" in switches.names() and switches.get("PDT_ATTN_MFMA_F32") == 1


def test_no_float32_case_of_the_suite_qualifies(lib):
    assert M.plan(lib, M.desc(**GOOD))[0] == 1
    for name, c in R.CASES.items():
        if c["dtype"] == "float32" and c["route"] == "dot":
            G, m = R.plan_shape(c)
            assert M.plan(lib, M.desc(G, m, c["T"], max(1, c["D"]), c["Dv"])) == (0, [0] * 7), name


@pytest.mark.parametrize("change", [
    dict(M=63), dict(D=56), dict(Dv=144), dict(D=16), dict(fs=2), dict(kv_ts=2 * 64 + 2), dict(q_row=66),
])  # fmt: skip
def test_plan_refuses_what_the_gate_excludes(lib, change):
    assert M.plan(lib, M.desc(**dict(GOOD, **change))) == (0, [0] * 7)


def test_plan_follows_the_switch_and_checks_the_descriptor(lib):
    from pydrobert_amd import _cabi, switches

    bad = M.desc(**GOOD)
    bad[1] += 1  # R != G * M
    assert M.plan(lib, bad)[0] == _cabi.PDT_E_ARG
    with switches.override(PDT_ATTN_MFMA_F32=0):
        assert M.plan(lib, M.desc(**GOOD)) == (0, [0] * 7)
    assert M.plan(lib, M.desc(**GOOD))[0] == 1


@pytest.mark.parametrize("name", list(M.CASES))
def test_plan_of_the_gpu_cases(lib, name):
    """rows per workgroup, rows per wave, frames per key block, then the spans, workspace and LDS each case is
    named for: two tiles of 64 rows of D + 4 and Dv + 4 floats, above 64 KiB at big-lds alone."""
    c = M.CASES[name]
    G, m, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    ok, p = M.plan(lib, M.desc(G, m, T, D, Dv))
    assert ok == 1 and p[:3] == [64, 16, 64]
    blocks = -(-T // 64)
    assert p[3] == c["splits"] and p[4] == 64 * -(-blocks // c["splits"])
    assert p[5] == (0 if c["splits"] == 1 else c["splits"] * G * m * (Dv + 2) * 4)
    assert p[6] == 256 * (D + Dv + 8) and (p[6] > 64 * 1024) == (name == "big-lds")
    assert (M.CASES["tails-length"]["M"] % 64, M.CASES["tails-length"]["T"] % 64) == (36, 6)


def test_entry_point_refuses_before_any_launch(lib):
    from pydrobert_amd import _cabi

    ARG, UNSUP = _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    scale = ctypes.c_double(1.0)
    sp = ctypes.addressof(scale)
    good, split = M.desc(**GOOD), M.desc(1, 64, 300, 64, 64)
    call = lambda d, p=16, s=sp, w=1 << 30, q=None: lib.pdt_attn_dot_mfma_f32(  # noqa: E731
        d, p if q is None else q, p, p, 0, s, p, p, p, w, 0)
    assert call(good, s=None) == ARG  # no scale
    assert call(M.desc(**dict(GOOD, M=63))) == UNSUP
    assert call(M.desc(**dict(GOOD, fs=2))) == UNSUP
    assert call(good, p=0) == ARG  # null pointers
    assert call(good, q=20) == ARG  # a query four bytes off
    need = M.plan(lib, split)[1][5]
    assert need > 0 and call(split, w=need - 1) == ARG
