"""CPU: the entry points of the float32 matrix-core attention backward exist in the header, the ctypes table and the
library; the plan admits exactly its gate and no float32 dot case of tests/_attn_ref.py; the launching entry point
refuses everything it must before anything touches a GPU."""
import ctypes
import re

import pytest

import _attn_mfma_f32 as M
import _attn_mfma_forms as F
import _attn_ref as R
from test_attn_mfma_cpu import GOOD, HEADER, lib  # noqa: F401 (the library fixture, built on demand)

NAMES = ("pdt_attn_dot_mfma_f32_backward_plan", "pdt_attn_dot_mfma_f32_backward")
GPU_CASES = dict(M.CASES, **{n: F.FORMS[n] for n in F.BACKWARD_FORMS})


def plan(lib, d):
    p = (ctypes.c_int64 * 5)()
    return lib.pdt_attn_dot_mfma_f32_backward_plan(d, ctypes.addressof(p)), list(p)


def test_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi, switches

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert name in _cabi.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(\s*const int64_t \*desc,\s*(const void|int64_t) \*", src), name
    half = _cabi.SIGNATURES["pdt_attn_dot_mfma_backward_elem"]
    assert _cabi.SIGNATURES[NAMES[1]] == (half[0], half[1][:1] + half[1][2:])  # (the same without elem)
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14
    assert "PDT_ATTN_MFMA_F32_BWD" in switches.names() and switches.get("PDT_ATTN_MFMA_F32_BWD") == 1


def test_no_float32_case_of_the_suite_qualifies(lib):
    assert plan(lib, M.desc(**GOOD))[0] == 1
    for name, c in R.CASES.items():
        if c["dtype"] == "float32" and c["route"] == "dot":
            G, m = R.plan_shape(c)
            assert plan(lib, M.desc(G, m, c["T"], max(1, c["D"]), c["Dv"])) == (0, [0] * 5), name


@pytest.mark.parametrize("change", [
    dict(M=63), dict(D=48 + 8), dict(Dv=144), dict(D=16), dict(fs=2), dict(kv_ts=2 * 64 + 2), dict(q_row=66),
])  # fmt: skip
def test_plan_refuses_what_the_gate_excludes(lib, change):
    assert plan(lib, M.desc(**dict(GOOD, **change))) == (0, [0] * 5)


def test_plan_follows_its_own_switch_and_checks_the_descriptor(lib):
    from pydrobert_amd import _cabi, switches

    bad = M.desc(**GOOD)
    bad[1] += 1  # R != G * M
    assert plan(lib, bad)[0] == _cabi.PDT_E_ARG
    with switches.override(PDT_ATTN_MFMA_F32_BWD=0):
        assert plan(lib, M.desc(**GOOD)) == (0, [0] * 5) and M.plan(lib, M.desc(**GOOD))[0] == 1
    with switches.override(PDT_ATTN_MFMA_F32=0):  # the forward's switch is not this one's
        assert plan(lib, M.desc(**GOOD))[0] == 1 and M.plan(lib, M.desc(**GOOD))[0] == 0


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_plan_of_the_gpu_cases(lib, name):
    """64 rows, 64 frames, R floats, and each kernel's dynamic LDS: two tiles of 64 rows of D + 4 and Dv + 4 floats."""
    c = GPU_CASES[name]
    G, m, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    ok, p = plan(lib, M.desc(G, m, T, D, Dv))
    assert ok == 1 and p[:3] == [64, 64, 4 * G * m]
    assert p[3] == p[4] == 256 * (D + Dv + 8) and (p[3] > 64 * 1024) == (D == 128 and Dv == 128)


def test_entry_point_refuses_before_any_launch(lib):
    from pydrobert_amd import _cabi

    ARG, UNSUP = _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    scale, good = ctypes.c_double(1.0), M.desc(**GOOD)

    def call(d, s=ctypes.addressof(scale), w=1 << 30, **ptr):  # every pointer 16 unless named
        a = {n: ptr.get(n, 16) for n in ("q", "k", "v", "out", "lse", "go", "gq", "gk", "gv", "ws")}
        return lib.pdt_attn_dot_mfma_f32_backward(d, a["q"], a["k"], a["v"], 0, s, a["out"], a["lse"], a["go"],
                                                  a["gq"], a["gk"], a["gv"], a["ws"], w, 0)  # fmt: skip

    assert call(good, s=None) == ARG  # no scale
    assert call(M.desc(**dict(GOOD, M=63))) == UNSUP
    assert call(M.desc(**dict(GOOD, fs=2))) == UNSUP
    for n in ("q", "k", "v", "out", "lse", "go", "gq", "gk", "gv", "ws"):
        assert call(good, **{n: 0}) == ARG, n  # a null pointer
        if n != "out":  # 16-byte loads and stores; float32 reads of lse and the workspace
            assert call(good, **{n: 18 if n in ("lse", "ws") else 24}) == ARG, n
    need = plan(lib, good)[1][2]
    assert need == 4 * 2 * 64 and call(good, w=need - 1) == ARG
