"""CPU: the entry points of the matrix-core attention backward (include/pdt_amd.h: pdt_attn_dot_mfma_backward_plan,
pdt_attn_dot_mfma_backward_elem) exist in the header, the ctypes table and the library; the plan admits exactly the
shapes of the forward's gate and no dot case of tests/_attn_ref.py (so the bit contract of tests/test_half_attn_* is
out of its reach); the launching entry point refuses everything it must before anything touches a GPU."""
import ctypes
import re

import pytest

import _attn_mfma as M
import _attn_ref as R
from test_attn_mfma_cpu import GOOD, HEADER, lib  # noqa: F401 (the fixture)

NAMES = ("pdt_attn_dot_mfma_backward_plan", "pdt_attn_dot_mfma_backward_elem")
BIG = dict(G=1, M=80, T=72, D=128, Dv=128)  # the GPU test's inline case


def plan(lib, d, elem):
    p = (ctypes.c_int64 * 5)()
    return lib.pdt_attn_dot_mfma_backward_plan(d, elem, ctypes.addressof(p)), list(p)


def test_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi, switches

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert name in _cabi.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(\s*const int64_t \*desc,\s*int elem,", src), name
    assert _cabi.SIGNATURES[NAMES[1]] == _cabi.SIGNATURES["pdt_attn_dot_backward_elem"]
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14
    assert "PDT_ATTN_MFMA_BWD" in switches.names() and switches.get("PDT_ATTN_MFMA_BWD") == 1


@pytest.mark.parametrize("elem", [2, 3])
def test_no_dot_case_of_the_suite_qualifies(lib, elem):
    for name, c in R.CASES.items():
        if c["route"] != "dot":
            continue
        G, m = R.plan_shape(c)
        assert plan(lib, M.desc(G, m, c["T"], max(1, c["D"]), c["Dv"]), elem) == (0, [0] * 5), name


@pytest.mark.parametrize("change", [
    dict(M=63), dict(D=48 + 8), dict(Dv=144), dict(D=16), dict(fs=2), dict(kv_ts=4), dict(q_row=68),
])  # fmt: skip
def test_plan_refuses_what_the_gate_excludes(lib, change):
    from pydrobert_amd import _cabi, switches

    assert plan(lib, M.desc(**GOOD), 2)[0] == 1
    assert plan(lib, M.desc(**dict(GOOD, **change)), 2) == (0, [0] * 5)
    assert plan(lib, M.desc(**GOOD), 0)[0] == 0  # float32
    assert plan(lib, M.desc(**GOOD), 1)[0] == _cabi.PDT_E_UNSUPPORTED
    assert plan(lib, M.desc(**GOOD), 7)[0] == _cabi.PDT_E_ARG
    bad = M.desc(**GOOD)
    bad[1] += 1  # R != G * M
    assert plan(lib, bad, 2)[0] == _cabi.PDT_E_ARG
    with switches.override(PDT_ATTN_MFMA_BWD=0):
        assert plan(lib, M.desc(**GOOD), 2) == (0, [0] * 5) and M.plan(lib, M.desc(**GOOD), 2)[0] == 1
    with switches.override(PDT_ATTN_MFMA=0):  # the forward's switch is not this one's
        assert plan(lib, M.desc(**GOOD), 2)[0] == 1 and M.plan(lib, M.desc(**GOOD), 2)[0] == 0


@pytest.mark.parametrize("name", list(M.CASES) + ["big"])
def test_plan_of_the_gpu_cases(lib, name):
    """rows and frames per workgroup, the workspace of R floats, and the LDS of each kernel by its tiles: K, K^T, V
    for grad_query; Q, Q^T, dO, dO^T for grad_key / grad_value, above 64 KiB exactly at D = Dv = 128."""
    c = BIG if name == "big" else M.CASES[name]
    G, m, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    for elem in (2, 3):
        ok, p = plan(lib, M.desc(G, m, T, D, Dv), elem)
        assert ok == 1 and p[:3] == [64, 64, 4 * G * m]
        assert p[3] == 2 * (64 * (D + 8) + D * 72 + 64 * (Dv + 8)) <= 64 * 1024
        assert p[4] == 2 * (64 * (D + 8) + D * 72 + 64 * (Dv + 8) + Dv * 72)
        assert (p[4] > 64 * 1024) == (D == 128 and Dv == 128)


def test_entry_point_refuses_before_any_launch(lib):
    from pydrobert_amd import _cabi

    ARG, UNSUP = _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    scale = ctypes.c_double(1.0)
    sp = ctypes.addressof(scale)
    good = M.desc(**GOOD)

    def call(d, e, s=sp, w=1 << 30, **ptr):  # every pointer 16 unless named: query .. workspace in argument order
        a = {n: ptr.get(n, 16) for n in ("q", "k", "v", "out", "lse", "go", "gq", "gk", "gv", "ws")}
        return lib.pdt_attn_dot_mfma_backward_elem(d, e, a["q"], a["k"], a["v"], 0, s, a["out"], a["lse"], a["go"],
                                                   a["gq"], a["gk"], a["gv"], a["ws"], w, 0)  # fmt: skip

    assert call(good, 0) == UNSUP and call(good, 1) == UNSUP and call(good, 5) == ARG
    for e in (2, 3):
        assert call(good, e, s=None) == ARG  # no scale
        assert call(M.desc(**dict(GOOD, M=63)), e) == UNSUP
        assert call(M.desc(**dict(GOOD, fs=2)), e) == UNSUP
        for n in ("q", "k", "v", "out", "lse", "go", "gq", "gk", "gv", "ws"):
            assert call(good, e, **{n: 0}) == ARG, n  # a null pointer
        for n in ("q", "k", "v", "go"):
            assert call(good, e, **{n: 24}) == ARG, n  # 16-byte loads
        for n, off in (("gq", 20), ("gk", 20), ("gv", 20), ("lse", 18), ("ws", 18)):
            assert call(good, e, **{n: off}) == ARG, n  # 8-byte stores, float32 reads
        need = plan(lib, good, e)[1][2]
        assert need == 4 * 2 * 64 and call(good, e, w=need - 1) == ARG
