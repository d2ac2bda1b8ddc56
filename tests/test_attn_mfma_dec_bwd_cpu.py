"""CPU: the entry points of the float32 decode attention backward (csrc/attn_mfma_dec_bwd.hip) exist in the header,
the ctypes table and the library; the plan admits every case of tests/_attn_mfma_dec.py with the forward's spans and
refuses one condition at a time; the launching entry point refuses everything it must before anything touches a GPU."""
import ctypes
import re

import pytest

import _attn_mfma_dec as M
from test_attn_mfma_cpu import HEADER, lib  # noqa: F401 (the library fixture, built on demand)

NAMES = ("pdt_attn_dot_mfma_dec_backward_plan", "pdt_attn_dot_mfma_dec_backward")
GOOD = dict(G=2, M=8, T=100, D=256, Dv=256)
PTRS = ("q", "k", "v", "out", "lse", "go", "gq", "gk", "gv", "ws")


def plan(lib, d):
    p = (ctypes.c_int64 * 5)()
    return lib.pdt_attn_dot_mfma_dec_backward_plan(d, ctypes.addressof(p)), list(p)


def grad_ts(d, ts):  # the T stride of grad_key
    from pydrobert_amd import _attn as A

    d[7 + A._MAX_DIMS + A._SGK * (A._MAX_DIMS + 2) + A._MAX_DIMS] = ts
    return d


def test_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi, switches

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        assert name in _cabi.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(\s*const int64_t \*desc,\s*(const void|int64_t) \*", src), name
        assert _cabi.SIGNATURES[name] == _cabi.SIGNATURES[name.replace("_dec_", "_f32_")]
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14
    assert "PDT_ATTN_MFMA_DEC_BWD" in switches.names() and switches.get("PDT_ATTN_MFMA_DEC_BWD") == 1


@pytest.mark.parametrize("name", list(M.CASES))
def test_plan_of_the_gpu_cases(lib, name):
    """The forward's spans; the dQ partials of several spans; LDS: P and dS [64][20] each, then the query and grad_out
    [16][D + 4] and [16][Dv + 4] or, if larger, the upper half of the frame slices' sums; the rows instance."""
    c = M.CASES[name]
    G, m, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    ok, p = plan(lib, M.desc(G, m, T, D, Dv))
    assert ok == 1 and p[0] == c["splits"] and p[1] == 64 * -(-(-(-T // 64)) // c["splits"])
    assert p[2] == (0 if c["splits"] == 1 else c["splits"] * G * m * D * 4)
    assert p[3] == 4 * (2 * 64 * 20 + max(16 * (D + Dv + 8), 256 // (D // 4) // 2 * m * D))
    assert (p[3] > 63 * 1024) == (name == "wide") and p[4] == (4 if m <= 4 else 8 if m <= 8 else 16)


@pytest.mark.parametrize("change", [dict(M=17), dict(D=48), dict(D=528), "grad T stride 6", "switch"], ids=str)
def test_gate_refuses_one_condition_at_a_time(lib, change):
    from pydrobert_amd import _cabi, switches

    bad = M.desc(**GOOD)
    bad[1] += 1  # R != G * M
    assert plan(lib, M.desc(**GOOD))[0] == 1 and plan(lib, bad)[0] == _cabi.PDT_E_ARG
    if change == "switch":
        with switches.override(PDT_ATTN_MFMA_DEC_BWD=0):
            assert plan(lib, M.desc(**GOOD)) == (0, [0] * 5) and M.plan(lib, M.desc(**GOOD))[0] == 1
        with switches.override(PDT_ATTN_MFMA_DEC=0):  # the forward's switch is not this one's
            assert plan(lib, M.desc(**GOOD))[0] == 1 and M.plan(lib, M.desc(**GOOD))[0] == 0
    elif isinstance(change, str):
        assert plan(lib, grad_ts(M.desc(**GOOD), 2 * 256 + 4))[0] == 1  # (a multiple of 4 is taken)
        assert plan(lib, grad_ts(M.desc(**GOOD), 6)) == (0, [0] * 5)
    else:
        assert plan(lib, M.desc(**dict(GOOD, **change))) == (0, [0] * 5)


def test_entry_point_refuses_before_any_launch(lib):
    from pydrobert_amd import _cabi

    ARG, UNSUP = _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    scale, good = ctypes.c_double(1.0), M.desc(**GOOD)

    def call(d, s=ctypes.addressof(scale), w=1 << 30, **ptr):  # every pointer 16 unless named
        a = {n: ptr.get(n, 16) for n in PTRS}
        return lib.pdt_attn_dot_mfma_dec_backward(d, a["q"], a["k"], a["v"], 0, s, a["out"], a["lse"], a["go"],
                                                  a["gq"], a["gk"], a["gv"], a["ws"], w, 0)  # fmt: skip

    assert call(good, s=None) == ARG  # no scale
    assert call(M.desc(**dict(GOOD, M=17))) == UNSUP and call(grad_ts(M.desc(**GOOD), 6)) == UNSUP
    for n in PTRS:
        assert call(good, **{n: 0}) == ARG, n  # a null pointer (GOOD has two spans: it needs its workspace)
        assert call(good, **{n: 18 if n in ("out", "lse") else 24}) == ARG, n  # 16-byte vectors; float32 reads
    need = plan(lib, good)[1][2]
    assert need == 2 * 2 * 8 * 256 * 4 and call(good, w=need - 1) == ARG
