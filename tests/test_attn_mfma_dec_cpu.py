"""CPU: the entry points of the float32 decode attention forward (include/pdt_amd.h: pdt_attn_dot_mfma_dec_plan,
pdt_attn_dot_mfma_dec) exist in the header, the ctypes table and the library; the plan admits exactly the shapes of
its gate and none of the float32 cases of tests/_attn_ref.py (so the bit contract of tests/test_half_attn_* is out of
its reach), and never asks for more workspace than pdt_attn_workspace_bytes reports; the launching entry point
refuses everything it must before anything touches a GPU."""
import ctypes
import re

import pytest

import _attn_mfma_dec as M
import _attn_ref as R
from test_attn_mfma_cpu import HEADER, lib  # noqa: F401 (the library fixture, built on demand)

GOOD = dict(G=2, M=8, T=100, D=256, Dv=256)


def test_entry_points_in_header_table_and_library(lib):
    from pydrobert_amd import _cabi, switches

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("pdt_attn_dot_mfma_dec_plan", "pdt_attn_dot_mfma_dec"):
        assert name in _cabi.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(\s*const int64_t \*desc,", src), name
        assert _cabi.SIGNATURES[name] == _cabi.SIGNATURES[name.replace("_dec", "_f32")]
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14
    assert "PDT_ATTN_MFMA_DEC" in switches.names() and switches.get("PDT_ATTN_MFMA_DEC") == 1


def test_no_float32_case_of_the_suite_qualifies(lib):
    assert M.plan(lib, M.desc(**GOOD))[0] == 1
    for name, c in R.CASES.items():
        if c["dtype"] == "float32" and c["route"] == "dot":
            G, m = R.plan_shape(c)
            assert M.plan(lib, M.desc(G, m, c["T"], max(1, c["D"]), c["Dv"])) == (0, [0] * 7), name


@pytest.mark.parametrize("change", [
    dict(M=17), dict(D=48), dict(D=72), dict(Dv=528), dict(fs=2), dict(kv_ts=6), "float64", "switch",
], ids=str)  # fmt: skip
def test_gate_refusal_by_refusal(lib, change):
    from pydrobert_amd import _attn, _cabi, switches

    bad = M.desc(**GOOD)
    bad[1] += 1  # R != G * M
    assert M.plan(lib, M.desc(**GOOD))[0] == 1 and M.plan(lib, bad)[0] == _cabi.PDT_E_ARG
    if change == "float64":  # (the plan is float32's: the host asks it for no other dtype -- GOOD's own tensors)
        import torch

        for dt, taken in ((torch.float32, True), (torch.float64, False)):
            q, k, v = (torch.zeros(s, dtype=dt) for s in ((2, 8, 256), (100, 2, 1, 256), (100, 2, 1, 256)))
            plan, ops = _attn._dot_plan(q, k, v, None, 0)
            code = _attn._dtype_code(q, k, v, mask=None, half=True)
            assert (_attn._mfma_dec_workspace_bytes(plan, code, ops) >= 0) == taken
    elif change == "switch":
        with switches.override(PDT_ATTN_MFMA_DEC=0):
            assert M.plan(lib, M.desc(**GOOD)) == (0, [0] * 7)
    else:
        assert M.plan(lib, M.desc(**dict(GOOD, **change))) == (0, [0] * 7)


@pytest.mark.parametrize("name", list(M.CASES))
def test_plan_of_the_gpu_cases(lib, name):
    """sixteen columns, sixteen frames a wave, 64 a key block; spans of whole blocks towards 512 workgroups; the
    partials of attn_fwd_kernel within its workspace; LDS: P [64][20], then the query [16][D + 4] or, if larger, the
    upper half of the frame slices' sums."""
    c = M.CASES[name]
    G, m, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    d = M.desc(G, m, T, D, Dv)
    ok, p = M.plan(lib, d)
    assert ok == 1 and p[:3] == [16, 16, 64]
    blocks = -(-T // 64)
    assert c["splits"] == min(max(1, -(-512 // G)), blocks) and p[3] == c["splits"]
    assert p[4] == 64 * -(-blocks // c["splits"])
    assert p[5] == (0 if c["splits"] == 1 else c["splits"] * G * m * (Dv + 2) * 4)
    assert p[5] <= lib.pdt_attn_workspace_bytes(d, 0, 0)
    assert p[6] == 4 * (64 * 20 + max(16 * (D + 4), 256 // (Dv // 4) // 2 * m * Dv)) and p[6] < 64 * 1024


def test_entry_point_refuses_before_any_launch(lib):
    from pydrobert_amd import _cabi

    ARG, UNSUP = _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    scale = ctypes.c_double(1.0)
    sp = ctypes.addressof(scale)
    good = M.desc(**GOOD)
    call = lambda d, p=16, s=sp, w=1 << 30, q=None: lib.pdt_attn_dot_mfma_dec(  # noqa: E731
        d, p if q is None else q, p, p, 0, s, p, p, p, w, 0)
    assert call(good, s=None) == ARG  # no scale
    assert call(M.desc(**dict(GOOD, M=17))) == UNSUP
    assert call(M.desc(**dict(GOOD, fs=2))) == UNSUP
    assert call(good, p=0) == ARG  # null pointers
    assert call(good, q=20) == ARG  # a query four bytes off
    need = M.plan(lib, good)[1][5]
    assert need > 0 and call(good, w=need - 1) == ARG
