"""CPU: the entry points through which the attention kernels read float16 / bfloat16 operands as they are
(include/pdt_amd.h: pdt_attn_*_elem) exist in the header, the ctypes table and the library, plan as the float32
entry points do and validate everything before anything touches a GPU; the host route admits half ROCm tensors
of one dtype under the float32 LDS rule; the operators' fake kernels give lse in float32 for half operands; and
the allowances of the GPU no-copy test are below the formula's intermediates."""
import ctypes
import os
import re

import pytest
import torch

import _attn_ref as R
import _half_attn as ha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdt_amd.h")


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
    for sibling in ha.ENTRIES:
        name = sibling + "_elem"
        assert name in _cabi.SIGNATURES, name + " is not in the ctypes table"
        assert hasattr(lib, name), "libpdt_amd.so does not export " + name
        assert _cabi.SIGNATURES[name] == _cabi.SIGNATURES[sibling], name  # (`int elem` in the place of `int dtype`)
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, name + " is not declared in pdt_amd.h"
        assert re.match(r"\s*const int64_t \*desc,\s*int elem,", m.group(1)), name
        m = re.search(r"\b" + sibling + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert re.match(r"\s*const int64_t \*desc,\s*int dtype,", m.group(1)), sibling  # (it keeps its declaration)
    assert _cabi.ABI_VERSION == 14 and lib.pdt_amd_abi_version() == 14


@pytest.mark.parametrize("name", ha.F32_CASES)
def test_half_types_plan_as_float32(lib, name):
    """pdt_attn_workspace_bytes_elem for elem 0, 2 and 3 is pdt_attn_workspace_bytes with dtype 0, and both are
    the restatement's at 4 bytes an element, for every float32 case and kind: the half types take the float32
    plan (splits, the rows kernel, frame chunks)."""
    c = R.CASES[name]
    G, M = R.plan_shape(c)
    for kind, code in R.KINDS.items():
        D = 0 if kind.startswith("pool") else max(1, c["D"])
        p = R.plan_of(G, M, c["T"], D, c["Dv"], 4, kind)
        d = ha.desc(R_=G * M, G=G, M=M, T=c["T"], D=D, Dv=c["Dv"], sizes=(G, M))
        f32 = lib.pdt_attn_workspace_bytes(d, 0, code)
        assert f32 == p["ws_bytes"], (kind, p)
        for e in (0, 2, 3):
            assert lib.pdt_attn_workspace_bytes_elem(d, e, code) == f32, (kind, e)


def _calls(lib, sp):
    """name -> f(desc, elem, p, ws_bytes): each launching _elem entry point with every pointer ``p`` (0: null; 1: a
    made-up address, never dereferenced: every call here returns before a launch)."""
    return {
        "pdt_attn_dot_elem": lambda d, e, p, w=0: lib.pdt_attn_dot_elem(d, e, p, p, p, 0, sp, p, p, p, w, 0),
        "pdt_attn_dot_backward_elem": lambda d, e, p, w=0: lib.pdt_attn_dot_backward_elem(
            d, e, p, p, p, 0, sp, p, p, p, p, p, p, p, w, 0),
        "pdt_attn_pool_elem": lambda d, e, p, w=0: lib.pdt_attn_pool_elem(d, e, p, p, 0, p, p, p, w, 0),
        "pdt_attn_pool_backward_elem": lambda d, e, p, w=0: lib.pdt_attn_pool_backward_elem(
            d, e, p, p, 0, p, p, p, p, p, p, w, 0),
    }  # fmt: skip


def test_elem_codes_arguments_and_workspace_without_gpu(lib):
    """elem 1 (float64) is PDT_E_UNSUPPORTED and any other code but 0, 2, 3 PDT_E_ARG, -1 from the workspace
    query for both, before the pointers are looked at; null pointers with rows to do, a missing scale and a
    workspace one byte short are PDT_E_ARG; no rows is PDT_OK.  The entry points without the suffix keep
    refusing codes 2 and 3."""
    from pydrobert_amd import _cabi

    OK, ARG, UNSUP = _cabi.PDT_OK, _cabi.PDT_E_ARG, _cabi.PDT_E_UNSUPPORTED
    scale = ctypes.c_double(1.0)
    calls = _calls(lib, ctypes.addressof(scale))
    descs = {n: ha.desc(D=0 if "pool" in n else 4) for n in calls}
    empty = {n: ha.desc(R_=0, G=0, M=3, D=0 if "pool" in n else 4, sizes=(0, 3)) for n in calls}
    for kind in range(4):
        d = ha.desc(D=0 if kind >= 2 else 4)
        assert lib.pdt_attn_workspace_bytes_elem(d, 1, kind) == -1
        assert lib.pdt_attn_workspace_bytes_elem(d, 5, kind) == -1
        assert lib.pdt_attn_workspace_bytes_elem(d, -1, kind) == -1
        assert lib.pdt_attn_workspace_bytes_elem(None, 2, kind) == -1
        assert lib.pdt_attn_workspace_bytes_elem(d, 2, kind) >= 0
        for e in (2, 3):
            assert lib.pdt_attn_workspace_bytes(d, e, kind) == -1
    assert lib.pdt_attn_workspace_bytes_elem(ha.desc(), 2, 4) == -1  # bad kind
    assert lib.pdt_attn_workspace_bytes_elem(ha.desc(), 3, 1) == lib.pdt_attn_workspace_bytes(ha.desc(), 0, 1) >= 6 * 4
    for name, f in calls.items():
        for p in (0, 1):
            assert f(descs[name], 1, p) == UNSUP, name
            assert f(descs[name], 5, p) == ARG, name
            assert f(empty[name], 1, p) == UNSUP, name  # (the code comes before the descriptor)
        for e in (0, 2, 3):
            assert f(descs[name], e, 0) == ARG, (name, e)  # null pointers with rows to do
            assert f(empty[name], e, 0) == OK, (name, e)  # R = 0: nothing to do
            assert f(ha.desc(T=0, D=0 if "pool" in name else 4), e, 1, 1 << 30) == ARG, (name, e)  # T = 0 with rows
    for e in (2, 3):
        assert lib.pdt_attn_dot_elem(ha.desc(), e, 1, 1, 1, 0, None, 1, 1, 1, 1 << 30, 0) == ARG  # no scale
        assert lib.pdt_attn_dot(ha.desc(), e, 1, 1, 1, 0, ctypes.addressof(scale), 1, 1, 1, 1 << 30, 0) == ARG
        assert lib.pdt_attn_pool(ha.desc(D=0), e, 1, 1, 0, 1, 1, 1, 1 << 30, 0) == ARG
    # a workspace one byte short: the forward's split partials, the backward's delta and dQ partials
    big = ha.desc(R_=2, G=2, M=1, T=4096, sizes=(2, 1))
    pbig = ha.desc(R_=2, G=2, M=1, T=4096, D=0, sizes=(2, 1))
    for e in (0, 2, 3):
        for name, d, kind in (("pdt_attn_dot_elem", big, 0), ("pdt_attn_dot_backward_elem", big, 1),
                              ("pdt_attn_pool_elem", pbig, 2), ("pdt_attn_pool_backward_elem", pbig, 3)):  # fmt: skip
            need = lib.pdt_attn_workspace_bytes_elem(d, e, kind)
            assert need > 0
            assert calls[name](d, e, 1, need - 1) == ARG, (name, e)


class Fake:  # (what _hip_route reads of a ROCm tensor, without a GPU)
    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

    def dim(self):
        return len(self.shape)


@pytest.mark.parametrize("dtname", list(ha.DTYPES))
def test_route_admits_half_under_the_float32_lds_rule(dtname):
    from pydrobert_amd import _attn

    dt = ha.DTYPES[dtname]
    v = Fake((5, 3, 2), dt)
    assert _attn._hip_route([5, 3], v, None, 0, [Fake((5, 3, 4), dt), v], 14336) is True
    assert _attn._hip_route([5, 3], v, None, 0, [Fake((5, 3, 4), dt), v], 14337) is False
    # operands of mixed dtypes stay on the formula
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    for odt in (torch.float32, other):
        assert _attn._hip_route([5, 3], v, None, 0, [Fake((5, 3, 4), odt), v], 8) is False
        assert _attn._hip_route([5, 3], v, None, 0, [Fake((5, 3, 4), dt), Fake((5, 3, 2), odt)], 8) is False
    with pytest.raises(TypeError):
        _attn._dtype_code(torch.zeros(1, dtype=dt), torch.zeros(1), half=True)
    with pytest.raises(TypeError):  # (the concat score kernels take no half tensors)
        _attn._dtype_code(torch.zeros(1, dtype=dt))
    assert _attn._dtype_code(torch.zeros(1, dtype=dt), torch.zeros(1, dtype=dt), half=True) == ha.ELEM[dtname]


def test_fake_kernels_give_float32_lse_for_half_operands():
    import pydrobert_amd.modules  # noqa: F401

    ops = torch.ops.pydrobert_amd
    for dt, lse_dt in ((torch.bfloat16, torch.float32), (torch.float16, torch.float32),
                       (torch.float32, torch.float32), (torch.float64, torch.float64)):  # fmt: skip
        q = torch.empty(3, 4, 5, device="meta", dtype=dt)
        k = torch.empty(7, 3, 1, 5, device="meta", dtype=dt)
        v = torch.empty(7, 3, 1, 6, device="meta", dtype=dt)
        e = torch.empty(7, 3, 4, device="meta", dtype=dt)
        mask = torch.empty(7, 3, 1, device="meta", dtype=torch.bool)
        out, lse = ops.dot_attention(q, k, v, mask, 0, 0.5)
        assert (out.shape, out.dtype, lse.shape, lse.dtype) == ((3, 4, 6), dt, (2, 12), lse_dt)
        g = torch.empty(3, 4, 6, device="meta", dtype=dt)
        grads = ops.dot_attention_backward(g, q, k, v, mask, out, lse, 0, 0.5)
        assert [(x.shape, x.dtype) for x in grads] == [(t.shape, dt) for t in (q, k, v)]
        out, lse = ops.attention_pool(e, v, mask, 0)
        assert (out.shape, out.dtype, lse.shape, lse.dtype) == ((3, 4, 6), dt, (2, 12), lse_dt)
        grads = ops.attention_pool_backward(g, e, v, mask, out, lse, 0)
        assert [(x.shape, x.dtype) for x in grads] == [(t.shape, dt) for t in (e, v)]


def test_sum_to_reduces_half_gradients_in_float32_and_only_when_shapes_differ():
    """The host reduction behind the kernel (an input broadcast beyond the group): a half gradient is summed in
    float32 and rounded once; a gradient of the input's shape is returned as it is."""
    from pydrobert_amd import _attn

    torch.manual_seed(3)
    for dt in ha.DTYPES.values():
        g = (torch.randn(300, 2, 1, 5) * 8).to(dt)
        assert _attn._sum_to(g, g.shape) is g
        got = _attn._sum_to(g, (1, 2, 1, 5))
        assert got.dtype == dt and ha.same_bits(got, g.float().sum(0, keepdim=True).to(dt))
    g = torch.randn(4, 2, 3)
    assert torch.equal(_attn._sum_to(g, (1, 2, 3)), g.sum_to_size(1, 2, 3))


def test_no_copy_allowances_rule_out_the_formula():
    """The GPU no-copy test is not vacuous: its allowances plus the 1 MiB of slack are several times below the
    smallest of the formula's intermediates at that shape."""
    fwd, bwd, formula = ha.nocopy_bytes(2)
    assert ha.NOCOPY["T"] * ha.NOCOPY["N"] * ha.NOCOPY["D"] * 2 == 16 * ha.MIB  # the key
    assert 4 * (fwd + ha.MIB) < formula and 2 * (bwd + ha.MIB) < formula


def test_forward_bound_is_the_suite_bound_plus_half_an_ulp():
    ref = torch.tensor([0.0, 1.0, 1.5, 1000.0, 3e-6], dtype=torch.float64)
    b = 2e-5 + 2e-5 * ref
    for dt, half_ulps in ((torch.bfloat16, [2.0 ** -24, 2.0 ** -8, 2.0 ** -8, 2.0 ** 1, 2.0 ** -24]),
                          (torch.float16, [2.0 ** -25, 2.0 ** -11, 2.0 ** -11, 2.0 ** -2, 2.0 ** -25])):  # fmt: skip
        half = torch.tensor(half_ulps, dtype=torch.float64)
        assert torch.equal(ha.ulp(ref + b, dt) / 2, half), dt
        assert torch.equal(ha.forward_bound(ref, dt), b + half), dt
