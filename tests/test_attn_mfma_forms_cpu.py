"""CPU: the forms of tests/_attn_mfma_forms.py, checked without a GPU.  The three plan entry points
(pdt_attn_dot_mfma_plan, pdt_attn_dot_mfma_backward_plan, pdt_attn_dot_mfma_f32_plan) accept every form's descriptor
as ``_attn._dot_plan`` builds it from the CPU tensors and report what the formulas of the kernels' headers give; each
form has the property it is named for, asserted from its inputs and descriptor alone; the float64 reference has NaN
exactly where intended."""
import ctypes

import pytest
import torch

from _attn_mfma import ELEM
import _attn_mfma_forms as F
from test_attn_mfma_cpu import lib  # noqa: F401 (the library fixture, built on demand)

DTNAMES = list(F.ALL_DTYPES)


def dot_plan(name, dtname, pad=0):
    from pydrobert_amd import _attn

    x = F.inputs(name, dtname, pad)
    plan, ops = _attn._dot_plan(x["q"], x["k"], x["v"], x["mask"], x["dim"])
    return x, plan, ops


def slot(plan, s):
    """Row strides (in the kernel's row order), T stride and feature stride of a descriptor slot."""
    from pydrobert_amd import _attn as A

    d, base = plan.desc.tolist(), 7 + A._MAX_DIMS + s * (A._MAX_DIMS + 2)
    return d[base:base + d[0]], d[base + A._MAX_DIMS], d[base + A._MAX_DIMS + 1]


def plans(lib, plan, dtname):
    """(return code, numbers) of the forward plan of the dtype and, for a half dtype, of the backward plan."""
    fwd, bwd = (ctypes.c_int64 * 7)(), (ctypes.c_int64 * 5)()
    if dtname == "float32":
        return (lib.pdt_attn_dot_mfma_f32_plan(plan.desc.data_ptr(), ctypes.addressof(fwd)), list(fwd)), None
    elem = ELEM[dtname]
    return ((lib.pdt_attn_dot_mfma_plan(plan.desc.data_ptr(), elem, ctypes.addressof(fwd)), list(fwd)),
            (lib.pdt_attn_dot_mfma_backward_plan(plan.desc.data_ptr(), elem, ctypes.addressof(bwd)), list(bwd)))  # fmt: skip


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", list(F.FORMS))
def test_plans_accept_the_form_and_follow_the_headers_formulas(lib, name, dtname):
    c, want = F.FORMS[name], F.plan_formulas(F.FORMS[name])
    _, plan, ops = dot_plan(name, dtname)
    d = plan.desc.tolist()
    assert d[1:7] == [c["G"] * c["M"], c["G"], c["M"], c["T"], c["D"], c["Dv"]]
    assert all(t.data_ptr() % 16 == 0 for t in ops[:3]), "query, key and value are 16-byte aligned"
    (ok, p), bwd = plans(lib, plan, dtname)
    assert ok == 1 and p[:3] == [64, 16, 64]
    assert want["splits"] == c["splits"] and p[3:6] == [want["splits"], want["span"], want["ws"]]
    assert p[6] == (want["lds_f32"] if dtname == "float32" else want["lds_half"])
    if bwd is not None:
        assert bwd == (1, [64, 64, want["delta_ws"], want["lds_q"], want["lds_kv"]])


def test_three_spans_plan_in_figures(lib):
    """9 key blocks, 3 spans of 192 frames, the last 136 frames long, a workspace of 3 x 64 x (48 + 2) floats."""
    for dtname in DTNAMES:
        (ok, p), _ = plans(lib, dot_plan("three-spans", dtname)[1], dtname)
        assert ok == 1 and p[3:6] == [3, 192, 3 * 64 * (48 + 2) * 4]
        assert p[4] == F.SPAN and F.FORMS["three-spans"]["T"] - 2 * p[4] == 136


@pytest.mark.parametrize("dtname", DTNAMES)
def test_head_dim_forms_leave_a_half_empty_chunk(dtname):
    """From the descriptors: 48, 80 and 112, whose last chunk of 32 columns is half empty in the half kernels, each
    stand for D and for Dv; 128 / 128 is there; 112 / 48 leaves the second 64-float half of D partly filled with Dv's
    absent."""
    seen = []
    for name in ("d48-dv112", "d112-dv48", "d80-dv80", "d128-dv128"):
        c, (x, plan, _) = F.FORMS[name], dot_plan(name, dtname)
        seen.append(tuple(plan.desc.tolist()[5:7]))
        assert plan.order == ([1, 2] if c["G"] > 1 else [2]) and list(x["q"].shape) == [c["G"], c["M"], c["D"]]
        assert list(x["k"].shape) == [c["T"], c["G"], 1, c["D"]] and list(x["v"].shape) == [c["T"], c["G"], 1, c["Dv"]]
    every = set(range(32, 129, 16))  # the gate's head dims
    assert {d for d, _ in seen if d % 32} == {dv for _, dv in seen if dv % 32} == {d for d in every if d % 32}
    assert (128, 128) in seen and any(d > 64 and d % 64 and dv <= 64 for d, dv in seen)
    x = F.inputs("d128-dv128", dtname)
    t, m = torch.arange(72).view(-1, 1, 1), torch.arange(80).view(1, 1, -1)
    assert torch.equal(x["mask"], (t <= m).expand(72, 1, 80))
    assert F.FORMS["d48-dv112"]["M"] % 64 and F.FORMS["d48-dv112"]["T"] % 64 and F.FORMS["d112-dv48"]["T"] > 128


@pytest.mark.parametrize("dtname", DTNAMES)
def test_nan_gaps_descriptor(dtname):
    """The shape and numbers' recipe of d48-dv112, every row sixteen elements wider: the sixteen elements behind a
    row, which a load of the empty half of its last chunk of 32 would fetch, are NaN, and nothing else is."""
    from pydrobert_amd import _attn as A

    x, plan, _ = dot_plan("nan-gaps", dtname)
    c = F.FORMS["nan-gaps"]
    assert [c[n] for n in "GMTD"] + [c["Dv"]] == [F.FORMS["d48-dv112"][n] for n in "GMTD"] + [112] and F.GAP == 16
    assert slot(plan, A._SQ) == ([80 * 64, 64], 0, 1) and slot(plan, A._SK) == ([64, 0], 2 * 64, 1)
    assert slot(plan, A._SV) == ([128, 0], 2 * 128, 1) and slot(plan, A._SO)[0] == [80 * 112, 112]
    for t, w in zip((x["q"], x["k"], x["v"]), x["wide"]):
        assert t.data_ptr() == w.data_ptr() and w.is_contiguous() and w.shape[-1] == t.shape[-1] + 16
        assert torch.isfinite(t).all() and torch.isnan(w[..., t.shape[-1]:]).all()
        flat, width = w.reshape(-1), t.shape[-1]
        assert torch.isnan(flat[width:width + 16]).all() and torch.isfinite(flat[width + 16:2 * width + 16]).all()


@pytest.mark.parametrize("dtname", DTNAMES)
def test_three_spans_mask(dtname):
    mask = F.inputs("three-spans", dtname)["mask"]
    assert list(mask.shape) == [520, 1, 64]
    spans = torch.stack([mask[i * F.SPAN:(i + 1) * F.SPAN].any(0)[0] for i in range(3)])  # (span, row)
    assert spans.any(0).all(), "no dead row"
    assert not spans[1].any(), "nobody attends the middle span"
    assert spans[0, :16].all() and not spans[1:, :16].any(), "rows 0..15 attend only span 0"
    assert spans[2, 16:32].all() and not spans[:2, 16:32].any(), "rows 16..31 attend only span 2"
    assert spans[0, 32:].all() and spans[2, 32:].all(), "the other rows attend both outer spans"
    assert mask[2 * F.SPAN + 128:].any(), "the tail beyond the last span's two whole key blocks is attended"


@pytest.mark.parametrize("dtname", DTNAMES)
def test_one_frame(dtname):
    x, plan, _ = dot_plan("one-frame", dtname)
    assert plan.T == 1 and x["mask"] is None and plan.M == 64 and plan.G == 2


@pytest.mark.parametrize("dtname", DTNAMES)
def test_batch_first_descriptor(dtname):
    from pydrobert_amd import _attn as A

    x, plan, _ = dot_plan("batch-first", dtname)
    assert x["dim"] == 1 and list(x["q"].shape) == [2, 66, 2, 32]
    assert list(x["k"].shape) == [2, 70, 1, 2, 32] and list(x["v"].shape) == [2, 70, 1, 2, 48]
    d = plan.desc.tolist()
    assert d[0] == 3 and plan.order == [0, 3, 2] and d[7:10] == [2, 2, 66] and plan.out_shape == [2, 66, 2, 48]
    assert slot(plan, A._SO)[0] == [6336, 48, 96], "out's rows are not in the kernel's order"
    assert list(x["mask"].shape) == [2, 70, 1, 1] and x["mask"].tolist() == [
        [[[t < n]] for t in range(70)] for n in F.LENGTHS]  # fmt: skip
    assert slot(plan, A._SM) == ([70, 0, 0], 1, 0), "the mask has stride 0 along heads and rows"
    for n, length in enumerate(F.LENGTHS):  # NaN in the padded frames of what the kernels read, and only there
        for t, ref in ((x["k"], x["k_ref"]), (x["v"], x["v_ref"])):
            assert torch.isnan(t[n, length:]).all() and torch.isfinite(t[n, :length]).all()
            assert torch.isfinite(ref).all() and torch.equal(t[n, :length], ref[n, :length])


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", ["shared-causal", "key-nan", "band-d48", "key-nan-d48"])
def test_shared_mask_descriptor(name, dtname):
    """The causal and the band mask are passed at (T, 1, M); a key-nan form is its base with one NaN key row, in a
    frame that rows of the first 64-row block both attend and mask.  The band form has half-empty chunks for D and
    Dv, and a row that attends the frame before the NaN one while it masks the NaN one: a key fragment read from LDS
    beyond D (frame 36's would hold frame 37's first columns) shows in that row."""
    from pydrobert_amd import _attn as A

    x, plan, _ = dot_plan(name, dtname)
    c = F.FORMS[name]
    base = c.get("base", name)
    assert list(x["mask"].shape) == [70, 1, 70] and plan.order == [1, 2] and (plan.G, plan.M) == (c["G"], 70)
    assert slot(plan, A._SM) == ([0, 1], 70, 0), "the mask has stride 0 along the groups"
    t, m = torch.arange(70).view(-1, 1, 1), torch.arange(70).view(1, 1, -1)
    assert torch.equal(x["mask"], t <= m if base == "shared-causal" else (t - m).abs() <= F.BAND)
    if base == "band-d48":
        assert plan.desc.tolist()[5:7] == [48, 80] and F.FORMS["key-nan-d48"]["D"] % 32 == 16
    bad = torch.isnan(x["k"])
    if "base" in c:
        f, g = F.NAN_KEY
        attend = x["mask"][f, 0]
        assert bad[f, g].all() and int(bad.sum()) == c["D"] and torch.isfinite(x["v"]).all()
        assert attend[:64].any() and not attend[:64].all() and f + 1 < 64, "both kinds of row in the first row block"
        assert (x["mask"][f - 1, 0] & ~attend).any(), "a row attends the frame before and masks this one"
        clean = F.inputs(base, dtname)
        assert torch.equal(x["q"], clean["q"]) and torch.equal(x["v"], clean["v"])
        assert torch.equal(x["k"].nan_to_num(0.0), clean["k"].masked_fill(bad, 0.0))
    else:
        assert not bad.any()


@pytest.mark.parametrize("dtname", DTNAMES)
def test_fused_qkv_descriptor(dtname):
    from pydrobert_amd import _attn as A

    x, plan, _ = dot_plan("fused-qkv", dtname)
    fused, esz = x["fused"], x["fused"].element_size()
    assert list(fused.shape) == [70, 2, 384] and fused.is_contiguous()
    assert list(x["q"].shape) == [70, 2, 4, 32] and list(x["k"].shape) == [70, 1, 2, 4, 32] == list(x["v"].shape)
    assert [t.data_ptr() - fused.data_ptr() for t in (x["q"], x["k"], x["v"])] == [0, 128 * esz, 256 * esz]
    assert plan.order == [2, 3, 1] and plan.desc.tolist()[7:10] == [2, 4, 70] and (plan.G, plan.M) == (8, 70)
    assert slot(plan, A._SK) == ([384, 32, 0], 768, 1) and slot(plan, A._SV) == ([384, 32, 0], 768, 1)
    assert slot(plan, A._SQ) == ([384, 32, 768], 0, 1) and slot(plan, A._SO)[0] == [128, 32, 256]
    assert list(x["mask"].shape) == [70, 70, 1, 1] and slot(plan, A._SM) == ([0, 0, 1], 70, 0)
    assert torch.equal(x["mask"][:, :, 0, 0], torch.ones(70, 70).triu().bool())  # key frame <= query frame


@pytest.mark.parametrize("dtname", DTNAMES)
def test_fused_qkv_four_elements_longer(lib, dtname):
    """The stride-level gate: with the fused axis 388 long every base is still 16-byte aligned, but the batch stride
    of query, key and value is 388 = 4 (mod 8) (the T stride, 776, is a multiple of 8): the half plans refuse, the
    float32 plan, whose 16 bytes are four elements, does not."""
    from pydrobert_amd import _attn as A

    x, plan, ops = dot_plan("fused-qkv", dtname, 4)
    assert all(t.data_ptr() % 16 == 0 for t in ops[:3])
    assert slot(plan, A._SK) == ([388, 32, 0], 776, 1) and 388 % 8 == 4 and 388 % 4 == 0
    assert torch.equal(x["q"], F.inputs("fused-qkv", dtname)["q"]) and torch.equal(x["v"], F.inputs("fused-qkv", dtname)["v"])
    fwd, bwd = plans(lib, plan, dtname)
    if dtname == "float32":
        assert fwd[0] == 1
    else:
        assert fwd == (0, [0] * 7) and bwd == (0, [0] * 5)


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", list(F.FORMS))
def test_reference_has_nan_exactly_where_intended(name, dtname):
    ref = F.reference(name, dtname)
    bad = torch.isnan(ref["out"])
    if "base" not in F.FORMS[name]:
        assert not bad.any() and torch.isfinite(ref["out"]).all()
        assert torch.isfinite(ref["m"]).all() and torch.isfinite(ref["logsum"]).all()
        return
    f, g = F.NAN_KEY
    want = torch.zeros(F.FORMS[name]["G"], 70, dtype=torch.bool)
    want[g] = F.inputs(name, dtname)["mask"][f, 0]  # the rows that attend the frame: 37..69 causal, 29..45 band
    assert int(want.sum()) == (33 if name == "key-nan" else 17)
    assert torch.equal(bad.all(-1), want) and torch.equal(bad.any(-1), want)
    zeroed, clean = F.reference(name, dtname, True), F.reference(F.FORMS[name]["base"], dtname)
    assert torch.isfinite(zeroed["out"]).all()
    assert torch.equal(zeroed["out"][~want], ref["out"][~want]) and torch.equal(zeroed["out"][~want], clean["out"][~want])


@pytest.mark.parametrize("dtname", DTNAMES)
def test_kernel_row_order_of_the_layout_forms(dtname):
    """``to_kernel_order`` against the descriptor: the out offset of kernel row r, by the sizes and strides of the
    descriptor's out slot, is where the r-th entry of the reordered row index came from."""
    from pydrobert_amd import _attn as A

    for name in ("batch-first", "fused-qkv", "d48-dv112"):
        x, plan, _ = dot_plan(name, dtname)
        sizes, (st, _, _) = plan.desc.tolist()[7:7 + len(plan.order)], slot(plan, A._SO)
        index = torch.arange(plan.R).view(plan.out_shape[:-1]) * plan.out_shape[-1]  # a row's offset into out
        got = F.to_kernel_order(index, plan.S, plan.order, x["dim"]).tolist()
        for r in (0, 1, plan.M - 1, plan.M, plan.R // 2 + 3, plan.R - 1):
            rem, off = r, 0
            for size, stride in zip(reversed(sizes), reversed(st)):
                off, rem = off + (rem % size) * stride, rem // size
            assert got[r] == off, (name, r)
