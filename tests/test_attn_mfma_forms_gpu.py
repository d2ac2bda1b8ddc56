"""GPU: the forms of tests/_attn_mfma_forms.py through ``pydrobert_amd::dot_attention`` and autograd, on the half
forward (csrc/attn_mfma.hip), the half backward (attn_mfma_bwd.hip) and the float32 forward (attn_mfma_f32.hip),
against float64 on the exactly widened operands.  Every case asserts from the plan that the route is taken.  No bound
is new: ``out`` in half is held to ``_attn_mfma.out_bound``, in float32 to ``_attn_ref.SUITE`` or 8 x the float32
formula's own error where that is larger, ``lse`` to 2e-5 (1 + |ref|), a half gradient to 1e-4 + 4 x the error of
``_attn._softmax_pool`` in the same half dtype; exact zeros, equal bits and the all-NaN rows are asserted as such."""
import functools

import numpy as np
import pytest
import torch

import _attn_mfma_forms as F
import _attn_ref as R
from _attn_mfma import DTYPES, out_bound
from test_attn_mfma_gpu import DEV, grads

pytestmark = pytest.mark.gpu

HALF = list(DTYPES)
OUT_TOL = R.SUITE["float32"][0]
INT = {"float16": torch.int16, "bfloat16": torch.int16, "float32": torch.int32}


def routes(q, k, v, mask, dim):
    """Which matrix-core kernels a call with these device tensors takes: (half forward, half backward, float32
    forward), from the plans (the operator's grad_out is a fresh contiguous tensor: aligned as ``q`` is here)."""
    from pydrobert_amd import _attn

    plan, ops = _attn._dot_plan(q, k, v, mask, dim)
    dt = {torch.float32: 0, torch.float16: 2, torch.bfloat16: 3}[q.dtype]
    return (_attn._mfma_workspace_bytes(plan, dt, ops) >= 0, _attn._mfma_bwd_workspace_bytes(plan, dt, ops, ops[0]) >= 0,
            _attn._mfma_f32_workspace_bytes(plan, dt, ops) >= 0)  # fmt: skip


def device_inputs(name, dtname, pad=0):
    """(q, k, v, mask, dim, scale) on the device with the CPU tensors' strides, and the tensors they are views of
    (``_attn_mfma_forms.leaves``: themselves for most forms)."""
    x = F.inputs(name, dtname, pad)
    leaves = [t.to(DEV) for t in F.leaves(name, x)]
    q, k, v = F.split_of(name)(*leaves)
    for t, n in ((q, "q"), (k, "k"), (v, "v")):  # (the stride of a dim of size 1 is nobody's)
        assert t.data_ptr() % 16 == 0 and t.shape == x[n].shape
        assert all(a == b for a, b, size in zip(t.stride(), x[n].stride(), t.shape) if size > 1)
    return (q, k, v, None if x["mask"] is None else x["mask"].to(DEV), x["dim"], x["scale"]), leaves


def attend(args):
    return torch.ops.pydrobert_amd.dot_attention(*args)


@functools.lru_cache(maxsize=None)
def forward(name, dtname):
    import pydrobert_amd.modules  # noqa: F401

    args, _ = device_inputs(name, dtname)
    took = routes(*args[:5])
    assert took[2 if dtname == "float32" else 0], "the plan refuses " + name
    out, lse = attend(args)
    return out.cpu(), lse.cpu()


def check_forward(name, dtname, bound_of):
    """``out`` within ``bound_of(ref)`` and both ``lse`` rows within 2e-5 (1 + |ref|) of float64, ``lse`` in the
    kernel's row order; a key-nan form: the rows that attend the NaN key all NaN, the others as if the key were 0."""
    from pydrobert_amd import _attn

    x, ref = F.inputs(name, dtname), F.reference(name, dtname, "base" in F.FORMS[name])
    plan, _ = _attn._dot_plan(x["q"], x["k"], x["v"], x["mask"], x["dim"])
    out, lse = forward(name, dtname)
    assert out.dtype == F.ALL_DTYPES[dtname] and lse.dtype == torch.float32
    assert out.shape == ref["out"].shape and list(lse.shape) == [2, plan.R]
    lost = torch.isnan(F.reference(name, dtname)["out"]).any(-1)  # (rows that attend a NaN key)
    attending = int(x["mask"][F.NAN_KEY[0], 0].sum()) if "base" in F.FORMS[name] else 0  # (33 causal, 17 band)
    assert int(lost.sum()) == attending and (attending > 0) == ("base" in F.FORMS[name])
    assert torch.equal(torch.isnan(out).all(-1), lost) and torch.equal(torch.isfinite(out).all(-1), ~lost)
    err, bound = (out.double() - ref["out"]).abs()[~lost], bound_of(ref)[~lost]
    print(name, dtname, "largest error / bound", float((err / bound).max()), "formula's float32 error", ref.get("err32"))
    assert (err <= bound).all()
    live = ~F.to_kernel_order(lost, plan.S, plan.order, x["dim"])
    for got, key in ((lse[0], "m"), (lse[1], "logsum")):
        want = F.to_kernel_order(ref[key], plan.S, plan.order, x["dim"])
        e = (got.double() - want).abs()[live] / (2e-5 * (1 + want.abs()[live]))
        print(name, dtname, "lse", key, "largest error / bound", float(e.max()))
        assert (e <= 1).all()
    if name == "one-frame":  # one frame attended by everyone: p = 1, l = 1, the value row itself
        v = x["v"][0].expand(out.shape).contiguous()
        assert torch.equal(out.view(INT[dtname]), v.view(INT[dtname])) and (lse[1] == 0).all()


def half_bound(name, dtname):
    return lambda ref: out_bound(ref["out"], ref["A"], ref["vmax"], F.FORMS[name]["T"], dtname)


def float32_bound(ref):
    return (OUT_TOL + OUT_TOL * ref["out"].abs()).clamp_min(8 * ref["err32"])


@pytest.mark.parametrize("dtname", HALF)
@pytest.mark.parametrize("name", list(F.FORMS))
def test_half_forward_against_float64(name, dtname):
    check_forward(name, dtname, half_bound(name, dtname))


@pytest.mark.parametrize("name", list(F.FORMS))
def test_float32_forward_against_float64(name):
    check_forward(name, "float32", float32_bound)


@pytest.mark.parametrize("dtname", list(F.ALL_DTYPES))
def test_two_forward_runs_of_three_spans_give_equal_bits(dtname):
    args, _ = device_inputs("three-spans", dtname)
    assert routes(*args[:5])[2 if dtname == "float32" else 0]
    a, b = attend(args), attend(args)
    assert torch.equal(a[0].view(INT[dtname]), b[0].view(INT[dtname])) and torch.equal(a[1], b[1])
    first = forward("three-spans", dtname)
    assert torch.equal(a[0].cpu().view(INT[dtname]), first[0].view(INT[dtname])) and torch.equal(a[1].cpu(), first[1])


# ----------------------------------------------------------------------------------------------------------
# the half backward


def gradients(fn, leaves, gout):
    """``grads`` of tests/test_attn_mfma_gpu.py, for fused-qkv's one leaf too."""
    if len(leaves) == 3:
        return grads(fn, *leaves, gout)
    (leaf,) = (t.detach().clone().requires_grad_(True) for t in leaves)
    return torch.autograd.grad((fn(leaf).double() * gout.to(leaf.device)).sum(), [leaf])


@functools.lru_cache(maxsize=None)
def backward(name, dtname):
    """The operator's gradients of a form with respect to its leaves, grad_out, and the route assertion."""
    (q, k, v, mask, dim, scale), leaves = device_inputs(name, dtname)
    assert routes(q, k, v, mask, dim)[:2] == (True, True), "the plan refuses " + name
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=F.reference(name, dtname)["out"].shape))
    split = F.split_of(name)  # (views of the leaves: fused-qkv's and nan-gaps' strides reach the backward operator)
    got = gradients(lambda *t: attend(split(*t) + (mask, dim, scale))[0], leaves, gout)
    return got, gout


@pytest.mark.parametrize("dtname", HALF)
@pytest.mark.parametrize("name", F.BACKWARD_FORMS)
def test_half_gradients_against_float64(name, dtname):
    from pydrobert_amd import _attn

    x = F.inputs(name, dtname)
    got, gout = backward(name, dtname)
    mask, dim, scale = x["mask"], x["dim"], x["scale"]
    leaves, split = F.leaves(name, x, ref=True), F.split_of(name)
    want = gradients(lambda *t: R.attend_ref(*split(*t), mask, dim, scale), [t.double() for t in leaves], gout)
    dmask = None if mask is None else mask.to(DEV)

    def formula(*t):
        a, b, c = split(*t)
        return _attn._softmax_pool((a.unsqueeze(dim) * b).sum(-1) * scale, c, dmask, dim)

    same = gradients(formula, [t.to(DEV) for t in leaves], gout)
    for n, g, w, f, leaf in zip(("fused",) if len(leaves) == 1 else "qkv", got, want, same, leaves):
        e_ref = float((f.cpu().double() - w).abs().max())
        err = float((g.cpu().double() - w).abs().max())
        print(name, dtname, "d" + n, "error", err, "formula's", e_ref, "error / bound", err / (1e-4 + 4 * e_ref))
        assert g.dtype == DTYPES[dtname] and g.shape == leaf.shape and torch.isfinite(g).all()
        assert err <= 1e-4 + 4 * e_ref
        if name == "nan-gaps":
            assert (g[..., -F.GAP:] == 0).all(), "nothing of a gap reaches a gradient"


@pytest.mark.parametrize("dtname", HALF)
def test_exact_zeros_of_frames_nobody_attends(dtname):
    (gq, gk, gv), _ = backward("batch-first", dtname)  # NaN planted in the padded keys and values
    assert all(torch.isfinite(g).all() for g in (gq, gk, gv))
    for n, length in enumerate(F.LENGTHS):
        assert (gk[n, length:] == 0).all() and (gv[n, length:] == 0).all()
        assert (gk[n, :length] != 0).any() and (gv[n, :length] != 0).any()
    (gq, gk, gv), _ = backward("three-spans", dtname)
    mid = slice(F.SPAN, 2 * F.SPAN)
    assert (gk[mid] == 0).all() and (gv[mid] == 0).all()
    assert (gk[:F.SPAN] != 0).any() and (gk[2 * F.SPAN:] != 0).any() and (gq != 0).any()


@pytest.mark.parametrize("dtname", HALF)
def test_two_backward_runs_of_d48_dv112_give_equal_bits(dtname):
    (q, k, v, mask, dim, scale), _ = device_inputs("d48-dv112", dtname)
    got, gout = backward("d48-dv112", dtname)
    again = gradients(lambda *t: attend(t + (mask, dim, scale))[0], [q, k, v], gout)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(got, again))


# ----------------------------------------------------------------------------------------------------------
# neighbours in LDS: band-d48 with one NaN planted, through the backward operator itself


@functools.lru_cache(maxsize=None)
def band_pass(dtname):
    """band-d48's device arguments, a finite grad_out, the forward's out and lse and the backward operator's three
    gradients on them: what a planted NaN must leave untouched wherever the planted row or frame is masked."""
    args, _ = device_inputs("band-d48", dtname)
    assert routes(*args[:5])[:2] == (True, True)
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(2, 70, 80))).to(DEV, args[0].dtype)
    out, lse = attend(args)
    return args, gout, out, lse, bwd_op(gout, args, out, lse)


def bwd_op(gout, args, out, lse):
    q, k, v, mask, dim, scale = args
    return torch.ops.pydrobert_amd.dot_attention_backward(gout, q, k, v, mask, out, lse, dim, scale)


@pytest.mark.parametrize("plant", ["key", "value", "query", "grad_out"])
@pytest.mark.parametrize("dtname", HALF)
def test_nan_next_door_in_lds_stays_next_door(dtname, plant):
    """The tiles in LDS are [row][width + 8]: sixteen columns beyond a half-empty chunk's eight valid ones are the
    padding and the NEXT row's first eight columns.  A NaN in those eight, in a frame (key, value) or row (query,
    grad_out) that its predecessor's partners mask, must not reach the predecessor: the gradients that do not depend
    on the planted row or frame keep the bits of the run without the NaN (held to float64 by
    test_half_gradients_against_float64[band-d48]), and those that do are NaN, so the plant was seen.  The forward's
    out and lse are those of the clean run, so only the backward kernels see the NaN.  Group 1; frame / row 38."""
    (q, k, v, mask, dim, scale), gout, out, lse, clean = band_pass(dtname)
    g, n, bits = 1, 38, lambda t: t.view(torch.int16)  # noqa: E731
    near = (torch.arange(70) - n).abs() <= F.BAND  # rows that attend frame n = frames that row n attends
    assert torch.equal(near, mask[n, 0].cpu()) and torch.equal(near, mask[:, 0, n].cpu())
    assert near[n - 1] and not near[n - 1 - F.BAND], "the predecessor has a partner that masks the planted one"
    q, k, v, gout = q.clone(), k.clone(), v.clone(), gout.clone()
    {"key": k[n, g, 0], "value": v[n, g, 0], "query": q[g, n], "grad_out": gout[g, n]}[plant][:8] = float("nan")
    gq, gk, gv = bwd_op(gout, (q, k, v, mask, dim, scale), out, lse)
    far = ~near.to(DEV)
    if plant in ("key", "value"):  # grad_query of the rows that mask frame n; a NaN key reaches columns 0..7 as 0 x NaN
        cols = slice(8, None) if plant == "key" else slice(None)
        assert torch.equal(bits(gq[g, far][:, cols]), bits(clean[0][g, far][:, cols]))
        assert torch.isnan(gq[g, near.to(DEV)]).all(-1).all(), "the rows that attend the frame saw the NaN"
        assert torch.equal(bits(gq[1 - g]), bits(clean[0][1 - g]))
    else:  # grad_key and grad_value of the frames that row n masks; 0 x NaN in the columns the plant is in
        kc, vc = (slice(8, None), slice(None)) if plant == "query" else (slice(None), slice(8, None))
        assert torch.equal(bits(gk[far, g, 0][:, kc]), bits(clean[1][far, g, 0][:, kc]))
        assert torch.equal(bits(gv[far, g, 0][:, vc]), bits(clean[2][far, g, 0][:, vc]))
        assert torch.isnan(gk[near.to(DEV), g, 0]).all(-1).all(), "the frames the row attends saw the NaN"
        assert torch.equal(bits(gk[:, 1 - g]), bits(clean[1][:, 1 - g]))
        assert torch.equal(bits(gv[:, 1 - g]), bits(clean[2][:, 1 - g]))


# ----------------------------------------------------------------------------------------------------------
# the gate at stride level: fused-qkv with the fused axis four elements longer


@pytest.mark.parametrize("dtname", HALF)
def test_half_stride_off_the_gate_takes_the_tile_kernels_to_the_bit(dtname):
    """The batch stride of query, key and value is 388 = 4 (mod 8) with every base still 16-byte aligned: no
    matrix-core plan takes the call, and forward and backward are those of the switches at 0, on the same tensors
    and on the contiguous projection, to the bit; the route's own bits are others."""
    from pydrobert_amd import switches

    (q, k, v, mask, dim, scale), _ = device_inputs("fused-qkv", dtname, 4)
    (q0, k0, v0, _, _, _), _ = device_inputs("fused-qkv", dtname)
    assert k.stride(0) == 776 and k.stride(2) == 388 and all(t.data_ptr() % 16 == 0 for t in (q, k, v))
    assert routes(q, k, v, mask, dim) == (False, False, False) and routes(q0, k0, v0, mask, dim)[:2] == (True, True)
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(70, 2, 4, 32))).to(DEV, q.dtype)

    def both_passes(a, b, c):
        out, lse = attend((a, b, c, mask, dim, scale))
        return (out, lse) + tuple(
            torch.ops.pydrobert_amd.dot_attention_backward(gout, a, b, c, mask, out, lse, dim, scale))

    got, route = both_passes(q, k, v), both_passes(q0, k0, v0)
    with switches.override(PDT_ATTN_MFMA=0, PDT_ATTN_MFMA_BWD=0):
        assert routes(q0, k0, v0, mask, dim) == (False, False, False)
        same, tile = both_passes(q, k, v), both_passes(q0, k0, v0)
    bits = lambda t: t.view(torch.int16) if t.dtype != torch.float32 else t  # noqa: E731
    for a, b, c in zip(got, same, tile):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))
    assert not torch.equal(bits(got[0]), bits(route[0])) and not torch.equal(bits(got[3]), bits(route[3]))


def test_float32_stride_of_four_stays_on_the_route():
    (q, k, v, mask, dim, scale), _ = device_inputs("fused-qkv", "float32", 4)
    assert k.stride(2) == 388 and routes(q, k, v, mask, dim) == (False, False, True)
    out, lse = attend((q, k, v, mask, dim, scale))
    ref = F.reference("fused-qkv", "float32")  # (the padding holds no operand: the same numbers)
    err, bound = (out.cpu().double() - ref["out"]).abs(), float32_bound(ref)
    print("fused-qkv + 4 float32 largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()
    first = forward("fused-qkv", "float32")
    assert torch.equal(out.cpu().view(torch.int32), first[0].view(torch.int32)) and torch.equal(lse.cpu(), first[1])
