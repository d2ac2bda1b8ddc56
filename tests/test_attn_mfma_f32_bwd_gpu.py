"""GPU: the float32 attention backward on the matrix cores (csrc/attn_mfma_f32_bwd.hip) through autograd, against
float64 autograd through the formula on the widened operands; every case asserts the route from the plan.  A gradient
is held to the suite's float32 ``tol + tol |ref|`` or, where larger, 8 x the float32 error of ``_softmax_pool``."""
import copy
import functools

import numpy as np
import pytest
import torch

import _attn_mfma_f32 as M
import _attn_mfma_forms as F
import _attn_ref as R
import test_attn_mfma_f32_gpu as G32
import test_attn_mfma_forms_gpu as GF
from test_attn_mfma_gpu import DEV

pytestmark = pytest.mark.gpu

GRAD_TOL = R.SUITE["float32"][1]
NAMES = list(M.CASES) + list(F.BACKWARD_FORMS)


def on_route(q, k, v, mask, dim=0):
    from pydrobert_amd import _attn

    plan, ops = _attn._dot_plan(q, k, v, mask, dim)
    return _attn._mfma_f32_bwd_workspace_bytes(plan, 0, ops, ops[0]) >= 0


@functools.lru_cache(maxsize=None)
def case(name):
    """Device arguments, the leaves they are views of, grad_out, their gradients, the reference's leaves and mask."""
    if name in M.CASES:
        x, (q, k, v, mask, scale) = M.inputs(name), G32.device_inputs(name)
        args, leaves, ref = (q, k, v, mask, 0, scale), [q, k, v], [x["q"], x["k_ref"], x["v_ref"]]
    else:
        x = F.inputs(name, "float32")
        args, leaves = GF.device_inputs(name, "float32")
        ref = F.leaves(name, x, ref=True)
    assert on_route(*args[:5]), "the plan refuses " + name
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(*args[0].shape[:-1], args[2].shape[-1])))
    got = GF.gradients(lambda *t: GF.attend(F.split_of(name)(*t) + args[3:])[0], leaves, gout)
    return args, leaves, gout, got, ref, x["mask"]


@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_float64(name):
    from pydrobert_amd import _attn

    (_, _, _, _, dim, scale), _, gout, got, ref, mask = case(name)
    if name == "dead-row":  # the reference attends everything from the dead row and gets no grad_out there: no 0 / 0
        mask, gout = mask.clone(), gout.clone()
        mask[(slice(None),) + M.DEAD], gout[M.DEAD] = True, 0.0
    split = F.split_of(name)
    want = GF.gradients(lambda *t: R.attend_ref(*split(*t), mask, dim, scale), [t.double() for t in ref], gout)

    def formula(*t):
        a, b, c = split(*t)
        return _attn._softmax_pool((a.unsqueeze(dim) * b).sum(-1) * scale, c, mask, dim)

    for n, g, w, f in zip(("fused",) if len(ref) == 1 else "qkv", got, want, GF.gradients(formula, ref, gout)):
        e_ref = float((f.double() - w).abs().max())
        err = (g.cpu().double() - w).abs()
        bound = (GRAD_TOL + GRAD_TOL * w.abs()).clamp_min(8 * e_ref)
        print("f32-bwd", name, "d" + n, "error/bound", float((err / bound).max()), "formula32", e_ref)
        assert g.dtype == torch.float32 and g.shape == w.shape and torch.isfinite(g).all() and (err <= bound).all()
        if name == "nan-gaps":
            assert (g[..., -F.GAP:] == 0).all(), "nothing of a gap reaches a gradient"


def test_exact_zeros_of_masked_rows_and_frames():
    gq, gk, gv = case("dead-row")[3]
    assert (gq[M.DEAD] == 0).all() and (gq != 0).any()
    gq, gk, gv = case("tails-length")[3]  # NaN planted in the padded keys and values
    for grp, n in enumerate(M.LENGTHS):
        assert (gk[n:, grp] == 0).all() and (gv[n:, grp] == 0).all() and (gk[:n, grp] != 0).any()
    gq, gk, gv = case("batch-first")[3]  # the same in the batch-first row order
    for n, length in enumerate(F.LENGTHS):
        assert (gk[n, length:] == 0).all() and (gv[n, length:] == 0).all() and (gv[n, :length] != 0).any()
    gq, gk, gv = case("split")[3]
    assert (gk[192:] == 0).all() and (gv[192:] == 0).all() and (gk[:192] != 0).any()
    gq, gk, gv = case("three-spans")[3]
    mid = slice(F.SPAN, 2 * F.SPAN)
    assert (gk[mid] == 0).all() and (gv[mid] == 0).all() and (gk[:F.SPAN] != 0).any() and (gk[2 * F.SPAN:] != 0).any()


def test_two_runs_give_equal_bits():
    args, leaves, gout, got, _, _ = case("tails-length")  # D = 64, Dv = 128
    again = GF.gradients(lambda *t: GF.attend(t + args[3:])[0], leaves, gout)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))


def test_misaligned_key_takes_the_tile_backward_to_the_bit():
    from pydrobert_amd import switches

    (q, k, v, mask, dim, scale), _, gout, _, _, _ = case("sixteens")
    k1 = torch.empty(k.numel() + 1, device=DEV, dtype=k.dtype)[1:].view(k.shape).copy_(k)  # one element off
    assert not on_route(q, k1, v, mask)
    out, lse = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, dim, scale)
    go = gout.to(DEV, q.dtype)

    def bwd(key):
        return torch.ops.pydrobert_amd.dot_attention_backward(go, q, key, v, mask, out, lse, dim, scale)

    a, c = bwd(k1), bwd(k)
    with switches.override(PDT_ATTN_MFMA_F32_BWD=0):
        assert not on_route(q, k, v, mask)
        b = bwd(k)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert not any(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(c, b))  # (the route ran)


def test_multi_headed_attention_in_float32():
    """4 heads of 64, T = 96, N = 2, causal: every parameter gradient within the suite's bound of the float64 module's,
    or within 2 x the switch-0 error where the Linears' own float32 rounding is beyond that (both are float32 sums)."""
    from pydrobert_amd import _attn, switches
    from pydrobert_amd.modules import DotProductSoftAttention, MultiHeadedAttention

    torch.manual_seed(1)
    T = 96
    mha = MultiHeadedAttention(256, 256, 256, 4, DotProductSoftAttention(64, 0, 64 ** -0.5)).to(DEV)
    x, gy = torch.randn(T, 2, 256, device=DEV), torch.randn(T, 2, 256, device=DEV)
    mask = torch.arange(T, device=DEV).view(T, 1, 1) <= torch.arange(T, device=DEV).view(1, T, 1)
    taken = []
    inner = _attn._mfma_f32_bwd_workspace_bytes
    _attn._mfma_f32_bwd_workspace_bytes = lambda *a: taken.append(inner(*a)) or taken[-1]

    def param_grads(mod, sw):
        y = x.to(next(mod.parameters()).dtype)
        with switches.override(PDT_ATTN_MFMA_F32_BWD=sw):
            return torch.autograd.grad((mod(y, y[:, None], y[:, None], mask) * gy).sum(), list(mod.parameters()))

    try:
        new = param_grads(mha, 1)
        assert taken[-1] >= 0, "the heads' backward did not take the matrix-core kernels"
        old = param_grads(mha, 0)
        assert taken[-1] < 0
        want = param_grads(copy.deepcopy(mha).double(), 1)
    finally:
        _attn._mfma_f32_bwd_workspace_bytes = inner
    for (n, _), w, a, b in zip(mha.named_parameters(), want, new, old):
        e_old = float((b.double() - w).abs().max())
        err, bound = (a.double() - w).abs(), (GRAD_TOL + GRAD_TOL * w.abs()).clamp_min(2 * e_old)
        print("f32-bwd MHA", n, "error/bound", float((err / bound).max()), "error/switch-0", float(err.max()) / e_old)
        assert (err <= bound).all()


def test_opcheck():
    (q, k, v, mask, dim, scale), _, gout, _, _, _ = case("one-block")
    out, lse = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, dim, scale)
    torch.library.opcheck(torch.ops.pydrobert_amd.dot_attention_backward.default,
                          (gout.to(DEV, q.dtype), q, k, v, mask, out, lse, dim, scale))  # fmt: skip
