"""GPU: the float32 dot-product attention backward of decode shapes (csrc/attn_mfma_dec_bwd.hip) through autograd of
``pydrobert_amd::dot_attention``, against float64 autograd of the formula on the same numbers.  Every case asserts from
the plan that the route is taken.  Bounds: the suite's 1e-4 + 1e-4 |ref| on every gradient, and on "wide" and "rising"
at most 4 x the error of the same call on attn_bwd_kernel (PDT_ATTN_MFMA_DEC_BWD=0), the project's limit of DESIGN.md
section 14.  Measured figures: profiles/attn_mfma_dec_bwd_errors.json."""
import functools

import numpy as np
import pytest
import torch

import _attn_mfma_dec as M
import _attn_ref as R
from test_attn_mfma_f32_gpu import GRAD_TOL
from test_attn_mfma_gpu import DEV, grads

pytestmark = pytest.mark.gpu
NAMES = ("one-block", "tails", "rising", "wide", "empty-span", "nonfinite", "projection")
bits = lambda t: t.view(torch.int32)  # noqa: E731


def on_route(q, k, v, mask, dim=0):
    from pydrobert_amd import _attn

    plan, ops = _attn._dot_plan(q, k, v, mask, dim)
    return _attn._mfma_dec_bwd_workspace_bytes(plan, 0, ops, ops[0]) >= 0


@functools.lru_cache(maxsize=None)
def run(name):
    """The case on the device, grad_out, the route's gradients and float64's (the dead row of "empty-span" attends
    everything and gets no grad_out in the reference: no 0 / 0 there)."""
    import pydrobert_amd.modules  # noqa: F401

    x = M.inputs(name, DEV)
    q, k, v, mask, dim, scale = (x[n] for n in ("q", "k", "v", "mask", "dim", "scale"))
    assert on_route(q, k, v, mask, dim), "the plan refuses " + name
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=M.reference(name)["out"].shape))
    fn = lambda a, b, c: torch.ops.pydrobert_amd.dot_attention(a, b, c, mask, dim, scale)[0]  # noqa: E731
    got = grads(fn, q, k, v, gout)
    cm, gref = None if mask is None else mask.cpu().clone(), gout.clone()
    if name == "empty-span":
        cm[(slice(None),) + M.DEAD], gref[M.DEAD] = True, 0.0
    ref = lambda a, b, c: R.attend_ref(a, b, c, cm, dim, scale)  # noqa: E731
    want = grads(ref, *(x[n].cpu().double() for n in ("q", "k_ref", "v_ref")), gref)
    return x, gout, fn, [g.cpu() for g in got], want


@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_float64(name):
    _, _, _, got, want = run(name)
    for n, g, w in zip("qkv", got, want):
        assert g.dtype == torch.float32 and g.shape == w.shape
        if name == "nonfinite":  # all but row 0 of group 0, which attends the bad frame, and group 0's dK / dV, which
            # carry that row's NaN: rows 1 to 8 mask the frame, stay finite and match the reference without it
            g, w = (g.reshape(-1, g.shape[-1])[1:], w.reshape(-1, w.shape[-1])[1:]) if n == "q" else (g[:, 1:], w[:, 1:])
        err = (g.double() - w).abs()
        print(name, "d" + n, "largest error / bound", float((err / (GRAD_TOL + GRAD_TOL * w.abs())).max()))
        assert torch.isfinite(g).all() and (err <= GRAD_TOL + GRAD_TOL * w.abs()).all()


@pytest.mark.parametrize("name", M.GRAD_CASES)
def test_error_within_four_times_the_tile_backward(name):
    from pydrobert_amd import switches

    x, gout, fn, got, want = run(name)
    with switches.override(PDT_ATTN_MFMA_DEC_BWD=0):
        assert not on_route(x["q"], x["k"], x["v"], x["mask"])
        old = grads(fn, x["q"], x["k"], x["v"], gout)
    for n, g, o, w in zip("qkv", got, old, want):
        e_new, e_old = float((g.double() - w).abs().max()), float((o.cpu().double() - w).abs().max())
        print(name, "d" + n, "error", e_new, "attn_bwd_kernel's", e_old, "ratio", e_new / e_old)
        assert e_new <= 4 * e_old


def test_exact_zeros_as_bits():
    _, gk, gv = run("wide")[3]  # NaN behind every group's length is never read
    for grp, n in enumerate(M.LENGTHS):
        assert not bits(gk[n:, grp]).any() and not bits(gv[n:, grp]).any() and (gk[:n, grp] != 0).any()
    gq, gk, gv = run("empty-span")[3]
    assert not bits(gq[M.DEAD]).any() and (gq[0] != 0).any()
    assert not bits(gk[64:128, 0]).any() and not bits(gv[64:128, 0]).any() and (gk[64:128, 1] != 0).any()


def test_routes_on_wide():
    """The switch at 0 and a key four bytes off give attn_bwd_kernel's bits; the route's own repeat and differ."""
    from pydrobert_amd import switches

    x, gout, _, _, _ = run("wide")
    q, k, v, mask, scale = (x[n] for n in ("q", "k", "v", "mask", "scale"))
    k1 = torch.empty(k.numel() + 1, device=DEV)[1:].view(k.shape).copy_(k)  # four bytes off
    assert not on_route(q, k1, v, mask)
    out, lse = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale)
    go = gout.to(DEV, q.dtype)
    bwd = lambda key: torch.ops.pydrobert_amd.dot_attention_backward(go, q, key, v, mask, out, lse, 0, scale)  # noqa: E731
    new, again, off = bwd(k), bwd(k), bwd(k1)
    with switches.override(PDT_ATTN_MFMA_DEC_BWD=0):
        old = bwd(k)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(off, old))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(new, again))
    assert not any(torch.equal(bits(a), bits(b)) for a, b in zip(new, old))  # (the route really ran)


def test_dot_product_soft_attention_over_beams():
    """N = 4 utterances, K = 8 beams sharing an utterance's keys, T = 96 frames, a length mask: forward + backward."""
    from pydrobert_amd.modules import DotProductSoftAttention

    torch.manual_seed(2)
    N, K, T, D = 4, 8, 96, 64
    q, k, v = torch.randn(N, K, D, device=DEV), torch.randn(T, N, 1, D, device=DEV), torch.randn(T, N, 1, D, device=DEV)
    mask = torch.arange(T, device=DEV).view(T, 1, 1) < torch.tensor([96, 64, 33, 1], device=DEV).view(1, N, 1)
    assert on_route(q, k, v, mask)
    gout, cm = torch.randn(N, K, D).double(), mask.cpu().expand(T, N, K)
    got = grads(lambda a, b, c: DotProductSoftAttention(D, 0, D ** -0.5)(a, b, c, mask), q, k, v, gout)
    want = grads(lambda a, b, c: R.attend_ref(a, b, c, cm, 0, D ** -0.5), *(t.cpu().double() for t in (q, k, v)), gout)
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and ((g.cpu().double() - w).abs() <= GRAD_TOL + GRAD_TOL * w.abs()).all()


def test_opcheck():
    x, gout, _, _, _ = run("tails")
    q, k, v, scale = x["q"], x["k"], x["v"], x["scale"]
    out, lse = torch.ops.pydrobert_amd.dot_attention(q, k, v, None, 0, scale)
    torch.library.opcheck(torch.ops.pydrobert_amd.dot_attention_backward.default,
                          (gout.to(DEV, q.dtype), q, k, v, None, out, lse, 0, scale))
