"""GPU: the float32 dot-product attention forward of decode shapes (csrc/attn_mfma_dec.hip), through
``pydrobert_amd::dot_attention`` and ``DotProductSoftAttention``, against the float64 formula on the same numbers.
Every case asserts from the plan that the route was taken.  The bounds are those tests/test_attn_mfma_f32_gpu.py
applies: ``out`` within the suite's float32 bound or, where the float32 formula itself is worse, 8 x its error;
``lse`` within 2e-5 (1 + |ref|); the gradients (the unchanged attn_bwd_kernel fed by this forward) within the suite's
1e-4 + 1e-4 |ref| and within 4 x the error of the same call on attn_fwd_kernel.

Measured on an MI355X (profiles/attn_mfma_dec_errors.json): every gradient within the 1e-4 bound (largest error
1.2e-5); the ratios to attn_fwd_kernel's error are 0.94 to 1.15 on "wide" and 1.08 to 1.72 on "rising"."""
import functools

import numpy as np
import pytest
import torch

import _attn_mfma_dec as M
import _attn_ref as R
from test_attn_mfma_f32_gpu import GRAD_TOL, OUT_TOL
from test_attn_mfma_gpu import DEV, grads

pytestmark = pytest.mark.gpu


def on_route(q, k, v, mask, dim=0):
    from pydrobert_amd import _attn

    plan, ops = _attn._dot_plan(q, k, v, mask, dim)
    return _attn._mfma_dec_workspace_bytes(plan, 0, ops) >= 0


def attend(x, k=None):
    import pydrobert_amd.modules  # noqa: F401

    return torch.ops.pydrobert_amd.dot_attention(x["q"], x["k"] if k is None else k, x["v"], x["mask"], x["dim"], x["scale"])


@functools.lru_cache(maxsize=None)
def run(name):
    x = M.inputs(name, DEV)
    assert on_route(x["q"], x["k"], x["v"], x["mask"], x["dim"]), "the plan refuses " + name
    out, lse = attend(x)
    return out.cpu(), lse.cpu()


@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_against_float64(name):
    ref = M.reference(name)
    out, lse = run(name)
    assert out.dtype == torch.float32 and lse.dtype == torch.float32 and out.shape == ref["out"].shape
    dead = torch.isnan(ref["out"]).any(-1)  # the all-masked row; "nonfinite": plus the row that attends the bad frame
    assert int(dead.sum()) == (1 if name == "empty-span" else 0)
    if name == "nonfinite":
        dead[0, 0] = True
        assert not torch.isfinite(out[0, 0]).any()
    else:
        assert torch.equal(torch.isnan(out).all(-1), dead)
    assert torch.equal(torch.isfinite(out).all(-1), ~dead)
    live = ~dead.reshape(-1)
    err = (out.double() - ref["out"]).abs().reshape(live.numel(), -1)[live]
    bound = (OUT_TOL + OUT_TOL * ref["out"].abs()).clamp_min(8 * ref["err32"]).reshape(live.numel(), -1)[live]
    print(name, "largest error / bound", float((err / bound).max()), "formula's float32 error", ref["err32"])
    assert (err <= bound).all()
    for got, want in ((lse[0], ref["m"]), (lse[1], ref["logsum"])):
        assert ((got.double() - want).abs()[live] <= 2e-5 * (1 + want.abs()[live])).all()
        if name != "nonfinite":
            assert (got[~live] == -float("inf")).all()  # (what attn_fwd_kernel stores for an all-masked row)


@pytest.mark.parametrize("name", M.GRAD_CASES)
def test_gradients_through_the_unchanged_backward(name):
    from pydrobert_amd import switches

    x = M.inputs(name, DEV)
    q, k, v, mask, scale = x["q"], x["k"], x["v"], x["mask"], x["scale"]
    assert on_route(q, k, v, mask)
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=M.reference(name)["out"].shape))
    fn = lambda a, b, c: torch.ops.pydrobert_amd.dot_attention(a, b, c, mask, 0, scale)[0]  # noqa: E731
    got = grads(fn, q, k, v, gout)
    with switches.override(PDT_ATTN_MFMA_DEC=0):
        old = grads(fn, q, k, v, gout)
    cm = None if mask is None else mask.cpu()
    want = grads(lambda a, b, c: R.attend_ref(a, b, c, cm, 0, scale), *(t.cpu().double() for t in (q, k, v)), gout)
    for n, g, o, w in zip("qkv", got, old, want):
        err, e_old = (g.cpu().double() - w).abs(), float((o.cpu().double() - w).abs().max())
        print(name, "d" + n, "error", float(err.max()), "attn_fwd_kernel's", e_old, "ratio", float(err.max()) / e_old)
        assert g.dtype == torch.float32 and (err <= GRAD_TOL + GRAD_TOL * w.abs()).all() and err.max() <= 4 * e_old


def test_switch_off_and_misaligned_key_take_the_tile_kernel_to_the_bit():
    from pydrobert_amd import switches

    x = M.inputs("wide", DEV)
    k1 = torch.empty(x["k"].numel() + 1, device=DEV)[1:].view(x["k"].shape).copy_(x["k"])  # four bytes off
    assert on_route(x["q"], x["k"], x["v"], x["mask"]) and not on_route(x["q"], k1, x["v"], x["mask"])
    new, again, off = attend(x), attend(x), attend(x, k1)
    with switches.override(PDT_ATTN_MFMA_DEC=0):
        assert not on_route(x["q"], x["k"], x["v"], x["mask"])
        old = attend(x)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(off[0]), bits(old[0])) and torch.equal(bits(off[1]), bits(old[1]))
    assert torch.equal(bits(new[0]), bits(again[0])) and torch.equal(bits(new[1]), bits(again[1]))
    assert not torch.equal(bits(new[0]), bits(old[0]))  # (the route really ran)


def test_dot_product_soft_attention_over_beams():
    """N = 4 utterances, K = 8 beams sharing an utterance's keys, T = 96 frames, a length mask."""
    from pydrobert_amd.modules import DotProductSoftAttention

    torch.manual_seed(2)
    N, K, T, D = 4, 8, 96, 64
    q, k, v = torch.randn(N, K, D, device=DEV), torch.randn(T, N, 1, D, device=DEV), torch.randn(T, N, 1, D, device=DEV)
    mask = torch.arange(T, device=DEV).view(T, 1, 1) < torch.tensor([96, 64, 33, 1], device=DEV).view(1, N, 1)
    assert on_route(q, k, v, mask)
    got = DotProductSoftAttention(D, 0, D ** -0.5)(q, k, v, mask)
    want = R.attend_ref(q.cpu().double(), k.cpu().double(), v.cpu().double(), mask.cpu().expand(T, N, K), 0, D ** -0.5)
    assert got.dtype == torch.float32 and ((got.cpu().double() - want).abs() <= OUT_TOL + OUT_TOL * want.abs()).all()


def test_opcheck():
    x = M.inputs("tails", DEV)
    assert on_route(x["q"], x["k"], x["v"], x["mask"])
    torch.library.opcheck(torch.ops.pydrobert_amd.dot_attention.default, (x["q"], x["k"], x["v"], x["mask"], 0, x["scale"]))
