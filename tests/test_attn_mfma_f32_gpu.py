"""GPU: the float32 dot-product attention forward on the matrix cores (csrc/attn_mfma_f32.hip), through
``pydrobert_amd::dot_attention`` and the modules, against the float64 formula on the same numbers.  Every case
asserts from the plan that the route was taken.  ``out`` is held to the suite's float32 bound
(``_attn_ref.SUITE``: 2e-5 + 2e-5 |ref|) or, where the float32 formula itself is worse, to 8 x the error of the
reference's formula in float32 on the CPU; ``lse`` to 2e-5 (1 + |ref|); the gradients (the unchanged float32
backward fed by this forward) to the suite's 1e-4 + 1e-4 |ref| or 8 x the formula's gradient error."""
import functools

import numpy as np
import pytest
import torch

import _attn_mfma_f32 as M
import _attn_ref as R
from test_attn_mfma_gpu import DEV, grads

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = R.SUITE["float32"]


def on_route(q, k, v, mask, dim=0):
    from pydrobert_amd import _attn

    plan, ops = _attn._dot_plan(q, k, v, mask, dim)
    return _attn._mfma_f32_workspace_bytes(plan, 0, ops) >= 0


def device_inputs(name):
    x = M.inputs(name)
    q, k, v = (torch.empty_strided(x[n].size(), x[n].stride(), device=DEV, dtype=x[n].dtype).copy_(x[n])
               for n in ("q", "k", "v"))  # fmt: skip
    return q, k, v, None if x["mask"] is None else x["mask"].to(DEV), x["scale"]


@functools.lru_cache(maxsize=None)
def run(name):
    import pydrobert_amd.modules  # noqa: F401

    q, k, v, mask, scale = device_inputs(name)
    assert on_route(q, k, v, mask), "the plan refuses " + name
    out, lse = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale)
    return out.cpu(), lse.cpu()


@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_against_float64(name):
    ref = M.reference(name)
    out, lse = run(name)
    assert out.dtype == torch.float32 and lse.dtype == torch.float32 and out.shape == ref["out"].shape
    dead = torch.isnan(ref["out"]).any(-1)
    assert int(dead.sum()) == (1 if name == "dead-row" else 0)
    # NaN exactly in the all-masked row: the NaN planted in padded frames and the empty span leave nothing behind
    assert torch.equal(torch.isnan(out).all(-1), dead) and torch.equal(torch.isfinite(out).all(-1), ~dead)
    live = ~dead.reshape(-1)
    err = (out.double() - ref["out"]).abs().reshape(live.numel(), -1)[live]
    bound = (OUT_TOL + OUT_TOL * ref["out"].abs()).clamp_min(8 * ref["err32"]).reshape(live.numel(), -1)[live]
    print(name, "largest error / bound", float((err / bound).max()), "formula's float32 error", ref["err32"])
    assert (err <= bound).all()
    for got, want in ((lse[0], ref["m"]), (lse[1], ref["logsum"])):
        assert ((got.double() - want).abs()[live] <= 2e-5 * (1 + want.abs()[live])).all()
        assert (got[~live] == -float("inf")).all()  # (what attn_fwd_kernel stores for an all-masked row)


@pytest.mark.parametrize("name", M.GRAD_CASES)
def test_gradients_through_the_unchanged_backward(name):
    from pydrobert_amd import _attn

    q, k, v, mask, scale = device_inputs(name)
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=M.reference(name)["out"].shape))
    got = grads(lambda a, b, c: torch.ops.pydrobert_amd.dot_attention(a, b, c, mask, 0, scale)[0], q, k, v, gout)
    cpu = [t.cpu() for t in (q, k, v)]
    cm = mask.cpu()
    want = grads(lambda a, b, c: R.attend_ref(a, b, c, cm, 0, scale), *(t.double() for t in cpu), gout)
    formula = grads(lambda a, b, c: _attn._softmax_pool((a.unsqueeze(0) * b).sum(-1) * scale, c, cm, 0), *cpu, gout)
    for n, g, w, f in zip("qkv", got, want, formula):
        e_ref = float((f.double() - w).abs().max())
        err = (g.cpu().double() - w).abs()
        bound = (GRAD_TOL + GRAD_TOL * w.abs()).clamp_min(8 * e_ref)
        print(name, "d" + n, "largest error / bound", float((err / bound).max()), "formula's float32 error", e_ref)
        assert g.dtype == torch.float32 and (err <= bound).all()


def test_two_runs_are_equal_to_the_bit():
    q, k, v, mask, scale = device_inputs("causal")
    a, b = (torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale) for _ in range(2))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_misaligned_key_takes_the_tile_kernel_to_the_bit():
    from pydrobert_amd import switches

    q, k, v, mask, scale = device_inputs("sixteens")
    k1 = torch.empty(k.numel() + 1, device=DEV, dtype=k.dtype)[1:].view(k.shape).copy_(k)  # one element off
    assert on_route(q, k, v, mask) and not on_route(q, k1, v, mask)
    a = torch.ops.pydrobert_amd.dot_attention(q, k1, v, mask, 0, scale)
    c = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale)
    with switches.override(PDT_ATTN_MFMA_F32=0):
        assert not on_route(q, k, v, mask)
        b = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert not torch.equal(c[0].view(torch.int32), b[0].view(torch.int32))  # (the route really ran)


def test_multi_headed_attention_in_float32():
    """The defaults of the attention modules: float32, T = 96, N = 2, causal.  The heads' self-attention takes the
    route and the output is within the suite's bound of the float64 module's."""
    import copy

    from pydrobert_amd import _attn
    from pydrobert_amd.modules import DotProductSoftAttention, MultiHeadedAttention

    torch.manual_seed(1)
    T, N = 96, 2
    mha = MultiHeadedAttention(256, 256, 256, 4, DotProductSoftAttention(64, 0, 64 ** -0.5)).to(DEV)
    x = torch.randn(T, N, 256, device=DEV)
    mask = torch.arange(T, device=DEV).view(T, 1, 1) <= torch.arange(T, device=DEV).view(1, T, 1)
    taken = []
    inner = _attn._mfma_f32_workspace_bytes
    _attn._mfma_f32_workspace_bytes = lambda *a: taken.append(inner(*a)) or taken[-1]
    try:
        with torch.no_grad():
            got = mha(x, x.unsqueeze(1), x.unsqueeze(1), mask)  # query (T, N, .), key and value (T, 1, N, .)
    finally:
        _attn._mfma_f32_workspace_bytes = inner
    assert taken and taken[-1] >= 0, "the heads' attention did not take the matrix-core forward"
    x64 = x.double()
    with torch.no_grad():
        want = copy.deepcopy(mha).double()(x64, x64.unsqueeze(1), x64.unsqueeze(1), mask)
    err = (got.double() - want).abs()
    print("float32 MHA: largest error / bound", float((err / (OUT_TOL + OUT_TOL * want.abs())).max()))
    assert got.dtype == torch.float32 and (err <= OUT_TOL + OUT_TOL * want.abs()).all()


def test_opcheck():
    q, k, v, mask, scale = device_inputs("one-block")
    assert on_route(q, k, v, mask)
    torch.library.opcheck(torch.ops.pydrobert_amd.dot_attention.default, (q, k, v, mask, 0, scale))
