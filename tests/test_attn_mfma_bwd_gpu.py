"""GPU: the dot-product attention backward on the matrix cores (csrc/attn_mfma_bwd.hip), through
``pydrobert_amd::dot_attention`` and autograd, for float16 and bfloat16 against float64 autograd through the formula
on the exactly widened operands.  Every case asserts from the plan that the route is taken.  A gradient is held to
1e-4 + 4 x the error of the reference's formula (``_attn._softmax_pool``) evaluated in the same half dtype on the same
inputs; the exact zeros of masked rows and frames, the equal bits of two runs and the tile backward behind a
misaligned key or the switch are asserted as such."""
import functools

import numpy as np
import pytest
import torch

import _attn_mfma as M
import _attn_ref as R
from test_attn_mfma_gpu import DEV, DTNAMES, device_inputs, grads

pytestmark = pytest.mark.gpu

BIG = dict(G=1, M=80, T=72, D=128, Dv=128)  # the LDS request above 64 KiB, a row tail and a frame tail


def on_route(q, k, v, mask, gout=None):
    from pydrobert_amd import _attn

    plan, ops = _attn._dot_plan(q, k, v, mask, 0)
    gout = q if gout is None else gout  # (the operator's grad_out is a fresh contiguous tensor)
    return _attn._mfma_bwd_workspace_bytes(plan, M.ELEM[str(q.dtype).split(".")[1]], ops, gout) >= 0


def attend(mask, scale):
    return lambda a, b, c: torch.ops.pydrobert_amd.dot_attention(a, b, c, mask, 0, scale)[0]


@functools.lru_cache(maxsize=None)
def case(name, dtname):
    """Device inputs, grad_out, the operator's gradients and the reference's operands (CPU, the half dtype)."""
    if name != "big":
        q, k, v, mask, scale = device_inputs(name, dtname)
        x = M.inputs(name, dtname)
        ref = (x["q"], x["k_ref"], x["v_ref"], x["mask"])
    else:
        rng, c = np.random.default_rng(11), BIG
        q, k, v = (torch.from_numpy(rng.normal(size=s)).to(M.DTYPES[dtname]) for s in (
            (c["G"], c["M"], c["D"]), (c["T"], c["G"], 1, c["D"]), (c["T"], c["G"], 1, c["Dv"])))  # fmt: skip
        mask = (torch.arange(c["T"]).view(-1, 1, 1) <= torch.arange(c["M"]).view(1, 1, -1)).expand(-1, c["G"], -1)
        ref, scale = (q, k, v, mask), c["D"] ** -0.5
        q, k, v, mask = (t.to(DEV) for t in ref)
    assert on_route(q, k, v, mask), "the plan refuses " + name
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(*q.shape[:-1], v.shape[-1])))
    return (q, k, v, mask, scale), gout, grads(attend(mask, scale), q, k, v, gout), ref


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", list(M.CASES) + ["big"])
def test_gradients_against_float64(name, dtname):
    from pydrobert_amd import _attn

    (q, k, v, mask, scale), gout, got, (rq, rk, rv, rmask) = case(name, dtname)
    if name == "dead-row":  # the reference attends everything from the dead row and is given no grad_out there:
        rmask, gout = rmask.clone(), gout.clone()  # its dQ is 0 and it adds 0 to dK and dV, without a 0 / 0
        rmask[(slice(None),) + M.DEAD], gout[M.DEAD] = True, 0.0
    want = grads(lambda a, b, c: R.attend_ref(a, b, c, rmask, 0, scale), rq.double(), rk.double(), rv.double(), gout)
    dmask = None if rmask is None else rmask.to(DEV)
    formula = grads(lambda a, b, c: _attn._softmax_pool((a.unsqueeze(0) * b).sum(-1) * scale, c, dmask, 0),
                    rq.to(DEV), rk.to(DEV), rv.to(DEV), gout)  # fmt: skip
    for n, g, w, f in zip("qkv", got, want, formula):
        e_ref = float((f.cpu().double() - w).abs().max())
        err = float((g.cpu().double() - w).abs().max())
        print(name, dtname, "d" + n, "error", err, "formula's", e_ref, "ratio", err / e_ref)
        assert g.dtype == M.DTYPES[dtname] and g.shape == w.shape and err <= 1e-4 + 4 * e_ref


@pytest.mark.parametrize("dtname", DTNAMES)
def test_exact_zeros_of_masked_rows_and_frames(dtname):
    gq, gk, gv = case("dead-row", dtname)[2]
    assert (gq[M.DEAD] == 0).all() and torch.isfinite(gk).all() and torch.isfinite(gv).all()
    gq, gk, gv = case("tails-length", dtname)[2]  # NaN planted in the padded keys and values
    assert all(torch.isfinite(g).all() for g in (gq, gk, gv))
    for grp, n in enumerate(M.LENGTHS):
        assert (gk[n:, grp] == 0).all() and (gv[n:, grp] == 0).all() and (gk[:n, grp] != 0).any()
    gq, gk, gv = case("split", dtname)[2]
    assert (gk[192:] == 0).all() and (gv[192:] == 0).all() and (gk[:192] != 0).any()


@pytest.mark.parametrize("dtname", DTNAMES)
def test_two_runs_give_equal_bits(dtname):
    (q, k, v, mask, scale), gout, got, _ = case("causal", dtname)
    again = grads(attend(mask, scale), q, k, v, gout)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(got, again))


@pytest.mark.parametrize("dtname", DTNAMES)
def test_misaligned_key_takes_the_tile_backward_to_the_bit(dtname):
    from pydrobert_amd import switches

    (q, k, v, mask, scale), gout, _, _ = case("random-96", dtname)
    k1 = torch.empty(k.numel() + 1, device=DEV, dtype=k.dtype)[1:].view(k.shape).copy_(k)  # one element off
    assert not on_route(q, k1, v, mask)

    def both_passes(key):  # (the operators themselves: a leaf cloned for autograd would be aligned again)
        out, lse = torch.ops.pydrobert_amd.dot_attention(q, key, v, mask, 0, scale)
        return torch.ops.pydrobert_amd.dot_attention_backward(gout.to(DEV, q.dtype), q, key, v, mask, out, lse, 0, scale)

    a = both_passes(k1)
    with switches.override(PDT_ATTN_MFMA_BWD=0, PDT_ATTN_MFMA=0):  # (the misaligned key keeps the forward off too)
        assert not on_route(q, k, v, mask)
        b = both_passes(k)
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))
    assert not torch.equal(a[1], both_passes(k)[1])  # (and the route's bits are others)


def test_multi_headed_attention_under_autocast():
    """float32 parameters under autocast(bfloat16), T = 96, N = 2, causal: the heads' backward takes the route, and
    every parameter gradient is as close to the float32 module's as with the switch at 0 allows: 1e-4 + 4 x the
    switch-0 error, which is the yardstick here."""
    from pydrobert_amd import _attn, switches
    from pydrobert_amd.modules import DotProductSoftAttention, MultiHeadedAttention

    torch.manual_seed(1)
    T, N = 96, 2
    mha = MultiHeadedAttention(256, 256, 256, 4, DotProductSoftAttention(64, 0, 64 ** -0.5)).to(DEV)
    x, gy = torch.randn(T, N, 256, device=DEV), torch.randn(T, N, 256, device=DEV)
    kv = x.unsqueeze(1)
    mask = torch.arange(T, device=DEV).view(T, 1, 1) <= torch.arange(T, device=DEV).view(1, T, 1)
    taken = []
    inner = _attn._mfma_bwd_workspace_bytes
    _attn._mfma_bwd_workspace_bytes = lambda *a: taken.append(inner(*a)) or taken[-1]

    def param_grads(autocast, sw):
        with switches.override(PDT_ATTN_MFMA_BWD=sw), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return torch.autograd.grad((mha(x, kv, kv, mask).float() * gy).sum(), list(mha.parameters()))

    try:
        want, new = param_grads(False, 1), param_grads(True, 1)
        assert taken[-1] >= 0, "the heads' backward did not take the matrix-core kernels"
        old = param_grads(True, 0)
        assert taken[-1] < 0
    finally:
        _attn._mfma_bwd_workspace_bytes = inner
    for (n, _), w, a, b in zip(mha.named_parameters(), want, new, old):
        e_new, e_old = float((a - w).abs().max()), float((b - w).abs().max())
        print("autocast MHA:", n, "error with the route", e_new, "without", e_old)
        assert e_new <= 1e-4 + 4 * e_old


def test_opcheck():
    (q, k, v, mask, scale), gout, _, _ = case("one-block", "bfloat16")
    out, lse = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale)
    torch.library.opcheck(torch.ops.pydrobert_amd.dot_attention_backward.default,
                          (gout.to(DEV, q.dtype), q, k, v, mask, out, lse, 0, scale))  # fmt: skip
