"""GPU: the dot-product attention forward on the matrix cores (csrc/attn_mfma.hip), through
``pydrobert_amd::dot_attention``, for float16 and bfloat16 against the float64 formula on the exactly widened
operands.  Every case asserts from the plan that the route was taken.  The bound of ``out`` is derived
(``_attn_mfma.out_bound``), ``lse`` is held to 2e-5 (1 + |ref|), the gradients (the unchanged half backward fed by
this forward) to 1e-4 + 4 x the error of the reference's formula evaluated in the same half dtype."""
import functools

import pytest
import torch

import _attn_mfma as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTNAMES = list(M.DTYPES)


def on_route(q, k, v, mask, dim=0):
    from pydrobert_amd import _attn

    plan, ops = _attn._dot_plan(q, k, v, mask, dim)
    return _attn._mfma_workspace_bytes(plan, M.ELEM[str(q.dtype).split(".")[1]], ops) >= 0


def device_inputs(name, dtname):
    x = M.inputs(name, dtname)
    q, k, v = (torch.empty_strided(x[n].size(), x[n].stride(), device=DEV, dtype=x[n].dtype).copy_(x[n])
               for n in ("q", "k", "v"))  # fmt: skip
    return q, k, v, None if x["mask"] is None else x["mask"].to(DEV), x["scale"]


@functools.lru_cache(maxsize=None)
def run(name, dtname):
    import pydrobert_amd.modules  # noqa: F401

    q, k, v, mask, scale = device_inputs(name, dtname)
    assert on_route(q, k, v, mask), "the plan refuses " + name
    out, lse = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale)
    return out.cpu(), lse.cpu()


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_against_float64(name, dtname):
    c, ref = M.CASES[name], M.reference(name, dtname)
    out, lse = run(name, dtname)
    assert out.dtype == M.DTYPES[dtname] and lse.dtype == torch.float32 and out.shape == ref["out"].shape
    dead = torch.isnan(ref["out"]).any(-1)
    assert int(dead.sum()) == (1 if name == "dead-row" else 0)
    assert torch.equal(torch.isnan(out).all(-1), dead) and torch.equal(torch.isnan(out).any(-1), dead)
    live = ~dead.reshape(-1)
    err = (out.double() - ref["out"]).abs().reshape(live.numel(), -1)[live]
    bound = M.out_bound(ref["out"], ref["A"], ref["vmax"], c["T"], dtname).reshape(live.numel(), -1)[live]
    print(name, dtname, "largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()
    for got, want in ((lse[0], ref["m"]), (lse[1], ref["logsum"])):
        assert ((got.double() - want).abs()[live] <= 2e-5 * (1 + want.abs()[live])).all()
        assert (got[~live] == -float("inf")).all()  # (what attn_fwd_kernel stores for an all-masked row)


def grads(fn, q, k, v, gout):
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    return torch.autograd.grad((fn(*leaves).double() * gout.to(q.device)).sum(), leaves)


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", M.GRAD_CASES + ("dead-row",))
def test_gradients_through_the_unchanged_backward(name, dtname):
    from pydrobert_amd import _attn
    import _attn_ref as R

    q, k, v, mask, scale = device_inputs(name, dtname)
    gout = torch.from_numpy(__import__("numpy").random.default_rng(5).normal(size=M.reference(name, dtname)["out"].shape))
    got = grads(lambda a, b, c: torch.ops.pydrobert_amd.dot_attention(a, b, c, mask, 0, scale)[0], q, k, v, gout)
    if name == "dead-row":  # its own dQ exactly 0, its group's dK / dV finite
        assert (got[0][M.DEAD] == 0).all() and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
        return
    cm = None if mask is None else mask.cpu()
    want = grads(lambda a, b, c: R.attend_ref(a, b, c, cm, 0, scale), q.cpu().double(), k.cpu().double(),
                 v.cpu().double(), gout)  # fmt: skip
    formula = grads(lambda a, b, c: _attn._softmax_pool((a.unsqueeze(0) * b).sum(-1) * scale, c, mask, 0), q, k, v, gout)
    for n, g, w, f in zip("qkv", got, want, formula):
        e_ref = float((f.cpu().double() - w).abs().max())
        err = float((g.cpu().double() - w).abs().max())
        print(name, dtname, "d" + n, "error", err, "formula's", e_ref, "ratio", err / e_ref)
        assert g.dtype == M.DTYPES[dtname] and err <= 1e-4 + 4 * e_ref


@pytest.mark.parametrize("dtname", DTNAMES)
def test_misaligned_input_takes_the_tile_kernels_to_the_bit(dtname):
    from pydrobert_amd import switches

    q, k, v, mask, scale = device_inputs("random-96", dtname)
    k1 = torch.empty(k.numel() + 1, device=DEV, dtype=k.dtype)[1:].view(k.shape).copy_(k)  # one element off
    assert on_route(q, k, v, mask) and not on_route(q, k1, v, mask)
    a = torch.ops.pydrobert_amd.dot_attention(q, k1, v, mask, 0, scale)
    with switches.override(PDT_ATTN_MFMA=0):
        assert not on_route(q, k, v, mask)
        b = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


def test_multi_headed_attention_under_autocast():
    """float32 parameters under autocast(bfloat16), T = 96, N = 2, causal: the heads' self-attention takes the
    route, and the output is as close to the float32 module's as with the switch at 0, within the forward bound
    (u for the attention output once more per projection: here simply both held to the same derived bound)."""
    from pydrobert_amd import _attn, switches
    from pydrobert_amd.modules import DotProductSoftAttention, MultiHeadedAttention

    torch.manual_seed(1)
    T, N = 96, 2
    mha = MultiHeadedAttention(256, 256, 256, 4, DotProductSoftAttention(64, 0, 64 ** -0.5)).to(DEV)
    x = torch.randn(T, N, 256, device=DEV)
    kv = x.unsqueeze(1)  # query (T, N, .), key and value (T, 1, N, .): the T queries are the group
    mask = torch.arange(T, device=DEV).view(T, 1, 1) <= torch.arange(T, device=DEV).view(1, T, 1)
    taken = []
    inner = _attn._mfma_workspace_bytes
    _attn._mfma_workspace_bytes = lambda *a: taken.append(inner(*a)) or taken[-1]
    try:
        with torch.no_grad():
            want = mha(x, kv, kv, mask)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                got = mha(x, kv, kv, mask)
                assert taken and taken[-1] >= 0, "the heads' attention did not take the matrix-core forward"
                with switches.override(PDT_ATTN_MFMA=0):
                    old = mha(x, kv, kv, mask)
                    assert taken[-1] < 0
    finally:
        _attn._mfma_workspace_bytes = inner
    e_new, e_old = (got.float() - want).abs().max(), (old.float() - want).abs().max()
    print("autocast MHA: error with the route", float(e_new), "without", float(e_old))
    # both are bfloat16 pipelines of three projections around the attention: u |x| per stage, |x| <= 4 here
    assert got.dtype == torch.bfloat16 and e_new <= e_old + 2.0 ** -8 * float(want.abs().max()) + 2e-5


def test_opcheck():
    q, k, v, mask, scale = device_inputs("one-block", "bfloat16")
    assert on_route(q, k, v, mask)
    torch.library.opcheck(torch.ops.pydrobert_amd.dot_attention.default, (q, k, v, mask, 0, scale))
