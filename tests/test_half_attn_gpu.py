"""GPU: float16 / bfloat16 operands on the attention kernels.  A half call is the float32 call on the exactly
widened operands with each result rounded once where it is stored, so the forward and every gradient are held to
the BIT against the float32 operators on ``leaf.float()``, for every float32 case of tests/_attn_ref.py (every
plan form: walks, rows per tile set by LDS, value column blocks, key loop tails, the rows kernel, frame chunks,
empty spans, spoiled masked frames, scores at -inf, all-masked rows, shifted scores) and both half dtypes; the
forward also against the float64 formula within the float32 bound plus one rounding; no float32 copy of an
operand is made; the five modules take the route, MultiHeadedAttention under autocast included."""
import functools

import pytest
import torch

import _attn_ref as R
import _half_attn as ha
from test_attn_cpu import cosine_attention

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTNAMES = list(ha.DTYPES)


@functools.lru_cache(maxsize=None)
def run(name, dtname):
    """One case in one half dtype, every operator called directly: the half forward and backward, and the float32
    ones on the widened leaves (the backward's on the widened upstream gradient and the widened HALF output, with
    the half call's lse).  Spoiled inputs where the case has them.  Cached: treat as read-only."""
    import pydrobert_amd.modules  # noqa: F401

    dt = ha.DTYPES[dtname]
    Lh = ha.leaves(name, dt, DEV, spoiled=True)
    Lf = ha.widened(Lh)
    out_h, lse_h = ha.forward(name, Lh)
    out_f, lse_f = ha.forward(name, Lf)
    g_h = Lh["gout"]
    grads_h = ha.backward(name, Lh, g_h, out_h, lse_h)
    grads_f = ha.backward(name, Lf, g_h.float(), out_h.float(), lse_h)
    return dict(Lh=Lh, out_h=out_h, lse_h=lse_h, out_f=out_f, lse_f=lse_f, grads_h=grads_h, grads_f=grads_f)


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", ha.BIT_CASES)
def test_forward_to_the_bit(name, dtname):
    """out has the bit patterns of the float32 operator's output on the widened leaves cast to the dtype (NaN rows
    included: float16 through the hardware convert both ways, bfloat16 the canonical quiet NaN both ways); lse is
    float32 with the float32 call's bit patterns."""
    r = run(name, dtname)
    dt = ha.DTYPES[dtname]
    c = R.CASES[name]
    assert r["out_h"].dtype == dt and r["lse_h"].dtype == torch.float32 and r["out_f"].dtype == torch.float32
    assert tuple(r["lse_h"].shape) == (2, c["G"] * c["M"])
    assert ha.same_bits(r["out_h"], r["out_f"].to(dt)), name
    assert ha.same_bits(r["lse_h"], r["lse_f"]), name
    dead = torch.from_numpy(R.build_inputs(name)["dead"].copy()).to(DEV)
    assert torch.equal(torch.isnan(r["out_h"]).any(-1), dead) and torch.equal(torch.isnan(r["out_h"]).all(-1), dead)


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", ha.BIT_CASES)
def test_backward_to_the_bit(name, dtname):
    """Every gradient has the bit patterns of the float32 backward operator's (on the widened upstream gradient,
    leaves and saved half output) cast to the dtype: the groups' dK / dV sums over several row tiles included,
    which must not pass through a half element.  An all-masked row's own gradient is exactly zero and its
    group's dK / dV are finite."""
    r = run(name, dtname)
    dt = ha.DTYPES[dtname]
    c, x = R.CASES[name], R.build_inputs(name)
    assert set(r["grads_h"]) == set(R.LEAVES[c["route"]])
    for n, got in r["grads_h"].items():
        assert got.dtype == dt and r["grads_f"][n].dtype == torch.float32
        if c["vbt"] and n == "v":
            continue  # (reduced on the host behind the kernel: test_value_broadcast_along_T_...)
        assert ha.same_bits(got, r["grads_f"][n].to(dt)), (name, n)
    if x["dead"].any():
        dead = torch.from_numpy(x["dead"].copy()).to(DEV)
        own = r["grads_h"]["q"][dead] if c["route"] == "dot" else r["grads_h"]["e"][:, dead]
        assert bool((own == 0).all()), "an all-masked row's own gradient is exactly 0"
        for n in ("k", "v"):
            if n in r["grads_h"]:
                assert bool(torch.isfinite(r["grads_h"][n]).all()), n


@pytest.mark.parametrize("dtname", DTNAMES)
def test_value_broadcast_along_T_is_summed_in_float32_and_rounded_once(dtname):
    """A value broadcast along T leaves a sum over T behind the kernel.  The kernel's elements are what the
    float32 kernel gives per frame (the float32 operator on the same value repeated along T, which plans
    alike) rounded to the dtype; the operator returns their float32 sum rounded once.  Held to the bit, as is the
    float32 route's own reduction, which stays float32 throughout."""
    name, dt = ha.VBT, ha.DTYPES[dtname]
    r = run(name, dtname)
    c = R.CASES[name]
    Lf = ha.widened(r["Lh"])
    assert Lf["v"].shape[0] == 1 and c["T"] > 1
    rep = dict(Lf, v=Lf["v"].expand(c["T"], -1, -1, -1).contiguous())
    out_rep, lse_rep = ha.forward(name, rep)
    assert ha.same_bits(out_rep, r["out_f"]) and ha.same_bits(lse_rep, r["lse_f"])
    per_frame = ha.backward(name, rep, r["Lh"]["gout"].float(), r["out_h"].float(), r["lse_h"])["v"]
    assert per_frame.shape[0] == c["T"]
    want = per_frame.to(dt).float().sum_to_size(Lf["v"].shape).to(dt)
    assert ha.same_bits(r["grads_h"]["v"], want)
    assert ha.same_bits(r["grads_f"]["v"], per_frame.sum_to_size(Lf["v"].shape))


@pytest.mark.parametrize("dtname", DTNAMES)
@pytest.mark.parametrize("name", ha.BOUND_CASES)
def test_forward_against_float64(name, dtname):
    """|out - ref| <= b + ulp_E(|ref| + b) / 2, b the suite's float32 bound, ref the float64 formula on the widened
    half leaves: the float32 kernels' bound plus one rounding (derived, not measured)."""
    r = run(name, dtname)
    dt = ha.DTYPES[dtname]
    c, x = R.CASES[name], R.build_inputs(name)
    L = ha.leaves(name, dt, "cpu")  # (the clean inputs: a spoiled frame is masked and reaches nothing)
    L64 = {n: t.double() if t is not None and t.is_floating_point() else t for n, t in L.items()}
    args = ha.operands(name, L64)
    ref = R.pool_ref(*args, L64["mask"], 0) if c["route"] == "pool" else R.attend_ref(*args, L64["mask"], 0, x["scale"])
    got = r["out_h"].double().cpu()
    ok = ~torch.isnan(ref)
    assert torch.equal(torch.isnan(got), ~ok)
    err, bound = (got - ref).abs()[ok], ha.forward_bound(ref, dt)[ok]
    worst = int(torch.argmax(err - bound)) if err.numel() else 0
    print("{} {}: max abs error {:.3e}; tightest element error {:.3e} of bound {:.3e}".format(
        name, dtname, float(err.max()) if err.numel() else 0.0, float(err[worst]) if err.numel() else 0.0,
        float(bound[worst]) if err.numel() else 0.0))  # fmt: skip
    assert bool((err <= bound).all()), (name, float(err[worst]), float(bound[worst]))


def _growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del keep
    return grown


def test_no_float32_copy_at_the_decode_shape():
    """Decode-shaped dot_attention on bfloat16 (query (64, 8, 256), key and value (512, 64, 1, 256), a length
    mask; the key is 16 MiB): one forward grows the peak by the output, lse and the plan's workspace at the most,
    the backward operator by the gradients, its workspace and the contiguous grad_out, each plus 1 MiB; the
    formula's first product alone is several times that (tests/test_half_attn_cpu.py)."""
    import pydrobert_amd.modules  # noqa: F401

    s, dt = ha.NOCOPY, torch.bfloat16
    N, K, T, D = s["N"], s["K"], s["T"], s["D"]
    torch.manual_seed(11)
    q = torch.randn(N, K, D, device=DEV).to(dt)
    k = torch.randn(T, N, 1, D, device=DEV).to(dt)
    v = torch.randn(T, N, 1, D, device=DEV).to(dt)
    assert k.numel() * k.element_size() == 16 * ha.MIB
    lens = torch.randint(T // 2, T + 1, (N,), device=DEV)
    mask = torch.arange(T, device=DEV).view(T, 1, 1) < lens.view(1, N, 1)
    g = torch.randn(N, K, D, device=DEV).to(dt)
    ops = torch.ops.pydrobert_amd
    fwd_allow, bwd_allow, formula = ha.nocopy_bytes(2)
    fwd = lambda: ops.dot_attention(q, k, v, mask, 0, D ** -0.5)  # noqa: E731
    out, lse = fwd()  # (warm-up: the library loads, the allocator settles)
    bwd = lambda: ops.dot_attention_backward(g, q, k, v, mask, out, lse, 0, D ** -0.5)  # noqa: E731
    bwd()
    for what, fn, allow in (("forward", fwd, fwd_allow), ("backward", bwd, bwd_allow)):
        grown = _growth(fn)
        print("{}: peak growth {} B, allowance {} B + 1 MiB, the formula's first product {} B".format(
            what, grown, allow, formula))  # fmt: skip
        assert grown <= allow + ha.MIB, (what, grown, allow)
    assert out.dtype == dt and lse.dtype == torch.float32 and all(x.dtype == dt for x in bwd())


def _no_formula(monkeypatch):
    from pydrobert_amd import _attn

    def refuse(*args, **kwargs):
        raise AssertionError("the torch formula was called")

    monkeypatch.setattr(_attn, "_softmax_pool", refuse)


@pytest.mark.parametrize("dtname", DTNAMES)
def test_modules_take_the_half_route(dtname, monkeypatch):
    """The four single-head modules on half tensors with the torch formula patched to raise: outputs equal the
    operators' results called directly; operands of mixed dtypes still reach the formula."""
    from pydrobert_amd import _attn
    from pydrobert_amd import modules as M

    dt = ha.DTYPES[dtname]
    torch.manual_seed(7)
    q = torch.randn(5, 3, 12, device=DEV).to(dt)
    k = torch.randn(9, 5, 1, 12, device=DEV).to(dt)
    v = torch.randn(9, 5, 1, 7, device=DEV).to(dt)
    lens = torch.tensor([9, 1, 4, 7, 2], device=DEV)
    mask = torch.arange(9, device=DEV).view(9, 1, 1) < lens.view(1, 5, 1)
    _no_formula(monkeypatch)
    ops = torch.ops.pydrobert_amd
    dot = M.DotProductSoftAttention(12, 0, 0.25)
    y = dot(q, k, v, mask)
    assert y.dtype == dt and ha.same_bits(y, ops.dot_attention(q, k, v, mask, 0, 0.25)[0])
    gen = M.GeneralizedDotProductSoftAttention(12, 12, 0, True).to(device=DEV, dtype=dt)
    y = gen(q, k, v, mask)
    assert y.dtype == dt and ha.same_bits(y, ops.dot_attention(gen._fused_query(q)[0], k, v, mask, 0, 1.0)[0])
    cat = M.ConcatSoftAttention(12, 12, 0, True, 6).to(device=DEV, dtype=dt)
    y = cat(q, k, v, mask)
    assert y.dtype == dt and ha.same_bits(y, ops.attention_pool(cat.score(q, k), v, mask, 0)[0])
    cos = cosine_attention()(12)
    y = cos(q, k, v, mask)
    assert y.dtype == dt and ha.same_bits(y, ops.attention_pool(cos.score(q, k), v, mask, 0)[0])
    # mixed dtypes: the formula (here the patch's error), for the fused scores and for a given score
    for bad in ((q.float(), k, v), (q, k, v.float()), (q.float(), k.float(), v)):
        with pytest.raises(AssertionError, match="the torch formula was called"):
            dot(*bad, mask)
    monkeypatch.undo()
    y = dot(q.float(), k.float(), v, mask)  # (and without the patch: the formula's own result)
    e = (q.float().unsqueeze(0) * k.float()).sum(-1) * 0.25
    assert torch.equal(y, _attn._softmax_pool(e, v, mask, 0))


def test_multi_headed_attention_under_autocast(monkeypatch):
    """MultiHeadedAttention with float32 parameters under torch.autocast("cuda", dtype=torch.bfloat16): its
    Linears hand bfloat16 heads to the fused operator (the formula is patched to raise), forward and backward;
    the parameter gradients are finite and float32."""
    from pydrobert_amd import modules as M

    torch.manual_seed(9)
    mha = M.MultiHeadedAttention(24, 24, 20, 4, M.DotProductSoftAttention(6, 0, 6 ** -0.5)).to(DEV)
    q = torch.randn(3, 11, 24, device=DEV, requires_grad=True)
    k = torch.randn(13, 3, 1, 24, device=DEV)
    v = torch.randn(13, 3, 1, 20, device=DEV)
    lens = torch.tensor([13, 5, 9], device=DEV)
    mask = torch.arange(13, device=DEV).view(13, 1, 1) < lens.view(1, 3, 1)
    seen = []
    real = torch.ops.pydrobert_amd.dot_attention

    def spy(query, key, value, *rest):
        seen.append((query.dtype, key.dtype, value.dtype))
        return real(query, key, value, *rest)

    from pydrobert_amd import _attn

    _no_formula(monkeypatch)
    monkeypatch.setattr(_attn, "dot_attention", lambda *a: spy(*a)[0])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = mha(q, k, v, mask)
    assert seen == [(torch.bfloat16,) * 3]
    assert y.dtype == torch.bfloat16 and bool(torch.isfinite(y).all())
    y.float().square().sum().backward()
    params = dict(mha.named_parameters())
    assert params and q.grad is not None and bool(torch.isfinite(q.grad).all())
    for n, p in params.items():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n


def test_opcheck_with_bfloat16_operands():
    """Schema, fake kernels and autograd registration of the four operators hold for bfloat16 operands."""
    import pydrobert_amd.modules  # noqa: F401
    from torch.library import opcheck

    torch.manual_seed(13)
    dt = torch.bfloat16
    q = torch.randn(3, 4, 5, device=DEV).to(dt).requires_grad_(True)
    k = torch.randn(7, 3, 1, 5, device=DEV).to(dt).requires_grad_(True)
    v = torch.randn(7, 3, 1, 6, device=DEV).to(dt).requires_grad_(True)
    e = torch.randn(7, 3, 4, device=DEV).to(dt).requires_grad_(True)
    mask = torch.arange(7, device=DEV).view(7, 1, 1) < torch.tensor([7, 3, 5], device=DEV).view(1, 3, 1)
    ops = torch.ops.pydrobert_amd
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    opcheck(ops.dot_attention.default, (q, k, v, mask, 0, 0.5), test_utils=utils)
    opcheck(ops.attention_pool.default, (e, v, mask, 0), test_utils=utils)
    with torch.no_grad():
        out, lse = ops.dot_attention(q, k, v, mask, 0, 0.5)
        pout, plse = ops.attention_pool(e, v, mask, 0)
    g = torch.randn(3, 4, 6, device=DEV).to(dt)
    qd, kd, vd, ed = (x.detach() for x in (q, k, v, e))
    opcheck(ops.dot_attention_backward.default, (g, qd, kd, vd, mask, out, lse, 0, 0.5),
            test_utils=("test_schema", "test_faketensor"))  # fmt: skip
    opcheck(ops.attention_pool_backward.default, (g, ed, vd, mask, pout, plse, 0),
            test_utils=("test_schema", "test_faketensor"))  # fmt: skip


@pytest.mark.parametrize("dtname", DTNAMES)
def test_empty_shapes(dtname):
    """R = 0 and T = 0 through the half operators: empty results and zeros, lse at -inf in float32; the backward
    returns zeros in the operands' shapes and dtype."""
    import pydrobert_amd.modules  # noqa: F401

    dt = ha.DTYPES[dtname]
    ops = torch.ops.pydrobert_amd
    for N, T in ((0, 5), (3, 0)):
        q = torch.zeros(N, 2, 4, device=DEV, dtype=dt)
        k = torch.zeros(T, N, 1, 4, device=DEV, dtype=dt)
        v = torch.ones(T, N, 1, 6, device=DEV, dtype=dt)
        e = torch.zeros(T, N, 2, device=DEV, dtype=dt)
        g = torch.ones(N, 2, 6, device=DEV, dtype=dt)
        for fwd, bwd, ins in ((ops.dot_attention, ops.dot_attention_backward, ((q, k, v, None), (0, 1.0))),
                              (ops.attention_pool, ops.attention_pool_backward, ((e, v, None), (0,)))):  # fmt: skip
            out, lse = fwd(*ins[0], *ins[1])
            assert (tuple(out.shape), out.dtype, tuple(lse.shape), lse.dtype) == ((N, 2, 6), dt, (2, 2 * N), torch.float32)
            assert bool((out == 0).all()) and bool(torch.isneginf(lse).all())
            grads = bwd(g, *ins[0], out, lse, *ins[1])
            for x, gx in zip(ins[0], grads):
                assert gx.shape == x.shape and gx.dtype == dt and bool((gx == 0).all())
