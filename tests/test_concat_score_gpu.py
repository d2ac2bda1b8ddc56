"""GPU: the fused ConcatSoftAttention score (``pydrobert_amd::concat_score``, csrc/concat_score.hip) in every plan form
and layout of tests/_concat_ref.py against the float64 formula, at saturation, under gradcheck, run to run, without
a hidden-sized intermediate, without host synchronisation, under trace and compile, and beyond 2^32 element offsets."""
import pytest
import torch

import _concat_ref as R
import _wide as W

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _op(wq, wk, v, dim):
    return torch.ops.pydrobert_amd.concat_score(wq, wk, v, dim)


def _check(name):
    """The operator fed wq and wk directly, then the module's own score(): e and the gradients of wq, wk, v, weight
    and bias against the float64 formula."""
    from pydrobert_amd import modules as M

    c = R.CASES[name]
    dtype = torch.float32 if c["dtype"] == "float32" else torch.float64
    got = R.run_case(name, _op, dtype, DEV)
    R.compare(name, got)
    if c["view"] is None:  # (a view is the operator's business: the module forms wk itself)
        t = R.tensors(name, dtype, DEV)
        m = M.ConcatSoftAttention(R.DQ, R.DK, c["dim"], True, c["H"]).to(device=DEV, dtype=dtype)
        with torch.no_grad():
            m.weight.copy_(t["weight"]), m.bias.copy_(t["bias"]), m.v.copy_(t["v"])
        e = m.score(t["query"], t["key"])
        gw, gb, gv = torch.autograd.grad(e, (m.weight, m.bias, m.v), t["gout"])
        R.compare(name, dict(got, e=e.detach(), weight=gw, bias=gb, v=gv), log=lambda s: print("module " + s))


@pytest.mark.parametrize("name", R.cases_of("hidden"))
def test_hidden_sizes(name):
    _check(name)


@pytest.mark.parametrize("name", R.cases_of("group"))
def test_group_sizes(name):
    _check(name)


@pytest.mark.parametrize("name", R.cases_of("lds"))
def test_rows_per_tile_set_by_lds(name):
    _check(name)


@pytest.mark.parametrize("name", R.cases_of("frames"))
def test_frames_and_backward_chunks(name):
    _check(name)


@pytest.mark.parametrize("name", R.cases_of("fill"))
def test_frames_per_workgroup(name):
    _check(name)


@pytest.mark.parametrize("name", R.cases_of("layout"))
def test_layouts(name):
    _check(name)


def test_expanded_key_keeps_one_gradient_slice_per_index():
    c = R.CASES["expanded"]
    t = R.tensors("expanded", torch.float32, DEV)
    wq, wk = (x.detach() for x in R.halves("expanded", t))
    S, _, _ = R.geometry(c)
    seen = R.as_seen("expanded", wk, S)
    assert seen.stride(2) == 0 and seen.shape[2] == 3
    _, gk, _ = torch.ops.pydrobert_amd.concat_score_backward(t["gout"], wq, seen, t["v"].detach(), 0)
    ref = R.expected("expanded")["wk"]
    assert gk.shape == ref.shape == seen.shape
    assert not torch.equal(gk[:, :, 0], gk[:, :, 1])
    assert torch.allclose(gk.double().cpu(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_saturation_is_exact(dtype):
    """|wq + wk| of 50 and more, 1e4 and inf: tanh is exactly +-1, so e is the signed sum of v, finite, and nothing
    reaches grad_wq or grad_wk; grad_v is the signed sum of the upstream gradient."""
    torch.manual_seed(11)
    N, K, T, H = 2, 3, 5, 70
    big = torch.tensor([51.0, -51.0, 1e4, -1e4, float("inf"), -float("inf")], dtype=dtype)
    wq = big[torch.randint(0, 6, (1, N, K, H))].to(DEV).requires_grad_(True)
    wk = (torch.rand(T, N, 1, H, dtype=dtype) * 2 - 1).to(DEV).requires_grad_(True)
    v = torch.randn(H, dtype=dtype, device=DEV, requires_grad=True)
    assert float((wq + wk).abs().min()) >= 50
    e = _op(wq, wk, v, 0)
    g = torch.randn_like(e)
    gq, gk, gv = torch.autograd.grad(e, (wq, wk, v), g)
    sign = torch.sign(wq.detach()).double()
    assert torch.isfinite(e).all()
    want = (sign * v.detach().double()).sum(-1).expand(T, N, K)
    tol = R.SUITE["float32" if dtype == torch.float32 else "float64"]
    assert torch.allclose(e.double(), want, rtol=tol[0], atol=tol[0]), (e.double() - want).abs().max()
    assert bool((gq == 0).all()) and bool((gk == 0).all())
    want_v = (g.double().unsqueeze(-1) * sign).sum((0, 1, 2))
    assert torch.allclose(gv.double(), want_v, rtol=tol[1], atol=tol[1]), (gv.double() - want_v).abs().max()


def test_tiny_arguments_hold_the_bound():
    """|x| near 1e-6, where 1 - 2 / (exp(2 x) + 1) would cancel: with v near 1e5 the score is of order 1 and the
    suite's float32 bound is a relative one of 1e-5."""
    torch.manual_seed(12)
    N, K, T, H = 2, 3, 5, 70
    wq = ((torch.rand(1, N, K, H, dtype=torch.float64) + 0.5) * 1e-6).float()
    wk = ((torch.rand(T, N, 1, H, dtype=torch.float64) - 0.5) * 1e-6).float()
    v = (torch.randn(H, dtype=torch.float64) * 1e5).float()
    g = torch.randn(T, N, K)
    leaves = [x.to(DEV).requires_grad_(True) for x in (wq, wk, v)]
    e = _op(*leaves, 0)
    grads = torch.autograd.grad(e, leaves, g.to(DEV))
    e64 = R.score_ref(wq.double(), wk.double(), v.double())
    assert float(e64.abs().median()) > 0.1
    assert torch.allclose(e.double().cpu(), e64, rtol=2e-5, atol=2e-5), (e.double().cpu() - e64).abs().max()
    # the gradients are of order 1e5 (grad_wq, grad_wk) and 1e-6 (grad_v): relative bounds
    for got, ref in zip(grads, R.grads_ref(g.double(), wq.double(), wk.double(), v.double())):
        assert torch.allclose(got.double().cpu(), ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))


EMPTY = {  # name -> (shape of wq, shape of wk): a batch dim, a group dim, the attended axis, the hidden axis of size 0
    "batch": ((1, 0, 3, 7), (5, 0, 1, 7)),
    "beams": ((1, 2, 0, 7), (5, 2, 1, 7)),
    "frames": ((1, 2, 3, 7), (0, 2, 1, 7)),
    "hidden": ((1, 2, 3, 0), (5, 2, 1, 0)),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("which", sorted(EMPTY))
def test_zero_sizes_through_the_operator(which, dtype):
    """Nothing is launched: an empty score for an empty batch, group or attended axis, zeros for no hidden units,
    and zero gradients of the inputs' shapes, as the torch body gives."""
    from pydrobert_amd import _attn

    qs, ks = EMPTY[which]
    wq = torch.randn(qs, device=DEV, dtype=dtype, requires_grad=True)
    wk = torch.randn(ks, device=DEV, dtype=dtype, requires_grad=True)
    v = torch.randn(qs[-1], device=DEV, dtype=dtype, requires_grad=True)
    assert _attn._concat_hip_route(wq, wk, v, 0)
    want = _attn._concat_score_torch(wq, wk, v)
    for e in (_op(wq, wk, v, 0), _attn.concat_score(wq.detach(), wk.detach(), v.detach(), 0)):
        assert e.shape == want.shape and e.dtype == dtype and torch.equal(e.detach(), want.detach())
    e = _op(wq, wk, v, 0)
    g = torch.ones_like(e)
    grads = torch.autograd.grad(e, (wq, wk, v), g)
    direct = torch.ops.pydrobert_amd.concat_score_backward(g, wq.detach(), wk.detach(), v.detach(), 0)
    for got, also, ref in zip(grads, direct, torch.autograd.grad(want, (wq, wk, v), g)):
        assert got.shape == ref.shape and torch.equal(got, ref) and torch.equal(also, ref)
        assert not bool(got.any())


@pytest.mark.parametrize("which", ["batch", "beams", "frames"])
def test_zero_sizes_through_the_module(which):
    from pydrobert_amd import _attn
    from pydrobert_amd import modules as M

    torch.manual_seed(19)
    N, K, T = (0, 3, 5) if which == "batch" else (2, 0, 5) if which == "beams" else (2, 3, 0)
    m = M.ConcatSoftAttention(4, 6, 0, True, 7).to(DEV)
    q = torch.randn(N, K, 4, device=DEV, requires_grad=True)
    k = torch.randn(T, N, 1, 6, device=DEV, requires_grad=True)
    value = torch.randn(T, N, 1, 5, device=DEV)
    e = m.score(q, k)
    assert e.shape == (T, N, K) and e.numel() == 0
    out = m(q, k, value)
    assert out.shape == (N, K, 5) and not bool(out.any())
    grads = torch.autograd.grad(out.sum() + m.score(q, k).sum(), (q, k, m.weight, m.bias, m.v))
    for g, x in zip(grads, (q, k, m.weight, m.bias, m.v)):
        assert g.shape == x.shape and not bool(g.any())
    # the torch body on the same inputs: the same empty score
    wq = torch.nn.functional.linear(q.unsqueeze(0), m.weight[:, :4], m.bias)
    wk = torch.nn.functional.linear(k, m.weight[:, 4:], None)
    assert torch.equal(e, _attn._concat_score_torch(wq, wk, m.v))


def test_tensors_on_different_devices_take_the_torch_body():
    """The route asks for one device; otherwise the torch body runs and raises torch's own error."""
    from pydrobert_amd import _attn

    wq, wk, v = torch.randn(1, 2, 3, 7, device=DEV), torch.randn(5, 2, 1, 7), torch.randn(7, device=DEV)
    assert not _attn._concat_hip_route(wq, wk, v, 0) and not _attn._concat_hip_route(wq, wk.to(DEV), v.cpu(), 0)
    assert _attn._concat_hip_route(wq, wk.to(DEV), v, 0)
    with pytest.raises(RuntimeError, match="same device"):
        _attn._concat_score(torch.randn(2, 3, 4, device=DEV), torch.randn(5, 2, 1, 6), torch.randn(7, 10, device=DEV),
                            None, v, 0)  # fmt: skip


def test_nan_propagates():
    wq = torch.zeros(1, 2, 3, 9, device=DEV)
    wk = torch.zeros(4, 2, 1, 9, device=DEV)
    wk[1, 0, 0, 5] = float("nan")
    e = _op(wq, wk, torch.ones(9, device=DEV), 0)
    assert torch.isnan(e[1, 0]).all() and int(torch.isnan(e).sum()) == 3


def test_gradcheck_and_double_backward():
    from pydrobert_amd import modules as M

    torch.manual_seed(13)
    wq = torch.randn(1, 2, 2, 4, dtype=torch.float64, device=DEV, requires_grad=True)
    wk = torch.randn(3, 2, 1, 4, dtype=torch.float64, device=DEV, requires_grad=True)
    v = torch.randn(4, dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b, c: _op(a, b, c, 0), (wq, wk, v), atol=1e-7)
    m = M.ConcatSoftAttention(3, 2, 0, True, 4).to(device=DEV, dtype=torch.float64)
    q = torch.randn(2, 2, 3, dtype=torch.float64, device=DEV, requires_grad=True)
    k = torch.randn(3, 2, 1, 2, dtype=torch.float64, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(m.score, (q, k), atol=1e-7)
    assert torch.autograd.gradgradcheck(m.score, (q, k), atol=1e-6)
    # the whole module's double backward still raises, through attention_pool
    value = torch.randn(3, 2, 1, 5, dtype=torch.float64, device=DEV)
    (gq,) = torch.autograd.grad(m(q, k, value).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError, match="double backward"):
        gq.sum().backward()


def _decode(seed, N=4, K=8, T=70, H=130):
    torch.manual_seed(seed)
    return (
        torch.randn(1, N, K, H, device=DEV, requires_grad=True), torch.randn(T, N, 1, H, device=DEV, requires_grad=True),
        torch.randn(H, device=DEV, requires_grad=True), torch.randn(T, N, K, device=DEV),
    )  # fmt: skip


def _run(wq, wk, v, g):
    e = _op(wq, wk, v, 0)
    return (e,) + torch.autograd.grad(e, (wq, wk, v), g)


def test_deterministic_and_second_stream():
    args = _decode(14)  # (three backward chunks: the combine passes run)
    first = _run(*args)
    second = _run(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        third = _run(*args)
    torch.cuda.current_stream().wait_stream(s)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_no_intermediate():
    """T = 64, N = 8, K = 8, H = 1000: the hidden-sized tensor would be 16 MiB.  One warm forward of the operator
    allocates e and nothing else (bytes(e) + the plan's workspace + 1 MiB); score(), which forms wq and wk with its
    two linears first, allocates those two besides (on an MI355X: the operator grew the peak by 16 384 bytes
    against a bound of 1 064 960; score() by 2 320 384, of which wq is 256 000 and wk 2 048 000; the torch body by
    more than 15 times the bound)."""
    from pydrobert_amd import _attn, _cabi
    from pydrobert_amd import modules as M

    T, N, K, H, D = 64, 8, 8, 1000, 16
    torch.manual_seed(15)
    m = M.ConcatSoftAttention(D, D, 0, True, H).to(DEV)
    q, k = torch.randn(N, K, D, device=DEV), torch.randn(T, N, 1, D, device=DEV)
    MiB = 1 << 20
    assert T * N * K * H * 4 >= 15 * MiB

    def growth(fn):
        fn()  # (warm)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    with torch.no_grad():
        wq = torch.nn.functional.linear(q.unsqueeze(0), m.weight[:, :D], m.bias)
        wk = torch.nn.functional.linear(k, m.weight[:, D:], None)
        plan = _attn._ConcatPlan(wq, wk, m.v, 0)
        ws = _cabi.lib().pdt_concat_score_workspace_bytes(plan.desc.data_ptr(), 0, 0)
        grown, e = growth(lambda: _attn.concat_score(wq, wk, m.v, 0))
        bound = e.numel() * 4 + ws + MiB
        print("operator: grew {} bytes, bound {}".format(grown, bound))
        assert ws == 0 and grown <= bound
        grown, e2 = growth(lambda: m.score(q, k))
        print("score(): grew {} bytes, bound {} + wq {} + wk {}".format(grown, bound, wq.numel() * 4, wk.numel() * 4))
        assert grown <= bound + (wq.numel() + wk.numel()) * 4
        assert torch.equal(e, e2)
        # what the condition rules out: the torch body at the same shape passes it 15-fold
        grown, e3 = growth(lambda: _attn._concat_score_torch(wq, wk, m.v))
        assert grown >= 15 * bound and torch.allclose(e, e3, rtol=2e-5, atol=2e-5)


def test_no_host_synchronisation():
    args = _decode(16)
    _run(*args)  # (warm: the library loads, the allocator settles)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run(*args)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_compile_and_trace_hold_the_operator():
    from pydrobert_amd import modules as M

    torch.manual_seed(17)
    m = M.ConcatSoftAttention(6, 5, 0, True, 33).to(DEV)
    q = torch.randn(3, 4, 6, device=DEV)
    k, value = torch.randn(40, 3, 1, 5, device=DEV), torch.randn(40, 3, 1, 7, device=DEV)
    mask = torch.arange(40, device=DEV).view(40, 1, 1) < torch.tensor([40, 7, 23], device=DEV).view(1, 3, 1)
    with torch.no_grad():
        want = m(q, k, value, mask)
        traced = torch.jit.trace(m, (q, k, value, mask))
        graph = str(traced.graph)
        assert "pydrobert_amd::concat_score" in graph and "pydrobert_amd::attention_pool" in graph
        assert "aten::tanh" not in graph
        assert torch.allclose(traced(q, k, value, mask), want, rtol=1e-6, atol=1e-6)
        assert torch.allclose(torch.jit.script(m)(q, k, value, mask), want, rtol=1e-6, atol=1e-6)
    torch._dynamo.reset()
    codes = []

    def recording(gm, example_inputs):  # (the eager backend, which also keeps the captured graph's code)
        codes.append(gm.code)
        return gm.forward

    with torch.no_grad():
        assert torch.allclose(torch.compile(m, backend=recording, fullgraph=True)(q, k, value, mask), want, rtol=1e-6, atol=1e-6)
    assert len(codes) == 1 and "pydrobert_amd.concat_score" in codes[0] and "pydrobert_amd.attention_pool" in codes[0]
    assert "tanh" not in codes[0]
    torch._dynamo.reset()
    comp = torch.compile(m, backend="eager", fullgraph=True)
    ql, kl = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    g = torch.randn_like(want)
    y = comp(ql, kl, value, mask)
    got = torch.autograd.grad(y, (ql, kl, m.weight, m.v), g)
    ref = torch.autograd.grad(m(ql, kl, value, mask), (ql, kl, m.weight, m.v), g)
    assert torch.allclose(y.detach(), want, rtol=1e-6, atol=1e-6)
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_offsets_beyond_32_bits():
    """wk is a view of one never-filled buffer with batch element 1 beyond 2^32 elements and decoys where a 32-bit
    wrap of its offsets lands (tests/_wide.py): e and the three gradients against the float64 formula."""
    try:
        buf = torch.empty(W.MIN_NUMEL, dtype=torch.float32, device=DEV)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip("no room for the {} GiB buffer: {}".format(W.MIN_NUMEL * 4 >> 30, e))
    try:
        _wide_case(buf)
    finally:
        del buf
        torch.cuda.empty_cache()


def _wide_case(buf):
    w = R.WIDE
    T, N, K, H = w["T"], w["N"], w["K"], w["H"]
    torch.manual_seed(18)
    wk0 = torch.randn(T, N, 1, H)
    wq0, v0, g0 = torch.randn(1, N, K, H), torch.randn(H), torch.randn(T, N, K)
    wk = W.wide_view(buf, wk0, w["wide_dim"]).requires_grad_(True)
    assert wk.stride(1) > W.WRAP
    wq, v = wq0.to(DEV).requires_grad_(True), v0.to(DEV).requires_grad_(True)
    e = _op(wq, wk, v, 0)
    grads = torch.autograd.grad(e, (wq, wk, v), g0.to(DEV))
    e64 = R.score_ref(wq0.double(), wk0.double(), v0.double())
    assert torch.allclose(e.double().cpu(), e64, rtol=2e-5, atol=2e-5), (e.double().cpu() - e64).abs().max()
    for got, ref in zip(grads, R.grads_ref(g0.double(), wq0.double(), wk0.double(), v0.double())):
        assert got.shape == ref.shape
        assert torch.allclose(got.double().cpu(), ref, rtol=1e-4, atol=1e-4), (got.double().cpu() - ref).abs().max()
