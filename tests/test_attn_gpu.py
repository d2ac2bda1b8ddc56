"""GPU: the attention modules on the HIP kernels -- the goldens (captured from the reference), random
broadcast patterns and strided inputs against the reference's formula in float64, gradcheck of both
operators, determinism, streams, no host synchronisation, and the route the modules take.

The sweeps, ``test_long_and_wide_against_formula`` and the decode shape have few groups, so their forward is
always split into spans of one 32-frame tile (with the combine pass); ``test_large_narrow_groups_against_formula``
runs the one-thread-per-row forward below one workgroup of rows.  Every other form the host plan can take is
reached by a named case of ``tests/_attn_ref.py`` (float64 formula, plan restatement, masks and tolerances
checked in ``test_attn_cpu.py``), run by the tests at the end of this file: several tiles per workgroup with
and without the combine, rows per tile set by LDS, value column blocks, key loop tails, the rows kernel's
instances and workgroups, the backward's frame chunks, empty spans, non-finite masked frames on every route,
scores at -inf, an all-masked row in a group, and shifted scores."""
import copy

import numpy as np
import pytest
import torch

import _attn_ref as R
from test_attn_cpu import check_case, cosine_attention, load_case, upstream  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn.npz"))


def reference_formula(m, query, key, value, mask):
    """The reference's forward restated in torch (_attn.py:212-223), any device."""
    from pydrobert_amd._attn import _softmax_pool

    return _softmax_pool(m.score(query, key), value, mask, m.dim)


def test_goldens_on_device(gold):
    for k in range(int(gold["case_n"])):
        m, ins, mask, spec = load_case(gold, k, DEV)
        check_case(gold, k, m, ins, mask, 1e-5, 1e-4)


def test_generalized_bias_gradient_is_zero_tensor():
    from pydrobert_amd import modules as M

    torch.manual_seed(0)
    m = M.GeneralizedDotProductSoftAttention(5, 6, 0, True).to(DEV)
    q, k, v = torch.randn(3, 5, device=DEV), torch.randn(7, 3, 6, device=DEV), torch.randn(7, 3, 4, device=DEV)
    m(q, k, v).sum().backward()
    assert m.bias.grad is not None and m.bias.grad.abs().max().item() < 1e-5
    assert m.weight.grad is not None


def _random_case(rng, dtype):
    """A random broadcast pattern: (leaves, (query, key, value), mask, dim).  Some operands are strided, some
    keys and values are expanded by the caller (stride 0 at full size), some masks are strided views."""
    nb = int(rng.integers(1, 4))  # batch dims besides T
    dim = int(rng.integers(0, nb + 1))
    full = [int(rng.integers(1, 5)) for _ in range(nb)]
    T = int(rng.integers(1, 70))
    D, Dv = int(rng.integers(1, 70)), int(rng.integers(1, 40))

    def shape(p_one):
        s = [1 if rng.random() < p_one else n for n in full]
        s.insert(dim, T)
        return s

    ks, vs = shape(0.4), shape(0.4)
    vs[dim] = T if rng.random() < 0.85 else 1
    qs = [1 if rng.random() < 0.3 else n for n in full]

    def make(s, last):
        x = torch.randn(*s, last * 2 if rng.random() < 0.3 else last, device=DEV, dtype=dtype)
        if x.shape[-1] != last:
            x = x[..., ::2]  # (a feature stride of 2)
        if x.dim() > 1 and rng.random() < 0.3:
            x = x.transpose(0, -2).contiguous().transpose(0, -2)  # (permuted strides)
        return x.requires_grad_(True)

    def expanded(x):
        """x with its size-1 batch dims expanded to full size (stride 0), as a caller may pass it"""
        if rng.random() >= 0.4:
            return x
        target = list(full)
        target.insert(dim, x.shape[dim])
        return x.expand(target + [x.shape[-1]])

    leaves = [make(qs, D), make(ks, D), make(vs, Dv)]
    used = [leaves[0], expanded(leaves[1]), expanded(leaves[2])]
    mask = None
    if rng.random() < 0.7:
        ms = shape(0.5)
        if rng.random() < 0.5:  # (a strided view: every other frame of a longer mask)
            big = list(ms)
            big[dim] = 2 * T
            mask = torch.from_numpy(rng.random(big) < 0.8).to(DEV)
            mask = mask[(slice(None),) * dim + (slice(None, None, 2),)]
            assert not mask.is_contiguous() or T == 1
        else:
            mask = torch.from_numpy(rng.random(ms) < 0.8).to(DEV)
        if rng.random() < 0.3:  # (expanded by the caller: stride 0 at full size)
            mask = mask.expand([n if i != dim else T for i, n in enumerate(full[:dim] + [T] + full[dim:])])
    return leaves, used, mask, dim


def test_random_broadcast_sweep_against_float64_formula():
    from pydrobert_amd import modules as M

    rng = np.random.default_rng(1234)
    for it in range(60):
        dtype = torch.float64 if it % 3 == 0 else torch.float32
        leaves, (q, k, v), mask, dim = _random_case(rng, dtype)
        scale = float(rng.uniform(0.1, 1.0))
        m = M.DotProductSoftAttention(q.shape[-1], dim, scale)
        y = m(q, k, v, mask)
        g = upstream(tuple(y.shape), dtype).to(DEV)
        grads = torch.autograd.grad(y, leaves, g)
        l64 = [x.detach().double().requires_grad_(True) for x in leaves]
        q64, k64, v64 = (u64.expand(u.shape) for u64, u in zip(l64, (q, k, v)))
        y64 = reference_formula(m, q64, k64, v64, mask)
        ok = ~torch.isnan(y64)
        assert torch.equal(torch.isnan(y), ~ok), it
        tol = 1e-9 if dtype == torch.float64 else 2e-5
        assert torch.allclose(y.double()[ok], y64[ok], rtol=tol, atol=tol), (it, (y.double() - y64)[ok].abs().max())
        if mask is not None and not bool(ok.all()):
            continue  # (the reference's gradients are NaN through an all-masked row)
        e64 = torch.autograd.grad(y64, l64, g.double())
        for name, a, b in zip("qkv", grads, e64):
            gt = 1e-8 if dtype == torch.float64 else 1e-4
            assert torch.allclose(a.double(), b, rtol=gt, atol=gt), (it, name, (a.double() - b).abs().max())


def test_pool_route_sweep_against_float64_formula():
    from pydrobert_amd import modules as M

    rng = np.random.default_rng(99)
    for it in range(20):
        leaves, (q, k, v), mask, dim = _random_case(rng, torch.float64)
        torch.manual_seed(it)
        m = M.ConcatSoftAttention(q.shape[-1], k.shape[-1], dim, bool(it % 2), 5).double().to(DEV)
        y = m(q, k, v, mask)
        y64 = reference_formula(m, q, k, v, mask)
        ok = ~torch.isnan(y64)
        assert torch.equal(torch.isnan(y), ~ok)
        assert torch.allclose(y[ok], y64[ok], rtol=1e-9, atol=1e-9), it
        if not bool(ok.all()):
            continue
        g = upstream(tuple(y.shape), torch.float64).to(DEV)
        ins = tuple(leaves) + (m.weight, m.v)
        for a, b in zip(torch.autograd.grad(y, ins, g), torch.autograd.grad(y64, ins, g)):
            assert torch.allclose(a, b, rtol=1e-8, atol=1e-8), it


def test_gradcheck_both_operators():
    from pydrobert_amd import _attn

    torch.manual_seed(0)
    opts = dict(device=DEV, dtype=torch.float64, requires_grad=True)
    q, k, v = torch.randn(3, 2, 5, **opts), torch.randn(7, 3, 1, 5, **opts), torch.randn(7, 3, 1, 4, **opts)
    mask = (torch.arange(7, device=DEV).view(7, 1, 1) < torch.tensor([7, 3, 5], device=DEV).view(1, 3, 1))
    assert torch.autograd.gradcheck(lambda a, b, c: _attn.dot_attention(a, b, c, mask, 0, 0.7), (q, k, v))
    e = torch.randn(7, 3, 2, **opts)
    assert torch.autograd.gradcheck(lambda a, c: _attn.attention_pool(a, c, mask, 0), (e, v))
    # double backward raises rather than returning a wrong value
    y = _attn.dot_attention(q, k, v, mask, 0, 0.7)
    (gq,) = torch.autograd.grad(y.sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gq.sum(), q)


@pytest.mark.parametrize("T,D,Dv,N,K", [(4096, 64, 64, 2, 3), (300, 2048, 2048, 2, 2), (1000, 16, 16, 16, 1)])
def test_long_and_wide_against_formula(T, D, Dv, N, K):
    from pydrobert_amd import modules as M

    torch.manual_seed(T + D)
    m = M.DotProductSoftAttention(D, 0, D ** -0.5)
    q = torch.randn(N, K, D, device=DEV, requires_grad=True)
    k = torch.randn(T, N, 1, D, device=DEV, requires_grad=True)
    v = torch.randn(T, N, 1, Dv, device=DEV, requires_grad=True)
    lens = torch.tensor([T, T // 3 + 1] + [T] * (N - 2), device=DEV)[:N]
    mask = torch.arange(T, device=DEV).view(T, 1, 1) < lens.view(1, N, 1)
    y = m(q, k, v, mask)
    g = torch.randn_like(y)
    grads = torch.autograd.grad(y, (q, k, v), g)
    q64, k64, v64 = (x.detach().double().requires_grad_(True) for x in (q, k, v))
    y64 = reference_formula(m, q64, k64, v64, mask)
    assert torch.allclose(y.double(), y64, rtol=1e-4, atol=1e-5), (y.double() - y64).abs().max()
    for a, b in zip(grads, torch.autograd.grad(y64, (q64, k64, v64), g.double())):
        assert torch.allclose(a.double(), b, rtol=1e-3, atol=1e-4), (a.double() - b).abs().max()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("D,Dv", [(16, 16), (7, 30), (32, 5)])
def test_large_narrow_groups_against_formula(dtype, D, Dv):
    """Many queries sharing one key sequence with narrow features (the one-thread-per-row forward), dot and
    pool routes, a causal mask, an all-masked query row and a caller-expanded key."""
    from pydrobert_amd import modules as M

    torch.manual_seed(D * 100 + Dv)
    Lq, N, T = 70, 3, 90
    q = torch.randn(Lq, N, D, device=DEV, dtype=dtype, requires_grad=True)
    k = torch.randn(T, 1, N, D, device=DEV, dtype=dtype, requires_grad=True)
    v = torch.randn(T, 1, N, Dv, device=DEV, dtype=dtype, requires_grad=True)
    mask = torch.arange(T, device=DEV).view(T, 1, 1) <= torch.arange(Lq, device=DEV).view(1, Lq, 1) + 5
    holed = mask.expand(T, Lq, N).clone()
    holed[:, 3, 1] = False  # (an all-masked query row: NaN, as in the reference)
    tol = (2e-5, 1e-4) if dtype == torch.float32 else (1e-9, 1e-8)
    mods = [M.DotProductSoftAttention(D, 0, D ** -0.5),
            M.ConcatSoftAttention(D, D, 0, True, 6).to(device=DEV, dtype=dtype)]  # fmt: skip
    for m in mods:
        m64 = copy.deepcopy(m).double()
        for key in (k, k.expand(T, Lq, N, D)):
            y = m(q, key, v, holed)
            y64 = reference_formula(m64, q.double(), key.double(), v.double(), holed)
            ok = ~torch.isnan(y64)
            assert torch.equal(torch.isnan(y), ~ok) and not bool(ok[3, 1].any())
            assert torch.allclose(y.double()[ok], y64[ok], rtol=tol[0], atol=tol[0]), type(m).__name__
            # gradients without the hole (the reference's are NaN through the whole group otherwise)
            y = m(q, key, v, mask)
            g = torch.randn_like(y)
            grads = torch.autograd.grad(y, (q, k, v), g)
            l64 = [x.detach().double().requires_grad_(True) for x in (q, k, v)]
            y64 = reference_formula(m64, l64[0], l64[1].expand(key.shape), l64[2], mask)
            assert torch.allclose(y.double(), y64, rtol=tol[0], atol=tol[0]), type(m).__name__
            for a, b in zip(grads, torch.autograd.grad(y64, l64, g.double())):
                assert torch.allclose(a.double(), b, rtol=tol[1], atol=tol[1]), (type(m).__name__, (a.double() - b).abs().max())


def test_masked_frames_contribute_exactly_zero():
    """The one deviation from the reference: a non-finite key or value in a masked frame does not reach the
    output or any gradient (the reference's 0 * inf gives NaN)."""
    from pydrobert_amd import modules as M

    torch.manual_seed(5)
    m = M.DotProductSoftAttention(6, 0)
    q = torch.randn(3, 6, device=DEV, requires_grad=True)
    k = torch.randn(8, 3, 6, device=DEV)
    v = torch.randn(8, 3, 4, device=DEV)
    lens = torch.tensor([8, 5, 2], device=DEV)
    mask = torch.arange(8, device=DEV).unsqueeze(1) < lens
    k_bad, v_bad = k.clone(), v.clone()
    k_bad[~mask] = float("inf")
    v_bad[~mask] = float("nan")
    k_bad.requires_grad_(True)
    v_bad.requires_grad_(True)
    y = m(q, k_bad, v_bad, mask)
    assert torch.isfinite(y).all()
    ref = torch.stack([reference_formula(m, q[n:n + 1], k[:l, n:n + 1], v[:l, n:n + 1], None)[0]
                       for n, l in enumerate(lens.tolist())])  # fmt: skip
    assert torch.allclose(y, ref, atol=1e-5)
    gq, gk, gv = torch.autograd.grad(y.sum(), (q, k_bad, v_bad))
    assert torch.isfinite(gq).all() and torch.isfinite(gk).all() and torch.isfinite(gv).all()
    assert bool((gk[~mask] == 0).all()) and bool((gv[~mask] == 0).all())


def _decode_inputs(seed=0):
    torch.manual_seed(seed)
    q = torch.randn(16, 8, 64, device=DEV, requires_grad=True)
    k = torch.randn(300, 16, 1, 64, device=DEV, requires_grad=True)
    v = torch.randn(300, 16, 1, 48, device=DEV, requires_grad=True)
    lens = torch.randint(1, 301, (16,), device=DEV)
    mask = torch.arange(300, device=DEV).view(300, 1, 1) < lens.view(1, 16, 1)
    return q, k, v, mask


def _run(m, q, k, v, mask, g):
    y = m(q, k, v, mask)
    return (y,) + torch.autograd.grad(y, (q, k, v), g)


def test_deterministic_and_second_stream():
    from pydrobert_amd import modules as M

    m = M.DotProductSoftAttention(64, 0, 0.125)
    q, k, v, mask = _decode_inputs()
    g = torch.randn(16, 8, 48, device=DEV)
    first = _run(m, q, k, v, mask, g)
    second = _run(m, q, k, v, mask, g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        third = _run(m, q, k, v, mask, g)
    torch.cuda.current_stream().wait_stream(s)
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_no_host_synchronisation():
    from pydrobert_amd import modules as M

    m_dot = M.GeneralizedDotProductSoftAttention(64, 64, 0, True).to(DEV)
    m_cat = M.ConcatSoftAttention(64, 64, 0, True, 16).to(DEV)
    q, k, v, mask = _decode_inputs(1)
    g = torch.randn(16, 8, 48, device=DEV)
    for m in (m_dot, m_cat):
        _run(m, q, k, v, mask, g)  # (warm: the library loads, the workspace allocator settles)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            _run(m, q, k, v, mask, g)
        finally:
            torch.cuda.set_sync_debug_mode(0)


def test_trace_graph_holds_the_fused_operators():
    from pydrobert_amd import modules as M

    q, k, v, mask = (x.detach() if x.dtype != torch.bool else x for x in _decode_inputs(2))
    for m, op in ((M.DotProductSoftAttention(64, 0), "pydrobert_amd::dot_attention"),
                  (M.GeneralizedDotProductSoftAttention(64, 64).to(DEV), "pydrobert_amd::dot_attention"),
                  (M.ConcatSoftAttention(64, 64, 0, False, 8).to(DEV), "pydrobert_amd::attention_pool"),
                  (cosine_attention()(64), "pydrobert_amd::attention_pool")):  # fmt: skip
        traced = torch.jit.trace(m, (q, k, v, mask))
        assert op in str(traced.graph), type(m).__name__
        assert torch.allclose(traced(q, k, v, mask), m(q, k, v, mask))
    # the multi-head module: its single head takes the fused route, the head axis one more broadcast dim
    mha = M.MultiHeadedAttention(64, 64, 48, 4, M.DotProductSoftAttention(16, 0, 0.25)).to(DEV)
    traced = torch.jit.trace(mha, (q, k, v, mask))  # (its mask gains the head axis itself)
    assert "pydrobert_amd::dot_attention" in str(traced.inlined_graph)
    # the scripted module takes the same route and agrees
    sm = torch.jit.script(M.DotProductSoftAttention(64, 0))
    assert torch.allclose(sm(q, k, v, mask), M.DotProductSoftAttention(64, 0)(q, k, v, mask))


def test_compile_on_device():
    from pydrobert_amd import modules as M

    torch._dynamo.reset()
    m = M.DotProductSoftAttention(64, 0, 0.125)
    q, k, v, mask = _decode_inputs(3)
    comp = torch.compile(m, backend="eager", fullgraph=True)
    g = torch.randn(16, 8, 48, device=DEV)
    for a, b in zip(_run(comp, q, k, v, mask, g), _run(m, q, k, v, mask, g)):
        assert torch.allclose(a, b, atol=1e-6)


# ----------------------------------------------------------------------------------------------------------
# the named cases of tests/_attn_ref.py: output, NaN pattern and every gradient against the float64 formula


def _hip_case(name, spoiled=False):
    """Runs a case on the kernels (the operators called directly, the mask as it is) and compares."""
    from pydrobert_amd import _attn

    c = R.CASES[name]
    dtype = torch.float32 if c["dtype"] == "float32" else torch.float64
    out, grads = R.run_case(name, _attn.dot_attention, _attn.attention_pool, dtype, DEV, spoiled=spoiled, dropped=False)
    R.compare(name, out, grads)
    return out, grads


@pytest.mark.parametrize("name", R.cases_of("walk"))
def test_forward_walks_several_tiles_per_workgroup(name):
    """attn_fwd_kernel over more than one 32-frame tile per workgroup: the online-softmax carry (m_old, alpha,
    the rescaled sum and accumulators).  1100 groups: splits 1, span 96, tiles of 32 + 32 + 6 frames, with scores
    rising (a new maximum per tile, alpha < 1), falling (alpha = 1), flat at -1e4, the first tile masked for a
    third of the rows (m_old = -inf), the middle tile masked for all (skipped) and one all-masked row (NaN).
    300 groups over T = 250: 4 spans of 64 (the last of 58), the carry and the combine together.  The control
    (130 groups of 9 rows) has one tile per span."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("lds"))
def test_rows_per_tile_set_by_lds(name):
    """attn_rows_per_tile below 8 by LDS with several row tiles: forward rt 7 (7 + 2 rows) and rt 1; a backward
    whose tile (rt 7 at 56000 bytes, rt 3) differs from the forward's, dK / dV accumulated across its tiles;
    the pool backward at rt 7.  Causal masks: every row of a tile has its own limit."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("cols"))
def test_value_column_blocks(name):
    """grid.z over value columns: Dv 1024 / 1025 / 1300 / 2049 (1 / 2 / 2 / 3 blocks, the last partial) with
    split T, float32 and float64, dot and pool; Dv 1300 over 600 groups: two blocks, unsplit."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("keys"))
def test_key_loop_tails(name):
    """The forward's key loop (four loads of 64 in flight: D strided by 256) and the backward's (by 64) at
    D 1, 63, 64, 65, 255, 256, 257, 300 and 513."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("rows"))
def test_rows_kernel_forms(name):
    """attn_fwd_rows_kernel: 600 rows in three workgroups (the last partial, a wave across the group boundary,
    an all-masked row), the 16-row threshold, the 16 and 32 instances (Dv 17, D 32, D = Dv = 1), dot and pool,
    a strided query, T = 2000; M = 15 and D = 33 take the tiles (controls)."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("chunks"))
def test_backward_frame_chunk_forms(name):
    """The backward at T 1, 31, 32 (one chunk: dQ written directly), 33, 64, 65 (attn_gq_combine_kernel), groups
    of 1, 8, 9 and 17 rows, R = 1, 3, 5 rows for the delta kernel's partial workgroup, dot and pool, a value
    broadcast along T, a key and value expanded by the caller."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("spans"))
def test_split_partials_with_empty_spans(name):
    """Split partials of rows that attend nothing in the first span, nothing in the last span, and nothing at
    all (NaN through the combine): outputs, the NaN pattern and the gradients of the rows that attend."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("bad"))
def test_masked_non_finite_frames_in_every_route(name):
    """The deviation (inf keys and NaN values in masked frames reach nothing) in a group of 9 rows that mask
    differently, the rows kernel, the pool route (a non-finite score at every masked (row, frame) too),
    splits == 1 and span > 32.  A key or value is shared by its group, so the spoiled frames are those no row
    of the group attends.  Reference: the float64 formula on the clean inputs."""
    out, grads = _hip_case(name, spoiled=True)
    c, x = R.CASES[name], R.build_inputs(name)
    assert bool(torch.isfinite(out).all())
    unseen = torch.from_numpy(~x["mask"].any(2)).to(DEV)
    assert bool((grads["v"][unseen] == 0).all())
    if c["route"] == "dot":
        assert bool((grads["k"][unseen] == 0).all())
    else:
        assert bool((grads["e"][torch.from_numpy(~x["mask"]).to(DEV)] == 0).all())


@pytest.mark.parametrize("name", R.cases_of("neginf"))
def test_pool_scores_at_minus_infinity(name):
    """attention_pool with -inf in the score itself, unmasked (the x == -inf branches of the tile and the rows
    kernel): equal to the formula, grad_score exactly 0 there and finite elsewhere."""
    out, grads = _hip_case(name)
    e = torch.from_numpy(R.build_inputs(name)["e"].copy()).to(DEV)
    assert bool((grads["e"][torch.isneginf(e)] == 0).all()) and bool(torch.isfinite(grads["e"]).all())


@pytest.mark.parametrize("name", R.cases_of("dead"))
def test_all_masked_row_leaves_its_group_alone(name):
    """One row of a group of 9 / 70 (rows kernel forward) masked everywhere: its output is NaN, every gradient
    is finite, its own dQ (dE) is exactly 0, and dK / dV equal the reference computed without that row."""
    _hip_case(name)


@pytest.mark.parametrize("name", R.cases_of("shift"))
def test_shifted_scores(name):
    """Every score of a row shifted by 0, 10 and 100 (float32, tiles and rows forward): the backward rebuilds
    a = exp(score - lse) from one stored float.  Bounds: max(suite, 8 x the float32 formula's own error)."""
    _hip_case(name)
