"""CPU: the attention modules without a GPU -- the reference's signatures, constants, state dicts, seeded
initialisation, error types, the torch body against the goldens (tests/golden/attn.npz, captured from the
reference), scripting, tracing and compiling, and the C entry points' argument checks."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "attn.npz"))


def upstream(shape, dtype):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


def _params(fn):
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name,
             repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]  # fmt: skip


def cosine_attention():
    from pydrobert_amd import modules as M

    class CosineAttention(M.GlobalSoftAttention):
        """A user subclass with its own score (the golden script defines the same one)."""

        def __init__(self, size: int, dim: int = 0):
            super().__init__(size, size, dim)

        def score(self, query: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
            query = query.unsqueeze(self.dim)
            return 3.0 * torch.nn.functional.cosine_similarity(query, key, dim=-1)

    return CosineAttention


def build(spec):
    from pydrobert_amd import modules as M

    kind, args = spec["module"], spec["args"]
    if kind == "MultiHeadedAttention":
        return M.MultiHeadedAttention(*args, single_head_attention=build(spec["head"]), **spec.get("kw", {}))
    cls = cosine_attention() if kind == "CosineAttention" else getattr(M, kind)
    return cls(*args)


def load_case(gold, k, device="cpu"):
    """(module, inputs, mask, spec) of golden case k, the reference's parameters loaded (strict)."""
    pre = "case_{}_".format(k)
    spec = json.loads(str(gold[pre + "spec"]))
    dtype = getattr(torch, spec.get("dtype", "float64"))
    m = build(spec).to(dtype)
    state = {n[len(pre + "param_"):]: torch.from_numpy(gold[n]) for n in gold.files if n.startswith(pre + "param_")}
    m.load_state_dict(state, strict=True)
    m = m.to(device)
    ins = [torch.from_numpy(gold[pre + n]).to(device).requires_grad_(True) for n in ("query", "key", "value")]
    mask = torch.from_numpy(gold[pre + "mask"]).to(device) if pre + "mask" in gold.files else None
    return m, ins, mask, spec


def check_case(gold, k, m, ins, mask, out_tol, grad_tol):
    """Output and every gradient against golden case k; NaN in the same places as the reference's output."""
    pre = "case_{}_".format(k)
    y = m(*ins, mask)
    exp = gold[pre + "out"]
    got = y.detach().cpu().numpy()
    assert got.shape == exp.shape, k
    assert np.array_equal(np.isnan(got), np.isnan(exp)), k
    fin = ~np.isnan(exp)
    assert np.allclose(got[fin], exp[fin], rtol=out_tol, atol=out_tol), (k, np.abs(got[fin] - exp[fin]).max())
    if y.numel() == 0:
        return
    params = dict(m.named_parameters())
    grads = torch.autograd.grad(y, ins + list(params.values()), upstream(tuple(y.shape), y.dtype).to(y.device),
                                allow_unused=True)  # fmt: skip
    for name, g in zip(["query", "key", "value"] + list(params), grads):
        key = pre + "grad_" + name
        if key not in gold.files:
            continue
        exp = gold[key]
        got = (torch.zeros_like(params[name]) if g is None else g).detach().cpu().numpy()
        fin = np.isfinite(exp)  # (an all-masked row: the reference's gradients through it are NaN)
        assert got.shape == exp.shape, (k, name)
        assert np.allclose(got[fin], exp[fin], rtol=grad_tol, atol=grad_tol), (k, name, np.abs(got[fin] - exp[fin]).max())


NAMES = ("GlobalSoftAttention", "DotProductSoftAttention", "GeneralizedDotProductSoftAttention",
         "ConcatSoftAttention", "MultiHeadedAttention")


def test_signatures_constants_and_repr_match_reference():
    from pydrobert_amd import modules as M

    sig = json.load(open(os.path.join(GOLD, "attn_signatures.json")))["modules"]
    samples = {
        "DotProductSoftAttention": M.DotProductSoftAttention(4, 1, 0.5),
        "GeneralizedDotProductSoftAttention": M.GeneralizedDotProductSoftAttention(3, 4, 1, True),
        "ConcatSoftAttention": M.ConcatSoftAttention(3, 4, 0, True, 9),
        "MultiHeadedAttention": M.MultiHeadedAttention(6, 5, 4, 2, M.GeneralizedDotProductSoftAttention(3, 2),
                                                       bias_WQ=True, bias_WC=True),
    }  # fmt: skip
    for name in NAMES:
        cls, exp = getattr(M, name), sig[name]
        for meth in ("__init__", "forward", "score", "check_input"):
            assert _params(getattr(cls, meth)) == exp[meth], (name, meth)
        assert list(cls.__constants__) == exp["__constants__"], name
        if name in samples:
            assert samples[name].extra_repr() == exp["extra_repr"], name
            assert sorted(samples[name].state_dict()) == exp["state_dict"], name


def test_seeded_parameters_bit_identical(gold):
    from pydrobert_amd import modules as M

    specs = {
        "gen": lambda: M.GeneralizedDotProductSoftAttention(5, 6, 0, True),
        "gen_nobias": lambda: M.GeneralizedDotProductSoftAttention(5, 6),
        "cat": lambda: M.ConcatSoftAttention(5, 6, 0, True, 9),
        "cat_nobias": lambda: M.ConcatSoftAttention(5, 6),
        "mha": lambda: M.MultiHeadedAttention(6, 5, 4, 2, M.GeneralizedDotProductSoftAttention(3, 2, 0, True),
                                              bias_WQ=True),
    }  # fmt: skip
    assert sorted(json.loads(str(gold["seed_tags"]))) == sorted(specs)
    for tag, make in specs.items():
        torch.manual_seed(7)
        m = make()
        for stage in ("init", "reset"):
            if stage == "reset":
                m.reset_parameters()
            for name, p in m.state_dict().items():
                assert torch.equal(p, torch.from_numpy(gold["seed_{}_{}_{}".format(tag, stage, name)])), (tag, stage, name)


def test_multi_head_bias_quirk():
    from pydrobert_amd import modules as M

    m = M.MultiHeadedAttention(4, 4, 4, 2, M.DotProductSoftAttention(2), bias_WK=True, bias_WV=True)
    assert m.WK.bias is None and m.WV.bias is None  # (bias_WQ decides, as in the reference)
    m = M.MultiHeadedAttention(4, 4, 4, 2, M.DotProductSoftAttention(2), bias_WQ=True)
    assert m.WK.bias is not None and m.WV.bias is not None and m.WC.bias is None


def test_error_types(gold):
    from pydrobert_amd import modules as M

    errors = json.loads(str(gold["errors"]))
    q, k, v = torch.randn(3, 4), torch.randn(5, 3, 4), torch.randn(5, 3, 2)
    dot = M.DotProductSoftAttention(4)
    mha = M.MultiHeadedAttention(4, 4, 2, 2, M.DotProductSoftAttention(2))
    cases = {
        "query_ndim": lambda: dot(torch.randn(4), k, v),
        "value_ndim": lambda: dot(q, k, torch.randn(5, 3, 2, 1)),
        "query_size": lambda: dot(torch.randn(3, 5), k, v),
        "key_size": lambda: M.GeneralizedDotProductSoftAttention(4, 3)(q, k, v),
        "dim_range": lambda: M.DotProductSoftAttention(4, dim=2)(q, k, v),
        "dim_minus_one": lambda: M.DotProductSoftAttention(4, dim=-1)(q, k, v),
        "broadcast": lambda: dot(torch.randn(2, 4), k, v),
        "mask_broadcast": lambda: dot(q, k, v, torch.ones(4, 3, dtype=torch.bool)),
        "mask_not_bool": lambda: dot(q, k, v, torch.ones(5, 3)),
        "mha_query_ndim": lambda: mha(torch.randn(4), k, v),
        "mha_dim_range": lambda: M.MultiHeadedAttention(4, 4, 2, 2, M.DotProductSoftAttention(2, dim=2))(q, k, v),
        "mha_value_size": lambda: mha(q, k, torch.randn(5, 3, 3)),
        "mha_score": lambda: mha.score(q, k),
        "mha_negative_dim": lambda: M.MultiHeadedAttention(4, 4, 2, 2, M.DotProductSoftAttention(2, dim=-2)),
        "ctor_size": lambda: M.DotProductSoftAttention(0),
        "ctor_bias": lambda: M.GeneralizedDotProductSoftAttention(3, 4, 0, "yes"),
        "ctor_hidden": lambda: M.ConcatSoftAttention(3, 4, hidden_size=0),
        "ctor_heads": lambda: M.MultiHeadedAttention(4, 4, 2, 0, M.DotProductSoftAttention(2)),
    }
    assert sorted(cases) == sorted(errors)
    for key, fn in cases.items():
        if errors[key] == "none":
            fn()
            continue
        with pytest.raises(Exception) as info:
            fn()
        assert type(info.value).__name__ == errors[key], (key, info.value)


def test_torch_body_matches_goldens(gold):
    for k in range(int(gold["case_n"])):
        m, ins, mask, _ = load_case(gold, k)
        check_case(gold, k, m, ins, mask, 1e-6, 1e-6)


def test_concat_score_matches_expanded_concatenation():
    from pydrobert_amd import modules as M

    torch.manual_seed(3)
    m = M.ConcatSoftAttention(3, 4, 1, True, 6).double()
    q, k = torch.randn(2, 3, dtype=torch.float64), torch.randn(2, 5, 4, dtype=torch.float64)
    qe = q.unsqueeze(1).expand(2, 5, 3)
    exp = torch.nn.functional.linear(torch.tanh(torch.nn.functional.linear(torch.cat([qe, k], -1), m.weight, m.bias)),
                                     m.v.unsqueeze(0)).squeeze(-1)  # fmt: skip
    assert torch.allclose(m.score(q, k), exp, atol=1e-12)


def test_script_trace_compile_cpu():
    from pydrobert_amd import modules as M

    torch.manual_seed(0)
    q, k, v = torch.randn(3, 4), torch.randn(5, 3, 4), torch.randn(5, 3, 2)
    mask = torch.arange(5).unsqueeze(1) < torch.tensor([5, 2, 4])
    mods = [M.DotProductSoftAttention(4, 0, 0.5), M.GeneralizedDotProductSoftAttention(4, 4, 0, True),
            M.ConcatSoftAttention(4, 4, 0, True, 6), cosine_attention()(4),
            M.MultiHeadedAttention(4, 4, 2, 2, M.GeneralizedDotProductSoftAttention(2, 2))]  # fmt: skip
    for mod in mods:
        mk = None if isinstance(mod, M.MultiHeadedAttention) else mask  # (its mask gains a head axis before the last)
        exp = mod(q, k, v, mk)
        assert torch.allclose(torch.jit.script(mod)(q, k, v, mk), exp, atol=1e-6), type(mod).__name__
        args = (q, k, v) if mk is None else (q, k, v, mk)
        assert torch.allclose(torch.jit.trace(mod, args)(*args), exp, atol=1e-6), type(mod).__name__
    torch._dynamo.reset()
    comp = torch.compile(mods[0], backend="eager", fullgraph=True)
    assert torch.allclose(comp(q, k, v, mask), mods[0](q, k, v, mask), atol=1e-6)


def test_ops_registered_and_entry_points_declared():
    import pydrobert_amd.modules  # noqa: F401
    from pydrobert_amd import _cabi

    for op in ("dot_attention", "dot_attention_backward", "attention_pool", "attention_pool_backward"):
        assert hasattr(torch.ops.pydrobert_amd, op)
    header = open(os.path.join(ROOT, "include", "pdt_amd.h")).read()
    for name in ("pdt_attn_dot", "pdt_attn_dot_backward", "pdt_attn_pool", "pdt_attn_pool_backward",
                 "pdt_attn_workspace_bytes"):  # fmt: skip
        assert name in _cabi.SIGNATURES and name + "(" in header


def _desc(R=6, G=2, M=3, T=5, D=4, Dv=3, sizes=(2, 3)):
    """A valid descriptor: rows (2, 3), the inner dim the group (key and value strides 0 there)."""
    from pydrobert_amd import _attn

    d = [0] * _attn._DESC_LEN
    d[0:7] = [len(sizes), R, G, M, T, D, Dv]
    d[7:7 + len(sizes)] = list(sizes)
    for slot in range(_attn._SLOTS):
        base = 7 + _attn._MAX_DIMS + slot * (_attn._MAX_DIMS + 2)
        d[base] = 7
        d[base + _attn._MAX_DIMS] = 1
        d[base + _attn._MAX_DIMS + 1] = 1
        if slot not in (_attn._SK, _attn._SV, _attn._SGK, _attn._SGV):
            d[base + 1] = 2
    return (ctypes.c_int64 * len(d))(*d)


def test_c_entry_points_validate_without_gpu():
    """Argument checks return before any launch, so these calls are safe without a GPU."""
    import __graft_entry__ as g
    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    lib = _cabi.lib()
    OK, ARG = _cabi.PDT_OK, _cabi.PDT_E_ARG
    scale = ctypes.c_double(1.0)
    sp = ctypes.addressof(scale)
    desc = _desc()
    assert lib.pdt_attn_workspace_bytes(desc, 0, 0) >= 0
    assert lib.pdt_attn_workspace_bytes(desc, 0, 1) >= 6 * 4  # (delta per row)
    assert lib.pdt_attn_workspace_bytes(desc, 1, 1) >= 6 * 8
    assert lib.pdt_attn_workspace_bytes(desc, 2, 0) == -1  # bad dtype
    assert lib.pdt_attn_workspace_bytes(desc, 0, 4) == -1  # bad kind
    assert lib.pdt_attn_workspace_bytes(None, 0, 0) == -1
    # null pointers with rows to do
    assert lib.pdt_attn_dot(desc, 0, 0, 0, 0, 0, sp, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_attn_dot_backward(desc, 0, 0, 0, 0, 0, sp, 0, 0, 0, 0, 0, 0, 0, 0, 0) == ARG
    pdesc = _desc(D=0)
    assert lib.pdt_attn_pool(pdesc, 0, 0, 0, 0, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_attn_pool_backward(pdesc, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == ARG
    assert lib.pdt_attn_dot(desc, 0, 1, 1, 1, 0, None, 1, 1, 0, 0, 0) == ARG  # no scale
    # rows == 0: OK, nothing to do
    empty = _desc(R=0, G=0, M=3, sizes=(0, 3))
    assert lib.pdt_attn_dot(empty, 0, 0, 0, 0, 0, sp, 0, 0, 0, 0, 0) == OK
    assert lib.pdt_attn_pool_backward(_desc(R=0, G=0, M=3, D=0, sizes=(0, 3)), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == OK
    # negative sizes, sizes that do not multiply to R, a group whose key is not broadcast, T == 0 with rows
    for bad in (_desc(T=-1), _desc(R=5), _desc(G=3, M=2), _desc(T=0), _desc(D=0), _desc(Dv=0)):
        assert lib.pdt_attn_dot(bad, 0, 1, 1, 1, 0, sp, 1, 1, 1, 1 << 30, 0) == ARG
    d = list(_desc())
    d[7 + 8 + 1 * 10 + 1] = 4  # key stride 4 along the group's dim
    assert lib.pdt_attn_dot((ctypes.c_int64 * len(d))(*d), 0, 1, 1, 1, 0, sp, 1, 1, 1, 1 << 30, 0) == ARG
    # too small a workspace
    big = _desc(R=2, G=2, M=1, T=4096, sizes=(2, 1))
    need = lib.pdt_attn_workspace_bytes(big, 0, 0)
    assert need > 0
    assert lib.pdt_attn_dot(big, 0, 1, 1, 1, 0, sp, 1, 1, 1, need - 1, 0) == ARG


def test_group_is_chosen_by_size_not_stride():
    """A key or value the caller expanded (stride 0 at full size) keeps a gradient per slice: only dims where
    the key and value have size 1 form the group the kernels sum over."""
    from pydrobert_amd import _attn

    q = torch.randn(3, 4, 5)
    k1, v1 = torch.randn(6, 3, 1, 5), torch.randn(6, 3, 1, 7)
    plan, _ = _attn._dot_plan(q, k1, v1, None, 0)
    assert (plan.shared_shape, plan.G, plan.M) == ([6, 3, 1], 3, 4)
    k, v = k1.expand(6, 3, 4, 5), v1.expand(6, 3, 4, 7)
    plan, _ = _attn._dot_plan(q, k, v, None, 0)
    assert (plan.shared_shape, plan.G, plan.M) == ([6, 3, 4], 12, 1)
    torch.zeros(plan.shared_shape + [5]).sum_to_size(k.shape)  # (the backward's reduction to the key's shape)
    plan, _ = _attn._pool_plan(torch.randn(6, 3, 4), v, None, 0)
    assert (plan.shared_shape, plan.G, plan.M) == ([6, 3, 4], 12, 1)
    plan, _ = _attn._pool_plan(torch.randn(6, 3, 4), v1, None, 0)
    assert (plan.shared_shape, plan.G, plan.M) == ([6, 3, 1], 3, 4)


def test_route_leaves_rows_too_wide_for_the_tiles_to_torch():
    from pydrobert_amd import _attn

    class Fake:  # (what _hip_route reads of a ROCm tensor, without a GPU)
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

        def dim(self):
            return len(self.shape)

    for dt, width, ok in ((torch.float32, 14336, True), (torch.float32, 14337, False),
                          (torch.float64, 7168, True), (torch.float64, 7169, False)):  # fmt: skip
        v = Fake((5, 3, 2), dt)
        assert _attn._hip_route([5, 3], v, None, 0, [Fake((5, 3, 4), dt), v], width) is ok


# ----------------------------------------------------------------------------------------------------------
# the float64 reference, the plan restatement and the case table of tests/_attn_ref.py (test_attn_gpu.py runs
# the cases on the kernels)

import _attn_ref as R  # noqa: E402


def test_reference_matches_torch_formula_and_goldens(gold):
    """attend_ref / pool_ref against _softmax_pool in float64 (values and gradients), and against the dot-product
    goldens captured from the reference."""
    from pydrobert_amd import modules as M
    from pydrobert_amd._attn import _softmax_pool

    for name in ("spans-dot-64", "spans-pool-64", "neginf-tiles-64", "chunks-key-and-value-expanded",
                 "chunks-value-broadcast-along-T", "rows-threshold-16-17-strided-64", "walk-pool-flat-64"):
        def dot(query, key, value, mask, dim, scale):
            return _softmax_pool((query.unsqueeze(dim) * key).sum(-1) * scale, value, mask, dim)

        out, grads = R.run_case(name, dot, _softmax_pool, torch.float64, "cpu")
        ref_out, ref_grads = R.expected(name)
        ok = ~torch.isnan(ref_out)
        assert torch.allclose(out[ok], ref_out[ok], rtol=1e-12, atol=1e-12), name
        for n in grads:
            assert torch.allclose(grads[n], ref_grads[n], rtol=1e-12, atol=1e-12), (name, n)
    seen = 0
    for k in range(int(gold["case_n"])):
        m, ins, mask, spec = load_case(gold, k)
        if type(m) is not M.DotProductSoftAttention or ins[0].dtype != torch.float64 or m.dim < 0:
            continue
        if ins[1].shape[m.dim] == 0:
            continue  # (T = 0: zeros by convention, not by the formula)
        out = R.attend_ref(ins[0], ins[1], ins[2], mask, m.dim, m.scale_factor).detach().numpy()
        exp = gold["case_{}_out".format(k)]
        fin = ~np.isnan(exp)
        assert np.array_equal(np.isnan(out), ~fin) and np.allclose(out[fin], exp[fin], rtol=1e-10, atol=1e-10), k
        seen += 1
    assert seen > 0


def test_dropped_row_variant_takes_the_row_out_of_every_gradient():
    """The reference used for an all-masked row: its gradients equal those of the same inputs with the row
    removed, and the row's own gradient is 0."""
    name = "dead-9-dot"
    c, x = R.CASES[name], R.build_inputs(name)
    (g0, m0), = np.argwhere(x["dead"])
    _, grads = R.expected(name)
    keep = [m for m in range(c["M"]) if m != m0]
    q = torch.from_numpy(x["q"][g0, keep]).requires_grad_(True)
    k = torch.from_numpy(x["k"][:, g0].copy()).requires_grad_(True)  # (T, 1, D)
    v = torch.from_numpy(x["v"][:, g0].copy()).requires_grad_(True)
    out = R.attend_ref(q, k, v, torch.from_numpy(x["mask"][:, g0][:, keep]), 0, x["scale"])
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), torch.from_numpy(x["gout"][g0, keep]))
    assert torch.allclose(grads["k"][:, g0], gk, rtol=1e-12, atol=1e-12)
    assert torch.allclose(grads["v"][:, g0], gv, rtol=1e-12, atol=1e-12)
    assert torch.allclose(grads["q"][g0, keep], gq, rtol=1e-12, atol=1e-12)
    assert bool((grads["q"][g0, m0] == 0).all())


def _lib():
    import __graft_entry__ as g
    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


@pytest.mark.parametrize("name", list(R.CASES))
def test_plan_restatement_matches_the_library(name):
    """plan_of against pdt_attn_workspace_bytes for every case and all four kinds (no launch: no GPU needed).
    Equal workspace sizes pin the forward's splits and its choice of the rows kernel, and the backward's
    frame chunks."""
    lib = _lib()
    c = R.CASES[name]
    G, M = R.plan_shape(c)
    for dt, esz in ((0, 4), (1, 8)):
        for kind, code in R.KINDS.items():
            pool = kind.startswith("pool")
            D = 0 if pool else max(1, c["D"])
            p = R.plan_of(G, M, c["T"], D, c["Dv"], esz, kind)
            desc = _desc(R=G * M, G=G, M=M, T=c["T"], D=D, Dv=c["Dv"], sizes=(G, M))
            assert lib.pdt_attn_workspace_bytes(desc, dt, code) == p["ws_bytes"], (kind, esz, p)
            if not kind.endswith("bwd"):
                assert (p["ws_bytes"] == 0) == (p["splits"] == 1)
                if c["T"] > 32 and G * p["tiles"] * max(1, p["zcols"]) < 512:
                    assert (p["ws_bytes"] == 0) == bool(p["rows_form"])  # (few workgroups: only the rows form is unsplit)


def test_rows_per_tile_by_element_size_decides_the_spans():
    """Shapes where the row tiles per group (rows per tile by LDS: the bytes of a row, so the element size)
    decide how T is split: the workspace pins the rows per tile."""
    lib = _lib()
    for G, M, T, D, Dv, esz, form in R.PLAN_ONLY:
        p = R.plan_of(G, M, T, D, Dv, esz, "dot")
        assert {k: p[k] for k in form} == form, p
        other = R.plan_of(G, -(-M // min(8, M)), T, 1, Dv, esz, "dot")  # (the spans if 8 rows fitted a tile)
        assert other["splits"] != p["splits"], "the shape is sensitive to the rows per tile"
        desc = _desc(R=G * M, G=G, M=M, T=T, D=D, Dv=Dv, sizes=(G, M))
        assert lib.pdt_attn_workspace_bytes(desc, 0 if esz == 4 else 1, 0) == p["ws_bytes"], (G, M, T, D, esz)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_has_the_plan_form_it_is_named_for(name):
    c = R.CASES[name]
    G, M = R.plan_shape(c)
    esz = 4 if c["dtype"] == "float32" else 8
    assert c["form"], "every case names a form"
    for side, claim in c["form"].items():
        p = R.plan_of(G, M, c["T"], c["D"], c["Dv"], esz, c["route"] + ("_bwd" if side == "bwd" else ""))
        assert {k: p[k] for k in claim} == claim, (side, p)
    assert max(c["G"] * c["M"] * max(c["D"], c["Dv"]), c["T"] * c["G"] * max(c["D"], c["Dv"])) <= 2.4e6  # (small tensors)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_mask_is_what_the_case_claims(name):
    """Each mask recipe's claims, from the mask alone; an all-masked row only in the cases named for one, and
    one at most.  The spoiled inputs are non-finite exactly where no row (pool score: not this row) attends."""
    c, x = R.CASES[name], R.build_inputs(name)
    dead = R.check_mask(c["mask"], x["mask"], c["T"], c["G"], c["M"])
    assert np.array_equal(dead, x["dead"]) and dead.sum() <= 1
    assert bool(dead.any()) == (c["mask"] in ("dead_row", "spans"))
    if c["bad"]:
        unseen = ~x["mask"].any(2)
        assert unseen.any() and np.array_equal(np.isnan(x["v_bad"]).all((2, 3)), unseen)
        if c["route"] == "dot":
            assert np.array_equal(np.isinf(x["k_bad"]).all((2, 3)), unseen)
        else:
            assert np.array_equal(~np.isfinite(x["e_bad"]), ~x["mask"])
    if c["neginf"]:
        seen = x["e"] if x["mask"] is None else np.where(x["mask"], x["e"], 0.0)
        assert np.isneginf(seen).any() and np.isfinite(np.where(np.isneginf(seen), -np.inf, x["e"])).any(0).all()
        kept = np.isfinite(x["e"]) & (True if x["mask"] is None else x["mask"])
        assert kept.any(0).all(), "every row keeps a finite score"
    if c["profile"] is not None and x["mask"] is None:  # (the 32-frame tiles' maxima follow the trend in every row)
        e = R.scores_of(name)
        tile_max = [e[a:a + 32].max(0) for a in range(0, c["T"], 32)]
        assert len(tile_max) == 3
        for a, b in zip(tile_max, tile_max[1:]):
            assert bool({"rising": b > a + 1, "falling": b < a - 1, "flat": (b == a) & (b == R.flat_score(c))}[c["profile"]].all())


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["measured"]])
def test_measured_tolerances_follow_the_rule(name):
    """The wide or long cases (D, Dv or T above 300) and the shifted ones: every recorded bound is the suite's
    or lies in [4, 16] x err32 (the float32 formula's own error on the case's inputs, recomputed here) and is
    not below the suite's; every bound is under 1 % of the median |reference| of its tensor (over its non-zero
    entries: gradients are exactly 0 at masked frames)."""
    c = R.CASES[name]
    ref_out, ref_grads = R.expected(name)
    refs = dict(ref_grads, out=ref_out[~torch.isnan(ref_out)])
    assert set(c["tol"]) <= set(refs)
    err32 = R.formula32_error(name) if c["dtype"] == "float32" else None
    for n, ref in refs.items():
        suite, atol = R.bound(name, n)
        if err32 is not None:
            print("{} {}: err32 {:.3e}, 8 x err32 {:.3e}, bound {:.1e}".format(name, n, err32[n], 8 * err32[n], atol))
            if atol != suite:
                assert atol > suite and 4 * err32[n] <= atol <= 16 * err32[n], (n, err32[n], atol)
            else:
                assert 8 * err32[n] <= suite, (n, err32[n], "needs a measured bound")
        else:
            assert atol == suite  # (float64: no case needs more than the suite's bound)
        mag = ref.abs()[ref != 0]
        assert atol < 0.01 * float(mag.median()), (n, atol, float(mag.median()))
