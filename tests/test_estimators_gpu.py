"""MI355X: the sample-axis reduction kernels and the IMH scan against tests/_estimators_ref.py, every golden case
through the estimators on the device, derivatives, seeded end-to-end runs, torch.compile and torch.jit.trace.

The reductions are held to the float64 yardstick within the tolerance the golden maker measured on the reference
and stored (``tol_op_<operation>_<v|g>_<dtype>``, units of eps (1 + |value|)); the scan is compared exactly.
"""
import math

import pytest
import torch

import _estimators_check as C
import _estimators_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("f", "a", "cz", "c", "lp", "lq")
OPS = {ref.MEAN: "MEAN", ref.SCORE: "SCORE", ref.WEIGHTED: "WEIGHTED"}
# (operation, mode, the inputs present)
CONFIGS = [
    (ref.MEAN, 0, ("f",)),
    (ref.SCORE, 0, ("f", "lp")),
    (ref.SCORE, 0, ("f", "a", "lp")),
    (ref.SCORE, 0, ("f", "a", "c", "lp")),
    (ref.SCORE, 0, ("f", "a", "cz", "lp")),
    (ref.WEIGHTED, ref.W_LOGM, ("f", "lp", "lq")),
    (ref.WEIGHTED, ref.W_SELF, ("f", "lp", "lq")),
    (ref.WEIGHTED, ref.W_NONE, ("f", "lp")),
]
IDS = ["{}-{}-{}".format(OPS[k], m, "+".join(p)) for k, m, p in CONFIGS]


def X():
    from pydrobert_amd import _estimators

    return _estimators


def op_tolerance(kind, output, dtype):
    return float(C.gold()["tol_op_{}_{}_{}".format(OPS[kind], output, str(dtype).split(".")[-1])])


def draw(gen, present, M, batch, dtype, support=False):
    """CPU inputs of shape (M,) + batch (c: batch) in ``dtype``.  The control variate ``a`` stays below ``f``
    sample by sample, so that in log space the mean of exp(f) - exp(a) is positive: at a mean below the floor the
    reference's ``log(mean) + score - score`` loses the logarithm to a score of 1e19, which the kernel, whose
    score term is 0, does not reproduce."""
    T = {}
    for name in present:
        if name == "a":
            T[name] = (T["f"].double() - 0.5 - 2 * torch.rand((M,) + batch, generator=gen).double()).to(dtype)
        elif name == "c":
            T[name] = torch.randn(batch, generator=gen).to(dtype)
        elif name == "lp" and support:  # log probabilities over an enumerated support: they sum to 1 down a column
            T[name] = (2 * torch.randn((M,) + batch, generator=gen)).double().log_softmax(0).to(dtype)
        elif name in ("lp", "lq"):
            T[name] = (-3 * torch.rand((M,) + batch, generator=gen)).to(dtype)
        else:
            T[name] = (2 * torch.randn((M,) + batch, generator=gen)).to(dtype)
    return T


def lay_out(f, layout):
    """``f`` on the device with the same values in another memory layout."""
    if layout == "dense":
        return f.to(DEV)
    if layout == "transposed":  # m the dense axis
        return f.to(DEV).movedim(0, -1).contiguous().movedim(-1, 0)
    assert layout == "gapped"  # the batch dimensions do not collapse onto one stride: the host copies
    wide = torch.zeros(f.shape[:-1] + (f.shape[-1] + 1,), dtype=f.dtype, device=DEV)
    wide[..., :-1] = f.to(DEV)
    return wide[..., :-1]


def compare(kind, is_log, mode, T, dtype, layout="dense", what=""):
    """The kernel's value and gradients against the yardstick's on the inputs ``T``; returns the figures."""
    eps = float(torch.finfo(dtype).eps)
    on = {n: (lay_out(t, layout) if n == "f" else t.to(DEV)).requires_grad_(True) for n, t in T.items()}
    if layout != "dense":
        assert not on["f"].is_contiguous() or on["f"].numel() <= max(on["f"].shape)
    v = X().mc_reduce(kind, is_log, **on, mode=mode)
    D = {n: ref.f64(t).requires_grad_(True) for n, t in T.items()}
    want = ref.reduce64(kind, is_log, mode, dtype, **D)
    assert v.shape == want.shape and v.dtype == dtype and v.device.type == DEV.type, what
    g = ref.upstream(want.shape)
    names = list(T)
    got_g = torch.autograd.grad(v, [on[n] for n in names], g.to(DEV, dtype), allow_unused=True)
    want_g = torch.autograd.grad(want, [D[n] for n in names], g, allow_unused=True)
    figures = {"v": ref.units(v, want, eps)}
    for n, a, b in zip(names, got_g, want_g):
        assert a is not None, (what, n)
        figures["g_" + n] = ref.units(a, torch.zeros_like(D[n]) if b is None else b, eps)
    print(what, {k: round(x, 2) for k, x in figures.items()})
    for name, d in figures.items():
        tol = op_tolerance(kind, "v" if name == "v" else "g", dtype)
        assert d <= tol, (what, name, d, tol)
    return figures


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("is_log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_reduction_parity(config, is_log, dtype):
    kind, mode, present = config
    gen = torch.Generator().manual_seed(1000 * kind + 10 * mode + len(present))
    for M, B, layout in C.PARITY_SHAPES:
        T = draw(gen, present, M, (B,), dtype, support=mode == ref.W_NONE)
        compare(kind, is_log, mode, T, dtype, layout, "{} M={} B={} {}".format(OPS[kind], M, B, layout))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", ["dense", "transposed", "gapped"])
def test_reduction_batch_shapes(layout, dtype):
    """A (2, 3) batch shape: collapsing onto one stride (dense, transposed) and not (the host's dense copy)."""
    gen = torch.Generator().manual_seed(77)
    for (kind, mode, present), is_log in ((CONFIGS[3], True), (CONFIGS[4], False), (CONFIGS[6], True), (CONFIGS[0], True)):
        T = draw(gen, present, 7, (2, 3), dtype)
        compare(kind, is_log, mode, T, dtype, layout, "{} (2, 3) {}".format(OPS[kind], layout))
    # cv_mean given as a scalar, and with the reference's leading 1: broadcast on the host
    T = draw(gen, CONFIGS[3][2], 7, (2, 3), dtype)
    for c in (T["c"][0, 0], T["c"][None]):
        on = {n: t.to(DEV) for n, t in dict(T, c=c).items()}
        want = ref.reduce64(ref.SCORE, True, 0, dtype, **{n: ref.f64(t) for n, t in dict(T, c=c.reshape(-1, 3)[-2:].expand(2, 3) if c.dim() else c.expand(2, 3)).items()})
        got = X().mc_reduce(ref.SCORE, True, **on)
        assert ref.units(got, want, float(torch.finfo(dtype).eps)) <= op_tolerance(ref.SCORE, "v", dtype)


def classes_agree(kind, is_log, mode, T, dtype, what):
    """Same class (finite, nan, +inf, -inf) as the torch body on the CPU, equal values where finite -- for the
    value and for every gradient."""
    body = X().mc_reduce_torch
    eps = float(torch.finfo(dtype).eps)
    cpu = {n: t.clone().requires_grad_(True) for n, t in T.items()}
    on = {n: t.to(DEV).requires_grad_(True) for n, t in T.items()}
    want = body(kind, is_log, mode, **cpu)
    got = X().mc_reduce(kind, is_log, **on, mode=mode)
    assert ref.units(got, want, eps) <= op_tolerance(kind, "v", dtype), (what, got, want)
    names = [n for n in T if n != "lq"]
    g = ref.upstream(want.shape, dtype)
    got_g = torch.autograd.grad(got, [on[n] for n in names], g.to(DEV))
    want_g = torch.autograd.grad(want, [cpu[n] for n in names], g)
    for n, a, b in zip(names, got_g, want_g):
        assert ref.units(a, b, eps) <= op_tolerance(kind, "g", dtype), (what, n, a, b)
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("M,B", [(7, 65), (65, 3)], ids=["columns", "wave"])
def test_non_finite_columns(M, B, dtype):
    gen = torch.Generator().manual_seed(5)
    inf = math.inf
    for is_log in (False, True):
        for mode in (ref.W_LOGM, ref.W_SELF, ref.W_NONE):
            present = ("f", "lp") if mode == ref.W_NONE else ("f", "lp", "lq")
            T = draw(gen, present, M, (B,), dtype)
            T["lp"][::3, 0] = -inf  # some samples outside the support of P
            T["lp"][:, 1] = -inf  # every weight of the column is 0
            got = classes_agree(ref.WEIGHTED, is_log, mode, T, dtype, "WEIGHTED mode {} log {}".format(mode, is_log))
            assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[2:]).all())
            if mode == ref.W_SELF:
                assert bool(torch.isnan(got[1]))
        # both clamps: f and its control variate far below the column maximum, cv(z) far above it
        T = draw(gen, ("f", "a", "cz", "lp"), M, (B,), dtype)
        T["f"][1:, 0] -= 100.0
        T["a"][1:, 0] -= 100.0
        T["cz"][-1, 0] = T["f"][:, 0].max() + 100.0
        T["cz"][-1, 1] = T["f"][:, 1].max() + 60.0
        if is_log:  # (not in log space -inf * lp - (-inf * lp) is NaN in the reference, by the score term)
            T["f"][0, 2] = -inf
        got = classes_agree(ref.SCORE, is_log, 0, T, dtype, "SCORE clamps log {}".format(is_log))
        if is_log:
            assert bool(torch.isfinite(got[:2]).all())
        T = draw(gen, ("f",), M, (B,), dtype)
        T["f"][::2, 0] = -inf
        T["f"][:, 1] = -inf
        T["f"][0, 2] = inf
        classes_agree(ref.MEAN, is_log, 0, T, dtype, "MEAN log {}".format(is_log))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_imh_scan_is_exact(dtype):
    gen = torch.Generator().manual_seed(11)
    for M, B in ((1, 1), (64, 65), (65, 257), (300, 65), (300, 1), (7, 257)):
        ratio = torch.randn((M, B), generator=gen).to(dtype)
        ratio0 = torch.randn((B,), generator=gen).to(dtype)
        log_u = torch.rand((M, B), generator=gen).log().to(dtype)
        ratio[torch.rand((M, B), generator=gen) < 0.15] = -math.inf  # proposals outside the support
        if M > 2:
            ratio[2::5] = ratio[1::5][: ratio[2::5].size(0)]  # equal consecutive ratios: a difference of exactly 0
        log_u[torch.rand((M, B), generator=gen) < 0.1] = -math.inf  # u = 0
        log_u[torch.rand((M, B), generator=gen) < 0.05] = 0.0  # u = 1: only a strict improvement is accepted
        want = ref.imh_loop(ratio, ratio0, log_u)
        for transposed in (False, True):
            r = ratio.to(DEV)
            if transposed:
                r = r.t().contiguous().t()
            got = X().imh_chain(r, ratio0.to(DEV), log_u.to(DEV))
            assert got[0].dtype == torch.int32 and got[1].dtype == dtype and got[2].dtype == torch.int32
            for a, b, name in zip(got, want, ("idx", "last", "last_idx")):
                assert torch.equal(a.cpu(), b), (M, B, transposed, name)
        assert (want[0] >= 0).any() or M == 1
    # a NaN on either side rejects; a batch shape; float32 uniforms against float64 ratios
    ratio = torch.tensor([[math.nan, 1.0], [2.0, math.nan], [3.0, 0.5]], dtype=dtype).reshape(3, 1, 2)
    log_u = torch.tensor([[-1.0, math.nan], [-1.0, -1.0], [-1.0, -1.0]]).reshape(3, 1, 2)
    idx, last, last_idx = X().imh_chain(ratio.to(DEV), torch.zeros(1, 2, dtype=dtype, device=DEV), log_u.to(DEV))
    assert idx.shape == (3, 1, 2) and idx.flatten().tolist() == [-1, -1, 1, -1, 2, 2]
    assert last.flatten().tolist() == [3.0, 0.5] and last_idx.flatten().tolist() == [2, 2]


@pytest.mark.parametrize("k", range(len(C.cases())))
def test_golden_case_on_the_device(k):
    C.check_case(k, DEV, report=lambda k, case, figures: print(k, case["est"], case["dtype"], figures))


def test_imh_chunks_on_the_device(monkeypatch):
    import pydrobert_amd.estimators as E

    gen = torch.Generator().manual_seed(3)
    M, batch, V = 300, (65,), 5
    plog, qlog = torch.randn(batch + (V,), generator=gen), torch.randn(batch + (V,), generator=gen)
    rows = torch.randint(0, V, (M + 1,) + batch, generator=gen)
    u, w = torch.rand((M,) + batch, generator=gen), torch.randn(V, generator=gen)
    results = []
    for budget in (None, 65 * 8 * 64):  # one chunk; 64 steps a chunk, five chunks
        if budget is not None:
            monkeypatch.setattr(X(), "IMH_CHUNK_BYTES", budget)
        calls = []
        est = E.IndependentMetropolisHastingsEstimator(
            ref.ReplayCategorical(qlog.to(DEV), rows.to(DEV)), lambda b: calls.append(b.size(0)) or w.to(DEV)[b], M,
            torch.distributions.Categorical(logits=plog.to(DEV)), burn_in=70, is_log=True)
        with ref.noise(u):
            results.append(est())
        assert sum(calls) == M - 70 and len(calls) == (1 if budget is None else 4)
    lp, lq = (torch.distributions.Categorical(logits=x).log_prob(rows) for x in (plog, qlog))
    ratio = lp - lq
    idx, _, _ = ref.imh_loop(ratio[1:], ratio[0], u.log())
    chain = w[rows].gather(0, idx[70:].long() + 1).double()
    want = ref.reduce64(ref.MEAN, True, 0, torch.float32, chain)
    for v in results:
        assert ref.units(v, want, 2.0 ** -23) <= C.tolerance("imh", "v", "float32")


@pytest.mark.parametrize("is_log", [False, True], ids=["lin", "log"])
@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_gradcheck_and_gradgradcheck(config, is_log):
    """First derivatives of the forward operator (the backward kernel) and second derivatives (the backward
    operator's registered derivative) against finite differences, float64."""
    from torch.autograd import gradcheck, gradgradcheck

    kind, mode, present = config
    gen = torch.Generator().manual_seed(9)
    T = draw(gen, present, 5, (3,), torch.float64)
    names = [n for n in present if n != "lq"]
    fixed = {n: T[n].to(DEV) for n in present if n == "lq"}

    def fn(*xs):
        return X().mc_reduce(kind, is_log, **dict(zip(names, xs)), **fixed, mode=mode)

    xs = [T[n].to(DEV).requires_grad_(True) for n in names]
    if kind == ref.SCORE:
        # lp does not enter the value (score - score.detach()): its derivative is the REINFORCE weight, which finite
        # differences cannot see; it is checked against the yardstick in test_reduction_parity
        xs[names.index("lp")].requires_grad_(False)
    assert gradcheck(fn, xs, eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)
    assert gradgradcheck(fn, xs, eps=1e-6, atol=1e-5, rtol=1e-4, nondet_tol=0.0)


def test_lq_gets_zeros_not_none():
    gen = torch.Generator().manual_seed(2)
    T = draw(gen, ("f", "lp", "lq"), 9, (5,), torch.float32)
    on = {n: t.to(DEV).requires_grad_(True) for n, t in T.items()}
    X().mc_reduce(ref.WEIGHTED, True, **on, mode=ref.W_SELF).sum().backward()
    assert on["lq"].grad is not None and not on["lq"].grad.any()


# ---- seeded end-to-end runs ---------------------------------------------------------------------------------------
def relax_variance(logits, t, temp, eta, nodes=4000):
    """(E X, Var X) of the RELAX term X = f(b) - c(zcond) + c(z) for LogisticBernoulli(logits), f(x) = (x - t)^2 +
    0.5 and the REBAR variate c(x) = eta f(sigmoid(x / temp)), float64.  z = logits + log u - log(1 - u) thresholds
    to b = [u >= 1 - p]; zcond = (2 b - 1) log(v / ((1 - v) q_b) + 1) with q_1 = 1 - p, q_0 = p (the eps that
    csample adds to it, 1e-7, is left out).  With A(u) = f(b) + c(z(u)) and C_b(v) = c(zcond(b, v)), u and v
    independent uniforms, E X^2 = sum_b [int_b A^2 du - 2 int_b A du int C_b dv + P(b) int C_b^2 dv]: six
    integrals of bounded smooth functions per element, Gauss-Legendre with ``nodes`` points each (the integrands
    are algebraic in u and v at temp = 0.5: 4000 points leave errors far below the 1e-6 the mean is checked to)."""
    import numpy as np

    x, w = np.polynomial.legendre.leggauss(nodes)
    x, w = torch.from_numpy((x + 1) / 2), torch.from_numpy(w / 2)  # nodes and weights on (0, 1)
    f = lambda s: (s - t) ** 2 + 0.5  # noqa: E731
    c = lambda z: eta * f((z / temp).sigmoid())  # noqa: E731
    p = logits.sigmoid()
    ex = torch.zeros_like(p)
    ex2 = torch.zeros_like(p)
    for b, lo, width, q in ((0.0, torch.zeros_like(p), 1 - p, p), (1.0, 1 - p, p, 1 - p)):
        u = lo + width * x[:, None]  # the u that threshold to b, (nodes, 4)
        A = f(torch.full_like(p, b)) + c(logits + u.log() - (-u).log1p())
        v = x[:, None].expand(-1, p.numel())
        C = c((2 * b - 1) * (v / ((1 - v) * q) + 1).log())
        i_a, i_a2 = width * (w[:, None] * A).sum(0), width * (w[:, None] * A * A).sum(0)
        i_c, i_c2 = (w[:, None] * C).sum(0), (w[:, None] * C * C).sum(0)
        ex = ex + i_a - width * i_c
        ex2 = ex2 + i_a2 - 2 * i_a * i_c + width * i_c2
    return ex, ex2 - ex * ex


def test_score_floored_mean():
    """Log-space SCORE with the control variate ABOVE f: the mean of exp(f) - exp(a) is negative, the floor
    exp(EPS_NINF) takes its place, and the value is log(floor) + max with no gradient through the mean (the path
    through the maximum remains).  Held to the yardstick, whose score term is exactly 0 as the kernel's is (the
    reference's own sum loses the logarithm to the 1e19 score there: INTEGRATION.md)."""
    gen = torch.Generator().manual_seed(13)
    for dtype in (torch.float32, torch.float64):
        for M, B in ((7, 65), (65, 3)):  # columns, wave
            for kind, mode, present in CONFIGS[2:5]:
                T = draw(gen, present, M, (B,), dtype)
                T["a"] = (T["f"].double() + 6 + 2 * torch.rand((M, B), generator=gen).double()).to(dtype)
                floor = ref.rounded(math.exp(ref.EPS_NINF), dtype)
                want = ref.reduce64(kind, True, mode, dtype, **{n: ref.f64(x) for n, x in T.items()})
                assert torch.equal(want, math.log(floor) + ref.f64(T["f"]).max(0)[0])  # (the branch is taken)
                compare(kind, True, mode, T, dtype, "dense", "floored {} M={} B={}".format("+".join(present), M, B))


def test_unbiased_estimators_meet_their_exact_value():
    r"""Four independent Bernoullis (a batch of 4), M = 4096.  v_exact is EnumerateEstimator's; every estimator here
    averages M i.i.d. terms X with mean v_exact, so its error is within 6 sqrt(Var X / M) except with probability
    below 1e-8 (Chebyshev gives 1/36 for any law; the average of 4096 bounded terms is normal to far better than
    that margin).  Var X in closed form: Direct and StraightThrough, Var f(b) = p (1 - p) (f(1) - f(0))^2;
    importance sampling, E_Q[(f P / Q)^2] - v^2, two terms; Relax, X = f(b) - c(zcond) + c(z): relax_variance below,
    E[X^2] by float64 quadrature over the two uniforms."""
    import pydrobert_amd.estimators as E
    from pydrobert_amd.distributions import LogisticBernoulli
    from pydrobert_amd.modules import LogisticBernoulliRebarControlVariate

    M = 4096
    logits = torch.tensor([-1.0, -0.2, 0.4, 1.5], device=DEV)
    qlogits = torch.tensor([-0.5, 0.3, 0.0, 1.0], device=DEV)
    t = torch.tensor([0.3, -0.5, 0.8, 0.1], device=DEV)
    func = lambda b: (b - t) ** 2 + 0.5  # noqa: E731
    P = torch.distributions.Bernoulli(logits=logits)
    Q = torch.distributions.Bernoulli(logits=qlogits)
    v_exact = E.EnumerateEstimator(P, func)()
    p, q = logits.sigmoid(), qlogits.sigmoid()
    f1, f0 = func(torch.ones(4, device=DEV)), func(torch.zeros(4, device=DEV))
    torch.testing.assert_close(v_exact, p * f1 + (1 - p) * f0)
    var_f = p * (1 - p) * (f1 - f0) ** 2
    var_is = q * (f1 * p / q) ** 2 + (1 - q) * (f0 * (1 - p) / (1 - q)) ** 2 - v_exact ** 2
    eta = 0.8
    mean_relax, var_relax = relax_variance(logits.cpu().double(), t.cpu().double(), 0.5, eta)
    torch.testing.assert_close(mean_relax, v_exact.cpu().double(), rtol=0, atol=1e-6)  # (v_exact is float32)
    var_relax = var_relax.to(DEV, torch.float32)
    torch.manual_seed(20261019)
    relaxed = LogisticBernoulli(logits=logits)
    cv = LogisticBernoulliRebarControlVariate(func, 0.5, eta).to(DEV)
    runs = {
        "direct": (E.DirectEstimator(P, func, M), var_f),
        "is": (E.ImportanceSamplingEstimator(Q, func, M, P), var_is),
        "relax": (E.RelaxEstimator(relaxed, func, M, cv), var_relax),
        "st": (E.StraightThroughEstimator(relaxed, func, M), var_f),
    }
    for name, (est, var) in runs.items():
        v = est()
        assert v.shape == (4,)
        bound = 6 * (var / M).sqrt()
        print(name, ((v - v_exact).abs() / bound).tolist())
        assert bool(((v - v_exact).abs() <= bound).all()), (name, v, v_exact, bound)
    # in log space the estimate is the log of the same average
    v = E.DirectEstimator(P, lambda b: func(b).log(), M, is_log=True)()
    assert v.shape == (1, 4) and bool(((v[0].exp() - v_exact).abs() <= 6 * (var_f / M).sqrt()).all())


# ---- torch.compile and torch.jit.trace ----------------------------------------------------------------------------
def _fused(f, a, cz, lp, lq):
    x = X()
    s = x.mc_reduce(x.SCORE, True, f, a=a, cz=cz, lp=lp)
    w = x.mc_reduce(x.WEIGHTED, False, f, lp=lp, lq=lq, mode=x.W_SELF)
    m = x.mc_reduce(x.MEAN, True, f)
    idx, last, last_idx = x.imh_chain(lp - lq, lp[0] - lq[0], a)
    return s + w + m, idx, last, last_idx


def _fused_ops(f, a, cz, lp, lq):
    ops = torch.ops.pydrobert_amd
    s = ops.mc_reduce(1, True, 0, f, a, cz, None, lp, None)[0]
    w = ops.mc_reduce(2, False, 1, f, None, None, None, lp, lq)[0]
    m = ops.mc_reduce(0, True, 0, f, None, None, None, None, None)[0]
    idx, last, last_idx = ops.imh_chain(lp - lq, lp[0] - lq[0], a)
    return s + w + m, idx, last, last_idx


def _jit_inputs():
    gen = torch.Generator().manual_seed(4)
    T = draw(gen, ("f", "a", "cz", "lp", "lq"), 9, (5,), torch.float32)
    return [T[n].to(DEV) for n in ("f", "a", "cz", "lp", "lq")]


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_torch_compile_sees_the_fused_operators():
    args = _jit_inputs()
    compiled = torch.compile(_fused_ops, backend="eager", fullgraph=True)
    _same(_fused(*args), compiled(*args))
    a1 = [t.clone().requires_grad_(True) for t in args]
    a2 = [t.clone().requires_grad_(True) for t in args]
    g1 = torch.autograd.grad(_fused(*a1)[0].sum(), a1[:4])
    g2 = torch.autograd.grad(compiled(*a2)[0].sum(), a2[:4])
    _same(g1, g2)


def test_jit_trace_of_the_fused_operators():
    args = _jit_inputs()
    traced = torch.jit.trace(_fused, args, check_trace=False)
    assert "pydrobert_amd::mc_reduce" in str(traced.graph) and "pydrobert_amd::imh_chain" in str(traced.graph)
    other = [t + 0.25 for t in args]
    _same(_fused(*other), traced(*other))
    a1 = [t.clone().requires_grad_(True) for t in other]
    a2 = [t.clone().requires_grad_(True) for t in other]
    _same(torch.autograd.grad(_fused(*a1)[0].sum(), a1[:4]), torch.autograd.grad(traced(*a2)[0].sum(), a2[:4]))


def test_opcheck_registrations():
    from torch.library import opcheck

    f, a, cz, lp, lq = (t.requires_grad_(True) for t in _jit_inputs())
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    ops = torch.ops.pydrobert_amd
    opcheck(ops.mc_reduce.default, (1, True, 0, f, a, cz, None, lp, None), test_utils=tests)
    opcheck(ops.mc_reduce.default, (2, False, 1, f, None, None, None, lp, lq), test_utils=tests)
    out, stats = ops.mc_reduce(1, True, 0, f, a, cz, None, lp, None)
    g = torch.ones_like(out)
    opcheck(ops.mc_reduce_backward.default, (1, True, 0, 0b10111, g, stats, f, a, cz, None, lp, None), test_utils=tests)
    opcheck(ops.imh_chain.default, (lp.detach(), lp[0].detach(), lq.detach()), test_utils=tests)
