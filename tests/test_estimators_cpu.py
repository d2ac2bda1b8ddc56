"""CPU: the estimators namespace against what the reference recorded (tests/golden/make_estimators_golden.py): the
torch bodies on every golden case, signatures, validation, the two documented departures of the IMH estimator,
its chunking, the variance-minimising branch of RELAX, and the C ABI of the new kernels.

Tolerances are those the golden maker measured and stored (tests/_estimators_check.py); where a torch body runs
the reference's own operations in the reference's order the recorded values are compared directly.
"""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import _estimators_check as C
import _estimators_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_namespace_is_the_references():
    import pydrobert_amd.estimators as E

    assert sorted(E.__all__) == C.signatures()["estimators_all"] and len(E.__all__) == 10
    for name in E.__all__:
        assert hasattr(E, name), name


def test_signatures_match_the_reference():
    import pydrobert_amd.estimators as E

    for name, methods in C.signatures()["classes"].items():
        cls = getattr(E, name)
        for method, want in methods.items():
            fn = getattr(cls, method)
            got = [[p.name, p.default is not inspect.Parameter.empty, p.kind.name,
                    repr(p.default) if p.default is not inspect.Parameter.empty else None]
                   for p in inspect.signature(fn).parameters.values() if p.name != "self"]
            assert got == want, (name, method, got, want)


def test_config_and_argcheck_additions():
    from pydrobert_amd import argcheck, config

    assert config.EPS_NINF == ref.EPS_NINF and config.EPS_INF == ref.EPS_INF
    assert config.EPS_0 == math.log1p(-2 * 1.1920928955078125e-07)
    assert argcheck.is_a(3, int, "x") == 3 and argcheck.is_a(None, int, "x", True) is None
    with pytest.raises(ValueError, match=r"x \(3\) is not a str"):
        argcheck.is_a(3, str, "x")
    with pytest.raises(ValueError, match=r"is not an int"):
        argcheck.is_a("a", int, "x")
    assert argcheck.is_lt(1, 2, "a", "b") == 1
    with pytest.raises(ValueError, match=r"a \(2\) is not less than b \(2\)"):
        argcheck.is_lt(2, 2, "a", "b")


@pytest.mark.parametrize("k", range(len(C.cases())))
def test_golden_case_through_the_torch_bodies(k):
    case = C.cases()[k]
    exact = case["est"] in C.EXACT_ON_CPU and not (case["est"] == "direct" and case["cv"] and case["is_log"])
    # (log-space Direct with a control variate: autograd adds the three gradients of the column maximum in another
    # order than in the reference's graph; the stored tolerance then)
    C.check_case(k, "cpu", exact=exact)
    if exact:
        C.check_case(k, "cpu")


def test_golden_file_covers_what_the_issue_lists():
    cases = C.cases()
    assert len(cases) % 2 == 0 and not ref_dropped_too_many()
    seen = {(c["est"], c["is_log"]) for c in cases}
    for est in ("direct", "reparam", "st", "is", "relax", "imh", "enumerate"):
        assert (est, False) in seen and (est, True) in seen, est
    assert {c["cv"] for c in cases if c["est"] == "direct"} == {False, True}
    assert {c["self_normalize"] for c in cases if c["est"] == "is"} == {False, True}
    assert {c["burn_in"] > 0 for c in cases if c["est"] == "imh"} == {False, True}
    for a, b in zip(cases[::2], cases[1::2]):
        assert a["dtype"] == "float32" and b["dtype"] == "float64" and dict(a, dtype=0) == dict(b, dtype=0)
    assert max(c["M"] for c in cases) <= 65 and max(math.prod(c["batch"]) for c in cases) <= 12


def ref_dropped_too_many():
    import json

    dropped = json.loads(str(C.gold()["dropped"]))
    return 20 * len(dropped) > len(C.cases()) // 2 + len(dropped)


def _bern(n=4):
    return torch.distributions.Bernoulli(logits=torch.zeros(n))


def test_constructor_validation():
    import pydrobert_amd.estimators as E
    from pydrobert_amd.distributions import LogisticBernoulli

    f = lambda b: b  # noqa: E731
    with pytest.raises(ValueError, match="proposal .* is not a Distribution"):
        E.DirectEstimator("a", f, 3)
    with pytest.raises(ValueError, match="mc_samples"):
        E.DirectEstimator(_bern(), f, 0)
    with pytest.raises(ValueError, match="is_log"):
        E.DirectEstimator(_bern(), f, 3, is_log=1)
    with pytest.raises(ValueError, match="cv_mean"):
        E.DirectEstimator(_bern(), f, 3, cv_mean=1.0)
    with pytest.raises(ValueError, match="proposal must implement rsample"):
        E.ReparameterizationEstimator(_bern(), f, 3)
    with pytest.raises(ValueError, match="is not a StraightThrough"):
        E.StraightThroughEstimator(_bern(), f, 3)
    with pytest.raises(ValueError, match="is not a ConditionalStraightThrough"):
        E.RelaxEstimator(_bern(), f, 3, f)
    with pytest.raises(ValueError, match="either both proposal_params and cv_params"):
        E.RelaxEstimator(LogisticBernoulli(logits=torch.zeros(2)), f, 3, f, proposal_params=[torch.zeros(1)])
    with pytest.raises(ValueError, match="self_normalize"):
        E.ImportanceSamplingEstimator(_bern(), f, 3, _bern(), self_normalize=None)
    with pytest.raises(ValueError, match="enumerate its support"):
        E.EnumerateEstimator(torch.distributions.Normal(0.0, 1.0), f)
    with pytest.raises(ValueError, match="burn_in .* is not less than mc_samples"):
        E.IndependentMetropolisHastingsEstimator(_bern(), f, 3, _bern(), burn_in=3)
    with pytest.raises(ValueError, match="burn_in"):
        E.IndependentMetropolisHastingsEstimator(_bern(), f, 3, _bern(), burn_in=-1)
    with pytest.raises(ValueError, match="initial_sample_tries must be positive"):
        E.IndependentMetropolisHastingsEstimator(_bern(), f, 3, _bern(), initial_sample_tries=0)
    with pytest.raises(TypeError):
        E.Estimator(_bern(), f)  # (abstract)


class _Half(torch.distributions.Bernoulli):
    """A density whose support is b = 1 only."""

    def log_prob(self, value):
        return torch.where(value > 0, torch.zeros_like(value), torch.full_like(value, -math.inf))


def test_departure_initial_sample_is_accepted_and_validated():
    import pydrobert_amd.estimators as E

    f = lambda b: b  # noqa: E731
    prop, density = _bern(), _Half(logits=torch.zeros(4))
    for init in (torch.ones(4), torch.ones(1, 4)):
        est = E.IndependentMetropolisHastingsEstimator(prop, f, 5, density, initial_sample=init)
        assert est.initial_sample.shape == (1, 4)
        assert est().shape == (4,)
    with pytest.raises(ValueError, match="Expected initial_sample to have shape"):
        E.IndependentMetropolisHastingsEstimator(prop, f, 5, density, initial_sample=torch.ones(3))
    with pytest.raises(ValueError, match="must lie in the support of density"):
        E.IndependentMetropolisHastingsEstimator(prop, f, 5, density, initial_sample=torch.zeros(4))


def test_departure_a_rejected_minus_inf_leaves_the_chain_moving():
    """Proposal 0 is outside the support (ratio -inf) and is rejected; the reference's blend would leave NaN as the
    chain's ratio and never accept again.  Here proposal 1, better than the start, is accepted."""
    from pydrobert_amd import _estimators as X

    ratio = torch.tensor([[-math.inf], [1.0], [0.5]])
    log_u = torch.tensor([[-1.0], [-0.5], [-0.1]])
    idx, last, last_idx = X.imh_chain(ratio, torch.tensor([0.0]), log_u)
    assert idx.flatten().tolist() == [-1, 1, 1] and last.item() == 1.0 and last_idx.item() == 1
    want = ref.imh_loop(ratio, torch.tensor([0.0]), log_u)
    assert torch.equal(idx, want[0]) and torch.equal(last, want[1]) and torch.equal(last_idx, want[2])
    # through the estimator: samples 0 are outside the support, samples 1 inside
    import pydrobert_amd.estimators as E

    rows = torch.tensor([[1.0], [0.0], [1.0], [0.0], [1.0]])
    prop = _ReplayBernoulli(torch.zeros(1), rows)
    est = E.IndependentMetropolisHastingsEstimator(prop, lambda b: b + 2.0, 4, _Half(logits=torch.zeros(1)))
    with ref.noise(torch.full((4, 1), 0.5)):
        v = est()
    assert torch.equal(v, torch.tensor([3.0]))  # (the chain never leaves b = 1, and is never NaN)


class _ReplayBernoulli(ref.ReplayCategorical):
    def __init__(self, logits, rows):
        torch.distributions.Distribution.__init__(self, logits.shape, validate_args=False)
        self.logits, self.rows, self.at = logits, rows, 0

    def log_prob(self, value):
        return -torch.nn.functional.binary_cross_entropy_with_logits(self.logits.expand_as(value), value, reduction="none")


@pytest.mark.parametrize("is_log", [False, True])
@pytest.mark.parametrize("burn_in", [0, 9])
def test_imh_chunks_agree_with_one_chunk(is_log, burn_in, monkeypatch):
    from pydrobert_amd import _estimators as X
    import pydrobert_amd.estimators as E

    g = torch.Generator().manual_seed(3)
    M, batch, V = 23, (2, 3), 5
    plog, qlog = torch.randn(batch + (V,), generator=g), torch.randn(batch + (V,), generator=g)
    rows = torch.randint(0, V, (M + 1,) + batch, generator=g)
    u = torch.rand((M,) + batch, generator=g)
    w = torch.randn(V, generator=g)
    calls = []

    def func(b):
        calls.append(b.size(0))
        return w[b]

    def run():
        est = E.IndependentMetropolisHastingsEstimator(
            ref.ReplayCategorical(qlog, rows), func, M, torch.distributions.Categorical(logits=plog), burn_in, is_log=is_log)
        with ref.noise(u):
            return est()

    one = run()
    assert calls == [M - burn_in]
    del calls[:]
    monkeypatch.setattr(X, "IMH_CHUNK_BYTES", 6 * 8 * 5)  # five steps of six int64 samples
    many = run()
    assert len(calls) >= 3 and sum(calls) == M - burn_in
    torch.testing.assert_close(many, one, rtol=1e-5, atol=1e-6)
    lp, lq = (torch.distributions.Categorical(logits=x).log_prob(rows) for x in (plog, qlog))
    ratio = (lp - lq).reshape(M + 1, -1)
    idx, _, _ = ref.imh_loop(ratio[1:], ratio[0], u.log().reshape(M, -1))
    chain = w[rows].reshape(M + 1, -1).gather(0, idx[burn_in:].long() + 1).double()
    want = ref.reduce64(ref.MEAN, is_log, 0, torch.float32, chain).reshape(batch)
    assert ref.units(many, want, 2.0 ** -23) <= C.tolerance("imh", "v", "float32")


def test_varmin_attaches_a_gradient_to_cv_params():
    import pydrobert_amd.estimators as E
    from pydrobert_amd.distributions import LogisticBernoulli
    from pydrobert_amd.modules import LogisticBernoulliRebarControlVariate

    logits = torch.randn(5, dtype=torch.double).requires_grad_(True)
    func = lambda x: (x - 0.3) ** 2  # noqa: E731
    grads = {}
    for varmin in (False, True):
        torch.manual_seed(7)
        cv = LogisticBernoulliRebarControlVariate(func, 0.5, 0.8).double()
        kw = dict(proposal_params=(logits,), cv_params=(cv.log_temp, cv.eta)) if varmin else {}
        v = E.RelaxEstimator(LogisticBernoulli(logits=logits), func, 16, cv, **kw)()
        assert v.shape == (5,)
        v.sum().backward()
        grads[varmin] = (cv.log_temp.grad.clone(), cv.eta.grad.clone())
        assert all(torch.isfinite(g).all() for g in grads[varmin])
    assert not torch.allclose(grads[True][0], grads[False][0]) and not torch.allclose(grads[True][1], grads[False][1])


def test_direct_log_result_keeps_the_references_leading_dimension():
    import pydrobert_amd.estimators as E

    v = E.DirectEstimator(_bern(), lambda b: b, 3, is_log=True)()
    assert v.shape == (1, 4)
    assert E.DirectEstimator(_bern(), lambda b: b, 3)().shape == (4,)


def test_direct_with_cv_needs_cv_mean_as_in_the_reference():
    import pydrobert_amd.estimators as E

    for is_log, error in ((False, TypeError), (True, AttributeError)):
        with pytest.raises(error):
            E.DirectEstimator(_bern(), lambda b: b + 1, 3, cv=lambda b: b, is_log=is_log)()


def test_torch_bodies_serve_other_dtypes():
    from pydrobert_amd import _estimators as X

    f = torch.randn(5, 3, dtype=torch.bfloat16)
    assert X.mc_reduce(X.MEAN, False, f).dtype == torch.bfloat16
    lp = torch.randn(5, 3, dtype=torch.bfloat16, requires_grad=True)
    X.mc_reduce(X.SCORE, True, f, lp=lp).sum().backward()
    assert lp.grad is not None


# ---- the C ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_declared():
    from pydrobert_amd import _cabi

    names = ("pdt_mc_reduce", "pdt_mc_reduce_backward", "pdt_mc_reduce_plan", "pdt_imh_chain")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdt_amd.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for n in names:
        assert n in _cabi.SIGNATURES and re.search(r"\b" + n + r"\s*\(", header) and hasattr(lib, n)
    assert lib.pdt_amd_abi_version() == _cabi.ABI_VERSION


def test_plan_returns_every_form_over_the_parity_shapes():
    from pydrobert_amd import _cabi
    from pydrobert_amd import _estimators as X

    lib = _cabi.lib()
    forms = {}
    for M, B, layout in C.PARITY_SHAPES:
        s_m, s_b = (B, 1) if layout == "dense" else (1, M)
        forms.setdefault(lib.pdt_mc_reduce_plan(M, B, s_m, s_b), []).append((M, B, layout))
    assert sorted(forms) == [X.FORM_COLUMNS, X.FORM_WAVE], forms
    # columns (fewer than 64 samples, or 16384 columns and more): one wave and less, two waves, a second workgroup
    # (256 columns each); columns shorter than the unrolled eight, and eight and a remainder
    cols = forms[X.FORM_COLUMNS]
    assert any(B < 64 for _, B, _ in cols) and any(64 < B <= 256 for _, B, _ in cols) and any(B > 256 for _, B, _ in cols)
    assert any(M < 8 for M, _, _ in cols) and any(M > 8 and M % 8 for M, _, _ in cols)
    assert any(M >= 64 and B >= 16384 for M, B, _ in cols)  # the columns form where the wave form stops
    # wave: exactly one trip of the lanes and one more, a part workgroup (4 columns each) and more than one
    wave = forms[X.FORM_WAVE]
    assert any(M == 64 for M, _, _ in wave) and any(M == 65 for M, _, _ in wave) and any(M > 1000 for M, _, _ in wave)
    assert any(B < 4 for _, B, _ in wave) and any(B > 4 and B % 4 for _, B, _ in wave)
    assert any(layout == "transposed" for _, _, layout in wave) and any(layout == "dense" for _, _, layout in wave)
    plan = lib.pdt_mc_reduce_plan
    assert plan(0, 4, 4, 1) == -1 and plan(4, 0, 1, 1) == -1
    assert plan(63, 1, 1, 1) == X.FORM_COLUMNS and plan(64, 1, 1, 1) == X.FORM_WAVE
    assert plan(64, 16383, 16383, 1) == X.FORM_WAVE and plan(64, 16384, 16384, 1) == X.FORM_COLUMNS
    assert plan(64, 16384, 1, 64) == X.FORM_WAVE and plan(63, 16384, 1, 63) == X.FORM_COLUMNS


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from pydrobert_amd import _cabi

    lib = _cabi.lib()
    E = _cabi.PDT_E_ARG
    P = ctypes.c_void_p
    x = (ctypes.c_double * 8)()
    one = ctypes.addressof(x)
    strides = (ctypes.c_int64 * 12)(*([1, 1] * 6))

    def ins(*present):
        return (P * 6)(*[one if i in present else None for i in range(6)])

    def fwd(kind, is_log, mode, dtype, M, B, in_, strides_=strides, out=one, stats=one):
        return lib.pdt_mc_reduce(kind, is_log, mode, dtype, M, B, in_, strides_, out, stats, None)

    assert fwd(3, 0, 0, 0, 1, 1, ins(0)) == E and fwd(-1, 0, 0, 0, 1, 1, ins(0)) == E  # kind
    assert fwd(0, 2, 0, 0, 1, 1, ins(0)) == E  # is_log
    assert fwd(0, 0, 0, 2, 1, 1, ins(0)) == E  # dtype
    assert fwd(0, 0, 0, 0, 0, 1, ins(0)) == E and fwd(0, 0, 0, 0, 1, -1, ins(0)) == E  # M, B
    assert fwd(0, 0, 0, 0, 1, 1, None) == E and fwd(0, 0, 0, 0, 1, 1, ins(0), None) == E
    assert fwd(0, 0, 0, 0, 1, 0, ins(0)) == _cabi.PDT_OK  # nothing to do
    assert fwd(0, 0, 0, 0, 1, 1, ins()) == E  # no f
    assert fwd(0, 0, 0, 0, 1, 1, ins(0), out=None) == E and fwd(0, 0, 0, 0, 1, 1, ins(0), stats=None) == E
    assert fwd(0, 0, 0, 0, 1, 1, ins(0, 4)) == E  # MEAN takes f alone
    assert fwd(1, 0, 0, 0, 1, 1, ins(0)) == E  # SCORE without lp
    assert fwd(1, 0, 0, 0, 1, 1, ins(0, 3, 4)) == E and fwd(1, 0, 0, 0, 1, 1, ins(0, 2, 4)) == E  # c or cz without a
    assert fwd(1, 0, 0, 0, 1, 1, ins(0, 1, 2, 3, 4)) == E and fwd(1, 0, 0, 0, 1, 1, ins(0, 4, 5)) == E
    assert fwd(2, 0, 3, 0, 1, 1, ins(0, 4, 5)) == E  # mode
    assert fwd(2, 0, 0, 0, 1, 1, ins(0, 4)) == E and fwd(2, 0, 2, 0, 1, 1, ins(0, 4, 5)) == E  # lq against the mode
    assert fwd(2, 0, 1, 0, 1, 1, ins(0, 5)) == E and fwd(2, 0, 1, 0, 1, 1, ins(0, 1, 4, 5)) == E

    def bwd(kind, in_, grads, g=one, stats=one, M=1, B=1):
        return lib.pdt_mc_reduce_backward(kind, 0, 0, 0, M, B, in_, strides, g, stats, grads, None)

    assert bwd(0, ins(0), ins(0), g=None) == E and bwd(0, ins(0), None) == E and bwd(0, ins(0), ins(0), stats=None) == E
    assert bwd(0, ins(0), ins(0, 1)) == E  # a gradient for an absent input
    assert bwd(5, ins(0), ins(0)) == E and bwd(0, ins(0), ins(0), M=0) == E
    assert bwd(0, ins(0), ins(0), B=0) == _cabi.PDT_OK

    def imh(dtype=0, ratio=one, ratio0=one, log_u=one, M=1, B=1, idx=one, last=one, last_idx=one):
        return lib.pdt_imh_chain(dtype, ratio, 1, 1, ratio0, 1, log_u, 1, 1, M, B, idx, last, last_idx, None)

    assert imh(dtype=2) == E and imh(M=-1) == E and imh(B=-1) == E
    for name in ("ratio", "ratio0", "log_u", "idx", "last", "last_idx"):
        assert imh(**{name: None}) == E, name
    assert imh(B=0) == _cabi.PDT_OK
    assert imh(M=2**31) == _cabi.PDT_E_TOO_LONG
