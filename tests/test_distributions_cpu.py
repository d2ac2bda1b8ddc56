"""CPU: the distributions namespace and the REBAR control variates against what the reference recorded
(tests/golden/make_distributions_golden.py): the torch bodies of the relaxed distributions on every golden
case, the CPU random stream, signatures, interfaces, constraints, validation, and the C ABI of the new kernels.

Tolerances are those the golden maker measured and stored (see tests/_distributions_check.py); what the
torch bodies compute with the reference's own operations is compared with its recorded values directly.
"""
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import _distributions_check as C
import _distributions_ref as ref

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_namespaces_are_the_references():
    import pydrobert_amd.distributions as D
    import pydrobert_amd.modules as M

    sigs = C.signatures()
    assert sorted(D.__all__) == sigs["distributions_all"] and len(D.__all__) == 9
    assert sorted(M.__all__) == sigs["modules_all"] and len(M.__all__) == 41
    ns = {}
    exec("from pydrobert_amd.distributions import *", ns)
    assert sorted(k for k in ns if not k.startswith("__")) == sigs["distributions_all"]
    for name in M.__all__:
        assert hasattr(M, name)


def _params(fn):
    fn = getattr(fn, "fget", fn)
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name,
             repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_signatures_of_every_public_class_and_method():
    import pydrobert_amd.distributions as D
    import pydrobert_amd.modules as M

    for cname, members in C.signatures()["classes"].items():
        cls = getattr(D, cname, None) or getattr(M, cname)
        for name, spec in members.items():
            member = inspect.getattr_static(cls, name)
            if spec[0] == "property":
                assert not inspect.isfunction(member), (cname, name)
            else:
                assert _params(member) == spec[1], (cname, name, _params(member), spec[1])


def test_dropped_cases_are_few():
    g = C.gold()
    dropped = json.loads(str(g["dropped"]))
    assert 20 * len(dropped) <= int(g["n_shapes"])
    assert 2 * (int(g["n_shapes"]) - len(dropped)) == len(C.cases())


@pytest.mark.parametrize("k", range(len(C.cases())), ids=lambda k: "{family}-{dtype}-{shape_index}".format(**C.cases()[k]))
def test_golden_cases_torch_bodies(k):
    C.check_case(k, CPU)
    # the reference's own operations: its recorded values
    case, dtype, rec = C.tensors(k)
    eps = float(torch.finfo(dtype).eps)
    dist = C.build(case["family"], rec["param"], case["probs"])
    with C.noise(rec["u"], rec["v"]):
        z = dist.rsample(tuple(case["sample"]))
        zcond = dist.csample(rec["b"])
    assert torch.equal(z, rec["z"]) and torch.equal(zcond, rec["zcond"])
    assert ref.units(dist.log_prob(rec["z"]), rec["log_prob"], eps) <= 2
    assert ref.units(dist.tlog_prob(rec["b"]), rec["tlog_prob"], eps) <= 2
    assert ref.units(dist.clog_prob(rec["zcond"], rec["b"]), rec["clog_prob"], eps) <= 2


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_seed_reproduces_the_references_cpu_stream(family, dt):
    g = C.gold()
    pre = "seed_{}_{}_".format(family, dt)
    dist = C.build(family, torch.from_numpy(g[pre + "param"]), False)
    torch.manual_seed(1234)
    z = dist.rsample([3])
    zcond = dist.csample(dist.threshold(z))
    assert torch.equal(z, torch.from_numpy(g[pre + "z"]))
    assert torch.equal(zcond, torch.from_numpy(g[pre + "zcond"]))


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_threshold_ties_nan_mismatch_and_guard(dt):
    g = C.gold()
    t = lambda key: torch.from_numpy(g[key])  # noqa: E731
    gum = C.build("gumbel", torch.zeros(5, dtype=getattr(torch, dt)), False, validate_args=False)
    assert torch.equal(gum.threshold(t("threshold_{}_z".format(dt))), t("threshold_{}_b".format(dt)))
    wide = C.build("gumbel", torch.zeros(70, dtype=getattr(torch, dt)), False, validate_args=False)
    assert torch.equal(wide.threshold(t("threshold_{}_wide_z".format(dt))), t("threshold_{}_wide_b".format(dt)))
    ber = C.build("bernoulli", torch.zeros(6, dtype=getattr(torch, dt)), False, validate_args=False)
    assert torch.equal(ber.threshold(t("threshold_{}_bern_z".format(dt))), t("threshold_{}_bern_b".format(dt)))
    for family in ("gumbel", "bernoulli"):
        pre = "mismatch_{}_{}_".format(family, dt)
        dist = C.build(family, t(pre + "param"), False, validate_args=False)
        got, want = dist.clog_prob(t(pre + "zcond"), t(pre + "b")), t(pre + "clog_prob")
        assert torch.isinf(want).any() and torch.equal(torch.isinf(got), torch.isinf(want))
        assert ref.units(got, want, float(torch.finfo(got.dtype).eps)) <= 2
    pre = "guard_{}_".format(dt)
    dist = C.build("gumbel", t(pre + "param"), False)
    with C.noise(t(pre + "v")):
        assert torch.equal(dist.csample(t(pre + "b")), t(pre + "zcond"))


def test_straight_through_threshold_and_b_with_gradient():
    z = torch.randn(3, 4, requires_grad=True)
    for family in ("gumbel", "bernoulli"):
        dist = C.build(family, torch.randn(4), False)
        b = dist.threshold(z)
        assert not b.requires_grad
        bst = dist.threshold(z, straight_through=True)
        assert torch.equal(bst.detach(), b)
        (gz,) = torch.autograd.grad(bst.sum(), z)
        assert torch.equal(gz, torch.ones_like(z))
        # a b that carries a gradient takes the reference's differentiable formulas
        (gz,) = torch.autograd.grad(dist.csample(bst).sum(), z)
        assert gz.abs().sum() > 0


def test_no_derivative_is_silently_zero():
    from pydrobert_amd import _relaxed as X

    logits = torch.randn(2, 3, dtype=torch.double)
    u = (torch.rand(2, 3, dtype=torch.double) * 0.9 + 0.05).requires_grad_(True)
    z = torch.ops.pydrobert_amd.relaxed(X.GUMBEL, X.RSAMPLE, logits, u, None)
    with pytest.raises(NotImplementedError):
        z.sum().backward()
    v = u.detach().clone().requires_grad_(True)
    b = torch.eye(3, dtype=torch.double)[:2]
    zc = torch.ops.pydrobert_amd.relaxed(X.BERNOULLI, X.CSAMPLE, logits.sigmoid(), b, v)
    with pytest.raises(NotImplementedError):
        zc.sum().backward()


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
def test_gradcheck_of_the_registered_backwards(family):
    """The backward formulas are the same on every device: first and second derivatives in float64."""
    from torch.autograd import gradcheck, gradgradcheck

    g = torch.Generator().manual_seed(5)
    logits = (2 * torch.randn(2, 3, dtype=torch.double, generator=g)).requires_grad_(True)
    u, v = (torch.rand(2, 2, 3, dtype=torch.double, generator=g) * 0.96 + 0.02 for _ in range(2))
    d0 = C.build(family, logits.detach(), False)
    with C.noise(u, v):
        z = d0.rsample([2])
        b = d0.threshold(z)
        zcond = d0.csample(b)

    def rsample(l):
        with C.noise(u):
            return C.build(family, l, False).rsample([2])

    def csample(l):
        with C.noise(v):
            return C.build(family, l, False).csample(b)

    z, zcond = z.detach().requires_grad_(True), zcond.detach().requires_grad_(True)
    for fn, args in ((rsample, (logits,)), (csample, (logits,)),
                     (lambda l, z_: C.build(family, l, False).log_prob(z_), (logits, z)),
                     (lambda l: C.build(family, l, False).tlog_prob(b), (logits,)),
                     (lambda l, z_: C.build(family, l, False).clog_prob(z_, b), (logits, zcond))):
        assert gradcheck(fn, args) and gradgradcheck(fn, args)


def test_statistics_properties_and_expand():
    g = C.gold()
    for family in ("gumbel", "bernoulli"):
        pre = "stats_{}_".format(family)
        dist = C.build(family, torch.from_numpy(g[pre + "param"]), False)
        for name in ("mean", "stddev", "variance", "probs", "logits"):
            got = getattr(dist, name)
            assert got.shape == g[pre + name].shape and np.allclose(got.numpy(), g[pre + name], rtol=1e-6), name
        assert np.allclose(dist.entropy().numpy(), g[pre + "entropy"], rtol=1e-6)
        e = dist.expand([3, 2] if family == "gumbel" else [3, 2, 5])
        assert type(e) is type(dist) and tuple(e.batch_shape) == tuple(g[pre + "expand_batch"])
        assert np.allclose(e.logits.numpy(), g[pre + "expand_logits"], rtol=1e-6)
        assert e.logits.stride(0) == 0 and e._validate_args == dist._validate_args
        assert e.rsample([2]).shape == (2,) + tuple(e.batch_shape) + tuple(e.event_shape)
        assert dist.has_rsample and not dist.has_enumerate_support
        built = C.build(family, dist.probs, True)
        assert np.allclose(built.logits.numpy(), g[pre + "logits"], rtol=1e-5, atol=1e-6)


def test_subclasshook_behaviour():
    from pydrobert_amd import distributions as D

    for cls in (D.GumbelOneHotCategorical, D.LogisticBernoulli):
        assert issubclass(cls, D.StraightThrough) and issubclass(cls, D.ConditionalStraightThrough)
        assert issubclass(cls, D.Density)
    assert issubclass(torch.distributions.Normal, D.Density)
    assert not issubclass(torch.distributions.Normal, D.StraightThrough)

    class Duck(torch.distributions.Distribution):
        has_rsample = True

        def rsample(self, sample_shape=torch.Size()):
            ...

        def threshold(self, z, straight_through=False):
            ...

        def tlog_prob(self, b):
            ...

    assert issubclass(Duck, D.StraightThrough) and not issubclass(Duck, D.ConditionalStraightThrough)

    class NoRsample(Duck):
        has_rsample = False

    assert not issubclass(NoRsample, D.StraightThrough)

    class Conditional(Duck):
        def csample(self, b):
            ...

        def clog_prob(self, zcond, b):
            ...

    assert issubclass(Conditional, D.ConditionalStraightThrough)

    class Removed(Conditional):
        csample = None

    assert not issubclass(Removed, D.ConditionalStraightThrough)
    assert not issubclass(int, D.Density)
    with pytest.raises(TypeError):
        D.StraightThrough()


def test_constraints():
    from pydrobert_amd import distributions as D

    g = C.gold()
    c = D.TokenSequenceConstraint(4, eos=1, max_iters=3)
    value = torch.tensor([[0, 2, 3], [1, 9, 9], [0, 2, 4], [0, -1, 1]])
    assert c.check(value).tolist() == [True, True, False, False]
    assert D.TokenSequenceConstraint(4, eos=1).check(torch.tensor([[0, 2], [0, 1]])).tolist() == [False, True]
    assert D.TokenSequenceConstraint(4, eos=1, max_iters=1).check(torch.tensor([[0, 1]])).tolist() == [False]
    assert D.TokenSequenceConstraint(4, max_iters=2).check(torch.tensor([[0, 3], [0, 4]])).tolist() == [True, False]
    assert D.TokenSequenceConstraint(4, max_iters=2).check(torch.tensor([[0.5, 3.0]])).tolist() == [False]
    dist = D.SimpleRandomSamplingWithoutReplacement(torch.from_numpy(g["srswor_given"]), torch.from_numpy(g["srswor_total"]), 7)
    value = torch.from_numpy(g["srswor_value"])
    got = dist.support.check(torch.stack([value[0], value[0].flip(-1)]))
    assert np.array_equal(got.numpy(), g["srswor_support_check"])
    assert not D.BinaryCardinalityConstraint(torch.tensor(2), 3).check(torch.tensor([1.0, 0.5, 0.5]))


def test_srswor_distribution_against_golden():
    from pydrobert_amd import distributions as D

    g = C.gold()
    dist = D.SimpleRandomSamplingWithoutReplacement(torch.from_numpy(g["srswor_given"]), torch.from_numpy(g["srswor_total"]), 7)
    value = torch.from_numpy(g["srswor_value"])
    assert np.allclose(dist.log_prob(value).numpy(), g["srswor_log_prob"], rtol=1e-6)
    for name in ("mean", "variance", "log_partition"):
        assert np.allclose(getattr(dist, name).numpy(), g["srswor_" + name], rtol=1e-6), name
    draw = dist.sample([5])
    assert draw.shape == (5, 4, 7) and dist.support.check(draw).all()
    uni = D.SimpleRandomSamplingWithoutReplacement(torch.tensor([2, 2]), 5, 6)
    assert np.array_equal(uni.enumerate_support().numpy(), g["srswor_uniform_support"])
    assert tuple(uni.enumerate_support(False).shape) == tuple(g["srswor_uniform_support_shape"])
    assert np.allclose(uni.log_prob(uni.enumerate_support()).numpy(), g["srswor_uniform_log_prob"], rtol=1e-6)
    assert [dist.has_enumerate_support, uni.has_enumerate_support] == g["srswor_has_enumerate"].tolist()
    e = dist.expand([3, 4])
    assert tuple(e.batch_shape) == (3, 4) and e.sample().shape == (3, 4, 7)


def test_validation_errors_by_type_name():
    from pydrobert_amd import distributions as D
    from pydrobert_amd import modules as M

    t = torch.tensor
    G, L = D.GumbelOneHotCategorical, D.LogisticBernoulli
    lm = M.LookupLanguageModel(4, 0)
    f = lambda x: x.sum(-1)  # noqa: E731
    cases = {
        "gumbel_neither": lambda: G(),
        "gumbel_both": lambda: G(logits=torch.zeros(3), probs=torch.ones(3) / 3),
        "gumbel_scalar_logits": lambda: G(logits=t(0.0)),
        "gumbel_scalar_probs": lambda: G(probs=t(1.0)),
        "gumbel_not_tensor": lambda: G(logits=[0.0, 1.0]),
        "bernoulli_neither": lambda: L(),
        "bernoulli_both": lambda: L(probs=t([0.5]), logits=t([0.0])),
        "bernoulli_not_tensor": lambda: L(logits=0.5),
        "gumbel_b_not_one_hot": lambda: G(logits=torch.zeros(3), validate_args=True).tlog_prob(t([1.0, 1.0, 0.0])),
        "gumbel_b_event_shape": lambda: G(logits=torch.zeros(3), validate_args=True).csample(t([1.0, 0.0])),
        "gumbel_b_batch_shape": lambda: G(logits=torch.zeros(2, 3), validate_args=True).csample(torch.eye(3)),
        "gumbel_b_not_tensor": lambda: G(logits=torch.zeros(3), validate_args=True).tlog_prob([1.0, 0.0, 0.0]),
        "bernoulli_b_not_boolean": lambda: L(logits=torch.zeros(3), validate_args=True).tlog_prob(t([1.0, 0.5, 0.0])),
        "bernoulli_z_nan": lambda: L(logits=torch.zeros(2), validate_args=True).log_prob(t([0.0, float("nan")])),
        "cv_temp_zero": lambda: M.LogisticBernoulliRebarControlVariate(f, 0.0),
        "cv_temp_str": lambda: M.GumbelOneHotCategoricalRebarControlVariate(f, "a"),
        "cv_eta_str": lambda: M.GumbelOneHotCategoricalRebarControlVariate(f, 0.1, "a"),
        "constraint_neither": lambda: D.TokenSequenceConstraint(4),
        "constraint_vocab_zero": lambda: D.TokenSequenceConstraint(0, 1),
        "constraint_max_iters_negative": lambda: D.TokenSequenceConstraint(4, None, -1),
        "seq_no_eos_no_max_iters": lambda: D.SequentialLanguageModelDistribution(M.RandomWalk(lm)),
        "seq_batch_size_zero": lambda: D.SequentialLanguageModelDistribution(M.RandomWalk(lm, 1), 0),
        "seq_cache_samples_int": lambda: D.SequentialLanguageModelDistribution(M.RandomWalk(lm, 1), cache_samples=1),
        "seq_initial_state": lambda: D.SequentialLanguageModelDistribution(
            M.RandomWalk(lm, 1), initial_state={"a": 1}, validate_args=True),
        "seq_enumerate_without_max_iters": lambda: D.SequentialLanguageModelDistribution(
            M.RandomWalk(lm, 1)).enumerate_support(),
        "srswor_given_exceeds": lambda: D.SimpleRandomSamplingWithoutReplacement(t([3]), t([2]), validate_args=True),
        "srswor_out_size_small": lambda: D.SimpleRandomSamplingWithoutReplacement(t([1]), t([4]), 3, validate_args=True),
        "srswor_negative": lambda: D.SimpleRandomSamplingWithoutReplacement(t([-1]), t([4]), validate_args=True),
        "srswor_enumerate_mixed": lambda: D.SimpleRandomSamplingWithoutReplacement(t([1, 2]), t([4, 4])).enumerate_support(),
        "cardinality_negative": lambda: D.BinaryCardinalityConstraint(t([-1]), 3),
        "cardinality_tmax_zero": lambda: D.BinaryCardinalityConstraint(t([1]), 0),
    }
    want = json.loads(str(C.gold()["errors"]))
    assert sorted(cases) == sorted(want)
    for key, fn in cases.items():
        try:
            fn()
            got = "none"
        except Exception as e:  # noqa: BLE001
            got = type(e).__name__
        assert got == want[key], (key, got, want[key])


@pytest.mark.parametrize("name", ["LogisticBernoulliRebarControlVariate", "GumbelOneHotCategoricalRebarControlVariate"])
def test_control_variates(name):
    from pydrobert_amd import modules as M

    g = C.gold()
    f = lambda x: (x * x).sum(-1)  # noqa: E731
    cv = getattr(M, name)(f, 0.3, 1.5)
    z = torch.from_numpy(g["cv_{}_z".format(name)])
    assert np.allclose(cv(z).detach().numpy(), g["cv_{}_out".format(name)], rtol=1e-6)
    assert np.allclose(cv.log_temp.detach().numpy(), g["cv_{}_log_temp".format(name)])
    assert cv.extra_repr() == str(g["cv_{}_repr".format(name)])
    with torch.no_grad():
        cv.log_temp.fill_(7.0)
        cv.eta.fill_(-3.0)
    cv.reset_parameters()
    assert math.isclose(cv.log_temp.item(), math.log(0.3), rel_tol=1e-6) and cv.eta.item() == 1.5
    default = getattr(M, name)(f)
    assert default.start_temp == 0.1 and default.start_eta == 1.0
    traced = torch.jit.trace(cv, (z,))
    z2 = torch.randn(4, 5)
    assert torch.allclose(traced(z2), cv(z2))
    # twice differentiable in z, log_temp and eta
    zd = z.double().requires_grad_(True)
    cvd = getattr(M, name)(f, 0.3, 1.5).double()
    (gz,) = torch.autograd.grad(cvd(zd).sum(), zd, create_graph=True)
    gg = torch.autograd.grad(gz.pow(2).sum(), [cvd.log_temp, cvd.eta])
    assert all(torch.isfinite(x).all() and x.abs().sum() > 0 for x in gg)


def test_new_symbols_exported_and_declared():
    from pydrobert_amd import _cabi

    names = ("pdt_relaxed_gumbel", "pdt_relaxed_bernoulli", "pdt_relaxed_group_width", "pdt_relaxed_rows_per_block")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdt_amd.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for n in names:
        assert n in _cabi.SIGNATURES and re.search(r"\b" + n + r"\s*\(", header) and hasattr(lib, n)
    assert lib.pdt_amd_abi_version() == _cabi.ABI_VERSION
    assert [lib.pdt_relaxed_group_width(v) for v in (0, 1, 2, 3, 5, 33, 64, 65, 1500)] == [0, 1, 2, 4, 8, 64, 64, 64, 64]
    assert [lib.pdt_relaxed_rows_per_block(v) for v in (1, 5, 65)] == [256, 32, 4]


def test_argument_validation_before_any_launch():
    from pydrobert_amd import _cabi

    lib = _cabi.lib()
    OK, ARG = _cabi.PDT_OK, _cabi.PDT_E_ARG
    for fn in (lib.pdt_relaxed_gumbel, lib.pdt_relaxed_bernoulli):
        for op in range(6):
            assert fn(op, 0, 0, 1, 0, 1, 0, 0, 0, 5, 0, 0) == OK  # R == 0
            assert fn(op, 1, 0, 1, 0, 1, 0, 0, 3, 0, 0, 0) == OK  # V == 0
            assert fn(op, 0, 0, 1, 0, 1, 0, 0, 3, 5, 0, 0) == ARG  # null pointers
            assert fn(op, 2, 0, 1, 0, 1, 0, 0, 0, 5, 0, 0) == ARG  # bad dtype
            assert fn(op, -1, 0, 1, 0, 1, 0, 0, 0, 5, 0, 0) == ARG
            assert fn(op, 0, 0, 1, 0, 1, 0, 0, -1, 5, 0, 0) == ARG  # negative sizes
        assert fn(6, 0, 0, 1, 0, 1, 0, 0, 0, 5, 0, 0) == ARG and fn(-1, 0, 0, 1, 0, 1, 0, 0, 0, 5, 0, 0) == ARG  # bad op
        assert fn(0, 0, 0, 1, 0, 1, 0, 0, 1, 2 ** 31, 0, 0) != OK
