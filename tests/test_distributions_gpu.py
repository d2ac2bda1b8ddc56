"""GPU: the distributions namespace on the HIP kernels of csrc/relaxed.hip, and the sequence and SRSWOR
distributions on the kernels they compose.

Every continuous result of the relaxed distributions is held to tests/_distributions_ref.py (float64, clamping
at the eps of the dtype under test) within the bound the golden maker measured and stored; discrete results
are exact and computed from the golden ``z`` / ``zcond`` (tests/_distributions_check.py).  Each golden case prints
its figures, in units of eps (1 + |value|), before it asserts.

Bounds set here, with their reasons:
* the RELAX composition (float64): 1e-9 (1 + |value|).  Two differentiations through ~10 elementwise operations,
  a softmax at temperature 0.5 and sums of fewer than 100 terms amplify float64's 2.2e-16 by well under 1e4; the
  device's log / exp differ from the CPU's by an ulp or two.  1e-9 leaves two decades and is ten decades below
  what a missing term of the second derivative would cost.
* the gradient of the broadcast test: 64 eps (1 + the largest entry).  It checks where the gradient lands, not its
  last bits (the golden cases do that): a sum of at most 280 terms of a few ulp each, against a gradient of the
  wrong rows, which is off by its own size.
* sequence log probabilities (float32): 16 T eps (1 + |value|) -- T log-softmaxes over at most 8 values, each a
  few roundings of numbers below 16 in magnitude, summed.
"""
import math

import numpy as np
import pytest
import torch

import _distributions_check as C
import _distributions_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = float(torch.finfo(torch.float32).eps)


def _print(k, case, figures):
    print("case", k, case, {n: round(d, 2) for n, d in figures.items()})


@pytest.mark.parametrize("k", range(len(C.cases())), ids=lambda k: "{family}-{dtype}-{shape_index}".format(**C.cases()[k]))
def test_golden_cases(k):
    C.check_case(k, DEV, _print)


def test_cases_sit_where_the_kernels_change_form():
    """The launcher's own constants: a row belongs to pdt_relaxed_group_width(V) lanes -- 1, 2, 4, ..., 64 -- and
    beyond 64 elements a lane takes more than one; a workgroup serves pdt_relaxed_rows_per_block(V) rows."""
    from pydrobert_amd import _cabi

    lib = _cabi.lib()
    widths = sorted({lib.pdt_relaxed_group_width(v) for v in range(1, 200)})
    assert widths == [1, 2, 4, 8, 16, 32, 64]
    for family in ("gumbel", "bernoulli"):
        mine = [c for c in C.cases() if c["family"] == family and c["dtype"] == "float32"]
        Vs = {c["V"] for c in mine}
        for w in widths:  # both sides of every width, and of the first second trip
            assert w in Vs and w + 1 in Vs, (family, w)
            assert lib.pdt_relaxed_group_width(w) == w and lib.pdt_relaxed_group_width(w + 1) == min(2 * w, 64)
        assert {1, 2, 5, 64, 65, 1500} <= Vs
        rows = {(c["V"], int(np.prod(c["sample"] + c["lead"]))) for c in mine}
        assert {(5, 1), (5, 7)} <= rows
        for V in (2, 5, 65):
            assert (V, lib.pdt_relaxed_rows_per_block(V) + 1) in rows
        assert {tuple(c["sample"]) for c in mine} >= {(), (3,), (2, 2)}
        assert {tuple(c["lead"]) for c in mine} >= {(), (2,), (2, 3)}
        assert any(c["probs"] for c in mine)
    probs = torch.from_numpy(C.gold()["case_{}_param".format(
        next(k for k, c in enumerate(C.cases()) if c["V"] == 1500 and c["family"] == "gumbel"))]).softmax(-1)
    assert (probs < EPS32).any()  # (the clamp is exercised)


def _layout_case(family, dtype, param, from_probs, sample, seed):
    """One distribution over ``param`` (any layout) against the yardstick over its dense copy."""
    gen = torch.Generator().manual_seed(seed)
    eps = float(torch.finfo(dtype).eps)
    dist = C.build(family, param, from_probs)
    shape = tuple(sample) + tuple(param.shape)
    u, v = (torch.rand(shape, generator=gen, dtype=torch.float32) * 0.96 + 0.02 for _ in range(2))
    want, _ = ref.evaluate(family, ref.f64(param).cpu(), from_probs, *ref.f64(u.to(dtype), v.to(dtype)), eps,
                           grads=False)
    with C.noise(u):
        z = dist.rsample(sample)
    tol = lambda name: C.tolerance(family, name, str(dtype).split(".")[1])  # noqa: E731
    assert ref.units(z, want["z"], eps) <= tol("z")
    z_in, b = want["z"].to(dtype).to(DEV), want["b"].to(dtype).to(DEV)
    assert torch.equal(dist.threshold(z_in), b)
    with C.noise(v):
        zcond = dist.csample(b)
    assert ref.units(zcond, want["zcond"], eps) <= tol("zcond")
    assert torch.equal(dist.threshold(zcond), b)
    exact, _ = ref.evaluate(family, ref.f64(param).cpu(), from_probs, *ref.f64(u.to(dtype), v.to(dtype)), eps,
                               ref.f64(z_in).cpu(), ref.f64(b).cpu(), ref.f64(zcond).cpu(), grads=False)
    assert ref.units(dist.log_prob(z_in), exact["log_prob"], eps) <= tol("log_prob")
    assert ref.units(dist.tlog_prob(b), exact["tlog_prob"], eps) <= tol("tlog_prob")
    assert ref.units(dist.clog_prob(zcond, b), exact["clog_prob"], eps) <= tol("clog_prob")


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_layouts(family, dtype):
    gen = torch.Generator().manual_seed(11)
    base = (2 * torch.randn((3, 4, 70), generator=gen)).to(dtype).to(DEV)
    # non-contiguous: a transposed buffer, every other row, a slice of the last dimension
    for param in (base.transpose(0, 1), base[:, ::2], base[..., 3:68], base[..., ::2]):
        assert not param.is_contiguous()
        _layout_case(family, dtype, param, False, (2,), 12)
    # expanded: stride 0 in front, in the middle, everywhere
    for param in (base[0, 0].expand(2, 3, 70), base[:, :1].expand(3, 4, 70), base[:1].expand(2, 4, 70)):
        assert 0 in param.stride()
        _layout_case(family, dtype, param, False, (3,), 13)
    dist = C.build(family, base[0], False).expand([5, 4] if family == "gumbel" else [5, 4, 70])
    assert dist.logits.stride(0) == 0
    _layout_case(family, dtype, dist.logits, False, (), 14)
    # built from probabilities (Gumbel: not normalised)
    probs = base[0].softmax(-1) * 3 if family == "gumbel" else base[0].sigmoid()
    _layout_case(family, dtype, probs, True, (2,), 15)
    _layout_case(family, dtype, probs.t().contiguous().t() if family == "bernoulli" else probs[::2], True, (2,), 16)
    # a b that needs broadcasting against the batch shape
    dist = C.build(family, base[0], False)
    b = dist.threshold(base[1, :1])
    assert dist.tlog_prob(b).shape == (4,) + (() if family == "gumbel" else (70,))
    assert torch.equal(dist.tlog_prob(b), dist.tlog_prob(b.expand(base[0].shape).contiguous()))


@pytest.mark.parametrize("family,shape,data", [
    ("gumbel", (2, 1, 7), (2, 3, 7)), ("gumbel", (2, 1, 70), (4, 2, 3, 70)), ("gumbel", (1, 3, 7), (2, 3, 7)),
    ("bernoulli", (5, 1), (5, 4)), ("bernoulli", (5, 1), (3, 5, 70)), ("bernoulli", (2, 1, 7), (2, 3, 7)),
    ("bernoulli", (1, 7), (6, 7)),
], ids=lambda x: str(x))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_data_broadcast_over_size_one_batch_dimensions(family, shape, data, dtype):
    """A data argument may be larger than the parameter in a batch dimension where the parameter has size 1 (the
    reference broadcasts): every method that takes data, against the yardstick, whose broadcasting is torch's."""
    gen = torch.Generator().manual_seed(17)
    dt = str(dtype).split(".")[1]
    eps = float(torch.finfo(dtype).eps)
    logits = (2 * torch.randn(shape, generator=gen)).to(dtype)
    u, v = ((torch.rand(data, generator=gen) * 0.96 + 0.02).to(dtype) for _ in range(2))
    dist = C.build(family, logits.to(DEV), False)
    fam = ref.FAMILY[family]
    l64 = fam["logits"](ref.f64(logits), False, eps)
    z = fam["rsample"](l64, ref.f64(u), eps).to(dtype)  # (a relaxed sample of the broadcast shape)
    b = fam["threshold"](ref.f64(z)).to(dtype)
    tol = lambda name: C.tolerance(family, name, dt)  # noqa: E731
    assert torch.equal(dist.threshold(z.to(DEV)).cpu(), b)
    assert ref.units(dist.log_prob(z.to(DEV)), fam["log_prob"](l64, ref.f64(z)), eps) <= tol("log_prob")
    assert ref.units(dist.tlog_prob(b.to(DEV)), fam["tlog_prob"](l64, ref.f64(b)), eps) <= tol("tlog_prob")
    with C.noise(v):
        zcond = dist.csample(b.to(DEV))
    want = fam["csample"](fam["probs"](ref.f64(logits), False), ref.f64(b), ref.f64(v), eps)
    assert zcond.shape == tuple(data) and ref.units(zcond, want, eps) <= tol("zcond")
    assert torch.equal(dist.threshold(zcond).cpu(), b)
    got = dist.clog_prob(zcond, b.to(DEV))
    assert ref.units(got, fam["clog_prob"](l64, ref.f64(zcond).cpu(), ref.f64(b)), eps) <= tol("clog_prob")
    # and the gradient lands on the parameter's own shape
    leaf = logits.to(DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(C.build(family, leaf, False).log_prob(z.to(DEV)).sum(), leaf)
    l_leaf = ref.f64(logits).requires_grad_(True)
    (gw,) = torch.autograd.grad(fam["log_prob"](fam["logits"](l_leaf, False, eps), ref.f64(z)).sum(), l_leaf)
    assert g.shape == tuple(shape)
    assert ((g.cpu().double() - gw).abs() <= 64 * eps * (1 + gw.abs().max())).all()


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_threshold_ties_nan_mismatch_and_guard(dt):
    g = C.gold()
    dtype = getattr(torch, dt)
    eps = float(torch.finfo(dtype).eps)
    t = lambda key: torch.from_numpy(g[key]).to(DEV)  # noqa: E731
    gum = C.build("gumbel", torch.zeros(5, dtype=dtype, device=DEV), False, validate_args=False)
    assert torch.equal(gum.threshold(t("threshold_{}_z".format(dt))), t("threshold_{}_b".format(dt)))
    wide = C.build("gumbel", torch.zeros(70, dtype=dtype, device=DEV), False, validate_args=False)
    assert torch.equal(wide.threshold(t("threshold_{}_wide_z".format(dt))), t("threshold_{}_wide_b".format(dt)))
    ber = C.build("bernoulli", torch.zeros(6, dtype=dtype, device=DEV), False, validate_args=False)
    assert torch.equal(ber.threshold(t("threshold_{}_bern_z".format(dt))), t("threshold_{}_bern_b".format(dt)))
    for family in ("gumbel", "bernoulli"):
        pre = "mismatch_{}_{}_".format(family, dt)
        dist = C.build(family, t(pre + "param"), False, validate_args=False)
        got = dist.clog_prob(t(pre + "zcond"), t(pre + "b"))
        param, zc, b = ref.f64(t(pre + "param").cpu(), t(pre + "zcond").cpu(), t(pre + "b").cpu())
        want = ref.FAMILY[family]["clog_prob"](ref.FAMILY[family]["logits"](param, False, eps), zc, b)
        assert torch.equal(torch.isinf(want), torch.isinf(t(pre + "clog_prob").cpu())) and torch.isinf(want).any()
        assert not torch.isinf(want).all()
        assert ref.units(got, want, eps) <= C.tolerance(family, "clog_prob", dt)  # (-inf exactly where recorded)
    pre = "guard_{}_".format(dt)
    dist = C.build("gumbel", t(pre + "param"), False)
    with C.noise(t(pre + "v").cpu()):
        zcond = dist.csample(t(pre + "b"))
    param, b, v = ref.f64(t(pre + "param").cpu(), t(pre + "b").cpu(), t(pre + "v").cpu())
    assert ref.gumbel_guard(param.softmax(-1), b, v, eps).any()
    want = ref.gumbel_csample(param.softmax(-1), b, v, eps)
    assert ref.units(zcond, want, eps) <= C.tolerance("gumbel", "zcond", dt)
    # where |z_k| >= 2 float32 rounds z_k - eps to z_k: the guarded element ties with the hot one, as recorded
    assert torch.equal(dist.threshold(zcond), dist.threshold(t(pre + "zcond")))


GRADCHECK = [("gumbel", (2,), (2,), 3), ("gumbel", (1,), (1,), 65), ("bernoulli", (2,), (), 3)]


@pytest.mark.parametrize("family,sample,lead,V", GRADCHECK, ids=lambda x: str(x))
@pytest.mark.parametrize("from_probs", [False, True], ids=["logits", "probs"])
def test_gradcheck_and_gradgradcheck(family, sample, lead, V, from_probs):
    from torch.autograd import gradcheck, gradgradcheck

    gen = torch.Generator().manual_seed(21)
    logits = 2 * torch.randn(lead + (V,), dtype=torch.double, generator=gen)
    if from_probs:
        # (flatter: csample is -log(a / p + c), and central differences of step 1e-6 are only good to gradcheck's
        # rtol of 1e-3 where p is well above 1e-4; at 2 randn over 65 entries the smallest p is about 1e-5)
        logits = logits / 4
        param = logits.softmax(-1) if family == "gumbel" else logits.sigmoid()
    else:
        param = logits
    param = param.to(DEV).requires_grad_(True)
    shape = sample + lead + (V,)
    u, v = (torch.rand(shape, dtype=torch.double, generator=gen) * 0.96 + 0.02 for _ in range(2))
    d0 = C.build(family, param.detach(), from_probs)
    with C.noise(u, v):
        z = d0.rsample(sample)
        b = d0.threshold(z)
        zcond = d0.csample(b)
    z, zcond = z.detach().requires_grad_(True), zcond.detach().requires_grad_(True)
    dist = lambda p: C.build(family, p, from_probs)  # noqa: E731

    def rsample(p):
        with C.noise(u):
            return dist(p).rsample(sample)

    def csample(p):
        with C.noise(v):
            return dist(p).csample(b)

    for fn, args in ((rsample, (param,)), (csample, (param,)), (lambda p, z_: dist(p).log_prob(z_), (param, z)),
                     (lambda p: dist(p).tlog_prob(b), (param,)), (lambda p, z_: dist(p).clog_prob(z_, b), (param, zcond))):
        assert gradcheck(fn, args)
        assert gradgradcheck(fn, args)


def _relax(family, logits, u, v, cv, M, rsample, threshold, csample, tlog_prob, f):
    """RELAX [grathwohl2017] written out.  Stage 1: z -> b -> zcond, log p(b), and the control variate on z and
    zcond.  Stage 2: the estimate of d E[f(b)] / d logits with the graph kept, then the gradient of its squared
    norm with respect to the control variate's parameters."""
    z = rsample(logits, u)
    b = threshold(z.detach())
    zcond = csample(logits, b, v)
    log_pb = tlog_prob(logits, b)
    c, ccond = cv(z), cv(zcond)
    surrogate = ((f(b) - ccond).detach() * log_pb + c - ccond).mean(0).sum()
    (ghat,) = torch.autograd.grad(surrogate, logits, create_graph=True)
    g_temp, g_eta = torch.autograd.grad(ghat.pow(2).sum(), [cv.log_temp, cv.eta])
    return ghat.detach(), g_temp, g_eta


@pytest.mark.parametrize("family", ["gumbel", "bernoulli"])
def test_relax_composition(family):
    from pydrobert_amd import modules as M

    gen = torch.Generator().manual_seed(31)
    Ms, N, V = 4, 3, 5
    logits = 2 * torch.randn((N, V), dtype=torch.double, generator=gen)
    u, v = (torch.rand((Ms, N, V), dtype=torch.double, generator=gen) * 0.96 + 0.02 for _ in range(2))
    target = torch.nn.functional.one_hot(torch.arange(N) % V, V).double()
    eps = float(torch.finfo(torch.double).eps)
    name = C.NAMES[family] + "RebarControlVariate"
    results = []
    for device in (DEV, torch.device("cpu")):
        tgt = target.to(device)
        if family == "gumbel":
            f = lambda x: ((x - tgt) ** 2).sum(-1)  # noqa: E731
        else:  # (every element is a Bernoulli variable of its own)
            f = lambda x: (x - tgt) ** 2  # noqa: E731
        cv = getattr(M, name)(f, 0.5, 0.8).double().to(device)
        leaf = logits.to(device).requires_grad_(True)
        if device.type == "cuda":  # the code under test

            def rsample(l, u_):
                with C.noise(u_):
                    return C.build(family, l, False).rsample([Ms])

            def csample(l, b, v_):
                with C.noise(v_):
                    return C.build(family, l, False).csample(b)

            threshold = lambda z: C.build(family, leaf.detach(), False).threshold(z)  # noqa: E731
            tlog_prob = lambda l, b: C.build(family, l, False).tlog_prob(b)  # noqa: E731
        else:  # the yardstick's differentiable restatement
            fam = ref.FAMILY[family]
            rsample = lambda l, u_: fam["rsample"](fam["logits"](l, False, eps), u_, eps)  # noqa: E731
            csample = lambda l, b, v_: fam["csample"](fam["probs"](l, False), b, v_, eps)  # noqa: E731
            threshold = fam["threshold"]
            tlog_prob = lambda l, b: fam["tlog_prob"](fam["logits"](l, False, eps), b)  # noqa: E731
        results.append(_relax(family, leaf, u, v, cv, Ms, rsample, threshold, csample, tlog_prob, f))
    for name, got, want in zip(("ghat", "g_log_temp", "g_eta"), *results):
        got, want = got.cpu(), want.cpu()
        print(family, name, float(((got - want).abs() / (1 + want.abs())).max()))
        assert want.abs().max() > 1e-3, name  # (a real second derivative, not a zero)
        assert ((got - want).abs() <= 1e-9 * (1 + want.abs())).all(), name


@pytest.fixture(scope="module")
def lm():
    return C.lookup_lm(DEV)


def _seq_close(got, want, T):
    got, want = got.cpu().double(), torch.as_tensor(want).double()
    assert got.shape == want.shape
    return bool(((got - want).abs() <= 16 * T * EPS32 * (1 + want.abs())).all())


@pytest.mark.parametrize("tag", ["eos", "noeos"])
def test_sequence_distribution_log_prob_and_support(lm, tag):
    from pydrobert_amd import distributions as D
    from pydrobert_amd import modules as M

    g = C.gold()
    model, (V, sos, eos, T) = lm
    walk = M.RandomWalk(model, eos if tag == "eos" else None).to(DEV)
    flat = D.SequentialLanguageModelDistribution(walk, max_iters=T, validate_args=True)
    batched = D.SequentialLanguageModelDistribution(walk, 3, max_iters=T, validate_args=True)
    pre = "seq_{}_".format(tag)
    assert _seq_close(flat.log_prob(torch.from_numpy(g[pre + "value"]).to(DEV)), g[pre + "log_prob"], T)
    assert _seq_close(batched.log_prob(torch.from_numpy(g[pre + "value_b"]).to(DEV)), g[pre + "log_prob_b"], T)
    assert flat.has_enumerate_support
    assert np.array_equal(flat.enumerate_support().cpu().numpy(), g[pre + "support"])
    assert np.array_equal(batched.enumerate_support().cpu().numpy(), g[pre + "support_b"])
    assert tuple(batched.enumerate_support(False).shape) == tuple(g[pre + "support_b_shape"])


@pytest.mark.parametrize("tag", ["eos", "noeos"])
def test_sequence_distribution_sample(lm, tag):
    from pydrobert_amd import distributions as D
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    model, (V, sos, eos, T) = lm
    e = eos if tag == "eos" else None
    walk = M.RandomWalk(model, e).to(DEV)
    for batch_size, sample_shape, lead in ((None, (), ()), (None, (6,), (6,)), (3, (), (3,)), (3, (4,), (4, 3))):
        dist = D.SequentialLanguageModelDistribution(walk, batch_size, max_iters=T, cache_samples=True)
        s = dist.sample(sample_shape)
        assert s.dtype == torch.long and s.device.type == "cuda"
        assert s.shape[:-1] == lead and (s.shape[-1] == T if e is None else 1 <= s.shape[-1] <= T)
        assert dist.support.check(s).all()
        if e is not None:  # what follows an eos is eos
            assert torch.equal(F.fill_after_eos(s, e, -1), s)
        cached = dist.log_prob(s)
        assert cached is dist._log_probs_cache and cached.shape == lead
        dist.clear_cache()
        assert dist._samples_cache is None and dist._log_probs_cache is None
        again = dist.log_prob(s)
        assert again is not cached and _seq_close(again, cached.cpu(), T)
        assert dist.sample((0,) + tuple(sample_shape)).numel() == 0
    if e is not None:  # walks of different lengths, padded with eos: no max_iters
        dist = D.SequentialLanguageModelDistribution(walk, 5)
        s = dist.sample([6])
        assert s.shape[:2] == (6, 5) and (s == e).any(-1).all() and torch.equal(F.fill_after_eos(s, e, -1), s)
        assert not dist.has_enumerate_support


def test_srswor_distribution():
    from pydrobert_amd import distributions as D

    g = C.gold()
    total, given = torch.from_numpy(g["srswor_total"]).to(DEV), torch.from_numpy(g["srswor_given"]).to(DEV)
    dist = D.SimpleRandomSamplingWithoutReplacement(given, total, 7, validate_args=True)
    draw = dist.sample([50])
    assert draw.shape == (50, 4, 7) and draw.device.type == "cuda"
    assert torch.equal(draw.sum(-1), given.to(draw.dtype).expand(50, 4))
    tail = torch.arange(7, device=DEV) >= total.unsqueeze(-1)
    assert not (draw * tail).any() and dist.support.check(draw).all()
    assert len({tuple(r.tolist()) for r in draw[:, 0]}) > 1
    value = torch.from_numpy(g["srswor_value"]).to(DEV)
    assert np.allclose(dist.log_prob(value).cpu().numpy(), g["srswor_log_prob"], rtol=1e-6)
    for name in ("mean", "variance", "log_partition"):
        assert np.allclose(getattr(dist, name).cpu().numpy(), g["srswor_" + name], rtol=1e-6), name
    uni = D.SimpleRandomSamplingWithoutReplacement(torch.tensor([2, 2], device=DEV), 5, 6)
    assert np.array_equal(uni.enumerate_support().cpu().numpy(), g["srswor_uniform_support"])
    assert tuple(uni.enumerate_support(False).shape) == tuple(g["srswor_uniform_support_shape"])
    assert np.allclose(uni.log_prob(uni.enumerate_support()).cpu().numpy(), g["srswor_uniform_log_prob"], rtol=1e-6)
    assert math.isclose(float(uni.log_prob(uni.enumerate_support()).exp().sum(0)[0]), 1.0, rel_tol=1e-5)


def test_non_default_stream():
    """The kernels are enqueued on torch's current stream."""
    k = next(i for i, c in enumerate(C.cases()) if c["family"] == "gumbel" and c["V"] == 65 and c["dtype"] == "float32")
    case, dtype, rec = C.tensors(k)

    def run():
        dist = C.build("gumbel", rec["param"].to(DEV), case["probs"])
        with C.noise(rec["u"], rec["v"]):
            z = dist.rsample(tuple(case["sample"]))
            b = dist.threshold(z)
            zcond = dist.csample(b)
        return z, b, zcond, dist.log_prob(z), dist.tlog_prob(b), dist.clog_prob(zcond, b)

    want = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
