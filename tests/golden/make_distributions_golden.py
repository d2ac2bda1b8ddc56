#!/usr/bin/env python
"""Generate tests/golden/distributions.npz and distributions_signatures.json from the LIVE reference's
distributions namespace and its REBAR control variates.

Run where the reference is checked out (it never travels to the GPU box), PDT_REFERENCE naming its root:

    python tests/golden/make_distributions_golden.py

Every array is DATA: inputs this script draws and what the reference returned for them.  While the reference
runs, ``torch.rand`` / ``torch.rand_like`` hand out the recorded noise ``u`` / ``v`` of the case, so each case
stores its noise with its outputs; the ``seed_*`` cases run without substitution and record the CPU stream.

Inputs are drawn in float32 and widened for the float64 twin of a case (which follows it and does not store
them again), so both dtypes see the same numbers:
u, v in [0.02, 0.98], logits 2 randn.  A gradient case is kept only if no element of its ``csample`` met the
``min`` guard and float32 and float64 thresholded to the same ``b``; the others are listed under ``dropped``.

Tolerances.  For every continuous output, and for its gradient (against the cos(0.7 n) upstream, with respect
to the distribution's own logits / probs, the yardstick evaluated at the values those tensors have in the
reference's distribution), the largest deviation of the reference from tests/_distributions_ref.py on the same
inputs is measured in units of eps (1 + |value|), eps the case's dtype's, and 4x that, 4 units at least, is
stored as ``tol_<family>_<output>_<dtype>`` / ``tol_<family>_g_<output>_<dtype>``: the device's log / exp are
good to 1-2 ulp where the CPU's are within 1, and the chains are two to three transcendentals deep.
"""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("PDT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pydrobert.torch.distributions as RD  # noqa: E402
import pydrobert.torch.modules as RM  # noqa: E402

import _distributions_ref as ref  # noqa: E402

warnings.simplefilter("ignore")
out = {}
DTYPES = ("float32", "float64")
CLASSES = {"gumbel": RD.GumbelOneHotCategorical, "bernoulli": RD.LogisticBernoulli}


def put(key, v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    out[key] = np.asarray(v)


class Noise:
    """``with Noise(u, v):`` -- torch.rand and torch.rand_like return the given tensors, in order."""

    def __init__(self, *tensors):
        self.queue = list(tensors)

    def __enter__(self):
        self.saved = torch.rand, torch.rand_like
        torch.rand = lambda shape, **kw: self.pop(tuple(shape), kw.get("dtype"))
        torch.rand_like = lambda t, **kw: self.pop(tuple(t.shape), t.dtype)
        return self

    def pop(self, shape, dtype):
        t = self.queue.pop(0)
        assert tuple(t.shape) == shape and t.dtype == dtype, (t.shape, shape, t.dtype, dtype)
        return t.clone()

    def __exit__(self, *exc):
        torch.rand, torch.rand_like = self.saved
        assert exc[0] is not None or not self.queue


# (sample_shape, leading batch shape, V, built from probs).  V is the event size of the Gumbel cases and the last
# batch dimension of the logistic ones.  V on both sides of every group width of csrc/relaxed.hip (1, 2, 4, ...,
# 64) and 65; row counts 1, 7 and one more than a workgroup serves (256 / width: 129 at V = 2, 33 at V = 5, 5 at
# V = 65); V = 1500 has probabilities below float32's eps.
SHAPES = [
    ((), (), 1, False), ((3,), (2,), 2, False), ((2, 2), (2, 3), 3, False), ((), (2,), 4, False),
    ((3,), (2, 3), 5, False), ((2, 2), (), 8, False), ((), (2, 3), 9, False), ((3,), (), 16, False),
    ((2, 2), (2,), 17, False), ((3,), (2,), 32, False), ((), (2,), 33, False), ((2,), (2,), 64, False),
    ((3,), (2,), 65, False),
    ((), (), 5, False), ((7,), (), 5, False), ((33,), (), 5, False), ((5,), (), 65, False), ((129,), (), 2, False),
    ((3,), (2,), 5, True), ((2,), (), 65, True),
    ((), (), 1500, False),
]


def draw(gen, shape, lo=0.02, hi=0.98):
    return torch.rand(shape, generator=gen, dtype=torch.float32) * (hi - lo) + lo


def run_case(family, dtype, param32, from_probs, sample, u32, v32, grads=True):
    """The reference on one case: dict of its inputs and outputs in ``dtype``, and its deviations (units)."""
    eps = float(torch.finfo(dtype).eps)
    param = param32.to(dtype).requires_grad_(grads)
    u, v = u32.to(dtype), v32.to(dtype)
    dist = CLASSES[family](**{"probs" if from_probs else "logits": param})
    with Noise(u, v):
        z = dist.rsample(sample)
        b = dist.threshold(z)
        zcond = dist.csample(b)
    got = dict(z=z, zcond=zcond, log_prob=dist.log_prob(z.detach()), tlog_prob=dist.tlog_prob(b),
               clog_prob=dist.clog_prob(zcond.detach(), b))
    rec = dict(param=param, u=u, v=v, b=b, **got)
    at = dict(logits=ref.f64(dist.logits), probs=ref.f64(dist.probs)) if grads else None
    want, gw = ref.evaluate(family, ref.f64(param), from_probs, *ref.f64(u, v), eps, *ref.f64(z, b, zcond),
                            grads=grads, at=at)
    dev = {k: ref.units(got[k], want[k], eps) for k in ref.CONTINUOUS}
    if grads:  # with respect to the tensor the method reads: the distribution's own logits, or probs (ref.WRT)
        for k in ref.CONTINUOUS:
            (g,) = torch.autograd.grad(got[k], getattr(dist, ref.WRT[k]), ref.upstream(got[k].shape, dtype),
                                       retain_graph=True)
            rec["g_" + k] = g
            dev["g_" + k] = ref.units(g, gw["g_" + k], eps)
    return rec, dev


def relaxed():
    gen = torch.Generator().manual_seed(0x5EED0D15)
    cases, dropped, worst = [], [], {}
    for family in ("gumbel", "bernoulli"):
        for si, (sample, lead, V, from_probs) in enumerate(SHAPES):
            logits = 2 * torch.randn(lead + (V,), generator=gen, dtype=torch.float32)
            if from_probs:  # (Gumbel: not normalised, the constructor's job)
                param32 = 1.7 * logits.softmax(-1) if family == "gumbel" else logits.sigmoid()
            else:
                param32 = logits
            shape = sample + lead + (V,)
            u32, v32 = draw(gen, shape), draw(gen, shape)
            recs = {}
            for dt in DTYPES:
                recs[dt] = run_case(family, getattr(torch, dt), param32, from_probs, sample, u32, v32)
            same_b = torch.equal(recs["float32"][0]["b"].double(), recs["float64"][0]["b"].double())
            guard = False
            if family == "gumbel":
                for dt in DTYPES:
                    r = recs[dt][0]
                    eps = float(torch.finfo(r["u"].dtype).eps)
                    probs = ref.gumbel_probs(ref.f64(r["param"]), from_probs)
                    guard = guard or bool(ref.gumbel_guard(probs, *ref.f64(r["b"], r["v"]), eps).any())
                    zk = (r["zcond"] * r["b"]).sum(-1, keepdim=True)
                    guard = guard or bool(((r["zcond"] >= zk - eps) & (r["b"] == 0)).any())
            if guard or not same_b:
                dropped.append([family, si, "guard" if guard else "b differs"])
                continue
            for dt in DTYPES:
                rec, dev = recs[dt]
                k = len(cases)
                cases.append(dict(family=family, dtype=dt, sample=list(sample), lead=list(lead), V=V,
                                  probs=from_probs, shape_index=si))
                for name, t in rec.items():
                    if dt == "float64" and name in ("param", "u", "v"):
                        continue  # (the float32 twin's, case k - 1, widened)
                    put("case_{}_{}".format(k, name), t.to(torch.uint8) if name == "b" else t)
                for name, d in dev.items():
                    key = "tol_{}_{}_{}".format(family, name, dt)
                    worst[key] = max(worst.get(key, 0.0), d)
    put("cases", json.dumps(cases))
    put("dropped", json.dumps(dropped))
    put("n_shapes", 2 * len(SHAPES))
    for key, d in sorted(worst.items()):
        put(key, max(4.0, 4.0 * d))
        print("{:44s} reference {:8.2f} units -> tolerance {:8.2f}".format(key, d, max(4.0, 4.0 * d)))
    print("cases kept:", len(cases), "dropped:", dropped)


def extras():
    gen = torch.Generator().manual_seed(0xE87A)
    for dt in DTYPES:
        dtype = getattr(torch, dt)
        # threshold: ties (the lowest index), -0 against +0, a NaN (the maximum), all -inf
        z = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0], [-0.0, 0.0, -1.0, -2.0, 0.0], [0.0, -0.0, -1.0, -2.0, -0.0],
                          [5.0, float("nan"), 7.0, 1.0, 2.0], [float("-inf")] * 5, [2.0, 2.0, 2.0, 2.0, 2.0]], dtype=dtype)
        wide = torch.zeros(3, 70, dtype=dtype)
        wide[0, 69] = wide[0, 3] = 1.5
        wide[1, 66] = float("nan")
        wide[2, 64] = 1e-30
        dist = RD.GumbelOneHotCategorical(logits=torch.zeros(5, dtype=dtype), validate_args=False)
        put("threshold_{}_z".format(dt), z)
        put("threshold_{}_b".format(dt), dist.threshold(z))
        put("threshold_{}_wide_z".format(dt), wide)
        put("threshold_{}_wide_b".format(dt), RD.GumbelOneHotCategorical(
            logits=torch.zeros(70, dtype=dtype), validate_args=False).threshold(wide))
        zb = torch.tensor([0.0, -0.0, 1.0, -1.0, float("nan"), 1e-40], dtype=dtype)
        put("threshold_{}_bern_z".format(dt), zb)
        put("threshold_{}_bern_b".format(dt), RD.LogisticBernoulli(
            logits=torch.zeros(6, dtype=dtype), validate_args=False).threshold(zb))
        # clog_prob with a b that is not the threshold of zcond: -inf on those rows / elements only
        for family in ("gumbel", "bernoulli"):
            logits32 = 2 * torch.randn((2, 5), generator=gen, dtype=torch.float32)
            u32, v32 = draw(gen, (3, 2, 5)), draw(gen, (3, 2, 5))
            rec, _ = run_case(family, dtype, logits32, False, (3,), u32, v32, grads=False)
            b = rec["b"].clone()
            if family == "gumbel":
                b[1, 0] = b[1, 0].roll(1)
                b[2, 1] = 0.0  # (not one-hot at all)
            else:
                b[1, 0] = 1 - b[1, 0]
            dist = CLASSES[family](logits=rec["param"].detach(), validate_args=False)
            pre = "mismatch_{}_{}_".format(family, dt)
            put(pre + "param", rec["param"])
            put(pre + "zcond", rec["zcond"])
            put(pre + "b", b)
            put(pre + "clog_prob", dist.clog_prob(rec["zcond"], b))
        # the min guard on purpose: off the hot index a probability near 1 with v = 1 adds less than half an ulp to
        # -log v_k, so the free value is z_k itself; in row 1 |z_k| >= 2, where float32 rounds z_k - eps to z_k
        logits32 = torch.tensor([[10.0, -1.0, 0.0, 0.0], [0.2, 0.1, 12.0, 0.0]])
        b = torch.tensor([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]], dtype=dtype)
        v = torch.tensor([[1.0, 1e-3, 0.5, 0.3], [0.7, 0.6, 1.0, 1e-4]], dtype=dtype)
        dist = RD.GumbelOneHotCategorical(logits=logits32.to(dtype))
        with Noise(v):
            zcond = dist.csample(b)
        zk = (zcond * b).sum(-1, keepdim=True)
        assert bool(((zcond >= zk - float(torch.finfo(dtype).eps)) & (b == 0)).any())
        pre = "guard_{}_".format(dt)
        put(pre + "param", logits32.to(dtype))
        put(pre + "b", b)
        put(pre + "v", v)
        put(pre + "zcond", zcond)
        # the CPU stream: no substitution, a seed alone
        for family in ("gumbel", "bernoulli"):
            logits = (2 * torch.randn((2, 5), generator=gen, dtype=torch.float32)).to(dtype)
            dist = CLASSES[family](logits=logits)
            torch.manual_seed(1234)
            z = dist.rsample([3])
            b = dist.threshold(z)
            zcond = dist.csample(b)
            pre = "seed_{}_{}_".format(family, dt)
            put(pre + "param", logits)
            put(pre + "z", z)
            put(pre + "zcond", zcond)
    # statistics and expand
    logits = 2 * torch.randn((2, 5), generator=gen, dtype=torch.float32)
    for family in ("gumbel", "bernoulli"):
        dist = CLASSES[family](logits=logits)
        pre = "stats_{}_".format(family)
        put(pre + "param", logits)
        for name in ("mean", "stddev", "variance"):
            put(pre + name, getattr(dist, name))
        put(pre + "entropy", dist.entropy())
        put(pre + "probs", dist.probs)
        put(pre + "logits", dist.logits)
        e = dist.expand([3, 2] if family == "gumbel" else [3, 2, 5])
        put(pre + "expand_batch", np.array(e.batch_shape))
        put(pre + "expand_logits", e.logits)
    # control variates
    z = torch.randn((3, 2, 5), generator=gen)
    for name in ("LogisticBernoulliRebarControlVariate", "GumbelOneHotCategoricalRebarControlVariate"):
        cv = getattr(RM, name)(lambda x: (x * x).sum(-1), 0.3, 1.5)
        put("cv_{}_z".format(name), z)
        put("cv_{}_out".format(name), cv(z))
        put("cv_{}_log_temp".format(name), cv.log_temp)
        put("cv_{}_repr".format(name), cv.extra_repr())


def sequences():
    rng = np.random.default_rng(0x5E0)
    # (a trigram table of more than 255 nodes: the reference's builder fails on uint8 trie offsets under NumPy 2)
    V, sos, eos, T, N = 6, 6, 1, 3, 3
    toks = list(range(V)) + [sos]
    dicts = [{k: (float(rng.normal() - 2.0), float(rng.normal() * 0.3)) for k in toks},
             {(a, c): (float(rng.normal() - 1.0), float(rng.normal() * 0.3)) for a in toks for c in range(V)},
             {(a, c, e): float(rng.normal() - 1.0) for a in toks for c in range(V) for e in range(V) if rng.random() < 0.9}]
    put("seq_cfg", np.array([V, sos, N, eos, T]))
    for n, dd in enumerate(dicts):
        put("seq_keys{}".format(n), np.array([[k] if n == 0 else list(k) for k in dd], dtype=np.int64).reshape(len(dd), n + 1))
        put("seq_vals{}".format(n), np.array([[x] if n == N - 1 else list(x) for x in dd.values()], dtype=np.float64))
    for tag, e in (("eos", eos), ("noeos", None)):
        lm = RM.LookupLanguageModel(V, sos, [d.copy() for d in dicts])
        walk = RM.RandomWalk(lm, e)
        flat = RD.SequentialLanguageModelDistribution(walk, max_iters=T)
        batched = RD.SequentialLanguageModelDistribution(walk, 3, max_iters=T)
        value = torch.from_numpy(rng.integers(0, V, (5, T)))
        value_b = torch.from_numpy(rng.integers(0, V, (2, 3, T)))
        if e is not None:
            value[0, 0] = value[1, 1] = value_b[0, 1, 1] = value_b[1, 2, 0] = e
        put("seq_{}_value".format(tag), value)
        put("seq_{}_log_prob".format(tag), flat.log_prob(value))
        put("seq_{}_value_b".format(tag), value_b)
        put("seq_{}_log_prob_b".format(tag), batched.log_prob(value_b))
        put("seq_{}_support".format(tag), flat.enumerate_support())
        put("seq_{}_support_b".format(tag), batched.enumerate_support())
        put("seq_{}_support_b_shape".format(tag), np.array(batched.enumerate_support(False).shape))


def srswor():
    total, given = torch.tensor([5, 4, 6, 1]), torch.tensor([2, 4, 0, 1])
    dist = RD.SimpleRandomSamplingWithoutReplacement(given, total, 7)
    put("srswor_total", total)
    put("srswor_given", given)
    value = dist.sample([2])
    put("srswor_value", value)
    put("srswor_log_prob", dist.log_prob(value))
    for name in ("mean", "variance", "log_partition"):
        put("srswor_" + name, getattr(dist, name))
    put("srswor_support_check", dist.support.check(torch.stack([value[0], value[0].flip(-1)])))
    uni = RD.SimpleRandomSamplingWithoutReplacement(torch.tensor([2, 2]), 5, 6)
    put("srswor_uniform_support", uni.enumerate_support())
    put("srswor_uniform_support_shape", np.array(uni.enumerate_support(False).shape))
    put("srswor_uniform_log_prob", uni.log_prob(uni.enumerate_support()))
    put("srswor_has_enumerate", np.array([dist.has_enumerate_support, uni.has_enumerate_support]))


def errors():
    t = torch.tensor
    G, L = RD.GumbelOneHotCategorical, RD.LogisticBernoulli
    lm = RM.LookupLanguageModel(4, 0)
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
        "cv_temp_zero": lambda: RM.LogisticBernoulliRebarControlVariate(f, 0.0),
        "cv_temp_str": lambda: RM.GumbelOneHotCategoricalRebarControlVariate(f, "a"),
        "cv_eta_str": lambda: RM.GumbelOneHotCategoricalRebarControlVariate(f, 0.1, "a"),
        "constraint_neither": lambda: RD.TokenSequenceConstraint(4),
        "constraint_vocab_zero": lambda: RD.TokenSequenceConstraint(0, 1),
        "constraint_max_iters_negative": lambda: RD.TokenSequenceConstraint(4, None, -1),
        "seq_no_eos_no_max_iters": lambda: RD.SequentialLanguageModelDistribution(RM.RandomWalk(lm)),
        "seq_batch_size_zero": lambda: RD.SequentialLanguageModelDistribution(RM.RandomWalk(lm, 1), 0),
        "seq_cache_samples_int": lambda: RD.SequentialLanguageModelDistribution(RM.RandomWalk(lm, 1), cache_samples=1),
        "seq_initial_state": lambda: RD.SequentialLanguageModelDistribution(
            RM.RandomWalk(lm, 1), initial_state={"a": 1}, validate_args=True),
        "seq_enumerate_without_max_iters": lambda: RD.SequentialLanguageModelDistribution(
            RM.RandomWalk(lm, 1)).enumerate_support(),
        "srswor_given_exceeds": lambda: RD.SimpleRandomSamplingWithoutReplacement(t([3]), t([2]), validate_args=True),
        "srswor_out_size_small": lambda: RD.SimpleRandomSamplingWithoutReplacement(t([1]), t([4]), 3, validate_args=True),
        "srswor_negative": lambda: RD.SimpleRandomSamplingWithoutReplacement(t([-1]), t([4]), validate_args=True),
        "srswor_enumerate_mixed": lambda: RD.SimpleRandomSamplingWithoutReplacement(t([1, 2]), t([4, 4])).enumerate_support(),
        "cardinality_negative": lambda: RD.BinaryCardinalityConstraint(t([-1]), 3),
        "cardinality_tmax_zero": lambda: RD.BinaryCardinalityConstraint(t([1]), 0),
    }
    names = {}
    for key, fn in cases.items():
        try:
            fn()
            names[key] = "none"
        except Exception as e:  # noqa: BLE001
            names[key] = type(e).__name__
    put("errors", json.dumps(names))
    print("errors:", names)


def params(fn):
    fn = getattr(fn, "fget", fn)
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name,
             repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def public(cls):
    """name -> kind and parameters of what the class itself (or a reference base below torch's) defines"""
    names = {}
    for B in cls.__mro__:
        if B.__module__.startswith("torch.") or B is object:
            continue
        for name, member in vars(B).items():
            if name.startswith("_") and name not in ("__init__", "_validate_thresholded_sample"):
                continue
            if name in names:
                continue
            if isinstance(member, (classmethod, staticmethod)):
                continue
            if isinstance(member, property) or type(member).__name__ in ("lazy_property", "_DependentProperty"):
                names[name] = ["property"]
            elif inspect.isfunction(member):
                names[name] = ["method", params(member)]
    return names


def signatures():
    sig = {"distributions_all": sorted(RD.__all__), "modules_all": sorted(RM.__all__), "classes": {}}
    for name in RD.__all__:
        sig["classes"][name] = public(getattr(RD, name))
    for name in ("LogisticBernoulliRebarControlVariate", "GumbelOneHotCategoricalRebarControlVariate"):
        sig["classes"][name] = public(getattr(RM, name))
    with open(os.path.join(HERE, "distributions_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


torch.manual_seed(0)
relaxed()
extras()
sequences()
srswor()
errors()
signatures()
path = os.path.join(HERE, "distributions.npz")
np.savez_compressed(path, **out)
print("wrote distributions.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")
