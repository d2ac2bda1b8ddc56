#!/usr/bin/env python
"""Generate tests/golden/estimators.npz and estimators_signatures.json from the LIVE reference's estimators.

Run where the reference is checked out (it never travels to the GPU box), PDT_REFERENCE naming its root:

    python tests/golden/make_estimators_golden.py

Every array is DATA: inputs this script draws and what the reference returned for them.  Every case is
deterministic (tests/_estimators_ref.py): a replay proposal hands out the recorded rows in order, and while the
reference runs ``torch.rand`` / ``torch.rand_like`` return the recorded uniforms (the IMH draws, and u and v of
the relaxed proposals).  Inputs are drawn in float32 and widened for the float64 twin of a case, which follows it
and does not store them again.

Ties.  In log space the SCORE reduction's gradient follows ``max``'s choice among equal maxima, so those cases get
samples that are distinct per column by construction: the replay rows are a permutation of the classes, and the
Gumbel noise of the log-space Relax case puts each sample's arg-max on its own class.  A case whose column maximum
is still attained twice, or whose float32 and float64 runs threshold to different ``b``, is dropped and listed.

Tolerances.  For the value and every gradient the largest deviation of the reference from the float64 yardstick
on the same inputs is measured in units of eps (1 + |value|), and 4x that, 4 units at least, is stored as
``tol_<estimator>_<output>_<dtype>``; ``tol_op_<operation>_<v|g>_<dtype>`` is the largest of the estimators that
reduce with that operation, IMH left out (the kernels' parity tests use it).  The margin is for the device's exp and log being
good to 1-2 ulp where the CPU's are within 1, and for the order of summation.
"""
import inspect
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = os.environ.get("PDT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pydrobert.torch.distributions as RD  # noqa: E402
import pydrobert.torch.estimators as RE  # noqa: E402
import pydrobert.torch.modules as RM  # noqa: E402

import _estimators_ref as ref  # noqa: E402

warnings.simplefilter("ignore")
NS = types.SimpleNamespace(E=RE, D=RD, M=RM)
DTYPES = ("float32", "float64")
# (IMH reduces with MEAN too, but its reference adds one sample at a time over the chain: a deviation that is not
# the reduction formula's, and stays out of the operator's tolerance)
OPS = {"direct": "SCORE", "relax": "SCORE", "reparam": "MEAN", "st": "MEAN", "is": "WEIGHTED", "enumerate": "WEIGHTED"}
out = {}


def put(key, v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    out[key] = np.asarray(v)


def case(est, M, batch, is_log, **kw):
    d = dict(est=est, M=M, batch=list(batch), is_log=is_log, cv=False, self_normalize=False, burn_in=0,
             family=None, varmin=False, V=0)
    d.update(kw)
    return d


CASES = []
for is_log in (False, True):
    for cv in (False, True):
        CASES.append(case("direct", 65, (12,), is_log, cv=cv, V=80))
    CASES.append(case("direct", 7, (2, 3), is_log, cv=True, V=9))
    CASES.append(case("reparam", 65, (12,), is_log))
    CASES.append(case("reparam", 1, (2, 3), is_log))
    CASES.append(case("st", 65, (12,), is_log))
    for sn in (False, True):
        CASES.append(case("is", 65, (12,), is_log, self_normalize=sn, V=80))
        CASES.append(case("is", 2, (2, 3), is_log, self_normalize=sn, V=5))
    CASES.append(case("relax", 65 if not is_log else 12, (12,) if not is_log else (3,), is_log,
                      family="bernoulli" if not is_log else "gumbel", V=0 if not is_log else 16))
    CASES.append(case("relax", 12, (2, 3), is_log, family="gumbel", V=16))
    for burn_in in (0, 5):
        CASES.append(case("imh", 65, (12,), is_log, burn_in=burn_in, V=11))
    CASES.append(case("imh", 7, (2, 3), is_log, burn_in=6, V=4))
    CASES.append(case("enumerate", 9, (12,), is_log, V=9))
CASES.append(case("relax", 7, (12,), False, family="bernoulli", varmin=True))
CASES.append(case("relax", 7, (3,), False, family="gumbel", varmin=True, V=16))


def draw(gen, shape, lo=0.02, hi=0.98):
    return torch.rand(shape, generator=gen, dtype=torch.float32) * (hi - lo) + lo


def permuted_rows(gen, n, batch, V):
    """(n,) + batch class indices, distinct down every column while n <= V."""
    cols = int(torch.Size(batch).numel())
    rows = torch.stack([torch.cat([torch.randperm(V, generator=gen) for _ in range(-(-n // V))])[:n] for _ in range(cols)], 1)
    return rows.reshape((n,) + tuple(batch))


def inputs(c, gen):
    """The float32 inputs of a case."""
    est, M, batch, V = c["est"], c["M"], tuple(c["batch"]), c["V"]
    T = {"theta": torch.tensor([1.3])}
    if est in ("direct", "is", "imh", "enumerate"):
        T["logits"] = torch.randn(batch + (V,), generator=gen)
        T["w"] = torch.randn((V,), generator=gen)
        T["w2"] = torch.randn((V,), generator=gen)
        T["qlogits"] = 0.5 * torch.randn(batch + (V,), generator=gen)
        n = M + 1 if est == "imh" else M
        if est == "imh":  # (a chain revisits classes: plain draws from the proposal)
            T["rows"] = torch.distributions.Categorical(logits=T["qlogits"]).sample([n])
            T["u"] = draw(gen, (M,) + batch, 1e-3, 1.0)
        elif est != "enumerate":
            T["rows"] = permuted_rows(gen, n, batch, V)
    elif est == "reparam":
        T["logits"] = torch.randn(batch, generator=gen)
        T["rows"] = torch.randn((M,) + batch, generator=gen)
    elif c["family"] == "gumbel":
        T["logits"] = 0.3 * torch.randn(batch + (V,), generator=gen)
        T["w"] = torch.randn((V,), generator=gen)
        shape = (M,) + batch + (V,)
        T["u"], T["nv"] = draw(gen, shape, 0.02, 0.6), draw(gen, shape)
        hot = torch.nn.functional.one_hot(permuted_rows(gen, M, batch, V), V).bool()
        T["u"] = torch.where(hot, torch.full_like(T["u"], 0.97), T["u"])
    else:  # logistic / Bernoulli: st and relax
        T["logits"] = torch.randn(batch, generator=gen)
        T["w"] = 0.5 * torch.randn(batch, generator=gen)
        T["u"], T["nv"] = draw(gen, (M,) + batch), draw(gen, (M,) + batch)
    return T


def discrete(c, T):
    """The ``b`` the reference's distribution thresholds the case's noise to (a constant of the case)."""
    if c["est"] not in ("st", "relax"):
        return None
    cls = RD.GumbelOneHotCategorical if c["family"] == "gumbel" else RD.LogisticBernoulli
    dist = cls(logits=T["logits"])
    with ref.noise(T["u"]):
        return dist.threshold(dist.rsample([c["M"]]))


def main():
    gen = torch.Generator().manual_seed(0xE571)
    kept, dropped, worst = [], [], {}
    for ci, c in enumerate(CASES):
        T32 = inputs(c, gen)
        runs, ok = {}, True
        for dt in DTYPES:
            dtype = getattr(torch, dt)
            T = {k: (t if t.dtype == torch.int64 else t.to(dtype)) for k, t in T32.items()}
            if "u" in T and c["est"] == "imh":
                T["u"] = T32["u"]  # (the reference draws the chain's uniforms in the default dtype)
            b = discrete(c, T)
            if b is not None:
                T["b"] = b
            cd = dict(c, dtype=dt)
            v, grads = ref.drive(NS, cd, T)
            want, want_g = ref.yardstick(cd, T)
            runs[dt] = (cd, T, v, grads, want, want_g)
        if "b" in runs["float32"][1] and not torch.equal(runs["float32"][1]["b"].double(), runs["float64"][1]["b"].double()):
            ok, why = False, "b differs"
        if ok and c["is_log"] and c["est"] in ("direct", "relax"):
            cd, T, *_ = runs["float64"]
            f = T["w"][T["rows"]] if c["est"] == "direct" else (T["b"] * T["w"]).sum(-1)
            if bool(((f == f.max(0, keepdim=True)[0]).sum(0) > 1).any()):
                ok, why = False, "tie at the column maximum"
        if not ok:
            dropped.append([ci, c["est"], why])
            continue
        for dt in DTYPES:
            cd, T, v, grads, want, want_g = runs[dt]
            eps = float(torch.finfo(getattr(torch, dt)).eps)
            k = len(kept)
            kept.append(cd)
            for name, t in T.items():
                if dt == "float64" and name != "b":
                    continue  # (the float32 twin's, case k - 1, widened)
                put("case_{}_{}".format(k, name), t.to(torch.uint8) if name == "b" else t)
            put("case_{}_v".format(k), v)
            devs = {"v": ref.units(v, want, eps)}
            for name, g in grads.items():
                put("case_{}_g_{}".format(k, name), g)
                devs["g_" + name] = ref.units(g, want_g[name], eps)
            for name, d in devs.items():
                key = "tol_{}_{}_{}".format(c["est"], name, dt)
                worst[key] = max(worst.get(key, 0.0), d)
                if c["est"] in OPS:
                    key = "tol_op_{}_{}_{}".format(OPS[c["est"]], "v" if name == "v" else "g", dt)
                    worst[key] = max(worst.get(key, 0.0), d)
    assert 20 * len(dropped) <= len(CASES), dropped
    put("cases", json.dumps(kept))
    put("dropped", json.dumps(dropped))
    for key, d in sorted(worst.items()):
        assert np.isfinite(d), key
        put(key, max(4.0, 4.0 * d))
        print("{:40s} reference {:8.2f} units -> tolerance {:8.2f}".format(key, d, max(4.0, 4.0 * d)))
    print("cases kept:", len(kept), "dropped:", dropped)


def params(fn):
    return [[p.name, p.default is not inspect.Parameter.empty, p.kind.name,
             repr(p.default) if p.default is not inspect.Parameter.empty else None]
            for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def signatures():
    sig = {"estimators_all": sorted(RE.__all__), "classes": {}}
    for name in RE.__all__:
        cls = getattr(RE, name)
        if not inspect.isclass(cls):
            continue
        names = {}
        for B in cls.__mro__:
            if B is object or B.__module__.startswith(("torch.", "abc")):
                continue
            for attr, member in vars(B).items():
                if attr.startswith("_") and attr not in ("__init__", "__call__"):
                    continue
                if inspect.isfunction(member) and attr not in names:
                    names[attr] = params(member)
        sig["classes"][name] = names
    with open(os.path.join(HERE, "estimators_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)


torch.manual_seed(0)
main()
signatures()
path = os.path.join(HERE, "estimators.npz")
np.savez_compressed(path, **out)
print("wrote estimators.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")
