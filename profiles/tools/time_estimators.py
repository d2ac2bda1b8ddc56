#!/usr/bin/env python
"""Time every estimator's call plus backward on the device against the same estimator reducing with its torch
body (``_estimators.mc_reduce_torch`` / ``imh_chain_torch``, the reference's formula as torch ops, called directly
on the same tensors), at M in {16, 1024} samples and B in {8, 4096} batch elements, float32.

Device events around ``--iters`` calls after a warm-up (1000 by default: windows of a quarter of a second and
more), the two contestants alternated over ``--rounds`` rounds; one JSON line: median microseconds per call and
the smallest and largest round of each contestant.  The torch body is put in place of the fused reduction here,
in this tool; the package has no switch for it.

    python profiles/tools/time_estimators.py [--out profiles/estimators_times.json]

Launch counts come from a run of their own under the kernel tracer.  ``--trace`` makes no measurement: per shape,
estimator and contestant it runs one call (after a warm-up call) between two launches of a marker kernel
(``return_columns_kernel``, which no estimator uses) and writes the order of those calls; ``--count DIR`` reads
the tracer's ``*kernel_trace.csv`` under DIR and counts the dispatches between each pair of markers.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/tools/time_estimators.py --trace --plan DIR/plan.json
    python profiles/tools/time_estimators.py --count DIR --plan DIR/plan.json [--out profiles/estimators_launches.json]
"""
import argparse
import contextlib
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

from pydrobert_amd import _estimators as X  # noqa: E402
from pydrobert_amd import distributions as D  # noqa: E402
from pydrobert_amd import modules as Mods  # noqa: E402


def _body_reduce(kind, is_log, f, a=None, cz=None, c=None, lp=None, lq=None, mode=X.W_LOGM):
    return X.mc_reduce_torch(kind, is_log, mode, f, a, cz, c, lp, lq)


def _body_chain(ratio, ratio0, log_u):
    return X.imh_chain_torch(ratio, ratio0.to(ratio.dtype), log_u.to(ratio.dtype))


@contextlib.contextmanager
def torch_bodies():
    saved = X.mc_reduce, X.imh_chain
    X.mc_reduce, X.imh_chain = _body_reduce, _body_chain
    try:
        yield
    finally:
        X.mc_reduce, X.imh_chain = saved


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def contest(fns, iters, rounds):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    return ({k: round(statistics.median(v), 2) for k, v in times.items()},
            {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()})


MARKER = "return_columns_kernel"


def trace(plan_path):
    """One call of every estimator and contestant between two marker launches, for the kernel tracer."""
    from pydrobert_amd import functional as F

    dev = torch.device("cuda:0")
    marker_input = torch.zeros((4, 3), device=dev)

    def marker():
        torch.cuda.synchronize()
        F.time_distributed_return(marker_input, 0.5)
        torch.cuda.synchronize()

    plan = []
    for M, B in ((16, 8), (1024, 4096)):
        for name, run in estimators(M, B, dev).items():
            def body():
                with torch_bodies():
                    return run()

            for contestant, fn in (("fused", run), ("torch_body", body)):
                fn()
                marker()
                fn()
                marker()
                plan.append(["M{}_B{}".format(M, B), name, contestant])
    with open(plan_path, "w") as f:
        json.dump(plan, f)


def count(directory, plan_path):
    """{shape: {estimator: {contestant: dispatches of one call}}} from the tracer's CSV and the plan of trace()."""
    (path,) = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    segments, current = [], None
    for r in rows:
        if MARKER in r["Kernel_Name"]:
            if current is None:
                current = []
            else:
                segments.append(len(current))
                current = None
        elif current is not None:
            current.append(r["Kernel_Name"])
    with open(plan_path) as f:
        plan = json.load(f)
    assert len(segments) == len(plan), (len(segments), len(plan))
    result = {}
    for (shape, name, contestant), n in zip(plan, segments):
        result.setdefault(shape, {}).setdefault(name, {})[contestant] = n
    return result


def estimators(M, B, dev):
    """name -> (a function that runs the estimator once and backpropagates, calls per timing window scale)."""
    gen = torch.Generator(dev).manual_seed(0)
    logits = torch.randn(B, device=dev, generator=gen).requires_grad_(True)
    qlogits = torch.randn(B, device=dev, generator=gen)
    theta = torch.tensor([1.3], device=dev, requires_grad=True)
    t = torch.randn(B, device=dev, generator=gen)
    func = lambda b: theta * (b - t) ** 2 + 0.5  # noqa: E731
    lfunc = lambda b: (theta * (b - t) ** 2 + 0.5).log()  # noqa: E731
    E = sys.modules["pydrobert_amd.estimators"]
    cat = torch.randn((B, min(M, 64)), device=dev, generator=gen).requires_grad_(True)
    w = torch.randn(min(M, 64), device=dev, generator=gen)

    def grad(v, *wrt):
        return torch.autograd.grad(v.sum(), wrt, allow_unused=True)

    def bern():
        return torch.distributions.Bernoulli(logits=logits)

    def relaxed():
        return D.LogisticBernoulli(logits=logits)

    cv = Mods.LogisticBernoulliRebarControlVariate(func, 0.5, 0.8).to(dev)
    runs = {
        "direct": lambda: grad(E.DirectEstimator(bern(), func, M)(), logits, theta),
        "direct_log_cv": lambda: grad(E.DirectEstimator(
            bern(), lfunc, M, cv=lambda b: 0.5 * lfunc(b), cv_mean=(0.5 * logits).detach(), is_log=True)(), logits, theta),
        "reparam_log": lambda: grad(E.ReparameterizationEstimator(
            torch.distributions.Normal(logits, 1.0), lambda z: theta * torch.sin(z), M, True)(), logits, theta),
        "straight_through": lambda: grad(E.StraightThroughEstimator(relaxed(), func, M)(), logits, theta),
        "importance_self_norm_log": lambda: grad(E.ImportanceSamplingEstimator(
            torch.distributions.Bernoulli(logits=qlogits), lfunc, M, bern(), True, True)(), logits, theta),
        "relax": lambda: grad(E.RelaxEstimator(relaxed(), func, M, cv)(), logits, theta, cv.log_temp, cv.eta),
        "enumerate": lambda: grad(E.EnumerateEstimator(
            torch.distributions.Categorical(logits=cat), lambda b: theta * w[b])(), cat, theta),
        "imh": lambda: E.IndependentMetropolisHastingsEstimator(
            torch.distributions.Bernoulli(logits=qlogits), func, M, bern(), burn_in=M // 4)(),
    }
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--count", default=None)
    ap.add_argument("--plan", default="estimators_trace_plan.json")
    args = ap.parse_args()
    import pydrobert_amd.estimators  # noqa: F401

    if args.count:
        line = json.dumps(count(args.count, args.plan), sort_keys=True)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    assert torch.cuda.is_available(), "needs a ROCm device"
    if args.trace:
        return trace(args.plan)
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "unit": "us per call plus backward (median of rounds)",
              "dtype": "float32", "iters": args.iters, "rounds": args.rounds}
    for M in (16, 1024):
        for B in (8, 4096):
            shape = {}
            for name, run in estimators(M, B, dev).items():
                def body():
                    with torch_bodies():
                        return run()

                iters = max(5, args.iters // 20) if name == "imh" and M > 16 else args.iters  # (25 ms a call there)
                res, spread = contest({"fused": run, "torch_body": body}, iters, args.rounds)
                res["min_max_over_rounds"] = spread
                res["fused_over_torch_body"] = round(res["fused"] / res["torch_body"], 3)
                shape[name] = res
                print(M, B, name, res, file=sys.stderr, flush=True)
            result["M{}_B{}".format(M, B)] = shape
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
