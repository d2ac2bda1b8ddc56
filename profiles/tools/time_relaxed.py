#!/usr/bin/env python
"""Time every method of GumbelOneHotCategorical and LogisticBernoulli, and its backward, on the device against the
reference's formula run as torch ops on the same tensors (what a caller ran before csrc/relaxed.hip).  Device
events around ``--iters`` calls after a warm-up (2000 by default: windows of 20 ms and more), the contestants
alternated over ``--rounds`` rounds; one JSON line (median microseconds per call and the smallest and largest round
of each contestant), with each kernel's traffic bound beside it: bytes read and written over the HBM rate.

``backward_alone`` is the backward of the kernel route on its own, called as autograd calls it: the operator
``pydrobert_amd::relaxed_backward`` where the package has it, the torch-composed backward and its ``sum_to_size``
where it does not (``--package-root`` points at the package of another commit, to time both in one visit).

    python profiles/tools/time_relaxed.py [--out profiles/relaxed_times.json] [--package-root DIR] [--families gumbel]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_US = 8.0e6  # MI355X: 8 TB/s peak


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--package-root", default=os.path.join(ROOT, "pydrobert-pytorch_amd"))
    ap.add_argument("--families", default="gumbel,logistic")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    from pydrobert_amd import _relaxed as X

    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    has_op = hasattr(X, "_relaxed_backward_op")
    result = {"device": torch.cuda.get_device_name(0), "unit": "us per call (median of rounds)", "dtype": "float32",
              "backward": "pydrobert_amd::relaxed_backward" if has_op else "torch-composed"}
    for family in args.families.split(","):
        fam = X.GUMBEL if family == "gumbel" else X.BERNOULLI
        chain_of, body_of = X._TORCH[fam], (X._gumbel_backward if family == "gumbel" else X._bernoulli_backward)
        for M, N, V in ((64, 32, 512), (64, 32, 32)):
            gen = torch.Generator(dev).manual_seed(0)
            raw = 2 * torch.randn((N, V), device=dev, generator=gen)
            logits = (raw.log_softmax(-1) if family == "gumbel" else raw).detach().requires_grad_(True)
            probs = (logits.detach().exp() if family == "gumbel" else raw.sigmoid()).requires_grad_(True)
            u = torch.rand((M, N, V), device=dev, generator=gen) * 0.96 + 0.02
            v = torch.rand((M, N, V), device=dev, generator=gen) * 0.96 + 0.02
            z = X._relaxed(fam, X.RSAMPLE, logits.detach(), u)
            b = X._relaxed(fam, X.THRESHOLD, None, z)
            zcond = X._relaxed(fam, X.CSAMPLE, probs.detach(), b, v)
            full, par = M * N * V * 4, N * V * 4
            rows = M * N * 4 if family == "gumbel" else full  # (the logistic methods do not reduce)
            # method: (op, parameter, data arguments, bytes the kernel reads and writes)
            methods = {
                "rsample": (X.RSAMPLE, logits, (u,), par + 2 * full),
                "threshold": (X.THRESHOLD, None, (z,), 2 * full),
                "tlog_prob": (X.TLOG_PROB, logits, (b,), par + full + rows),
                "csample": (X.CSAMPLE, probs, (b, v), par + 3 * full),
                "log_prob": (X.LOG_PROB, logits, (z,), par + full + rows),
                "clog_prob": (X.CLOG_PROB, logits, (zcond, b), par + 2 * full + rows),
            }
            shape = {}
            for name, (op, param, data, nbytes) in methods.items():
                x2 = data[1] if len(data) > 1 else None
                detached = None if param is None else param.detach()
                kernel = lambda: X._relaxed(fam, op, detached, data[0], x2)  # noqa: E731
                chain = lambda: chain_of(op, detached, data[0], x2)  # noqa: E731
                got, want = kernel(), chain()
                fin = torch.isfinite(want)
                assert torch.equal(torch.isfinite(got), fin)
                err = float(((got[fin] - want[fin]).abs() / (1 + want[fin].abs())).max())
                fns = {"kernel": kernel, "torch_chain": chain}
                if param is not None and name != "threshold":
                    up = torch.randn_like(got)

                    def kernel_fb():
                        out = torch.ops.pydrobert_amd.relaxed(fam, op, param, data[0], x2)
                        return torch.autograd.grad(out, param, up)

                    def chain_fb():
                        return torch.autograd.grad(chain_of(op, param, data[0], x2), param, up)

                    if has_op and name == "rsample":  # (the identity: the host reduces the gradient itself)
                        def backward_alone():
                            return (up.sum_to_size(detached.shape),)
                    elif has_op:  # (the plain call that an ordinary backward makes)
                        def backward_alone():
                            return X._backward_body(fam, op, 1, up, detached, data[0], x2)
                    else:
                        def backward_alone():
                            return body_of(op, up, detached, data[0], x2)[0].sum_to_size(detached.shape)

                    with torch.no_grad():  # (against the float64 sum of the body's terms, on their magnitude)
                        terms = body_of(op, up, detached, data[0], x2)[0].double().expand(data[0].shape)
                        diff = (backward_alone()[0] if has_op else backward_alone()) - terms.sum_to_size(detached.shape)
                    assert float((diff.abs() / (1 + terms.abs().sum_to_size(detached.shape))).max()) < 1e-5
                    fns.update(kernel_forward_backward=kernel_fb, torch_chain_forward_backward=chain_fb,
                               backward_alone=backward_alone)
                res, spread = contest(fns, args.iters, args.rounds)
                res["min_max_over_rounds"] = spread
                res["kernel_bytes"] = nbytes
                res["traffic_bound_us"] = round(nbytes / HBM_BYTES_PER_US, 2)
                res["max_rel_diff_to_chain"] = err
                res["kernel_over_chain"] = round(res["kernel"] / res["torch_chain"], 3)
                if "kernel_forward_backward" in res:
                    res["backward_kernel_route"] = round(res["kernel_forward_backward"] - res["kernel"], 2)
                    res["backward_torch_chain"] = round(res["torch_chain_forward_backward"] - res["torch_chain"], 2)
                shape[name] = res
            key = "M{}_N{}_V{}".format(M, N, V)
            result[key if family == "gumbel" else "logistic_" + key] = shape
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
