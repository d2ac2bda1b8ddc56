#!/usr/bin/env python
"""Time the gradients of the image warps with respect to where they sample -- the HIP operators
(``dense_image_warp_flow_backward``, ``sparse_image_warp_points_backward``) against the torch bodies they
replaced, which the package keeps as private functions (``_img._dense_flow_grad_torch``,
``_img._sparse_points_grad_torch``: autograd through ``grid_sample``, the spline's query-sized sums as
elementwise float64 ops), called directly on the same tensors.  The package has no switch between them.

Shape: N x 1 x 1000 x 80 images (N = 2048 by default, the project's C4 shape), float32; the points' gradient
with 3 control points + 4 pinned corners, order 2, the no-flow form.  Device events around ``--iters`` calls
after a warm-up, the two contestants alternated over ``--rounds`` rounds; per contestant the median
milliseconds per call, the smallest and largest round, and the growth of allocated memory across one call
(peak minus what was allocated before it).  Where the torch body cannot allocate at N, that is recorded, both
contestants are timed at the largest N / 2^k at which it runs, and the HIP operator alone at N.

    python profiles/tools/time_warp_grads.py [--out profiles/warp_grad_times.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

from pydrobert_amd import _img  # noqa: E402

H, W, C = 1000, 80, 1
DENSE_CFG = ("hw", "bilinear", "border")
POINTS_CFG = ("hw", 2, 0.0, 1, "bilinear", "border", False)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def growth(fn):
    """Bytes by which allocated memory peaks above its level before one call."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return peak - before


def contest(fns, iters, rounds):
    """{name: {"ms": median, "min_max": [..], "growth_bytes": ..}}: warm-up, then alternating rounds."""
    result = {k: {"growth_bytes": growth(fn)} for k, fn in fns.items()}  # (the first call is the warm-up's first)
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    for k, v in times.items():
        result[k]["growth_bytes"] = growth(fns[k])  # (steady state: caches of constants are filled)
        result[k]["ms"] = round(statistics.median(v), 3)
        result[k]["min_max"] = [round(min(v), 3), round(max(v), 3)]
    return result


def verdict(res, new="hip", old="torch_body"):
    """The project's criterion: the other route's median exceeds the new one's by more than their combined
    spread (largest minus smallest round of each)."""
    spread = sum(res[k]["min_max"][1] - res[k]["min_max"][0] for k in (new, old))
    res["torch_over_hip"] = round(res[old]["ms"] / res[new]["ms"], 2)
    res["faster_beyond_spread"] = bool(res[old]["ms"] - res[new]["ms"] > spread)
    return res


def inputs(N, dev):
    gen = torch.Generator(dev).manual_seed(0)
    image = torch.randn((N, C, H, W), device=dev, generator=gen)
    g = torch.randn((N, C, H, W), device=dev, generator=gen)
    flow = torch.randn((N, H, W, 2), device=dev, generator=gen) * 3.0
    # three control points across the middle of the time axis ("hw": (h, w)), moved by a few frames
    dst = torch.tensor([[H * 0.25, W * 0.5], [H * 0.5, W * 0.3], [H * 0.75, W * 0.6]], device=dev).expand(N, 3, 2)
    dst = dst + torch.randn((N, 3, 2), device=dev, generator=gen) * 4.0
    src = dst + torch.randn((N, 3, 2), device=dev, generator=gen) * 5.0
    return image, g, flow, src.contiguous(), dst.contiguous()


def dense_fns(image, g, flow):
    return {
        "hip": lambda: torch.ops.pydrobert_amd.dense_image_warp_flow_backward(g, image, flow, *DENSE_CFG),
        "torch_body": lambda: _img._dense_flow_grad_torch(g, image, flow, *DENSE_CFG),
    }


def points_fns(image, g, src, dst):
    return {
        "hip": lambda: torch.ops.pydrobert_amd.sparse_image_warp_points_backward(g, None, image, src, dst, *POINTS_CFG),
        "torch_body": lambda: _img._sparse_points_grad_torch(g, None, image, src, dst, *POINTS_CFG),
    }


def runs(fn):
    """True when one call of ``fn`` finds its memory."""
    try:
        fn()
        torch.cuda.synchronize()
        return True
    except torch.cuda.OutOfMemoryError:
        return False
    finally:
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda:0")
    N = args.n
    result = {"device": torch.cuda.get_device_name(0), "unit": "ms per call (median of rounds)", "dtype": "float32",
              "shape": [N, C, H, W], "iters": args.iters, "rounds": args.rounds,
              "one_dxc_bytes": N * H * W * 7 * 2 * 8}  # fmt: skip
    image, g, flow, src, dst = inputs(N, dev)
    result["dense_flow"] = verdict(contest(dense_fns(image, g, flow), args.iters, args.rounds))
    print("dense_flow", result["dense_flow"], file=sys.stderr, flush=True)
    del flow
    torch.cuda.empty_cache()
    fns = points_fns(image, g, src, dst)
    if runs(fns["torch_body"]):
        result["points"] = verdict(contest(fns, args.iters, args.rounds))
    else:
        result["points_torch_body_at_full_shape"] = "cannot allocate"
        one = contest({"hip": fns["hip"]}, args.iters, args.rounds)
        result["points_hip_alone"] = one["hip"]
        n = N // 2
        while n >= 1:
            sub = points_fns(image[:n].contiguous(), g[:n].contiguous(), src[:n].contiguous(), dst[:n].contiguous())
            if runs(sub["torch_body"]):
                result["points"] = verdict(contest(sub, args.iters, args.rounds))
                result["points"]["N"] = n
                break
            n //= 2
    print("points", result.get("points"), file=sys.stderr, flush=True)
    # the two routes compute the same gradients (the torch body in float32 sampling, float64 sums)
    n = min(N, 8)
    sub = points_fns(image[:n].contiguous(), g[:n].contiguous(), src[:n].contiguous(), dst[:n].contiguous())
    a, b = sub["hip"](), sub["torch_body"]()
    result["points_max_relative_difference"] = [
        round(float((x - y).abs().max() / y.abs().max()), 6) for x, y in zip(a, b)
    ]
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
