"""The one-launch CTC search for beams of 33 to 128 prefixes (csrc/ctc_search_wide.hip) against the
frame-by-frame route it replaces for those widths, in one process:

    python profiles/tools/time_ctc_wide.py [--out profiles/ctc_wide_times.json]

For each shape: ``CTCPrefixSearch(K)(logits)`` and ``CTCPrefixSearch(K)._frame_by_frame(logits, None, {})``
on the same peaky logits (peak scale 8); two warm-ups, then five repetitions timed with device events around
the call; median, minimum and spread of the five, and the ratio of the medians.  The requirement: the new
route's median is below the old route's minimum at both shapes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pydrobert_amd import modules as M  # noqa: E402

SHAPES = [(300, 1024, 256, 64), (300, 1024, 1000, 128)]  # (T, N, V, K)


def peaky_logits(T, N, V, device, seed, scale=8.0):
    gen = torch.Generator(device=device).manual_seed(seed)
    lg = torch.randn((T, N, V + 1), device=device, generator=gen)
    peak = torch.randint(0, V + 1, (T, N, 1), device=device, generator=gen)
    return lg.scatter_add_(2, peak, torch.full((T, N, 1), scale, device=device))


def timed(call, warm=2, reps=5):
    for _ in range(warm):
        call()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return {
        "median_ms": float(np.median(times)),
        "min_ms": float(np.min(times)),
        "max_ms": float(np.max(times)),
        "spread": float((np.max(times) - np.min(times)) / np.median(times)),
        "times_ms": [float(x) for x in times],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_wide_times.json"))
    args = ap.parse_args()
    device = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(device), "warmups": 2, "repetitions": 5, "peak_scale": 8.0, "shapes": []}
    for T, N, V, K in SHAPES:
        lg = peaky_logits(T, N, V, device, 1000 + K)
        search = M.CTCPrefixSearch(K)
        with torch.no_grad():
            new = timed(lambda: search(lg))
            old = timed(lambda: search._frame_by_frame(lg, None, {}))
            (y1, l1, _), (y2, l2, _) = search(lg), search._frame_by_frame(lg, None, {})
            same = int(((y1 == y2).all(0).all(-1) & (l1 == l2).all(-1)).sum().item())  # (near ties may differ)
        row = {
            "T": T, "N": N, "V": V, "width": K,
            "one_launch": new, "frame_by_frame": old,
            "ratio_of_medians": old["median_ms"] / new["median_ms"],
            "new_median_below_old_minimum": new["median_ms"] < old["min_ms"],
            "utterances_with_equal_beams": same,
        }  # fmt: skip
        result["shapes"].append(row)
        print(json.dumps(row))
        del lg
        # write after every shape, so a run that is cut short still leaves what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
