"""Call times of multi-head self-attention in float16 / bfloat16, forward + backward, with the matrix-core backward
(PDT_ATTN_MFMA_BWD=1, csrc/attn_mfma_bwd.hip) and without it (0: attn_bwd_half_kernel), the forward on its default,
through the public API only.  Method and shapes of profiles/tools/time_half_attn_mfma.py: one
sample is a WINDOW of back-to-back calls between two device events, divided by the number of calls, sized to about
30 ms from three timed calls; 15 windows per setting, the two settings alternating in one run on one device; every
shape warmed first; min / median / max per setting.

  python profiles/tools/time_half_attn_mfma_bwd.py [--windows 15] [--shapes hd64,hd128,hd64_n1] [--out FILE]

``backward_gflop`` is the five matrix products of the heads' attention backward, 10 N H T T d, halved for the causal
mask; ``backward_gflop_executed`` the seven that the two kernels form (S and dP twice).  Divide by the two kernels'
time of a ``rocprofv3 --kernel-trace --stats`` run of this tool (a process of its own) for the rate."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_half_attn_mfma import DTYPES, ROOT, SHAPES, stats3  # noqa: E402


def measure(args):
    import torch

    from pydrobert_amd import modules as M
    from pydrobert_amd import switches

    dev = torch.device("cuda:0")

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    result = {"windows": args.windows, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        T, N, model, H = SHAPES[name]
        d = model // H
        entry = {"T": T, "N": N, "model": model, "heads": H, "head_dim": d,
                 "backward_gflop": round(10 * N * H * T * T * d / 2 / 1e9, 3),
                 "backward_gflop_executed": round(14 * N * H * T * T * d / 2 / 1e9, 3), "forward_backward": {}}  # fmt: skip
        mask = torch.arange(T, device=dev).view(T, 1, 1) <= torch.arange(T, device=dev).view(1, T, 1)
        for dt in DTYPES:
            tdt = getattr(torch, dt)
            torch.manual_seed(0)
            m = M.MultiHeadedAttention(model, model, model, H, M.DotProductSoftAttention(d, 0, d ** -0.5)).to(dev, tdt)
            leaf = torch.randn(T, N, model, device=dev).to(tdt).requires_grad_(True)
            with torch.no_grad():
                gy = torch.randn_like(m(leaf, leaf.unsqueeze(1), leaf.unsqueeze(1), mask))

            def fwd_bwd():
                leaf.grad = None
                m.zero_grad(set_to_none=True)
                m(leaf, leaf.unsqueeze(1), leaf.unsqueeze(1), mask).backward(gy)

            calls, times = {}, {0: [], 1: []}
            for sw in (0, 1):  # warm-up, then the calls of a window of about 30 ms
                with switches.override(PDT_ATTN_MFMA_BWD=sw):
                    fwd_bwd()
                    fwd_bwd()
                    torch.cuda.synchronize()
                    calls[sw] = max(1, min(200, math.ceil(30.0 / max(window(fwd_bwd, 3), 1e-3))))
            for _ in range(args.windows):
                for sw in (0, 1):
                    with switches.override(PDT_ATTN_MFMA_BWD=sw):
                        times[sw].append(window(fwd_bwd, calls[sw]))
            rec = {}
            for sw in (0, 1):
                lo, med, hi = stats3(times[sw])
                rec["bwd_%d" % sw] = {"ms_min": lo, "ms_median": med, "ms_max": hi, "calls_per_window": calls[sw]}
            a, b = rec["bwd_1"], rec["bwd_0"]
            spread = (a["ms_max"] - a["ms_min"]) + (b["ms_max"] - b["ms_min"])
            rec["combined_spread_ms"] = round(spread, 4)
            rec["ratio_0_over_1"] = round(b["ms_median"] / a["ms_median"], 3)
            rec["meets"] = a["ms_median"] < b["ms_median"] - spread
            entry["forward_backward"][dt] = rec
            print(name, dt, json.dumps(rec), flush=True)
        result["shapes"][name] = entry
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_attn_mfma_bwd_times.json"))
    args = ap.parse_args()
    result = measure(args)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
