"""Call times and peak memory of SpecAugment for float32, float16 and bfloat16 features through the public API
only -- so the same file runs on a checkout where half features still go through float32 copies (DESIGN.md
section 13 compares the two).

  python profiles/tools/time_half_spec.py [--windows 15] [--shapes apply_parameters,module_forward,rows_backward]
                                          [--label NAME] [--out profiles/half_spec_times.json]
  python profiles/tools/time_half_spec.py --compare OTHER.json [--out THIS.json] [--write BOTH.json]   (no device work)

Protocol (that of profiles/tools/time_half_attn.py): one sample is a WINDOW of back-to-back calls between two
device events, divided by the number of calls; 15 windows per dtype, the dtypes alternating; min / median / max
per dtype.  The calls per window are sized from three timed calls so that a window is about 30 ms.  Peak memory:
growth of max_memory_allocated across one call.

Shapes: the benchmark's C4, N=2048 x T=1000 x F=80 with a time warp, two time and two frequency masks --
``apply_parameters`` on drawn parameters (one launch of the rows kernel), the same through ``SpecAugment.forward``
(draw + apply behind one operator), and the rows (gather) backward: ``torch.autograd.grad`` of ``apply_parameters``'
output, the forward outside the window.

--compare: for every shape and dtype, THIS median against OTHER's; the criterion is that THIS median does not
exceed OTHER's by more than the two runs' combined spread (max - min over the windows of each); for float32, that
the two medians differ by less than that spread.  --write stores both runs and the comparison in one file."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

DTYPES = ("float32", "float16", "bfloat16")
SHAPES = ("apply_parameters", "module_forward", "rows_backward")


def stats3(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


def measure(args):
    import torch

    from pydrobert_amd import modules as M

    dev = torch.device("cuda:0")
    tdt = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    def growth(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        del out
        return int(peak - base)

    N, T, Fq = 2048, 1000, 80
    g = torch.Generator(device=dev).manual_seed(7)
    feats32 = torch.randn((N, T, Fq), device=dev, generator=g)
    lens = torch.randint(500, T + 1, (N,), device=dev, generator=g)
    sa = M.SpecAugment(max_time_warp=80.0, max_freq_warp=0.0, max_time_mask=100, max_freq_mask=27,
                       max_time_mask_proportion=0.04, num_time_mask=2, num_time_mask_proportion=1.0,
                       num_freq_mask=2, interpolation_order=1)  # fmt: skip
    torch.manual_seed(0)
    params = sa.draw_parameters(feats32, lens)
    result = {"label": args.label, "windows": args.windows, "device": torch.cuda.get_device_name(0),
              "workload": "N=2048 T=1000 F=80, time warp + 2 time + 2 freq masks", "shapes": {}}  # fmt: skip
    fns = {s: {} for s in SHAPES}
    for d in DTYPES:
        x = feats32.to(tdt[d])
        leaf = x.clone().requires_grad_(True)
        y = sa.apply_parameters(leaf, params, lens)
        gy = torch.randn((N, T, Fq), device=dev, generator=g).to(tdt[d])

        def apply_(x=x):
            with torch.no_grad():
                return sa.apply_parameters(x, params, lens)

        def forward_(x=x):
            with torch.no_grad():
                return sa(x, lens)

        def backward_(y=y, leaf=leaf, gy=gy):
            return torch.autograd.grad(y, leaf, gy, retain_graph=True)[0]

        fns["apply_parameters"][d], fns["module_forward"][d], fns["rows_backward"][d] = apply_, forward_, backward_
    for s in args.shapes.split(","):
        calls, times = {}, {d: [] for d in DTYPES}
        for d in DTYPES:  # warm-up, then the calls of a window of about 30 ms
            fns[s][d]()
            fns[s][d]()
            torch.cuda.synchronize()
            calls[d] = max(1, min(200, math.ceil(30.0 / max(window(fns[s][d], 3), 1e-3))))
        for _ in range(args.windows):
            for d in DTYPES:
                times[d].append(window(fns[s][d], calls[d]))
        entry = {}
        for d in DTYPES:
            lo, med, hi = stats3(times[d])
            entry[d] = {"ms_min": lo, "ms_median": med, "ms_max": hi, "calls_per_window": calls[d],
                        "peak_growth_bytes": growth(fns[s][d])}  # fmt: skip
            print("{:18s} {:9s} ms/call {} / {} / {}   peak growth {:.1f} MB".format(
                s, d, lo, med, hi, entry[d]["peak_growth_bytes"] / 1e6), flush=True)
        result["shapes"][s] = entry
    return result


def compare(this, other):
    rows = []
    for s, e in this["shapes"].items():
        o = other["shapes"].get(s)
        if o is None:
            continue
        for d in DTYPES:
            a, b = e[d], o[d]
            spread = (a["ms_max"] - a["ms_min"]) + (b["ms_max"] - b["ms_min"])
            if d == "float32":
                meets = abs(a["ms_median"] - b["ms_median"]) < spread
            else:
                meets = a["ms_median"] <= b["ms_median"] + spread
            rows.append({
                "shape": s, "dtype": d, "this_ms": a["ms_median"], "other_ms": b["ms_median"],
                "combined_spread_ms": round(spread, 4),
                "ratio_other_over_this": round(b["ms_median"] / a["ms_median"], 3), "meets": meets,
                "this_peak_MB": round(a["peak_growth_bytes"] / 1e6, 1),
                "other_peak_MB": round(b["peak_growth_bytes"] / 1e6, 1),
            })  # fmt: skip
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", default=None, help="another run's JSON: compare the run in --out against it")
    ap.add_argument("--write", default=None, help="with --compare: store both runs and the comparison here")
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", "half_spec_times.json")
    if args.compare:
        this, other = json.load(open(out)), json.load(open(args.compare))
        this, other = this.get("this", this), other.get("this", other)
        rows = compare(this, other)
        for r in rows:
            print(json.dumps(r))
        if args.write:
            with open(args.write, "w") as f:
                json.dump({"this": this, "parent": other, "comparison": rows}, f, indent=1)
                f.write("\n")
        return
    result = measure(args)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
