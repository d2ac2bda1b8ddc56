"""Call times and peak memory of the hard optimal-completion distillation loss, forward + backward of the
"mean" loss, for float32, float16 and bfloat16 logits, through the public API only -- so the same file runs on a
checkout that still makes float32 copies of half logits (DESIGN.md section 11 compares the two).

  python profiles/tools/time_half_loss.py [--windows 15] [--shapes v256,v1000,v5000] [--label NAME]
                                          [--out profiles/half_loss_times.json]
  python profiles/tools/time_half_loss.py --compare OTHER.json [--out THIS.json]     (no device work)

Protocol (that of profiles/tools/time_half_logits.py): one sample is a WINDOW of back-to-back calls between two
events, divided by the number of calls; 15 windows per dtype, the dtypes alternating; min / median / max per
dtype.  The calls per window are sized so that a window is tens of milliseconds.  Peak memory: growth of
max_memory_allocated across one call that starts without a gradient, the returned gradient included.

Shapes: H = 256 prefixes, N = 1024 utterances, references of R = 40 tokens, one vocabulary per row form of
csrc/ocd_loss.hip: V = 256 (8 registers per lane), V = 1000 (16 registers), V = 5000 (streamed).

--compare: for every dtype and shape, THIS median against OTHER's; the criterion is that THIS median does not
exceed OTHER's by more than the two runs' combined spread (max - min over the windows of each)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

DTYPES = ("float32", "float16", "bfloat16")
SHAPES = {
    # name: (H, N, V, R, calls per window)
    "v256": (256, 1024, 256, 40, 20),
    "v1000": (256, 1024, 1000, 40, 10),
    "v5000": (256, 1024, 5000, 40, 4),
}


def stats3(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


def measure(args):
    import torch

    from pydrobert_amd import functional as F

    dev = torch.device("cuda:0")

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls

    def growth(fn, leaf):
        leaf.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        del out
        return int(peak - base)

    result = {"label": args.label, "windows": args.windows, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        H, N, V, R, calls = SHAPES[name]
        gen = torch.Generator(device=dev).manual_seed(1)
        base = torch.empty((H, N, V), device=dev, dtype=torch.float32)
        for h0 in range(0, H, 64):  # (filled in slices: no second logits-sized temporary)
            base[h0 : h0 + 64].normal_(0.0, 3.0, generator=gen)
        ref = torch.randint(0, V, (R, N), device=dev, generator=gen)
        hyp = torch.randint(0, V, (H, N), device=dev, generator=gen)
        leaves = {"float32": base, "float16": base.half(), "bfloat16": base.bfloat16()}
        fns = {}
        for d in DTYPES:
            leaf = leaves[d].requires_grad_(True)

            def step(leaf=leaf):
                leaf.grad = None
                F.hard_optimal_completion_distillation_loss(leaf, ref, hyp, reduction="mean", warn=False).backward()
                return leaf.grad

            fns[d] = step
        entry = {"operator": "hard_optimal_completion_distillation_loss forward + backward", "H": H, "N": N, "V": V,
                 "R": R, "calls_per_window": calls, "elements": H * N * V, "dtypes": {}}
        times = {d: [] for d in DTYPES}
        for d in DTYPES:  # warm-up: instance selection, allocator
            fns[d]()
            fns[d]()
        torch.cuda.synchronize()
        for _ in range(args.windows):
            for d in DTYPES:
                times[d].append(window(fns[d], calls))
        for d in DTYPES:
            lo, med, hi = stats3(times[d])
            entry["dtypes"][d] = {"ms_min": lo, "ms_median": med, "ms_max": hi,
                                  "peak_growth_bytes": growth(fns[d], leaves[d])}
            print("{:6s} {:9s} ms/call {} / {} / {}   peak growth {:.1f} MB".format(
                name, d, lo, med, hi, entry["dtypes"][d]["peak_growth_bytes"] / 1e6), flush=True)
        result["shapes"][name] = entry
        for d in DTYPES:
            leaves[d].grad = None
        del leaves, base, fns, ref, hyp
        torch.cuda.empty_cache()
    return result


def compare(this, other):
    rows = []
    for name, e in this["shapes"].items():
        o = other["shapes"].get(name)
        if o is None:
            continue
        for d in DTYPES:
            a, b = e["dtypes"][d], o["dtypes"][d]
            spread = (a["ms_max"] - a["ms_min"]) + (b["ms_max"] - b["ms_min"])
            rows.append({
                "shape": name, "dtype": d, "this_ms": a["ms_median"], "other_ms": b["ms_median"],
                "combined_spread_ms": round(spread, 4), "ratio_other_over_this": round(b["ms_median"] / a["ms_median"], 3),
                "meets": a["ms_median"] <= b["ms_median"] + spread,
                "this_peak_MB": round(a["peak_growth_bytes"] / 1e6, 1), "other_peak_MB": round(b["peak_growth_bytes"] / 1e6, 1),
            })
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_loss_times.json"))
    ap.add_argument("--compare", default=None, help="another run's JSON: compare the run in --out against it")
    args = ap.parse_args()
    if args.compare:
        this, other = json.load(open(args.out)), json.load(open(args.compare))
        for r in compare(this, other):
            print(json.dumps(r))
        return
    result = measure(args)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
