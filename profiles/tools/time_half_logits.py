"""Call times and peak memory of the logits-sized decoders and scorers for float32, float16 and bfloat16
logits, through the public API only -- so the same file runs on a checkout that still makes a float32 copy of
half logits (DESIGN.md section 11 compares the two).

  python profiles/tools/time_half_logits.py [--windows 15] [--shapes headline,c3,c5,greedy,slp] [--label NAME]
                                            [--out profiles/half_logits_times.json]
  python profiles/tools/time_half_logits.py --compare OTHER.json [--out THIS.json]     (no device work)

Protocol: one sample is a WINDOW of back-to-back calls between two events, divided by
the number of calls; 15 windows per dtype, the dtypes alternating; min / median / max per dtype.  The calls per
window are sized so that a window is tens of milliseconds.  Peak memory: growth of max_memory_allocated across
one call, outputs included.

Shapes: ctc_prefix_search at the headline (N=4096, T=512, V=256, K=16), C3 (N=1024, T=1000, V=1000, K=16) and
the C5 shard (N=4096, T=512, V=5000, K=16); ctc_greedy_search and sequence_log_probs forward + backward at
N=4096, T=512, 257 classes.

--compare: for every half dtype and shape, THIS median against OTHER's; the criterion is that THIS median does
not exceed OTHER's by more than the two runs' combined spread (max - min over the windows of each)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

DTYPES = ("float32", "float16", "bfloat16")
SHAPES = {
    # name: (operator, T, N, classes, width, calls per window)
    "headline": ("ctc_prefix_search", 512, 4096, 257, 16, 12),
    "c3": ("ctc_prefix_search", 1000, 1024, 1001, 16, 8),
    "c5": ("ctc_prefix_search", 512, 4096, 5001, 16, 4),
    "greedy": ("ctc_greedy_search", 512, 4096, 257, 0, 20),
    "slp": ("sequence_log_probs", 512, 4096, 257, 0, 10),
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

    def growth(fn):
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
        op, T, N, C, W, calls = SHAPES[name]
        gen = torch.Generator(device=dev).manual_seed(1)
        base = torch.empty((T, N, C), device=dev, dtype=torch.float32)
        for t0 in range(0, T, 64):  # (filled in slices: no second logits-sized temporary)
            base[t0 : t0 + 64].normal_(0.0, 3.0, generator=gen)
        xs = {"float32": base, "float16": base.half(), "bfloat16": base.bfloat16()}
        hyp = torch.randint(0, C, (T, N), device=dev, generator=gen)
        fns = {}
        for d in DTYPES:
            x = xs[d]
            if op == "ctc_prefix_search":
                fns[d] = lambda x=x: F.ctc_prefix_search(x, W)
            elif op == "ctc_greedy_search":
                fns[d] = lambda x=x: F.ctc_greedy_search(x)
            else:
                leaf = x.requires_grad_(True)
                go = torch.ones((N,), device=dev, dtype=x.dtype)

                def slp(leaf=leaf, go=go):
                    leaf.grad = None
                    F.sequence_log_probs(leaf, hyp, 0).backward(go)
                    return leaf.grad

                fns[d] = slp
        entry = {"operator": op, "T": T, "N": N, "classes": C, "width": W, "calls_per_window": calls,
                 "elements": T * N * C, "dtypes": {}}
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
            entry["dtypes"][d] = {"ms_min": lo, "ms_median": med, "ms_max": hi, "peak_growth_bytes": growth(fns[d])}
            print("{:9s} {:9s} ms/call {} / {} / {}   peak growth {:.1f} MB".format(
                name, d, lo, med, hi, entry["dtypes"][d]["peak_growth_bytes"] / 1e6), flush=True)
        result["shapes"][name] = entry
        del xs, base, fns, hyp
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_logits_times.json"))
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
