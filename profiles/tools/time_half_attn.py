"""Call times and peak memory of the attention modules for float32, float16 and bfloat16 operands, forward alone
and forward + backward, through the public API only -- so the same file runs on a checkout where half operands
still take the reference's formula in torch (DESIGN.md section 12 compares the two).

  python profiles/tools/time_half_attn.py [--windows 15] [--shapes decode_dot,training_dot,self_attention_4heads]
                                          [--label NAME] [--out profiles/half_attn_times.json]
  python profiles/tools/time_half_attn.py --compare OTHER.json [--out THIS.json]     (no device work)
  python profiles/tools/time_half_attn.py --errors [--out profiles/half_attn_errors.json]

Protocol (that of profiles/tools/time_half_loss.py): one sample is a WINDOW of back-to-back calls between two
device events, divided by the number of calls; 15 windows per dtype, the dtypes alternating; min / median / max
per dtype.  The calls per window are sized from three timed calls so that a window is about 30 ms.  Peak memory:
growth of max_memory_allocated across one call.

Shapes: decode dot (N=128 utterances, K=8 beams, T=512, D=512, a length mask), the
training step (N=256, T=512, D=512, no group) and four-head causal self-attention (T=1000, N=16, D=64).  Modules
and inputs are in the dtype (``module.to(dtype)``: a model kept in half precision).

--compare: for every dtype, shape and pass, THIS median against OTHER's; the criterion is that THIS median does
not exceed OTHER's by more than the two runs' combined spread (max - min over the windows of each).

--errors: the largest absolute error of the output and of every gradient against the float64 formula on the
widened half inputs, for the HIP route and for the reference's formula in torch on the same half tensors, over the
float32 cases of tests/_attn_ref.py whose bounds are the suite's (not ``measured``)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

DTYPES = ("float32", "float16", "bfloat16")
SHAPES = ("decode_dot", "training_dot", "self_attention_4heads")
PASSES = ("forward", "forward_backward")


def stats3(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


def build(name, torch, M, dev):
    """(module, (query, key, value), mask) of a shape, float32."""
    g = torch.Generator(device=dev).manual_seed(0)
    torch.manual_seed(0)
    if name == "decode_dot":
        N, K, T, D = 128, 8, 512, 512
        lens = torch.randint(T // 2, T + 1, (N,), device=dev, generator=g)
        mask = torch.arange(T, device=dev).view(T, 1, 1) < lens.view(1, N, 1)
        ins = (torch.randn(N, K, D, device=dev, generator=g), torch.randn(T, N, 1, D, device=dev, generator=g),
               torch.randn(T, N, 1, D, device=dev, generator=g))  # fmt: skip
        return M.DotProductSoftAttention(D, 0, D ** -0.5), ins, mask
    if name == "training_dot":
        N, T, D = 256, 512, 512
        ins = (torch.randn(N, D, device=dev, generator=g), torch.randn(T, N, D, device=dev, generator=g),
               torch.randn(T, N, D, device=dev, generator=g))  # fmt: skip
        return M.DotProductSoftAttention(D, 0, D ** -0.5), ins, None
    T, N, D = 1000, 16, 64
    ins = (torch.randn(T, N, D, device=dev, generator=g), torch.randn(T, 1, N, D, device=dev, generator=g),
           torch.randn(T, 1, N, D, device=dev, generator=g))  # fmt: skip
    mask = torch.arange(T, device=dev).view(T, 1, 1) <= torch.arange(T, device=dev).view(1, T, 1)
    m = M.MultiHeadedAttention(D, D, D, 4, M.DotProductSoftAttention(D // 4, 0, (D // 4) ** -0.5)).to(dev)
    return m, ins, mask


def measure(args):
    import copy

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

    result = {"label": args.label, "windows": args.windows, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        m32, ins32, mask = build(name, torch, M, dev)
        entry = {"passes": {}}
        fns = {p: {} for p in PASSES}
        for d in DTYPES:
            m = copy.deepcopy(m32).to(tdt[d])
            ins = [x.to(tdt[d]) for x in ins32]
            leaves = [x.clone().requires_grad_(True) for x in ins]
            with torch.no_grad():
                gy = torch.randn_like(m(*ins, mask))

            def fwd(m=m, ins=ins):
                with torch.no_grad():
                    return m(*ins, mask)

            def fwd_bwd(m=m, leaves=leaves, gy=gy):
                for x in leaves:
                    x.grad = None
                m.zero_grad(set_to_none=True)
                m(*leaves, mask).backward(gy)
                return [x.grad for x in leaves]

            fns["forward"][d], fns["forward_backward"][d] = fwd, fwd_bwd
        for p in PASSES:
            calls, times = {}, {d: [] for d in DTYPES}
            for d in DTYPES:  # warm-up, then the calls of a window of about 30 ms
                fns[p][d]()
                fns[p][d]()
                torch.cuda.synchronize()
                calls[d] = max(1, min(200, math.ceil(30.0 / max(window(fns[p][d], 3), 1e-3))))
            for _ in range(args.windows):
                for d in DTYPES:
                    times[d].append(window(fns[p][d], calls[d]))
            entry["passes"][p] = {}
            for d in DTYPES:
                lo, med, hi = stats3(times[d])
                entry["passes"][p][d] = {"ms_min": lo, "ms_median": med, "ms_max": hi, "calls_per_window": calls[d],
                                         "peak_growth_bytes": growth(fns[p][d])}  # fmt: skip
                print("{:22s} {:16s} {:9s} ms/call {} / {} / {}   peak growth {:.1f} MB".format(
                    name, p, d, lo, med, hi, entry["passes"][p][d]["peak_growth_bytes"] / 1e6), flush=True)
        result["shapes"][name] = entry
        del fns, m32, ins32
        torch.cuda.empty_cache()
    return result


def compare(this, other):
    rows = []
    for name, e in this["shapes"].items():
        o = other["shapes"].get(name)
        if o is None:
            continue
        for p in PASSES:
            for d in DTYPES:
                a, b = e["passes"][p][d], o["passes"][p][d]
                spread = (a["ms_max"] - a["ms_min"]) + (b["ms_max"] - b["ms_min"])
                rows.append({
                    "shape": name, "pass": p, "dtype": d, "this_ms": a["ms_median"], "other_ms": b["ms_median"],
                    "combined_spread_ms": round(spread, 4),
                    "ratio_other_over_this": round(b["ms_median"] / a["ms_median"], 3),
                    "meets": a["ms_median"] <= b["ms_median"] + spread,
                    "this_peak_MB": round(a["peak_growth_bytes"] / 1e6, 1),
                    "other_peak_MB": round(b["peak_growth_bytes"] / 1e6, 1),
                })  # fmt: skip
    return rows


def errors():
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _attn_ref as R

    from pydrobert_amd import _attn

    dev = torch.device("cuda:0")

    def formula_dot(query, key, value, mask, dim, scale):
        return _attn._softmax_pool((query.unsqueeze(dim) * key).sum(-1) * scale, value, mask, dim)

    def run(name, dot, pool, half, dtype, device, dropped):
        """R.run_case with the leaves rounded to ``half`` first (then widened to ``dtype``)."""
        c, x = R.CASES[name], R.build_inputs(name)
        G, M, T, Dv = c["G"], c["M"], c["T"], c["Dv"]
        mask, gout = x["mask"], x["gout"]
        if dropped and x["dead"].any():
            mask, gout = R.drop_rows(mask, gout, x["dead"])
        L = {n: torch.from_numpy(x[n].copy()).to(half).to(device=device, dtype=dtype).requires_grad_(True)
             for n in R.LEAVES[c["route"]]}  # fmt: skip
        mask_t = None if mask is None else torch.from_numpy(mask.copy()).to(device)
        value = L["v"].expand(T, G, M, Dv) if c["expand"] else L["v"]
        if c["route"] == "dot":
            key = L["k"].expand(T, G, M, c["D"]) if c["expand"] else L["k"]
            out = dot(L["q"][..., ::c["qstride"]], key, value, mask_t, 0, x["scale"])
        else:
            out = pool(L["e"], value, mask_t, 0)
        g = torch.from_numpy(gout.copy()).to(half).to(device=device, dtype=dtype)
        grads = torch.autograd.grad(out, list(L.values()), g)
        return out.detach().double().cpu(), {n: t.detach().double().cpu() for n, t in zip(L, grads)}

    names = [n for n, c in R.CASES.items() if c["dtype"] == "float32" and not c["measured"]]
    result = {"cases": {}, "worst_ratio_hip_over_formula": {}}
    for hname, half in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        worst = {}
        for name in names:
            ref_out, ref_g = run(name, R.attend_ref, R.pool_ref, half, torch.float64, "cpu", True)
            ok = ~torch.isnan(ref_out) & ~torch.from_numpy(R.build_inputs(name)["dead"].copy()).unsqueeze(-1)
            rec = {}
            for route, dot, pool, dropped in (("hip", _attn.dot_attention, _attn.attention_pool, False),
                                              ("formula", formula_dot, _attn._softmax_pool, True)):  # fmt: skip
                out, g = run(name, dot, pool, half, half, dev, dropped)
                rec[route] = {"out": float((out - ref_out)[ok].abs().max())}
                for n in g:
                    rec[route][n] = float((g[n] - ref_g[n]).abs().max())
            result["cases"].setdefault(name, {})[hname] = rec
            for t in rec["hip"]:
                if rec["formula"][t] > 0:
                    r = rec["hip"][t] / rec["formula"][t]
                    if r > worst.get(t, (0.0, ""))[0]:
                        worst[t] = (round(r, 3), name)
        result["worst_ratio_hip_over_formula"][hname] = worst
        print(hname, json.dumps(worst), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", default=None, help="another run's JSON: compare the run in --out against it")
    ap.add_argument("--errors", action="store_true")
    args = ap.parse_args()
    default = "half_attn_errors.json" if args.errors else "half_attn_times.json"
    out = args.out or os.path.join(ROOT, "profiles", default)
    if args.compare:
        this, other = json.load(open(out)), json.load(open(args.compare))
        for r in compare(this, other):
            print(json.dumps(r))
        return
    result = errors() if args.errors else measure(args)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
