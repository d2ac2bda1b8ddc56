"""Call times of multi-head self-attention in float32 with the matrix-core forward (PDT_ATTN_MFMA_F32=1,
csrc/attn_mfma_f32.hip) and without it (0: attn_fwd_kernel, the parent's route in the same library), forward alone
and forward + backward, through the public API only.  Method of
profiles/tools/time_half_attn_mfma.py: one sample is a WINDOW of back-to-back calls between two device events,
divided by the number of calls, sized to about 30 ms from three timed calls; 15 windows per setting, the two
settings alternating in one run on one device; every shape warmed first; min / median / max per setting.

  python profiles/tools/time_f32_attn_mfma.py [--windows 15] [--shapes hd64,hd128,hd64_n1] [--out FILE]
  python profiles/tools/time_f32_attn_mfma.py --errors [--out profiles/f32_attn_mfma_errors.json]
  python profiles/tools/time_f32_attn_mfma.py --switch PDT_ATTN_MFMA_F32_BWD --passes forward_backward \
      --out profiles/f32_attn_mfma_bwd_times.json

--switch: the switch that alternates between 0 and 1 (every other one on its default): PDT_ATTN_MFMA_F32_BWD times the
matrix-core backward (csrc/attn_mfma_f32_bwd.hip) against attn_bwd_kernel with the forward on
the matrix cores under both settings; ``attention_gflop`` is the forward's either way.

Shapes: causal self-attention over T = 1000 frames; hd64: N = 16, model 256, 4 heads; hd128: N = 16, model 1024,
8 heads; hd64_n1: N = 1, model 256, 4 heads (few groups: T is split).  ``attention_gflop`` is the two matrix
products of the heads' attention, 4 N H T T d, halved for the causal mask; divide it by the kernel time of a
``rocprofv3 --kernel-trace --stats`` run of this tool (a process of its own) for the rate.

--errors: for every case of tests/_attn_mfma_f32.py the largest error / bound of ``out`` and of ``lse`` against
float64 (the bounds of tests/test_attn_mfma_f32_gpu.py), and for its gradient cases those of dQ, dK, dV."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

SHAPES = {"hd64": (1000, 16, 256, 4), "hd128": (1000, 16, 1024, 8), "hd64_n1": (1000, 1, 256, 4)}
PASSES = ("forward", "forward_backward")


def stats3(v):
    v = sorted(v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


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

    result = {"switch": args.switch, "windows": args.windows, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes.split(","):
        T, N, model, H = SHAPES[name]
        d = model // H
        entry = {"T": T, "N": N, "model": model, "heads": H, "head_dim": d,
                 "attention_gflop": round(4 * N * H * T * T * d / 2 / 1e9, 3), "passes": {}}  # fmt: skip
        mask = torch.arange(T, device=dev).view(T, 1, 1) <= torch.arange(T, device=dev).view(1, T, 1)
        torch.manual_seed(0)
        m = M.MultiHeadedAttention(model, model, model, H, M.DotProductSoftAttention(d, 0, d ** -0.5)).to(dev)
        x = torch.randn(T, N, model, device=dev)
        leaf = x.clone().requires_grad_(True)
        with torch.no_grad():
            gy = torch.randn_like(m(x, x.unsqueeze(1), x.unsqueeze(1), mask))

        def fwd():
            with torch.no_grad():
                return m(x, x.unsqueeze(1), x.unsqueeze(1), mask)

        def fwd_bwd():
            leaf.grad = None
            m.zero_grad(set_to_none=True)
            m(leaf, leaf.unsqueeze(1), leaf.unsqueeze(1), mask).backward(gy)

        for p, fn in zip(PASSES, (fwd, fwd_bwd)):
            if p not in args.passes.split(","):
                continue
            calls, times = {}, {0: [], 1: []}
            for sw in (0, 1):  # warm-up, then the calls of a window of about 30 ms
                with switches.override(**{args.switch: sw}):
                    fn()
                    fn()
                    torch.cuda.synchronize()
                    calls[sw] = max(1, min(200, math.ceil(30.0 / max(window(fn, 3), 1e-3))))
            for _ in range(args.windows):
                for sw in (0, 1):
                    with switches.override(**{args.switch: sw}):
                        times[sw].append(window(fn, calls[sw]))
            rec = {}
            for sw in (0, 1):
                lo, med, hi = stats3(times[sw])
                rec["mfma_%d" % sw] = {"ms_min": lo, "ms_median": med, "ms_max": hi, "calls_per_window": calls[sw]}
            a, b = rec["mfma_1"], rec["mfma_0"]
            spread = (a["ms_max"] - a["ms_min"]) + (b["ms_max"] - b["ms_min"])
            rec["combined_spread_ms"] = round(spread, 4)
            rec["ratio_0_over_1"] = round(b["ms_median"] / a["ms_median"], 3)
            rec["meets"] = a["ms_median"] < b["ms_median"] - spread
            entry["passes"][p] = rec
            print(name, p, json.dumps(rec), flush=True)
        result["shapes"][name] = entry
    return result


def errors():
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _attn_mfma_f32 as C
    import _attn_ref as R

    from pydrobert_amd import _attn

    dev = torch.device("cuda:0")
    out_tol, grad_tol = R.SUITE["float32"]

    def grads(fn, q, k, v, gout):
        leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad((fn(*leaves).double() * gout.to(q.device)).sum(), leaves)

    result = {}
    for name in C.CASES:
        x, ref = C.inputs(name), C.reference(name)
        q, k, v = (torch.empty_strided(x[n].size(), x[n].stride(), device=dev).copy_(x[n]) for n in ("q", "k", "v"))
        mask, scale = None if x["mask"] is None else x["mask"].to(dev), x["scale"]
        plan, ops = _attn._dot_plan(q, k, v, mask, 0)
        assert _attn._mfma_f32_workspace_bytes(plan, 0, ops) >= 0, name
        out, lse = (t.cpu().double() for t in torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, 0, scale))
        live = ~torch.isnan(ref["out"]).any(-1).reshape(-1)
        err = (out - ref["out"]).abs().reshape(live.numel(), -1)[live]
        bound = (out_tol + out_tol * ref["out"].abs()).clamp_min(8 * ref["err32"]).reshape(live.numel(), -1)[live]
        rec = {"formula_error_float32": ref["err32"], "out": round(float((err / bound).max()), 4)}
        for n, got, want in (("lse_max", lse[0], ref["m"]), ("lse_logsum", lse[1], ref["logsum"])):
            rec[n] = round(float(((got - want).abs()[live] / (2e-5 * (1 + want.abs()[live]))).max()), 4)
        if name in C.GRAD_CASES:
            gout = torch.from_numpy(np.random.default_rng(5).normal(size=ref["out"].shape))
            cpu, cm = [x["q"], x["k"], x["v"]], x["mask"]
            got = grads(lambda a, b, c: _attn.dot_attention(a, b, c, mask, 0, scale), q, k, v, gout)
            want = grads(lambda a, b, c: R.attend_ref(a, b, c, cm, 0, scale), *(t.double() for t in cpu), gout)
            form = grads(lambda a, b, c: _attn._softmax_pool((a.unsqueeze(0) * b).sum(-1) * scale, c, cm, 0), *cpu, gout)
            for n, g, w, f in zip(("dq", "dk", "dv"), got, want, form):
                e_ref = float((f.double() - w).abs().max())
                b = (grad_tol + grad_tol * w.abs()).clamp_min(8 * e_ref)
                rec[n] = round(float(((g.cpu().double() - w).abs() / b).max()), 4)
        result[name] = rec
        print(name, json.dumps(rec), flush=True)
    return {"largest_error_over_bound": result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--switch", default="PDT_ATTN_MFMA_F32")
    ap.add_argument("--passes", default=",".join(PASSES))
    ap.add_argument("--errors", action="store_true")
    args = ap.parse_args()
    default = "f32_attn_mfma_errors.json" if args.errors else "f32_attn_mfma_times.json"
    out = args.out or os.path.join(ROOT, "profiles", default)
    result = errors() if args.errors else measure(args)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
