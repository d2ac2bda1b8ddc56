"""Call times of float32 decode attention with the matrix-core-score forward (PDT_ATTN_MFMA_DEC=1,
csrc/attn_mfma_dec.hip) and without it (0: attn_fwd_kernel, the parent's route in the same library), forward alone
and forward + backward, through DotProductSoftAttention only.  Method of
profiles/tools/time_f32_attn_mfma.py: one sample is a WINDOW of back-to-back calls between two device events, divided
by the number of calls, sized to about 30 ms from three timed calls; 15 windows per setting, the two settings
alternating in one run on one device; every shape warmed first; min / median / max per setting.

  python profiles/tools/time_attn_mfma_dec.py [--windows 15] [--shapes decode,train,small,decode_peaked] [--out FILE]
  python profiles/tools/time_attn_mfma_dec.py --errors [--out profiles/attn_mfma_dec_errors.json]
  python profiles/tools/time_attn_mfma_dec.py --switch PDT_ATTN_MFMA_DEC_BWD [--errors]

--switch: the switch that alternates between 0 and 1 (every other one on its default).  PDT_ATTN_MFMA_DEC_BWD times the
one-kernel backward (csrc/attn_mfma_dec_bwd.hip) against attn_bwd_kernel with the forward on
csrc/attn_mfma_dec.hip either way, forward + backward only; it writes profiles/attn_mfma_dec_bwd_times.json and, with
--errors, profiles/attn_mfma_dec_bwd_errors.json (the gradient cases of tests/test_attn_mfma_dec_bwd_gpu.py: the
largest error / bound of dQ, dK, dV against float64 and, on the ratio cases, both switches' errors and their ratio).
Its criterion: the switch-1 median below switch 0's by more than the combined spread; at ``small`` not above it by more.

Shapes (N utterances, K rows a group, T frames, D = Dv, lengths from T / 2 to T): decode, section 4.7's: N = 128,
K = 8, T = 512, D = 512; train, a decoder step of a training batch: N = 256, K = 1, T = 512, D = 512; small: N = 16,
K = 4, T = 256, D = 256; decode_peaked: decode with the query times 8, so the scores have a deviation of 8 where the
others have 1 and a few frames carry a row (the kernel sums such scores a second time).  ``kv_mbytes`` is what the
attended frames' keys and values hold; divide it by the kernel time of a ``rocprofv3 --kernel-trace --stats`` run of
this tool (a process of its own) for the rate.

--errors: for every case of tests/_attn_mfma_dec.py the largest error / bound of ``out`` against float64 (the bound
of tests/test_attn_mfma_dec_gpu.py), and for its gradient cases the largest errors of dQ, dK, dV through the
unchanged backward with the switch at 1 and at 0, and their ratio."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

SHAPES = {"decode": (128, 8, 512, 512, 1.0), "train": (256, 1, 512, 512, 1.0), "small": (16, 4, 256, 256, 1.0),
          "decode_peaked": (128, 8, 512, 512, 8.0)}
PASSES = ("forward", "forward_backward")
SWITCH = "PDT_ATTN_MFMA_DEC"
BWD_SWITCH = "PDT_ATTN_MFMA_DEC_BWD"


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
        N, K, T, D, sharp = SHAPES[name]
        torch.manual_seed(0)
        lens = torch.linspace(T // 2, T, N, device=dev).long()
        mask = torch.arange(T, device=dev).view(T, 1, 1) < lens.view(1, N, 1)
        q, k, v = torch.randn(N, K, D, device=dev) * sharp, torch.randn(T, N, 1, D, device=dev), torch.randn(T, N, 1, D, device=dev)
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        gy = torch.randn(N, K, D, device=dev)
        m = M.DotProductSoftAttention(D, 0, D ** -0.5)
        entry = {"N": N, "K": K, "T": T, "D": D, "query_scale": sharp, "kv_mbytes": round(int(lens.sum()) * 2 * D * 4 / 1e6, 3), "passes": {}}

        def fwd():
            with torch.no_grad():
                return m(q, k, v, mask)

        def fwd_bwd():
            for t in leaves:
                t.grad = None
            m(*leaves, mask).backward(gy)

        for p, fn in zip(PASSES, (fwd, fwd_bwd)):
            if args.switch == BWD_SWITCH and p == "forward":
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
                rec["dec_%d" % sw] = {"ms_min": lo, "ms_median": med, "ms_max": hi, "calls_per_window": calls[sw]}
            a, b = rec["dec_1"], rec["dec_0"]
            spread = (a["ms_max"] - a["ms_min"]) + (b["ms_max"] - b["ms_min"])
            rec["combined_spread_ms"] = round(spread, 4)
            rec["ratio_0_over_1"] = round(b["ms_median"] / a["ms_median"], 3)
            # forward: faster by more than the spread; forward + backward: not slower by more than it
            # (the backward's switch: forward + backward faster by more than it, but at the host-bound small shape)
            faster = p == "forward" if args.switch == SWITCH else name != "small"
            rec["meets"] = a["ms_median"] < (b["ms_median"] - spread if faster else b["ms_median"] + spread)
            entry["passes"][p] = rec
            print(name, p, json.dumps(rec), flush=True)
        result["shapes"][name] = entry
    return result


def errors():
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _attn_mfma_dec as C
    import _attn_ref as R

    from pydrobert_amd import _attn, switches

    dev = torch.device("cuda:0")
    out_tol = R.SUITE["float32"][0]

    def grads(fn, q, k, v, gout):
        leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad((fn(*leaves).double() * gout.to(q.device)).sum(), leaves)

    result = {}
    for name in C.CASES:
        x, ref = C.inputs(name, dev), C.reference(name)
        q, k, v, mask, dim, scale = (x[n] for n in ("q", "k", "v", "mask", "dim", "scale"))
        plan, ops = _attn._dot_plan(q, k, v, mask, dim)
        assert _attn._mfma_dec_workspace_bytes(plan, 0, ops) >= 0, name
        out = torch.ops.pydrobert_amd.dot_attention(q, k, v, mask, dim, scale)[0].cpu().double()
        live = torch.isfinite(out).all(-1).reshape(-1)  # (not the all-masked row, not the row that attends a NaN key)
        err = (out - ref["out"]).abs().reshape(live.numel(), -1)[live]
        bound = (out_tol + out_tol * ref["out"].abs()).clamp_min(8 * ref["err32"]).reshape(live.numel(), -1)[live]
        rec = {"formula_error_float32": ref["err32"], "out": round(float((err / bound).max()), 4)}
        if name in C.GRAD_CASES:
            gout = torch.from_numpy(np.random.default_rng(5).normal(size=ref["out"].shape))
            cm = None if mask is None else mask.cpu()
            fn = lambda a, b, c: _attn.dot_attention(a, b, c, mask, 0, scale)  # noqa: E731
            got = grads(fn, q, k, v, gout)
            with switches.override(**{SWITCH: 0}):
                old = grads(fn, q, k, v, gout)
            want = grads(lambda a, b, c: R.attend_ref(a, b, c, cm, 0, scale), *(t.cpu().double() for t in (q, k, v)), gout)
            for n, g, o, w in zip(("dq", "dk", "dv"), got, old, want):
                e1, e0 = (float((t.cpu().double() - w).abs().max()) for t in (g, o))
                rec[n] = {"error_switch_1": e1, "error_switch_0": e0, "ratio": round(e1 / e0, 4)}
        result[name] = rec
        print(name, json.dumps(rec), flush=True)
    return {"largest_error_over_bound_and_gradient_ratios": result}


def errors_backward():
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _attn_mfma_dec as C
    import _attn_ref as R

    from pydrobert_amd import _attn, switches

    dev = torch.device("cuda:0")
    tol = R.SUITE["float32"][1]

    def grads(fn, q, k, v, gout):
        leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        return torch.autograd.grad((fn(*leaves).double() * gout.to(q.device)).sum(), leaves)

    result = {}
    for name in ("one-block", "tails", "rising", "wide", "projection"):  # (the cases with a finite reference throughout)
        x = C.inputs(name, dev)
        q, k, v, mask, dim, scale = (x[n] for n in ("q", "k", "v", "mask", "dim", "scale"))
        plan, ops = _attn._dot_plan(q, k, v, mask, dim)
        assert _attn._mfma_dec_bwd_workspace_bytes(plan, 0, ops, ops[0]) >= 0, name
        gout = torch.from_numpy(np.random.default_rng(5).normal(size=C.reference(name)["out"].shape))
        cm = None if mask is None else mask.cpu()
        fn = lambda a, b, c: _attn.dot_attention(a, b, c, mask, dim, scale)  # noqa: E731
        got = grads(fn, q, k, v, gout)
        with switches.override(**{BWD_SWITCH: 0}):
            old = grads(fn, q, k, v, gout)
        want = grads(lambda a, b, c: R.attend_ref(a, b, c, cm, dim, scale), *(t.cpu().double() for t in (q, k, v)), gout)
        rec = {}
        for n, g, o, w in zip(("dq", "dk", "dv"), got, old, want):
            e1, e0 = ((t.cpu().double() - w).abs() for t in (g, o))
            rec[n] = {"error_over_bound": round(float((e1 / (tol + tol * w.abs())).max()), 4)}
            if name in C.GRAD_CASES:
                rec[n].update(error_switch_1=float(e1.max()), error_switch_0=float(e0.max()),
                              ratio=round(float(e1.max()) / float(e0.max()), 4))
        result[name] = rec
        print(name, json.dumps(rec), flush=True)
    return {"gradient_errors_over_bound_and_ratios_to_attn_bwd_kernel": result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--switch", default=SWITCH, choices=(SWITCH, BWD_SWITCH))
    args = ap.parse_args()
    stem = "attn_mfma_dec_bwd" if args.switch == BWD_SWITCH else "attn_mfma_dec"
    out = args.out or os.path.join(ROOT, "profiles", stem + ("_errors.json" if args.errors else "_times.json"))
    result = (errors_backward() if args.switch == BWD_SWITCH else errors()) if args.errors else measure(args)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
