"""The slicing and chunking operators at the front-end shape: the HIP route against the package's torch body
run on the device (the chain of stock torch ops a user would otherwise run), and pad_variable at the same
byte count beside the two copy operators.

  python profiles/tools/time_chunk.py [--windows 15] [--calls 40] [--kernel-stats CSV] [--out JSON]
  rocprofv3 --kernel-trace --stats -d DIR -o x --output-format csv -- python profiles/tools/time_chunk.py --kernels-only

Call times: one sample is a WINDOW of --calls back-to-back calls between two events (tens of milliseconds of
work, so that one slow call does not make the spread), divided by the number of calls; windows of the two
routes alternate.  Per operation: min / median / max ms per call of each route, the spread (max - min over
the windows) of each, and whether the torch median exceeds the HIP median by more than the two spreads
combined.  The byte fraction of a call time is of the whole call (host work and read-backs included).

Kernel times come from a separate profiler run of --kernels-only (each HIP route a few times, nothing else)
whose kernel_stats.csv is given back with --kernel-stats: average ns per kernel, the bytes that kernel moves
and the fraction of the measured HBM copy rate (6.29 TB/s) it reaches.

Shapes: chunk_by_slices / pad_masked_sequence / pad_variable N=2048, T=1000, F=80 float32 (pad_masked_sequence
in both layouts); the token chunks N=2048, R=200; slice_spect_data 'ali' N=2048, T=1000, lobe_size=2."""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

from pydrobert_amd import _feats, _pad  # noqa: E402
from pydrobert_amd import functional as F  # noqa: E402

DEV = torch.device("cuda:0")
HBM_TBPS = 6.29


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def torch_chunk(x, slices, lens, mode):
    # one read-back (the largest chunk; none of the reflect / replicate checks), then the torch body
    Tp = int((slices[:, 1] - slices[:, 0]).max().item())
    return _pad._chunk_torch(x, slices, lens, mode, 0.0, Tp)


def stats3(v):
    v = sorted(v)
    return v[0], v[len(v) // 2], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    N, T, Fd, R = 2048, 1000, 80, 200
    x = torch.randn(N, T, Fd, device=DEV)
    xt = x.transpose(0, 1).contiguous()  # time-major
    lens = torch.randint(T // 2, T + 1, (N,), device=DEV)
    # chunks of 400 steps, up to 100 of them before the start or beyond the end of the row
    start = (torch.rand(N, device=DEV) * (lens - 200)).long() - 100
    slices = torch.stack([start, start + 400], 1)
    chunk_bytes = 2 * 4 * N * 400 * Fd
    mask = torch.rand(N, T, device=DEV) < 0.8
    mask_t = mask.t().contiguous()
    kept = int(mask.sum())
    gather_bytes = 4 * Fd * (kept + N * T) + 4 * N * T  # payload read and written, the int32 map read
    compact_bytes = N * T * (1 + 4)  # the mask read, the map written
    # pad_variable moving the chunk operator's bytes: 380 steps in, 10 + 380 + 10 out
    pv_lens = torch.full((N,), 380, device=DEV)
    pv_pad = torch.full((2, N), 10, device=DEV)
    pv_bytes = 4 * N * Fd * (380 + 400)
    rs = torch.randint(0, T, (N, R), device=DEV)
    refs = torch.stack([torch.randint(0, 50, (N, R), device=DEV), rs, rs + torch.randint(0, 40, (N, R), device=DEV)], 2)
    ref_lens = torch.randint(R // 2, R + 1, (N,), device=DEV)
    tok_bytes = 8 * 3 * N * R * 2
    ali = torch.randint(0, 40, (N, 1), device=DEV) + torch.arange(T, device=DEV) // 8  # runs of 8 equal labels
    n_slices = F.slice_spect_data(ali, lens, None, "ali", "symmetric", True, 2)[1].numel()
    ali_bytes = 8 * N * T + 8 * 3 * n_slices
    work = {
        "chunk_by_slices_constant": (lambda: F.chunk_by_slices(x, slices, lens), lambda: torch_chunk(x, slices, lens, "constant"), chunk_bytes),
        "chunk_by_slices_reflect": (lambda: F.chunk_by_slices(x, slices, lens, "reflect"), lambda: torch_chunk(x, slices, lens, "reflect"), chunk_bytes),
        "chunk_by_slices_replicate": (lambda: F.chunk_by_slices(x, slices, lens, "replicate"), lambda: torch_chunk(x, slices, lens, "replicate"), chunk_bytes),
        "pad_variable_reflect": (lambda: F.pad_variable(x, pv_lens, pv_pad, "reflect"), None, pv_bytes),
        "pad_masked_sequence": (lambda: F.pad_masked_sequence(x, mask, True), lambda: _pad._pad_masked_torch(x, mask, True, 0.0), gather_bytes + compact_bytes),
        "pad_masked_sequence_time_major": (lambda: F.pad_masked_sequence(xt, mask_t), lambda: _pad._pad_masked_torch(xt, mask_t, False, 0.0), gather_bytes + compact_bytes),
        "chunk_token_sequences": (lambda: F.chunk_token_sequences_by_slices(refs, slices, ref_lens, True), lambda: _feats._chunk_tokens_torch(refs, slices, ref_lens, True, False), tok_bytes),
        "slice_spect_data_ali": (lambda: F.slice_spect_data(ali, lens, None, "ali", "symmetric", True, 2), lambda: _feats._slice_spect_torch(ali, lens, None, "ali", "symmetric", True, 2), ali_bytes),
    }  # fmt: skip
    if args.kernels_only:
        for name, (hip, _, _) in work.items():
            if name == "pad_masked_sequence_time_major":
                continue  # (its kernels carry the same names: profiled by the call times only)
            for _ in range(5):
                hip()
        torch.cuda.synchronize()
        return
    results = []
    for name, (hip, ref, nb) in work.items():
        for _ in range(3):
            hip()
            if ref is not None:
                ref()
        torch.cuda.synchronize()
        th, tr = [], []
        for _ in range(args.windows):
            th.append(window(hip, args.calls))
            if ref is not None:
                tr.append(window(ref, args.calls))
        h = stats3(th)
        row = {"op": name, "windows": args.windows, "calls_per_window": args.calls, "hip_ms_min": round(h[0], 4),
               "hip_ms_median": round(h[1], 4), "hip_ms_max": round(h[2], 4), "MB": round(nb / 1e6, 2),
               "hip_call_TBps": round(nb / h[1] / 1e9, 3),
               "hip_call_fraction_of_hbm": round(nb / h[1] / 1e9 / HBM_TBPS, 3)}  # fmt: skip
        if tr:
            t = stats3(tr)
            spread = (h[2] - h[0]) + (t[2] - t[0])
            row.update({"torch_ms_min": round(t[0], 4), "torch_ms_median": round(t[1], 4), "torch_ms_max": round(t[2], 4),
                        "combined_spread_ms": round(spread, 4), "median_gain_ms": round(t[1] - h[1], 4),
                        "hip_beats_torch_beyond_spread": bool(t[1] - h[1] > spread)})  # fmt: skip
        results.append(row)
        print(json.dumps(row))
    kernels = []
    if args.kernel_stats:
        moved = {"SliceSrc": chunk_bytes, "MapSrc": gather_bytes, "MaskPolicy": compact_bytes,
                 "pad_variable_kernel": pv_bytes, "TokenPolicy": tok_bytes, "AliPolicy": 8 * N * T + 4 * N * T // 8,
                 "ali_emit_kernel": 8 * 3 * n_slices + 4 * N * T // 8, "chunk_stats_kernel": 8 * 4 * N}  # fmt: skip
        with open(args.kernel_stats) as f:
            for rec in csv.DictReader(f):
                for key, nb in moved.items():
                    if key in rec["Name"]:
                        avg = float(rec["AverageNs"])
                        row = {"kernel": rec["Name"], "calls": int(rec["Calls"]), "avg_us": round(avg / 1e3, 2),
                               "min_us": round(float(rec["MinNs"]) / 1e3, 2), "max_us": round(float(rec["MaxNs"]) / 1e3, 2),
                               "MB": round(nb / 1e6, 2), "fraction_of_hbm": round(nb / avg / 1e3 / HBM_TBPS, 3)}  # fmt: skip
                        kernels.append(row)
                        print(json.dumps(row))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "hbm_TBps": HBM_TBPS, "calls": results,
                       "kernels": kernels}, f, indent=1)  # fmt: skip


if __name__ == "__main__":
    main()
