"""Where the headline launch's tail comes from: per-utterance end time of the consumer loop (-DPDT_UTT_STATS build) by
workgroup position.  PDT_AMD_LIB=.../variants/utt/lib.so python profiles/tools/utt_balance.py [--json FILE [--label TEXT]]
(--json: the table by dispatch-position eighth and the launch's time, as a record; --label: what the record calls the
library, in place of its path)"""
import os, sys, ctypes, json, numpy as np, torch
sys.path.insert(0, "."); sys.path.insert(0, "pydrobert-pytorch_amd")
import bench
from pydrobert_amd import functional as F
json_out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
label = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else None
dev = torch.device("cuda:0")
T, N, V, K = 512, 4096, 256, 16
L = ctypes.CDLL(os.environ["PDT_AMD_LIB"])
L.pdt_debug_read_utt_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
lg = bench.peaky_logits(T, N, V, dev, 0x5EED0003, chunk=T)
buf = np.zeros((N, 4), dtype=np.uint32)
ms = []
for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); F.ctc_prefix_search(lg, K); e1.record(); torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
    L.pdt_debug_read_utt_stats(buf.ctypes.data, N, 1)
end = buf[:, 0].astype(np.float64); wait = buf[:, 3].astype(np.float64)
print("end: min %.0f p10 %.0f p50 %.0f p90 %.0f p99 %.0f max %.0f (x16 cycles)" % (end.min(), *np.percentile(end, [10, 50, 90, 99]), end.max()))
print("wait share of the loop: p10 %.2f p50 %.2f p90 %.2f" % tuple(np.percentile(wait / end, [10, 50, 90])))
wg = np.arange(N) // 2
# the kernel maps workgroup b -> utterances through xcd_remap: utterance pair index = remapped b; XCD of the hosting workgroup = b % 8
nwg = N // 2; q = nwg // 8
xcd = wg // q  # (nwg divisible by 8: contiguous ranges per XCD)
for x in range(8):
    m = xcd == x
    print("  XCD %d: end p50 %.0f p99 %.0f max %.0f" % (x, np.median(end[m]), np.percentile(end[m], 99), end[m].max()))
# position inside the XCD's range (dispatch order)
pos = wg % q
eighths = []
for lo in range(0, q, q // 8):
    m = (pos >= lo) & (pos < lo + q // 8)
    print("  dispatch position %4d..%4d: end p50 %.0f max %.0f, wait share p50 %.2f" % (lo, lo + q // 8 - 1, np.median(end[m]), end[m].max(), np.median(wait[m] / end[m])))
    eighths.append({"positions": [lo, lo + q // 8 - 1], "end_p50_x16cycles": float(np.median(end[m])), "end_max_x16cycles": float(end[m].max()),
                    "wait_share_p50": round(float(np.median(wait[m] / end[m])), 4)})
print("  pair partner difference |end0 - end1| p50 %.0f p99 %.0f" % tuple(np.percentile(np.abs(end[0::2] - end[1::2]), [50, 99])))
print("launch ms (diagnostic build, last of three): %.4f" % ms[-1])
if json_out:
    rec = {"tool": "profiles/tools/utt_balance.py", "library": label or os.environ["PDT_AMD_LIB"], "shape": {"T": T, "N": N, "V": V, "K": K},
           "launch": "last of three", "ms": round(ms[-1], 4), "ms_all": [round(x, 4) for x in ms],
           "end_p50_x16cycles": float(np.median(end)), "end_max_x16cycles": float(end.max()),
           "last_eighth_over_first_end_p50": round(eighths[-1]["end_p50_x16cycles"] / eighths[0]["end_p50_x16cycles"], 4),
           "by_dispatch_eighth": eighths}
    with open(json_out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
