"""Who ends the headline launch: per-utterance end time of the consumer loop and count of frames with a rounded tie
among the best K + 1 (-DPDT_UTT_STATS -DPDT_UTT_REASONS build of ctc_search.hip under PDT_AMD_LIB) on the bench's own
logits and the four draws of C2_ctc_prefix_search_other_draws (profiles/r12_utt_stats.json).
python profiles/tools/utt_ties.py TAG OUT.json [PARENT.json]   (PARENT.json: a run of another build -- the end times
here of the utterances that had 20 or more tie frames there)"""
import os, sys, json, ctypes, numpy as np, torch
sys.path.insert(0, "."); sys.path.insert(0, "pydrobert-pytorch_amd")
import bench
from pydrobert_amd import functional as F
dev = torch.device("cuda:0")
T, N, V, K = 512, 4096, 256, 16
L = ctypes.CDLL(os.environ["PDT_AMD_LIB"])
L.pdt_debug_read_utt_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
tag, out_path = sys.argv[1], sys.argv[2]
parent_path = sys.argv[3] if len(sys.argv) > 3 else None
out = {}
draws = [("bench: seed 0x5EED0003 in 512-frame chunks", 0x5EED0003, 512), ("seed 3 in 64-frame chunks", 3, 64),
         ("seed 3 in 512-frame chunks", 3, 512), ("seed 4 in 64-frame chunks", 4, 64), ("seed 4 in 512-frame chunks", 4, 512)]
for name, seed, chunk in draws:
    lg = bench.peaky_logits(T, N, V, dev, seed, chunk=chunk)
    buf = np.zeros((N, 4), dtype=np.uint32)
    F.ctc_prefix_search(lg, K); torch.cuda.synchronize()
    L.pdt_debug_read_utt_stats(buf.ctypes.data, N, 1)
    F.ctc_prefix_search(lg, K); torch.cuda.synchronize()
    L.pdt_debug_read_utt_stats(buf.ctypes.data, N, 1)
    ms = bench.event_ms(lambda: F.ctc_prefix_search(lg, K), reps=5, warm=1)
    end = buf[:, 0].astype(np.float64) * 16 / 1e6  # Mcycles of the shader clock since the wave started
    exits, ties, zties = buf[:, 1].astype(int), buf[:, 2].astype(int), buf[:, 3].astype(int)
    med = float(np.median(end))
    order = np.argsort(-end)
    last = order[:16]
    tie_class = ties >= 20
    rec = {
        "launch_ms_diagnostic_build": ms,
        "loop_end_mcycles": {"median": med, "p90": float(np.percentile(end, 90)), "p99": float(np.percentile(end, 99)), "max": float(end.max())},
        "tie_frames_per_utterance": {"median": float(np.median(ties)), "p90": float(np.percentile(ties, 90)), "p99": float(np.percentile(ties, 99)), "max": int(ties.max())},
        "lean_exits_per_utterance": {"median": float(np.median(exits)), "p99": float(np.percentile(exits, 99)), "max": int(exits.max())},
        "utterances_with_20_or_more_tie_frames": int(tie_class.sum()),
        "their_loop_end_minus_median_mcycles": sorted((round(float(x - med), 4) for x in end[tie_class]), reverse=True),
        "those_utterances": [int(i) for i in np.where(tie_class)[0]],
        "rank_by_end_time_of_those": sorted(int(np.where(order == i)[0][0]) for i in np.where(tie_class)[0]),
        "last_16_utterances": [{"n": int(i), "end_minus_median_mcycles": round(float(end[i] - med), 4), "tie_frames": int(ties[i]),
                                "underflow_tie_frames": int(zties[i]), "lean_exits": int(exits[i])} for i in last],
        "corr_end_tie_frames": float(np.corrcoef(end, ties)[0, 1]),
        "corr_end_lean_exits": float(np.corrcoef(end, exits)[0, 1]),
    }
    if parent_path:
        par = json.load(open(parent_path))[name]
        idx = par["those_utterances"]
        rec["parents_tie_class_utterances"] = idx
        rec["their_loop_end_minus_median_mcycles_here"] = [round(float(end[i] - med), 4) for i in idx]
        rec["their_rank_by_end_time_here"] = [int(np.where(order == i)[0][0]) for i in idx]
    out[name] = rec
    print(tag, name, "launch %.3f ms | end median %.3f max %.3f | ties max %d, >=20: %d | last 4:" % (ms, med, end.max(), ties.max(), tie_class.sum()),
          [(r["end_minus_median_mcycles"], r["tie_frames"], r["lean_exits"]) for r in rec["last_16_utterances"][:4]], flush=True)
    del lg
json.dump(out, open(out_path, "w"), indent=1)
