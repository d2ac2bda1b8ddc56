"""RandomWalk: the loop of the previous release (torch ops, multinomial, a host read per iteration) against
the HIP routes, in one process on the same seed, runs alternated.

  python profiles/tools/time_random_walk.py [--reps 5]

Workloads:
  bigram  LookupLanguageModel, V = 1000, N = 4096, eos probability ~1/32, max_iters=None: the table route
          (pdt_random_walk_table) and the per-iteration route (PDT_WALK_TABLE=0)
  trigram LookupLanguageModel, V = 5000, N = 1024, same eos rate: its context table is far above 64 MiB,
          so the per-iteration route (the model's scoring kernel + pydrobert_amd::random_walk_step)
Prints one JSON line per workload with the min / median / max of each route's wall time (ms), the mean
length, and for the table route the modelled bytes read per token (row statistics, the 64-token chunks
the scan reads -- one chunk ahead -- and the token written)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

from pydrobert_amd import modules as M  # noqa: E402
from pydrobert_amd import switches  # noqa: E402

DEV = torch.device("cuda:0")


def previous_walk(lm, eos, N, max_iters=1 << 30):
    """The previous release's RandomWalk.forward and random_walk_advance on a ROCm device (stock torch ops)."""
    y = torch.empty((0, N), device=DEV, dtype=torch.long)
    prev = lm.update_input(dict(), y)
    y_lens = torch.zeros(N, dtype=torch.long, device=DEV)
    eos_mask = torch.zeros(N, device=DEV, dtype=torch.bool)
    log_probs = torch.zeros(N, device=DEV)
    for t in range(max_iters):
        if bool(eos_mask.all()):
            break
        lp_t, prev = lm.calc_idx_log_probs(y[:t], prev, torch.tensor(t, device=DEV))
        lp_t = lp_t.log_softmax(-1)
        lp_t = lp_t.masked_fill(eos_mask.unsqueeze(1), -float("inf"))
        lp_t[:, eos] = lp_t[:, eos].masked_fill(eos_mask, 0.0)
        y_t = torch.multinomial(lp_t.exp(), 1, True)
        log_probs = log_probs + lp_t.gather(1, y_t).squeeze(1)
        y_t = y_t.T
        if t:
            y_next = torch.cat([y, y_t], 0) if int(y_lens.max().item()) >= y.size(0) else y
            y = y_next.scatter(0, y_lens.unsqueeze(0), y_t)
        else:
            y = y_t
        y_lens = y_lens + (~eos_mask).long()
        eos_mask = y.gather(0, y_lens.unsqueeze(0) - 1).squeeze(0) == eos
    return y, y_lens, log_probs


def make_lm(V, order, eos, seed):
    """Every unigram, 16 random successors per context at each higher order; eos's unigram weight set so that
    about 1 token in 32 is eos."""
    rng = np.random.default_rng(seed)
    uni = {v: (float(rng.normal()), float(rng.normal() * 0.1)) for v in range(V)}
    uni[eos] = (float(np.log(V / 19.0)), 0.0)
    uni[V] = (-99.0, 0.0)  # (the start-of-sequence token, outside the vocabulary)
    dicts = [uni]
    for n in range(2, order + 1):
        d = {}
        for _ in range(16 * V):
            key = tuple(int(x) for x in rng.integers(0, V, n))
            if key[-1] != eos:
                d[key] = float(rng.normal()) if n == order else (float(rng.normal()), float(rng.normal() * 0.1))
        dicts.append(d)
    return M.LookupLanguageModel(V, V, dicts).to(DEV)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def table_bytes_per_token(y, lens, V):
    """Bytes the table kernel reads and writes per token of a live walk: 8 (row statistics) + 256 per chunk
    scanned (the token's chunk and those before it, plus the one loaded ahead) + 8 (the token)."""
    T = y.size(0)
    live = torch.arange(T, device=y.device).unsqueeze(1) < lens.unsqueeze(0)
    n_chunks = (V + 63) // 64
    chunks = torch.clamp(y // 64 + 2, max=n_chunks)
    tokens = int(live.sum())
    return float((8 + 256 * chunks.double() + 8)[live].sum()) / max(tokens, 1), tokens


def run(name, lm, N, reps, routes):
    V, eos = lm.vocab_size, 1
    walk = M.RandomWalk(lm, eos=eos).to(DEV)
    times = {r: [] for r in ["previous"] + list(routes)}
    info = {}
    for rep in range(reps + 1):  # (rep 0: warm-up -- tables built, kernels loaded)
        for r in times:
            torch.manual_seed(100 + rep)
            if r == "previous":
                ms, out = timed(lambda: previous_walk(lm, eos, N))
            else:
                with switches.override(PDT_WALK_TABLE=1 if r == "table" else 0):
                    ms, out = timed(lambda: walk(None, N))
            if rep:
                times[r].append(ms)
            y, lens, _ = out
            info.setdefault(r + "_mean_len", float(lens.double().mean()))
            info.setdefault(r + "_T", int(y.size(0)))
            if r == "table" and "table_bytes_per_token" not in info:
                bpt, toks = table_bytes_per_token(y, lens, V)
                info["table_bytes_per_token"] = round(bpt, 1)
                info["table_tokens"] = toks
    rec = {"workload": name, "V": V, "N": N, "reps": reps}
    for r, ts in times.items():
        rec[r + "_ms"] = [round(min(ts), 3), round(float(np.median(ts)), 3), round(max(ts), 3)]
    for r in routes:
        rec["speedup_" + r] = round(float(np.median(times["previous"])) / float(np.median(times[r])), 1)
    rec.update(info)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    run("bigram", make_lm(1000, 2, 1, 0), 4096, args.reps, ("table", "per_iteration"))
    run("trigram", make_lm(5000, 3, 1, 1), 1024, args.reps, ("per_iteration",))


if __name__ == "__main__":
    main()
