"""Which frames of the headline CTC search miss the steady tier, per utterance (CPU only: numpy and the oracle).

python profiles/tools/steady_ties_cpu.py [utterances = 512] [seed = 11] [--json]

Draws the bench's distribution with numpy (N(0, 1) + 12 on a uniformly drawn class per frame, blank included;
T = 512, V = 256, K = 16), runs the oracle's ctc_prefix_search_advance frame by frame and counts, per
utterance: STEADY frames -- full beam, next_src == arange(K), no winner a non-extension, the new masses in
strictly descending 64-ulp buckets of the lean tier's rounded sort (what tests/test_ctc_steady_gpu.py's
_steady_frames_cpu counts) -- and TIE-LOST frames, which meet all of that except the strict buckets: two
neighbouring masses share a bucket.  A launch ends with its slowest utterance, so the table is about the
largest counts, not the means.  About three minutes for 512 utterances on one core."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import oracle  # noqa: E402

T, V, K = 512, 256, 16


def bucket(mass):
    key = np.asarray(mass, np.float32).view(np.uint32).astype(np.int64) + 1
    return (key + 63) >> 6


def count(N, seed):
    rng = np.random.default_rng(seed)
    nb, b = np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)
    y = np.zeros((0, N, 1), np.int64)
    y_last = y_lens = np.zeros((N, 1), np.int64)
    isp = np.ones((N, 1, 1), bool)
    steady, tie_lost = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(T):
        lg = rng.normal(size=(N, V + 1)).astype(np.float32)
        peak = rng.integers(0, V + 1, (N, 1))
        np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 1) + np.float32(12.0), 1)
        e = np.exp(lg - lg.max(1, keepdims=True))
        probs = (e / e.sum(1, keepdims=True)).astype(np.float32)
        nonext, blank = np.ascontiguousarray(probs[:, :V]), np.ascontiguousarray(probs[:, V])
        Kp = nb.shape[1]
        ext = np.ascontiguousarray(np.broadcast_to(nonext[:, None, :], (N, Kp, V)))
        full = (Kp == K) & ((nb + b) > 0).all(1)
        y, y_last, y_lens, (nb, b), isp, src, kept = oracle.ctc_prefix_search_advance(
            (ext, nonext, blank), K, (nb, b), y, y_last, y_lens, isp
        )
        bk = bucket(nb + b)
        in_place = full & (src == np.arange(K)[None]).all(1) & ~kept.any(1)
        strict = (bk[:, :-1] > bk[:, 1:]).all(1)
        steady += in_place & strict
        tie_lost += in_place & ~strict
    return steady, tie_lost


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    N = int(args[0]) if args else 512
    seed = int(args[1]) if len(args) > 1 else 11
    steady, tie_lost = count(N, seed)
    non = T - steady
    top = np.argsort(-non)[:5]
    rec = {
        "seed": seed,
        "utterances": N,
        "frames": T,
        "non_steady_median": float(np.median(non)),
        "non_steady_p90": float(np.percentile(non, 90)),
        "non_steady_max": int(non.max()),
        "tie_lost_max": int(tie_lost.max()),
        "utterances_with_20_or_more_tie_lost": int((tie_lost >= 20).sum()),
        "top5_non_steady": [int(non[i]) for i in top],
        "top5_their_tie_lost": [int(tie_lost[i]) for i in top],
        "steady_share": float(steady.sum() / (N * T)),
    }
    if "--json" in sys.argv:
        print(json.dumps(rec))
        return
    print("seed %d, %d utterances of %d frames (steady share %.4f)" % (seed, N, T, rec["steady_share"]))
    print("| per utterance, of %d frames | value |\n|---|---|" % T)
    print("| non-steady frames, median / p90 | %g / %g |" % (rec["non_steady_median"], rec["non_steady_p90"]))
    print("| non-steady frames, largest | %d |" % rec["non_steady_max"])
    print("| tie-lost frames, largest | %d |" % rec["tie_lost_max"])
    print("| utterances with >= 20 tie-lost frames | %d of %d |" % (rec["utterances_with_20_or_more_tie_lost"], N))
    print("| five largest non-steady counts (their tie-lost frames) | %s |"
          % " / ".join("%d (%d)" % p for p in zip(rec["top5_non_steady"], rec["top5_their_tie_lost"])))


if __name__ == "__main__":
    main()
