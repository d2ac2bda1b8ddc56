"""How often ctc_two_steady_frames applies, counted on the CPU with the oracle's step function (the model of
tests/test_ctc_twoframe_gpu.py): bench distribution (N(0, 1) + PEAK on a uniformly drawn class), T = 512,
V = 256, K = 16.   python profiles/tools/twoframe_pairs_cpu.py [utterances] [seed] [peak]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "pydrobert-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import test_ctc_twoframe_gpu as m

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
peak_add = float(sys.argv[3]) if len(sys.argv) > 3 else 12.0
T = 512
rng = np.random.default_rng(seed)
lg = rng.normal(size=(T, N, m.V + 1)).astype(np.float32)
peak = rng.integers(0, m.V + 1, (T, N, 1))
np.put_along_axis(lg, peak, np.take_along_axis(lg, peak, 2) + np.float32(peak_add), 2)
m.SHAPES["count"] = (T, N, False)
m._input.cache_clear()
_orig = m._input.__wrapped__
m._input = lambda shape, kind: lg if shape == "count" else _orig(shape, kind)
frames = m._frames_cpu.__wrapped__("count", "bench")
steady = sum("steady" in f for fr in frames for f in fr.values())
rel = sum("relation" in f for fr in frames for f in fr.values())
print("utterances %d, seed %d, peak +%g: steady frames %.2f %%, frames entered with a strict-prefix relation %.2f %%"
      % (N, seed, peak_add, 100.0 * steady / (N * T), 100.0 * rel / (N * T)))


def share(lo, hi):
    q = f = s = 0
    for fr in frames:
        for t in range(lo, hi, 2):
            ok0 = "steady" in fr.get(t, ()) and "relation" not in fr.get(t, ())
            q += m._qualifies(fr, t)
            f += ok0 and "steady" not in fr.get(t + 1, ())
            s += not ok0
    n = N * (hi - lo) // 2
    return 100.0 * q / n, 100.0 * f / n, 100.0 * s / n


for lo, hi in ((0, T), (0, 64), (64, 256), (256, T)):
    print("frames %3d-%3d: qualifying pairs %.1f %%, first steady and second not %.1f %%, first not steady (or a relation) %.1f %%"
          % ((lo, hi - 1) + share(lo, hi)))
