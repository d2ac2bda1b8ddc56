"""feat_deltas, mean_var_norm and MeanVarianceNormalization.accumulate at the C4 shape: the HIP path against
the same math as stock torch ops on the device (the package's CPU body run on device tensors), runs alternated
in pairs and timed with events.

  python profiles/tools/time_feats.py [--reps 10]

Prints one JSON line per operation: min / median ms of each route and the achieved TB/s of algorithmic bytes
(deltas 4*N*T*F*(1 + U); normalisation with computed statistics three passes, with given ones two;
accumulate one read)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pydrobert-pytorch_amd"))

from pydrobert_amd import _feats  # noqa: E402
from pydrobert_amd import functional as F  # noqa: E402
from pydrobert_amd import modules as M  # noqa: E402

DEV = torch.device("cuda:0")


def torch_deltas(x):
    f = _feats._feat_delta_filters(2, 2).to(DEV)
    return _feats._feat_deltas_torch(x, f, 1, 2, True, 2, 2, "replicate", 0.0)


def torch_mvn(x, mean=None, std=None):
    X = x.shape[-1]
    xd = x.reshape(-1, X)
    if mean is None:
        mean = xd.double().mean(0)
    c = x - mean.to(x.dtype)
    if std is None:
        cd = c.reshape(-1, X).double()
        std = (cd - cd.mean(0)).square().mean(0).sqrt()
    return c / std.to(x.dtype).clamp_min(1.1754943508222875e-38)


def torch_accumulate(x, count, sum_, sumsq):
    xd = x.reshape(-1, x.shape[-1]).double()
    count += xd.shape[0]
    sum_ += xd.sum(0)
    sumsq += xd.square().sum(0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    N, T, Fd = 2048, 1000, 80
    x = torch.randn(N, T, Fd, device=DEV)
    nbytes = 4 * N * T * Fd
    mean = x.reshape(-1, Fd).double().mean(0)
    std = x.reshape(-1, Fd).double().std(0, unbiased=False)
    m = M.MeanVarianceNormalization()
    m.accumulate(x)
    cnt, s1, s2 = torch.zeros(1, device=DEV, dtype=torch.double), torch.zeros(Fd, device=DEV, dtype=torch.double), \
        torch.zeros(Fd, device=DEV, dtype=torch.double)  # fmt: skip
    work = {
        "deltas_order2": (lambda: F.feat_deltas(x), lambda: torch_deltas(x), nbytes * 4),
        "mvn_computed": (lambda: F.mean_var_norm(x), lambda: torch_mvn(x), nbytes * 3),
        "mvn_given": (lambda: F.mean_var_norm(x, -1, mean, std), lambda: torch_mvn(x, mean, std), nbytes * 2),
        "accumulate": (lambda: m.accumulate(x), lambda: torch_accumulate(x, cnt, s1, s2), nbytes),
    }
    for name, (hip, ref, nb) in work.items():
        for _ in range(2):
            hip(), ref()
        th, tr = [], []
        for _ in range(args.reps):
            th.append(timed(hip))
            tr.append(timed(ref))
        th.sort()
        tr.sort()
        print(json.dumps({
            "op": name, "hip_ms_min": round(th[0], 4), "hip_ms_median": round(th[len(th) // 2], 4),
            "torch_ms_min": round(tr[0], 4), "torch_ms_median": round(tr[len(tr) // 2], 4),
            "hip_TBps": round(nb / th[len(th) // 2] / 1e9, 3), "torch_TBps": round(nb / tr[len(tr) // 2] / 1e9, 3),
            "GB": round(nb / 1e9, 3),
        }))  # fmt: skip


if __name__ == "__main__":
    main()
