#!/usr/bin/env python
"""How far torch's device softmax and log_softmax of float64 rows lie from the CPU's, by row width: the reason
GumbelOneHotCategorical.probs is ``logits.exp()`` for float64 on a device.  One JSON line.

    python profiles/tools/softmax_f64.py [--out profiles/softmax_f64.json]
"""
import argparse
import json

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device"
    gen = torch.Generator().manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "what": "max relative difference to the CPU, float64 rows of 2 randn"}
    for V in (65, 512, 1024, 1025, 1500, 4096):
        x = (2 * torch.randn((4, V), generator=gen, dtype=torch.float64)).log_softmax(-1)
        p, lp = x.softmax(-1), x.log_softmax(-1)
        pd, lpd, ed = x.cuda().softmax(-1).cpu(), x.cuda().log_softmax(-1).cpu(), x.cuda().exp().cpu()
        result["V{}".format(V)] = {
            "softmax": float(((pd - p).abs() / p).max()),
            "exp_of_normalised_logits": float(((ed - p).abs() / p).max()),
            "log_softmax_abs": float((lpd - lp).abs().max()),
        }
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
