"""How often the one-launch wide CTC search (csrc/ctc_search_wide.hip) reads a token off the trie in its
next-token update, on the hand-built input of tests/test_ctc_wide_search_gpu.py (a re-created
intermediate prefix) and on random peaky logits.  Needs the diagnostic build:

    PDT_AMD_LIB=$(profiles/tools/build_var.sh walks ctc_search_wide.hip -DPDT_WIDE_WALKS) \\
        python profiles/tools/count_wide_walks.py
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "pydrobert-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_ctc_wide_search_gpu as cases  # noqa: E402
from pydrobert_amd import _cabi  # noqa: E402
from pydrobert_amd import functional as F  # noqa: E402


def walks(lg, K):
    L = _cabi.lib()
    n = ctypes.c_ulonglong(0)
    assert L.pdt_debug_read_wide_walks(ctypes.byref(n), 1) == 0
    F.ctc_prefix_search(torch.from_numpy(lg).to("cuda:0"), K)
    torch.cuda.synchronize()
    assert L.pdt_debug_read_wide_walks(ctypes.byref(n), 1) == 0
    return n.value


lg = cases._recreated_prefix_logits()
print("hand-built input, width 33: CPU replay says frames", cases._frames_that_walk(lg, 33), "-- kernel walks:", walks(lg, 33))
rng = np.random.default_rng(0)
for T, N, V, K in [(70, 5, 127, 128), (33, 4, 64, 64)]:
    print("random peaky logits", (T, N, V, K), "-- kernel walks:", walks(cases._peaky_logits(rng, T, N, V, 8.0), K))
