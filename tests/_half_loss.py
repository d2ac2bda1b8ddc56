"""float16 / bfloat16 logits through the hard optimal-completion distillation loss without a float32 copy:
the sizes and helpers shared by tests/test_half_loss_cpu.py and tests/test_half_loss_gpu.py.

The contract is the one of tests/_half_logits.py, and has no tolerance in it: the loss on half ``x`` has the
bits of the float32 route's loss on ``x.float()``, the gradient -- returned in ``x.dtype`` -- those of the
float32 route's gradient cast with ``.to(x.dtype)``.
"""
from _half_logits import MIB  # noqa: F401  (the allocator's rounding both no-copy tests allow)

# "the copies are gone": 2.048 M logits, a float32 copy of them is 8 192 000 bytes
NOCOPY = dict(H=64, N=16, V=2000, R=12)


def forced_tokens(V):
    """Both sides of every register-chunk (64) and staging (512, 1024) boundary of csrc/row_reduce.hpp
    (the helper of tests/test_losses_gpu.py::test_hocd_row_forms)."""
    return sorted({t for t in (0, 63, 64, 511, 512, 1023, 1024, V - 1) if t < V})


def forward_allowance(lib, H, N, V, R):
    """Bytes ``ocd_loss_rows`` may allocate on half logits: the class bitmask, the class tokens, the three
    status words, the mask kernel's workspace, ``loss`` and ``count`` -- nothing of the logits' size."""
    W = int(lib.pdt_oc_mask_words(R))
    bitmask = H * N * W * 4
    class_tokens = N * max(R, 1) * 8
    status = 3 * 4
    workspace = int(lib.pdt_oc_mask_workspace_bytes(R, H, N))
    return bitmask + class_tokens + status + workspace + H * N * 4 + H * N * 4


def backward_allowance(H, N, V, elem_size):
    """Bytes ``ocd_loss_rows_backward`` may allocate: the gradient in the logits' type and a float32
    ``grad_loss``."""
    return H * N * V * elem_size + H * N * 4
