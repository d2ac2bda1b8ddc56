"""Shared by the CPU (oracle) and GPU (kernels) suites: the hard optimal-completion distillation loss in
SET FORM, as a torch float64 graph -- so ``torch.autograd.grad`` gives the reference gradient under any
upstream weight -- without the ``(H, N, C, V)`` logit expansion of the reference's cross-entropy call.

Per prefix row, with ``M[v]`` the number of times class v is a target of the row:
    count = sum_v M[v],    loss = - sum_v M[v] w[v] log_softmax(x)[v] / max(count, 1).
``tests/test_oracle_golden.py`` pins this against ``oracle.hard_optimal_completion_distillation_loss``."""
import numpy as np
import torch

import oracle

# loss and gradient tolerances of the suite (rtol, atol): tests/test_losses_gpu.py for rows of at most
# 1024 classes, test_sequence_ops_row_forms (tests/test_seqops_gpu.py) for longer ones
LOSS_TOL = (1e-5, 1e-6)
LOSS_TOL_WIDE = (2e-5, 1e-4)
GRAD_TOL = (1e-4, 1e-5)


def loss_tol(V):
    return LOSS_TOL if V <= 1024 else LOSS_TOL_WIDE


def multiplicity(targets, V, ignore_index):
    """``targets``: ``(A, B, C)`` int64 as ``oracle.optimal_completion(..., padding=ignore_index)`` returns
    it.  ``(A, B, V)`` float64: how often each class is a target; entries equal to ``ignore_index`` (the
    padding, and a class of that value) are skipped."""
    t = torch.as_tensor(np.ascontiguousarray(targets))
    keep = t != ignore_index
    assert bool(((t >= 0) & (t < V))[keep].all())
    M = torch.zeros(tuple(t.shape[:2]) + (V,), dtype=torch.float64)
    if t.shape[2]:
        M.scatter_add_(2, t.masked_fill(~keep, 0), keep.double())
    return M


def oracle_multiplicity(ref, hyp, V, eos=None, include_eos=True, batch_first=False, ignore_index=-2):
    """(M, targets): the multiplicities of the oracle's completion sets, in the layout of ``hyp``."""
    tgt = oracle.optimal_completion(ref, hyp, eos=eos, include_eos=include_eos, batch_first=batch_first,
                                    padding=ignore_index, exclude_last=True)  # fmt: skip
    return multiplicity(tgt, V, ignore_index), tgt


def prefix_set_multiplicity(ref, H, V):
    """``(H, 1, V)`` float64 with row h the set ``{ref[0..h]}``: the completion sets of one utterance whose
    reference tokens are distinct and whose hypothesis is H copies of a token outside the reference (every
    edit is then a substitution or an insertion, and prefix h is completed best by any of ref[0..h])."""
    r = torch.as_tensor(np.ascontiguousarray(ref))[:H]
    assert r.numel() == H and r.unique().numel() == H
    first = torch.full((V,), H, dtype=torch.long)  # position in ref; H: not among the first H tokens
    first[r] = torch.arange(H)
    return (first.unsqueeze(0) <= torch.arange(H).unsqueeze(1)).double().unsqueeze(1)


def set_loss(x64, M, weight=None):
    """(loss, count), each ``M.shape[:2]``, float64, differentiable in ``x64`` (any strides).  A class outside
    the set contributes nothing even where its logit is -inf."""
    w = 1.0 if weight is None else torch.as_tensor(weight).to(x64.device, torch.float64)
    M = M.to(x64.device)
    count = M.sum(-1)
    terms = torch.where(M > 0, M * w * x64.log_softmax(-1), torch.zeros((), dtype=x64.dtype, device=x64.device))
    return -terms.sum(-1) / count.clamp_min(1), count


def reduce(loss, count, reduction, batch_first=False):
    """The reference's reductions (its _string.py:1243-1249) of a ``"none"`` loss."""
    if reduction == "sum":
        return loss.sum()
    if reduction == "mean":
        sd = 1 if batch_first else 0
        return (loss.sum(sd) / (count > 0).sum(sd).clamp_min(1)).mean()
    return loss


def close(act, exp, tol):
    """|act - exp| <= atol + rtol |exp| everywhere (the form of numpy's allclose), in float64; returns the
    largest excess ratio for the assertion message as well."""
    act, exp = torch.as_tensor(act).detach().double().cpu(), torch.as_tensor(exp).detach().double().cpu()
    if act.shape != exp.shape:
        return False, float("inf")
    if act.numel() == 0:
        return True, 0.0
    ratio = ((act - exp).abs() / (tol[1] + tol[0] * exp.abs())).nan_to_num(nan=float("inf"))
    return bool((ratio <= 1.0).all()), float(ratio.max())
