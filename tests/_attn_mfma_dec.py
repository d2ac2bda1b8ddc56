"""Shared by tests/test_attn_mfma_dec_cpu.py and tests/test_attn_mfma_dec_gpu.py: the cases of the float32 decode
attention forward (csrc/attn_mfma_dec.hip), their inputs and the float64 reference on the same numbers.  Layout as in
tests/_attn_mfma.py (dim 0 the attended axis; query (G, M, D), key (T, G, 1, D), value (T, G, 1, Dv), mask (T, G, M)),
but for "projection": batch first, query (G, D), key and value (G, T, D), all three slices of one tensor."""
import functools

import numpy as np
import torch

import _attn_ref as R
from _attn_mfma import desc  # noqa: F401

# name -> shape and the spans of T the plan must give (512 workgroups wanted, spans of whole 64-frame blocks)
CASES = {
    "one-block": dict(G=2, M=16, T=64, D=64, Dv=64, splits=1),
    "tails": dict(G=3, M=1, T=70, D=64, Dv=80, splits=2),  # fifteen padded columns, a frame tail of 6
    "rising": dict(G=520, M=2, T=130, D=64, Dv=64, splits=1),  # the unsplit walk over three blocks
    "falling": dict(G=520, M=2, T=130, D=64, Dv=64, splits=1),
    "wide": dict(G=3, M=8, T=200, D=512, Dv=512, splits=4),  # lengths 200, 130 and 1
    "empty-span": dict(G=2, M=4, T=192, D=64, Dv=64, splits=3),  # DEAD attends nothing, others not frames 64 .. 127
    "nonfinite": dict(G=2, M=9, T=64, D=80, Dv=112, splits=1),  # frame BAD of group 0: attended by row 0 alone
    "projection": dict(G=5, M=1, T=96, D=64, Dv=64, splits=2),
}
GRAD_CASES = ("wide", "rising")  # split and unsplit
DEAD, BAD, LENGTHS = (1, 2), 5, (200, 130, 1)


def plan(lib, d):
    import ctypes

    p = (ctypes.c_int64 * 7)()
    return lib.pdt_attn_dot_mfma_dec_plan(d, ctypes.addressof(p)), list(p)


def inputs(name, device="cpu"):
    """``q``, ``k``, ``v``, ``mask``, ``dim``, ``scale`` on ``device``.  Key and value are views of longer buffers
    with NaN behind frame T; ``k_ref`` / ``v_ref`` are what the reference reads ("nonfinite": without the bad frame)."""
    c = CASES[name]
    G, M, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    rng = np.random.default_rng(list(CASES).index(name))
    f = lambda *s: torch.from_numpy(rng.normal(size=s)).float()  # noqa: E731
    if name == "projection":
        p = f(G, T, 3 * D).to(device)
        q, k, v = p[:, 0, :D], p[..., D:2 * D], p[..., 2 * D:]
        return dict(q=q, k=k, v=v, k_ref=k, v_ref=v, mask=None, dim=1, scale=0.25)
    q, k, v = f(G, M, D), f(T + 2, G, 1, D), f(T + 2, G, 1, Dv)
    k[T:], v[T:] = float("nan"), float("nan")
    if name in ("rising", "falling"):  # the running maximum moves in every block, or only in the first
        q[..., 0] = 2.0
        k[:T, ..., 0] = (12.0 if name == "rising" else -12.0) * torch.arange(T).view(T, 1, 1) / T
    t = torch.arange(T).view(T, 1, 1)
    mask = None
    if name == "wide":
        mask = (t < torch.tensor(LENGTHS).view(1, G, 1)).expand(T, G, M).clone()
    if name == "empty-span":
        mask = torch.from_numpy(R.make_mask("random", rng, T, G, M))
        mask[64:128, 0], mask[64:128, 1, 0] = False, False
        mask[(slice(None),) + DEAD] = False
    if name == "nonfinite":
        mask = torch.ones(T, G, M, dtype=torch.bool)
        mask[BAD, 0, 1:] = False
        k[BAD, 0], v[BAD, 0] = float("nan"), float("inf")
    q, k, v = q.to(device), k.to(device)[:T], v.to(device)[:T]
    x = dict(q=q, k=k, v=v, k_ref=k, v_ref=v, mask=None if mask is None else mask.to(device), dim=0, scale=0.25)
    if name == "nonfinite":
        x["k_ref"], x["v_ref"] = k.clone(), v.clone()
        x["k_ref"][BAD, 0], x["v_ref"][BAD, 0] = 0.0, 0.0
    return x


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 on the same numbers: ``out``, the row maximum ``m`` and ``logsum`` of the scores (rows in the kernel's
    order), and ``err32``, the largest error of the reference's own formula evaluated in float32 on the CPU."""
    from pydrobert_amd import _attn

    x = inputs(name)
    q, k, v, dim = x["q"], x["k_ref"], x["v_ref"], x["dim"]
    s = (q.double().unsqueeze(dim) * k.double()).sum(-1) * x["scale"]
    mv = None if x["mask"] is None else x["mask"].view(s.shape)
    if mv is not None:
        s = torch.where(mv, s, torch.full_like(s, -float("inf")))
    m = s.max(dim).values
    out = R.attend_ref(q.double(), k.double(), v.double(), mv, dim, x["scale"])
    f32 = _attn._softmax_pool((q.unsqueeze(dim) * k).sum(-1) * x["scale"], v, mv, dim)
    return dict(out=out, m=m.reshape(-1), logsum=torch.log(torch.exp(s - m.unsqueeze(dim)).nan_to_num(0.0).sum(dim)).reshape(-1),
                err32=float((f32.double() - out).abs().nan_to_num(0.0).max()))  # fmt: skip
