"""Shared by tests/test_attn_mfma_f32_cpu.py and tests/test_attn_mfma_f32_gpu.py: the cases of the float32
matrix-core attention forward (csrc/attn_mfma_f32.hip), their float32 inputs and the float64 reference on the same
numbers.  Descriptors, masks and the layout (dim 0 the attended axis; query (G, M, D), key (T, G, 1, D), value
(T, G, 1, Dv), mask (T, G, M)) are those of tests/_attn_mfma.py."""
import functools

import numpy as np
import torch

import _attn_ref as R
from _attn_mfma import DEAD, LENGTHS, _mask, desc  # noqa: F401

# name -> shape, mask recipe, and what the plan must say: spans of T (a span is at least two key blocks of 64)
CASES = {
    "one-block": dict(G=3, M=64, T=64, D=64, Dv=64, mask=None, splits=1),
    "tails-length": dict(G=2, M=100, T=70, D=64, Dv=128, mask="length", splits=1),
    "causal": dict(G=2, M=200, T=200, D=128, Dv=64, mask="causal", splits=2),
    "sixteens": dict(G=2, M=96, T=96, D=48, Dv=80, mask="random", splits=1),
    "split": dict(G=1, M=64, T=300, D=64, Dv=64, mask="empty-span", splits=2),
    "dead-row": dict(G=2, M=70, T=40, D=64, Dv=64, mask="dead-row", splits=1),
    "big-lds": dict(G=1, M=80, T=72, D=128, Dv=128, mask="causal", splits=1),
    "strided": dict(G=4, M=64, T=64, D=64, Dv=64, mask=None, splits=1),
    "shifted": dict(G=2, M=64, T=64, D=32, Dv=32, mask=None, splits=1),
}
GRAD_CASES = ("causal", "split")


def plan(lib, d):
    import ctypes

    p = (ctypes.c_int64 * 7)()
    return lib.pdt_attn_dot_mfma_f32_plan(d, ctypes.addressof(p)), list(p)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The operator's arguments of a case as float32 CPU tensors (``q``, ``k``, ``v``, ``mask``, ``scale``) and
    ``k_ref`` / ``v_ref``, the copies the reference reads (without the NaN planted in padded frames)."""
    c = CASES[name]
    G, M, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    rng = np.random.default_rng(sorted(CASES).index(name))
    q, k, v = rng.normal(size=(G, M, D)), rng.normal(size=(T, G, 1, D)), rng.normal(size=(T, G, 1, Dv))
    scale = 0.25
    if name == "causal":  # scores rising along T, then falling: the running maximum moves, then stays
        q[..., 0] = 2.0
        k[..., 0] = 12.0 * (1.0 - np.abs(np.arange(T) - T / 2) / (T / 2)).reshape(T, 1, 1)
    if name == "shifted":
        q[..., 0], k[..., 0], scale = 10.0, 10.0, 1.0
        q[..., 1:] *= 0.25
    q, k, v = (torch.from_numpy(x).float() for x in (q, k, v))
    mask = _mask(c, rng)
    x = dict(scale=scale, mask=None if mask is None else torch.from_numpy(mask), k_ref=k, v_ref=v)
    if name == "tails-length":
        k, v = k.clone(), v.clone()
        for g, n in enumerate(LENGTHS):
            k[n:, g], v[n:, g] = float("nan"), float("nan")
    if name == "strided":  # key and value views of one (2, T, 2, 2, d) stack; query rows D + 4 elements apart
        kv = torch.stack([k.view(T, 2, 2, D), v.view(T, 2, 2, D)])
        k, v = kv[0].unsqueeze(3), kv[1].unsqueeze(3)
        q = torch.cat([q.view(2, 2, M, D), torch.zeros(2, 2, M, 4)], -1)[..., :D]
        x.update(k_ref=k, v_ref=v)
    x.update(q=q, k=k, v=v)
    return x


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 on the same numbers: ``out``, the row maximum ``m`` and ``logsum`` of the scores (rows in the kernel's
    order), and ``err32``, the largest error of the reference's own formula evaluated in float32 on the CPU."""
    from pydrobert_amd import _attn

    x = inputs(name)
    q, k, v, mask = x["q"], x["k_ref"], x["v_ref"], x["mask"]
    s = (q.double().unsqueeze(0) * k.double()).sum(-1) * x["scale"]
    mv = None if mask is None else mask.view(s.shape)
    if mv is not None:
        s = torch.where(mv, s, torch.full_like(s, -float("inf")))
    m = s.max(0).values
    out = R.attend_ref(q.double(), k.double(), v.double(), mv, 0, x["scale"])
    f32 = _attn._softmax_pool((q.unsqueeze(0) * k).sum(-1) * x["scale"], v, mv, 0)
    return dict(out=out, m=m.reshape(-1), logsum=torch.log(torch.exp(s - m).nan_to_num(0.0).sum(0)).reshape(-1),
                err32=float((f32.double() - out).abs().nan_to_num(0.0).max()))  # fmt: skip
