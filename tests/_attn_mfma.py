"""Shared by tests/test_attn_mfma_cpu.py and tests/test_attn_mfma_gpu.py: the cases of the matrix-core attention
forward (csrc/attn_mfma.hip), their inputs in a half dtype, the float64 reference on the exactly widened inputs and
the derived bounds.  The formula and the random mask are those of tests/_attn_ref.py.

Layout as there: dim 0 is the attended axis; query (G, M, D), key (T, G, 1, D), value (T, G, 1, Dv), mask (T, G, M).
"""
import functools

import numpy as np
import torch

import _attn_ref as R

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ELEM = {"float16": 2, "bfloat16": 3}
U = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}

# name -> shape, mask recipe, and what the plan must say: spans of T (a span is at least two key blocks of 64)
CASES = {
    "one-block": dict(G=3, M=64, T=64, D=64, Dv=64, mask=None, splits=1),
    "tails-length": dict(G=2, M=100, T=70, D=64, Dv=128, mask="length", splits=1),
    "causal": dict(G=2, M=200, T=200, D=128, Dv=64, mask="causal", splits=2),
    "random-96": dict(G=2, M=96, T=96, D=96, Dv=32, mask="random", splits=1),
    "split": dict(G=1, M=64, T=300, D=64, Dv=64, mask="empty-span", splits=2),
    "dead-row": dict(G=2, M=70, T=40, D=64, Dv=64, mask="dead-row", splits=1),
    "strided": dict(G=4, M=64, T=64, D=64, Dv=64, mask=None, splits=1),
    "shifted": dict(G=2, M=64, T=64, D=32, Dv=32, mask=None, splits=1),
}
GRAD_CASES = ("causal", "split")
DEAD = (1, 35)  # the all-masked row of "dead-row"
LENGTHS = (70, 40)  # "tails-length": group 1 ends inside key block 0, its block 1 is attended by no row


def desc(G, M, T, D, Dv, q_row=0, kv_ts=0, fs=1):
    """A descriptor (include/pdt_amd.h) of rows (G, M) in the layout above with a contiguous out; ``q_row`` the
    query's stride between rows (default D), ``kv_ts`` the T stride of key and value (default: contiguous), ``fs``
    the feature stride of query, key, value and out.  Only the host reads it here."""
    import ctypes

    from pydrobert_amd import _attn as A

    q_row = q_row or D
    d = [0] * A._DESC_LEN
    d[0:9] = [2, G * M, G, M, T, D, Dv, G, M]
    slots = {  # slot: (stride of G, stride of M, T stride, feature stride)
        A._SQ: (M * q_row, q_row, 0, fs), A._SK: (D, 0, kv_ts or G * D, fs), A._SV: (Dv, 0, kv_ts or G * Dv, fs),
        A._SM: (M, 1, G * M, 0), A._SO: (M * Dv, Dv, 0, fs), A._SGQ: (M * D, D, 0, 1), A._SGK: (D, 0, G * D, 1),
        A._SGV: (Dv, 0, G * Dv, 1),
    }  # fmt: skip
    for slot, (sg, sm, ts, f) in slots.items():
        base = 7 + A._MAX_DIMS + slot * (A._MAX_DIMS + 2)
        d[base:base + 2] = [sg, sm]
        d[base + A._MAX_DIMS:base + A._MAX_DIMS + 2] = [ts, f]
    return (ctypes.c_int64 * len(d))(*d)


def plan(lib, d, elem):
    import ctypes

    p = (ctypes.c_int64 * 7)()
    return lib.pdt_attn_dot_mfma_plan(d, elem, ctypes.addressof(p)), list(p)


def _mask(c, rng):
    T, G, M = c["T"], c["G"], c["M"]
    t = np.arange(T).reshape(T, 1, 1)
    if c["mask"] is None:
        return None
    if c["mask"] == "length":
        return np.broadcast_to(t < np.array(LENGTHS).reshape(1, G, 1), (T, G, M)).copy()
    if c["mask"] == "causal":
        return np.broadcast_to(t <= np.arange(M).reshape(1, 1, M), (T, G, M)).copy()
    mask = R.make_mask("random", rng, T, G, M)
    if c["mask"] == "empty-span":
        mask[192:] = False  # the second span of 192 frames
    if c["mask"] == "dead-row":
        mask[(slice(None),) + DEAD] = False
    return mask


@functools.lru_cache(maxsize=None)
def inputs(name, dtname):
    """The operator's arguments of a case as CPU tensors of the half dtype (``q``, ``k``, ``v``, ``mask``, ``scale``)
    and ``k_ref`` / ``v_ref``, the copies the reference reads (without the NaN planted in padded frames)."""
    c, dt = CASES[name], DTYPES[dtname]
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
    q, k, v = (torch.from_numpy(x).to(dt) for x in (q, k, v))
    mask = _mask(c, rng)
    x = dict(scale=scale, mask=None if mask is None else torch.from_numpy(mask), k_ref=k, v_ref=v)
    if name == "tails-length":
        k, v = k.clone(), v.clone()
        for g, n in enumerate(LENGTHS):
            k[n:, g], v[n:, g] = float("nan"), float("nan")
    if name == "strided":  # key and value of a (T, N, H, d) tensor with the heads a row dim; query rows 2 d apart
        kv = torch.stack([k.view(T, 2, 2, D), v.view(T, 2, 2, D)])
        k, v = kv[0].unsqueeze(3), kv[1].unsqueeze(3)
        q = torch.cat([q.view(2, 2, M, D), torch.zeros(2, 2, M, D, dtype=dt)], -1)[..., :D]
        x.update(k_ref=k, v_ref=v, mask=None)
    x.update(q=q, k=k, v=v)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, dtname):
    """float64 on the widened inputs: ``out``, the row maximum ``m`` and ``logsum`` of the scores (rows in the
    kernel's order), ``A`` = sum_t a_t |v_t| per output element, and max |v|."""
    x = inputs(name, dtname)
    q, k, v = x["q"].double(), x["k_ref"].double(), x["v_ref"].double()
    s = (q.unsqueeze(0) * k).sum(-1) * x["scale"]
    if x["mask"] is not None:
        s = torch.where(x["mask"].view(s.shape), s, torch.full_like(s, -float("inf")))
    m = s.max(0).values
    a = torch.exp(s - m).nan_to_num(0.0)
    a = a / a.sum(0, keepdim=True)
    return dict(out=R.attend_ref(q, k, v, None if x["mask"] is None else x["mask"].view(s.shape), 0, x["scale"]),
                m=m.reshape(-1), logsum=torch.log(torch.exp(s - m).nan_to_num(0.0).sum(0)).reshape(-1),
                A=(a.unsqueeze(-1) * v.abs()).sum(0), vmax=float(v.abs().max()))  # fmt: skip


def out_bound(ref, A, vmax, T, dtname):
    """(2e-5 + 2e-5 |ref|) + u A + u |ref| + [float16] T 2^-25 max|v|: the suite's float32 bound, the one rounding
    of P, the one rounding of out, and p below float16's normal range.  Derived, not measured."""
    u = U[dtname]
    return 2e-5 + 2e-5 * ref.abs() + u * A + u * ref.abs() + (T * 2.0 ** -25 * vmax if dtname == "float16" else 0.0)
