"""Shared by tests/test_attn_mfma_forms_cpu.py and tests/test_attn_mfma_forms_gpu.py: the forms of the matrix-core
attention kernels (csrc/attn_mfma.hip, attn_mfma_bwd.hip, attn_mfma_f32.hip) that the cases of tests/_attn_mfma.py and
tests/_attn_mfma_f32.py leave out, as one table for the half forward, the half backward and the float32 forward.

Head-dim and walk forms are in the layout of tests/_attn_mfma.py (dim 0 the attended axis; query (G, M, D), key
(T, G, 1, D), value (T, G, 1, Dv), mask (T, G, M)); the layout forms hold the operator's arguments themselves.  Every
form has a seed of its own, normal deviates and scale 0.25; ``float32`` is a dtype name here beside the two of
``_attn_mfma.DTYPES``.
"""
import functools

import numpy as np
import torch

import _attn_ref as R
from _attn_mfma import DTYPES

ALL_DTYPES = dict(DTYPES, float32=torch.float32)
SCALE = 0.25

# name -> the seed, (G, M, T, D, Dv) as the plan sees them, and the spans of T the forward plans must report
FORMS = {
    # head dims that are odd multiples of 16: the last 32-column chunk of the half kernels is half empty
    "d48-dv112": dict(seed=101, G=2, M=80, T=100, D=48, Dv=112, mask="random", splits=1),
    "d112-dv48": dict(seed=102, G=1, M=64, T=130, D=112, Dv=48, mask="random", splits=1),
    "d80-dv80": dict(seed=103, G=2, M=64, T=64, D=80, Dv=80, mask=None, splits=1),
    "d128-dv128": dict(seed=104, G=1, M=80, T=72, D=128, Dv=128, mask="t<=m", splits=1),
    # d48-dv112 with every row of query, key and value followed by sixteen NaN: what a load of the empty half of the
    # last chunk would fetch (each product zeroes both of its operands there, so finite neighbours would hide one)
    "nan-gaps": dict(seed=110, G=2, M=80, T=100, D=48, Dv=112, mask="random", splits=1),
    # walks: three partials through the combine, and the smallest T
    "three-spans": dict(seed=105, G=1, M=64, T=520, D=64, Dv=48, mask="three-spans", splits=3),
    "one-frame": dict(seed=106, G=2, M=64, T=1, D=32, Dv=32, mask=None, splits=1),
    # layouts: the kernel's row order is not the output's, dim 1, masks of stride 0, slices of one projection
    "batch-first": dict(seed=107, G=4, M=66, T=70, D=32, Dv=48, splits=1),
    "shared-causal": dict(seed=108, G=3, M=70, T=70, D=64, Dv=64, mask="causal", splits=1),
    "fused-qkv": dict(seed=109, G=8, M=70, T=70, D=32, Dv=32, splits=1),
    # half-empty chunks (48, 80) under a band |t - m| <= 8 shared by the groups: consecutive rows attend frames the
    # other masks and consecutive frames are attended by rows the other is not, which is what shows a fragment read
    # from LDS beyond D or Dv -- it holds the NEXT row's first eight columns (the neighbour tests plant a NaN there)
    "band-d48": dict(seed=111, G=2, M=70, T=70, D=48, Dv=80, mask="band", splits=1),
}
# ``base`` with one NaN key in a frame that some rows of its 64-row block attend and others mask (forward only)
for _name, _base in (("key-nan", "shared-causal"), ("key-nan-d48", "band-d48")):
    FORMS[_name] = dict(FORMS[_base], base=_base)
BACKWARD_FORMS = tuple(n for n in FORMS if "base" not in FORMS[n])
BAND = 8
SPAN = 192  # three-spans: 9 key blocks of 64 in 3 spans of 3; the last span has 520 - 384 = 136 frames
LENGTHS = (70, 41)  # batch-first: the second batch element ends inside key block 0, its block 1 is attended by no row
NAN_KEY = (37, 1)  # key-nan*: (frame, group); causal: rows 37..69 of the group attend the frame, band: rows 29..45
FUSED = dict(T=70, N=2, H=4, d=32)
GAP = 16  # nan-gaps: the NaN elements behind every row, the empty half of a chunk of 32


def split_fused(fused):
    """Query, key and value of a (T, N, 3 H d [+ padding]) projection: three slices of the last axis viewed
    (T, N, H, d), key and value with the query axis of size 1 in front of N."""
    T, N, H, d = FUSED["T"], FUSED["N"], FUSED["H"], FUSED["d"]
    q, k, v = (fused[..., i * H * d:(i + 1) * H * d].view(T, N, H, d) for i in range(3))
    return q, k.unsqueeze(1), v.unsqueeze(1)


def split_of(name):
    """How a form's query, key and value come from its autograd leaves (``leaves``): views, so that the views'
    strides reach the operators."""
    if name == "fused-qkv":
        return split_fused
    if name == "nan-gaps":
        D, Dv = FORMS[name]["D"], FORMS[name]["Dv"]
        return lambda a, b, c: (a[..., :D], b[..., :D], c[..., :Dv])
    return lambda a, b, c: (a, b, c)


def leaves(name, x, ref=False):
    """The tensors a form's gradients are taken of: fused-qkv's one projection, nan-gaps' three wide tensors, else
    query, key and value themselves (``ref``: the copies the reference reads)."""
    if name == "fused-qkv":
        return [x["fused"]]
    if name == "nan-gaps":
        return list(x["wide"])
    return [x["q"], x["k_ref"], x["v_ref"]] if ref else [x["q"], x["k"], x["v"]]


def _three_spans_mask(rng, T, G, M):
    mask = R.make_mask("random", rng, T, G, M)
    mask[SPAN:2 * SPAN] = False  # an empty middle span
    mask[SPAN:, 0, 0:16] = False  # rows 0..15: only span 0
    mask[:2 * SPAN, 0, 16:32] = False  # rows 16..31: only the tail span
    for m in np.flatnonzero(~mask.any(0)[0]):  # (no row may be dead: one frame of the span the row keeps)
        mask[2 * SPAN + m if 16 <= m < 32 else m, 0, m] = True
    return mask


@functools.lru_cache(maxsize=None)
def inputs(name, dtname, pad=0):
    """The operator's arguments of a form as CPU tensors of the dtype: ``q``, ``k``, ``v``, ``mask`` (as it is passed:
    dims of size 1 where it is shared), ``dim``, ``scale``; ``k_ref`` / ``v_ref``, the copies the reference reads
    (without the NaN planted in padded frames; key-nan's NaN key is no padding and stays); for fused-qkv ``fused``,
    the one tensor the three are slices of, its last axis ``pad`` elements longer than 3 H d; for nan-gaps ``wide``,
    the three tensors with ``GAP`` NaN behind every row that query, key and value are views of.  Cached: read-only."""
    c, dt = FORMS[name], ALL_DTYPES[dtname]
    if "base" in c:
        x = dict(inputs(c["base"], dtname))
        x["k"] = x["k"].clone()
        x["k"][NAN_KEY] = float("nan")
        x["k_ref"] = x["k"]
        return x
    G, M, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    rng = np.random.default_rng(c["seed"])
    x = dict(dim=0, scale=SCALE)
    if name == "batch-first":
        N, H = 2, 2
        q, k, v = rng.normal(size=(N, M, H, D)), rng.normal(size=(N, T, 1, H, D)), rng.normal(size=(N, T, 1, H, Dv))
        q, k, v = (torch.from_numpy(a).to(dt) for a in (q, k, v))
        x.update(dim=1, k_ref=k, v_ref=v)
        x["mask"] = (torch.arange(T).view(1, T, 1, 1) < torch.tensor(LENGTHS).view(N, 1, 1, 1))
        k, v = k.clone(), v.clone()
        for n, length in enumerate(LENGTHS):
            k[n, length:], v[n, length:] = float("nan"), float("nan")
    elif name == "fused-qkv":
        H, d = FUSED["H"], FUSED["d"]
        fused = torch.zeros(T, FUSED["N"], 3 * H * d + pad, dtype=dt)
        fused[..., :3 * H * d] = torch.from_numpy(rng.normal(size=(T, FUSED["N"], 3 * H * d))).to(dt)
        q, k, v = split_fused(fused)
        x.update(fused=fused, k_ref=k, v_ref=v)
        x["mask"] = (torch.arange(T).view(T, 1, 1, 1) <= torch.arange(T).view(1, T, 1, 1))  # (key frame, query frame)
    else:
        q, k, v = rng.normal(size=(G, M, D)), rng.normal(size=(T, G, 1, D)), rng.normal(size=(T, G, 1, Dv))
        q, k, v = (torch.from_numpy(a).to(dt) for a in (q, k, v))
        if name == "nan-gaps":
            wide = tuple(torch.full(t.shape[:-1] + (t.shape[-1] + GAP,), float("nan"), dtype=dt) for t in (q, k, v))
            for w, t in zip(wide, (q, k, v)):
                w[..., :t.shape[-1]] = t
            q, k, v = split_of(name)(*wide)
            x["wide"] = wide
        if c["mask"] == "causal":
            x["mask"] = (torch.arange(T).view(T, 1, 1) <= torch.arange(M).view(1, 1, M))  # (T, 1, M): every group's
        elif c["mask"] == "band":
            x["mask"] = ((torch.arange(T).view(T, 1, 1) - torch.arange(M).view(1, 1, M)).abs() <= BAND)  # (T, 1, M)
        elif c["mask"] == "t<=m":
            x["mask"] = (torch.arange(T).view(T, 1, 1) <= torch.arange(M).view(1, 1, M)).expand(T, G, M).contiguous()
        elif c["mask"] == "three-spans":
            x["mask"] = torch.from_numpy(_three_spans_mask(rng, T, G, M))
        else:
            mask = R.make_mask(c["mask"], rng, T, G, M)
            x["mask"] = None if mask is None else torch.from_numpy(mask)
        x.update(k_ref=k, v_ref=v)
    assert pad == 0 or name == "fused-qkv"
    x.update(q=q, k=k, v=v)
    return x


def to_kernel_order(t, S, order, dim):
    """``t`` of shape ``S`` without ``dim`` (the output's row dims) as a vector in the kernel's row order: the dims of
    ``_Plan.order`` outermost to innermost; row dims of size 1 are in no order and do not matter."""
    assert list(t.shape) == [s for i, s in enumerate(S) if i != dim]
    perm = [i if i < dim else i - 1 for i in order]
    rest = [j for j in range(t.dim()) if j not in perm]
    assert all(t.shape[j] == 1 for j in rest)
    return t.permute(rest + perm).reshape(-1)


@functools.lru_cache(maxsize=None)
def reference(name, dtname, zero_nan_key=False):
    """float64 on the exactly widened reference operands: ``out``; the row maximum ``m`` and ``logsum`` of the scores
    at the output's row shape; ``A`` = sum_t a_t |v_t| per output element and max |v| (``_attn_mfma.out_bound``);
    ``err32`` (float32 only), the largest error of the reference's formula evaluated in float32 on the CPU.
    ``zero_nan_key``: a key-nan form with its NaN key replaced by 0, what the rows that mask the frame must not differ from."""
    from pydrobert_amd import _attn

    x = inputs(name, dtname)
    dim, scale, mask = x["dim"], x["scale"], x["mask"]
    q, k, v = x["q"], x["k_ref"], x["v_ref"]
    if zero_nan_key:
        k = k.nan_to_num(0.0)
    q64, k64, v64 = q.double(), k.double(), v.double()
    s = (q64.unsqueeze(dim) * k64).sum(-1) * scale
    if mask is not None:
        s = torch.where(mask, s, torch.full_like(s, -float("inf")))
    m = s.max(dim, keepdim=True).values
    p = torch.exp(s - m)
    a = p / p.sum(dim, keepdim=True)
    ref = dict(out=R.attend_ref(q64, k64, v64, mask, dim, scale), m=m.squeeze(dim), logsum=torch.log(p.sum(dim)),
               A=(a.unsqueeze(-1) * v64.abs()).sum(dim), vmax=float(v64.abs().max()))  # fmt: skip
    if dtname == "float32":
        f32 = _attn._softmax_pool((q.unsqueeze(dim) * k).sum(-1) * scale, v, mask, dim)
        ref["err32"] = float((f32.double() - ref["out"]).abs().nan_to_num(0.0).max())
    return ref


def plan_formulas(c):
    """What the kernels' headers say the plans report for a form: spans of T and the frames of one (a span is at
    least two key blocks of 64, and T is split only while G x row blocks leave the chip unfilled: 512 workgroups),
    the forward's workspace, and the LDS bytes of the half forward, the two backward kernels and the float32 forward."""
    G, M, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    blocks, frame_blocks = G * -(-M // 64), -(-T // 64)
    splits = min(max(1, -(-512 // blocks)), max(1, frame_blocks // 2))
    span = -(-frame_blocks // splits) * 64
    splits = -(-T // span)
    lds_q = 2 * (64 * (D + 8) + 72 * D + 64 * (Dv + 8))
    return dict(splits=splits, span=span, ws=0 if splits == 1 else splits * G * M * (Dv + 2) * 4,
                lds_half=2 * (64 * (D + 8) + 72 * Dv), lds_q=lds_q, lds_kv=lds_q + 144 * Dv,
                lds_f32=256 * (D + Dv + 8), delta_ws=4 * G * M)  # fmt: skip
