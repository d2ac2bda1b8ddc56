"""Shared by tests/test_half_attn_cpu.py and tests/test_half_attn_gpu.py: the cases, the leaves in a half dtype, the
operator calls of a case (forward and backward, called directly), bit patterns, the derived forward bound and the
byte counts of the no-copy test.  The inputs, the plan restatement and the float64 formula are those of
tests/_attn_ref.py, which this file only reads.

Inputs: the float32 cases of ``R.CASES`` (the smallest shapes that reach each plan form), their float64 arrays
cast to the half dtype; and the one case with a host reduction behind the kernel, a value broadcast along T
(``VBT``: float64 in the table, here cast to half like the others)."""
import ctypes

import torch

import _attn_ref as R

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
ELEM = {"float32": 0, "float16": 2, "bfloat16": 3}
F32_CASES = [n for n, c in R.CASES.items() if c["dtype"] == "float32"]
VBT = "chunks-value-broadcast-along-T"
BIT_CASES = F32_CASES + [VBT]
BOUND_CASES = [n for n in F32_CASES if not R.CASES[n]["measured"]]
assert R.CASES[VBT]["vbt"] and len(F32_CASES) > 60 and len(BOUND_CASES) > 30
MIB = 1 << 20

ENTRIES = ("pdt_attn_workspace_bytes", "pdt_attn_dot", "pdt_attn_dot_backward", "pdt_attn_pool",
           "pdt_attn_pool_backward")  # fmt: skip


def desc(R_=6, G=2, M=3, T=5, D=4, Dv=3, sizes=(2, 3)):
    """A valid descriptor (include/pdt_amd.h): rows ``sizes``, the inner dim the group (key and value strides 0
    there), every other stride made up (no call that takes it here reaches a launch)."""
    from pydrobert_amd import _attn

    d = [0] * _attn._DESC_LEN
    d[0:7] = [len(sizes), R_, G, M, T, D, Dv]
    d[7:7 + len(sizes)] = list(sizes)
    for slot in range(_attn._SLOTS):
        base = 7 + _attn._MAX_DIMS + slot * (_attn._MAX_DIMS + 2)
        d[base] = 7
        d[base + _attn._MAX_DIMS] = 1
        d[base + _attn._MAX_DIMS + 1] = 1
        if slot not in (_attn._SK, _attn._SV, _attn._SGK, _attn._SGV):
            d[base + 1] = 2
    return (ctypes.c_int64 * len(d))(*d)


def leaves(name, dtype, device, spoiled=False):
    """{leaf name: tensor of ``dtype``} of a case (``q``, ``k``, ``v`` or ``e``, ``v``), ``gout`` and ``mask`` (bool
    or None): the case's float64 arrays cast once; ``spoiled`` takes the copies with non-finite masked frames."""
    c, x = R.CASES[name], R.build_inputs(name)
    L = {}
    for n in R.LEAVES[c["route"]] + ("gout",):
        a = x[n + "_bad"] if spoiled and n + "_bad" in x else x[n]
        L[n] = torch.from_numpy(a.copy()).to(device=device, dtype=dtype)
    L["mask"] = None if x["mask"] is None else torch.from_numpy(x["mask"].copy()).to(device)
    return L


def widened(L):
    return {n: t.float() if t is not None and t.is_floating_point() else t for n, t in L.items()}


def operands(name, L):
    """The operator's tensor arguments of a case from its leaves, as ``R.run_case`` forms them: (query, key, value)
    or (score, value), the strided query view and the caller's expansion included."""
    c = R.CASES[name]
    G, M, T, Dv = c["G"], c["M"], c["T"], c["Dv"]
    value = L["v"].expand(T, G, M, Dv) if c["expand"] else L["v"]
    if c["route"] == "pool":
        return (L["e"], value)
    key = L["k"].expand(T, G, M, c["D"]) if c["expand"] else L["k"]
    return (L["q"][..., ::c["qstride"]], key, value)


def forward(name, L):
    """(out, lse) of the case's operator called directly (no autograd)."""
    ops = torch.ops.pydrobert_amd
    x = R.build_inputs(name)
    if R.CASES[name]["route"] == "pool":
        return ops.attention_pool(*operands(name, L), L["mask"], 0)
    return ops.dot_attention(*operands(name, L), L["mask"], 0, x["scale"])


def backward(name, L, g, out, lse):
    """{leaf name: gradient} of the case's backward operator called directly, in the operands' shapes."""
    ops = torch.ops.pydrobert_amd
    x = R.build_inputs(name)
    if R.CASES[name]["route"] == "pool":
        return dict(zip(("e", "v"), ops.attention_pool_backward(g, *operands(name, L), L["mask"], out, lse, 0)))
    grads = ops.dot_attention_backward(g, *operands(name, L), L["mask"], out, lse, 0, x["scale"])
    return dict(zip(("q", "k", "v"), grads))


def bits(x):
    """The bit patterns of a tensor, NaNs included."""
    return x.contiguous().view({2: torch.int16, 4: torch.int32}[x.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def ulp(x, dtype):
    """ulp_E(x) = 2^(floor(log2 x) - p): p = 10 for float16, floored at 2^-24 (its subnormal spacing), p = 7 for
    bfloat16.  ``x`` a float64 tensor of non-negative numbers."""
    p = 10 if dtype == torch.float16 else 7
    e = torch.floor(torch.log2(x.clamp_min(1e-300)))
    u = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - p)
    return u.clamp_min(2.0 ** -24) if dtype == torch.float16 else u


def forward_bound(ref, dtype):
    """|out - ref| <= b + ulp_E(|ref| + b) / 2 with b = 2e-5 + 2e-5 |ref|: the float32 kernels' bound in the suite
    (``R.SUITE``, as ``R.compare`` applies it) plus one rounding to the element type of a number that far from
    ``ref`` at the most.  Derived, not measured."""
    tol = R.SUITE["float32"][0]
    b = tol + tol * ref.abs()
    return b + ulp(ref.abs() + b, dtype) / 2


# the no-copy test: decode-shaped dot_attention, the key 16 MiB in bfloat16
NOCOPY = dict(N=64, K=8, T=512, D=256)


def nocopy_bytes(esz):
    """What the no-copy test allows, from the shapes and the plan restatement alone: (forward, backward, the
    torch formula's smallest intermediate) in bytes for operands of ``esz`` bytes an element."""
    s = NOCOPY
    N, K, T, D = s["N"], s["K"], s["T"], s["D"]
    rows = N * K
    out, lse = rows * D * esz, 2 * rows * 4
    fwd_ws = R.plan_of(N, K, T, D, D, 4, "dot")["ws_bytes"]
    bwd_ws = R.plan_of(N, K, T, D, D, 4, "dot_bwd")["ws_bytes"]
    grads = (rows * D + 2 * T * N * D) * esz
    formula = T * N * K * D * esz  # (query * key at the full broadcast shape)
    return out + lse + fwd_ws, grads + bwd_ws + out, formula
