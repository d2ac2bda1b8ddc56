"""float16 / bfloat16 logits read without a float32 copy: the case table and the input builders of
tests/test_half_logits_cpu.py and tests/test_half_logits_gpu.py.

The contract under test has no tolerance in it: a half element is widened exactly where a kernel loads
it, and everything behind the load is the float32 kernel, so every output of a call on ``x`` equals,
bit for bit, the output of the float32 entry point on ``x.float()`` (cast to the half type where the
operator returns ``logits.dtype``).  The inputs therefore carry what an inexact or reordered load would
trip over: exact ties inside a row (one of them for the row maximum), both zeros, float16 subnormals,
the largest finite float16 and a peaky row -- no inf, no NaN.
"""
import torch

HALF_DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}

# ---- CTC prefix search: one case per kernel form, at the smallest shape that selects it --------------
# name -> dict(V, W, T, N, layout, form).  `form` is what tests/test_half_logits_cpu.py asserts through the
# plan queries (plan5 of pdt_ctc_prefix_search_plan: producers, ring slots, utterances per workgroup, where a
# row is held -- 1 registers of one producer, 3 registers of three (rowreg), 0 LDS ring, 2 workspace --, register
# chunks of the rowreg instance):
#   ("narrow", producers, where, chunks, rowreg_contiguous)  -- the plan that serves the case's LAYOUT: strided
#       vocabularies never take rowreg, so their plan is the one PDT_CTC_ROWREG=0 reports;
#   ("wide", row_lds, nxt_lds).
# layouts: "contig"; "transposed" (a (T, V + 1, N) buffer viewed as (T, N, V + 1): vocabulary stride N);
# "offset" (contiguous rows one element behind an aligned buffer: row starts are 2-byte aligned only);
# "padded" (rows of V + 1 inside rows of V + 4: lg_sn != V + 1).
CTC_CASES = {
    "general_tiny": dict(V=5, W=3, T=37, N=3, layout="contig", form=("narrow", 1, 1, 0)),
    "general_w32": dict(V=200, W=32, T=37, N=3, layout="contig", form=("narrow", 1, 1, 0)),
    "four_chunk": dict(V=300, W=4, T=37, N=3, layout="contig", form=("narrow", 1, 1, 0)),
    "four_chunk_w16": dict(V=300, W=16, T=37, N=3, layout="contig", form=("narrow", 1, 1, 0)),
    "headline": dict(V=256, W=16, T=37, N=3, layout="contig", form=("narrow", 1, 1, 0)),
    "rowreg_rem0_nr8": dict(V=320, W=16, T=37, N=3, layout="contig", form=("narrow", 3, 3, 8)),
    "rowreg_rem63_nr16": dict(V=1023, W=5, T=37, N=3, layout="contig", form=("narrow", 3, 3, 16)),
    "rowreg_nt_nr24": dict(V=1100, W=16, T=37, N=3, layout="contig", form=("narrow", 3, 3, 24)),
    "rowreg_nr80": dict(V=5000, W=16, T=24, N=3, layout="contig", form=("narrow", 3, 3, 80)),
    "strided_one_producer": dict(V=400, W=8, T=37, N=3, layout="transposed", form=("narrow", 1, 1, 0)),
    "strided_lds_ring": dict(V=600, W=8, T=37, N=3, layout="transposed", form=("narrow", 3, 0, 0)),
    "workspace_rows": dict(V=17000, W=4, T=8, N=2, layout="contig", form=("narrow", 3, 2, 0)),
    "offset_headline": dict(V=256, W=16, T=37, N=3, layout="offset", form=("narrow", 1, 1, 0)),
    "offset_rowreg": dict(V=320, W=16, T=37, N=3, layout="offset", form=("narrow", 3, 3, 8)),
    "padded_v256": dict(V=256, W=16, T=37, N=3, layout="padded", form=("narrow", 1, 1, 0)),
    # the wide kernel: V = None stands for the first V whose row leaves the LDS (wide_row_bound)
    "wide33_lds": dict(V=40, W=33, T=12, N=2, layout="contig", form=("wide", 1, 1)),
    "wide128_lds": dict(V=40, W=128, T=12, N=2, layout="contig", form=("wide", 1, 0)),
    "wide33_ws": dict(V=None, W=33, T=5, N=2, layout="contig", form=("wide", 0, 1)),
    "wide128_ws": dict(V=None, W=128, T=5, N=2, layout="contig", form=("wide", 0, 0)),
}
# cases whose narrow plan is asked for with PDT_CTC_ROWREG=0 (what their strided layout is served by)
STRIDED_VOCAB = ("strided_one_producer", "strided_lds_ring")

GREEDY_CLASSES = (9, 512, 513, 1024, 1025)  # register form of 8 chunks / of 16 / streamed, at their edges
SLP_CLASSES = (9, 512, 513, 1025)

# "the copy is gone": 2.05 M logits, a float32 copy of them is 8.2 MB
NOCOPY = dict(T=64, N=16, V=1999, W=4)
MIB = 1 << 20


def wide_row_bound(lib, W):
    """The first V whose row of probabilities the wide kernel keeps in the workspace (plan bit 0 = 0)."""
    import ctypes

    plan = (ctypes.c_int32 * 2)()

    def in_lds(V):
        assert lib.pdt_ctc_prefix_search_wide_plan(V, W, plan) == 0, (V, W)
        return plan[0] == 1

    lo, hi = 40, 1 << 16
    assert in_lds(lo) and not in_lds(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if in_lds(mid):
            lo = mid
        else:
            hi = mid
    return hi


def case_vocab(lib, name):
    case = CTC_CASES[name]
    return case["V"] if case["V"] is not None else wide_row_bound(lib, case["W"])


def planted(shape, dtype, seed, device="cpu"):
    """A seeded float32 draw of ``shape`` = (..., classes), rounded to ``dtype``, with the special values planted
    in the rows (row r = flattened leading index; columns taken modulo the row length, so tiny rows keep what
    fits).  Returned contiguous, on ``device``."""
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = (torch.randn(shape, generator=g) * 3.0).to(dtype)
    rows = x.view(-1, C)
    R = rows.shape[0]

    def col(c):
        return c % C

    for r in range(R):
        row = rows[r]
        # exact ties: two pairs somewhere in the row
        row[col(3)] = row[col(1)]
        if C > 70:
            row[col(69)] = row[col(5)]  # (across two 64-element chunks: another lane's register)
        if r % 3 == 0:  # a tie for the row maximum at two indices
            top = (row.float().max() + 1.0).to(dtype)
            row[col(2)] = top
            row[col(C - 2)] = top
        if r % 4 == 1:  # both zeros
            row[col(0)] = 0.0
            row[col(4)] = -0.0
        if r % 4 == 2:  # float16 subnormals (bfloat16 holds them as normal numbers)
            row[col(6)] = torch.tensor(3 * 2.0**-24).to(dtype)
            row[col(7)] = torch.tensor(-(2.0**-24)).to(dtype)
            row[col(C - 1)] = torch.tensor(1023 * 2.0**-24).to(dtype)
        if r % 5 == 3:  # a peaky row
            row[col(r)] = torch.tensor(30.0).to(dtype)
    # the largest finite float16 (rounded to the type), once, in the last row: every other numerator of that
    # row underflows to 0
    rows[R - 1][col(C // 2)] = torch.tensor(65504.0).to(dtype)
    assert torch.isfinite(x.float()).all()
    return x.to(device)


def lay_out(x, layout):
    """The (T, N, C) tensor ``x`` as a view of the named layout holding the same values."""
    T, N, C = x.shape
    if layout == "contig":
        return x
    if layout == "transposed":
        return x.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    if layout == "offset":
        buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
        v = buf[1:].view(T, N, C)
        v.copy_(x)
        assert v.storage_offset() == 1
        return v
    if layout == "padded":
        buf = torch.zeros((T, N, C + 3), dtype=x.dtype, device=x.device)
        v = buf[..., :C]
        v.copy_(x)
        return v
    raise KeyError(layout)


def ctc_lens(T, N, device="cpu"):
    """Lengths with a 0 and a value above T; the last utterance (whose last frame holds the largest finite
    float16) runs to the end."""
    vals = [(0, T - 5, T // 2)[n % 3] for n in range(N)]
    vals[N - 1] = T + 3
    return torch.tensor(vals, dtype=torch.long, device=device)
