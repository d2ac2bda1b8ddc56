"""Inputs of tests/test_fill_forms_gpu.py: token tensors whose first eos along the walked axis sits exactly where
the case says, for every launch form of csrc/fill_after_eos.hip.  Conditions on them that need no GPU are in
tests/test_fill_forms_cpu.py.

The kernels' geometry, restated from the header comment of fill_after_eos.hip (the tensor is (outer, L, inner)
around the walked axis):

* ``inner == 1``, the rows kernel: one wave per sequence, four sequences per workgroup.  A pass covers 512
  positions as eight sub-blocks of 64 (one position per lane); the first eos of a sub-block is found by a ballot
  and "an eos was seen" is carried into the later sub-blocks and passes.
* ``inner > 1``, the columns kernel: a workgroup owns 64 consecutive columns of the flattened (outer, inner) and
  has nw waves, nw = 1 doubling while ``nw < 16 and nw * 8 < L``.  Wave w takes the rows w, w + nw, ..., eight of
  them (slots 0..7) per pass, so a pass covers 8 nw rows; the first eos of a column is the minimum over the waves.
"""
import itertools
from collections import namedtuple

import numpy as np

import oracle

NONE = -1  # "no eos in this sequence"

ROWS_L = (1, 63, 64, 65, 511, 512, 513, 1024, 1025, 1500)
ROWS_OUTER = (1, 3, 4, 5, 9)
ROWS_FIXED = ("none", 0, 63, 64, 511, 512, "last")

COLS_L = (2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300)
COLS_INNER = (2, 63, 64, 65, 130)
COLS_OUTER = (1, 3)

ROWS_PASS = 512
SUB_BLOCK = 64
ROWS_PER_GROUP = 4
COLS_PER_GROUP = 64

# (numpy bit type, torch dtype names of that width); bfloat16 has no numpy type: its words are built as int16
WIDTHS = {
    1: (np.uint8, ("bool", "uint8")),
    2: (np.int16, ("int16", "float16", "bfloat16")),
    4: (np.int32, ("int32", "float32")),
    8: (np.int64, ("int64", "float64")),
}
# fill values whose bit pattern matters, with the bits each must leave in the output (two's complement for the
# negative integers; sign bit only for -0.0; the quiet NaN torch.full writes)
FILLS = {
    "bool": [(1.0, 1)],
    "uint8": [(200.0, 200)],
    "int16": [(-12345.0, -12345)],
    "int32": [(-7.0, -7)],
    "int64": [(-(2.0**40) - 3.0, -(2**40) - 3)],
    "float16": [(-0.0, -(2**15)), (float("nan"), 0x7E00), (-7.5, 0xC780 - (1 << 16))],
    "bfloat16": [(-0.0, -(2**15)), (float("nan"), 0x7FC0), (-7.5, 0xC0F0 - (1 << 16))],
    "float32": [(-0.0, -(2**31)), (float("nan"), 0x7FC00000), (-7.5, 0xC0F00000 - (1 << 32))],
    "float64": [(-0.0, -(2**63)), (float("nan"), 0x7FF8 << 48), (-7.5, (0xC01E << 48) - (1 << 64))],
}
DTYPES = tuple(FILLS)


def width_of(dtype_name):
    return next(w for w, (_, names) in WIDTHS.items() if dtype_name in names)


# ---- geometry ------------------------------------------------------------------------------------------------


def rows_place(pos):
    """(pass, sub-block, lane) of position ``pos`` in the rows kernel."""
    return pos // ROWS_PASS, (pos % ROWS_PASS) // SUB_BLOCK, pos % SUB_BLOCK


def cols_waves(L):
    nw = 1
    while nw < 16 and nw * 8 < L:
        nw *= 2
    return nw


def cols_place(L, pos):
    """(pass, wave, slot) of row ``pos`` in the columns kernel's launch for sequence length L."""
    nw = cols_waves(L)
    return pos // (8 * nw), pos % nw, (pos // nw) % 8


def pass_length(L, inner):
    return ROWS_PASS if inner == 1 else 8 * cols_waves(L)


# ---- where the first eos goes ----------------------------------------------------------------------------------


def _seed(*key):
    return [int(k) for k in key]


def rows_rounds(L, outer):
    """The launches of the rows kernel at (outer, L): a list of (outer,) arrays of first-eos positions (NONE: no
    eos).  The fixed positions that exist at this L (none, 0, 63, 64, 511, 512, L - 1) are dealt over the
    sequences and rotated by one from round to round, so every sequence -- every wave of a workgroup that the
    batch has -- meets every one of them; the last round is one random interior position per sequence."""
    fixed = []
    for p in ROWS_FIXED:
        p = NONE if p == "none" else (L - 1 if p == "last" else p)
        if p < L and p not in fixed:
            fixed.append(p)
    rounds = [np.array([fixed[(r + i) % len(fixed)] for i in range(outer)], np.int64) for r in range(len(fixed))]
    rng = np.random.default_rng(_seed(1, L, outer))
    rounds.append(rng.integers(1, L - 1, outer) if L > 2 else np.zeros(outer, np.int64))
    return rounds


def cols_positions(L, inner, outer):
    """(outer, inner) first-eos positions of the columns kernel's case: none, 0 and L - 1, then every column its
    own position: a random permutation of the rows dealt over the columns (drawn again once it runs out), so
    that the columns of a workgroup end in different waves, slots and passes; the last column ends at L - 1."""
    n = outer * inner
    rng = np.random.default_rng(_seed(2, L, inner, outer))
    pos = rng.permutation(L)[np.arange(n) % L]
    if n > L:  # more columns than rows: the second time round in another order
        pos[L:] = rng.integers(0, L, n - L)
    pos[0] = NONE
    if n > 1:
        pos[1] = 0
    if n > 2:
        pos[2] = L - 1
    pos[n - 1] = L - 1 if n > 3 else pos[n - 1]  # (the last live column of the last workgroup)
    return pos.reshape(outer, inner).astype(np.int64)


# ---- tokens ----------------------------------------------------------------------------------------------------

ALPHABET = (0, 1, 2, 3, 4)
EOS = 2
INT64_ENDS = (2**63 - 1, -(2**63), 0, 5, -1)


def build_tokens(first, L, eos=EOS, alphabet=ALPHABET, seed=0):
    """(outer, L, inner) int64 tokens whose first ``eos`` along axis 1 is at ``first[o, i]`` (NONE: nowhere).

    Before that position the tokens are drawn from the alphabet without eos.  After it they are drawn from all of
    it in two sequences of three (eos included: later eos tokens, one in five) and from the alphabet without eos
    in the third, where only what the kernel remembers of the first eos fills the rest.  Where the tokens are
    free, an eos is also put at the first position of the next pass, which lies in an earlier sub-block (rows
    kernel) or belongs to an earlier slot of wave 0 (columns kernel) than the first eos may: "first" has to mean
    the position, not the order in which the waves and sub-blocks come by."""
    first = np.asarray(first, np.int64)
    outer, inner = first.shape
    rng = np.random.default_rng(_seed(3, L, inner, outer, seed))
    alphabet = np.asarray(alphabet, np.int64)
    others = alphabet[alphabet != eos]
    tok = rng.choice(others, (outer, L, inner))
    free = rng.choice(alphabet, (outer, L, inner))
    pos = np.arange(L).reshape(1, L, 1)
    f = first[:, None, :]
    sparse = (np.arange(outer * inner).reshape(outer, 1, inner) % 3) == 2
    after = (f != NONE) & (pos > f)
    tok = np.where(after & ~sparse, free, tok)
    plen = pass_length(L, inner)
    late = (f // plen + 1) * plen
    tok = np.where(after & ~sparse & (pos == late), eos, tok)
    tok = np.where(pos == f, eos, tok)
    return tok


def first_eos(tok, eos):
    """The planted positions read back from the tokens ((outer, inner); NONE where there is none)."""
    hit = tok == eos
    return np.where(hit.any(1), hit.argmax(1), NONE)


def keep_mask(tok, eos):
    """The oracle's keep-mask: True where fill_after_eos leaves the value."""
    return oracle.fill_after_eos(tok, eos, 1, 0.0, np.ones(tok.shape, np.uint8)).astype(bool)


def value_bits(shape, dtype_name, seed=0):
    """Random words of the dtype's width (every bit pattern; 0 / 1 for bool), as the numpy integer type of that
    width."""
    rng = np.random.default_rng(_seed(4, seed, *shape))
    np_bits = WIDTHS[width_of(dtype_name)][0]
    if dtype_name == "bool":
        return rng.integers(0, 2, shape).astype(np_bits)
    info = np.iinfo(np_bits)
    return rng.integers(info.min, info.max, shape, dtype=np_bits, endpoint=True)


def expected_bits(tok, eos, vbits, fill_bits):
    return np.where(keep_mask(tok, eos), vbits, np.array(fill_bits, dtype=vbits.dtype))


Case = namedtuple("Case", "kernel outer L inner first")


def rows_cases(L):
    return [Case("rows", outer, L, 1, r.reshape(outer, 1)) for outer in ROWS_OUTER for r in rows_rounds(L, outer)]


def cols_cases(L):
    return [Case("cols", outer, L, inner, cols_positions(L, inner, outer))
            for inner, outer in itertools.product(COLS_INNER, COLS_OUTER)]  # fmt: skip


# the shapes of the dtype sweep and of the other cases: on every side of a pass and of a workgroup
DTYPE_ROWS = [(5, 65), (5, 513), (3, 1500)]
DTYPE_COLS = [(3, 9, 65), (1, 129, 130), (3, 300, 63)]
LONG_ROWS = (5, 1025)
LONG_COLS = (3, 300, 65)


def shape_cases(shape):
    if len(shape) == 2:
        return [Case("rows", shape[0], shape[1], 1, r.reshape(-1, 1)) for r in rows_rounds(shape[1], shape[0])]
    outer, L, inner = shape
    return [Case("cols", outer, L, inner, cols_positions(L, inner, outer))]
