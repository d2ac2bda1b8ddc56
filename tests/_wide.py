"""Views whose element offsets leave 32 bits, laid out so that a wrapped offset stays in bounds.

A kernel that forms an address term in 32-bit arithmetic is wrong only once an element offset passes
2^31 or 2^32, and the rest of the suite stays far below that.  The tensors here reach it without the
memory traffic: ``wide_view`` places slice 1 of a two-slice dimension ``2^32 + A`` elements behind
slice 0 of one large, never-filled buffer, so only the two slices are touched.

The layout, in elements of the buffer (``A`` = dense extent of one slice, rounded up to 64)::

    [0, A)                     slice 0                      (true values)
    [A, 2 A)                   decoys                       (what a wrapped offset of slice 1 reads)
    [2^32 + A, 2^32 + 2 A)     slice 1                      (true values)

Every offset of slice 1 taken ``mod 2^32`` -- and the same offset formed with the wide stride cut to
``int`` -- falls into the decoy region, which holds finite values of the same kind as slice 1 but
different ones: a kernel with such a bug returns a deterministic wrong answer for slice 1 and never
leaves the buffer.  ``2 A <= 2^31`` keeps a sign-extended truncation in front of 2^31 as well.  These
properties are computed for every offset of every view and asserted (``check_layout``); they are the
condition under which such a test may run on a shared machine, not a measurement.

``LAYOUTS`` names every (dtype, shape, wide_dim) the GPU tests use; ``wide_case`` only builds views
listed there, and tests/test_wide_offsets_cpu.py checks each entry on ``meta`` tensors.
"""
import numpy as np
import torch

WRAP = 1 << 32
HALF = 1 << 31
MIN_NUMEL = WRAP + (1 << 23)  # elements a buffer must have (of the dtype under test)


def _prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


def wide_strides(shape, wide_dim):
    """(strides, A): row-major strides of the other dimensions, ``2^32 + A`` along ``wide_dim``."""
    shape = tuple(int(s) for s in shape)
    wide_dim = wide_dim % len(shape)
    if shape[wide_dim] != 2:
        raise ValueError("the wide dimension must have size 2, got {}".format(shape[wide_dim]))
    rest = [s for d, s in enumerate(shape) if d != wide_dim]
    A = max(64, -(-_prod(rest) // 64) * 64)
    dense, acc = [], 1
    for s in reversed(rest):
        dense.append(acc)
        acc *= s
    dense.reverse()
    strides = dense[:wide_dim] + [WRAP + A] + dense[wide_dim:]
    return tuple(strides), A


def offsets(shape, strides, storage_offset=0):
    """Every element offset of a view, as an int64 array of its shape (host arithmetic only)."""
    off = np.full((1,) * len(shape), int(storage_offset), dtype=np.int64)
    for d, (n, s) in enumerate(zip(shape, strides)):
        idx = np.arange(int(n), dtype=np.int64) * np.int64(s)
        off = off + idx.reshape([-1 if e == d else 1 for e in range(len(shape))])
    return np.broadcast_to(off, tuple(int(n) for n in shape))


def _int32(x):
    """x cut to 32 bits and sign-extended, as a C ``(int)`` cast does."""
    x = np.asarray(x, dtype=np.int64) & np.int64(WRAP - 1)
    return np.where(x >= HALF, x - WRAP, x)


def check_layout(shape, strides, wide_dim, numel):
    """Assert the three properties of the module docstring for a wide view; returns
    (offsets of slice 0, of slice 1, of the decoys)."""
    wide_dim = wide_dim % len(shape)
    off = offsets(shape, strides)
    s0 = np.take(off, 0, axis=wide_dim).ravel()
    s1 = np.take(off, 1, axis=wide_dim).ravel()
    assert off.min() >= 0 and off.max() < numel, (off.min(), off.max(), numel)
    assert s1.min() >= WRAP, "slice 1 must lie beyond 2^32 elements"
    wrapped = off % WRAP
    assert wrapped.max() < HALF, wrapped.max()
    # what a wide stride narrowed to int addresses, and every single term cut to 32 bits
    narrow = list(strides)
    narrow[wide_dim] = int(_int32(strides[wide_dim]))
    cut = np.take(offsets(shape, narrow), 1, axis=wide_dim).ravel()
    assert cut.min() >= 0 and cut.max() < HALF
    assert np.array_equal(_int32(s1), s1 % WRAP)  # sign- and zero-extension agree: below 2^31
    decoy = np.union1d(s1 % WRAP, cut)
    assert len(np.unique(s0)) == len(s0) and len(np.unique(s1)) == len(s1)
    assert not np.intersect1d(s0, s1).size
    assert not np.intersect1d(s0, decoy).size
    assert not np.intersect1d(s1, decoy).size
    assert decoy.max() < HALF and decoy.max() < numel
    return s0, s1, decoy


def decoys_like(values, seed=0):
    """Finite values of the same kind as ``values`` (same dtype, shape and range), but different."""
    g = torch.Generator().manual_seed(1234567 + seed)
    v = values.detach().cpu()
    if v.dtype == torch.bool:
        d = ~v
    elif v.dtype.is_floating_point:
        flat = v.reshape(-1)
        if flat.numel() > 1:
            # the same numbers in another order: sums and ranges of a row are kept, its places are not
            d = flat[torch.randperm(flat.numel(), generator=g)].reshape(v.shape)
            if torch.equal(d, v):
                d = flat.roll(1).reshape(v.shape)
        else:
            d = v * 0.5 + 0.125
    else:
        lo, hi = int(v.min()), int(v.max())
        d = torch.randint(lo, hi + 1, v.shape, generator=g, dtype=torch.int64).to(v.dtype)
        if hi > lo:
            d = torch.where(d == v, torch.where(v < hi, v + 1, torch.full_like(v, lo)), d)
        else:  # (one value only: nothing else of its range exists)
            d = v + 1
    assert d.dtype == v.dtype and d.shape == v.shape
    if v.dtype.is_floating_point:
        assert torch.isfinite(d).all() or not torch.isfinite(v).all()
    return d


def wide_view(buf, values, wide_dim, seed=0):
    """``buf.as_strided(...)`` holding ``values`` with a stride of ``2^32 + A`` along ``wide_dim`` (of
    size 2), decoys written where a 32-bit wrap of slice 1's offsets lands.  ``buf``: one-dimensional,
    of ``values.dtype``, at least MIN_NUMEL elements; a ``meta`` buffer gives the view without writes."""
    assert buf.dim() == 1 and buf.dtype == values.dtype, (buf.dtype, values.dtype)
    assert buf.numel() >= MIN_NUMEL, buf.numel()
    shape = tuple(values.shape)
    wide_dim = wide_dim % len(shape)
    strides, A = wide_strides(shape, wide_dim)
    check_layout(shape, strides, wide_dim, buf.numel())
    view = buf.as_strided(shape, strides)
    if buf.device.type == "meta":
        return view
    narrow = list(strides)
    narrow[wide_dim] = A  # (int)(2^32 + A) == (2^32 + A) mod 2^32 == A
    decoy_view = buf.as_strided(shape, narrow).select(wide_dim, 1)
    truth = values.detach().select(wide_dim, 1)
    decoy = decoys_like(truth, seed)
    if truth.numel() > 1 or truth.dtype != torch.bool:
        assert not torch.equal(decoy, truth.cpu()), "decoys must differ from slice 1"
    decoy_view.copy_(decoy.to(buf.device))
    view.copy_(values.detach().to(buf.device))
    # the writes themselves pass 2^32: read them back through the same views
    assert torch.equal(view, values.detach().to(buf.device))
    assert torch.equal(decoy_view, decoy.to(buf.device))
    return view


def dense_at_2_31(buf, shape):
    """A contiguous view of ``shape`` that starts at element 2^31 of ``buf``: a sign-extended wrap of an
    offset in [2^31, 2^31 + d) lands at the front of the buffer, not in front of the allocation."""
    shape = tuple(int(s) for s in shape)
    n = _prod(shape)
    assert buf.dim() == 1 and HALF + n <= buf.numel(), (n, buf.numel())
    dense, acc = [], 1
    for s in reversed(shape):
        dense.append(acc)
        acc *= s
    return buf.as_strided(shape, tuple(reversed(dense)), HALF)


# ---- the case table ------------------------------------------------------------------------------
# name -> (dtype, shape, wide_dim).  Every wide view of tests/test_wide_offsets_gpu.py is built through
# ``wide_case`` from an entry of this table; tests/test_wide_offsets_cpu.py checks every entry.
LAYOUTS = {}


def _layout(name, dtype, shape, wide_dim):
    assert name not in LAYOUTS, name
    LAYOUTS[name] = (dtype, tuple(shape), wide_dim)
    return name


def wide_case(buf, name, values, seed=0):
    """``wide_view`` for the entry ``name`` of LAYOUTS; ``values`` must have its dtype and shape."""
    dtype, shape, wide_dim = LAYOUTS[name]
    assert values.dtype == dtype and tuple(values.shape) == shape, (name, values.dtype, tuple(values.shape))
    return wide_view(buf if buf.dtype == dtype else buf.view(dtype), values, wide_dim, seed)


f32, f64, i64 = torch.float32, torch.float64, torch.int64

# ctc_greedy_search: logits (T, N, V); wide batch stride (N = 2) and wide frame stride (T = 2)
for _V in (65, 1100):
    _layout("greedy_sn_V%d" % _V, f32, (20, 2, _V), 1)
    _layout("greedy_st_V%d" % _V, f32, (2, 3, _V), 0)
# ctc_prefix_search: logits (T, N, V + 1); general kernel (V = 70), long rows (V = 513: registers / LDS
# ring), the wide-beam kernel (V = 70, width 40), the V = 256, W = 16 instance (lg_sn == 257: frames only)
for _V in (70, 513):
    _layout("ctc_sn_V%d" % _V, f32, (9, 2, _V + 1), 1)
    _layout("ctc_st_V%d" % _V, f32, (2, 3, _V + 1), 0)
_layout("ctc_default_st", f32, (2, 3, 257), 0)
# the searches with an n-gram model in the loop (V = 65: tests/_lm_forms.py inst_V65_K32)
_layout("ctc_lm_sn", f32, (12, 2, 66), 1)
_layout("ctc_lm_st", f32, (2, 5, 66), 0)
# step operators: scores (N, K', V) / (N, V) with a wide batch stride
for _Kp in (1, 3, 9, 17):
    _layout("step_ext_Kp%d" % _Kp, f32, (2, _Kp, 70), 0)
for _V in (64, 1000):
    _layout("walk_V%d" % _V, f32, (2, _V), 0)
# string operators: tokens (L, N) or, batch first, (N, L), int64
for _L in (29, 137, 150, 600, 2049):
    _layout("tok_L%d" % _L, i64, (_L, 2), 1)
    _layout("tok_bf_L%d" % _L, i64, (2, _L), 0)
# hard-OCD loss: logits (H, N, V)
for _V in (65, 1100):
    _layout("ocd_V%d" % _V, f32, (5, 2, _V), 1)
# estimators, returns: matrices (M, B) / (T, N) with either stride wide, float32 and float64
for _dt, _tag in ((f32, "f32"), (f64, "f64")):
    _layout("mat_%s_7x2_d1" % _tag, _dt, (7, 2), 1)
    _layout("mat_%s_65x2_d1" % _tag, _dt, (65, 2), 1)
    _layout("mat_%s_2x65_d0" % _tag, _dt, (2, 65), 0)
# pad_masked_sequence / chunk_by_slices: x (N, T, F) or (T, N, F), rows of 16-byte words (F = 8) and of
# elements (F = 3); the mask (N, T) / (T, N) of bool bytes
for _F in (8, 3):
    _layout("seq_2x37x%d_d0" % _F, f32, (2, 37, _F), 0)
    _layout("seq_37x2x%d_d1" % _F, f32, (37, 2, _F), 1)
_layout("mask_2x37_d0", torch.bool, (2, 37), 0)
_layout("mask_37x2_d1", torch.bool, (37, 2), 1)
# spec_augment_apply_parameters: feats (N, T, F); the relaxed samplers: parameter rows (B, V)
_layout("spec_2x50x10_d0", f32, (2, 50, 10), 0)
_layout("spec_2x50x12_d0", f32, (2, 50, 12), 0)
_layout("mat_f32_2x70_d0", f32, (2, 70), 0)
_layout("mat_f64_2x70_d0", f64, (2, 70), 0)
# feat_deltas: x (N, T, D), the collapsed outermost stride wide; soft attention: query (N, K, D), key and
# value (T, N, 1, D) with the batch stride wide
_layout("feat_2x40x260_d0", f32, (2, 40, 260), 0)
_layout("attn_q_2x3x16_d0", f32, (2, 3, 16), 0)
_layout("attn_kv_40x2x1x16_d1", f32, (40, 2, 1, 16), 1)


# ---- dense tensors just over 2^31 elements ---------------------------------------------------------
# name -> (dtype, shape): contiguous inputs that start at element 2^31 of the buffer (dense_at_2_31)
ROW = 1023  # bytes per step of the uint8 cases: no multiple of 16, so the copy kernels move single bytes
GUARD = (1 << 32) - 4096  # elements the 32-bit index of csrc/pad_variable.hip and csrc/seq_chunk.hip holds
STEPS_MAX = (GUARD - 1) // ROW  # the longest output those kernels take: just under 2^32 bytes
DENSE = {
    "slp_logits": (f32, (512, 4096, 1025)),        # sequence_log_probs: (T, N, V)
    "ocd_logits": (f32, (8, 262144, 1025)),        # hard-OCD loss: (H, N, V)
    "mc_f": (f32, (64, (1 << 25) + (1 << 14))),    # mc_reduce MEAN: (M, B)
    "gumbel_logits": (f32, (2095200, 1025)),       # relaxed Gumbel rsample: (B, V)
    "u8_masked": (torch.uint8, (2, STEPS_MAX // 2, ROW)),  # pad_masked_sequence: (N, T, F) bytes
}


def dense_case(buf, name):
    dtype, shape = DENSE[name]
    assert _prod(shape) > HALF
    return dense_at_2_31(buf if buf.dtype == dtype else buf.view(dtype), shape)


def rows_around(shape_rows, row_elems, count=16, seed=0):
    """``count`` row indices of a dense (rows, row_elems) tensor: row 0, the rows on both sides of element
    2^31, the last row and random others, sorted."""
    edge = HALF // row_elems
    assert 0 < edge < shape_rows - 1
    picked = {0, edge - 1, edge, edge + 1, shape_rows - 1}
    rng = np.random.default_rng(seed)
    while len(picked) < count:
        picked.add(int(rng.integers(0, shape_rows)))
    return sorted(picked)
