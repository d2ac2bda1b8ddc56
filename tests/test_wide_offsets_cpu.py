"""CPU: the arithmetic of tests/_wide.py for every layout the GPU tests use, and the size guards.

Every entry of ``_wide.LAYOUTS`` -- the only layouts tests/test_wide_offsets_gpu.py can build -- is laid
out on a ``meta`` buffer and its offsets are checked here a second time, in closed form: in bounds, below
2^31 after a 32-bit wrap, slice 0, slice 1 and the decoys pairwise disjoint.  The writes are checked on a
small real buffer with the wrap point moved down.  The over-the-limit calls return PDT_E_TOO_LONG before
any launch (tests/test_cabi.py relies on the same), so they run without a GPU.
"""
import os

import numpy as np
import pytest
import torch

import _wide as W


@pytest.mark.parametrize("name", sorted(W.LAYOUTS))
def test_layout_stays_in_bounds_when_an_offset_wraps(name):
    dtype, shape, wide_dim = W.LAYOUTS[name]
    buf = torch.empty(W.MIN_NUMEL, dtype=dtype, device="meta")
    view = W.wide_view(buf, torch.empty(shape, dtype=dtype, device="meta"), wide_dim)
    assert view.device.type == "meta" and tuple(view.shape) == shape and view.storage_offset() == 0
    strides = view.stride()
    assert shape[wide_dim] == 2
    rest = int(np.prod([s for d, s in enumerate(shape) if d != wide_dim]))
    A = strides[wide_dim] - W.WRAP
    assert A % 64 == 0 and rest <= A < rest + 64 + 64
    # closed form: the other dimensions are dense, so a slice spans [base, base + rest)
    span = sum((n - 1) * s for d, (n, s) in enumerate(zip(shape, strides)) if d != wide_dim) + 1
    assert span == rest
    slice0, decoys, slice1 = (0, rest), (A, A + rest), (W.WRAP + A, W.WRAP + A + rest)
    assert slice0[1] <= decoys[0] and decoys[1] <= W.HALF < W.WRAP <= slice1[0]
    assert slice1[1] <= buf.numel()
    assert (slice1[0] % W.WRAP, (slice1[1] - 1) % W.WRAP + 1) == decoys
    assert int(np.int32(np.int64(strides[wide_dim]) & 0x7FFFFFFF)) == A  # the stride as an int
    # ... and offset by offset (what wide_view asserted already, from its own return value)
    s0, s1, dec = W.check_layout(shape, strides, wide_dim, buf.numel())
    assert (s0.min(), s0.max() + 1) == slice0 and (s1.min(), s1.max() + 1) == slice1
    assert (dec.min(), dec.max() + 1) == decoys and len(dec) == rest
    assert (W.offsets(shape, strides) % W.WRAP).max() < W.HALF


def test_layouts_cover_both_buffer_widths():
    sizes = {torch.empty((), dtype=d).element_size() for d, _, _ in W.LAYOUTS.values()}
    assert sizes >= {4, 8}


def test_check_layout_refuses_what_would_leave_the_buffer():
    shape, (strides, A) = (3, 2, 5), W.wide_strides((3, 2, 5), 1)
    W.check_layout(shape, strides, 1, W.MIN_NUMEL)
    with pytest.raises(AssertionError):  # too small a buffer
        W.check_layout(shape, strides, 1, W.WRAP)
    with pytest.raises(AssertionError):  # a stride whose wrap lands in [2^31, 2^32)
        W.check_layout(shape, (5, W.WRAP + W.HALF, 1), 1, 3 * W.WRAP)
    with pytest.raises(AssertionError):  # decoys on top of slice 0
        W.check_layout(shape, (5, W.WRAP, 1), 1, 3 * W.WRAP)
    with pytest.raises(ValueError):
        W.wide_strides((3, 4, 5), 1)
    big = (2, 2048)  # slice 1 ends beyond the buffer
    with pytest.raises(AssertionError):
        W.check_layout(big, W.wide_strides(big, 0)[0], 0, W.WRAP + 2048 + 1000)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64, torch.bool])
def test_writes_land_where_a_wrapped_read_looks(monkeypatch, dtype):
    """The real writes, on the CPU, with the wrap point at 2^16 instead of 2^32: reading slice 1 through
    offsets taken mod the wrap point, or through the stride cut to that many bits, returns the decoys."""
    monkeypatch.setattr(W, "WRAP", 1 << 16)
    monkeypatch.setattr(W, "HALF", 1 << 15)
    monkeypatch.setattr(W, "MIN_NUMEL", (1 << 16) + (1 << 10))
    torch.manual_seed(0)
    for shape, wide_dim in (((7, 2, 13), 1), ((2, 5, 9), 0), ((33, 2), 1), ((2,), 0)):
        if dtype == torch.float32:
            values = torch.randn(shape)
        elif dtype == torch.int64:
            values = torch.randint(0, 6, shape)
        else:
            values = torch.rand(shape) < 0.5
        buf = torch.full((W.MIN_NUMEL,), 0, dtype=dtype)
        view = W.wide_view(buf, values, wide_dim)
        assert torch.equal(view, values) and view.stride(wide_dim) > W.WRAP
        strides = list(view.stride())
        strides[wide_dim] %= W.WRAP
        wrapped = buf.as_strided(shape, strides)
        assert torch.equal(wrapped.select(wide_dim, 0), values.select(wide_dim, 0))
        got, truth = wrapped.select(wide_dim, 1), values.select(wide_dim, 1)
        assert not torch.equal(got, truth)
        assert torch.equal(got, W.decoys_like(truth))
        if dtype == torch.float32:
            assert torch.isfinite(got).all()
            assert torch.equal(got.flatten().sort()[0], truth.flatten().sort()[0]) or truth.numel() == 1
        elif dtype == torch.int64:
            assert (got != truth).all() and (truth.numel() == 1 or (got.min() >= truth.min() and got.max() <= truth.max()))


def test_dense_at_2_31():
    buf = torch.empty(W.MIN_NUMEL, dtype=torch.float32, device="meta")
    rows = (W.HALF + 4096) // 1025 + 1
    for shape in ((rows, 1025), (3, 5, 7), (W.HALF + (1 << 23),)):
        v = W.dense_at_2_31(buf, shape)
        assert v.is_contiguous() and v.storage_offset() == W.HALF and tuple(v.shape) == shape
        assert v.storage_offset() + v.numel() <= buf.numel()
    with pytest.raises(AssertionError):
        W.dense_at_2_31(buf, (W.HALF + (1 << 23) + 1,))
    # narrower types reinterpret the buffer: four times the elements
    assert W.dense_at_2_31(buf.view(torch.uint8), (W.WRAP - 4097,)).numel() > W.HALF


# ---- size guards: one step over the limit returns PDT_E_TOO_LONG before any launch ---------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    from pydrobert_amd import _cabi

    if not os.path.exists(_cabi.LIB_PATH):
        g.build()
    return _cabi.lib()


P = 4096  # a non-null "pointer": these calls return before anything reads it


def test_vocabulary_guards_of_the_sequence_operators(lib):
    """V is an ``int`` in the kernels of csrc/seq_ops.hip: V >= 2^30 is refused."""
    from pydrobert_amd import _cabi

    big = 1 << 30
    assert lib.pdt_ctc_greedy_search(P, 4, 2, big, big * 2, big, 1, 0, 0, 0, P, P, 2, 1, P, 0) == _cabi.PDT_E_TOO_LONG
    assert lib.pdt_sequence_log_probs_forward(P, P, 2, 3, 2, big, 0, 0, P, 0) == _cabi.PDT_E_TOO_LONG
    assert lib.pdt_sequence_log_probs_backward(P, P, 2, 3, 2, big, 0, 0, P, P, 0) == _cabi.PDT_E_TOO_LONG
    # the guards that were there: batch and step counts
    assert lib.pdt_ctc_greedy_search(P, 4, 1 << 31, 9, 9, 36, 1, 0, 0, 0, P, P, 2, 1, P, 0) == _cabi.PDT_E_TOO_LONG
    assert lib.pdt_ctc_greedy_search(P, 1 << 20, 2, 9, 18, 9, 1, 0, 0, 0, P, P, 2, 1, P, 0) == _cabi.PDT_E_TOO_LONG
    assert lib.pdt_sequence_log_probs_forward(P, P, 1 << 16, 3, 1 << 15, 9, 0, 0, P, 0) == _cabi.PDT_E_TOO_LONG
    assert lib.pdt_sequence_log_probs_backward(P, P, 2, 1 << 31, 2, 9, 0, 0, P, P, 0) == _cabi.PDT_E_TOO_LONG


def test_search_guards(lib):
    from pydrobert_amd import _cabi

    E = _cabi.PDT_E_TOO_LONG
    # T * width >= 2^31, V >= 2^30, T >= 2^24
    assert lib.pdt_ctc_prefix_search(P, 1 << 24, 2, 30, 62, 31, 1, 0, 16, 5, P, P, P, P, 0) == E
    assert lib.pdt_ctc_prefix_search(P, 5, 2, 1 << 30, 1 << 31, 1 << 30, 1, 0, 16, 5, P, P, P, P, 0) == E
    assert lib.pdt_ctc_prefix_search(P, 5, 1 << 31, 30, 1 << 36, 31, 1, 0, 16, 5, P, P, P, P, 0) == E
    assert lib.pdt_ctc_prefix_search_wide(P, 1 << 24, 2, 30, 62, 31, 1, 0, 40, 5, P, P, P, P, 0) == E
    assert lib.pdt_ctc_prefix_search_wide(P, 5, 2, 1 << 25, 1 << 26, 1 << 25, 1, 0, 100, 5, P, P, P, P, 0) == E


@pytest.mark.parametrize("name", sorted(W.DENSE))
def test_dense_cases_pass_2_31_inside_the_buffer(name):
    dtype, shape = W.DENSE[name]
    # (the 4-byte buffer, reinterpreted for narrower types, as the GPU fixture holds it)
    buf = torch.empty(W.MIN_NUMEL, dtype=torch.int32 if dtype == torch.uint8 else dtype, device="meta")
    v = W.dense_case(buf, name)
    buf = buf if buf.dtype == dtype else buf.view(dtype)
    assert v.is_contiguous() and v.storage_offset() == W.HALF
    assert W.HALF < v.numel() and v.storage_offset() + v.numel() <= buf.numel()
    # a sign-extended 32-bit wrap of an offset in [2^31, numel) lands in [0, numel - 2^31) of the view's own
    # storage offset: inside the buffer, in front of the view
    assert v.numel() - W.HALF <= W.HALF
    assert v.dtype == dtype
    if name == "mc_f":  # (sampled by column: the one whose last sample lies at element 2^31)
        M, B = shape
        assert 0 < W.HALF - (M - 1) * B < B - 1
        return
    if name == "u8_masked":  # (every row is compared; sequence 1 starts just under byte 2^31)
        assert v.numel() < W.GUARD and shape[1] * shape[2] < W.HALF < 2 * shape[1] * shape[2]
        return
    rows = W.rows_around(int(np.prod(shape[:-1])), shape[-1])
    assert len(rows) == 16 and rows[0] == 0 and rows[-1] == int(np.prod(shape[:-1])) - 1
    edge = W.HALF // shape[-1]
    assert edge * shape[-1] <= W.HALF < (edge + 1) * shape[-1] and {edge - 1, edge, edge + 1} <= set(rows)


def test_copy_kernel_guards(lib):
    """csrc/pad_variable.hip and csrc/seq_chunk.hip number their output elements with an ``unsigned`` and keep
    their sizes as ``int``: an output of 2^32 - 4096 elements or more, and any size beyond 2^31 - 1, is refused."""
    from pydrobert_amd import _cabi

    E = _cabi.PDT_E_TOO_LONG
    row, guard = 1023, (1 << 32) - 4096
    over = (guard - 1) // row + 1  # the first step count whose output reaches the guard
    assert (over - 1) * row < guard <= over * row
    big = 1 << 31
    # pdt_pad_variable(x, N, T, F, elem_bytes, lens, pad, mode, fill, Tp, out, stream)
    assert lib.pdt_pad_variable(P, 1, 16, row, 1, P, P, 2, P, over, P, 0) == E
    assert lib.pdt_pad_variable(P, big, 1, 1, 1, P, P, 0, P, 1, P, 0) == E
    assert lib.pdt_pad_variable(P, 1, big, 1, 1, P, P, 0, P, 4, P, 0) == E
    # pdt_pad_variable_backward(grad_out, dtype, N, T, F, lens, pad, mode, Tp, grad_x, stream)
    assert lib.pdt_pad_variable_backward(P, 0, 1, over, row, P, P, 0, 8, P, 0) == E
    assert lib.pdt_pad_variable_backward(P, 0, 1, 4, 1, P, P, 0, big, P, 0) == E
    # pdt_gather_steps(x, N, T, F, elem_bytes, x_sn, x_st, map, m_sn, m_st, To, time_major, fill, out, stream)
    assert lib.pdt_gather_steps(P, 1, 16, row, 1, 16 * row, row, P, over, 1, over, 0, P, P, 0) == E
    assert lib.pdt_gather_steps(P, 1, big, 1, 1, big, 1, P, 4, 1, 4, 0, P, P, 0) == E
    # pdt_chunk_by_slices(x, N, T, F, elem_bytes, x_sn, x_st, slices, lens, mode, fill, Tp, out, stream)
    assert lib.pdt_chunk_by_slices(P, 1, 16, row, 1, 16 * row, row, P, P, 2, P, over, P, 0) == E
    assert lib.pdt_chunk_by_slices(P, 1, big, 1, 1, big, 1, P, P, 0, P, 4, P, 0) == E
    # pdt_chunk_by_slices_backward(grad_out, dtype, N, T, F, slices, lens, mode, Tp, grad_x, stream)
    assert lib.pdt_chunk_by_slices_backward(P, 0, 1, over, row, P, P, 0, 8, P, 0) == E
    assert lib.pdt_chunk_by_slices_backward(P, 0, 1, 8, row, P, P, 0, over, P, 0) == E
    assert lib.pdt_chunk_by_slices_backward(P, 0, 1, 1, 1, P, P, 0, big, P, 0) == E
    # pdt_compact_mask(mask, N, T, m_sn, m_st, src, rank, o_sn, o_st, counts, stream)
    assert lib.pdt_compact_mask(P, 1, big - 256, big, 1, P, 0, big, 1, P, 0) == E
    assert lib.pdt_compact_mask(P, big, 4, 4, 1, P, 0, 4, 1, P, 0) == E
    # pdt_chunk_stats(slices, lens, N, T, chunk_lens, stats, stream)
    assert lib.pdt_chunk_stats(P, P, big, 4, P, P, 0) == E


def test_loss_and_estimator_guards(lib):
    from pydrobert_amd import _cabi

    E = _cabi.PDT_E_TOO_LONG
    big = 1 << 31
    # pdt_ocd_loss_forward(logits, H, N, V, lg_sh, lg_sn, lg_sv, bitmask, class_tokens, R, weight, ignore, loss, count, status, stream)
    assert lib.pdt_ocd_loss_forward(P, 2, 2, big, 2 * big, big, 1, P, P, 4, 0, -2, P, P, 0, 0) == E
    assert lib.pdt_ocd_loss_forward(P, 1 << 17, 1 << 16, 9, 9 << 16, 9, 1, P, P, 4, 0, -2, P, P, 0, 0) == E
    # pdt_ocd_loss_backward(..., grad_loss, grad_logits, stream)
    assert lib.pdt_ocd_loss_backward(P, 2, 2, big, 2 * big, big, 1, P, P, 4, 0, -2, P, P, 0) == E
    # pdt_imh_chain(dtype, ratio, r_sm, r_sb, ratio0, r0_s, log_u, u_sm, u_sb, M, B, idx, last, last_idx, stream)
    assert lib.pdt_imh_chain(0, P, 2, 1, P, 1, P, 2, 1, big, 2, P, P, P, 0) == E


# ---- every PDT_E_TOO_LONG guard of DESIGN.md section 10, one over-the-limit call each ------------------
# (label, entry point, arguments).  The pointers are never read: each call returns from the guard the label
# names, before any launch.  Arrays the host does read (gamma, the estimators' pointer and stride lists, the
# attention descriptor) are real.
import ctypes  # noqa: E402

B28, B30, B31 = (1 << 28) + 1, 1 << 30, 1 << 31
gam = ctypes.c_double(0.9)
G = ctypes.addressof(gam)
ins = (ctypes.c_void_p * 6)(P, None, None, None, None, None)  # the estimators' inputs: f alone
IN = ctypes.addressof(ins)
st = (ctypes.c_int64 * 12)(*([1, 1] * 6))
ST = ctypes.addressof(st)
gr = (ctypes.c_void_p * 6)(P, None, None, None, None, None)
GR = ctypes.addressof(gr)
lev_tail = (0, 0, 0, 1.0, 1.0, 1.0, 0, 0, 0, 0.0, 0, P, 0, 1, 0, 0, 0, 0, 0, 0)  # has_eos .. stream of pdt_lev
adv_out = (P,) * 8 + (0,)  # the eight outputs of a CTC step and the stream




def ctc_adv(N, Kp, V, W, S=3):
    return (P,Kp*V,V,1, P,V,1, P,1, N,Kp,V,W, P,Kp,1, P,Kp,1, P,S,N*Kp,Kp,1, P,Kp,1, P,Kp,1, P,Kp*Kp,Kp,1)+adv_out


def ctc_adv_lm(N, Kp, V, W, S=3):
    return (P,0.3,0, P,V,1, P,1, N,Kp,V,W, P,Kp,1, P,Kp,1, P,S,N*Kp,Kp,1, P,Kp,1, P,Kp,1, P,Kp*Kp,Kp,1)+adv_out


def beam_adv(N, Kp, V, W, S=3):
    return (P,Kp*V,V,1, N,Kp,V,W, P,Kp,1, P,S,N*Kp,Kp,1, P,Kp,1, S+1, P,P,P,P,0)


def beam_step(N, Kp, V, W, S=3):
    return (P,Kp*V,V,1, N,Kp,V,W, P,Kp,1, P,S,N*Kp,Kp,1, P,Kp,1, 0,0,0,0, P,P,P,P,P,P,0)


def beam_step_table(N, Kp, V, W, S=3):
    return (P,V,1,5,P,P, N,Kp,V,W, P,Kp,1, P,S,N*Kp,Kp,1, P,Kp,1, 0,0,0,0, P,P,P,P,P,P,0)


# attention descriptors (include/pdt_amd.h): one row dim of 2^40 rows; the pool form has D = 0
desc = (ctypes.c_int64 * 87)()
desc[0:8] = [1, 1 << 40, 1 << 40, 1, 4, 4, 4, 1 << 40]
D = ctypes.addressof(desc)
desc2 = (ctypes.c_int64 * 87)(*list(desc))
desc2[5] = 0
D2 = ctypes.addressof(desc2)
# fmt: off
GUARD_CALLS = [
 ("lev R", "pdt_lev", (P,B28,1,1,P,5,1,1,2)+lev_tail),
 ("lev H", "pdt_lev", (P,5,1,1,P,B28,1,1,2)+lev_tail),
 ("lev N", "pdt_lev", (P,5,1,1,P,5,1,1,B31)+lev_tail),
 ("lev_keep", "pdt_lev_keep", (P,B28,1,1,P,5,1,1,2)+lev_tail),
 ("lev_classified", "pdt_lev_classified", (P,B28,1,1,P,5,1,1,2)+lev_tail),
 ("oc_mask", "pdt_oc_mask", (P,5,1,1,P,B28,1,1,2,0,0,0,1.,1.,1.,0,P,P,P,0,0,0,0)),
 ("fill outer", "pdt_fill_after_eos", (P,1<<34,4,1,0,P,4,0,P,0)),
 ("fill L", "pdt_fill_after_eos", (P,2,B31,2,0,P,4,0,P,0)),
 ("ctc_adv V", "pdt_ctc_prefix_search_advance", ctc_adv(2,2,B30,2)),
 ("ctc_adv S", "pdt_ctc_prefix_search_advance", ctc_adv(2,2,9,2,S=1<<26)),
 ("ctc_adv N", "pdt_ctc_prefix_search_advance", ctc_adv(B31,2,9,2)),
 ("ctc_adv wide KV", "pdt_ctc_prefix_search_advance", ctc_adv(2,64,1<<25,2)),
 ("ctc_adv_lm S", "pdt_ctc_prefix_search_advance_lm", ctc_adv_lm(2,2,9,2,S=1<<26)),
 ("beam_adv V", "pdt_beam_search_advance", beam_adv(2,2,B30,2)),
 ("beam_adv wide KV", "pdt_beam_search_advance", beam_adv(2,128,1<<24,2)),
 ("beam_step Kp", "pdt_beam_search_step", beam_step(2,65,9,2)),
 ("beam_step V", "pdt_beam_search_step", beam_step(2,2,B30,2)),
 ("beam_step_table V", "pdt_beam_search_step_table", beam_step_table(2,2,B30,2)),
 ("beam_table iters", "pdt_beam_search_table", (P,100,1,5,P,0,2,100,4,1<<24,0,0,0,P,P,P,P,P,0)),
 ("beam_table N", "pdt_beam_search_table", (P,100,1,5,P,0,B31,100,4,8,0,0,0,P,P,P,P,P,0)),
 ("walk_adv V", "pdt_random_walk_advance", (P,B30,1,2,B30,P,1,P,1,P,3,2,1,P,1,P,P,P,P,0)),
 ("walk_adv SN", "pdt_random_walk_advance", (P,9,1,1<<20,9,P,1,P,1,P,1<<20,1<<20,1,P,1,P,P,P,P,0)),
 ("walk_step V", "pdt_random_walk_step", (P,B30,1,2,B30,P,0,0,P,P,P,P,P,P,0)),
 ("walk_step N", "pdt_random_walk_step", (P,9,1,B31,9,P,0,0,P,P,P,P,P,P,0)),
 ("walk_table C", "pdt_random_walk_table", (P,9,5,5,9,P,P,2,1<<24,0,0,P,P,P,P,P,P,P,0)),
 ("walk_table RU", "pdt_random_walk_table", (P,9,1<<20,1<<20,9,P,P,2,4,0,0,P,P,P,P,P,P,P,0)),
 ("fusion V", "pdt_fusion_ext", (P,2,2,B30,P,B30,1,P,1,0.3,0,P,0)),
 ("fusion Kp", "pdt_fusion_ext", (P,1,B31,4,P,4,1,P,1,0.3,0,P,0)),
 ("fusion rows", "pdt_fusion_ext", (P,1<<17,1<<16,4,P,4,1,P,1,0.3,0,P,0)),
 ("factor V", "pdt_lm_factor_table", (P,4,B30,0.3,0,P,B30,0)),
 ("factor rows", "pdt_lm_factor_table", (P,1<<33,4,0.3,0,P,4,0)),
 ("return blocks", "pdt_time_distributed_return", (P,0,1,1<<40,1<<40,1,G,0,P,1<<40,1,0,0,0)),
 ("gumbel V", "pdt_relaxed_gumbel", (0,0,P,1,B31,1,P,0,1,B31,P,0)),
 ("gumbel blocks", "pdt_relaxed_gumbel", (0,0,P,1,1,1,P,0,1<<40,1,P,0)),
 ("bernoulli V", "pdt_relaxed_bernoulli", (0,0,P,1,B31,1,P,0,1,B31,P,0)),
 ("gumbel_bwd V", "pdt_relaxed_gumbel_backward", (0,0,P,P,1,B31,1,P,0,1,B31,P,0,0,0)),
 ("bernoulli_bwd V", "pdt_relaxed_bernoulli_backward", (0,0,P,P,1,B31,1,P,0,1,B31,P,0,0,0)),
 ("mc blocks", "pdt_mc_reduce", (0,0,0,0,1,1<<40,IN,ST,P,P,0)),
 ("mc MB", "pdt_mc_reduce", (0,0,0,0,1<<40,1<<40,IN,ST,P,P,0)),
 ("mc_bwd blocks", "pdt_mc_reduce_backward", (0,0,0,0,1<<20,1<<22,IN,ST,P,P,GR,0)),
 ("imh blocks", "pdt_imh_chain", (0,P,1<<40,1,P,1,P,1<<40,1,4,1<<40,P,P,P,0)),
 ("lookup_search V", "pdt_ctc_lookup_lm_search", (P,9,9,1,0,4,2,B30,4,P,P,P,P,P,P,P,2,B30+2,0,0.3,0,P,P,P,P,P,1<<20,0)),
 ("lookup_search frames", "pdt_ctc_lookup_lm_search", (P,9,9,1,0,1<<26,2,8,4,P,P,P,P,P,P,P,2,10,0,0.3,0,P,P,P,P,P,1<<20,0)),
 ("lookup_search V16", "pdt_ctc_lookup_lm_search", (P,9,9,1,0,4,2,32768,4,P,P,P,P,P,P,P,2,32770,0,0.3,0,P,P,P,P,P,1<<20,0)),
 ("lm_table T", "pdt_ctc_lm_table_search", (P,1<<24,2,8,18,9,1,0,4,4,P,P,9,8,8,9,1,0.3,0,P,P,P,P,0)),
 ("lm_table contexts", "pdt_ctc_lm_table_search", (P,4,2,8,18,9,1,0,4,4,P,P,B30,8,8,B30,1,0.3,0,P,P,P,P,0)),
 ("lm_table N", "pdt_ctc_lm_table_search", (P,4,B31,8,18,9,1,0,4,4,P,P,9,8,8,9,1,0.3,0,P,P,P,P,0)),
 ("dense_warp N", "pdt_dense_image_warp", (P,P,65536,1,4,4,0,0,0,P,0)),
 ("dense_warp HW", "pdt_dense_image_warp", (P,P,1,1,1<<16,1<<15,0,0,0,P,0)),
 ("dense_warp_bwd N", "pdt_dense_image_warp_backward", (P,P,65536,1,4,4,0,0,0,P,0)),
 ("dense_warp_f64 N", "pdt_dense_image_warp_f64", (P,P,65536,1,4,4,0,0,0,P,0)),
 ("dense_warp_bwd_f64 N", "pdt_dense_image_warp_backward_f64", (P,P,65536,1,4,4,0,0,0,P,0)),
 ("sparse_warp N", "pdt_sparse_image_warp", (P,P,P,65536,1,4,4,3,2,0.,0,0,0,P,0,0,P,0)),
 ("sparse_warp_bwd N", "pdt_sparse_image_warp_backward", (P,P,P,65536,1,4,4,3,2,0.,0,0,0,P,P,0)),
 ("sparse_warp_f64 N", "pdt_sparse_image_warp_f64", (P,P,P,65536,1,4,4,3,2,0.,0,0,0,P,0,0,P,0)),
 ("sparse_warp_bwd_f64 N", "pdt_sparse_image_warp_backward_f64", (P,P,P,65536,1,4,4,3,2,0.,0,0,0,P,P,0)),
 ("spline_solve N", "pdt_spline_solve", (P,P,0,65536,3,1,1,2,0.,P,P,0)),
 ("spline_solve S", "pdt_spline_solve", (P,P,0,2,4096,1,1,2,0.,P,P,0)),
 ("spline N", "pdt_polyharmonic_spline", (P,P,P,65536,3,1,1,4,2,0.,P,P,0)),
 ("spline O", "pdt_polyharmonic_spline", (P,P,P,2,3,1,65,4,2,0.,P,P,0)),
 ("vocab length", "pdt_enumerate_vocab_sequences", (B30,2,0,P,0)),
 ("vocab rows", "pdt_enumerate_vocab_sequences", (32,2,0,P,0)),
 ("binom blocks", "pdt_binomial_coefficient", (P,P,1<<40,P,P,P,0)),
 ("card width", "pdt_enumerate_cardinality", (P,P,0,0,2,4,63,P,0,P,0)),
 ("card tiles", "pdt_enumerate_cardinality", (P,P,0,0,1<<20,1<<40,8,P,0,P,0)),
 ("srswor blocks", "pdt_srswor", (P,P,P,1<<42,4,P,0)),
 ("spec TF", "pdt_spec_augment_apply", (P,2,1<<20,1<<11,B31,1<<11,1,0,0,0,0,0,0,0,0,P,0)),
 ("spec N", "pdt_spec_augment_apply", (P,B31,5,5,25,5,1,0,0,0,0,0,0,0,0,P,0)),
 ("attn_dot R", "pdt_attn_dot", (D,0,P,P,P,0,G,P,P,P,1<<20,0)),
 ("attn_pool R", "pdt_attn_pool", (D2,0,P,P,0,P,P,P,1<<20,0)),
 ("feat P", "pdt_feat_deltas", (P,0,1,1,8,1,4,32,32,4,4,1,P,3,B28,0,0,0,P,0)),
 ("feat blocks", "pdt_feat_deltas", (P,0,1<<40,1,8,1,4,32,32,4,4,1,P,3,2,0,0,0,P,0)),
 ("feat_bwd blocks", "pdt_feat_deltas_backward", (P,0,1<<40,1,8,1,4,P,3,2,0,0,P,0)),
 ("mvn_apply blocks", "pdt_mvn_apply", (P,0,1<<42,4,1,P,P,P,0)),
 ("mvn_stats X", "pdt_mvn_stats", (P,0,0,0,1,B31,1,0,P,P,P,P,1<<62,0)),
 ("mvn_bwd blocks", "pdt_mvn_backward", (P,P,0,1<<42,4,1,P,P,P,0)),
 ("slice_ali_emit T", "pdt_slice_ali_emit", (P,1,3000000000,P,P,P,P,0,0,0,P,P,0)),
 ("slice_ali_emit NT", "pdt_slice_ali_emit", (P,1<<17,1<<16,P,P,P,P,0,0,0,P,P,0)),
 ("slice_ali_segments T", "pdt_slice_ali_segments", (P,1,B31-256,P,P,P,0)),
 ("slice_ref T", "pdt_slice_ref", (P,1,B31-256,P,0,0,0,0,0,0,0,0,P,0)),
 ("slice_fixed TT", "pdt_slice_fixed", (1,B31-256,P,0,1,4,0,0,0,0,0,P,0)),
 ("chunk_tokens R", "pdt_chunk_tokens", (P,1,B31-256,P,0,0,0,P,P,0)),
 ("ocd H", "pdt_ocd_loss_forward", (P,B31,1,9,9,9,1,P,P,4,0,-2,P,P,0,0)),
 ("ocd N", "pdt_ocd_loss_backward", (P,1,1<<32,9,9,9,1,P,P,4,0,-2,P,P,0)),
 ("ocd V30", "pdt_ocd_loss_forward", (P,2,2,B30,2*B30,B30,1,P,P,4,0,-2,P,P,0,0)),
 ("ocd R", "pdt_ocd_loss_forward", (P,2,2,9,18,9,1,P,P,B31,0,-2,P,P,0,0)),
 ("fill grid", "pdt_fill_after_eos", (P,1<<40,4,2,0,P,4,0,P,0)),
 ("lookup_lm S", "pdt_lookup_lm_log_probs", (P,B31,2,2,1,P,0,2,P,P,P,P,0,0,0,10,3,11,0,P,0,0)),
 ("lookup_lm rows", "pdt_lookup_lm_log_probs", (P,3,B31,B31,1,P,0,B31,P,P,P,P,0,0,0,10,3,11,0,P,0,0)),
 ("gumbel_bwd blocks", "pdt_relaxed_gumbel_backward", (0,0,P,P,1<<40,1,1,P,0,1<<40,1,P,0,0,0)),
 ("lm_table width", "pdt_ctc_lm_table_search", (P,4,2,8,18,9,1,0,33,4,P,P,9,8,8,9,1,0.3,0,P,P,P,P,0)),
 ("ctc_search width", "pdt_ctc_prefix_search", (P,5,2,30,62,31,1,0,33,5,P,P,P,P,0)),
 ("ctc_wide width", "pdt_ctc_prefix_search_wide", (P,5,2,30,62,31,1,0,129,5,P,P,P,P,0)),
 ("lookup_search width", "pdt_ctc_lookup_lm_search", (P,9,9,1,0,4,2,8,33,P,P,P,P,P,P,P,2,10,0,0.3,0,P,P,P,P,P,1<<20,0)),
 ("lookup_search order", "pdt_ctc_lookup_lm_search", (P,9,9,1,0,4,2,8,4,P,P,P,P,P,P,P,17,10,0,0.3,0,P,P,P,P,P,1<<20,0)),
]
# fmt: on


@pytest.mark.parametrize("label,fn,args", GUARD_CALLS, ids=[c[0].replace(" ", "_") for c in GUARD_CALLS])
def test_guard_refuses_before_any_launch(lib, label, fn, args):
    from pydrobert_amd import _cabi

    assert len(args) == len(_cabi.SIGNATURES[fn][1]), (fn, len(args))
    assert getattr(lib, fn)(*args) == _cabi.PDT_E_TOO_LONG, label
