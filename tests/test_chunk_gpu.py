"""GPU: the HIP route of pad_masked_sequence, chunk_by_slices, chunk_token_sequences_by_slices and
slice_spect_data (csrc/seq_chunk.hip) -- bit-equal to the goldens captured from the reference and, on
randomised sweeps, to the package's torch body run on the CPU (which test_chunk_cpu.py holds to the same
goldens); gradients by gradcheck in float64; streams, determinism, host read counts, script / trace /
compile."""
import warnings

import numpy as np
import pytest
import torch

from test_chunk_cpu import (  # noqa: F401
    check_chunk_goldens, check_errors, check_masked_goldens, check_slice_goldens, check_token_goldens, gold, head,
)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ("constant", "reflect", "replicate")


def _eq(act, exp):
    assert len(act) == len(exp)
    for a, e in zip(act, exp):
        assert a.device.type == "cuda" and a.dtype == e.dtype and a.shape == e.shape, (a.shape, e.shape)
        assert torch.equal(a.cpu(), e)


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _slices(rng, N, T, lens, mode):
    """Random slices that the mode admits (reflect: pads below the length; replicate: lens >= 1)."""
    ln = lens if lens is not None else np.full(N, T)
    if mode == "reflect":
        start = rng.integers(-(ln - 1), 2 * ln - 1)
        end = np.minimum(start + rng.integers(-1, 2 * T + 1, N), 2 * ln - 1)
    else:
        start = rng.integers(-T, 2 * T, N)
        end = start + rng.integers(-2, 2 * T + 1, N)
    return torch.from_numpy(np.stack([start, end], 1).astype(np.int64))


def test_goldens_bit_equal(gold):
    from pydrobert_amd import functional as F

    check_chunk_goldens(gold, F, DEV)
    check_masked_goldens(gold, F, DEV)
    check_token_goldens(gold, F, DEV)
    check_slice_goldens(gold, F, DEV)


def test_error_types_on_device(gold):
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    check_errors(gold, F, M, DEV)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000, 4097])
def test_pad_masked_sequence_sweep(T):
    from pydrobert_amd import functional as F

    rng = np.random.default_rng(T)
    for Fd, batch_first, dtype in ((1, True, torch.float32), (3, False, torch.int64), (80, True, torch.float16),
                                   (None, False, torch.bool), (3, True, torch.bfloat16), (None, True, torch.float64)):  # fmt: skip
        N = 5
        shape = ((N, T) if batch_first else (T, N)) + (() if Fd is None else (Fd,))
        x = torch.from_numpy(rng.standard_normal(shape) * 8)
        x = (x > 0) if dtype == torch.bool else x.to(dtype)
        mask = torch.from_numpy(rng.random(shape[:2]) < rng.random())
        _eq(F.pad_masked_sequence(*_dev(x, mask), batch_first, -2.0), F.pad_masked_sequence(x, mask, batch_first, -2.0))
    # non-contiguous x and mask: strided steps, a transposed mask, trailing dims that are not dense
    x = torch.from_numpy(rng.standard_normal((4, 2 * T, 6))).float()
    mask = torch.from_numpy(rng.random((T, 4)) < 0.6)
    xd, md = _dev(x, mask)
    _eq(F.pad_masked_sequence(xd[:, ::2], md.t(), True, 0.5), F.pad_masked_sequence(x[:, ::2], mask.t(), True, 0.5))
    _eq(F.pad_masked_sequence(xd[:, :T, ::2], md.t(), True), F.pad_masked_sequence(x[:, :T, ::2], mask.t(), True))
    _eq(F.pad_masked_sequence(xd[:, :T].transpose(0, 1), md), F.pad_masked_sequence(x[:, :T].transpose(0, 1), mask))


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000, 4097])
@pytest.mark.parametrize("mode", MODES)
def test_chunk_by_slices_sweep(T, mode):
    from pydrobert_amd import functional as F

    rng = np.random.default_rng(T + len(mode))
    for Fd, dtype, with_lens in ((1, torch.float32, True), (3, torch.int64, False), (80, torch.float16, True),
                                 (None, torch.bool, True), (3, torch.bfloat16, False), (None, torch.float64, True)):  # fmt: skip
        N = 6
        x = torch.from_numpy(rng.standard_normal((N, T) + (() if Fd is None else (Fd,))) * 8)
        x = (x > 0) if dtype == torch.bool else x.to(dtype)
        lens = rng.integers(1, T + 1, N) if with_lens else None
        slices = _slices(rng, N, T, lens, mode)
        tl = None if lens is None else torch.from_numpy(lens)
        _eq(F.chunk_by_slices(*_dev(x, slices, tl), mode, 1.0), F.chunk_by_slices(x, slices, tl, mode, 1.0))
    x = torch.from_numpy(rng.standard_normal((4, 2 * T, 6))).float()
    slices = _slices(rng, 4, T, None, mode)
    xd, sd = _dev(x, slices)
    _eq(F.chunk_by_slices(xd[:, ::2], sd, None, mode), F.chunk_by_slices(x[:, ::2], slices, None, mode))
    _eq(F.chunk_by_slices(xd[:, :T, ::2], sd, None, mode), F.chunk_by_slices(x[:, :T, ::2], slices, None, mode))


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000, 4097])
def test_chunk_tokens_sweep(R):
    from pydrobert_amd import functional as F

    rng = np.random.default_rng(R)
    N = 7
    start = rng.integers(-2, 3 * R, (N, R))
    refs = torch.from_numpy(np.stack([rng.integers(0, 50, (N, R)), start, start + rng.integers(-2, R + 2, (N, R))], 2))
    s0 = rng.integers(-3, R, N)
    slices = torch.from_numpy(np.stack([s0, s0 + rng.integers(0, 3 * R, N)], 1))
    lens = torch.from_numpy(rng.integers(0, R + 1, N))
    for partial in (False, True):
        for retain in (False, True):
            for rl in (None, lens):
                act = F.chunk_token_sequences_by_slices(*_dev(refs, slices, rl), partial, retain)
                _eq(act, F.chunk_token_sequences_by_slices(refs, slices, rl, partial, retain))
                tail = torch.arange(R, device=DEV).unsqueeze(0) >= act[1].unsqueeze(1)
                assert bool((act[0][tail] == 0).all())  # zeros beyond chunked_lens


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000, 4097])
def test_slice_spect_data_sweep(T):
    from pydrobert_amd import functional as F

    rng = np.random.default_rng(T)
    N = 5
    ali = torch.from_numpy(rng.integers(0, 2, (N, T)))
    lens = torch.from_numpy(rng.integers(0, T + 1, N))
    lens[0], lens[1] = T, 0
    start = np.sort(rng.integers(-1, 2 * T, (N, T)), 1)
    refs = torch.from_numpy(np.stack([rng.integers(0, 9, (N, T)), start, start + rng.integers(-1, 6, (N, T))], 2))
    other = torch.from_numpy(rng.integers(T, 2 * T + 4, N))
    feats = torch.zeros((N, T, 2))
    for window in ("symmetric", "causal", "future"):
        for valid in (True, False):
            for lobe in (0, 1, 2, 5):
                cfg = (window, valid, lobe)
                for args in ((feats, None, None, "fixed"), (feats, lens, None, "fixed"), (ali, lens, None, "ali"),
                             (ali, None, None, "ali"), (refs, lens, other, "ref"), (refs, None, None, "ref"),
                             (refs, lens, None, "ref")):  # fmt: skip
                    _eq(F.slice_spect_data(*_dev(*args[:3]), args[3], *cfg), F.slice_spect_data(*args, *cfg))


def test_front_end_shape_sampled_rows():
    """N=2048, T=1000, F=80 float32: rows sampled across the batch against the torch body on the CPU."""
    from pydrobert_amd import functional as F

    rng = np.random.default_rng(7)
    N, T, Fd = 2048, 1000, 80
    x = torch.randn(N, T, Fd, device=DEV)
    lens = torch.from_numpy(rng.integers(T // 2, T + 1, N))
    rows = torch.from_numpy(np.concatenate([[0, 1, N - 1], rng.integers(0, N, 13)]))
    for mode in MODES:
        slices = _slices(rng, N, T, lens.numpy(), mode)
        y, yl = F.chunk_by_slices(x, *_dev(slices, lens), mode, -1.0)
        ey, eyl = F.chunk_by_slices(x[rows.to(DEV)].cpu(), slices[rows], lens[rows], mode, -1.0)
        Tp = ey.shape[1]  # (the sampled rows' T' may be below the batch's)
        assert torch.equal(yl.cpu()[rows], eyl) and y.shape[1] >= Tp
        assert torch.equal(y[rows.to(DEV)].cpu()[:, :Tp], ey) and bool((y[rows.to(DEV)][:, Tp:] == -1.0).all())
    mask = torch.from_numpy(rng.random((N, T)) < 0.7)
    y, yl = F.pad_masked_sequence(x, mask.to(DEV), True, -1.0)
    ey, eyl = F.pad_masked_sequence(x[rows.to(DEV)].cpu(), mask[rows], True, -1.0)
    assert torch.equal(yl.cpu(), mask.sum(1)) and torch.equal(y[rows.to(DEV)].cpu(), ey)


def test_pipeline_end_to_end():
    """SliceSpectData -> x[sources] -> ChunkBySlices / ChunkTokenSequencesBySlices, device against CPU."""
    from pydrobert_amd import modules as M

    rng = np.random.default_rng(11)
    N, T, Fd, R = 16, 300, 8, 12
    feats = torch.randn(N, T, Fd)
    lens = torch.from_numpy(rng.integers(T // 2, T + 1, N))
    start = np.sort(rng.integers(0, T // 2, (N, R)), 1)
    refs = torch.from_numpy(np.stack([rng.integers(0, 30, (N, R)), start, start + rng.integers(1, 30, (N, R))], 2))
    ref_lens = torch.from_numpy(rng.integers(1, R + 1, N))
    for slicer, chunker in ((M.SliceSpectData("fixed", "symmetric", False, 20), M.ChunkBySlices("reflect")),
                            (M.SliceSpectData("ref", "causal", True, 3), M.ChunkBySlices("replicate"))):  # fmt: skip
        tokens = M.ChunkTokenSequencesBySlices(partial=True)
        res = []
        for dev in ("cpu", DEV):
            f, l, r, rl = (t.to(dev) for t in (feats, lens, refs, ref_lens))
            if slicer.policy == "ref":
                slices, sources = slicer(r, rl, l)
            else:
                slices, sources = slicer(f, l)
            assert slices.shape[0] > N
            res.append((slices, sources) + chunker(f[sources], slices, l[sources]) + tokens(r[sources], slices, rl[sources]))
        _eq(res[1], res[0])


@pytest.mark.parametrize("mode", MODES)
def test_chunk_by_slices_gradcheck(mode):
    from pydrobert_amd import functional as F

    rng = np.random.default_rng(3)
    N, T = 4, 9
    lens = np.array([9, 5, 1 if mode != "reflect" else 3, 7])
    slices = _slices(rng, N, T, lens, mode).to(DEV)
    for rest in ((), (3,)):
        x = torch.randn((N, T) + rest, device=DEV, dtype=torch.float64, requires_grad=True)
        for tl in (torch.from_numpy(lens).to(DEV), None):
            if tl is None and mode == "reflect":
                continue  # (the slices were drawn for the lengths)
            torch.autograd.gradcheck(lambda v: F.chunk_by_slices(v, slices, tl, mode, 0.5)[0], (x,))
    x32 = torch.randn(N, T, 3, device=DEV, requires_grad=True)
    tl = torch.from_numpy(lens).to(DEV)
    y = F.chunk_by_slices(x32, slices, tl, mode)[0]
    g = torch.randn_like(y)
    (gx,) = torch.autograd.grad(y, x32, g)
    xc = x32.detach().cpu().requires_grad_(True)
    (ex,) = torch.autograd.grad(F.chunk_by_slices(xc, slices.cpu(), tl.cpu(), mode)[0], xc, g.cpu())
    assert torch.allclose(gx.cpu(), ex, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("batch_first", [False, True])
def test_pad_masked_sequence_gradcheck(batch_first):
    from pydrobert_amd import functional as F

    N, T = 3, 70
    for rest in ((), (2,)):
        shape = ((N, T) if batch_first else (T, N)) + rest
        x = torch.randn(shape, device=DEV, dtype=torch.float64, requires_grad=True)
        mask = torch.rand(shape[:2], device=DEV) < 0.5
        torch.autograd.gradcheck(lambda v: F.pad_masked_sequence(v, mask, batch_first, 0.5)[0], (x,))
    x32 = torch.randn(shape, device=DEV, requires_grad=True)
    g = torch.randn(shape, device=DEV)
    (gx,) = torch.autograd.grad(F.pad_masked_sequence(x32, mask, batch_first)[0], x32, g)
    xc = x32.detach().cpu().requires_grad_(True)
    (ex,) = torch.autograd.grad(F.pad_masked_sequence(xc, mask.cpu(), batch_first)[0], xc, g.cpu())
    assert torch.equal(gx.cpu(), ex)


def _all_ops(x, mask, slices, lens, refs, ali):
    from pydrobert_amd import functional as F

    return (F.pad_masked_sequence(x, mask, True) + F.chunk_by_slices(x, slices, lens, "replicate")
            + F.chunk_token_sequences_by_slices(refs, slices, None, True)
            + F.slice_spect_data(ali, lens, None, "ali", "symmetric", False, 2)
            + F.slice_spect_data(refs, None, None, "ref", "future", False, 1))  # fmt: skip


def _inputs():
    rng = np.random.default_rng(5)
    N, T = 32, 500
    x = torch.randn(N, T, 16)
    lens = torch.from_numpy(rng.integers(1, T + 1, N))
    start = rng.integers(0, T, (N, 40))
    refs = torch.from_numpy(np.stack([rng.integers(0, 9, (N, 40)), start, start + rng.integers(0, 50, (N, 40))], 2))
    return _dev(x, torch.rand(N, T) < 0.5, _slices(rng, N, T, lens.numpy(), "replicate"), lens, refs,
                torch.from_numpy(rng.integers(0, 3, (N, T))))  # fmt: skip


def test_side_stream_and_determinism():
    args = _inputs()
    first = _all_ops(*args)
    second = _all_ops(*args)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _all_ops(*args)
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def _host_reads(fn):
    """How many times ``fn`` makes the host wait for the device.  Counted as the warnings of sync-debug mode
    "warn": mode "error" stops at the first read, so it can assert "none" but not "exactly one"."""
    fn()  # (warm: the library loads, the allocator settles)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return len([w for w in seen if "synchroniz" in str(w.message)])


def test_host_read_counts():
    from pydrobert_amd import functional as F

    x, mask, slices, lens, refs, ali = _inputs()
    assert _host_reads(lambda: F.pad_masked_sequence(x, mask, True)) == 0
    assert _host_reads(lambda: F.pad_masked_sequence(x.transpose(0, 1), mask.t())) == 0
    assert _host_reads(lambda: F.chunk_token_sequences_by_slices(refs, slices, lens.clamp_max(40))) == 0
    assert _host_reads(lambda: F.slice_spect_data(x, None, None, "fixed", "symmetric", False, 3)) == 0
    for mode in MODES:
        sl = slices if mode != "reflect" else torch.stack([-(lens // 2), lens + lens // 2], 1)
        assert _host_reads(lambda: F.chunk_by_slices(x, sl, lens, mode)) == 1
    assert _host_reads(lambda: F.slice_spect_data(x, lens, None, "fixed", "causal", False, 3)) == 1
    assert _host_reads(lambda: F.slice_spect_data(ali, lens, None, "ali", "symmetric", True, 2)) == 1
    assert _host_reads(lambda: F.slice_spect_data(ali, None, None, "ali", "future", False, 2)) == 1
    assert _host_reads(lambda: F.slice_spect_data(refs, None, lens, "ref", "symmetric", False, 2)) == 1
    assert _host_reads(lambda: F.slice_spect_data(refs, None, None, "ref")) == 1


def test_script_trace_compile_on_device():
    from pydrobert_amd import modules as M

    x, mask, slices, lens, refs, ali = _inputs()
    cases = (
        (M.PadMaskedSequence(True, -1.0), (x, mask)),
        (M.ChunkBySlices("replicate"), (x, slices, lens)),
        (M.ChunkTokenSequencesBySlices(True, True), (refs, slices, lens.clamp_max(40))),
        (M.SliceSpectData("ali", "symmetric", False, 1), (ali, lens)),
        (M.SliceSpectData("fixed", "causal", True, 2), (x, lens)),
        (M.SliceSpectData("ref", "symmetric", False, 1), (refs, lens.clamp_max(40), lens)),
        (M.PadMaskedSequence(), (x.transpose(0, 1), mask.t())),
    )
    for mod, args in cases:
        exp = mod(*args)
        for other in (torch.jit.script(mod), torch.jit.trace(mod, args), torch.compile(mod, backend="eager")):
            got = other(*args)
            assert all(torch.equal(a, b) for a, b in zip(got, exp)), mod
