"""GPU: the string operators whose recurrence kernel classifies its own utterances (the fused form
of lev_bitpar_kernel, csrc/lev_bitpar.hip) against the CPU oracle AND against the two-launch route
(pdt_lev_keep: lev_classify_kernel into the workspace, then the recurrence; pdt_lev_classified: the
recurrence alone on those tables).  Results are small integers and quotients of them: every
comparison is exact, and the warning word of the fused call is the two-launch call's.

optimal_completion's mask kernel classifies its own utterances too (oc_bitpar_kernel,
csrc/oc_bitpar.hip); pdt_oc_mask has no keeping variant, so its other routes are reached the way a
caller reaches them: the row-synchronous kernel through the switch PDT_OC_BITPAR = 0 (every case),
and the two launches
(lev_classify_kernel, then the mask kernel on the workspace's tables) through a hypothesis tensor of
513 rows -- one row past what the fused form takes -- whose extra row lies behind every eos, so the
first 513 rows of the result are the same problem's (the cases with an eos and include_eos=False).
"""
import warnings

import numpy as np
import pytest
import torch

from pydrobert_amd import switches

import oracle
from pydrobert_amd import _cabi
from pydrobert_amd import functional as F

pytestmark = pytest.mark.gpu

OPS = ["error_rate", "prefix_error_rates", "prefix_edit_distances", "optimal_completion"]


def _ragged(rng, T, N, V, eos, lo):
    """(T, N) tokens below V with `eos` written at a length drawn from [lo, T] (T: no eos at all)."""
    x = rng.integers(0, V, (T, N))
    lens = rng.integers(lo, T + 1, N)
    for n, l in enumerate(lens):
        if l < T:
            x[l, n] = eos
    return x


def _lev_abi(entry, tr, th, batch_first, eos, include_eos, norm, mode, exclude_last, mistakes, ws):
    """One call of a pdt_lev-shaped entry point; returns (out, lengths, warning word)."""
    L = _cabi.lib()
    if batch_first:
        (N, R), (_, H) = tr.shape, th.shape
        rst, rsn, hst, hsn = tr.stride(1), tr.stride(0), th.stride(1), th.stride(0)
    else:
        (R, N), (H, _) = tr.shape, th.shape
        rst, rsn, hst, hsn = tr.stride(0), tr.stride(1), th.stride(0), th.stride(1)
    dev = tr.device
    Hout = H + (0 if exclude_last else 1)
    out = torch.full((Hout, N) if mode == _cabi.MODE_PREFIX else (N,), -7.0, device=dev)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    rl = torch.full((N,), -1, device=dev, dtype=torch.int64)
    hl = torch.full((N,), -1, device=dev, dtype=torch.int64)
    rc = getattr(L, entry)(
        _cabi.ptr(tr), R, rst, rsn, _cabi.ptr(th), H, hst, hsn, N,
        int(eos is not None), int(eos) if eos is not None else 0, int(include_eos),
        1.0, 1.0, 1.0, int(norm), mode, int(exclude_last), -100.0, int(mistakes),
        _cabi.ptr(out), out.stride(0) if mode == _cabi.MODE_PREFIX else 0, out.stride(-1),
        _cabi.ptr(rl), _cabi.ptr(hl), _cabi.ptr(status), _cabi.ptr(ws), ws.numel(), _cabi.stream_ptr(dev),
    )  # fmt: skip
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return out.cpu(), rl.cpu(), hl.cpu(), int(status.item())


def _check(device, ref, hyp, eos=None, include_eos=False, exclude_last=False, batch_first=False, oracle_ops=OPS):
    """Every operator on (ref, hyp): fused == two launches == recurrence on kept tables (bits, lengths,
    warning word), and the public functions == the oracle."""
    tr, th = torch.from_numpy(ref).to(device), torch.from_numpy(hyp).to(device)
    if batch_first:  # (N, T) views of time-major storage: the strides of a transposed batch
        tr, th = tr.t(), th.t()
        ref, hyp = ref.T, hyp.T
    R, H = (tr.shape[1], th.shape[1]) if batch_first else (tr.shape[0], th.shape[0])
    N = tr.shape[0] if batch_first else tr.shape[1]
    nbytes = int(_cabi.lib().pdt_lev_workspace_bytes(R, H, N))
    assert nbytes > 0
    # (garbage in the workspace: the fused call must not depend on it, the keeping call must fill it)
    ws = torch.randint(0, 255, (nbytes,), device=device, dtype=torch.uint8)
    flavours = [  # (mode, norm, mistakes, exclude_last)
        (_cabi.MODE_FINAL, 1, 1, False),  # error_rate
        (_cabi.MODE_PREFIX, 1, 1, exclude_last),  # prefix_error_rates
        (_cabi.MODE_PREFIX, 0, 0, exclude_last),  # prefix_edit_distances
    ]
    for mode, norm, mistakes, excl in flavours:
        if excl and H == 0:
            continue
        args = (tr, th, batch_first, eos, include_eos, norm, mode, excl, mistakes)
        fused = _lev_abi("pdt_lev", *args, ws)
        ws2 = torch.randint(0, 255, (nbytes,), device=device, dtype=torch.uint8)
        kept = _lev_abi("pdt_lev_keep", *args, ws2)
        again = _lev_abi("pdt_lev_classified", *args, ws2)
        what = (R, H, N, eos, include_eos, excl, batch_first, mode)
        assert torch.equal(fused[0], kept[0]), what
        assert torch.equal(fused[1], kept[1]) and torch.equal(fused[2], kept[2]), what
        assert fused[3] == kept[3], (what, fused[3], kept[3])
        assert torch.equal(fused[0], again[0]), what
        assert again[3] == 0, what  # (pdt_lev_classified does not write the word)
    kw = dict(eos=eos, include_eos=include_eos, batch_first=batch_first)
    for name in oracle_ops:
        k = dict(kw)
        if name != "error_rate":
            k["exclude_last"] = exclude_last
            if exclude_last and H == 0:
                continue
        exp = getattr(oracle, name)(ref, hyp, faithful=False, **k)  # (unit costs: the plain recurrence)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            act = getattr(F, name)(tr, th, warn=False, **k).cpu().numpy()
        assert exp.shape == act.shape and exp.dtype == act.dtype, (name, exp.shape, act.shape)
        assert np.array_equal(exp, act), (name, k, np.argwhere(exp != act)[:5])
        if name != "optimal_completion":
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with switches.override(PDT_OC_BITPAR=0):  # the row-synchronous kernel
                other = getattr(F, name)(tr, th, warn=False, **k).cpu().numpy()
            assert np.array_equal(act, other), ("row-synchronous route", k)
            if eos is not None and not include_eos and H == 512:
                # two launches: a 513th hypothesis row of eos (every sequence has ended by then, or ends there)
                pad = torch.full((N, 1) if batch_first else (1, N), eos, device=device, dtype=th.dtype)
                th2 = torch.cat([th, pad], 1 if batch_first else 0)
                two = getattr(F, name)(tr, th2, warn=False, **k).cpu().numpy()
            else:
                two = None
        if two is not None:
            rows = act.shape[1] if batch_first else act.shape[0]
            two = two[:, :rows] if batch_first else two[:rows]
            # (the extra row holds padding only: the largest completion set, the last dimension, is the same)
            assert two.shape == act.shape and np.array_equal(two, act), ("two-launch route", k, two.shape, act.shape)


def test_bench_shape(device):
    """N = 4096, R = H = 512, V = 256, no eos: the benchmark's string inputs.  (optimal_completion's
    (513, N, C) int64 result is 1.5 GB at this N: its oracle comparison takes the first 256 utterances.)"""
    rng = np.random.default_rng(701)
    ref, hyp = rng.integers(0, 256, (512, 4096)), rng.integers(0, 256, (512, 4096))
    _check(device, ref, hyp, oracle_ops=OPS[:3])
    _check(device, np.ascontiguousarray(ref[:, :256]), np.ascontiguousarray(hyp[:, :256]), oracle_ops=OPS[3:])


@pytest.mark.parametrize("include_eos", [False, True])
@pytest.mark.parametrize("exclude_last", [False, True])
def test_ragged_eos(device, include_eos, exclude_last):
    """Lengths anywhere in [0, T] (some sequences without any eos: the missing-eos warning bits),
    N not a multiple of 4, few distinct tokens (empty references under norm: the third bit)."""
    rng = np.random.default_rng(702 + 2 * include_eos + exclude_last)
    T, N, V = 512, 203, 5
    ref, hyp = _ragged(rng, T, N, V, V, 0), _ragged(rng, T - 9, N, V, V, 0)
    _check(device, ref, hyp, eos=V, include_eos=include_eos, exclude_last=exclude_last)
    ref, hyp = _ragged(rng, T, N, 300, 300, 100), _ragged(rng, T, N, 300, 300, 100)  # 512 rows: see the module's note
    _check(device, ref, hyp, eos=300, include_eos=include_eos, exclude_last=exclude_last)


@pytest.mark.parametrize("R,H", [(1, 511), (31, 512), (32, 300), (33, 257), (511, 511), (512, 512), (513, 512),
                                 (512, 513), (512, 1), (512, 31), (512, 32), (512, 33), (300, 400)])
def test_lengths_around_the_block_and_shape_limits(device, R, H):
    """Tensor lengths 1, 31, 32, 33, 511-513 on either side (512 is the last length the fused form and
    the bit-parallel completion kernel take; past it the other routes must give the same), and the
    same numbers as eos positions inside 512-token tensors."""
    rng = np.random.default_rng(1000 * R + H)
    N, V = 7, 9
    _check(device, rng.integers(0, V, (R, N)), rng.integers(0, V, (H, N)))
    _check(device, rng.integers(0, V, (R, N)), rng.integers(0, V, (H, N)), eos=3, include_eos=True)


def test_sequence_lengths_inside_full_tensors(device):
    """eos at 0 (empty reference / empty hypothesis), 1, 31, 32, 33, 511 in 512-token tensors."""
    rng = np.random.default_rng(704)
    cuts = [0, 1, 31, 32, 33, 511, 512]
    N, V = len(cuts) ** 2 + 1, 40
    ref, hyp = rng.integers(0, V, (512, N)), rng.integers(0, V, (512, N))
    for i, (a, b) in enumerate((a, b) for a in cuts for b in cuts):
        if a < 512:
            ref[a, i] = V
        if b < 512:
            hyp[b, i] = V
    for include_eos in (False, True):
        for exclude_last in (False, True):
            _check(device, ref, hyp, eos=V, include_eos=include_eos, exclude_last=exclude_last)


def test_empty_reference_and_hypothesis_everywhere(device):
    """Every reference empty, then every hypothesis empty (eos first), at the fused shape."""
    rng = np.random.default_rng(705)
    N, V = 6, 11
    ref, hyp = rng.integers(0, V, (512, N)), rng.integers(0, V, (512, N))
    e = ref.copy()
    e[0] = V
    _check(device, e, hyp, eos=V)
    e = hyp.copy()
    e[0] = V
    _check(device, ref, e, eos=V)
    _check(device, ref, e, eos=V, include_eos=True, exclude_last=True)


@pytest.mark.parametrize("span", ["all_large", "mixed", "negative"])
def test_tokens_beyond_the_presence_map(device, span):
    """Tokens at or above 8192 (or negative) send an utterance through the sorted table and the binary
    searches; utterances of one workgroup may take different routes."""
    rng = np.random.default_rng(706)
    T, N = 512, 13
    pool = {
        "all_large": np.concatenate([np.arange(8192, 8200), [1 << 40, (1 << 62) + 5]]),
        "mixed": np.array([0, 5, 8191, 8192, 8193, 70000]),
        "negative": np.array([-3, -1, 0, 2, 8192, -(1 << 50)]),
    }[span]
    ref, hyp = rng.choice(pool, (T, N)), rng.choice(pool, (T - 40, N))
    if span == "mixed":  # some utterances with small tokens only
        ref[:, ::3] = rng.integers(0, 6, ref[:, ::3].shape)
        hyp[:, ::3] = rng.integers(0, 6, hyp[:, ::3].shape)
    _check(device, ref, hyp)
    _check(device, ref, hyp, eos=int(pool[1]), include_eos=True)
    many = rng.integers(8192, 1 << 20, (T, N))  # up to 512 distinct classes per utterance
    _check(device, many, many[::-1].copy())


def test_batch_first_strides(device):
    """(N, T) arguments: the sequence stride is 1 and the batch stride T."""
    rng = np.random.default_rng(707)
    N, V = 37, 17
    ref, hyp = _ragged(rng, 512, N, V, V, 200), _ragged(rng, 480, N, V, V, 200)
    tr = np.ascontiguousarray(ref.T).T  # time-major VIEW of batch-first storage
    th = np.ascontiguousarray(hyp.T).T
    _check(device, tr, th, eos=V, include_eos=True, batch_first=True)
    _check(device, tr, th, batch_first=True, exclude_last=True)


def test_classified_after_a_call_that_kept_nothing(device):
    """The sequence of earlier callers -- pdt_lev, then pdt_lev_classified on the same workspace -- at a
    shape where pdt_lev now leaves no tables behind: the second call must notice and classify for
    itself (garbage in the workspace, right distances), also right after a keeping call on the same
    workspace was followed by a plain one."""
    rng = np.random.default_rng(708)
    R, H, N, V = 512, 500, 9, 12
    ref, hyp = rng.integers(0, V, (R, N)), rng.integers(0, V, (H, N))
    tr, th = torch.from_numpy(ref).to(device), torch.from_numpy(hyp).to(device)
    nbytes = int(_cabi.lib().pdt_lev_workspace_bytes(R, H, N))
    ws = torch.randint(0, 255, (nbytes,), device=device, dtype=torch.uint8)
    exp = torch.from_numpy(oracle.prefix_error_rates(ref, hyp, eos=None, faithful=False))
    args = (tr, th, False, None, False, 1, _cabi.MODE_PREFIX, False, 1)
    for first in (("pdt_lev",), ("pdt_lev_keep", "pdt_lev")):
        for entry in first:
            assert torch.equal(_lev_abi(entry, *args, ws)[0], exp), entry
        ws.copy_(torch.randint(0, 255, (nbytes,), device=device, dtype=torch.uint8))
        assert torch.equal(_lev_abi("pdt_lev_classified", *args, ws)[0], exp), first
