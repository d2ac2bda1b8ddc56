"""GPU: pdt_oc_expand through the C ABI on synthetic class bitmasks, against a numpy expansion.
The ABI takes any C at least the largest set -- C > R included -- and either row layout, so these
cases reach shapes the operator never passes: odd and even C over and beyond a 2 048-element run of
a tile, C > R, the batch-first layout.  Targets start as a sentinel, so an element left unwritten
shows up."""
import numpy as np
import pytest
import torch

from pydrobert_amd import _cabi

pytestmark = pytest.mark.gpu
SENTINEL = 0x7777777777


def draw_masks(rng, R, Hout, N, cmax):
    """(Hout, N, W) uint32 words with at most cmax of the first R bits set per row, and tokens."""
    W = max(1, (R + 31) // 32)
    bits = rng.random((Hout, N, R)) < rng.uniform(0.05, 0.9)
    bits &= np.cumsum(bits, -1) <= cmax
    full = np.zeros((Hout, N, W * 32), bool)
    full[..., :R] = bits
    words = (full.reshape(Hout, N, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)
    tokens = rng.integers(-(1 << 40), 1 << 40, (N, max(R, 1)))
    return words.astype(np.uint32), tokens, bits


def expand(bits, tokens, C, padding):
    Hout, N, R = bits.shape
    out = np.full((Hout, N, C), padding, np.int64)
    h, n, k = np.nonzero(bits)
    rank = (np.cumsum(bits, -1) - 1)[h, n, k]
    out[h, n, rank] = tokens[n, k]
    return out


def run(device, words, tokens, R, Hout, N, C, padding, batch_first):
    bm = torch.from_numpy(words.view(np.int32).copy()).to(device)
    tab = torch.from_numpy(tokens).to(device)
    if batch_first:
        tgt = torch.full((N, Hout, C), SENTINEL, dtype=torch.long, device=device)
        sh, sn = tgt.stride(1), tgt.stride(0)
    else:
        tgt = torch.full((Hout, N, C), SENTINEL, dtype=torch.long, device=device)
        sh, sn = tgt.stride(0), tgt.stride(1)
    L = _cabi.lib()
    rc = L.pdt_oc_expand(_cabi.ptr(bm), _cabi.ptr(tab), R, Hout, N, C, padding, _cabi.ptr(tgt), sh, sn,
                         _cabi.stream_ptr(device))
    _cabi.check(rc, "pdt_oc_expand")
    torch.cuda.synchronize(device)
    out = tgt.cpu().numpy()
    return out.transpose(1, 0, 2) if batch_first else out


# (R, C, cmax): NB = 64 / Wp utterances per tile; runs of NB * C elements below, at and beyond 2 048
CASES = [
    (16, 20, 16),     # C > R, NB = 64: 1 280 elements
    (32, 32, 32),     # NB * C = 2 048 exactly
    (32, 34, 32),     # 2 176: beyond one tile's 2 048
    (40, 33, 33),     # odd C
    (300, 130, 130),  # NB = 4: 520
    (300, 300, 300),  # 1 200
    (300, 640, 300),  # C > R: 2 560
    (512, 512, 512),  # 2 048
    (512, 2000, 200), # far beyond
    (700, 90, 90),    # W > 16
]


@pytest.mark.parametrize("R,C,cmax", CASES)
@pytest.mark.parametrize("N", [1, 6, 67])
def test_expand_any_width(device, R, C, cmax, N):
    rng = np.random.default_rng(R * 7919 + C * 31 + N)
    Hout = 11
    words, tokens, bits = draw_masks(rng, R, Hout, N, cmax)
    exp = expand(bits, tokens, C, -100)
    got = run(device, words, tokens, R, Hout, N, C, -100, False)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("R,C", [(48, 50), (300, 152), (512, 401)])
def test_expand_batch_first_layout_and_padding(device, R, C):
    rng = np.random.default_rng(R + C)
    Hout, N = 9, 13
    words, tokens, bits = draw_masks(rng, R, Hout, N, min(R, C))
    exp = expand(bits, tokens, C, 1 << 41)
    assert np.array_equal(run(device, words, tokens, R, Hout, N, C, 1 << 41, True), exp)
    assert np.array_equal(run(device, words, tokens, R, Hout, N, C, 1 << 41, False), exp)
