"""GPU: optimal_completion's expansion (class bitmasks -> int64 targets) bit for bit against the
oracle over the shapes its launcher tells apart: tiles of NB = 64 / Wp utterances (Wp = mask
words per row rounded up to a power of two: NB = 64 ... 4 for R <= 512), a last tile that is
not full, a single tile, one value of h, odd widths (element-wise stores), tiny and large C,
another padding value, int32 inputs, tokens beyond int32 and references longer than 512."""
import os

import numpy as np
import pytest
import torch

import oracle
from pydrobert_amd import functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def check(got, exp, padding=-100, batch_first=False):
    """got (torch) against exp (numpy): equal up to exp's width, padding beyond it."""
    got = got.cpu()
    if batch_first:
        got = got.transpose(0, 1)
        exp = exp.transpose(1, 0, 2)
    Ce = exp.shape[2]
    assert got.shape[:2] == exp.shape[:2] and got.shape[2] >= Ce
    assert torch.equal(got[:, :, :Ce], torch.from_numpy(np.ascontiguousarray(exp)))
    assert bool((got[:, :, Ce:] == padding).all())


def draw(rng, T_ref, T_hyp, N, V):
    return rng.integers(0, V, (T_ref, N)), rng.integers(0, V, (T_hyp, N))


@pytest.mark.parametrize("N", [4096, 4095])
def test_c2_shape_sampled(device, N):
    rng = np.random.default_rng(0x5EED0002)
    ref, hyp = draw(rng, 512, 512, N, 256)
    oc = F.optimal_completion(T(ref, device), T(hyp, device), warn=False)
    assert oc.shape[:2] == (513, N)
    # the first and last tiles whole, and a spread over the batch
    idx = np.unique(np.concatenate([np.arange(8), np.arange(N - 9, N), np.arange(0, N, 31)]))
    exp = oracle.optimal_completion(ref[:, idx], hyp[:, idx], faithful=False)
    got = oc[:, torch.from_numpy(idx).to(device)]
    assert got.shape[2] >= exp.shape[2]
    check(got[:, :, : exp.shape[2]], exp)
    # the width is the batch's largest set, padding after every set
    valid = oc != -100
    assert int(valid.sum(2).max()) == oc.shape[2]
    assert bool((valid[:, :, 1:] <= valid[:, :, :-1]).all())


@pytest.mark.parametrize("R", [1, 20, 40, 70, 100, 200, 300, 512, 513, 700])
@pytest.mark.parametrize("N", [1, 3, 4, 37])
def test_reference_lengths_and_batch_sizes(device, R, N):
    rng = np.random.default_rng(R * 1000 + N)
    ref, hyp = draw(rng, R, max(1, R // 2 + 3), N, max(2, R // 3))
    exp = oracle.optimal_completion(ref, hyp, faithful=False)
    check(F.optimal_completion(T(ref, device), T(hyp, device), warn=False), exp)


@pytest.mark.parametrize("batch_first", [False, True])
@pytest.mark.parametrize("include_eos", [False, True])
def test_ragged_with_eos(device, batch_first, include_eos):
    rng = np.random.default_rng(7 + batch_first + 2 * include_eos)
    N, Tr, Th, V = 45, 300, 260, 50
    eos = V
    ref, hyp = draw(rng, Tr, Th, N, V)
    for x, Tx in ((ref, Tr), (hyp, Th)):
        lens = rng.integers(0, Tx, N)
        for n in range(N):
            x[lens[n]:, n] = eos
    if batch_first:
        ref, hyp = ref.T.copy(), hyp.T.copy()
    kw = dict(eos=eos, include_eos=include_eos, batch_first=batch_first)
    exp = oracle.optimal_completion(ref, hyp, faithful=False, **kw)
    got = F.optimal_completion(T(ref, device), T(hyp, device), warn=False, **kw)
    if batch_first:
        assert got.shape[0] == N
        got, exp = got.transpose(0, 1), exp.transpose(1, 0, 2)
    check(got, exp)


def test_string_golden(device):
    g = np.load(os.path.join(G, "string_s2.npz"))
    eos = int(g["eos"])
    for inc in (0, 1):
        for bf in (0, 1):
            ref, hyp = (g["ref"].T, g["hyp"].T) if bf else (g["ref"], g["hyp"])
            for ex in (0, 1):
                got = F.optimal_completion(T(ref, device), T(hyp, device), eos=eos, include_eos=bool(inc),
                                           batch_first=bool(bf), exclude_last=bool(ex), warn=False)
                assert np.array_equal(got.cpu().numpy(), g["oc_i{}_b{}_x{}".format(inc, bf, ex)])


def test_one_value_of_h(device):
    rng = np.random.default_rng(11)
    ref, hyp = draw(rng, 400, 1, 4096, 30)
    exp = oracle.optimal_completion(ref[:, :64], hyp[:, :64], exclude_last=True, faithful=False)
    got = F.optimal_completion(T(ref, device), T(hyp, device), exclude_last=True, warn=False)
    assert got.shape[0] == 1
    check(got[:, :64, : exp.shape[2]], exp)
    # an empty hypothesis: one row as well
    hyp0 = np.zeros((0, 9), np.int64)
    exp = oracle.optimal_completion(ref[:, :9], hyp0, faithful=False)
    check(F.optimal_completion(T(ref[:, :9], device), T(hyp0, device), warn=False), exp)


def test_tiny_and_large_sets(device):
    rng = np.random.default_rng(12)
    N = 10
    # one token everywhere: C = 1
    ref = np.full((480, N), 5)
    hyp = rng.integers(0, 9, (300, N))
    exp = oracle.optimal_completion(ref, hyp, faithful=False)
    got = F.optimal_completion(T(ref, device), T(hyp, device), warn=False)
    assert got.shape[2] == 1
    check(got, exp)
    # all-distinct references against an empty-ish hypothesis: sets of hundreds of tokens
    ref = np.stack([rng.permutation(512) for _ in range(N)], 1)
    hyp = rng.integers(600, 700, (400, N))
    exp = oracle.optimal_completion(ref, hyp, faithful=False)
    got = F.optimal_completion(T(ref, device), T(hyp, device), warn=False)
    assert got.shape[2] > 200
    check(got, exp)


@pytest.mark.parametrize("padding", [-7, 3, 1 << 40])
def test_padding_values(device, padding):
    rng = np.random.default_rng(13)
    ref, hyp = draw(rng, 450, 300, 13, 90)
    exp = oracle.optimal_completion(ref, hyp, padding=padding, faithful=False)
    got = F.optimal_completion(T(ref, device), T(hyp, device), padding=padding, warn=False)
    check(got, exp, padding=padding)


def test_int32_inputs_and_wide_tokens(device):
    rng = np.random.default_rng(14)
    ref, hyp = draw(rng, 500, 480, 21, 200)
    base = F.optimal_completion(T(ref, device), T(hyp, device), warn=False)
    check(base, oracle.optimal_completion(ref, hyp, faithful=False))
    got = F.optimal_completion(T(ref.astype(np.int32), device), T(hyp.astype(np.int32), device), warn=False)
    assert got.dtype == torch.long and torch.equal(got, base)
    # tokens at and above 2^31: the tables stay int64
    for off in ((1 << 40) + 12345, (1 << 31) - 100):
        r2, h2 = ref + off, hyp + off
        exp = oracle.optimal_completion(r2, h2, faithful=False)
        got = F.optimal_completion(T(r2, device), T(h2, device), warn=False)
        check(got, exp)
        valid = base != -100
        assert torch.equal(got[valid], base[valid] + off)


@pytest.mark.parametrize("R,L", [(512, 199), (512, 399), (300, 151), (64, 63), (64, 40)])
def test_even_sets_over_many_pairs(device, R, L):
    """Even C with runs of NB * C elements across the 16-byte store blocks: (512, 199) -> C = 200,
    NB * C = 800; (512, 399) -> 1 600; (64, 63) -> NB = 32, 2 048 elements; (64, 40) -> odd C = 41."""
    rng = np.random.default_rng(R + L)
    N = 9
    ref = np.stack([rng.permutation(R) for _ in range(N)], 1)
    hyp = rng.integers(R + 100, R + 200, (L, N))
    exp = oracle.optimal_completion(ref, hyp, faithful=False)
    got = F.optimal_completion(T(ref, device), T(hyp, device), warn=False)
    check(got, exp)
