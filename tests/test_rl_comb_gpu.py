"""GPU: time_distributed_return on the scan kernels of csrc/returns.hip and the combinatorics functions on
csrc/combinatorics.hip -- the recorded goldens on the device, then what the goldens cannot reach.

The sweep bound of the returns: a recurrence of k terms rounds each term at most 2 k times (one product and
one sum per step), so |R - R64| <= 2 (k + 1) eps A, k = T - t terms at frame t (t + 1 with ``reverse``),
A the same recurrence over |r| with |gamma|, eps that of the accumulation type.  The chunked kernels round
each term fewer times than that.  float16 / bfloat16 add the rounding of the stored result; they run over
fewer cases than float32 / float64 (T in {1, 33, 65, 1025}, no gamma above 1, no T = 3100): the kernels differ
between the types only in the conversions on load and store, and float16 cannot hold the larger returns.
"""
import os

import numpy as np
import pytest
import torch

from test_rl_comb_cpu import check_combinatorics_goldens, check_errors, check_return_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))

# csrc/returns.hip: 32 steps per lane (columns kernel), 64 per wave pass and 1024 per wave (rows kernel)
SWEEP_T = (1, 2, 31, 32, 33, 63, 64, 65, 100, 1023, 1024, 1025, 3100)
SWEEP_N = (1, 3, 63, 64, 65)
SWEEP_GAMMA = (0.5, 0.999, 1.0, -0.9, 1.01)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "rl_comb.npz"))


def op(r, gamma, batch_first=False, reverse=False):
    return torch.ops.pydrobert_amd.time_distributed_return(r, gamma, batch_first, reverse)


def references(x64, gammas, reverse):
    """(R64, bound / eps), each (T, len(gammas), N), of a time-major float64 (T, N) tensor, on its device."""
    T = x64.shape[0]
    g = torch.tensor(gammas, dtype=torch.float64, device=x64.device).view(-1, 1)
    R = torch.empty((T, len(gammas), x64.shape[1]), dtype=torch.float64, device=x64.device)
    A = torch.empty_like(R)
    acc, mag = torch.zeros_like(R[0]), torch.zeros_like(R[0])
    for s in range(T):
        t = s if reverse else T - 1 - s
        acc = x64[t] + g * acc
        mag = x64[t].abs() + g.abs() * mag
        R[t], A[t] = acc, mag
    terms = torch.arange(1, T + 1, dtype=torch.float64, device=x64.device)
    if not reverse:
        terms = terms.flip(0)
    return R, 2 * (terms + 1).view(T, 1, 1) * A


def reference(x64, gamma, reverse):
    R, unit = references(x64, [gamma], reverse)
    return R[:, 0], unit[:, 0]


def within(got, R64, unit_bound, acc_dtype):
    """got (time-major) against the reference, with the output rounding of a 16-bit type."""
    bound = unit_bound * float(torch.finfo(acc_dtype).eps)
    if got.dtype in (torch.float16, torch.bfloat16):
        bound = bound + 0.5 * float(torch.finfo(got.dtype).eps) * (R64.abs() + bound)
    return bool(((got.double() - R64).abs() <= bound).all())


def test_return_goldens(gold):
    for k in range(int(gold["return_n"])):
        check_return_case(gold, k, DEV)


@pytest.mark.parametrize("T", SWEEP_T)
def test_return_sweep(T):
    base = torch.randn(T, 65, dtype=torch.float64).numpy()
    for dtype in (torch.float32, torch.float64):
        x = torch.from_numpy(base).to(DEV).to(dtype)  # (T, 65) time-major
        xT = x.T.contiguous()  # (65, T) batch-major
        wide = torch.zeros(T, 130, device=DEV, dtype=dtype)  # x in every other column / row
        wide[:, ::2] = x
        wideT = wide.T.contiguous()
        for reverse in (False, True):
            # the references on the host (a loop over T of small vector operations), all gammas at once
            R64s, units = (v.to(DEV) for v in references(x.double().cpu(), SWEEP_GAMMA, reverse))
            for gi, gamma in enumerate(SWEEP_GAMMA):
                R64, unit = R64s[:, gi], units[:, gi]
                for N in SWEEP_N:
                    tag = (T, N, dtype, gamma, reverse)
                    got = op(x[:, :N].contiguous(), gamma, False, reverse)
                    assert got.shape == (T, N) and got.dtype == dtype
                    assert within(got, R64[:, :N], unit[:, :N], dtype), tag
                    got = op(xT[:N].contiguous(), gamma, True, reverse)
                    assert got.shape == (N, T)
                    assert within(got.T, R64[:, :N], unit[:, :N], dtype), tag
                # views: the transposed buffer read as time-major, a column slice, a row slice
                assert within(op(xT.T, gamma, False, reverse), R64, unit, dtype), (T, "transposed", gamma)
                assert within(op(x.T, gamma, True, reverse).T, R64, unit, dtype), (T, "transposed bf", gamma)
                assert within(op(x[:, ::2], gamma, False, reverse), R64[:, ::2], unit[:, ::2], dtype)
                assert within(op(xT[::2], gamma, True, reverse).T, R64[:, ::2], unit[:, ::2], dtype)
                # ... and all 65 columns (64, one more) at a stride of two elements, both layouts
                assert within(op(wide[:, ::2], gamma, False, reverse), R64, unit, dtype), (T, "stride 2", gamma)
                assert within(op(wideT[::2], gamma, True, reverse).T, R64, unit, dtype), (T, "stride 2 bf", gamma)
                assert within(op(wide[:, :128:2], gamma, False, reverse), R64[:, :64], unit[:, :64], dtype)
                assert within(op(wideT[:128:2], gamma, True, reverse).T, R64[:, :64], unit[:, :64], dtype)


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
def test_return_half_types(dtype):
    for T in (1, 33, 65, 1025):
        x = torch.randn(T, 65, device=DEV).to(dtype)
        for gamma in (0.5, 1.0, -0.9):  # (returns that stay inside float16's range)
            for reverse in (False, True):
                R64, unit = reference(x.double(), gamma, reverse)
                assert within(op(x, gamma, False, reverse), R64, unit, torch.float32), (T, gamma)
                assert within(op(x.T.contiguous(), gamma, True, reverse).T, R64, unit, torch.float32), (T, gamma)


def test_return_unsplit_paths():
    """Enough columns (rows) to fill the device: time is not split, whatever T."""
    for T, N, bf in ((70, 131072 + 5, False), (1100, 2048 + 3, True)):
        x = torch.randn(T, N, device=DEV)
        R64, unit = reference(x.double(), 0.9, False)
        got = op(x.T.contiguous(), 0.9, True) if bf else op(x, 0.9)
        assert within(got.T if bf else got, R64, unit, torch.float32), (T, N)


def test_return_long_sequences_stay_finite():
    """T = 200 with gamma 0.5 and 2.0: the reference's gamma**i / gamma**j is 0 / 0 or inf / inf in float32.
    (gamma = 2 in float32: rewards scaled by 2**-100 so that the return itself, ~ 2**199 r, has a value.)"""
    from pydrobert_amd import functional as F

    for dtype in (torch.float32, torch.float64):
        for gamma in (0.5, 2.0):
            x = torch.randn(200, 3, device=DEV, dtype=dtype)
            if gamma > 1 and dtype == torch.float32:
                x = x * 2.0 ** -100
            R64, unit = reference(x.double(), gamma, False)
            assert torch.isfinite(R64).all()
            for bf in (False, True):
                got = F.time_distributed_return(x.T.contiguous() if bf else x, gamma, bf)
                got = got.T if bf else got
                assert torch.isfinite(got).all(), (dtype, gamma, bf)
                assert within(got, R64, unit, dtype), (dtype, gamma, bf)


def test_return_huge_gamma_is_the_plain_recurrence():
    """gamma**32 is not a float32: the kernels must not form it.  Rewards only on the frames that run last."""
    x = torch.zeros(100, 5, device=DEV)
    x[:3] = torch.randn(3, 5, device=DEV)
    R64, unit = reference(x.double(), 1e3, False)
    for bf in (False, True):
        got = op(x.T.contiguous() if bf else x, 1e3, bf)
        got = got.T if bf else got
        assert torch.isfinite(got).all() and within(got, R64, unit, torch.float32)
        assert not got[3:].any()


def test_return_autograd():
    from pydrobert_amd import functional as F

    for bf in (False, True):
        r = torch.randn((3, 7) if bf else (7, 3), device=DEV, dtype=torch.float64, requires_grad=True)
        fn = lambda r: F.time_distributed_return(r, 0.9, bf)  # noqa: E731
        assert torch.autograd.gradcheck(fn, (r,))
        assert torch.autograd.gradgradcheck(fn, (r,))
    r = torch.randn(7, 3, device=DEV, requires_grad=True)
    assert F.time_distributed_return(r, 0.0) is r


def test_return_traceable_on_device():
    from pydrobert_amd import modules as M

    r = torch.randn(40, 6, device=DEV)
    for mod in (M.TimeDistributedReturn(0.9, False), M.TimeDistributedReturn(-0.5, True)):
        exp = mod(r)
        assert torch.equal(torch.jit.script(mod)(r), exp)
        assert torch.equal(torch.jit.trace(mod, r)(r), exp)
        assert torch.equal(torch.compile(mod, backend="eager")(r), exp)


def test_return_determinism_and_streams():
    from pydrobert_amd import functional as F

    for shape, bf in (((1500, 70), False), ((70, 1500), True)):
        r = torch.randn(shape, device=DEV)
        first = F.time_distributed_return(r, 0.97, bf)
        assert torch.equal(F.time_distributed_return(r, 0.97, bf), first)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            other = F.time_distributed_return(r, 0.97, bf)
        side.synchronize()
        assert torch.equal(other, first)


def test_return_no_host_synchronisation():
    from pydrobert_amd import functional as F

    r = torch.randn(100, 8, device=DEV, requires_grad=True)
    rb = torch.randn(8, 2100, device=DEV, requires_grad=True)
    F.time_distributed_return(r.detach(), 0.9)  # (the library is loaded)
    up, upb = torch.ones_like(r), torch.ones_like(rb)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        F.time_distributed_return(r, 0.9).backward(up)
        F.time_distributed_return(rb, 0.9, True).backward(upb)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(r.grad).all() and torch.isfinite(rb.grad).all()


def test_combinatorics_goldens(gold):
    check_combinatorics_goldens(gold, DEV)


def test_combinatorics_errors(gold):
    check_errors(gold, DEV)


def test_cardinality_beyond_full_enumeration():
    from pydrobert_amd import functional as F

    s = F.enumerate_binary_sequences_with_cardinality(60, 2, DEV)
    assert s.shape == (1770, 60) and s.dtype == torch.int64
    assert s.sum(1).eq(2).all() and ((s == 0) | (s == 1)).all()
    value = (s << torch.arange(60, device=DEV)).sum(1)
    assert (value[1:] > value[:-1]).all()
    n = F.binomial_coefficient(torch.tensor(60, device=DEV), torch.tensor(2, device=DEV))
    assert int(n) == s.shape[0]


def test_cardinality_tensor_form():
    from pydrobert_amd import functional as F

    length = torch.tensor([[0], [1], [7], [12]], device=DEV)
    count = torch.tensor([0, 1, 3, 6, 9], device=DEV)
    support, binom = F.enumerate_binary_sequences_with_cardinality(length, count)
    assert support.shape == (4, 5, 924, 12) and binom.shape == (4, 5)
    for i, l in enumerate(length.flatten().tolist()):
        for j, c in enumerate(count.tolist()):
            exp = F.enumerate_binary_sequences_with_cardinality(l, c, DEV)
            n = exp.shape[0]
            assert int(binom[i, j]) == n
            assert torch.equal(support[i, j, :n, :l], exp)
            assert not support[i, j, n:].any() and not support[i, j, :, l:].any()


def test_vocab_enumeration_closed_form():
    from pydrobert_amd import functional as F

    cases = ((6, 3, torch.int64), (1, 5, torch.int64), (7, 5, torch.int32), (18, 2, torch.uint8),
             (18, 2, torch.int64), (3, 6, torch.float64), (5, 1, torch.float32))  # fmt: skip
    for L, V, dtype in cases:
        got = F.enumerate_vocab_sequences(L, V, DEV, dtype)
        s = torch.arange(V ** L, device=DEV).unsqueeze(1)
        powers = torch.tensor([V ** t for t in range(L)], device=DEV)
        assert got.shape == (V ** L, L) and got.dtype == dtype
        assert torch.equal(got.long(), (s // powers) % V), (L, V, dtype)


def srswor_rule(total, given, u):
    out = torch.empty_like(u)
    ell = given.clone()
    for t in range(u.shape[1]):
        rem = (total - t).clamp_min(1)
        b = u[:, t] < ell.float() / rem.float()
        out[:, t] = b.float()
        ell = ell - b.long()
    return out


def test_sampler_exact_against_the_rule():
    for B in (1, 64, 65, 1000):
        for O in (1, 7, 64, 65, 130):
            total = torch.randint(0, O + 1, (B,), device=DEV)
            total[::5] = 0
            total[1::7] = O
            kind = torch.arange(B, device=DEV) % 3  # 0: none, 1: all, 2: between
            between = (torch.rand(B, device=DEV) * (total + 1)).long().clamp_max(total)
            given = torch.where(kind == 0, torch.zeros_like(total), torch.where(kind == 1, total, between))
            u = torch.rand(B, O, device=DEV)
            got = torch.ops.pydrobert_amd.srswor(total, given, u)
            assert got.dtype == torch.float32 and got.shape == (B, O)
            assert torch.equal(got, srswor_rule(total, given, u)), (B, O)
            assert torch.equal(got.sum(1).long(), given), (B, O)


def test_sampler_properties():
    from pydrobert_amd import functional as F

    total = torch.randint(0, 40, (5, 1, 7), device=DEV)
    given = (torch.rand(3, 1, device=DEV) * (total + 1)).long().clamp_max(total)
    b = F.simple_random_sampling_without_replacement(total, given, 45)
    assert b.shape == (5, 3, 7, 45) and b.dtype == torch.get_default_dtype() and b.device == DEV
    assert torch.equal(b.sum(-1).long(), given)
    beyond = torch.arange(45, device=DEV) >= total.expand(5, 3, 7).unsqueeze(-1)
    assert not (b * beyond).any()
    assert F.simple_random_sampling_without_replacement(total, given).shape == (5, 3, 7, int(total.max()))
    torch.manual_seed(5)
    first = F.simple_random_sampling_without_replacement(total, given, 45)
    torch.manual_seed(5)
    assert torch.equal(F.simple_random_sampling_without_replacement(total, given, 45), first)


def test_sampler_uniform_over_subsets():
    from pydrobert_amd import functional as F

    n = 200000
    torch.manual_seed(0)
    b = F.simple_random_sampling_without_replacement(
        torch.full((n,), 6, device=DEV), torch.full((n,), 3, device=DEV)
    )
    assert b.shape == (n, 6)
    code = (b.long() << torch.arange(6, device=DEV)).sum(1)
    freq = torch.bincount(code, minlength=64).double() / n
    assert int((freq > 0).sum()) == 20
    sd = (0.05 * 0.95 / n) ** 0.5
    assert ((freq[freq > 0] - 0.05).abs() <= 5 * sd).all(), freq[freq > 0]


def test_sampler_errors():
    from pydrobert_amd import functional as F

    t = lambda v: torch.tensor(v, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="given_count"):
        F.simple_random_sampling_without_replacement(t([3, 2]), t([1, 3]))
    with pytest.raises(RuntimeError, match="out_size"):
        F.simple_random_sampling_without_replacement(t([3, 5]), t([1, 2]), 4)
