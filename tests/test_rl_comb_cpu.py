"""CPU: the functional namespace is complete, and the torch bodies of time_distributed_return and the
combinatorics functions reproduce what the reference recorded (tests/golden/make_rl_comb_golden.py).

Tolerances of the returns: the reference's product with a matrix of power ratios was recorded only where
it lies within (T + 8) eps A[t] of a float64 recurrence, A[t] = sum_{t' >= t} |gamma|^(t' - t) |r[t']|; a
T-term float32 recurrence adds 2 (T + 1) eps A[t]: (3 T + 10) eps A[t].  float64: 1e-12 relative to A.
"""
import inspect
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "rl_comb.npz"))


@pytest.fixture(scope="module")
def sigs():
    with open(os.path.join(HERE, "golden", "rl_comb_signatures.json")) as f:
        return json.load(f)


def upstream(shape, dtype):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.7).reshape(shape).to(dtype)


def magnitude(r, gamma, time_dim, reverse=False):
    """A: the recurrence of |r| with |gamma| in float64 (reverse: the adjoint's)."""
    x = r.detach().double().abs().movedim(time_dim, 0)
    A = torch.zeros_like(x)
    acc = torch.zeros_like(x[0])
    T = x.shape[0]
    for s in range(T):
        t = s if reverse else T - 1 - s
        acc = x[t] + abs(gamma) * acc
        A[t] = acc
    return A.movedim(0, time_dim)


def check_return_case(gold, k, device):
    from pydrobert_amd import functional as F

    pre = "return_{}_".format(k)
    kw = json.loads(str(gold[pre + "kw"]))
    r = torch.from_numpy(gold[pre + "r"]).to(device).requires_grad_(True)
    R = F.time_distributed_return(r, **kw)
    assert R.dtype == r.dtype and R.shape == r.shape
    if kw["gamma"] == 0:
        assert R is r
    g = upstream(tuple(R.shape), r.dtype).to(device)
    (gr,) = torch.autograd.grad(R, r, g)
    td = 1 if kw["batch_first"] else 0
    T = r.shape[td]
    rel = 1e-12 if r.dtype == torch.float64 else (3 * T + 10) * float(torch.finfo(r.dtype).eps)
    for got, name, src, rev in ((R, "R", r, False), (gr, "gr", g, True)):
        exp = torch.from_numpy(gold[pre + name]).double()
        bound = rel * magnitude(src.cpu(), kw["gamma"], td, rev)
        err = (got.detach().cpu().double() - exp).abs()
        assert (err <= bound).all(), (k, kw, name, float((err - bound).max()))


def test_namespaces_complete(sigs):
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    missing = [n for n in sigs["functional_all"] if n not in F.__all__ or not hasattr(F, n)]
    assert not missing, missing
    assert "TimeDistributedReturn" in sigs["modules_all"]
    assert "TimeDistributedReturn" in M.__all__ and hasattr(M, "TimeDistributedReturn")


def _bind(fn, params):
    sig = inspect.signature(fn)
    got = [p for p in sig.parameters.values() if p.name != "self" and not p.name.startswith("_")]
    assert [p.name for p in got] == [p[0] for p in params], (fn, got)
    for p, (name, has_default, kind, default) in zip(got, params):
        assert p.kind.name == kind, (fn, name)
        assert (p.default is not inspect.Parameter.empty) == has_default, (fn, name)
        if has_default:
            assert repr(p.default) == default, (fn, name, p.default)


def test_signatures(sigs):
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    assert len(sigs["functional"]) == 6
    for name, params in sigs["functional"].items():
        _bind(getattr(F, name), params)
    for name, methods in sigs["modules"].items():
        cls = getattr(M, name)
        _bind(cls.__init__, methods["__init__"])
        _bind(cls.forward, methods["forward"])


def test_return_goldens(gold):
    n = int(gold["return_n"])
    assert n == 192 and json.loads(str(gold["return_dropped"])) == []
    for k in range(n):
        check_return_case(gold, k, "cpu")


def test_return_module_and_edges():
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    m = M.TimeDistributedReturn(0.5, True)
    assert "gamma=0.5" in repr(m) and "batch_first=True" in repr(m)
    r = torch.tensor([[1.0, 2.0, 4.0]])
    assert torch.equal(m(r), torch.tensor([[3.0, 4.0, 4.0]]))
    assert torch.equal(torch.jit.script(m)(r), m(r))
    assert F.time_distributed_return(torch.zeros(0, 3), 0.5).shape == (0, 3)
    assert F.time_distributed_return(torch.zeros(3, 0), 0.5, True).shape == (3, 0)
    # where the reference's power ratios leave float32: finite, and the recurrence
    r = torch.randn(200, 3)
    for gamma in (0.5, 2.0):
        x = r * 2.0 ** -100 if gamma > 1 else r
        R = F.time_distributed_return(x, gamma)
        assert torch.isfinite(R).all()
        exp = torch.zeros(3, dtype=torch.float64)
        for t in range(199, -1, -1):
            exp = x[t].double() + gamma * exp
        A = magnitude(x, gamma, 0)
        assert ((R[0].double() - exp).abs() <= 2 * 201 * float(torch.finfo(torch.float32).eps) * A[0]).all()


def check_combinatorics_goldens(gold, device):
    from pydrobert_amd import functional as F

    dev = torch.device(device)
    count = torch.arange(67, device=dev).view(1, 67).expand(67, 67)
    length = torch.arange(67, device=dev).view(67, 1).expand(67, 67)
    assert np.array_equal(F.binomial_coefficient(length[:21], count[:21]).cpu().numpy(), gold["binom_small"])
    big = F.binomial_coefficient(length, count)
    assert big.dtype == torch.int64 and big.device.type == dev.type
    assert np.array_equal(big.cpu().numpy(), gold["binom_large"])
    for k in range(int(gold["vocab_n"])):
        kw = json.loads(str(gold["vocab_{}_kw".format(k)]))
        exp = gold["vocab_{}_out".format(k)]
        for dtype in (torch.int64, torch.int32, torch.uint8, torch.float32, torch.float64, torch.int16, torch.float16):
            got = F.enumerate_vocab_sequences(device=dev, dtype=dtype, **kw)
            assert got.dtype == dtype and got.device.type == dev.type and tuple(got.shape) == exp.shape, (kw, dtype)
            assert np.array_equal(got.cpu().double().numpy(), exp.astype(np.float64)), (kw, dtype)
    assert np.array_equal(F.enumerate_vocab_sequences(3, 3, dev, torch.float32).cpu().numpy(), gold["vocab_float"])
    assert np.array_equal(F.enumerate_binary_sequences(4, dev).cpu().numpy(), gold["binary_4"])
    for k in range(int(gold["card_n"])):
        kw = json.loads(str(gold["card_{}_kw".format(k)]))
        exp = gold["card_{}_out".format(k)]
        got = F.enumerate_binary_sequences_with_cardinality(kw["length"], kw["count"], dev)
        assert got.dtype == torch.int64 and tuple(got.shape) == exp.shape, kw
        assert np.array_equal(got.cpu().numpy(), exp), kw
    got = F.enumerate_binary_sequences_with_cardinality(5, 2, dev, torch.float32)
    assert got.dtype == torch.float32 and got.sum(1).eq(2).all() and got.shape == (10, 5)
    length = torch.from_numpy(gold["cardt_length"]).to(dev)
    count = torch.from_numpy(gold["cardt_count"]).to(dev)
    support, binom = F.enumerate_binary_sequences_with_cardinality(length, count)
    assert np.array_equal(binom.cpu().numpy(), gold["cardt_binom"])
    assert tuple(support.shape) == tuple(gold["cardt_shape"]) and support.dtype == torch.int64
    for i in range(3):
        for j in range(4):
            n, l = int(binom[i, j]), int(length[i, 0])
            assert np.array_equal(support[i, j, :n, :l].cpu().numpy(), gold["cardt_valid_{}_{}".format(i, j)])
            assert not support[i, j, n:].any() and not support[i, j, :, l:].any()  # padding is zeros here


def test_combinatorics_goldens(gold):
    check_combinatorics_goldens(gold, "cpu")


def error_cases(device):
    from pydrobert_amd import functional as F
    from pydrobert_amd import modules as M

    def t(v):
        return torch.tensor(v, device=device)

    return {
        "return_1d": lambda: F.time_distributed_return(torch.randn(5, device=device), 0.5),
        "return_3d": lambda: F.time_distributed_return(torch.randn(5, 2, 2, device=device), 0.5),
        "ctor_gamma": lambda: M.TimeDistributedReturn("a", False),
        "ctor_batch_first": lambda: M.TimeDistributedReturn(0.5, 1),
        "vocab_length_negative": lambda: F.enumerate_vocab_sequences(-1, 2, device),
        "vocab_size_zero": lambda: F.enumerate_vocab_sequences(2, 0, device),
        "binary_length_negative": lambda: F.enumerate_binary_sequences(-1, device),
        "binom_length_negative": lambda: F.binomial_coefficient(t([-1, 2]), t([0, 1])),
        "binom_count_negative": lambda: F.binomial_coefficient(t([1, 2]), t([0, -1])),
        "card_mixed": lambda: F.enumerate_binary_sequences_with_cardinality(3, t(1)),
        "card_mixed_other": lambda: F.enumerate_binary_sequences_with_cardinality(t(3), 1),
        "card_length_negative": lambda: F.enumerate_binary_sequences_with_cardinality(-1, 0, device),
        "srswor_given_exceeds": lambda: F.simple_random_sampling_without_replacement(t([3, 2]), t([1, 3])),
        "srswor_out_size_small": lambda: F.simple_random_sampling_without_replacement(t([3, 5]), t([1, 2]), 4),
    }


def check_errors(gold, device):
    from pydrobert_amd import functional as F

    recorded = json.loads(str(gold["errors"]))
    cases = error_cases(device)
    assert sorted(cases) == sorted(recorded)
    for key, fn in cases.items():
        assert recorded[key] != "none", key
        with pytest.raises(Exception) as info:
            fn()
        assert type(info.value).__name__ == recorded[key], (key, info.value)
    # the documented differences: overflow is refused, not wrapped; the enumeration's own limits
    t = torch.tensor([67], device=device)
    with pytest.raises(RuntimeError, match="overflow"):
        F.binomial_coefficient(t, t)
    with pytest.raises(RuntimeError, match="limited to 62"):
        F.enumerate_binary_sequences_with_cardinality(63, 1, device)
    with pytest.raises(RuntimeError, match="too long"):
        F.enumerate_vocab_sequences(32, 2, device)


def test_errors(gold):
    check_errors(gold, "cpu")


def test_sampler_cpu_body():
    from pydrobert_amd import functional as F

    total = torch.tensor([[6], [0], [9]])
    given = torch.tensor([0, 3, 6, 9]).clamp_max(total)
    b = F.simple_random_sampling_without_replacement(total, given, 11)
    assert b.shape == (3, 4, 11) and b.dtype == torch.get_default_dtype()
    assert torch.equal(b.sum(-1).long(), given)
    assert not (b * (torch.arange(11) >= total.unsqueeze(-1))).any()
    assert F.simple_random_sampling_without_replacement(total, given).shape == (3, 4, 9)
