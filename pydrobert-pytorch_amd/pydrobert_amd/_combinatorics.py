"""Combinatorics on MI355X (reference _combinatorics.py:27-412): enumerations of small discrete supports,
binomial coefficients, and draws of binary vectors of fixed cardinality.

On a ROCm device every result is written by a kernel of ``csrc/combinatorics.hip``.  The enumeration with a
given cardinality unranks each row in the combinatorial number system, so the ``2**length`` rows of the full
enumeration are never formed; the sampler is one launch over explicit uniforms.  CPU tensors, and the
``device="cpu"`` default of the enumerations, take torch bodies written from the same formulas.
"""
from typing import Any, Optional, Tuple, Union

import torch
from torch.distributions import constraints
from torch.distributions.utils import lazy_property
from torch.library import custom_op

from . import _cabi, argcheck

__all__ = [
    "BinaryCardinalityConstraint",
    "SimpleRandomSamplingWithoutReplacement",
    "binomial_coefficient",
    "enumerate_binary_sequences",
    "enumerate_binary_sequences_with_cardinality",
    "enumerate_vocab_sequences",
    "simple_random_sampling_without_replacement",
]

MAX_BINOMIAL_LENGTH = 66  # the largest length whose every coefficient fits int64
MAX_CARDINALITY_LENGTH = 62
_OUT_TYPES = {torch.int64: 0, torch.int32: 1, torch.uint8: 2, torch.float32: 3, torch.float64: 4}
_FLAG_NEGATIVE, _FLAG_OVERFLOW = 1, 2


def _pascal_host() -> torch.Tensor:
    """(67, 67) int64, [l, c] = C(l, c), built with Python integers."""
    n = MAX_BINOMIAL_LENGTH + 1
    rows = [[0] * n for _ in range(n)]
    for l in range(n):
        rows[l][0] = 1
        for c in range(1, l + 1):
            rows[l][c] = rows[l - 1][c - 1] + rows[l - 1][c]
    assert max(rows[-1]) < 2 ** 63
    return torch.tensor(rows, dtype=torch.int64)


_PASCAL = {}


def _pascal(device: torch.device) -> torch.Tensor:
    """The table on ``device``, cached: copied once from pinned memory without blocking the host, with an
    event that the stream of every later call waits on (as ``_feats._taps`` keeps its filters)."""
    entry = _PASCAL.get(device)
    if entry is None:
        host = _pascal_host()
        if device.type == "cpu":
            entry = (host, host, None)
        else:
            host = host.pin_memory()
            with torch.cuda.device(device):
                dev = host.to(device, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record()
            entry = (host, dev, ready)
        _PASCAL[device] = entry
    if entry[2] is not None:
        torch.cuda.current_stream(device).wait_event(entry[2])
    return entry[1]


def _full_device(device: torch.device) -> torch.device:
    if device.type == "cuda" and device.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return device


def _raise_binomial_flags(flags: int) -> None:
    if flags & _FLAG_NEGATIVE:
        raise RuntimeError("length and count must be non-negative")
    if flags & _FLAG_OVERFLOW:
        raise RuntimeError(
            "binomial_coefficient: a length above {} has coefficients that overflow int64".format(MAX_BINOMIAL_LENGTH)
        )


def _binomial(length: torch.Tensor, count: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(binom, flags): the broadcast coefficients and a (1,) int32 word of _FLAG_* bits, not yet read."""
    length, count = torch.broadcast_tensors(length.long(), count.long())
    device = _full_device(length.device)
    if device.type == "cpu":
        flags = ((length < 0) | (count < 0)).any().int() * _FLAG_NEGATIVE
        flags = flags + (length > MAX_BINOMIAL_LENGTH).any().int() * _FLAG_OVERFLOW
        l, c = length.clamp(0, MAX_BINOMIAL_LENGTH), count.clamp(0, MAX_BINOMIAL_LENGTH)
        binom = _pascal(device)[l, c].masked_fill(count > length, 0)
        return binom, flags.view(1)
    _cabi.require_hip(length, count)
    length, count = length.contiguous(), count.contiguous()
    binom = torch.empty(length.shape, dtype=torch.int64, device=device)
    flags = torch.zeros((1,), dtype=torch.int32, device=device)
    table = _pascal(device)
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_binomial_coefficient(
            _cabi.ptr(length), _cabi.ptr(count), length.numel(), _cabi.ptr(table), _cabi.ptr(binom), _cabi.ptr(flags),
            _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_binomial_coefficient")
    return binom, flags


def binomial_coefficient(length: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """``length`` choose ``count`` for broadcast long tensors (reference _combinatorics.py:123-189): a gather
    from a Pascal table of lengths up to 66.  ``count > length`` gives 0; a negative value raises, and so does
    a length above 66, whose coefficients overflow int64 (the reference returns wrapped values there)."""
    binom, flags = _binomial(length, count)
    if binom.numel():
        _raise_binomial_flags(int(flags.item()))  # (the one host read)
    return binom


def _int_or_float_dtype(dtype: torch.dtype) -> torch.dtype:
    """The type a kernel writes for a result of ``dtype``: itself when there is a kernel for it, else int32 or
    float32, cast afterwards."""
    if dtype in _OUT_TYPES:
        return dtype
    return torch.float32 if (dtype.is_floating_point or dtype.is_complex) else torch.int32


def enumerate_vocab_sequences(
    length: int,
    vocab_size: int,
    device: torch.device = torch.device("cpu"),
    dtype: torch.dtype = torch.long,
) -> torch.Tensor:
    """All ``vocab_size ** length`` sequences of ``length`` values below ``vocab_size`` (reference
    _combinatorics.py:208-251): ``support[s, t] = (s // vocab_size ** t) % vocab_size``."""
    if length < 0:
        raise RuntimeError("length must be non-negative, got {}".format(length))
    if vocab_size <= 0:
        raise RuntimeError("vocab_size must be positive, got {}".format(vocab_size))
    device = _full_device(torch.device(device))
    rows = vocab_size ** length if vocab_size > 1 else 1
    if rows >= 2 ** 32 or length >= 2 ** 30:
        _cabi.check(_cabi.PDT_E_TOO_LONG, "pdt_enumerate_vocab_sequences")
    if device.type == "cpu":
        s = torch.arange(rows).unsqueeze(1)
        powers = torch.tensor([vocab_size ** t for t in range(length)], dtype=torch.long)
        return ((s // powers) % vocab_size).to(dtype)
    written = _int_or_float_dtype(dtype)
    out = torch.empty((rows, length), dtype=written, device=device)
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_enumerate_vocab_sequences(
            length, vocab_size, _OUT_TYPES[written], _cabi.ptr(out) if out.numel() else None, _cabi.stream_ptr(device)
        )
    _cabi.check(rc, "pdt_enumerate_vocab_sequences")
    return out.to(dtype)


def enumerate_binary_sequences(
    length: int, device: torch.device = torch.device("cpu"), dtype: torch.dtype = torch.long
) -> torch.Tensor:
    """All ``2 ** length`` binary sequences of ``length`` (reference _combinatorics.py:263-304)."""
    return enumerate_vocab_sequences(length, 2, device, dtype)


def _cardinality_rows_torch(length: int, count: int, rows: int) -> torch.Tensor:
    """(rows, length) int64 on the CPU: row k unranked in the combinatorial number system."""
    table = _pascal(torch.device("cpu"))
    k = torch.arange(rows)
    out = torch.zeros((rows, length), dtype=torch.long)
    for i in range(count, 0, -1):
        # the largest p with C(p, i) <= k (the column ascends in p)
        p = torch.searchsorted(table[:length, i].contiguous(), k, right=True) - 1
        out.scatter_(1, p.unsqueeze(1), 1)
        k = k - table[p, i]
    return out


def _cardinality_hip(length, count, length0, count0, B, rows, width, written, device):
    out = torch.empty((B, rows, width), dtype=written, device=device)
    table = _pascal(device)
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_enumerate_cardinality(
            _cabi.ptr(length), _cabi.ptr(count), length0, count0, B, rows, width, _cabi.ptr(table),
            _OUT_TYPES[written], _cabi.ptr(out) if out.numel() else None, _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_enumerate_cardinality")
    return out


def _check_cardinality_length(length: int) -> None:
    if length > MAX_CARDINALITY_LENGTH:
        raise RuntimeError(
            "enumerate_binary_sequences_with_cardinality: lengths are limited to {}, got {}".format(
                MAX_CARDINALITY_LENGTH, length
            )
        )


def _cardinality_int(length: int, count: int, device, dtype: torch.dtype) -> torch.Tensor:
    if length < 0:
        raise RuntimeError("length must be non-negative, got {}".format(length))
    _check_cardinality_length(length)
    device = _full_device(torch.device(device))
    rows = int(_pascal_host_entry(length, count)) if 0 <= count <= length else 0
    if device.type == "cpu":
        return _cardinality_rows_torch(length, max(count, 0), rows).to(dtype)
    written = _int_or_float_dtype(dtype)
    if rows == 0:
        return torch.empty((0, length), dtype=dtype, device=device)
    return _cardinality_hip(None, None, length, count, 1, rows, length, written, device)[0].to(dtype)


def _pascal_host_entry(length: int, count: int) -> int:
    return int(_pascal(torch.device("cpu"))[length, count])


def _cardinality_tensor(length: torch.Tensor, count: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    binom, flags = _binomial(length, count)
    length_b, count_b = torch.broadcast_tensors(length.long(), count.long())
    device = binom.device
    if binom.numel() == 0:
        return torch.empty(binom.shape + (0, 0), dtype=torch.long, device=device), binom
    # the one host read: the flag word and the two maxima
    stats = torch.stack([flags[0].long().to(device), binom.max(), length_b.max()]).tolist()
    _raise_binomial_flags(stats[0])
    rows, width = stats[1], stats[2]
    _check_cardinality_length(width)
    if device.type == "cpu":
        support = torch.zeros(binom.shape + (rows, width), dtype=torch.long)
        flat = support.view(-1, rows, width)
        for b, (l, c, n) in enumerate(zip(length_b.flatten().tolist(), count_b.flatten().tolist(),
                                          binom.flatten().tolist())):  # fmt: skip
            flat[b, :n, :l] = _cardinality_rows_torch(l, c, n)
        return support, binom
    l, c = length_b.contiguous(), count_b.contiguous()
    support = _cardinality_hip(l, c, 0, 0, binom.numel(), rows, width, torch.int64, device)
    return support.view(binom.shape + (rows, width)), binom


def enumerate_binary_sequences_with_cardinality(
    length: Any,
    count: Any,
    device: torch.device = torch.device("cpu"),
    dtype: torch.dtype = torch.long,
) -> Any:
    """The binary sequences of ``length`` elements that sum to ``count``, in the order they have within
    :func:`enumerate_binary_sequences` (reference _combinatorics.py:358-412).

    Two ints give a ``(C(length, count), length)`` tensor on ``device``.  Two broadcasting long tensors give
    ``(support, binom)``: ``support[b, :binom[b], :length[b]]`` holds the sequences of batch element ``b``
    and the rest of ``support`` is zero (the reference leaves it uninitialised).  Lengths are limited to 62.
    """
    if isinstance(length, torch.Tensor) and isinstance(count, torch.Tensor):
        return _cardinality_tensor(length, count)
    if isinstance(length, int) and isinstance(count, int):
        return _cardinality_int(length, count, device, dtype)
    raise RuntimeError("length and count must both be tensors or ints")


def _srswor_torch(total: torch.Tensor, given: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(u)
    ell = given.clone()
    for t in range(u.shape[1]):
        rem = (total - t).clamp_min(1)
        b = u[:, t] < ell.float() / rem.float()
        out[:, t] = b.float()
        ell = ell - b.long()
    return out


@custom_op("pydrobert_amd::srswor", mutates_args=())
def _srswor_op(total_count: torch.Tensor, given_count: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Fan's sequential draw over explicit uniforms ``u`` (B, out_size) float32: with ``ell`` the ones of
    row ``b`` still to place, ``out[b, t] = u[b, t] < float(ell) / float(max(total_count[b] - t, 1))``.
    Preconditions, which :func:`simple_random_sampling_without_replacement` checks or guarantees and this
    operator does not (it reads nothing back): ``0 <= given_count <= total_count`` and ``u`` in ``[0, 1)``.
    Outside them nothing is read or written out of bounds, but a row's sum is not its ``given_count``."""
    if u.dim() != 2 or u.dtype != torch.float32:
        raise RuntimeError("srswor: u must be a float32 matrix (rows, out_size)")
    total, given = torch.broadcast_tensors(total_count, given_count)
    total, given = total.long().reshape(-1).contiguous(), given.long().reshape(-1).contiguous()
    B, O = u.shape
    if total.numel() != B:
        raise RuntimeError("srswor: u has {} rows for {} pairs of counts".format(B, total.numel()))
    if u.device.type == "cpu":
        return _srswor_torch(total, given, u.detach())
    device = _cabi.require_hip(total, given, u)
    u = u.detach().contiguous()
    out = torch.empty_like(u)
    with _cabi.on_device(device):
        rc = _cabi.lib().pdt_srswor(
            _cabi.ptr(total), _cabi.ptr(given), _cabi.ptr(u) if u.numel() else None, B, O,
            _cabi.ptr(out) if out.numel() else None, _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_srswor")
    return out


@_srswor_op.register_fake
def _(total_count, given_count, u):
    return torch.empty_like(u, memory_format=torch.contiguous_format)


def simple_random_sampling_without_replacement(
    total_count: torch.Tensor, given_count: torch.Tensor, out_size: Optional[int] = None
) -> torch.Tensor:
    """Draw binary vectors of ``out_size`` elements, uniform among those whose first ``total_count`` elements
    sum to ``given_count`` and whose others are zero (reference _combinatorics.py:27-85; [fan1962]).  The
    uniforms come from :func:`torch.rand` on the device, so :func:`torch.manual_seed` governs the draw."""
    total, given = torch.broadcast_tensors(total_count, given_count)
    device = total.device
    largest = 0
    if total.numel():
        # the one host read: the largest total and whether some given count exceeds its total
        largest, exceeds = torch.stack([total.max().long(), (given > total).any().long()]).tolist()
        if exceeds:
            raise RuntimeError("given_count cannot exceed total_count")
    if out_size is None:
        out_size = largest
    if out_size < largest:
        raise RuntimeError("out_size ({}) must not be less than max of total_count ({})".format(out_size, largest))
    u = torch.rand((total.numel(), out_size), device=device, dtype=torch.float32)
    b = torch.ops.pydrobert_amd.srswor(total, given, u)
    return b.view(total.shape + (out_size,)).to(torch.get_default_dtype())


def _nonnegative_tensor(val: Any, name: str) -> torch.Tensor:
    if not isinstance(val, torch.Tensor):
        raise ValueError("{} is not a tensor".format(name))
    if (val < 0).any():
        raise ValueError("{} must be non-negative".format(name))
    return val


class BinaryCardinalityConstraint(constraints.Constraint):
    """A binary vector that sums to ``given_count`` and is zero from ``total_count`` on (reference
    _combinatorics.py:88-119)."""

    is_discrete = True
    event_dim = 1

    def __init__(self, given_count: torch.Tensor, tmax: int, total_count: Optional[torch.Tensor] = None) -> None:
        tmax = argcheck.is_posi(tmax, "tmax")
        given_count = _nonnegative_tensor(given_count, "given_count")
        if total_count is None:
            beyond = torch.zeros(1, dtype=torch.bool, device=given_count.device)
        else:
            total_count = _nonnegative_tensor(total_count, "total_count")
            beyond = total_count.unsqueeze(-1) <= torch.arange(tmax, device=total_count.device)
        super().__init__()
        self.given_count, self.total_count_mask = given_count, beyond

    def check(self, value: torch.Tensor) -> torch.Tensor:
        binary = ((value == 0) | (value == 1)).all(-1)
        tail_empty = (self.total_count_mask.expand_as(value) * value).sum(-1) == 0
        total = value.sum(-1)
        return binary & tail_empty & (total == self.given_count.expand_as(total))


class SimpleRandomSamplingWithoutReplacement(torch.distributions.ExponentialFamily):
    r"""Binary vectors of ``out_size`` elements, uniform among those whose first ``total_count`` elements sum to
    ``given_count`` and whose others are zero (reference _combinatorics.py:415-598): SRSWOR,
    :math:`P(b | L) = I[\sum_t b_t = L] / \binom{T}{L}`, a special case of the conditional Bernoulli [chen1994]
    and an exponential family.

    ``total_count`` (:math:`T`) and ``given_count`` (:math:`L \le T`) broadcast to the batch shape;
    ``out_size`` is at least ``total_count.max()``, its default.  :func:`sample` is one launch of the
    sequential draw (:func:`simple_random_sampling_without_replacement`); the support is enumerated by
    unranking, and only when every batch element has the same counts.
    """

    arg_constraints = {
        "total_count": constraints.nonnegative_integer,
        "given_count": constraints.nonnegative_integer,
    }
    _mean_carrier_measure = 0

    def __init__(
        self,
        given_count: Union[int, torch.Tensor],
        total_count: Union[int, torch.Tensor],
        out_size: Optional[int] = None,
        validate_args: Optional[bool] = None,
    ):
        device = None
        if isinstance(given_count, torch.Tensor):
            device = given_count.device
            if isinstance(total_count, torch.Tensor) and given_count.device != total_count.device:
                raise ValueError("given_count and total_count must be on the same device")
        elif isinstance(total_count, torch.Tensor):
            device = total_count.device
        given_count = torch.as_tensor(given_count, device=device)
        total_count = torch.as_tensor(total_count, device=device)
        if out_size is None:
            out_size = int(total_count.max().item())
        given_count, total_count = torch.broadcast_tensors(given_count, total_count)
        self.total_count, self.given_count = total_count, given_count
        super().__init__(given_count.size(), torch.Size([out_size]), validate_args)
        if self._validate_args:
            _nonnegative_tensor(given_count, "given_count")
            _nonnegative_tensor(total_count, "total_count")
            if (given_count > total_count).any():
                raise ValueError("given_count must be less than or equal to total_count")
            if (total_count > out_size).any():
                raise ValueError("out_size must be greater than or equal to total_count")

    @constraints.dependent_property
    def support(self):
        return BinaryCardinalityConstraint(self.given_count, self.event_shape[0], self.total_count)

    @property
    def has_enumerate_support(self) -> bool:
        total, given = self.total_count.flatten(), self.given_count.flatten()
        return bool(((total == total[0]).all() & (given == given[0]).all()).item())

    def enumerate_support(self, expand=True) -> torch.Tensor:
        if not self.has_enumerate_support:
            raise NotImplementedError(
                "total_count must all be equal and given_count must all be equal to enumerate support"
            )
        total = int(self.total_count.flatten()[0].item())
        given = int(self.given_count.flatten()[0].item())
        support = enumerate_binary_sequences_with_cardinality(total, given, self.total_count.device, dtype=torch.float)
        out_size = self.event_shape[0]
        if out_size != total:
            support = torch.nn.functional.pad(support, (0, out_size - total))
        support = support.view((-1,) + (1,) * len(self.batch_shape) + (out_size,))
        if expand:
            support = support.expand((-1,) + self.batch_shape + (out_size,))
        return support

    @lazy_property
    def log_partition(self) -> torch.Tensor:
        """``log C(total_count, given_count)`` from a running sum of logs, in float32 as the reference's."""
        log_factorial = torch.arange(
            1, self.event_shape[0] + 1, device=self.total_count.device, dtype=torch.float
        ).log().cumsum(0)  # fmt: skip
        total, given = self.total_count.long(), self.given_count.long()
        t, g, d = ((x - 1).clamp_min(0) for x in (total, given, total - given))
        return log_factorial[t] - log_factorial[g] - log_factorial[d]

    @property
    def mean(self):
        beyond = self.total_count.unsqueeze(-1) <= torch.arange(self.event_shape[0], device=self.total_count.device)
        rate = (self.given_count / self.total_count.clamp_min(1.0)).unsqueeze(-1)
        return rate.expand(self.batch_shape + self.event_shape).masked_fill(beyond, 0.0)

    @property
    def variance(self):
        return self.mean * (1 - self.mean)

    @property
    def _natural_params(self):
        return self.total_count.new_zeros(self.batch_shape + self.event_shape)

    def _log_normalizer(self, logits):
        if (logits == 0).all():
            raise RuntimeError("Logits invalid")
        return self.log_partition

    def expand(self, batch_shape, _instance=None):
        new = self._get_checked_instance(SimpleRandomSamplingWithoutReplacement, _instance)
        batch_shape = list(batch_shape)
        new.given_count = self.given_count.expand(batch_shape)
        new.total_count = self.total_count.expand(batch_shape)
        if "log_partition" in self.__dict__:
            new.log_partition = self.log_partition.expand(batch_shape)
        super(SimpleRandomSamplingWithoutReplacement, new).__init__(
            torch.Size(batch_shape), self.event_shape, validate_args=False
        )
        new._validate_args = self._validate_args
        return new

    def sample(self, sample_shape=torch.Size([])):
        shape = self._extended_shape(torch.Size(sample_shape))
        with torch.no_grad():
            return simple_random_sampling_without_replacement(
                self.total_count.expand(shape[:-1]), self.given_count.expand(shape[:-1]), self.event_shape[0]
            )

    def log_prob(self, value):
        if self._validate_args:
            self._validate_sample(value)
        return (-self.log_partition).expand(value.shape[:-1])
