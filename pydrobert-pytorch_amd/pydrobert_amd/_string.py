"""Batched edit-distance family on MI355X.

Host-side mirror of the reference's ``_string.py``: same functions, argument order,
defaults, output shapes/dtypes, exceptions and warnings; the dynamic programming itself
runs behind ``pdt_lev``, ``pdt_oc_mask`` and ``pdt_oc_expand`` (``include/pdt_amd.h``):
uniform costs in the bit-parallel kernels of ``csrc/lev_bitpar.hip`` and ``csrc/oc_bitpar.hip``,
other costs cell by cell in ``csrc/lev_skewed.hip`` / ``csrc/lev_rowsync.hip``, references
beyond 2048 tokens in ``csrc/lev_generic.hip``; the expansion is ``csrc/oc_expand.hip``.
"""

import contextlib
import warnings
from typing import Optional, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck, config, switches
from ._step import _logits_elem

__all__ = [
    "EditDistance",
    "ErrorRate",
    "FillAfterEndOfSequence",
    "HardOptimalCompletionDistillationLoss",
    "MinimumErrorRateLoss",
    "OptimalCompletion",
    "PrefixEditDistances",
    "PrefixErrorRates",
    "edit_distance",
    "error_rate",
    "fill_after_eos",
    "hard_optimal_completion_distillation_loss",
    "minimum_error_rate_loss",
    "optimal_completion",
    "prefix_edit_distances",
    "prefix_error_rates",
]


@custom_op("pydrobert_amd::fill_after_eos", mutates_args=())
def _fill_after_eos_op(tokens: torch.Tensor, eos: int, dim: int, fill: float, value: torch.Tensor) -> torch.Tensor:
    """One walk along ``dim`` (reference _string.py:30-42; csrc/fill_after_eos.hip)."""
    device = _cabi.require_hip(tokens, value)
    # `dim` indexes tokens' OWN shape: the reference runs cumsum(dim) on the tokens and lets
    # masked_fill broadcast the finished mask against the value (_string.py:40-42)
    nd = tokens.dim()
    if nd == 0:
        if dim not in (-1, 0):
            raise IndexError("Dimension out of range (expected to be in range of [-1, 0], but got {})".format(dim))
        return value.clone()
    if dim < -nd or dim >= nd:
        raise IndexError(
            "Dimension out of range (expected to be in range of [{}, {}], but got {})".format(-nd, nd - 1, dim)
        )
    dim = dim % nd
    if value.shape != tokens.shape:  # masked_fill would broadcast; the reference's callers never do
        value = value.expand(torch.broadcast_shapes(value.shape, tokens.shape))
        if tokens.size(dim) == 1:  # one token along the walk: nothing comes after it, whatever it broadcasts to
            return value.clone(memory_format=torch.contiguous_format)
        dim += value.dim() - nd  # leading dimensions the broadcast put in front of the tokens'
        tokens = tokens.expand(value.shape)
    if tokens.dtype == torch.long:
        tok, eos_ = tokens.detach().contiguous(), int(eos)
    else:  # any dtype compares against eos the way ``tokens == eos`` does
        tok, eos_ = (tokens.detach() == eos).long().contiguous(), 1
    val = value.detach().contiguous()
    if val.dtype.is_complex:
        raise RuntimeError("fill_after_eos: complex values are not supported")
    out = torch.empty_like(val)
    # the fill value converted the way masked_fill converts its scalar, then its raw bits
    if val.dtype == torch.long and fill == float(eos) and -(2**63) <= eos < 2**63:
        # eos itself (the default fill): a double does not hold every int64, masked_fill's integer scalar does
        bits = int(eos)
    else:
        one = torch.full((1,), fill, dtype=val.dtype)
        bits = int(one.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[val.element_size()]).item())
    outer = 1
    for d in range(dim):
        outer *= tok.shape[d]
    L = tok.shape[dim]
    inner = tok.numel() // max(1, outer * L) if outer * L else 0
    with torch.cuda.device(device):
        rc = _cabi.lib().pdt_fill_after_eos(
            _cabi.ptr(tok), outer, L, inner, eos_, _cabi.ptr(val), val.element_size(),
            bits, _cabi.ptr(out), _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, "pdt_fill_after_eos")
    return out


@_fill_after_eos_op.register_fake
def _(tokens, eos, dim, fill, value):
    return torch.empty_like(value.expand(torch.broadcast_shapes(value.shape, tokens.shape)), memory_format=torch.contiguous_format)


def _fill_after_eos_backward(ctx, grad):
    # masked_fill's adjoint: the gradient passes where the value was kept
    tokens, = ctx.saved_tensors
    g = torch.ops.pydrobert_amd.fill_after_eos(tokens, ctx.eos, ctx.dim, 0.0, grad)
    if g.shape != ctx.value_shape:
        g = g.sum_to_size(ctx.value_shape)
    return None, None, None, None, g


def _fill_after_eos_setup(ctx, inputs, output):
    tokens, eos, dim, fill, value = inputs
    ctx.save_for_backward(tokens)
    ctx.eos, ctx.dim, ctx.value_shape = eos, dim, value.shape


register_autograd("pydrobert_amd::fill_after_eos", _fill_after_eos_backward, setup_context=_fill_after_eos_setup)


def fill_after_eos(
    tokens: torch.Tensor,
    eos: int,
    dim: int = 0,
    fill: Optional[float] = None,
    value: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Fill everything after the first ``eos`` along ``dim`` (reference _string.py:30-42)."""
    out = tokens if value is None else value
    fill_ = float(eos) if fill is None else fill
    return torch.ops.pydrobert_amd.fill_after_eos(tokens, eos, dim, fill_, out)


def _seq_strides(t: torch.Tensor, batch_first: bool):
    """(T, N, stride_t, stride_n) in elements for a (T, N) or (N, T) token tensor."""
    if batch_first:
        return t.shape[1], t.shape[0], t.stride(1), t.stride(0)
    return t.shape[0], t.shape[1], t.stride(0), t.stride(1)


def _prep(ref: torch.Tensor, hyp: torch.Tensor, batch_first: bool):
    if ref.dim() != 2 or hyp.dim() != 2:
        raise RuntimeError("ref and hyp must be 2 dimensional")  # _string.py:166-167
    if (ref.shape[0] if batch_first else ref.shape[1]) != (hyp.shape[0] if batch_first else hyp.shape[1]):
        raise RuntimeError(
            "ref has batch size {}, but hyp has {}".format(
                ref.shape[0] if batch_first else ref.shape[1],
                hyp.shape[0] if batch_first else hyp.shape[1],
            )
        )  # _string.py:191-194
    device = _cabi.require_hip(ref, hyp)
    ref, hyp = ref.detach(), hyp.detach()  # _string.py:186-187
    if ref.dtype != torch.long:
        ref = ref.long()
    if hyp.dtype != torch.long:
        hyp = hyp.long()
    R, N, rst, rsn = _seq_strides(ref, batch_first)
    H, _, hst, hsn = _seq_strides(hyp, batch_first)
    return device, ref, hyp, (R, rst, rsn), (H, hst, hsn), N


_NO_EOS_MSG = (
    "include_eos=True, but a transcription in {} did not contain the eos symbol ({}). "
    "To suppress this warning, set warn=False"
)


def _emit_warnings(flags: int, eos, prefix: bool):
    if flags & _cabi.WARN_REF_NO_EOS:
        warnings.warn(_NO_EOS_MSG.format("ref", eos))  # _string.py:202-207
    if flags & _cabi.WARN_HYP_NO_EOS:
        warnings.warn(_NO_EOS_MSG.format("hyp", eos))  # _string.py:212-217
    if flags & _cabi.WARN_EMPTY_REF:
        if prefix:  # _string.py:362-367
            warnings.warn(
                "ref contains empty transcripts. Error rates will be 0 for prefixes of "
                "length 0, 1 otherwise. To suppress this warning, set warn=False"
            )
        else:  # _string.py:399-404
            warnings.warn(
                "ref contains empty transcripts. Error rates for entries will be 1 if "
                "any insertion and 0 otherwise. To suppress this warning, set warn=False"
            )


def _uniform_costs(ins_cost, del_cost, sub_cost) -> bool:
    """The costs the native side runs as unit costs (_string.py:168-174)."""
    return float(ins_cost) == float(del_cost) == float(sub_cost) > 0.0


def _workspace(size_fn, uniform: bool, R: int, H: int, N: int, device):
    """Scratch memory of one call, ``(tensor or None, bytes)``; ``size_fn`` is the entry point's
    ``pdt_*_workspace_bytes``.  Only the bit-parallel kernels -- uniform costs -- and the plain kernel
    for references beyond 2048 tokens read a workspace; every other call launches without one, and so
    does a shape for which ``size_fn`` reports 0 (served by the cell-by-cell kernels).  torch's
    caching allocator hands the same block back call after call."""
    nbytes = int(size_fn(R, H, N)) if (uniform or R > 2048) else 0
    if nbytes <= 0:
        return None, 0
    return torch.empty(nbytes, device=device, dtype=torch.uint8), nbytes


# OPT-IN (PDT_LEV_CACHE=1, or `with reuse_classification():`): the classification of a (ref, hyp)
# pair -- lengths, token classes, match tables -- is kept for the NEXT string operator on the same
# pair (error_rate followed by prefix_error_rates builds them once; include/pdt_amd.h:
# pdt_lev_keep, pdt_lev_classified).  A hit is decided by identity (address, version counter, geometry, eos handling,
# stream), NOT by content: writes that do not move the version counter (`t.data[...] = ...`, kernels
# writing through a raw pointer, graph replays into static buffers, DLPack aliases) leave the key
# unchanged and the next operator would run on the previous contents' tables.  Hence off by default;
# the caller who turns it on promises not to write the tensors between the two operators.
# One entry per device; it holds the two token tensors (their addresses cannot be recycled while it
# stands) and the workspace, serves ONE hit and is dropped; leaving `reuse_classification()` drops it
# too.  Tensors without a version counter (inference tensors) never enter it.
_CLASSIFIED = {}


def _classified_key(device, ref, hyp, geom, eos, include_eos, norm):
    try:
        versions = (ref._version, hyp._version)
    except RuntimeError:  # inference tensors do not track a version counter: no identity to match on
        return None
    stream = _cabi.stream_ptr(device)
    stream = stream if isinstance(stream, int) else getattr(stream, "value", None)
    # (without an eos every sequence has its full length: include_eos changes nothing)
    return (ref.data_ptr(), versions[0], hyp.data_ptr(), versions[1], geom, eos,
            bool(include_eos) and eos is not None, bool(norm), stream)


def _classified_take(device, key, warn):
    """Drops the device's entry (it serves one hit) and returns its ``(workspace, status)`` if it was
    made for ``key`` -- with the warning bits of the classifying call when this call wants them --
    else ``None``."""
    hit = _CLASSIFIED.pop(device.index, None)
    if key is None or hit is None or hit[0] != key or (hit[4] is None and warn):
        return None
    return hit[3], hit[4]


def _classified_store(device, key, ref, hyp, ws, status):
    _CLASSIFIED[device.index] = (key, ref, hyp, ws, status)


@contextlib.contextmanager
def reuse_classification():
    """Within the block, a string operator with uniform costs keeps the classification of its
    ``(ref, hyp)`` pair for the next operator on the same pair (``error_rate`` then
    ``prefix_error_rates``: 0.19 -> 0.144 ms at N=4096, T=512).  The caller must not write ``ref`` or
    ``hyp`` between the two calls in ways the version counter does not see (see above)."""
    old = switches.get("PDT_LEV_CACHE")
    switches.set("PDT_LEV_CACHE", 1)
    try:
        yield
    finally:
        switches.set("PDT_LEV_CACHE", old)
        _CLASSIFIED.clear()


@custom_op("pydrobert_amd::string_matching", mutates_args=())
def _string_matching_op(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int],
    include_eos: bool,
    batch_first: bool,
    ins_cost: float,
    del_cost: float,
    sub_cost: float,
    warn: bool,
    norm: bool,
    return_prf_dsts: bool,
    exclude_last: bool,
    padding: int,
    return_mistakes: bool,
) -> torch.Tensor:
    """FINAL / PREFIX flavours of the reference's ``_string_matching`` (_string.py:146-406)."""
    device, ref, hyp, (R, rst, rsn), (H, hst, hsn), N = _prep(ref, hyp, batch_first)
    uniform = _uniform_costs(ins_cost, del_cost, sub_cost)
    if return_mistakes and not uniform and warn:  # _string.py:175-180
        warnings.warn(
            "The behaviour for non-uniform error rates has changed after v0.3.0. Please "
            "switch to edit_distance functions for old behaviour. Set warn=False to "
            "suppress this warning"
        )
    if return_prf_dsts:
        Hout = H + (0 if exclude_last else 1)
        if Hout == 0:  # the reference writes row 0 of a (0, N) buffer (_string.py:280-285)
            raise IndexError("index 0 is out of bounds for dimension 0 with size 0")
        out = torch.empty((Hout, N), device=device, dtype=torch.float)
        out_sh, out_sn = out.stride(0), out.stride(1)
        mode = _cabi.MODE_PREFIX
    else:
        out = torch.empty((N,), device=device, dtype=torch.float)
        out_sh, out_sn = 0, 1
        mode = _cabi.MODE_FINAL
    L = _cabi.lib()
    with torch.cuda.device(device):
        status = torch.zeros(1, device=device, dtype=torch.int32) if warn else None
        caching = uniform and switches.get("PDT_LEV_CACHE")
        geom = (R, rst, rsn, H, hst, hsn, N)
        key = _classified_key(device, ref, hyp, geom, eos, include_eos, norm) if caching else None
        kept = _classified_take(device, key, warn) if caching else None
        remember = False
        if kept is not None:  # the tables the previous operator on this pair left, and its warning bits
            (ws, status), entry, name = kept, L.pdt_lev_classified, "pdt_lev"
            ws_bytes = ws.numel()
        else:
            ws, ws_bytes = _workspace(L.pdt_lev_workspace_bytes, uniform, R, H, N, device)
            # (pdt_lev leaves no tables behind: the call a later hit reads from keeps them)
            remember = key is not None and ws is not None
            entry, name = (L.pdt_lev_keep, "pdt_lev_keep") if remember else (L.pdt_lev, "pdt_lev")
        rc = entry(
            _cabi.ptr(ref), R, rst, rsn, _cabi.ptr(hyp), H, hst, hsn, N,
            int(eos is not None), int(eos) if eos is not None else 0, int(include_eos),
            float(ins_cost), float(del_cost), float(sub_cost), int(norm), mode,
            int(exclude_last), float(padding), int(return_mistakes),
            _cabi.ptr(out), out_sh, out_sn, 0, 0, _cabi.ptr(status), _cabi.ptr(ws), ws_bytes,
            _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, name)
    if remember:
        _classified_store(device, key, ref, hyp, ws, status)
    if warn:
        flags = int(status.item())
        if flags:
            _emit_warnings(flags, eos, return_prf_dsts)
    if return_prf_dsts and batch_first:
        out = out.t()  # _string.py:387-388
    return out


@_string_matching_op.register_fake
def _(ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn, norm,
      return_prf_dsts, exclude_last, padding, return_mistakes):  # fmt: skip
    N = ref.shape[0] if batch_first else ref.shape[1]
    if not return_prf_dsts:
        return ref.new_empty((N,), dtype=torch.float)
    Hout = (hyp.shape[1] if batch_first else hyp.shape[0]) + (0 if exclude_last else 1)
    out = ref.new_empty((Hout, N), dtype=torch.float)
    return out.t() if batch_first else out


def _string_matching(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int],
    include_eos: bool,
    batch_first: bool,
    ins_cost: float,
    del_cost: float,
    sub_cost: float,
    warn: bool,
    norm: bool = False,
    return_prf_dsts: bool = False,
    exclude_last: bool = False,
    padding: int = config.INDEX_PAD_VALUE,
    return_mistakes: bool = False,
) -> torch.Tensor:
    """TorchScript-visible entry: one opaque ``pydrobert_amd::string_matching`` node."""
    return torch.ops.pydrobert_amd.string_matching(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn, norm,
        return_prf_dsts, exclude_last, padding, return_mistakes,
    )  # fmt: skip


def error_rate(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int] = None,
    include_eos: bool = False,
    norm: bool = True,
    batch_first: bool = False,
    ins_cost: float = config.DEFT_INS_COST,
    del_cost: float = config.DEFT_DEL_COST,
    sub_cost: float = config.DEFT_SUB_COST,
    warn: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`ErrorRate` (reference _string.py:409-434)."""
    return _string_matching(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn,
        norm=norm, return_mistakes=True,
    )  # fmt: skip


def edit_distance(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int] = None,
    include_eos: bool = False,
    norm: bool = False,
    batch_first: bool = False,
    ins_cost: float = config.DEFT_INS_COST,
    del_cost: float = config.DEFT_DEL_COST,
    sub_cost: float = config.DEFT_SUB_COST,
    warn: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`EditDistance` (reference _string.py:437-461)."""
    return _string_matching(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn, norm=norm
    )


def prefix_error_rates(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int] = None,
    include_eos: bool = True,
    norm: bool = True,
    batch_first: bool = False,
    ins_cost: float = config.DEFT_INS_COST,
    del_cost: float = config.DEFT_DEL_COST,
    sub_cost: float = config.DEFT_SUB_COST,
    padding: int = config.INDEX_PAD_VALUE,
    exclude_last: bool = False,
    warn: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`PrefixErrorRates` (reference _string.py:520-550)."""
    return _string_matching(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn,
        norm=norm, return_prf_dsts=True, exclude_last=exclude_last, padding=padding,
        return_mistakes=True,
    )  # fmt: skip


def prefix_edit_distances(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int] = None,
    include_eos: bool = True,
    norm: bool = False,
    batch_first: bool = False,
    ins_cost: float = config.DEFT_INS_COST,
    del_cost: float = config.DEFT_DEL_COST,
    sub_cost: float = config.DEFT_SUB_COST,
    padding: int = config.INDEX_PAD_VALUE,
    exclude_last: bool = False,
    warn: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`PrefixEditDistances` (reference _string.py:553-583)."""
    return _string_matching(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn,
        norm=norm, return_prf_dsts=True, exclude_last=exclude_last, padding=padding,
        return_mistakes=False,
    )  # fmt: skip


@custom_op("pydrobert_amd::optimal_completion", mutates_args=())
def _optimal_completion_op(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int],
    include_eos: bool,
    batch_first: bool,
    ins_cost: float,
    del_cost: float,
    sub_cost: float,
    padding: int,
    exclude_last: bool,
    warn: bool,
) -> torch.Tensor:
    """Two kernels with one host read-back in between, like the reference's
    ``counts.max().item()`` (_string.py:511): the DP emits per-prefix class bitmasks plus the
    maximum set size ``C``; the expansion writes the ``(H', N, C)`` int64 targets."""
    device, bitmask, class_tokens, scal, (R, Hout, N) = _oc_mask(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, exclude_last, warn,
        "pdt_oc_mask", initial_row_always=True,
    )  # fmt: skip
    L = _cabi.lib()
    with torch.cuda.device(device):
        stream = _cabi.stream_ptr(device)
        C, flags = (int(x) for x in scal[:2].tolist())  # the one host sync (:511)
        if warn and flags:
            _emit_warnings(flags, eos, True)
        targets = torch.empty((Hout, N, C), device=device, dtype=torch.long)
        if C > 0 and N > 0:
            rc = L.pdt_oc_expand(
                _cabi.ptr(bitmask), _cabi.ptr(class_tokens), R, Hout, N,
                C, int(padding), _cabi.ptr(targets), targets.stride(0), targets.stride(1), stream,
            )  # fmt: skip
            _cabi.check(rc, "pdt_oc_expand")
    if batch_first:
        targets = targets.transpose(0, 1)  # _string.py:515-516
    return targets


@_optimal_completion_op.register_fake
def _(ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, padding,
      exclude_last, warn):  # fmt: skip
    N = ref.shape[0] if batch_first else ref.shape[1]
    Hout = max(1, (hyp.shape[1] if batch_first else hyp.shape[0]) + (0 if exclude_last else 1))
    C = torch.library.get_ctx().new_dynamic_size()  # the data-dependent set size (:511)
    out = ref.new_empty((Hout, N, C), dtype=torch.long)
    return out.transpose(0, 1) if batch_first else out


def optimal_completion(
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int] = None,
    include_eos: bool = True,
    batch_first: bool = False,
    ins_cost: float = config.DEFT_INS_COST,
    del_cost: float = config.DEFT_DEL_COST,
    sub_cost: float = config.DEFT_SUB_COST,
    padding: int = config.INDEX_PAD_VALUE,
    exclude_last: bool = False,
    warn: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`OptimalCompletion` (reference _string.py:464-517)."""
    return torch.ops.pydrobert_amd.optimal_completion(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, padding,
        exclude_last, warn,
    )  # fmt: skip


def _oc_mask(ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, exclude_last,
             warn, what, initial_row_always=False):
    """Phase 1 of optimal completion: (bitmask (H', N, W), class_tokens (N, R), scal, sizes).

    The reference appends the initial row mask BEFORE its loop (_string.py:271-278, :286), so the mask
    of an EMPTY hypothesis has one row whether or not ``exclude_last`` is set: with
    ``initial_row_always`` (optimal_completion itself) ``H == 0, exclude_last=True`` is computed as
    ``H == 0, exclude_last=False`` -- the same single row ``{ref[0]}``.  The loss (`ocd_loss_rows`)
    pairs every row with a row of logits and has none to pair it with (the reference fails in
    ``view_as``, _string.py:1238), so it keeps the error."""
    device, ref, hyp, (R, rst, rsn), (H, hst, hsn), N = _prep(ref, hyp, batch_first)
    if R == 0:  # the reference sets row 0 of a (0, N) mask (_string.py:275)
        raise IndexError("index 0 is out of bounds for dimension 0 with size 0")
    if H == 0 and exclude_last and initial_row_always:
        exclude_last = False
    Hout = H + (0 if exclude_last else 1)
    if Hout == 0:
        raise RuntimeError("hyp has no steps to compute prefixes of")
    L = _cabi.lib()
    W = int(L.pdt_oc_mask_words(R))
    with torch.cuda.device(device):
        bitmask = torch.empty((Hout, N, W), device=device, dtype=torch.int32)
        class_tokens = torch.empty((N, max(R, 1)), device=device, dtype=torch.long)
        scal = torch.zeros(3, device=device, dtype=torch.int32)  # [max_count, status, aux status]
        # the bit-parallel kernel's tables (uniform costs, R <= 512) or the plain formulation's rows
        # (R > 2048); everything else runs out of registers
        ws, ws_bytes = _workspace(L.pdt_oc_mask_workspace_bytes, _uniform_costs(ins_cost, del_cost, sub_cost), R, H, N, device)
        rc = L.pdt_oc_mask(
            _cabi.ptr(ref), R, rst, rsn, _cabi.ptr(hyp), H, hst, hsn, N,
            int(eos is not None), int(eos) if eos is not None else 0, int(include_eos),
            float(ins_cost), float(del_cost), float(sub_cost), int(exclude_last),
            _cabi.ptr(bitmask), _cabi.ptr(class_tokens), scal.data_ptr(),
            scal.data_ptr() + 4, _cabi.ptr(ws), ws_bytes, _cabi.stream_ptr(device),
        )  # fmt: skip
    _cabi.check(rc, what)
    return device, bitmask, class_tokens, scal, (R, Hout, N)


@custom_op("pydrobert_amd::ocd_loss_rows", mutates_args=())
def _ocd_loss_rows_op(
    logits: torch.Tensor,
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int],
    include_eos: bool,
    batch_first: bool,
    ins_cost: float,
    del_cost: float,
    sub_cost: float,
    weight: Optional[torch.Tensor],
    ignore_index: int,
    warn: bool,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss (H, N), count (H, N), bitmask, class_tokens): the DP kernel's class bitmasks go
    straight into the fused cross-entropy kernel; the last two outputs are what the backward
    kernel needs.  Differentiable w.r.t. ``logits``."""
    if logits.dim() != 3:
        raise RuntimeError("logits must be 3 dimensional")
    if logits.shape[:-1] != hyp.shape:
        raise RuntimeError("first two dims of logits must match hyp shape")
    if include_eos:
        if eos is not None and ((eos < 0) or (eos >= logits.size(-1))):
            raise RuntimeError("If include_eos=True, eos ({}) must be a class idx".format(eos))
        if eos is not None and eos == ignore_index:
            raise RuntimeError("If include_eos=True, eos cannot equal ignore_index ({}".format(eos))
    if logits.size(-1) >= 2**30:  # the one bound on V, forward and backward alike (csrc/ocd_loss.hip)
        raise RuntimeError(
            "logits has V = {} classes; the MI355X kernels index a row of logits with 32 bits "
            "(V < 2**30)".format(logits.size(-1))
        )
    _cabi.require_hip(logits, weight)
    device, bitmask, class_tokens, scal, (R, H, N) = _oc_mask(
        ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, True, warn,
        "pdt_oc_mask",
    )  # fmt: skip
    x, elem = _logits_elem(logits)  # (float16 / bfloat16: read as they are, strides kept, no float32 copy)
    if batch_first:
        x = x.transpose(0, 1)
    V = x.shape[2]
    w = None if weight is None else weight.detach().float().contiguous()
    with torch.cuda.device(device):
        loss = torch.empty((H, N), device=device, dtype=torch.float)
        count = torch.empty((H, N), device=device, dtype=torch.int32)
        args = (
            _cabi.ptr(x), H, N, V, x.stride(0), x.stride(1), x.stride(2), _cabi.ptr(bitmask),
            _cabi.ptr(class_tokens), max(R, 1), _cabi.ptr(w), int(ignore_index), _cabi.ptr(loss),
            _cabi.ptr(count), scal.data_ptr() + 8, _cabi.stream_ptr(device),
        )  # fmt: skip
        L = _cabi.lib()
        rc = L.pdt_ocd_loss_forward_elem(*args, elem) if elem else L.pdt_ocd_loss_forward(*args)
    _cabi.check(rc, "pdt_ocd_loss_forward")
    if warn:
        _, flags, bad = (int(x) for x in scal.tolist())
        if bad:
            raise RuntimeError("ref contains tokens that are not class indices of logits")
        _emit_warnings(flags, eos, True)
    return loss, count, bitmask, class_tokens


@_ocd_loss_rows_op.register_fake
def _(logits, ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, weight,
      ignore_index, warn):  # fmt: skip
    N, H = (hyp.shape[0], hyp.shape[1]) if batch_first else (hyp.shape[1], hyp.shape[0])
    R = max(ref.shape[1] if batch_first else ref.shape[0], 1)
    return (
        logits.new_empty((H, N), dtype=torch.float),
        logits.new_empty((H, N), dtype=torch.int32),
        logits.new_empty((H, N, (R + 31) // 32), dtype=torch.int32),
        logits.new_empty((N, R), dtype=torch.long),
    )


@custom_op("pydrobert_amd::ocd_loss_rows_backward", mutates_args=())
def _ocd_loss_rows_backward_op(
    logits: torch.Tensor,
    bitmask: torch.Tensor,
    class_tokens: torch.Tensor,
    weight: Optional[torch.Tensor],
    ignore_index: int,
    batch_first: bool,
    grad_loss: torch.Tensor,
) -> torch.Tensor:
    """d loss / d logits of ``ocd_loss_rows`` (csrc/ocd_loss.hip, BACKWARD)."""
    device = logits.device
    x, elem = _logits_elem(logits)
    if batch_first:
        x = x.transpose(0, 1)
    H, N, V = x.shape
    w = None if weight is None else weight.detach().float().contiguous()
    g = grad_loss.detach().float().contiguous()
    with torch.cuda.device(device):
        # (the dtype the kernel reads: a half gradient is rounded element by element as .to(dtype) would)
        grad = torch.empty((H, N, V), device=device, dtype=x.dtype)
        args = (
            _cabi.ptr(x), H, N, V, x.stride(0), x.stride(1), x.stride(2), _cabi.ptr(bitmask),
            _cabi.ptr(class_tokens), class_tokens.shape[1], _cabi.ptr(w), int(ignore_index),
            _cabi.ptr(g), _cabi.ptr(grad), _cabi.stream_ptr(device),
        )  # fmt: skip
        L = _cabi.lib()
        rc = L.pdt_ocd_loss_backward_elem(*args, elem) if elem else L.pdt_ocd_loss_backward(*args)
    _cabi.check(rc, "pdt_ocd_loss_backward")
    if batch_first:
        grad = grad.transpose(0, 1)
    return grad.to(logits.dtype)  # (float64 logits only: every other dtype is the kernel's already)


@_ocd_loss_rows_backward_op.register_fake
def _(logits, bitmask, class_tokens, weight, ignore_index, batch_first, grad_loss):
    return torch.empty_like(logits)


def _ocd_setup_context(ctx, inputs, output):
    logits, _, _, _, _, batch_first, _, _, _, weight, ignore_index, _ = inputs
    _, _, bitmask, class_tokens = output
    ctx.save_for_backward(logits, bitmask, class_tokens, weight)
    ctx.cfg = (ignore_index, batch_first)


def _ocd_backward(ctx, grad_loss, _gc, _gb, _gt):
    logits, bitmask, class_tokens, weight = ctx.saved_tensors
    ignore_index, batch_first = ctx.cfg
    grad = torch.ops.pydrobert_amd.ocd_loss_rows_backward(
        logits, bitmask, class_tokens, weight, ignore_index, batch_first, grad_loss
    )
    return (grad,) + (None,) * 11


register_autograd(
    "pydrobert_amd::ocd_loss_rows", _ocd_backward, setup_context=_ocd_setup_context
)


def hard_optimal_completion_distillation_loss(
    logits: torch.Tensor,
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int] = None,
    include_eos: bool = True,
    batch_first: bool = False,
    ins_cost: float = config.DEFT_INS_COST,
    del_cost: float = config.DEFT_DEL_COST,
    sub_cost: float = config.DEFT_SUB_COST,
    weight: Optional[torch.Tensor] = None,
    reduction: str = "mean",
    ignore_index: int = -2,
    warn: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`HardOptimalCompletionDistillationLoss` (reference
    _string.py:1188-1251).

    The completion sets never leave their compact form: the DP kernel emits per-prefix class
    bitmasks and one fused kernel evaluates the mean cross entropy over each set straight from
    the logits -- no ``(H, N, C)`` target tensor, no ``(H, N, C, V)`` logit expansion.
    """
    if reduction != "mean" and reduction != "sum" and reduction != "none":
        raise RuntimeError("'{}' is not a valid value for reduction".format(reduction))
    loss, count, _, _ = torch.ops.pydrobert_amd.ocd_loss_rows(
        logits, ref, hyp, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, weight,
        ignore_index, warn,
    )  # fmt: skip
    if reduction == "mean":
        # per utterance: sum over prefixes / number of prefixes with a non-empty set, then the
        # batch mean (:1243-1247)
        loss = (loss.sum(0) / (count > 0).sum(0).clamp_min(1)).mean()
    elif reduction == "sum":
        loss = loss.sum()
    elif batch_first:
        loss = loss.t()
    return loss


def minimum_error_rate_loss(
    log_probs: torch.Tensor,
    ref: torch.Tensor,
    hyp: torch.Tensor,
    eos: Optional[int] = None,
    include_eos: bool = True,
    sub_avg: bool = True,
    batch_first: bool = False,
    norm: bool = True,
    ins_cost: float = config.DEFT_INS_COST,
    del_cost: float = config.DEFT_DEL_COST,
    sub_cost: float = config.DEFT_SUB_COST,
    reduction: str = "mean",
    warn: bool = True,
) -> torch.Tensor:
    """Functional version of :class:`MinimumErrorRateLoss` (reference _string.py:1400-1472):
    expected error rate of ``samples`` hypotheses per batch element under
    ``softmax(log_probs)``; the error rates come from one ``pdt_lev`` launch over
    ``batch * samples`` utterances."""
    if log_probs.dim() != 2:
        raise RuntimeError("log_probs must be 2 dimensional")
    if hyp.dim() != 3:
        raise RuntimeError("hyp must be 3 dimensional")
    if ref.dim() != 2 and ref.dim() != 3:
        raise RuntimeError("ref must be 2 or 3 dimensional")
    if batch_first:
        batch_size, samples, max_hyp_steps = hyp.size(0), hyp.size(1), hyp.size(2)
        if ref.dim() == 2:
            ref = ref.unsqueeze(1).repeat(1, samples, 1)
        if (
            ref.size(0) != batch_size
            or ref.size(1) != samples
            or log_probs.size(0) != batch_size
            or log_probs.size(1) != samples
        ):
            raise RuntimeError("ref and hyp batch_size and sample dimensions must match")
        ref = ref.reshape(-1, ref.size(-1))
        hyp = hyp.reshape(-1, max_hyp_steps)
    else:
        max_hyp_steps, batch_size, samples = hyp.size(0), hyp.size(1), hyp.size(2)
        if ref.dim() == 2:
            ref = ref.unsqueeze(-1).repeat(1, 1, samples)
        if (
            ref.size(1) != batch_size
            or ref.size(2) != samples
            or log_probs.size(0) != batch_size
            or log_probs.size(1) != samples
        ):
            raise RuntimeError("ref and hyp batch_size and sample dimensions must match")
        ref = ref.reshape(ref.size(0), -1)
        hyp = hyp.reshape(max_hyp_steps, -1)
    if samples < 2:
        raise RuntimeError("Batch must have at least two samples, got {}".format(samples))
    if reduction != "mean" and reduction != "sum" and reduction != "none":
        raise RuntimeError("'{}' is not a valid value for reduction".format(reduction))
    er = error_rate(
        ref, hyp, eos=eos, include_eos=include_eos, norm=norm, batch_first=batch_first,
        ins_cost=ins_cost, del_cost=del_cost, sub_cost=sub_cost, warn=warn,
    ).view(batch_size, samples)  # fmt: skip
    if sub_avg:
        er = er - er.mean(1, keepdim=True)
    loss = er * torch.nn.functional.softmax(log_probs, 1)
    if reduction == "mean":
        loss = loss.mean()
    elif reduction == "sum":
        loss = loss.sum()
    return loss


# ---------------------------------------------------------------------------------------
# Modules (reference _string.py:45-134, :680-1166): constructor validation with argcheck,
# plain attributes listed in __constants__, forward = the functional with those attributes.
# ---------------------------------------------------------------------------------------


class FillAfterEndOfSequence(torch.nn.Module):
    """Fill after the first end-of-sequence token with a value (_string.py:45-134)."""

    __constants__ = "eos", "dim", "fill"

    def __init__(self, eos: int, dim: int = 0, fill: Optional[float] = None) -> None:
        eos = argcheck.is_int(eos, "eos")
        dim = argcheck.is_int(dim, "dim")
        fill = float(eos) if fill is None else argcheck.is_float(fill, "fill")
        super().__init__()
        self.eos, self.dim, self.fill = eos, dim, fill

    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)

    def forward(self, tokens: torch.Tensor, value: Optional[torch.Tensor] = None) -> torch.Tensor:
        return fill_after_eos(tokens, self.eos, self.dim, self.fill, value)


class _StringMatching(torch.nn.Module):
    __constants__ = ("eos", "include_eos", "batch_first", "ins_cost", "del_cost", "sub_cost", "warn")

    def __init__(self, eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn):
        eos = argcheck.is_int(eos, "eos", True)
        include_eos = argcheck.is_bool(include_eos, "include_eos")
        batch_first = argcheck.is_bool(batch_first, "batch_first")
        ins_cost = argcheck.is_float(ins_cost, "ins_cost")
        del_cost = argcheck.is_float(del_cost, "del_cost")
        sub_cost = argcheck.is_float(sub_cost, "sub_cost")
        warn = argcheck.is_bool(warn, "warn")
        super().__init__()
        self.eos, self.include_eos, self.batch_first = eos, include_eos, batch_first
        self.ins_cost, self.del_cost, self.sub_cost, self.warn = ins_cost, del_cost, sub_cost, warn

    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)


class EditDistance(_StringMatching):
    """Weighted Levenshtein distance between ref and hyp (_string.py:722-797)."""

    __constants__ = (
        "eos", "include_eos", "norm", "batch_first", "ins_cost", "del_cost", "sub_cost", "warn",
    )  # fmt: skip

    def __init__(
        self,
        eos: Optional[int] = None,
        include_eos: bool = False,
        norm: bool = False,
        batch_first: bool = False,
        ins_cost: float = config.DEFT_INS_COST,
        del_cost: float = config.DEFT_DEL_COST,
        sub_cost: float = config.DEFT_SUB_COST,
        warn: bool = True,
    ):
        norm = argcheck.is_bool(norm, "norm")
        super().__init__(eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn)
        self.norm = norm

    def forward(self, ref: torch.Tensor, hyp: torch.Tensor) -> torch.Tensor:
        return edit_distance(
            ref, hyp, self.eos, self.include_eos, self.norm, self.batch_first,
            self.ins_cost, self.del_cost, self.sub_cost, self.warn,
        )  # fmt: skip


class ErrorRate(_StringMatching):
    """Number of mistakes on the cheapest alignment, optionally / ref length (_string.py:888-967)."""

    __constants__ = EditDistance.__constants__

    def __init__(
        self,
        eos: Optional[int] = None,
        include_eos: bool = False,
        norm: bool = True,
        batch_first: bool = False,
        ins_cost: float = config.DEFT_INS_COST,
        del_cost: float = config.DEFT_DEL_COST,
        sub_cost: float = config.DEFT_SUB_COST,
        warn: bool = True,
    ):
        norm = argcheck.is_bool(norm, "norm")
        super().__init__(eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn)
        self.norm = norm

    def forward(self, ref: torch.Tensor, hyp: torch.Tensor) -> torch.Tensor:
        return error_rate(
            ref, hyp, self.eos, self.include_eos, self.norm, self.batch_first,
            self.ins_cost, self.del_cost, self.sub_cost, self.warn,
        )  # fmt: skip


class _Prefix(_StringMatching):
    __constants__ = (
        "eos", "include_eos", "norm", "batch_first", "ins_cost", "del_cost", "sub_cost",
        "padding", "exclude_last", "warn",
    )  # fmt: skip

    def __init__(self, eos, include_eos, norm, batch_first, ins_cost, del_cost, sub_cost,
                 padding, exclude_last, warn):  # fmt: skip
        norm = argcheck.is_bool(norm, "norm")
        padding = argcheck.is_int(padding, "padding")
        exclude_last = argcheck.is_bool(exclude_last, "exclude_last")
        super().__init__(eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn)
        self.norm, self.padding, self.exclude_last = norm, padding, exclude_last


class PrefixEditDistances(_Prefix):
    """Edit distance between ref and every prefix of hyp (_string.py:800-885)."""

    def __init__(
        self,
        eos: Optional[int] = None,
        include_eos: bool = True,
        norm: bool = False,
        batch_first: bool = False,
        ins_cost: float = config.DEFT_INS_COST,
        del_cost: float = config.DEFT_DEL_COST,
        sub_cost: float = config.DEFT_SUB_COST,
        padding: int = config.INDEX_PAD_VALUE,
        exclude_last: bool = False,
        warn: bool = True,
    ):
        super().__init__(eos, include_eos, norm, batch_first, ins_cost, del_cost, sub_cost,
                         padding, exclude_last, warn)  # fmt: skip

    def forward(self, ref: torch.Tensor, hyp: torch.Tensor) -> torch.Tensor:
        return prefix_edit_distances(
            ref, hyp, self.eos, self.include_eos, self.norm, self.batch_first, self.ins_cost,
            self.del_cost, self.sub_cost, self.padding, self.exclude_last, self.warn,
        )  # fmt: skip


class PrefixErrorRates(_Prefix):
    """Error rate between ref and every prefix of hyp (_string.py:970-1049)."""

    def __init__(
        self,
        eos: Optional[int] = None,
        include_eos: bool = True,
        norm: bool = True,
        batch_first: bool = False,
        ins_cost: float = config.DEFT_INS_COST,
        del_cost: float = config.DEFT_DEL_COST,
        sub_cost: float = config.DEFT_SUB_COST,
        padding: int = config.INDEX_PAD_VALUE,
        exclude_last: bool = False,
        warn: bool = True,
    ):
        super().__init__(eos, include_eos, norm, batch_first, ins_cost, del_cost, sub_cost,
                         padding, exclude_last, warn)  # fmt: skip

    def forward(self, ref: torch.Tensor, hyp: torch.Tensor) -> torch.Tensor:
        return prefix_error_rates(
            ref, hyp, self.eos, self.include_eos, self.norm, self.batch_first, self.ins_cost,
            self.del_cost, self.sub_cost, self.padding, self.exclude_last, self.warn,
        )  # fmt: skip


class OptimalCompletion(_StringMatching):
    """Optimal next tokens of every hyp prefix w.r.t. ref (_string.py:1052-1166)."""

    __constants__ = (
        "eos", "include_eos", "batch_first", "ins_cost", "del_cost", "sub_cost", "padding",
        "exclude_last", "warn",
    )  # fmt: skip

    def __init__(
        self,
        eos: Optional[int] = None,
        include_eos: bool = True,
        batch_first: bool = False,
        ins_cost: float = config.DEFT_INS_COST,
        del_cost: float = config.DEFT_DEL_COST,
        sub_cost: float = config.DEFT_SUB_COST,
        padding: int = config.INDEX_PAD_VALUE,
        exclude_last: bool = False,
        warn: bool = True,
    ):
        padding = argcheck.is_int(padding, "padding")
        exclude_last = argcheck.is_bool(exclude_last, "exclude_last")
        super().__init__(eos, include_eos, batch_first, ins_cost, del_cost, sub_cost, warn)
        self.padding, self.exclude_last = padding, exclude_last

    def forward(self, ref: torch.Tensor, hyp: torch.Tensor) -> torch.Tensor:
        return optimal_completion(
            ref, hyp, self.eos, self.include_eos, self.batch_first, self.ins_cost,
            self.del_cost, self.sub_cost, self.padding, self.exclude_last, self.warn,
        )  # fmt: skip


class HardOptimalCompletionDistillationLoss(torch.nn.Module):
    """A categorical loss based on how likely a model outputs optimal completions (reference
    _string.py:1254-1378)."""

    __constants__ = (
        "eos", "include_eos", "batch_first", "ins_cost", "del_cost", "sub_cost", "reduction",
        "ignore_index",
    )  # fmt: skip

    def __init__(
        self,
        eos: Optional[int] = None,
        include_eos: bool = True,
        batch_first: bool = False,
        ins_cost: float = config.DEFT_INS_COST,
        del_cost: float = config.DEFT_DEL_COST,
        sub_cost: float = config.DEFT_SUB_COST,
        weight: Optional[torch.Tensor] = None,
        reduction: str = "mean",
        ignore_index: int = config.INDEX_PAD_VALUE,
    ):
        eos = argcheck.is_int(eos, "eos", True)
        include_eos = argcheck.is_bool(include_eos, "include_eos")
        batch_first = argcheck.is_bool(batch_first, "batch_first")
        ins_cost = argcheck.is_float(ins_cost, "ins_cost")
        del_cost = argcheck.is_float(del_cost, "del_cost")
        sub_cost = argcheck.is_float(sub_cost, "sub_cost")
        weight = argcheck.is_tensor(weight, "weight", True)
        reduction = argcheck.is_in(reduction, ("mean", "sum", "none"), "reduction")
        ignore_index = argcheck.is_int(ignore_index, "ignore_index")
        super().__init__()
        self.eos, self.include_eos, self.batch_first = eos, include_eos, batch_first
        self.ins_cost, self.del_cost, self.sub_cost = ins_cost, del_cost, sub_cost
        self.reduction, self.ignore_index = reduction, ignore_index
        self.register_buffer("weight", weight)

    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)

    def forward(
        self, logits: torch.Tensor, ref: torch.Tensor, hyp: torch.Tensor, warn: bool = True
    ) -> torch.Tensor:
        return hard_optimal_completion_distillation_loss(
            logits, ref, hyp, self.eos, self.include_eos, self.batch_first, self.ins_cost,
            self.del_cost, self.sub_cost, self.weight, self.reduction, self.ignore_index, warn,
        )  # fmt: skip


class MinimumErrorRateLoss(torch.nn.Module):
    """Error rate expectation normalized over some number of transcripts (reference
    _string.py:1475-1646)."""

    __constants__ = (
        "eos", "include_eos", "sub_avg", "batch_first", "norm", "ins_cost", "del_cost",
        "sub_cost", "reduction",
    )  # fmt: skip

    def __init__(
        self,
        eos: Optional[int] = None,
        include_eos: bool = True,
        sub_avg: bool = True,
        batch_first: bool = False,
        norm: bool = True,
        ins_cost: float = config.DEFT_INS_COST,
        del_cost: float = config.DEFT_DEL_COST,
        sub_cost: float = config.DEFT_SUB_COST,
        reduction: str = "mean",
    ):
        eos = argcheck.is_int(eos, "eos", True)
        include_eos = argcheck.is_bool(include_eos, "include_eos")
        sub_avg = argcheck.is_bool(sub_avg, "sub_avg")
        batch_first = argcheck.is_bool(batch_first, "batch_first")
        norm = argcheck.is_bool(norm, "norm")
        ins_cost = argcheck.is_float(ins_cost, "ins_cost")
        del_cost = argcheck.is_float(del_cost, "del_cost")
        sub_cost = argcheck.is_float(sub_cost, "sub_cost")
        reduction = argcheck.is_in(reduction, ("mean", "sum", "none"), "reduction")
        super().__init__()
        self.eos, self.include_eos, self.sub_avg = eos, include_eos, sub_avg
        self.batch_first, self.norm, self.reduction = batch_first, norm, reduction
        self.ins_cost, self.del_cost, self.sub_cost = ins_cost, del_cost, sub_cost

    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)

    def forward(
        self, log_probs: torch.Tensor, ref: torch.Tensor, hyp: torch.Tensor, warn: bool = True
    ) -> torch.Tensor:
        return minimum_error_rate_loss(
            log_probs, ref, hyp, self.eos, self.include_eos, self.sub_avg, self.batch_first,
            self.norm, self.ins_cost, self.del_cost, self.sub_cost, self.reduction, warn,
        )  # fmt: skip
