"""The step functions of the two beam searches on MI355X: ``beam_search_advance``,
``ctc_prefix_search_advance`` (with the operator that mixes a language model's scores into the step
itself) and ``fusion_ext``.  They run in ``csrc/beam_advance.hip``, ``csrc/ctc_advance.hip``,
``csrc/advance_wide.hip`` and ``csrc/fusion_ext.hip`` through the C ABI (``include/pdt_amd.h``).
"""
from typing import Optional, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _cabi

__all__ = ["beam_search_advance", "ctc_prefix_search_advance"]


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.requires_grad:
        t = t.detach()
    return t if t.dtype == torch.float else t.float()


# element codes of the ``_elem`` entry points the kernels read as they are (include/pdt_amd.h; _feats._DTYPES)
_ELEM = {torch.float32: 0, torch.float16: 2, torch.bfloat16: 3}


def _logits_elem(t: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """``(tensor, elem)`` for the logits of an ``_elem`` entry point: float32, float16 and bfloat16 are passed
    as they are (detached, strides kept: the kernel widens a half element where it loads it); anything else --
    float64 -- takes the narrowing copy of ``_f32``."""
    if t.dtype in _ELEM:
        return (t.detach() if t.requires_grad else t), _ELEM[t.dtype]
    return _f32(t), 0


def _i64(t: torch.Tensor) -> torch.Tensor:
    if t.requires_grad:
        t = t.detach()
    return t if t.dtype == torch.long else t.long()


def _expect_shape(t: torch.Tensor, shape: Tuple[int, ...], wording: str) -> None:
    # `wording` up to the shape: the reference's messages differ from operator to operator
    if t.shape != shape:
        raise RuntimeError("{} {}, got {}".format(wording, shape, tuple(t.shape)))


def _beam_search_advance_impl(
    log_probs_t: torch.Tensor,
    width: int,
    log_probs_prev: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_lens: Optional[torch.Tensor],
    grows: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    # `grows`: the caller already knows whether some path is as long as the history (y_next
    # then has one row more, reference :133-135), which saves the read-back of max(y_prev_lens);
    # None = find out here
    if log_probs_t.dim() != 3:
        raise RuntimeError("log_probs_t must be 3 dimensional")
    N, Kp, V = log_probs_t.shape
    if width < 1:
        raise RuntimeError("Expected width to be >= 1, got {}".format(width))
    _expect_shape(log_probs_prev, (N, Kp), "Expected log_probs_prev to be of shape")
    if y_prev.dim() != 3:
        raise RuntimeError("y_prev must be 3 dimensional")
    if y_prev.shape[1:] != (N, Kp):
        raise RuntimeError(
            "Expected the last two dimensions of y_prev to be {}, got {}".format(
                (N, Kp), tuple(y_prev.shape[1:])
            )
        )
    S = y_prev.size(0)
    if y_prev_lens is not None:
        _expect_shape(y_prev_lens, (N, Kp), "Expected y_prev_lens to have shape")
    device = _cabi.require_hip(log_probs_t, log_probs_prev, y_prev, y_prev_lens)
    lpt, lpp, yp = _f32(log_probs_t), _f32(log_probs_prev), _i64(y_prev)
    ypl = None if y_prev_lens is None else _i64(y_prev_lens)
    grow = True
    if grows is not None:
        grow = grows
    elif ypl is not None and N * Kp:
        # :133-135 don't make y bigger unless we have to; :139-140 -- the reference's own host read
        # (`y_prev_lens.max()`), as one small kernel that raises a word in pinned host memory
        report = _cabi.host_report(device)
        with _cabi.on_device(device):
            rc = _cabi.lib().pdt_lens_reach(
                _cabi.ptr(ypl), ypl.stride(0), ypl.stride(1), N, Kp, S, report.ptr, _cabi.stream_ptr(device)
            )
            if rc:
                report.disarm()
                _cabi.check(rc, "pdt_lens_reach")
        seen = report.wait()
        if S:
            grow = bool(seen & 1)
        elif seen & 2:
            raise RuntimeError("Invalid lengths for t=0")
    S_out = S + (1 if grow else 0)
    with _cabi.on_device(device):
        y_next = torch.empty((S_out, N, width), device=device, dtype=torch.long)
        y_next_lens = torch.empty((N, width), device=device, dtype=torch.long)
        next_src = torch.empty((N, width), device=device, dtype=torch.long)
        lp_next = torch.empty((N, width), device=device, dtype=torch.float)
        if N and V:
            rc = _cabi.lib().pdt_beam_search_advance(
                _cabi.ptr(lpt), lpt.stride(0), lpt.stride(1), lpt.stride(2), N, Kp, V, int(width),
                _cabi.ptr(lpp), lpp.stride(0), lpp.stride(1),
                _cabi.ptr(yp), S, yp.stride(0), yp.stride(1), yp.stride(2),
                _cabi.ptr(ypl), 0 if ypl is None else ypl.stride(0), 0 if ypl is None else ypl.stride(1),
                S_out, _cabi.ptr(y_next), _cabi.ptr(y_next_lens), _cabi.ptr(lp_next),
                _cabi.ptr(next_src), _cabi.stream_ptr(device),
            )  # fmt: skip
            _cabi.check(rc, "pdt_beam_search_advance")
    return y_next, y_next_lens, lp_next.to(log_probs_t.dtype), next_src


@custom_op("pydrobert_amd::beam_search_advance", mutates_args=())
def _beam_search_advance_op(
    log_probs_t: torch.Tensor,
    width: int,
    log_probs_prev: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_lens: Optional[torch.Tensor],
    grows: Optional[bool] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _beam_search_advance_impl(log_probs_t, width, log_probs_prev, y_prev, y_prev_lens, grows)


@_beam_search_advance_op.register_fake
def _(log_probs_t, width, log_probs_prev, y_prev, y_prev_lens, grows=None):
    N = log_probs_t.shape[0]
    S = y_prev.shape[0]
    if grows is not None:
        S_out = S + (1 if grows else 0)
    elif y_prev_lens is not None:  # data dependent: S or S + 1 (:133-135)
        S_out = torch.library.get_ctx().new_dynamic_size()
    else:
        S_out = S + 1
    return (
        y_prev.new_empty((S_out, N, width), dtype=torch.long),
        y_prev.new_empty((N, width), dtype=torch.long),
        log_probs_t.new_empty((N, width)),
        y_prev.new_empty((N, width), dtype=torch.long),
    )


def _beam_search_advance_setup(ctx, inputs, output):
    log_probs_t, _, log_probs_prev = inputs[:3]
    y_next, y_next_lens, lp_next, next_src = output
    # the token a new path ends in sits at its last position
    tok = y_next.gather(0, (y_next_lens - 1).clamp(min=0).unsqueeze(0)).squeeze(0)
    ctx.save_for_backward(next_src, tok, torch.isfinite(lp_next))
    ctx.shape_t, ctx.dtype_t, ctx.dtype_prev = log_probs_t.shape, log_probs_t.dtype, log_probs_prev.dtype


def _beam_search_advance_backward(ctx, g_y, g_lens, g_lp, g_src):
    # log_probs_next[n, k] = log_probs_prev[n, src] + log_probs_t[n, src, tok] (reference
    # _decoding.py:121-131: the top-k VALUES stay in the graph), so the gradient of an entry goes
    # to exactly those two addends; padded (-inf) entries carry none
    src, tok, valid = ctx.saved_tensors
    N, Kp, V = ctx.shape_t
    g = torch.where(valid, g_lp, torch.zeros_like(g_lp)).float()
    g_prev = g.new_zeros((N, Kp)).scatter_add_(1, src, g)
    g_t = g.new_zeros((N, Kp * V)).scatter_add_(1, src * V + tok.clamp(0, V - 1), g).view(N, Kp, V)
    return g_t.to(ctx.dtype_t), None, g_prev.to(ctx.dtype_prev), None, None, None


register_autograd(
    "pydrobert_amd::beam_search_advance", _beam_search_advance_backward, setup_context=_beam_search_advance_setup
)


def beam_search_advance(
    log_probs_t: torch.Tensor,
    width: int,
    log_probs_prev: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_lens: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Beam search step function (reference _decoding.py:41-155).

    Returns ``(y_next, y_next_lens, log_probs_next, next_src)``.
    """
    if not torch.jit.is_scripting():
        # nothing to trace, transform or differentiate: the implementation behind the operator, directly
        if _cabi.plain_call(log_probs_t, log_probs_prev, y_prev, y_prev_lens):
            return _beam_search_advance_impl(log_probs_t, width, log_probs_prev, y_prev, y_prev_lens)
    return torch.ops.pydrobert_amd.beam_search_advance(
        log_probs_t, width, log_probs_prev, y_prev, y_prev_lens
    )


def _ctc_prefix_search_advance_impl(
    ext: torch.Tensor,
    nonext: torch.Tensor,
    blank: torch.Tensor,
    width: int,
    nb: torch.Tensor,
    b: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_last: torch.Tensor,
    y_prev_lens: torch.Tensor,
    prev_is_prefix: torch.Tensor,
    lm_mix: Optional[Tuple[float, bool]] = None,
) -> Optional[Tuple[
    torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
    torch.Tensor, torch.Tensor,
]]:  # fmt: skip
    # `lm_mix` = (beta, valid_mixture): `ext` then holds the language model's scores (N, K', V) and the
    # kernel mixes them with the frame's probabilities itself (pdt_ctc_prefix_search_advance_lm); None is
    # returned when that entry point does not take the shapes (the caller makes the two calls)
    if width < 1:
        raise RuntimeError("width must be positive")
    if ext.dim() != 3:
        raise RuntimeError("ext_probs_t must be 3 dimensional")
    N, Kp, V = ext.shape
    _expect_shape(nonext, (N, V), "expected nonext_probs_t to have shape")
    _expect_shape(blank, (N,), "expected blank_probs_t to have shape")
    _expect_shape(nb, (N, Kp), "expected nb_probs_prev to have shape")
    _expect_shape(b, (N, Kp), "expected b_probs_prev to have shape")
    if y_prev.dim() != 3:
        raise RuntimeError("y_prev must be 3 dimensional")
    if y_prev.shape[1:] != (N, Kp):
        raise RuntimeError(
            "expected last two dimensions of y_prev to be {}, got {}".format(
                (N, Kp), tuple(y_prev.shape[1:])
            )
        )
    S = y_prev.size(0)
    _expect_shape(y_prev_last, (N, Kp), "expected y_prev_last to have shape")
    _expect_shape(y_prev_lens, (N, Kp), "expected y_prev_lens to have shape")
    _expect_shape(prev_is_prefix, (N, Kp, Kp), "expected prev_is_prefix to have shape")
    device = _cabi.require_hip(ext, nonext, blank, nb, b, y_prev, y_prev_last, y_prev_lens,
                               prev_is_prefix)  # fmt: skip
    dtype = ext.dtype if lm_mix is None else nonext.dtype
    ext, nonext, blank, nb, b = (_f32(x) for x in (ext, nonext, blank, nb, b))
    yp, last, lens = _i64(y_prev), _i64(y_prev_last), _i64(y_prev_lens)
    isp = prev_is_prefix.detach() if prev_is_prefix.requires_grad else prev_is_prefix
    if isp.dtype != torch.bool:
        isp = isp.bool()
    W = int(width)
    with _cabi.on_device(device):
        y_next = torch.empty((S + 1, N, W), device=device, dtype=torch.long)
        o_last = torch.empty((N, W), device=device, dtype=torch.long)
        o_lens = torch.empty((N, W), device=device, dtype=torch.long)
        o_src = torch.empty((N, W), device=device, dtype=torch.long)
        o_nb = torch.empty((N, W), device=device, dtype=torch.float)
        o_b = torch.empty((N, W), device=device, dtype=torch.float)
        o_isp = torch.empty((N, W, W), device=device, dtype=torch.bool)
        o_non = torch.empty((N, W), device=device, dtype=torch.bool)
        if N:
            # what the two entry points share: everything behind their leading arguments
            shared = (
                _cabi.ptr(nonext), nonext.stride(0), nonext.stride(1),
                _cabi.ptr(blank), blank.stride(0), N, Kp, V, W,
                _cabi.ptr(nb), nb.stride(0), nb.stride(1), _cabi.ptr(b), b.stride(0), b.stride(1),
                _cabi.ptr(yp), S, yp.stride(0), yp.stride(1), yp.stride(2),
                _cabi.ptr(last), last.stride(0), last.stride(1),
                _cabi.ptr(lens), lens.stride(0), lens.stride(1),
                _cabi.ptr(isp), isp.stride(0), isp.stride(1), isp.stride(2),
                _cabi.ptr(y_next), _cabi.ptr(o_last), _cabi.ptr(o_lens), _cabi.ptr(o_nb),
                _cabi.ptr(o_b), _cabi.ptr(o_isp), _cabi.ptr(o_src), _cabi.ptr(o_non),
                _cabi.stream_ptr(device),
            )  # fmt: skip
            if lm_mix is not None:
                ext = ext.contiguous()
                rc = _cabi.lib().pdt_ctc_prefix_search_advance_lm(
                    _cabi.ptr(ext), float(lm_mix[0]), int(lm_mix[1]), *shared
                )
                if rc == _cabi.PDT_E_UNSUPPORTED:
                    return None
                _cabi.check(rc, "pdt_ctc_prefix_search_advance_lm")
            else:
                rc = _cabi.lib().pdt_ctc_prefix_search_advance(
                    _cabi.ptr(ext), ext.stride(0), ext.stride(1), ext.stride(2), *shared
                )
                _cabi.check(rc, "pdt_ctc_prefix_search_advance")
    if dtype != torch.float:
        o_nb, o_b = o_nb.to(dtype), o_b.to(dtype)
    return y_next, o_last, o_lens, o_nb, o_b, o_isp, o_src, o_non


@custom_op("pydrobert_amd::ctc_prefix_search_advance", mutates_args=())
def _ctc_prefix_search_advance_op(
    ext: torch.Tensor,
    nonext: torch.Tensor,
    blank: torch.Tensor,
    width: int,
    nb: torch.Tensor,
    b: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_last: torch.Tensor,
    y_prev_lens: torch.Tensor,
    prev_is_prefix: torch.Tensor,
) -> Tuple[
    torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
    torch.Tensor, torch.Tensor,
]:  # fmt: skip
    return _ctc_prefix_search_advance_impl(
        ext, nonext, blank, width, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix
    )


def _ctc_prefix_search_advance_lm_impl(
    lm_log_probs: torch.Tensor,
    beta: float,
    valid_mixture: bool,
    nonext: torch.Tensor,
    blank: torch.Tensor,
    width: int,
    nb: torch.Tensor,
    b: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_last: torch.Tensor,
    y_prev_lens: torch.Tensor,
    prev_is_prefix: torch.Tensor,
) -> Tuple[
    torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
    torch.Tensor, torch.Tensor,
]:  # fmt: skip
    """``fusion_ext`` + ``ctc_prefix_search_advance`` as ONE kernel: the extension probabilities (reference
    _decoding.py:1110-1135) are formed inside the step and never written.  ``lm_log_probs`` is ``(N, K', V)``.
    No gradient; shapes the kernel does not take (V > 1024, beams above 32) make the two calls here."""
    out = _ctc_prefix_search_advance_impl(
        lm_log_probs, nonext, blank, width, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix,
        (beta, valid_mixture),
    )  # fmt: skip
    if out is None:
        N, Kp, V = lm_log_probs.shape
        ext = _fusion_ext_impl(lm_log_probs.reshape(N * Kp, V), nonext, blank, beta, valid_mixture)
        out = _ctc_prefix_search_advance_impl(
            ext, nonext, blank, width, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix
        )
    return out


@custom_op("pydrobert_amd::ctc_prefix_search_advance_lm", mutates_args=())
def _ctc_prefix_search_advance_lm_op(
    lm_log_probs: torch.Tensor,
    beta: float,
    valid_mixture: bool,
    nonext: torch.Tensor,
    blank: torch.Tensor,
    width: int,
    nb: torch.Tensor,
    b: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_last: torch.Tensor,
    y_prev_lens: torch.Tensor,
    prev_is_prefix: torch.Tensor,
) -> Tuple[
    torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
    torch.Tensor, torch.Tensor,
]:  # fmt: skip
    return _ctc_prefix_search_advance_lm_impl(
        lm_log_probs, beta, valid_mixture, nonext, blank, width, nb, b, y_prev, y_prev_last, y_prev_lens,
        prev_is_prefix,
    )  # fmt: skip


@_ctc_prefix_search_advance_lm_op.register_fake
def _(lm_log_probs, beta, valid_mixture, nonext, blank, width, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix):
    N, W, S = lm_log_probs.shape[0], width, y_prev.shape[0]
    i64 = lambda *s: y_prev.new_empty(s, dtype=torch.long)  # noqa: E731
    return (
        i64(S + 1, N, W), i64(N, W), i64(N, W), nonext.new_empty((N, W)), nonext.new_empty((N, W)),
        nonext.new_empty((N, W, W), dtype=torch.bool), i64(N, W), nonext.new_empty((N, W), dtype=torch.bool),
    )  # fmt: skip


def _ctc_step_with_lm_scores(lm_log_probs, beta, valid_mixture, nonext, blank, width, nb, b, y_prev, y_prev_last,
                             y_prev_lens, prev_is_prefix):
    """The operator above, or -- nothing tracing, transforming or differentiating -- what is behind it."""
    args = (lm_log_probs, beta, valid_mixture, nonext, blank, width, nb, b, y_prev, y_prev_last, y_prev_lens,
            prev_is_prefix)  # fmt: skip
    if _cabi.plain_call(lm_log_probs, nonext, blank, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix):
        return _ctc_prefix_search_advance_lm_impl(*args)
    return torch.ops.pydrobert_amd.ctc_prefix_search_advance_lm(*args)


@_ctc_prefix_search_advance_op.register_fake
def _(ext, nonext, blank, width, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix):
    N, W, S = ext.shape[0], width, y_prev.shape[0]
    i64 = lambda *s: y_prev.new_empty(s, dtype=torch.long)  # noqa: E731
    return (
        i64(S + 1, N, W), i64(N, W), i64(N, W), ext.new_empty((N, W)), ext.new_empty((N, W)),
        ext.new_empty((N, W, W), dtype=torch.bool), i64(N, W), ext.new_empty((N, W), dtype=torch.bool),
    )  # fmt: skip


def _ctc_advance_setup(ctx, inputs, output):
    ext, nonext, blank, _, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix = inputs
    _, o_last, _, o_nb, _, _, o_src, o_non = output
    ctx.save_for_backward(ext, nonext, blank, nb, b, y_prev, y_prev_last, y_prev_lens, prev_is_prefix,
                          o_last, o_nb, o_src, o_non)  # fmt: skip


def _ctc_advance_backward(ctx, g_y, g_last, g_lens, g_nb, g_b, g_isp, g_src, g_non):
    """Adjoint of the masses of one CTC prefix-search step (reference _decoding.py:777-880; the
    selection itself is piecewise constant).  A new entry i with source s = next_src[i] holds
      extension by v:   nb' = w(s, v) * ext[s, v],  b' = 0,   w(s, v) = (nb[s] if v != last[s] else 0) + b[s]
      non-extension:    nb' = nb[s] * nonext[last[s]] + sum over prefixes k that BECOME s when extended
                              by need(k, s) of w(k, need) * ext[k, need],
                        b'  = (nb[s] + b[s]) * blank
    The dense work is (N, K', K') -- nothing of size V besides the scatter into grad ext."""
    (ext, nonext, blank, nb, b, y_prev, last, lens, is_prefix, o_last, o_nb, src, non) = ctx.saved_tensors
    N, Kp, V = ext.shape
    S = y_prev.shape[0]
    f = torch.float
    ext_, nonext_, blank_, nb_, b_ = ext.to(f), nonext.to(f), blank.to(f), nb.to(f), b.to(f)
    valid = torch.isfinite(o_nb)
    zero = torch.zeros((), device=ext.device, dtype=f)
    # absent (padded) prefixes hold -inf masses: they are the source of nothing valid
    nb_, b_ = torch.where(torch.isfinite(nb_), nb_, zero), torch.where(torch.isfinite(b_), b_, zero)
    gnb = torch.where(valid, g_nb.to(f), zero)
    gb = torch.where(valid & non, g_b.to(f), zero)
    lastc = last.clamp(0, V - 1)
    # --- extension entries
    is_ext = valid & ~non
    tok = o_last.clamp(0, V - 1)
    last_s = lastc.gather(1, src)
    w = torch.where(tok != last_s, nb_.gather(1, src), zero) + b_.gather(1, src)
    e = ext_.reshape(N, Kp * V).gather(1, src * V + tok)
    ge = torch.where(is_ext, gnb, zero)
    g_ext = ge.new_zeros((N, Kp * V)).scatter_add_(1, src * V + tok, ge * w)
    g_nb_prev = ge.new_zeros((N, Kp)).scatter_add_(1, src, torch.where(tok != last_s, ge * e, zero))
    g_b_prev = ge.new_zeros((N, Kp)).scatter_add_(1, src, ge * e)
    # --- non-extension entries: gradient of stay_nb[s] / stay_b[s], summed over the entries that kept s
    gs_nb = ge.new_zeros((N, Kp)).scatter_add_(1, src, torch.where(non, gnb, zero))
    gs_b = ge.new_zeros((N, Kp)).scatter_add_(1, src, gb)
    p_last = nonext_.gather(1, lastc)
    g_nonext = ge.new_zeros((N, V)).scatter_add_(1, lastc, gs_nb * nb_)
    g_nb_prev = g_nb_prev + gs_nb * p_last + gs_b * blank_.unsqueeze(1)
    g_b_prev = g_b_prev + gs_b * blank_.unsqueeze(1)
    g_blank = (gs_b * (nb_ + b_)).sum(1)
    # merged extensions: prefix k + need(k, s) == prefix s
    if S:
        at = lens.clamp(max=S - 1).unsqueeze(2).expand(N, Kp, Kp).transpose(0, 1)
        need = y_prev.gather(0, at).transpose(0, 1).clamp(0, V - 1)  # (N, k, s)
    else:
        need = torch.zeros((N, Kp, Kp), dtype=torch.long, device=ext.device)
    becomes = ((lens + 1).unsqueeze(2) == lens.unsqueeze(1)) & is_prefix.bool()
    gm = torch.where(becomes, gs_nb.unsqueeze(1).expand(N, Kp, Kp), zero)  # d stay_nb[s] / d term(k, s)
    differs = need != lastc.unsqueeze(2)
    wk = torch.where(differs, nb_.unsqueeze(2), zero) + b_.unsqueeze(2)
    ek = ext_.gather(2, need)
    k_idx = torch.arange(Kp, device=ext.device).view(1, Kp, 1)
    g_ext.scatter_add_(1, (k_idx * V + need).reshape(N, Kp * Kp), (gm * wk).reshape(N, Kp * Kp))
    g_nb_prev = g_nb_prev + torch.where(differs, gm * ek, zero).sum(2)
    g_b_prev = g_b_prev + (gm * ek).sum(2)
    return (g_ext.view(N, Kp, V).to(ext.dtype), g_nonext.to(nonext.dtype), g_blank.to(blank.dtype), None,
            g_nb_prev.to(nb.dtype), g_b_prev.to(b.dtype), None, None, None, None)  # fmt: skip


register_autograd(
    "pydrobert_amd::ctc_prefix_search_advance", _ctc_advance_backward, setup_context=_ctc_advance_setup
)


def ctc_prefix_search_advance(
    probs_t: Tuple[torch.Tensor, torch.Tensor, torch.Tensor],
    width: int,
    probs_prev: Tuple[torch.Tensor, torch.Tensor],
    y_prev: torch.Tensor,
    y_prev_last: torch.Tensor,
    y_prev_lens: torch.Tensor,
    prev_is_prefix: torch.Tensor,
) -> Tuple[
    torch.Tensor, torch.Tensor, torch.Tensor, Tuple[torch.Tensor, torch.Tensor], torch.Tensor,
    torch.Tensor, torch.Tensor,
]:  # fmt: skip
    """CTC prefix search step function (reference _decoding.py:636-934).

    Returns ``(y_next, y_next_last, y_next_lens, (nb_probs_next, b_probs_next),
    next_is_prefix, next_src, next_is_nonext)``.
    """
    if not torch.jit.is_scripting():
        # nothing to trace, transform or differentiate: the implementation behind the operator, directly
        if _cabi.plain_call(probs_t[0], probs_t[1], probs_t[2], probs_prev[0], probs_prev[1], y_prev,
                            y_prev_last, y_prev_lens, prev_is_prefix):  # fmt: skip
            y_next, last, lens, nb, b, isp, src, non = _ctc_prefix_search_advance_impl(
                probs_t[0], probs_t[1], probs_t[2], width, probs_prev[0], probs_prev[1], y_prev,
                y_prev_last, y_prev_lens, prev_is_prefix,
            )  # fmt: skip
            return y_next, last, lens, (nb, b), isp, src, non
    y_next, last, lens, nb, b, isp, src, non = torch.ops.pydrobert_amd.ctc_prefix_search_advance(
        probs_t[0], probs_t[1], probs_t[2], width, probs_prev[0], probs_prev[1], y_prev,
        y_prev_last, y_prev_lens, prev_is_prefix,
    )  # fmt: skip
    return y_next, last, lens, (nb, b), isp, src, non


def _fusion_ext_impl(
    lm_log_probs: torch.Tensor, nonext: torch.Tensor, blank: torch.Tensor, beta: float, valid_mixture: bool
) -> torch.Tensor:
    """Extension probabilities ``(N, K', V)`` of one frame from the LM scores ``(N * K', V)`` and
    the frame's CTC probabilities, in one pass (``csrc/fusion_ext.hip``; reference
    _decoding.py:1110-1135).  No gradient: ``CTCPrefixSearch`` composes torch ops instead when
    one is wanted."""
    N, V = nonext.shape
    if lm_log_probs.dim() != 2 or lm_log_probs.size(1) != V or (N and lm_log_probs.size(0) % N):
        raise RuntimeError("lm_log_probs must be of shape (N * K', V)")
    Kp = lm_log_probs.size(0) // N if N else 1
    device = _cabi.require_hip(lm_log_probs, nonext, blank)
    lm, ne, bl = _f32(lm_log_probs).contiguous(), _f32(nonext), _f32(blank)
    with _cabi.on_device(device):
        out = torch.empty((N, Kp, V), device=device, dtype=torch.float)
        if N and V:
            rc = _cabi.lib().pdt_fusion_ext(
                _cabi.ptr(lm), N, Kp, V, _cabi.ptr(ne), ne.stride(0), ne.stride(1), _cabi.ptr(bl),
                bl.stride(0), float(beta), int(valid_mixture), _cabi.ptr(out), _cabi.stream_ptr(device),
            )  # fmt: skip
            _cabi.check(rc, "pdt_fusion_ext")
    return out.to(nonext.dtype)


@custom_op("pydrobert_amd::fusion_ext", mutates_args=())
def _fusion_ext_op(
    lm_log_probs: torch.Tensor, nonext: torch.Tensor, blank: torch.Tensor, beta: float, valid_mixture: bool
) -> torch.Tensor:
    return _fusion_ext_impl(lm_log_probs, nonext, blank, beta, valid_mixture)


@_fusion_ext_op.register_fake
def _(lm_log_probs, nonext, blank, beta, valid_mixture):
    N, V = nonext.shape
    return nonext.new_empty((N, lm_log_probs.shape[0] // max(N, 1), V))
