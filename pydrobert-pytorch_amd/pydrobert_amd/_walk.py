"""Sampling from language models on MI355X (``csrc/random_walk.hip``): ``random_walk_advance`` and
``RandomWalk``.
"""
from typing import Dict, Optional, Tuple, Union

import torch
from torch.distributions import constraints
from torch.library import custom_op, register_autograd

from . import _cabi, argcheck, switches
from ._combinatorics import enumerate_vocab_sequences
from ._decoding import _dense_table
from ._lm import LookupLanguageModel
from ._seqops import SequenceLogProbabilities
from ._step import _f32, _i64
from ._string import fill_after_eos

__all__ = ["RandomWalk", "SequentialLanguageModelDistribution", "TokenSequenceConstraint", "random_walk_advance"]


_WALK_INVALID, _WALK_REACH, _WALK_BAD_LENS = 2, 4, 8


def _walk_launch(device: torch.device, launch, what: str) -> Tuple[int, int, int]:
    """``launch(host_report_ptr)`` enqueues one random-walk kernel; returns its report ``(bits, live,
    longest)`` once it is done (include/pdt_amd.h, "Random walks": word 0 = PDT_WALK_DONE | bits, stored
    last; one wait on it in pinned host memory, no device-to-host copy).  A row the kernel could draw
    nothing from raises (the reference's sampler would hit a device assert)."""
    report = _cabi.host_report(device)
    rc = launch(report.ptr)
    if rc:
        report.disarm()
        _cabi.check(rc, what)
    bits = report.wait()
    if bits & _WALK_INVALID:
        raise RuntimeError(
            "{}: a row of log-probabilities has no positive finite mass (every entry -inf, a NaN or +inf); "
            "nothing can be sampled from it".format(what)
        )
    return bits, report.read(1), report.read(2)


def _random_walk_checks(
    log_probs_t: torch.Tensor,
    log_probs_prev: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_lens: Optional[torch.Tensor],
) -> None:
    if log_probs_t.dim() != 2:
        raise RuntimeError("log_probs_t must be 2-dimensional")
    N = log_probs_t.size(0)
    if log_probs_prev.dim() != 1 or log_probs_prev.size(0) != N:
        raise RuntimeError(
            "Expected log_probs_prev to be of shape ({},), got {}".format(N, log_probs_prev.shape)
        )
    if y_prev.dim() != 2:
        raise RuntimeError("y_prev must be 2-dimensional")
    if y_prev.size(1) != N:
        raise RuntimeError("Expected dim 1 of y_prev to be {}, got {}".format(N, y_prev.size(-1)))
    if y_prev_lens is not None and (y_prev_lens.dim() != 1 or y_prev_lens.size(0) != N):
        raise RuntimeError(
            "Expected y_prev_lens to have shape ({},), got {}".format(N, y_prev_lens.shape)
        )


@custom_op("pydrobert_amd::random_walk_advance", mutates_args=())
def _random_walk_advance_op(
    log_probs_t: torch.Tensor,
    u: torch.Tensor,
    log_probs_prev: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_lens: Optional[torch.Tensor],
) -> Tuple[torch.Tensor, torch.Tensor]:
    """random_walk_advance with the uniforms given: token n is drawn from row n of ``log_probs_t`` by the
    rule of include/pdt_amd.h with ``u[n]``; one kernel (csrc/random_walk.hip), one host wait."""
    _random_walk_checks(log_probs_t, log_probs_prev, y_prev, y_prev_lens)
    N, V = log_probs_t.shape
    if u.shape != (N,):
        raise RuntimeError("Expected u to be of shape ({},), got {}".format(N, tuple(u.shape)))
    device = _cabi.require_hip(log_probs_t, u, log_probs_prev, y_prev, y_prev_lens)
    lpt, uu, lpp, yp = _f32(log_probs_t), _f32(u), _f32(log_probs_prev), _i64(y_prev)
    ypl = None if y_prev_lens is None else _i64(y_prev_lens)
    S = yp.size(0)
    grow = True
    with _cabi.on_device(device):
        y_next = torch.empty((S + 1, N), device=device, dtype=torch.long)
        lp_next = torch.empty((N,), device=device, dtype=torch.float)
        if N:
            ctl = torch.zeros((4,), device=device, dtype=torch.int32)
            bits, _, _ = _walk_launch(
                device,
                lambda host: _cabi.lib().pdt_random_walk_advance(
                    _cabi.ptr(lpt), lpt.stride(0), lpt.stride(1), N, V, _cabi.ptr(uu), uu.stride(0),
                    _cabi.ptr(lpp), lpp.stride(0), _cabi.ptr(yp), S, yp.stride(0), yp.stride(1),
                    _cabi.ptr(ypl), 0 if ypl is None else ypl.stride(0), _cabi.ptr(y_next), _cabi.ptr(lp_next),
                    _cabi.ptr(ctl), host, _cabi.stream_ptr(device),
                ),
                "random_walk_advance",
            )  # fmt: skip
            if bits & _WALK_BAD_LENS:
                raise RuntimeError("random_walk_advance: y_prev_lens must lie in [0, {}]".format(S))
            # :1272-1276 don't make y bigger unless some path reaches the end of the history
            grow = ypl is None or S == 0 or bool(bits & _WALK_REACH)
    if not grow:
        y_next = y_next[:S]
    return y_next, lp_next.to(torch.promote_types(log_probs_prev.dtype, log_probs_t.dtype))


@_random_walk_advance_op.register_fake
def _(log_probs_t, u, log_probs_prev, y_prev, y_prev_lens):
    N, S = log_probs_t.shape[0], y_prev.shape[0]
    if y_prev_lens is None or S == 0:
        S_out = S + 1
    else:  # data dependent: S or S + 1 (:1272-1276)
        S_out = torch.library.get_ctx().new_dynamic_size()
    return (
        log_probs_t.new_empty((S_out, N), dtype=torch.long),
        log_probs_t.new_empty((N,), dtype=torch.promote_types(log_probs_prev.dtype, log_probs_t.dtype)),
    )


def _rwa_setup_context(ctx, inputs, output):
    log_probs_t, _, log_probs_prev, y_prev, y_prev_lens = inputs
    y_next = output[0]
    S = y_prev.size(0)
    if S == 0 or y_prev_lens is None or y_next.size(0) > S:
        tok = y_next[S]  # (the row the reference appends holds every walk's token)
    else:
        tok = y_next.gather(0, y_prev_lens.long().unsqueeze(0)).squeeze(0)
    ctx.save_for_backward(tok)
    ctx.cfg = (tuple(log_probs_t.shape), log_probs_t.dtype, log_probs_prev.dtype)


def _rwa_backward(ctx, g_y, g_lp):
    """``log_probs_next = log_probs_prev + log_probs_t[n, token]``: the gradient is ``g`` at the drawn token
    of each row and ``g`` itself for ``log_probs_prev`` (the reference's gather, :1268)."""
    (tok,) = ctx.saved_tensors
    shape, lpt_dtype, lpp_dtype = ctx.cfg
    if g_lp is None:
        return None, None, None, None, None
    g_lpt = torch.zeros(shape, dtype=lpt_dtype, device=tok.device)
    g_lpt.scatter_(1, tok.unsqueeze(1), g_lp.unsqueeze(1).to(lpt_dtype))
    return g_lpt, None, g_lp.to(lpp_dtype), None, None


register_autograd("pydrobert_amd::random_walk_advance", _rwa_backward, setup_context=_rwa_setup_context)


@custom_op("pydrobert_amd::random_walk_step", mutates_args=("y", "lens", "ended", "log_probs", "ctl"))
def _random_walk_step_op(
    scores: torch.Tensor,
    u: torch.Tensor,
    y: torch.Tensor,
    t: int,
    lens: torch.Tensor,
    ended: torch.Tensor,
    log_probs: torch.Tensor,
    ctl: torch.Tensor,
    eos: Optional[int],
) -> int:
    """One iteration of RandomWalk.forward with the default hook (csrc/random_walk.hip): from the model's
    ``scores (N, V)`` and ``u (N,)``, row ``t`` of ``y (T, N)`` and the walks' ``lens`` / ``ended`` /
    ``log_probs`` in place.  ``ctl``: four int32 on the device, zero.  Returns how many walks have not
    ended (all of them when ``eos`` is None)."""
    if scores.dim() != 2:
        raise RuntimeError("scores must be 2-dimensional")
    N, V = scores.shape
    if y.dim() != 2 or y.size(1) != N or not 0 <= t < y.size(0):
        raise RuntimeError("random_walk_step: y must be (T, {}) with T > t = {}".format(N, t))
    for name, x, dt in (("u", u, torch.float), ("lens", lens, torch.long), ("ended", ended, torch.bool),
                        ("log_probs", log_probs, torch.float)):  # fmt: skip
        if x.shape != (N,) or x.dtype != dt or not x.is_contiguous():
            raise RuntimeError("random_walk_step: {} must be a contiguous {} tensor of shape ({},)".format(name, dt, N))
    if y.dtype != torch.long or not y.is_contiguous() or ctl.dtype != torch.int32 or ctl.numel() < 4:
        raise RuntimeError("random_walk_step: y must be contiguous int64, ctl four int32")
    device = _cabi.require_hip(scores, u, y, lens, ended, log_probs, ctl)
    x = _f32(scores)
    if N == 0:
        return 0
    _, live, _ = _walk_launch(
        device,
        lambda host: _cabi.lib().pdt_random_walk_step(
            _cabi.ptr(x), x.stride(0), x.stride(1), N, V, _cabi.ptr(u), int(eos is not None), int(eos or 0),
            y.data_ptr() + 8 * t * N, _cabi.ptr(lens), _cabi.ptr(ended), _cabi.ptr(log_probs), _cabi.ptr(ctl),
            host, _cabi.stream_ptr(device),
        ),
        "random_walk_step",
    )  # fmt: skip
    return live


@_random_walk_step_op.register_fake
def _(scores, u, y, t, lens, ended, log_probs, ctl, eos):
    return scores.shape[0]


def random_walk_advance(
    log_probs_t: torch.Tensor,
    log_probs_prev: torch.Tensor,
    y_prev: torch.Tensor,
    y_prev_lens: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Random walk step function (reference _decoding.py:1207-1283).  On the GPU: one uniform per row from
    torch's generator on the device, then ONE kernel draws every token (the rule of include/pdt_amd.h),
    forms the log-probabilities and the next history; differentiable with respect to ``log_probs_t`` and
    ``log_probs_prev``.  CPU tensors take the reference's torch body."""
    _random_walk_checks(log_probs_t, log_probs_prev, y_prev, y_prev_lens)
    if log_probs_t.device.type == "cuda":
        u = torch.rand((log_probs_t.size(0),), device=log_probs_t.device, dtype=torch.float)
        return torch.ops.pydrobert_amd.random_walk_advance(log_probs_t, u, log_probs_prev, y_prev, y_prev_lens)
    S = y_prev.size(0)
    y_t = torch.multinomial(log_probs_t.exp(), 1, True)  # (N, 1)
    log_probs_next = log_probs_prev + log_probs_t.gather(1, y_t).squeeze(1)
    y_t = y_t.T
    if S:
        if y_prev_lens is None:
            y_next = torch.cat([y_prev, y_t], 0)
        else:
            y_next = torch.cat([y_prev, y_t], 0) if int(y_prev_lens.max().item()) >= S else y_prev
            y_next = y_next.scatter(0, y_prev_lens.unsqueeze(0), y_t)
    else:
        y_next = y_t
    return y_next, log_probs_next


def _walk_chunk(t: int, max_iters: int) -> int:
    """How many iterations from ``t``, the first of a chunk, one ``torch.rand((C, N))`` call draws the
    uniforms of: C = 64, doubling up to 4096 (the chunks start at 0, 64, 192, 448, ...: C = t + 64 until
    then), cut off at ``max_iters`` -- every route of RandomWalk draws on this schedule."""
    return min(min(t + 64, 4096), max_iters - t)


class RandomWalk(torch.nn.Module):
    """Perform a random walk on the outputs of a language model (reference
    _decoding.py:1286-1513).

    On the GPU every token is drawn by one rule (include/pdt_amd.h, "Random walks") from uniforms drawn
    with torch's generator on the device, ``torch.rand((C, N))`` once per chunk of iterations (C = 64,
    doubling up to 4096).  Three routes, which draw the same uniforms:

    * a :class:`LookupLanguageModel` whose dense context table is at most 64 MiB, the default hook, no
      gradients, no initial state: each chunk of iterations is ONE launch over the table
      (``pdt_random_walk_table``; switch ``PDT_WALK_TABLE``);
    * any model, the default hook, an output that wants no gradient: the model's call and ONE kernel per
      iteration (``pydrobert_amd::random_walk_step``: log_softmax, the eos rule, the draw, the state);
    * a subclass's hook or a model output that wants gradients: the reference's ``log_softmax``, hook and
      eos masking, then ``pydrobert_amd::random_walk_advance``.

    A LookupLanguageModel gets the same tensors from the first two.  CPU tensors take the reference's loop.
    """

    __constants__ = ["eos", "default_hook"]

    def __init__(self, lm, eos: Optional[int] = None):
        eos = argcheck.is_int(eos, "eos", True)
        super().__init__()
        if eos is not None:
            if eos < -lm.vocab_size or eos > lm.vocab_size - 1:
                raise ValueError(
                    "Expected eos to be in the range [{}, {}], got {}".format(
                        -lm.vocab_size, lm.vocab_size - 1, eos
                    )
                )
            eos = (eos + lm.vocab_size) % lm.vocab_size
        self.lm, self.eos = lm, eos
        # (a constant: eager and scripted code take the same branches)
        self.default_hook = type(self).update_log_probs_for_step is RandomWalk.update_log_probs_for_step
        try:
            device = next(iter(lm.parameters())).device
        except StopIteration:
            device = torch.device("cpu")
        self.register_buffer("device_buffer", torch.empty(0, device=device))

    def reset_parameters(self) -> None:
        if hasattr(self.lm, "reset_parameters"):
            self.lm.reset_parameters()

    def extra_repr(self) -> str:
        return "eos={}".format(self.eos)

    def update_log_probs_for_step(self, log_probs_prev, log_probs_t, y_prev, y_prev_lens, eos_mask):
        """Hook (reference _decoding.py:1393-1436); identity by default."""
        return log_probs_prev, log_probs_t

    @torch.jit.unused
    def _table_walk(
        self, prev: Dict[str, torch.Tensor], N: int, max_iters: int
    ) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """Every chunk of iterations over a LookupLanguageModel's dense context table in ONE launch, the
        walks' state on the device between chunks and one host wait per chunk (walks still live, the longest
        walk).  ``None`` when the route does not apply."""
        lm = self.lm
        device = self.device_buffer.device
        if (type(lm) is not LookupLanguageModel or not self.default_hook or len(prev) or N < 1
                or not switches.get("PDT_WALK_TABLE")):  # fmt: skip
            return None
        if torch.is_grad_enabled() and any(p.requires_grad for p in lm.parameters()):
            return None
        dense = _dense_table(lm, device)
        if dense is None:
            return None
        table, stats, sos_row, U = dense
        R, V = table.shape
        has_eos = self.eos is not None
        L = _cabi.lib()
        with torch.no_grad(), _cabi.on_device(device):
            ctx = torch.full((N,), sos_row, device=device, dtype=torch.long)
            lens = torch.zeros((N,), device=device, dtype=torch.long)
            ended = torch.zeros((N,), device=device, dtype=torch.bool)
            lp = torch.zeros((N,), device=device, dtype=torch.float)
            ctl = torch.zeros((4,), device=device, dtype=torch.int32)
            y = torch.empty((0, N), device=device, dtype=torch.long)
            t, longest, stream = 0, 0, _cabi.stream_ptr(device)
            while t < max_iters:
                C = _walk_chunk(t, max_iters)
                u = torch.rand((C, N), device=device, dtype=torch.float)
                y_new = torch.empty((t + C, N), device=device, dtype=torch.long)
                y_new[:t] = y
                y = y_new
                _, live, longest = _walk_launch(
                    device,
                    lambda host: L.pdt_random_walk_table(
                        _cabi.ptr(table), table.stride(0), R, U, V, _cabi.ptr(stats), _cabi.ptr(u), N, C,
                        int(has_eos), int(self.eos or 0), y.data_ptr() + 8 * t * N, _cabi.ptr(ctx), _cabi.ptr(lens),
                        _cabi.ptr(ended), _cabi.ptr(lp), _cabi.ptr(ctl), host, stream,
                    ),
                    "RandomWalk",
                )  # fmt: skip
                if has_eos and live == 0:
                    break
                t += C
        # the reference leaves its loop at the first iteration that finds every walk ended
        T = min(max_iters, longest) if has_eos else max_iters
        return y[:T], lens, lp

    def _forward_torch(
        self, prev: Dict[str, torch.Tensor], N: int, max_iters: int
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        # the reference's loop (:1466-1507), for CPU tensors
        device = self.device_buffer.device
        y = torch.empty((0, N), device=device, dtype=torch.long)
        prev = self.lm.update_input(prev, y)
        y_lens = torch.zeros(N, dtype=torch.long, device=device)
        eos_mask = torch.zeros(N, device=device, dtype=torch.bool)
        log_probs = torch.zeros(N, device=device)
        for t in range(max_iters):
            if bool(eos_mask.all()):
                break
            t_ = torch.tensor(t, device=device)
            lp_t, prev = self.lm.calc_idx_log_probs(y[:t], prev, t_)
            lp_t = lp_t.log_softmax(-1)
            log_probs, lp_t = self.update_log_probs_for_step(log_probs, lp_t, y[:t], y_lens, eos_mask)
            if self.eos is not None:  # ended paths emit eos for free (:1483-1492)
                lp_t = lp_t.masked_fill(eos_mask.unsqueeze(1), -float("inf"))
                lp_t[:, self.eos] = lp_t[:, self.eos].masked_fill(eos_mask, 0.0)
            y, log_probs = random_walk_advance(lp_t, log_probs, y, y_lens)
            if self.eos is not None:
                y_lens = y_lens + (~eos_mask).long()
                eos_mask = y.gather(0, y_lens.unsqueeze(0) - 1).squeeze(0) == self.eos
            else:
                y_lens = y_lens + 1
        return y, y_lens, log_probs

    def forward(
        self,
        prev_: Optional[Dict[str, torch.Tensor]] = None,
        batch_size: Optional[int] = None,
        max_iters: Optional[int] = None,
        initial_state: Optional[Dict[str, torch.Tensor]] = None,
    ):
        # (``prev_``: the reference's runtime keyword, _decoding.py:1446-1449; ``initial_state``: its
        # documented call signature -- both are accepted)
        if initial_state is None:
            initial_state = prev_
        prev = dict() if initial_state is None else initial_state
        device = self.device_buffer.device
        N = 1 if batch_size is None else batch_size
        if max_iters is None:
            if self.eos is None:
                raise RuntimeError("max_iters must be set when eos is unset")
            max_iters = 1073741824
        elif max_iters < 0:
            raise RuntimeError("max_iters must be non-negative, got {}".format(max_iters))
        if device.type != "cuda":
            y, y_lens, log_probs = self._forward_torch(prev, N, max_iters)
        else:
            walked: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
            if not torch.jit.is_scripting():
                walked = self._table_walk(prev, N, max_iters)
            if walked is None:
                y, y_lens, log_probs = self._forward_hip(prev, N, max_iters)
            else:
                y, y_lens, log_probs = walked
        if batch_size is None:
            y, y_lens, log_probs = y.squeeze(1), y_lens.squeeze(0), log_probs.squeeze(0)
        return y, y_lens, log_probs

    def _forward_hip(
        self, prev: Dict[str, torch.Tensor], N: int, max_iters: int
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        # The reference's loop (:1466-1507) around any model: the model's call every iteration, then ONE kernel
        # (pydrobert_amd::random_walk_step) with the default hook and an output that wants no gradient, else the
        # reference's log_softmax / hook / eos masking and pydrobert_amd::random_walk_advance.  The uniforms of
        # iterations [t, t + C) come from one torch.rand((C, N)) after the model's call of iteration t (the
        # chunks of _walk_chunk), and y grows by the chunk.  The one host read per iteration -- whether some
        # walk is still live -- comes back with the step's kernel: the model is called exactly as often as
        # under the reference.
        device = self.device_buffer.device
        y = torch.empty((0, N), device=device, dtype=torch.long)
        prev = self.lm.update_input(prev, y)
        y_lens = torch.zeros(N, dtype=torch.long, device=device)
        eos_mask = torch.zeros(N, device=device, dtype=torch.bool)
        log_probs = torch.zeros(N, device=device)
        ctl = torch.zeros((4,), device=device, dtype=torch.int32)
        u = torch.empty((0, N), device=device)
        fused = self.default_hook
        out_dtype = log_probs.dtype
        live, u_from, u_to, T = N, 0, 0, 0
        for t in range(max_iters):
            if self.eos is not None and live == 0:
                break
            t_ = torch.tensor(t, device=device)
            lp_t, prev = self.lm.calc_idx_log_probs(y[:t], prev, t_)
            if t == u_to:
                u_from, u_to = t, t + _walk_chunk(t, max_iters)
                u = torch.rand((u_to - t, N), device=device, dtype=torch.float)
                y_new = torch.empty((u_to, N), device=device, dtype=torch.long)
                y_new[:t] = y[:t]
                y = y_new
            fused = fused and not lp_t.requires_grad
            if fused:
                out_dtype = torch.promote_types(out_dtype, lp_t.dtype)
                live = torch.ops.pydrobert_amd.random_walk_step(
                    lp_t, u[t - u_from], y, t, y_lens, eos_mask, log_probs, ctl, self.eos
                )
            else:
                lp_t = lp_t.log_softmax(-1)
                log_probs, lp_t = self.update_log_probs_for_step(log_probs, lp_t, y[:t], y_lens, eos_mask)
                if self.eos is not None:  # ended paths emit eos for free (:1483-1492)
                    lp_t = lp_t.masked_fill(eos_mask.unsqueeze(1), -float("inf"))
                    lp_t[:, self.eos] = lp_t[:, self.eos].masked_fill(eos_mask, 0.0)
                y_t, log_probs = torch.ops.pydrobert_amd.random_walk_advance(
                    lp_t, u[t - u_from], log_probs, y[:0], None
                )
                y = y.index_copy(0, t_.view(1), y_t)  # (not in place: the model may have saved views of y)
                if self.eos is not None:
                    y_lens = y_lens + (~eos_mask).long()
                    eos_mask = eos_mask | (y_t[0] == self.eos)
                    live = 0 if bool(eos_mask.all()) else 1
                else:
                    y_lens = y_lens + 1
            T = t + 1
        return y[:T], y_lens, log_probs.to(torch.promote_types(out_dtype, log_probs.dtype))


class TokenSequenceConstraint(constraints.Constraint):
    """Completed token sequences (reference _decoding.py:1724-1770): vectors of integers in ``[0, vocab_size)``
    that either have ``max_iters`` elements, or have at most that many (any number when unset) and contain
    ``eos``.  Whatever follows the first ``eos`` of a sequence is ignored."""

    vocab_size: int
    eos: Optional[int]
    max_iters: Union[int, float]
    is_discrete = True
    event_dim = 1

    def __init__(self, vocab_size: int, eos: Optional[int] = None, max_iters: Optional[int] = None) -> None:
        vocab_size = argcheck.is_posi(vocab_size, "vocab_size")
        if eos is None and max_iters is None:
            raise ValueError("At least one of max_iters or eos must be non-none")
        eos = argcheck.is_int(eos, "eos", True)
        max_iters = argcheck.is_nonnegi(max_iters, "max_iters", True)
        super().__init__()
        self.vocab_size, self.eos = vocab_size, eos
        self.max_iters = float("inf") if max_iters is None else max_iters

    def check(self, value: torch.Tensor):
        completed = value.size(-1) == self.max_iters
        if self.eos is not None:
            if value.device.type == "cuda":
                value = fill_after_eos(value, self.eos, -1)
            else:  # (the kernel's rule in torch ops: constraints are checked on the CPU too)
                is_eos = value == self.eos
                value = value.masked_fill((is_eos.cumsum(-1) - is_eos.long()) > 0, self.eos)
            completed = (value == self.eos).any(-1) & (value.size(-1) <= self.max_iters) | completed
        in_vocab = ((value % 1 == 0) & (value >= 0) & (value < self.vocab_size)).all(-1)
        return in_vocab & completed


class SequentialLanguageModelDistribution(torch.distributions.distribution.Distribution):
    """A :class:`RandomWalk` over a :class:`SequentialLanguageModel` as a ``Distribution`` (reference
    _decoding.py:1773-2029), the object the sequence-level estimators are written against.

    :func:`sample` runs the walk; :func:`log_prob` runs the model over the given sequences and
    :class:`SequenceLogProbabilities`; :func:`enumerate_support` (``max_iters`` set) lists every sequence, with
    those that agree up to their first ``eos`` merged.  All three run on this package's kernels.

    Two batching modes.  With ``batch_size`` unset the samples themselves are the model's batch:
    ``sample()`` is ``(T,)`` and ``sample([M])`` is ``(M, T)``, drawn in one walk.  With ``batch_size = N`` (a
    model conditioned on N inputs through ``initial_state``) ``sample()`` is ``(N, T)`` and ``sample([M])`` is
    ``(M, N, T)``: M walks of batch N one after the other, stacked, and padded with ``eos`` to one length.

    ``cache_samples`` keeps the last samples with their log probabilities, so that a :func:`log_prob` of the
    value just drawn costs a comparison, until :func:`clear_cache` or the next value.  As in the reference, the
    log probabilities are those of the default ``update_log_probs_for_step``; a subclassed walk's adjusted ones
    are what :func:`sample` caches.
    """

    arg_constraints = dict()

    def __init__(
        self,
        random_walk: RandomWalk,
        batch_size: Optional[int] = None,
        initial_state: Optional[Dict[str, torch.Tensor]] = None,
        max_iters: Optional[int] = None,
        cache_samples: bool = False,
        validate_args: Optional[bool] = None,
    ):
        if batch_size is None:
            batch_shape = torch.Size([])
        else:
            batch_shape = torch.Size([argcheck.is_posi(batch_size, "batch_size")])
        if max_iters is None:
            if random_walk.eos is None:
                raise ValueError("random_walk.eos must be set if max_iters isn't")
            event_shape = torch.Size([1])
        else:
            max_iters = argcheck.is_nonnegi(max_iters, "max_iters")
            event_shape = torch.Size([max_iters])
        cache_samples = argcheck.is_bool(cache_samples, "cache_samples")
        validate_args = argcheck.is_bool(validate_args, "validate_args", True)
        self.random_walk = random_walk
        super().__init__(batch_shape, event_shape, validate_args)
        self.initial_state = dict() if initial_state is None else initial_state
        self.cache_samples, self.max_iters = cache_samples, max_iters
        self._samples_cache: Optional[torch.Tensor] = None
        self._log_probs_cache: Optional[torch.Tensor] = None
        if self._validate_args and not all(
            isinstance(k, str) and isinstance(v, torch.Tensor) for k, v in self.initial_state.items()
        ):
            raise ValueError("initial_state is not a dictionary of str:Tensor")

    def _validate_sample(self, value: torch.Tensor):
        # (the event dimension is as long as the walk was; its length is the support's to check)
        exp_shape, act_shape = tuple(self.batch_shape + self.event_shape), tuple(value.shape)
        try:
            torch.broadcast_shapes(exp_shape, act_shape)
        except RuntimeError:
            raise ValueError(
                "value of shape {} cannot broadcast with batch_shape+event_shape {}".format(act_shape, exp_shape)
            )
        ok = self.support.check(value)
        if not ok.all():
            raise ValueError("value of shape {} has values outside of the support: {}".format(act_shape, ok))

    @constraints.dependent_property
    def support(self):
        return TokenSequenceConstraint(self.random_walk.lm.vocab_size, self.random_walk.eos, self.max_iters)

    def sample(self, sample_shape: torch.Size = torch.Size([])) -> torch.Tensor:
        shape = list(self._extended_shape(sample_shape))
        num_samples = 1
        for d in sample_shape:
            num_samples *= d
        walk = self.random_walk
        if num_samples == 0:
            return torch.empty(shape, device=walk.device_buffer.device)
        if len(self.batch_shape):
            drawn = [walk(self.initial_state.copy(), self.batch_shape[0], self.max_iters) for _ in range(num_samples)]
            log_probs = torch.stack([d[2] for d in drawn])
            if walk.eos is None:  # (every walk took max_iters steps)
                samples = torch.stack([d[0].T for d in drawn])
            else:  # walks of different lengths: padded with eos to the longest
                samples = torch.nn.utils.rnn.pad_sequence([d[0] for d in drawn], padding_value=walk.eos)
                samples = samples.flatten(1).T
        else:
            samples, _, log_probs = walk(self.initial_state.copy(), num_samples, self.max_iters)
            samples = samples.T
        shape[-1] = samples.size(-1)
        samples = samples.reshape(shape)
        if self.cache_samples:
            self._samples_cache = samples
            self._log_probs_cache = log_probs.view(shape[:-1])
        return samples

    @property
    def has_enumerate_support(self) -> bool:
        return self.max_iters is not None

    def enumerate_support(self, expand=True) -> torch.Tensor:
        if not self.has_enumerate_support:
            raise NotImplementedError("random_walk.max_iters must be set in order to enumerate support")
        walk = self.random_walk
        support = enumerate_vocab_sequences(self.max_iters, walk.lm.vocab_size, walk.device_buffer.device)
        if walk.eos is not None:
            support = torch.unique(fill_after_eos(support, walk.eos, 1), dim=0)
        if len(self.batch_shape):
            support = support.view((-1,) + (1,) * len(self.batch_shape) + support.shape[-1:])
            if expand:
                support = support.expand((-1,) + self.batch_shape + support.shape[-1:])
        return support

    def clear_cache(self):
        """Forget the cached samples and their log probabilities."""
        self._samples_cache = self._log_probs_cache = None

    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        if self._validate_args:
            self._validate_sample(value)
        batch_size = self.batch_shape[0] if len(self.batch_shape) else 1
        num_samples = value.numel() // (batch_size * value.size(-1))
        shape = value.shape[:-1]
        if num_samples == 0:
            return torch.empty(shape, device=value.device)
        if (
            self.cache_samples
            and self._samples_cache is not None
            and self._samples_cache.shape == value.shape
            and (self._samples_cache == value).all()
        ):
            assert self._log_probs_cache is not None
            return self._log_probs_cache
        if self.cache_samples:
            self._samples_cache = value
        lm = self.random_walk.lm
        if len(self.batch_shape):  # one call of the model per sample, each over the batch
            value = value.reshape((-1,) + value.shape[-2:]).transpose(1, 2)
            log_probs = torch.stack([lm(hist[:-1].long(), self.initial_state.copy()) for hist in value])
        else:  # every sample in one batch
            value = value.reshape(-1, value.size(-1))
            log_probs = lm(value.T[:-1].long(), self.initial_state.copy()).transpose(0, 1)
        log_probs = SequenceLogProbabilities(1, self.random_walk.eos)(log_probs, value.long()).view(shape)
        if self.cache_samples:
            self._log_probs_cache = log_probs
        return log_probs
