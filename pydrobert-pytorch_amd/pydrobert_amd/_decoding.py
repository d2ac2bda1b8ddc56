"""Beam-search decoding on MI355X.

Host-side mirror of the reference's ``_decoding.py`` for the operators on the hot path:
``ctc_prefix_search`` / ``CTCPrefixSearch`` and ``BeamSearch``, with the caches of the n-gram
tables they search over.  The fused CTC search runs in ``csrc/ctc_search.hip``, BeamSearch's
iterations in ``csrc/beam_step.hip`` and ``csrc/beam_search_table.hip``, through the C ABI
(``include/pdt_amd.h``); the Modules keep the reference's control flow around a user-supplied
language model.  The step functions are in ``_step.py``, greedy search and sequence
log-probabilities in ``_seqops.py``, the random walks in ``_walk.py``.
"""
import ctypes
import math
import weakref
from typing import Dict, Optional, Tuple

import torch
from torch.library import custom_op

from . import _cabi, argcheck, config, switches
from ._lm import ExtractableSequentialLanguageModel, LookupLanguageModel, MixableSequentialLanguageModel
from ._step import _ctc_step_with_lm_scores, _f32, _i64, _logits_elem, ctc_prefix_search_advance

__all__ = ["BeamSearch", "CTCPrefixSearch", "ctc_prefix_search"]

MAX_CTC_WIDTH = 128  # one launch: the wave-wide kernels up to MAX_CTC_WAVE_WIDTH, csrc/ctc_search_wide.hip beyond
MAX_CTC_WAVE_WIDTH = 32


@custom_op("pydrobert_amd::ctc_prefix_search", mutates_args=())
def _ctc_prefix_search_op(
    logits: torch.Tensor, width: int, lens: Optional[torch.Tensor]
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    if logits.dim() != 3:
        raise RuntimeError("logits must be 3 dimensional")  # :1073-1074
    device = _cabi.require_hip(logits, lens)
    T, N, Vp1 = logits.shape
    V = Vp1 - 1
    if V < 1:
        raise RuntimeError("logits must have at least one non-blank class")
    if width < 1:
        raise RuntimeError("width must be positive")
    if width > MAX_CTC_WIDTH:  # (CTCPrefixSearch / ctc_prefix_search run such beams frame by frame)
        raise RuntimeError("the one-kernel search holds at most {} prefixes".format(MAX_CTC_WIDTH))
    wide = width > MAX_CTC_WAVE_WIDTH
    dtype = logits.dtype
    logits, elem = _logits_elem(logits)  # (float16 / bfloat16: read as they are, no float32 copy)
    if lens is None:
        S = T
    elif lens.dim() != 1:
        raise RuntimeError("lens must be 1 dimensional")  # :1084-1085
    elif lens.size(0) != N:
        raise RuntimeError("expected dim 0 of lens to be {}, got {}".format(N, lens.size(0)))
    else:
        lens = _i64(lens).contiguous()
        S = int(lens.max().item()) if N else 0  # the reference's len_max host read (:1089)
        S = max(0, min(S, T))
    L = _cabi.lib()
    with torch.cuda.device(device):
        y = torch.empty((S, N, width), device=device, dtype=torch.long)
        y_lens = torch.empty((N, width), device=device, dtype=torch.long)
        y_probs = torch.empty((N, width), device=device, dtype=torch.float)
        ws_bytes = L.pdt_ctc_prefix_search_wide_workspace_bytes if wide else L.pdt_ctc_prefix_search_workspace_bytes
        ws = torch.empty((int(ws_bytes(T, N, V, width)),), device=device, dtype=torch.uint8)
        args = (
            _cabi.ptr(logits), T, N, V, logits.stride(0), logits.stride(1), logits.stride(2),
            _cabi.ptr(lens), int(width), S, _cabi.ptr(y), _cabi.ptr(y_lens), _cabi.ptr(y_probs),
            _cabi.ptr(ws), _cabi.stream_ptr(device),
        )  # fmt: skip
        if elem:  # float16 / bfloat16: the entry point that takes the element type
            rc = (L.pdt_ctc_prefix_search_wide_elem if wide else L.pdt_ctc_prefix_search_elem)(*args, elem)
        else:
            rc = (L.pdt_ctc_prefix_search_wide if wide else L.pdt_ctc_prefix_search)(*args)
    _cabi.check(rc, "pdt_ctc_prefix_search_wide" if wide else "pdt_ctc_prefix_search")
    return y, y_lens, y_probs.to(dtype)


@_ctc_prefix_search_op.register_fake
def _(logits, width, lens):
    T, N = logits.shape[0], logits.shape[1]
    S = T if lens is None else torch.library.get_ctx().new_dynamic_size()  # lens.max() (:1089)
    return (
        logits.new_empty((S, N, width), dtype=torch.long),
        logits.new_empty((N, width), dtype=torch.long),
        logits.new_empty((N, width)),
    )


def ctc_prefix_search(
    logits: torch.Tensor, width: int, lens: Optional[torch.Tensor] = None
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``CTCPrefixSearch(width)(logits, lens)`` without a language model, as ONE kernel.

    Reference: ``CTCPrefixSearch.forward`` (_decoding.py:1064-1202) with ``lm=None``.
    Returns ``(y (S, N, width) int64, y_lens (N, width) int64, y_probs (N, width))``; rows of
    ``y`` beyond ``y_lens`` are zero (the reference leaves them undefined).  The fused kernel's
    probabilities are cut off from the graph; logits that require grad take the frame-by-frame
    route of :class:`CTCPrefixSearch` instead (same beams, differentiable probabilities).
    """
    if torch.jit.is_scripting() or not (
        width > 128 or (torch.is_grad_enabled() and logits.requires_grad)  # (128: MAX_CTC_WIDTH)
    ):
        return torch.ops.pydrobert_amd.ctc_prefix_search(logits, width, lens)
    return CTCPrefixSearch(width)(logits, lens)


class CTCPrefixSearch(torch.nn.Module):
    """Beam search over CTC prefixes, optionally with shallow fusion (reference
    _decoding.py:937-1204).

    Without a language model (``lm=None`` or ``beta == 0``) the whole search is one fused
    kernel.  With one, the reference's per-frame loop is kept -- the LM forward is the
    user's PyTorch code -- and each frame's prefix bookkeeping is one kernel
    (``ctc_prefix_search_advance``).
    """

    __constants__ = ["width", "beta", "valid_mixture"]

    def __init__(
        self,
        width: int,
        beta: float = 0.2,
        lm: Optional[MixableSequentialLanguageModel] = None,
        valid_mixture: bool = False,
    ):
        width = argcheck.is_posi(width, name="width")
        beta = argcheck.is_closed01(beta, name="beta")
        valid_mixture = argcheck.is_bool(valid_mixture, "valid_mixture")
        super().__init__()
        self.width, self.beta, self.valid_mixture = width, beta, valid_mixture
        if lm is None:
            self.add_module("lm", None)
        else:
            self.lm = lm

    def reset_parameters(self) -> None:
        if self.lm is not None and hasattr(self.lm, "reset_parameters"):
            self.lm.reset_parameters()

    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)

    def forward(
        self,
        logits: torch.Tensor,
        lens: Optional[torch.Tensor] = None,
        prev_: Optional[Dict[str, torch.Tensor]] = None,
        initial_state: Optional[Dict[str, torch.Tensor]] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        # (``prev_`` is the reference's runtime keyword, _decoding.py:1064-1068; ``initial_state`` the
        # name its documented call signature uses, :1053-1060 -- both are accepted)
        if initial_state is None:
            initial_state = prev_
        if logits.dim() != 3:
            raise RuntimeError("logits must be 3 dimensional")
        # The one-kernel search returns probabilities that are cut off from the graph.  When the
        # caller wants gradients with respect to the logits (the reference's probabilities are
        # differentiable, _decoding.py:1093, :1188), the search runs frame by frame instead: every
        # frame is one kernel whose masses carry an autograd formula.
        # Beams wider than the one-kernel search holds (128 prefixes) also go frame by frame, on the
        # plain step kernel (csrc/advance_wide.hip).
        stepwise = (torch.is_grad_enabled() and logits.requires_grad) or self.width > 128  # (MAX_CTC_WIDTH; TorchScript takes no globals)
        prev: Dict[str, torch.Tensor] = dict()
        if initial_state is not None:
            prev = initial_state
        if self.lm is None:
            if stepwise:
                return self._frame_by_frame(logits, lens, prev)
            return ctc_prefix_search(logits, self.width, lens)
        else:
            if self.lm.vocab_size != logits.size(2) - 1:
                raise RuntimeError(
                    "Expected dim 2 of logits to be {}, got {}".format(self.lm.vocab_size + 1, logits.size(2))
                )
            if self.beta == 0.0 and not stepwise:
                return ctc_prefix_search(logits, self.width, lens)
            return self._frame_by_frame(logits, lens, prev)

    @torch.jit.unused
    def _fuses_lookup_lm(self, logits: torch.Tensor) -> bool:
        """Whether the search with the language model in the loop can run from one call of the library
        (csrc/ctc_lm_step.hip, csrc/ctc_lm_table.hip): the model is this package's n-gram
        LookupLanguageModel with its own scoring methods (a subclass that overrides them must be called),
        of order two or more with its forward index built, the beam fits the frame routine, the logits
        are float32 and nothing wants gradients."""
        lm = self.lm
        if type(lm) is not LookupLanguageModel or not switches.get("PDT_CTC_LM_FUSED"):
            return False
        if lm.max_ngram < 2 or self.width > 32 or self.beta == 0.0 or logits.device.type != "cuda":
            return False
        if logits.dtype != torch.float:
            return False
        if lm.succ_start.numel() != lm.vocab_size + lm.shift + 2 or lm.logps.device != logits.device:
            return False
        return not (torch.is_grad_enabled() and logits.requires_grad)

    @torch.jit.unused
    def _lookup_lm_search(
        self, probs: torch.Tensor, lens: Optional[torch.Tensor], n_frames: int
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Every frame of the search with the n-gram model in the loop from ONE call of the library
        (include/pdt_amd.h: pdt_ctc_lookup_lm_search): every frame in one launch, the beam's state and
        histories in a workspace in between."""
        lm, W = self.lm, self.width
        T, N, V = probs.size(0), probs.size(1), probs.size(2) - 1
        device = _cabi.require_hip(probs, lens, *_lm_buffers(lm))
        probs = _f32(probs)
        L = _cabi.lib()
        with torch.cuda.device(device):
            y = torch.empty((n_frames, N, W), device=device, dtype=torch.long)
            y_lens = torch.empty((N, W), device=device, dtype=torch.long)
            nb = torch.empty((N, W), device=device, dtype=torch.float)
            b = torch.empty((N, W), device=device, dtype=torch.float)
            if N:
                ws_bytes = int(L.pdt_ctc_lookup_lm_search_workspace_bytes(n_frames, N, V, W, lm.max_ngram, V + lm.shift + 1))
                ws = torch.empty(ws_bytes, device=device, dtype=torch.uint8)
                lens_dev = None if lens is None else _i64(lens).contiguous()
                rc = L.pdt_ctc_lookup_lm_search(
                    _cabi.ptr(probs), probs.stride(0), probs.stride(1), probs.stride(2), _cabi.ptr(lens_dev),
                    n_frames, N, V, W, _cabi.ptr(lm.logps), _cabi.ptr(lm.logbs), _cabi.ptr(lm.child_start),
                    _cabi.ptr(lm.ids_wide), _cabi.ptr(lm.succ_start), _cabi.ptr(lm.succ_tok),
                    _cabi.ptr(lm.succ_node), lm.max_ngram, V + lm.shift + 1, lm.sos, float(self.beta),
                    int(self.valid_mixture), _cabi.ptr(y), _cabi.ptr(y_lens), _cabi.ptr(nb), _cabi.ptr(b),
                    _cabi.ptr(ws), ws_bytes, _cabi.stream_ptr(device),
                )  # fmt: skip
                _cabi.check(rc, "pdt_ctc_lookup_lm_search")
        return y, y_lens, nb + b

    @torch.jit.unused
    def _searches_through_a_factor_table(self, n_frames: int) -> bool:
        """Of the searches :meth:`_fuses_lookup_lm` admits, those whose (contexts, V) factor table is
        small enough and whose sizes the kernel's host plan takes: the search of csrc/ctc_lm_table.hip
        (PDT_CTC_LM_TABLE=0: the one of csrc/ctc_lm_step.hip, for comparisons)."""
        lm = self.lm
        if not switches.get("PDT_CTC_LM_TABLE"):
            return False
        V = lm.vocab_size
        # (a row per context: U^(order - 1) of them -- 4 MB for a bigram model over 1000 tokens, 4 GB for a
        # trigram model: the card has 288)
        rows = (V + 1) ** (lm.max_ngram - 1)
        if not (V + 1 <= 80 * 64 and rows < (1 << 30) and rows * V * 4 <= _FACTOR_TABLE_MAX_BYTES):
            return False
        return _lm_table_plan(n_frames, V, self.width) is not None

    @torch.jit.unused
    def _searches_from_one_call(self) -> bool:
        """Of the searches :meth:`_fuses_lookup_lm` admits, those whose rows fit a workgroup's LDS in
        csrc/ctc_lm_step.hip (two rows of V floats and the beam's tables in 160 KB: about twenty thousand
        tokens); larger vocabularies go frame by frame, which takes any."""
        return int(_cabi.lib().pdt_ctc_lookup_lm_search_lds_bytes(self.lm.vocab_size, self.width)) > 0

    @torch.jit.unused
    def _lm_table_search(
        self, logits: torch.Tensor, lens: Optional[torch.Tensor], n_frames: int
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The whole search in one launch, the softmax of the logits included, the model's factor rows
        read from a table (include/pdt_amd.h: pdt_ctc_lm_table_search)."""
        lm, W = self.lm, self.width
        T, N, V = logits.size(0), logits.size(1), logits.size(2) - 1
        device = _cabi.require_hip(logits, lens, *_lm_buffers(lm))
        logits = _f32(logits)
        factors, fmax, sos_row, ctx_base = _factor_table(lm, self.beta, self.valid_mixture, device)
        L = _cabi.lib()
        with torch.cuda.device(device):
            y = torch.empty((n_frames, N, W), device=device, dtype=torch.long)
            y_lens = torch.empty((N, W), device=device, dtype=torch.long)
            y_probs = torch.empty((N, W), device=device, dtype=torch.float)
            if N:
                ws = torch.empty(int(L.pdt_ctc_lm_table_search_workspace_bytes(n_frames, N, V, W)), device=device,
                                 dtype=torch.uint8)
                lens_dev = None if lens is None else _i64(lens).contiguous()
                rc = L.pdt_ctc_lm_table_search(
                    _cabi.ptr(logits), n_frames, N, V, logits.stride(0), logits.stride(1), logits.stride(2),
                    _cabi.ptr(lens_dev), W, n_frames, _cabi.ptr(factors), _cabi.ptr(fmax), factors.size(0),
                    factors.stride(0), sos_row, ctx_base, factors.size(0) // ctx_base,
                    float(self.beta), int(self.valid_mixture), _cabi.ptr(y), _cabi.ptr(y_lens), _cabi.ptr(y_probs),
                    _cabi.ptr(ws), _cabi.stream_ptr(device),
                )  # fmt: skip
                _cabi.check(rc, "pdt_ctc_lm_table_search")
        return y, y_lens, y_probs

    def _frame_by_frame(
        self, logits: torch.Tensor, lens: Optional[torch.Tensor], state: Dict[str, torch.Tensor]
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One ``ctc_prefix_search_advance`` kernel per frame, around the user's language model
        when there is one (the semantics of reference _decoding.py:1083-1202).  Utterances whose
        frames have run out are frozen on the device (a ``where`` per state tensor); the only
        host read is the number of frames to run."""
        T, N, V, W = logits.size(0), logits.size(1), logits.size(2) - 1, self.width
        device, dtype = logits.device, logits.dtype
        n_frames = T
        if lens is not None:
            if lens.dim() != 1:
                raise RuntimeError("lens must be 1 dimensional")
            if lens.size(0) != N:
                raise RuntimeError("expected dim 0 of lens to be {}, got {}".format(N, lens.size(0)))
            n_frames = min(T, int(lens.max().item())) if N else 0
        if not torch.jit.is_scripting():
            # this package's n-gram model in the loop: the whole search from one call of the library
            if self.lm is not None and self.beta != 0.0 and n_frames > 0 and self._fuses_lookup_lm(logits):
                if self._searches_through_a_factor_table(n_frames):
                    return self._lm_table_search(logits, lens, n_frames)
                if self._searches_from_one_call():
                    return self._lookup_lm_search(logits.softmax(2), lens, n_frames)
        probs = logits.softmax(2)
        # beam state: one empty prefix per utterance, all of its mass on "ends in blank"
        nb = torch.zeros((N, 1), device=device, dtype=dtype)
        b = torch.ones((N, 1), device=device, dtype=dtype)
        y = torch.empty((0, N, 1), dtype=torch.long, device=device)
        y_lens = torch.zeros((N, 1), dtype=torch.long, device=device)
        y_last = y_lens
        is_prefix = torch.ones((N, 1, 1), device=device, dtype=torch.bool)
        fuse = self.beta != 0.0
        if self.lm is not None and fuse:
            state = self.lm.update_input(state, y)
        Kp = 1
        # row of batch element n's first prefix in the flattened (N * K') LM state, before and after
        # the beam has its full width
        first_rows = torch.arange(0, N, 1, device=device).unsqueeze(1)
        beam_rows = torch.arange(0, W * N, W, device=device).unsqueeze(1)
        for t in range(n_frames):
            nonext_t, blank_t = probs[t, :, :V], probs[t, :, V]
            ext_t = nonext_t.unsqueeze(1).expand(N, Kp, V)
            state_next: Dict[str, torch.Tensor] = dict()
            mix_in_step = False
            lm_lp = nonext_t
            if self.lm is not None:
                if fuse:
                    lm_lp, state_next = self.lm.calc_idx_log_probs(y.flatten(1), state, y_lens.flatten())
                    if not (torch.is_grad_enabled() and (lm_lp.requires_grad or probs.requires_grad)):
                        # one pass over the LM scores instead of four (csrc/fusion_ext.hip) -- scripted;
                        # else inside the step kernel itself, below
                        if torch.jit.is_scripting():
                            ext_t = torch.ops.pydrobert_amd.fusion_ext(
                                lm_lp.reshape(N * Kp, V), nonext_t, blank_t, self.beta, self.valid_mixture
                            )
                        else:
                            mix_in_step = True
                    elif self.valid_mixture:  # convex combination that still sums to 1 - blank (:1120-1128)
                        lm_p = lm_lp.softmax(-1).view(N, Kp, V) * (1 - blank_t.view(N, 1, 1))
                        ext_t = (1.0 - self.beta) * ext_t + self.beta * lm_p
                    else:  # shallow fusion: p_ctc * p_lm ** beta (:1130-1135)
                        ext_t = ext_t * (self.beta * lm_lp.log_softmax(-1)).exp().view(N, Kp, V)
            if torch.jit.is_scripting():
                y_new, last_new, lens_new, masses, is_prefix, src, kept = ctc_prefix_search_advance(
                    (ext_t, nonext_t, blank_t), W, (nb, b), y, y_last, y_lens, is_prefix
                )
                nb_new, b_new = masses
            else:
                if mix_in_step:
                    y_new, last_new, lens_new, nb_new, b_new, is_prefix, src, kept = _ctc_step_with_lm_scores(
                        lm_lp.reshape(N, Kp, V), self.beta, self.valid_mixture, nonext_t, blank_t, W, nb, b, y,
                        y_last, y_lens, is_prefix,
                    )  # fmt: skip
                else:
                    y_new, last_new, lens_new, masses, is_prefix, src, kept = ctc_prefix_search_advance(
                        (ext_t, nonext_t, blank_t), W, (nb, b), y, y_last, y_lens, is_prefix
                    )
                    nb_new, b_new = masses
            if self.lm is not None:
                if fuse:
                    rows = (src + (first_rows if Kp == 1 else beam_rows)).flatten()
                    state = self.lm.mix_by_mask(
                        self.lm.extract_by_src(state, rows), self.lm.extract_by_src(state_next, rows), kept.flatten()
                    )  # :1154-1163
            if lens is not None:
                live = (lens > t).unsqueeze(1)  # (N, 1): utterances that still have this frame
                if Kp < W:  # the first frame: widen the old state with absent entries
                    absent = nb.new_full((N, W - Kp), -float("inf"))
                    nb, b = torch.cat([nb, absent], 1), torch.cat([b, absent], 1)
                    y, y_lens = y.expand(-1, -1, W), y_lens.expand(-1, W)
                y_old = torch.cat([y, y.new_zeros((1, N, W))], 0)
                y_new = torch.where(live.unsqueeze(0), y_new, y_old)
                lens_new = torch.where(live, lens_new, y_lens)
                nb_new, b_new = torch.where(live, nb_new, nb), torch.where(live, b_new, b)
            y, y_last, y_lens, nb, b, Kp = y_new, last_new, lens_new, nb_new, b_new, W
        y = y.contiguous()
        total = nb + b
        if Kp < W:  # no frame at all: fill the beam with absent entries (:1190-1200)
            y, y_lens = y.repeat(1, 1, W), y_lens.repeat(1, W)
            total = torch.cat([total, total.new_full((N, W - Kp), -float("inf"))], 1)
        return y, y_lens, total


def _lm_buffers(lm: "LookupLanguageModel"):
    """Every trie buffer of an n-gram model the kernels read through raw pointers."""
    return (lm.logps, lm.logbs, lm.child_start, lm.ids_wide, lm.succ_start, lm.succ_tok, lm.succ_node)


def _identity_of(*tensors):
    """(address, version) of every tensor, or None when one carries no version counter (inference
    tensors): then there is nothing to recognise an unchanged tensor by and the caller rebuilds."""
    try:
        return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tensors)
    except RuntimeError:
        return None


# dense tables of LookupLanguageModels, per model object: a bigram model's (_dense_table: BeamSearch's and
# RandomWalk's), those of order 3 and up (_dense_table: RandomWalk's), and the factor table of the last mix
# CTCPrefixSearch searched a model with (_factor_table)
_BIGRAM_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_CONTEXT_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_FACTOR_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_DENSE_TABLE_MAX_BYTES = 64 << 20  # (the table stays in the 256 MiB Infinity Cache)
_FACTOR_TABLE_MAX_BYTES = 6 << 30  # (a trigram model over 1000 tokens: 4 GB of this card's 288)


def _cached_table(cache, lm: "LookupLanguageModel", device: torch.device, build, *params):
    """``cache[lm]``'s table when it was built on ``device`` with ``params`` from every trie buffer of ``lm``
    as it is now (the same tensor at the same version), else ``build()``'s, kept in its place.  Models whose
    buffers carry no version counter -- built under inference_mode -- get a fresh table per call.  Writes the
    counter does not see (``.data``, raw pointers) are the caller's to announce: ``del cache[lm]``."""
    ident = _identity_of(*_lm_buffers(lm))
    key = None if ident is None else (ident, str(device)) + params
    ent = cache.get(lm)
    if key is not None and ent is not None and ent[0] == key:
        return ent[1:]
    table = build()
    if key is not None:
        cache[lm] = (key,) + table
    return table


def _context_scores(lm: "LookupLanguageModel", device: torch.device):
    """``(scores (U^(n-1), V) float32, sos_row, U)`` of an n-gram model: its scores after EVERY context of
    ``n - 1`` symbols -- row ``r`` = the context whose symbols are the digits of ``r`` in base ``U``, oldest
    first; the symbols are the V tokens, then the start-of-sequence token when it lies outside the vocabulary
    (``U = V + 1``); ``sos_row`` = the all-sos context of the empty prefix (the reference pads short
    histories with sos, _lm.py:403-515).  One call of the model's own scoring kernel."""
    V, shift = lm.vocab_size, lm.shift
    U, n1 = V + shift, lm.max_ngram - 1
    sos_sym = lm.sos if shift == 0 else V
    with torch.no_grad():
        rows = torch.arange(U**n1, device=device)
        digits = [(rows // (U ** (n1 - 1 - i))) % U for i in range(n1)]
        hist = torch.stack(digits)  # (order - 1, rows), oldest symbol first
        if shift:
            hist = torch.where(hist == V, torch.full_like(hist, lm.sos), hist)
        table, _ = lm.calc_idx_log_probs(hist, dict(), torch.tensor(n1, device=device))
    sos_row = sum(sos_sym * U**i for i in range(n1))
    return _f32(table).contiguous(), sos_row, U


def _dense_table(lm: "LookupLanguageModel", device: torch.device):
    """``(table (U^(n-1), V), stats (U^(n-1), 2), sos_row, U)`` of an n-gram :class:`LookupLanguageModel`
    whose dense context table (_context_scores) stays within _DENSE_TABLE_MAX_BYTES on ``device``, else
    ``None``; ``stats`` = every row's maximum and log-sum-exp (pdt_row_log_softmax_stats).  Built once per
    model and device, kept while the model's buffers are unchanged (_cached_table)."""
    V = lm.vocab_size
    U, n1 = V + lm.shift, lm.max_ngram - 1
    if n1 < 1 or (U**n1) * V * 4 > _DENSE_TABLE_MAX_BYTES or lm.logps.device != device:
        return None

    def build():
        table, sos_row, _ = _context_scores(lm, device)
        R = table.size(0)
        with torch.no_grad():
            stats = torch.empty((R, 2), device=device, dtype=torch.float)
            with torch.cuda.device(device):
                rc = _cabi.lib().pdt_row_log_softmax_stats(
                    _cabi.ptr(table), table.stride(0), table.stride(1), R, V, _cabi.ptr(stats),
                    _cabi.stream_ptr(device),
                )
            _cabi.check(rc, "pdt_row_log_softmax_stats")
        return table, stats, sos_row, U

    return _cached_table(_BIGRAM_TABLES if n1 == 1 else _CONTEXT_TABLES, lm, device, build)


def _lm_table_plan(n_frames: int, V: int, width: int):
    """``(checkpoint shift, checkpoints, chunks of the kernel instance, its constant width or 0, ring bytes,
    LDS bytes)`` of the factor-table search for these sizes (include/pdt_amd.h: pdt_ctc_lm_table_search_plan;
    host arithmetic only), ``None`` for sizes it does not take."""
    plan = (ctypes.c_int32 * 6)()
    if _cabi.lib().pdt_ctc_lm_table_search_plan(n_frames, V, width, plan) != _cabi.PDT_OK:
        return None
    return tuple(plan)


def _factor_table(lm: "LookupLanguageModel", beta: float, valid_mixture: bool, device: torch.device):
    """``(factors (rows, V), row maxima (rows,), sos_row, U)``: the model's factor of CTCPrefixSearch's mix for
    every context (include/pdt_amd.h: pdt_lm_factor_table), built once per model, mix and device and kept
    while the model's buffers are unchanged (_cached_table).  The factors overwrite the scores they are
    formed from (a trigram model's table is gigabytes)."""

    def build():
        factors, sos_row, U = _context_scores(lm, device)
        rows, V = factors.shape
        with torch.cuda.device(device):
            rc = _cabi.lib().pdt_lm_factor_table(
                _cabi.ptr(factors), rows, V, float(beta), int(valid_mixture), _cabi.ptr(factors), factors.stride(0),
                _cabi.stream_ptr(device),
            )
        _cabi.check(rc, "pdt_lm_factor_table")
        return factors, factors.max(1)[0].contiguous(), sos_row, U

    return _cached_table(_FACTOR_TABLES, lm, device, build, float(beta), bool(valid_mixture))


class BeamSearch(torch.nn.Module):
    """Beam search driven by an :class:`ExtractableSequentialLanguageModel` (reference
    _decoding.py:158-504).  Each iteration is the user's LM forward, a ``log_softmax``, the
    overridable :meth:`update_log_probs_for_step` hook and ONE ``beam_search_advance`` kernel.
    """

    __constants__ = ["width", "eos", "finish_all_paths", "pad_value"]
    # iterations between host reads of the termination count in the fused loop (None: 8 for this
    # package's LookupLanguageModel, 1 -- the reference's behaviour -- for any other model)
    host_check_interval: Optional[int] = None

    def __init__(
        self,
        lm: ExtractableSequentialLanguageModel,
        width: int,
        eos: Optional[int] = None,
        finish_all_paths: bool = False,
        pad_value: int = config.INDEX_PAD_VALUE,
    ):
        width = argcheck.is_posi(width, "width")
        eos = argcheck.is_int(eos, "eos", True)
        finish_all_paths = argcheck.is_bool(finish_all_paths, "finish_all_paths")
        pad_value = argcheck.is_int(pad_value, "pad_value")
        super().__init__()
        if eos is not None:
            if eos < -lm.vocab_size or eos > lm.vocab_size - 1:
                raise ValueError(
                    "Expected eos to be in the range [{}, {}], got {}".format(
                        -lm.vocab_size, lm.vocab_size - 1, eos
                    )
                )
            eos = (eos + lm.vocab_size) % lm.vocab_size
        self.lm, self.width, self.eos = lm, width, eos
        self.finish_all_paths, self.pad_value = finish_all_paths, pad_value
        try:
            device = next(iter(lm.parameters())).device
        except StopIteration:
            device = torch.device("cpu")
        self.register_buffer("device_buffer", torch.empty(0, device=device))

    def reset_parameters(self) -> None:
        if hasattr(self.lm, "reset_parameters"):
            self.lm.reset_parameters()

    def extra_repr(self) -> str:
        return ", ".join("{}={}".format(x, getattr(self, x)) for x in self.__constants__)

    def update_log_probs_for_step(
        self,
        log_probs_prev: torch.Tensor,
        log_probs_t: torch.Tensor,
        y_prev: torch.Tensor,
        y_prev_lens: torch.Tensor,
        eos_mask: torch.Tensor,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Hook: subclasses may rescore paths ``(N, K)`` and extensions ``(N, K, V)`` at every
        step (reference _decoding.py:306-350).  The default is the identity."""
        return log_probs_prev, log_probs_t

    def _to_width(self, y, log_probs, lens):
        # reference _decoding.py:352-372
        S, N, Kp = y.shape
        if Kp < self.width:
            rem = self.width - Kp
            log_probs = torch.cat([log_probs, log_probs.new_full((N, rem), -float("inf"))], 1)
            y = torch.cat([y, y.new_zeros(S, N, rem)], 2)
            lens = torch.cat([lens, lens.new_zeros(N, rem)], 1)
        elif Kp > self.width:
            log_probs, src = log_probs.topk(self.width, 1)
            y = y.gather(2, src.unsqueeze(0).expand(S, N, self.width))
            lens = lens.gather(1, src)
        return y, log_probs, lens

    @torch.jit.unused
    def _check_growth(self, lens: torch.Tensor, hist: torch.Tensor) -> None:
        if switches.get("PDT_CHECK_INVARIANTS") == 1 and lens.numel():
            if int(lens.max()) < hist.size(0):
                raise RuntimeError("BeamSearch: no path is as long as the history ({} < {}): the step must not "
                                   "grow y".format(int(lens.max()), hist.size(0)))

    @torch.jit.unused
    def _bigram_table(self, device: torch.device):
        """``(table (U, V), stats (U, 2), sos_row, U)`` of a bigram :class:`LookupLanguageModel` whose dense
        table stays within 64 MiB (_dense_table), else ``None``: row ``c`` holds the model's scores after
        context token ``c``, ``stats`` every row's maximum and log-sum-exp.  An iteration of the search then
        reads its prefixes' rows straight from the table (``pdt_beam_search_step_table``) instead of having
        the model write ``(N K, V)`` scores first.  (PDT_BEAM_TABLE=0 or ``del _BIGRAM_TABLES[lm]`` after a
        write the buffers' version counters do not see.)"""
        lm = self.lm
        if type(lm) is not LookupLanguageModel or lm.max_ngram != 2 or not switches.get("PDT_BEAM_TABLE"):
            return None
        return _dense_table(lm, device)

    @torch.jit.unused
    def _table_search(self, dense, N: int, max_iters: int, squeeze: bool):
        """``pdt_beam_search_table`` + ``pdt_beam_search_table_paths``: the whole search in one launch, the
        paths written once at the end (one host read in between: the number of rows ``y`` has).  ``None``
        when the kernel does not take the shape."""
        table, stats, sos_row, _ = dense
        device, W, V = table.device, self.width, self.lm.vocab_size
        L = _cabi.lib()
        with _cabi.on_device(device):
            trie = torch.empty((N, max_iters, W), dtype=torch.int32, device=device)
            lp = torch.empty((N, W), device=device)
            lens = torch.empty((N, W), dtype=torch.long, device=device)
            finish = torch.empty((N,), dtype=torch.int32, device=device)
            t_stop = torch.zeros((1,), dtype=torch.int32, device=device)
            stream = _cabi.stream_ptr(device)
            rc = L.pdt_beam_search_table(
                _cabi.ptr(table), table.stride(0), table.stride(1), table.size(0), _cabi.ptr(stats), int(sos_row),
                N, V, W, max_iters, int(self.eos is not None), int(self.eos or 0), int(self.finish_all_paths),
                _cabi.ptr(trie), _cabi.ptr(lp), _cabi.ptr(lens), _cabi.ptr(finish), _cabi.ptr(t_stop), stream,
            )  # fmt: skip
            if rc == _cabi.PDT_E_UNSUPPORTED:
                return None
            _cabi.check(rc, "pdt_beam_search_table")
            T = int(t_stop.item())  # the reference leaves its loop at the iteration that finds every element finished
            y = torch.empty((T, N, W), dtype=torch.long, device=device)
            rc = L.pdt_beam_search_table_paths(
                _cabi.ptr(trie), _cabi.ptr(finish), N, max_iters, W, T, int(self.pad_value), _cabi.ptr(y), stream
            )
            _cabi.check(rc, "pdt_beam_search_table_paths")
        if squeeze:
            y, lens, lp = y.squeeze(1), lens.squeeze(0), lp.squeeze(0)
        return y, lens, lp

    @torch.jit.unused
    def _forward_fused(
        self, prev: Dict[str, torch.Tensor], batch_size: Optional[int], max_iters: int
    ) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """The search with every iteration's bookkeeping in ONE kernel (csrc/beam_step.hip) around the
        language model's forward: no ``log_softmax`` / ``masked_fill`` / ``where`` passes over
        ``(N, K, V)``, no per-iteration clamp of the history, and the number of unfinished batch
        elements is read from the device every eighth iteration instead of every one (iterations run
        past the end only append padding, which is cut off again).  Taken when the step hook is the
        default one (a subclass that overrides ``update_log_probs_for_step`` must see the tensors),
        nothing wants gradients and the beam fits a wave; returns ``None`` otherwise."""
        if type(self).update_log_probs_for_step is not BeamSearch.update_log_probs_for_step:
            return None
        if self.width > 64 or not switches.get("PDT_BEAM_FUSED"):
            return None
        if torch.is_grad_enabled() and (
            any(p.requires_grad for p in self.lm.parameters())
            or any(torch.is_tensor(v) and v.requires_grad for v in prev.values())
        ):
            return None
        device = self.device_buffer.device
        if device.type != "cuda":
            return None
        N = 1 if batch_size is None else batch_size
        V, W = self.lm.vocab_size, self.width
        L = _cabi.lib()
        has_eos = self.eos is not None
        y = torch.empty((0, N), dtype=torch.long, device=device)
        prev = self.lm.update_input(prev, y)
        y = y.unsqueeze(2)
        log_probs = torch.zeros((N, 1), device=device)
        lens = torch.zeros((N, 1), dtype=torch.long, device=device)
        # Iterations between host reads of the "everything finished" count.  Between reads the search may
        # call the language model up to `check_every - 1` times past the reference's stopping point (their
        # output is cut off again) -- invisible for a stateless, deterministic model like this package's
        # LookupLanguageModel, but a stochastic or stateful user model would see extra calls: those are
        # checked every iteration unless the caller says otherwise through `host_check_interval`.  Even
        # then the count of iteration i is read AFTER the model's call of iteration i has been issued, so
        # such a model sees AT MOST ONE call more than under the reference, which breaks before calling
        # it (_decoding.py:426); the call's output is discarded.
        check_every = self.host_check_interval
        if check_every is None:
            check_every = 8 if type(self.lm) is LookupLanguageModel else 1
        check_every = max(1, min(int(check_every), 1024))
        counts = torch.zeros((check_every,), dtype=torch.int32, device=device)
        pad_from = torch.full((N,), 2147483647, dtype=torch.int32, device=device)
        steps = torch.arange(0, 1024, device=device)
        row_base = {1: torch.zeros((N, 1), dtype=torch.long, device=device),
                    W: torch.arange(0, W * N, W, device=device).unsqueeze(1)}
        Kp, t, t_stop = 1, 0, -1
        out_dtype = torch.float
        dense = self._bigram_table(device)
        if (dense is not None and 0 < max_iters <= 4096 and N > 0 and 4 * N * max_iters * W <= (1 << 30)
                and switches.get("PDT_BEAM_SEARCH")):  # (the trie: a word per beam entry and iteration, 1 GiB at most)
            # a bigram table model, a bounded search: every iteration in ONE launch, no history copies
            done = self._table_search(dense, N, max_iters, batch_size is None)
            if done is not None:
                return done
        # (what does not change from one iteration to the next, once)
        eos_args = (int(has_eos), int(self.eos or 0), int(self.finish_all_paths), int(self.pad_value))
        counts_ptr, pad_from_ptr, stream = counts.data_ptr(), pad_from.data_ptr(), _cabi.stream_ptr(device)
        if dense is not None:
            table, stats, sos_row, _ = dense
            table_args = (table.data_ptr(), table.stride(0), table.stride(1), table.size(0), stats.data_ptr())
            first_rows = torch.full((N, 1), sos_row, dtype=torch.long, device=device)
        while t < max_iters:
            if dense is None:  # the model's scores of every prefix
                if t and t % 1024 == 0:
                    steps = torch.arange(t, t + 1024, device=device)
                scores, state_next = self.lm.calc_idx_log_probs(y.flatten(1), prev, steps[t % 1024])
                if torch.is_grad_enabled() and scores.requires_grad:
                    if t == 0:  # (a model whose weights are no registered parameters: the differentiable loop)
                        return None
                    raise RuntimeError("BeamSearch: the language model's output wants gradients inside a search "
                                       "that was started without any (set PDT_BEAM_FUSED=0)")
                out_dtype = scores.dtype
                scores = _f32(scores).reshape(N, Kp, V)
            with _cabi.on_device(device):
                y_new = torch.empty((t + 1, N, W), dtype=torch.long, device=device)
                lens_new = torch.empty((N, W), dtype=torch.long, device=device)
                lp_new = torch.empty((N, W), device=device)
                src = torch.empty((N, W), dtype=torch.long, device=device)
                state_args = (
                    log_probs.data_ptr(), log_probs.stride(0), log_probs.stride(1),
                    y.data_ptr(), t, y.stride(0), y.stride(1), y.stride(2),
                    lens.data_ptr(), lens.stride(0), lens.stride(1), *eos_args,
                    y_new.data_ptr(), lens_new.data_ptr(), lp_new.data_ptr(), src.data_ptr(),
                    counts_ptr + 4 * (t % check_every), pad_from_ptr, stream,
                )  # fmt: skip
                if dense is not None:  # a bigram table model: the prefixes' rows of its table, by their last tokens
                    rows = first_rows if t == 0 else y[t - 1]
                    rc = L.pdt_beam_search_step_table(*table_args, rows.data_ptr(), N, Kp, V, W, *state_args)
                else:
                    rc = L.pdt_beam_search_step(
                        scores.data_ptr(), scores.stride(0), scores.stride(1), scores.stride(2), N, Kp, V, W, *state_args
                    )
            if rc:
                _cabi.check(rc, "pdt_beam_search_step" if dense is None else "pdt_beam_search_step_table")
            if dense is None:
                prev = self.lm.extract_by_src(state_next, (src + row_base[Kp]).flatten())
            y, lens, log_probs, Kp = y_new, lens_new, lp_new, W
            t += 1
            if has_eos and (t % check_every == 0 or t == max_iters):
                # the one host read per `check_every` iterations: an iteration that started with every
                # batch element finished is where the reference leaves its loop (:426)
                seen = counts.tolist()
                lo = t - ((t - 1) % check_every + 1)
                for i in range(lo, t):
                    if i > 0 and seen[i % check_every] == 0:
                        t_stop = i
                        break
                if t_stop >= 0:
                    break
                counts.zero_()
        if t_stop >= 0:  # the iterations from t_stop on only appended padding
            y = y[:t_stop]
        if has_eos and y.size(0):  # finished elements: pad_value from their first padding row on
            rows = torch.arange(y.size(0), device=device).view(-1, 1, 1)
            y = torch.where(rows >= pad_from.view(1, N, 1), y.new_full((), self.pad_value), y)
        y, log_probs, lens = self._to_width(y, log_probs.to(out_dtype), lens)
        if batch_size is None:
            y, lens, log_probs = y.squeeze(1), lens.squeeze(0), log_probs.squeeze(0)
        return y, lens, log_probs

    def forward(
        self,
        initial_state_: Optional[Dict[str, torch.Tensor]] = None,
        batch_size: Optional[int] = None,
        max_iters: Optional[int] = None,
        initial_state: Optional[Dict[str, torch.Tensor]] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        # (``initial_state_`` is the reference's runtime keyword, _decoding.py:383-386;
        # ``initial_state`` the name of its documented call signature -- both are accepted)
        if initial_state is None:
            initial_state = initial_state_
        prev = dict() if initial_state is None else initial_state
        device = self.device_buffer.device
        N = 1 if batch_size is None else batch_size
        V, W = self.lm.vocab_size, self.width
        if max_iters is None:
            if self.eos is None:
                raise RuntimeError("max_iters must be set when eos is unset")
            max_iters = 1073741824
        elif max_iters < 0:
            raise RuntimeError("max_iters must be non-negative, got {}".format(max_iters))
        if not torch.jit.is_scripting():
            fused = self._forward_fused(prev, batch_size, max_iters)
            if fused is not None:
                return fused
        Kp = 1
        y = torch.empty((0, N), dtype=torch.long, device=device)
        prev = self.lm.update_input(prev, y)
        y = y.unsqueeze(2)
        log_probs = torch.full((N, Kp), -math.log(Kp), device=device)
        lens = torch.zeros((N, Kp), dtype=torch.long, device=device)
        pad_row = torch.full((1, N, W), self.pad_value, device=device, dtype=torch.long)
        track_eos = self.eos is not None
        for t in range(max_iters):
            step = torch.tensor(t, device=device)
            ended = torch.zeros((N, Kp), device=device, dtype=torch.bool)
            frozen = ended[:, :1]  # batch elements whose search is over (:413-427)
            any_frozen = False
            if track_eos and t:
                tail = y.permute(1, 2, 0).gather(2, (lens - 1).clamp(min=0).unsqueeze(2)).squeeze(2)
                ended = (tail == self.eos) & (lens > 0)
                frozen = ended.all(1, keepdim=True) if self.finish_all_paths else ended[:, :1]
                # the one host read of the step: (everything is over, something is over)
                code = int((frozen.all().long() * 2 + frozen.any().long()).item())
                any_frozen = code > 0
                if code > 1:
                    break
            hist = y.clamp(0, V - 1)
            lp_t, state_next = self.lm.calc_idx_log_probs(hist.flatten(1), prev, step)
            lp_t = lp_t.reshape(N, Kp, V).log_softmax(-1)
            log_probs, lp_t = self.update_log_probs_for_step(log_probs, lp_t, hist, lens, ended)
            if track_eos:  # a path that has ended repeats eos at no cost and emits nothing else (:448-458)
                only_eos = torch.full_like(lp_t, -float("inf"))
                only_eos[..., self.eos] = 0.0
                lp_t = torch.where(ended.unsqueeze(2), only_eos, lp_t)
            # some path is as long as the history whenever the loop gets here (a live element has
            # a live path of t tokens), so y grows by a row: no read-back of the lengths
            # (PDT_CHECK_INVARIANTS=1 reads them back and checks)
            if not torch.jit.is_scripting():
                self._check_growth(lens, hist)
            y_new, lens_new, lp_new, src = torch.ops.pydrobert_amd.beam_search_advance(
                lp_t, W, log_probs, hist, lens, True
            )
            if track_eos:  # ended sources stay as long as they were (:465-468)
                lens_new = lens_new - ended.gather(1, src).to(lens_new)
            rows = (src + torch.arange(0, Kp * N, Kp, device=device).unsqueeze(1)).flatten()
            prev = self.lm.extract_by_src(state_next, rows)
            if any_frozen:  # finished batch elements keep what they had (:479-486)
                y, log_probs, lens = self._to_width(y, log_probs, lens)
                grown = torch.cat([y, pad_row.expand(y_new.size(0) - y.size(0), -1, -1)], 0)
                y_new = torch.where(frozen.unsqueeze(0), grown, y_new)
                lp_new = torch.where(frozen, log_probs, lp_new)
                lens_new = torch.where(frozen, lens, lens_new)
            y, lens, log_probs, Kp = y_new, lens_new, lp_new, W
        y, log_probs, lens = self._to_width(y, log_probs, lens)
        if batch_size is None:
            y, lens, log_probs = y.squeeze(1), lens.squeeze(0), log_probs.squeeze(0)
        return y, lens, log_probs
