/*
 * pdt_amd.h -- C ABI of libpdt_amd.so: MI355X (gfx950) kernels for the sequence-level
 * hot path of pydrobert-pytorch.
 *
 * The reference (sdrobert/pydrobert-pytorch) is pure Python on stock ATen ops and has
 * no FFI of its own; its boundary for this path is the Python functional API
 * (src/pydrobert/torch/functional.py:24-58).  Each entry point below is what a binding
 * for one of those functions calls; the citation names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers that the
 *     library borrows for the duration of the call (never frees, never retains);
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, never synchronised;
 *   - strides are in ELEMENTS: token (t, n) of a sequence tensor is tok[t*st + n*sn], so
 *     batch_first inputs/outputs are expressed by swapping strides, not by copies;
 *   - return value: 0 ok, <0 invalid argument (PDT_E_*), >0 a hipError_t;
 *   - `status` (optional, device int32) is OR-ed with PDT_WARN_* data-irregularity bits
 *     (the reference raises warnings.warn for them when warn=True).
 */
#ifndef PDT_AMD_H
#define PDT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDT_OK 0
#define PDT_E_ARG -1      /* malformed argument (null pointer, negative size, bad mode) */
#define PDT_E_TOO_LONG -2 /* a sequence dimension exceeds what the kernel supports */
#define PDT_E_UNSUPPORTED -3 /* this entry point has no kernel for the layout given; the general entry point has */

#define PDT_MODE_FINAL 0
#define PDT_MODE_PREFIX 1

#define PDT_WARN_REF_NO_EOS 1 /* _string.py:201-207 */
#define PDT_WARN_HYP_NO_EOS 2 /* _string.py:211-217 */
#define PDT_WARN_EMPTY_REF 4  /* _string.py:361-367, :398-404 */

/* Library / build identification. */
int pdt_amd_abi_version(void);

/* Run-time switches (kernel selection for comparisons; INTEGRATION.md "Switches").  Each is
 * initialised ONCE from the environment variable of the same name the first time the library
 * needs one -- nothing on a launch path calls getenv -- and can be changed / read afterwards.
 * Unknown names return PDT_E_ARG.  No counterpart in the reference (it has one route per operator). */
int pdt_amd_set_switch(const char *name, int value);
int pdt_amd_get_switch(const char *name, int *value);

/* ---------------------------------------------------------------------------------------
 * Batched Levenshtein: error_rate, edit_distance, prefix_error_rates,
 * prefix_edit_distances.  Replaces _string_matching (_string.py:146-406) for
 * return_mask=False, including _lens_from_eos (_string.py:137-143), the include_eos
 * fix-ups (:195-218), the uniform-cost shortcut (:168-174), normalisation and padding
 * (:356-405).
 *
 *   ref (R, N), hyp (H, N) int64 tokens addressed through element strides.
 *   mode FINAL : out[n * out_sn]                          (N,)      float32
 *   mode PREFIX: out[h * out_sh + n * out_sn], h < Hout   (Hout, N) float32,
 *                Hout = H + (exclude_last ? 0 : 1)
 *   return_mistakes: 1 = error-count semantics (error_rate / prefix_error_rates),
 *                    0 = cost semantics (edit_distance / prefix_edit_distances).
 *   ref_lens_out / hyp_lens_out (optional, (N,) int64) receive the sequence lengths.
 *   workspace (optional): pdt_lev_workspace_bytes(R, H, N) bytes of device memory, 256-byte
 *   aligned, contents irrelevant.  With it, unit (i.e. uniform) costs run on the bit-parallel
 *   kernels of lev_bitpar.hip; without it (NULL / too small), or when that function returns 0
 *   (a hypothesis longer than 1024 tokens), on the cell-by-cell kernels.  Same results.
 *   Cost semantics with costs that are NOT exact in float32 and R > 2048 need the workspace (the
 *   plain workgroup kernel of lev_generic.hip keeps its rows there): PDT_E_TOO_LONG without it.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_lev_workspace_bytes(int64_t R, int64_t H, int64_t N);

int pdt_lev(const int64_t *ref, int64_t R, int64_t ref_st, int64_t ref_sn,
            const int64_t *hyp, int64_t H, int64_t hyp_st, int64_t hyp_sn, int64_t N,
            int has_eos, int64_t eos, int include_eos, float ins_cost, float del_cost,
            float sub_cost, int norm, int mode, int exclude_last, float padding,
            int return_mistakes, float *out, int64_t out_sh, int64_t out_sn,
            int64_t *ref_lens_out, int64_t *hyp_lens_out, int32_t *status, void *workspace,
            int64_t workspace_bytes, void *stream);

/* pdt_lev that also LEAVES its classification -- lengths, token classes, match tables -- in
 * `workspace` for a following pdt_lev_classified.  (pdt_lev itself builds them inside its recurrence
 * kernel where the shape allows and leaves nothing behind; this call always takes the two launches,
 * classification then recurrence.)  Same results, same warning bits. */
int pdt_lev_keep(const int64_t *ref, int64_t R, int64_t ref_st, int64_t ref_sn,
                 const int64_t *hyp, int64_t H, int64_t hyp_st, int64_t hyp_sn, int64_t N,
                 int has_eos, int64_t eos, int include_eos, float ins_cost, float del_cost,
                 float sub_cost, int norm, int mode, int exclude_last, float padding,
                 int return_mistakes, float *out, int64_t out_sh, int64_t out_sn,
                 int64_t *ref_lens_out, int64_t *hyp_lens_out, int32_t *status, void *workspace,
                 int64_t workspace_bytes, void *stream);

/* The same call for inputs a previous pdt_lev_keep has already classified into `workspace` (a
 * workspace that no such call filled -- e.g. one that only a pdt_lev saw -- is recognised on the
 * host and the call then classifies for itself, as pdt_lev does; that is a guard against the
 * never-filled case only, keyed by the workspace's address, not a check that its tables are still
 * valid -- what follows stays the caller's promise): same ref /
 * hyp contents, shapes and strides, same eos / include_eos, same workspace bytes untouched since,
 * issued on the same stream (or ordered after it).  On the bit-parallel path (unit costs) the
 * lengths, token classes and match tables are then read from the workspace instead of being rebuilt
 * -- half the work of a call; error_rate followed by prefix_error_rates on one (ref, hyp) pair is
 * the case (the Python host keeps the last workspace for exactly that, _string.py).  The warning
 * bits are those the classifying call reported; `status` is not written.  Everywhere else it is
 * pdt_lev. */
int pdt_lev_classified(const int64_t *ref, int64_t R, int64_t ref_st, int64_t ref_sn,
                       const int64_t *hyp, int64_t H, int64_t hyp_st, int64_t hyp_sn, int64_t N,
                       int has_eos, int64_t eos, int include_eos, float ins_cost, float del_cost,
                       float sub_cost, int norm, int mode, int exclude_last, float padding,
                       int return_mistakes, float *out, int64_t out_sh, int64_t out_sn,
                       int64_t *ref_lens_out, int64_t *hyp_lens_out, int32_t *status, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * fill_after_eos (_string.py:30-42): out = value, except that every position strictly after
 * the first `eos` along the sequence dimension holds the fill value.
 *   tokens int64, value / out of elem_bytes (1, 2, 4 or 8) per element, all contiguous and
 *   viewed as (outer, L, inner) around the sequence dimension; fill_bits = the fill value's bit
 *   pattern in the low elem_bytes bytes.
 * ------------------------------------------------------------------------------------- */
int pdt_fill_after_eos(const int64_t *tokens, int64_t outer, int64_t L, int64_t inner,
                       int64_t eos, const void *value, int64_t elem_bytes, int64_t fill_bits,
                       void *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Optimal completion, two phases (optimal_completion, _string.py:464-517; the DP is
 * _string_matching with return_mask=True, :271-278, :319-355).
 *
 * Phase 1, pdt_oc_mask: per utterance, ranks the distinct reference tokens
 * (class k = k-th smallest distinct token of ref[:ref_len]), runs the DP and for each
 * hypothesis prefix h records WHICH classes are optimal next tokens as a bitmask:
 *     bitmask[(h * N + n) * W + w], W = pdt_oc_mask_words(R) 32-bit words, bit k of the
 *     row set iff class k is in the completion set of prefix h.
 *     class_tokens[n * R + k] = token value of class k            (N, R) int64
 *     max_count (device int32, must be zeroed by the caller) = max set size = the
 *     reference's `C = counts.max().item()` (:511).
 *     workspace: pdt_oc_mask_workspace_bytes(R, H, N) bytes.  R <= 512: the tables of the bit-parallel
 *     kernel (uniform costs; a caller that passes no workspace, or other costs, gets the same masks
 *     from the row-synchronous kernel, whose DP row lives in registers); 512 < R <= 2048: 0; longer
 *     references run a plain one-workgroup-per-utterance form whose rows, sort buffer and class ids
 *     live there (costs that are not exact in float32 replay the reference's unrolled deletion term
 *     by term there as well, O(R^2) per row).
 * Phase 2, pdt_oc_expand (after the caller has read max_count and allocated targets):
 *     targets[h * tgt_sh + n * tgt_sn + i], i < C, ascending tokens then `padding`.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_oc_mask_words(int64_t R);
int64_t pdt_oc_mask_workspace_bytes(int64_t R, int64_t H, int64_t N);

int pdt_oc_mask(const int64_t *ref, int64_t R, int64_t ref_st, int64_t ref_sn,
                const int64_t *hyp, int64_t H, int64_t hyp_st, int64_t hyp_sn, int64_t N,
                int has_eos, int64_t eos, int include_eos, float ins_cost, float del_cost,
                float sub_cost, int exclude_last, uint32_t *bitmask,
                int64_t *class_tokens, int32_t *max_count, int32_t *status, void *workspace,
                int64_t workspace_bytes, void *stream);

int pdt_oc_expand(const uint32_t *bitmask, const int64_t *class_tokens, int64_t R,
                  int64_t Hout, int64_t N, int64_t C, int64_t padding, int64_t *targets,
                  int64_t tgt_sh, int64_t tgt_sn, void *stream);

/* ---------------------------------------------------------------------------------------
 * Hard optimal-completion distillation loss, fused (hard_optimal_completion_distillation_loss,
 * _string.py:1188-1251).  Consumes pdt_oc_mask's outputs directly (exclude_last = 1, so the
 * bitmask has H rows) instead of the expanded (H, N, C) targets:
 *   loss[h*N + n]  = mean over the completion set S of  -weight[t] * log_softmax(logits[h,n])[t]
 *   count[h*N + n] = |S| (targets equal to ignore_index are skipped), loss uses max(count, 1).
 * logits (H, N, V) float32 (float16 / bfloat16: the _elem entry points below) through element strides;
 * weight (V,) or NULL.
 * Backward: grad_logits (H, N, V) contiguous from grad_loss (H, N).
 * status (optional) bit 0 is set when a target lies outside [0, V).
 * PDT_E_TOO_LONG: V >= 2^30, H, N or R above 2^31 - 1 (ints in the kernel), H * N >= 2^33.
 * ------------------------------------------------------------------------------------- */
int pdt_ocd_loss_forward(const float *logits, int64_t H, int64_t N, int64_t V, int64_t lg_sh,
                         int64_t lg_sn, int64_t lg_sv, const uint32_t *bitmask,
                         const int64_t *class_tokens, int64_t R, const float *weight,
                         int64_t ignore_index, float *loss, int32_t *count, int32_t *status,
                         void *stream);

int pdt_ocd_loss_backward(const float *logits, int64_t H, int64_t N, int64_t V, int64_t lg_sh,
                          int64_t lg_sn, int64_t lg_sv, const uint32_t *bitmask,
                          const int64_t *class_tokens, int64_t R, const float *weight,
                          int64_t ignore_index, const float *grad_loss, float *grad_logits,
                          void *stream);

/* The same with logits -- and, in the backward, grad_logits -- of the element type `elem` (0 float32,
 * 2 float16, 3 bfloat16; 1 returns PDT_E_UNSUPPORTED, any other value PDT_E_ARG: see
 * pdt_ctc_prefix_search_elem), read and written as they are, without a float32 copy.  loss has the bits the
 * float32 entry point gives on the widened logits, grad_logits those of its gradient rounded to the element
 * type (nearest even).  weight, grad_loss, loss and count stay float32 / int32; rows need no alignment
 * beyond the element's.  The element code and the pointers are checked before any device work. */
int pdt_ocd_loss_forward_elem(const void *logits, int64_t H, int64_t N, int64_t V, int64_t lg_sh,
                              int64_t lg_sn, int64_t lg_sv, const uint32_t *bitmask,
                              const int64_t *class_tokens, int64_t R, const float *weight,
                              int64_t ignore_index, float *loss, int32_t *count, int32_t *status,
                              void *stream, int elem);

int pdt_ocd_loss_backward_elem(const void *logits, int64_t H, int64_t N, int64_t V, int64_t lg_sh,
                               int64_t lg_sn, int64_t lg_sv, const uint32_t *bitmask,
                               const int64_t *class_tokens, int64_t R, const float *weight,
                               int64_t ignore_index, const float *grad_loss, void *grad_logits,
                               void *stream, int elem);

/* ---------------------------------------------------------------------------------------
 * CTC prefix beam search with an N-GRAM language model in the loop, every frame from one launch
 * (reference _decoding.py:1064-1202 with shallow fusion / valid mixture, :1113-1135, around a
 * LookupLanguageModel, _lm.py:403-515, whose contexts -- U^(order - 1) of them -- fit a table).
 *
 *   pdt_lm_factor_table: the model's factor of the mix for every context token, from its scores
 *     lm_log_probs (rows, V) contiguous (row c = the model's scores after context token c):
 *     out[c][v] = exp(beta * log_softmax(lm_log_probs[c])[v])   (valid_mixture = 0; ext = p * out)
 *              or softmax(lm_log_probs[c])[v]                    (valid_mixture = 1;
 *                 ext = (1 - beta) * p + beta * (out * (1 - p_blank))) -- pdt_fusion_ext's expressions.
 *     Built once per model and mix by the host; rows out_stride floats apart.
 *   pdt_ctc_lm_table_search: logits / lens / width / S / y / y_lens / y_probs as
 *     pdt_ctc_prefix_search (the softmax of :1093 is fused); factors (contexts, V) the table above,
 *     factor_max (contexts,) the largest value of every row (it bounds a prefix's extension masses:
 *     lists are built only for prefixes whose extensions can be among a frame's winners);
 *     sos_row the row of the empty prefix's context.  A prefix's row is its last (order - 1) tokens read as
 *     digits in base ctx_base, start-of-sequence padding in front: an extension by token v moves row r to
 *     (r mod ctx_mod) * ctx_base + v, with ctx_mod = ctx_base^(order - 2) and contexts = ctx_base * ctx_mod
 *     (a bigram model: ctx_mod = 1, the row is the last token; a trigram model over U context symbols:
 *     ctx_base = ctx_mod = U, U^2 rows -- 4 GB at U = 1001, V = 1000: sized for this card's HBM, built once
 *     per model by the model's own scoring kernel over every context).
 *     width <= 32, V <= 5119.  workspace: pdt_ctc_lm_table_search_workspace_bytes (trie + checkpoints),
 *     0 for sizes the search does not take.
 *   pdt_ctc_lm_table_search_plan (host only, no device work): what the launch decides from the sizes --
 *     plan6 = {checkpoint shift, checkpoints per utterance, 64-token chunks per row of the kernel instance
 *     (8 / 16 / 32 / 48 / 80), 16 for the instance with the width as a constant else 0, bytes of the row
 *     ring, LDS bytes per workgroup}.  Returns PDT_OK or the code pdt_ctc_lm_table_search returns for
 *     (T, V, width).  Checkpoints lie 2^shift frames apart: the shift is the smallest >= 5 at which the
 *     (T / 2^shift + 1) x width table of the output walk fits the row ring.
 * ------------------------------------------------------------------------------------- */
int pdt_lm_factor_table(const float *lm_log_probs, int64_t rows, int64_t V, float beta, int valid_mixture,
                        float *out, int64_t out_stride, void *stream);
int64_t pdt_ctc_lm_table_search_workspace_bytes(int64_t T, int64_t N, int64_t V, int64_t width);
int pdt_ctc_lm_table_search_plan(int64_t T, int64_t V, int64_t width, int32_t *plan6);
int pdt_ctc_lm_table_search(const float *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st, int64_t lg_sn,
                            int64_t lg_sv, const int64_t *lens, int64_t width, int64_t S, const float *factors,
                            const float *factor_max, int64_t contexts, int64_t f_stride, int64_t sos_row,
                            int64_t ctx_base, int64_t ctx_mod, float beta, int valid_mixture,
                            int64_t *y, int64_t *y_lens, float *y_probs, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * CTC prefix beam search without a language model: CTCPrefixSearch(width)(logits, lens)
 * (reference _decoding.py:1064-1202; the per-frame step is ctc_prefix_search_advance,
 * :636-934; the softmax of :1093 is fused).
 *
 *   logits (T, N, V + 1) float32 (float16 / bfloat16: the _elem entry point below) through element
 *          strides, blank = index V.
 *   lens   (N,) int64 or NULL (all T).  S = number of rows of y = max(lens) (T if NULL).
 *   y      (S, N, width) int64 contiguous; every element is written (rows beyond a prefix's
 *          length are 0; the reference leaves them undefined);
 *   y_lens (N, width) int64, y_probs (N, width) float32 (probabilities, not logs).
 *   workspace: pdt_ctc_prefix_search_workspace_bytes(T, N, V, width) bytes of scratch
 *          (the prefix trie: one (parent, token) record per frame and beam entry, the
 *          checkpoints of the output walk and, for rows beyond the LDS, the rows of the ring).
 *   width <= 32 (wider beams, up to 128 prefixes: pdt_ctc_prefix_search_wide below).  S must be at least min(T, max lens): frames beyond S are not decoded.
 *   Rows of up to 511 tokens and of 512 .. 16 447 tokens (contiguous logits) are held in the
 *   registers of the producer wave that reads them (ctc_search.hip / ctc_rowreg.hip); other rows
 *   of up to about 10 000 tokens live in LDS (one row of probabilities per slot of a three-slot
 *   ring); longer ones stay in the workspace (L2-resident), any V below 2^30.
 * pdt_ctc_prefix_search_plan (host only, no device work): the launch configuration the library
 *   picks for rows of V tokens and this width -- plan5 = {producer waves per utterance, ring
 *   slots, utterances per workgroup, where a row is held: 1 the producer's registers (short
 *   rows), 3 the same for long rows (the ring then carries lists, not rows), 0 LDS, 2 the
 *   workspace; for 3: 64-token register chunks of the instantiation, else 0}.  Lets callers and
 *   tests see where the configurations change.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_ctc_prefix_search_workspace_bytes(int64_t T, int64_t N, int64_t V, int64_t width);

int pdt_ctc_prefix_search_plan(int64_t V, int64_t width, int32_t *plan5);

int pdt_ctc_prefix_search(const float *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                          int64_t lg_sn, int64_t lg_sv, const int64_t *lens, int64_t width,
                          int64_t S, int64_t *y, int64_t *y_lens, float *y_probs,
                          void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Logits of float16 / bfloat16 (and float32) without a float32 copy: the _elem entry points.
 * Each takes the arguments of its sibling plus the element type of the logits -- and, in
 * pdt_sequence_log_probs_backward_elem, of grad_logits:
 *   elem  0 float32 (what the sibling forwards with), 2 float16, 3 bfloat16;
 *         1 (float64) returns PDT_E_UNSUPPORTED, any other value PDT_E_ARG.
 * A half element is widened to float32, exactly, where the kernel loads it, and the arithmetic is
 * the float32 kernel's: every output has the bits the sibling gives on the widened tensor.
 * Strides stay element strides, rows need no alignment beyond the element's.  The other tensors,
 * y_probs / max_out / out / grad_out among them, are float32 as before; grad_logits is written in
 * the element type, rounded to nearest even.  Workspace sizes do not depend on the element type.
 * The same shape takes the same kernel form for every element type; with rows held in registers
 * (ctc_rowreg.hip) and width 16, where float32 has instances with the width as a constant, the
 * half types take the any-width instance -- same results: every instance gives the same bits.
 * ------------------------------------------------------------------------------------- */
int pdt_ctc_prefix_search_elem(const void *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                               int64_t lg_sn, int64_t lg_sv, const int64_t *lens, int64_t width,
                               int64_t S, int64_t *y, int64_t *y_lens, float *y_probs,
                               void *workspace, void *stream, int elem);

/* ---------------------------------------------------------------------------------------
 * The same search for beams the kernels above cannot hold: width <= 128, every frame in one launch
 * (csrc/ctc_search_wide.hip: one workgroup of eight waves per utterance, the beam's state in LDS
 * between frames, the workgroup selection of the plain step kernel; workgroups never wait on one
 * another).  Arguments, element types (pdt_ctc_prefix_search_wide_elem), outputs and status codes as
 * pdt_ctc_prefix_search; narrower widths are
 * accepted too and give the same beams (probabilities may differ in the last bits: merged masses
 * are summed in index order here).  A frame with fewer than `width` candidates leaves the rest of
 * the beam absent: probability -inf, length 0, a zero column of y.
 *   workspace: pdt_ctc_prefix_search_wide_workspace_bytes(T, N, V, width) bytes -- the prefix trie,
 *          the next-token tables of widths above 64 (8 width^2 bytes per utterance) and one row of
 *          probabilities per utterance (read by rows of more than about 17 000 tokens, which do not
 *          fit the LDS); 0 for arguments the search does not take.
 *   PDT_E_TOO_LONG: width > 128, width * (V + 1) >= 2^31, and the index limits of
 *          pdt_ctc_prefix_search.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_ctc_prefix_search_wide_workspace_bytes(int64_t T, int64_t N, int64_t V, int64_t width);

int pdt_ctc_prefix_search_wide(const float *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                               int64_t lg_sn, int64_t lg_sv, const int64_t *lens, int64_t width,
                               int64_t S, int64_t *y, int64_t *y_lens, float *y_probs,
                               void *workspace, void *stream);

/* The same with logits of the element type `elem` (see pdt_ctc_prefix_search_elem). */
int pdt_ctc_prefix_search_wide_elem(const void *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                                    int64_t lg_sn, int64_t lg_sv, const int64_t *lens, int64_t width,
                                    int64_t S, int64_t *y, int64_t *y_lens, float *y_probs,
                                    void *workspace, void *stream, int elem);

/* Host only, no device work: the forms the wide search takes for rows of V tokens and this width --
 * plan2 = {1: a frame's row of probabilities in LDS, 0: in the workspace; 1: the next-token tables in
 * LDS, 0: in the workspace}.  PDT_E_TOO_LONG where pdt_ctc_prefix_search_wide returns it for the shape. */
int pdt_ctc_prefix_search_wide_plan(int64_t V, int64_t width, int32_t *plan2);

/* ---------------------------------------------------------------------------------------
 * ctc_prefix_search_advance (reference _decoding.py:636-934): one CTC prefix-search step with
 * per-prefix extension probabilities (shallow fusion) and dense histories.
 * Inputs through element strides (a stride of 0 expresses a broadcast):
 *   ext (N, Kp, V), nonext (N, V), blank (N,) float32 probabilities;
 *   nb_prev, b_prev (N, Kp) float32; y_prev (S, N, Kp) int64; y_prev_last, y_prev_lens
 *   (N, Kp) int64; prev_is_prefix (N, Kp, Kp) bool bytes.
 * Outputs, contiguous: y_next (S + 1, N, width) int64 (entries beyond y_next_lens
 *   unspecified, as in the reference); y_next_last, y_next_lens, next_src (N, width) int64;
 *   nb_next, b_next (N, width) float32; next_is_prefix (N, width, width) and next_is_nonext
 *   (N, width) bool bytes.  Kp or width above 32: the plain workgroup form (csrc/advance_wide.hip),
 *   same results; PDT_E_TOO_LONG once its LDS (about 56 Kp + 32 width bytes + 10 KB) exceeds 160 KB.
 * ------------------------------------------------------------------------------------- */
int pdt_ctc_prefix_search_advance(
    const float *ext, int64_t ext_sn, int64_t ext_sk, int64_t ext_sv, const float *nonext,
    int64_t ne_sn, int64_t ne_sv, const float *blank, int64_t bl_sn, int64_t N, int64_t Kp,
    int64_t V, int64_t width, const float *nb_prev, int64_t nb_sn, int64_t nb_sk,
    const float *b_prev, int64_t b_sn, int64_t b_sk, const int64_t *y_prev, int64_t S,
    int64_t yp_ss, int64_t yp_sn, int64_t yp_sk, const int64_t *y_prev_last, int64_t la_sn,
    int64_t la_sk, const int64_t *y_prev_lens, int64_t le_sn, int64_t le_sk,
    const uint8_t *prev_is_prefix, int64_t ip_sn, int64_t ip_sa, int64_t ip_sb, int64_t *y_next,
    int64_t *y_next_last, int64_t *y_next_lens, float *nb_next, float *b_next,
    uint8_t *next_is_prefix, int64_t *next_src, uint8_t *next_is_nonext, void *stream);

/* ---------------------------------------------------------------------------------------
 * The same step with the extension probabilities formed inside it (reference _decoding.py:1110-1135
 * in front of :636-934): lm_log_probs (N * Kp, V) float32 contiguous -- the language model's scores of
 * the frame, any normalisation -- are mixed with nonext / blank as pdt_fusion_ext mixes them
 * (shallow fusion p * exp(beta * log_softmax(lm)), or the valid mixture), to the bit, and never
 * written: what a call of pdt_fusion_ext followed by pdt_ctc_prefix_search_advance returns, in one
 * kernel.  PDT_E_UNSUPPORTED for V above 1024, Kp or width above 32, or LDS beyond 160 KB: the two
 * calls serve those.
 * ------------------------------------------------------------------------------------- */
int pdt_ctc_prefix_search_advance_lm(
    const float *lm_log_probs, float beta, int valid_mixture, const float *nonext, int64_t ne_sn,
    int64_t ne_sv, const float *blank, int64_t bl_sn, int64_t N, int64_t Kp, int64_t V, int64_t width,
    const float *nb_prev, int64_t nb_sn, int64_t nb_sk, const float *b_prev, int64_t b_sn, int64_t b_sk,
    const int64_t *y_prev, int64_t S, int64_t yp_ss, int64_t yp_sn, int64_t yp_sk,
    const int64_t *y_prev_last, int64_t la_sn, int64_t la_sk, const int64_t *y_prev_lens, int64_t le_sn,
    int64_t le_sk, const uint8_t *prev_is_prefix, int64_t ip_sn, int64_t ip_sa, int64_t ip_sb,
    int64_t *y_next, int64_t *y_next_last, int64_t *y_next_lens, float *nb_next, float *b_next,
    uint8_t *next_is_prefix, int64_t *next_src, uint8_t *next_is_nonext, void *stream);

/* ---------------------------------------------------------------------------------------
 * What a caller of pdt_beam_search_advance must know to choose S_out (reference _decoding.py:133-140):
 * *host_flag (a word in pinned host memory, valid once the stream has been synchronised) = bit 0: some
 * y_prev_lens[n, k] >= S; bit 1: some length is non-zero; bit 2: written (a system-scope release store: a
 * host that zeroed the word before the call may poll for it instead of synchronising).  One small kernel
 * and no device-to-host copy.
 * ------------------------------------------------------------------------------------- */
int pdt_lens_reach(const int64_t *lens, int64_t le_sn, int64_t le_sk, int64_t N, int64_t Kp, int64_t S,
                   int32_t *host_flag, void *stream);

/* ---------------------------------------------------------------------------------------
 * beam_search_advance (reference _decoding.py:41-155): one beam-search step.
 *   log_probs_t (N, Kp, V), log_probs_prev (N, Kp) float32; y_prev (S, N, Kp) int64;
 *   y_prev_lens (N, Kp) int64 or NULL (all S).  S_out = rows of y_next: S + 1 when
 *   y_prev_lens is NULL or some length equals S (the caller decides, :133-135), else S.
 * Outputs, contiguous: y_next (S_out, N, width), y_next_lens / next_src (N, width) int64,
 *   log_probs_next (N, width).  Slots beyond min(width, Kp * V) get -inf / length 0 / source 0.
 *   Kp or width above 64: the plain workgroup form (csrc/advance_wide.hip), same results.
 * ------------------------------------------------------------------------------------- */
int pdt_beam_search_advance(const float *log_probs_t, int64_t lt_sn, int64_t lt_sk, int64_t lt_sv,
                            int64_t N, int64_t Kp, int64_t V, int64_t width,
                            const float *log_probs_prev, int64_t lp_sn, int64_t lp_sk,
                            const int64_t *y_prev, int64_t S, int64_t yp_ss, int64_t yp_sn,
                            int64_t yp_sk, const int64_t *y_prev_lens, int64_t le_sn,
                            int64_t le_sk, int64_t S_out, int64_t *y_next, int64_t *y_next_lens,
                            float *log_probs_next, int64_t *next_src, void *stream);
/* ---------------------------------------------------------------------------------------
 * One iteration of BeamSearch.forward (_decoding.py:410-486 with the default
 * update_log_probs_for_step) as one kernel: eos bookkeeping, log_softmax of the language model's
 * scores (not materialised), eos-mass reallocation of ended paths, beam_search_advance, lengths
 * that do not grow for ended sources, finished batch elements keeping their beam.
 *   scores (N, Kp, V) float32 through element strides: the LM's output, any normalisation;
 *   log_probs_prev (N, Kp); y_prev (S, N, Kp) int64 with every token in [0, V - 1] (the clamped
 *   history the reference hands its LM, :434); y_prev_lens (N, Kp).
 *   has_eos / eos in [0, V); finish_all_paths; pad_value (written clamped, see pad_from).
 *   y_next (S + 1, N, width) int64 contiguous, y_next_lens / next_src (N, width) int64,
 *   log_probs_next (N, width) float32.
 *   active [1] int32: set to 1 if some batch element was NOT finished at the start of this
 *   iteration (the caller zeroes it; reading 0 means the reference would have left its loop before
 *   this iteration -- every later row of y is padding).  A flag, not a count: plain stores.
 *   pad_from (N,) int32, INT32_MAX initially: the first row of y that is padding for a finished
 *   element; the caller writes pad_value into rows >= pad_from[n] at the end.
 *   width, Kp <= 64.
 * ------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------
 * BeamSearch.forward over a bigram table, EVERY iteration in one launch (reference _decoding.py:383-504
 * with the default step hook; the table and its row statistics as for pdt_beam_search_step_table):
 * a workgroup runs its batch element's iterations back to back and stops at the one that finds the
 * element finished.  Starts from one empty path whose table row is sos_row.
 *   trie (N, n_iters, width) uint32: an iteration's (source << 20 | token) per beam entry;
 *   log_probs_out / lens_out (N, width): the final beam; finish (N,) int32: the iteration that found the
 *   element finished (n_iters: none); t_stop [1] int32, zeroed by the caller: max over the elements --
 *   the rows y has (the reference leaves its loop there).
 * pdt_beam_search_table_paths then writes y (T, N, width) int64 from the trie (T = t_stop): row s of a
 * path = the token its ancestor chose in iteration s, pad_value from finish[n] on.
 * PDT_E_UNSUPPORTED for rows of at most 64 tokens, width above 64 or width * ceil(V / 64) above 256: the
 * per-iteration entry points serve those.
 * ------------------------------------------------------------------------------------- */
int pdt_beam_search_table(const float *table, int64_t tb_sr, int64_t tb_sv, int64_t U, const float *row_stats,
                          int64_t sos_row, int64_t N, int64_t V, int64_t width, int64_t n_iters, int has_eos,
                          int64_t eos, int finish_all_paths, uint32_t *trie, float *log_probs_out,
                          int64_t *lens_out, int32_t *finish, int32_t *t_stop, void *stream);
int pdt_beam_search_table_paths(const uint32_t *trie, const int32_t *finish, int64_t N, int64_t n_iters,
                                int64_t width, int64_t T, int64_t pad_value, int64_t *y, void *stream);
/* Host only, no device work: what the launchers decide from the sizes (they call these themselves).
 *   pdt_beam_search_table_plan: the instance of the one-launch search for a (U, V) table with token stride
 *   tb_sv -- 0 a wave owns whole rows (width <= 16 and V <= 1024), 1 chunks numbered across the rows;
 *   PDT_E_UNSUPPORTED where pdt_beam_search_table returns it, PDT_E_ARG for sizes below 1.
 *   pdt_beam_search_step_plan: the kernel of one iteration (pdt_beam_search_step: has_rows = 0;
 *   pdt_beam_search_step_table with row_stats: has_rows = 1; sc_sv the token stride) -- 0 the sorted list
 *   per prefix, with the waves per batch element (the power of two <= min(Kp, 8)) written to *waves when
 *   it is not NULL; 1 one selection over all Kp * V candidates (table rows of more than 64 tokens at stride
 *   1 with Kp * ceil(V / 64) <= 256); PDT_E_ARG / PDT_E_TOO_LONG where the entry points refuse the sizes
 *   (Kp or width above 64).  The run-time switch PDT_STEP_FLAT=0 sends the shapes of form 1 to form 0; the
 *   plan reports the shape's answer with the switch on. */
int pdt_beam_search_table_plan(int64_t U, int64_t V, int64_t width, int64_t tb_sv);
int pdt_beam_search_step_plan(int64_t Kp, int64_t V, int64_t width, int has_rows, int64_t sc_sv,
                              int32_t *waves);

/* ---------------------------------------------------------------------------------------
 * The whole CTCPrefixSearch with a LookupLanguageModel in the loop (_decoding.py:1083-1202 with
 * :1110-1163 per frame; scores: _lm.py:403-515), every frame in one launch, the beam's state kept in
 * `workspace` between the frames.  A frame: the back-off n-gram scores of every prefix's context (its
 * last max_ngram - 1 tokens), shallow fusion (valid_mixture = 0: ext = p_ctc * exp(beta *
 * log_softmax(lm))) or the valid mixture, the per-prefix sorted lists and the prefix step.  The
 * model's buffers are those of pdt_lookup_lm_log_probs (the forward index is required); max_ngram >= 2.
 *   probs (T, N, V + 1) float32 through element strides: softmax of the logits, blank last; frames
 *   0 .. n_frames - 1 are read (n_frames >= 1).  frame_lens (N,) int64 or NULL: a batch element keeps
 *   its beam from frame frame_lens[n] on (:1165-1181).
 *   Histories are not copied from frame to frame: every batch element has 2 * width history slots;
 *   a prefix that survives a frame keeps its slot, an extended prefix gets a free slot, a copy of its
 *   source's tokens and the new token (int16 tokens).
 *   Outputs, contiguous: y (n_frames, N, width) int64, zero beyond an entry's length and for absent
 *   entries; y_lens (N, width) int64; nb, b (N, width) float32 -- the two masses of every entry (the
 *   module returns nb + b).  Same bits as pdt_lookup_lm_log_probs -> pdt_fusion_ext ->
 *   pdt_ctc_prefix_search_advance frame after frame.
 *   workspace: pdt_ctc_lookup_lm_search_workspace_bytes(n_frames, N, V, width, max_ngram, U) bytes.
 * width <= 32; max_ngram <= 16.
 *   pdt_ctc_lookup_lm_search_lds_bytes (host only, no device work): the dynamic LDS of the launch for
 *   (V, width), 0 when the shape does not fit -- pdt_ctc_lookup_lm_search then returns PDT_E_TOO_LONG.
 *   A workgroup holds two rows of V floats at the least, so no V above 20 480 fits at any width.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_ctc_lookup_lm_search_lds_bytes(int64_t V, int64_t width);
int64_t pdt_ctc_lookup_lm_search_workspace_bytes(int64_t n_frames, int64_t N, int64_t V, int64_t width,
                                                 int64_t max_ngram, int64_t U);
int pdt_ctc_lookup_lm_search(
    const float *probs, int64_t p_st, int64_t p_sn, int64_t p_sv, const int64_t *frame_lens, int64_t n_frames,
    int64_t N, int64_t V, int64_t width, const float *logps, const float *logbs, const int32_t *child_start,
    const int32_t *ids, const int32_t *succ_start, const int32_t *succ_tok, const int32_t *succ_node,
    int64_t max_ngram, int64_t U, int64_t sos, float beta, int valid_mixture, int64_t *y, int64_t *y_lens,
    float *nb, float *b, void *workspace, int64_t workspace_bytes, void *stream);

int pdt_beam_search_step(const float *scores, int64_t sc_sn, int64_t sc_sk, int64_t sc_sv, int64_t N,
                         int64_t Kp, int64_t V, int64_t width, const float *log_probs_prev,
                         int64_t lp_sn, int64_t lp_sk, const int64_t *y_prev, int64_t S,
                         int64_t yp_ss, int64_t yp_sn, int64_t yp_sk, const int64_t *y_prev_lens,
                         int64_t le_sn, int64_t le_sk, int has_eos, int64_t eos, int finish_all_paths,
                         int64_t pad_value, int64_t *y_next, int64_t *y_next_lens,
                         float *log_probs_next, int64_t *next_src, int32_t *active,
                         int32_t *pad_from, void *stream);


/* Table form of pdt_beam_search_step: the scores of prefix (n, k) are row rows[n * Kp + k] (int64,
 * in [0, U)) of a (U, V) table -- e.g. the rows of a bigram LookupLanguageModel by context token,
 * computed once -- and, if row_stats (U, 2) is given (pdt_row_log_softmax_stats of the same table), a
 * row's maximum and log-sum-exp are read from it instead of being recomputed every iteration.
 * Everything else as pdt_beam_search_step; the same bits. */
int pdt_beam_search_step_table(const float *table, int64_t tb_sr, int64_t tb_sv, int64_t U,
                               const float *row_stats, const int64_t *rows, int64_t N, int64_t Kp,
                               int64_t V, int64_t width, const float *log_probs_prev, int64_t lp_sn,
                               int64_t lp_sk, const int64_t *y_prev, int64_t S, int64_t yp_ss,
                               int64_t yp_sn, int64_t yp_sk, const int64_t *y_prev_lens, int64_t le_sn,
                               int64_t le_sk, int has_eos, int64_t eos, int finish_all_paths,
                               int64_t pad_value, int64_t *y_next, int64_t *y_next_lens,
                               float *log_probs_next, int64_t *next_src, int32_t *active,
                               int32_t *pad_from, void *stream);
/* stats[2 r], stats[2 r + 1] = max_v table[r][v], log sum_v exp(table[r][v] - max) */
int pdt_row_log_softmax_stats(const float *table, int64_t tb_sr, int64_t tb_sv, int64_t U, int64_t V,
                              float *stats, void *stream);

/* ---------------------------------------------------------------------------------------
 * Random walks (reference _decoding.py:1207-1513).  Every token is drawn by one rule from a row x of
 * log-weights (any normalisation) and a uniform u in [0, 1) the caller draws: with m = max x and
 * lse = log sum exp(x - m) (as pdt_row_log_softmax_stats forms them), w_v = exp(x_v - m) and Z = exp(lse),
 * the token is the smallest v with w_v > 0 whose running prefix sum of w exceeds u Z, else the largest v
 * with w_v > 0.  A row without positive finite mass (all -inf, a NaN, +inf) draws nothing: it raises
 * PDT_WALK_INVALID and writes token 0.  One wave per walk.
 * A launch reports through ctl (device int32[4], zeroed before the first launch that uses it; every launch
 * leaves it zeroed) into host_words (int32[3], pinned host memory): host_words[1] = walks still live,
 * host_words[2] = the longest walk (table form), and host_words[0] = PDT_WALK_DONE | PDT_WALK_* bits,
 * stored last with release semantics at system scope -- the host may poll it instead of synchronising.
 *
 * pdt_random_walk_advance: random_walk_advance.  log_probs_t (N, V), u / log_probs_prev (N,) float32;
 *   y_prev (S, N) int64; y_prev_lens (N,) or NULL.  y_next (S + 1, N) contiguous: the history, the token
 *   in row S and, with lengths and S > 0, in row y_prev_lens[n] (:1272-1279); PDT_WALK_REACH when some
 *   length reaches S -- the caller keeps S + 1 rows then, or when there are no lengths or S = 0, else S.
 *   A length outside [0, S] raises PDT_WALK_BAD_LENS and is not written.
 *   log_probs_next[n] = log_probs_prev[n] + log_probs_t[n, token] (float32; not renormalised).
 * pdt_random_walk_step: one iteration of RandomWalk.forward with the default hook.  scores (N, V) are the
 *   model's output; a walk with ended[n] set emits eos at no cost; otherwise it draws from
 *   log_softmax(scores) with u[n], log_probs[n] += its log-probability, lens[n] += 1, ended[n] = (token ==
 *   eos).  The token goes to y_t[n].  host_words[1]: walks not ended afterwards.
 * pdt_random_walk_table: C iterations of the same walk over a dense context table (R, V) of an n-gram
 *   model and its row_stats (R, 2): walk n continues from context row ctx[n], moving to
 *   (ctx * U + token) mod R after each token; u (C, N), y (C, N) contiguous; the state (ctx, lens, ended,
 *   log_probs) is read at the start and written back at the end.
 * ------------------------------------------------------------------------------------- */
#define PDT_WALK_DONE 1
#define PDT_WALK_INVALID 2
#define PDT_WALK_REACH 4
#define PDT_WALK_BAD_LENS 8
int pdt_random_walk_advance(const float *log_probs_t, int64_t lt_sn, int64_t lt_sv, int64_t N, int64_t V,
                            const float *u, int64_t u_sn, const float *log_probs_prev, int64_t lp_sn,
                            const int64_t *y_prev, int64_t S, int64_t yp_ss, int64_t yp_sn,
                            const int64_t *y_prev_lens, int64_t le_sn, int64_t *y_next, float *log_probs_next,
                            int32_t *ctl, int32_t *host_words, void *stream);
int pdt_random_walk_step(const float *scores, int64_t sc_sn, int64_t sc_sv, int64_t N, int64_t V, const float *u,
                         int has_eos, int64_t eos, int64_t *y_t, int64_t *lens, uint8_t *ended, float *log_probs,
                         int32_t *ctl, int32_t *host_words, void *stream);
int pdt_random_walk_table(const float *table, int64_t tb_sr, int64_t R, int64_t U, int64_t V, const float *row_stats,
                          const float *u, int64_t N, int64_t C, int has_eos, int64_t eos, int64_t *y, int64_t *ctx,
                          int64_t *lens, uint8_t *ended, float *log_probs, int32_t *ctl, int32_t *host_words,
                          void *stream);

/* ---------------------------------------------------------------------------------------
 * ctc_greedy_search (reference _decoding.py:507-558).  logits (T, N, V) float32 (float16 /
 * bfloat16: the _elem entry points below, see pdt_ctc_prefix_search_elem) through element
 * strides; blank_idx already normalised to [0, V).  max_out (N,): sum of the per-frame maximum
 * log-probabilities (is_probs: product of the maxima, no normalisation) over frames below
 * in_lens; paths (T, N) int64 through strides: the first out_lens[n] entries of column n are
 * the collapsed tokens, the rest the raw per-frame arg-max (as the reference leaves them).
 *
 * sequence_log_probs on tensors (_decoding.py:1516-1551).  hyp viewed as (A, S, B) with S the
 * step axis, logits (A, S, B, V) contiguous, of the same element types; out (A, B) float32 = sum over valid steps of
 * log_softmax(logits)[hyp]; tokens outside [0, V) and steps after the first eos are skipped.
 * Backward: grad_logits (same layout, the logits' element type) from grad_out (A, B) float32.
 * PDT_E_TOO_LONG: V >= 2^30 (all three; V is an int in the kernels), T beyond the LDS of the greedy
 * search (more than 20 480 frames), N, A, S, B or A * B >= 2^31.
 * ------------------------------------------------------------------------------------- */
int pdt_ctc_greedy_search(const float *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                          int64_t lg_sn, int64_t lg_sv, const int64_t *in_lens, int64_t blank_idx,
                          int is_probs, float *max_out, int64_t *paths, int64_t pa_st,
                          int64_t pa_sn, int64_t *out_lens, void *stream);

/* (the three below: logits of the element type `elem`, see pdt_ctc_prefix_search_elem) */
int pdt_ctc_greedy_search_elem(const void *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                               int64_t lg_sn, int64_t lg_sv, const int64_t *in_lens, int64_t blank_idx,
                               int is_probs, float *max_out, int64_t *paths, int64_t pa_st,
                               int64_t pa_sn, int64_t *out_lens, void *stream, int elem);

int pdt_sequence_log_probs_forward(const float *logits, const int64_t *hyp, int64_t A, int64_t S,
                                   int64_t B, int64_t V, int has_eos, int64_t eos, float *out,
                                   void *stream);

int pdt_sequence_log_probs_forward_elem(const void *logits, const int64_t *hyp, int64_t A, int64_t S,
                                        int64_t B, int64_t V, int has_eos, int64_t eos, float *out,
                                        void *stream, int elem);

int pdt_sequence_log_probs_backward(const float *logits, const int64_t *hyp, int64_t A, int64_t S,
                                    int64_t B, int64_t V, int has_eos, int64_t eos,
                                    const float *grad_out, float *grad_logits, void *stream);

int pdt_sequence_log_probs_backward_elem(const void *logits, const int64_t *hyp, int64_t A, int64_t S,
                                         int64_t B, int64_t V, int has_eos, int64_t eos,
                                         const float *grad_out, void *grad_logits, void *stream, int elem);

/* ---------------------------------------------------------------------------------------
 * Feature augmentation / image warps (reference _img.py).  All tensors float32 and
 * contiguous unless strides are given.
 *
 * pdt_polyharmonic_spline: polyharmonic_spline (_img.py:59-150).  train_points (N,T,I),
 *   train_values (N,T,O), query_points (N,Q,I) -> out (N,Q,O).  The bordered system is solved
 *   exactly (float64, partial pivoting; in LDS up to ~140 unknowns, in the workspace beyond),
 *   which covers both of the reference's `full_matrix` evaluation orders.
 *   workspace: pdt_spline_workspace_bytes(N,T,I,O) bytes.
 * pdt_spline_solve: the solve alone, with an optional right-hand-side tail: solution (N, T+I+1, O)
 *   float64 of [[phi(|c_i - c_j|) + reg I, [c 1]], [[c 1]^T, 0]] X = [train_values; tail]
 *   (tail (N, I+1, O) or NULL = zeros).  The spline's weights (_img.py:79-130), and -- the matrix
 *   being symmetric -- the adjoint system of its backward pass.
 * pdt_warp_1d_grid: warp_1d_grid (_img.py:268-303): src, flow, lengths (N,) -> grid (N,T).
 * pdt_spec_augment_apply: spec_augment_apply_parameters (_img.py:1142-1211).  feats (N,T,F)
 *   through element strides; time_grid (N,T) / freq_grid (N,F) normalised sampling grids or
 *   NULL (no warp along that axis); t_0/t_len (N,MT), f_0/f_len (N,MF) int64 mask bands
 *   (MT / MF = 0: none); out (N,T,F) contiguous.
 * pdt_dense_image_warp: dense_image_warp (_img.py:393-439).  image (N,C,H,W), flow (N,H,W,2);
 *   flow_is_hw: last dim of flow is (h, w) ("hw" indexing) instead of (w, h).
 *   mode: 0 bilinear, 1 nearest; padding: 0 zeros, 1 border, 2 reflection.
 * pdt_sparse_image_warp: sparse_image_warp (_img.py:520-714) after the caller has appended the
 *   pinned boundary points and put points in (x=w, y=h) order: train_points (N,M,2) = dest
 *   points; train_values (N,M,2) = dest - source (flow form) or the normalised source grid
 *   (values_are_grid = 1, the include_flow=False form).  flow_out (N,H,W,2) optional
 *   (flow form only), stored (h, w)-ordered when flow_out_is_hw.
 *   workspace: pdt_spline_workspace_bytes(N, M, 2, 2) bytes.
 * pdt_*_backward: adjoints of the three resampling operators with respect to the features /
 *   image (what autograd derives through grid_sample in the reference, _img.py:436, :1203):
 *   grad_out has the forward output's shape, contiguous; grad_feats / grad_image (contiguous)
 *   is overwritten.  The sampling arguments are the forward call's.  Accumulation uses the
 *   hardware float atomic, so sums are not bit-reproducible from run to run.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_spline_workspace_bytes(int64_t N, int64_t T, int64_t I, int64_t O);

int pdt_spline_solve(const float *train_points, const float *train_values, const float *tail,
                     int64_t N, int64_t T, int64_t I, int64_t O, int order,
                     float regularization_weight, double *solution, void *workspace, void *stream);

int pdt_polyharmonic_spline(const float *train_points, const float *train_values,
                            const float *query_points, int64_t N, int64_t T, int64_t I, int64_t O,
                            int64_t Q, int order, float regularization_weight, float *out,
                            void *workspace, void *stream);

int pdt_warp_1d_grid(const float *src, const float *flow, const float *lengths, int64_t N, int64_t T,
                     int order, float *grid, void *stream);

/* spec_augment_draw_parameters (_img.py:1056-1139) from one (N, R) tensor of uniform draws u in
 * [0, 1): column c is utterance n's c-th draw in the reference's order (w_0, w | v_0, v | t x MT,
 * t_0 x MT | f x MF, f_0 x MF; groups the configuration disables take no columns and their outputs
 * may be NULL); every parameter is the reference's float32 expression of its uniform.  lengths (N,)
 * int64 or NULL (all T).  is_double: the features are float64 (the reference's eps follows them). */
int pdt_spec_augment_draw(const float *u, int64_t N, int64_t R, const int64_t *lengths, int64_t T,
                          int64_t F, float max_time_warp, float max_freq_warp, int64_t max_time_mask,
                          int64_t max_freq_mask, float max_time_mask_proportion, int64_t num_time_mask,
                          float num_time_mask_proportion, int64_t num_freq_mask, int is_double,
                          float *w_0, float *w, float *v_0, float *v, int64_t *t_0, int64_t *t,
                          int64_t *f_0, int64_t *f, void *stream);

int pdt_spec_augment_apply(const float *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn,
                           int64_t f_st, int64_t f_sf, const float *time_grid,
                           const float *freq_grid, const int64_t *t_0, const int64_t *t_len,
                           int64_t MT, const int64_t *f_0, const int64_t *f_len, int64_t MF,
                           float *out, void *stream);

/* spec_augment_apply_parameters with the TIME WARP given by its parameters (w_0 = warp_src, w =
 * warp_flow, float (N,); lengths int64 (N,) or NULL = all T; interpolation order) instead of a grid:
 * warp_1d_grid's three-knot spline (_img.py:283-302) is solved in closed form (float64) and evaluated
 * inside the one pass over the features -- one launch, no (N, T) grid in memory.  No frequency warp.
 * PDT_E_UNSUPPORTED when the one-pass kernel does not take the layout (F not a multiple of 4 or above
 * 256, strided or unaligned rows): form the grid with pdt_warp_1d_grid and call pdt_spec_augment_apply.
 * bad_lengths (optional): an int32 in device-visible memory (e.g. pinned host memory) the caller has
 * set to 0; an utterance whose length is outside [1, T] stores 1 there -- the reference's
 * "values of lengths must be between (1, T)" check (_img.py:1037-1041) decided where the lengths are
 * read, for the caller to look at once the stream has drained (the result is then to be dropped). */
int pdt_spec_augment_apply_warp(const float *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn,
                                int64_t f_st, int64_t f_sf, const float *warp_src, const float *warp_flow,
                                const int64_t *lengths, int order, const int64_t *t_0,
                                const int64_t *t_len, int64_t MT, const int64_t *f_0,
                                const int64_t *f_len, int64_t MF, float *out, int32_t *bad_lengths,
                                void *stream);

int pdt_dense_image_warp(const float *image, const float *flow, int64_t N, int64_t C, int64_t H,
                         int64_t W, int flow_is_hw, int mode, int padding, float *out,
                         void *stream);

int pdt_sparse_image_warp(const float *image, const float *train_points,
                          const float *train_values, int64_t N, int64_t C, int64_t H, int64_t W,
                          int64_t M, int order, float regularization_weight, int values_are_grid,
                          int mode, int padding, float *out, float *flow_out, int flow_out_is_hw,
                          void *workspace, void *stream);

/* float64 images: the reference samples a double image on a double grid (_img.py:423-436) while
 * flows and spline points stay float32 (:420, :537-538).  Same arguments as the float32 entries. */
int pdt_dense_image_warp_f64(const double *image, const float *flow, int64_t N, int64_t C, int64_t H,
                             int64_t W, int flow_is_hw, int mode, int padding, double *out,
                             void *stream);
int pdt_dense_image_warp_backward_f64(const double *grad_out, const float *flow, int64_t N, int64_t C,
                                      int64_t H, int64_t W, int flow_is_hw, int mode, int padding,
                                      double *grad_image, void *stream);
int pdt_sparse_image_warp_f64(const double *image, const float *train_points,
                              const float *train_values, int64_t N, int64_t C, int64_t H, int64_t W,
                              int64_t M, int order, float regularization_weight, int values_are_grid,
                              int mode, int padding, double *out, float *flow_out, int flow_out_is_hw,
                              void *workspace, void *stream);
int pdt_sparse_image_warp_backward_f64(const double *grad_out, const float *train_points,
                                       const float *train_values, int64_t N, int64_t C, int64_t H,
                                       int64_t W, int64_t M, int order, float regularization_weight,
                                       int values_are_grid, int mode, int padding, double *grad_image,
                                       void *workspace, void *stream);

int pdt_spec_augment_apply_backward(const float *grad_out, int64_t N, int64_t T, int64_t F,
                                    const float *time_grid, const float *freq_grid,
                                    const int64_t *t_0, const int64_t *t_len, int64_t MT,
                                    const int64_t *f_0, const int64_t *f_len, int64_t MF,
                                    float *grad_feats, void *stream);

/* The three application entry points on features kept in float16 / bfloat16, read and written as they are
 * (new names; the declarations above are unchanged).  elem: 0 float32 -- the very launch of the entry point
 * without the suffix --, 2 float16, 3 bfloat16; 1 (float64) is PDT_E_UNSUPPORTED, anything else PDT_E_ARG,
 * judged with every pointer before any device work.  feats / out / grad_out / grad_feats are of that type,
 * strides in elements; grids, warp parameters and masks stay float32 / int64.  The arithmetic is float32: a
 * call is the float32 call on the exactly widened features, each result rounded once, to nearest even, where
 * it is stored; a masked element is +0 whatever lies under the mask.
 *   pdt_spec_augment_apply_form: host only, no device work -- the kernel the launchers take (they decide
 *   through this function): 0 the general kernel, 1 the rows kernel (no frequency grid, F % 4 == 0, F <= 256,
 *   f_sf == 1, f_st and f_sn multiples of 4 elements, in_addr and out_addr multiples of 4 element sizes; the
 *   adjoint (backward = 1) takes its tensors as contiguous whatever strides are passed and adds 12 T + 1296
 *   <= 65536 bytes of LDS).  No form moves eight elements per lane: 2 is never returned.  Negative: PDT_E_*
 *   (the element code, negative sizes, T * F >= 2^31).  pdt_spec_augment_apply_warp(_elem) returns
 *   PDT_E_UNSUPPORTED wherever this is not 1 with both grid flags 0.
 *   pdt_spec_augment_apply_backward_elem: with a grid, on the general (scatter) form, a half type accumulates
 *   in `workspace`, N * T * F floats the entry point zeroes itself, and rounds them into grad_feats in a
 *   second launch; PDT_E_ARG when it is NULL or shorter.  Every other route ignores it.
 *   pdt_spec_augment_backward_workspace_bytes: host only -- that size; has_grid: bit 0 a time grid, bit 1 a
 *   frequency grid.  0 for float32, for no grid and for a time grid alone on a shape of the rows form (the
 *   tensors taken as aligned to 8 bytes: ask pdt_spec_augment_apply_form with the addresses to be sure);
 *   -1 for an element code that is not 0, 2 or 3 and for negative sizes. */
int pdt_spec_augment_apply_elem(const void *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st,
                                int64_t f_sf, const float *time_grid, const float *freq_grid, const int64_t *t_0,
                                const int64_t *t_len, int64_t MT, const int64_t *f_0, const int64_t *f_len,
                                int64_t MF, void *out, void *stream, int elem);
int pdt_spec_augment_apply_warp_elem(const void *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st,
                                     int64_t f_sf, const float *warp_src, const float *warp_flow,
                                     const int64_t *lengths, int order, const int64_t *t_0, const int64_t *t_len,
                                     int64_t MT, const int64_t *f_0, const int64_t *f_len, int64_t MF, void *out,
                                     int32_t *bad_lengths, void *stream, int elem);
int pdt_spec_augment_apply_backward_elem(const void *grad_out, int64_t N, int64_t T, int64_t F, const float *time_grid,
                                         const float *freq_grid, const int64_t *t_0, const int64_t *t_len, int64_t MT,
                                         const int64_t *f_0, const int64_t *f_len, int64_t MF, void *grad_feats,
                                         void *stream, int elem, void *workspace, int64_t workspace_bytes);
int64_t pdt_spec_augment_backward_workspace_bytes(int64_t N, int64_t T, int64_t F, int has_grid, int elem);
int pdt_spec_augment_apply_form(int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st, int64_t f_sf,
                                uint64_t in_addr, uint64_t out_addr, int has_time_grid, int has_freq_grid,
                                int backward, int elem);

int pdt_dense_image_warp_backward(const float *grad_out, const float *flow, int64_t N, int64_t C,
                                  int64_t H, int64_t W, int flow_is_hw, int mode, int padding,
                                  float *grad_image, void *stream);

int pdt_sparse_image_warp_backward(const float *grad_out, const float *train_points,
                                   const float *train_values, int64_t N, int64_t C, int64_t H,
                                   int64_t W, int64_t M, int order, float regularization_weight,
                                   int values_are_grid, int mode, int padding, float *grad_image,
                                   void *workspace, void *stream);

/* Gradients of the warps with respect to WHERE they sample (what autograd derives through grid_sample's
 * grid in the reference, _img.py:436): per pixel, grad_out times the derivative of the bilinear blend,
 * chained through the padding rule (torch's clip_coordinates_set_grad / reflect_coordinates_set_grad), the
 * un-normalisation and the grid formula.  grad_out and image (N,C,H,W) in one type (float, or double for the
 * _f64 entries); the outputs are float32 (N,H,W,2), overwritten.  mode = 1 (nearest): zeros.  Limits and
 * argument checks are those of the forward entry points.
 * pdt_dense_image_warp_flow_backward: grad_flow, in the flow's own order (flow_is_hw).
 * pdt_sparse_image_warp_position_backward: grad_values = the gradient with respect to the spline's value
 *   at every pixel in (x, y) order -- the G of pdt_spline_eval_adjoint over the pixel lattice.  solution: the
 *   (N, M + 3, 2) float64 solution of the spline (pdt_spline_solve of the forward call's train_points /
 *   train_values); grad_flow: optional (N,H,W,2) gradient of the returned flow (flow form only), (h, w)-
 *   ordered when grad_flow_is_hw, added.  workspace: pdt_spline_workspace_bytes(N, M, 2, 2) bytes.
 *
 * pdt_spline_eval_adjoint: the query-sized half of the spline's backward as a deterministic two-stage
 *   reduction over the Q queries (float64 sums; per-workgroup partials, then a fixed-order sum; the same
 *   bits every run).  grad_out G (N,Q,O) float; train_points (N,T,I); solution (N, T+I+1, O) float64;
 *   query_points (N,Q,I), or NULL = the pixel lattice x_q = (q % W, q / W) of an H x W image (I = 2,
 *   Q = H * W).  Out, float64: rhs (N, T+I+1, O) = [Phi(x, c)^T G; [x 1]^T G], the right-hand side of the
 *   adjoint system; grad_points (N,T,I) = -sum_q (G w^T)[q,t] slope(r_qt) (x_q - c_t), the evaluation's
 *   share of the centres' gradient; grad_query (N,Q,I) or NULL = the queries' gradient.  I, O <= 4, else
 *   PDT_E_UNSUPPORTED.  workspace: plan[2] bytes of pdt_spline_eval_adjoint_plan.
 * pdt_spline_eval_adjoint_plan (host only): returns the form -- 0: a workgroup holds all T + I + 1 rows and
 *   several slices of q; 1: more rows than a workgroup has lanes, row tiles -- or an error code, and fills
 *   plan[6] (may be NULL): form, workgroups per batch element, workspace bytes, grad_query's kernel reads
 *   solution and centres from LDS (1) or global memory (0), slices, queries per workgroup. */
int pdt_dense_image_warp_flow_backward(const float *grad_out, const float *image, const float *flow, int64_t N,
                                       int64_t C, int64_t H, int64_t W, int flow_is_hw, int mode, int padding,
                                       float *grad_flow, void *stream);
int pdt_dense_image_warp_flow_backward_f64(const double *grad_out, const double *image, const float *flow,
                                           int64_t N, int64_t C, int64_t H, int64_t W, int flow_is_hw, int mode,
                                           int padding, float *grad_flow, void *stream);
int pdt_sparse_image_warp_position_backward(const float *grad_out, const float *image, const float *train_points,
                                            const double *solution, int64_t N, int64_t C, int64_t H, int64_t W,
                                            int64_t M, int order, int values_are_grid, int mode, int padding,
                                            const float *grad_flow, int grad_flow_is_hw, float *grad_values,
                                            void *workspace, void *stream);
int pdt_sparse_image_warp_position_backward_f64(const double *grad_out, const double *image,
                                                const float *train_points, const double *solution, int64_t N,
                                                int64_t C, int64_t H, int64_t W, int64_t M, int order,
                                                int values_are_grid, int mode, int padding, const float *grad_flow,
                                                int grad_flow_is_hw, float *grad_values, void *workspace,
                                                void *stream);
int pdt_spline_eval_adjoint_plan(int64_t N, int64_t T, int64_t I, int64_t O, int64_t Q, int64_t *plan);
int pdt_spline_eval_adjoint(const float *grad_out, const float *train_points, const double *solution,
                            const float *query_points, int64_t N, int64_t T, int64_t I, int64_t O, int64_t Q,
                            int64_t H, int64_t W, int order, double *rhs, double *grad_points,
                            double *grad_query, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Back-off n-gram language model scoring (reference _lm.py:403-515, LookupLanguageModel
 * :518-1110), the on-device LM of CTCPrefixSearch / BeamSearch with shallow fusion.
 *
 * The model is the reference's reverse trie (:609-677) in widened form: logps [P] and
 * logbs [O] float32 as stored; child_start [O] int32 = node index + offsets[node] (absolute
 * index of the node's first child; the children of i are [child_start[i], child_start[i+1]));
 * ids [I] int32 = labels of the nodes >= U (index node - U).  V vocabulary size, N >= 2 the
 * n-gram order, U = V + shift + 1 the unigram count + dummy (shift = 1 when sos is not a
 * vocabulary id; it is then stored as unigram V).
 *
 * hist (S, B) int64 through element strides.  idx != NULL: rows == B, row b is queried at
 * position idx[b * idx_stride] in [0, S] (idx_stride 0 = one shared position) --
 * calc_idx_log_probs (:769-790).  idx == NULL: rows == (S + 1) * B, row t * B + b is batch
 * element b at position t -- calc_full_log_probs (:793-848).  Positions before the start of
 * the history read sos (:452-461).  out (rows, V) float32: log P(v | the N - 1 tokens before
 * the position).  status bit 0: a position outside [0, S] (clamped).
 *
 * succ_start [U + 1], succ_tok [E], succ_node [E] int32 (all three or NULL): a forward index of
 * the trie's second level, derived from the buffers above -- for a context token c, entries
 * succ_start[c] .. succ_start[c + 1] list the last tokens v (ascending) and nodes of the bigrams
 * "c v".  With it a row searches the children of the listed successors only (same results).
 * ------------------------------------------------------------------------------------- */
int pdt_lookup_lm_log_probs(const int64_t *hist, int64_t S, int64_t B, int64_t h_ss, int64_t h_sb,
                            const int64_t *idx, int64_t idx_stride, int64_t rows,
                            const float *logps, const float *logbs, const int32_t *child_start,
                            const int32_t *ids, const int32_t *succ_start, const int32_t *succ_tok,
                            const int32_t *succ_node, int64_t V, int64_t N, int64_t U, int64_t sos,
                            float *out, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Extension probabilities of one frame of CTCPrefixSearch with a language model (reference
 * _decoding.py:1110-1135), fused into one pass over the LM scores:
 *   lm_log_probs (N, Kp, V) float32 contiguous (unnormalised scores, as the LM returns them),
 *   nonext (N, V) / blank (N,) the frame's CTC probabilities through element strides;
 *   valid_mixture == 0: out = nonext * exp(beta * log_softmax(lm_log_probs))        (shallow fusion)
 *   valid_mixture != 0: out = (1 - beta) * nonext + beta * softmax(lm_log_probs) * (1 - blank)
 *   out (N, Kp, V) float32 contiguous.  No gradient (the differentiable path composes torch ops).
 *   PDT_E_TOO_LONG: V >= 2^30, Kp above 2^31 - 1, N * Kp >= 2^33 (pdt_lm_factor_table: V, rows >= 2^33).
 * ------------------------------------------------------------------------------------- */
int pdt_fusion_ext(const float *lm_log_probs, int64_t N, int64_t Kp, int64_t V, const float *nonext,
                   int64_t ne_sn, int64_t ne_sv, const float *blank, int64_t bl_sn, float beta,
                   int valid_mixture, float *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Variable-length padding (reference _pad.py:108-149), the data movement of RandomShift
 * (_img.py:883-908).  x (N, T, F) contiguous, elements of elem_bytes in {1, 2, 4, 8} moved as
 * opaque words; lens (N,), pad (2, N) int64; out (N, Tp, F) with Tp >= max(lens + pad sums):
 *   out[n, :pad[0,n]]                          left padding
 *   out[n, pad[0,n] : pad[0,n] + lens[n]]      x[n, :lens[n]]
 *   ... + pad[1,n]                             right padding;  the rest: *fill
 * mode 0 constant (*fill), 1 reflect (x[n, pad0 - t], x[n, lens - 2 - j]; the caller checks
 * pad < lens), 2 replicate (x[n, 0], x[n, lens - 1]; the caller checks lens >= 1).
 * pdt_pad_variable_backward: the adjoint with respect to x, written as a gather (deterministic),
 * dtype 0 float32 / 1 float64; grad_out (N, Tp, F), grad_x (N, T, F) of that type.
 * PDT_E_TOO_LONG: an output (backward: grad_x) of 2^32 - 4096 elements or more -- elements are numbered
 * with 32 bits -- or N, T, F or Tp above 2^31 - 1; the same for pdt_gather_steps and pdt_chunk_by_slices.
 * ------------------------------------------------------------------------------------- */
int pdt_pad_variable(const void *x, int64_t N, int64_t T, int64_t F, int64_t elem_bytes,
                     const int64_t *lens, const int64_t *pad, int mode, const void *fill,
                     int64_t Tp, void *out, void *stream);

int pdt_pad_variable_backward(const void *grad_out, int dtype, int64_t N, int64_t T, int64_t F,
                              const int64_t *lens, const int64_t *pad, int mode, int64_t Tp,
                              void *grad_x, void *stream);

/* ---------------------------------------------------------------------------------------
 * Feature deltas (reference _feats.py:216-286).  x is indexed (A, B, T, C, D) with element
 * strides xs_*; dtype 0 float32, 1 float64, 2 float16, 3 bfloat16.  taps (U, 1 + 2P) are in the
 * compute type (float64 for float64, float32 otherwise); fill is one compute-type element read in
 * mode 3.  out[u] at position t is sum_k taps[u, k] * xpad[t + k - P] over the padded time axis:
 * mode 0 replicate, 1 reflect (the caller checks P < T), 2 circular (P <= T), 3 constant.  out
 * is contiguous (A, U, B, T, C, D), or (A, B, T, C, U, D) when u_inner.  T == 0 is an error.
 * pdt_feat_deltas_backward: the adjoint, grad_out in the forward's output layout, grad_x
 * (A, B, T, C, D) contiguous; a gather, deterministic.
 * ------------------------------------------------------------------------------------- */
int pdt_feat_deltas(const void *x, int dtype, int64_t A, int64_t B, int64_t T, int64_t C, int64_t D,
                    int64_t xs_a, int64_t xs_b, int64_t xs_t, int64_t xs_c, int64_t xs_d, const void *taps,
                    int64_t U, int64_t P, int mode, const void *fill, int u_inner, void *out, void *stream);

int pdt_feat_deltas_backward(const void *grad_out, int dtype, int64_t A, int64_t B, int64_t T, int64_t C,
                             int64_t D, const void *taps, int64_t U, int64_t P, int mode, int u_inner,
                             void *grad_x, void *stream);

/* ---------------------------------------------------------------------------------------
 * Mean/variance normalisation (reference _feats.py:29-214).  x (A, X, B) contiguous, statistics
 * per index of X over the A * B samples; dtype as for the deltas.
 * pdt_mvn_stats: a two-stage float64 reduction through a workspace of
 * pdt_mvn_stats_workspace_bytes(A, X, B) bytes, fixed order, no atomics:
 *   mode 0  out0 = mean, out1 = population std (sums shifted by the index's first sample)
 *   mode 1  out0 += sum x, out1 += sum x^2, count[0] += A * B (in place, on the stream)
 *   mode 2  out0 = sum g, out1 = sum g * c, c = x - mean[i] rounded to x's dtype (g like x)
 * pdt_mvn_apply: y = (x - mean[i]) / scale[i], mean / scale (X,) in x's dtype, the difference
 * rounded to x's dtype first.  pdt_mvn_backward: grad_x = grad_y * coef[0, i] + coef[1, i] +
 * coef[2, i] * c, coef (3, X) in the compute type.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_mvn_stats_workspace_bytes(int64_t A, int64_t X, int64_t B);

int pdt_mvn_stats(const void *x, const void *g, const void *mean, int dtype, int64_t A, int64_t X, int64_t B,
                  int mode, double *out0, double *out1, double *count, void *workspace, int64_t workspace_bytes,
                  void *stream);

int pdt_mvn_apply(const void *x, int dtype, int64_t A, int64_t X, int64_t B, const void *mean, const void *scale,
                  void *y, void *stream);

int pdt_mvn_backward(const void *grad_y, const void *x, int dtype, int64_t A, int64_t X, int64_t B, const void *mean,
                     const void *coef, void *grad_x, void *stream);

/* ---------------------------------------------------------------------------------------
 * Soft attention (reference _attn.py:200-223): out[r] = sum_t a[r, t] value[r, t], a the softmax
 * over t of the scores with masked frames at -inf; lse[r] the row's largest score and lse[R + r] the
 * log of its sum of exp(score - largest) (kept apart: their sum would round away the second next to
 * a large |score|).  dtype 0 float32,
 * 1 float64 (accumulated in the same type).
 * desc: PDT_ATTN_DESC_LEN int64, read on the host and copied into the kernel arguments:
 *   [0] nd <= PDT_ATTN_MAX_DIMS row dims, [1] R rows = product of the sizes = G * M, [2] G groups,
 *   [3] M rows per group (the innermost row dims, over which key, value and their gradients are
 *   broadcast), [4] T, [5] D (0 in the pool forms), [6] Dv, [7 .. 7 + MAX) the row sizes (outermost
 *   first), then per operand slot (query or score, key, value, mask, out / grad_out, grad_query or
 *   grad_score, grad_key, grad_value) MAX row strides, the T stride and the feature stride, in
 *   elements; 0 broadcasts.  lse is (2, R) in row order.  mask is bool bytes or NULL (all kept).
 * pdt_attn_dot: scores *scale * query . key (scale: one double in host memory).  pdt_attn_pool: the scores given (score slot).
 * pdt_attn_*_backward: the gradients, recomputing a from lse; grad_key / grad_value are summed
 * over the group.  Masked frames contribute exactly 0.  No float atomics: bitwise reproducible.
 * Workspaces of pdt_attn_workspace_bytes(desc, dtype, kind) bytes (kind 0 dot, 1 dot backward,
 * 2 pool, 3 pool backward; -1 for a bad descriptor).  R == 0 is OK; T == 0 with rows is an error
 * (the caller returns zeros).
 * ------------------------------------------------------------------------------------- */
#define PDT_ATTN_MAX_DIMS 8
#define PDT_ATTN_SLOTS 8
#define PDT_ATTN_DESC_LEN (7 + PDT_ATTN_MAX_DIMS + PDT_ATTN_SLOTS * (PDT_ATTN_MAX_DIMS + 2))

int64_t pdt_attn_workspace_bytes(const int64_t *desc, int dtype, int kind);

int pdt_attn_dot(const int64_t *desc, int dtype, const void *query, const void *key, const void *value,
                 const void *mask, const double *scale, void *out, void *lse, void *workspace, int64_t workspace_bytes,
                 void *stream);

int pdt_attn_dot_backward(const int64_t *desc, int dtype, const void *query, const void *key, const void *value,
                          const void *mask, const double *scale, const void *out, const void *lse, const void *grad_out,
                          void *grad_query, void *grad_key, void *grad_value, void *workspace,
                          int64_t workspace_bytes, void *stream);

int pdt_attn_pool(const int64_t *desc, int dtype, const void *score, const void *value, const void *mask, void *out,
                  void *lse, void *workspace, int64_t workspace_bytes, void *stream);

int pdt_attn_pool_backward(const int64_t *desc, int dtype, const void *score, const void *value, const void *mask,
                           const void *out, const void *lse, const void *grad_out, void *grad_score,
                           void *grad_value, void *workspace, int64_t workspace_bytes, void *stream);

/* The same for operands of the element type `elem` (0 float32, 2 float16, 3 bfloat16; 1 returns
 * PDT_E_UNSUPPORTED, any other value PDT_E_ARG, and the workspace query -1 for both: see
 * pdt_ctc_prefix_search_elem).  query, key, value, score, out and grad_out are read, out and the gradients
 * written, as elements of that type, without a float32 copy; rows need no alignment beyond the element's.
 * Everything between is float32: lse is float32 (2, R) for every element type, and the plan -- tiles, spans,
 * the choice of kernel, LDS and workspace bytes -- is that of the float32 call of the same descriptor.  out
 * has the bits of the float32 entry point's on the widened operands rounded to the element type (nearest
 * even), and the gradients those of its gradients on the widened operands and the widened out: each element
 * is rounded once, where it is stored.  (The gradients are therefore exact for the rounded out that was saved,
 * delta = rowsum(grad_out * out) included, not for the unrounded one.)  The element code and every argument
 * are checked before any launch.  The entry points above keep refusing every dtype but 0 and 1. */
int64_t pdt_attn_workspace_bytes_elem(const int64_t *desc, int elem, int kind);

int pdt_attn_dot_elem(const int64_t *desc, int elem, const void *query, const void *key, const void *value,
                      const void *mask, const double *scale, void *out, void *lse, void *workspace,
                      int64_t workspace_bytes, void *stream);

int pdt_attn_dot_backward_elem(const int64_t *desc, int elem, const void *query, const void *key, const void *value,
                               const void *mask, const double *scale, const void *out, const void *lse,
                               const void *grad_out, void *grad_query, void *grad_key, void *grad_value,
                               void *workspace, int64_t workspace_bytes, void *stream);

int pdt_attn_pool_elem(const int64_t *desc, int elem, const void *score, const void *value, const void *mask,
                       void *out, void *lse, void *workspace, int64_t workspace_bytes, void *stream);

int pdt_attn_pool_backward_elem(const int64_t *desc, int elem, const void *score, const void *value, const void *mask,
                                const void *out, const void *lse, const void *grad_out, void *grad_score,
                                void *grad_value, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * The additive ("concat") attention score (reference _attn.py:344-361) with the two halves of W
 * applied by the caller: e[r, t] = sum_h v[h] * tanh(a[r, h] + b[group(r), t, h]), formed without
 * a hidden-sized intermediate, and its adjoint with tanh recomputed:
 *   g = grad_e[r, t] * v[h] * (1 - tanh^2); grad_a[r, h] = sum_t g; grad_b[group, t, h] = sum over
 *   the group's rows of g; grad_v[h] = sum_{r, t} grad_e[r, t] * tanh.
 * dtype 0 float32, 1 float64 (accumulated in the same type).  tanh is exactly +-1 with an exact zero
 * derivative once it saturates (+-inf included); NaN propagates.  No mask: every frame is scored.
 * desc: PDT_ATTN_DESC_LEN int64 in the layout above, read on the host: [0] nd, [1] R = G * M,
 *   [2] G, [3] M rows per group (the innermost row dims, over which b and grad_b are broadcast),
 *   [4] T, [5] H, [6] the element stride of v, [7 ..) the row sizes, then the slots: 0 a (row
 *   strides, H stride), 1 b (row, T and H strides), 3 grad_e (row and T strides), 4 e (row and T
 *   strides), 5 grad_a (row and H strides), 6 grad_b (row, T and H strides); slots 2 and 7 are not
 *   read.  Strides in elements, 0 broadcasts, offsets are 64-bit.  grad_v is H contiguous elements.
 * pdt_concat_score_workspace_bytes(desc, dtype, kind): kind 0 forward (0 bytes), 1 backward (the
 *   grad_v partials of every workgroup and, with several frame chunks, those of grad_a; a combine
 *   pass adds them in a fixed order: no float atomics, bitwise reproducible); -1 for a bad descriptor.
 * pdt_concat_score_plan (host only, no device work): plan5 = rows per forward tile, H chunks,
 *   frames per forward workgroup, backward frame chunks (1: grad_a written directly, more: combined),
 *   backward workspace bytes.  All 0 when R, T or H is 0.
 * R == 0, T == 0 and H == 0 return PDT_OK without a launch (the sum over no features is 0: the
 * caller fills e and the gradients with zeros).
 * ------------------------------------------------------------------------------------- */
int64_t pdt_concat_score_workspace_bytes(const int64_t *desc, int dtype, int kind);

int pdt_concat_score_plan(const int64_t *desc, int dtype, int64_t *plan5);

int pdt_concat_score(const int64_t *desc, int dtype, const void *a, const void *b, const void *v, void *e,
                     void *stream);

int pdt_concat_score_backward(const int64_t *desc, int dtype, const void *a, const void *b, const void *v,
                              const void *grad_e, void *grad_a, void *grad_b, void *grad_v, void *workspace,
                              int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Slicing and chunking (reference _pad.py:257-548, _feats.py:417-930) on two primitives: stable
 * compaction within a row (one workgroup per row; ranks by wave ballot + popcount with a carry)
 * and a copy with an index map and a padding rule.  All lengths, slices and counts are int64;
 * maps are int32.  Every output element is written once: no pre-fill, no atomics.
 * pdt_compact_mask: mask bool bytes at mask[n * m_sn + t * m_st]; src[n, j] = the step of the j-th
 *   kept one (-1 for j >= counts[n]), rank[n, t] = where step t goes (-1 if dropped), both at
 *   [n * o_sn + . * o_st]; either may be NULL.
 * pdt_gather_steps: out[n, t, :] = x[n, map[n, t], :] (x through the element strides x_sn / x_st,
 *   F contiguous; map through m_sn / m_st), *fill where the map is negative; out (N, To, F), or
 *   (To, N, F) when time_major.  Elements of elem_bytes in {1, 2, 4, 8, 16} move as opaque words
 *   (16: a caller whose F elements, strides and pointers are multiples of 16 bytes passes groups
 *   of elements as one word, with F, the strides and *fill in those units; also pdt_chunk_by_slices).
 * pdt_chunk_by_slices: out[n, t, :], t < Tp, reads step s = slices[n, 0] + t of x[n] for
 *   t < slices[n, 1] - slices[n, 0]; with len = lens[n] (NULL: T), 0 <= s < len is x[n, s]; outside,
 *   mode 0 is *fill, 1 reflect (x[n, -s], x[n, 2 (len - 1) - s]), 2 replicate (x[n, clamp(s)]);
 *   the other steps are *fill.  The caller checks what reflect / replicate require.
 * pdt_chunk_stats: what the caller reads back first, in one launch: chunk_lens[n] =
 *   max(end - start, 0) and stats[0] = T' (the largest left pad, chunk length or right pad, pads of
 *   empty slices counting 0), stats[1] = max(pad - len) over both pads (>= 0: reflect is refused),
 *   stats[2] = min len (< 1: replicate is refused).  A len beyond T counts as T in the two copies.
 * pdt_chunk_by_slices_backward: the adjoint as a gather, dtype 0 float32 / 1 float64;
 *   grad_out (N, Tp, F), grad_x (N, T, F) contiguous.
 * pdt_chunk_tokens: refs (N, R, 3), slices (N, 2), ref_lens (N,) or NULL; out (N, R, 3) holds the
 *   kept triples left-packed (boundaries + slices[n, 0] unless retain), zeros past counts[n].
 * pdt_slice_*: the (slices, sources) lists of slice_spect_data.  With emit == 0 only counts[n]
 *   (kept candidates per row) is written; with emit != 0 row n's slices go to base[n] + rank
 *   (base NULL: n * TT, pdt_slice_fixed without lengths).  fixed: candidate k < TT is
 *   [a0 + k shift, a0 + k shift + width), kept when in_lens[n] > m0 + k shift.  ref: input
 *   (N, T, 3); other_lens NULL means the end of the row's last triple.  ali: input (N, T) labels;
 *   pdt_slice_ali_segments writes the first step of each run of equal labels (seg (N, T) int32,
 *   counts = runs per row), pdt_slice_ali_emit slice k < cnt[n] of row n from them: valid_only
 *   (seg[k], end of run k + left + right), else (seg[max(k - left, 0)], end of run
 *   min(k + right, runs - 1)); the last run ends at min(in_lens[n], T).
 * ------------------------------------------------------------------------------------- */
int pdt_compact_mask(const void *mask, int64_t N, int64_t T, int64_t m_sn, int64_t m_st, int32_t *src,
                     int32_t *rank, int64_t o_sn, int64_t o_st, int64_t *counts, void *stream);

int pdt_gather_steps(const void *x, int64_t N, int64_t T, int64_t F, int64_t elem_bytes, int64_t x_sn,
                     int64_t x_st, const int32_t *map, int64_t m_sn, int64_t m_st, int64_t To,
                     int time_major, const void *fill, void *out, void *stream);

int pdt_chunk_by_slices(const void *x, int64_t N, int64_t T, int64_t F, int64_t elem_bytes, int64_t x_sn,
                        int64_t x_st, const int64_t *slices, const int64_t *lens, int mode,
                        const void *fill, int64_t Tp, void *out, void *stream);

int pdt_chunk_stats(const int64_t *slices, const int64_t *lens, int64_t N, int64_t T, int64_t *chunk_lens,
                    int64_t *stats, void *stream);

int pdt_chunk_by_slices_backward(const void *grad_out, int dtype, int64_t N, int64_t T, int64_t F,
                                 const int64_t *slices, const int64_t *lens, int mode, int64_t Tp,
                                 void *grad_x, void *stream);

int pdt_chunk_tokens(const int64_t *refs, int64_t N, int64_t R, const int64_t *slices, const int64_t *ref_lens,
                     int partial, int retain, int64_t *out, int64_t *counts, void *stream);

int pdt_slice_fixed(int64_t N, int64_t TT, const int64_t *in_lens, int64_t a0, int64_t shift, int64_t width,
                    int64_t m0, const int64_t *base, int emit, int64_t *slices, int64_t *sources,
                    int64_t *counts, void *stream);

int pdt_slice_ref(const int64_t *input, int64_t N, int64_t T, const int64_t *in_lens, const int64_t *other_lens,
                  int64_t left, int64_t right, int valid_only, const int64_t *base, int emit, int64_t *slices,
                  int64_t *sources, int64_t *counts, void *stream);

int pdt_slice_ali_segments(const int64_t *input, int64_t N, int64_t T, const int64_t *in_lens, int32_t *seg,
                           int64_t *counts, void *stream);

int pdt_slice_ali_emit(const int32_t *seg, int64_t N, int64_t T, const int64_t *in_lens, const int64_t *nseg,
                       const int64_t *cnt, const int64_t *base, int64_t left, int64_t right, int valid_only,
                       int64_t *slices, int64_t *sources, void *stream);

/* ---------------------------------------------------------------------------------------
 * Discounted returns (reference _rl.py:24-41) as a scan.  r and R are indexed (t, n), t < T,
 * n < N, through element strides (any layout, no copy); dtype as for the deltas, accumulated in
 * float32 (float64 for float64).  gamma: one double in host memory, read before the call returns
 * (as the scale of pdt_attn_dot: the scalar types of this ABI are int, int64_t and float).
 *   reverse == 0: R[t] = r[t] + gamma * R[t + 1]   (R[T] = 0)
 *   reverse == 1: R[t] = r[t] + gamma * R[t - 1]   (R[-1] = 0), the adjoint of the above
 * The kernel follows R's dense axis; time is split into chunks (32 steps per lane when n is dense,
 * 1024 per wave when t is) when the other axis alone would leave the device idle, through a
 * workspace of pdt_time_distributed_return_workspace_bytes(...) bytes (0: none needed; -1: bad
 * arguments).  No power of gamma beyond one chunk is formed, none divided.  T == 0 or N == 0 is OK.
 * ------------------------------------------------------------------------------------- */
int64_t pdt_time_distributed_return_workspace_bytes(int64_t T, int64_t N, int dtype, int64_t R_st, int64_t R_sn);

int pdt_time_distributed_return(const void *r, int dtype, int64_t T, int64_t N, int64_t r_st, int64_t r_sn,
                                const double *gamma, int reverse, void *R, int64_t R_st, int64_t R_sn,
                                void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Combinatorics (reference _combinatorics.py:27-412).  out_type 0 int64, 1 int32, 2 uint8,
 * 3 float32, 4 float64.  table: the (67, 67) int64 Pascal table, table[l * 67 + c] = C(l, c), on
 * the device.
 * pdt_enumerate_vocab_sequences: out (vocab_size^length, length) contiguous, 16-byte aligned,
 *   out[s, t] = (s / vocab_size^t) % vocab_size.  length == 0 is OK (nothing to write);
 *   PDT_E_TOO_LONG when vocab_size^length reaches 2^32 (the row arithmetic is 32-bit).
 * pdt_binomial_coefficient: out[i] = C(length[i], count[i]), 0 when count > length.  flags[0]
 *   (zeroed by the caller) gets bit 0 for a negative input, bit 1 for a length above 66; such
 *   elements are written as 0.
 * pdt_enumerate_cardinality: out (B, rows, width): out[b, k, :] is the k-th binary sequence of
 *   length[b] elements with count[b] ones in ascending order of sum_t out[b, k, t] 2^t; rows at or
 *   beyond C(length[b], count[b]) and columns at or beyond length[b] are zeros.  length == count ==
 *   NULL: B == 1 and the scalars length0 / count0.  width <= 62.
 * pdt_srswor: Fan's sequential draw.  total_count, given_count (B,), u and out (B, out_size)
 *   float32 contiguous: with ell = given_count[b], for t = 0 .. out_size - 1
 *   out[b, t] = u[b, t] < (float)ell / (float)max(total_count[b] - t, 1), ell -= out[b, t].
 *   The caller guarantees 0 <= given_count <= total_count and u in [0, 1): a row's sum is then
 *   exactly given_count[b] and its elements from total_count[b] on are 0.  Not checked here.
 * ------------------------------------------------------------------------------------- */
int pdt_enumerate_vocab_sequences(int64_t length, int64_t vocab_size, int out_type, void *out, void *stream);

int pdt_binomial_coefficient(const int64_t *length, const int64_t *count, int64_t n, const int64_t *table,
                             int64_t *out, int32_t *flags, void *stream);

int pdt_enumerate_cardinality(const int64_t *length, const int64_t *count, int64_t length0, int64_t count0,
                              int64_t B, int64_t rows, int64_t width, const int64_t *table, int out_type,
                              void *out, void *stream);

int pdt_srswor(const int64_t *total_count, const int64_t *given_count, const float *u, int64_t B,
               int64_t out_size, float *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Relaxed sampling (reference _straight_through.py:251-598): one launch per method of the Gumbel /
 * one-hot categorical relaxation and of the logistic / Bernoulli one.  dtype 0 float32, 1 float64.
 * in1, in2 and out are R dense rows of V elements (out is (R,) for the Gumbel methods that reduce);
 * sample row r reads parameter row r mod B at param[(r mod B) * p_sr + j * p_sv].  The noise comes in
 * as data: u and v are clamped to [eps, 1 - eps] of the dtype, as are the probabilities.
 *   op  method     param   in1    in2  out
 *   0   rsample    logits  u      -    z      Gumbel: logits - log(-log u); logistic: logits + log u - log1p(-u)
 *   1   threshold  -       z      -    b      Gumbel: one-hot of the row arg-max (lowest index of a tie, -0 ties
 *                                             with +0, a NaN is the maximum); logistic: z >= 0
 *   2   tlog_prob  logits  b      -    lp     Gumbel (R,): sum_j [b_j != 0] logits_j; logistic: b logits - softplus(logits)
 *   3   csample    probs   b      v    zcond  Gumbel: k the first nonzero of b, z_k = -log(-log v_k), else
 *                                             min(z_k - eps, -log(-log v_j / p_j - log v_k)); logistic: lines 368-375
 *   4   log_prob   logits  z      -    lp     Gumbel (R,): sum_j g - exp g, g = logits - z; logistic: lines 340-347
 *   5   clog_prob  logits  zcond  b    lp     Gumbel (R,), lines 558-577, -inf unless b is the one-hot of zcond's
 *                                             arg-max; logistic: lines 377-393, -inf where (zcond >= 0) != b
 * R == 0 or V == 0 is OK (nothing to do).  PDT_E_TOO_LONG when V exceeds 2^31 - 65.
 * pdt_relaxed_group_width(V): the lanes that share a row, the power of two at or above V, 64 at most: the
 * widths at which the kernels change form (and 64, beyond which a lane takes more than one element).
 * pdt_relaxed_rows_per_block(V): rows served by one workgroup.  Both 0 for V < 1.
 * ------------------------------------------------------------------------------------- */
int pdt_relaxed_group_width(int64_t V);

int pdt_relaxed_rows_per_block(int64_t V);

int pdt_relaxed_gumbel(int op, int dtype, const void *param, int64_t B, int64_t p_sr, int64_t p_sv,
                       const void *in1, const void *in2, int64_t R, int64_t V, void *out, void *stream);

int pdt_relaxed_bernoulli(int op, int dtype, const void *param, int64_t B, int64_t p_sr, int64_t p_sv,
                          const void *in1, const void *in2, int64_t R, int64_t V, void *out, void *stream);

/* The backward of the methods above, one launch each (two in the parts form).  g is the gradient of the
 * method's result, dense: (R,) for the Gumbel methods that reduce (ops 2, 4, 5), (R, V) otherwise; param,
 * in1 and in2 are the forward's.  grad_param is (B, V) dense, summed over the S = R / B sample rows that
 * read each parameter row (float64 sums in one fixed order: no atomics, the same bits on every call);
 * grad_in1 is (R, V) dense, the gradient of z (op 4) or zcond (op 5).  Either may be null, not both.  The
 * arithmetic is that of the host's torch bodies in the data's type: masks that they multiply by are
 * products, masks that they select with are selects (csample: zero on the hot index, where the min guard
 * holds and where p is clamped; clog_prob: zero for a row whose b is not the one-hot of zcond's arg-max).
 * The sums over b of csample and clog_prob (log v_k, z_k) run over the nonzeros of b.
 * pdt_relaxed_backward_parts(R, B, V): P, the parts the S sample rows are cut into so that few parameter
 * rows with many samples still fill the device; P > 1 needs a workspace of
 * pdt_relaxed_backward_workspace_bytes (P * B * V float64; 0 for P == 1; PDT_E_ARG for an unknown dtype)
 * and a second launch that adds the parts in their order.  0 for an empty size or R % B != 0.
 * PDT_E_ARG, before any launch: an unknown op or dtype, op 1 (threshold has no derivative), B < 1,
 * R % B != 0, both gradients null, grad_in1 for an op other than 4 and 5, a missing g, param or in1, a
 * missing in2 for ops 3 and 5, a missing ws when P > 1.  R == 0 or V == 0 is OK (nothing to do).
 * PDT_E_TOO_LONG when V exceeds 2^31 - 513. */
int pdt_relaxed_backward_parts(int64_t R, int64_t B, int64_t V);

int64_t pdt_relaxed_backward_workspace_bytes(int dtype, int64_t R, int64_t B, int64_t V);

int pdt_relaxed_gumbel_backward(int op, int dtype, const void *g, const void *param, int64_t B, int64_t p_sr,
                                int64_t p_sv, const void *in1, const void *in2, int64_t R, int64_t V,
                                void *grad_param, void *grad_in1, void *ws, void *stream);

int pdt_relaxed_bernoulli_backward(int op, int dtype, const void *g, const void *param, int64_t B, int64_t p_sr,
                                   int64_t p_sv, const void *in1, const void *in2, int64_t R, int64_t V,
                                   void *grad_param, void *grad_in1, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sample-axis reductions of the Monte Carlo estimators (reference _mc.py:145-173, 230-233, 297-301,
 * 390-404, 530-564; _enumerate_estimator.py:68-77): the whole formula of a column in one launch, its
 * backward in one elementwise launch.  dtype 0 float32, 1 float64.  Data are (M, B), M >= 1 samples of
 * B columns.  in[6] are f, a, cz, c, lp, lq in that order, null where absent; strides[12] their element
 * strides (s_m, s_b), pair by pair (0 is allowed: c is (B,), s_m = 0).  out is (B,) dense; stats is
 * (5, B) float64, written by the forward and read by the backward (max, arg-max, mean or normaliser).
 *   kind 0  MEAN      f                 mean_m f;  is_log: logsumexp_m f - log M
 *   kind 1  SCORE     f [a [cz | c]] lp mean_m(f - a + c + cz);  is_log: with x = clamp(max_m f, lowest / 2,
 *                                       max / 2) and e(t) = exp(clamp(t - x, EPS_NINF, EPS_INF)):
 *                                       log(max(mean_m(e(f) - e(a) + e(c) + e(cz)), exp(EPS_NINF))) + x.
 *                                       lp does not enter the value; its gradient is the REINFORCE weight
 *                                       g (f - a + c) / M (is_log: the e() terms, over the floored mean)
 *   kind 2  WEIGHTED  f lp [lq]         sum_m f exp(l);  is_log: logsumexp_m(f + l);  l = lp - lq - kappa,
 *                                       mode 0 kappa = log M, 1 l = log_softmax_m(lp - lq), 2 l = lp (no lq)
 * pdt_mc_reduce_backward: g is (B,) dense; grads[6] are dense (M, B) (grads[3], of c: (B,)), null where
 * not wanted.  The clamps pass the gradient on their bounds; the path through the column maximum goes to
 * the index the forward selected (the lowest of equals).  grads[5] (lq) is written with zeros.
 * PDT_E_ARG: an unknown kind / mode / dtype, M < 1, B < 0, a missing f / lp / stats / out / g, an input
 * that the kind does not take, a gradient asked for an absent input.  B == 0 is OK (nothing to do).
 * pdt_mc_reduce_plan: the form that serves (M, B) with f read through (s_m, s_b): 0 lane = column,
 * 1 one wave per column (M >= 64, and B < 16384 or m the denser axis).  -1 for M < 1 or B < 1.
 * ------------------------------------------------------------------------------------- */
int pdt_mc_reduce_plan(int64_t M, int64_t B, int64_t s_m, int64_t s_b);

int pdt_mc_reduce(int kind, int is_log, int mode, int dtype, int64_t M, int64_t B, const void *const *in,
                  const int64_t *strides, void *out, double *stats, void *stream);

int pdt_mc_reduce_backward(int kind, int is_log, int mode, int dtype, int64_t M, int64_t B,
                           const void *const *in, const int64_t *strides, const void *g, const double *stats,
                           void *const *grads, void *stream);

/* ---------------------------------------------------------------------------------------
 * The accept / reject scan of independent Metropolis-Hastings (reference _mc.py:715-733), one lane per
 * batch column.  dtype 0 float32, 1 float64.  ratio (M, B) through (r_sm, r_sb) is log P - log Q of the
 * M proposals, ratio0 (B,) through r0_s that of the sample carried in, log_u (M, B) through (u_sm, u_sb).
 * Per column, last = ratio0, cur = -1; for n = 0 .. M - 1: if (ratio[n] - last) > log_u[n] then
 * last = ratio[n], cur = n; idx[n] = cur.  idx is (M, B) int32 dense, last (B,), last_idx (B,) int32 the
 * final cur.  A NaN rejects; a rejected -inf leaves last as it was (selected, not blended).
 * PDT_E_ARG: an unknown dtype, M < 0, B < 0, a null array that would be touched.  PDT_E_TOO_LONG: M >= 2^31.
 * ------------------------------------------------------------------------------------- */
int pdt_imh_chain(int dtype, const void *ratio, int64_t r_sm, int64_t r_sb, const void *ratio0, int64_t r0_s,
                  const void *log_u, int64_t u_sm, int64_t u_sb, int64_t M, int64_t B, int32_t *idx, void *last,
                  int32_t *last_idx, void *stream);

#ifdef __cplusplus
}
#endif
#endif
