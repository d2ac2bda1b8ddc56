// The launch layer of the step functions and BeamSearch (ctc_advance.hip, beam_advance.hip: the wave
// forms; advance_wide.hip: beams wider than a wave; beam_step.hip, beam_search_table.hip; the n-gram
// fused step in ctc_lm_step.hip): the argument blocks two files share, every launcher that one file
// defines for another, and the host arithmetic that has to agree between them.  Each defining file
// and each calling file includes it, so a signature that changes on one side only fails to compile.
#pragma once
#include "wave_select.hpp"

namespace pdt {

struct CtcAdvArgs {
  const float *ext;     int64_t ext_sn, ext_sk, ext_sv;   // (N, Kp, V)
  const float *nonext;  int64_t ne_sn, ne_sv;             // (N, V)
  const float *blank;   int64_t bl_sn;                    // (N,)
  const float *nb_prev; const float *b_prev; int64_t pb_sn, pb_sk, pbb_sn, pbb_sk;  // (N, Kp)
  const int64_t *y_prev; int64_t yp_ss, yp_sn, yp_sk;     // (S, N, Kp)
  const int64_t *last;  int64_t la_sn, la_sk;             // (N, Kp)
  const int64_t *lens;  int64_t le_sn, le_sk;             // (N, Kp)
  const uint8_t *isp;   int64_t ip_sn, ip_sa, ip_sb;      // (N, Kp, Kp) bool
  int N, Kp, V, W, S;
  // outputs, contiguous
  int64_t *y_next;      // (S + 1, N, W)
  int64_t *y_next_last, *y_next_lens, *next_src;  // (N, W)
  float *nb_next, *b_next;                        // (N, W)
  uint8_t *next_isp;                              // (N, W, W)
  uint8_t *next_nonext;                           // (N, W)
  int frame_bytes, waves_per_wg;  // LDS of the frame routine (the per-wave survivor scratch follows it)
  int ext_shared;                 // ext_sk == 0: every prefix reads the same row of extension probabilities
  // the fused form (pdt_ctc_prefix_search_advance_lm): no ext -- the language model's scores (N * Kp, V),
  // contiguous, mixed with the frame's probabilities on the fly (fusion_ext.hip's arithmetic)
  const float *lm;
  float beta;
  int valid_mixture;
};

struct BeamAdvArgs {
  const float *lpt;     int64_t lt_sn, lt_sk, lt_sv;   // log_probs_t (N, Kp, V)
  const float *lpp;     int64_t lp_sn, lp_sk;          // log_probs_prev (N, Kp)
  const int64_t *y_prev; int64_t yp_ss, yp_sn, yp_sk;  // (S, N, Kp)
  const int64_t *lens;  int64_t le_sn, le_sk;          // (N, Kp) or null
  int N, Kp, V, W, S, S_out;
  int64_t *y_next;      // (S_out, N, W)
  int64_t *y_next_lens, *next_src;  // (N, W)
  float *lp_next;                   // (N, W)
  int waves_per_wg;
};

// advance_wide.hip, called by launch_ctc_advance (ctc_advance.hip) and launch_beam_advance (beam_advance.hip)
int launch_ctc_advance_wide(CtcAdvArgs a, hipStream_t stream);
int launch_beam_advance_wide(BeamAdvArgs a, hipStream_t stream);

// The flat selections of beam_step.hip and beam_search_table.hip: eight waves per element, up to 32
// chunks of 64 candidates in the registers of each.
constexpr int kStepFlatWaves = 8, kStepFlatRegs = 32;
#ifndef PDT_BS_WAVES  // waves per SIMD the ROWS16 form is compiled for (8: 64 registers, 13 of them spilled; 6: 80)
#define PDT_BS_WAVES 8
#endif

// Waves per batch element of the kernels whose waves take the K' prefixes in turn: the power of two
// <= min(K', 8).  (ctc_advance.hip's fused form and ctc_lm_step.hip then lower it for their LDS and
// register budgets, at the call.)
static inline int step_waves(int Kp) {
  int nw = 1;
  while (nw < 8 && nw * 2 <= Kp) nw *= 2;
  return nw;
}

// The two size checks of the four step entry points: PDT_E_ARG for a size that makes no sense, then
// PDT_E_TOO_LONG for one beyond what the kernels' 32-bit index arithmetic holds.  It returns a code
// (PDT_OK when both pass), not a truth value.  An entry returns PDT_E_ARG at once and
// PDT_E_TOO_LONG only after "nothing to do" (N == 0) and its own pointer, S_out and eos tests, which
// is the order they have always had.
static inline int step_sizes_ok(int64_t N, int64_t Kp, int64_t V, int64_t width, int64_t S) {
  if (N < 0 || Kp < 1 || V < 1 || width < 1 || S < 0) return PDT_E_ARG;
  if (V >= (1 << 30) || S >= (1 << 26) || N >= (1ll << 31)) return PDT_E_TOO_LONG;
  return PDT_OK;
}

// Dynamic LDS of the list-merge kernels (beam_advance_kernel, beam_step_kernel): one survivor scratch
// per wave, the K' lists of 64 (token, value) pairs, source / token / length of the W new entries, and
// `per_prefix` more bytes per prefix -- 8 in beam_step_kernel, which also keeps whether a path has
// ended and how long its list is.
static inline size_t step_list_lds(int nw, int Kp, int W, int per_prefix) {
  return ((size_t)nw * PDT_SURV_CAP * 8 + (size_t)Kp * PDT_WAVE * 8 + (size_t)W * 12 + (size_t)Kp * per_prefix + 15) &
         ~(size_t)15;
}

}  // namespace pdt
