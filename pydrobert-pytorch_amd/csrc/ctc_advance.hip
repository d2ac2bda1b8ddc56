// Step function of the CTC prefix search for gfx950, one workgroup per batch element:
// pdt_ctc_prefix_search_advance -- ctc_prefix_search_advance (reference _decoding.py:636-934) with
// arbitrary per-prefix extension probabilities (language-model fusion) and dense (S, N, K') histories,
// as the reference's signature requires -- and pdt_ctc_prefix_search_advance_lm, which mixes a language
// model's scores into the frame's probabilities itself.
// The top-K of the K'*V + K' candidates are selected WITHOUT materialising them: each old prefix gets
// the sorted list of its best tokens (wave_top_sorted; the waves of the workgroup share the prefixes),
// then the frame routine (ctc_frame.hpp) merges the list heads.  Ties go to the lowest flat candidate
// index (the reference's torch.topk leaves them unspecified).  Beams wider than 32: advance_wide.hip.
#include "step_launch.hpp"
#include "ctc_frame.hpp"
#include "row_reduce.hpp"
#include "switches.hpp"

#ifndef PDT_FUSED_STEP_WAVES
#define PDT_FUSED_STEP_WAVES 4
#endif

namespace pdt {

// One WORKGROUP per batch element (a.waves_per_wg waves).  The Kp per-prefix selections over the
// dense extension probabilities are independent and each is a chain of round trips to HBM for a
// lone wave: the waves take prefixes k = w, w + NW, ... in turn (every wave with its own survivor
// scratch), wave 0 runs the frame on the finished lists, all waves copy the histories.
// FUSED (round 5, pdt_ctc_prefix_search_advance_lm): the extension probabilities are never written --
// a wave reads its prefix's row of language-model scores once (registers), reduces it, mixes it with the
// frame's probabilities (the arithmetic of fusion_ext.hip, to the bit) into a row of its own in LDS and
// selects from there; what the frame reads of a row besides its list -- the entries at the prefixes' last
// tokens -- goes to a K' x K' table (DenseCtx::etab).  One kernel and 4 V bytes per prefix instead of two
// kernels and 12 V: fusion_ext 43 us + step 45 us -> see DESIGN.md section 4.4.
template <bool FUSED>
__global__ void __launch_bounds__(512, FUSED ? 4 : 8) ctc_advance_kernel(const CtcAdvArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6), NW = a.waves_per_wg;
  const int64_t n = blockIdx.x;
  const int V = a.V, W = a.W, Kp = a.Kp, S = a.S;
  float *p = reinterpret_cast<float *>(smem);
  FrameLds L;
  L.carve(smem + (size_t)((V + 1 + 3) & ~3) * 4, V, W, Kp, true);
  int *srcs = reinterpret_cast<int *>(L.surv);  // reused after the frame
  u64 *my_surv = reinterpret_cast<u64 *>(smem + a.frame_bytes) + (size_t)wave * PDT_SURV_CAP;

  const int M = ctc_list_len(V, W, Kp);
  // (prefixes that share ONE row of extension probabilities -- the search without a language model hands
  // over nonext.unsqueeze(1).expand(N, K', V), stride 0 -- share one list: built once, copied below)
  const int n_lists = FUSED ? 0 : (a.ext_shared ? 1 : Kp);
  float *etab = nullptr;
  if constexpr (FUSED) {
    const int row_floats = (V + 3) & ~3;
    float *rows_w = reinterpret_cast<float *>(smem + a.frame_bytes + (size_t)NW * PDT_SURV_CAP * 8);
    etab = rows_w;  // [Kp x Kp]; behind it ONE row for the rare fall-back below (wave 0's turn only)
    float *row = etab + ((Kp * Kp + 3) & ~3);
    (void)row_floats;
    const float keep = 1.0f - a.beta, beta = a.beta;
    const bool vm = a.valid_mixture != 0;
    const float scale = vm ? 1.0f - a.blank[n * a.bl_sn] : 0.0f;
    const float *pc = a.nonext + n * a.ne_sn;
    const int lastc = lane < Kp ? (int)min(max(a.last[n * a.la_sn + lane * a.la_sk], (int64_t)0), (int64_t)(V - 1)) : 0;
    const float p_last = lane < Kp ? pc[(int64_t)lastc * a.ne_sv] : 0.0f;
    unsigned overflowed = 0u;  // bit k / NW (wave-uniform): rows of this wave whose survivor buffer overflowed
    // the frame's probabilities are the same for every row of the element: once, in registers
    float pr[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = lane + i * PDT_WAVE;
      pr[i] = (i * PDT_WAVE < V && v < V) ? pc[(int64_t)v * a.ne_sv] : 0.0f;
    }
    for (int k = wave; k < Kp; k += NW) {
      const float *x = a.lm + (n * Kp + k) * (int64_t)V;
      float r[16];
      const RowStats st = row_stats<false, true, 16>(x, 1, V, r);  // (V <= 1024: the launcher)
      const float log_sum = logf(st.sum);
      auto mix = [&](const float p, const float xv) {
        if (vm) {
          const float lm_p = (expf(xv - st.mx) / st.sum) * scale;
          return keep * p + beta * lm_p;
        }
        return p * expf(beta * ((xv - st.mx) - log_sum));
      };
      // what the frame reads of this row besides its list: the entries at the prefixes' last tokens
      if (lane < Kp) etab[k * Kp + lane] = mix(p_last, x[lastc]);
      unsigned keys[16];  // ordering keys of the mixed values (every one >= +0), 0 beyond the row
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int v = lane + i * PDT_WAVE;
        keys[i] = 0u;
        if (i * PDT_WAVE < V && v < V) keys[i] = fkey_nonneg(mix(pr[i], r[i]));
      }
      u64 tk;
      if (wave_top_sorted_keys<16>(keys, M, my_surv, tk)) {
        if (lane < M) {
          L.tl_tok[k * PDT_WAVE + lane] = (int)idx_of(tk);
          L.tl_p[k * PDT_WAVE + lane] = fkey_nonneg_inv(key_of(tk));
        }
      } else {
        overflowed |= 1u << (k / NW);
      }
      wave_sync();
    }
    // heavy ties in a row (more survivors than the buffer holds): the row through LDS and the chunked merge,
    // one wave at a time -- they share the one LDS row
    for (int w = 0; w < NW; ++w) {
      if (__syncthreads_or(wave == w && overflowed != 0u)) {
        if (wave == w) {
          for (int k = wave; k < Kp; k += NW) {
            if (!((overflowed >> (k / NW)) & 1u)) continue;
            const float *x = a.lm + (n * Kp + k) * (int64_t)V;
            float r[16];
            const RowStats st = row_stats<false, true, 16>(x, 1, V, r);
            const float log_sum = logf(st.sum);
            for (int v = lane; v < V; v += PDT_WAVE) {
              const float p = pc[(int64_t)v * a.ne_sv], xv = x[v];
              row[v] = vm ? keep * p + beta * ((expf(xv - st.mx) / st.sum) * scale) : p * expf(beta * ((xv - st.mx) - log_sum));
            }
            wave_sync();
            const u64 tk = wave_top_sorted<false, true>(row, V, M, my_surv);
            if (lane < M) {
              L.tl_tok[k * PDT_WAVE + lane] = (int)idx_of(tk);
              L.tl_p[k * PDT_WAVE + lane] = fkey_nonneg_inv(key_of(tk));
            }
            wave_sync();
          }
        }
        __syncthreads();
      }
    }
  }
  for (int k = wave; k < n_lists; k += NW) {
    // (rows of 513 .. 1024 elements are read once, into 16 registers per lane: 0.056 -> 0.047 ms at
    // V = 1000; shorter rows measured no better that way, longer ones are streamed twice)
    const float *xk = a.ext + n * a.ext_sn + k * a.ext_sk;
    const u64 tk = V > 8 * PDT_WAVE ? wave_top_sorted_regs<16>(xk, a.ext_sv, V, M, my_surv)
                                    : wave_top_sorted_strided<true>(xk, a.ext_sv, V, M, my_surv);
    if (lane < M) {
      L.tl_tok[k * PDT_WAVE + lane] = (int)idx_of(tk);
      L.tl_p[k * PDT_WAVE + lane] = fkey_inv(key_of(tk));
    }
    wave_sync();
  }
  for (int v = (int)threadIdx.x; v < V; v += NW * PDT_WAVE) p[v] = a.nonext[n * a.ne_sn + v * a.ne_sv];
  if (threadIdx.x == 0) p[V] = a.blank[n * a.bl_sn];
  __syncthreads();
  if (!FUSED && n_lists < Kp) {
    for (int idx = PDT_WAVE + (int)threadIdx.x; idx < Kp * PDT_WAVE; idx += NW * PDT_WAVE) {
      L.tl_tok[idx] = L.tl_tok[idx & (PDT_WAVE - 1)];
      L.tl_p[idx] = L.tl_p[idx & (PDT_WAVE - 1)];
    }
    __syncthreads();
  }

  DenseCtx dc;
  dc.ext = FUSED ? nullptr : a.ext + n * a.ext_sn;
  dc.ext_sk = FUSED ? 0 : a.ext_sk;
  dc.ext_sv = FUSED ? 0 : a.ext_sv;
  if constexpr (FUSED) {
    dc.etab = etab;
    dc.etab_stride = Kp;
  }
  dc.y_prev = a.y_prev + n * a.yp_sn;
  dc.yp_ss = a.yp_ss;
  dc.yp_sk = a.yp_sk;
  dc.S = S;
  dc.lists_ready = 1;
  if (wave == 0) {
    Beam bm;
    bm.nb = lane < Kp ? a.nb_prev[n * a.pb_sn + lane * a.pb_sk] : -PDT_INF;
    bm.b = lane < Kp ? a.b_prev[n * a.pbb_sn + lane * a.pbb_sk] : -PDT_INF;
    bm.last = lane < Kp ? (int)min(max(a.last[n * a.la_sn + lane * a.la_sk], (int64_t)-1), (int64_t)V) : 0;
    bm.len = lane < Kp ? (int)a.lens[n * a.le_sn + lane * a.le_sk] : 0;
    bm.node = -1;
    unsigned m = 0u;
    if (lane < Kp)
      for (int b = 0; b < Kp; ++b)
        if (a.isp[n * a.ip_sn + lane * a.ip_sa + b * a.ip_sb]) m |= 1u << b;
    bm.isp = m;
    CtcArgs dummy{};
    dummy.N = a.N;
    int new_src, new_tok, new_kind;
#ifdef PDT_STAMPS
    unsigned pdt_stamp_acc[14] = {0};  // wave-uniform: scalar registers
#endif
    ctc_frame<true>(bm, p, 1.0f, V, W, Kp, 0, n, dummy, dc, L, new_src, new_tok, new_kind PDT_STAMP_ARG);

    // ---- outputs (:855-934) --------------------------------------------------------------
    if (lane < W) {
      const bool valid = new_kind >= 0;
      a.y_next_last[n * W + lane] = bm.last;
      a.y_next_lens[n * W + lane] = bm.len;
      a.nb_next[n * W + lane] = bm.nb;
      a.b_next[n * W + lane] = bm.b;
      a.next_src[n * W + lane] = valid ? new_src : 0;
      a.next_nonext[n * W + lane] = (uint8_t)(new_kind == 2);
      for (int b = 0; b < W; ++b) a.next_isp[(n * W + lane) * W + b] = (uint8_t)((bm.isp >> b) & 1u);
      srcs[lane] = valid ? new_src : -1;
      L.info[lane] = bm.len;        // the frame's scratch is free again: per-entry length and
      L.info[W + lane] = new_kind;  // kind for the copy loop
      // the new token sits right after the source prefix (:862-864)
      if (valid && new_kind != 2) a.y_next[((int64_t)(bm.len - 1) * a.N + n) * W + lane] = new_tok;
    }
  }
  __syncthreads();
  // history rows of the source prefix, below the position just written
  for (int idx = (int)threadIdx.x; idx < (S + 1) * W; idx += NW * PDT_WAVE) {
    const int s = idx / W, i = idx - s * W;
    const int src = srcs[i];
    const int len_i = L.info[i], kind_i = L.info[W + i];
    const bool ext_i = kind_i == 0 || kind_i == 1;
    const int plen = len_i - (ext_i ? 1 : 0);
    if (src < 0)
      a.y_next[((int64_t)s * a.N + n) * W + i] = 0;
    else if (!(ext_i && s == plen))
      a.y_next[((int64_t)s * a.N + n) * W + i] = s < S ? dc.y_prev[(int64_t)s * dc.yp_ss + src * dc.yp_sk] : 0;
  }
}

int launch_ctc_advance(CtcAdvArgs a, hipStream_t stream) {
  if (a.W < 1 || a.Kp < 1) return PDT_E_ARG;
  const bool force_wide = switches().step_wide != 0;
  if (a.lm && (force_wide || a.W > kMaxWidth || a.Kp > kMaxWidth || a.V > 16 * PDT_WAVE)) return PDT_E_UNSUPPORTED;
  if (force_wide || a.W > kMaxWidth || a.Kp > kMaxWidth) return launch_ctc_advance_wide(a, stream);  // (advance_wide.hip)
  int nw = step_waves(a.Kp);
  size_t frame = (size_t)((a.V + 1 + 3) & ~3) * 4 + FrameLds::bytes(a.V, a.W, a.Kp, true);
  frame = (frame + 15) & ~(size_t)15;
  const bool fused = a.lm != nullptr;
  // (the fused form needs ~110 vector registers: four waves per SIMD.  Four-wave workgroups keep every batch
  // element of N = 1024 resident at once -- four rows per wave -- where eight-wave ones run in two rounds)
  if (fused && nw > PDT_FUSED_STEP_WAVES) nw = PDT_FUSED_STEP_WAVES;
  size_t smem = frame + (size_t)nw * PDT_SURV_CAP * 8;  // + one survivor scratch per wave
  if (fused) smem += ((size_t)((a.V + 3) & ~3) + (size_t)((a.Kp * a.Kp + 3) & ~3)) * 4;  // + the K' x K' table, one mixed row (ties)
  if (smem > 160 * 1024) return fused ? PDT_E_UNSUPPORTED : PDT_E_TOO_LONG;
  a.waves_per_wg = nw;
  a.frame_bytes = (int)frame;
  a.ext_shared = (!fused && a.Kp > 1 && a.ext_sk == 0 && switches().step_flat != 0) ? 1 : 0;
  if (fused) {
    if (const int rc = set_lds(ctc_advance_kernel<true>, smem)) return rc;
    hipLaunchKernelGGL(ctc_advance_kernel<true>, dim3((unsigned)a.N), dim3(64 * nw), smem, stream, a);
  } else {
    if (const int rc = set_lds(ctc_advance_kernel<false>, smem)) return rc;
    hipLaunchKernelGGL(ctc_advance_kernel<false>, dim3((unsigned)a.N), dim3(64 * nw), smem, stream, a);
  }
  return (int)hipGetLastError();
}

// The fields the two entry points share (each then sets its own three: the extension probabilities and
// their strides, or the language model's scores and the mixture).
static CtcAdvArgs ctc_adv_args(
    const float *nonext, int64_t ne_sn, int64_t ne_sv, const float *blank, int64_t bl_sn, int64_t N, int64_t Kp,
    int64_t V, int64_t width, const float *nb_prev, int64_t nb_sn, int64_t nb_sk, const float *b_prev, int64_t b_sn,
    int64_t b_sk, const int64_t *y_prev, int64_t S, int64_t yp_ss, int64_t yp_sn, int64_t yp_sk,
    const int64_t *y_prev_last, int64_t la_sn, int64_t la_sk, const int64_t *y_prev_lens, int64_t le_sn,
    int64_t le_sk, const uint8_t *prev_is_prefix, int64_t ip_sn, int64_t ip_sa, int64_t ip_sb, int64_t *y_next,
    int64_t *y_next_last, int64_t *y_next_lens, float *nb_next, float *b_next, uint8_t *next_is_prefix,
    int64_t *next_src, uint8_t *next_is_nonext) {
  CtcAdvArgs a{};
  a.nonext = nonext; a.ne_sn = ne_sn; a.ne_sv = ne_sv;
  a.blank = blank; a.bl_sn = bl_sn;
  a.nb_prev = nb_prev; a.pb_sn = nb_sn; a.pb_sk = nb_sk;
  a.b_prev = b_prev; a.pbb_sn = b_sn; a.pbb_sk = b_sk;
  a.y_prev = y_prev; a.yp_ss = yp_ss; a.yp_sn = yp_sn; a.yp_sk = yp_sk;
  a.last = y_prev_last; a.la_sn = la_sn; a.la_sk = la_sk;
  a.lens = y_prev_lens; a.le_sn = le_sn; a.le_sk = le_sk;
  a.isp = prev_is_prefix; a.ip_sn = ip_sn; a.ip_sa = ip_sa; a.ip_sb = ip_sb;
  a.N = (int)N; a.Kp = (int)Kp; a.V = (int)V; a.W = (int)width; a.S = (int)S;
  a.y_next = y_next; a.y_next_last = y_next_last; a.y_next_lens = y_next_lens;
  a.next_src = next_src; a.nb_next = nb_next; a.b_next = b_next;
  a.next_isp = next_is_prefix; a.next_nonext = next_is_nonext;
  return a;
}

}  // namespace pdt

extern "C" {

int pdt_ctc_prefix_search_advance(
    const float *ext, int64_t ext_sn, int64_t ext_sk, int64_t ext_sv, const float *nonext,
    int64_t ne_sn, int64_t ne_sv, const float *blank, int64_t bl_sn, int64_t N, int64_t Kp,
    int64_t V, int64_t width, const float *nb_prev, int64_t nb_sn, int64_t nb_sk,
    const float *b_prev, int64_t b_sn, int64_t b_sk, const int64_t *y_prev, int64_t S,
    int64_t yp_ss, int64_t yp_sn, int64_t yp_sk, const int64_t *y_prev_last, int64_t la_sn,
    int64_t la_sk, const int64_t *y_prev_lens, int64_t le_sn, int64_t le_sk,
    const uint8_t *prev_is_prefix, int64_t ip_sn, int64_t ip_sa, int64_t ip_sb, int64_t *y_next,
    int64_t *y_next_last, int64_t *y_next_lens, float *nb_next, float *b_next,
    uint8_t *next_is_prefix, int64_t *next_src, uint8_t *next_is_nonext, void *stream) {
  using namespace pdt;
  const int sizes = step_sizes_ok(N, Kp, V, width, S);
  if (sizes == PDT_E_ARG) return sizes;
  if (N == 0) return PDT_OK;
  if (!ext || !nonext || !blank || !nb_prev || !b_prev || !y_prev_last || !y_prev_lens ||
      !prev_is_prefix || (S > 0 && !y_prev) || !y_next || !y_next_last || !y_next_lens ||
      !nb_next || !b_next || !next_is_prefix || !next_src || !next_is_nonext)
    return PDT_E_ARG;
  if (sizes != PDT_OK) return sizes;
  CtcAdvArgs a = ctc_adv_args(nonext, ne_sn, ne_sv, blank, bl_sn, N, Kp, V, width, nb_prev, nb_sn, nb_sk, b_prev, b_sn, b_sk,
                              y_prev, S, yp_ss, yp_sn, yp_sk, y_prev_last, la_sn, la_sk, y_prev_lens, le_sn, le_sk,
                              prev_is_prefix, ip_sn, ip_sa, ip_sb, y_next, y_next_last, y_next_lens, nb_next, b_next,
                              next_is_prefix, next_src, next_is_nonext);
  a.ext = ext; a.ext_sn = ext_sn; a.ext_sk = ext_sk; a.ext_sv = ext_sv;
  return launch_ctc_advance(a, (hipStream_t)stream);
}

int pdt_ctc_prefix_search_advance_lm(
    const float *lm_log_probs, float beta, int valid_mixture, const float *nonext, int64_t ne_sn,
    int64_t ne_sv, const float *blank, int64_t bl_sn, int64_t N, int64_t Kp, int64_t V, int64_t width,
    const float *nb_prev, int64_t nb_sn, int64_t nb_sk, const float *b_prev, int64_t b_sn, int64_t b_sk,
    const int64_t *y_prev, int64_t S, int64_t yp_ss, int64_t yp_sn, int64_t yp_sk,
    const int64_t *y_prev_last, int64_t la_sn, int64_t la_sk, const int64_t *y_prev_lens, int64_t le_sn,
    int64_t le_sk, const uint8_t *prev_is_prefix, int64_t ip_sn, int64_t ip_sa, int64_t ip_sb,
    int64_t *y_next, int64_t *y_next_last, int64_t *y_next_lens, float *nb_next, float *b_next,
    uint8_t *next_is_prefix, int64_t *next_src, uint8_t *next_is_nonext, void *stream) {
  using namespace pdt;
  const int sizes = step_sizes_ok(N, Kp, V, width, S);
  if (sizes == PDT_E_ARG) return sizes;
  if (N == 0) return PDT_OK;
  if (!lm_log_probs || !nonext || !blank || !nb_prev || !b_prev || !y_prev_last || !y_prev_lens ||
      !prev_is_prefix || (S > 0 && !y_prev) || !y_next || !y_next_last || !y_next_lens ||
      !nb_next || !b_next || !next_is_prefix || !next_src || !next_is_nonext)
    return PDT_E_ARG;
  if (sizes != PDT_OK) return sizes;
  CtcAdvArgs a = ctc_adv_args(nonext, ne_sn, ne_sv, blank, bl_sn, N, Kp, V, width, nb_prev, nb_sn, nb_sk, b_prev, b_sn, b_sk,
                              y_prev, S, yp_ss, yp_sn, yp_sk, y_prev_last, la_sn, la_sk, y_prev_lens, le_sn, le_sk,
                              prev_is_prefix, ip_sn, ip_sa, ip_sb, y_next, y_next_last, y_next_lens, nb_next, b_next,
                              next_is_prefix, next_src, next_is_nonext);
  a.lm = lm_log_probs; a.beta = beta; a.valid_mixture = valid_mixture;
  return launch_ctc_advance(a, (hipStream_t)stream);
}

}  // extern "C"
