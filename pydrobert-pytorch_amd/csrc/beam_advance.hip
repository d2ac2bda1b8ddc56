// Step function of the beam search for gfx950, one workgroup per batch element:
// pdt_beam_search_advance -- beam_search_advance (reference _decoding.py:41-155) -- and pdt_lens_reach,
// what its caller must know before it can size y_next.
// The top-K of the K'*V candidates are selected WITHOUT materialising them.  List form: each old prefix
// gets the sorted list of its best tokens (wave_top_sorted; the waves of the workgroup share the
// prefixes), then K rounds of a wave-wide max-reduce over the list heads pick the winners in order.
// Flat form: one selection over all the candidates of the element.  Ties go to the lowest flat candidate
// index (the reference's torch.topk leaves them unspecified).  Beams wider than a wave: advance_wide.hip.
#include "step_launch.hpp"
#include "ctc_frame.hpp"
#include "row_reduce.hpp"
#include "switches.hpp"

namespace pdt {

// -------------------------------------------------------------------------------------------
// One WORKGROUP per batch element (a.waves_per_wg waves): the Kp selections are independent and
// each is a chain of round trips to HBM for a lone wave, so the waves take prefixes k = w, w + NW,
// ... in turn; wave 0 merges the lists (values are kept with the tokens: no global load in the K
// rounds); the history copy is spread over all the waves again.  N = 1024, K = 16, V = 1000:
// 0.164 ms with one wave per element doing everything -> see DESIGN.md section 4.4.
__global__ void __launch_bounds__(512, 8) beam_advance_kernel(const BeamAdvArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6), NW = a.waves_per_wg;
  const int64_t n = blockIdx.x;
  const int V = a.V, W = a.W, Kp = a.Kp, S = a.S;
  const int K = min(W, (int)min((int64_t)Kp * V, (int64_t)PDT_WAVE));  // :121
  const int M = min(V, K);
  u64 *surv = reinterpret_cast<u64 *>(smem) + (size_t)wave * PDT_SURV_CAP;  // one scratch per wave
  int *tl = reinterpret_cast<int *>(reinterpret_cast<u64 *>(smem) + (size_t)NW * PDT_SURV_CAP);
  float *tlm = reinterpret_cast<float *>(tl + Kp * PDT_WAVE);
  int *srcs = reinterpret_cast<int *>(tlm + Kp * PDT_WAVE);
  int *toks = srcs + W;
  int *plens = toks + W;

  // per-prefix lists of the best tokens, ranked by the candidate value itself -- the float32 sum
  // log_probs_prev[k] + log_probs_t[k, v] (:122) -- so that candidates whose SUMS are equal come
  // out lowest token first although their log_probs_t differ: with "lowest lane first" in the
  // merge below an exact tie goes to the lowest flat index k * V + v, the oracle's order
  for (int k = wave; k < Kp; k += NW) {
    // (rows in HBM: read once, into registers, where they are short enough -- ctc_advance_kernel's choice)
    const float *row = a.lpt + n * a.lt_sn + k * a.lt_sk;
    const float bias = a.lpp[n * a.lp_sn + k * a.lp_sk];
    const u64 tk = V > 8 * PDT_WAVE ? wave_top_sorted_regs<16, true>(row, a.lt_sv, V, M, surv, bias)
                                    : wave_top_sorted_strided<true, false, true>(row, a.lt_sv, V, M, surv, nullptr, nullptr, 1, bias);
    if (lane < M) {
      tl[k * PDT_WAVE + lane] = (int)idx_of(tk);
      tlm[k * PDT_WAVE + lane] = fkey_inv(key_of(tk));  // the sum that was ranked
    }
    wave_sync();
  }
  __syncthreads();
  if (wave == 0) {
    const bool live = lane < Kp;
    const int *mytl = tl + (live ? lane : 0) * PDT_WAVE;
    const float *mytlm = tlm + (live ? lane : 0) * PDT_WAVE;
    int ptr = 0;
    int new_src = 0, new_tok = 0;
    float new_lp = -PDT_INF;
    bool valid = false;
    for (int i = 0; i < K; ++i) {
      const bool has = live && ptr < M;
      const int tok = has ? mytl[ptr] : 0;
      const float mass = has ? mytlm[ptr] : 0.0f;  // :122
      const unsigned key = has ? fkey(mass) : 0u;
      const unsigned mx = wave_max_u32(key);
      if (mx == 0u) break;
      const int win = (int)__builtin_ctzll(__ballot(key == mx));
      const int wtok = __builtin_amdgcn_readlane(tok, win);
      const float wmass = readlane_f(mass, win);
      if (lane == i) {
        new_src = win;
        new_tok = wtok;
        new_lp = wmass;
        valid = true;
      }
      if (lane == win) ++ptr;
    }
    if (lane < W) {
      const int plen = valid ? (a.lens ? (int)a.lens[n * a.le_sn + new_src * a.le_sk] : S) : -1;
      a.lp_next[n * W + lane] = valid ? new_lp : -PDT_INF;            // :145-153 for the overflow
      a.next_src[n * W + lane] = valid ? new_src : 0;
      a.y_next_lens[n * W + lane] = valid ? plen + 1 : 0;
      srcs[lane] = valid ? new_src : -1;
      toks[lane] = new_tok;
      plens[lane] = plen;
    }
  }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < a.S_out * W; idx += NW * PDT_WAVE) {
    const int s = idx / W, i = idx - s * W;
    const int src = srcs[i];
    const int pl = plens[i];
    int64_t v;
    if (src < 0)
      v = 0;
    else if (s == pl || s >= S)  // :130/:135 the appended token row, :137 the scatter
      v = toks[i];
    else
      v = a.y_prev[(int64_t)s * a.yp_ss + n * a.yp_sn + src * a.yp_sk];
    a.y_next[((int64_t)s * a.N + n) * W + i] = v;
  }
}

// -------------------------------------------------------------------------------------------
// The FLAT form (round 5), for dense log_probs_t (the K' * V candidates of a batch element contiguous):
// the K winners are the K largest of ALL the candidates -- no per-prefix lists (sixteen 64-key sorts +
// sixteen survivor sorts per batch element: the lists were 26 of the kernel's 35 us, vector-issue bound).
// The candidates sit in the registers of the element's eight waves, flat index f = k * V + v = 64 * chunk +
// lane, up to kFlatRegs chunks per wave, every load in flight at once:
//   1. per-lane maxima -> one "column" maximum per lane over the eight waves (LDS); the K-th largest of
//      the 64 columns is a lower bound tau of the K-th largest candidate (wave 0: one 64-key sort);
//   2. every wave appends its candidates >= tau to ONE survivor list (LDS cursor), typically K .. K + 4;
//   3. wave 0 sorts them by (sum, lowest flat index first): lane i holds winner i.
// Fewer than K columns with a finite maximum (tau = -inf: finished beams, whose rows are -inf but for one
// token): the survivors are the finite candidates, and -inf candidates fill the rest in flat order, as the
// lists did.  More survivors than the list holds (top candidates crowding a few lanes): every candidate
// again from memory through the chunked top-64 merge.  Same winners, same order, same bits as the list form.
constexpr int kFlatWaves = 8, kFlatRegs = 32;

__global__ void __launch_bounds__(64 * kFlatWaves, 6) beam_advance_flat_kernel(const BeamAdvArgs a) {
  __shared__ unsigned colmax[kFlatWaves * PDT_WAVE];
  __shared__ u64 surv[PDT_SURV_CAP];
  __shared__ unsigned ctl[4];  // [0] the threshold (float bits), [1] the survivor cursor
  __shared__ int srcs[PDT_WAVE], toks[PDT_WAVE], plens[PDT_WAVE];
  int lane = lane_id();
  asm volatile("" : "+v"(lane));
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (scalar: so is everything derived)
  const int64_t n = blockIdx.x;
  const int V = a.V, W = a.W, Kp = a.Kp, S = a.S;
  const int K = min(W, (int)min((int64_t)Kp * V, (int64_t)PDT_WAVE));  // :121
  const int FV = Kp * V, total = (FV + PDT_WAVE - 1) >> 6;
  const int per = (total + kFlatWaves - 1) / kFlatWaves;  // chunks per wave, <= kFlatRegs (the launcher)
  const float *lpt = a.lpt + n * a.lt_sn;
  if (threadIdx.x == 0) ctl[1] = 0u;
  // log_probs_prev of prefix k in lane k (K' <= 64): a candidate's addend is one permute away
  const float bias_v = lane < Kp ? a.lpp[n * a.lp_sn + lane * a.lp_sk] : 0.0f;

  // ---- 1. the candidates, (log_probs_prev[k] + log_probs_t[k, v]) + 0 (:122; + 0.0f: the two zeros tie)
  const int c0 = wave * per;
  const int f0 = c0 * PDT_WAVE + lane;
  float x[kFlatRegs];
#pragma unroll
  for (int j = 0; j < kFlatRegs; ++j) {
    x[j] = -PDT_INF;  // (beyond the candidates: never a survivor, see the threshold below)
    if (j < per) {
      if ((c0 + j + 1) * PDT_WAVE <= FV)
        x[j] = lpt[f0 + j * PDT_WAVE];
      else if ((c0 + j) * PDT_WAVE < FV && f0 + j * PDT_WAVE < FV)
        x[j] = lpt[f0 + j * PDT_WAVE];
    }
  }
  // (every load in flight before the first is used: the sums in a second loop; a lane's prefix k moves on
  // by at most one per chunk, V > 64)
  float lmax = -PDT_INF;
  {
    int k = f0 / V, v = f0 - k * V;
#pragma unroll
    for (int j = 0; j < kFlatRegs; ++j) {
      if ((j & 7) == 0) __builtin_amdgcn_sched_barrier(0);  // (eight permutes ahead at most: registers)
      x[j] = (shfl_f(bias_v, k) + x[j]) + 0.0f;
      lmax = fmaxf(lmax, x[j]);
      v += PDT_WAVE;
      const bool wrap = v >= V;
      v -= wrap ? V : 0;
      k += wrap ? 1 : 0;
    }
  }
  colmax[wave * PDT_WAVE + lane] = fkey(lmax);
  __syncthreads();
  if (wave == 0) {
    unsigned cm = colmax[lane];
#pragma unroll
    for (int w = 1; w < kFlatWaves; ++w) cm = max(cm, colmax[w * PDT_WAVE + lane]);
    const unsigned sorted_max = wave_sort_desc<unsigned>(cm);
    // x >= the lowest finite float <=> x > -inf: the padding and the -inf candidates stay out
    const float tau = fmaxf(fkey_inv((unsigned)__builtin_amdgcn_readlane((int)sorted_max, K - 1)), -3.4028234664e38f);
    if (lane == 0) ctl[0] = __float_as_uint(tau);
  }
  __syncthreads();
  // ---- 2. survivors ------------------------------------------------------------------------
  const float tau = __uint_as_float(ctl[0]);
  if (__ballot(lmax >= tau)) {
#pragma unroll
    for (int j = 0; j < kFlatRegs; ++j) {
      const bool pred = x[j] >= tau;
      if (__ballot(pred)) {
        if (pred) {
          const unsigned at = atomicAdd(&ctl[1], 1u);
          if (at < PDT_SURV_CAP) surv[at] = pack_key(fkey(x[j]), (unsigned)(f0 + j * PDT_WAVE));
        }
      }
    }
  }
  __syncthreads();
  // ---- 3. the winners in order ---------------------------------------------------------------
  if (wave == 0) {
    const int count = (int)ctl[1];
    u64 tk = 0ull;
    int filled = 0;  // winners that are in tk
    if (count <= PDT_SURV_CAP) {
      tk = wave_sort_desc<u64>(lane < count ? surv[lane] : 0ull);
      filled = min(count, K);
    } else {
      // every candidate, -inf ones included, from memory
      for (int g0 = 0; g0 < FV; g0 += PDT_WAVE) {
        const int f = g0 + lane;
        const float xv = f < FV ? (a.lpp[n * a.lp_sn + (f / V) * a.lp_sk] + lpt[f]) + 0.0f : 0.0f;
        tk = wave_merge_top64(tk, f < FV ? pack_key(fkey(xv), (unsigned)f) : 0ull);
      }
      filled = K;
    }
    const int flat = (int)idx_of(tk);
    int new_src = flat / V, new_tok = flat - new_src * V;
    float new_lp = fkey_inv(key_of(tk));
    if (filled < K) {
      // tau = -inf and fewer than K finite candidates: -inf candidates in flat order behind them
      int have = filled;
      for (int g0 = 0; g0 < FV && have < K; g0 += PDT_WAVE) {
        const int f = g0 + lane;
        const int k = f / V;
        const bool is = f < FV && (a.lpp[n * a.lp_sn + k * a.lp_sk] + lpt[f]) + 0.0f == -PDT_INF;
        const u64 b = __ballot(is);
        const int rank = have + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        // winner number `rank` is this lane's candidate: hand it to lane `rank`
        if (is && rank < K) {
          srcs[rank] = k;
          toks[rank] = f - k * V;
        }
        have += __popcll(b);
      }
      wave_sync();
      if (lane >= filled && lane < K) {
        new_src = srcs[lane];
        new_tok = toks[lane];
        new_lp = -PDT_INF;
      }
      wave_sync();
    }
    if (lane < W) {
      const bool valid = lane < K;
      const int plen = valid ? (a.lens ? (int)a.lens[n * a.le_sn + new_src * a.le_sk] : S) : -1;
      a.lp_next[n * W + lane] = valid ? new_lp : -PDT_INF;  // :145-153 for the overflow
      a.next_src[n * W + lane] = valid ? new_src : 0;
      a.y_next_lens[n * W + lane] = valid ? plen + 1 : 0;
      srcs[lane] = valid ? new_src : -1;
      toks[lane] = new_tok;
      plens[lane] = plen;
    }
  }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < a.S_out * W; idx += kFlatWaves * PDT_WAVE) {
    const int s = idx / W, i = idx - s * W;
    const int src = srcs[i];
    const int pl = plens[i];
    int64_t v;
    if (src < 0)
      v = 0;
    else if (s == pl || s >= S)  // :130/:135 the appended token row, :137 the scatter
      v = toks[i];
    else
      v = a.y_prev[(int64_t)s * a.yp_ss + n * a.yp_sn + src * a.yp_sk];
    a.y_next[((int64_t)s * a.N + n) * W + i] = v;
  }
}

// What beam_search_advance's caller must know before it can size y_next (reference :133-140): does some path
// reach the history's S rows (bit 0), is some length non-zero (bit 1: invalid at S = 0).  One workgroup, one
// plain store to a word in pinned host memory the host reads after synchronising the stream -- instead of a
// reduction kernel, a device-to-host copy and the synchronisation.
__global__ void __launch_bounds__(1024) lens_reach_kernel(const int64_t *lens, const int64_t le_sn, const int64_t le_sk,
                                                         const int N, const int Kp, const int64_t S, int32_t *flag) {
  __shared__ int any_[2];
  if (threadIdx.x < 2) any_[threadIdx.x] = 0;
  __syncthreads();
  bool reach = false, nonzero = false;
  for (int64_t i = threadIdx.x; i < (int64_t)N * Kp; i += 1024) {
    const int64_t n = i / Kp, k = i - n * Kp;
    const int64_t l = lens[n * le_sn + k * le_sk];
    reach = reach || l >= S;
    nonzero = nonzero || l != 0;
  }
  if (__ballot(reach) && lane_id() == 0) any_[0] = 1;
  if (__ballot(nonzero) && lane_id() == 0) any_[1] = 1;
  __syncthreads();
  // (bit 2: the word has been written -- a system-scope store the host may poll for instead of synchronising)
  if (threadIdx.x == 0) __hip_atomic_store(flag, any_[0] | (any_[1] << 1) | 4, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int launch_beam_advance(BeamAdvArgs a, hipStream_t stream) {
  if (a.W < 1 || a.Kp < 1) return PDT_E_ARG;
  const bool force_wide = switches().step_wide != 0;
  if (force_wide || a.W > PDT_WAVE || a.Kp > PDT_WAVE) return launch_beam_advance_wide(a, stream);  // (advance_wide.hip)
  const int64_t cands = (int64_t)a.Kp * a.V;
  if (switches().step_flat != 0 && a.V > PDT_WAVE && a.lt_sv == 1 && a.lt_sk == a.V &&
      cands <= (int64_t)kFlatWaves * kFlatRegs * PDT_WAVE) {
    hipLaunchKernelGGL(beam_advance_flat_kernel, dim3((unsigned)a.N), dim3(64 * kFlatWaves), 0, stream, a);
    return (int)hipGetLastError();
  }
  const int nw = step_waves(a.Kp);
  const size_t smem = step_list_lds(nw, a.Kp, a.W, 0);
  a.waves_per_wg = nw;
  hipLaunchKernelGGL(beam_advance_kernel, dim3((unsigned)a.N), dim3(64 * nw), smem, stream, a);
  return (int)hipGetLastError();
}

}  // namespace pdt

extern "C" {

int pdt_lens_reach(const int64_t *lens, int64_t le_sn, int64_t le_sk, int64_t N, int64_t Kp, int64_t S,
                   int32_t *host_flag, void *stream) {
  using namespace pdt;
  if (N < 0 || Kp < 0 || !host_flag || N >= (1ll << 31) || Kp >= (1ll << 31)) return PDT_E_ARG;
  if (N * Kp == 0) {
    *host_flag = 4;
    return PDT_OK;
  }
  if (!lens) return PDT_E_ARG;
  hipLaunchKernelGGL(lens_reach_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lens, le_sn, le_sk, (int)N, (int)Kp, S,
                     host_flag);
  return (int)hipGetLastError();
}

int pdt_beam_search_advance(const float *log_probs_t, int64_t lt_sn, int64_t lt_sk, int64_t lt_sv,
                            int64_t N, int64_t Kp, int64_t V, int64_t width,
                            const float *log_probs_prev, int64_t lp_sn, int64_t lp_sk,
                            const int64_t *y_prev, int64_t S, int64_t yp_ss, int64_t yp_sn,
                            int64_t yp_sk, const int64_t *y_prev_lens, int64_t le_sn,
                            int64_t le_sk, int64_t S_out, int64_t *y_next, int64_t *y_next_lens,
                            float *log_probs_next, int64_t *next_src, void *stream) {
  using namespace pdt;
  const int sizes = step_sizes_ok(N, Kp, V, width, S);
  if (sizes == PDT_E_ARG || (S_out != S && S_out != S + 1)) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!log_probs_t || !log_probs_prev || (S > 0 && !y_prev) || !y_next || !y_next_lens ||
      !log_probs_next || !next_src)
    return PDT_E_ARG;
  if (sizes != PDT_OK) return sizes;
  BeamAdvArgs a{};
  a.lpt = log_probs_t; a.lt_sn = lt_sn; a.lt_sk = lt_sk; a.lt_sv = lt_sv;
  a.lpp = log_probs_prev; a.lp_sn = lp_sn; a.lp_sk = lp_sk;
  a.y_prev = y_prev; a.yp_ss = yp_ss; a.yp_sn = yp_sn; a.yp_sk = yp_sk;
  a.lens = y_prev_lens; a.le_sn = le_sn; a.le_sk = le_sk;
  a.N = (int)N; a.Kp = (int)Kp; a.V = (int)V; a.W = (int)width; a.S = (int)S; a.S_out = (int)S_out;
  a.y_next = y_next; a.y_next_lens = y_next_lens; a.lp_next = log_probs_next; a.next_src = next_src;
  return launch_beam_advance(a, (hipStream_t)stream);
}

}  // extern "C"
