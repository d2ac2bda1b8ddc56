// Random walks on a language model's outputs (reference _decoding.py:1207-1283 and :1286-1513), every token
// drawn by the one sampling rule of row_sample.hpp (sample_row) from a uniform the caller draws with torch's
// generator:
//   pdt_random_walk_advance   the step function random_walk_advance: sample, log-probability, the history
//                             copied into y_next with the token appended / scattered at the lengths
//   pdt_random_walk_step      one iteration of RandomWalk.forward around any language model (the default
//                             hook): log_softmax of the model's scores (never materialised: a row's maximum
//                             and log-sum-exp), the eos rule, the draw and the walk's state, in ONE kernel
//   pdt_random_walk_table     a chunk of iterations of the same walk over the dense context table of an
//                             n-gram model in ONE launch, each walk's state in registers across the chunk
// One wave per walk.  A launch reports to two int32 words of the caller: `ctl` (device, zeroed once; the
// workgroups gather into it and the last one zeroes it again) and `host` (pinned host memory, read by the
// host once the launch is done): host[1] = walks still live, host[2] = the longest walk (table),
// host[0] = PDT_WALK_DONE | the PDT_WALK_* bits, stored last (release, system scope) -- the host polls it.
#include "row_sample.hpp"

namespace pdt {

constexpr int kWalkWaves = 4;  // walks per workgroup

// every workgroup adds its part; the last one to finish writes the caller's host words and re-zeroes ctl
__device__ __forceinline__ void walk_report(int32_t *ctl, int32_t *host, int live, int bits, int maxlen) {
  __shared__ int part[3];
  if (threadIdx.x == 0) part[0] = part[1] = part[2] = 0;
  __syncthreads();
  if (lane_id() == 0) {
    if (live) atomicAdd(&part[0], live);
    if (bits) atomicOr(&part[1], bits);
    if (maxlen) atomicMax(&part[2], maxlen);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (part[0]) atomicAdd(&ctl[0], part[0]);
  if (part[1]) atomicOr(&ctl[1], part[1]);
  if (part[2]) atomicMax(&ctl[3], part[2]);
  __threadfence();
  if (atomicAdd(&ctl[2], 1) != (int)gridDim.x - 1) return;
  __threadfence();
  const int l = atomicExch(&ctl[0], 0), b = atomicExch(&ctl[1], 0), m = atomicExch(&ctl[3], 0);
  atomicExch(&ctl[2], 0);
  __hip_atomic_store(&host[1], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host[2], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host[0], b | PDT_WALK_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct WalkAdvArgs {
  const float *lpt; int64_t lt_sn, lt_sv;     // log_probs_t (N, V)
  const float *u; int64_t u_sn;               // (N,)
  const float *lpp; int64_t lp_sn;            // log_probs_prev (N,)
  const int64_t *y_prev; int64_t yp_ss, yp_sn;  // (S, N)
  const int64_t *lens; int64_t le_sn;         // (N,) or null
  int N, V;
  int64_t S;
  int64_t *y_next;                            // (S + 1, N) contiguous
  float *lp_next;                             // (N,)
  int32_t *ctl, *host;
};

// where walk n's token goes besides row S (reference :1272-1279: y_next.scatter(0, y_prev_lens, y_t)); S: nowhere
// else.  A length outside [0, S] is flagged and writes nothing.
__device__ __forceinline__ int64_t advance_pos(const WalkAdvArgs &a, int n, int &bits) {
  if (!a.lens || a.S == 0) return a.S;
  const int64_t l = a.lens[(int64_t)n * a.le_sn];
  if (l >= a.S) bits |= PDT_WALK_REACH;
  if (l < 0 || l > a.S) {
    bits |= PDT_WALK_BAD_LENS;
    return a.S;
  }
  return l;
}

__global__ void __launch_bounds__(64 * kWalkWaves) random_walk_advance_kernel(const WalkAdvArgs a) {
  const int n = (int)(blockIdx.x * kWalkWaves + (threadIdx.x >> 6));
  int bits = 0;
  if (n < a.N) {
    const float *row = a.lpt + (int64_t)n * a.lt_sn;
    float mx, lse;
    row_log_softmax_stats(row, a.lt_sv, a.V, mx, lse);
    int tok = sample_row(row, a.lt_sv, a.V, mx, lse, a.u[(int64_t)n * a.u_sn]);
    if (tok < 0) {
      bits |= PDT_WALK_INVALID;
      tok = 0;
    }
    const int64_t pos = advance_pos(a, n, bits);
    if (lane_id() == 0) {
      a.lp_next[n] = a.lpp[(int64_t)n * a.lp_sn] + row[(int64_t)tok * a.lt_sv];
      a.y_next[a.S * a.N + n] = tok;  // (the row cat appends; dropped by the caller when y does not grow)
      if (pos != a.S) a.y_next[pos * a.N + n] = tok;
    }
  }
  // the history, every thread of the grid: y_next[s, n] = y_prev[s, n] for s < S but the scatter's row
  const int64_t total = a.S * a.N, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t s = i / a.N;
    const int m = (int)(i - s * a.N);
    int ignored = 0;
    if (s != advance_pos(a, m, ignored)) a.y_next[i] = a.y_prev[s * a.yp_ss + (int64_t)m * a.yp_sn];
  }
  walk_report(a.ctl, a.host, 0, bits, 0);
}

struct WalkStepArgs {
  const float *sc; int64_t sc_sn, sc_sv;  // the model's scores (N, V), any normalisation
  const float *u;                         // (N,) contiguous
  int N, V;
  int64_t *y_t;                           // row t of y: (N,) contiguous
  int64_t *lens; uint8_t *ended; float *lp;  // (N,) each, contiguous: the walks' state
  int has_eos, eos;
  int32_t *ctl, *host;
};

__global__ void __launch_bounds__(64 * kWalkWaves) random_walk_step_kernel(const WalkStepArgs a) {
  const int n = (int)(blockIdx.x * kWalkWaves + (threadIdx.x >> 6));
  int bits = 0, live = 0;
  if (n < a.N) {
    int tok = a.eos;
    if (!(a.has_eos && a.ended[n])) {  // (an ended walk repeats eos at no cost, :1483-1492)
      const float *row = a.sc + (int64_t)n * a.sc_sn;
      float mx, lse;
      row_log_softmax_stats(row, a.sc_sv, a.V, mx, lse);
      tok = sample_row(row, a.sc_sv, a.V, mx, lse, a.u[n]);
      if (tok < 0) {
        bits |= PDT_WALK_INVALID;
        tok = 0;
      }
      const float x_tok = row[(int64_t)tok * a.sc_sv];
      const bool ends = a.has_eos && tok == a.eos;
      live = !ends;
      if (lane_id() == 0) {
        a.lp[n] = walk_lp_add(a.lp[n], x_tok, mx, lse);
        a.lens[n] += 1;
        a.ended[n] = ends;
      }
    }
    if (lane_id() == 0) a.y_t[n] = tok;
  }
  walk_report(a.ctl, a.host, live, bits, 0);
}

struct WalkTableArgs {
  const float *table; int64_t tb_sr;  // (R, V), unit element stride
  const float *stats;                 // (R, 2): pdt_row_log_softmax_stats of the table
  int64_t R, U;                       // rows (U^(n-1)), symbols per context position
  const float *u;                     // (C, N) contiguous
  int N, V, C;
  int64_t *y;                         // (C, N) contiguous: rows t .. t + C - 1 of the walk's y
  int64_t *ctx, *lens; uint8_t *ended; float *lp;  // (N,) each: the state, read at the start, written at the end
  int has_eos, eos;
  int32_t *ctl, *host;
};

// The walk's state stays in registers for the chunk; an iteration reads the context row's statistics and
// about half of the row itself.  Tables are at most 64 MiB: they stay in the Infinity Cache.
__global__ void __launch_bounds__(64 * kWalkWaves) random_walk_table_kernel(const WalkTableArgs a) {
  const int n = (int)(blockIdx.x * kWalkWaves + (threadIdx.x >> 6));
  int bits = 0, live = 0, maxlen = 0;
  if (n < a.N) {
    int64_t r = a.ctx[n], len = a.lens[n];
    bool ended = a.has_eos && a.ended[n];
    float lp = a.lp[n];
    if (r < 0 || r >= a.R) {  // (a state the host did not start from the table's rows: nothing is read)
      bits |= PDT_WALK_INVALID;
      ended = true;
    }
    for (int c = 0; c < a.C; ++c) {
      int tok = a.eos;
      if (!ended) {
        const float *row = a.table + r * a.tb_sr;
        const float mx = a.stats[2 * r], lse = a.stats[2 * r + 1];
        tok = sample_row(row, 1, a.V, mx, lse, a.u[(int64_t)c * a.N + n]);
        if (tok < 0) {
          bits |= PDT_WALK_INVALID;
          ended = true;
          tok = 0;
        } else {
          lp = walk_lp_add(lp, row[tok], mx, lse);
          len += 1;
          ended = a.has_eos && tok == a.eos;
          r = (r * a.U + tok) % a.R;
        }
      }
      if (lane_id() == 0) a.y[(int64_t)c * a.N + n] = tok;
    }
    if (lane_id() == 0) {
      a.ctx[n] = r;
      a.lens[n] = len;
      a.ended[n] = ended;
      a.lp[n] = lp;
    }
    live = !(bits & PDT_WALK_INVALID) && !ended;
    maxlen = len > 0x7fffffff ? 0x7fffffff : (int)len;
  }
  walk_report(a.ctl, a.host, live, bits, maxlen);
}

static unsigned walk_blocks(int64_t N) { return (unsigned)((N + kWalkWaves - 1) / kWalkWaves); }

}  // namespace pdt

extern "C" {

int pdt_random_walk_advance(const float *log_probs_t, int64_t lt_sn, int64_t lt_sv, int64_t N, int64_t V,
                            const float *u, int64_t u_sn, const float *log_probs_prev, int64_t lp_sn,
                            const int64_t *y_prev, int64_t S, int64_t yp_ss, int64_t yp_sn,
                            const int64_t *y_prev_lens, int64_t le_sn, int64_t *y_next, float *log_probs_next,
                            int32_t *ctl, int32_t *host_words, void *stream) {
  using namespace pdt;
  if (N < 0 || V < 1 || S < 0) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!log_probs_t || !u || !log_probs_prev || (S > 0 && !y_prev) || !y_next || !log_probs_next || !ctl ||
      !host_words)
    return PDT_E_ARG;
  if (V >= (1 << 30) || N >= (1ll << 31) || S >= (1ll << 40) / N) return PDT_E_TOO_LONG;
  WalkAdvArgs a{};
  a.lpt = log_probs_t; a.lt_sn = lt_sn; a.lt_sv = lt_sv;
  a.u = u; a.u_sn = u_sn; a.lpp = log_probs_prev; a.lp_sn = lp_sn;
  a.y_prev = y_prev; a.yp_ss = yp_ss; a.yp_sn = yp_sn; a.lens = y_prev_lens; a.le_sn = le_sn;
  a.N = (int)N; a.V = (int)V; a.S = S;
  a.y_next = y_next; a.lp_next = log_probs_next; a.ctl = ctl; a.host = host_words;
  hipLaunchKernelGGL(random_walk_advance_kernel, dim3(walk_blocks(N)), dim3(64 * kWalkWaves), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int pdt_random_walk_step(const float *scores, int64_t sc_sn, int64_t sc_sv, int64_t N, int64_t V, const float *u,
                         int has_eos, int64_t eos, int64_t *y_t, int64_t *lens, uint8_t *ended, float *log_probs,
                         int32_t *ctl, int32_t *host_words, void *stream) {
  using namespace pdt;
  if (N < 0 || V < 1) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!scores || !u || !y_t || !lens || !ended || !log_probs || !ctl || !host_words) return PDT_E_ARG;
  if (has_eos && (eos < 0 || eos >= V)) return PDT_E_ARG;
  if (V >= (1 << 30) || N >= (1ll << 31)) return PDT_E_TOO_LONG;
  WalkStepArgs a{};
  a.sc = scores; a.sc_sn = sc_sn; a.sc_sv = sc_sv; a.u = u;
  a.N = (int)N; a.V = (int)V; a.y_t = y_t; a.lens = lens; a.ended = ended; a.lp = log_probs;
  a.has_eos = has_eos; a.eos = has_eos ? (int)eos : 0; a.ctl = ctl; a.host = host_words;
  hipLaunchKernelGGL(random_walk_step_kernel, dim3(walk_blocks(N)), dim3(64 * kWalkWaves), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

int pdt_random_walk_table(const float *table, int64_t tb_sr, int64_t R, int64_t U, int64_t V, const float *row_stats,
                          const float *u, int64_t N, int64_t C, int has_eos, int64_t eos, int64_t *y, int64_t *ctx,
                          int64_t *lens, uint8_t *ended, float *log_probs, int32_t *ctl, int32_t *host_words,
                          void *stream) {
  using namespace pdt;
  if (N < 0 || C < 0 || V < 1 || R < 1 || U < 1 || tb_sr < V) return PDT_E_ARG;
  if (N == 0 || C == 0) return PDT_OK;
  if (!table || !row_stats || !u || !y || !ctx || !lens || !ended || !log_probs || !ctl || !host_words)
    return PDT_E_ARG;
  if (has_eos && (eos < 0 || eos >= V)) return PDT_E_ARG;
  if (V >= (1 << 30) || N >= (1ll << 31) || C >= (1 << 24) || R >= (1ll << 40) / U) return PDT_E_TOO_LONG;
  WalkTableArgs a{};
  a.table = table; a.tb_sr = tb_sr; a.stats = row_stats; a.R = R; a.U = U; a.u = u;
  a.N = (int)N; a.V = (int)V; a.C = (int)C; a.y = y; a.ctx = ctx; a.lens = lens; a.ended = ended; a.lp = log_probs;
  a.has_eos = has_eos; a.eos = has_eos ? (int)eos : 0; a.ctl = ctl; a.host = host_words;
  hipLaunchKernelGGL(random_walk_table_kernel, dim3(walk_blocks(N)), dim3(64 * kWalkWaves), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // extern "C"
