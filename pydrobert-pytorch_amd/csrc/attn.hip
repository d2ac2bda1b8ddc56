// Soft attention (reference _attn.py:200-223, 276, 336): scores, masked softmax and the weighted
// sum of values in one pass, and its adjoint.
//
// Every call is reduced by the host to rows x T x D: a row is one query (one output vector), T the
// attended axis, D the feature axis of query and key, Dv that of value.  The descriptor (see
// include/pdt_amd.h) gives up to eight row dimensions and, per operand, their element strides
// (0 = broadcast), the T stride and the feature stride.  The host orders the row dimensions so that
// the ones over which key and value are both broadcast -- "the group": beams sharing an utterance,
// or the queries of a self-attention -- come innermost: rows g * M .. g * M + M - 1 share one key
// and one value sequence.
//
// Forward.  One workgroup serves a tile of up to eight rows of one group over a span of T (the span
// is all of T unless groups x tiles cannot fill the chip, when T is split as flash-decoding does).
// Per tile of 32 frames: the mask of the tile's rows, then one wave per frame forms the tile's scores
// (lanes across D, the query rows in LDS: each key element loaded serves every row), a half-wave per row
// updates the running maximum and sum, then every thread adds p * value into the accumulators of its
// value columns.  Four frames' (or four key chunks') loads are issued before their products.  Frames no row of
// the tile attends to are skipped, keys and values included.  Split
// spans leave (max, sum, accumulator) partials that one combine pass merges in split order.  The
// per-row maximum and log of the sum are kept for the backward as two numbers (lse[r], lse[R + r]): their
// sum in the input's type would round away log(sum) next to a large |maximum|.
//
// Large groups of narrow rows (D, Dv <= 32, 16 or more rows per group) take attn_fwd_rows_kernel instead:
// one thread per row over all of T, the group's rows reading each key and value element together.
//
// Backward.  One workgroup per (group, 32 frames) walks every row tile of its group: it recomputes
// a = exp((score - max) - log sum), dP = dout . value and dS = a (dP - delta), delta = rowsum(dout * out) (a
// separate pass), then sums dK and dV for its frames over the whole group itself -- each element
// is owned by one thread for the whole walk, so no atomics and a fixed order -- and writes the
// frames' dQ partial; a combine pass adds the partials in frame order.  The pool forms take the
// scores as given and return dE instead of dQ / dK.
//
// Masked frames contribute exactly 0 to outputs and gradients: they are skipped, never multiplied
// by 0.  No float atomics anywhere: outputs and gradients are bitwise reproducible.
//
// Element types.  Every kernel is a template over the element type E of the operands (float, double, f16_t,
// bf16_t) and computes in F = AttnAcc<E>: double for double, float for the other three.  A half instance is
// the float instance with elem_load at its global reads of query, key, value, score, out and grad_out and
// elem_store at its global writes of out and the gradients; the LDS tiles, AttnShared, lse and everything in
// the workspace are float, and the plan is the float one (esz 4).  So a half call gives the bits of the float
// call on the exactly widened operands, each result rounded once where it is stored.  One place needs more
// than that: the backward adds a group's row tiles into dK / dV, and the running sum may not pass through a
// half element -- attn_bwd_half_kernel.
#include "pdt_common.hpp"

#include <cmath>

namespace pdt {

constexpr int kAttnThreads = 256;
constexpr int kAttnWaves = kAttnThreads / PDT_WAVE;
constexpr int kAttnRows = 8;     // rows per tile (at most)
constexpr int kAttnFrames = 32;  // frames per tile
constexpr int kAttnCols = 1024;  // value columns per forward workgroup (grid.z covers wider values)
constexpr int kAttnColsPer = kAttnCols / kAttnThreads;
static_assert(kAttnRows * kAttnFrames == kAttnThreads, "the softmax step gives every (row, frame) one lane");
constexpr int kAttnRowsMaxD = 32;    // the one-thread-per-row forward: D, Dv up to this
constexpr int64_t kAttnRowsGroup = 16;  // ... and at least this many rows per group
constexpr int64_t kAttnLdsBytes = 57344;  // query / upstream tiles in LDS (plus the static state: under 64 KiB)

enum { SQ = 0, SK, SV, SM, SO, SGQ, SGK, SGV, NSLOT };  // Q doubles as E, GQ as GE in the pool forms

struct AttnDesc {
  int64_t nd, R, G, M, T, D, Dv;
  int64_t size[PDT_ATTN_MAX_DIMS];
  int64_t st[NSLOT][PDT_ATTN_MAX_DIMS];
  int64_t ts[NSLOT], fs[NSLOT];
};

struct AttnArgs {
  AttnDesc d;
  const void *q, *k, *v, *e;
  const uint8_t *mask;
  const void *out, *lse, *gout;
  void *o, *l, *gq, *gk, *gv, *ge;
  void *ws;
  double scale;
  int64_t rt;      // rows per tile
  int64_t tiles;   // row tiles per group
  int64_t splits;  // forward: spans of T; backward: frame chunks
  int64_t span;    // frames per span (forward)
};

// element offsets of row r in every operand slot (row dims innermost last; static indexing only)
__device__ __forceinline__ void attn_row_offsets(const AttnDesc &d, int64_t r, int64_t off[NSLOT]) {
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) off[s] = 0;
#pragma unroll
  for (int i = PDT_ATTN_MAX_DIMS - 1; i >= 0; --i) {
    if (i < d.nd) {
      const int64_t n = d.size[i], idx = r % n;
      r /= n;
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) off[s] += idx * d.st[s][i];
    }
  }
}

template <typename F> __device__ __forceinline__ F wave_sum(F x) {
#pragma unroll
  for (int o = PDT_WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

template <typename F> __device__ __forceinline__ F neg_inf() { return -(F)INFINITY; }

template <typename E> struct AttnAcc { using type = float; };
template <> struct AttnAcc<double> { using type = double; };
__device__ __forceinline__ double elem_load(const double *p) { return *p; }
__device__ __forceinline__ void elem_store(double *p, double x) { *p = x; }

// Per-tile shared state of the forward and backward kernels.
template <typename F> struct AttnShared {
  int64_t roff[kAttnRows][NSLOT];
  F sc[kAttnRows][kAttnFrames];  // scores, then probabilities (forward) / a (backward)
  F ds[kAttnRows][kAttnFrames];  // dS (backward)
  F rm[kAttnRows], rl[kAttnRows], ra[kAttnRows];  // running max, sum, rescale / max, delta, log sum
  uint8_t vm[kAttnRows][kAttnFrames];             // (row, frame) attended
  int fv[kAttnFrames];                            // frame attended by some row of the tile
};

// rows [r0, r0 + nr): offsets into sh.roff; frames [t0, t0 + nt): sh.vm and sh.fv
template <typename F>
__device__ __forceinline__ void attn_load_mask(const AttnArgs &a, AttnShared<F> &sh, int nr, int64_t t0, int nt) {
  const int tid = threadIdx.x;
  if (tid < kAttnFrames) {
    int any = 0;
    const int64_t t = t0 + tid;
#pragma unroll
    for (int r = 0; r < kAttnRows; ++r) {
      uint8_t ok = 0;
      if (r < nr && tid < nt) ok = a.mask ? (uint8_t)(a.mask[sh.roff[r][SM] + t * a.d.ts[SM]] != 0) : (uint8_t)1;
      sh.vm[r][tid] = ok;
      any |= ok;
    }
    sh.fv[tid] = any;
  }
}

template <typename E, bool POOL>
__global__ __launch_bounds__(kAttnThreads) void attn_fwd_kernel(AttnArgs a) {
  using F = typename AttnAcc<E>::type;
  extern __shared__ __align__(16) unsigned char attn_smem[];
  F *qs = reinterpret_cast<F *>(attn_smem);  // [rt][D] (dot)
  __shared__ AttnShared<F> sh;
  const AttnDesc &d = a.d;
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int64_t g = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int64_t r0 = g * d.M + tile * a.rt;
  const int nr = (int)min(a.rt, d.M - tile * a.rt);
  const int64_t t_begin = (int64_t)blockIdx.y * a.span, t_end = min(d.T, t_begin + a.span);
  const int64_t col0 = (int64_t)blockIdx.z * kAttnCols;
  const E *q = (const E *)a.q, *k = (const E *)a.k, *v = (const E *)a.v, *e = (const E *)a.e;

  if (tid < nr) {
    int64_t off[NSLOT];
    attn_row_offsets(d, r0 + tid, off);
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) sh.roff[tid][s] = off[s];
    sh.rm[tid] = neg_inf<F>();
    sh.rl[tid] = 0;
  }
  __syncthreads();
  const int64_t koff = sh.roff[0][SK], voff = sh.roff[0][SV];  // (the same for every row of the group)
  if (!POOL) {
    for (int64_t i = tid; i < (int64_t)nr * d.D; i += kAttnThreads) {
      const int r = (int)(i / d.D);
      const int64_t c = i - r * d.D;
      qs[i] = elem_load(q + sh.roff[r][SQ] + c * d.fs[SQ]);
    }
  }

  F acc[kAttnRows][kAttnColsPer];
#pragma unroll
  for (int r = 0; r < kAttnRows; ++r)
#pragma unroll
    for (int j = 0; j < kAttnColsPer; ++j) acc[r][j] = 0;

  for (int64_t t0 = t_begin; t0 < t_end; t0 += kAttnFrames) {
    const int nt = (int)min((int64_t)kAttnFrames, t_end - t0);
    attn_load_mask(a, sh, nr, t0, nt);
    __syncthreads();
    // scores
    if (POOL) {
      for (int i = tid; i < kAttnRows * kAttnFrames; i += kAttnThreads) {
        const int r = i / kAttnFrames, j = i % kAttnFrames;
        sh.sc[r][j] = sh.vm[r][j] ? elem_load(e + sh.roff[r][SQ] + (t0 + j) * d.ts[SQ]) : neg_inf<F>();
      }
    } else {
      for (int j = wave; j < kAttnFrames; j += kAttnWaves) {
        F s[kAttnRows];
#pragma unroll
        for (int r = 0; r < kAttnRows; ++r) s[r] = 0;
        if (sh.fv[j]) {
          const E *kp = k + koff + (t0 + j) * d.ts[SK];
          for (int64_t c0 = lane; c0 < d.D; c0 += 4 * PDT_WAVE) {
            F kv[4];  // (four loads in flight before the products)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int64_t c = c0 + u * PDT_WAVE;
              kv[u] = c < d.D ? elem_load(kp + c * d.fs[SK]) : (F)0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int64_t c = c0 + u * PDT_WAVE;
              if (c < d.D) {
#pragma unroll
                for (int r = 0; r < kAttnRows; ++r)
                  if (r < nr) s[r] += qs[r * d.D + c] * kv[u];
              }
            }
          }
#pragma unroll
          for (int r = 0; r < kAttnRows; ++r) s[r] = wave_sum(s[r]);
        }
        if (lane < kAttnRows) {
          F mine = 0;
#pragma unroll
          for (int r = 0; r < kAttnRows; ++r) mine = lane == r ? s[r] : mine;
          sh.sc[lane][j] = sh.vm[lane][j] ? mine * (F)a.scale : neg_inf<F>();
        }
      }
    }
    __syncthreads();
    // online softmax: 32 lanes per row, one per frame (kAttnRows * kAttnFrames == kAttnThreads)
    {
      const int r = tid / kAttnFrames, j = tid % kAttnFrames;
      const F x = r < nr && j < nt ? sh.sc[r][j] : neg_inf<F>();
      F m = x;
#pragma unroll
      for (int o = kAttnFrames / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
      const F m_old = r < nr ? sh.rm[r] : neg_inf<F>();
      m = fmax(m, m_old);
      const F p = x == neg_inf<F>() ? (F)0 : exp(x - m);
      F sum = p;
#pragma unroll
      for (int o = kAttnFrames / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      __syncthreads();  // (every lane has read its score before any is overwritten)
      sh.sc[r][j] = p;
      if (j == 0 && r < nr) {
        const F alpha = m == neg_inf<F>() ? (F)1 : (m_old == neg_inf<F>() ? (F)0 : exp(m_old - m));
        sh.rm[r] = m;
        sh.rl[r] = sh.rl[r] * alpha + sum;
        sh.ra[r] = alpha;
      }
    }
    __syncthreads();
    // weighted values
#pragma unroll
    for (int r = 0; r < kAttnRows; ++r) {
      const F alpha = r < nr ? sh.ra[r] : (F)0;
#pragma unroll
      for (int j = 0; j < kAttnColsPer; ++j) acc[r][j] *= alpha;
    }
    const int ncols = (int)min((int64_t)kAttnColsPer, (d.Dv - col0 + kAttnThreads - 1) / kAttnThreads);
    for (int j0 = 0; j0 < nt; j0 += 4) {
      F vv[4][kAttnColsPer];  // (the frames' loads in flight before the products)
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int j = j0 + f;
        const bool live = j < nt && sh.fv[j];
        const E *vp = v + voff + (t0 + j) * d.ts[SV];
#pragma unroll
        for (int u = 0; u < kAttnColsPer; ++u) {
          const int64_t c = col0 + tid + u * kAttnThreads;
          vv[f][u] = live && u < ncols && c < d.Dv ? elem_load(vp + c * d.fs[SV]) : (F)0;
        }
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (j0 + f >= nt) break;
#pragma unroll
        for (int r = 0; r < kAttnRows; ++r) {
          const F p = sh.sc[r][j0 + f];  // (0 for a masked frame, an idle row or a frame no row attends)
          if (p != (F)0) {
#pragma unroll
            for (int u = 0; u < kAttnColsPer; ++u)
              if (u < ncols) acc[r][u] += p * vv[f][u];
          }
        }
      }
    }
    __syncthreads();
  }

  if (a.splits == 1) {
    E *o = (E *)a.o;
#pragma unroll
    for (int r = 0; r < kAttnRows; ++r) {
      if (r >= nr) break;
      const F l = sh.rl[r];
#pragma unroll
      for (int u = 0; u < kAttnColsPer; ++u) {
        const int64_t c = col0 + tid + u * kAttnThreads;
        if (c < d.Dv) elem_store(o + sh.roff[r][SO] + c * d.fs[SO], acc[r][u] / l);  // (0 / 0: an all-masked row is NaN)
      }
    }
    if (blockIdx.z == 0 && tid < nr) {
      ((F *)a.l)[r0 + tid] = sh.rm[tid];
      ((F *)a.l)[d.R + r0 + tid] = log(sh.rl[tid]);
    }
  } else {
    // partials: m [splits][R], l [splits][R], acc [splits][R][Dv]
    F *pm = (F *)a.ws, *pl = pm + a.splits * d.R, *pa = pl + a.splits * d.R;
    const int64_t sp = blockIdx.y;
#pragma unroll
    for (int r = 0; r < kAttnRows; ++r) {
      if (r >= nr) break;
      F *row = pa + (sp * d.R + r0 + r) * d.Dv;
#pragma unroll
      for (int u = 0; u < kAttnColsPer; ++u) {
        const int64_t c = col0 + tid + u * kAttnThreads;
        if (c < d.Dv) row[c] = acc[r][u];
      }
    }
    if (blockIdx.z == 0 && tid < nr) {
      pm[sp * d.R + r0 + tid] = sh.rm[tid];
      pl[sp * d.R + r0 + tid] = sh.rl[tid];
    }
  }
}

// Large groups of narrow rows (D, Dv <= 32, at least kAttnRowsGroup rows sharing a key and value sequence,
// as in a multi-head self-attention): one thread per row, its query and accumulators in registers, over
// all of T.  The lanes of a wave are consecutive rows of one group, so they read the same key and value
// element together; no lane idles on a narrow feature axis and no cross-lane sums are needed.
template <typename E, bool POOL, int DMAX>
__global__ __launch_bounds__(kAttnThreads) void attn_fwd_rows_kernel(AttnArgs a) {
  using F = typename AttnAcc<E>::type;
  const AttnDesc &d = a.d;
  const int64_t r = (int64_t)blockIdx.x * kAttnThreads + threadIdx.x;
  if (r >= d.R) return;
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  const E *k = (const E *)a.k + off[SK], *v = (const E *)a.v + off[SV], *e = (const E *)a.e + off[SQ];
  const uint8_t *mk = a.mask ? a.mask + off[SM] : nullptr;
  const F scale = (F)a.scale;
  F qr[DMAX], acc[DMAX];
#pragma unroll
  for (int c = 0; c < DMAX; ++c) {
    qr[c] = !POOL && c < d.D ? elem_load((const E *)a.q + off[SQ] + c * d.fs[SQ]) : (F)0;
    acc[c] = 0;
  }
  F m = neg_inf<F>(), l = 0;
  for (int64_t t = 0; t < d.T; ++t) {
    if (mk && !mk[t * d.ts[SM]]) continue;  // (a masked frame contributes exactly 0)
    F x;
    if (POOL) {
      x = elem_load(e + t * d.ts[SQ]);
    } else {
      // the products summed pairwise at distances DMAX / 2 .. 1: the order of the backward's wave_sum over
      // lanes across D, so that it rebuilds these very scores (bit for bit: a and delta stay consistent)
      const E *kp = k + t * d.ts[SK];
      F pr[DMAX];
#pragma unroll
      for (int c = 0; c < DMAX; ++c) pr[c] = c < d.D ? qr[c] * elem_load(kp + c * d.fs[SK]) : (F)0;
#pragma unroll
      for (int o = DMAX / 2; o > 0; o >>= 1)
#pragma unroll
        for (int c = 0; c < o; ++c) pr[c] += pr[c + o];
      x = pr[0] * scale;
    }
    if (x == neg_inf<F>()) continue;
    if (x > m) {  // (a new maximum: rescale what is summed so far)
      const F alpha = m == neg_inf<F>() ? (F)0 : exp(m - x);
      l *= alpha;
#pragma unroll
      for (int c = 0; c < DMAX; ++c) acc[c] *= alpha;
      m = x;
    }
    const F p = exp(x - m);
    l += p;
    const E *vp = v + t * d.ts[SV];
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
      if (c < d.Dv) acc[c] += p * elem_load(vp + c * d.fs[SV]);
  }
  E *o = (E *)a.o + off[SO];
#pragma unroll
  for (int c = 0; c < DMAX; ++c)
    if (c < d.Dv) elem_store(o + c * d.fs[SO], acc[c] / l);  // (0 / 0: an all-masked row is NaN)
  ((F *)a.l)[r] = m;
  ((F *)a.l)[d.R + r] = log(l);
}

// merge the split partials in split order: one thread per (row, column)
template <typename E> __global__ __launch_bounds__(kAttnThreads) void attn_fwd_combine_kernel(AttnArgs a) {
  using F = typename AttnAcc<E>::type;
  const AttnDesc &d = a.d;
  const int64_t i = (int64_t)blockIdx.x * kAttnThreads + threadIdx.x;
  if (i >= d.R * d.Dv) return;
  const int64_t r = i / d.Dv, c = i - r * d.Dv;
  const F *pm = (const F *)a.ws, *pl = pm + a.splits * d.R, *pa = pl + a.splits * d.R;
  F m = neg_inf<F>();
  for (int64_t s = 0; s < a.splits; ++s) m = fmax(m, pm[s * d.R + r]);
  F l = 0, acc = 0;
  if (m != neg_inf<F>()) {
    for (int64_t s = 0; s < a.splits; ++s) {
      const F ms = pm[s * d.R + r];
      if (ms == neg_inf<F>()) continue;
      const F w = exp(ms - m);
      l += pl[s * d.R + r] * w;
      acc += pa[(s * d.R + r) * d.Dv + c] * w;
    }
  }
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  elem_store((E *)a.o + off[SO] + c * d.fs[SO], acc / l);
  if (c == 0) {
    ((F *)a.l)[r] = m;
    ((F *)a.l)[d.R + r] = log(l);
  }
}

// delta[r] = sum_c dout[r, c] * out[r, c]: one wave per row (dout shares out's layout)
template <typename E> __global__ __launch_bounds__(kAttnThreads) void attn_delta_kernel(AttnArgs a) {
  using F = typename AttnAcc<E>::type;
  const AttnDesc &d = a.d;
  const int64_t r = (int64_t)blockIdx.x * kAttnWaves + threadIdx.x / PDT_WAVE;
  if (r >= d.R) return;
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  const E *o = (const E *)a.out + off[SO], *go = (const E *)a.gout + off[SO];
  F s = 0;
  for (int64_t c = threadIdx.x & (PDT_WAVE - 1); c < d.Dv; c += PDT_WAVE)
    s += elem_load(o + c * d.fs[SO]) * elem_load(go + c * d.fs[SO]);
  s = wave_sum(s);
  if ((threadIdx.x & (PDT_WAVE - 1)) == 0) ((F *)a.ws)[r] = s;
}

template <typename F, bool POOL>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_kernel(AttnArgs a) {
  extern __shared__ __align__(16) unsigned char attn_smem[];
  const AttnDesc &d = a.d;
  F *qs = reinterpret_cast<F *>(attn_smem);  // [rt][D] (dot)
  F *dos = qs + (POOL ? 0 : a.rt * d.D);     // [rt][Dv]
  __shared__ AttnShared<F> sh;
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int64_t g = blockIdx.x / a.splits, chunk = blockIdx.x % a.splits;
  const int64_t t0 = chunk * kAttnFrames;
  const int nt = (int)min((int64_t)kAttnFrames, d.T - t0);
  const F *q = (const F *)a.q, *k = (const F *)a.k, *v = (const F *)a.v, *e = (const F *)a.e;
  const F *go = (const F *)a.gout, *lse = (const F *)a.lse, *delta = (const F *)a.ws;
  F *gq_part = (F *)a.ws + d.R;  // [splits][R][D]
  const F scale = (F)a.scale;

  for (int64_t tile = 0; tile < a.tiles; ++tile) {
    const int64_t r0 = g * d.M + tile * a.rt;
    const int nr = (int)min(a.rt, d.M - tile * a.rt);
    if (tid < nr) {
      int64_t off[NSLOT];
      attn_row_offsets(d, r0 + tid, off);
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) sh.roff[tid][s] = off[s];
      sh.rm[tid] = lse[r0 + tid];
      sh.ra[tid] = lse[d.R + r0 + tid];
      sh.rl[tid] = delta[r0 + tid];
    }
    __syncthreads();
    const int64_t koff = sh.roff[0][SK], voff = sh.roff[0][SV], gkoff = sh.roff[0][SGK], gvoff = sh.roff[0][SGV];
    if (!POOL) {
      for (int64_t i = tid; i < (int64_t)nr * d.D; i += kAttnThreads) {
        const int r = (int)(i / d.D);
        const int64_t c = i - r * d.D;
        qs[i] = q[sh.roff[r][SQ] + c * d.fs[SQ]];
      }
    }
    for (int64_t i = tid; i < (int64_t)nr * d.Dv; i += kAttnThreads) {
      const int r = (int)(i / d.Dv);
      const int64_t c = i - r * d.Dv;
      dos[i] = go[sh.roff[r][SO] + c * d.fs[SO]];
    }
    attn_load_mask(a, sh, nr, t0, nt);
    __syncthreads();
    // a and dS, one wave per frame
    for (int j = wave; j < kAttnFrames; j += kAttnWaves) {
      F s[kAttnRows], dp[kAttnRows];
#pragma unroll
      for (int r = 0; r < kAttnRows; ++r) s[r] = dp[r] = 0;
      if (sh.fv[j]) {
        const int64_t t = t0 + j;
        const F *vp = v + voff + t * d.ts[SV];
        for (int64_t c = lane; c < d.Dv; c += PDT_WAVE) {
          const F vv = vp[c * d.fs[SV]];
#pragma unroll
          for (int r = 0; r < kAttnRows; ++r)
            if (r < nr) dp[r] += dos[r * d.Dv + c] * vv;
        }
        if (!POOL) {
          const F *kp = k + koff + t * d.ts[SK];
          for (int64_t c = lane; c < d.D; c += PDT_WAVE) {
            const F kv = kp[c * d.fs[SK]];
#pragma unroll
            for (int r = 0; r < kAttnRows; ++r)
              if (r < nr) s[r] += qs[r * d.D + c] * kv;
          }
        }
#pragma unroll
        for (int r = 0; r < kAttnRows; ++r) {
          dp[r] = wave_sum(dp[r]);
          if (!POOL) s[r] = wave_sum(s[r]);
        }
      }
      if (lane < kAttnRows) {
        F ms = 0, mdp = 0;
#pragma unroll
        for (int r = 0; r < kAttnRows; ++r) {
          ms = lane == r ? s[r] : ms;
          mdp = lane == r ? dp[r] : mdp;
        }
        F p = 0, dsv = 0;
        if (lane < nr && j < nt && sh.vm[lane][j]) {
          const F score = POOL ? e[sh.roff[lane][SQ] + (t0 + j) * d.ts[SQ]] : ms * scale;
          p = exp((score - sh.rm[lane]) - sh.ra[lane]);  // (score - max first: exact near a large |max|)
          dsv = p * (mdp - sh.rl[lane]);
        }
        sh.sc[lane][j] = p;
        sh.ds[lane][j] = dsv;
      }
    }
    __syncthreads();
    if (POOL) {
      F *ge = (F *)a.ge;
      for (int i = tid; i < nr * nt; i += kAttnThreads) {
        const int r = i / nt, j = i % nt;
        ge[sh.roff[r][SGQ] + (t0 + j) * d.ts[SGQ]] = sh.ds[r][j];
      }
    } else {
      // dK for the chunk's frames, summed over the group (this thread owns these elements for the walk)
      F *gk = (F *)a.gk;
      for (int64_t i = tid; i < (int64_t)nt * d.D; i += kAttnThreads) {
        const int j = (int)(i / d.D);
        const int64_t c = i - j * d.D;
        F s = 0;
        if (sh.fv[j]) {
#pragma unroll
          for (int r = 0; r < kAttnRows; ++r)
            if (r < nr) s += sh.ds[r][j] * qs[r * d.D + c];
          s *= scale;
        }
        F *dst = gk + gkoff + (t0 + j) * d.ts[SGK] + c * d.fs[SGK];
        *dst = tile == 0 ? s : *dst + s;
      }
    }
    {
      F *gv = (F *)a.gv;
      for (int64_t i = tid; i < (int64_t)nt * d.Dv; i += kAttnThreads) {
        const int j = (int)(i / d.Dv);
        const int64_t c = i - j * d.Dv;
        F s = 0;
        if (sh.fv[j]) {
#pragma unroll
          for (int r = 0; r < kAttnRows; ++r)
            if (r < nr) s += sh.sc[r][j] * dos[r * d.Dv + c];
        }
        F *dst = gv + gvoff + (t0 + j) * d.ts[SGV] + c * d.fs[SGV];
        *dst = tile == 0 ? s : *dst + s;
      }
    }
    if (!POOL) {
      // this chunk's share of dQ
      for (int64_t i = tid; i < (int64_t)nr * d.D; i += kAttnThreads) {
        const int r = (int)(i / d.D);
        const int64_t c = i - r * d.D;
        F s = 0;
        for (int j = 0; j < nt; ++j) {
          const F w = sh.ds[r][j];
          if (w != (F)0) s += w * k[koff + (t0 + j) * d.ts[SK] + c * d.fs[SK]];
        }
        s *= scale;
        if (a.splits == 1)
          ((F *)a.gq)[sh.roff[r][SGQ] + c * d.fs[SGQ]] = s;
        else
          gq_part[(chunk * d.R + r0 + r) * d.D + c] = s;
      }
    }
    __syncthreads();
  }
}

// attn_bwd_kernel for E = f16_t / bf16_t: the same walk, computed in float, with elem_load at the global reads of
// query, key, value, score and grad_out and elem_store at the writes of the gradients.  It is a kernel of its own
// for one reason.  dK / dV of a group with several row tiles are sums over the tiles, and attn_bwd_kernel keeps
// the running sum in the output element (the thread wrote it at the tile before).  A half element cannot hold
// it -- that would round once per tile -- and the workspace is the float plan's, so this kernel keeps the sums of
// kAttnOwn dK and kAttnOwn dV elements per thread in registers across the walk, stores each once after the
// last tile, and walks the group again for the next kAttnOwn elements (D, Dv <= 64 need one walk; every walk
// rebuilds a and dS).  The additions are attn_bwd_kernel<float>'s, in its order.  With one row tile per group
// every element is written once, as there.  (Kept apart so that the float and double instances stay what they
// were instruction for instruction: folded into one template, their register allocation moved.)
constexpr int kAttnOwn = 8;

template <typename E, bool POOL>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_half_kernel(AttnArgs a) {
  using F = float;
  static_assert(sizeof(E) == 2, "the half element types");
  extern __shared__ __align__(16) unsigned char attn_smem[];
  const AttnDesc &d = a.d;
  F *qs = reinterpret_cast<F *>(attn_smem);  // [rt][D] (dot)
  F *dos = qs + (POOL ? 0 : a.rt * d.D);     // [rt][Dv]
  __shared__ AttnShared<F> sh;
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int64_t g = blockIdx.x / a.splits, chunk = blockIdx.x % a.splits;
  const int64_t t0 = chunk * kAttnFrames;
  const int nt = (int)min((int64_t)kAttnFrames, d.T - t0);
  const E *q = (const E *)a.q, *k = (const E *)a.k, *v = (const E *)a.v, *e = (const E *)a.e;
  const E *go = (const E *)a.gout;
  const F *lse = (const F *)a.lse, *delta = (const F *)a.ws;
  F *gq_part = (F *)a.ws + d.R;  // [splits][R][D]
  const F scale = (F)a.scale;
  const bool own = a.tiles > 1;  // (sums in registers: see above)
  const int64_t per_walk = (int64_t)kAttnOwn * kAttnThreads;
  const int walks = own ? (int)((nt * max(d.D, d.Dv) + per_walk - 1) / per_walk) : 1;

  for (int walk = 0; walk < walks; ++walk) {
    F own_k[kAttnOwn], own_v[kAttnOwn];
#pragma unroll
    for (int u = 0; u < kAttnOwn; ++u) own_k[u] = own_v[u] = 0;
    for (int64_t tile = 0; tile < a.tiles; ++tile) {
      const int64_t r0 = g * d.M + tile * a.rt;
      const int nr = (int)min(a.rt, d.M - tile * a.rt);
      if (tid < nr) {
        int64_t off[NSLOT];
        attn_row_offsets(d, r0 + tid, off);
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) sh.roff[tid][s] = off[s];
        sh.rm[tid] = lse[r0 + tid];
        sh.ra[tid] = lse[d.R + r0 + tid];
        sh.rl[tid] = delta[r0 + tid];
      }
      __syncthreads();
      const int64_t koff = sh.roff[0][SK], voff = sh.roff[0][SV], gkoff = sh.roff[0][SGK], gvoff = sh.roff[0][SGV];
      if (!POOL) {
        for (int64_t i = tid; i < (int64_t)nr * d.D; i += kAttnThreads) {
          const int r = (int)(i / d.D);
          const int64_t c = i - r * d.D;
          qs[i] = elem_load(q + sh.roff[r][SQ] + c * d.fs[SQ]);
        }
      }
      for (int64_t i = tid; i < (int64_t)nr * d.Dv; i += kAttnThreads) {
        const int r = (int)(i / d.Dv);
        const int64_t c = i - r * d.Dv;
        dos[i] = elem_load(go + sh.roff[r][SO] + c * d.fs[SO]);
      }
      attn_load_mask(a, sh, nr, t0, nt);
      __syncthreads();
      // a and dS, one wave per frame
      for (int j = wave; j < kAttnFrames; j += kAttnWaves) {
        F s[kAttnRows], dp[kAttnRows];
#pragma unroll
        for (int r = 0; r < kAttnRows; ++r) s[r] = dp[r] = 0;
        if (sh.fv[j]) {
          const int64_t t = t0 + j;
          const E *vp = v + voff + t * d.ts[SV];
          for (int64_t c = lane; c < d.Dv; c += PDT_WAVE) {
            const F vv = elem_load(vp + c * d.fs[SV]);
#pragma unroll
            for (int r = 0; r < kAttnRows; ++r)
              if (r < nr) dp[r] += dos[r * d.Dv + c] * vv;
          }
          if (!POOL) {
            const E *kp = k + koff + t * d.ts[SK];
            for (int64_t c = lane; c < d.D; c += PDT_WAVE) {
              const F kv = elem_load(kp + c * d.fs[SK]);
#pragma unroll
              for (int r = 0; r < kAttnRows; ++r)
                if (r < nr) s[r] += qs[r * d.D + c] * kv;
            }
          }
#pragma unroll
          for (int r = 0; r < kAttnRows; ++r) {
            dp[r] = wave_sum(dp[r]);
            if (!POOL) s[r] = wave_sum(s[r]);
          }
        }
        if (lane < kAttnRows) {
          F ms = 0, mdp = 0;
#pragma unroll
          for (int r = 0; r < kAttnRows; ++r) {
            ms = lane == r ? s[r] : ms;
            mdp = lane == r ? dp[r] : mdp;
          }
          F p = 0, dsv = 0;
          if (lane < nr && j < nt && sh.vm[lane][j]) {
            const F score = POOL ? elem_load(e + sh.roff[lane][SQ] + (t0 + j) * d.ts[SQ]) : ms * scale;
            p = exp((score - sh.rm[lane]) - sh.ra[lane]);  // (score - max first: exact near a large |max|)
            dsv = p * (mdp - sh.rl[lane]);
          }
          sh.sc[lane][j] = p;
          sh.ds[lane][j] = dsv;
        }
      }
      __syncthreads();
      E *gk = (E *)a.gk, *gv = (E *)a.gv;
      if (POOL) {
        E *ge = (E *)a.ge;
        for (int i = tid; i < nr * nt && walk == 0; i += kAttnThreads) {
          const int r = i / nt, j = i % nt;
          elem_store(ge + sh.roff[r][SGQ] + (t0 + j) * d.ts[SGQ], sh.ds[r][j]);
        }
      } else if (!own) {
        // dK for the chunk's frames, summed over the group (this thread owns these elements for the walk)
        for (int64_t i = tid; i < (int64_t)nt * d.D; i += kAttnThreads) {
          const int j = (int)(i / d.D);
          const int64_t c = i - j * d.D;
          F s = 0;
          if (sh.fv[j]) {
#pragma unroll
            for (int r = 0; r < kAttnRows; ++r)
              if (r < nr) s += sh.ds[r][j] * qs[r * d.D + c];
            s *= scale;
          }
          elem_store(gk + gkoff + (t0 + j) * d.ts[SGK] + c * d.fs[SGK], s);  // (one row tile: the only write)
        }
      }
      if (!own) {
        for (int64_t i = tid; i < (int64_t)nt * d.Dv; i += kAttnThreads) {
          const int j = (int)(i / d.Dv);
          const int64_t c = i - j * d.Dv;
          F s = 0;
          if (sh.fv[j]) {
#pragma unroll
            for (int r = 0; r < kAttnRows; ++r)
              if (r < nr) s += sh.sc[r][j] * dos[r * d.Dv + c];
          }
          elem_store(gv + gvoff + (t0 + j) * d.ts[SGV] + c * d.fs[SGV], s);
        }
      } else {
        // (half, several row tiles: this walk's kAttnOwn elements of dK and of dV per thread, in registers)
        const bool last = tile == a.tiles - 1;
#pragma unroll
        for (int u = 0; u < kAttnOwn; ++u) {
          const int64_t i = ((int64_t)walk * kAttnOwn + u) * kAttnThreads + tid;
          if (!POOL && i < (int64_t)nt * d.D) {
            const int j = (int)(i / d.D);
            const int64_t c = i - j * d.D;
            F s = 0;
            if (sh.fv[j]) {
#pragma unroll
              for (int r = 0; r < kAttnRows; ++r)
                if (r < nr) s += sh.ds[r][j] * qs[r * d.D + c];
              s *= scale;
            }
            own_k[u] = tile == 0 ? s : own_k[u] + s;
            if (last) elem_store(gk + gkoff + (t0 + j) * d.ts[SGK] + c * d.fs[SGK], own_k[u]);
          }
          if (i < (int64_t)nt * d.Dv) {
            const int j = (int)(i / d.Dv);
            const int64_t c = i - j * d.Dv;
            F s = 0;
            if (sh.fv[j]) {
#pragma unroll
              for (int r = 0; r < kAttnRows; ++r)
                if (r < nr) s += sh.sc[r][j] * dos[r * d.Dv + c];
            }
            own_v[u] = tile == 0 ? s : own_v[u] + s;
            if (last) elem_store(gv + gvoff + (t0 + j) * d.ts[SGV] + c * d.fs[SGV], own_v[u]);
          }
        }
      }
      if (!POOL && walk == 0) {
        // this chunk's share of dQ
        for (int64_t i = tid; i < (int64_t)nr * d.D; i += kAttnThreads) {
          const int r = (int)(i / d.D);
          const int64_t c = i - r * d.D;
          F s = 0;
          for (int j = 0; j < nt; ++j) {
            const F w = sh.ds[r][j];
            if (w != (F)0) s += w * elem_load(k + koff + (t0 + j) * d.ts[SK] + c * d.fs[SK]);
          }
          s *= scale;
          if (a.splits == 1)
            elem_store((E *)a.gq + sh.roff[r][SGQ] + c * d.fs[SGQ], s);
          else
            gq_part[(chunk * d.R + r0 + r) * d.D + c] = s;
        }
      }
      __syncthreads();
    }
  }
}

// dQ: the chunks' partials added in chunk order, one thread per (row, column)
template <typename E> __global__ __launch_bounds__(kAttnThreads) void attn_gq_combine_kernel(AttnArgs a) {
  using F = typename AttnAcc<E>::type;
  const AttnDesc &d = a.d;
  const int64_t i = (int64_t)blockIdx.x * kAttnThreads + threadIdx.x;
  if (i >= d.R * d.D) return;
  const int64_t r = i / d.D, c = i - r * d.D;
  const F *part = (const F *)a.ws + d.R;
  F s = 0;
  for (int64_t ch = 0; ch < a.splits; ++ch) s += part[(ch * d.R + r) * d.D + c];
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  elem_store((E *)a.gq + off[SGQ] + c * d.fs[SGQ], s);
}

// ------------------------------------------------------------------------------------------
// host side

enum { ATTN_DOT = 0, ATTN_DOT_BWD = 1, ATTN_POOL = 2, ATTN_POOL_BWD = 3 };

// Reads and checks the descriptor; the sizes must multiply to R = G * M, the innermost dims whose
// sizes multiply to M (the group) must broadcast key, value and their gradients.
static int attn_desc(const int64_t *in, int kind, AttnDesc *d) {
  if (!in) return PDT_E_ARG;
  const bool pool = kind >= ATTN_POOL;
  d->nd = in[0]; d->R = in[1]; d->G = in[2]; d->M = in[3]; d->T = in[4]; d->D = in[5]; d->Dv = in[6];
  if (d->nd < 0 || d->nd > PDT_ATTN_MAX_DIMS || d->R < 0 || d->G < 0 || d->M < 0 || d->T < 0 || d->Dv < 1)
    return PDT_E_ARG;
  if (pool ? d->D != 0 : d->D < 1) return PDT_E_ARG;
  int64_t prod = 1;
  for (int i = 0; i < PDT_ATTN_MAX_DIMS; ++i) {
    d->size[i] = i < d->nd ? in[7 + i] : 1;
    if (d->size[i] < 0) return PDT_E_ARG;
    prod *= d->size[i];
  }
  for (int s = 0; s < NSLOT; ++s) {
    const int64_t *b = in + 7 + PDT_ATTN_MAX_DIMS + s * (PDT_ATTN_MAX_DIMS + 2);
    for (int i = 0; i < PDT_ATTN_MAX_DIMS; ++i) d->st[s][i] = i < d->nd ? b[i] : 0;
    d->ts[s] = b[PDT_ATTN_MAX_DIMS];
    d->fs[s] = b[PDT_ATTN_MAX_DIMS + 1];
  }
  if (prod != d->R || d->G * d->M != d->R) return PDT_E_ARG;
  if (d->R == 0) return PDT_OK;
  int64_t m = 1;
  for (int i = (int)d->nd - 1; i >= 0 && m < d->M; --i) {
    m *= d->size[i];
    if (d->st[SK][i] || d->st[SV][i] || d->st[SGK][i] || d->st[SGV][i]) return PDT_E_ARG;
  }
  if (m != d->M) return PDT_E_ARG;
  return PDT_OK;
}

static int64_t attn_rows_per_tile(const AttnDesc &d, int64_t lds_cols, int64_t esz) {
  const int64_t by_lds = lds_cols ? kAttnLdsBytes / (lds_cols * esz) : kAttnRows;
  return std::min<int64_t>(std::min<int64_t>(kAttnRows, d.M), by_lds);
}

struct AttnPlan {
  int64_t rt, tiles, zcols, splits, span, ws_bytes, lds_bytes;
  int rows_form;  // forward: 0 tiles, else the one-thread-per-row kernel for D, Dv <= rows_form
};

static int attn_plan(const AttnDesc &d, int kind, int64_t esz, AttnPlan *p) {
  const bool pool = kind >= ATTN_POOL, bwd = kind == ATTN_DOT_BWD || kind == ATTN_POOL_BWD;
  *p = AttnPlan{};
  if (d.R == 0) return PDT_OK;
  const int64_t cols = bwd ? (pool ? 0 : d.D) + d.Dv : (pool ? 0 : d.D);
  p->rt = attn_rows_per_tile(d, cols, esz);
  if (p->rt < 1) return PDT_E_TOO_LONG;
  p->tiles = (d.M + p->rt - 1) / p->rt;
  p->lds_bytes = p->rt * cols * esz;
  const int64_t frame_tiles = (d.T + kAttnFrames - 1) / kAttnFrames;
  if (bwd) {
    p->splits = std::max<int64_t>(1, frame_tiles);
    p->span = kAttnFrames;
    p->ws_bytes = d.R * esz + (pool || p->splits == 1 ? 0 : p->splits * d.R * d.D * esz);
    if (d.G * p->splits > 0x7fffffffll) return PDT_E_TOO_LONG;
  } else if (d.M >= kAttnRowsGroup && d.D <= kAttnRowsMaxD && d.Dv <= kAttnRowsMaxD) {
    p->rows_form = d.D <= 16 && d.Dv <= 16 ? 16 : kAttnRowsMaxD;
    p->splits = 1;
    if ((d.R + kAttnThreads - 1) / kAttnThreads > 0x7fffffffll) return PDT_E_TOO_LONG;
  } else {
    p->zcols = (d.Dv + kAttnCols - 1) / kAttnCols;
    const int64_t blocks = d.G * p->tiles * p->zcols;
    // fill the 256 CUs about four workgroups deep; split T only when the rows cannot
    int64_t splits = std::min<int64_t>(std::max<int64_t>(1, (1024 + blocks - 1) / blocks), std::max<int64_t>(1, frame_tiles));
    p->span = std::max<int64_t>(1, (frame_tiles + splits - 1) / splits) * kAttnFrames;
    p->splits = std::max<int64_t>(1, (d.T + p->span - 1) / p->span);
    p->ws_bytes = p->splits == 1 ? 0 : p->splits * d.R * (d.Dv + 2) * esz;
    if (d.G * p->tiles > 0x7fffffffll || p->splits > 65535 || p->zcols > 65535) return PDT_E_TOO_LONG;
  }
  return PDT_OK;
}

// et: the element type, 0 float, 1 double, 2 f16_t, 3 bf16_t (the dtype codes of pdt_attn_*, which take 0 and 1,
// and the elem codes of pdt_attn_*_elem, which take 0, 2 and 3).  The half types plan as float does.
static int attn_prepare(const int64_t *desc, int et, int kind, AttnDesc *d, AttnPlan *p) {
  if (et < 0 || et > 3) return PDT_E_ARG;
  int rc = attn_desc(desc, kind, d);
  if (rc != PDT_OK) return rc;
  if (d->R > 0 && d->T == 0) return PDT_E_ARG;  // (the host returns zeros for an empty T)
  return attn_plan(*d, kind, et == 1 ? 8 : 4, p);
}

static unsigned attn_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <typename E> static int attn_fwd_launch(AttnArgs &a, const AttnPlan &p, bool pool, hipStream_t s) {
  const dim3 blk(kAttnThreads);
  if (p.rows_form) {
    const dim3 rg(attn_blocks(a.d.R, kAttnThreads));
    if (p.rows_form == 16) {
      if (pool) hipLaunchKernelGGL((attn_fwd_rows_kernel<E, true, 16>), rg, blk, 0, s, a);
      else hipLaunchKernelGGL((attn_fwd_rows_kernel<E, false, 16>), rg, blk, 0, s, a);
    } else {
      if (pool) hipLaunchKernelGGL((attn_fwd_rows_kernel<E, true, kAttnRowsMaxD>), rg, blk, 0, s, a);
      else hipLaunchKernelGGL((attn_fwd_rows_kernel<E, false, kAttnRowsMaxD>), rg, blk, 0, s, a);
    }
    return (int)hipGetLastError();
  }
  const dim3 grid((unsigned)(a.d.G * p.tiles), (unsigned)p.splits, (unsigned)p.zcols);
  if (pool)
    hipLaunchKernelGGL((attn_fwd_kernel<E, true>), grid, blk, 0, s, a);
  else
    hipLaunchKernelGGL((attn_fwd_kernel<E, false>), grid, blk, (size_t)p.lds_bytes, s, a);
  if (p.splits > 1) {
    const int64_t n = a.d.R * a.d.Dv;
    if (n / kAttnThreads >= 0x7fffffffll) return PDT_E_TOO_LONG;
    hipLaunchKernelGGL(attn_fwd_combine_kernel<E>, dim3(attn_blocks(n, kAttnThreads)), blk, 0, s, a);
  }
  return (int)hipGetLastError();
}

template <typename E> static int attn_bwd_launch(AttnArgs &a, const AttnPlan &p, bool pool, hipStream_t s) {
  const dim3 blk(kAttnThreads);
  if (a.d.R / kAttnWaves >= 0x7fffffffll) return PDT_E_TOO_LONG;
  hipLaunchKernelGGL(attn_delta_kernel<E>, dim3(attn_blocks(a.d.R, kAttnWaves)), blk, 0, s, a);
  const dim3 grid((unsigned)(a.d.G * p.splits));
  if constexpr (sizeof(E) == 2) {
    if (pool)
      hipLaunchKernelGGL((attn_bwd_half_kernel<E, true>), grid, blk, (size_t)p.lds_bytes, s, a);
    else
      hipLaunchKernelGGL((attn_bwd_half_kernel<E, false>), grid, blk, (size_t)p.lds_bytes, s, a);
  } else if (pool) {
    hipLaunchKernelGGL((attn_bwd_kernel<E, true>), grid, blk, (size_t)p.lds_bytes, s, a);
  } else {
    hipLaunchKernelGGL((attn_bwd_kernel<E, false>), grid, blk, (size_t)p.lds_bytes, s, a);
  }
  if (!pool && p.splits > 1) {
    const int64_t n = a.d.R * a.d.D;
    if (n / kAttnThreads >= 0x7fffffffll) return PDT_E_TOO_LONG;
    hipLaunchKernelGGL(attn_gq_combine_kernel<E>, dim3(attn_blocks(n, kAttnThreads)), blk, 0, s, a);
  }
  return (int)hipGetLastError();
}

static int attn_forward(const int64_t *desc, int et, int kind, const void *q, const void *k, const void *v,
                        const void *e, const void *mask, double scale, void *out, void *lse, void *ws,
                        int64_t ws_bytes, void *stream) {
  AttnDesc d;
  AttnPlan p;
  int rc = attn_prepare(desc, et, kind, &d, &p);
  if (rc != PDT_OK || d.R == 0) return rc;
  const bool pool = kind == ATTN_POOL;
  if (!v || !out || !lse || (pool ? !e : (!q || !k))) return PDT_E_ARG;
  if (ws_bytes < p.ws_bytes || (p.ws_bytes && !ws)) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = q; a.k = k; a.v = v; a.e = e; a.mask = (const uint8_t *)mask; a.o = out; a.l = lse; a.ws = ws;
  a.scale = scale; a.rt = p.rt; a.tiles = p.tiles; a.splits = p.splits; a.span = p.span;
  hipStream_t s = (hipStream_t)stream;
  switch (et) {
    case 1: return attn_fwd_launch<double>(a, p, pool, s);
    case 2: return attn_fwd_launch<f16_t>(a, p, pool, s);
    case 3: return attn_fwd_launch<bf16_t>(a, p, pool, s);
    default: return attn_fwd_launch<float>(a, p, pool, s);
  }
}

static int attn_backward(const int64_t *desc, int et, int kind, const void *q, const void *k, const void *v,
                         const void *e, const void *mask, double scale, const void *out, const void *lse,
                         const void *gout, void *gq, void *gk, void *gv, void *ge, void *ws, int64_t ws_bytes,
                         void *stream) {
  AttnDesc d;
  AttnPlan p;
  int rc = attn_prepare(desc, et, kind, &d, &p);
  if (rc != PDT_OK || d.R == 0) return rc;
  const bool pool = kind == ATTN_POOL_BWD;
  if (!v || !out || !lse || !gout || !gv || (pool ? (!e || !ge) : (!q || !k || !gq || !gk))) return PDT_E_ARG;
  if (ws_bytes < p.ws_bytes || !ws) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = q; a.k = k; a.v = v; a.e = e; a.mask = (const uint8_t *)mask; a.out = out; a.lse = lse;
  a.gout = gout; a.gq = gq; a.gk = gk; a.gv = gv; a.ge = ge; a.ws = ws;
  a.scale = scale; a.rt = p.rt; a.tiles = p.tiles; a.splits = p.splits; a.span = p.span;
  hipStream_t s = (hipStream_t)stream;
  switch (et) {
    case 1: return attn_bwd_launch<double>(a, p, pool, s);
    case 2: return attn_bwd_launch<f16_t>(a, p, pool, s);
    case 3: return attn_bwd_launch<bf16_t>(a, p, pool, s);
    default: return attn_bwd_launch<float>(a, p, pool, s);
  }
}

}  // namespace pdt

extern "C" {

// dtype of the five entry points without a suffix: 0 float32, 1 float64 and nothing else
#define PDT_ATTN_DTYPE(dtype) \
  if ((dtype) != 0 && (dtype) != 1) return PDT_E_ARG

int64_t pdt_attn_workspace_bytes(const int64_t *desc, int dtype, int kind) {
  using namespace pdt;
  if (kind < ATTN_DOT || kind > ATTN_POOL_BWD || (dtype != 0 && dtype != 1)) return -1;
  AttnDesc d;
  AttnPlan p;
  if (attn_prepare(desc, dtype, kind, &d, &p) != PDT_OK) return -1;
  return p.ws_bytes;
}

int pdt_attn_dot(const int64_t *desc, int dtype, const void *query, const void *key, const void *value,
                 const void *mask, const double *scale, void *out, void *lse, void *workspace, int64_t workspace_bytes,
                 void *stream) {
  if (!scale) return PDT_E_ARG;
  PDT_ATTN_DTYPE(dtype);
  return pdt::attn_forward(desc, dtype, pdt::ATTN_DOT, query, key, value, nullptr, mask, *scale, out, lse, workspace,
                           workspace_bytes, stream);
}

int pdt_attn_dot_backward(const int64_t *desc, int dtype, const void *query, const void *key, const void *value,
                          const void *mask, const double *scale, const void *out, const void *lse, const void *grad_out,
                          void *grad_query, void *grad_key, void *grad_value, void *workspace,
                          int64_t workspace_bytes, void *stream) {
  if (!scale) return PDT_E_ARG;
  PDT_ATTN_DTYPE(dtype);
  return pdt::attn_backward(desc, dtype, pdt::ATTN_DOT_BWD, query, key, value, nullptr, mask, *scale, out, lse,
                            grad_out, grad_query, grad_key, grad_value, nullptr, workspace, workspace_bytes, stream);
}

int pdt_attn_pool(const int64_t *desc, int dtype, const void *score, const void *value, const void *mask, void *out,
                  void *lse, void *workspace, int64_t workspace_bytes, void *stream) {
  PDT_ATTN_DTYPE(dtype);
  return pdt::attn_forward(desc, dtype, pdt::ATTN_POOL, nullptr, nullptr, value, score, mask, 1.0, out, lse, workspace,
                           workspace_bytes, stream);
}

int pdt_attn_pool_backward(const int64_t *desc, int dtype, const void *score, const void *value, const void *mask,
                           const void *out, const void *lse, const void *grad_out, void *grad_score,
                           void *grad_value, void *workspace, int64_t workspace_bytes, void *stream) {
  PDT_ATTN_DTYPE(dtype);
  return pdt::attn_backward(desc, dtype, pdt::ATTN_POOL_BWD, nullptr, nullptr, value, score, mask, 1.0, out, lse,
                            grad_out, nullptr, nullptr, grad_value, grad_score, workspace, workspace_bytes, stream);
}

// The same for operands of the element type `elem` (0 float32, 2 float16, 3 bfloat16): the element code is checked
// first, then everything the entry points above check, all before any launch.
#define PDT_ATTN_ELEM(elem)                  \
  {                                          \
    const int rc_ = pdt::elem_status(elem);  \
    if (rc_ != PDT_OK) return rc_;           \
  }

int64_t pdt_attn_workspace_bytes_elem(const int64_t *desc, int elem, int kind) {
  using namespace pdt;
  if (kind < ATTN_DOT || kind > ATTN_POOL_BWD || elem_status(elem) != PDT_OK) return -1;
  AttnDesc d;
  AttnPlan p;
  if (attn_prepare(desc, elem, kind, &d, &p) != PDT_OK) return -1;
  return p.ws_bytes;
}

int pdt_attn_dot_elem(const int64_t *desc, int elem, const void *query, const void *key, const void *value,
                      const void *mask, const double *scale, void *out, void *lse, void *workspace,
                      int64_t workspace_bytes, void *stream) {
  PDT_ATTN_ELEM(elem);
  if (!scale) return PDT_E_ARG;
  return pdt::attn_forward(desc, elem, pdt::ATTN_DOT, query, key, value, nullptr, mask, *scale, out, lse, workspace,
                           workspace_bytes, stream);
}

int pdt_attn_dot_backward_elem(const int64_t *desc, int elem, const void *query, const void *key, const void *value,
                               const void *mask, const double *scale, const void *out, const void *lse,
                               const void *grad_out, void *grad_query, void *grad_key, void *grad_value,
                               void *workspace, int64_t workspace_bytes, void *stream) {
  PDT_ATTN_ELEM(elem);
  if (!scale) return PDT_E_ARG;
  return pdt::attn_backward(desc, elem, pdt::ATTN_DOT_BWD, query, key, value, nullptr, mask, *scale, out, lse,
                            grad_out, grad_query, grad_key, grad_value, nullptr, workspace, workspace_bytes, stream);
}

int pdt_attn_pool_elem(const int64_t *desc, int elem, const void *score, const void *value, const void *mask,
                       void *out, void *lse, void *workspace, int64_t workspace_bytes, void *stream) {
  PDT_ATTN_ELEM(elem);
  return pdt::attn_forward(desc, elem, pdt::ATTN_POOL, nullptr, nullptr, value, score, mask, 1.0, out, lse, workspace,
                           workspace_bytes, stream);
}

int pdt_attn_pool_backward_elem(const int64_t *desc, int elem, const void *score, const void *value, const void *mask,
                                const void *out, const void *lse, const void *grad_out, void *grad_score,
                                void *grad_value, void *workspace, int64_t workspace_bytes, void *stream) {
  PDT_ATTN_ELEM(elem);
  return pdt::attn_backward(desc, elem, pdt::ATTN_POOL_BWD, nullptr, nullptr, value, score, mask, 1.0, out, lse,
                            grad_out, nullptr, nullptr, grad_value, grad_score, workspace, workspace_bytes, stream);
}

}  // extern "C"
