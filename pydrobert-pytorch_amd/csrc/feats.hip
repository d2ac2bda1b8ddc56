// Feature deltas and mean/variance normalisation (reference _feats.py:29-251): the two
// streaming operators of the feature front end ahead of SpecAugment.
//
// Deltas.  x is indexed (A, B, T, C, D) with element strides; the output is written straight
// into its final contiguous layout (A, U, B, T, C, D) or (A, B, T, C, U, D) -- the order axis
// sits just before the axis the caller's `dim` names, so both `concatenate` forms are the same
// memory.  A workgroup stages a T-tile of one (a, b) row plus P = width * order halo rows across
// a span of the (c, d) columns in LDS (padding applied while staging), then every thread forms
// the U outputs of its column vector with the 1 + 2P taps (scalar loads: the tap index is
// uniform).  16-byte loads and stores when d is the unit-stride axis and the rows align.
// Backward is the adjoint written as a gather: one thread per input sample collects the
// correlations of its own position and of every padded position that copied it.  No atomics.
//
// Mean/variance.  x is (A, X, B) contiguous; statistics per index of X.  A two-stage float64
// reduction: fixed-order per-workgroup partials of sums shifted by a per-index pivot (the
// first sample of the index; zero for `accumulate`, which wants the raw sums), merged in a
// fixed order by one workgroup per index.  No float atomics, so every result is bit-identical
// run to run and stream to stream.  B == 1 (the common dim = -1) is a column reduction whose
// rows are read coalesced; B > 1 walks the (a, b) pairs of one index.  Apply and backward are
// elementwise passes with per-index coefficients.
#include "pdt_common.hpp"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

namespace pdt {

enum { FEATS_F32 = 0, FEATS_F64 = 1, FEATS_F16 = 2, FEATS_BF16 = 3 };
enum { DPAD_REPLICATE = 0, DPAD_REFLECT = 1, DPAD_CIRCULAR = 2, DPAD_CONSTANT = 3 };
enum { MVN_STATS = 0, MVN_ACCUM = 1, MVN_GRAD = 2 };

constexpr int kFeatThreads = 256;

// storage <-> compute conversions (float32 compute for the 16-bit types)
template <typename T> struct Cvt;
template <> struct Cvt<float> {
  using C = float;
  __device__ static float in(float v) { return v; }
  __device__ static float out(float v) { return v; }
};
template <> struct Cvt<double> {
  using C = double;
  __device__ static double in(double v) { return v; }
  __device__ static double out(double v) { return v; }
};
template <> struct Cvt<__half> {
  using C = float;
  __device__ static float in(__half v) { return __half2float(v); }
  __device__ static __half out(float v) { return __float2half(v); }
};
template <> struct Cvt<__hip_bfloat16> {
  using C = float;
  __device__ static float in(__hip_bfloat16 v) { return __bfloat162float(v); }
  __device__ static __hip_bfloat16 out(float v) { return __float2bfloat16(v); }
};

template <typename T, int V> struct alignas(sizeof(T) * V) Vec { T v[V]; };

// ------------------------------------------------------------------------------------------
// deltas

struct DeltaArgs {
  const void *x;
  const void *taps;   // (U, K) compute type
  const void *fill;   // one compute-type element (constant mode)
  void *out;
  int64_t A, B, T, C, D, E;             // E = C * D
  int64_t xs_a, xs_b, xs_t, xs_c, xs_d;  // element strides of x
  int64_t os_a, os_b, os_t, os_c, os_d, os_u;
  int U, P, K, mode;
  int EC, TT;                           // tile: columns (multiple of V), time rows
  int64_t e_tiles, t_tiles;
};

// index of x read by padded position j in [-P, T + P), or -1 for the constant
__device__ __forceinline__ int64_t delta_src(int64_t j, int64_t T, int mode) {
  if (j >= 0 && j < T) return j;
  switch (mode) {
    case DPAD_REPLICATE: return j < 0 ? 0 : T - 1;
    case DPAD_REFLECT: return j < 0 ? -j : 2 * (T - 1) - j;
    case DPAD_CIRCULAR: return j < 0 ? j + T : j - T;
    default: return -1;
  }
}

template <typename T, int V>
__global__ void __launch_bounds__(kFeatThreads) feat_deltas_kernel(const DeltaArgs a) {
  using CT = typename Cvt<T>::C;
  extern __shared__ __align__(16) unsigned char feats_smem[];
  CT *tile = reinterpret_cast<CT *>(feats_smem);
  const T *__restrict__ x = reinterpret_cast<const T *>(a.x);
  const CT *__restrict__ taps = reinterpret_cast<const CT *>(a.taps);
  T *__restrict__ out = reinterpret_cast<T *>(a.out);

  int64_t bid = blockIdx.x;
  const int64_t et = bid % a.e_tiles;
  bid /= a.e_tiles;
  const int64_t tt = bid % a.t_tiles;
  const int64_t row = bid / a.t_tiles;
  const int64_t ia = row / a.B, ib = row - ia * a.B;
  const int64_t e0 = et * a.EC, t0 = tt * a.TT;
  const int ecn = (int)min((int64_t)a.EC, a.E - e0);
  const int ttn = (int)min((int64_t)a.TT, a.T - t0);
  const int nvec = ecn / V, rows = ttn + 2 * a.P;
  const T *xrow = x + ia * a.xs_a + ib * a.xs_b;
  const CT fill = a.mode == DPAD_CONSTANT ? *reinterpret_cast<const CT *>(a.fill) : CT(0);

  for (int idx = threadIdx.x; idx < rows * nvec; idx += kFeatThreads) {
    const int r = idx / nvec, j = idx - r * nvec;
    const int64_t s = delta_src(t0 - a.P + r, a.T, a.mode);
    const int64_t e = e0 + (int64_t)j * V, c = e / a.D, d = e - c * a.D;
    CT *dst = tile + (int64_t)r * a.EC + j * V;
    if (s < 0) {
#pragma unroll
      for (int v = 0; v < V; ++v) dst[v] = fill;
    } else {
      const T *src = xrow + s * a.xs_t + c * a.xs_c + d * a.xs_d;
      if constexpr (V > 1) {
        const Vec<T, V> w = *reinterpret_cast<const Vec<T, V> *>(src);
#pragma unroll
        for (int v = 0; v < V; ++v) dst[v] = Cvt<T>::in(w.v[v]);
      } else {
        dst[0] = Cvt<T>::in(*src);
      }
    }
  }
  __syncthreads();

  const int K = a.K;
  for (int idx = threadIdx.x; idx < ttn * nvec; idx += kFeatThreads) {
    const int r = idx / nvec, j = idx - r * nvec;
    const int64_t e = e0 + (int64_t)j * V, c = e / a.D, d = e - c * a.D;
    T *o = out + ia * a.os_a + ib * a.os_b + (t0 + r) * a.os_t + c * a.os_c + d * a.os_d;
    const CT *col = tile + (int64_t)r * a.EC + j * V;
    for (int u0 = 0; u0 < a.U; u0 += 4) {
      CT acc[4][V];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[q][v] = CT(0);
      for (int k = 0; k < K; ++k) {
        CT w[V];
#pragma unroll
        for (int v = 0; v < V; ++v) w[v] = col[(int64_t)k * a.EC + v];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (u0 + q < a.U) {
            const CT f = taps[(u0 + q) * K + k];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[q][v] += f * w[v];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (u0 + q < a.U) {
          T *oq = o + (int64_t)(u0 + q) * a.os_u;
          if constexpr (V > 1) {
            Vec<T, V> w;
#pragma unroll
            for (int v = 0; v < V; ++v) w.v[v] = Cvt<T>::out(acc[q][v]);
            *reinterpret_cast<Vec<T, V> *>(oq) = w;
          } else {
            oq[0] = Cvt<T>::out(acc[q][0]);
          }
        }
      }
    }
  }
}

// The same outputs without LDS, one thread per (row, t, column): for halos too wide for a tile in 64 KiB
// (1 + 2P rows of one column vector beyond it).  Every tap reads x through L1 / L2.
template <typename T>
__global__ void __launch_bounds__(kFeatThreads) feat_deltas_direct_kernel(const DeltaArgs a, int64_t total) {
  using CT = typename Cvt<T>::C;
  const int64_t gid = (int64_t)blockIdx.x * kFeatThreads + threadIdx.x;
  if (gid >= total) return;
  const T *__restrict__ x = reinterpret_cast<const T *>(a.x);
  const CT *__restrict__ taps = reinterpret_cast<const CT *>(a.taps);
  const int64_t e = gid % a.E, rt = gid / a.E, t = rt % a.T, row = rt / a.T;
  const int64_t ia = row / a.B, ib = row - ia * a.B, c = e / a.D, d = e - c * a.D;
  const T *xc = x + ia * a.xs_a + ib * a.xs_b + c * a.xs_c + d * a.xs_d;
  T *o = reinterpret_cast<T *>(a.out) + ia * a.os_a + ib * a.os_b + t * a.os_t + c * a.os_c + d * a.os_d;
  const CT fill = a.mode == DPAD_CONSTANT ? *reinterpret_cast<const CT *>(a.fill) : CT(0);
  for (int u = 0; u < a.U; ++u) {
    CT acc = CT(0);
    for (int k = 0; k < a.K; ++k) {
      const int64_t s = delta_src(t + k - a.P, a.T, a.mode);
      acc += taps[u * a.K + k] * (s < 0 ? fill : Cvt<T>::in(xc[s * a.xs_t]));
    }
    o[(int64_t)u * a.os_u] = Cvt<T>::out(acc);
  }
}

// sum over u, k of taps[u, k] * g_u[j + P - k] (the t inside [0, T))
template <typename CT, typename T>
__device__ __forceinline__ CT delta_adjoint_at(const DeltaArgs &a, const T *g, const CT *taps, int64_t j) {
  const int64_t klo = max((int64_t)0, j + a.P - a.T + 1), khi = min((int64_t)a.K - 1, j + a.P);
  CT acc = CT(0);
  for (int u = 0; u < a.U; ++u) {
    const T *gu = g + (int64_t)u * a.os_u;
    for (int64_t k = klo; k <= khi; ++k) acc += taps[u * a.K + k] * Cvt<T>::in(gu[(j + a.P - k) * a.os_t]);
  }
  return acc;
}

// grad_x (A, B, T, C, D) contiguous, one thread per sample; grad_out in the forward's layout
template <typename T>
__global__ void __launch_bounds__(kFeatThreads) feat_deltas_backward_kernel(const DeltaArgs a, int64_t total) {
  using CT = typename Cvt<T>::C;
  const int64_t gid = (int64_t)blockIdx.x * kFeatThreads + threadIdx.x;
  if (gid >= total) return;
  const T *__restrict__ go = reinterpret_cast<const T *>(a.x);
  const CT *__restrict__ taps = reinterpret_cast<const CT *>(a.taps);
  const int64_t e = gid % a.E, rt = gid / a.E, s = rt % a.T, row = rt / a.T;
  const int64_t ia = row / a.B, ib = row - ia * a.B, c = e / a.D, d = e - c * a.D;
  const T *g = go + ia * a.os_a + ib * a.os_b + c * a.os_c + d * a.os_d;
  const int64_t T_ = a.T, P = a.P;
  CT acc = delta_adjoint_at<CT>(a, g, taps, s);
  if (a.mode == DPAD_REPLICATE) {
    // the P copies of an end sample are summed on their own: each is far smaller than the sample's own
    // term, and added to it one by one a wide halo's copies round away (1e-4 of the gradient at P = 8191)
    CT edge = CT(0);
    if (s == 0)
      for (int64_t j = -P; j < 0; ++j) edge += delta_adjoint_at<CT>(a, g, taps, j);
    if (s == T_ - 1)
      for (int64_t j = T_; j < T_ + P; ++j) edge += delta_adjoint_at<CT>(a, g, taps, j);
    acc += edge;
  } else if (a.mode == DPAD_REFLECT) {
    if (s >= 1 && s <= P) acc += delta_adjoint_at<CT>(a, g, taps, -s);
    if (s <= T_ - 2 && s >= T_ - 1 - P) acc += delta_adjoint_at<CT>(a, g, taps, 2 * (T_ - 1) - s);
  } else if (a.mode == DPAD_CIRCULAR) {
    if (s - T_ >= -P) acc += delta_adjoint_at<CT>(a, g, taps, s - T_);
    if (s + T_ < T_ + P) acc += delta_adjoint_at<CT>(a, g, taps, s + T_);
  }
  reinterpret_cast<T *>(a.out)[gid] = Cvt<T>::out(acc);
}

// ------------------------------------------------------------------------------------------
// mean / variance

struct MvnArgs {
  const void *x, *g, *m;  // (A, X, B) contiguous; m (X,) in x's dtype (MVN_GRAD)
  int64_t A, X, B;
  int64_t splits, per_split;  // per_split: rows (B == 1) or (a, b) pairs (B > 1) per workgroup
  double *ws;                 // (splits, X, 2)
};

// the pair a sample contributes: (x - p, (x - p)^2) or (g, g * c) with c = x - m in x's dtype
template <typename T, int MODE>
__device__ __forceinline__ void mvn_terms(const MvnArgs &a, int64_t off, double p, typename Cvt<T>::C m,
                                          double &s1, double &s2) {
  const T *x = reinterpret_cast<const T *>(a.x);
  if constexpr (MODE == MVN_GRAD) {
    const double g = (double)Cvt<T>::in(reinterpret_cast<const T *>(a.g)[off]);
    const double c = (double)Cvt<T>::in(Cvt<T>::out(Cvt<T>::in(x[off]) - m));
    s1 += g;
    s2 += g * c;
  } else {
    const double v = (double)Cvt<T>::in(x[off]) - p;
    s1 += v;
    s2 += v * v;
  }
}

template <typename T, int MODE>
__device__ __forceinline__ void mvn_index_setup(const MvnArgs &a, int64_t i, double &p, typename Cvt<T>::C &m) {
  p = 0.0;
  m = 0;
  if constexpr (MODE == MVN_STATS) p = (double)Cvt<T>::in(reinterpret_cast<const T *>(a.x)[i * a.B]);
  if constexpr (MODE == MVN_GRAD) m = Cvt<T>::in(reinterpret_cast<const T *>(a.m)[i]);
}

// B == 1: grid (column tiles, splits); RP rows of CW columns per sweep, 4 sweeps in flight
template <typename T, int MODE>
__global__ void __launch_bounds__(kFeatThreads) mvn_partial_cols(const MvnArgs a) {
  __shared__ double red[2][kFeatThreads];
  const int CW = (int)min(a.X, (int64_t)kFeatThreads), RP = kFeatThreads / CW;
  const int r = threadIdx.x / CW, cc = threadIdx.x - r * CW;
  const int64_t col = (int64_t)blockIdx.x * CW + cc;
  const int64_t a0 = (int64_t)blockIdx.y * a.per_split, a1 = min(a.A, a0 + a.per_split);
  double s1 = 0.0, s2 = 0.0;
  if (r < RP && col < a.X) {
    double p;
    typename Cvt<T>::C m;
    mvn_index_setup<T, MODE>(a, col, p, m);
    int64_t row = a0 + r;
    for (; row + 3 * RP < a1; row += 4 * RP) {
#pragma unroll
      for (int q = 0; q < 4; ++q) mvn_terms<T, MODE>(a, (row + q * RP) * a.X + col, p, m, s1, s2);
    }
    for (; row < a1; row += RP) mvn_terms<T, MODE>(a, row * a.X + col, p, m, s1, s2);
  }
  red[0][threadIdx.x] = s1;
  red[1][threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x < CW && col < a.X) {
    for (int q = 1; q < RP; ++q) {
      s1 += red[0][q * CW + threadIdx.x];
      s2 += red[1][q * CW + threadIdx.x];
    }
    double *w = a.ws + (blockIdx.y * a.X + col) * 2;
    w[0] = s1;
    w[1] = s2;
  }
}

// fixed-order tree sum of both rows of red[][] into red[.][0]
__device__ __forceinline__ void block_tree_sum(double (*red)[kFeatThreads]) {
  for (int h = kFeatThreads / 2; h > 0; h >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
    }
  }
  __syncthreads();
}

// B > 1: grid (X, splits); the workgroup walks a range of the (a, b) pairs of one index
template <typename T, int MODE>
__global__ void __launch_bounds__(kFeatThreads) mvn_partial_inner(const MvnArgs a) {
  __shared__ double red[2][kFeatThreads];
  const int64_t i = blockIdx.x, M = a.A * a.B;
  const int64_t m0 = (int64_t)blockIdx.y * a.per_split, m1 = min(M, m0 + a.per_split);
  double p;
  typename Cvt<T>::C m;
  mvn_index_setup<T, MODE>(a, i, p, m);
  double s1 = 0.0, s2 = 0.0;
  int64_t mm = m0 + threadIdx.x;
  if (mm < m1) {
    int64_t ia = mm / a.B, ib = mm - ia * a.B;
    const int64_t da = kFeatThreads / a.B, db = kFeatThreads - da * a.B;
    for (; mm < m1; mm += kFeatThreads) {
      mvn_terms<T, MODE>(a, (ia * a.X + i) * a.B + ib, p, m, s1, s2);
      ia += da;
      ib += db;
      if (ib >= a.B) ib -= a.B, ++ia;
    }
  }
  red[0][threadIdx.x] = s1;
  red[1][threadIdx.x] = s2;
  block_tree_sum(red);
  if (threadIdx.x == 0) {
    double *w = a.ws + (blockIdx.y * a.X + i) * 2;
    w[0] = red[0][0];
    w[1] = red[1][0];
  }
}

// one workgroup per index: the partials in a fixed order, then what the mode asks for
template <typename T, int MODE>
__global__ void __launch_bounds__(kFeatThreads)
mvn_finalize(const MvnArgs a, double *out0, double *out1, double *count) {
  __shared__ double red[2][kFeatThreads];
  const int64_t i = blockIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t s = threadIdx.x; s < a.splits; s += kFeatThreads) {
    s1 += a.ws[(s * a.X + i) * 2];
    s2 += a.ws[(s * a.X + i) * 2 + 1];
  }
  red[0][threadIdx.x] = s1;
  red[1][threadIdx.x] = s2;
  block_tree_sum(red);
  if (threadIdx.x != 0) return;
  s1 = red[0][0];
  s2 = red[1][0];
  const double n = (double)(a.A * a.B);
  if constexpr (MODE == MVN_STATS) {
    double p;
    typename Cvt<T>::C m;
    mvn_index_setup<T, MODE>(a, i, p, m);
    out0[i] = p + s1 / n;
    out1[i] = sqrt(fmax(s2 - s1 * (s1 / n), 0.0) / n);
  } else if constexpr (MODE == MVN_ACCUM) {
    out0[i] += s1;
    out1[i] += s2;
    if (i == 0) count[0] += n;
  } else {
    out0[i] = s1;
    out1[i] = s2;
  }
}

// y = (x - m[i]) / s[i], the difference rounded to x's dtype first (as the reference does)
template <typename T>
__global__ void __launch_bounds__(kFeatThreads)
mvn_apply_kernel(const T *__restrict__ x, const T *__restrict__ mean, const T *__restrict__ scale,
                 T *__restrict__ y, int64_t X, int64_t B, int64_t total) {
  const int64_t gid = (int64_t)blockIdx.x * kFeatThreads + threadIdx.x;
  if (gid >= total) return;
  const int64_t i = (gid / B) % X;
  const typename Cvt<T>::C c = Cvt<T>::in(Cvt<T>::out(Cvt<T>::in(x[gid]) - Cvt<T>::in(mean[i])));
  y[gid] = Cvt<T>::out(c / Cvt<T>::in(scale[i]));
}

// the same with 16-byte accesses: B == 1, total a multiple of V, 16-byte aligned pointers
template <typename T, int V>
__global__ void __launch_bounds__(kFeatThreads)
mvn_apply_rows_kernel(const T *__restrict__ x, const T *__restrict__ mean, const T *__restrict__ scale,
                      T *__restrict__ y, int64_t X, int64_t nvec) {
  const int64_t gid = (int64_t)blockIdx.x * kFeatThreads + threadIdx.x;
  if (gid >= nvec) return;
  int64_t i = (gid * V) % X;
  const Vec<T, V> w = reinterpret_cast<const Vec<T, V> *>(x)[gid];
  Vec<T, V> o;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const typename Cvt<T>::C c = Cvt<T>::in(Cvt<T>::out(Cvt<T>::in(w.v[v]) - Cvt<T>::in(mean[i])));
    o.v[v] = Cvt<T>::out(c / Cvt<T>::in(scale[i]));
    if (++i == X) i = 0;
  }
  reinterpret_cast<Vec<T, V> *>(y)[gid] = o;
}

// grad_x = g * coef[0, i] + coef[1, i] + coef[2, i] * (x - m[i]); coef in the compute type
template <typename T>
__global__ void __launch_bounds__(kFeatThreads)
mvn_backward_kernel(const T *__restrict__ g, const T *__restrict__ x, const T *__restrict__ mean,
                    const typename Cvt<T>::C *__restrict__ coef, T *__restrict__ gx, int64_t X, int64_t B,
                    int64_t total) {
  using CT = typename Cvt<T>::C;
  const int64_t gid = (int64_t)blockIdx.x * kFeatThreads + threadIdx.x;
  if (gid >= total) return;
  const int64_t i = (gid / B) % X;
  const CT c = Cvt<T>::in(Cvt<T>::out(Cvt<T>::in(x[gid]) - Cvt<T>::in(mean[i])));
  gx[gid] = Cvt<T>::out(Cvt<T>::in(g[gid]) * coef[i] + coef[X + i] + coef[2 * X + i] * c);
}

static int64_t mvn_splits(int64_t A, int64_t X, int64_t B, int64_t *per_split) {
  int64_t splits;
  if (B == 1) {
    const int64_t CW = std::min<int64_t>(X, kFeatThreads), RP = kFeatThreads / CW;
    const int64_t tiles = (X + CW - 1) / CW;
    splits = std::max<int64_t>(1, std::min<int64_t>((A + RP * 32 - 1) / (RP * 32), std::max<int64_t>(1, 2048 / tiles)));
    *per_split = (A + splits - 1) / splits;
  } else {
    const int64_t M = A * B;
    splits = std::max<int64_t>(1, std::min<int64_t>((M + 8191) / 8192, std::max<int64_t>(1, 2048 / X)));
    *per_split = (M + splits - 1) / splits;
  }
  return splits;
}

template <typename T>
static int mvn_stats_launch(const MvnArgs &a, int mode, double *out0, double *out1, double *count, hipStream_t s) {
  const dim3 blk(kFeatThreads);
  const int64_t CW = std::min<int64_t>(a.X, kFeatThreads);
  const dim3 grid1 = a.B == 1 ? dim3((unsigned)((a.X + CW - 1) / CW), (unsigned)a.splits)
                              : dim3((unsigned)a.X, (unsigned)a.splits);
#define PDT_MVN_CASE(MODE)                                                                  \
  if (a.B == 1) hipLaunchKernelGGL((mvn_partial_cols<T, MODE>), grid1, blk, 0, s, a);       \
  else hipLaunchKernelGGL((mvn_partial_inner<T, MODE>), grid1, blk, 0, s, a);               \
  hipLaunchKernelGGL((mvn_finalize<T, MODE>), dim3((unsigned)a.X), blk, 0, s, a, out0, out1, count);
  switch (mode) {
    case MVN_STATS: PDT_MVN_CASE(MVN_STATS) break;
    case MVN_ACCUM: PDT_MVN_CASE(MVN_ACCUM) break;
    default: PDT_MVN_CASE(MVN_GRAD) break;
  }
#undef PDT_MVN_CASE
  return (int)hipGetLastError();
}

static int feats_grid(int64_t total, unsigned *blocks) {
  const int64_t b = (total + kFeatThreads - 1) / kFeatThreads;
  if (b > 0x7fffffffll) return PDT_E_TOO_LONG;
  *blocks = (unsigned)b;
  return PDT_OK;
}

}  // namespace pdt

extern "C" {

int pdt_feat_deltas(const void *x, int dtype, int64_t A, int64_t B, int64_t T, int64_t C, int64_t D,
                    int64_t xs_a, int64_t xs_b, int64_t xs_t, int64_t xs_c, int64_t xs_d, const void *taps,
                    int64_t U, int64_t P, int mode, const void *fill, int u_inner, void *out, void *stream) {
  using namespace pdt;
  if (A < 0 || B < 0 || T < 0 || C < 0 || D < 0 || U < 1 || P < 0 || mode < 0 || mode > 3) return PDT_E_ARG;
  if (dtype < FEATS_F32 || dtype > FEATS_BF16) return PDT_E_ARG;
  if (T == 0) return PDT_E_ARG;  // (the reference's padding / conv1d raise on an empty time axis)
  if ((mode == DPAD_REFLECT && P >= T) || (mode == DPAD_CIRCULAR && P > T)) return PDT_E_ARG;
  const int64_t E = C * D;
  if (A == 0 || B == 0 || E == 0) return PDT_OK;
  if (!x || !taps || !out || (mode == DPAD_CONSTANT && !fill)) return PDT_E_ARG;
  const int esz = dtype == FEATS_F64 ? 8 : dtype == FEATS_F32 ? 4 : 2;
  const int csz = dtype == FEATS_F64 ? 8 : 4;
  const int V = 16 / esz;
  const bool vec = D % V == 0 && xs_d == 1 && xs_c % V == 0 && xs_t % V == 0 && xs_b % V == 0 &&
                   xs_a % V == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0;
  const int vw = vec ? V : 1;
  DeltaArgs a{};
  a.x = x; a.taps = taps; a.fill = fill; a.out = out;
  a.A = A; a.B = B; a.T = T; a.C = C; a.D = D; a.E = E;
  a.xs_a = xs_a; a.xs_b = xs_b; a.xs_t = xs_t; a.xs_c = xs_c; a.xs_d = xs_d;
  a.os_d = 1;
  if (u_inner) {  // (A, B, T, C, U, D)
    a.os_u = D; a.os_c = U * D; a.os_t = C * U * D; a.os_b = T * C * U * D; a.os_a = B * a.os_b;
  } else {        // (A, U, B, T, C, D)
    a.os_c = D; a.os_t = C * D; a.os_b = T * C * D; a.os_u = B * a.os_b; a.os_a = U * a.os_u;
  }
  a.U = (int)U; a.P = (int)P; a.K = (int)(1 + 2 * P); a.mode = mode;
  hipStream_t s = (hipStream_t)stream;
  if ((1 + 2 * P) * vw * csz > 65536) {  // no tile fits: the kernel without LDS
    if (P > (1 << 28)) return PDT_E_TOO_LONG;
    const int64_t total = A * B * T * E;
    unsigned nb;
    if (feats_grid(total, &nb) != PDT_OK) return PDT_E_TOO_LONG;
    const dim3 g(nb), b(kFeatThreads);
    switch (dtype) {
      case FEATS_F32: hipLaunchKernelGGL(feat_deltas_direct_kernel<float>, g, b, 0, s, a, total); break;
      case FEATS_F64: hipLaunchKernelGGL(feat_deltas_direct_kernel<double>, g, b, 0, s, a, total); break;
      case FEATS_F16: hipLaunchKernelGGL(feat_deltas_direct_kernel<__half>, g, b, 0, s, a, total); break;
      default: hipLaunchKernelGGL(feat_deltas_direct_kernel<__hip_bfloat16>, g, b, 0, s, a, total); break;
    }
    return (int)hipGetLastError();
  }
  // tile: up to 64 column vectors, ~4096 samples, in at most 64 KiB of LDS
  int64_t EC = std::min<int64_t>(E, 64 * vw);
  if (vw > 1) EC -= EC % vw;
  int64_t TT = std::max<int64_t>(1, std::min<int64_t>(T, 4096 / EC));
  while ((TT + 2 * P) * EC * csz > 65536) {  // (terminates: one row of 1 + 2P vectors fits, checked above)
    if (TT > 8) TT /= 2;
    else if (EC > vw) EC = std::max<int64_t>(vw, (EC / 2) - (EC / 2) % vw);
    else TT = 1;
  }
  a.EC = (int)EC; a.TT = (int)TT;
  a.e_tiles = (E + EC - 1) / EC;
  a.t_tiles = (T + TT - 1) / TT;
  const int64_t blocks = A * B * a.t_tiles * a.e_tiles;
  if (blocks > 0x7fffffffll) return PDT_E_TOO_LONG;
  const size_t lds = (size_t)((TT + 2 * P) * EC * csz);
  const dim3 grid((unsigned)blocks), blk(kFeatThreads);
  switch (dtype * 2 + (vec ? 1 : 0)) {
    case FEATS_F32 * 2: hipLaunchKernelGGL((feat_deltas_kernel<float, 1>), grid, blk, lds, s, a); break;
    case FEATS_F32 * 2 + 1: hipLaunchKernelGGL((feat_deltas_kernel<float, 4>), grid, blk, lds, s, a); break;
    case FEATS_F64 * 2: hipLaunchKernelGGL((feat_deltas_kernel<double, 1>), grid, blk, lds, s, a); break;
    case FEATS_F64 * 2 + 1: hipLaunchKernelGGL((feat_deltas_kernel<double, 2>), grid, blk, lds, s, a); break;
    case FEATS_F16 * 2: hipLaunchKernelGGL((feat_deltas_kernel<__half, 1>), grid, blk, lds, s, a); break;
    case FEATS_F16 * 2 + 1: hipLaunchKernelGGL((feat_deltas_kernel<__half, 8>), grid, blk, lds, s, a); break;
    case FEATS_BF16 * 2: hipLaunchKernelGGL((feat_deltas_kernel<__hip_bfloat16, 1>), grid, blk, lds, s, a); break;
    default: hipLaunchKernelGGL((feat_deltas_kernel<__hip_bfloat16, 8>), grid, blk, lds, s, a); break;
  }
  return (int)hipGetLastError();
}

int pdt_feat_deltas_backward(const void *grad_out, int dtype, int64_t A, int64_t B, int64_t T, int64_t C,
                             int64_t D, const void *taps, int64_t U, int64_t P, int mode, int u_inner,
                             void *grad_x, void *stream) {
  using namespace pdt;
  if (A < 0 || B < 0 || T < 0 || C < 0 || D < 0 || U < 1 || P < 0 || mode < 0 || mode > 3) return PDT_E_ARG;
  if (dtype < FEATS_F32 || dtype > FEATS_BF16) return PDT_E_ARG;
  if (T == 0) return PDT_E_ARG;
  if ((mode == DPAD_REFLECT && P >= T) || (mode == DPAD_CIRCULAR && P > T)) return PDT_E_ARG;
  const int64_t E = C * D, total = A * B * T * E;
  if (total == 0) return PDT_OK;
  if (!grad_out || !taps || !grad_x) return PDT_E_ARG;
  DeltaArgs a{};
  a.x = grad_out; a.taps = taps; a.out = grad_x;
  a.A = A; a.B = B; a.T = T; a.C = C; a.D = D; a.E = E;
  a.os_d = 1;
  if (u_inner) {
    a.os_u = D; a.os_c = U * D; a.os_t = C * U * D; a.os_b = T * C * U * D; a.os_a = B * a.os_b;
  } else {
    a.os_c = D; a.os_t = C * D; a.os_b = T * C * D; a.os_u = B * a.os_b; a.os_a = U * a.os_u;
  }
  a.U = (int)U; a.P = (int)P; a.K = (int)(1 + 2 * P); a.mode = mode;
  unsigned blocks;
  if (feats_grid(total, &blocks) != PDT_OK) return PDT_E_TOO_LONG;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case FEATS_F32: hipLaunchKernelGGL(feat_deltas_backward_kernel<float>, dim3(blocks), dim3(kFeatThreads), 0, s, a, total); break;
    case FEATS_F64: hipLaunchKernelGGL(feat_deltas_backward_kernel<double>, dim3(blocks), dim3(kFeatThreads), 0, s, a, total); break;
    case FEATS_F16: hipLaunchKernelGGL(feat_deltas_backward_kernel<__half>, dim3(blocks), dim3(kFeatThreads), 0, s, a, total); break;
    default: hipLaunchKernelGGL(feat_deltas_backward_kernel<__hip_bfloat16>, dim3(blocks), dim3(kFeatThreads), 0, s, a, total); break;
  }
  return (int)hipGetLastError();
}

int64_t pdt_mvn_stats_workspace_bytes(int64_t A, int64_t X, int64_t B) {
  if (A <= 0 || X <= 0 || B <= 0) return 0;
  int64_t per;
  return pdt::mvn_splits(A, X, B, &per) * X * 2 * (int64_t)sizeof(double);
}

int pdt_mvn_stats(const void *x, const void *g, const void *mean, int dtype, int64_t A, int64_t X, int64_t B,
                  int mode, double *out0, double *out1, double *count, void *workspace, int64_t workspace_bytes,
                  void *stream) {
  using namespace pdt;
  if (A < 0 || X < 0 || B < 0 || mode < MVN_STATS || mode > MVN_GRAD) return PDT_E_ARG;
  if (dtype < FEATS_F32 || dtype > FEATS_BF16) return PDT_E_ARG;
  if (X == 0) return PDT_OK;
  if (!out0 || !out1 || (mode == MVN_ACCUM && !count)) return PDT_E_ARG;
  if (A == 0 || B == 0) {
    if (mode != MVN_ACCUM) return PDT_E_ARG;  // (statistics of nothing)
    return PDT_OK;
  }
  if (!x || (mode == MVN_GRAD && (!g || !mean))) return PDT_E_ARG;
  if (workspace_bytes < pdt_mvn_stats_workspace_bytes(A, X, B) || !workspace) return PDT_E_ARG;
  if (X > 0x7fffffffll) return PDT_E_TOO_LONG;
  MvnArgs a{};
  a.x = x; a.g = g; a.m = mean; a.A = A; a.X = X; a.B = B;
  a.splits = mvn_splits(A, X, B, &a.per_split);
  a.ws = reinterpret_cast<double *>(workspace);
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case FEATS_F32: return mvn_stats_launch<float>(a, mode, out0, out1, count, s);
    case FEATS_F64: return mvn_stats_launch<double>(a, mode, out0, out1, count, s);
    case FEATS_F16: return mvn_stats_launch<__half>(a, mode, out0, out1, count, s);
    default: return mvn_stats_launch<__hip_bfloat16>(a, mode, out0, out1, count, s);
  }
}

int pdt_mvn_apply(const void *x, int dtype, int64_t A, int64_t X, int64_t B, const void *mean, const void *scale,
                  void *y, void *stream) {
  using namespace pdt;
  if (A < 0 || X < 0 || B < 0 || dtype < FEATS_F32 || dtype > FEATS_BF16) return PDT_E_ARG;
  const int64_t total = A * X * B;
  if (total == 0) return PDT_OK;
  if (!x || !mean || !scale || !y) return PDT_E_ARG;
  const int esz = dtype == FEATS_F64 ? 8 : dtype == FEATS_F32 ? 4 : 2, V = 16 / esz;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kFeatThreads);
  unsigned blocks;
  if (B == 1 && total % V == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0) {
    if (feats_grid(total / V, &blocks) != PDT_OK) return PDT_E_TOO_LONG;
    const int64_t nv = total / V;
    switch (dtype) {
      case FEATS_F32: hipLaunchKernelGGL((mvn_apply_rows_kernel<float, 4>), dim3(blocks), blk, 0, s, (const float *)x, (const float *)mean, (const float *)scale, (float *)y, X, nv); break;
      case FEATS_F64: hipLaunchKernelGGL((mvn_apply_rows_kernel<double, 2>), dim3(blocks), blk, 0, s, (const double *)x, (const double *)mean, (const double *)scale, (double *)y, X, nv); break;
      case FEATS_F16: hipLaunchKernelGGL((mvn_apply_rows_kernel<__half, 8>), dim3(blocks), blk, 0, s, (const __half *)x, (const __half *)mean, (const __half *)scale, (__half *)y, X, nv); break;
      default: hipLaunchKernelGGL((mvn_apply_rows_kernel<__hip_bfloat16, 8>), dim3(blocks), blk, 0, s, (const __hip_bfloat16 *)x, (const __hip_bfloat16 *)mean, (const __hip_bfloat16 *)scale, (__hip_bfloat16 *)y, X, nv); break;
    }
    return (int)hipGetLastError();
  }
  if (feats_grid(total, &blocks) != PDT_OK) return PDT_E_TOO_LONG;
  switch (dtype) {
    case FEATS_F32: hipLaunchKernelGGL(mvn_apply_kernel<float>, dim3(blocks), blk, 0, s, (const float *)x, (const float *)mean, (const float *)scale, (float *)y, X, B, total); break;
    case FEATS_F64: hipLaunchKernelGGL(mvn_apply_kernel<double>, dim3(blocks), blk, 0, s, (const double *)x, (const double *)mean, (const double *)scale, (double *)y, X, B, total); break;
    case FEATS_F16: hipLaunchKernelGGL(mvn_apply_kernel<__half>, dim3(blocks), blk, 0, s, (const __half *)x, (const __half *)mean, (const __half *)scale, (__half *)y, X, B, total); break;
    default: hipLaunchKernelGGL(mvn_apply_kernel<__hip_bfloat16>, dim3(blocks), blk, 0, s, (const __hip_bfloat16 *)x, (const __hip_bfloat16 *)mean, (const __hip_bfloat16 *)scale, (__hip_bfloat16 *)y, X, B, total); break;
  }
  return (int)hipGetLastError();
}

int pdt_mvn_backward(const void *grad_y, const void *x, int dtype, int64_t A, int64_t X, int64_t B, const void *mean,
                     const void *coef, void *grad_x, void *stream) {
  using namespace pdt;
  if (A < 0 || X < 0 || B < 0 || dtype < FEATS_F32 || dtype > FEATS_BF16) return PDT_E_ARG;
  const int64_t total = A * X * B;
  if (total == 0) return PDT_OK;
  if (!grad_y || !x || !mean || !coef || !grad_x) return PDT_E_ARG;
  unsigned blocks;
  if (feats_grid(total, &blocks) != PDT_OK) return PDT_E_TOO_LONG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kFeatThreads);
  switch (dtype) {
    case FEATS_F32: hipLaunchKernelGGL(mvn_backward_kernel<float>, dim3(blocks), blk, 0, s, (const float *)grad_y, (const float *)x, (const float *)mean, (const float *)coef, (float *)grad_x, X, B, total); break;
    case FEATS_F64: hipLaunchKernelGGL(mvn_backward_kernel<double>, dim3(blocks), blk, 0, s, (const double *)grad_y, (const double *)x, (const double *)mean, (const double *)coef, (double *)grad_x, X, B, total); break;
    case FEATS_F16: hipLaunchKernelGGL(mvn_backward_kernel<__half>, dim3(blocks), blk, 0, s, (const __half *)grad_y, (const __half *)x, (const __half *)mean, (const float *)coef, (__half *)grad_x, X, B, total); break;
    default: hipLaunchKernelGGL(mvn_backward_kernel<__hip_bfloat16>, dim3(blocks), blk, 0, s, (const __hip_bfloat16 *)grad_y, (const __hip_bfloat16 *)x, (const __hip_bfloat16 *)mean, (const float *)coef, (__hip_bfloat16 *)grad_x, X, B, total); break;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
