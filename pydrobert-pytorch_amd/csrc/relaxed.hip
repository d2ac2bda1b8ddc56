// Relaxed sampling (reference _straight_through.py:251-598): the six methods of the Gumbel / one-hot
// categorical relaxation and of the logistic / Bernoulli one, each as ONE pass over a row where the
// reference chains six to fifteen elementwise passes and up to two row reductions.
//
// Data are rows of V elements, R of them, dense; sample row r reads parameter row r mod B through
// element strides (p_sr, p_sv), so an expanded parameter (stride 0) is read in place.  A row belongs to
// a GROUP of G adjacent lanes, G the power of two at or above V, 64 at most (group_width): rows of up
// to 32 elements share a wave (64 / G rows of it), longer ones get a wave each and its lanes stride
// over the row.  Reductions are xor butterflies inside the group, so every lane of it holds the result.
// Every array is read once: where a method needs a number of the hot element before it can visit the
// others (csample: log v_k; clog_prob: zcond_k) the pass over b that finds k comes first and the one
// element is loaded on its own.  Nothing is kept between passes, so no row width changes the form
// of a kernel beyond the group widths and the first row that takes more than one trip (V > 64).
//
// The arithmetic is the reference's, operation for operation, in the data's own type (float32 or
// float64): the same clamps at the type's eps, the same `min` guard, the same `+ b * eps`.
//
// The backward of every differentiable method is a kernel of its own further down ("backward"): the
// gradient of the relaxed sample, and the gradient of the parameter summed over the sample rows in
// the launch.
#include "pdt_common.hpp"

#include <cmath>
#include <limits>

namespace pdt {
namespace {

enum { RLX_F32 = 0, RLX_F64 = 1 };
enum { RLX_RSAMPLE = 0, RLX_THRESHOLD, RLX_TLOG_PROB, RLX_CSAMPLE, RLX_LOG_PROB, RLX_CLOG_PROB, RLX_OPS };

constexpr int kRelaxedThreads = 256;
constexpr int kNoIndex = 0x7fffffff;

template <typename T> struct RelaxedArgs {
  const T *param;  // logits, or probs for csample: (B, V) through (p_sr, p_sv)
  const T *in1;    // (R, V)
  const T *in2;    // (R, V), the methods of two data arguments
  T *out;          // (R, V), or (R,) for the Gumbel *log_prob
  int64_t B, p_sr, p_sv, R;
  int V, G;
};

int group_width(int64_t V) {
  int g = 1;
  while (g < PDT_WAVE && g < V) g <<= 1;
  return g;
}

template <typename T> __device__ __forceinline__ T eps_of() { return std::numeric_limits<T>::epsilon(); }
// clamp_probs: a NaN stays a NaN
template <typename T> __device__ __forceinline__ T clamp_unit(T x) {
  const T lo = eps_of<T>(), hi = T(1) - eps_of<T>();
  return x < lo ? lo : (x > hi ? hi : x);
}
__device__ __forceinline__ float log_(float x) { return logf(x); }
__device__ __forceinline__ double log_(double x) { return log(x); }
__device__ __forceinline__ float exp_(float x) { return expf(x); }
__device__ __forceinline__ double exp_(double x) { return exp(x); }
__device__ __forceinline__ float log1p_(float x) { return log1pf(x); }
__device__ __forceinline__ double log1p_(double x) { return log1p(x); }

template <typename T> __device__ __forceinline__ T group_sum(T v, const int G) {
  for (int o = G >> 1; o; o >>= 1) v += __shfl_xor(v, o, PDT_WAVE);
  return v;
}
__device__ __forceinline__ int group_min(int v, const int G) {
  for (int o = G >> 1; o; o >>= 1) {
    const int w = __shfl_xor(v, o, PDT_WAVE);
    v = w < v ? w : v;
  }
  return v;
}
// does (a, ia) precede (b, ib) as the arg-max?  A NaN is the maximum, equal values (-0 == +0) go to
// the lower index.
template <typename T> __device__ __forceinline__ bool arg_before(T a, int ia, T b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}
template <typename T> __device__ __forceinline__ void group_argmax(T &val, int &idx, const int G) {
  for (int o = G >> 1; o; o >>= 1) {
    const T v = __shfl_xor(val, o, PDT_WAVE);
    const int i = __shfl_xor(idx, o, PDT_WAVE);
    if (arg_before(v, i, val, idx)) val = v, idx = i;
  }
}
template <typename T> __device__ __forceinline__ int row_argmax(const T *__restrict__ z, int V, int G, int sub, T *at) {
  T best = -std::numeric_limits<T>::infinity();
  int idx = kNoIndex;
#pragma unroll 4
  for (int j = sub; j < V; j += G) {
    const T x = z[j];
    if (arg_before(x, j, best, idx)) best = x, idx = j;
  }
  group_argmax(best, idx, G);
  if (at) *at = best;
  return idx;
}
// the first nonzero of b (kNoIndex: none), and whether b is exactly one 1 among zeros
template <typename T> __device__ __forceinline__ int row_hot(const T *__restrict__ b, int V, int G, int sub, bool *one_hot) {
  int k = kNoIndex, other = 0;
#pragma unroll 4
  for (int j = sub; j < V; j += G) {
    const T x = b[j];
    if (x != T(0)) {
      other += (k != kNoIndex) | (x != T(1));
      k = k == kNoIndex ? j : k;
    }
  }
  const int first = group_min(k, G);
  if (one_hot) {
    other += k != kNoIndex && k != first;
    *one_hot = first != kNoIndex && group_sum(other, G) == 0;
  }
  return first;
}

// ---- Gumbel / one-hot categorical --------------------------------------------------------------
template <typename T, int OP>
__global__ void __launch_bounds__(kRelaxedThreads) gumbel_kernel(const RelaxedArgs<T> a) {
  const int G = a.G, V = a.V;
  const int sub = (int)threadIdx.x & (G - 1);
  const int64_t r = (int64_t)blockIdx.x * (kRelaxedThreads / G) + ((int)threadIdx.x / G);
  if (r >= a.R) return;  // (a whole group leaves together)
  const T *__restrict__ p = a.param ? a.param + (r % a.B) * a.p_sr : nullptr;
  const T *__restrict__ x1 = a.in1 + r * V;
  const T *__restrict__ x2 = a.in2 ? a.in2 + r * V : nullptr;
  const T eps = eps_of<T>();
  if (OP == RLX_RSAMPLE) {
    T *__restrict__ z = a.out + r * V;
#pragma unroll 4
    for (int j = sub; j < V; j += G) z[j] = p[(int64_t)j * a.p_sv] - log_(-log_(clamp_unit(x1[j])));
  } else if (OP == RLX_THRESHOLD) {
    T *__restrict__ b = a.out + r * V;
    const int k = row_argmax<T>(x1, V, G, sub, nullptr);
#pragma unroll 4
    for (int j = sub; j < V; j += G) b[j] = j == k ? T(1) : T(0);
  } else if (OP == RLX_TLOG_PROB) {
    T s = T(0);
#pragma unroll 4
    for (int j = sub; j < V; j += G)
      if (x1[j] != T(0)) s += p[(int64_t)j * a.p_sv];
    s = group_sum(s, G);
    if (sub == 0) a.out[r] = s;
  } else if (OP == RLX_CSAMPLE) {
    T *__restrict__ z = a.out + r * V;
    const int k = row_hot<T>(x1, V, G, sub, nullptr);
    // (no hot element: the reference's sums over b are empty, z_k = 0 and log v_k = 0)
    const T lvk = k == kNoIndex ? T(0) : log_(clamp_unit(x2[k]));
    const T zk = k == kNoIndex ? T(0) : -log_(-lvk);
    const T lim = zk - eps;
#pragma unroll 4
    for (int j = sub; j < V; j += G) {
      const T pj = clamp_unit(p[(int64_t)j * a.p_sv]);
      const T nm = -log_(-log_(clamp_unit(x2[j])) / pj - lvk);
      z[j] = j == k ? zk : (lim < nm ? lim : nm);
    }
  } else if (OP == RLX_LOG_PROB) {
    T s = T(0);
#pragma unroll 4
    for (int j = sub; j < V; j += G) {
      const T g = p[(int64_t)j * a.p_sv] - x1[j];
      s += g - exp_(g);
    }
    s = group_sum(s, G);
    if (sub == 0) a.out[r] = s;
  } else {  // RLX_CLOG_PROB: x1 = zcond, x2 = b
    bool one_hot;
    const int k = row_hot<T>(x2, V, G, sub, &one_hot);
    const T zk = one_hot ? x1[k] : T(0);
    T best = -std::numeric_limits<T>::infinity(), s = T(0);
    int idx = kNoIndex;
#pragma unroll 4
    for (int j = sub; j < V; j += G) {
      const T zj = x1[j];
      if (arg_before(zj, j, best, idx)) best = zj, idx = j;
      const T l = j == k ? T(0) : p[(int64_t)j * a.p_sv];
      T g = l - zj;
      g = g - exp_(g);
      s += j == k ? g : g + exp_(l - zk);
    }
    group_argmax(best, idx, G);
    s = group_sum(s, G);
    if (sub == 0) a.out[r] = (one_hot && idx == k) ? s : -std::numeric_limits<T>::infinity();
  }
}

// ---- logistic / Bernoulli: elementwise, the rows only carry the parameter's broadcast -----------
template <typename T, int OP>
__global__ void __launch_bounds__(kRelaxedThreads) bernoulli_kernel(const RelaxedArgs<T> a) {
  const int G = a.G, V = a.V;
  const int sub = (int)threadIdx.x & (G - 1);
  const int64_t r = (int64_t)blockIdx.x * (kRelaxedThreads / G) + ((int)threadIdx.x / G);
  if (r >= a.R) return;
  const T *__restrict__ p = a.param ? a.param + (r % a.B) * a.p_sr : nullptr;
  const T *__restrict__ x1 = a.in1 + r * V;
  const T *__restrict__ x2 = a.in2 ? a.in2 + r * V : nullptr;
  T *__restrict__ out = a.out + r * V;
  const T eps = eps_of<T>();
#pragma unroll 4
  for (int j = sub; j < V; j += G) {
    const T q = p ? p[(int64_t)j * a.p_sv] : T(0);
    const T x = x1[j];
    T y;
    if (OP == RLX_RSAMPLE) {
      const T u = clamp_unit(x);
      y = q + log_(u) - log1p_(-u);
    } else if (OP == RLX_THRESHOLD) {
      y = x >= T(0) ? T(1) : T(0);
    } else if (OP == RLX_TLOG_PROB) {  // b * logits - softplus(logits), the stable form
      y = x * q - ((q > T(0) ? q : T(0)) + log1p_(exp_(-(q < T(0) ? -q : q))));
    } else if (OP == RLX_CSAMPLE) {  // x = b, x2 = v, q = probs
      const T v = clamp_unit(x2[j]), pr = clamp_unit(q);
      const T t = v / ((T(1) - v) * ((T(1) - x) * pr + x * (T(1) - pr))) + T(1);
      y = (T(2) * x - T(1)) * log_(t) + x * eps;
    } else if (OP == RLX_LOG_PROB) {
      const T d = q - x;
      y = d - T(2) * log1p_(exp_(d));
    } else {  // RLX_CLOG_PROB: x = zcond, x2 = b
      const T b = x2[j];
      const T bc = x >= T(0) ? T(1) : T(0);
      y = -x + (T(1) - b) * q + log1p_(exp_(q)) - T(2) * log1p_(exp_(q - x));
      if (bc != b) y = -std::numeric_limits<T>::infinity();
    }
    out[j] = y;
  }
}

template <typename T, int OP, bool GUMBEL> int launch_op(const RelaxedArgs<T> &a, hipStream_t s) {
  const int64_t per_block = kRelaxedThreads / a.G;
  const int64_t blocks = (a.R + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  if (GUMBEL) hipLaunchKernelGGL((gumbel_kernel<T, OP>), dim3((unsigned)blocks), dim3(kRelaxedThreads), 0, s, a);
  else hipLaunchKernelGGL((bernoulli_kernel<T, OP>), dim3((unsigned)blocks), dim3(kRelaxedThreads), 0, s, a);
  return (int)hipGetLastError();
}

template <typename T, bool GUMBEL> int launch_typed(int op, const RelaxedArgs<T> &a, hipStream_t s) {
  switch (op) {
    case RLX_RSAMPLE: return launch_op<T, RLX_RSAMPLE, GUMBEL>(a, s);
    case RLX_THRESHOLD: return launch_op<T, RLX_THRESHOLD, GUMBEL>(a, s);
    case RLX_TLOG_PROB: return launch_op<T, RLX_TLOG_PROB, GUMBEL>(a, s);
    case RLX_CSAMPLE: return launch_op<T, RLX_CSAMPLE, GUMBEL>(a, s);
    case RLX_LOG_PROB: return launch_op<T, RLX_LOG_PROB, GUMBEL>(a, s);
    default: return launch_op<T, RLX_CLOG_PROB, GUMBEL>(a, s);
  }
}

template <bool GUMBEL>
int relaxed(int op, int dtype, const void *param, int64_t B, int64_t p_sr, int64_t p_sv, const void *in1,
            const void *in2, int64_t R, int64_t V, void *out, void *stream) {
  if (op < 0 || op >= RLX_OPS || (dtype != RLX_F32 && dtype != RLX_F64) || R < 0 || V < 0 || B < 0) return PDT_E_ARG;
  if (R == 0 || V == 0) return PDT_OK;
  if (V > 0x7fffffffLL - PDT_WAVE) return PDT_E_TOO_LONG;  // (the lanes' `j += G` stays inside int)
  const bool two = op == RLX_CSAMPLE || op == RLX_CLOG_PROB;
  if (in1 == nullptr || out == nullptr || (two && in2 == nullptr)) return PDT_E_ARG;
  if (op != RLX_THRESHOLD && (param == nullptr || B == 0)) return PDT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RLX_F32) {
    RelaxedArgs<float> a{(const float *)param, (const float *)in1, (const float *)in2, (float *)out,
                         B, p_sr, p_sv, R, (int)V, group_width(V)};
    if (op == RLX_THRESHOLD) a.param = nullptr, a.B = 1;
    return launch_typed<float, GUMBEL>(op, a, s);
  }
  RelaxedArgs<double> a{(const double *)param, (const double *)in1, (const double *)in2, (double *)out,
                        B, p_sr, p_sv, R, (int)V, group_width(V)};
  if (op == RLX_THRESHOLD) a.param = nullptr, a.B = 1;
  return launch_typed<double, GUMBEL>(op, a, s);
}

// ---- backward -----------------------------------------------------------------------------------
// One launch per method: the gradient of the parameter as (B, V) dense, ALREADY summed over the
// S = R / B sample rows that read each parameter row, and the gradient of in1 (z of log_prob, zcond
// of clog_prob) as (R, V) dense.  The arithmetic is that of the host's torch bodies (_gumbel_backward,
// _bernoulli_backward), operation for operation in the data's type: a mask is a product where they
// multiply and a select where they use `where`, so a non-finite value spreads as it does there.
//
// A UNIT is a group of G lanes that owns (part, parameter row, chunk of columns) and walks the part's
// sample rows s, r = s * B + row.  Lane `sub` keeps the sums of columns c0 + sub + t * G, t <
// kBackwardTrips, in float64 registers -- a chunk is G * kBackwardTrips columns, 512 of a wave's --
// and stores them once at the end, so the sum over the samples has one order, needs no atomics and is
// the same on every call.  Rows beyond 512 columns are several units, adjacent in a workgroup; the
// methods with row-wide quantities (Gumbel csample, clog_prob) then repeat the row-wide passes per
// chunk, out of the cache.  With P > 1 the S sample rows are cut into P parts of `per` rows, every
// part stores its float64 sums to a (P, B, V) workspace and parts_sum_kernel adds them in the order
// of the parts.  With S == 1 a unit is a row, as in the forward.
constexpr int kBackwardTrips = 8;
// backward_parts: fill the device.  A unit walks its sample rows one after the other, and a row costs it
// a memory latency or three (the row-wide passes of csample and clog_prob), about a microsecond each
// whatever the row holds, so what the rule buys is waves: 256 CUs of 4 SIMDs, and four waves per SIMD
// (the kernels take 46 to 146 VGPRs: three to eight fit) before the rows of a parameter stop being
// cut.  Below kBackwardMinSamples sample rows nothing is cut: the second launch would cost what it saves.
// A part may be a single row -- its float64 partial costs 16 bytes of traffic per column against the
// row's 8 to 24, but where the rule cuts at all the device is not full and latency binds, not traffic.
constexpr int64_t kBackwardTargetWaves = 4096;
constexpr int64_t kBackwardMinSamples = 8;

template <typename T> struct RelaxedBackwardArgs {
  const T *g;       // (R, V), or (R,) for the Gumbel *log_prob
  const T *param;   // (B, V) through (p_sr, p_sv)
  const T *in1;     // (R, V)
  const T *in2;     // (R, V), the methods of two data arguments
  T *grad_param;    // (B, V), or null
  T *grad_in1;      // (R, V), or null
  double *parts;    // (P, B, V) when P > 1
  int64_t B, p_sr, p_sv, S, per, units;
  int V, G, chunks;
};

int64_t backward_chunks(int64_t V) {
  const int64_t span = (int64_t)PDT_WAVE * kBackwardTrips;
  return group_width(V) < PDT_WAVE ? 1 : (V + span - 1) / span;
}

int backward_parts(int64_t R, int64_t B, int64_t V) {
  if (R < 1 || B < 1 || V < 1 || R % B) return 0;
  const int64_t S = R / B, G = group_width(V);
  const int64_t waves = (B * backward_chunks(V) * G + PDT_WAVE - 1) / PDT_WAVE;
  if (waves >= kBackwardTargetWaves || S < kBackwardMinSamples) return 1;
  int64_t want = (kBackwardTargetWaves + waves - 1) / waves;
  if (want > S) want = S;
  const int64_t per = (S + want - 1) / want;
  return (int)((S + per - 1) / per);  // (no part is empty)
}

template <typename T> __device__ __forceinline__ T sigmoid_(T x) { return T(1) / (T(1) + exp_(-x)); }

// what a unit is, and the rows it walks
template <typename T> struct BackwardUnit {
  int sub, c0;
  int64_t row, part, s0, s1;
  __device__ __forceinline__ bool init(const RelaxedBackwardArgs<T> &a) {
    sub = (int)threadIdx.x & (a.G - 1);
    const int64_t u = (int64_t)blockIdx.x * (kRelaxedThreads / a.G) + ((int)threadIdx.x / a.G);
    if (u >= a.units) return false;  // (a whole group leaves together)
    c0 = (int)(u % a.chunks) * (a.G * kBackwardTrips);
    row = (u / a.chunks) % a.B;
    part = u / (a.chunks * a.B);
    s0 = part * a.per;
    s1 = s0 + a.per < a.S ? s0 + a.per : a.S;
    return true;
  }
  __device__ __forceinline__ void store(const RelaxedBackwardArgs<T> &a, const double (&acc)[kBackwardTrips]) const {
    if (a.grad_param == nullptr) return;
#pragma unroll
    for (int t = 0; t < kBackwardTrips; ++t) {
      const int j = c0 + sub + t * a.G;
      if (j >= a.V) break;
      if (a.parts) a.parts[(part * a.B + row) * a.V + j] = acc[t];
      else a.grad_param[row * a.V + j] = (T)acc[t];
    }
  }
};

template <typename T, int OP>
__global__ void __launch_bounds__(kRelaxedThreads) gumbel_backward_kernel(const RelaxedBackwardArgs<T> a) {
  const int G = a.G, V = a.V;
  BackwardUnit<T> u;
  if (!u.init(a)) return;
  const int sub = u.sub;
  const T *__restrict__ p = a.param + u.row * a.p_sr;
  const T eps = eps_of<T>();
  constexpr bool kReduces = OP == RLX_TLOG_PROB || OP == RLX_LOG_PROB || OP == RLX_CLOG_PROB;
  double acc[kBackwardTrips];
#pragma unroll
  for (int t = 0; t < kBackwardTrips; ++t) acc[t] = 0.0;
  for (int64_t s = u.s0; s < u.s1; ++s) {
    const int64_t r = s * a.B + u.row;
    const T *__restrict__ x1 = a.in1 + r * V;
    const T *__restrict__ x2 = a.in2 ? a.in2 + r * V : nullptr;
    const T *__restrict__ gd = a.g + r * V;  // (the methods that do not reduce)
    T gr = kReduces ? a.g[r] : T(0);
    T *__restrict__ dx = a.grad_in1 ? a.grad_in1 + r * V : nullptr;
    // the row-wide quantities.  The body's sums over b are those of its nonzeros (a term of b_j = 0 is a
    // zero for every finite operand, and is skipped): one term for a one-hot row, none for an empty one.
    T lvk = T(0), zk = T(0), se = T(0);
    if (OP == RLX_CSAMPLE) {
      bool one_hot;
      const int k = row_hot<T>(x1, V, G, sub, &one_hot);
      if (one_hot) {
        lvk = log_(clamp_unit(x2[k]));
        zk = -log_(-lvk);
      } else if (k != kNoIndex) {
        for (int j = sub; j < V; j += G) {
          const T b = x1[j];
          if (b != T(0)) {
            const T lv = log_(clamp_unit(x2[j]));
            lvk += lv * b;
            zk += -log_(-lv) * b;
          }
        }
        lvk = group_sum(lvk, G);
        zk = group_sum(zk, G);
      }
    } else if (OP == RLX_CLOG_PROB) {  // x1 = zcond, x2 = b
      bool one_hot;
      const int k = row_hot<T>(x2, V, G, sub, &one_hot);
      if (one_hot) {
        zk = x1[k];
      } else if (k != kNoIndex) {
        for (int j = sub; j < V; j += G) {
          const T b = x2[j];
          if (b != T(0)) zk += x1[j] * b;
        }
        zk = group_sum(zk, G);
      }
      T best = -std::numeric_limits<T>::infinity();
      int idx = kNoIndex;
#pragma unroll 4
      for (int j = sub; j < V; j += G) {
        const T zj = x1[j];
        if (arg_before(zj, j, best, idx)) best = zj, idx = j;
        const T rest = T(1) - x2[j];
        se += exp_(p[(int64_t)j * a.p_sv] * rest - zk) * rest;
      }
      group_argmax(best, idx, G);
      se = group_sum(se, G);
      if (!(one_hot && idx == k)) gr = T(0);  // (a select: the products below still see the row's values)
    }
#pragma unroll
    for (int t = 0; t < kBackwardTrips; ++t) {
      if ((int64_t)u.c0 + t * G >= V) break;
      const int j = u.c0 + sub + t * G;
      if (j >= V) continue;
      T d;
      if (OP == RLX_RSAMPLE) {
        d = gd[j];
      } else if (OP == RLX_TLOG_PROB) {
        d = gr * (x1[j] != T(0) ? T(1) : T(0));
      } else if (OP == RLX_LOG_PROB) {
        d = gr * (T(1) - exp_(p[(int64_t)j * a.p_sv] - x1[j]));
        if (dx) dx[j] = -d;
      } else if (OP == RLX_CSAMPLE) {
        const T b = x1[j], lv = log_(clamp_unit(x2[j])), raw = p[(int64_t)j * a.p_sv];
        const T pj = clamp_unit(raw);
        const T w = -lv / pj - lvk;
        const bool open = (-log_(w) <= zk - eps) && (raw >= eps) && (raw <= T(1) - eps);
        d = gd[j] * (-lv / (pj * pj * w)) * (T(1) - b) * (open ? T(1) : T(0));
      } else {  // RLX_CLOG_PROB
        const T zj = x1[j], b = x2[j];
        const T rest = T(1) - b;
        const T l = p[(int64_t)j * a.p_sv] * rest;
        const T aj = T(1) - exp_(l - zj);
        const T e = exp_(l - zk) * rest;
        d = gr * rest * (aj + e);
        if (dx) dx[j] = gr * (-aj - b * se);
      }
      acc[t] += (double)d;
    }
  }
  u.store(a, acc);
}

template <typename T, int OP>
__global__ void __launch_bounds__(kRelaxedThreads) bernoulli_backward_kernel(const RelaxedBackwardArgs<T> a) {
  const int G = a.G, V = a.V;
  BackwardUnit<T> u;
  if (!u.init(a)) return;
  const int sub = u.sub;
  const T *__restrict__ p = a.param + u.row * a.p_sr;
  const T eps = eps_of<T>();
  double acc[kBackwardTrips];
#pragma unroll
  for (int t = 0; t < kBackwardTrips; ++t) acc[t] = 0.0;
  for (int64_t s = u.s0; s < u.s1; ++s) {
    const int64_t r = s * a.B + u.row;
    const T *__restrict__ x1 = a.in1 + r * V;
    const T *__restrict__ x2 = a.in2 ? a.in2 + r * V : nullptr;
    const T *__restrict__ gd = a.g + r * V;
    T *__restrict__ dx = a.grad_in1 ? a.grad_in1 + r * V : nullptr;
#pragma unroll
    for (int t = 0; t < kBackwardTrips; ++t) {
      if ((int64_t)u.c0 + t * G >= V) break;
      const int j = u.c0 + sub + t * G;
      if (j >= V) continue;
      const T g = gd[j];
      const T q = OP == RLX_RSAMPLE ? T(0) : p[(int64_t)j * a.p_sv];  // (rsample passes g on: nothing else is read)
      const T x = OP == RLX_RSAMPLE ? T(0) : x1[j];
      T d;
      if (OP == RLX_RSAMPLE) {
        d = g;
      } else if (OP == RLX_TLOG_PROB) {
        d = g * (x - sigmoid_(q));
      } else if (OP == RLX_LOG_PROB) {
        d = g * (T(1) - T(2) * sigmoid_(q - x));
        if (dx) dx[j] = -d;
      } else if (OP == RLX_CSAMPLE) {  // x = b, x2 = v, q = probs
        const T v = clamp_unit(x2[j]), pr = clamp_unit(q);
        const T m = (T(1) - x) * pr + x * (T(1) - pr);
        const T tt = v / ((T(1) - v) * m) + T(1);
        const T sg = T(2) * x - T(1);
        const bool open = (q >= eps) && (q <= T(1) - eps);
        d = g * (sg * sg) * v / ((T(1) - v) * m * m * tt) * (open ? T(1) : T(0));
      } else {  // RLX_CLOG_PROB: x = zcond, x2 = b
        const T b = x2[j];
        const T sg = sigmoid_(q - x);
        const T gs = (x >= T(0) ? T(1) : T(0)) == b ? g : T(0);
        d = gs * ((T(1) - b) + sigmoid_(q) - T(2) * sg);
        if (dx) dx[j] = gs * (T(2) * sg - T(1));
      }
      acc[t] += (double)d;
    }
  }
  u.store(a, acc);
}

// the parts of (P, B, V), added in their order
template <typename T>
__global__ void __launch_bounds__(kRelaxedThreads) parts_sum_kernel(const double *__restrict__ parts, T *__restrict__ out,
                                                                    int64_t n, int P) {
  const int64_t i = (int64_t)blockIdx.x * kRelaxedThreads + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
#pragma unroll 8
  for (int q = 0; q < P; ++q) s += parts[q * n + i];
  out[i] = (T)s;
}

template <typename T, int OP, bool GUMBEL> int launch_backward_op(const RelaxedBackwardArgs<T> &a, hipStream_t s) {
  const int64_t per_block = kRelaxedThreads / a.G;
  const int64_t blocks = (a.units + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  if (GUMBEL) hipLaunchKernelGGL((gumbel_backward_kernel<T, OP>), dim3((unsigned)blocks), dim3(kRelaxedThreads), 0, s, a);
  else hipLaunchKernelGGL((bernoulli_backward_kernel<T, OP>), dim3((unsigned)blocks), dim3(kRelaxedThreads), 0, s, a);
  return (int)hipGetLastError();
}

template <typename T, bool GUMBEL>
int backward_typed(int op, const void *g, const void *param, int64_t B, int64_t p_sr, int64_t p_sv, const void *in1,
                   const void *in2, int64_t R, int64_t V, void *grad_param, void *grad_in1, void *ws, int P,
                   hipStream_t s) {
  RelaxedBackwardArgs<T> a{(const T *)g, (const T *)param, (const T *)in1, (const T *)in2, (T *)grad_param,
                           (T *)grad_in1, nullptr, B, p_sr, p_sv, R / B, 0, 0, (int)V, group_width(V), 0};
  a.chunks = (int)backward_chunks(V);
  a.per = (a.S + P - 1) / P;
  a.units = (int64_t)P * B * a.chunks;
  if (P > 1 && grad_param) a.parts = (double *)ws;
  const int64_t n = B * V;
  const int64_t sum_blocks = (n + kRelaxedThreads - 1) / kRelaxedThreads;
  if (a.parts && sum_blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  int rc;
  switch (op) {
    case RLX_RSAMPLE: rc = launch_backward_op<T, RLX_RSAMPLE, GUMBEL>(a, s); break;
    case RLX_TLOG_PROB: rc = launch_backward_op<T, RLX_TLOG_PROB, GUMBEL>(a, s); break;
    case RLX_CSAMPLE: rc = launch_backward_op<T, RLX_CSAMPLE, GUMBEL>(a, s); break;
    case RLX_LOG_PROB: rc = launch_backward_op<T, RLX_LOG_PROB, GUMBEL>(a, s); break;
    default: rc = launch_backward_op<T, RLX_CLOG_PROB, GUMBEL>(a, s); break;
  }
  if (rc != PDT_OK || a.parts == nullptr) return rc;
  hipLaunchKernelGGL((parts_sum_kernel<T>), dim3((unsigned)sum_blocks), dim3(kRelaxedThreads), 0, s, a.parts,
                     (T *)grad_param, n, P);
  return (int)hipGetLastError();
}

template <bool GUMBEL>
int relaxed_backward(int op, int dtype, const void *g, const void *param, int64_t B, int64_t p_sr, int64_t p_sv,
                     const void *in1, const void *in2, int64_t R, int64_t V, void *grad_param, void *grad_in1,
                     void *ws, void *stream) {
  if (op < 0 || op >= RLX_OPS || op == RLX_THRESHOLD || (dtype != RLX_F32 && dtype != RLX_F64)) return PDT_E_ARG;
  if (R < 0 || V < 0 || B < 1 || R % B) return PDT_E_ARG;
  const bool two = op == RLX_CSAMPLE || op == RLX_CLOG_PROB;
  const bool has_in1_grad = op == RLX_LOG_PROB || op == RLX_CLOG_PROB;
  if (grad_param == nullptr && grad_in1 == nullptr) return PDT_E_ARG;
  if (grad_in1 != nullptr && !has_in1_grad) return PDT_E_ARG;
  if (R == 0 || V == 0) return PDT_OK;
  if (g == nullptr || in1 == nullptr || param == nullptr || (two && in2 == nullptr)) return PDT_E_ARG;
  // (the lanes' `c0 + sub + t * G` stays inside int)
  if (V > 0x7fffffffLL - PDT_WAVE * kBackwardTrips) return PDT_E_TOO_LONG;
  const int P = backward_parts(R, B, V);
  if (P > 1 && ws == nullptr) return PDT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RLX_F32)
    return backward_typed<float, GUMBEL>(op, g, param, B, p_sr, p_sv, in1, in2, R, V, grad_param, grad_in1, ws, P, s);
  return backward_typed<double, GUMBEL>(op, g, param, B, p_sr, p_sv, in1, in2, R, V, grad_param, grad_in1, ws, P, s);
}

}  // namespace
}  // namespace pdt

extern "C" int pdt_relaxed_backward_parts(int64_t R, int64_t B, int64_t V) { return pdt::backward_parts(R, B, V); }

extern "C" int64_t pdt_relaxed_backward_workspace_bytes(int dtype, int64_t R, int64_t B, int64_t V) {
  if (dtype != pdt::RLX_F32 && dtype != pdt::RLX_F64) return PDT_E_ARG;
  const int P = pdt::backward_parts(R, B, V);
  return P > 1 ? (int64_t)P * B * V * (int64_t)sizeof(double) : 0;
}

extern "C" int pdt_relaxed_gumbel_backward(int op, int dtype, const void *g, const void *param, int64_t B,
                                           int64_t p_sr, int64_t p_sv, const void *in1, const void *in2, int64_t R,
                                           int64_t V, void *grad_param, void *grad_in1, void *ws, void *stream) {
  return pdt::relaxed_backward<true>(op, dtype, g, param, B, p_sr, p_sv, in1, in2, R, V, grad_param, grad_in1, ws,
                                     stream);
}

extern "C" int pdt_relaxed_bernoulli_backward(int op, int dtype, const void *g, const void *param, int64_t B,
                                              int64_t p_sr, int64_t p_sv, const void *in1, const void *in2, int64_t R,
                                              int64_t V, void *grad_param, void *grad_in1, void *ws, void *stream) {
  return pdt::relaxed_backward<false>(op, dtype, g, param, B, p_sr, p_sv, in1, in2, R, V, grad_param, grad_in1, ws,
                                      stream);
}

extern "C" int pdt_relaxed_group_width(int64_t V) { return V < 1 ? 0 : pdt::group_width(V); }

extern "C" int pdt_relaxed_rows_per_block(int64_t V) {
  return V < 1 ? 0 : pdt::kRelaxedThreads / pdt::group_width(V);
}

extern "C" int pdt_relaxed_gumbel(int op, int dtype, const void *param, int64_t B, int64_t p_sr, int64_t p_sv,
                                  const void *in1, const void *in2, int64_t R, int64_t V, void *out, void *stream) {
  return pdt::relaxed<true>(op, dtype, param, B, p_sr, p_sv, in1, in2, R, V, out, stream);
}

extern "C" int pdt_relaxed_bernoulli(int op, int dtype, const void *param, int64_t B, int64_t p_sr, int64_t p_sv,
                                     const void *in1, const void *in2, int64_t R, int64_t V, void *out,
                                     void *stream) {
  return pdt::relaxed<false>(op, dtype, param, B, p_sr, p_sv, in1, in2, R, V, out, stream);
}
