// Reductions over the sample axis of the Monte Carlo estimators (reference _mc.py:145-173, 230-233,
// 297-301, 390-404, 530-564; _enumerate_estimator.py:68-77).  The reference chains a clamp, exp, max,
// mean, log or softmax per line and autograd walks the chain back; here the whole formula of a column
// is ONE launch, and its backward ONE elementwise launch from the column statistics the forward left.
//
// Data are (M, B): M samples of B batch columns, every input read through its own element strides
// (s_m, s_b).  Stride 0 is allowed (cv_mean is (B,) broadcast over M).  Two forms, chosen by the
// shape and the strides of f (plan_for):
//   columns  lane = column: loads coalesce across the wave when b is the dense axis, every lane walks
//            its own column, the loop unrolled by eight so that the loads run ahead of the sums;
//   wave     one wave per column, lane l takes samples l, l + 64, ...: for columns of 64 samples and more
//            when there are fewer than kWideColumns of them (lane = column would launch B / 64 waves, under
//            one per compute unit, each walking M / 8 groups of loads one after the other: DirectEstimator's
//            call and backward took 0.57 ms that way at M = 1024, B = 4096, 0.39 ms this way; EXPERIMENTS.md
//            section 16), or when m is the dense axis; the lanes meet in xor butterflies.
// The column maximum (with the index `max` selects: the lowest of equals, a NaN first) comes first,
// then the sums: up to four passes over M (self-normalised, in log space).  Elements are computed in
// the data's type in the reference's order (subtract, clamp, exp; -ffp-contract=off); the sums over M
// accumulate in float64 with compensation (Sum) for both types, so that the order of summation does not show at
// any M.
//
// stats is (5, B) float64, the rows by operation:
//   MEAN      log: 0 = logsumexp_m f
//   SCORE     log: 0 = clamped maximum, 1 = its index, 2 = floored mean, 3 = [mean >= floor],
//                  4 = the factor of g that reaches f at the index through the maximum
//   WEIGHTED  0 = max_m (lp - lq), 1 = log sum_m exp(lp - lq - max) (self-normalised), 2 = the result
#include "pdt_common.hpp"

#include <cmath>
#include <limits>

namespace pdt {
namespace {

enum { MC_F32 = 0, MC_F64 = 1 };
enum { MC_MEAN = 0, MC_SCORE = 1, MC_WEIGHTED = 2, MC_KINDS };
enum { MC_W_LOGM = 0, MC_W_SELF = 1, MC_W_NONE = 2, MC_W_MODES };  // kappa of WEIGHTED
enum { MC_IN_F = 0, MC_IN_A, MC_IN_CZ, MC_IN_C, MC_IN_LP, MC_IN_LQ, MC_INPUTS };
enum { MC_FORM_COLUMNS = 0, MC_FORM_WAVE = 1 };

constexpr int kMcThreads = 256;
constexpr int64_t kWideColumns = 16384;  // 256 waves of 64 columns: one per compute unit
// config.EPS_NINF, config.EPS_INF: log(smallest normal float32) / 2, log(largest float32) / 2, by the host's
// log as config.py takes them
inline double eps_ninf() { return std::log(1.1754943508222875e-38) / 2; }
inline double eps_inf() { return std::log(3.4028234663852886e38) / 2; }

template <typename T> struct McArgs {
  const T *in[MC_INPUTS];
  int64_t sm[MC_INPUTS], sb[MC_INPUTS];
  const T *g;     // backward: (B,)
  T *out;         // forward: (B,)
  T *grad[MC_INPUTS];  // backward: (M, B) dense, grad[MC_IN_C] (B,); null where not wanted
  double *stats;  // (5, B)
  int64_t M, B;
  int mode;
  T eps_ninf, eps_inf, floor_, log_m;
};

__device__ __forceinline__ float mc_log(float x) { return logf(x); }
__device__ __forceinline__ double mc_log(double x) { return log(x); }
__device__ __forceinline__ float mc_exp(float x) { return expf(x); }
__device__ __forceinline__ double mc_exp(double x) { return exp(x); }

// does (a, ia) precede (b, ib) as the arg-max?  A NaN is the maximum, equals go to the lower index.
template <typename T> __device__ __forceinline__ bool mc_before(T a, int64_t ia, T b, int64_t ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}

// A sum over the sample axis: float64 with the rounding error of every addition kept beside it (Neumaier), so
// that neither the length of a column nor the order its lanes meet in shows in float32 or in float64 results.
struct Sum {
  double s = 0.0, c = 0.0;
  __device__ __forceinline__ void operator+=(double x) {
    const double t = s + x;
    c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;  // (a non-finite term leaves NaN here: total() below)
    s = t;
  }
  __device__ __forceinline__ double total() const {
    const double t = s + c;
    return t == t ? t : s;  // +-inf or NaN terms: the plain sum has the reference's class
  }
};
template <bool WAVE> __device__ __forceinline__ double col_sum(Sum v) {
  if (WAVE)
    for (int o = PDT_WAVE >> 1; o; o >>= 1) {
      const double c = __shfl_xor(v.c, o, PDT_WAVE);
      v += __shfl_xor(v.s, o, PDT_WAVE);
      v.c += c;
    }
  return v.total();
}
template <bool WAVE, typename T> __device__ __forceinline__ void col_argmax(T &val, int64_t &idx) {
  if (WAVE)
    for (int o = PDT_WAVE >> 1; o; o >>= 1) {
      const T v = __shfl_xor(val, o, PDT_WAVE);
      const int lo = __shfl_xor((int)(idx & 0xffffffffLL), o, PDT_WAVE);
      const int hi = __shfl_xor((int)(idx >> 32), o, PDT_WAVE);
      const int64_t i = ((int64_t)hi << 32) | (unsigned)lo;
      if (mc_before(v, i, val, idx)) val = v, idx = i;
    }
}

// the samples of one column that this lane visits: all of them, or every 64th from its own
#define MC_FOR(m) _Pragma("unroll 8") for (int64_t m = m0; m < M; m += step)

template <typename T> struct Clamped {
  T e;      // exp(clamp(x, EPS_NINF, EPS_INF))
  T inner;  // 1 where the clamp passes the gradient (its bounds included), else 0
};
template <typename T> __device__ __forceinline__ Clamped<T> clamp_exp(T x, T lo, T hi) {
  const T xc = x < lo ? lo : (x > hi ? hi : x);  // (a NaN stays a NaN)
  Clamped<T> r;
  r.e = mc_exp(xc);
  r.inner = (x >= lo && x <= hi) ? T(1) : T(0);
  return r;
}

// the maximum of column x over the lane's samples, then over the wave
template <bool WAVE, typename T, typename F>
__device__ __forceinline__ T col_max(int64_t M, int64_t m0, int64_t step, int64_t *at, F x) {
  T best = -std::numeric_limits<T>::infinity();
  int64_t idx = std::numeric_limits<int64_t>::max();
  MC_FOR(m) {
    const T v = x(m);
    if (mc_before(v, m, best, idx)) best = v, idx = m;
  }
  col_argmax<WAVE>(best, idx);
  if (at) *at = idx;
  return best;
}

template <typename T, int KIND, bool LOG, bool WAVE>
__global__ void __launch_bounds__(kMcThreads) mc_reduce_kernel(const McArgs<T> a) {
  const int64_t M = a.M, B = a.B;
  int64_t b, m0, step;
  if (WAVE) {
    b = (int64_t)blockIdx.x * (kMcThreads / PDT_WAVE) + ((int)threadIdx.x >> 6);
    m0 = lane_id(), step = PDT_WAVE;
  } else {
    b = (int64_t)blockIdx.x * kMcThreads + (int)threadIdx.x;
    m0 = 0, step = 1;
  }
  if (b >= B) return;  // (a whole wave of the wave form leaves together)
  const bool writer = !WAVE || m0 == 0;
  const T *__restrict__ f = a.in[MC_IN_F] + b * a.sb[MC_IN_F];
  const int64_t f_sm = a.sm[MC_IN_F];
  double *__restrict__ st = a.stats + b;
  const T inf = std::numeric_limits<T>::infinity();

  if (KIND == MC_MEAN) {
    if (!LOG) {
      Sum s;
      MC_FOR(m) s += (double)f[m * f_sm];
      const double total = col_sum<WAVE>(s);
      if (writer) a.out[b] = (T)(total / (double)M);
    } else {
      T mx = col_max<WAVE, T>(M, m0, step, nullptr, [&](int64_t m) { return f[m * f_sm]; });
      if (mx == inf || mx == -inf) mx = T(0);  // (logsumexp's own guard)
      Sum s;
      MC_FOR(m) s += (double)mc_exp(f[m * f_sm] - mx);
      const T lse = mc_log((T)col_sum<WAVE>(s)) + mx;
      if (writer) a.out[b] = lse - a.log_m, st[0] = (double)lse;
    }
  } else if (KIND == MC_SCORE) {
    const T *__restrict__ pa = a.in[MC_IN_A] ? a.in[MC_IN_A] + b * a.sb[MC_IN_A] : nullptr;
    const T *__restrict__ pz = a.in[MC_IN_CZ] ? a.in[MC_IN_CZ] + b * a.sb[MC_IN_CZ] : nullptr;
    const T *__restrict__ pc = a.in[MC_IN_C] ? a.in[MC_IN_C] + b * a.sb[MC_IN_C] : nullptr;
    const int64_t a_sm = a.sm[MC_IN_A], z_sm = a.sm[MC_IN_CZ];
    if (!LOG) {
      const T c = pc ? pc[0] : T(0);
      Sum s;
      MC_FOR(m) {
        T w = f[m * f_sm];
        if (pa) w = w - pa[m * a_sm];
        if (pc) w = w + c;
        if (pz) w = w + pz[m * z_sm];
        s += (double)w;
      }
      const double total = col_sum<WAVE>(s);
      if (writer) a.out[b] = (T)(total / (double)M);
    } else {
      const T lo = std::numeric_limits<T>::lowest() / T(2), hi = std::numeric_limits<T>::max() / T(2);
      int64_t arg;
      const T raw = col_max<WAVE, T>(M, m0, step, &arg, [&](int64_t m) { return f[m * f_sm]; });
      const T mx = raw < lo ? lo : (raw > hi ? hi : raw);
      Clamped<T> C{T(0), T(0)};
      if (pc) C = clamp_exp<T>(pc[0] - mx, a.eps_ninf, a.eps_inf);
      Sum s, ds;  // the sum of the elements, and of their derivatives in -mx
      MC_FOR(m) {
        const Clamped<T> F = clamp_exp<T>(f[m * f_sm] - mx, a.eps_ninf, a.eps_inf);
        T w = F.e, d = F.e * F.inner;
        if (pa) {
          const Clamped<T> A = clamp_exp<T>(pa[m * a_sm] - mx, a.eps_ninf, a.eps_inf);
          w = w - A.e, d = d - A.e * A.inner;
        }
        if (pc) w = w + C.e, d = d + C.e * C.inner;
        if (pz) {
          const Clamped<T> Z = clamp_exp<T>(pz[m * z_sm] - mx, a.eps_ninf, a.eps_inf);
          w = w + Z.e, d = d + Z.e * Z.inner;
        }
        s += (double)w, ds += (double)d;
      }
      const double total = col_sum<WAVE>(s), dtotal = col_sum<WAVE>(ds);
      const T mu = (T)(total / (double)M);
      const T muc = mu < a.floor_ ? a.floor_ : mu;
      const double pass = mu >= a.floor_ ? 1.0 : 0.0;
      if (writer) {
        a.out[b] = mc_log(muc) + mx;
        st[0] = (double)mx, st[B] = (double)arg, st[2 * B] = (double)muc, st[3 * B] = pass;
        st[4 * B] = (raw >= lo && raw <= hi) ? 1.0 - pass * dtotal / ((double)muc * (double)M) : 0.0;
      }
    }
  } else {  // MC_WEIGHTED
    const T *__restrict__ lp = a.in[MC_IN_LP] + b * a.sb[MC_IN_LP];
    const T *__restrict__ lq = a.in[MC_IN_LQ] ? a.in[MC_IN_LQ] + b * a.sb[MC_IN_LQ] : nullptr;
    const int64_t p_sm = a.sm[MC_IN_LP], q_sm = a.sm[MC_IN_LQ];
    const int mode = a.mode;
    T dmax = T(0), lnorm = T(0);
    if (mode == MC_W_SELF) {  // log_softmax over m of lp - lq
      dmax = col_max<WAVE, T>(M, m0, step, nullptr, [&](int64_t m) { return lp[m * p_sm] - lq[m * q_sm]; });
      Sum s;
      MC_FOR(m) s += (double)mc_exp((lp[m * p_sm] - lq[m * q_sm]) - dmax);
      lnorm = mc_log((T)col_sum<WAVE>(s));
    }
    auto ell = [&](int64_t m) -> T {
      if (mode == MC_W_NONE) return lp[m * p_sm];
      const T d = lp[m * p_sm] - lq[m * q_sm];
      return mode == MC_W_SELF ? (d - dmax) - lnorm : d - a.log_m;
    };
    T v;
    if (!LOG) {
      Sum s;
      MC_FOR(m) s += (double)(f[m * f_sm] * mc_exp(ell(m)));
      v = (T)col_sum<WAVE>(s);
    } else {
      T mx = col_max<WAVE, T>(M, m0, step, nullptr, [&](int64_t m) { return f[m * f_sm] + ell(m); });
      if (mx == inf || mx == -inf) mx = T(0);
      Sum s;
      MC_FOR(m) s += (double)mc_exp((f[m * f_sm] + ell(m)) - mx);
      v = mc_log((T)col_sum<WAVE>(s)) + mx;
    }
    if (writer) a.out[b] = v, st[0] = (double)dmax, st[B] = (double)lnorm, st[2 * B] = (double)v;
  }
}

// one thread per element of (M, B), b the fast index: the gradient of every input from the statistics
template <typename T, int KIND, bool LOG>
__global__ void __launch_bounds__(kMcThreads) mc_reduce_backward_kernel(const McArgs<T> a) {
  const int64_t i = (int64_t)blockIdx.x * kMcThreads + (int)threadIdx.x;
  const int64_t M = a.M, B = a.B;
  if (i >= M * B) return;
  const int64_t m = i / B, b = i % B;
  const double *__restrict__ st = a.stats + b;
  const T g = a.g[b];
  const T f = a.in[MC_IN_F][m * a.sm[MC_IN_F] + b * a.sb[MC_IN_F]];
  T *__restrict__ gf = a.grad[MC_IN_F];
  if (KIND == MC_MEAN) {
    if (gf) gf[i] = LOG ? g * mc_exp(f - (T)st[0]) : g / (T)M;
  } else if (KIND == MC_SCORE) {
    const T *pa = a.in[MC_IN_A], *pz = a.in[MC_IN_CZ], *pc = a.in[MC_IN_C];
    T *__restrict__ ga = a.grad[MC_IN_A], *__restrict__ gz = a.grad[MC_IN_CZ], *__restrict__ gc = a.grad[MC_IN_C];
    T *__restrict__ glp = a.grad[MC_IN_LP];
    const T av = pa ? pa[m * a.sm[MC_IN_A] + b * a.sb[MC_IN_A]] : T(0);
    const T zv = pz ? pz[m * a.sm[MC_IN_CZ] + b * a.sb[MC_IN_CZ]] : T(0);
    const T cv = pc ? pc[b * a.sb[MC_IN_C]] : T(0);
    if (!LOG) {
      const T r = g / (T)M;
      T w = f;
      if (pa) w = w - av;
      if (pc) w = w + cv;
      if (glp) glp[i] = r * w;
      if (gf) gf[i] = r;
      if (ga) ga[i] = -r;
      if (gz) gz[i] = r;
      if (gc && m == 0) gc[b] = g;
    } else {
      const T mx = (T)st[0], muc = (T)st[2 * B];
      const T r = g / (muc * (T)M), k = (T)st[3 * B] * r;
      const Clamped<T> F = clamp_exp<T>(f - mx, a.eps_ninf, a.eps_inf);
      T w = F.e;
      if (pa) {
        const Clamped<T> A = clamp_exp<T>(av - mx, a.eps_ninf, a.eps_inf);
        w = w - A.e;
        if (ga) ga[i] = -(k * A.e * A.inner);
      }
      if (pc) {
        const Clamped<T> C = clamp_exp<T>(cv - mx, a.eps_ninf, a.eps_inf);
        w = w + C.e;
        if (gc && m == 0) gc[b] = k * (T)M * C.e * C.inner;
      }
      if (pz && gz) {
        const Clamped<T> Z = clamp_exp<T>(zv - mx, a.eps_ninf, a.eps_inf);
        gz[i] = k * Z.e * Z.inner;
      }
      if (glp) glp[i] = r * w;
      if (gf) {
        T d = k * F.e * F.inner;
        if ((double)m == st[B]) d = d + g * (T)st[4 * B];
        gf[i] = d;
      }
    }
  } else {  // MC_WEIGHTED
    const T *plq = a.in[MC_IN_LQ];
    T *__restrict__ glp = a.grad[MC_IN_LP], *__restrict__ glq = a.grad[MC_IN_LQ];
    const T lp = a.in[MC_IN_LP][m * a.sm[MC_IN_LP] + b * a.sb[MC_IN_LP]];
    const int mode = a.mode;
    T l = lp;
    if (mode != MC_W_NONE) {
      const T d = lp - plq[m * a.sm[MC_IN_LQ] + b * a.sb[MC_IN_LQ]];
      l = mode == MC_W_SELF ? (d - (T)st[0]) - (T)st[B] : d - a.log_m;
    }
    const T v = (T)st[2 * B];
    const T e = mc_exp(l);
    T d_f, d_l;
    if (!LOG) {
      d_f = g * e, d_l = (g * f) * e;
      if (mode == MC_W_SELF) d_l = d_l - e * (g * v);  // log_softmax: minus exp(l) times the column's sum
    } else {
      d_f = d_l = g * mc_exp((f + l) - v);
      if (mode == MC_W_SELF) d_l = d_l - e * g;
    }
    if (gf) gf[i] = d_f;
    if (glp) glp[i] = d_l;
    if (glq) glq[i] = T(0);
  }
}

// which form serves (M, B) with f read through (s_m, s_b)
int plan_for(int64_t M, int64_t B, int64_t s_m, int64_t s_b) {
  if (M < PDT_WAVE) return MC_FORM_COLUMNS;  // (a wave would idle most of its lanes)
  return (B < kWideColumns || llabs(s_m) < llabs(s_b)) ? MC_FORM_WAVE : MC_FORM_COLUMNS;
}

template <typename T, int KIND, bool LOG> int launch_forward(const McArgs<T> &a, hipStream_t s) {
  const bool wave = plan_for(a.M, a.B, a.sm[MC_IN_F], a.sb[MC_IN_F]) == MC_FORM_WAVE;
  const int64_t per_block = wave ? kMcThreads / PDT_WAVE : kMcThreads;
  const int64_t blocks = (a.B + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  if (wave) hipLaunchKernelGGL((mc_reduce_kernel<T, KIND, LOG, true>), dim3((unsigned)blocks), dim3(kMcThreads), 0, s, a);
  else hipLaunchKernelGGL((mc_reduce_kernel<T, KIND, LOG, false>), dim3((unsigned)blocks), dim3(kMcThreads), 0, s, a);
  return (int)hipGetLastError();
}

template <typename T, int KIND, bool LOG> int launch_backward(const McArgs<T> &a, hipStream_t s) {
  const int64_t blocks = (a.M * a.B + kMcThreads - 1) / kMcThreads;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  hipLaunchKernelGGL((mc_reduce_backward_kernel<T, KIND, LOG>), dim3((unsigned)blocks), dim3(kMcThreads), 0, s, a);
  return (int)hipGetLastError();
}

template <typename T, bool BACKWARD> int dispatch(int kind, int is_log, const McArgs<T> &a, hipStream_t s) {
#define MC_CASE(K)                                                                                  \
  case K:                                                                                           \
    if (BACKWARD) return is_log ? launch_backward<T, K, true>(a, s) : launch_backward<T, K, false>(a, s); \
    return is_log ? launch_forward<T, K, true>(a, s) : launch_forward<T, K, false>(a, s);
  switch (kind) {
    MC_CASE(MC_MEAN)
    MC_CASE(MC_SCORE)
    default:
    MC_CASE(MC_WEIGHTED)
  }
#undef MC_CASE
}

template <typename T, bool BACKWARD>
int run(int kind, int is_log, int mode, int64_t M, int64_t B, const void *const *in, const int64_t *strides,
        const void *g, void *out, double *stats, void *const *grads, hipStream_t s) {
  McArgs<T> a;
  for (int i = 0; i < MC_INPUTS; ++i) {
    a.in[i] = (const T *)in[i];
    a.sm[i] = strides[2 * i], a.sb[i] = strides[2 * i + 1];
    a.grad[i] = BACKWARD ? (T *)grads[i] : nullptr;
  }
  a.g = (const T *)g, a.out = (T *)out, a.stats = stats;
  a.M = M, a.B = B, a.mode = mode;
  a.eps_ninf = (T)eps_ninf(), a.eps_inf = (T)eps_inf();
  a.floor_ = (T)std::exp(eps_ninf()), a.log_m = (T)std::log((double)M);
  return dispatch<T, BACKWARD>(kind, is_log, a, s);
}

// what both entry points ask of their arguments; 1 = nothing to do
int check(int kind, int is_log, int mode, int dtype, int64_t M, int64_t B, const void *const *in,
          const int64_t *strides, const void *stats) {
  if (kind < 0 || kind >= MC_KINDS || (is_log != 0 && is_log != 1) || (dtype != MC_F32 && dtype != MC_F64)) return PDT_E_ARG;
  if (M < 1 || B < 0 || in == nullptr || strides == nullptr) return PDT_E_ARG;
  if (kind == MC_WEIGHTED && (mode < 0 || mode >= MC_W_MODES)) return PDT_E_ARG;
  if (B == 0) return 1;
  if (M > 0x7fffffffffffffffLL / B) return PDT_E_TOO_LONG;
  if (in[MC_IN_F] == nullptr || stats == nullptr) return PDT_E_ARG;
  const bool a = in[MC_IN_A], cz = in[MC_IN_CZ], c = in[MC_IN_C], lp = in[MC_IN_LP], lq = in[MC_IN_LQ];
  if (kind == MC_MEAN && (a || cz || c || lp || lq)) return PDT_E_ARG;
  if (kind == MC_SCORE && (lq || !lp || (c && !a) || (c && cz) || (cz && !a))) return PDT_E_ARG;
  if (kind == MC_WEIGHTED && (a || cz || c || !lp || lq == (mode == MC_W_NONE))) return PDT_E_ARG;
  return PDT_OK;
}

}  // namespace
}  // namespace pdt

extern "C" int pdt_mc_reduce_plan(int64_t M, int64_t B, int64_t s_m, int64_t s_b) {
  return (M < 1 || B < 1) ? -1 : pdt::plan_for(M, B, s_m, s_b);
}

extern "C" int pdt_mc_reduce(int kind, int is_log, int mode, int dtype, int64_t M, int64_t B, const void *const *in,
                             const int64_t *strides, void *out, double *stats, void *stream) {
  const int rc = pdt::check(kind, is_log, mode, dtype, M, B, in, strides, stats);
  if (rc != PDT_OK) return rc < 0 ? rc : PDT_OK;
  if (out == nullptr) return PDT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == pdt::MC_F32) return pdt::run<float, false>(kind, is_log, mode, M, B, in, strides, nullptr, out, stats, nullptr, s);
  return pdt::run<double, false>(kind, is_log, mode, M, B, in, strides, nullptr, out, stats, nullptr, s);
}

extern "C" int pdt_mc_reduce_backward(int kind, int is_log, int mode, int dtype, int64_t M, int64_t B,
                                      const void *const *in, const int64_t *strides, const void *g,
                                      const double *stats, void *const *grads, void *stream) {
  const int rc = pdt::check(kind, is_log, mode, dtype, M, B, in, strides, stats);
  if (rc != PDT_OK) return rc < 0 ? rc : PDT_OK;
  if (g == nullptr || grads == nullptr) return PDT_E_ARG;
  for (int i = 0; i < pdt::MC_INPUTS; ++i)
    if (grads[i] != nullptr && in[i] == nullptr) return PDT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == pdt::MC_F32)
    return pdt::run<float, true>(kind, is_log, mode, M, B, in, strides, g, nullptr, (double *)stats, grads, s);
  return pdt::run<double, true>(kind, is_log, mode, M, B, in, strides, g, nullptr, (double *)stats, grads, s);
}
