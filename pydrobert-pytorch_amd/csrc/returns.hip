// Discounted returns (reference _rl.py:24-41): R[t] = r[t] + gamma * R[t + 1], or with `reverse`
// R[t] = r[t] + gamma * R[t - 1], the adjoint.  A scan: O(T) work, no (T, T) matrix of power
// ratios, no power of gamma beyond one chunk, no division.  Below, "step s" counts in the order the
// recurrence runs (s = 0 is the last frame unless `reverse`), so both directions are one code path.
//
// r and R are indexed (t, n) through element strides.  Two kernels, chosen by R's layout:
//   columns  n is the dense axis (time-major): lane = column, loads and stores coalesce across the
//            wave, every lane runs its own recurrence over a chunk of kColChunk steps;
//   rows     t is the dense axis (batch-major), or N == 1: lane = step, a wave takes 64 steps of one
//            row per pass, scans them with the shifts of a Kogge-Stone ladder (lane l adds
//            gamma^d times lane l - d, d = 1 .. 32) and carries gamma^(l + 1) times the running
//            return into them; a wave walks kRowSegment steps.
// The chunks of time run in parallel when the columns (rows) alone leave the machine idle: pass 1
// leaves the return-at-its-end from a zero start of each chunk but the last, a one-thread-per-column
// pass turns those into each chunk's incoming return (in = partial + gamma^L * in of the chunk
// before), pass 2 reruns the chunks from there and stores.  The largest power formed is gamma^L, L the chunk length; when
// that is not finite in the compute type (|gamma| far above 1), and for the rows kernel gamma^64,
// the columns kernel runs unsplit instead -- the plain recurrence, finite wherever the result is.
// Accumulation in float32, float64 for float64 data.
#include "pdt_common.hpp"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdlib>

namespace pdt {
namespace {

enum { RET_F32 = 0, RET_F64 = 1, RET_F16 = 2, RET_BF16 = 3 };

constexpr int kRetThreads = 256;
constexpr int kColChunk = 32;      // steps of one lane of the columns kernel when time is split
constexpr int kRowSegment = 1024;  // steps of one wave of the rows kernel when time is split
constexpr int64_t kFillWaves = 2048;  // time is split below this many waves (256 CUs x 4 SIMDs x 2)

template <typename T> struct Ret;
template <> struct Ret<float> {
  using C = float;
  __device__ static float in(float v) { return v; }
  __device__ static float out(float v) { return v; }
};
template <> struct Ret<double> {
  using C = double;
  __device__ static double in(double v) { return v; }
  __device__ static double out(double v) { return v; }
};
template <> struct Ret<__half> {
  using C = float;
  __device__ static float in(__half v) { return __half2float(v); }
  __device__ static __half out(float v) { return __float2half(v); }
};
template <> struct Ret<__hip_bfloat16> {
  using C = float;
  __device__ static float in(__hip_bfloat16 v) { return __bfloat162float(v); }
  __device__ static __hip_bfloat16 out(float v) { return __float2bfloat16(v); }
};

template <typename C> struct ReturnArgs {
  const void *r;
  void *R;
  C *carry;  // (chunks, N): pass 1 writes each chunk's partial, pass 2 reads its incoming return
  int64_t T, N, r_st, r_sn, R_st, R_sn;
  int64_t chunk, chunks;  // steps per chunk, number of chunks
  C gamma;
  int reverse;
};

// frame of step s
template <typename C> __device__ __forceinline__ int64_t frame(const ReturnArgs<C> &a, int64_t s) {
  return a.reverse ? s : a.T - 1 - s;
}

// STORE == 0: pass 1 (partials only);  STORE == 1: the returns, from carry[chunk] when there is one
template <typename T, int STORE>
__global__ void __launch_bounds__(kRetThreads) return_columns_kernel(const ReturnArgs<typename Ret<T>::C> a) {
  using C = typename Ret<T>::C;
  const int64_t nb = (a.N + kRetThreads - 1) / kRetThreads;
  const int64_t c = blockIdx.x / nb;
  const int64_t n = (blockIdx.x % nb) * kRetThreads + threadIdx.x;
  if (n >= a.N) return;
  const T *__restrict__ r = (const T *)a.r + n * a.r_sn;
  T *__restrict__ R = (T *)a.R + n * a.R_sn;
  const int64_t s0 = c * a.chunk;
  const int64_t s1 = s0 + a.chunk < a.T ? s0 + a.chunk : a.T;
  C acc = (STORE && a.carry != nullptr) ? a.carry[c * a.N + n] : C(0);
  int64_t s = s0;
  for (; s + 8 <= s1; s += 8) {  // eight loads in flight ahead of the dependent chain
    C v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = Ret<T>::in(r[frame(a, s + i) * a.r_st]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc = v[i] + a.gamma * acc;
      if (STORE) R[frame(a, s + i) * a.R_st] = Ret<T>::out(acc);
    }
  }
  for (; s < s1; ++s) {
    acc = Ret<T>::in(r[frame(a, s) * a.r_st]) + a.gamma * acc;
    if (STORE) R[frame(a, s) * a.R_st] = Ret<T>::out(acc);
  }
  if (!STORE) a.carry[c * a.N + n] = acc;
}

// partial[c] -> the return that enters chunk c: one thread per column, the chunks in order
template <typename C>
__global__ void __launch_bounds__(kRetThreads) return_carry_kernel(C *carry, int64_t N, int64_t chunks, C gpow) {
  const int64_t n = (int64_t)blockIdx.x * kRetThreads + threadIdx.x;
  if (n >= N) return;
  C in = C(0);
  for (int64_t c = 0; c < chunks; ++c) {
    const C p = c + 1 < chunks ? carry[c * N + n] : C(0);  // (pass 1 skips the last chunk: nothing follows it)
    carry[c * N + n] = in;
    in = p + gpow * in;
  }
}

template <typename T, int STORE>
__global__ void __launch_bounds__(kRetThreads) return_rows_kernel(const ReturnArgs<typename Ret<T>::C> a) {
  using C = typename Ret<T>::C;
  const int lane = lane_id();
  const int64_t item = (int64_t)blockIdx.x * (kRetThreads / PDT_WAVE) + (threadIdx.x >> 6);
  if (item >= a.chunks * a.N) return;  // (wave-uniform)
  const int64_t c = item / a.N, n = item % a.N;
  const T *__restrict__ r = (const T *)a.r + n * a.r_sn;
  T *__restrict__ R = (T *)a.R + n * a.R_sn;
  // gamma^d of the ladder (uniform), and gamma^(lane + 1) by the same ladder
  C gd[6];
  gd[0] = a.gamma;
#pragma unroll
  for (int i = 1; i < 6; ++i) gd[i] = gd[i - 1] * gd[i - 1];
  C glane = a.gamma;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const C up = __shfl_up(glane, 1u << i, PDT_WAVE);
    if (lane >= (1 << i)) glane = glane * up;
  }
  const int64_t s0 = c * a.chunk;
  const int64_t s1 = s0 + a.chunk < a.T ? s0 + a.chunk : a.T;
  C carry = (STORE && a.carry != nullptr) ? a.carry[c * a.N + n] : C(0);
  for (int64_t base = s0; base < s1; base += PDT_WAVE) {
    const int64_t s = base + lane;
    const bool live = s < s1;
    const int64_t t = frame(a, live ? s : s0);
    C v = live ? Ret<T>::in(r[t * a.r_st]) : C(0);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const C up = __shfl_up(v, 1u << i, PDT_WAVE);
      if (lane >= (1 << i)) v = v + gd[i] * up;
    }
    v = v + glane * carry;
    if (STORE && live) R[t * a.R_st] = Ret<T>::out(v);
    carry = __shfl(v, PDT_WAVE - 1, PDT_WAVE);  // (of a full pass; a short one is the chunk's last)
  }
  // pass 1 runs only chunks that another follows, which are whole passes: lane 63 of the last is the partial
  if (!STORE && lane == 0) a.carry[c * a.N + n] = carry;
}

// gamma^L in the compute type by squaring and multiplying; false if some power on the way is not finite
template <typename C> bool power(C gamma, int64_t L, C *out) {
  C p = C(1), sq = gamma;
  for (int64_t e = L; e; e >>= 1) {
    if (!std::isfinite(sq)) return false;
    if (e & 1) p = p * sq;
    sq = sq * sq;
  }
  *out = p;
  return std::isfinite(p);
}

struct Plan {
  bool rows;      // the rows kernel (lane = step)
  int64_t chunk;  // steps per chunk (T: no split)
};

// what depends on the shape alone; gamma may still withdraw the split or the rows kernel
Plan plan_for(int64_t T, int64_t N, int64_t R_st, int64_t R_sn) {
  Plan p;
  p.rows = N == 1 || (T > 1 && llabs(R_st) < llabs(R_sn));
  const int64_t waves = p.rows ? N : (N + PDT_WAVE - 1) / PDT_WAVE;
  const int64_t L = p.rows ? kRowSegment : kColChunk;
  p.chunk = (waves < kFillWaves && T > L) ? L : T;
  return p;
}

template <typename T>
int launch(const void *r, void *R, int64_t T_, int64_t N, int64_t r_st, int64_t r_sn, int64_t R_st, int64_t R_sn,
           double gamma, int reverse, void *workspace, int64_t workspace_bytes, hipStream_t s) {
  using C = typename Ret<T>::C;
  Plan p = plan_for(T_, N, R_st, R_sn);
  C gpow = C(0), g64;
  if (p.rows && !power<C>((C)gamma, PDT_WAVE, &g64)) p = Plan{false, T_};
  if (p.chunk < T_ && !power<C>((C)gamma, p.chunk, &gpow)) p = Plan{false, T_};
  ReturnArgs<C> a;
  a.r = r, a.R = R, a.carry = nullptr;
  a.T = T_, a.N = N, a.r_st = r_st, a.r_sn = r_sn, a.R_st = R_st, a.R_sn = R_sn;
  a.chunk = p.chunk, a.chunks = (T_ + p.chunk - 1) / p.chunk;
  a.gamma = (C)gamma, a.reverse = reverse;
  const int64_t per_block = p.rows ? kRetThreads / PDT_WAVE : kRetThreads;
  const int64_t cols = p.rows ? N : (N + kRetThreads - 1) / kRetThreads;  // blocks (rows: items) per chunk
  const int64_t blocks = p.rows ? (a.chunks * cols + per_block - 1) / per_block : a.chunks * cols;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  const dim3 grid((unsigned)blocks), blk(kRetThreads);
  if (a.chunks > 1) {
    if (workspace == nullptr || workspace_bytes < a.chunks * N * (int64_t)sizeof(C)) return PDT_E_ARG;
    a.carry = (C *)workspace;
    ReturnArgs<C> first = a;  // pass 1: every chunk but the last, whose partial nothing would read
    first.chunks = a.chunks - 1;
    const int64_t first_blocks = p.rows ? (first.chunks * cols + per_block - 1) / per_block : first.chunks * cols;
    const dim3 first_grid((unsigned)first_blocks);
    if (p.rows) hipLaunchKernelGGL((return_rows_kernel<T, 0>), first_grid, blk, 0, s, first);
    else hipLaunchKernelGGL((return_columns_kernel<T, 0>), first_grid, blk, 0, s, first);
    hipLaunchKernelGGL(return_carry_kernel<C>, dim3((unsigned)((N + kRetThreads - 1) / kRetThreads)), blk, 0, s,
                       a.carry, N, a.chunks, gpow);
  }
  if (p.rows) hipLaunchKernelGGL((return_rows_kernel<T, 1>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((return_columns_kernel<T, 1>), grid, blk, 0, s, a);
  return (int)hipGetLastError();
}

bool bad_shape(int64_t T, int64_t N, int dtype) { return T < 0 || N < 0 || dtype < RET_F32 || dtype > RET_BF16; }

}  // namespace
}  // namespace pdt

extern "C" int64_t pdt_time_distributed_return_workspace_bytes(int64_t T, int64_t N, int dtype, int64_t R_st,
                                                               int64_t R_sn) {
  if (pdt::bad_shape(T, N, dtype)) return -1;
  if (T == 0 || N == 0) return 0;
  const pdt::Plan p = pdt::plan_for(T, N, R_st, R_sn);
  if (p.chunk >= T) return 0;
  return (T + p.chunk - 1) / p.chunk * N * (int64_t)(dtype == pdt::RET_F64 ? sizeof(double) : sizeof(float));
}

extern "C" int pdt_time_distributed_return(const void *r, int dtype, int64_t T, int64_t N, int64_t r_st, int64_t r_sn,
                                           const double *gamma, int reverse, void *R, int64_t R_st, int64_t R_sn,
                                           void *workspace, int64_t workspace_bytes, void *stream) {
  if (pdt::bad_shape(T, N, dtype) || gamma == nullptr || (reverse != 0 && reverse != 1)) return PDT_E_ARG;
  if (T == 0 || N == 0) return PDT_OK;
  if (r == nullptr || R == nullptr || workspace_bytes < 0) return PDT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case pdt::RET_F32:
      return pdt::launch<float>(r, R, T, N, r_st, r_sn, R_st, R_sn, *gamma, reverse, workspace, workspace_bytes, s);
    case pdt::RET_F64:
      return pdt::launch<double>(r, R, T, N, r_st, r_sn, R_st, R_sn, *gamma, reverse, workspace, workspace_bytes, s);
    case pdt::RET_F16:
      return pdt::launch<__half>(r, R, T, N, r_st, r_sn, R_st, R_sn, *gamma, reverse, workspace, workspace_bytes, s);
    default:
      return pdt::launch<__hip_bfloat16>(r, R, T, N, r_st, r_sn, R_st, R_sn, *gamma, reverse, workspace,
                                         workspace_bytes, s);
  }
}
