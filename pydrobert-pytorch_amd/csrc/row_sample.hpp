// One row of scores through a wave: its (maximum, log-sum-exp) and the sampling rule of every random-walk
// kernel (random_walk.hip).  BeamSearch's step kernels (beam_step.hip) and the row-stats kernel (beam_search_table.hip) use the same
// row_log_softmax_stats, so a row's statistics have the same bits whichever kernel forms them.
#pragma once
#include "wave_select.hpp"

namespace pdt {

// maximum and log-sum-exp of a strided row (two passes, eight loads in flight)
__device__ __forceinline__ void row_log_softmax_stats(const float *x, const int64_t sx, const int V, float &mx_out,
                                                      float &lse_out) {
  const int lane = lane_id();
  float mx = -PDT_INF;
  int v = lane;
  for (; v + 7 * PDT_WAVE < V; v += 8 * PDT_WAVE) {
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = x[(int64_t)(v + i * PDT_WAVE) * sx];
#pragma unroll
    for (int i = 0; i < 8; ++i) mx = fmaxf(mx, t[i]);
  }
  for (; v < V; v += PDT_WAVE) mx = fmaxf(mx, x[(int64_t)v * sx]);
  mx = wave_max_f(mx);
  float s = 0.0f;
  v = lane;
  for (; v + 7 * PDT_WAVE < V; v += 8 * PDT_WAVE) {
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = x[(int64_t)(v + i * PDT_WAVE) * sx];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += expf(t[i] - mx);
  }
  for (; v < V; v += PDT_WAVE) s += expf(x[(int64_t)v * sx] - mx);
  s = wave_sum_f(s);
  mx_out = mx;
  lse_out = logf(s);
}

// inclusive prefix sum over the wave: wave_sum_f's DPP chain without the final read of lane 63
__device__ __forceinline__ float wave_incl_scan_f(float x) {
  float v = x;
  asm volatile(
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xe\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "s_nop 1"
      : "+v"(v));
  return v;
}

// The sampling rule.  Row x[0..V) (stride sx) of log-weights with maximum mx and log-sum-exp lse
// (row_log_softmax_stats), u in [0, 1): w_v = exp(x_v - mx), Z = exp(lse); the token is the smallest v with
// w_v > 0 whose running prefix sum of w exceeds u * Z; when rounding leaves none, the largest v with w_v > 0.
// The prefix is formed chunk by chunk (64 tokens, one per lane) and the scan stops at the chunk that crosses
// u * Z: a row costs about half its length in reads.  Returns -1 for a row with no positive finite mass
// (every entry -inf, a NaN, or +inf) -- nothing can be drawn from it.  Wave-uniform result.
__device__ __forceinline__ int sample_row(const float *x, const int64_t sx, const int V, const float mx,
                                          const float lse, const float u) {
  if (!(mx > -PDT_INF && mx < PDT_INF) || !(lse == lse)) return -1;  // (a NaN entry makes the sum NaN)
  const float target = u * expf(lse);
  const int lane = lane_id();
  float carry = 0.0f;
  int last = -1;
  float xn = lane < V ? x[(int64_t)lane * sx] : -PDT_INF;
  for (int v0 = 0; v0 < V; v0 += PDT_WAVE) {
    const float xc = xn;
    if (v0 + PDT_WAVE < V) {  // the next chunk's load in flight while this one is scanned
      const int vn = v0 + PDT_WAVE + lane;
      xn = vn < V ? x[(int64_t)vn * sx] : -PDT_INF;
    }
    const float w = expf(xc - mx);  // (0 beyond V)
    const float p = carry + wave_incl_scan_f(w);
    const unsigned long long hit = __ballot(w > 0.0f && p > target);
    if (hit) return v0 + __builtin_ctzll(hit);
    const unsigned long long pos = __ballot(w > 0.0f);
    if (pos) last = v0 + 63 - __builtin_clzll(pos);
    carry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), 63));
  }
  return last;
}

// a walk's log-probability after drawing a token with score x_tok from a row with statistics (mx, lse):
// lp + log_softmax(row)[tok], one expression for every kernel (the routes agree bit for bit)
__device__ __forceinline__ float walk_lp_add(const float lp, const float x_tok, const float mx, const float lse) {
  return lp + ((x_tok - mx) - lse);
}

}  // namespace pdt
