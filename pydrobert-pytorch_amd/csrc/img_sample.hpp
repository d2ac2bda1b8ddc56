// Device code the image families share (spline.hip, spec_augment.hip, image_warp.hip): the radial
// basis functions, grid_sample's coordinate arithmetic, warp_1d_grid's spline in closed form, and the
// division-free index split.
#pragma once
#include <cfloat>
#include <cmath>

#include "pdt_common.hpp"

namespace pdt {

__device__ __forceinline__ double phi_d(double r, int order) {
  // _img.py:59-64; eps = float32 epsilon (train/query points are cast to float, :142-143)
  double rk = 1.0;
  for (int i = 0; i < order; ++i) rk *= r;
  if (order & 1) return rk;
  return rk * log(fmax(r, (double)FLT_EPSILON));
}
__device__ __forceinline__ float phi_f(float r, int order) {
  float rk = 1.0f;
  for (int i = 0; i < order; ++i) rk *= r;
  if (order & 1) return rk;
  return rk * logf(fmaxf(r, FLT_EPSILON));
}

// phi(r) from the SQUARED distance, float32, for the per-pixel spline evaluation of the sparse
// warp (7-100 centres per pixel: this is where its time goes).  Even orders need no square
// root (r^k log r = d2^(k/2) * log(d2) / 2) and the logarithm is the hardware v_log_f32
// (1 ulp) instead of OCML's logf; order 2 -- the default -- costs ~8 VALU per centre
// instead of ~35.
// ORDER = 1, 2, 3: that order, compiled without branches; ORDER = 0: any order (runtime).
// ln(x) for finite x >= eps^2 (1.4e-14: no denormals, no infinities): the arithmetic of __logf
// without its guards -- v_log_f32 (log2) and the compensated product with ln 2 in two pieces --
// five instructions instead of twelve, the same bits for these arguments.
__device__ __forceinline__ float ln_fast(float x) {
  const float r = __builtin_amdgcn_logf(x);
  const float hi = __uint_as_float(0x3f317217u), lo = __uint_as_float(0x3377d1cfu);  // ln 2 = hi + lo
  const float t = r * hi;
  float e = __builtin_fmaf(r, hi, -t);
  e = __builtin_fmaf(r, lo, e);
  return t + e;
}

template <int ORDER>
__device__ __forceinline__ float phi_from_d2(float d2, int order) {
#ifndef PDT_WARP_REFERENCE_PHI
  // d2 + 1e-37 is d2 itself for every distance that is not 0 (and 0 * ln(1e-37) = 0 there); the
  // half and ln 2 folded into one factor
  if (ORDER == 2) return d2 * (__builtin_amdgcn_logf(d2 + 1e-37f) * 0.34657359f);
#endif
  if (ORDER == 2) return d2 * (0.5f * ln_fast(fmaxf(d2, FLT_EPSILON * FLT_EPSILON)));
  if (ORDER == 1) return sqrtf(d2);
  if (ORDER == 3) return d2 * sqrtf(d2);
  float pw = 1.0f;  // d2^(order / 2)
  for (int i = 0; i < (order >> 1); ++i) pw *= d2;
  if (order & 1) return pw * sqrtf(d2);
  return pw * (0.5f * ln_fast(fmaxf(d2, FLT_EPSILON * FLT_EPSILON)));
}

// ---- grid_sample arithmetic (align_corners = False) -----------------------------------------
enum { PAD_ZEROS = 0, PAD_BORDER = 1, PAD_REFLECTION = 2 };
enum { INTERP_BILINEAR = 0, INTERP_NEAREST = 1 };

// (CT: the coordinate type -- float, or double for float64 images, whose grid the reference forms
// and samples in float64, _img.py:420-436)
template <typename CT>
__device__ __forceinline__ CT unnormalize(CT g, int size) {
  return ((g + CT(1)) * (CT)size - CT(1)) * CT(0.5);
}
template <typename CT>
__device__ __forceinline__ CT clip_coord(CT x, int size) {
  return fmin((CT)(size - 1), fmax(x, CT(0)));
}
__device__ __forceinline__ float clip_coord(float x, int size) {
  return fminf((float)(size - 1), fmaxf(x, 0.0f));
}
template <typename CT>
__device__ __forceinline__ CT reflect_coord(CT x, int twice_low, int twice_high) {
  if (twice_low == twice_high) return CT(0);
  const CT mn = (CT)twice_low * CT(0.5), span = (CT)(twice_high - twice_low) * CT(0.5);
  x = fabs(x - mn);
  const CT extra = fmod(x, span);
  const int flips = (int)floor(x / span);
  return (flips & 1) ? span - extra + mn : extra + mn;
}
__device__ __forceinline__ float reflect_coord(float x, int twice_low, int twice_high) {
  if (twice_low == twice_high) return 0.0f;
  const float mn = (float)twice_low * 0.5f, span = (float)(twice_high - twice_low) * 0.5f;
  x = fabsf(x - mn);
  const float extra = fmodf(x, span);
  const int flips = (int)floorf(x / span);
  return (flips & 1) ? span - extra + mn : extra + mn;
}
template <typename CT>
__device__ __forceinline__ CT source_index(CT g, int size, int padding) {
  CT x = unnormalize(g, size);
  if (padding == PAD_BORDER) x = clip_coord(x, size);
  else if (padding == PAD_REFLECTION) x = clip_coord(reflect_coord(x, -1, 2 * size - 1), size);
  return x;
}

// The derivatives of clip_coord / reflect_coord with respect to their argument, as torch's
// clip_coordinates_set_grad / reflect_coordinates_set_grad choose them at the kinks: the clip passes
// nothing at or beyond its limits (x <= 0, x >= size - 1); the reflection's sign is that of x - low,
// turned once more on an odd number of folds (a zero span passes nothing).
template <typename CT>
__device__ __forceinline__ CT clip_coord_factor(CT x, int size) {
  return (x <= CT(0) || x >= (CT)(size - 1)) ? CT(0) : CT(1);
}
template <typename CT>
__device__ __forceinline__ CT reflect_coord_factor(CT x, int twice_low, int twice_high) {
  if (twice_low == twice_high) return CT(0);
  const CT mn = (CT)twice_low * CT(0.5), span = (CT)(twice_high - twice_low) * CT(0.5);
  x -= mn;
  const CT sign = x < CT(0) ? CT(-1) : CT(1);
  const int flips = (int)floor(fabs(x) / span);
  return (flips & 1) ? -sign : sign;
}
// d source_index / d unnormalize(g): the padding rule's factor (zeros padding: 1)
template <typename CT>
__device__ __forceinline__ CT source_index_factor(CT g, int size, int padding) {
  const CT x = unnormalize(g, size);
  if (padding == PAD_BORDER) return clip_coord_factor(x, size);
  if (padding == PAD_REFLECTION)
    return reflect_coord_factor(x, -1, 2 * size - 1) * clip_coord_factor(reflect_coord(x, -1, 2 * size - 1), size);
  return CT(1);
}

// warp_1d_grid's spline (_img.py:283-302) in closed form.  Knots c0 < c1 < c2 = {lo, dst, up}, values
// {lo, src, up}; the bordered 5 x 5 system [[A, [c 1]], [[c 1]^T, 0]] [w; v] = [f; 0] with A_ij =
// phi(|c_i - c_j|): the two constraints leave w = alpha u, u = (c1 - c2, c2 - c0, c0 - c1); u kills
// the affine part, so alpha = u.f / u^T A u, and v from rows 0 and 2 of f - alpha A u = v0 c + v1.
struct Warp1D {
  double c[3], w[3], v0, v1;
};
__device__ inline Warp1D warp_1d_spline(double src, double flow, double len, int T, int order) {
  const double eps = (double)FLT_EPSILON;
  double s = fmax(fmin(src, len - 1.0), 0.0);
  double d = fmax(fmin(s + flow, len - 1.0), 0.0);
  s = (2.0 * s + 1.0) / T - 1.0;
  d = (2.0 * d + 1.0) / T - 1.0;
  const double lo = 1.0 / T - 1.0 - eps, up = (2.0 * len - 1.0) / T - 1.0 + eps;
  Warp1D r;
  r.c[0] = lo; r.c[1] = d; r.c[2] = up;
  const double f0 = lo, f1 = s, f2 = up;
  const double u0 = d - up, u1 = up - lo, u2 = lo - d;
  const double a = phi_d(fabs(d - lo), order), b = phi_d(fabs(up - lo), order), e = phi_d(fabs(up - d), order);
  const double Au0 = a * u1 + b * u2, Au1 = a * u0 + e * u2, Au2 = b * u0 + e * u1;
  const double den = u0 * Au0 + u1 * Au1 + u2 * Au2;
  const double alpha = den != 0.0 ? (u0 * f0 + u1 * f1 + u2 * f2) / den : 0.0;
  r.w[0] = alpha * u0; r.w[1] = alpha * u1; r.w[2] = alpha * u2;
  const double r0 = f0 - alpha * Au0, r2 = f2 - alpha * Au2;
  r.v0 = (r2 - r0) / (up - lo);
  r.v1 = r0 - r.v0 * lo;
  return r;
}
__device__ __forceinline__ float warp_1d_eval(const Warp1D &sp, int j, int T, int order) {
  const double t = (2.0 * j + 1.0) / T - 1.0;
  return (float)(sp.w[0] * phi_d(fabs(t - sp.c[0]), order) + sp.w[1] * phi_d(fabs(t - sp.c[1]), order) +
                 sp.w[2] * phi_d(fabs(t - sp.c[2]), order) + sp.v0 * t + sp.v1);
}

// idx -> (row, col) = (idx / width, idx % width) without an integer division, for idx below 2^23 (a
// float holds idx + 0.5 exactly): the quotient estimated with inv = 1.0f / width, one step of fix-up.
__device__ __forceinline__ void split_index(int idx, float inv, int width, int &row, int &col) {
  row = (int)(((float)idx + 0.5f) * inv);
  col = idx - row * width;
  if (col < 0) { --row; col += width; }
  if (col >= width) { ++row; col -= width; }
}

}  // namespace pdt
