// SpecAugment for gfx950: the parameters from one tensor of uniform draws, and their application.
//
// Replaces, from the reference's _img.py:
//   spec_augment_draw_parameters (:1056-1139) -> spec_augment_draw_kernel
//   spec_augment_apply_parameters (:1142-1211)-> spec_augment_apply_kernel: ONE pass that reads
//       feats once and writes the result once; the reference materialises an (N,T,F,2) grid
//       (64 % of its time is the torch.stack building it) and calls grid_sample + masked_fill
// Gathers follow torch.nn.functional.grid_sample(align_corners=False) arithmetic in float32; the
// coordinate helpers and warp_1d_grid's closed-form spline come from img_sample.hpp.
#include <algorithm>
#include <initializer_list>

#include "img_sample.hpp"

namespace pdt {

// E: the features' element type (float, f16_t, bf16_t: pdt_common.hpp).  The arithmetic is float32 for each;
// a half element is widened exactly where it is read and rounded once (to nearest even) where it is stored.
template <typename E>
struct SpecAugArgsT {
  const E *feats; int64_t f_sn, f_st, f_sf;  // strides in elements
  const float *tgrid, *fgrid;          // (N,T) / (N,F) normalised grids or null
  const int64_t *t0, *tl, *f0, *fl;    // (N,MT) / (N,MF) masks or null
  int N, T, F, MT, MF;
  E *out;                              // (N,T,F) contiguous
  // the time warp by its PARAMETERS instead of a grid (spec_augment_rows_kernel only): w_0, w (N,)
  // float and the lengths (N,) int64 (null: all T) -- the three-knot spline of warp_1d_grid is solved
  // in closed form and evaluated where the rows are planned, no (N, T) grid in memory
  const float *tw_src, *tw_flow; const int64_t *tw_len; int tw_order;
  // (with tw_len) set to 1 by an utterance whose length is not in [1, T]: the reference's input check
  // (_img.py:1037-1041) made where the lengths are read; device-visible memory the caller zeroed, or null
  int32_t *bad_lengths;
};
using SpecAugArgs = SpecAugArgsT<float>;

// Four neighbouring elements as one access: 16 bytes of float32, 8 bytes of a half type.
__device__ __forceinline__ float4 load4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 load4(const f16_t *p) {
  typedef f16_t f16x4 __attribute__((ext_vector_type(4)));
  const f16x4 h = *reinterpret_cast<const f16x4 *>(p);
  return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
}
__device__ __forceinline__ float4 load4(const bf16_t *p) {
  const uint2 u = *reinterpret_cast<const uint2 *>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
// (elem_store's roundings, as bits: the float16 value is kept from being fused with a product in front of it)
__device__ __forceinline__ unsigned half_bits(const f16_t *, float x) {
  asm volatile("" : "+v"(x));
  return (unsigned)__builtin_bit_cast(unsigned short, (f16_t)x);
}
__device__ __forceinline__ unsigned half_bits(const bf16_t *, float x) {
  const unsigned u = __float_as_uint(x);
  return x != x ? 0x7FC0u : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
template <typename E>
__device__ __forceinline__ uint2 pack4(const E *tag, const float4 v) {
  return make_uint2(half_bits(tag, v.x) | (half_bits(tag, v.y) << 16), half_bits(tag, v.z) | (half_bits(tag, v.w) << 16));
}
__device__ __forceinline__ void store4(float *p, const float4 v) { *reinterpret_cast<float4 *>(p) = v; }
template <typename E>
__device__ __forceinline__ void store4(E *p, const float4 v) { *reinterpret_cast<uint2 *>(p) = pack4(p, v); }
// (non-temporal: written once, never read here -- apply 0.30 -> 0.29 ms on the box that measured both)
__device__ __forceinline__ void store4_nt(float *p, const float4 v) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4 *>(p));
}
template <typename E>
__device__ __forceinline__ void store4_nt(E *p, const float4 v) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  const uint2 u = pack4(p, v);
  __builtin_nontemporal_store(u32x2{u.x, u.y}, reinterpret_cast<u32x2 *>(p));
}


// One pass: bilinear gather along time and frequency + band masks.  Workgroup = 256 threads
// walking a contiguous range of (t, f) positions of one utterance.
template <typename E>
__global__ void __launch_bounds__(256) spec_augment_apply_kernel(const SpecAugArgsT<E> a, int tiles) {
  const int64_t n = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int T = a.T, F = a.F;
  const int rows_per_tile = (T + tiles - 1) / tiles;
  const int t_begin = tile * rows_per_tile, t_end = min(T, t_begin + rows_per_tile);
  const E *fn = a.feats + n * a.f_sn;
  for (int idx = t_begin * F + (int)threadIdx.x; idx < t_end * F; idx += 256) {
    const int t = idx / F, f = idx - t * F;
    bool masked = false;
    for (int m = 0; m < a.MT; ++m) {
      const int64_t s = a.t0[n * a.MT + m];
      masked = masked || (t >= s && t < s + a.tl[n * a.MT + m]);
    }
    for (int m = 0; m < a.MF; ++m) {
      const int64_t s = a.f0[n * a.MF + m];
      masked = masked || (f >= s && f < s + a.fl[n * a.MF + m]);
    }
    float v = 0.0f;
    if (!masked) {
      if (!a.tgrid && !a.fgrid) {
        v = elem_load(fn + ((int64_t)t * a.f_st + (int64_t)f * a.f_sf));
      } else {
        // identity grids when only one axis is warped (:1173-1180)
        const float gy = a.tgrid ? a.tgrid[n * T + t] : (2.0f * (float)t + 1.0f) / (float)T - 1.0f;
        const float gx = a.fgrid ? a.fgrid[n * F + f] : (2.0f * (float)f + 1.0f) / (float)F - 1.0f;
        const float iy = clip_coord(unnormalize(gy, T), T), ix = clip_coord(unnormalize(gx, F), F);
        const float y0f = floorf(iy), x0f = floorf(ix);
        const int y0 = (int)y0f, x0 = (int)x0f, y1 = y0 + 1, x1 = x0 + 1;
        const float wy1 = iy - y0f, wx1 = ix - x0f, wy0 = (y0f + 1.0f) - iy, wx0 = (x0f + 1.0f) - ix;
        const E *r0 = fn + (int64_t)y0 * a.f_st;
        const E *r1 = fn + (int64_t)min(y1, T - 1) * a.f_st;
        const int64_t c0 = (int64_t)x0 * a.f_sf, c1 = (int64_t)min(x1, F - 1) * a.f_sf;
        // taps outside the image carry weight 0 under border padding
        v = elem_load(r0 + c0) * (wx0 * wy0);
        if (x1 < F) v += elem_load(r0 + c1) * (wx1 * wy0);
        if (y1 < T) v += elem_load(r1 + c0) * (wx0 * wy1);
        if (x1 < F && y1 < T) v += elem_load(r1 + c1) * (wx1 * wy1);
      }
    }
    elem_store(a.out + ((n * T + t) * (int64_t)F + f), v);
  }
}

// Fast path of the above for the common SpecAugment setting (no frequency warp, F % 4 == 0,
// unit stride along F): an output row is a 2-tap blend of two source rows, so a thread moves
// four elements -- 16-byte coalesced loads and stores of float32, 8-byte ones of a half type.  Per-row
// (source row, weights, time mask) and per-column (frequency mask) decisions are made once per workgroup
// and kept in LDS.
constexpr int kRowsPerTile = 256;
template <typename E>
__global__ void __launch_bounds__(256) spec_augment_rows_kernel(const SpecAugArgsT<E> a, int tiles) {
  __shared__ int row_y0[kRowsPerTile];      // source row, or -1 when the row is masked
  __shared__ float row_w1[kRowsPerTile];    // weight of source row y0 + 1
  __shared__ unsigned col_keep[64];         // per float4 column: 4 keep bits
  const int64_t n = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int T = a.T, F4 = a.F >> 2;
  const int t_begin = tile * kRowsPerTile, t_end = min(T, t_begin + kRowsPerTile);
  const int tid = (int)threadIdx.x;
  const bool warped = a.tgrid != nullptr || a.tw_src != nullptr;
  __shared__ Warp1D spline;
  if (a.tw_src) {  // (uniform: one extra barrier per workgroup)
    if (tid == 0) {
      const int64_t len = a.tw_len ? a.tw_len[n] : (int64_t)T;
      if (a.bad_lengths && tile == 0 && (len > T || len <= 0)) *a.bad_lengths = 1;
      spline = warp_1d_spline((double)a.tw_src[n], (double)a.tw_flow[n], (double)len, T, a.tw_order);
    }
    __syncthreads();
  }
  if (t_begin + tid < t_end) {
    const int t = t_begin + tid;
    bool masked = false;
    for (int m = 0; m < a.MT; ++m) {
      const int64_t s = a.t0[n * a.MT + m];
      masked = masked || (t >= s && t < s + a.tl[n * a.MT + m]);
    }
    int y0 = t;
    float w1 = 0.0f;
    if (warped) {
      const float g = a.tw_src ? warp_1d_eval(spline, t, T, a.tw_order) : a.tgrid[n * T + t];
      const float iy = clip_coord(unnormalize(g, T), T);
      const float y0f = floorf(iy);
      y0 = (int)y0f;
      w1 = iy - y0f;
    }
    row_y0[tid] = masked ? -1 : y0;
    row_w1[tid] = w1;
  }
  for (int c = tid; c < F4; c += 256) {
    unsigned keep = 0u;
    for (int j = 0; j < 4; ++j) {
      const int f = 4 * c + j;
      bool fm = false;
      for (int m = 0; m < a.MF; ++m) {
        const int64_t s = a.f0[n * a.MF + m];
        fm = fm || (f >= s && f < s + a.fl[n * a.MF + m]);
      }
      keep |= fm ? 0u : (1u << j);
    }
    col_keep[c] = keep;
  }
  __syncthreads();
  const E *fn = a.feats + n * a.f_sn;
  E *on = a.out + n * (int64_t)T * a.F;
  const float inv = 1.0f / (float)F4;
  const int total = (t_end - t_begin) * F4;
  for (int idx = tid; idx < total; idx += 256) {
    int r = (int)(((float)idx + 0.5f) * inv);  // (split_index written out: called here, the compiler schedules this loop differently)
    int f4 = idx - r * F4;
    if (f4 < 0) { --r; f4 += F4; }
    if (f4 >= F4) { ++r; f4 -= F4; }
    const int y0 = row_y0[r];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (y0 >= 0) {
      const float w1 = row_w1[r];
      const float4 r0 = load4(fn + (int64_t)y0 * a.f_st + 4 * f4);
      if (warped && y0 + 1 < T) {
        // same arithmetic as the 4-tap form with wx0 = 1, wx1 = 0; a row at y0 + 1 == T lies
        // outside the image and carries weight 0 under border padding
        const float w0 = ((float)y0 + 1.0f) - ((float)y0 + w1);
        const float4 r1 = load4(fn + (int64_t)(y0 + 1) * a.f_st + 4 * f4);
        v.x = r0.x * w0 + r1.x * w1;
        v.y = r0.y * w0 + r1.y * w1;
        v.z = r0.z * w0 + r1.z * w1;
        v.w = r0.w * w0 + r1.w * w1;
      } else if (warped) {
        const float w0 = ((float)y0 + 1.0f) - ((float)y0 + w1);
        v.x = r0.x * w0; v.y = r0.y * w0; v.z = r0.z * w0; v.w = r0.w * w0;
      } else {
        v = r0;
      }
      const unsigned keep = col_keep[f4];
      v.x = (keep & 1u) ? v.x : 0.0f;
      v.y = (keep & 2u) ? v.y : 0.0f;
      v.z = (keep & 4u) ? v.z : 0.0f;
      v.w = (keep & 8u) ? v.w : 0.0f;
    }
    store4_nt(on + (int64_t)(t_begin + r) * a.F + 4 * f4, v);
  }
}

// Adjoint of the two kernels above with respect to the features: every unmasked output element
// scatters its gradient to its (up to) four taps.  grad_feats is zeroed by the caller; the
// accumulation uses the hardware float atomic (order of addition is not fixed, like
// grid_sample's own backward).  `grad_feats` is float32 whenever there is a grid -- a half element cannot
// hold a running sum: for E a half type the caller's workspace, rounded once by round_rows_kernel -- and E
// with no grid at all, where every element has its one writer.
template <typename E>
__global__ void __launch_bounds__(256)
spec_augment_backward_kernel(const SpecAugArgsT<E> a, const E *__restrict__ grad_out,
                             float *__restrict__ grad_feats, int tiles) {
  const int64_t n = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int T = a.T, F = a.F;
  const int rows_per_tile = (T + tiles - 1) / tiles;
  const int t_begin = tile * rows_per_tile, t_end = min(T, t_begin + rows_per_tile);
  float *gn = grad_feats + n * (int64_t)T * F;
  for (int idx = t_begin * F + (int)threadIdx.x; idx < t_end * F; idx += 256) {
    const int t = idx / F, f = idx - t * F;
    bool masked = false;
    for (int m = 0; m < a.MT; ++m) {
      const int64_t s = a.t0[n * a.MT + m];
      masked = masked || (t >= s && t < s + a.tl[n * a.MT + m]);
    }
    for (int m = 0; m < a.MF; ++m) {
      const int64_t s = a.f0[n * a.MF + m];
      masked = masked || (f >= s && f < s + a.fl[n * a.MF + m]);
    }
    if (masked) continue;
    const float g = elem_load(grad_out + ((n * T + t) * (int64_t)F + f));
    if (!a.tgrid && !a.fgrid) {
      // one-to-one: no other writer (grad_feats is of E here)
      if constexpr (sizeof(E) == sizeof(float)) gn[(int64_t)t * F + f] = g;
      else elem_store(reinterpret_cast<E *>(grad_feats) + ((n * T + t) * (int64_t)F + f), g);
      continue;
    }
    const float gy = a.tgrid ? a.tgrid[n * T + t] : (2.0f * (float)t + 1.0f) / (float)T - 1.0f;
    const float gx = a.fgrid ? a.fgrid[n * F + f] : (2.0f * (float)f + 1.0f) / (float)F - 1.0f;
    const float iy = clip_coord(unnormalize(gy, T), T), ix = clip_coord(unnormalize(gx, F), F);
    const float y0f = floorf(iy), x0f = floorf(ix);
    const int y0 = (int)y0f, x0 = (int)x0f, y1 = y0 + 1, x1 = x0 + 1;
    const float wy1 = iy - y0f, wx1 = ix - x0f, wy0 = (y0f + 1.0f) - iy, wx0 = (x0f + 1.0f) - ix;
    float *r0 = gn + (int64_t)y0 * F, *r1 = gn + (int64_t)min(y1, T - 1) * F;
    unsafeAtomicAdd(r0 + x0, g * (wx0 * wy0));
    if (x1 < F && wx1 != 0.0f) unsafeAtomicAdd(r0 + x1, g * (wx1 * wy0));
    if (y1 < T && wy1 != 0.0f) unsafeAtomicAdd(r1 + x0, g * (wx0 * wy1));
    if (x1 < F && y1 < T && wx1 != 0.0f && wy1 != 0.0f) unsafeAtomicAdd(r1 + x1, g * (wx1 * wy1));
  }
}

// Adjoint of spec_augment_rows_kernel written as a GATHER (no atomics, no zero fill,
// deterministic): a workgroup owns 256 source rows of one utterance; a source row y collects
// w0(t) * g[t] from the output rows t sampled at y0(t) = y and w1(t) * g[t] from those at
// y0(t) = y - 1.  Warp grids are non-decreasing (warp_1d_grid pins both ends), so those rows
// form one contiguous range found by binary search over the per-row table in LDS; for any
// other grid the range degrades to all rows (still exact, just slower).
template <typename E>
__global__ void __launch_bounds__(256)
spec_augment_rows_backward_kernel(const SpecAugArgsT<E> a, const E *__restrict__ grad_out,
                                  E *__restrict__ grad_feats, int tiles) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int T = a.T, F4 = a.F >> 2;
  int *sy0 = reinterpret_cast<int *>(smem);             // [T] source row of output row t
  float *sw0 = reinterpret_cast<float *>(sy0 + T);      // [T] weight of row y0 (0 if masked)
  float *sw1 = sw0 + T;                                 // [T] weight of row y0 + 1
  int *lb = reinterpret_cast<int *>(sw1 + T);           // [258] first t with y0(t) >= y_b - 1 + i
  unsigned *col_keep = reinterpret_cast<unsigned *>(lb + 260);  // [64]
  const int64_t n = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x % tiles);
  const int y_b = tile * kRowsPerTile, y_e = min(T, y_b + kRowsPerTile);
  const int tid = (int)threadIdx.x;
  bool bad = false;
  for (int t = tid; t < T; t += 256) {
    bool masked = false;
    for (int m = 0; m < a.MT; ++m) {
      const int64_t s = a.t0[n * a.MT + m];
      masked = masked || (t >= s && t < s + a.tl[n * a.MT + m]);
    }
    int y0 = t;
    float w0 = 1.0f, w1 = 0.0f;
    if (a.tgrid) {
      const float iy = clip_coord(unnormalize(a.tgrid[n * T + t], T), T);
      const float y0f = floorf(iy);
      y0 = (int)y0f;
      w1 = iy - y0f;
      w0 = ((float)y0 + 1.0f) - ((float)y0 + w1);  // as the forward kernel
      if (y0 + 1 >= T) w1 = 0.0f;                  // tap outside the image
      if (t > 0) {
        const float ip = clip_coord(unnormalize(a.tgrid[n * T + t - 1], T), T);
        bad = bad || ((int)floorf(ip) > y0);
      }
    }
    sy0[t] = y0;
    sw0[t] = masked ? 0.0f : w0;
    sw1[t] = masked ? 0.0f : w1;
  }
  for (int c = tid; c < F4; c += 256) {
    unsigned keep = 0u;
    for (int j = 0; j < 4; ++j) {
      const int f = 4 * c + j;
      bool fm = false;
      for (int m = 0; m < a.MF; ++m) {
        const int64_t s = a.f0[n * a.MF + m];
        fm = fm || (f >= s && f < s + a.fl[n * a.MF + m]);
      }
      keep |= fm ? 0u : (1u << j);
    }
    col_keep[c] = keep;
  }
  const bool monotone = !__syncthreads_or(bad);
  for (int i = tid; i < kRowsPerTile + 2; i += 256) {
    int lo = 0, hi = T;
    if (monotone) {
      const int target = y_b - 1 + i;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sy0[mid] < target) lo = mid + 1; else hi = mid;
      }
    } else {
      lo = i == 0 ? 0 : T;  // every range becomes [0, T)
    }
    lb[i] = lo;
  }
  __syncthreads();
  const E *gn = grad_out + n * (int64_t)T * a.F;
  E *on = grad_feats + n * (int64_t)T * a.F;
  const float inv = 1.0f / (float)F4;
  const int total = (y_e - y_b) * F4;
  for (int idx = tid; idx < total; idx += 256) {
    int r, f4;
    split_index(idx, inv, F4, r, f4);
    const int y = y_b + r;
    const int t_lo = monotone ? lb[r] : 0, t_hi = monotone ? lb[r + 2] : T;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int t = t_lo; t < t_hi; ++t) {
      const int y0 = sy0[t];
      const float w = y0 == y ? sw0[t] : (y0 + 1 == y ? sw1[t] : 0.0f);
      if (w != 0.0f) {
        const float4 g = load4(gn + (int64_t)t * a.F + 4 * f4);
        acc.x += g.x * w; acc.y += g.y * w; acc.z += g.z * w; acc.w += g.w * w;
      }
    }
    const unsigned keep = col_keep[f4];
    acc.x = (keep & 1u) ? acc.x : 0.0f;
    acc.y = (keep & 2u) ? acc.y : 0.0f;
    acc.z = (keep & 4u) ? acc.z : 0.0f;
    acc.w = (keep & 8u) ? acc.w : 0.0f;
    store4(on + (int64_t)y * a.F + 4 * f4, acc);
  }
}

// The half scatter's last step: the float32 sums of the workspace, each rounded once into grad_feats.
template <typename E>
__global__ void __launch_bounds__(256) round_rows_kernel(const float *__restrict__ ws, E *__restrict__ grad_feats,
                                                         int64_t total) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) elem_store(grad_feats + i, ws[i]);
}


// spec_augment_draw_parameters (_img.py:1056-1139) from ONE tensor of uniform draws: the reference
// makes six torch.rand calls and ~30 tiny tensor ops around them (clamp, floor, masked_fill, long) --
// launch-bound, 0.2-0.5 ms at N = 2048 against the 0.25 ms of the kernel that applies the parameters.
// Here column c of u (N, R) is the c-th draw of utterance n, in the reference's order (w_0, w, v_0, v,
// then the time masks' t, t_0, the frequency masks' f, f_0), and every expression is the reference's
// float32 expression.  (Bitwise parity of the DRAWS with the reference is no goal -- different
// generators per device, SURVEY A.12 -- the mapping from a uniform to a parameter is.)
struct SpecDrawArgs {
  const float *u;
  int R;
  const int64_t *lengths;  // (N,) or null (all T)
  int N, T, F, MT, MF;
  int time_warp, freq_warp, time_mask, freq_mask;  // which groups are drawn
  float max_time_warp, Vf, max_time_mask, max_time_mask_proportion, num_time_mask, num_time_mask_proportion;
  float maxf, eps, omeps;
  float *w_0, *w, *v_0, *v;
  int64_t *t_0, *t, *f_0, *f;
};

__global__ void __launch_bounds__(256) spec_augment_draw_kernel(const SpecDrawArgs a) {
  const int n = (int)(blockIdx.x * 256 + threadIdx.x);
  if (n >= a.N) return;
  const float *u = a.u + (int64_t)n * a.R;
  const float len = a.lengths ? (float)a.lengths[n] : (float)a.T;
  int c = 0;
  if (a.time_warp) {  // :1082-1090
    const float Wt = fminf(fmaxf(len / 2.0f - a.eps, 0.0f), a.max_time_warp);
    a.w_0[n] = u[c] * (len - 2.0f * Wt) + Wt;
    a.w[n] = u[c + 1] * (2.0f * Wt) - Wt;
    c += 2;
  }
  if (a.freq_warp) {  // :1091-1098
    a.v_0[n] = u[c] * ((float)a.F - 2.0f * a.Vf) + a.Vf;
    a.v[n] = u[c + 1] * (2.0f * a.Vf) - a.Vf;
    c += 2;
  }
  if (a.time_mask) {  // :1099-1126
    const float max_ = floorf(fminf(len * a.max_time_mask_proportion, a.max_time_mask));
    const float nums_ = floorf(fminf(len * a.num_time_mask_proportion, a.num_time_mask));
    for (int m = 0; m < a.MT; ++m) {
      int64_t t = (int64_t)(u[c + m] * (max_ + a.omeps));
      if (nums_ <= (float)m) t = 0;
      a.t[(int64_t)n * a.MT + m] = t;
      a.t_0[(int64_t)n * a.MT + m] = (int64_t)(u[c + a.MT + m] * ((len - (float)t) + a.omeps));
    }
    c += 2 * a.MT;
  }
  if (a.freq_mask) {  // :1127-1137
    for (int m = 0; m < a.MF; ++m) {
      const int64_t f = (int64_t)(u[c + m] * (a.maxf + a.omeps));
      a.f[(int64_t)n * a.MF + m] = f;
      a.f_0[(int64_t)n * a.MF + m] = (int64_t)(u[c + a.MF + m] * (((float)a.F - (float)f) + a.omeps));
    }
  }
}

}  // namespace pdt

extern "C" {

int pdt_spec_augment_draw(const float *u, int64_t N, int64_t R, const int64_t *lengths, int64_t T,
                          int64_t F, float max_time_warp, float max_freq_warp, int64_t max_time_mask,
                          int64_t max_freq_mask, float max_time_mask_proportion, int64_t num_time_mask,
                          float num_time_mask_proportion, int64_t num_freq_mask, int is_double,
                          float *w_0, float *w, float *v_0, float *v, int64_t *t_0, int64_t *t,
                          int64_t *f_0, int64_t *f, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0 || F < 0 || R < 0 || num_time_mask < 0 || num_freq_mask < 0) return PDT_E_ARG;
  SpecDrawArgs a{};
  a.time_warp = max_time_warp != 0.0f;
  a.freq_warp = max_freq_warp != 0.0f;
  a.time_mask = max_time_mask != 0 && max_time_mask_proportion != 0.0f && num_time_mask != 0 &&
                num_time_mask_proportion != 0.0f;
  a.freq_mask = max_freq_mask != 0 && num_freq_mask != 0;
  a.MT = a.time_mask ? (int)num_time_mask : 0;
  a.MF = a.freq_mask ? (int)num_freq_mask : 0;
  if (R < 2 * a.time_warp + 2 * a.freq_warp + 2 * a.MT + 2 * a.MF) return PDT_E_ARG;
  if (N == 0 || (!a.time_warp && !a.freq_warp && !a.time_mask && !a.freq_mask)) return PDT_OK;  // nothing to draw
  if (!u || (a.time_warp && (!w_0 || !w)) || (a.freq_warp && (!v_0 || !v)) || (a.time_mask && (!t_0 || !t)) ||
      (a.freq_mask && (!f_0 || !f)))
    return PDT_E_ARG;
  // (the reference's eps is that of the features' dtype; its arithmetic on the draws is float32 either way)
  const double eps = is_double ? 2.220446049250313e-16 : 1.1920928955078125e-07;
  a.u = u; a.R = (int)R; a.lengths = lengths;
  a.N = (int)N; a.T = (int)T; a.F = (int)F;
  a.eps = (float)eps;
  a.omeps = (float)(1.0 - eps);
  a.max_time_warp = max_time_warp;
  a.Vf = (float)std::fmin(std::fmax((double)F / 2.0 - eps, 0.0), (double)max_freq_warp);
  a.max_time_mask = (float)max_time_mask;
  a.max_time_mask_proportion = max_time_mask_proportion;
  a.num_time_mask = (float)num_time_mask;
  a.num_time_mask_proportion = num_time_mask_proportion;
  a.maxf = (float)std::min<int64_t>(max_freq_mask, F);
  a.w_0 = w_0; a.w = w; a.v_0 = v_0; a.v = v; a.t_0 = t_0; a.t = t; a.f_0 = f_0; a.f = f;
  hipLaunchKernelGGL(spec_augment_draw_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

extern "C++" {
// What the three application entry points check alike, in their order, and the fields they all fill.
// `need`: the entry point's own pointers that must not be null.  False: return *rc (PDT_OK: nothing to do).
template <typename E>
static bool spec_aug_args(pdt::SpecAugArgsT<E> &a, int *rc, std::initializer_list<const void *> need, int64_t N,
                          int64_t T, int64_t F, const int64_t *t_0, const int64_t *t_len, int64_t MT,
                          const int64_t *f_0, const int64_t *f_len, int64_t MF) {
  *rc = PDT_E_ARG;
  if (N < 0 || T < 0 || F < 0 || MT < 0 || MF < 0) return false;
  *rc = PDT_OK;
  if (N == 0 || T == 0 || F == 0) return false;
  *rc = PDT_E_ARG;
  for (const void *p : need)
    if (!p) return false;
  if ((MT > 0 && (!t_0 || !t_len)) || (MF > 0 && (!f_0 || !f_len))) return false;
  *rc = PDT_E_TOO_LONG;
  if (T * F >= (1ll << 31) || N > 0x7fffffffll || MT > 0x7fffffffll || MF > 0x7fffffffll) return false;  // ints below
  a.t0 = t_0; a.tl = t_len; a.f0 = f_0; a.fl = f_len;
  a.N = (int)N; a.T = (int)T; a.F = (int)F; a.MT = (int)MT; a.MF = (int)MF;
  *rc = PDT_OK;
  return true;
}

// The rows kernels move four elements along F as one access (16 bytes of float32, 8 of a half type): F a
// multiple of 4 (at most 256: col_keep has 64 words), unit stride along F, and every row of `in` and `out`
// aligned to those 4 * esz bytes.  The callers differ in what they know: the forward entries pass the
// strides of a view; the adjoint's tensors are contiguous, (T * F, F, 1), which F % 4 == 0 already aligns,
// and it adds its own LDS bound (three words per frame).  A frequency grid rules the rows kernels out.
static bool rows_layout_ok(size_t esz, int64_t F, int64_t f_sn, int64_t f_st, int64_t f_sf, uint64_t in, uint64_t out) {
  return (F % 4 == 0) && F <= 256 && f_sf == 1 && (f_st % 4 == 0) && (f_sn % 4 == 0) && (in % (4 * esz) == 0) &&
         (out % (4 * esz) == 0);
}
static size_t rows_backward_smem(int64_t T) { return (size_t)T * 12 + 260 * 4 + 64 * 4; }
static unsigned rows_tiles(int64_t T) { return (unsigned)((T + pdt::kRowsPerTile - 1) / pdt::kRowsPerTile); }
// ~16K elements per workgroup keeps >= 8 workgroups per CU in flight at N = 2048
static unsigned elem_tiles(int64_t T, int64_t F) { return (unsigned)std::max<int64_t>((T * F + 16383) / 16384, 1); }
}  // extern "C++"

int pdt_spec_augment_apply_form(int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st, int64_t f_sf,
                                uint64_t in_addr, uint64_t out_addr, int has_time_grid, int has_freq_grid,
                                int backward, int elem) {
  (void)has_time_grid;  // (a time grid is served by either form)
  const int es = pdt::elem_status(elem);
  if (es != PDT_OK) return es;
  if (N < 0 || T < 0 || F < 0) return PDT_E_ARG;
  if (T * F >= (1ll << 31) || N > 0x7fffffffll) return PDT_E_TOO_LONG;
  const size_t esz = elem == 0 ? 4 : 2;
  if (has_freq_grid) return 0;
  if (backward) return rows_layout_ok(esz, F, T * F, F, 1, in_addr, out_addr) && rows_backward_smem(T) <= 64 * 1024;
  return rows_layout_ok(esz, F, f_sn, f_st, f_sf, in_addr, out_addr);
}

int64_t pdt_spec_augment_backward_workspace_bytes(int64_t N, int64_t T, int64_t F, int has_grid, int elem) {
  if (pdt::elem_status(elem) != PDT_OK || N < 0 || T < 0 || F < 0) return -1;
  if (elem == 0 || has_grid == 0) return 0;  // float32 accumulates in grad_feats; no grid: one writer per element
  if (!(has_grid & 2) && pdt_spec_augment_apply_form(N, T, F, T * F, F, 1, 0, 0, 1, 0, 1, elem) == 1) return 0;
  return 4 * N * T * F;
}

extern "C++" {
template <typename E>
static int apply_impl(int elem, const E *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st,
                      int64_t f_sf, const float *time_grid, const float *freq_grid, const int64_t *t_0,
                      const int64_t *t_len, int64_t MT, const int64_t *f_0, const int64_t *f_len, int64_t MF, E *out,
                      void *stream) {
  using namespace pdt;
  SpecAugArgsT<E> a{};
  int rc;
  if (!spec_aug_args(a, &rc, {feats, out}, N, T, F, t_0, t_len, MT, f_0, f_len, MF)) return rc;
  a.feats = feats; a.f_sn = f_sn; a.f_st = f_st; a.f_sf = f_sf; a.out = out;
  a.tgrid = time_grid; a.fgrid = freq_grid;
  const int form = pdt_spec_augment_apply_form(N, T, F, f_sn, f_st, f_sf, (uint64_t)(uintptr_t)feats,
                                               (uint64_t)(uintptr_t)out, time_grid != nullptr,
                                               freq_grid != nullptr, 0, elem);
  if (form < 0) return form;
  if (form == 1) {
    const unsigned rtiles = rows_tiles(T);
    hipLaunchKernelGGL(spec_augment_rows_kernel<E>, dim3((unsigned)N * rtiles), dim3(256), 0, (hipStream_t)stream, a,
                       (int)rtiles);
  } else {
    const unsigned tiles = elem_tiles(T, F);
    hipLaunchKernelGGL(spec_augment_apply_kernel<E>, dim3((unsigned)N * tiles), dim3(256), 0, (hipStream_t)stream, a,
                       (int)tiles);
  }
  return (int)hipGetLastError();
}

template <typename E>
static int apply_warp_impl(int elem, const E *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st,
                           int64_t f_sf, const float *warp_src, const float *warp_flow, const int64_t *lengths,
                           int order, const int64_t *t_0, const int64_t *t_len, int64_t MT, const int64_t *f_0,
                           const int64_t *f_len, int64_t MF, E *out, int32_t *bad_lengths, void *stream) {
  using namespace pdt;
  if (order < 1) return PDT_E_ARG;
  SpecAugArgsT<E> a{};
  int rc;
  if (!spec_aug_args(a, &rc, {feats, out, warp_src, warp_flow}, N, T, F, t_0, t_len, MT, f_0, f_len, MF)) return rc;
  const int form = pdt_spec_augment_apply_form(N, T, F, f_sn, f_st, f_sf, (uint64_t)(uintptr_t)feats,
                                               (uint64_t)(uintptr_t)out, 0, 0, 0, elem);
  if (form < 0) return form;
  if (form != 1) return PDT_E_UNSUPPORTED;
  a.feats = feats; a.f_sn = f_sn; a.f_st = f_st; a.f_sf = f_sf; a.out = out;
  a.tw_src = warp_src; a.tw_flow = warp_flow; a.tw_len = lengths; a.tw_order = order;
  a.bad_lengths = lengths ? bad_lengths : nullptr;
  const unsigned rtiles = rows_tiles(T);
  hipLaunchKernelGGL(spec_augment_rows_kernel<E>, dim3((unsigned)N * rtiles), dim3(256), 0, (hipStream_t)stream, a,
                     (int)rtiles);
  return (int)hipGetLastError();
}

// `workspace`: N * T * F floats for a half E on the scatter route with a grid (zeroed here); unused otherwise.
template <typename E>
static int apply_backward_impl(int elem, const E *grad_out, int64_t N, int64_t T, int64_t F, const float *time_grid,
                               const float *freq_grid, const int64_t *t_0, const int64_t *t_len, int64_t MT,
                               const int64_t *f_0, const int64_t *f_len, int64_t MF, E *grad_feats, void *workspace,
                               int64_t workspace_bytes, void *stream) {
  using namespace pdt;
  SpecAugArgsT<E> a{};
  int rc;
  if (!spec_aug_args(a, &rc, {grad_out, grad_feats}, N, T, F, t_0, t_len, MT, f_0, f_len, MF)) return rc;
  a.tgrid = time_grid; a.fgrid = freq_grid;
  const int form = pdt_spec_augment_apply_form(N, T, F, T * F, F, 1, (uint64_t)(uintptr_t)grad_out,
                                               (uint64_t)(uintptr_t)grad_feats, time_grid != nullptr,
                                               freq_grid != nullptr, 1, elem);
  if (form < 0) return form;
  if (form == 1) {
    const unsigned rtiles = rows_tiles(T);
    hipLaunchKernelGGL(spec_augment_rows_backward_kernel<E>, dim3((unsigned)N * rtiles), dim3(256),
                       rows_backward_smem(T), (hipStream_t)stream, a, grad_out, grad_feats, (int)rtiles);
    return (int)hipGetLastError();
  }
  const int64_t total = N * T * F;
  const bool sums = sizeof(E) != sizeof(float) && (time_grid || freq_grid);  // float32 sums, rounded afterwards
  if (sums && (!workspace || workspace_bytes < total * (int64_t)sizeof(float))) return PDT_E_ARG;
  float *acc = sums ? (float *)workspace : reinterpret_cast<float *>(grad_feats);
  hipError_t e = hipMemsetAsync(acc, 0, (size_t)total * (sums ? sizeof(float) : sizeof(E)), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const unsigned tiles = elem_tiles(T, F);
  hipLaunchKernelGGL(spec_augment_backward_kernel<E>, dim3((unsigned)N * tiles), dim3(256), 0, (hipStream_t)stream, a,
                     grad_out, acc, (int)tiles);
  if constexpr (sizeof(E) != sizeof(float)) {
    if (sums) {
      const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 16);
      hipLaunchKernelGGL(round_rows_kernel<E>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                         (const float *)workspace, grad_feats, total);
    }
  }
  return (int)hipGetLastError();
}
}  // extern "C++"

int pdt_spec_augment_apply(const float *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn,
                           int64_t f_st, int64_t f_sf, const float *time_grid,
                           const float *freq_grid, const int64_t *t_0, const int64_t *t_len,
                           int64_t MT, const int64_t *f_0, const int64_t *f_len, int64_t MF,
                           float *out, void *stream) {
  return apply_impl<float>(0, feats, N, T, F, f_sn, f_st, f_sf, time_grid, freq_grid, t_0, t_len, MT, f_0, f_len, MF,
                           out, stream);
}

int pdt_spec_augment_apply_warp(const float *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn,
                                int64_t f_st, int64_t f_sf, const float *warp_src, const float *warp_flow,
                                const int64_t *lengths, int order, const int64_t *t_0,
                                const int64_t *t_len, int64_t MT, const int64_t *f_0,
                                const int64_t *f_len, int64_t MF, float *out, int32_t *bad_lengths,
                                void *stream) {
  return apply_warp_impl<float>(0, feats, N, T, F, f_sn, f_st, f_sf, warp_src, warp_flow, lengths, order, t_0, t_len,
                                MT, f_0, f_len, MF, out, bad_lengths, stream);
}

int pdt_spec_augment_apply_backward(const float *grad_out, int64_t N, int64_t T, int64_t F,
                                    const float *time_grid, const float *freq_grid,
                                    const int64_t *t_0, const int64_t *t_len, int64_t MT,
                                    const int64_t *f_0, const int64_t *f_len, int64_t MF,
                                    float *grad_feats, void *stream) {
  return apply_backward_impl<float>(0, grad_out, N, T, F, time_grid, freq_grid, t_0, t_len, MT, f_0, f_len, MF,
                                    grad_feats, nullptr, 0, stream);
}

// The same three on features of element type `elem` (0 float32: the launch above; 2 float16; 3 bfloat16).
// The element code is judged first; CALL names the element type as E.
#define PDT_SPEC_ELEM(CALL)                                \
  {                                                        \
    const int es_ = pdt::elem_status(elem);                \
    if (es_ != PDT_OK) return es_;                         \
  }                                                        \
  if (elem == 2) { using E = pdt::f16_t; return CALL; }    \
  if (elem == 3) { using E = pdt::bf16_t; return CALL; }   \
  { using E = float; return CALL; }

int pdt_spec_augment_apply_elem(const void *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st,
                                int64_t f_sf, const float *time_grid, const float *freq_grid, const int64_t *t_0,
                                const int64_t *t_len, int64_t MT, const int64_t *f_0, const int64_t *f_len,
                                int64_t MF, void *out, void *stream, int elem) {
  PDT_SPEC_ELEM((apply_impl<E>(elem, (const E *)feats, N, T, F, f_sn, f_st, f_sf, time_grid, freq_grid, t_0, t_len, MT,
                               f_0, f_len, MF, (E *)out, stream)))
}

int pdt_spec_augment_apply_warp_elem(const void *feats, int64_t N, int64_t T, int64_t F, int64_t f_sn, int64_t f_st,
                                     int64_t f_sf, const float *warp_src, const float *warp_flow,
                                     const int64_t *lengths, int order, const int64_t *t_0, const int64_t *t_len,
                                     int64_t MT, const int64_t *f_0, const int64_t *f_len, int64_t MF, void *out,
                                     int32_t *bad_lengths, void *stream, int elem) {
  PDT_SPEC_ELEM((apply_warp_impl<E>(elem, (const E *)feats, N, T, F, f_sn, f_st, f_sf, warp_src, warp_flow, lengths,
                                    order, t_0, t_len, MT, f_0, f_len, MF, (E *)out, bad_lengths, stream)))
}

int pdt_spec_augment_apply_backward_elem(const void *grad_out, int64_t N, int64_t T, int64_t F, const float *time_grid,
                                         const float *freq_grid, const int64_t *t_0, const int64_t *t_len, int64_t MT,
                                         const int64_t *f_0, const int64_t *f_len, int64_t MF, void *grad_feats,
                                         void *stream, int elem, void *workspace, int64_t workspace_bytes) {
  PDT_SPEC_ELEM((apply_backward_impl<E>(elem, (const E *)grad_out, N, T, F, time_grid, freq_grid, t_0, t_len, MT, f_0,
                                        f_len, MF, (E *)grad_feats, workspace, workspace_bytes, stream)))
}
#undef PDT_SPEC_ELEM

}  // extern "C"

