// Dense and sparse image warps for gfx950.
//
// Replaces, from the reference's _img.py:
//   dense_image_warp (:393-439), sparse_image_warp (:520-714) -> image_warp_kernel: per pixel,
//       sampling position from a flow field or straight from the spline (knots in LDS), then the
//       grid_sample gather (bilinear / nearest; zeros / border / reflection) for every channel;
//       sparse_warp_bands_kernel for the sparse warp's common shape.
// The spline's system is solved by spline.hip (pdt::spline_solve); gathers follow
// torch.nn.functional.grid_sample(align_corners=False) arithmetic in the image's type.
#include <type_traits>

#include "img_launch.hpp"
#include "img_sample.hpp"

namespace pdt {

// PT: the pixel type (float; double for float64 images -- image_warp_kernel only, see there)
template <typename PT>
struct WarpArgsT {
  const PT *image;     // (N,C,H,W) contiguous
  PT *out;             // (N,C,H,W)
  int N, C, H, W;
  int mode, padding;
  // source of the sampling position, one of:
  const float *flow;   // dense: (N,H,W,2); position = pixel - flow (x = last dim 0 unless flip)
  int flip;            // dense: flow[..., 0] is the H component ("hw" indexing)
  const float *knots;  // sparse: (N,M,2) spline centres (x, y), float
  const float *wv;     // sparse: (N, M+3, 2) float weights (w, then v_x, v_y, v_1)
  int M, order, as_grid;  // as_grid: the spline yields the normalised grid itself (no-flow form)
  float inv_w;         // 1 / W (sparse_warp_bands_kernel)
  float *flow_out;     // sparse, optional (N,H,W,2)
  int flow_out_flip;
  PT *grad_image;      // BACKWARD: (N,C,H,W), zeroed by the caller; `out` then holds grad_out
  float *grad_pos;     // WARP_POSITION: (N,H,W,2), dL/d(flow) or dL/d(spline value); `out` holds grad_out
  const float *grad_flow_in;  // WARP_POSITION, sparse, optional: (N,H,W,2) added (flow_out_flip: its order)
};
using WarpArgs = WarpArgsT<float>;

// BACKWARD = adjoint with respect to the image: the same sampling positions, each pixel scatters
// its gradient to its taps with the hardware float atomic.
// PT = double: a float64 image.  The reference keeps flows and spline points in float32 whatever
// the image's type (_img.py:420, :537-538) but forms the sampling grid and samples it in the
// image's type (:423-436), so here the flow / spline value stays float and everything from the grid
// on (un-normalisation, padding, weights, blend, the adjoint's atomics) is double.
//
// WARP_POSITION = gradient with respect to WHERE a pixel samples: per pixel dL/d(ix, iy) = sum over the
// channels of grad_out x the derivative of the bilinear blend (the four taps under the forward's validity
// tests), chained through the padding rule (img_sample.hpp: clip_coord_factor / reflect_coord_factor,
// torch's *_set_grad), the un-normalisation (size / 2) and the grid formula (-2 / size for a flow: -1
// together; the no-flow spline form keeps size / 2).  Each pixel writes its own two numbers: no atomics.
// Dense: the flow's gradient in the flow's own order (flip).  Sparse: the gradient with respect to the
// spline's value at the pixel in (x, y) order -- what pdt_spline_eval_adjoint reduces -- plus the caller's
// gradient of the returned flow (grad_flow_in, in flow_out_flip's order).
constexpr int kPixPerWG = 2048;
enum { WARP_FORWARD = 0, WARP_ADJOINT = 1, WARP_POSITION = 2 };
template <int FORM, typename PT = float>
__global__ void __launch_bounds__(256) image_warp_kernel(const WarpArgsT<PT> a) {
  using CT = PT;  // coordinate type
  constexpr bool BACKWARD = FORM == WARP_ADJOINT;
  constexpr bool POSITION = FORM == WARP_POSITION;
  extern __shared__ __align__(16) unsigned char smem[];
  float *lk = reinterpret_cast<float *>(smem);  // knots (M,2) then weights (M+3,2)
  float *lw = lk + 2 * a.M;
  const int64_t n = blockIdx.y;
  const int H = a.H, W = a.W;
  if (a.knots) {
    for (int i = (int)threadIdx.x; i < 2 * a.M; i += 256) lk[i] = a.knots[n * 2 * a.M + i];
    for (int i = (int)threadIdx.x; i < 2 * (a.M + 3); i += 256) lw[i] = a.wv[n * 2 * (a.M + 3) + i];
    __syncthreads();
  }
  const float inv_w = 1.0f / (float)W, inv_h = 1.0f / (float)H;  // wave-uniform: two divisions per wave
  // a workgroup covers kPixPerWG pixels: the LDS staging + barrier above is paid once per
  // 2048 pixels instead of once per 256 (it dominated at one pixel per thread)
  for (int pix = (int)(blockIdx.x * kPixPerWG + threadIdx.x);
       pix < min(H * W, (int)((blockIdx.x + 1) * kPixPerWG)); pix += 256) {
    // (h, w) of the pixel without an integer division where a float holds pix exactly
    int h, w;
    if (H * W < (1 << 23)) {
      split_index(pix, inv_w, W, h, w);
    } else {
      h = pix / W;
      w = pix - h * W;
    }
    CT gx, gy;
    const CT inv_wc = std::is_same<CT, float>::value ? (CT)inv_w : CT(1) / (CT)W;
    const CT inv_hc = std::is_same<CT, float>::value ? (CT)inv_h : CT(1) / (CT)H;
    if (a.knots) {
      const float x = (float)w, y = (float)h;
      float sx = lw[2 * a.M + 0] * x + lw[2 * (a.M + 1) + 0] * y + lw[2 * (a.M + 2) + 0];
      float sy = lw[2 * a.M + 1] * x + lw[2 * (a.M + 1) + 1] * y + lw[2 * (a.M + 2) + 1];
      // the order is wave-uniform: pick the specialised loop once, outside the centre loop
      auto centres = [&](auto tag) {
        constexpr int ORDER = decltype(tag)::value;
#pragma unroll 4
        for (int m = 0; m < a.M; ++m) {
          const float dx = x - lk[2 * m], dy = y - lk[2 * m + 1];
          const float p = phi_from_d2<ORDER>(dx * dx + dy * dy, a.order);
          sx += p * lw[2 * m];
          sy += p * lw[2 * m + 1];
        }
      };
      if (a.order == 2) centres(std::integral_constant<int, 2>{});
      else if (a.order == 1) centres(std::integral_constant<int, 1>{});
      else if (a.order == 3) centres(std::integral_constant<int, 3>{});
      else centres(std::integral_constant<int, 0>{});
      if (a.as_grid) {
        gx = sx;
        gy = sy;
      } else {
        if (FORM == WARP_FORWARD && a.flow_out) {
          float *fo = a.flow_out + ((n * H + h) * (int64_t)W + w) * 2;
          fo[0] = a.flow_out_flip ? sy : sx;
          fo[1] = a.flow_out_flip ? sx : sy;
        }
        gx = (CT(2) * (CT)x - CT(2) * (CT)sx + CT(1)) * inv_wc - CT(1);  // _img.py:432
        gy = (CT(2) * (CT)y - CT(2) * (CT)sy + CT(1)) * inv_hc - CT(1);
      }
    } else {
      const float *fl = a.flow + ((n * H + h) * (int64_t)W + w) * 2;
      const float fx = a.flip ? fl[1] : fl[0], fy = a.flip ? fl[0] : fl[1];
      gx = (CT(2) * (CT)w - CT(2) * (CT)fx + CT(1)) * inv_wc - CT(1);
      gy = (CT(2) * (CT)h - CT(2) * (CT)fy + CT(1)) * inv_hc - CT(1);
    }
    const CT ix = source_index<CT>(gx, W, a.padding), iy = source_index<CT>(gy, H, a.padding);
    const int64_t plane = (int64_t)H * W;
    const PT *img = a.image + n * a.C * plane;
    PT *o = a.out + n * a.C * plane + pix;
    PT *gi = a.grad_image + n * a.C * plane;
    if (POSITION) {
      // (sx, sy): dL/d(the x and y component of the flow or of the spline's value) at this pixel
      CT sx = CT(0), sy = CT(0);
      if (a.mode == INTERP_BILINEAR) {  // (nearest: piecewise constant in the position)
        const CT x0f = floor(ix), y0f = floor(iy);
        const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
        const CT wx1 = ix - x0f, wy1 = iy - y0f, wx0 = (x0f + CT(1)) - ix, wy0 = (y0f + CT(1)) - iy;
        const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W;
        const bool vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
        CT dix = CT(0), diy = CT(0);
        for (int c = 0; c < a.C; ++c) {
          const PT *pl = img + c * plane;
          const PT g = o[c * plane];
          if (vx0 && vy0) { const PT t = pl[(int64_t)y0 * W + x0] * g; dix -= t * wy0; diy -= t * wx0; }
          if (vx1 && vy0) { const PT t = pl[(int64_t)y0 * W + x1] * g; dix += t * wy0; diy -= t * wx1; }
          if (vx0 && vy1) { const PT t = pl[(int64_t)y1 * W + x0] * g; dix -= t * wy1; diy += t * wx0; }
          if (vx1 && vy1) { const PT t = pl[(int64_t)y1 * W + x1] * g; dix += t * wy1; diy += t * wx1; }
        }
        // padding rule, then un-normalisation x grid formula: size / 2 x -2 / size = -1 for a flow
        const CT fx = source_index_factor<CT>(gx, W, a.padding), fy = source_index_factor<CT>(gy, H, a.padding);
        const bool grid = a.knots && a.as_grid;
        sx = dix * fx * (grid ? CT(0.5) * (CT)W : CT(-1));
        sy = diy * fy * (grid ? CT(0.5) * (CT)H : CT(-1));
      }
      const int64_t at = ((n * H + h) * (int64_t)W + w) * 2;
      float r0 = (float)sx, r1 = (float)sy;
      if (a.knots) {
        if (a.grad_flow_in) {
          r0 += a.grad_flow_in[at + (a.flow_out_flip ? 1 : 0)];
          r1 += a.grad_flow_in[at + (a.flow_out_flip ? 0 : 1)];
        }
      } else if (a.flip) {
        const float t = r0;
        r0 = r1;
        r1 = t;
      }
      a.grad_pos[at] = r0;
      a.grad_pos[at + 1] = r1;
      continue;
    }
    if (a.mode == INTERP_NEAREST) {
      const int xn = (int)nearbyint(ix), yn = (int)nearbyint(iy);
      const bool ok = xn >= 0 && xn < W && yn >= 0 && yn < H;
      if (BACKWARD) {
        if (ok)
          for (int c = 0; c < a.C; ++c) unsafeAtomicAdd(gi + c * plane + (int64_t)yn * W + xn, o[c * plane]);
        continue;
      }
      for (int c = 0; c < a.C; ++c) o[c * plane] = ok ? img[c * plane + (int64_t)yn * W + xn] : PT(0);
      continue;
    }
    const CT x0f = floor(ix), y0f = floor(iy);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    const CT wx1 = ix - x0f, wy1 = iy - y0f, wx0 = (x0f + CT(1)) - ix, wy0 = (y0f + CT(1)) - iy;
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W;
    const bool vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
    if (BACKWARD) {
      for (int c = 0; c < a.C; ++c) {
        PT *pl = gi + c * plane;
        const PT g = o[c * plane];
        if (vx0 && vy0) unsafeAtomicAdd(pl + (int64_t)y0 * W + x0, g * (wx0 * wy0));
        if (vx1 && vy0) unsafeAtomicAdd(pl + (int64_t)y0 * W + x1, g * (wx1 * wy0));
        if (vx0 && vy1) unsafeAtomicAdd(pl + (int64_t)y1 * W + x0, g * (wx0 * wy1));
        if (vx1 && vy1) unsafeAtomicAdd(pl + (int64_t)y1 * W + x1, g * (wx1 * wy1));
      }
      continue;
    }
    for (int c = 0; c < a.C; ++c) {
      const PT *pl = img + c * plane;
      PT v = PT(0);
      if (vx0 && vy0) v += pl[(int64_t)y0 * W + x0] * (wx0 * wy0);
      if (vx1 && vy0) v += pl[(int64_t)y0 * W + x1] * (wx1 * wy0);
      if (vx0 && vy1) v += pl[(int64_t)y1 * W + x0] * (wx0 * wy1);
      if (vx1 && vy1) v += pl[(int64_t)y1 * W + x1] * (wx1 * wy1);
      o[c * plane] = v;
    }
}
}

// Sparse warp, the common shape (bilinear, forward, no flow output, at most kWarpFastM spline
// centres -- SpecAugment-style calls have 3 + 4 pinned): image_warp_kernel's per-pixel work, the
// spline sum in fused multiply-adds (one rounding per term instead of two; the results differ from
// image_warp_kernel's in the last bits, far inside the 1e-4 the spline is good to), with a lane = one
// COLUMN of a band of ROWS rows: the pixels (h .. h + ROWS - 1, w) share x, so a centre's dx, dx^2 and the x part of the affine term are formed once per lane, the
// pixel -> (h, w) split once, and the chains are written as float2 chains (v_pk_add / v_pk_mul /
// v_pk_fma carry two pixels per instruction; v_log_f32 stays scalar).  A wave's lanes are consecutive
// columns (bands flattened with their columns: lane order = memory order within a row), so each
// row-round of taps and stores is coalesced.
//
// What the lanes do NOT do: everything that is the same for a whole image sits in a TABLE that
// warp_table_kernel writes once per call (per image: MC centres x (kx, ky, wx, wy), then ax, ay, bx,
// by, cx, cy) and the kernel reads with scalar loads -- no LDS staging, no barrier, no readfirstlane.
// The table's weights carry (a) grid_sample's un-normalisation ((g + 1) * size - 1) / 2 -- or, in
// the flow form, pixel - flow -- so the spline's value IS the source pixel coordinate, (b) order 2's
// ln 2 / 2, so phi is d2 * log2(d2) here; both products are formed in double before the cast.
// Centres beyond M have zero weights: fma(phi, 0, s) = s exactly, phi finite everywhere.
//
// Taps (border / reflection padding, coordinates inside [0, size - 1]): buffer loads with the plane's
// base in scalar registers and 32-bit byte offsets; the first tap's offset is one float fma + convert
// (exact below 2^23 pixels), the others add 4 / 4W -- or, where the neighbour lies outside the image,
// an offset beyond the buffer: the load returns 0 and the tap drops out as in image_warp_kernel
// (never a product of an inf / NaN pixel with a zero weight).
typedef float wf2 __attribute__((ext_vector_type(2)));
constexpr int kWarpFastM = 8;
constexpr int kBandRows = 4;  // (8 measured slower: 0.42 ms against 0.40 at C4)

__global__ void warp_table_kernel(const double *__restrict__ wv, const float *__restrict__ knots, float *__restrict__ tab,
                                  int64_t N, int M, int MC, int as_grid, int H, int W, int order) {
  const int stride = warp_table_stride(MC);
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N * stride) return;
  const int64_t n = i / stride;
  const int e = (int)(i - n * stride);
  const double *sol = wv + n * (int64_t)(M + 3) * 2;
  const int d = e & 1;                                     // 0: x (columns), 1: y (rows)
  const double size = d ? (double)H : (double)W;
  // source coordinate = scale * spline + (identity part) + shift
  const double scale = as_grid ? 0.5 * size : -1.0;
  const double phi_scale = order == 2 ? 0.34657359027997264 : 1.0;
  float v = 0.0f;
  if (e < 4 * MC) {
    const int m = e >> 2, k = e & 3;
    if (m < M) v = k < 2 ? knots[(n * M + m) * 2 + k] : (float)(sol[m * 2 + (k - 2)] * scale * phi_scale);
  } else if (e < 4 * MC + 6) {
    const int r = (e - 4 * MC) >> 1;                       // 0: coefficient of x, 1: of y, 2: constant
    double t = sol[(M + r) * 2 + d] * scale;
    if (as_grid) {
      if (r == 2) t += 0.5 * (size - 1.0);
    } else if (r == d) {
      t += 1.0;
    }
    v = (float)t;
  }
  tab[i] = v;
}

template <int ORDER>
__device__ __forceinline__ wf2 phi2_unscaled(const wf2 d2, const int order) {
  if (ORDER == 2) {  // d2 * log2(d2); d2 + 1e-37 is d2 for every distance but 0, and 0 * log2(1e-37) = 0
    const wf2 t = d2 + wf2{1e-37f, 1e-37f};
    return d2 * wf2{__builtin_amdgcn_logf(t.x), __builtin_amdgcn_logf(t.y)};
  }
  return wf2{phi_from_d2<ORDER>(d2.x, order), phi_from_d2<ORDER>(d2.y, order)};
}

template <int ORDER, int PADDING, int MC, int ROWS>
__global__ void __launch_bounds__(256) sparse_warp_bands_kernel(const WarpArgs a) {
  static_assert(ROWS % 2 == 0, "rows are carried in pairs");
  constexpr int RP = ROWS / 2;
  const int64_t n = blockIdx.y;
  const int H = a.H, W = a.W;
  const float *__restrict__ tab = a.wv + n * warp_table_stride(MC);  // (wave-uniform addresses: scalar loads)
  const int HW = H * W, bands = (H + ROWS - 1) / ROWS;
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
  if (idx >= bands * W) return;
  // (split_index written out: called here, the compiler schedules all 24 instances differently)
  int band = (int)(((float)idx + 0.5f) * a.inv_w), w = idx - band * W;  // (bands * W < 2^23: checked by the launcher)
  if (w < 0) { --band; w += W; }
  if (w >= W) { ++band; w -= W; }
  const int h0 = band * ROWS;
  const float x = (float)w, yb = (float)h0;
  wf2 yv[RP], sx[RP], sy[RP];
  {
    const float *af = tab + 4 * MC;
    const float axc = __builtin_fmaf(af[0], x, af[4]), ayc = __builtin_fmaf(af[1], x, af[5]);
    const wf2 bx = {af[2], af[2]}, by = {af[3], af[3]};
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      yv[i] = wf2{yb + (float)(2 * i), yb + (float)(2 * i + 1)};
      sx[i] = __builtin_elementwise_fma(yv[i], bx, wf2{axc, axc});
      sy[i] = __builtin_elementwise_fma(yv[i], by, wf2{ayc, ayc});
    }
  }
#pragma unroll
  for (int m = 0; m < MC; ++m) {
    const float kx = tab[4 * m], ky = tab[4 * m + 1], wx = tab[4 * m + 2], wy = tab[4 * m + 3];
    const float dx = x - kx, dx2 = dx * dx;
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      const wf2 dy = yv[i] - wf2{ky, ky};
      const wf2 p = phi2_unscaled<ORDER>(__builtin_elementwise_fma(dy, dy, wf2{dx2, dx2}), a.order);
      sx[i] = __builtin_elementwise_fma(p, wf2{wx, wx}, sx[i]);
      sy[i] = __builtin_elementwise_fma(p, wf2{wy, wy}, sy[i]);
    }
  }
  float ix[ROWS], iy[ROWS], x0f[ROWS], y0f[ROWS];
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    float px = (j & 1) ? sx[j >> 1].y : sx[j >> 1].x, py = (j & 1) ? sy[j >> 1].y : sy[j >> 1].x;
    if (PADDING == PAD_REFLECTION) {
      px = reflect_coord(px, -1, 2 * W - 1);
      py = reflect_coord(py, -1, 2 * H - 1);
    }
    if (PADDING != PAD_ZEROS) {  // clip_coord
      px = fminf(wm1, fmaxf(px, 0.0f));
      py = fminf(hm1, fmaxf(py, 0.0f));
    }
    ix[j] = px;
    iy[j] = py;
    x0f[j] = floorf(px);
    y0f[j] = floorf(py);
  }
  const float wf = (float)W;
  for (int c = 0; c < a.C; ++c) {
    const float *pl = a.image + (n * a.C + c) * (int64_t)HW;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pl), 0, HW * 4, 0x00020000);
    unsigned t00[ROWS], t01[ROWS], t10[ROWS], t11[ROWS];  // (the pixels' BITS: the loads return integers)
    if (PADDING == PAD_ZEROS) {
#pragma unroll
      for (int j = 0; j < ROWS; ++j) {  // taps outside the image: any valid address, left out below
        const int x0 = (int)x0f[j], y0 = (int)y0f[j];
        const int xc0 = min(max(x0, 0), W - 1), xc1 = min(max(x0 + 1, 0), W - 1);
        const int yc0 = min(max(y0, 0), H - 1) * W, yc1 = min(max(y0 + 1, 0), H - 1) * W;
        t00[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (yc0 + xc0) << 2, 0, 0);
        t01[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (yc0 + xc1) << 2, 0, 0);
        t10[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (yc1 + xc0) << 2, 0, 0);
        t11[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (yc1 + xc1) << 2, 0, 0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < ROWS; ++j) {  // all the taps in flight
        // (unsigned: with both neighbours outside the two out-of-buffer steps add up to 2^31, which
        //  wraps by definition and is still beyond num_records -- the load returns 0)
        const unsigned o00 = (unsigned)(int)__builtin_fmaf(y0f[j], wf, x0f[j]) << 2;
        const unsigned right = x0f[j] < wm1 ? 4u : 0x40000000u, down = y0f[j] < hm1 ? 4u * (unsigned)W : 0x40000000u;
        const unsigned o10 = o00 + down;
        t00[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)o00, 0, 0);
        t01[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(o00 + right), 0, 0);
        t10[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)o10, 0, 0);
        t11[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(o10 + right), 0, 0);
      }
    }
    float *po = a.out + (n * a.C + c) * (int64_t)HW;
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(po, 0, HW * 4, 0x00020000);
    const int obase = (h0 * W + w) << 2;
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
      const float wx1 = ix[j] - x0f[j], wy1 = iy[j] - y0f[j], wx0 = (x0f[j] + 1.0f) - ix[j], wy0 = (y0f[j] + 1.0f) - iy[j];
      float acc;
      if (PADDING == PAD_ZEROS) {
        const int x0 = (int)x0f[j], y0 = (int)y0f[j], x1 = x0 + 1, y1 = y0 + 1;
        const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
        // (a select, not a product with 0: that would turn an inf / NaN pixel into NaN)
        acc = (vx0 && vy0) ? __uint_as_float(t00[j]) * (wx0 * wy0) : 0.0f;
        acc += (vx1 && vy0) ? __uint_as_float(t01[j]) * (wx1 * wy0) : 0.0f;
        acc += (vx0 && vy1) ? __uint_as_float(t10[j]) * (wx0 * wy1) : 0.0f;
        acc += (vx1 && vy1) ? __uint_as_float(t11[j]) * (wx1 * wy1) : 0.0f;
      } else {
        acc = __uint_as_float(t00[j]) * (wx0 * wy0);
        acc += __uint_as_float(t01[j]) * (wx1 * wy0);
        acc += __uint_as_float(t10[j]) * (wx0 * wy1);
        acc += __uint_as_float(t11[j]) * (wx1 * wy1);
      }
      if (h0 + j < H) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc), ro, obase + j * (4 * W), 0, 0);
    }
  }
}
// copy the double solution into float (w, v) laid out (N, M+3, 2) for image_warp_kernel
__global__ void cast_wv_kernel(const double *__restrict__ wv, float *__restrict__ out, int64_t total) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < total) out[i] = (float)wv[i];
}

}  // namespace pdt

extern "C" {

extern "C++" {
// the fields every warp fills
template <typename PT>
static pdt::WarpArgsT<PT> warp_args(const PT *image, PT *out, int64_t N, int64_t C, int64_t H, int64_t W, int mode,
                                    int padding, PT *grad_image) {
  pdt::WarpArgsT<PT> a{};
  a.image = image; a.out = out; a.N = (int)N; a.C = (int)C; a.H = (int)H; a.W = (int)W;
  a.mode = mode; a.padding = padding;
  a.grad_image = grad_image;
  return a;
}

// image_warp_kernel over kPixPerWG pixels per workgroup: the adjoint (grad_image set: zeroed here, the
// kernel scatters into it), the position gradient (grad_pos set) or the forward gather
template <typename PT>
static int launch_image_warp(const pdt::WarpArgsT<PT> &a, size_t smem, hipStream_t stream) {
  using namespace pdt;
  const int64_t plane = (int64_t)a.H * a.W;
  const dim3 grid((unsigned)((plane + kPixPerWG - 1) / kPixPerWG), (unsigned)a.N);
  if (a.grad_image) {
    hipError_t e = hipMemsetAsync(a.grad_image, 0, (size_t)a.N * a.C * plane * sizeof(PT), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((image_warp_kernel<WARP_ADJOINT, PT>), grid, dim3(256), smem, stream, a);
  } else if (a.grad_pos) {
    hipLaunchKernelGGL((image_warp_kernel<WARP_POSITION, PT>), grid, dim3(256), smem, stream, a);
  } else {
    hipLaunchKernelGGL((image_warp_kernel<WARP_FORWARD, PT>), grid, dim3(256), smem, stream, a);
  }
  return (int)hipGetLastError();
}

template <typename PT>
static int dense_warp_launch(const PT *image, const float *flow, int64_t N, int64_t C, int64_t H,
                             int64_t W, int flow_is_hw, int mode, int padding, PT *out,
                             PT *grad_image, void *stream) {
  using namespace pdt;
  if (N < 0 || C < 0 || H < 0 || W < 0 || mode < 0 || mode > 1 || padding < 0 || padding > 2)
    return PDT_E_ARG;
  if (N == 0 || C == 0 || H == 0 || W == 0) return PDT_OK;
  if ((!image && !grad_image) || !flow || !out) return PDT_E_ARG;
  if (H * W >= (1ll << 31) || N > 65535) return PDT_E_TOO_LONG;
  WarpArgsT<PT> a = warp_args(image, out, N, C, H, W, mode, padding, grad_image);
  a.flow = flow; a.flip = flow_is_hw;
  return launch_image_warp(a, 0, (hipStream_t)stream);
}
}  // extern "C++"

int pdt_dense_image_warp(const float *image, const float *flow, int64_t N, int64_t C, int64_t H,
                         int64_t W, int flow_is_hw, int mode, int padding, float *out,
                         void *stream) {
  return dense_warp_launch<float>(image, flow, N, C, H, W, flow_is_hw, mode, padding, out, nullptr, stream);
}

int pdt_dense_image_warp_backward(const float *grad_out, const float *flow, int64_t N, int64_t C,
                                  int64_t H, int64_t W, int flow_is_hw, int mode, int padding,
                                  float *grad_image, void *stream) {
  if (!grad_image && N && C && H && W) return PDT_E_ARG;
  return dense_warp_launch<float>(nullptr, flow, N, C, H, W, flow_is_hw, mode, padding,
                                  const_cast<float *>(grad_out), grad_image, stream);
}

extern "C++" {
template <typename PT>
static int sparse_warp_launch(const PT *image, const float *train_points,
                              const float *train_values, int64_t N, int64_t C, int64_t H, int64_t W,
                              int64_t M, int order, float regularization_weight, int values_are_grid,
                              int mode, int padding, PT *out, float *flow_out, int flow_out_is_hw,
                              PT *grad_image, void *workspace, void *stream) {
  using namespace pdt;
  if (N < 0 || C < 0 || H < 0 || W < 0 || M < 1 || order < 1 || mode < 0 || mode > 1 ||
      padding < 0 || padding > 2)
    return PDT_E_ARG;
  if (N == 0 || C == 0 || H == 0 || W == 0) return PDT_OK;
  if ((!image && !grad_image) || !train_points || !train_values || !out || !workspace)
    return PDT_E_ARG;
  if (H * W >= (1ll << 31) || N > 65535) return PDT_E_TOO_LONG;
  double *wv = reinterpret_cast<double *>(workspace);
  int rc = spline_solve(train_points, train_values, nullptr, N, M, 2, 2, order, regularization_weight, wv,
                        (hipStream_t)stream);
  if (rc != PDT_OK) return rc;
  const int64_t total = N * (M + 3) * 2;
  float *wvf = reinterpret_cast<float *>(wv + total);
  // (the bands kernel reads its own table, written from the double solution by warp_table_kernel)
  constexpr bool kFloat = std::is_same<PT, float>::value;  // (the fast form is a float32 kernel)
  const bool fast_shape = kFloat && !grad_image && mode == INTERP_BILINEAR && !flow_out && M <= kWarpFastM && H * W < (1 << 23);
  if (!fast_shape)
    hipLaunchKernelGGL(cast_wv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, wv, wvf, total);
  WarpArgsT<PT> a = warp_args(image, out, N, C, H, W, mode, padding, grad_image);
  a.knots = train_points; a.wv = wvf; a.M = (int)M; a.order = order; a.as_grid = values_are_grid;
  a.flow_out = flow_out; a.flow_out_flip = flow_out_is_hw;
  if constexpr (kFloat) {
   if (fast_shape) {  // (never the adjoint)
    // a lane = a column of kBandRows rows, the image's constants from a table (sparse_warp_bands_kernel)
    const int64_t lanes = ((H + kBandRows - 1) / kBandRows) * W;
    const dim3 gf((unsigned)((lanes + 255) / 256), (unsigned)N);
    auto go = [&](auto ord) {
      constexpr int O = decltype(ord)::value;
      auto bands = [&](auto mc) {
        constexpr int MC = decltype(mc)::value;
        float *tab = wvf + total;
        const int64_t entries = N * warp_table_stride(MC);
        hipLaunchKernelGGL(warp_table_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           wv, train_points, tab, N, (int)M, MC, values_are_grid, (int)H, (int)W, order);
        a.wv = tab;
        a.inv_w = 1.0f / (float)W;
        if (padding == PAD_BORDER) hipLaunchKernelGGL((sparse_warp_bands_kernel<O, PAD_BORDER, MC, kBandRows>), gf, dim3(256), 0, (hipStream_t)stream, a);
        else if (padding == PAD_ZEROS) hipLaunchKernelGGL((sparse_warp_bands_kernel<O, PAD_ZEROS, MC, kBandRows>), gf, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((sparse_warp_bands_kernel<O, PAD_REFLECTION, MC, kBandRows>), gf, dim3(256), 0, (hipStream_t)stream, a);
      };
      // (seven centres = three control points + four pinned corners, the SpecAugment-style call)
      if (M == 7) bands(std::integral_constant<int, 7>{}); else bands(std::integral_constant<int, kWarpFastM>{});
    };
    if (order == 2) go(std::integral_constant<int, 2>{});
    else if (order == 1) go(std::integral_constant<int, 1>{});
    else if (order == 3) go(std::integral_constant<int, 3>{});
    else go(std::integral_constant<int, 0>{});
    return (int)hipGetLastError();
   }
  }
  return launch_image_warp(a, (size_t)(2 * M + 2 * (M + 3)) * sizeof(float), (hipStream_t)stream);
}
}  // extern "C++"

int pdt_sparse_image_warp(const float *image, const float *train_points,
                          const float *train_values, int64_t N, int64_t C, int64_t H, int64_t W,
                          int64_t M, int order, float regularization_weight, int values_are_grid,
                          int mode, int padding, float *out, float *flow_out, int flow_out_is_hw,
                          void *workspace, void *stream) {
  return sparse_warp_launch<float>(image, train_points, train_values, N, C, H, W, M, order,
                                   regularization_weight, values_are_grid, mode, padding, out, flow_out,
                                   flow_out_is_hw, nullptr, workspace, stream);
}

int pdt_sparse_image_warp_backward(const float *grad_out, const float *train_points,
                                   const float *train_values, int64_t N, int64_t C, int64_t H,
                                   int64_t W, int64_t M, int order, float regularization_weight,
                                   int values_are_grid, int mode, int padding, float *grad_image,
                                   void *workspace, void *stream) {
  if (!grad_image && N && C && H && W) return PDT_E_ARG;
  return sparse_warp_launch<float>(nullptr, train_points, train_values, N, C, H, W, M, order,
                                   regularization_weight, values_are_grid, mode, padding,
                                   const_cast<float *>(grad_out), nullptr, 0, grad_image, workspace, stream);
}

// float64 images (the reference samples a double image on a double grid, _img.py:423-436; flows and
// spline points are float32 there whatever the image's type, :420, :537-538): image_warp_kernel in
// double from the grid on.  Same arguments as the float32 entries.
int pdt_dense_image_warp_f64(const double *image, const float *flow, int64_t N, int64_t C, int64_t H,
                             int64_t W, int flow_is_hw, int mode, int padding, double *out,
                             void *stream) {
  return dense_warp_launch<double>(image, flow, N, C, H, W, flow_is_hw, mode, padding, out, nullptr, stream);
}

int pdt_dense_image_warp_backward_f64(const double *grad_out, const float *flow, int64_t N, int64_t C,
                                      int64_t H, int64_t W, int flow_is_hw, int mode, int padding,
                                      double *grad_image, void *stream) {
  if (!grad_image && N && C && H && W) return PDT_E_ARG;
  return dense_warp_launch<double>(nullptr, flow, N, C, H, W, flow_is_hw, mode, padding,
                                   const_cast<double *>(grad_out), grad_image, stream);
}

int pdt_sparse_image_warp_f64(const double *image, const float *train_points,
                              const float *train_values, int64_t N, int64_t C, int64_t H, int64_t W,
                              int64_t M, int order, float regularization_weight, int values_are_grid,
                              int mode, int padding, double *out, float *flow_out, int flow_out_is_hw,
                              void *workspace, void *stream) {
  return sparse_warp_launch<double>(image, train_points, train_values, N, C, H, W, M, order,
                                    regularization_weight, values_are_grid, mode, padding, out, flow_out,
                                    flow_out_is_hw, nullptr, workspace, stream);
}

int pdt_sparse_image_warp_backward_f64(const double *grad_out, const float *train_points,
                                       const float *train_values, int64_t N, int64_t C, int64_t H,
                                       int64_t W, int64_t M, int order, float regularization_weight,
                                       int values_are_grid, int mode, int padding, double *grad_image,
                                       void *workspace, void *stream) {
  if (!grad_image && N && C && H && W) return PDT_E_ARG;
  return sparse_warp_launch<double>(nullptr, train_points, train_values, N, C, H, W, M, order,
                                    regularization_weight, values_are_grid, mode, padding,
                                    const_cast<double *>(grad_out), nullptr, 0, grad_image, workspace, stream);
}

// The position gradients (image_warp_kernel<WARP_POSITION>): the forward entry points' limits and checks.
extern "C++" {
template <typename PT>
static int dense_flow_backward_launch(const PT *grad_out, const PT *image, const float *flow, int64_t N, int64_t C,
                                      int64_t H, int64_t W, int flow_is_hw, int mode, int padding, float *grad_flow,
                                      void *stream) {
  using namespace pdt;
  if (N < 0 || C < 0 || H < 0 || W < 0 || mode < 0 || mode > 1 || padding < 0 || padding > 2)
    return PDT_E_ARG;
  if (N == 0 || H == 0 || W == 0) return PDT_OK;
  if (!grad_flow) return PDT_E_ARG;
  if (C == 0 || mode == INTERP_NEAREST)  // (no launch: a nearest sample does not move with its position)
    return (int)hipMemsetAsync(grad_flow, 0, (size_t)N * H * W * 2 * sizeof(float), (hipStream_t)stream);
  if (!grad_out || !image || !flow) return PDT_E_ARG;
  if (H * W >= (1ll << 31) || N > 65535) return PDT_E_TOO_LONG;
  WarpArgsT<PT> a = warp_args(image, const_cast<PT *>(grad_out), N, C, H, W, mode, padding, (PT *)nullptr);
  a.flow = flow; a.flip = flow_is_hw; a.grad_pos = grad_flow;
  return launch_image_warp(a, 0, (hipStream_t)stream);
}

// solution: the (N, M + 3, 2) float64 solution of the spline (pdt_spline_solve); its float copy goes to the
// head of the workspace, as in sparse_warp_launch
template <typename PT>
static int sparse_position_backward_launch(const PT *grad_out, const PT *image, const float *train_points,
                                           const double *solution, int64_t N, int64_t C, int64_t H, int64_t W,
                                           int64_t M, int order, int values_are_grid, int mode, int padding,
                                           const float *grad_flow, int grad_flow_is_hw, float *grad_values,
                                           void *workspace, void *stream) {
  using namespace pdt;
  if (N < 0 || C < 0 || H < 0 || W < 0 || M < 1 || order < 1 || mode < 0 || mode > 1 ||
      padding < 0 || padding > 2)
    return PDT_E_ARG;
  if (N == 0 || H == 0 || W == 0) return PDT_OK;
  if (!grad_values || (C > 0 && (!grad_out || !image)) || !train_points || !solution || !workspace)
    return PDT_E_ARG;
  if (grad_flow && values_are_grid) return PDT_E_ARG;  // (the no-flow form returns no flow)
  if (H * W >= (1ll << 31) || N > 65535) return PDT_E_TOO_LONG;
  const int64_t total = N * (M + 3) * 2;
  float *wvf = reinterpret_cast<float *>(workspace);
  hipLaunchKernelGGL(cast_wv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     solution, wvf, total);
  WarpArgsT<PT> a = warp_args(image, const_cast<PT *>(grad_out), N, C, H, W, mode, padding, (PT *)nullptr);
  a.knots = train_points; a.wv = wvf; a.M = (int)M; a.order = order; a.as_grid = values_are_grid;
  a.grad_pos = grad_values; a.grad_flow_in = grad_flow; a.flow_out_flip = grad_flow_is_hw;
  return launch_image_warp(a, (size_t)(2 * M + 2 * (M + 3)) * sizeof(float), (hipStream_t)stream);
}
}  // extern "C++"

int pdt_dense_image_warp_flow_backward(const float *grad_out, const float *image, const float *flow, int64_t N,
                                       int64_t C, int64_t H, int64_t W, int flow_is_hw, int mode, int padding,
                                       float *grad_flow, void *stream) {
  return dense_flow_backward_launch<float>(grad_out, image, flow, N, C, H, W, flow_is_hw, mode, padding, grad_flow,
                                           stream);
}

int pdt_dense_image_warp_flow_backward_f64(const double *grad_out, const double *image, const float *flow,
                                           int64_t N, int64_t C, int64_t H, int64_t W, int flow_is_hw, int mode,
                                           int padding, float *grad_flow, void *stream) {
  return dense_flow_backward_launch<double>(grad_out, image, flow, N, C, H, W, flow_is_hw, mode, padding,
                                            grad_flow, stream);
}

int pdt_sparse_image_warp_position_backward(const float *grad_out, const float *image, const float *train_points,
                                            const double *solution, int64_t N, int64_t C, int64_t H, int64_t W,
                                            int64_t M, int order, int values_are_grid, int mode, int padding,
                                            const float *grad_flow, int grad_flow_is_hw, float *grad_values,
                                            void *workspace, void *stream) {
  return sparse_position_backward_launch<float>(grad_out, image, train_points, solution, N, C, H, W, M, order,
                                                values_are_grid, mode, padding, grad_flow, grad_flow_is_hw,
                                                grad_values, workspace, stream);
}

int pdt_sparse_image_warp_position_backward_f64(const double *grad_out, const double *image,
                                                const float *train_points, const double *solution, int64_t N,
                                                int64_t C, int64_t H, int64_t W, int64_t M, int order,
                                                int values_are_grid, int mode, int padding, const float *grad_flow,
                                                int grad_flow_is_hw, float *grad_values, void *workspace,
                                                void *stream) {
  return sparse_position_backward_launch<double>(grad_out, image, train_points, solution, N, C, H, W, M, order,
                                                 values_are_grid, mode, padding, grad_flow, grad_flow_is_hw,
                                                 grad_values, workspace, stream);
}

}  // extern "C"
