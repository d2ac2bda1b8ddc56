// Polyharmonic splines for gfx950: the solver, the evaluation at query points, and warp_1d_grid.
//
// Replaces, from the reference's _img.py:
//   polyharmonic_spline (:59-150)            -> spline_solve_kernel + spline_apply_kernel
//   warp_1d_grid (:268-303)                  -> warp_1d_grid_kernel (3-knot spline, 5x5 solve)
//   the spline's backward, query-sized half  -> spline_adjoint_partial_kernel + spline_adjoint_sum_kernel
//       (what autograd derives through :67-76)  (+ spline_adjoint_gx_kernel for the queries' gradient)
// The small dense systems are solved in float64 (partial pivoting).  pdt::spline_solve also serves
// the sparse image warp (image_warp.hip, through img_launch.hpp).
#include "img_launch.hpp"
#include "img_sample.hpp"

namespace pdt {

// Solve the bordered system [[A + reg*I, B], [B^T, 0]] [w; v] = [f; 0] (_img.py:79-130) for one
// batch element with the whole workgroup: Gaussian elimination with partial pivoting, then back
// substitution.  a: (S, S + O) augmented matrix in LDS (doubles); the solution replaces its last O columns.
__device__ void solve_in_lds(double *a, int S, int O, int *piv_row) {
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int ld = S + O;
  for (int p = 0; p < S; ++p) {
    if (tid == 0) {  // partial pivoting
      int best = p;
      double bv = fabs(a[p * ld + p]);
      for (int r = p + 1; r < S; ++r) {
        const double v = fabs(a[r * ld + p]);
        if (v > bv) {
          bv = v;
          best = r;
        }
      }
      *piv_row = best;
    }
    __syncthreads();
    const int pr = *piv_row;
    if (pr != p)
      for (int c = tid; c < ld; c += nt) {
        const double t = a[p * ld + c];
        a[p * ld + c] = a[pr * ld + c];
        a[pr * ld + c] = t;
      }
    __syncthreads();
    const double inv = 1.0 / a[p * ld + p];
    // eliminate column p from the rows below: rows x columns over the threads.  (Column p itself is left
    // as it is below the diagonal: nothing reads it again.)
    const int ncol = ld - p - 1;
    for (int i = tid; i < (S - p - 1) * ncol; i += nt) {
      const int q = i / ncol, r = p + 1 + q, c = p + 1 + (i - q * ncol);
      a[r * ld + c] -= a[r * ld + p] * inv * a[p * ld + c];
    }
    __syncthreads();
  }
  // back substitution, last unknown first: x_p = b_p / a_pp leaves every row above it.  (Gaussian
  // elimination with partial pivoting is backward stable; the Gauss-Jordan sweep that stood here is not,
  // and lost a digit and more on ill-conditioned systems: 1.6e-5 against 1.3e-6 at T = 316 of order 3.)
  for (int p = S - 1; p > 0; --p) {
    const double app = a[p * ld + p];
    for (int i = tid; i < p * O; i += nt) {
      const int r = i / O, c = S + (i - r * O);
      a[r * ld + c] -= a[r * ld + p] * (a[p * ld + c] / app);
    }
    __syncthreads();
  }
  for (int i = tid; i < S * O; i += nt) {
    const int r = i / O, c = S + (i - r * O);
    a[r * ld + c] /= a[r * ld + r];
  }
  __syncthreads();
}

// train points c (N,T,I), values f (N,T,O) -> wv (N, T+I+1, O) doubles.  `tail` (N, I+1, O) or
// null: the last I + 1 rows of the right-hand side (zeros for the interpolation problem itself;
// the adjoint system of the backward pass has them).  `gmat` non-null: the augmented matrix of
// batch element n lives at gmat + n * S * (S + O) in global memory instead of LDS (systems too
// large for LDS; a workgroup's own global writes are visible to it after __syncthreads()).
__global__ void __launch_bounds__(256)
spline_solve_kernel(const float *__restrict__ c, const float *__restrict__ f,
                    const float *__restrict__ tail, int T, int I, int O, int order, float reg,
                    double *__restrict__ wv, double *gmat) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int S = T + I + 1, ld = S + O;
  const int64_t n = blockIdx.x;
  double *a = gmat ? gmat + n * (int64_t)S * ld : reinterpret_cast<double *>(smem);
  int *piv = gmat ? reinterpret_cast<int *>(smem) : reinterpret_cast<int *>(a + (size_t)S * ld);
  const float *cn = c + n * (int64_t)T * I;
  const float *fn = f + n * (int64_t)T * O;
  for (int i = (int)threadIdx.x; i < S * ld; i += (int)blockDim.x) {
    const int r = i / ld, col = i - r * ld;
    double v = 0.0;
    if (r < T && col < T) {
      double d2 = 0.0;
      for (int k = 0; k < I; ++k) {
        const double d = (double)cn[r * I + k] - (double)cn[col * I + k];
        d2 += d * d;
      }
      v = phi_d(sqrt(d2), order);
      if (r == col && reg > 0.0f) v += (double)reg;
    } else if (r < T && col < S) {  // B
      v = (col - T) < I ? (double)cn[r * I + (col - T)] : 1.0;
    } else if (r >= T && col < T) {  // B^T
      v = (r - T) < I ? (double)cn[col * I + (r - T)] : 1.0;
    } else if (r < T && col >= S) {
      v = (double)fn[r * O + (col - S)];
    } else if (r >= T && col >= S && tail) {
      v = (double)tail[(n * (I + 1) + (r - T)) * O + (col - S)];
    }
    a[i] = v;
  }
  __syncthreads();
  solve_in_lds(a, S, O, piv);
  for (int i = (int)threadIdx.x; i < S * O; i += (int)blockDim.x) {
    const int r = i / O, o = i - r * O;
    wv[(n * S + r) * O + o] = a[r * ld + S + o];
  }
}

// out[n,q,o] = sum_t phi(|x_q - c_t|) w[t,o] + x_q . v[:I,o] + v[I,o]     (_img.py:67-76)
// STAGE: the solution and the centres of batch element n are copied into LDS first (the launcher asks
// for spline_apply_lds_bytes); otherwise every lane reads them from global memory, at addresses the
// whole wave shares -- the same sums in the same order, for systems whose solution does not fit.
template <bool STAGE>
__global__ void __launch_bounds__(256)
spline_apply_kernel(const float *__restrict__ c, const double *__restrict__ wv,
                    const float *__restrict__ x, int T, int I, int O, int Q, int order,
                    float *__restrict__ out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int64_t n = blockIdx.y;
  const double *lw = wv + n * (int64_t)(T + I + 1) * O;  // (T + I + 1, O)
  const float *lc = c + n * (int64_t)T * I;              // (T, I)
  if (STAGE) {
    double *sw = reinterpret_cast<double *>(smem);
    float *sc = reinterpret_cast<float *>(sw + (size_t)(T + I + 1) * O);
    for (int i = (int)threadIdx.x; i < (T + I + 1) * O; i += (int)blockDim.x) sw[i] = lw[i];
    for (int i = (int)threadIdx.x; i < T * I; i += (int)blockDim.x) sc[i] = lc[i];
    __syncthreads();
    lw = sw;
    lc = sc;
  }
  const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (q >= Q) return;
  const float *xq = x + (n * (int64_t)Q + q) * I;
  for (int o = 0; o < O; ++o) {
    double acc = lw[(T + I) * O + o];
    for (int k = 0; k < I; ++k) acc += (double)xq[k] * lw[(T + k) * O + o];
    for (int t = 0; t < T; ++t) {
      double d2 = 0.0;
      for (int k = 0; k < I; ++k) {
        const double d = (double)xq[k] - (double)lc[t * I + k];
        d2 += d * d;
      }
      acc += phi_d(sqrt(d2), order) * lw[t * O + o];
    }
    out[(n * (int64_t)Q + q) * O + o] = (float)acc;
  }
}

// spline_apply_kernel's LDS copy of one batch element's solution and centres
static size_t spline_apply_lds_bytes(int64_t T, int64_t I, int64_t O) {
  return (size_t)(T + I + 1) * O * sizeof(double) + (size_t)T * I * sizeof(float);
}

// Evaluate the N solved splines in wv at their Q query points.  Every size spline_solve accepts is
// served: the copy in LDS up to kSplineLdsCap (beyond 64 KiB behind the function attribute, like the
// solver's), from global memory beyond it.
static int spline_apply(const float *c, const double *wv, const float *x, int64_t N, int64_t T, int64_t I, int64_t O,
                        int64_t Q, int order, float *out, hipStream_t stream) {
  const dim3 grid((unsigned)((Q + 255) / 256), (unsigned)N);
  const size_t smem = spline_apply_lds_bytes(T, I, O);
  if (smem > kSplineLdsCap) {
    hipLaunchKernelGGL(spline_apply_kernel<false>, grid, dim3(256), 0, stream, c, wv, x, (int)T, (int)I, (int)O,
                       (int)Q, order, out);
    return (int)hipGetLastError();
  }
  if (const int rc = set_lds(spline_apply_kernel<true>, smem)) return rc;
  hipLaunchKernelGGL(spline_apply_kernel<true>, grid, dim3(256), smem, stream, c, wv, x, (int)T, (int)I, (int)O,
                     (int)Q, order, out);
  return (int)hipGetLastError();
}

// ---- the evaluation's adjoint --------------------------------------------------------------------
// out = Phi(x, c) w + [x 1] v and G = dL/dout (N, Q, O): the query-sized sums of the spline's backward,
//   rhs[t]     = sum_q phi(r_qt) G[q]            (t < T; the adjoint system's right-hand side)
//   rhs[T + k] = sum_q x_qk G[q], rhs[T + I] = sum_q G[q]
//   g_c[t]     = -sum_q (G[q] . w[t]) slope(r_qt) (x_q - c_t)          (the evaluation's share)
// as a reduction over q that never forms anything of size Q x T.  phi and slope = phi'(r) / r as the
// float64 formulas of the host's backward have them (slope 0 at r = 0, the log clamped at eps).
//
// Lane = (row, slice of q): a row is a centre t or one of the I + 1 affine rows, and keeps its centre, its
// weights and its O + I float64 sums in registers for the whole walk; the workgroup's `nsl` slices step
// through its queries side by side (slice s takes q0 + s, q0 + s + nsl, ...), so no lane waits for a
// cross-lane sum per centre.  Rows vary fastest within the workgroup: a wave's lanes read a handful of
// neighbouring queries.  The slices are combined once per workgroup in LDS, in slice order, and the
// workgroup stores its partial sums; spline_adjoint_sum_kernel adds the workgroups' partials in their
// fixed order -- no floating-point atomics, the same bits every run.
// Systems of more than kAdjRows rows: one slice, the rows in tiles of kAdjRows over further workgroups.
constexpr int kAdjRows = 256;     // threads of a workgroup = rows x slices
constexpr int kAdjMinSteps = 64;  // queries a slice walks at least (while there are that many)
constexpr int kAdjMaxChunks = 128;  // workgroups along q per batch element at most (bounds the partials)
constexpr int kAdjMaxDim = 4;     // I and O served in registers

struct AdjPlan {
  int form;        // 0: all rows in one workgroup, nsl slices; 1: row tiles, one slice
  int nsl, tiles, chunks, qper;  // slices, row tiles, workgroups along q, queries per workgroup
  int gx_staged;   // spline_adjoint_gx_kernel reads solution and centres from LDS (else global memory)
  int64_t partial_doubles;  // per batch element
};
static AdjPlan adj_plan(int64_t T, int64_t I, int64_t O, int64_t Q) {
  AdjPlan p;
  const int64_t S = T + I + 1;
  p.form = S > kAdjRows ? 1 : 0;
  p.nsl = p.form ? 1 : (int)(kAdjRows / S);
  p.tiles = (int)((S + kAdjRows - 1) / kAdjRows);
  const int64_t per_min = (int64_t)p.nsl * kAdjMinSteps;
  int64_t chunks = (Q + per_min - 1) / per_min;
  if (chunks > kAdjMaxChunks) chunks = kAdjMaxChunks;
  if (chunks < 1) chunks = 1;
  int64_t qper = (Q + chunks - 1) / chunks;
  qper = (qper + p.nsl - 1) / p.nsl * p.nsl;
  if (qper < p.nsl) qper = p.nsl;
  p.chunks = (int)((Q + qper - 1) / qper);
  if (p.chunks < 1) p.chunks = 1;
  p.qper = (int)qper;
  p.gx_staged = spline_apply_lds_bytes(T, I, O) <= kSplineLdsCap;
  p.partial_doubles = (int64_t)p.chunks * (S * O + T * I);
  return p;
}

__device__ __forceinline__ double ipow_d(double r, int k) {
  double p = 1.0;
  for (int i = 0; i < k; ++i) p *= r;
  return p;
}
// phi(r) and phi'(r) / r (zero where r = 0: the direction vector vanishes there)
__device__ __forceinline__ void phi_and_slope_d(double r, int order, double &phi, double &slope) {
  const double eps = (double)FLT_EPSILON;
  const bool pos = r > 0.0;
  const double safe = pos ? r : 1.0;
  const double pw = order >= 2 ? ipow_d(safe, order - 2) : 1.0 / safe;  // safe^(order - 2)
  if (order & 1) {
    phi = ipow_d(r, order);
    slope = (double)order * pw;
  } else {
    const double lg = log(fmax(safe, eps));
    phi = ipow_d(r, order) * lg;
    slope = pw * (safe > eps ? (double)order * lg + 1.0 : (double)order * log(eps));
  }
  if (!pos) slope = 0.0;
}

// x: (N, Q, I) or null = the pixel lattice (q % W, q / W) with I = 2.  part: (N, chunks, S*O + T*I).
__global__ void __launch_bounds__(kAdjRows)
spline_adjoint_partial_kernel(const float *__restrict__ G, const float *__restrict__ c,
                              const double *__restrict__ sol, const float *__restrict__ x, int T, int I, int O, int Q,
                              int W, int order, int nsl, int tiles, int qper, double *__restrict__ part) {
  __shared__ double buf[kAdjRows * 2 * kAdjMaxDim];
  const int S = T + I + 1, NV = O + I;
  const int64_t n = blockIdx.y;
  const int tile = (int)(blockIdx.x % (unsigned)tiles), chunk = (int)(blockIdx.x / (unsigned)tiles);
  const int rows = min(kAdjRows, S - tile * kAdjRows);  // rows of this workgroup
  const int tid = (int)threadIdx.x;
  const int s = tid / rows, rr = tid - s * rows, row = tile * kAdjRows + rr;
  const bool live = s < nsl;
  double acc[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0}, gcv[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0};
  double ct[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0}, wt[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0};
  if (live && row < T) {
#pragma unroll
    for (int k = 0; k < kAdjMaxDim; ++k)
      if (k < I) ct[k] = (double)c[(n * T + row) * I + k];
#pragma unroll
    for (int o = 0; o < kAdjMaxDim; ++o)
      if (o < O) wt[o] = sol[(n * S + row) * O + o];
  }
  const int q0 = chunk * qper, q1 = min(Q, q0 + qper);
  if (live) {
    for (int q = q0 + s; q < q1; q += nsl) {
      double xq[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0}, g[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0};
      if (x) {
#pragma unroll
        for (int k = 0; k < kAdjMaxDim; ++k)
          if (k < I) xq[k] = (double)x[(n * Q + q) * I + k];
      } else {
        const int h = q / W;
        xq[0] = (double)(q - h * W);
        xq[1] = (double)h;
      }
#pragma unroll
      for (int o = 0; o < kAdjMaxDim; ++o)
        if (o < O) g[o] = (double)G[(n * Q + q) * O + o];
      if (row < T) {
        double d[kAdjMaxDim], d2 = 0.0, a = 0.0, phi, slope;
#pragma unroll
        for (int k = 0; k < kAdjMaxDim; ++k) {
          d[k] = xq[k] - ct[k];  // (components beyond I: 0 - 0)
          d2 += d[k] * d[k];
        }
        phi_and_slope_d(sqrt(d2), order, phi, slope);
#pragma unroll
        for (int o = 0; o < kAdjMaxDim; ++o) {
          acc[o] += phi * g[o];
          a += g[o] * wt[o];
        }
        a *= slope;
#pragma unroll
        for (int k = 0; k < kAdjMaxDim; ++k) gcv[k] -= a * d[k];
      } else {  // an affine row: x_qk (row T + k) or 1 (row T + I) in phi's place
        double f = 1.0;
#pragma unroll
        for (int k = 0; k < kAdjMaxDim; ++k)
          if (row - T == k && k < I) f = xq[k];
#pragma unroll
        for (int o = 0; o < kAdjMaxDim; ++o) acc[o] += f * g[o];
      }
    }
#pragma unroll
    for (int o = 0; o < kAdjMaxDim; ++o)
      if (o < O) buf[tid * NV + o] = acc[o];
#pragma unroll
    for (int k = 0; k < kAdjMaxDim; ++k)
      if (k < I) buf[tid * NV + O + k] = gcv[k];
  }
  __syncthreads();
  // the slices' sums in slice order: thread j owns value v of row rr
  double *pn = part + (n * gridDim.x / tiles + chunk) * ((int64_t)S * O + (int64_t)T * I);
  for (int j = tid; j < rows * NV; j += kAdjRows) {
    const int r = j / NV, v = j - r * NV, grow = tile * kAdjRows + r;
    double sum = 0.0;
    for (int sl = 0; sl < nsl; ++sl) sum += buf[(sl * rows + r) * NV + v];
    if (v < O) pn[(int64_t)grow * O + v] = sum;
    else if (grow < T) pn[(int64_t)S * O + (int64_t)grow * I + (v - O)] = sum;
  }
}

// rhs (N, S, O) then g_c (N, T, I): each element the sum of its `chunks` partials, first to last
__global__ void __launch_bounds__(256)
spline_adjoint_sum_kernel(const double *__restrict__ part, int chunks, int64_t so, int64_t ti,
                          double *__restrict__ rhs, double *__restrict__ gc) {
  const int64_t n = blockIdx.y, per = so + ti;
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= per) return;
  const double *p = part + n * chunks * per + e;
  double sum = 0.0;
  for (int k = 0; k < chunks; ++k) sum += p[k * per];
  if (e < so) rhs[n * so + e] = sum;
  else gc[n * ti + (e - so)] = sum;
}

// g_x[q] = sum_t (G[q] . w[t]) slope(r_qt) (x_q - c_t) + v[:I] G[q]: lane = query, the centres in a loop
// (spline_apply_kernel's structure and staging)
template <bool STAGE>
__global__ void __launch_bounds__(256)
spline_adjoint_gx_kernel(const float *__restrict__ G, const float *__restrict__ c, const double *__restrict__ wv,
                         const float *__restrict__ x, int T, int I, int O, int Q, int order,
                         double *__restrict__ gx) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int64_t n = blockIdx.y;
  const double *lw = wv + n * (int64_t)(T + I + 1) * O;
  const float *lc = c + n * (int64_t)T * I;
  if (STAGE) {
    double *sw = reinterpret_cast<double *>(smem);
    float *sc = reinterpret_cast<float *>(sw + (size_t)(T + I + 1) * O);
    for (int i = (int)threadIdx.x; i < (T + I + 1) * O; i += (int)blockDim.x) sw[i] = lw[i];
    for (int i = (int)threadIdx.x; i < T * I; i += (int)blockDim.x) sc[i] = lc[i];
    __syncthreads();
    lw = sw;
    lc = sc;
  }
  const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (q >= Q) return;
  double xq[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0}, g[kAdjMaxDim] = {0.0, 0.0, 0.0, 0.0}, out[kAdjMaxDim];
#pragma unroll
  for (int k = 0; k < kAdjMaxDim; ++k)
    if (k < I) xq[k] = (double)x[(n * Q + q) * I + k];
#pragma unroll
  for (int o = 0; o < kAdjMaxDim; ++o)
    if (o < O) g[o] = (double)G[(n * Q + q) * O + o];
#pragma unroll
  for (int k = 0; k < kAdjMaxDim; ++k) {
    out[k] = 0.0;
    if (k < I)
      for (int o = 0; o < O; ++o) out[k] += g[o] * lw[(T + k) * O + o];
  }
  for (int t = 0; t < T; ++t) {
    double d[kAdjMaxDim], d2 = 0.0, a = 0.0, phi, slope;
#pragma unroll
    for (int k = 0; k < kAdjMaxDim; ++k) {
      d[k] = k < I ? xq[k] - (double)lc[t * I + k] : 0.0;
      d2 += d[k] * d[k];
    }
    phi_and_slope_d(sqrt(d2), order, phi, slope);
#pragma unroll
    for (int o = 0; o < kAdjMaxDim; ++o)
      if (o < O) a += g[o] * lw[t * O + o];
    a *= slope;
#pragma unroll
    for (int k = 0; k < kAdjMaxDim; ++k) out[k] += a * d[k];
  }
#pragma unroll
  for (int k = 0; k < kAdjMaxDim; ++k)
    if (k < I) gx[(n * Q + q) * I + k] = out[k];
}

// warp_1d_grid (_img.py:268-303): one workgroup per batch element
__global__ void __launch_bounds__(256)
warp_1d_grid_kernel(const float *__restrict__ src, const float *__restrict__ flow,
                    const float *__restrict__ lengths, int T, int order,
                    float *__restrict__ grid) {
  __shared__ double a[5 * 6];
  __shared__ int piv;
  __shared__ double knots[3];
  const int64_t n = blockIdx.x;
  const double len = (double)lengths[n];
  if (threadIdx.x == 0) {
    const double eps = (double)FLT_EPSILON;
    double s = fmax(fmin((double)src[n], len - 1.0), 0.0);
    double d = fmax(fmin(s + (double)flow[n], len - 1.0), 0.0);
    s = (2.0 * s + 1.0) / T - 1.0;
    d = (2.0 * d + 1.0) / T - 1.0;
    const double lo = 1.0 / T - 1.0 - eps, up = (2.0 * len - 1.0) / T - 1.0 + eps;
    const double cp[3] = {lo, d, up}, fv[3] = {lo, s, up};  // spline FROM dst TO src
    for (int r = 0; r < 5; ++r)
      for (int c = 0; c < 6; ++c) {
        double v = 0.0;
        if (r < 3 && c < 3) v = phi_d(fabs(cp[r] - cp[c]), order);
        else if (r < 3 && c == 3) v = cp[r];
        else if (r < 3 && c == 4) v = 1.0;
        else if (r == 3 && c < 3) v = cp[c];
        else if (r == 4 && c < 3) v = 1.0;
        else if (r < 3 && c == 5) v = fv[r];
        a[r * 6 + c] = v;
      }
    for (int k = 0; k < 3; ++k) knots[k] = cp[k];
  }
  __syncthreads();
  solve_in_lds(a, 5, 1, &piv);
  const double w0 = a[0 * 6 + 5], w1 = a[1 * 6 + 5], w2 = a[2 * 6 + 5];
  const double v0 = a[3 * 6 + 5], v1 = a[4 * 6 + 5];
  for (int j = (int)threadIdx.x; j < T; j += (int)blockDim.x) {
    const double t = (2.0 * j + 1.0) / T - 1.0;
    const double g = w0 * phi_d(fabs(t - knots[0]), order) + w1 * phi_d(fabs(t - knots[1]), order) +
                     w2 * phi_d(fabs(t - knots[2]), order) + v0 * t + v1;
    grid[n * (int64_t)T + j] = (float)g;
  }
}

int spline_solve(const float *c, const float *f, const float *tail, int64_t N, int64_t T, int64_t I, int64_t O,
                 int order, float reg, double *wv, hipStream_t stream) {
  const int64_t S = T + I + 1;
  if (S > 4096 || O > 64) return PDT_E_TOO_LONG;
  size_t smem = (size_t)S * (S + O) * sizeof(double) + 16;
  double *gmat = nullptr;
  if (smem > kSplineLdsCap) {  // the matrix follows the (N, S, O) doubles + floats of the solutions
    gmat = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(wv) +
                                      (((size_t)N * S * O * (sizeof(double) + sizeof(float)) + 63) & ~(size_t)63));
    smem = 16;
  }
  if (const int rc = set_lds(spline_solve_kernel, smem)) return rc;
  hipLaunchKernelGGL(spline_solve_kernel, dim3((unsigned)N), dim3(256), smem, stream, c, f, tail,
                     (int)T, (int)I, (int)O, order, reg, wv, gmat);
  return (int)hipGetLastError();
}

}  // namespace pdt

extern "C" {

int64_t pdt_spline_workspace_bytes(int64_t N, int64_t T, int64_t I, int64_t O) {
  if (N < 0 || T < 0 || I < 0 || O < 0) return 0;
  const int64_t S = T + I + 1;
  int64_t bytes = N * S * O * (int64_t)(sizeof(double) + sizeof(float)) + 64;
  bytes += N * pdt::kWarpTableFloats * (int64_t)sizeof(float);  // sparse_warp_bands_kernel's per-image table
  // systems beyond the LDS are eliminated in global memory, after the solutions
  if ((size_t)S * (S + O) * sizeof(double) + 16 > pdt::kSplineLdsCap) bytes += N * S * (S + O) * (int64_t)sizeof(double);
  return bytes;
}

int pdt_spline_solve(const float *train_points, const float *train_values, const float *tail,
                     int64_t N, int64_t T, int64_t I, int64_t O, int order,
                     float regularization_weight, double *solution, void *workspace, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 1 || I < 1 || O < 1 || order < 1) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!train_points || !train_values || !solution || !workspace) return PDT_E_ARG;
  if (N > 65535) return PDT_E_TOO_LONG;
  double *wv = reinterpret_cast<double *>(workspace);
  int rc = spline_solve(train_points, train_values, tail, N, T, I, O, order, regularization_weight, wv,
                        (hipStream_t)stream);
  if (rc != PDT_OK) return rc;
  return (int)hipMemcpyAsync(solution, wv, (size_t)N * (T + I + 1) * O * sizeof(double),
                             hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

int pdt_polyharmonic_spline(const float *train_points, const float *train_values,
                            const float *query_points, int64_t N, int64_t T, int64_t I, int64_t O,
                            int64_t Q, int order, float regularization_weight, float *out,
                            void *workspace, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 1 || I < 1 || O < 1 || Q < 0 || order < 1) return PDT_E_ARG;
  if (N == 0 || Q == 0) return PDT_OK;
  if (!train_points || !train_values || !query_points || !out || !workspace) return PDT_E_ARG;
  if (N > 65535) return PDT_E_TOO_LONG;
  double *wv = reinterpret_cast<double *>(workspace);
  int rc = spline_solve(train_points, train_values, nullptr, N, T, I, O, order, regularization_weight, wv,
                        (hipStream_t)stream);
  if (rc != PDT_OK) return rc;
  return spline_apply(train_points, wv, query_points, N, T, I, O, Q, order, out, (hipStream_t)stream);
}

// the checks pdt_spline_eval_adjoint and its plan share
static int eval_adjoint_check(int64_t N, int64_t T, int64_t I, int64_t O, int64_t Q, int order) {
  if (N < 0 || T < 1 || I < 1 || O < 1 || Q < 0 || order < 1) return PDT_E_ARG;
  if (I > pdt::kAdjMaxDim || O > pdt::kAdjMaxDim) return PDT_E_UNSUPPORTED;
  if (N > 65535 || Q >= (1ll << 31) || T > (1ll << 20)) return PDT_E_TOO_LONG;
  return PDT_OK;
}

int pdt_spline_eval_adjoint_plan(int64_t N, int64_t T, int64_t I, int64_t O, int64_t Q, int64_t *plan) {
  if (const int rc = eval_adjoint_check(N, T, I, O, Q, 1)) return rc;
  const pdt::AdjPlan p = pdt::adj_plan(T, I, O, Q);
  if (plan) {
    plan[0] = p.form;
    plan[1] = (int64_t)p.chunks * p.tiles;                                // workgroups per batch element
    plan[2] = N * p.partial_doubles * (int64_t)sizeof(double) + 64;      // workspace bytes
    plan[3] = p.gx_staged;
    plan[4] = p.nsl;
    plan[5] = p.qper;
  }
  return p.form;
}

int pdt_spline_eval_adjoint(const float *grad_out, const float *train_points, const double *solution,
                            const float *query_points, int64_t N, int64_t T, int64_t I, int64_t O, int64_t Q,
                            int64_t H, int64_t W, int order, double *rhs, double *grad_points,
                            double *grad_query, void *workspace, void *stream) {
  using namespace pdt;
  if (const int rc = eval_adjoint_check(N, T, I, O, Q, order)) return rc;
  if (!query_points && (I != 2 || H < 0 || W < 0 || H * W != Q || grad_query)) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!train_points || !solution || !rhs || !grad_points || !workspace || (Q > 0 && !grad_out)) return PDT_E_ARG;
  const AdjPlan p = adj_plan(T, I, O, Q);
  const int64_t S = T + I + 1;
  double *part = reinterpret_cast<double *>(workspace);
  hipLaunchKernelGGL(spline_adjoint_partial_kernel, dim3((unsigned)(p.chunks * p.tiles), (unsigned)N), dim3(kAdjRows),
                     0, (hipStream_t)stream, grad_out, train_points, solution, query_points, (int)T, (int)I, (int)O,
                     (int)Q, (int)(W > 0 ? W : 1), order, p.nsl, p.tiles, p.qper, part);
  const int64_t per = S * O + T * I;
  hipLaunchKernelGGL(spline_adjoint_sum_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)N), dim3(256), 0,
                     (hipStream_t)stream, part, p.chunks, S * O, T * I, rhs, grad_points);
  if (grad_query && Q > 0) {
    const dim3 grid((unsigned)((Q + 255) / 256), (unsigned)N);
    if (p.gx_staged) {
      const size_t smem = spline_apply_lds_bytes(T, I, O);
      if (const int rc = set_lds(spline_adjoint_gx_kernel<true>, smem)) return rc;
      hipLaunchKernelGGL(spline_adjoint_gx_kernel<true>, grid, dim3(256), smem, (hipStream_t)stream, grad_out,
                         train_points, solution, query_points, (int)T, (int)I, (int)O, (int)Q, order, grad_query);
    } else {
      hipLaunchKernelGGL(spline_adjoint_gx_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, grad_out,
                         train_points, solution, query_points, (int)T, (int)I, (int)O, (int)Q, order, grad_query);
    }
  }
  return (int)hipGetLastError();
}

int pdt_warp_1d_grid(const float *src, const float *flow, const float *lengths, int64_t N, int64_t T,
                     int order, float *grid, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0 || order < 1) return PDT_E_ARG;
  if (N == 0 || T == 0) return PDT_OK;
  if (!src || !flow || !lengths || !grid) return PDT_E_ARG;
  hipLaunchKernelGGL(warp_1d_grid_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, src,
                     flow, lengths, (int)T, order, grid);
  return (int)hipGetLastError();
}

}  // extern "C"
