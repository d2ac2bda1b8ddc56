// The additive attention score (reference _attn.py:344-361) without its hidden-sized intermediate:
//   e[r, t] = sum_h v[h] * tanh(a[r, h] + b[group(r), t, h])
// a = the query half of W applied to the query (rows x H), b = the key half applied to the key
// (groups x T x H).  Rows, groups and strides are those of csrc/attn.hip: up to eight row dims, the
// ones over which b is broadcast (the group: beams sharing an utterance) innermost, per-operand
// element strides with 0 for a broadcast, every offset in 64 bits.
//
// Forward.  One workgroup serves a tile of up to eight rows of one group over a block of frames.
// H goes by chunks of up to 2048 features: the tile's chunk of a and the chunk of v sit in LDS
// (fewer rows per tile when that would pass 56 KiB), one wave per frame walks the chunk with lanes
// across H and four loads of b in flight, every element of b loaded serves every row of the tile,
// and one cross-lane sum per (row, frame) and chunk is added to the frame's score in LDS.
//
// Backward.  One workgroup per (group, 32 frames), one thread per feature h (blocks of 256): the
// thread keeps b[t, h] of its 32 frames in registers, walks every row of the group, recomputes
// th = tanh(a + b) and g = dE * v * (1 - th^2), and owns grad_b[t, h] for the whole walk (written
// once), the frames' share of grad_a[r, h] and the workgroup's share of grad_v[h].  grad_v's shares,
// and grad_a's when there are several frame chunks, go to a workspace that a combine pass adds in
// chunk order.  No float atomics anywhere: every result is bitwise reproducible.
#include "pdt_common.hpp"

#include <algorithm>
#include <cmath>

namespace pdt {

constexpr int kCsThreads = 256;
constexpr int kCsWaves = kCsThreads / PDT_WAVE;
constexpr int kCsRows = 8;           // rows per tile (at most)
constexpr int kCsFrames = 32;        // frames per workgroup (forward: at most; backward: per chunk)
constexpr int kCsMinFrames = 4;      // forward: one frame per wave at least
constexpr int64_t kCsChunk = 2048;   // features of a and v in LDS at a time
constexpr int64_t kCsLdsBytes = 57344;
constexpr int64_t kCsFill = 1024;    // workgroups that fill the 256 CUs four deep
constexpr int kCsSegs = 16;          // grad_v combine: segments of partials summed side by side

// the slots the kernels keep (and where the descriptor of include/pdt_amd.h holds them)
enum { CA = 0, CB, CGE, CE, CGA, CGB, CSLOT };
constexpr int kCsDescSlot[CSLOT] = {0, 1, 3, 4, 5, 6};

struct ConcatDesc {
  int64_t nd, R, G, M, T, H, vs;
  int64_t size[PDT_ATTN_MAX_DIMS];
  int64_t st[CSLOT][PDT_ATTN_MAX_DIMS];
  int64_t ts[CSLOT], fs[CSLOT];
};

struct ConcatArgs {
  ConcatDesc d;
  const void *a, *b, *v, *ge;
  void *e, *ga, *gb, *gv, *ws;
  int64_t rt, tiles, hc, fpw, fblocks;  // forward
  int64_t chunks;                       // backward frame chunks
};

struct ConcatPlan {
  int64_t rt, tiles, hc, hchunks, fpw, fblocks, lds_bytes;
  int64_t chunks, ws_bytes;
};

// element offsets of row r in the slots the kernels read (row dims innermost last)
__device__ __forceinline__ void cs_row_offsets(const ConcatDesc &d, int64_t r, int64_t off[CSLOT]) {
#pragma unroll
  for (int s = 0; s < CSLOT; ++s) off[s] = 0;
#pragma unroll
  for (int i = PDT_ATTN_MAX_DIMS - 1; i >= 0; --i) {
    if (i < d.nd) {
      const int64_t n = d.size[i], idx = r % n;
      r /= n;
#pragma unroll
      for (int s = 0; s < CSLOT; ++s) off[s] += idx * d.st[s][i];
    }
  }
}

template <typename F> __device__ __forceinline__ F cs_wave_sum(F x) {
#pragma unroll
  for (int o = PDT_WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// tanh.  float64: the device library's.  float32: 1 - 2 / (exp(2|x|) + 1) with the hardware's exp2 and
// reciprocal; exp overflows to +inf from |x| = 44.4 on and the quotient is then exactly 0, so the result is
// exactly +-1 (for +-inf too) and 1 - th^2 exactly 0, and a NaN goes through exp.  Below 0.125 the difference
// would cancel (an error of 6e-8 next to |x| = 1e-6), so the odd series to x^9 is taken there (its first
// dropped term is 8.9e-3 x^11: under 1e-11 relative).
__device__ __forceinline__ double cs_tanh(double x) { return tanh(x); }
__device__ __forceinline__ float cs_tanh(float x) {
  const float ax = fabsf(x);
  const float ex = __builtin_amdgcn_exp2f(ax * 2.8853900817779268f);  // exp(2 |x|)
  const float big = 1.0f - 2.0f * __builtin_amdgcn_rcpf(ex + 1.0f);
  const float x2 = ax * ax;
  const float small =
      ax * (1.0f + x2 * (-0.33333333333f + x2 * (0.13333333333f + x2 * (-0.05396825397f + x2 * 0.02186948854f))));
  return copysignf(ax < 0.125f ? small : big, x);
}

template <typename F> __global__ __launch_bounds__(kCsThreads) void concat_fwd_kernel(ConcatArgs a) {
  extern __shared__ __align__(16) unsigned char concat_smem[];
  const ConcatDesc &d = a.d;
  F *as = reinterpret_cast<F *>(concat_smem);  // [rt][hc]
  F *vs = as + a.rt * a.hc;                    // [hc]
  __shared__ int64_t roff[kCsRows][CSLOT];  // (CA, CB and CE are kept)
  __shared__ F acc[kCsRows][kCsFrames];
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int64_t fb = (int64_t)blockIdx.x % a.fblocks, gt = (int64_t)blockIdx.x / a.fblocks;
  const int64_t g = gt / a.tiles, tile = gt % a.tiles;
  const int64_t r0 = g * d.M + tile * a.rt;
  const int nr = (int)min(a.rt, d.M - tile * a.rt);
  const int64_t t0 = fb * a.fpw;
  const int nf = (int)min(a.fpw, d.T - t0);
  const F *pa = (const F *)a.a, *pb = (const F *)a.b, *pv = (const F *)a.v;

  if (tid < nr) {
    int64_t off[CSLOT];
    cs_row_offsets(d, r0 + tid, off);
    roff[tid][CA] = off[CA];
    roff[tid][CB] = off[CB];
    roff[tid][CE] = off[CE];
  }
  __syncthreads();
  const int64_t boff = roff[0][CB];  // (the same for every row of the group)
  const int hc = (int)a.hc;

  for (int64_t h0 = 0; h0 < d.H; h0 += a.hc) {
    const int hn = (int)min(a.hc, d.H - h0);
    if (h0 > 0) __syncthreads();  // (the previous chunk has been read)
    for (int i = tid; i < nr * hn; i += kCsThreads) {
      const int r = i / hn, c = i - r * hn;
      as[r * hc + c] = pa[roff[r][CA] + (h0 + c) * d.fs[CA]];
    }
    for (int c = tid; c < hn; c += kCsThreads) vs[c] = pv[(h0 + c) * d.vs];
    __syncthreads();
    for (int j = wave; j < nf; j += kCsWaves) {
      F s[kCsRows];
#pragma unroll
      for (int r = 0; r < kCsRows; ++r) s[r] = 0;
      const F *bp = pb + boff + (t0 + j) * d.ts[CB] + h0 * d.fs[CB];
      for (int c0 = lane; c0 < hn; c0 += 4 * PDT_WAVE) {
        F bv[4];  // (four loads in flight before the tanh's)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c0 + u * PDT_WAVE;
          bv[u] = c < hn ? bp[(int64_t)c * d.fs[CB]] : (F)0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c0 + u * PDT_WAVE;
          if (c < hn) {
            const F vv = vs[c];
#pragma unroll
            for (int r = 0; r < kCsRows; ++r)
              if (r < nr) s[r] += vv * cs_tanh(as[r * hc + c] + bv[u]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < kCsRows; ++r) s[r] = cs_wave_sum(s[r]);
      if (lane < kCsRows) {  // (this lane owns acc[lane][j] for every chunk)
        F mine = 0;
#pragma unroll
        for (int r = 0; r < kCsRows; ++r) mine = lane == r ? s[r] : mine;
        acc[lane][j] = h0 == 0 ? mine : acc[lane][j] + mine;
      }
    }
  }
  __syncthreads();
  F *pe = (F *)a.e;
  for (int i = tid; i < nr * nf; i += kCsThreads) {
    const int r = i / nf, j = i - r * nf;
    pe[roff[r][CE] + (t0 + j) * d.ts[CE]] = acc[r][j];
  }
}

template <typename F> __global__ __launch_bounds__(kCsThreads) void concat_bwd_kernel(ConcatArgs a) {
  const ConcatDesc &d = a.d;
  __shared__ int64_t roff[kCsRows][CSLOT];
  __shared__ F ges[kCsRows][kCsFrames];
  const int tid = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x % a.chunks;
  const int64_t t0 = chunk * kCsFrames;
  const int nf = (int)min((int64_t)kCsFrames, d.T - t0);
  const int64_t tiles = (d.M + kCsRows - 1) / kCsRows;
  const F *pa = (const F *)a.a, *pb = (const F *)a.b, *pv = (const F *)a.v, *pge = (const F *)a.ge;
  F *gv_part = (F *)a.ws;                             // [G * chunks][H]
  F *ga_part = gv_part + d.G * a.chunks * d.H;        // [chunks][R][H]
  F *pga = (F *)a.ga, *pgb = (F *)a.gb;
  int64_t off0[CSLOT];
  cs_row_offsets(d, g * d.M, off0);
  const int64_t boff = off0[CB], gboff = off0[CGB];  // (the same for every row of the group)

  for (int64_t h0 = 0; h0 < d.H; h0 += kCsThreads) {
    const int64_t h = h0 + tid;
    const bool live = h < d.H;
    const F vh = live ? pv[h * d.vs] : (F)0;
    F bj[kCsFrames], gbacc[kCsFrames];
    F gvacc = 0;
#pragma unroll
    for (int j = 0; j < kCsFrames; ++j) {
      bj[j] = live && j < nf ? pb[boff + (t0 + j) * d.ts[CB] + h * d.fs[CB]] : (F)0;
      gbacc[j] = 0;
    }
    for (int64_t tile = 0; tile < tiles; ++tile) {
      const int64_t r0 = g * d.M + tile * kCsRows;
      const int nr = (int)min((int64_t)kCsRows, d.M - tile * kCsRows);
      __syncthreads();  // (the previous tile has been read)
      if (tid < nr) {
        int64_t off[CSLOT];
        cs_row_offsets(d, r0 + tid, off);
        roff[tid][CA] = off[CA];
        roff[tid][CGE] = off[CGE];
        roff[tid][CGA] = off[CGA];
      }
      __syncthreads();
      {
        const int r = tid / kCsFrames, j = tid % kCsFrames;  // (kCsRows * kCsFrames == kCsThreads)
        ges[r][j] = r < nr && j < nf ? pge[roff[r][CGE] + (t0 + j) * d.ts[CGE]] : (F)0;
      }
      __syncthreads();
      for (int r = 0; r < nr; ++r) {
        const F ar = live ? pa[roff[r][CA] + h * d.fs[CA]] : (F)0;
        F gaacc = 0;
#pragma unroll
        for (int j = 0; j < kCsFrames; ++j) {
          if (j < nf) {
            const F th = cs_tanh(ar + bj[j]);
            const F ge = ges[r][j];
            gvacc += ge * th;
            const F gg = ge * vh * ((F)1 - th * th);
            gaacc += gg;
            gbacc[j] += gg;
          }
        }
        if (live) {
          if (a.chunks == 1)
            pga[roff[r][CGA] + h * d.fs[CGA]] = gaacc;
          else
            ga_part[(chunk * d.R + r0 + r) * d.H + h] = gaacc;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < kCsFrames; ++j)
        if (j < nf) pgb[gboff + (t0 + j) * d.ts[CGB] + h * d.fs[CGB]] = gbacc[j];
      gv_part[(int64_t)blockIdx.x * d.H + h] = gvacc;
    }
  }
}
static_assert(kCsRows * kCsFrames == kCsThreads, "the upstream tile gives every (row, frame) one thread");

// grad_a: the chunks' partials added in chunk order, one thread per (row, feature)
template <typename F> __global__ __launch_bounds__(kCsThreads) void concat_ga_combine_kernel(ConcatArgs a) {
  const ConcatDesc &d = a.d;
  const int64_t i = (int64_t)blockIdx.x * kCsThreads + threadIdx.x;
  if (i >= d.R * d.H) return;
  const int64_t r = i / d.H, h = i - r * d.H;
  const F *part = (const F *)a.ws + d.G * a.chunks * d.H;
  F s = 0;
  for (int64_t ch = 0; ch < a.chunks; ++ch) s += part[(ch * d.R + r) * d.H + h];
  int64_t off[CSLOT];
  cs_row_offsets(d, r, off);
  ((F *)a.ga)[off[CGA] + h * d.fs[CGA]] = s;
}

// grad_v: the workgroups' partials in a fixed order.  64 features per workgroup; kCsSegs waves each add a
// contiguous run of partials in order, then the runs' sums are added in order.
template <typename F> __global__ __launch_bounds__(PDT_WAVE *kCsSegs) void concat_gv_combine_kernel(ConcatArgs a) {
  const ConcatDesc &d = a.d;
  __shared__ F seg[kCsSegs][PDT_WAVE];
  const int lane = threadIdx.x & (PDT_WAVE - 1), w = threadIdx.x / PDT_WAVE;
  const int64_t h = (int64_t)blockIdx.x * PDT_WAVE + lane;
  const int64_t P = d.G * a.chunks, per = (P + kCsSegs - 1) / kCsSegs;
  const int64_t p0 = min(P, w * per), p1 = min(P, p0 + per);
  const F *part = (const F *)a.ws;
  F s = 0;
  if (h < d.H)
    for (int64_t p = p0; p < p1; ++p) s += part[p * d.H + h];
  seg[w][lane] = s;
  __syncthreads();
  if (w == 0 && h < d.H) {
    F t = 0;
#pragma unroll
    for (int k = 0; k < kCsSegs; ++k) t += seg[k][lane];
    ((F *)a.gv)[h] = t;
  }
}

// ------------------------------------------------------------------------------------------
// host side

// Reads and checks the descriptor: the sizes multiply to R = G * M, and the innermost dims whose sizes
// multiply to M (the group) broadcast b and grad_b.
static int concat_desc(const int64_t *in, ConcatDesc *d) {
  if (!in) return PDT_E_ARG;
  d->nd = in[0]; d->R = in[1]; d->G = in[2]; d->M = in[3]; d->T = in[4]; d->H = in[5]; d->vs = in[6];
  if (d->nd < 0 || d->nd > PDT_ATTN_MAX_DIMS || d->R < 0 || d->G < 0 || d->M < 0 || d->T < 0 || d->H < 0)
    return PDT_E_ARG;
  int64_t prod = 1;
  for (int i = 0; i < PDT_ATTN_MAX_DIMS; ++i) {
    d->size[i] = i < d->nd ? in[7 + i] : 1;
    if (d->size[i] < 0) return PDT_E_ARG;
    prod *= d->size[i];
  }
  for (int s = 0; s < CSLOT; ++s) {
    const int64_t *b = in + 7 + PDT_ATTN_MAX_DIMS + kCsDescSlot[s] * (PDT_ATTN_MAX_DIMS + 2);
    for (int i = 0; i < PDT_ATTN_MAX_DIMS; ++i) d->st[s][i] = i < d->nd ? b[i] : 0;
    d->ts[s] = b[PDT_ATTN_MAX_DIMS];
    d->fs[s] = b[PDT_ATTN_MAX_DIMS + 1];
  }
  if (prod != d->R || d->G * d->M != d->R) return PDT_E_ARG;
  if (d->R == 0) return PDT_OK;
  int64_t m = 1;
  for (int i = (int)d->nd - 1; i >= 0 && m < d->M; --i) {
    m *= d->size[i];
    if (d->st[CB][i] || d->st[CGB][i]) return PDT_E_ARG;
  }
  if (m != d->M) return PDT_E_ARG;
  return PDT_OK;
}

static int concat_plan(const ConcatDesc &d, int64_t esz, ConcatPlan *p) {
  *p = ConcatPlan{};
  if (d.R == 0 || d.T == 0 || d.H == 0) return PDT_OK;
  p->hc = std::min<int64_t>(d.H, kCsChunk);
  p->hchunks = (d.H + p->hc - 1) / p->hc;
  const int64_t by_lds = kCsLdsBytes / (p->hc * esz) - 1;  // (one more row of LDS holds v's chunk)
  p->rt = std::min<int64_t>(std::min<int64_t>(kCsRows, d.M), by_lds);
  p->tiles = (d.M + p->rt - 1) / p->rt;
  p->lds_bytes = (p->rt + 1) * p->hc * esz;
  // fewer frames per workgroup when the rows cannot fill the chip
  p->fpw = kCsFrames;
  while (p->fpw > kCsMinFrames && d.G * p->tiles * ((d.T + p->fpw - 1) / p->fpw) < kCsFill) p->fpw /= 2;
  p->fblocks = (d.T + p->fpw - 1) / p->fpw;
  p->chunks = (d.T + kCsFrames - 1) / kCsFrames;
  if (d.G * p->tiles > 0x7fffffffll / p->fblocks || d.G > 0x7fffffffll / p->chunks) return PDT_E_TOO_LONG;
  if (d.R > 0x7fffffffll * kCsThreads / d.H) return PDT_E_TOO_LONG;
  p->ws_bytes = (d.G * p->chunks * d.H + (p->chunks > 1 ? p->chunks * d.R * d.H : 0)) * esz;
  return PDT_OK;
}

static int concat_prepare(const int64_t *desc, int dtype, ConcatDesc *d, ConcatPlan *p) {
  if (dtype != 0 && dtype != 1) return PDT_E_ARG;
  int rc = concat_desc(desc, d);
  if (rc != PDT_OK) return rc;
  return concat_plan(*d, dtype == 1 ? 8 : 4, p);
}

static void concat_args(ConcatArgs &a, const ConcatDesc &d, const ConcatPlan &p) {
  a.d = d;
  a.rt = p.rt; a.tiles = p.tiles; a.hc = p.hc; a.fpw = p.fpw; a.fblocks = p.fblocks; a.chunks = p.chunks;
}

template <typename F> static int concat_fwd_launch(const ConcatArgs &a, const ConcatPlan &p, hipStream_t s) {
  const dim3 grid((unsigned)(a.d.G * p.tiles * p.fblocks));
  hipLaunchKernelGGL(concat_fwd_kernel<F>, grid, dim3(kCsThreads), (size_t)p.lds_bytes, s, a);
  return (int)hipGetLastError();
}

template <typename F> static int concat_bwd_launch(const ConcatArgs &a, const ConcatPlan &p, hipStream_t s) {
  const ConcatDesc &d = a.d;
  hipLaunchKernelGGL(concat_bwd_kernel<F>, dim3((unsigned)(d.G * p.chunks)), dim3(kCsThreads), 0, s, a);
  if (p.chunks > 1) {
    const unsigned blocks = (unsigned)((d.R * d.H + kCsThreads - 1) / kCsThreads);
    hipLaunchKernelGGL(concat_ga_combine_kernel<F>, dim3(blocks), dim3(kCsThreads), 0, s, a);
  }
  const unsigned hblocks = (unsigned)((d.H + PDT_WAVE - 1) / PDT_WAVE);
  hipLaunchKernelGGL(concat_gv_combine_kernel<F>, dim3(hblocks), dim3(PDT_WAVE * kCsSegs), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace pdt

extern "C" {

int64_t pdt_concat_score_workspace_bytes(const int64_t *desc, int dtype, int kind) {
  using namespace pdt;
  if (kind != 0 && kind != 1) return -1;
  ConcatDesc d;
  ConcatPlan p;
  if (concat_prepare(desc, dtype, &d, &p) != PDT_OK) return -1;
  return kind == 1 ? p.ws_bytes : 0;
}

int pdt_concat_score_plan(const int64_t *desc, int dtype, int64_t *plan5) {
  using namespace pdt;
  if (!plan5) return PDT_E_ARG;
  ConcatDesc d;
  ConcatPlan p;
  int rc = concat_prepare(desc, dtype, &d, &p);
  if (rc != PDT_OK) return rc;
  plan5[0] = p.rt; plan5[1] = p.hchunks; plan5[2] = p.fpw; plan5[3] = p.chunks; plan5[4] = p.ws_bytes;
  return PDT_OK;
}

int pdt_concat_score(const int64_t *desc, int dtype, const void *a, const void *b, const void *v, void *e,
                     void *stream) {
  using namespace pdt;
  ConcatDesc d;
  ConcatPlan p;
  int rc = concat_prepare(desc, dtype, &d, &p);
  if (rc != PDT_OK || d.R == 0 || d.T == 0 || d.H == 0) return rc;
  if (!a || !b || !v || !e) return PDT_E_ARG;
  ConcatArgs k{};
  concat_args(k, d, p);
  k.a = a; k.b = b; k.v = v; k.e = e;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 1 ? concat_fwd_launch<double>(k, p, s) : concat_fwd_launch<float>(k, p, s);
}

int pdt_concat_score_backward(const int64_t *desc, int dtype, const void *a, const void *b, const void *v,
                              const void *grad_e, void *grad_a, void *grad_b, void *grad_v, void *workspace,
                              int64_t workspace_bytes, void *stream) {
  using namespace pdt;
  ConcatDesc d;
  ConcatPlan p;
  int rc = concat_prepare(desc, dtype, &d, &p);
  if (rc != PDT_OK || d.R == 0 || d.T == 0 || d.H == 0) return rc;
  if (!a || !b || !v || !grad_e || !grad_a || !grad_b || !grad_v) return PDT_E_ARG;
  if (!workspace || workspace_bytes < p.ws_bytes) return PDT_E_ARG;
  ConcatArgs k{};
  concat_args(k, d, p);
  k.a = a; k.b = b; k.v = v; k.ge = grad_e; k.ga = grad_a; k.gb = grad_b; k.gv = grad_v; k.ws = workspace;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 1 ? concat_bwd_launch<double>(k, p, s) : concat_bwd_launch<float>(k, p, s);
}

}  // extern "C"
