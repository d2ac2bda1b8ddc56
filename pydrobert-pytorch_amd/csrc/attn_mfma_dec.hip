// Dot-product attention forward for float32 DECODE shapes: groups of 1 to 16 rows sharing a key
// sequence (a decoder step over encoder frames, M = 1; beams sharing an utterance's keys, M = K), one wide head, D and
// Dv multiples of 16 in [64, 512].  attn_fwd_kernel scores such a group's frames one after another with eight
// cross-lane sums each and is bound by that latency; here one 16x16x4 matrix product forms the scores of sixteen
// frames for all rows of the group with no cross-lane sum.  out and lse keep their layout and meaning, so the
// unchanged attn_bwd_kernel reads them.
//
// Work split.  A workgroup of four waves owns ONE group over a span of T (all of T unless the groups alone give fewer
// than 512 workgroups: then spans of whole key blocks leave the partials that attn.hip's attn_fwd_combine_kernel<float>
// merges in span order).  T is walked in key blocks of 64 frames; wave w scores frames 16 w .. 16 w + 15 of a block.
//
// Scores, S^T (frames x rows) = K (A operand) . Q^T (B operand) on v_mfma_f32_16x16x4_f32.  The group's M rows are
// padded to the tile's 16 columns; a padded column's query is zero.  Lane l is frame l % 16 of the A operand and row
// l % 16 of the B operand, and its k slot is g = l / 16: of a chunk of sixteen features it takes 16 c + 4 g .. + 3
// and feeds element j to instruction j (the k-slot freedom of §16).  The keys go from global memory straight into
// registers, 16 bytes a chunk: a key element is used by exactly one tile, all rows of the group at once, so LDS buys
// no reuse.  Eight chunks' loads are issued before the first product, and a chunk's registers take the chunk eight
// ahead once its products are issued.  The products go to four accumulators added pairwise (shorter rounding chains).
// Q^T comes from LDS, where the group's query sits once per workgroup as [16][D + 4] floats, one ds_read_b128 a
// chunk (128 registers a lane at D = 512 is why it is not kept in registers).  Banks, §16's argument for its K tile
// unchanged: sixteen lanes a pass, rows D + 4 = 4 (D / 4 + 1) dwords apart with D / 4 + 1 odd -- sixteen different
// multiples of four, no conflict (an argument; no counter was collected).  After D / 4 instructions the lane holds
// the four scores of row l % 16 and frames 16 w + 4 g .. + 3.
//
// Softmax, float32 per row across the four waves: every wave's row maxima go through LDS, there is one new running
// maximum per row and block (every lane keeps its row's maximum and sum, all waves the same bits), and
// p = exp(s - m), exactly 0 for a masked (row, frame), goes to the LDS tile P[64 frames][16 rows] (pitch 20 floats:
// a lane group's four frames are 80 = 16 (mod 64) dwords apart, four disjoint runs of sixteen banks).  Sums and the
// rescale follow attn_fwd_kernel.
//
// Weighted sum on the vector unit: the float32 MFMA peak is the packed-FMA peak, V is read once with 16-byte loads in
// its own layout, and nothing is transposed.  The 256 threads are dealt as Dv / 4 column quads times 256 / (Dv / 4)
// frame slices (slice s takes frames s, s + slices, ... of a block); a thread accumulates M rows x 4 columns in
// registers, p read from LDS as a broadcast, skipped where it is 0.  The first sixteen frames a thread owns in a block
// (ten in the 16-row instance; all of them up to Dv = 256 resp. 160) are loaded before the block's scores are
// formed, so they are in flight across the products and the softmax.  At the end of the span the slices are added pairwise through LDS in a fixed order.
//
// Masks and skipping are §14's frame word: the workgroup ORs a 64-bit word of the frames some row attends; a block
// with none is skipped before any load; frames no row attends are never loaded (zeros take their place).  The numbers
// contract is the TILE kernels': the select comes after the product and p = 0 exactly, p = 0 is never multiplied, so
// a non-finite key or value in a frame that one row masks and another attends leaves the masking row finite; an
// all-masked row is NaN with lse (-inf, -inf); no float atomics, the same bits run to run.
#include "attn_mfma.hpp"
#include "switches.hpp"

#include <algorithm>
#include <cmath>

namespace pdt {

constexpr int kDecKAhead = 8;            // key chunks (sixteen features) a lane loads at once

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x4 dec_fma(float p, f32x4 v, f32x4 acc) {
  const f32x4 p4 = {p, p, p, p};
  return __builtin_elementwise_fma(p4, v, acc);
}

// MR: the rows a thread of the weighted sum holds accumulators for (4, 8 or 16: the least that covers M)
template <int MR> __global__ __launch_bounds__(kMfmaThreads, 2) void attn_mfma_dec_fwd_kernel(AttnArgs a) {
  constexpr int kDecVAhead = MR == 16 ? 10 : 16;  // value frames a thread loads ahead (256 VGPRs hold no more at MR = 16)
  extern __shared__ __align__(16) unsigned char mfma_dec_smem[];
  __shared__ unsigned long long fany[3];  // frames of a key block some row attends (block it: slot it % 3)
  __shared__ int64_t roff[kDecRows][3], kvoff[2];  // a row's query, mask and out offsets; the group's key and value
  __shared__ __align__(16) float wmax[4][kDecRows], wsum[4][kDecRows], wfirst[4][kDecRows], ralpha[kDecRows];
  __shared__ float rfinal[2][kDecRows];  // the span's maximum and sum per row (words nothing reads inside the walk)
  const AttnDesc &d = a.d;
  const int M = (int)d.M, D = (int)d.D, Dv = (int)d.Dv, qpitch = D + kDecQPad;
  float *ps = reinterpret_cast<float *>(mfma_dec_smem);  // P [64][20]
  float *qs = ps + kDecPFloats;                          // Q [16][D + 4], then the slices' sums
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const bool live = col < M;
  const int64_t g = blockIdx.x;
  const int64_t t_begin = (int64_t)blockIdx.y * a.span, t_end = min(d.T, t_begin + a.span);
  const int64_t kts = d.ts[SK], vts = d.ts[SV], mts = d.ts[SM];
  const float scale = (float)a.scale;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // the weighted sum's deal: column quad cq, frame slice sl of ns
  const int nq = Dv / 4, ns = kMfmaThreads / nq, cq = tid % nq, sl = tid / nq;
  const bool vact = sl < ns;
  const int64_t vstep = ns * d.ts[SV];

  if (tid < kDecRows) {
    int64_t off[NSLOT];
    attn_row_offsets(d, g * d.M + min(tid, M - 1), off);  // (a padded column takes the last row's offsets, unread)
    roff[tid][0] = off[SQ];
    roff[tid][1] = off[SM];
    roff[tid][2] = off[SO];
    if (tid == 0) {
      kvoff[0] = off[SK];
      kvoff[1] = off[SV];
      fany[0] = 0;
    }
  }
  __syncthreads();
  {  // the group's query -> LDS, zero rows behind the M-th
    const int dq = D / 4;
    for (int i = tid; i < kDecRows * dq; i += kMfmaThreads) {
      const int r = i / dq, c4 = i - r * dq;
      *reinterpret_cast<f32x4 *>(qs + r * qpitch + 4 * c4) =
          r < M ? *reinterpret_cast<const f32x4 *>((const float *)a.q + roff[r][0] + 4 * c4) : zero4;
    }
  }
  const float *k = (const float *)a.k + kvoff[0], *v = (const float *)a.v + kvoff[1];
  const uint8_t *mk = a.mask ? a.mask + roff[col][1] : nullptr;
  const float *qrow = qs + col * qpitch + 4 * grp;

  f32x4 acc[MR];
#pragma unroll
  for (int r = 0; r < MR; ++r) acc[r] = zero4;
  float m_run = -PDT_INF, l_run = 0.f;  // of row col: the same bits in every lane that holds the row

  int it = 0;
  for (int64_t t0 = t_begin; t0 < t_end; t0 += kMfmaFrames, ++it) {
    // which of the lane's four (row, frame) pairs are attended: bit i is frame 16 wave + 4 grp + i
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t t = t0 + 16 * wave + 4 * grp + i;
      bool ok = live && t < t_end;
      if (ok && mk) ok = mk[t * mts] != 0;
      bits |= ok ? 1u << i : 0u;
    }
    {
      unsigned any = bits;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) any |= (unsigned)__shfl_xor((int)any, o);
      if (tid == 0) fany[(it + 1) % 3] = 0;  // (read last at block it - 2, before the barrier of block it - 1)
      if (col == 0 && any) atomicOr(&fany[it % 3], (unsigned long long)any << (16 * wave + 4 * grp));
    }
    __syncthreads();  // (also: the query is in LDS, and every thread is done with the previous block's P)
    const unsigned long long fa = fany[it % 3];
    if (fa == 0) continue;  // no row attends these frames: keys and values stay unread

    // the lane's key frame, chunks 0 .. 7, then the thread's first value frames: all issued before a product
    const bool kon = (fa >> (16 * wave + col)) & 1;
    const float *kp = k + (t0 + 16 * wave + col) * kts + 4 * grp;
    f32x4 kf[kDecKAhead];
#pragma unroll
    for (int c = 0; c < kDecKAhead; ++c)
      kf[c] = kon && 16 * c < D ? *reinterpret_cast<const f32x4 *>(kp + 16 * c) : zero4;
    // (the thread's frame i of the block is block frame sl + ns i, vstep i elements further; fnext's bit 0 says
    // whether the next one to load is attended, and shifting runs it out to 0 behind the block)
    const float *vp = v + (t0 + sl) * vts + 4 * cq;
    const unsigned long long fmine = vact ? fa >> sl : 0ull;
    unsigned long long fnext = fmine;
    f32x4 vr[kDecVAhead];
#pragma unroll
    for (int i = 0; i < kDecVAhead; ++i) {
      vr[i] = fnext & 1 ? *reinterpret_cast<const f32x4 *>(vp) : zero4;
      vp += vstep;
      fnext >>= ns;
    }

    // S^T = K Q^T: D / 4 instructions; a chunk's registers take the chunk eight ahead as soon
    // as its four products are issued, so eight loads a lane stay in flight along the row
    // (four accumulators, chunk c into c % 4, added pairwise: chains a quarter as long over sums half as large
    // keep the scores' rounding error near that of the backward's tree sum, which rebuilds them -- DESIGN.md §18)
    f32x4 sa[4] = {zero4, zero4, zero4, zero4};
    const int nc = D / 16;
    for (int c0 = 0; c0 < nc; c0 += kDecKAhead) {
#pragma unroll
      for (int c = 0; c < kDecKAhead; ++c) {
        if (c0 + c < nc) {
          const f32x4 qf = *reinterpret_cast<const f32x4 *>(qrow + 16 * (c0 + c));
#pragma unroll
          for (int j = 0; j < 4; ++j) sa[c % 4] = mfma_16x16x4(kf[c][j], qf[j], sa[c % 4]);
          if (c0 + c + kDecKAhead < nc)
            kf[c] = kon ? *reinterpret_cast<const f32x4 *>(kp + 16 * (c0 + c + kDecKAhead)) : zero4;
        }
      }
    }

    const f32x4 s = (sa[0] + sa[1]) + (sa[2] + sa[3]);
    // online softmax of row col: the wave's maximum over its sixteen frames, then the block's through LDS
    float x[4], mx = -PDT_INF;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[i] = (bits >> i) & 1u ? s[i] * scale : -PDT_INF;
      mx = fmaxf(mx, x[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (grp == 0) wmax[wave][col] = mx;
    __syncthreads();
    const float m_new = fmaxf(fmaxf(m_run, fmaxf(wmax[0][col], wmax[1][col])), fmaxf(wmax[2][col], wmax[3][col]));
    const float alpha = m_new == -PDT_INF ? 1.f : (m_run == -PDT_INF ? 0.f : expf(m_run - m_new));
    float p[4], psum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = x[i] == -PDT_INF ? 0.f : expf(x[i] - m_new);
      psum += p[i];
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    if (grp == 0) wfirst[wave][col] = psum;
    __syncthreads();
    // The backward rebuilds a = exp((s - max) - log sum) from scores summed in ITS order (attn.hip: lane l adds
    // features l, l + 64, .., then wave_sum).  Where a frame carries an eighth or more of its row's sum so far, a
    // last-place difference between that s and the product above would reach the gradients whole (a row that attends
    // one frame has a = 1 exactly only if the two agree to the bit), so such a score -- eight a row and block at
    // the most, none in a flat row -- is summed again here in that very order, the wave's lanes across D.
    {
      const float lsofar = l_run * alpha + ((wfirst[0][col] + wfirst[1][col]) + (wfirst[2][col] + wfirst[3][col]));
      bool redone = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned long long todo = __ballot(p[i] > 0.f && p[i] >= 0.125f * lsofar);
        redone |= todo != 0;
        while (todo) {
          const int src = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const float *kr = k + (t0 + 16 * wave + 4 * (src >> 4) + i) * kts, *qr = qs + (src & 15) * qpitch;
          float sb = 0.f;
          for (int c = lane; c < D; c += PDT_WAVE) sb = __fadd_rn(sb, __fmul_rn(qr[c], kr[c]));
#pragma unroll
          for (int o = PDT_WAVE / 2; o > 0; o >>= 1) sb = __fadd_rn(sb, __shfl_xor(sb, o));
          if (lane == src) {
            x[i] = sb * scale;
            p[i] = expf(x[i] - m_new);  // (m_new stays the reference; it may lie a last place beside the maximum)
          }
        }
      }
      if (redone) {  // (wave-uniform)
        psum = (p[0] + p[1]) + (p[2] + p[3]);
        psum += __shfl_xor(psum, 16);
        psum += __shfl_xor(psum, 32);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) ps[(16 * wave + 4 * grp + i) * kDecPPitch + col] = p[i];
    if (grp == 0) wsum[wave][col] = psum;
    if (tid < kDecRows) ralpha[col] = alpha;
    __syncthreads();
    l_run = l_run * alpha + ((wsum[0][col] + wsum[1][col]) + (wsum[2][col] + wsum[3][col]));
    m_run = m_new;

    // O = alpha O + P V: the thread's frames of the block, M rows x 4 columns
    if (vact) {
#pragma unroll
      for (int rq = 0; rq < MR / 4; ++rq) {
        const f32x4 al = *reinterpret_cast<const f32x4 *>(&ralpha[4 * rq]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * rq + e] *= al[e];
      }
      // the frames in registers, then (few slices, wide Dv) the rest, each loaded kDecVAhead frames ahead of its sum
      const float *pj = ps + sl * kDecPPitch;
      for (unsigned long long fsum = fmine; fsum != 0;) {
#pragma unroll
        for (int i = 0; i < kDecVAhead; ++i) {
          if (fsum & 1) {
#pragma unroll
            for (int rq = 0; rq < MR / 4; ++rq) {
              const f32x4 p4 = *reinterpret_cast<const f32x4 *>(pj + 4 * rq);
#pragma unroll
              for (int e = 0; e < 4; ++e)  // (0 is never multiplied; a padded row's p is 0)
                if (p4[e] != 0.f) acc[4 * rq + e] = dec_fma(p4[e], vr[i], acc[4 * rq + e]);
            }
          }
          if (fnext & 1) vr[i] = *reinterpret_cast<const f32x4 *>(vp);
          vp += vstep;
          pj += ns * kDecPPitch;
          fsum >>= ns;
          fnext >>= ns;
        }
      }
    }
  }

  if (tid < kDecRows) {
    rfinal[0][col] = m_run;  // (not wsum: a late wave may still be reading the last block's sums)
    rfinal[1][col] = l_run;
  }
  __syncthreads();  // (every wave is done with the query: its LDS takes the slices' sums)
  // slices n - 1 .. h are added to slices n - h - 1 .. 0, halving n: a fixed order
  for (int n = ns; n > 1;) {
    const int h = (n + 1) / 2;
    if (vact && sl >= h && sl < n) {
#pragma unroll
      for (int r = 0; r < MR; ++r)
        if (r < M) *reinterpret_cast<f32x4 *>(qs + ((sl - h) * M + r) * Dv + 4 * cq) = acc[r];
    }
    __syncthreads();
    if (sl < n - h) {
#pragma unroll
      for (int r = 0; r < MR; ++r)
        if (r < M) acc[r] += *reinterpret_cast<const f32x4 *>(qs + (sl * M + r) * Dv + 4 * cq);
    }
    __syncthreads();
    n = h;
  }

  const int64_t row0 = g * d.M;
  if (a.splits == 1) {
    if (sl == 0) {
#pragma unroll
      for (int r = 0; r < MR; ++r)
        if (r < M)  // (0 / 0: an all-masked row is NaN)
          *reinterpret_cast<f32x4 *>((float *)a.o + roff[r][2] + 4 * cq) = acc[r] / rfinal[1][r];
    }
    if (tid < M) {
      ((float *)a.l)[row0 + tid] = rfinal[0][tid];
      ((float *)a.l)[d.R + row0 + tid] = logf(rfinal[1][tid]);
    }
  } else {
    // partials as attn_fwd_kernel leaves them: m [splits][R], l [splits][R], acc [splits][R][Dv]
    float *pm = (float *)a.ws, *pl = pm + a.splits * d.R, *pa = pl + a.splits * d.R;
    const int64_t sp = blockIdx.y;
    if (sl == 0) {
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        if (r < M) {
          float *dst = pa + (sp * d.R + row0 + r) * Dv + 4 * cq;  // (8 splits R bytes into the workspace: 8-byte stores)
          *reinterpret_cast<f32x2 *>(dst) = f32x2{acc[r][0], acc[r][1]};
          *reinterpret_cast<f32x2 *>(dst + 2) = f32x2{acc[r][2], acc[r][3]};
        }
      }
    }
    if (tid < M) {
      pm[sp * d.R + row0 + tid] = rfinal[0][tid];
      pl[sp * d.R + row0 + tid] = rfinal[1][tid];
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side

struct MfmaDecPlan {
  int64_t splits, span, ws_bytes, lds_bytes;
};

// 1: the descriptor takes the kernel above (plan filled), 0: it does not
static int attn_mfma_dec_plan(const AttnDesc &d, MfmaDecPlan *p) {
  *p = MfmaDecPlan{};
  if (!attn_mfma_dec_gate(d)) return 0;
  const int64_t frame_blocks = (d.T + kMfmaFrames - 1) / kMfmaFrames;
  // split T only when the groups cannot fill the chip, into spans of whole key blocks, and never into more partials
  // than the tile kernel's workspace holds (the allocator's figure for this descriptor stays what it is)
  const int64_t cap = attn_fwd_tile_ws_bytes(d);
  for (int64_t want = std::min<int64_t>(std::max<int64_t>(1, (kDecFill + d.G - 1) / d.G), frame_blocks);; --want) {
    p->span = (frame_blocks + want - 1) / want * kMfmaFrames;
    p->splits = (d.T + p->span - 1) / p->span;
    p->ws_bytes = p->splits == 1 ? 0 : p->splits * d.R * (d.Dv + 2) * 4;
    if (p->ws_bytes <= cap) break;  // (one span needs none)
  }
  const int64_t slices = kMfmaThreads / (d.Dv / 4);
  p->lds_bytes = 4 * (kDecPFloats + std::max<int64_t>(kDecRows * (d.D + kDecQPad), slices / 2 * d.M * d.Dv));
  if (d.G > 0x7fffffffll || p->splits > 65535) return 0;
  return 1;
}

}  // namespace pdt

extern "C" {

int pdt_attn_dot_mfma_dec_plan(const int64_t *desc, int64_t *plan) {
  using namespace pdt;
  if (!plan) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT, &d);
  if (rd != PDT_OK) return rd;
  MfmaDecPlan p;
  const int ok = switches().attn_mfma_dec != 0 ? attn_mfma_dec_plan(d, &p) : 0;
  const int64_t out[7] = {kDecRows, kDecRows, kMfmaFrames, p.splits, p.span, p.ws_bytes, p.lds_bytes};
  for (int i = 0; i < 7; ++i) plan[i] = ok ? out[i] : 0;
  return ok;
}

int pdt_attn_dot_mfma_dec(const int64_t *desc, const void *query, const void *key, const void *value, const void *mask,
                          const double *scale, void *out, void *lse, void *workspace, int64_t workspace_bytes,
                          void *stream) {
  using namespace pdt;
  if (!scale) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT, &d);
  if (rd != PDT_OK) return rd;
  if (d.R > 0 && d.T == 0) return PDT_E_ARG;
  MfmaDecPlan p;
  if (!attn_mfma_dec_plan(d, &p)) return PDT_E_UNSUPPORTED;  // (an empty call too)
  if (!query || !key || !value || !out || !lse) return PDT_E_ARG;
  if (((uintptr_t)query | (uintptr_t)key | (uintptr_t)value | (uintptr_t)out) & 15) return PDT_E_ARG;
  if (workspace_bytes < p.ws_bytes || (p.ws_bytes && !workspace)) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = query; a.k = key; a.v = value; a.mask = (const uint8_t *)mask; a.o = out; a.l = lse; a.ws = workspace;
  a.scale = *scale; a.rt = kDecRows; a.tiles = 1; a.splits = p.splits; a.span = p.span;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)d.G, (unsigned)p.splits);
  const dim3 blk(kMfmaThreads);  // (dynamic LDS is under 64 KiB at every shape of the gate)
  if (d.M <= 4) hipLaunchKernelGGL(attn_mfma_dec_fwd_kernel<4>, grid, blk, (size_t)p.lds_bytes, s, a);
  else if (d.M <= 8) hipLaunchKernelGGL(attn_mfma_dec_fwd_kernel<8>, grid, blk, (size_t)p.lds_bytes, s, a);
  else hipLaunchKernelGGL(attn_mfma_dec_fwd_kernel<16>, grid, blk, (size_t)p.lds_bytes, s, a);
  if (p.splits > 1) return attn_fwd_combine_launch(a, 0, s);
  return (int)hipGetLastError();
}

}  // extern "C"
