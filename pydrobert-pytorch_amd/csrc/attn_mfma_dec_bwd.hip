// Dot-product attention backward for float32 DECODE shapes, the shapes of attn_mfma_dec.hip's forward:
// groups of 1 to 16 rows sharing a key sequence, D and Dv multiples of 16 in [64, 512].  attn_bwd_kernel scores such a
// group one frame per wave pass with eight cross-lane sums against an 8-row tile, walks a group of 9 to 16 rows twice
// with a read-modify-write of dK / dV, and needs a delta launch before it and a dQ combine behind it.  Here ONE kernel
// forms the scores and dP of sixteen frames for all rows of the group by matrix products, dK and dV by matrix products
// too, stores every dK / dV element once, and computes delta itself.  It reads only out and lse, whichever float32
// forward wrote them.  Deterministic: no atomics on floats, every sum in a fixed order.
//
// Work split (the forward's).  A workgroup of four waves owns ONE group over a span of T (all of T unless the groups
// alone give fewer than 512 workgroups: then spans of whole key blocks).  T is walked in key blocks of 64 frames; wave
// w owns frames 16 w .. 16 w + 15 of a block.  Each (group, frame) belongs to one workgroup, so dK and dV need no
// combine; dQ is summed over T, and with several spans each span leaves a partial [span][R][D] that
// attn_mfma_dec_gq_combine_kernel adds in span order.
//
// Preamble.  Q^T and dO^T of the group go to LDS as [16][D + 4] and [16][Dv + 4] floats, zero rows behind the M-th
// (the forward's layout and bank argument: rows 4 (D / 4 + 1) dwords apart with D / 4 + 1 odd, sixteen different
// multiples of four banks for the sixteen lanes of a ds_read_b128 pass).  delta_r = dO_r . O_r is summed here, wave
// w rows w, w + 4, .., in attn_delta_kernel's order (lane l adds columns l, l + 64, .., then the wave's butterfly), so
// no launch and no R floats of workspace are spent on it.
//
// Per block, two score-shaped products on v_mfma_f32_16x16x4_f32 with the forward's operand scheme: S^T (frames x
// rows) = K (A) . Q^T (B) and dP^T = V (A) . dO^T (B).  Lane l is frame l % 16 of A and row l % 16 of B, its k slot
// g = l / 16 takes features 16 c + 4 g .. + 3 of chunk c, element j in instruction j.  Key and value rows go from
// global memory straight into registers, 16 bytes a chunk, as ONE stream of D / 16 + Dv / 16 chunks with eight in
// flight, so the value's first chunks load under the key's last products.  Four accumulators per product, added
// pairwise (§18: one chain is too inaccurate at D = 512).
//
// P = exp((scale s - m) - log sum) where the mask holds, exactly 0 elsewhere by a select after the products;
// dS = P (dP - delta), selected the same way; scale multiplies dK and dQ once at their stores, as in attn_bwd_kernel.
// A score whose P comes out at 1/8 or more (eight a row at the most) is summed again in attn_bwd_kernel's order -- the
// order both forwards used for the lse this P is normalised by -- and P and dS are formed from that score: a row
// carried by one frame has P = 1 to the bit (§18 measured that a last-place difference reaches dV whole).
//
// dV and dK on the matrix cores.  P and dS go to two LDS tiles [64 frames][16 rows] (pitch 20: a lane group's four
// frames are 80 = 16 (mod 64) dwords apart).  A wave computes, for each 16-column tile, dV^T (columns x frames) =
// dO^T (A: one dword of row k, column 16 ct + l % 16 of the dO tile) . P^T (B: the lane's frame l % 16, row k, read
// once a block), k = NK g + j in instruction j with NK = MR / 4 instructions (MR = 4, 8, 16: the least that covers M).
// The accumulator is then frame l % 16, columns 16 ct + 4 g .. + 3: one 16-byte store, once per element.  dK likewise
// from Q and dS.  A frame nobody attends gets zeros by a select; a wave or block of such frames stores zeros without a
// product or a load.  Banks of the dword reads: sixteen consecutive dwords a lane group, the groups NK (D + 4) dwords
// apart: 16 (mod 64) at NK = 4 (four disjoint runs), 8 or 40 at NK = 2 and 4, 20, 36 or 52 at NK = 1 (two groups share
// half a run: two-way at the worst; an argument, no counter was collected).
//
// dQ on the vector unit, as the forward's weighted sum: the 256 threads are D / 4 column quads times 256 / (D / 4)
// frame slices, a thread holds M rows x 4 columns, dS is read from LDS as a broadcast and dS == 0 is never multiplied
// (so a non-finite key in a frame that a row masks never reaches that row), the key is read a second time (from L2)
// with 16-byte loads issued before the block's products.  At the end of the span the slices are added pairwise through
// LDS in a fixed order.
//
// Numbers contract: pdt_attn_dot_backward's own.  A masked (row, frame) adds exactly 0 everywhere; an all-masked row
// (lse -inf, delta NaN) never reaches a sum: its dQ is exactly 0; a frame no row attends has dK = dV = 0 whatever its
// key and value hold, unread; the same bits run to run.
#include "attn_mfma.hpp"
#include "switches.hpp"

#include <algorithm>
#include <cmath>

namespace pdt {

constexpr int kDecKAhead = 8;              // key / value chunks (sixteen features) a lane loads at once
constexpr int64_t kDecBwdStatic = 1024;    // an upper bound of the kernel's static LDS

__device__ __forceinline__ f32x4 dec_fma(float p, f32x4 v, f32x4 acc) {
  const f32x4 p4 = {p, p, p, p};
  return __builtin_elementwise_fma(p4, v, acc);
}

// MR: the rows a thread of the dQ sum holds accumulators for, and four times the k-steps of the dK / dV products
template <int MR> __global__ __launch_bounds__(kMfmaThreads, 2) void attn_mfma_dec_bwd_kernel(AttnArgs a) {
  constexpr int NK = MR / 4;
  constexpr int kAhead = MR == 16 ? 6 : MR == 8 ? 10 : 12;  // key frames a thread of the dQ sum loads ahead
  extern __shared__ __align__(16) unsigned char mfma_dec_bwd_smem[];
  __shared__ unsigned long long fany[3];  // frames of a key block some row attends (block it: slot it % 3)
  __shared__ int64_t roff[kDecRows][4], goff[4];  // a row's query, mask, out and dQ offsets; the group's K, V, dK, dV
  __shared__ float rdelta[kDecRows];
  const AttnDesc &d = a.d;
  const int M = (int)d.M, D = (int)d.D, Dv = (int)d.Dv, qpitch = D + kDecQPad, gpitch = Dv + kDecQPad;
  float *ps = reinterpret_cast<float *>(mfma_dec_bwd_smem);  // P [64][20]
  float *dss = ps + kDecPFloats;                             // dS [64][20]
  float *qs = dss + kDecPFloats;                             // Q [16][D + 4], then the slices' sums
  float *gs = qs + kDecRows * qpitch;                        // dO [16][Dv + 4]
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const bool live = col < M;
  const int64_t g = blockIdx.x, row0 = g * d.M;
  const int64_t t_begin = (int64_t)blockIdx.y * a.span, t_end = min(d.T, t_begin + a.span);
  const int64_t kts = d.ts[SK], vts = d.ts[SV], mts = d.ts[SM], gkts = d.ts[SGK], gvts = d.ts[SGV];
  const float scale = (float)a.scale;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // the dQ sum's deal: column quad cq, frame slice sl of ns
  const int nq = D / 4, ns = kMfmaThreads / nq, cq = tid % nq, sl = tid / nq;
  const bool vact = sl < ns;
  const int64_t kstep = ns * kts;

  if (tid < kDecRows) {
    int64_t off[NSLOT];
    attn_row_offsets(d, row0 + min(tid, M - 1), off);  // (a padded column takes the last row's offsets, unread)
    roff[tid][0] = off[SQ];
    roff[tid][1] = off[SM];
    roff[tid][2] = off[SO];
    roff[tid][3] = off[SGQ];
    if (tid == 0) {
      goff[0] = off[SK];
      goff[1] = off[SV];
      goff[2] = off[SGK];
      goff[3] = off[SGV];
      fany[0] = 0;
    }
  }
  __syncthreads();
  {  // the group's query and grad_out -> LDS, zero rows behind the M-th
    const int dq = D / 4, dg = Dv / 4;
    for (int i = tid; i < kDecRows * dq; i += kMfmaThreads) {
      const int r = i / dq, c4 = i - r * dq;
      *reinterpret_cast<f32x4 *>(qs + r * qpitch + 4 * c4) =
          r < M ? *reinterpret_cast<const f32x4 *>((const float *)a.q + roff[r][0] + 4 * c4) : zero4;
    }
    for (int i = tid; i < kDecRows * dg; i += kMfmaThreads) {
      const int r = i / dg, c4 = i - r * dg;
      *reinterpret_cast<f32x4 *>(gs + r * gpitch + 4 * c4) =
          r < M ? *reinterpret_cast<const f32x4 *>((const float *)a.gout + roff[r][2] + 4 * c4) : zero4;
    }
    // delta of row r in attn_delta_kernel's order (an all-masked row's out is NaN: its delta is never used)
    for (int r = wave; r < M; r += kMfmaThreads / PDT_WAVE) {
      const float *o = (const float *)a.out + roff[r][2], *go = (const float *)a.gout + roff[r][2];
      float s = 0.f;
      for (int c = lane; c < Dv; c += PDT_WAVE) s = __fadd_rn(s, __fmul_rn(o[c], go[c]));
#pragma unroll
      for (int o2 = PDT_WAVE / 2; o2 > 0; o2 >>= 1) s = __fadd_rn(s, __shfl_xor(s, o2));
      if (lane == 0) rdelta[r] = s;
    }
  }
  __syncthreads();
  const float *k = (const float *)a.k + goff[0], *v = (const float *)a.v + goff[1];
  float *gk = (float *)a.gk + goff[2], *gv = (float *)a.gv + goff[3];
  const uint8_t *mk = a.mask ? a.mask + roff[col][1] : nullptr;
  const float *qrow = qs + col * qpitch + 4 * grp, *grow = gs + col * gpitch + 4 * grp;
  const int64_t myrow = row0 + min(col, M - 1);
  const float rm = ((const float *)a.lse)[myrow], rl = ((const float *)a.lse)[d.R + myrow];
  const float delta = rdelta[min(col, M - 1)];

  f32x4 acc[MR];
#pragma unroll
  for (int r = 0; r < MR; ++r) acc[r] = zero4;

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
    __syncthreads();  // (also: every thread is done with the previous block's P and dS)
    const unsigned long long fa = fany[it % 3];
    // the lane's frame of the dK / dV tiles: frame col of the wave's sixteen, columns 16 ct + 4 grp .. + 3
    const unsigned wf = (unsigned)(fa >> (16 * wave)) & 0xffffu;
    const int64_t tf = t0 + 16 * wave + col;
    const bool inb = tf < t_end, kon = (wf >> col) & 1;
    float *gkp = gk + tf * gkts + 4 * grp, *gvp = gv + tf * gvts + 4 * grp;
    if (wf == 0) {  // nobody attends the wave's frames: zeros, and nothing of them is read (wave-uniform)
      if (inb) {
        for (int c = 0; c < Dv; c += 16) *reinterpret_cast<f32x4 *>(gvp + c) = zero4;
        for (int c = 0; c < D; c += 16) *reinterpret_cast<f32x4 *>(gkp + c) = zero4;
      }
    }
    if (fa == 0) continue;  // no row attends this block: keys and values stay unread

    // the lane's key frame and then its value frame as one stream of chunks, eight in flight; before the first
    // product the thread's first key frames of the dQ sum are issued too
    const float *kp = k + tf * kts + 4 * grp, *vp = v + tf * vts + 4 * grp;
    const int nck = D / 16, nct = nck + Dv / 16;
    f32x4 kf[kDecKAhead];
#pragma unroll
    for (int c = 0; c < kDecKAhead; ++c)  // (D >= 64: the first four chunks are the key's)
      kf[c] = !kon ? zero4 : *reinterpret_cast<const f32x4 *>(c < nck ? kp + 16 * c : vp + 16 * (c - nck));
    // (the thread's frame i of the block is block frame sl + ns i, kstep i elements further; fnext's bit 0 says
    // whether the next one to load is attended, and shifting runs it out to 0 behind the block)
    const float *kq = k + (t0 + sl) * kts + 4 * cq;
    const unsigned long long fmine = vact ? fa >> sl : 0ull;
    unsigned long long fnext = fmine;
    f32x4 kr[kAhead];
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      kr[i] = fnext & 1 ? *reinterpret_cast<const f32x4 *>(kq) : zero4;
      kq += kstep;
      fnext >>= ns;
    }

    f32x4 sa[4] = {zero4, zero4, zero4, zero4}, da[4] = {zero4, zero4, zero4, zero4};
    for (int c0 = 0; c0 < nct; c0 += kDecKAhead) {
#pragma unroll
      for (int c = 0; c < kDecKAhead; ++c) {
        const int u = c0 + c;
        if (u < nct) {
          if (u < nck) {
            const f32x4 qf = *reinterpret_cast<const f32x4 *>(qrow + 16 * u);
#pragma unroll
            for (int j = 0; j < 4; ++j) sa[c % 4] = mfma_16x16x4(kf[c][j], qf[j], sa[c % 4]);
          } else {
            const f32x4 gf = *reinterpret_cast<const f32x4 *>(grow + 16 * (u - nck));
#pragma unroll
            for (int j = 0; j < 4; ++j) da[c % 4] = mfma_16x16x4(kf[c][j], gf[j], da[c % 4]);
          }
          const int n = u + kDecKAhead;
          if (n < nct)
            kf[c] = !kon ? zero4 : *reinterpret_cast<const f32x4 *>(n < nck ? kp + 16 * n : vp + 16 * (n - nck));
        }
      }
    }
    const f32x4 s = (sa[0] + sa[1]) + (sa[2] + sa[3]), dp = (da[0] + da[1]) + (da[2] + da[3]);

    // P of row col and the lane's four frames: selects after the products
    float p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = (bits >> i) & 1u ? expf((s[i] * scale - rm) - rl) : 0.f;
    // a score that carries an eighth of its row or more: summed again in attn_bwd_kernel's order (lane l adds features
    // l, l + 64, .., then the wave's butterfly), the wave's lanes across D -- see the head of the file
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned long long todo = __ballot(p[i] >= 0.125f);
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float *kr2 = k + (t0 + 16 * wave + 4 * (src >> 4) + i) * kts, *qr = qs + (src & 15) * qpitch;
        float sb = 0.f;
        for (int c = lane; c < D; c += PDT_WAVE) sb = __fadd_rn(sb, __fmul_rn(qr[c], kr2[c]));
#pragma unroll
        for (int o = PDT_WAVE / 2; o > 0; o >>= 1) sb = __fadd_rn(sb, __shfl_xor(sb, o));
        if (lane == src) p[i] = expf((sb * scale - rm) - rl);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = (16 * wave + 4 * grp + i) * kDecPPitch + col;
      ps[f] = p[i];
      dss[f] = (bits >> i) & 1u ? p[i] * (dp[i] - delta) : 0.f;
    }
    __syncthreads();

    // dV^T = dO^T P^T and dK^T = Q^T dS^T of the wave's sixteen frames, a 16-column tile at a time, four tiles'
    // chains interleaved; a frame nobody attends stores zeros
    if (wf != 0) {
      float pb[NK], db[NK];
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        pb[j] = ps[(16 * wave + col) * kDecPPitch + NK * grp + j];
        db[j] = dss[(16 * wave + col) * kDecPPitch + NK * grp + j];
      }
      const float *ga = gs + NK * grp * gpitch + col, *qa = qs + NK * grp * qpitch + col;
      for (int c0 = 0; c0 < Dv; c0 += 64) {
        f32x4 x[4] = {zero4, zero4, zero4, zero4};
#pragma unroll
        for (int j = 0; j < NK; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c0 + 16 * e < Dv) x[e] = mfma_16x16x4(ga[j * gpitch + c0 + 16 * e], pb[j], x[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (inb && c0 + 16 * e < Dv) *reinterpret_cast<f32x4 *>(gvp + c0 + 16 * e) = kon ? x[e] : zero4;
      }
      for (int c0 = 0; c0 < D; c0 += 64) {
        f32x4 x[4] = {zero4, zero4, zero4, zero4};
#pragma unroll
        for (int j = 0; j < NK; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c0 + 16 * e < D) x[e] = mfma_16x16x4(qa[j * qpitch + c0 + 16 * e], db[j], x[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (inb && c0 + 16 * e < D) *reinterpret_cast<f32x4 *>(gkp + c0 + 16 * e) = kon ? x[e] * scale : zero4;
      }
    }

    // dQ += dS^T K: the thread's frames of the block, M rows x 4 columns; the frames in registers, then (few slices,
    // wide D) the rest, each loaded kAhead frames ahead of its sum
    if (vact) {
      const float *dj = dss + sl * kDecPPitch;
      for (unsigned long long fsum = fmine; fsum != 0;) {
#pragma unroll
        for (int i = 0; i < kAhead; ++i) {
          if (fsum & 1) {
#pragma unroll
            for (int rq = 0; rq < MR / 4; ++rq) {
              const f32x4 d4 = *reinterpret_cast<const f32x4 *>(dj + 4 * rq);
#pragma unroll
              for (int e = 0; e < 4; ++e)  // (0 is never multiplied; a padded row's dS is 0)
                if (d4[e] != 0.f) acc[4 * rq + e] = dec_fma(d4[e], kr[i], acc[4 * rq + e]);
            }
          }
          if (fnext & 1) kr[i] = *reinterpret_cast<const f32x4 *>(kq);
          kq += kstep;
          dj += ns * kDecPPitch;
          fsum >>= ns;
          fnext >>= ns;
        }
      }
    }
  }

  __syncthreads();  // (every wave is done with the query and grad_out: their LDS takes the slices' sums)
  // slices n - 1 .. h are added to slices n - h - 1 .. 0, halving n: a fixed order
  for (int n = ns; n > 1;) {
    const int h = (n + 1) / 2;
    if (vact && sl >= h && sl < n) {
#pragma unroll
      for (int r = 0; r < MR; ++r)
        if (r < M) *reinterpret_cast<f32x4 *>(qs + ((sl - h) * M + r) * D + 4 * cq) = acc[r];
    }
    __syncthreads();
    if (sl < n - h) {
#pragma unroll
      for (int r = 0; r < MR; ++r)
        if (r < M) acc[r] += *reinterpret_cast<const f32x4 *>(qs + (sl * M + r) * D + 4 * cq);
    }
    __syncthreads();
    n = h;
  }

  if (sl == 0) {  // (an all-masked row, or a span no row attends: zeros)
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      if (r < M) {
        float *dst = a.splits == 1 ? (float *)a.gq + roff[r][3] + 4 * cq
                                   : (float *)a.ws + ((int64_t)blockIdx.y * d.R + row0 + r) * D + 4 * cq;
        *reinterpret_cast<f32x4 *>(dst) = acc[r] * scale;
      }
    }
  }
}

// dQ of a split call: the spans' partials [span][R][D] added in span order, one thread per (row, column quad)
__global__ __launch_bounds__(kMfmaThreads) void attn_mfma_dec_gq_combine_kernel(AttnArgs a) {
  const AttnDesc &d = a.d;
  const int64_t nq = d.D / 4, i = (int64_t)blockIdx.x * kMfmaThreads + threadIdx.x;
  if (i >= d.R * nq) return;
  const int64_t r = i / nq, c4 = i - r * nq;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int64_t sp = 0; sp < a.splits; ++sp)
    s += *reinterpret_cast<const f32x4 *>((const float *)a.ws + (sp * d.R + r) * d.D + 4 * c4);
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  *reinterpret_cast<f32x4 *>((float *)a.gq + off[SGQ] + 4 * c4) = s;
}

// ------------------------------------------------------------------------------------------
// host side

struct MfmaDecBwdPlan {
  int64_t splits, span, ws_bytes, lds_bytes, mr;
};

// 1: the descriptor takes the kernel above (plan filled), 0: it does not
static int attn_mfma_dec_bwd_plan(const AttnDesc &d, MfmaDecBwdPlan *p) {
  *p = MfmaDecBwdPlan{};
  if (!attn_mfma_dec_gate(d)) return 0;
  // beyond the forward's gate (which has the 16-byte loads of grad_out rows, out's layout): 16-byte stores of the
  // three gradients
  if (d.fs[SGQ] != 1 || d.fs[SGK] != 1 || d.fs[SGV] != 1 || d.ts[SGK] % 4 || d.ts[SGV] % 4) return 0;
  for (int i = 0; i < d.nd; ++i)
    if (d.st[SGQ][i] % 4 || d.st[SGK][i] % 4 || d.st[SGV][i] % 4) return 0;
  // the forward's spans: split T only when the groups cannot fill the chip, into spans of whole key blocks (the
  // partials are this plan's own workspace, so no allocator's figure caps them)
  const int64_t frame_blocks = (d.T + kMfmaFrames - 1) / kMfmaFrames;
  const int64_t want = std::min<int64_t>(std::max<int64_t>(1, (kDecFill + d.G - 1) / d.G), frame_blocks);
  p->span = (frame_blocks + want - 1) / want * kMfmaFrames;
  p->splits = (d.T + p->span - 1) / p->span;
  p->ws_bytes = p->splits == 1 ? 0 : p->splits * d.R * d.D * 4;
  const int64_t slices = kMfmaThreads / (d.D / 4);
  p->lds_bytes = 4 * (2 * kDecPFloats + std::max<int64_t>(kDecRows * (d.D + d.Dv + 2 * kDecQPad), slices / 2 * d.M * d.D));
  p->mr = d.M <= 4 ? 4 : d.M <= 8 ? 8 : 16;
  if (d.G > 0x7fffffffll || p->splits > 65535 || d.R * (d.D / 4) / kMfmaThreads >= 0x7fffffffll) return 0;
  return 1;
}

template <int MR> static int attn_mfma_dec_bwd_launch(const AttnArgs &a, const MfmaDecBwdPlan &p, hipStream_t s) {
  // (the attribute is asked for where static + dynamic LDS may pass 64 KiB: D + Dv above 888)
  const int rc = set_lds(attn_mfma_dec_bwd_kernel<MR>, (size_t)p.lds_bytes, 64 * 1024 - kDecBwdStatic);
  if (rc) return rc;
  hipLaunchKernelGGL(attn_mfma_dec_bwd_kernel<MR>, dim3((unsigned)a.d.G, (unsigned)p.splits), dim3(kMfmaThreads),
                     (size_t)p.lds_bytes, s, a);
  return 0;
}

}  // namespace pdt

extern "C" {

int pdt_attn_dot_mfma_dec_backward_plan(const int64_t *desc, int64_t *plan) {
  using namespace pdt;
  if (!plan) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT_BWD, &d);
  if (rd != PDT_OK) return rd;
  MfmaDecBwdPlan p;
  const int ok = switches().attn_mfma_dec_bwd != 0 ? attn_mfma_dec_bwd_plan(d, &p) : 0;
  const int64_t out[5] = {p.splits, p.span, p.ws_bytes, p.lds_bytes, p.mr};
  for (int i = 0; i < 5; ++i) plan[i] = ok ? out[i] : 0;
  return ok;
}

int pdt_attn_dot_mfma_dec_backward(const int64_t *desc, const void *query, const void *key, const void *value,
                                   const void *mask, const double *scale, const void *out, const void *lse,
                                   const void *grad_out, void *grad_query, void *grad_key, void *grad_value,
                                   void *workspace, int64_t workspace_bytes, void *stream) {
  using namespace pdt;
  if (!scale) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT_BWD, &d);
  if (rd != PDT_OK) return rd;
  if (d.R > 0 && d.T == 0) return PDT_E_ARG;
  MfmaDecBwdPlan p;
  if (!attn_mfma_dec_bwd_plan(d, &p)) return PDT_E_UNSUPPORTED;  // (an empty call too)
  if (!query || !key || !value || !out || !lse || !grad_out || !grad_query || !grad_key || !grad_value)
    return PDT_E_ARG;
  if (((uintptr_t)query | (uintptr_t)key | (uintptr_t)value | (uintptr_t)grad_out | (uintptr_t)grad_query |
       (uintptr_t)grad_key | (uintptr_t)grad_value) & 15)
    return PDT_E_ARG;
  if (((uintptr_t)out | (uintptr_t)lse) & 3) return PDT_E_ARG;
  if (p.ws_bytes && (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < p.ws_bytes)) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = query; a.k = key; a.v = value; a.mask = (const uint8_t *)mask; a.out = out; a.lse = lse;
  a.gout = grad_out; a.gq = grad_query; a.gk = grad_key; a.gv = grad_value; a.ws = workspace;
  a.scale = *scale; a.rt = kDecRows; a.tiles = 1; a.splits = p.splits; a.span = p.span;
  hipStream_t s = (hipStream_t)stream;
  const int rc = p.mr == 4 ? attn_mfma_dec_bwd_launch<4>(a, p, s)
                           : p.mr == 8 ? attn_mfma_dec_bwd_launch<8>(a, p, s) : attn_mfma_dec_bwd_launch<16>(a, p, s);
  if (rc) return rc;
  if (p.splits > 1) {
    const int64_t n = d.R * (d.D / 4);
    hipLaunchKernelGGL(attn_mfma_dec_gq_combine_kernel, dim3((unsigned)((n + kMfmaThreads - 1) / kMfmaThreads)),
                       dim3(kMfmaThreads), 0, s, a);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
