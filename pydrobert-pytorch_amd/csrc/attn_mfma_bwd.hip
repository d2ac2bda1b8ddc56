// Dot-product attention backward on the matrix cores, for the shapes of attn_mfma.hip's forward: two
// deterministic kernels without atomics on v_mfma_f32_16x16x32_{f16,bf16}.  Each rebuilds P and dS from lse
// (maximum and log of the sum, kept apart) and delta (attn.hip's attn_delta_kernel, the tile backward's to the bit),
// so every gradient element is summed in float32 registers by one lane, written once and rounded once; the
// workspace is delta's R floats.  Seven matrix products where a fused kernel needs five.
//
// attn_mfma_bwd_q_kernel: dQ, row-owner.  The forward's walk: a workgroup of four waves owns 64 rows of a group, a
// wave 16, one row per lane column; T is walked in key blocks of 64.  The row's query and grad_out are B fragments
// in registers for the walk.  Per block, all transposed as in the forward,
//   S^T  (frames x rows) = K (A: LDS [frame][D + 8]) . Q^T        dP^T (frames x rows) = V (A: LDS [frame][Dv + 8]) . dO^T
//   p = exp((s scale - m) - log l), ds = p (dp - delta) scale   per lane, its own row's sixteen frames
//   dQ^T (d x rows)     += K^T (A: LDS [d][64 + 8]) . dS^T (B: the lane's own ds rounded to E once)
// The B slots of dS^T are the forward's P^T slots (slot j of lane group g of product kk is frame
// 32 kk + 16 (j / 4) + 4 g + j % 4) and K^T is written and read the way the forward does V^T.
//
// attn_mfma_bwd_kv_kernel: dK and dV, frame-owner, the mirror image.  A workgroup owns 64 frames of one group, a
// wave 16, one frame per lane column, key and value as B fragments in registers; the group's M rows are walked in
// blocks of 64.  Per row block Q, Q^T, dO, dO^T go to LDS, the rows' m, log l, delta and offsets too;
//   S  (rows x frames) = Q (A: LDS [row][D + 8]) . K^T            dP (rows x frames) = dO (A: LDS [row][Dv + 8]) . V^T
//   dV^T (dv x frames) += dO^T (A: LDS [dv][72]) . P              dK^T (d x frames) += Q^T (A: LDS [d][72]) . dS
// with the same slot order over rows.
//
// Masks.  A lane reads the mask bytes of its own sixteen (row, frame) pairs; rows beyond M, frames beyond T and
// masked pairs count as masked and get p = 0, ds = 0 by a select AFTER the products (an all-masked row's
// lse = -inf, delta = NaN never reach a sum).  A block pair nobody attends is skipped before anything of it is
// loaded.  In the q kernel frames no row of the block attends go to LDS as zeros, unread; the kv kernel reads its
// own frames' keys and values regardless, and a frame nobody attends gets gradients of exactly 0 whatever they
// hold.  Deviation (the reference's result): a non-finite key in a frame that some rows of a 64-row block attend
// reaches the rows that mask it as 0 * inf = NaN in dQ, a non-finite query or grad_out the same in dK / dV.
#include "attn_mfma.hpp"
#include "switches.hpp"

#include <algorithm>
#include <cmath>

namespace pdt {

// A tile that goes to LDS both as it is ([row][pitch]) and transposed ([column][72]) is moved in units of two
// consecutive rows' 16 bytes: unit i is the row pair i % 32 and one chunk of eight columns.  Row pairs 8..15 and
// 24..31 take the neighbouring chunk of the pair (2 j, 2 j + 1) that the two half waves cover together (chunks
// per row are even), which keeps both writes free of bank conflicts.
__device__ __forceinline__ void pair_unit(int i, int &rp, int &c) {
  rp = i & 31;
  c = (i >> 5) ^ ((rp >> 3) & 1);
}

__device__ __forceinline__ void pair_store(const u32x4 (&r)[2][2], int tid, int n, unsigned short *plain, int pitch,
                                           unsigned short *trans) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = tid + u * kMfmaThreads;
    if (i < n) {
      int rp, c;
      pair_unit(i, rp, c);
#pragma unroll
      for (int h = 0; h < 2; ++h) *reinterpret_cast<u32x4 *>(plain + (2 * rp + h) * pitch + 8 * c) = r[u][h];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned x = r[u][0][e >> 1], y = r[u][1][e >> 1];
        const unsigned w = e & 1 ? (x >> 16) | (y & 0xffff0000u) : (x & 0xffffu) | (y << 16);
        *reinterpret_cast<unsigned *>(trans + (8 * c + e) * kMfmaVtPitch + 2 * rp) = w;
      }
    }
  }
}

// the A fragment of a transposed tile: row `r`, the eight k slots of lane group grp of product kk
__device__ __forceinline__ u32x4 trans_frag(const unsigned short *trans, int r, int kk, int grp) {
  const unsigned short *p = trans + r * kMfmaVtPitch + 32 * kk + 4 * grp;
  const u32x2 lo = *reinterpret_cast<const u32x2 *>(p), hi = *reinterpret_cast<const u32x2 *>(p + 16);
  return u32x4{lo[0], lo[1], hi[0], hi[1]};
}

// sixteen float32 of the accumulator layout (four tiles x four) as two B fragments, rounded to E once
template <typename E> __device__ __forceinline__ void pack_frags(const f32x4 (&x)[4], u32x4 (&f)[2]) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    f[kk] = u32x4{pack2<E>(x[2 * kk][0], x[2 * kk][1]), pack2<E>(x[2 * kk][2], x[2 * kk][3]),
                  pack2<E>(x[2 * kk + 1][0], x[2 * kk + 1][1]), pack2<E>(x[2 * kk + 1][2], x[2 * kk + 1][3])};
}

template <typename E> __global__ __launch_bounds__(kMfmaThreads) void attn_mfma_bwd_q_kernel(AttnArgs a) {
  extern __shared__ __align__(16) unsigned char mfma_bwd_smem[];
  __shared__ unsigned long long fany[3];  // frames of a key block some row attends (block it: slot it % 3)
  const AttnDesc &d = a.d;
  const int D = (int)d.D, Dv = (int)d.Dv, kpitch = D + kMfmaPad, vpitch = Dv + kMfmaPad;
  unsigned short *ks = reinterpret_cast<unsigned short *>(mfma_bwd_smem);  // [64][D + 8]
  unsigned short *kt = ks + kMfmaFrames * kpitch;                          // [D][72]
  unsigned short *vs = kt + D * kMfmaVtPitch;                              // [64][Dv + 8]
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const int64_t g = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int64_t m_row = tile * kMfmaRows + wave * kMfmaWaveRows + col;
  const bool live = m_row < d.M;
  const int64_t r = g * d.M + (live ? m_row : d.M - 1);  // (an idle lane takes the group's last row's offsets)
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  const unsigned short *q = (const unsigned short *)a.q + off[SQ];
  const unsigned short *go = (const unsigned short *)a.gout + off[SO];
  const unsigned short *k = (const unsigned short *)a.k + off[SK];  // (the same for every row of the group)
  const unsigned short *v = (const unsigned short *)a.v + off[SV];
  const uint8_t *mk = a.mask ? a.mask + off[SM] : nullptr;
  const int64_t kts = d.ts[SK], vts = d.ts[SV], mts = d.ts[SM];
  const float scale = (float)a.scale;
  const float rm = ((const float *)a.lse)[r], rl = ((const float *)a.lse)[d.R + r], delta = ((const float *)a.ws)[r];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // the row's query and grad_out as B fragments: column 32 s + 8 grp .. + 7 (beyond D / Dv: zeros)
  u32x4 qf[kMfmaMaxD / 32], gf[kMfmaMaxD / 32];
#pragma unroll
  for (int s = 0; s < kMfmaMaxD / 32; ++s) {
    const int c = 32 * s + 8 * grp;
    qf[s] = live && c < D ? *reinterpret_cast<const u32x4 *>(q + c) : zero4;
    gf[s] = live && c < Dv ? *reinterpret_cast<const u32x4 *>(go + c) : zero4;
  }
  f32x4 acc[kMfmaMaxD / 16];
#pragma unroll
  for (int t = 0; t < kMfmaMaxD / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tid == 0) fany[0] = 0;
  __syncthreads();
  int it = 0;
  for (int64_t t0 = 0; t0 < d.T; t0 += kMfmaFrames, ++it) {
    // which of the lane's sixteen (row, frame) pairs are attended: bit 4 ft + i is frame 16 ft + 4 grp + i
    unsigned bits = 0;
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t t = t0 + 16 * ft + 4 * grp + i;
        bool ok = live && t < d.T;
        if (ok && mk) ok = mk[t * mts] != 0;
        bits |= ok ? 1u << (4 * ft + i) : 0u;
      }
    {
      unsigned any = bits;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) any |= (unsigned)__shfl_xor((int)any, o);
      if (tid == 0) fany[(it + 1) % 3] = 0;  // (read last at block it - 2, before the barrier of block it - 1)
      if (col == 0 && any) {
        unsigned long long w = 0;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) w |= (unsigned long long)((any >> (4 * ft)) & 15u) << (16 * ft + 4 * grp);
        atomicOr(&fany[it % 3], w);
      }
    }
    __syncthreads();  // (also: every wave is done with the previous block's LDS tiles)
    const unsigned long long fa = fany[it % 3];
    if (fa == 0) continue;  // no row of the block attends these frames: keys and values stay unread

    // keys -> LDS both ways, values -> LDS as they are; every global load is issued before the first LDS write
    {
      const int kn = (kMfmaFrames / 2) * (D >> 3);       // (frame pair, chunk) units
      const int vc = Dv >> 3, vn = kMfmaFrames * vc;     // 16-byte chunks per frame, per block
      u32x4 kr[2][2], vr[4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + u * kMfmaThreads;
        int fp, c;
        pair_unit(i, fp, c);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int f = 2 * fp + h;
          kr[u][h] = i < kn && ((fa >> f) & 1) ? *reinterpret_cast<const u32x4 *>(k + (t0 + f) * kts + 8 * c) : zero4;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * kMfmaThreads, f = i / vc, c = i - f * vc;
        vr[u] = i < vn && ((fa >> f) & 1) ? *reinterpret_cast<const u32x4 *>(v + (t0 + f) * vts + 8 * c) : zero4;
      }
      pair_store(kr, tid, kn, ks, kpitch, kt);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * kMfmaThreads, f = i / vc, c = i - f * vc;
        if (i < vn) *reinterpret_cast<u32x4 *>(vs + f * vpitch + 8 * c) = vr[u];
      }
    }
    __syncthreads();

    // S^T = K Q^T and dP^T = V dO^T: four frame tiles of 16, the wave's 16 rows
    f32x4 s[4], dp[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) {
      s[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c0 = 0; c0 < kMfmaMaxD; c0 += 32) {
        const int c = c0 + 8 * grp;
        if (c0 < D) {
          const u32x4 kf = c < D ? *reinterpret_cast<const u32x4 *>(ks + (16 * ft + col) * kpitch + c) : zero4;
          s[ft] = mfma_16x16x32(E{}, kf, qf[c0 / 32], s[ft]);
        }
        if (c0 < Dv) {
          const u32x4 vf = c < Dv ? *reinterpret_cast<const u32x4 *>(vs + (16 * ft + col) * vpitch + c) : zero4;
          dp[ft] = mfma_16x16x32(E{}, vf, gf[c0 / 32], dp[ft]);
        }
      }
    }
    // dS of the lane's row: a select after the products, so nothing of a masked pair reaches a sum
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __expf((s[ft][i] * scale - rm) - rl);  // (score - maximum first: exact near a large |max|)
        const float x = p * (dp[ft][i] - delta) * scale;
        s[ft][i] = (bits >> (4 * ft + i)) & 1u ? x : 0.f;
      }
    u32x4 dsf[2];
    pack_frags<E>(s, dsf);
    // dQ^T += K^T dS^T
#pragma unroll
    for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
      if (16 * dt < D) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) acc[dt] = mfma_16x16x32(E{}, trans_frag(kt, 16 * dt + col, kk, grp), dsf[kk], acc[dt]);
      }
    }
  }

  if (!live) return;
  unsigned short *gq = (unsigned short *)a.gq + off[SGQ];
#pragma unroll
  for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
    if (16 * dt < D)
      *reinterpret_cast<u32x2 *>(gq + 16 * dt + 4 * grp) =
          u32x2{pack2<E>(acc[dt][0], acc[dt][1]), pack2<E>(acc[dt][2], acc[dt][3])};
  }
}

template <typename E> __global__ __launch_bounds__(kMfmaThreads) void attn_mfma_bwd_kv_kernel(AttnArgs a) {
  extern __shared__ __align__(16) unsigned char mfma_bwd_smem[];
  __shared__ unsigned rany[3];  // does any frame of the workgroup attend a row of the block (block it: slot it % 3)
  // the rows of a block, two blocks deep (block it: slot it % 2): maximum, log of the sum, delta and the element
  // offsets of query, grad_out and mask
  __shared__ __align__(16) float rs_m[2][kMfmaRows];
  __shared__ __align__(16) float rs_l[2][kMfmaRows];
  __shared__ __align__(16) float rs_d[2][kMfmaRows];
  __shared__ int64_t ro_q[2][kMfmaRows], ro_g[2][kMfmaRows], ro_m[2][kMfmaRows];
  const AttnDesc &d = a.d;
  const int D = (int)d.D, Dv = (int)d.Dv, qpitch = D + kMfmaPad, gpitch = Dv + kMfmaPad;
  unsigned short *qs = reinterpret_cast<unsigned short *>(mfma_bwd_smem);  // [64][D + 8]
  unsigned short *qt = qs + kMfmaRows * qpitch;                            // [D][72]
  unsigned short *gs = qt + D * kMfmaVtPitch;                              // [64][Dv + 8]
  unsigned short *gt = gs + kMfmaRows * gpitch;                            // [Dv][72]
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const int64_t g = blockIdx.x / a.splits, t = (blockIdx.x % a.splits) * kMfmaFrames + wave * kMfmaWaveRows + col;
  const bool live = t < d.T;
  int64_t off[NSLOT];
  attn_row_offsets(d, g * d.M, off);  // (key, value and their gradients: the same for every row of the group)
  const int64_t tc = live ? t : d.T - 1, mts = d.ts[SM];
  const unsigned short *k = (const unsigned short *)a.k + off[SK] + tc * d.ts[SK];
  const unsigned short *v = (const unsigned short *)a.v + off[SV] + tc * d.ts[SV];
  const unsigned short *q = (const unsigned short *)a.q, *go = (const unsigned short *)a.gout;
  const float *lse = (const float *)a.lse, *delta = (const float *)a.ws;
  const float scale = (float)a.scale;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // the frame's key and value as B fragments: column 32 s + 8 grp .. + 7 (beyond D / Dv: zeros)
  u32x4 kf[kMfmaMaxD / 32], vf[kMfmaMaxD / 32];
#pragma unroll
  for (int s = 0; s < kMfmaMaxD / 32; ++s) {
    const int c = 32 * s + 8 * grp;
    kf[s] = live && c < D ? *reinterpret_cast<const u32x4 *>(k + c) : zero4;
    vf[s] = live && c < Dv ? *reinterpret_cast<const u32x4 *>(v + c) : zero4;
  }
  f32x4 acck[kMfmaMaxD / 16], accv[kMfmaMaxD / 16];
#pragma unroll
  for (int i = 0; i < kMfmaMaxD / 16; ++i) acck[i] = accv[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (tid == 0) rany[0] = 0;
  int it = 0;
  for (int64_t m0 = 0; m0 < d.M; m0 += kMfmaRows, ++it) {
    const int par = it & 1;
    if (tid < kMfmaRows) {  // (a row beyond M takes the group's last row's: it is masked everywhere and loads zeros)
      const int64_t r = g * d.M + min(m0 + tid, d.M - 1);
      int64_t ro[NSLOT];
      attn_row_offsets(d, r, ro);
      ro_q[par][tid] = ro[SQ];
      ro_g[par][tid] = ro[SO];
      ro_m[par][tid] = ro[SM];
      rs_m[par][tid] = lse[r];
      rs_l[par][tid] = lse[d.R + r];
      rs_d[par][tid] = delta[r];
    }
    if (tid == 0) rany[(it + 1) % 3] = 0;  // (read last at block it - 2, before the barriers of block it - 1)
    __syncthreads();                        // (also: every wave is done with the previous block's LDS tiles)
    // which of the lane's sixteen (row, frame) pairs are attended: bit 4 rt + i is row 16 rt + 4 grp + i
    unsigned bits = 0;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * rt + 4 * grp + i;
        bool ok = live && m0 + row < d.M;
        if (ok && a.mask) ok = a.mask[ro_m[par][row] + t * mts] != 0;
        bits |= ok ? 1u << (4 * rt + i) : 0u;
      }
    if (__any(bits != 0) && lane == 0) atomicOr(&rany[it % 3], 1u);
    __syncthreads();
    if (rany[it % 3] == 0) continue;  // no frame of the workgroup attends these rows: nothing of them is loaded

    // queries and grad_out -> LDS both ways (rows beyond M: zeros); every global load before the first LDS write
    {
      const int qn = (kMfmaRows / 2) * (D >> 3), gn = (kMfmaRows / 2) * (Dv >> 3);  // (row pair, chunk) units
      u32x4 qr[2][2], gr[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + u * kMfmaThreads;
        int rp, c;
        pair_unit(i, rp, c);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int row = 2 * rp + h;
          const bool in = m0 + row < d.M;
          qr[u][h] = in && i < qn ? *reinterpret_cast<const u32x4 *>(q + ro_q[par][row] + 8 * c) : zero4;
          gr[u][h] = in && i < gn ? *reinterpret_cast<const u32x4 *>(go + ro_g[par][row] + 8 * c) : zero4;
        }
      }
      pair_store(qr, tid, qn, qs, qpitch, qt);
      pair_store(gr, tid, gn, gs, gpitch, gt);
    }
    __syncthreads();

    // S = Q K^T and dP = dO V^T: four row tiles of 16, the wave's 16 frames
    f32x4 s[4], dp[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      s[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c0 = 0; c0 < kMfmaMaxD; c0 += 32) {
        const int c = c0 + 8 * grp;
        if (c0 < D) {
          const u32x4 x = c < D ? *reinterpret_cast<const u32x4 *>(qs + (16 * rt + col) * qpitch + c) : zero4;
          s[rt] = mfma_16x16x32(E{}, x, kf[c0 / 32], s[rt]);
        }
        if (c0 < Dv) {
          const u32x4 x = c < Dv ? *reinterpret_cast<const u32x4 *>(gs + (16 * rt + col) * gpitch + c) : zero4;
          dp[rt] = mfma_16x16x32(E{}, x, vf[c0 / 32], dp[rt]);
        }
      }
    }
    // P and dS of the lane's frame: selects after the products
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const int row = 16 * rt + 4 * grp;
      const f32x4 rm = *reinterpret_cast<const f32x4 *>(&rs_m[par][row]);
      const f32x4 rl = *reinterpret_cast<const f32x4 *>(&rs_l[par][row]);
      const f32x4 rd = *reinterpret_cast<const f32x4 *>(&rs_d[par][row]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = (bits >> (4 * rt + i)) & 1u;
        const float p = __expf((s[rt][i] * scale - rm[i]) - rl[i]);
        const float x = p * (dp[rt][i] - rd[i]) * scale;
        s[rt][i] = ok ? p : 0.f;
        dp[rt][i] = ok ? x : 0.f;
      }
    }
    u32x4 pf[2], dsf[2];
    pack_frags<E>(s, pf);
    pack_frags<E>(dp, dsf);
    // dV^T += dO^T P and dK^T += Q^T dS
#pragma unroll
    for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (16 * dt < Dv) accv[dt] = mfma_16x16x32(E{}, trans_frag(gt, 16 * dt + col, kk, grp), pf[kk], accv[dt]);
        if (16 * dt < D) acck[dt] = mfma_16x16x32(E{}, trans_frag(qt, 16 * dt + col, kk, grp), dsf[kk], acck[dt]);
      }
    }
  }

  if (!live) return;
  unsigned short *gk = (unsigned short *)a.gk + off[SGK] + t * d.ts[SGK];
  unsigned short *gv = (unsigned short *)a.gv + off[SGV] + t * d.ts[SGV];
#pragma unroll
  for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
    if (16 * dt < D)
      *reinterpret_cast<u32x2 *>(gk + 16 * dt + 4 * grp) =
          u32x2{pack2<E>(acck[dt][0], acck[dt][1]), pack2<E>(acck[dt][2], acck[dt][3])};
    if (16 * dt < Dv)
      *reinterpret_cast<u32x2 *>(gv + 16 * dt + 4 * grp) =
          u32x2{pack2<E>(accv[dt][0], accv[dt][1]), pack2<E>(accv[dt][2], accv[dt][3])};
  }
}

// ------------------------------------------------------------------------------------------
// host side

struct MfmaBwdPlan {
  int64_t tiles, frame_blocks, ws_bytes, lds_q, lds_kv;
};

// 1: the descriptor takes the kernels above (plan filled), 0: it does not
static int attn_mfma_bwd_plan(const AttnDesc &d, int elem, MfmaBwdPlan *p) {
  *p = MfmaBwdPlan{};
  if (!attn_mfma_gate(d, elem)) return 0;
  // beyond the forward's gate: 16-byte loads of grad_out rows (out's layout), 8-byte stores of the gradients
  if (d.fs[SGQ] != 1 || d.fs[SGK] != 1 || d.fs[SGV] != 1 || d.ts[SGK] % 4 || d.ts[SGV] % 4) return 0;
  for (int i = 0; i < d.nd; ++i)
    if (d.st[SO][i] % 8 || d.st[SGQ][i] % 4 || d.st[SGK][i] % 4 || d.st[SGV][i] % 4) return 0;
  p->tiles = (d.M + kMfmaRows - 1) / kMfmaRows;
  p->frame_blocks = (d.T + kMfmaFrames - 1) / kMfmaFrames;
  p->ws_bytes = 4 * d.R;
  p->lds_q = (kMfmaFrames * (d.D + kMfmaPad) + d.D * kMfmaVtPitch + kMfmaFrames * (d.Dv + kMfmaPad)) * 2;
  p->lds_kv = (kMfmaRows * (d.D + kMfmaPad) + d.D * kMfmaVtPitch + kMfmaRows * (d.Dv + kMfmaPad) +
               d.Dv * kMfmaVtPitch) * 2;
  if (d.G * p->tiles > 0x7fffffffll || d.G * p->frame_blocks > 0x7fffffffll) return 0;
  return 1;
}

template <typename E> static int attn_mfma_bwd_launch(AttnArgs &a, const MfmaBwdPlan &p, int elem, hipStream_t s) {
  int rc = set_lds(attn_mfma_bwd_q_kernel<E>, (size_t)p.lds_q);
  if (rc) return rc;
  rc = set_lds(attn_mfma_bwd_kv_kernel<E>, (size_t)p.lds_kv);
  if (rc) return rc;
  rc = attn_delta_launch(a, elem, s);
  if (rc) return rc;
  a.tiles = p.tiles;
  a.splits = p.frame_blocks;
  hipLaunchKernelGGL(attn_mfma_bwd_q_kernel<E>, dim3((unsigned)(a.d.G * p.tiles)), dim3(kMfmaThreads), (size_t)p.lds_q,
                     s, a);
  hipLaunchKernelGGL(attn_mfma_bwd_kv_kernel<E>, dim3((unsigned)(a.d.G * p.frame_blocks)), dim3(kMfmaThreads),
                     (size_t)p.lds_kv, s, a);
  return (int)hipGetLastError();
}

}  // namespace pdt

extern "C" {

int pdt_attn_dot_mfma_backward_plan(const int64_t *desc, int elem, int64_t *plan) {
  using namespace pdt;
  const int rc = elem_status(elem);
  if (rc != PDT_OK) return rc;
  if (!plan) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT_BWD, &d);
  if (rd != PDT_OK) return rd;
  MfmaBwdPlan p;
  const int ok = switches().attn_mfma_bwd != 0 ? attn_mfma_bwd_plan(d, elem, &p) : 0;
  const int64_t out[5] = {kMfmaRows, kMfmaFrames, p.ws_bytes, p.lds_q, p.lds_kv};
  for (int i = 0; i < 5; ++i) plan[i] = ok ? out[i] : 0;
  return ok;
}

int pdt_attn_dot_mfma_backward_elem(const int64_t *desc, int elem, const void *query, const void *key,
                                    const void *value, const void *mask, const double *scale, const void *out,
                                    const void *lse, const void *grad_out, void *grad_query, void *grad_key,
                                    void *grad_value, void *workspace, int64_t workspace_bytes, void *stream) {
  using namespace pdt;
  const int rc = elem_status(elem);
  if (rc != PDT_OK) return rc;
  if (!scale) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT_BWD, &d);
  if (rd != PDT_OK) return rd;
  if (d.R > 0 && d.T == 0) return PDT_E_ARG;
  MfmaBwdPlan p;
  if (!attn_mfma_bwd_plan(d, elem, &p)) return PDT_E_UNSUPPORTED;  // (float32 included; an empty call too)
  if (!query || !key || !value || !out || !lse || !grad_out || !grad_query || !grad_key || !grad_value || !workspace)
    return PDT_E_ARG;
  if (((uintptr_t)query | (uintptr_t)key | (uintptr_t)value | (uintptr_t)grad_out) & 15) return PDT_E_ARG;
  if (((uintptr_t)grad_query | (uintptr_t)grad_key | (uintptr_t)grad_value) & 7) return PDT_E_ARG;
  if (((uintptr_t)lse | (uintptr_t)workspace) & 3) return PDT_E_ARG;
  if (workspace_bytes < p.ws_bytes) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = query; a.k = key; a.v = value; a.mask = (const uint8_t *)mask; a.out = out; a.lse = lse;
  a.gout = grad_out; a.gq = grad_query; a.gk = grad_key; a.gv = grad_value; a.ws = workspace;
  a.scale = *scale; a.rt = kMfmaRows;
  hipStream_t s = (hipStream_t)stream;
  return elem == 2 ? attn_mfma_bwd_launch<f16_t>(a, p, elem, s) : attn_mfma_bwd_launch<bf16_t>(a, p, elem, s);
}

}  // extern "C"
