// Dot-product attention backward on the matrix cores for float32 self-attention shapes, the shapes
// of attn_mfma_f32.hip's forward: two deterministic kernels without atomics on v_mfma_f32_16x16x4_f32, §15's plan in
// float32.  Each rebuilds P and dS from lse (maximum and log of the sum, kept apart) and delta (attn.hip's
// attn_delta_kernel<float>, the tile backward's to the bit), so every gradient element is summed in float32 by one
// lane and stored exactly once; the workspace is delta's R floats.  P and dS are never rounded and never moved.
//
// Operands.  An instruction takes ONE float32 per lane and operand: lane l gives A[l % 16][k = l / 16] and
// B[k = l / 16][l % 16] and holds column l % 16, rows 4 (l / 16) .. + 3 of the 16x16 accumulator.  The k slots are
// dealt as in §16: of a chunk of sixteen, lane group g = l / 16 takes element 4 g + j in instruction j.  For a
// product that sums over a tile's COLUMNS (d or dv) a lane's four A values are one ds_read_b128 of the tile's row
// l % 16; for a product that sums over the tile's ROWS (frames or rows) the A value of instruction j is one dword of
// row 4 g + j, column l % 16 of the SAME untransposed tile -- the forward's V read -- so no tile has a second,
// transposed copy in LDS, and the B value is the lane's own accumulator register of the product before.
//
// attn_mfma_f32_bwd_q_kernel: dQ, row-owner.  A workgroup of four waves owns 64 rows of a group, a wave 16, one row
// per lane column; T is walked in key blocks of 64.  The row's query and grad_out are B values in registers for the
// walk (16-byte global loads), its m, log l and delta three scalars.  Per block
//   S^T  (frames x rows) = K (A: LDS [frame][D + 4], b128) . Q^T      dP^T (frames x rows) = V (A: LDS [frame][Dv + 4], b128) . dO^T
//   p = exp((s scale - m) - log l), ds = p (dp - delta) scale          per lane, frames 16 ft + 4 g + i of its row
//   dQ^T (d x rows) += K^T (A: K[16 ft + 4 g + j][16 dt + col], one dword) . dS^T (B: the lane's own ds[ft][j])
//
// attn_mfma_f32_bwd_kv_kernel: dK and dV, frame-owner, the mirror image.  A workgroup owns 64 frames of a group, a
// wave 16, one frame per lane column, key and value as B values in registers; the group's M rows are walked in blocks
// of 64.  Per row block Q [row][D + 4] and dO [row][Dv + 4] go to LDS, the rows' m, log l, delta and offsets too;
//   S  (rows x frames) = Q (A: b128) . K^T                             dP (rows x frames) = dO (A: b128) . V^T
//   dV^T (dv x frames) += dO^T (A: dO[16 rt + 4 g + j][16 dt + col]) . P     dK^T (d x frames) += Q^T (A: Q[..][16 dt + col]) . dS
//
// LDS.  Dynamic: 256 (D + Dv + 8) bytes in both kernels (66 KiB at D = Dv = 128, at most 62 KiB otherwise); the kv
// kernel adds 4624 static bytes of row statistics (2 x 64 x (3 floats + 3 int64) + the flags), the q kernel 32.
// Banks (64 of 4 bytes; an argument, no counter was collected).  b128 reads: sixteen lanes a pass, rows D + 4 =
// 4 (D / 4 + 1) dwords apart with D / 4 + 1 odd: sixteen different multiples of four banks.  Dword reads: a lane
// group reads sixteen consecutive dwords, the four groups rows 4 g + j, 4 g (D + 4) = 16 g (mod 64) dwords apart:
// four disjoint runs of sixteen banks.  Writes: 16 bytes per lane, the sixteen lanes of a pass the consecutive chunks
// of ONE row, 64 consecutive dwords or fewer.  The kv kernel's statistics are read 16 bytes per lane at dword
// 16 rt + 4 g, one address per lane group (a broadcast) four banks wide: no conflict.
//
// Registers.  Global loads are staged tile by tile (the K or Q tile goes to LDS before the V or dO tile is loaded),
// which halves the staging registers; see §17 for the figures.
//
// Masks, skipping and exact zeros are §15's: a lane reads the mask bytes of its own sixteen pairs; rows beyond M and
// frames beyond T count as masked; p = 0 and ds = 0 by a select AFTER the products (an all-masked row's lse = -inf
// and delta = NaN never reach a sum: its dQ is exactly 0); an empty block pair is skipped before anything of it is
// loaded; in the q kernel frames no row of the block attends go to LDS as zeros, unread; a frame nobody attends has
// dK and dV exactly 0 whatever it holds.  Deviation (the reference's result): a non-finite key in a frame that some
// rows of a 64-row block attend reaches the rows that mask it as 0 * inf = NaN in dQ, a non-finite query or grad_out
// the same in dK / dV.
#include "attn_mfma.hpp"
#include "switches.hpp"

#include <algorithm>
#include <cmath>

namespace pdt {

constexpr int kMfmaF32BwdPad = 4;  // floats of padding per LDS row (every tile)
// static LDS of the kv kernel: the row statistics and offsets two blocks deep, and the three flags
constexpr int64_t kMfmaF32BwdKvStatic = 2 * kMfmaRows * (3 * 4 + 3 * 8) + 16;

// 64 rows of `width` floats -> LDS [row][width + 4] in 16-byte chunks: sixteen lanes take the chunks cl + 16 h of one
// row, the sixteen such rows of the workgroup rows fr + 16 e.  src(row) is the row's first element, or null for a row
// that goes in as zeros, unread.  Every global load is issued before the first LDS write.
template <typename Src> __device__ __forceinline__ void tile_to_lds(float *tile, int width, int tid, Src src) {
  const int cl = tid & 15, fr = tid >> 4, pitch = width + kMfmaF32BwdPad;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 r[4][2];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float *p = src(fr + 16 * e);
#pragma unroll
    for (int h = 0; h < 2; ++h)
      r[e][h] = p && 4 * cl + 64 * h < width ? *reinterpret_cast<const f32x4 *>(p + 4 * cl + 64 * h) : zero4;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (4 * cl + 64 * h < width) *reinterpret_cast<f32x4 *>(tile + (fr + 16 * e) * pitch + 4 * cl + 64 * h) = r[e][h];
}

// x (16-tiles x lane columns) += tile (A: rows 16 i + col, b128 reads over its columns) . b (B: chunks of sixteen)
__device__ __forceinline__ void rows_dot(const float *tile, int width, int col, int grp,
                                         const f32x4 (&b)[kMfmaMaxD / 16], f32x4 (&x)[4]) {
  const int pitch = width + kMfmaF32BwdPad;
#pragma unroll
  for (int c = 0; c < kMfmaMaxD / 16; ++c) {
    if (16 * c < width) {
      f32x4 af[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const f32x4 *>(tile + (16 * i + col) * pitch + 16 * c + 4 * grp);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = mfma_16x16x4(af[i][j], b[c][j], x[i]);
    }
  }
}

// acc (column tiles x lane columns) += tile^T (A: one dword, row 16 i + 4 grp + j, column 16 dt + col) . b (B: the
// lane's own b[i][j]); instruction (i, j) sums rows 16 i + 4 g + j of the four lane groups g
__device__ __forceinline__ void cols_dot(const float *tile, int width, int col, int grp, const f32x4 (&b)[4],
                                         f32x4 (&acc)[kMfmaMaxD / 16]) {
  const int pitch = width + kMfmaF32BwdPad;
#pragma unroll
  for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
    if (16 * dt < width) {
      const float *p = tile + (4 * grp) * pitch + 16 * dt + col;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[dt] = mfma_16x16x4(p[(16 * i + j) * pitch], b[i][j], acc[dt]);
    }
  }
}

__global__ __launch_bounds__(kMfmaThreads, 2) void attn_mfma_f32_bwd_q_kernel(AttnArgs a) {
  extern __shared__ __align__(16) unsigned char mfma_f32_bwd_smem[];
  __shared__ unsigned long long fany[3];  // frames of a key block some row attends (block it: slot it % 3)
  const AttnDesc &d = a.d;
  const int D = (int)d.D, Dv = (int)d.Dv;
  float *ks = reinterpret_cast<float *>(mfma_f32_bwd_smem);    // [64][D + 4]
  float *vs = ks + kMfmaFrames * (D + kMfmaF32BwdPad);         // [64][Dv + 4]
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const int64_t g = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int64_t m_row = tile * kMfmaRows + wave * kMfmaWaveRows + col;
  const bool live = m_row < d.M;
  const int64_t r = g * d.M + (live ? m_row : d.M - 1);  // (an idle lane takes the group's last row's offsets)
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  const float *q = (const float *)a.q + off[SQ];
  const float *go = (const float *)a.gout + off[SO];
  const float *k = (const float *)a.k + off[SK];  // (the same for every row of the group)
  const float *v = (const float *)a.v + off[SV];
  const uint8_t *mk = a.mask ? a.mask + off[SM] : nullptr;
  const int64_t kts = d.ts[SK], vts = d.ts[SV], mts = d.ts[SM];
  const float scale = (float)a.scale;
  const float rm = ((const float *)a.lse)[r], rl = ((const float *)a.lse)[d.R + r], delta = ((const float *)a.ws)[r];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // the row's query and grad_out as B values: chunk c holds columns 16 c + 4 grp .. + 3 (beyond D / Dv: zeros)
  f32x4 qf[kMfmaMaxD / 16], gf[kMfmaMaxD / 16], acc[kMfmaMaxD / 16];
#pragma unroll
  for (int c = 0; c < kMfmaMaxD / 16; ++c) {
    qf[c] = live && 16 * c < D ? *reinterpret_cast<const f32x4 *>(q + 16 * c + 4 * grp) : zero4;
    gf[c] = live && 16 * c < Dv ? *reinterpret_cast<const f32x4 *>(go + 16 * c + 4 * grp) : zero4;
    acc[c] = zero4;
  }

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

    // keys, then values -> LDS as they are; frames no row attends (those beyond T among them) as zeros, unread
    tile_to_lds(ks, D, tid, [&](int f) { return (fa >> f) & 1 ? k + (t0 + f) * kts : nullptr; });
    tile_to_lds(vs, Dv, tid, [&](int f) { return (fa >> f) & 1 ? v + (t0 + f) * vts : nullptr; });
    __syncthreads();

    // S^T = K Q^T and dP^T = V dO^T: four frame tiles of 16, the wave's 16 rows
    f32x4 s[4], dp[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) s[ft] = dp[ft] = zero4;
    rows_dot(ks, D, col, grp, qf, s);
    rows_dot(vs, Dv, col, grp, gf, dp);
    // dS of the lane's row: a select after the products, so nothing of a masked pair reaches a sum
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __expf((s[ft][i] * scale - rm) - rl);  // (score - maximum first: exact near a large |max|)
        const float x = p * (dp[ft][i] - delta) * scale;
        s[ft][i] = (bits >> (4 * ft + i)) & 1u ? x : 0.f;
      }
    // dQ^T += K^T dS^T
    cols_dot(ks, D, col, grp, s, acc);
  }

  if (!live) return;
  float *gq = (float *)a.gq + off[SGQ];
#pragma unroll
  for (int dt = 0; dt < kMfmaMaxD / 16; ++dt)
    if (16 * dt < D) *reinterpret_cast<f32x4 *>(gq + 16 * dt + 4 * grp) = acc[dt];
}

__global__ __launch_bounds__(kMfmaThreads, 2) void attn_mfma_f32_bwd_kv_kernel(AttnArgs a) {
  extern __shared__ __align__(16) unsigned char mfma_f32_bwd_smem[];
  __shared__ unsigned rany[3];  // does any frame of the workgroup attend a row of the block (block it: slot it % 3)
  // the rows of a block, two blocks deep (block it: slot it % 2): maximum, log of the sum, delta and the element
  // offsets of query, grad_out and mask
  __shared__ __align__(16) float rs_m[2][kMfmaRows];
  __shared__ __align__(16) float rs_l[2][kMfmaRows];
  __shared__ __align__(16) float rs_d[2][kMfmaRows];
  __shared__ int64_t ro_q[2][kMfmaRows], ro_g[2][kMfmaRows], ro_m[2][kMfmaRows];
  const AttnDesc &d = a.d;
  const int D = (int)d.D, Dv = (int)d.Dv;
  float *qs = reinterpret_cast<float *>(mfma_f32_bwd_smem);  // [64][D + 4]
  float *gs = qs + kMfmaRows * (D + kMfmaF32BwdPad);         // [64][Dv + 4]
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const int64_t g = blockIdx.x / a.splits, t = (blockIdx.x % a.splits) * kMfmaFrames + wave * kMfmaWaveRows + col;
  const bool live = t < d.T;
  int64_t off[NSLOT];
  attn_row_offsets(d, g * d.M, off);  // (key, value and their gradients: the same for every row of the group)
  const int64_t tc = live ? t : d.T - 1, mts = d.ts[SM];
  const float *k = (const float *)a.k + off[SK] + tc * d.ts[SK];
  const float *v = (const float *)a.v + off[SV] + tc * d.ts[SV];
  const float *q = (const float *)a.q, *go = (const float *)a.gout;
  const float *lse = (const float *)a.lse, *delta = (const float *)a.ws;
  const float scale = (float)a.scale;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // the frame's key and value as B values: chunk c holds columns 16 c + 4 grp .. + 3 (beyond D / Dv: zeros)
  f32x4 kf[kMfmaMaxD / 16], vf[kMfmaMaxD / 16], acck[kMfmaMaxD / 16], accv[kMfmaMaxD / 16];
#pragma unroll
  for (int c = 0; c < kMfmaMaxD / 16; ++c) {
    kf[c] = live && 16 * c < D ? *reinterpret_cast<const f32x4 *>(k + 16 * c + 4 * grp) : zero4;
    vf[c] = live && 16 * c < Dv ? *reinterpret_cast<const f32x4 *>(v + 16 * c + 4 * grp) : zero4;
    acck[c] = accv[c] = zero4;
  }

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

    // queries, then grad_out -> LDS as they are (rows beyond M: zeros)
    tile_to_lds(qs, D, tid, [&](int row) { return m0 + row < d.M ? q + ro_q[par][row] : nullptr; });
    tile_to_lds(gs, Dv, tid, [&](int row) { return m0 + row < d.M ? go + ro_g[par][row] : nullptr; });
    __syncthreads();

    // S = Q K^T and dP = dO V^T: four row tiles of 16, the wave's 16 frames
    f32x4 s[4], dp[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) s[rt] = dp[rt] = zero4;
    rows_dot(qs, D, col, grp, kf, s);
    rows_dot(gs, Dv, col, grp, vf, dp);
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
    // dV^T += dO^T P and dK^T += Q^T dS
    cols_dot(gs, Dv, col, grp, s, accv);
    cols_dot(qs, D, col, grp, dp, acck);
  }

  if (!live) return;
  float *gk = (float *)a.gk + off[SGK] + t * d.ts[SGK];
  float *gv = (float *)a.gv + off[SGV] + t * d.ts[SGV];
#pragma unroll
  for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
    if (16 * dt < D) *reinterpret_cast<f32x4 *>(gk + 16 * dt + 4 * grp) = acck[dt];
    if (16 * dt < Dv) *reinterpret_cast<f32x4 *>(gv + 16 * dt + 4 * grp) = accv[dt];
  }
}

// ------------------------------------------------------------------------------------------
// host side

struct MfmaF32BwdPlan {
  int64_t tiles, frame_blocks, ws_bytes, lds_q, lds_kv;
};

// 1: the descriptor takes the kernels above (plan filled), 0: it does not
static int attn_mfma_f32_bwd_plan(const AttnDesc &d, MfmaF32BwdPlan *p) {
  *p = MfmaF32BwdPlan{};
  if (!attn_mfma_f32_gate(d)) return 0;
  // beyond the forward's gate: 16-byte loads of grad_out rows (out's layout: in the gate), 16-byte stores of the
  // gradients
  if (d.fs[SGQ] != 1 || d.fs[SGK] != 1 || d.fs[SGV] != 1 || d.ts[SGK] % 4 || d.ts[SGV] % 4) return 0;
  for (int i = 0; i < d.nd; ++i)
    if (d.st[SO][i] % 4 || d.st[SGQ][i] % 4 || d.st[SGK][i] % 4 || d.st[SGV][i] % 4) return 0;
  p->tiles = (d.M + kMfmaRows - 1) / kMfmaRows;
  p->frame_blocks = (d.T + kMfmaFrames - 1) / kMfmaFrames;
  p->ws_bytes = 4 * d.R;
  p->lds_q = p->lds_kv = kMfmaFrames * (d.D + d.Dv + 2 * kMfmaF32BwdPad) * 4;
  if (d.G * p->tiles > 0x7fffffffll || d.G * p->frame_blocks > 0x7fffffffll) return 0;
  return 1;
}

}  // namespace pdt

extern "C" {

int pdt_attn_dot_mfma_f32_backward_plan(const int64_t *desc, int64_t *plan) {
  using namespace pdt;
  if (!plan) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT_BWD, &d);
  if (rd != PDT_OK) return rd;
  MfmaF32BwdPlan p;
  const int ok = switches().attn_mfma_f32_bwd != 0 ? attn_mfma_f32_bwd_plan(d, &p) : 0;
  const int64_t out[5] = {kMfmaRows, kMfmaFrames, p.ws_bytes, p.lds_q, p.lds_kv};
  for (int i = 0; i < 5; ++i) plan[i] = ok ? out[i] : 0;
  return ok;
}

int pdt_attn_dot_mfma_f32_backward(const int64_t *desc, const void *query, const void *key, const void *value,
                                   const void *mask, const double *scale, const void *out, const void *lse,
                                   const void *grad_out, void *grad_query, void *grad_key, void *grad_value,
                                   void *workspace, int64_t workspace_bytes, void *stream) {
  using namespace pdt;
  if (!scale) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT_BWD, &d);
  if (rd != PDT_OK) return rd;
  if (d.R > 0 && d.T == 0) return PDT_E_ARG;
  MfmaF32BwdPlan p;
  if (!attn_mfma_f32_bwd_plan(d, &p)) return PDT_E_UNSUPPORTED;  // (an empty call too: no rows of 64)
  if (!query || !key || !value || !out || !lse || !grad_out || !grad_query || !grad_key || !grad_value || !workspace)
    return PDT_E_ARG;
  if (((uintptr_t)query | (uintptr_t)key | (uintptr_t)value | (uintptr_t)grad_out | (uintptr_t)grad_query |
       (uintptr_t)grad_key | (uintptr_t)grad_value) & 15)
    return PDT_E_ARG;
  if (((uintptr_t)lse | (uintptr_t)workspace) & 3) return PDT_E_ARG;
  if (workspace_bytes < p.ws_bytes) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = query; a.k = key; a.v = value; a.mask = (const uint8_t *)mask; a.out = out; a.lse = lse;
  a.gout = grad_out; a.gq = grad_query; a.gk = grad_key; a.gv = grad_value; a.ws = workspace;
  a.scale = *scale; a.rt = kMfmaRows; a.tiles = p.tiles; a.splits = p.frame_blocks;
  hipStream_t s = (hipStream_t)stream;
  // (the attribute is asked for where static + dynamic LDS pass 64 KiB)
  int rc = set_lds(attn_mfma_f32_bwd_q_kernel, (size_t)p.lds_q, 64 * 1024 - 32);
  if (rc) return rc;
  rc = set_lds(attn_mfma_f32_bwd_kv_kernel, (size_t)p.lds_kv, 64 * 1024 - kMfmaF32BwdKvStatic);
  if (rc) return rc;
  rc = attn_delta_launch(a, 0, s);
  if (rc) return rc;
  hipLaunchKernelGGL(attn_mfma_f32_bwd_q_kernel, dim3((unsigned)(d.G * p.tiles)), dim3(kMfmaThreads), (size_t)p.lds_q, s,
                     a);
  hipLaunchKernelGGL(attn_mfma_f32_bwd_kv_kernel, dim3((unsigned)(d.G * p.frame_blocks)), dim3(kMfmaThreads),
                     (size_t)p.lds_kv, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
