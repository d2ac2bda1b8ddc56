// Dot-product attention forward on the matrix cores for float32 self-attention shapes: groups of 64
// or more rows, head dims D, Dv that are multiples of 16 in [32, 128].  A flash-attention walk of its own on
// v_mfma_f32_16x16x4_f32: products and sums are float32, so P is never rounded and the result stays inside the
// float32 bound of attn_fwd_kernel.  The backward that reads this out and lse is attn_mfma_f32_bwd.hip (§17).
//
// Work split (that of attn_mfma.hip, §14, so plans, partials and the combine are shared).  A workgroup of four waves
// owns 64 consecutive rows of one group, a wave 16 of them, over a span of T (all of T unless groups x row blocks
// cannot fill the chip: then spans leave the partials that attn.hip's attn_fwd_combine_kernel<float> merges).  T is
// walked in key blocks of 64 frames.
//
// Products.  Both are formed TRANSPOSED, so a query row lives in one lane column for the whole walk:
//   S^T (frames x rows) = K (A operand: frames x d, from LDS) . Q^T (B operand: d x rows, in registers for the walk)
//   O^T (dv x rows)    += V^T (A operand: dv x frames, from LDS) . P^T (B operand: frames x rows, registers)
// An instruction takes ONE float32 per lane and operand: lane l gives A[l % 16][k = l / 16] and B[k = l / 16][l % 16]
// and holds column l % 16 (the query row), rows 4 (l / 16) .. + 3 of the 16x16 accumulator.  The product sums over
// the k slots whatever their order, so the slots are dealt to make the loads wide: of a chunk of sixteen d, lane
// group g = l / 16 takes element 4 g + j in instruction j.  A lane's four A values of K are then one ds_read_b128,
// its four B values of Q one 16-byte global load kept for the walk (D / 4 registers).  After the four frame tiles of
// a block the lane holds sixteen scores of its own row, frames 16 ft + 4 g + i: in the second product lane group g
// supplies frame 16 ft + 4 g + j in instruction (ft, j) -- its own p, straight from the accumulator register, never
// rounded, never moved -- and V is read in that same order.
//
// LDS.  K block as [frame][D + 4] floats, V block as [frame][Dv + 4] floats (NOT transposed: the A operand of the
// second product is one dword per lane, sixteen consecutive dv of one frame per lane group).  256 (D + Dv + 8)
// bytes: 66 KiB at D = Dv = 128 (asked for through set_lds), at most 62 KiB otherwise.  Banks (64 of 4 bytes, an
// argument, no counter was collected): the K read is 16 bytes per lane, sixteen lanes a pass, rows D + 4 =
// 4 (D / 4 + 1) dwords apart with D / 4 + 1 odd: sixteen different multiples of four -- no conflict.  The V read is
// 4 bytes per lane: a lane group reads sixteen consecutive dwords, the four groups frames 4 g + j, that is
// 4 g (Dv + 4) = 16 g (mod 64) dwords apart: four disjoint runs of sixteen banks -- no conflict.  Writes of both
// tiles are 16 bytes per lane, the sixteen lanes of a pass the consecutive chunks of ONE row: 64 consecutive dwords or
// fewer -- no conflict, at every D and Dv of the gate.
//
// Masks, skipping and the non-finite deviation are those of attn_mfma.hip, word for word: the workgroup ORs a
// 64-bit word of the frames some row attends; a block with none is skipped before its keys and values are loaded;
// frames no row attends go to LDS as zeros and are never read; the select comes after the product (a non-finite key
// cannot leak) and p = 0 exactly there; a non-finite VALUE in a frame that other rows of the block attend reaches
// the rows that mask it as 0 * inf = NaN through the matrix product -- the reference's own result.
#include "attn_mfma.hpp"
#include "switches.hpp"

#include <algorithm>
#include <cmath>

namespace pdt {

constexpr int64_t kMfmaF32Fill = 512;  // workgroups wanted before T is split: two per CU
constexpr int kMfmaF32Pad = 4;         // floats of padding per LDS row (both tiles)

__global__ __launch_bounds__(kMfmaThreads, 2) void attn_mfma_f32_fwd_kernel(AttnArgs a) {
  extern __shared__ __align__(16) unsigned char mfma_f32_smem[];
  __shared__ unsigned long long fany[3];  // frames of a key block some row attends (block it: slot it % 3)
  const AttnDesc &d = a.d;
  const int D = (int)d.D, Dv = (int)d.Dv, kpitch = D + kMfmaF32Pad, vpitch = Dv + kMfmaF32Pad;
  float *ks = reinterpret_cast<float *>(mfma_f32_smem);  // [64][D + 4]
  float *vs = ks + kMfmaFrames * kpitch;                 // [64][Dv + 4]
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const int64_t g = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int64_t m_row = tile * kMfmaRows + wave * kMfmaWaveRows + col;
  const bool live = m_row < d.M;
  const int64_t r = g * d.M + (live ? m_row : d.M - 1);  // (an idle lane takes the group's last row's offsets)
  const int64_t t_begin = (int64_t)blockIdx.y * a.span, t_end = min(d.T, t_begin + a.span);
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  const float *q = (const float *)a.q + off[SQ];
  const float *k = (const float *)a.k + off[SK];  // (the same for every row of the group)
  const float *v = (const float *)a.v + off[SV];
  const uint8_t *mk = a.mask ? a.mask + off[SM] : nullptr;
  const int64_t kts = d.ts[SK], vts = d.ts[SV], mts = d.ts[SM];
  const float scale = (float)a.scale;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // the row's query as B values: chunk c holds d = 16 c + 4 grp .. + 3 (instruction j of the chunk takes [j])
  f32x4 qf[kMfmaMaxD / 16];
#pragma unroll
  for (int c = 0; c < kMfmaMaxD / 16; ++c)
    qf[c] = live && 16 * c < D ? *reinterpret_cast<const f32x4 *>(q + 16 * c + 4 * grp) : zero4;
  f32x4 acc[kMfmaMaxD / 16];
#pragma unroll
  for (int t = 0; t < kMfmaMaxD / 16; ++t) acc[t] = zero4;
  float m_run = -PDT_INF, l_run = 0.f;  // (l_run: the sum over this lane's frames only, added up at the end)

  if (tid == 0) fany[0] = 0;
  __syncthreads();
  int it = 0;
  for (int64_t t0 = t_begin; t0 < t_end; t0 += kMfmaFrames, ++it) {
    // which of the lane's sixteen (row, frame) pairs are attended: bit 4 ft + i is frame 16 ft + 4 grp + i
    unsigned bits = 0;
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t t = t0 + 16 * ft + 4 * grp + i;
        bool ok = live && t < t_end;
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

    // keys and values -> LDS as they are, 16-byte chunks: sixteen lanes take the sixteen chunks c = cl + 16 h of a
    // frame's 64 floats (half h exists where 64 h < D, a chunk where 4 c < D), the sixteen such rows of the workgroup
    // frames fr + 16 e -- 256 contiguous bytes of memory and 64 consecutive dwords of LDS per sixteen lanes; every
    // global load is issued before the first LDS write
    {
      const int cl = tid & 15, fr = tid >> 4;
      const float *kp = k + (t0 + fr) * kts + 4 * cl, *vp = v + (t0 + fr) * vts + 4 * cl;
      f32x4 kr[2][4], vr[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          kr[h][e] = 4 * cl + 64 * h < D && ((fa >> (fr + 16 * e)) & 1)
                         ? *reinterpret_cast<const f32x4 *>(kp + 16 * e * kts + 64 * h) : zero4;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          vr[h][e] = 4 * cl + 64 * h < Dv && ((fa >> (fr + 16 * e)) & 1)
                         ? *reinterpret_cast<const f32x4 *>(vp + 16 * e * vts + 64 * h) : zero4;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * cl + 64 * h < D) *reinterpret_cast<f32x4 *>(ks + (fr + 16 * e) * kpitch + 4 * cl + 64 * h) = kr[h][e];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * cl + 64 * h < Dv) *reinterpret_cast<f32x4 *>(vs + (fr + 16 * e) * vpitch + 4 * cl + 64 * h) = vr[h][e];
    }
    __syncthreads();

    // S^T = K Q^T: four frame tiles of 16, the wave's 16 rows; a chunk of sixteen d is four instructions a tile
    f32x4 s[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) s[ft] = zero4;
#pragma unroll
    for (int c = 0; c < kMfmaMaxD / 16; ++c) {
      if (16 * c < D) {
        f32x4 kf[4];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
          kf[ft] = *reinterpret_cast<const f32x4 *>(ks + (16 * ft + col) * kpitch + 16 * c + 4 * grp);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ft = 0; ft < 4; ++ft) s[ft] = mfma_16x16x4(kf[ft][j], qf[c][j], s[ft]);
      }
    }
    // online softmax of the lane's row over its sixteen frames and its three partner lanes'
    float mx = -PDT_INF;
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float x = (bits >> (4 * ft + i)) & 1u ? s[ft][i] * scale : -PDT_INF;
        s[ft][i] = x;
        mx = fmaxf(mx, x);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = m_new == -PDT_INF ? 1.f : (m_run == -PDT_INF ? 0.f : __expf(m_run - m_new));
    float psum = 0.f;
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = s[ft][i] == -PDT_INF ? 0.f : __expf(s[ft][i] - m_new);
        s[ft][i] = p;
        psum += p;
      }
    l_run = l_run * alpha + psum;
    m_run = m_new;
    // O^T = alpha O^T + V^T P^T: instruction (ft, j) sums frames 16 ft + 4 g + j of the four lane groups g
#pragma unroll
    for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
      if (16 * dt < Dv) {
        acc[dt] *= alpha;
        const float *vp = vs + (4 * grp) * vpitch + 16 * dt + col;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[dt] = mfma_16x16x4(vp[(16 * ft + j) * vpitch], s[ft][j], acc[dt]);
      }
    }
  }

  float l = l_run + __shfl_xor(l_run, 16);
  l += __shfl_xor(l, 32);
  if (!live) return;
  const int64_t row = g * d.M + m_row;
  if (a.splits == 1) {
    float *o = (float *)a.o + off[SO];
#pragma unroll
    for (int dt = 0; dt < kMfmaMaxD / 16; ++dt)
      if (16 * dt < Dv) *reinterpret_cast<f32x4 *>(o + 16 * dt + 4 * grp) = acc[dt] / l;  // (0 / 0: an all-masked row is NaN)
    if (grp == 0) {
      ((float *)a.l)[row] = m_run;
      ((float *)a.l)[d.R + row] = logf(l);
    }
  } else {
    // partials as attn_fwd_kernel leaves them: m [splits][R], l [splits][R], acc [splits][R][Dv]
    float *pm = (float *)a.ws, *pl = pm + a.splits * d.R, *pa = pl + a.splits * d.R;
    const int64_t sp = blockIdx.y;
    float *dst = pa + (sp * d.R + row) * Dv;  // (8 splits R bytes into the workspace: dword stores)
#pragma unroll
    for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
      if (16 * dt < Dv) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[16 * dt + 4 * grp + i] = acc[dt][i];
      }
    }
    if (grp == 0) {
      pm[sp * d.R + row] = m_run;
      pl[sp * d.R + row] = l;
    }
  }
}

// ------------------------------------------------------------------------------------------
// host side

struct MfmaF32Plan {
  int64_t tiles, splits, span, ws_bytes, lds_bytes;
};

// 1: the descriptor takes the kernel above (plan filled), 0: it does not
static int attn_mfma_f32_plan(const AttnDesc &d, MfmaF32Plan *p) {
  *p = MfmaF32Plan{};
  if (!attn_mfma_f32_gate(d)) return 0;
  p->tiles = (d.M + kMfmaRows - 1) / kMfmaRows;
  const int64_t blocks = d.G * p->tiles, frame_blocks = (d.T + kMfmaFrames - 1) / kMfmaFrames;
  // split T only when the rows cannot fill the chip, and never below two key blocks a span (§14's rule)
  const int64_t splits = std::min<int64_t>(std::max<int64_t>(1, (kMfmaF32Fill + blocks - 1) / blocks),
                                           std::max<int64_t>(1, frame_blocks / 2));
  p->span = (frame_blocks + splits - 1) / splits * kMfmaFrames;
  p->splits = (d.T + p->span - 1) / p->span;
  p->ws_bytes = p->splits == 1 ? 0 : p->splits * d.R * (d.Dv + 2) * 4;
  p->lds_bytes = kMfmaFrames * (d.D + d.Dv + 2 * kMfmaF32Pad) * 4;
  if (blocks > 0x7fffffffll || p->splits > 65535) return 0;
  return 1;
}

}  // namespace pdt

extern "C" {

int pdt_attn_dot_mfma_f32_plan(const int64_t *desc, int64_t *plan) {
  using namespace pdt;
  if (!plan) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT, &d);
  if (rd != PDT_OK) return rd;
  MfmaF32Plan p;
  const int ok = switches().attn_mfma_f32 != 0 ? attn_mfma_f32_plan(d, &p) : 0;
  const int64_t out[7] = {kMfmaRows, kMfmaWaveRows, kMfmaFrames, p.splits, p.span, p.ws_bytes, p.lds_bytes};
  for (int i = 0; i < 7; ++i) plan[i] = ok ? out[i] : 0;
  return ok;
}

int pdt_attn_dot_mfma_f32(const int64_t *desc, const void *query, const void *key, const void *value, const void *mask,
                          const double *scale, void *out, void *lse, void *workspace, int64_t workspace_bytes,
                          void *stream) {
  using namespace pdt;
  if (!scale) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT, &d);
  if (rd != PDT_OK) return rd;
  if (d.R > 0 && d.T == 0) return PDT_E_ARG;
  MfmaF32Plan p;
  if (!attn_mfma_f32_plan(d, &p)) return PDT_E_UNSUPPORTED;  // (an empty call too: no rows of 64)
  if (!query || !key || !value || !out || !lse) return PDT_E_ARG;
  if (((uintptr_t)query | (uintptr_t)key | (uintptr_t)value | (uintptr_t)out) & 15) return PDT_E_ARG;
  if (workspace_bytes < p.ws_bytes || (p.ws_bytes && !workspace)) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = query; a.k = key; a.v = value; a.mask = (const uint8_t *)mask; a.o = out; a.l = lse; a.ws = workspace;
  a.scale = *scale; a.rt = kMfmaRows; a.tiles = p.tiles; a.splits = p.splits; a.span = p.span;
  hipStream_t s = (hipStream_t)stream;
  const int rc = set_lds(attn_mfma_f32_fwd_kernel, (size_t)p.lds_bytes);
  if (rc) return rc;
  const dim3 grid((unsigned)(d.G * p.tiles), (unsigned)p.splits);
  hipLaunchKernelGGL(attn_mfma_f32_fwd_kernel, grid, dim3(kMfmaThreads), (size_t)p.lds_bytes, s, a);
  if (p.splits > 1) return attn_fwd_combine_launch(a, 0, s);
  return (int)hipGetLastError();
}

}  // extern "C"
