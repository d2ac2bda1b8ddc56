// Dot-product attention forward on the matrix cores, for float16 / bfloat16 self-attention shapes:
// groups of 64 or more rows, head dims D, Dv that are multiples of 16 in [32, 128].  A flash-attention walk on
// v_mfma_f32_16x16x32_{f16,bf16}; the backward that reads this out and lse is attn_mfma_bwd.hip (§15).
//
// Work split.  A workgroup of four waves owns 64 consecutive rows of one group, a wave 16 of them, over a span of
// T (all of T unless groups x row blocks cannot fill the chip: then spans leave the partials that attn.hip's
// attn_fwd_combine_kernel merges).  T is walked in key blocks of 64 frames.
//
// Products.  Both are formed TRANSPOSED, so that a query row lives in one lane column for the whole walk and P goes
// from the accumulator to the operand registers without leaving the lane:
//   S^T (frames x rows) = K (A operand: frames x d, from LDS) . Q^T (B operand: d x rows, in registers for the walk)
//   O^T (dv x rows)    += V^T (A operand: dv x frames, from LDS) . P^T (B operand: frames x rows, registers)
// In the 16x16 accumulator lane l holds column l % 16 (the query row) and rows 4 (l / 16) .. + 3; as a B operand
// it holds column l % 16 and eight k slots.  A lane's sixteen scores of a key block (four frame tiles x four) are
// all of its own row: the row's maximum and sum need two cross-lane steps (lanes l, l ^ 16, l ^ 32), the rescale
// of O^T is a per-lane scalar, and the eight k slots of P^T are filled with the lane's own p of two frame tiles --
// slot j of lane group g of product kk is frame 32 kk + 16 (j / 4) + 4 g + j % 4.  The matrix product sums over all
// (g, j) slots whatever their order, so V^T is read from LDS in that same slot order and nothing is permuted.
//
// LDS.  K block as [frame][D + 8] halves: a lane's A fragment is one 16-byte read; the row pitch is 4 (D / 8 + 1)
// dwords with D / 8 + 1 odd, so the sixteen rows a 16-lane pass reads start at sixteen different multiples of four
// of the 64 banks -- no conflict.  V block TRANSPOSED as [dv][64 + 8] halves (the A operand wants frames
// contiguous, memory has dv contiguous): a thread loads two consecutive frames' 16 bytes and writes eight dwords
// (frame pair, one dv each); writes of a wave go to 32 consecutive dwords per dv row, reads are 8-byte at pitch 36
// dwords, 36 r + 2 g covering all 64 banks over the 32 lanes of a pass -- no conflict either.  At most 35.2 KiB.
//
// Masks.  Every lane reads the mask bytes of its own sixteen (row, frame) pairs; the workgroup ORs them into a
// 64-bit word of frames some row attends.  A block with none is skipped before its keys and values are loaded, and
// inside a walked block the frames no row attends are not loaded either (zeros go to LDS): padded frames are never
// read.  A masked (row, frame) has its score replaced by -inf after the product (a non-finite key cannot leak) and
// p = 0 exactly; a non-finite VALUE in a frame that other rows of the block attend reaches the rows that mask it as
// 0 * inf = NaN through the matrix product -- the reference's own result, a deviation from the tile kernels.
#include "attn_mfma.hpp"
#include "switches.hpp"

#include <algorithm>
#include <cmath>

namespace pdt {

constexpr int64_t kMfmaFill = 512;  // workgroups wanted before T is split: two per CU

template <typename E> __global__ __launch_bounds__(kMfmaThreads) void attn_mfma_fwd_kernel(AttnArgs a) {
  extern __shared__ __align__(16) unsigned char mfma_smem[];
  __shared__ unsigned long long fany[3];  // frames of a key block some row attends (block it: slot it % 3)
  const AttnDesc &d = a.d;
  const int D = (int)d.D, Dv = (int)d.Dv, kpitch = D + kMfmaPad;
  unsigned short *ks = reinterpret_cast<unsigned short *>(mfma_smem);  // [64][D + 8]
  unsigned short *vt = ks + kMfmaFrames * kpitch;                      // [Dv][72]
  const int tid = threadIdx.x, lane = tid & (PDT_WAVE - 1), wave = tid / PDT_WAVE;
  const int col = lane & 15, grp = lane >> 4;
  const int64_t g = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int64_t m_row = tile * kMfmaRows + wave * kMfmaWaveRows + col;
  const bool live = m_row < d.M;
  const int64_t r = g * d.M + (live ? m_row : d.M - 1);  // (an idle lane takes the group's last row's offsets)
  const int64_t t_begin = (int64_t)blockIdx.y * a.span, t_end = min(d.T, t_begin + a.span);
  int64_t off[NSLOT];
  attn_row_offsets(d, r, off);
  const unsigned short *q = (const unsigned short *)a.q + off[SQ];
  const unsigned short *k = (const unsigned short *)a.k + off[SK];  // (the same for every row of the group)
  const unsigned short *v = (const unsigned short *)a.v + off[SV];
  const uint8_t *mk = a.mask ? a.mask + off[SM] : nullptr;
  const int64_t kts = d.ts[SK], vts = d.ts[SV], mts = d.ts[SM];
  const float scale = (float)a.scale;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // the row's query as B fragments: d = 32 s + 8 grp .. + 7 (beyond D: zeros, and the key fragment is zeroed too)
  u32x4 qf[kMfmaMaxD / 32];
#pragma unroll
  for (int s = 0; s < kMfmaMaxD / 32; ++s) {
    const int c = 32 * s + 8 * grp;
    qf[s] = live && c < D ? *reinterpret_cast<const u32x4 *>(q + c) : zero4;
  }
  f32x4 acc[kMfmaMaxD / 16];
#pragma unroll
  for (int t = 0; t < kMfmaMaxD / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
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

    // keys -> LDS as they are, values -> LDS transposed; every global load is issued before the first LDS write
    {
      const int kc = D >> 3, kn = kMfmaFrames * kc;  // 16-byte chunks per frame, per block
      const int vn = (kMfmaFrames / 2) * (Dv >> 3);  // (frame pair, chunk) units
      u32x4 kr[4], vr[2][2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * kMfmaThreads, f = i / kc, c = i - f * kc;
        kr[u] = i < kn && ((fa >> f) & 1) ? *reinterpret_cast<const u32x4 *>(k + (t0 + f) * kts + 8 * c) : zero4;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + u * kMfmaThreads, fp = i & 31, c = i >> 5;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int f = 2 * fp + h;
          vr[u][h] = i < vn && ((fa >> f) & 1) ? *reinterpret_cast<const u32x4 *>(v + (t0 + f) * vts + 8 * c) : zero4;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = tid + u * kMfmaThreads, f = i / kc, c = i - f * kc;
        if (i < kn) *reinterpret_cast<u32x4 *>(ks + f * kpitch + 8 * c) = kr[u];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + u * kMfmaThreads, fp = i & 31, c = i >> 5;
        if (i < vn) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const unsigned x = vr[u][0][e >> 1], y = vr[u][1][e >> 1];
            const unsigned w = e & 1 ? (x >> 16) | (y & 0xffff0000u) : (x & 0xffffu) | (y << 16);
            *reinterpret_cast<unsigned *>(vt + (8 * c + e) * kMfmaVtPitch + 2 * fp) = w;
          }
        }
      }
    }
    __syncthreads();

    // S^T = K Q^T: four frame tiles of 16, the wave's 16 rows
    f32x4 s[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) {
      s[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c0 = 0; c0 < kMfmaMaxD; c0 += 32) {
        if (c0 < D) {
          const int c = c0 + 8 * grp;
          const u32x4 kf = c < D ? *reinterpret_cast<const u32x4 *>(ks + (16 * ft + col) * kpitch + c) : zero4;
          s[ft] = mfma_16x16x32(E{}, kf, qf[c0 / 32], s[ft]);
        }
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
        psum += p;  // (the unrounded p)
      }
    l_run = l_run * alpha + psum;
    m_run = m_new;
    u32x4 pf[2];  // P^T as B fragments, rounded to E once
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      pf[kk] = u32x4{pack2<E>(s[2 * kk][0], s[2 * kk][1]), pack2<E>(s[2 * kk][2], s[2 * kk][3]),
                     pack2<E>(s[2 * kk + 1][0], s[2 * kk + 1][1]), pack2<E>(s[2 * kk + 1][2], s[2 * kk + 1][3])};
    // O^T = alpha O^T + V^T P^T
#pragma unroll
    for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
      if (16 * dt < Dv) {
        acc[dt] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const unsigned short *vp = vt + (16 * dt + col) * kMfmaVtPitch + 32 * kk + 4 * grp;
          const u32x2 lo = *reinterpret_cast<const u32x2 *>(vp), hi = *reinterpret_cast<const u32x2 *>(vp + 16);
          acc[dt] = mfma_16x16x32(E{}, u32x4{lo[0], lo[1], hi[0], hi[1]}, pf[kk], acc[dt]);
        }
      }
    }
  }

  float l = l_run + __shfl_xor(l_run, 16);
  l += __shfl_xor(l, 32);
  if (!live) return;
  const int64_t row = g * d.M + m_row;
  if (a.splits == 1) {
    unsigned short *o = (unsigned short *)a.o + off[SO];
#pragma unroll
    for (int dt = 0; dt < kMfmaMaxD / 16; ++dt) {
      if (16 * dt < Dv) {
        const f32x4 x = acc[dt] / l;  // (0 / 0: an all-masked row is NaN)
        *reinterpret_cast<u32x2 *>(o + 16 * dt + 4 * grp) = u32x2{pack2<E>(x[0], x[1]), pack2<E>(x[2], x[3])};
      }
    }
    if (grp == 0) {
      ((float *)a.l)[row] = m_run;
      ((float *)a.l)[d.R + row] = logf(l);
    }
  } else {
    // partials as attn_fwd_kernel leaves them: m [splits][R], l [splits][R], acc [splits][R][Dv]
    float *pm = (float *)a.ws, *pl = pm + a.splits * d.R, *pa = pl + a.splits * d.R;
    const int64_t sp = blockIdx.y;
    float *dst = pa + (sp * d.R + row) * Dv;
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

struct MfmaPlan {
  int64_t tiles, splits, span, ws_bytes, lds_bytes;
};

// 1: the descriptor takes the kernel above (plan filled), 0: it does not
static int attn_mfma_plan(const AttnDesc &d, int elem, MfmaPlan *p) {
  *p = MfmaPlan{};
  if (!attn_mfma_gate(d, elem)) return 0;
  p->tiles = (d.M + kMfmaRows - 1) / kMfmaRows;
  const int64_t blocks = d.G * p->tiles, frame_blocks = (d.T + kMfmaFrames - 1) / kMfmaFrames;
  // split T only when the rows cannot fill the chip, and never below two key blocks a span (a span pays for its
  // partials and for the combine pass)
  const int64_t splits = std::min<int64_t>(std::max<int64_t>(1, (kMfmaFill + blocks - 1) / blocks),
                                           std::max<int64_t>(1, frame_blocks / 2));
  p->span = (frame_blocks + splits - 1) / splits * kMfmaFrames;
  p->splits = (d.T + p->span - 1) / p->span;
  p->ws_bytes = p->splits == 1 ? 0 : p->splits * d.R * (d.Dv + 2) * 4;
  p->lds_bytes = (kMfmaFrames * (d.D + kMfmaPad) + d.Dv * kMfmaVtPitch) * 2;
  if (blocks > 0x7fffffffll || p->splits > 65535) return 0;
  return 1;
}

template <typename E> static int attn_mfma_launch(AttnArgs &a, const MfmaPlan &p, int elem, hipStream_t s) {
  int rc = set_lds(attn_mfma_fwd_kernel<E>, (size_t)p.lds_bytes);
  if (rc) return rc;
  const dim3 grid((unsigned)(a.d.G * p.tiles), (unsigned)p.splits);
  hipLaunchKernelGGL(attn_mfma_fwd_kernel<E>, grid, dim3(kMfmaThreads), (size_t)p.lds_bytes, s, a);
  if (p.splits > 1) return attn_fwd_combine_launch(a, elem, s);
  return (int)hipGetLastError();
}

}  // namespace pdt

extern "C" {

int pdt_attn_dot_mfma_plan(const int64_t *desc, int elem, int64_t *plan) {
  using namespace pdt;
  const int rc = elem_status(elem);
  if (rc != PDT_OK) return rc;
  if (!plan) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT, &d);
  if (rd != PDT_OK) return rd;
  MfmaPlan p;
  const int ok = switches().attn_mfma != 0 ? attn_mfma_plan(d, elem, &p) : 0;
  const int64_t out[7] = {kMfmaRows, kMfmaWaveRows, kMfmaFrames, p.splits, p.span, p.ws_bytes, p.lds_bytes};
  for (int i = 0; i < 7; ++i) plan[i] = ok ? out[i] : 0;
  return ok;
}

int pdt_attn_dot_mfma_elem(const int64_t *desc, int elem, const void *query, const void *key, const void *value,
                           const void *mask, const double *scale, void *out, void *lse, void *workspace,
                           int64_t workspace_bytes, void *stream) {
  using namespace pdt;
  const int rc = elem_status(elem);
  if (rc != PDT_OK) return rc;
  if (!scale) return PDT_E_ARG;
  AttnDesc d;
  const int rd = attn_desc(desc, ATTN_DOT, &d);
  if (rd != PDT_OK) return rd;
  if (d.R > 0 && d.T == 0) return PDT_E_ARG;
  MfmaPlan p;
  if (!attn_mfma_plan(d, elem, &p)) return PDT_E_UNSUPPORTED;  // (float32 included; an empty call too: no rows of 64)
  if (!query || !key || !value || !out || !lse) return PDT_E_ARG;
  if (((uintptr_t)query | (uintptr_t)key | (uintptr_t)value | (uintptr_t)out) & 15) return PDT_E_ARG;
  if (workspace_bytes < p.ws_bytes || (p.ws_bytes && !workspace)) return PDT_E_ARG;
  AttnArgs a{};
  a.d = d; a.q = query; a.k = key; a.v = value; a.mask = (const uint8_t *)mask; a.o = out; a.l = lse; a.ws = workspace;
  a.scale = *scale; a.rt = kMfmaRows; a.tiles = p.tiles; a.splits = p.splits; a.span = p.span;
  hipStream_t s = (hipStream_t)stream;
  return elem == 2 ? attn_mfma_launch<f16_t>(a, p, elem, s) : attn_mfma_launch<bf16_t>(a, p, elem, s);
}

}  // extern "C"
