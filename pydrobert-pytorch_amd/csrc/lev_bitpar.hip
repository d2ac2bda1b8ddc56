// Bit-parallel Levenshtein distances for unit costs (ins = del = sub = 1, what every uniform-cost
// call becomes after the rescaling of reference _string.py:168-174) on gfx950: the plan of a call
// (plan_bitpar), the column recurrence (lev_bitpar_kernel, lev_bitpar_staged_kernel) and its launch.
//
// The cell recurrence of _string_matching (reference _string.py:286-346) moves by -1 / 0 / +1
// between neighbouring cells, so a whole DP column is two bit-vectors of vertical deltas
// (Pv: +1, Mv: -1) and one column update costs ~20 word operations per 32 cells (Myers 1999;
// the block form with carried horizontal deltas is Hyyro 2003) instead of ~5 per cell in
// lev_skewed.hip.  Values are small integers either way: results are identical.
//
// L = 2^k >= |X| / 32 lanes per utterance, 64 / L utterances per wave (X = hyp, the bit-vector
// sequence; Y = ref, the consumed one).  Lane b owns block b (rows 32 b + 1 .. 32 b + 32) and runs
// one column behind lane b - 1, which hands it the horizontal delta of its last row through one DPP
// shift -- an anti-diagonal pipeline over blocks.  After the last reference token the vectors hold
// D[ref_len][h] - D[ref_len][h-1] for every h: all prefix distances come out of one final prefix
// sum.  (With X = hyp the transposed table is computed; unit costs make it the same table.)
//
// The match masks the recurrence reads come from classify_utterance (bitpar_classify.hpp).  Where
// the plan says `fused` (four 16-lane utterances per workgroup, Y <= 512) lev_bitpar_kernel runs it
// itself, one wave per utterance, straight into the LDS arrays the recurrence reads, and a call is
// ONE launch that never touches the workspace; every other shape, and a call that keeps or is given
// its tables (pdt_lev_keep, pdt_lev_classified), goes through lev_classify_kernel
// (bitpar_classify.hip) and lev_bitpar_staged_kernel.
//
// Optimal completion's bit-parallel kernel is oc_bitpar.hip, with the bit-vectors along the
// REFERENCE.  (A form of the hypothesis-major pipeline here that dumped every column's (Pv, Mv) words
// and searched them for the arg-min rows measured 0.48 ms against the row-synchronous kernel's 0.51;
// the reference-major kernel runs the C2 shape in 0.24 ms.)
#include <algorithm>
#include <type_traits>

#include "bitpar_classify.hpp"
#include "lev_launch.hpp"

namespace pdt {

// the recurrence kernel's ring of match words: two buffers of 16 words per lane, lane stride 20
// words (conflict-free 16-byte accesses)
constexpr int kBitparChunk = 16, kBitparLaneStride = 20;
constexpr size_t kBitparRingBytes = (size_t)2 * PDT_WAVE * kBitparLaneStride * 4;
constexpr int kFusedLensBytes = 32;  // fused lev_bitpar_kernel: (ref_len, hyp_len) of the workgroup's four utterances

// X: length of the bit-vector sequence, Y: of the consumed one.  Blocks are 32 rows and the
// presence word has 32 bits: X <= 1024.
BitparPlan plan_bitpar(int64_t X, int64_t Y, int64_t N) {
  BitparPlan p{};
  if (X > 1024 || Y > (1 << 20) || N <= 0) return p;
  int lgL = 0;
  while ((32 << lgL) < X) ++lgL;
  p.lgL = lgL;
  const size_t Xs = (size_t)(X > 0 ? X : 1), Ys = (size_t)(Y > 0 ? Y : 1);
  // classify: [(presence, offset) per class X * 8] [tokens (X + 1) * 8 (later: the mask words)]
  //           [classes of Y, 2 bytes each]
  // (the token table's region also holds the presence map of small tokens, lev_classes.hpp: at
  // least kDirectWords * 8 bytes)
  p.lds_classify = align_up(Xs * 8 + std::max((Xs + 1) * 8, (size_t)kDirectWords * 8) + Ys * 2, 16);
  // DP: per utterance [yh Y * 8] [mask words (X + 1) * 4]; per workgroup the ring of match words
  // (two chunks of kRingWords per lane), which the distances (X + 1) * 4 per utterance take over
  p.lds_sub = align_up(Ys * 8 + (Xs + 1) * 4, 16);
  int upw = 64 >> lgL;
  auto tail = [&](int u) { return align_up(std::max<size_t>((size_t)u * (Xs + 1) * 4, kBitparRingBytes), 16); };
  while (upw > 1 && p.lds_sub * upw + tail(upw) > 40 * 1024) upw >>= 1;  // (four workgroups per CU)
  if (p.lds_sub * upw + tail(upw) > 150 * 1024 || p.lds_classify * 4 > 160 * 1024) return p;
  p.upw = upw;
  p.lds_tail = tail(upw);
  // The fused form of lev_bitpar_kernel (classification inside the recurrence kernel): a 16-lane
  // utterance per wave quarter, four waves = four utterances, the classes of Y in eight registers
  // per lane, and the workgroup's LDS within the 40 KiB that keep four workgroups on a CU.  Every
  // other shape keeps the two launches.
  if (lgL == 4 && upw == 4 && Ys <= 8 * PDT_WAVE) {
    const size_t sub_f = align_up(std::max(Xs, Ys) * 8 + (Xs + 1) * 4, 16);
    if (sub_f * 4 + kFusedLensBytes + p.lds_tail <= 40 * 1024) {
      p.fused = 1;
      p.lds_sub_fused = sub_f;
    }
  }
  // The same for oc_bitpar_kernel (X = reference, 16 lanes whatever its length; Y = hypothesis).
  if (X <= 16 * 32 && Ys <= 8 * PDT_WAVE && oc_fused_lds_bytes(X, Y) <= 40 * 1024) p.oc_fused = 1;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  };
  p.off_lens = take((size_t)N * 8);
  p.off_yh = take((size_t)N * Ys * 8);
  p.off_msk = take((size_t)N * (Xs + 1) * 4);
  p.total = off;
  p.ok = 1;
  return p;
}

// ---- the column recurrence --------------------------------------------------------------------
// Two waves per workgroup: wave 1 looks the match words up one chunk of steps ahead and leaves
// them in an LDS ring, wave 0 runs the recurrence -- a lone wave issues an instruction every ~5.5
// cycles whatever it is, and the look-ups were 12 of the loop's 40 instructions per step.
//
// FUSED (plan.fused: four utterances per workgroup, X <= 512, Y <= 512): the workgroup starts with
// four waves and each classifies one of its four utterances straight into that utterance's tables
// (classify_utterance<8, kClassifyInPlace>); after one barrier waves 2 and 3 leave and waves 0 and 1 carry on as
// below.  No classification launch, no tables in the workspace, nothing to stage.  An utterance's
// region is [max(X, Y) * 8: token table, then po, then yh] [(X + 1) * 4: mask words]; the lengths of
// the four sit in the 32 bytes in front of the ring.
template <bool FUSED>
__device__ __forceinline__ void lev_bitpar_body(const BitparArgs &a, const int lds_per_sub, const int ring_off) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int L = 1 << a.lgL;
  const int sub = lane >> a.lgL, b = lane & (L - 1);
  // (FUSED: the classification's workgroup order -- its token reads are what the order is for)
  const int64_t grp = FUSED ? (int64_t)xcd_remap(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int64_t n_raw = grp * a.upw + sub;
  const bool valid = sub < a.upw && n_raw < a.N;
  const int64_t n = valid ? n_raw : grp * a.upw;  // (a safe utterance to address)
  const int X = a.X > 0 ? a.X : 1, Y = a.Y > 0 ? a.Y : 1;
  const int yh_cap = FUSED ? max(X, Y) : Y;  // entries of the region that yh shares (FUSED) or owns
  unsigned char *base = smem + (size_t)(valid ? sub : 0) * lds_per_sub;
  uint2 *yh_l = reinterpret_cast<uint2 *>(base);
  unsigned *msk_l = reinterpret_cast<unsigned *>(yh_l + yh_cap);
  unsigned *ring = reinterpret_cast<unsigned *>(smem + ring_off);
  float *bnd = reinterpret_cast<float *>(smem + ring_off) + (size_t)(valid ? sub : 0) * (X + 1);  // (after the loop)

  int ref_len, hyp_len;
  if (FUSED) {
    int32_t *lens_l = reinterpret_cast<int32_t *>(smem + ring_off - kFusedLensBytes);
    const int64_t nw = grp * 4 + wave;  // wave w classifies utterance w of the group
    if (nw < a.N) {
      unsigned char *r = smem + (size_t)wave * lds_per_sub;
      const Classified c = classify_utterance<8, kClassifyInPlace>(
          a, nw, reinterpret_cast<uint2 *>(r), reinterpret_cast<int64_t *>(r),
          reinterpret_cast<unsigned *>(r + (size_t)yh_cap * 8), nullptr, reinterpret_cast<uint2 *>(r));
      if (lane == 0) {
        lens_l[2 * wave] = c.ref_len;
        lens_l[2 * wave + 1] = c.hyp_len;
      }
    }
    __syncthreads();
    // (16 waves per CU up to here instead of 8; a wave that has ended no longer counts at a barrier,
    // so the loop's barriers below are between waves 0 and 1 as in the staged kernel)
    if (wave >= 2) return;
    ref_len = lens_l[2 * (valid ? sub : 0)];
    hyp_len = lens_l[2 * (valid ? sub : 0) + 1];
  } else {
    ref_len = a.lens[2 * n];
    hyp_len = a.lens[2 * n + 1];
  }
  int Heff = a.exclude_last ? hyp_len - 1 : hyp_len;
  if (Heff < 0) Heff = 0;
  const int x_len = valid ? Heff : 0, y_len = valid ? ref_len : 0;

  // ---- stage this utterance's lookups in LDS (eight loads in flight per lane) --------------
  if (!FUSED) {
    const uint2 *src = a.yh + n * (int64_t)Y;
    for (int j0 = b + wave * 8 * L; j0 < y_len; j0 += 16 * L) {
      uint2 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = j0 + q * L < y_len ? src[j0 + q * L] : make_uint2(0u, 0u);
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (j0 + q * L < y_len) yh_l[j0 + q * L] = v[q];
    }
    if (valid && y_len == 0 && b == 0 && wave == 0) yh_l[0] = make_uint2(0u, 0u);
    const unsigned *msrc = a.msk + n * (int64_t)(X + 1);
    for (int i0 = b + wave * 8 * L; i0 <= x_len && valid; i0 += 16 * L) {
      unsigned v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = i0 + q * L <= x_len ? msrc[i0 + q * L] : 0u;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (i0 + q * L <= x_len) msk_l[i0 + q * L] = v[q];
    }
    __syncthreads();
  }
  int ymax = y_len;
#pragma unroll
  for (int t = 1; t < PDT_WAVE; t <<= 1) ymax = max(ymax, __shfl_xor(ymax, t));
  ymax = __builtin_amdgcn_readfirstlane(ymax);
  const int nsteps = ymax > 0 ? ymax + L - 1 : 0;

  // ---- the pipeline: lane b handles Y[s - b] at step s ---------------------------------------
  // A lone wave issues a dependent instruction every ~8.5 cycles and nothing else runs on its SIMD
  // (four utterances per SIMD at the bench shape, all in this wave), so the loop is as long as its
  // instruction count: the match masks of kChunk steps are looked up first (independent LDS reads,
  // batched), then kChunk recurrence steps run out of registers.
  //
  // Steps need no guard while every lane is either working or still waiting for its first column:
  // a waiting lane sees Eq = 0 (its lookups are forced to 0) and the horizontal delta 0 its waiting
  // neighbour emits, which leaves the column-0 state (Pv = ~0, Mv = 0) as it is and emits 0 again.
  // Only the last steps (the first utterance of the wave to finish, onwards) are guarded.
  constexpr int kChunk = kBitparChunk;
  unsigned Pv = 0xffffffffu, Mv = 0u;  // column 0: D[i][0] = i
  unsigned hop = 0u, hon = 0u;         // horizontal delta of this block's last row: +1 / -1 flags
  const unsigned lowmask = (1u << b) - 1u, bbit = 1u << b;
  const int jcap = y_len > 0 ? y_len - 1 : 0;
  int ymin = (sub < a.upw && n_raw < a.N) ? y_len : (1 << 30);
#pragma unroll
  for (int t = 1; t < PDT_WAVE; t <<= 1) ymin = min(ymin, __shfl_xor(ymin, t));
  ymin = __builtin_amdgcn_readfirstlane(ymin);
  const int nfree = (ymin / kChunk) * kChunk;  // steps [0, nfree): no lane has run out of columns
  const bool row16 = a.lgL == 4;               // a DPP row is one utterance: row_shr:1 feeds +1 into b = 0
  auto lookups = [&](int s0, unsigned (&eq)[kChunk]) {
    uint2 hq[kChunk];
#pragma unroll
    for (int q = 0; q < kChunk; ++q) hq[q] = yh_l[min(max(s0 + q - b, 0), jcap)];
#pragma unroll
    for (int q = 0; q < kChunk; ++q) eq[q] = msk_l[hq[q].y + (unsigned)__popc(hq[q].x & lowmask)];
#pragma unroll
    for (int q = 0; q < kChunk; ++q) eq[q] = ((hq[q].x & bbit) && s0 + q >= b) ? eq[q] : 0u;
  };
  auto step = [&](const unsigned eq0, const unsigned hp, const unsigned hn) {
    const unsigned Xv = eq0 | Mv;
    const unsigned Eq = eq0 | hn;
    const unsigned Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    unsigned Ph = Mv | ~(Xh | Pv);
    unsigned Mh = Pv & Xh;
    hop = Ph >> 31;
    hon = Mh >> 31;
    Ph = (Ph << 1) | hp;
    Mh = (Mh << 1) | hn;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
  };
  // ROW16 form of the step: the neighbour's WHOLE Ph / Mh words travel (xp, xm; lane b = 0 of a
  // row is never written by the row shift and keeps the D[0][j] = j deltas: bit 31 of xp set, of xm
  // clear), and (Ph << 1) | (xp >> 31) is one v_alignbit -- three instructions per step less than
  // shifting the top bits out first and presetting the shift's `old` operand every step.
  unsigned xp = b == 0 ? 0x80000000u : 0u, xm = 0u, Phw = 0u, Mhw = 0u;
  auto step16 = [&](const unsigned eq0) {
    const unsigned hn = xm >> 31;
    const unsigned Xv = eq0 | Mv;
    const unsigned Eq = eq0 | hn;
    const unsigned Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    Phw = Mv | ~(Xh | Pv);
    Mhw = Pv & Xh;
    const unsigned Ph = __builtin_amdgcn_alignbit(Phw, xp, 31);
    const unsigned Mh = __builtin_amdgcn_alignbit(Mhw, xm, 31);
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
  };
  auto ring_at = [&](const int s0) {
    return reinterpret_cast<uint4 *>(ring + ((s0 / kChunk) & 1) * (PDT_WAVE * kBitparLaneStride) + lane * kBitparLaneStride);
  };
  auto sweep = [&](auto row16_tag, auto guarded_tag, const int s_begin, const int s_end) {
    constexpr bool ROW16 = decltype(row16_tag)::value, GUARDED = decltype(guarded_tag)::value;
    for (int s0 = s_begin; s0 < s_end; s0 += kChunk) {
      __syncthreads();  // chunk s0 is in the ring (and wave 1 may fill the other buffer)
      unsigned eq[kChunk];
      {
        const uint4 *src = ring_at(s0);
#pragma unroll
        for (int q = 0; q < kChunk / 4; ++q) {
          const uint4 v = src[q];
          eq[4 * q] = v.x; eq[4 * q + 1] = v.y; eq[4 * q + 2] = v.z; eq[4 * q + 3] = v.w;
        }
      }
#pragma unroll
      for (int q = 0; q < kChunk; ++q) {
        unsigned hp = 0u, hn = 0u;
        if (ROW16) {
          xp = (unsigned)__builtin_amdgcn_update_dpp((int)xp, (int)Phw, PDT_DPP_ROW_SHR(1), 0xf, 0xf, false);
          xm = (unsigned)__builtin_amdgcn_update_dpp((int)xm, (int)Mhw, PDT_DPP_ROW_SHR(1), 0xf, 0xf, false);
        } else {
          hp = (unsigned)shr1((int)hop, 0);
          hn = (unsigned)shr1((int)hon, 0);
          if (b == 0) {  // D[0][j] = j
            hp = 1u;
            hn = 0u;
          }
        }
        const int j = s0 + q - b;
        if (!GUARDED || (unsigned)j < (unsigned)y_len) {
          if (ROW16) step16(eq[q]);
          else step(eq[q], hp, hn);
        }
      }
    }
  };
  using T = std::true_type;
  using F = std::false_type;
  if (wave == 1) {  // the look-ups, one chunk ahead of the recurrence (one barrier per chunk on both sides)
    for (int s0 = 0; s0 < nsteps; s0 += kChunk) {
      unsigned eq[kChunk];
      lookups(s0, eq);
      uint4 *dst = ring_at(s0);
#pragma unroll
      for (int q = 0; q < kChunk / 4; ++q) dst[q] = make_uint4(eq[4 * q], eq[4 * q + 1], eq[4 * q + 2], eq[4 * q + 3]);
      __syncthreads();
    }
    return;
  }
  if (row16) {
    sweep(T{}, F{}, 0, nfree);
    sweep(T{}, T{}, nfree, nsteps);
  } else {
    sweep(F{}, F{}, 0, nfree);
    sweep(F{}, T{}, nfree, nsteps);
  }

  // ---- distances: D[ref_len][h] = ref_len + sum_{k <= h} (Pv_k - Mv_k) (_string.py:357-405) --
  const int nvalid = min(max(x_len - 32 * b, 0), 32);
  const unsigned vm = nvalid == 32 ? 0xffffffffu : (1u << nvalid) - 1u;
  const int bs = __popc(Pv & vm) - __popc(Mv & vm);
  const int incl = wave_incl_scan_add(bs);
  const int seg = lane & ~(L - 1);
  const int before = __builtin_amdgcn_ds_bpermute((seg > 0 ? seg - 1 : 0) << 2, incl);
  int run = ref_len + incl - bs - (seg > 0 ? before : 0);
  if (valid) {
    if (b == 0) bnd[0] = (float)ref_len;
    for (int k = 0; k < nvalid; ++k) {
      run += (int)((Pv >> k) & 1u) - (int)((Mv >> k) & 1u);
      bnd[32 * b + k + 1] = (float)run;
    }
  }
  wave_sync();
  if (!valid) return;
  if (a.mode == PDT_MODE_FINAL) {
    if (b == 0)
      a.out[n * a.out_sn] = lev_finish(bnd[Heff], a.mult, a.norm, ref_len, hyp_len > 0 ? 1.0f : 0.0f);
  } else {
    const int Hout = a.H + (a.exclude_last ? 0 : 1);
    const int pad_from = hyp_len + (a.exclude_last ? 0 : 1);  // :379-386
    for (int h = b; h < Hout; h += L) {
      float v;
      if (h >= pad_from)
        v = a.padding;
      else
        v = lev_finish(bnd[h], a.mult, a.norm, ref_len, h > 0 ? 1.0f : 0.0f);
      a.out[(int64_t)h * a.out_sh + n * a.out_sn] = v;
    }
  }
}

__global__ void __launch_bounds__(256) lev_bitpar_kernel(const BitparArgs a, const int lds_per_sub, const int ring_off) {
  lev_bitpar_body<true>(a, lds_per_sub, ring_off);
}

// the recurrence alone, on tables that lev_classify_kernel left in the workspace
__global__ void __launch_bounds__(128) lev_bitpar_staged_kernel(const BitparArgs a, const int lds_per_sub, const int ring_off) {
  lev_bitpar_body<false>(a, lds_per_sub, ring_off);
}

// LevArgs -> the launches.  `ws` must hold plan.total bytes.
int launch_lev_bitpar(const LevArgs &la, const BitparPlan &p, void *ws, hipStream_t stream, LevTables tables) {
  const BitparArgs a = bitpar_args(la, p, ws, /*oc=*/false);
  int rc = 0;
  if (tables == kTablesOwn && p.fused) {  // one launch, nothing goes through the workspace
    const size_t smem = p.lds_sub_fused * 4 + kFusedLensBytes + p.lds_tail;
    rc = set_lds(lev_bitpar_kernel, smem);
    if (rc) return rc;
    hipLaunchKernelGGL(lev_bitpar_kernel, dim3((unsigned)((a.N + 3) / 4)), dim3(256), smem, stream, a,
                       (int)p.lds_sub_fused, (int)(p.lds_sub_fused * 4 + kFusedLensBytes));
    return (int)hipGetLastError();
  }
  if (tables != kTablesGiven) {  // (pdt_lev_classified: the workspace holds these inputs' tables already)
    rc = launch_bitpar_classify(a, p, stream);
    if (rc) return rc;
  }
  const size_t smem = p.lds_sub * p.upw + p.lds_tail;
  const unsigned grid = (unsigned)((a.N + p.upw - 1) / p.upw);
  rc = set_lds(lev_bitpar_staged_kernel, smem);
  if (rc) return rc;
  hipLaunchKernelGGL(lev_bitpar_staged_kernel, dim3(grid), dim3(128), smem, stream, a, (int)p.lds_sub,
                     (int)(p.lds_sub * p.upw));
  return (int)hipGetLastError();
}

}  // namespace pdt
