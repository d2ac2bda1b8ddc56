// Optimal completion's class bitmasks for unit costs and references of up to 512 tokens, bit-parallel
// (pdt_oc_mask): the block-minimum table, decode and spread helpers, oc_bitpar_kernel /
// oc_bitpar_staged_kernel, their workspace and their launch.  Classification is classify_utterance
// (bitpar_classify.hpp) -- inside oc_bitpar_kernel where the plan says `oc_fused`, else
// lev_classify_kernel (bitpar_classify.hip) in front of oc_bitpar_staged_kernel.
#include "bitpar_classify.hpp"
#include "lev_launch.hpp"

namespace pdt {

// ---- optimal completion: the arg-min sets of every row, bit-parallel --------------------------
// (reference _string.py:271-278, :333-354: after hypothesis token h, the set of reference tokens
// ref[c] over the columns c < ref_len where D[h][c] is the row minimum.)
//
// Bit-vectors run along the REFERENCE here: after h hypothesis tokens Pv / Mv hold
// D[h][c] - D[h][c-1] for every column, so the row's profile relative to D[h][0] = h is a prefix sum
// of +1 / -1 bits and the row minimum needs no DP value at all.  16 lanes (one DPP row) per
// utterance, four utterances per wave, lane b owns columns 32 b + 1 .. 32 b + 32, every lane on the
// SAME row:
//   * the 512-bit addition of Myers' step is 16 word additions whose carries are resolved on the
//     scalar unit -- generate / propagate lane masks (v_add_co's carry mask, one v_cmp), one 64-bit
//     add (Gm << 1) + Pm, xor, and a v_addc_co that takes the result as its carry-in mask;
//   * the shifts take the neighbour's word through a row_shr:1 and one v_alignbit;
//   * a block's (total, min prefix, arg-min bits) come from a 256-entry table over 4 columns at a
//     time (index = plus nibble | minus nibble << 4), block starts from a 4-step row scan, the row
//     minimum from a 4-step row all-reduce;
//   * the arg-min bits are permuted so that neighbouring columns sit in different lanes (oc_spread)
//     and turned into class bits by LDS ORs; the row's W words leave with one exchange each.
// Utterances whose hypothesis has ended write empty sets.
//
// What bounds it (profiles/r03_oc_*): the four utterances of a SIMD are one wave's worth of
// lanes, and a lone wave issues an instruction every ~5.5 cycles.  One wave doing everything took
// 0.375 ms (0.46 before the rows of a pass were processed phase by phase); splitting the rows'
// independent part over consumer waves (below) 0.24 ms, at which point the SIMDs' vector issue is
// ~80 % busy (profiles/tools/micro/valu_cost.hip: with several waves per SIMD most integer
// instructions other than add / sub / and / or / xor / right shifts issue at half rate).
constexpr int kOcChunk = 4;      // rows per pass of oc_bitpar_kernel
constexpr int kOcConsumers = 3;  // consumer waves per workgroup of oc_bitpar_kernel
constexpr int oc_slots(const int nc) { return 2 * nc; }  // ring slots (passes in flight) per workgroup

struct OcBitArgs {
  int N, X, Y, W, Hout, exclude_last;
  const int32_t *lens;
  const uint2 *yh;
  const uint32_t *msk;
  const uint16_t *xcls;
  uint32_t *bitmask;
  int32_t *max_count;
};

#define PDT_DPP_QUAD_XOR1 0xB1
#define PDT_DPP_QUAD_XOR2 0x4E
#define PDT_DPP_ROW_HALF_MIRROR 0x141
#define PDT_DPP_ROW_MIRROR 0x140

// The block-minimum table over 4 columns (index = plus nibble | minus nibble << 4): the sum of the
// deltas, the minimum prefix (over the prefixes of length >= 1) and the columns that reach it, as
// byte fields, 32 bits per entry: byte 0 = sum (signed), byte 1 = min prefix
// (signed), byte 2 = arg-min bits -- SDWA operands then fold the field extraction (and the sign
// extension) into the additions and the shift of the decode: 5 instructions per nibble instead of 8
__device__ __forceinline__ void oc_build_table32(unsigned *tab) {
  for (int idx = (int)threadIdx.x; idx < 256; idx += (int)blockDim.x) {
    const int p = idx & 15, m = idx >> 4;
    int run = 0, mn = 99, am = 0;
    for (int j = 0; j < 4; ++j) {
      run += ((p >> j) & 1) - ((m >> j) & 1);
      if (run < mn) {
        mn = run;
        am = 1 << j;
      } else if (run == mn) {
        am |= 1 << j;
      }
    }
    tab[idx] = (unsigned)(run & 0xff) | ((unsigned)(mn & 0xff) << 8) | ((unsigned)am << 16);
  }
}

// byte `I` of z, times four (one SDWA shift: the table's byte offset)
template <int I>
__device__ __forceinline__ unsigned byte_times4(const unsigned z, const unsigned two) {
  unsigned r;
  if (I == 0) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(two), "v"(z));
  if (I == 1) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(two), "v"(z));
  if (I == 2) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(two), "v"(z));
  if (I == 3) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(two), "v"(z));
  return r;
}

// the eight table entries of a block: index = plus nibble | minus nibble << 4, a byte of one of two
// interleaved words
__device__ __forceinline__ void oc_table_reads32(const unsigned *tab, const unsigned pv, const unsigned mv,
                                                 unsigned (&e)[8]) {
  const unsigned ze = (pv & 0x0f0f0f0fu) | ((mv << 4) & 0xf0f0f0f0u);  // nibbles 0, 2, 4, 6
  const unsigned zo = ((pv >> 4) & 0x0f0f0f0fu) | (mv & 0xf0f0f0f0u);  // nibbles 1, 3, 5, 7
  unsigned two = 2u;
  asm volatile("" : "+v"(two));
  const unsigned char *t = reinterpret_cast<const unsigned char *>(tab);
  e[0] = *reinterpret_cast<const unsigned *>(t + byte_times4<0>(ze, two));
  e[1] = *reinterpret_cast<const unsigned *>(t + byte_times4<0>(zo, two));
  e[2] = *reinterpret_cast<const unsigned *>(t + byte_times4<1>(ze, two));
  e[3] = *reinterpret_cast<const unsigned *>(t + byte_times4<1>(zo, two));
  e[4] = *reinterpret_cast<const unsigned *>(t + byte_times4<2>(ze, two));
  e[5] = *reinterpret_cast<const unsigned *>(t + byte_times4<2>(zo, two));
  e[6] = *reinterpret_cast<const unsigned *>(t + byte_times4<3>(ze, two));
  e[7] = *reinterpret_cast<const unsigned *>(t + byte_times4<3>(zo, two));
}

// total of each block's deltas, its minimum prefix and the columns that reach it, from its eight
// entries.  R rows at once, their chains interleaved instruction by instruction (a dependent SDWA instruction
// right behind its producer costs wait states: 20 s_nop per row when the rows were decoded one after
// the other)
template <int R>
__device__ __forceinline__ void oc_block_decode32(const unsigned (&e)[R][8], int (&total)[R], int (&best)[R],
                                                  unsigned (&am)[R]) {
  int run[R], cand[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) run[r] = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      asm("v_add_u32_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(cand[r][k]) : "v"(run[r]), "v"(e[r][k]));
#pragma unroll
    for (int r = 0; r < R; ++r)
      asm("v_add_u32_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(run[r]) : "v"(run[r]), "v"(e[r][k]));
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    best[r] = min(min(min(cand[r][0], cand[r][1]), min(cand[r][2], cand[r][3])),
                  min(min(cand[r][4], cand[r][5]), min(cand[r][6], cand[r][7])));
    am[r] = 0u;
    total[r] = run[r];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    unsigned t[R];
    const unsigned sh = 4u * k;  // (a scalar operand: no vector move per nibble)
#pragma unroll
    for (int r = 0; r < R; ++r)
      asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(t[r]) : "s"(sh), "v"(e[r][k]));
#pragma unroll
    for (int r = 0; r < R; ++r) am[r] |= cand[r][k] == best[r] ? t[r] : 0u;
  }
}

// min over the 16 lanes of a DPP row, in every lane (written out: left to the compiler every
// stage is two moves, the DPP move and the v_min)
__device__ __forceinline__ int row_all_min(int v) {
  asm volatile(
      "s_nop 1\n\tv_min_i32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_i32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_i32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_i32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1"
      : "+v"(v));
  return v;
}

// The arg-min columns of a row come in runs (a dozen neighbouring columns at the bench shape), i.e.
// in ONE lane's word, and turning a bit into a class bit is a dependent LDS read + LDS OR.  Four
// exchange stages (partner lanes l^8, l^7, l^2, l^1 inside the DPP row; keep half of the bits, take
// the partner's other half rotated by the stage's distance) permute the 512 bits of an utterance so
// that any 16 neighbouring columns end up in 16 different lanes.  Which column a (lane, bit) pair
// holds afterwards is found once per kernel by sending the nine bit-planes of the column index
// through the same network; the class table is staged in that order.
struct OcSpread {
  unsigned keep[4];  // bits this lane keeps at each stage
  unsigned amt[4];   // v_alignbit shift that rotates the partner's word the right way
};
__device__ __forceinline__ OcSpread oc_spread_setup(const int b) {
  OcSpread sp;
  const unsigned clear[4] = {0x00ff00ffu, 0x0f0f0f0fu, 0x33333333u, 0x55555555u};  // bit d of the position clear
  const int dist[4] = {8, 4, 2, 1};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bool hi = (b & dist[s]) != 0;
    sp.keep[s] = hi ? ~clear[s] : clear[s];
    sp.amt[s] = hi ? (unsigned)dist[s] : (unsigned)(32 - dist[s]);  // alignbit(x, x, k) rotates right by k
  }
  return sp;
}
__device__ __forceinline__ unsigned oc_spread(const OcSpread &sp, unsigned x) {
  unsigned p, t;
  auto bfi = [](const unsigned mask, const unsigned a, const unsigned b) {  // (mask & a) | (~mask & b)
    unsigned r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(a), "v"(b));
    return r;
  };
  p = (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x128 /* row_ror:8 */, 0xf, 0xf, true);
  t = __builtin_amdgcn_alignbit(p, p, sp.amt[0]);
  x = bfi(sp.keep[0], x, t);
  p = (unsigned)__builtin_amdgcn_mov_dpp((int)x, PDT_DPP_ROW_HALF_MIRROR, 0xf, 0xf, true);
  t = __builtin_amdgcn_alignbit(p, p, sp.amt[1]);
  x = bfi(sp.keep[1], x, t);
  p = (unsigned)__builtin_amdgcn_mov_dpp((int)x, PDT_DPP_QUAD_XOR2, 0xf, 0xf, true);
  t = __builtin_amdgcn_alignbit(p, p, sp.amt[2]);
  x = bfi(sp.keep[2], x, t);
  p = (unsigned)__builtin_amdgcn_mov_dpp((int)x, PDT_DPP_QUAD_XOR1, 0xf, 0xf, true);
  t = __builtin_amdgcn_alignbit(p, p, sp.amt[3]);
  x = bfi(sp.keep[3], x, t);
  return x;
}

// Workgroup = four utterances (one per DPP row of every wave) and 1 + NC waves.  The recurrence is
// the only part of a row that depends on the row before and it is a tenth of the row's
// instructions, so ONE wave (the producer) runs it and leaves each row's masked (Pv, Mv) words in an
// LDS ring, a pass of kOcChunk rows per slot; NC consumer waves take passes in turn and do the rest
// (block minima, row minimum, spreading, class bits, the store).  A lone wave issues an instruction
// every ~5.5 cycles; with the waves of four such workgroups on a CU every SIMD has several to pick
// from.  Roles rotate with the workgroup index so that producers do not all land on one SIMD.
//
// FUSED (the plan's oc_fused: hypotheses of up to 512 tokens, LDS within 40 KiB): the four waves first
// classify the group's four utterances, one each (classify_utterance<8, kClassifyPacked>), and only
// then take their roles.  An utterance's region is [match words][yh, ONE word per hypothesis token:
// presence of the 16 blocks | offset << 16][classes in spread order]; the token table lies over the
// whole region while it lives, the per-class words and the classes in position order use the
// passes' ring, which nobody writes before the roles start.  Nothing but `class_tokens` -- the
// call's output -- goes to memory, and the producer reads its look-ups from LDS instead of
// fetching them 16 rows ahead.
struct OcLds {
  size_t flags, ring, bm, sub, total;  // byte offsets; sub = first utterance's tables
  size_t per_sub;
  size_t yh, scratch;  // FUSED: yh inside an utterance's region; a wave's share of the ring while classifying
};
constexpr size_t kOcLensOff = 128;  // FUSED: (ref_len, hyp_len) x 4 behind the ring's flags
static __host__ __device__ inline OcLds oc_lds(const int X, const int Y, const int NC, const bool fused) {
  OcLds l;
  const size_t Xs = (size_t)(X > 0 ? X : 1), Ys = (size_t)(Y > 0 ? Y : 1);
  const int S = oc_slots(NC);
  l.flags = 1024;                                          // after the 256-entry table (room for 32-bit entries)
  l.ring = l.flags + 256;                                  // ready[S], done[S]
  l.bm = l.ring + (size_t)S * kOcChunk * PDT_WAVE * 8;     // a slot: kOcChunk rows of (Pv, Mv) per lane
  l.sub = l.bm + (size_t)NC * kOcChunk * PDT_WAVE * 4;     // per consumer: kOcChunk rows of 16 words per utterance
  l.per_sub = ((Xs + 1) * 4 + 15) / 16 * 16 + 256 + 512 * 2;  // match words; 2 x 16 look-ups; classes in spread order
  l.yh = l.scratch = 0;
  if (fused) {
    l.yh = ((Xs + 1) * 4 + 15) / 16 * 16;
    l.per_sub = l.yh + (Ys * 4 + 15) / 16 * 16 + 512 * 2;
    const size_t tab = Xs * 8 > (size_t)kDirectWords * 8 ? Xs * 8 : (size_t)kDirectWords * 8;  // token table / presence map
    if (l.per_sub < tab) l.per_sub = tab;
    l.scratch = (l.bm - l.ring) / 4;  // >= X * 4 (per-class words) + X * 2 (classes): 3 072 B at S = 6
  }
  l.total = l.sub + 4 * l.per_sub;
  return l;
}

template <int NC, bool FUSED>
__device__ __forceinline__ void oc_bitpar_body(const OcBitArgs &a, const BitparArgs &ca) {
  static_assert(!FUSED || NC == 3, "the fused form classifies with the workgroup's four waves");
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int S = oc_slots(NC), kChunk = kOcChunk, NG = 8;
  unsigned *tab = reinterpret_cast<unsigned *>(smem);
  oc_build_table32(tab);
  const OcLds L = oc_lds(a.X, a.Y, NC, FUSED);
  int *ready = reinterpret_cast<int *>(smem + L.flags), *done = ready + S;
  uint2 *ring = reinterpret_cast<uint2 *>(smem + L.ring);
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  // (FUSED: the classification's workgroup order -- its token reads are what the order is for)
  const int64_t grp = FUSED ? (int64_t)xcd_remap(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int role = (wave + (int)grp) % (NC + 1);  // 0: producer, 1 .. NC: consumers
  const int q = lane >> 4, b = lane & 15;
  const int64_t n_raw = grp * 4 + q;
  const bool valid = n_raw < a.N;
  const int64_t n = valid ? n_raw : (int64_t)a.N - 1;
  const int X = a.X > 0 ? a.X : 1, Y = a.Y > 0 ? a.Y : 1;
  unsigned char *base = smem + L.sub + (size_t)q * L.per_sub;
  unsigned *msk_l = reinterpret_cast<unsigned *>(base);
  uint16_t *xc_l = reinterpret_cast<uint16_t *>(base + L.per_sub - 1024);
  const unsigned *yh_l = reinterpret_cast<const unsigned *>(base + L.yh);  // (FUSED)

  int ref_len, hyp_len;
  const uint16_t *csrc;
  if (FUSED) {
    int32_t *lens_l = reinterpret_cast<int32_t *>(smem + L.flags + kOcLensOff);
    const int64_t nw = grp * 4 + wave;  // wave w classifies utterance w of the group
    if (nw < a.N) {
      unsigned char *r = smem + L.sub + (size_t)wave * L.per_sub, *scr = smem + L.ring + (size_t)wave * L.scratch;
      const Classified c = classify_utterance<8, kClassifyPacked>(
          ca, nw, reinterpret_cast<uint2 *>(scr), reinterpret_cast<int64_t *>(r), reinterpret_cast<unsigned *>(r),
          reinterpret_cast<short *>(scr + (size_t)X * 4), reinterpret_cast<uint2 *>(r + L.yh));
      if (lane == 0) {
        lens_l[2 * wave] = c.ref_len;
        lens_l[2 * wave + 1] = c.hyp_len;
      }
    } else if (lane == 0) {
      // (no such utterance: its quarter of the producer still runs the rows, on look-up 0 = no match)
      *reinterpret_cast<unsigned *>(smem + L.sub + (size_t)wave * L.per_sub + L.yh) = 0u;
    }
    __syncthreads();
    ref_len = valid ? lens_l[2 * q] : 0;
    hyp_len = valid ? lens_l[2 * q + 1] : 0;
    csrc = reinterpret_cast<const uint16_t *>(smem + L.ring + (size_t)(valid ? q : 0) * L.scratch + (size_t)X * 4);
  } else {
    ref_len = valid ? a.lens[2 * n] : 0;
    hyp_len = valid ? a.lens[2 * n + 1] : 0;
    csrc = a.xcls + n * (int64_t)X;
  }
  int Heff = a.exclude_last ? hyp_len - 1 : hyp_len;
  if (Heff < 0) Heff = 0;
  if (threadIdx.x < 2 * S) ready[threadIdx.x] = 0;
  const OcSpread sp = oc_spread_setup(b);
  const int rank0 = ref_len > 0 ? (int)csrc[0] : 0;  // class of ref[0]
  if (FUSED && role == 0) {  // (the match words are where the classification built them)
  } else if (role == 0) {  // the match words of this utterance: 16 lanes, eight loads in flight each
    const unsigned *msrc = a.msk + n * (int64_t)(X + 1);
    for (int i0 = b; i0 <= ref_len; i0 += 8 * 16) {
      unsigned v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = i0 + r * 16 <= ref_len ? msrc[i0 + r * 16] : 0u;
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (i0 + r * 16 <= ref_len) msk_l[i0 + r * 16] = v[r];
    }
  } else {
    // xc_l[32 b + t] = class of ref[c] for the column c that the network leaves in bit t of lane b
    unsigned *bm0 = reinterpret_cast<unsigned *>(smem + L.bm) + (size_t)(role - 1) * kChunk * PDT_WAVE;
    for (int r = 0; r < kChunk; ++r) bm0[r * PDT_WAVE + lane] = 0u;
    unsigned plane[9];
    const unsigned low[5] = {0xaaaaaaaau, 0xccccccccu, 0xf0f0f0f0u, 0xff00ff00u, 0xffff0000u};
#pragma unroll
    for (int k = 0; k < 9; ++k) plane[k] = oc_spread(sp, k < 5 ? low[k] : (((b >> (k - 5)) & 1) ? 0xffffffffu : 0u));
    for (int t0 = 8 * (role - 1); t0 < 32; t0 += 8 * NC) {
      uint16_t v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        int c = 1;  // column = (bit index of the unspread layout) + 1
#pragma unroll
        for (int k = 0; k < 9; ++k) c += (int)((plane[k] >> (t0 + r)) & 1u) << k;
        v[r] = c < ref_len ? csrc[c] : (uint16_t)0;
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) xc_l[32 * b + t0 + r] = v[r];
    }
  }
  __syncthreads();  // (the only one: from here on the waves meet through the ring's flags)

  const int W = a.W;
  // columns of this block that exist (<= ref_len) and those that have a next token (< ref_len)
  const int nvalid = min(max(ref_len - 32 * b, 0), 32), nnext = min(max(ref_len - 1 - 32 * b, 0), 32);
  const unsigned vmask = nvalid == 32 ? 0xffffffffu : (1u << nvalid) - 1u;
  const unsigned nmask = nnext == 32 ? 0xffffffffu : (1u << nnext) - 1u;
  int hmax = Heff;
#pragma unroll
  for (int t = 16; t < PDT_WAVE; t <<= 1) hmax = max(hmax, __shfl_xor(hmax, t));
  hmax = __builtin_amdgcn_readfirstlane(hmax);
  const int nchunks = (hmax + kChunk - 1) / kChunk;
  const int64_t row_stride = (int64_t)a.N * W;
  uint32_t *out_row = a.bitmask + n * (int64_t)W + b;  // row 0 of this lane's word

  if (role == 0) {
    // ---- producer: Myers' step on the 512-bit column, four utterances side by side ------------
    if (valid && b < W) {  // h = 0: only column 0 (:271-278)
      unsigned w = 0u;
      if (ref_len > 0 && (rank0 >> 5) == b) w = 1u << (rank0 & 31);
      out_row[0] = w;
    }
    // rows nobody in the workgroup reaches (`& not_done`, :334)
    for (int h = hmax + 1; h < a.Hout; ++h)
      if (valid && b < W) out_row[h * row_stride] = 0u;
    const unsigned lowmask = (1u << b) - 1u, bbit = 1u << b;
    const int jcap = Heff > 0 ? Heff - 1 : 0;
    const uint2 *ysrc = a.yh + n * (int64_t)Y;
    unsigned Pv = 0xffffffffu, Mv = 0u;  // row 0: D[0][c] = c
    unsigned xp = b == 0 ? 0x80000000u : 0u, xm = 0u;  // (lane 0 of a row keeps D[h][0] - D[h-1][0] = +1)
    u64 notop = 0x7fff7fff7fff7fffull;  // carries stay inside an utterance's 16 lanes
    asm volatile("" : "+s"(notop));     // (in a register pair: the literal would split every AND in two)
    // (presence, offset) of the hypothesis tokens' classes: lane b fetches row 16 k + b a block of 16
    // rows ahead (a load per pass would cost its whole latency every pass) and leaves it in LDS
    static_assert(16 % kChunk == 0, "a block of look-ups is a whole number of passes");
    uint2 *ybuf = reinterpret_cast<uint2 *>(base + L.per_sub - 1024 - 256);
    uint2 pre = make_uint2(0u, 0u);
    if (!FUSED) pre = Heff > 0 ? ysrc[min(b, jcap)] : make_uint2(0u, 0u);
    for (int i = 0; i < nchunks; ++i) {
      uint2 hq[kChunk];
      if (FUSED) {  // (rows past the hypothesis read its last entry, as the clamped fetches below do)
#pragma unroll
        for (int r = 0; r < kChunk; ++r) {
          const unsigned v = yh_l[min(i * kChunk + r, jcap)];
          hq[r] = make_uint2(v & 0xffffu, v >> 16);
        }
      } else {
        if ((i * kChunk) % 16 == 0) {
          const int blk = (i * kChunk) >> 4;
          ybuf[(blk & 1) * 16 + b] = pre;
          pre = Heff > 0 ? ysrc[min((blk + 1) * 16 + b, jcap)] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int r = 0; r < kChunk; ++r) hq[r] = ybuf[(i * kChunk + r) & 31];
      }
      unsigned eq[kChunk];
#pragma unroll
      for (int r = 0; r < kChunk; ++r) eq[r] = msk_l[hq[r].y + (unsigned)__popc(hq[r].x & lowmask)];
#pragma unroll
      for (int r = 0; r < kChunk; ++r) eq[r] = (hq[r].x & bbit) ? eq[r] : 0u;
      const int slot = i % S;
      if (i >= S)
        while (__hip_atomic_load(&done[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < i - S + 1)
          __builtin_amdgcn_s_sleep(2);
      uint2 *dst = ring + (size_t)slot * kChunk * PDT_WAVE + lane;
#pragma unroll
      for (int r = 0; r < kChunk; ++r) {
        const unsigned Eq = eq[r];
        const unsigned Xv = Eq | Mv;
        const unsigned A = Eq & Pv;
        unsigned sum;
        u64 Gm;
        asm volatile("v_add_co_u32 %0, %1, %2, %3" : "=v"(sum), "=s"(Gm) : "v"(A), "v"(Pv));
        Gm &= notop;
        const u64 Pm = __ballot(sum == 0xffffffffu) & notop;
        const u64 C = ((Gm << 1) + Pm) ^ Pm;
        asm volatile("v_addc_co_u32 %0, %1, 0, %2, %3" : "=v"(sum), "=s"(Gm) : "v"(sum), "s"(C));
        const unsigned Xh = (sum ^ Pv) | Eq;
        const unsigned Phw = Mv | ~(Xh | Pv);
        const unsigned Mhw = Pv & Xh;
        xp = (unsigned)__builtin_amdgcn_update_dpp((int)xp, (int)Phw, PDT_DPP_ROW_SHR(1), 0xf, 0xf, false);
        xm = (unsigned)__builtin_amdgcn_update_dpp((int)xm, (int)Mhw, PDT_DPP_ROW_SHR(1), 0xf, 0xf, false);
        const unsigned Ph = __builtin_amdgcn_alignbit(Phw, xp, 31);
        const unsigned Mh = __builtin_amdgcn_alignbit(Mhw, xm, 31);
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
        dst[r * PDT_WAVE] = make_uint2(Pv & vmask, Mv & vmask);
      }
      if (lane == 0) __hip_atomic_store(&ready[slot], i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return;
  }

  // ---- consumers: passes role - 1, role - 1 + NC, ... ---------------------------------------------
  unsigned *bm = reinterpret_cast<unsigned *>(smem + L.bm) + (size_t)(role - 1) * kChunk * PDT_WAVE + 16 * q;
  int max_cnt = (role == 1 && ref_len > 0) ? 1 : 0;  // (row 0)
  for (int i = role - 1; i < nchunks; i += NC) {
    const int slot = i % S, h0 = i * kChunk;
    while (__hip_atomic_load(&ready[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < i + 1)
      __builtin_amdgcn_s_sleep(2);
    const uint2 *src = ring + (size_t)slot * kChunk * PDT_WAVE + lane;
    uint2 pm[kChunk];
#pragma unroll
    for (int r = 0; r < kChunk; ++r) pm[r] = src[r * PDT_WAVE];
    unsigned e[kChunk][NG];
#pragma unroll
    for (int r = 0; r < kChunk; ++r) oc_table_reads32(tab, pm[r].x, pm[r].y, e[r]);
    if (lane == 0) __hip_atomic_store(&done[slot], i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    unsigned rest[kChunk], or0[kChunk], or1[kChunk];
    int c0[kChunk], c1[kChunk];
    bool zero_min[kChunk];
    int total_r[kChunk], best_r[kChunk];
    unsigned am_r[kChunk];
    oc_block_decode32<kChunk>(e, total_r, best_r, am_r);
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      const bool active = h0 + r + 1 <= Heff;
      const int total = total_r[r], best = best_r[r];
      const unsigned am = am_r[r];
      int incl = total;  // D[h][32 b + 32] - D[h][0]
      incl += dpp_or<PDT_DPP_ROW_SHR(1)>(incl, 0);
      incl += dpp_or<PDT_DPP_ROW_SHR(2)>(incl, 0);
      incl += dpp_or<PDT_DPP_ROW_SHR(4), 0xf, 0xe>(incl, 0);
      incl += dpp_or<PDT_DPP_ROW_SHR(8), 0xf, 0xc>(incl, 0);
      const int cand = incl - total + best;
      const int m = row_all_min(min(cand, 0));  // (0: column 0)
      zero_min[r] = active && m == 0;
      unsigned bits = (active && cand == m) ? am & nmask : 0u;  // :334 and the c < ref_len cut of :349-354
      bits = oc_spread(sp, bits);
      // the first two bits of a lane go the short way (a lane rarely holds more)
      const int j0 = bits ? __builtin_ctz(bits) : 0;
      or0[r] = bits ? 1u : 0u;
      bits &= bits - 1u;
      const int j1 = bits ? __builtin_ctz(bits) : 0;
      or1[r] = bits ? 1u : 0u;
      bits &= bits - 1u;
      rest[r] = bits;
      c0[r] = xc_l[32 * b + j0];
      c1[r] = xc_l[32 * b + j1];
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {  // (an OR of 0 where there is no bit: no branches)
      unsigned *bmr = bm + PDT_WAVE * r;
      atomicOr(&bmr[c0[r] >> 5], or0[r] << (c0[r] & 31));
      atomicOr(&bmr[c1[r] >> 5], or1[r] << (c1[r] & 31));
      if (b == 0) atomicOr(&bmr[rank0 >> 5], (zero_min[r] && ref_len > 0) ? 1u << (rank0 & 31) : 0u);
    }
    unsigned any_rest = 0u;
#pragma unroll
    for (int r = 0; r < kChunk; ++r) any_rest |= rest[r];
    if (__ballot(any_rest != 0u)) {
#pragma unroll
      for (int r = 0; r < kChunk; ++r) {
        unsigned bits = rest[r];
        while (__ballot(bits != 0u)) {
          if (bits) {
            const int cls = xc_l[32 * b + __builtin_ctz(bits)];
            bits &= bits - 1u;
            atomicOr(&bm[PDT_WAVE * r + (cls >> 5)], 1u << (cls & 31));
          }
        }
      }
    }
    // (the LDS serves one wave's instructions in order: the exchanges see every lane's OR)
    __builtin_amdgcn_wave_barrier();
    unsigned w[kChunk];
#pragma unroll
    for (int r = 0; r < kChunk; ++r)
      w[r] = __hip_atomic_exchange(&bm[PDT_WAVE * r + b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __builtin_amdgcn_wave_barrier();
    if (valid && b < W) {
#pragma unroll
      for (int r = 0; r < kChunk; ++r)
        if (h0 + r + 1 <= hmax && h0 + r + 1 < a.Hout) out_row[(h0 + r + 1) * row_stride] = w[r];
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      int cnt = __popc(w[r]);
      cnt += dpp_or<PDT_DPP_QUAD_XOR1>(cnt, 0);
      cnt += dpp_or<PDT_DPP_QUAD_XOR2>(cnt, 0);
      cnt += dpp_or<PDT_DPP_ROW_HALF_MIRROR>(cnt, 0);
      cnt += dpp_or<PDT_DPP_ROW_MIRROR>(cnt, 0);
      max_cnt = max(max_cnt, cnt);
    }
  }
  if (valid && b == 0 && a.max_count && max_cnt > 0) atomicMax(a.max_count, max_cnt);
}

template <int NC>
__global__ void __launch_bounds__(64 * (NC + 1)) oc_bitpar_kernel(const OcBitArgs a, const BitparArgs ca) {
  oc_bitpar_body<NC, true>(a, ca);
}

// the mask kernel alone, on tables that lev_classify_kernel left in the workspace
template <int NC>
__global__ void __launch_bounds__(64 * (NC + 1)) oc_bitpar_staged_kernel(const OcBitArgs a) {
  oc_bitpar_body<NC, false>(a, BitparArgs{});
}

constexpr int64_t kOcBitparMaxR = 512;  // 16 lanes of 32 columns

// (a ring too small for the classification's scratch -- other oc_slots / kOcChunk -- reads as
// "does not fit": two launches)
size_t oc_fused_lds_bytes(int64_t X, int64_t Y) {
  const OcLds l = oc_lds((int)X, (int)Y, kOcConsumers, true);
  return l.scratch >= (size_t)(X > 0 ? X : 1) * 6 ? l.total : ~(size_t)0;
}

int64_t oc_bitpar_workspace_bytes(int64_t R, int64_t H, int64_t N) {
  if (R > kOcBitparMaxR || H < 0 || N <= 0) return 0;
  const BitparPlan p = plan_bitpar(R, H, N);
  if (!p.ok) return 0;
  return (int64_t)(p.total + align_up((size_t)N * (size_t)(R > 0 ? R : 1) * 2, 256));
}

// the mask kernel's own arguments, next to the classification's
static OcBitArgs oc_bit_args(const LevArgs &la, const BitparArgs &a) {
  OcBitArgs o{};
  o.N = la.N; o.X = la.R; o.Y = la.H; o.W = la.W;
  o.Hout = la.H + (la.exclude_last ? 0 : 1);
  o.exclude_last = la.exclude_last;
  o.lens = a.lens; o.yh = a.yh; o.msk = a.msk; o.xcls = a.xcls;
  o.bitmask = la.bitmask; o.max_count = la.max_count;
  return o;
}

// Unit costs only.  Returns -1 when the shape is not served (the caller falls back to
// lev_rowsync.hip), else the launch status.
int launch_oc_mask_bitpar(const LevArgs &la, void *ws, int64_t ws_bytes, hipStream_t stream) {
  if (la.R > kOcBitparMaxR || !ws) return -1;
  const BitparPlan p = plan_bitpar(la.R, la.H, la.N);
  const int64_t need = oc_bitpar_workspace_bytes(la.R, la.H, la.N);
  if (!p.ok || need == 0 || need > ws_bytes) return -1;
  const BitparArgs a = bitpar_args(la, p, ws, /*oc=*/true);
  const OcBitArgs o = oc_bit_args(la, a);
  constexpr int NC = kOcConsumers;
  const dim3 grid((unsigned)((la.N + 3) / 4)), block(64 * (NC + 1));
  const OcLds L = oc_lds(o.X, o.Y, NC, p.oc_fused != 0);
  int rc = 0;
  if (p.oc_fused) {  // one launch: nothing but class_tokens leaves the kernel's classification
    rc = set_lds(oc_bitpar_kernel<NC>, L.total);
    if (rc) return rc;
    hipLaunchKernelGGL(oc_bitpar_kernel<NC>, grid, block, L.total, stream, o, a);
    return (int)hipGetLastError();
  }
  rc = launch_bitpar_classify(a, p, stream);
  if (rc) return rc;
  rc = set_lds(oc_bitpar_staged_kernel<NC>, L.total);
  if (rc) return rc;
  hipLaunchKernelGGL(oc_bitpar_staged_kernel<NC>, grid, block, L.total, stream, o);
  return (int)hipGetLastError();
}

}  // namespace pdt
