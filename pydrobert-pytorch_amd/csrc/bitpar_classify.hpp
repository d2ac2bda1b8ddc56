// What the bit-parallel string kernels share (unit costs: lev_bitpar.hip, oc_bitpar.hip,
// bitpar_classify.hip): their argument block, and the classification of one utterance by one wave.
//
// Classification: the sequence lengths, the distinct tokens of the bit-vector sequence X in
// ascending order (ranks from a presence map of small tokens, or a bitonic sort in registers --
// lev_classes.hpp), and the match masks Eq[class][block] in compressed rows -- per class a 32-bit
// block-presence word + an offset into a packed array of mask words (one word per (class, block)
// pair that has a match: at most |X| words).  Every position of the consumed sequence Y gets its
// class's (presence, offset) pair, so a recurrence never sees a token.  X = hyp, Y = ref for the
// distances; the other way round for optimal completion (BitparArgs::oc).
#pragma once
#include "lev_classes.hpp"

namespace pdt {

struct BitparArgs {
  const int64_t *ref, *hyp;
  int64_t ref_st, ref_sn, hyp_st, hyp_sn;
  int R, H, N;
  int has_eos, include_eos;
  int64_t eos;
  int exclude_last, norm, mode;
  float mult, padding;
  float *out;
  int64_t out_sh, out_sn;
  int64_t *ref_lens_out, *hyp_lens_out;
  int32_t *status;
  int X, Y;      // capacities of the bit-vector sequence and of the consumed sequence
  int lgL, upw;  // lanes per utterance = 1 << lgL; utterances per wave (<= 64 >> lgL)
  int32_t *lens;   // [N][2]     ref_len, hyp_len
  uint2 *yh;       // [N][Y]     (block presence, offset) of the class of Y[j]; (0, 0) = no match
  uint32_t *msk;   // [N][X + 1] packed match-mask words
  // optimal-completion form (oc_bitpar_kernel): bit-vectors along the REFERENCE, hypothesis consumed
  int oc;
  int64_t *class_tokens;  // [N][R]  the distinct reference tokens, ascending (pdt_oc_mask's output)
  uint16_t *xcls;         // [N][X]  class of every reference position
};

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// LevArgs -> the kernels' arguments.  `ws` holds the plan's tables (plan.total bytes) and, for
// optimal completion (plan of (R, H); 16 lanes per utterance whatever the reference's length), the
// classes of the reference positions behind them (oc_bitpar_workspace_bytes).
static inline BitparArgs bitpar_args(const LevArgs &la, const BitparPlan &p, void *ws, const bool oc) {
  BitparArgs a{};
  a.ref = la.ref; a.hyp = la.hyp;
  a.ref_st = la.ref_st; a.ref_sn = la.ref_sn; a.hyp_st = la.hyp_st; a.hyp_sn = la.hyp_sn;
  a.R = la.R; a.H = la.H; a.N = la.N;
  a.has_eos = la.has_eos; a.include_eos = la.include_eos; a.eos = la.eos;
  a.exclude_last = la.exclude_last; a.status = la.status;
  a.X = oc ? la.R : la.H;
  a.Y = oc ? la.H : la.R;
  a.lgL = oc ? 4 : p.lgL; a.upw = oc ? 4 : p.upw;
  unsigned char *w = reinterpret_cast<unsigned char *>(ws);
  a.lens = reinterpret_cast<int32_t *>(w + p.off_lens);
  a.yh = reinterpret_cast<uint2 *>(w + p.off_yh);
  a.msk = reinterpret_cast<uint32_t *>(w + p.off_msk);
  if (oc) {  // (no distances: nothing is normalised, scaled or padded)
    a.mode = -1;
    a.oc = 1;
    a.class_tokens = la.class_tokens;
    a.xcls = reinterpret_cast<uint16_t *>(w + p.total);
  } else {
    a.norm = la.norm; a.mode = la.mode;
    a.mult = la.mult; a.padding = la.padding;
    a.out = la.out; a.out_sh = la.out_sh; a.out_sn = la.out_sn;
    a.ref_lens_out = la.ref_lens_out; a.hyp_lens_out = la.hyp_lens_out;
  }
  return a;
}

// ---- classification: lengths, classes, compressed match masks ---------------------------------
// One wave, one utterance, the tables left in LDS.  Three layouts:
//   kClassifyStaged   (lev_classify_kernel)  po, the token table (later the mask words) and the
//                     classes of Y (`yc`, two bytes each) are separate regions; the caller sends
//                     yh[j] = po[yc[j]] and the mask words to the workspace.
//   kClassifyInPlace  (the fused form of lev_bitpar_kernel; Y <= 8 * 64)  `po`, `ctok` and `yh_l`
//                     are ONE region of max(X, Y) * 8 bytes that holds, one after the other, the token
//                     table / presence map, then po, then the finished yh -- the classes of Y wait
//                     in registers while the region changes hands -- and `msk` is the recurrence's
//                     own array: classification needs no LDS beyond what the recurrence reads.
//   kClassifyPacked   (the fused form of oc_bitpar_kernel; X <= 512, Y <= 8 * 64)  po and yh are
//                     ONE 32-bit word per entry (presence of the 16 blocks | offset << 16), the
//                     classes of X go to LDS (`yc`, two bytes each, in position order) instead of
//                     the workspace; the token table may share its bytes with `msk` and `yh_l`
//                     (all written after it is dead), `po` and `yc` are scratch of their own.
struct Classified {
  int ref_len, hyp_len, x_len, y_len;
};
enum ClassifyMode { kClassifyStaged, kClassifyInPlace, kClassifyPacked };

template <int NR, ClassifyMode MODE>
__device__ __forceinline__ Classified classify_utterance(const BitparArgs &a, const int64_t n, uint2 *po,
                                                         int64_t *ctok, unsigned *msk, short *yc, uint2 *yh_l) {
  constexpr bool IN_PLACE = MODE != kClassifyStaged;  // (the classes of Y stay in registers)
  constexpr bool PACKED = MODE == kClassifyPacked;
  unsigned *po32 = reinterpret_cast<unsigned *>(po), *yh32 = reinterpret_cast<unsigned *>(yh_l);
  const int lane = lane_id();
  const int X = a.X > 0 ? a.X : 1;
  uint2 *pmap = reinterpret_cast<uint2 *>(ctok);  // (instead of the token table: one or the other)

  // ---- lengths (_string.py:195-228) -----------------------------------------------------
  int ref_len = a.R, hyp_len = a.H;
  bool rmiss = false, hmiss = false;
  const int64_t roff = n * a.ref_sn, hoff = n * a.hyp_sn;
  if (a.has_eos) {
    ref_len = first_eos(a.ref, a.R, a.ref_st, roff, a.eos);
    hyp_len = first_eos(a.hyp, a.H, a.hyp_st, hoff, a.eos);
    if (a.include_eos) {
      if (ref_len == a.R) rmiss = true; else ref_len += 1;
      if (hyp_len == a.H) hmiss = true; else hyp_len += 1;
    }
  }
  int Heff = a.exclude_last ? hyp_len - 1 : hyp_len;  // rows that are updated (:286-288)
  if (Heff < 0) Heff = 0;
  // bit-vectors along the hypothesis (only its first Heff tokens matter), reference consumed;
  // the other way round for optimal completion, whose row minima run along the reference
  const bool oc = a.oc != 0;
  const int64_t *x = oc ? a.ref : a.hyp, *y = oc ? a.hyp : a.ref;
  const int64_t x_st = oc ? a.ref_st : a.hyp_st, y_st = oc ? a.hyp_st : a.ref_st;
  const int64_t xoff = oc ? roff : hoff, yoff = oc ? hoff : roff;
  const int x_len = oc ? ref_len : Heff, y_len = oc ? Heff : ref_len;

  // ---- distinct tokens of X in ascending order (lev_classes.hpp) ---------------------------
  // (vocabulary indices below kDirectBits: ranks from a presence map, no sort -- lev_classes.hpp;
  // anything else: the sorted table and binary searches.  The classes are the same numbers.)
  int64_t xt[NR];
  load_sequence<NR>(x, x_len, x_st, xoff, xt);
  const bool direct = tokens_are_small<NR>(x_len, xt);
  int U, lgP = 0;
  int xc[NR];  // classes of X[lane + 64 q]
  if (direct) {
    U = presence_map<NR>(x_len, xt, pmap);
    if (oc) tokens_from_map(pmap, a.class_tokens + n * (int64_t)a.R);
    classes_from_map<NR>(pmap, xt, xc);
#pragma unroll
    for (int q = 0; q < NR; ++q) xc[q] = lane + q * PDT_WAVE < x_len ? xc[q] : -1;
  } else {
    U = distinct_sorted_regs<NR>(x_len, xt, ctok);
    wave_sync();
    if (oc)
      for (int k = lane; k < U; k += PDT_WAVE) a.class_tokens[n * (int64_t)a.R + k] = ctok[k];
    lgP = search_depth(U);
    classes_of<NR>(ctok, U, lgP, xt, xc);
  }
  if (oc && !PACKED) {
#pragma unroll
    for (int q = 0; q < NR; ++q)
      if (lane + q * PDT_WAVE < x_len) a.xcls[n * (int64_t)X + lane + q * PDT_WAVE] = (uint16_t)xc[q];
  }
  int cy[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // IN_PLACE: the classes of Y[lane + 64 q]
  for (int j0 = 0; j0 < y_len; j0 += 8 * PDT_WAVE) {
    int64_t yt[8];
    int c[8];
    load_tokens(y, y_len, y_st, yoff, j0, 0, yt);
    if (direct) classes_from_map<8>(pmap, yt, c);
    else classes_of<8>(ctok, U, lgP, yt, c);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (IN_PLACE) cy[q] = c[q];
      else if (j0 + lane + q * PDT_WAVE < y_len) yc[j0 + lane + q * PDT_WAVE] = (short)c[q];
    }
  }
  // The token table is dead from here on: po (kClassifyInPlace) / the mask words take it over.
  // (Only that overlay needs po zeroed this late; for the standalone kernel, whose po is a region of
  // its own, the place is as good as any.)
  wave_sync();
  if (PACKED) {
    for (int k = lane; k < U; k += PDT_WAVE) po32[k] = 0u;
#pragma unroll
    for (int q = 0; q < NR; ++q)
      if (lane + q * PDT_WAVE < x_len) yc[lane + q * PDT_WAVE] = (short)xc[q];
  } else {
    for (int k = lane; k < U; k += PDT_WAVE) po[k] = make_uint2(0u, 0u);
  }
  for (int i = lane; i <= x_len; i += PDT_WAVE) msk[i] = 0u;
  wave_sync();
  auto for_x = [&](auto &&f) {  // f(position, class) over this lane's positions of X
#pragma unroll
    for (int q = 0; q < NR; ++q)
      if (lane + q * PDT_WAVE < x_len) f(lane + q * PDT_WAVE, xc[q]);
  };
  for_x([&](const int i, const int c) {  // blocks that hold the class
    if (PACKED) atomicOr(&po32[c], 1u << (i >> 5));
    else atomicOr(&po[c].x, 1u << (i >> 5));
  });
  wave_sync();
  {  // offsets = exclusive scan of the presence popcounts
    const int B = (U + PDT_WAVE - 1) / PDT_WAVE;
    const int i0 = lane * B;
    auto presence = [&](const int k) { return PACKED ? po32[k] : po[k].x; };
    int sum = 0;
    for (int q = 0; q < B; ++q)
      if (i0 + q < U) sum += __popc(presence(i0 + q));
    const int incl = wave_incl_scan_add(sum);
    int pos = incl - sum;
    for (int q = 0; q < B; ++q)
      if (i0 + q < U) {
        const int cnt = __popc(presence(i0 + q));
        if (PACKED) po32[i0 + q] |= (unsigned)pos << 16;
        else po[i0 + q].y = (unsigned)pos;
        pos += cnt;
      }
  }
  wave_sync();
  for_x([&](const int i, const int c) {
    uint2 e;
    if (PACKED) e = make_uint2(po32[c] & 0xffffu, po32[c] >> 16);
    else e = po[c];
    atomicOr(&msk[e.y + (unsigned)__popc(e.x & ((1u << (i >> 5)) - 1u))], 1u << (i & 31));
  });
  wave_sync();
  if (PACKED) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (lane + q * PDT_WAVE < y_len) yh32[lane + q * PDT_WAVE] = cy[q] >= 0 ? po32[cy[q]] : 0u;
    if (y_len == 0 && lane == 0) yh32[0] = 0u;  // (the entry the clamped look-ups read)
  } else if (IN_PLACE) {  // yh over po: every look-up is in a register before the first entry is written
    uint2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
      v[q] = (lane + q * PDT_WAVE < y_len && cy[q] >= 0) ? po[cy[q]] : make_uint2(0u, 0u);
    wave_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (lane + q * PDT_WAVE < y_len) yh_l[lane + q * PDT_WAVE] = v[q];
    if (y_len == 0 && lane == 0) yh_l[0] = make_uint2(0u, 0u);  // (the entry the clamped look-ups read)
  }
  if (lane == 0) {
    int flags = 0;
    if (rmiss) flags |= PDT_WARN_REF_NO_EOS;
    if (hmiss) flags |= PDT_WARN_HYP_NO_EOS;
    if (a.norm && ref_len == 0) flags |= PDT_WARN_EMPTY_REF;
    if (flags && a.status) atomicOr(a.status, flags);
    if (a.ref_lens_out) a.ref_lens_out[n] = ref_len;
    if (a.hyp_lens_out) a.hyp_lens_out[n] = hyp_len;
  }
  return Classified{ref_len, hyp_len, x_len, y_len};
}

}  // namespace pdt
