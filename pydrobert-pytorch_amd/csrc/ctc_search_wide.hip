// pdt_ctc_prefix_search_wide[_elem] -- CTCPrefixSearch(width)(logits, lens) without a language model, logits
// of float32, float16 or bfloat16
// (reference _decoding.py:1064-1202) for beams of up to 128 prefixes, every frame in ONE launch: the
// persistent form of ctc_advance_wide_kernel (advance_wide.hip).  One workgroup of eight waves per
// utterance loops over that utterance's frames; workgroups never wait on one another (no ring, no
// spin-wait, no cross-workgroup synchronisation of any kind: every wait is a workgroup barrier).
//
// Per frame: the softmax of the row (max, exp(x - max), times 1 / sum: the narrow kernels'
// expressions) into a row of probabilities -- LDS when it fits, else this utterance's row of the
// workspace; the masses NB / B of the old entries with the merged extensions added in index order of
// k (:804-837); block_top_k over the flat candidates k * V + v followed by the K' non-extensions
// (ties to the lowest flat index); the new entries; the is-prefix relation of the new beam.
//
// The beam state stays in LDS between frames: nb, b, last token, length, trie node per entry and the
// is-prefix relation as bit rows (two 64-bit words per entry).  There are no dense histories.  A
// prefix is a node of a trie in the workspace -- one (parent node, token) record per frame and beam
// entry, node t * W + j, the narrow search's layout -- and what the step kernel reads from y_prev is
// answered without it:
//   * the token that turns prefix k into prefix k' (CtcWide::need) is only wanted when
//     len(k) + 1 == len(k'), where it is the last token of k';
//   * "the token of new prefix b at position len(a)" of the is-prefix update (:883-898) comes from a
//     next-token table nxt[a][b], defined where a is a strict prefix of b, rebuilt from the old one
//     every frame (ctc_frame.hpp does the same for up to 32 entries inside a wave).  One case is out
//     of the old table's reach: a is an extension whose prefix was NOT in the old beam but is an
//     inner prefix of a longer entry's source (a re-created intermediate prefix); then the token is
//     read off the trie, walking up from that source's node.
// nxt is int32, W * W entries, two copies: in LDS up to width 64 (32 KB), in the workspace (L2
// resident, 128 KB per utterance at width 128) beyond.
//
// Degenerate beams: a selected candidate of mass -inf (a merged extension, or anything drawn from an
// absent entry, when a frame has fewer than `width` real candidates) is an ABSENT entry: masses -inf,
// length 0, no trie node, related to nothing.  An absent entry's candidates are all -inf, so NaN
// never appears (the step kernel would form -inf * 0 there).
//
// At the end every entry walks its parents and writes its column of y; rows at and beyond a
// prefix's length are written 0.
#include "ctc_ring.hpp"
#include "wide_select.hpp"

namespace pdt {

constexpr int kWideMaxWidth = 128;
#ifndef PDT_WIDE_NXT_LDS_WIDTH  // (diagnostic builds move the boundary)
#define PDT_WIDE_NXT_LDS_WIDTH 64
#endif
constexpr int kWideNxtLdsWidth = PDT_WIDE_NXT_LDS_WIDTH;  // widths up to this keep the next-token tables in LDS

struct CtcWideArgs {
  const void *logits; int64_t lg_st, lg_sn, lg_sv;   // (T, N, V + 1) of the kernel's element type
  const int64_t *lens;                               // (N,) or null
  int T, N, V, W, S;
  int64_t *y;       // (S, N, W)
  int64_t *y_lens;  // (N, W)
  float *y_probs;   // (N, W)
  int2 *trie;       // (N, T, W): (parent node, token)
  int *nxt;         // (N, 2, W, W) for widths above kWideNxtLdsWidth
  float *rows;      // (N, row_stride) for rows that do not fit the LDS
  int64_t row_stride;
};

// Dynamic LDS: the selection scratch, the bit rows (2 sets x W x 16 bytes), 13 arrays of W words
// (nb, b, NB, B, last, len, node; source, length, kind, token, last token, node of the new
// entries), the per-wave lists of merged tokens, 16 words of reduction scratch; then the row and
// the next-token tables where they are held here.
struct CtcWideLds {
  size_t fixed, total;
  bool row_lds, nxt_lds;
};
__host__ inline CtcWideLds ctc_wide_lds(int V, int W) {
  CtcWideLds l;
  l.fixed = WideSel::bytes(W) + (size_t)W * (32 + 13 * 4 + 4 * kWideWaves) + 64;
  l.nxt_lds = W <= kWideNxtLdsWidth;
  const size_t nxt = l.nxt_lds ? (size_t)2 * W * W * 4 : 0;
  l.row_lds = l.fixed + nxt + ((size_t)V + 1) * 4 <= 96 * 1024;
  l.total = (l.fixed + nxt + (l.row_lds ? ((size_t)V + 1) * 4 : 0) + 15) & ~(size_t)15;
  return l;
}

template <typename T>
__host__ __device__ __forceinline__ T *carve_as(void *p) {
  return __builtin_bit_cast(T *, p);
}

#ifdef PDT_WIDE_WALKS  // diagnostic build (profiles/tools/count_wide_walks.py): trie walks of the next-token update
__device__ unsigned long long g_wide_walks;
#endif

// bit b of entry a's row: a is a prefix of b
__device__ __forceinline__ bool wide_rel(const u64 *bits, int a, int b) { return (bits[2 * a + (b >> 6)] >> (b & 63)) & 1ull; }

// E: the logits' element type (float32, float16, bfloat16), widened exactly where the frame's row is read
// (pdt_common.hpp: elem_load); the row of float32 values in LDS or the workspace and all behind it are one code.
template <bool ROW_LDS, typename E = float>
__global__ void __launch_bounds__(kWideThreads) ctc_search_wide_kernel(const CtcWideArgs a, const int nxt_in_lds) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const int64_t n = blockIdx.x;
  const int V = a.V, W = a.W;
  WideSel sel;
  u64 *isp = carve_as<u64>(sel.carve(smem, W));
  u64 *isp_new = isp + 2 * W;
  float *nb = carve_as<float>(isp_new + 2 * W), *b = nb + W, *NB = b + W, *B = NB + W;
  int *last = carve_as<int>(B + W), *len = last + W, *node = len + W;
  int *o_src = node + W, *o_len = o_src + W, *o_non = o_len + W, *o_tok = o_non + W, *o_last = o_tok + W, *o_node = o_last + W;
  int *merged = o_node + W + wave * W;  // this wave's list of merged tokens of the row at hand
  float *red = carve_as<float>(o_node + W + kWideWaves * W);
  float *tail = red + 16;
  float *row = ROW_LDS ? tail : a.rows + n * a.row_stride;
  int *nxt_old = nxt_in_lds ? carve_as<int>(tail + (ROW_LDS ? V + 1 : 0)) : a.nxt + n * 2 * W * W;
  int *nxt_new = nxt_old + W * W;
  int2 *trie = a.trie + n * (int64_t)a.T * W;

  // one empty prefix, all of its mass on "ends in blank" (:1097-1105); the rest of the beam absent
  for (int k = tid; k < W; k += kWideThreads) {
    nb[k] = k == 0 ? 0.0f : -PDT_INF;
    b[k] = k == 0 ? 1.0f : -PDT_INF;
    last[k] = 0;
    len[k] = 0;
    node[k] = -1;
    isp[2 * k] = k == 0 ? 1ull : 0ull;
    isp[2 * k + 1] = 0ull;
  }
  int Tn = a.T;
  if (a.lens) Tn = (int)min((int64_t)Tn, max(a.lens[n], (int64_t)0));
  Tn = min(Tn, a.S);
  int Kp = 1;
  __syncthreads();

#pragma unroll 1
  for (int t = 0; t < Tn; ++t) {
    // ---- the frame's softmax (:1093), blank = index V ----
    const E *lg = static_cast<const E *>(a.logits) + (int64_t)t * a.lg_st + n * a.lg_sn;
    float mx = -PDT_INF;
    for (int v = tid; v <= V; v += kWideThreads) {
      const float x = elem_load(&lg[(int64_t)v * a.lg_sv]);
      row[v] = x;
      mx = fmaxf(mx, x);
    }
    mx = wave_max_f(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < kWideWaves; ++w) mx = fmaxf(mx, red[w]);
    float s = 0.0f;
    for (int v = tid; v <= V; v += kWideThreads) {
      const float e = exp_nonpos(row[v] - mx);
      row[v] = e;
      s += e;
    }
    s = wave_sum_f(s);
    if (lane == 0) red[8 + wave] = s;
    __syncthreads();
    s = red[8];
    for (int w = 1; w < kWideWaves; ++w) s += red[8 + w];
    const float inv0 = __builtin_amdgcn_rcpf(s);  // reciprocal + one Newton step, as ctc_search.hip
    const float inv = __builtin_fmaf(__builtin_fmaf(-s, inv0, 1.0f), inv0, inv0);
    for (int v = tid; v <= V; v += kWideThreads) row[v] = row[v] * inv;
    __syncthreads();

    // ---- masses of the old entries (:777-794) with the merged extensions (:804-831) ----
    const float blank = row[V];
    for (int kp = tid; kp < Kp; kp += kWideThreads) {
      float nbv = -PDT_INF, bv = -PDT_INF;
      if (b[kp] > -PDT_INF) {
        const int lt = last[kp], lk1 = len[kp] - 1;
        const float p = row[lt];
        float add = 0.0f;
        for (int k = 0; k < Kp; ++k)  // summed over k in index order
          if (len[k] == lk1 && wide_rel(isp, k, kp)) add += ((lt == last[k] ? 0.0f : nb[k]) + b[k]) * p;
        nbv = nb[kp] * p + add;
        bv = (nb[kp] + b[kp]) * blank;
      }
      NB[kp] = nbv;
      B[kp] = bv;
    }
    __syncthreads();

    // ---- the K best of the Kp * V extensions and Kp non-extensions (:842-846) ----
    const int K = (int)min((int64_t)W, (int64_t)Kp * (V + 1));
    int k0, k1;
    wave_rows(Kp, k0, k1);
    auto scan = [&](auto &&f) {
      for (int k = k0; k < k1; ++k) {
        int nm = 0;
        const int lk1 = len[k] + 1;
        for (int q0 = 0; q0 < Kp; q0 += PDT_WAVE) {
          const int kp = q0 + lane;
          const bool ex = kp < Kp && len[kp] == lk1 && ((isp[2 * k + (q0 >> 6)] >> lane) & 1ull);
          const int tm = ex ? last[kp] : 0;  // the token that turns prefix k into prefix k'
          const u64 bal = __ballot(ex);
          if (ex) merged[nm + lanes_below(bal)] = tm;
          nm += (int)__popcll(bal);
        }
        wave_sync();
        const float wn = nb[k], wb = b[k];
        const bool present = wb > -PDT_INF;
        const int lk = last[k];
        for (int v0 = 0; v0 < V; v0 += 4 * PDT_WAVE) {
          float x[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int v = v0 + q * PDT_WAVE + lane;
            x[q] = v < V ? row[v] : 0.0f;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int v = v0 + q * PDT_WAVE + lane;
            if (v0 + q * PDT_WAVE < V) {
              float e = present ? ((v == lk ? 0.0f : wn) + wb) * x[q] : -PDT_INF;
              for (int j = 0; j < nm; ++j)
                if (merged[j] == v) e = -PDT_INF;  // :833-837
              f(fkey(e + 0.0f), (unsigned)(k * V + v), v < V);
            }
          }
        }
        wave_sync();
      }
      if (wave == kWideWaves - 1)  // the non-extensions come last in the flat order
        for (int q0 = 0; q0 < Kp; q0 += PDT_WAVE) {
          const int k = q0 + lane;
          f(fkey(k < Kp ? (NB[k] + B[k]) + 0.0f : 0.0f), (unsigned)(Kp * V + k), k < Kp);
        }
    };
    block_top_k(K, scan, sel);

    // ---- the new entries (:849-880); an extension adds a record to the trie ----
    for (int j = tid; j < W; j += kWideThreads) {
      const u64 e = j < K ? sel.sorted[j] : 0ull;
      const bool valid = j < K && key_of(e) > fkey(-PDT_INF);
      const int ind = valid ? (int)idx_of(e) : 0;
      const bool non = ind >= Kp * V;
      const int src = non ? ind - Kp * V : ind / V;
      const int tok = non ? 0 : ind - src * V;
      o_src[j] = valid ? src : -1;
      o_len[j] = valid ? len[src] + (non ? 0 : 1) : 0;
      o_non[j] = non ? 1 : 0;
      o_tok[j] = tok;
      o_last[j] = valid ? (non ? last[src] : tok) : 0;
      o_node[j] = valid ? (non ? node[src] : t * W + j) : -1;
      if (valid && !non) trie[t * W + j] = make_int2(node[src], tok);
      nb[j] = valid ? (non ? NB[src] : fkey_inv(key_of(e))) : -PDT_INF;
      b[j] = valid ? (non ? B[src] : 0.0f) : -PDT_INF;
    }
    __syncthreads();

    // ---- is-prefix relation and next-token table of the new beam (:883-898) ----
    // A wave takes (new entry x, 64 new entries y) at a time; the ballot is the bit word.
    for (int task = wave; task < 2 * W; task += kWideWaves) {
      const int x = task >> 1, wd = task & 1, y = wd * PDT_WAVE + lane;
      const int sx = o_src[x];
      bool ok = false;
      if (sx >= 0 && y < W) {
        const int sy = o_src[y];
        const int la = o_len[x], lb = o_len[y];
        if (sy >= 0 && la <= lb && wide_rel(isp, sx, sy)) {
          const int p = len[sx], lsy = len[sy];  // p <= lsy: sx is a prefix of sy
          const bool xnon = o_non[x] != 0;
          // token of new prefix y at position p (none: y is sy itself and no longer than sx)
          const int tok_at = lsy > p ? nxt_old[sx * W + sy] : (o_non[y] ? -1 : o_tok[y]);
          ok = xnon || tok_at == o_tok[x];
          if (ok && la < lb) {  // strict prefix: the token that follows x inside y
            int nx;
            if (xnon) {
              nx = tok_at;
            } else if (lsy == p + 1) {
              nx = o_tok[y];  // y = (new prefix x) + its token
            } else {
              // rare: x re-creates an inner prefix of sy that the old beam did not hold.  Token of
              // sy at position la = token of the ancestor of sy's node at depth la + 1.
              int nd = node[sy];
#ifdef PDT_WIDE_WALKS
              atomicAdd(&g_wide_walks, 1ull);
#endif
              for (int depth = lsy; depth > la + 1 && nd >= 0; --depth) nd = trie[nd].x;
              nx = nd >= 0 ? trie[nd].y : -1;
            }
            nxt_new[x * W + y] = nx;
          }
        }
      }
      const u64 bal = __ballot(ok);
      if (lane == 0) isp_new[2 * x + wd] = bal;
    }
    __syncthreads();
    for (int j = tid; j < W; j += kWideThreads) {
      last[j] = o_last[j];
      len[j] = o_len[j];
      node[j] = o_node[j];
    }
    {
      u64 *tb = isp; isp = isp_new; isp_new = tb;
      int *tn = nxt_old; nxt_old = nxt_new; nxt_new = tn;
    }
    Kp = W;
    __syncthreads();
  }

  // ---- outputs (:1188-1200): probabilities, lengths, and the prefixes read off the trie ----
  for (int j = tid; j < W; j += kWideThreads) {
    a.y_probs[n * W + j] = nb[j] + b[j];
    a.y_lens[n * W + j] = len[j];
    int nd = node[j];
    for (int pos = len[j] - 1; pos >= 0 && nd >= 0; --pos) {
      const int2 rec = trie[nd];
      a.y[((int64_t)pos * a.N + n) * W + j] = rec.y;
      nd = rec.x;
    }
  }
  for (int64_t idx = tid; idx < (int64_t)a.S * W; idx += kWideThreads) {
    const int pos = (int)(idx / W), j = (int)(idx - (int64_t)pos * W);
    if (pos >= len[j]) a.y[((int64_t)pos * a.N + n) * W + j] = 0;
  }
}

template <bool ROW_LDS, typename E = float>
static int launch_ctc_search_wide_p(const CtcWideArgs &a, const CtcWideLds &l, hipStream_t stream) {
  if (const int rc = set_lds(ctc_search_wide_kernel<ROW_LDS, E>, l.total)) return rc;
  hipLaunchKernelGGL((ctc_search_wide_kernel<ROW_LDS, E>), dim3((unsigned)a.N), dim3(kWideThreads), l.total, stream, a,
                     l.nxt_lds ? 1 : 0);
  return (int)hipGetLastError();
}

static inline int64_t wide_align(int64_t x) { return (x + 255) & ~(int64_t)255; }
static inline int64_t wide_row_stride(int64_t V) { return (V + 1 + 63) & ~(int64_t)63; }
static inline int64_t wide_trie_bytes(int64_t T, int64_t N, int64_t W) { return wide_align(T * N * W * (int64_t)sizeof(int2)); }
static inline int64_t wide_nxt_bytes(int64_t N, int64_t W) { return W > kWideNxtLdsWidth ? wide_align(N * 2 * W * W * 4) : 0; }

}  // namespace pdt

extern "C" {

// the trie, the next-token tables of widths beyond 64, a row of probabilities per utterance (used
// by rows beyond the LDS; a few KB otherwise)
int64_t pdt_ctc_prefix_search_wide_workspace_bytes(int64_t T, int64_t N, int64_t V, int64_t width) {
  if (T < 0 || N < 0 || V < 1 || width < 1 || width > pdt::kWideMaxWidth || V >= (1 << 30)) return 0;
  return pdt::wide_trie_bytes(T, N, width) + pdt::wide_nxt_bytes(N, width) + pdt::wide_align(N * pdt::wide_row_stride(V) * 4) + 256;
}

int pdt_ctc_prefix_search_wide_plan(int64_t V, int64_t width, int32_t *plan2) {
  if (V < 1 || width < 1 || !plan2) return PDT_E_ARG;
  if (width > pdt::kWideMaxWidth || V >= (1 << 30) || width * (V + 1) >= (1ll << 31)) return PDT_E_TOO_LONG;
  const pdt::CtcWideLds l = pdt::ctc_wide_lds((int)V, (int)width);
  if (l.total > 160 * 1024) return PDT_E_TOO_LONG;
  plan2[0] = l.row_lds ? 1 : 0;
  plan2[1] = l.nxt_lds ? 1 : 0;
  return PDT_OK;
}

int pdt_ctc_prefix_search_wide_elem(const void *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                                    int64_t lg_sn, int64_t lg_sv, const int64_t *lens, int64_t width,
                                    int64_t S, int64_t *y, int64_t *y_lens, float *y_probs,
                                    void *workspace, void *stream, int elem) {
  using namespace pdt;
  if (T < 0 || N < 0 || V < 1 || width < 1 || S < 0) return PDT_E_ARG;
  if (const int rc = elem_status(elem)) return rc;
  if (N == 0) return PDT_OK;
  if (!y_lens || !y_probs || (T > 0 && (!logits || !workspace)) || (S > 0 && !y)) return PDT_E_ARG;
  if (width > kWideMaxWidth) return PDT_E_TOO_LONG;
  if (T * width >= (1ll << 31) || V >= (1 << 30) || N >= (1ll << 31) || T >= (1 << 24)) return PDT_E_TOO_LONG;
  if (width * (V + 1) >= (1ll << 31)) return PDT_E_TOO_LONG;
  const CtcWideLds l = ctc_wide_lds((int)V, (int)width);
  if (l.total > 160 * 1024) return PDT_E_TOO_LONG;
  CtcWideArgs a{};
  a.logits = logits; a.lg_st = lg_st; a.lg_sn = lg_sn; a.lg_sv = lg_sv;
  a.lens = lens;
  a.T = (int)T; a.N = (int)N; a.V = (int)V; a.W = (int)width; a.S = (int)S;
  a.y = y; a.y_lens = y_lens; a.y_probs = y_probs;
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  a.trie = carve_as<int2>(ws);
  a.nxt = carve_as<int>(ws + wide_trie_bytes(T, N, width));
  a.rows = carve_as<float>(ws + wide_trie_bytes(T, N, width) + wide_nxt_bytes(N, width));
  a.row_stride = wide_row_stride(V);
  if (elem == 2)
    return l.row_lds ? launch_ctc_search_wide_p<true, f16_t>(a, l, (hipStream_t)stream)
                     : launch_ctc_search_wide_p<false, f16_t>(a, l, (hipStream_t)stream);
  if (elem == 3)
    return l.row_lds ? launch_ctc_search_wide_p<true, bf16_t>(a, l, (hipStream_t)stream)
                     : launch_ctc_search_wide_p<false, bf16_t>(a, l, (hipStream_t)stream);
  if (l.row_lds) return launch_ctc_search_wide_p<true>(a, l, (hipStream_t)stream);
  return launch_ctc_search_wide_p<false>(a, l, (hipStream_t)stream);
}

int pdt_ctc_prefix_search_wide(const float *logits, int64_t T, int64_t N, int64_t V, int64_t lg_st,
                               int64_t lg_sn, int64_t lg_sv, const int64_t *lens, int64_t width,
                               int64_t S, int64_t *y, int64_t *y_lens, float *y_probs,
                               void *workspace, void *stream) {
  return pdt_ctc_prefix_search_wide_elem(logits, T, N, V, lg_st, lg_sn, lg_sv, lens, width, S, y, y_lens, y_probs,
                                         workspace, stream, 0);
}

}  // extern "C"

#ifdef PDT_WIDE_WALKS
extern "C" int pdt_debug_read_wide_walks(unsigned long long *host, int reset) {
  hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(pdt::g_wide_walks), sizeof(unsigned long long));
  if (e == hipSuccess && reset) {
    const unsigned long long z = 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(pdt::g_wide_walks), &z, sizeof(z));
  }
  return (int)e;
}
#endif
