// Phase 2 of optimal completion (pdt_oc_expand) for references of up to 2 048 tokens: the class
// bitmasks of pdt_oc_mask -> padded ascending token lists (reference _string.py:509-514).  Three
// kernels, fastest first, and the launcher that picks among them by the layout of the targets:
//   oc_expand_runs_kernel   a workgroup owns 64 / Wp utterances for a range of h (W <= 16, even C,
//                           utterances contiguous at one h): the operator's own case;
//   oc_expand_tiles_kernel  contiguous runs of rows along n or along h, through an LDS image;
//   oc_expand_kernel        one workgroup per utterance, a row at a time: any strides.
// (Longer references: oc_expand_generic_kernel, lev_generic.hip.)
#include "lev_launch.hpp"

namespace pdt {

// ---- row-at-a-time form ----------------------------------------------------------------------
// One workgroup per utterance: the class-token table is staged once in LDS, the four waves take
// rows h = wave, wave + 4, ... and keep the next row's bitmask word in flight while the current
// row is expanded and written (C * 8 contiguous bytes per row).
__global__ void __launch_bounds__(256)
oc_expand_kernel(const uint32_t *__restrict__ bitmask, const int64_t *__restrict__ class_tokens,
                 int R, int W, int Hout, int64_t N, int C, int64_t padding,
                 int64_t *__restrict__ targets, int64_t tgt_sh, int64_t tgt_sn) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int64_t n = xcd_remap(blockIdx.x, gridDim.x);
  int64_t *ctok = reinterpret_cast<int64_t *>(smem);
  int64_t *stage = ctok + R + (size_t)wave * W * 32;
  for (int k = (int)threadIdx.x; k < R; k += 256) ctok[k] = class_tokens[n * (int64_t)R + k];
  __syncthreads();
  const bool wide = (C & 1) == 0 && ((tgt_sh | tgt_sn) & 1) == 0 &&
                    (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
  unsigned w_next = (wave < Hout && lane < W) ? bitmask[((int64_t)wave * N + n) * W + lane] : 0u;
  for (int h = wave; h < Hout; h += 4) {
    unsigned w = w_next;
    if (h + 4 < Hout && lane < W) w_next = bitmask[((int64_t)(h + 4) * N + n) * W + lane];
    const int cnt = __popc(w);
    const int incl = wave_incl_scan_add(cnt);
    const int total = __builtin_amdgcn_readlane(incl, PDT_WAVE - 1);
    int pos = incl - cnt;
    while (w) {
      const int b = __builtin_ctz(w);
      w &= w - 1u;
      stage[pos++] = ctok[lane * 32 + b];
    }
    wave_sync();
    int64_t *dst = targets + (int64_t)h * tgt_sh + n * tgt_sn;
    if (wide) {  // 16-byte stores: two targets per lane
      for (int i = lane; i < (C >> 1); i += PDT_WAVE) {
        longlong2 v;
        v.x = 2 * i < total ? stage[2 * i] : padding;
        v.y = 2 * i + 1 < total ? stage[2 * i + 1] : padding;
        *reinterpret_cast<longlong2 *>(dst + 2 * i) = v;
      }
    } else {
      for (int i = lane; i < C; i += PDT_WAVE) dst[i] = i < total ? stage[i] : padding;
    }
    wave_sync();
  }
}

// ---- tiled form ------------------------------------------------------------------------------
// Two things hold the row-at-a-time form at 3.6 TB/s (measured, profiles/microbench `stores`):
// a row is C * 8 bytes (992 at the bench shape), so almost every store instruction starts and
// ends inside a 128-byte line (62-lane stores of such rows: 3.4 TB/s whatever their order, against
// 5.5-6.2 for whole KiB); and vmcnt counts loads and stores together, in order, so a wave that
// loads the next bitmask words after storing a row waits for that store to reach memory.
// Here (a) the rows of NB consecutive utterances at one h -- or, batch-first, of NB consecutive h
// of one utterance -- are ONE contiguous run of NB * C * 8 bytes: a wave expands them into an LDS
// image of the run and streams it out with 16-byte stores, 1 KiB of consecutive bytes per
// instruction; (b) a workgroup loads every bitmask word and class-token table it will need into
// LDS up front, so its main loop issues no global load at all and never waits for a store.
//   over_n = 1: tile = utterances n0 .. n0 + NB at one h; the workgroup owns `chunk` values of h
//               and its four waves take them in turn;
//   over_n = 0: tile = rows h0 .. h0 + NB of one utterance (one table); the workgroup owns
//               `chunk` tiles.
// A pass expands 64 / Wp rows at once (Wp = bitmask words per row rounded up to a power of two:
// lane = (row, word)); positions inside a row come from one wave scan minus the scan value at
// the row's first lane.  The image holds int32 indices into the token tables (-1 = padding), so
// the per-bit loop only writes LDS and the tokens are looked up on the way out by all 64 lanes.
struct OcTileArgs {
  const uint32_t *bitmask;
  const int64_t *class_tokens;
  int64_t *targets;
  int64_t N, padding, outer_stride;  // outer_stride: elements between tiles' outer index
  int R, W, lgWp, Hout, C, NB, over_n, chunk, ntiles, wide;
  int nw;  // waves per workgroup
};

__host__ __device__ inline size_t oc_tile_lds(int R, int W, int C, int NB, int over_n, int chunk, int nw,
                                              size_t *bm_off, size_t *stage_off) {
  const size_t ctok = (((size_t)(over_n ? NB : 1) * R + 1) & ~(size_t)1) * 8;
  const size_t bm = (((size_t)chunk * NB * W + 3) & ~(size_t)3) * 4;  // rows of the chunk x W words
  const size_t stage = (((size_t)NB * C + 3) & ~(size_t)3) * 4;
  if (bm_off) *bm_off = ctok;
  if (stage_off) *stage_off = ctok + bm;
  return ctok + bm + (size_t)nw * stage;
}

constexpr int kOcTileRows = 4;     // rows per tile (the measurement is with launch_oc_expand)
constexpr int kOcTileHChunk = 64;  // over_n: values of h per table load

template <int NW>
__global__ void __launch_bounds__(NW * PDT_WAVE) oc_expand_tiles_kernel(const OcTileArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int C = a.C, NB = a.NB, W = a.W, R = a.R;
  size_t bm_off, stage_off;
  constexpr int kOcWaves = NW, kOcThreads = NW * PDT_WAVE;
  oc_tile_lds(R, W, C, NB, a.over_n, a.chunk, a.nw, &bm_off, &stage_off);
  int64_t *ctok = reinterpret_cast<int64_t *>(smem);
  unsigned *bm = reinterpret_cast<unsigned *>(smem + bm_off);
  int *stage = reinterpret_cast<int *>(smem + stage_off) + (size_t)wave * (((size_t)NB * C + 3) & ~(size_t)3);
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  // over_n: item = (h chunk, n tile); else item = (utterance, chunk of h tiles)
  const int inner_items = a.over_n ? a.ntiles : (a.ntiles + a.chunk - 1) / a.chunk;
  const int64_t outer = item / inner_items;
  const int inner = (int)(item - outer * inner_items);
  const int64_t n_first = a.over_n ? (int64_t)inner * NB : outer;
  const int tabs_valid = a.over_n ? (int)min((int64_t)NB, a.N - n_first) : 1;
  // the h rows this workgroup covers, and (over_n) the utterances of its tile
  const int h_base = a.over_n ? (int)outer * a.chunk : inner * a.chunk * NB;
  const int h_count = min(a.Hout - h_base, a.over_n ? a.chunk : a.chunk * NB);
  // (eight loads in flight per thread: left to itself the compiler waits for every load before
  // the LDS write that follows it, and a workgroup's preamble becomes 32 round trips to L2)
  {  // the tables of consecutive utterances are one contiguous block of class_tokens
    const int64_t *src = a.class_tokens + n_first * (int64_t)R;
    const int total = tabs_valid * R;
    for (int k0 = (int)threadIdx.x; k0 < total; k0 += kOcThreads * 8) {
      int64_t v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = k0 + q * kOcThreads < total ? src[k0 + q * kOcThreads] : 0;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (k0 + q * kOcThreads < total) ctok[k0 + q * kOcThreads] = v[q];
    }
  }
  {  // bm[(hi * tabs_valid + u) * W + word]: tabs_valid * W consecutive words per h
    const int per_h = tabs_valid * W, total = h_count * per_h;
    for (int k0 = (int)threadIdx.x; k0 < total; k0 += kOcThreads * 8) {
      unsigned v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int k = k0 + q * kOcThreads;
        const int hi = k / per_h, r = k - hi * per_h;
        v[q] = k < total ? a.bitmask[((int64_t)(h_base + hi) * a.N + n_first) * W + r] : 0u;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (k0 + q * kOcThreads < total) bm[k0 + q * kOcThreads] = v[q];
    }
  }
  __syncthreads();  // from here on: LDS reads and global stores only
  const int Wp = 1 << a.lgWp, rows_per_pass = PDT_WAVE >> a.lgWp;
  const int ur = lane >> a.lgWp, word = lane & (Wp - 1);
  const int seg = lane & ~(Wp - 1);
  // the jobs of this wave: over_n -> h = h_base + wave, + 4, ...; else tiles of NB rows
  const int j_end = a.over_n ? h_base + h_count : min(a.ntiles, (inner + 1) * a.chunk);
  for (int j = (a.over_n ? h_base : inner * a.chunk) + wave; j < j_end; j += kOcWaves) {
    const int h_first = a.over_n ? j : j * NB;
    const int rows = a.over_n ? tabs_valid : min(NB, a.Hout - h_first);
    // image of the run as indices into the class-token tables: -1 (padding) everywhere, then
    // the classes of every row
    {
      const int4 neg = make_int4(-1, -1, -1, -1);
      int4 *s4 = reinterpret_cast<int4 *>(stage);
      for (int i = lane; i < (rows * C + 3) >> 2; i += PDT_WAVE) s4[i] = neg;
    }
    wave_sync();
    for (int u0 = 0; u0 < rows; u0 += rows_per_pass) {
      const int u = u0 + ur;
      const bool live = u < rows && word < W;
      // row (h, n) of the chunk: over_n -> (h_first, u), else (h_first + u, the utterance)
      const int row = a.over_n ? (h_first - h_base) * tabs_valid + u : h_first - h_base + u;
      unsigned w = live ? bm[row * W + word] : 0u;
      const int cnt = __popc(w);
      const int incl = wave_incl_scan_add(cnt);
      const int before = __builtin_amdgcn_ds_bpermute((seg > 0 ? seg - 1 : 0) << 2, incl);
      int pos = incl - cnt - (seg > 0 ? before : 0);
      const int tab = (a.over_n ? u : 0) * R + word * 32;
      int *srow = stage + u * C;
      while (w) {
        const int b = __builtin_ctz(w);
        w &= w - 1u;
        srow[pos++] = tab + b;
      }
    }
    wave_sync();
    int64_t *dst = a.targets + (a.over_n ? (int64_t)h_first * a.outer_stride + n_first * C
                                         : n_first * a.outer_stride + (int64_t)h_first * C);
    const int total = rows * C;
    auto tok_of = [&](int id) { return id < 0 ? a.padding : ctok[id]; };
    if (a.wide) {  // 16-byte stores, four in flight per lane (total is even here or the odd last
                   // element goes out alone)
      const int2 *s2 = reinterpret_cast<const int2 *>(stage);
      longlong2 *d2 = reinterpret_cast<longlong2 *>(dst);
      const int pairs = total >> 1;
      int i = lane;
      for (; i + 3 * PDT_WAVE < pairs; i += 4 * PDT_WAVE) {
        int2 id[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) id[q] = s2[i + q * PDT_WAVE];
        longlong2 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[q].x = tok_of(id[q].x);
          v[q].y = tok_of(id[q].y);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // (non-temporal: 1.95 GB written once and never read by this kernel -- 0.74 -> 0.71 ms for the operator)
          typedef long long ll2 __attribute__((ext_vector_type(2)));
          ll2 t;
          t.x = v[q].x;
          t.y = v[q].y;
          __builtin_nontemporal_store(t, reinterpret_cast<ll2 *>(&d2[i + q * PDT_WAVE]));
        }
      }
      for (; i < pairs; i += PDT_WAVE) {
        const int2 id = s2[i];
        longlong2 v;
        v.x = tok_of(id.x);
        v.y = tok_of(id.y);
        d2[i] = v;
      }
      if ((total & 1) && lane == 0) dst[total - 1] = tok_of(stage[total - 1]);
    } else {
      for (int i = lane; i < total; i += PDT_WAVE) dst[i] = tok_of(stage[i]);
    }
    // (the next tile's fill may not overtake these reads of the image: the LDS serves a wave's
    // instructions in order, so only the compiler has to be told)
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- utterance-tile form over n (W <= 16) ----------------------------------------------------
// The tiled form above reads every tile's tables once per chunk of h (nine times at the bench
// shape, ~150 MB next to 2.08 GB of writes) and starts each chunk behind a barrier.  Here a
// workgroup owns NB = 64 / Wp consecutive utterances for a range of h -- all of them unless the
// grid would leave CUs idle -- loads their class-token tables into LDS once, and after that one
// barrier its waves take the values of h in turn with nothing but the target stream in flight:
//   * the run of one h (NB rows, NB * C * 8 contiguous bytes) has ONE bitmask word per lane
//     (lane = (row, word)), fetched two values of h ahead into registers;
//   * positions come from the wave scan as in the tiled form; each set bit writes its table index
//     into a per-wave list at (row, position) -- no padding image is filled, since element (u, c)
//     of the run is a token iff c < cnt_u, with cnt_u read from the row's last lane (ds_bpermute);
//   * the way out has a fixed shape the compiler can count: per lane KB blocks of four pairs, every
//     LDS read issued (padding elements read entry 0), 16-byte non-temporal stores.
// It serves runs of at most 2 048 elements (KB <= 4) with C even, the operator's own case (C <= R);
// everything else -- C > R or odd C from the C ABI, longer references -- goes to the tiled form.
// Bench shape: 0.39 -> 0.34 ms, the fill rate of the box (EXPERIMENTS.md section 12.1).
struct OcRunArgs {
  const uint32_t *bitmask;
  const int64_t *class_tokens;
  int64_t *targets;
  int64_t N, padding, tgt_sh;
  int R, W, lgWp, Hout, C, NB, hchunk, ntiles;
  int step_u, step_c;  // a lane's next pair: (128 / C, 128 % C) elements on
};

constexpr int kOcRunWaves = 8;
constexpr int kOcRunMaxElems = 4 * 4 * 2 * PDT_WAVE;  // KB = 4 blocks of four 16-byte stores per lane

__host__ __device__ inline size_t oc_run_lds(int R, int C, int NB) {
  const size_t list = (((size_t)NB * C + 3) & ~(size_t)3) * 4;
  return (size_t)NB * R * 8 + (size_t)kOcRunWaves * list;
}

template <int KB>
__global__ void __launch_bounds__(kOcRunWaves * PDT_WAVE) oc_expand_runs_kernel(const OcRunArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NW = kOcRunWaves;
  constexpr int kThreads = NW * PDT_WAVE;
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int C = a.C, W = a.W, R = a.R, NB = a.NB, lgWp = a.lgWp;
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);  // item = (h range, tile)
  const int hc = (int)(item / (unsigned)a.ntiles);
  const int tile = (int)(item - (unsigned)hc * (unsigned)a.ntiles);
  const int64_t n_first = (int64_t)tile * NB;
  const int rows = (int)min((int64_t)NB, a.N - n_first);
  const int h_end = min(a.Hout, (hc + 1) * a.hchunk);
  int64_t *ctok = reinterpret_cast<int64_t *>(smem);
  int *list = reinterpret_cast<int *>(smem + (size_t)NB * R * 8) + (size_t)wave * (((size_t)NB * C + 3) & ~(size_t)3);
  {  // the tile's tables: one contiguous block of class_tokens, eight loads in flight per thread
    const int64_t *src = a.class_tokens + n_first * (int64_t)R;
    const int total = rows * R;
    for (int k0 = (int)threadIdx.x; k0 < total; k0 += kThreads * 8) {
      int64_t v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = k0 + q * kThreads < total ? src[k0 + q * kThreads] : 0;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (k0 + q * kThreads < total) ctok[k0 + q * kThreads] = v[q];
    }
  }
  __syncthreads();  // the only one: from here on each wave runs alone
  const int Wp = 1 << lgWp;
  const int ur = lane >> lgWp, word = lane & (Wp - 1), seg = lane & ~(Wp - 1);
  const bool live = ur < rows && word < W;
  // every lane loads, from a clamped address, so that the loads are unconditional and the
  // compiler counts them (a conditional load made it wait for all stores, vmcnt(0), every run)
  const uint32_t *bm = a.bitmask + (n_first + min(ur, rows - 1)) * W + min(word, W - 1);
  const int64_t bm_sh = a.N * W;
  const int tab = ur * R + word * 32;
  int *lrow = list + ur * C;
  const int total = rows * C;
  // the first element of this lane in the run, as (row, column)
  const int e0 = 2 * lane;
  const int u0 = e0 / C, c0 = e0 - u0 * C;
  int h = hc * a.hchunk + wave;
  const int h_last = h_end - 1;
  unsigned w_next = bm[(int64_t)min(h, h_last) * bm_sh];
  unsigned w_next2 = bm[(int64_t)min(h + NW, h_last) * bm_sh];
  for (; h < h_end; h += NW) {
    unsigned w = live ? w_next : 0u;
    w_next = w_next2;
    w_next2 = bm[(int64_t)min(h + 2 * NW, h_last) * bm_sh];
    const int cnt = __popc(w);
    const int incl = wave_incl_scan_add(cnt);
    const int prev = __builtin_amdgcn_ds_bpermute((seg > 0 ? seg - 1 : 0) << 2, incl);
    const int before = seg > 0 ? prev : 0;
    const int row_cnt = incl - before;  // cnt_u at the row's last lane
    // the word's classes into the list from both ends at once (a row's ~13 classes are neighbours,
    // mostly in one or two words: half the serial iterations)
    int lo = incl - cnt - before, hi = incl - 1 - before;
    while (w) {
      const int b0 = __builtin_ctz(w), b1 = 31 - __builtin_clz(w);
      w &= ~((1u << b0) | (1u << b1));
      lrow[lo++] = tab + b0;
      lrow[hi--] = tab + b1;  // (b0 == b1: the same slot twice)
    }
    wave_sync();
    int64_t *dst = a.targets + (int64_t)h * a.tgt_sh + n_first * C;
    int u = u0, c = c0;
    {
      // 16-byte stores (C even: a pair never straddles two rows), 4 * KB per lane, a count the
      // compiler sees; all LDS reads issued unconditionally, from index 0 for padding elements
      typedef long long ll2 __attribute__((ext_vector_type(2)));
      ll2 *d2 = reinterpret_cast<ll2 *>(dst);
      const int2 *l2 = reinterpret_cast<const int2 *>(list);
      const int pairs = total >> 1;
#pragma unroll
      for (int blk = 0; blk < KB; ++blk) {
        int k[4], cc[4];
        int2 id[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = (blk * 4 + q) * PDT_WAVE + lane;
          k[q] = __builtin_amdgcn_ds_bpermute(((u << lgWp) + Wp - 1) << 2, row_cnt);
          cc[q] = i < pairs ? c : C;
          id[q] = l2[i < pairs ? i : 0];
          u += a.step_u;
          c += a.step_c;
          if (c >= C) {
            c -= C;
            ++u;
          }
        }
        ll2 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool vx = cc[q] < k[q], vy = cc[q] + 1 < k[q];
          const int64_t tx = ctok[vx ? id[q].x : 0], ty = ctok[vy ? id[q].y : 0];
          v[q].x = vx ? tx : a.padding;
          v[q].y = vy ? ty : a.padding;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = (blk * 4 + q) * PDT_WAVE + lane;
          // (non-temporal: written once, never read back by this kernel)
          if (i < pairs) __builtin_nontemporal_store(v[q], &d2[i]);
        }
      }
    }
    // (the next h's list writes may not overtake these reads: the LDS serves a wave's instructions
    // in order, so only the compiler has to be told)
    __builtin_amdgcn_wave_barrier();
  }
}

int launch_oc_expand(const uint32_t *bitmask, const int64_t *class_tokens, int R, int Hout,
                     int64_t N, int C, int64_t padding, int64_t *targets, int64_t tgt_sh,
                     int64_t tgt_sn, hipStream_t stream) {
  const int W = (int)pdt_oc_mask_words(R);
  if (W > PDT_WAVE) return PDT_E_TOO_LONG;
  // tiled form: rows that follow each other in memory (stride C along n or along h)
  const bool over_n = tgt_sn == C, over_h = tgt_sh == C;
  // utterance-tile form: NB = 64 / Wp rows, one bitmask word per lane (4 at the bench shape),
  // 16-byte stores (C even, runs on 16 bytes), a run of NB * C <= 2 048 elements
  int lgWp = 0;
  while ((1 << lgWp) < W) ++lgWp;
  const int NB = PDT_WAVE >> lgWp;
  const bool runs = over_n && W <= 16 && N < (1ll << 31) && (C & 1) == 0 && (tgt_sh & 1) == 0 &&
                    (reinterpret_cast<uintptr_t>(targets) & 15) == 0 && (int64_t)NB * C <= kOcRunMaxElems;
  if (runs) {
    // LDS = NB tables (int64, <= 16 KiB) + one index list per wave (NB * C int32, <= 8 KiB): 31 KiB
    // at the bench shape, so four workgroups of eight waves -- 32 waves, the most a CU holds -- fit
    // on a CU (80 KiB at most: two).  The h range is split only when the tiles alone would leave
    // CUs (256 on MI355X) with fewer than two workgroups -- below N = 2 048 at NB = 4; at the bench
    // shape 1 024 tiles, one workgroup each, every table read once.
    OcRunArgs a{};
    a.bitmask = bitmask; a.class_tokens = class_tokens; a.targets = targets;
    a.N = N; a.padding = padding; a.tgt_sh = tgt_sh; a.R = R; a.W = W; a.Hout = Hout; a.C = C;
    a.lgWp = lgWp;
    a.NB = NB;
    const int64_t ntiles = (N + NB - 1) / NB;
    const int nw = kOcRunWaves;
    const int64_t want = 2 * 256;
    int64_t hsplit = ntiles >= want ? 1 : (want + ntiles - 1) / ntiles;
    hsplit = min(hsplit, (int64_t)((Hout + 2 * nw - 1) / (2 * nw)));  // >= two runs per wave
    if (hsplit < 1) hsplit = 1;
    a.hchunk = (int)((Hout + hsplit - 1) / hsplit);
    hsplit = (Hout + a.hchunk - 1) / a.hchunk;
    a.ntiles = (int)ntiles;
    const int pairs = NB * C / 2;
    const int KB = pairs <= 4 * PDT_WAVE ? 1 : pairs <= 8 * PDT_WAVE ? 2 : 4;
    a.step_u = 2 * PDT_WAVE / C;
    a.step_c = 2 * PDT_WAVE % C;
    const int64_t grid = ntiles * hsplit;
    if (grid < (1ll << 31)) {
      const size_t smem = oc_run_lds(R, C, NB);
      const auto kern = KB == 1 ? oc_expand_runs_kernel<1> : KB == 2 ? oc_expand_runs_kernel<2>
                                                                     : oc_expand_runs_kernel<4>;
      if (const int rc = set_lds(kern, smem)) return rc;
      hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(nw * PDT_WAVE), smem, stream, a);
      return (int)hipGetLastError();
    }
  }
  if ((over_n || over_h) && N < (1ll << 31)) {
    OcTileArgs a{};
    a.bitmask = bitmask; a.class_tokens = class_tokens; a.targets = targets;
    a.N = N; a.padding = padding; a.R = R; a.W = W; a.Hout = Hout; a.C = C;
    a.over_n = over_n ? 1 : 0;
    a.outer_stride = over_n ? tgt_sh : tgt_sn;
    while ((1 << a.lgWp) < W) ++a.lgWp;
    // rows per tile: 4 (a run of 4 * C * 8 bytes: 31 whole lines at the bench shape; measured
    // 0.55 ms against 0.61 with 8 rows, whose tables leave room for two workgroups per CU only),
    // fewer while the tables + bitmask words + four images exceed 64 KiB; jobs per workgroup:
    // 64 values of h per table load (over_n) / 16 tiles of one utterance
    const size_t cap = 64 * 1024;
    int NB = kOcTileRows;
    int chunk = over_n ? kOcTileHChunk : 16;
    while (oc_tile_lds(R, W, C, NB, a.over_n, chunk, 4, nullptr, nullptr) > cap && (NB > 1 || chunk > 8)) {
      if (chunk > 16 || NB == 1) chunk >>= 1; else NB >>= 1;
    }
    // waves per workgroup (they share the tables): eight when that puts more waves on a CU than
    // four do (bench shape: 3 x 8 against 4 x 4, 1.05-1.07 -> 0.98-1.00 ms for the whole op,
    // batch-first 1.04 -> 0.95; with the wide images of V = 5000 a workgroup of eight would be
    // alone on its CU)
    int nw = 4;
    {
      const size_t l4 = oc_tile_lds(R, W, C, NB, a.over_n, chunk, 4, nullptr, nullptr);
      const size_t l8 = oc_tile_lds(R, W, C, NB, a.over_n, chunk, 8, nullptr, nullptr);
      const size_t lds_cu = 160 * 1024;
      if (min(lds_cu / l8, (size_t)4) * 8 > min(lds_cu / l4, (size_t)8) * 4) nw = 8;
    }
    a.nw = nw;
    const size_t smem = oc_tile_lds(R, W, C, NB, a.over_n, chunk, nw, nullptr, nullptr);
    if (smem <= 160 * 1024) {
      a.NB = NB;
      a.chunk = chunk;
      const int64_t inner_len = over_n ? N : Hout;
      a.ntiles = (int)((inner_len + NB - 1) / NB);
      const int64_t grid = over_n ? (int64_t)a.ntiles * ((Hout + a.chunk - 1) / a.chunk)
                                  : N * ((a.ntiles + a.chunk - 1) / a.chunk);
      a.wide = ((a.outer_stride & 1) == 0 && (((int64_t)NB * C) & 1) == 0 &&
                (reinterpret_cast<uintptr_t>(targets) & 15) == 0) ? 1 : 0;
      if (grid > 0 && grid < (1ll << 31)) {
        auto kern = nw == 8 ? oc_expand_tiles_kernel<8> : oc_expand_tiles_kernel<4>;
        if (const int rc = set_lds(kern, smem, cap)) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(nw * PDT_WAVE), smem, stream, a);
        return (int)hipGetLastError();
      }
    }
  }
  const size_t smem = (((size_t)R + (size_t)4 * W * 32) * 8 + 15) & ~(size_t)15;
  if (smem > 160 * 1024) return PDT_E_TOO_LONG;
  if (const int rc = set_lds(oc_expand_kernel, smem)) return rc;
  hipLaunchKernelGGL(oc_expand_kernel, dim3((unsigned)N), dim3(256), smem, stream, bitmask,
                     class_tokens, R, W, Hout, N, C, padding, targets, tgt_sh, tgt_sn);
  return (int)hipGetLastError();
}

}  // namespace pdt
