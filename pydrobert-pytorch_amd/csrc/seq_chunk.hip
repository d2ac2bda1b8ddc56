// Slicing and chunking (reference _pad.py:257-548, _feats.py:417-930): pad_masked_sequence,
// chunk_by_slices, chunk_token_sequences_by_slices and slice_spect_data on two primitives.
//
// 1. Stable compaction within a row (compact_rows_kernel): one workgroup per row walks the row
//    256 steps at a time; a step's rank among the kept ones is the popcount of the wave ballot
//    below its lane, plus the counts of the waves before it (LDS), plus the carry of the passes
//    before.  The keep test and what a kept step writes are a policy (template parameter): the
//    bool mask of pad_masked_sequence, the triple test of the token chunks, the three policies of
//    slice_spect_data.  A policy addresses its output by a per-row base, so rows pack inside
//    themselves (base n * stride, tail filled) or into one flat list (base = exclusive scan of the
//    row counts, taken from a first run that only counts).  Every output element has one writer.
// 2. Copy with an index map and a padding rule (steps_copy_kernel): pad_variable_kernel with a
//    source-step functor -- the map a compaction wrote (pad_masked_sequence and its adjoint) or
//    start + t under constant / reflect / replicate (chunk_by_slices).  Elements move as opaque
//    1/2/4/8-byte words, or 16-byte groups of them when the caller finds rows, strides and
//    pointers to be multiples of 16 bytes; one read of what is kept, one write of the output, both along F (and
//    along N for time-major layouts).
//
// The adjoint of chunk_by_slices (float32 / float64) is a gather like pad_variable's.
#include "pdt_common.hpp"

namespace pdt {

enum { CHUNK_CONSTANT = 0, CHUNK_REFLECT = 1, CHUNK_REPLICATE = 2 };

// ------------------------------------------------------------------------------------------------
// row compaction

template <typename P>
__global__ void __launch_bounds__(256)
compact_rows_kernel(const P p, int T, int fill_to, int emit, int64_t *__restrict__ counts) {
  __shared__ int wave_total[4];
  const int n = (int)blockIdx.x, lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  int carry = 0;
  for (int t0 = 0; t0 < T; t0 += 256) {  // (uniform trip count: the barriers are safe)
    const int t = t0 + (int)threadIdx.x;
    const bool keep = t < T && p.keep(n, t);
    const unsigned long long kept = __ballot(keep);
    const int below = __popcll(kept & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(kept);
    __syncthreads();
    int before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wave_total[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (emit && t < T) p.emit(n, t, keep, before + below);
    carry += total;
    __syncthreads();
  }
  if (emit)
    for (int j = carry + (int)threadIdx.x; j < fill_to; j += 256) p.fill(n, j);
  if (threadIdx.x == 0 && counts) counts[n] = carry;
}

// pad_masked_sequence: src[n, j] = the step the j-th kept one came from (-1 past the count),
// rank[n, t] = where step t went (-1 if dropped); either may be null.  mask and the maps are
// read / written through element strides, so both batch_first layouts are served in place.
struct MaskPolicy {
  const uint8_t *mask;
  int64_t m_sn, m_st;
  int32_t *src, *rank;
  int64_t o_sn, o_st;
  __device__ bool keep(int n, int t) const { return mask[n * m_sn + t * m_st] != 0; }
  __device__ void emit(int n, int t, bool keep, int r) const {
    if (keep && src) src[n * o_sn + r * o_st] = t;
    if (rank) rank[n * o_sn + t * o_st] = keep ? r : -1;
  }
  __device__ void fill(int n, int j) const {
    if (src) src[n * o_sn + j * o_st] = -1;
  }
};

// chunk_token_sequences_by_slices (_feats.py:811-836): refs (N, R, 3), slices (N, 2) int64
struct TokenPolicy {
  const int64_t *refs, *slices, *ref_lens;
  int64_t *out;
  int R, partial, retain;
  __device__ bool keep(int n, int r) const {
    if (ref_lens && r >= ref_lens[n]) return false;
    const int64_t *tr = refs + ((int64_t)n * R + r) * 3;
    const int64_t rs = tr[1], re = tr[2], ss = slices[2 * n], se = slices[2 * n + 1];
    if (rs < 0 || re < 0 || re < rs) return false;
    return partial ? (ss < re && se > rs) : (ss <= rs && se >= re);
  }
  __device__ void emit(int n, int r, bool keep, int j) const {
    if (!keep) return;
    const int64_t *tr = refs + ((int64_t)n * R + r) * 3;
    const int64_t off = retain ? 0 : slices[2 * n];  // (:836 ADDS the slice start)
    int64_t *o = out + ((int64_t)n * R + j) * 3;
    o[0] = tr[0];
    o[1] = tr[1] + off;
    o[2] = tr[2] + off;
  }
  __device__ void fill(int n, int j) const {
    int64_t *o = out + ((int64_t)n * R + j) * 3;
    o[0] = o[1] = o[2] = 0;
  }
};

// where the kept candidates of a slice_spect_data row go: base[n] + rank, or n * stride + rank
struct SliceOut {
  int64_t *slices, *sources;
  const int64_t *base;
  int64_t stride;
  __device__ void put(int n, int r, int64_t start, int64_t end) const {
    const int64_t i = (base ? base[n] : (int64_t)n * stride) + r;
    slices[2 * i] = start;
    slices[2 * i + 1] = end;
    sources[i] = n;
  }
};

// policy 'fixed' (_feats.py:459-501): candidate k is [a0 + k shift, a0 + k shift + width), kept
// when in_lens[n] > m0 + k shift
struct FixedPolicy {
  const int64_t *in_lens;
  int64_t a0, shift, width, m0;
  SliceOut o;
  __device__ bool keep(int n, int k) const { return !in_lens || in_lens[n] > m0 + k * shift; }
  __device__ void emit(int n, int k, bool keep, int r) const {
    if (keep) o.put(n, r, a0 + k * shift, a0 + k * shift + width);
  }
  __device__ void fill(int, int) const {}
};

// policy 'ref' (:544-583): input (N, T, 3); other_lens null = the end of the row's last segment
struct RefPolicy {
  const int64_t *input, *in_lens, *other_lens;
  int T;
  int64_t left, right;
  int valid_only;
  SliceOut o;
  __device__ bool window(int n, int t, int64_t &s, int64_t &e) const {
    int64_t len = in_lens ? in_lens[n] : T;
    if (len > T) len = T;
    if (t >= len) return false;
    const int64_t *tr = input + ((int64_t)n * T + t) * 3;
    s = tr[1];
    e = tr[2];
    if (s < 0 || e < 0) return false;
    const int64_t other = other_lens ? other_lens[n] : input[((int64_t)n * T + len - 1) * 3 + 2];
    s -= left;
    e += right;
    if (valid_only ? !(s >= 0 && e <= other) : !(e > 0 && s < other)) return false;
    return s < e;
  }
  __device__ bool keep(int n, int t) const {
    int64_t s, e;
    return window(n, t, s, e);
  }
  __device__ void emit(int n, int t, bool keep, int r) const {
    int64_t s, e;
    if (keep && window(n, t, s, e)) o.put(n, r, s, e);
  }
  __device__ void fill(int, int) const {}
};

// policy 'ali' (:502-543), first half: seg[n, k] = the first step of the row's k-th run of equal
// labels within in_lens[n]
struct AliPolicy {
  const int64_t *input, *in_lens;
  int32_t *seg;
  int T;
  __device__ bool keep(int n, int t) const {
    if (in_lens && t >= in_lens[n]) return false;
    const int64_t *row = input + (int64_t)n * T;
    return t == 0 || row[t] != row[t - 1];
  }
  __device__ void emit(int n, int t, bool keep, int r) const {
    if (keep) seg[(int64_t)n * T + r] = t;
  }
  __device__ void fill(int, int) const {}
};

// 'ali', second half: slice k of row n from its segment starts (closed form of the lobe loop)
__global__ void __launch_bounds__(256)
ali_emit_kernel(const int32_t *__restrict__ seg, const int64_t *__restrict__ in_lens,
                const int64_t *__restrict__ nseg, const int64_t *__restrict__ cnt, int T, int64_t left,
                int64_t right, int valid_only, SliceOut o, unsigned total) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  if (gid >= total) return;
  const int n = (int)(gid / (unsigned)T), k = (int)(gid - (unsigned)n * (unsigned)T);
  if (k >= cnt[n]) return;
  const int64_t K = nseg[n];
  int64_t len = in_lens ? in_lens[n] : T;
  if (len > T) len = T;
  const int32_t *row = seg + (int64_t)n * T;
  int64_t first, last;  // the segments the slice starts and ends with
  if (valid_only) {
    first = k;
    last = k + left + right;
  } else {
    first = k - left < 0 ? 0 : k - left;
    last = k + right > K - 1 ? K - 1 : k + right;
  }
  if (first < 0 || last >= K) return;  // (cnt never admits it)
  o.put(n, k, row[first], last + 1 < K ? (int64_t)row[last + 1] : len);
}

// ------------------------------------------------------------------------------------------------
// copy with an index map and a padding rule

struct CopyArgs {
  const void *x;   // step s of row n at x + (n * x_sn + s * x_st + f) elements, f < F
  void *out;       // (N, To, F), or (To, N, F) when time_major; contiguous
  const void *fill;
  int64_t x_sn, x_st;
  int N, T, F, To, time_major;
  const int32_t *map;  // MapSrc: source step of output step t of row n, < 0 for the fill
  int64_t m_sn, m_st;
  const int64_t *slices, *lens;  // SliceSrc: (N, 2) start / end, (N,) or null
  int mode;
};

struct MapSrc {
  static __device__ __forceinline__ int64_t step(const CopyArgs &a, int n, int t) {
    return a.map[n * a.m_sn + t * a.m_st];
  }
};

// chunk_by_slices: output step t of row n reads s = start + t
struct SliceSrc {
  static __device__ __forceinline__ int64_t step(const CopyArgs &a, int n, int t) {
    const int64_t start = a.slices[2 * n], end = a.slices[2 * n + 1];
    int64_t len = a.lens ? a.lens[n] : a.T;
    if (len > a.T) len = a.T;  // (as the adjoint does: a length beyond T counts as T)
    if (t >= end - start) return -1;  // at or beyond chunk_len: the fill, in every mode
    int64_t s = start + t;
    if (s < 0) s = a.mode == CHUNK_REFLECT ? -s : a.mode == CHUNK_REPLICATE ? 0 : -1;
    else if (s >= len) s = a.mode == CHUNK_REFLECT ? 2 * (len - 1) - s : a.mode == CHUNK_REPLICATE ? len - 1 : -1;
    return s < len ? s : -1;  // (a reflection or replication the caller's checks exclude)
  }
};

constexpr int kPerThread = 4;

// As pad_variable_kernel: one thread per output element, flat over the output, so consecutive
// lanes move consecutive words whatever F is.
template <typename W, typename Src>
__global__ void __launch_bounds__(256) steps_copy_kernel(const CopyArgs a, unsigned total) {
  const W fill = *reinterpret_cast<const W *>(a.fill);
  const unsigned F = (unsigned)a.F, To = (unsigned)a.To, N = (unsigned)a.N;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gid = (blockIdx.x * kPerThread + i) * 256u + threadIdx.x;
    if (gid >= total) return;
    const unsigned row = gid / F, f = gid - row * F;
    unsigned n, t;
    if (a.time_major) {
      t = row / N;
      n = row - t * N;
    } else {
      n = row / To;
      t = row - n * To;
    }
    const int64_t s = Src::step(a, (int)n, (int)t);
    W v = fill;
    if (s >= 0 && s < a.T) v = reinterpret_cast<const W *>(a.x)[n * a.x_sn + s * a.x_st + f];
    reinterpret_cast<W *>(a.out)[gid] = v;
  }
}

template <typename Src>
static int launch_copy(const CopyArgs &a, int64_t elem_bytes, hipStream_t s) {
  const unsigned total = (unsigned)((int64_t)a.N * a.To * a.F);
  const dim3 grid((total + 256 * kPerThread - 1) / (256 * kPerThread));
  switch (elem_bytes) {
    case 1: hipLaunchKernelGGL((steps_copy_kernel<uint8_t, Src>), grid, dim3(256), 0, s, a, total); break;
    case 2: hipLaunchKernelGGL((steps_copy_kernel<uint16_t, Src>), grid, dim3(256), 0, s, a, total); break;
    case 4: hipLaunchKernelGGL((steps_copy_kernel<uint32_t, Src>), grid, dim3(256), 0, s, a, total); break;
    case 8: hipLaunchKernelGGL((steps_copy_kernel<uint64_t, Src>), grid, dim3(256), 0, s, a, total); break;
    case 16: hipLaunchKernelGGL((steps_copy_kernel<uint4, Src>), grid, dim3(256), 0, s, a, total); break;
    default: return PDT_E_ARG;
  }
  return (int)hipGetLastError();
}

// grad_x[n, s, :] = sum of grad_out[n, t, :] over the chunk steps t that read x[n, s, :]
template <typename R>
__global__ void __launch_bounds__(256)
chunk_backward_kernel(const R *__restrict__ grad_out, const int64_t *__restrict__ slices,
                      const int64_t *__restrict__ lens, int T, int F, int Tp, int mode,
                      R *__restrict__ grad_x, unsigned total) {
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const unsigned gid = (blockIdx.x * kPerThread + i) * 256u + threadIdx.x;
    if (gid >= total) return;
    const unsigned row = gid / (unsigned)F, f = gid - row * (unsigned)F;
    const unsigned n = row / (unsigned)T;
    const int64_t s = row - n * (unsigned)T;
    const int64_t start = slices[2 * n], end = slices[2 * n + 1];
    int64_t len = lens ? lens[n] : T, chunk = end - start;
    if (len > T) len = T;
    if (chunk > Tp) chunk = Tp;
    const R *go = grad_out + (int64_t)n * Tp * F + f;
    R acc = 0;
    if (s < len && chunk > 0) {
      int64_t t = s - start;  // its own copy
      if (t >= 0 && t < chunk) acc = go[t * F];
      if (mode == CHUNK_REFLECT) {
        t = -s - start;  // read as the reflection of step -s
        if (s >= 1 && t >= 0 && t < chunk) acc += go[t * F];
        t = 2 * (len - 1) - s - start;  // ... and of step 2 (len - 1) - s >= len
        if (s <= len - 2 && t >= 0 && t < chunk) acc += go[t * F];
      } else if (mode == CHUNK_REPLICATE) {
        if (s == 0)
          for (int64_t u = 0; u < chunk && start + u < 0; ++u) acc += go[u * F];
        if (s == len - 1)
          for (int64_t u = len - start > 0 ? len - start : 0; u < chunk; ++u) acc += go[u * F];
      }
    }
    grad_x[gid] = acc;
  }
}

// T' and the data checks of chunk_by_slices in one launch (the reference's _pad.py:406-416, :57, :84):
// per row the left pad, the chunk length and the right pad (pads zero for an empty slice);
// stats[0] = the largest of all of them (T'), stats[1] = max (pad - len) over both pads (>= 0: a pad
// reaches the length), stats[2] = min len.  One workgroup, a fixed-order LDS tree: N numbers.
__global__ void __launch_bounds__(256)
chunk_stats_kernel(const int64_t *__restrict__ slices, const int64_t *__restrict__ lens, int N, int64_t T,
                   int64_t *__restrict__ chunk_lens, int64_t *__restrict__ stats) {
  __shared__ int64_t red[3][256];
  int64_t longest = 0, over = INT64_MIN, shortest = INT64_MAX;
  for (int n = (int)threadIdx.x; n < N; n += 256) {
    const int64_t start = slices[2 * n], end = slices[2 * n + 1], len = lens ? lens[n] : T;
    const int64_t chunk = end - start > 0 ? end - start : 0;
    const int64_t left = chunk && start < 0 ? -start : 0, right = chunk && end > len ? end - len : 0;
    chunk_lens[n] = chunk;
    const int64_t pad = left > right ? left : right;
    longest = longest > chunk ? longest : chunk;
    longest = longest > pad ? longest : pad;
    over = over > pad - len ? over : pad - len;
    shortest = shortest < len ? shortest : len;
  }
  red[0][threadIdx.x] = longest;
  red[1][threadIdx.x] = over;
  red[2][threadIdx.x] = shortest;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const int o = (int)threadIdx.x + w;
      if (red[0][o] > red[0][threadIdx.x]) red[0][threadIdx.x] = red[0][o];
      if (red[1][o] > red[1][threadIdx.x]) red[1][threadIdx.x] = red[1][o];
      if (red[2][o] < red[2][threadIdx.x]) red[2][threadIdx.x] = red[2][o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) stats[threadIdx.x] = red[threadIdx.x][0];
}

static bool fits32(int64_t elems) { return elems < (1ll << 32) - 1024 * kPerThread; }
// sizes the argument blocks keep as int
static bool fits_int(int64_t a, int64_t b, int64_t c, int64_t d) { return (a | b | c | d) <= 0x7fffffffll; }

}  // namespace pdt

extern "C" {

int pdt_compact_mask(const void *mask, int64_t N, int64_t T, int64_t m_sn, int64_t m_st, int32_t *src,
                     int32_t *rank, int64_t o_sn, int64_t o_st, int64_t *counts, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!counts || (T > 0 && (!mask || (!src && !rank)))) return PDT_E_ARG;
  if (N >= (1ll << 31) || T >= (1ll << 31) - 256) return PDT_E_TOO_LONG;
  const MaskPolicy p{(const uint8_t *)mask, m_sn, m_st, src, rank, o_sn, o_st};
  hipLaunchKernelGGL(compact_rows_kernel<MaskPolicy>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p,
                     (int)T, (int)T, 1, counts);
  return (int)hipGetLastError();
}

int pdt_gather_steps(const void *x, int64_t N, int64_t T, int64_t F, int64_t elem_bytes, int64_t x_sn,
                     int64_t x_st, const int32_t *map, int64_t m_sn, int64_t m_st, int64_t To,
                     int time_major, const void *fill, void *out, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0 || F < 0 || To < 0) return PDT_E_ARG;
  if (N == 0 || To == 0 || F == 0) return PDT_OK;
  if (!map || !fill || !out || (T > 0 && !x)) return PDT_E_ARG;
  if (!fits_int(N, T, F, To)) return PDT_E_TOO_LONG;
  if (!fits32(N * To * F)) return PDT_E_TOO_LONG;
  CopyArgs a{};
  a.x = x; a.out = out; a.fill = fill; a.x_sn = x_sn; a.x_st = x_st;
  a.N = (int)N; a.T = (int)T; a.F = (int)F; a.To = (int)To; a.time_major = time_major;
  a.map = map; a.m_sn = m_sn; a.m_st = m_st;
  return launch_copy<MapSrc>(a, elem_bytes, (hipStream_t)stream);
}

int pdt_chunk_by_slices(const void *x, int64_t N, int64_t T, int64_t F, int64_t elem_bytes, int64_t x_sn,
                        int64_t x_st, const int64_t *slices, const int64_t *lens, int mode,
                        const void *fill, int64_t Tp, void *out, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0 || F < 0 || Tp < 0 || mode < 0 || mode > 2) return PDT_E_ARG;
  if (N == 0 || Tp == 0 || F == 0) return PDT_OK;
  if (!slices || !fill || !out || (T > 0 && !x)) return PDT_E_ARG;
  if (!fits_int(N, T, F, Tp)) return PDT_E_TOO_LONG;
  if (!fits32(N * Tp * F)) return PDT_E_TOO_LONG;
  CopyArgs a{};
  a.x = x; a.out = out; a.fill = fill; a.x_sn = x_sn; a.x_st = x_st;
  a.N = (int)N; a.T = (int)T; a.F = (int)F; a.To = (int)Tp; a.time_major = 0;
  a.slices = slices; a.lens = lens; a.mode = mode;
  return launch_copy<SliceSrc>(a, elem_bytes, (hipStream_t)stream);
}

int pdt_chunk_stats(const int64_t *slices, const int64_t *lens, int64_t N, int64_t T, int64_t *chunk_lens,
                    int64_t *stats, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!slices || !chunk_lens || !stats) return PDT_E_ARG;
  if (N >= (1ll << 31)) return PDT_E_TOO_LONG;
  hipLaunchKernelGGL(chunk_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, slices, lens, (int)N, T,
                     chunk_lens, stats);
  return (int)hipGetLastError();
}

int pdt_chunk_by_slices_backward(const void *grad_out, int dtype, int64_t N, int64_t T, int64_t F,
                                 const int64_t *slices, const int64_t *lens, int mode, int64_t Tp,
                                 void *grad_x, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0 || F < 0 || Tp < 0 || mode < 0 || mode > 2 || dtype < 0 || dtype > 1) return PDT_E_ARG;
  if (N == 0 || T == 0 || F == 0) return PDT_OK;
  if (!slices || !grad_x || (Tp > 0 && !grad_out)) return PDT_E_ARG;
  if (!fits_int(N, T, F, Tp)) return PDT_E_TOO_LONG;
  if (!fits32(N * T * F) || !fits32(N * Tp * F)) return PDT_E_TOO_LONG;
  const unsigned total = (unsigned)(N * T * F);
  const dim3 grid((total + 256 * kPerThread - 1) / (256 * kPerThread));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(chunk_backward_kernel<float>, grid, dim3(256), 0, s, (const float *)grad_out, slices, lens,
                       (int)T, (int)F, (int)Tp, mode, (float *)grad_x, total);
  else
    hipLaunchKernelGGL(chunk_backward_kernel<double>, grid, dim3(256), 0, s, (const double *)grad_out, slices,
                       lens, (int)T, (int)F, (int)Tp, mode, (double *)grad_x, total);
  return (int)hipGetLastError();
}

int pdt_chunk_tokens(const int64_t *refs, int64_t N, int64_t R, const int64_t *slices, const int64_t *ref_lens,
                     int partial, int retain, int64_t *out, int64_t *counts, void *stream) {
  using namespace pdt;
  if (N < 0 || R < 0) return PDT_E_ARG;
  if (N == 0) return PDT_OK;
  if (!slices || !counts || (R > 0 && (!refs || !out))) return PDT_E_ARG;
  if (N >= (1ll << 31) || R >= (1ll << 31) - 256) return PDT_E_TOO_LONG;
  const TokenPolicy p{refs, slices, ref_lens, out, (int)R, partial, retain};
  hipLaunchKernelGGL(compact_rows_kernel<TokenPolicy>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p,
                     (int)R, (int)R, 1, counts);
  return (int)hipGetLastError();
}

int pdt_slice_fixed(int64_t N, int64_t TT, const int64_t *in_lens, int64_t a0, int64_t shift, int64_t width,
                    int64_t m0, const int64_t *base, int emit, int64_t *slices, int64_t *sources,
                    int64_t *counts, void *stream) {
  using namespace pdt;
  if (N < 0 || TT < 0 || shift < 1) return PDT_E_ARG;
  if (N == 0 || TT == 0) return PDT_OK;
  if (emit ? (!slices || !sources) : !counts) return PDT_E_ARG;
  if (N >= (1ll << 31) || TT >= (1ll << 31) - 256) return PDT_E_TOO_LONG;
  const FixedPolicy p{in_lens, a0, shift, width, m0, SliceOut{slices, sources, base, TT}};
  hipLaunchKernelGGL(compact_rows_kernel<FixedPolicy>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p,
                     (int)TT, 0, emit, counts);
  return (int)hipGetLastError();
}

int pdt_slice_ref(const int64_t *input, int64_t N, int64_t T, const int64_t *in_lens, const int64_t *other_lens,
                  int64_t left, int64_t right, int valid_only, const int64_t *base, int emit, int64_t *slices,
                  int64_t *sources, int64_t *counts, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0 || left < 0 || right < 0) return PDT_E_ARG;
  if (N == 0 || T == 0) return PDT_OK;
  if (!input || (emit ? (!slices || !sources || !base) : !counts)) return PDT_E_ARG;
  if (N >= (1ll << 31) || T >= (1ll << 31) - 256) return PDT_E_TOO_LONG;
  const RefPolicy p{input, in_lens, other_lens, (int)T, left, right, valid_only, SliceOut{slices, sources, base, T}};
  hipLaunchKernelGGL(compact_rows_kernel<RefPolicy>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p,
                     (int)T, 0, emit, counts);
  return (int)hipGetLastError();
}

int pdt_slice_ali_segments(const int64_t *input, int64_t N, int64_t T, const int64_t *in_lens, int32_t *seg,
                           int64_t *counts, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0) return PDT_E_ARG;
  if (N == 0 || T == 0) return PDT_OK;
  if (!input || !seg || !counts) return PDT_E_ARG;
  if (N >= (1ll << 31) || T >= (1ll << 31) - 256) return PDT_E_TOO_LONG;
  const AliPolicy p{input, in_lens, seg, (int)T};
  hipLaunchKernelGGL(compact_rows_kernel<AliPolicy>, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p,
                     (int)T, 0, 1, counts);
  return (int)hipGetLastError();
}

int pdt_slice_ali_emit(const int32_t *seg, int64_t N, int64_t T, const int64_t *in_lens, const int64_t *nseg,
                       const int64_t *cnt, const int64_t *base, int64_t left, int64_t right, int valid_only,
                       int64_t *slices, int64_t *sources, void *stream) {
  using namespace pdt;
  if (N < 0 || T < 0 || left < 0 || right < 0) return PDT_E_ARG;
  if (N == 0 || T == 0) return PDT_OK;
  if (!seg || !nseg || !cnt || !base || !slices || !sources) return PDT_E_ARG;
  if (!fits_int(N, T, 0, 0) || !fits32(N * T)) return PDT_E_TOO_LONG;
  const unsigned total = (unsigned)(N * T);
  hipLaunchKernelGGL(ali_emit_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, seg, in_lens,
                     nseg, cnt, (int)T, left, right, valid_only, SliceOut{slices, sources, base, T}, total);
  return (int)hipGetLastError();
}

}  // extern "C"
