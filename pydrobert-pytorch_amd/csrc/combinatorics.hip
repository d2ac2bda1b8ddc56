// Combinatorics (reference _combinatorics.py:27-412): the enumerations behind exact expectations
// over small discrete supports, binomial coefficients, and Fan's sequential draw of a binary
// vector of fixed cardinality.
//
// enumerate_vocab   out (V^L, L), out[s, t] = (s / V^t) % V: a pure store stream.  A thread owns 16
//                   contiguous bytes of the flat output, finds its row and column with one 32-bit
//                   division from the tile's (uniform) origin, then peels digits off the row index by
//                   repeated division (shifts when V is a power of two) and stores one vector.
// binomial          a gather from the Pascal table (67 x 67 int64, rows 0 .. 66: the largest length
//                   whose every coefficient fits int64); out-of-range inputs set a flag word.
// cardinality       one thread per output row unranks its index in the combinatorial number system
//                   (for i = count .. 1 the largest p with C(p, i) <= k) against the table in LDS and
//                   leaves a bit mask in LDS; the workgroup then writes its rows as one contiguous
//                   run, zeros where the row or the column is beyond its batch element's extent.
// srswor            lane = row; ell (ones still to place) and the row's total stay in registers for the
//                   whole vector.  u and b move through a 64 x 64 LDS tile (rows padded to 65) so
//                   that global accesses run along out_size and LDS accesses are conflict-free.
#include "pdt_common.hpp"

namespace pdt {
namespace {

enum { ENUM_I64 = 0, ENUM_I32 = 1, ENUM_U8 = 2, ENUM_F32 = 3, ENUM_F64 = 4 };

constexpr int kCombThreads = 256;
constexpr int kPascal = 67;       // table rows / columns: lengths 0 .. 66
constexpr int kMaxCardLength = 62;
constexpr int kSrsTile = 64;

template <typename O, int V> struct alignas(sizeof(O) * V) OutVec { O v[V]; };

struct VocabArgs {
  void *out;
  int64_t total;     // V^L * L elements
  uint32_t L, V, lg; // lg = log2 V when V is a power of two
  uint32_t pw[32];   // V^t (t < L <= 32 whenever V >= 2: V^L < 2^32)
};

template <typename O, bool POW2>
__global__ void __launch_bounds__(kCombThreads) enumerate_vocab_kernel(const VocabArgs a) {
  constexpr int VEC = 16 / sizeof(O);
  constexpr int64_t TILE = (int64_t)kCombThreads * VEC;
  O *out = (O *)a.out;
  for (int64_t e0 = (int64_t)blockIdx.x * TILE; e0 < a.total; e0 += (int64_t)gridDim.x * TILE) {
    const int64_t e = e0 + (int64_t)threadIdx.x * VEC;
    if (e >= a.total) continue;
    const uint32_t s0 = (uint32_t)(e0 / a.L), t0 = (uint32_t)(e0 % a.L);  // (uniform)
    const uint32_t off = threadIdx.x * VEC + t0;
    uint32_t s = s0 + off / a.L, t = off % a.L;
    uint32_t q = POW2 ? s >> (t * a.lg) : s / a.pw[t];
    OutVec<O, VEC> vals;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      vals.v[i] = (O)(POW2 ? (q & (a.V - 1u)) : (q % a.V));
      if (++t == a.L) t = 0, q = ++s;
      else q = POW2 ? q >> a.lg : q / a.V;
    }
    if (e + VEC <= a.total) {
      *reinterpret_cast<OutVec<O, VEC> *>(out + e) = vals;
    } else {
      for (int i = 0; i < VEC && e + i < a.total; ++i) out[e + i] = vals.v[i];
    }
  }
}

__global__ void __launch_bounds__(kCombThreads)
binomial_kernel(const int64_t *length, const int64_t *count, const int64_t *table, int64_t *out, int *flags,
                int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kCombThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t l = length[i], c = count[i];
  int bad = (l < 0 || c < 0 ? 1 : 0) | (l >= kPascal ? 2 : 0);
  out[i] = (bad || c > l) ? 0 : table[l * kPascal + c];
  if (bad) atomicOr(flags, bad);
}

struct CardArgs {
  void *out;
  const int64_t *length, *count;  // (B,), or NULL: len0 / cnt0
  const int64_t *table;
  int64_t len0, cnt0, B, NB, W;   // out (B, NB, W)
};

template <typename O>
__global__ void __launch_bounds__(kCombThreads) enumerate_cardinality_kernel(const CardArgs a) {
  __shared__ int64_t tab[kPascal * kPascal];
  __shared__ uint64_t mask[kCombThreads];
  for (int i = threadIdx.x; i < kPascal * kPascal; i += kCombThreads) tab[i] = a.table[i];
  __syncthreads();
  const int64_t tiles = (a.NB + kCombThreads - 1) / kCombThreads;
  const int64_t b = blockIdx.x / tiles, k0 = (blockIdx.x % tiles) * kCombThreads;
  const int64_t len = a.length ? a.length[b] : a.len0, cnt = a.count ? a.count[b] : a.cnt0;
  const bool ok = len >= 0 && len <= kMaxCardLength && cnt >= 0 && cnt <= len;  // (the host refuses the rest)
  const int64_t nrows = ok ? tab[len * kPascal + cnt] : 0;
  const int64_t k = k0 + threadIdx.x;
  uint64_t m = 0;
  if (k < nrows) {
    int64_t rem = k;
    int p = (int)len;
    for (int i = (int)cnt; i >= 1; --i) {
      do --p; while (tab[p * kPascal + i] > rem);  // (ends at p = i - 1 at the latest: C(i - 1, i) = 0)
      m |= 1ull << p;
      rem -= tab[p * kPascal + i];
    }
  }
  mask[threadIdx.x] = m;
  __syncthreads();
  const int64_t rows_here = a.NB - k0 < kCombThreads ? a.NB - k0 : kCombThreads;
  const int total = (int)(rows_here * a.W);
  O *out = (O *)a.out + (b * a.NB + k0) * a.W;
  const int W = (int)a.W;
  for (int e = threadIdx.x; e < total; e += kCombThreads) out[e] = (O)((mask[e / W] >> (e % W)) & 1ull);
}

__global__ void __launch_bounds__(kSrsTile)
srswor_kernel(const int64_t *total, const int64_t *given, const float *u, float *out, int64_t B, int64_t O) {
  __shared__ float tile[kSrsTile][kSrsTile + 1];
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kSrsTile, row = row0 + lane;
  const int rows_here = (int)(B - row0 < kSrsTile ? B - row0 : kSrsTile);
  const int64_t tot = row < B ? total[row] : 0;
  int64_t ell = row < B ? given[row] : 0;
  for (int64_t c0 = 0; c0 < O; c0 += kSrsTile) {
    const int cols = (int)(O - c0 < kSrsTile ? O - c0 : kSrsTile);
    if (lane < cols)
      for (int j = 0; j < rows_here; ++j) tile[j][lane] = u[(row0 + j) * O + c0 + lane];
    __syncthreads();
    if (lane < rows_here) {
      for (int c = 0; c < cols; ++c) {
        int64_t rem = tot - (c0 + c);
        rem = rem < 1 ? 1 : rem;
        const bool b = tile[lane][c] < (float)ell / (float)rem;
        ell -= b ? 1 : 0;
        tile[lane][c] = b ? 1.0f : 0.0f;
      }
    }
    __syncthreads();
    if (lane < cols)
      for (int j = 0; j < rows_here; ++j) out[(row0 + j) * O + c0 + lane] = tile[j][lane];
    __syncthreads();
  }
}

template <typename O> int launch_vocab(const VocabArgs &a, bool pow2, hipStream_t s) {
  constexpr int64_t TILE = (int64_t)kCombThreads * (16 / sizeof(O));
  int64_t blocks = (a.total + TILE - 1) / TILE;
  if (blocks > 65536) blocks = 65536;
  if (pow2) hipLaunchKernelGGL((enumerate_vocab_kernel<O, true>), dim3((unsigned)blocks), dim3(kCombThreads), 0, s, a);
  else hipLaunchKernelGGL((enumerate_vocab_kernel<O, false>), dim3((unsigned)blocks), dim3(kCombThreads), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace pdt

extern "C" int pdt_enumerate_vocab_sequences(int64_t length, int64_t vocab_size, int out_type, void *out,
                                             void *stream) {
  using namespace pdt;
  if (length < 0 || vocab_size <= 0 || out_type < ENUM_I64 || out_type > ENUM_F64) return PDT_E_ARG;
  if (length >= (1ll << 30)) return PDT_E_TOO_LONG;
  // rows = vocab_size^length must stay below 2^32: the kernel's row arithmetic is 32-bit
  VocabArgs a;
  uint64_t rows = 1;
  for (int64_t t = 0; t < length && vocab_size > 1; ++t) {
    if (t < 32) a.pw[t] = (uint32_t)rows;
    rows *= (uint64_t)vocab_size;
    if (rows >= (1ull << 32)) return PDT_E_TOO_LONG;
  }
  if (length == 0) return PDT_OK;  // (1, 0): nothing to write
  if (out == nullptr || ((uintptr_t)out & 15u)) return PDT_E_ARG;
  a.out = out;
  a.total = (int64_t)rows * length;
  a.L = (uint32_t)length, a.V = (uint32_t)vocab_size, a.lg = 0;
  const bool pow2 = (vocab_size & (vocab_size - 1)) == 0;
  while (pow2 && (1ll << a.lg) < vocab_size) ++a.lg;
  hipStream_t s = (hipStream_t)stream;
  switch (out_type) {
    case ENUM_I64: return launch_vocab<int64_t>(a, pow2, s);
    case ENUM_I32: return launch_vocab<int32_t>(a, pow2, s);
    case ENUM_U8: return launch_vocab<uint8_t>(a, pow2, s);
    case ENUM_F32: return launch_vocab<float>(a, pow2, s);
    default: return launch_vocab<double>(a, pow2, s);
  }
}

extern "C" int pdt_binomial_coefficient(const int64_t *length, const int64_t *count, int64_t n,
                                        const int64_t *table, int64_t *out, int32_t *flags, void *stream) {
  using namespace pdt;
  if (n < 0) return PDT_E_ARG;
  if (n == 0) return PDT_OK;
  if (!length || !count || !table || !out || !flags) return PDT_E_ARG;
  const int64_t blocks = (n + kCombThreads - 1) / kCombThreads;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  hipLaunchKernelGGL(binomial_kernel, dim3((unsigned)blocks), dim3(kCombThreads), 0, (hipStream_t)stream, length,
                     count, table, out, flags, n);
  return (int)hipGetLastError();
}

extern "C" int pdt_enumerate_cardinality(const int64_t *length, const int64_t *count, int64_t length0,
                                         int64_t count0, int64_t B, int64_t rows, int64_t width,
                                         const int64_t *table, int out_type, void *out, void *stream) {
  using namespace pdt;
  if (B < 0 || rows < 0 || width < 0 || out_type < ENUM_I64 || out_type > ENUM_F64) return PDT_E_ARG;
  if ((length == nullptr) != (count == nullptr)) return PDT_E_ARG;
  if (width > kMaxCardLength) return PDT_E_TOO_LONG;
  if (length == nullptr && (B != 1 || length0 < 0 || length0 > width || count0 < 0)) return PDT_E_ARG;
  if (B == 0 || rows == 0 || width == 0) return PDT_OK;
  if (!table || !out) return PDT_E_ARG;
  const int64_t tiles = (rows + kCombThreads - 1) / kCombThreads;
  if (tiles > 0x7fffffffLL / B) return PDT_E_TOO_LONG;
  CardArgs a;
  a.out = out, a.length = length, a.count = count, a.table = table;
  a.len0 = length0, a.cnt0 = count0, a.B = B, a.NB = rows, a.W = width;
  const dim3 grid((unsigned)(B * tiles)), blk(kCombThreads);
  hipStream_t s = (hipStream_t)stream;
  switch (out_type) {
    case ENUM_I64: hipLaunchKernelGGL(enumerate_cardinality_kernel<int64_t>, grid, blk, 0, s, a); break;
    case ENUM_I32: hipLaunchKernelGGL(enumerate_cardinality_kernel<int32_t>, grid, blk, 0, s, a); break;
    case ENUM_U8: hipLaunchKernelGGL(enumerate_cardinality_kernel<uint8_t>, grid, blk, 0, s, a); break;
    case ENUM_F32: hipLaunchKernelGGL(enumerate_cardinality_kernel<float>, grid, blk, 0, s, a); break;
    default: hipLaunchKernelGGL(enumerate_cardinality_kernel<double>, grid, blk, 0, s, a); break;
  }
  return (int)hipGetLastError();
}

extern "C" int pdt_srswor(const int64_t *total_count, const int64_t *given_count, const float *u, int64_t B,
                          int64_t out_size, float *out, void *stream) {
  using namespace pdt;
  if (B < 0 || out_size < 0) return PDT_E_ARG;
  if (B == 0 || out_size == 0) return PDT_OK;
  if (!total_count || !given_count || !u || !out) return PDT_E_ARG;
  const int64_t blocks = (B + kSrsTile - 1) / kSrsTile;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  hipLaunchKernelGGL(srswor_kernel, dim3((unsigned)blocks), dim3(kSrsTile), 0, (hipStream_t)stream, total_count,
                     given_count, u, out, B, out_size);
  return (int)hipGetLastError();
}
