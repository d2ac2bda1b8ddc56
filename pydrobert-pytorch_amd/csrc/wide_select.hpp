// The workgroup-wide selection of the plain beam-search forms (advance_wide.hip: the step functions for
// beams wider than a wave; ctc_search_wide.hip: the whole CTC search for such beams).  One workgroup of
// eight waves per batch element.  The top K of the candidates come from a radix select on the
// order-preserving float keys -- three histogram passes (11 + 11 + 10 bits) find the K-th largest key,
// one more pass collects everything above it, and candidates EQUAL to it are taken lowest flat index
// first (each wave owns a contiguous range of the flat index, so "first" is well defined) -- then the K
// winners are ranked by counting.  The candidates are never materialised: every pass re-evaluates them.
#pragma once
#include "wave_select.hpp"

namespace pdt {

constexpr int kWideWaves = 8;
constexpr int kWideThreads = kWideWaves * PDT_WAVE;

struct WideSel {
  u64 *list, *sorted;  // [K] the winners: as collected, then best first
  unsigned *hist;      // [2048]
  unsigned *part;      // [256]
  int *ctl;            // [16]: 0 collected count, 1 digit, 2 count above it, 3 count in it, 8.. per-wave ties
  static size_t bytes(int K) { return (size_t)K * 16 + 2048 * 4 + 256 * 4 + 16 * 4; }
  __device__ unsigned char *carve(unsigned char *p, int K) {
    list = reinterpret_cast<u64 *>(p);
    sorted = list + K;
    hist = reinterpret_cast<unsigned *>(sorted + K);
    part = hist + 2048;
    ctl = reinterpret_cast<int *>(part + 256);
    return reinterpret_cast<unsigned char *>(ctl + 16);
  }
};

__device__ __forceinline__ int lanes_below(u64 bal) {  // set bits of bal below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

// scan(f): every wave calls f(key, flat index, active) on its own contiguous range of the flat
// candidate index, ascending, all 64 lanes together (inactive lanes pad the last chunk of a row).
// The candidates hold at least K entries.  Result: s.sorted[0..K) = (key, index) best first.
template <typename SCAN>
__device__ __forceinline__ void block_top_k(const int K, SCAN &&scan, const WideSel &s) {
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  unsigned prefix = 0u;
  int need = K, cnt_eq = 0;
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const int hi = pass == 1 ? 21 : 10;  // (pass 0 looks at every key)
    const unsigned mask = pass == 2 ? 1023u : 2047u;
    for (int i = tid; i < 2048; i += kWideThreads) s.hist[i] = 0u;
    __syncthreads();
    scan([&](const unsigned key, const unsigned, const bool active) {
      if (active && (pass == 0 || (key >> hi) == (prefix >> hi))) atomicAdd(&s.hist[(key >> shift) & mask], 1u);
    });
    __syncthreads();
    if (tid < 256) {
      unsigned sum = 0u;
      for (int b = 0; b < 8; ++b) sum += s.hist[tid * 8 + b];
      s.part[tid] = sum;
    }
    __syncthreads();
    if (tid < 256) {  // the one thread whose eight bins hold the need-th largest key says which
      unsigned above = 0u;
      for (int u = 255; u > tid; --u) above += s.part[u];
      if (above < (unsigned)need && (unsigned)need <= above + s.part[tid]) {
        unsigned acc = above;
        for (int b = tid * 8 + 7; b >= tid * 8; --b) {
          const unsigned h = s.hist[b];
          if (acc + h >= (unsigned)need) {
            s.ctl[1] = b;
            s.ctl[2] = (int)acc;
            s.ctl[3] = (int)h;
            break;
          }
          acc += h;
        }
      }
    }
    __syncthreads();
    prefix |= (unsigned)s.ctl[1] << shift;
    need -= s.ctl[2];
    cnt_eq = s.ctl[3];
    __syncthreads();
  }
  // prefix: the K-th largest key; need (>= 1) of the cnt_eq candidates that equal it are wanted
  const unsigned T = prefix;
  const bool all_eq = cnt_eq == need;
  if (tid == 0) s.ctl[0] = 0;
  __syncthreads();
  int eq_seen = 0;
  scan([&](const unsigned key, const unsigned idx, const bool active) {
    const bool take = active && (key > T || (all_eq && key == T));
    const u64 bal = __ballot(take);
    if (bal) {
      int base = 0;
      if (lane_id() == (int)__builtin_ctzll(bal)) base = atomicAdd(&s.ctl[0], (int)__popcll(bal));
      base = __builtin_amdgcn_readlane(base, (int)__builtin_ctzll(bal));
      if (take) s.list[base + lanes_below(bal)] = pack_key(key, idx);
    }
    if (!all_eq) eq_seen += (int)__popcll(__ballot(active && key == T));
  });
  if (lane_id() == 0) s.ctl[8 + wave] = eq_seen;
  __syncthreads();
  if (!all_eq) {  // ties at the threshold: the lowest flat indexes
    int rank = 0;
    for (int u = 0; u < wave; ++u) rank += s.ctl[8 + u];
    const int first = K - need;
    if (rank < need)
      scan([&](const unsigned key, const unsigned idx, const bool active) {
        const bool eq = active && key == T;
        const u64 bal = __ballot(eq);
        const int r = rank + lanes_below(bal);
        if (eq && r < need) s.list[first + r] = pack_key(key, idx);
        rank += (int)__popcll(bal);
      });
    __syncthreads();
  }
  for (int i = tid; i < K; i += kWideThreads) {
    const u64 e = s.list[i];
    int r = 0;
    for (int j = 0; j < K; ++j) r += s.list[j] > e ? 1 : 0;
    s.sorted[r] = e;
  }
  __syncthreads();
}

// rows [k0, k1) of the K' prefixes for this wave: contiguous, so that the flat index ascends
__device__ __forceinline__ void wave_rows(const int Kp, int &k0, int &k1) {
  const int wave = (int)(threadIdx.x >> 6), per = (Kp + kWideWaves - 1) / kWideWaves;
  k0 = min(Kp, wave * per);
  k1 = min(Kp, k0 + per);
}

}  // namespace pdt
