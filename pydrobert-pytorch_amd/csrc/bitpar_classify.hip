// Classification as a launch of its own: lev_classify_kernel leaves the tables of
// classify_utterance (bitpar_classify.hpp) in the caller's workspace (pdt_lev_workspace_bytes,
// pdt_oc_mask_workspace_bytes) for lev_bitpar_staged_kernel / oc_bitpar_staged_kernel.  The shapes
// whose plan says `fused` / `oc_fused` never come here: their recurrence kernels classify for
// themselves.
#include "bitpar_classify.hpp"
#include "lev_launch.hpp"

namespace pdt {

// ---- classification into the workspace ---------------------------------------------------------
// (Time-major inputs cost this kernel ~15 us at the bench shape -- a wave's tokens sit in 512
// different 32-byte sectors; reading (T, 4) strips with the whole workgroup and exchanging them
// through LDS measured no better.)
template <int NR>
__global__ void __launch_bounds__(256) lev_classify_kernel(const BitparArgs a, const int lds_per_wave) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  // (time-major tokens: one 128-byte line of a row holds 16 neighbouring utterances' tokens = four
  // workgroups; with the XCD-aware order those four run on ONE XCD and its L2 fetches the line once
  // -- under the dispatcher's round-robin they sat on four XCDs and HBM delivered it four times)
  const int64_t n = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
  if (n >= a.N) return;  // waves never synchronise with each other
  unsigned char *base = smem + (size_t)wave * lds_per_wave;
  const int X = a.X > 0 ? a.X : 1, Y = a.Y > 0 ? a.Y : 1;
  // [(presence, offset) per class: X * 8] [distinct tokens (X + 1) * 8; later the packed mask
  // words] [classes of Y, 2 bytes each]
  uint2 *po = reinterpret_cast<uint2 *>(base);
  int64_t *ctok = reinterpret_cast<int64_t *>(base + (size_t)X * 8);
  unsigned *msk = reinterpret_cast<unsigned *>(ctok);
  short *yc = reinterpret_cast<short *>(ctok + max(X + 1, kDirectWords));
  const Classified c = classify_utterance<NR, kClassifyStaged>(a, n, po, ctok, msk, yc, nullptr);
  for (int j = lane; j < c.y_len; j += PDT_WAVE) {
    const int k = yc[j];
    a.yh[n * (int64_t)Y + j] = k >= 0 ? po[k] : make_uint2(0u, 0u);
  }
  for (int i = lane; i <= c.x_len; i += PDT_WAVE) a.msk[n * (int64_t)(X + 1) + i] = msk[i];
  if (lane == 0) {
    a.lens[2 * n] = c.ref_len;
    a.lens[2 * n + 1] = c.hyp_len;
  }
}

// One workgroup of four waves per four utterances; 0 or the error of asking for the LDS.  (The launch
// itself reports through the hipGetLastError of the recurrence launch that follows.)
int launch_bitpar_classify(const BitparArgs &a, const BitparPlan &p, hipStream_t stream) {
  auto ck = a.X <= 8 * PDT_WAVE ? lev_classify_kernel<8> : lev_classify_kernel<16>;
  const int rc = set_lds(ck, p.lds_classify * 4);
  if (rc) return rc;
  hipLaunchKernelGGL(ck, dim3((unsigned)((a.N + 3) / 4)), dim3(256), p.lds_classify * 4, stream, a,
                     (int)p.lds_classify);
  return 0;
}

}  // namespace pdt
