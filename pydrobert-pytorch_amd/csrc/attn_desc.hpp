// What the attention translation units share (attn.hip, attn_mfma.hip, attn_mfma_bwd.hip): the descriptor as the
// kernels read it, the kernel arguments, a row's element offsets, and the host functions of attn.hip that the
// matrix-core files call.
#pragma once
#include "pdt_common.hpp"

namespace pdt {

enum { SQ = 0, SK, SV, SM, SO, SGQ, SGK, SGV, NSLOT };  // Q doubles as E, GQ as GE in the pool forms

struct AttnDesc {
  int64_t nd, R, G, M, T, D, Dv;
  int64_t size[PDT_ATTN_MAX_DIMS];
  int64_t st[NSLOT][PDT_ATTN_MAX_DIMS];
  int64_t ts[NSLOT], fs[NSLOT];
};

struct AttnArgs {
  AttnDesc d;
  const void *q, *k, *v, *e;
  const uint8_t *mask;
  const void *out, *lse, *gout;
  void *o, *l, *gq, *gk, *gv, *ge;
  void *ws;
  double scale;
  int64_t rt;      // rows per tile
  int64_t tiles;   // row tiles per group
  int64_t splits;  // forward: spans of T; backward: frame chunks
  int64_t span;    // frames per span (forward)
};

// element offsets of row r in every operand slot (row dims innermost last; static indexing only)
__device__ __forceinline__ void attn_row_offsets(const AttnDesc &d, int64_t r, int64_t off[NSLOT]) {
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) off[s] = 0;
#pragma unroll
  for (int i = PDT_ATTN_MAX_DIMS - 1; i >= 0; --i) {
    if (i < d.nd) {
      const int64_t n = d.size[i], idx = r % n;
      r /= n;
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) off[s] += idx * d.st[s][i];
    }
  }
}

enum { ATTN_DOT = 0, ATTN_DOT_BWD = 1, ATTN_POOL = 2, ATTN_POOL_BWD = 3 };

// attn.hip: reads and checks a descriptor (PDT_OK or PDT_E_ARG)
int attn_desc(const int64_t *in, int kind, AttnDesc *d);
// attn.hip: launches attn_fwd_combine_kernel<E> over the split partials in a.ws (et: 2 f16_t, 3 bf16_t, 1 double,
// else float)
int attn_fwd_combine_launch(AttnArgs &a, int et, hipStream_t s);
// attn.hip: the workspace bytes of the float32 dot forward on attn_fwd_kernel (what pdt_attn_workspace_bytes reports;
// attn_mfma_dec.hip keeps its own partials within it)
int64_t attn_fwd_tile_ws_bytes(const AttnDesc &d);
// attn.hip: launches attn_delta_kernel<E>: delta[r] = sum_c grad_out[r, c] * out[r, c] into a.ws (et as above)
int attn_delta_launch(AttnArgs &a, int et, hipStream_t s);

}  // namespace pdt
