// What crosses the file boundaries of the image kernels on the host (spline.hip, image_warp.hip):
// the solver both the spline entry points and the sparse warp call, and the constants by which
// pdt_spline_workspace_bytes sizes the one workspace they share.  Both files include it, so a
// signature that changes on one side only fails to compile.
#pragma once
#include "pdt_common.hpp"

namespace pdt {

// T + I + 1 up to which the augmented system of one batch element fits the 160 KB of LDS (with
// O <= 4 right-hand sides); larger systems are eliminated in a global-memory workspace
constexpr size_t kSplineLdsCap = 160 * 1024 - 64;

// image_warp.hip: sparse_warp_bands_kernel's per-image table, which follows the solutions in the workspace
constexpr int kWarpTableFloats = 40;  // per image: 4 * 8 + 6, rounded up to 16 bytes (workspace stride)
__host__ __device__ constexpr int warp_table_stride(int MC) { return (4 * MC + 6 + 3) & ~3; }

// spline.hip: solve the N bordered systems into wv (N, T + I + 1, O) doubles at the head of the workspace
int spline_solve(const float *c, const float *f, const float *tail, int64_t N, int64_t T, int64_t I, int64_t O,
                 int order, float reg, double *wv, hipStream_t stream);

}  // namespace pdt
