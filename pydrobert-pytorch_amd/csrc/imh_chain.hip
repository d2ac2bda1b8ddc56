// The accept / reject recurrence of independent Metropolis-Hastings (reference _mc.py:715-733), as a
// scan down each batch column.  ratio[n] = log P - log Q of proposal n, last = the ratio of the sample
// the chain stands on (ratio0 to start with).  For n = 0 .. M - 1: accept iff (ratio[n] - last) >
// log_u[n], one subtraction and one comparison in the data's type; on accept last = ratio[n] and
// idx[n] = n, otherwise idx[n] = idx[n - 1], from -1, the sample carried in.  `last` is SELECTED (the
// reference's accept * cur + (~accept) * last turns a rejected -inf into NaN, after which nothing is
// accepted again).  A NaN on either side of the comparison rejects.
//
// Lane = column: the chain is serial in M, so the loads of eight steps are issued ahead of it, as
// return_columns_kernel does; ratio and log_u are read through element strides, idx is dense.
#include "pdt_common.hpp"

namespace pdt {
namespace {

enum { IMH_F32 = 0, IMH_F64 = 1 };
constexpr int kImhThreads = 256;

template <typename T> struct ImhArgs {
  const T *ratio, *ratio0, *log_u;
  int64_t M, B, r_sm, r_sb, r0_s, u_sm, u_sb;
  int32_t *idx;  // (M, B)
  T *last;       // (B,)
  int32_t *last_idx;  // (B,)
};

template <typename T> __global__ void __launch_bounds__(kImhThreads) imh_chain_kernel(const ImhArgs<T> a) {
  const int64_t b = (int64_t)blockIdx.x * kImhThreads + (int)threadIdx.x;
  if (b >= a.B) return;
  const T *__restrict__ r = a.ratio + b * a.r_sb;
  const T *__restrict__ u = a.log_u + b * a.u_sb;
  int32_t *__restrict__ idx = a.idx + b;
  T last = a.ratio0[b * a.r0_s];
  int32_t cur = -1;
  int64_t n = 0;
  for (; n + 8 <= a.M; n += 8) {
    T rv[8], uv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) rv[i] = r[(n + i) * a.r_sm], uv[i] = u[(n + i) * a.u_sm];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool accept = (rv[i] - last) > uv[i];
      last = accept ? rv[i] : last;
      cur = accept ? (int32_t)(n + i) : cur;
      idx[(n + i) * a.B] = cur;
    }
  }
  for (; n < a.M; ++n) {
    const T rv = r[n * a.r_sm];
    const bool accept = (rv - last) > u[n * a.u_sm];
    last = accept ? rv : last;
    cur = accept ? (int32_t)n : cur;
    idx[n * a.B] = cur;
  }
  a.last[b] = last;
  a.last_idx[b] = cur;
}

template <typename T>
int launch(const void *ratio, int64_t r_sm, int64_t r_sb, const void *ratio0, int64_t r0_s, const void *log_u,
           int64_t u_sm, int64_t u_sb, int64_t M, int64_t B, int32_t *idx, void *last, int32_t *last_idx, hipStream_t s) {
  const int64_t blocks = (B + kImhThreads - 1) / kImhThreads;
  if (blocks > 0x7fffffffLL) return PDT_E_TOO_LONG;
  ImhArgs<T> a{(const T *)ratio, (const T *)ratio0, (const T *)log_u, M, B, r_sm, r_sb, r0_s, u_sm, u_sb,
               idx, (T *)last, last_idx};
  hipLaunchKernelGGL(imh_chain_kernel<T>, dim3((unsigned)blocks), dim3(kImhThreads), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace pdt

extern "C" int pdt_imh_chain(int dtype, const void *ratio, int64_t r_sm, int64_t r_sb, const void *ratio0,
                             int64_t r0_s, const void *log_u, int64_t u_sm, int64_t u_sb, int64_t M, int64_t B,
                             int32_t *idx, void *last, int32_t *last_idx, void *stream) {
  if ((dtype != pdt::IMH_F32 && dtype != pdt::IMH_F64) || M < 0 || B < 0) return PDT_E_ARG;
  if (M > 0x7fffffffLL) return PDT_E_TOO_LONG;  // (idx is int32)
  if (B == 0) return PDT_OK;
  if (ratio0 == nullptr || last == nullptr || last_idx == nullptr) return PDT_E_ARG;
  if (M > 0 && (ratio == nullptr || log_u == nullptr || idx == nullptr)) return PDT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == pdt::IMH_F32)
    return pdt::launch<float>(ratio, r_sm, r_sb, ratio0, r0_s, log_u, u_sm, u_sb, M, B, idx, last, last_idx, s);
  return pdt::launch<double>(ratio, r_sm, r_sb, ratio0, r0_s, log_u, u_sm, u_sb, M, B, idx, last, last_idx, s);
}
