// The per-column error reduction of the K-column handles, kernel and launch: included by
// fu_rev_round.h (the rev-gather round of fu_lossy.hip and fu_churn.hip at K columns) and by
// fu_pair.hip (fu_pair_create_k). It sits on csrc/fu_handle.h. DESIGN.md §4.19, §4.22.
#pragma once

#include "fu_handle.h"

namespace fu {
namespace {

// A handle of K value columns (*_create_k) has at most this many.
constexpr int kMaxCols = 16;

// The per-column error reduction of every K-column handle (the rev-gather round's and the pair
// engine's), with the block size and the index type it was written over.
namespace cols_err {
constexpr int kBlock = 256;
using i64 = long long;

// max |a - target| per column as uint64 bit patterns, the rule of the scaffold's k_max_err for
// a_old = x[i * K + c]: a NaN raises its own column's slot and no other. With `alive`, over the
// alive nodes only. Each thread keeps one column: a block uses (kBlock / K) * K threads and the
// stride is a multiple of K.
__global__ __launch_bounds__(kBlock) void k_max_err_cols(i64 total, int K, const double *__restrict__ a,
                                                         const double *__restrict__ target,
                                                         const unsigned char *__restrict__ alive, u64 *__restrict__ err) {
  __shared__ u64 s_m[kMaxCols];
  const int tb = (kBlock / K) * K;
  const int tid = threadIdx.x;
  if (tid < kMaxCols) s_m[tid] = 0ull;
  __syncthreads();
  if (tid < tb) {
    u64 m = 0ull;
    const i64 stride = (i64)gridDim.x * tb;
    for (i64 q = (i64)blockIdx.x * tb + tid; q < total; q += stride) {
      if (alive != nullptr && !alive[q / K]) continue;
      const u64 x = (u64)__double_as_longlong(fabs(a[q] - target[q]));
      m = x > m ? x : m;
    }
    if (m) atomicMax(&s_m[tid % K], m);
  }
  __syncthreads();
  if (tid < K && s_m[tid]) atomicMax(&err[tid], s_m[tid]);
}

// launch_err of a handle of K = h->width columns: a holds n * K doubles, alive may be null, the
// K maxima go to slot[0 .. K-1]. The kernel's block is its own, whatever the includer's is.
inline int launch(const handle_base *h, const double *a, const unsigned char *alive, u64 *slot) {
  const int K = h->width;
  const i64 total = (i64)h->n * K;
  const int tb = (kBlock / K) * K;
  const unsigned grid = (unsigned)std::min<i64>(1024, (total + tb - 1) / tb);
  hipLaunchKernelGGL(k_max_err_cols, dim3(grid), dim3(kBlock), 0, h->stream, total, K, a, h->target, alive, slot);
  HIP_TRY(hipGetLastError());
  return FU_OK;
}
}  // namespace cols_err

}  // namespace
}  // namespace fu
