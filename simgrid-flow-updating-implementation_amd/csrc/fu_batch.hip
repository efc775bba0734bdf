// libfu batched collect-all engine for MI355X (gfx950): K value columns over one graph in one
// pass per round. C ABI: the fu_batch section of include/fu.h. DESIGN.md §4.15.
//
// Every column is an independent scalar run of SURVEY.md App. A.1:
//   fr[e] = -f_prev[rev e], er[e] = a_prev[col e]
//   S = 0.0 + fr[e0] + fr[e1] + ...  (left to right, row order),  T likewise over er
//   a = ((v - S) + T) / (deg + 1),   f[e] = (fr[e] + a) - er[e]
// with the reverse flow reconstructed as kernel 4 does: node i holds
// f_{r-2}[i->j], a_{r-2}[i] and gathers a_{r-1}[j], so
//   f_{r-1}[j->i] = ((-f_{r-2}[i->j]) + a_{r-1}[j]) - a_{r-2}[i]
// comes out of the same IEEE operations node j ran. No reverse-edge index on the device.
//
// Layout: estimates node-major A[i * K + k], flows edge-major F[e * K + k] in the caller's
// CSR order, so the K estimates of a neighbour are one contiguous K * 8-byte gather and the
// column index, the row pointers and the degree are read once for all columns. Offsets are
// 64-bit (E * K may pass 2^31). State as in the scalar engine: F[r & 1] updated in place
// (f_{r-2} -> f_r), A[r % 3] = a_r.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fu_common.h"

using namespace fu;

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return fu::fail(FU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
  } while (0)

namespace {

constexpr int kBlock = 256;     // threads per block (4 waves of 64)
constexpr int kMaxK = 16;       // columns per handle
constexpr int kRegDeg = 16;     // light rows up to this degree keep (fr, er) in registers
constexpr int kHeavyDeg = 64;   // rows above this degree run one block per row
constexpr int kChunk = 2048;    // heavy rows: (fr, er) elements staged in LDS per chunk

using i64 = long long;

// The flow two rounds back: round 1 reads f_{-1} = -0.0 and round 2 reads
// f_0 = (0.0 + a_0[i]) - 0.0 without memory (round 0 writes no flows); fm 0 reads F.
__device__ inline double old_flow(int fm, const double *__restrict__ F, i64 idx, double own2) {
  if (fm == 1) return -0.0;
  if (fm == 2) return (0.0 + own2) - 0.0;
  return F[idx];
}

// fr = -f_{r-1}[j->i], rebuilt from node i's own operands and the gathered a_{r-1}[j]
__device__ inline double recon(double f2, double er, double own2) { return -(((-f2) + er) - own2); }

// Round 0: the timeout fire on zero state; a_{-1} = 0.0. One thread per (row, column).
__global__ __launch_bounds__(kBlock) void kb_round0(i64 total, int K, const i64 *__restrict__ rowptr,
                                                    const double *__restrict__ v, double *__restrict__ a0,
                                                    double *__restrict__ a_m1) {
  const i64 t = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (t >= total) return;
  const i64 row = t / K;
  a_m1[t] = 0.0;
  a0[t] = ((v[t] - 0.0) + 0.0) / (double)(rowptr[row + 1] - rowptr[row] + 1);
}

// f_0[i->j] = (0.0 + a_0[i]) - 0.0, on demand (fu_batch_get_flows after round 0 alone)
__global__ __launch_bounds__(kBlock) void kb_flows0(i64 total, int K, const i64 *__restrict__ rowptr,
                                                    const double *__restrict__ a0, double *__restrict__ F) {
  const i64 t = (i64)blockIdx.x * kBlock + threadIdx.x;
  if (t >= total) return;
  const i64 row = t / K;
  const int k = (int)(t - row * K);
  const double f = (0.0 + a0[t]) - 0.0;
  for (i64 e = rowptr[row]; e < rowptr[row + 1]; ++e) F[e * K + k] = f;
}

// Rows of degree <= kHeavyDeg: one thread per (row, column); each thread owns one sequential
// chain. The K threads of a row gather K contiguous doubles per edge and read and write K
// contiguous flows; consecutive rows' flows are consecutive in memory. Loads come in groups
// of four edges, each lane loading only the edges its row has; a group is skipped when no
// row of the wave reaches it. Rows up to kRegDeg keep (fr, er) in registers for the flow
// pass; longer light rows load them again.
__global__ __launch_bounds__(kBlock) void kb_light(i64 total, int K, int fm, const i64 *__restrict__ rowptr,
                                                   const int *__restrict__ col, const double *__restrict__ v,
                                                   const double *__restrict__ a1, const double *__restrict__ a2,
                                                   double *__restrict__ a_out, double *__restrict__ F) {
  const i64 t = (i64)blockIdx.x * kBlock + threadIdx.x;
  const bool live = t < total;
  const i64 tc = live ? t : 0;  // total >= 1
  const i64 row = tc / K;
  const int k = (int)(tc - row * K);
  const i64 b = rowptr[row];
  const i64 dl = rowptr[row + 1] - b;
  const bool mine = live && dl <= kHeavyDeg;  // heavy rows: kb_heavy
  const int d = mine ? (int)dl : 0;
  const double own2 = a2[tc], val = v[tc];
  double S = 0.0, T = 0.0, a;
  if (d <= kRegDeg) {
    double fr[kRegDeg], er[kRegDeg];
#pragma unroll
    for (int g = 0; g < kRegDeg; g += 4) {
      if (__any(d > g)) {
        bool on[4];
        i64 e[4];
        int c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          on[u] = g + u < d;
          e[u] = b + g + u;
          c[u] = on[u] ? col[e[u]] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          er[g + u] = on[u] ? a1[(i64)c[u] * K + k] : 0.0;
          fr[g + u] = on[u] ? old_flow(fm, F, e[u] * K + k, own2) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) fr[g + u] = recon(fr[g + u], er[g + u], own2);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) fr[g + u] = er[g + u] = 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < kRegDeg; ++j)
      if (j < d) {
        S = S + fr[j];
        T = T + er[j];
      }
    a = ((val - S) + T) / (double)(d + 1);
#pragma unroll
    for (int j = 0; j < kRegDeg; ++j)
      if (j < d) F[(b + j) * K + k] = (fr[j] + a) - er[j];
  } else {
    for (int j0 = 0; j0 < d; j0 += 4) {
      double fr[4], er[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const i64 e = b + (j0 + u < d ? j0 + u : d - 1);
        er[u] = a1[(i64)col[e] * K + k];
        fr[u] = recon(old_flow(fm, F, e * K + k, own2), er[u], own2);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j0 + u < d) {
          S = S + fr[u];
          T = T + er[u];
        }
    }
    a = ((val - S) + T) / (double)(d + 1);
    for (int j = 0; j < d; ++j) {
      const i64 e = b + j;
      const double er = a1[(i64)col[e] * K + k];
      const double fr = recon(old_flow(fm, F, e * K + k, own2), er, own2);
      F[e * K + k] = (fr + a) - er;
    }
  }
  if (mine) a_out[t] = a;
}

// Rows above kHeavyDeg: one block per row. All threads load a chunk of (edge, column)
// elements coalesced and leave (fr, er) in LDS; K lanes then run the K chains through the
// chunk in row order, carrying S and T from chunk to chunk. Once a is known, the flow pass
// rebuilds (fr, er) per element (the operands are unchanged: F is written only here, by
// the thread that read the element) and writes the flows coalesced.
__global__ __launch_bounds__(kBlock) void kb_heavy(int K, int fm, const int *__restrict__ hrows,
                                                   const i64 *__restrict__ rowptr, const int *__restrict__ col,
                                                   const double *__restrict__ v, const double *__restrict__ a1,
                                                   const double *__restrict__ a2, double *__restrict__ a_out,
                                                   double *__restrict__ F) {
  __shared__ double s_fr[kChunk], s_er[kChunk];
  __shared__ double s_a[kMaxK], s_own2[kMaxK];
  const int tid = threadIdx.x;
  const i64 row = hrows[blockIdx.x];
  const i64 b = rowptr[row];
  const i64 d = rowptr[row + 1] - b;
  if (tid < K) s_own2[tid] = a2[row * K + tid];
  __syncthreads();
  const int ce = kChunk / K;  // edges per chunk
  double S = 0.0, T = 0.0;
  for (i64 e0 = 0; e0 < d; e0 += ce) {
    const int ne = (int)(d - e0 < ce ? d - e0 : ce);
    const int m = ne * K;  // <= kChunk
    for (int q = tid; q < m; q += kBlock) {
      const int je = q / K, kk = q - je * K;
      const i64 e = b + e0 + je;
      const double er = a1[(i64)col[e] * K + kk];
      const double own2 = s_own2[kk];
      s_er[q] = er;
      s_fr[q] = recon(old_flow(fm, F, e * K + kk, own2), er, own2);
    }
    __syncthreads();
    if (tid < K)
      for (int je = 0; je < ne; ++je) {
        S = S + s_fr[je * K + tid];
        T = T + s_er[je * K + tid];
      }
    __syncthreads();
  }
  if (tid < K) {
    const double a = ((v[row * K + tid] - S) + T) / (double)(d + 1);
    a_out[row * K + tid] = a;
    s_a[tid] = a;
  }
  __syncthreads();
  const i64 m = d * K;
  for (i64 q = tid; q < m; q += kBlock) {
    const i64 je = q / K;
    const int kk = (int)(q - je * K);
    const i64 e = b + je;
    const double er = a1[(i64)col[e] * K + kk];
    const double own2 = s_own2[kk];
    const double fr = recon(old_flow(fm, F, e * K + kk, own2), er, own2);
    F[e * K + kk] = (fr + s_a[kk]) - er;
  }
}

// max |a - target| per column as uint64 bit patterns (non-negative doubles order like their
// bits; a NaN with its sign cleared is above +inf, so a NaN stays in its own column). Each
// thread keeps one column: a block uses (kBlock / K) * K threads and the stride is a
// multiple of K.
__global__ __launch_bounds__(kBlock) void kb_max_err(i64 total, int K, const double *__restrict__ a,
                                                     const double *__restrict__ target,
                                                     unsigned long long *__restrict__ err) {
  __shared__ unsigned long long s_m[kMaxK];
  const int tb = (kBlock / K) * K;
  const int tid = threadIdx.x;
  if (tid < kMaxK) s_m[tid] = 0ull;
  __syncthreads();
  if (tid < tb) {
    unsigned long long m = 0ull;
    const i64 stride = (i64)gridDim.x * tb;
    for (i64 q = (i64)blockIdx.x * tb + tid; q < total; q += stride) {
      const unsigned long long x = (unsigned long long)__double_as_longlong(fabs(a[q] - target[q]));
      m = x > m ? x : m;
    }
    if (m) atomicMax(&s_m[tid % K], m);
  }
  __syncthreads();
  if (tid < K && s_m[tid]) atomicMax(&err[tid], s_m[tid]);
}

inline unsigned grid_for(i64 work) { return (unsigned)((work + kBlock - 1) / kBlock); }

}  // namespace

struct fu_batch {
  int device = 0;
  int32_t n = 0, k = 0;
  int64_t E = 0;
  int64_t round = 0;
  bool has_target = false;
  int32_t n_heavy = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  i64 *rowptr = nullptr;
  int *col = nullptr, *hrows = nullptr;
  double *v = nullptr, *target = nullptr, *a[3] = {nullptr, nullptr, nullptr}, *f[2] = {nullptr, nullptr};
  unsigned long long *err = nullptr;
  int64_t errcap = 0;
};

namespace {

template <typename T>
int dmalloc(T **p, int64_t count) {
  if (hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * (size_t)std::max<int64_t>(count, 1)) != hipSuccess) {
    *p = nullptr;
    return fail(FU_ERR_ALLOC, "fu_batch: hipMalloc failed");
  }
  return FU_OK;
}

int set_device(fu_batch *b) {
  HIP_TRY(hipSetDevice(b->device));
  return FU_OK;
}

int err_slots(fu_batch *b, int64_t count) {
  if (count <= b->errcap) return FU_OK;
  if (b->err) hipFree(b->err);
  b->err = nullptr;
  b->errcap = 0;
  if (int rc = dmalloc(&b->err, count)) return rc;
  b->errcap = count;
  return FU_OK;
}

int launch_err(fu_batch *b, unsigned long long *slot) {
  const i64 total = (i64)b->n * b->k;
  const int tb = (kBlock / b->k) * b->k;
  const unsigned grid = (unsigned)std::min<i64>(1024, (total + tb - 1) / tb);
  hipLaunchKernelGGL(kb_max_err, dim3(grid), dim3(kBlock), 0, b->stream, total, b->k,
                     b->a[(b->round + 2) % 3], b->target, slot);  // a_{round-1}: the last round run
  HIP_TRY(hipGetLastError());
  return FU_OK;
}

int launch_round(fu_batch *b) {
  const int64_t r = b->round;
  const i64 total = (i64)b->n * b->k;
  if (r == 0) {
    hipLaunchKernelGGL(kb_round0, dim3(grid_for(total)), dim3(kBlock), 0, b->stream, total, b->k, b->rowptr, b->v,
                       b->a[0], b->a[2]);
  } else {
    const int fm = r == 1 ? 1 : r == 2 ? 2 : 0;
    double *a1 = b->a[(r + 2) % 3], *a2 = b->a[(r + 1) % 3], *ao = b->a[r % 3], *F = b->f[r & 1];
    hipLaunchKernelGGL(kb_light, dim3(grid_for(total)), dim3(kBlock), 0, b->stream, total, b->k, fm, b->rowptr, b->col,
                       b->v, a1, a2, ao, F);
    if (b->n_heavy > 0)
      hipLaunchKernelGGL(kb_heavy, dim3(b->n_heavy), dim3(kBlock), 0, b->stream, b->k, fm, b->hrows, b->rowptr, b->col,
                         b->v, a1, a2, ao, F);
  }
  HIP_TRY(hipGetLastError());
  b->round = r + 1;
  return FU_OK;
}

}  // namespace

extern "C" {

int fu_batch_destroy(fu_batch *b) {
  if (!b) return fail(FU_ERR_ARG, "fu_batch_destroy: bad arguments");
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (void *p : {(void *)b->rowptr, (void *)b->col, (void *)b->hrows, (void *)b->v, (void *)b->target, (void *)b->a[0],
                  (void *)b->a[1], (void *)b->a[2], (void *)b->f[0], (void *)b->f[1], (void *)b->err})
    if (p) (void)hipFree(p);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
  return FU_OK;
}

// Every check on the arguments comes before the first HIP call, so a host without a GPU
// reports a bad k or an asymmetric graph as such.
int fu_batch_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev, int32_t k,
                    const double *value, int32_t device, fu_batch **out) {
  FU_TRY_BEGIN
  if (!out || !rowptr || !value || n <= 0 || e < 0 || (e > 0 && !col)) return fail(FU_ERR_ARG, "fu_batch_create: bad arguments");
  if (k < 1 || k > kMaxK) return fail(FU_ERR_ARG, "fu_batch_create: k must be in 1..16, got " + std::to_string(k));
  if (rowptr[0] != 0 || rowptr[n] != e) return fail(FU_ERR_ARG, "fu_batch_create: rowptr[0] must be 0 and rowptr[n] == e");
  std::vector<int32_t> heavy;
  for (int32_t i = 0; i < n; ++i) {
    if (rowptr[i + 1] < rowptr[i]) return fail(FU_ERR_ARG, "fu_batch_create: rowptr not monotone");
    if (rowptr[i + 1] - rowptr[i] > kHeavyDeg) heavy.push_back(i);
  }
  for (int64_t q = 0; q < e; ++q)
    if (col[q] < 0 || col[q] >= n) return fail(FU_ERR_ARG, "fu_batch_create: col index out of range at edge " + std::to_string(q));
  if (e > 0 && !rev) {  // the flow reconstruction needs every i -> j to have its j -> i
    fu_graph g;
    g.n = n;
    g.rowptr.assign(rowptr, rowptr + n + 1);
    g.col.assign(col, col + e);
    if (int rc = fu::build_rev(g)) return rc;
  } else if (e > 0) {
    for (int32_t i = 0; i < n; ++i)
      for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
        const int32_t j = col[q];
        const int64_t r = rev[q];
        if (r < rowptr[j] || r >= rowptr[j + 1] || col[r] != i)
          return fail(FU_ERR_GRAPH, "fu_batch_create: rev is not the reverse-edge pairing (the graph must be symmetric) at edge " +
                                        std::to_string(q));
      }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FU_ERR_HIP, "fu_batch_create: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(FU_ERR_ARG, "fu_batch_create: device out of range");
  auto *b = new fu_batch();
  b->device = device;
  b->n = n;
  b->k = k;
  b->E = e;
  b->n_heavy = (int32_t)heavy.size();
  auto cleanup = [&](int code) { fu_batch_destroy(b); return code; };
  int rc = FU_OK;
  if ((rc = set_device(b))) return cleanup(rc);
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_batch_create: hipStreamCreate failed"));
  if (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_batch_create: hipEventCreate failed"));
  const int64_t nk = (int64_t)n * k, ek = e * k;
  if ((rc = dmalloc(&b->rowptr, (int64_t)n + 1)) || (rc = dmalloc(&b->col, e)) || (rc = dmalloc(&b->hrows, b->n_heavy)) ||
      (rc = dmalloc(&b->v, nk)) || (rc = dmalloc(&b->target, nk)) || (rc = dmalloc(&b->a[0], nk)) ||
      (rc = dmalloc(&b->a[1], nk)) || (rc = dmalloc(&b->a[2], nk)) || (rc = dmalloc(&b->f[0], ek)) ||
      (rc = dmalloc(&b->f[1], ek)) || (rc = err_slots(b, k)))
    return cleanup(rc);
  static_assert(sizeof(i64) == sizeof(int64_t), "rowptr is uploaded as is");
  if (hipMemcpy(b->rowptr, rowptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice) != hipSuccess ||
      (e && hipMemcpy(b->col, col, sizeof(int32_t) * (size_t)e, hipMemcpyHostToDevice) != hipSuccess) ||
      (b->n_heavy && hipMemcpy(b->hrows, heavy.data(), sizeof(int32_t) * heavy.size(), hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(b->v, value, sizeof(double) * (size_t)nk, hipMemcpyHostToDevice) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_batch_create: upload failed"));
  if ((e == 0 && hipMemset(b->col, 0, sizeof(int32_t)) != hipSuccess) ||
      hipMemset(b->a[0], 0, sizeof(double) * (size_t)nk) != hipSuccess ||
      hipMemset(b->a[1], 0, sizeof(double) * (size_t)nk) != hipSuccess ||
      hipMemset(b->a[2], 0, sizeof(double) * (size_t)nk) != hipSuccess ||
      hipMemset(b->f[0], 0, sizeof(double) * (size_t)std::max<int64_t>(ek, 1)) != hipSuccess ||
      hipMemset(b->f[1], 0, sizeof(double) * (size_t)std::max<int64_t>(ek, 1)) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_batch_create: memset failed"));
  *out = b;
  return FU_OK;
  FU_TRY_END
}

int fu_batch_create_from_graph(const fu_graph *g, int32_t k, const double *value, int32_t device, fu_batch **out) {
  FU_TRY_BEGIN
  if (!g || !value || !out) return fail(FU_ERR_ARG, "fu_batch_create_from_graph: bad arguments");
  if (k < 1 || k > kMaxK) return fail(FU_ERR_ARG, "fu_batch_create_from_graph: k must be in 1..16, got " + std::to_string(k));
  const int64_t E = g->rowptr[g->n];
  if ((int64_t)g->rev.size() != E) return fail(FU_ERR_GRAPH, "fu_batch_create_from_graph: graph is not symmetric");
  return fu_batch_create(g->n, E, g->rowptr.data(), g->col.data(), E ? g->rev.data() : nullptr, k, value, device, out);
  FU_TRY_END
}

int fu_batch_reset(fu_batch *b) {
  if (!b) return fail(FU_ERR_ARG, "fu_batch_reset: bad arguments");
  if (int rc = set_device(b)) return rc;
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->round = 0;  // round 0 rewrites a_0 and a_{-1}; rounds 1 and 2 write their flows without reading any
  return FU_OK;
}

int fu_batch_set_targets(fu_batch *b, const double *target) {
  FU_TRY_BEGIN
  if (!b || !target) return fail(FU_ERR_ARG, "fu_batch_set_targets: bad arguments");
  if (int rc = set_device(b)) return rc;
  HIP_TRY(hipMemcpyAsync(b->target, target, sizeof(double) * (size_t)b->n * b->k, hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->has_target = true;
  return FU_OK;
  FU_TRY_END
}

int fu_batch_run(fu_batch *b, int32_t rounds, int32_t err_every, double *err_trace) {
  FU_TRY_BEGIN
  if (!b || rounds < 0) return fail(FU_ERR_ARG, "fu_batch_run: bad arguments");
  if (err_every > 0 && !b->has_target) return fail(FU_ERR_STATE, "fu_batch_run: err_every > 0 needs fu_batch_set_targets");
  if (int rc = set_device(b)) return rc;
  const int64_t nerr = err_every > 0 ? rounds / err_every : 0;
  if (nerr > 0) {
    if (int rc = err_slots(b, nerr * b->k)) return rc;
    HIP_TRY(hipMemsetAsync(b->err, 0, sizeof(unsigned long long) * (size_t)(nerr * b->k), b->stream));
  }
  for (int32_t r = 0; r < rounds; ++r) {
    if (int rc = launch_round(b)) return rc;
    if (nerr > 0 && (r + 1) % err_every == 0)
      if (int rc = launch_err(b, b->err + (int64_t)((r + 1) / err_every - 1) * b->k)) return rc;
  }
  if (nerr > 0) {
    std::vector<unsigned long long> bits((size_t)(nerr * b->k));
    HIP_TRY(hipMemcpyAsync(bits.data(), b->err, sizeof(unsigned long long) * bits.size(), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (err_trace) std::memcpy(err_trace, bits.data(), sizeof(double) * bits.size());
  }
  return FU_OK;
  FU_TRY_END
}

int fu_batch_run_timed(fu_batch *b, int32_t rounds, float *ms) {
  FU_TRY_BEGIN
  if (!b || !ms || rounds < 0) return fail(FU_ERR_ARG, "fu_batch_run_timed: bad arguments");
  if (int rc = set_device(b)) return rc;
  HIP_TRY(hipEventRecord(b->ev0, b->stream));
  for (int32_t r = 0; r < rounds; ++r)
    if (int rc = launch_round(b)) return rc;
  HIP_TRY(hipEventRecord(b->ev1, b->stream));
  HIP_TRY(hipEventSynchronize(b->ev1));
  HIP_TRY(hipEventElapsedTime(ms, b->ev0, b->ev1));
  return FU_OK;
  FU_TRY_END
}

int fu_batch_max_err(fu_batch *b, double *out) {
  FU_TRY_BEGIN
  if (!b || !out) return fail(FU_ERR_ARG, "fu_batch_max_err: bad arguments");
  if (!b->has_target) return fail(FU_ERR_STATE, "fu_batch_max_err: call fu_batch_set_targets first");
  if (b->round == 0) return fail(FU_ERR_STATE, "fu_batch_max_err: no round has run");
  if (int rc = set_device(b)) return rc;
  HIP_TRY(hipMemsetAsync(b->err, 0, sizeof(unsigned long long) * b->k, b->stream));
  if (int rc = launch_err(b, b->err)) return rc;
  unsigned long long bits[kMaxK];
  HIP_TRY(hipMemcpyAsync(bits, b->err, sizeof(unsigned long long) * b->k, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  std::memcpy(out, bits, sizeof(double) * b->k);
  return FU_OK;
  FU_TRY_END
}

int fu_batch_get_estimates(fu_batch *b, double *a_out) {
  FU_TRY_BEGIN
  if (!b || !a_out) return fail(FU_ERR_ARG, "fu_batch_get_estimates: bad arguments");
  const size_t nk = (size_t)b->n * b->k;
  if (b->round == 0) {  // zero state
    std::fill(a_out, a_out + nk, 0.0);
    return FU_OK;
  }
  if (int rc = set_device(b)) return rc;
  HIP_TRY(hipMemcpyAsync(a_out, b->a[(b->round + 2) % 3], sizeof(double) * nk, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return FU_OK;
  FU_TRY_END
}

int fu_batch_get_flows(fu_batch *b, double *f_out) {
  FU_TRY_BEGIN
  if (!b || (!f_out && b->E)) return fail(FU_ERR_ARG, "fu_batch_get_flows: bad arguments");
  if (b->E == 0) return FU_OK;
  const size_t ek = (size_t)b->E * b->k;
  if (b->round == 0) {  // zero state
    std::fill(f_out, f_out + ek, 0.0);
    return FU_OK;
  }
  if (int rc = set_device(b)) return rc;
  if (b->round == 1) {  // round 0 wrote no flows: f_0 on demand (round 2 never reads it from memory)
    const i64 total = (i64)b->n * b->k;
    hipLaunchKernelGGL(kb_flows0, dim3(grid_for(total)), dim3(kBlock), 0, b->stream, total, b->k, b->rowptr, b->a[0], b->f[0]);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(f_out, b->f[(b->round - 1) & 1], sizeof(double) * ek, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return FU_OK;
  FU_TRY_END
}

int fu_batch_get_round(fu_batch *b, int64_t *rounds_done) {
  if (!b || !rounds_done) return fail(FU_ERR_ARG, "fu_batch_get_round: bad arguments");
  *rounds_done = b->round;
  return FU_OK;
}

int fu_batch_synchronize(fu_batch *b) {
  if (!b) return fail(FU_ERR_ARG, "fu_batch_synchronize: bad arguments");
  if (int rc = set_device(b)) return rc;
  HIP_TRY(hipStreamSynchronize(b->stream));
  return FU_OK;
}

}  // extern "C"
