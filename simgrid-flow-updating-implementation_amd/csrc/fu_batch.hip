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
//
// The handle scaffold (create and destroy, the run loops, the error slots, the small entry
// points) is csrc/fu_handle.h, shared with the lossy and pairwise engines.
#include "fu_handle.h"

using namespace fu;

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

struct fu_batch : handle_base {  // width = K
  static constexpr const char *kTag = "fu_batch";
  int32_t n_heavy = 0;
  i64 *rowptr = nullptr;
  int *col = nullptr, *hrows = nullptr;
  double *v = nullptr, *a[3] = {nullptr, nullptr, nullptr}, *f[2] = {nullptr, nullptr};
};

static int launch_err(fu_batch *b, u64 *slot) {
  const int K = b->width;
  const i64 total = (i64)b->n * K;
  const int tb = (kBlock / K) * K;
  const unsigned grid = (unsigned)std::min<i64>(1024, (total + tb - 1) / tb);
  hipLaunchKernelGGL(kb_max_err, dim3(grid), dim3(kBlock), 0, b->stream, total, K, b->a[(b->round + 2) % 3], b->target,
                     slot);  // a_{round-1}: the last round run
  HIP_TRY(hipGetLastError());
  return FU_OK;
}

static int launch_round(fu_batch *b) {
  const int64_t r = b->round;
  const int K = b->width;
  const i64 total = (i64)b->n * K;
  if (r == 0) {
    hipLaunchKernelGGL(kb_round0, dim3(grid_for(total)), dim3(kBlock), 0, b->stream, total, K, b->rowptr, b->v, b->a[0],
                       b->a[2]);
  } else {
    const int fm = r == 1 ? 1 : r == 2 ? 2 : 0;
    double *a1 = b->a[(r + 2) % 3], *a2 = b->a[(r + 1) % 3], *ao = b->a[r % 3], *F = b->f[r & 1];
    hipLaunchKernelGGL(kb_light, dim3(grid_for(total)), dim3(kBlock), 0, b->stream, total, K, fm, b->rowptr, b->col, b->v,
                       a1, a2, ao, F);
    if (b->n_heavy > 0)
      hipLaunchKernelGGL(kb_heavy, dim3(b->n_heavy), dim3(kBlock), 0, b->stream, K, fm, b->hrows, b->rowptr, b->col, b->v,
                         a1, a2, ao, F);
  }
  HIP_TRY(hipGetLastError());
  b->round = r + 1;
  return FU_OK;
}

extern "C" {

int fu_batch_destroy(fu_batch *b) {
  if (!b) return bad_arguments<fu_batch>("destroy");
  handle_close(b, {b->rowptr, b->col, b->hrows, b->v, b->a[0], b->a[1], b->a[2], b->f[0], b->f[1]});
  delete b;
  return FU_OK;
}

// Every check on the arguments comes before the first HIP call, so a host without a GPU
// reports a bad k or an asymmetric graph as such.
int fu_batch_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev, int32_t k,
                    const double *value, int32_t device, fu_batch **out) {
  FU_TRY_BEGIN
  if (!out || !rowptr || !value || n <= 0 || e < 0 || (e > 0 && !col)) return bad_arguments<fu_batch>("create");
  if (k < 1 || k > kMaxK) return fail(FU_ERR_ARG, "fu_batch_create: k must be in 1..16, got " + std::to_string(k));
  if (int rc = check_csr("fu_batch_create", n, e, rowptr, col)) return rc;
  // The flow reconstruction needs every i -> j to have its j -> i and nothing else of rev,
  // which never reaches the device: a caller's rev is checked for that alone.
  if (e > 0)
    if (int rc = rev ? check_rev("fu_batch_create", RevCheck::kSymmetric, n, rowptr, col, rev)
                     : rev_of_csr(n, e, rowptr, col, nullptr))
      return rc;
  std::vector<int32_t> heavy;
  for (int32_t i = 0; i < n; ++i)
    if (rowptr[i + 1] - rowptr[i] > kHeavyDeg) heavy.push_back(i);
  auto *b = new fu_batch();
  b->n_heavy = (int32_t)heavy.size();
  auto cleanup = [&](int code) { fu_batch_destroy(b); return code; };
  int rc = FU_OK;
  if ((rc = handle_open(b, device, n, e, k))) return cleanup(rc);
  const int64_t nk = (int64_t)n * k, ek = std::max<int64_t>(e * k, 1);
  if ((rc = dmalloc(b, &b->rowptr, (int64_t)n + 1)) || (rc = dmalloc(b, &b->col, e)) ||
      (rc = dmalloc(b, &b->hrows, b->n_heavy)) || (rc = dmalloc(b, &b->v, nk)) || (rc = dmalloc(b, &b->a[0], nk)) ||
      (rc = dmalloc(b, &b->a[1], nk)) || (rc = dmalloc(b, &b->a[2], nk)) || (rc = dmalloc(b, &b->f[0], ek)) ||
      (rc = dmalloc(b, &b->f[1], ek)))
    return cleanup(rc);
  static_assert(sizeof(i64) == sizeof(int64_t), "rowptr is uploaded as is");
  if ((rc = put(b, b->rowptr, rowptr, (int64_t)n + 1)) || (rc = put(b, b->col, col, e)) ||
      (rc = put(b, b->hrows, heavy.data(), b->n_heavy)) || (rc = put(b, b->v, value, nk)))
    return cleanup(rc);
  // without edges col is one element, and it is written too (the other engines leave theirs)
  if ((rc = zero(b, b->col, e == 0 ? 1 : 0)) || (rc = zero(b, b->a[0], nk)) || (rc = zero(b, b->a[1], nk)) ||
      (rc = zero(b, b->a[2], nk)) || (rc = zero(b, b->f[0], ek)) || (rc = zero(b, b->f[1], ek)))
    return cleanup(rc);
  *out = b;
  return FU_OK;
  FU_TRY_END
}

int fu_batch_create_from_graph(const fu_graph *g, int32_t k, const double *value, int32_t device, fu_batch **out) {
  FU_TRY_BEGIN
  if (g && value && out && (k < 1 || k > kMaxK))  // after the null checks, before the graph's
    return fail(FU_ERR_ARG, "fu_batch_create_from_graph: k must be in 1..16, got " + std::to_string(k));
  return create_from_graph<fu_batch>(g, value, out, [&](auto... csr) { return fu_batch_create(csr..., k, value, device, out); });
  FU_TRY_END
}

int fu_batch_reset(fu_batch *b) {
  if (!b) return bad_arguments<fu_batch>("reset");
  if (int rc = synchronize(b)) return rc;
  b->round = 0;  // round 0 rewrites a_0 and a_{-1}; rounds 1 and 2 write their flows without reading any
  return FU_OK;
}

int fu_batch_set_targets(fu_batch *b, const double *target) { return set_targets(b, target); }
int fu_batch_run(fu_batch *b, int32_t rounds, int32_t err_every, double *err_trace) { return run(b, rounds, err_every, err_trace); }
int fu_batch_run_timed(fu_batch *b, int32_t rounds, float *ms) { return run_timed(b, rounds, ms); }
int fu_batch_max_err(fu_batch *b, double *out) { return max_err(b, out, /*needs_a_round=*/true); }
int fu_batch_get_round(fu_batch *b, int64_t *rounds_done) { return get_round(b, rounds_done); }
int fu_batch_synchronize(fu_batch *b) { return synchronize(b); }

int fu_batch_get_estimates(fu_batch *b, double *a_out) {
  if (!b || !a_out) return bad_arguments<fu_batch>("get_estimates");
  const size_t nk = (size_t)b->n * b->width;
  if (b->round == 0) {  // zero state
    std::fill(a_out, a_out + nk, 0.0);
    return FU_OK;
  }
  return download(b, a_out, b->a[(b->round + 2) % 3], sizeof(double) * nk);
}

int fu_batch_get_flows(fu_batch *b, double *f_out) {
  FU_TRY_BEGIN
  if (!b || (!f_out && b->E)) return bad_arguments<fu_batch>("get_flows");
  if (b->E == 0) return FU_OK;
  const size_t ek = (size_t)b->E * b->width;
  if (b->round == 0) {  // zero state
    std::fill(f_out, f_out + ek, 0.0);
    return FU_OK;
  }
  if (b->round == 1) {  // round 0 wrote no flows: f_0 on demand (round 2 never reads it from memory)
    if (int rc = set_device(b)) return rc;
    const i64 total = (i64)b->n * b->width;
    hipLaunchKernelGGL(kb_flows0, dim3(grid_for(total)), dim3(kBlock), 0, b->stream, total, b->width, b->rowptr, b->a[0],
                       b->f[0]);
    HIP_TRY(hipGetLastError());
  }
  return download(b, f_out, b->f[(b->round - 1) & 1], sizeof(double) * ek);
  FU_TRY_END
}

}  // extern "C"
