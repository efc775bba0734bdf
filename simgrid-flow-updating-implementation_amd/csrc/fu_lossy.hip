// libfu lossy collect-all engine for MI355X (gfx950): generation-synchronous rounds in which
// a message can be lost. C ABI: the fu_lossy section of include/fu.h. DESIGN.md §4.16.
//
// Round r, slot k = (i -> j) of row i, j = col[k]:
//   delivered (message j -> i of round r-1 arrived):  F = -f_old[rev k],  E = a_old[j]   CA:98-99
//   lost (node i fires on what it stored itself):     F =  f_old[k],      E = a_old[i]   CA:118-119
//   S = 0.0 + F_b + ...,  T = 0.0 + E_b + ...   (left to right, row order)
//   a_new[i] = ((v[i] - S) + T) / (deg + 1),   f_new[k] = (F_k + a_new[i]) - E_k
// Round 0 is the timeout fire on zero state: every slot lost, f_old = a_old = 0.0.
//
// The scalar and batched engines rebuild f_old[rev k] from estimates. That is
// exact only while every message arrives: after one loss the two ends of a link no longer
// hold flows that are each other's negation, so here the reverse flow is gathered through a
// device copy of rev, and f and a are double-buffered (round r reads [(r + 1) & 1] and
// writes [r & 1]).
//
// Slot k of round r >= 1 is lost iff down[k] != 0 or u01(splitmix_at(splitmix_at(seed, r), k))
// < p, with k the caller's slot index: no mask memory, no dependence on the launch shape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
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

constexpr int kBlock = 256;        // threads per block (4 waves of 64)
constexpr int kTileRows = kBlock;  // light tiles: at most one row per thread
constexpr int kTileEdges = 2048;   // light tiles: (F, E, lost) of the tile's slots in LDS (34 KB: 4 blocks per CU)
constexpr int kHeavyDeg = 128;     // rows above this degree run one block per row
constexpr int kChunk = 2048;       // heavy rows: (F, E) elements staged in LDS per chunk

using i64 = long long;
using u64 = unsigned long long;

// The key of round r's decisions, and the decision itself: the kernels and
// fu_lossy_delivered share both. The compare is fp64 on both sides.
FU_HD inline uint64_t round_key(uint64_t seed, uint64_t r) { return splitmix_at(seed, r); }
FU_HD inline bool slot_lost(uint64_t key, uint64_t k, double p) { return u01(splitmix_at(key, k)) < p; }

struct RoundArgs {
  const i64 *rowptr;
  const int *col, *rev;
  const unsigned char *down;  // may be null
  const double *v, *f_old, *a_old;
  double *f_new, *a_new;
  u64 *lost;      // the handle's lost-message counter
  uint64_t key;   // round_key(seed, r)
  double p;
  int zero;       // round 0: zero state, every slot "lost", nothing counted
};

// Slot k's operands. Returns true if the message was lost: F is then the node's own flow and
// E is the row owner's own estimate, which the caller supplies.
__device__ inline bool fetch(const RoundArgs &A, i64 k, double &F, double &E) {
  if (A.zero) {
    F = 0.0;
    E = 0.0;
    return true;
  }
  bool lost = A.down != nullptr && A.down[k] != 0;
  if (!lost && A.p > 0.0) lost = slot_lost(A.key, (uint64_t)k, A.p);
  if (lost) {
    F = A.f_old[k];
    E = 0.0;
  } else {
    F = -A.f_old[A.rev[k]];
    E = A.a_old[A.col[k]];
  }
  return lost;
}

// One atomic per block that lost something.
__device__ inline void block_count_to(int cnt, u64 *dst) {
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  __shared__ int s_w[kBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_w[w] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int q = 0; q < kBlock / 64; ++q) t += s_w[q];
    if (t) atomicAdd(dst, (u64)t);
  }
}

// Light tiles: consecutive rows of degree <= kHeavyDeg, at most kTileRows rows and
// kTileEdges slots. All threads load the tile's slots coalesced (col, rev, down, the own flow
// of a lost slot) and leave the gathered (F, E) in LDS; thread t then runs row t's two
// chains from LDS in row order and leaves the new flows there; all threads write them out
// coalesced.
__global__ __launch_bounds__(kBlock) void kl_light(RoundArgs A, const int2 *__restrict__ tiles) {
  __shared__ double s_F[kTileEdges], s_E[kTileEdges];
  __shared__ unsigned char s_lost[kTileEdges];
  const int tid = threadIdx.x;
  const int2 tile = tiles[blockIdx.x];
  const i64 e0 = A.rowptr[tile.x];
  const int ne = (int)(A.rowptr[tile.y] - e0);  // <= kTileEdges (the host's tile plan)
  int cnt = 0;
  if (A.zero) {
    for (int q = tid; q < ne; q += kBlock) {
      s_F[q] = 0.0;
      s_E[q] = 0.0;
      s_lost[q] = 1;
    }
  } else if (ne > 0) {
    // Branch-free: a thread's kSlots slots (indices past the tile's end clamped to its last
    // slot, their results dropped) issue all their loads before the first use, so the two
    // gathers of every slot are in flight together. A lost slot reads its own flow through
    // the same load (index k instead of rev k) and gathers no estimate.
    constexpr int kSlots = kTileEdges / kBlock;
    i64 k[kSlots];
    int c[kSlots], rv[kSlots];
    bool lost[kSlots];
    double F[kSlots], E[kSlots];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int q = tid + u * kBlock;
      k[u] = e0 + (q < ne ? q : ne - 1);
      c[u] = A.col[k[u]];
      rv[u] = A.rev[k[u]];
      lost[u] = false;
    }
    if (A.down != nullptr) {
#pragma unroll
      for (int u = 0; u < kSlots; ++u) lost[u] = A.down[k[u]] != 0;
    }
    if (A.p > 0.0) {
#pragma unroll
      for (int u = 0; u < kSlots; ++u) lost[u] = lost[u] || slot_lost(A.key, (uint64_t)k[u], A.p);
    }
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      F[u] = A.f_old[lost[u] ? k[u] : (i64)rv[u]];
      E[u] = lost[u] ? 0.0 : A.a_old[c[u]];
    }
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int q = tid + u * kBlock;
      if (q < ne) {
        s_F[q] = lost[u] ? F[u] : -F[u];
        s_E[q] = E[u];
        s_lost[q] = lost[u];
        cnt += lost[u];
      }
    }
  }
  __syncthreads();
  const int row = tile.x + tid;
  if (row < tile.y) {
    const int b = (int)(A.rowptr[row] - e0);
    const int d = (int)(A.rowptr[row + 1] - e0) - b;
    const double own = A.zero ? 0.0 : A.a_old[row];
    double S = 0.0, T = 0.0;
    for (int j = b; j < b + d; ++j) {
      S = S + s_F[j];
      T = T + (s_lost[j] ? own : s_E[j]);
    }
    const double a = ((A.v[row] - S) + T) / (double)(d + 1);
    A.a_new[row] = a;
    for (int j = b; j < b + d; ++j) s_F[j] = (s_F[j] + a) - (s_lost[j] ? own : s_E[j]);
  }
  __syncthreads();
  for (int q = tid; q < ne; q += kBlock) A.f_new[e0 + q] = s_F[q];
  if (!A.zero) block_count_to(cnt, A.lost);
}

// Rows above kHeavyDeg: one block per row. All threads load a chunk of slots coalesced and
// leave (F, E) in LDS; lane 0 of wave 0 carries S and lane 0 of wave 1 carries T through the
// chunk in row order, from chunk to chunk. Once a is known, a second pass fetches the
// operands again (f_old and a_old are not written in this round) and writes the flows
// coalesced.
__global__ __launch_bounds__(kBlock) void kl_heavy(RoundArgs A, const int *__restrict__ hrows) {
  __shared__ double s_F[kChunk], s_E[kChunk];
  __shared__ double s_T, s_a;
  const int tid = threadIdx.x;
  const int row = hrows[blockIdx.x];
  const i64 b = A.rowptr[row];
  const i64 d = A.rowptr[row + 1] - b;
  const double own = A.zero ? 0.0 : A.a_old[row];
  double acc = 0.0;  // S in thread 0, T in thread 64
  int cnt = 0;
  for (i64 c0 = 0; c0 < d; c0 += kChunk) {
    const int m = (int)(d - c0 < kChunk ? d - c0 : kChunk);
#pragma unroll 4
    for (int q = tid; q < m; q += kBlock) {
      double F, E;
      const bool lost = fetch(A, b + c0 + q, F, E);
      s_F[q] = F;
      s_E[q] = lost ? own : E;
      cnt += lost;
    }
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < m; ++q) acc = acc + s_F[q];
    else if (tid == 64)
      for (int q = 0; q < m; ++q) acc = acc + s_E[q];
    __syncthreads();
  }
  if (tid == 64) s_T = acc;
  __syncthreads();
  if (tid == 0) {
    const double a = ((A.v[row] - acc) + s_T) / (double)(d + 1);
    A.a_new[row] = a;
    s_a = a;
  }
  __syncthreads();
  const double a = s_a;
  for (i64 q = tid; q < d; q += kBlock) {
    double F, E;
    const bool lost = fetch(A, b + q, F, E);
    A.f_new[b + q] = (F + a) - (lost ? own : E);
  }
  if (!A.zero) block_count_to(cnt, A.lost);
}

// max_i |a_i - target_i| as a uint64 bit pattern, the rule of the scalar engine's k_max_err:
// non-negative doubles order like their bits, and a NaN with its sign cleared is above +inf,
// so one NaN makes the result NaN.
__global__ __launch_bounds__(kBlock) void kl_max_err(int n, const double *__restrict__ a,
                                                     const double *__restrict__ target, u64 *__restrict__ err) {
  u64 m = 0;
  for (i64 i = (i64)blockIdx.x * kBlock + threadIdx.x; i < n; i += (i64)gridDim.x * kBlock) {
    const u64 x = (u64)__double_as_longlong(fabs(a[i] - target[i]));
    m = x > m ? x : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const u64 y = __shfl_xor(m, off, 64);
    m = m > y ? m : y;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(err, m);
}

}  // namespace

struct fu_lossy {
  int device = 0;
  int32_t n = 0;
  int64_t E = 0;
  int64_t round = 0;
  double p = 0.0;
  uint64_t seed = 0;
  bool has_target = false, has_mask = false;
  int32_t n_tiles = 0, n_heavy = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  i64 *rowptr = nullptr;
  int *col = nullptr, *rev = nullptr, *hrows = nullptr;
  int2 *tiles = nullptr;
  unsigned char *down = nullptr;
  double *v = nullptr, *target = nullptr, *a[2] = {nullptr, nullptr}, *f[2] = {nullptr, nullptr};
  u64 *lost = nullptr;
  u64 *err = nullptr;
  int64_t errcap = 0;
};

namespace {

template <typename T>
int dmalloc(T **p, int64_t count) {
  if (hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * (size_t)std::max<int64_t>(count, 1)) != hipSuccess) {
    *p = nullptr;
    return fail(FU_ERR_ALLOC, "fu_lossy: hipMalloc failed");
  }
  return FU_OK;
}

int set_device(fu_lossy *h) {
  HIP_TRY(hipSetDevice(h->device));
  return FU_OK;
}

int err_slots(fu_lossy *h, int64_t count) {
  if (count <= h->errcap) return FU_OK;
  if (h->err) hipFree(h->err);
  h->err = nullptr;
  h->errcap = 0;
  if (int rc = dmalloc(&h->err, count)) return rc;
  h->errcap = count;
  return FU_OK;
}

int launch_err(fu_lossy *h, u64 *slot) {
  const unsigned grid = (unsigned)std::min<i64>(1024, ((i64)h->n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(kl_max_err, dim3(grid), dim3(kBlock), 0, h->stream, h->n, h->a[(h->round + 1) & 1], h->target,
                     slot);  // a of the last round run
  HIP_TRY(hipGetLastError());
  return FU_OK;
}

int launch_round(fu_lossy *h) {
  const int64_t r = h->round;
  RoundArgs A;
  A.rowptr = h->rowptr;
  A.col = h->col;
  A.rev = h->rev;
  A.down = h->has_mask ? h->down : nullptr;
  A.v = h->v;
  A.f_old = h->f[(r + 1) & 1];
  A.a_old = h->a[(r + 1) & 1];
  A.f_new = h->f[r & 1];
  A.a_new = h->a[r & 1];
  A.lost = h->lost;
  A.key = round_key(h->seed, (uint64_t)r);
  A.p = h->p;
  A.zero = r == 0;
  if (h->n_tiles > 0) hipLaunchKernelGGL(kl_light, dim3(h->n_tiles), dim3(kBlock), 0, h->stream, A, h->tiles);
  if (h->n_heavy > 0) hipLaunchKernelGGL(kl_heavy, dim3(h->n_heavy), dim3(kBlock), 0, h->stream, A, h->hrows);
  HIP_TRY(hipGetLastError());
  h->round = r + 1;
  return FU_OK;
}

// rev must pair every slot with its reverse slot: in range, an involution, and pointing into
// the row of the slot's neighbour at a slot that points back. A rev that fails this would be an
// out-of-bounds or wrong gather on the device.
int check_rev(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev) {
  for (int32_t i = 0; i < n; ++i)
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int64_t r = rev[k];
      if (r < 0 || r >= e || rev[r] != k || col[r] != i || r < rowptr[col[k]] || r >= rowptr[col[k] + 1])
        return fail(FU_ERR_GRAPH, "fu_lossy_create: rev is not the reverse-edge pairing (the graph must be symmetric) at edge " +
                                      std::to_string(k));
    }
  return FU_OK;
}

}  // namespace

extern "C" {

int fu_lossy_destroy(fu_lossy *h) {
  if (!h) return fail(FU_ERR_ARG, "fu_lossy_destroy: bad arguments");
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void *p : {(void *)h->rowptr, (void *)h->col, (void *)h->rev, (void *)h->hrows, (void *)h->tiles, (void *)h->down,
                  (void *)h->v, (void *)h->target, (void *)h->a[0], (void *)h->a[1], (void *)h->f[0], (void *)h->f[1],
                  (void *)h->lost, (void *)h->err})
    if (p) (void)hipFree(p);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return FU_OK;
}

// Every check on the arguments comes before the first HIP call, so a host without a GPU
// reports an asymmetric graph or a bad rev as such.
int fu_lossy_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                    const double *value, int32_t device, fu_lossy **out) {
  FU_TRY_BEGIN
  if (!out || !rowptr || !value || n <= 0 || e < 0 || (e > 0 && !col)) return fail(FU_ERR_ARG, "fu_lossy_create: bad arguments");
  if (e > (int64_t)INT32_MAX) return fail(FU_ERR_ARG, "fu_lossy_create: more than 2^31-1 directed edges (rev is int32)");
  if (rowptr[0] != 0 || rowptr[n] != e) return fail(FU_ERR_ARG, "fu_lossy_create: rowptr[0] must be 0 and rowptr[n] == e");
  for (int32_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(FU_ERR_ARG, "fu_lossy_create: rowptr not monotone");
  for (int64_t q = 0; q < e; ++q)
    if (col[q] < 0 || col[q] >= n) return fail(FU_ERR_ARG, "fu_lossy_create: col index out of range at edge " + std::to_string(q));
  std::vector<int32_t> built;
  if (e > 0 && !rev) {
    fu_graph g;
    g.n = n;
    g.rowptr.assign(rowptr, rowptr + n + 1);
    g.col.assign(col, col + e);
    if (int rc = fu::build_rev(g)) return rc;
    built.swap(g.rev);
    rev = built.data();
  }
  if (e > 0)
    if (int rc = check_rev(n, e, rowptr, col, rev)) return rc;
  // the launch plan: heavy rows one block each; the rows between them in tiles of at most
  // kTileRows rows and kTileEdges slots
  std::vector<int32_t> heavy;
  std::vector<int2> tiles;
  for (int32_t i = 0; i < n;) {
    if (rowptr[i + 1] - rowptr[i] > kHeavyDeg) {
      heavy.push_back(i++);
      continue;
    }
    int32_t j = i;
    while (j < n && j - i < kTileRows && rowptr[j + 1] - rowptr[j] <= kHeavyDeg && rowptr[j + 1] - rowptr[i] <= kTileEdges) ++j;
    tiles.push_back(make_int2(i, j));  // j > i: a light row alone always fits
    i = j;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FU_ERR_HIP, "fu_lossy_create: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(FU_ERR_ARG, "fu_lossy_create: device out of range");
  auto *h = new fu_lossy();
  h->device = device;
  h->n = n;
  h->E = e;
  h->n_tiles = (int32_t)tiles.size();
  h->n_heavy = (int32_t)heavy.size();
  auto cleanup = [&](int code) { fu_lossy_destroy(h); return code; };
  int rc = FU_OK;
  if ((rc = set_device(h))) return cleanup(rc);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_lossy_create: hipStreamCreate failed"));
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_lossy_create: hipEventCreate failed"));
  if ((rc = dmalloc(&h->rowptr, (int64_t)n + 1)) || (rc = dmalloc(&h->col, e)) || (rc = dmalloc(&h->rev, e)) ||
      (rc = dmalloc(&h->hrows, h->n_heavy)) || (rc = dmalloc(&h->tiles, h->n_tiles)) || (rc = dmalloc(&h->down, e)) ||
      (rc = dmalloc(&h->v, n)) || (rc = dmalloc(&h->target, n)) || (rc = dmalloc(&h->a[0], n)) ||
      (rc = dmalloc(&h->a[1], n)) || (rc = dmalloc(&h->f[0], e)) || (rc = dmalloc(&h->f[1], e)) ||
      (rc = dmalloc(&h->lost, 1)) || (rc = err_slots(h, 1)))
    return cleanup(rc);
  static_assert(sizeof(i64) == sizeof(int64_t), "rowptr is uploaded as is");
  if (hipMemcpy(h->rowptr, rowptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice) != hipSuccess ||
      (e && hipMemcpy(h->col, col, sizeof(int32_t) * (size_t)e, hipMemcpyHostToDevice) != hipSuccess) ||
      (e && hipMemcpy(h->rev, rev, sizeof(int32_t) * (size_t)e, hipMemcpyHostToDevice) != hipSuccess) ||
      (h->n_heavy && hipMemcpy(h->hrows, heavy.data(), sizeof(int32_t) * heavy.size(), hipMemcpyHostToDevice) != hipSuccess) ||
      (h->n_tiles && hipMemcpy(h->tiles, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(h->v, value, sizeof(double) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_lossy_create: upload failed"));
  if (hipMemset(h->a[0], 0, sizeof(double) * (size_t)n) != hipSuccess ||
      hipMemset(h->a[1], 0, sizeof(double) * (size_t)n) != hipSuccess ||
      hipMemset(h->f[0], 0, sizeof(double) * (size_t)std::max<int64_t>(e, 1)) != hipSuccess ||
      hipMemset(h->f[1], 0, sizeof(double) * (size_t)std::max<int64_t>(e, 1)) != hipSuccess ||
      hipMemset(h->lost, 0, sizeof(u64)) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_lossy_create: memset failed"));
  *out = h;
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_create_from_graph(const fu_graph *g, const double *value, int32_t device, fu_lossy **out) {
  FU_TRY_BEGIN
  if (!g || !value || !out) return fail(FU_ERR_ARG, "fu_lossy_create_from_graph: bad arguments");
  const int64_t E = g->rowptr[g->n];
  if ((int64_t)g->rev.size() != E) return fail(FU_ERR_GRAPH, "fu_lossy_create_from_graph: graph is not symmetric");
  return fu_lossy_create(g->n, E, g->rowptr.data(), g->col.data(), E ? g->rev.data() : nullptr, value, device, out);
  FU_TRY_END
}

int fu_lossy_set_loss(fu_lossy *h, double p, uint64_t seed) {
  if (!h) return fail(FU_ERR_ARG, "fu_lossy_set_loss: bad arguments");
  if (!(p >= 0.0 && p <= 1.0)) return fail(FU_ERR_ARG, "fu_lossy_set_loss: p must be in [0, 1]");
  h->p = p;  // kernel arguments of the rounds launched from now on
  h->seed = seed;
  return FU_OK;
}

int fu_lossy_set_link_mask(fu_lossy *h, const uint8_t *down) {
  FU_TRY_BEGIN
  if (!h) return fail(FU_ERR_ARG, "fu_lossy_set_link_mask: bad arguments");
  if (!down || h->E == 0) {
    h->has_mask = false;  // rounds already queued keep their own argument copy; the buffer stays
    return FU_OK;
  }
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemcpyAsync(h->down, down, (size_t)h->E, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->has_mask = true;
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_set_values(fu_lossy *h, const double *value) {
  FU_TRY_BEGIN
  if (!h || !value) return fail(FU_ERR_ARG, "fu_lossy_set_values: bad arguments");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemcpyAsync(h->v, value, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_reset(fu_lossy *h) {
  if (!h) return fail(FU_ERR_ARG, "fu_lossy_reset: bad arguments");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemsetAsync(h->lost, 0, sizeof(u64), h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->round = 0;  // round 0 reads no state
  return FU_OK;
}

int fu_lossy_set_targets(fu_lossy *h, const double *target) {
  FU_TRY_BEGIN
  if (!h || !target) return fail(FU_ERR_ARG, "fu_lossy_set_targets: bad arguments");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemcpyAsync(h->target, target, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->has_target = true;
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_run(fu_lossy *h, int32_t rounds, int32_t err_every, double *err_trace) {
  FU_TRY_BEGIN
  if (!h || rounds < 0) return fail(FU_ERR_ARG, "fu_lossy_run: bad arguments");
  if (err_every > 0 && !h->has_target) return fail(FU_ERR_STATE, "fu_lossy_run: err_every > 0 needs fu_lossy_set_targets");
  if (int rc = set_device(h)) return rc;
  const int64_t nerr = err_every > 0 ? rounds / err_every : 0;
  if (nerr > 0) {
    if (int rc = err_slots(h, nerr)) return rc;
    HIP_TRY(hipMemsetAsync(h->err, 0, sizeof(u64) * (size_t)nerr, h->stream));
  }
  for (int32_t r = 0; r < rounds; ++r) {
    if (int rc = launch_round(h)) return rc;
    if (nerr > 0 && (r + 1) % err_every == 0)
      if (int rc = launch_err(h, h->err + ((r + 1) / err_every - 1))) return rc;
  }
  if (nerr > 0) {
    std::vector<u64> bits((size_t)nerr);
    HIP_TRY(hipMemcpyAsync(bits.data(), h->err, sizeof(u64) * bits.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (err_trace) std::memcpy(err_trace, bits.data(), sizeof(double) * bits.size());
  }
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_run_timed(fu_lossy *h, int32_t rounds, float *ms) {
  FU_TRY_BEGIN
  if (!h || !ms || rounds < 0) return fail(FU_ERR_ARG, "fu_lossy_run_timed: bad arguments");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  for (int32_t r = 0; r < rounds; ++r)
    if (int rc = launch_round(h)) return rc;
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev1));
  HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_max_err(fu_lossy *h, double *out) {
  FU_TRY_BEGIN
  if (!h || !out) return fail(FU_ERR_ARG, "fu_lossy_max_err: bad arguments");
  if (!h->has_target) return fail(FU_ERR_STATE, "fu_lossy_max_err: call fu_lossy_set_targets first");
  if (h->round == 0) return fail(FU_ERR_STATE, "fu_lossy_max_err: no round has run");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemsetAsync(h->err, 0, sizeof(u64), h->stream));
  if (int rc = launch_err(h, h->err)) return rc;
  u64 bits = 0;
  HIP_TRY(hipMemcpyAsync(&bits, h->err, sizeof(bits), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::memcpy(out, &bits, sizeof(double));
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_get_estimates(fu_lossy *h, double *a_out) {
  FU_TRY_BEGIN
  if (!h || !a_out) return fail(FU_ERR_ARG, "fu_lossy_get_estimates: bad arguments");
  if (h->round == 0) {  // zero state
    std::fill(a_out, a_out + h->n, 0.0);
    return FU_OK;
  }
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemcpyAsync(a_out, h->a[(h->round + 1) & 1], sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_get_flows(fu_lossy *h, double *f_out) {
  FU_TRY_BEGIN
  if (!h || (!f_out && h->E)) return fail(FU_ERR_ARG, "fu_lossy_get_flows: bad arguments");
  if (h->E == 0) return FU_OK;
  if (h->round == 0) {  // zero state
    std::fill(f_out, f_out + h->E, 0.0);
    return FU_OK;
  }
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemcpyAsync(f_out, h->f[(h->round + 1) & 1], sizeof(double) * (size_t)h->E, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_get_round(fu_lossy *h, int64_t *rounds_done) {
  if (!h || !rounds_done) return fail(FU_ERR_ARG, "fu_lossy_get_round: bad arguments");
  *rounds_done = h->round;
  return FU_OK;
}

int fu_lossy_get_stats(fu_lossy *h, int64_t out[2]) {
  FU_TRY_BEGIN
  if (!h || !out) return fail(FU_ERR_ARG, "fu_lossy_get_stats: bad arguments");
  if (int rc = set_device(h)) return rc;
  u64 lost = 0;
  HIP_TRY(hipMemcpyAsync(&lost, h->lost, sizeof(lost), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  out[0] = h->round > 1 ? h->E * (h->round - 1) : 0;  // round 0 offers nothing
  out[1] = (int64_t)lost;
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_synchronize(fu_lossy *h) {
  if (!h) return fail(FU_ERR_ARG, "fu_lossy_synchronize: bad arguments");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
}

int fu_lossy_delivered(uint64_t seed, int64_t round, int64_t first, int64_t count, double p, uint8_t *out) {
  if (round < 0 || first < 0 || count < 0 || (count > 0 && !out) || !(p >= 0.0 && p <= 1.0))
    return fail(FU_ERR_ARG, "fu_lossy_delivered: bad arguments");
  const uint64_t key = round_key(seed, (uint64_t)round);
  for (int64_t q = 0; q < count; ++q)
    out[q] = round == 0 ? 0 : (p > 0.0 && slot_lost(key, (uint64_t)(first + q), p)) ? 0 : 1;
  return FU_OK;
}

}  // extern "C"
