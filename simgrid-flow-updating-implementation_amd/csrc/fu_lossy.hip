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
//
// The handle scaffold (create and destroy, the run loops, the error slots and k_max_err, the
// small entry points) is csrc/fu_handle.h, shared with the batched and pairwise engines.
#include "fu_handle.h"

using namespace fu;

namespace {

constexpr int kBlock = 256;        // threads per block (4 waves of 64)
constexpr int kTileRows = kBlock;  // light tiles: at most one row per thread
constexpr int kTileEdges = 2048;   // light tiles: (F, E, lost) of the tile's slots in LDS (34 KB: 4 blocks per CU)
constexpr int kHeavyDeg = 128;     // rows above this degree run one block per row
constexpr int kChunk = 2048;       // heavy rows: (F, E) elements staged in LDS per chunk

using i64 = long long;

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
  if (!A.zero) block_count_to<kBlock>(cnt, A.lost);  // one atomic per block that lost something
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
  if (!A.zero) block_count_to<kBlock>(cnt, A.lost);
}

}  // namespace

struct fu_lossy : handle_base {
  static constexpr const char *kTag = "fu_lossy";
  double p = 0.0;
  uint64_t seed = 0;
  bool has_mask = false;
  int32_t n_tiles = 0, n_heavy = 0;
  i64 *rowptr = nullptr;
  int *col = nullptr, *rev = nullptr, *hrows = nullptr;
  int2 *tiles = nullptr;
  unsigned char *down = nullptr;
  double *v = nullptr, *a[2] = {nullptr, nullptr}, *f[2] = {nullptr, nullptr};
  u64 *lost = nullptr;
};

static int launch_err(fu_lossy *h, u64 *slot) {
  return launch_max_err<kBlock>(h, h->a[(h->round + 1) & 1], slot);  // a of the last round run
}

static int launch_round(fu_lossy *h) {
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

extern "C" {

int fu_lossy_destroy(fu_lossy *h) {
  if (!h) return bad_arguments<fu_lossy>("destroy");
  handle_close(h, {h->rowptr, h->col, h->rev, h->hrows, h->tiles, h->down, h->v, h->a[0], h->a[1], h->f[0], h->f[1], h->lost});
  delete h;
  return FU_OK;
}

// Every check on the arguments comes before the first HIP call, so a host without a GPU
// reports an asymmetric graph or a bad rev as such.
int fu_lossy_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                    const double *value, int32_t device, fu_lossy **out) {
  FU_TRY_BEGIN
  if (!out || !rowptr || !value || n <= 0 || e < 0 || (e > 0 && !col)) return bad_arguments<fu_lossy>("create");
  if (e > (int64_t)INT32_MAX) return fail(FU_ERR_ARG, "fu_lossy_create: more than 2^31-1 directed edges (rev is int32)");
  if (int rc = check_csr("fu_lossy_create", n, e, rowptr, col)) return rc;
  std::vector<int32_t> built;
  if (e > 0 && !rev) {
    if (int rc = rev_of_csr(n, e, rowptr, col, &built)) return rc;
    rev = built.data();
  }
  if (int rc = check_rev("fu_lossy_create", RevCheck::kPairing, n, rowptr, col, rev)) return rc;
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
  auto *h = new fu_lossy();
  h->n_tiles = (int32_t)tiles.size();
  h->n_heavy = (int32_t)heavy.size();
  auto cleanup = [&](int code) { fu_lossy_destroy(h); return code; };
  int rc = FU_OK;
  if ((rc = handle_open(h, device, n, e, 1))) return cleanup(rc);
  const int64_t e1 = std::max<int64_t>(e, 1);
  if ((rc = dmalloc(h, &h->rowptr, (int64_t)n + 1)) || (rc = dmalloc(h, &h->col, e)) || (rc = dmalloc(h, &h->rev, e)) ||
      (rc = dmalloc(h, &h->hrows, h->n_heavy)) || (rc = dmalloc(h, &h->tiles, h->n_tiles)) ||
      (rc = dmalloc(h, &h->down, e)) || (rc = dmalloc(h, &h->v, n)) || (rc = dmalloc(h, &h->a[0], n)) ||
      (rc = dmalloc(h, &h->a[1], n)) || (rc = dmalloc(h, &h->f[0], e1)) || (rc = dmalloc(h, &h->f[1], e1)) ||
      (rc = dmalloc(h, &h->lost, 1)))
    return cleanup(rc);
  static_assert(sizeof(i64) == sizeof(int64_t), "rowptr is uploaded as is");
  if ((rc = put(h, h->rowptr, rowptr, (int64_t)n + 1)) || (rc = put(h, h->col, col, e)) || (rc = put(h, h->rev, rev, e)) ||
      (rc = put(h, h->hrows, heavy.data(), h->n_heavy)) || (rc = put(h, h->tiles, tiles.data(), h->n_tiles)) ||
      (rc = put(h, h->v, value, n)))
    return cleanup(rc);
  if ((rc = zero(h, h->a[0], n)) || (rc = zero(h, h->a[1], n)) || (rc = zero(h, h->f[0], e1)) ||
      (rc = zero(h, h->f[1], e1)) || (rc = zero(h, h->lost, 1)))
    return cleanup(rc);
  *out = h;
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_create_from_graph(const fu_graph *g, const double *value, int32_t device, fu_lossy **out) {
  return create_from_graph<fu_lossy>(g, value, out, [&](auto... csr) { return fu_lossy_create(csr..., value, device, out); });
}

int fu_lossy_set_loss(fu_lossy *h, double p, uint64_t seed) {
  if (!h) return bad_arguments<fu_lossy>("set_loss");
  if (!(p >= 0.0 && p <= 1.0)) return fail(FU_ERR_ARG, "fu_lossy_set_loss: p must be in [0, 1]");
  h->p = p;  // kernel arguments of the rounds launched from now on
  h->seed = seed;
  return FU_OK;
}

int fu_lossy_set_link_mask(fu_lossy *h, const uint8_t *down) {
  if (!h) return bad_arguments<fu_lossy>("set_link_mask");
  if (!down || h->E == 0) {
    h->has_mask = false;  // rounds already queued keep their own argument copy; the buffer stays
    return FU_OK;
  }
  if (int rc = upload(h, h->down, down, (size_t)h->E)) return rc;
  h->has_mask = true;
  return FU_OK;
}

int fu_lossy_set_values(fu_lossy *h, const double *value) {
  if (!h || !value) return bad_arguments<fu_lossy>("set_values");
  return upload(h, h->v, value, sizeof(double) * (size_t)h->n);
}

// The flow and estimate buffers stay as they are: round 0 reads no state.
int fu_lossy_reset(fu_lossy *h) {
  if (!h) return bad_arguments<fu_lossy>("reset");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemsetAsync(h->lost, 0, sizeof(u64), h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->round = 0;
  return FU_OK;
}

int fu_lossy_set_targets(fu_lossy *h, const double *target) { return set_targets(h, target); }
int fu_lossy_run(fu_lossy *h, int32_t rounds, int32_t err_every, double *err_trace) { return run(h, rounds, err_every, err_trace); }
int fu_lossy_run_timed(fu_lossy *h, int32_t rounds, float *ms) { return run_timed(h, rounds, ms); }
int fu_lossy_max_err(fu_lossy *h, double *out) { return max_err(h, out, /*needs_a_round=*/true); }
int fu_lossy_get_round(fu_lossy *h, int64_t *rounds_done) { return get_round(h, rounds_done); }
int fu_lossy_synchronize(fu_lossy *h) { return synchronize(h); }

int fu_lossy_get_estimates(fu_lossy *h, double *a_out) {
  if (!h || !a_out) return bad_arguments<fu_lossy>("get_estimates");
  if (h->round == 0) {  // zero state
    std::fill(a_out, a_out + h->n, 0.0);
    return FU_OK;
  }
  return download(h, a_out, h->a[(h->round + 1) & 1], sizeof(double) * (size_t)h->n);
}

int fu_lossy_get_flows(fu_lossy *h, double *f_out) {
  if (!h || (!f_out && h->E)) return bad_arguments<fu_lossy>("get_flows");
  if (h->round == 0) {  // zero state
    std::fill(f_out, f_out + h->E, 0.0);
    return FU_OK;
  }
  return download(h, f_out, h->f[(h->round + 1) & 1], sizeof(double) * (size_t)h->E);
}

int fu_lossy_get_stats(fu_lossy *h, int64_t out[2]) {
  if (!h || !out) return bad_arguments<fu_lossy>("get_stats");
  u64 lost = 0;
  if (int rc = download(h, &lost, h->lost, sizeof(lost))) return rc;
  out[0] = h->round > 1 ? h->E * (h->round - 1) : 0;  // round 0 offers nothing
  out[1] = (int64_t)lost;
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
