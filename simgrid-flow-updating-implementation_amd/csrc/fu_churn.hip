// libfu churn collect-all engine for MI355X (gfx950): generation-synchronous rounds over a
// fixed CSR whose nodes and links are switched off and on between runs. C ABI: the fu_churn
// section of include/fu.h. DESIGN.md §4.18.
//
// Slot k = (i -> j) of row i, j = col[k], carries one state byte: UP, DOWN or FRESH. It is
// live iff link_up[k] && alive[i] && alive[j]. fu_churn_set_topology moves it
//   live -> not live: DOWN (both ends drop the neighbour; its flow entry is gone),
//   not live -> live: FRESH (the neighbour was just added; nothing received from it, CA:33-34),
//   live -> live:     as it was.
// Round r, alive node i, the slots of row i in row order, the DOWN ones skipped:
//   UP:    F = -f_old[rev k],  E = a_old[j]                                   CA:98-99
//   FRESH: F = 0.0,            E = 0.0                                        CA:33-34
//   S = 0.0 + F..,  T = 0.0 + E..  (left to right),  d = the number of live slots
//   a_new[i] = ((v[i] - S) + T) / (d + 1),  f_new[k] = (F + a_new[i]) - E,  DOWN: f_new[k] = +0.0
// and every FRESH slot is UP afterwards. A dead node does not fire: a_new[i] = a_old[i]. After
// create and after reset every live slot is FRESH and all state is zero, so round 0 is this
// rule and nothing else.
//
// A skipped slot adds +0.0 to both chains instead of branching out of them. That is bit-exact:
// S and T start from +0.0, and x + y is -0.0 only where x and y both are, so neither chain can
// ever hold -0.0, and x + (+0.0) returns every other x as it is (a NaN stays a NaN).
//
// The reverse flow is gathered through a device copy of rev: the flow reconstruction of the
// scalar engine needs the two ends of a link to hold flows that negate each other, which a
// FRESH slot breaks as a lost message does. f and a are double-buffered (round r reads
// [(r + 1) & 1] and writes [r & 1]).
//
// The state byte of slot k is read and written by the block that runs row i and by no other
// (the reverse slot has its own byte, which its own row turns), so the FRESH -> UP write goes
// with the flow write: no race, no extra pass.
//
// The handle scaffold is csrc/fu_handle.h; the error check over alive nodes is this file's own.
#include "fu_handle.h"

using namespace fu;

namespace {

constexpr int kBlock = 256;        // threads per block (4 waves of 64)
constexpr int kTileRows = kBlock;  // light tiles: at most one row per thread
constexpr int kTileEdges = 2048;   // light tiles: (F, E, state) of the tile's slots in LDS (34 KB: 4 blocks per CU)
constexpr int kHeavyDeg = 128;     // rows above this degree run one block per row
constexpr int kChunk = 2048;       // heavy rows: (F, E) elements staged in LDS per chunk

constexpr unsigned char kUp = 0, kDown = 1, kFresh = 2;

using i64 = long long;

struct RoundArgs {
  const i64 *rowptr;
  const int *col, *rev;
  const unsigned char *alive;
  unsigned char *state;
  const double *v, *f_old, *a_old;
  double *f_new, *a_new;
};

// Light tiles: consecutive rows of degree <= kHeavyDeg, at most kTileRows rows and kTileEdges
// slots. All threads load the tile's slots coalesced (col, rev, state) and leave the gathered
// (F, E) in LDS; thread t then runs row t's two chains from LDS in row order and leaves the
// new flows there; all threads write them out coalesced and turn the FRESH bytes to UP.
__global__ __launch_bounds__(kBlock) void kc_light(RoundArgs A, const int2 *__restrict__ tiles) {
  __shared__ double s_F[kTileEdges], s_E[kTileEdges];
  __shared__ unsigned char s_st[kTileEdges];
  const int tid = threadIdx.x;
  const int2 tile = tiles[blockIdx.x];
  const i64 e0 = A.rowptr[tile.x];
  const int ne = (int)(A.rowptr[tile.y] - e0);  // <= kTileEdges (the host's tile plan)
  if (ne > 0) {
    // Branch-free: a thread's kSlots slots (indices past the tile's end clamped to its last
    // slot, their results dropped) issue all their loads before the first use. A slot that is
    // not UP gathers nothing: its flow load reads its own slot (index k instead of rev k, the
    // value dropped) and its estimate load is masked off.
    constexpr int kSlots = kTileEdges / kBlock;
    i64 k[kSlots];
    int c[kSlots], rv[kSlots];
    unsigned char st[kSlots];
    double F[kSlots], E[kSlots];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int q = tid + u * kBlock;
      k[u] = e0 + (q < ne ? q : ne - 1);
      c[u] = A.col[k[u]];
      rv[u] = A.rev[k[u]];
      st[u] = A.state[k[u]];
    }
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      F[u] = A.f_old[st[u] == kUp ? (i64)rv[u] : k[u]];
      E[u] = st[u] == kUp ? A.a_old[c[u]] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int q = tid + u * kBlock;
      if (q < ne) {
        s_F[q] = st[u] == kUp ? -F[u] : 0.0;
        s_E[q] = E[u];
        s_st[q] = st[u];
      }
    }
  }
  __syncthreads();
  const int row = tile.x + tid;
  if (row < tile.y) {
    const int b = (int)(A.rowptr[row] - e0);
    const int d = (int)(A.rowptr[row + 1] - e0) - b;
    double S = 0.0, T = 0.0;
    int live = 0;
    for (int j = b; j < b + d; ++j) {
      S = S + s_F[j];  // a DOWN slot adds +0.0 (the argument at the top of the file)
      T = T + s_E[j];
      live += s_st[j] != kDown;
    }
    // a dead row's slots are all DOWN: its flows come out as +0.0 below
    const double a = A.alive[row] ? ((A.v[row] - S) + T) / (double)(live + 1) : A.a_old[row];
    A.a_new[row] = a;
    for (int j = b; j < b + d; ++j) s_F[j] = s_st[j] != kDown ? (s_F[j] + a) - s_E[j] : 0.0;
  }
  __syncthreads();
  for (int q = tid; q < ne; q += kBlock) {
    A.f_new[e0 + q] = s_F[q];
    if (s_st[q] == kFresh) A.state[e0 + q] = kUp;
  }
}

// Slot k's operands and state, for the heavy rows.
__device__ inline unsigned char fetch(const RoundArgs &A, i64 k, double &F, double &E) {
  const unsigned char st = A.state[k];
  if (st == kUp) {
    F = -A.f_old[A.rev[k]];
    E = A.a_old[A.col[k]];
  } else {
    F = 0.0;
    E = 0.0;
  }
  return st;
}

// Rows above kHeavyDeg: one block per row. All threads load a chunk of slots coalesced and
// leave (F, E) in LDS; lane 0 of wave 0 carries S and lane 0 of wave 1 carries T through the
// chunk in row order, from chunk to chunk, and every thread counts the live slots it loaded,
// over all chunks. Once the block's count and a are known, a second pass fetches the operands
// again (f_old, a_old and the state bytes are not written before it), writes the flows
// coalesced and turns the FRESH bytes to UP.
__global__ __launch_bounds__(kBlock) void kc_heavy(RoundArgs A, const int *__restrict__ hrows) {
  __shared__ double s_F[kChunk], s_E[kChunk];
  __shared__ double s_T, s_a;
  __shared__ int s_live[kBlock / 64];
  const int tid = threadIdx.x;
  const int row = hrows[blockIdx.x];
  const i64 b = A.rowptr[row];
  const i64 d = A.rowptr[row + 1] - b;
  double acc = 0.0;  // S in thread 0, T in thread 64
  int live = 0;
  for (i64 c0 = 0; c0 < d; c0 += kChunk) {
    const int m = (int)(d - c0 < kChunk ? d - c0 : kChunk);
#pragma unroll 4
    for (int q = tid; q < m; q += kBlock) {
      double F, E;
      live += fetch(A, b + c0 + q, F, E) != kDown;
      s_F[q] = F;
      s_E[q] = E;
    }
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < m; ++q) acc = acc + s_F[q];
    else if (tid == 64)
      for (int q = 0; q < m; ++q) acc = acc + s_E[q];
    __syncthreads();
  }
  for (int off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off, 64);
  if ((tid & 63) == 0) s_live[tid >> 6] = live;
  if (tid == 64) s_T = acc;
  __syncthreads();
  if (tid == 0) {
    int dl = 0;
    for (int q = 0; q < kBlock / 64; ++q) dl += s_live[q];
    const double a = A.alive[row] ? ((A.v[row] - acc) + s_T) / (double)(dl + 1) : A.a_old[row];
    A.a_new[row] = a;
    s_a = a;
  }
  __syncthreads();
  const double a = s_a;
  for (i64 q = tid; q < d; q += kBlock) {
    double F, E;
    const unsigned char st = fetch(A, b + q, F, E);
    A.f_new[b + q] = st != kDown ? (F + a) - E : 0.0;
    if (st == kFresh) A.state[b + q] = kUp;
  }
}

// fu_churn_set_topology and fu_churn_reset: one pass over the slots, from the uploaded alive
// and link_up and the old state byte to the new one. Slot k's row is col[rev k]. A slot that is
// not live loses its flow entry in `f`, the buffer the next round reads. all_fresh (reset):
// every live slot ends FRESH. count[0] += alive nodes, count[1] += live slots, one atomic per
// block and counter.
__global__ __launch_bounds__(kBlock) void kc_topology(int n, i64 E, const int *__restrict__ col, const int *__restrict__ rev,
                                                      const unsigned char *__restrict__ alive,
                                                      const unsigned char *__restrict__ link_up, unsigned char *__restrict__ state,
                                                      double *__restrict__ f, int all_fresh, u64 *__restrict__ count) {
  const i64 k = (i64)blockIdx.x * kBlock + threadIdx.x;
  int live = 0;
  if (k < E) {
    live = link_up[k] != 0 && alive[col[rev[k]]] != 0 && alive[col[k]] != 0;
    if (live) {
      if (all_fresh || state[k] == kDown) state[k] = kFresh;
    } else {
      state[k] = kDown;
      f[k] = 0.0;
    }
  }
  int up = k < n && alive[k] != 0;
  block_count_to<kBlock>(up, count);
  __syncthreads();  // block_count_to's wave sums are one LDS array: the first call has read it
  block_count_to<kBlock>(live, count + 1);
}

// k_max_err of the scaffold over the alive nodes only: a dead node's frozen estimate never
// enters the maximum, and with no node alive the slot keeps its +0.0.
__global__ __launch_bounds__(kBlock) void kc_max_err(int n, const double *__restrict__ a, const double *__restrict__ target,
                                                     const unsigned char *__restrict__ alive, u64 *__restrict__ err) {
  u64 m = 0;
  for (i64 i = (i64)blockIdx.x * kBlock + threadIdx.x; i < n; i += (i64)gridDim.x * kBlock) {
    if (!alive[i]) continue;
    const u64 x = (u64)__double_as_longlong(fabs(a[i] - target[i]));
    m = x > m ? x : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const u64 y = __shfl_xor(m, off, 64);
    m = m > y ? m : y;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(err, m);
}

// A link is up or down as a whole: FU_ERR_ARG where link_up (may be null: all ones) differs
// between a slot and its reverse. rev has passed check_rev.
int check_link_up(const char *who, int64_t e, const int32_t *rev, const uint8_t *link_up) {
  for (int64_t k = 0; link_up && k < e; ++k)
    if ((link_up[k] != 0) != (link_up[rev[k]] != 0))
      return fail(FU_ERR_ARG, std::string(who) + ": link_up differs between slot " + std::to_string(k) + " and its reverse");
  return FU_OK;
}

}  // namespace

struct fu_churn : handle_base {
  static constexpr const char *kTag = "fu_churn";
  int32_t n_tiles = 0, n_heavy = 0;
  i64 *rowptr = nullptr;
  int *col = nullptr, *rev = nullptr, *hrows = nullptr;
  int2 *tiles = nullptr;
  unsigned char *alive = nullptr, *link_up = nullptr, *state = nullptr;
  double *v = nullptr, *a[2] = {nullptr, nullptr}, *f[2] = {nullptr, nullptr};
  u64 *count = nullptr;
  std::vector<int32_t> h_rev;  // host copy: the symmetry check of link_up
  int64_t stats[2] = {0, 0};   // alive nodes, live slots of the current topology
};

static int launch_err(fu_churn *h, u64 *slot) {
  const unsigned grid = (unsigned)std::min<int64_t>(1024, ((int64_t)h->n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(kc_max_err, dim3(grid), dim3(kBlock), 0, h->stream, h->n, h->a[(h->round + 1) & 1], h->target, h->alive,
                     slot);  // a of the last round run
  HIP_TRY(hipGetLastError());
  return FU_OK;
}

static int launch_round(fu_churn *h) {
  const int64_t r = h->round;
  RoundArgs A;
  A.rowptr = h->rowptr;
  A.col = h->col;
  A.rev = h->rev;
  A.alive = h->alive;
  A.state = h->state;
  A.v = h->v;
  A.f_old = h->f[(r + 1) & 1];
  A.a_old = h->a[(r + 1) & 1];
  A.f_new = h->f[r & 1];
  A.a_new = h->a[r & 1];
  if (h->n_tiles > 0) hipLaunchKernelGGL(kc_light, dim3(h->n_tiles), dim3(kBlock), 0, h->stream, A, h->tiles);
  if (h->n_heavy > 0) hipLaunchKernelGGL(kc_heavy, dim3(h->n_heavy), dim3(kBlock), 0, h->stream, A, h->hrows);
  HIP_TRY(hipGetLastError());
  h->round = r + 1;
  return FU_OK;
}

// The state bytes from the device's alive and link_up, behind the rounds already queued;
// complete on return, with the counts in h->stats.
static int apply_topology(fu_churn *h, bool all_fresh) {
  const int64_t work = std::max<int64_t>(h->E, h->n);
  HIP_TRY(hipMemsetAsync(h->count, 0, 2 * sizeof(u64), h->stream));
  hipLaunchKernelGGL(kc_topology, dim3((unsigned)((work + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->n, (i64)h->E,
                     h->col, h->rev, h->alive, h->link_up, h->state, h->f[(h->round + 1) & 1], all_fresh ? 1 : 0, h->count);
  HIP_TRY(hipGetLastError());
  u64 c[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(c, h->count, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->stats[0] = (int64_t)c[0];
  h->stats[1] = (int64_t)c[1];
  return FU_OK;
}

extern "C" {

int fu_churn_destroy(fu_churn *h) {
  if (!h) return bad_arguments<fu_churn>("destroy");
  handle_close(h, {h->rowptr, h->col, h->rev, h->hrows, h->tiles, h->alive, h->link_up, h->state, h->v, h->a[0], h->a[1],
                   h->f[0], h->f[1], h->count});
  delete h;
  return FU_OK;
}

// Every check on the arguments comes before the first HIP call, so a host without a GPU
// reports an asymmetric graph or a bad rev as such.
int fu_churn_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                    const double *value, int32_t device, fu_churn **out) {
  FU_TRY_BEGIN
  if (!out || !rowptr || !value || n <= 0 || e < 0 || (e > 0 && !col)) return bad_arguments<fu_churn>("create");
  if (e > (int64_t)INT32_MAX) return fail(FU_ERR_ARG, "fu_churn_create: more than 2^31-1 directed edges (rev is int32)");
  if (int rc = check_csr("fu_churn_create", n, e, rowptr, col)) return rc;
  std::vector<int32_t> built;
  if (e > 0 && !rev) {
    if (int rc = rev_of_csr(n, e, rowptr, col, &built)) return rc;
    rev = built.data();
  }
  if (int rc = check_rev("fu_churn_create", RevCheck::kPairing, n, rowptr, col, rev)) return rc;
  // the launch plan of fu_lossy_create: heavy rows one block each; the rows between them in
  // tiles of at most kTileRows rows and kTileEdges slots
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
  auto *h = new fu_churn();
  h->n_tiles = (int32_t)tiles.size();
  h->n_heavy = (int32_t)heavy.size();
  if (e > 0) h->h_rev.assign(rev, rev + e);
  auto cleanup = [&](int code) { fu_churn_destroy(h); return code; };
  int rc = FU_OK;
  if ((rc = handle_open(h, device, n, e, 1))) return cleanup(rc);
  const int64_t e1 = std::max<int64_t>(e, 1);
  if ((rc = dmalloc(h, &h->rowptr, (int64_t)n + 1)) || (rc = dmalloc(h, &h->col, e)) || (rc = dmalloc(h, &h->rev, e)) ||
      (rc = dmalloc(h, &h->hrows, h->n_heavy)) || (rc = dmalloc(h, &h->tiles, h->n_tiles)) ||
      (rc = dmalloc(h, &h->alive, n)) || (rc = dmalloc(h, &h->link_up, e)) || (rc = dmalloc(h, &h->state, e)) ||
      (rc = dmalloc(h, &h->v, n)) || (rc = dmalloc(h, &h->a[0], n)) || (rc = dmalloc(h, &h->a[1], n)) ||
      (rc = dmalloc(h, &h->f[0], e1)) || (rc = dmalloc(h, &h->f[1], e1)) || (rc = dmalloc(h, &h->count, 2)))
    return cleanup(rc);
  static_assert(sizeof(i64) == sizeof(int64_t), "rowptr is uploaded as is");
  if ((rc = put(h, h->rowptr, rowptr, (int64_t)n + 1)) || (rc = put(h, h->col, col, e)) || (rc = put(h, h->rev, rev, e)) ||
      (rc = put(h, h->hrows, heavy.data(), h->n_heavy)) || (rc = put(h, h->tiles, tiles.data(), h->n_tiles)) ||
      (rc = put(h, h->v, value, n)))
    return cleanup(rc);
  if ((rc = zero(h, h->a[0], n)) || (rc = zero(h, h->a[1], n)) || (rc = zero(h, h->f[0], e1)) || (rc = zero(h, h->f[1], e1)))
    return cleanup(rc);
  // everything alive and up, every slot FRESH
  if (hipMemset(h->alive, 1, (size_t)n) != hipSuccess || hipMemset(h->link_up, 1, (size_t)e1) != hipSuccess ||
      hipMemset(h->state, kFresh, (size_t)e1) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_churn_create: memset failed"));
  h->stats[0] = n;
  h->stats[1] = e;
  *out = h;
  return FU_OK;
  FU_TRY_END
}

int fu_churn_create_from_graph(const fu_graph *g, const double *value, int32_t device, fu_churn **out) {
  return create_from_graph<fu_churn>(g, value, out, [&](auto... csr) { return fu_churn_create(csr..., value, device, out); });
}

int fu_churn_set_topology(fu_churn *h, const uint8_t *alive, const uint8_t *link_up) {
  FU_TRY_BEGIN
  if (!h) return bad_arguments<fu_churn>("set_topology");
  if (int rc = check_link_up("fu_churn_set_topology", h->E, h->h_rev.data(), link_up)) return rc;
  if (int rc = set_device(h)) return rc;
  if (alive)
    HIP_TRY(hipMemcpyAsync(h->alive, alive, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  else
    HIP_TRY(hipMemsetAsync(h->alive, 1, (size_t)h->n, h->stream));
  if (h->E > 0) {
    if (link_up)
      HIP_TRY(hipMemcpyAsync(h->link_up, link_up, (size_t)h->E, hipMemcpyHostToDevice, h->stream));
    else
      HIP_TRY(hipMemsetAsync(h->link_up, 1, (size_t)h->E, h->stream));
  }
  return apply_topology(h, /*all_fresh=*/false);
  FU_TRY_END
}

int fu_churn_set_values(fu_churn *h, const double *value) {
  if (!h || !value) return bad_arguments<fu_churn>("set_values");
  return upload(h, h->v, value, sizeof(double) * (size_t)h->n);
}

// Dead nodes keep their estimate and DOWN slots their +0.0 from round to round, so the
// buffers are zeroed here and round 0 is an ordinary round.
int fu_churn_reset(fu_churn *h) {
  FU_TRY_BEGIN
  if (!h) return bad_arguments<fu_churn>("reset");
  if (int rc = set_device(h)) return rc;
  for (int q = 0; q < 2; ++q) {
    HIP_TRY(hipMemsetAsync(h->a[q], 0, sizeof(double) * (size_t)h->n, h->stream));
    HIP_TRY(hipMemsetAsync(h->f[q], 0, sizeof(double) * (size_t)std::max<int64_t>(h->E, 1), h->stream));
  }
  h->round = 0;
  return apply_topology(h, /*all_fresh=*/true);
  FU_TRY_END
}

int fu_churn_set_targets(fu_churn *h, const double *target) { return set_targets(h, target); }
int fu_churn_run(fu_churn *h, int32_t rounds, int32_t err_every, double *err_trace) { return run(h, rounds, err_every, err_trace); }
int fu_churn_run_timed(fu_churn *h, int32_t rounds, float *ms) { return run_timed(h, rounds, ms); }
int fu_churn_max_err(fu_churn *h, double *out) { return max_err(h, out, /*needs_a_round=*/true); }
int fu_churn_get_round(fu_churn *h, int64_t *rounds_done) { return get_round(h, rounds_done); }
int fu_churn_synchronize(fu_churn *h) { return synchronize(h); }

int fu_churn_get_estimates(fu_churn *h, double *a_out) {
  if (!h || !a_out) return bad_arguments<fu_churn>("get_estimates");
  return download(h, a_out, h->a[(h->round + 1) & 1], sizeof(double) * (size_t)h->n);
}

int fu_churn_get_flows(fu_churn *h, double *f_out) {
  if (!h || (!f_out && h->E)) return bad_arguments<fu_churn>("get_flows");
  return download(h, f_out, h->f[(h->round + 1) & 1], sizeof(double) * (size_t)h->E);
}

int fu_churn_get_stats(fu_churn *h, int64_t out[2]) {
  if (!h || !out) return bad_arguments<fu_churn>("get_stats");
  out[0] = h->stats[0];
  out[1] = h->stats[1];
  return FU_OK;
}

int fu_churn_get_slot_state(fu_churn *h, uint8_t *state_out) {
  if (!h || (!state_out && h->E)) return bad_arguments<fu_churn>("get_slot_state");
  return download(h, state_out, h->state, (size_t)h->E);
}

int fu_churn_live(int32_t n, const int64_t *rowptr, const int32_t *col, const int32_t *rev, const uint8_t *alive,
                  const uint8_t *link_up, uint8_t *live_out) {
  FU_TRY_BEGIN
  if (!rowptr || n <= 0) return bad_arguments<fu_churn>("live");
  const int64_t e = rowptr[n];
  if (e < 0 || (e > 0 && (!col || !live_out))) return bad_arguments<fu_churn>("live");
  if (e > (int64_t)INT32_MAX) return fail(FU_ERR_ARG, "fu_churn_live: more than 2^31-1 directed edges (rev is int32)");
  if (int rc = check_csr("fu_churn_live", n, e, rowptr, col)) return rc;
  std::vector<int32_t> built;
  if (e > 0 && !rev) {
    if (int rc = rev_of_csr(n, e, rowptr, col, &built)) return rc;
    rev = built.data();
  }
  if (int rc = check_rev("fu_churn_live", RevCheck::kPairing, n, rowptr, col, rev)) return rc;
  if (int rc = check_link_up("fu_churn_live", e, rev, link_up)) return rc;
  for (int32_t i = 0; i < n; ++i)
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      live_out[k] = (!link_up || link_up[k] != 0) && (!alive || (alive[i] != 0 && alive[col[k]] != 0));
  return FU_OK;
  FU_TRY_END
}

}  // extern "C"
