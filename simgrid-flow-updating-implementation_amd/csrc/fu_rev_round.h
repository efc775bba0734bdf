// The collect-all round that gathers the reverse flow through `rev`: included by fu_lossy.hip
// and fu_churn.hip and by nothing else. It sits on csrc/fu_handle.h. DESIGN.md §4.16, §4.18.
//
// Round r over a fixed CSR, f and a double-buffered (round r reads [(r + 1) & 1] and writes
// [r & 1]). Every slot k = (i -> j) of row i is of one kind:
//   kGather: F = -f_old[rev k],  E = a_old[j]       counts in the divisor
//   kOwn:    F =  f_old[k],      E = a_old[i]       counts in the divisor
//   kZero:   F = 0.0,            E = 0.0            counts in the divisor
//   kSkip:   adds +0.0 to both chains, does not count, and its flow comes out as +0.0
//   S = 0.0 + F..,  T = 0.0 + E..  (left to right, row order),  live = the slots that count
//   a_new[i] = ((v[i] - S) + T) / (live + 1),   f_new[k] = (F + a_new[i]) - E
// A row that does not fire keeps a_old[i] and writes +0.0 flows (its slots are all kSkip).
//
// An engine's handle derives from rev_handle and the engine supplies a Rule:
//   struct Args;                                         its own kernel arguments
//   static constexpr bool kHasOwn, kHasSkip, kDeadRows;  can kOwn / kSkip occur, can a row not fire:
//                                                        what is false is compiled out
//   template <int N> __device__ static void classify(const Args &, const i64 (&k)[N], unsigned char (&kind)[N]);
//                                                        the kinds of a thread's N slots, all its
//                                                        loads issued before the first use
//   __device__ static bool fires(const Args &, int row);             only with kDeadRows
//   __device__ static void wrote(const Args &, i64 k, unsigned char kind);   with slot k's flow write,
//                                                        by the block that owns the row
//   __device__ static void block_end(const Args &, int &own_slots);  every thread, once: the kOwn
//                                                        slots this thread loaded
// A handle of K > 1 value columns (h->width; *_create_k) keeps estimates, values and targets
// node-major (x[i * K + c]) and flows edge-major (f[k * K + c]); one slot still has one col, one
// rev and one kind, and column c follows the rule above on its own. Such a handle runs
// k_light_cols and k_heavy_cols below, over a launch plan made for its K; a handle of one column
// runs k_light and k_heavy. DESIGN.md §4.19.
// The host half is written once over the handle type: the launch plan, the front half of
// *_create, the common part of *_destroy, the launch with its buffer rotation, and set_values,
// get_estimates and get_flows. Everything has internal linkage.
#pragma once

#include "fu_cols_err.h"
#include "fu_handle.h"

namespace fu {
namespace {

constexpr int kBlock = 256;        // threads per block (4 waves of 64)
constexpr int kTileRows = kBlock;  // light tiles: at most one row per thread
constexpr int kTileEdges = 2048;   // light tiles: (F, E, kind) of the tile's slots in LDS (34 KB: 4 blocks per CU)
constexpr int kHeavyDeg = 128;     // rows above this degree run one block per row
constexpr int kChunk = 2048;       // heavy rows: (F, E) elements staged in LDS per chunk

constexpr unsigned char kGather = 0, kSkip = 1, kZero = 2, kOwn = 3;

using i64 = long long;

struct RoundArgs {
  const i64 *rowptr;
  const int *col, *rev;
  const double *v, *f_old, *a_old;
  double *f_new, *a_new;
};

// ---- kernels ------------------------------------------------------------------------------
// Light tiles: consecutive rows of degree <= kHeavyDeg, at most kTileRows rows and kTileEdges
// slots. All threads load the tile's slots coalesced (col, rev, what the rule reads) and leave
// (F, E, kind) in LDS; thread t then runs row t's two chains from LDS in row order and leaves
// the new flows there; all threads write them out coalesced. The loading threads do not know
// the row, so a kOwn slot's estimate is chosen at chain time from the kind byte.
template <typename R>
__global__ __launch_bounds__(kBlock) void k_light(RoundArgs A, typename R::Args X, const int2 *__restrict__ tiles) {
  __shared__ double s_F[kTileEdges], s_E[kTileEdges];
  __shared__ unsigned char s_kind[kTileEdges];
  const int tid = threadIdx.x;
  const int2 tile = tiles[blockIdx.x];
  const i64 e0 = A.rowptr[tile.x];
  const int ne = (int)(A.rowptr[tile.y] - e0);  // <= kTileEdges (the host's tile plan)
  int own_slots = 0;
  if (ne > 0) {
    // Branch-free: a thread's kSlots slots (indices past the tile's end clamped to its last
    // slot, their results dropped) issue all their loads before the first use, so the two
    // gathers of every slot are in flight together. A slot that does not gather reads its own
    // flow through the same load (index k instead of rev k; kept only by kOwn) and its
    // estimate load is masked off.
    constexpr int kSlots = kTileEdges / kBlock;
    i64 k[kSlots];
    int c[kSlots], rv[kSlots];
    unsigned char kind[kSlots];
    double F[kSlots], E[kSlots];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int q = tid + u * kBlock;
      k[u] = e0 + (q < ne ? q : ne - 1);
      c[u] = A.col[k[u]];
      rv[u] = A.rev[k[u]];
    }
    R::classify(X, k, kind);
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      F[u] = A.f_old[kind[u] == kGather ? (i64)rv[u] : k[u]];
      E[u] = kind[u] == kGather ? A.a_old[c[u]] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int q = tid + u * kBlock;
      if (q < ne) {
        s_F[q] = kind[u] == kGather ? -F[u] : (R::kHasOwn && kind[u] == kOwn) ? F[u] : 0.0;
        s_E[q] = E[u];
        s_kind[q] = kind[u];
        if constexpr (R::kHasOwn) own_slots += kind[u] == kOwn;
      }
    }
  }
  __syncthreads();
  const int row = tile.x + tid;
  if (row < tile.y) {
    const int b = (int)(A.rowptr[row] - e0);
    const int d = (int)(A.rowptr[row + 1] - e0) - b;
    double own = 0.0;
    if constexpr (R::kHasOwn) own = A.a_old[row];
    double S = 0.0, T = 0.0;
    int live = d;
    for (int j = b; j < b + d; ++j) {
      S = S + s_F[j];  // a kSkip slot adds +0.0
      T = T + (R::kHasOwn && s_kind[j] == kOwn ? own : s_E[j]);
      if constexpr (R::kHasSkip) live -= s_kind[j] == kSkip;
    }
    double a = ((A.v[row] - S) + T) / (double)(live + 1);
    if constexpr (R::kDeadRows)
      if (!R::fires(X, row)) a = A.a_old[row];  // its slots are all kSkip: +0.0 flows below
    A.a_new[row] = a;
    for (int j = b; j < b + d; ++j) {
      const double f = (s_F[j] + a) - (R::kHasOwn && s_kind[j] == kOwn ? own : s_E[j]);
      s_F[j] = R::kHasSkip && s_kind[j] == kSkip ? 0.0 : f;
    }
  }
  __syncthreads();
  for (int q = tid; q < ne; q += kBlock) {
    A.f_new[e0 + q] = s_F[q];
    R::wrote(X, e0 + q, s_kind[q]);
  }
  R::block_end(X, own_slots);
}

// Slot k's kind and operands, for the heavy rows; own is the row's a_old.
template <typename R>
__device__ inline unsigned char fetch(const RoundArgs &A, const typename R::Args &X, i64 k, double own, double &F, double &E) {
  const i64 slot[1] = {k};
  unsigned char kinds[1];
  R::classify(X, slot, kinds);
  const unsigned char kind = kinds[0];
  if (kind == kGather) {
    F = -A.f_old[A.rev[k]];
    E = A.a_old[A.col[k]];
  } else if (R::kHasOwn && kind == kOwn) {
    F = A.f_old[k];
    E = own;
  } else {
    F = 0.0;
    E = 0.0;
  }
  return kind;
}

// Rows above kHeavyDeg: one block per row. All threads load a chunk of slots coalesced and
// leave (F, E) in LDS; lane 0 of wave 0 carries S and lane 0 of wave 1 carries T through the
// chunk in row order, from chunk to chunk, and every thread counts the kSkip slots it loaded,
// over all chunks. Once the block's count and a are known, a second pass fetches the operands
// again (nothing a slot's kind or operands depend on is written before it) and writes the
// flows coalesced.
template <typename R>
__global__ __launch_bounds__(kBlock) void k_heavy(RoundArgs A, typename R::Args X, const int *__restrict__ hrows) {
  __shared__ double s_F[kChunk], s_E[kChunk];
  __shared__ double s_T, s_a;
  const int tid = threadIdx.x;
  const int row = hrows[blockIdx.x];
  const i64 b = A.rowptr[row];
  const i64 d = A.rowptr[row + 1] - b;
  double own = 0.0;
  if constexpr (R::kHasOwn) own = A.a_old[row];
  double acc = 0.0;  // S in thread 0, T in thread 64
  int own_slots = 0, skipped = 0;
  for (i64 c0 = 0; c0 < d; c0 += kChunk) {
    const int m = (int)(d - c0 < kChunk ? d - c0 : kChunk);
#pragma unroll 4
    for (int q = tid; q < m; q += kBlock) {
      double F, E;
      const unsigned char kind = fetch<R>(A, X, b + c0 + q, own, F, E);
      s_F[q] = F;
      s_E[q] = E;
      if constexpr (R::kHasOwn) own_slots += kind == kOwn;
      if constexpr (R::kHasSkip) skipped += kind == kSkip;
    }
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < m; ++q) acc = acc + s_F[q];
    else if (tid == 64)
      for (int q = 0; q < m; ++q) acc = acc + s_E[q];
    __syncthreads();
  }
  __shared__ int s_skipped[kBlock / 64];  // each wave's count; no rule without kSkip touches it
  if constexpr (R::kHasSkip) {
    for (int off = 32; off > 0; off >>= 1) skipped += __shfl_xor(skipped, off, 64);
    if ((tid & 63) == 0) s_skipped[tid >> 6] = skipped;
  }
  if (tid == 64) s_T = acc;
  __syncthreads();
  if (tid == 0) {
    i64 live = d;
    if constexpr (R::kHasSkip)
      for (int q = 0; q < kBlock / 64; ++q) live -= s_skipped[q];
    double a = ((A.v[row] - acc) + s_T) / (double)(live + 1);
    if constexpr (R::kDeadRows)
      if (!R::fires(X, row)) a = A.a_old[row];
    A.a_new[row] = a;
    s_a = a;
  }
  __syncthreads();
  const double a = s_a;
  for (i64 q = tid; q < d; q += kBlock) {
    double F, E;
    const unsigned char kind = fetch<R>(A, X, b + q, own, F, E);
    A.f_new[b + q] = R::kHasSkip && kind == kSkip ? 0.0 : (F + a) - E;
    R::wrote(X, b + q, kind);
  }
  R::block_end(X, own_slots);
}

// ---- K value columns ------------------------------------------------------------------------
// 2 <= K <= kMaxCols. The unit is the (slot, column) element e = q * K + c of a tile or chunk of
// m slots, m * K <= kTileEdges elements. The slots are classified once each, by m threads; the
// operands are then loaded by element, so that a slot's K flows and K estimates are one
// contiguous read spread over K adjacent lanes. Between the two, a slot's kind sits in s_kind[q]
// and its two gather indices in the first element of its own LDS rows (s_F[q * K], s_E[q * K],
// as bit patterns): no LDS beyond the scalar kernels' 34 KB.
static_assert(kChunk == kTileEdges, "stash_slots and load_elems serve both kernels");
static_assert(kHeavyDeg * kMaxCols <= kTileEdges, "a light row alone fits a tile at every K");

// Slots k0 .. k0 + m - 1 (0 < m <= kTileEdges / 2): col, rev and the kind, once per slot. The
// flow index is rev k for a slot that gathers and k for every other (kept only by kOwn). With
// `last`, this is the pass that writes the flows and R::wrote goes with it: from here on the
// slot's kind is read from LDS alone.
template <typename R>
__device__ inline void stash_slots(const RoundArgs &A, const typename R::Args &X, i64 k0, int m, int K, double *s_F, double *s_E,
                                   unsigned char *s_kind, int &own_slots, int &skipped, bool last) {
  constexpr int kSlots = kTileEdges / 2 / kBlock;
  const int tid = threadIdx.x;
  i64 k[kSlots];
  int c[kSlots], rv[kSlots];
  unsigned char kind[kSlots];
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int q = tid + u * kBlock;
    k[u] = k0 + (q < m ? q : m - 1);
    c[u] = A.col[k[u]];
    rv[u] = A.rev[k[u]];
  }
  R::classify(X, k, kind);
#pragma unroll
  for (int u = 0; u < kSlots; ++u) {
    const int q = tid + u * kBlock;
    if (q < m) {
      s_kind[q] = kind[u];
      s_F[q * K] = __longlong_as_double(kind[u] == kGather ? (i64)rv[u] : k[u]);
      s_E[q * K] = __longlong_as_double((i64)c[u]);
      if constexpr (R::kHasOwn) own_slots += kind[u] == kOwn;
      if constexpr (R::kHasSkip) skipped += kind[u] == kSkip;
      if (last) R::wrote(X, k[u], kind[u]);
    }
  }
}

// The nel = m * K elements of the slots stashed above, after a barrier: every thread takes the
// kinds and indices of its elements out of LDS, a second barrier frees the rows, then all its
// loads are issued before the first use and use(e, c, kind, F, E) gets each element's operands:
// F signed as the chains add it, E the gathered estimate (0.0 for a slot that does not gather;
// the caller puts in the row's own estimate for kOwn).
template <typename R, typename Use>
__device__ inline void load_elems(const RoundArgs &A, int K, int nel, const double *s_F, const double *s_E,
                                  const unsigned char *s_kind, Use use) {
  constexpr int kElems = kTileEdges / kBlock;
  const int tid = threadIdx.x;
  i64 fi[kElems], ai[kElems];
  int c[kElems];
  unsigned char kind[kElems];
  double F[kElems], E[kElems];
#pragma unroll
  for (int u = 0; u < kElems; ++u) {
    const int e = tid + u * kBlock;
    const int q = (e < nel ? e : nel - 1) / K;
    c[u] = (e < nel ? e : nel - 1) - q * K;
    kind[u] = s_kind[q];
    fi[u] = __double_as_longlong(s_F[q * K]) * K + c[u];
    ai[u] = __double_as_longlong(s_E[q * K]) * K + c[u];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kElems; ++u) {
    F[u] = A.f_old[fi[u]];
    E[u] = kind[u] == kGather ? A.a_old[ai[u]] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < kElems; ++u) {
    const int e = tid + u * kBlock;
    if (e < nel) use(e, c[u], kind[u], kind[u] == kGather ? -F[u] : (R::kHasOwn && kind[u] == kOwn) ? F[u] : 0.0, E[u]);
  }
}

// Light tiles of K columns: at most kTileRows / K rows and kTileEdges / K slots (the host's plan
// for this K). The elements go to LDS as above; thread (row, c) = (t / K, t % K) runs the two
// chains of column c of its row from LDS in row order, with the row's one divisor, and leaves the
// new flows there; all threads write them out coalesced.
template <typename R>
__global__ __launch_bounds__(kBlock) void k_light_cols(RoundArgs A, typename R::Args X, const int2 *__restrict__ tiles, int K) {
  __shared__ double s_F[kTileEdges], s_E[kTileEdges];
  __shared__ unsigned char s_kind[kTileEdges / 2];
  const int tid = threadIdx.x;
  const int2 tile = tiles[blockIdx.x];
  const i64 e0 = A.rowptr[tile.x];
  const int ne = (int)(A.rowptr[tile.y] - e0);  // <= kTileEdges / K
  const int nel = ne * K;
  int own_slots = 0, skipped = 0;
  if (ne > 0) {
    stash_slots<R>(A, X, e0, ne, K, s_F, s_E, s_kind, own_slots, skipped, false);
    __syncthreads();
    load_elems<R>(A, K, nel, s_F, s_E, s_kind, [&](int e, int, unsigned char, double F, double E) {
      s_F[e] = F;
      s_E[e] = E;
    });
  }
  __syncthreads();
  const int r = tid / K, c = tid - r * K;
  const int row = tile.x + r;
  if (row < tile.y) {  // a tile has at most kBlock / K rows
    const i64 x = (i64)row * K + c;
    const int b = (int)(A.rowptr[row] - e0);
    const int d = (int)(A.rowptr[row + 1] - e0) - b;
    double own = 0.0;
    if constexpr (R::kHasOwn) own = A.a_old[x];
    double S = 0.0, T = 0.0;
    int live = d;
    for (int j = b; j < b + d; ++j) {
      S = S + s_F[j * K + c];  // a kSkip slot adds +0.0
      T = T + (R::kHasOwn && s_kind[j] == kOwn ? own : s_E[j * K + c]);
      if constexpr (R::kHasSkip) live -= s_kind[j] == kSkip;
    }
    double a = ((A.v[x] - S) + T) / (double)(live + 1);
    if constexpr (R::kDeadRows)
      if (!R::fires(X, row)) a = A.a_old[x];  // its slots are all kSkip: +0.0 flows below
    A.a_new[x] = a;
    for (int j = b; j < b + d; ++j) {
      const double f = (s_F[j * K + c] + a) - (R::kHasOwn && s_kind[j] == kOwn ? own : s_E[j * K + c]);
      s_F[j * K + c] = R::kHasSkip && s_kind[j] == kSkip ? 0.0 : f;
    }
  }
  __syncthreads();
  for (int e = tid; e < nel; e += kBlock) A.f_new[e0 * K + e] = s_F[e];
  for (int q = tid; q < ne; q += kBlock) R::wrote(X, e0 + q, s_kind[q]);
  R::block_end(X, own_slots);
}

// Heavy rows of K columns: one block per row, chunks of kChunk / K slots. Threads 0 .. K-1 carry
// the K values of S and threads 64 .. 64+K-1 the K values of T through the chunks in row order;
// the kSkip slots are counted per row. The second pass stages the chunks again (nothing a slot's
// kind or operands depend on is written before it) and writes the flows coalesced.
template <typename R>
__global__ __launch_bounds__(kBlock) void k_heavy_cols(RoundArgs A, typename R::Args X, const int *__restrict__ hrows, int K) {
  __shared__ double s_F[kChunk], s_E[kChunk];
  __shared__ unsigned char s_kind[kChunk / 2];
  __shared__ double s_own[kMaxCols], s_T[kMaxCols], s_a[kMaxCols];
  __shared__ int s_skipped[kBlock / 64];
  const int tid = threadIdx.x;
  const int row = hrows[blockIdx.x];
  const i64 b = A.rowptr[row];
  const i64 d = A.rowptr[row + 1] - b;
  const int cs = kChunk / K;
  if constexpr (R::kHasOwn)
    if (tid < K) s_own[tid] = A.a_old[(i64)row * K + tid];  // read after the first chunk's barrier
  double acc = 0.0;  // column c's S in thread c, its T in thread 64 + c
  int own_slots = 0, skipped = 0;
  for (i64 c0 = 0; c0 < d; c0 += cs) {
    const int m = (int)(d - c0 < cs ? d - c0 : cs);
    stash_slots<R>(A, X, b + c0, m, K, s_F, s_E, s_kind, own_slots, skipped, false);
    __syncthreads();
    load_elems<R>(A, K, m * K, s_F, s_E, s_kind, [&](int e, int c, unsigned char kind, double F, double E) {
      s_F[e] = F;
      s_E[e] = R::kHasOwn && kind == kOwn ? s_own[c] : E;
    });
    __syncthreads();
    if (tid < K)
      for (int q = 0; q < m; ++q) acc = acc + s_F[q * K + tid];
    else if (tid >= 64 && tid < 64 + K)
      for (int q = 0; q < m; ++q) acc = acc + s_E[q * K + tid - 64];
    __syncthreads();
  }
  if constexpr (R::kHasSkip) {
    for (int off = 32; off > 0; off >>= 1) skipped += __shfl_xor(skipped, off, 64);
    if ((tid & 63) == 0) s_skipped[tid >> 6] = skipped;
  }
  if (tid >= 64 && tid < 64 + K) s_T[tid - 64] = acc;
  __syncthreads();
  if (tid < K) {
    const i64 x = (i64)row * K + tid;
    i64 live = d;
    if constexpr (R::kHasSkip)
      for (int q = 0; q < kBlock / 64; ++q) live -= s_skipped[q];
    double a = ((A.v[x] - acc) + s_T[tid]) / (double)(live + 1);
    if constexpr (R::kDeadRows)
      if (!R::fires(X, row)) a = A.a_old[x];
    A.a_new[x] = a;
    s_a[tid] = a;
  }
  __syncthreads();
  int counted = 0;  // both counts are the first pass's
  for (i64 c0 = 0; c0 < d; c0 += cs) {
    const int m = (int)(d - c0 < cs ? d - c0 : cs);
    stash_slots<R>(A, X, b + c0, m, K, s_F, s_E, s_kind, counted, counted, true);
    __syncthreads();
    // every thread has its elements in registers after load_elems' barrier, so the next chunk's
    // stash needs no barrier of its own
    load_elems<R>(A, K, m * K, s_F, s_E, s_kind, [&](int e, int c, unsigned char kind, double F, double E) {
      const double own_or_E = R::kHasOwn && kind == kOwn ? s_own[c] : E;
      A.f_new[(b + c0) * K + e] = R::kHasSkip && kind == kSkip ? 0.0 : (F + s_a[c]) - own_or_E;
    });
  }
  R::block_end(X, own_slots);
}

// ---- the handle -----------------------------------------------------------------------------
struct rev_handle : handle_base {
  int32_t n_tiles = 0, n_heavy = 0;
  i64 *rowptr = nullptr;
  int *col = nullptr, *rev = nullptr, *hrows = nullptr;
  int2 *tiles = nullptr;
  double *v = nullptr, *a[2] = {nullptr, nullptr}, *f[2] = {nullptr, nullptr};
};

// The launch plan for K columns: heavy rows one block each; the rows between them in tiles of at
// most kTileRows / K rows and kTileEdges / K slots.
inline void plan_rows(int32_t n, const int64_t *rowptr, int32_t K, std::vector<int32_t> *heavy, std::vector<int2> *tiles) {
  const int max_rows = kTileRows / K, max_slots = kTileEdges / K;
  for (int32_t i = 0; i < n;) {
    if (rowptr[i + 1] - rowptr[i] > kHeavyDeg) {
      heavy->push_back(i++);
      continue;
    }
    int32_t j = i;
    while (j < n && j - i < max_rows && rowptr[j + 1] - rowptr[j] <= kHeavyDeg && rowptr[j + 1] - rowptr[i] <= max_slots) ++j;
    tiles->push_back(make_int2(i, j));  // j > i: a light row alone always fits
    i = j;
  }
}

// The front half of *_create and *_create_k (`entry` names the one called, for the messages; k is
// the number of value columns). Every check on the arguments comes before the first HIP call, so
// a host without a GPU reports a bad k, an asymmetric graph or a bad rev as such. *hp stays null
// until the checks have passed; from then on the caller destroys it on any failure, of this
// function or of its own half. *rev comes back checked: the caller's, or the one built into *built.
template <typename H>
int rev_create(H **hp, const void *out, const char *entry, int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
               const int32_t **rev, std::vector<int32_t> *built, int32_t k, const double *value, int32_t device) {
  if (!out || !rowptr || !value || n <= 0 || e < 0 || (e > 0 && !col)) return bad_arguments<H>(entry);
  const std::string who = std::string(H::kTag) + "_" + entry;
  if (k < 1 || k > kMaxCols) return fail(FU_ERR_ARG, who + ": k must be in 1..16, got " + std::to_string(k));
  if (int rc = pairing_rev(who, n, e, rowptr, col, rev, built)) return rc;
  std::vector<int32_t> heavy;
  std::vector<int2> tiles;
  plan_rows(n, rowptr, k, &heavy, &tiles);
  H *h = *hp = new H();
  h->n_tiles = (int32_t)tiles.size();
  h->n_heavy = (int32_t)heavy.size();
  int rc = FU_OK;
  if ((rc = handle_open(h, device, n, e, k))) return rc;
  const int64_t nk = (int64_t)n * k, ek = std::max<int64_t>(e * k, 1);
  if ((rc = dmalloc(h, &h->rowptr, (int64_t)n + 1)) || (rc = dmalloc(h, &h->col, e)) || (rc = dmalloc(h, &h->rev, e)) ||
      (rc = dmalloc(h, &h->hrows, h->n_heavy)) || (rc = dmalloc(h, &h->tiles, h->n_tiles)) || (rc = dmalloc(h, &h->v, nk)) ||
      (rc = dmalloc(h, &h->a[0], nk)) || (rc = dmalloc(h, &h->a[1], nk)) || (rc = dmalloc(h, &h->f[0], ek)) ||
      (rc = dmalloc(h, &h->f[1], ek)))
    return rc;
  static_assert(sizeof(i64) == sizeof(int64_t), "rowptr is uploaded as is");
  if ((rc = put(h, h->rowptr, rowptr, (int64_t)n + 1)) || (rc = put(h, h->col, col, e)) || (rc = put(h, h->rev, *rev, e)) ||
      (rc = put(h, h->hrows, heavy.data(), h->n_heavy)) || (rc = put(h, h->tiles, tiles.data(), h->n_tiles)) ||
      (rc = put(h, h->v, value, nk)))
    return rc;
  if ((rc = zero(h, h->a[0], nk)) || (rc = zero(h, h->a[1], nk)) || (rc = zero(h, h->f[0], ek)) || (rc = zero(h, h->f[1], ek)))
    return rc;
  return FU_OK;
}

// *_destroy: the engine's own buffers and the common ones.
inline void rev_close(rev_handle *h, std::vector<void *> own) {
  own.insert(own.end(), {h->rowptr, h->col, h->rev, h->hrows, h->tiles, h->v, h->a[0], h->a[1], h->f[0], h->f[1]});
  handle_close(h, own);
}

// launch_round: round h->round with the rule's arguments X, and the counter advanced.
template <typename R, typename H>
int launch_rev_round(H *h, const typename R::Args &X) {
  const int64_t r = h->round;
  const RoundArgs A = {h->rowptr, h->col, h->rev, h->v, h->f[(r + 1) & 1], h->a[(r + 1) & 1], h->f[r & 1], h->a[r & 1]};
  const int K = h->width;
  if (K == 1) {
    if (h->n_tiles > 0) hipLaunchKernelGGL(k_light<R>, dim3(h->n_tiles), dim3(kBlock), 0, h->stream, A, X, h->tiles);
    if (h->n_heavy > 0) hipLaunchKernelGGL(k_heavy<R>, dim3(h->n_heavy), dim3(kBlock), 0, h->stream, A, X, h->hrows);
  } else {
    if (h->n_tiles > 0) hipLaunchKernelGGL(k_light_cols<R>, dim3(h->n_tiles), dim3(kBlock), 0, h->stream, A, X, h->tiles, K);
    if (h->n_heavy > 0) hipLaunchKernelGGL(k_heavy_cols<R>, dim3(h->n_heavy), dim3(kBlock), 0, h->stream, A, X, h->hrows, K);
  }
  HIP_TRY(hipGetLastError());
  h->round = r + 1;
  return FU_OK;
}

// launch_err of a handle of K > 1 columns: a is the last round's, alive may be null.
template <typename H>
int launch_max_err_cols(const H *h, const unsigned char *alive, u64 *slot) {
  return cols_err::launch(h, h->a[(h->round + 1) & 1], alive, slot);
}

// ---- the shared entry points ----------------------------------------------------------------
template <typename H>
int set_values(H *h, const double *value) {
  if (!h || !value) return bad_arguments<H>("set_values");
  return upload(h, h->v, value, sizeof(double) * (size_t)h->n * h->width);
}

// The last round's buffer, count doubles per column. zero_before_round_0: the engine's round 0 reads no
// state, so its buffers may hold an earlier run's and the zero state is written here; an
// engine that zeroes them on reset downloads like after any round.
template <typename H>
int get_last(H *h, double *out, double *const buf[2], int64_t count, bool zero_before_round_0) {
  count *= h->width;
  if (zero_before_round_0 && h->round == 0) {
    std::fill(out, out + count, 0.0);
    return FU_OK;
  }
  return download(h, out, buf[(h->round + 1) & 1], sizeof(double) * (size_t)count);
}

template <typename H>
int get_columns(H *h, int32_t *k) {
  if (!h || !k) return bad_arguments<H>("get_columns");
  *k = h->width;
  return FU_OK;
}

template <typename H>
int get_estimates(H *h, double *a_out, bool zero_before_round_0) {
  if (!h || !a_out) return bad_arguments<H>("get_estimates");
  return get_last(h, a_out, h->a, h->n, zero_before_round_0);
}

template <typename H>
int get_flows(H *h, double *f_out, bool zero_before_round_0) {
  if (!h || (!f_out && h->E)) return bad_arguments<H>("get_flows");
  return get_last(h, f_out, h->f, h->E, zero_before_round_0);
}

}  // namespace
}  // namespace fu
