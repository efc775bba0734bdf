// libfu synchronous pairwise engine for MI355X (gfx950): every round a matching of the graph is
// chosen on the device and each matched pair runs one full pairwise exchange. C ABI: the
// fu_pair section of include/fu.h. DESIGN.md §4.17.
//
// The matching of round r (key = splitmix_at(seed, r), h_i = splitmix_at(key, i)):
//   node i of degree > 0 proposes iff h_i & 1, over its slot p_i = (h_i >> 1) % deg_i, to
//   j = col[rowptr[i] + p_i]; the proposal is valid iff j listens (h_j & 1 == 0); a listener
//   accepts the valid proposal with the smallest ((h_i >> 32) << 32) | i. pair_proposal below is
//   the one statement of that rule: the kernels and fu_pair_matching share it.
//
// The exchange of a pair (i, s, j, t), t = rev[rowptr[i] + s] - rowptr[j]:
//   1. i fires on s (PW:102-117): S = 0.0 + f[row i].. in row order, a_i = (c[s] + (v_i - S)) / 2,
//      F1 = (f[s] + a_i) - c[s], last[i] = a_i.
//   2. j receives (PW:98-99): c[t] = a_i, f[t] = -F1; j fires on t: S over row j with the new
//      f[t], a_j = (a_i + (v_j - S)) / 2, F2 = (-F1 + a_j) - a_i, last[j] = a_j.
//   3. i receives: c[s] = a_j, f[s] = -F2, and does not fire again (the reference's ping-pong,
//      PW:100, never ends).
// What a pair leaves behind: f[s] = -F2, f[t] = F2, c[s] = c[t] = a_j, last[i] = a_i,
// last[j] = a_j. Rows of different pairs are disjoint, so the update is in place.
//
// Under loss the matching stays what it is; the message received on slot k in
// round r is lost iff down[k] != 0 or u01(splitmix_at(splitmix_at(~loss_seed, r), k)) < p: the
// receiver's slot decides, as in fu_lossy.hip. With ks = rowptr[i] + s and kt = rowptr[j] + t,
// m1 (i -> j) is received on kt and m2 (j -> i) on ks. The three outcomes of a pair:
//   m1 lost:   step 1 alone. f[ks] = F1, c[ks] = a_i, last[i] = a_i, fired[i] = 1; row j is
//              neither read nor written, fired[j] and last[j] stay, no m2 exists.
//   m2 lost:   steps 1 and 2. f[kt] = F2, c[kt] = a_j, last[j] = a_j, fired[j] = 1, and node i
//              keeps what it fired: f[ks] = F1, c[ks] = a_i.
//   delivered: steps 1 to 3, the lossless exchange bit for bit.
// Each is the reference's avg_and_send / on_receive with one message not handed over; the next
// message delivered over the link, in either direction, makes f antisymmetric on it again
// (PW:98-99). No new race: the matching does not look at the loss, so the rows of different
// pairs are still disjoint, every outcome writes only into rows i and j of its own pair (fewer
// slots than the full exchange, never others), `down` is read-only in a round, and the
// counters are atomics. So the update stays in place.
// The lossy forms of kp_exchange and kp_heavy are launched only when p > 0 or a mask is set;
// the lossless handle runs the instantiation it always ran.
//
// A round is kp_propose (one 64-bit atomicMin per valid proposal into the listener's word) or
// kp_scan (every listener hashes its own row; no atomics), then kp_exchange (a block compacts
// its matched listeners, 8 lanes per pair load both flow rows into LDS, one lane carries the
// two chains), then kp_heavy<Args, true> for the pairs with a row above kLightDeg (one block per
// pair, the rows in LDS chunks, thread 0 carrying). Nothing in a round waits for the host.
//
// A handle of K value columns (fu_pair_create_k) keeps v and last node-major
// (x[i * K + c]) and f and c edge-major (f[k * K + c]). The matching, the loss decisions, the
// heavy list, `fired` and the counters are per handle, as for one column; column c follows the
// exchange above on its own and no arithmetic crosses columns. Such a handle runs kp_propose or
// kp_scan as they are, then kp_exchange_cols (lane l of a pair's group carries columns l and
// l + 8 and reads its rows straight from memory) and kp_heavy<Args, false> (threads 0 .. K-1
// carry a column each through chunks of kColsChunk / K slots).
//
// What the kernels share is stated once: compact_matched (a block's words consumed, its pairs
// in listener order), `fire` (the arithmetic of steps 1 and 2), fired_unheard and settle (what
// each of the three outcomes writes into one column's cells: kp_exchange_cols and kp_heavy call
// them, kp_exchange writes its one column out itself, for a measured reason given there),
// list_heavy and the two flushes of the lost-message counters. The two exchange kernels differ
// on purpose; the heavy kernel is one body in two instantiations.
//
// Under a topology (fu_pair_set_topology) slot k = (i -> j) is live iff
// link_up[k] && alive[i] && alive[j], the churn engine's rule, and the handle keeps one live byte
// per slot and the live degree ldeg_i per node. kp_topology turns the uploaded masks into both; a
// slot that stops being live loses f and c in every column (+0.0: both ends drop the neighbour),
// one that becomes live keeps the +0.0 it holds (a neighbour just added, PW:33-34). The matching
// is the rule above on the live subgraph: a node with ldeg_i == 0 (a dead node has none) is idle,
// a proposer takes its p_i-th live slot in row order, p_i = (h_i >> 1) % ldeg_i; live_proposal
// below states it once for the kernels and fu_pair_matching_live. kp_pick writes the chosen slot
// into pick[i] (and pushes the proposal, form A; form B's kp_scan_live reads pick), and the
// <Topo<..>> instantiations of the exchange kernels take ks = pick[i] (if constexpr) in place of
// rowptr[i] + pair_slot(h_i, deg_i); kt = rev[ks] is live too, liveness being symmetric. Nothing
// else in them changes. The row sums keep running over the whole CSR row:
//   1. a dropped slot holds +0.0 (kp_topology wrote it, or it was never written);
//   2. no pair ever writes a dropped slot: only ks and kt are written, and both are live;
//   3. S starts from +0.0, and x + y is -0.0 only where x and y both are;
//   4. so S is never -0.0, and S + (+0.0) == S bit for bit, a NaN included;
//   5. hence the sum equals the reference's sum over the live neighbours only.
// The light/heavy split stays by CSR degree, and the loss decisions stay on the caller's slot
// index. A handle that never got a topology call launches the kernels it always launched.
//
// The handle scaffold (create and destroy, the run loops, the error slots and k_max_err, the
// small entry points) is csrc/fu_handle.h, shared with the batched and lossy engines; the
// per-column error reduction, kernel and launch, is csrc/fu_cols_err.h, shared with the
// rev-gather round.
#include "fu_cols_err.h"
#include "fu_handle.h"

using namespace fu;

namespace {

constexpr int kBlock = 256;                 // threads per block (4 waves of 64)
constexpr int kGroup = 8;                   // kp_exchange: lanes that load one pair's rows
constexpr int kGroups = kBlock / kGroup;    // pairs a block works on at once
constexpr int kLightDeg = 64;               // a pair with a row above this degree goes to kp_heavy
constexpr int kChunk = 1024;                // kp_heavy<Args, true>: flows staged in LDS per chunk
constexpr int kHeavyBlocks = 1024;          // kp_heavy: at most this many blocks share the round's heavy pairs
constexpr int kColsChunk = 2048;            // kp_heavy<Args, false>: doubles staged in LDS per chunk, kColsChunk / K slots
constexpr int kColsBatch = 8;               // kp_exchange_cols: a lane's loads of one column in flight before the adds
static_assert(kMaxCols <= 2 * kGroup, "a lane of a group carries at most two columns");
static_assert(kColsChunk / kMaxCols >= 1, "a chunk holds a slot at every K");

// The lost-message counters: kLostLines pairs (first messages lost, answers lost), a 128-byte
// line each; block b adds into pair b % kLostLines and fu_pair_get_loss_stats sums them. With
// one pair for all blocks the two more atomics per block on the line of the pair counter doubled
// the round.
constexpr int kLostLines = 64, kLostStride = 16;

constexpr u64 kNone = ~0ull;  // a listener's word without a proposal (no key is all-ones: i < 2^31)

static_assert(sizeof(u64) == sizeof(uint64_t), "the words are read as uint64_t on the host");

// ---- the rule, for host and device -----------------------------------------------------
FU_HD inline uint64_t round_key(uint64_t seed, uint64_t r) { return splitmix_at(seed, r); }
FU_HD inline int64_t pair_slot(uint64_t h, int64_t deg) { return (int64_t)((h >> 1) % (uint64_t)deg); }
// Does node i make a valid proposal in the round keyed `key`? If so j is the listener it
// proposes to and pk its priority there.
FU_HD inline bool pair_proposal(uint64_t key, int32_t i, const int64_t *rowptr, const int32_t *col, int32_t &j,
                                uint64_t &pk) {
  const uint64_t h = splitmix_at(key, (uint64_t)i);
  if (!(h & 1)) return false;  // i listens
  const int64_t b = rowptr[i], d = rowptr[i + 1] - b;
  if (d == 0) return false;  // idle
  j = col[b + pair_slot(h, d)];
  if (splitmix_at(key, (uint64_t)j) & 1) return false;  // j proposes too
  pk = ((h >> 32) << 32) | (uint64_t)(uint32_t)i;
  return true;
}

struct RoundArgs {
  int32_t n;
  const int64_t *rowptr;
  const int32_t *col, *rev;
  const double *v;
  double *f, *c, *last;
  u64 *word;             // per node: the smallest proposal key of this round, or kNone
  unsigned char *fired;  // per node: 1 once the node has fired
  u64 *pairs;            // the handle's pair counter
  int2 *heavy;           // (i, j) of this round's heavy pairs
  unsigned *n_heavy;
  int32_t heavy_cap;
  uint64_t key;          // round_key(seed, r)
  static constexpr bool kLossy = false;
  static constexpr bool kTopo = false;
};

// The rule under a topology: does node i propose in the round keyed `key`? If so ks is the slot
// it proposes over, the p_i-th live one of its row, and pk its priority at the listener
// col[ks]; whether that listener listens is the caller's to ask. `live` holds a byte per slot
// and ldeg the live slots per row (0 for a dead node).
FU_HD inline bool live_proposal(uint64_t key, int32_t i, const int64_t *rowptr, const unsigned char *live,
                                const int32_t *ldeg, int64_t &ks, uint64_t &pk) {
  const uint64_t h = splitmix_at(key, (uint64_t)i);
  if (!(h & 1)) return false;  // i listens
  const int32_t d = ldeg[i];
  if (d == 0) return false;  // idle
  int64_t p = pair_slot(h, d);
  for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
    if (live[k] && p-- == 0) {
      ks = k;
      pk = ((h >> 32) << 32) | (uint64_t)(uint32_t)i;
      return true;
    }
  return false;  // never: the row has ldeg[i] live bytes
}

// What the topology forms of the matching kernels read and write beside RoundArgs.
struct TopoArgs {
  const unsigned char *live;  // per slot
  const int32_t *ldeg;        // per node: live slots of its row
  int32_t *pick;              // per node: the slot a proposer chose this round, or -1
};

// The arguments of the topology instantiations of kp_exchange, kp_exchange_cols and kp_heavy,
// over RoundArgs or LossArgs: ks comes from pick.
template <class Base>
struct Topo : Base {
  const int32_t *pick;
  static constexpr bool kTopo = true;
};

// The arguments of the lossy instantiations of kp_exchange, kp_exchange_cols and kp_heavy; a
// handle without loss or mask runs the <RoundArgs> ones.
struct LossArgs : RoundArgs {
  const unsigned char *down;  // per slot: non-zero loses every message received on it; may be null
  u64 *lost;                  // the handle's counter pairs: [q * kLostStride] first messages lost, [.. + 1] answers lost
  uint64_t lkey;              // loss_key(loss_seed, r)
  double p;
  static constexpr bool kLossy = true;
};

// The key of round r's loss decisions (the complement keeps the stream apart from the
// matching's when both seeds are the same number), and the decision for the message received
// on slot k: the kernels and fu_pair_lost share both. The compare is fp64 on both sides.
FU_HD inline uint64_t loss_key(uint64_t seed, uint64_t r) { return splitmix_at(~seed, r); }
FU_HD inline bool slot_lost(uint64_t key, uint64_t k, double p) { return u01(splitmix_at(key, k)) < p; }
__device__ inline bool message_lost(const LossArgs &X, int64_t k) {
  return (X.down != nullptr && X.down[k] != 0) || (X.p > 0.0 && slot_lost(X.lkey, (uint64_t)k, X.p));
}

__device__ inline double fire_avg(double c, double v, double S) { return (c + (v - S)) / 2.0; }

// ---- one pair, one column: the arithmetic and the three outcomes ------------------------------
// A node of value v whose row sums to S fires on a slot holding flow f and cache c: its new
// average a and the flow F it sends. Step 1 is fire(f[ks], c[ks], v_i, S_i, a_i, F1); step 2,
// after j has received (c[kt] = a_i, f[kt] = -F1, the latter already in S_j), is
// fire(-F1, a_i, v_j, S_j, a_j, F2), so F2 = (-F1 + a_j) - a_i.
__device__ inline void fire(double f, double c, double v, double S, double &a, double &F) {
  a = fire_avg(c, v, S);
  F = (f + a) - c;
}

// What a pair leaves in one column's cells: fs, cs = f, c at ks; ft, ct = f, c at kt; li, lj =
// last at i, j. `fired` and the counters are per pair and stay with the caller.
// m1 lost: i fired into a message nobody received; row j is not touched.
__device__ inline void fired_unheard(double *fs, double *cs, double *li, double F1, double a_i) {
  *fs = F1;
  *cs = a_i;
  *li = a_i;
}
// m1 received. kept: m2 lost, j answered and i never heard it, so i keeps what it fired;
// otherwise delivered, the lossless exchange.
__device__ inline void settle(double *fs, double *cs, double *ft, double *ct, double *li, double *lj, double a_i,
                              double a_j, double F1, double F2, bool kept) {
  *fs = kept ? F1 : -F2;
  *cs = kept ? a_i : a_j;
  *ft = F2;
  *ct = a_j;
  *li = a_i;
  *lj = a_j;
}

// A pair with a row above kLightDeg goes on the round's list for kp_heavy: one lane per pair.
__device__ inline void list_heavy(const RoundArgs &A, int i, int j) {
  const unsigned slot = atomicAdd(A.n_heavy, 1u);
  if ((int64_t)slot < A.heavy_cap) A.heavy[slot] = make_int2(i, j);  // always: a heavy row is in one pair
}

// The lost-message counters of a block, into its line. The exchange kernels count per thread
// (every thread calls this: one atomic per block and counter), kp_heavy in thread 0 alone.
__device__ inline u64 *lost_line(const LossArgs &X) { return X.lost + (size_t)(blockIdx.x % kLostLines) * kLostStride; }
__device__ inline void flush_lost_block(const LossArgs &X, int n_lost1, int n_lost2) {
  block_count_to<kBlock>(n_lost1, lost_line(X));
  __syncthreads();  // block_count_to's LDS words are read by thread 0 until here
  block_count_to<kBlock>(n_lost2, lost_line(X) + 1);
}
__device__ inline void flush_lost_thread0(const LossArgs &X, unsigned n_lost1, unsigned n_lost2) {
  if (threadIdx.x == 0 && n_lost1) atomicAdd(lost_line(X), (u64)n_lost1);
  if (threadIdx.x == 0 && n_lost2) atomicAdd(lost_line(X) + 1, (u64)n_lost2);
}

// ---- matching, form A: proposers push -----------------------------------------------------
__global__ __launch_bounds__(kBlock) void kp_propose(RoundArgs A) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) *A.n_heavy = 0;  // the list of the round before has been consumed
  if (i >= A.n) return;
  int32_t j;
  uint64_t pk;
  if (pair_proposal(A.key, (int32_t)i, A.rowptr, A.col, j, pk)) atomicMin(&A.word[j], (u64)pk);
}

// ---- matching, form B: listeners pull -------------------------------------------------------
__global__ __launch_bounds__(kBlock) void kp_scan(RoundArgs A) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j == 0) *A.n_heavy = 0;
  if (j >= A.n) return;
  if (splitmix_at(A.key, (uint64_t)j) & 1) return;
  u64 best = kNone;
  for (int64_t k = A.rowptr[j]; k < A.rowptr[j + 1]; ++k) {
    int32_t to;
    uint64_t pk;
    if (pair_proposal(A.key, A.col[k], A.rowptr, A.col, to, pk) && to == (int32_t)j) best = pk < best ? (u64)pk : best;
  }
  if (best != kNone) A.word[j] = best;
}

// ---- the matching under a topology ---------------------------------------------------------
// Launched only once a topology has been set. Every proposer finds its chosen live slot from the
// live bytes of its row (contiguous; one thread a row, a long row included) and records it in
// pick[i] for the exchange. kPush (form A): a valid proposal goes into the listener's word as in
// kp_propose, and only proposers write pick. Without kPush (form B) every node writes pick, -1
// if it does not propose, and kp_scan_live reads it.
template <bool kPush>
__global__ __launch_bounds__(kBlock) void kp_pick(RoundArgs A, TopoArgs T) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) *A.n_heavy = 0;  // the list of the round before has been consumed
  if (i >= A.n) return;
  int64_t ks;
  uint64_t pk;
  const bool proposes = live_proposal(A.key, (int32_t)i, A.rowptr, T.live, T.ldeg, ks, pk);
  if (!kPush || proposes) T.pick[i] = proposes ? (int32_t)ks : -1;
  if (kPush && proposes) {
    const int32_t j = A.col[ks];
    if (!(splitmix_at(A.key, (uint64_t)j) & 1)) atomicMin(&A.word[j], (u64)pk);
  }
}

// Form B: listener j takes the smallest key among the neighbours whose pick is the reverse of
// one of its live slots. No atomics; kp_pick<false> of the same round has run.
__global__ __launch_bounds__(kBlock) void kp_scan_live(RoundArgs A, TopoArgs T) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= A.n) return;
  if (splitmix_at(A.key, (uint64_t)j) & 1) return;
  if (T.ldeg[j] == 0) return;
  u64 best = kNone;
  for (int64_t k = A.rowptr[j]; k < A.rowptr[j + 1]; ++k) {
    if (!T.live[k]) continue;
    const int32_t i = A.col[k];
    if (T.pick[i] != A.rev[k]) continue;
    const u64 pk = ((splitmix_at(A.key, (uint64_t)i) >> 32) << 32) | (u64)(uint32_t)i;
    best = pk < best ? pk : best;
  }
  if (best != kNone) A.word[j] = best;
}

// fu_pair_set_topology: one pass over the slots, from the uploaded alive and link_up and the
// old live byte to the new one. Slot k's row is col[rev k]. A slot that stops being live loses
// its K doubles of f and of c; a live slot adds one to its row's ldeg, zeroed before the launch.
// count[0] += alive nodes, count[1] += live slots, one atomic per block and counter; the grid
// covers max(E, n) threads, so every node is counted where E is small.
__global__ __launch_bounds__(kBlock) void kp_topology(int n, int64_t E, const int32_t *__restrict__ col,
                                                      const int32_t *__restrict__ rev, const unsigned char *__restrict__ alive,
                                                      const unsigned char *__restrict__ link_up, unsigned char *__restrict__ live,
                                                      int32_t *__restrict__ ldeg, double *__restrict__ f, double *__restrict__ c,
                                                      int K, u64 *__restrict__ count) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int now = 0;
  if (k < E) {
    const int32_t row = col[rev[k]];
    now = link_up[k] != 0 && alive[row] != 0 && alive[col[k]] != 0;
    if (now) {
      atomicAdd(&ldeg[row], 1);
    } else if (live[k]) {
      for (int q = 0; q < K; ++q) {
        f[k * K + q] = 0.0;
        c[k * K + q] = 0.0;
      }
    }
    live[k] = (unsigned char)now;
  }
  int up = k < n && alive[k] != 0;
  block_count_to<kBlock>(up, count);
  __syncthreads();  // block_count_to's wave sums are one LDS array: the first call has read it
  block_count_to<kBlock>(now, count + 1);
}

// ---- the exchange ------------------------------------------------------------------------
// Thread t of block b looks at node b * kBlock + t: a listener whose word holds a key is
// matched with the key's low half, and writes the word back to kNone. The block compacts its
// pairs (ballot, listener order) into s_pair[0 .. np-1] as (i, j); np is returned, the same in
// every thread. Every thread of the block calls it: both barriers are in here, and s_pair is
// complete on return.
__device__ inline int compact_matched(const RoundArgs &A, int2 *s_pair) {
  __shared__ int s_cnt[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t node = (int64_t)blockIdx.x * kBlock + tid;
  u64 word = kNone;
  if (node < A.n) {
    word = A.word[node];
    if (word != kNone) A.word[node] = kNone;
  }
  const bool matched = word != kNone;
  const u64 bal = __ballot(matched);
  if (lane == 0) s_cnt[w] = __popcll(bal);
  __syncthreads();
  int base = 0, np = 0;
  for (int q = 0; q < kBlock / 64; ++q) {
    if (q < w) base += s_cnt[q];
    np += s_cnt[q];
  }
  if (matched) s_pair[base + __popcll(bal & ((1ull << lane) - 1))] = make_int2((int)(uint32_t)word, (int)node);
  __syncthreads();
  return np;
}

// One column. The block works on kGroups of its pairs at a time: the 8 lanes of a group load
// the pair's two flow rows coalesced into the group's LDS rows, then lane 0 runs both chains
// from LDS in row order.
//
// Args::kLossy: all 8 lanes of a group read rev[ks] (one address: a broadcast) and with it hold both
// decisions of the pair, so a group whose m1 is lost never loads row j; without loss only lane 0
// reads it. The barriers of the q0 loop stay outside every per-pair branch. The lost messages
// are counted per thread (lane 0 of a group counts).
template <class Args>
__global__ __launch_bounds__(kBlock) void kp_exchange(Args A) {
  constexpr bool kLossy = Args::kLossy;
  __shared__ int2 s_pair[kBlock];
  __shared__ double s_f[kGroups][2 * kLightDeg];
  const int np = compact_matched(A, s_pair);
  const int tid = threadIdx.x, g = tid / kGroup, l = tid % kGroup;
  int n_lost1 = 0, n_lost2 = 0;
  for (int q0 = 0; q0 < np; q0 += kGroups) {  // np is the same in every thread: the barriers are uniform
    const int q = q0 + g;
    bool light = false, lost1 = false, lost2 = false;
    int i = 0, j = 0, di = 0, dj = 0, t = 0;
    int64_t bi = 0, bj = 0, ks = 0;
    double cs = 0.0, vi = 0.0, vj = 0.0;
    if (q < np) {
      i = s_pair[q].x;
      j = s_pair[q].y;
      bi = A.rowptr[i];
      di = (int)(A.rowptr[i + 1] - bi);
      bj = A.rowptr[j];
      dj = (int)(A.rowptr[j + 1] - bj);
      if (di > kLightDeg || dj > kLightDeg) {
        if (l == 0) list_heavy(A, i, j);
      } else {
        light = true;
        if constexpr (Args::kTopo)
          ks = A.pick[i];  // the proposer's chosen live slot (kp_pick)
        else
          ks = bi + pair_slot(splitmix_at(A.key, (uint64_t)i), di);
        for (int d = l; d < di; d += kGroup) s_f[g][d] = A.f[bi + d];
        if constexpr (kLossy) {
          const int64_t kt = A.rev[ks];  // in row j: fu_pair_create checked rev as a pairing
          t = (int)(kt - bj);
          lost1 = message_lost(A, kt);
          lost2 = message_lost(A, ks);
          if (!lost1)
            for (int d = l; d < dj; d += kGroup) s_f[g][kLightDeg + d] = A.f[bj + d];
          if (l == 0) {
            cs = A.c[ks];
            vi = A.v[i];
            if (!lost1) vj = A.v[j];
          }
        } else {
          for (int d = l; d < dj; d += kGroup) s_f[g][kLightDeg + d] = A.f[bj + d];
          if (l == 0) {
            t = (int)(A.rev[ks] - bj);
            cs = A.c[ks];
            vi = A.v[i];
            vj = A.v[j];
          }
        }
      }
    }
    __syncthreads();
    if (light && l == 0) {
      const double *fi = s_f[g], *fj = s_f[g] + kLightDeg;
      double S = 0.0, a_i, F1;
      for (int d = 0; d < di; ++d) S = S + fi[d];
      fire(fi[ks - bi], cs, vi, S, a_i, F1);
      // The three outcomes are written out here, not through fired_unheard and settle: with the
      // helpers the compiler forms all six addresses before the first store, and that order
      // measured 0.1-0.9 us a round slower on RR-1M (MEASUREMENTS.md §19.2, §19.3).
      if (kLossy && lost1) {  // i fired into a message nobody received
        A.f[ks] = F1;
        A.c[ks] = a_i;
        A.last[i] = a_i;
        A.fired[i] = 1;
        n_lost1 += 1;
      } else {
        S = 0.0;
        for (int d = 0; d < dj; ++d) S = S + (d == t ? -F1 : fj[d]);
        double a_j, F2;
        fire(-F1, a_i, vj, S, a_j, F2);
        if (kLossy && lost2) {  // j answered, i never heard it
          A.f[ks] = F1;
          A.c[ks] = a_i;
          n_lost2 += 1;
        } else {
          A.f[ks] = -F2;
          A.c[ks] = a_j;
        }
        A.f[bj + t] = F2;
        A.c[bj + t] = a_j;
        A.last[i] = a_i;
        A.last[j] = a_j;
        A.fired[i] = 1;
        A.fired[j] = 1;
      }
    }
    __syncthreads();
  }
  if (tid == 0 && np > 0) atomicAdd(A.pairs, (u64)np);
  if constexpr (kLossy) flush_lost_block(A, n_lost1, n_lost2);
}

// ---- K value columns ------------------------------------------------------------------------
// The sums of one row for a lane's two columns: S0 = 0.0 + p[0], p[K], .. and S1 the same from
// p + kGroup (only if `two`), in row order; slot `sub` of the row counts as (r0, r1) in place of
// what is stored (-1: no slot). The loads do not depend on the adds, so kColsBatch slots of both
// columns are in flight before the first add of a batch.
__device__ inline void row_sums(const double *__restrict__ p, int deg, int K, bool two, int sub, double r0, double r1,
                                double &S0, double &S1) {
  S0 = 0.0;
  S1 = 0.0;
  for (int d0 = 0; d0 < deg; d0 += kColsBatch) {
    double x0[kColsBatch], x1[kColsBatch];
#pragma unroll
    for (int u = 0; u < kColsBatch; ++u) {
      const int d = d0 + u;
      x0[u] = d < deg ? p[(int64_t)d * K] : 0.0;
      x1[u] = d < deg && two ? p[(int64_t)d * K + kGroup] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kColsBatch; ++u) {
      const int d = d0 + u;
      if (d < deg) {
        S0 = S0 + (d == sub ? r0 : x0[u]);
        S1 = S1 + (d == sub ? r1 : x1[u]);
      }
    }
  }
}

// kp_exchange for K columns: the same compaction and the same group of 8 lanes per pair. Lane l
// of a group carries columns l and l + 8 of its pair through both chains. Nothing is staged in
// LDS: at K columns the two rows of kGroups pairs do not fit it, the loads of a row do not
// depend on the adds, and across the lanes of a group the loads of f[(b + d) * K + c] are
// contiguous, as are the writes of f, c and last. So the q0 loop has no barrier, and a lane
// without a column (l >= K) sits a pair out. Lane 0 writes `fired`, lists a heavy pair and
// counts the lost messages: once per pair, as in kp_exchange.
template <class Args>
__global__ __launch_bounds__(kBlock) void kp_exchange_cols(Args A, int K) {
  constexpr bool kLossy = Args::kLossy;
  __shared__ int2 s_pair[kBlock];
  const int np = compact_matched(A, s_pair);
  const int tid = threadIdx.x, g = tid / kGroup, l = tid % kGroup;
  const bool two = l + kGroup < K;
  int n_lost1 = 0, n_lost2 = 0;
  for (int q = g; q < np; q += kGroups) {
    const int i = s_pair[q].x, j = s_pair[q].y;
    const int64_t bi = A.rowptr[i], bj = A.rowptr[j];
    const int di = (int)(A.rowptr[i + 1] - bi), dj = (int)(A.rowptr[j + 1] - bj);
    if (di > kLightDeg || dj > kLightDeg) {
      if (l == 0) list_heavy(A, i, j);
      continue;
    }
    int64_t ks;
    if constexpr (Args::kTopo)
      ks = A.pick[i];  // the proposer's chosen live slot (kp_pick)
    else
      ks = bi + pair_slot(splitmix_at(A.key, (uint64_t)i), di);
    const int64_t kt = A.rev[ks];  // in row j: fu_pair_create_k checked rev as a pairing
    bool lost1 = false, lost2 = false;
    if constexpr (kLossy) {
      lost1 = message_lost(A, kt);
      lost2 = message_lost(A, ks);
    }
    if (l < K) {
      // this lane's columns are l and, if `two`, l + kGroup; the second of a lane that has one
      // is computed on zeros and never written
      const int64_t o1 = two ? kGroup : 0;
      double *fs = A.f + ks * K + l, *cs = A.c + ks * K + l, *li = A.last + (int64_t)i * K + l;
      double *ft = A.f + kt * K + l, *ct = A.c + kt * K + l, *lj = A.last + (int64_t)j * K + l;
      const double *vi = A.v + (int64_t)i * K + l, *vj = A.v + (int64_t)j * K + l;
      const double c0 = cs[0], c1 = cs[o1], v0 = vi[0], v1 = vi[o1], f0 = fs[0], f1 = fs[o1];
      double w0 = 0.0, w1 = 0.0;
      if (!lost1) {
        w0 = vj[0];
        w1 = vj[o1];
      }
      double S0, S1, ai0, ai1, F10, F11;
      row_sums(A.f + bi * K + l, di, K, two, -1, 0.0, 0.0, S0, S1);
      fire(f0, c0, v0, S0, ai0, F10);
      fire(f1, c1, v1, S1, ai1, F11);
      if (kLossy && lost1) {
        fired_unheard(fs, cs, li, F10, ai0);
        if (two) fired_unheard(fs + kGroup, cs + kGroup, li + kGroup, F11, ai1);
      } else {
        row_sums(A.f + bj * K + l, dj, K, two, (int)(kt - bj), -F10, -F11, S0, S1);
        double aj0, aj1, F20, F21;
        fire(-F10, ai0, w0, S0, aj0, F20);
        fire(-F11, ai1, w1, S1, aj1, F21);
        const bool kept = kLossy && lost2;
        settle(fs, cs, ft, ct, li, lj, ai0, aj0, F10, F20, kept);
        if (two) settle(fs + kGroup, cs + kGroup, ft + kGroup, ct + kGroup, li + kGroup, lj + kGroup, ai1, aj1, F11, F21, kept);
      }
    }
    if (l == 0) {
      A.fired[i] = 1;
      if (kLossy && lost1) {
        n_lost1 += 1;
      } else {
        A.fired[j] = 1;
        if (kLossy && lost2) n_lost2 += 1;
      }
    }
  }
  if (tid == 0 && np > 0) atomicAdd(A.pairs, (u64)np);
  if constexpr (kLossy) flush_lost_block(A, n_lost1, n_lost2);
}

// ---- heavy pairs ------------------------------------------------------------------------------
// kp_heavy's sum over one row of K columns (`row` is its first double, `deg` its slots): all
// threads load a chunk of `chunk` slots coalesced into s_f as they lie in memory, and thread
// c < K carries column c's sum through the chunk in row order (K consecutive LDS words per slot:
// no bank conflict), from chunk to chunk. With kSub, slot t of the row counts as r in place of
// what is stored. Every thread of the block calls it: the barriers are uniform.
template <bool kSub>
__device__ inline double heavy_row_sum(const double *row, int64_t deg, int K, int chunk, int64_t t, double r, double *s_f) {
  const int tid = threadIdx.x;
  double S = 0.0;
  for (int64_t c0 = 0; c0 < deg; c0 += chunk) {
    const int m = (int)(deg - c0 < chunk ? deg - c0 : chunk);
    const double *src = row + c0 * K;
    for (int e = tid; e < m * K; e += kBlock) s_f[e] = src[e];
    __syncthreads();
    if (tid < K) {
      const int64_t tc = t - c0;  // slot t's place in this chunk, if it is in it
      for (int d = 0; d < m; ++d) S = S + (kSub && d == tc ? r : s_f[d * K + tid]);
    }
    __syncthreads();
  }
  return S;
}

// Pairs with a row above kLightDeg: one block per pair, at most kHeavyBlocks blocks sharing the
// list; first the sum over row i and then, with -F1 in slot t's place, over row j. Two
// instantiations of one body:
//   kOne = true, the scalar handle's: K is 1 at compile time, chunks of kChunk slots (8 KB of
//     LDS), thread 0 carrying; K_ is not read.
//   kOne = false, a handle of fu_pair_create_k at every K = K_, 1 included: chunks of
//     kColsChunk / K slots (16 KB), threads 0 .. K-1 carrying a column each.
//
// Args::kLossy: every thread holds kt and the loss key, so every thread of the block takes the same
// decision on m1 and the sum over row j, which has barriers, is skipped by all or by none.
// Thread 0 writes `fired` and counts the lost messages: once per pair.
template <class Args, bool kOne>
__global__ __launch_bounds__(kBlock) void kp_heavy(Args A, int K_) {
  constexpr bool kLossy = Args::kLossy;
  __shared__ double s_f[kOne ? kChunk : kColsChunk];
  const int K = kOne ? 1 : K_;
  const int chunk = kOne ? kChunk : kColsChunk / K;  // slots per chunk
  const int tid = threadIdx.x;
  const unsigned listed = *A.n_heavy;
  const unsigned cnt = (int64_t)listed < A.heavy_cap ? listed : (unsigned)A.heavy_cap;
  unsigned n_lost1 = 0, n_lost2 = 0;
  for (unsigned q = blockIdx.x; q < cnt; q += gridDim.x) {
    const int i = A.heavy[q].x, j = A.heavy[q].y;
    const int64_t bi = A.rowptr[i], di = A.rowptr[i + 1] - bi;
    const int64_t bj = A.rowptr[j], dj = A.rowptr[j + 1] - bj;
    int64_t ks;
    if constexpr (Args::kTopo)
      ks = A.pick[i];  // the proposer's chosen live slot (kp_pick)
    else
      ks = bi + pair_slot(splitmix_at(A.key, (uint64_t)i), di);
    const int64_t kt = A.rev[ks];
    bool lost1 = false, lost2 = false;
    if constexpr (kLossy) {
      lost1 = message_lost(A, kt);
      lost2 = message_lost(A, ks);
    }
    // this thread's column of the pair's cells, if tid < K
    const int64_t os = ks * K + tid, ot = kt * K + tid, oi = (int64_t)i * K + tid, oj = (int64_t)j * K + tid;
    double S = heavy_row_sum<false>(A.f + bi * K, di, K, chunk, 0, 0.0, s_f);
    double a_i = 0.0, F1 = 0.0;
    if (tid < K) fire(A.f[os], A.c[os], A.v[oi], S, a_i, F1);
    if (kLossy && lost1) {  // the same in every thread of the block
      if (tid < K) fired_unheard(A.f + os, A.c + os, A.last + oi, F1, a_i);
      if (tid == 0) {
        A.fired[i] = 1;
        n_lost1 += 1;
      }
      continue;
    }
    S = heavy_row_sum<true>(A.f + bj * K, dj, K, chunk, kt - bj, -F1, s_f);
    const bool kept = kLossy && lost2;
    if (tid < K) {
      double a_j, F2;
      fire(-F1, a_i, A.v[oj], S, a_j, F2);
      settle(A.f + os, A.c + os, A.f + ot, A.c + ot, A.last + oi, A.last + oj, a_i, a_j, F1, F2, kept);
    }
    if (tid == 0) {
      A.fired[i] = 1;
      A.fired[j] = 1;
      n_lost2 += kept;
    }
  }
  if constexpr (kLossy) flush_lost_thread0(A, n_lost1, n_lost2);
}

// How many nodes have never fired: one atomic per block that found some.
__global__ __launch_bounds__(kBlock) void kp_count_unfired(int n, const unsigned char *__restrict__ fired,
                                                           u64 *__restrict__ out) {
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) cnt += fired[i] == 0;
  block_count_to<kBlock>(cnt, out);
}

}  // namespace

struct fu_pair : handle_base {
  static constexpr const char *kTag = "fu_pair";
  uint64_t seed = 0;
  int match = 0;             // 0: kp_propose, 1: kp_scan
  int32_t n_heavy_rows = 0;  // rows above kLightDeg: the bound on a round's heavy pairs
  int64_t *rowptr = nullptr;
  int32_t *col = nullptr, *rev = nullptr;
  double *v = nullptr, *f = nullptr, *c = nullptr, *last = nullptr;
  u64 *word = nullptr;
  unsigned char *fired = nullptr;
  int2 *heavy = nullptr;
  unsigned *n_heavy = nullptr;
  u64 *stat = nullptr;  // [0] matched pairs, [1] scratch of kp_count_unfired, from [2] on the kLostLines lost-message counter pairs
  double p = 0.0;       // loss probability and seed of the rounds launched from now on
  uint64_t loss_seed = 0;
  bool has_mask = false;
  unsigned char *down = nullptr;  // E bytes, allocated when a mask is first set
  // The topology (fu_pair_set_topology). Until the first call every slot is live, none of the
  // buffers exists and the rounds are the ones without a topology.
  bool has_topo = false;
  unsigned char *alive = nullptr, *link_up = nullptr, *live = nullptr;  // n, E, E bytes
  int32_t *ldeg = nullptr, *pick = nullptr;                             // n each
  u64 *count = nullptr;                                                 // kp_topology's two counters
  std::vector<int32_t> h_rev;  // host copy: the symmetry check of link_up
  int64_t topo_stats[2] = {0, 0};  // alive nodes, live slots of the current topology
  bool cols = false;  // made by fu_pair_create_k: v and last hold n * width doubles, f and c E * width, and the rounds are kp_exchange_cols and kp_heavy<Args, false>
};

constexpr int kStats = 2 + kLostLines * kLostStride;

static unsigned node_grid(const fu_pair *h) { return (unsigned)(((int64_t)h->n + kBlock - 1) / kBlock); }

static int launch_err(fu_pair *h, u64 *slot) {
  const unsigned char *alive = h->has_topo ? h->alive : nullptr;  // once a topology is set: over the alive nodes
  if (h->cols) return cols_err::launch(h, h->last, alive, slot);
  if (alive) return launch_max_err_alive<kBlock>(h, h->last, alive, slot);
  return launch_max_err<kBlock>(h, h->last, slot);
}

// The exchange of a round in the handle's form, after the matching: K columns (a handle of
// fu_pair_create_k, at every K) or one, and kp_heavy's instantiation with it.
template <class Args>
static void launch_exchange(const fu_pair *h, const Args &X) {
  const dim3 grid(node_grid(h)), heavy_grid(std::min(h->n_heavy_rows, kHeavyBlocks)), block(kBlock);
  if (h->cols) {
    hipLaunchKernelGGL(kp_exchange_cols<Args>, grid, block, 0, h->stream, X, h->width);
    if (h->n_heavy_rows > 0) hipLaunchKernelGGL((kp_heavy<Args, false>), heavy_grid, block, 0, h->stream, X, h->width);
  } else {
    hipLaunchKernelGGL(kp_exchange<Args>, grid, block, 0, h->stream, X);
    if (h->n_heavy_rows > 0) hipLaunchKernelGGL((kp_heavy<Args, true>), heavy_grid, block, 0, h->stream, X, 1);
  }
}

// launch_exchange with the handle's topology, if it has one: the <Topo<Args>> instantiations.
template <class Args>
static void launch_in_topology(const fu_pair *h, const Args &X) {
  if (!h->has_topo) return launch_exchange(h, X);
  Topo<Args> Y;
  static_cast<Args &>(Y) = X;
  Y.pick = h->pick;
  launch_exchange(h, Y);
}

static int launch_round(fu_pair *h) {
  RoundArgs A;
  A.n = h->n;
  A.rowptr = h->rowptr;
  A.col = h->col;
  A.rev = h->rev;
  A.v = h->v;
  A.f = h->f;
  A.c = h->c;
  A.last = h->last;
  A.word = h->word;
  A.fired = h->fired;
  A.pairs = h->stat;
  A.heavy = h->heavy;
  A.n_heavy = h->n_heavy;
  A.heavy_cap = h->n_heavy_rows;
  A.key = round_key(h->seed, (uint64_t)h->round);
  if (h->E > 0) {  // without edges every node is idle
    const dim3 grid(node_grid(h)), block(kBlock);
    if (h->has_topo) {
      const TopoArgs T{h->live, h->ldeg, h->pick};
      if (h->match == 0) {
        hipLaunchKernelGGL(kp_pick<true>, grid, block, 0, h->stream, A, T);
      } else {
        hipLaunchKernelGGL(kp_pick<false>, grid, block, 0, h->stream, A, T);
        hipLaunchKernelGGL(kp_scan_live, grid, block, 0, h->stream, A, T);
      }
    } else if (h->match == 0) {
      hipLaunchKernelGGL(kp_propose, grid, block, 0, h->stream, A);
    } else {
      hipLaunchKernelGGL(kp_scan, grid, block, 0, h->stream, A);
    }
    if (h->p > 0.0 || h->has_mask) {
      LossArgs X;
      static_cast<RoundArgs &>(X) = A;
      X.down = h->has_mask ? h->down : nullptr;
      X.lost = h->stat + 2;
      X.lkey = loss_key(h->loss_seed, (uint64_t)h->round);
      X.p = h->p;
      launch_in_topology(h, X);
    } else {  // no loss, no mask: the lossless kernels as they always ran
      launch_in_topology(h, A);
    }
    HIP_TRY(hipGetLastError());
  }
  h->round += 1;
  return FU_OK;
}

// Zero state: flows, caches, last averages, fired flags, counters; every word without a proposal.
static int zero_state(fu_pair *h) {
  const size_t e = (size_t)std::max<int64_t>(h->E, 1), n = (size_t)h->n, k = (size_t)h->width;
  HIP_TRY(hipMemsetAsync(h->f, 0, sizeof(double) * e * k, h->stream));
  HIP_TRY(hipMemsetAsync(h->c, 0, sizeof(double) * e * k, h->stream));
  HIP_TRY(hipMemsetAsync(h->last, 0, sizeof(double) * n * k, h->stream));
  HIP_TRY(hipMemsetAsync(h->fired, 0, n, h->stream));
  HIP_TRY(hipMemsetAsync(h->word, 0xFF, sizeof(u64) * n, h->stream));
  HIP_TRY(hipMemsetAsync(h->stat, 0, sizeof(u64) * kStats, h->stream));
  HIP_TRY(hipMemsetAsync(h->n_heavy, 0, sizeof(unsigned), h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->round = 0;
  return FU_OK;
}

extern "C" {

int fu_pair_destroy(fu_pair *h) {
  if (!h) return bad_arguments<fu_pair>("destroy");
  handle_close(h, {h->rowptr, h->col, h->rev, h->v, h->f, h->c, h->last, h->word, h->fired, h->heavy, h->n_heavy, h->stat, h->down,
                   h->alive, h->link_up, h->live, h->ldeg, h->pick, h->count});
  delete h;
  return FU_OK;
}

}  // extern "C"

// fu_pair_create (k = 1, cols = false) and fu_pair_create_k (`entry` names the one called, for
// the messages). Every check on the arguments comes before the first HIP call, so a host without
// a GPU reports a bad k, an asymmetric graph or a bad rev as such.
static int pair_create(const char *entry, int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                       int32_t k, bool cols, const double *value, int32_t device, fu_pair **out) {
  FU_TRY_BEGIN
  if (!out || !rowptr || !value || n <= 0 || e < 0 || (e > 0 && !col)) return bad_arguments<fu_pair>(entry);
  const std::string who = std::string("fu_pair_") + entry;
  if (k < 1 || k > kMaxCols) return fail(FU_ERR_ARG, who + ": k must be in 1..16, got " + std::to_string(k));
  std::vector<int32_t> built;
  if (int rc = pairing_rev(who, n, e, rowptr, col, &rev, &built)) return rc;
  int32_t heavy_rows = 0;
  for (int32_t i = 0; i < n; ++i) heavy_rows += rowptr[i + 1] - rowptr[i] > kLightDeg;
  auto *h = new fu_pair();
  h->n_heavy_rows = heavy_rows;
  h->cols = cols;
  if (e > 0) h->h_rev.assign(rev, rev + e);
  h->topo_stats[0] = n;
  h->topo_stats[1] = e;
  auto cleanup = [&](int code) { fu_pair_destroy(h); return code; };
  int rc = FU_OK;
  if ((rc = handle_open(h, device, n, e, k))) return cleanup(rc);
  const int64_t nk = (int64_t)n * k, ek = std::max<int64_t>(e, 1) * k;
  if ((rc = dmalloc(h, &h->rowptr, (int64_t)n + 1)) || (rc = dmalloc(h, &h->col, e)) || (rc = dmalloc(h, &h->rev, e)) ||
      (rc = dmalloc(h, &h->v, nk)) || (rc = dmalloc(h, &h->f, ek)) || (rc = dmalloc(h, &h->c, ek)) ||
      (rc = dmalloc(h, &h->last, nk)) || (rc = dmalloc(h, &h->word, n)) || (rc = dmalloc(h, &h->fired, n)) ||
      (rc = dmalloc(h, &h->heavy, heavy_rows)) || (rc = dmalloc(h, &h->n_heavy, 1)) || (rc = dmalloc(h, &h->stat, kStats)))
    return cleanup(rc);
  if ((rc = put(h, h->rowptr, rowptr, (int64_t)n + 1)) || (rc = put(h, h->col, col, e)) || (rc = put(h, h->rev, rev, e)) ||
      (rc = put(h, h->v, value, nk)) || (rc = zero_state(h)))
    return cleanup(rc);
  *out = h;
  return FU_OK;
  FU_TRY_END
}

extern "C" {

int fu_pair_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                   const double *value, int32_t device, fu_pair **out) {
  return pair_create("create", n, e, rowptr, col, rev, 1, /*cols=*/false, value, device, out);
}

int fu_pair_create_k(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev, int32_t k,
                     const double *value, int32_t device, fu_pair **out) {
  return pair_create("create_k", n, e, rowptr, col, rev, k, /*cols=*/true, value, device, out);
}

int fu_pair_create_from_graph(const fu_graph *g, const double *value, int32_t device, fu_pair **out) {
  return create_from_graph<fu_pair>(g, value, out, [&](auto... csr) { return fu_pair_create(csr..., value, device, out); });
}

int fu_pair_create_from_graph_k(const fu_graph *g, int32_t k, const double *value, int32_t device, fu_pair **out) {
  FU_TRY_BEGIN
  if (g && value && out && (k < 1 || k > kMaxCols))  // after the null checks, before the graph's
    return fail(FU_ERR_ARG, "fu_pair_create_from_graph_k: k must be in 1..16, got " + std::to_string(k));
  return create_from_graph<fu_pair>(g, value, out, [&](auto... csr) { return fu_pair_create_k(csr..., k, value, device, out); });
  FU_TRY_END
}

int fu_pair_get_columns(fu_pair *h, int32_t *k) {
  if (!h || !k) return bad_arguments<fu_pair>("get_columns");
  *k = h->width;
  return FU_OK;
}

int fu_pair_set_seed(fu_pair *h, uint64_t seed) {
  if (!h) return bad_arguments<fu_pair>("set_seed");
  h->seed = seed;  // a kernel argument of the rounds launched from now on
  return FU_OK;
}

int fu_pair_set_loss(fu_pair *h, double p, uint64_t seed) {
  if (!h) return bad_arguments<fu_pair>("set_loss");
  if (!(p >= 0.0 && p <= 1.0)) return fail(FU_ERR_ARG, "fu_pair_set_loss: p must be in [0, 1]");
  h->p = p;  // kernel arguments of the rounds launched from now on
  h->loss_seed = seed;
  return FU_OK;
}

int fu_pair_set_link_mask(fu_pair *h, const uint8_t *down) {
  FU_TRY_BEGIN
  if (!h) return bad_arguments<fu_pair>("set_link_mask");
  if (!down || h->E == 0) {
    h->has_mask = false;  // rounds already queued keep their own argument copy; the buffer stays
    return FU_OK;
  }
  if (int rc = set_device(h)) return rc;
  if (!h->down)
    if (int rc = dmalloc(h, &h->down, h->E)) return rc;
  // over the handle's stream: the rounds queued before the call read the old bytes first
  if (int rc = upload(h, h->down, down, (size_t)h->E)) return rc;
  h->has_mask = true;
  return FU_OK;
  FU_TRY_END
}

// The first call allocates the topology's buffers, every slot live as it has been since create.
// Each buffer is guarded by its own pointer: a call after a failed one allocates only what is missing.
static int topology_buffers(fu_pair *h) {
  if (h->live) return FU_OK;
  int rc = FU_OK;
  if ((!h->alive && (rc = dmalloc(h, &h->alive, h->n))) || (!h->link_up && (rc = dmalloc(h, &h->link_up, h->E))) ||
      (!h->ldeg && (rc = dmalloc(h, &h->ldeg, h->n))) || (!h->pick && (rc = dmalloc(h, &h->pick, h->n))) ||
      (!h->count && (rc = dmalloc(h, &h->count, 2))))
    return rc;
  unsigned char *live = nullptr;
  if ((rc = dmalloc(h, &live, h->E))) return rc;
  if (hipMemsetAsync(live, 1, (size_t)std::max<int64_t>(h->E, 1), h->stream) != hipSuccess) {
    (void)hipFree(live);
    return fail(FU_ERR_HIP, "fu_pair_set_topology: memset failed");
  }
  h->live = live;
  return FU_OK;
}

int fu_pair_set_topology(fu_pair *h, const uint8_t *alive, const uint8_t *link_up) {
  FU_TRY_BEGIN
  if (!h) return bad_arguments<fu_pair>("set_topology");
  if (int rc = check_link_up("fu_pair_set_topology", h->E, h->h_rev.data(), link_up)) return rc;
  if (int rc = set_device(h)) return rc;
  if (int rc = topology_buffers(h)) return rc;
  // over the handle's stream: the rounds queued before the call run under the old topology
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
  HIP_TRY(hipMemsetAsync(h->ldeg, 0, sizeof(int32_t) * (size_t)h->n, h->stream));
  HIP_TRY(hipMemsetAsync(h->count, 0, 2 * sizeof(u64), h->stream));
  const int64_t work = std::max<int64_t>(h->E, h->n);
  hipLaunchKernelGGL(kp_topology, dim3((unsigned)((work + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->n, h->E, h->col,
                     h->rev, h->alive, h->link_up, h->live, h->ldeg, h->f, h->c, h->width, h->count);
  HIP_TRY(hipGetLastError());
  // The pass is queued: the live bytes and the cells are the new topology's whatever follows, so
  // the rounds launched from now on take the topology kernels even if the counts cannot be read
  // (FU_ERR_HIP then, with the statistics of the call before).
  h->has_topo = true;
  u64 c[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(c, h->count, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->topo_stats[0] = (int64_t)c[0];
  h->topo_stats[1] = (int64_t)c[1];
  return FU_OK;
  FU_TRY_END
}

int fu_pair_get_topology_stats(fu_pair *h, int64_t out[2]) {
  if (!h || !out) return bad_arguments<fu_pair>("get_topology_stats");
  out[0] = h->topo_stats[0];
  out[1] = h->topo_stats[1];
  return FU_OK;
}

// Before the first topology call every slot is live and no buffer holds that.
int fu_pair_get_slot_live(fu_pair *h, uint8_t *live_out) {
  if (!h || (!live_out && h->E)) return bad_arguments<fu_pair>("get_slot_live");
  if (!h->live) {
    std::fill(live_out, live_out + h->E, (uint8_t)1);
    return FU_OK;
  }
  return download(h, live_out, h->live, (size_t)h->E);
}

int fu_pair_set_option(fu_pair *h, const char *key, int64_t value) {
  if (!h || !key) return bad_arguments<fu_pair>("set_option");
  if (std::strcmp(key, "match") == 0 && (value == 0 || value == 1)) {
    h->match = (int)value;
    return FU_OK;
  }
  return fail(FU_ERR_ARG, std::string("fu_pair_set_option: unknown option or value: ") + key);
}

int fu_pair_set_values(fu_pair *h, const double *value) {
  if (!h || !value) return bad_arguments<fu_pair>("set_values");
  return upload(h, h->v, value, sizeof(double) * (size_t)h->n * h->width);
}

int fu_pair_reset(fu_pair *h) {
  if (!h) return bad_arguments<fu_pair>("reset");
  if (int rc = set_device(h)) return rc;
  return zero_state(h);
}

int fu_pair_set_targets(fu_pair *h, const double *target) { return set_targets(h, target); }
int fu_pair_run(fu_pair *h, int32_t rounds, int32_t err_every, double *err_trace) { return run(h, rounds, err_every, err_trace); }
int fu_pair_run_timed(fu_pair *h, int32_t rounds, float *ms) { return run_timed(h, rounds, ms); }
// Allowed before any round: every node's last average is 0.0 then.
int fu_pair_max_err(fu_pair *h, double *out) { return max_err(h, out, /*needs_a_round=*/false); }
int fu_pair_get_round(fu_pair *h, int64_t *rounds_done) { return get_round(h, rounds_done); }
int fu_pair_synchronize(fu_pair *h) { return synchronize(h); }

// The state is on the device from create on: round 0 downloads like any other.
int fu_pair_get_estimates(fu_pair *h, double *last_out) {
  if (!h || !last_out) return bad_arguments<fu_pair>("get_estimates");
  return download(h, last_out, h->last, sizeof(double) * (size_t)h->n * h->width);
}

int fu_pair_get_flows(fu_pair *h, double *f_out) {
  if (!h || (!f_out && h->E)) return bad_arguments<fu_pair>("get_flows");
  return download(h, f_out, h->f, sizeof(double) * (size_t)h->E * h->width);
}

int fu_pair_get_cache(fu_pair *h, double *c_out) {
  if (!h || (!c_out && h->E)) return bad_arguments<fu_pair>("get_cache");
  return download(h, c_out, h->c, sizeof(double) * (size_t)h->E * h->width);
}

int fu_pair_get_stats(fu_pair *h, int64_t out[2]) {
  FU_TRY_BEGIN
  if (!h || !out) return bad_arguments<fu_pair>("get_stats");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemsetAsync(h->stat + 1, 0, sizeof(u64), h->stream));
  hipLaunchKernelGGL(kp_count_unfired, dim3(std::min(1024u, node_grid(h))), dim3(kBlock), 0, h->stream, h->n, h->fired,
                     h->stat + 1);
  HIP_TRY(hipGetLastError());
  u64 s[2] = {0, 0};
  if (int rc = download(h, s, h->stat, sizeof(s))) return rc;
  out[0] = (int64_t)s[0];
  out[1] = (int64_t)s[1];
  return FU_OK;
  FU_TRY_END
}

// complete = matched pairs minus the two kinds of loss: the lossless kernels count pairs only.
int fu_pair_get_loss_stats(fu_pair *h, int64_t out[3]) {
  FU_TRY_BEGIN
  if (!h) return fail(FU_ERR_ARG, "fu_pair_get_loss_stats: the handle is NULL");
  if (!out) return fail(FU_ERR_ARG, "fu_pair_get_loss_stats: out is NULL (three int64 are written)");
  std::vector<u64> s((size_t)kStats);
  if (int rc = download(h, s.data(), h->stat, sizeof(u64) * s.size())) return rc;
  u64 lost1 = 0, lost2 = 0;
  for (int q = 0; q < kLostLines; ++q) {
    lost1 += s[2 + q * kLostStride];
    lost2 += s[3 + q * kLostStride];
  }
  out[0] = (int64_t)lost1;
  out[1] = (int64_t)lost2;
  out[2] = (int64_t)(s[0] - lost1 - lost2);
  return FU_OK;
  FU_TRY_END
}

int fu_pair_lost(uint64_t seed, int64_t round, int64_t first, int64_t count, double p, uint8_t *out) {
  if (round < 0 || first < 0 || count < 0 || (count > 0 && !out) || !(p >= 0.0 && p <= 1.0))
    return fail(FU_ERR_ARG, "fu_pair_lost: bad arguments");
  if (first > INT64_MAX - count) return fail(FU_ERR_ARG, "fu_pair_lost: first + count is past 2^63 - 1");
  const uint64_t key = loss_key(seed, (uint64_t)round);
  for (int64_t q = 0; q < count; ++q) out[q] = p > 0.0 && slot_lost(key, (uint64_t)(first + q), p) ? 1 : 0;
  return FU_OK;
}

}  // extern "C"

// fu_pair_matching (live == nullptr) and fu_pair_matching_live (a byte per slot): the proposals
// of the round into the listeners' words, then the pairs out of them.
static int host_matching(int32_t n, const int64_t *rowptr, const int32_t *col, const unsigned char *live,
                         uint64_t seed, int64_t round, int32_t *mate, uint8_t *initiator) {
  const uint64_t key = round_key(seed, (uint64_t)round);
  std::vector<uint64_t> word((size_t)n, (uint64_t)kNone);
  std::vector<int32_t> ldeg;
  if (live) {
    ldeg.assign((size_t)n, 0);
    for (int32_t i = 0; i < n; ++i)
      for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) ldeg[i] += live[k] != 0;
  }
  for (int32_t i = 0; i < n; ++i) {
    int32_t j;
    uint64_t pk;
    if (live) {
      int64_t ks;
      if (!live_proposal(key, i, rowptr, live, ldeg.data(), ks, pk)) continue;
      j = col[ks];
      if (splitmix_at(key, (uint64_t)j) & 1) continue;  // j proposes too
      word[j] = std::min(word[j], pk);
    } else if (pair_proposal(key, i, rowptr, col, j, pk)) {
      word[j] = std::min(word[j], pk);
    }
  }
  std::fill(mate, mate + n, -1);
  std::fill(initiator, initiator + n, (uint8_t)0);
  for (int32_t j = 0; j < n; ++j)
    if (word[j] != (uint64_t)kNone) {
      const int32_t i = (int32_t)(uint32_t)word[j];
      mate[i] = j;
      mate[j] = i;
      initiator[i] = 1;
    }
  return FU_OK;
}

extern "C" {

int fu_pair_matching(int32_t n, const int64_t *rowptr, const int32_t *col, uint64_t seed, int64_t round, int32_t *mate,
                     uint8_t *initiator) {
  FU_TRY_BEGIN
  if (n <= 0 || !rowptr || round < 0 || !mate || !initiator || rowptr[0] != 0 || (rowptr[n] > 0 && !col))
    return fail(FU_ERR_ARG, "fu_pair_matching: bad arguments");
  if (int rc = check_csr("fu_pair_matching", n, rowptr[n], rowptr, col)) return rc;
  return host_matching(n, rowptr, col, nullptr, seed, round, mate, initiator);
  FU_TRY_END
}

int fu_pair_matching_live(int32_t n, const int64_t *rowptr, const int32_t *col, const uint8_t *alive, const uint8_t *link_up,
                          uint64_t seed, int64_t round, int32_t *mate, uint8_t *initiator) {
  FU_TRY_BEGIN
  if (n <= 0 || !rowptr || round < 0 || !mate || !initiator || rowptr[0] != 0 || (rowptr[n] > 0 && !col))
    return fail(FU_ERR_ARG, "fu_pair_matching_live: bad arguments");
  if (!alive && !link_up) return fu_pair_matching(n, rowptr, col, seed, round, mate, initiator);
  const int64_t e = rowptr[n];
  const int32_t *rev = nullptr;
  std::vector<int32_t> built;
  if (int rc = pairing_rev("fu_pair_matching_live", n, e, rowptr, col, &rev, &built)) return rc;
  if (int rc = check_link_up("fu_pair_matching_live", e, rev, link_up)) return rc;
  std::vector<unsigned char> live((size_t)std::max<int64_t>(e, 1));
  for (int32_t i = 0; i < n; ++i)
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      live[k] = (!link_up || link_up[k] != 0) && (!alive || (alive[i] != 0 && alive[col[k]] != 0));
  return host_matching(n, rowptr, col, live.data(), seed, round, mate, initiator);
  FU_TRY_END
}

}  // extern "C"
