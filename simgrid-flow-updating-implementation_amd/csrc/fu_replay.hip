// libfu tick replay for MI355X (gfx950): the per-tick kernel, the two persistent kernels and
// the fu_replay_* entry points, on the stream part of the handle scaffold (fu_handle.h).
// C ABI declared in include/fu.h; DESIGN.md §4.10.
#include "fu_handle.h"
#include "fu_tuning.h"

using namespace fu;

namespace {

constexpr int kBlock = 256;  // threads per block (4 waves of 64)
inline unsigned grid_for(long long work) { return (unsigned)((work + kBlock - 1) / kBlock); }

__global__ void k_fill(long long cnt, double val, double *__restrict__ p) {
  long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (q < cnt) p[q] = val;
}

// ------------------------------------------------------------------------------------
// Tick replay: one thread per task (= one node's events in one tick, in program order).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_replay_tick(
    long long task_begin, int ntasks, const int *__restrict__ tasks,
    const long long *__restrict__ rowptr, const int *__restrict__ events,
    const int *__restrict__ out_ids, const double *__restrict__ v, double *__restrict__ flow,
    double *__restrict__ est, double *__restrict__ last, double2 *__restrict__ msg) {
  int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= ntasks) return;
  const int *tk = tasks + 3 * (task_begin + q);
  const int node = tk[0], evb = tk[1], eve = tk[2];
  double *fl = flow + rowptr[node];
  double *es = est + rowptr[node];
  const double val = v[node];
  for (int p = evb; p < eve; ++p) {
    const int4 ev = *reinterpret_cast<const int4 *>(events + 4 * (long long)p);
    if (ev.x == FU_EV_RECV) {  // CA:98-99 / PW:98-99
      const double2 m = msg[ev.z];
      es[ev.y] = m.y;
      fl[ev.y] = -m.x;
    } else if (ev.x == FU_EV_FIRE_CA) {  // CA:105-125
      const int k = ev.y;
      double S = 0.0, T = 0.0;
      for (int j = 0; j < k; ++j) S = S + fl[j];
      const double estimate = val - S;
      for (int j = 0; j < k; ++j) T = T + es[j];
      const double avg = (estimate + T) / (double)(k + 1);
      last[node] = avg;
      for (int j = 0; j < k; ++j) {
        const double nf = (fl[j] + avg) - es[j];
        fl[j] = nf;
        es[j] = avg;
        msg[out_ids[ev.z + j]] = make_double2(nf, avg);
      }
    } else {  // FIRE_PW, PW:102-117
      const int s = ev.y, k = ev.z;
      double S = 0.0;
      for (int j = 0; j < k; ++j) S = S + fl[j];
      const double estimate = val - S;
      const double avg = (es[s] + estimate) / 2.0;
      last[node] = avg;
      const double nf = (fl[s] + avg) - es[s];
      fl[s] = nf;
      es[s] = avg;
      msg[ev.w] = make_double2(nf, avg);
    }
  }
}

// ------------------------------------------------------------------------------------
// Persistent replay: one launch for all ticks, dataflow order. Each thread owns nodes
// {gtid, gtid + G, ...} and walks each node's events in program order (events regrouped
// per node on the host). A RECV waits until its message exists. Messages have unique slots
// (no recycling), so a slot is written once: it starts as a signalling-NaN sentinel that
// arithmetic never produces, and each 8-byte half is its own readiness tag (data-tagged
// granule: agent-scope relaxed sc1 store, sc1 load; MI355X_MICROARCH.md "hand-off"). Per-node
// order + produce-before-consume is exactly the dependence structure of the tick batches,
// so the results are the same bits. A thread never blocks on one node: it polls once and
// moves on. The globally earliest pending event is always ready, so a fully resident grid
// always makes progress. The grid is sized below the occupancy bound.
// ------------------------------------------------------------------------------------
constexpr unsigned long long kMsgSentinel = 0x7FF7A5A5A5A5A5A5ull;

__device__ inline unsigned long long ld_tag(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st_tag(unsigned long long *p, double v) {
  __hip_atomic_store(p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void k_replay_persist(
    int n, int tick_end, const long long *__restrict__ node_off, const int4 *__restrict__ node_ev,
    const int *__restrict__ node_tick, const int *__restrict__ out_uid,
    const long long *__restrict__ rowptr, const double *__restrict__ v, double *__restrict__ flow,
    double *__restrict__ est, double *__restrict__ last, unsigned long long *__restrict__ pay,
    long long *__restrict__ cursor, int *__restrict__ scur, int n_snap,
    const int *__restrict__ snap_ticks, double *__restrict__ snaps, int *__restrict__ status,
    long long max_iters) {
  const int G = gridDim.x * kBlock;
  const int g = blockIdx.x * kBlock + threadIdx.x;
  long long it = 0;
  bool left = true;
  while (left) {
    left = false;
    bool progressed = false;
    for (int node = g; node < n; node += G) {
      long long p = cursor[node];
      const long long pe = node_off[node + 1];
      int sc = scur[node];
      double *fl = flow + rowptr[node];
      double *es = est + rowptr[node];
      const double val = v[node];
      double lst = last[node];
      while (p < pe) {
        const int tk = node_tick[p];
        if (tk >= tick_end) break;
        while (sc < n_snap && snap_ticks[sc] < tk) snaps[(long long)sc++ * n + node] = lst;
        const int4 ev = node_ev[p];
        if (ev.x == FU_EV_RECV) {
          const unsigned long long fx = ld_tag(pay + 2 * (long long)ev.z);
          const unsigned long long fy = ld_tag(pay + 2 * (long long)ev.z + 1);
          if (fx == kMsgSentinel || fy == kMsgSentinel) break;  // not sent yet
          es[ev.y] = __longlong_as_double((long long)fy);
          fl[ev.y] = -__longlong_as_double((long long)fx);
        } else if (ev.x == FU_EV_FIRE_CA) {
          const int k = ev.y;
          double S = 0.0, T = 0.0;
          for (int j = 0; j < k; ++j) S = S + fl[j];
          const double estimate = val - S;
          for (int j = 0; j < k; ++j) T = T + es[j];
          const double avg = (estimate + T) / (double)(k + 1);
          lst = avg;
          for (int j = 0; j < k; ++j) {
            const double nf = (fl[j] + avg) - es[j];
            fl[j] = nf;
            es[j] = avg;
            const long long m = out_uid[ev.z + j];
            st_tag(pay + 2 * m, nf);
            st_tag(pay + 2 * m + 1, avg);
          }
        } else {
          const int sl = ev.y, k = ev.z;
          double S = 0.0;
          for (int j = 0; j < k; ++j) S = S + fl[j];
          const double estimate = val - S;
          const double avg = (es[sl] + estimate) / 2.0;
          lst = avg;
          const double nf = (fl[sl] + avg) - es[sl];
          fl[sl] = nf;
          es[sl] = avg;
          st_tag(pay + 2 * (long long)ev.w, nf);
          st_tag(pay + 2 * (long long)ev.w + 1, avg);
        }
        ++p;
        progressed = true;
      }
      const bool done = p == pe || node_tick[p] >= tick_end;
      if (done)
        while (sc < n_snap && snap_ticks[sc] < tick_end) snaps[(long long)sc++ * n + node] = lst;
      cursor[node] = p;
      scur[node] = sc;
      last[node] = lst;
      if (!done) left = true;
    }
    if (left && !progressed) __builtin_amdgcn_s_sleep(2);
    if (++it > max_iters) {  // bounded spin: a bug must end the kernel, not hang the GPU
      atomicExch(status, 1);
      break;
    }
  }
}


// k_replay_persist with one node per thread and the node's state (its row of flows and
// estimate caches, cursor, snapshot cursor, last average) kept in registers for the whole
// run (degree <= MAXD): an event costs its own loads instead of also re-reading the node's
// state from memory on every pass. Same event semantics and order as k_replay_persist.
//
// The replay is bound by the time one lock-step iteration of a wave takes, not by the
// trace's dependence depth (RR-64K pairwise: ~6 message hops per 100 ticks; a node runs
// {receive, fire} every other tick), and an iteration ends waiting for its vector-memory
// operations, which retire in issue order: loads, and the write-through message stores.
// So an iteration issues as few of them as it can, in a fixed order:
//   * the lane's next events sit in a 16-entry LDS ring of packed 8-byte descriptors
//     (ev_dec), refilled 8 at a time (64 contiguous bytes); they land during one iteration
//     and are written to the ring at the head of the next;
//   * every iteration ends with exactly TWO 16-byte sc1 polls (the payloads of the lane's
//     next two receives, both tagged halves each) and then, on the pairwise path
//     (CA = false), exactly TWO 16-byte sc1 stores (the iteration's messages {flow, avg}),
//     each aimed at the node's scratch slot when there is none: the next iteration waits
//     for the polls and leaves the stores in flight (vmcnt(2)), instead of waiting for every
//     store's write-through;
//   * an iteration runs up to kRW events in program order, a receive only once its payload
//     has arrived in one of the two polls, at most two pairwise fires: RR-64K runs two
//     {receive, fire} pairs per iteration.
// The collect-all path (k messages per fire) stores its messages as it goes.
constexpr int kRW = 4;       // events per iteration at most
constexpr int kScan = 4;     // ring entries searched for the next two receives
constexpr int kRing = 16;    // LDS ring entries per lane
constexpr int kRefill = 8;   // events per refill (64 contiguous bytes)
// packed 8-byte event: x = type | slot << 2 | k << 7 | tick << 12 (deg <= 16, tick < 2^20),
// y = message slot (receive, pairwise fire) or out_ids offset (collect-all fire); decoded to
// the int4 {type, slot | k << 8 (pairwise) / slot (receive) / k (collect-all), y, tick}
__device__ __forceinline__ int4 ev_dec(int2 e) {
  const int ty = e.x & 3, sl = (e.x >> 2) & 31, k = (e.x >> 7) & 31, tk = (int)((unsigned)e.x >> 12);
  return make_int4(ty, ty == FU_EV_FIRE_PW ? (sl | k << 8) : ty == FU_EV_RECV ? sl : k, e.y, tk);
}
template <int MAXD, bool CA>
__global__ __launch_bounds__(kBlock) void k_replay_persist_reg(
    int n, int tick_end, const long long *__restrict__ node_off, const int2 *__restrict__ node_evt,
    const int *__restrict__ out_uid, int n_uid,
    const long long *__restrict__ rowptr, const double *__restrict__ v, double *__restrict__ flow,
    double *__restrict__ est, double *__restrict__ last, unsigned long long *__restrict__ pay,
    long long *__restrict__ cursor, int *__restrict__ scur, int n_snap,
    const int *__restrict__ snap_ticks, double *__restrict__ snaps, int *__restrict__ status,
    long long max_iters) {
  __shared__ int2 s_ring[kRing * kBlock];  // entry k of lane t at k * kBlock + t
  const int node = blockIdx.x * kBlock + threadIdx.x;
  if (node >= n) return;  // (no block barrier below)
  int2 *ring = s_ring + threadIdx.x;
  long long p = cursor[node];
  const long long pe = node_off[node + 1];
  int sc = scur[node];
  const long long rb = rowptr[node];
  const int deg = (int)(rowptr[node + 1] - rb);
  double fl[MAXD], es[MAXD];
#pragma unroll
  for (int j = 0; j < MAXD; ++j) {
    fl[j] = j < deg ? flow[rb + j] : 0.0;
    es[j] = j < deg ? est[rb + j] : 0.0;
  }
  const double val = v[node];
  double lst = last[node];
  // ring: events p .. p + rv - 1 at entries rh, rh + 1, ... (mod kRing); fill = next event to load
  int rh = 0, rv = 0;
  long long fill = p;
  int2 r0, r1, r2, r3, r4, r5, r6, r7;  // the refill in flight (named registers: no private array)
  bool pend = false;
  int pcnt = 0;
#define FU_RING_REFILL()                                                    \
  do {                                                                      \
    const long long lo = max(0ll, pe - 1);                                  \
    r0 = node_evt[max(0ll, min(fill, lo))];                                 \
    r1 = node_evt[max(0ll, min(fill + 1, lo))];                             \
    r2 = node_evt[max(0ll, min(fill + 2, lo))];                             \
    r3 = node_evt[max(0ll, min(fill + 3, lo))];                             \
    r4 = node_evt[max(0ll, min(fill + 4, lo))];                             \
    r5 = node_evt[max(0ll, min(fill + 5, lo))];                             \
    r6 = node_evt[max(0ll, min(fill + 6, lo))];                             \
    r7 = node_evt[max(0ll, min(fill + 7, lo))];                             \
    pcnt = (int)max(0ll, min((long long)kRefill, pe - fill));               \
    fill += kRefill;                                                        \
    pend = true;                                                            \
  } while (0)
#define FU_RING_COMMIT()                                                    \
  do {                                                                      \
    ring[((rh + rv) & (kRing - 1)) * kBlock] = r0;                          \
    ring[((rh + rv + 1) & (kRing - 1)) * kBlock] = r1;                      \
    ring[((rh + rv + 2) & (kRing - 1)) * kBlock] = r2;                      \
    ring[((rh + rv + 3) & (kRing - 1)) * kBlock] = r3;                      \
    ring[((rh + rv + 4) & (kRing - 1)) * kBlock] = r4;                      \
    ring[((rh + rv + 5) & (kRing - 1)) * kBlock] = r5;                      \
    ring[((rh + rv + 6) & (kRing - 1)) * kBlock] = r6;                      \
    ring[((rh + rv + 7) & (kRing - 1)) * kBlock] = r7;                      \
    rv += pcnt;                                                             \
    pend = false;                                                           \
  } while (0)
  static_assert(kRefill == 8, "eight refill registers");
  FU_RING_REFILL();
  FU_RING_COMMIT();
  FU_RING_REFILL();
  FU_RING_COMMIT();
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(pay, 0, 0x7FFFFFF0, 0x00020000);
  const int scratch = n_uid + node;  // this node's scratch slot (idle polls and stores)
  // two polls in flight: the payloads of the lane's next two receives (slots pa, pb)
  unsigned long long ax = kMsgSentinel, ay = kMsgSentinel, bx = kMsgSentinel, by = kMsgSentinel;
  int pa = -1, pb = -1;
  auto ld16 = [&](int msg, unsigned long long &x, unsigned long long &y) {  // 16-byte sc1 load
    const u4 w = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(prs, msg * 16, 0, 16));
    x = (unsigned long long)w.x | ((unsigned long long)w.y << 32);
    y = (unsigned long long)w.z | ((unsigned long long)w.w << 32);
  };
  // a message = one 16-byte sc1 store (write-through, aux 16) of {flow, avg}: one fabric write
  // instead of two 8-byte ones (narrow sc1 stores cost 2.7x per byte, MI355X_MICROARCH.md)
  auto send = [&](int msg, double f, double a) {
    const unsigned long long fb = (unsigned long long)__double_as_longlong(f);
    const unsigned long long ab = (unsigned long long)__double_as_longlong(a);
    const u4 w = {(unsigned)fb, (unsigned)(fb >> 32), (unsigned)ab, (unsigned)(ab >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(w, prs, msg * 16, 0, 16);
  };
  // the slots of the first two receives among the ring's next kScan events (scratch if fewer;
  // scratch is never a message slot)
#define FU_NEXT_RECVS(ida, idb)                                              \
  do {                                                                       \
    ida = idb = scratch;                                                     \
    _Pragma("unroll") for (int j = 0; j < kScan; ++j) {                      \
      const int4 e = ev_dec(ring[((rh + j) & (kRing - 1)) * kBlock]);        \
      if (j < rv && e.w < tick_end && e.x == FU_EV_RECV) {                   \
        if (ida == scratch) ida = e.z;                                       \
        else if (idb == scratch) idb = e.z;                                  \
      }                                                                      \
    }                                                                        \
  } while (0)
  {
    int ia, ib;
    FU_NEXT_RECVS(ia, ib);
    pa = ia;
    ld16(ia, ax, ay);
    pb = ib;
    ld16(ib, bx, by);
    if (!CA) {
      send(scratch, 0.0, 0.0);
      send(scratch, 0.0, 0.0);
    }
  }
  long long it = 0;
  bool done = false;
  for (;;) {
    if (pend) FU_RING_COMMIT();
    const int4 h0 = ev_dec(ring[rh * kBlock]);
    done = rv > 0 ? h0.w >= tick_end : !pend && fill >= pe;
    if (__all(done)) break;
    bool prog = false;
    int o1 = scratch, o2 = scratch;  // the iteration's (at most two) pairwise messages
    double f1 = 0.0, a1 = 0.0, f2 = 0.0, a2 = 0.0;
    if (!done && rv > 0) {
      int m = 0;   // events run this iteration
      int nfo = 0; // pairwise fires this iteration
#pragma unroll
      for (int k = 0; k < kRW; ++k) {
        if (k >= rv) break;
        const int4 ev = k == 0 ? h0 : ev_dec(ring[((rh + k) & (kRing - 1)) * kBlock]);
        const int tk = ev.w;
        if (tk >= tick_end) break;
        unsigned long long mx = 0, my = 0;
        if (ev.x == FU_EV_RECV) {  // its payload must be one of the two polls, arrived
          if (pa == ev.z && ax != kMsgSentinel && ay != kMsgSentinel) {
            mx = ax;
            my = ay;
            pa = -1;
          } else if (pb == ev.z && bx != kMsgSentinel && by != kMsgSentinel) {
            mx = bx;
            my = by;
            pb = -1;
          } else {
            break;  // not arrived (or not polled yet): polled again at the end
          }
        } else if (!CA && nfo == 2) {
          break;  // two pairwise messages per iteration
        }
        while (sc < n_snap && snap_ticks[sc] < tk) snaps[(long long)sc++ * n + node] = lst;
        if (ev.x == FU_EV_RECV) {  // CA:98-99 / PW:98-99
#pragma unroll
          for (int j = 0; j < MAXD; ++j)
            if (j == ev.y) {
              es[j] = __longlong_as_double((long long)my);
              fl[j] = -__longlong_as_double((long long)mx);
            }
        } else if (CA && ev.x == FU_EV_FIRE_CA) {  // CA:105-125
          const int kk = ev.y;
          double S = 0.0, T = 0.0;
#pragma unroll
          for (int j = 0; j < MAXD; ++j)
            if (j < kk) S = S + fl[j];
          const double estimate = val - S;
#pragma unroll
          for (int j = 0; j < MAXD; ++j)
            if (j < kk) T = T + es[j];
          const double avg = (estimate + T) / (double)(kk + 1);
          lst = avg;
#pragma unroll
          for (int j = 0; j < MAXD; ++j)
            if (j < kk) {
              const double nf = (fl[j] + avg) - es[j];
              fl[j] = nf;
              es[j] = avg;
              send(out_uid[ev.z + j], nf, avg);
            }
        } else {  // FIRE_PW, PW:102-117: y = slot | k << 8
          const int sl = ev.y & 0xFF, kk = ev.y >> 8;
          double S = 0.0, fs = 0.0, esl = 0.0;
#pragma unroll
          for (int j = 0; j < MAXD; ++j) {
            if (j < kk) S = S + fl[j];
            if (j == sl) {
              fs = fl[j];
              esl = es[j];
            }
          }
          const double estimate = val - S;
          const double avg = (esl + estimate) / 2.0;
          lst = avg;
          const double nf = (fs + avg) - esl;
#pragma unroll
          for (int j = 0; j < MAXD; ++j)
            if (j == sl) {
              fl[j] = nf;
              es[j] = avg;
            }
          if (CA) {
            send(ev.z, nf, avg);
          } else if (nfo == 0) {
            o1 = ev.z;
            f1 = nf;
            a1 = avg;
          } else {
            o2 = ev.z;
            f2 = nf;
            a2 = avg;
          }
          ++nfo;
        }
        ++m;
      }
      if (m) {
        p += m;
        rh = (rh + m) & (kRing - 1);
        rv -= m;
        prog = true;
      }
    }
    if (!pend && rv <= kRing - kRefill && fill < pe) FU_RING_REFILL();  // lands during the next pass
    {  // the youngest operations, in this order every iteration: two polls, then two stores
      int ia, ib;
      FU_NEXT_RECVS(ia, ib);
      pa = ia;
      ld16(ia, ax, ay);
      pb = ib;
      ld16(ib, bx, by);
      if (!CA) {
        send(o1, f1, a1);
        send(o2, f2, a2);
      }
    }
    if (!__any(prog)) __builtin_amdgcn_s_sleep(kReplaySleep);
    if (++it > max_iters) {  // bounded spin: a bug must end the kernel, not hang the GPU
      atomicExch(status, 1);
      break;
    }
  }
  if (done)
    while (sc < n_snap && snap_ticks[sc] < tick_end) snaps[(long long)sc++ * n + node] = lst;
#pragma unroll
  for (int j = 0; j < MAXD; ++j)
    if (j < deg) {
      flow[rb + j] = fl[j];
      est[rb + j] = es[j];
    }
  cursor[node] = p;
  scur[node] = sc;
  last[node] = lst;
}
#undef FU_RING_REFILL
#undef FU_RING_COMMIT
#undef FU_NEXT_RECVS

// A device buffer of one call, freed on every way out of it.
template <typename T>
struct scoped_dev {
  T *p = nullptr;
  ~scoped_dev() { if (p) (void)hipFree(p); }
};
}  // namespace

// ======================================================================================
// replay
// ======================================================================================
struct fu_replay : stream_base {
  static constexpr const char *kTag = "fu_replay";
  int32_t n = 0, ticks = 0, cur_tick = 0;
  int64_t E = 0, n_msgs = 0;
  std::vector<int64_t> h_tto;
  long long *rowptr = nullptr;
  int *tasks = nullptr, *events = nullptr, *out_ids = nullptr;
  double *v = nullptr, *flow = nullptr, *est = nullptr, *last = nullptr;
  double2 *msg = nullptr;
  // persistent mode (built on first use)
  int persistent = 0;
  unsigned pers_blocks = 1;     // generic persistent launch: the occupancy-derived grid
  int64_t pers_blocks_req = 0;  // option "persistent_blocks" (tests): 0 = pers_blocks
  std::vector<int32_t> h_tasks, h_events, h_out_ids;
  long long *node_off = nullptr, *cursor = nullptr;
  int4 *node_ev = nullptr;
  int2 *node_evt = nullptr;  // register kernel: packed 8-byte events (ev_dec)
  int *node_tick = nullptr, *out_uid = nullptr, *scur = nullptr, *status = nullptr;
  unsigned long long *pay = nullptr;
  int64_t n_uid = 0;
  bool pers_ready = false;
  int64_t max_deg = 0;
  int pers_reg = 1;       // option "persistent_reg": one node per thread, state in registers
  bool reg_ok = false;    // degree <= kReplayRegDeg and every node's thread resident at once
  bool has_ca = false;    // the trace holds collect-all fires
};
constexpr int kReplayRegDeg = 16;

// The register variant for the trace: row registers for degree <= 8 or <= 16, the collect-all
// fire path only when the trace has one (both cost registers, and the variant must keep
// every node's thread resident).
using ReplayRegKernel = void (*)(int, int, const long long *, const int2 *, const int *, int,
                                 const long long *, const double *, double *, double *, double *,
                                 unsigned long long *, long long *, int *, int, const int *, double *, int *,
                                 long long);
static ReplayRegKernel replay_reg_kernel(const fu_replay *r) {
  if (r->max_deg <= 8) return r->has_ca ? k_replay_persist_reg<8, true> : k_replay_persist_reg<8, false>;
  return r->has_ca ? k_replay_persist_reg<16, true> : k_replay_persist_reg<16, false>;
}

// Blocks of the generic persistent launch. "persistent_blocks" can only lower the grid
// (fewer threads, more nodes each), never raise it above the resident bound.
static unsigned replay_pers_blocks(const fu_replay *r) {
  return r->pers_blocks_req > 0 ? (unsigned)std::min<int64_t>(r->pers_blocks, r->pers_blocks_req) : r->pers_blocks;
}

static int replay_build_persistent(fu_replay *r) {
  if (r->pers_ready) return FU_OK;
  if (int rc = set_device(r)) return rc;
  const int32_t n = r->n;
  const int64_t nt = (int64_t)r->h_tasks.size() / 3, ne = (int64_t)r->h_events.size() / 4;
  std::vector<int64_t> off(n + 1, 0);
  for (int64_t q = 0; q < nt; ++q) off[r->h_tasks[3 * q] + 1] += r->h_tasks[3 * q + 2] - r->h_tasks[3 * q + 1];
  for (int32_t i = 0; i < n; ++i) off[i + 1] += off[i];
  std::vector<int64_t> pos(off.begin(), off.end() - 1);
  std::vector<int4> nev(ne > 0 ? ne : 1);
  std::vector<int32_t> ntick(ne > 0 ? ne : 1);
  std::vector<int2> nevt(ne > 0 ? ne : 1);
  bool pack_ok = r->ticks < (1 << 20);  // the register kernel's 8-byte events: tick < 2^20, slot, k < 32
  std::vector<int32_t> ouid(r->h_out_ids.size() > 0 ? r->h_out_ids.size() : 1);
  std::vector<int64_t> slot_uid(r->n_msgs > 0 ? r->n_msgs : 1, -1);
  int64_t U = 0;
  for (int32_t t = 0; t < r->ticks; ++t) {
    for (int64_t q = r->h_tto[t]; q < r->h_tto[t + 1]; ++q) {
      const int32_t node = r->h_tasks[3 * q];
      for (int32_t p = r->h_tasks[3 * q + 1]; p < r->h_tasks[3 * q + 2]; ++p) {
        const int32_t *e = &r->h_events[4 * (int64_t)p];
        int4 o = make_int4(e[0], e[1], e[2], e[3]);
        if (e[0] == FU_EV_RECV) {
          const int64_t u = slot_uid[e[2]];
          if (u < 0) return fail(FU_ERR_ARG, "replay: RECV of a message slot never written");
          o.z = (int)u;
        } else if (e[0] == FU_EV_FIRE_CA) {
          for (int32_t j = 0; j < e[1]; ++j) {
            slot_uid[r->h_out_ids[e[2] + j]] = U;
            ouid[e[2] + j] = (int32_t)U++;
          }
        } else {
          slot_uid[e[3]] = U;
          o.w = (int)U++;
        }
        if (U >= (int64_t)INT32_MAX) return fail(FU_ERR_ALLOC, "replay: more than 2^31 messages");
        nev[pos[node]] = o;
        {
          const int sl = o.x == FU_EV_FIRE_CA ? 0 : o.y;
          const int kk = o.x == FU_EV_FIRE_CA ? o.y : o.x == FU_EV_FIRE_PW ? o.z : 0;
          pack_ok &= sl < 32 && kk < 32;
          nevt[pos[node]] = make_int2((int)((unsigned)o.x | (unsigned)(sl & 31) << 2 | (unsigned)(kk & 31) << 7 |
                                            (unsigned)t << 12),
                                      o.x == FU_EV_FIRE_PW ? o.w : o.z);
        }
        ntick[pos[node]++] = t;
      }
    }
  }
  r->n_uid = U;
  int rc;
  // pay's slots [U, U + n): per-node scratch slots of the register kernel's idle polls and stores
  if ((rc = dmalloc(r, &r->node_off, (int64_t)n + 1)) || (rc = dmalloc(r, &r->node_ev, nev.size())) ||
      (rc = dmalloc(r, &r->node_tick, ntick.size())) || (rc = dmalloc(r, &r->node_evt, nevt.size())) ||
      (rc = dmalloc(r, &r->out_uid, ouid.size())) || (rc = dmalloc(r, &r->pay, 2 * (U + n))) ||
      (rc = dmalloc(r, &r->cursor, n)) || (rc = dmalloc(r, &r->scur, n)) || (rc = dmalloc(r, &r->status, 1)))
    return rc;
  if ((rc = put(r, r->node_off, off.data(), (int64_t)n + 1)) || (rc = put(r, r->node_ev, nev.data(), nev.size())) ||
      (rc = put(r, r->node_tick, ntick.data(), ntick.size())) || (rc = put(r, r->node_evt, nevt.data(), nevt.size())) ||
      (rc = put(r, r->out_uid, ouid.data(), ouid.size())) || (rc = put(r, r->cursor, off.data(), n)) ||
      (rc = zero(r, r->scur, n)))
    return rc;
  double sentinel;
  std::memcpy(&sentinel, &kMsgSentinel, sizeof(double));
  hipLaunchKernelGGL(k_fill, dim3(grid_for(2 * (U + n))), dim3(kBlock), 0, r->stream,
                     (long long)(2 * (U + n)), sentinel, reinterpret_cast<double *>(r->pay));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(r->stream));
  int per_cu = 0, ncu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_replay_persist, kBlock, 0));
  HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, r->device));
  // stay below the occupancy bound (the API can over-report by one block per CU)
  const long long cap = std::max(1LL, (long long)std::max(1, per_cu - 1) * ncu);
  r->pers_blocks = (unsigned)std::min<long long>(cap, grid_for(r->n));
  // the register variant needs one resident thread per node (a node's blocked receive is
  // retried by its own thread only)
  int per_cu_reg = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_reg, replay_reg_kernel(r), kBlock, 0));
  const long long cap_reg = (long long)std::max(0, per_cu_reg - 1) * ncu;
  // (and 16-byte payload polls at 32-bit byte offsets: below 2^27 messages)
  r->reg_ok = r->max_deg <= kReplayRegDeg && (long long)grid_for(r->n) <= cap_reg && U + n < (1LL << 27) && pack_ok;
  r->pers_ready = true;
  return FU_OK;
}

extern "C" {
int fu_replay_create(int32_t n, const int64_t *rowptr, const double *value, int32_t ticks,
                     const int64_t *tick_task_off, int64_t n_tasks, const int32_t *tasks,
                     int64_t n_events, const int32_t *events, int64_t n_out_ids,
                     const int32_t *out_ids, int64_t n_msgs, int32_t device,
                     fu_replay **out) {
  FU_TRY_BEGIN
  if (!out || n <= 0 || !rowptr || !value || ticks < 0 || !tick_task_off || n_tasks < 0 || n_events < 0 ||
      n_out_ids < 0 || n_msgs < 0 || (n_tasks > 0 && !tasks) || (n_events > 0 && !events) || (n_out_ids > 0 && !out_ids))
    return bad_arguments<fu_replay>("create");
  if (tick_task_off[0] != 0 || tick_task_off[ticks] != n_tasks) return fail(FU_ERR_ARG, "fu_replay_create: tick_task_off inconsistent");
  const int64_t E = rowptr[n];
  bool has_ca = false;
  // validate the trace on the host: every index a kernel will dereference
  for (int64_t q = 0; q < n_tasks; ++q) {
    int32_t node = tasks[3 * q], b = tasks[3 * q + 1], e = tasks[3 * q + 2];
    if (node < 0 || node >= n || b < 0 || e < b || e > n_events) return fail(FU_ERR_ARG, "fu_replay_create: bad task " + std::to_string(q));
    const int64_t deg = rowptr[node + 1] - rowptr[node];
    for (int32_t p = b; p < e; ++p) {
      const int32_t *ev = events + 4 * (int64_t)p;
      bool ok;
      if (ev[0] == FU_EV_RECV) ok = ev[1] >= 0 && ev[1] < deg && ev[2] >= 0 && ev[2] < n_msgs;
      else if (ev[0] == FU_EV_FIRE_CA) ok = ev[1] >= 0 && ev[1] <= deg && ev[2] >= 0 && (int64_t)ev[2] + ev[1] <= n_out_ids;
      else if (ev[0] == FU_EV_FIRE_PW) ok = ev[1] >= 0 && ev[1] < deg && ev[2] > ev[1] && ev[2] <= deg && ev[3] >= 0 && ev[3] < n_msgs;
      else ok = false;
      if (!ok) return fail(FU_ERR_ARG, "fu_replay_create: bad event " + std::to_string(p));
      has_ca |= ev[0] == FU_EV_FIRE_CA;
    }
  }
  for (int64_t q = 0; q < n_out_ids; ++q)
    if (out_ids[q] < 0 || out_ids[q] >= n_msgs) return fail(FU_ERR_ARG, "fu_replay_create: bad out_id");
  auto *r = new fu_replay();
  auto cleanup = [&](int code) { fu_replay_destroy(r); return code; };
  r->n = n;
  r->ticks = ticks;
  r->E = E;
  r->n_msgs = n_msgs;
  r->has_ca = has_ca;
  for (int32_t i = 0; i < n; ++i) r->max_deg = std::max<int64_t>(r->max_deg, rowptr[i + 1] - rowptr[i]);
  r->h_tto.assign(tick_task_off, tick_task_off + ticks + 1);
  r->h_tasks.assign(tasks, tasks + 3 * n_tasks);
  r->h_events.assign(events, events + 4 * n_events);
  r->h_out_ids.assign(out_ids, out_ids + n_out_ids);
  int rc;
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  if ((rc = stream_open(r, device)) || (rc = dmalloc(r, &r->rowptr, (int64_t)n + 1)) ||
      (rc = dmalloc(r, &r->tasks, 3 * n_tasks)) || (rc = dmalloc(r, &r->events, 4 * n_events)) ||
      (rc = dmalloc(r, &r->out_ids, n_out_ids)) || (rc = dmalloc(r, &r->v, n)) || (rc = dmalloc(r, &r->flow, E)) ||
      (rc = dmalloc(r, &r->est, E)) || (rc = dmalloc(r, &r->last, n)) || (rc = dmalloc(r, &r->msg, n_msgs)) ||
      (rc = put(r, r->rowptr, rowptr, (int64_t)n + 1)) || (rc = put(r, r->tasks, tasks, 3 * n_tasks)) ||
      (rc = put(r, r->events, events, 4 * n_events)) || (rc = put(r, r->out_ids, out_ids, n_out_ids)) ||
      (rc = put(r, r->v, value, n)) || (rc = zero(r, r->flow, std::max<int64_t>(E, 1))) ||
      (rc = zero(r, r->est, std::max<int64_t>(E, 1))) || (rc = zero(r, r->last, n)) ||
      (rc = zero(r, r->msg, std::max<int64_t>(n_msgs, 1))))
    return cleanup(rc);
  *out = r;
  return FU_OK;
  FU_TRY_END
}

const fu_trace *fu__trace_view(const fu_trace *t, int32_t *n, int32_t *ticks,
                               const int64_t **urowptr, const int64_t **tto,
                               const int32_t **tasks, int64_t *n_tasks,
                               const int32_t **events, int64_t *n_events,
                               const int32_t **out_ids, int64_t *n_out, int64_t *n_msgs);

int fu_replay_create_from_trace(const fu_trace *t, const double *value, int32_t device,
                                fu_replay **out) {
  FU_TRY_BEGIN
  if (!t) return fail(FU_ERR_ARG, "fu_replay_create_from_trace: NULL trace");
  int32_t n, ticks;
  const int64_t *urp, *tto;
  const int32_t *tasks, *events, *oids;
  int64_t nt, ne, no, nm;
  fu__trace_view(t, &n, &ticks, &urp, &tto, &tasks, &nt, &events, &ne, &oids, &no, &nm);
  return fu_replay_create(n, urp, value, ticks, tto, nt, tasks, ne, events, no, oids, nm, device, out);
  FU_TRY_END
}

static int replay_ticks(fu_replay *r, int32_t tick_end, int32_t n_snap, const int32_t *snap_ticks,
                        double *snaps_dev) {
  if (r->persistent) {
    if (r->cur_tick > 0 && !r->pers_ready) return fail(FU_ERR_STATE, "replay: cannot switch to persistent mode mid-run");
    if (int rc = replay_build_persistent(r)) return rc;
    scoped_dev<int32_t> d_st;
    if (n_snap > 0) {
      if (int rc = dmalloc(r, &d_st.p, n_snap)) return rc;
      HIP_TRY(hipMemcpyAsync(d_st.p, snap_ticks, sizeof(int32_t) * n_snap, hipMemcpyHostToDevice, r->stream));
    }
    HIP_TRY(hipMemsetAsync(r->scur, 0, sizeof(int) * r->n, r->stream));
    HIP_TRY(hipMemsetAsync(r->status, 0, sizeof(int), r->stream));
    if (r->reg_ok && r->pers_reg)
      hipLaunchKernelGGL(replay_reg_kernel(r), dim3(grid_for(r->n)), dim3(kBlock), 0, r->stream,
                         r->n, tick_end, r->node_off, r->node_evt, r->out_uid, (int)r->n_uid, r->rowptr, r->v,
                         r->flow, r->est, r->last, r->pay, r->cursor, r->scur, n_snap, d_st.p, snaps_dev, r->status,
                         (long long)1 << 22);
    else
      hipLaunchKernelGGL(k_replay_persist, dim3(replay_pers_blocks(r)), dim3(kBlock), 0, r->stream, r->n, tick_end,
                         r->node_off, r->node_ev, r->node_tick, r->out_uid, r->rowptr, r->v, r->flow,
                         r->est, r->last, r->pay, r->cursor, r->scur, n_snap, d_st.p, snaps_dev, r->status,
                         (long long)1 << 22);
    HIP_TRY(hipGetLastError());
    int st = 0;
    HIP_TRY(hipMemcpyAsync(&st, r->status, sizeof(int), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (st) return fail(FU_ERR_STATE, "replay: persistent kernel hit its iteration bound");
    r->cur_tick = tick_end;
    return FU_OK;
  }
  int32_t si = 0;
  while (si < n_snap && snap_ticks[si] < r->cur_tick) ++si;
  for (int32_t t = r->cur_tick; t < tick_end; ++t) {
    const long long b = r->h_tto[t];
    const int cnt = (int)(r->h_tto[t + 1] - b);
    if (cnt > 0) {
      hipLaunchKernelGGL(k_replay_tick, dim3(grid_for(cnt)), dim3(kBlock), 0, r->stream, b, cnt,
                         r->tasks, r->rowptr, r->events, r->out_ids, r->v, r->flow, r->est,
                         r->last, r->msg);
      HIP_TRY(hipGetLastError());
    }
    while (si < n_snap && snap_ticks[si] == t) {
      HIP_TRY(hipMemcpyAsync(snaps_dev + (int64_t)si * r->n, r->last, sizeof(double) * r->n,
                             hipMemcpyDeviceToDevice, r->stream));
      ++si;
    }
  }
  r->cur_tick = tick_end;
  return FU_OK;
}

int fu_replay_run(fu_replay *r, int32_t tick_end, int32_t n_snap, const int32_t *snap_ticks,
                  double *snaps) {
  FU_TRY_BEGIN
  if (!r || tick_end < r->cur_tick || tick_end > r->ticks || n_snap < 0 || (n_snap > 0 && (!snap_ticks || !snaps)))
    return fail(FU_ERR_ARG, "fu_replay_run: bad arguments");
  for (int32_t k = 1; k < n_snap; ++k)
    if (snap_ticks[k] <= snap_ticks[k - 1]) return fail(FU_ERR_ARG, "fu_replay_run: snap_ticks must be ascending");
  HIP_TRY(hipSetDevice(r->device));
  scoped_dev<double> d_snaps;
  if (n_snap > 0) {
    if (int rc = dmalloc(r, &d_snaps.p, (int64_t)n_snap * r->n)) return rc;
    HIP_TRY(hipMemsetAsync(d_snaps.p, 0, sizeof(double) * n_snap * r->n, r->stream));
  }
  int rc = replay_ticks(r, tick_end, n_snap, snap_ticks, d_snaps.p);
  if (rc == FU_OK && n_snap > 0) {
    if (hipMemcpyAsync(snaps, d_snaps.p, sizeof(double) * n_snap * r->n, hipMemcpyDeviceToHost, r->stream) != hipSuccess)
      rc = fail(FU_ERR_HIP, "fu_replay_run: snapshot copy failed");
  }
  if (hipStreamSynchronize(r->stream) != hipSuccess && rc == FU_OK) rc = fail(FU_ERR_HIP, "fu_replay_run: sync failed");
  return rc;
  FU_TRY_END
}

int fu_replay_run_timed(fu_replay *r, int32_t tick_end, float *ms) {
  FU_TRY_BEGIN
  if (!r || !ms || tick_end < r->cur_tick || tick_end > r->ticks) return fail(FU_ERR_ARG, "fu_replay_run_timed: bad arguments");
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(hipEventRecord(r->ev0, r->stream));
  if (int rc = replay_ticks(r, tick_end, 0, nullptr, nullptr)) return rc;
  HIP_TRY(hipEventRecord(r->ev1, r->stream));
  HIP_TRY(hipEventSynchronize(r->ev1));
  HIP_TRY(hipEventElapsedTime(ms, r->ev0, r->ev1));
  return FU_OK;
  FU_TRY_END
}

int fu_replay_get(fu_replay *r, double *last_avg, double *flows, double *est) {
  FU_TRY_BEGIN
  if (!r) return fail(FU_ERR_ARG, "fu_replay_get: NULL replay");
  int rc = last_avg ? download(r, last_avg, r->last, sizeof(double) * r->n) : FU_OK;
  if (!rc && flows) rc = download(r, flows, r->flow, sizeof(double) * r->E);
  return !rc && est ? download(r, est, r->est, sizeof(double) * r->E) : rc;
  FU_TRY_END
}

int fu_replay_set_option(fu_replay *r, const char *key, int64_t value) {
  FU_TRY_BEGIN
  if (!r || !key) return fail(FU_ERR_ARG, "fu_replay_set_option: NULL argument");
  if (!std::strcmp(key, "persistent")) {
    if (r->cur_tick != 0) return fail(FU_ERR_STATE, "fu_replay_set_option: persistent must be set before the first tick");
    r->persistent = value != 0;
    if (!r->persistent) return FU_OK;
    // build the per-node event lists now, so that no host work lands inside a timed run
    return replay_build_persistent(r);
  }
  if (!std::strcmp(key, "persistent_reg")) {  // persistent mode: node state in registers (1, default)
    r->pers_reg = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "persistent_blocks")) {  // tests: blocks of the generic persistent launch
    if (value < 0) return fail(FU_ERR_ARG, "fu_replay_set_option: persistent_blocks must be >= 0");
    if (r->cur_tick != 0) return fail(FU_ERR_STATE, "fu_replay_set_option: persistent_blocks must be set before the first tick");
    r->pers_blocks_req = value;
    return FU_OK;
  }
  return fail(FU_ERR_ARG, std::string("fu_replay_set_option: unknown key '") + key + "'");
  FU_TRY_END
}

int fu_replay_get_info(fu_replay *r, int64_t info[8]) {
  FU_TRY_BEGIN
  if (!r || !info) return fail(FU_ERR_ARG, "fu_replay_get_info: NULL argument");
  if (r->persistent)
    if (int rc = replay_build_persistent(r)) return rc;
  const bool reg = r->persistent && r->pers_ready && r->reg_ok && r->pers_reg;
  info[0] = r->persistent;
  info[1] = reg;
  info[2] = reg ? (r->max_deg <= 8 ? 8 : 16) : 0;
  info[3] = r->has_ca;
  info[4] = r->pers_ready ? (int64_t)replay_pers_blocks(r) : 0;
  info[5] = r->pers_ready ? r->n_uid : 0;
  info[6] = r->max_deg;
  info[7] = r->cur_tick;
  return FU_OK;
  FU_TRY_END
}

int fu_replay_destroy(fu_replay *r) {
  if (!r) return FU_OK;
  stream_close(r, {r->rowptr, r->tasks, r->events, r->out_ids, r->v, r->flow, r->est, r->last, r->msg, r->node_off,
                   r->cursor, r->node_ev, r->node_evt, r->node_tick, r->out_uid, r->scur, r->status, r->pay});
  delete r;
  return FU_OK;
}

}  // extern "C"
