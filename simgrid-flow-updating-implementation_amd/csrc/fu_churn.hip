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
// This file holds the churn rule (the state byte is the slot's kind: UP gathers, DOWN is
// skipped, FRESH is kZero and turns UP at write-out; a dead row does not fire), the topology
// pass; the error check over alive nodes is the scaffold's k_max_err_alive. The round itself
// (the kernels, the launch plan, the common buffers, the front half of create) is
// csrc/fu_rev_round.h, shared with the lossy engine; the handle scaffold under it is
// csrc/fu_handle.h.
#include "fu_rev_round.h"

using namespace fu;

namespace {

constexpr unsigned char kUp = 0, kDown = 1, kFresh = 2;
static_assert(kUp == kGather && kDown == kSkip && kFresh == kZero, "the state byte is the slot's kind");

struct churn_rule {
  struct Args {
    const unsigned char *alive;
    unsigned char *state;
  };
  static constexpr bool kHasOwn = false, kHasSkip = true, kDeadRows = true;
  template <int N>
  __device__ static void classify(const Args &X, const i64 (&k)[N], unsigned char (&kind)[N]) {
#pragma unroll
    for (int u = 0; u < N; ++u) kind[u] = X.state[k[u]];
  }
  __device__ static bool fires(const Args &X, int row) { return X.alive[row] != 0; }
  __device__ static void wrote(const Args &X, i64 k, unsigned char kind) {
    if (kind == kFresh) X.state[k] = kUp;
  }
  __device__ static void block_end(const Args &, int &) {}
};

// fu_churn_set_topology and fu_churn_reset: one pass over the slots, from the uploaded alive
// and link_up and the old state byte to the new one. Slot k's row is col[rev k]. A slot that is
// not live loses its K flow entries in `f` (f[k * K ..]), the buffer the next round reads. all_fresh (reset):
// every live slot ends FRESH. count[0] += alive nodes, count[1] += live slots, one atomic per
// block and counter.
__global__ __launch_bounds__(kBlock) void kc_topology(int n, i64 E, const int *__restrict__ col, const int *__restrict__ rev,
                                                      const unsigned char *__restrict__ alive,
                                                      const unsigned char *__restrict__ link_up, unsigned char *__restrict__ state,
                                                      double *__restrict__ f, int K, int all_fresh, u64 *__restrict__ count) {
  const i64 k = (i64)blockIdx.x * kBlock + threadIdx.x;
  int live = 0;
  if (k < E) {
    live = link_up[k] != 0 && alive[col[rev[k]]] != 0 && alive[col[k]] != 0;
    if (live) {
      if (all_fresh || state[k] == kDown) state[k] = kFresh;
    } else {
      state[k] = kDown;
      for (int c = 0; c < K; ++c) f[k * K + c] = 0.0;
    }
  }
  int up = k < n && alive[k] != 0;
  block_count_to<kBlock>(up, count);
  __syncthreads();  // block_count_to's wave sums are one LDS array: the first call has read it
  block_count_to<kBlock>(live, count + 1);
}

}  // namespace

struct fu_churn : rev_handle {
  static constexpr const char *kTag = "fu_churn";
  unsigned char *alive = nullptr, *link_up = nullptr, *state = nullptr;
  u64 *count = nullptr;
  std::vector<int32_t> h_rev;  // host copy: the symmetry check of link_up
  int64_t stats[2] = {0, 0};   // alive nodes, live slots of the current topology
};

static int launch_err(fu_churn *h, u64 *slot) {
  if (h->width > 1) return launch_max_err_cols(h, h->alive, slot);
  return launch_max_err_alive<kBlock>(h, h->a[(h->round + 1) & 1], h->alive, slot);  // a of the last round run
}

static int launch_round(fu_churn *h) { return launch_rev_round<churn_rule>(h, {h->alive, h->state}); }

// The state bytes from the device's alive and link_up, behind the rounds already queued;
// complete on return, with the counts in h->stats.
static int apply_topology(fu_churn *h, bool all_fresh) {
  const int64_t work = std::max<int64_t>(h->E, h->n);
  HIP_TRY(hipMemsetAsync(h->count, 0, 2 * sizeof(u64), h->stream));
  hipLaunchKernelGGL(kc_topology, dim3((unsigned)((work + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->n, (i64)h->E,
                     h->col, h->rev, h->alive, h->link_up, h->state, h->f[(h->round + 1) & 1], h->width, all_fresh ? 1 : 0, h->count);
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
  rev_close(h, {h->alive, h->link_up, h->state, h->count});
  delete h;
  return FU_OK;
}

// The back half of both creates: the topology and the slot states, per node and per slot.
static int churn_create(const char *entry, int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                        int32_t k, const double *value, int32_t device, fu_churn **out) {
  FU_TRY_BEGIN
  fu_churn *h = nullptr;
  std::vector<int32_t> built;
  auto cleanup = [&](int code) { if (h) fu_churn_destroy(h); return code; };
  int rc = rev_create(&h, out, entry, n, e, rowptr, col, &rev, &built, k, value, device);
  if (rc || (rc = dmalloc(h, &h->alive, n)) || (rc = dmalloc(h, &h->link_up, e)) || (rc = dmalloc(h, &h->state, e)) ||
      (rc = dmalloc(h, &h->count, 2)))
    return cleanup(rc);
  if (e > 0) h->h_rev.assign(rev, rev + e);
  // everything alive and up, every slot FRESH
  const size_t e1 = (size_t)std::max<int64_t>(e, 1);
  if (hipMemset(h->alive, 1, (size_t)n) != hipSuccess || hipMemset(h->link_up, 1, e1) != hipSuccess ||
      hipMemset(h->state, kFresh, e1) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_churn_create: memset failed"));
  h->stats[0] = n;
  h->stats[1] = e;
  *out = h;
  return FU_OK;
  FU_TRY_END
}

int fu_churn_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                    const double *value, int32_t device, fu_churn **out) {
  return churn_create("create", n, e, rowptr, col, rev, 1, value, device, out);
}

int fu_churn_create_k(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev, int32_t k,
                      const double *value, int32_t device, fu_churn **out) {
  return churn_create("create_k", n, e, rowptr, col, rev, k, value, device, out);
}

int fu_churn_create_from_graph(const fu_graph *g, const double *value, int32_t device, fu_churn **out) {
  return create_from_graph<fu_churn>(g, value, out, [&](auto... csr) { return fu_churn_create(csr..., value, device, out); });
}

int fu_churn_create_from_graph_k(const fu_graph *g, int32_t k, const double *value, int32_t device, fu_churn **out) {
  FU_TRY_BEGIN
  if (g && value && out && (k < 1 || k > kMaxCols))  // after the null checks, before the graph's
    return fail(FU_ERR_ARG, "fu_churn_create_from_graph_k: k must be in 1..16, got " + std::to_string(k));
  return create_from_graph<fu_churn>(g, value, out, [&](auto... csr) { return fu_churn_create_k(csr..., k, value, device, out); });
  FU_TRY_END
}

int fu_churn_get_columns(fu_churn *h, int32_t *k) { return get_columns(h, k); }

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

int fu_churn_set_values(fu_churn *h, const double *value) { return set_values(h, value); }

// Dead nodes keep their estimate and DOWN slots their +0.0 from round to round, so the
// buffers are zeroed here and round 0 is an ordinary round.
int fu_churn_reset(fu_churn *h) {
  FU_TRY_BEGIN
  if (!h) return bad_arguments<fu_churn>("reset");
  if (int rc = set_device(h)) return rc;
  for (int q = 0; q < 2; ++q) {
    HIP_TRY(hipMemsetAsync(h->a[q], 0, sizeof(double) * (size_t)h->n * h->width, h->stream));
    HIP_TRY(hipMemsetAsync(h->f[q], 0, sizeof(double) * (size_t)std::max<int64_t>(h->E * h->width, 1), h->stream));
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

// reset zeroes the buffers: before round 0 they download like after any round.
int fu_churn_get_estimates(fu_churn *h, double *a_out) { return get_estimates(h, a_out, /*zero_before_round_0=*/false); }
int fu_churn_get_flows(fu_churn *h, double *f_out) { return get_flows(h, f_out, /*zero_before_round_0=*/false); }

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
  std::vector<int32_t> built;
  if (int rc = pairing_rev("fu_churn_live", n, e, rowptr, col, &rev, &built)) return rc;
  if (int rc = check_link_up("fu_churn_live", e, rev, link_up)) return rc;
  for (int32_t i = 0; i < n; ++i)
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      live_out[k] = (!link_up || link_up[k] != 0) && (!alive || (alive[i] != 0 && alive[col[k]] != 0));
  return FU_OK;
  FU_TRY_END
}

}  // extern "C"
