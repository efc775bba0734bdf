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
// This file holds the loss rule (a lost slot is kOwn, round 0's slots are kZero), the loss
// decision, the link mask and the lost-message counter. The round itself (the kernels, the
// launch plan, the common buffers, the front half of create) is csrc/fu_rev_round.h, shared
// with the churn engine; the handle scaffold under it is csrc/fu_handle.h.
#include "fu_rev_round.h"

using namespace fu;

namespace {

// The key of round r's decisions, and the decision itself: the kernels and
// fu_lossy_delivered share both. The compare is fp64 on both sides.
FU_HD inline uint64_t round_key(uint64_t seed, uint64_t r) { return splitmix_at(seed, r); }
FU_HD inline bool slot_lost(uint64_t key, uint64_t k, double p) { return u01(splitmix_at(key, k)) < p; }

struct lossy_rule {
  struct Args {
    const unsigned char *down;  // may be null
    u64 *lost;                  // the handle's lost-message counter
    uint64_t key;               // round_key(seed, r)
    double p;
    int zero;  // round 0: the timeout fire on zero state, whatever the buffers hold
  };
  static constexpr bool kHasOwn = true, kHasSkip = false, kDeadRows = false;
  template <int N>
  __device__ static void classify(const Args &X, const i64 (&k)[N], unsigned char (&kind)[N]) {
    bool lost[N] = {};
    if (X.down != nullptr) {
#pragma unroll
      for (int u = 0; u < N; ++u) lost[u] = X.down[k[u]] != 0;
    }
    if (X.p > 0.0) {
#pragma unroll
      for (int u = 0; u < N; ++u) lost[u] = lost[u] || slot_lost(X.key, (uint64_t)k[u], X.p);
    }
#pragma unroll
    for (int u = 0; u < N; ++u) kind[u] = X.zero ? kZero : lost[u] ? kOwn : kGather;
  }
  __device__ static void wrote(const Args &, i64, unsigned char) {}
  // one atomic per block that lost something; round 0 has no kOwn slot and counts nothing
  __device__ static void block_end(const Args &X, int &own_slots) { block_count_to<kBlock>(own_slots, X.lost); }
};

}  // namespace

struct fu_lossy : rev_handle {
  static constexpr const char *kTag = "fu_lossy";
  double p = 0.0;
  uint64_t seed = 0;
  bool has_mask = false;
  unsigned char *down = nullptr;
  u64 *lost = nullptr;
};

static int launch_err(fu_lossy *h, u64 *slot) {
  if (h->width > 1) return launch_max_err_cols(h, nullptr, slot);
  return launch_max_err<kBlock>(h, h->a[(h->round + 1) & 1], slot);  // a of the last round run
}

static int launch_round(fu_lossy *h) {
  const uint64_t r = (uint64_t)h->round;
  return launch_rev_round<lossy_rule>(h, {h->has_mask ? h->down : nullptr, h->lost, round_key(h->seed, r), h->p, r == 0});
}

extern "C" {

int fu_lossy_destroy(fu_lossy *h) {
  if (!h) return bad_arguments<fu_lossy>("destroy");
  rev_close(h, {h->down, h->lost});
  delete h;
  return FU_OK;
}

// The back half of both creates: the mask buffer and the lost-message counter, per slot.
static int lossy_create(const char *entry, int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                        int32_t k, const double *value, int32_t device, fu_lossy **out) {
  FU_TRY_BEGIN
  fu_lossy *h = nullptr;
  std::vector<int32_t> built;
  int rc = rev_create(&h, out, entry, n, e, rowptr, col, &rev, &built, k, value, device);
  if (rc || (rc = dmalloc(h, &h->down, e)) || (rc = dmalloc(h, &h->lost, 1)) || (rc = zero(h, h->lost, 1))) {
    if (h) fu_lossy_destroy(h);
    return rc;
  }
  *out = h;
  return FU_OK;
  FU_TRY_END
}

int fu_lossy_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                    const double *value, int32_t device, fu_lossy **out) {
  return lossy_create("create", n, e, rowptr, col, rev, 1, value, device, out);
}

int fu_lossy_create_k(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col, const int32_t *rev, int32_t k,
                      const double *value, int32_t device, fu_lossy **out) {
  return lossy_create("create_k", n, e, rowptr, col, rev, k, value, device, out);
}

int fu_lossy_create_from_graph(const fu_graph *g, const double *value, int32_t device, fu_lossy **out) {
  return create_from_graph<fu_lossy>(g, value, out, [&](auto... csr) { return fu_lossy_create(csr..., value, device, out); });
}

int fu_lossy_create_from_graph_k(const fu_graph *g, int32_t k, const double *value, int32_t device, fu_lossy **out) {
  FU_TRY_BEGIN
  if (g && value && out && (k < 1 || k > kMaxCols))  // after the null checks, before the graph's
    return fail(FU_ERR_ARG, "fu_lossy_create_from_graph_k: k must be in 1..16, got " + std::to_string(k));
  return create_from_graph<fu_lossy>(g, value, out, [&](auto... csr) { return fu_lossy_create_k(csr..., k, value, device, out); });
  FU_TRY_END
}

int fu_lossy_get_columns(fu_lossy *h, int32_t *k) { return get_columns(h, k); }

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

int fu_lossy_set_values(fu_lossy *h, const double *value) { return set_values(h, value); }
// Round 0 reads no state and reset leaves the buffers as they are: before round 0 the zero
// state is written here, without touching the device.
int fu_lossy_get_estimates(fu_lossy *h, double *a_out) { return get_estimates(h, a_out, /*zero_before_round_0=*/true); }
int fu_lossy_get_flows(fu_lossy *h, double *f_out) { return get_flows(h, f_out, /*zero_before_round_0=*/true); }

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
