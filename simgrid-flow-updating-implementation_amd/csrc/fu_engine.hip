// libfu device engine for MI355X (gfx950): the collect-all engine's translation unit. Its round
// kernels, handle, layouts and launchers are the fu_ca_*.h pieces included below; this file
// holds the autotuner and the C entry points (the tick replay is fu_replay.hip). C ABI
// declared in include/fu.h.
//
// Arithmetic spec (bitwise parity with the reference's Python floats):
//   receive  (flowupdating-collectall.py:98-99):  fr[e] = -f_old[rev e], er[e] = a_old[col e]
//   fire     (CA:106-119):  S = 0.0 + fr[e0] + fr[e1] + ...  (left to right, row order)
//                           T = 0.0 + er[e0] + er[e1] + ...
//                           a = ((v - S) + T) / (deg + 1)
//                           f_new[e] = (fr[e] + a) - er[e]
// Compiled with -ffp-contract=off and without fast-math. There are no multiplies to
// contract, and `/` is the correctly rounded IEEE fp64 division. Every sum is a sequential
// dependency chain in row order, including for hubs (k_round_recon's heavy rows and mega
// hubs, fu_ca_recon.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

// The pieces, in dependency order (each includes only earlier ones): every kernel of the
// collect-all engine is compiled here, once.
#include "fu_ca_pack.h"       // PackCtl, the code helpers, k_pack_plan
#include "fu_ca_recon.h"      // kernel 4: round 0, chains, k_round_recon, hubs, k_max_err
#include "fu_ca_stage.h"      // kernel 8: k_stage, k_round_staged
#include "fu_ca_pregather.h"  // kernel 9: k_transpose, k_isolated, k_heavy_multi, k_lag_final
#include "fu_ca_handle.h"     // struct fu_handle, RoundCtx, the fu__dist_* hooks
#include "fu_ca_layout.h"     // tiles, hubs, slices and buckets onto the device
#include "fu_ca_launch.h"     // launch_round and the launchers per kernel

namespace {

// Autotune candidates, fixed order (fu_get_info reports per index). Kernel 8 is single-GPU.
using FP::kCands;
using FP::kNCands;
using FP::kTimed;
using FP::TuneCand;
static int width_class(int w) { return w == 8 ? 1 : w == 16 ? 2 : w == 32 ? 3 : 0; }
static void use_cand(fu_handle *h, const TuneCand &c) {
  h->kernel = c.kernel;
  h->geo = c.geo;
}

int set_device(fu_handle *h) {
  HIP_TRY(hipSetDevice(h->device));
  return FU_OK;
}

}  // namespace

extern "C" {

int fu_device_count(int32_t *out) {
  if (!out) return fail(FU_ERR_ARG, "fu_device_count: NULL");
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *out = c;
  return FU_OK;
}

// Internal constructor shared by fu_create / fu_dist_create: uploads the local CSR. The
// kernels never read a reverse-edge index (flows are reconstructed, kernel 4 §4.1), so only
// rowptr, col and the values go to the device. a_extra: ghost estimate slots (multi-GPU).
// The arguments have passed fu::check_create (every caller runs it first): the device probe
// is the first thing here, so a bad array is reported on a host without a GPU too.
int fu__create_common(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                      const double *value, int32_t device, int32_t a_extra, fu_handle **out) {
  FU_TRY_BEGIN
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(FU_ERR_HIP, "fu_create: no HIP device visible");
  if (device < 0 || device >= ndev) return fail(FU_ERR_ARG, "fu_create: device out of range");
  auto *h = new fu_handle();
  h->device = device;
  h->n = n;
  h->E = e;
  h->h_rowptr.assign(rowptr, rowptr + n + 1);
  if (e > 0) h->h_col.assign(col, col + e);
  std::vector<int32_t> rp32(n + 1);
  int32_t md = 0;
  for (int32_t i = 0; i <= n; ++i) {
    rp32[i] = (int32_t)rowptr[i];
    if (i < n) md = std::max<int32_t>(md, (int32_t)(rowptr[i + 1] - rowptr[i]));
  }
  h->max_deg = md;
  const int32_t na = n + a_extra;
  h->na = na;
  int rc = FU_OK;
  auto cleanup = [&](int code) { fu_destroy(h); return code; };
  if ((rc = set_device(h))) return cleanup(rc);
  {  // the side stream (kernel 4's heavy tiles: the long exact chains) gets the highest
     // priority, so its blocks are dispatched ahead of the light tiles when CU slots free up
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, hi) != hipSuccess)
      return cleanup(fail(FU_ERR_HIP, "hipStreamCreate failed"));
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->n_cu = cus;
  }
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
      hipEventCreate(&h->ev2) != hipSuccess || hipEventCreate(&h->ev3) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_pw, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "hipEventCreate failed"));
  // the marks a timed window uses (bench.py: up to 12) exist before any window starts: event
  // creation costs the host tens of microseconds, which a window must not contain
  for (int k = 0; k < kPreMarks; ++k)
    if (hipEventCreate(&h->marks[k]) != hipSuccess) return cleanup(fail(FU_ERR_HIP, "hipEventCreate failed"));
  if (hipHostMalloc(reinterpret_cast<void **>(&h->h_pw), sizeof(int), hipHostMallocDefault) != hipSuccess)
    return cleanup(fail(FU_ERR_ALLOC, "hipHostMalloc failed"));
  *h->h_pw = 0;
  if (hipHostGetDevicePointer(reinterpret_cast<void **>(&h->pw_dev), h->h_pw, 0) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "hipHostGetDevicePointer failed"));
  const int64_t fe = std::max<int64_t>(32, (e + 31) / 32 * 32);  // split-word flows: whole 32-edge blocks (one at least: clamped loads read edge 0)
  if ((rc = dmalloc(&h->rowptr, n + 1)) || (rc = dmalloc(&h->col, e)) || (rc = dmalloc(&h->v, n)) ||
      (rc = dmalloc(&h->f[0], fe)) || (rc = dmalloc(&h->f[1], fe)) || (rc = dmalloc(&h->a[0], na)) ||
      (rc = dmalloc(&h->a[1], na)) || (rc = dmalloc(&h->a[2], na)) || (rc = dmalloc(&h->target, n)) ||
      (rc = dmalloc(&h->err, 1)))
    return cleanup(rc);
  h->errcap = 1;
  if (hipMemcpy(h->rowptr, rp32.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice) != hipSuccess ||
      (e && hipMemcpy(h->col, col, sizeof(int) * e, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(h->v, value, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_create: upload failed"));
  if ((e == 0 && hipMemset(h->col, 0, sizeof(int)) != hipSuccess) ||
      hipMemset(h->f[0], 0, sizeof(double) * std::max<int64_t>(fe, 1)) != hipSuccess ||
      hipMemset(h->f[1], 0, sizeof(double) * std::max<int64_t>(fe, 1)) != hipSuccess ||
      hipMemset(h->a[0], 0, sizeof(double) * na) != hipSuccess || hipMemset(h->a[1], 0, sizeof(double) * na) != hipSuccess ||
      hipMemset(h->a[2], 0, sizeof(double) * na) != hipSuccess)
    return cleanup(fail(FU_ERR_HIP, "fu_create: memset failed"));
  {  // round 0's per-block rows; kernel 4's 2-byte column offsets (FP::build_blocks)
    std::vector<int32_t> br;
    std::vector<uint16_t> c16;
    FP::build_blocks(n, e, rowptr, col, br, h->h_cbase, c16);
    if ((rc = upload(&h->blk_row, br)) || (rc = upload(&h->col16, c16)) || (rc = upload(&h->cbase, h->h_cbase)))
      return cleanup(rc);
  }
  if ((rc = build_tiles(h))) return cleanup(rc);
  if ((rc = dmalloc(&h->pctl, 3)) || (rc = dmalloc(&h->code[0], 4 * (size_t)na)) ||
      (rc = dmalloc(&h->code[1], 4 * (size_t)na)))
    return cleanup(rc);
  if (hipMemset(h->pctl, 0, sizeof(PackCtl) * 3) != hipSuccess) return cleanup(fail(FU_ERR_HIP, "fu_create: memset failed"));
  if (e > 0) {  // plan sample: the targets of 4096 pseudo-random edges (degree-weighted)
    const int ns = kPlanSamples;
    std::vector<int32_t> smp(ns);
    for (int q = 0; q < ns; ++q) smp[q] = col[splitmix_at(0x9ac4u, (uint64_t)q) % (uint64_t)e];
    if ((rc = dmalloc(&h->psample, ns))) return cleanup(rc);
    if (hipMemcpy(h->psample, smp.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice) != hipSuccess)
      return cleanup(fail(FU_ERR_HIP, "fu_create: upload failed"));
    h->n_psample = ns;
  }
  *out = h;
  return FU_OK;
  FU_TRY_END
}

// Every argument and CSR check (fu::check_fu_create) comes before anything walks the arrays. The
// flow reconstruction needs every i -> j to have its j -> i: a caller's rev is checked to be
// that pairing; without one, fu::build_rev checks symmetry (the index itself is not kept).
int fu_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
              const int32_t *rev, const double *value, int32_t device, fu_handle **out) {
  FU_TRY_BEGIN
  if (int rc = fu::check_fu_create(n, e, rowptr, col, rev, value, out)) return rc;
  return fu__create_common(n, e, rowptr, col, value, device, 0, out);
  FU_TRY_END
}

int fu_create_from_graph(const fu_graph *g, const double *value, int32_t device,
                         fu_handle **out) {
  FU_TRY_BEGIN
  if (!g) return fail(FU_ERR_ARG, "fu_create_from_graph: NULL graph");
  const int64_t E = g->rowptr[g->n];
  if ((int64_t)g->rev.size() != E) return fail(FU_ERR_GRAPH, "fu_create_from_graph: graph is not symmetric");
  if (int rc = fu::check_create("fu_create_from_graph", g->n, E, g->rowptr.data(), g->col.data(), value, 0, out)) return rc;
  return fu__create_common(g->n, E, g->rowptr.data(), g->col.data(), value, device, 0, out);
  FU_TRY_END
}

int fu_create_from_graph_ex(const fu_graph *g, const double *value, int32_t device,
                            int32_t layout, fu_handle **out) {
  FU_TRY_BEGIN
  if (!g || !value || !out || layout < 0 || layout > 1) return fail(FU_ERR_ARG, "fu_create_from_graph_ex: bad arguments");
  if (layout == 0) return fu_create_from_graph(g, value, device, out);
  const int32_t n = g->n;
  std::vector<int32_t> nofo(n);
  fu_graph *rg = nullptr;
  if (int rc = fu_graph_relabel(g, 1, nofo.data(), &rg)) return rc;
  std::vector<double> v2(n);
  for (int32_t i = 0; i < n; ++i) v2[nofo[i]] = value[i];
  const int rc = fu_create_from_graph(rg, v2.data(), device, out);
  fu_graph_free(rg);
  if (rc) return rc;
  (*out)->h_new_of_old.swap(nofo);
  (*out)->h_orig_rowptr = g->rowptr;
  return FU_OK;
  FU_TRY_END
}

int fu_set_option(fu_handle *h, const char *key, int64_t value) {
  FU_TRY_BEGIN
  if (!h || !key) return fail(FU_ERR_ARG, "fu_set_option: NULL argument");
  if (int rc = set_device(h)) return rc;
  if (!std::strcmp(key, "kernel")) {
    if (value != 0 && value != 4 && value != 8 && value != 9)
      return fail(FU_ERR_ARG, "fu_set_option: kernel must be 0 (auto), 4 (recon), 8 (stage) or 9 (pregather)");
    if (h->rounds != 0) return fail(FU_ERR_STATE, "fu_set_option: kernel can only change before the first round (call fu_reset)");
    int rc = FU_OK;
    if (value == 8) rc = ensure_stage(h);
    if (value == 9) rc = ensure_transpose(h);  // the slice limit counts ghost slots: rank-dependent
    if (h->dist) {  // RCCL ranks: a kernel that fails on one rank fails on all (collective)
      const std::string why = rc ? fu_last_error() : "";
      int all_ok = 1;
      if (int rc2 = fu__dist_agree(h, rc == FU_OK, &all_ok)) return rc2;
      // a rank without a layout (FU_ERR_GRAPH on one GPU) reports what its peers report: the
      // partition, not the graph, decides which rank it is. The handle keeps its kernel.
      if (rc == FU_ERR_GRAPH) return fail(FU_ERR_STATE, why);
      if (rc) return fail(rc, why);
      if (!all_ok) return fail(FU_ERR_STATE, "fu_set_option: kernel " + std::to_string(value) + " failed on another rank");
    }
    if (rc) return rc;
    if (value == 9) h->geo = 1;
    h->kernel = value == 0 ? 4 : (int)value;
    h->autotune = value == 0;
    h->tuned = false;
    h->tune_for_width = false;
    return FU_OK;
  }
  if (!std::strcmp(key, "stage_layout")) {  // kernel 8: -1 = by packing width, 0..3 forced
    if (value < -1 || value > 3) return fail(FU_ERR_ARG, "fu_set_option: stage_layout must be -1..3");
    h->st_force = (int)value;
    return FU_OK;
  }
  if (!std::strcmp(key, "pack")) {
    h->pack = value != 0;
    if (!h->pack) {  // stop encoding (and drop a plan still due)
      h->plan_pending = false;
      HIP_TRY(hipMemsetAsync(h->pctl + 2, 0, sizeof(PackCtl), h->stream));
    }
    return FU_OK;
  }
  if (!std::strcmp(key, "pack_every")) {
    if (value < 1 || value > (1 << 20)) return fail(FU_ERR_ARG, "fu_set_option: pack_every must be in [1, 2^20]");
    h->pack_every = (int)value;
    return FU_OK;
  }
  if (!std::strcmp(key, "tile_edges")) {
    if (value != 2048 && value != 1024 && value != 512) return fail(FU_ERR_ARG, "fu_set_option: tile_edges must be 2048, 1024 or 512");
    h->tile_edges = (int)value;
    h->geo = h->tile_edges == 2048 ? 0 : h->tile_edges == 512 ? 3 : h->tile_nodes == 256 ? 2 : 1;
    return FU_OK;
  }
  if (!std::strcmp(key, "tile_nodes")) {
    if (value != 0 && value != 128 && value != 256) return fail(FU_ERR_ARG, "fu_set_option: tile_nodes must be 0, 128 or 256");
    h->tile_nodes = (int)value;
    h->geo = h->tile_edges == 2048 ? 0 : h->tile_edges == 512 ? 3 : h->tile_nodes == 256 ? 2 : 1;
    return FU_OK;
  }
  if (!std::strcmp(key, "fork_heavy")) {  // kernel 4: heavy tiles on a side stream (1) or in order (0)
    h->fork_heavy = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "split_hubs")) {  // kernel 4: mega-hub tiles alone on the side stream (1)
    h->split_hubs = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "staged_lo")) {  // accepted, no effect: the interleaved order (0) is gone
    return FU_OK;
  }
  if (!std::strcmp(key, "tr_bpx")) {  // kernel 9: transpose blocks per XCD (0 = one per bucket)
    if (value < 0 || value > 1 << 20) return fail(FU_ERR_ARG, "fu_set_option: tr_bpx must be in [0, 2^20]");
    h->tr_bpx = (int)value;
    return FU_OK;
  }
  if (!std::strcmp(key, "lag")) {  // kernel 9: the multi-row heavy rows write f_r in round r + 2
    const int lv = value != 0;
    if (lv != h->lag) {
      if (int rc = lag_finalize_all(h)) return rc;  // flows first, with the current G_B ring
      free_transpose(h);                            // the ring's size follows the option
      h->lag = lv;
    }
    return FU_OK;
  }
  if (!std::strcmp(key, "tr_nt")) {  // kernel 9: k_transpose stores G_B non-temporally (1)
    if (value != 0 && value != 1) return fail(FU_ERR_ARG, "fu_set_option: tr_nt must be 0 or 1");
    h->tr_nt = (int)value;
    return FU_OK;
  }
  if (!std::strcmp(key, "multi_short")) {  // kernel 9: rows of 129-256 edges as multi-row blocks (1)
    h->multi_short = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "iso_rows")) {  // kernel 9: trailing isolated rows one thread each (1) or as tiles (0)
    h->iso_rows = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "multi_heavy")) {  // kernel 9: rows > 256 edges with many rows per chain wave (1)
    h->multi_heavy = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "c16")) {  // kernel 4: 2-byte column offsets for narrow light tiles (1) or not (0)
    h->c16 = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "multi_mid")) {  // kernel 9: rows of 257-1024 edges in k_heavy_multi (1) or in registers (0)
    h->multi_mid = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "mid_heavy")) {  // kernel 9: register-resident launch for rows of 257-1024 edges
    h->mid_heavy = value != 0;
    return FU_OK;
  }
  if (!std::strcmp(key, "wave_heavy")) {  // kernel 4: heavy rows one per wave (1) or per block (0)
    h->wave_heavy = value != 0;
    return build_tiles(h);
  }
  if (!std::strcmp(key, "mega_hub")) {  // kernel 4: staged-chain rows (tests lower it)
    if (value < 1) return fail(FU_ERR_ARG, "fu_set_option: mega_hub must be >= 1");
    h->mega_hub = (int)std::min<int64_t>(value, INT32_MAX);
    return build_tiles(h);
  }
  if (!std::strcmp(key, "hub_threshold")) {
    if (value < 1) return fail(FU_ERR_ARG, "fu_set_option: hub_threshold must be >= 1");
    if (h->st_tiles) return fail(FU_ERR_STATE, "fu_set_option: hub_threshold must be set before kernel 8 is prepared");
    h->hub_threshold = (int)std::min<int64_t>(value, 2048);
    return build_tiles(h);
  }
  return fail(FU_ERR_ARG, std::string("fu_set_option: unknown key '") + key + "'");
  FU_TRY_END
}

int fu_reset(fu_handle *h) {
  FU_TRY_BEGIN
  if (!h) return fail(FU_ERR_ARG, "fu_reset: NULL handle");
  if (int rc = set_device(h)) return rc;
  if (h->dist) {  // phase 1: wait for the last halo, drain the comm stream, forget its rounds
    if (int rc = fu__dist_round_hook(h, 1)) return rc;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->rounds = 0;
  h->lagf[0] = h->lagf[1] = 0;  // zero state: nothing lagged
  h->pw_pending = false;  // the stream is idle: no plan in flight
  h->plan_pending = false;  // round 0 clears the plan
  *h->h_pw = 0;           // round 0 clears the packing plan
  h->seen_width = 0;
  // unpacked again: its winner. A pass still pending for a width the rounds before the reset
  // reached (seen in calls too short for a pass) no longer applies; one armed by the kernel
  // option still runs. Where no pass ever ran unpacked (the first one ran at a packed width),
  // there is no winner to return to: the winner of a packed width would stay in use at width 0
  // with tuned_width claiming that width, so a pass for width 0 is armed as on a new handle.
  if (h->autotune && (h->tuned || h->tune_for_width)) {
    h->tuned_width = 0;
    h->tune_for_width = false;
    h->tuned = h->tune_cache[0] >= 0;
    if (h->tuned) use_cand(h, kCands[h->tune_cache[0]]);
  }
  return FU_OK;
  FU_TRY_END
}

int fu_set_targets(fu_handle *h, const double *target) {
  FU_TRY_BEGIN
  if (!h || !target) return fail(FU_ERR_ARG, "fu_set_targets: NULL argument");
  if (int rc = set_device(h)) return rc;
  std::vector<double> t2;
  if (!h->h_new_of_old.empty()) {  // caller numbering -> device numbering
    t2.resize(h->n);
    for (int32_t i = 0; i < h->n; ++i) t2[h->h_new_of_old[i]] = target[i];
    target = t2.data();
  }
  HIP_TRY(hipMemcpyAsync(h->target, target, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->has_target = true;
  return FU_OK;
  FU_TRY_END
}

int fu__err_slots(fu_handle *h, int count) {
  if (count <= h->errcap) return FU_OK;
  if (h->err) hipFree(h->err);
  h->err = nullptr;
  h->errcap = 0;
  if (int rc = dmalloc(&h->err, count)) return rc;
  h->errcap = count;
  return FU_OK;
}

// Kernels 4 (every geometry) and 8 share the state layout (F[r & 1], A[r % 3]) and are
// bitwise identical, so switching between them mid-run changes nothing but speed. "auto"
// times each candidate on real rounds (1 warm + 8 timed each) and keeps the fastest. The
// rounds count toward the caller's total and the results are unchanged. The pass re-runs
// when the packing plan changes width (the packed gather shifts the balance between the
// candidates), at most kMaxTunes times; fu_tune runs one pass on demand.
constexpr int kMaxTunes = 4;

static int autotune_kernel(fu_handle *h, int32_t *budget, int width) {
  // which candidate runs (FP::tune_steps): multi-GPU, every rank must run the same rounds
  // (each one is a halo exchange), so no candidate is dropped and none stops early on
  // rank-local timings (tools/plan_check --tune checks the count is rank-independent)
  FP::TuneRank tr;
  tr.dist = h->dist != nullptr;
  tr.width = width;
  for (int c = 0; c < kNCands; ++c) tr.tune_out[c] = h->tune_out[c];
  if (FP::tune_need(tr) > *budget) return FU_OK;  // not enough rounds in this call: try again later
  // the pass runs at the table's current width: the host's copy of it is exact once the stream
  // is idle, and no plan runs until the pass ends (h->tuning)
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->pw_pending = false;
  h->seen_width = width = *h->h_pw;
  tr.width = width;
  if (FP::tune_need(tr) > *budget) return FU_OK;
  int steps[kNCands];
  FP::tune_steps(tr, steps);
  if (steps[2] != FP::kTuneSkip && ensure_stage(h) != FU_OK) {  // no slice layout fits this graph
    set_error("");
    tr.k8_ok = false;
  }
  if (steps[4] != FP::kTuneSkip && ensure_transpose(h) != FU_OK) {  // too many nodes for the slices
    set_error("");
    tr.k9_ok = false;
  }
  FP::tune_steps(tr, steps);
  const int32_t budget0 = *budget;
  h->tuning = true;
  struct Untune {
    fu_handle *h;
    ~Untune() { h->tuning = false; }
  } untune{h};
  float best = 1e30f;
  int bi = -1;
  for (int c = 0; c < kNCands; ++c) {
    if (!h->dist && h->tune_out[c] >= 2) continue;  // its last ns per round stays reported
    h->tune_ms[c] = 0.f;
    if (steps[c] == FP::kTuneSkip) continue;
    if (steps[c] == FP::kTuneStandIn) {
      // multi-GPU: this rank still runs the candidate's rounds (kernel 4), so that every
      // rank runs the same rounds (each is a halo exchange); its time is never the best
      use_cand(h, kCands[0]);
      for (int k = 0; k < 1 + kTimed; ++k)
        if (int rc = launch_round(h, nullptr)) return rc;
      *budget -= 1 + kTimed;
      h->tune_ms[c] = 1e30f;
      continue;
    }
    use_cand(h, kCands[c]);
    // the warm round is timed too: a candidate more than twice the best per-round time so far
    // stops there (on R-MAT-24 the staged kernel would take 3x kernel 4 for 8 rounds). The
    // events are recorded on an idle stream, so the warm round's time also holds the host's
    // first launch of the candidate's kernels; a slow warm round is therefore confirmed by a
    // second one, launched behind it, before the candidate is dropped
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    if (int rc = launch_round(h, nullptr)) return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    if (best < 1e30f && !h->dist) {
      HIP_TRY(hipEventSynchronize(h->ev1));
      float wms = 0.f;
      HIP_TRY(hipEventElapsedTime(&wms, h->ev0, h->ev1));
      *budget -= 1;
      if (wms > 2.f * best / kTimed) {
        HIP_TRY(hipEventRecord(h->ev0, h->stream));
        if (int rc = launch_round(h, nullptr)) return rc;
        if (int rc = launch_round(h, nullptr)) return rc;
        HIP_TRY(hipEventRecord(h->ev1, h->stream));
        HIP_TRY(hipEventSynchronize(h->ev1));
        HIP_TRY(hipEventElapsedTime(&wms, h->ev0, h->ev1));
        *budget -= 2;
        if (wms > 2.f * 2.f * best / kTimed) {
          h->tune_ms[c] = wms / 2.f;
          continue;
        }
      }
      *budget += 1;  // counted below with the timed rounds
    }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    for (int k = 0; k < kTimed; ++k)
      if (int rc = launch_round(h, nullptr)) return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->tune_ms[c] = ms / kTimed;
    *budget -= 1 + kTimed;
    if (ms < best) {
      best = ms;
      bi = c;
    }
  }
  if (bi < 0) return fail(FU_ERR_STATE, "autotune: no candidate ran");
  if (h->dist && budget0 - *budget != FP::tune_rounds_fixed(tr))
    return fail(FU_ERR_STATE, "autotune: a multi-GPU pass ran " + std::to_string(budget0 - *budget) + " rounds, not " +
                                  std::to_string(FP::tune_rounds_fixed(tr)) + " (the ranks would diverge)");
  for (int c = 0; c < kNCands; ++c)
    if (h->tune_ms[c] > 1.3f * h->tune_ms[bi]) h->tune_out[c]++;
  use_cand(h, kCands[bi]);
  h->tune_cache[width_class(width)] = bi;
  h->tuned_width = width;
  h->tuned = true;
  h->tune_for_width = false;
  h->n_tunes++;
  return FU_OK;
}

// After each packing plan the host keeps an asynchronous copy of its width; a changed width
// re-arms the autotuner (checked without blocking).
static void poll_pack_width(fu_handle *h) {
  if (!h->pw_pending || hipEventQuery(h->ev_pw) != hipSuccess) return;
  h->pw_pending = false;
  h->seen_width = *h->h_pw;
  if (!h->autotune || !h->tuned || *h->h_pw == h->tuned_width) return;
  const int cached = h->tune_cache[width_class(*h->h_pw)];
  if (cached >= 0) {  // this width was tuned before (e.g. before fu_reset): reuse its winner
    use_cand(h, kCands[cached]);
    h->tuned_width = *h->h_pw;
  } else if (h->n_tunes < kMaxTunes) {
    h->tuned = false;
    h->tune_for_width = true;
  }
}

// The round loop shared by fu_run_collectall and fu_run_collectall_timed.
static int run_rounds(fu_handle *h, int32_t rounds, int32_t err_every, int nerr) {
  for (int32_t r = 0; r < rounds; ++r) {
    poll_pack_width(h);
    // tune between rounds when no error slot is pending in the rounds it would consume
    if (h->autotune && !h->tuned && h->rounds >= 1 && nerr == 0) {
      int32_t budget = rounds - r;
      const int w = h->pw_pending ? h->tuned_width : *h->h_pw;
      if (int rc = autotune_kernel(h, &budget, w)) return rc;
      r = rounds - budget;
      if (r >= rounds) break;
    }
    unsigned long long *slot = nullptr;
    if (nerr > 0 && (r + 1) % err_every == 0) slot = h->err + ((r + 1) / err_every - 1);
    if (int rc = launch_round(h, slot)) return rc;
  }
  return FU_OK;
}

int fu_run_collectall(fu_handle *h, int32_t rounds, int32_t err_every, double *err_trace) {
  FU_TRY_BEGIN
  if (!h || rounds < 0) return fail(FU_ERR_ARG, "fu_run_collectall: bad arguments");
  if (err_every > 0 && !h->has_target) return fail(FU_ERR_STATE, "fu_run_collectall: err_every > 0 needs fu_set_targets");
  if (int rc = set_device(h)) return rc;
  const int nerr = err_every > 0 ? rounds / err_every : 0;
  if (nerr > 0) {
    if (int rc = fu__err_slots(h, nerr)) return rc;
    HIP_TRY(hipMemsetAsync(h->err, 0, sizeof(unsigned long long) * nerr, h->stream));
  }
  if (int rc = run_rounds(h, rounds, err_every, nerr)) return rc;
  if (nerr > 0) {
    if (h->dist) {
      if (int rc = fu__dist_round_hook(h, 100 + nerr)) return rc;  // all-reduce max, in place
    }
    std::vector<unsigned long long> bits(nerr);
    HIP_TRY(hipMemcpyAsync(bits.data(), h->err, sizeof(unsigned long long) * nerr, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (err_trace) std::memcpy(err_trace, bits.data(), sizeof(double) * nerr);
  }
  return FU_OK;
  FU_TRY_END
}

int fu_run_collectall_timed(fu_handle *h, int32_t rounds, float *ms) {
  FU_TRY_BEGIN
  if (!h || !ms || rounds < 0) return fail(FU_ERR_ARG, "fu_run_collectall_timed: bad arguments");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipEventRecord(h->ev2, h->stream));
  if (int rc = run_rounds(h, rounds, 0, 0)) return rc;
  if (h->dist) {  // the last round's halo (comm stream) inside the timed window
    if (int rc = fu__dist_round_hook(h, 0)) return rc;
  }
  HIP_TRY(hipEventRecord(h->ev3, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev3));
  HIP_TRY(hipEventElapsedTime(ms, h->ev2, h->ev3));
  return FU_OK;
  FU_TRY_END
}

// A timed window in one host call: mark k (HIP event slot k) is recorded once rounds_at[k]
// rounds of this call have been queued (rounds_at[0] = 0: before the first). A window that
// starts with round 0 (after fu_reset, single GPU) takes mark 0 from k_round0's own start and,
// when mark 1 follows round 0, mark 1 from its end (hipExtLaunchKernel's start / stop events):
// an event recorded on the idle stream ahead of the launch would time-stamp at once and hold
// the first dispatch's latency, and a marker behind it its own ~5 us, in round 0's time.
int fu_run_collectall_marked(fu_handle *h, int32_t n_marks, const int32_t *rounds_at) {
  FU_TRY_BEGIN
  if (!h || !rounds_at || n_marks < 1 || n_marks > 64 || rounds_at[0] < 0)
    return fail(FU_ERR_ARG, "fu_run_collectall_marked: bad arguments (1..64 marks, rounds_at[0] >= 0)");
  for (int k = 1; k < n_marks; ++k)
    if (rounds_at[k] < rounds_at[k - 1]) return fail(FU_ERR_ARG, "fu_run_collectall_marked: rounds_at must not decrease");
  if (int rc = set_device(h)) return rc;
  for (int k = 0; k < n_marks; ++k)
    if (!h->marks[k]) HIP_TRY(hipEventCreate(&h->marks[k]));
  int32_t done = 0;
  const bool r0 = rounds_at[0] == 0 && n_marks > 1 && rounds_at[1] > 0 && h->rounds == 0 && !h->dist;
  const bool r0_end = r0 && rounds_at[1] == 1;
  for (int k = 0; k < n_marks; ++k) {
    if (rounds_at[k] > done) {
      if (int rc = run_rounds(h, rounds_at[k] - done, 0, 0)) {
        h->r0_start = h->r0_stop = nullptr;  // a failed call leaves no event armed for a later round 0
        return rc;
      }
      done = rounds_at[k];
    }
    if (h->dist) {  // a mark after a round includes that round's halo (comm stream)
      if (int rc = fu__dist_round_hook(h, 0)) return rc;
    }
    if (k == 0 && r0) {  // recorded by round 0's own launch
      h->r0_start = h->marks[0];
      if (r0_end) h->r0_stop = h->marks[1];
    } else if (!(k == 1 && r0_end)) {
      HIP_TRY(hipEventRecord(h->marks[k], h->stream));
    }
  }
  if (h->r0_start) {  // round 0 did not launch through launch_round0: never the case
    h->r0_start = h->r0_stop = nullptr;
    return fail(FU_ERR_STATE, "fu_run_collectall_marked: round 0 was not launched");
  }
  return FU_OK;
  FU_TRY_END
}

int fu_tune(fu_handle *h) {
  FU_TRY_BEGIN
  if (!h) return fail(FU_ERR_ARG, "fu_tune: NULL handle");
  if (!h->autotune) return fail(FU_ERR_STATE, "fu_tune: the kernel is pinned (option kernel != 0)");
  if (int rc = set_device(h)) return rc;
  if (h->rounds == 0)
    if (int rc = launch_round(h, nullptr)) return rc;  // round 0 is not a tuning candidate
  HIP_TRY(hipStreamSynchronize(h->stream));
  poll_pack_width(h);
  const int w = h->pw_pending ? h->tuned_width : *h->h_pw;
  int32_t budget = INT32_MAX;
  if (int rc = autotune_kernel(h, &budget, w)) return rc;
  return FU_OK;
  FU_TRY_END
}

int fu_mark(fu_handle *h, int32_t slot) {
  if (!h || slot < 0 || slot >= 64) return fail(FU_ERR_ARG, "fu_mark: slot must be in [0, 64)");
  if (int rc = set_device(h)) return rc;
  if (!h->marks[slot]) HIP_TRY(hipEventCreate(&h->marks[slot]));
  if (h->dist) {  // a mark after a round includes that round's halo (comm stream)
    if (int rc = fu__dist_round_hook(h, 0)) return rc;
  }
  HIP_TRY(hipEventRecord(h->marks[slot], h->stream));
  return FU_OK;
}

int fu_mark_elapsed(fu_handle *h, int32_t from, int32_t to, float *ms) {
  if (!h || !ms || from < 0 || from >= 64 || to < 0 || to >= 64 || !h->marks[from] || !h->marks[to])
    return fail(FU_ERR_ARG, "fu_mark_elapsed: unrecorded slot");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipEventSynchronize(h->marks[to]));
  HIP_TRY(hipEventElapsedTime(ms, h->marks[from], h->marks[to]));
  return FU_OK;
}

int fu_max_err(fu_handle *h, double *out) {
  FU_TRY_BEGIN
  if (!h || !out) return fail(FU_ERR_ARG, "fu_max_err: NULL argument");
  if (!h->has_target) return fail(FU_ERR_STATE, "fu_max_err: call fu_set_targets first");
  if (int rc = set_device(h)) return rc;
  HIP_TRY(hipMemsetAsync(h->err, 0, sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(k_max_err, dim3(std::min(1024u, grid_for(h->n))), dim3(kBlock), 0, h->stream,
                     h->n, cur_a(h), h->target, h->err);
  HIP_TRY(hipGetLastError());
  if (h->dist) {
    if (int rc = fu__dist_round_hook(h, 101)) return rc;  // all-reduce max of slot 0
  }
  unsigned long long bits = 0;
  HIP_TRY(hipMemcpyAsync(&bits, h->err, sizeof(bits), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::memcpy(out, &bits, sizeof(double));
  return FU_OK;
  FU_TRY_END
}

// Device memory -> the caller's (pageable) host memory through two pinned kXfer-byte
// buffers: the DMA of chunk k runs while the host copies chunk k-1 out. A pageable
// hipMemcpyAsync stages through the runtime's own buffers one at a time (ER-1M's 8 MB of
// estimates: 31 ms on the box, profiles/r05/g/).
constexpr size_t kXfer = (size_t)4 << 20;

static int copy_out(fu_handle *h, void *dst, const void *src, size_t bytes) {
  for (int k = 0; k < 2; ++k) {
    if (!h->h_xfer[k] && hipHostMalloc(&h->h_xfer[k], kXfer, hipHostMallocDefault) != hipSuccess)
      return fail(FU_ERR_ALLOC, "hipHostMalloc (copy-out buffer) failed");
    if (!h->ev_xfer[k] && hipEventCreateWithFlags(&h->ev_xfer[k], hipEventDisableTiming) != hipSuccess)
      return fail(FU_ERR_HIP, "hipEventCreate failed");
  }
  const size_t nk = (bytes + kXfer - 1) / kXfer;
  for (size_t k = 0; k <= nk; ++k) {
    if (k < nk) {  // chunk k into buffer k & 1 (its previous chunk, k - 2, was copied out at k - 1)
      const size_t len = std::min(kXfer, bytes - k * kXfer);
      HIP_TRY(hipMemcpyAsync(h->h_xfer[k & 1], static_cast<const char *>(src) + k * kXfer, len,
                             hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipEventRecord(h->ev_xfer[k & 1], h->stream));
    }
    if (k > 0) {  // chunk k - 1 out while chunk k is in flight
      const size_t j = k - 1, len = std::min(kXfer, bytes - j * kXfer);
      HIP_TRY(hipEventSynchronize(h->ev_xfer[j & 1]));
      std::memcpy(static_cast<char *>(dst) + j * kXfer, h->h_xfer[j & 1], len);
    }
  }
  return FU_OK;
}

int fu_get_estimates(fu_handle *h, double *a_out) {
  FU_TRY_BEGIN
  if (!h || !a_out) return fail(FU_ERR_ARG, "fu_get_estimates: NULL argument");
  if (int rc = set_device(h)) return rc;
  if (!h->h_new_of_old.empty()) {  // device numbering -> caller numbering
    std::vector<double> a2(h->n);
    if (int rc = copy_out(h, a2.data(), cur_a(h), sizeof(double) * h->n)) return rc;
    for (int32_t i = 0; i < h->n; ++i) a_out[i] = a2[h->h_new_of_old[i]];
    return FU_OK;
  }
  return copy_out(h, a_out, cur_a(h), sizeof(double) * h->n);
  FU_TRY_END
}

int fu_get_flows(fu_handle *h, double *f_out) {
  FU_TRY_BEGIN
  if (!h || (!f_out && h->E)) return fail(FU_ERR_ARG, "fu_get_flows: NULL argument");
  if (h->E == 0) return FU_OK;
  if (h->rounds == 0) {  // no round yet: every flow is 0.0 (CA:33)
    std::memset(f_out, 0, sizeof(double) * (size_t)h->E);
    return FU_OK;
  }
  if (int rc = set_device(h)) return rc;
  if (!h->ftmp) {
    if (int rc = dmalloc(&h->ftmp, (size_t)h->E)) return rc;
  }
  if (h->rounds >= 2) {  // kernel 9's lag: the last round's flows of its lagged rows
    if (int rc = lag_finalize(h, (int)((h->rounds - 1) & 1))) return rc;
  }
  if (h->rounds == 1)  // round 0 writes no flows (fm): f_0 = (0.0 + a_0[i]) - 0.0 on demand
    hipLaunchKernelGGL(k_round0_flows, dim3((unsigned)((h->E + kR0E - 1) / kR0E)), dim3(kBlock), 0, h->stream,
                       (long long)h->E, h->rowptr, h->blk_row, h->a[0], h->f[0], nullptr);
  // split words -> doubles
  hipLaunchKernelGGL(k_unsplit, dim3(grid_for(h->E)), dim3(kBlock), 0, h->stream, (long long)h->E, cur_f(h), h->ftmp);
  HIP_TRY(hipGetLastError());
  const double *src = h->ftmp;
  if (!h->h_new_of_old.empty()) {  // rows back to the caller's order (blocks, same order inside)
    std::vector<double> f2(h->E);
    if (int rc = copy_out(h, f2.data(), src, sizeof(double) * h->E)) return rc;
    const auto &orp = h->h_orig_rowptr;
    for (int32_t i = 0; i < h->n; ++i) {
      const int64_t nb = h->h_rowptr[h->h_new_of_old[i]];
      std::memcpy(f_out + orp[i], f2.data() + nb, sizeof(double) * (orp[i + 1] - orp[i]));
    }
    return FU_OK;
  }
  return copy_out(h, f_out, src, sizeof(double) * h->E);
  FU_TRY_END
}

int fu_get_info(fu_handle *h, int64_t info[32]) {
  if (!h || !info) return fail(FU_ERR_ARG, "fu_get_info: NULL argument");
  for (int k = 0; k < 32; ++k) info[k] = 0;
  info[0] = h->kernel;
  info[1] = 0;  // (reserved: kernel 4's removed "nt" option)
  info[2] = h->autotune ? (h->tuned ? 2 : 1) : 0;
  info[3] = h->rounds;
  info[4] = kGeoEdges[h->geo];
  info[5] = kGeoNodes[h->geo];
  info[6] = h->n_tunes;
  info[7] = h->tuned_width;
  for (int k = 0; k < kNCands; ++k) info[8 + k] = (int64_t)((double)h->tune_ms[k] * 1e6);  // ns per round
  info[20] = h->n_hub;
  for (int k = 0; k < 4; ++k)  // autotune winner per packing width 0, 8, 16, 32 (kernel * 10 + geometry; -1 = none)
    info[23 + k] = h->tune_cache[k] < 0 ? -1 : kCands[h->tune_cache[k]].kernel * 10 + kCands[h->tune_cache[k]].geo;
  for (int li = 0; li < 4; ++li) info[27 + li] = h->st[li].P;  // kernel 8 slices per layout (0 = not built)
  return FU_OK;
}

int fu_get_pack(fu_handle *h, int32_t width[3]) {
  FU_TRY_BEGIN
  if (!h || !width) return fail(FU_ERR_ARG, "fu_get_pack: NULL argument");
  if (int rc = set_device(h)) return rc;
  if (h->plan_pending && h->rounds > 0) {  // the plan due after the last round, as the next round would run it
    hipLaunchKernelGGL(k_pack_plan, dim3(1), dim3(kBlock), 0, h->stream, cur_a(h), h->psample, h->pctl, h->pw_dev);
    HIP_TRY(hipGetLastError());
    h->plan_pending = false;
  }
  PackCtl p[3];
  HIP_TRY(hipMemcpyAsync(p, h->pctl, sizeof(p), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 3; ++k) width[k] = p[k].width;
  return FU_OK;
  FU_TRY_END
}

int fu_get_round(fu_handle *h, int64_t *rounds_done) {
  if (!h || !rounds_done) return fail(FU_ERR_ARG, "fu_get_round: NULL argument");
  *rounds_done = h->rounds;
  return FU_OK;
}

int fu_mem_info(int32_t device, int64_t *free_bytes, int64_t *total_bytes) {
  if (!free_bytes || !total_bytes) return fail(FU_ERR_ARG, "fu_mem_info: NULL argument");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return fail(FU_ERR_HIP, "fu_mem_info: no HIP device visible");
  if (device < 0 || device >= nd) return fail(FU_ERR_ARG, "fu_mem_info: bad device");
  HIP_TRY(hipSetDevice(device));
  size_t fr = 0, tot = 0;
  HIP_TRY(hipMemGetInfo(&fr, &tot));
  *free_bytes = (int64_t)fr;
  *total_bytes = (int64_t)tot;
  return FU_OK;
}

int fu_copy_bandwidth(int32_t device, int64_t bytes, int32_t iters, double *gbs) {
  FU_TRY_BEGIN
  if (!gbs || bytes < 16 * 1024 || iters < 1) return fail(FU_ERR_ARG, "fu_copy_bandwidth: bad arguments");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return fail(FU_ERR_HIP, "fu_copy_bandwidth: no HIP device visible");
  if (device < 0 || device >= nd) return fail(FU_ERR_ARG, "fu_copy_bandwidth: bad device");
  HIP_TRY(hipSetDevice(device));
  const long long cnt = bytes / 2 / 16;  // half read, half written
  float4 *a = nullptr, *b = nullptr;
  if (int rc = dmalloc(&a, (size_t)cnt)) return rc;
  if (int rc = dmalloc(&b, (size_t)cnt)) {
    hipFree(a);
    return rc;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = FU_OK;
  float best = 1e30f;
  const unsigned grid = 8u * 256u * 8u;  // 8 blocks per CU, grid-stride
  if (hipMemset(a, 0, sizeof(float4) * cnt) != hipSuccess || hipEventCreate(&e0) != hipSuccess ||
      hipEventCreate(&e1) != hipSuccess)
    rc = fail(FU_ERR_HIP, "fu_copy_bandwidth: setup");
  for (int k = 0; rc == FU_OK && k <= iters; ++k) {  // the first copy warms up, untimed
    hipEventRecord(e0, nullptr);
    hipLaunchKernelGGL(k_copy4, dim3(grid), dim3(kBlock), 0, nullptr, cnt, a, b);
    hipEventRecord(e1, nullptr);
    float ms = 0.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
      rc = fail(FU_ERR_HIP, "fu_copy_bandwidth: copy");
    else if (k > 0)
      best = std::min(best, ms);
  }
  if (e0) hipEventDestroy(e0);
  if (e1) hipEventDestroy(e1);
  hipFree(a);
  hipFree(b);
  if (rc) return rc;
  *gbs = 2.0 * 16.0 * (double)cnt / (best * 1e-3) / 1e9;
  return FU_OK;
  FU_TRY_END
}

int fu_synchronize(fu_handle *h) {
  if (!h) return fail(FU_ERR_ARG, "fu_synchronize: NULL handle");
  if (int rc = set_device(h)) return rc;
  if (h->dist) {
    if (int rc = fu__dist_round_hook(h, 0)) return rc;  // the stream waits for the last halo
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return FU_OK;
}

int fu_destroy(fu_handle *h) {
  if (!h) return FU_OK;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->stream2) hipStreamSynchronize(h->stream2);
  if (h->dist) fu__dist_free(h);
  std::vector<void *> ptrs = {h->rowptr, h->col, h->blk_row, h->v, h->f[0], h->f[1], h->a[0], h->a[1], h->a[2], h->target,
                              h->err, h->ftmp, h->tiles_geo[0], h->tiles_geo[1], h->tiles_geo[2], h->tiles_geo[3],
                              h->hrows, h->hub_rows, h->hub_off, h->hubxy, h->hub_blk, h->code[0], h->code[1], h->pctl,
                              h->psample, h->st_tiles, h->st_heavy, h->stG, h->col16, h->cbase,
                              h->tnar_geo[0], h->tnar_geo[1], h->tnar_geo[2], h->tnar_geo[3]};
  free_transpose(h);
  for (const auto &L : h->st) {
    ptrs.push_back(L.brange);
    ptrs.push_back(L.colS);
    ptrs.push_back(L.sidx16);
    ptrs.push_back(L.dtab);
  }
  for (void *p : ptrs)
    if (p) hipFree(p);
  for (hipEvent_t e : {h->ev0, h->ev1, h->ev2, h->ev3, h->ev_pw, h->ev_fork, h->ev_join, h->ev_xfer[0], h->ev_xfer[1]})
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : h->marks)
    if (e) hipEventDestroy(e);
  if (h->h_pw) hipHostFree(h->h_pw);
  for (void *p : h->h_xfer)
    if (p) hipHostFree(p);
  if (h->stream) hipStreamDestroy(h->stream);
  if (h->stream2) hipStreamDestroy(h->stream2);
  delete h;
  return FU_OK;
}

}  // extern "C"
