// Collect-all engine, piece 5 of 7 (see fu_ca_pack.h): struct fu_handle, the round context and
// the multi-GPU hooks. No device code: fu_dist.hip includes this piece alone and reads the
// handle's fields directly.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "fu_common.h"
#include "fu_plan.h"

namespace fu {
struct PackCtl;  // fu_ca_pack.h
}

// One round's launch context (state of round r-1 -> round r).
struct RoundCtx {
  int64_t r;
  int fm;                     // flow mode: rounds 1, 2 compute the old flows instead of reading them
  double *F;                  // F[r & 1]: f_{r-2} in, f_r out
  const double *ap, *ap2;     // a_{r-1}, a_{r-2}
  double *an;                 // a_r
  unsigned long long *err;    // error slot (nullptr: no check)
  bool plan;                  // a packing plan from a_{r-1} is still to run
};

// ======================================================================================
// handle
// ======================================================================================
constexpr int kPreMarks = 12;  // fu_mark slots created with the handle (a window's marks)

struct fu_handle {
  int device = 0;
  // layout 1 (fu_create_from_graph_ex): device node p = caller node old_of_new[p]; the
  // caller's row pointer maps flows back (rows moved as blocks)
  std::vector<int32_t> h_new_of_old;
  std::vector<int64_t> h_orig_rowptr;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;            // kernel 4's heavy tiles, concurrently (fork_heavy)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // autotune timing
  hipEvent_t ev2 = nullptr, ev3 = nullptr;  // fu_run_collectall_timed
  hipEvent_t marks[64] = {};                // fu_mark slots (the first kPreMarks at creation, others on first use)
  hipEvent_t r0_start = nullptr;            // fu_run_collectall_marked: mark 0 = the start of k_round0,
  hipEvent_t r0_stop = nullptr;             //   mark 1 (when it follows round 0) = its end
  hipEvent_t ev_pw = nullptr, ev_fork = nullptr, ev_join = nullptr;
  int32_t n = 0;
  int64_t E = 0;
  int32_t na = 0;  // estimate slots: n local + ghost estimates (multi-GPU)
  int32_t max_deg = 0;
  int *rowptr = nullptr, *col = nullptr;
  int *blk_row = nullptr;  // round 0: row of edge b * kR0E for every block b, then of edge E - 1
  unsigned short *col16 = nullptr;  // kernel 4 narrow tiles: col - cbase[e >> 10] + 32768 (0 where wide)
  int *cbase = nullptr;             // per 1024-edge block: its first edge's row, or -1 (a column >= 32K ids away)
  std::vector<int32_t> h_cbase;
  double *v = nullptr;
  double *f[2] = {nullptr, nullptr};           // F[r & 1]: f_{r-2} in, f_r out (split words)
  double *a[3] = {nullptr, nullptr, nullptr};  // A[r % 3] = a_r
  double *target = nullptr;
  unsigned long long *err = nullptr;
  int errcap = 0;
  double *ftmp = nullptr;
  int64_t rounds = 0;
  int kernel = 4;        // 4 = recon (LDS tiles), 8 = stage (LDS-staged slices + recon tiles)
  int geo = 1;           // kernel 4 tile geometry (kGeoEdges x kGeoNodes)
  int hub_threshold = 128;  // rows above it run as heavy rows (R-MAT-24: 128 beat 64, 256, 512)
  int mega_hub = 8192;   // degree above which a row's (fr, er) pairs are staged by many blocks
  int wave_heavy = 1;    // kernel 4: heavy rows one per wave
  int mid_heavy = 1;     // kernel 9: heavy rows of <= 64 x kMidRL edges in a register-resident launch
  int tr_bpx = 32;       // kernel 9: k_transpose blocks per XCD (1 per CU), each looping over buckets; 0 = one per bucket
  int c16 = 1;           // kernel 4: narrow light tiles read 2-byte column offsets
  int multi_mid = 1;     // kernel 9: k_heavy_multi also takes the register launch's rows (257-1024)
  int split_hubs = 1;     // kernel 4: mega-hub tiles alone on the side stream
  int fork_heavy = 1;    // kernel 4: heavy tiles on stream2, concurrently with the light tiles
  bool autotune = true;  // kernel "auto": candidates timed on real rounds, fastest kept
  bool tuned = false;
  bool tune_for_width = false;  // the pending pass was armed by a packing-width change (poll_pack_width)
  bool tuning = false;     // inside an autotune pass: packing plans wait until it ends
  float tune_ms[8] = {};  // per candidate (tune_cands order), ms per round of the last pass
  int tune_out[8] = {};   // passes in which the candidate was > 1.3x the best (2: dropped)
  int n_tunes = 0;        // autotune passes so far (re-run when the packing width changes)
  int tuned_width = 0;    // packing width the last pass ran under
  int tune_cache[4] = {-1, -1, -1, -1};  // winner per packing width (0, 8, 16, 32), kept across fu_reset
  int *h_pw = nullptr;    // pinned copy of the plan's width, refreshed after each plan
  void *h_xfer[2] = {nullptr, nullptr};           // pinned bounce buffers of copy_out (kXfer bytes each)
  hipEvent_t ev_xfer[2] = {nullptr, nullptr};
  bool pw_pending = false;
  int *pw_dev = nullptr;      // h_pw as the device sees it (the plan kernels write the width there)
  bool plan_pending = false;  // a packing plan is due before the next round (from its table)
  std::vector<int64_t> h_rowptr;
  std::vector<int32_t> h_col;
  // kernel 4 tiles per geometry (all four built up front so autotuning can switch between
  // rounds): mega hubs, heavy rows, then light tiles
  int4 *tiles_geo[4] = {nullptr, nullptr, nullptr, nullptr};
  int *tnar_geo[4] = {nullptr, nullptr, nullptr, nullptr};  // per tile: narrow (col16) or not (int: a scalar load)
  int ntiles_geo[4] = {0, 0, 0, 0};
  int nheavy_geo[4] = {0, 0, 0, 0};  // leading non-light tiles
  int nbound_geo[4] = {0, 0, 0, 0};  // multi-GPU: light tiles with ghost neighbours, right after the heavy ones
  int niso_geo[4] = {0, 0, 0, 0};    // kernel 9: trailing light tiles of isolated rows only (k_isolated runs them)
  int iso0_geo[4] = {0, 0, 0, 0};    // ... their first row (rows [iso0, n) are isolated)
  fu::plan::Tiles tiles1;            // host copy of geometry 1's plan (kernel 9's schedule)
  int mid_geo[4][2] = {};            // heavy tiles [mid_geo[0], mid_geo[1]) lead with a row of 64 x (kHeavyRL, kMidRL] edges
  int multi_geo[4][2] = {};          // hrows offset and count of this geometry's sorted heavy rows
  int multi_heavy = 1;               // kernel 9: rows > 64 x kHeavyRL as k_heavy_multi blocks
  double *halo_a = nullptr;          // multi-GPU: the estimate buffer the round being launched writes
  std::vector<int32_t> h_hrows;
  int *hrows = nullptr;  // heavy rows of the wave-per-row tiles, longest first (per geometry)
  int n_hub = 0;
  int64_t hub_total = 0;
  int4 *hub_rows = nullptr;  // {node, row begin, row end, offset in hubxy}
  int *hub_blk = nullptr;    // per 256-edge block of the hub edges: the hub of its first edge
  int iso_rows = 1;           // kernel 9: trailing isolated-row tiles as k_isolated (1) or as light tiles (0)
  int multi_short = 1;        // kernel 9: the rows of 129-256 edges in the multi-row blocks too (1)
  int tr_nt = 1;              // kernel 9: non-temporal G_B stores in k_transpose (1)
  int *hub_off = nullptr;    // per mega tile: offset in hubxy
  double2 *hubxy = nullptr;  // (fr, er) per hub edge, staged each round
  // packed estimate table (see PackCtl): code[r & 1] = codes of a_r
  unsigned char *code[2] = {nullptr, nullptr};
  fu::PackCtl *pctl = nullptr;  // [0], [1]: per code table; [2]: current encoding plan
  int *psample = nullptr;   // gather targets sampled for the plan
  int n_psample = 0;
  int pack = 1;             // 0 = off
  int pack_every = 16;      // rounds between encoding plans
  int tile_edges = 1024;    // option shadow of geo
  int tile_nodes = 0;
  bool has_target = false;
  // kernel 8 (LDS-staged slices): light tiles of kStageTE x kStageTN, heavy rows as kernel 4
  // heavy tiles, one slice layout per table element width
  struct StageLayout {
    int P = 0, Q = 0, SN = 0, NB = 0;     // slices, blocks per slice, nodes per slice, blocks (P = 0: not built)
    int4 *brange = nullptr;               // per stage block: {begin, end} in G, slice, 0
    unsigned short *colS = nullptr;       // per G element: column offset in its slice
    unsigned short *sidx16 = nullptr;     // per light-tile edge (slice order): position | run << 10
    int *dtab = nullptr;                  // per light tile: kStageRuns run offsets (G index - m)
  };
  StageLayout st[4];                      // element bytes 1, 2, 4, 8
  bool st_ready = false;
  std::string st_why;                     // why no layout could be built (kernel 8 unavailable)
  int4 *st_tiles = nullptr;               // light tiles
  int st_ntiles = 0;
  int st_nbound = 0;                      // multi-GPU: leading light tiles with ghost neighbours
  int4 *st_heavy = nullptr;               // rows above the tile limit ({i, -1, b, e})
  int st_nheavy = 0;
  void *stG = nullptr;                    // staged estimates, 8 B per G element
  int seen_width = 0;                     // packing width the host last saw
  int st_force = -1;                      // tests: force layout 0..3 (element bytes 1, 2, 4, 8)
  std::vector<fu::plan::I4> h_light;      // host copy (layout construction)
  // kernel 9 (pregather): slice-major G_A, per-bucket run starts, edge-order Gb
  struct TransLayout {
    int P = 0, Q = 0, NB = 0, B = 0;      // slices, blocks per slice, stage blocks, buckets
    int Bh = 0;                           // buckets [0, Bh) hold the mega-hub rows' edges
    int Bm = 0;                           // buckets [0, Bm) hold every edge of the k_heavy_multi rows
    int4 *brange = nullptr;               // stage blocks: {begin, end} in G_A, slice, 0
    unsigned short *colS = nullptr;       // per G_A element: column offset in its slice
    unsigned short *pos16 = nullptr;      // per G_A element: position in its bucket
    int *offT = nullptr;                  // (B + 1) x P: G_A index where bucket b's run of slice s starts
    double *GA = nullptr;
    double *GBr[3] = {nullptr, nullptr, nullptr};  // G_B of round r in GBr[r % 3] (one buffer without lag)
    double *hist[2] = {nullptr, nullptr};          // lag: per parity, a_{r-2} of every lagged row
  };
  TransLayout tr;
  bool tr_ready = false;
  // kernel 9 option "lag" (k_heavy_multi<LAG>): per parity p, lagf[p] = F[p] holds f_{r'-2}
  // (not f_{r'}) on the lagged rows, r' = lag_round[p] the last round of that parity; the
  // lagged rows: lag_nmulti[p] heavy rows
  int lag = 1;
  int lagf[2] = {0, 0};
  int64_t lag_round[2] = {0, 0};
  int lag_nmulti[2] = {0, 0};
  std::string tr_why;
  int n_cu = 256;
  void *dist = nullptr;  // multi-GPU (fu_dist.hip)
};

extern "C" int fu__dist_round_hook(fu_handle *h, int phase);
extern "C" void fu__dist_free(fu_handle *h);
extern "C" int fu__dist_agree(fu_handle *h, int ok_local, int *ok_all);

namespace {

// Current estimate / flow buffers (A[r % 3] and F[r & 1] of the last round r).
inline double *cur_a(fu_handle *h) { return h->a[(int)((h->rounds + 2) % 3)]; }
inline double *cur_f(fu_handle *h) { return h->f[(int)((h->rounds + 1) & 1)]; }

}  // namespace
