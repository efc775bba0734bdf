/* fu.h — C ABI of libfu.so, the MI355X-native Flow Updating engine.
 *
 * Drop-in boundary. The reference (AvilaAndre/simgrid-flow-updating-implementation) has no
 * library API. Its "operator API" is the SimGrid actor contract of
 * flowupdating-collectall.py (CA) and flowupdating-pairwise.py (PW):
 *   e.load_platform(...)            CA:154 / PW:143
 *   e.register_actor("peer", Peer)  CA:156 / PW:145
 *   e.load_deployment(...)          CA:157 / PW:146
 *   e.run_until(10000)              CA:164 / PW:153
 *   the watcher + global_values     CA:131-148 / PW:120-137
 * Every `peer` actor and the SimGrid engine behind it are replaced by the entry points
 * below. Host-side Python (the `fu` package) binds them with ctypes, mirroring the
 * Engine/Peer surface. The integration stub is in INTEGRATION.md.
 *
 * Conventions: every function returns int status, 0 = FU_OK and < 0 = error;
 * fu_last_error() returns a thread-local message. All pointers are plain host pointers
 * owned by the caller unless stated. fp64 everywhere (Python float). Indices are int32
 * (n < 2^31, E < 2^31). Each handle owns one HIP stream. Calls on one handle are
 * stream-ordered and not reentrant.
 */
#ifndef FU_H_
#define FU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FU_OK 0
#define FU_ERR_ARG (-1)
#define FU_ERR_HIP (-2)
#define FU_ERR_ALLOC (-3)
#define FU_ERR_STATE (-4)
#define FU_ERR_GRAPH (-5)
#define FU_ERR_NCCL (-6)

/* Thread-local message for the last failing call on this thread. */
const char *fu_last_error(void);
/* ABI version (bumped when a signature changes). */
int fu_version(void);
/* Number of visible HIP devices (0 without a GPU; never an error on a CPU-only host). */
int fu_device_count(int32_t *out);
/* Free and total bytes of HBM on `device` (hipMemGetInfo): how large a graph still fits. */
int fu_mem_info(int32_t device, int64_t *free_bytes, int64_t *total_bytes);

/* ======================================================================================
 * Host graphs (native C++; no GPU needed)
 * Replaces the deployment parsing SimGrid does for `peer` actors: neighbour lists from
 * actors.xml (ACT:4-27) parsed by Peer.__init__ (CA:29-31, CA:38-40). CSR rows keep the
 * caller's neighbour order, because that order fixes the summation order (CA:106, 110).
 * Generators provide the synthetic BASELINE configs. All are seeded and deterministic
 * (SplitMix64 counter streams, independent of thread count).
 * ==================================================================================== */
typedef struct fu_graph fu_graph;

/* Undirected edge list -> symmetric CSR: drop self-loops, dedup, rows sorted by id. */
int fu_graph_from_edges(int32_t n, int64_t m, const int32_t *src, const int32_t *dst,
                        fu_graph **out);
/* CSR as given (row order kept). If require_symmetric, fails unless every i->j has j->i. */
int fu_graph_from_csr(int32_t n, const int64_t *rowptr, const int32_t *col,
                      int32_t require_symmetric, fu_graph **out);
/* Erdos-Renyi G(n, m): m uniform pairs, self-loops dropped, deduplicated, symmetrised. */
int fu_graph_gen_er(int32_t n, int64_t m, uint64_t seed, fu_graph **out);
/* Random d-regular graph (pairing model + edge switches). n*d must be even. */
int fu_graph_gen_rr(int32_t n, int32_t d, uint64_t seed, fu_graph **out);
/* R-MAT (scale, edge factor, a, b, c; d = 1-a-b-c), symmetrised and deduplicated. */
int fu_graph_gen_rmat(int32_t scale, int32_t edge_factor, double a, double b, double c,
                      uint64_t seed, fu_graph **out);
/* Random geometric graph: n points in the unit square, edge iff distance < radius.
 * Nodes are numbered in cell (x-major) order, which gives locality. */
int fu_graph_gen_rgg(int32_t n, double radius, uint64_t seed, fu_graph **out);
/* n, directed edge count, max degree, 1 if symmetric. */
int fu_graph_info(const fu_graph *g, int32_t *n, int64_t *e, int32_t *max_deg,
                  int32_t *symmetric);
/* Copy out; any output may be NULL. rev[e] = index of the reverse edge (symmetric only). */
int fu_graph_export(const fu_graph *g, int64_t *rowptr, int32_t *col, int32_t *rev);
int fu_graph_free(fu_graph *g);
/* Node relabelling for gather locality: node i of g becomes node new_of_old[i] of *out.
 * Rows move as blocks and keep their neighbour order (the summation order of
 * avg_and_send, CA:106 / CA:110), so a round on *out computes, per node, the same bits.
 * order 0: new_of_old is given (must be a permutation); order 1: degree descending, ties
 * by id (the nodes most gathered first), written to new_of_old. rev follows the rows. */
int fu_graph_relabel(const fu_graph *g, int32_t order, int32_t *new_of_old, fu_graph **out);
/* value[i] = lo + (hi - lo) * U_i, U_i = (splitmix64(seed + (i+1)*0x9E3779B97F4A7C15) >> 11) * 2^-53 */
int fu_values_uniform(int64_t n, uint64_t seed, double lo, double hi, double *out);

/* ======================================================================================
 * Synchronous collect-all engine — THE HOT PATH.
 * One call to fu_run_collectall(h, R, ...) = R generation-synchronous rounds. Each round
 * is Peer.on_receive (CA:93-103) for every directed edge, then Peer.avg_and_send
 * (CA:105-128) for every node, as one data-parallel pass in HBM.
 * Round 0 = the timeout fire on zero state (CA:33-34, CA:87-91). The graph must be
 * symmetric (rev index). Results are bitwise equal to the reference's Python floats.
 * ==================================================================================== */
typedef struct fu_handle fu_handle;

/* rowptr[n+1], col[e], rev[e] (rev may be NULL: computed natively), value[n].
 * Arguments are checked before any HIP call and before any array is walked, also on a host
 * without a GPU: the scalars, e, rowptr's ends, rowptr monotone, col in range (FU_ERR_ARG),
 * then the graph (FU_ERR_GRAPH); fu_dist_create(_local) report a bad local CSR under the
 * same "fu_create: ..." texts.
 * A row that holds its own id is refused by every entry point that takes raw arrays (this
 * one, fu_batch_create, fu_lossy_create(_k), fu_churn_create(_k), fu_pair_create,
 * fu_dist_create(_local) for a local column equal to its local row, fu_churn_live,
 * fu_pair_matching) as fu_graph_from_csr refuses it: FU_ERR_GRAPH, "<entry point>: self-loop
 * at node i" (both partitioned entry points say "fu_dist_create"). */
int fu_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
              const int32_t *rev, const double *value, int32_t device, fu_handle **out);
int fu_create_from_graph(const fu_graph *g, const double *value, int32_t device,
                         fu_handle **out);
/* layout 0 = as fu_create_from_graph; 1 = the device graph is relabelled by degree
 * (fu_graph_relabel order 1) so the most-gathered estimates share cache lines. value,
 * targets, estimates and flows stay in the caller's numbering: the handle maps them. */
int fu_create_from_graph_ex(const fu_graph *g, const double *value, int32_t device,
                            int32_t layout, fu_handle **out);
/* Options (fu_set_option; FU_ERR_ARG for an unknown key or value):
 * "kernel"        0 = auto (fu_tune / autotuned between rounds), 4 = recon (LDS tiles, flow
 *                 reconstruction, direct estimate gathers), 8 = stage (estimates staged slice
 *                 by slice through LDS; single GPU, needs a slice layout), 9 = pregather
 *                 (stage + per-bucket transpose into edge order; single GPU, <= 2^25 nodes).
 *                 All kernels are bitwise equal. On an RCCL rank (fu_dist_create) this
 *                 option is collective: every rank sets it, and a kernel whose layout fails
 *                 on one rank (the slice limits count ghost slots, so they are rank-local)
 *                 fails with FU_ERR_STATE on every rank, so no rank starts rounds alone.
 *                 Kernel 9 on partitions sends its halo after the round (no overlap): it is
 *                 meant for the in-process transport and power-law graphs; auto never picks it.
 * "tile_edges"    kernel 4 tile edges: 2048, 1024 (default) or 512; "tile_nodes" 0/128/256.
 * "hub_threshold" rows of higher degree run as heavy rows, one wave each (default 128).
 * "mega_hub"      rows of higher degree run as mega hubs: one chain-only block each, their
 *                 (fr, er) staged by many blocks (default 8192).
 * "wave_heavy"    heavy rows one per wave (1, default) or one per block (0).
 * "fork_heavy"    kernel 4: heavy tiles on a side stream beside the light tiles (default 1).
 * "split_hubs"    kernel 4: only the mega-hub tiles on the side stream (default 1).
 * "mid_heavy"     kernel 9: heavy rows of 257-1024 edges in a launch of their own that keeps
 *                 the whole row in registers (default 1).
 * "tr_bpx"        kernel 9: transpose blocks per XCD, each looping over buckets (default 32;
 *                 0 = one block per bucket).
 * "multi_heavy"   kernel 9: rows of more than 256 edges as multi-row chain blocks (default 1);
 *                 "multi_mid" 0 keeps the rows of 257-1024 edges in the register launch.
 * "lag"           kernel 9: the multi-row heavy rows leave f_r unwritten and write f_{r-2}
 *                 from f_{r-4} and their kept a_{r-4}, two rounds later (default 1); the
 *                 lagged flows are finalized before fu_get_flows, other kernels and rebuilds.
 * "iso_rows"      kernel 9: the trailing run of degree-0 rows (the degree layout's last rows)
 *                 runs as one thread per row (k_isolated, 1, default) or as light tiles (0).
 * "multi_short"   kernel 9: the rows of 129-256 edges run in the multi-row blocks too (default 1;
 *                 0: one row per wave, four per block).
 * "tr_nt"         kernel 9: k_transpose's G_B stores non-temporal (default 1; its G_A loads are plain
 *                 since round 5: non-temporal loads measured slower, profiles/r05/u).
 * "c16"           kernel 4: 2-byte column offsets for light tiles whose columns lie within
 *                 32K ids of their 1024-edge block's first row (default 1).
 * "pack"          gather lossless 8/16/32-bit codes of the estimates once they cluster
 *                 (default 1); "pack_every" rounds between encoding plans (default 16).
 * "stage_layout"  kernel 8, tests: -1 = by packing width, 0..3 = the 1/2/4/8-byte layout.
 * "staged_lo"     accepted and ignored: kernel 8 loads its staged indices ahead of the flows;
 *                 the interleaved order (0) measured slower and is gone.
 * Removed after measurement (FU_ERR_ARG; the numbers are in DESIGN.md §4 and
 * profiles/MEASUREMENTS.md): "tr_pipe", "hub_prio", "side_tiles", "split_tr", "hub_multi",
 * "hub_blocks", "fuse", "light_geo", "tr_hot" (kernel 9), "hub_cus" / "hub_cu_stride" (the
 * hub path on CU-masked streams, profiles/r05/b), "st_split" (kernel 8's next stage beside
 * this round's tiles, profiles/r05/c), "nt" (kernel 4's non-temporal column loads) and "g56"
 * (kernel 8's 7-byte staged codes, profiles/r06/g). */
int fu_set_option(fu_handle *h, const char *key, int64_t value);
/* Zero the state: the next round run is round 0. Kernel "auto": the unpacked width's cached
 * winner is back in use (autotune done); a handle never tuned unpacked has a pass pending. */
int fu_reset(fu_handle *h);
/* Per-node convergence targets (e.g. exact component means) for the error check. */
int fu_set_targets(fu_handle *h, const double *target);
/* Run `rounds` rounds. If err_every > 0 (targets required), err_trace receives
 * max_i |a_i - target_i| after every err_every-th round (rounds / err_every entries).
 * Asynchronous unless err_trace != NULL. */
int fu_run_collectall(fu_handle *h, int32_t rounds, int32_t err_every, double *err_trace);
/* Same, timed with HIP events on the handle's stream: *ms = elapsed device time of the
 * whole region (synchronises). */
int fu_run_collectall_timed(fu_handle *h, int32_t rounds, float *ms);
/* Kernel "auto": one autotune pass now, at the current packing width, on real rounds
 * (1 warm + 8 timed per candidate, 2 more to confirm a slow warm round before the candidate
 * is dropped; ~45-55 rounds; round 0 first if none ran; packing plans wait). The rounds
 * advance the state: call fu_reset before a run that must start from zero. The winner is
 * kept across fu_reset. Synchronises. Lets a caller tune outside a timed region. */
int fu_tune(fu_handle *h);
/* A timed window in one call: runs rounds_at[n_marks - 1] rounds and records mark k (the
 * event of fu_mark slot k) once rounds_at[k] of them are queued (non-decreasing, rounds_at[0]
 * = 0 marks the start; n_marks <= 64). A single-GPU window that starts at round 0 takes mark 0
 * from round 0's own kernel start and, when rounds_at[1] == 1, mark 1 from its end (events of
 * the launch itself: an event on the idle stream ahead of it would hold the dispatch latency).
 * Asynchronous; read the times with fu_mark_elapsed. bench.py times its windows with it. */
int fu_run_collectall_marked(fu_handle *h, int32_t n_marks, const int32_t *rounds_at);
/* Record HIP event `slot` (0..63) on the handle's stream (asynchronous). */
int fu_mark(fu_handle *h, int32_t slot);
/* *ms = device time between two recorded marks (waits for `to`). */
int fu_mark_elapsed(fu_handle *h, int32_t from, int32_t to, float *ms);
/* max_i |a_i - target_i| on the current estimates (synchronises). */
int fu_max_err(fu_handle *h, double *out);
/* Per-node estimate = last_avg (CA:114, CA:56-63). */
int fu_get_estimates(fu_handle *h, double *a_out);
/* Per-directed-edge flow f[e] = flows[col[e]] of node i (CA:117-118), CSR order. */
int fu_get_flows(fu_handle *h, double *f_out);
int fu_get_round(fu_handle *h, int64_t *rounds_done);
/* info[0] = kernel in use, [1] = nt, [2] = autotune (0 off, 1 pending, 2 done),
 * [3] = rounds done, [4]/[5] = kernel 4 tile geometry (edges / nodes), [6] = autotune
 * passes, [7] = packing width of the last pass, [8..12] = the last pass's ns per round for
 * its candidates (kernel 4 at 2048x256, kernel 4 at 512x64, kernel 8, kernel 4 at
 * 1024x128, kernel 9; 0 = not run), [20] = mega hubs, [23..26] = the autotune winner per
 * packing width 0, 8, 16, 32 (kernel * 10 + kernel-4 geometry index, -1 = not tuned yet),
 * [27..30] = kernel 8 slices per layout (element bytes 1, 2, 4, 8; 0 = not built).
 * With kernel "auto" (the default) fu_tune, or a run with enough rounds left, times the
 * candidates on real rounds (they share state and are bitwise identical) and keeps the
 * fastest; the pass re-runs when the packing plan changes width. */
int fu_get_info(fu_handle *h, int64_t info[32]);  /* ABI 2: 32 entries */
/* Packed estimate table widths (0 = doubles): [0]/[1] = the code tables of the last
 * even/odd round, [2] = the current encoding plan (synchronises). */
int fu_get_pack(fu_handle *h, int32_t width[3]);
int fu_synchronize(fu_handle *h);
int fu_destroy(fu_handle *h);
/* Measurement helper (no reference counterpart): the device's streaming rate, a float4
 * copy of `bytes` bytes (read + write counted) repeated `iters` times on `device`, best of
 * the repetitions in GB/s. bench.py reports it beside the roofline (roofline.copy_GBs) so a
 * slow box reads as a slow copy too. */
int fu_copy_bandwidth(int32_t device, int64_t bytes, int32_t iters, double *gbs);

/* ======================================================================================
 * Batched collect-all engine: K value columns (1 <= K <= 16) over one graph, one pass per
 * round. Each column is an independent scalar run of the engine above (the same arithmetic,
 * bitwise equal to K separate handles): AVG, COUNT, SUM, moments and histogram bins of one
 * network share the column indices, the row structure and one K-wide estimate gather per
 * edge. value, target and estimates are node-major ([i * k + c]); flows are edge-major
 * ([e * k + c]) in the caller's CSR order. The graph must be symmetric. Arguments are
 * checked before any HIP call: k outside 1..16 is FU_ERR_ARG, an asymmetric graph
 * FU_ERR_GRAPH, also on a host without a GPU. No options: one kernel, every degree.
 * ==================================================================================== */
typedef struct fu_batch fu_batch;

/* rowptr[n+1], col[e], rev[e] (rev may be NULL: symmetry is checked natively), value[n*k]. */
int fu_batch_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                    const int32_t *rev, int32_t k, const double *value, int32_t device,
                    fu_batch **out);
int fu_batch_create_from_graph(const fu_graph *g, int32_t k, const double *value,
                               int32_t device, fu_batch **out);
/* Zero the state: the next round run is round 0. */
int fu_batch_reset(fu_batch *b);
/* Run `rounds` rounds. If err_every > 0 (targets required), err_trace receives, after every
 * err_every-th round, max_i |a[i][c] - target[i][c]| per column: (rounds / err_every) * k
 * entries, round-major. A NaN in one column makes only that column's entries NaN.
 * Asynchronous unless err_every > 0. */
int fu_batch_run(fu_batch *b, int32_t rounds, int32_t err_every, double *err_trace);
/* Same rounds, timed with HIP events on the handle's stream (synchronises). */
int fu_batch_run_timed(fu_batch *b, int32_t rounds, float *ms);
/* Per-node, per-column convergence targets, target[n*k]. */
int fu_batch_set_targets(fu_batch *b, const double *target);
/* out[k]: max_i |a[i][c] - target[i][c]| on the current estimates (synchronises). */
int fu_batch_max_err(fu_batch *b, double *out);
int fu_batch_get_estimates(fu_batch *b, double *a_out /* n*k */);
int fu_batch_get_flows(fu_batch *b, double *f_out /* e*k */);
int fu_batch_get_round(fu_batch *b, int64_t *rounds_done);
int fu_batch_synchronize(fu_batch *b);
int fu_batch_destroy(fu_batch *b);

/* ======================================================================================
 * Lossy collect-all engine: the synchronous round of the engine above with a loss model.
 * In round r >= 1, slot k = (i -> j) of row i either received the message j -> i of round
 * r - 1 (F = -f[rev k], E = a[j]; CA:98-99) or lost it, and node i fires on the pair it
 * stored itself (F = f[k], E = a[i]; CA:87-91, CA:117-119). Then, as everywhere,
 * S = 0.0 + F.., T = 0.0 + E.. in row order, a = ((v - S) + T) / (deg + 1), f = (F + a) - E.
 * Slot k of round r is lost iff down[k] != 0 or
 *   u01(splitmix64_at(splitmix64_at(seed, r), k)) < p
 * (the counter streams of fu_values_uniform; k = the caller's slot index, r = rounds since the
 * last reset): a pure function of (seed, r, k, p), so run(17) equals run(5); run(12), and
 * fu_lossy_delivered restates it on the host. p = 0 with no mask is bit-equal to
 * fu_run_collectall; p = 1 loses everything. Round 0 delivers nothing. The reverse flow is
 * gathered through rev (the flow reconstruction of the other engines needs every message to
 * arrive). Arguments are checked before any HIP call, also on a host without a GPU.
 * ==================================================================================== */
typedef struct fu_lossy fu_lossy;

/* rowptr[n+1], col[e], rev[e] (rev may be NULL: built natively), value[n]. A caller's rev is
 * validated (in range, rev[rev[k]] == k, col[rev[k]] == row of k): FU_ERR_GRAPH otherwise,
 * as for an asymmetric graph. */
int fu_lossy_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                    const int32_t *rev, const double *value, int32_t device, fu_lossy **out);
int fu_lossy_create_from_graph(const fu_graph *g, const double *value, int32_t device,
                               fu_lossy **out);
/* K value columns over one graph under one loss pattern, 1 <= k <= 16 (else FU_ERR_ARG):
 * value[n*k], node-major (value[i*k + c]). One message carries all k (flow, estimate) pairs, so
 * the loss decision, the mask and the statistics are per slot, exactly those of a handle of one
 * column with the same (seed, p, mask), and column c is bit-equal to a fu_lossy_create handle
 * run on column c alone. On such a handle every entry point below works with arrays scaled as in
 * fu_batch: set_values, set_targets and get_estimates take or return n*k doubles (x[i*k + c]),
 * get_flows returns e*k doubles (f[slot*k + c], the caller's slot order), the error trace has
 * (rounds / err_every) * k entries, round-major, and max_err writes out[k]. */
int fu_lossy_create_k(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                      const int32_t *rev, int32_t k, const double *value /* n*k */, int32_t device,
                      fu_lossy **out);
int fu_lossy_create_from_graph_k(const fu_graph *g, int32_t k, const double *value,
                                 int32_t device, fu_lossy **out);
/* The handle's number of columns (1 for fu_lossy_create). */
int fu_lossy_get_columns(fu_lossy *h, int32_t *k);
/* Loss probability and seed of the rounds run after the call (defaults 0, 0). p outside
 * [0, 1] or NaN: FU_ERR_ARG. */
int fu_lossy_set_loss(fu_lossy *h, double p, uint64_t seed);
/* down[e]: a non-zero byte loses slot k in every round run after the call (a link outage sets
 * both directions; both ends keep the neighbour). NULL clears the mask (the default). */
int fu_lossy_set_link_mask(fu_lossy *h, const uint8_t *down);
/* The inputs change (value[n]); flows, estimates and the round counter are kept. */
int fu_lossy_set_values(fu_lossy *h, const double *value);
/* Zero the state, the round counter and the statistics. Loss, mask and values are kept. */
int fu_lossy_reset(fu_lossy *h);
/* As fu_batch_run with the handle's k (1 for fu_lossy_create): (rounds / err_every) * k entries
 * of max_i |a[i][c] - target[i][c]|, round-major. */
int fu_lossy_run(fu_lossy *h, int32_t rounds, int32_t err_every, double *err_trace);
int fu_lossy_run_timed(fu_lossy *h, int32_t rounds, float *ms);
int fu_lossy_set_targets(fu_lossy *h, const double *target);
int fu_lossy_max_err(fu_lossy *h, double *out);
int fu_lossy_get_estimates(fu_lossy *h, double *a_out /* n, or n*k */);
int fu_lossy_get_flows(fu_lossy *h, double *f_out /* e, or e*k */);
int fu_lossy_get_round(fu_lossy *h, int64_t *rounds_done);
/* out[0] = messages offered since the last reset (e per round >= 1), out[1] = how many of
 * them were lost (loss probability or mask). Synchronises. */
int fu_lossy_get_stats(fu_lossy *h, int64_t out[2]);
int fu_lossy_synchronize(fu_lossy *h);
int fu_lossy_destroy(fu_lossy *h);
/* Host only, no GPU: out[q] = 1 if slot first + q is delivered in round `round` under
 * (p, seed) with no mask, else 0 (round 0 delivers nothing). */
int fu_lossy_delivered(uint64_t seed, int64_t round, int64_t first, int64_t count, double p,
                       uint8_t *out);

/* ======================================================================================
 * Churn collect-all engine: the synchronous round over a fixed CSR whose nodes and links are
 * switched off and on between runs (nodes that crash or arrive, links that disappear or
 * return). A node that may ever join is in the graph from the start, switched off.
 *
 * State: per directed slot k = (i -> j), in the caller's CSR order, the flow f[k] and a slot
 * state UP, DOWN or FRESH; per node the estimate a[i], the input v[i] and alive[i].
 * Topology: the pair (alive[n], link_up[e]), given whole at every call, NULL = all ones;
 * link_up[k] != link_up[rev k] is FU_ERR_ARG. Slot k is live iff link_up[k] && alive[i] &&
 * alive[col k]. Applying a topology moves a slot
 *   live -> not live: DOWN. Both ends drop the neighbour; its flow entry is gone (f[k] = +0.0).
 *   not live -> live: FRESH. The neighbour was just added; nothing has been received from it.
 *   live -> live:     as it was (UP stays UP; FRESH stays FRESH if no round ran in between).
 * After create and after reset every live slot is FRESH and all state is zero, so round 0 is
 * the timeout fire on zero state without a special case.
 * Round r, alive node i: row i's slots in row order, the DOWN ones skipped;
 *   UP slot:    F = -f_old[rev k],  E = a_old[col k]          (CA:98-99)
 *   FRESH slot: F = 0.0,            E = 0.0                   (CA:33-34)
 *   S = 0.0 + F..,  T = 0.0 + E.. left to right,  d = the number of live slots,
 *   a_new[i] = ((v[i] - S) + T) / (double)(d + 1),
 *   f_new[k] = (F + a_new[i]) - E for the live slots, +0.0 for the DOWN ones;
 * after the round every FRESH slot is UP. A dead node does not fire (a_new[i] = a_old[i]) and
 * all its slots are DOWN; an alive node whose slots are all DOWN gets a = v.
 * With everything alive and up the rounds are bit-equal to fu_run_collectall; a topology set
 * before round 0 and never changed gives fu_run_collectall on the live subgraph (live slots
 * only, row order kept); run(17) equals run(5); run(12); after any sequence of events the
 * alive nodes converge to the mean of the alive inputs of their component of the live graph.
 * The reverse flow is gathered through rev, as in the lossy engine. Arguments are checked
 * before any HIP call, also on a host without a GPU.
 * ==================================================================================== */
typedef struct fu_churn fu_churn;

/* As fu_lossy_create (rev may be NULL: built natively; a caller's rev is validated). Everything
 * starts alive and up. */
int fu_churn_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                    const int32_t *rev, const double *value, int32_t device, fu_churn **out);
int fu_churn_create_from_graph(const fu_graph *g, const double *value, int32_t device,
                               fu_churn **out);
/* K value columns over one graph under one topology, 1 <= k <= 16 (else FU_ERR_ARG): value[n*k],
 * node-major. Topology, slot states and statistics are per node and per slot as for one column
 * (get_slot_state stays e bytes); a slot that goes DOWN loses all its k flow entries; column c is
 * bit-equal to a fu_churn_create handle run on column c alone. The arrays of the entry points
 * below scale as for fu_lossy_create_k; the error entries are per column over the alive nodes,
 * and a NaN raises only its own column's. */
int fu_churn_create_k(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                      const int32_t *rev, int32_t k, const double *value /* n*k */, int32_t device,
                      fu_churn **out);
int fu_churn_create_from_graph_k(const fu_graph *g, int32_t k, const double *value,
                                 int32_t device, fu_churn **out);
/* The handle's number of columns (1 for fu_churn_create). */
int fu_churn_get_columns(fu_churn *h, int32_t *k);
/* alive[n] and link_up[e], non-zero = on, NULL = all ones. Ordered behind the rounds already
 * queued; complete on return. */
int fu_churn_set_topology(fu_churn *h, const uint8_t *alive, const uint8_t *link_up);
/* The inputs change (value[n]); flows, estimates, states and the round counter are kept. */
int fu_churn_set_values(fu_churn *h, const double *value);
/* Zero the state and the round counter; topology and values are kept; live slots FRESH. */
int fu_churn_reset(fu_churn *h);
/* As fu_lossy_run, but the error entries are the maximum of |a_i - target_i| over the alive
 * nodes only (+0.0 if none is alive). */
int fu_churn_run(fu_churn *h, int32_t rounds, int32_t err_every, double *err_trace);
int fu_churn_run_timed(fu_churn *h, int32_t rounds, float *ms);
int fu_churn_set_targets(fu_churn *h, const double *target);
int fu_churn_max_err(fu_churn *h, double *out);
int fu_churn_get_estimates(fu_churn *h, double *a_out /* n, or n*k */);
int fu_churn_get_flows(fu_churn *h, double *f_out /* e, or e*k */);
int fu_churn_get_round(fu_churn *h, int64_t *rounds_done);
/* out[0] = alive nodes, out[1] = live directed slots, of the current topology. */
int fu_churn_get_stats(fu_churn *h, int64_t out[2]);
/* state_out[e]: 0 UP, 1 DOWN, 2 FRESH. */
int fu_churn_get_slot_state(fu_churn *h, uint8_t *state_out);
int fu_churn_synchronize(fu_churn *h);
int fu_churn_destroy(fu_churn *h);
/* Host only, no GPU: live_out[k] (e = rowptr[n] bytes) of a topology; alive, link_up and rev
 * may be NULL. FU_ERR_ARG if link_up is not symmetric under rev or the CSR is malformed,
 * FU_ERR_GRAPH for an asymmetric graph or a bad rev. */
int fu_churn_live(int32_t n, const int64_t *rowptr, const int32_t *col, const int32_t *rev,
                  const uint8_t *alive, const uint8_t *link_up, uint8_t *live_out);

/* ======================================================================================
 * Synchronous pairwise engine: every round a matching of the graph is chosen on the device
 * and each matched pair runs one full pairwise exchange. State: per directed slot k (the
 * caller's CSR order) the flow f[k] and the cached estimate c[k], per node last[i] (last_avg,
 * PW:107); all zero after create and after reset. The graph must be symmetric.
 *
 * The matching of round r (r = rounds since the last reset; round 0 is an ordinary round),
 * with key = splitmix64_at(seed, r) and h_i = splitmix64_at(key, i) (the counter streams of
 * fu_values_uniform): a node of degree 0 is idle; node i proposes iff h_i & 1, else it
 * listens; a proposer picks slot p_i = (h_i >> 1) % deg_i (unsigned 64-bit) and with it
 * j = col[rowptr[i] + p_i]; the proposal is valid iff j listens; a listener with valid
 * proposals accepts the one with the smallest ((h_i >> 32) << 32) | i. The accepted i is the
 * pair's initiator, s = p_i, t = rev[rowptr[i] + s] - rowptr[j]. A pure function of (seed, r,
 * graph): it does not depend on the launch shape, run(17) equals run(5); run(12), and
 * fu_pair_matching restates it on the host.
 *
 * The exchange of a pair (i, s, j, t), without contraction:
 *   1. i fires on s (PW:102-117): S = 0.0 + f[row i].. in row order, x = v_i - S,
 *      a = (c[s] + x) / 2.0, f[s] = (f[s] + a) - c[s], c[s] = a, last[i] = a; message (f[s], a).
 *   2. j receives (PW:98-99): c[t] = A, f[t] = -F; then j fires on t as in 1 (S over the whole
 *      row j with the new f[t]); last[j] is set; message (f[t], a_j).
 *   3. i receives: c[s] = a_j, f[s] = -f[t]. Node i does NOT fire again.
 * Step 3 is the one deviation from the reference: at PW:100 every receive answers with a fire,
 * so the ping-pong between two peers never ends; here it stops after one answer. That leaves f
 * antisymmetric on the pair, and in exact arithmetic both ends then hold (x_i + x_j) / 2: the
 * mass is conserved and the run is gossip averaging over the matching. Rows of different
 * pairs are disjoint, so a round updates the state in place.
 *
 * Message loss (fu_pair_set_loss, fu_pair_set_link_mask; off by default). The matching does not
 * look at the loss or the mask: a peer cannot know that its message will be lost, and an
 * initiator that proposes over a dead link fires into it. With ks = rowptr[i] + s and
 * kt = rowptr[j] + t, a pair has two messages: m1 goes i -> j and is received on slot kt, m2
 * goes j -> i and is received on slot ks. A message is lost by the slot that would receive it:
 * the message received on slot k in round r is lost iff down[k] != 0 or
 * u01(splitmix64_at(splitmix64_at(~loss_seed, r), k)) < p, u01(x) = (x >> 11) * 2^-53. The
 * complement keeps the loss stream apart from the matching's when both seeds are one number.
 * Round 0 is an ordinary round (fu_lossy's round 0 delivers nothing; this one can). A pure
 * function of (loss_seed, r, k, p): fu_pair_lost restates it on the host. The outcomes:
 *   m1 lost:       step 1 alone: f[ks] = F1, c[ks] = a_i, last[i] = a_i. Node j does nothing: its
 *                  row is not read or written, it does not count as having fired, no m2 exists.
 *   m2 lost:       steps 1 and 2; node i keeps what it fired, f[ks] = F1, c[ks] = a_i.
 *   both arrive:   steps 1 to 3, the lossless exchange bit for bit.
 * Each is the reference's avg_and_send / on_receive with one message not handed over. After a
 * lost answer the two ends of the link hold flows that do not negate each other; the next
 * message delivered over it, in either direction, restores that (PW:98-99). With p = 0 and no
 * mask the handle launches the lossless kernels; with p = 1 every initiator fires alone.
 * Arguments are checked before any HIP call, also on a host without a GPU.
 *
 * Churn (fu_pair_set_topology; after create every slot is live). The topology is fu_churn's:
 * the pair (alive[n], link_up[e]) given whole at every call, slot k = (i -> j) live iff
 * link_up[k] && alive[i] && alive[j] (fu_churn_live). A call moves a slot
 *   live -> not live: f[k] = c[k] = +0.0 in every column, on both ends (both drop the neighbour
 *                     and its `flows` and `estimates` entries, whatever a lost answer left there);
 *   not live -> live: nothing: the cells hold +0.0, a neighbour just added (PW:33-34, PW:94-96);
 *   live -> live:     as it was.
 * last, the fired flags and the values are untouched. The matching of a round is the rule above
 * on the live subgraph: with ldeg_i the live slots of row i, a dead node or one with ldeg_i == 0
 * is idle, a proposer takes its p_i-th live slot in row order, p_i = (h_i >> 1) % ldeg_i, and
 * validity and priority are unchanged; fu_pair_matching_live restates it on the host. The
 * exchange is unchanged but for the chosen slot, and a fire's sum S runs over the live slots
 * only. Loss and mask compose with no further rule: their decisions stay on the caller's slot
 * index. With everything live this is the engine without a topology, bit for bit. Once a
 * topology has been set, max_err and the error trace run over the alive nodes only (+0.0 if none).
 * ==================================================================================== */
typedef struct fu_pair fu_pair;

/* rowptr[n+1], col[e], rev[e] (rev may be NULL: built natively), value[n]; n >= 1. A caller's
 * rev is validated as by fu_lossy_create: FU_ERR_GRAPH otherwise, as for an asymmetric graph. */
int fu_pair_create(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                   const int32_t *rev, const double *value, int32_t device, fu_pair **out);
int fu_pair_create_from_graph(const fu_graph *g, const double *value, int32_t device,
                              fu_pair **out);
/* K value columns over one graph and one matching, 1 <= k <= 16 (else FU_ERR_ARG): value[n*k],
 * node-major (value[i*k + c]). One message carries all k (flow, estimate) pairs, so the matching
 * of a round, the three loss outcomes of a pair, the link mask, the statistics and the loss
 * statistics are per handle, exactly those of a handle of one column with the same graph and
 * seeds, and column c (last, f and c after every round) is bit-equal to a fu_pair_create handle
 * run on column c alone; no arithmetic crosses columns. On such a handle every entry point below
 * works with arrays scaled as for fu_lossy_create_k: set_values, set_targets and get_estimates
 * take or return n*k doubles (x[i*k + c]), get_flows and get_cache return e*k doubles
 * (f[slot*k + c], the caller's slot order), the error trace has (rounds / err_every) * k entries,
 * round-major, max_err writes out[k] (a NaN raises only its own column's entry), and the link
 * mask stays e bytes. A handle made here with k = 1 is bit-equal to one of fu_pair_create. */
int fu_pair_create_k(int32_t n, int64_t e, const int64_t *rowptr, const int32_t *col,
                     const int32_t *rev, int32_t k, const double *value /* n*k */, int32_t device,
                     fu_pair **out);
int fu_pair_create_from_graph_k(const fu_graph *g, int32_t k, const double *value,
                                int32_t device, fu_pair **out);
/* The handle's number of columns (1 for fu_pair_create). */
int fu_pair_get_columns(fu_pair *h, int32_t *k);
/* Seed of the matchings of the rounds run after the call (default 0). */
int fu_pair_set_seed(fu_pair *h, uint64_t seed);
/* Loss probability and seed of the rounds run after the call (defaults 0, 0). p outside [0, 1]
 * or NaN: FU_ERR_ARG. */
int fu_pair_set_loss(fu_pair *h, double p, uint64_t seed);
/* down[e]: a non-zero byte loses every message received on slot k in the rounds run after the
 * call. NULL clears the mask. */
int fu_pair_set_link_mask(fu_pair *h, const uint8_t *down);
/* alive[n], link_up[e]: non-zero = on, NULL = all ones; the whole topology of the rounds run
 * after the call, queued behind the rounds already queued (synchronises). link_up must agree on
 * a slot and its reverse: FU_ERR_ARG naming the first offending slot, checked on the host before
 * any HIP call. fu_pair_reset keeps the topology. */
int fu_pair_set_topology(fu_pair *h, const uint8_t *alive, const uint8_t *link_up);
/* out[0] = alive nodes, out[1] = live directed slots of the current topology (n and e before
 * any topology call). */
int fu_pair_get_topology_stats(fu_pair *h, int64_t out[2]);
/* out[e]: 1 where the slot is live, else 0. */
int fu_pair_get_slot_live(fu_pair *h, uint8_t *out /* e */);
/* "match": how the device finds the matching, 0 = proposers push one 64-bit atomicMin per valid
 * proposal (default), 1 = every listener hashes its own row. Same matching, same bits; the
 * switch exists for the A/B of tools/bench_pair.py. Unknown key or value: FU_ERR_ARG. */
int fu_pair_set_option(fu_pair *h, const char *key, int64_t value);
/* The inputs change (value[n], or value[n*k]); flows, caches, last averages and the round counter
 * are kept. */
int fu_pair_set_values(fu_pair *h, const double *value);
/* Zero the state, the round counter and the statistics (the loss counters too). The seeds, the
 * loss, the mask, the topology and the values are kept. */
int fu_pair_reset(fu_pair *h);
/* Run `rounds` rounds. If err_every > 0 (targets required), err_trace receives, after every
 * err_every-th round, max_i |last_i - target_i| (rounds / err_every entries; the maximum is
 * taken over bit patterns, so one NaN makes the entry NaN). Asynchronous unless err_every > 0;
 * nothing inside a run waits for the host. */
int fu_pair_run(fu_pair *h, int32_t rounds, int32_t err_every, double *err_trace);
/* Same rounds, timed with HIP events on the handle's stream (synchronises). */
int fu_pair_run_timed(fu_pair *h, int32_t rounds, float *ms);
int fu_pair_set_targets(fu_pair *h, const double *target /* n, or n*k */);
/* max_i |last_i - target_i| on the current state, out[k] per column on a handle of k columns
 * (synchronises). */
int fu_pair_max_err(fu_pair *h, double *out);
/* last[n]: every node's average at its last fire (0.0 for a node that has not fired). */
int fu_pair_get_estimates(fu_pair *h, double *last_out /* n, or n*k */);
int fu_pair_get_flows(fu_pair *h, double *f_out /* e, or e*k */);
/* c[e]: the cached estimate of every slot. */
int fu_pair_get_cache(fu_pair *h, double *c_out /* e, or e*k */);
int fu_pair_get_round(fu_pair *h, int64_t *rounds_done);
/* out[0] = pairs exchanged since the last reset, out[1] = nodes that have never fired since
 * then. Synchronises. */
int fu_pair_get_stats(fu_pair *h, int64_t out[2]);
/* out[0] = first messages lost, out[1] = answers lost, out[2] = complete exchanges, since the
 * last reset; their sum is out[0] of fu_pair_get_stats, the matched pairs. Synchronises. */
int fu_pair_get_loss_stats(fu_pair *h, int64_t out[3]);
int fu_pair_synchronize(fu_pair *h);
int fu_pair_destroy(fu_pair *h);
/* Host only, no GPU: the matching of round `round` under `seed`. mate[i] = i's partner or -1,
 * initiator[i] = 1 for the proposer of a pair, else 0. */
int fu_pair_matching(int32_t n, const int64_t *rowptr, const int32_t *col, uint64_t seed,
                     int64_t round, int32_t *mate /* n */, uint8_t *initiator /* n */);
/* The same under a topology (alive[n], link_up[e], NULL = all ones; both NULL is
 * fu_pair_matching). The graph must be symmetric; link_up as for fu_pair_set_topology. */
int fu_pair_matching_live(int32_t n, const int64_t *rowptr, const int32_t *col,
                          const uint8_t *alive, const uint8_t *link_up, uint64_t seed,
                          int64_t round, int32_t *mate /* n */, uint8_t *initiator /* n */);
/* Host only, no GPU: out[q] = 1 if the message received on slot first + q in round `round` is
 * lost under (p, seed), no mask. */
int fu_pair_lost(uint64_t seed, int64_t round, int64_t first, int64_t count, double p,
                 uint8_t *out);

/* ======================================================================================
 * Tick-level replay (pairwise mode, and faithful collect-all on small platforms).
 * Replaces the SimGrid maestro + Peer.loop (CA:70-85 / PW:69-84): the loop's control flow
 * never depends on fp values, so the whole schedule is precomputed on the host as a trace.
 * The GPU then replays one tick per batch. Events of one tick are on distinct nodes and
 * touch only their own row and message slots, so they commute. Mailbox model: SURVEY.md
 * App. B.
 * ==================================================================================== */
#define FU_MODE_COLLECTALL 0
#define FU_MODE_PAIRWISE 1

#define FU_EV_RECV 0    /* {0, slot, msg_in, 0}     est[slot]=msg.a; flow[slot]=-msg.f (CA:98-99, PW:98-99) */
#define FU_EV_FIRE_CA 1 /* {1, k, out_off, 0}       avg over slots [0,k), k msgs to out_ids[out_off..] (CA:105-125) */
#define FU_EV_FIRE_PW 2 /* {2, slot, k, msg_out}    pairwise avg with slot; flows summed over [0,k) (PW:102-117) */

typedef struct fu_trace fu_trace;

/* Declared neighbour lists (ACT:4-27) in CSR: decl_rowptr[n+1], decl_col. ticks = number
 * of ticks simulated (t = 0 .. ticks-1). order: "fwd" | "rev" | "rand:<seed>" (intra-tick
 * actor order; SimGrid's real tie order is not observable offline). */
int fu_trace_build(int32_t n, const int64_t *decl_rowptr, const int32_t *decl_col,
                   int32_t mode, int32_t ticks, const char *order, fu_trace **out);
/* Same, with fault injection (not in the reference): faults =
 * "drop=P,delay=D:Q,seed=S" (any subset; NULL or "" = none). Each put is lost with
 * probability P or delayed by D ticks with probability Q (SplitMix64 stream in put order).
 * Lost messages exercise the timeouts (CA:87-91, PW:86-91). */
int fu_trace_build_ex(int32_t n, const int64_t *decl_rowptr, const int32_t *decl_col,
                      int32_t mode, int32_t ticks, const char *order, const char *faults,
                      fu_trace **out);
/* Same, with route transfer times: route_s[src * n + dst] = seconds
 * a message from src to dst takes (SimGrid's LV08 model: 13.01 * sum(latency) +
 * size / (0.97 * min bandwidth), fu/platform.py; no link sharing: fu_trace_build_links). A message
 * matched at tick t is consumed from tick t + floor(T) + 1 (t + 1 for T < 1 s, the only
 * case on the reference platform, CA:76). route_s NULL = every route under one tick. */
int fu_trace_build_routes(int32_t n, const int64_t *decl_rowptr, const int32_t *decl_col,
                          int32_t mode, int32_t ticks, const char *order, const char *faults,
                          const double *route_s, fu_trace **out);
/* Same, with link sharing (parity-unpinned against SimGrid): the
 * platform's links (bandwidth B/s, latency s, shared = 0 for FATPIPE) and every route
 * (route_links[route_off[src * n + dst] .. route_off[src * n + dst + 1]), n * n + 1 offsets;
 * an empty route = same host, or a pair the platform does not route: delivery within one
 * tick). A message matched at tick t starts a transfer at time t: lat_factor * sum(latency)
 * with no bandwidth, then msg_bytes at the max-min fair share of bw_factor * bandwidth on
 * every shared link it crosses (capped by its FATPIPE links); it is consumed at the first tick
 * after its end. Alone, a transfer takes the per-route time above (SimGrid LV08: lat_factor
 * 13.01, bw_factor 0.97, 154-byte messages). Every flow on a link gets an EQUAL max-min
 * share here; fu_trace_build_links_ex adds LV08's weighting by sharing penalty and the TCP
 * window bound (the drop-in Engine uses it). The reference platform's 154-byte transfers all
 * end within one tick, where every variant gives the plain schedule. */
int fu_trace_build_links(int32_t n, const int64_t *decl_rowptr, const int32_t *decl_col, int32_t mode,
                         int32_t ticks, const char *order, const char *faults, int32_t n_links,
                         const double *link_bw, const double *link_lat, const int32_t *link_shared,
                         const int64_t *route_off, const int32_t *route_links, double msg_bytes,
                         double lat_factor, double bw_factor, fu_trace **out);
/* fu_trace_build_links with SimGrid LV08's weighted sharing: a transfer's share of a shared
 * link is proportional to 1 / its sharing penalty, the route's latency sum + weight_S /
 * bandwidth of each of its links (LV08: weight_S = 20537), and with tcp_gamma > 0 its rate
 * is capped at tcp_gamma / (2 * latency sum), the TCP window (LV08: 4194304). weight_S = 0
 * and tcp_gamma = 0 are fu_trace_build_links. Parity-unpinned (SimGrid is not installable
 * offline); oracle/oracle.py's LinkNet restates it operation for operation. */
int fu_trace_build_links_ex(int32_t n, const int64_t *decl_rowptr, const int32_t *decl_col, int32_t mode,
                            int32_t ticks, const char *order, const char *faults, int32_t n_links,
                            const double *link_bw, const double *link_lat, const int32_t *link_shared,
                            const int64_t *route_off, const int32_t *route_links, double msg_bytes,
                            double lat_factor, double bw_factor, double weight_S, double tcp_gamma,
                            fu_trace **out);
/* fu_trace_build_links_ex with SimGrid's network/crosstraffic: every transfer also loads each
 * shared link of its reverse route (route dst -> src) with crosstraffic x its rate (the TCP
 * acknowledgements; SimGrid: 0.05), and a FATPIPE link of the reverse route alone caps it at
 * bw_factor * bandwidth / crosstraffic. crosstraffic = 0 is fu_trace_build_links_ex. SimGrid
 * enables it by default, but this repository keeps it OFF by default (the drop-in Engine
 * turns it on with --cfg=network/crosstraffic:1): its effect on a schedule cannot be pinned
 * offline, and on the reference platform every 154-byte transfer ends within its tick with or
 * without it. Parity-unpinned; oracle/oracle.py's LinkNet restates it operation for operation. */
int fu_trace_build_links_cross(int32_t n, const int64_t *decl_rowptr, const int32_t *decl_col, int32_t mode,
                               int32_t ticks, const char *order, const char *faults, int32_t n_links,
                               const double *link_bw, const double *link_lat, const int32_t *link_shared,
                               const int64_t *route_off, const int32_t *route_links, double msg_bytes,
                               double lat_factor, double bw_factor, double weight_S, double tcp_gamma,
                               double crosstraffic, fu_trace **out);
int fu_trace_fault_stats(const fu_trace *t, int64_t *dropped, int64_t *delayed);
/* info[0]=union edges, [1]=tasks, [2]=events, [3]=out_ids, [4]=message slots,
 * [5]=ticks, [6]=dynamic neighbour additions (CA:94-96 errors), [7]=messages sent. */
int fu_trace_info(const fu_trace *t, int64_t info[8]);
/* union_rowptr[n+1] / union_col: neighbour slots in insertion order (declared, then first
 * arrival). tick_task_off[ticks+1]; tasks[3*n_tasks] = (node, ev_begin, ev_end);
 * events[4*n_events]; out_ids[n_out_ids]; first_avg_seq[n] (order of first average:
 * key order of global_values["last_avg"], -1 = never averaged); fires[n]. Any may be NULL. */
int fu_trace_export(const fu_trace *t, int64_t *union_rowptr, int32_t *union_col,
                    int64_t *tick_task_off, int32_t *tasks, int32_t *events,
                    int32_t *out_ids, int64_t *first_avg_seq, int32_t *fires);
int fu_trace_free(fu_trace *t);

typedef struct fu_replay fu_replay;
/* Raw-array form (the trace arrays above, caller-owned). */
int fu_replay_create(int32_t n, const int64_t *rowptr, const double *value, int32_t ticks,
                     const int64_t *tick_task_off, int64_t n_tasks, const int32_t *tasks,
                     int64_t n_events, const int32_t *events, int64_t n_out_ids,
                     const int32_t *out_ids, int64_t n_msgs, int32_t device,
                     fu_replay **out);
int fu_replay_create_from_trace(const fu_trace *t, const double *value, int32_t device,
                                fu_replay **out);
/* Run ticks [current, tick_end). snaps[k*n .. ] receives last_avg after tick
 * snap_ticks[k] (ascending, within the range); snaps may be NULL if n_snap == 0. */
int fu_replay_run(fu_replay *r, int32_t tick_end, int32_t n_snap, const int32_t *snap_ticks,
                  double *snaps);
/* Timed variant: *ms = device time of the tick kernels (synchronises). */
int fu_replay_run_timed(fu_replay *r, int32_t tick_end, float *ms);
int fu_replay_get(fu_replay *r, double *last_avg, double *flows, double *est);
/* "persistent" = 1: one launch for all ticks in dataflow order (per-node event streams,
 * unique message slots tagged by a sentinel); 0 = one launch per tick (default). Same bits.
 * "persistent_reg" = 1 (default): in persistent mode, when every node's thread can be
 * resident and the degree is <= 16, each thread keeps its node's state in registers.
 * "persistent_blocks", tests: B >= 1 = the generic persistent kernel launches min(B, its
 * occupancy-derived grid) blocks, so each thread owns several nodes; 0 = that grid
 * (default). Before the first tick only (FU_ERR_STATE after); negative = FU_ERR_ARG. No
 * effect on the register kernel. */
int fu_replay_set_option(fu_replay *r, const char *key, int64_t value);
/* Which path a handle runs (read-only; in persistent mode it builds the per-node event
 * streams if they are not built yet, as "persistent" = 1 does):
 * info[0] persistent mode on; info[1] the register kernel will be used; info[2] its row
 * registers (8 or 16; 0 if not used); info[3] the trace holds collect-all fires; info[4]
 * blocks of the generic persistent launch (0 before the streams are built); info[5] unique
 * message slots (likewise); info[6] max union degree; info[7] current tick. */
int fu_replay_get_info(fu_replay *r, int64_t info[8]);
int fu_replay_destroy(fu_replay *r);

/* ======================================================================================
 * Multi-GPU (one process per GPU, RCCL over xGMI). The graph is partitioned into
 * contiguous node ranges. Each rank holds its rows plus ghost slots for the reverse flows
 * and estimates of cut edges. One halo exchange per round (ncclSend/ncclRecv to each
 * neighbouring part in one group) replaces the simulated mailboxes (CA:74, CA:124).
 * ==================================================================================== */
#define FU_UNIQUE_ID_BYTES 128
int fu_dist_unique_id(uint8_t *id_out /* FU_UNIQUE_ID_BYTES */);
/* Local part, in local numbering:
 *   n_local rows (global ids [row_begin, row_begin + n_local)), rowptr[n_local+1];
 *   col[e]: < n_local = local node, >= n_local = ghost estimate slot (n_local + g);
 *   rev[e]: < e_local = local edge, >= e_local = ghost flow slot (e_local + q).
 * Halo plan (per peer rank, CSR over peers):
 *   send_f_off[nranks+1] / send_f_idx: local edges whose flow goes to each peer, in the
 *     order that peer stores them in its ghost flow slots;
 *   recv_f_off[nranks+1]: ghost flow slots per peer (contiguous, peer order);
 *   send_a_off / send_a_idx, recv_a_off: the same for estimates of boundary nodes.
 * The round kernels rebuild the neighbours' flows from estimates (flow reconstruction), so
 * the halo carries estimates only: rev must be NULL, n_ghost_f 0 and the flow plan empty
 * (send_f_off / recv_f_off all zero; the parameters stay for ABI stability). */
int fu_dist_create(int32_t n_local, int64_t e_local, const int64_t *rowptr,
                   const int32_t *col, const int32_t *rev, const double *value,
                   int32_t n_ghost_a, int64_t n_ghost_f, int32_t nranks, int32_t rank,
                   const int64_t *send_f_off, const int32_t *send_f_idx,
                   const int64_t *recv_f_off, const int64_t *send_a_off,
                   const int32_t *send_a_idx, const int64_t *recv_a_off,
                   const uint8_t *unique_id, int32_t device, fu_handle **out);

/* In-process transport (one process, e.g. all ranks on one GPU): the same rank handle
 * without a communicator, and the same comm-stream / event chain as RCCL. Each round packs
 * the rank's boundary estimates on its comm stream behind the boundary tiles; after every
 * rank has launched round r, fu_dist_exchange_local(hs, nranks) queues, on each receiver's
 * comm stream, device copies of its peers' packed slots into its ghost slots (the order
 * RCCL uses), beside the interior tiles of round r; round r + 1 waits for them. No host
 * synchronisation. Errors: FU_ERR_STATE if the ranks have run different numbers of rounds
 * or round r's halo was already exchanged. fu_dist_run_local runs `rounds` rounds of every
 * rank, each followed by the exchange. The error all-reduce is left to the caller. This
 * exercises the ghost-slot reads, the pack kernel and the overlapped halo ordering without
 * a multi-GPU box (two RCCL ranks cannot share one GPU). */
int fu_dist_create_local(int32_t n_local, int64_t e_local, const int64_t *rowptr,
                         const int32_t *col, const double *value, int32_t n_ghost_a,
                         int32_t nranks, int32_t rank, const int64_t *send_a_off,
                         const int32_t *send_a_idx, const int64_t *recv_a_off, int32_t device,
                         fu_handle **out);
int fu_dist_exchange_local(fu_handle **hs, int32_t nranks);
int fu_dist_run_local(fu_handle **hs, int32_t nranks, int32_t rounds);
/* Device time (ms) of the last round's halo on the rank's communication stream: from the
 * start of the pack (boundary tiles done) to the ghost slots written. The halo overlaps the
 * round's interior tiles. Waits for that halo. FU_ERR_STATE before the first exchange; 0 for
 * an RCCL rank with nothing to send or receive (one rank), whose rounds skip the
 * communication stream altogether. */
int fu_dist_halo_time(fu_handle *h, float *ms);

/* Partition-aware random geometric graph: rank `part` of `nparts` generates only its slab
 * of cell columns (plus the two halo columns) of the graph fu_graph_gen_rgg(n_total, radius,
 * seed) would build, with the same global node ids and row order. Output: local CSR in
 * ghost numbering and the estimates-only halo plan for fu_dist_create (rev = NULL). */
typedef struct fu_part fu_part;
int fu_part_gen_rgg(int64_t n_total, double radius, uint64_t seed, int32_t nparts,
                    int32_t part, fu_part **out);
/* info[0]=n_local [1]=e_local [2]=lo [3]=hi (global ids) [4]=ghost estimates
 * [5]=boundary sends [6]=max degree [7]=n_total */
int fu_part_info(const fu_part *p, int64_t info[8]);
int fu_part_export(const fu_part *p, int64_t *rowptr, int32_t *col, int64_t *ghost_gid,
                   int64_t *send_a_off, int32_t *send_a_idx, int64_t *recv_a_off);
int fu_part_free(fu_part *p);
/* out[k] = lo + (hi - lo) * U_{first+k}: a slice of the fu_values_uniform stream. */
int fu_values_uniform_range(int64_t first, int64_t count, uint64_t seed, double lo, double hi,
                            double *out);

#ifdef __cplusplus
}
#endif

#endif /* FU_H_ */
