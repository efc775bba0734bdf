// Collect-all engine, piece 4 of 7 (see fu_ca_pack.h): kernel 9, "pregather". k_transpose, the
// isolated rows, the multi-row heavy blocks and their lagged flows. (Its first pass is
// fu_ca_stage.h's k_stage; its tiles, heavy rows and mega hubs are fu_ca_recon.h's, PRE = true.)
#pragma once

#include "fu_ca_recon.h"

namespace {

// row-class and table constants shared with the host plans (fu_plan.h)
using FP::kMR;
using FP::kTrBE;
using FP::kTrMaxP;

// ------------------------------------------------------------------------------------
// Kernel 9, "pregather": propagation blocking for power-law graphs, where tiles touch far
// more slices than kernel 8's u16 index can address and most edges sit in heavy rows. Two
// passes turn every random gather a_{r-1}[col e] into streams:
//   * k_stage (doubles, 128 KB slices): G_A in slice-major order, within slice s the edges
//     whose neighbour lies in s, in edge order (so each bucket of kTrBE consecutive edges
//     has one contiguous run per slice);
//   * k_transpose: one block per bucket reads its runs (the run starts of every slice are
//     precomputed per bucket), scatters the values into LDS by their position in the bucket
//     and writes Gb[e] for the bucket's edges, coalesced.
// The round kernels (kernel 4's tiles, heavy rows and mega hubs, PRE = true) then read Gb[e]
// beside the flows. Bytes per edge: stage 2 + 8, transpose 8 + 2 + 8, round 8 (instead of
// col 4 + one random 8-byte gather).
// ------------------------------------------------------------------------------------
constexpr int kTrThreads = 1024;

// Persistent over its buckets: grid = 8 x (blocks per XCD); XCD x owns the contiguous
// bucket range [x per, (x + 1) per) and its blocks take every nj-th bucket of it. The next
// bucket's run starts (offT) are loaded while this bucket's G_A loads are in flight, and its
// G_B stores drain while the next bucket is scanned (with one block per bucket, each block
// paid the offT round trip first and held its slot until its stores were done).
template <bool NT>  // NT: the streamed G_B stores non-temporal
__global__ __launch_bounds__(kTrThreads, kTrWaves) void k_transpose(int b0, int nbk, int P, long long E,
                                                        const int *__restrict__ offT,
                                                        const double *__restrict__ GA,
                                                        const unsigned short *__restrict__ pos16,
                                                        double *__restrict__ GB) {
  __shared__ double s_v[kTrBE];
  __shared__ unsigned short s_m[kTrMaxP + 1];  // first element (bucket order) of each slice's run
  __shared__ int s_o[kTrMaxP];      // G_A index of each run
  __shared__ int s_c[kTrBE / 64 + 1];
  __shared__ int s_w[kTrThreads / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // XCD-contiguous buckets (block b runs on XCD b % 8): a G_A line that ends one bucket's
  // run and starts the next bucket's is fetched into one L2, not two
  const int per = (nbk + 7) >> 3;
  const int nj = (int)(gridDim.x >> 3);
  int bk = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  const int bend = min((int)(blockIdx.x & 7) * per + per, nbk);
  if (bk >= bend) return;
  // runs: thread t owns slices 2t, 2t + 1
  int o[2], len[2];
  auto load_runs = [&](int bkk, int (&oo)[2], int (&ll)[2]) {
    const int bb = b0 + bkk;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int sl = 2 * t + j;
      oo[j] = sl < P ? offT[(long long)bb * P + sl] : 0;
      ll[j] = sl < P ? offT[(long long)(bb + 1) * P + sl] - oo[j] : 0;
    }
  };
  load_runs(bk, o, len);
  for (;;) {
  const int bb = b0 + bk;
  const long long e0 = (long long)bb * kTrBE;
  const int ne = (int)min((long long)kTrBE, E - e0);
  // exclusive scan of len0 + len1 over the block: wave shuffles, then the 16 wave totals
  int x = len[0] + len[1];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; ++k) base += s_w[k];
  const int excl = base + x - (len[0] + len[1]);
  if (2 * t < P) {
    s_m[2 * t] = excl;
    s_o[2 * t] = o[0];
  }
  if (2 * t + 1 < P) {
    s_m[2 * t + 1] = excl + len[0];
    s_o[2 * t + 1] = o[1];
  }
  if (t == 0) {  // staged elements of the bucket (< ne when mega-hub edges are left out)
    int tot = 0;
    for (int k = 0; k < kTrThreads / 64; ++k) tot += s_w[k];
    s_m[P] = tot;
  }
  __syncthreads();
  const int nst = s_m[P];
  // coarse table: the run holding element 64 k (s_c), so each element's search spans only
  // the runs of its 64-element stretch
  if (t < kTrBE / 64) {
    const int m = t * 64;
    int lo = 1, hi = P;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_m[mid] > m) hi = mid; else lo = mid + 1;
    }
    s_c[t] = lo;
  }
  if (t == 0) s_c[kTrBE / 64] = P;
  __syncthreads();
  // element m (the bucket's G_A runs in slice order) -> G_A index; all searches first, then
  // every load of the thread in flight at once, then the LDS scatter by bucket position
  constexpr int kPerT = kTrBE / kTrThreads;
  int g[kPerT];
#pragma unroll
  for (int k = 0; k < kPerT; ++k) {
    const int m = t + k * kTrThreads;
    g[k] = -1;
    if (m < nst) {
      int lo = s_c[m >> 6], hi = s_c[(m >> 6) + 1];  // first boundary s_m[s] > m lies in [lo, hi]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_m[mid] > m) hi = mid; else lo = mid + 1;
      }
      const int run = lo - 1;  // s_m[run] <= m < s_m[run + 1]: a non-empty run
      g[k] = s_o[run] + (m - s_m[run]);
    }
  }
  double val[kPerT];
  unsigned short pos[kPerT];
#pragma unroll
  for (int k = 0; k < kPerT; ++k) {
    // plain loads (non-temporal G_A loads beside the non-temporal stores: 6,703 vs 6,612 us
    // per round on R-MAT-24, profiles/r05/u)
    val[k] = g[k] >= 0 ? GA[g[k]] : 0.0;
    pos[k] = g[k] >= 0 ? pos16[g[k]] : (unsigned short)0;
  }
  const int next = bk + nj;
  if (next < bend) load_runs(next, o, len);  // in flight beside this bucket's loads
#pragma unroll
  for (int k = 0; k < kPerT; ++k)
    if (g[k] >= 0) s_v[pos[k]] = val[k];
  __syncthreads();
  for (int q = t; q < ne; q += kTrThreads) {
    if constexpr (NT) __builtin_nontemporal_store(s_v[q], GB + e0 + q);
    else GB[e0 + q] = s_v[q];
  }
  if (next >= bend) break;
  __syncthreads();  // the shared tables and s_v are rewritten for the next bucket
  bk = next;
  }
}

// Kernel 9: the isolated rows at the end of the degree layout (the last light tiles have no
// edges): a_r = ((v - 0.0) + 0.0) / 1 (CA:106-113 with no neighbours), as a light tile
// computes it, one thread per row instead of a tile block per 128 rows.
__global__ __launch_bounds__(kBlock) void k_isolated(int i0, int n, const double *__restrict__ v,
                                                     double *__restrict__ a_new, const double *__restrict__ target,
                                                     unsigned long long *__restrict__ err, void *__restrict__ code_new,
                                                     PackCtl *__restrict__ ctl, int rslot, int check) {
  const PackCtl pc = ctl[2];
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl[rslot] = pc;
  const int i = i0 + blockIdx.x * kBlock + threadIdx.x;
  unsigned long long eb = 0;
  if (i < n) {
    const double a = ((v[i] - 0.0) + 0.0) / (double)1;
    *(a_new + i) = a;
    if (pc.width) put_code(pc, code_new, i, a);
    if (check) eb = err_bits(a, target[i]);
  }
  if (check) block_max_to(eb, err);
}

// ------------------------------------------------------------------------------------
// Kernel 9's heavy rows (degree > 64 x kHeavyRL, <= mega_hub), many rows per chain wave.
// A row's two sums are exact left-to-right chains (CA:106, CA:110), so each element costs
// one dependent fp64 add per sum. With one row per wave (k_round_recon's heavy tiles) a
// wave64 v_add_f64 advances two chains (even lanes S, odd lanes T), and on R-MAT-24 the
// chains of these rows kept the SIMDs busy for ~1.2 ms per round beside their memory
// traffic. Here a block takes kMR rows of similar length (the rows are sorted by degree),
// its four waves stage chunks of kMCH elements of every row, (fr, er) into LDS, and ONE
// wave runs all 2 kMR chains at once (lane 2r: S of row r, lane 2r + 1: T), with the loads
// of the next chunk in flight meanwhile. Then a flow pass re-reads the old flows and the
// pre-gathered estimates (CA:117-118). Same operations in the same order as every other
// path: the results are bitwise equal.
// ------------------------------------------------------------------------------------
//
// LAG (option "lag", kernel 9): no flow pass. Round r leaves f_r unwritten and instead
// materialises f_{r-2} while it stages the row: F holds f_{r-4} and f_{r-2} = (recon(f_{r-4}, er_{r-2}, a_{r-4}) +
// a_{r-2}) - er_{r-2} is exactly what round r - 2's flow pass would have written (CA:117-118,
// same operations, same operands: er_{r-2} from the G_B ring, a_{r-4} from the per-row
// history `hist`). So a lagged row costs 32 B per edge (f and G_B of two rounds, one flow
// store) instead of 40 (both re-read for the flow pass). LAGM = 1: F holds f_{r-2}
// already (fm = 1, 2: computed, and stored as the base of round r + 2); LAGM = 2: F holds
// f_{r-4} (the previous round of this parity was lagged). lag_finalize
// writes f_r when another kernel, fu_get_flows or a tile rebuild needs it.
constexpr int kMCH = 64;  // elements per row per chunk (one per lane)
template <bool CHECK, int LAGM = 0>  // LAGM: 0 = no lag, 1 = lagin 0, 2 = lagin 1
__global__ __launch_bounds__(kBlock) void k_heavy_multi(
    const int *__restrict__ hrows, int nrows, const int *__restrict__ rowptr, const double *__restrict__ v,
    double *__restrict__ F, const double *__restrict__ a_prev2, double *__restrict__ a_new,
    const double *__restrict__ target, unsigned long long *__restrict__ err, void *__restrict__ code_new,
    PackCtl *__restrict__ ctl, const double *__restrict__ Gb, int fm,
    const double *__restrict__ Gb_old = nullptr, double *__restrict__ hist = nullptr) {
  constexpr bool LAG = LAGM > 0;
  constexpr bool mat = LAGM == 2;
  // sh[buf][2 r + {0: fr, 1: er}][q]; a row stride of kMCH + 1 doubles puts the 32 chain lanes'
  // reads of one step on 32 different bank pairs
  __shared__ double sh[2][2 * kMR][kMCH + 1];
  __shared__ int s_b[kMR], s_d[kMR];
  __shared__ double s_o2[kMR], s_a[kMR], s_o4[kMR];
  const PackCtl pc = ctl[2];  // packing of a_r (the table written here)
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int r0 = blockIdx.x * kMR;
  if (t < kMR) {
    const bool ok = r0 + t < nrows;
    const int i = ok ? hrows[r0 + t] : 0;
    const int b = ok ? rowptr[i] : 0;
    s_b[t] = b;
    s_d[t] = ok ? rowptr[i + 1] - b : 0;
    const double o2 = ok ? a_prev2[i] : 0.0;
    s_o2[t] = o2;
    if (LAG) {  // a_{r-4} of the row (written by round r - 2), then a_{r-2} for round r + 2
      s_o4[t] = ok && mat ? hist[r0 + t] : 0.0;
      if (ok) hist[r0 + t] = o2;
    }
  }
  __syncthreads();
  // wave w stages rows 4 w .. 4 w + 3; element c kMCH + lane of each
  int rb[4], rd[4];
  double ro2[4], ro4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rb[j] = s_b[4 * w + j];
    rd[j] = s_d[4 * w + j];
    ro2[j] = s_o2[4 * w + j];
    ro4[j] = LAG ? s_o4[4 * w + j] : 0.0;
  }
  const int nch = (s_d[0] + kMCH - 1) / kMCH;  // rows sorted longest first
  // two register sets, each one chunk of the wave's 4 rows: the loads run two chunks ahead of
  // the chain. Loads are unconditional from clamped indices (the compiler then waits for a
  // set by count, vmcnt(N), not for everything)
  double fo0[4], er0[4], fo1[4], er1[4];
  double eo0[4], eo1[4];  // LAGM 2: er_{r-2} (G_B of round r - 2)
  auto load = [&](double (&fo)[4], double (&er)[4], double (&eo)[4], int c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = min(c * kMCH + lane, max(rd[j] - 1, 0));
      er[j] = Gb[rb[j] + k];
      if constexpr (mat) eo[j] = Gb_old[rb[j] + k];
      if constexpr (mat) fo[j] = ld_f(F, rb[j] + k);
      else fo[j] = ld_fo(F, rb[j] + k, fm, ro2[j]);
    }
  };
  auto put = [&](const double (&fo)[4], const double (&er)[4], const double (&eo)[4], int c, int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 4 * w + j;
      const bool in = c * kMCH + lane < rd[j];
      double f2 = fo[j];  // f_{r-2}
      if (LAG && in) {
        const int e = rb[j] + c * kMCH + lane;
        if constexpr (mat) {  // round r - 2's flow (CA:117-118), from f_{r-4}
          f2 = (recon_fr(fo[j], eo[j], ro4[j]) + ro2[j]) - eo[j];
          st_f(F, e, f2, fo[j]);
        } else if (fm) {  // f_{-1} / f_0, the base round r + 2 materialises from
          st_f_full(F, e, f2);
        }
      }
      sh[buf][2 * r][lane] = in ? recon_fr(f2, er[j], ro2[j]) : 0.0;
      sh[buf][2 * r + 1][lane] = in ? er[j] : 0.0;
    }
  };
  // chain lanes: lane 2 r + h (wave 0, lanes < 2 kMR)
  const int cr = lane >> 1, ch = lane & 1;
  double acc = 0.0;
  auto chain = [&](int c, int buf) {
    if (w == 0 && lane < 2 * kMR) {
      const int len = min(kMCH, max(0, s_d[cr] - c * kMCH));
      const double *src = sh[buf][lane];
      int q = 0;
      if (len == kMCH) {  // a full chunk: the next 8 LDS reads in flight beside the 8 dependent adds
        double x[8], y[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = src[u];
#pragma unroll
        for (int b = 0; b < kMCH; b += 16) {
#pragma unroll
          for (int u = 0; u < 8; ++u) y[u] = src[b + 8 + u];
#pragma unroll
          for (int u = 0; u < 8; ++u) acc = acc + x[u];
          if (b + 16 < kMCH) {
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = src[b + 16 + u];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc = acc + y[u];
        }
        q = len;
      }
      for (; q + 8 <= len; q += 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = src[q + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + x[u];
      }
      for (; q < len; ++q) acc = acc + src[q];
    }
  };
  if (nch > 0) {
    load(fo0, er0, eo0, 0);
    load(fo1, er1, eo1, 1);
    put(fo0, er0, eo0, 0, 0);
  }
  __syncthreads();
  for (int c = 0; c < nch; c += 2) {
    // chunk c in buffer 0, chunk c + 1 in flight in set 1
    if (c + 2 < nch) load(fo0, er0, eo0, c + 2);
    chain(c, 0);
    __syncthreads();
    if (c + 1 >= nch) break;
    put(fo1, er1, eo1, c + 1, 1);
    __syncthreads();
    // chunk c + 1 in buffer 1, chunk c + 2 in flight in set 0
    if (c + 3 < nch) load(fo1, er1, eo1, c + 3);
    chain(c + 1, 1);
    __syncthreads();
    if (c + 2 >= nch) break;
    put(fo0, er0, eo0, c + 2, 0);
    __syncthreads();
  }
  unsigned long long eb = 0;
  if (w == 0) {
    const double T = __shfl(acc, (lane & ~1) + 1);  // row cr's T (lane 2 cr + 1)
    if (lane < 2 * kMR && ch == 0 && r0 + cr < nrows) {
      const int i = hrows[r0 + cr];
      const double a = ((v[i] - acc) + T) / (double)(s_d[cr] + 1);
      s_a[cr] = a;
      *(a_new + i) = a;
      if (pc.width) put_code(pc, code_new, i, a);
      if (CHECK) eb = err_bits(a, target[i]);
    }
  }
  if (LAG) {  // round r + 2 (or k_lag_final) writes the flows
    if (CHECK) block_max_to(eb, err);
    return;
  }
  __syncthreads();
  // flows (CA:117-118): wave w, its rows, 8 elements per lane in flight
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    const int b = rb[j], d = rd[j];
    const double own2 = ro2[j], a = s_a[4 * w + j];
    for (int k0 = 0; k0 < d; k0 += 8 * 64) {
      double f8[8], e8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + lane + 64 * u;
        e8[u] = k < d ? Gb[b + k] : 0.0;
        f8[u] = k < d ? ld_fo(F, b + k, fm, own2) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + lane + 64 * u;
        if (k < d) st_fo(F, b + k, (recon_fr(f8[u], e8[u], own2) + a) - e8[u], f8[u], fm);
      }
    }
  }
  if (CHECK) block_max_to(eb, err);
}

// Lagged rows (k_heavy_multi<LAG>): write the flows f_{r'} their last round r' of this
// parity left unwritten: F holds f_{r'-2}, Gb = er_{r'} (G_B of round r'), hist = a_{r'-2},
// a = a_{r'} (CA:117-118, the flow pass k_heavy_multi would have run). One block per row.
__global__ __launch_bounds__(kBlock) void k_lag_final(const int *__restrict__ rows, const int *__restrict__ rowptr,
                                                      double *__restrict__ F, const double *__restrict__ Gb,
                                                      const double *__restrict__ hist,
                                                      const double *__restrict__ a) {
  const int i = rows[blockIdx.x];
  const int b = rowptr[i], d = rowptr[i + 1] - b;
  const double own2 = hist[blockIdx.x], an = a[i];
  for (int k0 = 0; k0 < d; k0 += 8 * kBlock) {
    double f8[8], e8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + (int)threadIdx.x + kBlock * u;
      e8[u] = k < d ? Gb[b + k] : 0.0;
      f8[u] = k < d ? ld_f(F, b + k) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + (int)threadIdx.x + kBlock * u;
      if (k < d) st_f(F, b + k, (recon_fr(f8[u], e8[u], own2) + an) - e8[u], f8[u]);
    }
  }
}

}  // namespace
