// Collect-all engine, piece 3 of 7 (see fu_ca_pack.h): kernel 8, "stage". k_stage (also the
// first pass of kernel 9) and the light tiles that read the staged estimates.
#pragma once

#include "fu_ca_recon.h"

namespace {

// row-class and table constants shared with the host plans (fu_plan.h)
using FP::kStageLds;
using FP::kStageRuns;

// ------------------------------------------------------------------------------------
// Kernel 8, "stage": LDS-staged slices. The a_{r-1}[col e] gather is the part of a round
// that does not stream: on ER every gather is a random L2 request (8 M per round), and the
// fp64 table (8 MB) does not fit an XCD's 4 MB L2. Kernel 8 splits a round into two launches:
//   * k_stage: the estimate table (codes, or doubles while unpacked) is cut into slices of
//     128 KB. A block copies slice s into LDS, then streams a contiguous range of the
//     slice's column offsets (u16) and writes the looked-up elements to G: coalesced reads,
//     16-byte lane-contiguous stores, random accesses only in LDS. G is slice-major: slice
//     s's region holds, tile by tile, the edges whose neighbour lies in slice s.
//   * k_round_staged: kernel 4's light tile (flow reconstruction, CA:98-99 + CA:105-128)
//     where each edge's estimate comes from G: the tile's edges of one slice are one
//     contiguous run of G, found through a u16 {position in the tile, run} per edge and
//     the tile's per-run offsets.
// One layout per table element width (1, 2, 4, 8 bytes; slice = 128 KB / width nodes). The
// device picks the layout from the table's actual packing width; a table wider than the
// layout is read from global memory by the stage launch, so correctness never depends on
// the host's view of the asynchronous packing plan. Rows above the tile limit run as
// kernel 4 heavy tiles in a launch of their own. Results are bitwise those of kernel 4.
// ------------------------------------------------------------------------------------
constexpr int kStageThreads = 1024;   // one block per CU (the slice takes 128 KB of its LDS)

struct StageArgs {
  int P[4], Q[4], SN[4], NB[4];        // slices, blocks per slice, nodes per slice, blocks
  const int4 *brange[4];               // per stage block: {begin, end} in G, slice, 0
  const unsigned short *colS[4];       // per G element: column offset in its slice (pads: 0)
  const unsigned short *sidx16[4];     // per light-tile edge, slice order: position | run << 10
  const int *dtab[4];                  // per light tile: kStageRuns x (G index - m) of each run
  int sel[4];                          // layout used for tables of width 8, 16, 32, 0
  int f64;                             // kernel 9: always stage the doubles (layout 3)
};
__device__ __forceinline__ int width_index(int width) {
  return width == 8 ? 0 : width == 16 ? 1 : width == 32 ? 2 : 3;
}

// EPL consecutive u16 column offsets (EPL = 16 / sizeof(T): one 16-byte G store per lane)
template <int EPL>
struct ColVec {
  uint4 w[EPL > 8 ? 2 : 1];
};
template <int EPL>
__device__ __forceinline__ void ld_cols(ColVec<EPL> &c, const unsigned short *p) {
  if constexpr (EPL == 2) c.w[0].x = *reinterpret_cast<const unsigned *>(p);
  else if constexpr (EPL == 4) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    c.w[0].x = v.x;
    c.w[0].y = v.y;
  } else if constexpr (EPL == 8) c.w[0] = *reinterpret_cast<const uint4 *>(p);
  else {
    c.w[0] = reinterpret_cast<const uint4 *>(p)[0];
    c.w[1] = reinterpret_cast<const uint4 *>(p)[1];
  }
}
template <int EPL>
__device__ __forceinline__ unsigned col_at(const ColVec<EPL> &c, int j) {
  const unsigned w = (&c.w[j >> 3].x)[(j >> 1) & 3];
  return (j & 1) ? w >> 16 : w & 0xFFFFu;
}

// Per lane per step: EPL = 16 / sizeof(T) elements, one lane-contiguous 16-byte G store.
// Steps per batch: enough that every lane keeps 64 B of column loads in flight whatever the
// element width (4 steps of 4-byte loads for doubles left 16 KB in flight per CU, ~2 TB/s at
// HBM latency).
template <typename T>
struct StageU {
  static constexpr int EPL = 16 / (int)sizeof(T);
  static constexpr int U = EPL >= 8 ? kStageU : kStageU * 8 / EPL;
};

// One batch: U steps of EPL elements per lane, all column loads first (caller), then the
// LDS (or global) lookups and one 16-byte store per step.
template <typename T, bool LDS>
__device__ __forceinline__ void stage_load(ColVec<StageU<T>::EPL> (&c)[StageU<T>::U], int g, int g1,
                                           const unsigned short *__restrict__ colS) {
  constexpr int EPL = StageU<T>::EPL, U = StageU<T>::U, STEP = kStageThreads * EPL;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (g + u * STEP < g1) ld_cols<EPL>(c[u], colS + g + u * STEP);
}
template <typename T, bool LDS>
__device__ __forceinline__ void stage_put(const ColVec<StageU<T>::EPL> (&c)[StageU<T>::U], int g, int g1,
                                          const unsigned char *s_tab, const T *__restrict__ tab, int nb,
                                          T *__restrict__ G) {
  constexpr int EPL = StageU<T>::EPL, U = StageU<T>::U, STEP = kStageThreads * EPL;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int gg = g + u * STEP;
    if (gg < g1) {
      T val[EPL];
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        const unsigned off = col_at<EPL>(c[u], j);
        if constexpr (LDS) val[j] = reinterpret_cast<const T *>(s_tab)[off];
        else val[j] = tab[nb + (int)off];
      }
      // doubles non-temporal: G (64 MB on ER-1M, 4 GB of G_A on R-MAT-24) is streamed out
      // once and read back by the next launch (ER-1M kernel 8: 61.8 vs 62.7 us per round,
      // R-MAT-24 kernel 9: 6,728 vs 6,807 us; process-separated A/Bs, profiles/r05/n, o).
      // Packed codes (8-32 MB) stay write-back: they fit on chip until the tiles read them
      // (non-temporal there: 41.0 vs 38.8 us per 8-bit round, profiles/r05/q)
      typedef unsigned v4u __attribute__((ext_vector_type(4)));
      v4u w;
      __builtin_memcpy(&w, val, 16);
      if constexpr (sizeof(T) >= kStageNtMinBytes)
        __builtin_nontemporal_store(w, reinterpret_cast<v4u *>(G + gg));
      else
        *reinterpret_cast<v4u *>(G + gg) = w;
    }
  }
}

// Slice s of the table (element type T) -> LDS (LDS = false: the table is wider than the
// layout and is read from global memory), then the block's G range [g0, g1), software
// pipelined: the next batch's column loads are issued before the current batch is looked
// up and stored (two register sets, so no in-flight register is copied).
template <typename T, bool LDS>
__device__ __forceinline__ void stage_body(unsigned char *s_tab, int nb, int cnt, int g0, int g1,
                                           const unsigned short *__restrict__ colS,
                                           const T *__restrict__ tab, T *__restrict__ G) {
  constexpr int EPL = StageU<T>::EPL, U = StageU<T>::U, BSTEP = U * kStageThreads * EPL;
  constexpr int kW = kStageLds / 16 / kStageThreads;
  const int t = threadIdx.x;
  uint4 buf[kW];
  const int bytes = LDS ? cnt * (int)sizeof(T) : 0;
  const int w16 = bytes >> 4;
  if constexpr (LDS) {
    const uint4 *s16 = reinterpret_cast<const uint4 *>(tab + nb);
#pragma unroll
    for (int u = 0; u < kW; ++u) {
      const int k = t + u * kStageThreads;
      buf[u] = k < w16 ? s16[k] : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  ColVec<EPL> ca[U], cb[U];
  int g = g0 + t * EPL;
  stage_load<T, LDS>(ca, g, g1, colS);
  if constexpr (LDS) {  // slice stores after the first batch's loads are in flight
#pragma unroll
    for (int u = 0; u < kW; ++u) {
      const int k = t + u * kStageThreads;
      if (k < w16) reinterpret_cast<uint4 *>(s_tab)[k] = buf[u];
    }
    const int tb = w16 << 4;
    if (t < bytes - tb) s_tab[tb + t] = reinterpret_cast<const unsigned char *>(tab + nb)[tb + t];
    __syncthreads();
  }
  for (;;) {
    if (g >= g1) break;
    stage_load<T, LDS>(cb, g + BSTEP, g1, colS);
    stage_put<T, LDS>(ca, g, g1, s_tab, tab, nb, G);
    g += BSTEP;
    if (g >= g1) break;
    stage_load<T, LDS>(ca, g + BSTEP, g1, colS);
    stage_put<T, LDS>(cb, g, g1, s_tab, tab, nb, G);
    g += BSTEP;
  }
}

__global__ __launch_bounds__(kStageThreads) void k_stage(StageArgs sa, int n,
                                                        const double *__restrict__ a_prev,
                                                        const void *__restrict__ code_prev,
                                                        PackCtl *ctl, int rslot,
                                                        void *__restrict__ G, const int *__restrict__ psample,
                                                        int *pw_host) {
  __shared__ __align__(16) unsigned char s_tab[kStageLds];
  // the packing plan from a_{r-1} (the table staged here; due after round r-1) rides on the
  // stage launch: k_round_staged, the plan's first reader, starts after this launch, so the
  // plan needs no launch (and stream slot) of its own. Its block is block 0, dispatched
  // first so its dependent loads overlap the staging; blocks 1-7 exit and the stage blocks
  // follow from block 8 on, on the XCDs (blockIdx % 8) they have without the plan.
  int bid = (int)blockIdx.x;
  if (psample) {
    if (bid == 0) plan_body<kStageThreads>(a_prev, psample, ctl, pw_host);
    if (bid < 8) return;
    bid -= 8;
  }
  const PackCtl pp = ctl[rslot ^ 1];
  // bytes per element of the table gathered (kernel 9 stages the doubles, always written)
  const int wb = (pp.width && !sa.f64) ? pp.width / 8 : 8;
  const int li = sa.f64 ? 3 : sa.sel[width_index(pp.width)];
  if (bid >= sa.NB[li]) return;
  const int4 rg = sa.brange[li][bid];
  if (rg.x >= rg.y) return;  // no slice here (grid rounded to whole XCD rows) or empty region
  const int LB = 1 << li;  // bytes per element the layout was built for
  const int SN = sa.SN[li];
  const int nb = rg.z * SN;
  const int cnt = min(SN, n - nb);
  const void *src = (pp.width && !sa.f64) ? code_prev : static_cast<const void *>(a_prev);
  const unsigned short *colS = sa.colS[li];
#define FU_BODY(T)                                                                                    \
  do {                                                                                                \
    if ((int)sizeof(T) <= LB)                                                                         \
      stage_body<T, true>(s_tab, nb, cnt, rg.x, rg.y, colS, reinterpret_cast<const T *>(src),         \
                          reinterpret_cast<T *>(G));                                                  \
    else                                                                                              \
      stage_body<T, false>(s_tab, nb, cnt, rg.x, rg.y, colS, reinterpret_cast<const T *>(src),        \
                           reinterpret_cast<T *>(G));                                                 \
  } while (0)
  if (wb == 1) FU_BODY(unsigned char);
  else if (wb == 2) FU_BODY(unsigned short);
  else if (wb == 4) FU_BODY(unsigned);
  else FU_BODY(unsigned long long);
#undef FU_BODY
}

// Kernel 8's light tiles. The tile's flows are taken by global 4-aligned quads: quad g holds
// edges 4 g .. 4 g + 3, whose split flow words (fhi_idx: a quad never straddles a 32-edge
// block) are one 16-byte load of high words, one of low words and one 16-byte store of low
// words. Lane t takes quad (e0 >> 2) + t; LDS slot p holds edge (e0 & ~3) + p, so the tile's
// own slots are [r, r + ne), r = e0 % 4, and a lane's four slots are 16-byte aligned. A tile
// of more than TE - r edges ends in a 257th quad: its at most three edges (slots TE .. TE +
// r - 1) go one each to the first lanes of wave 0. The staged estimates keep the other
// mapping, element t + 256 k of the tile's slice order to lane t: consecutive lanes read
// consecutive elements of G, and an estimate meets its flow only in LDS (with the quads'
// mapping for G too, lane-strided 8-byte loads, the unpacked rounds ran 59.5 against 56.5 us).
// The edges of a boundary quad outside [e0, e0 + ne) belong to the neighbouring tile, which
// may be rewriting them in place meanwhile: they are loaded with the quad (the loads stay
// unconditional, from always-valid addresses, see the load order below), and then dropped:
// they reach neither LDS nor a sum nor a store, and a boundary quad stores word by word.
template <bool CHECK, int TE, int TN, bool RF = true>
__global__ __launch_bounds__(kBlock) void k_round_staged(
    const int4 *__restrict__ tiles, int t0, int ntl,
    const int *__restrict__ rowptr, const int *__restrict__ col,
    const StageArgs sa, const void *__restrict__ G, const double *__restrict__ v,
    double *F, const double *__restrict__ a_prev, const double *__restrict__ a_prev2,
    double *__restrict__ a_new, const double *__restrict__ target,
    unsigned long long *__restrict__ err, void *__restrict__ code_new, PackCtl *__restrict__ ctl,
    int rslot, int fm) {
  static_assert(TE == 4 * kBlock && TN <= kBlock, "tile geometry: one quad of edges per lane");
  static_assert(TE <= 1024, "the u16 staged index holds a 10-bit tile position");
  const PackCtl pp = ctl[rslot ^ 1];
  const int lsel = sa.sel[width_index(pp.width)];
  const PackCtl pc = ctl[2];
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl[rslot] = pc;
  __shared__ __align__(16) double s_x[TE + 4];
  __shared__ __align__(16) double s_er[TE + 4];
  __shared__ __align__(4) unsigned char s_own[TE + 4];
  __shared__ int s_rp[TN + 1];
  __shared__ double s_a[TN];
  const int t = threadIdx.x;
  unsigned long long eb = 0;
  // XCD-aware order: block b runs on XCD b % 8; consecutive tiles go to the same XCD, so
  // the G runs that neighbouring tiles share in every slice region meet in one L2
  const int xcd = blockIdx.x & 7, per = ntl >> 3, rem = ntl & 7;
  const int tile = t0 + xcd * per + min(xcd, rem) + (int)(blockIdx.x >> 3);
  const int4 tl = tiles[tile];
  const int nb = tl.x, nn = tl.y - tl.x;
  const int e0 = tl.z, ne = tl.w - tl.z;
  const unsigned short *__restrict__ s16 = sa.sidx16[lsel];
  // the flows' split words (fhi_idx). F is not __restrict__ here: the fence below does not
  // hold back the loads of a noalias argument (the flow loads sank past it, behind the wait
  // for the staged indices)
  unsigned *fo = reinterpret_cast<unsigned *>(F);
  const unsigned *fw = fo;
  // quads: slot p <-> edge eq0 + p <-> tile position p - r; the tile's slots are [r, pe)
  const int r = e0 & 3, eq0 = e0 - r, pe = r + ne;
  const int p0 = 4 * t;
  bool ok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) ok[u] = p0 + u >= r && p0 + u < pe;
  const bool any = ne > 0 && p0 + 3 >= r && p0 < pe;  // the quad holds an edge of the tile
  const bool full = p0 >= r && p0 + 3 < pe;  // all four are the tile's
  const int eq = any ? eq0 + p0 : 0;         // quad 0 otherwise: always inside the arrays
  const bool tok = TE + t < pe;              // the 257th quad: slot TE + t (t < r <= 3)
  const int et = eq0 + TE + t;
  unsigned si[4];  // position in the tile
  double g[4];
  // the old flows' words as loaded (the high words are kept for the stores); what a quad
  // holds of a neighbouring tile stays in these registers and goes nowhere
  uint4 hq = make_uint4(0u, 0u, 0u, 0u), lq = hq;
  unsigned hwt = 0u, lwt = 0u;
  int gi[4];
  // Load order: the run offsets and staged indices first, the flows and node words after
  // them, so the G loads (which need only the former) issue while the flows are in flight
  // (in-order completion: waiting for a load waits for every load issued before it). The
  // interleaved order measured slower.
  int rp;
  double vv, own2;
  {  // u16 position | run << 10; G index = m + D[run] (lane `run` holds D)
    // the 257th quad's flows first (a few lanes of the full tiles only): older than the staged
    // indices, so the counted wait below covers them on either path
    if constexpr (RF) {
      if (tok) {
        const long long i = fhi_idx(et);
        hwt = fw[i];
        lwt = fw[i + 32];
      }
    }
    const int dl = sa.dtab[lsel][(size_t)tile * kStageRuns + (t & 63)];
    // unconditional loads from always-valid addresses, so the compiler can wait for the
    // staged indices alone (vmcnt(N)) instead of for every load (a skipped load would change
    // the count)
    unsigned c16[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = t + k * kBlock;
      c16[k] = s16[q < ne ? e0 + q : 0];
    }
    if constexpr (RF) {
      const long long i = fhi_idx(eq);
      hq = *reinterpret_cast<const uint4 *>(fw + i);
      lq = *reinterpret_cast<const uint4 *>(fw + i + 32);
    }
    const int tn = min(t, nn - 1);  // a light tile has at least one node
    const int rp0 = rowptr[nb + min(t, nn)];
    const double v0 = v[nb + tn], o0 = a_prev2[nb + tn];
    asm volatile("" ::: "memory");  // every load above issued before the first wait (no sinking)
    rp = t <= nn ? rp0 : 0;
    vv = t < nn ? v0 : 0.0;
    own2 = t < nn ? o0 : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = t + k * kBlock;
      const int dd = __shfl(dl, (int)(c16[k] >> 10));
      si[k] = c16[k] & 1023u;
      gi[k] = q < ne ? q + dd : -1;
    }
  }
  // every G load of the tile first, then decode (escapes gather the double via col). The
  // loads are unconditional too (index 0 for an edge that is not the tile's), and the 1-, 2-
  // and 4-byte codes share one path: the aligned 4-byte word that holds the code is loaded
  // and the code shifted out of it (a load per width in branches of their own made the
  // compiler drain every load in flight, the flows included, before the 1-byte loads)
  if (pp.width == 0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double d = reinterpret_cast<const double *>(G)[max(gi[u], 0)];
      g[u] = gi[u] >= 0 ? d : 0.0;
    }
  } else {
    const int lb = pp.width == 8 ? 0 : pp.width == 16 ? 1 : 2;  // log2 of the code's bytes
    const unsigned esc = 0xFFFFFFFFu >> (32 - pp.width);        // the escape code: all ones
    const char *Gc = reinterpret_cast<const char *>(G);
    auto ld_word = [&](int i) {  // the word holding code i (codes are aligned to their size)
      const size_t b = (size_t)max(i, 0) << lb;
      return *reinterpret_cast<const unsigned *>(Gc + (b & ~(size_t)3));
    };
    auto code_of = [&](unsigned w, int i) { return (w >> ((((unsigned)max(i, 0) << lb) & 3u) * 8u)) & esc; };
    unsigned cd[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cd[u] = ld_word(gi[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      cd[u] = code_of(cd[u], gi[u]);
      g[u] = gi[u] < 0 ? 0.0 : cd[u] == esc ? a_prev[col[e0 + (int)si[u]]] : dkey_inv(pp.base + cd[u]);
    }
  }
  // s_x: the lane's own slots (16-byte writes for a whole quad); s_er: a scatter by position
  const unsigned hw[4] = {hq.x, hq.y, hq.z, hq.w}, lw[4] = {lq.x, lq.y, lq.z, lq.w};
  double x[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) x[u] = __hiloint2double((int)hw[u], (int)lw[u]);
  if (full) {
    *reinterpret_cast<double2 *>(&s_x[p0]) = make_double2(x[0], x[1]);
    *reinterpret_cast<double2 *>(&s_x[p0 + 2]) = make_double2(x[2], x[3]);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (ok[u]) s_x[p0 + u] = x[u];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (gi[k] >= 0) s_er[r + (int)si[k]] = g[k];
  if (tok) s_x[TE + t] = __hiloint2double((int)hwt, (int)lwt);
  if (t <= nn) s_rp[t] = rp;
  __syncthreads();
  if (t < nn) {  // phase B (CA:106-113)
    const int qb = s_rp[t] - eq0, qe = s_rp[t + 1] - eq0;  // the row's slots
    double S = 0.0, T = 0.0;
    const double fo0 = fm ? old_flow(fm, own2) : 0.0;
    for (int q = qb; q < qe; ++q) {
      const double er = s_er[q];
      const double fr = recon_fr(fm ? fo0 : s_x[q], er, own2);
      s_x[q] = fr;
      s_own[q] = (unsigned char)t;
      S = S + fr;
      T = T + er;
    }
    const double a = ((vv - S) + T) / (double)(qe - qb + 1);
    s_a[t] = a;
    *(a_new + nb + t) = a;
    if (pc.width) put_code(pc, code_new, nb + t, a);
    if (CHECK) eb = err_bits(a, target[nb + t]);
  }
  __syncthreads();
  // phase C: new flows in place (CA:117-118). A whole quad: its low words are one 16-byte
  // store, its high words one more when all four changed (or the slots hold no earlier
  // value, fm), else only those that changed; a boundary quad: its own edges, word by word
  if (any) {
    const double2 xa = *reinterpret_cast<const double2 *>(&s_x[p0]), xb = *reinterpret_cast<const double2 *>(&s_x[p0 + 2]);
    const double2 ea = *reinterpret_cast<const double2 *>(&s_er[p0]), ec = *reinterpret_cast<const double2 *>(&s_er[p0 + 2]);
    const unsigned ow = *reinterpret_cast<const unsigned *>(&s_own[p0]);
    const double xs[4] = {xa.x, xa.y, xb.x, xb.y}, es[4] = {ea.x, ea.y, ec.x, ec.y};
    unsigned nh[4], nl[4];
    bool ch[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int own = ok[u] ? (int)((ow >> (8 * u)) & 0xFFu) : 0;  // (a foreign slot's bytes are dropped)
      const double f = (xs[u] + s_a[own]) - es[u];
      nh[u] = (unsigned)__double2hiint(f);
      nl[u] = (unsigned)__double2loint(f);
      ch[u] = !RF || fm || nh[u] != hw[u];
    }
    unsigned *w = fo + fhi_idx(eq);
    if (full) {
      *reinterpret_cast<uint4 *>(w + 32) = make_uint4(nl[0], nl[1], nl[2], nl[3]);
      if (ch[0] && ch[1] && ch[2] && ch[3]) {
        *reinterpret_cast<uint4 *>(w) = make_uint4(nh[0], nh[1], nh[2], nh[3]);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (ch[u]) st_fw(w + u, nh[u]);
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) {
          st_fw(w + 32 + u, nl[u]);
          if (ch[u]) st_fw(w + u, nh[u]);
        }
    }
  }
  if (tok) {
    const double f = (s_x[TE + t] + s_a[s_own[TE + t]]) - s_er[TE + t];
    unsigned *w = fo + fhi_idx(et);
    st_fw(w + 32, (unsigned)__double2loint(f));
    if (!RF || fm || (unsigned)__double2hiint(f) != hwt) st_fw(w, (unsigned)__double2hiint(f));
  }
  if (CHECK) block_max_to(eb, err);
}

}  // namespace
