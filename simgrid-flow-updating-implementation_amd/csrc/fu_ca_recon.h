// Collect-all engine, piece 2 of 7 (see fu_ca_pack.h): kernel 4, "recon". The error reduction,
// round 0, the split-word flow storage, the exact chains, k_round_recon (light tiles, heavy
// rows, mega hubs), the hub kernels and the small copy kernels.
#pragma once

#include "fu_ca_pack.h"

namespace {

// row-class and table constants shared with the host plans (fu_plan.h)
using FP::kHeavyRL;
using FP::kR0E;

static_assert(kBlock == FP::kHubBlk, "k_hub_stage / k_hub_flows blocks follow the plan's hub table");
constexpr int kTileEdges = 2048;  // max edges staged in LDS per light tile
constexpr int kTileNodes = kBlock;

// ------------------------------------------------------------------------------------
// error reduction: max over |a - target| as uint64 bit patterns (non-negative doubles
// order like their bits; a NaN (sign cleared) is larger than +inf, so NaN propagates)
// ------------------------------------------------------------------------------------
__device__ inline unsigned long long err_bits(double a, double t) {
  return (unsigned long long)__double_as_longlong(fabs(a - t));
}

__device__ inline void block_max_to(unsigned long long x, unsigned long long *dst) {
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long y = __shfl_xor(x, off, 64);
    x = x > y ? x : y;
  }
  __shared__ unsigned long long s_w[kBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_w[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = s_w[0];
    for (int k = 1; k < kBlock / 64; ++k) m = m > s_w[k] ? m : s_w[k];
    // a plain read first: only blocks that raise the running max issue the atomic (a stale
    // read only costs an extra atomic, never a wrong max). Without it 16K blocks serialise
    // on one address.
    if (m && m > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, m);
  }
}

// ------------------------------------------------------------------------------------
// Round 0: the timeout fire on zero state (CA:33-34, CA:87-91 -> CA:105-128)
// ------------------------------------------------------------------------------------
// a_0 (the timeout fire on zero state) into A[0]; a_{-1} = 0.0 into A[2] (na slots, ghosts
// included); the three packing slots cleared (no codes yet)
__global__ __launch_bounds__(kBlock) void k_round0(int n, int na, const int *__restrict__ rowptr,
                                                   const double *__restrict__ v, double *__restrict__ a,
                                                   double *__restrict__ a_m1, unsigned long long *__restrict__ pctl) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < 6) pctl[i] = 0ull;  // 3 x 16-byte PackCtl
  if (i < na) a_m1[i] = 0.0;
  if (i >= n) return;
  a[i] = ((v[i] - 0.0) + 0.0) / (double)(rowptr[i + 1] - rowptr[i] + 1);
}

// ------------------------------------------------------------------------------------
// Flow storage of kernels >= 4 (state shared by kernels 4-10): split words. The flow of
// edge e is stored as its double's high and low 32-bit words in separate 128-byte lines:
// block e / 32 holds 32 high words, then 32 low words. Each round rewrites every low word,
// but a high word (sign, exponent, top 20 mantissa bits) only when it changes. Once the
// estimates have converged the flows move by a few ulps per round and their high words
// stay put, so a round writes 4 instead of 8 bytes per edge (the store of an identical
// word is skipped; the value in memory is always the exact f_r).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ long long fhi_idx(int e) { return ((long long)(e & ~31) << 1) | (e & 31); }
// (non-temporal flow loads, stores or both measured slower again in round 5: ER-1M kernel 8
// +1.4 / +1.2 / +3.2 %, R-MAT-24 +1.2 / +8.9 / +11 %, profiles/r05/p)
__device__ __forceinline__ double ld_f(const double *F, int e) {
  const unsigned *w = reinterpret_cast<const unsigned *>(F);
  const long long i = fhi_idx(e);
  return __hiloint2double((int)w[i], (int)w[i + 32]);
}
__device__ __forceinline__ void st_fw(unsigned *p, unsigned v) { *p = v; }
// store f_r over f_old (the value the slot held)
__device__ __forceinline__ void st_f(double *F, int e, double v, double f_old) {
  unsigned *w = reinterpret_cast<unsigned *>(F);
  const long long i = fhi_idx(e);
  st_fw(w + i + 32, (unsigned)__double2loint(v));
  if (__double2hiint(v) != __double2hiint(f_old)) st_fw(w + i, (unsigned)__double2hiint(v));
}
__device__ __forceinline__ void st_f_full(double *F, int e, double v) {
  unsigned *w = reinterpret_cast<unsigned *>(F);
  const long long i = fhi_idx(e);
  st_fw(w + i + 32, (unsigned)__double2loint(v));
  st_fw(w + i, (unsigned)__double2hiint(v));
}

// Flow mode of a round launch (fm): round 0 writes no flows at all. f_{r-2} of round 1 is
// f_{-1} = -0.0 and f_{r-2} of round 2 is f_0 = (0.0 + a_0[i]) - 0.0 (CA:117 on zero state),
// a per-row constant of a_{r-2}[i] = own2, so rounds 1 and 2 compute the old flow instead of
// reading it (fm = 1, 2; fm = 0: read F) and store both words of the new one (the slot holds
// no earlier value). fu_get_flows after round 0 materialises f_0 (k_round0_flows).
__device__ __forceinline__ double old_flow(int fm, double own2) { return fm == 1 ? -0.0 : (0.0 + own2) - 0.0; }
__device__ __forceinline__ double ld_fo(const double *F, int e, int fm, double own2) {
  return fm == 0 ? ld_f(F, e) : old_flow(fm, own2);
}
__device__ __forceinline__ void st_fo(double *F, int e, double v, double f_old, int fm) {
  if (fm) st_f_full(F, e, v);
  else st_f(F, e, v, f_old);
}

// Round 0's flows, one thread per edge: f_0[e] = (0.0 + a_0[row]) - 0.0 into F[0]
// (CA:117 on zero state) and, if F1 is given, f_{-1} = -0.0 into F[1] (split words). The
// rounds never need them (fm above); fu_get_flows after round 0 does. A block owns kR0E consecutive edges: the host
// listed the row of every block's first edge (blk_row), the block's rows' pointers go to
// LDS, and each edge's row is a short binary search there (a hub's edges all land in one
// row; a block whose rows span more than kR0E, runs of isolated nodes, searches rowptr).
__global__ __launch_bounds__(kBlock) void k_round0_flows(long long E, const int *__restrict__ rowptr,
                                                         const int *__restrict__ blk_row,
                                                         const double *__restrict__ a, double *__restrict__ F0,
                                                         double *__restrict__ F1) {
  __shared__ int s_r[2];
  __shared__ int s_rp[kR0E + 1];
  const long long e0 = (long long)blockIdx.x * kR0E;
  const int t = threadIdx.x;
  if (t < 2) s_r[t] = blk_row[blockIdx.x + t];  // rows holding edges e0 and e0 + kR0E (host)
  __syncthreads();
  const int r0 = s_r[0], span = s_r[1] - s_r[0] + 1;
  const bool lds = span <= kR0E;
  if (lds)
    for (int q = t; q <= span; q += kBlock) s_rp[q] = rowptr[r0 + q];
  __syncthreads();
  // thread t: edges k0 .. k0 + 3, 4-aligned, so each split-word store is one 16-byte lane store
  const long long k0 = e0 + 4 * t;
  if (k0 >= E) return;
  auto rp = [&](int q) { return lds ? s_rp[q] : rowptr[r0 + q]; };
  int lo = 0, hi = span - 1;  // row of k0 relative to r0
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rp(mid) <= k0) lo = mid; else hi = mid - 1;
  }
  unsigned hw[4], lw[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long k = k0 + u;
    while (lo + 1 < span && rp(lo + 1) <= k) ++lo;  // next rows (empty ones skipped)
    const double fv = k < E ? (0.0 + a[r0 + lo]) - 0.0 : 0.0;
    hw[u] = (unsigned)__double2hiint(fv);
    lw[u] = (unsigned)__double2loint(fv);
  }
  // split words: block k / 32 holds 32 high words, then 32 low words; E is padded to whole
  // 32-edge blocks in F, so the tail lanes write padding
  const long long j = ((k0 & ~31LL) << 1) | (k0 & 31);
  unsigned *w0 = reinterpret_cast<unsigned *>(F0), *w1 = reinterpret_cast<unsigned *>(F1);
  *reinterpret_cast<uint4 *>(w0 + j) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
  *reinterpret_cast<uint4 *>(w0 + j + 32) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
  if (!F1) return;
  const unsigned mh = (unsigned)__double2hiint(-0.0), ml = (unsigned)__double2loint(-0.0);
  *reinterpret_cast<uint4 *>(w1 + j) = make_uint4(mh, mh, mh, mh);
  *reinterpret_cast<uint4 *>(w1 + j + 32) = make_uint4(ml, ml, ml, ml);
}

// ------------------------------------------------------------------------------------
// Variant 4: flow reconstruction ("recon"). Node j computed, in round r-1,
//     f_{r-1}[j->i] = ((-f_{r-2}[i->j]) + a_{r-1}[j]) - a_{r-2}[i]        (CA:99, CA:117)
// from three operands that node i also holds: its own previous flow f_{r-2}[i->j] (its
// own row), its own estimate a_{r-2}[i], and j's estimate a_{r-1}[j]. So i recomputes the
// reverse flow with the same IEEE operations on the same operands, and gets the same bits,
// instead of gathering f_old[rev[e]] from a 64 MB array. Per edge, the only random access
// left is a_{r-1}[col e] (8 B from an 8 MB array). Flows are updated in place: round r
// reads f_{r-2} and writes f_r in the same rows, owned by the same block. Buffers:
// F[r & 1], A[r % 3] (see launch_round). Round 1 reads f_{-1} = -0.0, a_{-1} = 0.0, which
// reproduces round 0's (0.0 + a) - 0.0 exactly.
// ------------------------------------------------------------------------------------
__device__ inline double recon_fr(double f_own_old, double a_nb, double a_own_old2) {
  const double f_rev = ((-f_own_old) + a_nb) - a_own_old2;  // j's f_{r-1}[j->i], bitwise
  return -f_rev;                                            // CA:99 flows[j] = -msg.flow
}

__device__ inline void wave_sync() {
  // LDS traffic of one wave is processed in order; this only stops the compiler from moving
  // LDS accesses across the hand-off between lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Exact left-to-right chains S += xs[q], T += es[q] over q = 0 .. cn-1 (one whole wave;
// S and T lane-uniform in and out). Even lanes run the S chain, odd lanes the T chain, so
// one fp64 add per element advances both sums: a wave64 v_add_f64 occupies the SIMD for the
// same cycles whatever the EXEC mask, and two separate chains cost two. The LDS reads of
// the next B elements are issued before the dependent adds of the current B (B = 16: the adds
// of one batch cover the LDS latency of the next), into two register batches used in turn
// (no register copies: those cost two more VALU instructions per element). The caller
// keeps xs and es in different LDS banks (es = xs + 8 TE + 8 bytes in the tiles), so the
// two addresses of one read do not conflict.
template <int B = kChainB>
__device__ __forceinline__ void chain_sum(const double *xs, const double *es, int cn, double &S, double &T) {
  const bool odd = threadIdx.x & 1;
  const double *src = odd ? es : xs;
  double acc = odd ? T : S;
  int q = 0;
  if (cn >= B) {
    double a[B], c[B];
#pragma unroll
    for (int k = 0; k < B; ++k) a[k] = src[k];
    q = B;
    for (;;) {
      if (q + B > cn) {
#pragma unroll
        for (int k = 0; k < B; ++k) acc = acc + a[k];
        break;
      }
#pragma unroll
      for (int k = 0; k < B; ++k) c[k] = src[q + k];
#pragma unroll
      for (int k = 0; k < B; ++k) acc = acc + a[k];
      q += B;
      if (q + B > cn) {
#pragma unroll
        for (int k = 0; k < B; ++k) acc = acc + c[k];
        break;
      }
#pragma unroll
      for (int k = 0; k < B; ++k) a[k] = src[q + k];
#pragma unroll
      for (int k = 0; k < B; ++k) acc = acc + c[k];
      q += B;
    }
  }
  for (; q < cn; ++q) acc = acc + src[q];
  S = __shfl(acc, 0);
  T = __shfl(acc, 1);
}


// Heavy rows (one per wave) up to 64 x max(kHeavyRL, chunk / 64) edges keep their operands
// in registers (measured on R-MAT-24: 8 or 16 per lane cost more in occupancy than the
// second pass they save).
// kernel 9's second heavy launch: rows of 64 x (kHeavyRL, kMidRL] edges keep their operands
// in registers (no second pass over the row for its flows), at a lower occupancy than the
// other heavy rows can afford (R-MAT-24: 19 % of the edges sit in rows of 641-1024)

// PRE (kernel 9): every edge's estimate a_{r-1}[col e] was pre-gathered into Gb[e] (edge
// order) by the two staging passes; the tile reads it coalesced instead of col + gather.
template <bool CHECK, int TE = kTileEdges, int TN = kTileNodes, int PART = 0,
          bool PRE = false, int HRL = kHeavyRL, bool RF = true>
__global__ __launch_bounds__(kBlock, (HRL > kHeavyRL ? 3 : 1)) void k_round_recon(
    const int4 *__restrict__ tiles, const int *__restrict__ rowptr,
    const int *__restrict__ col, const double *__restrict__ v, double *__restrict__ F,
    const double *__restrict__ a_prev, const double *__restrict__ a_prev2,
    double *__restrict__ a_new, const double *__restrict__ target,
    unsigned long long *__restrict__ err,
    const void *__restrict__ code_prev, void *__restrict__ code_new, PackCtl *__restrict__ ctl,
    int rslot, const double2 *__restrict__ hubxy, const int *__restrict__ hub_off,
    const int *__restrict__ hrows, int hub_sep, const double *__restrict__ Gb, int fm,
    const unsigned short *__restrict__ col16 = nullptr, const int *__restrict__ cbase = nullptr,
    const int *__restrict__ tnar = nullptr) {
  static_assert(TE % kBlock == 0 && TN <= kBlock && TN <= 256, "tile geometry");
  const PackCtl pp = ctl[rslot ^ 1];  // packing of a_{r-1} (the table gathered here)
  const PackCtl pc = ctl[2];          // packing of a_r (the table written here)
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl[rslot] = pc;
  __shared__ double s_x[TE];   // f_{r-2} on load, fr after phase B
  __shared__ double s_er_buf[TE + 2];  // a_{r-1}[col e], one double off s_x's banks
  double *const s_er = s_er_buf + 1;
  __shared__ unsigned char s_own[TE];
  __shared__ int s_rp[TN + 1];
  __shared__ double s_a[TN];
  const int t = threadIdx.x;
  const int4 tl = tiles[blockIdx.x];
  unsigned long long eb = 0;


  if constexpr (PART != 1) {  // heavy tiles (PART 1: light tiles only, 64 VGPRs)
  if (tl.y == -4) {
    // ---------------- heavy rows, one per wave ----------------
    // Rows hrows[tl.x .. tl.x + tl.z) (degree > hub_threshold, <= mega_hub, sorted by
    // degree so a block's waves finish together): wave w owns one row and its quarter of
    // s_x / s_er, stages the row chunk by chunk (each lane TE / 256 elements), runs the
    // exact left-to-right chain (lane-uniform) and rewrites the row's flows. No block
    // barrier: 4 rows per block progress independently.
    constexpr int CH = TE / 4, PL = CH / 64;
    const int w = t >> 6, lane = t & 63;
    if (w < tl.z) {
      const int i = hrows[tl.x + w];
      const int b = rowptr[i], e = rowptr[i + 1], d = e - b;
      const double own2 = a_prev2[i];
      double *xs = s_x + w * CH, *es = s_er + w * CH;
      double S = 0.0, T = 0.0;
      constexpr int RL = HRL > PL ? HRL : PL;  // whole chunks (TE 2048: PL = 8)
      if (d <= 64 * RL) {
        // the whole row in registers (RL elements per lane, all loads in flight at
        // once): the chain runs chunk by chunk through the wave's LDS quarter and the flows
        // are written from the same registers, with no second pass over the row
        double fo[RL], er[RL];
        int cc[RL];
#pragma unroll
        for (int u = 0; u < RL; ++u) {
          const int k = lane + 64 * u;
          if constexpr (PRE) er[u] = k < d ? Gb[b + k] : 0.0;
          else cc[u] = k < d ? col[b + k] : 0;
          fo[u] = k < d ? ld_fo(F, b + k, fm, own2) : 0.0;
        }
        if constexpr (!PRE) {
#pragma unroll
          for (int u = 0; u < RL; ++u) er[u] = lane + 64 * u < d ? ld_est(pp, code_prev, a_prev, cc[u]) : 0.0;
        }
#pragma unroll
        for (int c = 0; c < RL / PL; ++c) {
          if (c * CH < d) {
            wave_sync();  // the previous chunk's chain is done with the buffer
#pragma unroll
            for (int j = 0; j < PL; ++j) {
              xs[lane + 64 * j] = recon_fr(fo[c * PL + j], er[c * PL + j], own2);
              es[lane + 64 * j] = er[c * PL + j];
            }
            wave_sync();
            // the register-resident mid launch: 8-element batches (its rows hold 64 VGPRs)
            chain_sum<(HRL > kHeavyRL ? 8 : kChainB)>(xs, es, min(CH, d - c * CH), S, T);
          }
        }
        const double a = ((v[i] - S) + T) / (double)(d + 1);
        if (lane == 0) {
          *(a_new + i) = a;
          if (pc.width) put_code(pc, code_new, i, a);
          if (CHECK) eb = err_bits(a, target[i]);
        }
#pragma unroll
        for (int u = 0; u < RL; ++u) {  // flows (CA:117-118)
          const int k = lane + 64 * u;
          if (k < d) st_fo(F, b + k, (recon_fr(fo[u], er[u], own2) + a) - er[u], fo[u], fm);
        }
      } else {
      // longer rows: chunk by chunk, the next chunk's loads in flight during this chunk's
      // chain; the flows in a second pass
      double fo[PL], er[PL], nf[PL], ng[PL];
      int nc[PL];
      auto fetch = [&](int c0) {
#pragma unroll
        for (int u = 0; u < PL; ++u) {
          const int k = c0 + lane + 64 * u;
          if constexpr (PRE) ng[u] = k < d ? Gb[b + k] : 0.0;
          else nc[u] = k < d ? col[b + k] : 0;
          nf[u] = k < d ? ld_fo(F, b + k, fm, own2) : 0.0;
        }
      };
      fetch(0);
      for (int c0 = 0; c0 < d; c0 += CH) {
#pragma unroll
        for (int u = 0; u < PL; ++u) {
          fo[u] = nf[u];
          if constexpr (PRE) er[u] = ng[u];
          else er[u] = c0 + lane + 64 * u < d ? ld_est(pp, code_prev, a_prev, nc[u]) : 0.0;
        }
        if (c0 + CH < d) fetch(c0 + CH);
        wave_sync();  // the previous chunk's chain is done with the buffer
#pragma unroll
        for (int u = 0; u < PL; ++u) {
          xs[lane + 64 * u] = recon_fr(fo[u], er[u], own2);
          es[lane + 64 * u] = er[u];
        }
        wave_sync();
        chain_sum(xs, es, min(CH, d - c0), S, T);
      }
      const double a = ((v[i] - S) + T) / (double)(d + 1);
      if (lane == 0) {
        *(a_new + i) = a;
        if (pc.width) put_code(pc, code_new, i, a);
        if (CHECK) eb = err_bits(a, target[i]);
      }
      for (int k0 = 0; k0 < d; k0 += 8 * 64) {  // flows (CA:117-118), 8 loads in flight per lane
        int cc[8];
        double fo[8], er[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + lane + 64 * u;
          if constexpr (PRE) er[u] = k < d ? Gb[b + k] : 0.0;
          else cc[u] = k < d ? col[b + k] : 0;
          fo[u] = k < d ? ld_fo(F, b + k, fm, own2) : 0.0;
        }
        if constexpr (!PRE) {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            er[u] = k0 + lane + 64 * u < d ? ld_est(pp, code_prev, a_prev, cc[u]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + lane + 64 * u;
          if (k < d) st_fo(F, b + k, (recon_fr(fo[u], er[u], own2) + a) - er[u], fo[u], fm);
        }
      }
      }  // rows longer than 64 x kHeavyRL
    }
    if (CHECK) block_max_to(eb, err);
    return;
  }

  if (tl.y == -3) {
    // ---------------- mega hub (degree > mega_hub, default 8192) ----------------
    // k_hub_stage has already put (fr, er) of every edge of the row into hubxy (many
    // blocks, coalesced), so the exact left-to-right chain is all that is left: wave 0
    // streams the pairs through two LDS halves (the loads of chunk c + 1 in flight while
    // chunk c is summed), with no block barrier and no gather on the chain's path.
    const int i = tl.x, b = tl.z, e = tl.w;
    const double2 *xy = PRE ? nullptr : hubxy + hub_off[blockIdx.x];
    const int d = e - b;
    double S = 0.0, T = 0.0;
    constexpr int CH = TE / 2, PL = CH / 64;  // pairs per chunk, per lane
    if (PRE && t < 64) {
      // kernel 9: the row's estimates are pre-gathered (Gb), so the chain wave streams Gb
      // and the old flows itself, coalesced, and rebuilds fr as k_hub_stage would
      const double own2 = a_prev2[i];
      double nf[PL], ng[PL];
#pragma unroll
      for (int u = 0; u < PL; ++u) {
        const int k = t + 64 * u;
        nf[u] = k < d ? ld_fo(F, b + k, fm, own2) : 0.0;
        ng[u] = k < d ? Gb[b + k] : 0.0;
      }
      for (int c0 = 0; c0 < d; c0 += CH) {
        double *xs = s_x + ((c0 / CH) & 1) * CH, *es = s_er + ((c0 / CH) & 1) * CH;
#pragma unroll
        for (int u = 0; u < PL; ++u) {
          xs[t + 64 * u] = recon_fr(nf[u], ng[u], own2);
          es[t + 64 * u] = ng[u];
        }
        const int c1 = c0 + CH;
#pragma unroll
        for (int u = 0; u < PL; ++u) {
          const int k = c1 + t + 64 * u;
          nf[u] = k < d ? ld_fo(F, b + k, fm, own2) : 0.0;
          ng[u] = k < d ? Gb[b + k] : 0.0;
        }
        wave_sync();
        chain_sum(xs, es, min(CH, d - c0), S, T);
        wave_sync();
      }
    } else if (!PRE && t < 64) {
      double2 nx[PL];
#pragma unroll
      for (int u = 0; u < PL; ++u) nx[u] = t + 64 * u < d ? xy[t + 64 * u] : make_double2(0.0, 0.0);
      for (int c0 = 0; c0 < d; c0 += CH) {
        double *xs = s_x + ((c0 / CH) & 1) * CH, *es = s_er + ((c0 / CH) & 1) * CH;
#pragma unroll
        for (int u = 0; u < PL; ++u) {
          xs[t + 64 * u] = nx[u].x;
          es[t + 64 * u] = nx[u].y;
        }
        const int c1 = c0 + CH;
#pragma unroll
        for (int u = 0; u < PL; ++u) {
          const int k = c1 + t + 64 * u;
          nx[u] = k < d ? xy[k] : make_double2(0.0, 0.0);
        }
        wave_sync();
        chain_sum(xs, es, min(CH, d - c0), S, T);
        wave_sync();
      }
    }
    if (t == 0) {
      const double a = ((v[i] - S) + T) / (double)(d + 1);
      s_a[0] = a;
      *(a_new + i) = a;
      if (pc.width) put_code(pc, code_new, i, a);
      if (CHECK) eb = err_bits(a, target[i]);
    }
    if (!PRE && !hub_sep) {  // else k_hub_flows writes the row's flows with many blocks
      __syncthreads();
      const double a = s_a[0];
      for (int k = t; k < d; k += kBlock) {
        const double2 p2 = xy[k];
        st_fo(F, b + k, (p2.x + a) - p2.y, fm ? 0.0 : ld_f(F, b + k), fm);
      }
    }
    if (CHECK) block_max_to(eb, err);
    return;
  }

  if (tl.y < 0) {
    // ---------------- heavy node ----------------
    // chunks of CH = TE / 2 in the two halves of s_x / s_er: wave 0 runs the exact
    // left-to-right chain of chunk c (lane-uniform) while waves 1-3 stage chunk c + 1
    const int i = tl.x;
    const int b = rowptr[i], e = rowptr[i + 1];
    const double own2 = a_prev2[i];
    double S = 0.0, T = 0.0;
    constexpr int CH = TE / 2;
    const int nch = (e - b + CH - 1) / CH;
    auto stage = [&](int c, int tid, int nthr) {
      const int c0 = b + c * CH, cn = min(CH, e - c0);
      double *xs = s_x + (c & 1) * CH, *es = s_er + (c & 1) * CH;
      for (int q = tid; q < cn; q += nthr) {
        const double er = PRE ? Gb[c0 + q] : ld_est(pp, code_prev, a_prev, col[c0 + q]);
        xs[q] = recon_fr(ld_fo(F, c0 + q, fm, own2), er, own2);
        es[q] = er;
      }
    };
    if (nch > 0) stage(0, t, kBlock);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      if (t >= 64) {
        if (c + 1 < nch) stage(c + 1, t - 64, kBlock - 64);
      } else {
        chain_sum(s_x + (c & 1) * CH, s_er + (c & 1) * CH, min(CH, e - (b + c * CH)), S, T);
      }
      __syncthreads();
    }
    if (t == 0) {
      const double a = ((v[i] - S) + T) / (double)(e - b + 1);
      s_a[0] = a;
      *(a_new + i) = a;
      if (pc.width) put_code(pc, code_new, i, a);
      if (CHECK) eb = err_bits(a, target[i]);
    }
    __syncthreads();
    const double a = s_a[0];
    for (int k = b + t; k < e; k += kBlock) {
      const double er = PRE ? Gb[k] : ld_est(pp, code_prev, a_prev, col[k]);
      const double fo = ld_fo(F, k, fm, own2);
      st_fo(F, k, (recon_fr(fo, er, own2) + a) - er, fo, fm);
    }
    if (CHECK) block_max_to(eb, err);
    return;
  }
  }  // PART != 1
  if constexpr (PART != 2) {  // light tiles

  // ---------------- light tile ----------------
  // Every global load of the tile is issued up front with no dependence on an earlier load
  // except the a_{r-1}[col] gathers (one hop): 2 serial memory latencies per tile.
  const int nb = tl.x, nn = tl.y - tl.x;
  const int e0 = tl.z, ne = tl.w - tl.z;
  constexpr int kPer = TE / kBlock;
  int c[kPer];
  double x[kPer], g[kPer];
  int rp, rp_last = 0;
  double vv, own2;
  if constexpr (PRE) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int q = t + k * kBlock;
      c[k] = 0;
      x[k] = 0.0;
      g[k] = 0.0;
      if (q < ne) {
        g[k] = Gb[e0 + q];
        x[k] = fm ? 0.0 : ld_f(F, e0 + q);
      }
    }
    rp = t <= nn ? rowptr[nb + t] : 0;
    if constexpr (TN == kBlock) rp_last = (t == 0 && nn == kBlock) ? rowptr[nb + kBlock] : 0;
    vv = t < nn ? v[nb + t] : 0.0;
    own2 = t < nn ? a_prev2[nb + t] : 0.0;
  } else {
    // the column indices first, then the flows (RF: round >= 3) and node words, every load
    // unconditional from a clamped index (col and F hold at least one element / 32-edge
    // block), so the gathers wait for the indices alone (in-order completion, vmcnt(N))
    // narrow tiles (tnar: every 1024-edge block of the tile has its columns within 32K ids of
    // the block's first row, cbase): a 2-byte offset per edge instead of the 4-byte column.
    // The column is formed after the flow and node loads are issued (below), so those stay
    // in flight while the gathers wait for the indices.
    const bool narrow = tnar && tnar[blockIdx.x];
    int cw[kPer], bs[kPer];
    if (narrow) {
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const int q = t + k * kBlock;
        const int ci = q < ne ? e0 + q : (ne > 0 ? e0 : 0);
        cw[k] = col16[ci];
        bs[k] = cbase[ci >> 10];
      }
    } else {
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const int q = t + k * kBlock;
        const int ci = q < ne ? e0 + q : (ne > 0 ? e0 : 0);
        cw[k] = col[ci];
        bs[k] = 32768;
      }
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) g[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int q = t + k * kBlock;
      if constexpr (RF) {
        const double f = ld_f(F, q < ne ? e0 + q : 0);
        x[k] = q < ne ? f : 0.0;
      } else {
        x[k] = 0.0;
      }
    }
    const int tn = min(t, nn - 1);  // a light tile has at least one node
    const int rp0 = rowptr[nb + min(t, nn)];
    const double v0 = v[nb + tn], o0 = a_prev2[nb + tn];
    int rl0 = 0;
    if constexpr (TN == kBlock) rl0 = rowptr[nb + nn];  // the tile's end (256-node tiles)
    asm volatile("" ::: "memory");  // the loads above are issued before the first wait
    rp = t <= nn ? rp0 : 0;
    if constexpr (TN == kBlock) rp_last = (t == 0 && nn == kBlock) ? rl0 : 0;
    vv = t < nn ? v0 : 0.0;
    own2 = t < nn ? o0 : 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) c[k] = t + k * kBlock < ne ? bs[k] + cw[k] - 32768 : 0;
  }
  if (PRE) {
  } else if (pp.width == 0) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int q = t + k * kBlock;
      g[k] = q < ne ? a_prev[c[k]] : 0.0;
    }
  } else if (pp.width == 8) {
    gather_packed<8>(c, g, t, ne, code_prev, pp.base, a_prev);
  } else if (pp.width == 16) {
    gather_packed<16>(c, g, t, ne, code_prev, pp.base, a_prev);
  } else {
    gather_packed<32>(c, g, t, ne, code_prev, pp.base, a_prev);
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int q = t + k * kBlock;
    if (q < ne) {
      s_x[q] = x[k];
      s_er[q] = g[k];
    }
  }
  if (t <= nn) s_rp[t] = rp;
  if constexpr (TN == kBlock) {
    if (t == 0 && nn == kBlock) s_rp[kBlock] = rp_last;
  }
  __syncthreads();
  // phase B: per node, reconstruct fr and sum in row order (CA:106-113)
  if (t < nn) {
    const int qb = s_rp[t] - e0, qe = s_rp[t + 1] - e0;
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
  // phase C: new flows, coalesced, in place (CA:117-118)
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int q = t + k * kBlock;
    if (q < ne) {
      st_fo(F, e0 + q, (s_x[q] + s_a[s_own[q]]) - s_er[q], x[k], fm);
    }
  }
  if (CHECK) block_max_to(eb, err);
  }  // PART != 2
}

// Mega hubs: (fr, er) of every hub edge into hubxy, hub-major (CA:98-99 + the flow
// reconstruction of kernel 4), so k_round_recon's hub block only runs the chain.
__global__ __launch_bounds__(kBlock) void k_hub_stage(int nhub, const int4 *__restrict__ hubs,
                                                      long long total, const int *__restrict__ col,
                                                      const double *__restrict__ F,
                                                      const double *__restrict__ a_prev,
                                                      const double *__restrict__ a_prev2,
                                                      const void *__restrict__ code_prev,
                                                      const PackCtl *__restrict__ ctl, int rslot,
                                                      double2 *__restrict__ hubxy, int fm,
                                                      const int *__restrict__ hub_blk) {
  const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= total) return;
  // hubs[h] = {node, row begin, row end, offset}: the block's first edge's hub from the host
  // table (a hub of > mega_hub edges spans whole blocks), then at most a step or two on
  int lo = hub_blk[blockIdx.x];
  while (lo + 1 < nhub && hubs[lo + 1].w <= q) ++lo;
  const int4 hb = hubs[lo];
  const int k = hb.y + (int)(q - hb.w);
  const PackCtl pp = ctl[rslot ^ 1];
  const double er = ld_est(pp, code_prev, a_prev, col[k]);
  const double own2 = a_prev2[hb.x];
  hubxy[q] = make_double2(recon_fr(ld_fo(F, k, fm, own2), er, own2), er);
}


// Mega hubs: the flows of every hub edge (CA:117-118) once the hub blocks have written a_r,
// with many blocks (the hub block's own loop would hold one CU for d / 256 iterations on
// the round's critical path).
__global__ __launch_bounds__(kBlock) void k_hub_flows(int nhub, const int4 *__restrict__ hubs, long long total,
                                                      const double2 *__restrict__ hubxy,
                                                      const double *__restrict__ a_new, double *__restrict__ F,
                                                      const double *__restrict__ Gb,
                                                      const double *__restrict__ a_prev2, int fm,
                                                      const int *__restrict__ hub_blk) {
  const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= total) return;
  // hubs[h] = {node, row begin, row end, offset}: the block's first edge's hub from the host
  // table (a hub of > mega_hub edges spans whole blocks), then at most a step or two on
  int lo = hub_blk[blockIdx.x];
  while (lo + 1 < nhub && hubs[lo + 1].w <= q) ++lo;
  const int4 hb = hubs[lo];
  const int k = hb.y + (int)(q - hb.w);
  const double a = a_new[hb.x];
  if (Gb) {  // kernel 9: (fr, er) rebuilt from the pre-gathered estimate and the old flow
    const double own2 = a_prev2[hb.x];
    const double er = Gb[k], fo = ld_fo(F, k, fm, own2);
    st_fo(F, k, (recon_fr(fo, er, own2) + a) - er, fo, fm);
    return;
  }
  const double2 p2 = hubxy[q];
  st_fo(F, k, (p2.x + a) - p2.y, fm ? 0.0 : ld_f(F, k), fm);
}

// split-word flows -> doubles (fu_get_flows of kernels >= 4)
__global__ void k_unsplit(long long cnt, const double *__restrict__ src, double *__restrict__ dst) {
  long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (q < cnt) dst[q] = ld_f(src, (int)q);
}
// fu_copy_bandwidth: a plain float4 copy, grid-stride (the part's streaming rate)
__global__ __launch_bounds__(kBlock) void k_copy4(long long cnt, const float4 *__restrict__ src,
                                                  float4 *__restrict__ dst) {
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < cnt; q += stride) dst[q] = src[q];
}

__global__ __launch_bounds__(kBlock) void k_max_err(int n, const double *__restrict__ a,
                                                    const double *__restrict__ target,
                                                    unsigned long long *__restrict__ err) {
  unsigned long long eb = 0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    unsigned long long x = err_bits(a[i], target[i]);
    eb = x > eb ? x : eb;
  }
  block_max_to(eb, err);
}

}  // namespace
