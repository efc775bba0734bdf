// Collect-all engine, piece 1 of 7: the packed estimate table. The pieces (fu_ca_pack.h,
// fu_ca_recon.h, fu_ca_stage.h, fu_ca_pregather.h, fu_ca_handle.h, fu_ca_layout.h,
// fu_ca_launch.h) are included by fu_engine.hip, in that order, into ONE translation unit:
// every kernel is compiled once, there. A piece includes only earlier pieces.
#pragma once

#include <hip/hip_runtime.h>

#include "fu_common.h"
#include "fu_plan.h"

// ------------------------------------------------------------------------------------
// Packed estimate table (kernel 4). Once the estimates have converged into a narrow
// cluster, the neighbour gather reads a W-bit code per node (W = 8, 16 or 32) instead of
// the 8-byte double: a 1-4 MB table instead of 8 MB for ER-1M, so the random gathers hit
// the XCD's L2. The code is a LOSSLESS offset of the double's order-preserving 64-bit key
// from a per-table base: key(x) - base in [0, 2^W - 2]. Any estimate outside that window
// is stored as the escape code 2^W - 1, and its reader gathers the double instead. Every
// decoded value is the exact bit pattern, so the results are unchanged. Each round writes
// the doubles (coalesced, always) and, when packing is on, the codes under the parameters
// pack_plan chose from a sample of gather targets. Slots: ctl[r & 1] describes the code
// table written in round r (copied by block 0 from ctl[2], the current encoding plan);
// width 0 = no codes (the reader gathers the doubles).
// ------------------------------------------------------------------------------------
namespace fu {  // a named namespace: fu_handle points to it, and fu_dist.hip sees fu_handle too
struct PackCtl {
  unsigned long long base;
  int width;
  int pad;
};
}  // namespace fu

using namespace fu;
namespace FP = fu::plan;

namespace {

constexpr int kBlock = 256;      // threads per block (4 waves of 64)

// Round outputs (flows, estimates, codes) use plain write-back stores. Write-through (sc1)
// stores, so that no dirty lines wait for the launch boundary's L2 writeback, were measured
// in round 2 and removed: on ER-1M kernel 4 lost 4.5 us per round and kernel 8 gained nothing.

__device__ inline unsigned long long dkey(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ inline double dkey_inv(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  return __longlong_as_double((long long)b);
}
template <int W>
__device__ inline unsigned ld_code(const void *tab, int i) {
  if constexpr (W == 8) return reinterpret_cast<const unsigned char *>(tab)[i];
  else if constexpr (W == 16) return reinterpret_cast<const unsigned short *>(tab)[i];
  else return reinterpret_cast<const unsigned *>(tab)[i];
}
__device__ inline void put_code(const PackCtl &pc, void *tab, int i, double a) {
  const unsigned long long off = dkey(a) - pc.base;
  const unsigned esc = pc.width == 32 ? 0xFFFFFFFFu : (1u << pc.width) - 1u;
  const unsigned cd = off < (unsigned long long)esc ? (unsigned)off : esc;
  if (pc.width == 8) *(reinterpret_cast<unsigned char *>(tab) + i) = (unsigned char)cd;
  else if (pc.width == 16) *(reinterpret_cast<unsigned short *>(tab) + i) = (unsigned short)cd;
  else *(reinterpret_cast<unsigned *>(tab) + i) = cd;
}
template <int W>
__device__ inline double decode_or(unsigned cd, unsigned long long base, const double *a_prev, int j) {
  constexpr unsigned esc = W == 32 ? 0xFFFFFFFFu : (1u << W) - 1u;
  return cd == esc ? a_prev[j] : dkey_inv(base + cd);
}
// One neighbour estimate a_{r-1}[j] under the table's packing (uniform branch).
__device__ inline double ld_est(const PackCtl &pp, const void *codes, const double *a_prev, int j) {
  if (pp.width == 8) return decode_or<8>(ld_code<8>(codes, j), pp.base, a_prev, j);
  if (pp.width == 16) return decode_or<16>(ld_code<16>(codes, j), pp.base, a_prev, j);
  if (pp.width == 32) return decode_or<32>(ld_code<32>(codes, j), pp.base, a_prev, j);
  return a_prev[j];
}
// The light tile's kPer neighbour estimates: all code loads first, then decode (escapes
// gather the double).
template <int W, int KP>
__device__ inline void gather_packed(const int (&c)[KP], double (&g)[KP], int t, int ne,
                                     const void *codes, unsigned long long base,
                                     const double *a_prev) {
  unsigned cd[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) cd[k] = t + k * kBlock < ne ? ld_code<W>(codes, c[k]) : 0u;
#pragma unroll
  for (int k = 0; k < KP; ++k) g[k] = t + k * kBlock < ne ? decode_or<W>(cd[k], base, a_prev, c[k]) : 0.0;
}
// Encoding plan from the estimates a_r of a fixed sample of kPlanSamples gather targets:
// the centre is the median of the first 64 sampled keys; the width is the smallest W whose
// window [centre - 2^(W-1), centre + 2^(W-1) - 2] holds >= 99.5 % of the sample; else 0.
constexpr int kPlanSamples = 4096;

// NT threads (every lane in flight: kPlanSamples / NT sample loads, then as many gathers).
// pw_host (pinned host memory, or null) receives the width for the autotuner's poll, so no
// copy sits on the round's stream.
template <int NT>
__device__ __forceinline__ void plan_body(const double *__restrict__ a, const int *__restrict__ sample,
                                          PackCtl *ctl, int *pw_host) {
  constexpr int kPer = kPlanSamples / NT;
  __shared__ unsigned long long s_centre;
  __shared__ int s_cnt[3];
  const int t = threadIdx.x;
  if (t < 3) s_cnt[t] = 0;
  int idx[kPer];
  unsigned long long key[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) idx[k] = sample[t + k * NT];  // all loads in flight
#pragma unroll
  for (int k = 0; k < kPer; ++k) key[k] = dkey(a[idx[k]]);
  if (t < 64) {  // median of samples 0..63: rank by comparison against every lane
    int below = 0;
    for (int l = 0; l < 64; ++l) {
      const unsigned long long o = __shfl(key[0], l, 64);
      below += (o < key[0]) || (o == key[0] && l < t);
    }
    if (below == 32) s_centre = key[0];
  }
  __syncthreads();
  const unsigned long long c = s_centre;
  int n8 = 0, n16 = 0, n32 = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const unsigned long long d = key[k] >= c ? key[k] - c : c - key[k];
    n8 += d + 2 <= (1ull << 7);
    n16 += d + 2 <= (1ull << 15);
    n32 += d + 2 <= (1ull << 31);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // wave sums, then one LDS add per wave
    n8 += __shfl_xor(n8, o, 64);
    n16 += __shfl_xor(n16, o, 64);
    n32 += __shfl_xor(n32, o, 64);
  }
  if ((t & 63) == 0) {
    atomicAdd(&s_cnt[0], n8);
    atomicAdd(&s_cnt[1], n16);
    atomicAdd(&s_cnt[2], n32);
  }
  __syncthreads();
  if (t == 0) {
    const int need = kPlanSamples - kPlanSamples / 200;
    const int w = s_cnt[0] >= need ? 8 : s_cnt[1] >= need ? 16 : s_cnt[2] >= need ? 32 : 0;
    PackCtl p;
    p.base = w ? c - (1ull << (w - 1)) : 0;
    p.width = w;
    p.pad = 0;
    ctl[2] = p;
    if (pw_host) *pw_host = w;
  }
}

__global__ __launch_bounds__(kBlock) void k_pack_plan(const double *__restrict__ a,
                                                      const int *__restrict__ sample,
                                                      PackCtl *__restrict__ ctl, int *pw_host) {
  plan_body<kBlock>(a, sample, ctl, pw_host);
}

}  // namespace
