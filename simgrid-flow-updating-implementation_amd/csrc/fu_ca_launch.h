// Collect-all engine, piece 7 of 7 (see fu_ca_pack.h): the round launchers of kernels 4, 8
// and 9, round 0, and launch_round, which the entry points and the autotuner call.
#pragma once

#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>

#include "fu_ca_layout.h"

namespace {

// row-class and table constants shared with the host plans (fu_plan.h)
using FP::kMidRL;
using FP::kStageTE;
using FP::kStageTN;

inline unsigned grid_for(long long work) { return (unsigned)((work + kBlock - 1) / kBlock); }

// k_transpose grid for nbk buckets: 8 XCDs x min(buckets per XCD, tr_bpx blocks per XCD)
// (tr_bpx 0: one block per bucket)
inline unsigned tr_grid(fu_handle *h, int nbk) {
  const int per = (nbk + 7) / 8;
  return 8u * (unsigned)(h->tr_bpx > 0 ? std::min(per, h->tr_bpx) : per);
}

// the packing plan as a one-block launch ahead of the round (paths without a stage launch)
void plan_alone(fu_handle *h, RoundCtx &c) {
  if (!c.plan) return;
  hipLaunchKernelGGL(k_pack_plan, dim3(1), dim3(kBlock), 0, h->stream, c.ap, h->psample, h->pctl, h->pw_dev);
  c.plan = false;
}

// Round 0 = the timeout fire on zero state (CA:33-34, CA:87-91): a_0 and a_{-1} = 0.0; no
// flows are written (rounds 1 and 2 compute f_{-1} and f_0 themselves: fm).
int launch_round0(fu_handle *h, RoundCtx &c) {
  static_assert(sizeof(PackCtl) * 3 == 6 * sizeof(unsigned long long), "k_round0 clears 3 PackCtl");
  h->lagf[0] = h->lagf[1] = 0;  // zero state: no lagged flows
  if (h->r0_start) {  // a timed window's first mark: the kernel's own start (hipExtLaunchKernel)
    hipExtLaunchKernelGGL(k_round0, dim3(grid_for(std::max(h->na, 6))), dim3(kBlock), 0, h->stream, h->r0_start,
                          h->r0_stop, 0, h->n, h->na, (const int *)h->rowptr, (const double *)h->v, h->a[0], h->a[2],
                          reinterpret_cast<unsigned long long *>(h->pctl));
    h->r0_start = h->r0_stop = nullptr;
  } else {
    hipLaunchKernelGGL(k_round0, dim3(grid_for(std::max(h->na, 6))), dim3(kBlock), 0, h->stream, h->n, h->na,
                       h->rowptr, h->v, h->a[0], h->a[2], reinterpret_cast<unsigned long long *>(h->pctl));
  }
  if (c.err)
    hipLaunchKernelGGL(k_max_err, dim3(std::min(1024u, grid_for(h->n))), dim3(kBlock), 0, h->stream, h->n,
                       h->a[0], h->target, c.err);
  if (h->dist) {  // a_0 of the boundary nodes to the peers
    h->halo_a = h->a[0];
    if (int rc = fu__dist_round_hook(h, 2)) return rc;
  }
  return FU_OK;
}

// Kernel 8: k_stage (carrying the packing plan), heavy rows as kernel 4 tiles, then the light
// tiles reading the staged estimates.
int launch_k8(fu_handle *h, RoundCtx &c) {
  constexpr bool C0 = false;
  const int r1 = (int)(c.r & 1);
  unsigned sgrid = 1;
  const StageArgs sa = stage_args(h, &sgrid);
  const void *cp = h->code[(c.r - 1) & 1];
  if (h->st_ntiles) {
    hipLaunchKernelGGL(k_stage, dim3(sgrid + (c.plan ? 8 : 0)), dim3(kStageThreads), 0, h->stream, sa, h->na, c.ap, cp,
                       h->pctl, r1, h->stG, c.plan ? h->psample : nullptr, h->pw_dev);
    c.plan = false;
  }
  plan_alone(h, c);
  auto heavy = [&](auto chk) {
    hipLaunchKernelGGL((k_round_recon<decltype(chk)::value, kStageTE, kStageTN>), dim3(h->st_nheavy),
                       dim3(kBlock), 0, h->stream, h->st_heavy, h->rowptr, h->col, h->v, c.F, c.ap, c.ap2, c.an,
                       h->target, c.err, cp, h->code[r1], h->pctl, r1, nullptr, nullptr, nullptr, 0, nullptr, c.fm);
  };
  if (h->st_nheavy) {
    if (c.err) heavy(std::true_type{});
    else heavy(std::false_type{});
  }
  // light tiles: rounds 1 and 2 (fm) read no flows (RF = false)
  // multi-GPU: the boundary tiles [0, st_nbound), then the halo goes out on the comm stream
  // beside the interior tiles
  auto light = [&](auto chk, auto rf) -> int {
    // multi-GPU: the boundary tiles [0, st_nbound), then the rest
    const int nb = h->dist ? h->st_nbound : 0;
    for (int part = 0; part < 2; ++part) {
      const int t0 = part ? nb : 0, cnt = part ? h->st_ntiles - nb : nb;
      if (cnt)
        hipLaunchKernelGGL((k_round_staged<decltype(chk)::value, kStageTE, kStageTN, decltype(rf)::value>),
                           dim3(cnt), dim3(kBlock), 0, h->stream, h->st_tiles, t0, cnt, h->rowptr, h->col, sa,
                           h->stG, h->v, c.F, c.ap, c.ap2, c.an, h->target, c.err, h->code[r1], h->pctl, r1, c.fm);
      if (!part && h->dist) {  // boundary rows (and the heavy rows) done
        h->halo_a = c.an;
        if (int rc = fu__dist_round_hook(h, 2)) return rc;
      }
    }
    return FU_OK;
  };
  auto light_rf = [&](auto chk) {
    return c.fm ? light(chk, std::false_type{}) : light(chk, std::true_type{});
  };
  if (h->st_ntiles || h->dist) {
    if (c.err) return light_rf(std::true_type{});
    return light_rf(std::integral_constant<bool, C0>{});
  }
  return FU_OK;
}

// Kernel 9: k_stage -> k_transpose (the mega-hub buckets first) -> kernel 4's tiles reading
// the pre-gathered estimates; the mega hubs' chains and k_hub_flows on the side stream beside
// the remaining buckets and tiles.
int launch_k9(fu_handle *h, RoundCtx &c) {
  if (int rc = ensure_transpose(h)) return rc;  // rebuilt after a tile option changed
  double *Gb = h->tr.GBr[c.r % 3];
  const double *Gb_old = h->tr.GBr[(c.r + 1) % 3];  // G_B of round r - 2 (lag)
  if (!Gb) return fail(FU_ERR_STATE, "kernel 9: no pre-gather buffer");
  const int r1 = (int)(c.r & 1);
  const void *cp = h->code[(c.r - 1) & 1];
  // which launch computes which rows (FP::k9_schedule; tools/plan_check.cpp re-runs it)
  FP::K9Opts ko;
  ko.mid_heavy = h->mid_heavy;
  ko.multi_mid = h->multi_mid;
  ko.multi_short = h->multi_short;
  ko.multi_heavy = h->multi_heavy;
  ko.wave_heavy = h->wave_heavy;
  ko.iso_rows = h->iso_rows;
  const FP::K9Sched ks = FP::k9_schedule(h->tiles1, h->n_hub, ko);
  const int nmega = ks.nmega, nh = ks.nh, niso = ks.niso, nl = ks.nl, m0 = ks.m0, m1 = ks.m1;
  const int4 *tl = h->tiles_geo[1];
  const bool hubs = nmega > 0;
  // lag: the rows this round leaves their flows to round r + 2 (k_heavy_multi<LAG>): the
  // multi-row heavy rows
  const int n_multi = ks.n_multi, m1s = ks.m1s;
  const bool multi = ks.multi;
  const bool lag_multi = h->lag && multi;
  const int p = r1;
  if (h->lagf[p] && h->lag_nmulti[p] != (lag_multi ? n_multi : 0)) {
    if (int rc = lag_finalize(h, p)) return rc;  // the lagged set changed: write its flows first
  }
  const int lagm = lag_multi ? (h->lagf[p] ? 2 : 1) : 0;
  StageArgs sa{};
  for (int li = 0; li < 4; ++li) sa.sel[li] = 3;
  sa.P[3] = h->tr.P;
  sa.Q[3] = h->tr.Q;
  sa.SN[3] = kStageLds / 8;
  sa.NB[3] = h->tr.NB;
  sa.brange[3] = h->tr.brange;
  sa.colS[3] = h->tr.colS;
  sa.f64 = 1;
  {
    hipLaunchKernelGGL(k_stage, dim3(h->tr.NB + (c.plan ? 8 : 0)), dim3(kStageThreads), 0, h->stream, sa, h->na, c.ap,
                       cp, h->pctl, r1, h->tr.GA, c.plan ? h->psample : nullptr, h->pw_dev);
    c.plan = false;
  }
  plan_alone(h, c);
  const int bh = hubs ? h->tr.Bh : 0;
  auto tr_launch = [&](int b0, int nb) {
    if (h->tr_nt)
      hipLaunchKernelGGL(k_transpose<true>, dim3(tr_grid(h, nb)), dim3(kTrThreads), 0, h->stream, b0, nb, h->tr.P,
                         (long long)h->E, h->tr.offT, h->tr.GA, h->tr.pos16, Gb);
    else
      hipLaunchKernelGGL(k_transpose<false>, dim3(tr_grid(h, nb)), dim3(kTrThreads), 0, h->stream, b0, nb, h->tr.P,
                         (long long)h->E, h->tr.offT, h->tr.GA, h->tr.pos16, Gb);
  };
  if (bh) tr_launch(0, bh);
  if (hubs) {
    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  }
  if (h->tr.B > bh) tr_launch(bh, h->tr.B - bh);
  const bool chk = c.err != nullptr;
  if (hubs) {
    auto chains = [&](auto C) {
      hipLaunchKernelGGL((k_round_recon<decltype(C)::value, 1024, 128, 2, true>), dim3(nmega), dim3(kBlock),
                         0, h->stream2, tl, h->rowptr, h->col, h->v, c.F, c.ap, c.ap2, c.an, h->target, c.err, cp,
                         h->code[r1], h->pctl, r1, nullptr, nullptr, h->hrows, 1, Gb, c.fm);
    };
    if (chk) chains(std::true_type{});
    else chains(std::false_type{});
    hipLaunchKernelGGL(k_hub_flows, dim3(grid_for(h->hub_total)), dim3(kBlock), 0, h->stream2, h->n_hub, h->hub_rows,
                       (long long)h->hub_total, nullptr, c.an, c.F, Gb, c.ap2, c.fm, h->hub_blk);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev_join, h->stream2));
  }
  // heavy tiles [t0, t1) with RL register elements per lane
  auto heavy = [&](auto C, auto RL, int t0, int t1) {
    if (t1 > t0)
      hipLaunchKernelGGL((k_round_recon<decltype(C)::value, 1024, 128, 2, true, decltype(RL)::value>),
                         dim3(t1 - t0), dim3(kBlock), 0, h->stream, tl + t0, h->rowptr, h->col, h->v, c.F, c.ap, c.ap2,
                         c.an, h->target, c.err, cp, h->code[r1], h->pctl, r1, h->hubxy, h->hub_off, h->hrows, 1, Gb,
                         c.fm);
  };
  // the rows of the heavy tiles [nmega, m1) (4 rows each, longest first: every row of more
  // than 64 x kHeavyRL edges, and the few shorter ones sharing the last tile) as
  // k_heavy_multi blocks, many rows per chain wave
  // (multi_mid = 0: only the rows of [nmega, m0), longer than the register launch's; the rows
  // of [m0, m1) then stay in registers, one pass)
  auto tiles = [&](auto C) {
    if (multi) {
      auto hm = [&](auto L) {
        hipLaunchKernelGGL((k_heavy_multi<decltype(C)::value, decltype(L)::value>), dim3((n_multi + kMR - 1) / kMR),
                           dim3(kBlock), 0, h->stream, h->hrows + h->multi_geo[1][0], n_multi,
                           h->rowptr, h->v, c.F, c.ap2, c.an, h->target, c.err, h->code[r1], h->pctl, Gb, c.fm, Gb_old,
                           h->tr.hist[p]);
      };
      if (!lag_multi) hm(std::integral_constant<int, 0>{});
      else if (lagm == 1) hm(std::integral_constant<int, 1>{});
      else hm(std::integral_constant<int, 2>{});
      if (!h->multi_mid) heavy(C, std::integral_constant<int, kMidRL>{}, m0, m1);
    } else {
      heavy(C, std::integral_constant<int, kHeavyRL>{}, nmega, m0);
      heavy(C, std::integral_constant<int, kMidRL>{}, m0, m1);
    }
    heavy(C, std::integral_constant<int, kHeavyRL>{}, m1s, nh);
    if (niso)
      hipLaunchKernelGGL(k_isolated, dim3(grid_for(h->n - h->iso0_geo[1])), dim3(kBlock), 0, h->stream,
                         h->iso0_geo[1], h->n, h->v, c.an, h->target, c.err, h->code[r1], h->pctl, r1,
                         decltype(C)::value ? 1 : 0);
    if (nl)
      hipLaunchKernelGGL((k_round_recon<decltype(C)::value, 1024, 128, 1, true>), dim3(nl), dim3(kBlock), 0,
                         h->stream, tl + nh, h->rowptr, h->col, h->v, c.F, c.ap, c.ap2, c.an, h->target, c.err, cp,
                         h->code[r1], h->pctl, r1, nullptr, nullptr, nullptr, 0, Gb, c.fm);
  };
  if (chk) tiles(std::true_type{});
  else tiles(std::false_type{});
  HIP_TRY(hipGetLastError());
  if (hubs) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  if (h->dist) {  // multi-GPU: boundary rows sit in every row class, so a_r goes out after the round
    h->halo_a = c.an;
    if (int rc = fu__dist_round_hook(h, 2)) return rc;
  }
  if (lagm) {  // F[p] now holds f_{r-2} on the lagged rows; round r + 2 (or lag_finalize) writes f_r
    h->lagf[p] = 1;
    h->lag_round[p] = c.r;
    h->lag_nmulti[p] = lag_multi ? n_multi : 0;
  }
  return FU_OK;
}

// Kernel 4: heavy tiles (mega hubs, heavy rows) lead the tile list; with fork_heavy they run
// on the side stream beside the light tiles' launch (which keeps kernel 4's light-path
// register budget). Multi-GPU: the heavy tiles stay on the main stream, then the boundary
// light tiles, then the halo goes out beside the interior light tiles.
template <int TE, int TN>
int launch_k4_geo(fu_handle *h, RoundCtx &c) {
  const int r1 = (int)(c.r & 1);
  const void *cp = h->code[(c.r - 1) & 1];
  const int nh = h->nheavy_geo[h->geo], nl = h->ntiles_geo[h->geo] - nh;
  const int hub_sep = h->n_hub ? 1 : 0;  // k_hub_flows writes the hubs' flows after the chains
  const int nb = h->nbound_geo[h->geo];  // boundary light tiles (multi-GPU), then the interior
  const bool fork = nh > 0 && h->fork_heavy && !h->dist;
  hipStream_t hs = fork ? h->stream2 : h->stream;
  // with mega hubs, only their tiles go to the side stream (k_hub_stage -> chains ->
  // k_hub_flows), so the other heavy tiles need not wait for k_hub_stage
  const int nmh = fork && h->n_hub && h->split_hubs ? h->n_hub : nh;
  const int4 *tiles = h->tiles_geo[h->geo];
  if (fork) {
    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  }
  if (h->n_hub)
    hipLaunchKernelGGL(k_hub_stage, dim3(grid_for(h->hub_total)), dim3(kBlock), 0, hs, h->n_hub, h->hub_rows,
                       (long long)h->hub_total, h->col, c.F, c.ap, c.ap2, cp, h->pctl, r1, h->hubxy, c.fm, h->hub_blk);
  auto heavy = [&](auto C, hipStream_t st, int t0, int cnt) {
    if (cnt)
      hipLaunchKernelGGL((k_round_recon<decltype(C)::value, TE, TN, 2>), dim3(cnt), dim3(kBlock), 0, st,
                         tiles + t0, h->rowptr, h->col, h->v, c.F, c.ap, c.ap2, c.an, h->target, c.err, cp, h->code[r1],
                         h->pctl, r1, h->hubxy, h->hub_off, h->hrows, hub_sep, nullptr, c.fm);
  };
  // light tiles: rounds 1 and 2 (fm) read no flows (RF = false)
  auto light = [&](auto C, auto RF, int t0, int cnt) {
    if (cnt)
      hipLaunchKernelGGL((k_round_recon<decltype(C)::value, TE, TN, 1, false, kHeavyRL,
                                        decltype(RF)::value>),
                         dim3(cnt), dim3(kBlock), 0, h->stream, tiles + t0, h->rowptr, h->col, h->v, c.F, c.ap, c.ap2,
                         c.an, h->target, c.err, cp, h->code[r1], h->pctl, r1, nullptr, nullptr, nullptr, 0, nullptr,
                         c.fm, h->col16, h->cbase, h->c16 ? h->tnar_geo[h->geo] + t0 : nullptr);
  };
  auto light_rf = [&](auto C, int t0, int cnt) {
    if (c.fm) light(C, std::false_type{}, t0, cnt);
    else light(C, std::true_type{}, t0, cnt);
  };
  auto body = [&](auto C) -> int {
    heavy(C, hs, 0, nmh);             // mega hubs (or every heavy tile) on the side stream
    heavy(C, h->stream, nmh, nh - nmh);  // the other heavy tiles ahead of the light ones
    light_rf(C, nh, nb);
    if (h->dist) {  // boundary rows done: their estimates go out beside the interior tiles
      h->halo_a = c.an;
      if (int rc = fu__dist_round_hook(h, 2)) return rc;
    }
    light_rf(C, nh + nb, nl - nb);
    return FU_OK;
  };
  int rc;
  if (c.err) rc = body(std::true_type{});
  else rc = body(std::false_type{});
  if (rc) return rc;
  if (hub_sep)
    hipLaunchKernelGGL(k_hub_flows, dim3(grid_for(h->hub_total)), dim3(kBlock), 0, hs, h->n_hub, h->hub_rows,
                       (long long)h->hub_total, h->hubxy, c.an, c.F, nullptr, nullptr, c.fm, h->hub_blk);
  if (fork) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev_join, h->stream2));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  }
  return FU_OK;
}

int launch_k4(fu_handle *h, RoundCtx &c) {
  plan_alone(h, c);
  if (h->geo == 0) return launch_k4_geo<2048, 256>(h, c);
  if (h->geo == 2) return launch_k4_geo<1024, 256>(h, c);
  if (h->geo == 1) return launch_k4_geo<1024, 128>(h, c);
  return launch_k4_geo<512, 64>(h, c);
}

// The round body of rounds >= 1 for the handle's kernel.
int launch_body(fu_handle *h, RoundCtx &c) {
  if (h->kernel == 8) return launch_k8(h, c);
  if (h->kernel == 9) return launch_k9(h, c);
  return launch_k4(h, c);
}

// One round: state of round r-1 -> round r. err_slot: nullptr = no check.
int launch_round(fu_handle *h, unsigned long long *err_slot) {
  if (h->dist) {
    if (int rc = fu__dist_round_hook(h, 0)) return rc;
  }
  const int64_t r = h->rounds;
  RoundCtx c;
  c.r = r;
  c.fm = r == 1 ? 1 : r == 2 ? 2 : 0;  // rounds 1, 2: the old flows are computed, not read
  c.F = h->f[r & 1];
  c.ap = r > 0 ? h->a[(r - 1) % 3] : nullptr;
  c.ap2 = h->a[(r + 1) % 3];
  c.an = h->a[r % 3];
  c.err = err_slot;
  // a packing plan due from a_{r-1}: the stage launch of kernels 8 and 9 carries it (one more
  // block); every other path runs it first as a launch of its own
  // (held back during an autotune pass, so every candidate runs at the pass's width; any plan
  // is lossless, so a late one changes nothing but the table's width)
  c.plan = h->plan_pending && r > 0 && !h->tuning;
  if (!h->tuning) h->plan_pending = false;
  const bool plan_done = c.plan;
  int rc;
  // kernel 9's lag: another kernel reads F[r & 1] as f_{r-2}, so the lagged rows' flows of
  // round r - 2 are written first
  if (r > 0 && h->kernel != 9 && h->lagf[r & 1]) {
    if (int rc2 = lag_finalize(h, (int)(r & 1))) return rc2;
  }
  if (r == 0) rc = launch_round0(h, c);
  else rc = launch_body(h, c);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  if (plan_done && !h->pw_pending) {  // the autotuner watches the width (poll_pack_width)
    HIP_TRY(hipEventRecord(h->ev_pw, h->stream));
    h->pw_pending = true;
  }
  h->rounds++;
  // a packing plan from a_r is due: the next round runs it ahead of its round kernels (on
  // its stage launch where it has one) and encodes a_{r+1} with it; once the host has seen
  // the narrowest width (8), every 8th time only
  const int every = h->seen_width == 8 ? 8 * h->pack_every : h->pack_every;
  if (h->pack && !h->dist && h->n_psample > 0 && h->rounds % every == 0) h->plan_pending = true;
  return FU_OK;
}

}  // namespace
