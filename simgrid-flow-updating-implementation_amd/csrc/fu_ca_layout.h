// Collect-all engine, piece 6 of 7 (see fu_ca_pack.h): the host side of the device layouts.
// Uploads of what fu_plan.cpp builds (kernel 4's tiles and hubs, kernel 8's slices, kernel 9's
// buckets) and the lagged rows' flow write-back.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "fu_ca_handle.h"
#include "fu_ca_pregather.h"
#include "fu_ca_stage.h"

namespace {

// row-class and table constants shared with the host plans (fu_plan.h)
using FP::kGeoEdges;
using FP::kGeoNodes;

template <typename T>
int dmalloc(T **p, size_t count) {
  if (count == 0) count = 1;
  hipError_t e = hipMalloc((void **)p, sizeof(T) * count);
  if (e != hipSuccess) {
    *p = nullptr;
    return fail(FU_ERR_ALLOC, std::string("hipMalloc(") + std::to_string(sizeof(T) * count) + "): " + hipGetErrorString(e));
  }
  return FU_OK;
}

// The handle's graph as the host plans see it (fu_plan.h).
FP::Graph plan_graph(const fu_handle *h) {
  FP::Graph g;
  g.n = h->n;
  g.na = h->na;
  g.E = h->E;
  g.rowptr = h->h_rowptr.data();
  g.col = h->h_col.data();
  g.cbase = h->h_cbase.data();
  return g;
}

// host vector -> fresh device array (at least one element)
template <typename D, typename S>
int upload(D **dst, const std::vector<S> &src) {
  static_assert(sizeof(D) == sizeof(S), "upload: element layouts differ");
  if (*dst) hipFree(*dst);
  *dst = nullptr;
  if (int rc = dmalloc(dst, std::max<size_t>(1, src.size()))) return rc;
  if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), sizeof(S) * src.size(), hipMemcpyHostToDevice));
  return FU_OK;
}

// Kernel 4 tiles of geometry g (FP::build_tiles_geom: mega hubs, heavy rows, light tiles, the
// trailing degree-0 rows), uploaded; the heavy rows are appended to h_hrows.
int build_tiles_geom(fu_handle *h, int geo) {
  FP::TileOpts o;
  o.hub_threshold = h->hub_threshold;
  o.mega_hub = h->mega_hub;
  o.wave_heavy = h->wave_heavy;
  FP::Tiles t;
  std::string why;
  if (!FP::build_tiles_geom(plan_graph(h), kGeoEdges[geo], kGeoNodes[geo], o, h->h_hrows, t, &why))
    return fail(FU_ERR_STATE, why);
  if (int rc = upload(&h->tiles_geo[geo], t.all)) return rc;
  if (int rc = upload(&h->tnar_geo[geo], t.narrow)) return rc;
  h->ntiles_geo[geo] = (int)t.all.size();
  h->nheavy_geo[geo] = t.nheavy;
  h->nbound_geo[geo] = t.nbound;
  h->mid_geo[geo][0] = t.mid[0];
  h->mid_geo[geo][1] = t.mid[1];
  h->multi_geo[geo][0] = t.multi[0];
  h->multi_geo[geo][1] = t.multi[1];
  h->niso_geo[geo] = t.niso;
  h->iso0_geo[geo] = t.iso0;
  if (geo == 1) h->tiles1 = t;
  return FU_OK;
}

// Mega-hub side arrays (same rows, same order as the -3 tiles of build_tiles_geom).
int build_hubs(fu_handle *h) {
  for (void *p : {(void *)h->hub_rows, (void *)h->hub_off, (void *)h->hubxy, (void *)h->hub_blk})
    if (p) hipFree(p);
  h->hub_blk = nullptr;
  h->hub_rows = nullptr;
  h->hub_off = nullptr;
  h->hubxy = nullptr;
  FP::Hubs hb;
  FP::build_hubs(plan_graph(h), h->mega_hub, hb);
  h->n_hub = (int)hb.rows.size();
  h->hub_total = hb.total;
  if (hb.rows.empty()) return FU_OK;
  if (int rc = upload(&h->hub_rows, hb.rows)) return rc;
  if (int rc = upload(&h->hub_off, hb.off)) return rc;
  if (int rc = dmalloc(&h->hubxy, (size_t)hb.total)) return rc;
  return upload(&h->hub_blk, hb.blk);
}

// ---- kernel 8 preparation -------------------------------------------------------------

// Light tiles (kStageTE x kStageTN) and the rows above the tile limit (kernel 8).
int ensure_light(fu_handle *h) {
  if (h->st_tiles) return FU_OK;
  FP::StageLight sl;
  FP::build_stage_light(plan_graph(h), h->hub_threshold, sl);
  h->st_nbound = sl.nbound;
  h->h_light = sl.light;
  if (int rc = upload(&h->st_tiles, sl.light)) return rc;
  if (int rc = upload(&h->st_heavy, sl.heavy)) return rc;
  h->st_ntiles = (int)sl.light.size();
  h->st_nheavy = (int)sl.heavy.size();
  return FU_OK;
}

// The staged-estimate buffer G and the four slice layouts (element bytes 1, 2, 4, 8; slice =
// kStageLds / bytes nodes; FP::build_stage_layouts). A tile's edges of one slice are one
// contiguous run of G: per edge the round kernel reads u16 {position, run} and per tile the
// run offsets D (G index = m + D[run], m = index in slice order).
int ensure_stage(fu_handle *h) {
  if (h->st_ready) return FU_OK;
  if (!h->st_why.empty()) return fail(FU_ERR_GRAPH, h->st_why);
  if (int rc = ensure_light(h)) return rc;
  FP::StageLayout L[4];
  std::string why;
  if (!FP::build_stage_layouts(plan_graph(h), h->h_light, h->n_cu, L, &why)) {
    h->st_why = why;
    return fail(FU_ERR_GRAPH, why);
  }
  int64_t gmax = 16;
  for (int li = 0; li < 4; ++li) {
    auto &D = h->st[li];
    for (void *p : {(void *)D.brange, (void *)D.colS, (void *)D.sidx16, (void *)D.dtab})
      if (p) hipFree(p);
    D = fu_handle::StageLayout{};
    if (!L[li].P) continue;
    if (int rc = upload(&D.brange, L[li].brange)) return rc;
    if (int rc = upload(&D.colS, L[li].colS)) return rc;
    if (int rc = upload(&D.sidx16, L[li].sidx16)) return rc;
    if (int rc = upload(&D.dtab, L[li].dtab)) return rc;
    D.P = L[li].P;
    D.Q = L[li].Q;
    D.SN = L[li].SN;
    D.NB = L[li].NB;
    gmax = std::max<int64_t>(gmax, L[li].total);
  }
  if (int rc = dmalloc(reinterpret_cast<unsigned long long **>(&h->stG), (size_t)gmax)) return rc;
  HIP_TRY(hipMemset(h->stG, 0, sizeof(unsigned long long) * (size_t)gmax));
  h->st_ready = true;
  return FU_OK;
}

// Layout per table width (device-side choice): the narrowest built layout whose elements
// hold the width's (the table sits in LDS), else the widest built one (the stage launch
// then reads the table from global memory); a forced layout (tests) for every width.
StageArgs stage_args(fu_handle *h, unsigned *grid) {
  StageArgs sa{};
  unsigned g = 1;
  for (int li = 0; li < 4; ++li) {
    const auto &L = h->st[li];
    sa.P[li] = L.P ? L.P : 1;
    sa.Q[li] = L.P ? L.Q : 0;
    sa.SN[li] = L.SN;
    sa.NB[li] = L.NB;
    sa.brange[li] = L.brange;
    sa.colS[li] = L.colS;
    sa.sidx16[li] = L.sidx16;
    sa.dtab[li] = L.dtab;
    if (L.P) g = std::max<unsigned>(g, (unsigned)L.NB);
  }
  for (int want = 0; want < 4; ++want) {
    int pick = -1;
    if (h->st_force >= 0 && h->st[h->st_force].P) pick = h->st_force;
    for (int li = want; li < 4 && pick < 0; ++li)
      if (h->st[li].P) pick = li;
    for (int li = want; li >= 0 && pick < 0; --li)
      if (h->st[li].P) pick = li;
    sa.sel[want] = pick < 0 ? 0 : pick;
  }
  if (grid) *grid = g;
  return sa;
}

// Kernel 9 preparation (see k_transpose): slices of 16K nodes, buckets of kTrBE edges. G_A:
// slice-major, within a slice in edge order, each slice's region starting at a multiple of
// 16 (the stage launch stores 16 bytes per lane); offT[b * P + s] = where bucket b's run of
// slice s starts (offT[B * P + s]: the end of slice s's elements); stage blocks cut each
// slice's region into Q pieces.
void free_transpose(fu_handle *h) {
  auto &T = h->tr;
  for (void *p : {(void *)T.brange, (void *)T.colS, (void *)T.pos16, (void *)T.offT, (void *)T.GA,
                  (void *)T.GBr[0], (void *)T.hist[0], (void *)T.hist[1]})
    if (p) hipFree(p);
  if (T.GBr[1] != T.GBr[0]) hipFree(T.GBr[1]);
  if (T.GBr[2] != T.GBr[0]) hipFree(T.GBr[2]);
  T = fu_handle::TransLayout{};
  h->tr_ready = false;
}

int ensure_transpose(fu_handle *h) {
  if (h->tr_ready) return FU_OK;
  if (!h->tr_why.empty()) return fail(FU_ERR_GRAPH, h->tr_why);
  FP::TransPlan tp;
  std::string why;
  const int32_t *mrows = h->h_hrows.empty() ? nullptr : h->h_hrows.data() + h->multi_geo[1][0];
  if (!FP::build_transpose(plan_graph(h), h->mega_hub, h->n_cu, mrows, h->multi_geo[1][1], tp, &why)) {
    h->tr_why = why;
    return fail(FU_ERR_GRAPH, why);
  }
  auto &T = h->tr;
  if (int rc = upload(&T.brange, tp.brange)) return rc;
  if (int rc = upload(&T.colS, tp.colS)) return rc;
  if (int rc = upload(&T.pos16, tp.pos)) return rc;
  if (int rc = upload(&T.offT, tp.offT)) return rc;
  if (int rc = dmalloc(&T.GA, (size_t)tp.total)) return rc;
  // G_B: a ring of three with lag (round r reads G_B of round r - 2 for the lagged rows)
  for (int k = 0; k < 3; ++k) {
    if (k && !h->lag) {
      T.GBr[k] = T.GBr[0];
      continue;
    }
    if (int rc = dmalloc(&T.GBr[k], (size_t)h->E)) return rc;
  }
  for (int p = 0; p < 2; ++p)
    if (int rc = dmalloc(&T.hist[p], (size_t)(h->multi_geo[1][1] + 1))) return rc;
  T.P = tp.P;
  T.Q = tp.Q;
  T.NB = tp.NB;
  T.B = tp.B;
  T.Bh = tp.Bh;
  T.Bm = tp.Bm;
  h->tr_ready = true;
  return FU_OK;
}

// Kernel 9 "lag": write the flows parity p's last round r' left unwritten on its lagged rows
// (k_lag_final: F[p] holds f_{r'-2}; G_B of r' is GBr[r' % 3], a_{r'} is A[r' % 3]). Valid
// while r' is one of the last two rounds (the A ring holds a_{r'}; no kernel-9 round has
// reused r''s G_B slot), which holds at every call site: before a round of another kernel,
// fu_get_flows, a tile rebuild, the option's change.
int lag_finalize(fu_handle *h, int p) {
  if (!h->lagf[p]) return FU_OK;
  const int64_t rr = h->lag_round[p];
  if (h->rounds - rr < 1 || h->rounds - rr > 2)  // A[rr % 3] or G_B[rr % 3] already reused
    return fail(FU_ERR_STATE, "lag_finalize: lagged round " + std::to_string(rr) + " is not one of the last two (" +
                                  std::to_string(h->rounds) + " rounds done)");
  const double *Gb = h->tr.GBr[rr % 3];
  const double *a = h->a[rr % 3];
  if (h->lag_nmulti[p])
    hipLaunchKernelGGL(k_lag_final, dim3(h->lag_nmulti[p]), dim3(kBlock), 0, h->stream, h->hrows + h->multi_geo[1][0],
                       h->rowptr, h->f[p], Gb, h->tr.hist[p], a);
  HIP_TRY(hipGetLastError());
  h->lagf[p] = 0;
  return FU_OK;
}
int lag_finalize_all(fu_handle *h) {
  for (int p = 0; p < 2; ++p)
    if (int rc = lag_finalize(h, p)) return rc;
  return FU_OK;
}

int build_tiles(fu_handle *h) {
  if (int rc = lag_finalize_all(h)) return rc;  // the lagged rows' flows, before their lists change
  free_transpose(h);  // its hub exclusion follows the tiles
  h->h_hrows.clear();
  for (int g = 0; g < 4; ++g)
    if (int rc = build_tiles_geom(h, g)) return rc;
  if (h->hrows) hipFree(h->hrows);
  h->hrows = nullptr;
  if (int rc = dmalloc(&h->hrows, std::max<size_t>(1, h->h_hrows.size()))) return rc;
  if (!h->h_hrows.empty())
    HIP_TRY(hipMemcpy(h->hrows, h->h_hrows.data(), sizeof(int32_t) * h->h_hrows.size(), hipMemcpyHostToDevice));
  return build_hubs(h);
}

}  // namespace
