// trx_api.hip -- C ABI of include/transit_hip.h on top of the gfx950 kernels.
//
// Host responsibilities (all layer- or geometry-only, O(N) or O(N^2) scalars):
//   * line-list preparation once per handle: wavenumbers, range flags, the
//     greedy co-adding groups (extinction.c:449-462) and their fine-grid
//     indices (:445-447) -- exact reference arithmetic, sequential by nature;
//   * per-run layer prologue: broadening widths, nearest table indices,
//     strength prefactors (extinction.c:364-395, 464, 473);
//   * Simpson weights of the ray geometry (numerical.c:390-425);
//   * the table-only halves of the CIA splines (crosssec.c:272-428), once per handle;
//   * the plan of a run: layers per step, streams, events, the exchanges of a sharded job.
// Everything per (line x layer), per (group x layer x bin) and per
// (wavenumber x layer) runs in the kernels of trx_kernels.hip.h.
//
// One translation unit in five files: the handle and its helpers (trx_handle.hip.h), here the handle's creation and the run
// path, the launches of a sweep step (trx_api_sweep.hip.h) between the two, then the run products (trx_api_products.hip.h)
// and the batch layer (trx_api_batch.hip.h), included at the end.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "transit_hip.h"
#include "trx_kernels.hip.h"
#include "trx_walk.hip.h"
#include "trx_rows.hip.h"
#include "trx_tail.hip.h"
#include "trx_lanes.hip.h"
#include "trx_bands.hip.h"
#include "trx_pixels.hip.h"
#include "trx_moments.hip.h"
#include "trx_trail.hip.h"
#include "trx_vmap.hip.h"
#include "trx_cellmap.hip.h"
#include "trx_expmap.hip.h"
#include "trx_filter.hip.h"
#include "trx_wfilter.hip.h"
#include "trx_sysrem.hip.h"
#include "trx_pca.hip.h"
#include "trx_regress.hip.h"
#include "trx_scatter.hip.h"
#include "trx_normalise.hip.h"
#include "trx_highpass.hip.h"
#include "trx_broaden.hip.h"
#include "trx_contrib.hip.h"
#include "../trx_groups.h"
#include "../trx_plan.h"
#include "../trx_sweep.h"
#include "../trx_schedule.h"
#include "../trx_table.h"
#include "../trx_broaden.h"
#include "../trx_vmap.h"
#include "../trx_products.h"
#include "../trx_exposures.h"
#include "../trx_expmap.h"
#include "../trx_wfilter.h"
#include "../trx_sysrem.h"
#include "../trx_pca.h"
#include "../trx_regress.h"
#include "../trx_scatter.h"
#include "../trx_normalise.h"
#include "../trx_launch.h"
#include "../trx_hpdata.h"

using namespace trx;

#include "trx_handle.hip.h"

namespace {

// The one place the handle's switches are read (struct Switches); trx_create calls it before any stage.
void read_switches(Switches &w)
{
  auto set = [](const char *name) { return std::getenv(name) != nullptr; };
  auto num = [](const char *name, long long otherwise) { const char *e = std::getenv(name); return e ? std::atoll(e) : otherwise; };
  auto clamped = [&](const char *name, int lo, int hi, int otherwise) { return (int)std::max<long long>(lo, std::min<long long>(hi, num(name, otherwise))); };
  w.no_row_copy = set("TRX_NO_ROW_COPY");
  w.no_rows32 = set("TRX_NO_ROWS32");
  w.row_staging = !set("TRX_NO_ROW_STAGING");
  w.row_m8_from = num("TRX_ROWS_M8_FROM", w.row_m8_from);
  w.packed_walk = !set("TRX_NO_PACKED_WALK");
  w.packed_max_layers = clamped("TRX_PACKED_MAX_LAYERS", 1, 32, w.packed_max_layers);
  w.xcd_map = (int)num("TRX_XCD_MAP", w.xcd_map);
  w.no_binrec = set("TRX_NO_BINREC");
  const long long lanes = num("TRX_LANES_WALK", 1);
  w.lanes_walk = lanes != 0; w.lanes_force = lanes == 2;
  w.lanes_parts_most = clamped("TRX_LANES_PARTS", 2, 4, w.lanes_parts_most);
  w.ray_tail = num("TRX_RAY_TAIL", 1) != 0;
  w.cia_sums = num("TRX_CIA_SUMS", 1) != 0;
  w.cia_segments = num("TRX_CIA_SEGMENTS", 1) != 0;
  w.cia_window = num("TRX_CIA_WINDOW", 1) != 0;
  w.two_queues = num("TRX_TWO_QUEUES", 1) != 0;
  w.tail_direct = num("TRX_TAIL_DIRECT", 1) != 0;
  w.range_reach = num("TRX_RANGE_REACH", 1) != 0;
  w.shard_frames = num("TRX_SHARD_FRAMES", 1) != 0;
}

// ---- the Voigt table: plan and layouts in ../trx_table.h; here the uploads and the kernels ----
struct TableBuild { TablePlan P; DevBuf d_jobs; };      // (d_jobs: read by every table kernel, alive until build_table's last synchronisation)

// fn(first job, jobs) over the jobs in batches of 32768 (gridDim.y)
template <class F>
void for_job_batches(const std::vector<ProfileJob> &jobs, F fn)
{
  for (size_t j0 = 0; j0 < jobs.size(); j0 += 32768) fn(j0, (int)std::min<size_t>(32768, jobs.size() - j0));
}

// the plan into the handle; the thresholds of the two width grids
int plan_into_handle(trx_handle *h, const trx_static *s, TableBuild &B)
{
  const char *text = "";
  const TablePlanError pe = plan_table(*s, B.P, &text);
  if (pe != kTablePlanOk) return fail(h, pe == kTablePlanArg ? TRX_E_ARG : TRX_E_UNSUPPORTED, text);
  h->adop = B.P.adop; h->alor = B.P.alor; h->psize = B.P.psize; h->poff = B.P.poff; h->tab_n = B.P.tab_n;
  h->psizeT = std::move(B.P.psizeT); h->psize_mono = B.P.psize_mono;
  // the steps of the nearest-index function (index_steps): the Doppler grid's go to the kernels (index_from) and must
  // exist; the Lorentz grid's serve the host's prologue (prep_layers), and a grid that fails the check keeps nearest_index
  if (!index_steps(h->adop.data(), s->ndop, h->dopthr)) return fail(h, TRX_E_ARG, "Doppler-width grid is not strictly increasing");
  if (!index_steps(h->alor.data(), s->nlor, h->lorthr)) h->lorthr.clear();
  return TRX_OK;
}

// constants, the job list, the zeroed table and the entry arrays, in the order they have always gone up
int upload_table_inputs(trx_handle *h, const trx_static *s, TableBuild &B)
{
  int rc;
  // series coefficients 1/(n!(2n+1)), voigt.c:45-108
  double coef[64]; long double fact = 1.0L;
  for (int n = 0; n < 64; n++) { if (n > 0) fact *= (long double)n; coef[n] = (double)(1.0L / (fact * (long double)(2 * n + 1))); }
  HIPCHK(h, hipMemcpyToSymbolAsync(HIP_SYMBOL(c_voigt_coef), coef, sizeof(coef), 0, hipMemcpyHostToDevice, h->stream));
  if ((rc = upload(h, B.d_jobs, B.P.jobs))) return rc;
  const size_t tab_alloc = table_alloc_floats(h->tab_n, s->osamp);
  if ((rc = ensure(h, h->d_tab, sizeof(float) * tab_alloc))) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_tab.p, 0, sizeof(float) * tab_alloc, h->stream));
  h->tab = h->d_tab.as<float>() + kTabPad;
  if ((rc = upload(h, h->d_psize, h->psize)) || (rc = upload(h, h->d_poff, h->poff)) || (rc = upload(h, h->d_adop, h->adop)) ||
      (rc = upload(h, h->d_dopthr, h->dopthr))) return rc;
  std::vector<double> e2(64);                       // 2^(j/64) for exp_neg (kernels)
  for (int j = 0; j < 64; j++) e2[j] = (double)exp2l((long double)j / 64.0L);
  return upload(h, h->d_e2tab, e2);                 // (pageable: the copy has left e2 when the call returns)
}

void table_kernels(trx_handle *h, const TableBuild &B)
{
  const int m_limit = 64;
  const std::vector<ProfileJob> &jobs = B.P.jobs;
  for_job_batches(jobs, [&](size_t j0, int nj) {
    int maxnv = 0; bool any_wave = false;
    for (int j = 0; j < nj; j++) { maxnv = std::max(maxnv, jobs[j0 + j].nv); any_wave |= (jobs[j0 + j].regime == 2 && jobs[j0 + j].m > m_limit); }
    const int gx = std::max(1, std::min(64, (maxnv + 255) / 256));
    hipLaunchKernelGGL(k_voigt_bins, dim3(gx, nj), dim3(256), 0, h->stream, B.d_jobs.as<ProfileJob>() + j0, h->tab, m_limit);
    if (any_wave)
      hipLaunchKernelGGL(k_voigt_bins_wave, dim3(std::max(1, std::min(256, maxnv)), nj), dim3(64), 0, h->stream,
                         B.d_jobs.as<ProfileJob>() + j0, h->tab, m_limit);
  });
}

// phase-major copy for the wide-profile kernel (osamp == 1: the table itself has that layout)
int phase_major_copy(trx_handle *h, const trx_static *s, const TableBuild &B)
{
  if (s->osamp == 1) { h->tabT = h->tab; h->poffT = h->d_poff.as<long long>(); return TRX_OK; }
  const PhaseMajorLayout T = phase_major_layout(B.P, s->osamp);
  const size_t bytes = sizeof(float) * ((size_t)T.totT + 2 * kTabPad);
  DevBuf d_joffT;
  int rc;
  if ((rc = upload(h, d_joffT, T.joffT)) || (rc = upload(h, h->d_poffT, T.poffT)) || (rc = ensure(h, h->d_tabT, bytes))) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_tabT.p, 0, bytes, h->stream));
  for_job_batches(B.P.jobs, [&](size_t j0, int nj) {
    hipLaunchKernelGGL(k_table_phase_major, dim3(32, nj), dim3(256), 0, h->stream, B.d_jobs.as<ProfileJob>() + j0,
                       d_joffT.as<long long>() + j0, h->tab, h->d_tabT.as<float>() + kTabPad, s->osamp, 0);
  });
  HIPCHK(h, hipStreamSynchronize(h->stream));      // d_joffT and T die here
  h->tabT = h->d_tabT.as<float>() + kTabPad; h->poffT = h->d_poffT.as<long long>();
  return TRX_OK;
}

// compact 32-byte rows, gathered from the walk's rows (d_joffW: where those are)
int compact_rows(trx_handle *h, const trx_static *s, const TableBuild &B, const DevBuf &d_joffW)
{
  const CompactLayout C = compact_layout(B.P, s->osamp);
  if (!compact_rows_fit(C.nq, C.tot32, s->osamp) || h->sw.no_rows32) return TRX_OK;
  DevBuf d_joff32;
  int rc;
  // (and kLanesRowSlack floats behind: the last lane of a layer holding fewer bins than the others reads on past the row)
  if ((rc = upload(h, d_joff32, C.joff32)) || (rc = upload(h, h->d_wp32, C.c32)) ||
      (rc = ensure(h, h->d_tabW32, sizeof(float) * ((size_t)C.tot32 + kLanesRowSlack)))) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_tabW32.as<float>() + C.tot32, 0, sizeof(float) * kLanesRowSlack, h->stream));
  for_job_batches(B.P.jobs, [&](size_t j0, int nj) {
    hipLaunchKernelGGL(k_table_rows32, dim3(16, nj), dim3(256), 0, h->stream, B.d_jobs.as<ProfileJob>() + j0, d_joffW.as<long long>() + j0,
                       d_joff32.as<long long>() + j0, h->d_tabW.as<float>() + kTabPad, h->d_tabW32.as<float>(), s->osamp, 8 * C.nq);
  });
  h->slab32 = (unsigned)(32 * C.nq);
  HIPCHK(h, hipStreamSynchronize(h->stream));      // d_joff32 and C die here
  h->tabW32 = h->d_tabW32.as<float>();
  return TRX_OK;
}

// the walk's rows and their descriptors, then the compact rows made from them
int walk_rows(trx_handle *h, const trx_static *s, const TableBuild &B)
{
  const WalkLayout W = walk_layout(B.P, s->osamp);
  h->tabw_ok = walk_rows_fit(W.totW) && !h->sw.no_row_copy;
  if (!h->tabw_ok) return TRX_OK;
  const size_t bytes = sizeof(float) * ((size_t)W.totW + 2 * kTabPad);
  DevBuf d_joffW;
  int rc;
  if ((rc = upload(h, d_joffW, W.joffW)) || (rc = upload(h, h->d_walkprof, W.prof)) || (rc = ensure(h, h->d_tabW, bytes))) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_tabW.p, 0, bytes, h->stream));
  for_job_batches(B.P.jobs, [&](size_t j0, int nj) {
    hipLaunchKernelGGL(k_table_phase_major, dim3(32, nj), dim3(256), 0, h->stream, B.d_jobs.as<ProfileJob>() + j0,
                       d_joffW.as<long long>() + j0, h->tab, h->d_tabW.as<float>() + kTabPad, s->osamp, 1);
  });
  if ((rc = compact_rows(h, s, B, d_joffW))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));      // d_joffW and W die here
  h->tabW = h->d_tabW.as<float>() + kTabPad;
  return TRX_OK;
}

int build_table(trx_handle *h, const trx_static *s)
{
  TableBuild B;
  int rc;
  if ((rc = plan_into_handle(h, s, B)) || (rc = upload_table_inputs(h, s, B))) return rc;
  hipEvent_t e0, e1;                               // ms_create_table: the table kernels and the three copies
  HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
  HIPCHK(h, hipEventRecord(e0, h->stream));
  table_kernels(h, B);
  if ((rc = phase_major_copy(h, s, B)) || (rc = walk_rows(h, s, B))) return rc;
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(e1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));      // B.d_jobs dies at return
  float ms = 0; HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  h->stats.ms_create_table = ms;
  h->stats.table_floats = h->tab_n;
  return TRX_OK;
}

// ---- line list preparation (the threaded host loops: ../trx_groups.h) -------
// what the stages of prepare_lines hand to one another (host arrays: they die with it, after the uploads' synchronisation)
struct LinePrep {
  int64_t n = 0; int nth = 1;
  double wn0 = 0, odwn = 0, own_last = 0;          // the fine grid: first point, step, last point
  StageTimer T;
  HostBuf<double> wavn; HostBuf<uint8_t> inr;      // [n] wavenumber, in-range flag
  LineGroups LG;
  std::vector<int32_t> gblock;                     // [niso + 1] first group of every isotope block
  HostBuf<int32_t> cntge, cntsub, lgroup, gimod, gidiv;
};

// wavenumbers and range flags
int line_wavenumbers(trx_handle *h, const trx_static *s, LinePrep &Q)
{
  Q.wavn.alloc((size_t)Q.n); Q.inr.alloc((size_t)Q.n);
  std::atomic<int64_t> inrange{0};
  const int bad = parallel_flags(Q.n, Q.nth, [&](int64_t i0, int64_t i1) {
    int64_t c = 0; int b = 0;
    for (int64_t i = i0; i < i1; i++) {
      if (s->isoid[i] < 0 || s->isoid[i] >= s->niso) { b = 1; continue; }
      Q.wavn[i] = 1.0 / (s->wl_um[i] * kTliWfct);
      Q.inr[i] = !(Q.wavn[i] < Q.wn0 || Q.wavn[i] > Q.own_last);             // extinction.c:410
      c += Q.inr[i];
    }
    inrange += c;
    return b;
  });
  if (bad) return fail(h, TRX_E_ARG, "isotope id out of range");
  h->ninrange += inrange;
  Q.T.lap("wavn + range flags");
  return TRX_OK;
}

// TLI order: isotope blocks in ascending id, wavelength ascending inside a
// block (pylineread.py:369-383); the gather kernel relies on it.
int check_line_order(trx_handle *h, const trx_static *s, LinePrep &Q)
{
  const int any = parallel_flags(Q.n, Q.nth, [&](int64_t i0, int64_t i1) {
    int b = 0;
    for (int64_t i = std::max<int64_t>(i0, 1); i < i1; i++) {
      if (s->isoid[i] < s->isoid[i-1]) b |= 1;
      else if (s->isoid[i] == s->isoid[i-1] && Q.wavn[i] > Q.wavn[i-1]) b |= 2;
    }
    return b;
  });
  if (any & 1) return fail(h, TRX_E_ORDER, "isotope blocks are not in ascending order");
  if (any & 2) return fail(h, TRX_E_ORDER, "wavelengths are not ascending inside an isotope block");
  Q.T.lap("order check");
  return TRX_OK;
}

// co-added groups (extinction.c:445-462), grouped in pieces side by side (trx_groups.h), and their isotope blocks
int group_and_check(trx_handle *h, const trx_static *s, LinePrep &Q)
{
  LineGroups &G = Q.LG;
  group_lines(Q.n, s->isoid, Q.wavn.data(), Q.inr.data(), s->niso, Q.wn0, Q.odwn, Q.nth, G);
  h->iso_wmin = G.iso_wmin; h->iso_wmax = G.iso_wmax; h->nadd += G.nadd;
  Q.T.lap("grouping");
  h->nlines = Q.n; h->ngroups = (int64_t)G.first.size();
  // (groups are in line order: the first group of every isotope by bisection)
  Q.gblock.assign(s->niso + 1, 0);
  for (int b = 0; b <= s->niso; b++) Q.gblock[b] = (int32_t)(std::lower_bound(G.iso.data(), G.iso.data() + G.iso.size(), (int16_t)b) - G.iso.data());
  const int bad = parallel_flags((int64_t)G.iown.size(), Q.nth, [&](int64_t g0, int64_t g1) {
    int b = 0;
    for (int64_t g = std::max<int64_t>(g0, 1); g < g1; g++) if (G.iso[g] == G.iso[g-1] && G.iown[g] > G.iown[g-1]) b = 1;
    return b;
  });
  if (bad) return fail(h, TRX_E_ORDER, "fine-grid indices are not descending inside an isotope block");
  return TRX_OK;
}

// the coarse-bin index over the blocks' groups (cntge), and the same counts at F sub-buckets per
// coarse cell (cntsub, key iown*F/osamp): k_accumulate sizes its windows with them, so that it does
// not stream whole cells of groups that lie between the reach of two bins.  F = 1 (cntge itself)
// when the fine grid is no finer or the table would be large.
void count_tables(trx_handle *h, const trx_static *s, LinePrep &Q)
{
  const int32_t *giown = Q.LG.iown.data();
  const long long osamp = s->osamp;
  Q.cntge.alloc((size_t)s->niso * (s->nwn + 1));
  for (int b = 0; b < s->niso; b++) {
    const long long kmaxc = s->nwn - 1;
    count_ge(giown, Q.gblock[b], Q.gblock[b + 1], s->nwn, [=](int32_t io) { return std::min<long long>(io / osamp, kmaxc); },
             &Q.cntge[(size_t)b * (s->nwn + 1)], Q.nth);
  }
  Q.T.lap("cnt_ge");
  int F = (int)std::min<long long>(16, s->osamp);
  while (F > 1 && (size_t)s->niso * (size_t)F * (size_t)s->nwn * 4 > ((size_t)64 << 20)) F /= 2;
  h->sub_f = F;
  if (F == 1) return;
  const size_t stride = (size_t)F * s->nwn + 1;
  Q.cntsub.alloc((size_t)s->niso * stride);
  for (int b = 0; b < s->niso; b++) {
    const long long kmaxs = (long long)stride - 2, FF = F;
    count_ge(giown, Q.gblock[b], Q.gblock[b + 1], (long long)stride - 1,
             [=](int32_t io) { return std::min<long long>((long long)io * FF / osamp, kmaxs); }, &Q.cntsub[(size_t)b * stride], Q.nth);
  }
}

// a line's group (anchors only), a group's fine-grid index as cell and phase
void group_indices(const trx_static *s, LinePrep &Q)
{
  const LineGroups &G = Q.LG;
  Q.lgroup.alloc((size_t)Q.n);
  parallel_parts(Q.n, Q.nth, [&](int, int64_t i0, int64_t i1) { std::fill(Q.lgroup.begin() + i0, Q.lgroup.begin() + i1, -1); });
  Q.gimod.alloc(G.iown.size()); Q.gidiv.alloc(G.iown.size());
  parallel_parts((int64_t)G.iown.size(), Q.nth, [&](int, int64_t g0, int64_t g1) {
    for (int64_t g = g0; g < g1; g++) { Q.lgroup[(size_t)G.first[g]] = (int32_t)g; Q.gimod[g] = G.iown[g] % s->osamp; Q.gidiv[g] = G.iown[g] / s->osamp; }
  });
  Q.T.lap("cnt_sub, lgroup, gimod");
}

// the walk's view of the list (k_line_walk): line ranges of ngw consecutive groups per isotope block
// (32-bit byte offsets into the widened table: 8*tab_n + 64*osamp must stay below 2^32)
int walk_ranges(trx_handle *h, const trx_static *s, const LinePrep &Q)
{
  h->walk_ok = s->osamp < (1 << 21) && h->tab_n < ((int64_t)1 << 28) && !Q.LG.first.empty();
  if (!h->walk_ok) return TRX_OK;
  const int ngw = h->ngw = groups_per_range((int64_t)Q.LG.first.size());
  h->h_wbase.assign(s->niso + 1, 0);
  for (int b = 0; b < s->niso; b++) h->h_wbase[b + 1] = h->h_wbase[b] + (Q.gblock[b + 1] - Q.gblock[b] + ngw - 1) / ngw;
  h->nwaves = h->h_wbase[s->niso];
  return upload(h, h->d_wbase, h->h_wbase);
}

// everything else goes up; the host keeps what the per-run prologue reads
int upload_lines(trx_handle *h, LinePrep &Q)
{
  LineGroups &G = Q.LG;
  int rc;
  if ((rc = upload(h, h->d_wavn, Q.wavn)) || (rc = upload(h, h->d_inr, Q.inr)) || (rc = upload(h, h->d_lgroup, Q.lgroup)) ||
      (rc = upload(h, h->d_gfirst, G.first)) || (rc = upload(h, h->d_gcount, G.count)) || (rc = upload(h, h->d_giown, G.iown)) ||
      (rc = upload(h, h->d_giso, G.iso)) || (rc = upload(h, h->d_gwavn, G.wavn)) || (rc = upload(h, h->d_gimod, Q.gimod)) ||
      (rc = upload(h, h->d_gidiv, Q.gidiv)) || (rc = upload(h, h->d_gblock, Q.gblock)) || (rc = upload(h, h->d_cntge, Q.cntge)) ||
      (rc = upload(h, h->d_cntsub, Q.cntsub)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));    // the host arrays may go now
  Q.T.lap("uploads + sync");
  h->h_gwavn = std::move(G.wavn); h->h_gblock = Q.gblock; h->h_cntge = std::move(Q.cntge); h->h_gfirst = std::move(G.first); h->h_gcount = std::move(G.count);
  Q.T.lap("host copies");
  LinesDev &L = h->L;
  L.nlines = Q.n; L.wavn = h->d_wavn.as<double>(); L.elow = h->d_elow.as<double>(); L.gf = h->d_gf.as<double>();
  L.iso = h->d_iso.as<int16_t>(); L.inrange = h->d_inr.as<uint8_t>(); L.lgroup = h->d_lgroup.as<int32_t>();
  L.ngroups = h->ngroups; L.gfirst = h->d_gfirst.as<int32_t>(); L.gcount = h->d_gcount.as<int32_t>();
  L.giown = h->d_giown.as<int32_t>(); L.giso = h->d_giso.as<int16_t>(); L.gwavn = h->d_gwavn.as<double>();
  L.gblock = h->d_gblock.as<int32_t>(); L.cnt_ge = h->d_cntge.as<int32_t>();
  return TRX_OK;
}

// the walk's records (trx_walk.hip.h): one 32-byte record per line, built where the arrays already are
int walk_records(trx_handle *h, const trx_static *s, const LinePrep &Q)
{
  const int64_t n = Q.n; const LinesDev &L = h->L;
  int rc;
  if ((rc = ensure(h, h->d_walk, sizeof(WalkLine) * ((size_t)n + 1))) || (rc = ensure(h, h->d_linebase, sizeof(double) * ((size_t)n + 1)))) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_linebase.p, 0, sizeof(double) * ((size_t)n + 1), h->stream));
  h->max_gcount = parallel_minmax<int>((int64_t)h->h_gcount.size(), Q.nth, 0, 0, [&](int64_t g, bool &) { return (int)h->h_gcount[(size_t)g]; }).hi;
  hipLaunchKernelGGL(k_walk_records, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, h->stream, (long long)n, L.wavn, L.elow, L.gf,
                     L.lgroup, L.giown, s->osamp, h->d_walk.as<WalkLine>());
  hipLaunchKernelGGL(k_walk_marks, dim3((unsigned)((h->nwaves + 63) / 64)), dim3(64), 0, h->stream, h->nwaves, h->ngw, s->niso,
                     h->d_wbase.as<int32_t>(), L.gblock, L.gfirst, L.gcount, h->d_walk.as<WalkLine>(), h->d_linebase.as<double>());
  if ((rc = ensure(h, h->d_rinfo, sizeof(RangeInfo) * (size_t)std::max(h->nwaves, 1)))) return rc;
  hipLaunchKernelGGL(k_range_info, dim3((unsigned)((h->nwaves + 255) / 256)), dim3(256), 0, h->stream, h->nwaves, h->ngw, s->niso,
                     h->d_wbase.as<int32_t>(), L.gblock, L.gfirst, L.gcount, h->d_walk.as<WalkLine>(), s->osamp, h->d_rinfo.as<RangeInfo>());
  return TRX_OK;
}

// candidates for the layer maximum: lines no other line of their isotope dominates
// (trx_walk.hip.h).  Falls back to "every line" when the filter would not pay.
int line_candidates(trx_handle *h, const trx_static *s, const LinePrep &Q)
{
  const int64_t n = Q.n; const LinesDev &L = h->L;
  h->ncand = -1;
  if (!(h->ninrange > 4096 && s->niso > 0)) return TRX_OK;
  const MinMax<double> e = parallel_minmax<double>(n, Q.nth, HUGE_VAL, -HUGE_VAL, [&](int64_t i, bool &use) { use = Q.inr[i]; return s->elow[i]; });
  CandGeom Gm{};
  Gm.e_min = e.lo; Gm.e_scale = e.hi > e.lo ? kCandGrid / (e.hi - e.lo) : 0.0;
  Gm.w_min = Q.wn0;  Gm.w_scale = Q.own_last > Q.wn0 ? kCandGrid / (Q.own_last - Q.wn0) : 0.0;
  const int cap = (int)std::max<int64_t>(4096, n / 8);
  DevBuf d_M, d_n;
  const size_t mbytes = sizeof(unsigned long long) * (size_t)s->niso * kCandGrid * kCandGrid;
  int rc;
  if ((rc = ensure(h, d_M, mbytes)) || (rc = ensure(h, d_n, sizeof(int))) || (rc = ensure(h, h->d_cand, sizeof(int32_t) * (size_t)cap))) return rc;
  HIPCHK(h, hipMemsetAsync(d_M.p, 0, mbytes, h->stream));
  HIPCHK(h, hipMemsetAsync(d_n.p, 0, sizeof(int), h->stream));
  const unsigned nb = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_cand_cellmax, dim3(nb), dim3(256), 0, h->stream, (long long)n, L.wavn, L.elow, L.gf, L.iso, L.inrange, Gm, d_M.as<unsigned long long>());
  hipLaunchKernelGGL(k_cand_prefix, dim3((unsigned)s->niso), dim3(kCandGrid), 0, h->stream, d_M.as<unsigned long long>());
  hipLaunchKernelGGL(k_cand_select, dim3(nb), dim3(256), 0, h->stream, (long long)n, L.wavn, L.elow, L.gf, L.iso, L.inrange, Gm,
                     d_M.as<unsigned long long>(), h->d_cand.as<int32_t>(), d_n.as<int>(), cap);
  int nc = 0;
  HIPCHK(h, hipMemcpyAsync(&nc, d_n.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  if (!(nc > 0 && nc <= cap)) return TRX_OK;
  h->ncand = nc;
  if ((rc = ensure(h, h->d_candrec, sizeof(CandLine) * (size_t)nc))) return rc;
  hipLaunchKernelGGL(k_cand_pack, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, h->stream, nc, h->d_cand.as<int32_t>(),
                     L.wavn, L.elow, L.gf, L.iso, L.inrange, h->d_candrec.as<CandLine>());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TRX_OK;
}

int prepare_lines(trx_handle *h, const trx_static *s)
{
  LinePrep Q;
  const int64_t n = Q.n = s->nlines;
  Q.nth = create_threads();
  Q.wn0 = s->wn_i; Q.odwn = s->wn_d / s->osamp; Q.own_last = Q.wn0 + (double)(s->nown - 1) * Q.odwn;
  if (n > 2000000000LL) return fail(h, TRX_E_UNSUPPORTED, "more than 2^31 lines per handle");
  // the three arrays that go up as they are leave now, on a thread of their own, under the grouping
  int rc_raw = TRX_OK;
  std::thread raw_up([&]() {
    (void)hipSetDevice(h->device);
    if ((rc_raw = upload_raw(h, h->d_elow, s->elow, (size_t)n)) || (rc_raw = upload_raw(h, h->d_gf, s->gf, (size_t)n)) ||
        (rc_raw = upload_raw(h, h->d_iso, s->isoid, (size_t)n))) return;
  });
  struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } raw_join{raw_up};
  int rc;
  if ((rc = line_wavenumbers(h, s, Q)) || (rc = check_line_order(h, s, Q)) || (rc = group_and_check(h, s, Q))) return rc;
  count_tables(h, s, Q);
  group_indices(s, Q);
  if ((rc = walk_ranges(h, s, Q))) return rc;
  raw_up.join();
  if (rc_raw) return rc_raw;
  if ((rc = upload_lines(h, Q))) return rc;
  if (h->walk_ok && (rc = walk_records(h, s, Q))) return rc;
  h->stats.nlines_inrange = h->ninrange; h->stats.ngroups = h->ngroups; h->stats.nadd = h->nadd;
  if ((rc = line_candidates(h, s, Q))) return rc;
  h->stats.ncandidates = h->ncand;
  Q.T.lap("candidates");
  return TRX_OK;
}

// ---- CIA: crosssec.c:272-344 + 354-428, device kernels ----------------------
// Host part: range checks and the no-extrapolation index windows only.
// density product of every CIA table and layer (crosssec.c:318-330), host side
void cia_densities(const trx_handle *h, const trx_atm *a, double *dens /* [ncia][nr] */)
{
  const int nr = a->nlayer;
  for (size_t n = 0; n < h->cia.size(); n++)
    for (int j = 0; j < nr; j++) {
      double d = 1.0;
      for (int k = 0; k < h->cia[n].nspec; k++) {
        const int m = h->cia[n].mol[k];
        d *= a->density[(size_t)m * nr + j] / (kAmu * h->mol_mass[m] * kAmagat);
      }
      dens[n * nr + j] = d;
    }
}

int cia_device(trx_handle *h, const trx_atm *a, const trx_opts *o, const double *d_tlay /* [nr] on device */,
               const double *d_dens /* [ncia][nr] on device */, hipStream_t cst)
{
  const int nr = a->nlayer; const long long nsh = h->nsh;
  if (h->cia.empty()) { HIPCHK(h, hipMemsetAsync(h->d_ecs.p, 0, sizeof(double) * (size_t)nr * nsh, cst)); return TRX_OK; }
  double tmin = 0.0, tmax = 70000.0;                        // crosssec.c:44-45, 175-176
  size_t nwmax = 0;
  for (auto &c : h->cia) { tmin = std::fmax(tmin, c.temp.front()); tmax = std::fmin(tmax, c.temp.back()); nwmax = std::max(nwmax, c.wn.size()); }
  for (int i = 0; i < nr; i++)
    if (a->temp[i] < tmin || a->temp[i] > tmax) return fail(h, TRX_E_RANGE, "layer temperature outside the CIA tables");
  int rc;
  // (per table of a batch: the table at the layers' temperatures, its second derivatives, and the sweeps' scratch -- one
  // piece per segment of k_cia_layers, each with room for its rows and both margins)
  const int seg_rows = h->sw.cia_segments ? 128 : 1 << 30;
  const size_t seg_vrows = h->sw.cia_segments ? (size_t)seg_rows + 2 * kCiaMargin + 8 : nwmax;
  const size_t seg_cap = h->sw.cia_segments ? (nwmax + (size_t)seg_rows - 1) / (size_t)seg_rows : 1;
  const size_t cia_job_doubles = (2 * nwmax + seg_cap * seg_vrows) * (size_t)nr;
  if ((rc = ensure(h, h->d_cia_ws, sizeof(double) * cia_job_doubles * std::min<size_t>(kCiaBatch, h->cia.size())))) return rc;
  auto wn_at = [&](long long i) { return o->wn_fct * (h->wn_i + (double)(h->lo + i) * h->wn_d); };
  CiaBatch B{};
  bool first = true;             // the first batch writes the whole array (k_cia_eval), also when it is empty
  auto flush = [&](bool last) {
    if (B.n == 0 && !(first && last)) return;
    int nwave = 0, fj0 = nr, lj1 = 0, fjl = nr, ljl = 0; long long fi0 = nsh, li1 = 0;
    for (int t = 0; t < B.n; t++) {
      nwave = std::max(nwave, B.J[t].iz - B.J[t].ia + 1);      // (rows of the widest window)
      fj0 = std::min(fj0, B.J[t].fj); lj1 = std::max(lj1, B.J[t].lj);
      fi0 = std::min(fi0, B.J[t].fi); li1 = std::max(li1, B.J[t].li);
    }
    fjl = fj0; ljl = lj1;
    if (first) { fj0 = 0; lj1 = nr; fi0 = 0; li1 = nsh; }
    if (B.n > 0) {
      hipLaunchKernelGGL(k_cia_rows, dim3((unsigned)(((long long)nwave * nr + 255) / 256), (unsigned)B.n), dim3(256), 0, cst, B, nr, d_tlay);
      bool sums = true;                    // every table of the batch has its weights: two sums per row instead of the sweeps
      for (int t = 0; t < B.n; t++) sums = sums && B.J[t].C.wf != nullptr;
      if (sums) {
        hipLaunchKernelGGL(k_cia_v, dim3((unsigned)(((long long)nwave * nr + 255) / 256), (unsigned)B.n), dim3(256), 0, cst, B, nr);
        hipLaunchKernelGGL(k_cia_z, dim3((unsigned)(((long long)nwave * nr + 255) / 256), (unsigned)B.n), dim3(256), 0, cst, B, nr);
      }
      unsigned nseg = 1;
      for (int t = 0; t < B.n && !sums; t++) {
        const long nw = B.J[t].C.nwave;
        const long need_a = B.J[t].ia == 0 ? 0 : B.J[t].ia + kCiaMargin, need_b = B.J[t].iz == nw - 1 ? nw - 1 : B.J[t].iz - kCiaMargin;
        if (h->sw.cia_segments && need_b >= need_a) nseg = std::max<unsigned>(nseg, (unsigned)((need_b - need_a + seg_rows) / seg_rows));
      }
      if (!sums)
        hipLaunchKernelGGL(k_cia_layers, dim3((unsigned)((ljl - fjl + 63) / 64), (unsigned)B.n, nseg), dim3(64), 0, cst, B, nr, seg_rows,
                           (long long)(seg_vrows * (size_t)nr));
    }
    if (nsh > 65536)
      hipLaunchKernelGGL(k_cia_eval<16>, dim3((unsigned)((li1 - fi0 + 255) / 256), (unsigned)((lj1 - fj0 + 15) / 16)), dim3(256), 0, cst,
                         B, nr, nsh, h->lo, h->wn_i, h->wn_d, o->wn_fct, fi0, li1, fj0, lj1, first ? 1 : 0, h->d_ecs.as<double>());
    else
      hipLaunchKernelGGL(k_cia_eval<1>, dim3((unsigned)((li1 - fi0 + 255) / 256), (unsigned)(lj1 - fj0)), dim3(256), 0, cst,
                         B, nr, nsh, h->lo, h->wn_i, h->wn_d, o->wn_fct, fi0, li1, fj0, lj1, first ? 1 : 0, h->d_ecs.as<double>());
    B.n = 0; first = false;
  };
  for (size_t n = 0; n < h->cia.size(); n++) {
    auto &c = h->cia[n];
    const long long nt1 = nsh; const int nt2 = nr;
    const double fx1 = c.wn.front(), lx1 = c.wn.back(), fx2 = c.temp.front(), lx2 = c.temp.back();
    if (wn_at(0) > lx1 || wn_at(nt1 - 1) < fx1 || a->temp[0] > lx2 || a->temp[nt2 - 1] < fx2) continue;   // crosssec.c:376-377
    // first index not below the table, first index above it (crosssec.c:381-393)
    long long fi = (long long)std::floor((fx1 / o->wn_fct - h->wn_i) / h->wn_d) - h->lo - 2;
    if (fi < 0) fi = 0;
    while (fi < nt1 && wn_at(fi) < fx1) fi++;
    long long li = (long long)std::ceil((lx1 / o->wn_fct - h->wn_i) / h->wn_d) - h->lo + 2;
    if (li > nt1) li = nt1;
    while (li > 0 && wn_at(li - 1) > lx1) li--;
    int fj = 0, lj = nt2;
    while (a->temp[fj] < fx2) fj++;
    for (int j = 0; j < lj; j++) if (a->temp[j] > lx2) lj = j;
    if (fi >= li || fj >= lj) continue;
    CiaJob &J = B.J[B.n];
    J.C = CiaDev{(int)c.wn.size(), (int)c.temp.size(), c.d_wn.as<double>(), c.d_temp.as<double>(), c.d_cs.as<double>(),
                 c.d_zt.as<double>(), c.d_uw.as<double>(), c.d_ruw.as<double>(), c.d_rh.as<double>(),
                 (h->sw.cia_sums && !c.wf.empty()) ? c.d_wf.as<double>() : nullptr, (h->sw.cia_sums && !c.wf.empty()) ? c.d_wb.as<double>() : nullptr};
    J.fj = fj; J.lj = lj; J.fi = fi; J.li = li;
    {   // table rows the wavenumber spline is solved for: those the run's wavenumbers bracket, a margin to spare (k_cia_layers)
      const int nw = (int)c.wn.size();
      J.ia = 0; J.iz = nw - 1;
      if (h->sw.cia_window && nw > 4 * kCiaMargin) {
        const double xa = wn_at(fi), xb = wn_at(li - 1);
        const int ra = (int)(std::upper_bound(c.wn.begin(), c.wn.end(), xa) - c.wn.begin()) - 1;      // last row at or below the first wavenumber
        const int rb = (int)(std::lower_bound(c.wn.begin(), c.wn.end(), xb) - c.wn.begin());          // first row at or above the last one
        const int ia = ra - 2 - kCiaMargin, iz = rb + 2 + kCiaMargin;
        if (ia >= 3) J.ia = ia;
        if (iz <= nw - 4) J.iz = iz;
      }
    }
    J.mid = h->d_cia_ws.as<double>() + cia_job_doubles * (size_t)B.n; J.z2 = J.mid + nwmax * nr; J.v = J.z2 + nwmax * nr;
    J.dens = d_dens + n * nr;
    if (++B.n == kCiaBatch) flush(false);
  }
  flush(true);
  HIPCHK(h, hipGetLastError());
  return TRX_OK;
}

// Simpson weights of one abscissa (numerical.c:390-425 geth, 486-495 makeh):
// per interval pair {2-hratio, hfactor, 2-1/hratio, hsum}; h0 = first interval.
// 1 / d for quotient_rn(x, d, 1/d) in place of x / d -- if that IS the division for this divisor:
// Markstein's theorem leaves out divisors with a mantissa of all ones, so the product form is
// compared with the division on a few thousand numerators of every magnitude an optical depth takes,
// exact multiples and their neighbours among them; any difference: 0 (the kernel divides).  Once per
// divisor and handle (a run's angles rarely change).
double checked_reciprocal(trx_handle *h, double d)
{
  for (auto &kv : h->recip_ok) if (kv.first == d) return kv.second;
  double rd = (d > 0 && std::isfinite(d)) ? 1.0 / d : 0.0;
  if (rd != 0.0) {
    uint64_t st = 0x9e3779b97f4a7c15ull ^ (uint64_t)(d * 1e15);
    for (int k = 0; k < 4096 && rd != 0.0; k++) {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      const double m = 1.0 + (double)(st >> 11) * 0x1.0p-53;                     // mantissa in [1, 2)
      const int ex = (int)((st >> 3) % 120) - 100;                                // 2^-100 .. 2^19
      double x = std::ldexp(m, ex);
      if (k % 4 == 1) x = std::ldexp((double)(1 + (st >> 40) % 4096), ex) * d;    // (near) exact multiples of the divisor
      if (k % 4 == 2) x = std::nextafter(std::ldexp((double)(1 + (st >> 40) % 4096), ex) * d, 0.0);
      if (quotient_rn(-x, d, rd) != -x / d) rd = 0.0;
    }
  }
  if (h->recip_ok.size() >= 64) h->recip_ok.clear();
  h->recip_ok.emplace_back(d, rd);
  return rd;
}

void simpson_weights(const double *x, int n, double *row, double *h0)
{
  *h0 = (n >= 2) ? x[1] - x[0] : 0.0;
  if (n < 3) return;
  const int even = (n % 2 == 0);
  for (int i = 0; i < (n - 1) / 2; i++) {
    const int j = 2 * i + even;
    const double ha = x[j+1] - x[j], hb = x[j+2] - x[j+1];
    const double hsum = ha + hb, hratio = hb / ha, hfactor = hsum * hsum / (ha * hb);
    row[4*i] = 2.0 - hratio; row[4*i+1] = hfactor; row[4*i+2] = 2.0 - 1.0 / hratio; row[4*i+3] = hsum;
  }
}

// smallest wavenumber w for which alphad*w/alphal >= 0.1 holds in double
// arithmetic (extinction.c:480); the predicate is monotone in w, so start from
// the algebraic root and walk the few ulps to the exact floating-point edge.
double doppler_refresh_cut(double alphad, double alphal)
{
  auto cond = [&](double w) { return alphad * w / alphal >= 1e-1; };
  if (!(alphad > 0) || !(alphal > 0)) {                 // degenerate widths: bisection over all doubles
    double lo = 0.0, hi = 1e300;
    if (!cond(hi)) return HUGE_VAL;
    if (cond(std::nextafter(0.0, 1.0))) return 0.0;
    while (std::nextafter(lo, hi) < hi) {
      double mid = lo + (hi - lo) / 2;
      if (mid <= lo || mid >= hi) mid = std::nextafter(lo, hi);
      if (cond(mid)) hi = mid; else lo = mid;
    }
    return hi;
  }
  double w = 1e-1 * alphal / alphad;
  if (!std::isfinite(w)) return HUGE_VAL;
  // (the neighbours of a positive finite double are its bit pattern +- 1: std::nextafter, a library call, was a
  // quarter of the prologue's time per (layer, isotope) pair)
  auto up = [](double x) { uint64_t u; std::memcpy(&u, &x, 8); u++; std::memcpy(&x, &u, 8); return x; };            // x > 0 finite -> next above (inf after DBL_MAX)
  auto down = [](double x) { uint64_t u; std::memcpy(&u, &x, 8); u--; std::memcpy(&x, &u, 8); return x; };          // x > 0 -> next below (+0 after the smallest denormal)
  if (!(w > 0)) w = std::nextafter(0.0, 1.0);
  while (!cond(w)) { w = up(w); if (!std::isfinite(w)) return HUGE_VAL; }
  for (;;) {
    const double p = down(w);
    if (p > 0 && cond(p)) w = p; else break;
  }
  return w;
}

// ---- RCCL, resolved at run time (the library must load on a CPU-only box) ---
struct Rccl {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  const char *(*GetLastError)(ncclComm_t) = nullptr;
  bool ok() const { return lib && GetUniqueId && CommInitRank && CommDestroy && AllGather; }
};
Rccl &rccl()
{
  static Rccl R;
  if (R.lib) return R;
  const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char *n : names) if ((R.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;    // the copy torch already mapped
  if (!R.lib) for (const char *n : names) if ((R.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
  if (!R.lib) return R;
  R.GetUniqueId  = (decltype(R.GetUniqueId))dlsym(R.lib, "ncclGetUniqueId");
  R.CommInitRank = (decltype(R.CommInitRank))dlsym(R.lib, "ncclCommInitRank");
  R.CommDestroy  = (decltype(R.CommDestroy))dlsym(R.lib, "ncclCommDestroy");
  R.CommAbort    = (decltype(R.CommAbort))dlsym(R.lib, "ncclCommAbort");
  R.AllGather    = (decltype(R.AllGather))dlsym(R.lib, "ncclAllGather");
  R.GetErrorString = (decltype(R.GetErrorString))dlsym(R.lib, "ncclGetErrorString");
  R.GetLastError = (decltype(R.GetLastError))dlsym(R.lib, "ncclGetLastError");
  return R;
}

// ---- per-layer scalars (extinction.c:364-395), shared by trx_run and trx_sweep_permol ----
struct LayerHost {
  size_t nli = 0, extra_off = 0;
  std::vector<double> &f64; std::vector<int32_t> &i32;      // (the handle's: no allocation per run)
  const int32_t *psmax = nullptr;
  LayerHost(std::vector<double> &f, std::vector<int32_t> &i) : f64(f), i32(i) {}
};

// -c/T per layer and the strength factor SIGCTE*ratio/(m*Z) per (layer, isotope): all k_layer_max needs of a run's
// inputs.  trx_run writes them first, straight into the pinned block, and launches the layer maxima before the rest of
// the prologue (prep_layers, which computes the same values again for the block's device copy).
inline double layer_negct(double temp) { return -kExpCte * kTliEfct / temp; }
inline double layer_strength(const trx_handle *h, int i, double z) { return kSigCte * h->iso_ratio[i] / (h->iso_mass[i] * z); }

// nearest_index(adop, v, 0, ndop) by its exact steps (build_table), walked from a nearby index: the Doppler indices
// one (layer, isotope) pair asks for lie a few steps apart, and a bisection each was most of prep_layers' time.
inline int dop_index(const trx_handle *h, double v, int from)
{
  const double *thr = h->dopthr.data();      // thr[0] = -inf, thr[ndop] = +inf
  while (from + 1 < h->ndop && v >= thr[from + 1]) from++;
  while (v < thr[from]) from--;
  return from;
}
inline int lor_index(const trx_handle *h, double v, int from)
{
  if (h->lorthr.empty()) return nearest_index(h->alor.data(), v, 0, h->nlor);
  const double *thr = h->lorthr.data();      // thr[0] = -inf, thr[nlor] = +inf
  while (from + 1 < h->nlor && v >= thr[from + 1]) from++;
  while (v < thr[from]) from--;
  return from;
}
inline int dop_index_far(const trx_handle *h, double v)
{
  const double *thr = h->dopthr.data();
  return (int)(std::upper_bound(thr + 1, thr + h->ndop, v) - thr) - 1;      // (thr[1 .. ndop-1] <= v, counted)
}

int prep_layers(trx_handle *h, int nr, const double *temp_k, const double *density /* [nmol][nr] */,
                const double *zpart /* [niso][nr] */, size_t extra_doubles, LayerHost &LH)
{
  const int niso = h->niso, nmol = h->nmol;
  const size_t nli = (size_t)nr * std::max(niso, 1);
  LH.nli = nli; LH.extra_off = 7 * nli;
  LH.f64.assign(7 * nli + extra_doubles, 0.0);
  LH.i32.assign(4 * nli, 0);
  double *negct = &LH.f64[0], *strength = negct + nr, *dens = strength + nli, *alphad = dens + nli,
         *alphal = alphad + nli, *wcut = alphal + nli;
  int32_t *idop0 = &LH.i32[0], *ilor = idop0 + nli, *psmax = ilor + nli, *npre = psmax + nli;
  LH.psmax = psmax;
  h->dens_over_m.resize(nmol);
  double *dm = h->dens_over_m.data();
  // (the indices of an isotope change by a step or two from a layer to the next: each isotope's walks start where the
  // layer above ended -- a bisection per pair and grid was a third of the prologue's time)
  h->guess_dop.assign((size_t)std::max(niso, 1), 0); h->guess_lor.assign((size_t)std::max(niso, 1), 0);
  h->guess_a0.assign((size_t)std::max(niso, 1), 0); h->guess_a1.assign((size_t)std::max(niso, 1), 0); h->guess_npre.assign((size_t)std::max(niso, 1), -1);
  for (int r = 0; r < nr; r++) {
    const double temp = temp_k[r];
    if (!(temp > 0)) return fail(h, TRX_E_ARG, "non-positive layer temperature");
    negct[r] = layer_negct(temp);
    const double fdoppler = std::sqrt(2 * kKb * temp / kAmu) * kSqrtLn2 / kLs;
    const double florentz = std::sqrt(2 * kKb * temp / kPi / kAmu) / (kAmu * kLs);
    for (int j = 0; j < nmol; j++) dm[j] = density[(size_t)j * nr + r] / h->mol_mass[j];      // (the first factor of the sum's terms, for every isotope)
    for (int i = 0; i < niso; i++) {
      double al = 0.0;
      const double *csd_i = &h->pair_csd[(size_t)i * nmol], *sq_i = &h->pair_sqrt[(size_t)i * nmol];
      for (int j = 0; j < nmol; j++)       // (the collision diameter and the reduced-mass root of the pair: constants of the handle)
        al += dm[j] * csd_i[j] * csd_i[j] * sq_i[j];
      al *= florentz;
      const double ad = fdoppler / h->iso_sqrtm[i];
      const size_t k = (size_t)r * niso + i;
      alphal[k] = al; alphad[k] = ad;
      idop0[k] = h->guess_dop[i] = dop_index(h, ad * h->wn_i, h->guess_dop[i]);
      ilor[k]  = h->guess_lor[i] = lor_index(h, al, h->guess_lor[i]);
      strength[k] = layer_strength(h, i, zpart[(size_t)i * nr + r]);
      dens[k] = density[(size_t)h->iso_imol[i] * nr + r];
      wcut[k] = doppler_refresh_cut(ad, al);
      // (Doppler indices at the ends of the isotope's lines, and the widest profile between two indices: asked for
      // several times per pair -- each index is looked up once, and on a table whose profiles widen with the Doppler
      // width, the usual case, the widest of a range is its last)
      const bool has_lines = h->iso_wmax[i] > 0;
      const int a0 = has_lines ? (h->guess_a0[i] = dop_index(h, ad * h->iso_wmin[i], h->guess_a0[i])) : idop0[k];
      const int a1 = has_lines ? (h->guess_a1[i] = dop_index(h, ad * h->iso_wmax[i], h->guess_a1[i])) : idop0[k];
      const int32_t *psl = &h->psizeT[(size_t)ilor[k] * h->ndop];
      auto widest_of = [&](int i0, int i1) {
        if (i0 > i1) std::swap(i0, i1);
        if (h->psize_mono) return psl[i1];
        int32_t m = 0;
        for (int d = i0; d <= i1; d++) m = std::max(m, psl[d]);
        return m;
      };
      int32_t pm = widest_of(std::min(idop0[k], std::min(a0, a1)), std::max(idop0[k], std::max(a0, a1)));
      // The bound is then tightened to the Doppler indices a line of this isotope can actually TAKE in
      // this layer, among the lines that can reach this handle's bins (all of the block, or -- a
      // shard -- those within the reach of the widest profile, pm, a cell to spare):
      //   * anchor >= wcut ("own", extinction.c:480-483): the index of its own wavenumber;
      //   * anchor < wcut: the sticky index -- the block's index at wn_i, or that of SOME anchor >= wcut
      //     anywhere in the block (k_sticky_index) -- whatever the window.
      // Doppler widths grow with the wavenumber: on a band that spans a factor of ten the widest
      // profile of the list is several times the widest one a low-wavenumber shard meets, and in the
      // deep layers (no anchor reaches wcut) every line takes the ONE profile of the index at wn_i.
      if (h->sw.shard_frames && has_lines) {
        double lo_w = h->iso_wmin[i], hi_w = h->iso_wmax[i];
        if (h->windowed()) {
          const double reach = ((double)pm + h->osamp) * (h->wn_d / h->osamp) + h->wn_d;
          lo_w = std::max(lo_w, h->wn_i + (double)h->lo * h->wn_d - reach);
          hi_w = std::min(hi_w, h->wn_i + (double)(h->hi - 1) * h->wn_d + reach);
        }
        const double wc = wcut[k];
        auto didx = [&](double w) { return w == h->iso_wmin[i] ? a0 : w == h->iso_wmax[i] ? a1 : dop_index_far(h, ad * w); };
        auto widest = [&](double wa, double wb) { return widest_of(didx(wa), didx(wb)); };
        int32_t pw = 0;
        if (lo_w <= hi_w) {
          const double own_lo = std::max(lo_w, wc), all_lo = std::max(h->iso_wmin[i], wc);
          int32_t w_own = -1;
          if (hi_w >= wc) pw = std::max(pw, w_own = widest(own_lo, hi_w));                      // own indices of the lines in reach
          if (lo_w < wc) {                                                                       // some line in reach takes the sticky index
            pw = std::max(pw, psl[idop0[k]]);
            if (h->iso_wmax[i] >= wc)
              pw = std::max(pw, w_own >= 0 && own_lo == all_lo && hi_w == h->iso_wmax[i] ? w_own : widest(all_lo, h->iso_wmax[i]));
          }
        }
        pm = std::min(pm, pw);
      }
      psmax[k] = pm;
      {   // groups of the block that refresh the Doppler index: wavn >= wcut (descending order)
        const double *gb = h->h_gwavn.data() + h->h_gblock[i];
        const double wc = wcut[k];
        // (the block's groups descend in wavenumber: bracketed by the per-cell counts first -- groups two cells above
        // wcut's are all >= it, groups two cells below all < it -- so that the bisection stays inside ~3 cells of groups
        // instead of walking 20 cold cache lines of a 10^6-entry array)
        const int32_t *cg = &h->h_cntge[(size_t)i * (h->nwn + 1)];
        const double kcd = std::floor((wc - h->wn_i) / h->wn_d);
        const long long kc = kcd < -4 ? -4 : kcd > (double)h->nwn + 4 ? h->nwn + 4 : (long long)kcd;
        const double *pa = gb + cg[std::min<long long>(std::max<long long>(kc + 2, 0), h->nwn)];
        const double *pz = gb + cg[std::min<long long>(std::max<long long>(kc - 2, 0), h->nwn)];
        // (the cut moves a little from a layer to the next: the search starts at the layer above's answer and doubles its
        // step -- the lines it touches are the ones the layer above left in the cache; the same partition point.  A step is
        // tested against what is left of [lo, hi) before the pointer is formed: none points outside the array)
        const double *lo = pa, *hi = pz;                       // [lo, hi): all of [gb, lo) >= wc, all of [hi, ..) < wc
        const long g0 = h->guess_npre[i];
        if (g0 >= 0 && gb + g0 >= pa && gb + g0 <= pz) {
          const double *p = gb + g0;
          long stepw = 1;
          if (p < pz && *p >= wc) {                            // the answer lies above p
            lo = p + 1;
            while (lo < hi) { if (stepw > hi - lo) break; const double *q = lo + stepw - 1; if (*q >= wc) { lo = q + 1; stepw *= 2; } else { hi = q; break; } }
          } else {                                             // at or below p
            hi = p;
            while (lo < hi) { if (stepw > hi - lo) break; const double *q = hi - stepw; if (*q >= wc) { lo = q + 1; break; } else { hi = q; stepw *= 2; } }
          }
        }
        const long np = (long)(std::partition_point(lo, hi, [wc](double w) { return w >= wc; }) - gb);
        npre[k] = (int32_t)np; h->guess_npre[i] = np;
      }
    }
  }
  return TRX_OK;
}

void layer_dev(const double *df, const int32_t *di, const LayerHost &LH, int nr, LayerDev &Y, const double *&d_wcut, const int32_t *&d_npre)
{
  const size_t nli = LH.nli;
  Y.negc_over_t = df; Y.strength_f = df + nr; Y.density = Y.strength_f + nli; Y.alphad = Y.density + nli;
  Y.alphal = Y.alphad + nli; d_wcut = Y.alphal + nli;
  Y.idop0 = di; Y.ilor = di + nli; Y.psmax = Y.ilor + nli; d_npre = Y.psmax + nli;
}

// ---- one step of the line sweep: Spans, walk_chunk, sweep_chunk, layer_maxima_and_sticky
#include "trx_api_sweep.hip.h"

}  // namespace

// ============================================================================
extern "C" {

int trx_comm_unique_id(void *id_out)
{
  if (!id_out) return TRX_E_ARG;
  static_assert(sizeof(ncclUniqueId) == TRX_COMM_ID_BYTES, "unique id size");
  Rccl &R = rccl();
  if (!R.ok()) return TRX_E_UNSUPPORTED;
  ncclUniqueId id;
  if (R.GetUniqueId(&id) != ncclSuccess) return TRX_E_HIP;
  std::memcpy(id_out, &id, sizeof(id));
  return TRX_OK;
}

// what went wrong in a call that has no handle to keep its message (trx_last_error(NULL))
thread_local std::string g_comm_err;

int trx_comm_create(const void *idp, int nranks, int rank, int device, void **comm_out)
{
  g_comm_err.clear();
  if (!idp || !comm_out || nranks < 1 || rank < 0 || rank >= nranks) return TRX_E_ARG;
  Rccl &R = rccl();
  if (!R.ok()) { g_comm_err = "librccl.so could not be loaded"; return TRX_E_UNSUPPORTED; }
  if (hipSetDevice(device) != hipSuccess) return TRX_E_NODEVICE;
  ncclUniqueId id; std::memcpy(&id, idp, sizeof(id));
  ncclComm_t c = nullptr;
  const ncclResult_t st = R.CommInitRank(&c, nranks, id, rank);
  if (st != ncclSuccess) {
    g_comm_err = std::string("ncclCommInitRank: ") + (R.GetErrorString ? R.GetErrorString(st) : "failed");
    if (R.GetLastError) { const char *m = R.GetLastError(nullptr); if (m && *m) g_comm_err += std::string(" -- ") + m; }
    return TRX_E_HIP;
  }
  *comm_out = (void *)c;
  return TRX_OK;
}

void trx_comm_destroy(void *comm)
{
  if (comm && rccl().ok()) (void)rccl().CommDestroy((ncclComm_t)comm);
}

void trx_comm_abort(void *comm)
{
  if (!comm || !rccl().ok()) return;
  if (rccl().CommAbort) (void)rccl().CommAbort((ncclComm_t)comm);
  else (void)rccl().CommDestroy((ncclComm_t)comm);
}


int trx_restore_extinction(trx_handle *h, int32_t nlayer, const double *e, const uint8_t *computed)
{
  if (!h || nlayer < 0 || (nlayer > 0 && (!e || !computed))) return TRX_E_ARG;
  h->saved.clear();
  if (nlayer == 0) return TRX_OK;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = ensure(h, h->d_e_saved, sizeof(double) * (size_t)nlayer * (size_t)h->nsh);
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(h->d_e_saved.p, e, sizeof(double) * (size_t)nlayer * (size_t)h->nsh, hipMemcpyHostToDevice));
  h->saved.assign(computed, computed + nlayer);
  return TRX_OK;
}

int trx_abi_version(void) { return TRX_ABI_VERSION; }

// HIP version the library was built with and the one of the runtime it is running on (a process
// may have mapped another copy of libamdhip64.so first, e.g. the one a PyTorch wheel bundles)
int trx_hip_versions(int *built, int *running)
{
  if (built) *built = HIP_VERSION;
  int v = 0;
  if (hipRuntimeGetVersion(&v) != hipSuccess) return TRX_E_HIP;
  if (running) *running = v;
  return TRX_OK;
}

int trx_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *trx_strerror(int st)
{
  switch (st) {
    case TRX_OK: return "success";
    case TRX_E_ARG: return "bad argument or inconsistent sizes";
    case TRX_E_NOMEM: return "host or device allocation failed";
    case TRX_E_HIP: return "HIP runtime call failed";
    case TRX_E_NODEVICE: return "no usable gfx950 device";
    case TRX_E_RANGE: return "value outside a table range";
    case TRX_E_UNSUPPORTED: return "option combination not implemented";
    case TRX_E_ORDER: return "line list is not sorted as the TLI format requires";
    case TRX_E_NOTREACHED: return "optical depth never reached toomuch (modlevel -1)";
  }
  return "unknown status";
}

const char *trx_last_error(const trx_handle *h) { return h ? h->err.c_str() : g_comm_err.c_str(); }

// The single exchange of a wavenumber-sharded job: every rank contributes `count` doubles (its
// spectrum slice, padded to the same length on every rank) and receives all of them, rank
// order, in d_all -- ncclAllGather on the handle's stream, synchronised on return.  Without a
// communicator (one rank) it is a device copy.
int trx_gather(trx_handle *h, const void *d_slice, void *d_all, int64_t count)
{
  if (!h || !d_slice || !d_all || count < 0) return TRX_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  if (h->comm) {
    if (rccl().AllGather(d_slice, d_all, (size_t)count, ncclDouble, (ncclComm_t)h->comm, h->stream) != ncclSuccess)
      return fail(h, TRX_E_HIP, "ncclAllGather failed");
  } else if (d_all != d_slice) {
    HIPCHK(h, hipMemcpyAsync(d_all, d_slice, sizeof(double) * (size_t)count, hipMemcpyDeviceToDevice, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TRX_OK;
}

// trx_gather for callers that keep their slices in host memory (the command-line driver): the
// slice goes to the device, is gathered there, and the whole comes back -- on every rank.
int trx_gather_host(trx_handle *h, const double *slice, double *all, int64_t count)
{
  if (!h || !slice || !all || count < 0) return TRX_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const int nranks = h->comm ? h->nranks : 1;
  DevBuf d_slice, d_all;
  int rc;
  if ((rc = ensure(h, d_slice, sizeof(double) * (size_t)std::max<int64_t>(count, 1))) ||
      (rc = ensure(h, d_all, sizeof(double) * (size_t)std::max<int64_t>(count, 1) * nranks))) return rc;
  HIPCHK(h, hipMemcpyAsync(d_slice.p, slice, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, h->stream));
  if ((rc = trx_gather(h, d_slice.p, d_all.p, count))) return rc;
  HIPCHK(h, hipMemcpy(all, d_all.p, sizeof(double) * (size_t)count * nranks, hipMemcpyDeviceToHost));
  return TRX_OK;
}

void trx_set_log(trx_log_fn fn, void *user, int max_level)
{
  LogSink &s = log_sink();
  s.fn = fn; s.user = user; s.max_level = max_level;
}

namespace {

// the checks that need no handle, in the order callers rely on (which code each bad argument returns)
int check_static(const trx_static *s)
{
  if (s->abi_version != TRX_ABI_VERSION) return TRX_E_ARG;
  if (s->nwn < 2 || s->osamp < 1 || s->nown != (s->nwn - 1) * s->osamp + 1) return TRX_E_ARG;
  if (s->ndop < 2 || s->nlor < 2 || s->ndop > kMaxDop) return TRX_E_UNSUPPORTED;
  if (s->niso < 0 || s->niso > kMaxIso || s->nmol < 1) return TRX_E_UNSUPPORTED;
  if (s->wn_lo < 0 || s->wn_hi > s->nwn || s->wn_lo >= s->wn_hi) return TRX_E_ARG;
  if (s->nlines < 0 || (s->nlines > 0 && (!s->wl_um || !s->isoid || !s->elow || !s->gf))) return TRX_E_ARG;
  if (s->nown > 2000000000LL) return TRX_E_UNSUPPORTED;     // iown/beg_j are int in the reference too
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || s->device < 0 || s->device >= ndev) return TRX_E_NODEVICE;
  return TRX_OK;
}

// ---- the queues.  Three streams that really overlap: the runtime hands out hardware queues round-robin, and with
// other streams in the process (an RCCL communicator, the caller's own) two of ours can land on
// ONE queue -- the CIA kernels then ran after the walks instead of under them, +0.11 ms per
// spectrum.  So every new stream is probed against the ones it must overlap and replaced (the
// next creation gets the next queue) until it does; after 12 tries it is taken as it is.
// (d_flag: 16 ints of device memory; a kernel on `a` waits for one on `b`: only two queues get through that)
bool streams_overlap(int *d_flag, hipStream_t a, hipStream_t b)
{
  int saw = 0; int *d_saw = d_flag + 8;
  if (hipMemsetAsync(d_flag, 0, 64, a) != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return true;
  hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, a, (volatile int *)d_flag, d_saw);
  hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, b, (volatile int *)d_flag);
  if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return true;
  if (hipMemcpy(&saw, d_saw, sizeof saw, hipMemcpyDeviceToHost) != hipSuccess) return true;
  return saw != 0;
}

int concurrent_stream(int *d_flag, hipStream_t *out, hipStream_t with1, hipStream_t with2)
{
  std::vector<hipStream_t> rejected;
  int code = TRX_OK;
  for (int attempt = 0; attempt < 12; attempt++) {
    hipStream_t s2 = nullptr;
    if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) { code = TRX_E_HIP; break; }
    if (attempt == 11 || (streams_overlap(d_flag, with1, s2) && (!with2 || streams_overlap(d_flag, with2, s2)))) { *out = s2; break; }
    rejected.push_back(s2);                  // kept alive until the end: destroying it would free its slot for the next try
  }
  for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
  return code;
}

int create_queues(trx_handle *h)
{
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return TRX_E_HIP;
  {
    DevBuf probe;
    int rc;
    if ((rc = ensure(h, probe, 64)) || (rc = concurrent_stream(probe.as<int>(), &h->stream4, h->stream, nullptr)) ||
        (rc = concurrent_stream(probe.as<int>(), &h->stream2, h->stream, h->stream4))) return rc;
  }
  if (hipEventCreateWithFlags(&h->ev_walk1, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_inputs, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_cia, hipEventDisableTiming) != hipSuccess) return TRX_E_HIP;
  return TRX_OK;
}

// grids, communicator, isotopes and molecules: host copies and the pair constants of the layer prologue
int species_constants(trx_handle *h, const trx_static *s)
{
  h->wn_i = s->wn_i; h->wn_d = s->wn_d; h->osamp = s->osamp; h->odwn = s->wn_d / s->osamp;
  h->nwn = s->nwn; h->nown = s->nown; h->lo = s->wn_lo; h->hi = s->wn_hi; h->nsh = s->wn_hi - s->wn_lo;
  h->niso = s->niso; h->nmol = s->nmol; h->ndop = s->ndop; h->nlor = s->nlor;
  h->comm = s->comm; h->nranks = s->comm ? std::max(1, s->nranks) : 1; h->rank = s->rank;
  if (h->comm && !rccl().ok()) return TRX_E_UNSUPPORTED;
  h->iso_mass.assign(s->iso_mass, s->iso_mass + s->niso);
  h->iso_sqrtm.resize(s->niso);
  for (int i = 0; i < s->niso; i++) h->iso_sqrtm[i] = std::sqrt(h->iso_mass[i]);
  h->iso_ratio.assign(s->iso_ratio, s->iso_ratio + s->niso);
  h->iso_imol.assign(s->iso_imol, s->iso_imol + s->niso);
  h->mol_mass.assign(s->mol_mass, s->mol_mass + s->nmol);
  h->mol_radius.assign(s->mol_radius, s->mol_radius + s->nmol);
  if (s->mol_pol) h->mol_pol.assign(s->mol_pol, s->mol_pol + s->nmol); else h->mol_pol.assign(s->nmol, 0.0);
  if (s->mol_is_h2) h->mol_is_h2.assign(s->mol_is_h2, s->mol_is_h2 + s->nmol); else h->mol_is_h2.assign(s->nmol, 0);
  for (int i = 0; i < s->niso; i++) if (s->iso_imol[i] < 0 || s->iso_imol[i] >= s->nmol) return TRX_E_ARG;
  h->pair_csd.assign((size_t)s->niso * s->nmol, 0.0); h->pair_sqrt.assign((size_t)s->niso * s->nmol, 0.0);
  for (int i = 0; i < s->niso; i++)
    for (int j = 0; j < s->nmol; j++) {
      h->pair_csd[(size_t)i * s->nmol + j] = h->mol_radius[j] + h->mol_radius[h->iso_imol[i]];
      h->pair_sqrt[(size_t)i * s->nmol + j] = std::sqrt(1 / h->iso_mass[i] + 1 / h->mol_mass[j]);
    }
  return TRX_OK;
}

// Weights of the sums that stand for the two sweeps of a CIA table's wavenumber spline (k_cia_v, k_cia_z): products of
// the sweeps' row-to-row factors, kCiaTerms of them per row.  What the sums leave out starts with a product of kCiaTerms
// factors; the weights are kept where the largest such product in the table (`worst`) is below 2^-60, else the sweeps run.
void cia_sum_weights(trx_handle::Cia &t, int k)
{
  const size_t nw = t.wn.size(), K = kCiaTerms;
  std::vector<double> wf(nw * K, 0.0), wb(nw * K, 0.0);
  double worst = 0.0;
  for (size_t i = 1; i + 1 < nw; i++) {
    double p = 1.0;                                   // forward: (-1)^k c[i] c[i-1] .. c[i-k+1], c[m] = h[m-1] / u[m-1] (m >= 2)
    for (size_t k = 0; k <= K; k++) {
      if (i < 1 + k) break;                           // row i - k < 1
      if (k < K) wf[i * K + k] = p; else worst = std::fmax(worst, std::fabs(p));
      const size_t m = i - k;                         // next factor: -c[m]
      if (m < 2) break;
      p *= -((t.wn[m] - t.wn[m - 1]) * t.ruw[m - 1]);
    }
    p = 1.0;                                          // backward: (-1)^k d[i] .. d[i+k-1] / u[i+k], d[m] = h[m] / u[m]
    for (size_t k = 0; k <= K; k++) {
      const size_t m = i + k;
      if (m + 1 >= nw) break;                         // row i + k > n - 2
      if (k < K) wb[i * K + k] = p * t.ruw[m]; else worst = std::fmax(worst, std::fabs(p));
      p *= -((t.wn[m + 1] - t.wn[m]) * t.ruw[m]);
    }
  }
  if (worst < 0x1p-60) { t.wf = std::move(wf); t.wb = std::move(wb); }
  if (log_sink().fn && log_sink().max_level >= TRX_LOG_DEBUG) {
    char msg[192];
    std::snprintf(msg, sizeof msg, "create: CIA table %d (%zu rows): second derivatives by %s (the largest product of %d row-to-row factors, the first the sums leave out: %.1e)",
                  k, nw, t.wf.empty() ? "the two sweeps" : "sums per row", kCiaTerms, worst);
    log_msg(TRX_LOG_DEBUG, msg);
  }
}

// one CIA table: host copies and the table-only halves of the two natural splines (spline_init,
// pu/src/spline.c:186-206) -- second derivatives along T of every row, and the pivots of the wavenumber sweep
int prepare_cia_table(const trx_cia &c, int k, trx_handle::Cia &t)
{
  if (c.nspec < 1 || c.nspec > 2 || c.nwave < 3 || c.ntemp < 3) return TRX_E_ARG;
  t.nspec = c.nspec; t.mol[0] = c.mol[0]; t.mol[1] = c.mol[1];
  t.wn.assign(c.wn, c.wn + c.nwave); t.temp.assign(c.temp, c.temp + c.ntemp);
  t.cs.assign(c.cs, c.cs + (size_t)c.nwave * c.ntemp);
  const size_t nw = (size_t)c.nwave, nt = (size_t)c.ntemp;
  std::vector<double> u(std::max(nw, nt)), v(std::max(nw, nt));
  t.zt.resize(nw * nt);
  for (size_t i = 0; i < nw; i++)
    spline_second_derivs(t.zt.data() + i * nt, t.temp.data(), t.cs.data() + i * nt, (long)nt, u.data(), v.data());
  std::vector<double> zdummy(nw), ydummy(nw, 0.0);
  t.uw.assign(nw, 0.0);
  spline_second_derivs(zdummy.data(), t.wn.data(), ydummy.data(), (long)nw, t.uw.data(), v.data());
  t.ruw.assign(nw, 0.0);                 // reciprocal pivots: the per-layer sweeps multiply instead of dividing
  for (size_t i = 0; i < nw; i++) if (t.uw[i] != 0.0) t.ruw[i] = 1.0 / t.uw[i];
  t.rh.assign(nw, 0.0);                  // reciprocal spacings 1/(wn[i+1]-wn[i])
  for (size_t i = 0; i + 1 < nw; i++) t.rh[i] = 1.0 / (t.wn[i + 1] - t.wn[i]);
  if (nw >= 8) cia_sum_weights(t, k);
  return TRX_OK;
}

int upload_cia(trx_handle *h)
{
  int rc;
  for (auto &c : h->cia)
    if ((rc = upload(h, c.d_wn, c.wn)) || (rc = upload(h, c.d_temp, c.temp)) || (rc = upload(h, c.d_cs, c.cs)) ||
        (rc = upload(h, c.d_zt, c.zt)) || (rc = upload(h, c.d_uw, c.uw)) || (rc = upload(h, c.d_ruw, c.ruw)) || (rc = upload(h, c.d_rh, c.rh)) ||
        (!c.wf.empty() && ((rc = upload(h, c.d_wf, c.wf)) || (rc = upload(h, c.d_wb, c.wb))))) return rc;
  return TRX_OK;
}

int opacity_grid(trx_handle *h, const trx_static *s)
{
  const trx_opacity_grid *g = s->ogrid;
  if (!g) return TRX_OK;
  if (g->nmol < 1 || g->ntemp < 2 || g->nlayer < 1 || g->nwave != s->nwn || !g->o || !g->temp || !g->mol_index) return TRX_E_ARG;
  for (long m = 0; m < g->nmol; m++) if (g->mol_index[m] < 0 || g->mol_index[m] >= s->nmol) return TRX_E_ARG;
  h->has_grid = true; h->og_nmol = g->nmol; h->og_ntemp = g->ntemp; h->og_nlayer = g->nlayer; h->og_nwave = g->nwave;
  h->og_temp.assign(g->temp, g->temp + g->ntemp); h->og_temp.push_back(HUGE_VAL);   // searched with hi = Ntemp (extinction.c:562)
  h->og_molidx.assign(g->mol_index, g->mol_index + g->nmol);
  const size_t no = (size_t)g->nlayer * g->ntemp * g->nmol * g->nwave;
  if (const int rc = ensure(h, h->d_og_o, sizeof(double) * no)) return rc;
  if (hipMemcpy(h->d_og_o.p, g->o, sizeof(double) * no, hipMemcpyHostToDevice) != hipSuccess) return TRX_E_HIP;
  return TRX_OK;
}

// the stages of trx_create behind the handle's allocation, in order; the first that fails ends it
int create_stages(trx_handle *h, const trx_static *s)
{
  int rc;
  if (hipSetDevice(h->device) != hipSuccess) return TRX_E_NODEVICE;
  if ((rc = create_queues(h)) || (rc = species_constants(h, s))) return rc;
  for (int k = 0; k < s->ncia; k++) {
    trx_handle::Cia t;
    if ((rc = prepare_cia_table(s->cia[k], k, t))) return rc;
    h->cia.push_back(std::move(t));
  }
  if ((rc = opacity_grid(h, s)) || (rc = upload_cia(h))) return rc;
  StageTimer TC;
  if ((rc = build_table(h, s))) return rc;
  TC.lap("Voigt table (plan+kernels+sync)");
  return prepare_lines(h, s);
}

}  // namespace

int trx_create(const trx_static *s, trx_handle **out)
{
  if (!s || !out) return TRX_E_ARG;
  *out = nullptr;
  if (const int rc = check_static(s)) return rc;
  trx_handle *h = new (std::nothrow) trx_handle();
  if (!h) return TRX_E_NOMEM;
  h->device = s->device;
  read_switches(h->sw);
  if (const int rc = create_stages(h, s)) {
    // the handle does not survive a failed create, so its error text cannot be asked for later:
    // without a message callback it goes to stderr
    if (!log_sink().fn && !h->err.empty()) std::fprintf(stderr, "trx_create: %s\n", h->err.c_str());
    trx_destroy(h);
    return rc;
  }
  char buf[256];
  std::snprintf(buf, sizeof buf, "trx_create: %lld lines (%lld in range, %lld co-added groups), %lld wavenumbers [%lld,%lld), "
                "Voigt table %dx%d = %lld floats, %zu CIA tables", (long long)s->nlines, (long long)h->stats.nlines_inrange,
                (long long)h->ngroups, (long long)s->nwn, (long long)h->lo, (long long)h->hi, s->ndop, s->nlor,
                (long long)h->tab_n, h->cia.size());
  log_msg(TRX_LOG_INFO, buf);
  *out = h;
  return TRX_OK;
}

void trx_destroy(trx_handle *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
  if (h->stream4) { (void)hipStreamSynchronize(h->stream4); (void)hipStreamDestroy(h->stream4); }
  for (auto e : h->ev_ac) (void)hipEventDestroy(e);
  for (auto e : h->ev_cb) (void)hipEventDestroy(e);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  for (hipEvent_t e : {h->ev_inputs, h->ev_run_a, h->ev_run_b, h->ev_join, h->ev_walk1, h->ev_cia}) if (e) (void)hipEventDestroy(e);
  delete h;                      // (the queues are idle: its device and pinned buffers go with it)
}

int trx_get_stats(const trx_handle *h, trx_stats *out)
{ if (!h || !out) return TRX_E_ARG; *out = h->stats; return TRX_OK; }

int trx_table_info(const trx_handle *h, int64_t *ps, int64_t *off, int64_t *total)
{
  if (!h) return TRX_E_ARG;
  const size_t n = (size_t)h->ndop * h->nlor;
  if (ps)  for (size_t k = 0; k < n; k++) ps[k] = h->psize[k];
  if (off) for (size_t k = 0; k < n; k++) off[k] = h->poff[k];
  if (total) *total = h->tab_n;
  return TRX_OK;
}

int trx_table_copy(const trx_handle *hc, float *out)
{
  trx_handle *h = const_cast<trx_handle *>(hc);
  if (!h || !out) return TRX_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpy(out, h->tab, sizeof(float) * (size_t)h->tab_n, hipMemcpyDeviceToHost));
  return TRX_OK;
}

int trx_width_grids(const trx_handle *h, double *adop, double *alor)
{
  if (!h) return TRX_E_ARG;
  if (adop) std::memcpy(adop, h->adop.data(), sizeof(double) * h->ndop);
  if (alor) std::memcpy(alor, h->alor.data(), sizeof(double) * h->nlor);
  return TRX_OK;
}

// ---- a run: what it is given (run_check), its state and the phases that queue it (Run), what it hands
// ---- back (Run::finish); run_once is the sequence of the phases
static int run_check(trx_handle *h, const trx_atm *a, const trx_opts *o)
{
  const int nr = a->nlayer;
  if (nr < 3) return fail(h, TRX_E_ARG, "at least three layers are needed");
  if (!h->saved.empty() && (int)h->saved.size() != nr) return fail(h, TRX_E_ARG, "restored extinction has another number of layers");
  if (!h->saved.empty() && h->has_grid) return fail(h, TRX_E_UNSUPPORTED, "restored extinction together with an opacity grid");
  if (o->solution != TRX_SOL_ECLIPSE && o->solution != TRX_SOL_TRANSIT) return fail(h, TRX_E_ARG, "unknown solution");
  if (o->solution == TRX_SOL_ECLIPSE && (o->nangles < 1 || o->nangles > kMaxAngles || !o->angles_deg))
    return fail(h, TRX_E_ARG, "eclipse needs 1..16 angles");
  if (o->solution == TRX_SOL_TRANSIT && o->modlevel != 1 && o->modlevel != -1) return fail(h, TRX_E_UNSUPPORTED, "modlevel must be 1 or -1");
  if (!(o->ethresh > 0)) return fail(h, TRX_E_ARG, "ethresh must be positive");
  if ((o->cloud_flag >= 2 || o->scat_flag == 2) && !a->abund && o->cloud_flag >= 2) return fail(h, TRX_E_ARG, "cloud model needs abundances");
  for (int i = 1; i < nr; i++) if (!(a->radius[i] > a->radius[i-1])) return fail(h, TRX_E_ARG, "radii must ascend");
  return TRX_OK;
}

namespace {

// the kernels' caps as the schedule reads them (trx_schedule.h)
constexpr ScheduleCaps kScheduleCaps{kEmisRowsAbove, kTailRays, kTailSteps, 65536, kMaxChunk, kTauH};
// (the side-queue tail waits for walk1 alone: the main queue may carry exactly one walk ahead of it -- tests/schedule_check.cpp
// shows the tail unordered against a third walk)
static_assert(kTailSteps == 2, "the side-queue tail waits for ev_walk1 alone: the main queue may carry exactly one walk ahead of it");

struct Run {
  // ---- what the run is given
  trx_handle *const h; const trx_atm *const a; const trx_opts *const o;
  double *const spectrum; void *const d_spectrum; trx_debug *const dbg; const Products want;
  const std::chrono::steady_clock::time_point t_host0;

  // ---- its shape and modes
  const int nr = a->nlayer; const int64_t nsh = h->nsh; const hipStream_t st = h->stream;
  const bool eager = o->eager != 0, prof = o->profile != 0, count = o->profile >= 2;
  const bool vertical = o->solution == TRX_SOL_ECLIPSE, extras_on = o->scat_flag != 0 || o->cloud_flag != 0;
  // Two streams: the line sweep of step c+1 (saturates the machine) runs on the main stream while the
  // optical depth of step c (a latency chain on a few waves) is integrated on stream4.
  const bool pipelined = !h->has_grid;
  // A handle remembers how deep the previous spectrum went (hint_layers) and plans its steps to
  // end exactly there; the run returns at that depth and goes on only if rays are still open.
  const bool stop_at_hint_ok = !h->has_grid && !eager && h->hint_layers > 0 && h->hint_layers <= nr;
  // (any run that hands its spectrum to pageable host memory stages it in the handle's pinned buffer when it is small:
  // the copy command into pageable memory is staged by the runtime anyway, 25 us behind the copy of the flags at configs[2])
  const bool stage_spec = spectrum && !d_spectrum && nsh <= (1 << 20);

  // ---- the input block (layout): its parts and their offsets, in doubles
  // [layer scalars f64 | ray geometry | impact parameters | CIA density products | layer scalars i32]
  LayerHost LH{h->run_f64, h->run_i32};
  int gstride = 0; size_t mw_doubles = 0, n_geom_all = 0, nli = 0, n_f64 = 0, n_geom = 0, n_ip = 0, n_cd = 0, n_i32 = 0;
  size_t off_geom = 0, off_ip = 0, off_cd = 0, off_i32 = 0, in_bytes = 0;

  // ---- the front end (layout, front_maxima)
  // (the start-up pass rides along with k_layer_max only where it is small next to it: a few
  // thousand threads striding over 10^7 rays took 20 ms at configs[4])
  const bool ride_along = nsh <= 65536;
  bool early_front = false; double *kmax_run = nullptr; RunInit RI{};      // (early_front: layer maxima launched from the pinned block, ahead of the host's prologue)

  // ---- the block in device memory (front_inputs), the spectrum's target, what the plan reads (workspaces)
  LayerDev Y{}; const double *d_wcut = nullptr; const int32_t *d_npre = nullptr;
  const double *d_press = nullptr, *d_tempk = nullptr, *d_mdens = nullptr, *d_nH = nullptr, *d_scatpol = nullptr, *d_rad = nullptr;
  const double *d_gw = nullptr, *d_gh0 = nullptr, *d_mw = nullptr, *d_mh0 = nullptr, *d_pw = nullptr, *d_ipv = nullptr, *d_ciadens = nullptr;
  double *d_out = nullptr; PlanInput P{};

  // ---- the queues: which kernel of a pass goes where, behind which event, is the schedule's (trx_schedule.h); here
  // its names become the handle's streams and events
  hipStream_t tst = nullptr;                   // the spectrum's queue (pass)
  hipStream_t queue(Queue q) const { return q == kQMain ? st : q == kQSide ? h->stream4 : h->stream2; }
  hipEvent_t event(const QueueOp &op) const {
    switch (op.ev) {
      case kEvInputs: return h->ev_inputs; case kEvCia: return h->ev_cia; case kEvJoin: return h->ev_join; case kEvWalk1: return h->ev_walk1;
      case kEvStepDone: return h->ev_ac[(size_t)op.idx]; case kEvRecordsFree: return h->ev_cb[(size_t)op.idx];
      default: return nullptr;
    }
  }

  // ---- the ray tail (plan_first_pass; all false once the run has resumed)
  TailChoice tail;
  TailArgs TA{}; int tail_nct = 0;
  const size_t tail_blocks = (size_t)((nsh + kTailRays - 1) / kTailRays);

  // ---- progress
  int r_top = nr - 1; bool resumed = false;
  ScheduleState sched;                         // steps and walks queued so far, over both passes
  CombineArgs comb[2];                         // a walk's combine, by record buffer, from its walk op to its combine op
  std::vector<uint8_t> layer_walked;           // [nr] (layout) layers swept by walk steps: 1 + the form that took them (stats)

  // ---- what comes back (results)
  int flags[8] = {}, status[4] = {}; double ms_cia = 0;
  std::vector<unsigned long long> counters;    // [3 * nr] (layout)
  Spans spans; Spans *const sp = prof ? &spans : nullptr;
  std::chrono::steady_clock::time_point t_host_prep = t_host0, t_host_queued = t_host0, t_lap = t_host0;
  const bool lap_on = log_sink().fn && log_sink().max_level >= TRX_LOG_DEBUG; std::string laps;

  // an error return must not leave work of this run in flight (the next run would overwrite its inputs underneath it)
  bool in_flight = false;
  ~Run() { if (in_flight) { (void)hipStreamSynchronize(h->stream4); (void)hipStreamSynchronize(h->stream2); (void)hipStreamSynchronize(h->stream); } }

  void lap(const char *what) {
    if (!lap_on) return;
    const auto n = std::chrono::steady_clock::now();
    char b[64]; std::snprintf(b, sizeof b, " %s %.0f", what, 1e3 * std::chrono::duration<double, std::milli>(n - t_lap).count());
    laps += b; t_lap = n;
  }
  // kernel arguments
  void model_args(TauArgs &T) const; void tau_args(TauArgs &T, int r_top_, int nc_) const; void emis_args(EmisArgs &E) const; void mod_args(ModArgs &M) const;
  // launches: the instantiation and the grid of a kernel family in one place
  void launch_tau(const TauArgs &T, hipStream_t q) const; void launch_ray_tail() const;
  void launch_run_init() const
  { hipLaunchKernelGGL(k_run_init, dim3((unsigned)std::min<long long>((std::max<long long>(nsh, 3LL * nr) + 255) / 256, 65536)), dim3(256), 0, st, RI); }
  // the phases, in the order run_once calls them
  int layout(); int front_maxima(); void host_inputs();            // (host_inputs: within front_maxima)
  int workspaces(); int front_inputs(); int grid_weights();        // (grid_weights: within front_inputs)
  int plan_first_pass(); int pass(); int resume(); int finish();
  // what a pass is made of: the ops of its schedule, issued one by one ...
  int issue(const QueueOp &op); SweepMode sweep_mode(const QueueOp &op) const;
  int walk(const QueueOp &op); int grid_step(const PlanStep &s); int cia_group(); int restore_rows(const QueueOp &op); int tau_substep(const QueueOp &op);
  int spectrum_kernel(); int ray_tail();
  // ... and the way back
  int results(const PassEnd &end);
  // ... and what the run makes of that spectrum (want), behind it on its queue
  int product_kernels();
};

// scattering / cloud models: the parameters of tau.c:193-214, extinction.c:587-693, and the per-ray
// wavenumber factors the optical-depth kernels multiply the layer parts with (k_extras_factors)
void Run::model_args(TauArgs &T) const
{
  T.nr = nr; T.nsh = nsh; T.lo = h->lo; T.wn_i = h->wn_i; T.wn_d = h->wn_d; T.wn_fct = o->wn_fct;
  T.scat_flag = o->scat_flag; T.cloud_flag = o->cloud_flag; T.nmol = h->nmol;
  T.scat_pref = std::pow(10.0, o->scat_logext) * kE0H2;
  T.press = d_press; T.temp = d_tempk; T.scat_pol = d_scatpol;
  T.cloud_top = o->cloud_top; T.cloud_bot = o->cloud_bot; T.cloud_ext = o->cloud_ext; T.cloud_gamma = o->cloud_gamma;
  T.cloud_Q = o->cloud_Q; T.cloud_r = o->cloud_r; T.cloud_sig = o->cloud_sig; T.cloud_refwn = o->cloud_refwn;
  T.mdens = d_mdens; T.nH = d_nH;
  if (extras_on) { T.xf_scat = h->d_xf.as<double>(); T.xf_cloud = T.xf_scat + nsh; T.xf_const = T.xf_cloud + nsh; }
}

void Run::tau_args(TauArgs &T, int r_top_, int nc_) const
{
  T.solution = o->solution; T.rad_fct = a->rad_fct; T.toomuch = o->toomuch;
  T.r_top = r_top_; T.nc = nc_; T.rad = d_rad; T.e = h->d_e.as<double>(); T.ecs = h->d_ecs.as<double>();
  T.er = h->d_er.as<double>(); T.tau = h->d_tau.as<double>(); T.last = h->d_last.as<int>();
  T.er_all = (dbg != nullptr || eager) ? 1 : 0;
  T.gw = d_gw; T.gstride = gstride; T.gh0 = d_gh0;
  model_args(T);
  T.flags = h->d_flags.as<int>(); T.eager = eager;
  T.pw = d_pw; T.acc = h->d_acc.as<double>(); T.lay = vertical ? d_pw + 6 * (size_t)nr : nullptr;
  T.hrs = d_pw + 4 * (size_t)nr; T.hr0 = T.hrs + nr; T.status = h->d_status.as<int>();
}

void Run::emis_args(EmisArgs &E) const
{
  E.nr = nr; E.nang = o->nangles; E.nsh = nsh; E.lo = h->lo; E.wn_i = h->wn_i; E.wn_d = h->wn_d; E.wn_fct = o->wn_fct;
  E.tau = h->d_tau.as<double>(); E.last = h->d_last.as<int>(); E.temp = d_tempk;
  std::vector<double> grid(o->nangles + 1);                    // eclipse.c:262-269
  grid[0] = 0.0 * kDeg; grid[o->nangles] = 90.0 * kDeg;
  for (int i = 1; i < o->nangles; i++) grid[i] = (o->angles_deg[i-1] + o->angles_deg[i]) * kDeg / 2.0;
  for (int i = 0; i < o->nangles; i++) {
    E.cosang[i] = std::cos(o->angles_deg[i] * kDeg);
    E.area[i] = std::pow(std::sin(grid[i+1]), 2.0) - std::pow(std::sin(grid[i]), 2.0);
    E.rcos[i] = checked_reciprocal(h, E.cosang[i]);
  }
  E.intens = h->d_intens.as<double>(); E.flux = d_out; E.e2tab = h->d_e2tab.as<double>();
}

void Run::mod_args(ModArgs &M) const
{
  M.nr = nr; M.modlevel = o->modlevel; M.transparent = o->transparent; M.nsh = nsh; M.toomuch = o->toomuch;
  M.ip_fct = a->rad_fct; M.srad = o->starrad_cm; M.tau = h->d_tau.as<double>(); M.last = h->d_last.as<int>();
  M.ip = d_ipv; M.gw = d_mw; M.gstride = gstride; M.gh0 = d_mh0; M.out = d_out; M.status = h->d_status.as<int>();
}

void Run::launch_tau(const TauArgs &T, hipStream_t q) const
{
  if (vertical) {
    // small shards: one wave per block spreads the (latency-bound) chains over more CUs
    const bool small = nsh <= 64 * 1024;
    const dim3 grid((unsigned)std::min<int64_t>((nsh + (small ? 63 : 255)) / (small ? 64 : 256), kTauMaxBlocks)), block(small ? 64 : 256);
    void (*const k[2][2])(TauArgs) = {{k_optical_depth_vertical<false, false>, k_optical_depth_vertical<false, true>},       // [small][extras]
                                      {k_optical_depth_vertical<true, false>, k_optical_depth_vertical<true, true>}};
    hipLaunchKernelGGL(k[small][extras_on], grid, block, 0, q, T);
    return;
  }
  const dim3 grid((unsigned)std::min<int64_t>((nsh + kTauW - 1) / kTauW, kTauMaxBlocks));
  hipLaunchKernelGGL(extras_on ? k_optical_depth<true> : k_optical_depth<false>, grid, dim3(256), 0, q, T);
}

void Run::launch_ray_tail() const
{
  void (*const k[2][3])(TailArgs) = {{k_ray_tail<0, false>, k_ray_tail<8, false>, k_ray_tail<kMaxAngles, false>},       // [extras][slant rays, <= 8 angles, more]
                                     {k_ray_tail<0, true>, k_ray_tail<8, true>, k_ray_tail<kMaxAngles, true>}};
  hipLaunchKernelGGL(k[extras_on][!vertical ? 0 : o->nangles <= 8 ? 1 : 2], dim3((unsigned)tail_blocks), dim3(kTailThreads), 0, tst, TA);
}

// ---- the input block's layout and what is sized by the run's shape alone
int Run::layout()
{
  int rc;
  // ray geometry: Simpson weights per start layer (eclipse.c:82-96, slantpath.c:76-95)
  // (eclipse geometry uses tabulated weights for its one three-point ray only: rows of one pair,
  // no modulation table -- 9 KB instead of 330 KB to build, copy and ship per run at 100 layers)
  gstride = vertical ? 4 : 4 * (nr / 2 + 1);
  mw_doubles = vertical ? 0 : (size_t)(nr + 1) * gstride;
  n_geom_all = (size_t)(nr + 1) * gstride + mw_doubles + 2 * (size_t)(nr + 1) + 4 * (size_t)nr + 2 * (size_t)nr +
               (vertical ? (size_t)kVertLay * nr : 0);       // (vertical rays: the chain's per-layer constants behind the rest)
  nli = (size_t)nr * std::max(h->niso, 1);
  n_f64 = 7 * nli + 8 * (size_t)nr; n_geom = vertical ? n_geom_all : 1; n_ip = (size_t)nr; n_cd = (size_t)nr * h->cia.size(); n_i32 = 4 * nli;
  off_geom = n_f64; off_ip = off_geom + n_geom; off_cd = off_ip + n_ip; off_i32 = off_cd + n_cd;
  in_bytes = (8 * off_i32 + 4 * n_i32 + 8 + 15) & ~(size_t)15;
  if ((rc = ensure_pinned(h, h->h_in, in_bytes)) || (rc = ensure(h, h->d_in, in_bytes)) || (rc = ensure_small(h, nr)) ||
      (rc = ensure(h, h->d_last, sizeof(int) * nsh)) || (rc = ensure(h, h->d_acc, sizeof(double) * 2 * nsh)) ||
      (rc = ensure(h, h->d_sticky, sizeof(int) * nli)))
    return rc;
  // the layer maxima of consecutive runs alternate between two arrays: the run's start-up pass
  // (which rides along with k_layer_max) zeroes the NEXT run's
  const size_t had = h->d_kmax.bytes;
  if ((rc = ensure(h, h->d_kmax, sizeof(double) * 2 * (size_t)nr))) return rc;
  if (h->d_kmax.bytes != had || !h->kmax_clean || h->kmax_nr != nr) {
    HIPCHK(h, hipMemsetAsync(h->d_kmax.p, 0, sizeof(double) * 2 * (size_t)nr, st));
    h->kmax_parity = 0; h->kmax_nr = nr;
  }
  h->kmax_clean = false;               // until this run has got through (an error return leaves the halves in doubt)
  kmax_run = h->d_kmax.as<double>() + (size_t)h->kmax_parity * nr;
  RI.last = h->d_last.as<int>(); RI.nsh = nsh; RI.acc = h->d_acc.as<double>();
  RI.counters = h->d_counters.as<unsigned long long>(); RI.ncounters = 3 * nr;
  RI.kmax = h->d_kmax.as<double>() + (size_t)(h->kmax_parity ^ 1) * nr; RI.nkmax = nr;
  RI.status = h->d_status.as<int>(); RI.flags = h->d_flags.as<int>(); RI.rays = (int)std::min<int64_t>(nsh, 0x7fffffff);
  h->kmax_parity ^= 1;
  counters.assign(3 * (size_t)nr, 0); layer_walked.assign((size_t)nr, 0);
  in_flight = true;
  return TRX_OK;
}

// ---- the device's first kernel, ahead of the host's prologue.  The strongest line of every layer (k_layer_max) needs
// -c/T and SIGCTE*ratio/(m*Z) only: they go into the pinned block first, the kernel reads them THERE (a few hundred
// doubles over the host link, once per block) and runs while the host computes widths, table indices, frames and ray
// geometry -- 12 us that used to lie in front of the device's first instruction.  The rest of the block reaches device
// memory by extra blocks of the next kernel (k_sticky_index, which reads its own few inputs from the pinned block too):
// no copy engine, no wait of a kernel for a copy's completion signal.  (Opacity-grid runs and runs without lines have
// no such kernels: the block is copied as before.)
int Run::front_maxima()
{
  int rc;
  early_front = !h->has_grid && h->ngroups > 0 && h->h_in.dev != nullptr;
  if (early_front) {
    double *hin = (double *)h->h_in.p;
    for (int r = 0; r < nr; r++) {
      if (!(a->temp[r] > 0)) return fail(h, TRX_E_ARG, "non-positive layer temperature");
      hin[r] = layer_negct(a->temp[r]);
      for (int i = 0; i < h->niso; i++) hin[(size_t)nr + (size_t)r * h->niso + i] = layer_strength(h, i, a->zpart[(size_t)i * nr + r]);
    }
    if (!ride_along) launch_run_init();
    LayerDev Yp{}; Yp.negc_over_t = (const double *)h->h_in.dev; Yp.strength_f = Yp.negc_over_t + nr;
    bool rode = false;
    if ((rc = launch_layer_max(h, Yp, nr, a->temp, 1, nullptr, st, kmax_run, ride_along ? &RI : nullptr, &rode))) return rc;
    lap("max");
  }
  // ---- layer prologue (extinction.c:364-395)
  if ((rc = prep_layers(h, nr, a->temp, a->density, a->zpart, 8 * (size_t)nr, LH))) return rc;
  lap("layers");
  h->walk_temp_ok = true;
  for (int r = 0; r < nr; r++) if (a->temp[r] < kWalkMinTemp) h->walk_temp_ok = false;
  host_inputs();
  lap("rays");
  if (LH.f64.size() != n_f64 || h->run_geom.size() != n_geom || h->run_ipv.size() != n_ip || LH.i32.size() != n_i32)
    return fail(h, TRX_E_HIP, "internal: the input block's layout");
  return TRX_OK;
}

// the host's share of a run's inputs beyond prep_layers: the layer scalars of the scattering / cloud
// models, the vertical rays' Simpson weights and per-layer chain constants, the impact parameters
void Run::host_inputs()
{
  const int nmol = h->nmol;
  std::vector<double> &f64 = LH.f64, &geom = h->run_geom, &ipv = h->run_ipv;
  // layer-only scalars of the scattering / cloud models (tau.c:193-214, extinction.c:617-621)
  double *press = &f64[LH.extra_off], *tempk = press + nr, *mdens = tempk + nr, *nH = mdens + nr,
         *scat_pol = nH + nr, *radv = scat_pol + nr;
  for (int r = 0; r < nr; r++) {
    press[r] = a->press ? a->press[r] : 0.0; tempk[r] = a->temp[r]; radv[r] = a->radius[r];
    double mm = 0, md = 0, sp = 0;
    for (int j = 0; j < nmol; j++) {
      const double d = a->density[(size_t)j * nr + r];
      if (a->abund) {
        const double q = a->abund[(size_t)j * nr + r];
        md += d / h->mol_mass[j] * q;
        if (h->mol_is_h2[j]) nH[r] = d / h->mol_mass[j] * q * kNavo;
        mm += h->mol_mass[j] * q;
      }
      sp += kPi * 8e-32 / 3. * std::pow(h->mol_pol[j], 2) * d / h->mol_mass[j] * kNavo;
    }
    mdens[r] = md * mm; scat_pol[r] = sp;
  }

  geom.assign(vertical ? n_geom_all : 1, 0.0);                    // (transit: device-built, k_slant_geometry -- nothing to prepare or ship here)
  if (vertical) {
    std::vector<double> sx(nr + 1);
    double *gw = &geom[0], *gh0 = gw + (size_t)(nr + 1) * gstride;
    double *pw = gh0 + (nr + 1) + mw_doubles + (nr + 1);    // pair weights by starting layer (vertical rays)
    // only the two-point ray (start layer nr-2) integrates with tabulated weights (eclipse.c:68-80);
    // all others run on the pair weights below
    const int rs = nr - 2;
    const double r3[3] = {a->radius[rs], (a->radius[rs] + a->radius[rs+1]) / 2.0, a->radius[rs+1]};
    sx[0] = 0.0;
    for (int i = 1; i < 3; i++) sx[i] = sx[i-1] + (r3[i] - r3[i-1]);
    simpson_weights(sx.data(), 3, gw + (size_t)rs * gstride, gh0 + rs);
    for (int k = 0; k + 2 < nr; k++) { double h0; simpson_weights(a->radius + k, 3, pw + 4 * (size_t)k, &h0); }
    // what the chain of bottom-point parabolas and Simpson sums needs per layer (VertLayer, trx_kernels.hip.h):
    // the same IEEE operations the kernels used to repeat in every block
    double *lay = pw + 6 * (size_t)nr;
    for (int rs = 0; rs < nr; rs++) {
      double *L = lay + (size_t)kVertLay * rs;
      if (rs + 1 < nr) {
        const double step = a->radius[rs + 1] - a->radius[rs];
        L[0] = step; L[1] = a->radius[rs] / step; L[2] = 2.0 * step * step;
        L[8] = 1.0 / step; L[9] = 1.0 / L[2]; L[10] = L[1] + 1.5;
      }
      for (int q = 0; q < 4; q++) L[3 + q] = pw[4 * (size_t)rs + q];
      L[7] = a->radius[rs]; L[11] = a->radius[rs] * a->radius[rs];
    }
  }
  ipv.resize((size_t)nr);
  for (int i = 0; i < nr; i++) ipv[i] = a->radius[nr - 1 - i];
}

// ---- workspaces, and what the step plan reads (trx_plan.h)
int Run::workspaces()
{
  int rc;
  // Layers per step.  The walk (narrow profiles) takes up to 64 layers, one per lane; its cost
  // hardly depends on how many lanes are busy, so its steps are as large as the plan allows.
  // The two-kernel form keeps a strength buffer per layer in flight: at most kMaxChunk, and
  // 8 where the profiles are wide.  Optical depths are integrated in sub-steps of at most tau_cap layers.
  const int user_chunk = o->layer_chunk > 0 ? std::max(3, o->layer_chunk) : 0;
  h->run_frame.resize((size_t)nr); h->run_wide.resize((size_t)nr);
  const bool any_wide = layer_frames(h, LH.psmax, nr, h->run_frame.data(), h->run_wide.data());      // some layer needs the two-kernel form
  const size_t gr_b = (size_t)std::max<int64_t>(h->ngroups, 1);
  P.sg_layers = any_wide ? (user_chunk ? std::min(user_chunk, kMaxChunk) : kMaxChunk) : 1;
  P.frame = h->run_frame.data(); P.very_wide = h->run_wide.data(); P.nr = nr; P.hint_layers = h->hint_layers; P.user_chunk = user_chunk;
  P.eager = eager; P.has_grid = h->has_grid; P.stop_at_hint_ok = stop_at_hint_ok; P.walk_cap = kWalkLayers; P.chunk_cap = kMaxChunk;
  if ((rc = ensure(h, h->d_SG, sizeof(double) * gr_b * P.sg_layers)) || (rc = ensure(h, h->d_idop8, gr_b * P.sg_layers)) ||
      (rc = ensure(h, h->d_e, sizeof(double) * nr * nsh)) || (rc = ensure(h, h->d_er, sizeof(double) * nr * nsh)) ||
      (rc = ensure(h, h->d_tau, sizeof(double) * nr * nsh)) ||
      (rc = ensure(h, h->d_intens, sizeof(double) * kMaxAngles * nsh)) || (rc = ensure(h, h->d_spec, sizeof(double) * nsh)))
    return rc;
  if (pipelined)
    while ((int)h->ev_ac.size() < nr + 1) {
      hipEvent_t e1, e2;
      if (hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&e2, hipEventDisableTiming) != hipSuccess) return fail(h, TRX_E_HIP, "event");
      h->ev_ac.push_back(e1); h->ev_cb.push_back(e2);
    }
  if (count && any_wide && (rc = ensure(h, h->d_part3, 24 * (size_t)kMaxChunk * ((((size_t)((nsh + kTileBins - 1) / kTileBins) + 3) / 4) + kXcds * kAccumXcdGroup))))
    return rc;
  return ensure(h, h->d_ecs, sizeof(double) * (size_t)nr * nsh);
}

// ---- the block filled and (no early front end) copied, the device's view of it; then the front kernels behind it
int Run::front_inputs()
{
  int rc;
  double *hin = (double *)h->h_in.p;
  // (-c/T and the strength factors are in place already where the layer maxima were launched from them -- the same
  // values: they are not written a second time under a kernel that may be reading them)
  const size_t skip = early_front ? (size_t)nr + nli : 0;
  std::memcpy(hin + skip, LH.f64.data() + skip, 8 * (n_f64 - skip));
  std::memcpy(hin + off_geom, h->run_geom.data(), 8 * n_geom);
  std::memcpy(hin + off_ip, h->run_ipv.data(), 8 * n_ip);
  cia_densities(h, a, hin + off_cd);
  std::memcpy(hin + off_i32, LH.i32.data(), 4 * n_i32);
  lap("block");
  t_host_prep = std::chrono::steady_clock::now();
  lap("prep");
  if (!early_front) { HIPCHK(h, hipMemcpyAsync(h->d_in.p, h->h_in.p, in_bytes, hipMemcpyHostToDevice, st)); lap("h2d"); }
  // With lines, every element of e the path reads is written first (the accumulation kernels
  // store every bin of a swept layer) and zeros only matter in the dumps.  Without any
  // in-range line (empty list, all lines outside the band, a CIA-only run) no kernel writes
  // e, but the optical-depth kernels still read it: it must be zero then.
  if (dbg || eager || (h->ngroups == 0 && !h->has_grid)) HIPCHK(h, hipMemsetAsync(h->d_e.p, 0, sizeof(double) * nr * nsh, st));
  if (dbg || eager) HIPCHK(h, hipMemsetAsync(h->d_tau.p, 0, sizeof(double) * nr * nsh, st));

  const double *df = h->d_in.as<double>();
  layer_dev(df, (const int32_t *)(df + off_i32), LH, nr, Y, d_wcut, d_npre);
  d_press = df + LH.extra_off; d_tempk = d_press + nr; d_mdens = d_tempk + nr; d_nH = d_mdens + nr; d_scatpol = d_nH + nr; d_rad = d_scatpol + nr;
  // (ray geometry: part of the input block in eclipse geometry, a device-built buffer of its own in transit geometry)
  if (!vertical && (rc = ensure(h, h->d_geom, sizeof(double) * n_geom_all))) return rc;
  d_gw = vertical ? df + off_geom : h->d_geom.as<double>(); d_gh0 = d_gw + (size_t)(nr + 1) * gstride;
  d_mw = d_gh0 + (nr + 1); d_mh0 = d_mw + mw_doubles; d_pw = d_mh0 + (nr + 1);
  d_ipv = df + off_ip; d_ciadens = df + off_cd;
  if (h->has_grid && (rc = grid_weights())) return rc;
  // ---- the sticky Doppler index of every layer (with the block's copy into device memory riding along), or -- no early
  // front end -- both front kernels behind the copy command.  The event marks the place of the main queue behind which
  // the inputs are in device memory: the CIA queue waits for it when its kernels are queued (behind the first walk's
  // launch, not on the host's way to the device's first kernel), the side queue in front of its first work of the run.
  if (early_front) {
    // (what k_sticky_index itself reads of the block, it reads from the pinned copy: nothing of a grid can wait for the
    // copy blocks of the same grid)
    const double *pf = (const double *)h->h_in.dev;
    LayerDev Yp{}; const double *p_wcut; const int32_t *p_npre;
    layer_dev(pf, (const int32_t *)(pf + off_i32), LH, nr, Yp, p_wcut, p_npre);
    if ((rc = launch_sticky(h, Yp, p_npre, nr, 1, nullptr, o->ethresh, st, kmax_run, pf, h->d_in.p, in_bytes))) return rc;
  } else {
    if (!ride_along) launch_run_init();
    bool rode = false;
    if (!h->has_grid &&
        (rc = layer_maxima_and_sticky(h, Y, d_npre, nr, a->temp, 1, nullptr, o->ethresh, st, kmax_run, ride_along ? &RI : nullptr, &rode))) return rc;
    if (ride_along && !rode) launch_run_init();      // no line kernel to ride along with (opacity-grid mode, no in-range line)
  }
  HIPCHK(h, hipEventRecord(h->ev_inputs, st));
  lap("kmax");
  return extras_on ? ensure(h, h->d_xf, sizeof(double) * (2 * (size_t)nsh + 8)) : TRX_OK;
}

// ---- opacity grid: temperature bracket and weights per layer (extinction.c:549-574)
int Run::grid_weights()
{
  if (h->og_nlayer != nr) return fail(h, TRX_E_ARG, "opacity grid has a different number of layers");
  const int nt = (int)h->og_ntemp, nm = (int)h->og_nmol;
  // (handle-kept like run_f64: the copies read them from the queue -- they must outlive this function -- and no allocation per run)
  std::vector<double> &og_layer = h->run_og_layer; std::vector<int> &og_itemp = h->run_og_itemp;
  og_layer.assign((size_t)(3 + nm) * nr, 0.0); og_itemp.assign((size_t)nr, 0);
  for (int r = 0; r < nr; r++) {
    const double temp = a->temp[r];
    if (temp < h->og_temp[0] || !(temp < h->og_temp[nt - 1])) return fail(h, TRX_E_RANGE, "layer temperature outside the opacity grid");
    int it = nearest_index(h->og_temp.data(), temp, 0, nt);
    if (temp < h->og_temp[it]) it--;
    og_itemp[r] = it;
    og_layer[r] = h->og_temp[it + 1] - temp; og_layer[nr + r] = temp - h->og_temp[it];
    og_layer[2 * (size_t)nr + r] = h->og_temp[it + 1] - h->og_temp[it];
    for (int m = 0; m < nm; m++) og_layer[(size_t)(3 + m) * nr + r] = a->density[(size_t)h->og_molidx[m] * nr + r];
  }
  const int rc = upload(h, h->d_og_layer, og_layer);
  return rc ? rc : upload(h, h->d_og_itemp, og_itemp);
}


// ---- the first pass planned (trx_plan.h), and with it whether the run ends in the ray tail (trx_tail.hip.h): a hinted
// run whose plan is one or two walk steps from the top ends in ONE kernel behind its walks -- no side
// queue, no combine / optical depth / emission launches.
int Run::plan_first_pass()
{
  int rc;
  // (the run's two timing events live with the handle: creating and destroying a pair per run was
  // ~10 us of host time, which a small shard waits for)
  if (!h->ev_run_a) { HIPCHK(h, hipEventCreate(&h->ev_run_a)); HIPCHK(h, hipEventCreate(&h->ev_run_b)); }
  // (device time of the run, trx_stats.ms_run_total: profiled runs only -- an event record is a
  // packet of its own between the spectrum kernel and the copy back)
  if (prof) HIPCHK(h, hipEventRecord(h->ev_run_a, st));
  h->stats.walk_steps = 0; h->stats.walk_records = 0; h->stats.walk_record_lanes = 0;
  for (int k = 0; k < 3; k++) h->stats.walk_form_steps[k] = h->stats.walk_form_layers[k] = h->stats.walk_form_record_lanes[k] = 0;
  if (!h->has_grid && lap_on) {
    std::string ln = "run: walk frame (bins) per layer, top first; 0 = two-kernel form:";
    for (int r = nr - 1; r >= 0; r--) ln += " " + std::to_string(h->run_frame[r]);
    log_msg(TRX_LOG_DEBUG, ln);
  }
  d_out = d_spectrum ? (double *)d_spectrum : h->d_spec.as<double>();
  plan_pass(P, r_top, stop_at_hint_ok, h->run_plan);
  TailIn ti;
  ti.ray_tail = h->sw.ray_tail; ti.tail_direct = h->sw.tail_direct; ti.two_queues = h->sw.two_queues;
  ti.stop_at_hint_ok = stop_at_hint_ok; ti.count = count; ti.has_lines = h->ngroups > 0; ti.no_saved = h->saved.empty(); ti.pipelined = pipelined;
  ti.nsh = nsh; ti.nwn = h->nwn; ti.pass = &h->run_plan;
  ti.host_spectrum = spectrum && !d_spectrum; ti.any_product = want.bs || want.px || want.br;
  tail = tail_choice(ti, kScheduleCaps);
  if ((tail.tail_spec || stage_spec) && (rc = ensure_pinned(h, h->h_spec, sizeof(double) * (size_t)nsh))) return rc;
  // Vertical rays: what the blocks of the tail add to the run's flags -- rays still open, deepest layer reached -- goes
  // into a pinned array, one entry per block, and the HOST adds it up behind the kernel (results).  The device-side sum was three
  // dependent device-scope atomics per block and, for the last block to arrive, four more round trips and a system-scope
  // fence: the kernel's last wave ended 5 us behind its last emission -- and every one of those fences writes back and
  // invalidates the L2 under the emission waves (8 us of emission with them, 3 without).  The run's status (slant
  // rays: what the reference exits on) goes into four slots behind the blocks' entries, one per code.
  return tail.tail_direct ? ensure_pinned(h, h->h_tailblk, 8 * tail_blocks + 16) : TRX_OK;
}

// CIA extinction (device), on a second stream: only the first optical-depth kernel needs
// e_cs, so the (latency-bound) spline kernels overlap the first sweep step.  Queued right
// after that step's kernels, which are what the GPU is waiting for.
int Run::cia_group()
{
  const auto t0 = std::chrono::steady_clock::now();
  if (extras_on) {        // (ahead of the first optical depth like everything on this queue)
    TauArgs X{};
    model_args(X);
    hipLaunchKernelGGL(k_extras_factors, dim3((unsigned)((nsh + 255) / 256)), dim3(256), 0, h->stream2, X,
                       h->d_xf.as<double>(), h->d_xf.as<double>() + nsh, h->d_xf.as<double>() + 2 * nsh);
  }
  if (!vertical) {        // the slant rays' geometry, ahead of the CIA kernels: both are waited for by the first optical depth
    SlantGeomArgs G{};
    G.rad = d_rad; G.nr = nr; G.fct = a->rad_fct; G.gstride = gstride;
    G.gw = const_cast<double *>(d_gw); G.gh0 = const_cast<double *>(d_gh0); G.mw = const_cast<double *>(d_mw); G.mh0 = const_cast<double *>(d_mh0);
    G.hrs = const_cast<double *>(d_pw) + 4 * (size_t)nr; G.hr0 = G.hrs + nr;
    hipLaunchKernelGGL(k_slant_geometry, dim3((unsigned)(nr + nr - 2)), dim3(64), 0, h->stream2, G);
  }
  if (const int rcc = cia_device(h, a, o, d_tempk, d_ciadens, h->stream2)) return rcc;
  ms_cia = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return TRX_OK;
}

// layers restored from an earlier run (trx_restore_extinction): their rows as they were saved
int Run::restore_rows(const QueueOp &op)
{
  const PlanStep &s = h->run_plan[(size_t)op.step];
  for (int c = 0; c < s.nc; c++) {
    const int r = s.r_top - c;
    if (h->saved[(size_t)r])
      HIPCHK(h, hipMemcpyAsync(h->d_e.as<double>() + (size_t)r * nsh, h->d_e_saved.as<double>() + (size_t)r * nsh, sizeof(double) * (size_t)nsh,
                               hipMemcpyDeviceToDevice, queue(op.q)));
  }
  return TRX_OK;
}

// one optical-depth sub-step; a profiled run brackets the sub-steps of a step together
int Run::tau_substep(const QueueOp &op)
{
  const hipStream_t q = queue(op.q);
  if (op.opens && prof && spans.begin(Spans::kTau, q)) return fail(h, TRX_E_HIP, "event");
  TauArgs T{};
  tau_args(T, op.r_top, op.nc);
  launch_tau(T, q);
  if (op.closes && prof && spans.end(q)) return fail(h, TRX_E_HIP, "event");
  if (op.closes) lap("tau");
  return TRX_OK;
}

int Run::grid_step(const PlanStep &s)
{
  if (prof && spans.begin(Spans::kSweep, st)) return fail(h, TRX_E_HIP, "event");
  GridArgs Gd{};
  Gd.o = h->d_og_o.as<double>(); Gd.nt = (int)h->og_ntemp; Gd.nm = (int)h->og_nmol; Gd.nr = nr;
  Gd.nwave = h->og_nwave; Gd.lo = h->lo; Gd.nsh = nsh; Gd.r_top = s.r_top; Gd.nc = s.nc; Gd.itemp = h->d_og_itemp.as<int>();
  Gd.w_lo = h->d_og_layer.as<double>(); Gd.w_hi = Gd.w_lo + nr; Gd.dg = Gd.w_hi + nr; Gd.dens = Gd.dg + nr;
  Gd.e = h->d_e.as<double>(); Gd.flags = h->d_flags.as<int>(); Gd.eager = eager;
  hipLaunchKernelGGL(k_grid_extinction, dim3((unsigned)((nsh + 255) / 256), (unsigned)s.nc), dim3(256), 0, st, Gd);
  if (prof && spans.end(st)) return fail(h, TRX_E_HIP, "event");
  return TRX_OK;
}

SweepMode Run::sweep_mode(const QueueOp &op) const
{
  SweepMode M{};
  M.eager = eager; M.prof = count; M.ethresh = o->ethresh;
  M.skip_done = (!eager && !(dbg && dbg->e));
  M.d_e = h->d_e.as<double>(); M.d_kmax = kmax_run; M.d_sticky = h->d_sticky.as<int>();
  M.st = queue(op.q);
  return M;
}

// a walk step's extinction as records: its combine is kept for the combine op, or (tail mode) its records wait for the tail
int Run::walk(const QueueOp &op)
{
  const PlanStep &s = h->run_plan[(size_t)op.step];
  WalkResult W;
  if (const int rc = walk_chunk(h, Y, d_wcut, s, sweep_mode(op), sp, op.parity, W)) return rc;
  if (tail.tail_mode) {
    TailStep &TS = TA.S[TA.nsteps++];
    TS.P = W.C.P; TS.part = W.C.part; TS.nc = s.nc;
    TA.skip = W.C.last;
  }
  else comb[op.parity] = W.C;
  for (int c = 0; c < s.nc; c++) layer_walked[(size_t)(s.r_top - c)] = (uint8_t)(1 + W.form);
  return TRX_OK;
}

// ---- one op of the pass's schedule (trx_schedule.h), on the queue and behind the events it names
int Run::issue(const QueueOp &op)
{
  int rc = TRX_OK;
  const PlanStep &s = h->run_plan[(size_t)op.step];
  switch (op.kind) {
    case kOpWait:     HIPCHK(h, hipStreamWaitEvent(queue(op.q), event(op), 0)); break;
    case kOpRecord:   HIPCHK(h, hipEventRecord(event(op), queue(op.q))); break;
    case kOpWalk:     rc = walk(op); lap("sweep"); break;
    case kOpSweep:    rc = sweep_chunk(h, Y, d_wcut, LH.psmax, s, P.sg_layers, sweep_mode(op), sp); lap("sweep"); break;
    case kOpGrid:     rc = grid_step(s); lap("sweep"); break;
    case kOpCombine:  rc = launch_combine(h, comb[op.parity], queue(op.q), sp); break;
    case kOpCia:      rc = cia_group(); lap("cia"); break;
    case kOpRestore:  rc = restore_rows(op); break;
    case kOpTau:      rc = tau_substep(op); break;
    case kOpTail:     rc = ray_tail(); break;
    case kOpSpectrum: rc = spectrum_kernel(); break;
  }
  return rc;
}

// ---- the ray tail: every address it reads or writes is checked on the host before the launch
int Run::ray_tail()
{
  const bool tail_direct = tail.tail_direct, tail_spec = tail.tail_spec;
  TA.niso = h->niso; TA.gblock = h->d_gblock.as<int32_t>(); TA.e = h->d_e.as<double>();
  for (int b = 0; b < h->niso && b < 64; b++) if (h->h_gblock[b] != h->h_gblock[b + 1]) TA.blocks |= 1ull << b;
  int nct = 0; for (int k = 0; k < TA.nsteps; k++) nct += TA.S[k].nc;
  tau_args(TA.T, nr - 1, nct);
  if (vertical) emis_args(TA.E); else mod_args(TA.M);
  if (tail_direct) {              // spectrum and flags straight into pinned host memory: no copy commands behind the kernel
    if (tail_spec) (vertical ? TA.E.flux : TA.M.out) = (double *)h->h_spec.dev;
    TA.host_flags = (int *)h->h_small.dev;
    TA.host_blocks = (int *)h->h_tailblk.dev;
    std::memset((char *)h->h_tailblk.p + 8 * tail_blocks, 0, 16);
    if (!vertical) TA.M.status_slots = TA.host_blocks + 2 * tail_blocks;
    tail_nct = nct;
  }
  // (a null or stale address here is a wild access of a whole grid: round 3's one memory fault -- a work-in-progress
  // tail storing the spectrum through a pinned buffer that no branch had allocated yet -- was exactly this kind)
  bool ok = TA.nsteps >= 1 && TA.nsteps <= kTailSteps && nct >= 3 && nct <= kTailLayers && TA.gblock && TA.e &&
            TA.T.ecs && TA.T.er && TA.T.tau && TA.T.last && TA.T.flags && TA.T.status && TA.T.rad &&
            (vertical ? (TA.T.acc && TA.T.lay && TA.T.gw && TA.E.flux && TA.E.intens && TA.E.temp && TA.E.e2tab)
                      : (TA.T.hrs && TA.T.hr0 && TA.T.gw && TA.M.out && TA.M.ip && TA.M.gw && TA.M.gh0 && TA.M.status)) &&
            (!extras_on || (TA.T.xf_scat && TA.T.xf_cloud)) && (!tail_direct || (TA.host_flags && TA.host_blocks));
  for (int k = 0; k < TA.nsteps && ok; k++)
    ok = TA.S[k].part && TA.S[k].nc >= 1 && TA.S[k].nc <= kWalkLayers && TA.S[k].P.blo && TA.S[k].P.bhi && TA.S[k].P.off && TA.S[k].P.wbase;
  if (!ok) return fail(h, TRX_E_HIP, "internal: incomplete arguments for the ray tail (not launched)");
  if (prof && spans.begin(Spans::kTau, tst)) return fail(h, TRX_E_HIP, "event");
  launch_ray_tail();
  if (prof && spans.end(tst)) return fail(h, TRX_E_HIP, "event");
  if (lap_on) log_msg(TRX_LOG_DEBUG, "run: ray tail over " + std::to_string(TA.nsteps) + " walk steps, " + std::to_string(nct) + " layers");
  return TRX_OK;
}

// ---- the spectrum of the layers swept so far, where no ray tail gives it: emission, or modulation
int Run::spectrum_kernel()
{
  if (resumed) HIPCHK(h, hipMemsetAsync(h->d_status.p, 0, 16, st));       // (a resumed run computes the spectrum a second time)
  const bool rows = h->nwn > kEmisRowsAbove;       // (by the job's grid, not the shard: all shards of a job add in the same order)
  const dim3 grows((unsigned)((nsh + 255) / 256));
  if (vertical) {
    EmisArgs E{};
    emis_args(E);
    if (rows) hipLaunchKernelGGL(k_emission_rows, grows, dim3(256), 0, st, E);
    else      hipLaunchKernelGGL(k_emission, dim3((unsigned)((nsh + kEmisWaves - 1) / kEmisWaves)), dim3(64 * kEmisWaves), 0, st, E);
  } else {
    ModArgs M{};
    mod_args(M);
    if (rows) hipLaunchKernelGGL(k_modulation_rows, grows, dim3(256), 0, st, M);
    else      hipLaunchKernelGGL(k_modulation, dim3((unsigned)((nsh + kModWaves - 1) / kModWaves)), dim3(64 * kModWaves), 0, st, M);
  }
  return TRX_OK;
}

// ---- results back: the copies, the wait, and (direct tail) the flags summed on the host
int Run::results(const PassEnd &end)
{
  const bool tail_direct = tail.tail_direct, tail_spec = tail.tail_spec;
  HIPCHK(h, hipGetLastError());
  if (prof) HIPCHK(h, hipEventRecord(h->ev_run_b, tst));
  // one copy into pinned memory: flags, status and (profiled runs) the counters
  if (!tail_direct) HIPCHK(h, hipMemcpyAsync(h->h_small.p, h->d_small.p, count ? 128 + 24 * (size_t)nr : 128, hipMemcpyDeviceToHost, st));
  // (on the spectrum's queue: a band run's tail may have run on the side queue)
  if (spectrum && !tail_spec) HIPCHK(h, hipMemcpyAsync(stage_spec ? h->h_spec.p : (void *)spectrum, d_out, sizeof(double) * nsh, hipMemcpyDeviceToHost, tst));
  lap("spectrum+copies");
  t_host_queued = std::chrono::steady_clock::now();
  if (end.sync_side) HIPCHK(h, hipStreamSynchronize(h->stream4));     // (the tail has waited for the main queue's walk: nothing is left there)
  HIPCHK(h, hipStreamSynchronize(st));
  // the tail stored the spectrum into the handle's pinned buffer, or the copy command did
  if (spectrum && (tail_spec || stage_spec)) std::memcpy(spectrum, h->h_spec.p, sizeof(double) * (size_t)nsh);
  if (tail_direct) {
    // the flags as tau_publish leaves them after the plan's last step (all of them zero but the rays' number
    // when the tail started: it covers the run from its first layer), from the blocks' entries.  (d_flags on the
    // device keeps its start-of-run values: resume() sends these there before any kernel reads them.)
    const int32_t *tb = (const int32_t *)h->h_tailblk.p;
    int still = 0, deep = 0;
    for (size_t b = 0; b < tail_blocks; b++) { still += tb[2 * b]; deep = std::max(deep, tb[2 * b + 1]); }
    const int f[8] = {still, 0, tail_nct, 0, deep, 0, 0, 0};
    std::memcpy(h->h_small.p, f, sizeof f);
    int st4[4] = {0, 0, 0, 0};
    for (int code = 1; code < 4; code++) if (tb[2 * tail_blocks + code]) st4[0] = code;      // (vertical rays raise none)
    std::memcpy((char *)h->h_small.p + 64, st4, 16);
  }
  std::memcpy(flags, h->h_small.p, sizeof(flags));
  std::memcpy(status, (const char *)h->h_small.p + 64, sizeof(status));
  if (count) std::memcpy(counters.data(), (const char *)h->h_small.p + 128, 24 * (size_t)nr);      // (else: zero, as made)
  return TRX_OK;
}

// ---- one pass: the planned steps (h->run_plan) from r_top down and the spectrum of what they swept as a schedule
// (trx_schedule.h; tests/schedule_check.cpp holds every consumer behind its producer), its ops issued in order, the
// products behind the spectrum, the way back
int Run::pass()
{
  int rc;
  ScheduleIn in;
  in.pipelined = pipelined; in.has_grid = h->has_grid; in.vertical = vertical; in.has_lines = h->ngroups > 0;
  in.tail = tail; in.saved = h->saved.empty() ? nullptr : h->saved.data(); in.nr = nr;
  const PassEnd end = schedule_pass(h->run_plan, in, kScheduleCaps, sched, h->run_sched);
  tst = queue(end.spectrum_q);
  for (const QueueOp &op : h->run_sched) if ((rc = issue(op))) return rc;
  r_top = h->run_plan.back().r_top - h->run_plan.back().nc;
  return (rc = product_kernels()) ? rc : results(end);
}

// Rays still descending below the expected depth (the atmosphere changed): the run goes on from there to the
// bottom, with the step kernels and no hint -- once; the second pass has nothing to resume to.
int Run::resume()
{
  // (the step kernels that go on from here read the flags on the device: where the host has added them up, they go there first)
  if (tail.tail_direct) HIPCHK(h, hipMemcpyAsync(h->d_flags.p, h->h_small.p, 32, hipMemcpyHostToDevice, st));
  tail = TailChoice{};
  resumed = true; h->hint_layers = P.hint_layers = 0;
  plan_pass(P, r_top, false, h->run_plan);
  return pass();
}

// what a run hands back: the handle's statistics and depth hint, the debug copies, the status raised on the device
int Run::finish()
{
  int rc;
  trx_stats &S = h->stats;
  S.layers_swept = flags[2];
  h->hint_layers = flags[4];
  S.neval = S.nskip = S.sum_bins = S.sum_bins_walk = S.walk_layers = 0;
  S.walk_form_bins[0] = S.walk_form_bins[1] = S.walk_form_bins[2] = 0;
  for (int r = 0; r < nr; r++) {
    S.sum_bins += (int64_t)counters[3*r]; S.neval += (int64_t)counters[3*r+1]; S.nskip += (int64_t)counters[3*r+2];
    if (const int fw = layer_walked[(size_t)r]) { S.walk_layers++; S.sum_bins_walk += (int64_t)counters[3*r]; S.walk_form_bins[fw - 1] += (int64_t)counters[3*r]; }
  }
  float ms = 0; if (prof) (void)hipEventElapsedTime(&ms, h->ev_run_a, h->ev_run_b); S.ms_run_total = ms;
  S.ms_cia = ms_cia;
  S.ms_host_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  if (lap_on) {
    char b[160];
    std::snprintf(b, sizeof b, "run: host %.0f us preparing inputs, %.0f us queueing, %.0f us waiting for the device",
                  1e3 * std::chrono::duration<double, std::milli>(t_host_prep - t_host0).count(),
                  1e3 * std::chrono::duration<double, std::milli>(t_host_queued - t_host_prep).count(),
                  1e3 * (S.ms_host_total - std::chrono::duration<double, std::milli>(t_host_queued - t_host0).count()));
    log_msg(TRX_LOG_DEBUG, std::string(b) + "; queueing by phase (us):" + laps);
  }
  S.ms_k_sweep = S.ms_k_walk = S.ms_k_accum = S.ms_tau = S.ms_sweep = 0; S.sweep_launches = 0;
  S.ms_k_walk_form[0] = S.ms_k_walk_form[1] = S.ms_k_walk_form[2] = 0; S.ms_walk_span = 0;
  if (prof) {
    // every launch counts (also the ~4 us gated ones after all rays stopped), so that
    // sum / launches is the average a kernel trace reports
    double t[Spans::kKinds] = {0, 0, 0, 0, 0, 0};
    spans.sum(t);
    S.ms_k_walk_form[0] = t[Spans::kWalk]; S.ms_k_walk_form[1] = t[Spans::kWalkLanes]; S.ms_k_walk_form[2] = t[Spans::kWalkPacked];
    S.ms_k_sweep = t[Spans::kSweep]; S.ms_k_walk = t[Spans::kWalk] + t[Spans::kWalkLanes] + t[Spans::kWalkPacked]; S.ms_k_accum = t[Spans::kAccum]; S.ms_tau = t[Spans::kTau];
    S.sweep_launches = sched.steps;
    S.ms_sweep = S.ms_k_sweep + S.ms_k_walk + S.ms_k_accum;
    S.ms_walk_span = spans.walk_span();
  }

  if (dbg) {
    if (dbg->e)    HIPCHK(h, hipMemcpy(dbg->e, h->d_e.p, sizeof(double) * nr * nsh, hipMemcpyDeviceToHost));
    if (dbg->e_cs) HIPCHK(h, hipMemcpy(dbg->e_cs, h->d_ecs.p, sizeof(double) * nr * nsh, hipMemcpyDeviceToHost));
    if (dbg->tau) {
      std::vector<double> t((size_t)nr * nsh);
      HIPCHK(h, hipMemcpy(t.data(), h->d_tau.p, sizeof(double) * nr * nsh, hipMemcpyDeviceToHost));
      for (int64_t w = 0; w < nsh; w++) for (int i = 0; i < nr; i++) dbg->tau[(size_t)w * nr + i] = t[(size_t)i * nsh + w];
    }
    if (dbg->last) {
      std::vector<int> l(nsh);
      HIPCHK(h, hipMemcpy(l.data(), h->d_last.p, sizeof(int) * nsh, hipMemcpyDeviceToHost));
      for (int64_t w = 0; w < nsh; w++) dbg->last[w] = l[w];
    }
    if (dbg->intens && o->solution == TRX_SOL_ECLIPSE)
      HIPCHK(h, hipMemcpy(dbg->intens, h->d_intens.p, sizeof(double) * o->nangles * nsh, hipMemcpyDeviceToHost));
    if (dbg->computed) for (int r = 0; r < nr; r++) dbg->computed[r] = (r >= nr - S.layers_swept) ? 1 : 0;
    if (dbg->er) HIPCHK(h, hipMemcpy(dbg->er, h->d_er.p, sizeof(double) * nr * nsh, hipMemcpyDeviceToHost));
    if (dbg->e_scat || dbg->e_cloud) {
      DevBuf d_x;
      if ((rc = ensure(h, d_x, sizeof(double) * 2 * (size_t)nr * nsh))) return rc;
      TauArgs T{};
      model_args(T);
      double *xs = d_x.as<double>(), *xc = xs + (size_t)nr * nsh;
      hipLaunchKernelGGL(k_extras_dump, dim3((unsigned)((nsh + 255) / 256), (unsigned)nr), dim3(256), 0, st, T, xs, xc);
      HIPCHK(h, hipStreamSynchronize(st));
      if (dbg->e_scat)  HIPCHK(h, hipMemcpy(dbg->e_scat, xs, sizeof(double) * nr * nsh, hipMemcpyDeviceToHost));
      if (dbg->e_cloud) HIPCHK(h, hipMemcpy(dbg->e_cloud, xc, sizeof(double) * nr * nsh, hipMemcpyDeviceToHost));
    }
  }
  if (status[0] == 1) return fail(h, TRX_E_NOTREACHED, "optical depth never reached toomuch (modlevel -1)");
  if (status[0] == 2) return fail(h, TRX_E_ARG, "fewer than three points for the radial integration");
  if (status[0] == 3) return fail(h, TRX_E_RANGE, "closest approach of a ray lies below the bottom layer (slantpath.c:39-44)");
  return TRX_OK;
}

}  // namespace

static int run_once(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, void *d_spectrum, trx_debug *dbg, const Products &want)
{
  const auto t_host0 = std::chrono::steady_clock::now();
  if (!h || !a || !o) return TRX_E_ARG;
  int rc;
  if ((rc = run_check(h, a, o))) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  Run R{h, a, o, spectrum, d_spectrum, dbg, want, t_host0};       // (behind run_check: its members are made from the run's shape)
  if ((rc = R.layout()) || (rc = R.front_maxima()) || (rc = R.workspaces()) || (rc = R.front_inputs()) || (rc = R.plan_first_pass()) || (rc = R.pass()))
    return rc;
  if (R.stop_at_hint_ok && R.flags[0] > 0 && R.r_top >= 0 && (rc = R.resume())) return rc;
  R.in_flight = false;                     // everything was joined into the main stream and waited for
  h->kmax_clean = true;
  return R.finish();
}

int trx_sweep_permol(trx_handle *h, int32_t nv, const double *temp, const double *density, const double *zpart,
                     double ethresh, int32_t nslot, const int32_t *iso_slot, double *out)
{
  if (!h || nv < 1 || !temp || !density || !zpart || !out || nslot < 1 || !iso_slot) return TRX_E_ARG;
  if (!(ethresh > 0)) return fail(h, TRX_E_ARG, "ethresh must be positive");
  const int niso = h->niso; const int64_t nsh = h->nsh;
  for (int i = 0; i < niso; i++) {
    if (iso_slot[i] < 0 || iso_slot[i] >= nslot) return fail(h, TRX_E_ARG, "isotope slot out of range");
    if (i > 0 && iso_slot[i] < iso_slot[i-1]) return fail(h, TRX_E_UNSUPPORTED, "isotopes of one molecule must be contiguous");
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  int rc;
  LayerHost LH(h->run_f64, h->run_i32);
  if ((rc = prep_layers(h, nv, temp, density, zpart, 0, LH))) return rc;
  h->walk_temp_ok = true;
  for (int r = 0; r < nv; r++) if (temp[r] < kWalkMinTemp) h->walk_temp_ok = false;
  const size_t gr_b = (size_t)std::max<int64_t>(h->ngroups, 1);
  std::vector<int32_t> slots(iso_slot, iso_slot + std::max(niso, 1));
  const std::unique_ptr<int[]> frame(new int[(size_t)nv]);      // the walk's frame per state, filled as a run's (Run::workspaces)
  const int sg_layers = layer_frames(h, LH.psmax, nv, frame.get(), nullptr) ? 12 : 1;
  if ((rc = ensure(h, h->d_SG, sizeof(double) * gr_b * sg_layers)) || (rc = ensure(h, h->d_idop8, gr_b * sg_layers)) ||
      (rc = ensure_small(h, nv)) ||
      (rc = ensure(h, h->d_pm, sizeof(double) * (size_t)nv * nslot * nsh)) ||
      (rc = upload(h, h->d_pm_f64, LH.f64)) || (rc = upload(h, h->d_pm_i32, LH.i32)) || (rc = upload(h, h->d_iso_mx, slots)))
    return rc;
  HIPCHK(h, hipMemsetAsync(h->d_pm.p, 0, sizeof(double) * (size_t)nv * nslot * nsh, st));
  LayerDev Y{}; const double *d_wcut; const int32_t *d_npre;
  layer_dev(h->d_pm_f64.as<double>(), h->d_pm_i32.as<int32_t>(), LH, nv, Y, d_wcut, d_npre);
  // (its own maxima array: [state][slot]; the runs' two halves are left dirty, trx_run re-zeroes them)
  if ((rc = ensure(h, h->d_kmax, sizeof(double) * (size_t)nv * nslot))) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_kmax.p, 0, sizeof(double) * (size_t)nv * nslot, st));
  h->kmax_clean = false;
  if ((rc = layer_maxima_and_sticky(h, Y, d_npre, nv, temp, nslot, h->d_iso_mx.as<int32_t>(), ethresh, st, h->d_kmax.as<double>()))) return rc;
  for (int r_top = nv - 1; r_top >= 0 && h->ngroups > 0; ) {
    const PlanStep s = plan_sweep_step(frame.get(), r_top, kWalkLayers, sg_layers);
    SweepMode M{};
    M.eager = true; M.ethresh = ethresh; M.nmx = nslot; M.d_iso_mx = h->d_iso_mx.as<int32_t>();
    M.permol = true; M.d_e = h->d_pm.as<double>(); M.d_kmax = h->d_kmax.as<double>(); M.d_sticky = h->d_sticky.as<int>();
    WalkResult W;      // (form -1: the two-kernel form)
    if (s.nb) { if (!(rc = walk_chunk(h, Y, d_wcut, s, M, nullptr, 0, W))) rc = launch_combine(h, W.C, st, nullptr); }
    else      rc = sweep_chunk(h, Y, d_wcut, LH.psmax, s, sg_layers, M, nullptr);
    if (rc) return rc;
    // (trx_stats does not count sweeps: the step plan goes to the log, one line per step -- tests read it)
    if (log_sink().fn && log_sink().max_level >= TRX_LOG_DEBUG)
      log_msg(TRX_LOG_DEBUG, std::string("sweep step: form ") + (W.form == 1 ? "lanes" : W.form == 2 ? "packed" : W.form == 0 ? "walk" : "two-kernel") +
                             ", states " + std::to_string(s.nc) + ", frame bins " + std::to_string(s.nb));
    r_top -= s.nc;
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, h->d_pm.p, sizeof(double) * (size_t)nv * nslot * nsh, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return TRX_OK;
}

int trx_run(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, trx_debug *dbg)
{
  if (!spectrum) return TRX_E_ARG;
  return run_once(h, a, o, spectrum, nullptr, dbg, Products{});
}

int trx_run_device(trx_handle *h, const trx_atm *a, const trx_opts *o, void *d_spectrum, trx_debug *dbg)
{
  if (!d_spectrum) return TRX_E_ARG;
  return run_once(h, a, o, nullptr, d_spectrum, dbg, Products{});
}

#include "trx_api_products.hip.h"
#include "trx_api_batch.hip.h"

}  // extern "C"
