// trx_sweep.h -- what the launch of one line-sweep step decides on the host: a layer's frame, the ranges a
// shard's walk launches, the lines its two-kernel form launches, which walk kernel takes the step, and which
// layers of a two-kernel step go to the wide kernels.  Plain C++ (no HIP): shared by hip/trx_api_sweep.hip.h,
// which launches what is decided here, and by tests/sweep_check.cpp, which holds every function against a
// plain count over seeded random group tables.  Everything is a pure function of the host's group tables
// (GroupView) and of numbers the caller hands over: the handle never comes here, and the kernels' caps arrive
// as arguments (WalkCaps) because their headers are HIP.  The functions are static: none of them becomes a symbol of
// the library.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#ifndef SWEEP_MUTATION
#define SWEEP_MUTATION 0      // tests/sweep_check.cpp: 1..4 state one piece WRONGLY, and the check must catch each
#endif

namespace trx {

// the host's copies of the group tables, and the shard's window [lo, hi) of the nwn coarse cells
struct GroupView {
  int niso = 0;
  const int32_t *gblock = nullptr;      // [niso + 1] groups of isotope block b: [gblock[b], gblock[b+1]), descending cells
  const int32_t *cntge = nullptr;       // [niso][nwn + 1] groups of the block with cell >= k
  const int32_t *wbase = nullptr;       // [niso + 1] first range of the block (ranges of ngw consecutive groups)
  const int32_t *gfirst = nullptr, *gcount = nullptr;      // [ngroups] a group's first line and its members
  int ngw = 1;
  int64_t nwn = 0, lo = 0, hi = 0;
  int osamp = 1;
  bool windowed = false;
  bool has_groups(int b) const { return gblock[b] != gblock[b + 1]; }
  const int32_t *cnt_ge(int b) const { return cntge + (size_t)b * (size_t)(nwn + 1); }
};

// widest profile (in fine-grid points) any isotope with lines can use in layer r (psmax: [layer][niso])
static inline long long layer_psmax(const GroupView &G, const int32_t *psmax, int r)
{
  long long pm = 0;
  for (int b = 0; b < G.niso; b++)
    if (G.has_groups(b)) pm = std::max<long long>(pm, psmax[(size_t)r * G.niso + b]);
  return pm;
}

// Frame size of the walk for a layer whose widest profile is psm fine-grid points (bins a line can reach =
// 2*Rc + 2 with Rc whole cells of profile half-width), or 0 when its profiles are wider than the largest
// frame: the layer then takes the two-kernel path.  A per-LAYER property, so that the path a layer takes --
// and with it the order of its sums -- does not depend on how the layers are grouped into steps.
static inline int walk_frame_bins(bool walk_ok, bool walk_temp_ok, long long psm, int osamp)
{
  if (!walk_ok || !walk_temp_ok) return 0;
  const long long rc = psm / osamp;
  // (The 16-bin frame -- profiles reaching 4-7 cells -- used to pay only on sparse lists: with a load
  // per bin it cost 1.4 ms for the 9 such layers of configs[2] against ~0.4 ms in the two-kernel
  // form.  Reading rows of the table copy, two lanes per layer, it is the cheaper one there too:
  // 2.32 -> 2.26 ms.)
  return rc <= 0 ? 2 : rc <= 1 ? 4 : rc <= 3 ? 8 : rc <= 7 ? 16 : 0;     // (tab_n >= Rc*osamp follows: a profile that wide is in the table)
}

// a layer whose profiles span 64 coarse bins or more: it goes to the lanes-own-bins kernels, and the plan caps
// steps of such layers at 8 (trx_plan.h)    (measured: 16 or 32 here is 4x slower at configs[2] size, 128/256 no better)
static inline bool very_wide(long long psm, int osamp)
{
  return (2 * psm) / osamp + 1 >= (SWEEP_MUTATION == 4 ? 63 : 64);
}

// ---- the walk's window -----------------------------------------------------------------------
constexpr int kSweepSegs = 16;       // == kWalkSegs (trx_walk.hip.h): isotope blocks a launch can address separately

// the ranges of each isotope block that a launch covers: block-run s starts at range seg_w0[s] and its
// waves are [seg_cum[s], seg_cum[s+1]) of the launch's nw; nseg = 0: every range, nw = all of them
struct WalkWindow { int nseg = 0; int seg_w0[kSweepSegs] = {}; int seg_cum[kSweepSegs + 1] = {}; unsigned nw = 0; };

// A shard launches only the ranges that can reach it: per isotope block the groups whose cells
// lie within Rc + 1 cells of [lo, hi) are one run of consecutive ranges (cnt_ge look-up).  A range
// reaches the bins of its whole span (the plan's blo..bhi: its lowest cell - Rc to its highest + Rc + 1),
// and the combine reads its records there: so a range whose groups sit on both sides of the window,
// none inside, is launched too (it writes the zeros; skipped, the combine would add whatever the record
// buffer held).  Groups below cell 0 (the grid's first line when it lies just below the band) count
// as in reach of a window that starts within Rc + 1 cells of the bottom.
static inline WalkWindow walk_window(const GroupView &G, int nb, int nwaves)
{
  WalkWindow W;
  W.nw = (unsigned)nwaves;
  if (!G.windowed || G.niso > kSweepSegs || nwaves <= 0) return W;
  const int Rc = nb / 2 - 1;
  const long long klo = std::max<long long>(0, G.lo - Rc - 1);
  const long long khi = std::min<long long>(G.nwn - 1, G.hi - 1 + Rc - (SWEEP_MUTATION == 1 ? 1 : 0));
  int cum = 0, ns = 0;
  for (int b = 0; b < G.niso; b++) {
    if (!G.has_groups(b)) continue;
    const int32_t *cg = G.cnt_ge(b);
    // groups of the block (descending cells) with cell in [klo, khi]: [ga, gz)
    const int ga = cg[khi + 1];
    const int gz = (G.lo - Rc - 1 <= 0 && SWEEP_MUTATION != 3) ? G.gblock[b + 1] - G.gblock[b] : cg[klo];
    if (SWEEP_MUTATION == 2 && ga >= gz) continue;
    // the ranges holding a group on each side of ga and of gz - 1: empty only where the window falls between two ranges
    const int wa = G.wbase[b] + ga / G.ngw, wz = G.wbase[b] + (gz + G.ngw - 1) / G.ngw;
    if (wz <= wa) continue;
    W.seg_w0[ns] = wa; W.seg_cum[ns] = cum; cum += wz - wa; ns++;
  }
  W.seg_cum[ns] = cum; W.nseg = ns;
  W.nw = (unsigned)cum;
  if (ns == 0) { W.nseg = 1; W.seg_w0[0] = 0; W.seg_cum[0] = 0; W.seg_cum[1] = 0; }     // nothing reaches: no wave does anything
  return W;
}

// Lines whose profiles can reach the shard in any layer r_top .. r_top-nc+1 of a two-kernel step (contiguous
// per isotope block): the size of k_group_sweep's launch.  The kernel finds the runs themselves with the same
// arithmetic (trx_kernels.hip.h, "the runs of lines"): the two must be changed together.
static inline long long sweep_window_lines(const GroupView &G, const int32_t *psmax, int r_top, int nc)
{
  long long lines = 0;
  for (int b = 0; b < G.niso; b++) {
    if (!G.has_groups(b)) continue;
    const int gb0 = G.gblock[b], gb1 = G.gblock[b + 1];
    int ga = gb0, gz = gb1;
    if (G.windowed) {
      long long psm = 0;
      for (int c = 0; c < nc; c++) psm = std::max<long long>(psm, psmax[(size_t)(r_top - c) * G.niso + b]);
      const long long lo_f = (long long)G.osamp * G.lo - psm;
      const long long klo = lo_f > 0 ? lo_f / G.osamp : 0;
      long long khi = ((long long)G.osamp * (G.hi - 1) + psm) / G.osamp;
      if (khi > G.nwn - 1) khi = G.nwn - 1;
      const int32_t *cg = G.cnt_ge(b);
      ga = gb0 + cg[khi + 1]; gz = gb0 + cg[klo];
    }
    if (ga >= gz) continue;
    lines += ((long long)G.gfirst[gz - 1] + G.gcount[gz - 1]) - G.gfirst[ga];
  }
  return lines;
}

// ---- which kernel walks a step ---------------------------------------------------------------
enum WalkKind { kFormWalk = 0, kFormLanes = 1, kFormPacked = 2 };      // k_line_walk, k_line_walk_lanes, k_line_walk_packed

struct WalkCaps { int lanes_max_layers, lanes_max_group, rows_from; };      // kLanesMaxLayers, kLanesMaxGroup, kWalkRowsFrom

struct WalkFormIn {
  unsigned nw = 0;             // waves of the launch (walk_window)
  bool row_copy = false;       // the table's row copy exists (it would have passed 4 GB otherwise)
  int nb = 2, nc = 1;
  bool lanes_walk = true, lanes_force = false, packed_walk = true; int packed_max_layers = 0;      // the handle's switches
  int max_gcount = 0; long long ngroups = 0, nwn = 0;
  bool prof = false;           // a counting run
  int lanes_parts = 2;         // lanes_parts(nc, most) of trx_lanes.hip.h
};

struct WalkForm {
  int prod = kFormWalk;       // the form the production run takes: what trx_stats and the run's layer marks book
  int launched = kFormWalk;   // the form launched: a counting run takes the instrumented k_line_walk for every step (its
                               // per-layer counters are what prices each form's bytes, bench.py)
  int parts = 0;               // lanes: lanes per layer in phase 2
  int S = 0, packed_nb = 0;    // packed: ranges per wave, and the frame of the instantiation (a 2-bin step runs in the 4-bin row form: the same values)
  bool per_bin = false;        // plain: the per-bin instantiation (counting runs; wide frames without the row copy)
};

static inline WalkForm walk_form(const WalkFormIn &in, const WalkCaps &caps)
{
  WalkForm F;
  // steps of few layers with wide frames on a dense list: lanes = lines for the strengths (trx_lanes.hip.h)
  const bool lanes = in.nw > 0 && in.row_copy && in.nb >= 8 && in.nc <= caps.lanes_max_layers && in.lanes_walk &&
                     in.max_gcount <= caps.lanes_max_group && (in.ngroups >= 8 * in.nwn || in.lanes_force);
  // steps of few layers: several ranges per wave (k_line_walk_packed: an instruction serves S lines)
  const bool packed = !lanes && in.nw > 0 && in.row_copy && in.nc <= in.packed_max_layers && in.packed_walk;
  F.prod = lanes ? kFormLanes : packed ? kFormPacked : kFormWalk;
  F.launched = in.prof ? kFormWalk : F.prod;
  if (F.launched == kFormLanes) F.parts = in.lanes_parts;
  if (F.launched == kFormPacked) { F.S = 64 / in.nc; F.packed_nb = in.nb <= 4 ? 4 : in.nb; }
  // (no row copy: the wide frames run their per-bin form, which is the counting instantiation with the counters switched off)
  if (F.launched == kFormWalk) F.per_bin = in.prof || (in.nb >= caps.rows_from && !in.row_copy);
  return F;
}

// ---- the two-kernel form's layers --------------------------------------------------------------
// bit c = layer r_top - c.  wide: very_wide layers (k_accumulate skips them); m8: those of them whose profiles are
// at least row_m8_from bins wide (tiles of 512 bins in k_accumulate_rows); all_wide: k_accumulate has nothing to do
struct WideMasks { unsigned wide = 0, m8 = 0; bool all_wide = false; };

static inline WideMasks wide_masks(const GroupView &G, const int32_t *psmax, int r_top, int nc, long long row_m8_from)
{
  WideMasks W;
  for (int c = 0; c < nc; c++) {
    const long long psm = layer_psmax(G, psmax, r_top - c);
    if (!very_wide(psm, G.osamp)) continue;
    W.wide |= 1u << c;
    if (2 * psm + 1 >= row_m8_from) W.m8 |= 1u << c;
  }
  W.all_wide = W.wide == (nc >= 32 ? 0xffffffffu : ((1u << nc) - 1u));
  return W;
}

}  // namespace trx
