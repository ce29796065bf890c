// trx_table.h -- the Voigt table's plan and the layouts of its three copies: everything about the
// table that depends on the grid fields of trx_static alone.  Plain C++ (no HIP): shared by
// trx_api.hip (build_table) and by tests/table_check.cpp, which checks the plan against the oracle
// and the layouts' invariants on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hip/trx_device.h"
#include "trx_numerics.h"

namespace trx {

// pu/src/iomisc.c:1064-1083 (logspace)
inline void logspace(double lo, double hi, int n, std::vector<double> &out)
{
  out.resize(n + 1);
  const double l0 = std::log10(lo), l1 = std::log10(hi);
  const double step = (l1 - l0) / (n - 1.0);
  for (int i = 0; i < n; i++) out[i] = std::pow(10, l0 + i * step);
  out[n] = HUGE_VAL;   // the reference searches with hi = n (extinction.c:393-394)
}

// Exact steps of the nearest-index function on an increasing grid of positive doubles (index_from in
// the kernels, dop_index / prep_layers on the host): thr[k] = smallest double v with
// nearest_index(grid, v, 0, n) >= k, found by bisection on the bit patterns; thr[0] = -inf,
// thr[n] = +inf.  False: the grid did not pass the check (thr is then not to be used).
inline bool index_steps(const double *grid, int n, std::vector<double> &thr)
{
  thr.assign((size_t)n + 1, 0.0);
  thr[0] = -HUGE_VAL; thr[n] = HUGE_VAL;
  auto idx = [&](double v) { return nearest_index(grid, v, 0, n); };
  for (int k = 1; k < n; k++) {
    if (!(grid[k - 1] > 0) || !(grid[k] > grid[k - 1])) return false;
    uint64_t a, b; double x;
    std::memcpy(&a, &grid[k - 1], 8); std::memcpy(&b, &grid[k], 8);      // idx(a) < k <= idx(b)
    while (b - a > 1) {
      const uint64_t m = a + (b - a) / 2;
      std::memcpy(&x, &m, 8);
      if (idx(x) >= k) b = m; else a = m;
    }
    std::memcpy(&thr[k], &b, 8);
    if (idx(thr[k]) != k || idx(std::nextafter(thr[k], 0.0)) != k - 1) return false;
  }
  return true;
}

// ---- the plan: opacity.c:219-277 + extinction.c:8-57 ------------------------
struct TablePlan {
  std::vector<double> adop, alor;                    // the width grids, +1 sentinel
  std::vector<int32_t> psize; std::vector<long long> poff; int64_t tab_n = 0;      // [ndop][nlor] half-widths and first floats; floats in all
  std::vector<ProfileJob> jobs;                      // the distinct profiles, in table order
  std::vector<int32_t> job_of;                       // [ndop][nlor] entry -> job (an alias: the job of the entry a Doppler row above)
  std::vector<int32_t> psizeT; bool psize_mono = true;      // psize as [nlor][ndop]; no profile narrower than the one a Doppler index below it
};

enum TablePlanError { kTablePlanOk = 0, kTablePlanArg, kTablePlanUnsupported };

// Grid: trx_static, or anything with its grid fields and their types -- int32 ndop, nlor, osamp; float dmin, dmax, lmin, lmax,
// timesalpha; double wn_d; int64 nown (the arithmetic below is the reference's).  text: what went wrong, for the caller's message.
template <class Grid>
TablePlanError plan_table(const Grid &g, TablePlan &P, const char **text)
{
  const int nd = g.ndop, nl = g.nlor;
  logspace((double)g.dmin, (double)g.dmax, nd, P.adop);
  logspace((double)g.lmin, (double)g.lmax, nl, P.alor);
  P.psize.assign((size_t)nd * nl, 0); P.poff.assign((size_t)nd * nl, 0); P.job_of.assign((size_t)nd * nl, 0);
  P.jobs.clear();
  const double dwn = g.wn_d / g.osamp;
  int64_t total = 0;
  for (int i = 0; i < nd; i++)
    for (int j = 0; j < nl; j++) {
      const size_t k = (size_t)i * nl + j;
      if (P.adop[i] * 10.0 < P.alor[j] && i != 0) {         // opacity.c:262-265: the alias rule
        P.psize[k] = P.psize[k - nl]; P.poff[k] = P.poff[k - nl]; P.job_of[k] = P.job_of[k - nl];
        continue;
      }
      const float dop = (float)P.adop[i], lor = (float)P.alor[j];   // extinction.c:11-12
      double big = dop; if (big < lor) big = lor;
      const double wv = big * g.timesalpha;
      int nv = 2 * (long)(wv / dwn + 0.5) + 1;
      if (nv < 2) nv = 3;
      if (nv > 2 * (int)g.nown) nv = 2 * (int)g.nown + 1;
      if (nv < 0) { *text = "negative Voigt profile size"; return kTablePlanArg; }
      ProfileJob J{};
      J.off = total; J.nv = nv; J.alphaL = lor; J.alphaD = dop;
      J.half = dwn * (long)(nv / 2);
      const bool quick = nv > 99999;                            // voigt.c:109, extinction.c:51
      // voigt.c:399-433
      double step = 2.0 * J.half / (nv - 1);
      int npts = 50; double sub = J.alphaD / (npts - 1);
      if (step < sub || quick) { sub = step; J.regime = quick ? 0 : 1; J.m = 1; }
      else {
        npts = (int)(step / sub) + 1;
        if (npts & 1) npts++;
        J.m = npts; J.regime = 2;
        const long long tot = (long long)nv * npts + 1;
        if (tot > 2000000000LL) { *text = "Voigt sub-sampling exceeds int range"; return kTablePlanUnsupported; }
        sub = 2.0 * J.half / (double)(tot - 1);
      }
      J.sub = sub; J.first_bin = total;
      P.job_of[k] = (int32_t)P.jobs.size();
      P.jobs.push_back(J);
      P.psize[k] = nv / 2; P.poff[k] = total;
      total += nv;
    }
  P.tab_n = total;
  P.psizeT.resize((size_t)nd * nl); P.psize_mono = true;
  for (int d = 0; d < nd; d++)
    for (int l = 0; l < nl; l++) {
      P.psizeT[(size_t)l * nd + d] = P.psize[(size_t)d * nl + l];
      if (d > 0 && P.psize[(size_t)d * nl + l] < P.psize[(size_t)(d - 1) * nl + l]) P.psize_mono = false;
    }
  return kTablePlanOk;
}

// floats of the table's allocation: kTabPad zeros in front and behind; behind the table kWalkMaxFrame
// cells of zeros, where the walk's lanes read what a slot does not reach; and kRowTail more:
// k_accumulate_rows stages whole 256-float pieces of a row (trx_rows.hip.h)
inline size_t table_alloc_floats(int64_t tab_n, int osamp)
{ return (size_t)tab_n + 2 * kTabPad + (size_t)kWalkMaxFrame * (size_t)std::min<int64_t>(osamp, 1 << 21) + kRowTail; }

// entries per row of a profile of nv points / of half-width ps (the same number: nv = 2 ps + 1)
inline int rows_entries(int nv, int osamp) { return (nv - 1) / osamp + 1; }

// ---- the phase-major copy (k_accumulate_wide): per job osamp rows back to back ----
struct PhaseMajorLayout { std::vector<long long> joffT, poffT; long long totT = 0; };      // per job, per entry; floats in all

inline PhaseMajorLayout phase_major_layout(const TablePlan &P, int osamp)
{
  PhaseMajorLayout T;
  T.joffT.resize(P.jobs.size()); T.poffT.resize(P.job_of.size());
  for (size_t j = 0; j < P.jobs.size(); j++) { T.joffT[j] = T.totT; T.totT += (long long)osamp * rows_entries(P.jobs[j].nv, osamp); }
  for (size_t e = 0; e < P.job_of.size(); e++) T.poffT[e] = T.joffT[(size_t)P.job_of[e]];
  return T;
}

// ---- the walk's rows (trx_walk.hip.h): phase-major rows, each between zeros (walk_row_layout) --
// the bins of a frame are CONSECUTIVE entries of one row, and what a narrow profile does not reach
// is zero by position (the pad behind a row is also the pad in front of the next).  One
// descriptor per table entry.
struct WalkLayout { std::vector<long long> joffW; std::vector<WalkProfile> prof; long long totW = 0; };

inline WalkLayout walk_layout(const TablePlan &P, int osamp)
{
  WalkLayout W;
  W.joffW.resize(P.jobs.size()); W.prof.resize(P.job_of.size());
  for (size_t j = 0; j < P.jobs.size(); j++) {
    int front, stride; walk_row_layout(rows_entries(P.jobs[j].nv, osamp), front, stride);
    W.joffW[j] = W.totW; W.totW += (long long)osamp * stride;
  }
  for (size_t e = 0; e < P.job_of.size(); e++) {
    const long long ps = P.psize[e], K = (2 * ps) / osamp + 1;
    int front, stride; walk_row_layout((int)K, front, stride);
    WalkProfile &D = W.prof[e];
    D.centre4 = (uint32_t)(4 * (W.joffW[(size_t)P.job_of[e]] + front + ps / osamp));
    D.rowb = (int32_t)(4 * stride);
    D.psr = (int32_t)(ps % osamp);
    D.ps = (int32_t)ps;
  }
  return W;
}

// 32-bit byte offsets: no copy when it would pass 4 GB (walk_chunk)
inline bool walk_rows_fit(long long totW) { return 4 * (totW + 2 * (long long)kTabPad) < (1LL << 32); }

// ---- compact rows (32 bytes) of the profiles with at most 8 entries per row: what
// k_line_walk_lanes<8> gathers, [phase][profile][8 floats] ----
struct CompactLayout {
  std::vector<long long> joff32;      // per job: first float of its row in a phase's slab (-1: no compact row)
  std::vector<uint32_t> c32;          // per entry: the same in bytes (0xffffffff: none)
  long long nq = 0, tot32 = 0;        // profiles with compact rows; floats in all
};

inline CompactLayout compact_layout(const TablePlan &P, int osamp)
{
  CompactLayout C;
  C.joff32.assign(P.jobs.size(), -1); C.c32.resize(P.job_of.size());
  for (size_t j = 0; j < P.jobs.size(); j++)
    if (rows_entries(P.jobs[j].nv, osamp) <= 8) C.joff32[j] = 8 * C.nq++;
  for (size_t e = 0; e < P.job_of.size(); e++) {
    const long long o = C.joff32[(size_t)P.job_of[e]];
    C.c32[e] = o < 0 ? 0xffffffffu : (uint32_t)(4 * o);
  }
  C.tot32 = C.nq * 8 * (long long)osamp;
  return C;
}

// a slab below 2^24 bytes and the phase below 2^24: the kernel's 24-bit multiply; the whole below 4 GB
inline bool compact_rows_fit(long long nq, long long tot32, int osamp)
{ return nq > 0 && 32 * nq < (1LL << 24) && osamp < (1 << 24) && 4 * tot32 < (1LL << 32); }

}  // namespace trx
