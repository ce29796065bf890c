// reach_check -- the reach bound of a line range and the whole-range exit of k_line_walk
// (transit_amd/csrc/hip/trx_device.h: walk_may_stick, walk_lane_reach, walk_range_reach, walk_cand_slots,
// walk_range_phases, walk_range_out_of_reach) on seeded random tables, layers and ranges, against brute force.
//
// A case draws a fine grid, a Voigt-table half-size array [ndop][nlor] (monotone in the Doppler index or not), a
// block of anchors over a band spanning a factor of 1.1 to 10, cut into ranges of 4 to 64 groups, and a step of
// 1 to 64 layers (Doppler width per wavenumber, Lorentz index, wcut inside / above / below the band, a sticky
// Doppler index).  The walk's start-up is restated for every range with the header's functions -- exactly what
// the kernel calls -- and held against every (group, layer): the profile the kernel would select for the lane
// (own: the nearest Doppler index of the anchor's wavenumber, anchor >= wcut; else sticky) reaches a bin of a
// frame exactly when imod <= ps or osamp - imod <= ps (the cell's own bin and the one above are the nearest
// slots on either side).
//   * no group the range's bound skips is within reach of a bin, in any layer;
//   * no range either exit test accepts holds such a group, and only ranges inside ONE cell are accepted (the
//     16-bit phases are recorded for those alone: the sparse block's ranges span cells and are always walked);
//   * the range's bound is never above the step's, and is the step's on a table that is not monotone;
//   * walk_cand_slots == 0 exactly when walk_group_out_of_reach, for frames of 2, 4, 8 and 16 bins.
// -DREACH_MUTATION=n restates the start-up WRONGLY (1: bound from the range's last anchor, 2: sticky profile left
// out, 3: "<=" for "<" at the zone's edges, 4: exit allowed when cell0 != cell1): each must be caught.
// Prints "<cases> cases, <bad> differ", then for a demo-shaped draw (2500-5000 cm-1, 313 groups per cell,
// osamp 2160, 64 Doppler-dominated layers whose widest profile reaches 0.331 of a cell at 5000 cm-1) the shares
// of groups evaluated under the step's and under the range's bound, and of ranges that exit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "hip/trx_device.h"

#ifndef REACH_MUTATION
#define REACH_MUTATION 0
#endif

using namespace trx;

static long bad = 0;
static int cases = 0;
#define EXPECT(cond, ...)                                                                          \
  do { if (!(cond)) { if (bad++ < 20) { std::printf("case %d: %s  ", cases, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Layer { double ad, wc; int il, idst; };
struct Table {
  int ndop, nlor; std::vector<double> thr; std::vector<int> psize; bool mono;
  int index(double v) const { return (int)(std::upper_bound(thr.begin() + 1, thr.begin() + ndop, v) - thr.begin()) - 1; }
  int ps(int d, int l) const { return psize[(size_t)d * nlor + l]; }
};
struct Block {
  double wn_i, odwn; int osamp, ngw;
  std::vector<double> wav; std::vector<int> iown;       // anchors, descending
};
struct Shares { long groups = 0, eval_step = 0, eval_range = 0, ranges = 0, exit1 = 0, exit2 = 0; };

// the profile half-size the kernel selects for a lane on a group (extinction.c:480-483)
static int selected(const Table &T, const Layer &Y, double w)
{
  return w >= Y.wc ? T.ps(T.index(Y.ad * w), Y.il) : T.ps(Y.idst, Y.il);
}

static void check_block(const Table &T, const Block &B, const std::vector<Layer> &Ls, int slack, bool switch_on, Shares &S)
{
  const int ng = (int)B.wav.size(), os = B.osamp;
  // the step's bound: the widest profile any lane takes on any group of the block (what prep_layers bounds
  // from above), plus slack
  int psm_s = 0;
  for (const Layer &Y : Ls) for (int g = 0; g < ng; g++) psm_s = std::max(psm_s, selected(T, Y, B.wav[g]));
  psm_s += slack;
  for (int g0 = 0; g0 < ng; g0 += B.ngw) {
    const int g1 = std::min(g0 + B.ngw, ng);
    const int cell0 = B.iown[g0] / os, cell1 = B.iown[g1 - 1] / os;
    // ---- k_range_info
    int imin = os, imax = 0;
    bool one_cell = cell0 == cell1;
    if (REACH_MUTATION == 4) one_cell = true;
    if (one_cell) for (int g = g0; g < g1; g++) { imin = std::min(imin, B.iown[g] % os); imax = std::max(imax, B.iown[g] % os); }
    const int32_t phases = walk_range_phases(one_cell, os, imin, imax);
    // ---- k_line_walk's start-up
    const bool range_reach = switch_on && T.mono;
    int lanes_max = 0;
    for (const Layer &Y : Ls) {
      const double w_first = REACH_MUTATION == 1 ? B.wav[g1 - 1] : B.wav[g0];
      const int ps_cur = T.ps(T.index(Y.ad * w_first), Y.il), ps_st = T.ps(Y.idst, Y.il);
      const bool may = REACH_MUTATION == 2 ? false : walk_may_stick(B.wn_i, B.odwn, os, cell1, Y.wc);
      lanes_max = std::max(lanes_max, walk_lane_reach(ps_cur, ps_st, may));
    }
    const int psm = walk_range_reach(psm_s, lanes_max, range_reach);
    EXPECT(psm <= psm_s, "range %d: %d > %d", g0, psm, psm_s);
    if (!range_reach) EXPECT(psm == psm_s, "range %d: %d != %d without the range's bound", g0, psm, psm_s);
    const int mut3 = REACH_MUTATION == 3 ? 1 : 0;
    const bool exit1 = range_reach && walk_range_out_of_reach(phases, os, psm_s - mut3);
    const bool exit2 = range_reach && walk_range_out_of_reach(phases, os, psm - mut3);
    EXPECT(!(exit1 && !exit2), "range %d: the step's bound exits, the range's does not", g0);
    const bool gone = exit1 || exit2;
    EXPECT(!gone || cell0 == cell1, "range %d exits with anchors in cells %d..%d", g0, cell1, cell0);
    S.ranges++; S.exit1 += exit1; S.exit2 += gone;
    // ---- every group of the range
    const int bound = psm - mut3, psq = bound / os, psr = bound - psq * os;
    for (int g = g0; g < g1; g++) {
      const int imod = B.iown[g] % os;
      const bool out = walk_group_out_of_reach(imod, os, bound);
      for (int NB = 2; NB <= 16; NB *= 2)
        if (psq <= NB / 2 - 1)
          EXPECT((walk_cand_slots(NB, imod, os, bound, psq, psr) == 0u) == out, "group %d, %d bins: slots disagree with the zone", g, NB);
      const bool skipped = gone || out;
      const bool skipped_step = walk_group_out_of_reach(imod, os, psm_s);
      S.groups++; S.eval_step += !skipped_step; S.eval_range += !skipped;
      if (!skipped) continue;
      for (size_t y = 0; y < Ls.size(); y++) {
        const int ps = selected(T, Ls[y], B.wav[g]);
        const bool reaches = imod <= ps || os - imod <= ps;
        EXPECT(!reaches, "group %d (range %d%s) skipped under bound %d, layer %zu reaches with ps %d at imod %d of %d",
               g, g0, gone ? ", exited" : "", bound, y, ps, imod, os);
      }
    }
  }
}

static Block draw_block(std::mt19937_64 &rng, double wlo, double whi, int ncells, int os, int ngw, double per_cell)
{
  std::uniform_real_distribution<double> U(0.0, 1.0);
  Block B; B.osamp = os; B.ngw = ngw;
  const double wn_d = (whi - wlo) / ncells;
  B.wn_i = wlo; B.odwn = wn_d / os;
  const long nown = (long)ncells * os + 1;
  const double last = B.wn_i + (double)(nown - 1) * B.odwn;
  const long n = std::max<long>(2, (long)(per_cell * ncells));
  std::vector<double> w((size_t)n);
  for (double &x : w) x = wlo + U(rng) * (last - wlo);
  // some anchors on, and half a step around, cell edges and the wcut-relevant grid points
  for (long k = 0; k < n / 16; k++) { const long c = (long)(rng() % (unsigned long)ncells); w[(size_t)k] = wlo + ((double)c * os + ((int)(rng() % 3) - 1) * 0.4999) * B.odwn; }
  std::sort(w.begin(), w.end(), std::greater<double>());
  int prev = -1;
  for (double x : w) {
    if (x < B.wn_i || x > last) continue;                       // extinction.c:410
    int iown = (int)((x - B.wn_i) / B.odwn);                     // extinction.c:445-447 (group_lines, trx_groups.h)
    auto own = [&](long k) { return B.wn_i + (double)k * B.odwn; };
    if (std::fabs(x - own(iown + 1)) < std::fabs(x - own(iown))) iown++;
    if (iown == prev) continue;                                  // (a line at an anchor's grid point joins its group)
    prev = iown;
    B.wav.push_back(x); B.iown.push_back(iown);
  }
  return B;
}

static Table draw_table(std::mt19937_64 &rng, int os, bool mono, double dlo, double dhi)
{
  Table T; T.ndop = 6 + (int)(rng() % 40); T.nlor = 2 + (int)(rng() % 6); T.mono = true;
  std::vector<double> adop((size_t)T.ndop);
  for (int d = 0; d < T.ndop; d++) adop[d] = dlo * std::pow(dhi / dlo, (double)d / (T.ndop - 1));
  T.thr.assign((size_t)T.ndop + 1, 0.0);
  T.thr[0] = -HUGE_VAL; T.thr[T.ndop] = HUGE_VAL;
  for (int d = 1; d < T.ndop; d++) T.thr[d] = 0.5 * (adop[d - 1] + adop[d]);
  T.psize.assign((size_t)T.ndop * T.nlor, 0);
  const double top = os * (0.05 + 1.6 * (double)(rng() % 1000) / 1000.0);      // widest Doppler-only half-size: 0.05 to 1.65 cells
  for (int l = 0; l < T.nlor; l++) {
    const int base = (int)(rng() % 4 == 0 ? top * (double)(rng() % 1000) / 500.0 : (rng() % 3));     // Lorentz floor of the column
    for (int d = 0; d < T.ndop; d++) {
      int v = std::max(base, (int)(top * adop[d] / dhi));
      if (!mono && rng() % 5 == 0) v = (int)(v * (double)(rng() % 1000) / 1000.0);
      T.psize[(size_t)d * T.nlor + l] = v;
    }
  }
  for (int l = 0; l < T.nlor; l++)
    for (int d = 1; d < T.ndop; d++) if (T.ps(d, l) < T.ps(d - 1, l)) T.mono = false;
  return T;
}

int main(int argc, char **argv)
{
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 400;
  std::mt19937_64 rng(20263);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int osamps[6] = {8, 24, 100, 400, 2160, 70000};
  const int ngws[4] = {4, 32, 64, 1};
  Shares all;
  long exits_seen = 0, nonmono = 0;
  for (int r = 0; r < rounds; r++, cases++) {
    const int os = osamps[r % 23 == 0 ? 5 : rng() % 5];
    const double wlo = 400.0 + 3000.0 * U(rng), factor = 1.1 + (r % 3 == 0 ? 8.9 : 1.5) * U(rng), whi = wlo * factor;
    const int ncells = 3 + (int)(rng() % 60);
    const bool dense = rng() % 2;
    const Block B = draw_block(rng, wlo, whi, ncells, os, ngws[rng() % 4], dense ? 40.0 + 300.0 * U(rng) : 0.2 + 3.0 * U(rng));
    if (B.wav.size() < 2) continue;
    // Doppler width per wavenumber of the layers: ad * w spans the table's grid over the band, and beyond its ends
    const double ad0 = 1e-6 * (0.5 + U(rng));
    const Table T = draw_table(rng, os, r % 4 != 3, ad0 * wlo * 0.8, ad0 * whi * 1.2);
    nonmono += !T.mono;
    const int ncs[4] = {1, 8, 24, 64};
    const int nc = ncs[rng() % 4];
    std::vector<Layer> Ls((size_t)nc);
    for (Layer &Y : Ls) {
      Y.ad = ad0 * (0.7 + 0.6 * U(rng)); Y.il = (int)(rng() % (unsigned)T.nlor); Y.idst = (int)(rng() % (unsigned)T.ndop);
      const unsigned kind = (unsigned)(rng() % 6);
      // wcut: below the band (every line own), above it (every line sticky), inside, or on / next to an anchor
      Y.wc = kind == 0 ? 0.0 : kind == 1 ? HUGE_VAL : kind == 2 ? B.wav[rng() % B.wav.size()] : kind == 3 ? std::nextafter(B.wav[rng() % B.wav.size()], HUGE_VAL) : wlo + U(rng) * (whi - wlo);
    }
    Shares S;
    check_block(T, B, Ls, rng() % 3 == 0 ? (int)(rng() % (unsigned)os) : 0, r % 11 != 10, S);
    exits_seen += S.exit2;
    all.groups += S.groups; all.ranges += S.ranges;
  }
  std::printf("%d cases, %ld differ\n", cases, bad);
  std::printf("(%ld groups in %ld ranges, %ld ranges exited, %ld tables not monotone)\n", all.groups, all.ranges, exits_seen, nonmono);

  // ---- a demo-shaped draw: the shares the walk's cost follows
  {
    std::mt19937_64 drng(1234);
    const int os = 2160, ncells = 2500;
    Block B = draw_block(drng, 2500.0, 5000.0, ncells, os, 64, 313.0);
    Table T; T.ndop = 200; T.nlor = 1; T.mono = true;
    // Doppler-dominated: half-size proportional to the wavenumber, 0.331 of a cell at 5000 cm-1 in the widest layer
    std::vector<double> adop((size_t)T.ndop);
    for (int d = 0; d < T.ndop; d++) adop[d] = 1800.0 * std::pow(5200.0 / 1800.0, (double)d / (T.ndop - 1));
    T.thr.assign((size_t)T.ndop + 1, 0.0); T.thr[0] = -HUGE_VAL; T.thr[T.ndop] = HUGE_VAL;
    for (int d = 1; d < T.ndop; d++) T.thr[d] = 0.5 * (adop[d - 1] + adop[d]);
    T.psize.resize((size_t)T.ndop);
    for (int d = 0; d < T.ndop; d++) T.psize[d] = (int)(0.331 * os * adop[d] / 5000.0);
    std::vector<Layer> Ls(64);
    for (int y = 0; y < 64; y++) { Ls[y].ad = 1.0 - 0.25 * y / 63.0; Ls[y].wc = 0.0; Ls[y].il = 0; Ls[y].idst = 0; }     // (widths fall by a quarter over the step's layers)
    Shares S;
    const long bad0 = bad;
    check_block(T, B, Ls, 0, true, S);
    std::printf("demo-shaped: %ld groups in %ld ranges; evaluated %.3f under the step's bound, %.3f under the range's; "
                "ranges exited %.3f by the step's bound, %.3f in all\n", S.groups, S.ranges, (double)S.eval_step / S.groups,
                (double)S.eval_range / S.groups, (double)S.exit1 / S.ranges, (double)S.exit2 / S.ranges);
    if (bad != bad0) std::printf("demo-shaped draw: %ld differ\n", bad - bad0);
  }
  return bad ? 1 : 0;
}
