// sweep_check -- the launch decisions of a line-sweep step (transit_amd/csrc/trx_sweep.h) on seeded random group tables,
// against plain counts over groups and ranges.
//
// A case draws 1 to 4 isotope blocks (one of them empty in most cases) of 0 to 60 groups in descending cells, clustered so
// that the grid has gaps, a few of them below cell 0 or past the last cell; nwn 8 to 200, 1 to 4 groups per range, osamp
// 1, 4 or 7; lines of 1 to 3 per group, in half of the cases with lines of no group between them.  The tables are built
// as trx_create builds them (trx_groups.h: count_ge with its key; the ranges' first per block).  Every case is held
// against every kind of window -- lo = 0, hi = nwn, width 1, at random, in every gap between two groups of a block
// (between two ranges, or inside one range) -- and Rc = 0, 1, 3, 7.
//   walk_window: every range holding a group whose cell lies in [lo - Rc - 1, hi - 1 + Rc] (or below cell 0 when the
//     window starts within Rc + 1 cells of the bottom) is launched; a block's launched ranges are one contiguous run
//     inside the block; seg_cum is the running sum and nw its last entry; at most one range at each end of a run
//     holds no group in reach, and none inside; a range with groups on both sides of the window and none inside is
//     launched; "nothing reaches" is one empty segment; no window or more than kSweepSegs blocks: every range.
//   sweep_window_lines: the lines from the first group to the last that a cell-by-cell count finds in reach --
//     the sum of their gcount where every line belongs to a group.
//   walk_frame_bins, very_wide, wide_masks: every boundary of their ladders, osamp 1 and 4.
//   walk_form: over every combination of its inputs -- one form; a counting run launches the plain walk and books the
//     production form; packed: S * nc <= 64; lanes exactly when all seven conditions hold, each dropped in turn.
// -DSWEEP_MUTATION=n states the header WRONGLY (1: khi one cell short, 2: the straddling range dropped, 3: gz without
// the below-cell-0 case, 4: very_wide from 63 bins): each must be caught.
// Prints "<cases> cases, <bad> differ", what the draws covered, and "ok <checks>".
#include <algorithm>
#include <random>
#include <vector>
#include "check_common.h"
#include "trx_groups.h"
#include "trx_sweep.h"

using namespace trx;

static int cases = 0;
#define EXPECT(cond)                                                                                   \
  do { g_checks++; if (!(cond)) { if (g_bad++ < 20) std::printf("case %d line %d: %s\n", cases, __LINE__, #cond); } } while (0)

static long n_straddle = 0, n_between = 0, n_in_gap = 0, n_nothing = 0, n_below0 = 0, n_windows = 0;

struct Tables {
  int niso, ngw, osamp; int64_t nwn;
  std::vector<int32_t> iown, gblock, wbase, gfirst, gcount;
  Heap<int32_t> cntge;
  bool lines_dense;
  Tables(int niso_, int64_t nwn_) : niso(niso_), nwn(nwn_), cntge((size_t)niso_ * (size_t)(nwn_ + 1)) {}
  long long cell(int g) const { return std::min<long long>(iown[(size_t)g] / osamp, nwn - 1); }      // count_tables' key
  int nwaves() const { return wbase[(size_t)niso]; }
  GroupView view(int64_t lo, int64_t hi) const {
    GroupView G;
    G.niso = niso; G.gblock = gblock.data(); G.cntge = cntge.get(); G.wbase = wbase.data();
    G.gfirst = gfirst.data(); G.gcount = gcount.data();
    G.ngw = ngw; G.nwn = nwn; G.lo = lo; G.hi = hi; G.osamp = osamp; G.windowed = lo > 0 || hi < nwn;
    return G;
  }
};

static Tables draw(std::mt19937_64 &rng, int niso, int64_t nwn, const std::vector<int> &ngroups)
{
  Tables T(niso, nwn);
  const int os[3] = {1, 4, 7};
  T.osamp = os[rng() % 3]; T.ngw = 1 + (int)(rng() % 4); T.lines_dense = rng() % 2;
  T.gblock.assign((size_t)niso + 1, 0);
  int32_t line = 0;
  for (int b = 0; b < niso; b++) {
    std::vector<int32_t> io;
    const int nclust = 1 + (int)(rng() % 3);
    std::vector<long long> centre, spread;
    for (int c = 0; c < nclust; c++) { centre.push_back((long long)(rng() % (uint64_t)(nwn * T.osamp))); spread.push_back(1 + (long long)(rng() % (uint64_t)(6 * T.osamp))); }
    for (int g = 0; g < ngroups[(size_t)b]; g++) {
      const int c = (int)(rng() % nclust);
      long long x = centre[(size_t)c] + (long long)(rng() % (uint64_t)(2 * spread[(size_t)c] + 1)) - spread[(size_t)c];
      if (rng() % 16 == 0) x = -1 - (long long)(rng() % (uint64_t)(2 * T.osamp));            // just below the band
      if (rng() % 16 == 0) x = nwn * T.osamp + (long long)(rng() % (uint64_t)(2 * T.osamp));   // just above it
      io.push_back((int32_t)std::max<long long>(x, -2LL * T.osamp));
    }
    std::sort(io.begin(), io.end(), [](int32_t a, int32_t z) { return a > z; });
    for (int32_t x : io) {
      if (!T.lines_dense) line += (int32_t)(rng() % 3);       // lines of no group (out of range) in between
      const int32_t n = 1 + (int32_t)(rng() % 3);
      T.iown.push_back(x); T.gfirst.push_back(line); T.gcount.push_back(n); line += n;
    }
    T.gblock[(size_t)b + 1] = (int32_t)T.iown.size();
  }
  const long long osamp = T.osamp, kmaxc = nwn - 1;
  for (int b = 0; b < niso; b++)
    count_ge(T.iown.data(), T.gblock[(size_t)b], T.gblock[(size_t)b + 1], nwn, [=](int32_t x) { return std::min<long long>(x / osamp, kmaxc); },
             &T.cntge[(size_t)b * (size_t)(nwn + 1)], 1);
  T.wbase.assign((size_t)niso + 1, 0);
  for (int b = 0; b < niso; b++) T.wbase[(size_t)b + 1] = T.wbase[(size_t)b] + (T.gblock[(size_t)b + 1] - T.gblock[(size_t)b] + T.ngw - 1) / T.ngw;
  return T;
}

// ---- walk_window against the plain count
static void check_window(const Tables &T, int64_t lo, int64_t hi, int Rc)
{
  const GroupView G = T.view(lo, hi);
  const WalkWindow W = walk_window(G, 2 * (Rc + 1), T.nwaves());
  n_windows++;
  if (!G.windowed || T.nwaves() == 0) { EXPECT(W.nseg == 0 && W.nw == (unsigned)T.nwaves()); return; }
  const long long c_lo = lo - Rc - 1, c_hi = hi - 1 + Rc;
  auto reach = [&](int g) { const long long c = T.cell(g); return (c >= c_lo && c <= c_hi) || (c < 0 && c_lo <= 0); };
  // the launch, range by range
  std::vector<char> launched((size_t)T.nwaves(), 0);
  EXPECT(W.nseg >= 1 && W.nseg <= kSweepSegs && W.seg_cum[0] == 0 && W.nw == (unsigned)W.seg_cum[W.nseg]);
  bool any_launched = false;
  int block_before = -1;
  for (int s = 0; s < W.nseg && s < kSweepSegs; s++) {
    const int n = W.seg_cum[s + 1] - W.seg_cum[s], w0 = W.seg_w0[s];
    EXPECT(n >= 0);
    if (n <= 0) continue;
    any_launched = true;
    int b = 0;
    while (b < T.niso && !(w0 >= T.wbase[(size_t)b] && w0 < T.wbase[(size_t)b + 1])) b++;
    EXPECT(b < T.niso && w0 + n <= T.wbase[(size_t)std::min(b, T.niso - 1) + 1]);        // one run, inside one block
    EXPECT(b > block_before);                                                             // one run per block, blocks in order
    block_before = b;
    if (b >= T.niso || w0 + n > T.nwaves()) return;
    for (int w = w0; w < w0 + n; w++) launched[(size_t)w] = 1;
  }
  bool any_reach = false;
  for (int b = 0; b < T.niso; b++) {
    const int gb0 = T.gblock[(size_t)b], gb1 = T.gblock[(size_t)b + 1];
    int first = -1, last = -1, block_reach = 0;
    for (int w = T.wbase[(size_t)b]; w < T.wbase[(size_t)b + 1]; w++) {
      const int g0 = gb0 + (w - T.wbase[(size_t)b]) * T.ngw, g1 = std::min(g0 + T.ngw, gb1);
      bool in = false, above = false, below = false;
      for (int g = g0; g < g1; g++) { in = in || reach(g); above = above || T.cell(g) > c_hi; below = below || T.cell(g) < c_lo; if (T.cell(g) < 0 && reach(g)) n_below0++; }
      if (in) { EXPECT(launched[(size_t)w]); block_reach++; }
      if (!in && above && below) { EXPECT(launched[(size_t)w]); n_straddle++; }         // it writes the zeros the combine reads
      if (launched[(size_t)w]) { if (first < 0) first = w; last = w; }
    }
    any_reach = any_reach || block_reach > 0;
    // at most one range at each end of the run holds no group in reach, and none inside
    for (int w = first; first >= 0 && w <= last; w++) {
      const int g0 = gb0 + (w - T.wbase[(size_t)b]) * T.ngw, g1 = std::min(g0 + T.ngw, gb1);
      bool in = false;
      for (int g = g0; g < g1; g++) in = in || reach(g);
      if (!in) EXPECT(w == first || w == last);
    }
  }
  if (!any_reach && !any_launched) {
    n_nothing++;
    EXPECT(W.nseg == 1 && W.seg_w0[0] == 0 && W.seg_cum[0] == 0 && W.seg_cum[1] == 0 && W.nw == 0);
  }
  if (any_reach) EXPECT(any_launched && W.nw > 0);
}

// ---- sweep_window_lines against the cell-by-cell count
static void check_lines(const Tables &T, int64_t lo, int64_t hi, std::mt19937_64 &rng)
{
  const GroupView G = T.view(lo, hi);
  const int nlayer = 1 + (int)(rng() % 6), nc = 1 + (int)(rng() % nlayer), r_top = nc - 1 + (int)(rng() % (nlayer - nc + 1));
  Heap<int32_t> psmax((size_t)nlayer * (size_t)T.niso);
  const int kind = (int)(rng() % 4);
  for (size_t i = 0; i < psmax.n; i++)
    psmax[i] = kind == 0 ? 0 : kind == 1 ? (int32_t)(rng() % (uint64_t)(T.osamp + 1)) : kind == 2 ? (int32_t)(rng() % (uint64_t)(8 * T.osamp)) : (int32_t)(rng() % (uint64_t)(70 * T.osamp));
  long long span = 0, members = 0;
  for (int b = 0; b < T.niso; b++) {
    long long psm = 0;
    for (int c = 0; c < nc; c++) psm = std::max<long long>(psm, psmax[(size_t)(r_top - c) * (size_t)T.niso + (size_t)b]);
    int ga = -1, gz = -1;
    for (int g = T.gblock[(size_t)b]; g < T.gblock[(size_t)b + 1]; g++) {
      bool in = true;
      if (G.windowed) {
        // the cell's fine-grid points are [osamp*k, osamp*k + osamp - 1]; the shard's [osamp*lo, osamp*(hi-1)] (its bins' own points)
        const long long k = T.cell(g);
        in = k >= 0 && (long long)T.osamp * k + T.osamp - 1 >= (long long)T.osamp * lo - psm && (long long)T.osamp * k <= (long long)T.osamp * (hi - 1) + psm;
      }
      if (in) { if (ga < 0) ga = g; gz = g; members += T.gcount[(size_t)g]; }
    }
    if (ga >= 0) span += (long long)T.gfirst[(size_t)gz] + T.gcount[(size_t)gz] - T.gfirst[(size_t)ga];
  }
  const long long got = sweep_window_lines(G, psmax.get(), r_top, nc);
  EXPECT(got == span);
  if (T.lines_dense) EXPECT(got == members);
}

// ---- the ladders at their boundaries
static void check_ladders()
{
  const long long rcs[7] = {0, 1, 2, 3, 4, 7, 8}; const int want[7] = {2, 4, 8, 8, 16, 16, 0};
  for (int osamp : {1, 4})
    for (int k = 0; k < 7; k++)
      for (long long psm : {rcs[k] * osamp, rcs[k] * osamp + osamp - 1}) {
        EXPECT(walk_frame_bins(true, true, psm, osamp) == want[k]);
        EXPECT(walk_frame_bins(false, true, psm, osamp) == 0 && walk_frame_bins(true, false, psm, osamp) == 0);
      }
  // 2*psm/osamp + 1 bins: 63 and 64 (osamp 1 gives odd counts only: 63 and 65)
  EXPECT(!very_wide(31, 1) && very_wide(32, 1));
  EXPECT(!very_wide(125, 4) && very_wide(126, 4) && !very_wide(0, 4));
  // wide_masks: bit c = layer r_top - c; block 1 has no groups and must not count
  const int32_t gblock[4] = {0, 3, 3, 5};
  for (int osamp : {1, 4})
    for (int nc : {1, 5, 31, 32})
      for (int pattern = 0; pattern < 4; pattern++) {
        GroupView G; G.niso = 3; G.gblock = gblock; G.osamp = osamp;
        const int nlayer = nc + 2, r_top = nc;
        Heap<int32_t> psmax((size_t)nlayer * 3);
        const long long wide_from = osamp == 1 ? 32 : 126, row_m8_from = 768, m8_from = 384;     // 2*384 + 1 = 769 >= 768 > 767
        unsigned want_wide = 0, want_m8 = 0;
        for (int c = 0; c < nc; c++) {
          const int r = r_top - c;
          const int w = pattern == 0 ? 0 : pattern == 1 ? 2 : (c * 7 + pattern) % 3;       // 0: narrow, 1: wide, 2: wide and m8
          const long long psm = w == 0 ? wide_from - 1 : w == 1 ? std::max(wide_from, m8_from - 1) : std::max(wide_from, m8_from);
          psmax[(size_t)r * 3 + 0] = (int32_t)(c % 2 ? psm : 0); psmax[(size_t)r * 3 + 2] = (int32_t)(c % 2 ? 0 : psm);
          psmax[(size_t)r * 3 + 1] = 1 << 20;
          EXPECT(layer_psmax(G, psmax.get(), r) == psm);
          if (w >= 1) want_wide |= 1u << c;
          if (w >= 1 && 2 * psm + 1 >= row_m8_from) want_m8 |= 1u << c;
        }
        const WideMasks K = wide_masks(G, psmax.get(), r_top, nc, row_m8_from);
        unsigned all = 0;
        for (int c = 0; c < nc; c++) all |= 1u << c;
        EXPECT(K.wide == want_wide && K.m8 == want_m8 && (K.m8 & ~K.wide) == 0);
        EXPECT(K.all_wide == (want_wide == all));
      }
}

// ---- walk_form over every combination of its inputs
static void check_forms()
{
  const WalkCaps caps{32, 16, 4};
  const long long nwn = 100;
  auto lanes_plain = [&](const WalkFormIn &in) {
    return in.nw > 0 && in.row_copy && in.nb >= 8 && in.nc <= 32 && in.lanes_walk && in.max_gcount <= 16 && (in.ngroups >= 8 * in.nwn || in.lanes_force);
  };
  for (unsigned nw : {0u, 5u}) for (int rowc = 0; rowc < 2; rowc++) for (int nb : {2, 4, 8, 16})
  for (int nc : {1, 2, 10, 11, 16, 21, 22, 32, 33, 64}) for (int sw = 0; sw < 8; sw++) for (int pmax : {0, 10, 32})
  for (int mg : {16, 17}) for (long long ng : {8 * nwn - 1, 8 * nwn}) {
    WalkFormIn in;
    in.nw = nw; in.row_copy = rowc; in.nb = nb; in.nc = nc; in.lanes_walk = sw & 1; in.lanes_force = sw & 2; in.packed_walk = sw & 4;
    in.packed_max_layers = pmax; in.max_gcount = mg; in.ngroups = ng; in.nwn = nwn; in.lanes_parts = nc <= 16 ? 4 : nc <= 21 ? 3 : 2;
    const WalkForm F = walk_form(in, caps);
    in.prof = true;
    const WalkForm C = walk_form(in, caps);
    in.prof = false;
    cases++;
    // one form, and only its own fields
    EXPECT(F.prod == kFormWalk || F.prod == kFormLanes || F.prod == kFormPacked);
    EXPECT(F.launched == F.prod);
    EXPECT((F.parts != 0) == (F.launched == kFormLanes) && (F.S != 0) == (F.launched == kFormPacked) && (F.packed_nb != 0) == (F.launched == kFormPacked));
    if (F.launched != kFormWalk) EXPECT(!F.per_bin);
    // lanes: exactly when all seven hold; else packed exactly when its four hold
    EXPECT((F.prod == kFormLanes) == lanes_plain(in));
    EXPECT((F.prod == kFormPacked) == (!lanes_plain(in) && nw > 0 && rowc && nc <= pmax && (sw & 4)));
    if (F.launched == kFormLanes) EXPECT(F.parts == in.lanes_parts);
    if (F.launched == kFormPacked) EXPECT(F.S >= 1 && F.S * nc <= 64 && (F.S + 1) * nc > 64 && F.packed_nb == (nb <= 4 ? 4 : nb));
    if (F.launched == kFormWalk) EXPECT(F.per_bin == (nb >= 4 && !rowc));
    // a counting run: the plain walk, per bin, booked under the production form
    EXPECT(C.prod == F.prod && C.launched == kFormWalk && C.per_bin && C.parts == 0 && C.S == 0 && C.packed_nb == 0);
  }
  // the lanes form needs every one of its seven conditions: drop one at a time
  WalkFormIn ok;
  ok.nw = 5; ok.row_copy = true; ok.nb = 8; ok.nc = 32; ok.lanes_walk = true; ok.lanes_force = false; ok.packed_walk = true; ok.packed_max_layers = 10;
  ok.max_gcount = 16; ok.ngroups = 8 * nwn; ok.nwn = nwn; ok.lanes_parts = 2;
  EXPECT(walk_form(ok, caps).prod == kFormLanes);
  for (int drop = 0; drop < 7; drop++) {
    WalkFormIn in = ok;
    if (drop == 0) in.nw = 0;
    if (drop == 1) in.row_copy = false;
    if (drop == 2) in.nb = 4;
    if (drop == 3) in.nc = 33;
    if (drop == 4) in.lanes_walk = false;
    if (drop == 5) in.max_gcount = 17;
    if (drop == 6) in.ngroups = 8 * nwn - 1;
    EXPECT(walk_form(in, caps).prod != kFormLanes);
  }
  WalkFormIn forced = ok; forced.ngroups = 0; forced.lanes_force = true;       // (the switch stands in for the density)
  EXPECT(walk_form(forced, caps).prod == kFormLanes);
}

int main(int argc, char **argv)
{
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 400;
  std::mt19937_64 rng(20263);
  for (int r = 0; r < rounds; r++, cases++) {
    const int niso = 1 + (int)(rng() % 4);
    const int64_t nwn = 8 + (int64_t)(rng() % 193);
    std::vector<int> ng((size_t)niso);
    for (int &n : ng) n = (int)(rng() % 61);
    if (niso > 1 && r % 4 != 0) ng[rng() % (uint64_t)niso] = 0;          // an empty block
    if (r % 50 == 7) for (int &n : ng) n = 0;                              // no group at all
    const Tables T = draw(rng, niso, nwn, ng);
    // the windows: whole grid, lo = 0, hi = nwn, width 1, at random, and inside the gaps between two groups of a block
    std::vector<std::pair<int64_t, int64_t>> win;
    win.push_back({0, nwn});
    win.push_back({0, 1 + (int64_t)(rng() % (uint64_t)(nwn - 1))});
    win.push_back({1 + (int64_t)(rng() % (uint64_t)(nwn - 1)), nwn});
    for (int k = 0; k < 3; k++) { const int64_t a = (int64_t)(rng() % (uint64_t)nwn); win.push_back({a, a + 1}); }
    win.push_back({0, 1}); win.push_back({nwn - 1, nwn});
    for (int k = 0; k < 3; k++) { const int64_t a = (int64_t)(rng() % (uint64_t)nwn), b = a + 1 + (int64_t)(rng() % (uint64_t)(nwn - a)); win.push_back({a, b}); }
    for (int b = 0; b < niso; b++)
      for (int g = T.gblock[(size_t)b] + 1; g < T.gblock[(size_t)b + 1]; g++) {
        const long long above = T.cell(g - 1), below = T.cell(g);
        if (below < 0 || above - below < 2) continue;
        const int64_t mid = (above + below) / 2;
        win.push_back({mid, mid + 1}); win.push_back({below + 1, above});
        if ((g - T.gblock[(size_t)b]) % T.ngw == 0) n_between++; else n_in_gap++;
      }
    for (const auto &w : win) {
      if (w.first >= w.second || (w.first == 0 && w.second == nwn && &w != &win[0])) continue;
      for (int Rc : {0, 1, 3, 7}) check_window(T, w.first, w.second, Rc);
      check_lines(T, w.first, w.second, rng);
    }
  }
  // more blocks than a launch can address: every range
  {
    std::vector<int> ng((size_t)kSweepSegs + 1, 2);
    const Tables T = draw(rng, kSweepSegs + 1, 40, ng);
    const WalkWindow W = walk_window(T.view(5, 9), 4, T.nwaves());
    EXPECT(W.nseg == 0 && W.nw == (unsigned)T.nwaves());
  }
  check_ladders();
  check_forms();
  std::printf("%d cases, %d differ\n", cases, g_bad);
  std::printf("(%ld windows: %ld ranges straddling one, %ld with nothing in reach, %ld groups below cell 0 in reach; gaps: %ld between two ranges, %ld inside one)\n",
              n_windows, n_straddle, n_nothing, n_below0, n_between, n_in_gap);
  if (!g_bad) std::printf("ok %d\n", g_checks);
  return g_bad ? 1 : 0;
}
