// table_check -- the Voigt table's plan and the layouts of its copies (transit_amd/csrc/trx_table.h) on the CPU.
//   table_check grid <ndop> <nlor> <dmin> <dmax> <lmin> <lmax> <timesalpha> <wn_d> <osamp> <nown>
//     prints the plan of that grid -- "total", then "adop", "alor" (hex floats), "psize", "poff", one line each -- for
//     the caller to compare with the oracle's table;
//   table_check <rounds>
//     seeded random grids (2..64 widths each way, osamp of 1, 2, 4, 24, 2160; widths and the profile reach drawn so that
//     rows of at most 8, of 9..16 and of more entries and alias entries all occur -- a class that never occurred fails
//     the check).  Per grid:
//       * the profiles tile [0, tab_n) in job order; first_bin is the offset;
//       * an alias entry (the rule is restated here) has psize, poff, job, walk descriptor and compact offset of the
//         entry a Doppler row above it; job_of counts the other entries in row-major order;
//       * in each derived layout the rows of distinct jobs are disjoint and inside the total;
//       * a walk row is a whole number of 16-float lines, `front` zeros ahead of its K entries and at least as many
//         behind; centre4 = 4 (row 0 + front + ps / osamp), inside the row; psr = ps % osamp; rowb = 4 stride;
//       * a compact row exists exactly when K <= 8; compact offsets are distinct multiples of 32 bytes below the slab;
//       * psizeT is the transpose, psize_mono what a direct scan says;
//       * index_steps: nearest_index(thr[k]) == k and k - 1 for the double just below; a look-up through the
//         thresholds == nearest_index at every grid point, midpoint, their neighbours (and on 10^5 random values for
//         every tenth grid); a grid with a repeated or a decreasing value is rejected.
//     Once: the predicates that switch a copy off fire exactly at their limits; the allocation size is what it is made of.
//   Prints "<cases> cases, <bad> differ".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include "trx_table.h"

using namespace trx;

struct TableGrid {      // the grid fields of trx_static, with its types
  int32_t ndop = 0, nlor = 0;
  float dmin = 0, dmax = 0, lmin = 0, lmax = 0, timesalpha = 0;
  double wn_d = 0; int32_t osamp = 1; int64_t nown = 0;
};

static int bad = 0, cases = 0;
#define EXPECT(cond) \
  do { if (!(cond)) { if (bad++ < 20) std::printf("case %d: %s (line %d)\n", cases, #cond, __LINE__); } } while (0)

static int print_grid(char **a)
{
  TableGrid g;
  g.ndop = std::atoi(a[0]); g.nlor = std::atoi(a[1]);
  g.dmin = (float)std::strtod(a[2], nullptr); g.dmax = (float)std::strtod(a[3], nullptr);
  g.lmin = (float)std::strtod(a[4], nullptr); g.lmax = (float)std::strtod(a[5], nullptr);
  g.timesalpha = (float)std::strtod(a[6], nullptr); g.wn_d = std::strtod(a[7], nullptr);
  g.osamp = std::atoi(a[8]); g.nown = std::atoll(a[9]);
  TablePlan P; const char *text = "";
  if (plan_table(g, P, &text) != kTablePlanOk) { std::printf("error %s\n", text); return 1; }
  std::printf("total %lld\nadop", (long long)P.tab_n);
  for (int i = 0; i < g.ndop; i++) std::printf(" %a", P.adop[i]);
  std::printf("\nalor");
  for (int i = 0; i < g.nlor; i++) std::printf(" %a", P.alor[i]);
  std::printf("\npsize");
  for (int32_t v : P.psize) std::printf(" %d", v);
  std::printf("\npoff");
  for (long long v : P.poff) std::printf(" %lld", v);
  std::printf("\n");
  return 0;
}

// the look-up the thresholds stand for: the number of steps at or below v
static int lookup(const std::vector<double> &thr, int n, double v)
{ return (int)(std::upper_bound(thr.begin() + 1, thr.begin() + n, v) - (thr.begin() + 1)); }

static void check_steps(const std::vector<double> &grid, int n, std::mt19937_64 &rng, bool many)
{
  std::vector<double> thr;
  EXPECT(index_steps(grid.data(), n, thr));
  if ((int)thr.size() != n + 1) { EXPECT(!"thr has n + 1 entries"); return; }
  EXPECT(thr[0] == -HUGE_VAL && thr[n] == HUGE_VAL);
  auto same = [&](double v) { EXPECT(lookup(thr, n, v) == nearest_index(grid.data(), v, 0, n)); };
  for (int k = 1; k < n; k++) {
    EXPECT(nearest_index(grid.data(), thr[k], 0, n) == k);
    EXPECT(nearest_index(grid.data(), std::nextafter(thr[k], 0.0), 0, n) == k - 1);
  }
  for (int k = 0; k < n; k++) {
    const double pts[2] = {grid[k], k + 1 < n ? 0.5 * (grid[k] + grid[k + 1]) : 2 * grid[k]};
    for (double p : pts) { same(p); same(std::nextafter(p, 0.0)); same(std::nextafter(p, HUGE_VAL)); }
  }
  same(0.0); same(-1.0); same(grid[0] / 3); same(grid[n - 1] * 3);
  if (many) {
    std::uniform_real_distribution<double> u(std::log(grid[0] / 10), std::log(grid[n - 1] * 10));
    for (int i = 0; i < 100000; i++) same(std::exp(u(rng)));
  }
  // a repeated and a decreasing value
  std::vector<double> g2(grid), out;
  const int k = 1 + (int)(rng() % (unsigned)(n - 1));
  g2[k] = g2[k - 1];
  EXPECT(!index_steps(g2.data(), n, out));
  g2[k] = std::nextafter(g2[k - 1], 0.0);
  EXPECT(!index_steps(g2.data(), n, out));
}

static void check_limits()
{
  const long long pad2 = 2 * (long long)kTabPad;
  EXPECT(walk_rows_fit((1LL << 30) - pad2 - 1) && !walk_rows_fit((1LL << 30) - pad2));
  EXPECT(!compact_rows_fit(0, 0, 4) && compact_rows_fit(1, 32, 4));
  EXPECT(compact_rows_fit((1LL << 19) - 1, 8 * ((1LL << 19) - 1), 1) && !compact_rows_fit(1LL << 19, 8 * (1LL << 19), 1));      // slab below 2^24 bytes
  EXPECT(compact_rows_fit(1, 8LL * ((1 << 24) - 1), (1 << 24) - 1) && !compact_rows_fit(1, 8LL * (1 << 24), 1 << 24));          // osamp below 2^24
  EXPECT(compact_rows_fit(1, (1LL << 30) - 1, 4) && !compact_rows_fit(1, 1LL << 30, 4));                                          // the whole below 4 GB
  const size_t fixed = 2 * (size_t)kTabPad + (size_t)kRowTail;
  EXPECT(table_alloc_floats(1000, 4) == 1000 + fixed + (size_t)kWalkMaxFrame * 4);
  EXPECT(table_alloc_floats(7, 1 << 21) == 7 + fixed + (size_t)kWalkMaxFrame * (1 << 21));
  EXPECT(table_alloc_floats(7, (1 << 21) + 1) == 7 + fixed + (size_t)kWalkMaxFrame * (1 << 21));
}

// rows of distinct jobs: [off[j], off[j] + len[j]) in job order, no overlap, inside total (len 0: the job has no row)
static void check_disjoint(const std::vector<long long> &off, const std::vector<long long> &len, long long total)
{
  long long at = 0;
  for (size_t j = 0; j < off.size(); j++) {
    if (!len[j]) continue;
    EXPECT(off[j] >= at);
    at = off[j] + len[j];
  }
  EXPECT(at <= total);
}

int main(int argc, char **argv)
{
  if (argc == 12 && !std::strcmp(argv[1], "grid")) return print_grid(argv + 2);
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
  std::mt19937_64 rng(20262);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int osamps[5] = {1, 2, 4, 24, 2160};
  long long n_class[3] = {0, 0, 0}, n_alias = 0, n_planned = 0;
  check_limits();
  for (int r = 0; r < rounds; r++, cases++) {
    TableGrid g;
    g.ndop = 2 + (int)(rng() % 63); g.nlor = 2 + (int)(rng() % 63);
    g.osamp = osamps[rng() % 5];
    g.dmin = (float)std::pow(10.0, -4 + 3 * U(rng)); g.dmax = (float)(g.dmin * std::pow(10.0, 0.3 + 2.7 * U(rng)));
    g.lmin = (float)std::pow(10.0, -5 + 4 * U(rng)); g.lmax = (float)(g.lmin * std::pow(10.0, 0.3 + 3.7 * U(rng)));
    g.wn_d = std::pow(10.0, -2 + 2.3 * U(rng));
    g.timesalpha = (float)std::pow(10.0, 0.2 + 2.2 * U(rng));
    g.nown = (20 + (int64_t)(rng() % 5000)) * g.osamp + 1;
    TablePlan P; const char *text = nullptr;
    const TablePlanError pe = plan_table(g, P, &text);
    if (pe != kTablePlanOk) { EXPECT(pe == kTablePlanUnsupported && text && std::strstr(text, "sub-sampling")); continue; }
    n_planned++;
    const int nd = g.ndop, nl = g.nlor, os = g.osamp;
    const size_t ne = (size_t)nd * nl;
    EXPECT(P.adop.size() == (size_t)nd + 1 && P.alor.size() == (size_t)nl + 1 && P.adop[nd] == HUGE_VAL && P.alor[nl] == HUGE_VAL);
    EXPECT(P.psize.size() == ne && P.poff.size() == ne && P.job_of.size() == ne && P.psizeT.size() == ne);
    // the profiles tile the table
    long long at = 0;
    for (const ProfileJob &J : P.jobs) { EXPECT(J.off == at && J.first_bin == at && (J.nv & 1) && J.nv >= 3); at += J.nv; }
    EXPECT(at == P.tab_n);
    const PhaseMajorLayout T = phase_major_layout(P, os);
    const WalkLayout W = walk_layout(P, os);
    const CompactLayout C = compact_layout(P, os);
    EXPECT(T.joffT.size() == P.jobs.size() && W.joffW.size() == P.jobs.size() && C.joff32.size() == P.jobs.size());
    EXPECT(T.poffT.size() == ne && W.prof.size() == ne && C.c32.size() == ne);
    // entries: aliases and the others
    int32_t next_job = 0; bool mono = true;
    std::set<uint32_t> offs32;
    for (int i = 0; i < nd; i++)
      for (int k = 0; k < nl; k++) {
        const size_t e = (size_t)i * nl + k;
        const bool alias = P.adop[i] * 10.0 < P.alor[k] && i != 0;          // opacity.c:262-265, restated
        EXPECT(P.psizeT[(size_t)k * nd + i] == P.psize[e]);
        if (i > 0 && P.psize[e] < P.psize[e - nl]) mono = false;
        const WalkProfile &D = W.prof[e];
        if (alias) {
          n_alias++;
          const size_t u = e - nl;
          EXPECT(P.psize[e] == P.psize[u] && P.poff[e] == P.poff[u] && P.job_of[e] == P.job_of[u] && T.poffT[e] == T.poffT[u]);
          EXPECT(D.centre4 == W.prof[u].centre4 && D.rowb == W.prof[u].rowb && D.psr == W.prof[u].psr && D.ps == W.prof[u].ps);
          EXPECT(C.c32[e] == C.c32[u]);
          continue;
        }
        EXPECT(P.job_of[e] == next_job);
        if (P.job_of[e] != next_job || (size_t)next_job >= P.jobs.size()) { next_job++; continue; }
        const ProfileJob &J = P.jobs[(size_t)next_job];
        const long long ps = P.psize[e], K = (2 * ps) / os + 1;
        n_class[K <= 8 ? 0 : K <= 16 ? 1 : 2]++;
        EXPECT(J.nv == 2 * ps + 1 && J.off == P.poff[e] && T.poffT[e] == T.joffT[(size_t)next_job]);
        int front, stride; walk_row_layout((int)K, front, stride);
        EXPECT(stride % 16 == 0 && front > 0 && stride - front - K >= front);
        const long long row0 = W.joffW[(size_t)next_job], centre = row0 + front + ps / os;
        EXPECT(D.centre4 == (uint32_t)(4 * centre) && centre >= row0 + front && centre < row0 + front + K);
        EXPECT(D.psr == ps % os && D.rowb == 4 * stride && D.ps == ps);
        EXPECT((C.c32[e] != 0xffffffffu) == (K <= 8) && (C.joff32[(size_t)next_job] >= 0) == (K <= 8));
        if (K <= 8) {
          EXPECT(C.c32[e] % 32 == 0 && C.c32[e] < 32 * C.nq && C.c32[e] == 4 * C.joff32[(size_t)next_job]);
          EXPECT(offs32.insert(C.c32[e]).second);
        }
        next_job++;
      }
    EXPECT((size_t)next_job == P.jobs.size() && (long long)offs32.size() == C.nq && C.tot32 == C.nq * 8 * os);
    EXPECT(P.psize_mono == mono);
    // rows of distinct jobs
    std::vector<long long> lenT(P.jobs.size()), lenW(P.jobs.size()), len32(P.jobs.size());
    for (size_t j = 0; j < P.jobs.size(); j++) {
      const int K = (P.jobs[j].nv - 1) / os + 1;
      int front, stride; walk_row_layout(K, front, stride);
      lenT[j] = (long long)os * K; lenW[j] = (long long)os * stride; len32[j] = K <= 8 ? 8 : 0;
    }
    check_disjoint(T.joffT, lenT, T.totT);
    check_disjoint(W.joffW, lenW, W.totW);
    check_disjoint(C.joff32, len32, 8 * C.nq);
    check_steps(P.adop, nd, rng, r % 10 == 0);
    check_steps(P.alor, nl, rng, r % 10 == 5);
  }
  if (rounds >= 200) {
    EXPECT(n_class[0] > 0 && n_class[1] > 0 && n_class[2] > 0 && n_alias > 0);
    EXPECT(2 * n_planned >= rounds);
  }
  std::printf("rows: %lld of at most 8, %lld of 9..16, %lld wider; %lld aliases; %lld of %d grids planned\n", n_class[0], n_class[1], n_class[2],
              n_alias, n_planned, rounds);
  std::printf("%d cases, %d differ\n", cases, bad);
  return bad != 0;
}
