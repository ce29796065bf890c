// wfilter_check.cpp -- the host side and the arithmetic of the weighted detrending filter (trx_set_weighted_filter) on the
// CPU: the refusals, the layout, the extents and the per-column functions of transit_amd/csrc/trx_wfilter.h.  The same
// source the library compiles; every buffer is a heap block of EXACTLY its extent, addressed the way the kernels of
// hip/trx_wfilter.hip.h address theirs (tile by tile, lane by lane, the factor component-major), so that an index outside
// one is an error under -fsanitize=address here and not a fault on the device.
//
//   wfilter_check                 the program's own checks: the refusal table, the extents, the layout, two columns whose
//                                 result is known exactly; prints "ok N" (N checks) or FAILED lines
//   wfilter_check set FILE        FILE: "nexp ncomp nseg", the nseg + 1 segment bounds, then the doubles (C99 hex) of the
//                                 basis [nseg][nexp][ncomp], the weights [nexp][npix] and g [nexp][npix].  Runs the factor
//                                 and the filter over the whole set at every padding from the layout's up to 16 -- they
//                                 must agree in every bit -- and prints per column "col p live" and then its nfac factor
//                                 entries and its nexp values as C99 hex
#include <cstdint>
#include <cstring>

#include "trx_wfilter.h"
#include "check_common.h"

using namespace trx;

static bool same_bits(double a, double b) { return !std::memcmp(&a, &b, sizeof a) || (a != a && b != b); }

// ---- the refusal table --------------------------------------------------------------------------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get();
  Heap<double> basis(2 * 3 * 2, 0.5);
  trx_wfilter F{2, 0, basis.get()};
  ACCEPTED(wfilter_set_checks(S, &F, msg));
  Heap<double> wide(2 * 3 * TRX_FILTER_MAX, 1.0);
  trx_wfilter W{TRX_FILTER_MAX, 0, wide.get()};
  ACCEPTED(wfilter_set_checks(S, &W, msg));
  ProductState N = S; N.seg = nullptr; N.nexp = N.nseg = 0;
  trx_wfilter bad{-1, 0, nullptr};
  REFUSED(wfilter_set_checks(N, &bad, msg), TRX_E_ARG, "weighted filter: no observed set installed (trx_set_observed)");
  N = S; N.npix = 0;
  REFUSED(wfilter_set_checks(N, &bad, msg), TRX_E_ARG, "weighted filter: no observed set installed (trx_set_observed)");
  REFUSED(wfilter_set_checks(S, &bad, msg), TRX_E_ARG, "weighted filter: ncomp < 0");
  bad.ncomp = TRX_FILTER_MAX + 1;
  REFUSED(wfilter_set_checks(S, &bad, msg), TRX_E_ARG, "weighted filter: ncomp above TRX_FILTER_MAX (16)");
  bad.ncomp = 2;
  REFUSED(wfilter_set_checks(S, &bad, msg), TRX_E_ARG, "weighted filter: NULL basis array");
  for (const double x : {kNaN, kInf, -kInf}) {
    basis[0] = x;
    REFUSED(wfilter_set_checks(S, &F, msg), TRX_E_ARG, "weighted filter: segment 0: basis entry must be finite");
    basis[0] = 0.5; basis[11] = x;                       // the last entry of the last segment
    REFUSED(wfilter_set_checks(S, &F, msg), TRX_E_ARG, "weighted filter: segment 1: basis entry must be finite");
    basis[11] = 0.5;
  }
  ACCEPTED(wfilter_set_checks(S, &F, msg));
}

// ---- the extents -----------------------------------------------------------------------------------------
static void extents()
{
  WfilterExtents X = wfilter_extents(800, 7, 8, 1, 4, 16, 4);
  CHECK(X.nfac == 1 && X.blocks == 4 && X.basis_bytes == 8u * 8 * 7 * 4 && X.fac_bytes == 8u * 800 && X.live_bytes == 4u * 800);
  X = wfilter_extents(800, 7, 8, 3, 4, 17, 4);
  CHECK(X.nfac == 6 && X.blocks == 5 && X.fac_bytes == 8u * 6 * 800);
  X = wfilter_extents(81920, 100, 40, 16, 16, 1280, 4);
  CHECK(X.nfac == 136 && X.blocks == 320 && X.basis_bytes == 8u * 40 * 100 * 16 && X.fac_bytes == (size_t)8 * 136 * 81920);
  X = wfilter_extents(1, 1, 1, 9, 16, 1, 4);
  CHECK(X.nfac == 45 && X.blocks == 1 && X.fac_bytes == 8u * 45);
  for (int j = 0, e = 0; j < TRX_FILTER_MAX; j++)
    for (int k = 0; k <= j; k++, e++) CHECK(wfilter_at(j, k) == e);                // row after row, no gap: nfac entries
}

// ---- the whole set, the way the device walks it ---------------------------------------------------------
// the basis [nseg][nexp][from] padded again to [nseg][nexp][NC]
static Heap<double> repad(const std::vector<double> &basis, size_t rows, int from, int NC)
{
  Heap<double> out(rows * (size_t)NC, 0.0);
  for (size_t r = 0; r < rows; r++)
    for (int j = 0; j < from; j++) out[r * (size_t)NC + (size_t)j] = basis[r * (size_t)from + (size_t)j];
  return out;
}

// k_wfilter_factor and k_pixel_wfilter over every tile and lane: fac [nfac][npix], live [npix], val [nexp][npix]
template <int NC>
static void device_walk(const ProductState &S, const WfilterLayout &L, int ncomp, const double *weight, const double *g, double *fac, int32_t *live,
                        double *val)
{
  const Heap<double> basis = repad(L.basis, (size_t)S.nseg * (size_t)S.nexp, L.npad, NC);
  const int64_t npix = S.npix; const int nexp = S.nexp;
  for (const FilterTile &T : L.tiles)
    for (int lane = 0; lane < 64; lane++) {
      if (lane >= T.count) continue;
      const int64_t p = T.first + lane;
      const double *const U = basis.get() + (int64_t)T.seg * nexp * NC;
      const bool good = wfilter_factor_column<NC>(U, weight ? weight + p : nullptr, weight != nullptr, fac + p, npix, nexp, ncomp);
      live[p] = good ? 1 : 0;
      double y[NC];
      for (int j = 0; j < NC; j++) y[j] = 0.0;
      for (int v = 0; v < nexp; v++) wfilter_rhs_term<NC>(U + (int64_t)v * NC, weight ? weight[(int64_t)v * npix + p] : 1.0, g[(int64_t)v * npix + p], y);
      wfilter_solve<NC>(ncomp, y, fac + p, npix);
      for (int v = 0; v < nexp; v++) val[(int64_t)v * npix + p] = good ? wfilter_value<NC>(U + (int64_t)v * NC, y, g[(int64_t)v * npix + p]) : kNaN;
    }
}

struct SetResult { Heap<double> fac, val; Heap<int32_t> live; int nfac; };

// the set at every padding from the layout's up to 16: the same bits; returns the narrowest one's
static SetResult run_set(const ProductState &S, const trx_wfilter &F, const double *weight, const double *g)
{
  std::string msg;
  WfilterLayout L;
  CHECK(wfilter_set_checks(S, &F, msg) == TRX_OK && wfilter_layout(S, &F, L, msg) == TRX_OK);
  CHECK(L.npad == (F.ncomp <= 4 ? 4 : F.ncomp <= 8 ? 8 : 16));
  const WfilterExtents X = wfilter_extents(S.npix, S.nexp, S.nseg, F.ncomp, L.npad, (int64_t)L.tiles.size(), 4);
  CHECK(X.basis_bytes == sizeof(double) * L.basis.size());
  const size_t nfac = (size_t)X.nfac, npix = (size_t)S.npix, nexp = (size_t)S.nexp;
  SetResult R{Heap<double>(nfac * npix, -7.0), Heap<double>(nexp * npix, -7.0), Heap<int32_t>(npix, -7), X.nfac};
  CHECK(X.fac_bytes == sizeof(double) * R.fac.n && X.live_bytes == sizeof(int32_t) * R.live.n);
  bool first = true;
  for (const int NC : {4, 8, 16}) {
    if (NC < L.npad) continue;
    Heap<double> fac(nfac * npix, -7.0), val(nexp * npix, -7.0); Heap<int32_t> live(npix, -7);
    if (NC == 4) device_walk<4>(S, L, F.ncomp, weight, g, fac.get(), live.get(), val.get());
    else if (NC == 8) device_walk<8>(S, L, F.ncomp, weight, g, fac.get(), live.get(), val.get());
    else device_walk<16>(S, L, F.ncomp, weight, g, fac.get(), live.get(), val.get());
    if (first) {
      for (size_t k = 0; k < fac.n; k++) R.fac[k] = fac[k];
      for (size_t k = 0; k < val.n; k++) R.val[k] = val[k];
      for (size_t k = 0; k < live.n; k++) R.live[k] = live[k];
      first = false;
      continue;
    }
    bool same = true;
    for (size_t k = 0; k < fac.n; k++) same = same && same_bits(fac[k], R.fac[k]);
    for (size_t k = 0; k < val.n; k++) same = same && same_bits(val[k], R.val[k]);
    for (size_t k = 0; k < live.n; k++) same = same && live[k] == R.live[k];
    CHECK(same);                                         // (a padded component changes no bit and is no pivot)
  }
  for (size_t k = 0; k < R.live.n; k++) if (R.live[k] != 0 && R.live[k] != 1) { CHECK(R.live[k] == 0 || R.live[k] == 1); break; }   // every pixel in a tile
  return R;
}

// ---- the layout: the basis exposure-major and zero-padded, the tiles the plain filter's -------------------
static void layout()
{
  Heap<int64_t> seg{0, 1, 66, 66, 200};
  ProductState S; S.npix = 200; S.nexp = 3; S.nseg = 4; S.seg = seg.get();
  for (const int ncomp : {1, 4, 5, 8, 9, 16}) {
    Heap<double> basis((size_t)S.nseg * 3 * (size_t)ncomp);
    for (size_t k = 0; k < basis.n; k++) basis[k] = 1.0 + (double)k;
    trx_wfilter F{ncomp, 0, basis.get()};
    std::string msg; WfilterLayout L;
    CHECK(wfilter_layout(S, &F, L, msg) == TRX_OK);
    const int np = ncomp <= 4 ? 4 : ncomp <= 8 ? 8 : 16;
    CHECK(L.npad == np && L.basis.size() == (size_t)S.nseg * 3 * (size_t)np);
    bool ok = true;
    for (int s = 0; s < S.nseg; s++)
      for (int v = 0; v < 3; v++)
        for (int j = 0; j < np; j++)
          ok = ok && L.basis[((size_t)s * 3 + (size_t)v) * (size_t)np + (size_t)j] == (j < ncomp ? basis[((size_t)s * 3 + (size_t)v) * (size_t)ncomp + (size_t)j] : 0.0);
    CHECK(ok);
    // tiles of 1, 64 + 1, none, 64 + 64 + 6: every pixel once, in order, never across a segment
    CHECK(L.tiles.size() == 6);
    int64_t next = 0; ok = true;
    for (const FilterTile &T : L.tiles) {
      ok = ok && T.first == next && T.count >= 1 && T.count <= 64 && T.seg >= 0 && T.seg < S.nseg && T.first >= seg[(size_t)T.seg] &&
           T.first + T.count <= seg[(size_t)T.seg + 1];
      next = T.first + T.count;
    }
    CHECK(ok && next == S.npix);
  }
}

// ---- two sets whose results are known exactly -----------------------------------------------------------
static void known()
{
  // one component, the constant vector, weights all 1: N = D = nexp, g' = g - mean(g)
  Heap<int64_t> seg{0, 3};
  ProductState S; S.npix = 3; S.nexp = 4; S.nseg = 1; S.seg = seg.get();
  Heap<double> ones(4, 1.0);
  trx_wfilter F{1, 0, ones.get()};
  Heap<double> g{1.0, 0.0, -4.0,  2.0, 0.0, 4.0,  3.0, 0.0, -4.0,  6.0, 0.0, 4.0};       // [nexp][npix]
  SetResult R = run_set(S, F, nullptr, g.get());
  CHECK(R.nfac == 1 && R.live[0] == 1 && R.live[1] == 1 && R.live[2] == 1 && R.fac[0] == 4.0 && R.fac[2] == 4.0);
  CHECK(R.val[0] == -2.0 && R.val[3] == -1.0 && R.val[6] == 0.0 && R.val[9] == 3.0 && R.val[1] == 0.0 && R.val[2] == -4.0 && R.val[11] == 4.0);
  // weights: column 0 masked at the last exposure (the mean of the first three: 2), column 1 masked everywhere (dead),
  // column 2 one positive weight (g' = g - g at that exposure)
  Heap<double> w{1.0, 0.0, 0.0,  1.0, 0.0, 0.0,  1.0, 0.0, 0.5,  0.0, 0.0, 0.0};
  R = run_set(S, F, w.get(), g.get());
  CHECK(R.live[0] == 1 && R.live[1] == 0 && R.live[2] == 1 && R.fac[0] == 3.0 && R.fac[1] == 0.0 && R.fac[2] == 0.5);
  CHECK(R.val[0] == -1.0 && R.val[3] == 0.0 && R.val[6] == 1.0 && R.val[9] == 4.0);
  CHECK(R.val[1] != R.val[1] && R.val[10] != R.val[10]);
  CHECK(R.val[2] == 0.0 && R.val[5] == 8.0 && R.val[8] == 0.0 && R.val[11] == 8.0);
  // two components that are the same vector: the second pivot is 0 of 4 -- singular; and two orthogonal ones: both live
  Heap<double> twice{1.0, 1.0,  1.0, 1.0,  1.0, 1.0,  1.0, 1.0}, ortho{1.0, 1.0,  1.0, -1.0,  1.0, 1.0,  1.0, -1.0};
  trx_wfilter T{2, 0, twice.get()};
  R = run_set(S, T, nullptr, g.get());
  CHECK(R.nfac == 3 && R.live[0] == 0 && R.live[2] == 0 && R.fac[0] == 4.0 && R.fac[3] == 1.0 && R.fac[6] == 0.0 && R.val[0] != R.val[0]);
  T.basis = ortho.get();
  R = run_set(S, T, nullptr, g.get());
  CHECK(R.live[0] == 1 && R.fac[0] == 4.0 && R.fac[3] == 0.0 && R.fac[6] == 4.0);
  CHECK(R.val[2] == 0.0 && R.val[5] == 0.0 && R.val[8] == 0.0 && R.val[11] == 0.0);          // g of column 2 is -4 times the second vector
  // with one positive weight fewer than components: singular
  Heap<double> one{0.0, 0.0, 0.0,  0.0, 0.0, 0.0,  2.0, 2.0, 2.0,  0.0, 0.0, 0.0};
  R = run_set(S, T, one.get(), g.get());
  CHECK(R.live[0] == 0 && R.live[1] == 0 && R.live[2] == 0);
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "set")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nexp, ncomp, nseg;
    if (std::fscanf(f, "%d %d %d", &nexp, &ncomp, &nseg) != 3 || nexp < 1 || ncomp < 1 || ncomp > TRX_FILTER_MAX || nseg < 1) {
      std::fprintf(stderr, "wfilter_check: bad header\n"); return 2;
    }
    Heap<int64_t> seg((size_t)nseg + 1);
    for (int s = 0; s <= nseg; s++) {
      long long x;
      if (std::fscanf(f, "%lld", &x) != 1) { std::fprintf(stderr, "wfilter_check: bad segment bounds\n"); return 2; }
      seg[(size_t)s] = x;
    }
    const size_t npix = (size_t)seg[(size_t)nseg];
    const auto basis = read_doubles(f, (size_t)nseg * (size_t)nexp * (size_t)ncomp), w = read_doubles(f, (size_t)nexp * npix),
               g = read_doubles(f, (size_t)nexp * npix);
    std::fclose(f);
    ProductState S; S.npix = (int64_t)npix; S.nexp = nexp; S.nseg = nseg; S.seg = seg.get();
    const trx_wfilter F{ncomp, 0, basis.get()};
    const SetResult R = run_set(S, F, w.get(), g.get());
    for (size_t p = 0; p < npix; p++) {
      std::printf("col %zu %d", p, (int)R.live[p]);
      for (int e = 0; e < R.nfac; e++) std::printf(" %a", R.fac[(size_t)e * npix + p]);
      for (int v = 0; v < nexp; v++) std::printf(" %a", R.val[(size_t)v * npix + p]);
      std::printf("\n");
    }
    if (g_bad) return 1;
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: wfilter_check [set FILE]\n"); return 2; }
  refusals();
  extents();
  layout();
  known();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
