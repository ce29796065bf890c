// regress_check.cpp -- the host side and the arithmetic of regressing the observed set on given time vectors
// (trx_regress_observed) on the CPU: the refusals, the extents, the merge of the two bases and regress_column of
// transit_amd/csrc/trx_regress.h.  The same source the library compiles; every buffer is a heap block of EXACTLY its extent,
// addressed the way k_wfilter_factor and k_regress_cols address theirs (tile by tile and lane by lane, the factor
// component-major, the data in place), so that an index outside one is an error under -fsanitize=address here and not a
// fault on the device.
//
//   regress_check               the program's own checks: the refusal table in the header's order, the extents and the
//                               grid guard, the merge, sets whose result is known; prints "ok N" (N checks) or FAILED lines
//   regress_check set FILE      FILE: "nexp nseg hasw nvec nc" (nc: the padded component count to run with, 0: the smallest
//                               of 4, 8 and 16 that holds nvec), the nseg + 1 segment bounds, then the doubles (C99 hex) of
//                               the vectors [nseg][nexp][nvec], the data [nexp][npix] and, with hasw = 1, the weights
//                               [nexp][npix].  Runs the two kernels over the whole set the way the device walks it and
//                               prints "coef" and its [nvec][npix] entries, "data" and its [nexp][npix] as C99 hex, and
//                               "nsingular N"
#include <cstdint>
#include <cstring>

#include "trx_regress.h"
#include "check_common.h"

using namespace trx;

// ---- the refusal table, in the header's order ------------------------------------------------------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get();
  const std::string who = "trx_regress_observed: ";
  const std::string none = who + "no observed set installed (trx_set_observed)";
  Heap<double> vec((size_t)2 * 3 * 16, 0.5);               // [nseg][nexp][nvec] for every nvec up to 16
  const double shift[3] = {1.0, 1.0, 1.0}, bad_shift[3] = {1.0, -1.0, 1.0};
  const int a = 0, o = 0;                                  // (stand-ins: the checks look at the pointers alone)
  CHECK(sizeof(trx_regress) == 40);
  const trx_regress ok{3, 0, 0, 0, 0.0, 0.0, vec.get()};
  ACCEPTED(regress_checks(S, &ok, nullptr, nullptr, 0, nullptr, msg));       // (nfit = 0: niter is not read; no injection: nothing of it)
  const trx_regress okfit{3, 2, 10, 1, 0.5, 1.0, vec.get()};
  ACCEPTED(regress_checks(S, &okfit, &a, &o, 3, shift, msg));
  const trx_regress most{14, 2, 64, 0, kNaN, kNaN, vec.get()};
  ACCEPTED(regress_checks(S, &most, nullptr, nullptr, 0, nullptr, msg));
  ACCEPTED(regress_checks(S, nullptr, nullptr, nullptr, 0, nullptr, msg));   // the undo
  const trx_regress undo{0, -1, 0, 2, kNaN, kNaN, nullptr};                   // nvec = 0: the undo, nothing else read
  ACCEPTED(regress_checks(S, &undo, nullptr, nullptr, 0, nullptr, msg));
  CHECK(regress_is_undo(nullptr) && regress_is_undo(&undo) && !regress_is_undo(&ok));

  // every later fault at once: the first in the order is the one named
  trx_regress b{-1, -1, 0, 2, kNaN, kNaN, nullptr};
  ProductState N;                                          // no pixel set, no observed set
  REFUSED(regress_checks(N, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, none.c_str());
  REFUSED(regress_checks(N, nullptr, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, none.c_str());
  N.npix = 6;                                              // a pixel set alone
  REFUSED(regress_checks(N, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, none.c_str());
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "nvec < 0").c_str());
  b.nvec = 17;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "nvec above TRX_FILTER_MAX (16)").c_str());
  b.nvec = 3;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "nfit < 0").c_str());
  b.nfit = 14;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "nvec + nfit above TRX_FILTER_MAX (16)").c_str());
  b.nfit = 13;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "niter < 1").c_str());
  b.niter = 65;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "niter above TRX_SYSREM_MAX_ITER (64)").c_str());
  b.niter = 64;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "NULL vectors array").c_str());
  b.nfit = 0; b.niter = -5;                                // (nfit = 0: niter is not read)
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "NULL vectors array").c_str());
  b.vectors = vec.get();
  for (const double x : {kNaN, kInf, -kInf}) {
    vec[(size_t)1 * 3 * 3 + 4] = x;                        // segment 1 of [2][3][3]
    REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "segment 1: vectors entry must be finite").c_str());
    vec[0] = x;                                            // and segment 0: the first one is named
    REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "segment 0: vectors entry must be finite").c_str());
    vec[0] = 0.5; vec[(size_t)1 * 3 * 3 + 4] = 0.5;
  }
  vec[(size_t)2 * 3 * 3] = kNaN;                           // (past [nseg][nexp][nvec] of nvec = 3: not looked at)
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "inject must be 0 or 1").c_str());
  vec[(size_t)2 * 3 * 3] = 0.5;
  b.inject = 1;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "p0 must be finite").c_str());
  b.p0 = 0.5; b.p1 = kInf;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "p1 must be finite").c_str());
  b.p1 = 1.0;
  REFUSED(regress_checks(S, &b, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "a is NULL").c_str());
  REFUSED(regress_checks(S, &b, &a, nullptr, 0, nullptr, msg), TRX_E_ARG, (who + "o is NULL").c_str());
  REFUSED(regress_checks(S, &b, &a, &o, 0, nullptr, msg), TRX_E_ARG, (who + "shift is NULL").c_str());
  REFUSED(regress_checks(S, &b, &a, &o, 2, shift, msg), TRX_E_ARG, (who + "nshift 2 is not the observed set's nexp 3").c_str());
  REFUSED(regress_checks(S, &b, &a, &o, 3, bad_shift, msg), TRX_E_ARG, (who + "shift 1 must be finite and > 0").c_str());
  ACCEPTED(regress_checks(S, &b, &a, &o, 3, shift, msg));
  // a shard: after every argument
  ProductState W = S; W.windowed = true;
  const std::string shard = who + "this handle's shard is not the whole grid; detrend on the host (xcor.regress_reference)";
  REFUSED(regress_checks(W, &ok, nullptr, nullptr, 0, nullptr, msg), TRX_E_UNSUPPORTED, shard.c_str());
  REFUSED(regress_checks(W, &b, &a, &o, 3, shift, msg), TRX_E_UNSUPPORTED, shard.c_str());
  REFUSED(regress_checks(W, &b, &a, &o, 2, shift, msg), TRX_E_ARG, (who + "nshift 2 is not the observed set's nexp 3").c_str());
  ACCEPTED(regress_checks(W, nullptr, nullptr, nullptr, 0, nullptr, msg));   // (the undo moves buffers alone)
}

// ---- the extents, the grid guard and the merge -------------------------------------------------------------
static void extents()
{
  RegressExtents X = regress_extents(800, 7, 8, 3, 2, 15, 4);
  CHECK(X.ncomp == 5 && X.cells == 5600 && X.tile_blocks == 4 && X.grid_ok);
  CHECK(X.r_bytes == 8u * 5600 && X.coef_bytes == 8u * 5 * 800 && X.coef_fit_bytes == 8u * 3 * 800 && X.basis_bytes == 8u * 8 * 7 * 5);
  X = regress_extents(81920, 100, 40, 3, 0, 1280, 4);
  CHECK(X.ncomp == 3 && X.cells == 8192000 && X.tile_blocks == 320 && X.grid_ok && X.r_bytes == (size_t)8 * 8192000 && X.coef_bytes == X.coef_fit_bytes);
  X = regress_extents(1, 1, 1, 1, 0, 1, 4);
  CHECK(X.cells == 1 && X.tile_blocks == 1 && X.grid_ok && X.coef_bytes == 8 && X.basis_bytes == 8);
  // the 32-bit grid guard: a launch of no block, or of more blocks than a grid's x extent takes, is not made
  CHECK(!regress_extents(5, 3, 1, 1, 0, 0, 4).grid_ok);
  CHECK(regress_extents(5, 1, 1, 1, 0, (int64_t)0x7fffffffLL * 4, 4).grid_ok && !regress_extents(5, 1, 1, 1, 0, (int64_t)0x7fffffffLL * 4 + 1, 4).grid_ok);
  // sizes past 32 bits stay whole
  X = regress_extents((int64_t)1 << 31, 3, 1, 16, 0, (int64_t)1 << 25, 4);
  CHECK(X.cells == (int64_t)3 << 31 && X.r_bytes == (size_t)24 << 31 && X.coef_bytes == (size_t)128 << 31 && X.grid_ok);
  CHECK(kRegressTrips == 4);

  // the merge: the given vectors ahead of the fitted ones, exposure by exposure
  Heap<double> given{1, 2, 3, 4, 5, 6, 7, 8}, fit{10, 20, 30, 40};             // [2][2][2] and [2][2][1]
  Heap<double> out((size_t)2 * 2 * 3, -7.0);
  regress_merge(given.get(), fit.get(), 2, 2, 2, 1, out.get());
  const double want[12] = {1, 2, 10, 3, 4, 20, 5, 6, 30, 7, 8, 40};
  bool same = true;
  for (int k = 0; k < 12; k++) same = same && out[(size_t)k] == want[k];
  CHECK(same);
  Heap<double> out0((size_t)8, -7.0);
  regress_merge(given.get(), nullptr, 2, 2, 2, 0, out0.get());              // (no fitted component: fit is not read)
  same = true;
  for (int k = 0; k < 8; k++) same = same && out0[(size_t)k] == given[(size_t)k];
  CHECK(same);
}

// ---- the whole set, the way the device walks it ---------------------------------------------------------
struct SetResult { Heap<double> coef, data; int64_t nsingular; };

static int pad_of(int nvec) { return nvec <= 4 ? 4 : nvec <= 8 ? 8 : 16; }

// k_wfilter_factor<NC> and k_regress_cols<NC> over every tile and lane; vec [nseg][nexp][nvec], data [nexp][npix], weight
// the same or null
template <int NC>
static SetResult run_set(const ProductState &S, int nvec, const double *vec, const double *data, const double *weight)
{
  std::string msg;
  std::vector<FilterTile> tiles;
  CHECK(sysrem_tiles(S, tiles, msg, "regress_check") == TRX_OK);
  const RegressExtents X = regress_extents(S.npix, S.nexp, S.nseg, nvec, 0, (int64_t)tiles.size(), 4);
  const WfilterExtents WX = wfilter_extents(S.npix, S.nexp, S.nseg, nvec, NC, (int64_t)tiles.size(), 4);
  CHECK(X.grid_ok && nvec >= 1 && nvec <= NC);
  const int64_t npix = S.npix; const int nexp = S.nexp;
  // the padded vectors [nseg][nexp][NC]: what wfilter_layout gives the device
  Heap<double> U(WX.basis_bytes / sizeof(double), 0.0);
  for (int s = 0; s < S.nseg; s++)
    for (int v = 0; v < nexp; v++)
      for (int j = 0; j < nvec; j++) U[((size_t)s * nexp + v) * NC + j] = vec[((size_t)s * nexp + v) * nvec + j];
  Heap<double> fac(WX.fac_bytes / sizeof(double), 0.0);
  Heap<int32_t> live(WX.live_bytes / sizeof(int32_t), 0);
  SetResult R{Heap<double>(X.coef_bytes / sizeof(double), -7.0), Heap<double>(X.r_bytes / sizeof(double)), 0};
  for (size_t k = 0; k < R.data.n; k++) R.data[k] = data[k];           // (steps 0 and 1 left f0 in the call's buffer)
  for (int64_t blk = 0; blk < X.tile_blocks; blk++)
    for (int wave = 0; wave < 4; wave++) {
      const int64_t tile = blk * 4 + wave;
      if (tile >= (int64_t)tiles.size()) continue;
      const FilterTile &T = tiles[(size_t)tile];
      for (int lane = 0; lane < 64; lane++) {
        if (lane >= T.count) continue;
        const int64_t p = T.first + lane;
        const double *const Us = U.get() + (int64_t)T.seg * nexp * NC;
        // the factor kernel: row after row of the normal matrix and of the factor
        live[(size_t)p] = wfilter_factor_column<NC>(Us, weight ? weight + p : nullptr, weight != nullptr, fac.get() + p, npix, nexp, nvec) ? 1 : 0;
      }
    }
  // (the device has every factor before the first fit: two launches)
  for (int64_t blk = 0; blk < X.tile_blocks; blk++)
    for (int wave = 0; wave < 4; wave++) {
      const int64_t tile = blk * 4 + wave;
      if (tile >= (int64_t)tiles.size()) continue;
      const FilterTile &T = tiles[(size_t)tile];
      for (int lane = 0; lane < 64; lane++) {
        if (lane >= T.count) continue;
        const int64_t p = T.first + lane;
        regress_column<NC>(U.get() + (int64_t)T.seg * nexp * NC, weight ? weight + p : nullptr, weight != nullptr, R.data.get() + p, fac.get() + p, live[(size_t)p] != 0,
                           R.coef.get() + p, npix, nexp, nvec);
      }
    }
  for (int64_t p = 0; p < npix; p++) R.nsingular += live[(size_t)p] ? 0 : 1;
  return R;
}

static SetResult run_set_nc(int nc, const ProductState &S, int nvec, const double *vec, const double *data, const double *weight)
{
  if (nc == 4) return run_set<4>(S, nvec, vec, data, weight);
  if (nc == 8) return run_set<8>(S, nvec, vec, data, weight);
  return run_set<16>(S, nvec, vec, data, weight);
}

static bool same_bits(const Heap<double> &a, const Heap<double> &b) { return a.n == b.n && std::memcmp(a.get(), b.get(), a.n * sizeof(double)) == 0; }

// ---- results known exactly ----------------------------------------------------------------------------------
static void known()
{
  // two segments of 2 and 3 columns, 5 exposures (one more than a trip), vectors 1 and t with t = -2 .. 2; the data are exact
  // combinations with small integers, so every sum is exact: the coefficients are the integers, the residuals +0
  Heap<int64_t> seg{0, 2, 5};
  ProductState S; S.npix = 5; S.nexp = 5; S.nseg = 2; S.seg = seg.get();
  Heap<double> vec((size_t)2 * 5 * 2);
  for (int s = 0; s < 2; s++)
    for (int v = 0; v < 5; v++) { vec[((size_t)s * 5 + v) * 2] = 1.0; vec[((size_t)s * 5 + v) * 2 + 1] = (s ? 2.0 : 1.0) * (v - 2); }
  const double c0[5] = {3.0, -1.0, 0.0, 8.0, 2.0}, c1[5] = {1.0, 4.0, -2.0, 0.0, 0.5};
  Heap<double> data((size_t)25), w((size_t)25, 1.0);
  for (int v = 0; v < 5; v++)
    for (int p = 0; p < 5; p++) data[(size_t)v * 5 + p] = c0[p] + c1[p] * (p >= 2 ? 2.0 : 1.0) * (v - 2);
  w[(size_t)1 * 5 + 0] = 0.0;                              // a dead entry: its residual is computed all the same
  w[(size_t)2 * 5 + 3] = 2.0;                              // (at t = 0: the normal matrix stays diagonal)
  for (const int nc : {4, 8, 16}) {
    const SetResult R = run_set_nc(nc, S, 2, vec.get(), data.get(), w.get());
    bool same = R.nsingular == 0;
    for (int p = 0; p < 5; p++) same = same && R.coef[(size_t)p] == c0[p] && R.coef[(size_t)5 + p] == c1[p];
    for (size_t k = 0; k < 25; k++) same = same && R.data[k] == 0.0;
    CHECK(same);
  }
  // (segment 1's slope vector is twice segment 0's: a walk that took segment 0's vectors everywhere would have given its
  // columns twice their slope coefficient above)
  // singular columns: masked everywhere, live at one exposure (fewer than the two vectors): c = +0, r keeps f0's bits
  Heap<double> ws((size_t)25, 1.0);
  for (int v = 0; v < 5; v++) { ws[(size_t)v * 5 + 1] = 0.0; ws[(size_t)v * 5 + 4] = v == 2 ? 1.0 : 0.0; }
  data[(size_t)2 * 5 + 1] = -0.0;
  {
    const SetResult R = run_set_nc(4, S, 2, vec.get(), data.get(), ws.get());
    bool same = R.nsingular == 2;
    for (const int p : {1, 4}) {
      same = same && R.coef[(size_t)p] == 0.0 && !std::signbit(R.coef[(size_t)p]) && R.coef[(size_t)5 + p] == 0.0 && !std::signbit(R.coef[(size_t)5 + p]);
      for (int v = 0; v < 5; v++) same = same && std::memcmp(&R.data[(size_t)v * 5 + p], &data[(size_t)v * 5 + p], sizeof(double)) == 0;
    }
    for (const int p : {0, 2, 3}) same = same && R.coef[(size_t)p] == c0[p] && R.coef[(size_t)5 + p] == c1[p];
    CHECK(same);
  }
  // a duplicate vector in segment 0 alone: its two columns are singular, segment 1's are fitted
  Heap<double> dup((size_t)2 * 5 * 2);
  for (size_t k = 0; k < dup.n; k++) dup[k] = vec[k];
  for (int v = 0; v < 5; v++) dup[(size_t)v * 2 + 1] = 1.0;
  {
    const SetResult R = run_set_nc(8, S, 2, dup.get(), data.get(), w.get());
    bool same = R.nsingular == 2;
    for (const int p : {0, 1}) {
      same = same && R.coef[(size_t)p] == 0.0 && R.coef[(size_t)5 + p] == 0.0;
      for (int v = 0; v < 5; v++) same = same && std::memcmp(&R.data[(size_t)v * 5 + p], &data[(size_t)v * 5 + p], sizeof(double)) == 0;
    }
    for (const int p : {2, 3, 4}) same = same && R.coef[(size_t)p] == c0[p] && R.coef[(size_t)5 + p] == c1[p];
    CHECK(same);
  }
  // without weights: weights of 1
  {
    Heap<double> ones((size_t)25, 1.0);
    const SetResult A = run_set_nc(4, S, 2, vec.get(), data.get(), nullptr), B = run_set_nc(4, S, 2, vec.get(), data.get(), ones.get());
    CHECK(same_bits(A.coef, B.coef) && same_bits(A.data, B.data) && A.nsingular == 0 && B.nsingular == 0);
  }
  // exposure counts about a trip: 1, 3, 4, 5, 8 and 9 exposures of one vector, the weighted mean of the column
  for (const int nexp : {1, 3, 4, 5, 8, 9}) {
    Heap<int64_t> seg1{0, 1};
    ProductState C; C.npix = 1; C.nexp = nexp; C.nseg = 1; C.seg = seg1.get();
    Heap<double> one((size_t)nexp, 1.0), col((size_t)nexp);
    double sum = 0.0;
    for (int v = 0; v < nexp; v++) { col[(size_t)v] = (double)(v * v); sum += col[(size_t)v]; }
    const SetResult R = run_set_nc(4, C, 1, one.get(), col.get(), nullptr);
    bool same = R.nsingular == 0 && R.coef[0] == sum / nexp;
    for (int v = 0; v < nexp; v++) same = same && R.data[(size_t)v] == col[(size_t)v] - sum / nexp;
    CHECK(same);
  }
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "set")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nexp, nseg, hasw, nvec, nc;
    if (std::fscanf(f, "%d %d %d %d %d", &nexp, &nseg, &hasw, &nvec, &nc) != 5 || nexp < 1 || nseg < 1 || nvec < 1 || nvec > TRX_FILTER_MAX ||
        (nc != 0 && nc != 4 && nc != 8 && nc != 16) || (nc != 0 && nc < nvec)) {
      std::fprintf(stderr, "regress_check: bad header\n"); return 2;
    }
    Heap<int64_t> seg((size_t)nseg + 1);
    for (int s = 0; s <= nseg; s++) {
      long long x;
      if (std::fscanf(f, "%lld", &x) != 1) { std::fprintf(stderr, "regress_check: bad segment bounds\n"); return 2; }
      seg[(size_t)s] = x;
    }
    const size_t npix = (size_t)seg[(size_t)nseg];
    const auto vec = read_doubles(f, (size_t)nseg * (size_t)nexp * (size_t)nvec);
    const auto data = read_doubles(f, (size_t)nexp * npix);
    std::unique_ptr<double[]> w;
    if (hasw) w = read_doubles(f, (size_t)nexp * npix);
    std::fclose(f);
    ProductState S; S.npix = (int64_t)npix; S.nexp = nexp; S.nseg = nseg; S.seg = seg.get();
    const trx_regress rg{nvec, 0, 0, 0, 0.0, 0.0, vec.get()};
    std::string msg;
    if (regress_checks(S, &rg, nullptr, nullptr, 0, nullptr, msg) != TRX_OK) { std::fprintf(stderr, "regress_check: %s\n", msg.c_str()); return 2; }
    const SetResult R = run_set_nc(nc ? nc : pad_of(nvec), S, nvec, vec.get(), data.get(), w.get());
    print_doubles("coef", R.coef); print_doubles("data", R.data);
    std::printf("nsingular %lld\n", (long long)R.nsingular);
    if (g_bad) return 1;
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: regress_check [set FILE]\n"); return 2; }
  refusals();
  extents();
  known();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
