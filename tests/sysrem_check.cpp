// sysrem_check.cpp -- the host side and the arithmetic of detrending the observed set (trx_detrend_observed) on the CPU: the
// refusals, the tiles, the extents and the arithmetic functions of transit_amd/csrc/trx_sysrem.h.  The same source the
// library compiles; every buffer is a heap block of EXACTLY its extent, addressed the way the kernels of
// hip/trx_sysrem.hip.h address theirs (tile by tile and lane by lane for the column kernels, row by row and lane by lane
// for the row kernel, the lane sums through the butterfly), so that an index outside one is an error under
// -fsanitize=address here and not a fault on the device.
//
//   sysrem_check                  the program's own checks: the refusal table in the header's order, the extents, the tiles,
//                                 sets whose result is known exactly; prints "ok N" (N checks) or FAILED lines
//   sysrem_check set FILE         FILE: "nexp ncomp niter nseg hasw", the nseg + 1 segment bounds, then the doubles (C99 hex)
//                                 of the data [nexp][npix] and, with hasw = 1, the weights [nexp][npix].  Runs SYSREM over
//                                 the whole set the way the device walks it and prints "U" and its [nseg][nexp][ncomp]
//                                 entries, "coef" and its [ncomp][npix], "r" and its [nexp][npix], as C99 hex
#include <cstdint>
#include <cstring>

#include "trx_sysrem.h"
#include "check_common.h"

using namespace trx;

constexpr int kElemBlock = 256, kTileWaves = 4, kRowWaves = 4, kRowTrips = 4;      // kPixBlock, kFiltWaves, kMomWaves, kMomTrips

// ---- the refusal table, in the header's order --------------------------------------------------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get();
  const int atm = 0, opts = 0;                           // (the checks look at the addresses only)
  Heap<double> shift{1.0, 1.0, 1.0};
  trx_detrend D{2, 10, 0, 0, 0.0, 0.0};
  ACCEPTED(detrend_checks(S, &D, nullptr, nullptr, 0, nullptr, msg));
  ACCEPTED(detrend_checks(S, nullptr, nullptr, nullptr, 0, nullptr, msg));                 // the undo
  trx_detrend I{TRX_FILTER_MAX, TRX_SYSREM_MAX_ITER, 1, 0, 1e-3, 1.0};
  ACCEPTED(detrend_checks(S, &I, &atm, &opts, 3, shift.get(), msg));
  CHECK(detrend_is_undo(nullptr) && !detrend_is_undo(&D));
  // every later fault at once: the first in the order is the one named
  trx_detrend bad{-1, 0, 2, 1, kNaN, kInf};
  ProductState N = S; N.seg = nullptr; N.nexp = N.nseg = 0; N.windowed = true;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: no observed set installed (trx_set_observed)");
  REFUSED(detrend_checks(N, nullptr, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: no observed set installed (trx_set_observed)");
  N = S; N.npix = 0;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: no observed set installed (trx_set_observed)");
  N = S; N.windowed = true;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: ncomp < 0");
  bad.ncomp = TRX_FILTER_MAX + 1;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: ncomp above TRX_FILTER_MAX (16)");
  bad.ncomp = 0;                                         // the undo: nothing else is looked at
  ACCEPTED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg));
  CHECK(detrend_is_undo(&bad));
  bad.ncomp = 3;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: niter < 1");
  bad.niter = TRX_SYSREM_MAX_ITER + 1;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: niter above TRX_SYSREM_MAX_ITER (64)");
  bad.niter = 1;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: inject must be 0 or 1");
  bad.inject = -1;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: inject must be 0 or 1");
  bad.inject = 1;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: pad must be 0");
  bad.pad = 0;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: p0 must be finite");
  bad.p0 = -kInf;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: p0 must be finite");
  bad.p0 = 0.5;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: p1 must be finite");
  bad.p1 = kNaN;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: p1 must be finite");
  bad.p1 = 1.0;
  REFUSED(detrend_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: a is NULL");
  REFUSED(detrend_checks(N, &bad, &atm, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: o is NULL");
  REFUSED(detrend_checks(N, &bad, &atm, &opts, 0, nullptr, msg), TRX_E_ARG, "trx_detrend_observed: shift is NULL");
  REFUSED(detrend_checks(N, &bad, &atm, &opts, 0, shift.get(), msg), TRX_E_ARG, "trx_detrend_observed: nshift 0 is not the observed set's nexp 3");
  REFUSED(detrend_checks(N, &bad, &atm, &opts, 4, shift.get(), msg), TRX_E_ARG, "trx_detrend_observed: nshift 4 is not the observed set's nexp 3");
  for (const double x : {kNaN, kInf, 0.0, -1.0}) {
    shift[2] = x;
    REFUSED(detrend_checks(N, &bad, &atm, &opts, 3, shift.get(), msg), TRX_E_ARG, "trx_detrend_observed: shift 2 must be finite and > 0");
    shift[2] = 1.0;
  }
  shift[0] = 0.0;
  REFUSED(detrend_checks(N, &bad, &atm, &opts, 3, shift.get(), msg), TRX_E_ARG, "trx_detrend_observed: shift 0 must be finite and > 0");
  shift[0] = 1.0;
  {
    // more pairs than one pixel launch takes (no array of that size is read: the shifts are nexp)
    Heap<int64_t> wide_seg{0, 0x7fffffffLL};
    ProductState W; W.npix = 0x7fffffffLL; W.nexp = 257; W.nseg = 1; W.seg = wide_seg.get(); W.windowed = true;
    Heap<double> sh(257, 1.0);
    REFUSED(detrend_checks(W, &bad, &atm, &opts, 257, sh.get(), msg), TRX_E_ARG, "trx_detrend_observed: nshift * npix above what one launch takes");
    W.nexp = 256; W.windowed = false;
    ACCEPTED(detrend_checks(W, &bad, &atm, &opts, 256, sh.get(), msg));
  }
  // the last: a shard of the grid, with and without an injection
  REFUSED(detrend_checks(N, &bad, &atm, &opts, 3, shift.get(), msg), TRX_E_UNSUPPORTED,
          "trx_detrend_observed: this handle's shard is not the whole grid; detrend on the host (xcor.sysrem_reference)");
  REFUSED(detrend_checks(N, &D, nullptr, nullptr, 0, nullptr, msg), TRX_E_UNSUPPORTED,
          "trx_detrend_observed: this handle's shard is not the whole grid; detrend on the host (xcor.sysrem_reference)");
  ACCEPTED(detrend_checks(S, &bad, &atm, &opts, 3, shift.get(), msg));
  // without an injection a, o, shift and the p's are not looked at
  trx_detrend plain{1, 1, 0, 0, kNaN, kInf};
  ACCEPTED(detrend_checks(S, &plain, nullptr, nullptr, -5, nullptr, msg));
  // the non-finite component
  Heap<double> U(2 * 3 * 2, 0.25);
  ACCEPTED(sysrem_basis_check(U.get(), 2, 3, 2, msg));
  for (const double x : {kNaN, kInf, -kInf}) {
    U[1] = x;                                            // segment 0, exposure 0, component 1
    REFUSED(sysrem_basis_check(U.get(), 2, 3, 2, msg), TRX_E_ARG, "trx_detrend_observed: component 1 of segment 0 is not finite");
    U[1] = 0.25; U[10] = x;                              // segment 1, exposure 2, component 0
    REFUSED(sysrem_basis_check(U.get(), 2, 3, 2, msg), TRX_E_ARG, "trx_detrend_observed: component 0 of segment 1 is not finite");
    U[10] = 0.25;
  }
}

// ---- the extents and the tiles ---------------------------------------------------------------------------
static void extents()
{
  SysremExtents X = sysrem_extents(800, 7, 8, 3, 10, 16, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.cells == 5600 && X.rows == 56 && X.elem_blocks == 22 && X.tile_blocks == 4 && X.row_blocks == 14 && X.launches == 66);
  CHECK(X.r_bytes == 8u * 5600 && X.a_bytes == 8u * 56 && X.c_bytes == 8u * 800 && X.coef_bytes == 8u * 3 * 800 && X.basis_bytes == 8u * 56 * 3);
  // steps 0 and 1 alone: the same four numbers whatever the call fits
  const FillExtents F = fill_extents(800, 7, kElemBlock);
  CHECK(F.cells == X.cells && F.elem_blocks == X.elem_blocks && F.r_bytes == X.r_bytes && F.c_bytes == X.c_bytes);
  X = sysrem_extents(81920, 100, 40, 5, 10, 1280, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.cells == 8192000 && X.rows == 4000 && X.elem_blocks == 32000 && X.tile_blocks == 320 && X.row_blocks == 1000 && X.launches == 110);
  CHECK(X.r_bytes == (size_t)8 * 8192000 && X.coef_bytes == (size_t)8 * 5 * 81920 && X.basis_bytes == (size_t)8 * 4000 * 5);
  X = sysrem_extents(1, 1, 1, 1, 1, 1, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.cells == 1 && X.elem_blocks == 1 && X.tile_blocks == 1 && X.row_blocks == 1 && X.launches == 4 && X.r_bytes == 8);
  X = sysrem_extents(257, 3, 5, 16, 64, 9, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.cells == 771 && X.elem_blocks == 4 && X.tile_blocks == 3 && X.row_blocks == 4 && X.launches == 16 * 130);

  // tiles of 1, 64 + 1, none, 64 + 64 + 6: every pixel once, in order, never across a segment -- filter_layout's
  Heap<int64_t> seg{0, 1, 66, 66, 200};
  ProductState S; S.npix = 200; S.nexp = 3; S.nseg = 4; S.seg = seg.get();
  std::vector<FilterTile> tiles; std::string msg;
  CHECK(sysrem_tiles(S, tiles, msg) == TRX_OK && tiles.size() == 6);
  int64_t next = 0; bool ok = true;
  for (const FilterTile &T : tiles) {
    ok = ok && T.first == next && T.count >= 1 && T.count <= 64 && T.seg >= 0 && T.seg < S.nseg && T.first >= seg[(size_t)T.seg] &&
         T.first + T.count <= seg[(size_t)T.seg + 1];
    next = T.first + T.count;
  }
  CHECK(ok && next == S.npix);
  Heap<double> ones(4 * 3 * 2, 1.0);                   // [nseg][nexp][ncomp] of a plain filter over the same set
  const trx_filter plain{2, 0, ones.get(), ones.get()};
  FilterLayout L;
  CHECK(filter_layout(S, &plain, L, msg) == TRX_OK && L.tiles.size() == tiles.size());
  ok = true;
  for (size_t k = 0; k < tiles.size() && k < L.tiles.size(); k++)
    ok = ok && tiles[k].first == L.tiles[k].first && tiles[k].seg == L.tiles[k].seg && tiles[k].count == L.tiles[k].count;
  CHECK(ok);
}

// ---- the trip loop of trx_columns.h --------------------------------------------------------------------------
// exposure_trips<K> over a heap array of exactly nexp doubles, nexp = 1 .. 2K + 1: load sees only exposures there are (the
// array itself is read: a load outside it is a sanitizer report), use gets every exposure once, ascending, with what load
// gave for that exposure; nothing at all for nexp = 0
template <int K>
static void trips()
{
  for (int nexp = 1; nexp <= 2 * K + 1; nexp++) {
    Heap<double> col((size_t)nexp);
    for (int v = 0; v < nexp; v++) col[(size_t)v] = 100.0 + v;
    int loads = 0, uses = 0; bool inside = true, ordered = true, matched = true;
    exposure_trips<K>(
        nexp, [&](int v) { loads++; inside = inside && v >= 0 && v <= nexp - 1; return inside ? col.get()[v] : kNaN; },
        [&](int v, double x) { ordered = ordered && v == uses; matched = matched && x == 100.0 + v; uses++; });
    CHECK(inside && ordered && matched && uses == nexp && loads == (nexp + K - 1) / K * K);
  }
  int calls = 0;
  exposure_trips<K>(0, [&](int) { calls++; return 0.0; }, [&](int, double) { calls++; });
  exposure_trips<K>(-3, [&](int) { calls++; return 0.0; }, [&](int, double) { calls++; });
  CHECK(calls == 0);
}

// ---- the whole set, the way the device walks it ---------------------------------------------------------
struct SetResult { Heap<double> U, coef, r; };

// k_sysrem_cols, k_sysrem_rows, k_sysrem_close and k_sysrem_subtract over every tile, row and lane, launch after launch;
// data [nexp][npix], weight the same or null
static SetResult run_set(const ProductState &S, int ncomp, int niter, const double *data, const double *weight)
{
  std::string msg;
  std::vector<FilterTile> tiles;
  CHECK(sysrem_tiles(S, tiles, msg) == TRX_OK);
  const SysremExtents X = sysrem_extents(S.npix, S.nexp, S.nseg, ncomp, niter, (int64_t)tiles.size(), kElemBlock, kTileWaves, kRowWaves);
  const int64_t npix = S.npix; const int nexp = S.nexp, nseg = S.nseg;
  SetResult R{Heap<double>(X.basis_bytes / sizeof(double), 0.0), Heap<double>(X.coef_bytes / sizeof(double), 0.0), Heap<double>(X.r_bytes / sizeof(double))};
  Heap<double> a(X.a_bytes / sizeof(double), -7.0), c(X.c_bytes / sizeof(double), -7.0);
  double *const r = R.r.get();
  for (int64_t k = 0; k < X.cells; k++) r[k] = data[k];
  int64_t launches = 0;
  for (int i = 0; i < ncomp; i++) {
    for (int it = 0; it < niter; it++) {
      // the column step: one lane per column of a tile
      for (const FilterTile &T : tiles)
        for (int lane = 0; lane < 64; lane++) {
          if (lane >= T.count) continue;
          const int64_t p = T.first + lane;
          const double *const av = it ? a.get() + (int64_t)T.seg * nexp : nullptr;
          c[(size_t)p] = sysrem_column_step(r + p, weight ? weight + p : nullptr, weight != nullptr, av, npix, nexp);
        }
      launches++;
      // the row step: one wave per (v, s), lane sums over trips of 64 pixels, then the butterfly
      for (int64_t row = 0; row < X.rows; row++) {
        const int64_t v = row / nseg, s = row - v * nseg;
        const int64_t first = S.seg[s], last = S.seg[s + 1], base = v * npix;
        double num[64], den[64];
        for (int l = 0; l < 64; l++) num[l] = den[l] = 0.0;
        for (int64_t p0 = first; p0 < last; p0 += 64 * kRowTrips)
          for (int t = 0; t < kRowTrips; t++)
            for (int lane = 0; lane < 64; lane++) {
              const int64_t q = p0 + 64 * t + lane;
              const bool in = q < last;
              const int64_t p = in ? q : last - 1;         // (a lane past the end reads the last pixel again)
              const double rr = r[base + p], ww = weight ? weight[base + p] : 1.0, cc = c[(size_t)p];
              if (in) sysrem_row_term(ww, rr, cc, num[lane], den[lane]);
            }
        a[(size_t)(s * nexp + v)] = sysrem_ratio(sysrem_wave_sum_host(num), sysrem_wave_sum_host(den));
      }
      launches++;
    }
    // the close: every tile computes its segment's norm, the segment's first tile writes U
    for (const FilterTile &T : tiles) {
      const double *const av = a.get() + (int64_t)T.seg * nexp;
      const double t = sysrem_norm(av, nexp);
      for (int lane = 0; lane < 64; lane++) {
        if (T.first == S.seg[T.seg])
          for (int v = lane; v < nexp; v += 64) R.U[(size_t)(((int64_t)T.seg * nexp + v) * ncomp + i)] = sysrem_close_a(av[v], t);
        if (lane >= T.count) continue;
        const int64_t p = T.first + lane;
        R.coef[(size_t)((int64_t)i * npix + p)] = sysrem_close_c(c[(size_t)p], t);
      }
    }
    launches++;
    for (const FilterTile &T : tiles)
      for (int lane = 0; lane < 64; lane++) {
        if (lane >= T.count) continue;
        const int64_t p = T.first + lane;
        sysrem_column_subtract(r + p, R.U.get() + (int64_t)T.seg * nexp * ncomp + i, ncomp, R.coef[(size_t)((int64_t)i * npix + p)], npix, nexp);
      }
    launches++;
  }
  CHECK(launches == X.launches);
  return R;
}

// ---- results known exactly ----------------------------------------------------------------------------------
static void known()
{
  // the injection: F (p0 g + p1) where b > 0, F's bits elsewhere
  CHECK(sysrem_inject(3.0, 1.0, 2.0, 4.0, 0.5, 1.0) == 6.0);
  CHECK(sysrem_inject(3.0, 1.0, 0.0, 4.0, 0.5, 1.0) == 3.0 && sysrem_inject(3.0, 1.0, -2.0, 4.0, 0.5, 1.0) == 3.0);
  CHECK(sysrem_inject(-0.7, 5.0, 3.0, 1.1, 0.0, 1.0) == -0.7);
  const double nan_b = sysrem_inject(3.0, 1.0, kNaN, 4.0, 0.5, 1.0);
  CHECK(nan_b == 3.0);
  CHECK(sysrem_ratio(1.0, 0.0) == 0.0 && sysrem_ratio(1.0, -2.0) == 0.0 && sysrem_ratio(1.0, kNaN) == 0.0 && sysrem_ratio(3.0, 2.0) == 1.5);
  CHECK(!std::signbit(sysrem_ratio(-1.0, 0.0)));
  // the butterfly: 0 + 1 + ... + 63, and a sum whose order shows: lane 0 holds 1, lane 32 holds 2^53, lane 1 holds 1
  double lanes[64];
  for (int l = 0; l < 64; l++) lanes[l] = (double)l;
  CHECK(sysrem_wave_sum_host(lanes) == 2016.0);
  for (int l = 0; l < 64; l++) lanes[l] = 0.0;
  lanes[0] = 1.0; lanes[32] = 0x1p53; lanes[1] = 1.0;
  CHECK(sysrem_wave_sum_host(lanes) == 0x1p53);         // (1 + 2^53 rounds to 2^53 first; 1 + 1 first would give 2^53 + 2)

  // one segment, four equal rows (2, 4, 8): c = the row, a = 1, t = 2: U = 1/2, coef = (4, 8, 16), r = 0 exactly
  Heap<int64_t> seg{0, 3};
  ProductState S; S.npix = 3; S.nexp = 4; S.nseg = 1; S.seg = seg.get();
  Heap<double> data{2.0, 4.0, 8.0,  2.0, 4.0, 8.0,  2.0, 4.0, 8.0,  2.0, 4.0, 8.0};
  for (const int niter : {1, 3}) {
    SetResult R = run_set(S, 1, niter, data.get(), nullptr);
    CHECK(R.U[0] == 0.5 && R.U[1] == 0.5 && R.U[2] == 0.5 && R.U[3] == 0.5);
    CHECK(R.coef[0] == 4.0 && R.coef[1] == 8.0 && R.coef[2] == 16.0);
    bool zero = true;
    for (size_t k = 0; k < R.r.n; k++) zero = zero && R.r[k] == 0.0;
    CHECK(zero);
  }
  // a second component on residuals of exact zeros: c = 0, then the row step's den = 0: vectors +0, the residuals stay
  SetResult R2 = run_set(S, 2, 2, data.get(), nullptr);
  CHECK(R2.U[0] == 0.5 && R2.U[1] == 0.0 && R2.U[3] == 0.0 && R2.coef[3] == 0.0 && R2.coef[5] == 0.0 && R2.r[0] == 0.0);
  // masked everywhere: zero vectors, the data as they were
  Heap<double> w0(12, 0.0);
  SetResult R0 = run_set(S, 2, 2, data.get(), w0.get());
  bool same = true, zero = true;
  for (size_t k = 0; k < R0.r.n; k++) same = same && R0.r[k] == data[k];
  for (size_t k = 0; k < R0.U.n; k++) zero = zero && R0.U[k] == 0.0 && !std::signbit(R0.U[k]);
  for (size_t k = 0; k < R0.coef.n; k++) zero = zero && R0.coef[k] == 0.0;
  CHECK(same && zero);
  // an exposure masked over the whole segment: its a_v is +0, its residuals stay; the others as without it
  Heap<double> w1{1.0, 1.0, 1.0,  0.0, 0.0, 0.0,  1.0, 1.0, 1.0,  1.0, 1.0, 1.0};
  Heap<double> d1{2.0, 4.0, 8.0,  5.0, 6.0, 7.0,  2.0, 4.0, 8.0,  2.0, 4.0, 8.0};
  SetResult R1 = run_set(S, 1, 2, d1.get(), w1.get());
  CHECK(R1.U[1] == 0.0 && !std::signbit(R1.U[1]) && R1.r[3] == 5.0 && R1.r[4] == 6.0 && R1.r[5] == 7.0);
  CHECK(R1.U[0] == 1.0 / std::sqrt(3.0) && R1.U[2] == R1.U[0] && R1.U[3] == R1.U[0]);
  // an empty segment between two: zero vectors, nothing of it read or written
  Heap<int64_t> seg3{0, 3, 3, 6};
  ProductState E; E.npix = 6; E.nexp = 4; E.nseg = 3; E.seg = seg3.get();
  Heap<double> d3(24);
  for (int v = 0; v < 4; v++) for (int p = 0; p < 6; p++) d3[(size_t)(v * 6 + p)] = data[(size_t)(v * 3 + p % 3)];
  SetResult R3 = run_set(E, 1, 2, d3.get(), nullptr);
  CHECK(R3.U[0] == 0.5 && R3.U[4] == 0.0 && R3.U[7] == 0.0 && R3.U[8] == 0.5 && R3.coef[3] == 4.0 && R3.coef[5] == 16.0);
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "set")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nexp, ncomp, niter, nseg, hasw;
    if (std::fscanf(f, "%d %d %d %d %d", &nexp, &ncomp, &niter, &nseg, &hasw) != 5 || nexp < 1 || ncomp < 1 || ncomp > TRX_FILTER_MAX || niter < 1 ||
        niter > TRX_SYSREM_MAX_ITER || nseg < 1) {
      std::fprintf(stderr, "sysrem_check: bad header\n"); return 2;
    }
    Heap<int64_t> seg((size_t)nseg + 1);
    for (int s = 0; s <= nseg; s++) {
      long long x;
      if (std::fscanf(f, "%lld", &x) != 1) { std::fprintf(stderr, "sysrem_check: bad segment bounds\n"); return 2; }
      seg[(size_t)s] = x;
    }
    const size_t npix = (size_t)seg[(size_t)nseg];
    const auto data = read_doubles(f, (size_t)nexp * npix);
    std::unique_ptr<double[]> w;
    if (hasw) w = read_doubles(f, (size_t)nexp * npix);
    std::fclose(f);
    ProductState S; S.npix = (int64_t)npix; S.nexp = nexp; S.nseg = nseg; S.seg = seg.get();
    const trx_detrend D{ncomp, niter, 0, 0, 0.0, 0.0};
    std::string msg;
    if (detrend_checks(S, &D, nullptr, nullptr, 0, nullptr, msg) != TRX_OK) { std::fprintf(stderr, "sysrem_check: %s\n", msg.c_str()); return 2; }
    const SetResult R = run_set(S, ncomp, niter, data.get(), w.get());
    print_doubles("U", R.U); print_doubles("coef", R.coef); print_doubles("r", R.r);
    if (g_bad) return 1;
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: sysrem_check [set FILE]\n"); return 2; }
  refusals();
  extents();
  trips<4>();
  trips<8>();
  CHECK(kSysTrips == 8 && kFiltTrips == 4);
  known();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
