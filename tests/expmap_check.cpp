// expmap_check.cpp -- the host side of the Kp-Vsys map under the exposure table (trx_run_exposed_map) on the CPU:
// exposed_map_checks, the spans, bases and row arrays, the index -> row transform and exposed_map_extents
// (transit_amd/csrc/trx_expmap.h), with vmap_track and vmap_nearest (transit_amd/csrc/trx_vmap.h) for the tracks.  The same
// source the library compiles; every buffer is a heap block of EXACTLY its extent, so that an index outside one is an error
// under -fsanitize=address here and not a fault on the device.
//
//   expmap_check                  the program's own checks: the refusal table, the hand cases of spans, bases, R and the
//                                 row arrays, the transform walked the way k_cell_rows and the cell kernels address their
//                                 buffers, the extents at the caps; prints "ok N" (N checks) or FAILED lines
//   expmap_check rows FILE        FILE: "nlag nkp nvsys nexp has_offset", then the doubles (C99 hex) of lag_kms [nlag], kp
//                                 [nkp], vsys [nvsys], orbit [nexp] and (has_offset) offset [nexp]; prints "lo hi base" of
//                                 every exposure, one per line, then "R"
#include <cstdint>
#include <cstring>

#include "trx_expmap.h"
#include "check_common.h"

using namespace trx;

// ---- the refusal table: a filtered map's refusals under this call's name, then no table ---------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.lo = 0; S.hi = 5000; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get();
  S.filter = true; S.exposures = true;
  const char *who = "trx_run_exposed_map";
  Heap<double> out(1), lag{0.9999, 1.0, 1.0001}, kms{-3.0, 0.0, 3.0}, kp{100.0, 150.0}, vsys{-5.0, 0.0, 5.0, 10.0}, orbit{0.1, 0.2, 0.3}, offset{0.0, 0.5, 1.0};
  auto good = [&]() { trx_vmap V{}; V.stat = TRX_STAT_CCF; V.nlag = 3; V.lag = lag.get(); V.lag_kms = kms.get(); V.nkp = 2; V.nvsys = 4; V.kp = kp.get(); V.vsys = vsys.get();
                      V.orbit = orbit.get(); V.offset = offset.get(); return V; };
  trx_vmap V = good();
  ACCEPTED(exposed_map_checks(S, who, &V, out.get(), msg));
  V.offset = nullptr; V.stat = TRX_STAT_CHI2;
  ACCEPTED(exposed_map_checks(S, who, &V, out.get(), msg));
  REFUSED(exposed_map_checks(S, "trx_run_batch_exposed_map", nullptr, nullptr, msg), TRX_E_ARG, "trx_run_batch_exposed_map: vm is NULL");
  // a filtered map's refusals come first, in its order: everything below is wrong as well, and neither a filter nor a table is installed
  ProductState U = S; U.filter = false; U.exposures = false;
  trx_vmap bad{}; bad.stat = 9; bad.p0 = kNaN;
  ProductState W = U; W.windowed = true;
  REFUSED(exposed_map_checks(W, who, &bad, nullptr, msg), TRX_E_UNSUPPORTED,
          "trx_run_exposed_map: this handle's shard is not the whole grid; take trx_run_pixels, add the ranks' pairs (trx_gather_host) and reduce them on the host");
  ProductState N = U; N.seg = nullptr; N.nexp = N.nseg = 0;
  REFUSED(exposed_map_checks(N, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_exposed_map: no observed set installed (trx_set_observed)");
  REFUSED(exposed_map_checks(U, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_exposed_map: nlag < 1");
  bad.nlag = 3;
  REFUSED(exposed_map_checks(U, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_exposed_map: lag is NULL");
  bad.lag = lag.get();
  REFUSED(exposed_map_checks(U, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_exposed_map: map is NULL");
  lag[1] = -1.0;
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: lag 1 must be finite and > 0");
  lag[1] = 1.0;
  ProductState B = U; B.npix = 0x7fffffffLL;
  bad.nlag = 257;
  REFUSED(exposed_map_checks(B, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: nlag * npix above what one pixel launch takes");
  B = U; B.nexp = 32768; B.nseg = 32768;
  REFUSED(exposed_map_checks(B, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: nlag * nexp * nseg above 2^31 - 1");
  bad.nlag = 3;
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: unknown stat 9");
  bad.stat = TRX_STAT_CHI2;
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: nkp < 1 or nvsys < 1");
  bad.nkp = 65536; bad.nvsys = 32768;
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: nkp * nvsys above 2^31 - 1");
  bad.nkp = 2; bad.nvsys = 4;
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: lag_kms is NULL");
  bad.lag_kms = kms.get();
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: kp is NULL");
  bad.kp = kp.get();
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: vsys is NULL");
  bad.vsys = vsys.get();
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: orbit is NULL");
  bad.orbit = orbit.get();
  REFUSED(exposed_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: p0 must be finite");
  V = good();
  orbit[2] = kNaN; kms[1] = kNaN;
  REFUSED(exposed_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: orbit 2 must be finite");
  orbit[2] = 0.3;
  REFUSED(exposed_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: lag_kms 1 must be finite and above the one before it (strictly increasing)");
  kms[1] = 0.0;
  // then no filter, then the index table's size, then -- its own -- no table
  REFUSED(exposed_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: no filter installed (trx_set_filter)");
  ProductState T = S; T.exposures = false;
  REFUSED(exposed_map_checks(T, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: no exposure table installed (trx_set_exposures)");
  REFUSED(exposed_map_checks(T, "trx_run_batch_exposed_map", &V, out.get(), msg), TRX_E_ARG, "trx_run_batch_exposed_map: no exposure table installed (trx_set_exposures)");
  Heap<double> longkp(32768, 100.0), longvs(21846, 0.0);
  V.nkp = 32768; V.kp = longkp.get(); V.nvsys = 21846; V.vsys = longvs.get();
  REFUSED(exposed_map_checks(T, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_exposed_map: nkp * nvsys * nexp above 2^31 - 1");
  V.nvsys = 21845;
  ACCEPTED(exposed_map_checks(S, who, &V, out.get(), msg));
}

// ---- a case walked whole: spans, bases, R, the row arrays and the transform over exact-size buffers -------------------
// index: [cells][nexp]; want_span: [nexp][2]; want_base: [nexp]; scale / smear: the table's arrays, or absent (n == 0)
static void walk(const Heap<int32_t> &index, int64_t cells, int32_t nexp, int32_t nlag, int64_t npix, const Heap<int32_t> &want_span, const Heap<int64_t> &want_base,
                 int64_t want_R, bool with_scale, bool with_smear)
{
  const char *who = "trx_run_exposed_map";
  CHECK(index.n == (size_t)cells * (size_t)nexp && want_span.n == 2 * (size_t)nexp && want_base.n == (size_t)nexp);
  Heap<int32_t> span(2 * (size_t)nexp, -7);
  exposed_map_spans(index.get(), cells, nexp, span.get());
  for (size_t k = 0; k < span.n; k++) CHECK(span[k] == want_span[k]);
  // the lane order of k_cell_spans gives the same spans: lane l takes the cells l, l + 64, ..., then the lanes are merged
  {
    Heap<int32_t> lo(64 * (size_t)nexp, kSpanEmptyLo), hi(64 * (size_t)nexp, kSpanEmptyHi);
    for (int32_t v = 0; v < nexp; v++)
      for (int lane = 0; lane < 64; lane++)
        for (int64_t c = lane; c < cells; c += 64) {
          const int32_t *idx = index.get() + c * nexp;
          if (index_row_outside(idx, nexp)) continue;
          span_take(lo[(size_t)v * 64 + lane], hi[(size_t)v * 64 + lane], idx[v]);
        }
    for (int32_t v = 0; v < nexp; v++) {
      int32_t a = kSpanEmptyLo, z = kSpanEmptyHi;
      for (int lane = 63; lane >= 0; lane--) { a = lo[(size_t)v * 64 + lane] < a ? lo[(size_t)v * 64 + lane] : a; z = hi[(size_t)v * 64 + lane] > z ? hi[(size_t)v * 64 + lane] : z; }
      CHECK(a == span[2 * (size_t)v] && z == span[2 * (size_t)v + 1]);
    }
  }
  ExposedMapRows L;
  ACCEPTED(exposed_map_bases(who, span.get(), nexp, nlag, L, msg));
  CHECK(L.R == want_R && L.base.size() == (size_t)nexp + 1 && L.base[(size_t)nexp] == want_R);
  for (int32_t v = 0; v < nexp; v++) CHECK(L.base[(size_t)v] == want_base[(size_t)v]);
  Heap<double> lag((size_t)nlag), scale((size_t)nexp), smear((size_t)nexp);
  for (int32_t l = 0; l < nlag; l++) lag[(size_t)l] = 1.0 + 1e-5 * l;
  for (int32_t v = 0; v < nexp; v++) { scale[(size_t)v] = 10.0 + v; smear[(size_t)v] = 1e-6 * (v + 1); }
  ACCEPTED(exposed_map_row_arrays(who, span.get(), nexp, lag.get(), with_scale ? scale.get() : nullptr, with_smear ? smear.get() : nullptr, L, msg));
  CHECK(L.shift.size() == (size_t)want_R && L.scale.size() == (with_scale ? (size_t)want_R : 0) && L.smear.size() == (with_smear ? (size_t)want_R : 0));
  ExposedMapExtents X;
  ACCEPTED(exposed_map_extents(who, L.R, npix, cells, nexp, X, msg));
  CHECK(X.rows == want_R && X.pairs == want_R * npix && X.pair_bytes == 16 * (size_t)(want_R * npix));
  CHECK(X.span_bytes == 8 * (size_t)nexp && X.row_bytes == 4 * (size_t)cells * (size_t)nexp);
  CHECK(X.span_blocks * kCellSpanWaves >= nexp && (X.span_blocks - 1) * kCellSpanWaves < nexp && X.span_lanes == 64 * (int64_t)nexp);
  // the pixel launch: row r of [R][npix] is (lag l, exposure v) -- tagged 1000 l + v -- with that row's shift, scale and smear
  Heap<double> G(X.pair_bytes / sizeof(double) / 2, -1.0);
  Heap<int32_t> seen((size_t)want_R, 0);
  for (int32_t v = 0; v < nexp; v++)
    for (int64_t l = span[2 * (size_t)v]; l <= span[2 * (size_t)v + 1]; l++) {
      const int64_t r = L.base[(size_t)v] + (l - span[2 * (size_t)v]);
      CHECK(r >= 0 && r < want_R);
      seen[(size_t)r]++;
      CHECK(L.shift[(size_t)r] == lag[(size_t)l]);
      if (with_scale) CHECK(L.scale[(size_t)r] == scale[(size_t)v]);
      if (with_smear) CHECK(L.smear[(size_t)r] == smear[(size_t)v]);
      for (int64_t p = 0; p < npix; p++) G[(size_t)(r * npix + p)] = 1000.0 * (double)l + v;
    }
  for (int64_t r = 0; r < want_R; r++) CHECK(seen[(size_t)r] == 1);      // (every row is one pair, no pair twice)
  // k_cell_rows: one lane per (cell, exposure), the last block ragged; then a cell kernel's reads through the row table
  Heap<int32_t> row(X.row_bytes / sizeof(int32_t), -7);
  const int64_t ntracks = cells * nexp, blocks = (ntracks + kCellTrackBlock - 1) / kCellTrackBlock;
  for (int64_t b = 0; b < blocks; b++)
    for (int t = 0; t < kCellTrackBlock; t++) {
      const int64_t k = b * kCellTrackBlock + t;
      if (k >= ntracks) continue;
      const int64_t v = k % nexp;
      row[(size_t)k] = exposed_map_row(index[(size_t)k], span[2 * (size_t)v], span[2 * (size_t)v + 1], L.base[(size_t)v]);
    }
  for (int64_t c = 0; c < cells; c++) {
    const bool outside = index_row_outside(index.get() + c * nexp, nexp);
    CHECK(outside == index_row_outside(row.get() + c * nexp, nexp));      // (the cell kernels leave out the same cells)
    for (int32_t v = 0; v < nexp; v++) {
      const int32_t r = row[(size_t)(c * nexp + v)], k = index[(size_t)(c * nexp + v)];
      CHECK(r >= -1 && r < want_R);
      if (k < 0) CHECK(r == -1);
      if (outside) continue;
      CHECK(r >= 0);
      for (int64_t p = 0; p < npix; p++) CHECK(G[(size_t)((int64_t)r * npix + p)] == 1000.0 * k + v);
    }
  }
}

static void hand_cases()
{
  const int32_t E = kSpanEmptyLo, H = kSpanEmptyHi;
  // one cell: every span is one lag
  walk(Heap<int32_t>{2, 0, 4}, 1, 3, 5, 3, Heap<int32_t>{2, 2, 0, 0, 4, 4}, Heap<int64_t>{0, 1, 2}, 3, true, true);
  // three cells, the second outside at exposure 1: its lags 4 and 0 at the other exposures widen no span, and are no row
  walk(Heap<int32_t>{1, 2, 3, 4, -1, 0, 3, 2, 1}, 3, 3, 5, 2, Heap<int32_t>{1, 3, 2, 2, 1, 3}, Heap<int64_t>{0, 3, 4}, 7, true, false);
  // all cells outside: R = 0, no row, every transform -1
  walk(Heap<int32_t>{-1, 2, 1, -1, -1, -1}, 2, 3, 4, 5, Heap<int32_t>{E, H, E, H, E, H}, Heap<int64_t>{0, 0, 0}, 0, false, true);
  // a span of one lag at every exposure although the cells differ elsewhere; one exposure
  walk(Heap<int32_t>{3, 0, 3, 1, 3, 2}, 3, 2, 4, 1, Heap<int32_t>{3, 3, 0, 2}, Heap<int64_t>{0, 1}, 4, false, true);
  walk(Heap<int32_t>{6, 2, 4}, 3, 1, 7, 2, Heap<int32_t>{2, 6}, Heap<int64_t>{0}, 5, true, true);
  // nlag = 1: lag 0 or outside
  walk(Heap<int32_t>{0, 0, 0, -1, 0, 0}, 3, 2, 1, 4, Heap<int32_t>{0, 0, 0, 0}, Heap<int64_t>{0, 1}, 2, true, true);
  // more cells than one wave's lanes, more tracks than one block: cell c takes the lags (c % 11, 10 - c % 11, 5)
  {
    const int64_t cells = 300; const int32_t nexp = 3;
    Heap<int32_t> idx((size_t)cells * nexp);
    for (int64_t c = 0; c < cells; c++) { idx[(size_t)(c * 3)] = (int32_t)(c % 11); idx[(size_t)(c * 3 + 1)] = 10 - (int32_t)(c % 11); idx[(size_t)(c * 3 + 2)] = c % 7 == 3 ? -1 : 5; }
    // (the cells with c % 11 == 0 and c % 7 == 3 are outside, others with c % 11 == 0 are not: the spans are whole)
    walk(idx, cells, nexp, 11, 2, Heap<int32_t>{0, 10, 0, 10, 5, 5}, Heap<int64_t>{0, 11, 22}, 23, true, true);
  }
  // an exposure without a span among exposures with one (spans as read back): it has no row, and the bases step over it
  {
    const char *who = "trx_run_exposed_map";
    Heap<int32_t> span{1, 3, E, H, 0, 0};
    Heap<double> lag{1.0, 1.1, 1.2, 1.3}, scale{5.0, 6.0, 7.0};
    ExposedMapRows L;
    ACCEPTED(exposed_map_bases(who, span.get(), 3, 4, L, msg));
    CHECK(L.R == 4 && L.base[0] == 0 && L.base[1] == 3 && L.base[2] == 3 && L.base[3] == 4);
    ACCEPTED(exposed_map_row_arrays(who, span.get(), 3, lag.get(), scale.get(), nullptr, L, msg));
    CHECK(L.shift.size() == 4 && L.smear.empty() && L.scale.size() == 4);
    CHECK(L.shift[0] == 1.1 && L.shift[1] == 1.2 && L.shift[2] == 1.3 && L.shift[3] == 1.0);
    CHECK(L.scale[0] == 5.0 && L.scale[2] == 5.0 && L.scale[3] == 7.0);
    CHECK(exposed_map_row(2, E, H, 3) == -1 && exposed_map_row(-1, 1, 3, 0) == -1 && exposed_map_row(0, 1, 3, 0) == -1 && exposed_map_row(4, 1, 3, 0) == -1);
    CHECK(exposed_map_row(1, 1, 3, 0) == 0 && exposed_map_row(3, 1, 3, 0) == 2 && exposed_map_row(0, 0, 0, 3) == 3);
    CHECK(span_count(E, H) == 0 && span_count(0, 0) == 1 && span_count(0, 0x7ffffffe) == 0x7fffffffLL);
    // spans the device cannot have written
    Heap<int32_t> wrong{1, 4, 0, 0, 0, 0};
    REFUSED(exposed_map_bases(who, wrong.get(), 3, 4, L, msg), TRX_E_HIP, "trx_run_exposed_map: internal: exposure 0: a span outside the lag grid");
    wrong[1] = 0;
    REFUSED(exposed_map_bases(who, wrong.get(), 3, 4, L, msg), TRX_E_HIP, "trx_run_exposed_map: internal: exposure 0: a span outside the lag grid");
    wrong[0] = 0; wrong[2] = -1; wrong[3] = 2;
    REFUSED(exposed_map_bases(who, wrong.get(), 3, 4, L, msg), TRX_E_HIP, "trx_run_exposed_map: internal: exposure 1: a span outside the lag grid");
  }
}

// ---- the extents at the caps ------------------------------------------------------------------------
static void extents()
{
  const char *who = "trx_run_exposed_map";
  ExposedMapExtents X;
  static_assert(kExposedMapPairBytes == (uint64_t)1 << 33, "the numbers below are worked for this cap");
  static_assert(kPixBlock == 256, "the numbers below are worked for this block");
  // a small cap: 4 rows of 3 pixels are 192 bytes
  ACCEPTED(exposed_map_extents(who, 4, 3, 10, 7, X, msg, 192));
  CHECK(X.rows == 4 && X.pairs == 12 && X.pair_bytes == 192 && X.span_bytes == 56 && X.row_bytes == 280 && X.span_blocks == 2);
  REFUSED(exposed_map_extents(who, 4, 3, 10, 7, X, msg, 191), TRX_E_ARG,
          "trx_run_exposed_map: R = 4 rows of 3 pixels are 192 bytes of pairs, above kExposedMapPairBytes (191)");
  ACCEPTED(exposed_map_extents(who, 0, 3, 10, 7, X, msg, 0));                    // no row is above no cap
  CHECK(X.rows == 0 && X.pairs == 0 && X.pair_bytes == 0);
  // at the cap: 2^19 rows of 2^10 pixels are 2^33 bytes; one pixel more in a row is above it, and so is a cap one byte short
  ACCEPTED(exposed_map_extents(who, 1 << 19, 1 << 10, 143, 100, X, msg));
  CHECK(X.pairs == (int64_t)1 << 29 && X.pair_bytes == (size_t)1 << 33);
  REFUSED(exposed_map_extents(who, 1 << 19, (1 << 10) + 1, 143, 100, X, msg), TRX_E_ARG,
          "trx_run_exposed_map: R = 524288 rows of 1025 pixels are 8598323200 bytes of pairs, above kExposedMapPairBytes (8589934592)");
  REFUSED(exposed_map_extents(who, (1 << 19) + 1, 1 << 10, 143, 100, X, msg), TRX_E_ARG,
          "trx_run_exposed_map: R = 524289 rows of 1024 pixels are 8589950976 bytes of pairs, above kExposedMapPairBytes (8589934592)");
  REFUSED(exposed_map_extents(who, 1 << 19, 1 << 10, 143, 100, X, msg, kExposedMapPairBytes - 1), TRX_E_ARG,
          "trx_run_exposed_map: R = 524288 rows of 1024 pixels are 8589934592 bytes of pairs, above kExposedMapPairBytes (8589934591)");
  // the launch: 2^31 - 1 blocks of 256 pairs, and R an int32 count of rows
  const uint64_t none = std::numeric_limits<uint64_t>::max();
  ACCEPTED(exposed_map_extents(who, 0x7fffffffLL, 256, 1, 1, X, msg, none));
  CHECK(X.pairs == 0x7fffffffLL * 256 && X.pair_bytes == (size_t)0x7fffffffLL * 4096);
  REFUSED(exposed_map_extents(who, 0x7fffffffLL, 257, 1, 1, X, msg, none), TRX_E_ARG, "trx_run_exposed_map: R * npix above what one pixel launch takes");
  REFUSED(exposed_map_extents(who, 0x80000000LL, 1, 1, 1, X, msg, none), TRX_E_ARG, "trx_run_exposed_map: R * npix above what one pixel launch takes");
  REFUSED(exposed_map_extents(who, -1, 1, 1, 1, X, msg, none), TRX_E_ARG, "trx_run_exposed_map: R * npix above what one pixel launch takes");
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "rows")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nlag, nkp, nvsys, nexp, has_offset;
    if (std::fscanf(f, "%d %d %d %d %d", &nlag, &nkp, &nvsys, &nexp, &has_offset) != 5 || nlag < 1 || nkp < 1 || nvsys < 1 || nexp < 1) {
      std::fprintf(stderr, "expmap_check: bad header\n"); return 2;
    }
    const auto kms = read_doubles(f, (size_t)nlag), kp = read_doubles(f, (size_t)nkp), vsys = read_doubles(f, (size_t)nvsys), orbit = read_doubles(f, (size_t)nexp);
    const auto offset = read_doubles(f, has_offset ? (size_t)nexp : 0);
    std::fclose(f);
    // k_cell_tracks, one (cell, exposure) after the other
    const int64_t cells = (int64_t)nkp * nvsys;
    Heap<int32_t> index((size_t)cells * (size_t)nexp), span(2 * (size_t)nexp);
    for (int64_t k = 0; k < cells * nexp; k++) {
      const int64_t cell = k / nexp, v = k - cell * nexp;
      index[(size_t)k] = vmap_nearest(kms.get(), nlag, vmap_track(kp[(size_t)(cell / nvsys)], vsys[(size_t)(cell % nvsys)], orbit[(size_t)v], has_offset ? offset.get() : nullptr, v));
    }
    exposed_map_spans(index.get(), cells, nexp, span.get());
    ExposedMapRows L; std::string msg;
    if (exposed_map_bases("expmap_check", span.get(), nexp, nlag, L, msg)) { std::fprintf(stderr, "%s\n", msg.c_str()); return 1; }
    for (int v = 0; v < nexp; v++) std::printf("%d %d %lld\n", (int)span[2 * (size_t)v], (int)span[2 * (size_t)v + 1], (long long)L.base[(size_t)v]);
    std::printf("%lld\n", (long long)L.R);
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: expmap_check [rows FILE]\n"); return 2; }
  refusals();
  hand_cases();
  extents();
  if (g_bad) { std::printf("%d of %d checks FAILED\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
