// cellmap_check.cpp -- the host side of the filtered Kp-Vsys map (trx_run_filtered_map) on the CPU: vmap_nearest
// (transit_amd/csrc/trx_vmap.h), filtered_map_checks and cell_map_extents (transit_amd/csrc/trx_products.h).  The same
// source the library compiles; every buffer is a heap block of EXACTLY its extent, so that an index outside one is an error
// under -fsanitize=address here and not a fault on the device.
//
//   cellmap_check                 the program's own checks: the refusal table, and the extents walked chunk by chunk the way
//                                 launch_filtered_map and the kernels of hip/trx_cellmap.hip.h address their buffers; prints
//                                 "ok N" (N checks) or FAILED lines
//   cellmap_check nearest FILE    FILE: "nlag n", then the doubles (C99 hex, nan, inf) of lag_kms [nlag] and x [n]; prints
//                                 vmap_nearest of every x, one per line
#include <cstdint>
#include <cstring>

#include "trx_products.h"
#include "trx_vmap.h"
#include "check_common.h"

using namespace trx;

// ---- the refusal table: a map run's refusals under this call's name, then its own two ---------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.lo = 0; S.hi = 5000; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get(); S.filter = true;
  const char *who = "trx_run_filtered_map";
  Heap<double> out(1), lag{0.9999, 1.0, 1.0001}, kms{-3.0, 0.0, 3.0}, kp{100.0, 150.0}, vsys{-5.0, 0.0, 5.0, 10.0}, orbit{0.1, 0.2, 0.3}, offset{0.0, 0.5, 1.0};
  auto good = [&]() { trx_vmap V{}; V.stat = TRX_STAT_CCF; V.nlag = 3; V.lag = lag.get(); V.lag_kms = kms.get(); V.nkp = 2; V.nvsys = 4; V.kp = kp.get(); V.vsys = vsys.get();
                      V.orbit = orbit.get(); V.offset = offset.get(); return V; };
  trx_vmap V = good();
  ACCEPTED(filtered_map_checks(S, who, &V, out.get(), msg));
  V.offset = nullptr; V.stat = TRX_STAT_LOGLIKE_BL19;
  ACCEPTED(filtered_map_checks(S, who, &V, out.get(), msg));
  REFUSED(filtered_map_checks(S, "trx_run_batch_filtered_map", nullptr, nullptr, msg), TRX_E_ARG, "trx_run_batch_filtered_map: vm is NULL");
  // a map run's refusals come first, and before them a trail run's: everything below is wrong as well, and no filter is installed
  ProductState U = S; U.filter = false;
  trx_vmap bad{}; bad.stat = 9; bad.p0 = kNaN;
  ProductState W = U; W.windowed = true;
  REFUSED(filtered_map_checks(W, who, &bad, nullptr, msg), TRX_E_UNSUPPORTED,
          "trx_run_filtered_map: this handle's shard is not the whole grid; take trx_run_pixels, add the ranks' pairs (trx_gather_host) and reduce them on the host");
  ProductState N = U; N.seg = nullptr; N.nexp = N.nseg = 0;
  REFUSED(filtered_map_checks(N, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_filtered_map: no observed set installed (trx_set_observed)");
  REFUSED(filtered_map_checks(U, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_filtered_map: nlag < 1");
  bad.nlag = 3;
  REFUSED(filtered_map_checks(U, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_filtered_map: lag is NULL");
  bad.lag = lag.get();
  REFUSED(filtered_map_checks(U, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_filtered_map: map is NULL");
  lag[1] = -1.0;
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: lag 1 must be finite and > 0");
  lag[1] = 1.0;
  ProductState B = U; B.npix = 0x7fffffffLL;
  bad.nlag = 257;
  REFUSED(filtered_map_checks(B, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: nlag * npix above what one pixel launch takes");
  B = U; B.nexp = 32768; B.nseg = 32768;
  REFUSED(filtered_map_checks(B, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: nlag * nexp * nseg above 2^31 - 1");
  bad.nlag = 3;
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: unknown stat 9");
  bad.stat = TRX_STAT_CHI2;
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: nkp < 1 or nvsys < 1");
  bad.nkp = 65536; bad.nvsys = 32768;
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: nkp * nvsys above 2^31 - 1");
  bad.nkp = 2; bad.nvsys = 4;
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: lag_kms is NULL");
  bad.lag_kms = kms.get();
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: kp is NULL");
  bad.kp = kp.get();
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: vsys is NULL");
  bad.vsys = vsys.get();
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: orbit is NULL");
  bad.orbit = orbit.get(); bad.p1 = kInf;
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: p0 must be finite");
  bad.p0 = 1.0;
  REFUSED(filtered_map_checks(U, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: p1 must be finite");
  V = good();
  kp[1] = kNaN; vsys[3] = kInf; orbit[2] = kNaN; offset[0] = kInf; kms[1] = kNaN;
  REFUSED(filtered_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: kp 1 must be finite");
  kp[1] = 150.0;
  REFUSED(filtered_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: vsys 3 must be finite");
  vsys[3] = 10.0;
  REFUSED(filtered_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: orbit 2 must be finite");
  orbit[2] = 0.3;
  REFUSED(filtered_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: offset 0 must be finite");
  offset[0] = 0.0;
  REFUSED(filtered_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: lag_kms 1 must be finite and above the one before it (strictly increasing)");
  kms[1] = 0.0;
  // its own: no filter, then the size of the index table
  REFUSED(filtered_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: no filter installed (trx_set_filter)");
  REFUSED(filtered_map_checks(U, "trx_run_batch_filtered_map", &V, out.get(), msg), TRX_E_ARG, "trx_run_batch_filtered_map: no filter installed (trx_set_filter)");
  ACCEPTED(filtered_map_checks(S, who, &V, out.get(), msg));
  // (the counts alone decide: the axes are not read beyond the entries there are -- 32768 x 21846 cells pass the map's own
  // limit, 3 exposures of them do not fit the table)
  Heap<double> longkp(32768, 100.0), longvs(21846, 0.0);
  V.nkp = 32768; V.kp = longkp.get(); V.nvsys = 21846; V.vsys = longvs.get();
  CHECK((int64_t)V.nkp * V.nvsys <= 0x7fffffffLL && (int64_t)V.nkp * V.nvsys * 3 > 0x7fffffffLL);
  REFUSED(filtered_map_checks(S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: nkp * nvsys * nexp above 2^31 - 1");
  REFUSED(filtered_map_checks(U, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_filtered_map: no filter installed (trx_set_filter)");
  V.nvsys = 21845;                                       // 32768 * 21845 * 3 = 2^31 - 32768
  ACCEPTED(filtered_map_checks(S, who, &V, out.get(), msg));
}

// ---- the extents, walked the way the launches and the kernels address their buffers -------------------
// Every buffer has exactly its extent's bytes.  k_cell_tracks writes index[cell][v]; per chunk k_cell_filter writes
// val[c][v][p], k_cell_moments reads it and writes mom[(c, v, s)][7], k_cell_stat reads that and writes map[cell0 + c].
static void walk(int64_t cells, int32_t nexp, int32_t nseg, int64_t npix, int64_t cell_cap, uint64_t val_cap, int64_t want_chunk, int64_t want_nchunks, int64_t want_last)
{
  const CellMapExtents X = cell_map_extents(cells, nexp, nseg, npix, cell_cap, val_cap);
  CHECK(X.cells == cells && X.chunk == want_chunk && X.nchunks == want_nchunks && X.last_chunk == want_last);
  CHECK(X.chunk >= 1 && X.chunk <= cell_cap && X.last_chunk >= 1 && X.last_chunk <= X.chunk && (X.nchunks - 1) * X.chunk + X.last_chunk == cells);
  CHECK(X.tracks == cells * nexp && X.track_blocks * kCellTrackBlock >= X.tracks && (X.track_blocks - 1) * kCellTrackBlock < X.tracks);
  CHECK(X.rows == X.chunk * nexp * nseg);
  CHECK(X.index_bytes == 4 * (size_t)cells * (size_t)nexp && X.map_bytes == 8 * (size_t)cells);
  CHECK(X.val_bytes == 8 * (size_t)X.chunk * (size_t)nexp * (size_t)npix && X.mom_bytes == 56 * (size_t)X.chunk * (size_t)nexp * (size_t)nseg);
  CHECK(X.chunk == 1 || X.val_bytes <= val_cap);
  Heap<int32_t> index(X.index_bytes / sizeof(int32_t), -7);
  Heap<double> val(X.val_bytes / sizeof(double)), mom(X.mom_bytes / sizeof(double)), map(X.map_bytes / sizeof(double), -7.0);
  // k_cell_tracks: one lane per (cell, exposure), the last block ragged
  for (int64_t b = 0; b < X.track_blocks; b++)
    for (int t = 0; t < kCellTrackBlock; t++) {
      const int64_t k = b * kCellTrackBlock + t;
      if (k >= X.tracks) continue;
      index[(size_t)k] = (int32_t)(k % nexp);
    }
  int64_t written = 0;
  for (int64_t q = 0; q < X.nchunks; q++) {
    const int64_t cell0 = q * X.chunk, n = q + 1 < X.nchunks ? X.chunk : X.last_chunk;
    const int32_t *idx = index.get() + cell0 * nexp;
    for (size_t k = 0; k < val.n; k++) val[k] = kNaN;
    for (size_t k = 0; k < mom.n; k++) mom[k] = kNaN;
    for (int64_t c = 0; c < n; c++)                            // k_cell_filter: val[c][v][p]
      for (int32_t v = 0; v < nexp; v++)
        for (int64_t p = 0; p < npix; p++) val[(size_t)((c * nexp + v) * npix + p)] = (double)idx[c * nexp + v];
    const int64_t nrows = n * nexp * nseg;                     // k_cell_moments: rows (c, v, s)
    CHECK(nrows <= X.rows);
    for (int64_t row = 0; row < nrows; row++) {
      const int64_t cv = row / nseg, c = cv / nexp, v = cv - c * nexp;
      const double g = npix > 0 ? val[(size_t)(cv * npix + (npix - 1))] : (double)v;
      for (int k = 0; k < TRX_NMOMENT; k++) mom[(size_t)(row * TRX_NMOMENT + k)] = g;
    }
    for (int64_t c = 0; c < n; c++) {                          // k_cell_stat: map[cell0 + c]
      double acc = 0.0;
      for (int32_t v = 0; v < nexp; v++) acc += mom[(size_t)(((c * nexp + v) * nseg + (nseg - 1)) * TRX_NMOMENT + 6)];
      CHECK(map[(size_t)(cell0 + c)] == -7.0);                 // (no cell twice)
      map[(size_t)(cell0 + c)] = acc;
      written++;
    }
  }
  CHECK(written == cells);
  const double want = 0.5 * (double)nexp * (double)(nexp - 1);       // the sum of v over the exposures
  for (int64_t c = 0; c < cells; c++) CHECK(map[(size_t)c] == want);
  for (size_t k = 0; k < index.n; k++) if (index[k] < 0) { CHECK(index[k] >= 0); break; }
}

static void extents()
{
  const uint64_t big = kCellMapValBytes;
  static_assert(kCellMapChunk >= 2, "the cases below need a cap of two cells at the least");
  walk(1, 7, 8, 37, kCellMapChunk, big, 1, 1, 1);                                  // one cell
  walk(kCellMapChunk, 7, 8, 37, kCellMapChunk, big, kCellMapChunk, 1, kCellMapChunk);      // the cells equal the cap
  walk(kCellMapChunk + 1, 7, 8, 37, kCellMapChunk, big, kCellMapChunk, 2, 1);      // cap + 1: a ragged last chunk of one
  walk(2 * kCellMapChunk + 15, 3, 2, 5, kCellMapChunk, big, kCellMapChunk, 3, 15);
  // the byte cap: one cell's values are 7 * 37 * 8 = 2072 bytes
  walk(10, 7, 8, 37, kCellMapChunk, 3 * 2072, 3, 4, 1);                            // three cells fit
  walk(10, 7, 8, 37, kCellMapChunk, 2072, 1, 10, 1);                               // exactly one
  walk(10, 7, 8, 37, kCellMapChunk, 2071, 1, 10, 1);                               // not even one: the chunk is never below one cell
  walk(5, 7, 8, 37, kCellMapChunk, 0, 1, 5, 1);
  // the sizes alone (nothing allocated): a spectrograph's 100 exposures of 160 000 pixels are 128 MB a cell -- 8 cells a chunk
  CellMapExtents X = cell_map_extents(10000, 100, 40, 160000);
  CHECK(X.chunk == 8 && X.nchunks == 1250 && X.last_chunk == 8 && X.val_bytes == (size_t)8 * 128000000 && X.rows == 32000);
  // the moment rows of a chunk stay below 2^31
  X = cell_map_extents(1000, 32768, 32767, 1);
  CHECK(X.chunk == 2 && X.rows == 2LL * 32768 * 32767 && X.rows <= 0x7fffffffLL);
  X = cell_map_extents(1000, 46340, 46340, 1);
  CHECK(X.chunk == 1 && X.nchunks == 1000);
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "nearest")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nlag, n;
    if (std::fscanf(f, "%d %d", &nlag, &n) != 2 || nlag < 1 || n < 0) { std::fprintf(stderr, "cellmap_check: bad header\n"); return 2; }
    const auto kms = read_doubles(f, (size_t)nlag), x = read_doubles(f, (size_t)n);
    std::fclose(f);
    for (int k = 0; k < n; k++) std::printf("%d\n", (int)vmap_nearest(kms.get(), nlag, x[(size_t)k]));
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: cellmap_check [nearest FILE]\n"); return 2; }
  refusals();
  extents();
  if (g_bad) { std::printf("%d of %d checks FAILED\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
