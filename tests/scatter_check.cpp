// scatter_check.cpp -- the host side and the arithmetic of weighing the observed set by its columns' scatter
// (trx_weigh_observed) on the CPU: the refusals, the tiles, the extents and the arithmetic functions of
// transit_amd/csrc/trx_scatter.h.  The same source the library compiles; every buffer is a heap block of EXACTLY its extent,
// addressed the way the kernels of hip/trx_scatter.hip.h address theirs (block by block and lane by lane for the column
// kernel; tile by tile and lane by lane, the segment's variances through a staging array of kScatLds doubles, for the
// median kernel; tile by tile and lane by lane for the weight kernel), so that an index outside one is an error under
// -fsanitize=address here and not a fault on the device.
//
//   scatter_check                 the program's own checks: the refusal table in the header's order, the extents, the tiles,
//                                 sets whose result is known exactly; prints "ok N" (N checks) or FAILED lines
//   scatter_check set FILE        FILE: "nexp kind min_live nseg hasw clip" (clip as C99 hex), the nseg + 1 segment bounds,
//                                 then the doubles (C99 hex) of the data [nexp][npix] and, with hasw = 1, the weights
//                                 [nexp][npix].  Runs the three kernels over the whole set the way the device walks it and
//                                 prints "var" and its [npix] entries, "med" and its [nseg], "w" and its [nexp][npix] as
//                                 C99 hex, and "nmasked N"
#include <cstdint>
#include <cstring>

#include "trx_scatter.h"
#include "check_common.h"

using namespace trx;

// ---- the refusal table, in the header's order --------------------------------------------------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get();
  const char *const who_none = "trx_weigh_observed: no observed set installed (trx_set_observed)";
  for (const int kind : {TRX_SCATTER_NONE, TRX_SCATTER_VARIANCE, TRX_SCATTER_MASK})
    for (const double clip : {0.0, 1.0, 3.0, 1e300})
      for (const int min_live : {2, 3}) {
        const trx_scatter ok{kind, min_live, clip};
        ACCEPTED(scatter_checks(S, &ok, msg));
      }
  ACCEPTED(scatter_checks(S, nullptr, msg));                                               // the undo
  const trx_scatter none{TRX_SCATTER_NONE, 2, 0.0}, var{TRX_SCATTER_VARIANCE, 2, 0.0};
  CHECK(scatter_is_undo(nullptr) && scatter_is_undo(&none) && !scatter_is_undo(&var));
  CHECK(sizeof(trx_scatter) == 16);
  // every later fault at once: the first in the order is the one named
  const trx_scatter bad{3, 1, kNaN};
  ProductState N;                                         // no pixel set, no observed set
  REFUSED(scatter_checks(N, &bad, msg), TRX_E_ARG, who_none);
  REFUSED(scatter_checks(N, nullptr, msg), TRX_E_ARG, who_none);
  N.npix = 6;                                            // a pixel set alone
  REFUSED(scatter_checks(N, &var, msg), TRX_E_ARG, who_none);
  REFUSED(scatter_checks(S, &bad, msg), TRX_E_ARG, "trx_weigh_observed: kind must be TRX_SCATTER_NONE, _VARIANCE or _MASK");
  trx_scatter b = bad;
  b.kind = -1;
  REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: kind must be TRX_SCATTER_NONE, _VARIANCE or _MASK");
  b.kind = TRX_SCATTER_MASK;
  REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: min_live < 2");
  b.min_live = -5;
  REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: min_live < 2");
  b.min_live = 4;
  REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: min_live 4 is above the observed set's nexp 3");
  b.min_live = 3;
  REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: clip must be finite");
  for (const double x : {kInf, -kInf}) {
    b.clip = x;
    REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: clip must be finite");
  }
  b.clip = -1.0;
  REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: clip < 0");
  for (const double x : {0.5, 0x1p-1074, 0x1.fffffffffffffp-1}) {
    b.clip = x;
    REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: clip must be 0 (none) or at least 1");
  }
  // the undo through a struct is checked whole
  b = trx_scatter{TRX_SCATTER_NONE, 1, 0.0};
  REFUSED(scatter_checks(S, &b, msg), TRX_E_ARG, "trx_weigh_observed: min_live < 2");
  // a shard: after every argument
  ProductState W = S; W.windowed = true;
  const char *const shard = "trx_weigh_observed: this handle's shard is not the whole grid; weigh on the host (xcor.scatter_reference)";
  REFUSED(scatter_checks(W, &var, msg), TRX_E_UNSUPPORTED, shard);
  REFUSED(scatter_checks(W, nullptr, msg), TRX_E_UNSUPPORTED, shard);
  b = trx_scatter{TRX_SCATTER_MASK, 2, 0.5};
  REFUSED(scatter_checks(W, &b, msg), TRX_E_ARG, "trx_weigh_observed: clip must be 0 (none) or at least 1");
}

// ---- the extents and the tiles ---------------------------------------------------------------------------
static void extents()
{
  ScatterExtents X = scatter_extents(800, 7, 8, 9, kScatBlock);
  CHECK(X.cells == 5600 && X.col_blocks == 4 && X.tile_blocks == 9 && X.grid_ok);
  CHECK(X.w_bytes == 8u * 5600 && X.var_bytes == 8u * 800 && X.med_bytes == 8u * 8 && X.flag_bytes == 4u * 800);
  X = scatter_extents(81920, 100, 40, 320, kScatBlock);
  CHECK(X.cells == 8192000 && X.col_blocks == 320 && X.tile_blocks == 320 && X.grid_ok && X.w_bytes == (size_t)8 * 8192000);
  X = scatter_extents(1, 2, 1, 1, kScatBlock);
  CHECK(X.cells == 2 && X.col_blocks == 1 && X.tile_blocks == 1 && X.grid_ok && X.w_bytes == 16 && X.var_bytes == 8 && X.flag_bytes == 4);
  X = scatter_extents(257, 3, 5, 6, kScatBlock);
  CHECK(X.col_blocks == 2 && X.grid_ok);
  // the 32-bit grid guard: a launch of no block, or of more blocks than a grid's x extent takes, is not made
  CHECK(!scatter_extents(5, 3, 1, 0, kScatBlock).grid_ok);
  CHECK(scatter_extents((int64_t)0x7fffffffLL * kScatBlock, 2, 1, 0x7fffffffLL, kScatBlock).grid_ok);
  CHECK(!scatter_extents((int64_t)0x7fffffffLL * kScatBlock + 1, 2, 1, 1, kScatBlock).grid_ok);
  CHECK(!scatter_extents(800, 2, 1, 0x80000000LL, kScatBlock).grid_ok);

  // tiles of 1, 256 + 44, none, 256 + 256 + 6: every pixel once, in order, never across a segment
  Heap<int64_t> seg{0, 1, 301, 301, 819};
  ProductState S; S.npix = 819; S.nexp = 3; S.nseg = 4; S.seg = seg.get();
  std::vector<FilterTile> tiles; std::string msg;
  CHECK(scatter_tiles(S, kScatBlock, tiles, msg) == TRX_OK && tiles.size() == 6);
  int64_t next = 0; bool ok = true;
  for (const FilterTile &T : tiles) {
    ok = ok && T.first == next && T.count >= 1 && T.count <= kScatBlock && T.seg >= 0 && T.seg < S.nseg && T.first >= seg[(size_t)T.seg] &&
         T.first + T.count <= seg[(size_t)T.seg + 1];
    next = T.first + T.count;
  }
  CHECK(ok && next == S.npix);
  CHECK(tiles.size() == 6 && tiles[0].count == 1 && tiles[1].count == 256 && tiles[2].count == 44 && tiles[2].seg == 1 && tiles[3].seg == 3 && tiles[5].count == 6);
}

// ---- the whole set, the way the device walks it ---------------------------------------------------------
struct SetResult { Heap<double> var, med, w; Heap<int32_t> flag; int64_t nmasked; };

// k_scatter_cols, k_scatter_median and k_scatter_weights over every block, tile and lane; data [nexp][npix], weight the same or
// null.  lds: the doubles of the staging array (kScatLds on the device; smaller here makes a short segment take several trips)
static SetResult run_set(const ProductState &S, const trx_scatter &sc, const double *data, const double *weight, int lds = kScatLds)
{
  std::string msg;
  std::vector<FilterTile> tiles;
  CHECK(scatter_tiles(S, kScatBlock, tiles, msg) == TRX_OK);
  const ScatterExtents X = scatter_extents(S.npix, S.nexp, S.nseg, (int64_t)tiles.size(), kScatBlock);
  CHECK(X.grid_ok);
  const int64_t npix = S.npix; const int nexp = S.nexp;
  SetResult R{Heap<double>(X.var_bytes / sizeof(double), -7.0), Heap<double>(X.med_bytes / sizeof(double), 0.0), Heap<double>(X.w_bytes / sizeof(double), -7.0),
              Heap<int32_t>(X.flag_bytes / sizeof(int32_t), -7), 0};
  // the column kernel: one lane per column, the last block's lanes past npix do nothing
  for (int64_t blk = 0; blk < X.col_blocks; blk++)
    for (int lane = 0; lane < kScatBlock; lane++) {
      const int64_t p = blk * kScatBlock + lane;
      if (p >= npix) continue;
      R.var[(size_t)p] = weight ? scatter_column<true>(data + p, weight + p, npix, nexp, sc.min_live) : scatter_column<false>(data + p, nullptr, npix, nexp, sc.min_live);
    }
  // the median kernel: one block per tile, the segment's variances staged `lds` at a time; the stores are counted: one per
  // segment with a live column, none elsewhere
  Heap<int> stores((size_t)S.nseg, 0);
  Heap<double> staged((size_t)scatter_padded(lds), -7.0);                  // (kScatLds on the device: kScatTrip divides it)
  Heap<int64_t> rank((size_t)kScatBlock), live_of_wave((size_t)kScatBlock / 64);
  for (const FilterTile &T : tiles) {
    const int64_t first = S.seg[T.seg], last = S.seg[T.seg + 1];
    for (int lane = 0; lane < kScatBlock; lane++) rank[(size_t)lane] = 0;
    for (int wave = 0; wave < kScatBlock / 64; wave++) live_of_wave[(size_t)wave] = 0;
    for (int64_t q0 = first; q0 < last; q0 += lds) {
      const int nq = last - q0 < lds ? (int)(last - q0) : lds;
      const int npad = scatter_padded(nq);
      for (int j0 = 0; j0 < npad; j0 += kScatBlock)
        for (int lane = 0; lane < kScatBlock; lane++) {
          const int j = j0 + lane;
          const double x = j < nq ? R.var[(size_t)(q0 + j)] : 0.0;
          if (j < npad) staged[(size_t)j] = scatter_staged(x);
          if (x > 0.0) live_of_wave[(size_t)lane / 64]++;      // (the wave's ballot)
        }
      for (int lane = 0; lane < kScatBlock; lane++) {
        const int64_t p = T.first + (lane < T.count ? lane : 0);
        const int pj = scatter_place(p, q0);
        int ahead = 0;
        for (int j0 = 0; j0 < npad; j0 += kScatTrip)
          for (int t = 0; t < kScatTrip; t++) scatter_rank_term(staged[(size_t)(j0 + t)], j0 + t, R.var[(size_t)p], pj, ahead);
        rank[(size_t)lane] += ahead;
      }
    }
    int64_t m = 0;
    for (int wave = 0; wave < kScatBlock / 64; wave++) m += live_of_wave[(size_t)wave];
    for (int lane = 0; lane < T.count; lane++) {
      const int64_t p = T.first + lane;
      if (scatter_is_median(R.var[(size_t)p], m, rank[(size_t)lane])) { R.med[(size_t)T.seg] = R.var[(size_t)p]; stores[(size_t)T.seg]++; }
    }
  }
  for (int s = 0; s < S.nseg; s++) {
    bool any = false;
    for (int64_t p = S.seg[s]; p < S.seg[s + 1]; p++) any = any || R.var[(size_t)p] > 0.0;
    CHECK(stores[(size_t)s] == (any ? 1 : 0));
  }
  // the weight kernel: one block per tile, one lane per column
  for (const FilterTile &T : tiles)
    for (int lane = 0; lane < kScatBlock; lane++) {
      if (lane >= T.count) continue;
      const int64_t p = T.first + lane;
      scatter_weights_column(R.var[(size_t)p], R.med[(size_t)T.seg], sc.clip, sc.kind, weight ? weight + p : nullptr, weight != nullptr, R.w.get() + p,
                             R.flag[(size_t)p], npix, nexp);
    }
  for (size_t p = 0; p < R.flag.n; p++) R.nmasked += R.flag[p] == kScatClipped ? 1 : 0;
  return R;
}

// ---- results known exactly ----------------------------------------------------------------------------------
static void known()
{
  // the terms
  int32_t n = 0; double s = 0.0, q = 0.0;
  scatter_sum_term(1.0, 3.0, n, s); scatter_sum_term(0.0, 100.0, n, s); scatter_sum_term(-1.0, 100.0, n, s); scatter_sum_term(kNaN, 100.0, n, s);
  scatter_sum_term(0.5, 5.0, n, s);
  CHECK(n == 2 && s == 8.0 && scatter_mean(s, n) == 4.0);
  scatter_square_term(1.0, 3.0, 4.0, q); scatter_square_term(0.0, 100.0, 4.0, q); scatter_square_term(0.5, 5.0, 4.0, q);
  CHECK(q == 2.0 && scatter_variance(q, 2, 2) == 2.0 && scatter_variance(q, 2, 3) == 0.0 && scatter_variance(q, 3, 2) == 1.0);
  CHECK(scatter_variance(0.0, 5, 2) == 0.0 && !std::signbit(scatter_variance(-0.0, 5, 2)) && scatter_variance(kNaN, 5, 2) == 0.0 &&
        scatter_variance(kInf, 5, 2) == 0.0 && scatter_variance(-1.0, 5, 2) == 0.0 && scatter_variance(0x1p-1074, 2, 2) == 0x1p-1074);
  CHECK(scatter_variance(1.0, 0, 2) == 0.0 && scatter_variance(1.0, 1, 2) == 0.0);
  CHECK(!scatter_enough(1, 2) && scatter_enough(2, 2));
  // the rank: a dead column is staged as +infinity and is ahead of nothing; ties go to the lower place
  CHECK(scatter_staged(0.0) == kInf && scatter_staged(3.0) == 3.0 && scatter_staged(0x1p-1074) == 0x1p-1074);
  int ahead = 0;
  scatter_rank_term(scatter_staged(0.0), 0, 2.0, 5, ahead); scatter_rank_term(1.0, 1, 2.0, 5, ahead); scatter_rank_term(2.0, 2, 2.0, 5, ahead);
  scatter_rank_term(2.0, 5, 2.0, 5, ahead); scatter_rank_term(2.0, 7, 2.0, 5, ahead); scatter_rank_term(3.0, 8, 2.0, 5, ahead);
  CHECK(ahead == 2 && scatter_is_median(2.0, 5, ahead) && !scatter_is_median(2.0, 5, 1) && !scatter_is_median(0.0, 1, 0));
  // the candidate's place in a trip: behind the trip (every tied value is ahead), inside it, ahead of it (none is)
  CHECK(scatter_padded(1) == 8 && scatter_padded(8) == 8 && scatter_padded(9) == 16 && scatter_padded(kScatLds) == kScatLds && kScatLds % kScatTrip == 0);
  CHECK(scatter_place(1030, 0) == 1030 && scatter_place(5, 5) == 0 && scatter_place(0, 1024) == -1024);
  CHECK(scatter_place((int64_t)1 << 40, 0) == 0x7fffffff && scatter_place(0, (int64_t)1 << 40) == -0x7fffffff);
  ahead = 0;
  scatter_rank_term(2.0, 1023, 2.0, scatter_place(2000, 0), ahead); scatter_rank_term(2.0, 0, 2.0, scatter_place(0, 1024), ahead);
  CHECK(ahead == 1);
  CHECK(scatter_is_median(2.0, 4, 1) && !scatter_is_median(2.0, 4, 2) && scatter_is_median(2.0, 1, 0) && scatter_is_median(2.0, 2, 0));
  // the keep rule: clip 0 keeps every live column; var = lim is kept; a dead column never is
  CHECK(scatter_keep(100.0, 1.0, 0.0) && !scatter_keep(0.0, 1.0, 0.0) && scatter_keep(9.0, 1.0, 3.0) && !scatter_keep(0x1.2000000000001p3, 1.0, 3.0));
  CHECK(!scatter_keep(1.0, 0.0, 3.0) && !scatter_keep(0.0, 0.0, 3.0));
  CHECK(scatter_flag(2.0, true) == kScatKept && scatter_flag(2.0, false) == kScatClipped && scatter_flag(0.0, false) == kScatDead);
  // the weights
  CHECK(scatter_inverse(4.0, true) == 0.25 && scatter_inverse(4.0, false) == 0.0);
  CHECK(scatter_weight(TRX_SCATTER_VARIANCE, 1.5, true, 0.25) == 0.25 && scatter_weight(TRX_SCATTER_VARIANCE, 0.0, true, 0.25) == 0.0 &&
        scatter_weight(TRX_SCATTER_VARIANCE, 1.5, false, 0.0) == 0.0 && scatter_weight(TRX_SCATTER_MASK, 1.5, true, 0.25) == 1.5 &&
        scatter_weight(TRX_SCATTER_MASK, 0.0, true, 0.25) == 0.0 && scatter_weight(TRX_SCATTER_MASK, 1.5, false, 0.0) == 0.0);

  // segments of 5, 0, 1 and 2 columns, 3 exposures: the columns' variances are 1, 4, 4, 0 (constant), 100 | | 16 | 1, 9
  Heap<int64_t> seg{0, 5, 5, 6, 8};
  ProductState S; S.npix = 8; S.nexp = 3; S.nseg = 4; S.seg = seg.get();
  Heap<double> data{ 1.0,  2.0, -2.0, 7.0,  10.0,   4.0,  1.0,  3.0,
                     2.0,  4.0,  0.0, 7.0,  20.0,   8.0,  2.0,  6.0,
                     3.0,  6.0,  2.0, 7.0,  30.0,  12.0,  3.0,  9.0};
  const double want_var[8] = {1.0, 4.0, 4.0, 0.0, 100.0, 16.0, 1.0, 9.0};
  for (const int lds : {kScatLds, 2, 1}) {
    // no clip: live columns 1, 4, 4, 100: the lower median of four is rank 1: 4 (the first of the tied pair)
    SetResult R = run_set(S, trx_scatter{TRX_SCATTER_VARIANCE, 2, 0.0}, data.get(), nullptr, lds);
    bool ok = true;
    for (int p = 0; p < 8; p++) ok = ok && R.var[(size_t)p] == want_var[p];
    CHECK(ok);
    CHECK(R.med[0] == 4.0 && R.med[1] == 0.0 && !std::signbit(R.med[1]) && R.med[2] == 16.0 && R.med[3] == 1.0 && R.nmasked == 0);
    CHECK(R.w[0] == 1.0 && R.w[1] == 0.25 && R.w[3] == 0.0 && R.w[4] == 0.01 && R.w[5] == 0.0625 && R.w[7] == 1.0 / 9.0 && R.w[16 + 7] == 1.0 / 9.0);
    CHECK(R.flag[3] == kScatDead && R.flag[4] == kScatKept);
    // clip 3: lim = 36 in segment 0 (100 goes), 9 in segment 3 (9 stays: var = lim)
    R = run_set(S, trx_scatter{TRX_SCATTER_MASK, 2, 3.0}, data.get(), nullptr, lds);
    CHECK(R.nmasked == 1 && R.flag[4] == kScatClipped && R.flag[7] == kScatKept && R.med[0] == 4.0);
    CHECK(R.w[0] == 1.0 && R.w[3] == 0.0 && R.w[4] == 0.0 && R.w[8 + 4] == 0.0 && R.w[7] == 1.0 && R.w[5] == 1.0);
    // clip 1: only the columns at or below the median stay
    R = run_set(S, trx_scatter{TRX_SCATTER_MASK, 2, 1.0}, data.get(), nullptr, lds);
    CHECK(R.nmasked == 2 && R.flag[0] == kScatKept && R.flag[1] == kScatKept && R.flag[2] == kScatKept && R.flag[4] == kScatClipped && R.flag[7] == kScatClipped);
  }
  // weights: exposure 1 masked in column 0 (n = 2: 1, 3 -> var 2), column 1 masked everywhere (dead), a negative weight is a mask
  Heap<double> w(24, 2.0);
  w[8 + 0] = 0.0; w[1] = 0.0; w[8 + 1] = -1.0; w[16 + 1] = 0.0;
  SetResult R = run_set(S, trx_scatter{TRX_SCATTER_VARIANCE, 2, 0.0}, data.get(), w.get());
  CHECK(R.var[0] == 2.0 && R.var[1] == 0.0 && R.med[0] == 4.0);          // (live: 2, 4, 100: rank (3 - 1) / 2 = 1)
  CHECK(R.w[0] == 0.5 && R.w[8] == 0.0 && R.w[16] == 0.5 && R.w[1] == 0.0 && R.w[2] == 0.25);
  // min_live = nexp: column 0 (n = 2) is dead now
  R = run_set(S, trx_scatter{TRX_SCATTER_MASK, 3, 0.0}, data.get(), w.get());
  CHECK(R.var[0] == 0.0 && R.var[2] == 4.0 && R.w[0] == 0.0 && R.w[2] == 2.0 && R.w[16 + 2] == 2.0 && R.med[0] == 4.0);
  // a NaN datum under a positive weight makes the column dead; under a mask it is not looked at
  data[8 + 2] = kNaN;
  R = run_set(S, trx_scatter{TRX_SCATTER_VARIANCE, 2, 0.0}, data.get(), nullptr);
  CHECK(R.var[2] == 0.0 && R.flag[2] == kScatDead && R.w[2] == 0.0);
  w[8 + 2] = 0.0;
  R = run_set(S, trx_scatter{TRX_SCATTER_VARIANCE, 2, 0.0}, data.get(), w.get());
  CHECK(R.var[2] == 8.0 && R.w[2] == 0.125 && R.w[8 + 2] == 0.0);
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "set")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nexp, kind, min_live, nseg, hasw; char clipword[64];
    if (std::fscanf(f, "%d %d %d %d %d %63s", &nexp, &kind, &min_live, &nseg, &hasw, clipword) != 6 || nexp < 1 || nseg < 1) {
      std::fprintf(stderr, "scatter_check: bad header\n"); return 2;
    }
    Heap<int64_t> seg((size_t)nseg + 1);
    for (int s = 0; s <= nseg; s++) {
      long long x;
      if (std::fscanf(f, "%lld", &x) != 1) { std::fprintf(stderr, "scatter_check: bad segment bounds\n"); return 2; }
      seg[(size_t)s] = x;
    }
    const size_t npix = (size_t)seg[(size_t)nseg];
    const auto data = read_doubles(f, (size_t)nexp * npix);
    std::unique_ptr<double[]> w;
    if (hasw) w = read_doubles(f, (size_t)nexp * npix);
    std::fclose(f);
    ProductState S; S.npix = (int64_t)npix; S.nexp = nexp; S.nseg = nseg; S.seg = seg.get();
    const trx_scatter sc{kind, min_live, std::strtod(clipword, nullptr)};
    std::string msg;
    if (scatter_checks(S, &sc, msg) != TRX_OK || scatter_is_undo(&sc)) { std::fprintf(stderr, "scatter_check: %s\n", msg.c_str()); return 2; }
    const SetResult R = run_set(S, sc, data.get(), w.get());
    print_doubles("var", R.var); print_doubles("med", R.med); print_doubles("w", R.w);
    std::printf("nmasked %lld\n", (long long)R.nmasked);
    if (g_bad) return 1;
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: scatter_check [set FILE]\n"); return 2; }
  refusals();
  extents();
  known();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
