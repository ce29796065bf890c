// normalise_check.cpp -- the host side and the arithmetic of normalising the observed set (trx_set_normalise,
// trx_normalise_observed) on the CPU: the refusals, the extents, the tiles and the arithmetic functions of
// transit_amd/csrc/trx_normalise.h.  The same source the library compiles; every buffer is a heap block of EXACTLY its extent,
// addressed the way the kernels of hip/trx_normalise.hip.h address theirs (row by row, one block's lanes per row, the keys of
// the row's first `cap` pixels staged per lane and the pixels past them read again at every step of the bisection, the counts
// per wave and then over the waves, for the row kernel; tile by tile and lane by lane, in place, for the column kernel), so
// that an index outside one is an error under -fsanitize=address here and not a fault on the device.
//
//   normalise_check               the program's own checks: the refusal tables in the header's order, the extents, the tiles,
//                                 the key, the rank, the bisection against a sort, sets whose result is known exactly; prints
//                                 "ok N" (N checks) or FAILED lines
//   normalise_check rank Q M      prints norm_rank(Q, M) (Q as C99 hex)
//   normalise_check set FILE      FILE: "nexp nseg hasw row_kind col_kind quantile clip" (the two doubles as C99 hex), the
//                                 nseg + 1 segment bounds, then the doubles (C99 hex) of the data [nexp][npix] and, with hasw
//                                 = 1, the weights [nexp][npix].  Runs the two kernels over the whole set the way the device
//                                 walks it and prints "data" and its [nexp][npix] entries, "scale" and its [nexp][nseg],
//                                 "centre" and its [npix] as C99 hex, "nclipped N" and "nbad N"
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "trx_normalise.h"
#include "check_common.h"

using namespace trx;

// ---- the refusal tables, in the header's order ---------------------------------------------------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get();
  const std::string who = "trx_set_normalise: ";
  const std::string none = who + "no observed set installed (trx_set_observed)";
  for (const int row : {TRX_NORM_ROW_NONE, TRX_NORM_ROW_QUANTILE})
    for (const int col : {TRX_NORM_COL_NONE, TRX_NORM_COL_DIVIDE, TRX_NORM_COL_RATIO, TRX_NORM_COL_SUBTRACT})
      for (const double q : {0.0, 0.5, 1.0})
        for (const double clip : {0.0, 1.0, 5.0, 1e300}) {
          const trx_normalise nm{row, col, q, clip};
          if (row == TRX_NORM_ROW_NONE && col == TRX_NORM_COL_NONE && clip == 0.0)
            REFUSED(normalise_set_checks(S, &nm, msg), TRX_E_ARG, (who + "a recipe that does nothing (pass NULL to clear)").c_str());
          else ACCEPTED(normalise_set_checks(S, &nm, msg));
        }
  ACCEPTED(normalise_set_checks(S, nullptr, msg));                                         // the clearing call
  CHECK(sizeof(trx_normalise) == 24);
  // every later fault at once: the first in the order is the one named
  trx_normalise b{2, 4, kNaN, kNaN};
  ProductState N;                                         // no pixel set, no observed set
  REFUSED(normalise_set_checks(N, &b, msg), TRX_E_ARG, none.c_str());
  REFUSED(normalise_set_checks(N, nullptr, msg), TRX_E_ARG, none.c_str());
  N.npix = 6;                                            // a pixel set alone
  REFUSED(normalise_set_checks(N, &b, msg), TRX_E_ARG, none.c_str());
  REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "row_kind must be TRX_NORM_ROW_NONE or _QUANTILE").c_str());
  b.row_kind = -1;
  REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "row_kind must be TRX_NORM_ROW_NONE or _QUANTILE").c_str());
  b.row_kind = TRX_NORM_ROW_NONE;
  REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "col_kind must be TRX_NORM_COL_NONE, _DIVIDE, _RATIO or _SUBTRACT").c_str());
  b.col_kind = -1;
  REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "col_kind must be TRX_NORM_COL_NONE, _DIVIDE, _RATIO or _SUBTRACT").c_str());
  b.col_kind = TRX_NORM_COL_NONE;                          // (the quantile is checked whatever row_kind is)
  for (const double q : {kNaN, kInf, -kInf, -0x1p-1074, 0x1.0000000000001p0}) {
    b.quantile = q;
    REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "quantile must be finite and in [0, 1]").c_str());
  }
  b.quantile = 0.5;
  for (const double x : {kNaN, kInf, -kInf}) {
    b.clip = x;
    REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "clip must be finite").c_str());
  }
  b.clip = -1.0;
  REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "clip < 0").c_str());
  for (const double x : {0.5, 0x1p-1074, 0x1.fffffffffffffp-1}) {
    b.clip = x;
    REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "clip must be 0 (none) or at least 1").c_str());
  }
  b.clip = 0.0;
  REFUSED(normalise_set_checks(S, &b, msg), TRX_E_ARG, (who + "a recipe that does nothing (pass NULL to clear)").c_str());
  // a shard: after every argument
  ProductState W = S; W.windowed = true;
  const std::string shard = who + "this handle's shard is not the whole grid; normalise on the host (xcor.normalise_reference)";
  const trx_normalise ok{TRX_NORM_ROW_QUANTILE, TRX_NORM_COL_RATIO, 0.5, 0.0};
  REFUSED(normalise_set_checks(W, &ok, msg), TRX_E_UNSUPPORTED, shard.c_str());
  REFUSED(normalise_set_checks(W, nullptr, msg), TRX_E_UNSUPPORTED, shard.c_str());
  REFUSED(normalise_set_checks(W, &b, msg), TRX_E_ARG, (who + "a recipe that does nothing (pass NULL to clear)").c_str());

  // trx_normalise_observed: no observed set, no recipe, then the injection's arguments as the detrend has them, the shard last
  const std::string run = "trx_normalise_observed: ";
  const double shift[3] = {1.0, 1.0, 1.0}, bad_shift[3] = {1.0, -1.0, 1.0};
  const int a = 0, o = 0;                                  // (stand-ins: the checks look at the pointers alone)
  ACCEPTED(normalise_checks(S, true, 0, kNaN, kNaN, nullptr, nullptr, 0, nullptr, msg));   // (without an injection nothing of it is looked at)
  ACCEPTED(normalise_checks(S, true, 1, 0.5, 1.0, &a, &o, 3, shift, msg));
  REFUSED(normalise_checks(N, false, 2, kNaN, kNaN, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "no observed set installed (trx_set_observed)").c_str());
  REFUSED(normalise_checks(S, false, 2, kNaN, kNaN, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "no recipe installed (trx_set_normalise)").c_str());
  REFUSED(normalise_checks(W, false, 0, 0.0, 0.0, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "no recipe installed (trx_set_normalise)").c_str());
  REFUSED(normalise_checks(S, true, 2, kNaN, kNaN, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "inject must be 0 or 1").c_str());
  REFUSED(normalise_checks(S, true, 1, kNaN, kNaN, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "p0 must be finite").c_str());
  REFUSED(normalise_checks(S, true, 1, 0.5, kInf, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "p1 must be finite").c_str());
  REFUSED(normalise_checks(S, true, 1, 0.5, 1.0, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "a is NULL").c_str());
  REFUSED(normalise_checks(S, true, 1, 0.5, 1.0, &a, nullptr, 0, nullptr, msg), TRX_E_ARG, (run + "o is NULL").c_str());
  REFUSED(normalise_checks(S, true, 1, 0.5, 1.0, &a, &o, 0, nullptr, msg), TRX_E_ARG, (run + "shift is NULL").c_str());
  REFUSED(normalise_checks(S, true, 1, 0.5, 1.0, &a, &o, 2, shift, msg), TRX_E_ARG, (run + "nshift 2 is not the observed set's nexp 3").c_str());
  REFUSED(normalise_checks(S, true, 1, 0.5, 1.0, &a, &o, 3, bad_shift, msg), TRX_E_ARG, (run + "shift 1 must be finite and > 0").c_str());
  REFUSED(normalise_checks(W, true, 0, 0.0, 0.0, nullptr, nullptr, 0, nullptr, msg), TRX_E_UNSUPPORTED,
          (run + "this handle's shard is not the whole grid; detrend on the host (xcor.normalise_reference)").c_str());
}

// ---- the extents and the tiles ---------------------------------------------------------------------------
static void extents()
{
  NormExtents X = normalise_extents(800, 7, 8, 15, kNormWaves);
  CHECK(X.cells == 5600 && X.rows == 56 && X.row_blocks == 56 && X.tile_blocks == 4 && X.grid_ok);
  CHECK(X.r_bytes == 8u * 5600 && X.scale_bytes == 8u * 56 && X.centre_bytes == 8u * 800 && X.count_bytes == 4u * 2 * 800);
  X = normalise_extents(81920, 100, 40, 1280, kNormWaves);
  CHECK(X.cells == 8192000 && X.rows == 4000 && X.row_blocks == 4000 && X.tile_blocks == 320 && X.grid_ok && X.r_bytes == (size_t)8 * 8192000);
  X = normalise_extents(1, 1, 1, 1, kNormWaves);
  CHECK(X.cells == 1 && X.row_blocks == 1 && X.tile_blocks == 1 && X.grid_ok && X.scale_bytes == 8 && X.count_bytes == 8);
  // the 32-bit grid guard: a launch of no block, or of more blocks than a grid's x extent takes, is not made
  CHECK(!normalise_extents(5, 3, 1, 0, kNormWaves).grid_ok);
  CHECK(normalise_extents(5, 0x7fffffff, 1, 1, kNormWaves).grid_ok && !normalise_extents(5, 0x7fffffff, 2, 1, kNormWaves).grid_ok);
  CHECK(normalise_extents(5, 1, 1, (int64_t)0x7fffffffLL * kNormWaves, kNormWaves).grid_ok && !normalise_extents(5, 1, 1, (int64_t)0x7fffffffLL * kNormWaves + 1, kNormWaves).grid_ok);
  CHECK(kNormCap == 2048 && kNormCap == kNormBlock * kNormPerLane && kNormBlock % 64 == 0 && kNormBits == 64);

  // tiles of 1, 64 + 6, none, 64 + 64 + 2: every pixel once, in order, never across a segment
  Heap<int64_t> seg{0, 1, 71, 71, 201};
  ProductState S; S.npix = 201; S.nexp = 3; S.nseg = 4; S.seg = seg.get();
  std::vector<FilterTile> tiles; std::string msg;
  CHECK(sysrem_tiles(S, tiles, msg, "who") == TRX_OK && tiles.size() == 6);
  int64_t next = 0; bool ok = true;
  for (const FilterTile &T : tiles) {
    ok = ok && T.first == next && T.count >= 1 && T.count <= 64 && T.seg >= 0 && T.seg < S.nseg && T.first >= seg[(size_t)T.seg] &&
         T.first + T.count <= seg[(size_t)T.seg + 1];
    next = T.first + T.count;
  }
  CHECK(ok && next == S.npix);
  CHECK(tiles[0].count == 1 && tiles[1].count == 64 && tiles[2].count == 6 && tiles[2].seg == 1 && tiles[3].seg == 3 && tiles[5].count == 2);
}

// ---- the whole set, the way the device walks it ---------------------------------------------------------
struct SetResult { Heap<double> data, scale, centre; int64_t nclipped, nbad; };

// k_norm_rowscale of one row: the block's lanes, the staged keys of the first `cap` pixels (lane l holds the pixels t * block + l),
// the pixels past them read again at every step; f and w: the row's segment [len] (w null: all 1).  steps: the counting steps
// taken, for the caller to hold against kNormBits
static double row_scale(const trx_normalise &nm, const double *f, const double *w, int64_t len, int cap, int *steps = nullptr)
{
  const int per = cap / kNormBlock, nwaves = kNormBlock / 64;
  CHECK(cap % kNormBlock == 0 && per >= 1);
  const int64_t nstaged = len < cap ? len : cap;
  Heap<uint64_t> key((size_t)cap, kNormDeadKey);           // [per][kNormBlock]: a lane's registers, lane by lane
  Heap<int64_t> of_wave((size_t)nwaves, 0);
  for (int t = 0; t < per; t++)
    for (int lane = 0; lane < kNormBlock; lane++) {
      const int64_t j = (int64_t)t * kNormBlock + lane;
      if (j < nstaged) {
        key[(size_t)j] = norm_staged(w ? w[j] : 1.0, f[j]);
        if ((w ? w[j] : 1.0) > 0.0) of_wave[(size_t)lane / 64]++;
      }
    }
  for (int64_t j0 = cap; j0 < len; j0 += kNormBlock)
    for (int lane = 0; lane < kNormBlock; lane++) {
      const int64_t j = j0 + lane;
      if (j < len && (w ? w[j] : 1.0) > 0.0) of_wave[(size_t)lane / 64]++;
    }
  int64_t m = 0;
  for (int k = 0; k < nwaves; k++) m += of_wave[(size_t)k];
  double x = 0.0; int taken = 0;
  if (nm.row_kind == TRX_NORM_ROW_QUANTILE && m >= 1) {
    const int64_t k = norm_rank(nm.quantile, m);
    CHECK(k >= 0 && k < m);
    uint64_t found = 0;
    for (int bit = kNormBits - 1; bit >= 0; bit--, taken++) {
      const uint64_t trial = norm_trial(found, bit);
      for (int kk = 0; kk < nwaves; kk++) of_wave[(size_t)kk] = 0;
      for (int t = 0; t < per; t++)
        for (int lane = 0; lane < kNormBlock; lane++)
          if (norm_below(key[(size_t)t * kNormBlock + (size_t)lane], trial)) of_wave[(size_t)lane / 64]++;
      for (int64_t j0 = cap; j0 < len; j0 += kNormBlock)
        for (int lane = 0; lane < kNormBlock; lane++) {
          const int64_t j = j0 + lane;
          const uint64_t kj = j < len ? norm_staged(w ? w[j] : 1.0, f[j]) : kNormDeadKey;
          if (norm_below(kj, trial)) of_wave[(size_t)lane / 64]++;
        }
      int64_t below = 0;
      for (int kk = 0; kk < nwaves; kk++) below += of_wave[(size_t)kk];
      found = norm_bisect_step(found, bit, below, k);
    }
    x = norm_unkey(found);
  }
  if (steps) *steps = taken;
  return norm_scale(nm.row_kind, x, m);
}

// k_norm_rowscale and k_norm_cols over every row, tile and lane; data [nexp][npix], weight the same or null.  cap: the staging
// capacity (kNormCap on the device; smaller here makes a short segment take the path that reads again)
static SetResult run_set(const ProductState &S, const trx_normalise &nm, const double *data, const double *weight, int cap = kNormCap)
{
  std::string msg;
  std::vector<FilterTile> tiles;
  CHECK(sysrem_tiles(S, tiles, msg, "normalise_check") == TRX_OK);
  const NormExtents X = normalise_extents(S.npix, S.nexp, S.nseg, (int64_t)tiles.size(), kNormWaves);
  CHECK(X.grid_ok);
  const int64_t npix = S.npix; const int nexp = S.nexp, nseg = S.nseg;
  SetResult R{Heap<double>(X.r_bytes / sizeof(double)), Heap<double>(X.scale_bytes / sizeof(double), 0.0), Heap<double>(X.centre_bytes / sizeof(double), -7.0), 0, 0};
  Heap<int32_t> count(X.count_bytes / sizeof(int32_t), -7);
  for (size_t k = 0; k < R.data.n; k++) R.data[k] = data[k];          // (steps 0 and 1 left f0 in the call's buffer)
  // the row kernel: one block per row (v, s)
  for (int64_t row = 0; row < X.row_blocks; row++) {
    const int64_t v = row / nseg, s = row - v * nseg;
    const int64_t first = S.seg[s], last = S.seg[s + 1];
    int steps = -1;
    R.scale[(size_t)row] = row_scale(nm, R.data.get() + v * npix + first, weight ? weight + v * npix + first : nullptr, last - first, cap, &steps);
    CHECK(steps == 0 || steps == kNormBits);
  }
  // the column kernel: kNormWaves tiles per block, a wave per tile, one lane per column, in place
  for (int64_t blk = 0; blk < X.tile_blocks; blk++)
    for (int wave = 0; wave < kNormWaves; wave++) {
      const int64_t tile = blk * kNormWaves + wave;
      if (tile >= (int64_t)tiles.size()) continue;
      const FilterTile &T = tiles[(size_t)tile];
      for (int lane = 0; lane < 64; lane++) {
        if (lane >= T.count) continue;
        const int64_t p = T.first + lane;
        const double *const scale = R.scale.get() + T.seg;
        if (weight) norm_column<true>(R.data.get(), weight, scale, p, npix, nseg, nexp, nm.row_kind, nm.col_kind, nm.clip, R.centre[(size_t)p], count[(size_t)p], count[(size_t)(npix + p)]);
        else norm_column<false>(R.data.get(), nullptr, scale, p, npix, nseg, nexp, nm.row_kind, nm.col_kind, nm.clip, R.centre[(size_t)p], count[(size_t)p], count[(size_t)(npix + p)]);
      }
    }
  for (int64_t p = 0; p < npix; p++) { R.nclipped += count[(size_t)p]; R.nbad += count[(size_t)(npix + p)]; }
  return R;
}

// ---- results known exactly ----------------------------------------------------------------------------------
static void known()
{
  // the key: its order is the values', -0 just below +0, and it has an inverse
  const double xs[] = {-kInf, -1.7976931348623157e308, -2.0, -1.0, -0x1p-1074, -0.0, 0.0, 0x1p-1074, 1.0, 0x1.0000000000001p0, 2.0, 1.7976931348623157e308, kInf};
  bool ok = true;
  for (size_t i = 0; i + 1 < sizeof xs / sizeof *xs; i++) ok = ok && norm_key(xs[i]) < norm_key(xs[i + 1]);
  for (const double x : xs) { const double back = norm_unkey(norm_key(x)); ok = ok && std::memcmp(&x, &back, sizeof x) == 0 && norm_key(x) != kNormDeadKey; }
  CHECK(ok);
  CHECK(norm_key(0.0) == 0x8000000000000000ULL && norm_key(-0.0) == 0x7fffffffffffffffULL && std::signbit(norm_unkey(0x7fffffffffffffffULL)));
  CHECK(norm_staged(0.0, 5.0) == kNormDeadKey && norm_staged(-1.0, 5.0) == kNormDeadKey && norm_staged(kNaN, 5.0) == kNormDeadKey && norm_staged(2.0, 5.0) == norm_key(5.0));
  CHECK(!norm_below(kNormDeadKey, kNormDeadKey) && norm_below(norm_key(1.0), norm_key(2.0)) && !norm_below(norm_key(2.0), norm_key(2.0)));
  // the rank
  CHECK(norm_rank(0.0, 1) == 0 && norm_rank(0.5, 1) == 0 && norm_rank(1.0, 1) == 0 && norm_rank(0.5, 2) == 0 && norm_rank(1.0, 2) == 1);
  CHECK(norm_rank(0.5, 3) == 1 && norm_rank(0.5, 4) == 1 && norm_rank(0.9, 3) == 1 && norm_rank(0.9, 64) == 56 && norm_rank(0.9, 65) == 57);
  CHECK(norm_rank(1.0, 65) == 64 && norm_rank(0.5, 64) == 31 && norm_rank(0.5, 65) == 32 && norm_rank(0.0, 65) == 0);
  // one step: the bit stays where no more than k keys are below the trial
  CHECK(norm_trial(0, 63) == 0x8000000000000000ULL && norm_trial(0x8000000000000000ULL, 0) == 0x8000000000000001ULL);
  CHECK(norm_bisect_step(0, 63, 3, 3) == 0x8000000000000000ULL && norm_bisect_step(0, 63, 4, 3) == 0 && norm_bisect_step(0xf0, 0, 0, 0) == 0xf1);
  // the bisection against a sort: ties, negatives, zeros of both signs, masked entries, every rank, and a capacity below the row
  {
    Heap<double> f{3.0, -1.0, 3.0, 0.0, -0.0, 7.5, 3.0, -1.0, 1e300, -1e-300, 2.0, 2.0, 99.0};
    Heap<double> w{1.0, 1.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, -1.0};
    std::vector<double> live;
    for (size_t j = 0; j < f.n; j++) if (w[j] > 0.0) live.push_back(f[j]);
    std::sort(live.begin(), live.end());
    bool same = true;
    for (int k = 0; k < (int)live.size(); k++) {
      const trx_normalise nm{TRX_NORM_ROW_QUANTILE, TRX_NORM_COL_NONE, (double)k / (double)(live.size() - 1), 0.0};
      const double at = live[(size_t)norm_rank(nm.quantile, (int64_t)live.size())], want = at > 0.0 ? at : 0.0;
      same = same && (k > 0 || at == -1.0) && (k < 10 || at == 1e300);
      // (the capacity is a whole number of blocks here as on the device: the row of 13 lies inside it)
      same = same && row_scale(nm, f.get(), w.get(), (int64_t)f.n, kNormCap) == want && !std::signbit(row_scale(nm, f.get(), w.get(), (int64_t)f.n, kNormCap));
    }
    CHECK(same && live.size() == 11);
    const trx_normalise med{TRX_NORM_ROW_QUANTILE, TRX_NORM_COL_NONE, 0.5, 0.0}, none{TRX_NORM_ROW_NONE, TRX_NORM_COL_RATIO, 0.5, 0.0};
    CHECK(row_scale(med, f.get(), w.get(), (int64_t)f.n, kNormCap) == 2.0);           // (-1 -1 -1e-300 -0 0 [2] 3 3 3 7.5 1e300)
    CHECK(row_scale(none, f.get(), w.get(), (int64_t)f.n, kNormCap) == 1.0 && row_scale(med, f.get(), w.get(), 0, kNormCap) == 0.0);
    Heap<double> dead(f.n, 0.0);
    CHECK(row_scale(med, f.get(), dead.get(), (int64_t)f.n, kNormCap) == 0.0 && row_scale(none, f.get(), dead.get(), (int64_t)f.n, kNormCap) == 0.0);
    // a row of 600 under a capacity of one block: 344 of its pixels are read again at every step
    Heap<double> g(600), gw(600, 1.0);
    uint64_t z = 12345;
    for (size_t j = 0; j < g.n; j++) { z = z * 6364136223846793005ULL + 1442695040888963407ULL; g[j] = (double)(int64_t)(z >> 40) / 1048576.0 - 8.0; gw[j] = (z >> 13) % 11 ? 1.0 : 0.0; }
    live.clear();
    for (size_t j = 0; j < g.n; j++) if (gw[j] > 0.0) live.push_back(g[j]);
    std::sort(live.begin(), live.end());
    same = true;
    for (const double q : {0.0, 0.25, 0.5, 0.9, 1.0}) {
      const trx_normalise nm{TRX_NORM_ROW_QUANTILE, TRX_NORM_COL_NONE, q, 0.0};
      const double want = live[(size_t)norm_rank(q, (int64_t)live.size())];
      for (const int cap : {kNormBlock, 2 * kNormBlock, kNormCap})
        same = same && row_scale(nm, g.get(), gw.get(), (int64_t)g.n, cap) == (want > 0.0 ? want : 0.0);
    }
    CHECK(same && live.size() > 500);
  }
  // the scale, the centre and the entry
  CHECK(norm_scale(TRX_NORM_ROW_QUANTILE, 2.0, 1) == 2.0 && norm_scale(TRX_NORM_ROW_QUANTILE, 2.0, 0) == 0.0 && norm_scale(TRX_NORM_ROW_QUANTILE, -2.0, 5) == 0.0);
  CHECK(!std::signbit(norm_scale(TRX_NORM_ROW_QUANTILE, -0.0, 5)) && norm_scale(TRX_NORM_ROW_QUANTILE, kNaN, 5) == 0.0 && norm_scale(TRX_NORM_ROW_NONE, -3.0, 5) == 1.0);
  CHECK(norm_row(TRX_NORM_ROW_QUANTILE, 3.0, 2.0) == 1.5 && norm_row(TRX_NORM_ROW_NONE, 3.0, 1.0) == 3.0 && norm_on(1.0, 2.0) && !norm_on(0.0, 2.0) && !norm_on(1.0, 0.0));
  bool good = true;
  CHECK(norm_centre(TRX_NORM_COL_DIVIDE, 6.0, 3, good) == 2.0 && good && norm_centre(TRX_NORM_COL_DIVIDE, 6.0, 0, good) == 0.0 && !good);
  CHECK(norm_centre(TRX_NORM_COL_RATIO, -6.0, 3, good) == 0.0 && !good && norm_centre(TRX_NORM_COL_SUBTRACT, -6.0, 3, good) == -2.0 && good);
  CHECK(norm_centre(TRX_NORM_COL_RATIO, 0.0, 3, good) == 0.0 && !good && norm_centre(TRX_NORM_COL_SUBTRACT, kInf, 3, good) == 0.0 && !good);
  CHECK(norm_centre(TRX_NORM_COL_DIVIDE, kNaN, 3, good) == 0.0 && !good && norm_centre(TRX_NORM_COL_NONE, -6.0, 3, good) == -2.0 && good);
  CHECK(norm_col(TRX_NORM_COL_DIVIDE, 3.0, 2.0) == 1.5 && norm_col(TRX_NORM_COL_RATIO, 3.0, 2.0) == 0.5 && norm_col(TRX_NORM_COL_SUBTRACT, 3.0, 2.0) == 1.0 &&
        norm_col(TRX_NORM_COL_NONE, 3.0, 2.0) == 3.0 && norm_entry(TRX_NORM_ROW_QUANTILE, TRX_NORM_COL_RATIO, 6.0, 2.0, 2.0) == 0.5);
  // the clip
  CHECK(!norm_clips(0.0, 5, true) && !norm_clips(3.0, 1, true) && !norm_clips(3.0, 5, false) && norm_clips(3.0, 2, true));
  double q = 0.0;
  norm_square_term(true, 3.0, 1.0, q); norm_square_term(false, 100.0, 1.0, q); norm_square_term(true, -1.0, 1.0, q);
  CHECK(q == 8.0 && norm_limit(2.0, q, 3) == 16.0 && norm_clipped(5.5, 1.0, 16.0) && !norm_clipped(5.0, 1.0, 16.0) && !norm_clipped(5.0, 1.0, kNaN));

  // two segments of 3 and 2 columns, 4 exposures; rows' lower medians 2, 4, (masked), 1 | 10, -2 (a bad row), 20, 40
  Heap<int64_t> seg{0, 3, 5};
  ProductState S; S.npix = 5; S.nexp = 4; S.nseg = 2; S.seg = seg.get();
  Heap<double> data{1.0, 2.0,  4.0,   10.0,  20.0,
                    2.0, 4.0,  8.0,   -1.0,  -2.0,
                    5.0, 5.0,  5.0,   20.0,  40.0,
                    0.5, 1.0,  2.0,   40.0,  80.0};
  Heap<double> w(20, 1.0);
  w[10] = w[11] = w[12] = 0.0;                            // exposure 2 masked over segment 0
  for (const int cap : {kNormCap, kNormBlock}) {
    SetResult R = run_set(S, trx_normalise{TRX_NORM_ROW_QUANTILE, TRX_NORM_COL_RATIO, 0.5, 0.0}, data.get(), w.get(), cap);
    const double want_scale[8] = {2.0, 10.0, 4.0, 0.0, 0.0, 20.0, 1.0, 40.0};
    bool same = true;
    for (int k = 0; k < 8; k++) same = same && R.scale[(size_t)k] == want_scale[k] && !std::signbit(R.scale[(size_t)k]);
    CHECK(same);
    // f1: 0.5 1 2 | 1 2;  0.5 1 2 | bad;  dead | 1 2;  0.5 1 2 | 1 2: the centres are the columns' own values, the data all +0
    CHECK(R.centre[0] == 0.5 && R.centre[1] == 1.0 && R.centre[2] == 2.0 && R.centre[3] == 1.0 && R.centre[4] == 2.0);
    same = true;
    for (size_t k = 0; k < R.data.n; k++) same = same && R.data[k] == 0.0 && !std::signbit(R.data[k]);
    CHECK(same && R.nclipped == 0 && R.nbad == 2);          // (the two live entries of the bad row)
    // SUBTRACT without the row step: the centres are the means in time over the live entries
    R = run_set(S, trx_normalise{TRX_NORM_ROW_NONE, TRX_NORM_COL_SUBTRACT, 0.5, 0.0}, data.get(), w.get(), cap);
    CHECK(R.scale[0] == 1.0 && R.scale[4] == 0.0 && R.scale[3] == 1.0 && R.centre[1] == 7.0 / 3.0 && R.centre[3] == 17.25 && R.data[3] == -7.25 && R.data[10] == 0.0 && R.nbad == 0);
  }
  // the clip: one column of 12 exposures about 1 with one entry at 100: that entry becomes the mean of all twelve
  Heap<int64_t> seg1{0, 1};
  ProductState C; C.npix = 1; C.nexp = 12; C.nseg = 1; C.seg = seg1.get();
  Heap<double> col(12, 1.0);
  col[4] = 100.0; col[5] = 1.5; col[6] = 0.5;
  SetResult R = run_set(C, trx_normalise{TRX_NORM_ROW_NONE, TRX_NORM_COL_NONE, 0.5, 3.0}, col.get(), nullptr);
  CHECK(R.nclipped == 1 && R.nbad == 0 && R.data[4] == 111.0 / 12.0 && R.data[5] == 1.5 && R.data[0] == 1.0 && R.centre[0] == 111.0 / 12.0);
}

int main(int argc, char **argv)
{
  if (argc == 4 && !std::strcmp(argv[1], "rank")) {
    std::printf("%lld\n", (long long)norm_rank(std::strtod(argv[2], nullptr), std::atoll(argv[3])));
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "set")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nexp, nseg, hasw, row_kind, col_kind; char qword[64], clipword[64];
    if (std::fscanf(f, "%d %d %d %d %d %63s %63s", &nexp, &nseg, &hasw, &row_kind, &col_kind, qword, clipword) != 7 || nexp < 1 || nseg < 1) {
      std::fprintf(stderr, "normalise_check: bad header\n"); return 2;
    }
    Heap<int64_t> seg((size_t)nseg + 1);
    for (int s = 0; s <= nseg; s++) {
      long long x;
      if (std::fscanf(f, "%lld", &x) != 1) { std::fprintf(stderr, "normalise_check: bad segment bounds\n"); return 2; }
      seg[(size_t)s] = x;
    }
    const size_t npix = (size_t)seg[(size_t)nseg];
    const auto data = read_doubles(f, (size_t)nexp * npix);
    std::unique_ptr<double[]> w;
    if (hasw) w = read_doubles(f, (size_t)nexp * npix);
    std::fclose(f);
    ProductState S; S.npix = (int64_t)npix; S.nexp = nexp; S.nseg = nseg; S.seg = seg.get();
    const trx_normalise nm{row_kind, col_kind, std::strtod(qword, nullptr), std::strtod(clipword, nullptr)};
    std::string msg;
    if (normalise_set_checks(S, &nm, msg) != TRX_OK) { std::fprintf(stderr, "normalise_check: %s\n", msg.c_str()); return 2; }
    const SetResult R = run_set(S, nm, data.get(), w.get());
    print_doubles("data", R.data); print_doubles("scale", R.scale); print_doubles("centre", R.centre);
    std::printf("nclipped %lld\nnbad %lld\n", (long long)R.nclipped, (long long)R.nbad);
    if (g_bad) return 1;
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: normalise_check [rank Q M | set FILE]\n"); return 2; }
  refusals();
  extents();
  known();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
