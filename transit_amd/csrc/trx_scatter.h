// trx_scatter.h -- the host side and the arithmetic of weighing the observed set by its columns' scatter on the device
// (trx_weigh_observed, include/transit_hip.h): what the call refuses, the tiles and the extents of its buffers, its launch
// sizes, and the arithmetic -- a column's sums, its variance, the rank test of the segment median, the keep rule and the new
// weight -- as plain host/device functions.  Plain C++ (no HIP): the kernels of hip/trx_scatter.hip.h call the functions per
// lane, tests/scatter_check.cpp runs the same source on the CPU over exact-size arrays.  Every operation is an IEEE double
// operation rounded once -- no fused multiply-add -- in the order transit_amd/xcor.py (scatter_reference) writes it.
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "transit_hip.h"
#include "trx_columns.h"
#include "trx_numerics.h"
#include "trx_products.h"

namespace trx {

constexpr int kScatBlock = 256;                       // lanes per block: whole waves; the candidate columns of a tile
constexpr int kScatLds = 1024;                        // variances of a segment that the median kernel stages in LDS at once
constexpr int kScatTrip = 8;                          // staged variances a lane reads before it compares the first (divides kScatLds)

// ---- the call: checks, tiles, extents ---------------------------------------------------------------
// Whether the call is the undo (sc NULL or kind = TRX_SCATTER_NONE): the weights of trx_set_observed back in force.
inline bool scatter_is_undo(const trx_scatter *sc) { return !sc || sc->kind == TRX_SCATTER_NONE; }

// What trx_weigh_observed refuses, in the header's order.  A NULL sc is checked for the observed set (and the shard) alone.
inline int scatter_checks(const ProductState &S, const trx_scatter *sc, std::string &msg)
{
  const char *const who = "trx_weigh_observed";
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (sc) {
    if (sc->kind < TRX_SCATTER_NONE || sc->kind > TRX_SCATTER_MASK) return no(TRX_E_ARG, "kind must be TRX_SCATTER_NONE, _VARIANCE or _MASK");
    if (sc->min_live < 2) return no(TRX_E_ARG, "min_live < 2");
    if (sc->min_live > S.nexp) return no(TRX_E_ARG, "min_live " + std::to_string(sc->min_live) + " is above the observed set's nexp " + std::to_string(S.nexp));
    if (!std::isfinite(sc->clip)) return no(TRX_E_ARG, "clip must be finite");
    if (sc->clip < 0.0) return no(TRX_E_ARG, "clip < 0");
    if (sc->clip > 0.0 && sc->clip < 1.0) return no(TRX_E_ARG, "clip must be 0 (none) or at least 1");
  }
  if (S.windowed) return no(TRX_E_UNSUPPORTED, "this handle's shard is not the whole grid; weigh on the host (xcor.scatter_reference)");
  return TRX_OK;
}

// The tiles of the observed set's segments: up to `width` consecutive pixels of one segment each, a segment's tiles in pixel
// order (FilterTile's fields; count goes up to width here).  One block of the median and the weight kernel owns one tile:
// its lanes are the tile's columns, its waves 64 of them each.  An empty segment has no tile.
inline int scatter_tiles(const ProductState &S, int width, std::vector<FilterTile> &tiles, std::string &msg)
{
  try {
    tiles.clear();
    for (int32_t s = 0; s < S.nseg; s++)
      for (int64_t p = S.seg[(size_t)s]; p < S.seg[(size_t)s + 1]; p += width)
        tiles.push_back(FilterTile{p, s, (int32_t)std::min<int64_t>(width, S.seg[(size_t)s + 1] - p)});
  } catch (...) { return refuse(msg, TRX_E_NOMEM, "trx_weigh_observed: out of host memory"); }
  return TRX_OK;
}

// The extents of a weigh call over nexp exposures, nseg segments, npix pixels and ntiles tiles: the new weights [nexp][npix],
// the variances [npix], the medians [nseg], the columns' flags [npix] (int32: kScatDead, kScatKept, kScatClipped); the
// blocks of the column kernel (block columns each) and of the median and weight kernels (one per tile).  grid_ok: every
// launch has at least one block and no more than a grid's 32-bit x extent takes.
struct ScatterExtents {
  int64_t cells = 0, col_blocks = 0, tile_blocks = 0;
  size_t w_bytes = 0, var_bytes = 0, med_bytes = 0, flag_bytes = 0;
  bool grid_ok = false;
};
inline ScatterExtents scatter_extents(int64_t npix, int32_t nexp, int32_t nseg, int64_t ntiles, int block)
{
  ScatterExtents X;
  X.cells = (int64_t)nexp * npix;
  X.col_blocks = (npix + block - 1) / block;
  X.tile_blocks = ntiles;
  X.w_bytes = sizeof(double) * (size_t)X.cells;
  X.var_bytes = sizeof(double) * (size_t)npix;
  X.med_bytes = sizeof(double) * (size_t)nseg;
  X.flag_bytes = sizeof(int32_t) * (size_t)npix;
  X.grid_ok = X.col_blocks >= 1 && X.col_blocks <= 0x7fffffffLL && X.tile_blocks >= 1 && X.tile_blocks <= 0x7fffffffLL;
  return X;
}

// a column's flag: dead (not live), kept, or live and removed by the clip
constexpr int32_t kScatDead = 0, kScatKept = 1, kScatClipped = 2;

// ---- the arithmetic ---------------------------------------------------------------------------------
// one exposure's term of a column's first pass: where W > 0, n = n + 1 and s = s + r
TRX_HD void scatter_sum_term(double W, double r, int32_t &n, double &s)
{
  if (W > 0.0) { n++; s = s + r; }
}

// one exposure's term of the second pass: where W > 0, d = r - mean and q = q + d * d
TRX_HD void scatter_square_term(double W, double r, double mean, double &q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (W > 0.0) {
    const double d = r - mean;
    const double dd = d * d;
    q = q + dd;
  }
}

// whether a column of n entries takes the second pass at all (min_live >= 2: n - 1 >= 1), and its mean
TRX_HD bool scatter_enough(int32_t n, int32_t min_live) { return n >= min_live; }
TRX_HD double scatter_mean(double s, int32_t n) { return s / (double)n; }

// the column's variance q / (n - 1) where the column is live -- n >= min_live, the variance > 0 and finite --, +0 elsewhere
// (so that var > 0 IS the live flag)
TRX_HD double scatter_variance(double q, int32_t n, int32_t min_live)
{
  if (!scatter_enough(n, min_live)) return 0.0;
  const double var = q / (double)(n - 1);
  return var > 0.0 && var <= 1.7976931348623157e308 ? var : 0.0;
}

// The rank of a live candidate p among its segment's live columns, ascending variance, ties by ascending pixel, is counted
// over the segment's variances in trips of up to kScatLds, staged with a dead column's +0 replaced by +infinity: a staged
// value is ahead of a live candidate only if its column is live.
TRX_HD double scatter_staged(double var) { return var > 0.0 ? var : __builtin_huge_val(); }
// the place of pixel p in the trip that starts at pixel q0, clamped to int (a trip's places are 0 .. kScatLds - 1)
TRX_HD int scatter_place(int64_t p, int64_t q0)
{
  const int64_t d = p - q0;
  return d > 0x7fffffffLL ? 0x7fffffff : d < -0x7fffffffLL ? -0x7fffffff : (int)d;
}
// one staged value x, at place j of its trip, against the candidate of variance varp at place pj: ahead counts those ahead
// (no branch: the kernel evaluates kScatTrip of them back to back from registers)
TRX_HD void scatter_rank_term(double x, int j, double varp, int pj, int &ahead)
{
  ahead += (int)((x < varp) | ((x == varp) & (j < pj)));
}
// the staged values are read kScatTrip at a time: a trip of nq values is padded with +infinity to a multiple of it
TRX_HD int scatter_padded(int nq) { return (nq + kScatTrip - 1) / kScatTrip * kScatTrip; }

// whether the live candidate of that rank among m live columns is the lower median
TRX_HD bool scatter_is_median(double varp, int64_t m, int64_t rank) { return varp > 0.0 && rank == (m - 1) / 2; }

// the keep rule: lim = clip * clip, lim = lim * med; kept if live and (clip == 0 or var <= lim)
TRX_HD bool scatter_keep(double var, double med, double clip)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double lim = clip * clip;
  lim = lim * med;
  return var > 0.0 && (clip == 0.0 || var <= lim);
}
TRX_HD int32_t scatter_flag(double var, bool keep) { return keep ? kScatKept : var > 0.0 ? kScatClipped : kScatDead; }

// what a kept column's entries get under TRX_SCATTER_VARIANCE: 1 / var, once per column (+0 for a column not kept)
TRX_HD double scatter_inverse(double var, bool keep) { return keep ? 1.0 / var : 0.0; }

// the new weight of one entry: VARIANCE: inv where W > 0 and the column is kept; MASK: W where it is kept; +0 elsewhere
TRX_HD double scatter_weight(int32_t kind, double W, bool keep, double inv)
{
  if (!keep) return 0.0;
  if (kind == TRX_SCATTER_VARIANCE) return W > 0.0 ? inv : 0.0;
  return W;
}

// ---- one column ---------------------------------------------------------------------------------------
// One column's variance: r its data (entry v at r[v * stride]), w its weights the same way.  HASW: the set has weights
// (without: every W is 1, nothing is loaded for it, w is not read).  A template, decided once per launch: the loads of a trip
// must all be issued before the first is waited for.  Two passes in trips of kSysTrips: the count and the sum, then -- a column
// of enough entries -- the squares about the mean.  The trips are written out here, exposure_trips' loop line for line: through
// the helper the device compiler turns the first term of every trip into a branch of its own (trx_columns.h).
template <bool HASW>
TRX_HD double scatter_column(const double *r, const double *w, int64_t stride, int nexp, int32_t min_live)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int last = nexp - 1;
  int32_t n = 0; double s = 0.0;
  for (int v0 = 0; v0 < nexp; v0 += kSysTrips) {
    WeightedEntry got[kSysTrips];
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < kSysTrips; t++) {
      const int64_t at = (int64_t)(v0 + t < last ? v0 + t : last) * stride;
      got[t] = WeightedEntry{r[at], HASW ? w[at] : 1.0};
    }
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < kSysTrips; t++)
      if (v0 + t < nexp) scatter_sum_term(got[t].w, got[t].f, n, s);
  }
  double q = 0.0;
  if (scatter_enough(n, min_live)) {
    const double mean = scatter_mean(s, n);
    for (int v0 = 0; v0 < nexp; v0 += kSysTrips) {
      WeightedEntry got[kSysTrips];
#if defined(__clang__)
#pragma unroll
#endif
      for (int t = 0; t < kSysTrips; t++) {
        const int64_t at = (int64_t)(v0 + t < last ? v0 + t : last) * stride;
        got[t] = WeightedEntry{r[at], HASW ? w[at] : 1.0};
      }
#if defined(__clang__)
#pragma unroll
#endif
      for (int t = 0; t < kSysTrips; t++)
        if (v0 + t < nexp) scatter_square_term(got[t].w, got[t].f, mean, q);
    }
  }
  return scatter_variance(q, n, min_live);
}

// One column's new weights: the keep rule and 1 / var once, then out[v * stride] for every exposure from the column's own
// weights w (read only where hasw: one answer for the whole launch; without: every W is 1), and the column's flag
TRX_HD void scatter_weights_column(double var, double med, double clip, int32_t kind, const double *w, bool hasw, double *out, int32_t &flag, int64_t stride,
                                   int nexp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool keep = scatter_keep(var, med, clip);
  const double inv = scatter_inverse(var, keep);
  flag = scatter_flag(var, keep);
  exposure_trips<kSysTrips>(
      nexp, [&](int v) { return hasw ? w[(int64_t)v * stride] : 1.0; },
      [&](int v, double W) { out[(int64_t)v * stride] = scatter_weight(kind, W, keep, inv); });
}

}  // namespace trx
