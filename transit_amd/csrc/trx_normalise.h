// trx_normalise.h -- the host side and the arithmetic of normalising the observed set on the device (trx_set_normalise,
// trx_normalise_observed and step 1b of trx_detrend_observed and trx_pca_observed, include/transit_hip.h): what the calls
// refuse, the extents of the step's buffers, its launch sizes, and the arithmetic -- the order-preserving key
// of a double and one step of its bisection, the rank of a quantile, the row scale, a column's sums, its centre, the
// centred entry and the clip -- as plain host/device functions.  Plain C++ (no HIP): the kernels of
// hip/trx_normalise.hip.h call the functions per lane, tests/normalise_check.cpp runs the same source on the CPU over
// exact-size arrays.  Every operation is an IEEE double operation rounded once -- no fused multiply-add -- in the order
// transit_amd/xcor.py (normalise_reference) writes it.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "transit_hip.h"
#include "trx_launch.h"
#include "trx_numerics.h"
#include "trx_products.h"
#include "trx_sysrem.h"

namespace trx {

constexpr int kNormBlock = 256;                       // lanes of the row kernel's block: one block per (exposure, segment) row
constexpr int kNormPerLane = 8;                       // keys of the row a lane of that block keeps in registers
constexpr int kNormCap = kNormBlock * kNormPerLane;   // the staging capacity: pixels of a row whose keys stay in registers (2048);
                                                      // the pixels past it are read from global memory again at every step
constexpr int kNormWaves = 4;                         // tiles (waves) per block of the column kernel
constexpr int kNormBits = 64;                         // steps of the bisection: one per bit of the key, from the top one down

// ---- the calls: checks, tiles, extents --------------------------------------------------------------
// What trx_set_normalise refuses, in the header's order.  A NULL nm (clear) is checked for the observed set and the shard alone.
inline int normalise_set_checks(const ProductState &S, const trx_normalise *nm, std::string &msg)
{
  const char *const who = "trx_set_normalise";
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (nm) {
    if (nm->row_kind < TRX_NORM_ROW_NONE || nm->row_kind > TRX_NORM_ROW_QUANTILE) return no(TRX_E_ARG, "row_kind must be TRX_NORM_ROW_NONE or _QUANTILE");
    if (nm->col_kind < TRX_NORM_COL_NONE || nm->col_kind > TRX_NORM_COL_SUBTRACT) return no(TRX_E_ARG, "col_kind must be TRX_NORM_COL_NONE, _DIVIDE, _RATIO or _SUBTRACT");
    if (!std::isfinite(nm->quantile) || nm->quantile < 0.0 || nm->quantile > 1.0) return no(TRX_E_ARG, "quantile must be finite and in [0, 1]");
    if (!std::isfinite(nm->clip)) return no(TRX_E_ARG, "clip must be finite");
    if (nm->clip < 0.0) return no(TRX_E_ARG, "clip < 0");
    if (nm->clip > 0.0 && nm->clip < 1.0) return no(TRX_E_ARG, "clip must be 0 (none) or at least 1");
    if (nm->row_kind == TRX_NORM_ROW_NONE && nm->col_kind == TRX_NORM_COL_NONE && nm->clip == 0.0)
      return no(TRX_E_ARG, "a recipe that does nothing (pass NULL to clear)");
  }
  if (S.windowed) return no(TRX_E_UNSUPPORTED, "this handle's shard is not the whole grid; normalise on the host (xcor.normalise_reference)");
  return TRX_OK;
}

// What trx_normalise_observed refuses, in the header's order: no observed set, no recipe, then the injection's arguments
// and the shard as trx_detrend_observed has them.
inline int normalise_checks(const ProductState &S, bool recipe, int32_t inject, double p0, double p1, const void *a, const void *o, int32_t nshift,
                            const double *shift, std::string &msg)
{
  const char *const who = "trx_normalise_observed";
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (!recipe) return no(TRX_E_ARG, "no recipe installed (trx_set_normalise)");
  return detrend_inject_checks(who, "xcor.normalise_reference", S, inject, 0, p0, p1, a, o, nshift, shift, msg);
}

// The extents of step 1b over nexp exposures, nseg segments, npix pixels and ntiles tiles (sysrem_tiles': the column kernel's
// column -> segment map, one wave per tile): the data [nexp][npix], the row
// scales [nexp][nseg], the centres [npix], the two counts of every column [2][npix] (int32: clipped, then bad); the blocks
// of the row kernel (one per row (v, s)) and of the column kernel (tiles_per_block tiles each).  grid_ok: every launch has at
// least one block and no more than a grid's 32-bit x extent takes.
struct NormExtents {
  int64_t cells = 0, rows = 0, row_blocks = 0, tile_blocks = 0;
  size_t r_bytes = 0, scale_bytes = 0, centre_bytes = 0, count_bytes = 0;
  bool grid_ok = false;
};
inline NormExtents normalise_extents(int64_t npix, int32_t nexp, int32_t nseg, int64_t ntiles, int tiles_per_block)
{
  NormExtents X;
  X.cells = (int64_t)nexp * npix; X.rows = (int64_t)nexp * nseg;
  X.row_blocks = X.rows;
  X.tile_blocks = (ntiles + tiles_per_block - 1) / tiles_per_block;
  X.r_bytes = sizeof(double) * (size_t)X.cells;
  X.scale_bytes = sizeof(double) * (size_t)X.rows;
  X.centre_bytes = sizeof(double) * (size_t)npix;
  X.count_bytes = sizeof(int32_t) * 2 * (size_t)npix;
  X.grid_ok = grid_ok(X.row_blocks) && grid_ok(X.tile_blocks);
  return X;
}

// ---- the selection ----------------------------------------------------------------------------------
// The order-preserving key of a double: every bit of a negative value flipped, the sign bit of the others -- as unsigned
// integers the keys stand in the order of the values (-0 just below +0), and the transform has an inverse.
TRX_HD uint64_t norm_key(double x)
{
  uint64_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = (uint64_t)__double_as_longlong(x);
#else
  std::memcpy(&b, &x, sizeof b);
#endif
  return (b >> 63) ? ~b : b ^ 0x8000000000000000ULL;
}
TRX_HD double norm_unkey(uint64_t k)
{
  const uint64_t b = (k >> 63) ? k ^ 0x8000000000000000ULL : ~k;
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)b);
#else
  double x;
  std::memcpy(&x, &b, sizeof x);
  return x;
#endif
}
// what a dead entry is staged as: above every trial of the bisection, counted by none
constexpr uint64_t kNormDeadKey = ~0ULL;
TRX_HD uint64_t norm_staged(double W, double f) { return W > 0.0 ? norm_key(f) : kNormDeadKey; }

// the rank of the quantile among m >= 1 live values, 0-based and ascending: (int64) floor(quantile * (double)(m - 1))
TRX_HD int64_t norm_rank(double quantile, int64_t m)
{
  return (int64_t)std::floor(quantile * (double)(m - 1));
}

// One step of the bisection for the key of rank k.  `found` holds the bits above `bit` of the answer; the trial sets `bit`
// in it; `below` is the number of live keys under the trial.  The bit stays where no more than k keys are below the trial:
// after bit 0 `found` is the largest key with at most k keys below it, which is the key of rank k itself.
TRX_HD uint64_t norm_trial(uint64_t found, int bit) { return found | (1ULL << bit); }
TRX_HD uint64_t norm_bisect_step(uint64_t found, int bit, int64_t below, int64_t k) { return below <= k ? norm_trial(found, bit) : found; }
// whether a staged key counts under a trial (a dead entry's never does: no trial is above it)
TRX_HD bool norm_below(uint64_t key, uint64_t trial) { return key < trial; }

// ---- the arithmetic ---------------------------------------------------------------------------------
// the scale of a row of m live values whose value of rank k is x (QUANTILE): x where the row is good -- m >= 1 and x > 0 --,
// +0 elsewhere (-0 and NaN included); with row_kind NONE 1.0 where m >= 1.  scale > 0 IS the row's good flag.
TRX_HD double norm_scale(int32_t row_kind, double x, int64_t m)
{
  if (m < 1) return 0.0;
  if (row_kind == TRX_NORM_ROW_NONE) return 1.0;
  return x > 0.0 ? x : 0.0;
}
// f1 of an entry of a good row: f0 / scale, or f0 with row_kind NONE
TRX_HD double norm_row(int32_t row_kind, double f0, double scale) { return row_kind == TRX_NORM_ROW_QUANTILE ? f0 / scale : f0; }
// whether an entry takes part: live, in a good row
TRX_HD bool norm_on(double W, double scale) { return W > 0.0 && scale > 0.0; }

// one exposure's term of a column's sum: where the entry takes part, n = n + 1 and s = s + f
TRX_HD void norm_sum_term(bool on, double f, int32_t &n, double &s)
{
  if (on) { n++; s = s + f; }
}
TRX_HD double norm_mean(double s, int32_t n) { return s / (double)n; }

// the column's centre s / (double)n and whether the column is good: n >= 1 and, under DIVIDE and RATIO, c > 0 and finite,
// under SUBTRACT c finite; +0 for a column that is not good
TRX_HD double norm_centre(int32_t col_kind, double s, int32_t n, bool &good)
{
  good = false;
  if (n < 1) return 0.0;
  const double c = norm_mean(s, n);
  const bool finite = c >= -1.7976931348623157e308 && c <= 1.7976931348623157e308;
  good = col_kind == TRX_NORM_COL_NONE ? true : col_kind == TRX_NORM_COL_SUBTRACT ? finite : (c > 0.0 && finite);
  return good ? c : 0.0;
}

// f2 of an entry of a good column: f1 / c;  t = f1 / c, t - 1.0;  f1 - c;  or f1
TRX_HD double norm_col(int32_t col_kind, double f1, double c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (col_kind == TRX_NORM_COL_DIVIDE) return f1 / c;
  if (col_kind == TRX_NORM_COL_RATIO) { const double t = f1 / c; return t - 1.0; }
  if (col_kind == TRX_NORM_COL_SUBTRACT) return f1 - c;
  return f1;
}
// f2 of an entry from its datum: both steps
TRX_HD double norm_entry(int32_t row_kind, int32_t col_kind, double f0, double scale, double c) { return norm_col(col_kind, norm_row(row_kind, f0, scale), c); }

// the clip, in trx_scatter.h's arithmetic: d = f2 - mean, dd = d * d, q = q + dd;  var = q / (double)(n - 1);
// lim = clip * clip, lim = lim * var;  an entry with d * d > lim is replaced by the mean
TRX_HD bool norm_clips(double clip, int32_t n, bool good) { return clip > 0.0 && good && n >= 2; }
TRX_HD double norm_dev2(double f2, double mean)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = f2 - mean;
  return d * d;
}
TRX_HD void norm_square_term(bool on, double f2, double mean, double &q)
{
  if (on) q = q + norm_dev2(f2, mean);
}
TRX_HD double norm_limit(double clip, double q, int32_t n)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double var = q / (double)(n - 1);
  double lim = clip * clip;
  lim = lim * var;
  return lim;
}
TRX_HD bool norm_clipped(double f2, double mean, double lim) { return norm_dev2(f2, mean) > lim; }

// ---- one column ---------------------------------------------------------------------------------------
// what a trip loads of an exposure: the datum f0, its weight and its row's scale
struct NormEntry { double f, w, sc; };

// One column p: r the set's data (the column's entry v at r[v * stride + p]: the arrays whole and the column's number, not a
// pointer per lane -- that form costs this kernel registers enough to lose a wave), w its weights the same way, scale the
// column's segment's row scales (exposure v's at scale[v * sstride]).  HASW: the set has weights (without: every W is 1, nothing
// is loaded for it, w is not read).  A template, decided once per launch: the loads of a trip must all be issued before the
// first is waited for.  Every pass takes the exposures in trips of kSysTrips, written out here, exposure_trips' loop line for
// line: through the helper the device compiler turns terms of a trip into branches of their own (trx_columns.h).  norm_trip
// loads the trip that starts at v0.
template <bool HASW>
TRX_HD void norm_trip(const double *r, const double *w, const double *scale, int64_t p, int64_t stride, int64_t sstride, int nexp, int v0,
                      NormEntry (&got)[kSysTrips])
{
  const int last = nexp - 1;
#if defined(__clang__)
#pragma unroll
#endif
  for (int t = 0; t < kSysTrips; t++) {
    const int v = v0 + t < last ? v0 + t : last;
    const int64_t at = (int64_t)v * stride + p;
    got[t] = NormEntry{r[at], HASW ? w[at] : 1.0, scale[(int64_t)v * sstride]};
  }
}

// PASS 0: n and the sum of f1; 1: the sum of f2; 2: the squares of f2 about the mean
template <bool HASW, int PASS>
TRX_HD void norm_column_pass(const double *r, const double *w, const double *scale, int64_t p, int64_t stride, int64_t sstride, int nexp, int32_t row_kind,
                             int32_t col_kind, double c, double mean, int32_t &n, double &acc)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int v0 = 0; v0 < nexp; v0 += kSysTrips) {
    NormEntry got[kSysTrips];
    norm_trip<HASW>(r, w, scale, p, stride, sstride, nexp, v0, got);
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < kSysTrips; t++)
      if (v0 + t < nexp) {
        const NormEntry &x = got[t];
        const bool on = norm_on(x.w, x.sc);
        // (an entry that takes no part is not divided: its scale may be +0)
        if (PASS == 0) norm_sum_term(on, on ? norm_row(row_kind, x.f, x.sc) : 0.0, n, acc);
        else if (PASS == 1) { int32_t unused = 0; norm_sum_term(on, on ? norm_entry(row_kind, col_kind, x.f, x.sc, c) : 0.0, unused, acc); }
        else norm_square_term(on, on ? norm_entry(row_kind, col_kind, x.f, x.sc, c) : 0.0, mean, acc);
      }
  }
}

// The column in place: the sum of f1 over the entries that take part and the centre, with a clip the mean and the squares of
// f2, then the pass that writes f2 -- the mean where the clip takes the entry, +0 where the entry is dead or its row or column
// bad.  Every pass forms f1 and f2 again from f0: the same operations, the same bits.  centre: the column's centre; nclip, nbad:
// the entries the clip replaced, the live entries that got +0
template <bool HASW>
TRX_HD void norm_column(double *r, const double *w, const double *scale, int64_t p, int64_t stride, int64_t sstride, int nexp, int32_t row_kind, int32_t col_kind,
                        double clip, double &centre, int32_t &nclip_out, int32_t &nbad_out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int32_t n = 0; double s = 0.0;
  norm_column_pass<HASW, 0>(r, w, scale, p, stride, sstride, nexp, row_kind, col_kind, 0.0, 0.0, n, s);
  bool good;
  const double c = norm_centre(col_kind, s, n, good);
  const bool clips = norm_clips(clip, n, good);
  double mean = 0.0, lim = 0.0;
  if (clips) {
    int32_t unused = 0; double s2 = 0.0, q = 0.0;
    norm_column_pass<HASW, 1>(r, w, scale, p, stride, sstride, nexp, row_kind, col_kind, c, 0.0, unused, s2);
    mean = norm_mean(s2, n);
    norm_column_pass<HASW, 2>(r, w, scale, p, stride, sstride, nexp, row_kind, col_kind, c, mean, unused, q);
    lim = norm_limit(clip, q, n);
  }
  int32_t nclip = 0, nbad = 0;
  for (int v0 = 0; v0 < nexp; v0 += kSysTrips) {
    NormEntry got[kSysTrips];
    norm_trip<HASW>(r, w, scale, p, stride, sstride, nexp, v0, got);
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < kSysTrips; t++)
      if (v0 + t < nexp) {
        const NormEntry &x = got[t];
        const bool on = norm_on(x.w, x.sc) && good;
        double out = 0.0;
        if (on) {
          out = norm_entry(row_kind, col_kind, x.f, x.sc, c);
          if (clips && norm_clipped(out, mean, lim)) { out = mean; nclip++; }
        } else if (x.w > 0.0) nbad++;
        r[(int64_t)(v0 + t) * stride + p] = out;
      }
  }
  centre = c;
  nclip_out = nclip;
  nbad_out = nbad;
}

}  // namespace trx
