// trx_sysrem.h -- the host side and the arithmetic of detrending the observed set on the device (trx_detrend_observed,
// include/transit_hip.h): what the call refuses, the tiles and the extents of its buffers, its launch counts, and the
// arithmetic -- the injection, SYSREM's column step, row step and close -- as plain host/device functions.  Plain C++ (no
// HIP): the kernels of hip/trx_sysrem.hip.h call the functions per lane, tests/sysrem_check.cpp runs the same source on the
// CPU over exact-size arrays.  Every operation is an IEEE double operation rounded once -- no fused multiply-add -- in the
// order transit_amd/xcor.py (inject_reference, sysrem_reference) writes it.
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

// ---- the call: checks, tiles, extents ---------------------------------------------------------------
// Whether the call is the undo (dt NULL or ncomp = 0): the raw data back, the filter slot cleared.
inline bool detrend_is_undo(const trx_detrend *dt) { return !dt || dt->ncomp == 0; }

// What the injection's part of a detrending call refuses, and the shard after it: inject, pad, p0, p1, a, o, the shifts.  who:
// the call that names itself in the text; mirror: the host routine the shard's refusal points to.
inline int detrend_inject_checks(const char *who, const char *mirror, const ProductState &S, int32_t inject, int32_t pad, double p0, double p1,
                                 const void *a, const void *o, int32_t nshift, const double *shift, std::string &msg)
{
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (inject != 0 && inject != 1) return no(TRX_E_ARG, "inject must be 0 or 1");
  if (pad != 0) return no(TRX_E_ARG, "pad must be 0");
  if (inject) {
    if (!std::isfinite(p0)) return no(TRX_E_ARG, "p0 must be finite");
    if (!std::isfinite(p1)) return no(TRX_E_ARG, "p1 must be finite");
    if (!a) return no(TRX_E_ARG, "a is NULL");
    if (!o) return no(TRX_E_ARG, "o is NULL");
    if (!shift) return no(TRX_E_ARG, "shift is NULL");
    if (nshift != S.nexp) return no(TRX_E_ARG, "nshift " + std::to_string(nshift) + " is not the observed set's nexp " + std::to_string(S.nexp));
    if (const int rc = pixel_run_checks(who, nshift, S.npix, shift, msg)) return rc;
  }
  // (the injection's pairs are a run's: the partial pairs of a shard are not the model)
  if (S.windowed) return no(TRX_E_UNSUPPORTED, std::string("this handle's shard is not the whole grid; detrend on the host (") + mirror + ")");
  return TRX_OK;
}

// What trx_detrend_observed refuses, in the header's order.  The undo is checked for the observed set (and ncomp's sign)
// alone; a call that detrends for everything.
inline int detrend_checks(const ProductState &S, const trx_detrend *dt, const void *a, const void *o, int32_t nshift, const double *shift, std::string &msg)
{
  const char *const who = "trx_detrend_observed";
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (!dt) return TRX_OK;
  if (dt->ncomp < 0) return no(TRX_E_ARG, "ncomp < 0");
  if (dt->ncomp > TRX_FILTER_MAX) return no(TRX_E_ARG, "ncomp above TRX_FILTER_MAX (" + std::to_string(TRX_FILTER_MAX) + ")");
  if (dt->ncomp == 0) return TRX_OK;
  if (dt->niter < 1) return no(TRX_E_ARG, "niter < 1");
  if (dt->niter > TRX_SYSREM_MAX_ITER) return no(TRX_E_ARG, "niter above TRX_SYSREM_MAX_ITER (" + std::to_string(TRX_SYSREM_MAX_ITER) + ")");
  return detrend_inject_checks(who, "xcor.sysrem_reference", S, dt->inject, dt->pad, dt->p0, dt->p1, a, o, nshift, shift, msg);
}

// The tiles of the observed set's segments, filter_layout's: up to 64 consecutive pixels of one segment each, a segment's
// tiles in pixel order.  They give the column kernels their column -> segment map (who: the call that names itself in a refusal).
inline int sysrem_tiles(const ProductState &S, std::vector<FilterTile> &tiles, std::string &msg, const char *who = "trx_detrend_observed")
{
  try {
    tiles.clear();
    for (int32_t s = 0; s < S.nseg; s++)
      for (int64_t p = S.seg[(size_t)s]; p < S.seg[(size_t)s + 1]; p += 64)
        tiles.push_back(FilterTile{p, s, (int32_t)std::min<int64_t>(64, S.seg[(size_t)s + 1] - p)});
  } catch (...) { return refuse(msg, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  return TRX_OK;
}

// The extents of steps 0 and 1 of a detrending call -- the raw or the injected data into the call's buffer --, whatever the
// call fits afterwards: the cells of [nexp][npix], the bytes of the residuals r and of a vector of one double per pixel (the
// gains the injection reads; SYSREM's c), the blocks of the element-wise kernel (elem_block cells each).
struct FillExtents { int64_t cells = 0, elem_blocks = 0; size_t r_bytes = 0, c_bytes = 0; };
inline FillExtents fill_extents(int64_t npix, int32_t nexp, int elem_block)
{
  FillExtents X;
  X.cells = (int64_t)nexp * npix;
  X.elem_blocks = (X.cells + elem_block - 1) / elem_block;
  X.r_bytes = sizeof(double) * (size_t)X.cells;
  X.c_bytes = sizeof(double) * (size_t)npix;
  return X;
}

// The extents of a detrend call of ncomp components and niter alternations over nexp exposures, nseg segments, npix pixels
// and ntiles tiles: the residuals r [nexp][npix], the time vector a [nseg][nexp], the column vector c [npix], coef
// [ncomp][npix] and U [nseg][nexp][ncomp]; the blocks of the element-wise kernel (elem_block cells each), of the column
// kernels (tiles_per_block tiles each) and of the row kernel (rows_per_block rows (v, s) each); the launches of the
// SYSREM kernels -- per component niter column steps, niter row steps, the close and the subtract.
struct SysremExtents {
  int64_t cells = 0, rows = 0, elem_blocks = 0, tile_blocks = 0, row_blocks = 0, launches = 0;
  size_t r_bytes = 0, a_bytes = 0, c_bytes = 0, coef_bytes = 0, basis_bytes = 0;
};
inline SysremExtents sysrem_extents(int64_t npix, int32_t nexp, int32_t nseg, int32_t ncomp, int32_t niter, int64_t ntiles, int elem_block,
                                    int tiles_per_block, int rows_per_block)
{
  SysremExtents X;
  const FillExtents F = fill_extents(npix, nexp, elem_block);
  X.cells = F.cells; X.elem_blocks = F.elem_blocks; X.r_bytes = F.r_bytes; X.c_bytes = F.c_bytes;
  X.rows = (int64_t)nexp * nseg;
  X.tile_blocks = (ntiles + tiles_per_block - 1) / tiles_per_block;
  X.row_blocks = (X.rows + rows_per_block - 1) / rows_per_block;
  X.launches = (int64_t)ncomp * (2 * (int64_t)niter + 2);
  X.a_bytes = sizeof(double) * (size_t)X.rows;
  X.coef_bytes = sizeof(double) * (size_t)ncomp * (size_t)npix;
  X.basis_bytes = sizeof(double) * (size_t)X.rows * (size_t)ncomp;
  return X;
}

// the first non-finite entry of U [nseg][nexp][ncomp] names the call's refusal (who: the call, trx_pca_observed's too)
inline int sysrem_basis_check(const double *U, int32_t nseg, int32_t nexp, int32_t ncomp, std::string &msg, const char *who = "trx_detrend_observed")
{
  for (int32_t s = 0; s < nseg; s++)
    for (int32_t v = 0; v < nexp; v++)
      for (int32_t i = 0; i < ncomp; i++)
        if (!std::isfinite(U[((size_t)s * (size_t)nexp + (size_t)v) * (size_t)ncomp + (size_t)i]))
          return refuse(msg, TRX_E_ARG, std::string(who) + ": component " + std::to_string(i) + " of segment " + std::to_string(s) + " is not finite");
  return TRX_OK;
}

// ---- the arithmetic ---------------------------------------------------------------------------------
// the injected datum: F * (p0 * g + p1) with g = gain * (a / b) where b > 0, F elsewhere
TRX_HD double sysrem_inject(double F, double a, double b, double gain, double p0, double p1)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(b > 0.0)) return F;
  const double g = gain * (a / b);
  double m = p0 * g;
  m = m + p1;
  return F * m;
}

// one exposure's terms of a column: num += (w * r) * a_v, den += (w * a_v) * a_v
TRX_HD void sysrem_col_term(double w, double r, double av, double &num, double &den)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  num += (w * r) * av;
  den += (w * av) * av;
}

// one pixel's terms of a row: num += (w * r) * c_p, den += (w * c_p) * c_p
TRX_HD void sysrem_row_term(double w, double r, double c, double &num, double &den)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  num += (w * r) * c;
  den += (w * c) * c;
}

// num / den where den > 0, +0 elsewhere (den = 0 and NaN included)
TRX_HD double sysrem_ratio(double num, double den) { return den > 0.0 ? num / den : 0.0; }

// the close's norm of a [nexp]: sqrt of the sum, ascending from +0, of a_v * a_v
TRX_HD double sysrem_norm(const double *a, int nexp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double n2 = 0.0;
  for (int v = 0; v < nexp; v++) n2 += a[v] * a[v];
  return std::sqrt(n2);
}
// a_v and c_p as the close leaves them: a_v / t and c_p * t where t > 0, as they are elsewhere
TRX_HD double sysrem_close_a(double av, double t) { return t > 0.0 ? av / t : av; }
TRX_HD double sysrem_close_c(double c, double t) { return t > 0.0 ? c * t : c; }

// the residual after a component: r - a_v * c_p
TRX_HD double sysrem_subtract(double r, double av, double c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m = av * c;
  return r - m;
}

// ---- one column -------------------------------------------------------------------------------------
// The column step of one column: r its residuals (entry v at r[v * stride]), w its weights the same way (read only where
// hasw: the set has weights -- one answer for the whole launch, never a test of a lane's own pointer; without: every w is 1),
// a its segment's time vector [nexp] (null: every a_v = 1, a component's first step).  v ascends, exposure_trips' way,
// kSysTrips at a time.
TRX_HD double sysrem_column_step(const double *r, const double *w, bool hasw, const double *a, int64_t stride, int nexp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double num = 0.0, den = 0.0;
  exposure_trips<kSysTrips>(
      nexp, [&](int v) { return WeightedEntry{r[(int64_t)v * stride], hasw ? w[(int64_t)v * stride] : 1.0}; },
      [&](int v, const WeightedEntry &x) { sysrem_col_term(x.w, x.f, a ? a[v] : 1.0, num, den); });
  return sysrem_ratio(num, den);
}

// The subtract of one column, in place: r[v] = r[v] - U_v * c with U_v at U[v * ustride] (its segment's component), every v
TRX_HD void sysrem_column_subtract(double *r, const double *U, int64_t ustride, double c, int64_t stride, int nexp)
{
  exposure_trips<kSysTrips>(
      nexp, [&](int v) { return r[(int64_t)v * stride]; },
      [&](int v, double f) { r[(int64_t)v * stride] = sysrem_subtract(f, U[(int64_t)v * ustride], c); });
}

// wave_sum's butterfly over 64 lane sums on the host: every lane adds its partner lane ^ 32, 16, 8, 4, 2, 1 in that order;
// lane 0's total (every lane holds the same bits: the addition commutes)
inline double sysrem_wave_sum_host(const double (&lanes)[64])
{
  double x[64], y[64];
  for (int l = 0; l < 64; l++) x[l] = lanes[l];
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < 64; l++) y[l] = x[l] + x[l ^ o];
    for (int l = 0; l < 64; l++) x[l] = y[l];
  }
  return x[0];
}

}  // namespace trx
