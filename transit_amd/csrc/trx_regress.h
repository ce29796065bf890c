// trx_regress.h -- the host side and the arithmetic of regressing the observed set on given time vectors on the device
// (trx_regress_observed, include/transit_hip.h): what the call refuses, the extents of its buffers and its launch sizes, the
// merge of the given vectors with the fitted ones, and the fit of one column as a plain host/device function.  Plain C++ (no
// HIP): the kernel of hip/trx_regress.hip.h calls regress_column per lane, tests/regress_check.cpp runs the same source on
// the CPU over exact-size arrays.  The arithmetic is ../trx_wfilter.h's, every line of it: the right-hand side
// (wfilter_rhs_term), the solve (wfilter_solve) and the value (wfilter_value) with g = f0 -- what the weighted filter does
// to the model, done to the data, by the factor k_wfilter_factor made.  Nothing is added to it here.
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "transit_hip.h"
#include "trx_launch.h"
#include "trx_numerics.h"
#include "trx_products.h"
#include "trx_sysrem.h"
#include "trx_wfilter.h"

namespace trx {

constexpr int kRegressTrips = 4;                      // exposures whose loads a lane has in flight at once (kFiltTrips)

// ---- the call: checks, extents, the merged basis -----------------------------------------------------
// Whether the call is the undo (rg NULL or nvec = 0): the raw data back, the filter slot cleared.
inline bool regress_is_undo(const trx_regress *rg) { return !rg || rg->nvec == 0; }

// What trx_regress_observed refuses, in the header's order.  The undo is checked for the observed set (and nvec's sign)
// alone; a call that regresses for everything.
inline int regress_checks(const ProductState &S, const trx_regress *rg, const void *a, const void *o, int32_t nshift, const double *shift, std::string &msg)
{
  const char *const who = "trx_regress_observed";
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (!rg) return TRX_OK;
  if (rg->nvec < 0) return no(TRX_E_ARG, "nvec < 0");
  if (rg->nvec > TRX_FILTER_MAX) return no(TRX_E_ARG, "nvec above TRX_FILTER_MAX (" + std::to_string(TRX_FILTER_MAX) + ")");
  if (rg->nvec == 0) return TRX_OK;
  if (rg->nfit < 0) return no(TRX_E_ARG, "nfit < 0");
  if (rg->nvec + rg->nfit > TRX_FILTER_MAX) return no(TRX_E_ARG, "nvec + nfit above TRX_FILTER_MAX (" + std::to_string(TRX_FILTER_MAX) + ")");
  if (rg->nfit > 0) {
    if (rg->niter < 1) return no(TRX_E_ARG, "niter < 1");
    if (rg->niter > TRX_SYSREM_MAX_ITER) return no(TRX_E_ARG, "niter above TRX_SYSREM_MAX_ITER (" + std::to_string(TRX_SYSREM_MAX_ITER) + ")");
  }
  if (!rg->vectors) return no(TRX_E_ARG, "NULL vectors array");
  const size_t per = (size_t)rg->nvec * (size_t)S.nexp;
  for (int32_t s = 0; s < S.nseg; s++)
    for (size_t k = 0; k < per; k++)
      if (!std::isfinite(rg->vectors[(size_t)s * per + k])) return no(TRX_E_ARG, "segment " + std::to_string(s) + ": vectors entry must be finite");
  return detrend_inject_checks(who, "xcor.regress_reference", S, rg->inject, 0, rg->p0, rg->p1, a, o, nshift, shift, msg);
}

// The extents of a call of nvec given vectors and nfit fitted components over nexp exposures, nseg segments, npix pixels and
// ntiles tiles (sysrem_tiles'): the data [nexp][npix], coef [nvec + nfit][npix] with the fitted components' rows behind
// coef_fit_bytes, the merged basis [nseg][nexp][nvec + nfit]; the blocks of the column kernel (tiles_per_block tiles each).
// grid_ok: the launch has at least one block and no more than a grid's 32-bit x extent takes.
struct RegressExtents {
  int32_t ncomp = 0;
  int64_t cells = 0, tile_blocks = 0;
  size_t r_bytes = 0, coef_bytes = 0, coef_fit_bytes = 0, basis_bytes = 0;
  bool grid_ok = false;
};
inline RegressExtents regress_extents(int64_t npix, int32_t nexp, int32_t nseg, int32_t nvec, int32_t nfit, int64_t ntiles, int tiles_per_block)
{
  RegressExtents X;
  X.ncomp = nvec + nfit;
  X.cells = (int64_t)nexp * npix;
  X.tile_blocks = (ntiles + tiles_per_block - 1) / tiles_per_block;
  X.r_bytes = sizeof(double) * (size_t)X.cells;
  X.coef_bytes = sizeof(double) * (size_t)X.ncomp * (size_t)npix;
  X.coef_fit_bytes = sizeof(double) * (size_t)nvec * (size_t)npix;
  X.basis_bytes = sizeof(double) * (size_t)nseg * (size_t)nexp * (size_t)X.ncomp;
  X.grid_ok = grid_ok(X.tile_blocks);
  return X;
}

// B[s][v] = (given[s][v][0 .. nvec), fit[s][v][0 .. nfit)): the basis the call installs, [nseg][nexp][nvec + nfit]
// (fit may be null where nfit = 0)
inline void regress_merge(const double *given, const double *fit, int32_t nseg, int32_t nexp, int32_t nvec, int32_t nfit, double *out)
{
  const size_t n = (size_t)nvec + (size_t)nfit;
  for (size_t sv = 0; sv < (size_t)nseg * (size_t)nexp; sv++) {
    for (int32_t j = 0; j < nvec; j++) out[sv * n + (size_t)j] = given[sv * (size_t)nvec + (size_t)j];
    for (int32_t i = 0; i < nfit; i++) out[sv * n + (size_t)nvec + (size_t)i] = fit[sv * (size_t)nfit + (size_t)i];
  }
}

// ---- one column ---------------------------------------------------------------------------------------
// The fit of one column of n components: U its segment's padded vectors [nexp][NC], w the column's weights (entry v at
// w[v * stride]; without hasw: all 1), r its data f0 in and its residuals out (entry v at r[v * stride]), fac its factor (entry e at
// fac[e * stride]), live whether no pivot of it was singular, coef its coefficients out (component j at coef[j * stride]).
//   pass 1   y_j = sum over v ascending of (U[v][j] * w[v]) * f0[v]               (wfilter_rhs_term)
//   solve    c = the factor's forward and back solve of y                        (wfilter_solve); a column with a singular
//            pivot: c_j = +0 for every j, the solve's result is not used
//   pass 2   r[v] = f0[v] - (sum over j ascending of U[v][j] * c_j), every v     (wfilter_value)
// Both passes take the exposures in exposure_trips' trips of kRegressTrips (trx_columns.h).  w is read only where hasw: the set
// has weights -- one answer for the whole launch, never a test of a lane's own pointer.
template <int NC>
TRX_HD void regress_column(const double *U, const double *w, bool hasw, double *r, const double *fac, bool live, double *coef, int64_t stride, int nexp, int n)
{
  double y[NC];
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < NC; j++) y[j] = 0.0;
  exposure_trips<kRegressTrips>(
      nexp, [&](int v) { return WeightedEntry{r[(int64_t)v * stride], hasw ? w[(int64_t)v * stride] : 1.0}; },
      [&](int v, const WeightedEntry &x) { wfilter_rhs_term<NC>(U + (int64_t)v * NC, x.w, x.f, y); });
  wfilter_solve<NC>(n, y, fac, stride);
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < NC; j++) {
    y[j] = live ? y[j] : 0.0;
    if (j < n) coef[(int64_t)j * stride] = y[j];
  }
  exposure_trips<kRegressTrips>(
      nexp, [&](int v) { return r[(int64_t)v * stride]; },
      [&](int v, double f) { r[(int64_t)v * stride] = wfilter_value<NC>(U + (int64_t)v * NC, y, f); });
}
// the same for a caller that holds one column's weights or none (w null: all 1) -- a host caller: one column, one answer
template <int NC>
TRX_HD void regress_column(const double *U, const double *w, double *r, const double *fac, bool live, double *coef, int64_t stride, int nexp, int n)
{
  regress_column<NC>(U, w, w != nullptr, r, fac, live, coef, stride, nexp, n);
}

}  // namespace trx
