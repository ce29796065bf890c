// trx_exposures.h -- the host side of the exposure table (trx_set_exposures, trx_run_exposed; include/transit_hip.h) and the
// range rule its pixel kernel shares with the host: the bins of a pixel's window at one exposure -- the Gaussian's cut
// widened by the half-width of the Doppler smear --, what the two calls refuse, and the extents of the table's device
// arrays.  Plain C++ (no HIP): k_pixel_pairs_exposed (hip/trx_pixels.hip.h) calls exposed_range, trx_api.hip checks and
// sizes with the rest, and tests/exposures_check.cpp runs the same source on the CPU over exact-size buffers.
#pragma once
#include <math.h>
#include <stdint.h>

#include <string>

#include "transit_hip.h"
#include "trx_numerics.h"
#include "trx_products.h"

namespace trx {

// The rest-frame window of pixel (centre_obs, fwhm_obs) at `shift` with smear half-width eta: centre, sigma, the box's
// half-width d = centre * eta in cm-1 (eta == 0: exactly 0) and the bins [first, last) of the whole grid within
// r = cut * sigma + d of the centre.  IEEE double, every operation rounded once -- no fused multiply-add --, so that host
// and device get the same integers; clipped to [0, nwn] in double: no conversion of a value out of int64's range, and a
// NaN edge (a shift so small that the centre overflows) gives no bin.  With eta == 0 these are the bins of the plain pixel
// kernel's pixel_range, operation for operation.
TRX_HD void exposed_range(double wn_i, double wn_d, int64_t nwn, double cut, double fwhm_sigma, double centre_obs, double fwhm_obs,
                          double shift, double eta, double &centre, double &sigma, double &d, int64_t &first, int64_t &last)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  centre = centre_obs / shift;
  const double fwhm = fwhm_obs / shift;
  sigma = fwhm / fwhm_sigma;
  d = eta > 0.0 ? centre * eta : 0.0;
  const double r = cut * sigma + d;
  const double a = ceil((centre - r - wn_i) / wn_d);
  const double z = floor((centre + r - wn_i) / wn_d) + 1.0;
  const double n = (double)nwn;
  if (!(a == a) || !(z == z)) { first = last = 0; return; }
  first = a <= 0 ? 0 : a >= n ? nwn : (int64_t)a;
  last = z <= 0 ? 0 : z >= n ? nwn : (int64_t)z;
  if (last < first) last = first;
}

// a table that is not a clearing call (ex non-null, nexp != 0)
inline int exposure_set_checks(const ProductState &S, const trx_exposures *ex, std::string &msg)
{
  if (S.npix < 1 || !S.seg) return refuse(msg, TRX_E_ARG, "exposures: no observed set installed (trx_set_observed)");
  if (ex->nexp < 0) return refuse(msg, TRX_E_ARG, "exposures: nexp < 0");
  if (ex->nexp != S.nexp) return refuse(msg, TRX_E_ARG, "exposures: nexp " + std::to_string(ex->nexp) + " is not the observed set's nexp " + std::to_string(S.nexp));
  if (!ex->scale && !ex->smear) return refuse(msg, TRX_E_ARG, "exposures: NULL scale and smear arrays");
  for (int32_t v = 0; v < ex->nexp; v++) {
    if (ex->scale && !std::isfinite(ex->scale[v])) return refuse(msg, TRX_E_ARG, "exposures: exposure " + std::to_string(v) + ": scale must be finite");
    if (ex->smear && (!std::isfinite(ex->smear[v]) || !(ex->smear[v] >= 0) || !(ex->smear[v] <= TRX_SMEAR_MAX)))
      return refuse(msg, TRX_E_ARG, "exposures: exposure " + std::to_string(v) + ": smear must be finite, >= 0 and at most TRX_SMEAR_MAX (" + std::to_string(TRX_SMEAR_MAX) + ")");
  }
  return TRX_OK;
}

// the table's device arrays, [nexp] each (an array the caller left out is not uploaded)
struct ExposureExtents { size_t scale_bytes, smear_bytes; };
inline ExposureExtents exposure_extents(int32_t nexp)
{
  const size_t bytes = sizeof(double) * (size_t)nexp;
  return ExposureExtents{bytes, bytes};
}

// What trx_run_exposed refuses, in this order: no observed set, no table, the count -- one shift per exposure --, the NULL
// arrays.  (A shard of the grid is served: the pairs are linear in the bins.)
inline int exposed_run_checks(const ProductState &S, const char *who, int32_t nshift, const void *shift, const void *out, std::string &msg)
{
  auto no = [&](const std::string &what) { return refuse(msg, TRX_E_ARG, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no("no observed set installed (trx_set_observed)");
  if (!S.exposures) return no("no exposure table installed (trx_set_exposures)");
  if (nshift != S.nexp) return no("nshift " + std::to_string(nshift) + " is not the observed set's nexp " + std::to_string(S.nexp));
  if (!shift) return no("shift is NULL");
  if (!out) return no("out is NULL");
  return TRX_OK;
}

}  // namespace trx
