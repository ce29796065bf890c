// trx_vmap.h -- the arithmetic of the Kp-Vsys detection map (trx_run_velocity_map, include/transit_hip.h): the statistic
// of one trail row, the place of a velocity on the lag grid and one exposure's interpolated term.  Plain host/device
// functions: k_trail_stat and k_velocity_map (hip/trx_vmap.hip.h) and k_cell_tracks and k_cell_stat (hip/trx_cellmap.hip.h,
// trx_run_filtered_map) call them per lane, tests/vmap_check.cpp and tests/cellmap_check.cpp run the same source on the
// CPU.  Every operation is an IEEE double operation rounded once -- no fused multiply-add -- in the order
// transit_amd/xcor.py (central, ccf, loglike_bl19, chi2, map_from_per) writes it, so that +, -, *, / and sqrt give numpy's
// bits on either side; only log is the platform's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "trx_numerics.h"

namespace trx {

// trx_vmap.stat (the values of TRX_STAT_* in transit_hip.h)
constexpr int kStatCcf = 1, kStatLoglikeBl19 = 2, kStatChi2 = 3;

TRX_HD double vmap_nan() { return __builtin_nan(""); }

// stat(m) of the seven moments m = (n, sum w, sum w g, sum w g^2, sum w f, sum w f g, sum w f^2) of a trail row; NaN where
// the statistic is undefined: n < 2, a variance that is not positive, a non-positive argument of the logarithm.
//   CCF           R / sqrt(s_f^2 s_g^2)
//   LOGLIKE_BL19  (-0.5 n) log(s_f^2 - (2 p0) R + (p0 p0) s_g^2)
//   CHI2          m6 - (2 p0) m5 - (2 p1) m4 + (p0 p0) m3 + ((2 p0) p1) m2 + (p1 p1) m1
// with <f> = m4 / m1, <g> = m2 / m1, s_f^2 = m6 / m1 - <f><f>, s_g^2 = m3 / m1 - <g><g>, R = m5 / m1 - <f><g>.
TRX_HD double vmap_stat(const double *m, int stat, double p0, double p1)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (stat == kStatChi2) {
    const double a2 = 2.0 * p0, b2 = 2.0 * p1;
    return m[6] - a2 * m[5] - b2 * m[4] + (p0 * p0) * m[3] + (a2 * p1) * m[2] + (p1 * p1) * m[1];
  }
  const double n = m[0], sw = m[1];
  const double mf = m[4] / sw, mg = m[2] / sw;
  const double sf2 = m[6] / sw - mf * mf;
  const double sg2 = m[3] / sw - mg * mg;
  const double r = m[5] / sw - mf * mg;
  if (!(n >= 2.0 && sf2 > 0.0 && sg2 > 0.0)) return vmap_nan();
  if (stat == kStatCcf) return r / sqrt(sf2 * sg2);
  const double arg = sf2 - (2.0 * p0) * r + (p0 * p0) * sg2;
  if (!(arg > 0.0)) return vmap_nan();
  return (-0.5 * n) * log(arg);
}

// one step of the sum over segments: undefined rows are skipped
TRX_HD double vmap_add_stat(double acc, double st) { return st != st ? acc : acc + st; }

// The velocity of cell (kp, vsys) at an exposure: (kp * orbit + vsys) + offset, the last addition only with an offset.
TRX_HD double vmap_track(double kp, double vsys, double orbit, const double *offset, int64_t v)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = kp * orbit + vsys;
  return offset ? x + offset[v] : x;
}

// Where x lies on the strictly increasing grid kms[0 .. nlag-1], nlag >= 2: k = clip(upper_bound(kms, x) - 1, 0, nlag - 2)
// and t = (x - kms[k]) / (kms[k+1] - kms[k]); x == kms[nlag-1] gives k = nlag - 2, t = 1.  False -- k = 0, t = 0 -- for an
// x outside [kms[0], kms[nlag-1]] or not finite (with nlag == 1: k = 0, t = 0 and the same test).
TRX_HD bool vmap_locate(const double *kms, int32_t nlag, double x, int32_t &k, double &t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  k = 0; t = 0.0;
  if (!(x >= kms[0] && x <= kms[nlag - 1])) return false;
  if (nlag < 2) return true;
  int32_t lo = 0, hi = nlag;                        // the first index in [lo, hi) whose velocity is above x
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (kms[mid] <= x) lo = mid + 1; else hi = mid;
  }
  k = lo - 1;
  if (k < 0) k = 0;
  if (k > nlag - 2) k = nlag - 2;
  t = (x - kms[k]) / (kms[k + 1] - kms[k]);
  return true;
}

// The lag NEAREST to x on that grid (trx_run_filtered_map): vmap_locate's k, or k + 1 when t > 0.5 -- a tie goes to the
// lower lag; nlag == 1: 0.  -1 for an x vmap_locate refuses.  In [0, nlag - 1] otherwise.
TRX_HD int32_t vmap_nearest(const double *kms, int32_t nlag, double x)
{
  int32_t k; double t;
  if (!vmap_locate(kms, nlag, x, k, t)) return -1;
  return k + (t > 0.5 ? 1 : 0);
}

// one exposure's term of a cell from the statistic at the two lags around its velocity
TRX_HD double vmap_term(double pk, double pk1, double t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return pk + t * (pk1 - pk);
}

}  // namespace trx
