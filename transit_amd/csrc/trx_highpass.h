// trx_highpass.h -- the arithmetic of the high-pass along the pixel axis (trx_set_highpass / trx_run_highpassed,
// include/transit_hip.h): one staged entry of a row, the values of the pixels a lane owns, the full-window denominator.
// Plain host/device functions: k_pixel_highpass and k_data_highpass (hip/trx_highpass.hip.h; the second high-passes the
// observed set's own data, trx_highpass_observed) call them per lane over their tile in LDS, tests/highpass_check.cpp and
// tests/hpdata_check.cpp run the same source on the CPU over exact-size arrays.  Every operation is an IEEE double
// operation rounded once -- no fused multiply-add -- in the order transit_amd/xcor.py (highpass_reference) writes it.
//
// The definition skips the terms whose pixel is outside the segment or not live.  Here such a pixel is STAGED as
// (g, m) = (+0, +0), a live one as (g, 1), and every term is added: with taps finite and >= 0, t * (+0) is +0, and a sum
// that started from +0 is never -0, so acc + (+0) is acc in every bit; t * 1 is t.  The sums are the definition's.
#pragma once
#include <stdint.h>

#include "trx_numerics.h"

namespace trx {

// the staged entry of one pixel of a row: (a, b) its pair, gain its gain (1 without a gain array), inside: the pixel lies
// in the segment of the tile that stages it
TRX_HD void highpass_stage(double a, double b, double gain, bool inside, double &g, double &m)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool live = inside && b > 0.0;
  g = live ? gain * (a / b) : 0.0;
  m = live ? 1.0 : 0.0;
}

// the staged entry of one datum of the observed set (trx_highpass_observed): r its value -- a residual, or the raw datum --,
// w its weight as trx_set_observed installed it (1 without weights), inside: the pixel lies in the segment of the tile that
// stages it.  The value goes in as it is: no pair, no quotient, no gain
TRX_HD void highpass_stage_datum(double r, double w, bool inside, double &g, double &m)
{
  const bool live = inside && w > 0.0;
  g = live ? r : 0.0;
  m = live ? 1.0 : 0.0;
}

// den of a pixel whose whole window is live and inside its segment: the taps added over k = -half .. half in that
// order from +0 -- the double the accumulated den is there (t * 1 is t)
inline double highpass_full_den(int half, const double *taps)
{
  double den = 0.0;
  for (int k = half; k >= 1; k--) den += taps[k];
  for (int k = 0; k <= half; k++) den += taps[k];
  return den;
}

// g' of the R pixels staged at g[at[j]], m[at[j]] (entries at[j] - half .. at[j] + half are staged).  Each output's sums run
// over k = -half .. half in that order; the R outputs share the tap.  full: every entry of every window is live (m = 1) --
// then den is den_full, highpass_full_den of these taps.  An output whose own pixel is dead is meaningless (0 / 0): the
// caller writes the dead value there.
template <int R>
TRX_HD void highpass_values(const double *g, const double *m, const int (&at)[R], int half, const double *taps, bool full, double den_full,
                            double (&out)[R])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double num[R], den[R];
  for (int j = 0; j < R; j++) { num[j] = 0.0; den[j] = 0.0; }
  if (full) {
    for (int k = half; k >= 1; k--) {
      const double t = taps[k];
      for (int j = 0; j < R; j++) num[j] += t * g[at[j] - k];
    }
    for (int k = 0; k <= half; k++) {
      const double t = taps[k];
      for (int j = 0; j < R; j++) num[j] += t * g[at[j] + k];
    }
    for (int j = 0; j < R; j++) den[j] = den_full;
  } else {
    for (int k = half; k >= 1; k--) {
      const double t = taps[k];
      for (int j = 0; j < R; j++) { num[j] += t * g[at[j] - k]; den[j] += t * m[at[j] - k]; }
    }
    for (int k = 0; k <= half; k++) {
      const double t = taps[k];
      for (int j = 0; j < R; j++) { num[j] += t * g[at[j] + k]; den[j] += t * m[at[j] + k]; }
    }
  }
  for (int j = 0; j < R; j++) out[j] = g[at[j]] - num[j] / den[j];
}

}  // namespace trx
