// trx_broaden.h -- the per-bin arithmetic of the rotational broadening (trx_set_broadening, include/transit_hip.h):
// the half-width of a bin's window, the weights of Gray's rotation profile and the paired sum over an indexable
// source.  Plain host/device functions: k_broaden (hip/trx_broaden.hip.h) runs them over a tile of the spectrum in
// LDS, trx_set_broadening sizes that tile with them, and tests/broaden_check.cpp runs the same source on the CPU
// over exact-size buffers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "trx_numerics.h"

namespace trx {

constexpr int kBroadBlock = 256;      // output bins (lanes) per block of k_broaden

// c1 = 2 (1 - limb), c2 = (pi / 2) limb: the two terms of the profile, w(x) = c1 sqrt(1 - x^2) + c2 (1 - x^2)
struct BroadWeights { double c1, c2; };
TRX_HD BroadWeights broaden_weights(double limb)
{
  BroadWeights W;
  W.c1 = 2.0 * (1.0 - limb);
  W.c2 = (3.14159265358979323846 / 2.0) * limb;
  return W;
}

// Bin i's half-width: d = nu_i * beta in cm-1 (returned through d) and floor(d / wn_d) in bins, as a double (the
// callers compare it with their cap before they convert it).  Every operation IEEE double rounded once -- no fused
// multiply-add -- so that host and device get the same integers; non-decreasing in i for wn_d > 0, beta > 0 (every
// step is a monotone function rounded monotonely).
TRX_HD double broaden_half(double wn_i, double wn_d, double beta, int64_t i, double &d)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double nu = wn_i + (double)i * wn_d;
  d = nu * beta;
  return floor(d / wn_d);
}

// What a block of k_broaden stages for the output bins [i0, i1] (i1 the block's last bin, H its half-width -- the
// block's largest): the bins [t0, t1] of the grid, both inclusive, at most i1 - i0 + 1 + 2 H of them.
TRX_HD void broaden_tile(int64_t i0, int64_t i1, int64_t H, int64_t nwn, int64_t &t0, int64_t &t1)
{
  t0 = i0 - H > 0 ? i0 - H : 0;
  t1 = i1 + H < nwn - 1 ? i1 + H : nwn - 1;
}

// B_i of the header from a source with S[j - base] = S_j for the bins j of [i - h, i + h] inside the grid [0, nwn):
// the centre first, then the pairs k = 1 .. h ascending, each pair's two bins added before the weight multiplies them;
// bins outside the grid enter as +0 and leave the weight out of the denominator.  h = 0: a copy.
template <class Src>
TRX_HD double broaden_bin(const Src &S, int64_t base, int64_t nwn, int64_t i, int h, double d, double wn_d, BroadWeights W)
{
  const int64_t c = i - base;
  if (h == 0) return S[c];
  const double w0 = W.c1 + W.c2;
  double num = w0 * S[c], den = w0;
  for (int k = 1; k <= h; k++) {
    const double x = ((double)k * wn_d) / d;
    double t = 1.0 - x * x;
    t = t > 0.0 ? t : 0.0;
    const double w = W.c1 * sqrt(t) + W.c2 * t;
    const bool below = i - k >= 0, above = i + k < nwn;
    const double s = (below ? S[c - k] : 0.0) + (above ? S[c + k] : 0.0);
    const double m = (double)((int)below + (int)above);
    num += w * s; den += w * m;
  }
  return num / den;
}

}  // namespace trx
