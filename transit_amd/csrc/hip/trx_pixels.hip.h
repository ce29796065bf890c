// trx_pixels.hip.h -- Doppler-shifted detector sampling of the spectrum on the device (trx_run_pixels,
// include/transit_hip.h).
//
// A high-resolution retrieval shifts the model spectrum to the planet's velocity at every exposure, convolves it
// with the spectrograph's line-spread function and samples it at the detector's pixel centres.  The pixel set
// (centre, fwhm per pixel, in the OBSERVED frame) is on the device from trx_set_pixels; a run brings its nshift
// shifts (nu_observed / nu_rest) and gets out[v][p] = (sum of w_i S_i, sum of w_i): the pair of the band
// TRX_BAND_GAUSS{centre_p / shift_v, fwhm_p / shift_v, cut}.  Nothing per (pixel, shift) pair is made on the host.
//
//   k_pixel_pairs  one lane per PAIR, pixels of one shift on consecutive lanes (neighbouring windows overlap in
//                  cache).  Every lane makes its pair's range (pixel_range: the band rule, each operation rounded
//                  once) and
//                    - a window of fewer than kPixWaveFrom in-shard bins is added by its lane, bins ascending;
//                    - a longer one is added by the whole wave once the lanes are done with the short ones: lane l
//                      adds the window's in-shard bins l, l + 64, ... in that order, then wave_sum's fixed butterfly.
//                  Which form a pair takes depends on its own in-shard window length alone.
//
// No atomics: the bits of a pair depend on the spectrum, its pixel, its shift and the shard only -- not on the other
// pixels or shifts of the call, the launch, the handle that ran it or the run's step plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"
#include "trx_bands.hip.h"

namespace trx {

// (kPixBlock, the lanes (pairs) per block: trx_device.h)
constexpr int kPixWaveFrom = 192;                     // in-shard window length from which the wave adds a pair

struct PixArgs {
  const double *spec;       // [nsh] the run's spectrum (device)
  const double *centre;     // [npix] observed frame, cm-1
  const double *fwhm;       // [npix]
  const double *shift;      // [nshift]
  double *out;              // [nshift][npix][2] (device)
  int64_t npix, npairs;     // npairs = nshift * npix
  int64_t nwn, lo, hi;      // the whole grid's bins; this shard's [lo, hi)
  double cut, fwhm_sigma;   // fwhm_sigma: 2 sqrt(2 ln 2), the host's double (the one trx_set_bands divides by)
  double wn_i, wn_d;
};

// The rest-frame Gaussian of pixel (centre, fwhm) at `shift`, and its bins [first, last) of the whole grid by the rule of
// TRX_BAND_GAUSS (make_band_set does the same on the host): IEEE double, every operation rounded once.
__device__ __forceinline__ void pixel_range(const PixArgs &A, double centre_obs, double fwhm_obs, double shift,
                                            double &centre, double &sigma, int64_t &first, int64_t &last)
{
#pragma clang fp contract(off)
  centre = centre_obs / shift;
  const double fwhm = fwhm_obs / shift;
  sigma = fwhm / A.fwhm_sigma;
  const double a = ceil((centre - A.cut * sigma - A.wn_i) / A.wn_d);
  const double z = floor((centre + A.cut * sigma - A.wn_i) / A.wn_d) + 1.0;
  const double n = (double)A.nwn;
  // (clipped to [0, nwn] in double: no conversion of a value out of int64's range; a shift so small that the centre
  // overflows gives no bin)
  if (!(a == a) || !(z == z)) { first = last = 0; return; }
  first = a <= 0 ? 0 : a >= n ? A.nwn : (int64_t)a;
  last = z <= 0 ? 0 : z >= n ? A.nwn : (int64_t)z;
  if (last < first) last = first;
}

__device__ __forceinline__ int64_t readlane_i64(int64_t v, int l)
{
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffLL), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l);
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

__global__ __launch_bounds__(kPixBlock) void k_pixel_pairs(PixArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t q = (int64_t)blockIdx.x * kPixBlock + threadIdx.x;      // pair q = v * npix + p
  const bool mine = q < A.npairs;
  // (no early return: the long windows below are added by whole waves)
  double centre = 0.0, sigma = 1.0;
  int64_t s = 0, e = 0;                                 // the pair's bins in the shard, local to it: [s, e) within [0, hi - lo)
  if (mine) {
    const int64_t v = q / A.npix, p = q - v * A.npix;
    int64_t first, last;
    pixel_range(A, A.centre[p], A.fwhm[p], A.shift[v], centre, sigma, first, last);
    first = first > A.lo ? first : A.lo;
    last = last < A.hi ? last : A.hi;
    if (last > first) { s = first - A.lo; e = last - A.lo; }
  }
  const bool wide = e - s >= kPixWaveFrom;
  double sum = 0.0, sw = 0.0;
  if (!wide)
    for (int64_t j = s; j < e; j++) {
      const double w = gauss_weight(A.wn_i, A.wn_d, A.lo + j, centre, sigma);
      sum += w * A.spec[j]; sw += w;
    }
  // the wave's long windows, one after the other in lane order (wave-uniform loop: every lane is here)
  for (unsigned long long m = __ballot(wide); m; m &= m - 1) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll(m) - 1);
    const int64_t ws = readlane_i64(s, src), we = readlane_i64(e, src);
    const double wc = readlane_f64(centre, src), wsig = readlane_f64(sigma, src);
    double t = 0.0, tw = 0.0;
    for (int64_t j = ws + lane; j < we; j += 64) {
      const double w = gauss_weight(A.wn_i, A.wn_d, A.lo + j, wc, wsig);
      t += w * A.spec[j]; tw += w;
    }
    t = wave_sum(t); tw = wave_sum(tw);
    if (lane == src) { sum = t; sw = tw; }
  }
  if (mine) { A.out[2 * q] = sum; A.out[2 * q + 1] = sw; }
}

}  // namespace trx
