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
//   k_pixel_pairs_exposed
//                  the same layout and the same two forms for the runs whose rows are exposures, on a handle with an
//                  exposure table (trx_set_exposures): row v = q / npix has a smear half-width eta_v and a scale c_v.  A
//                  row with eta == 0 takes the Gaussian weight above over the same range; one with eta > 0 the box of
//                  half-width d = centre * eta convolved with the Gaussian, W = erf((x + d) / q) - erf((x - d) / q), over
//                  the range widened by d (exposed_range, ../trx_exposures.h: the host's source).  The choice is per lane
//                  in the short form and per broadcast source lane in the wave form; a is then multiplied by c_v.
//
// No atomics: the bits of a pair depend on the spectrum, its pixel, its shift (its row's eta and c) and the shard only --
// not on the other pixels or shifts of the call, the launch, the handle that ran it or the run's step plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"
#include "trx_bands.hip.h"
#include "../trx_exposures.h"

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
  // k_pixel_pairs_exposed alone (the plain kernel reads none of them)
  const double *scale;      // [nshift] the rows' factors on a, or null: none
  const double *smear;      // [nshift] the rows' eta, or null: 0
  double sqrt2;             // sqrt(2), the host's double
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

// the weight of global bin g under the box of half-width d (> 0) convolved with the Gaussian of q = sigma sqrt(2), unnormalised:
// what trx_set_exposures defines
__device__ __forceinline__ double smear_weight(double wn_i, double wn_d, int64_t g, double centre, double d, double q)
{
#pragma clang fp contract(off)
  const double nu = wn_i + (double)g * wn_d;
  const double x = nu - centre;
  return erf((x + d) / q) - erf((x - d) / q);
}

__global__ __launch_bounds__(kPixBlock) void k_pixel_pairs_exposed(PixArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t q = (int64_t)blockIdx.x * kPixBlock + threadIdx.x;      // pair q = v * npix + p (a block straddles rows)
  const bool mine = q < A.npairs;
  // (no early return: the long windows below are added by whole waves)
  double centre = 0.0, sigma = 1.0, d = 0.0, c = 1.0;
  int64_t s = 0, e = 0;                                 // the pair's bins in the shard, local to it: [s, e) within [0, hi - lo)
  if (mine) {
    const int64_t v = q / A.npix, p = q - v * A.npix;
    const double eta = A.smear ? A.smear[v] : 0.0;
    if (A.scale) c = A.scale[v];
    int64_t first, last;
    exposed_range(A.wn_i, A.wn_d, A.nwn, A.cut, A.fwhm_sigma, A.centre[p], A.fwhm[p], A.shift[v], eta, centre, sigma, d, first, last);
    first = first > A.lo ? first : A.lo;
    last = last < A.hi ? last : A.hi;
    if (last > first) { s = first - A.lo; e = last - A.lo; }
  }
  const double wq = sigma * A.sqrt2;                    // (read by the rows with d > 0 alone)
  const bool wide = e - s >= kPixWaveFrom;
  double sum = 0.0, sw = 0.0;
  if (!wide) {
    if (d > 0.0)
      for (int64_t j = s; j < e; j++) {
        const double w = smear_weight(A.wn_i, A.wn_d, A.lo + j, centre, d, wq);
        sum += w * A.spec[j]; sw += w;
      }
    else
      for (int64_t j = s; j < e; j++) {
        const double w = gauss_weight(A.wn_i, A.wn_d, A.lo + j, centre, sigma);
        sum += w * A.spec[j]; sw += w;
      }
  }
  // the wave's long windows, one after the other in lane order (wave-uniform loop: every lane is here)
  for (unsigned long long m = __ballot(wide); m; m &= m - 1) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll(m) - 1);
    const int64_t ws = readlane_i64(s, src), we = readlane_i64(e, src);
    const double wc = readlane_f64(centre, src), wsig = readlane_f64(sigma, src);
    const double wd = readlane_f64(d, src), wwq = readlane_f64(wq, src);
    double t = 0.0, tw = 0.0;
    if (wd > 0.0)                                       // (wave-uniform: wd is the source lane's)
      for (int64_t j = ws + lane; j < we; j += 64) {
        const double w = smear_weight(A.wn_i, A.wn_d, A.lo + j, wc, wd, wwq);
        t += w * A.spec[j]; tw += w;
      }
    else
      for (int64_t j = ws + lane; j < we; j += 64) {
        const double w = gauss_weight(A.wn_i, A.wn_d, A.lo + j, wc, wsig);
        t += w * A.spec[j]; tw += w;
      }
    t = wave_sum(t); tw = wave_sum(tw);
    if (lane == src) { sum = t; sw = tw; }
  }
  // (a pair with no bin in the shard stays (+0, +0) whatever the factor's sign)
  if (mine) { A.out[2 * q] = (A.scale && e > s) ? c * sum : sum; A.out[2 * q + 1] = sw; }
}

}  // namespace trx
