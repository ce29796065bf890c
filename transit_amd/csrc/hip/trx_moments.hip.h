// trx_moments.hip.h -- cross-correlation moments of the detector pixels against observed data on the device
// (trx_set_observed / trx_run_moments, include/transit_hip.h).
//
// k_pixel_pairs (trx_pixels.hip.h) leaves out[v][p] = (a, b) in device memory: the model at exposure v's shift, at
// pixel p.  What a driver does with that matrix is always the same: per exposure and spectral order (a SEGMENT of
// consecutive pixels) it forms a correlation coefficient, a log-likelihood or a chi-square against the observed
// values f with weights w -- all functions of seven sums over the segment's contributing pixels (b > 0 and w > 0),
// with g = gain_p * (a / b):
//   n, sum w, sum w g, sum w g^2, sum w f, sum w f g, sum w f^2
// The observed set (segments, data, weights, gain) is on the device from trx_set_observed; only the
// [nexp][nseg][7] moments go back to the host.
//
//   k_pixel_moments  one wavefront per ROW (v, s), row = v * nseg + s: the segments of one exposure on consecutive
//                    waves, kMomWaves waves per block, the last block ragged.  Lane l adds the segment's pixels
//                    first + l, first + l + 64, ... in that order into seven accumulators; the 64 lane sums of each
//                    go through wave_sum's fixed butterfly once, at the end.  The terms are w, w*g, (w*g)*g, w*f,
//                    (w*f)*g, (w*f)*f, every operation rounded once (no contraction).
//                    A segment is ONE wave's work whatever its length: nexp * nseg, not the segment length, is the
//                    parallel axis (a spectrograph's 100 exposures x 40 orders are 4000 waves).  It is a streaming
//                    reduction of 40 bytes per pixel (the pair, f, w; the gain comes from cache), all loads
//                    coalesced; a wave issues the loads of kMomTrips trips of 64 pixels before it adds the first
//                    (a lane past the segment's end reads the segment's last pixel again and adds nothing).
//
//   k_pixel_moments<true>   the same sums over the FILTERED values of the run (trx_filter.hip.h, trx_run_filtered_moments):
//                    the model value is val[v][p] as it stands, a pixel contributes when that is not NaN and w > 0;
//                    24 bytes per pixel.  <false> is the form above.
//
// No atomics: the bits of a row depend on the pairs, data and weights of that exposure over that segment's pixels and
// on their gains -- not on the other segments or exposures of the call, the launch, the handle that ran it or the
// run's step plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"

namespace trx {

constexpr int kMomWaves = 4;                          // rows (waves) per block
constexpr int kMomTrips = 4;                          // trips of 64 pixels whose loads a wave has in flight at once

struct MomArgs {
  const double2 *pairs;     // [nexp][npix] (a, b): d_pixout of this run
  const double *val;        // [nexp][npix] k_pixel_moments<true>: the filtered values of this run (trx_filter.hip.h), NaN = none
  const double *data;       // [nexp][npix]
  const double *weight;     // [nexp][npix], or null: all 1
  const double *gain;       // [npix], or null: all 1
  const int64_t *seg_first; // [nseg + 1]
  double *mom;              // [nexp][nseg][TRX_NMOMENT] (device)
  int64_t npix, nrows;      // nrows = nexp * nseg
  int32_t nseg;
};

// kValues: the model value of a pixel is val[v][p] as it stands (gain and division are in it already), and the pixel
// contributes when that is not NaN and w > 0; the terms, their order and the butterfly are the same
template <bool kValues>
__global__ __launch_bounds__(64 * kMomWaves) void k_pixel_moments(MomArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t row = (int64_t)blockIdx.x * kMomWaves + (threadIdx.x >> 6);
  if (row >= A.nrows) return;                          // (a whole wave: the butterfly below has all its lanes)
  const int64_t v = row / A.nseg, s = row - v * A.nseg;
  const int64_t first = A.seg_first[s], last = A.seg_first[s + 1];
  const int64_t base = v * A.npix;
  double n = 0.0, sw = 0.0, swg = 0.0, swgg = 0.0, swf = 0.0, swfg = 0.0, swff = 0.0;
  // kMomTrips trips at a time: their loads first (a lane past the segment's end reads the segment's last pixel again), then their
  // terms in trip order -- the order of a lane's sum is that of its pixels
  for (int64_t p0 = first; p0 < last; p0 += 64 * kMomTrips) {
    double2 ab[kMomTrips]; double f[kMomTrips], w[kMomTrips], g0[kMomTrips]; bool in[kMomTrips];
#pragma unroll
    for (int t = 0; t < kMomTrips; t++) {
      const int64_t q = p0 + 64 * t + lane;
      in[t] = q < last;
      const int64_t p = in[t] ? q : last - 1;
      if constexpr (kValues) { ab[t].x = A.val[base + p]; ab[t].y = 1.0; g0[t] = 1.0; }
      else { ab[t] = A.pairs[base + p]; g0[t] = A.gain ? A.gain[p] : 1.0; }
      f[t] = A.data[base + p];
      w[t] = A.weight ? A.weight[base + p] : 1.0;
    }
#pragma unroll
    for (int t = 0; t < kMomTrips; t++)
      if (in[t] && (kValues ? ab[t].x == ab[t].x : ab[t].y > 0.0) && w[t] > 0.0) {
        const double g = kValues ? ab[t].x : g0[t] * (ab[t].x / ab[t].y);
        const double wg = w[t] * g, wf = w[t] * f[t];
        n += 1.0; sw += w[t]; swg += wg; swgg += wg * g; swf += wf; swfg += wf * g; swff += wf * f[t];
      }
  }
  n = wave_sum(n); sw = wave_sum(sw); swg = wave_sum(swg); swgg = wave_sum(swgg);
  swf = wave_sum(swf); swfg = wave_sum(swfg); swff = wave_sum(swff);
  // (every lane holds the seven sums: lanes 0 .. 6 store one each)
  const double r = lane == 0 ? n : lane == 1 ? sw : lane == 2 ? swg : lane == 3 ? swgg : lane == 4 ? swf : lane == 5 ? swfg : swff;
  if (lane < TRX_NMOMENT) A.mom[row * TRX_NMOMENT + lane] = r;
}

}  // namespace trx
