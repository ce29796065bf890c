// trx_bands.hip.h -- band integrals of the spectrum on the device (trx_run_bands, include/transit_hip.h).
//
// A retrieval compares its data with the spectrum reduced to the instrument's channels: filter curves, top-hat
// bins, a Gaussian line-spread function sampled at pixel centres.  Each band b of a set is a weight per coarse
// bin; a run returns sums[b] = (sum of w_i S_i, sum of w_i) over the band's bins in this handle's shard.
//
//   k_band_pieces  one wave per PIECE: kBandPiece consecutive in-shard bins of one band, counted from the band's
//                  first bin in the shard.  Lane l adds bins l, l + 64, ... of its piece in that order, then the
//                  wave adds its lanes with wave_sum's fixed butterfly.  Bands from one bin to the whole grid, and
//                  overlapping ones, all cost a wave per kBandPiece bins: the work is balanced by pieces.
//   k_band_sums    one wave per band: lane l adds the band's pieces l, l + 64, ... in ascending order, then
//                  wave_sum; lane 0 stores the pair into the pinned block the host reads.
//
// No atomics: every sum has one order, fixed by the band and the shard alone -- not by the launch size, the
// other bands of the set, the handle that ran it or the run's step plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"

namespace trx {

constexpr int kBandWaves = 4;                         // waves per block of both kernels

// (kBandLaneBins, kBandPiece, BandDev, BandPiece: trx_device.h)
struct BandArgs {
  const double *spec;       // [nsh] the run's spectrum (device)
  const BandDev *bands;     // [nbands]
  const BandPiece *pieces;  // [npieces]
  const double *w;          // WEIGHTS bands' in-shard weights, concatenated
  double *part;             // [npieces][2] piece sums (device)
  double *out;              // [nbands][2] pinned host memory, as the device sees it
  int64_t npieces, lo;
  int32_t nbands, pad;
  double wn_i, wn_d;
};

// the weight of global bin g under a Gaussian (centre, sigma): what TRX_BAND_GAUSS defines.  The pixel kernel
// (trx_pixels.hip.h) calls it too: the two paths differ in the order of their sums only.
__device__ __forceinline__ double gauss_weight(double wn_i, double wn_d, int64_t g, double centre, double sigma)
{
  const double nu = wn_i + (double)g * wn_d;
  const double x = (nu - centre) / sigma;
  return exp(-0.5 * (x * x));
}

__global__ __launch_bounds__(64 * kBandWaves) void k_band_pieces(BandArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t p = (int64_t)blockIdx.x * kBandWaves + (threadIdx.x >> 6);
  if (p >= A.npieces) return;                         // (wave-uniform)
  const BandPiece P = A.pieces[p];
  const BandDev B = A.bands[P.band];
  double s = 0.0, sw = 0.0;
  if (B.kind == TRX_BAND_GAUSS) {
#pragma unroll 4
    for (int k = 0; k < kBandLaneBins; k++) {
      const int t = k * 64 + lane;
      if (t < P.len) {
        const int64_t j = P.start + t;
        const double w = gauss_weight(A.wn_i, A.wn_d, A.lo + j, B.centre, B.sigma);
        s += w * A.spec[j]; sw += w;
      }
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < kBandLaneBins; k++) {
      const int t = k * 64 + lane;
      if (t < P.len) {
        const int64_t j = P.start + t;
        const double wj = A.w[B.woff + (j - B.s)];
        s += wj * A.spec[j]; sw += wj;
      }
    }
  }
  s = wave_sum(s); sw = wave_sum(sw);
  if (lane == 0) { A.part[2 * p] = s; A.part[2 * p + 1] = sw; }
}

__global__ __launch_bounds__(64 * kBandWaves) void k_band_sums(BandArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t b = (int64_t)blockIdx.x * kBandWaves + (threadIdx.x >> 6);
  if (b >= A.nbands) return;                          // (wave-uniform)
  const BandDev B = A.bands[b];
  double s = 0.0, sw = 0.0;
  for (int64_t q = lane; q < B.npieces; q += 64) {
    const double *pp = A.part + 2 * (B.piece0 + q);
    s += pp[0]; sw += pp[1];
  }
  s = wave_sum(s); sw = wave_sum(sw);
  if (lane == 0) { A.out[2 * b] = s; A.out[2 * b + 1] = sw; }
}

}  // namespace trx
