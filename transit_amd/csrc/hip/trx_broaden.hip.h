// trx_broaden.hip.h -- rotational broadening of the spectrum on the device, between the spectrum and the detector
// pixels (trx_set_broadening / trx_run_broadened, include/transit_hip.h).
//
// A retrieval that fits the planet's v sin i convolves the model spectrum with the rotation profile before the
// instrument sees it; the width changes with every likelihood call and the profile is no Gaussian, so it cannot ride
// on the pixel set's fwhm.  The arithmetic of one output bin is in ../trx_broaden.h (shared with the host and with
// tests/broaden_check.cpp); this file holds the launch shape.
//
//   k_broaden  one block of kBroadBlock lanes for kBroadBlock consecutive output bins.  The block stages the bins
//              [i0 - H, i1 + H] of the spectrum, clipped to the grid, in LDS -- H the half-width of its LAST bin, which
//              is its largest (broaden_half is non-decreasing) -- and every lane then walks its own window over the
//              tile, pairs k = 1 .. h_i ascending: consecutive lanes read consecutive doubles.  A window is never
//              split over lanes: the order of a bin's sum is the definition's.
//
// LDS is sized per launch from the run's h_{nwn-1} (Broadening::hmax on the host): (kBroadBlock + 2 hmax) doubles,
// 34.8 KB at TRX_BROADEN_MAX_HALF.  No atomics: the bits of B_i depend on S over [i - h_i, i + h_i], beta and limb only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "../trx_broaden.h"

namespace trx {

struct BroadArgs {
  const double *spec;       // [nwn] the run's spectrum (device)
  double *out;              // [nwn] the broadened spectrum (device)
  int64_t nwn;
  double wn_i, wn_d, beta;
  BroadWeights W;
  int hmax;                 // h_{nwn-1}: the launch's LDS holds kBroadBlock + 2 * hmax doubles
};

__global__ __launch_bounds__(kBroadBlock) void k_broaden(BroadArgs A)
{
  extern __shared__ __attribute__((aligned(16))) char broad_lds[];
  double *tile = (double *)broad_lds;
  const int64_t i0 = (int64_t)blockIdx.x * kBroadBlock;
  const int64_t i1 = i0 + kBroadBlock - 1 < A.nwn - 1 ? i0 + kBroadBlock - 1 : A.nwn - 1;
  // (the half-widths are held to the launch's: the tile is what the host sized, whatever the arithmetic says)
  double d;
  const double hl = broaden_half(A.wn_i, A.wn_d, A.beta, i1, d);
  const int H = hl < (double)A.hmax ? (hl > 0.0 ? (int)hl : 0) : A.hmax;
  int64_t t0, t1;
  broaden_tile(i0, i1, H, A.nwn, t0, t1);
  for (int64_t j = t0 + threadIdx.x; j <= t1; j += kBroadBlock) tile[j - t0] = A.spec[j];
  __syncthreads();
  const int64_t i = i0 + threadIdx.x;
  if (i > i1) return;
  const double hf = broaden_half(A.wn_i, A.wn_d, A.beta, i, d);
  const int h = hf < (double)H ? (hf > 0.0 ? (int)hf : 0) : H;
  A.out[i] = broaden_bin(tile, t0, A.nwn, i, h, d, A.wn_d, A.W);
}

}  // namespace trx
