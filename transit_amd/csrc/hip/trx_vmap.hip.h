// trx_vmap.hip.h -- the Kp-Vsys detection map on the device, reduced from the trail k_trail_moments (trx_trail.hip.h) has
// just left in device memory (trx_run_velocity_map, include/transit_hip.h).  The arithmetic is trx_vmap.h's; what is
// fixed here is the ORDER of the two sums, which is what fixes the bits: both are taken in index order, one term after
// the other, from +0.
//
//   k_trail_stat     one wavefront per trail row pair (lag l, exposure v), kVmapWaves per block, the last block ragged.
//                    Lane k takes segment s0 + k: its seven moments are 56 contiguous bytes, the wave's 64 x 56 bytes are
//                    one contiguous piece of the trail, read once.  Every lane forms its segment's statistic
//                    (vmap_stat); then the wave adds the statistics of the trip in segment order -- each read from its
//                    lane (v_readlane), NaN skipped -- to a sum every lane carries alike.  per[l][v] goes out twice:
//                    lag-major for the host, exposure-major for k_velocity_map.
//   k_velocity_map   one wavefront per map cell (i, j), kVmapWaves per block.  Lane k takes exposure v0 + k: its velocity
//                    (vmap_track), its place on the lag grid (vmap_locate: a bisection over lag_kms, which every lane
//                    of every wave reads -- it stays in the vector L1) and its term (vmap_term) from the two entries of
//                    the exposure-major per, which are neighbours in memory; then the in-order sum over the trip's
//                    exposures as above, nothing skipped.  A cell with an exposure outside the grid is NaN.
//
// No atomics, no LDS.  per[l][v] depends on the trail rows (l, v, .) only; a cell on its kp, its vsys, orbit, offset,
// lag_kms and per -- not on the other cells of the call or on the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"
#include "../trx_vmap.h"

namespace trx {

constexpr int kVmapWaves = 4;                         // rows of k_trail_stat / cells of k_velocity_map (waves) per block

struct TrailStatArgs {
  const double *trail;      // [nlag][nexp][nseg][TRX_NMOMENT] (device): d_trail of this run
  double *per_lv;           // [nlag][nexp]
  double *per_vl;           // [nexp][nlag]
  int64_t nrows;            // nlag * nexp
  int32_t nlag, nexp, nseg, stat;
  double p0, p1;
};

struct VelMapArgs {
  const double *per_vl;     // [nexp][nlag]
  const double *lag_kms;    // [nlag]
  const double *kp, *vsys;  // [nkp], [nvsys]
  const double *orbit;      // [nexp]
  const double *offset;     // [nexp], or null: none
  double *map;              // [nkp][nvsys]
  int64_t ncells;           // nkp * nvsys
  int32_t nlag, nexp, nvsys;
};

// acc plus the first `count` lanes' values of v in lane order, one addition each; SKIP: a NaN adds nothing.  Every lane
// of the wave must be here, and `count` the same in all of them; all return the same sum.
template <bool SKIP>
__device__ __forceinline__ double wave_add_in_order(double acc, double v, int count)
{
#pragma clang fp contract(off)
  for (int j = 0; j < count; j++) {
    const double t = readlane_f64(v, j);
    acc = SKIP ? vmap_add_stat(acc, t) : acc + t;
  }
  return acc;
}

__global__ __launch_bounds__(64 * kVmapWaves) void k_trail_stat(TrailStatArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t row = (int64_t)blockIdx.x * kVmapWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (row >= A.nrows) return;                          // (a whole wave: the in-order sums below have all their lanes)
  const double *m0 = A.trail + row * A.nseg * TRX_NMOMENT;
  double acc = 0.0;
  for (int32_t s0 = 0; s0 < A.nseg; s0 += 64) {
    const int32_t s = s0 + lane;
    double st = vmap_nan();
    if (s < A.nseg) {
      double m[TRX_NMOMENT];
#pragma unroll
      for (int c = 0; c < TRX_NMOMENT; c++) m[c] = m0[(int64_t)s * TRX_NMOMENT + c];
      st = vmap_stat(m, A.stat, A.p0, A.p1);
    }
    acc = wave_add_in_order<true>(acc, st, A.nseg - s0 < 64 ? A.nseg - s0 : 64);
  }
  if (lane == 0) {
    const int64_t l = row / A.nexp, v = row % A.nexp;
    A.per_lv[row] = acc;
    A.per_vl[v * A.nlag + l] = acc;
  }
}

__global__ __launch_bounds__(64 * kVmapWaves) void k_velocity_map(VelMapArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t cell = (int64_t)blockIdx.x * kVmapWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (cell >= A.ncells) return;                        // (a whole wave)
  const double kp = A.kp[cell / A.nvsys], vsys = A.vsys[cell % A.nvsys];
  double acc = 0.0;
  bool outside = false;
  for (int32_t v0 = 0; v0 < A.nexp; v0 += 64) {
    const int32_t v = v0 + lane;
    double term = 0.0;
    if (v < A.nexp) {
      int32_t k; double t;
      if (!vmap_locate(A.lag_kms, A.nlag, vmap_track(kp, vsys, A.orbit[v], A.offset, v), k, t)) outside = true;
      const double *p = A.per_vl + (int64_t)v * A.nlag;
      term = A.nlag < 2 ? p[0] : vmap_term(p[k], p[k + 1], t);
    }
    acc = wave_add_in_order<false>(acc, term, A.nexp - v0 < 64 ? A.nexp - v0 : 64);
  }
  const bool any_outside = __ballot(outside) != 0;
  if (lane == 0) A.map[cell] = any_outside ? vmap_nan() : acc;
}

}  // namespace trx
