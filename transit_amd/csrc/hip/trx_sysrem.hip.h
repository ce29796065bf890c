// trx_sysrem.hip.h -- detrending the observed exposures themselves on the device (trx_detrend_observed,
// include/transit_hip.h): the injection of the model into the raw data and SYSREM (Tamuz, Mazeh & Zucker 2005) per
// segment, one component after another.  The arithmetic is ../trx_sysrem.h's, the same source a CPU program runs.
//
// The residuals r [nexp][npix] start as the raw data (or the injected data) in a buffer of their own.  Per component the
// time vector a [nseg][nexp] starts at 1 and alternates niter times with the column vector c [npix]:
//
//   k_sysrem_inject    element-wise over [nexp][npix]: r = F * (p0 g + p1) where the run's pair has b > 0, F elsewhere.
//   k_sysrem_cols      the column step.  One lane per pixel column, one wavefront per tile of filter_layout's tile table
//                    (<= 64 pixels of one segment), kFiltWaves tiles per block (tile_column).  The lane's column is
//                    sysrem_column_step of ../trx_sysrem.h: v ascends in exposure_trips' trips of kSysTrips
//                    (../trx_columns.h); a_v is wave-uniform (a null a: every a_v = 1, a component's first step).
//   k_sysrem_rows      the row step.  k_pixel_moments' structure: one wavefront per row (v, s), kMomWaves rows per
//                    block; lane l adds the segment's pixels first + l, first + l + 64, ... in that order, kMomTrips
//                    trips in flight (a lane past the end reads the last pixel again and adds nothing), then wave_sum's
//                    butterfly.  nexp * nseg is the parallel axis.
//   k_sysrem_close     one wavefront per tile: the norm t of its segment's a (every tile of a segment computes the same
//                    t from the same a, which the kernel does not change), the scaled c into coef[i][p], and -- the
//                    segment's first tile -- the scaled a into U[s][v][i].
//   k_sysrem_subtract  one wavefront per tile: r[v][p] = r[v][p] - U[s][v][i] * coef[i][p] (sysrem_column_subtract, the same trips).
//
// No LDS, no atomics; cross-lane work goes through wave_sum only.  The bits of a segment's result depend on that segment's
// data and weights, ncomp and niter -- not on other segments, the launch or the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "trx_kernels.hip.h"
#include "trx_filter.hip.h"
#include "trx_moments.hip.h"
#include "../trx_sysrem.h"

namespace trx {

struct SysremInjectArgs {
  const double2 *pairs;     // [nexp][npix] (a, b) of the run
  const double *raw;        // [nexp][npix] F
  const double *gain;       // [npix], or null: all 1
  double *r;                // [nexp][npix]
  int64_t npix, cells;      // cells = nexp * npix
  double p0, p1;
};

struct SysremArgs {
  double *r;                // [nexp][npix] the residuals
  const double *weight;     // [nexp][npix], or null: all 1
  const FilterTile *tiles;  // [ntiles]
  const int64_t *seg_first; // [nseg + 1]
  double *a;                // [nseg][nexp]; k_sysrem_cols: null = all 1
  double *c;                // [npix]
  double *coef;             // [ncomp][npix]
  double *basis;            // U [nseg][nexp][ncomp]
  int64_t npix, ntiles, nrows;      // nrows = nexp * nseg
  int32_t nexp, nseg, ncomp, comp;  // comp: the component being fitted
};

__global__ __launch_bounds__(kPixBlock) void k_sysrem_inject(SysremInjectArgs A)
{
  const int64_t k = (int64_t)blockIdx.x * kPixBlock + threadIdx.x;
  if (k >= A.cells) return;
  const int64_t p = k % A.npix;
  const double2 ab = A.pairs[k];
  A.r[k] = sysrem_inject(A.raw[k], ab.x, ab.y, A.gain ? A.gain[p] : 1.0, A.p0, A.p1);
}

__global__ __launch_bounds__(64 * kFiltWaves) void k_sysrem_cols(SysremArgs A)
{
  tile_column<kFiltWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) {
    const bool hasw = A.weight != nullptr;
    A.c[p] = sysrem_column_step(A.r + p, hasw ? A.weight + p : nullptr, hasw, A.a ? A.a + (int64_t)T.seg * A.nexp : nullptr, A.npix, A.nexp);
  });
}

__global__ __launch_bounds__(64 * kMomWaves) void k_sysrem_rows(SysremArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t row = (int64_t)blockIdx.x * kMomWaves + (threadIdx.x >> 6);
  if (row >= A.nrows) return;                          // (a whole wave: the butterfly below has all its lanes)
  const int64_t v = row / A.nseg, s = row - v * A.nseg;
  const int64_t first = A.seg_first[s], last = A.seg_first[s + 1];
  const int64_t base = v * A.npix;
  double num = 0.0, den = 0.0;
  for (int64_t p0 = first; p0 < last; p0 += 64 * kMomTrips) {
    double r[kMomTrips], w[kMomTrips], c[kMomTrips]; bool in[kMomTrips];
#pragma unroll
    for (int t = 0; t < kMomTrips; t++) {
      const int64_t q = p0 + 64 * t + lane;
      in[t] = q < last;
      const int64_t p = in[t] ? q : last - 1;
      r[t] = A.r[base + p];
      w[t] = A.weight ? A.weight[base + p] : 1.0;
      c[t] = A.c[p];
    }
#pragma unroll
    for (int t = 0; t < kMomTrips; t++)
      if (in[t]) sysrem_row_term(w[t], r[t], c[t], num, den);
  }
  num = wave_sum(num); den = wave_sum(den);
  if (lane == 0) A.a[s * A.nexp + v] = sysrem_ratio(num, den);
}

__global__ __launch_bounds__(64 * kFiltWaves) void k_sysrem_close(SysremArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t tile = (int64_t)blockIdx.x * kFiltWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= A.ntiles) return;
  const FilterTile T = A.tiles[tile];
  const int nexp = A.nexp;
  const double *const a = A.a + (int64_t)T.seg * nexp;
  const double t = sysrem_norm(a, nexp);
  if (T.first == A.seg_first[T.seg])
    for (int v = lane; v < nexp; v += 64) A.basis[((int64_t)T.seg * nexp + v) * A.ncomp + A.comp] = sysrem_close_a(a[v], t);
  if (lane >= T.count) return;
  const int64_t p = T.first + lane;
  A.coef[(int64_t)A.comp * A.npix + p] = sysrem_close_c(A.c[p], t);
}

__global__ __launch_bounds__(64 * kFiltWaves) void k_sysrem_subtract(SysremArgs A)
{
  tile_column<kFiltWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) {
    sysrem_column_subtract(A.r + p, A.basis + (int64_t)T.seg * A.nexp * A.ncomp + A.comp, A.ncomp, A.coef[(int64_t)A.comp * A.npix + p], A.npix, A.nexp);
  });
}

}  // namespace trx
