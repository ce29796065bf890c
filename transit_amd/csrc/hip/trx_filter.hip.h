// trx_filter.hip.h -- the detrending filter of the detector pixels on the device, between the pixel pairs and their
// moments (trx_set_filter / trx_run_filtered_moments, include/transit_hip.h).
//
// Observed exposures are detrended before they are compared with a model: per spectral order (a SEGMENT) the leading
// components in time are fitted and taken out, and the same linear map has to be applied to the model (Brogi & Line
// 2019 in the linear form of Gibson et al. 2022, M' = M - U (U^+ M)).  It acts along the EXPOSURE axis of one pixel
// column: with g[v] = gain_p * (a / b) from the column's pairs, C = fwd[s] ([ncomp][nexp]) and B = back[s]
// ([nexp][ncomp]) of the column's segment,
//   c_j   = sum over v = 0 .. nexp-1, in that order, of C[j][v] * g[v]
//   r_v   = sum over j = 0 .. ncomp-1, in that order, of B[v][j] * c_j
//   g'[v] = g[v] - r_v
// every product and sum rounded once (no contraction), both sums started from +0.  A column with b > 0 at every
// exposure is LIVE; any other is DEAD and all its values are quiet NaN (the projection needs the whole column).
//
//   k_pixel_filter<NC>  one lane per pixel column, one wavefront per TILE of up to 64 consecutive pixels of one
//                    segment (the tile table is made at trx_set_filter: tiles never cross a segment), kFiltWaves
//                    tiles per block.  The segment's matrices are wave-uniform: the device holds them zero-padded to
//                    NC components and exposure-major, fwd as [nseg][nexp][NC] and back as [nseg][nexp][NC], so that
//                    an exposure's NC coefficients are consecutive doubles at a uniform address (loads only).  A
//                    padded component adds exact zeros to r_v: the bits do not depend on NC.
//                    Pass 1 walks v upwards: the pair (16 bytes per lane, coalesced), g, the live flag, and NC
//                    accumulators in registers.  Pass 2 walks v again: the pair once more (from L2), the same g,
//                    r_v, and g' or NaN to val[v][p], coalesced.  Both passes issue the loads of kFiltTrips
//                    exposures before they use the first.  No LDS, no cross-lane operation, no atomics: a lane past
//                    the tile's end computes and stores nothing.
//
// The bits of a value depend on its column's pairs and gain and on its segment's matrices and ncomp -- not on other
// columns or segments, the launch, the handle that ran it or the run's step plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "../trx_columns.h"

namespace trx {

constexpr int kFiltWaves = 4;                         // tiles (waves) per block (kFiltTrips: ../trx_columns.h)

// The prologue of a kernel of one wavefront per tile, WAVES tiles per block, one lane per pixel column: column(T, p) with the
// wave's tile T and the lane's column p; a wave past the last tile and a lane past its tile's end do nothing.  The wave's
// number is a value the compiler knows to be the same in all its lanes: what follows from it -- the tile, its segment, the
// addresses of the segment's matrices and vectors -- is read through scalar loads.  (The column is a callable and not a
// returned flag: the two early returns stay two plain branches, as written out in a kernel.)
template <int WAVES, class Column>
__device__ __forceinline__ void tile_column(const FilterTile *tiles, int64_t ntiles, Column column)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t tile = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= ntiles) return;
  const FilterTile T = tiles[tile];
  if (lane >= T.count) return;
  column(T, T.first + lane);
}

struct FilterArgs {
  const double2 *pairs;     // [nexp][npix] (a, b): d_pixout of this run
  const double *gain;       // [npix], or null: all 1
  const double *fwd;        // [nseg][nexp][NC], zero-padded
  const double *back;       // [nseg][nexp][NC], zero-padded
  const FilterTile *tiles;  // [ntiles]
  double *val;              // [nexp][npix]: g' or NaN
  int64_t npix, ntiles;
  int32_t nexp;
};

template <int NC>
__global__ __launch_bounds__(64 * kFiltWaves) void k_pixel_filter(FilterArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  // (the wave's number, as a value the compiler knows to be the same in all its lanes: what follows from it -- the
  // tile, its segment, the matrices' addresses -- is read through scalar loads)
  const int64_t tile = (int64_t)blockIdx.x * kFiltWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= A.ntiles) return;
  const FilterTile T = A.tiles[tile];
  if (lane >= T.count) return;
  const int64_t p = T.first + lane;
  const int nexp = A.nexp;
  const double gn = A.gain ? A.gain[p] : 1.0;
  const double *const F = A.fwd + (int64_t)T.seg * nexp * NC, *const B = A.back + (int64_t)T.seg * nexp * NC;
  double c[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) c[j] = 0.0;
  bool live = true;
  // pass 1: the coefficients.  kFiltTrips exposures at a time: their loads first (a trip past the last exposure reads
  // the last one again and adds nothing), then their terms in exposure order
  for (int v0 = 0; v0 < nexp; v0 += kFiltTrips) {
    double2 ab[kFiltTrips];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++) ab[t] = A.pairs[(int64_t)min(v0 + t, nexp - 1) * A.npix + p];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++)
      if (v0 + t < nexp) {
        live = live && ab[t].y > 0.0;
        const double g = gn * (ab[t].x / ab[t].y);
        const double *const Fv = F + (int64_t)(v0 + t) * NC;
#pragma unroll
        for (int j = 0; j < NC; j++) c[j] += Fv[j] * g;
      }
  }
  // pass 2: the values
  const double nan = __builtin_nan("");
  for (int v0 = 0; v0 < nexp; v0 += kFiltTrips) {
    double2 ab[kFiltTrips];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++) ab[t] = A.pairs[(int64_t)min(v0 + t, nexp - 1) * A.npix + p];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++)
      if (v0 + t < nexp) {
        const double g = gn * (ab[t].x / ab[t].y);
        const double *const Bv = B + (int64_t)(v0 + t) * NC;
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < NC; j++) r += Bv[j] * c[j];
        A.val[(int64_t)(v0 + t) * A.npix + p] = live ? g - r : nan;
      }
  }
}

}  // namespace trx
