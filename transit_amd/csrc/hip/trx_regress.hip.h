// trx_regress.hip.h -- regressing the observed set on given time vectors on the device (trx_regress_observed,
// include/transit_hip.h): the weighted filter's projector (trx_wfilter.hip.h) applied to the data instead of the model.
// Every column p has its own least-squares fit of its segment's vectors U ([nexp][nvec]) under its own weights
// w[v] = W[v][p]:
//   r = f0 - U (U^T diag(w) U)^-1 U^T diag(w) f0
// The column's factor is k_wfilter_factor's, made from the same vectors and weights for the filter the call installs; the
// arithmetic is ../trx_regress.h's composition of ../trx_wfilter.h's functions, the same source a CPU program runs.
//
//   k_regress_cols<NC>  k_pixel_wfilter's shape: one lane per pixel column, one wavefront per tile of the sysrem_tiles table,
//                    kFiltWaves tiles per block.  Pass 1 walks v upwards -- f0 and the weight (16 bytes per lane, coalesced)
//                    and NC accumulators y in registers, the vectors through wave-uniform loads; then the solve, the
//                    column's factor entries loaded as they are used (coalesced, each once per triangle); pass 2 walks v
//                    again -- f0 once more, r_v from U and the coefficients, and the residual written over f0 in place.
//                    Both passes walk in exposure_trips' trips of kFiltTrips (../trx_columns.h); the prologue is
//                    tile_column's.  coef[j][p] is written
//                    between the passes.  A column with a singular pivot gets the coefficients +0 and keeps f0.
//
// No LDS, no cross-lane operation, no atomics: a lane past the tile's end loads and stores nothing.  The bits of a column's
// residuals and coefficients depend on its own f0 and weights and on its segment's vectors and nvec -- not on NC, other
// columns or segments, the launch, or the handle that ran it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "trx_filter.hip.h"
#include "../trx_regress.h"

namespace trx {

static_assert(kRegressTrips == kFiltTrips, "regress_column walks the exposures the way the filter kernels do");

struct RegressArgs {
  double *r;                // [nexp][npix]: f0 in, the residuals out
  const double *weight;     // [nexp][npix], or null: all 1
  const double *basis;      // [nseg][nexp][NC], zero-padded
  const double *fac;        // [nfac][npix]
  const int32_t *live;      // [npix]: 1 no pivot singular, 0 one was
  const FilterTile *tiles;  // [ntiles]
  double *coef;             // [nvec][npix]
  int64_t npix, ntiles;
  int32_t nexp, nvec;
};

template <int NC>
__global__ __launch_bounds__(64 * kFiltWaves) void k_regress_cols(RegressArgs A)
{
  tile_column<kFiltWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) {
    const bool hasw = A.weight != nullptr;
    regress_column<NC>(A.basis + (int64_t)T.seg * A.nexp * NC, hasw ? A.weight + p : nullptr, hasw, A.r + p, A.fac + p, A.live[p] != 0, A.coef + p,
                       A.npix, A.nexp, A.nvec);
  });
}

}  // namespace trx
