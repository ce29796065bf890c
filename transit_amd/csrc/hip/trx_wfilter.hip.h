// trx_wfilter.hip.h -- the weighted detrending filter of the detector pixels on the device: the filter slot's second kind
// (trx_set_weighted_filter, include/transit_hip.h), between the pixel pairs and their moments where trx_filter.hip.h's is.
//
// The plain filter projects every pixel column of a segment with the same coefficients.  Here every column p has its own
// least-squares projector, from its own weights w[v] = weight[v][p] and its segment's time vectors U ([nexp][ncomp]):
//   g' = g - U (U^T diag(w) U)^-1 U^T diag(w) g
// The column's ncomp x ncomp normal matrix depends on the installed set only: it is factorised once, at install, and a
// run solves with the factor.  The arithmetic is ../trx_wfilter.h's, the same source a CPU program runs.
//
//   k_wfilter_factor<NC>  at install.  One lane per pixel column, one wavefront per tile of the filter's tile table,
//                    kFiltWaves tiles per block (tile_column).  The lane's column is wfilter_factor_column of
//                    ../trx_wfilter.h: for row j = 0 .. ncomp-1 one pass over the exposures (exposure_trips' trips of
//                    kFiltTrips, ../trx_columns.h) adds row j of the
//                    normal matrix (j + 1 accumulators in registers; the basis through wave-uniform loads, the weights
//                    coalesced), then row j of the factor is made from it and from the rows below j, which the lane reads
//                    back from where it stored them.  It writes fac[e][p] (component-major: coalesced) and live[p].
//   k_pixel_wfilter<NC>  the run.  k_pixel_filter's structure: pass 1 walks v upwards -- the pair and the weight (24 bytes
//                    per lane, coalesced), g, the b > 0 flag, and NC accumulators y in registers; then the solve, the
//                    column's factor entries loaded as they are used (coalesced, each once per triangle); pass 2 walks v
//                    again -- the pair once more, the same g, r_v from U and the coefficients, and g' or NaN to val[v][p].
//                    Both passes issue the loads of kFiltTrips exposures before they use the first.
//   k_cell_wfilter<NC>  the same with the pair of exposure v taken from row index[c][v] of the lag rows (the weight is
//                    exposure v's), one wavefront per (cell of the chunk, tile): k_cell_filter's relation to
//                    k_pixel_filter.  A cell with a -1 in its index row is left out by the whole wave.
//
// No LDS, no cross-lane operation, no atomics: a lane past the tile's end computes and stores nothing.  The bits of a
// value depend on its column's pairs, gain and weights and on its segment's basis and ncomp -- not on NC, other columns or
// segments, the launch, or the handle that ran it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "trx_filter.hip.h"
#include "../trx_wfilter.h"

namespace trx {

struct WfilterFactorArgs {
  const double *weight;     // [nexp][npix], or null: all 1
  const double *basis;      // [nseg][nexp][NC], zero-padded
  const FilterTile *tiles;  // [ntiles]
  double *fac;              // [nfac][npix]
  int32_t *live;            // [npix]: 1 no pivot singular, 0 one was
  int64_t npix, ntiles;
  int32_t nexp, ncomp;
};

struct WfilterArgs {
  const double2 *pairs;     // [nexp][npix] (a, b) of this run; the cell kernel: [nlag][npix]
  const double *gain;       // [npix], or null: all 1
  const double *weight;     // [nexp][npix], or null: all 1
  const double *basis;      // [nseg][nexp][NC], zero-padded
  const double *fac;        // [nfac][npix]
  const int32_t *live;      // [npix]
  const FilterTile *tiles;  // [ntiles]
  const int32_t *index;     // the cell kernel: [nexp] per cell, the chunk's first cell first
  double *val;              // [nexp][npix]: g' or NaN; the cell kernel: [ncells][nexp][npix]
  int64_t npix, ntiles, nwaves;      // the cell kernel: nwaves = ncells * ntiles
  int32_t nexp, ncomp;
};

template <int NC>
__global__ __launch_bounds__(64 * kFiltWaves) void k_wfilter_factor(WfilterFactorArgs A)
{
  tile_column<kFiltWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) {
    const bool hasw = A.weight != nullptr;
    const bool good = wfilter_factor_column<NC>(A.basis + (int64_t)T.seg * A.nexp * NC, hasw ? A.weight + p : nullptr, hasw, A.fac + p, A.npix, A.nexp, A.ncomp);
    A.live[p] = good ? 1 : 0;
  });
}

// one column p of the run: CELL: exposure v's pair from row idx[v] of the pairs
template <int NC, bool CELL>
__device__ __forceinline__ void wfilter_column(const WfilterArgs &A, const FilterTile &T, int64_t p, const int32_t *idx, double *val)
{
#pragma clang fp contract(off)
  const int nexp = A.nexp;
  const double gn = A.gain ? A.gain[p] : 1.0;
  const double *const U = A.basis + (int64_t)T.seg * nexp * NC;
  double y[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) y[j] = 0.0;
  bool live = A.live[p] != 0;
  // pass 1: the right-hand side.  kFiltTrips exposures at a time: their loads first (a trip past the last exposure reads
  // the last one again and adds nothing), then their terms in exposure order
  for (int v0 = 0; v0 < nexp; v0 += kFiltTrips) {
    double2 ab[kFiltTrips]; double w[kFiltTrips];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++) {
      const int v = min(v0 + t, nexp - 1);
      ab[t] = A.pairs[(int64_t)(CELL ? idx[v] : v) * A.npix + p];
      w[t] = A.weight ? A.weight[(int64_t)v * A.npix + p] : 1.0;
    }
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++)
      if (v0 + t < nexp) {
        live = live && ab[t].y > 0.0;
        wfilter_rhs_term<NC>(U + (int64_t)(v0 + t) * NC, w[t], gn * (ab[t].x / ab[t].y), y);
      }
  }
  // the coefficients, in place
  wfilter_solve<NC>(A.ncomp, y, A.fac + p, A.npix);
  // pass 2: the values
  const double nan = __builtin_nan("");
  for (int v0 = 0; v0 < nexp; v0 += kFiltTrips) {
    double2 ab[kFiltTrips];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++) {
      const int v = min(v0 + t, nexp - 1);
      ab[t] = A.pairs[(int64_t)(CELL ? idx[v] : v) * A.npix + p];
    }
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++)
      if (v0 + t < nexp) {
        const double gp = wfilter_value<NC>(U + (int64_t)(v0 + t) * NC, y, gn * (ab[t].x / ab[t].y));
        val[(int64_t)(v0 + t) * A.npix + p] = live ? gp : nan;
      }
  }
}

template <int NC>
__global__ __launch_bounds__(64 * kFiltWaves) void k_pixel_wfilter(WfilterArgs A)
{
  tile_column<kFiltWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) { wfilter_column<NC, false>(A, T, p, nullptr, A.val); });
}

template <int NC>
__global__ __launch_bounds__(64 * kFiltWaves) void k_cell_wfilter(WfilterArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t w = (int64_t)blockIdx.x * kFiltWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= A.nwaves) return;
  const int64_t c = w / A.ntiles, tile = w - c * A.ntiles;
  const int32_t *const idx = A.index + c * A.nexp;
  bool out = false;                                    // (cell_is_outside of trx_cellmap.hip.h: a whole wave)
  for (int v = 0; v < A.nexp; v++) out = out || idx[v] < 0;
  if (out) return;
  const FilterTile T = A.tiles[tile];
  if (lane >= T.count) return;
  wfilter_column<NC, true>(A, T, T.first + lane, idx, A.val + c * A.nexp * A.npix);
}

}  // namespace trx
