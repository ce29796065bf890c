// trx_cellmap.hip.h -- the Kp-Vsys detection map with the detrending filter applied to every cell's own model matrix
// (trx_run_filtered_map, include/transit_hip.h).
//
// The filter couples the exposures of a pixel column, and in a map cell the model at exposure v sits at that cell's own
// velocity: the column is not a constant, and the filtered model differs from cell to cell.  One pixel pass at the lags
// leaves the rows G[l][p] (pairs, [nlag][npix]) in device memory; a cell (i, j) takes at exposure v the row of the lag
// NEAREST to its velocity (vmap_nearest, ../trx_vmap.h), and its matrix M[v][p] = G[k_v][p] goes through the filter of
// trx_filter.hip.h and the <true> moments of trx_moments.hip.h as the matrix of trx_run_filtered_moments does: the same
// operations in the same order, so the same bits.  The cells go through in chunks (cell_map_extents, ../trx_products.h).
//
//   k_cell_tracks    once, for all cells: one lane per (cell, exposure) writes index[cell][v] = k_v, or -1 for a velocity
//                    outside the lag grid or not finite.  A cell with a -1 is OUTSIDE: the three kernels below leave it out
//                    by the whole wave, and its map value is NaN.
//   k_cell_filter<NC>  k_pixel_filter with the row of exposure v taken from the cell's index table: one wavefront per
//                    (cell of the chunk, tile of the filter's tile table), kFiltWaves per block, one lane per pixel
//                    column.  The table entries are wave-uniform loads, a lane's loads stay coalesced along the pixel
//                    axis; many cells read the same rows, which stay in L2.  It writes val[c][v][p], g' or NaN.
//   k_cell_moments   k_pixel_moments<true> with rows (c, v, s): val indexed by (c, v), data and weights by v.  Lane l adds
//                    the segment's pixels first + l, first + l + 64, ... in that order, then wave_sum's butterfly.
//   k_cell_stat      one wavefront per cell of the chunk.  Lane k takes exposure v0 + k and adds vmap_stat of its nseg
//                    rows in segment order from +0, undefined rows skipped (vmap_add_stat); then the wave adds the
//                    exposures' sums in exposure order from +0 (wave_add_in_order).  NaN for a cell that is outside.
//
// No atomics, no LDS.  A cell's bits depend on its own index row, the rows G it names, the observed set and the filter --
// not on the other cells, the chunk it was computed in or its place there, or the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"
#include "trx_filter.hip.h"
#include "trx_moments.hip.h"
#include "trx_vmap.hip.h"
#include "../trx_vmap.h"

namespace trx {

constexpr int kCellStatWaves = 4;                     // cells (waves) per block of k_cell_stat

struct CellTrackArgs {
  const double *lag_kms;    // [nlag]
  const double *kp, *vsys;  // [nkp], [nvsys]
  const double *orbit;      // [nexp]
  const double *offset;     // [nexp], or null: none
  int32_t *index;           // [ncells][nexp]: the nearest lag, or -1
  int64_t ntracks;          // ncells * nexp
  int32_t nlag, nexp, nvsys;
};

struct CellFilterArgs {
  const double2 *pairs;     // [nlag][npix] (a, b): d_pixout (d_pixhp with a high-pass) of this run
  const double *gain;       // [npix], or null: all 1
  const double *fwd;        // [nseg][nexp][NC], zero-padded
  const double *back;       // [nseg][nexp][NC], zero-padded
  const FilterTile *tiles;  // [ntiles]
  const int32_t *index;     // [nexp] per cell, the chunk's first cell first
  double *val;              // [ncells][nexp][npix]: g' or NaN
  int64_t npix, ntiles, nwaves;      // nwaves = ncells * ntiles
  int32_t nexp;
};

struct CellMomArgs {
  const double *val;        // [ncells][nexp][npix]
  const double *data;       // [nexp][npix]
  const double *weight;     // [nexp][npix], or null: all 1
  const int64_t *seg_first; // [nseg + 1]
  const int32_t *index;     // [nexp] per cell, the chunk's first cell first
  double *mom;              // [ncells][nexp][nseg][TRX_NMOMENT]
  int64_t npix, nrows;      // nrows = ncells * nexp * nseg
  int32_t nexp, nseg;
};

struct CellStatArgs {
  const double *mom;        // [ncells][nexp][nseg][TRX_NMOMENT]
  const int32_t *index;     // [nexp] per cell, the chunk's first cell first
  double *map;              // [ncells], the chunk's first cell first
  int64_t ncells;
  int32_t nexp, nseg, stat;
  double p0, p1;
};

// a cell whose index row idx[0 .. nexp-1] has a -1; idx the same in all lanes of the wave (scalar loads)
__device__ __forceinline__ bool cell_is_outside(const int32_t *idx, int nexp)
{
  bool out = false;
  for (int v = 0; v < nexp; v++) out = out || idx[v] < 0;
  return out;
}

__global__ __launch_bounds__(kCellTrackBlock) void k_cell_tracks(CellTrackArgs A)
{
#pragma clang fp contract(off)
  const int64_t k = (int64_t)blockIdx.x * kCellTrackBlock + threadIdx.x;
  if (k >= A.ntracks) return;
  const int64_t cell = k / A.nexp, v = k - cell * A.nexp;
  const double x = vmap_track(A.kp[cell / A.nvsys], A.vsys[cell % A.nvsys], A.orbit[v], A.offset, v);
  A.index[k] = vmap_nearest(A.lag_kms, A.nlag, x);
}

template <int NC>
__global__ __launch_bounds__(64 * kFiltWaves) void k_cell_filter(CellFilterArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t w = (int64_t)blockIdx.x * kFiltWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= A.nwaves) return;
  const int64_t c = w / A.ntiles, tile = w - c * A.ntiles;
  const int nexp = A.nexp;
  const int32_t *const idx = A.index + c * nexp;
  if (cell_is_outside(idx, nexp)) return;              // (a whole wave)
  const FilterTile T = A.tiles[tile];
  if (lane >= T.count) return;
  const int64_t p = T.first + lane;
  const double gn = A.gain ? A.gain[p] : 1.0;
  const double *const F = A.fwd + (int64_t)T.seg * nexp * NC, *const B = A.back + (int64_t)T.seg * nexp * NC;
  double *const val = A.val + c * nexp * A.npix;
  double cf[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) cf[j] = 0.0;
  bool live = true;
  // pass 1: the coefficients, as k_pixel_filter takes them -- exposure v's pair from row idx[v]
  for (int v0 = 0; v0 < nexp; v0 += kFiltTrips) {
    double2 ab[kFiltTrips];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++) ab[t] = A.pairs[(int64_t)idx[min(v0 + t, nexp - 1)] * A.npix + p];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++)
      if (v0 + t < nexp) {
        live = live && ab[t].y > 0.0;
        const double g = gn * (ab[t].x / ab[t].y);
        const double *const Fv = F + (int64_t)(v0 + t) * NC;
#pragma unroll
        for (int j = 0; j < NC; j++) cf[j] += Fv[j] * g;
      }
  }
  // pass 2: the values
  const double nan = __builtin_nan("");
  for (int v0 = 0; v0 < nexp; v0 += kFiltTrips) {
    double2 ab[kFiltTrips];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++) ab[t] = A.pairs[(int64_t)idx[min(v0 + t, nexp - 1)] * A.npix + p];
#pragma unroll
    for (int t = 0; t < kFiltTrips; t++)
      if (v0 + t < nexp) {
        const double g = gn * (ab[t].x / ab[t].y);
        const double *const Bv = B + (int64_t)(v0 + t) * NC;
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < NC; j++) r += Bv[j] * cf[j];
        val[(int64_t)(v0 + t) * A.npix + p] = live ? g - r : nan;
      }
  }
}

__global__ __launch_bounds__(64 * kMomWaves) void k_cell_moments(CellMomArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t row = (int64_t)blockIdx.x * kMomWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (row >= A.nrows) return;                          // (a whole wave: the butterfly below has all its lanes)
  const int64_t cv = row / A.nseg, s = row - cv * A.nseg;      // cv = c * nexp + v
  const int64_t c = cv / A.nexp, v = cv - c * A.nexp;
  if (cell_is_outside(A.index + c * A.nexp, A.nexp)) return;   // (a whole wave)
  const int64_t first = A.seg_first[s], last = A.seg_first[s + 1];
  const double *const val = A.val + cv * A.npix;
  const int64_t base = v * A.npix;
  double n = 0.0, sw = 0.0, swg = 0.0, swgg = 0.0, swf = 0.0, swfg = 0.0, swff = 0.0;
  // kMomTrips trips at a time, as k_pixel_moments<true> takes them: a lane's sum is in the order of its pixels
  for (int64_t p0 = first; p0 < last; p0 += 64 * kMomTrips) {
    double g[kMomTrips], f[kMomTrips], wt[kMomTrips]; bool in[kMomTrips];
#pragma unroll
    for (int t = 0; t < kMomTrips; t++) {
      const int64_t q = p0 + 64 * t + lane;
      in[t] = q < last;
      const int64_t p = in[t] ? q : last - 1;
      g[t] = val[p];
      f[t] = A.data[base + p];
      wt[t] = A.weight ? A.weight[base + p] : 1.0;
    }
#pragma unroll
    for (int t = 0; t < kMomTrips; t++)
      if (in[t] && g[t] == g[t] && wt[t] > 0.0) {
        const double wg = wt[t] * g[t], wf = wt[t] * f[t];
        n += 1.0; sw += wt[t]; swg += wg; swgg += wg * g[t]; swf += wf; swfg += wf * g[t]; swff += wf * f[t];
      }
  }
  n = wave_sum(n); sw = wave_sum(sw); swg = wave_sum(swg); swgg = wave_sum(swgg);
  swf = wave_sum(swf); swfg = wave_sum(swfg); swff = wave_sum(swff);
  // (every lane holds the seven sums: lanes 0 .. 6 store one each)
  const double r = lane == 0 ? n : lane == 1 ? sw : lane == 2 ? swg : lane == 3 ? swgg : lane == 4 ? swf : lane == 5 ? swfg : swff;
  if (lane < TRX_NMOMENT) A.mom[row * TRX_NMOMENT + lane] = r;
}

__global__ __launch_bounds__(64 * kCellStatWaves) void k_cell_stat(CellStatArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  const int64_t c = (int64_t)blockIdx.x * kCellStatWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (c >= A.ncells) return;                           // (a whole wave: the in-order sum below has all its lanes)
  if (cell_is_outside(A.index + c * A.nexp, A.nexp)) {
    if (lane == 0) A.map[c] = vmap_nan();
    return;
  }
  double acc = 0.0;
  for (int32_t v0 = 0; v0 < A.nexp; v0 += 64) {
    const int32_t v = v0 + lane;
    double per = 0.0;
    if (v < A.nexp) {
      const double *m0 = A.mom + (c * A.nexp + v) * A.nseg * TRX_NMOMENT;
      for (int32_t s = 0; s < A.nseg; s++) {
        double m[TRX_NMOMENT];
#pragma unroll
        for (int k = 0; k < TRX_NMOMENT; k++) m[k] = m0[(int64_t)s * TRX_NMOMENT + k];
        per = vmap_add_stat(per, vmap_stat(m, A.stat, A.p0, A.p1));
      }
    }
    acc = wave_add_in_order<false>(acc, per, A.nexp - v0 < 64 ? A.nexp - v0 : 64);
  }
  if (lane == 0) A.map[c] = acc;
}

}  // namespace trx
