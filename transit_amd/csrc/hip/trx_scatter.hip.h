// trx_scatter.hip.h -- weighing the observed set by the scatter of its pixel columns on the device (trx_weigh_observed,
// include/transit_hip.h): every column's variance in time, every segment's median variance, and the new weights -- the
// inverse variance of the columns kept, or a mask of them.  The arithmetic is ../trx_scatter.h's, the same source a CPU
// program runs.
//
//   k_scatter_cols     one lane per pixel column, kScatBlock columns per block, a wave's loads coalesced.  The lane's column
//                    is scatter_column of ../trx_scatter.h: two passes over the exposures, v ascending in trips of
//                    kSysTrips (exposure_trips' loop of ../trx_columns.h, written out there): the
//                    count and the sum, then the squares about the mean.  Writes var[p]: > 0 for a live column, +0 for a
//                    dead one.
//   k_scatter_median   one block per tile of scatter_tiles (<= kScatBlock columns of one segment), a wave owning 64 of the
//                    tile's columns as candidates.  The block stages the segment's variances through LDS, kScatLds at a
//                    time (padded to a multiple of kScatTrip), a dead column's +0 as +infinity -- every lane of the block takes every trip of that loop, the
//                    two barriers in it are block-uniform --, and every lane counts the staged values ahead of its own
//                    candidate (all lanes read the same LDS word: a broadcast).  The live columns are counted as they are
//                    staged: a ballot per wave, the waves' totals added through LDS -- integers, exact in any order.  The
//                    one live lane of the segment whose rank is (m - 1) / 2 stores med[s]; med is zeroed before the launch,
//                    which is the answer of an empty segment (no tile) and of one without a live column (no lane stores).
//   k_scatter_weights  one block per tile, one lane per column (scatter_weights_column): the keep rule and 1 / var once, then
//                    the column's new weights for every exposure (exposure_trips' trips of kSysTrips) and the column's flag.
//
// No atomics, no scratch; LDS in k_scatter_median alone (kScatLds doubles and a count per wave).  The bits of a segment's result depend on that
// segment's data and weights and on the call's parameters -- not on other segments, the launch or the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "trx_sysrem.hip.h"
#include "../trx_scatter.h"

namespace trx {

struct ScatterArgs {
  const double *r;          // [nexp][npix] the data installed
  const double *weight;     // W [nexp][npix] as trx_set_observed installed it, or null: all 1
  const FilterTile *tiles;  // [ntiles], scatter_tiles'
  const int64_t *seg_first; // [nseg + 1]
  double *var;              // [npix]
  double *med;              // [nseg]
  double *out;              // w' [nexp][npix]
  int32_t *flag;            // [npix]: kScatDead, kScatKept, kScatClipped
  int64_t npix, ntiles;
  int32_t nexp, kind, min_live;
  double clip;
};

__global__ __launch_bounds__(kScatBlock) void k_scatter_cols(ScatterArgs A)
{
  const int64_t p = (int64_t)blockIdx.x * kScatBlock + threadIdx.x;
  if (p >= A.npix) return;
  A.var[p] = A.weight ? scatter_column<true>(A.r + p, A.weight + p, A.npix, A.nexp, A.min_live) : scatter_column<false>(A.r + p, nullptr, A.npix, A.nexp, A.min_live);
}

static_assert(kScatLds % kScatTrip == 0 && kScatBlock % 64 == 0, "a padded trip fits the staging array; whole waves");

__global__ __launch_bounds__(kScatBlock) void k_scatter_median(ScatterArgs A)
{
  __shared__ double staged[kScatLds];
  __shared__ long long live_of_wave[kScatBlock / 64];
  const int lane = (int)threadIdx.x;
  const FilterTile T = A.tiles[blockIdx.x];            // (the grid is the tile table: ntiles blocks)
  const int64_t first = A.seg_first[T.seg], last = A.seg_first[T.seg + 1];
  const bool mine = lane < T.count;
  const int64_t p = T.first + (mine ? lane : 0);       // (a lane past the tile's end counts for the tile's first column and stores nothing)
  const double varp = A.var[p];
  long long live = 0, rank = 0;                        // live: the live columns this lane's WAVE has staged (wave-uniform)
  for (int64_t q0 = first; q0 < last; q0 += kScatLds) {
    const int nq = last - q0 < kScatLds ? (int)(last - q0) : kScatLds;
    const int pj = scatter_place(p, q0);
    __syncthreads();                                   // (the trip before has been read by every lane)
    const int npad = scatter_padded(nq);               // (<= kScatLds: kScatTrip divides it)
    for (int j0 = 0; j0 < npad; j0 += kScatBlock) {    // (block-uniform: every lane takes every trip, the ballot has whole waves)
      const int j = j0 + lane;
      const double x = j < nq ? A.var[q0 + j] : 0.0;   // (the padding is staged as a dead column: ahead of nothing)
      if (j < npad) staged[j] = scatter_staged(x);
      live += __popcll(__ballot(x > 0.0));
    }
    __syncthreads();
    int ahead = 0;
    for (int j0 = 0; j0 < npad; j0 += kScatTrip) {
      double x[kScatTrip];
#pragma unroll
      for (int t = 0; t < kScatTrip; t++) x[t] = staged[j0 + t];
#pragma unroll
      for (int t = 0; t < kScatTrip; t++) scatter_rank_term(x[t], j0 + t, varp, pj, ahead);
    }
    rank += ahead;
  }
  if ((lane & 63) == 0) live_of_wave[lane >> 6] = live;
  __syncthreads();
  long long m = 0;
  for (int k = 0; k < kScatBlock / 64; k++) m += live_of_wave[k];
  if (mine && scatter_is_median(varp, m, rank)) A.med[T.seg] = varp;
}

__global__ __launch_bounds__(kScatBlock) void k_scatter_weights(ScatterArgs A)
{
  const int lane = (int)threadIdx.x;
  const FilterTile T = A.tiles[blockIdx.x];
  if (lane >= T.count) return;
  const int64_t p = T.first + lane;
  const bool hasw = A.weight != nullptr;
  scatter_weights_column(A.var[p], A.med[T.seg], A.clip, A.kind, hasw ? A.weight + p : nullptr, hasw, A.out + p, A.flag[p], A.npix, A.nexp);
}

}  // namespace trx
