// trx_normalise.hip.h -- normalising the observed set on the device, step 1b of a detrending call (trx_set_normalise,
// trx_normalise_observed, include/transit_hip.h): every (exposure, segment) row's quantile, every column's centre in time,
// the centred data and the clip of single entries.  The arithmetic is ../trx_normalise.h's, the same source a CPU program runs.
//
//   k_norm_rowscale   one block of kNormBlock lanes per row (v, s): an exact selection of the value of rank k among the row's
//                    live data by bisecting the order-preserving 64-bit key of a double from the top bit down.  A lane keeps
//                    the keys of kNormPerLane of the row's first kNormCap pixels in registers (a dead entry's key is above
//                    every trial); the pixels of a longer row past kNormCap are read from global memory again at every step
//                    -- no cap on a segment's length.  A step counts the keys below the trial: a ballot and a popcount per
//                    wave and key, the waves' totals added through LDS (two slots in turn: one barrier per step) -- integers,
//                    exact in any order.  Every lane of the block takes every trip of every loop: their counts come from the
//                    segment's length alone, the barriers are block-uniform.  Lane 0 stores scale[v][s]; the array is zeroed
//                    before the launch.  With row_kind NONE only the live entries are counted.
//   k_norm_cols       one lane per pixel column, a wave per tile of <= 64 columns of one segment (tile_column), in place in
//                    the call's buffer.  The lane's column is norm_column of ../trx_normalise.h: the sum of f1 = f0 / scale
//                    over the entries live in a good row (v ascending in trips of kSysTrips, exposure_trips' loop of
//                    ../trx_columns.h written out there), the centre, with a clip the mean and the squares of
//                    f2, then the pass that writes f2 -- the mean where the clip takes the entry, +0 where the entry is dead
//                    or its row or column bad --, centre[p] and the column's two counts.  Every pass forms f1 and f2 again
//                    from f0: the same operations, the same bits.
//
// No atomics, no scratch; LDS in k_norm_rowscale alone (two counts per wave).  The bits of a segment's result depend on that
// segment's data and weights and on the recipe -- not on other segments, the launch or the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "trx_sysrem.hip.h"
#include "../trx_normalise.h"

namespace trx {

struct NormArgs {
  double *r;                // [nexp][npix] f0 in, the normalised data out (k_norm_cols, in place)
  const double *weight;     // W [nexp][npix] as trx_set_observed installed it, or null: all 1
  const FilterTile *tiles;  // [ntiles], sysrem_tiles'
  const int64_t *seg_first; // [nseg + 1]
  double *scale;            // [nexp][nseg]
  double *centre;           // [npix]
  int32_t *count;           // [2][npix]: the entries the clip replaced, the live entries that got +0
  int64_t npix, ntiles;
  int32_t nexp, nseg, row_kind, col_kind;
  double quantile, clip;
};

static_assert(kNormBlock % 64 == 0 && kNormCap == kNormBlock * kNormPerLane, "whole waves; the staged keys fill the lanes' registers");

// the block's total of a wave-uniform count: the waves' counts through LDS slot `slot`, one barrier (block-uniform)
__device__ __forceinline__ long long norm_block_total(long long mine, long long (*of_wave)[kNormBlock / 64], int slot)
{
  if ((threadIdx.x & 63) == 0) of_wave[slot][threadIdx.x >> 6] = mine;
  __syncthreads();
  long long total = 0;
#pragma unroll
  for (int k = 0; k < kNormBlock / 64; k++) total += of_wave[slot][k];
  return total;
}

__global__ __launch_bounds__(kNormBlock) void k_norm_rowscale(NormArgs A)
{
  // (two slots in turn: a step's totals are read before the next step's barrier, and written again only after it)
  __shared__ long long of_wave[2][kNormBlock / 64];
  const int lane = (int)threadIdx.x;
  const int64_t row = blockIdx.x;                      // (the grid is the rows: nexp * nseg blocks)
  const int64_t v = row / A.nseg, s = row - v * A.nseg;
  const int64_t first = A.seg_first[s], last = A.seg_first[s + 1];
  const int64_t len = last - first;                    // (block-uniform, as every loop bound below)
  const double *const f = A.r + v * A.npix + first;
  const double *const w = A.weight ? A.weight + v * A.npix + first : nullptr;
  const int64_t nstaged = len < kNormCap ? len : kNormCap;
  // the staged keys, and the live entries of the whole row
  uint64_t key[kNormPerLane];
  long long live = 0;
#pragma unroll
  for (int t = 0; t < kNormPerLane; t++) {
    const int64_t j = (int64_t)t * kNormBlock + lane;
    const bool in = j < nstaged;
    key[t] = in ? norm_staged(w ? w[j] : 1.0, f[j]) : kNormDeadKey;
    live += __popcll(__ballot(in && (w ? w[j] : 1.0) > 0.0));
  }
  for (int64_t j0 = kNormCap; j0 < len; j0 += kNormBlock) {
    const int64_t j = j0 + lane;
    live += __popcll(__ballot(j < len && (w ? w[j] : 1.0) > 0.0));
  }
  const int64_t m = norm_block_total(live, of_wave, 0);
  double x = 0.0;
  if (A.row_kind == TRX_NORM_ROW_QUANTILE && m >= 1) { // (block-uniform: m is the block's total)
    const int64_t k = norm_rank(A.quantile, m);
    uint64_t found = 0;
    for (int bit = kNormBits - 1; bit >= 0; bit--) {
      const uint64_t trial = norm_trial(found, bit);
      long long below = 0;
#pragma unroll
      for (int t = 0; t < kNormPerLane; t++) below += __popcll(__ballot(norm_below(key[t], trial)));
      for (int64_t j0 = kNormCap; j0 < len; j0 += kNormBlock) {
        const int64_t j = j0 + lane;
        const uint64_t kj = j < len ? norm_staged(w ? w[j] : 1.0, f[j]) : kNormDeadKey;
        below += __popcll(__ballot(norm_below(kj, trial)));
      }
      // (slot 1, 0, 1, ... from bit 63 down: the total of m above went through slot 0)
      found = norm_bisect_step(found, bit, norm_block_total(below, of_wave, bit & 1), k);
    }
    x = norm_unkey(found);
  }
  if (lane == 0) A.scale[row] = norm_scale(A.row_kind, x, m);
}

__global__ __launch_bounds__(64 * kNormWaves) void k_norm_cols(NormArgs A)
{
  tile_column<kNormWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) {
    const double *const scale = A.scale + T.seg;       // scale[v * nseg] is this segment's at exposure v
    if (A.weight) norm_column<true>(A.r, A.weight, scale, p, A.npix, A.nseg, A.nexp, A.row_kind, A.col_kind, A.clip, A.centre[p], A.count[p], A.count[A.npix + p]);
    else norm_column<false>(A.r, nullptr, scale, p, A.npix, A.nseg, A.nexp, A.row_kind, A.col_kind, A.clip, A.centre[p], A.count[p], A.count[A.npix + p]);
  });
}

}  // namespace trx
