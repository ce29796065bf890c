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
//   k_norm_cols       one lane per pixel column, a wave per tile of <= 64 columns of one segment, in place in the call's
//                    buffer: the sum of f1 = f0 / scale over the entries live in a good row (v ascending, the loads of
//                    kSysTrips exposures issued before the first add), the centre, with a clip the mean and the squares of
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

// one column, in place; HASW: the set has weights (without: every W is 1, nothing is loaded for it).  A template, not a test
// per load: the loads of a trip must all be issued before the first is waited for.  PASS 0: n and the sum of f1; 1: the sum
// of f2; 2: the squares of f2 about the mean
template <bool HASW, int PASS>
__device__ __forceinline__ void norm_column_pass(const NormArgs &A, int64_t p, const double *scale, double c, double mean, int32_t &n, double &acc)
{
#pragma clang fp contract(off)
  const int nexp = A.nexp;
  for (int v0 = 0; v0 < nexp; v0 += kSysTrips) {
    double w[kSysTrips], r[kSysTrips], sc[kSysTrips];
#pragma unroll
    for (int t = 0; t < kSysTrips; t++) {
      const int v = min(v0 + t, nexp - 1);
      const int64_t at = (int64_t)v * A.npix + p;
      r[t] = A.r[at];
      w[t] = HASW ? A.weight[at] : 1.0;
      sc[t] = scale[(int64_t)v * A.nseg];
    }
#pragma unroll
    for (int t = 0; t < kSysTrips; t++)
      if (v0 + t < nexp) {
        const bool on = norm_on(w[t], sc[t]);
        // (an entry that takes no part is not divided: its scale may be +0)
        if (PASS == 0) norm_sum_term(on, on ? norm_row(A.row_kind, r[t], sc[t]) : 0.0, n, acc);
        else if (PASS == 1) { int32_t unused = 0; norm_sum_term(on, on ? norm_entry(A.row_kind, A.col_kind, r[t], sc[t], c) : 0.0, unused, acc); }
        else norm_square_term(on, on ? norm_entry(A.row_kind, A.col_kind, r[t], sc[t], c) : 0.0, mean, acc);
      }
  }
}

template <bool HASW>
__device__ __forceinline__ void norm_column(const NormArgs &A, int64_t p, int32_t seg)
{
#pragma clang fp contract(off)
  const int nexp = A.nexp;
  const double *const scale = A.scale + seg;           // scale[v * nseg] is this segment's at exposure v
  int32_t n = 0; double s = 0.0;
  norm_column_pass<HASW, 0>(A, p, scale, 0.0, 0.0, n, s);
  bool good;
  const double c = norm_centre(A.col_kind, s, n, good);
  const bool clips = norm_clips(A.clip, n, good);
  double mean = 0.0, lim = 0.0;
  if (clips) {
    int32_t unused = 0; double s2 = 0.0, q = 0.0;
    norm_column_pass<HASW, 1>(A, p, scale, c, 0.0, unused, s2);
    mean = norm_mean(s2, n);
    norm_column_pass<HASW, 2>(A, p, scale, c, mean, unused, q);
    lim = norm_limit(A.clip, q, n);
  }
  int32_t nclip = 0, nbad = 0;
  for (int v0 = 0; v0 < nexp; v0 += kSysTrips) {
    double w[kSysTrips], r[kSysTrips], sc[kSysTrips];
#pragma unroll
    for (int t = 0; t < kSysTrips; t++) {
      const int v = min(v0 + t, nexp - 1);
      const int64_t at = (int64_t)v * A.npix + p;
      r[t] = A.r[at];
      w[t] = HASW ? A.weight[at] : 1.0;
      sc[t] = scale[(int64_t)v * A.nseg];
    }
#pragma unroll
    for (int t = 0; t < kSysTrips; t++)
      if (v0 + t < nexp) {
        const bool on = norm_on(w[t], sc[t]) && good;
        double out = 0.0;
        if (on) {
          out = norm_entry(A.row_kind, A.col_kind, r[t], sc[t], c);
          if (clips && norm_clipped(out, mean, lim)) { out = mean; nclip++; }
        } else if (w[t] > 0.0) nbad++;
        A.r[(int64_t)(v0 + t) * A.npix + p] = out;
      }
  }
  A.centre[p] = c;
  A.count[p] = nclip;
  A.count[A.npix + p] = nbad;
}

__global__ __launch_bounds__(64 * kNormWaves) void k_norm_cols(NormArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t tile = (int64_t)blockIdx.x * kNormWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= A.ntiles) return;
  const FilterTile T = A.tiles[tile];
  if (lane >= T.count) return;
  if (A.weight) norm_column<true>(A, T.first + lane, T.seg); else norm_column<false>(A, T.first + lane, T.seg);
}

}  // namespace trx
