// trx_highpass.hip.h -- the high-pass of the detector pixels along each order on the device, between the pixel pairs
// and everything that reads them (trx_set_highpass / trx_run_highpassed, include/transit_hip.h).
//
// Observed exposures are continuum-normalised per spectral order (a SEGMENT) before they are compared with a model: a
// running weighted mean along the PIXEL axis is taken out, and the model goes through the same high-pass.  With
// g_q = gain_q * (a / b) from a row's pairs and the symmetric taps t[0 .. half],
//   g'_p = g_p - (sum of t[|k|] g_{p+k}) / (sum of t[|k|]),  k = -half .. half in that order, both sums from +0,
// over the pixels p + k that lie in p's segment and are live (b > 0); every operation rounded once (no contraction).
// The arithmetic is ../trx_highpass.h's, shared with the CPU check.
//
//   k_pixel_highpass  one block of kHpBlock lanes per (row, TILE): up to kHpTile consecutive pixels of one segment (the
//                    tile table is made at trx_set_highpass: tiles never cross a segment).  The block stages, for the
//                    tile's pixels and a halo of `half` on either side, g and a 0/1 live flag as doubles into LDS --
//                    coalesced double2 loads of the pairs, g formed once per pixel, (0, 0) for a pixel outside the
//                    segment or dead: (count + 2 half) * 16 bytes, 40 KB at the most.  After the barrier lane l owns
//                    the pixels l, l + kHpBlock of the tile and walks k = -half .. half for both at once: one tap,
//                    wave-uniform and read through scalar loads, and per output one ds_read_b64 of g (and one of the
//                    flag) at consecutive doubles in consecutive lanes -- no bank conflict.  Where a wave finds every
//                    entry of its lanes' windows live (a ballot), den is the host-made full-window constant and the
//                    flags are not read: half the LDS traffic and half the arithmetic, the same bits.
//                    It writes (g', 1) for a live pixel and (+0, +0) for a dead one, coalesced: k_pixel_moments<false>,
//                    k_pixel_filter and k_trail_moments then form 1 * (g' / 1) = g' with gain = nullptr, unchanged.
//
//   k_data_highpass   the same high-pass of the OBSERVED SET's own data (trx_highpass_observed): one block per (exposure,
//                    tile) of the same tile table.  It stages the tile and its halo straight from the data r and the
//                    weights W, both [nexp][npix] doubles -- two coalesced streams of 8 bytes a lane, no intermediate
//                    pair buffer and no second pass over them --: (r, 1) where W > 0 (everywhere without
//                    weights), (+0, +0) for an entry that is dead or outside the segment (highpass_stage_datum).  The
//                    window walk, the ballot and the full-window constant are k_pixel_highpass's, the same
//                    highpass_values; it writes r' for a live entry and +0 for a dead one, one coalesced double a lane.
//
// No atomics, no cross-lane arithmetic, no matrix instruction: the order of each output's sum is the contract, as the
// lane order is for the trail (trx_trail.hip.h).  The bits of a value depend on its row's pairs over its window, the
// gains and the taps -- not on other rows or segments, the tile the pixel fell into, the launch or the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "../trx_highpass.h"

namespace trx {

struct HpArgs {
  const double2 *pairs;     // [nrow][npix] (a, b): d_pixout of this run
  const double *gain;       // [npix], or null: all 1
  const double *taps;       // [half + 1]
  const HpTile *tiles;      // [ntiles]
  double2 *out;             // [nrow][npix]: (g', 1) or (0, 0)
  int64_t npix, ntiles;
  double den_full;          // highpass_full_den of taps
  int32_t half;
};

__global__ __launch_bounds__(kHpBlock) void k_pixel_highpass(HpArgs A)
{
#pragma clang fp contract(off)
  extern __shared__ double hp_lds[];
  const int half = A.half;
  const int64_t row = (int64_t)blockIdx.x / A.ntiles, tile = (int64_t)blockIdx.x - row * A.ntiles;
  const HpTile T = A.tiles[tile];
  const int count = T.count, n = count + 2 * half;      // staged entry i is pixel T.first - half + i
  double *const g = hp_lds, *const m = hp_lds + n;
  const int64_t base = row * A.npix;
  for (int i = (int)threadIdx.x; i < n; i += kHpBlock) {
    const int64_t q = T.first - half + i;
    const bool inside = q >= T.seg_first && q < T.seg_last;
    double2 ab = make_double2(0.0, 0.0); double gn = 1.0;
    if (inside) { ab = A.pairs[base + q]; if (A.gain) gn = A.gain[q]; }
    highpass_stage(ab.x, ab.y, gn, inside, g[i], m[i]);
  }
  __syncthreads();
  // (the wave's number as a value the compiler knows to be the same in all its lanes)
  const int lane = (int)(threadIdx.x & 63), w0 = 64 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w0 >= count) return;                              // (a whole wave, behind the block's only barrier)
  // the wave's windows: for its output pixels [o, min(o + 64, count)) the entries [o, that end + 2 half) -- all live?
  bool ok = true;
  int at[kHpOuts];
#pragma unroll
  for (int j = 0; j < kHpOuts; j++) {
    const int o = w0 + j * kHpBlock;
    at[j] = half + min(o + lane, count - 1);             // (a lane past the tile's end computes its last pixel again and stores nothing)
    const int end = o < count ? min(o + 64, count) + 2 * half : 0;      // (no output of this wave there: nothing to ask)
    for (int i = o + lane; i < end; i += 64) ok = ok && m[i] != 0.0;
  }
  const bool full = __all(ok) != 0;
  double v[kHpOuts];
  highpass_values<kHpOuts>(g, m, at, half, A.taps, full, A.den_full, v);
#pragma unroll
  for (int j = 0; j < kHpOuts; j++) {
    const int p = w0 + j * kHpBlock + lane;
    if (p < count) A.out[base + T.first + p] = m[at[j]] != 0.0 ? make_double2(v[j], 1.0) : make_double2(0.0, 0.0);
  }
}

struct HpDataArgs {
  const double *r;          // [nexp][npix]: the data the high-pass reads -- the residuals, or the raw set
  const double *weight;     // [nexp][npix] as trx_set_observed installed them, or null: all 1
  const double *taps;       // [half + 1]
  const HpTile *tiles;      // [ntiles]: the installed high-pass's
  double *out;              // [nexp][npix]: r', or +0 for a dead entry -- never r itself
  int64_t npix, ntiles;
  double den_full;          // highpass_full_den of taps
  int32_t half;
};

__global__ __launch_bounds__(kHpBlock) void k_data_highpass(HpDataArgs A)
{
#pragma clang fp contract(off)
  extern __shared__ double hp_lds[];
  const int half = A.half;
  const int64_t row = (int64_t)blockIdx.x / A.ntiles, tile = (int64_t)blockIdx.x - row * A.ntiles;
  const HpTile T = A.tiles[tile];
  const int count = T.count, n = count + 2 * half;      // staged entry i is pixel T.first - half + i
  double *const g = hp_lds, *const m = hp_lds + n;
  const int64_t base = row * A.npix;
  for (int i = (int)threadIdx.x; i < n; i += kHpBlock) {
    const int64_t q = T.first - half + i;
    const bool inside = q >= T.seg_first && q < T.seg_last;
    double r = 0.0, w = 1.0;
    if (inside) { r = A.r[base + q]; if (A.weight) w = A.weight[base + q]; }
    highpass_stage_datum(r, w, inside, g[i], m[i]);
  }
  __syncthreads();
  // (the wave's number as a value the compiler knows to be the same in all its lanes)
  const int lane = (int)(threadIdx.x & 63), w0 = 64 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w0 >= count) return;                              // (a whole wave, behind the block's only barrier)
  // the wave's windows, as in k_pixel_highpass: all live?
  bool ok = true;
  int at[kHpOuts];
#pragma unroll
  for (int j = 0; j < kHpOuts; j++) {
    const int o = w0 + j * kHpBlock;
    at[j] = half + min(o + lane, count - 1);             // (a lane past the tile's end computes its last pixel again and stores nothing)
    const int end = o < count ? min(o + 64, count) + 2 * half : 0;      // (no output of this wave there: nothing to ask)
    for (int i = o + lane; i < end; i += 64) ok = ok && m[i] != 0.0;
  }
  const bool full = __all(ok) != 0;
  double v[kHpOuts];
  highpass_values<kHpOuts>(g, m, at, half, A.taps, full, A.den_full, v);
#pragma unroll
  for (int j = 0; j < kHpOuts; j++) {
    const int p = w0 + j * kHpBlock + lane;
    if (p < count) A.out[base + T.first + p] = m[at[j]] != 0.0 ? v[j] : 0.0;
  }
}

}  // namespace trx
