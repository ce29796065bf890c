// trx_trail.hip.h -- the cross-correlation trail on the device: the moments of EVERY exposure of the observed set against
// the model at EVERY lag of a velocity grid (trx_run_trail, include/transit_hip.h).
//
// k_pixel_pairs (trx_pixels.hip.h) leaves out[l][p] = (a, b) in device memory, the model at lag l's shift at pixel p.  A
// trail row (l, v, s) is the row k_pixel_moments (trx_moments.hip.h) makes for exposure v and segment s when that
// exposure's shift is lag l: the same contributing rule (b > 0 and w > 0), the same terms w, w*g, (w*g)*g, w*f, (w*f)*g,
// (w*f)*f with g = gain_p * (a / b), every operation rounded once (no contraction), and the same order of the sum --
// lane k adds the segment's pixels first + k, first + k + 64, ... in that order, then wave_sum's fixed butterfly.  The
// row has that kernel's bits.
//
//   k_trail_moments<TL, TV>  one wavefront per (segment, tile of TL lags x TV exposures): the parallel axis is
//                    nseg * ceil(nlag / TL) * ceil(nexp / TV) waves, kTrailWaves per block, the exposure tiles of one
//                    (segment, lag tile) on consecutive waves (they read the same pairs), the last block ragged; the
//                    blocks of one XCD work through the segments one after the other (xcd_block, trx_walk.hip.h).
//                    Per trip of 64 pixels a wave
//                      - loads the TL pairs and the gain once and forms g and the live flag once per (lag, pixel);
//                      - loads the TV (f, w) once and forms w*f and (w*f)*f once per (exposure, pixel);
//                      - updates TL x TV x 7 register accumulators: nine fp64 operations and an integer one per (lag,
//                        exposure, pixel) -- the count is kept as an integer per lane and turned into a double for its
//                        butterfly, which is exact either way.
//                    The loads of the next trip are issued before the sums of this one.  A ragged tile (nlag or nexp
//                    no multiple of the tile) clamps its indices to the last lag / exposure and discards the surplus
//                    rows at the end; no lane leaves before the butterflies, which run once, at the end, 7 per row.
//
//                    How a pixel that does not contribute adds nothing: a lane past the segment's end, or a pixel with
//                    w = 0, takes w = +0 -- then every term is a zero, and an accumulator that started at +0 is never
//                    -0, so adding a zero of either sign leaves its bits as they are.  That needs a finite g.  A lag
//                    at which any pixel of the trip has b <= 0 or a g that is not finite (wave-uniform test) takes the
//                    literal form instead: the terms under the contributing condition, as k_pixel_moments has them.
//                    (One mask per lag in place of the test, which would serve trips with and without such pixels
//                    alike, was measured: 12 % slower where every pixel is on the grid -- the accumulators are copied
//                    around the masked region --, and no faster where 88 % are off it.)
//
// No atomics: the bits of a row depend on the pairs of that lag, on that exposure's data and weights over that segment's
// pixels and on their gains -- not on the other lags or exposures of the call, the tile the row fell into, the launch,
// the handle that ran it or the run's step plan.
//
// No MFMA: the sums are a [lags x pixels] x [pixels x exposures] product and v_mfma_f64_16x16x4_f64 would take it, but
// it adds the pixels of a row in ITS order, four at a time down the k axis, and not in the lane-strided order plus
// butterfly that k_pixel_moments uses -- the row would be a correctly rounded-per-step sum of the same terms with other
// bits, and the contract is the bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"
#include "trx_walk.hip.h"

namespace trx {

constexpr int kTrailWaves = 4;                        // tiles (waves) per block
constexpr int kTrailLags = 2, kTrailExps = 4;         // the tile trx_run_trail launches (docs/history.md: the others measured)

struct TrailArgs {
  const double2 *pairs;     // [nlag][npix] (a, b): d_pixout of this run
  const double *data;       // [nexp][npix]
  const double *weight;     // [nexp][npix], or null: all 1
  const double *gain;       // [npix], or null: all 1
  const int64_t *seg_first; // [nseg + 1]
  double *trail;            // [nlag][nexp][nseg][TRX_NMOMENT] (device)
  int64_t npix, nwaves;     // nwaves = nseg * ntl * ntv
  int32_t nlag, nexp, nseg;
  int32_t ntl, ntv;         // ceil(nlag / TL), ceil(nexp / TV)
  int32_t xcd_map;          // blocks -> tiles by xcd_block (0: in launch order; measurements)
};

// what a wave loads per trip: the pairs of its lags, the gain, (f, w) of its exposures -- at its lane's pixel
template <int TL, int TV>
struct TrailTrip { double2 ab[TL]; double gn; double f[TV], w[TV]; };

template <int TL, int TV>
__device__ __forceinline__ void trail_load(const TrailArgs &A, const int64_t (&lrow)[TL], const int64_t (&vrow)[TV], int64_t p, TrailTrip<TL, TV> &T)
{
#pragma unroll
  for (int i = 0; i < TL; i++) T.ab[i] = A.pairs[lrow[i] + p];
  T.gn = A.gain ? A.gain[p] : 1.0;
#pragma unroll
  for (int j = 0; j < TV; j++) {
    T.f[j] = A.data[vrow[j] + p];
    T.w[j] = A.weight ? A.weight[vrow[j] + p] : 1.0;
  }
}

template <int TL, int TV>
__global__ __launch_bounds__(64 * kTrailWaves) void k_trail_moments(TrailArgs A)
{
#pragma clang fp contract(off)
  const int lane = (int)(threadIdx.x & 63);
  // (blocks go to the XCDs in turn: with xcd_block an XCD takes one contiguous eighth of the tiles in order, so that its L2
  // holds ONE segment's data and weights at a time, read again by every lag tile, and not an eighth of every block's)
  const int64_t blk = A.xcd_map ? xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const int64_t tile = blk * kTrailWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= A.nwaves) return;                        // (a whole wave: the butterflies below have all their lanes)
  const int64_t tv = tile % A.ntv, rest = tile / A.ntv, tl = rest % A.ntl, s = rest / A.ntl;
  const int64_t first = A.seg_first[s], last = A.seg_first[s + 1];
  const int64_t l0 = tl * TL, v0 = tv * TV;
  // (a ragged tile: the surplus lags and exposures are the last one again, dropped at the stores)
  int64_t lrow[TL], vrow[TV];
#pragma unroll
  for (int i = 0; i < TL; i++) lrow[i] = (l0 + i < A.nlag ? l0 + i : (int64_t)A.nlag - 1) * A.npix;
#pragma unroll
  for (int j = 0; j < TV; j++) vrow[j] = (v0 + j < A.nexp ? v0 + j : (int64_t)A.nexp - 1) * A.npix;

  int n[TL][TV];
  double sw[TL][TV], swg[TL][TV], swgg[TL][TV], swf[TL][TV], swfg[TL][TV], swff[TL][TV];
#pragma unroll
  for (int i = 0; i < TL; i++)
#pragma unroll
    for (int j = 0; j < TV; j++) { n[i][j] = 0; sw[i][j] = swg[i][j] = swgg[i][j] = swf[i][j] = swfg[i][j] = swff[i][j] = 0.0; }

  if (first < last) {
    // (a lane past the segment's end reads the segment's last pixel again and adds nothing)
    TrailTrip<TL, TV> next;
    { const int64_t q = first + lane; trail_load<TL, TV>(A, lrow, vrow, q < last ? q : last - 1, next); }
    for (int64_t p0 = first; p0 < last; p0 += 64) {
      const TrailTrip<TL, TV> T = next;
      if (p0 + 64 < last) { const int64_t q = p0 + 64 + lane; trail_load<TL, TV>(A, lrow, vrow, q < last ? q : last - 1, next); }
      const bool in = p0 + lane < last;
      // once per (exposure, pixel)
      double we[TV], wf[TV], wff[TV]; int c[TV];
#pragma unroll
      for (int j = 0; j < TV; j++) {
        const bool on = in && T.w[j] > 0.0;
        c[j] = on ? 1 : 0;
        we[j] = on ? T.w[j] : 0.0;
        wf[j] = we[j] * T.f[j];
        wff[j] = wf[j] * T.f[j];
      }
#pragma unroll
      for (int i = 0; i < TL; i++) {
        // once per (lag, pixel)
        const bool live = in && T.ab[i].y > 0.0;
        const double g = T.gn * (T.ab[i].x / T.ab[i].y);
        if (__ballot(in && !(live && __builtin_isfinite(g))) == 0) {
          const double g0 = in ? g : 0.0;              // (here every term of a pixel with w = +0 is a zero)
#pragma unroll
          for (int j = 0; j < TV; j++) {
            const double wg = we[j] * g0;
            n[i][j] += c[j]; sw[i][j] += we[j]; swg[i][j] += wg; swgg[i][j] += wg * g0;
            swf[i][j] += wf[j]; swfg[i][j] += wf[j] * g0; swff[i][j] += wff[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < TV; j++)
            if (live && c[j]) {
              const double wg = we[j] * g;
              n[i][j] += 1; sw[i][j] += we[j]; swg[i][j] += wg; swgg[i][j] += wg * g;
              swf[i][j] += wf[j]; swfg[i][j] += wf[j] * g; swff[i][j] += wff[j];
            }
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < TL; i++)
#pragma unroll
    for (int j = 0; j < TV; j++) {
      const double m0 = wave_sum((double)n[i][j]), m1 = wave_sum(sw[i][j]), m2 = wave_sum(swg[i][j]), m3 = wave_sum(swgg[i][j]);
      const double m4 = wave_sum(swf[i][j]), m5 = wave_sum(swfg[i][j]), m6 = wave_sum(swff[i][j]);
      // (every lane holds the seven sums: lanes 0 .. 6 store one each)
      const double r = lane == 0 ? m0 : lane == 1 ? m1 : lane == 2 ? m2 : lane == 3 ? m3 : lane == 4 ? m4 : lane == 5 ? m5 : m6;
      if (l0 + i < A.nlag && v0 + j < A.nexp && lane < TRX_NMOMENT)
        A.trail[(((l0 + i) * A.nexp + (v0 + j)) * A.nseg + s) * TRX_NMOMENT + lane] = r;
    }
}

}  // namespace trx
