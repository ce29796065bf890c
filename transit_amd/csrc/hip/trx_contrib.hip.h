// trx_contrib.hip.h -- contribution functions per band and layer on the device (trx_run_contrib, include/transit_hip.h).
//
// Where in the atmosphere a channel comes from: for every band b of the installed set and every layer r, the
// band-weighted sum over the band's bins of
//   eclipse geometry   F_i = B_i W_i, the reference's flux quadrature (eclipse.c:118-160, 243-287) regrouped by node:
//                      g_i = pi sum_a area_a exp(-tau_i / cos a), d_i = g_i - g_{i+1},
//                      W_0 = d_0 / 2, W_i = (d_{i-1} + d_i) / 2, W_last = d_{last-1} / 2 + g_last  (last = 0: W_0 = g_0)
//   transit geometry   T_i = exp(-tau_i)  (what modulation1 integrates, slantpath.c:374-386)
// for i <= last, zero below; i counts heights from the top, layer r = nlayer - 1 - i.  The optical depths are the
// run's own (d_tau [height][nsh], d_last); entries below a ray's `last` are not defined and never read.
//
//   k_contrib_pieces  one block per (quarter of a piece, 16 heights): a piece of the band set (kBandPiece = 1024
//                     consecutive in-shard bins of one band, trx_bands.hip.h) is four sub-pieces of 256 bins, wave k of
//                     a block takes bins 64 k .. 64 k + 63 of its sub-piece, one bin per lane.  A node needs its two
//                     neighbours only, so the heights are cut into slices of 16 that different blocks take: a lane
//                     reads its 18 optical depths (a height's row segment of tau is one coalesced 512-byte read per
//                     wave), makes their g side by side, and closes its 16 nodes.  Per height the wave adds its lanes
//                     with wave_sum's fixed butterfly; the four wave sums are staged in LDS and added in wave order,
//                     lanes = heights.  Rays end at different `last`: the per-lane conditions are selects, and a block
//                     below the deepest `last` of its bins stores zeros.  (One block per whole piece walking all
//                     heights was measured first: 183 us at the demo shape, 1024 bins x 80 heights of exponentials on
//                     ONE compute unit.)
//   k_contrib_sums    one wave per (band, layer): lane l adds the band's sub-pieces l, l + 64, ... in ascending order,
//                     then wave_sum; lane 0 stores the entry into the pinned block the host reads.
//
// No atomics on a sum: every sum has one order, fixed by the band and the shard alone -- not by the launch, the other
// bands of the set, the handle or batch way that ran it, the depth hint or the kernels that made tau.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_kernels.hip.h"
#include "trx_bands.hip.h"

namespace trx {

constexpr int kContribHeights = 16;                               // heights per block (kContribWaves, kContribSplit: trx_device.h)

struct ContribArgs {
  EmisArgs E;               // eclipse: angles, area weights, temperatures, e2tab; both: nr, nsh, lo, grid, tau, last
  const BandDev *bands;     // [nbands]
  const BandPiece *pieces;  // [npieces]
  const double *w;          // WEIGHTS bands' in-shard weights, concatenated
  double *part;             // [npieces * kContribSplit][nr] sub-piece rows, atmosphere's layer order (device)
  double *out;              // [nbands][nr] pinned host memory, as the device sees it
  int64_t npieces;
  int32_t nbands, vertical;
};

// g = pi sum_a area_a exp(-tau / cos a), the angles in order (flux(), eclipse.c:271-285)
template <int NANG>
__device__ __forceinline__ double contrib_g(const EmisArgs &E, double tv, const double *s_e2)
{
  double g = 0.0;
#pragma unroll
  for (int a = 0; a < NANG; a++)
    if (a < E.nang) g += E.area[a] * exp_neg(slant_depth(E, a, tv), s_e2);       // (wave-uniform)
  return kPi * g;
}

// NANG: the angles the kernel holds constants for (8 or kMaxAngles, like k_ray_tail: 16 angles' cosines, reciprocals and
// areas are 96 scalar registers)
template <int NANG>
__global__ __launch_bounds__(64 * kContribWaves) void k_contrib_pieces(ContribArgs A)
{
  constexpr int KH = kContribHeights;
  __shared__ double s_e2[64];
  __shared__ double s_row[kContribWaves][KH + 1];       // (odd row stride)
  __shared__ double s_tk[KH];                           // the slice's temperatures
  __shared__ int s_deep;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t sub = blockIdx.x, p = sub / kContribSplit;
  const int q = (int)(sub % kContribSplit);
  const int nr = A.E.nr, i0 = (int)blockIdx.y * KH;     // the block's nodes: heights i0 .. i0 + KH - 1
  if (p >= A.npieces || i0 >= nr) return;               // (block-uniform)
  const BandPiece P = A.pieces[p];
  double *prow = A.part + sub * nr;
  const int first = q * 64 * kContribWaves;             // the sub-piece's first bin in the piece
  if (first >= P.len) {                                 // (block-uniform) no bin: rows of zeros
    if (tid < KH && i0 + tid < nr) prow[nr - 1 - (i0 + tid)] = 0.0;
    return;
  }
  if (tid < 64) s_e2[tid] = A.E.e2tab[tid];
  if (tid >= 64 && tid < 64 + KH) s_tk[tid - 64] = A.E.temp[max(nr - 1 - (i0 + tid - 64), 0)];      // (past the bottom: not used)
  if (tid == 0) s_deep = -1;
  __syncthreads();
  const BandDev B = A.bands[P.band];
  const int64_t nsh = A.E.nsh;
  const int t = first + wave * 64 + lane;
  const bool mine = t < P.len;
  const bool wave_has = first + wave * 64 < P.len;      // (wave-uniform: a wave past the piece's end stages zeros)
  const int64_t j = P.start + (mine ? t : 0);
  // the band's weight of this bin, as k_band_pieces makes it
  double wj = 0.0;
  int last = -1;                                        // (< 0: no bin, or a ray still descending -- nothing yet)
  if (mine) {
    if (B.kind == TRX_BAND_GAUSS) {
      const double nu = A.E.wn_i + (double)(A.E.lo + j) * A.E.wn_d;
      const double x = (nu - B.centre) / B.sigma;
      wj = exp(-0.5 * (x * x));
    } else wj = A.w[B.woff + (j - B.s)];
    last = A.E.last[j];
    if (last > nr - 1) last = nr - 1;
  }
  atomicMax(&s_deep, last);                             // (a maximum: no order to depend on)
  __syncthreads();
  const int n = min(KH, s_deep + 1 - i0);               // block-uniform: nodes i0 .. i0 + n - 1 can be non-zero (n <= 0: none)
  const double *tw = A.E.tau + j;                       // tw[i * nsh] = tau[i][j]
  double out[KH];
#pragma unroll
  for (int c = 0; c < KH; c++) out[c] = 0.0;

  if (wave_has && n > 0) {
    if (!A.vertical) {
      double tv[KH];
#pragma unroll
      for (int c = 0; c < KH; c++) {
        const int i = i0 + c;
        tv[c] = 0.0;
        if (i <= last) tv[c] = tw[(int64_t)i * nsh];
      }
#pragma unroll
      for (int c = 0; c < KH; c++)
        if (c < n) {                                    // (block-uniform)
          const double v = wj * exp(-tv[c]);
          out[c] = wave_sum(i0 + c <= last ? v : 0.0);
        }
    } else {
      // g at heights i0 - 1 .. i0 + KH: entry u is height i0 - 1 + u; zero outside [0, last]
      double gv[KH + 2];
#pragma unroll
      for (int u = 0; u < KH + 2; u++) {
        const int i = i0 - 1 + u;
        gv[u] = 0.0;
        if (i >= 0 && i <= last) gv[u] = tw[(int64_t)i * nsh];       // (the optical depth, for now)
      }
#pragma unroll
      for (int u = 0; u < KH + 2; u++)
        if (u < n + 2) {                                // (block-uniform)
          const int i = i0 - 1 + u;
          const double g = contrib_g<NANG>(A.E, gv[u], s_e2);
          gv[u] = (i >= 0 && i <= last) ? g : 0.0;
        }
      const double wv = (A.E.wn_i + (double)(A.E.lo + j) * A.E.wn_d) * A.E.wn_fct;
      const double pl_num = planck_num(wv), pl_ex = kH * wv * kLs;      // RayPlanck's
#pragma unroll
      for (int c = 0; c < KH; c++)
        if (c < n) {                                    // (block-uniform)
          const int m = i0 + c;                         // the node: d_{m-1} = g_{m-1} - g_m (d_{-1} = 0), d_m = g_m - g_{m+1}
          const double d_b = m >= 1 ? gv[c] - gv[c + 1] : 0.0, d_m = gv[c + 1] - gv[c + 2];
          const double W = m < last ? 0.5 * (d_b + d_m) : m == last ? 0.5 * d_b + gv[c + 1] : 0.0;
          const double Bm = planck_from(pl_num, pl_ex / (kKb * s_tk[c]), s_e2);
          out[c] = wave_sum(wj * (Bm * W));
        }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < KH; c++) s_row[wave][c] = out[c];
  }
  __syncthreads();
  if (tid < KH && i0 + tid < nr) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kContribWaves; k++) s += s_row[k][tid];
    prow[nr - 1 - (i0 + tid)] = s;
  }
}

// one wave per (band, layer): lane l adds the band's sub-pieces l, l + 64, ... in ascending order, then wave_sum
// (k_band_sums' order)
__global__ __launch_bounds__(64 * kBandWaves) void k_contrib_sums(ContribArgs A)
{
  const int nr = A.E.nr;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t idx = (int64_t)blockIdx.x * kBandWaves + (threadIdx.x >> 6);
  if (idx >= (int64_t)A.nbands * nr) return;            // (wave-uniform)
  const int b = (int)(idx / nr), r = (int)(idx % nr);
  const BandDev B = A.bands[b];
  const int64_t s0 = B.piece0 * kContribSplit, ns = B.npieces * kContribSplit;
  double s = 0.0;
  for (int64_t q = lane; q < ns; q += 64) s += A.part[(s0 + q) * nr + r];
  s = wave_sum(s);
  if (lane == 0) A.out[idx] = s;
}

}  // namespace trx
