// trx_pca.hip.h -- the principal-component detrend of the observed exposures on the device (trx_pca_observed,
// include/transit_hip.h): per segment the Gram matrix of the whole columns, its eigenvectors by a fixed number of Jacobi
// sweeps in a fixed parallel order, and the components' coefficients and residuals on every column.  The arithmetic, the
// schedule and the rank and sign rules are ../trx_pca.h's, the same source a CPU program runs.
//
// The residuals r [nexp][npix] start as the raw data (or the injected data, k_sysrem_inject) in a buffer of their own:
//
//   k_pca_live      k_sysrem_rows' structure: one wavefront per row (v, s), kMomWaves rows per block; the lanes look at the
//                   segment's weights 64 at a time and leave at the first trip that finds one > 0.  live [nseg][nexp].
//   k_pca_whole     one lane per pixel column, one wavefront per tile of the tile table, kFiltWaves tiles per block
//                   (tile_column); the lane's column is pca_whole_column of ../trx_pca.h: v ascends over the live exposures.
//                   whole [npix].
//   k_pca_gram      one wavefront per tile of kPcaGramTile x kPcaGramTile entries (v, u) of a segment's G, bv <= bu,
//                   kPcaGramWaves tiles per block.  Lane l carries the 16 accumulators at its own pixels first + l, first +
//                   l + 64, ..., 8 loads a step in place of 32, then one wave_sum butterfly per entry; lane 0 stores
//                   G[v][u] and G[u][v] for u >= v.  An empty segment's G is +0.
//   k_pca_jacobi    one block of kPcaBlock threads per segment.  A sits in LDS with an odd row stride (a column's entries
//                   fall on different banks), beside the round's pairs and (c, s), the eigenvalues and the rows' maxima;
//                   V sits transposed in global scratch (Vt[j][i] = V[i][j]: the column phase reads and writes along i).
//                   A round is: the parameters (thread k: pair k), barrier, the column phase over (pair, row) items of A
//                   and Vt, barrier, the row phase over (pair, column) items of A, barrier -- nsweep * (m - 1) rounds,
//                   no convergence test.  Then the eigenvalues, offdiag, the ranks by counting, the sign, U and eigen;
//                   the block also counts its segment's whole columns.
//   k_pca_project   k_sysrem_subtract's tiling: one lane per pixel column, pca_project_column of ../trx_pca.h; the
//                   coefficients of all components in registers (v ascending), then the residuals in place (i ascending
//                   per entry).
//
// No atomics; cross-lane work goes through wave_sum, wave_sum_ll and the block's barriers only.  The bits of a segment's
// result depend on that segment's data and weights, ncomp and nsweep -- not on other segments, the launch or the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "transit_hip.h"
#include "trx_device.h"
#include "trx_kernels.hip.h"
#include "trx_filter.hip.h"
#include "trx_moments.hip.h"
#include "trx_sysrem.hip.h"
#include "../trx_pca.h"

namespace trx {

struct PcaArgs {
  double *r;                // [nexp][npix] f0, then the residuals
  const double *weight;     // [nexp][npix], or null: all 1
  const FilterTile *tiles;  // [ntiles]
  const int64_t *seg_first; // [nseg + 1]
  int32_t *live;            // [nseg][nexp]
  int32_t *whole;           // [npix]
  double *G;                // [nseg][nexp][nexp]
  double *Vt;               // [nseg][nexp][nexp], Vt[j][i] = V[i][j]
  double *coef;             // [ncomp][npix]
  double *basis;            // U [nseg][nexp][ncomp]
  double *eigen;            // [nseg][ncomp]
  double *offdiag;          // [nseg]
  int64_t *nwhole;          // [nseg]
  int64_t npix, ntiles, nrows, gram_tiles;      // nrows = nexp * nseg; gram_tiles = nseg * pca_gram_tiles(nexp)
  int32_t nexp, nseg, ncomp, nsweep, stride;    // stride: A's row stride in LDS
};

__global__ __launch_bounds__(64 * kMomWaves) void k_pca_live(PcaArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t row = (int64_t)blockIdx.x * kMomWaves + (threadIdx.x >> 6);
  if (row >= A.nrows) return;
  const int64_t v = row / A.nseg, s = row - v * A.nseg;
  const int64_t first = A.seg_first[s], last = A.seg_first[s + 1];
  bool any = false;
  if (!A.weight) any = last > first;
  else
    for (int64_t p0 = first; p0 < last && !any; p0 += 64) {
      const int64_t q = p0 + lane;
      any = __any(q < last && A.weight[v * A.npix + q] > 0.0) != 0;
    }
  if (lane == 0) A.live[s * A.nexp + v] = any ? 1 : 0;
}

__global__ __launch_bounds__(64 * kFiltWaves) void k_pca_whole(PcaArgs A)
{
  tile_column<kFiltWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) {
    const bool hasw = A.weight != nullptr;
    A.whole[p] = pca_whole_column(A.live + (int64_t)T.seg * A.nexp, hasw ? A.weight + p : nullptr, hasw, A.npix, A.nexp) ? 1 : 0;
  });
}

__global__ __launch_bounds__(64 * kPcaGramWaves) void k_pca_gram(PcaArgs A)
{
#pragma clang fp contract(off)
  constexpr int T = kPcaGramTile;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t tile = (int64_t)blockIdx.x * kPcaGramWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= A.gram_tiles) return;                    // (a whole wave: the butterflies below have all their lanes)
  const int nexp = A.nexp, nb = pca_gram_blocks(nexp), per = pca_gram_tiles(nexp);
  const int64_t s = tile / per;
  int bv, bu;
  pca_gram_tile(nb, (int)(tile - s * per), bv, bu);
  const int64_t first = A.seg_first[s], last = A.seg_first[s + 1];
  const int32_t *const live = A.live + s * nexp;
  // (a row past the last exposure reads the last one again; its entries are not stored)
  int64_t rv[T], ru[T]; bool lv[T], lu[T];
#pragma unroll
  for (int a = 0; a < T; a++) {
    const int v = min(bv * T + a, nexp - 1), u = min(bu * T + a, nexp - 1);
    rv[a] = (int64_t)v * A.npix; ru[a] = (int64_t)u * A.npix;
    lv[a] = live[v] != 0; lu[a] = live[u] != 0;
  }
  double acc[T][T];
#pragma unroll
  for (int a = 0; a < T; a++)
#pragma unroll
    for (int b = 0; b < T; b++) acc[a][b] = 0.0;
  for (int64_t p = first + lane; p < last; p += 64) {
    const bool whole = A.whole[p] != 0;
    double xv[T], xu[T];
#pragma unroll
    for (int a = 0; a < T; a++) { xv[a] = A.r[rv[a] + p]; xu[a] = A.r[ru[a] + p]; }
#pragma unroll
    for (int a = 0; a < T; a++) { xv[a] = whole && lv[a] ? xv[a] : 0.0; xu[a] = whole && lu[a] ? xu[a] : 0.0; }
#pragma unroll
    for (int a = 0; a < T; a++)
#pragma unroll
      for (int b = 0; b < T; b++) { const double m = xv[a] * xu[b]; acc[a][b] = acc[a][b] + m; }
  }
  double *const G = A.G + s * nexp * nexp;
#pragma unroll
  for (int a = 0; a < T; a++)
#pragma unroll
    for (int b = 0; b < T; b++) {
      const double g = wave_sum(acc[a][b]);
      const int v = bv * T + a, u = bu * T + b;
      if (lane == 0 && u >= v && u < nexp) { G[(int64_t)v * nexp + u] = g; G[(int64_t)u * nexp + v] = g; }
    }
}

__global__ __launch_bounds__(kPcaBlock) void k_pca_jacobi(PcaArgs A)
{
  extern __shared__ double pca_lds[];
  const int tid = (int)threadIdx.x, nexp = A.nexp, stride = A.stride, npairs = pca_pairs(nexp), nrounds = pca_rounds(nexp);
  const int64_t s = blockIdx.x;
  double *const M = pca_lds;                           // A [nexp][stride]
  double *const cs = M + (size_t)nexp * stride;        // (c, s) [npairs][2]; c = 0: the pair is dropped or skipped
  double *const lam = cs + 2 * npairs;                 // [nexp]
  double *const rowmax = lam + nexp;                   // [nexp]
  long long *const counts = (long long *)(rowmax + nexp);      // [kPcaBlock / 64]
  int *const pq = (int *)(counts + kPcaBlock / 64);    // (p, q) [npairs][2]
  const double *const G = A.G + s * nexp * nexp;
  double *const Vt = A.Vt + s * nexp * nexp;
  const int cells = nexp * nexp;
  for (int w = tid; w < cells; w += kPcaBlock) {
    const int i = w / nexp, j = w - i * nexp;
    M[i * stride + j] = G[w];
    Vt[w] = i == j ? 1.0 : 0.0;
  }
  // the segment's whole columns, counted (integers: any order)
  {
    long long n = 0;
    for (int64_t p = A.seg_first[s] + tid; p < A.seg_first[s + 1]; p += kPcaBlock) n += A.whole[p] != 0;
    n = wave_sum_ll(n);
    if ((tid & 63) == 0) counts[tid >> 6] = n;
  }
  __syncthreads();
  if (tid == 0) {
    long long n = 0;
    for (int k = 0; k < kPcaBlock / 64; k++) n += counts[k];
    A.nwhole[s] = n;
  }
  const int items = npairs * nexp;
  for (int sweep = 0; sweep < A.nsweep; sweep++)
    for (int t = 0; t < nrounds; t++) {
      if (tid < npairs) {
        int p, q; double c = 0.0, sn = 0.0;
        if (pca_pair(nexp, t, tid, p, q)) { if (!pca_rotation(M[p * stride + p], M[q * stride + q], M[p * stride + q], c, sn)) c = 0.0; }
        else p = q = 0;
        pq[2 * tid] = p; pq[2 * tid + 1] = q; cs[2 * tid] = c; cs[2 * tid + 1] = sn;
      }
      __syncthreads();
      // the column phase: item (pair k, row i) of A and of V
      for (int w = tid; w < items; w += kPcaBlock) {
        const int k = w / nexp, i = w - k * nexp;
        const double c = cs[2 * k], sn = cs[2 * k + 1];
        if (c == 0.0) continue;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        double x = M[i * stride + p], y = M[i * stride + q];
        pca_rotate(x, y, c, sn);
        M[i * stride + p] = x; M[i * stride + q] = y;
        double vx = Vt[p * nexp + i], vy = Vt[q * nexp + i];
        pca_rotate(vx, vy, c, sn);
        Vt[p * nexp + i] = vx; Vt[q * nexp + i] = vy;
      }
      __syncthreads();
      // the row phase: item (pair k, column j) of A; then A[p][q] = A[q][p] = +0
      for (int w = tid; w < items; w += kPcaBlock) {
        const int k = w / nexp, j = w - k * nexp;
        const double c = cs[2 * k], sn = cs[2 * k + 1];
        if (c == 0.0) continue;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        double x = M[p * stride + j], y = M[q * stride + j];
        pca_rotate(x, y, c, sn);
        M[p * stride + j] = j == q ? 0.0 : x; M[q * stride + j] = j == p ? 0.0 : y;
      }
      __syncthreads();
    }
  if (tid < nexp) {
    lam[tid] = M[tid * stride + tid];
    double mx = 0.0;
    for (int q = tid + 1; q < nexp; q++) mx = pca_absmax(mx, M[tid * stride + q]);
    rowmax[tid] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    double mx = 0.0;
    for (int i = 0; i < nexp; i++) mx = pca_absmax(mx, rowmax[i]);
    A.offdiag[s] = mx;
  }
  if (tid < nexp) {
    const double mine = lam[tid];
    int rank = 0;
    for (int k = 0; k < nexp; k++) rank += pca_ahead(lam[k], k, mine, tid) ? 1 : 0;
    if (rank < A.ncomp) {
      const double *const col = Vt + tid * nexp;
      const bool valid = pca_valid(mine);
      const bool neg = valid && col[pca_largest(col, nexp, 1)] < 0.0;
      double *const U = A.basis + s * nexp * A.ncomp + rank;
      for (int v = 0; v < nexp; v++) U[(int64_t)v * A.ncomp] = !valid ? 0.0 : neg ? pca_flip(col[v]) : col[v];
      A.eigen[s * A.ncomp + rank] = valid ? mine : 0.0;
    }
  }
}

__global__ __launch_bounds__(64 * kFiltWaves) void k_pca_project(PcaArgs A)
{
  tile_column<kFiltWaves>(A.tiles, A.ntiles, [&](const FilterTile &T, int64_t p) {
    const bool hasw = A.weight != nullptr;
    pca_project_column(A.r + p, hasw ? A.weight + p : nullptr, hasw, A.basis + (int64_t)T.seg * A.nexp * A.ncomp, A.coef + p, A.npix, A.nexp, A.ncomp);
  });
}

}  // namespace trx
