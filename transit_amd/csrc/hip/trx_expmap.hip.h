// trx_expmap.hip.h -- the Kp-Vsys detection map under the exposure table (trx_run_exposed_map, include/transit_hip.h).
//
// trx_run_filtered_map's pixel rows are lags, and a lag has no exposure: the table (scale[v], smear[v]) cannot act on them.
// Here a pixel row is a PAIR (lag l, exposure v): k_cell_tracks (trx_cellmap.hip.h) runs ahead of the pixel pass, the two
// kernels below find which pairs the cells of the call need -- per exposure the span of lags lo_v .. hi_v its inside cells
// take, the spans end to end (../trx_expmap.h) -- and ONE launch of k_pixel_pairs_exposed makes those R rows, each with its
// own shift lag[l], smear[v] and scale[v].  The cell kernels of trx_cellmap.hip.h and trx_wfilter.hip.h then run unchanged:
// they reach their rows through an index table, and get the row table where the filtered map hands them the lag table.
//
//   k_cell_spans   one wavefront per exposure v.  Lane l looks at the cells l, l + 64, ...: a cell with a -1 anywhere in its
//                  index row is OUTSIDE and skipped whole; of the others the lane keeps the least and the largest index[c][v]
//                  (span_take), and a butterfly of integer min and max gives the wave's.  Lane 0 stores span[v] = (lo_v, hi_v),
//                  (kSpanEmptyLo, kSpanEmptyHi) where no cell is inside.  Integer min / max: no order dependence.
//   k_cell_rows    one lane per (cell, exposure): row[c][v] = base_v + (index[c][v] - lo_v), or -1 (exposed_map_row).  The
//                  lag table keeps the lags: it is what the caller gets back.
//
// No atomics, no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "trx_device.h"
#include "../trx_expmap.h"

namespace trx {

struct CellSpanArgs {
  const int32_t *index;     // [ncells][nexp]: the nearest lag, or -1 (k_cell_tracks)
  int32_t *span;            // [nexp][2]: (lo_v, hi_v)
  int64_t ncells;
  int32_t nexp;
};

struct CellRowArgs {
  const int32_t *index;     // [ncells][nexp]
  const int32_t *span;      // [nexp][2]
  const int64_t *base;      // [nexp]: the first row of exposure v
  int32_t *row;             // [ncells][nexp]: the pixel row of (index[c][v], v), or -1
  int64_t ntracks;          // ncells * nexp
  int32_t nexp;
};

__global__ __launch_bounds__(64 * kCellSpanWaves) void k_cell_spans(CellSpanArgs A)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t v = (int64_t)blockIdx.x * kCellSpanWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (v >= A.nexp) return;                             // (a whole wave: the butterfly below has all its lanes)
  int32_t lo = kSpanEmptyLo, hi = kSpanEmptyHi;
  for (int64_t c = lane; c < A.ncells; c += 64) {
    const int32_t *const idx = A.index + c * A.nexp;
    if (index_row_outside(idx, A.nexp)) continue;
    span_take(lo, hi, idx[v]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) { A.span[2 * v] = lo; A.span[2 * v + 1] = hi; }
}

__global__ __launch_bounds__(kCellTrackBlock) void k_cell_rows(CellRowArgs A)
{
  const int64_t k = (int64_t)blockIdx.x * kCellTrackBlock + threadIdx.x;
  if (k >= A.ntracks) return;
  const int64_t v = k % A.nexp;
  A.row[k] = exposed_map_row(A.index[k], A.span[2 * v], A.span[2 * v + 1], A.base[v]);
}

}  // namespace trx
