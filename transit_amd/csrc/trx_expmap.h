// trx_expmap.h -- the host side of the Kp-Vsys map under the exposure table (trx_run_exposed_map, include/transit_hip.h):
// what the call refuses, the row spans of the exposures and their bases, the per-row arrays the exposed pixel kernel takes,
// the index -> row transform and the extents of the run's buffers.  Plain C++ (no HIP): k_cell_spans and k_cell_rows
// (hip/trx_expmap.hip.h) call span_take, span_count and exposed_map_row per lane, trx_api.hip checks, lays out and sizes
// with the rest, and tests/expmap_check.cpp runs the same source on the CPU over exact-size buffers.
//
// The map's pixel rows are (lag, exposure) pairs: exposure v needs the lags lo_v .. hi_v that the cells inside the lag grid
// take at v, n_v = hi_v - lo_v + 1 of them (0 where no cell is inside), and they lie end to end from base_v = n_0 + ... +
// n_{v-1}: row r = base_v + (l - lo_v) is lag l at exposure v, R = the sum of the n_v rows in all.  The spans are dense -- no
// compaction -- and come from integer min / max alone, so they do not depend on the order the cells are looked at in.  The
// track rule is vmap_track and vmap_nearest of trx_vmap.h; there is no second one here.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "transit_hip.h"
#include "hip/trx_device.h"
#include "trx_exposures.h"
#include "trx_numerics.h"
#include "trx_products.h"
#include "trx_vmap.h"

namespace trx {

// the span of an exposure no inside cell has touched: span_take's start, n_v = 0
constexpr int32_t kSpanEmptyLo = 0x7fffffff, kSpanEmptyHi = -1;

// one inside cell's lag k at an exposure, taken into that exposure's span
TRX_HD void span_take(int32_t &lo, int32_t &hi, int32_t k)
{
  lo = k < lo ? k : lo;
  hi = k > hi ? k : hi;
}
// n_v
TRX_HD int64_t span_count(int32_t lo, int32_t hi) { return hi >= lo ? (int64_t)hi - lo + 1 : 0; }

// an index row idx[0 .. nexp-1] with a -1: its cell is OUTSIDE
TRX_HD bool index_row_outside(const int32_t *idx, int32_t nexp)
{
  bool out = false;
  for (int32_t v = 0; v < nexp; v++) out = out || idx[v] < 0;
  return out;
}

// The index -> row transform: the pixel row of lag k at the exposure whose span is [lo, hi] and whose rows start at base;
// -1 for k = -1 and for a k outside the span -- which only a cell that is outside at another exposure can have, and the
// cell kernels leave such a cell out whole.  So every entry that is not -1 lies in [base, base + n_v), inside [0, R).
TRX_HD int32_t exposed_map_row(int32_t k, int32_t lo, int32_t hi, int64_t base)
{
  return k < 0 || k < lo || k > hi ? -1 : (int32_t)(base + (k - lo));
}

// what an exposed map refuses for `who` ahead of its tracks: every refusal of a filtered map, then no exposure table
inline int exposed_map_checks(const ProductState &S, const char *who, const trx_vmap *vm, const void *map, std::string &msg)
{
  if (const int rc = filtered_map_checks(S, who, vm, map, msg)) return rc;
  if (!S.exposures) return refuse(msg, TRX_E_ARG, std::string(who) + ": no exposure table installed (trx_set_exposures)");
  return TRX_OK;
}

// The spans span[v] = (lo_v, hi_v) of an index table [cells][nexp] on the host, by k_cell_spans' rule: the cells that are
// not outside alone, an outside cell skipped by its whole index row.
inline void exposed_map_spans(const int32_t *index, int64_t cells, int32_t nexp, int32_t *span /* [nexp][2] */)
{
  for (int32_t v = 0; v < nexp; v++) { span[2 * v] = kSpanEmptyLo; span[2 * v + 1] = kSpanEmptyHi; }
  for (int64_t c = 0; c < cells; c++) {
    const int32_t *idx = index + c * nexp;
    if (index_row_outside(idx, nexp)) continue;
    for (int32_t v = 0; v < nexp; v++) span_take(span[2 * v], span[2 * v + 1], idx[v]);
  }
}

// The rows of a map from its spans (read back from the device): base[v], v = 0 .. nexp (base[nexp] = R), and per row the
// shift lag[l], and the table's smear[v] and scale[v] -- an array the table leaves out stays empty, and NULL for the kernel.
// TRX_E_HIP for a span that is not inside [0, nlag - 1]: the device's table was not what k_cell_tracks writes.
struct ExposedMapRows {
  int64_t R = 0;
  std::vector<int64_t> base;                           // [nexp + 1]
  std::vector<double> shift, smear, scale;             // [R] each, or empty
};
inline int exposed_map_bases(const char *who, const int32_t *span, int32_t nexp, int32_t nlag, ExposedMapRows &L, std::string &msg)
{
  try { L.base.assign((size_t)nexp + 1, 0); } catch (...) { return refuse(msg, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  for (int32_t v = 0; v < nexp; v++) {
    const int32_t lo = span[2 * v], hi = span[2 * v + 1];
    const bool empty = lo == kSpanEmptyLo && hi == kSpanEmptyHi;
    if (!empty && (lo < 0 || hi < lo || hi > nlag - 1)) return refuse(msg, TRX_E_HIP, std::string(who) + ": internal: exposure " + std::to_string(v) + ": a span outside the lag grid");
    L.base[(size_t)v + 1] = L.base[(size_t)v] + span_count(lo, hi);
  }
  L.R = L.base[(size_t)nexp];
  return TRX_OK;
}
inline int exposed_map_row_arrays(const char *who, const int32_t *span, int32_t nexp, const double *lag, const double *scale /* [nexp] or null */,
                                  const double *smear /* [nexp] or null */, ExposedMapRows &L, std::string &msg)
{
  try {
    const size_t R = (size_t)L.R;
    L.shift.assign(R, 0.0); L.smear.assign(smear ? R : 0, 0.0); L.scale.assign(scale ? R : 0, 0.0);
  } catch (...) { return refuse(msg, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  for (int32_t v = 0; v < nexp; v++) {
    const int64_t n = span_count(span[2 * v], span[2 * v + 1]);
    for (int64_t k = 0; k < n; k++) {
      const size_t r = (size_t)(L.base[(size_t)v] + k);
      L.shift[r] = lag[span[2 * v] + k];
      if (smear) L.smear[r] = smear[v];
      if (scale) L.scale[r] = scale[v];
    }
  }
  return TRX_OK;
}

// The extents of an exposed map of R rows: the spans' read-back [nexp][2] int32, the row table [cells][nexp] int32 beside
// the lag table, the pairs [R][npix][2] of the one pixel launch (with a high-pass a second buffer of that size).  Refused
// for `who` (TRX_E_ARG): R * npix above what one pixel launch takes -- and an R that is no int32 count of rows with it --,
// then pairs above `cap` bytes.
struct ExposedMapExtents {
  int64_t rows = 0, pairs = 0;                         // R, R * npix
  int64_t span_lanes = 0, span_blocks = 0;             // k_cell_spans: one wave per exposure, kCellSpanWaves of them a block
  size_t span_bytes = 0, row_bytes = 0, pair_bytes = 0;
};
inline int exposed_map_extents(const char *who, int64_t R, int64_t npix, int64_t cells, int32_t nexp, ExposedMapExtents &X, std::string &msg,
                               uint64_t cap = kExposedMapPairBytes)
{
  X = ExposedMapExtents{};
  X.span_lanes = 64 * (int64_t)nexp; X.span_blocks = ((int64_t)nexp + kCellSpanWaves - 1) / kCellSpanWaves;
  X.span_bytes = sizeof(int32_t) * 2 * (size_t)nexp;
  X.row_bytes = sizeof(int32_t) * (size_t)cells * (size_t)nexp;
  // (R and npix are int32 counts: their product does not overflow)
  if (R < 0 || R > 0x7fffffffLL || npix > 0x7fffffffLL || R * npix > 0x7fffffffLL * kPixBlock)
    return refuse(msg, TRX_E_ARG, std::string(who) + ": R * npix above what one pixel launch takes");
  X.rows = R; X.pairs = R * npix;
  const uint64_t bytes = 16 * (uint64_t)X.pairs;      // (pairs <= 2^31 * kPixBlock: no overflow)
  if (bytes > cap)
    return refuse(msg, TRX_E_ARG, std::string(who) + ": R = " + std::to_string(R) + " rows of " + std::to_string(npix) + " pixels are " + std::to_string(bytes) +
                                      " bytes of pairs, above kExposedMapPairBytes (" + std::to_string(cap) + ")");
  X.pair_bytes = (size_t)bytes;
  return TRX_OK;
}

}  // namespace trx
