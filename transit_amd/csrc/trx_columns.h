// trx_columns.h -- how a pixel column of the observed set is walked: the trip loop the "one lane per column, loop over the
// exposures" kernels share, and its trip counts.  Plain C++ (no HIP): the column functions of trx_sysrem.h, trx_scatter.h,
// trx_wfilter.h and trx_regress.h walk their exposures through exposure_trips, on the device per lane and in the tests' check
// programs on the CPU over exact-size arrays -- one clamp and one guard for all of them.
//
// Two column functions keep the loop written out, line for line the one below: scatter_column (trx_scatter.h) and norm_column
// (trx_normalise.h).  Their terms are conditional on the entry's own weight, and through the helper the device compiler sinks
// the first exposure's load of every trip into that condition: a branch under the exec mask per trip, and a load that waits
// for another.  Written out it does not.  They are plain host/device functions all the same: their check programs call them.
#pragma once
#include <stdint.h>

#include "trx_numerics.h"

namespace trx {

constexpr int kSysTrips = 8;                          // exposures whose loads a column of the observed set has in flight at once
constexpr int kFiltTrips = 4;                         // the same where a lane carries a component's accumulators: the filter kernels

// an exposure's datum and weight, as a trip loads them
struct WeightedEntry { double f, w; };

// The exposures 0 .. nexp-1 in trips of K: load(v) of a trip's K exposures first -- a trip past the last exposure loads the last
// one again, so that every load is of an exposure there is --, then use(v, what load(v) gave) for the exposures of the trip
// there are, ascending.  Both inner loops unroll: a trip's loads are all issued before its first use.  nexp < 1: nothing.
template <int K, class Load, class Use>
TRX_HD void exposure_trips(int nexp, Load load, Use use)
{
  const int last = nexp - 1;
  for (int v0 = 0; v0 < nexp; v0 += K) {
    decltype(load(0)) got[K];
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < K; t++) got[t] = load(v0 + t < last ? v0 + t : last);
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < K; t++)
      if (v0 + t < nexp) use(v0 + t, got[t]);
  }
}

}  // namespace trx
