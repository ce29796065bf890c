// trx_hpdata.h -- the host side of high-passing the observed set itself on the device (trx_highpass_observed,
// include/transit_hip.h): what the call refuses, the extents of its buffers, its launch's size, and the third level of the
// observed set's data -- the high-passed version over the residuals or the raw set.  Plain C++ (no HIP): trx_api.hip checks
// and sizes with it, tests/hpdata_check.cpp runs the same source on the CPU and drives the buffer transitions with a
// counting fake.  The arithmetic is trx_highpass.h's (highpass_stage_datum, highpass_values), the tiles are the installed
// high-pass's own (highpass_layout, trx_products.h).
#pragma once
#include <stdint.h>

#include <string>

#include "transit_hip.h"
#include "trx_launch.h"
#include "trx_products.h"

namespace trx {

// Whether the call is the undo (apply = 0): the data from before the high-pass back in force.
inline bool hpdata_is_undo(int32_t apply) { return apply == 0; }

// What trx_highpass_observed refuses, in the header's order.
inline int hpdata_checks(const ProductState &S, int32_t apply, std::string &msg)
{
  const char *const who = "trx_highpass_observed";
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (apply != 0 && apply != 1) return no(TRX_E_ARG, "apply must be 0 (undo) or 1");
  if (apply == 1 && !S.highpass) return no(TRX_E_ARG, "no high-pass installed (trx_set_highpass)");
  if (S.windowed) return no(TRX_E_UNSUPPORTED, "this handle's shard is not the whole grid; high-pass on the host (xcor.highpass_observed_reference)");
  return TRX_OK;
}

// The extents of a call over nexp exposures of npix pixels with the installed high-pass's ntiles tiles and half-width: the
// high-passed data [nexp][npix] (what the data and the weights it reads are, too), the kernel's blocks -- one per exposure
// and tile -- and the LDS of one: g and the flags over a tile and its two halos, as highpass_extents sizes them.
struct HpDataExtents { int64_t cells = 0, blocks = 0; size_t r_bytes = 0, lds_bytes = 0; };
inline HpDataExtents hpdata_extents(int64_t npix, int32_t nexp, int64_t ntiles, int32_t half)
{
  HpDataExtents X;
  X.cells = (int64_t)nexp * npix; X.blocks = (int64_t)nexp * ntiles;
  X.r_bytes = sizeof(double) * (size_t)X.cells;
  X.lds_bytes = sizeof(double) * 2 * ((size_t)kHpTile + 2 * (size_t)half);
  return X;
}

// what one launch takes: refused on the host before anything is launched
inline int hpdata_launch_checks(const HpDataExtents &X, std::string &msg)
{
  if (X.blocks < 1) return refuse(msg, TRX_E_ARG, "trx_highpass_observed: the observed set has no pixel in any segment");
  if (!grid_ok(X.blocks)) return refuse(msg, TRX_E_ARG, "trx_highpass_observed: nexp * ntiles above what one launch takes");
  return TRX_OK;
}

// The observed set's DATA have three levels: F as trx_set_observed installed them, SYSREM's residuals r (InForce: adopt,
// restore, raw()), and over either of the two the high-passed version r'.  `covered` says that `now` is an r' and `under`
// what it was made from -- a residual if `adopted`, F otherwise: both flags are explicit, an empty buffer says nothing.
//   cover(fresh)    r' in force: the first time what was in force goes under, later the two swap (fresh then holds the
//                   previous r', a spare for the next call)
//   uncover(spare)  what is under back in force; the r' goes to `spare` where that is empty, and is released otherwise
//   base()          what a high-pass call reads: never an earlier call's r'
//   raw()           F, whatever lies over it
// adopt and restore are InForce's on the uncovered data: a high-pass over them is discarded first (its buffer released,
// unless the caller has uncovered into a spare before).
template <class Buf>
struct DataInForce : InForce<Buf> {
  Buf under; bool covered = false;
  const Buf &base() const { return covered ? under : this->now; }
  const Buf &raw() const { return this->adopted ? this->aside : base(); }
  void cover(Buf &fresh)
  {
    if (!covered) { exchange_buf(under, this->now); covered = true; }
    exchange_buf(this->now, fresh);
  }
  void uncover(Buf &spare)
  {
    if (!covered) return;
    if (!spare.p) exchange_buf(spare, this->now);
    this->now.release(); exchange_buf(this->now, under); covered = false;
  }
  void discard() { if (covered) { this->now.release(); exchange_buf(this->now, under); covered = false; } }
  void adopt(Buf &fresh) { discard(); InForce<Buf>::adopt(fresh); }
  void restore(Buf &spare) { discard(); InForce<Buf>::restore(spare); }
};

}  // namespace trx
