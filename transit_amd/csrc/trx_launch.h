// trx_launch.h -- the conditions the product launchers of trx_api.hip share, each decided once: a grid's size, the filter's
// padded component counts, who reads a run's pairs, when the observed set and the filter over it are whole on the device,
// and which buffer of the observed set is in force.  Plain C++ (no HIP): the predicates are templates over anything with
// .p / .bytes members and the sets' plain counts, so tests/products_check.cpp calls them with plain structs and drives the
// buffer transitions with a counting fake.
#pragma once
#include <stdint.h>

#include <cstddef>

#include "trx_products.h"
#include "trx_wfilter.h"

namespace trx {

// ---- grids -------------------------------------------------------------------------------------------
// what one launch takes as gridDim.x
inline bool grid_ok(int64_t blocks) { return blocks >= 1 && blocks <= 0x7fffffffLL; }
// the blocks of `per` items that cover n, and whether they are a grid
inline bool blocks_for(int64_t n, int64_t per, int64_t *blocks) { *blocks = (n + per - 1) / per; return grid_ok(*blocks); }

// the padded component counts the filter kernels are instantiated for (filter_layout pads to them)
inline bool npad_ok(int32_t npad) { return npad == 4 || npad == 8 || npad == 16; }

// ---- who reads the pairs -----------------------------------------------------------------------------
// What a reader of a pixel run's pairs takes: the high-passed pairs where the run has a high-pass (hpx non-null: its
// extents) -- (g', 1) or (0, 0), the gain in them already, so none is given --, the pixel kernel's otherwise, with the
// gains of the observed set that applies (gain null: none does).  whole: every byte behind both pointers is there, X the
// run's extents -- the pixel kernel's own pairs too, which the high-pass read.
struct PairSource { void *pairs = nullptr; void *gain = nullptr; bool whole = false; };
template <class Buf>
inline PairSource pair_source(const PixelExtents &X, const HighpassExtents *hpx, const Buf &pixout, const Buf &pixhp, const Buf *gain, int64_t npix)
{
  PairSource S;
  S.pairs = hpx ? pixhp.p : pixout.p; S.gain = gain && !hpx ? gain->p : nullptr;
  S.whole = S.pairs && npix >= 1 && pixout.bytes >= X.pair_bytes && (!hpx || (hpx->pairs == X.pairs && pixhp.bytes >= hpx->pair_bytes)) &&
            (!S.gain || gain->bytes >= sizeof(double) * (size_t)npix);
  return S;
}

// ---- a buffer in force with its raw version aside ----------------------------------------------------
// two owning buffers trade what they hold (never by copy: each releases what it holds when it goes)
template <class Buf>
inline void exchange_buf(Buf &a, Buf &b) { void *p = a.p; a.p = b.p; b.p = p; const size_t n = a.bytes; a.bytes = b.bytes; b.bytes = n; }

// The observed set's data and weights: `now` is what every run reads; a call that makes a new version adopts it, and the
// version trx_set_observed installed waits aside until restore puts it back.  The flag is explicit: a set without weights
// has an empty raw version, which is a legal one.  Buf: p, bytes, release().
template <class Buf>
struct InForce {
  Buf now, aside; bool adopted = false;
  const Buf &raw() const { return adopted ? aside : now; }
  // `fresh` in force: the first time the raw version goes aside, later the two swap (fresh then holds the previous one)
  void adopt(Buf &fresh)
  {
    if (adopted) { exchange_buf(now, fresh); return; }
    exchange_buf(aside, now); exchange_buf(now, fresh); adopted = true;
  }
  // the raw version back in force; the buffer that was goes to `spare` where that is empty, and is released otherwise
  void restore(Buf &spare)
  {
    if (!adopted) return;
    if (!spare.p) exchange_buf(spare, now);
    now.release(); exchange_buf(now, aside); adopted = false;
  }
};

// ---- the sets, whole on the device -------------------------------------------------------------------
// The observed set O as the kernels over it read it: counts of at least one, the host's bounds [nseg + 1] from 0 to npix
// and their copy on the device, the weights `weight` (O's in force, or its raw ones; none: all 1) and the gains (none:
// all 1) over their extents, and (reads_data) the data in force over [nexp][npix].
template <class Obs, class Buf>
inline bool observed_set_whole(const Obs &O, const Buf &weight, bool reads_data)
{
  const size_t cells = sizeof(double) * (size_t)O.nexp * (size_t)O.npix;
  return O.nexp >= 1 && O.nseg >= 1 && O.npix >= 1 && O.seg.size() == (size_t)O.nseg + 1 && O.seg.front() == 0 && O.seg.back() == O.npix &&
         O.d_seg.p && O.d_seg.bytes >= sizeof(int64_t) * ((size_t)O.nseg + 1) && (!reads_data || (O.d_data.now.p && O.d_data.now.bytes >= cells)) &&
         (!weight.p || weight.bytes >= cells) && (!O.d_gain.p || O.d_gain.bytes >= sizeof(double) * (size_t)O.npix);
}

// what a plain and a weighted filter F over O share: the counts, O's shape, and the tiles
template <class Filt, class Obs>
inline bool filter_frame_whole(const Filt &F, const Obs &O)
{
  return F.nexp >= 1 && F.nseg >= 1 && F.ncomp >= 1 && F.ncomp <= F.npad && npad_ok(F.npad) && F.npix >= 1 && F.ntiles >= 1 &&
         F.npix == O.npix && F.nexp == O.nexp && F.nseg == O.nseg && F.d_tiles.p && F.d_tiles.bytes >= sizeof(FilterTile) * (size_t)F.ntiles;
}

// the plain filter F over O: its two padded matrices [nseg][nexp][npad] and the frame
template <class Filt, class Obs>
inline bool filter_set_whole(const Filt &F, const Obs &O)
{
  const size_t mat = sizeof(double) * (size_t)F.nseg * (size_t)F.nexp * (size_t)F.npad;
  return !F.weighted && filter_frame_whole(F, O) && F.d_fwd.p && F.d_fwd.bytes >= mat && F.d_back.p && F.d_back.bytes >= mat;
}

// what the factor kernel reads of the weighted filter F over O: the padded basis and the frame (WX: F's extents)
template <class Filt, class Obs>
inline bool wfilter_basis_whole(const Filt &F, const Obs &O, const WfilterExtents &WX)
{
  return F.weighted && filter_frame_whole(F, O) && F.nfac == WX.nfac && F.d_back.p && F.d_back.bytes >= WX.basis_bytes;
}

// what the weighted kernels read of F over O, whole: that, every column's factor and flag, and O's weights in force
template <class Filt, class Obs>
inline bool wfilter_set_complete(const Filt &F, const Obs &O)
{
  const WfilterExtents WX = wfilter_extents(F.npix, F.nexp, F.nseg, F.ncomp, F.npad, F.ntiles, 1);
  return wfilter_basis_whole(F, O, WX) && F.d_fac.p && F.d_live.p && F.d_fac.bytes >= WX.fac_bytes && F.d_live.bytes >= WX.live_bytes &&
         (!O.d_weight.now.p || O.d_weight.now.bytes >= sizeof(double) * (size_t)O.nexp * (size_t)O.npix);
}

}  // namespace trx
