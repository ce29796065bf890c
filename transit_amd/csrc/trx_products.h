// trx_products.h -- the host side of the run products (bands, contributions, pixels, moments, filter, high-pass, trail,
// velocity map, filtered map, broadening; include/transit_hip.h): what their calls refuse, the layouts the device gets, and the extents of a run's
// buffers.  Plain C++ (no HIP), pure arithmetic over the public structs: trx_api.hip checks with it, uploads what it lays
// out and grows, guards and copies by its extents; tests/products_check.cpp runs the same source on the CPU over
// exact-size buffers.  A check returns a TRX_* code and leaves the refusal's text in `msg`; the caller logs it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "transit_hip.h"
#include "hip/trx_device.h"
#include "trx_broaden.h"
#include "trx_highpass.h"
#include "trx_numerics.h"

namespace trx {

// What the checks need to know of a handle (trx_api.hip fills it, product_state): its grid and shard, and the sets installed.
struct ProductState {
  bool windowed = false;                               // the shard [lo, hi) is not the whole grid
  double wn_i = 0, wn_d = 0; int64_t nwn = 0, lo = 0, hi = 0;
  int64_t npix = 0;                                    // the pixel set's (0: none installed)
  int32_t nexp = 0, nseg = 0; const int64_t *seg = nullptr;      // the observed set's, seg its [nseg + 1] host bounds (null: none)
  bool filter = false;                                 // a filter is installed
  bool highpass = false;                               // a high-pass is installed
  bool exposures = false;                              // an exposure table is installed (trx_exposures.h)
};

inline int refuse(std::string &msg, int code, std::string text) { msg = std::move(text); return code; }

// ---- band integrals (hip/trx_bands.hip.h) ----------------------------------------------------------
// The bins [first, last) of the whole grid under a Gaussian (centre, sigma) cut at `cut` sigmas: the rule of TRX_BAND_GAUSS,
// in double, clipped to [0, nwn] there -- no conversion of a value out of int64's range.
inline void gauss_band_range(double wn_i, double wn_d, int64_t nwn, double centre, double sigma, double cut, int64_t &first, int64_t &last)
{
  const double a = std::ceil((centre - cut * sigma - wn_i) / wn_d);
  const double z = std::floor((centre + cut * sigma - wn_i) / wn_d) + 1.0;
  first = a <= 0 ? 0 : a >= (double)nwn ? nwn : (int64_t)a;
  last = z <= 0 ? 0 : z >= (double)nwn ? nwn : (int64_t)z;
  last = std::max(first, last);
}

// The set as the shard [S.lo, S.hi) sees it, checked whole: ranges on the host in double (the header's rule), each band's
// in-shard bins cut into pieces of kBandPiece from its first in-shard bin, WEIGHTS' in-shard weights end to end.
struct BandLayout { std::vector<BandDev> bands; std::vector<BandPiece> pieces; std::vector<double> w; };
inline int band_layout(const ProductState &S, int32_t nbands, const trx_band *bands, BandLayout &L, std::string &msg)
{
  if (nbands < 0) return refuse(msg, TRX_E_ARG, "bands: nbands < 0");
  if (nbands > 0 && !bands) return refuse(msg, TRX_E_ARG, "bands: NULL band array");
  const int64_t nwn = S.nwn, lo = S.lo, hi = S.hi;
  L.bands.assign((size_t)nbands, BandDev{}); L.pieces.clear(); L.w.clear();
  const double fwhm_sigma = 2.0 * std::sqrt(2.0 * std::log(2.0));
  for (int32_t b = 0; b < nbands; b++) {
    const trx_band &B = bands[b];
    const std::string name = "band " + std::to_string(b) + ": ";
    BandDev &D = L.bands[(size_t)b];
    D.kind = B.kind;
    int64_t first = 0, last = 0;                         // [first, last) of the whole grid
    if (B.kind == TRX_BAND_WEIGHTS) {
      if (B.n < 1) return refuse(msg, TRX_E_ARG, name + "n < 1");
      if (B.first < 0) return refuse(msg, TRX_E_ARG, name + "first < 0");
      if (B.first > nwn - B.n) return refuse(msg, TRX_E_ARG, name + "first + n > nwn");
      if (!B.weights) return refuse(msg, TRX_E_ARG, name + "NULL weights");
      for (int64_t k = 0; k < B.n; k++)
        if (!std::isfinite(B.weights[k])) return refuse(msg, TRX_E_ARG, name + "weight " + std::to_string(k) + " is not finite");
      first = B.first; last = B.first + B.n;
    } else if (B.kind == TRX_BAND_GAUSS) {
      if (!std::isfinite(B.centre) || !std::isfinite(B.fwhm) || !std::isfinite(B.cut))
        return refuse(msg, TRX_E_ARG, name + "centre, fwhm and cut must be finite");
      if (!(B.fwhm > 0)) return refuse(msg, TRX_E_ARG, name + "fwhm <= 0");
      if (!(B.cut > 0)) return refuse(msg, TRX_E_ARG, name + "cut <= 0");
      D.centre = B.centre; D.sigma = B.fwhm / fwhm_sigma;
      gauss_band_range(S.wn_i, S.wn_d, nwn, B.centre, D.sigma, B.cut, first, last);
    } else return refuse(msg, TRX_E_ARG, name + "unknown kind " + std::to_string(B.kind));
    const int64_t s = std::max(first, lo), e = std::min(last, hi);
    D.s = s - lo; D.piece0 = (int64_t)L.pieces.size(); D.npieces = 0; D.woff = (int64_t)L.w.size();
    if (e <= s) { D.s = 0; continue; }                   // no bin in this shard: (0, 0)
    if (B.kind == TRX_BAND_WEIGHTS) L.w.insert(L.w.end(), B.weights + (s - first), B.weights + (e - first));
    for (int64_t q = s; q < e; q += kBandPiece) {
      BandPiece P{};
      P.start = q - lo; P.band = b; P.len = (int32_t)std::min<int64_t>(kBandPiece, e - q);
      L.pieces.push_back(P);
    }
    D.npieces = (int64_t)L.pieces.size() - D.piece0;
  }
  return TRX_OK;
}

// the buffers of a contribution run (hip/trx_contrib.hip.h): sub-piece rows [npieces * kContribSplit][nlayer] on the device,
// the pinned result [nbands][nlayer]
struct ContribExtents { size_t cpart_bytes, out_bytes; };
inline ContribExtents contrib_extents(int32_t nlayer, int64_t npieces, int32_t nbands)
{
  const size_t row = sizeof(double) * (size_t)nlayer;
  return ContribExtents{row * (size_t)npieces * kContribSplit, row * (size_t)nbands};
}

// ---- detector pixels (hip/trx_pixels.hip.h) --------------------------------------------------------
// a set that is not a clearing call (px non-null, npix != 0)
inline int pixel_set_checks(const trx_pixels *px, std::string &msg)
{
  if (px->npix < 0) return refuse(msg, TRX_E_ARG, "pixels: npix < 0");
  if (!px->centre || !px->fwhm) return refuse(msg, TRX_E_ARG, "pixels: NULL centre or fwhm array");
  if (!std::isfinite(px->cut) || !(px->cut > 0)) return refuse(msg, TRX_E_ARG, "pixels: cut must be finite and > 0");
  if (px->npix > 0x7fffffffLL) return refuse(msg, TRX_E_ARG, "pixels: npix above 2^31 - 1");
  for (int64_t p = 0; p < px->npix; p++) {
    if (!std::isfinite(px->centre[p]) || !(px->centre[p] > 0)) return refuse(msg, TRX_E_ARG, "pixel " + std::to_string(p) + ": centre must be finite and > 0");
    if (!std::isfinite(px->fwhm[p]) || !(px->fwhm[p] > 0)) return refuse(msg, TRX_E_ARG, "pixel " + std::to_string(p) + ": fwhm must be finite and > 0");
  }
  return TRX_OK;
}

// the shifts of a pixel run for `who`, and what one launch of the pixel kernel takes
inline int pixel_run_checks(const char *who, int32_t nshift, int64_t npix, const double *shift, std::string &msg)
{
  for (int32_t v = 0; v < nshift; v++)
    if (!std::isfinite(shift[v]) || !(shift[v] > 0)) return refuse(msg, TRX_E_ARG, std::string(who) + ": shift " + std::to_string(v) + " must be finite and > 0");
  if ((int64_t)nshift * npix > 0x7fffffffLL * kPixBlock) return refuse(msg, TRX_E_ARG, std::string(who) + ": nshift * npix above what one launch takes");
  return TRX_OK;
}

// The extents of a pixel run of nshift shifts over npix pixels: with an observed set (nexp > 0) its moments [nexp][nseg],
// or (trail) its trail [nshift][nexp][nseg]; with a filter the filtered values [nshift][npix].  What pixel_run grows the
// handle's buffers to, what the launchers' guards hold the buffers against, what the calls copy back.
struct PixelExtents {
  int64_t pairs = 0, blocks = 0;                       // nshift * npix, and the pixel kernel's blocks of kPixBlock of them
  int64_t rows = 0;                                    // rows of TRX_NMOMENT sums: moments or trail (0: neither)
  size_t shift_bytes = 0, pair_bytes = 0;              // d_pixshift [nshift], d_pixout [nshift][npix][2]
  size_t mom_bytes = 0, trail_bytes = 0, val_bytes = 0;      // d_mom, d_trail, d_pixval (0: not of this run)
};
inline PixelExtents pixel_extents(int64_t npix, int32_t nshift, int32_t nexp, int32_t nseg, bool filter, bool trail)
{
  PixelExtents X;
  X.pairs = (int64_t)nshift * npix; X.blocks = (X.pairs + kPixBlock - 1) / kPixBlock;
  X.shift_bytes = sizeof(double) * (size_t)nshift;
  X.pair_bytes = sizeof(double) * 2 * (size_t)X.pairs;
  if (nexp > 0) {
    X.rows = (trail ? (int64_t)nshift : 1) * nexp * nseg;
    const size_t bytes = sizeof(double) * TRX_NMOMENT * (size_t)X.rows;
    if (trail) X.trail_bytes = bytes; else X.mom_bytes = bytes;
  }
  if (filter) X.val_bytes = sizeof(double) * (size_t)X.pairs;
  return X;
}

// ---- moments against observed data (hip/trx_moments.hip.h) -----------------------------------------
// a set that is not a clearing call (ob non-null, nexp != 0)
inline int observed_set_checks(const ProductState &S, const trx_observed *ob, std::string &msg)
{
  if (S.npix < 1) return refuse(msg, TRX_E_ARG, "observed: no pixel set installed (trx_set_pixels)");
  const int64_t npix = S.npix;
  if (ob->nexp < 0) return refuse(msg, TRX_E_ARG, "observed: nexp < 0");
  if (ob->nseg < 1) return refuse(msg, TRX_E_ARG, "observed: nseg < 1");
  if (!ob->seg_first || !ob->data) return refuse(msg, TRX_E_ARG, "observed: NULL seg_first or data array");
  if (ob->seg_first[0] != 0) return refuse(msg, TRX_E_ARG, "observed: seg_first[0] must be 0");
  for (int32_t s = 0; s < ob->nseg; s++)
    if (ob->seg_first[s + 1] < ob->seg_first[s]) return refuse(msg, TRX_E_ARG, "observed: seg_first decreases at segment " + std::to_string(s));
  if (ob->seg_first[ob->nseg] != npix) return refuse(msg, TRX_E_ARG, "observed: seg_first[nseg] must be the pixel set's npix (" + std::to_string(npix) + ")");
  if ((int64_t)ob->nexp * ob->nseg > 0x7fffffffLL) return refuse(msg, TRX_E_ARG, "observed: nexp * nseg above 2^31 - 1");
  auto where = [npix](size_t k) { return "exposure " + std::to_string(k / (size_t)npix) + " pixel " + std::to_string(k % (size_t)npix); };
  const size_t cells = (size_t)ob->nexp * (size_t)npix;
  for (size_t k = 0; k < cells; k++) {
    if (!std::isfinite(ob->data[k])) return refuse(msg, TRX_E_ARG, "observed: " + where(k) + ": datum must be finite");
    if (ob->weight && (!std::isfinite(ob->weight[k]) || !(ob->weight[k] >= 0))) return refuse(msg, TRX_E_ARG, "observed: " + where(k) + ": weight must be finite and >= 0");
  }
  if (ob->gain)
    for (int64_t p = 0; p < npix; p++)
      if (!std::isfinite(ob->gain[p])) return refuse(msg, TRX_E_ARG, "observed: pixel " + std::to_string(p) + ": gain must be finite");
  return TRX_OK;
}

// What a run against the observed set refuses for `who`, in this order: a shard of the grid, no observed set, (Filtered) no
// filter, (Highpassed) no high-pass, the count -- one shift per exposure, or (Trail) at least one lag, or (Highpassed) at
// least one shift: its rows are independent --, the NULL arrays: in (named shift, or lag) and out (named out_name).
enum class ObservedRun { Moments, Filtered, Trail, Highpassed };
inline int observed_run_checks(const ProductState &S, const char *who, ObservedRun kind, int32_t n, const void *in, const void *out, const char *out_name,
                               std::string &msg)
{
  const bool lags = kind == ObservedRun::Trail;
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };      // (no string is built for a run that goes ahead)
  // (the moments are not linear in the pairs: the partial pairs of a shard say nothing about them -- nor about the filtered
  // values' live flags)
  if (S.windowed)
    return no(TRX_E_UNSUPPORTED, std::string("this handle's shard is not the whole grid; take trx_run_pixels, add the ranks' pairs (trx_gather_host) and ") +
                                 (kind == ObservedRun::Filtered ? "filter and reduce" : kind == ObservedRun::Highpassed ? "high-pass" : "reduce") + " them on the host");
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (kind == ObservedRun::Filtered && !S.filter) return no(TRX_E_ARG, "no filter installed (trx_set_filter)");
  if (kind == ObservedRun::Highpassed && !S.highpass) return no(TRX_E_ARG, "no high-pass installed (trx_set_highpass)");
  if (lags && n < 1) return no(TRX_E_ARG, "nlag < 1");
  if (kind == ObservedRun::Highpassed && n < 1) return no(TRX_E_ARG, "nshift < 1");
  if (!lags && kind != ObservedRun::Highpassed && n != S.nexp) return no(TRX_E_ARG, "nshift " + std::to_string(n) + " is not the observed set's nexp " + std::to_string(S.nexp));
  if (!in) return no(TRX_E_ARG, std::string(lags ? "lag" : "shift") + " is NULL");
  if (!out) return no(TRX_E_ARG, std::string(out_name) + " is NULL");
  return TRX_OK;
}

// ---- the cross-correlation trail (hip/trx_trail.hip.h) ---------------------------------------------
// what a trail run refuses, for `who` (trx_run_trail, trx_run_velocity_map); out: where its result goes, named out_name
inline int trail_run_checks(const ProductState &S, const char *who, int32_t nlag, const double *lag, const void *out, const char *out_name, std::string &msg)
{
  if (const int rc = observed_run_checks(S, who, ObservedRun::Trail, nlag, lag, out, out_name, msg)) return rc;
  // (the counts first: a refused nlag is not an extent to read lag[] over)
  if ((int64_t)nlag * S.npix > 0x7fffffffLL * kPixBlock) return refuse(msg, TRX_E_ARG, std::string(who) + ": nlag * npix above what one pixel launch takes");
  if ((int64_t)nlag * S.nexp * S.nseg > 0x7fffffffLL) return refuse(msg, TRX_E_ARG, std::string(who) + ": nlag * nexp * nseg above 2^31 - 1");
  for (int32_t l = 0; l < nlag; l++)
    if (!std::isfinite(lag[l]) || !(lag[l] > 0)) return refuse(msg, TRX_E_ARG, std::string(who) + ": lag " + std::to_string(l) + " must be finite and > 0");
  return TRX_OK;
}

// ---- the Kp-Vsys map of that trail (hip/trx_vmap.hip.h) --------------------------------------------
inline int all_finite(const char *who, const char *name, const double *x, int32_t n, std::string &msg)
{
  for (int32_t k = 0; k < n; k++)
    if (!std::isfinite(x[k])) return refuse(msg, TRX_E_ARG, std::string(who) + ": " + name + " " + std::to_string(k) + " must be finite");
  return TRX_OK;
}

// what a map run refuses on top of a trail run's refusals, for `who`
inline int velocity_map_checks(const ProductState &S, const char *who, const trx_vmap *vm, const void *map, std::string &msg)
{
  if (!vm) return refuse(msg, TRX_E_ARG, std::string(who) + ": vm is NULL");
  if (const int rc = trail_run_checks(S, who, vm->nlag, vm->lag, map, "map", msg)) return rc;
  const int32_t nexp = S.nexp;
  auto no = [&](const std::string &what) { return refuse(msg, TRX_E_ARG, std::string(who) + ": " + what); };
  if (vm->stat != TRX_STAT_CCF && vm->stat != TRX_STAT_LOGLIKE_BL19 && vm->stat != TRX_STAT_CHI2) return no("unknown stat " + std::to_string(vm->stat));
  if (vm->nkp < 1 || vm->nvsys < 1) return no("nkp < 1 or nvsys < 1");
  if ((int64_t)vm->nkp * vm->nvsys > 0x7fffffffLL) return no("nkp * nvsys above 2^31 - 1");
  if (!vm->lag_kms) return no("lag_kms is NULL");
  if (!vm->kp) return no("kp is NULL");
  if (!vm->vsys) return no("vsys is NULL");
  if (!vm->orbit) return no("orbit is NULL");
  if (!std::isfinite(vm->p0)) return no("p0 must be finite");
  if (!std::isfinite(vm->p1)) return no("p1 must be finite");
  int rc;
  if ((rc = all_finite(who, "kp", vm->kp, vm->nkp, msg)) || (rc = all_finite(who, "vsys", vm->vsys, vm->nvsys, msg)) ||
      (rc = all_finite(who, "orbit", vm->orbit, nexp, msg)) || (vm->offset && (rc = all_finite(who, "offset", vm->offset, nexp, msg))))
    return rc;
  for (int32_t l = 0; l < vm->nlag; l++)
    if (!std::isfinite(vm->lag_kms[l]) || (l > 0 && !(vm->lag_kms[l] > vm->lag_kms[l - 1])))
      return no("lag_kms " + std::to_string(l) + " must be finite and above the one before it (strictly increasing)");
  return TRX_OK;
}

// A map run's buffers: the call's arrays lag_kms, kp, vsys, orbit and (given) offset end to end -- `nin` doubles, each
// array at its at_* --, the statistic [nlag][nexp] (`rows` entries) followed by its transpose, the map's `cells`.
struct VmapExtents {
  size_t at_kp, at_vsys, at_orbit, at_offset, nin, rows, cells;
  size_t in_bytes, per_bytes, per2_bytes, map_bytes;   // d_vm_in, one orientation of the statistic, d_vm_per (both), d_vm_map
};
inline VmapExtents vmap_extents(const trx_vmap &vm, int32_t nexp_)
{
  const size_t nlag = (size_t)vm.nlag, nexp = (size_t)nexp_, nkp = (size_t)vm.nkp, nvsys = (size_t)vm.nvsys;
  VmapExtents X{};
  X.at_kp = nlag; X.at_vsys = X.at_kp + nkp; X.at_orbit = X.at_vsys + nvsys; X.at_offset = X.at_orbit + nexp; X.nin = X.at_offset + (vm.offset ? nexp : 0);
  X.rows = nlag * nexp; X.cells = nkp * nvsys;
  X.in_bytes = sizeof(double) * X.nin; X.per_bytes = sizeof(double) * X.rows; X.per2_bytes = 2 * X.per_bytes; X.map_bytes = sizeof(double) * X.cells;
  return X;
}
// the call's arrays end to end into `in`, as the device gets them
inline int vmap_pack(const char *who, const trx_vmap &vm, const VmapExtents &X, std::vector<double> &in, std::string &msg)
{
  try {
    in.resize(X.nin);
  } catch (...) { return refuse(msg, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  std::copy(vm.lag_kms, vm.lag_kms + X.at_kp, in.begin());
  std::copy(vm.kp, vm.kp + vm.nkp, in.begin() + (std::ptrdiff_t)X.at_kp);
  std::copy(vm.vsys, vm.vsys + vm.nvsys, in.begin() + (std::ptrdiff_t)X.at_vsys);
  std::copy(vm.orbit, vm.orbit + (X.at_offset - X.at_orbit), in.begin() + (std::ptrdiff_t)X.at_orbit);
  if (vm.offset) std::copy(vm.offset, vm.offset + (X.nin - X.at_offset), in.begin() + (std::ptrdiff_t)X.at_offset);
  return TRX_OK;
}

// ---- the detrending filter (hip/trx_filter.hip.h) --------------------------------------------------
// a filter that is not a clearing call (f non-null, ncomp != 0)
inline int filter_set_checks(const ProductState &S, const trx_filter *f, std::string &msg)
{
  if (S.npix < 1 || !S.seg) return refuse(msg, TRX_E_ARG, "filter: no observed set installed (trx_set_observed)");
  if (f->ncomp < 0) return refuse(msg, TRX_E_ARG, "filter: ncomp < 0");
  if (f->ncomp > TRX_FILTER_MAX) return refuse(msg, TRX_E_ARG, "filter: ncomp above TRX_FILTER_MAX (" + std::to_string(TRX_FILTER_MAX) + ")");
  if (!f->fwd || !f->back) return refuse(msg, TRX_E_ARG, "filter: NULL fwd or back array");
  const size_t per = (size_t)f->ncomp * (size_t)S.nexp;
  for (int32_t s = 0; s < S.nseg; s++)
    for (size_t k = 0; k < per; k++) {
      if (!std::isfinite(f->fwd[(size_t)s * per + k])) return refuse(msg, TRX_E_ARG, "filter: segment " + std::to_string(s) + ": fwd entry must be finite");
      if (!std::isfinite(f->back[(size_t)s * per + k])) return refuse(msg, TRX_E_ARG, "filter: segment " + std::to_string(s) + ": back entry must be finite");
    }
  return TRX_OK;
}

// What the device gets of a checked filter over the observed set of S: the two matrices exposure-major [nseg][nexp][npad] and
// zero-padded to the kernel's 4, 8 or 16 components, and the tiles of the set's segments: up to 64 consecutive pixels of
// one segment each, a segment's tiles in pixel order.
struct FilterLayout { int32_t npad = 0; std::vector<double> fwd, back; std::vector<FilterTile> tiles; };
inline int filter_layout(const ProductState &S, const trx_filter *f, FilterLayout &L, std::string &msg)
{
  L.npad = f->ncomp <= 4 ? 4 : f->ncomp <= 8 ? 8 : 16;
  try {
    const size_t nc = (size_t)f->ncomp, ne = (size_t)S.nexp, np = (size_t)L.npad;
    L.fwd.assign((size_t)S.nseg * ne * np, 0.0); L.back.assign((size_t)S.nseg * ne * np, 0.0); L.tiles.clear();
    for (size_t s = 0; s < (size_t)S.nseg; s++)
      for (size_t v = 0; v < ne; v++)
        for (size_t j = 0; j < nc; j++) {
          L.fwd[(s * ne + v) * np + j] = f->fwd[(s * nc + j) * ne + v];
          L.back[(s * ne + v) * np + j] = f->back[(s * ne + v) * nc + j];
        }
    for (int32_t s = 0; s < S.nseg; s++)
      for (int64_t p = S.seg[(size_t)s]; p < S.seg[(size_t)s + 1]; p += 64)
        L.tiles.push_back(FilterTile{p, s, (int32_t)std::min<int64_t>(64, S.seg[(size_t)s + 1] - p)});
  } catch (...) { return refuse(msg, TRX_E_NOMEM, "filter: out of host memory"); }
  return TRX_OK;
}

// ---- the high-pass along the pixel axis (hip/trx_highpass.hip.h) ------------------------------------
// a high-pass that is not a clearing call (hp and hp->taps non-null)
inline int highpass_set_checks(const ProductState &S, const trx_highpass *hp, std::string &msg)
{
  if (S.npix < 1 || !S.seg) return refuse(msg, TRX_E_ARG, "highpass: no observed set installed (trx_set_observed)");
  if (hp->half < 0) return refuse(msg, TRX_E_ARG, "highpass: half < 0");
  if (hp->half > TRX_HIGHPASS_MAX_HALF) return refuse(msg, TRX_E_ARG, "highpass: half above TRX_HIGHPASS_MAX_HALF (" + std::to_string(TRX_HIGHPASS_MAX_HALF) + ")");
  for (int32_t k = 0; k <= hp->half; k++)
    if (!std::isfinite(hp->taps[k]) || !(hp->taps[k] >= 0)) return refuse(msg, TRX_E_ARG, "highpass: tap " + std::to_string(k) + " must be finite and >= 0");
  if (!(hp->taps[0] > 0)) return refuse(msg, TRX_E_ARG, "highpass: tap 0 must be > 0");
  return TRX_OK;
}

// What the device gets of a checked high-pass over the observed set of S: the taps, the full-window denominator
// (highpass_full_den: the sum in the kernel's order) and the tiles of the set's segments: up to kHpTile consecutive pixels
// of one segment each, with that segment's bounds, a segment's tiles in pixel order.
struct HighpassLayout { int32_t half = 0; double den_full = 0; std::vector<double> taps; std::vector<HpTile> tiles; };
inline int highpass_layout(const ProductState &S, const trx_highpass *hp, HighpassLayout &L, std::string &msg)
{
  try {
    L.half = hp->half; L.taps.assign(hp->taps, hp->taps + hp->half + 1); L.tiles.clear();
    L.den_full = highpass_full_den(L.half, L.taps.data());
    for (int32_t s = 0; s < S.nseg; s++) {
      const int64_t a = S.seg[(size_t)s], z = S.seg[(size_t)s + 1];
      for (int64_t p = a; p < z; p += kHpTile) L.tiles.push_back(HpTile{p, a, z, (int32_t)std::min<int64_t>(kHpTile, z - p), 0});
    }
  } catch (...) { return refuse(msg, TRX_E_NOMEM, "highpass: out of host memory"); }
  return TRX_OK;
}

// The extents of a high-pass over nshift rows of npix pixels with ntiles tiles: the pair buffer [nshift][npix][2] the kernel
// writes (d_pixhp) -- and a highpassed run copies to pinned memory whole --, its values [nshift][npix], the kernel's blocks
// (one per row and tile) and the LDS of one: g and the flags over a tile and its two halos.
struct HighpassExtents { int64_t pairs = 0, blocks = 0; size_t pair_bytes = 0, val_bytes = 0, lds_bytes = 0; };
inline HighpassExtents highpass_extents(int64_t npix, int32_t nshift, int64_t ntiles, int32_t half)
{
  HighpassExtents X;
  X.pairs = (int64_t)nshift * npix; X.blocks = (int64_t)nshift * ntiles;
  X.pair_bytes = sizeof(double) * 2 * (size_t)X.pairs; X.val_bytes = sizeof(double) * (size_t)X.pairs;
  X.lds_bytes = sizeof(double) * 2 * ((size_t)kHpTile + 2 * (size_t)half);
  return X;
}

// ---- the Kp-Vsys map with the filter applied per cell (hip/trx_cellmap.hip.h) -----------------------
// what a filtered map refuses for `who`: every refusal of a map run, then no filter, then more index entries than int32 counts
inline int filtered_map_checks(const ProductState &S, const char *who, const trx_vmap *vm, const void *map, std::string &msg)
{
  if (const int rc = velocity_map_checks(S, who, vm, map, msg)) return rc;
  if (!S.filter) return refuse(msg, TRX_E_ARG, std::string(who) + ": no filter installed (trx_set_filter)");
  if ((int64_t)vm->nkp * vm->nvsys * S.nexp > 0x7fffffffLL) return refuse(msg, TRX_E_ARG, std::string(who) + ": nkp * nvsys * nexp above 2^31 - 1");
  return TRX_OK;
}

// A filtered map's buffers.  The cells go through the filter and the moments in chunks: `chunk` cells at a time -- cell_cap
// at the most, fewer where the chunk's values would be above val_cap bytes or its moment rows above 2^31 - 1, never fewer
// than one --, `nchunks` of them, the last with last_chunk cells.  The index table [cells][nexp] int32 and the map [cells]
// are the whole call's; the values [chunk][nexp][npix] and the moments [chunk][nexp][nseg][TRX_NMOMENT] are one chunk's.
struct CellMapExtents {
  int64_t cells = 0, chunk = 0, nchunks = 0, last_chunk = 0;
  int64_t tracks = 0, track_blocks = 0;                // cells * nexp, and k_cell_tracks' blocks of kCellTrackBlock of them
  int64_t rows = 0;                                    // moment rows of a full chunk: chunk * nexp * nseg
  size_t index_bytes = 0, val_bytes = 0, mom_bytes = 0, map_bytes = 0;
};
inline CellMapExtents cell_map_extents(int64_t cells, int32_t nexp, int32_t nseg, int64_t npix, int64_t cell_cap = kCellMapChunk,
                                       uint64_t val_cap = kCellMapValBytes)
{
  CellMapExtents X;
  const uint64_t cell_val = sizeof(double) * (uint64_t)nexp * (uint64_t)npix;      // one cell's values
  const int64_t cell_rows = (int64_t)nexp * nseg;
  X.cells = cells;
  X.chunk = std::min(cells, cell_cap);
  if (cell_val > 0) X.chunk = std::min<int64_t>(X.chunk, (int64_t)std::min<uint64_t>(val_cap / cell_val, 0x7fffffffULL));
  if (cell_rows > 0) X.chunk = std::min<int64_t>(X.chunk, 0x7fffffffLL / cell_rows);
  X.chunk = std::max<int64_t>(X.chunk, 1);
  X.nchunks = (cells + X.chunk - 1) / X.chunk;
  X.last_chunk = cells - (X.nchunks - 1) * X.chunk;
  X.tracks = cells * nexp; X.track_blocks = (X.tracks + kCellTrackBlock - 1) / kCellTrackBlock;
  X.rows = X.chunk * cell_rows;
  X.index_bytes = sizeof(int32_t) * (size_t)X.tracks;
  X.val_bytes = (size_t)cell_val * (size_t)X.chunk;
  X.mom_bytes = sizeof(double) * TRX_NMOMENT * (size_t)X.rows;
  X.map_bytes = sizeof(double) * (size_t)cells;
  return X;
}

// ---- rotational broadening (hip/trx_broaden.hip.h) -------------------------------------------------
// a broadening that is not a clearing call (br non-null, kind != TRX_BROADEN_NONE); hmax: the half-width of the grid's last
// bin -- the largest
inline int broadening_checks(const ProductState &S, const trx_broadening *br, int &hmax, std::string &msg)
{
  if (br->kind != TRX_BROADEN_ROTATION) return refuse(msg, TRX_E_ARG, "broadening: unknown kind " + std::to_string(br->kind));
  if (!std::isfinite(br->beta) || !(br->beta > 0)) return refuse(msg, TRX_E_ARG, "broadening: beta must be finite and > 0");
  if (!std::isfinite(br->limb) || !(br->limb >= 0) || !(br->limb <= 1)) return refuse(msg, TRX_E_ARG, "broadening: limb must be finite and in [0, 1]");
  if (!(S.wn_i > 0) || !(S.wn_d > 0)) return refuse(msg, TRX_E_ARG, "broadening: the handle's grid needs wn_i > 0 and wn_d > 0");
  // (the window needs neighbours across the shard's edge)
  if (S.windowed)
    return refuse(msg, TRX_E_UNSUPPORTED, "broadening: this handle's shard is not the whole grid; gather the spectrum (trx_gather_host) and broaden it on the host");
  double d;
  const double half = broaden_half(S.wn_i, S.wn_d, br->beta, S.nwn - 1, d);
  if (!(half <= (double)TRX_BROADEN_MAX_HALF)) {
    char b[160]; std::snprintf(b, sizeof b, "broadening: half-width of %.0f bins at the grid's last bin is above TRX_BROADEN_MAX_HALF (%d)", half, TRX_BROADEN_MAX_HALF);
    return refuse(msg, TRX_E_ARG, b);
  }
  hmax = (int)half;
  return TRX_OK;
}
// the broadened spectrum [nwn] (d_broad)
inline size_t broadened_bytes(int64_t nwn) { return sizeof(double) * (size_t)nwn; }

// ---- several atmospheres per call -------------------------------------------------------------------
// a NULL row among the k rows of the arrays named: by atmosphere, then in the order given (an array that is NULL itself is
// an optional one the caller left out)
struct BatchRows { const char *name; const double *const *rows; };
inline int batch_rows_check(const char *who, int32_t k, std::initializer_list<BatchRows> arrays, std::string &msg)
{
  for (int32_t j = 0; j < k; j++)
    for (const BatchRows &A : arrays)
      if (A.rows && !A.rows[j]) return refuse(msg, TRX_E_ARG, std::string(who) + ": " + A.name + "[" + std::to_string(j) + "] is NULL");
  return TRX_OK;
}

}  // namespace trx
