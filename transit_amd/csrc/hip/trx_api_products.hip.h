// trx_api_products.hip.h -- the run products behind the spectrum: the launchers of their kernels, Run::product_kernels,
// which queues them behind a pass's spectrum, and the calls of include/transit_hip.h that install a set or run a product,
// from the band integrals to the broadening.  What the calls refuse, the layouts and the extents are ../trx_products.h's
// and its neighbours'; the conditions the launchers share are ../trx_launch.h's.  Part of the one translation unit
// trx_api.hip, which includes it inside its extern "C" block behind the run path (Run, run_once).
#pragma once

namespace {

// ---- the product launchers: what a run makes of a pass's spectrum d_out [nsh] (Run::product_kernels), each behind it on
// the queue st.  A pass that resumes deeper queues them again behind its own spectrum: what the host reads is the last pass's.
// a kernel template over the filter's padded component count (npad_ok, ../trx_launch.h), launched for npad
#define LAUNCH_NPAD(kernel, npad, grid, block, st, args)                                        \
  do { if ((npad) == 4) hipLaunchKernelGGL(kernel<4>, grid, block, 0, st, args);                \
       else if ((npad) == 8) hipLaunchKernelGGL(kernel<8>, grid, block, 0, st, args);           \
       else hipLaunchKernelGGL(kernel<16>, grid, block, 0, st, args); } while (0)

// who reads px's pairs (pair_source, ../trx_launch.h): O the observed set whose gains apply (null: none)
static PairSource pair_source(const trx_handle *h, const PixelRun &px, const ObservedSet *O)
{ return pair_source(px.ext, px.hp ? &px.hpx : nullptr, h->d_pixout, h->d_pixhp, O ? &O->d_gain : nullptr, px.set->npix); }

// ---- band integrals of the spectrum (trx_bands.hip.h)
static int launch_bands(trx_handle *h, const BandSet *bs, const double *d_out, hipStream_t st)
{
  if (!bs || bs->nbands <= 0) return TRX_OK;
  BandArgs BA{};
  BA.spec = d_out; BA.bands = bs->d_bands.as<BandDev>(); BA.pieces = bs->d_pieces.as<BandPiece>();
  BA.w = bs->d_w.as<double>(); BA.part = bs->d_part.as<double>(); BA.out = (double *)bs->h_out.dev;
  BA.npieces = bs->npieces; BA.lo = h->lo; BA.nbands = bs->nbands; BA.wn_i = h->wn_i; BA.wn_d = h->wn_d;
  if (!BA.spec || !BA.bands || !BA.part || !BA.out || (bs->npieces > 0 && !BA.pieces))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the band kernels (not launched)");
  if (bs->npieces > 0)
    hipLaunchKernelGGL(k_band_pieces, dim3((unsigned)((bs->npieces + kBandWaves - 1) / kBandWaves)), dim3(64 * kBandWaves), 0, st, BA);
  hipLaunchKernelGGL(k_band_sums, dim3((unsigned)((bs->nbands + kBandWaves - 1) / kBandWaves)), dim3(64 * kBandWaves), 0, st, BA);
  return TRX_OK;
}

// ---- the contribution functions of the pass's optical depths (trx_contrib.hip.h), behind the band kernels: E the run's
// grid, tau and last, with the angles of vertical rays (Run::contrib_args)
static int launch_contrib(trx_handle *h, const BandSet *bs, const EmisArgs &E, bool vertical, hipStream_t st)
{
  if (!bs || bs->nbands <= 0) return TRX_OK;
  ContribArgs CA{};
  CA.E = E;
  CA.bands = bs->d_bands.as<BandDev>(); CA.pieces = bs->d_pieces.as<BandPiece>(); CA.w = bs->d_w.as<double>();
  CA.part = h->d_cpart.as<double>(); CA.out = (double *)h->h_contrib.dev;
  CA.npieces = bs->npieces; CA.nbands = bs->nbands; CA.vertical = vertical ? 1 : 0;
  const int nr = E.nr; const int64_t nsh = E.nsh;
  const size_t rows = sizeof(double) * (size_t)nr;
  const ContribExtents CX = contrib_extents(nr, bs->npieces, bs->nbands);
  if (!CA.E.tau || !CA.E.last || !CA.E.temp || !CA.E.e2tab || !CA.bands || !CA.part || !CA.out || (bs->npieces > 0 && !CA.pieces) ||
      (vertical && (CA.E.nang < 1 || CA.E.nang > kMaxAngles)) || h->d_tau.bytes < rows * (size_t)nsh || h->d_last.bytes < sizeof(int) * (size_t)nsh ||
      h->d_cpart.bytes < CX.cpart_bytes || h->h_contrib.bytes < CX.out_bytes)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the contribution kernels (not launched)");
  if (bs->npieces > 0) {
    const dim3 cgrid((unsigned)(bs->npieces * kContribSplit), (unsigned)((nr + kContribHeights - 1) / kContribHeights));
    hipLaunchKernelGGL(CA.E.nang <= 8 ? k_contrib_pieces<8> : k_contrib_pieces<kMaxAngles>, cgrid, dim3(64 * kContribWaves), 0, st, CA);
  }
  hipLaunchKernelGGL(k_contrib_sums, dim3((unsigned)(((int64_t)bs->nbands * nr + kBandWaves - 1) / kBandWaves)), dim3(64 * kBandWaves), 0, st, CA);
  return TRX_OK;
}

// ---- the rotational broadening of the spectrum (trx_broaden.hip.h), ahead of the pixel kernel, which then reads d_broad
static int launch_broaden(trx_handle *h, const Broadening *br, const double *d_out, int64_t nsh, hipStream_t st)
{
  if (!br) return TRX_OK;
  BroadArgs BA{};
  BA.spec = d_out; BA.out = h->d_broad.as<double>(); BA.nwn = h->nwn;
  BA.wn_i = h->wn_i; BA.wn_d = h->wn_d; BA.beta = br->beta; BA.W = broaden_weights(br->limb); BA.hmax = br->hmax;
  int64_t blocks;
  const bool grid = blocks_for(BA.nwn, kBroadBlock, &blocks);
  const size_t lds = sizeof(double) * ((size_t)kBroadBlock + 2 * (size_t)(br->hmax > 0 ? br->hmax : 0));
  // (every address the kernel reads or writes: the spectrum -- the handle's own where the run has no other target -- and the
  // broadened one over [0, nwn) = [0, nsh) -- the whole grid, or trx_set_broadening would have refused --, and a tile of at
  // most kBroadBlock + 2 hmax doubles of LDS)
  double d_last;
  if (!BA.spec || !BA.out || h->windowed() || nsh != h->nwn || h->d_broad.bytes < broadened_bytes(nsh) ||
      (d_out == h->d_spec.as<double>() && h->d_spec.bytes < sizeof(double) * (size_t)nsh) || !(BA.wn_i > 0) || !(BA.wn_d > 0) || !(BA.beta > 0) ||
      br->hmax < 0 || br->hmax > TRX_BROADEN_MAX_HALF || broaden_half(BA.wn_i, BA.wn_d, BA.beta, BA.nwn - 1, d_last) != (double)br->hmax || !grid)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the broadening kernel (not launched)");
  hipLaunchKernelGGL(k_broaden, dim3((unsigned)blocks), dim3(kBroadBlock), lds, st, BA);
  return TRX_OK;
}

// ---- the detector pixels of the spectrum -- spec: d_out, or d_broad behind a broadening -- at the run's shifts (trx_pixels.hip.h)
static int launch_pixels(trx_handle *h, const PixelRun *px, const double *spec, int64_t nsh, hipStream_t st)
{
  if (!px) return TRX_OK;
  const PixelSet &S = *px->set; const PixelExtents &X = px->ext;
  PixArgs PA{};
  PA.spec = spec; PA.centre = S.d_centre.as<double>(); PA.fwhm = S.d_fwhm.as<double>();
  PA.shift = h->d_pixshift.as<double>(); PA.out = h->d_pixout.as<double>();
  PA.npix = S.npix; PA.npairs = S.npix * (int64_t)px->nshift;
  PA.nwn = h->nwn; PA.lo = h->lo; PA.hi = h->hi; PA.cut = S.cut; PA.fwhm_sigma = 2.0 * std::sqrt(2.0 * std::log(2.0));
  PA.wn_i = h->wn_i; PA.wn_d = h->wn_d;
  const int64_t blocks = X.blocks;
  // (every address the kernel reads or writes: the spectrum over [0, hi - lo) = [0, nsh), the set's arrays, the shifts, the pairs
  // -- by the extents pixel_run grew the buffers to, which are this launch's: X.pairs)
  if (!PA.spec || !PA.centre || !PA.fwhm || !PA.shift || !PA.out || S.npix < 1 || px->nshift < 1 || h->hi - h->lo != nsh || X.pairs != PA.npairs ||
      S.d_centre.bytes < sizeof(double) * (size_t)S.npix || S.d_fwhm.bytes < sizeof(double) * (size_t)S.npix ||
      h->d_pixshift.bytes < X.shift_bytes || h->d_pixout.bytes < X.pair_bytes || !grid_ok(blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the pixel kernel (not launched)");
  const ExposureSet *const ex = px->ex;
  if (!ex) {
    hipLaunchKernelGGL(k_pixel_pairs, dim3((unsigned)blocks), dim3(kPixBlock), 0, st, PA);
    return TRX_OK;
  }
  // the rows are exposures: the table's arrays, one entry per row (pixel_run sent them ahead with the shifts)
  const ExposureExtents EX = exposure_extents(ex->nexp);
  if (!ex->scale.empty()) PA.scale = h->d_exscale.as<double>();
  if (!ex->smear.empty()) PA.smear = h->d_exsmear.as<double>();
  PA.sqrt2 = std::sqrt(2.0);
  // (every further address the kernel reads: scale and smear over [0, nshift) = [0, nexp))
  // (the set is the handle's -- or the rows' own of an exposed map, which never has obs, filt or trail)
  if ((px->ex_rows ? px->obs || px->filt || px->trail : ex != h->exposures.get()) || ex->nexp != px->nshift || (ex->scale.empty() && ex->smear.empty()) ||
      (!ex->scale.empty() && (ex->scale.size() != (size_t)ex->nexp || !PA.scale || h->d_exscale.bytes < EX.scale_bytes)) ||
      (!ex->smear.empty() && (ex->smear.size() != (size_t)ex->nexp || !PA.smear || h->d_exsmear.bytes < EX.smear_bytes)))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the exposed pixel kernel (not launched)");
  hipLaunchKernelGGL(k_pixel_pairs_exposed, dim3((unsigned)blocks), dim3(kPixBlock), 0, st, PA);
  return TRX_OK;
}

// ---- the high-pass of those pairs along the pixel axis (trx_highpass.hip.h), ahead of the filter, the moments and the
// trail, which then read d_pixhp
static int launch_highpass(trx_handle *h, const PixelRun *px, hipStream_t st)
{
  if (!px || !px->hp) return TRX_OK;
  const HighPassSet &F = *px->hp; const PixelExtents &X = px->ext; const HighpassExtents &HX = px->hpx;
  const ObservedSet *O = F.obs;
  HpArgs HA{};
  HA.pairs = h->d_pixout.as<double2>(); HA.gain = O ? O->d_gain.as<double>() : nullptr; HA.taps = F.d_taps.as<double>();
  HA.tiles = F.d_tiles.as<HpTile>(); HA.out = h->d_pixhp.as<double2>();
  HA.npix = F.npix; HA.ntiles = F.ntiles; HA.den_full = F.den_full; HA.half = F.half;
  const HighpassExtents want_x = highpass_extents(F.npix, px->nshift, F.ntiles, F.half);
  // (every address the kernel reads or writes: pairs in and out over [nshift][npix] -- the tiles lie in [0, npix) within their
  // segments' bounds, made so from the observed set's when the high-pass was --, the gains, the taps [half + 1], the tiles,
  // and (count + 2 half) * 2 doubles of LDS, count <= kHpTile)
  if (!O || O != h->observed.get() || (px->obs && px->obs != O) || !HA.pairs || !HA.taps || !HA.tiles || !HA.out || F.half < 0 || F.half > TRX_HIGHPASS_MAX_HALF ||
      F.npix < 1 || F.npix != px->set->npix || F.npix != O->npix || F.nseg != O->nseg || px->nshift < 1 || F.ntiles < 1 ||
      X.pairs != (int64_t)px->nshift * F.npix || HX.pairs != X.pairs || HX.blocks != want_x.blocks || HX.pair_bytes != want_x.pair_bytes || HX.lds_bytes != want_x.lds_bytes ||
      h->d_pixout.bytes < X.pair_bytes || h->d_pixhp.bytes < HX.pair_bytes || (HA.gain && O->d_gain.bytes < sizeof(double) * (size_t)F.npix) ||
      F.d_taps.bytes < sizeof(double) * ((size_t)F.half + 1) || F.d_tiles.bytes < sizeof(HpTile) * (size_t)F.ntiles ||
      HX.lds_bytes > 65536 || !grid_ok(HX.blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the high-pass kernel (not launched)");
  hipLaunchKernelGGL(k_pixel_highpass, dim3((unsigned)HX.blocks), dim3(kHpBlock), HX.lds_bytes, st, HA);
  return TRX_OK;
}

// ---- the weighted filter of those pairs (trx_wfilter.hip.h), where the plain one runs
static int launch_wfilter(trx_handle *h, const PixelRun &px, hipStream_t st)
{
  const FilterSet &F = *px.filt; const PixelExtents &X = px.ext;
  const ObservedSet *O = px.obs;
  const PairSource P = pair_source(h, px, O);
  WfilterArgs FA{};
  FA.pairs = (double2 *)P.pairs; FA.gain = (double *)P.gain;
  FA.weight = O ? O->d_weight.now.as<double>() : nullptr; FA.basis = F.d_back.as<double>(); FA.fac = F.d_fac.as<double>(); FA.live = F.d_live.as<int32_t>();
  FA.tiles = F.d_tiles.as<FilterTile>(); FA.val = h->d_pixval.as<double>();
  FA.npix = F.npix; FA.ntiles = F.ntiles; FA.nexp = F.nexp; FA.ncomp = F.ncomp;
  int64_t blocks;
  // (every address the kernel reads or writes: pairs and values over [nexp][npix] -- the tiles lie in [0, npix) and name
  // segments below nseg, made so when the filter was --, the gains, and the set's own arrays: wfilter_set_complete)
  if (!O || !P.whole || !FA.val || !wfilter_set_complete(F, *O) || F.npix != px.set->npix || F.nexp != px.nshift ||
      X.pairs != (int64_t)F.nexp * F.npix || X.val_bytes < 1 || h->d_pixval.bytes < X.val_bytes || !blocks_for(FA.ntiles, kFiltWaves, &blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the weighted filter kernel (not launched)");
  LAUNCH_NPAD(k_pixel_wfilter, F.npad, dim3((unsigned)blocks), dim3(64 * kFiltWaves), st, FA);
  return TRX_OK;
}

// ---- the filter of those pairs along the exposure axis (trx_filter.hip.h), ahead of the moment kernel, which then reads
// its values
static int launch_filter(trx_handle *h, const PixelRun *px, hipStream_t st)
{
  if (!px || !px->filt) return TRX_OK;
  if (px->filt->weighted) return launch_wfilter(h, *px, st);
  const FilterSet &F = *px->filt; const PixelExtents &X = px->ext;
  const ObservedSet *O = px->obs;
  const PairSource P = pair_source(h, *px, O);
  FilterArgs FA{};
  FA.pairs = (double2 *)P.pairs; FA.gain = (double *)P.gain;
  FA.fwd = F.d_fwd.as<double>(); FA.back = F.d_back.as<double>(); FA.tiles = F.d_tiles.as<FilterTile>(); FA.val = h->d_pixval.as<double>();
  FA.npix = F.npix; FA.ntiles = F.ntiles; FA.nexp = F.nexp;
  int64_t blocks;
  // (every address the kernel reads or writes: pairs and values over [nexp][npix] -- the tiles lie in [0, npix) and name
  // segments below nseg, made so when the filter was --, the gains, the two padded matrices, the tiles: filter_set_whole)
  if (!O || !P.whole || !FA.val || !filter_set_whole(F, *O) || F.npix != px->set->npix || F.nexp != px->nshift ||
      X.pairs != (int64_t)F.nexp * F.npix || X.val_bytes < 1 || h->d_pixval.bytes < X.val_bytes || !blocks_for(FA.ntiles, kFiltWaves, &blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the filter kernel (not launched)");
  LAUNCH_NPAD(k_pixel_filter, F.npad, dim3((unsigned)blocks), dim3(64 * kFiltWaves), st, FA);
  return TRX_OK;
}

// ---- the trail of those pairs -- one shift per LAG -- against every exposure of the observed set (trx_trail.hip.h)
static int launch_trail(trx_handle *h, const PixelRun &px, hipStream_t st)
{
  const ObservedSet &O = *px.obs; const PixelExtents &X = px.ext;
  constexpr int TL = kTrailLags, TV = kTrailExps;
  const PairSource P = pair_source(h, px, &O);
  TrailArgs TA{};
  TA.pairs = (double2 *)P.pairs; TA.gain = (double *)P.gain;
  TA.data = O.d_data.now.as<double>(); TA.weight = O.d_weight.now.as<double>();
  TA.seg_first = O.d_seg.as<int64_t>(); TA.trail = h->d_trail.as<double>();
  TA.npix = O.npix; TA.nlag = px.nshift; TA.nexp = O.nexp; TA.nseg = O.nseg;
  TA.ntl = (px.nshift + TL - 1) / TL; TA.ntv = (O.nexp + TV - 1) / TV;
  TA.nwaves = (int64_t)O.nseg * TA.ntl * TA.ntv; TA.xcd_map = 1;
  int64_t blocks;
  // (every address the kernel reads or writes: the pairs over [nlag][npix], data and weights over [nexp][npix] -- the segments
  // lie in [0, npix), checked when the set was made, and a ragged tile's surplus indices are nlag - 1 and nexp - 1 --, the
  // gains, the segment bounds: observed_set_whole; the rows of [nlag][nexp][nseg])
  if (!P.whole || !observed_set_whole(O, O.d_weight.now, true) || !TA.trail || px.filt || px.nshift < 1 || O.npix != px.set->npix || !grid_ok(X.rows) ||
      X.pairs != (int64_t)px.nshift * O.npix || X.trail_bytes < 1 || h->d_trail.bytes < X.trail_bytes || !blocks_for(TA.nwaves, kTrailWaves, &blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the trail kernel (not launched)");
  hipLaunchKernelGGL((k_trail_moments<TL, TV>), dim3((unsigned)blocks), dim3(64 * kTrailWaves), 0, st, TA);
  return TRX_OK;
}

// ---- the moments of those pairs (of the filter's values: a filtered run) against the observed set (trx_moments.hip.h).
// (A trail run: its kernel instead.)
static int launch_moments(trx_handle *h, const PixelRun *px, hipStream_t st)
{
  if (!px || !px->obs) return TRX_OK;
  const ObservedSet &O = *px->obs; const PixelExtents &X = px->ext;
  if (px->trail) return launch_trail(h, *px, st);
  const PairSource P = pair_source(h, *px, &O);
  MomArgs MA{};
  MA.val = px->filt ? h->d_pixval.as<double>() : nullptr;
  MA.pairs = (double2 *)P.pairs; MA.gain = (double *)P.gain;
  MA.data = O.d_data.now.as<double>(); MA.weight = O.d_weight.now.as<double>();
  MA.seg_first = O.d_seg.as<int64_t>(); MA.mom = h->d_mom.as<double>();
  MA.npix = O.npix; MA.nseg = O.nseg; MA.nrows = (int64_t)O.nexp * O.nseg;
  int64_t blocks;
  // (every address the kernel reads or writes: pairs, data and weights over [nexp][npix] -- the segments lie in [0, npix),
  // checked when the set was made --, the gains, the segment bounds: observed_set_whole; the rows)
  if (!P.whole || !observed_set_whole(O, O.d_weight.now, true) || !MA.mom || O.npix != px->set->npix || O.nexp != px->nshift ||
      X.pairs != (int64_t)O.nexp * O.npix || X.rows != MA.nrows || h->d_mom.bytes < X.mom_bytes || !blocks_for(MA.nrows, kMomWaves, &blocks) ||
      (px->filt && (!MA.val || X.val_bytes < 1 || h->d_pixval.bytes < X.val_bytes)))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the moment kernel (not launched)");
  if (px->filt) hipLaunchKernelGGL(k_pixel_moments<true>, dim3((unsigned)blocks), dim3(64 * kMomWaves), 0, st, MA);
  else hipLaunchKernelGGL(k_pixel_moments<false>, dim3((unsigned)blocks), dim3(64 * kMomWaves), 0, st, MA);
  return TRX_OK;
}

// ---- what the run makes of this pass's spectrum (want), all of it on the spectrum's queue.  The order is a dependency:
// the bands and contributions read the spectrum and the optical depths only, but the broadening writes d_broad, which the
// pixels then sample; the high-pass reads the pixels' pairs and writes its own, which stand in for them from there on; the
// filter reads the pairs; the moments (or the trail) read the pairs or the filter's values.
int Run::product_kernels()
{
  int rc;
  if ((rc = launch_bands(h, want.bs, d_out, tst))) return rc;
  if (want.contrib) {
    EmisArgs E{};
    if (vertical) emis_args(E);
    else {                                             // (transit geometry: the grid, tau and last; no angles)
      E.nr = nr; E.nang = 0; E.nsh = nsh; E.lo = h->lo; E.wn_i = h->wn_i; E.wn_d = h->wn_d; E.wn_fct = o->wn_fct;
      E.tau = h->d_tau.as<double>(); E.last = h->d_last.as<int>(); E.temp = d_tempk; E.e2tab = h->d_e2tab.as<double>();
    }
    if ((rc = launch_contrib(h, want.bs, E, vertical, tst))) return rc;
  }
  return (rc = launch_broaden(h, want.br, d_out, nsh, tst)) || (rc = launch_pixels(h, want.px, want.br ? h->d_broad.as<double>() : d_out, nsh, tst)) ||
         (rc = launch_highpass(h, want.px, tst)) || (rc = launch_filter(h, want.px, tst)) || (rc = launch_moments(h, want.px, tst)) ? rc : TRX_OK;
}

}  // namespace

// ---- the run products: their checks, layouts and extents are ../trx_products.h's; here they meet the handle and the device
// what that header's checks need to know of h
static ProductState product_state(const trx_handle *h)
{
  ProductState S;
  S.windowed = h->windowed(); S.wn_i = h->wn_i; S.wn_d = h->wn_d; S.nwn = h->nwn; S.lo = h->lo; S.hi = h->hi;
  if (h->pixels) S.npix = h->pixels->npix;
  if (h->observed) { S.nexp = h->observed->nexp; S.nseg = h->observed->nseg; S.seg = h->observed->seg.data(); }
  S.filter = h->filter != nullptr; S.highpass = h->highpass != nullptr; S.exposures = h->exposures != nullptr;
  return S;
}

// ---- band integrals (trx_bands.hip.h) -------------------------------------------------------------
// The set as h's shard sees it (band_layout), checked whole before anything is replaced.
static int make_band_set(trx_handle *h, int32_t nbands, const trx_band *bands, std::unique_ptr<BandSet> &out)
{
  out.reset();
  std::string msg; BandLayout L;
  if (const int rc = band_layout(product_state(h), nbands, bands, L, msg)) return fail(h, rc, msg);
  if (nbands == 0) return TRX_OK;                       // (clear)
  std::unique_ptr<BandSet> S(new (std::nothrow) BandSet);
  if (!S) return fail(h, TRX_E_NOMEM, "bands: out of host memory");
  S->nbands = nbands; S->npieces = (int64_t)L.pieces.size();
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload(h, S->d_bands, L.bands)) || (rc = upload(h, S->d_pieces, L.pieces)) ||
      (rc = upload(h, S->d_w, L.w)) || (rc = ensure(h, S->d_part, sizeof(double) * 2 * (size_t)S->npieces)) ||
      (rc = ensure_pinned(h, S->h_out, sizeof(double) * 2 * (size_t)nbands)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (the caller's arrays may go once this returns)
  out = std::move(S);
  return TRX_OK;
}

static void install_band_set(trx_handle *h, std::unique_ptr<BandSet> &S) { h->bands = std::move(S); }

int trx_set_bands(trx_handle *h, int32_t nbands, const trx_band *bands)
{
  if (!h) return TRX_E_ARG;
  std::unique_ptr<BandSet> S;
  if (const int rc = make_band_set(h, nbands, bands, S)) return rc;
  install_band_set(h, S);
  return TRX_OK;
}

int trx_run_bands(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, double *sums, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  if (!h->bands) return fail(h, TRX_E_ARG, "trx_run_bands: no band set installed (trx_set_bands)");
  if (!sums) return fail(h, TRX_E_ARG, "trx_run_bands: sums is NULL");
  Products want; want.bs = h->bands.get();
  const int rc = run_once(h, a, o, spectrum, nullptr, dbg, want);
  if (rc == TRX_OK) std::memcpy(sums, h->bands->h_out.p, sizeof(double) * 2 * (size_t)h->bands->nbands);
  return rc;
}

// ---- contribution functions per band and layer (trx_contrib.hip.h) --------------------------------
int trx_run_contrib(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, double *sums, double *contrib, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  if (!h->bands) return fail(h, TRX_E_ARG, "trx_run_contrib: no band set installed (trx_set_bands)");
  if (!sums) return fail(h, TRX_E_ARG, "trx_run_contrib: sums is NULL");
  if (!contrib) return fail(h, TRX_E_ARG, "trx_run_contrib: contrib is NULL");
  if (!a || !o) return TRX_E_ARG;
  if (a->nlayer < 1) return fail(h, TRX_E_ARG, "trx_run_contrib: nlayer < 1");
  const BandSet *bs = h->bands.get();
  const ContribExtents X = contrib_extents(a->nlayer, bs->npieces, bs->nbands);
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = ensure(h, h->d_cpart, X.cpart_bytes)) || (rc = ensure_pinned(h, h->h_contrib, X.out_bytes))) return rc;
  Products want; want.bs = bs; want.contrib = true;
  rc = run_once(h, a, o, spectrum, nullptr, dbg, want);
  if (rc == TRX_OK) {
    std::memcpy(sums, bs->h_out.p, sizeof(double) * 2 * (size_t)bs->nbands);
    std::memcpy(contrib, h->h_contrib.p, X.out_bytes);
  }
  return rc;
}

// ---- detector pixels at Doppler shifts (trx_pixels.hip.h) ------------------------------------------
// The set, checked whole before anything is replaced; the device gets the arrays as they are.
static int make_pixel_set(trx_handle *h, const trx_pixels *px, std::unique_ptr<PixelSet> &out)
{
  out.reset();
  if (!px || px->npix == 0) return TRX_OK;              // (clear)
  std::string msg;
  if (const int rc = pixel_set_checks(px, msg)) return fail(h, rc, msg);
  std::unique_ptr<PixelSet> S(new (std::nothrow) PixelSet);
  if (!S) return fail(h, TRX_E_NOMEM, "pixels: out of host memory");
  S->npix = px->npix; S->cut = px->cut;
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload_raw(h, S->d_centre, px->centre, (size_t)px->npix)) || (rc = upload_raw(h, S->d_fwhm, px->fwhm, (size_t)px->npix))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (the caller's arrays may go once this returns)
  out = std::move(S);
  return TRX_OK;
}

// (the observed set belongs to the pixel set it was installed over, the filter, the high-pass and the exposure table to the
// observed set, and so does the recipe of trx_set_normalise: they go with it -- the high-pass first, which points into the
// observed set)
static void install_pixel_set(trx_handle *h, std::unique_ptr<PixelSet> &S) { h->highpass.reset(); h->pixels = std::move(S); h->observed.reset(); h->filter.reset(); h->exposures.reset(); h->norm_on = false; }
static void install_observed_set(trx_handle *h, std::unique_ptr<ObservedSet> &S) { h->highpass.reset(); h->observed = std::move(S); h->filter.reset(); h->exposures.reset(); h->norm_on = false; }

int trx_set_pixels(trx_handle *h, const trx_pixels *px)
{
  if (!h) return TRX_E_ARG;
  std::unique_ptr<PixelSet> S;
  if (const int rc = make_pixel_set(h, px, S)) return rc;
  install_pixel_set(h, S);
  return TRX_OK;
}

// the pixel run PR for `who` (trx_run_pixels; PR.obs: trx_run_moments; PR.filt: trx_run_filtered_moments; PR.trail: trx_run_trail,
// the shifts its lags; PR.hp: trx_run_highpassed) at PR.nshift shifts: the pairs are in h->d_pixout, the moments in h->d_mom,
// the filtered values in h->d_pixval, the trail in h->d_trail, when it returns -- each over its extent in PR.ext --, the
// high-passed pairs (a run with PR.hp, given or taken from the handle here) in h->d_pixhp over PR.hpx
static int pixel_run(trx_handle *h, const char *who, const trx_atm *a, const trx_opts *o, double *spectrum, PixelRun &PR, const double *shift,
                     trx_debug *dbg)
{
  std::string msg;
  if (const int rc = pixel_run_checks(who, PR.nshift, PR.set->npix, shift, msg)) return fail(h, rc, msg);
  const PixelExtents &X = PR.ext = pixel_extents(PR.set->npix, PR.nshift, PR.obs ? PR.obs->nexp : 0, PR.obs ? PR.obs->nseg : 0, PR.filt != nullptr, PR.trail);
  // (every run against the observed set takes the high-pass installed over it)
  if (PR.obs && h->highpass) PR.hp = h->highpass.get();
  if (PR.hp) PR.hpx = highpass_extents(PR.hp->npix, PR.nshift, PR.hp->ntiles, PR.hp->half);
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  // (the shifts go ahead of the run's own inputs on its main queue; every queue of the run waits for those)
  if ((rc = ensure(h, h->d_pixout, X.pair_bytes)) || (X.mom_bytes && (rc = ensure(h, h->d_mom, X.mom_bytes))) ||
      (X.trail_bytes && (rc = ensure(h, h->d_trail, X.trail_bytes))) || (X.val_bytes && (rc = ensure(h, h->d_pixval, X.val_bytes))) ||
      (PR.hp && (rc = ensure(h, h->d_pixhp, PR.hpx.pair_bytes))) ||
      (h->broad_on && (rc = ensure(h, h->d_broad, broadened_bytes(h->nwn)))) ||
      (rc = upload_raw(h, h->d_pixshift, shift, (size_t)PR.nshift)))
    return rc;
  // (the exposure table with them: it changes from call to call, as the shifts do)
  if (PR.ex && ((!PR.ex->scale.empty() && (rc = upload(h, h->d_exscale, PR.ex->scale))) || (!PR.ex->smear.empty() && (rc = upload(h, h->d_exsmear, PR.ex->smear)))))
    return rc;
  // (with a broadening installed the pixels sample the broadened spectrum)
  Products want; want.px = &PR; if (h->broad_on) want.br = &h->broad;
  return run_once(h, a, o, spectrum, nullptr, dbg, want);
}

int trx_run_pixels(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift,
                   double *out, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  if (!h->pixels) return fail(h, TRX_E_ARG, "trx_run_pixels: no pixel set installed (trx_set_pixels)");
  if (nshift < 1) return fail(h, TRX_E_ARG, "trx_run_pixels: nshift < 1");
  if (!shift) return fail(h, TRX_E_ARG, "trx_run_pixels: shift is NULL");
  if (!out) return fail(h, TRX_E_ARG, "trx_run_pixels: out is NULL");
  PixelRun PR{h->pixels.get(), nshift};
  if (const int rc = pixel_run(h, "trx_run_pixels", a, o, spectrum, PR, shift, dbg)) return rc;
  HIPCHK(h, hipMemcpy(out, h->d_pixout.p, PR.ext.pair_bytes, hipMemcpyDeviceToHost));      // (the run has been waited for)
  return TRX_OK;
}

// ---- cross-correlation moments of the pixels against observed data (trx_moments.hip.h) -------------
// The set, checked whole before anything is replaced; the device gets the arrays as they are.
static int make_observed_set(trx_handle *h, const trx_observed *ob, std::unique_ptr<ObservedSet> &out)
{
  out.reset();
  if (!ob || ob->nexp == 0) return TRX_OK;              // (clear)
  std::string msg;
  if (const int rc = observed_set_checks(product_state(h), ob, msg)) return fail(h, rc, msg);
  const int64_t npix = h->pixels->npix;
  const size_t cells = (size_t)ob->nexp * (size_t)npix;
  std::unique_ptr<ObservedSet> S(new (std::nothrow) ObservedSet);
  if (!S) return fail(h, TRX_E_NOMEM, "observed: out of host memory");
  S->nexp = ob->nexp; S->nseg = ob->nseg; S->npix = npix;
  try { S->seg.assign(ob->seg_first, ob->seg_first + ob->nseg + 1); } catch (...) { return fail(h, TRX_E_NOMEM, "observed: out of host memory"); }
  if (ob->weight) for (size_t k = 0; k < cells; k++) S->ndead += ob->weight[k] > 0.0 ? 0 : 1;
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload_raw(h, S->d_seg, ob->seg_first, (size_t)ob->nseg + 1)) || (rc = upload_raw(h, S->d_data.now, ob->data, cells)) ||
      (ob->weight && (rc = upload_raw(h, S->d_weight.now, ob->weight, cells))) || (ob->gain && (rc = upload_raw(h, S->d_gain, ob->gain, (size_t)npix))))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (the caller's arrays may go once this returns)
  out = std::move(S);
  return TRX_OK;
}

int trx_set_observed(trx_handle *h, const trx_observed *ob)
{
  if (!h) return TRX_E_ARG;
  std::unique_ptr<ObservedSet> S;
  if (const int rc = make_observed_set(h, ob, S)) return rc;
  install_observed_set(h, S);
  return TRX_OK;
}

int trx_run_moments(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift,
                    double *mom, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  std::string msg;
  if (const int rc = observed_run_checks(product_state(h), "trx_run_moments", ObservedRun::Moments, nshift, shift, mom, "mom", msg)) return fail(h, rc, msg);
  PixelRun PR{h->pixels.get(), nshift, h->observed.get()}; PR.ex = h->exposures.get();
  if (const int rc = pixel_run(h, "trx_run_moments", a, o, spectrum, PR, shift, dbg)) return rc;
  HIPCHK(h, hipMemcpy(mom, h->d_mom.p, PR.ext.mom_bytes, hipMemcpyDeviceToHost));      // (the run has been waited for)
  return TRX_OK;
}

// ---- the exposure table: a scale and a Doppler smear per exposure, in the pixel stage (trx_pixels.hip.h) ----
// The table as h would keep it, checked whole before anything is replaced (null: a clearing call); the arrays stay on the host.
static int make_exposure_set(trx_handle *h, const trx_exposures *ex, std::unique_ptr<ExposureSet> &out)
{
  out.reset();
  if (!ex || ex->nexp == 0) return TRX_OK;              // (clear)
  std::string msg;
  if (const int rc = exposure_set_checks(product_state(h), ex, msg)) return fail(h, rc, msg);
  std::unique_ptr<ExposureSet> S(new (std::nothrow) ExposureSet);
  if (!S) return fail(h, TRX_E_NOMEM, "exposures: out of host memory");
  S->nexp = ex->nexp;
  try {
    if (ex->scale) S->scale.assign(ex->scale, ex->scale + ex->nexp);
    if (ex->smear) S->smear.assign(ex->smear, ex->smear + ex->nexp);
  } catch (...) { return fail(h, TRX_E_NOMEM, "exposures: out of host memory"); }
  out = std::move(S);
  return TRX_OK;
}

int trx_set_exposures(trx_handle *h, const trx_exposures *ex)
{
  if (!h) return TRX_E_ARG;
  std::unique_ptr<ExposureSet> S;
  if (const int rc = make_exposure_set(h, ex, S)) return rc;
  h->exposures = std::move(S);
  return TRX_OK;
}

int trx_run_exposed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift,
                    double *out, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  std::string msg;
  if (const int rc = exposed_run_checks(product_state(h), "trx_run_exposed", nshift, shift, out, msg)) return fail(h, rc, msg);
  // (the pairs alone: no moments, and no high-pass -- a run of the pixel stage, as trx_run_pixels is)
  PixelRun PR{h->pixels.get(), nshift}; PR.ex = h->exposures.get();
  if (const int rc = pixel_run(h, "trx_run_exposed", a, o, spectrum, PR, shift, dbg)) return rc;
  HIPCHK(h, hipMemcpy(out, h->d_pixout.p, PR.ext.pair_bytes, hipMemcpyDeviceToHost));      // (the run has been waited for)
  return TRX_OK;
}

// ---- the cross-correlation trail: every exposure against every lag of a grid (trx_trail.hip.h) -----
int trx_run_trail(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nlag, const double *lag,
                  double *trail, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  std::string msg;
  if (const int rc = trail_run_checks(product_state(h), "trx_run_trail", nlag, lag, trail, "trail", msg)) return fail(h, rc, msg);
  // (an installed filter takes no part: it couples the exposures, and a trail's model is the same at all of them)
  PixelRun PR{h->pixels.get(), nlag, h->observed.get()}; PR.trail = true;
  if (const int rc = pixel_run(h, "trx_run_trail", a, o, spectrum, PR, lag, dbg)) return rc;
  HIPCHK(h, hipMemcpy(trail, h->d_trail.p, PR.ext.trail_bytes, hipMemcpyDeviceToHost));      // (the run has been waited for)
  return TRX_OK;
}

// ---- the Kp-Vsys map of that trail, reduced on the device (trx_vmap.hip.h) --------------------------
// the statistic of PR's trail (in h->d_trail, the run waited for) and the map of it, behind the upload of the call's arrays
// on the main queue: X their extents, the arrays at X.at_* of h->d_vm_in
static int launch_velocity_map(trx_handle *h, const PixelRun &PR, const trx_vmap *vm, const VmapExtents &X)
{
  const ObservedSet *ob = PR.obs;
  const double *in = h->d_vm_in.as<double>();
  TrailStatArgs SA{};
  SA.trail = h->d_trail.as<double>(); SA.per_lv = h->d_vm_per.as<double>(); SA.per_vl = SA.per_lv + X.rows;
  SA.nrows = (int64_t)X.rows; SA.nlag = vm->nlag; SA.nexp = ob->nexp; SA.nseg = ob->nseg; SA.stat = vm->stat; SA.p0 = vm->p0; SA.p1 = vm->p1;
  VelMapArgs MA{};
  MA.per_vl = SA.per_vl; MA.lag_kms = in; MA.kp = in + X.at_kp; MA.vsys = in + X.at_vsys; MA.orbit = in + X.at_orbit; MA.offset = vm->offset ? in + X.at_offset : nullptr;
  MA.map = h->d_vm_map.as<double>(); MA.ncells = (int64_t)X.cells; MA.nlag = vm->nlag; MA.nexp = ob->nexp; MA.nvsys = vm->nvsys;
  int64_t sblocks, mblocks;
  // (every address the kernels read or write: the trail rows [nlag][nexp][nseg], the statistic twice over [nlag][nexp], the
  // call's arrays -- a cell's lag indices lie in [0, nlag - 1], vmap_locate --, the cells)
  if (!SA.trail || !SA.per_lv || !in || !MA.map || X.rows < 1 || X.cells < 1 || ob->nseg < 1 ||
      PR.ext.rows != SA.nrows * ob->nseg || h->d_trail.bytes < PR.ext.trail_bytes || h->d_vm_per.bytes < X.per2_bytes ||
      h->d_vm_in.bytes < X.in_bytes || h->d_vm_map.bytes < X.map_bytes ||
      !blocks_for(SA.nrows, kVmapWaves, &sblocks) || !blocks_for(MA.ncells, kVmapWaves, &mblocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the map kernels (not launched)");
  hipLaunchKernelGGL(k_trail_stat, dim3((unsigned)sblocks), dim3(64 * kVmapWaves), 0, h->stream, SA);
  hipLaunchKernelGGL(k_velocity_map, dim3((unsigned)mblocks), dim3(64 * kVmapWaves), 0, h->stream, MA);
  HIPCHK(h, hipGetLastError());
  return TRX_OK;
}

int trx_run_velocity_map(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, const trx_vmap *vm, double *map, double *per,
                         trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_run_velocity_map";
  std::string msg;
  if (const int rc = velocity_map_checks(product_state(h), who, vm, map, msg)) return fail(h, rc, msg);
  const VmapExtents X = vmap_extents(*vm, h->observed->nexp);
  if (const int rc = vmap_pack(who, *vm, X, h->vm_in, msg)) return fail(h, rc, msg);
  // the trail of the lags into d_trail, as trx_run_trail leaves it; it stays there
  PixelRun PR{h->pixels.get(), vm->nlag, h->observed.get()}; PR.trail = true;
  if (const int rc = pixel_run(h, who, a, o, spectrum, PR, vm->lag, dbg)) return rc;
  int rc;
  // (the run has been waited for: the two kernels follow the upload on the main queue)
  if ((rc = ensure(h, h->d_vm_per, X.per2_bytes)) || (rc = ensure(h, h->d_vm_map, X.map_bytes)) || (rc = upload(h, h->d_vm_in, h->vm_in)) ||
      (rc = launch_velocity_map(h, PR, vm, X)))
    return rc;
  HIPCHK(h, hipMemcpyAsync(map, h->d_vm_map.p, X.map_bytes, hipMemcpyDeviceToHost, h->stream));
  if (per) HIPCHK(h, hipMemcpyAsync(per, h->d_vm_per.p, X.per_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TRX_OK;
}

// ---- the detrending filter between the pairs and the moments (trx_filter.hip.h) ---------------------
// The filter, checked whole before anything is replaced; the device gets filter_layout's matrices and tiles.
static int make_filter_set(trx_handle *h, const trx_filter *f, std::unique_ptr<FilterSet> &out)
{
  out.reset();
  if (!f || f->ncomp == 0) return TRX_OK;               // (clear)
  const ProductState P = product_state(h);
  std::string msg; FilterLayout L;
  if (const int rc = filter_set_checks(P, f, msg)) return fail(h, rc, msg);
  std::unique_ptr<FilterSet> S(new (std::nothrow) FilterSet);
  if (!S) return fail(h, TRX_E_NOMEM, "filter: out of host memory");
  if (const int rc = filter_layout(P, f, L, msg)) return fail(h, rc, msg);
  S->ncomp = f->ncomp; S->npad = L.npad; S->nexp = P.nexp; S->nseg = P.nseg; S->npix = P.npix; S->ntiles = (int64_t)L.tiles.size();
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload(h, S->d_fwd, L.fwd)) || (rc = upload(h, S->d_back, L.back)) || (rc = upload(h, S->d_tiles, L.tiles))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (the staging vectors go when this returns)
  out = std::move(S);
  return TRX_OK;
}

static void install_filter_set(trx_handle *h, std::unique_ptr<FilterSet> &S) { h->filter = std::move(S); }

int trx_set_filter(trx_handle *h, const trx_filter *f)
{
  if (!h) return TRX_E_ARG;
  std::unique_ptr<FilterSet> S;
  if (const int rc = make_filter_set(h, f, S)) return rc;
  install_filter_set(h, S);
  return TRX_OK;
}

// Every column's factor and pivot flag of the weighted filter S over the observed set O against `weight` ([nexp][npix] of
// weight_bytes, or null: all 1), into fac and live (grown to size): k_wfilter_factor from S's own basis and tiles, which are
// on the device.  The flags come back once for the count of the singular columns.  trx_set_weighted_filter installs with
// it; trx_weigh_observed makes an installed filter's factor again against other weights, in buffers of its own.
static int factor_wfilter(trx_handle *h, const FilterSet &S, const ObservedSet *O, const double *weight, size_t weight_bytes, DevBuf &fac, DevBuf &live,
                          int64_t *nsingular)
{
  if (nsingular) *nsingular = 0;
  const WfilterExtents WX = wfilter_extents(S.npix, S.nexp, S.nseg, S.ncomp, S.npad, S.ntiles, kFiltWaves);
  std::vector<int32_t> flags;
  try { flags.assign((size_t)S.npix, 0); } catch (...) { return fail(h, TRX_E_NOMEM, "weighted filter: out of host memory"); }
  int rc;
  if ((rc = ensure(h, fac, WX.fac_bytes)) || (rc = ensure(h, live, WX.live_bytes))) return rc;
  // (a pixel outside every tile -- none: the segments cover [0, npix) -- would keep a zero factor and a zero flag)
  HIPCHK(h, hipMemsetAsync(fac.p, 0, WX.fac_bytes, h->stream));
  HIPCHK(h, hipMemsetAsync(live.p, 0, WX.live_bytes, h->stream));
  WfilterFactorArgs A{};
  A.weight = weight; A.basis = S.d_back.as<double>(); A.tiles = S.d_tiles.as<FilterTile>();
  A.fac = fac.as<double>(); A.live = live.as<int32_t>(); A.npix = S.npix; A.ntiles = S.ntiles; A.nexp = S.nexp; A.ncomp = S.ncomp;
  // (every address the kernel reads or writes: the padded basis, the tiles -- the segments cover [0, npix): at least one --,
  // the weights, the factor and the flags)
  if (!O || !wfilter_basis_whole(S, *O, WX) || (weight && weight_bytes < sizeof(double) * (size_t)S.nexp * (size_t)S.npix) ||
      fac.bytes < WX.fac_bytes || live.bytes < WX.live_bytes || !grid_ok(WX.blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the weighted filter's factor kernel (not launched)");
  LAUNCH_NPAD(k_wfilter_factor, S.npad, dim3((unsigned)WX.blocks), dim3(64 * kFiltWaves), h->stream, A);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(flags.data(), live.p, WX.live_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (the staging vector goes when this returns)
  if (nsingular) for (int32_t x : flags) *nsingular += x ? 0 : 1;
  return TRX_OK;
}

// The weighted filter (trx_wfilter.hip.h), checked whole before anything is replaced: the device gets wfilter_layout's basis
// and tiles, and factor_wfilter makes every column's factor and flag from them and the weights w -- null: the observed
// set's weights in force (trx_set_weighted_filter); trx_detrend_observed gives the weights as trx_set_observed installed them.
static int make_wfilter_set(trx_handle *h, const trx_wfilter *f, std::unique_ptr<FilterSet> &out, int64_t *nsingular, const DevBuf *w = nullptr)
{
  out.reset();
  if (nsingular) *nsingular = 0;
  if (!f || f->ncomp == 0) return TRX_OK;               // (clear)
  const ProductState P = product_state(h);
  std::string msg; WfilterLayout L;
  if (const int rc = wfilter_set_checks(P, f, msg)) return fail(h, rc, msg);
  std::unique_ptr<FilterSet> S(new (std::nothrow) FilterSet);
  if (!S) return fail(h, TRX_E_NOMEM, "weighted filter: out of host memory");
  if (const int rc = wfilter_layout(P, f, L, msg)) return fail(h, rc, msg);
  S->weighted = true;
  S->ncomp = f->ncomp; S->npad = L.npad; S->nexp = P.nexp; S->nseg = P.nseg; S->npix = P.npix; S->ntiles = (int64_t)L.tiles.size();
  S->nfac = wfilter_extents(S->npix, S->nexp, S->nseg, S->ncomp, S->npad, S->ntiles, kFiltWaves).nfac;
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload(h, S->d_back, L.basis)) || (rc = upload(h, S->d_tiles, L.tiles))) return rc;
  const ObservedSet *O = h->observed.get();
  if (!w && O) w = &O->d_weight.now;
  // (factor_wfilter waits for the queue: the staging vectors may go when it returns)
  if ((rc = factor_wfilter(h, *S, O, w ? w->as<double>() : nullptr, w ? w->bytes : 0, S->d_fac, S->d_live, nsingular))) return rc;
  out = std::move(S);
  return TRX_OK;
}

int trx_set_weighted_filter(trx_handle *h, const trx_wfilter *f, int64_t *nsingular)
{
  if (!h) return TRX_E_ARG;
  std::unique_ptr<FilterSet> S;
  if (const int rc = make_wfilter_set(h, f, S, nsingular)) return rc;
  install_filter_set(h, S);
  return TRX_OK;
}

int trx_run_filtered_moments(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift,
                             double *values, double *mom, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  std::string msg;
  if (const int rc = observed_run_checks(product_state(h), "trx_run_filtered_moments", ObservedRun::Filtered, nshift, shift, mom, "mom", msg)) return fail(h, rc, msg);
  PixelRun PR{h->pixels.get(), nshift, h->observed.get(), h->filter.get()}; PR.ex = h->exposures.get();
  if (const int rc = pixel_run(h, "trx_run_filtered_moments", a, o, spectrum, PR, shift, dbg)) return rc;
  // (the run has been waited for)
  HIPCHK(h, hipMemcpy(mom, h->d_mom.p, PR.ext.mom_bytes, hipMemcpyDeviceToHost));
  if (values) HIPCHK(h, hipMemcpy(values, h->d_pixval.p, PR.ext.val_bytes, hipMemcpyDeviceToHost));
  return TRX_OK;
}

// ---- the high-pass between the pairs and whatever reads them (trx_highpass.hip.h) -------------------
// The high-pass, checked whole before anything is replaced; the device gets highpass_layout's taps and tiles.
static int make_highpass_set(trx_handle *h, const trx_highpass *hp, std::unique_ptr<HighPassSet> &out)
{
  out.reset();
  if (!hp || !hp->taps) return TRX_OK;                  // (clear)
  const ProductState P = product_state(h);
  std::string msg; HighpassLayout L;
  if (const int rc = highpass_set_checks(P, hp, msg)) return fail(h, rc, msg);
  std::unique_ptr<HighPassSet> S(new (std::nothrow) HighPassSet);
  if (!S) return fail(h, TRX_E_NOMEM, "highpass: out of host memory");
  if (const int rc = highpass_layout(P, hp, L, msg)) return fail(h, rc, msg);
  S->half = L.half; S->nseg = P.nseg; S->npix = P.npix; S->ntiles = (int64_t)L.tiles.size(); S->den_full = L.den_full; S->obs = h->observed.get();
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = upload(h, S->d_taps, L.taps)) || (rc = upload(h, S->d_tiles, L.tiles))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (the staging vectors go when this returns)
  out = std::move(S);
  return TRX_OK;
}

static void install_highpass_set(trx_handle *h, std::unique_ptr<HighPassSet> &S) { h->highpass = std::move(S); }

int trx_set_highpass(trx_handle *h, const trx_highpass *hp)
{
  if (!h) return TRX_E_ARG;
  std::unique_ptr<HighPassSet> S;
  if (const int rc = make_highpass_set(h, hp, S)) return rc;
  install_highpass_set(h, S);
  return TRX_OK;
}

int trx_run_highpassed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift,
                       double *values, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  std::string msg;
  if (const int rc = observed_run_checks(product_state(h), "trx_run_highpassed", ObservedRun::Highpassed, nshift, shift, values, "values", msg)) return fail(h, rc, msg);
  // (no moments: the observed set only lends the high-pass its segments and gains)
  PixelRun PR{h->pixels.get(), nshift}; PR.hp = h->highpass.get();
  if (const int rc = pixel_run(h, "trx_run_highpassed", a, o, spectrum, PR, shift, dbg)) return rc;
  // (the run has been waited for) the pairs whole -- into pinned memory grown once the run's checks have passed its size --,
  // then their first components: (g', 1) is g', (0, 0) is a dead pixel
  if (const int rc = ensure_pinned(h, h->h_pixhp, PR.hpx.pair_bytes)) return rc;
  HIPCHK(h, hipMemcpy(h->h_pixhp.p, h->d_pixhp.p, PR.hpx.pair_bytes, hipMemcpyDeviceToHost));
  const double *const ab = (const double *)h->h_pixhp.p; const double nan = __builtin_nan("");
  for (int64_t k = 0; k < PR.hpx.pairs; k++) values[k] = ab[2 * k + 1] > 0.0 ? ab[2 * k] : nan;
  return TRX_OK;
}

// ---- the Kp-Vsys map with the filter applied to every cell's own model matrix (trx_cellmap.hip.h) ---
// the index table of the call's cells (k_cell_tracks) into h->d_cm_index, behind the upload of the call's arrays on the main
// queue.  VX: the extents of the call's arrays at VX.at_* of h->d_vm_in; CX: those of the cell buffers.
static int launch_cell_tracks(trx_handle *h, const trx_vmap *vm, const VmapExtents &VX, const CellMapExtents &CX)
{
  const ObservedSet *O = h->observed.get();
  const double *in = h->d_vm_in.as<double>();
  if (!O || !in) return fail(h, TRX_E_HIP, "internal: incomplete arguments for the cell track kernel (not launched)");
  const int32_t nlag = vm->nlag, nexp = O->nexp;
  CellTrackArgs TA{};
  TA.lag_kms = in; TA.kp = in + VX.at_kp; TA.vsys = in + VX.at_vsys; TA.orbit = in + VX.at_orbit; TA.offset = vm->offset ? in + VX.at_offset : nullptr;
  TA.index = h->d_cm_index.as<int32_t>(); TA.ntracks = CX.tracks; TA.nlag = nlag; TA.nexp = nexp; TA.nvsys = vm->nvsys;
  // (every address the kernel reads or writes: the call's arrays -- a track's cell below nkp * nvsys, its exposure below
  // nexp --, the bisection inside lag_kms [nlag], the table over [cells][nexp])
  if (!TA.index || nlag < 1 || nexp < 1 || vm->nvsys < 1 || vm->nkp < 1 || CX.cells != (int64_t)vm->nkp * vm->nvsys || (int64_t)VX.cells != CX.cells ||
      CX.tracks != CX.cells * nexp || CX.tracks > 0x7fffffffLL || h->d_vm_in.bytes < VX.in_bytes || VX.at_kp != (size_t)nlag ||
      VX.at_offset - VX.at_orbit != (size_t)nexp || h->d_cm_index.bytes < CX.index_bytes || CX.index_bytes < sizeof(int32_t) * (size_t)CX.tracks ||
      !grid_ok(CX.track_blocks) || CX.track_blocks * kCellTrackBlock < CX.tracks)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the cell track kernel (not launched)");
  hipLaunchKernelGGL(k_cell_tracks, dim3((unsigned)CX.track_blocks), dim3(kCellTrackBlock), 0, h->stream, TA);
  return TRX_OK;
}

// chunk after chunk the filter, the moments and the statistic of the cells, each cell's rows of PR's pairs named by its
// entries of `table` [cells][nexp]: the lag table (trx_run_filtered_map: nrow = nlag rows) or the row table of an exposed
// map (nrow = R rows), every entry -1 or in [0, nrow)
static int launch_cell_chunks(trx_handle *h, const PixelRun &PR, const trx_vmap *vm, const CellMapExtents &CX, const DevBuf &table, int64_t nrow)
{
  const ObservedSet *O = h->observed.get(); const FilterSet *F = h->filter.get();
  if (!O || !F || !table.p || table.bytes < CX.index_bytes || CX.index_bytes < sizeof(int32_t) * (size_t)CX.tracks)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the cell map kernels (not launched)");
  const int32_t nexp = O->nexp, nseg = O->nseg;
  const int64_t npix = O->npix;
  const int32_t *const index = table.as<int32_t>();
  CellFilterArgs FA{};
  const PairSource P = pair_source(h, PR, O);
  FA.pairs = (double2 *)P.pairs; FA.gain = (double *)P.gain;
  FA.fwd = F->d_fwd.as<double>(); FA.back = F->d_back.as<double>(); FA.tiles = F->d_tiles.as<FilterTile>(); FA.val = h->d_cm_val.as<double>();
  FA.npix = npix; FA.ntiles = F->ntiles; FA.nexp = nexp;
  // (a weighted filter: k_cell_wfilter in k_cell_filter's place, over the same pairs, tiles, index rows and values)
  const bool wt = F->weighted;
  WfilterArgs WA{};
  WA.pairs = FA.pairs; WA.gain = FA.gain; WA.weight = O->d_weight.now.as<double>(); WA.basis = FA.back; WA.fac = F->d_fac.as<double>();
  WA.live = F->d_live.as<int32_t>(); WA.tiles = FA.tiles; WA.val = FA.val; WA.npix = npix; WA.ntiles = F->ntiles; WA.nexp = nexp; WA.ncomp = F->ncomp;
  CellMomArgs MA{};
  MA.val = FA.val; MA.data = O->d_data.now.as<double>(); MA.weight = O->d_weight.now.as<double>(); MA.seg_first = O->d_seg.as<int64_t>();
  MA.mom = h->d_cm_mom.as<double>(); MA.npix = npix; MA.nexp = nexp; MA.nseg = nseg;
  CellStatArgs SA{};
  SA.mom = MA.mom; SA.nexp = nexp; SA.nseg = nseg; SA.stat = vm->stat; SA.p0 = vm->p0; SA.p1 = vm->p1;
  const size_t obs_cells = sizeof(double) * (size_t)nexp * (size_t)npix;
  int64_t fblocks;
  // (every address the three kernels read or write, for the largest chunk: the pairs over [nrow][npix] -- a table entry the
  // filter follows lies in [0, nrow - 1], vmap_nearest or exposed_map_row, and a cell with a -1 is left out by all three --, the tiles in
  // [0, npix) naming segments below nseg, made so when the filter was, the gains, the two padded matrices; the values over
  // [chunk][nexp][npix]; data and weights over [nexp][npix], the segments in [0, npix), checked when the set was made; the
  // moment rows over [chunk][nexp][nseg]; the chunk's cells of the map)
  if (!(wt ? wfilter_set_complete(*F, *O) : filter_set_whole(*F, *O)) || !P.whole || !observed_set_whole(*O, O->d_weight.now, true) ||
      !FA.val || !MA.mom || !h->d_cm_map.p || npix != PR.set->npix || nrow < 1 || PR.nshift != nrow || PR.filt || PR.trail || PR.obs ||
      PR.ext.pairs != nrow * npix || CX.chunk < 1 || CX.nchunks < 1 || CX.last_chunk < 1 || CX.last_chunk > CX.chunk || (CX.nchunks - 1) * CX.chunk + CX.last_chunk != CX.cells ||
      CX.rows != CX.chunk * nexp * nseg || CX.rows > 0x7fffffffLL ||
      CX.val_bytes < obs_cells * (size_t)CX.chunk || h->d_cm_val.bytes < CX.val_bytes ||
      CX.mom_bytes < sizeof(double) * TRX_NMOMENT * (size_t)CX.rows || h->d_cm_mom.bytes < CX.mom_bytes ||
      CX.map_bytes < sizeof(double) * (size_t)CX.cells || h->d_cm_map.bytes < CX.map_bytes ||
      !blocks_for(CX.chunk * F->ntiles, kFiltWaves, &fblocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the cell map kernels (not launched)");
  for (int64_t q = 0; q < CX.nchunks; q++) {
    const int64_t cell0 = q * CX.chunk, n = q + 1 < CX.nchunks ? CX.chunk : CX.last_chunk;      // cells [cell0, cell0 + n)
    FA.index = MA.index = SA.index = index + cell0 * nexp;
    FA.nwaves = n * F->ntiles; MA.nrows = n * nexp * nseg;
    WA.index = FA.index; WA.nwaves = FA.nwaves;
    SA.map = h->d_cm_map.as<double>() + cell0; SA.ncells = n;
    const dim3 fgrid((unsigned)((FA.nwaves + kFiltWaves - 1) / kFiltWaves)), fblock(64 * kFiltWaves);
    if (wt) LAUNCH_NPAD(k_cell_wfilter, F->npad, fgrid, fblock, h->stream, WA);
    else LAUNCH_NPAD(k_cell_filter, F->npad, fgrid, fblock, h->stream, FA);
    hipLaunchKernelGGL(k_cell_moments, dim3((unsigned)((MA.nrows + kMomWaves - 1) / kMomWaves)), dim3(64 * kMomWaves), 0, h->stream, MA);
    hipLaunchKernelGGL(k_cell_stat, dim3((unsigned)((n + kCellStatWaves - 1) / kCellStatWaves)), dim3(64 * kCellStatWaves), 0, h->stream, SA);
  }
  HIPCHK(h, hipGetLastError());
  return TRX_OK;
}

// The map of PR's rows (the pairs of the lags in h->d_pixout, or h->d_pixhp with a high-pass; the run waited for), behind the
// upload of the call's arrays on the main queue: the index table once, then the chunks, which follow that table.
static int launch_filtered_map(trx_handle *h, const PixelRun &PR, const trx_vmap *vm, const VmapExtents &VX, const CellMapExtents &CX)
{
  if (const int rc = launch_cell_tracks(h, vm, VX, CX)) return rc;
  return launch_cell_chunks(h, PR, vm, CX, h->d_cm_index, vm->nlag);
}

int trx_run_filtered_map(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, const trx_vmap *vm, double *map, int32_t *lag_index,
                         trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_run_filtered_map";
  std::string msg;
  if (const int rc = filtered_map_checks(product_state(h), who, vm, map, msg)) return fail(h, rc, msg);
  const ObservedSet *O = h->observed.get();
  const VmapExtents VX = vmap_extents(*vm, O->nexp);
  const CellMapExtents CX = cell_map_extents((int64_t)vm->nkp * vm->nvsys, O->nexp, O->nseg, O->npix);
  if (const int rc = vmap_pack(who, *vm, VX, h->vm_in, msg)) return fail(h, rc, msg);
  // one pixel pass of nlag rows, the one trx_run_trail makes -- no moments, no trail; the high-pass when one is installed
  PixelRun PR{h->pixels.get(), vm->nlag}; PR.hp = h->highpass.get();
  if (const int rc = pixel_run(h, who, a, o, spectrum, PR, vm->lag, dbg)) return rc;
  int rc;
  // (the run has been waited for: the kernels follow the upload on the main queue)
  if ((rc = ensure(h, h->d_cm_index, CX.index_bytes)) || (rc = ensure(h, h->d_cm_val, CX.val_bytes)) || (rc = ensure(h, h->d_cm_mom, CX.mom_bytes)) ||
      (rc = ensure(h, h->d_cm_map, CX.map_bytes)) || (rc = upload(h, h->d_vm_in, h->vm_in)) || (rc = launch_filtered_map(h, PR, vm, VX, CX)))
    return rc;
  HIPCHK(h, hipMemcpyAsync(map, h->d_cm_map.p, CX.map_bytes, hipMemcpyDeviceToHost, h->stream));
  if (lag_index) HIPCHK(h, hipMemcpyAsync(lag_index, h->d_cm_index.p, CX.index_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TRX_OK;
}

// ---- the Kp-Vsys map under the exposure table: its pixel rows are (lag, exposure) pairs (trx_expmap.hip.h) ----
// the spans of the lags the inside cells take at every exposure (k_cell_spans), behind k_cell_tracks on the main queue, read
// back into h->em_span [nexp][2]: the queue is waited for
static int launch_cell_spans(trx_handle *h, const CellMapExtents &CX, const ExposedMapExtents &EX, int32_t nexp)
{
  CellSpanArgs SA{};
  SA.index = h->d_cm_index.as<int32_t>(); SA.span = h->d_em_span.as<int32_t>(); SA.ncells = CX.cells; SA.nexp = nexp;
  // (every address the kernel reads or writes: the index table over [cells][nexp], the spans over [nexp][2])
  if (!SA.index || !SA.span || nexp < 1 || CX.cells < 1 || CX.tracks != CX.cells * nexp || h->d_cm_index.bytes < CX.index_bytes ||
      CX.index_bytes < sizeof(int32_t) * (size_t)CX.tracks || EX.span_bytes < sizeof(int32_t) * 2 * (size_t)nexp || h->d_em_span.bytes < EX.span_bytes ||
      !grid_ok(EX.span_blocks) || EX.span_blocks * kCellSpanWaves < nexp)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the cell span kernel (not launched)");
  try { h->em_span.assign(2 * (size_t)nexp, 0); } catch (...) { return fail(h, TRX_E_NOMEM, "trx_run_exposed_map: out of host memory"); }
  hipLaunchKernelGGL(k_cell_spans, dim3((unsigned)EX.span_blocks), dim3(64 * kCellSpanWaves), 0, h->stream, SA);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(h->em_span.data(), h->d_em_span.p, EX.span_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return TRX_OK;
}

// the row table of the call's cells (k_cell_rows) into h->d_em_row from the lag table, the spans on the device and the rows'
// bases L.base, which go up first
static int launch_cell_rows(trx_handle *h, const CellMapExtents &CX, const ExposedMapExtents &EX, int32_t nexp, const ExposedMapRows &L)
{
  if (const int rc = upload(h, h->d_em_base, L.base)) return rc;
  CellRowArgs RA{};
  RA.index = h->d_cm_index.as<int32_t>(); RA.span = h->d_em_span.as<int32_t>(); RA.base = h->d_em_base.as<int64_t>(); RA.row = h->d_em_row.as<int32_t>();
  RA.ntracks = CX.tracks; RA.nexp = nexp;
  // (every address the kernel reads or writes: the two tables over [cells][nexp], the spans over [nexp][2], the bases over
  // [nexp] of the [nexp + 1] there are; a row it writes is below base[nexp] = R, an int32 count)
  if (!RA.index || !RA.span || !RA.base || !RA.row || nexp < 1 || CX.tracks != CX.cells * nexp || CX.tracks < 1 || CX.tracks > 0x7fffffffLL ||
      h->d_cm_index.bytes < CX.index_bytes || EX.row_bytes < sizeof(int32_t) * (size_t)CX.tracks || h->d_em_row.bytes < EX.row_bytes ||
      h->d_em_span.bytes < EX.span_bytes || L.base.size() != (size_t)nexp + 1 || h->d_em_base.bytes < sizeof(int64_t) * ((size_t)nexp + 1) ||
      L.base.back() != L.R || L.R != EX.rows || L.R < 1 || L.R > 0x7fffffffLL ||
      !grid_ok(CX.track_blocks) || CX.track_blocks * kCellTrackBlock < CX.tracks)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the cell row kernel (not launched)");
  hipLaunchKernelGGL(k_cell_rows, dim3((unsigned)CX.track_blocks), dim3(kCellTrackBlock), 0, h->stream, RA);
  return TRX_OK;
}

int trx_run_exposed_map(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, const trx_vmap *vm, double *map, int32_t *lag_index,
                        int64_t *nrows, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_run_exposed_map";
  std::string msg;
  if (const int rc = exposed_map_checks(product_state(h), who, vm, map, msg)) return fail(h, rc, msg);
  if (!a || !o) return TRX_E_ARG;
  const ObservedSet *O = h->observed.get(); const ExposureSet *T = h->exposures.get();
  const int32_t nexp = O->nexp;
  const VmapExtents VX = vmap_extents(*vm, nexp);
  const CellMapExtents CX = cell_map_extents((int64_t)vm->nkp * vm->nvsys, nexp, O->nseg, O->npix);
  ExposedMapExtents EX;
  // (the two tables' extents do not depend on R: no row refuses nothing)
  if (const int rc = exposed_map_extents(who, 0, O->npix, CX.cells, nexp, EX, msg)) return fail(h, rc, msg);
  if (const int rc = vmap_pack(who, *vm, VX, h->vm_in, msg)) return fail(h, rc, msg);
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  // the tracks and the spans AHEAD of the pixel pass: they say which (lag, exposure) rows it has to make
  if ((rc = ensure(h, h->d_cm_index, CX.index_bytes)) || (rc = ensure(h, h->d_em_span, EX.span_bytes)) || (rc = ensure(h, h->d_em_row, EX.row_bytes)) ||
      (rc = upload(h, h->d_vm_in, h->vm_in)) || (rc = launch_cell_tracks(h, vm, VX, CX)) || (rc = launch_cell_spans(h, CX, EX, nexp)))
    return rc;
  ExposedMapRows L;
  if ((rc = exposed_map_bases(who, h->em_span.data(), nexp, vm->nlag, L, msg)) || (rc = exposed_map_extents(who, L.R, O->npix, CX.cells, nexp, EX, msg)))
    return fail(h, rc, msg);
  if (L.R == 0) {
    // no cell inside the lag grid: the spectrum alone -- no pixel, filter or moment kernel --, and a map of NaN
    if ((rc = run_once(h, a, o, spectrum, nullptr, dbg, Products{}))) return rc;
    const double nan = __builtin_nan("");
    for (int64_t c = 0; c < CX.cells; c++) map[c] = nan;
    if (lag_index) HIPCHK(h, hipMemcpy(lag_index, h->d_cm_index.p, CX.index_bytes, hipMemcpyDeviceToHost));
    if (nrows) *nrows = 0;
    return TRX_OK;
  }
  if ((rc = exposed_map_row_arrays(who, h->em_span.data(), nexp, vm->lag, T->scale.empty() ? nullptr : T->scale.data(),
                                   T->smear.empty() ? nullptr : T->smear.data(), L, msg)))
    return fail(h, rc, msg);
  // one pixel pass of R rows with a table of their own -- row r's shift, smear and scale --, not the handle's: no moments,
  // no trail; the high-pass when one is installed
  ExposureSet rows; rows.nexp = (int32_t)L.R; rows.scale = std::move(L.scale); rows.smear = std::move(L.smear);
  PixelRun PR{h->pixels.get(), (int32_t)L.R}; PR.hp = h->highpass.get(); PR.ex = &rows; PR.ex_rows = true;
  // (a call that fails leaves no copy from this call's own arrays -- the rows', the bases -- in flight when they go)
  auto failed = [&](int code) { (void)hipStreamSynchronize(h->stream); return code; };
  if ((rc = pixel_run(h, who, a, o, spectrum, PR, L.shift.data(), dbg))) return failed(rc);
  // (the run has been waited for: the kernels follow on the main queue, the cells' rows named by the row table)
  if ((rc = ensure(h, h->d_cm_val, CX.val_bytes)) || (rc = ensure(h, h->d_cm_mom, CX.mom_bytes)) || (rc = ensure(h, h->d_cm_map, CX.map_bytes)) ||
      (rc = launch_cell_rows(h, CX, EX, nexp, L)) || (rc = launch_cell_chunks(h, PR, vm, CX, h->d_em_row, L.R)))
    return failed(rc);
  HIPCHK(h, hipMemcpyAsync(map, h->d_cm_map.p, CX.map_bytes, hipMemcpyDeviceToHost, h->stream));
  if (lag_index) HIPCHK(h, hipMemcpyAsync(lag_index, h->d_cm_index.p, CX.index_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (nrows) *nrows = L.R;
  return TRX_OK;
}

// ---- detrending the observed set itself: model injection and SYSREM (trx_sysrem.hip.h) --------------
// the SYSREM kernels of dt over the residuals in h->d_sr_r, on the main queue: X the call's extents, ntiles the tiles in h->d_sr_tiles;
// coef_first: the row of h->d_sr_coef the first component's column vector goes to (trx_regress_observed: behind the given vectors')
static int launch_sysrem(trx_handle *h, const ObservedSet *O, const trx_detrend *dt, const SysremExtents &X, int64_t ntiles, int32_t coef_first = 0)
{
  const size_t coef_at = sizeof(double) * (size_t)coef_first * (size_t)O->npix;
  SysremArgs A{};
  A.r = h->d_sr_r.as<double>(); A.weight = O->d_weight.raw().as<double>(); A.tiles = h->d_sr_tiles.as<FilterTile>(); A.seg_first = O->d_seg.as<int64_t>();
  A.a = h->d_sr_a.as<double>(); A.c = h->d_sr_c.as<double>(); A.coef = h->d_sr_coef.p ? h->d_sr_coef.as<double>() + (size_t)coef_first * (size_t)O->npix : nullptr; A.basis = h->d_sr_basis.as<double>();
  A.npix = O->npix; A.ntiles = ntiles; A.nrows = X.rows; A.nexp = O->nexp; A.nseg = O->nseg; A.ncomp = dt->ncomp;
  // (every address the kernels read or write: the residuals and the weights [nexp][npix], the tiles -- which cover [0, npix) --,
  // the bounds [nseg + 1], a [nseg][nexp], c [npix], coef [ncomp][npix], U [nseg][nexp][ncomp])
  if (!A.r || !A.tiles || !A.a || !A.c || !A.coef || !A.basis || !observed_set_whole(*O, O->d_weight.raw(), false) || ntiles < 1 || coef_first < 0 ||
      h->d_sr_r.bytes < X.r_bytes || (A.weight && O->d_weight.raw().bytes < X.r_bytes) || h->d_sr_tiles.bytes < sizeof(FilterTile) * (size_t)ntiles ||
      h->d_sr_a.bytes < X.a_bytes || h->d_sr_c.bytes < X.c_bytes || h->d_sr_coef.bytes < coef_at + X.coef_bytes || h->d_sr_basis.bytes < X.basis_bytes ||
      !grid_ok(X.tile_blocks) || !grid_ok(X.row_blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the SYSREM kernels (not launched)");
  // (an empty segment has no tile: its vectors stay zero)
  HIPCHK(h, hipMemsetAsync(A.basis, 0, X.basis_bytes, h->stream));
  HIPCHK(h, hipMemsetAsync(A.coef, 0, X.coef_bytes, h->stream));
  const dim3 tgrid((unsigned)X.tile_blocks), tblock(64 * kFiltWaves), rgrid((unsigned)X.row_blocks), rblock(64 * kMomWaves);
  for (int32_t i = 0; i < dt->ncomp; i++) {
    A.comp = i;
    for (int32_t k = 0; k < dt->niter; k++) {
      SysremArgs C = A;
      if (k == 0) C.a = nullptr;                       // (a component starts from a = 1)
      hipLaunchKernelGGL(k_sysrem_cols, tgrid, tblock, 0, h->stream, C);
      hipLaunchKernelGGL(k_sysrem_rows, rgrid, rblock, 0, h->stream, A);
    }
    hipLaunchKernelGGL(k_sysrem_close, tgrid, tblock, 0, h->stream, A);
    hipLaunchKernelGGL(k_sysrem_subtract, tgrid, tblock, 0, h->stream, A);
  }
  HIPCHK(h, hipGetLastError());
  return TRX_OK;
}

// step 1b of a detrending call (who), on the main queue behind steps 0 and 1: the recipe installed on h over f0 in h->d_sr_r,
// in place (trx_normalise.hip.h); the row scales, the centres and the columns' counts are left in h->d_nm_*
static int launch_normalise(trx_handle *h, const char *who, const ObservedSet *O)
{
  std::string msg; int rc;
  if ((rc = sysrem_tiles(product_state(h), h->nm_tiles, msg, who))) return fail(h, rc, msg);
  const int64_t ntiles = (int64_t)h->nm_tiles.size();
  if (ntiles < 1) return fail(h, TRX_E_ARG, std::string(who) + ": the observed set has no pixel in any segment");
  const NormExtents X = normalise_extents(O->npix, O->nexp, O->nseg, ntiles, kNormWaves);
  if ((rc = ensure(h, h->d_nm_scale, X.scale_bytes)) || (rc = ensure(h, h->d_nm_centre, X.centre_bytes)) || (rc = ensure(h, h->d_nm_count, X.count_bytes)) ||
      (rc = upload(h, h->d_nm_tiles, h->nm_tiles)))
    return rc;
  const DevBuf &W = O->d_weight.raw();
  NormArgs A{};
  A.r = h->d_sr_r.as<double>(); A.weight = W.as<double>(); A.tiles = h->d_nm_tiles.as<FilterTile>(); A.seg_first = O->d_seg.as<int64_t>();
  A.scale = h->d_nm_scale.as<double>(); A.centre = h->d_nm_centre.as<double>(); A.count = h->d_nm_count.as<int32_t>();
  A.npix = O->npix; A.ntiles = ntiles; A.nexp = O->nexp; A.nseg = O->nseg;
  A.row_kind = h->norm.row_kind; A.col_kind = h->norm.col_kind; A.quantile = h->norm.quantile; A.clip = h->norm.clip;
  // (every address the kernels read or write: the data and the weights [nexp][npix], the tiles -- which cover [0, npix) and
  // name segments below nseg --, the bounds [nseg + 1], scale [nexp][nseg] -- one block per row --, centre [npix], the counts
  // [2][npix])
  if (!A.r || !A.tiles || !A.scale || !A.centre || !A.count || !observed_set_whole(*O, W, false) || A.nexp < 1 || A.nseg < 1 || !X.grid_ok ||
      h->d_sr_r.bytes < X.r_bytes || (A.weight && W.bytes < X.r_bytes) || h->d_nm_tiles.bytes < sizeof(FilterTile) * (size_t)ntiles ||
      h->d_nm_scale.bytes < X.scale_bytes || h->d_nm_centre.bytes < X.centre_bytes || h->d_nm_count.bytes < X.count_bytes)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the normalise kernels (not launched)");
  HIPCHK(h, hipMemsetAsync(A.scale, 0, X.scale_bytes, h->stream));
  hipLaunchKernelGGL(k_norm_rowscale, dim3((unsigned)X.row_blocks), dim3(kNormBlock), 0, h->stream, A);
  hipLaunchKernelGGL(k_norm_cols, dim3((unsigned)X.tile_blocks), dim3(64 * kNormWaves), 0, h->stream, A);
  HIPCHK(h, hipGetLastError());
  return TRX_OK;
}

// steps 0, 1 and -- with a recipe installed (trx_set_normalise) -- 1b of a detrending call (who), on the main queue.
// Steps 0 and 1: the raw data, or the injected data, into h->d_sr_r.  With an
// injection the pairs come from the pixel stage alone, as trx_run_exposed (or, without a table, trx_run_pixels) runs it -- no
// moments, no high-pass, no filter; they are in h->d_pixout and the run has been waited for.
// The caller's part of it: who it is, whether and how it injects, the run's arguments as it got them.
struct FillCall {
  const char *who; bool inject; double p0, p1;
  const trx_atm *a; const trx_opts *o; double *spectrum; int32_t nshift; const double *shift; trx_debug *dbg;
};
static int detrend_fill(trx_handle *h, const ObservedSet *O, const FillCall &C)
{
  const FillExtents X = fill_extents(O->npix, O->nexp, kPixBlock);
  if (C.inject) {
    PixelRun PR{h->pixels.get(), C.nshift}; PR.ex = h->exposures.get();
    if (const int rc = pixel_run(h, C.who, C.a, C.o, C.spectrum, PR, C.shift, C.dbg)) return rc;
    if (PR.ext.pairs != X.cells || h->d_pixout.bytes < PR.ext.pair_bytes) return fail(h, TRX_E_HIP, "internal: the injection's pairs are not the observed set's size");
  }
  if (const int rc = ensure(h, h->d_sr_r, X.r_bytes)) return rc;
  const DevBuf &raw = O->d_data.raw();
  if (!raw.p || raw.bytes < X.r_bytes) return fail(h, TRX_E_HIP, "internal: the observed set's data are not its size");
  if (C.inject) {
    SysremInjectArgs IA{};
    IA.pairs = h->d_pixout.as<double2>(); IA.raw = raw.as<double>(); IA.gain = O->d_gain.as<double>(); IA.r = h->d_sr_r.as<double>();
    IA.npix = O->npix; IA.cells = X.cells; IA.p0 = C.p0; IA.p1 = C.p1;
    if ((IA.gain && O->d_gain.bytes < X.c_bytes) || !grid_ok(X.elem_blocks))
      return fail(h, TRX_E_HIP, "internal: incomplete arguments for the injection kernel (not launched)");
    hipLaunchKernelGGL(k_sysrem_inject, dim3((unsigned)X.elem_blocks), dim3(kPixBlock), 0, h->stream, IA);
    HIPCHK(h, hipGetLastError());
  } else HIPCHK(h, hipMemcpyAsync(h->d_sr_r.p, raw.p, X.r_bytes, hipMemcpyDeviceToDevice, h->stream));
  // step 1b (without a recipe nothing is launched: the call's bits are what they were)
  return h->norm_on ? launch_normalise(h, C.who, O) : TRX_OK;
}

// The swap that ends a detrending call: the call's buffer in force as the data (a high-pass over them goes first, as in the
// undo), the weights of trx_set_observed back, and S in the filter slot -- an empty S clears it.
static void detrend_swap(trx_handle *h, ObservedSet *O, std::unique_ptr<FilterSet> &S)
{
  O->d_data.uncover(h->d_hp_r);
  O->d_data.adopt(h->d_sr_r); O->d_weight.restore(h->d_sc_w);
  install_filter_set(h, S);
}

// step 3 of a detrending call (who), every kernel finished and U [nseg][nexp][ncomp] in h->sr_basis: the weighted filter of U
// as trx_set_weighted_filter makes it -- it reads the set's weights as trx_set_observed installed them, not its data --, the
// outputs, and only then the swap, which puts those weights back in force.  made: that filter where the call has made it
// already, with made_nsingular its count (trx_regress_observed without fitted components: the factor its fit ran from)
static int detrend_install(trx_handle *h, const char *who, ObservedSet *O, int32_t ncomp, size_t basis_bytes, size_t coef_bytes, size_t r_bytes,
                           double *basis, double *coef, double *data, int64_t *nsingular, std::unique_ptr<FilterSet> *made = nullptr,
                           int64_t made_nsingular = 0)
{
  std::string msg; int rc;
  if ((rc = sysrem_basis_check(h->sr_basis.data(), O->nseg, O->nexp, ncomp, msg, who))) return fail(h, rc, msg);
  const trx_wfilter wf{ncomp, 0, h->sr_basis.data()};
  std::unique_ptr<FilterSet> S; int64_t nsing = made_nsingular;
  if (made) S = std::move(*made);
  else if ((rc = make_wfilter_set(h, &wf, S, &nsing, &O->d_weight.raw()))) return rc;
  if (coef) HIPCHK(h, hipMemcpy(coef, h->d_sr_coef.p, coef_bytes, hipMemcpyDeviceToHost));
  if (data) HIPCHK(h, hipMemcpy(data, h->d_sr_r.p, r_bytes, hipMemcpyDeviceToHost));
  if (basis) std::memcpy(basis, h->sr_basis.data(), basis_bytes);
  detrend_swap(h, O, S);
  if (nsingular) *nsingular = nsing;
  return TRX_OK;
}

// the undo of either detrending call: the raw data back, the filter slot cleared
static int detrend_undo(trx_handle *h, ObservedSet *O, int64_t *nsingular)
{
  // (the buffers of the residuals and of a weigh call's weights are kept for the next call when the handle has none)
  O->d_data.uncover(h->d_hp_r);                         // (a high-pass over the data goes first: its buffer is kept for the next one)
  O->d_data.restore(h->d_sr_r); O->d_weight.restore(h->d_sc_w);
  h->filter.reset();
  if (nsingular) *nsingular = 0;
  return TRX_OK;
}

int trx_detrend_observed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift,
                         const trx_detrend *dt, double *basis, double *coef, double *data, int64_t *nsingular, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_detrend_observed";
  const ProductState P = product_state(h);
  std::string msg;
  if (const int rc = detrend_checks(P, dt, a, o, nshift, shift, msg)) return fail(h, rc, msg);
  ObservedSet *const O = h->observed.get();
  HIPCHK(h, hipSetDevice(h->device));
  if (detrend_is_undo(dt)) return detrend_undo(h, O, nsingular);
  std::vector<FilterTile> tiles;
  if (const int rc = sysrem_tiles(P, tiles, msg)) return fail(h, rc, msg);
  const int64_t ntiles = (int64_t)tiles.size();
  const SysremExtents X = sysrem_extents(O->npix, O->nexp, O->nseg, dt->ncomp, dt->niter, ntiles, kPixBlock, kFiltWaves, kMomWaves);
  try { h->sr_basis.assign(X.basis_bytes / sizeof(double), 0.0); } catch (...) { return fail(h, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  int rc;
  // step 0 and 1: the raw data, or the injected data, into the call's own buffer
  if ((rc = detrend_fill(h, O, FillCall{who, dt->inject != 0, dt->p0, dt->p1, a, o, spectrum, nshift, shift, dbg}))) return rc;
  if ((rc = ensure(h, h->d_sr_a, X.a_bytes)) || (rc = ensure(h, h->d_sr_c, X.c_bytes)) ||
      (rc = ensure(h, h->d_sr_coef, X.coef_bytes)) || (rc = ensure(h, h->d_sr_basis, X.basis_bytes)) || (rc = upload(h, h->d_sr_tiles, tiles)))
    return rc;
  // step 2
  if ((rc = launch_sysrem(h, O, dt, X, ntiles))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->sr_basis.data(), h->d_sr_basis.p, X.basis_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (every kernel has finished; the tiles' staging vector may go)
  // step 3
  return detrend_install(h, who, O, dt->ncomp, X.basis_bytes, X.coef_bytes, X.r_bytes, basis, coef, data, nsingular);
}

// ---- the principal components of the observed set in SYSREM's place (trx_pca.hip.h) ------------------
// the PCA kernels of pc over the data in h->d_sr_r, on the main queue: X the call's extents, ntiles the tiles in h->d_sr_tiles
static int launch_pca(trx_handle *h, const ObservedSet *O, const trx_pca *pc, const PcaExtents &X, int64_t ntiles)
{
  PcaArgs A{};
  A.r = h->d_sr_r.as<double>(); A.weight = O->d_weight.raw().as<double>(); A.tiles = h->d_sr_tiles.as<FilterTile>(); A.seg_first = O->d_seg.as<int64_t>();
  A.live = h->d_pc_live.as<int32_t>(); A.whole = h->d_pc_whole.as<int32_t>(); A.G = h->d_pc_g.as<double>(); A.Vt = h->d_pc_v.as<double>();
  A.coef = h->d_sr_coef.as<double>(); A.basis = h->d_sr_basis.as<double>(); A.eigen = h->d_pc_eigen.as<double>(); A.offdiag = h->d_pc_off.as<double>();
  A.nwhole = h->d_pc_nwhole.as<int64_t>();
  A.npix = O->npix; A.ntiles = ntiles; A.nrows = X.rows; A.gram_tiles = X.gram_tiles;
  A.nexp = O->nexp; A.nseg = O->nseg; A.ncomp = pc->ncomp; A.nsweep = pc->nsweep; A.stride = X.stride;
  // (every address the kernels read or write: the data and the weights [nexp][npix], the tiles -- which cover [0, npix) and
  // name segments below nseg --, the bounds [nseg + 1], live [nseg][nexp], whole [npix], G and Vt [nseg][nexp][nexp], coef
  // [ncomp][npix], U [nseg][nexp][ncomp], eigen [nseg][ncomp], offdiag and nwhole [nseg], and X.lds_bytes of LDS: A
  // [nexp][stride] with the round's tables behind it)
  if (!A.r || !A.tiles || !A.live || !A.whole || !A.G || !A.Vt || !A.coef || !A.basis || !A.eigen || !A.offdiag || !A.nwhole ||
      !observed_set_whole(*O, O->d_weight.raw(), false) || ntiles < 1 || A.nexp > TRX_PCA_MAX_EXP || A.ncomp < 1 || A.ncomp > TRX_FILTER_MAX ||
      A.ncomp > A.nexp || A.nsweep < 1 || A.nsweep > TRX_PCA_MAX_SWEEP || A.stride < A.nexp ||
      h->d_sr_r.bytes < X.r_bytes || (A.weight && O->d_weight.raw().bytes < X.r_bytes) || h->d_sr_tiles.bytes < sizeof(FilterTile) * (size_t)ntiles ||
      h->d_pc_live.bytes < X.live_bytes || h->d_pc_whole.bytes < X.whole_bytes || h->d_pc_g.bytes < X.g_bytes || h->d_pc_v.bytes < X.g_bytes ||
      h->d_sr_coef.bytes < X.coef_bytes || h->d_sr_basis.bytes < X.basis_bytes || h->d_pc_eigen.bytes < X.eigen_bytes ||
      h->d_pc_off.bytes < X.offdiag_bytes || h->d_pc_nwhole.bytes < X.nwhole_bytes || !X.grid_ok)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the PCA kernels (not launched)");
  // (the Jacobi block's LDS is dynamic and above the default limit of a launch at the larger sets: raised once per handle, to
  // the most a workgroup may take -- X.grid_ok holds every call's own size under it)
  if (!h->pc_lds_raised) {
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_pca_jacobi), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPcaLdsMost));
    h->pc_lds_raised = true;
  }
  // (a launch that fails is named)
  auto launched = [&](const char *kernel) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRX_OK : fail(h, TRX_E_HIP, std::string("trx_pca_observed: launch of ") + kernel + ": " + hipGetErrorString(e));
  };
  int rc;
  hipLaunchKernelGGL(k_pca_live, dim3((unsigned)X.row_blocks), dim3(64 * kMomWaves), 0, h->stream, A);
  if ((rc = launched("k_pca_live"))) return rc;
  hipLaunchKernelGGL(k_pca_whole, dim3((unsigned)X.tile_blocks), dim3(64 * kFiltWaves), 0, h->stream, A);
  if ((rc = launched("k_pca_whole"))) return rc;
  hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)X.gram_blocks), dim3(64 * kPcaGramWaves), 0, h->stream, A);
  if ((rc = launched("k_pca_gram"))) return rc;
  hipLaunchKernelGGL(k_pca_jacobi, dim3((unsigned)X.jacobi_blocks), dim3(kPcaBlock), X.lds_bytes, h->stream, A);
  if ((rc = launched("k_pca_jacobi"))) return rc;
  hipLaunchKernelGGL(k_pca_project, dim3((unsigned)X.tile_blocks), dim3(64 * kFiltWaves), 0, h->stream, A);
  return launched("k_pca_project");
}

int trx_pca_observed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift, const trx_pca *pc,
                     double *basis, double *coef, double *data, double *eigen, double *offdiag, int64_t *nwhole, int64_t *nsingular, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_pca_observed";
  const ProductState P = product_state(h);
  std::string msg;
  if (const int rc = pca_checks(P, pc, a, o, nshift, shift, msg)) return fail(h, rc, msg);
  ObservedSet *const O = h->observed.get();
  HIPCHK(h, hipSetDevice(h->device));
  if (pca_is_undo(pc)) return detrend_undo(h, O, nsingular);
  std::vector<FilterTile> tiles;
  if (const int rc = sysrem_tiles(P, tiles, msg)) return fail(h, rc, msg);
  const int64_t ntiles = (int64_t)tiles.size();
  const PcaExtents X = pca_extents(O->npix, O->nexp, O->nseg, pc->ncomp, ntiles, kPixBlock, kFiltWaves, kMomWaves);
  try { h->sr_basis.assign(X.basis_bytes / sizeof(double), 0.0); } catch (...) { return fail(h, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  int rc;
  // step 0 and 1, as trx_detrend_observed's
  if ((rc = detrend_fill(h, O, FillCall{who, pc->inject != 0, pc->p0, pc->p1, a, o, spectrum, nshift, shift, dbg}))) return rc;
  if ((rc = ensure(h, h->d_pc_live, X.live_bytes)) || (rc = ensure(h, h->d_pc_whole, X.whole_bytes)) || (rc = ensure(h, h->d_pc_g, X.g_bytes)) ||
      (rc = ensure(h, h->d_pc_v, X.g_bytes)) || (rc = ensure(h, h->d_sr_coef, X.coef_bytes)) || (rc = ensure(h, h->d_sr_basis, X.basis_bytes)) ||
      (rc = ensure(h, h->d_pc_eigen, X.eigen_bytes)) || (rc = ensure(h, h->d_pc_off, X.offdiag_bytes)) || (rc = ensure(h, h->d_pc_nwhole, X.nwhole_bytes)) ||
      (rc = upload(h, h->d_sr_tiles, tiles)))
    return rc;
  // step 2
  if ((rc = launch_pca(h, O, pc, X, ntiles))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->sr_basis.data(), h->d_sr_basis.p, X.basis_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (every kernel has finished; the tiles' staging vector may go)
  // the fit's own outputs (a non-finite U refuses with every output untouched), then step 3: the swap comes last
  if ((rc = sysrem_basis_check(h->sr_basis.data(), O->nseg, O->nexp, pc->ncomp, msg, who))) return fail(h, rc, msg);
  if (eigen) HIPCHK(h, hipMemcpy(eigen, h->d_pc_eigen.p, X.eigen_bytes, hipMemcpyDeviceToHost));
  if (offdiag) HIPCHK(h, hipMemcpy(offdiag, h->d_pc_off.p, X.offdiag_bytes, hipMemcpyDeviceToHost));
  if (nwhole) HIPCHK(h, hipMemcpy(nwhole, h->d_pc_nwhole.p, X.nwhole_bytes, hipMemcpyDeviceToHost));
  return detrend_install(h, who, O, pc->ncomp, X.basis_bytes, X.coef_bytes, X.r_bytes, basis, coef, data, nsingular);
}

// ---- regressing the observed set on given time vectors (trx_regress.hip.h) ----------------------------
// step 2b of the call, on the main queue behind steps 0, 1 and 1b: every column of f0 in h->d_sr_r fitted with the vectors
// and the factor of F -- the weighted filter of the given vectors against the set's weights as installed --, in place;
// the coefficients into the first F.ncomp rows of h->d_sr_coef.  X the call's extents, ntiles the tiles in h->d_sr_tiles
static int launch_regress(trx_handle *h, const ObservedSet *O, const FilterSet &F, const RegressExtents &X, int64_t ntiles)
{
  const DevBuf &W = O->d_weight.raw();
  const WfilterExtents WX = wfilter_extents(F.npix, F.nexp, F.nseg, F.ncomp, F.npad, F.ntiles, kFiltWaves);
  RegressArgs A{};
  A.r = h->d_sr_r.as<double>(); A.weight = W.as<double>(); A.basis = F.d_back.as<double>(); A.fac = F.d_fac.as<double>(); A.live = F.d_live.as<int32_t>();
  A.tiles = h->d_sr_tiles.as<FilterTile>(); A.coef = h->d_sr_coef.as<double>();
  A.npix = O->npix; A.ntiles = ntiles; A.nexp = O->nexp; A.nvec = F.ncomp;
  // (every address the kernel reads or writes: the data and the weights [nexp][npix], the tiles -- which cover [0, npix) and
  // name segments below nseg --, the padded vectors [nseg][nexp][npad], the factor [nfac][npix] and the flags [npix] -- made
  // against W, the weights the kernel reads --, coef [nvec][npix] of the [nvec + nfit][npix] there are)
  if (!A.r || !A.tiles || !A.coef || !A.fac || !A.live || !observed_set_whole(*O, W, false) || !wfilter_basis_whole(F, *O, WX) || ntiles < 1 ||
      F.ncomp < 1 || F.ncomp > X.ncomp || X.ncomp > TRX_FILTER_MAX || h->d_sr_r.bytes < X.r_bytes || X.r_bytes < sizeof(double) * (size_t)O->nexp * (size_t)O->npix ||
      (A.weight && W.bytes < X.r_bytes) || h->d_sr_tiles.bytes < sizeof(FilterTile) * (size_t)ntiles || F.d_fac.bytes < WX.fac_bytes || F.d_live.bytes < WX.live_bytes ||
      X.coef_fit_bytes != sizeof(double) * (size_t)F.ncomp * (size_t)O->npix || h->d_sr_coef.bytes < X.coef_bytes || X.coef_bytes < X.coef_fit_bytes ||
      X.tile_blocks * kFiltWaves < ntiles || !X.grid_ok)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the regression kernel (not launched)");
  LAUNCH_NPAD(k_regress_cols, F.npad, dim3((unsigned)X.tile_blocks), dim3(64 * kFiltWaves), h->stream, A);
  HIPCHK(h, hipGetLastError());
  return TRX_OK;
}

int trx_regress_observed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift, const trx_regress *rg,
                         double *basis, double *coef, double *data, int64_t *nsingular_fit, int64_t *nsingular, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_regress_observed";
  const ProductState P = product_state(h);
  std::string msg;
  if (const int rc = regress_checks(P, rg, a, o, nshift, shift, msg)) return fail(h, rc, msg);
  ObservedSet *const O = h->observed.get();
  HIPCHK(h, hipSetDevice(h->device));
  if (regress_is_undo(rg)) {
    if (nsingular_fit) *nsingular_fit = 0;
    return detrend_undo(h, O, nsingular);
  }
  std::vector<FilterTile> tiles;
  if (const int rc = sysrem_tiles(P, tiles, msg, who)) return fail(h, rc, msg);
  const int64_t ntiles = (int64_t)tiles.size();
  const int32_t nvec = rg->nvec, nfit = rg->nfit;
  const RegressExtents X = regress_extents(O->npix, O->nexp, O->nseg, nvec, nfit, ntiles, kFiltWaves);
  // (the fitted components' own extents: none of them is used where nfit = 0)
  const SysremExtents SX = sysrem_extents(O->npix, O->nexp, O->nseg, nfit, nfit > 0 ? rg->niter : 0, ntiles, kPixBlock, kFiltWaves, kMomWaves);
  std::vector<double> fit;
  try {
    h->sr_basis.assign(X.basis_bytes / sizeof(double), 0.0);
    fit.assign(SX.basis_bytes / sizeof(double), 0.0);
  } catch (...) { return fail(h, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  int rc;
  // steps 0, 1 and 1b, as trx_detrend_observed's
  if ((rc = detrend_fill(h, O, FillCall{who, rg->inject != 0, rg->p0, rg->p1, a, o, spectrum, nshift, shift, dbg}))) return rc;
  // step 2a: the weighted filter of the given vectors against W -- its factor is the fit's (factor_wfilter waits for the queue)
  const trx_wfilter wf{nvec, 0, rg->vectors};
  std::unique_ptr<FilterSet> S; int64_t nsing_fit = 0;
  if ((rc = make_wfilter_set(h, &wf, S, &nsing_fit, &O->d_weight.raw()))) return rc;
  if (!S) return fail(h, TRX_E_HIP, "internal: the given vectors' filter was not made");
  // step 2b
  if ((rc = ensure(h, h->d_sr_coef, X.coef_bytes)) || (rc = upload(h, h->d_sr_tiles, tiles)) || (rc = launch_regress(h, O, *S, X, ntiles))) return rc;
  // step 2c: SYSREM on what is left
  if (nfit > 0) {
    const trx_detrend dt{nfit, rg->niter, 0, 0, 0.0, 0.0};
    if ((rc = ensure(h, h->d_sr_a, SX.a_bytes)) || (rc = ensure(h, h->d_sr_c, SX.c_bytes)) || (rc = ensure(h, h->d_sr_basis, SX.basis_bytes)) ||
        (rc = launch_sysrem(h, O, &dt, SX, ntiles, nvec)))
      return rc;
    HIPCHK(h, hipMemcpyAsync(fit.data(), h->d_sr_basis.p, SX.basis_bytes, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (every kernel has finished; the tiles' staging vector may go)
  regress_merge(rg->vectors, fit.data(), O->nseg, O->nexp, nvec, nfit, h->sr_basis.data());
  // step 3: without fitted components the filter of step 2a is the one to install
  int64_t nsing = 0;
  if ((rc = detrend_install(h, who, O, X.ncomp, X.basis_bytes, X.coef_bytes, X.r_bytes, basis, coef, data, &nsing, nfit == 0 ? &S : nullptr, nsing_fit))) return rc;
  if (nsingular_fit) *nsingular_fit = nsing_fit;
  if (nsingular) *nsingular = nsing;
  return TRX_OK;
}

// ---- normalising the observed set: the recipe of step 1b and the detrend of zero components (trx_normalise.hip.h) ----
int trx_set_normalise(trx_handle *h, const trx_normalise *nm)
{
  if (!h) return TRX_E_ARG;
  std::string msg;
  if (const int rc = normalise_set_checks(product_state(h), nm, msg)) return fail(h, rc, msg);
  // (host work alone: the data, the weights and the filter in force stay; the next detrending call takes the recipe)
  h->norm_on = nm != nullptr;
  h->norm = nm ? *nm : trx_normalise{};
  return TRX_OK;
}

int trx_normalise_observed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, int32_t nshift, const double *shift,
                           int32_t inject, double p0, double p1, double *data, double *rowscale, double *centre, int64_t *nclipped, int64_t *nbad,
                           trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_normalise_observed";
  const ProductState P = product_state(h);
  std::string msg;
  if (const int rc = normalise_checks(P, h->norm_on, inject, p0, p1, a, o, nshift, shift, msg)) return fail(h, rc, msg);
  ObservedSet *const O = h->observed.get();
  HIPCHK(h, hipSetDevice(h->device));
  const NormExtents N = normalise_extents(O->npix, O->nexp, O->nseg, 1, kNormWaves);
  try { h->nm_count.assign(N.count_bytes / sizeof(int32_t), 0); } catch (...) { return fail(h, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  int rc;
  // steps 0, 1 and 1b, into the call's own buffer
  if ((rc = detrend_fill(h, O, FillCall{who, inject != 0, p0, p1, a, o, spectrum, nshift, shift, dbg}))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->nm_count.data(), h->d_nm_count.p, N.count_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (every kernel has finished)
  if (data) HIPCHK(h, hipMemcpy(data, h->d_sr_r.p, N.r_bytes, hipMemcpyDeviceToHost));
  if (rowscale) HIPCHK(h, hipMemcpy(rowscale, h->d_nm_scale.p, N.scale_bytes, hipMemcpyDeviceToHost));
  if (centre) HIPCHK(h, hipMemcpy(centre, h->d_nm_centre.p, N.centre_bytes, hipMemcpyDeviceToHost));
  // the swap comes last, as detrend_install's: the data in force, the weights of trx_set_observed back, no filter
  std::unique_ptr<FilterSet> none;
  detrend_swap(h, O, none);
  // (the counts are integers: per column on the device, over the columns here)
  int64_t nc = 0, nb = 0;
  const size_t npix = (size_t)O->npix;
  for (size_t p = 0; p < npix; p++) { nc += h->nm_count[p]; nb += h->nm_count[npix + p]; }
  if (nclipped) *nclipped = nc;
  if (nbad) *nbad = nb;
  return TRX_OK;
}

// ---- weighing the observed set by its columns' scatter (trx_scatter.hip.h) --------------------------
int trx_weigh_observed(trx_handle *h, const trx_scatter *sc, double *variance, double *median, double *weight, int64_t *nmasked, int64_t *nsingular)
{
  if (!h) return TRX_E_ARG;
  const char *const who = "trx_weigh_observed";
  const ProductState P = product_state(h);
  std::string msg;
  if (const int rc = scatter_checks(P, sc, msg)) return fail(h, rc, msg);
  ObservedSet *const O = h->observed.get();
  FilterSet *const F = h->filter && h->filter->weighted ? h->filter.get() : nullptr;
  HIPCHK(h, hipSetDevice(h->device));
  int rc; int64_t nsing = 0;
  if (scatter_is_undo(sc)) {
    const DevBuf &W = O->d_weight.raw();
    if (F && (rc = factor_wfilter(h, *F, O, W.as<double>(), W.bytes, h->d_sc_fac, h->d_sc_live, &nsing))) return rc;
    O->d_weight.restore(h->d_sc_w);
    if (F) { exchange_buf(F->d_fac, h->d_sc_fac); exchange_buf(F->d_live, h->d_sc_live); }
    if (nmasked) *nmasked = 0;
    if (nsingular) *nsingular = nsing;
    return TRX_OK;
  }
  std::vector<FilterTile> tiles; std::vector<int32_t> flags;
  if ((rc = scatter_tiles(P, kScatBlock, tiles, msg))) return fail(h, rc, msg);
  const int64_t ntiles = (int64_t)tiles.size();
  const ScatterExtents X = scatter_extents(O->npix, O->nexp, O->nseg, ntiles, kScatBlock);
  try { flags.assign((size_t)O->npix, 0); } catch (...) { return fail(h, TRX_E_NOMEM, std::string(who) + ": out of host memory"); }
  if ((rc = ensure(h, h->d_sc_w, X.w_bytes)) || (rc = ensure(h, h->d_sc_var, X.var_bytes)) || (rc = ensure(h, h->d_sc_med, X.med_bytes)) ||
      (rc = ensure(h, h->d_sc_flag, X.flag_bytes)) || (rc = upload(h, h->d_sc_tiles, tiles)))
    return rc;
  const DevBuf &W = O->d_weight.raw();
  ScatterArgs A{};
  A.r = O->d_data.now.as<double>(); A.weight = W.as<double>(); A.tiles = h->d_sc_tiles.as<FilterTile>(); A.seg_first = O->d_seg.as<int64_t>();
  A.var = h->d_sc_var.as<double>(); A.med = h->d_sc_med.as<double>(); A.out = h->d_sc_w.as<double>(); A.flag = h->d_sc_flag.as<int32_t>();
  A.npix = O->npix; A.ntiles = ntiles; A.nexp = O->nexp; A.kind = sc->kind; A.min_live = sc->min_live; A.clip = sc->clip;
  // (every address the kernels read or write: the data and the weights [nexp][npix], the tiles -- which cover [0, npix) and
  // name segments below nseg --, the bounds [nseg + 1], var and the flags [npix], med [nseg], w' [nexp][npix])
  if (!observed_set_whole(*O, W, true) || !A.tiles || !A.var || !A.med || !A.out || !A.flag || A.nexp < 2 || !X.grid_ok ||
      O->d_data.now.bytes < X.w_bytes || (A.weight && W.bytes < X.w_bytes) || h->d_sc_tiles.bytes < sizeof(FilterTile) * (size_t)ntiles ||
      h->d_sc_var.bytes < X.var_bytes || h->d_sc_med.bytes < X.med_bytes ||
      h->d_sc_w.bytes < X.w_bytes || h->d_sc_flag.bytes < X.flag_bytes)
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the scatter kernels (not launched)");
  // (an empty segment has no tile, a segment without a live column no lane that stores: their medians stay +0)
  HIPCHK(h, hipMemsetAsync(A.med, 0, X.med_bytes, h->stream));
  hipLaunchKernelGGL(k_scatter_cols, dim3((unsigned)X.col_blocks), dim3(kScatBlock), 0, h->stream, A);
  hipLaunchKernelGGL(k_scatter_median, dim3((unsigned)X.tile_blocks), dim3(kScatBlock), 0, h->stream, A);
  hipLaunchKernelGGL(k_scatter_weights, dim3((unsigned)X.tile_blocks), dim3(kScatBlock), 0, h->stream, A);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(flags.data(), h->d_sc_flag.p, X.flag_bytes, hipMemcpyDeviceToHost, h->stream));
  // the installed weighted filter's factor against w', in the handle's own buffers (factor_wfilter waits for the queue: every
  // kernel has finished, the staging vectors may go)
  if (F) { if ((rc = factor_wfilter(h, *F, O, A.out, h->d_sc_w.bytes, h->d_sc_fac, h->d_sc_live, &nsing))) return rc; }
  else HIPCHK(h, hipStreamSynchronize(h->stream));
  if (variance) HIPCHK(h, hipMemcpy(variance, h->d_sc_var.p, X.var_bytes, hipMemcpyDeviceToHost));
  if (median) HIPCHK(h, hipMemcpy(median, h->d_sc_med.p, X.med_bytes, hipMemcpyDeviceToHost));
  if (weight) HIPCHK(h, hipMemcpy(weight, h->d_sc_w.p, X.w_bytes, hipMemcpyDeviceToHost));
  // the swap: W aside on the first call (empty where the set had no weights), w' in force, the new factor in the filter
  O->d_weight.adopt(h->d_sc_w);
  if (F) { exchange_buf(F->d_fac, h->d_sc_fac); exchange_buf(F->d_live, h->d_sc_live); }
  int64_t nm = 0;
  for (int32_t x : flags) nm += x == kScatClipped ? 1 : 0;
  if (nmasked) *nmasked = nm;
  if (nsingular) *nsingular = nsing;
  return TRX_OK;
}

// ---- high-passing the observed set itself (k_data_highpass, trx_highpass.hip.h) ----------------------
int trx_highpass_observed(trx_handle *h, int32_t apply, double *data, int64_t *ndead)
{
  if (!h) return TRX_E_ARG;
  std::string msg;
  if (const int rc = hpdata_checks(product_state(h), apply, msg)) return fail(h, rc, msg);
  ObservedSet *const O = h->observed.get();
  HIPCHK(h, hipSetDevice(h->device));
  if (hpdata_is_undo(apply)) {
    // (the buffer of the high-passed data is kept for the next call when the handle has none)
    O->d_data.uncover(h->d_hp_r);
    if (ndead) *ndead = 0;
    return TRX_OK;
  }
  const HighPassSet &F = *h->highpass;
  const HpDataExtents X = hpdata_extents(O->npix, O->nexp, F.ntiles, F.half);
  if (const int rc = hpdata_launch_checks(X, msg)) return fail(h, rc, msg);
  int rc;
  if ((rc = ensure(h, h->d_hp_r, X.r_bytes))) return rc;
  // r: what the last successful detrend left -- never an earlier high-pass's result --; W: as trx_set_observed installed them
  const DevBuf &R = O->d_data.base(), &W = O->d_weight.raw();
  HpDataArgs A{};
  A.r = R.as<double>(); A.weight = W.as<double>(); A.taps = F.d_taps.as<double>(); A.tiles = F.d_tiles.as<HpTile>(); A.out = h->d_hp_r.as<double>();
  A.npix = F.npix; A.ntiles = F.ntiles; A.den_full = F.den_full; A.half = F.half;
  // (every address the kernel reads or writes: data in and out and the weights over [nexp][npix] -- the tiles lie in [0, npix)
  // within their segments' bounds, made so from this observed set's when the high-pass was --, the taps [half + 1], the tiles,
  // and (count + 2 half) * 2 doubles of LDS, count <= kHpTile; the output is a buffer of its own)
  if (F.obs != O || !observed_set_whole(*O, W, true) || !A.r || R.bytes < X.r_bytes || (A.weight && W.bytes < X.r_bytes) || !A.taps || !A.tiles || !A.out ||
      A.out == A.r || h->d_hp_r.bytes < X.r_bytes || F.half < 0 || F.half > TRX_HIGHPASS_MAX_HALF || F.npix != O->npix || F.nseg != O->nseg || F.ntiles < 1 ||
      F.d_taps.bytes < sizeof(double) * ((size_t)F.half + 1) || F.d_tiles.bytes < sizeof(HpTile) * (size_t)F.ntiles || X.lds_bytes > 65536 || !grid_ok(X.blocks))
    return fail(h, TRX_E_HIP, "internal: incomplete arguments for the data high-pass kernel (not launched)");
  hipLaunchKernelGGL(k_data_highpass, dim3((unsigned)X.blocks), dim3(kHpBlock), X.lds_bytes, h->stream, A);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (every kernel has finished)
  if (data) HIPCHK(h, hipMemcpy(data, h->d_hp_r.p, X.r_bytes, hipMemcpyDeviceToHost));
  // the swap: what was in force goes under on the first call, r' in force; the previous r' waits in d_hp_r for the next call
  O->d_data.cover(h->d_hp_r);
  if (ndead) *ndead = O->ndead;                         // (the weights as installed do not change: counted when they were)
  return TRX_OK;
}

// ---- rotational broadening between the spectrum and the pixels (trx_broaden.hip.h) ------------------
// The broadening as h would keep it, checked whole before anything is replaced: on = false for a clearing call.
static int make_broadening(trx_handle *h, const trx_broadening *br, bool &on, Broadening &out)
{
  on = false; out = Broadening{};
  if (!br || br->kind == TRX_BROADEN_NONE) return TRX_OK;      // (clear)
  std::string msg; int hmax = 0;
  if (const int rc = broadening_checks(product_state(h), br, hmax, msg)) return fail(h, rc, msg);
  on = true; out.beta = br->beta; out.limb = br->limb; out.hmax = hmax;
  return TRX_OK;
}

int trx_set_broadening(trx_handle *h, const trx_broadening *br)
{
  if (!h) return TRX_E_ARG;
  bool on; Broadening B;
  if (const int rc = make_broadening(h, br, on, B)) return rc;
  h->broad_on = on; h->broad = B;
  return TRX_OK;
}

int trx_run_broadened(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum, double *broadened, trx_debug *dbg)
{
  if (!h) return TRX_E_ARG;
  if (!h->broad_on) return fail(h, TRX_E_ARG, "trx_run_broadened: no broadening installed (trx_set_broadening)");
  if (!broadened) return fail(h, TRX_E_ARG, "trx_run_broadened: broadened is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  if (const int rc = ensure(h, h->d_broad, broadened_bytes(h->nwn))) return rc;
  Products want; want.br = &h->broad;
  if (const int rc = run_once(h, a, o, spectrum, nullptr, dbg, want)) return rc;
  HIPCHK(h, hipMemcpy(broadened, h->d_broad.p, broadened_bytes(h->nwn), hipMemcpyDeviceToHost));      // (the run has been waited for)
  return TRX_OK;
}
