// products_check.cpp -- the host side of the run products (transit_amd/csrc/trx_products.h) without a device: the refusal
// table against literal texts, the band and filter layouts' invariants, the extents of hand-worked shapes -- and the launch
// conditions of trx_launch.h over plain structs, its buffer transitions over a counting fake.  Stand-alone
// (tests/test_products_host.py builds it under -fsanitize=address,undefined); every array handed to the header is a heap
// allocation of exactly the stated length, so a read past an extent is a sanitizer report.
//
//   products_check              every check; prints "gauss <wn_i> <wn_d> <nwn> <centre> <fwhm> <cut> <first> <last>" for
//                               its GAUSS bands (doubles as %a) and "ok <checks>" at the end
//   products_check gauss FILE   FILE: lines "wn_i wn_d nwn centre fwhm cut"; prints the same lines for them
#include <cmath>
#include <cstring>
#include <vector>

#include "transit_hip.h"
#include "trx_products.h"
#include "trx_launch.h"
#include "check_common.h"

using namespace trx;

static_assert(TRX_OK == 0 && TRX_E_ARG == -1 && TRX_E_UNSUPPORTED == -6, "the codes the tests of the interface pin");

// a whole-grid handle of 5000 bins with a pixel set of 6 pixels, an observed set of 3 exposures by 2 segments and a filter
struct Installed {
  Heap<int64_t> seg{0, 2, 6};
  ProductState S;
  Installed() { S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.lo = 0; S.hi = 5000; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get(); S.filter = true; }
};

// ---- the refusal table -------------------------------------------------------------------------------
static trx_band weights_band(int64_t first, int64_t n, const double *w) { trx_band B{}; B.kind = TRX_BAND_WEIGHTS; B.first = first; B.n = n; B.weights = w; return B; }
static trx_band gauss_band(double centre, double fwhm, double cut) { trx_band B{}; B.kind = TRX_BAND_GAUSS; B.centre = centre; B.fwhm = fwhm; B.cut = cut; return B; }

static void band_refusals()
{
  const Installed I; BandLayout L;
  Heap<double> w{1.0, 2.0, 3.0};
  auto one = [&](const trx_band &B, std::string &msg) { Heap<trx_band> a{gauss_band(2100.0, 1.0, 4.0), B}; return band_layout(I.S, 2, a.get(), L, msg); };
  REFUSED(band_layout(I.S, -1, nullptr, L, msg), TRX_E_ARG, "bands: nbands < 0");
  REFUSED(band_layout(I.S, 2, nullptr, L, msg), TRX_E_ARG, "bands: NULL band array");
  ACCEPTED(band_layout(I.S, 0, nullptr, L, msg));
  REFUSED(one(weights_band(-1, 0, nullptr), msg), TRX_E_ARG, "band 1: n < 1");                  // (and first < 0, and NULL weights)
  REFUSED(one(weights_band(-1, 6000, nullptr), msg), TRX_E_ARG, "band 1: first < 0");           // (and too long, and NULL weights)
  REFUSED(one(weights_band(4998, 3, nullptr), msg), TRX_E_ARG, "band 1: first + n > nwn");      // (and NULL weights)
  REFUSED(one(weights_band(4997, 3, nullptr), msg), TRX_E_ARG, "band 1: NULL weights");
  w[2] = kInf;
  REFUSED(one(weights_band(4997, 3, w.get()), msg), TRX_E_ARG, "band 1: weight 2 is not finite");
  w[0] = kNaN;
  REFUSED(one(weights_band(4997, 3, w.get()), msg), TRX_E_ARG, "band 1: weight 0 is not finite");
  w[0] = 1.0; w[2] = 3.0;
  ACCEPTED(one(weights_band(4997, 3, w.get()), msg));
  REFUSED(one(gauss_band(kNaN, -1.0, -1.0), msg), TRX_E_ARG, "band 1: centre, fwhm and cut must be finite");
  REFUSED(one(gauss_band(2100.0, kInf, 4.0), msg), TRX_E_ARG, "band 1: centre, fwhm and cut must be finite");
  REFUSED(one(gauss_band(2100.0, 1.0, -kInf), msg), TRX_E_ARG, "band 1: centre, fwhm and cut must be finite");
  REFUSED(one(gauss_band(2100.0, 0.0, 0.0), msg), TRX_E_ARG, "band 1: fwhm <= 0");                // (and cut <= 0)
  REFUSED(one(gauss_band(2100.0, 1.0, -4.0), msg), TRX_E_ARG, "band 1: cut <= 0");
  trx_band odd = gauss_band(2100.0, 1.0, 4.0); odd.kind = 7;
  REFUSED(one(odd, msg), TRX_E_ARG, "band 1: unknown kind 7");
  // the first band that is wrong wins
  Heap<trx_band> two{gauss_band(2100.0, 1.0, 0.0), weights_band(0, 0, nullptr)};
  REFUSED(band_layout(I.S, 2, two.get(), L, msg), TRX_E_ARG, "band 0: cut <= 0");
}

static void pixel_refusals()
{
  Heap<double> c{2100.0, 2200.0, 2300.0}, f{1.0, 1.0, 1.0};
  auto set = [&](int64_t npix, const double *centre, const double *fwhm, double cut) { trx_pixels P{}; P.npix = npix; P.centre = centre; P.fwhm = fwhm; P.cut = cut; return P; };
  trx_pixels P = set(-2, nullptr, nullptr, kNaN);
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixels: npix < 0");
  P = set(3, c.get(), nullptr, kNaN);
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixels: NULL centre or fwhm array");
  P = set(3, nullptr, f.get(), 4.0);
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixels: NULL centre or fwhm array");
  for (double cut : {kNaN, kInf, 0.0, -1.0}) {
    P = set(0x80000000LL, c.get(), f.get(), cut);                                                 // (and too many)
    REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixels: cut must be finite and > 0");
  }
  P = set(0x80000000LL, c.get(), f.get(), 4.0);                                                   // (refused before an array is read)
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixels: npix above 2^31 - 1");
  P = set(3, c.get(), f.get(), 4.0);
  ACCEPTED(pixel_set_checks(&P, msg));
  c[2] = 0.0; f[1] = kNaN;
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixel 1: fwhm must be finite and > 0");          // (by pixel, then centre before fwhm)
  f[2] = -1.0; f[1] = 1.0;
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixel 2: centre must be finite and > 0");
  c[2] = kInf;
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixel 2: centre must be finite and > 0");
  c[2] = 2300.0;
  REFUSED(pixel_set_checks(&P, msg), TRX_E_ARG, "pixel 2: fwhm must be finite and > 0");
  // the run's shifts
  Heap<double> sh{1.0, 1.0001, 0.9999};
  ACCEPTED(pixel_run_checks("trx_run_pixels", 3, 6, sh.get(), msg));
  ACCEPTED(pixel_run_checks("trx_run_pixels", 256, 0x7fffffffLL, Heap<double>(256, 1.0).get(), msg));      // (exactly what one launch takes)
  REFUSED(pixel_run_checks("trx_run_pixels", 257, 0x7fffffffLL, Heap<double>(257, 1.0).get(), msg), TRX_E_ARG, "trx_run_pixels: nshift * npix above what one launch takes");
  sh[1] = 0.0;
  REFUSED(pixel_run_checks("trx_run_moments", 3, 6, sh.get(), msg), TRX_E_ARG, "trx_run_moments: shift 1 must be finite and > 0");
  sh[1] = kNaN; sh[2] = -1.0;
  REFUSED(pixel_run_checks("trx_run_filtered_moments", 3, 0x7fffffffLL * 256, sh.get(), msg), TRX_E_ARG, "trx_run_filtered_moments: shift 1 must be finite and > 0");
  sh[1] = 1.0;
  REFUSED(pixel_run_checks("trx_run_trail", 3, 6, sh.get(), msg), TRX_E_ARG, "trx_run_trail: shift 2 must be finite and > 0");
}

static void observed_refusals()
{
  Installed I;
  Heap<int64_t> seg{0, 2, 6};
  Heap<double> data(18, 1.0), weight(18, 1.0), gain(6, 1.0);
  auto set = [&](int32_t nexp, int32_t nseg, const int64_t *sf, const double *d, const double *w, const double *g) {
    trx_observed O{}; O.nexp = nexp; O.nseg = nseg; O.seg_first = sf; O.data = d; O.weight = w; O.gain = g; return O; };
  trx_observed O = set(-1, 0, nullptr, nullptr, nullptr, nullptr);
  ProductState none = I.S; none.npix = 0; none.seg = nullptr; none.nexp = none.nseg = 0;
  REFUSED(observed_set_checks(none, &O, msg), TRX_E_ARG, "observed: no pixel set installed (trx_set_pixels)");
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: nexp < 0");
  O.nexp = 3;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: nseg < 1");
  O.nseg = 2;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: NULL seg_first or data array");
  O.seg_first = seg.get();
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: NULL seg_first or data array");
  O = set(3, 2, seg.get(), data.get(), weight.get(), gain.get());
  ACCEPTED(observed_set_checks(I.S, &O, msg));
  O.weight = O.gain = nullptr;
  ACCEPTED(observed_set_checks(I.S, &O, msg));
  O = set(3, 2, seg.get(), data.get(), weight.get(), gain.get());
  seg[0] = 1; seg[1] = 0; seg[2] = 7;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: seg_first[0] must be 0");
  seg[0] = 0; seg[1] = 8;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: seg_first decreases at segment 1");
  seg[1] = 2;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: seg_first[nseg] must be the pixel set's npix (6)");
  seg[2] = 6;
  {                                                       // (the counts before a datum is read: one exposure's worth is there)
    Heap<int64_t> many(32769, 6); many[0] = 0;
    trx_observed big = set(65536, 32768, many.get(), data.get(), nullptr, nullptr);
    REFUSED(observed_set_checks(I.S, &big, msg), TRX_E_ARG, "observed: nexp * nseg above 2^31 - 1");
  }
  data[8] = kInf; weight[7] = -1.0; gain[0] = kNaN;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: exposure 1 pixel 1: weight must be finite and >= 0");
  weight[7] = 0.0; weight[8] = kNaN;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: exposure 1 pixel 2: datum must be finite");
  data[8] = 1.0;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: exposure 1 pixel 2: weight must be finite and >= 0");
  weight[8] = 1.0;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: pixel 0: gain must be finite");
  gain[0] = 1.0; gain[5] = -kInf;
  REFUSED(observed_set_checks(I.S, &O, msg), TRX_E_ARG, "observed: pixel 5: gain must be finite");
}

static void observed_run_refusals()
{
  const Installed I;
  Heap<double> in(3, 1.0), out(1);
  struct Form { const char *who; ObservedRun kind; const char *reduce, *in_name, *count0; };
  const Form forms[] = {{"trx_run_moments", ObservedRun::Moments, "reduce", "shift", "nshift 0 is not the observed set's nexp 3"},
                        {"trx_run_filtered_moments", ObservedRun::Filtered, "filter and reduce", "shift", "nshift 0 is not the observed set's nexp 3"},
                        {"trx_run_trail", ObservedRun::Trail, "reduce", "lag", "nlag < 1"}};
  for (const Form &F : forms) {
    const std::string who(F.who);
    auto run = [&](const ProductState &S, int32_t n, const void *i, const void *o, std::string &msg) { return observed_run_checks(S, F.who, F.kind, n, i, o, "mom", msg); };
    // a shard of the grid: refused first, whatever is installed and whatever else is wrong
    ProductState W{}; W.windowed = true;
    const std::string windowed = who + ": this handle's shard is not the whole grid; take trx_run_pixels, add the ranks' pairs (trx_gather_host) and " + F.reduce + " them on the host";
    REFUSED(run(W, 0, nullptr, nullptr, msg), TRX_E_UNSUPPORTED, windowed.c_str());
    W = I.S; W.windowed = true;
    REFUSED(run(W, 3, in.get(), out.get(), msg), TRX_E_UNSUPPORTED, windowed.c_str());
    // nothing installed, a pixel set alone
    ProductState N = I.S; N.filter = false; N.seg = nullptr; N.nexp = N.nseg = 0;
    REFUSED(run(N, 0, nullptr, nullptr, msg), TRX_E_ARG, (who + ": no observed set installed (trx_set_observed)").c_str());
    N.npix = 0;
    REFUSED(run(N, 3, in.get(), out.get(), msg), TRX_E_ARG, (who + ": no observed set installed (trx_set_observed)").c_str());
    // no filter: only the filtered run's business, and ahead of its count
    N = I.S; N.filter = false;
    if (F.kind == ObservedRun::Filtered) REFUSED(run(N, 0, nullptr, nullptr, msg), TRX_E_ARG, "trx_run_filtered_moments: no filter installed (trx_set_filter)");
    else ACCEPTED(run(N, 3, in.get(), out.get(), msg));
    // the count, then the arrays: in before out
    REFUSED(run(I.S, 0, in.get(), out.get(), msg), TRX_E_ARG, (who + ": " + F.count0).c_str());
    REFUSED(run(I.S, 0, nullptr, nullptr, msg), TRX_E_ARG, (who + ": " + F.count0).c_str());
    REFUSED(run(I.S, 3, nullptr, nullptr, msg), TRX_E_ARG, (who + ": " + F.in_name + " is NULL").c_str());
    REFUSED(run(I.S, 3, in.get(), nullptr, msg), TRX_E_ARG, (who + ": mom is NULL").c_str());
    ACCEPTED(run(I.S, 3, in.get(), out.get(), msg));
  }
  REFUSED(observed_run_checks(I.S, "trx_run_moments", ObservedRun::Moments, 4, in.get(), out.get(), "mom", msg), TRX_E_ARG, "trx_run_moments: nshift 4 is not the observed set's nexp 3");
  REFUSED(observed_run_checks(I.S, "trx_run_moments", ObservedRun::Moments, 2, in.get(), out.get(), "mom", msg), TRX_E_ARG, "trx_run_moments: nshift 2 is not the observed set's nexp 3");
  ACCEPTED(observed_run_checks(I.S, "trx_run_trail", ObservedRun::Trail, 1, in.get(), out.get(), "trail", msg));      // (a trail takes any number of lags)
}

static void trail_refusals()
{
  Installed I;
  Heap<double> out(1), none(0), one{1.0}, lag{1.0, 1.0001, 0.9999};
  // (the counts first: a refused nlag is not an extent to read lag[] over)
  REFUSED(trail_run_checks(I.S, "trx_run_trail", 0, none.get(), out.get(), "trail", msg), TRX_E_ARG, "trx_run_trail: nlag < 1");
  REFUSED(trail_run_checks(I.S, "trx_run_trail", -3, none.get(), out.get(), "trail", msg), TRX_E_ARG, "trx_run_trail: nlag < 1");
  REFUSED(trail_run_checks(I.S, "trx_run_trail", 3, nullptr, nullptr, "trail", msg), TRX_E_ARG, "trx_run_trail: lag is NULL");
  REFUSED(trail_run_checks(I.S, "trx_run_trail", 3, lag.get(), nullptr, "trail", msg), TRX_E_ARG, "trx_run_trail: trail is NULL");
  REFUSED(trail_run_checks(I.S, "trx_run_velocity_map", 3, lag.get(), nullptr, "map", msg), TRX_E_ARG, "trx_run_velocity_map: map is NULL");
  ProductState B = I.S; B.npix = 0x7fffffffLL;
  ACCEPTED(trail_run_checks(B, "trx_run_trail", 1, one.get(), out.get(), "trail", msg));
  REFUSED(trail_run_checks(B, "trx_run_trail", 257, one.get(), out.get(), "trail", msg), TRX_E_ARG, "trx_run_trail: nlag * npix above what one pixel launch takes");
  B = I.S; B.nexp = 32768; B.nseg = 32768;
  REFUSED(trail_run_checks(B, "trx_run_trail", 2, one.get(), out.get(), "trail", msg), TRX_E_ARG, "trx_run_trail: nlag * nexp * nseg above 2^31 - 1");
  B.npix = 0x7fffffffLL;                                 // (both: the pixel launch's first)
  REFUSED(trail_run_checks(B, "trx_run_batch_velocity_map", 257, one.get(), out.get(), "map", msg), TRX_E_ARG, "trx_run_batch_velocity_map: nlag * npix above what one pixel launch takes");
  ACCEPTED(trail_run_checks(I.S, "trx_run_trail", 3, lag.get(), out.get(), "trail", msg));
  lag[2] = 0.0;
  REFUSED(trail_run_checks(I.S, "trx_run_trail", 3, lag.get(), out.get(), "trail", msg), TRX_E_ARG, "trx_run_trail: lag 2 must be finite and > 0");
  lag[0] = kInf; lag[1] = kNaN;
  REFUSED(trail_run_checks(I.S, "trx_run_trail", 3, lag.get(), out.get(), "trail", msg), TRX_E_ARG, "trx_run_trail: lag 0 must be finite and > 0");
}

static void map_refusals()
{
  const Installed I;
  const char *who = "trx_run_velocity_map";
  Heap<double> out(1), lag{0.9999, 1.0, 1.0001}, kms{-3.0, 0.0, 3.0}, kp{100.0, 150.0}, vsys{-5.0, 0.0, 5.0, 10.0}, orbit{0.1, 0.2, 0.3}, offset{0.0, 0.5, 1.0};
  auto good = [&]() { trx_vmap V{}; V.stat = TRX_STAT_CCF; V.nlag = 3; V.lag = lag.get(); V.lag_kms = kms.get(); V.nkp = 2; V.nvsys = 4; V.kp = kp.get(); V.vsys = vsys.get();
                      V.orbit = orbit.get(); V.offset = offset.get(); return V; };
  trx_vmap V = good();
  ACCEPTED(velocity_map_checks(I.S, who, &V, out.get(), msg));
  V.offset = nullptr; V.stat = TRX_STAT_CHI2;
  ACCEPTED(velocity_map_checks(I.S, who, &V, out.get(), msg));
  REFUSED(velocity_map_checks(I.S, "trx_run_batch_velocity_map", nullptr, nullptr, msg), TRX_E_ARG, "trx_run_batch_velocity_map: vm is NULL");
  // a trail run's refusals come before the map's own: everything below is wrong as well
  trx_vmap bad{}; bad.stat = 9; bad.p0 = kNaN;
  ProductState W = I.S; W.windowed = true;
  REFUSED(velocity_map_checks(W, who, &bad, nullptr, msg), TRX_E_UNSUPPORTED,
          "trx_run_velocity_map: this handle's shard is not the whole grid; take trx_run_pixels, add the ranks' pairs (trx_gather_host) and reduce them on the host");
  ProductState N = I.S; N.seg = nullptr; N.nexp = N.nseg = 0;
  REFUSED(velocity_map_checks(N, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_velocity_map: no observed set installed (trx_set_observed)");
  REFUSED(velocity_map_checks(I.S, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_velocity_map: nlag < 1");
  bad.nlag = 3;
  REFUSED(velocity_map_checks(I.S, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_velocity_map: lag is NULL");
  bad.lag = lag.get();
  REFUSED(velocity_map_checks(I.S, who, &bad, nullptr, msg), TRX_E_ARG, "trx_run_velocity_map: map is NULL");
  lag[1] = -1.0;
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: lag 1 must be finite and > 0");
  lag[1] = 1.0;
  // the map's own, in order
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: unknown stat 9");
  bad.stat = TRX_STAT_LOGLIKE_BL19;
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: nkp < 1 or nvsys < 1");
  bad.nkp = 2;
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: nkp < 1 or nvsys < 1");
  bad.nkp = 65536; bad.nvsys = 32768;
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: nkp * nvsys above 2^31 - 1");
  bad.nkp = 2; bad.nvsys = 4;
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: lag_kms is NULL");
  bad.lag_kms = kms.get();
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: kp is NULL");
  bad.kp = kp.get();
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: vsys is NULL");
  bad.vsys = vsys.get();
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: orbit is NULL");
  bad.orbit = orbit.get(); bad.p1 = kInf;
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: p0 must be finite");
  bad.p0 = 1.0;
  REFUSED(velocity_map_checks(I.S, who, &bad, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: p1 must be finite");
  // the arrays: kp, vsys, orbit, offset, then the lags' velocities
  V = good();
  kp[1] = kNaN; vsys[3] = kInf; orbit[2] = kNaN; offset[0] = kInf; kms[1] = kNaN;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: kp 1 must be finite");
  kp[1] = 150.0;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: vsys 3 must be finite");
  vsys[3] = 10.0;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: orbit 2 must be finite");
  orbit[2] = 0.3;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: offset 0 must be finite");
  offset[0] = 0.0;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: lag_kms 1 must be finite and above the one before it (strictly increasing)");
  kms[1] = 3.0;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: lag_kms 2 must be finite and above the one before it (strictly increasing)");
  kms[1] = -3.0;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: lag_kms 1 must be finite and above the one before it (strictly increasing)");
  kms[0] = kInf; kms[1] = 0.0;
  REFUSED(velocity_map_checks(I.S, who, &V, out.get(), msg), TRX_E_ARG, "trx_run_velocity_map: lag_kms 0 must be finite and above the one before it (strictly increasing)");
}

static void filter_refusals()
{
  const Installed I;
  Heap<double> fwd(2 * 2 * 3, 0.5), back(2 * 3 * 2, 0.25);      // [nseg][ncomp][nexp], [nseg][nexp][ncomp]: ncomp = 2
  auto set = [&](int32_t ncomp, const double *f, const double *b) { trx_filter F{}; F.ncomp = ncomp; F.fwd = f; F.back = b; return F; };
  trx_filter F = set(-1, nullptr, nullptr);
  ProductState N = I.S; N.seg = nullptr; N.nexp = N.nseg = 0;
  REFUSED(filter_set_checks(N, &F, msg), TRX_E_ARG, "filter: no observed set installed (trx_set_observed)");
  N = I.S; N.npix = 0;
  REFUSED(filter_set_checks(N, &F, msg), TRX_E_ARG, "filter: no observed set installed (trx_set_observed)");
  REFUSED(filter_set_checks(I.S, &F, msg), TRX_E_ARG, "filter: ncomp < 0");
  F.ncomp = 17;
  REFUSED(filter_set_checks(I.S, &F, msg), TRX_E_ARG, "filter: ncomp above TRX_FILTER_MAX (16)");
  F.ncomp = 2;
  REFUSED(filter_set_checks(I.S, &F, msg), TRX_E_ARG, "filter: NULL fwd or back array");
  F.fwd = fwd.get();
  REFUSED(filter_set_checks(I.S, &F, msg), TRX_E_ARG, "filter: NULL fwd or back array");
  F.back = back.get();
  ACCEPTED(filter_set_checks(I.S, &F, msg));
  fwd[7] = kNaN; back[6] = kInf; back[1] = kNaN;         // (by segment, then by entry, fwd before back)
  REFUSED(filter_set_checks(I.S, &F, msg), TRX_E_ARG, "filter: segment 0: back entry must be finite");
  back[1] = 0.25;
  REFUSED(filter_set_checks(I.S, &F, msg), TRX_E_ARG, "filter: segment 1: back entry must be finite");
  back[6] = 0.25; back[7] = -kInf;
  REFUSED(filter_set_checks(I.S, &F, msg), TRX_E_ARG, "filter: segment 1: fwd entry must be finite");
}

static void broadening_refusals()
{
  const Installed I;
  int hmax = -1;
  auto set = [](int32_t kind, double beta, double limb) { trx_broadening B{}; B.kind = kind; B.beta = beta; B.limb = limb; return B; };
  ProductState W = I.S; W.windowed = true; W.wn_i = 0.0;
  trx_broadening B = set(5, kNaN, 2.0);
  REFUSED(broadening_checks(W, &B, hmax, msg), TRX_E_ARG, "broadening: unknown kind 5");
  for (double beta : {kNaN, kInf, 0.0, -1e-5}) {
    B = set(TRX_BROADEN_ROTATION, beta, 2.0);
    REFUSED(broadening_checks(W, &B, hmax, msg), TRX_E_ARG, "broadening: beta must be finite and > 0");
  }
  for (double limb : {kNaN, kInf, -0.1, 1.5}) {
    B = set(TRX_BROADEN_ROTATION, 1e-5, limb);
    REFUSED(broadening_checks(W, &B, hmax, msg), TRX_E_ARG, "broadening: limb must be finite and in [0, 1]");
  }
  B = set(TRX_BROADEN_ROTATION, 1e-5, 0.6);
  REFUSED(broadening_checks(W, &B, hmax, msg), TRX_E_ARG, "broadening: the handle's grid needs wn_i > 0 and wn_d > 0");
  W.wn_i = 2000.0; W.wn_d = 0.0;
  REFUSED(broadening_checks(W, &B, hmax, msg), TRX_E_ARG, "broadening: the handle's grid needs wn_i > 0 and wn_d > 0");
  W.wn_d = 0.1; B.beta = 1.0;                            // (and far too wide)
  REFUSED(broadening_checks(W, &B, hmax, msg), TRX_E_UNSUPPORTED,
          "broadening: this handle's shard is not the whole grid; gather the spectrum (trx_gather_host) and broaden it on the host");
  // the last bin is at 2000 + 4999 * 0.1 = 2499.9 cm-1: beta = 0.1 gives 249.99 cm-1 = 2499 whole bins
  B.beta = 0.1;
  REFUSED(broadening_checks(I.S, &B, hmax, msg), TRX_E_ARG, "broadening: half-width of 2499 bins at the grid's last bin is above TRX_BROADEN_MAX_HALF (2048)");
  CHECK(hmax == -1);
  B.beta = 0.01;                                         // 24.999 cm-1: 249 bins
  ACCEPTED(broadening_checks(I.S, &B, hmax, msg));
  CHECK(hmax == 249);
  B.beta = 1e-9; B.limb = 0.0;
  ACCEPTED(broadening_checks(I.S, &B, hmax, msg));
  CHECK(hmax == 0);
}

static void batch_rows_refusals()
{
  Heap<double> x(1);
  const double *a[3] = {x.get(), x.get(), x.get()}, *b[3] = {x.get(), x.get(), x.get()};
  ACCEPTED(batch_rows_check("trx_run_batch_moments", 3, {{"shift", a}, {"mom", b}}, msg));
  ACCEPTED(batch_rows_check("trx_run_batch_velocity_map", 3, {{"map", a}, {"per", nullptr}}, msg));      // (an optional array left out)
  a[1] = nullptr;
  ACCEPTED(batch_rows_check("trx_run_batch_moments", 1, {{"shift", a}, {"mom", b}}, msg));               // (rows past k are not looked at)
  ACCEPTED(batch_rows_check("trx_run_batch_moments", 0, {{"shift", nullptr}, {"mom", nullptr}}, msg));
  REFUSED(batch_rows_check("trx_run_batch_moments", 3, {{"shift", a}, {"mom", b}}, msg), TRX_E_ARG, "trx_run_batch_moments: shift[1] is NULL");
  b[1] = nullptr;                                        // by atmosphere first, then in the order of the arrays
  REFUSED(batch_rows_check("trx_run_batch_trail", 3, {{"lag", a}, {"trail", b}}, msg), TRX_E_ARG, "trx_run_batch_trail: lag[1] is NULL");
  b[0] = nullptr;
  REFUSED(batch_rows_check("trx_run_batch_trail", 3, {{"lag", a}, {"trail", b}}, msg), TRX_E_ARG, "trx_run_batch_trail: trail[0] is NULL");
  REFUSED(batch_rows_check("trx_run_batch_bands", 3, {{"sums", b}}, msg), TRX_E_ARG, "trx_run_batch_bands: sums[0] is NULL");
}

// ---- the band layout ---------------------------------------------------------------------------------
// [first, last) of a GAUSS band one bin at a time: bin i is in when a <= i <= z in double, a and z the window's edges in bins
static void gauss_members(const ProductState &S, const trx_band &B, int64_t &first, int64_t &last)
{
  const double sigma = B.fwhm / (2.0 * std::sqrt(2.0 * std::log(2.0)));
  const double a = (B.centre - B.cut * sigma - S.wn_i) / S.wn_d, z = (B.centre + B.cut * sigma - S.wn_i) / S.wn_d;
  int64_t n = 0; first = -1;
  for (int64_t i = 0; i < S.nwn; i++)
    if (a <= (double)i && (double)i <= z) { if (first < 0) first = i; n++; CHECK(i == first + n - 1); }
  if (first < 0) first = a > (double)(S.nwn - 1) ? S.nwn : 0;      // (empty: where the rule's clipping leaves it does not matter to a shard)
  last = first + n;
}

static void print_gauss(double wn_i, double wn_d, int64_t nwn, double centre, double fwhm, double cut)
{
  int64_t first, last;
  gauss_band_range(wn_i, wn_d, nwn, centre, fwhm / (2.0 * std::sqrt(2.0 * std::log(2.0))), cut, first, last);
  std::printf("gauss %a %a %lld %a %a %a %lld %lld\n", wn_i, wn_d, (long long)nwn, centre, fwhm, cut, (long long)first, (long long)last);
}

// the layout of `bands` on shard [lo, hi) of the 5000-bin grid against the rule written out: every band's pieces tile its
// in-shard bins once, in order; s, piece0, npieces and woff agree with them; the weights are the in-shard slice
static void check_layout(const std::vector<trx_band> &set, int64_t lo, int64_t hi)
{
  ProductState S; S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.lo = lo; S.hi = hi; S.windowed = lo > 0 || hi < 5000;
  Heap<trx_band> bands(set.size());
  for (size_t b = 0; b < set.size(); b++) bands[b] = set[b];
  BandLayout L; std::string msg;
  const int rc = band_layout(S, (int32_t)set.size(), bands.get(), L, msg);
  CHECK(rc == TRX_OK && msg.empty());
  CHECK(L.bands.size() == set.size());
  if (rc != TRX_OK || L.bands.size() != set.size()) return;
  int64_t piece = 0, wat = 0;
  for (size_t b = 0; b < set.size(); b++) {
    const trx_band &B = set[b]; const BandDev &D = L.bands[b];
    int64_t first, last;
    if (B.kind == TRX_BAND_WEIGHTS) { first = B.first; last = B.first + B.n; }
    else gauss_members(S, B, first, last);
    const int64_t s = std::max(first, lo), e = std::min(last, hi);
    CHECK(D.kind == B.kind && D.pad == 0 && D.piece0 == piece && D.woff == wat);
    if (B.kind == TRX_BAND_GAUSS) CHECK(D.centre == B.centre && D.sigma == B.fwhm / (2.0 * std::sqrt(2.0 * std::log(2.0))));
    if (e <= s) { CHECK(D.s == 0 && D.npieces == 0); continue; }
    CHECK(D.s == s - lo && D.npieces == (e - s + kBandPiece - 1) / kBandPiece);
    CHECK(piece + D.npieces <= (int64_t)L.pieces.size());
    if (piece + D.npieces > (int64_t)L.pieces.size()) return;
    int64_t at = s - lo;
    for (int64_t k = 0; k < D.npieces; k++) {
      const BandPiece &P = L.pieces[(size_t)(piece + k)];
      CHECK(P.band == (int32_t)b && P.start == at && P.len >= 1 && P.len <= kBandPiece);
      CHECK(k + 1 == D.npieces || P.len == kBandPiece);
      at += P.len;
    }
    CHECK(at == e - lo);
    piece += D.npieces;
    if (B.kind == TRX_BAND_WEIGHTS) {
      CHECK(wat + (e - s) <= (int64_t)L.w.size());
      if (wat + (e - s) > (int64_t)L.w.size()) return;
      bool same = true;
      for (int64_t i = 0; i < e - s; i++) same = same && L.w[(size_t)(wat + i)] == B.weights[s - first + i];
      CHECK(same);
      wat += e - s;
    }
  }
  CHECK(piece == (int64_t)L.pieces.size() && wat == (int64_t)L.w.size());
}

static void band_layouts()
{
  static_assert(kBandPiece == 1024, "the piece the cases below are cut for");
  // WEIGHTS of 1, kBandPiece - 1, kBandPiece, kBandPiece + 1 and 3 kBandPiece bins, each its own exact-size array: bands
  // that straddle bin 1000, straddle bin 2000, lie inside [1000, 2000) and lie outside it
  std::vector<Heap<double>> w;
  std::vector<trx_band> set;
  const int64_t lens[] = {1, kBandPiece - 1, kBandPiece, kBandPiece + 1, 3 * kBandPiece};
  const int64_t firsts[] = {0, 999, 1000, 1500, 1999, 2000, 3000};
  for (int64_t n : lens)
    for (int64_t first : firsts) {
      if (first + n > 5000) continue;
      w.emplace_back((size_t)n);
      for (int64_t k = 0; k < n; k++) w.back()[(size_t)k] = 0.5 + (double)(first + 7 * k);
    }
  size_t at = 0;
  for (int64_t n : lens)
    for (int64_t first : firsts) {
      if (first + n > 5000) continue;
      set.push_back(weights_band(first, n, w[at++].get()));
    }
  set.push_back(weights_band(4999, 1, w[0].get()));
  // GAUSS: inside, clipped at 0, clipped at nwn, wholly off either end, centres of +-1e300, edges on grid points (sigma = 0.5
  // exactly: 4 sigmas are 20 bins), a window narrower than a bin
  const double on_grid = 0.5 * (2.0 * std::sqrt(2.0 * std::log(2.0)));
  const trx_band g[] = {gauss_band(2100.03, 1.7, 4.0), gauss_band(2000.2, 3.0, 4.0), gauss_band(1999.0, 3.0, 3.0), gauss_band(2499.5, 3.0, 4.0),
                        gauss_band(2501.0, 2.0, 4.0), gauss_band(1500.0, 1.0, 4.0), gauss_band(3000.0, 1.0, 4.0), gauss_band(1e300, 1.0, 4.0),
                        gauss_band(-1e300, 1.0, 4.0), gauss_band(2100.0, on_grid, 4.0), gauss_band(2199.9, on_grid, 4.0), gauss_band(2200.04, 0.01, 1.0),
                        gauss_band(2150.0, 300.0, 4.0), gauss_band(2250.0, 1e6, 4.0)};
  for (const trx_band &B : g) { set.push_back(B); print_gauss(2000.0, 0.1, 5000, B.centre, B.fwhm, B.cut); }
  check_layout(set, 0, 5000);
  check_layout(set, 1000, 2000);
  check_layout(set, 0, 1000);
  check_layout(set, 2000, 5000);
  check_layout(set, 4999, 5000);
  check_layout({}, 0, 5000);
  // by hand: on the whole grid 4 sigmas of 0.5 cm-1 around bin 1000 are bins 980 .. 1020, both edges in
  ProductState S; S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.hi = 5000;
  Heap<trx_band> one{gauss_band(2100.0, on_grid, 4.0)};
  BandLayout L; std::string msg;
  CHECK(band_layout(S, 1, one.get(), L, msg) == TRX_OK && L.bands[0].s == 980 && L.pieces.size() == 1 && L.pieces[0].len == 41 && L.w.empty());
  S.lo = 1000; S.hi = 1010; S.windowed = true;
  CHECK(band_layout(S, 1, one.get(), L, msg) == TRX_OK && L.bands[0].s == 0 && L.pieces.size() == 1 && L.pieces[0].start == 0 && L.pieces[0].len == 10);
}

// ---- the filter layout -------------------------------------------------------------------------------
static void filter_layouts()
{
  // segments of 0, 1, 64, 65 and 129 pixels, and an empty one at the end
  Heap<int64_t> seg{0, 0, 1, 65, 130, 259, 259};
  ProductState S; S.nwn = 100; S.hi = 100; S.npix = 259; S.nexp = 3; S.nseg = 6; S.seg = seg.get();
  const size_t ne = 3, ns = 6;
  const int want_pad[17] = {0, 4, 4, 4, 4, 8, 8, 8, 8, 16, 16, 16, 16, 16, 16, 16, 16};
  for (int32_t ncomp : {1, 4, 5, 8, 9, 16, 3, 12}) {
    const size_t nc = (size_t)ncomp;
    Heap<double> fwd(ns * nc * ne), back(ns * ne * nc);
    for (size_t s = 0; s < ns; s++)
      for (size_t j = 0; j < nc; j++)
        for (size_t v = 0; v < ne; v++) {
          fwd[(s * nc + j) * ne + v] = -(1.0 + (double)(s * 1000 + j * 10 + v));      // (negative: a padded entry copied from a neighbour would show its sign)
          back[(s * ne + v) * nc + j] = -(0.5 + (double)(s * 1000 + j * 10 + v));
        }
    trx_filter F{}; F.ncomp = ncomp; F.fwd = fwd.get(); F.back = back.get();
    FilterLayout L; std::string msg;
    CHECK(filter_set_checks(S, &F, msg) == TRX_OK);
    CHECK(filter_layout(S, &F, L, msg) == TRX_OK && msg.empty());
    CHECK(L.npad == want_pad[ncomp]);
    const size_t np = (size_t)L.npad;
    CHECK(L.fwd.size() == ns * ne * np && L.back.size() == ns * ne * np);
    if (L.fwd.size() != ns * ne * np || L.back.size() != ns * ne * np) continue;
    bool values = true, zeros = true;
    for (size_t s = 0; s < ns; s++)
      for (size_t v = 0; v < ne; v++)
        for (size_t j = 0; j < np; j++) {
          const double f = L.fwd[s * ne * np + v * np + j], b = L.back[s * ne * np + v * np + j];
          if (j < nc) values = values && f == -(1.0 + (double)(s * 1000 + j * 10 + v)) && b == -(0.5 + (double)(s * 1000 + j * 10 + v));
          else zeros = zeros && f == 0.0 && !std::signbit(f) && b == 0.0 && !std::signbit(b);
        }
    CHECK(values); CHECK(zeros);
    // the tiles partition each segment in pixel order, 1 .. 64 pixels each, all but a segment's last full; none for an empty one
    size_t t = 0; bool tiles = true;
    for (int32_t s = 0; s < S.nseg; s++) {
      int64_t p = seg[(size_t)s];
      while (p < seg[(size_t)s + 1]) {
        if (t >= L.tiles.size()) { tiles = false; break; }
        const FilterTile &T = L.tiles[t++];
        tiles = tiles && T.seg == s && T.first == p && T.count >= 1 && T.count <= 64 && (T.count == 64 || p + T.count == seg[(size_t)s + 1]);
        p += T.count > 0 ? T.count : 1;
      }
      tiles = tiles && p == seg[(size_t)s + 1];
    }
    CHECK(tiles && t == L.tiles.size());
    CHECK(L.tiles.size() == 0 + 1 + 1 + 2 + 3 + 0);
  }
}

// ---- the extents -------------------------------------------------------------------------------------
static void extents()
{
  static_assert(TRX_NMOMENT == 7 && kPixBlock == 256 && kContribSplit == 4, "the numbers below are worked for these");
  // the documented trail shape: 201 lags, 100 exposures, 40 segments, 81 920 pixels
  PixelExtents X = pixel_extents(81920, 201, 100, 40, false, true);
  CHECK(X.pairs == 16465920 && X.blocks == 64320 && X.rows == 804000);
  CHECK(X.shift_bytes == 1608 && X.pair_bytes == 263454720 && X.trail_bytes == 45024000 && X.mom_bytes == 0 && X.val_bytes == 0);
  // the same sets' moment run (one shift per exposure), without and with the filter, and the plain pixel run
  X = pixel_extents(81920, 100, 100, 40, false, false);
  CHECK(X.pairs == 8192000 && X.blocks == 32000 && X.rows == 4000);
  CHECK(X.shift_bytes == 800 && X.pair_bytes == 131072000 && X.mom_bytes == 224000 && X.trail_bytes == 0 && X.val_bytes == 0);
  X = pixel_extents(81920, 100, 100, 40, true, false);
  CHECK(X.pairs == 8192000 && X.blocks == 32000 && X.rows == 4000);
  CHECK(X.shift_bytes == 800 && X.pair_bytes == 131072000 && X.mom_bytes == 224000 && X.trail_bytes == 0 && X.val_bytes == 65536000);
  X = pixel_extents(81920, 100, 0, 0, false, false);
  CHECK(X.pairs == 8192000 && X.blocks == 32000 && X.rows == 0);
  CHECK(X.shift_bytes == 800 && X.pair_bytes == 131072000 && X.mom_bytes == 0 && X.trail_bytes == 0 && X.val_bytes == 0);
  // the smallest: 1, 1, 1, 1
  X = pixel_extents(1, 1, 1, 1, false, true);
  CHECK(X.pairs == 1 && X.blocks == 1 && X.rows == 1 && X.shift_bytes == 8 && X.pair_bytes == 16 && X.trail_bytes == 56 && X.mom_bytes == 0 && X.val_bytes == 0);
  X = pixel_extents(1, 1, 1, 1, true, false);
  CHECK(X.pairs == 1 && X.blocks == 1 && X.rows == 1 && X.shift_bytes == 8 && X.pair_bytes == 16 && X.trail_bytes == 0 && X.mom_bytes == 56 && X.val_bytes == 8);
  X = pixel_extents(1, 1, 0, 0, false, false);
  CHECK(X.pairs == 1 && X.blocks == 1 && X.rows == 0 && X.shift_bytes == 8 && X.pair_bytes == 16 && X.trail_bytes == 0 && X.mom_bytes == 0 && X.val_bytes == 0);
  // a block boundary: 257 pairs are two blocks
  CHECK(pixel_extents(257, 1, 0, 0, false, false).blocks == 2 && pixel_extents(256, 1, 0, 0, false, false).blocks == 1);
  // the largest a trail run admits (trail_run_checks): 2^31 - 1 rows
  CHECK(pixel_extents(1, 0x7fffffff, 1, 1, false, true).trail_bytes == 56ull * 0x7fffffffull);

  // the map over that trail: 3 Kp by 5 Vsys, with and without the offsets; its packing on exact-size arrays
  Heap<double> lag(201, 1.0), kms(201), kp{1.0, 2.0, 3.0}, vsys{-2.0, -1.0, 0.0, 1.0, 2.0}, orbit(100), offset(100);
  for (size_t i = 0; i < 201; i++) kms[i] = 1000.0 + (double)i;
  for (size_t i = 0; i < 100; i++) { orbit[i] = 2000.0 + (double)i; offset[i] = 3000.0 + (double)i; }
  trx_vmap V{}; V.stat = TRX_STAT_CCF; V.nlag = 201; V.lag = lag.get(); V.lag_kms = kms.get(); V.nkp = 3; V.nvsys = 5; V.kp = kp.get(); V.vsys = vsys.get();
  V.orbit = orbit.get(); V.offset = offset.get();
  VmapExtents M = vmap_extents(V, 100);
  CHECK(M.at_kp == 201 && M.at_vsys == 204 && M.at_orbit == 209 && M.at_offset == 309 && M.nin == 409 && M.rows == 20100 && M.cells == 15);
  CHECK(M.in_bytes == 3272 && M.per_bytes == 160800 && M.per2_bytes == 321600 && M.map_bytes == 120);
  std::vector<double> in(7, -1.0); std::string msg;
  CHECK(vmap_pack("trx_run_velocity_map", V, M, in, msg) == TRX_OK && msg.empty() && in.size() == 409);
  CHECK(in[0] == 1000.0 && in[200] == 1200.0 && in[201] == 1.0 && in[203] == 3.0 && in[204] == -2.0 && in[208] == 2.0 && in[209] == 2000.0 && in[308] == 2099.0 &&
        in[309] == 3000.0 && in[408] == 3099.0);
  V.offset = nullptr;
  M = vmap_extents(V, 100);
  CHECK(M.at_kp == 201 && M.at_vsys == 204 && M.at_orbit == 209 && M.at_offset == 309 && M.nin == 309 && M.rows == 20100 && M.cells == 15);
  CHECK(M.in_bytes == 2472 && M.per_bytes == 160800 && M.per2_bytes == 321600 && M.map_bytes == 120);
  CHECK(vmap_pack("trx_run_velocity_map", V, M, in, msg) == TRX_OK && in.size() == 309 && in[308] == 2099.0);
  Heap<double> a{5.0}, b{6.0}, c{7.0}, d{8.0}, e{9.0};
  trx_vmap W{}; W.stat = TRX_STAT_CCF; W.nlag = 1; W.lag = a.get(); W.lag_kms = a.get(); W.nkp = 1; W.nvsys = 1; W.kp = b.get(); W.vsys = c.get(); W.orbit = d.get(); W.offset = e.get();
  M = vmap_extents(W, 1);
  CHECK(M.at_kp == 1 && M.at_vsys == 2 && M.at_orbit == 3 && M.at_offset == 4 && M.nin == 5 && M.rows == 1 && M.cells == 1);
  CHECK(M.in_bytes == 40 && M.per_bytes == 8 && M.per2_bytes == 16 && M.map_bytes == 8);
  CHECK(vmap_pack("trx_run_velocity_map", W, M, in, msg) == TRX_OK && in == std::vector<double>({5.0, 6.0, 7.0, 8.0, 9.0}));
  W.offset = nullptr;
  M = vmap_extents(W, 1);
  CHECK(M.nin == 4 && M.in_bytes == 32 && M.at_offset == 4);
  CHECK(vmap_pack("trx_run_velocity_map", W, M, in, msg) == TRX_OK && in == std::vector<double>({5.0, 6.0, 7.0, 8.0}));

  // a contribution run of 100 layers over 7 pieces of 3 bands: four sub-pieces per piece; and the smallest
  ContribExtents C = contrib_extents(100, 7, 3);
  CHECK(C.cpart_bytes == 22400 && C.out_bytes == 2400);
  C = contrib_extents(1, 1, 1);
  CHECK(C.cpart_bytes == 32 && C.out_bytes == 8);
  CHECK(contrib_extents(5, 0, 2).cpart_bytes == 0);
  CHECK(broadened_bytes(5000) == 40000 && broadened_bytes(1) == 8);
}

// ---- the launch conditions (transit_amd/csrc/trx_launch.h) -------------------------------------------
// the sets as plain structs: a buffer is a pointer that is never followed and a byte count
struct PlainBuf { void *p = nullptr; size_t bytes = 0; void release() { p = nullptr; bytes = 0; } };
struct PlainObs {
  int32_t nexp = 0, nseg = 0; int64_t npix = 0; std::vector<int64_t> seg;
  PlainBuf d_seg, d_gain; InForce<PlainBuf> d_data, d_weight;
};
struct PlainFilt {
  int32_t ncomp = 0, npad = 0, nexp = 0, nseg = 0; int64_t npix = 0, ntiles = 0; bool weighted = false; int32_t nfac = 0;
  PlainBuf d_fwd, d_back, d_tiles, d_fac, d_live;
};
static char g_there;                                     // what a non-null pointer points at
static PlainBuf of(size_t bytes) { return PlainBuf{&g_there, bytes}; }

// the smallest shapes with every branch: 2 exposures, 2 segments -- the first empty --, 3 pixels; a filter of 3 components
// padded to 4 with the one tile of the second segment
static PlainObs whole_obs(bool weights, bool gain)
{
  PlainObs O; O.nexp = 2; O.nseg = 2; O.npix = 3; O.seg = {0, 0, 3};
  O.d_seg = of(24); O.d_data.now = of(48);
  if (weights) O.d_weight.now = of(48);
  if (gain) O.d_gain = of(24);
  return O;
}
static PlainFilt whole_filt(bool weighted)
{
  PlainFilt F; F.ncomp = 3; F.npad = 4; F.nexp = 2; F.nseg = 2; F.npix = 3; F.ntiles = 1; F.weighted = weighted;
  F.d_back = of(128); F.d_tiles = of(sizeof(FilterTile));
  if (weighted) { F.nfac = 6; F.d_fac = of(144); F.d_live = of(12); } else F.d_fwd = of(128);
  return F;
}

static void grid_conditions()
{
  int64_t blocks = -1;
  CHECK(!blocks_for(0, 4, &blocks) && blocks == 0);
  CHECK(blocks_for(1, 4, &blocks) && blocks == 1);
  CHECK(blocks_for(5, 4, &blocks) && blocks == 2);
  CHECK(blocks_for(0x7fffffffLL * 4, 4, &blocks) && blocks == 0x7fffffffLL);
  CHECK(!blocks_for(0x7fffffffLL * 4 + 1, 4, &blocks) && blocks == 0x80000000LL);
  CHECK(!grid_ok(0) && grid_ok(1) && grid_ok(0x7fffffffLL) && !grid_ok(0x80000000LL) && !grid_ok(-1));
  for (int32_t npad = -1; npad <= 33; npad++) CHECK(npad_ok(npad) == (npad == 4 || npad == 8 || npad == 16));
}

static void observed_set_conditions()
{
  for (const bool weights : {false, true})
    for (const bool gain : {false, true}) {
      const PlainObs O = whole_obs(weights, gain);
      CHECK(observed_set_whole(O, O.d_weight.now, true) && observed_set_whole(O, O.d_weight.now, false));
      // one defect each: refused whether or not the data are read, unless the defect is the data's
      auto refused_with = [&](void (*spoil)(PlainObs &), bool data_only = false) {
        PlainObs B = whole_obs(weights, gain); spoil(B);
        CHECK(!observed_set_whole(B, B.d_weight.now, true) && observed_set_whole(B, B.d_weight.now, false) == data_only);
      };
      refused_with([](PlainObs &B) { B.d_seg.p = nullptr; });
      refused_with([](PlainObs &B) { B.d_seg.bytes--; });
      refused_with([](PlainObs &B) { B.d_data.now.p = nullptr; }, true);
      refused_with([](PlainObs &B) { B.d_data.now.bytes--; }, true);
      refused_with([](PlainObs &B) { B.nexp++; }, !weights);           // (the data, and the weights where there are any, are one exposure short)
      refused_with([](PlainObs &B) { B.nexp = 0; });
      refused_with([](PlainObs &B) { B.nseg++; });
      refused_with([](PlainObs &B) { B.nseg--; });
      refused_with([](PlainObs &B) { B.npix++; });
      refused_with([](PlainObs &B) { B.npix--; });
      refused_with([](PlainObs &B) { B.seg.front() = 1; });
      refused_with([](PlainObs &B) { B.seg.back() = 2; });
      if (weights) refused_with([](PlainObs &B) { B.d_weight.now.bytes--; });
      if (gain) refused_with([](PlainObs &B) { B.d_gain.bytes--; });
      // the weights a caller names are the ones held against the extent: the raw ones of a weighed set
      PlainObs W = whole_obs(weights, gain);
      PlainBuf fresh = of(47);
      W.d_weight.adopt(fresh);
      CHECK(!observed_set_whole(W, W.d_weight.now, true) && observed_set_whole(W, W.d_weight.raw(), true));
    }
}

static void filter_set_conditions()
{
  for (const bool weighted : {false, true}) {
    auto whole = [&](const PlainFilt &F, const PlainObs &O) { return weighted ? wfilter_set_complete(F, O) : filter_set_whole(F, O); };
    const PlainObs O = whole_obs(true, true);
    CHECK(whole(whole_filt(weighted), O) && whole(whole_filt(weighted), whole_obs(false, false)));
    CHECK(!(weighted ? filter_set_whole(whole_filt(true), O) : wfilter_set_complete(whole_filt(false), O)));      // (the other kind's predicate)
    auto refused_with = [&](void (*spoil)(PlainFilt &)) { PlainFilt B = whole_filt(weighted); spoil(B); CHECK(!whole(B, O)); };
    refused_with([](PlainFilt &B) { B.d_back.p = nullptr; });
    refused_with([](PlainFilt &B) { B.d_back.bytes--; });
    refused_with([](PlainFilt &B) { B.d_tiles.p = nullptr; });
    refused_with([](PlainFilt &B) { B.d_tiles.bytes--; });
    refused_with([](PlainFilt &B) { B.weighted = !B.weighted; });
    refused_with([](PlainFilt &B) { B.nexp++; });
    refused_with([](PlainFilt &B) { B.nexp--; });
    refused_with([](PlainFilt &B) { B.nseg++; });
    refused_with([](PlainFilt &B) { B.nseg--; });
    refused_with([](PlainFilt &B) { B.npix++; });
    refused_with([](PlainFilt &B) { B.npix--; });
    refused_with([](PlainFilt &B) { B.ncomp = 0; });
    refused_with([](PlainFilt &B) { B.ncomp = 5; B.nfac = 15; B.d_fac.bytes = 1 << 20; });      // ncomp > npad
    refused_with([](PlainFilt &B) { B.ntiles = 0; });
    // a padded count no kernel is made for, behind buffers that would hold it
    for (const int32_t npad : {0, 3, 5, 12, 32}) {
      PlainFilt B = whole_filt(weighted); B.npad = npad; B.d_fwd.bytes = B.d_back.bytes = 1 << 20;
      if (npad < B.ncomp) { B.ncomp = 1; B.nfac = 1; }
      CHECK(!whole(B, O));
      B.npad = 16; CHECK(whole(B, O));                                       // (the count alone refused it)
    }
    if (weighted) {
      refused_with([](PlainFilt &B) { B.d_fac.p = nullptr; });
      refused_with([](PlainFilt &B) { B.d_fac.bytes--; });
      refused_with([](PlainFilt &B) { B.d_live.p = nullptr; });
      refused_with([](PlainFilt &B) { B.d_live.bytes--; });
      refused_with([](PlainFilt &B) { B.nfac++; });
      PlainObs S = whole_obs(true, true); S.d_weight.now.bytes--;
      CHECK(!wfilter_set_complete(whole_filt(true), S));                      // the weights in force, one byte short
      // what the factor kernel reads is whole without a factor, and with other weights in force
      PlainFilt B = whole_filt(true); B.d_fac = B.d_live = PlainBuf{};
      const WfilterExtents WX = wfilter_extents(B.npix, B.nexp, B.nseg, B.ncomp, B.npad, B.ntiles, 4);
      CHECK(wfilter_basis_whole(B, S, WX) && !wfilter_set_complete(B, O));
      CHECK(WX.nfac == 6 && WX.basis_bytes == 128 && WX.fac_bytes == 144 && WX.live_bytes == 12 && WX.blocks == 1);
    } else {
      refused_with([](PlainFilt &B) { B.d_fwd.p = nullptr; });
      refused_with([](PlainFilt &B) { B.d_fwd.bytes--; });
    }
  }
}

static void pair_source_conditions()
{
  const PixelExtents X = pixel_extents(3, 2, 0, 0, false, false);
  const HighpassExtents HX = highpass_extents(3, 2, 1, 1);
  static char out_there, hp_there, gain_there;
  const PlainBuf out{&out_there, X.pair_bytes}, hp{&hp_there, HX.pair_bytes}, gain{&gain_there, 24}, none{};
  CHECK(X.pair_bytes == 96 && HX.pair_bytes == 96 && HX.pairs == X.pairs);
  // without a high-pass: the pixel kernel's pairs and the gains that apply
  PairSource P = pair_source(X, (const HighpassExtents *)nullptr, out, none, &gain, 3);
  CHECK(P.pairs == &out_there && P.gain == &gain_there && P.whole);
  P = pair_source(X, (const HighpassExtents *)nullptr, out, none, (const PlainBuf *)nullptr, 3);
  CHECK(P.pairs == &out_there && !P.gain && P.whole);
  P = pair_source(X, (const HighpassExtents *)nullptr, out, none, &none, 3);      // (a set without gains)
  CHECK(P.pairs == &out_there && !P.gain && P.whole);
  // with one: its pairs and no gain -- the high-pass applied it
  P = pair_source(X, &HX, out, hp, &gain, 3);
  CHECK(P.pairs == &hp_there && !P.gain && P.whole);
  // one defect each
  auto whole_with = [&](const HighpassExtents *hx, PlainBuf o, PlainBuf h, PlainBuf g, int64_t npix = 3) { return pair_source(X, hx, o, h, &g, npix).whole; };
  auto shorter = [](PlainBuf b) { b.bytes--; return b; };
  auto null_of = [](PlainBuf b) { b.p = nullptr; return b; };
  CHECK(!whole_with(nullptr, null_of(out), hp, gain) && !whole_with(nullptr, shorter(out), hp, gain) && !whole_with(nullptr, out, hp, shorter(gain)));
  CHECK(whole_with(nullptr, out, null_of(hp), gain) && whole_with(nullptr, out, shorter(hp), gain));      // (not read without a high-pass)
  CHECK(!whole_with(&HX, out, null_of(hp), gain) && !whole_with(&HX, out, shorter(hp), gain) && !whole_with(&HX, shorter(out), hp, gain));
  CHECK(whole_with(&HX, out, hp, shorter(gain)));                                                         // (not read behind a high-pass)
  HighpassExtents other = HX; other.pairs++;
  CHECK(!whole_with(&other, out, hp, gain));
  CHECK(!whole_with(nullptr, out, hp, gain, 0) && !whole_with(nullptr, out, hp, gain, 4));                // (the gains are npix long)
}

// a buffer that owns a heap block and counts: a leak or a double release is a count that is off, and a sanitizer report
struct CountedBuf {
  void *p = nullptr; size_t bytes = 0;
  static int live, released;
  CountedBuf() = default;
  explicit CountedBuf(size_t n) : p(std::malloc(n)), bytes(n) { live++; }
  CountedBuf(const CountedBuf &) = delete;
  CountedBuf &operator=(const CountedBuf &) = delete;
  ~CountedBuf() { release(); }
  void release() { if (p) { std::free(p); p = nullptr; bytes = 0; live--; released++; } }
};
int CountedBuf::live = 0, CountedBuf::released = 0;

static void in_force_transitions()
{
  auto empty = [](const CountedBuf &b) { return !b.p && b.bytes == 0; };
  {  // adopt, adopt, restore: the raw version aside, then the two calls' buffers swap, then the raw one back
    InForce<CountedBuf> S; CountedBuf raw(8), one(16), two(24), spare;
    const void *const A = raw.p, *const B = one.p, *const C = two.p;
    exchange_buf(S.now, raw);
    CHECK(S.raw().p == A && !S.adopted);
    S.adopt(one);
    CHECK(S.now.p == B && S.now.bytes == 16 && S.raw().p == A && S.raw().bytes == 8 && S.adopted && empty(one));
    S.adopt(two);
    CHECK(S.now.p == C && S.raw().p == A && two.p == B && two.bytes == 16 && S.adopted);
    S.restore(spare);
    CHECK(S.now.p == A && S.now.bytes == 8 && S.raw().p == A && !S.adopted && empty(S.aside) && spare.p == C && spare.bytes == 24);
    CHECK(CountedBuf::live == 3 && CountedBuf::released == 0);              // raw in force, `one` in two, `two` in spare
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 3);
  {  // restore without adopt: nothing moves
    InForce<CountedBuf> S; CountedBuf raw(8), spare;
    const void *const A = raw.p;
    exchange_buf(S.now, raw);
    S.restore(spare);
    CHECK(S.now.p == A && S.raw().p == A && !S.adopted && empty(spare) && empty(S.aside) && CountedBuf::live == 1);
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 4);
  {  // a set without weights: the empty raw version goes aside and comes back
    InForce<CountedBuf> S; CountedBuf one(16), spare;
    const void *const B = one.p;
    S.adopt(one);
    CHECK(S.now.p == B && S.adopted && empty(S.raw()) && empty(one));
    S.restore(spare);
    CHECK(empty(S.now) && empty(S.raw()) && !S.adopted && spare.p == B && CountedBuf::live == 1);
    S.adopt(spare);                                                       // (and again, from the spare)
    CHECK(S.now.p == B && empty(S.raw()) && empty(spare) && CountedBuf::live == 1);
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 5);
  {  // restore with a spare that is taken: the buffer that was in force is released, not leaked
    InForce<CountedBuf> S; CountedBuf raw(8), one(16), spare(32);
    const void *const A = raw.p, *const D = spare.p;
    exchange_buf(S.now, raw);
    S.adopt(one);
    S.restore(spare);
    CHECK(S.now.p == A && !S.adopted && empty(S.aside) && spare.p == D && spare.bytes == 32);
    CHECK(CountedBuf::live == 2 && CountedBuf::released == 6);
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 8);
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "gauss")) {
    std::FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::printf("cannot read %s\n", argv[2]); return 2; }
    char a[64], b[64], c[64], d[64], e[64]; long long nwn;
    while (std::fscanf(f, "%63s %63s %lld %63s %63s %63s", a, b, &nwn, c, d, e) == 6)
      print_gauss(std::strtod(a, nullptr), std::strtod(b, nullptr), nwn, std::strtod(c, nullptr), std::strtod(d, nullptr), std::strtod(e, nullptr));
    std::fclose(f);
    return 0;
  }
  band_refusals(); pixel_refusals(); observed_refusals(); observed_run_refusals(); trail_refusals(); map_refusals(); filter_refusals();
  broadening_refusals(); batch_rows_refusals();
  band_layouts(); filter_layouts(); extents();
  grid_conditions(); observed_set_conditions(); filter_set_conditions(); pair_source_conditions(); in_force_transitions();
  std::printf("%s %d\n", g_bad ? "bad" : "ok", g_checks);
  return g_bad ? 1 : 0;
}
