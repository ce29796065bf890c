// exposures_check.cpp -- the host side of the exposure table (transit_amd/csrc/trx_exposures.h) without a device: the refusals
// of trx_set_exposures and trx_run_exposed against literal texts, the extents, and the range rule the pixel kernel shares.
// Stand-alone (tests/test_exposures_host.py builds it under -fsanitize=address,undefined); every array handed to the header
// is a heap allocation of exactly the stated length, so a read past an extent is a sanitizer report.
//
//   exposures_check              every check; prints "range <wn_i> <wn_d> <nwn> <cut> <centre_obs> <fwhm_obs> <shift> <eta>
//                                <centre> <sigma> <d> <first> <last>" for its edge cases (doubles as %a) and "ok <checks>"
//   exposures_check range FILE   FILE: lines "wn_i wn_d nwn cut centre_obs fwhm_obs shift eta"; prints the same lines for them
#include <cmath>
#include <cstring>

#include "transit_hip.h"
#include "trx_exposures.h"
#include "check_common.h"

using namespace trx;

static_assert(sizeof(trx_exposures) == 24, "trx_exposures is 24 bytes");
static_assert(TRX_OK == 0 && TRX_E_ARG == -1, "the codes the tests of the interface pin");

static const double kFwhmSigma = 2.0 * std::sqrt(2.0 * std::log(2.0));

// a whole-grid handle of 5000 bins with a pixel set of 6 pixels and an observed set of 3 exposures by 2 segments
struct Installed {
  Heap<int64_t> seg{0, 2, 6};
  ProductState S;
  Installed() { S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.lo = 0; S.hi = 5000; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get(); }
};

static trx_exposures table(int32_t nexp, const double *scale, const double *smear) { trx_exposures E{}; E.nexp = nexp; E.pad = 77; E.scale = scale; E.smear = smear; return E; }

static void set_refusals()
{
  const Installed I;
  Heap<double> scale{1.0, 0.0, -0.25}, smear{0.0, 1e-5, TRX_SMEAR_MAX};
  trx_exposures E = table(3, scale.get(), smear.get());
  ACCEPTED(exposure_set_checks(I.S, &E, msg));
  { ProductState N = I.S; N.seg = nullptr; REFUSED(exposure_set_checks(N, &E, msg), TRX_E_ARG, "exposures: no observed set installed (trx_set_observed)"); }
  { ProductState N = I.S; N.npix = 0; REFUSED(exposure_set_checks(N, &E, msg), TRX_E_ARG, "exposures: no observed set installed (trx_set_observed)"); }
  E = table(-3, nullptr, nullptr);                                                                  // (before the arrays are looked at)
  REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, "exposures: nexp < 0");
  E = table(2, Heap<double>(2, 1.0).get(), nullptr);
  REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, "exposures: nexp 2 is not the observed set's nexp 3");
  E = table(4, nullptr, nullptr);
  REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, "exposures: nexp 4 is not the observed set's nexp 3");
  E = table(3, nullptr, nullptr);
  REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, "exposures: NULL scale and smear arrays");
  // one array alone is a table
  E = table(3, scale.get(), nullptr); ACCEPTED(exposure_set_checks(I.S, &E, msg));
  E = table(3, nullptr, smear.get()); ACCEPTED(exposure_set_checks(I.S, &E, msg));
  E = table(3, scale.get(), smear.get());
  for (double bad : {kNaN, kInf, -kInf}) {
    scale[2] = bad;
    REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, "exposures: exposure 2: scale must be finite");
  }
  scale[2] = -0.25;
  const std::string smear_text = "smear must be finite, >= 0 and at most TRX_SMEAR_MAX (" + std::to_string(TRX_SMEAR_MAX) + ")";
  for (double bad : {kNaN, kInf, -1e-300, -1.0, std::nextafter(TRX_SMEAR_MAX, 1.0), 1.0}) {
    smear[1] = bad;
    REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, ("exposures: exposure 1: " + smear_text).c_str());
  }
  // by exposure, then the scale before the smear
  scale[1] = kNaN; smear[0] = -1.0;
  REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, ("exposures: exposure 0: " + smear_text).c_str());
  smear[0] = 0.0;
  REFUSED(exposure_set_checks(I.S, &E, msg), TRX_E_ARG, "exposures: exposure 1: scale must be finite");
  scale[1] = 0.0; smear[1] = 0.0;
  ACCEPTED(exposure_set_checks(I.S, &E, msg));
  // a large set: every entry of both arrays is read, none past the end
  { Heap<int64_t> seg{0, 6}; ProductState B = I.S; B.nexp = 1000; B.nseg = 1; B.seg = seg.get();
    Heap<double> sc(1000, 2.0), sm(1000, 1e-6);
    trx_exposures T = table(1000, sc.get(), sm.get());
    ACCEPTED(exposure_set_checks(B, &T, msg));
    sm[999] = 0.011;
    REFUSED(exposure_set_checks(B, &T, msg), TRX_E_ARG, ("exposures: exposure 999: " + smear_text).c_str()); }
}

static void run_refusals()
{
  Installed I; I.S.exposures = true;
  const char *who = "trx_run_exposed";
  Heap<double> sh{1.0, 1.0001, 0.9999}, out(3 * 6 * 2);
  ACCEPTED(exposed_run_checks(I.S, who, 3, sh.get(), out.get(), msg));
  // (a shard of the grid is served: the pairs are linear in the bins)
  { ProductState W = I.S; W.windowed = true; W.lo = 10; ACCEPTED(exposed_run_checks(W, who, 3, sh.get(), out.get(), msg)); }
  { ProductState N = I.S; N.seg = nullptr; REFUSED(exposed_run_checks(N, who, 3, sh.get(), out.get(), msg), TRX_E_ARG, "trx_run_exposed: no observed set installed (trx_set_observed)"); }
  { ProductState N = I.S; N.exposures = false; REFUSED(exposed_run_checks(N, who, 2, nullptr, nullptr, msg), TRX_E_ARG, "trx_run_exposed: no exposure table installed (trx_set_exposures)"); }
  REFUSED(exposed_run_checks(I.S, who, 2, nullptr, nullptr, msg), TRX_E_ARG, "trx_run_exposed: nshift 2 is not the observed set's nexp 3");
  REFUSED(exposed_run_checks(I.S, who, 0, sh.get(), out.get(), msg), TRX_E_ARG, "trx_run_exposed: nshift 0 is not the observed set's nexp 3");
  REFUSED(exposed_run_checks(I.S, who, -3, sh.get(), out.get(), msg), TRX_E_ARG, "trx_run_exposed: nshift -3 is not the observed set's nexp 3");
  REFUSED(exposed_run_checks(I.S, who, 3, nullptr, nullptr, msg), TRX_E_ARG, "trx_run_exposed: shift is NULL");
  REFUSED(exposed_run_checks(I.S, who, 3, sh.get(), nullptr, msg), TRX_E_ARG, "trx_run_exposed: out is NULL");
  // the shifts themselves: the pixel runs' check under this call's name
  sh[2] = 0.0;
  REFUSED(pixel_run_checks(who, 3, 6, sh.get(), msg), TRX_E_ARG, "trx_run_exposed: shift 2 must be finite and > 0");
  // the moment runs stay refused on a shard, with or without a table
  { ProductState W = I.S; W.windowed = true; std::string msg; CHECK(observed_run_checks(W, "trx_run_moments", ObservedRun::Moments, 3, sh.get(), out.get(), "mom", msg) == TRX_E_UNSUPPORTED); }
}

static void extents()
{
  ExposureExtents X = exposure_extents(3);
  CHECK(X.scale_bytes == 24 && X.smear_bytes == 24);
  X = exposure_extents(0);
  CHECK(X.scale_bytes == 0 && X.smear_bytes == 0);
  X = exposure_extents(0x7fffffff);
  CHECK(X.scale_bytes == 8ull * 0x7fffffffull && X.smear_bytes == X.scale_bytes);
  // the table's arrays read over exactly that extent (what a run uploads)
  Heap<double> a(5, 1.0); double s = 0; for (size_t k = 0; k < exposure_extents(5).scale_bytes / sizeof(double); k++) s += a[k];
  CHECK(s == 5.0);
}

static void print_range(double wn_i, double wn_d, int64_t nwn, double cut, double c, double f, double sh, double eta)
{
  double centre, sigma, d; int64_t first, last;
  exposed_range(wn_i, wn_d, nwn, cut, kFwhmSigma, c, f, sh, eta, centre, sigma, d, first, last);
  std::printf("range %a %a %lld %a %a %a %a %a %a %a %a %lld %lld\n", wn_i, wn_d, (long long)nwn, cut, c, f, sh, eta, centre, sigma, d, (long long)first, (long long)last);
}

static void ranges()
{
  const double wn_i = 2000.0, wn_d = 0.1; const int64_t nwn = 5000;
  double centre, sigma, d; int64_t a, z;
  // eta == 0: the plain Gaussian's bins (gauss_band_range), d exactly 0
  for (double c : {2100.03, 2000.0, 2499.9, 1999.0, 2600.0, 1e300, -1e300})
    for (double f : {1.0, 0.05, 300.0}) {
      exposed_range(wn_i, wn_d, nwn, 4.0, kFwhmSigma, c, f, 1.0, 0.0, centre, sigma, d, a, z);
      int64_t ga, gz; gauss_band_range(wn_i, wn_d, nwn, c, f / kFwhmSigma, 4.0, ga, gz);
      CHECK(a == ga && z == gz && d == 0.0 && centre == c && sigma == f / kFwhmSigma);
      print_range(wn_i, wn_d, nwn, 4.0, c, f, 1.0, 0.0);
    }
  // eta > 0 widens by d = centre * eta either side: sigma 0.05 and cut 4 reach 0.2 = 2 bins; eta = 1e-3 adds 2.1 cm-1 = 21 bins
  exposed_range(wn_i, wn_d, nwn, 4.0, kFwhmSigma, 2100.03, 0.05 * kFwhmSigma, 1.0, 0.0, centre, sigma, d, a, z);
  CHECK(a == 999 && z == 1003);
  exposed_range(wn_i, wn_d, nwn, 4.0, kFwhmSigma, 2100.03, 0.05 * kFwhmSigma, 1.0, 1e-3, centre, sigma, d, a, z);
  CHECK(a == 978 && z == 1024 && d == 2100.03 * 1e-3);
  // clipped at 0 and at nwn, off either end, TRX_SMEAR_MAX, a shift that moves the window, NaN edges: no bin
  for (double eta : {1e-9, 1e-5, 1e-3, (double)TRX_SMEAR_MAX}) {
    for (double c : {2100.03, 2000.0, 2000.4, 2499.9, 2499.5, 1990.0, 2510.0, 1000.0, 5000.0, 1e300, -1e300})
      print_range(wn_i, wn_d, nwn, 4.0, c, 1.0, 1.0, eta);
    print_range(wn_i, wn_d, nwn, 4.0, 2100.03, 1.0, 1.0 - 150.0 / 299792.458, eta);
    print_range(wn_i, wn_d, nwn, 4.0, 2100.03, 1.0, 1e-306, eta);       // (the centre overflows: inf - inf)
    print_range(wn_i, wn_d, nwn, 4.0, 2100.03, 1.0, 1e300, eta);
  }
  exposed_range(wn_i, wn_d, nwn, 4.0, kFwhmSigma, 2100.03, 1.0, 1e-306, 1e-5, centre, sigma, d, a, z);
  CHECK(a == 0 && z == 0);
  exposed_range(wn_i, wn_d, nwn, 4.0, kFwhmSigma, 1e300, 1.0, 1.0, TRX_SMEAR_MAX, centre, sigma, d, a, z);
  CHECK(a == nwn && z == nwn);
  exposed_range(wn_i, wn_d, nwn, 4.0, kFwhmSigma, 2250.0, 1.0, 1.0, TRX_SMEAR_MAX, centre, sigma, d, a, z);
  CHECK(a > 2250 && z < 2750 + 30 && z - a > 440);                      // (d = 22.5 cm-1 = 225 bins either side)
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "range")) {
    std::FILE *f = std::fopen(argv[2], "r");
    if (!f) return 2;
    double wn_i, wn_d, cut, c, w, sh, eta; long long nwn;
    while (std::fscanf(f, "%la %la %lld %la %la %la %la %la", &wn_i, &wn_d, &nwn, &cut, &c, &w, &sh, &eta) == 8) print_range(wn_i, wn_d, nwn, cut, c, w, sh, eta);
    std::fclose(f);
    return 0;
  }
  set_refusals(); run_refusals(); extents(); ranges();
  if (g_bad) { std::printf("%d of %d checks FAILED\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
