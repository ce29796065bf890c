// transit_lib.cpp -- libtransit.so, the reference's library interface (include/transit_lib.h):
// transit_init() -> trh_load() [+ the opacity-grid build] + trx_create(), run_transit() ->
// trh_reload_atm() + trx_run() on the resident handle + the files of one do_transit()
// (transit.c:125-207), free_memory() -> trx_destroy() + trh_free().  The module-global state
// of the reference (transit.c:7-12) is the one `g` below; it is not exported.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "transit_lib.h"
#pragma GCC visibility pop

#include "transit_hip.h"
#include "transit_host.h"
#include "transit_outputs.h"

namespace {

const char *const kProg = "transit";

struct State {
  trh_problem *P = nullptr;
  trx_handle *h = nullptr;
  bool opabreak = false;             // --justOpacity: initialised, but runs compute nothing (transit.c:133-136)
  int verblevel = 2;
};

State g;
int g_status = TRX_OK;
std::string g_error;

void ok() { g_status = TRX_OK; g_error.clear(); }

// record a failure; loud = also one line on stderr
void fail(int rc, const std::string &msg, bool loud = true)
{
  g_status = rc == TRX_OK ? TRX_E_ARG : rc;
  g_error = msg;
  if (loud) std::fprintf(stderr, "%s: %s (%s)\n", kProg, msg.c_str(), trx_strerror(g_status));
}

void release()
{
  if (g.h) trx_destroy(g.h);
  if (g.P) trh_free(g.P);
  g = State();
}

void fill_nan(double *out, int n)
{
  for (int i = 0; out && i < n; i++) out[i] = std::numeric_limits<double>::quiet_NaN();
}

}  // namespace

extern "C" {

void transit_init(int argc, char **argv)
{
  release();
  ok();
  char err[512] = {0};
  trh_problem *P = nullptr;
  int rc = trh_load(argc, argv, &P, err, sizeof(err));
  if (rc == 1) return;                                     // --help / --version: printed, nothing to run
  if (rc != TRX_OK) { fail(rc, err); return; }
  const int verblevel = trr::verb_level(P);
  trr::print_messages(P, verblevel, kProg);
  std::string oerr;
  if ((rc = trr::build_opacity_grid(P, verblevel, oerr)) != TRX_OK) { trh_free(P); fail(rc, oerr); return; }
  trx_handle *h = nullptr;
  const bool opabreak = trh_option(P, "justOpacity") != nullptr;
  if (!opabreak && (rc = trx_create(trh_static(P), &h)) != TRX_OK) {
    const char *detail = trx_last_error(nullptr);
    const std::string msg = std::string("trx_create failed") + (detail && *detail ? std::string(": ") + detail : "");
    trh_free(P); fail(rc, msg); return;
  }
  g.P = P; g.h = h; g.opabreak = opabreak; g.verblevel = verblevel;
}

int get_no_samples(void)
{
  if (!g.P) { fail(TRX_E_ARG, "transit_init has not been called", false); return 0; }
  ok();
  return (int)trh_nwn(g.P);
}

void get_waveno_arr(double *waveno_arr, int waveno)
{
  if (!g.P) {
    std::printf("Transit not initialized, please run init. Values set -1\n");      // transit.c:90
    for (int i = 0; waveno_arr && i < waveno; i++) waveno_arr[i] = -1;
    fail(TRX_E_ARG, "transit_init has not been called", false);
    return;
  }
  ok();
  if (!waveno_arr || waveno <= 0) return;
  std::vector<double> wn((size_t)trh_nwn(g.P));
  trh_wavenumbers(g.P, wn.data());
  for (int i = 0; i < waveno; i++) waveno_arr[i] = (size_t)i < wn.size() ? wn[(size_t)i] : 0.0;
}

void set_radius(double refradius)
{
  if (!g.P) { fail(TRX_E_ARG, "set_radius: transit_init has not been called", false); return; }
  ok(); trh_set_radius(g.P, refradius);
}

void set_cloudtop(double cloudtop)
{
  if (!g.P) { fail(TRX_E_ARG, "set_cloudtop: transit_init has not been called", false); return; }
  ok(); trh_set_cloudtop(g.P, cloudtop);
}

void set_scattering(int flag, double scattering)
{
  if (!g.P) { fail(TRX_E_ARG, "set_scattering: transit_init has not been called", false); return; }
  ok(); trh_set_scattering(g.P, flag, scattering);
}

void run_transit(double *re_input, int transint, double *transit_out, int transit_out_size)
{
  if (!g.P) {
    std::printf("Transit init not run, please initialize transit.\n");             // transit.c:130
    fill_nan(transit_out, transit_out_size);
    fail(TRX_E_ARG, "run_transit: transit_init has not been called", false);
    return;
  }
  ok();
  int rc = trh_reload_atm(g.P, re_input, transint);
  if (rc != TRX_OK) {
    fill_nan(transit_out, transit_out_size);
    fail(rc, "run_transit: the atmosphere (" + std::to_string(transint) + " values) cannot be reloaded");
    return;
  }
  if (g.opabreak) return;
  const trr::Plan plan = trr::plan_outputs(g.P);
  trr::Saved saved;
  trr::before_spectrum(g.P, plan, g.verblevel, kProg, saved);
  if (plan.saveext &&                                      // this call's file, or forget the previous call's rows
      (rc = trx_restore_extinction(g.h, saved.restored ? plan.nr : 0, saved.e.data(), saved.flags.data())) != TRX_OK) {
    fill_nan(transit_out, transit_out_size);
    fail(rc, std::string("trx_restore_extinction: ") + trx_last_error(g.h));
    return;
  }
  std::vector<double> spectrum((size_t)plan.nwn);
  trr::Buffers buf;
  trx_debug dbg{};
  trx_opts opts = *trh_opts(g.P);
  const bool any = buf.attach(plan, plan.nwn, dbg, opts);
  if ((rc = trx_run(g.h, trh_atm(g.P), &opts, spectrum.data(), any ? &dbg : nullptr)) != TRX_OK) {
    fill_nan(transit_out, transit_out_size);
    fail(rc, std::string("trx_run: ") + trx_last_error(g.h));
    return;
  }
  if ((rc = trr::write_outputs(g.P, plan, saved, spectrum.data(), buf, kProg)) != TRX_OK)
    fail(rc, "run_transit: cannot write the spectrum file", false);         // (reported on stderr already)
  for (int i = 0; transit_out && i < transit_out_size; i++)
    transit_out[i] = (size_t)i < spectrum.size() ? spectrum[(size_t)i] : 0.0;
}

void free_memory(void)
{
  release();
  ok();
}

int transit_status(void) { return g_status; }
const char *transit_error(void) { return g_error.c_str(); }

}  // extern "C"
