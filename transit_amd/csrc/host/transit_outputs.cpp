// transit_outputs.cpp -- see transit_outputs.h.
#include "transit_outputs.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace trr {

static double now_s()
{ return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int verb_level(const trh_problem *P)
{
  const char *verb = trh_option(P, "verb");
  return verb ? std::atoi(verb) : 2;
}

void print_messages(const trh_problem *P, int verblevel, const char *prog)
{
  if (verblevel < 2) return;
  for (const char *m = trh_messages(P); m && *m; ) {
    const char *e = std::strchr(m, '\n'); const size_t n = e ? (size_t)(e - m) : std::strlen(m);
    if (m[0] == 'W' || verblevel >= 3) std::fprintf(stderr, "%s: %s: %.*s\n", prog, m[0] == 'W' ? "warning" : "note", (int)(n > 3 ? n - 3 : 0), m + 3);
    m = e ? e + 1 : m + n;
  }
}

int build_opacity_grid(trh_problem *P, int verblevel, std::string &err)
{
  if (!trh_needs_opacity_build(P)) return TRX_OK;
  const double t0 = now_s();
  trx_handle *h = nullptr;
  int rc = trx_create(trh_static(P), &h);
  if (rc != TRX_OK) { err = std::string("trx_create failed: ") + trx_strerror(rc); return rc; }
  int32_t nv = 0, nslot = 0; const double *gt, *gd, *gz; const int32_t *gs;
  trh_grid_request(P, &nv, &gt, &gd, &gz, &nslot, &gs);
  std::vector<double> grid((size_t)nv * nslot * trh_nwn(P));
  rc = trx_sweep_permol(h, nv, gt, gd, gz, trh_opts(P)->ethresh, nslot, gs, grid.data());
  if (rc == TRX_OK) rc = trh_install_opacity(P, grid.data());
  if (rc != TRX_OK) {
    err = std::string("opacity-grid build failed: ") + trx_strerror(rc) + " (" + trx_last_error(h) + ")";
    trx_destroy(h);
    return rc;
  }
  if (verblevel > 3) std::printf("Check point: 00 - 05 opacity grid (%d states x %d molecules):  dt = %.4f sec.\n\n", nv, nslot, now_s() - t0);
  trx_destroy(h);
  return TRX_OK;
}

Plan plan_outputs(const trh_problem *P)
{
  Plan p;
  p.nwn = trh_nwn(P);
  p.nr = trh_atm(P)->nlayer;
  p.nang = trh_opts(P)->nangles;
  p.toomuch = trh_option(P, "outtoomuch") != nullptr;
  const char *sf = trh_option(P, "savefiles");
  p.dumps = sf && std::strncmp(sf, "yes", 3) == 0;                              // argum.c:461-470
  p.det_tau = trh_wants_detail(P, 0); p.det_ext = trh_wants_detail(P, 1); p.det_cia = trh_wants_detail(P, 2);
  p.intens = trh_option(P, "outintens") != nullptr && trh_opts(P)->solution == TRX_SOL_ECLIPSE;
  // --saveext: the extinction of an earlier run back in (restfile_extinct, tau.c:155-156), this run's out (tau.c:340-341)
  p.saveext = trh_option(P, "saveext") != nullptr;
  p.need_tau = p.toomuch || p.dumps || p.det_tau || p.det_ext;
  p.need_e = p.dumps || p.det_ext || p.saveext;
  p.need_ecs = p.dumps || p.det_cia;
  return p;
}

void before_spectrum(trh_problem *P, const Plan &plan, int verblevel, const char *prog, Saved &saved)
{
  saved.restored = false;
  if (plan.saveext) {
    saved.e.resize((size_t)plan.nwn * plan.nr); saved.flags.assign((size_t)plan.nr, 0);
    saved.restored = trh_saveext_read(P, saved.e.data(), saved.flags.data()) == TRX_OK;
    if (!saved.restored && verblevel >= 2) std::fprintf(stderr, "%s: note: no extinction restored from '%s'\n", prog, trh_option(P, "saveext"));
  }
  if (plan.dumps && trh_write_sample(P, nullptr) != TRX_OK)                     // makesample.c:598-599
    std::fprintf(stderr, "%s: cannot write the sampling file\n", prog);
}

bool Buffers::attach(const Plan &plan, int64_t n, trx_debug &dbg, trx_opts &opts)
{
  const size_t nr = (size_t)plan.nr;
  if (plan.need_tau) { tau.resize((size_t)n * nr); last.resize((size_t)n); dbg.tau = tau.data(); dbg.last = last.data(); }
  if (plan.need_e) { e.resize((size_t)n * nr); dbg.e = e.data(); }
  if (plan.saveext) { comp.assign(nr, 0); dbg.computed = comp.data(); }
  if (plan.need_ecs) { ecs.resize((size_t)n * nr); dbg.e_cs = ecs.data(); }
  if (plan.intens) { intens.resize((size_t)n * plan.nang); dbg.intens = intens.data(); }
  if (plan.dumps) {                                        // the dump writers redo the reference's laziness from `last`
    opts.eager = 1;
    er.resize((size_t)n * nr); es.resize((size_t)n * nr); ec.resize((size_t)n * nr);
    dbg.er = er.data(); dbg.e_scat = es.data(); dbg.e_cloud = ec.data();
  }
  return dbg.tau || dbg.e || dbg.e_cs || dbg.intens;
}

int write_outputs(trh_problem *P, const Plan &plan, const Saved &saved, const double *spectrum, Buffers &full,
                  const char *prog)
{
  const int64_t nwn = plan.nwn;
  const int nr = plan.nr;
  std::vector<double> &e = full.e;
  if (plan.saveext) {
    // a layer is in the file when every part of the run swept it or it came out of the file already (whose row it keeps)
    std::vector<uint8_t> flags(full.comp);
    for (int l = 0; l < nr; l++) {
      if (saved.restored && saved.flags[(size_t)l]) { flags[(size_t)l] = 1; std::memcpy(&e[(size_t)l * nwn], &saved.e[(size_t)l * nwn], sizeof(double) * (size_t)nwn); }
      if (!flags[(size_t)l]) std::fill(e.begin() + (size_t)l * nwn, e.begin() + (size_t)(l + 1) * nwn, 0.0);
    }
    if (trh_saveext_write(P, e.data(), flags.data()) != TRX_OK) std::fprintf(stderr, "%s: cannot write the extinction savefile\n", prog);
  }
  if (plan.need_e && plan.need_tau) {                      // the run may have swept deeper than the deepest ray: give the rows
    int64_t deep = 0;                                      // below it back the zeros the reference's lazy sweep leaves there
    for (int64_t w = 0; w < nwn; w++) deep = std::max(deep, full.last[(size_t)w]);
    std::fill(e.begin(), e.begin() + (size_t)(nr - 1 - deep) * nwn, 0.0);
  }
  if (plan.toomuch) trh_write_toomuch(P, full.tau.data(), full.last.data(), nullptr);
  if (plan.intens) trh_write_intens(P, full.intens.data(), nullptr);
  if (plan.dumps && (trh_write_dumps_masked(P, e.data(), full.ecs.data(), full.tau.data(), full.last.data(), nullptr) != TRX_OK ||
                     trh_write_ext_dumps(P, e.data(), full.ecs.data(), full.last.data(), full.er.data(), full.es.data(), full.ec.data(), nullptr) != TRX_OK))
    std::fprintf(stderr, "%s: cannot write the savefiles dumps\n", prog);
  if ((plan.det_tau && trh_write_detail(P, 0, full.tau.data()) != TRX_OK) || (plan.det_ext && trh_write_detail(P, 1, e.data()) != TRX_OK) ||
      (plan.det_cia && trh_write_detail(P, 2, full.ecs.data()) != TRX_OK))
    std::fprintf(stderr, "%s: cannot write a detail file\n", prog);
  const int rc = trh_write_spectrum(P, spectrum, nullptr);
  if (rc != TRX_OK) std::fprintf(stderr, "%s: cannot write the spectrum file\n", prog);
  return rc;
}

}  // namespace trr
