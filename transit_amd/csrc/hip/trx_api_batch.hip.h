// trx_api_batch.hip.h -- several atmospheres per call: trx_batch, its workers, the installers and the trx_run_batch_* calls
// with their one preflight.  Part of the one translation unit trx_api.hip, which includes it inside its extern "C" block
// behind the product calls it deals out (trx_api_products.hip.h).
#pragma once

// ---- several atmospheres per call -----------------------------------------------------------------
// A retrieval driver runs many chains over one line list (the reference: one run_transit per atmosphere,
// transit.c:118-122, one process each).  One spectrum leaves the device idle between its kernels and while
// the host prepares and queues (about a fifth of a CH4-demo spectrum), and another
// spectrum's kernels fit there: a batch keeps `ways` handles made from ONE description, each with a host
// thread of its own, and deals the K atmospheres of a call to them.  Every spectrum is what trx_run gives
// for its atmosphere, bit for bit -- it IS a trx_run, on whichever handle was free (a run's sums do not
// depend on the handle's history: the depth hint only changes the step plan).
extern "C++" {      // (BatchJob's constructor and batch_install are templates: they cannot have C linkage)
// one call's job, "run atmosphere j on handle h": a callable of its trx_run_batch_* function, held by address -- it lives on
// the stack of that function, which waits inside batch_call until every worker is done with it.  Nothing is allocated,
// nothing can throw.
struct BatchJob {
  const void *call = nullptr; int (*run)(const void *call, trx_handle *h, int32_t j) = nullptr;
  BatchJob() = default;
  template <class F>
  BatchJob(const F &f) : call(&f), run([](const void *c, trx_handle *h, int32_t j) { return (*static_cast<const F *>(c))(h, j); }) {}
  int operator()(trx_handle *h, int32_t j) const { return run(call, h, j); }
};

struct trx_batch {
  std::vector<trx_handle *> hs;
  std::vector<std::thread> workers;
  std::mutex mu; std::condition_variable cv_work, cv_done;
  // the call being served (under mu): k atmospheres, the job that runs one of them, and whether a worker installs the
  // atmosphere's broadening on its handle first (a pixel, moment, filtered-moment, trail, map or broadened run)
  uint64_t epoch = 0; bool quit = false;
  int32_t k = 0; BatchJob job; bool wants_broadening = false;
  // trx_batch_set_broadening: one entry for all atmospheres or one per atmosphere (empty: none)
  std::vector<trx_broadening> broad;
  // trx_batch_set_exposures: one table for all atmospheres or one per atmosphere (empty: none), the arrays copied; a worker
  // installs the atmosphere's on its handle first where the call's rows are exposures (wants_exposures: an exposed, moment,
  // filtered-moment or exposed-map run)
  std::vector<ExposureSet> expo; bool wants_exposures = false;
  std::atomic<int32_t> next{0};
  int32_t busy = 0; int rc = TRX_OK; std::string err;
};

// every handle of the batch gets the same set, or none does: all sets are built (make) before any is installed (install);
// the failing handle's text goes to trx_last_error(NULL)
template <class Set, class Make>
static int batch_install(trx_batch *b, Make make, void (*install)(trx_handle *, std::unique_ptr<Set> &))
{
  g_comm_err.clear();
  if (!b) return TRX_E_ARG;
  std::vector<std::unique_ptr<Set>> sets(b->hs.size());
  for (size_t i = 0; i < b->hs.size(); i++) {
    const int rc = make(b->hs[i], sets[i]);
    if (rc) { g_comm_err = b->hs[i]->err; return rc; }
  }
  for (size_t i = 0; i < b->hs.size(); i++) install(b->hs[i], sets[i]);
  return TRX_OK;
}
}  // extern "C++"

int trx_batch_create(const trx_static *st, int32_t ways, trx_batch **out)
{
  g_comm_err.clear();
  if (!st || !out || ways < 1 || ways > TRX_BATCH_MAX_WAYS) { g_comm_err = "batch: bad argument (ways 1.." + std::to_string(TRX_BATCH_MAX_WAYS) + ")"; return TRX_E_ARG; }
  *out = nullptr;
  std::unique_ptr<trx_batch> B(new (std::nothrow) trx_batch);
  if (!B) { g_comm_err = "batch: out of host memory"; return TRX_E_NOMEM; }
  // (no C++ exception crosses the C boundary: a failed handle, allocation or thread start gives the handles back,
  // joins the workers that did start and returns a code, its text through trx_last_error(NULL))
  auto give_up = [&](int rc, const std::string &why) {
    { std::lock_guard<std::mutex> lk(B->mu); B->quit = true; }
    B->cv_work.notify_all();
    for (std::thread &t : B->workers) if (t.joinable()) t.join();
    for (trx_handle *x : B->hs) trx_destroy(x);
    B->hs.clear(); B->workers.clear();
    g_comm_err = why;
    return rc;
  };
  for (int i = 0; i < ways; i++) {
    trx_handle *h = nullptr;
    const int rc = trx_create(st, &h);
    if (rc != TRX_OK) return give_up(rc, "batch: handle " + std::to_string(i) + ": " + trx_strerror(rc));
    try { B->hs.push_back(h); } catch (...) { trx_destroy(h); return give_up(TRX_E_NOMEM, "batch: out of host memory"); }
  }
  trx_batch *b = B.get();
  try {
  for (int i = 0; i < ways; i++)
    b->workers.emplace_back([b, i]() {
      uint64_t seen = 0;
      for (;;) {
        {
          std::unique_lock<std::mutex> lk(b->mu);
          b->cv_work.wait(lk, [&] { return b->quit || b->epoch != seen; });
          if (b->quit) return;
          seen = b->epoch;
        }
        for (;;) {
          const int32_t j = b->next.fetch_add(1);
          if (j >= b->k) break;
          trx_handle *const hj = b->hs[(size_t)i];
          int rc = TRX_OK;
          // (this atmosphere's broadening first -- checked whole by trx_batch_set_broadening; none: cleared)
          if (b->wants_broadening)
            rc = trx_set_broadening(hj, b->broad.empty() ? nullptr : &b->broad[b->broad.size() == 1 ? 0 : (size_t)j]);
          // (and its exposure table -- checked whole by trx_batch_set_exposures; none: cleared)
          if (rc == TRX_OK && b->wants_exposures) {
            if (b->expo.empty()) rc = trx_set_exposures(hj, nullptr);
            else {
              const ExposureSet &E = b->expo[b->expo.size() == 1 ? 0 : (size_t)j];
              const trx_exposures ex{E.nexp, 0, E.scale.empty() ? nullptr : E.scale.data(), E.smear.empty() ? nullptr : E.smear.data()};
              rc = trx_set_exposures(hj, &ex);
            }
          }
          if (rc == TRX_OK) rc = b->job(hj, j);
          if (rc != TRX_OK) {
            std::lock_guard<std::mutex> lk(b->mu);
            if (b->rc == TRX_OK) { b->rc = rc; b->err = "atmosphere " + std::to_string(j) + ": " + hj->err; }
            b->next.store(b->k);                           // (the others finish the spectrum they are on and stop)
          }
        }
        std::lock_guard<std::mutex> lk(b->mu);
        if (--b->busy == 0) b->cv_done.notify_all();
      }
    });
  } catch (const std::bad_alloc &) { return give_up(TRX_E_NOMEM, "batch: out of host memory");
  } catch (const std::exception &e) { return give_up(TRX_E_HIP, std::string("batch: worker thread: ") + e.what()); }
  *out = B.release();
  return TRX_OK;
}

// one call of the batch: `job` for each of k atmospheres on whichever handle is free; returns when every worker is done
static int batch_call(trx_batch *b, int32_t k, bool wants_broadening, const BatchJob &job, bool wants_exposures = false)
{
  if (k == 0) return TRX_OK;
  std::unique_lock<std::mutex> lk(b->mu);
  b->k = k; b->job = job; b->wants_broadening = wants_broadening; b->wants_exposures = wants_exposures;
  b->next.store(0); b->rc = TRX_OK; b->err.clear();
  b->busy = (int32_t)b->workers.size();
  b->epoch++;
  b->cv_work.notify_all();
  b->cv_done.wait(lk, [&] { return b->busy == 0; });
  b->job = BatchJob{};                                     // (the caller's callable goes when this returns)
  if (b->rc != TRX_OK) g_comm_err = b->err;                // trx_last_error(NULL)
  return b->rc;
}

// ---- the preflight of a batch call, in the order every call has checked it: the arguments (args: atm, opts and the
// call's required arrays are there), what the call needs installed (the handles are made from one description: the first
// speaks for all), its count where it has one (named count_name), a NULL row among its arrays.  The text goes to
// trx_last_error(NULL) as "<who>: ..." -- who null: trx_run_batch, which refuses with the bare code.
enum : unsigned { kNeedBands = 1, kNeedPixels = 2, kNeedObserved = 4, kNeedFilter = 8, kNeedBroadening = 16, kNeedExposures = 32 };
static int batch_preflight(trx_batch *b, const char *who, int32_t k, bool args, unsigned needs, const char *count_name, int32_t count,
                           std::initializer_list<BatchRows> rows)
{
  g_comm_err.clear();
  auto no = [&](const std::string &what) { if (who) g_comm_err = std::string(who) + ": " + what; return TRX_E_ARG; };
  if (!b || k < 0 || (k > 0 && !args)) return no("bad argument");
  const trx_handle *const h0 = b->hs.empty() ? nullptr : b->hs[0];
  if ((needs & kNeedBands) && !(h0 && h0->bands)) return no("no band set installed (trx_batch_set_bands)");
  if ((needs & kNeedPixels) && !(h0 && h0->pixels)) return no("no pixel set installed (trx_batch_set_pixels)");
  if ((needs & kNeedObserved) && !(h0 && h0->observed)) return no("no observed set installed (trx_batch_set_observed)");
  if ((needs & kNeedFilter) && !(h0 && h0->filter)) return no("no filter installed (trx_batch_set_filter)");
  if ((needs & kNeedBroadening) && b->broad.empty()) return no("no broadening installed (trx_batch_set_broadening)");
  if ((needs & kNeedExposures) && b->expo.empty()) return no("no exposure table installed (trx_batch_set_exposures)");
  if (count_name && count < 1) return no(std::string(count_name) + " < 1");
  const int rc = batch_rows_check(who ? who : "", k, rows, g_comm_err);
  if (rc && !who) g_comm_err.clear();
  return rc;
}

// ... and behind it (and a map call's own checks): a run of k atmospheres takes one broadening for all, one each, or none,
// and (exposures: its rows are exposures) one exposure table for all, one each, or none
static int batch_fits(trx_batch *b, int32_t k, const char *who, bool exposures)
{
  auto fits = [&](size_t n, const char *what) {
    if (n <= 1 || n == (size_t)k || k == 0) return TRX_OK;
    g_comm_err = std::string(who) + ": " + std::to_string(n) + what + std::to_string(k) + " atmospheres";
    return TRX_E_ARG;
  };
  if (const int rc = fits(b->broad.size(), " broadenings installed (trx_batch_set_broadening) for ")) return rc;
  return exposures ? fits(b->expo.size(), " exposure tables installed (trx_batch_set_exposures) for ") : TRX_OK;
}

int trx_run_batch(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, double *const *spectra)
{
  if (const int rc = batch_preflight(b, nullptr, k, atm && opts && spectra, 0, nullptr, 0, {{"spectra", spectra}})) return rc;
  return batch_call(b, k, false, [=](trx_handle *h, int32_t j) { return trx_run(h, atm + j, opts, spectra[j], nullptr); });
}

int trx_batch_set_bands(trx_batch *b, int32_t nbands, const trx_band *bands)
{
  return batch_install<BandSet>(b, [=](trx_handle *h, std::unique_ptr<BandSet> &S) { return make_band_set(h, nbands, bands, S); }, install_band_set);
}

int trx_run_batch_bands(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, double *const *sums)
{
  if (const int rc = batch_preflight(b, "trx_run_batch_bands", k, atm && opts && sums, kNeedBands, nullptr, 0, {{"sums", sums}})) return rc;
  return batch_call(b, k, false, [=](trx_handle *h, int32_t j) { return trx_run_bands(h, atm + j, opts, nullptr, sums[j], nullptr); });
}

int trx_run_batch_contrib(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, double *const *sums, double *const *contrib)
{
  if (const int rc = batch_preflight(b, "trx_run_batch_contrib", k, atm && opts && sums && contrib, kNeedBands, nullptr, 0, {{"sums", sums}, {"contrib", contrib}})) return rc;
  return batch_call(b, k, false, [=](trx_handle *h, int32_t j) { return trx_run_contrib(h, atm + j, opts, nullptr, sums[j], contrib[j], nullptr); });
}

// the batch's broadenings, one for all atmospheres or one each: all entries are checked before any is kept, or none is
int trx_batch_set_broadening(trx_batch *b, int32_t n, const trx_broadening *br)
{
  g_comm_err.clear();
  if (!b || b->hs.empty()) return TRX_E_ARG;
  if (n < 0 || (n > 0 && !br)) { g_comm_err = "trx_batch_set_broadening: n < 0 or a NULL array"; return TRX_E_ARG; }
  std::vector<trx_broadening> keep;
  try { keep.assign(br, br + n); } catch (...) { g_comm_err = "trx_batch_set_broadening: out of host memory"; return TRX_E_NOMEM; }
  // (the handles are made from one description: what the first accepts, all accept)
  for (int32_t j = 0; j < n; j++) {
    bool on; Broadening B;
    const int rc = make_broadening(b->hs[0], &keep[(size_t)j], on, B);
    if (rc) { g_comm_err = "entry " + std::to_string(j) + ": " + b->hs[0]->err; return rc; }
    if (!on) { g_comm_err = "trx_batch_set_broadening: entry " + std::to_string(j) + " is of kind TRX_BROADEN_NONE (n = 0 clears)"; return TRX_E_ARG; }
  }
  b->broad = std::move(keep);
  if (n == 0) for (trx_handle *h : b->hs) { h->broad_on = false; h->broad = Broadening{}; }
  return TRX_OK;
}

int trx_run_batch_broadened(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, double *const *broadened)
{
  const char *const who = "trx_run_batch_broadened";
  int rc;
  if ((rc = batch_preflight(b, who, k, atm && opts && broadened, kNeedBroadening, nullptr, 0, {{"broadened", broadened}})) || (rc = batch_fits(b, k, who, false))) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_broadened(h, atm + j, opts, nullptr, broadened[j], nullptr); });
}

int trx_batch_set_pixels(trx_batch *b, const trx_pixels *px)
{
  const int rc = batch_install<PixelSet>(b, [=](trx_handle *h, std::unique_ptr<PixelSet> &S) { return make_pixel_set(h, px, S); }, install_pixel_set);
  if (rc == TRX_OK) b->expo.clear();                      // (the exposure tables go with the observed set)
  return rc;
}

int trx_run_batch_pixels(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, int32_t nshift, const double *const *shift,
                         double *const *out)
{
  const char *const who = "trx_run_batch_pixels";
  int rc;
  if ((rc = batch_preflight(b, who, k, atm && opts && shift && out, kNeedPixels, "nshift", nshift, {{"shift", shift}, {"out", out}})) || (rc = batch_fits(b, k, who, false))) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_pixels(h, atm + j, opts, nullptr, nshift, shift[j], out[j], nullptr); });
}

int trx_batch_set_observed(trx_batch *b, const trx_observed *ob)
{
  const int rc = batch_install<ObservedSet>(b, [=](trx_handle *h, std::unique_ptr<ObservedSet> &S) { return make_observed_set(h, ob, S); }, install_observed_set);
  if (rc == TRX_OK) b->expo.clear();                      // (the exposure tables go with the observed set)
  return rc;
}

// the batch's exposure tables, one for all atmospheres or one each: all entries are checked before any is kept, or none is
int trx_batch_set_exposures(trx_batch *b, int32_t n, const trx_exposures *ex)
{
  g_comm_err.clear();
  if (!b || b->hs.empty()) return TRX_E_ARG;
  if (n < 0 || (n > 0 && !ex)) { g_comm_err = "trx_batch_set_exposures: n < 0 or a NULL array"; return TRX_E_ARG; }
  std::vector<ExposureSet> keep;
  // (the handles are made from one description and carry one observed set: what the first accepts, all accept)
  for (int32_t j = 0; j < n; j++) {
    std::unique_ptr<ExposureSet> S;
    const int rc = make_exposure_set(b->hs[0], ex + j, S);
    if (rc) { g_comm_err = "entry " + std::to_string(j) + ": " + b->hs[0]->err; return rc; }
    if (!S) { g_comm_err = "trx_batch_set_exposures: entry " + std::to_string(j) + " has nexp 0 (n = 0 clears)"; return TRX_E_ARG; }
    try { keep.push_back(std::move(*S)); } catch (...) { g_comm_err = "trx_batch_set_exposures: out of host memory"; return TRX_E_NOMEM; }
  }
  b->expo = std::move(keep);
  if (n == 0) for (trx_handle *h : b->hs) h->exposures.reset();
  return TRX_OK;
}

int trx_run_batch_exposed(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, int32_t nshift, const double *const *shift,
                          double *const *out)
{
  const char *const who = "trx_run_batch_exposed";
  int rc;
  if ((rc = batch_preflight(b, who, k, atm && opts && shift && out, kNeedObserved | kNeedExposures, nullptr, 0, {{"shift", shift}, {"out", out}})) || (rc = batch_fits(b, k, who, true))) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_exposed(h, atm + j, opts, nullptr, nshift, shift[j], out[j], nullptr); }, true);
}

int trx_run_batch_moments(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, int32_t nshift, const double *const *shift,
                          double *const *mom)
{
  const char *const who = "trx_run_batch_moments";
  int rc;
  if ((rc = batch_preflight(b, who, k, atm && opts && shift && mom, kNeedObserved, nullptr, 0, {{"shift", shift}, {"mom", mom}})) || (rc = batch_fits(b, k, who, true))) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_moments(h, atm + j, opts, nullptr, nshift, shift[j], mom[j], nullptr); }, true);
}

int trx_run_batch_trail(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, int32_t nlag, const double *const *lag,
                        double *const *trail)
{
  const char *const who = "trx_run_batch_trail";
  int rc;
  if ((rc = batch_preflight(b, who, k, atm && opts && lag && trail, kNeedObserved, "nlag", nlag, {{"lag", lag}, {"trail", trail}})) || (rc = batch_fits(b, k, who, false))) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_trail(h, atm + j, opts, nullptr, nlag, lag[j], trail[j], nullptr); });
}

int trx_run_batch_velocity_map(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, const trx_vmap *vm, double *const *map,
                               double *const *per)
{
  const char *const who = "trx_run_batch_velocity_map";
  if (const int rc = batch_preflight(b, who, k, atm && opts && map, kNeedObserved, nullptr, 0, {{"map", map}, {"per", per}})) return rc;
  // (the handles are made from one description and carry one observed set: what the first refuses, all refuse)
  if (k > 0)
    if (const int rc = velocity_map_checks(product_state(b->hs[0]), who, vm, map[0], g_comm_err)) return fail(b->hs[0], rc, g_comm_err);
  if (const int rc = batch_fits(b, k, who, false)) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_velocity_map(h, atm + j, opts, nullptr, vm, map[j], per ? per[j] : nullptr, nullptr); });
}

int trx_batch_set_highpass(trx_batch *b, const trx_highpass *hp)
{
  return batch_install<HighPassSet>(b, [=](trx_handle *h, std::unique_ptr<HighPassSet> &S) { return make_highpass_set(h, hp, S); }, install_highpass_set);
}

int trx_batch_set_filter(trx_batch *b, const trx_filter *f)
{
  return batch_install<FilterSet>(b, [=](trx_handle *h, std::unique_ptr<FilterSet> &S) { return make_filter_set(h, f, S); }, install_filter_set);
}

int trx_batch_set_weighted_filter(trx_batch *b, const trx_wfilter *f)
{
  return batch_install<FilterSet>(b, [=](trx_handle *h, std::unique_ptr<FilterSet> &S) { return make_wfilter_set(h, f, S, nullptr); }, install_filter_set);
}

int trx_run_batch_filtered_moments(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, int32_t nshift, const double *const *shift,
                                   double *const *mom)
{
  const char *const who = "trx_run_batch_filtered_moments";
  int rc;
  if ((rc = batch_preflight(b, who, k, atm && opts && shift && mom, kNeedObserved | kNeedFilter, nullptr, 0, {{"shift", shift}, {"mom", mom}})) || (rc = batch_fits(b, k, who, true))) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_filtered_moments(h, atm + j, opts, nullptr, nshift, shift[j], nullptr, mom[j], nullptr); }, true);
}

// a filtered or exposed map of k atmospheres (needs: what it needs installed): the preflight, the map's own checks on the
// first handle -- the handles are made from one description and carry one observed set and one filter: what the first
// refuses, all refuse; the tables of an exposed map are the batch's, installed per atmosphere by the workers --, the fits
static int batch_map_preflight(trx_batch *b, const char *who, int32_t k, const trx_atm *atm, const trx_opts *opts, const trx_vmap *vm, double *const *map, unsigned needs)
{
  if (const int rc = batch_preflight(b, who, k, atm && opts && map, needs, nullptr, 0, {{"map", map}})) return rc;
  if (k > 0)
    if (const int rc = filtered_map_checks(product_state(b->hs[0]), who, vm, map[0], g_comm_err)) return fail(b->hs[0], rc, g_comm_err);
  return batch_fits(b, k, who, (needs & kNeedExposures) != 0);
}

int trx_run_batch_filtered_map(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, const trx_vmap *vm, double *const *map)
{
  if (const int rc = batch_map_preflight(b, "trx_run_batch_filtered_map", k, atm, opts, vm, map, kNeedObserved | kNeedFilter)) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_filtered_map(h, atm + j, opts, nullptr, vm, map[j], nullptr, nullptr); });
}

int trx_run_batch_exposed_map(trx_batch *b, int32_t k, const trx_atm *atm, const trx_opts *opts, const trx_vmap *vm, double *const *map)
{
  if (const int rc = batch_map_preflight(b, "trx_run_batch_exposed_map", k, atm, opts, vm, map, kNeedObserved | kNeedFilter | kNeedExposures)) return rc;
  return batch_call(b, k, true, [=](trx_handle *h, int32_t j) { return trx_run_exposed_map(h, atm + j, opts, nullptr, vm, map[j], nullptr, nullptr, nullptr); }, true);
}

int trx_batch_ways(const trx_batch *b) { return b ? (int)b->hs.size() : 0; }

void trx_batch_destroy(trx_batch *b)
{
  if (!b) return;
  { std::lock_guard<std::mutex> lk(b->mu); b->quit = true; }
  b->cv_work.notify_all();
  for (std::thread &t : b->workers) t.join();
  for (trx_handle *h : b->hs) trx_destroy(h);
  delete b;
}
