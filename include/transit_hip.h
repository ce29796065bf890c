/* transit_hip.h -- C ABI of the MI355X line-by-line spectrum core.
 *
 * Drop-in boundary for the spectrum-computation path of exosports/transit
 * (reference transit/src/transit.c:125-214, do_transit(): interpcs -> extwn ->
 * tau -> emergent_intens/flux | modulation, plus the Voigt-table build of
 * opacity.c:219-277 done once per handle).
 *
 * The reference dispatches this path through a per-ray plugin vtable
 *   ray_solution { name, file, monospace, optdepth(tr,b,ex), spectrum(tr,tau,w,last,toomuch,r) }
 *   (transit/include/structures_tr.h:68-83; instances eclipse.c:408, slantpath.c:573;
 *    selected by name in argum.c:752-765)
 * and through per-layer operators
 *   int computemolext(struct transit*, PREC_RES **kiso, PREC_ATM temp,
 *                     PREC_ATM *density, double *Z, int permol)   (extinction.h:25)
 * which are one-scalar-per-call and cannot feed a GPU.  This ABI keeps the same
 * selection surface (solution = "eclipse" | "transit") and the same data
 * contract, batched: one create (static data: line list, grids, Voigt grid,
 * CIA tables) and one run per atmosphere.  Plain pointers and sizes only; the
 * caller owns every host buffer, the library owns device memory.
 *
 * All functions return 0 on success and a negative trx_status on failure; they
 * never exit()/abort (reference: fw() macro transit.h:91-98 exits).
 */
#ifndef TRANSIT_HIP_H
#define TRANSIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRX_ABI_VERSION 5

typedef enum {
  TRX_OK            =  0,
  TRX_E_ARG         = -1,   /* bad argument / inconsistent sizes               */
  TRX_E_NOMEM       = -2,   /* host or device allocation failed                */
  TRX_E_HIP         = -3,   /* a HIP runtime call failed (see trx_last_error)  */
  TRX_E_NODEVICE    = -4,   /* no usable gfx950 device                         */
  TRX_E_RANGE       = -5,   /* layer temperature outside CIA / table range     */
  TRX_E_UNSUPPORTED = -6,   /* option combination not implemented              */
  TRX_E_ORDER       = -7,   /* line list not sorted as the TLI format requires */
  TRX_E_NOTREACHED  = -8    /* modlevel -1 and tau never reached toomuch       */
} trx_status;

typedef enum { TRX_SOL_ECLIPSE = 0, TRX_SOL_TRANSIT = 1 } trx_solution;

/* One collision-induced-absorption / cross-section table
 * (reference struct cross, structures_tr.h:296-307; file grammar crosssec.c:87-233). */
typedef struct {
  int32_t nspec;          /* 1 or 2 species                                    */
  int32_t mol[2];         /* indices into the atmosphere species list          */
  int32_t nwave, ntemp;
  const double *wn;       /* [nwave] cm-1                                      */
  const double *temp;     /* [ntemp] K                                         */
  const double *cs;       /* [nwave][ntemp] cm-1 amagat^-nspec                 */
} trx_cia;

/* Pre-computed opacity grid (reference struct opacity, structures_tr.h:154-171;
 * file layout opacity.c:405-421): extinction per unit density of each molecule
 * on (layer, temperature, wavenumber).  When trx_static.ogrid is set, trx_run
 * interpolates it in temperature (interpolmolext, extinction.c:535-581) instead
 * of sweeping the line list. */
typedef struct {
  int64_t nmol, ntemp, nlayer, nwave;
  const int32_t *mol_index;  /* [nmol] atmosphere species index of each grid molecule */
  const double  *temp;       /* [ntemp] K, ascending                                   */
  const double  *o;          /* [nlayer][ntemp][nmol][nwave] cm2 g-1 ... cm-1 per g cm-3 */
} trx_opacity_grid;

/* Everything that does not change between spectra
 * (reference: transit_init(), transit.c:25-74). */
typedef struct {
  int32_t abi_version;    /* TRX_ABI_VERSION                                   */
  int32_t device;         /* HIP device ordinal                                */

  /* wavenumber sampling (makewnsample, makesample.c:309-400)                 */
  double  wn_i;           /* wns.i  first coarse wavenumber, cm-1              */
  double  wn_d;           /* wns.d  coarse spacing, cm-1                       */
  int64_t nwn;            /* wns.n  coarse samples                             */
  int32_t osamp;          /* owns.o oversampling factor (wnosamp)              */
  int64_t nown;           /* owns.n fine samples = (nwn-1)*osamp+1             */
  /* this handle computes coarse bins [wn_lo, wn_hi) only (wavenumber shard of
   * a multi-GPU job); 0, nwn for the whole grid                               */
  int64_t wn_lo, wn_hi;

  /* Voigt-profile grid (opacity.c:219-277; hint fields are float,
   * structures_tr.h:326-333)                                                  */
  int32_t ndop, nlor;
  float   dmin, dmax, lmin, lmax;
  float   timesalpha;     /* nwidth                                            */

  /* line transitions, SoA as in struct line_transition (structures_tr.h:95-102);
   * TLI order: isotope blocks, ascending wavelength inside a block            */
  int64_t nlines;
  const double  *wl_um;   /* [nlines] wavelength, microns                      */
  const int16_t *isoid;   /* [nlines] cumulative isotope index                 */
  const double  *elow;    /* [nlines] lower-state energy, cm-1                 */
  const double  *gf;      /* [nlines]                                          */

  /* isotopes (struct isotopes, structures_tr.h)                               */
  int32_t niso;
  const double  *iso_mass;   /* [niso] amu                                     */
  const double  *iso_ratio;  /* [niso]                                         */
  const int32_t *iso_imol;   /* [niso] index into the species list             */

  /* atmosphere species (struct molecules)                                     */
  int32_t nmol;
  const double  *mol_mass;   /* [nmol] amu                                     */
  const double  *mol_radius; /* [nmol] cm                                      */
  const double  *mol_pol;    /* [nmol] polarizability A^3 (scattering flag 2)  */
  const int32_t *mol_is_h2;  /* [nmol] 1 for the species named "H2" (cloud P19)*/

  /* CIA tables                                                                */
  int32_t ncia;
  const trx_cia *cia;

  /* multi-GPU job: communicator from trx_comm_create (NULL for one GPU); used by
   * trx_gather only.  A handle whose shard [wn_lo, wn_hi) is a part of the grid
   * sweeps only the lines whose profiles can reach it. */
  void   *comm;
  int32_t nranks, rank;

  /* optional pre-computed opacity grid (NULL: line-by-line)                   */
  const trx_opacity_grid *ogrid;
} trx_static;

/* Per-spectrum atmosphere, already on transit's layer grid, bottom layer first
 * (reference: makeradsample(), makesample.c:409-549; the density[]/Z[] vectors
 * handed to computemolext at tau.c:164-167, 254-257). */
typedef struct {
  int32_t nlayer;
  double  rad_fct;        /* rads.fct: radius units -> cm                      */
  const double *radius;   /* [nlayer] rads.v, units of rad_fct                 */
  const double *temp;     /* [nlayer] K (atm.t * tfct; the reference's Planck
                             and scattering terms read atm.t without tfct,
                             eclipse.c:155 -- identical when ut = 1)            */
  const double *press;    /* [nlayer] atm.p as the reference stores it, i.e. in
                             atmosphere-file units; its cloud and scattering
                             models (extinction.c:608,661) assume these are bar */
  const double *density;  /* [nmol][nlayer] g cm-3                             */
  const double *abund;    /* [nmol][nlayer] mixing ratio q (cloud/scatter only; may be NULL) */
  const double *zpart;    /* [niso][nlayer] partition function Z_i(T_layer)    */
} trx_atm;

/* Per-spectrum options (reference: struct transithint fields accepted in
 * argum.c:774-911 and tau.c:12-52). */
typedef struct {
  int32_t solution;       /* trx_solution                                      */
  double  toomuch;        /* optical-depth cut (tau.c:277)                     */
  double  ethresh;        /* line-strength threshold (extinction.c:467)        */
  double  wn_fct;         /* wns.fct (output wavenumber units factor)          */
  /* eclipse */
  int32_t nangles;
  const double *angles_deg;   /* raygrid                                       */
  /* transit */
  double  starrad_cm;     /* sg->starrad * sg->starradfct                      */
  int32_t transparent;    /* sg->transpplanet                                  */
  int32_t modlevel;       /* 1 or -1                                           */
  /* clouds (struct extcloud) and scattering (struct extscat)                  */
  int32_t cloud_flag;     /* 0 none, 1 ext, 2 opa, 3 B17, 4 F18, 5 P19         */
  double  cloud_ext, cloud_top, cloud_bot, cloud_gamma, cloud_Q, cloud_r,
          cloud_sig, cloud_refwn;
  int32_t scat_flag;      /* 0 none, 1 Lecavelier, 2 polarizability            */
  double  scat_logext;
  /* execution knobs (no effect on results)                                    */
  int32_t layer_chunk;    /* layers swept per top-down step; 0 = automatic: up to 64 where the
                             profiles are narrow (one kernel walks the line list with one lane
                             per layer), up to 32 otherwise; the depth the previous spectrum
                             reached is split into equal steps                          */
  int32_t eager;          /* 1 = sweep every layer (debug dumps of all layers) */
  int32_t profile;        /* 1 = bracket the production kernels with HIP events on their own
                             streams (trx_stats ms_* timings: the run's own plan, queues and kernels,
                             with the events' packets between them); 2 = also count evaluated /
                             skipped groups and bins with the instrumented kernel variants
                             (trx_stats neval/nskip/sum_bins; those kernels run slower)   */
} trx_opts;

/* Optional intermediate outputs (host buffers, any may be NULL).  They mirror
 * the reference's --savefiles dumps (tau.c:180-190, 293-329). */
typedef struct {
  double  *e;             /* [nlayer][nwn_shard] molecular extinction          */
  double  *e_cs;          /* [nlayer][nwn_shard] CIA extinction (ref: [wn][layer]) */
  double  *tau;           /* [nwn_shard][nlayer] optical depth                 */
  int64_t *last;          /* [nwn_shard]                                       */
  double  *intens;        /* [nangles][nwn_shard] (eclipse)                    */
  uint8_t *computed;      /* [nlayer] 1 if the layer was swept                 */
  /* the arrays behind the reference's total/cloud/scatt_extion.dat dumps (tau.c:293-329):      */
  double  *er;            /* [nlayer][nwn_shard] total extinction as the ray solution left it:
                             defined for the layers a ray went through (layer >= nlayer-1-last);
                             eclipse geometry keeps its bottom-point parabola values in it
                             (eclipse.c:65-66)                                               */
  double  *e_scat;        /* [nlayer][nwn_shard] scattering extinction (extinction.c:587-624) */
  double  *e_cloud;       /* [nlayer][nwn_shard] cloud extinction (extinction.c:630-693)     */
} trx_debug;

/* Counters and device timings of the last trx_run (reference DEBUG counters
 * extinction.c:513-518; stage timers transitstd.c:359-374). */
typedef struct {
  int64_t nlines_inrange; /* lines passing the range test (extinction.c:410)   */
  int64_t ngroups;        /* co-added groups (anchors), layer independent      */
  int64_t nadd;           /* co-added lines per layer (layer independent)      */
  int64_t layers_swept;
  int64_t neval;          /* evaluated groups, summed over swept layers (these three
                             counters are collected by counting runs only: profile 2) */
  int64_t nskip;          /* groups below ethresh*kmax, summed over layers     */
  int64_t sum_bins;       /* accumulated (group,layer,bin) triples             */
  int64_t table_floats;   /* Voigt table size                                  */
  double  ms_create_table;/* device time of the Voigt-table build              */
  double  ms_run_total;   /* device time of the last run, first to last kernel (profiled runs, trx_opts.profile; else 0) */
  double  ms_sweep;       /* line-sweep kernels (profile >= 1; as ms_k_* and ms_tau) */
  double  ms_k_sweep;      /* sum over launches of k_group_sweep (the steps whose profiles are wider than the walk's widest frame) */
  double  ms_k_walk;       /* sum over launches of the walk kernels (k_line_walk, k_line_walk_lanes, k_line_walk_packed)      */
  double  ms_k_accum;     /* sum over launches of k_walk_combine and k_accumulate(_wide/_rows) */
  int64_t sweep_launches; /* launches of each sweep kernel (gated no-op ones too) */
  double  ms_tau;         /* optical-depth kernels                             */
  double  ms_cia;         /* host wall time of queueing the CIA kernels          */
  double  ms_host_total;  /* host wall time of the whole trx_run call           */
  double  ms_spectrum;    /* intensity/flux or modulation                      */
  int64_t ncandidates;    /* lines that can be a layer's strongest line (the others are
                             dominated, trx_walk.hip.h); -1: every line is looked at */
  int64_t walk_steps;     /* steps of the last run taken by the one-kernel line walk (the
                             rest, sweep_launches - walk_steps, took the two-kernel form)  */
  int64_t walk_records;   /* partial-sum records (64 lane slots each) those steps wrote   */
  int64_t walk_record_lanes; /* lane slots of them actually written and read: sum over steps of
                             records x layers of the step (8 bytes each)                 */
  int64_t walk_layers;    /* layers of the last run swept by walk steps (the rest of layers_swept: two-kernel steps) */
  int64_t sum_bins_walk;  /* the part of sum_bins accumulated by walk steps (counting runs)                          */
  /* the walk steps by kernel form (ABI 4): [0] k_line_walk (lanes = layers, one range per wave),
     [1] k_line_walk_lanes (lanes = lines for the strengths), [2] k_line_walk_packed (several ranges per wave) */
  int64_t walk_form_steps[3];        /* steps of the last run                                                   */
  int64_t walk_form_layers[3];       /* layers they swept                                                       */
  int64_t walk_form_record_lanes[3]; /* their share of walk_record_lanes                                        */
  int64_t walk_form_bins[3];         /* their share of sum_bins_walk (counting runs)                            */
  double  ms_k_walk_form[3];         /* their share of ms_k_walk (profile >= 1)                                 */
  double  ms_walk_span;              /* (ABI 5) first walk's start to last walk's end of the last run: where the walks of a hinted run share
                                        the device on two queues, less than ms_k_walk, the sum of their own durations (profile >= 1) */
} trx_stats;

typedef struct trx_handle trx_handle;

int  trx_abi_version(void);
/* Extinction of layers computed by an earlier run (the reference's --saveext file: restfile_extinct,
 * extinction.c:97-137, called at the head of tau(), tau.c:155-156).  The following trx_run calls take
 * e[layer][.] of every flagged layer from here instead of sweeping it (a step whose layers are all
 * flagged launches no line kernel); flags and values stay until replaced (nlayer = 0: forget them).
 * e: [nlayer][nwn_shard] host memory, this handle's shard; computed: [nlayer]. */
int  trx_restore_extinction(trx_handle *h, int32_t nlayer, const double *e, const uint8_t *computed);
int  trx_device_count(void);
/* HIP version the library was built with / of the runtime it runs on (HIP_VERSION encoding:
 * major*10000000 + minor*100000 + patch); a caller that maps a runtime of its own first can check. */
int  trx_hip_versions(int *built, int *running);

int  trx_create (const trx_static *st, trx_handle **out);
int  trx_run    (trx_handle *h, const trx_atm *atm, const trx_opts *opts,
                 double *spectrum /* [wn_hi-wn_lo], host */, trx_debug *dbg /* may be NULL */);
/* Same as trx_run but leaves the spectrum in device memory (d_spectrum is a
 * device pointer on the handle's device, e.g. a torch tensor for an RCCL
 * gather); work is enqueued on the handle's stream and synchronised on return. */
int  trx_run_device(trx_handle *h, const trx_atm *atm, const trx_opts *opts,
                    void *d_spectrum, trx_debug *dbg);
void trx_destroy(trx_handle *h);

/* Several atmospheres per call -- what a retrieval driver does with the reference by calling run_transit
 * (transit.c:118-122) once per atmosphere.  A batch keeps `ways` handles made from one description (line list
 * and tables `ways` times in device memory) and a host thread for each; trx_run_batch deals the k
 * atmospheres to them and returns when all are done.  spectra[j] ([wn_hi-wn_lo], host) is what
 * trx_run(h, &atm[j], opts, spectra[j], NULL) gives, bit for bit.  On failure: the first error's code, its
 * text through trx_last_error(NULL); spectra of other atmospheres may or may not have been written. */
#define TRX_BATCH_MAX_WAYS 8
typedef struct trx_batch trx_batch;
int  trx_batch_create(const trx_static *st, int32_t ways, trx_batch **out);
int  trx_run_batch(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *opts,
                   double *const *spectra /* [k] */);
int  trx_batch_ways(const trx_batch *b);
void trx_batch_destroy(trx_batch *b);

/* Band integrals on the device: the spectrum reduced to an instrument's channels (filter curves, top-hat
 * bins, a Gaussian line-spread function at pixel centres) without handing the whole spectrum back.
 *
 * A band is a weight w_i per coarse bin i of the whole grid (i = 0 .. nwn-1, nu_i = wn_i + i*wn_d):
 *   TRX_BAND_WEIGHTS  bins first .. first+n-1, w_{first+k} = weights[k] (finite; copied at trx_set_bands)
 *   TRX_BAND_GAUSS    sigma = fwhm / (2 sqrt(2 ln 2)); bins i_lo = ceil((centre - cut*sigma - wn_i)/wn_d) to
 *                     i_hi = floor((centre + cut*sigma - wn_i)/wn_d), clipped to [0, nwn) (computed on the host in
 *                     double; an empty range is allowed); w_i = exp(-((nu_i - centre)/sigma)^2 / 2), evaluated on
 *                     the device
 * A run gives sums[b][0] = sum of w_i S_i and sums[b][1] = sum of w_i over the band's bins in this handle's shard
 * [wn_lo, wn_hi); the band's value is sums[b][0] / sums[b][1].  A sharded job adds the ranks' sums in rank order
 * (e.g. trx_gather_host of the [nbands][2] partials); a band with no bin in the shard gives exactly (0, 0).
 * The sums have no atomics: the bits of a band's pair depend on the spectrum, the band and the shard only -- not on
 * the other bands of the set, the launch, the batch way that ran it or the handle's depth hint.
 *
 * trx_set_bands copies the set to the device (nbands = 0: clear it).  It returns TRX_E_ARG, naming the band in
 * trx_last_error, for nbands < 0, an unknown kind, n < 1, first < 0, first + n > nwn, a NULL or non-finite weight,
 * a non-finite centre, fwhm or cut, fwhm <= 0 or cut <= 0; a refused set leaves the previous one in force.
 * trx_run_bands is trx_run plus the band sums: spectrum may be NULL (then the spectrum stays on the device), and
 * when it is given it holds the bits trx_run gives.  It returns TRX_E_ARG with no set installed or sums NULL.
 * trx_batch_set_bands installs the same set on every handle of the batch, or on none (its reason through
 * trx_last_error(NULL)); trx_run_batch_bands is trx_run_batch with sums[j] ([nbands][2]) for spectra[j]. */
typedef enum { TRX_BAND_WEIGHTS = 0, TRX_BAND_GAUSS = 1 } trx_band_kind;
typedef struct {
  int32_t kind, pad;        /* trx_band_kind; pad is ignored                                       */
  int64_t first, n;         /* WEIGHTS: global coarse bins first .. first+n-1 of the whole grid     */
  const double *weights;    /* WEIGHTS: [n], finite                                                 */
  double centre, fwhm, cut; /* GAUSS: cm-1, cm-1 (> 0), half-width in sigmas (> 0)                  */
} trx_band;
int  trx_set_bands(trx_handle *h, int32_t nbands, const trx_band *bands);
int  trx_run_bands(trx_handle *h, const trx_atm *a, const trx_opts *o,
                   double *spectrum /* [wn_hi-wn_lo], host; may be NULL */, double *sums /* [nbands][2] */,
                   trx_debug *dbg /* may be NULL */);
int  trx_batch_set_bands(trx_batch *b, int32_t nbands, const trx_band *bands);
int  trx_run_batch_bands(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                         double *const *sums /* [k] -> [nbands][2] */);

/* Contribution functions on the device: where in the atmosphere each band of the installed set comes from, one
 * number per (band, layer), from the run's own optical depths -- the optical depths never leave the device.
 *
 * Heights are counted as the optical-depth arrays count them: i = 0 is the top layer, height i is atmosphere layer
 * r = nlayer-1-i, `last` is the ray's last height (trx_debug.last).  Per wavenumber bin j:
 *   eclipse geometry   t_a,i = exp(-tau_i / cos(angle_a)),  area_a = sin^2(grid_{a+1}) - sin^2(grid_a) (eclipse.c:262-276),
 *                      B_i = the Planck function at layer nlayer-1-i (eclipse.c:154)
 *                        g_i = pi * sum_a area_a * t_a,i                     i = 0 .. last
 *                        d_i = g_i - g_{i+1}                                 i = 0 .. last-1
 *                        W_0 = d_0 / 2,  W_i = (d_{i-1} + d_i) / 2 (0 < i < last),  W_last = d_{last-1} / 2 + g_last
 *                        (last = 0: W_0 = g_0);  W_i = 0 for i > last
 *                        F_i = B_i * W_i
 *                      This is the reference's quadrature (eclipse_intens: B[last] dtau[last] - integ_trapz(dtau, B,
 *                      last+1), then flux()) regrouped by node: sum_i F_i is the flux of bin j, every term is >= 0.
 *   transit geometry   F_i = exp(-tau_i) for i <= last, 0 below (what modulation1 integrates, slantpath.c:374-386),
 *                      whatever modlevel.
 * contrib[b][r] = sum over the band's bins j in this handle's shard of w_j * F_{nlayer-1-r}(j), rows in the
 * ATMOSPHERE's layer order (bottom first, like trx_atm), the weights w_j exactly those of the band sums.  Eclipse:
 * sum_r contrib[b][r] = sums[b][0] up to summation rounding.  Transit: contrib[b][r] / sums[b][1] is the band-averaged
 * transmittance at layer r's impact parameter.
 *
 * A sharded job adds the ranks' rows in rank order, like the band sums (e.g. trx_gather_host of the nbands*nlayer
 * partials); a band with no bin in the shard gives a row of exact zeros.  No atomics: a row's bits depend on the
 * optical depths, the band and the shard only -- not on the other bands of the set, the launch, the batch way, the
 * handle's depth hint or the kernels that made the optical depths.
 *
 * trx_run_contrib is trx_run_bands plus contrib: spectrum (when asked for) and sums hold the bits trx_run_bands
 * gives.  TRX_E_ARG (reason in trx_last_error) with no set installed, sums NULL or contrib NULL.  A run that fails
 * leaves contrib undefined.  trx_run_batch_contrib is trx_run_batch_bands with contrib[j] ([nbands][atm[j].nlayer])
 * next to sums[j]. */
int  trx_run_contrib(trx_handle *h, const trx_atm *a, const trx_opts *o,
                     double *spectrum /* [wn_hi-wn_lo], host; may be NULL */, double *sums /* [nbands][2] */,
                     double *contrib /* [nbands][a->nlayer] */, trx_debug *dbg /* may be NULL */);
int  trx_run_batch_contrib(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                           double *const *sums /* [k] -> [nbands][2] */,
                           double *const *contrib /* [k] -> [nbands][atm[j].nlayer] */);

/* Detector pixels at Doppler shifts on the device: the last step of a high-resolution cross-correlation retrieval --
 * the spectrum shifted to the planet's velocity at each exposure, convolved with the spectrograph's Gaussian
 * line-spread function and sampled at the detector's pixel centres -- without handing the spectrum back, and without
 * a band per (pixel, shift) pair: the pixel set is installed once, the shifts come with every run, ranges and weights
 * are made on the device.
 *
 * shift[v] = nu_observed / nu_rest: 1 at rest, below 1 for a receding source.  The pair out[v][p] is exactly the pair
 * of the band TRX_BAND_GAUSS{centre = centre_p / shift_v, fwhm = fwhm_p / shift_v, cut} under the rules of
 * trx_set_bands above:
 *   centre' = centre_p / shift_v,  fwhm' = fwhm_p / shift_v,  sigma = fwhm' / (2 sqrt(2 ln 2))
 *   i_lo = ceil((centre' - cut*sigma - wn_i)/wn_d),  i_hi = floor((centre' + cut*sigma - wn_i)/wn_d),
 *   clipped to [0, nwn) and then to the shard (an empty range is allowed)
 *   w_i = exp(-((nu_i - centre')/sigma)^2 / 2)
 *   out[v][p] = (sum of w_i S_i, sum of w_i) over those bins; the pixel's value is out[v][p][0] / out[v][p][1].
 * The two divisions and the range expressions are IEEE double with every operation rounded once (no fused
 * multiply-add, on the device either): the range of a pair is the same integers as the equivalent band's.  The
 * weight is the expression the band kernel evaluates (one device function serves both): the two paths differ in the
 * order of their sums only.
 *
 * No atomics: the bits of a pair depend on the spectrum, that pixel, that shift and the shard only -- not on the other
 * pixels or shifts of the call, the launch, the batch way that ran it or the handle's depth hint.  (A window of fewer
 * than 192 in-shard bins is added by one lane in ascending bin order; a longer one by a wave, lane l adding its bins
 * l, l + 64, ... in that order, then a fixed butterfly over the lanes.)  A sharded job adds the ranks' pairs in rank
 * order, as for bands; a pair with no bin in the shard is exactly (+0, +0).
 *
 * trx_set_pixels copies the set to the device (px NULL or npix = 0: clear it).  It returns TRX_E_ARG, the reason in
 * trx_last_error (naming "pixel N" where one pixel is at fault), for npix < 0, a NULL array, a non-finite or <= 0
 * centre or fwhm, a non-finite or <= 0 cut; a refused set leaves the previous one in force.
 * trx_run_pixels is trx_run plus the pairs: spectrum may be NULL (then the spectrum stays on the device), and when it
 * is given it holds the bits trx_run gives.  TRX_E_ARG with no set installed, nshift < 1, shift or out NULL, a
 * non-finite or <= 0 shift (naming "shift N").  A run that fails leaves out undefined.  trx_run, trx_run_bands and
 * trx_run_contrib on a handle with pixels installed are unchanged.
 * trx_batch_set_pixels installs the same set on every handle of the batch, or on none (its reason through
 * trx_last_error(NULL)); trx_run_batch_pixels is trx_run_batch with atmosphere j's own shifts shift[j] ([nshift]) and
 * its pairs out[j] ([nshift][npix][2]). */
typedef struct {
  int64_t npix;
  const double *centre;     /* [npix] pixel centres, cm-1, OBSERVED frame; finite, > 0; any order         */
  const double *fwhm;       /* [npix] line-spread FWHM at that pixel, cm-1, observed frame; finite, > 0   */
  double cut;               /* half-width of the window in sigmas; finite, > 0                            */
} trx_pixels;
int  trx_set_pixels(trx_handle *h, const trx_pixels *px);
int  trx_run_pixels(trx_handle *h, const trx_atm *a, const trx_opts *o,
                    double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                    int32_t nshift, const double *shift /* [nshift] */,
                    double *out /* [nshift][npix][2], host */, trx_debug *dbg /* may be NULL */);
int  trx_batch_set_pixels(trx_batch *b, const trx_pixels *px);
int  trx_run_batch_pixels(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                          int32_t nshift, const double *const *shift /* [k] -> [nshift] */,
                          double *const *out /* [k] -> [nshift][npix][2] */);

/* Cross-correlation moments of the detector pixels against observed data, on the device: what a driver reduces the
 * [nshift][npix][2] matrix of trx_run_pixels to -- per exposure and spectral order a correlation coefficient, a
 * log-likelihood or a chi-square, all functions of seven weighted sums over the order's pixels -- without handing the
 * matrix back: the observed set is installed once over the pixel set, a run returns [nexp][nseg][TRX_NMOMENT] doubles.
 *
 * An exposure is a shift of the run (nshift = nexp); a segment s is the pixels [seg_first[s], seg_first[s+1]) of the
 * installed pixel set.  For exposure v and pixel p, (a, b) = out[v][p] is exactly the pair trx_run_pixels gives for
 * that shift and pixel (the same kernel, the same bits), f = data[v][p], w = weight[v][p] (1 without weights).
 *   a pixel CONTRIBUTES when b > 0 and w > 0
 *   its model value is g = gain_p * (a / b): one division, one product, each rounded once (no fused multiply-add)
 * and over the contributing pixels of segment s
 *   mom[v][s][0] = n, their number (as a double)     mom[v][s][4] = sum of w f
 *   mom[v][s][1] = sum of w                          mom[v][s][5] = sum of w f g
 *   mom[v][s][2] = sum of w g                        mom[v][s][6] = sum of w f^2
 *   mom[v][s][3] = sum of w g^2
 * with the terms (w g) g, (w f) g and (w f) f, every product rounded once.  A segment with no contributing pixel gives
 * seven exact +0.
 *
 * The order of the sums is fixed: one wavefront adds a (v, s) row, lane l the segment's pixels first + l,
 * first + l + 64, ... in that order, then the fixed butterfly over the 64 lanes that the long pixel windows use.  No
 * atomics: the bits of a row depend on the spectrum, that segment's pixels, data and weights, that shift and nothing
 * else -- not on the other segments or exposures of the call, the launch, the batch way that ran it or the handle's
 * depth hint.  (A segment is one wave's work whatever its length: nexp * nseg is the parallel axis.)
 *
 * The observed set belongs to the pixel set it was installed over: trx_set_observed without a pixel set is TRX_E_ARG,
 * a successful trx_set_pixels (a clearing one included) drops the observed set, a refused one leaves both in force.
 * trx_set_observed copies seg_first, data, weight and gain to the device (ob NULL or nexp = 0: clear it).  It returns
 * TRX_E_ARG, the reason in trx_last_error, for nexp < 0, nseg < 1, a NULL seg_first or data, seg_first[0] != 0, a
 * decreasing entry, seg_first[nseg] != npix, nexp * nseg above 2^31 - 1, a non-finite datum or a negative or
 * non-finite weight (naming "exposure N pixel M"), a non-finite gain (naming "pixel M"); a refused set leaves the
 * previous one in force.
 * trx_run_moments is trx_run_pixels plus the reduction: spectrum may be NULL, and when it is given it holds the bits
 * trx_run gives; only mom is copied back, the pairs stay in device memory.  TRX_E_ARG with no observed set installed,
 * nshift != nexp, shift or mom NULL, a non-finite or <= 0 shift (naming "shift N").  The moments are not linear in the
 * pairs, so the partial pairs of shards cannot be reduced rank by rank: on a handle whose shard is not the whole grid
 * (wn_lo != 0 or wn_hi != nwn) it returns TRX_E_UNSUPPORTED -- such a job takes trx_run_pixels, adds the ranks' pairs
 * (trx_gather_host) and reduces them itself.  A run that fails leaves mom undefined.  trx_run, trx_run_bands,
 * trx_run_contrib and trx_run_pixels on a handle with an observed set installed are unchanged.
 * trx_batch_set_observed installs the same set on every handle of the batch, or on none (its reason through
 * trx_last_error(NULL)); trx_run_batch_moments is trx_run_batch with atmosphere j's own shifts shift[j] ([nshift]) and
 * its moments mom[j] ([nexp][nseg][TRX_NMOMENT]). */
#define TRX_NMOMENT 7
typedef struct {
  int32_t nexp, nseg;        /* exposures (= the shifts of a run), segments (orders / detectors)            */
  const int64_t *seg_first;  /* [nseg+1] segment s = pixels [seg_first[s], seg_first[s+1]) of the installed  */
                             /* pixel set; seg_first[0] = 0, non-decreasing (an empty segment is allowed),   */
                             /* seg_first[nseg] = npix                                                       */
  const double *data;        /* [nexp][npix] observed value f, finite                                        */
  const double *weight;      /* [nexp][npix] w >= 0, finite (1/sigma^2; 0 masks a pixel); NULL: all 1        */
  const double *gain;        /* [npix] finite factor on the model value (e.g. (Rp/Rs)^2 / Fstar); NULL: 1    */
} trx_observed;
int  trx_set_observed(trx_handle *h, const trx_observed *ob);
int  trx_run_moments(trx_handle *h, const trx_atm *a, const trx_opts *o,
                     double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                     int32_t nshift, const double *shift /* [nshift], nshift = nexp */,
                     double *mom /* [nexp][nseg][TRX_NMOMENT], host */, trx_debug *dbg /* may be NULL */);
int  trx_batch_set_observed(trx_batch *b, const trx_observed *ob);
int  trx_run_batch_moments(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                           int32_t nshift, const double *const *shift /* [k] -> [nshift] */,
                           double *const *mom /* [k] -> [nexp][nseg][TRX_NMOMENT] */);

/* The detrending filter between the pixels and their moments, on the device.  Observed exposures are detrended before
 * they are compared with a model -- per spectral order the leading components in time (airmass, throughput, tellurics)
 * are fitted and taken out -- and the same operation has to be applied to the model, or the likelihood is biased: the
 * model reprocessing of Brogi & Line (2019) in the linear form of Gibson et al. (2022), M' = M - U (U^+ M).  It is a
 * small linear map along the EXPOSURE axis of every pixel column; with it installed the whole likelihood stays on the
 * device: spectrum -> pixels -> filter -> moments.
 *
 * A filter belongs to the observed set it is installed over.  It has one ncomp (1 .. TRX_FILTER_MAX) for all segments
 * and per segment s two matrices: fwd[s][j][v] ([nseg][ncomp][nexp]), the coefficients C, and back[s][v][j]
 * ([nseg][nexp][ncomp]), the basis B; a segment that wants fewer components pads with zeros.  For pixel p of segment
 * s and exposure v, (a, b) is the pair trx_run_pixels gives and g[v][p] = gain_p * (a / b) as in the moments.
 *   column p is LIVE when b > 0 at every exposure
 *   otherwise it is DEAD, and all its values are quiet NaN: the projection needs the whole column, so a pixel whose
 *   window leaves the grid at some exposures cannot be filtered
 * and for a live column
 *   c_j      = sum over v = 0 .. nexp-1, in that order, of fwd[s][j][v] * g[v][p]        j = 0 .. ncomp-1
 *   r_v      = sum over j = 0 .. ncomp-1, in that order, of back[s][v][j] * c_j
 *   g'[v][p] = g[v][p] - r_v
 * every product and sum rounded once (no fused multiply-add), both sums started from +0.  The weights take no part in
 * the projection: a caller who wants a weighted fit folds them into fwd.
 *
 * The filtered moments are the seven sums of trx_run_moments with g' in place of g, over the pixels whose value is not
 * NaN and whose w > 0: the same terms, roundings, lane order and butterfly.  A row with no such pixel gives seven exact
 * +0.  No atomics: the bits of a value depend on its column's pairs and gain and on its segment's two matrices and
 * ncomp -- not on other columns or segments, the launch, the batch way that ran it or the handle's depth hint.
 *
 * trx_set_filter copies both matrices to the device (f NULL or ncomp = 0: clear the filter).  It returns TRX_E_ARG, the
 * reason in trx_last_error, with no observed set installed, for ncomp < 0 or > TRX_FILTER_MAX, a NULL fwd or back, a
 * non-finite entry (naming "segment S"); a refused filter leaves the previous one in force.  A successful
 * trx_set_observed (a clearing one included) drops the filter, a successful trx_set_pixels drops both.
 * trx_run_filtered_moments is trx_run_moments plus the filter: spectrum may be NULL, and when it is given it holds the
 * bits trx_run gives; values, when given, receives g' ([nexp][npix], NaN in dead columns) for inspection and tests --
 * without it only mom is copied back.  TRX_E_ARG with no filter installed, for every refusal of trx_run_moments, or
 * with mom NULL; TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid.  A run that fails leaves values and
 * mom undefined.  trx_run, trx_run_bands, trx_run_contrib, trx_run_pixels and trx_run_moments on a handle with a filter
 * installed are unchanged, bit for bit.
 * trx_batch_set_filter installs the same filter on every handle of the batch, or on none (its reason through
 * trx_last_error(NULL)); trx_run_batch_filtered_moments deals the atmospheres exactly as trx_run_batch_moments does. */
#define TRX_FILTER_MAX 16
typedef struct {
  int32_t ncomp, pad;        /* components, 1 .. TRX_FILTER_MAX (0: clear); pad: 0                           */
  const double *fwd;         /* [nseg][ncomp][nexp] coefficients, finite                                     */
  const double *back;        /* [nseg][nexp][ncomp] basis, finite                                            */
} trx_filter;
int  trx_set_filter(trx_handle *h, const trx_filter *f);
int  trx_run_filtered_moments(trx_handle *h, const trx_atm *a, const trx_opts *o,
                              double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                              int32_t nshift, const double *shift /* [nshift], nshift = nexp */,
                              double *values /* [nexp][npix], host; may be NULL */,
                              double *mom /* [nexp][nseg][TRX_NMOMENT], host */, trx_debug *dbg /* may be NULL */);
int  trx_batch_set_filter(trx_batch *b, const trx_filter *f);
int  trx_run_batch_filtered_moments(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                                    int32_t nshift, const double *const *shift /* [k] -> [nshift] */,
                                    double *const *mom /* [k] -> [nexp][nseg][TRX_NMOMENT] */);

/* The WEIGHTED detrending filter: the filter slot's second kind.  The plain filter projects every pixel column of a
 * segment with the same coefficients; the detrending applied to real data (SYSREM, PCA with masks) is a WEIGHTED fit
 * per column, and the model has to go through the same operation (Gibson et al. 2022):
 *   M' = M - U (U^T L U)^-1 U^T L M,    L = diag of the column's own weights
 * A weighted filter has one ncomp (1 .. TRX_FILTER_MAX) and per segment s the time vectors U = basis[s] ([nexp][ncomp]);
 * a segment that wants fewer components must not pad with zeros (a zero vector is a singular pivot).  The weights are the
 * observed set's weight[v][p] (NULL: all 1).  For pixel p of segment s, g[v] = gain_p * (a / b) as in the plain filter,
 * w[v] = weight[v][p], n = ncomp.  Every operation is IEEE double rounded once, no fused multiply-add; sums start from
 * +0 and run in the order written.
 *
 * At install, once per column:
 *   for j = 0 .. n-1, k = 0 .. j:   N_jk = sum over v ascending of (U[v][j] * w[v]) * U[v][k]
 *   for j = 0 .. n-1:
 *     for k = 0 .. j-1:  s = N_jk;  for m = 0 .. k-1: s = s - T_jm * L_km;   T_jk = s;  L_jk = s / D_k
 *     D_j = N_jj;        for k = 0 .. j-1: D_j = D_j - T_jk * L_jk
 *     pivot j is SINGULAR if not (D_j > TRX_WFILTER_PIVOT * N_jj)             (N_jj = 0 and NaN included)
 * Per run:
 *   y_j = sum over v ascending of (U[v][j] * w[v]) * g[v]
 *   z_j = y_j - (sum over k < j, k ascending, of L_jk * z_k);   q_j = z_j / D_j            j ascending
 *   c_j = q_j - (sum over k > j, k ascending, of L_kj * c_k)                               j descending
 *   r_v = sum over j ascending of U[v][j] * c_j;                g'[v] = g[v] - r_v
 * A column is LIVE when b > 0 at every exposure (the plain filter's rule) AND no pivot was singular; any other column is
 * DEAD and all its values are quiet NaN.  The pivot rule makes dead a column with fewer positive weights than
 * components, a column masked at every exposure, and a column whose basis is degenerate under its weights.  The moments
 * skip NaN values: such a column contributes nothing.  The kernels pad the components to 4, 8 or 16; a padded component
 * takes no part in a pivot and changes no bit.  The bits of a value depend on its column's pairs, gain and weights and on
 * its segment's basis and ncomp only.
 *
 * The weighted filter occupies the handle's ONE filter slot: trx_set_weighted_filter replaces a plain filter,
 * trx_set_filter a weighted one; f NULL or ncomp = 0 clears the slot; trx_set_observed and trx_set_pixels drop it as
 * they drop the plain one.  nsingular, when given, receives the number of columns, over all npix, with a singular pivot
 * (0 for a clearing call).  With it installed trx_run_filtered_moments, trx_run_filtered_map and their batch forms run
 * the weighted kernels where they ran the plain ones: same signatures, refusals and outputs, the same input pairs (after
 * the exposure table and the high-pass where those are installed).  Every other entry point is unchanged, bit for bit.
 * TRX_E_ARG, the reason in trx_last_error, the previous filter of either kind left in force: no observed set installed,
 * ncomp < 0 or > TRX_FILTER_MAX, a NULL basis, a non-finite basis entry (naming "segment S").
 * trx_batch_set_weighted_filter installs it on every handle of the batch, or on none (trx_last_error(NULL)). */
#define TRX_WFILTER_PIVOT 0x1p-26           /* a pivot at or below this share of its diagonal entry: singular */
typedef struct {
  int32_t ncomp, pad;        /* components, 1 .. TRX_FILTER_MAX (0: clear); pad: 0                       */
  const double *basis;       /* [nseg][nexp][ncomp], finite: the time vectors U of every segment          */
} trx_wfilter;               /* 16 bytes */
int  trx_set_weighted_filter(trx_handle *h, const trx_wfilter *f, int64_t *nsingular /* may be NULL */);
int  trx_batch_set_weighted_filter(trx_batch *b, const trx_wfilter *f);

/* Rotational broadening of the spectrum on the device, between the spectrum and the detector pixels: the planet's own
 * velocity broadening -- the rotation kernel of v sin i with linear limb darkening -- that a high-resolution retrieval
 * applies before the instrument's line-spread function.  Its width is a fitted parameter (it changes with every
 * likelihood call) and its profile is not a Gaussian, so it cannot be folded into the pixel set's fwhm; with it
 * installed the chain spectrum -> broadening -> pixels -> filter -> moments stays on the device.  (An extra GAUSSIAN
 * velocity broadening needs none of this: it is exact through the pixels' fwhm, added in quadrature.)
 *
 * The grid is nu_i = wn_i + i*wn_d, i = 0 .. nwn-1, as for bands.  A broadening is {kind = TRX_BROADEN_ROTATION,
 * beta = v sin i / c, limb = the linear limb-darkening coefficient in [0, 1]}.  For output bin i, every operation
 * IEEE double rounded once, and without fused multiply-add where marked # (the integers h_i are then the same on host
 * and device):
 *   nu_i = wn_i + (double)i * wn_d        #
 *   d_i  = nu_i * beta                    #   half-width in cm-1 (first order in beta)
 *   h_i  = floor(d_i / wn_d)              #   half-width in bins; non-decreasing in i
 *   h_i == 0:  B_i = S_i exactly (a copy)
 *   else
 *     w_0 = c1 + c2,   c1 = 2 (1 - limb),  c2 = (pi / 2) limb
 *     num = w_0 * S_i,  den = w_0
 *     for k = 1 .. h_i, ascending:
 *         x = ((double)k * wn_d) / d_i ;  t = max(0, 1 - x*x) ;  w = c1 * sqrt(t) + c2 * t
 *         s = (S_{i-k} if i-k >= 0 else +0) + (S_{i+k} if i+k < nwn else +0)
 *         m = the number of those two bins inside the grid (0, 1 or 2)
 *         num += w * s ;  den += w * m
 *     B_i = num / den
 * This is Gray's rotation profile sampled at the bin centres and renormalised by the weights actually used: at the
 * grid's ends the window is one-sided, as the pixel windows are clipped there.  No atomics: the bits of B_i depend on S
 * over [i - h_i, i + h_i], on beta and on limb only -- not on the launch, the batch way that ran it or the handle's
 * depth hint.
 *
 * trx_set_broadening stores the two scalars (nothing is copied to the device); br NULL or kind TRX_BROADEN_NONE clears
 * it.  The broadening stays in force until it is replaced or cleared and is independent of the pixel, observed and
 * filter sets: trx_set_pixels does not drop it.  It returns TRX_E_ARG, the reason in trx_last_error, for an unknown
 * kind, a non-finite or <= 0 beta, a non-finite limb or one outside [0, 1], a handle with wn_i <= 0 or wn_d <= 0, and
 * for h_{nwn-1} > TRX_BROADEN_MAX_HALF (the error names the half-width); TRX_E_UNSUPPORTED on a handle whose shard is
 * not the whole grid (the window needs neighbours across the shard's edge: such a job gathers the spectrum and
 * broadens it itself, as it already does for the moments).  A refused call leaves the previous broadening in force.
 *
 * trx_run_broadened is trx_run plus B: spectrum may be NULL, and when it is given it holds the bits trx_run gives --
 * never the broadened spectrum.  TRX_E_ARG with no broadening installed or broadened NULL.  A run that fails leaves
 * broadened undefined.
 * With a broadening installed, trx_run_pixels, trx_run_moments and trx_run_filtered_moments (and their batch forms)
 * sample B in place of S: every pair is exactly what the pixel kernel gives when its spectrum is the buffer
 * trx_run_broadened returns -- the same kernel, unchanged.  trx_run, trx_run_device, trx_run_bands, trx_run_contrib and
 * trx_sweep_permol are unchanged bit for bit whatever is installed, and with nothing installed every entry point is.
 *
 * trx_batch_set_broadening: a retrieval's walkers carry a v sin i each, so br[j] belongs to atmosphere j of the
 * following batch pixel, moment, filtered-moment and broadened runs; n = 1: the same broadening for every atmosphere;
 * n = 0: clear it.  All n entries are checked before any is kept, or none is (the reason through
 * trx_last_error(NULL)).  Such a run of k atmospheres with n != 1 and n != k returns TRX_E_ARG.  trx_run_batch,
 * trx_run_batch_bands and trx_run_batch_contrib ignore the broadening.  trx_run_batch_broadened is trx_run_batch with
 * broadened[j] ([nwn]) in place of the spectra. */
typedef enum { TRX_BROADEN_NONE = 0, TRX_BROADEN_ROTATION = 1 } trx_broaden_kind;
typedef struct {
  int32_t kind, pad;         /* trx_broaden_kind; pad is ignored                                             */
  double beta, limb;         /* v sin i / c (finite, > 0); limb-darkening coefficient, finite, in [0, 1]     */
} trx_broadening;
#define TRX_BROADEN_MAX_HALF 2048          /* largest h_i a handle accepts */
int  trx_set_broadening(trx_handle *h, const trx_broadening *br);
int  trx_run_broadened(trx_handle *h, const trx_atm *a, const trx_opts *o,
                       double *spectrum /* [nwn], host; may be NULL */, double *broadened /* [nwn], host */,
                       trx_debug *dbg /* may be NULL */);
int  trx_batch_set_broadening(trx_batch *b, int32_t n, const trx_broadening *br /* [n] */);
int  trx_run_batch_broadened(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                             double *const *broadened /* [k] -> [nwn] */);

/* The cross-correlation trail on the device: one model against EVERY exposure of the observed set at EVERY lag of a
 * velocity grid -- CCF[lag][exposure], and the Kp-Vsys map a driver makes from it -- from one spectrum and one pass over
 * the data.  (trx_run_moments answers the other question: one shift per exposure, the likelihood at one (Kp, Vsys).)
 *
 * lag[l] is a Doppler factor nu_observed / nu_rest, as shift[] is.  trail[l][v][s][:] are the seven moments of
 * trx_run_moments for exposure v and segment s of the installed observed set -- its data, weights and gain -- with the
 * model pair of pixel p the pair trx_run_pixels gives for the shift lag[l].  The contributing rule (b > 0 and w > 0), the
 * terms (w g, (w g) g, w f, (w f) g, (w f) f, each rounded once, no fused multiply-add) and the order of the sums (lane k
 * adds the segment's pixels first + k, first + k + 64, ..., then the same butterfly over the 64 lanes) are those of
 * trx_run_moments, so
 *   trail[l] is bit for bit what trx_run_moments returns on the same handle when all nexp shifts equal lag[l]
 *   (on a handle without an exposure table: the trail ignores one, trx_set_exposures).
 * It follows that
 *   - there are no atomics;
 *   - the bits of a row depend on the spectrum, that lag, and that exposure's data, weights and gains over that segment:
 *     not on the other lags of the call (a repeated lag gives a repeated row), the tile of lags and exposures a row was
 *     computed in, the launch, the batch way that ran it or the handle's depth hint;
 *   - a row with no contributing pixel is seven exact +0;
 *   - the sums cannot go through the matrix cores, whose order of addition is another.
 *
 * With a broadening installed the pairs sample the broadened spectrum, as in every other pixel run.  An installed FILTER
 * IS IGNORED: the filter couples the exposures of a pixel column, and a trail's model is the same at all of them (the
 * column is a constant) -- the trail's bits are the same with and without a filter on the handle.  A driver that detrends
 * applies the filter to the data it installs -- or takes trx_run_filtered_map, which applies it to every map cell's
 * own model matrix.
 *
 * trx_run_trail is trx_run_pixels with nshift = nlag plus the reduction: spectrum may be NULL, and when it is given it
 * holds the bits trx_run gives; only trail is copied back, the [nlag][npix] pairs stay in device memory.  TRX_E_ARG, the
 * reason in trx_last_error, with no observed set installed, nlag < 1, lag or trail NULL, a non-finite or <= 0 lag
 * (naming "lag N"), nlag * npix above what one pixel launch takes (2^31 - 1 blocks of 256 pairs), nlag * nexp * nseg
 * above 2^31 - 1; TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid, for trx_run_moments' reason.  A run
 * that fails leaves trail undefined.  Every other run on the handle is unchanged, bit for bit.
 * trx_run_batch_trail is trx_run_batch with atmosphere j's own lags lag[j] ([nlag]) and its trail trail[j]; the batch's
 * broadenings apply as in trx_run_batch_moments. */
int  trx_run_trail(trx_handle *h, const trx_atm *a, const trx_opts *o,
                   double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                   int32_t nlag, const double *lag /* [nlag], nu_observed / nu_rest, as shift[] */,
                   double *trail /* [nlag][nexp][nseg][TRX_NMOMENT], host */, trx_debug *dbg /* may be NULL */);
int  trx_run_batch_trail(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                         int32_t nlag, const double *const *lag /* [k] -> [nlag] */,
                         double *const *trail /* [k] -> [nlag][nexp][nseg][TRX_NMOMENT] */);

/* The Kp-Vsys detection map on the device, reduced from the trail: trx_run_trail followed, on the device, by the two
 * products an observer looks at -- the CCF trail per[lag][exposure], a statistic of every trail row added over the
 * segments (orders), and the map[Kp][Vsys], per interpolated along each cell's velocity track and added over the
 * exposures.  Only the map ([nkp][nvsys] doubles) and, when asked for, per ([nlag][nexp]) are copied back; the
 * [nlag][nexp][nseg][TRX_NMOMENT] trail stays in device memory.
 *
 * A trx_vmap is {stat, nlag, p0, p1, lag, lag_kms, nkp, nvsys, kp, vsys, orbit, offset}: lag[l] the lags as trx_run_trail
 * takes them, lag_kms[l] their velocities (km/s, strictly increasing), kp[i] and vsys[j] the map's axes (km/s),
 * orbit[v] what multiplies Kp at exposure v (sin(2 pi phase_v) for a circular orbit), offset[v] a velocity added at
 * exposure v (the barycentric correction) or NULL.  nexp and nseg are the installed observed set's.  Every operation
 * below is IEEE double, rounded once, no fused multiply-add; +, -, *, / and sqrt are correctly rounded on the device, so
 * only log can differ from a host evaluation of the same lines.
 *
 * 1. The statistic of a row, stat(m) of its moments m0 .. m6 (n, sum w, sum w g, sum w g^2, sum w f, sum w f g, sum w f^2):
 *      <f> = m4 / m1     <g> = m2 / m1
 *      sf2 = m6 / m1 - <f> * <f>      sg2 = m3 / m1 - <g> * <g>      R = m5 / m1 - <f> * <g>
 *      TRX_STAT_CCF           R / sqrt(sf2 * sg2)
 *      TRX_STAT_LOGLIKE_BL19  (-0.5 * n) * log(arg),  arg = sf2 - (2 * p0) * R + (p0 * p0) * sg2        (p0: the scale)
 *      TRX_STAT_CHI2          m6 - (2 p0) m5 - (2 p1) m4 + (p0 p0) m3 + ((2 p0) p1) m2 + (p1 p1) m1, added left to right
 *                             (sum w (f - p0 g - p1)^2)
 *    The first two are undefined (NaN) for n < 2, for sf2 <= 0 or sg2 <= 0 (or not a number), BL19 also for arg <= 0.
 * 2. per[l][v] = the sum of stat(trail[l][v][s]) over s = 0 .. nseg-1 IN THAT ORDER, one addition each, from +0;
 *    undefined rows are skipped (all skipped: +0).
 * 3. Cell (i, j): for v = 0 .. nexp-1 in that order, x_v = (kp[i] * orbit[v] + vsys[j]) + offset[v] (the last addition
 *    only with an offset),
 *      k = clip(upper_bound(lag_kms, x_v) - 1, 0, nlag - 2)       (upper_bound: the number of lag_kms <= x_v)
 *      t = (x_v - lag_kms[k]) / (lag_kms[k+1] - lag_kms[k])       (x_v == lag_kms[nlag-1]: k = nlag - 2, t = 1)
 *      map[i][j] += per[k][v] + t * (per[k+1][v] - per[k][v])     (nlag == 1: += per[0][v])
 *    from +0.  A cell with any x_v outside [lag_kms[0], lag_kms[nlag-1]], or not finite, is NaN.
 * It follows that
 *   - there are no atomics: per[l][v] depends on the trail rows (l, v, .) only, a cell on its kp, its vsys, orbit,
 *     offset, lag_kms and per -- not on the other cells of the call, the launch, the batch way or the depth hint;
 *   - map is, bit for bit, steps 3 applied on the host to the per the same call returned;
 *   - per is steps 1-2 applied on the host to the trail trx_run_trail returns, bit for bit for CCF and CHI2 and to the
 *     accuracy of log for LOGLIKE_BL19 (the device's within 3 ulp).
 *
 * Everything else is trx_run_trail's: a broadening applies, a filter is ignored, spectrum may be NULL and when given
 * holds the bits trx_run gives, the device's trail buffer holds afterwards what trx_run_trail would have left there,
 * and every other run on the handle is unchanged, bit for bit.  per may be NULL.
 * TRX_E_ARG, the reason in trx_last_error, with nothing touched and the handle usable: every refusal of trx_run_trail
 * (no observed set, nlag < 1, lag NULL, a lag that is not finite and > 0, the two products above their limits); vm or
 * map NULL; an unknown stat; nkp < 1 or nvsys < 1; nkp * nvsys above 2^31 - 1; lag_kms, kp, vsys or orbit NULL; a
 * non-finite p0 or p1; a non-finite kp, vsys, orbit or offset (naming e.g. "orbit N"); a lag_kms that is not finite and
 * strictly increasing ("lag_kms N").  TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid.
 * trx_run_batch_velocity_map is trx_run_batch with ONE vm for all atmospheres, atmosphere j's map in map[j] and, with
 * per not NULL, its statistic in per[j]; it also refuses a NULL map[j] or per[j].  The batch's broadenings apply as in
 * trx_run_batch_trail. */
#define TRX_STAT_CCF 1          /* the weighted Pearson coefficient                  */
#define TRX_STAT_LOGLIKE_BL19 2 /* Brogi & Line (2019) log-likelihood, p0 = scale    */
#define TRX_STAT_CHI2 3         /* chi-square of f against p0 g + p1                 */
typedef struct {
  int32_t stat, nlag;
  double  p0, p1;
  const double *lag;      /* [nlag] nu_observed / nu_rest, as trx_run_trail takes them       */
  const double *lag_kms;  /* [nlag] the lags' velocities, strictly increasing                */
  int32_t nkp, nvsys;
  const double *kp;       /* [nkp]   km/s                                                     */
  const double *vsys;     /* [nvsys] km/s                                                     */
  const double *orbit;    /* [nexp]  what multiplies Kp at exposure v, e.g. sin(2 pi phase_v) */
  const double *offset;   /* [nexp]  km/s added at exposure v (barycentric), or NULL: none    */
} trx_vmap;
int  trx_run_velocity_map(trx_handle *h, const trx_atm *a, const trx_opts *o,
                          double *spectrum /* [wn_hi-wn_lo], host; may be NULL */, const trx_vmap *vm,
                          double *map /* [nkp][nvsys], host */, double *per /* [nlag][nexp], host; may be NULL */,
                          trx_debug *dbg /* may be NULL */);
int  trx_run_batch_velocity_map(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                                const trx_vmap *vm /* one for all */, double *const *map /* [k] -> [nkp][nvsys] */,
                                double *const *per /* NULL, or [k] -> [nlag][nexp] */);

/* The high-pass of the model pixels along each order, on the device, between the pixels and everything that reads them.
 * Observed exposures are continuum-normalised before they are compared with a model: per spectral order a smooth
 * function along the PIXEL axis -- in practice a running Gaussian or boxcar mean -- is taken out, and the model has to
 * go through the same high-pass, or its broadband slope biases every statistic (the moments remove a weighted mean per
 * order only).  With it installed the chain spectrum -> broadening -> pixels -> high-pass -> filter -> moments / trail /
 * map stays on the device.
 *
 * A high-pass belongs to the observed set it is installed over; the segments are that set's.  It is a symmetric tap
 * table taps[0 .. half]: every tap finite and >= 0, taps[0] > 0, taps[k] the weight at a distance of k pixels,
 * 0 <= half <= TRX_HIGHPASS_MAX_HALF.  For a row r (a shift, or a lag of a trail), segment s = [first, last) and pixel
 * p in it, with (a, b) the pair trx_run_pixels gives for that row and pixel:
 *   live_q = b[r][q] > 0
 *   g_q    = gain_q * (a[r][q] / b[r][q])            (gain 1 without a gain array)
 *   num_p  = sum of taps[|k|] * g_{p+k}
 *   den_p  = sum of taps[|k|]
 *   g'_p   = g_p - num_p / den_p
 *   - both sums run over k = -half .. +half IN THAT ORDER and start from +0; a term whose q = p + k lies outside
 *     [first, last) or is not live is skipped;
 *   - every product, sum, the division and the subtraction are rounded once (no fused multiply-add);
 *   - a pixel that is not live is DEAD: quiet NaN in values, and nothing downstream counts it;
 *   - a non-finite g propagates as IEEE arithmetic gives; den_p >= taps[0] > 0 for a live p;
 *   - half = 0 gives g' = g - (t g) / t: +0 at every live pixel when taps[0] is a power of two (1 in a Gaussian or a
 *     boxcar table), for which the product and the quotient are exact.
 * Only + - * / and no atomics: the bits of a value depend on its row's pairs over its window, the gains and the taps --
 * not on other rows or segments, the launch, the batch way that ran it or the handle's depth hint.
 *
 * trx_set_highpass copies the taps (hp NULL or hp->taps NULL: clear it).  It returns TRX_E_ARG, the reason in
 * trx_last_error, with no observed set installed, half < 0 or above TRX_HIGHPASS_MAX_HALF, a non-finite or negative
 * tap (naming "tap N"), taps[0] not above 0; a refused one leaves the previous high-pass in force.  A successful
 * trx_set_observed (a clearing one included) or trx_set_pixels drops it, as they drop the filter; it is independent of
 * the broadening and of the filter.
 * trx_run_highpassed is trx_run_pixels plus the high-pass, for any nshift >= 1 (rows are independent): spectrum may be
 * NULL, and when it is given it holds the bits trx_run gives; values[r][p] = g'_p of row r, NaN where dead.  TRX_E_ARG
 * with no observed set or no high-pass installed, nshift < 1, shift or values NULL, a non-finite or <= 0 shift (naming
 * "shift N"), nshift * npix above what one pixel launch takes; TRX_E_UNSUPPORTED on a handle whose shard is not the
 * whole grid, for trx_run_moments' reason.  A run that fails leaves values undefined.
 * WITH A HIGH-PASS INSTALLED trx_run_moments, trx_run_filtered_moments, trx_run_trail and trx_run_velocity_map (and
 * their batch forms) take g' where they took g and skip the dead pixels: the same kernels, the same order of every sum,
 * so trail[l] stays bit for bit trx_run_moments with all shifts equal to lag[l] on the same handle (on a handle without
 * an exposure table).  trx_run,
 * trx_run_bands, trx_run_contrib, trx_run_pixels, trx_run_broadened and trx_sweep_permol are unchanged bit for bit, as
 * is every run on a handle without a high-pass.
 * trx_batch_set_highpass installs the same high-pass on every handle of the batch, or on none (its reason through
 * trx_last_error(NULL)). */
#define TRX_HIGHPASS_MAX_HALF 1024
typedef struct {
  int32_t half, pad;         /* taps[0 .. half]; pad is ignored                                              */
  const double *taps;        /* [half + 1] finite, >= 0, taps[0] > 0                                         */
} trx_highpass;
int  trx_set_highpass(trx_handle *h, const trx_highpass *hp);
int  trx_run_highpassed(trx_handle *h, const trx_atm *a, const trx_opts *o,
                        double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                        int32_t nshift, const double *shift /* [nshift] */,
                        double *values /* [nshift][npix], host; NaN = dead */, trx_debug *dbg /* may be NULL */);
int  trx_batch_set_highpass(trx_batch *b, const trx_highpass *hp);

/* The Kp-Vsys detection map with the detrending filter applied to every cell's own model matrix, from one spectrum.
 * trx_run_trail and trx_run_velocity_map ignore an installed filter, because a trail's model is the same at all
 * exposures; in a map cell it is not -- at exposure v it sits at the cell's own velocity kp * orbit[v] + vsys -- and the
 * reprocessed model M' = M - U (U^+ M) (Brogi & Line 2019; Gibson et al. 2022) differs from cell to cell.  This call
 * does for every cell what trx_run_filtered_moments does for one velocity hypothesis, from ONE spectrum and ONE pixel
 * pass at the lags; only the map ([nkp][nvsys] doubles) and, when asked for, the lag table are copied back.
 *
 * vm is the trx_vmap of trx_run_velocity_map; nexp, nseg, the data, weights and gains are the installed observed set's,
 * the matrices the installed filter's.  Every operation below is IEEE double, rounded once, no fused multiply-add.
 *
 * 1. The rows.  G[l][p] is the pair trx_run_pixels gives for the shift vm->lag[l] and pixel p.  With a broadening
 *    installed the pairs sample the broadened spectrum; with a high-pass installed G[l][p] is that row's high-passed
 *    pair (g', 1) / (0, 0), as every observed run takes it.  This is one pixel pass of nlag rows, exactly the one
 *    trx_run_trail makes; the trail kernel does not run, and the device's trail buffer is not written.
 * 2. The track of a cell.  For cell (i, j) and exposure v, x_v = (kp[i] * orbit[v] + vsys[j]) + offset[v] (the last
 *    addition only with an offset), and with k and t of x_v as in step 3 of trx_run_velocity_map the cell takes the
 *    NEAREST lag, not an interpolation:
 *      k_v = k + (t > 0.5 ? 1 : 0)            (a tie goes to the lower lag; nlag == 1: k_v = 0)
 *    lag_index[i][j][v] = k_v.  If any x_v is outside [lag_kms[0], lag_kms[nlag-1]] or not finite, the whole cell is NaN
 *    in map, and its lag_index entries are -1 at the offending exposures and the nearest index elsewhere.  (Nearest, so
 *    that every cell is an existing product at shifts the caller can name, point 6; a driver makes it as fine as it wants
 *    with the lag step.)
 * 3. The cell's model matrix M[v][p] = G[k_v][p].  For each pixel column this is the filter of trx_set_filter unchanged:
 *    the column is LIVE when b > 0 at every one of the cell's rows k_v; c_j is taken over v ascending and r_v over j
 *    ascending, both from +0; g' = g - r_v; a DEAD column is NaN.  A column can be live in one cell and dead in another.
 * 4. The cell's moments.  For every (v, s) the seven sums of trx_run_filtered_moments over g' against exposure v's data
 *    and weights: the same terms, the same lane order (first + l, first + l + 64, ...), the same butterfly.
 * 5. The cell's value.  per_v = the sum over s = 0 .. nseg-1 IN THAT ORDER, from +0, of stat(mom[v][s]) (step 1 of
 *    trx_run_velocity_map), undefined rows skipped; map[i][j] = the sum over v = 0 .. nexp-1 IN THAT ORDER, from +0, of
 *    per_v.
 * 6. It follows that, for a cell inside the lag grid,
 *   - its moments are bit for bit what trx_run_filtered_moments returns on the same handle with shift[v] = lag[k_v]
 *     (on a handle without an exposure table: the map ignores one, trx_set_exposures; trx_run_exposed_map is the map
 *     that takes it);
 *   - map[i][j] is point 5 applied on the host to those moments, in the same bits for CCF and CHI2 and to the accuracy
 *     of the device's log (within 3 ulp) for LOGLIKE_BL19;
 *   - there are no atomics: a cell's bits do not depend on the other cells of the call, the chunk of cells it was
 *     computed in, the launch, the batch way or the handle's depth hint.
 *
 * spectrum may be NULL, and when it is given it holds the bits trx_run gives; lag_index may be NULL.  trx_run_trail,
 * trx_run_velocity_map and every other run on the handle are unchanged, bit for bit.  A run that fails leaves map and
 * lag_index undefined.
 * TRX_E_ARG, the reason in trx_last_error, with nothing touched and the handle usable: every refusal of
 * trx_run_velocity_map under this call's name; no filter installed; nkp * nvsys * nexp above 2^31 - 1.
 * TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid.
 * trx_run_batch_filtered_map is trx_run_batch with ONE vm for all atmospheres and atmosphere j's map in map[j]; it also
 * refuses a NULL map[j].  The batch's broadenings apply as in trx_run_batch_velocity_map. */
int  trx_run_filtered_map(trx_handle *h, const trx_atm *a, const trx_opts *o,
                          double *spectrum /* [wn_hi-wn_lo], host; may be NULL */, const trx_vmap *vm,
                          double *map /* [nkp][nvsys], host */,
                          int32_t *lag_index /* [nkp][nvsys][nexp], host; may be NULL */,
                          trx_debug *dbg /* may be NULL */);
int  trx_run_batch_filtered_map(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                                const trx_vmap *vm /* one for all */, double *const *map /* [k] -> [nkp][nvsys] */);

/* The exposure table on the device: the two parts of a time series' forward model that differ from exposure to exposure
 * and must act on the pixels BEFORE the filter, which mixes the exposures of a column.
 *   scale[v]  the model's amplitude at exposure v: the light curve in transit (0 out of transit), the phase function in
 *             emission.  (trx_observed.gain is per pixel only.)
 *   smear[v]  eta_v = dv / (2 c), the HALF-width of the change of the planet's Doppler factor over exposure v, relative:
 *             the lines are smeared by a box in velocity whose width differs from exposure to exposure.
 * The table belongs to the observed set: row v of the pixel matrix is exposure v.  For exposure v (shift s, eta = smear[v],
 * c = scale[v]) and pixel p, every operation IEEE double, rounded once, no fused multiply-add:
 *   eta == 0:  the pair is exactly the pair trx_run_pixels gives for (s, p): the same range, the same Gaussian weight, the
 *              same lane and wave order.
 *   eta > 0:   centre' = centre_p / s ; fwhm' = fwhm_p / s ; sigma = fwhm' / (2 sqrt(2 ln 2))       (as trx_run_pixels)
 *              d = centre' * eta                 the box's half-width in cm-1, first order in eta as the broadening is in beta
 *              r = cut * sigma + d
 *              i_lo = ceil((centre' - r - wn_i) / wn_d) ; i_hi = floor((centre' + r - wn_i) / wn_d), clipped to [0, nwn)
 *              and then to the shard, as trx_run_pixels clips (a NaN edge: no bin)
 *              q = sigma * sqrt(2)               (the host's double sqrt(2.0))
 *              x = nu_i - centre' ; W_i = erf((x + d) / q) - erf((x - d) / q)
 *              (a, b) = (sum of W_i S_i, sum of W_i)
 *              W is the box of half-width d convolved with the Gaussian, unnormalised: the value is a / b.  The order of
 *              the sums is trx_run_pixels' rule applied to THIS window's in-shard length: fewer than 192 bins, one lane,
 *              bins ascending; otherwise the wave, lane l adding bins l, l + 64, ..., then the fixed butterfly.
 *   scale:     a is replaced by c * a, one product; b is untouched, so the contributing, live and dead rules of the
 *              moments, the filter and the high-pass do not move.  c = 0 makes the model 0 at that exposure, not the pixel
 *              dead.  A pair with no bin in the shard is exactly (+0, +0), whatever c.
 * No atomics: the bits of a pair depend on the spectrum, its pixel, its shift, its own eta and c, and the shard -- not on
 * the rest of the table, the other rows, the launch, the batch way that ran it or the handle's depth hint.
 *
 * WHERE THE TABLE ACTS: in the runs whose rows are exposures.  trx_run_exposed returns these pairs; trx_run_moments and
 * trx_run_filtered_moments (and their batch forms) take them where they took the plain pairs, with the high-pass and the
 * filter behind them unchanged.  WHERE IT IS IGNORED: in trx_run_pixels, trx_run_highpassed, trx_run_trail,
 * trx_run_velocity_map and trx_run_filtered_map a row is a shift or a lag, not an exposure; their bits are the same with
 * and without a table on the handle, as the trail's are with and without a filter.  (The map whose rows are (lag, exposure)
 * pairs, and which therefore takes the table, is trx_run_exposed_map below.)  Every run on a handle without a table is
 * unchanged, bit for bit.
 *
 * trx_set_exposures keeps the two arrays on the host (no device work, no synchronisation: the table changes with every
 * likelihood call, as v sin i does); a run uploads them with its shifts, ahead of its kernels.  ex NULL or nexp == 0 clears
 * it.  A successful trx_set_observed or trx_set_pixels drops it, clearing calls included; a refused one keeps it.  It is
 * independent of the broadening, the filter and the high-pass.  TRX_E_ARG, the reason in trx_last_error, the previous table
 * in force and the handle usable: no observed set; nexp < 0 or not the observed set's; both arrays NULL; a non-finite
 * scale; a smear that is not finite, negative or above TRX_SMEAR_MAX (both naming "exposure N").
 * trx_run_exposed is trx_run_pixels with the table: spectrum may be NULL, and when it is given it holds the bits trx_run
 * gives.  TRX_E_ARG with no observed set or no table installed, nshift not the set's nexp, shift or out NULL, a non-finite
 * or <= 0 shift (naming "shift N").  It works on a handle whose shard is not the whole grid: the pairs are linear in the
 * bins, and the ranks add theirs in rank order.  (The moment runs stay TRX_E_UNSUPPORTED there.)
 * trx_batch_set_exposures follows trx_batch_set_broadening: ex[j] belongs to atmosphere j of the following batch exposed,
 * moment, filtered-moment and exposed-map runs; n = 1: one table for all; n = 0: clear.  All entries are checked before any is kept, and
 * the arrays are copied.  Such a run of k atmospheres with n != 1 and n != k returns TRX_E_ARG (n = 0: the moment runs go
 * without a table; trx_run_batch_exposed refuses). */
#define TRX_SMEAR_MAX 0.01
typedef struct {
  int32_t nexp, pad;         /* = the installed observed set's nexp; pad is ignored                          */
  const double *scale;       /* [nexp] finite factor on the model at exposure v, or NULL: 1                  */
  const double *smear;       /* [nexp] eta_v >= 0, finite, <= TRX_SMEAR_MAX, or NULL: 0                      */
} trx_exposures;             /* 24 bytes */
int  trx_set_exposures(trx_handle *h, const trx_exposures *ex);
int  trx_run_exposed(trx_handle *h, const trx_atm *a, const trx_opts *o,
                     double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                     int32_t nshift, const double *shift /* [nshift], nshift = nexp */,
                     double *out /* [nexp][npix][2], host */, trx_debug *dbg /* may be NULL */);
int  trx_batch_set_exposures(trx_batch *b, int32_t n, const trx_exposures *ex /* [n] */);
int  trx_run_batch_exposed(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                           int32_t nshift, const double *const *shift /* [k] -> [nexp] */,
                           double *const *out /* [k] -> [nexp][npix][2] */);

/* The detrended Kp-Vsys map UNDER THE EXPOSURE TABLE, from one spectrum: trx_run_filtered_map with the model of exposure v
 * scaled by scale[v] and smeared by smear[v] BEFORE the filter, which mixes the exposures of a column.  This is the map for
 * a transit series with out-of-transit frames (scale[v] = 0 there) and for planets whose lines smear by several km/s per
 * exposure; trx_run_filtered_map ignores the table because its pixel rows are lags, and a lag has no exposure.  Here a pixel
 * row is a PAIR (lag, exposure), and the pixel pass makes exactly the pairs the call's cells need.
 *
 * vm is the trx_vmap of trx_run_velocity_map; nexp, nseg, the data, weights and gains are the installed observed set's, the
 * filter (of either kind) and the table the installed ones.  Every operation is IEEE double, rounded once, no fused
 * multiply-add.
 *
 * 1. The tracks.  Step 2 of trx_run_filtered_map, unchanged: x_v, the nearest lag k_v, lag_index[i][j][v] = k_v.  A cell with
 *    any x_v outside the lag grid or not finite is OUTSIDE: NaN in map, -1 in lag_index at the offending exposures.
 * 2. The row spans.  Over the cells that are not outside, for every exposure v: lo_v = min k_v, hi_v = max k_v,
 *    n_v = hi_v - lo_v + 1 (n_v = 0 when no cell is inside); base_v = n_0 + ... + n_{v-1}; R = the sum of the n_v, returned in
 *    *nrows.  Row r = base_v + (l - lo_v) is the pair (lag l, exposure v).  The spans are dense on purpose -- no compaction,
 *    integer min and max only --, so nothing depends on the order the cells are looked at in.
 * 3. The rows.  G[r][p] is exactly the pair trx_run_exposed gives on this handle for exposure v and pixel p when
 *    shift[v] = vm->lag[l]: ONE launch of the exposed pixel kernel over R rows with shift_r = lag[l], smear_r = smear[v],
 *    scale_r = scale[v]; an array the table leaves out (NULL) stays out.  With a broadening installed the rows sample the
 *    broadened spectrum; with a high-pass installed G[r] is that row's high-passed pair.
 * 4. The cell.  M[v][p] = G[base_v + k_v - lo_v][p]; then points 3 - 5 of trx_run_filtered_map word for word: the installed
 *    filter with its live and dead rule over the cell's own rows, the moments, the statistic added over the segments and
 *    then over the exposures.  The same kernels run, reading a row table where they read the lag table.
 * 5. It follows that, for a cell inside the lag grid,
 *   - its moments are bit for bit what trx_run_filtered_moments returns on the same handle, table installed, with
 *     shift[v] = lag[k_v];
 *   - map[i][j] is point 5 of trx_run_filtered_map applied on the host to those moments: the same bits for CCF and CHI2, the
 *     accuracy of the device's log (within 3 ulp) for LOGLIKE_BL19;
 *   - with a table of scale all 1 and smear all 0 (or either NULL) map and lag_index are bit for bit trx_run_filtered_map's;
 *   - there are no atomics: a cell's bits do not depend on the other cells of the call, the spans, the row numbers, the
 *     chunk, the launch, the batch way or the handle's depth hint.
 * 6. It leaves no trace: the handle's table, what its buffers mean to later calls, the trail buffer and every other entry
 *    point are unchanged, bit for bit; trx_run_filtered_map, trx_run_trail and trx_run_velocity_map keep ignoring the table.
 * 7. R = 0 (every cell outside): no pixel, filter or moment kernel runs, map is all NaN, and spectrum, when given, still
 *    holds trx_run's bits.
 *
 * spectrum, lag_index and nrows may be NULL.  A run that fails leaves map, lag_index and *nrows undefined.
 * TRX_E_ARG, the reason in trx_last_error, no output touched and the handle usable: every refusal of trx_run_filtered_map
 * under this call's name; no exposure table installed; R * npix above what one pixel launch takes; R * npix * 16 bytes of
 * pairs above 2^33 (kExposedMapPairBytes -- with a high-pass a second buffer of that size stands beside the first; a design
 * limit, not a measurement: a driver above it splits the orders or coarsens the lags), naming R and the bytes.
 * TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid.
 * trx_run_batch_exposed_map is trx_run_batch_filtered_map with the batch's tables as trx_run_batch_exposed takes them: one
 * for all atmospheres or one each (n != 1 and n != k: TRX_E_ARG), none installed: TRX_E_ARG; a NULL map[j] is refused. */
int  trx_run_exposed_map(trx_handle *h, const trx_atm *a, const trx_opts *o,
                         double *spectrum /* [wn_hi-wn_lo], host; may be NULL */, const trx_vmap *vm,
                         double *map /* [nkp][nvsys], host */,
                         int32_t *lag_index /* [nkp][nvsys][nexp], host; may be NULL */,
                         int64_t *nrows /* R; may be NULL */, trx_debug *dbg /* may be NULL */);
int  trx_run_batch_exposed_map(trx_batch *b, int32_t k, const trx_atm *atm /* [k] */, const trx_opts *o,
                               const trx_vmap *vm /* one for all */, double *const *map /* [k] -> [nkp][nvsys] */);

/* Detrending the observed exposures THEMSELVES on the device, with model injection: the step of an injection-recovery
 * test that ran on the host.  One call multiplies a model into the raw exposures (optional), runs SYSREM (Tamuz, Mazeh &
 * Zucker 2005) on them per segment, leaves the residuals installed as the observed set's data and the weighted filter of
 * the fitted time vectors in the filter slot.  trx_run_filtered_moments, trx_run_filtered_map and trx_run_exposed_map
 * after it are the recovery, unchanged.
 *
 * Every operation is IEEE double rounded once, no fused multiply-add; sums start from +0 and run in the order written.
 * F is the data as trx_set_observed installed them -- the RAW set, never the result of an earlier detrend call --, w the
 * set's weights (1 without), gain the set's gain.
 * 0. f0 = F.
 * 1. Injection (inject = 1).  (a, b)[v][p] is the pair trx_run_moments forms on this handle ahead of the high-pass for
 *    shift[v]: trx_run_exposed's with an exposure table installed, trx_run_pixels' without, behind the broadening where
 *    one is installed -- one spectrum and one pixel pass of the same kernels, the same bits.  Where b > 0:
 *      g = gain_p * (a / b);  m = p0 * g;  m = m + p1;  f0[v][p] = F[v][p] * m       (the "p0 g + p1" of TRX_STAT_CHI2)
 *    where b <= 0: f0[v][p] = F[v][p].  The high-pass and the filter take no part.  With inject = 0, a, o, shift and
 *    spectrum are not looked at and no spectrum is computed.
 * 2. SYSREM per segment s over its pixels [first, last), r = f0.  For component i = 0 .. ncomp-1: a_v = 1 for all v, then
 *    niter times
 *      column step, per pixel p:    num = sum over v ascending of (w[v][p] * r[v][p]) * a_v
 *                                   den = sum over v ascending of (w[v][p] * a_v) * a_v
 *                                   c_p = num / den if den > 0, else +0
 *      row step, per exposure v:    num = sum over p of (w * r) * c_p;   den = sum over p of (w * c_p) * c_p
 *                                   a_v = num / den if den > 0, else +0
 *    the row sums in the order of the moments: lane l of 64 adds the pixels first + l, first + l + 64, ... in that order,
 *    then the 64 lane sums go through the butterfly (every lane adds its partner lane ^ 32, 16, 8, 4, 2, 1).  Then the close:
 *      n2 = sum over v ascending of a_v * a_v;  t = sqrt(n2);  if t > 0: a_v = a_v / t and c_p = c_p * t
 *      U[s][v][i] = a_v;  coef[i][p] = c_p;  r[v][p] = r[v][p] - a_v * c_p
 *    An empty segment, or one masked everywhere, gives zero vectors.  The bits of a segment's result depend on that
 *    segment's f0 and w, ncomp and niter only -- not on other segments, the launch or the handle's depth hint; there are no
 *    atomics.  sqrt is the device's, correctly rounded.
 * 3. U is copied to the host; a non-finite entry is TRX_E_ARG ("component I of segment S is not finite") with nothing
 *    installed.  Otherwise, at once and only after every kernel has finished, the observed set's data become r and the
 *    filter slot takes the weighted filter of U through trx_set_weighted_filter's path (the same factor kernel and pivot
 *    rule, nsingular as there), replacing a filter of either kind.  The weights, gain, segments, high-pass, exposure table,
 *    broadening and pixel set stay installed.  basis, coef and data, where given, receive U, coef and r.
 * 4. From raw, always: the handle keeps F on the device -- the first call moves it aside, later calls read it --, so a call
 *    with the same arguments gives the same bits however many detrend calls came before.  dt NULL or ncomp = 0 is the UNDO:
 *    data <- F, the filter slot cleared, TRX_OK even if nothing had been detrended (nsingular, when given, 0).
 *    trx_set_observed and trx_set_pixels drop everything as they do for the set.
 * 5. TRX_E_ARG, the reason in trx_last_error, nothing touched -- data, filter and outputs as they were --, checked in this
 *    order: no observed set; ncomp < 0 or > TRX_FILTER_MAX; niter < 1 or > TRX_SYSREM_MAX_ITER; inject not 0 or 1;
 *    pad != 0; with inject = 1: a non-finite p0 or p1, a NULL a, o or shift, nshift != nexp, a bad shift ("shift N"),
 *    nexp * npix above what one pixel launch takes.  TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid.  The
 *    residuals are built in a buffer of their own and swapped in at step 3: a call that fails later (TRX_E_HIP,
 *    TRX_E_NOMEM) also leaves the previous data and filter in force.
 * Not here: a batch form (a driver takes basis and data from one handle and installs them on a trx_batch through
 * trx_batch_set_observed and trx_batch_set_weighted_filter), high-passing the data or division by a column's scatter,
 * shards.  The per-order normalisation ahead of the fit is step 1b, the recipe of trx_set_normalise (below): with one
 * installed f0 goes through it between steps 1 and 2; without one the call is what it was.  A principal-component analysis
 * in SYSREM's place is trx_pca_observed, below. */
#define TRX_SYSREM_MAX_ITER 64
typedef struct {
  int32_t ncomp, niter;      /* components 1 .. TRX_FILTER_MAX (0: undo); alternations per component, 1 .. TRX_SYSREM_MAX_ITER */
  int32_t inject, pad;       /* 0: detrend the raw data; 1: inject the model first; pad: 0 */
  double  p0, p1;            /* injected exposure: f0 = F * (p0 g + p1) */
} trx_detrend;               /* 32 bytes */
int  trx_detrend_observed(trx_handle *h, const trx_atm *a, const trx_opts *o,
                          double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                          int32_t nshift, const double *shift /* [nexp]; inject = 1 only */, const trx_detrend *dt,
                          double *basis /* [nseg][nexp][ncomp], host; may be NULL */,
                          double *coef /* [ncomp][npix], host; may be NULL */,
                          double *data /* [nexp][npix]: the residuals now installed, host; may be NULL */,
                          int64_t *nsingular /* may be NULL */, trx_debug *dbg /* may be NULL */);

/* The same call with a PRINCIPAL-COMPONENT ANALYSIS IN TIME in SYSREM's place (de Kok et al. 2013): per segment the leading
 * eigenvectors of the exposures x exposures Gram matrix of the data -- the left singular vectors of the exposures x pixels
 * matrix -- are fitted and removed.  The injection (steps 0 and 1), the outcome and the undo (steps 3 and 4) are
 * trx_detrend_observed's, through the same state: either call undoes either, and pca -> detrend or detrend -> pca gives
 * the second call the bits of a fresh one.  Every operation is IEEE double rounded once, no fused multiply-add; sums start
 * from +0 in the order written; there are no atomics.  Per segment s over its pixels [first, last), W the set's weights:
 * 2a. Exposure v is LIVE in s if W[v][p] > 0 for some p of the segment.  Column p is WHOLE if W[v][p] > 0 for every v live
 *     in s and at least one v is live; nwhole[s] counts them.  x[v][p] = f0[v][p] where p is whole and v live, +0 elsewhere.
 *     PCA has no definition under scattered masks (zero-filled entries where the data are ~ 1 would dominate the Gram
 *     matrix): whole-column and whole-exposure masks are exact, columns with holes take no part in the fit -- they still
 *     get coefficients and residuals in 2d.  SYSREM (trx_detrend_observed) is the tool for scattered masks.
 * 2b. G[v][u] = sum over p of x[v][p] * x[u][p] for u >= v, in the order of the moments: lane l of 64 adds the pixels
 *     first + l, first + l + 64, ... from +0, then the butterfly with partner lane ^ 32, 16, 8, 4, 2, 1.  G[u][v] = G[v][u].
 * 2c. Eigenvectors by cyclic Jacobi in a fixed parallel order, nsweep sweeps, no convergence test.  A = G, V = I, m = nexp
 *     rounded up to even.  A sweep is the rounds t = 0 .. m-2 of the circle tournament: round t has the pair (m-1, t) and, for
 *     k = 1 .. m/2-1, ((t+k) mod (m-1), (t-k) mod (m-1)), each ordered p < q; pairs with q >= nexp are dropped.  Every
 *     rotation of a round takes its parameters from A as the round finds it.  apq = A[p][q]; apq == 0: the pair is skipped,
 *     nothing of A or V rewritten; otherwise
 *       theta = (A[q][q] - A[p][p]) / (2.0 * apq);  t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0))
 *       c = 1.0 / sqrt(t * t + 1.0);  s = t * c
 *     Column phase, every row i, both old values read first: A[i][p] <- c A[i][p] - s A[i][q], A[i][q] <- s A[i][p] + c A[i][q],
 *     the same for V.  Then the row phase, every column j: A[p][j] <- c A[p][j] - s A[q][j], A[q][j] <- s A[p][j] + c A[q][j];
 *     then A[p][q] = A[q][p] = +0.  Each product is rounded, then the sum or difference.  After the last sweep lambda_j =
 *     A[j][j], offdiag[s] = max over p < q of |A[p][q]|; the j are ranked by descending lambda, ties by ascending j, a lambda
 *     that is not > 0 and finite (NaN and +-inf included) ranking as 0; component
 *     i is the column of V of rank i if its lambda is > 0 and finite, the zero vector otherwise; the entry of largest
 *     magnitude, the first on ties, is made positive by negating the column (0 - x: a zero entry stays +0).  U[s][v][i] is that column, eigen[s][i] its
 *     lambda (+0 for a zero vector).  An empty segment, or one without a whole column, has G = 0: every vector is zero (singular
 *     pivots of the filter, counted by nsingular).
 * 2d. Every column, the ones with holes included: coef[i][p] = sum over v ascending of U[s][v][i] * y[v][p], y = f0 where
 *     W > 0, +0 elsewhere; r = f0, then for i ascending r[v][p] = r[v][p] - U[s][v][i] * coef[i][p].
 * The Gram route squares the condition number: components whose singular value is below about 1e-8 of the largest are
 * noise -- far below anything a detrend of <= TRX_FILTER_MAX components asks for.  offdiag against eigen[s][0] tells how
 * far nsweep sweeps have converged: nothing is left after 8 sweeps at a dozen exposures; at 100 exposures 8 sweeps leave up to
 * 3e-11 of eigen[s][0] where G's spectrum is crowded (fewer whole columns than exposures, or many close noise eigenvalues), 10
 * to 12 sweeps reach rounding level; the leading components are converged long before.
 * TRX_E_ARG, the reason in trx_last_error, nothing touched, checked in this order: no observed set; nexp above
 * TRX_PCA_MAX_EXP; ncomp < 0, above TRX_FILTER_MAX or above nexp; nsweep < 1 or above TRX_PCA_MAX_SWEEP; then inject, pad and
 * the injection's arguments as trx_detrend_observed has them.  TRX_E_UNSUPPORTED on a shard.  A later TRX_E_HIP or
 * TRX_E_NOMEM leaves the previous data and filter in force.  pc NULL or ncomp = 0 is trx_detrend_observed's undo.
 * Not here: a batch form, shards, standardising the columns ahead of the PCA (trx_weigh_observed and the filter carry
 * that), a sweep count driven by convergence, more than TRX_PCA_MAX_EXP exposures.  Centring the columns ahead of the PCA
 * is step 1b, the recipe of trx_set_normalise (below), as in trx_detrend_observed. */
#define TRX_PCA_MAX_SWEEP 32
#define TRX_PCA_MAX_EXP   128
typedef struct {
  int32_t ncomp, nsweep;     /* components 1 .. min(TRX_FILTER_MAX, nexp) (0: undo); Jacobi sweeps 1 .. TRX_PCA_MAX_SWEEP */
  int32_t inject, pad;       /* as trx_detrend */
  double  p0, p1;
} trx_pca;                   /* 32 bytes */
int  trx_pca_observed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum /* as trx_detrend_observed */,
                      int32_t nshift, const double *shift, const trx_pca *pc,
                      double *basis /* [nseg][nexp][ncomp] */, double *coef /* [ncomp][npix] */,
                      double *data /* [nexp][npix]: the residuals now installed */, double *eigen /* [nseg][ncomp] */,
                      double *offdiag /* [nseg] */, int64_t *nwhole /* [nseg] */,
                      int64_t *nsingular, trx_debug *dbg);      /* every output may be NULL */

/* The same call with a REGRESSION ON GIVEN TIME VECTORS in SYSREM's place: every pixel column is fitted by weighted least
 * squares with vectors the caller already has -- 1, airmass and airmass^2 (Brogi et al. 2012), a basis frozen from an
 * earlier trx_detrend_observed or another night, the vectors of a telluric-rich order for all orders --, optionally
 * followed by a few SYSREM components on what is left.  It is trx_set_weighted_filter's projector applied to the data:
 * one factor serves the data here and the model in every run after it, so the data went through exactly the operation
 * the model goes through.  The injection (steps 0, 1 and 1b), the outcome and the undo (steps 3 and 4) are
 * trx_detrend_observed's, through the same state.  Every operation is IEEE double rounded once, no fused multiply-add;
 * sums start from +0 in the order written; there are no atomics.  W is the weights as trx_set_observed installed them
 * (1 without), NEVER a weigh call's result.  Per segment s, U = vectors[s] ([nexp][nvec]), per pixel column p of it,
 * w[v] = W[v][p]:
 * 2a. The factor: the normal matrix N = U^T diag(w) U, its L D L^T factor and the pivot rule exactly as
 *     trx_set_weighted_filter defines them (the same kernel, TRX_WFILTER_PIVOT).  nsingular_fit counts the columns with a
 *     singular pivot: a column live at fewer than nvec exposures or masked everywhere, a segment whose vectors are
 *     linearly dependent.
 * 2b. The fit, for a column with no singular pivot:
 *       y_j = sum over v ascending of (U[v][j] * w[v]) * f0[v][p]
 *       c = that definition's forward and back solve of y;  coef[j][p] = c_j
 *       r[v][p] = f0[v][p] - (sum over j ascending of U[v][j] * c_j)          every v, dead entries included
 *     For a column with a singular pivot c_j = +0 for every j, the solve's result is not used and r = f0, as SYSREM's
 *     den = 0 has it.  The bits of a column depend on its own f0 and w and on its segment's vectors and nvec only.
 * 2c. nfit > 0: SYSREM of nfit components and niter alternations on r, step 2 of trx_detrend_observed unchanged, giving
 *     U_fit[s][v][i] and coef[nvec + i][p].
 * 3.  trx_detrend_observed's outcome with the merged basis B[s][v] = (vectors[s][v][0 .. nvec), U_fit[s][v][0 .. nfit)):
 *     at once and only after every kernel has finished r becomes the observed data, the filter slot takes the weighted
 *     filter of B through trx_set_weighted_filter's path against W (nsingular as there; with nfit = 0 the factor of 2a IS
 *     the filter's, made once), the set's weights go back in force and a high-pass over the data is discarded.  basis,
 *     coef and data, where given, receive B, coef and r.
 * 4.  rg NULL or nvec = 0 is trx_detrend_observed's undo (nsingular_fit and nsingular, when given, 0).  Any of
 *     trx_detrend_observed, trx_pca_observed, trx_normalise_observed and this call undoes any other, and every call starts
 *     from F.
 * TRX_E_ARG, the reason in trx_last_error, nothing touched, checked in this order: no observed set; nvec < 0 or above
 * TRX_FILTER_MAX; nfit < 0; nvec + nfit above TRX_FILTER_MAX; with nfit > 0 niter < 1 or above TRX_SYSREM_MAX_ITER; a NULL
 * vectors; a non-finite entry of it (naming "segment S"); then inject and the injection's arguments as
 * trx_detrend_observed has them.  TRX_E_UNSUPPORTED on a shard.  A later TRX_E_HIP or TRX_E_NOMEM leaves the data, the
 * weights and the filter in force as they were.
 * Not here: a batch form, shards, a fit in log flux, vectors that differ from column to column. */
typedef struct {
  int32_t nvec, nfit;        /* given vectors 1 .. TRX_FILTER_MAX (0: undo); SYSREM components fitted after them, >= 0 */
  int32_t niter, inject;     /* alternations per fitted component (read only if nfit > 0); as trx_detrend            */
  double  p0, p1;            /* as trx_detrend */
  const double *vectors;     /* [nseg][nexp][nvec], finite: trx_wfilter's basis layout */
} trx_regress;               /* 40 bytes */
int  trx_regress_observed(trx_handle *h, const trx_atm *a, const trx_opts *o, double *spectrum /* as trx_detrend_observed */,
                          int32_t nshift, const double *shift, const trx_regress *rg,
                          double *basis /* [nseg][nexp][nvec+nfit] */, double *coef /* [nvec+nfit][npix] */,
                          double *data /* [nexp][npix]: the residuals now installed */,
                          int64_t *nsingular_fit, int64_t *nsingular, trx_debug *dbg);      /* every output may be NULL */

/* Weighing the observed set by the scatter of its pixel columns, on the device: the step of a detection pipeline between
 * SYSREM and the map.  One call reads the data the handle holds, forms every column's variance in time and every
 * segment's median variance, masks the columns whose variance stands out of their segment's, writes the new weights and
 * factorises the installed weighted filter again against them.  The data are not divided: the weights carry the step.
 *
 * Every operation is IEEE double rounded once, no fused multiply-add; sums start from +0 and run in the order written.
 * r is the data currently installed -- the residuals after trx_detrend_observed, the raw set otherwise --, W the weights
 * as trx_set_observed installed them (1 everywhere without) -- NEVER the result of an earlier weigh call.
 * 1. Column pass, per pixel p, v ascending over the entries with W[v][p] > 0:  n their count;  s = sum of r;
 *    mean = s / (double)n;  q = sum of d * d with d = r - mean (a second pass, the same order);  var_p = q / (double)(n - 1).
 *    The column is LIVE if n >= min_live, var_p > 0 and var_p is finite; otherwise var_p = +0.
 * 2. Segment median, per segment over its m live columns: med_s is the lower median of their var, the value of rank
 *    (m - 1) / 2 in ascending var, ties by ascending p; m = 0: med_s = +0.  (Found by counting -- exact, order-free, no
 *    atomics.)
 * 3. Keep rule:  lim = clip * clip;  lim = lim * med_s;  p is KEPT if it is live and (clip == 0 or var_p <= lim).
 *    nmasked is the number of live columns the clip removed.
 * 4. New weights:  TRX_SCATTER_VARIANCE: w'[v][p] = 1.0 / var_p (divided once per column) where W[v][p] > 0 and p is kept,
 *    +0 elsewhere;  TRX_SCATTER_MASK: w'[v][p] = W[v][p] where p is kept, +0 elsewhere.
 * 5. At once and only after every kernel has finished, w' -- built in a buffer of its own -- becomes the observed set's
 *    weights; the handle keeps W aside on the device.  If the filter slot holds a WEIGHTED filter, its factor and pivot
 *    flags are made again from its own basis against w' (trx_set_weighted_filter's kernel and pivot rule; nsingular as
 *    there, 0 without a weighted filter) in new buffers and swapped in with the weights.  A plain filter, the high-pass,
 *    exposure table, broadening, gain, data and pixel set stay as they are.  variance, median and weight, where given,
 *    receive var, med and w'.
 * 6. The undo, and "from raw": sc NULL or kind = TRX_SCATTER_NONE puts W back in force and factorises the weighted filter
 *    again against it; TRX_OK even if nothing had been weighed; nmasked 0, and variance, median and weight are not written.
 *    trx_detrend_observed's SYSREM and filter factor always read W, and a successful detrend call (its undo included)
 *    leaves W as the weights in force -- a failed one the weights as they were --: detrend, weigh, detrend gives the second
 *    detrend the bits of a fresh one.  trx_set_weighted_filter after a weigh factorises against the weights in force.
 *    trx_set_observed and trx_set_pixels drop everything.
 * 7. TRX_E_ARG, the reason in trx_last_error, nothing touched, checked in this order: no observed set; kind outside 0 .. 2;
 *    min_live < 2 or above nexp; clip non-finite, negative or in (0, 1) (a non-NULL sc is checked whole, whatever its
 *    kind).  TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid.  A call that fails later (TRX_E_HIP,
 *    TRX_E_NOMEM) leaves the previous weights and filter in force.
 * Not here: a batch form, shards, dividing the data.  Sigma-clipping single entries is trx_set_normalise's clip (below). */
#define TRX_SCATTER_NONE     0   /* undo: the weights as trx_set_observed installed them */
#define TRX_SCATTER_VARIANCE 1   /* w' = 1 / var_p on the kept columns' live entries      */
#define TRX_SCATTER_MASK     2   /* w' = W on the kept columns, 0 on the others           */
typedef struct { int32_t kind, min_live; double clip; } trx_scatter;      /* 16 bytes */
int  trx_weigh_observed(trx_handle *h, const trx_scatter *sc,
                        double *variance /* [npix], host; may be NULL */, double *median /* [nseg], host; may be NULL */,
                        double *weight /* [nexp][npix], host; may be NULL */,
                        int64_t *nmasked /* may be NULL */, int64_t *nsingular /* may be NULL */);

/* High-passing the observed set itself along the pixel axis, on the device: the data-side twin of trx_set_highpass.  The
 * model of a run against the observed set goes through the installed high-pass; SYSREM's residuals (or the raw set) go
 * through the SAME table with this call, so the two are compared like with like.  The documented order is
 * trx_detrend_observed, trx_highpass_observed, trx_weigh_observed, the map.
 *
 * Every operation is IEEE double rounded once, no fused multiply-add; sums start from +0; no atomics.
 * W is the weights as trx_set_observed installed them (1 everywhere without) -- the array trx_detrend_observed reads, NEVER
 * a weigh call's result.  r is the data as the last successful trx_detrend_observed left them -- its residuals, or the raw
 * set if the set is not detrended --, NEVER an earlier high-pass call's result: calling twice gives the bits of calling once.
 * taps[0 .. half] is the high-pass installed on the handle.
 * 1. An entry (v, q) is LIVE if W[v][q] > 0.  For a row v, a segment [first, last) and a live pixel p in it
 *      r'[v][p] = r[v][p] - (sum of taps[|k|] * r[v][p+k]) / (sum of taps[|k|]),   k = -half .. half in that order,
 *    over the q = p + k inside the segment and live: trx_set_highpass's formula with g = r and live = (W > 0).  A dead entry
 *    gets r' = +0 (after SYSREM it holds an unweighted junk residual); ndead is their count.
 * 2. At once and only after every kernel has finished, r' -- built in a buffer of its own -- becomes the observed set's
 *    data; r is kept aside on the device.  Nothing else changes: the weights in force, a filter of either kind and its
 *    factor, the high-pass, the exposure table, the broadening, the gain and the pixel set stay.  data, where given,
 *    receives r'.
 * 3. The undo: apply = 0 puts r back in force; TRX_OK even if nothing had been high-passed, and no high-pass need be
 *    installed; ndead 0, data not written.
 * 4. Every successful trx_detrend_observed, its undo included, discards the high-pass: detrend, high-pass, detrend gives the
 *    second detrend the bits of a fresh one.  trx_weigh_observed reads the data in force -- r' after this call --, and its
 *    undo does not touch the data; this call after a weigh neither reads nor changes the weights in force.
 *    trx_set_highpass afterwards, with a new table or NULL, leaves the data as they are.  trx_set_observed and
 *    trx_set_pixels drop everything.
 * 5. TRX_E_ARG, the reason in trx_last_error, nothing touched, checked in this order: no observed set; apply not 0 or 1;
 *    with apply = 1, no high-pass installed.  TRX_E_UNSUPPORTED on a handle whose shard is not the whole grid.  nexp * ntiles
 *    above one launch's grid is refused before anything is launched.  A call that fails later (TRX_E_HIP, TRX_E_NOMEM)
 *    leaves the previous data in force.
 * Not here: a batch form, shards, a high-pass ahead of SYSREM, a table other than the installed one.  Clipping single
 * entries is trx_set_normalise's clip (below), ahead of the fit. */
int  trx_highpass_observed(trx_handle *h, int32_t apply /* 1: high-pass, 0: undo */,
                           double *data /* [nexp][npix]: the data now installed, host; may be NULL */,
                           int64_t *ndead /* may be NULL */);

/* Normalising the observed set on the device, ahead of SYSREM and PCA: the first step of every published pipeline, and
 * STEP 1b of the detrending calls.  Each (exposure, segment) row is divided by its own continuum level -- a quantile of its
 * live data --, each pixel column is divided by, or has subtracted, its mean in time, and single outlying entries are
 * clipped.  The recipe sits in a slot on the handle (trx_set_normalise); with one installed trx_detrend_observed and
 * trx_pca_observed run it on f0 in the call's own buffer between the injection (step 1) and the fit (step 2), so that an
 * injection-recovery loop injects into the RAW data and normalises afterwards, as the pipeline under test does, without
 * the data leaving the device.  trx_normalise_observed is "the detrend of zero components": steps 0, 1 and 1b alone.  The
 * documented order is normalise, detrend, pca or regress, high-pass, weigh, the map.
 *
 * Every operation is IEEE double rounded once, no fused multiply-add; sums start from +0 in the order written; no atomics.
 * W is the weights as trx_set_observed installed them (1 without) -- never a weigh call's --; an entry is LIVE if W[v][p] > 0.
 * 1. Row scale, per exposure v and segment s.  m is the number of live pixels of the row.  row_kind QUANTILE:
 *      k = (int64) floor(quantile * (double)(m - 1));  scale[v][s] = the value of rank k (0-based, ascending) among the
 *    row's live f0 (an exact selection; ties are equal values; quantile 0.5 is the lower median).  The row is GOOD if m >= 1
 *    and scale > 0; otherwise scale = +0 (a scale of -0 included).  f1 = f0 / scale.  row_kind NONE: every row with a live
 *    pixel is good, scale = 1.0 and f1 = f0.
 * 2. Column centre, per pixel p, v ascending over the entries that are live in a good row: n their count, s the sum of f1,
 *    c_p = s / (double)n.  The column is GOOD if n >= 1 and -- DIVIDE and RATIO: c_p > 0 and finite; SUBTRACT: c_p finite;
 *    col_kind NONE: nothing more.  A column that is not good has c_p = +0.  f2 = f1 / c_p;  or t = f1 / c_p, t - 1.0;  or
 *    f1 - c_p;  or f1.
 * 3. Clip (clip > 0), per good column with n >= 2, one pass, not iterated, in trx_weigh_observed's arithmetic:
 *      mean = (sum of f2) / (double)n;  q = sum of d * d with d = f2 - mean;  var = q / (double)(n - 1);
 *      lim = clip * clip;  lim = lim * var;  an entry with d * d > lim becomes mean and counts in nclipped.
 * 4. Every entry that is dead, in a bad row or in a bad column gets +0; nbad counts the LIVE entries among them.
 * A segment's output bits depend only on that segment's f0 and W and on the recipe -- not on other segments, the launch or
 * the handle.
 *
 * trx_set_normalise installs the recipe (nm NULL: clears it): host work only, nothing in force changes -- data, weights and
 * filter stay --, the recipe acts from the next detrending call on.  trx_set_observed and trx_set_pixels drop it with
 * everything else.  TRX_E_ARG, nothing touched, checked in this order: no observed set; row_kind outside 0 .. 1; col_kind
 * outside 0 .. 3; quantile non-finite or outside [0, 1] (whatever row_kind is); clip non-finite, negative or in (0, 1);
 * both kinds NONE and clip == 0 (a recipe that does nothing: pass NULL).  TRX_E_UNSUPPORTED on a shard.
 *
 * trx_normalise_observed runs steps 0, 1 and 1b with trx_detrend_observed's injection and its checks; at once and only after
 * every kernel has finished the result -- built in the detrend's residual buffer -- becomes the observed data, the filter
 * slot is cleared, the weights of trx_set_observed go back in force and a high-pass over the data is discarded.  It goes
 * through the state of the other two calls: any of the three undoes any other, trx_detrend_observed with ncomp = 0 undoes
 * it, and every call starts from the raw F.  data, rowscale and centre, where given, receive the data now installed,
 * scale and c; nclipped and nbad the two counts.  A driver needs those once per data set: a row with rowscale == 0, or a
 * column that turned bad, is to be masked in the weights of trx_set_observed, and so is a column whose centre is low (a
 * deep telluric).  TRX_E_ARG, nothing touched, in this order: no observed set; no recipe installed; then inject and the
 * injection's arguments as trx_detrend_observed has them.  TRX_E_UNSUPPORTED on a shard.  A later TRX_E_HIP or
 * TRX_E_NOMEM leaves the data and the filter in force as they were.
 * Not here: a change of the WEIGHTS (the call masks nothing: the driver does, above), a batch form, shards, an iterated
 * clip, a polynomial continuum per row. */
#define TRX_NORM_ROW_NONE      0
#define TRX_NORM_ROW_QUANTILE  1   /* divide each (exposure, segment) row by its quantile */
#define TRX_NORM_COL_NONE      0
#define TRX_NORM_COL_DIVIDE    1   /* f / c_p        (about 1) */
#define TRX_NORM_COL_RATIO     2   /* f / c_p - 1.0  (about 0) */
#define TRX_NORM_COL_SUBTRACT  3   /* f - c_p        (about 0) */
typedef struct {
  int32_t row_kind, col_kind;
  double  quantile;      /* in [0, 1]; 0.5: the lower median */
  double  clip;          /* 0: none; otherwise >= 1: entries beyond clip sigma of their column are replaced */
} trx_normalise;         /* 24 bytes */
int  trx_set_normalise(trx_handle *h, const trx_normalise *nm /* NULL: clear */);
int  trx_normalise_observed(trx_handle *h, const trx_atm *a, const trx_opts *o,
                            double *spectrum /* [wn_hi-wn_lo], host; may be NULL */,
                            int32_t nshift, const double *shift /* [nexp]; inject = 1 only */,
                            int32_t inject, double p0, double p1,
                            double *data /* [nexp][npix]: the data now installed, host; may be NULL */,
                            double *rowscale /* [nexp][nseg], host; may be NULL */,
                            double *centre /* [npix], host; may be NULL */,
                            int64_t *nclipped /* may be NULL */, int64_t *nbad /* may be NULL */,
                            trx_debug *dbg /* may be NULL */);

/* The per-layer operator of the reference in its per-molecule form,
 *   computemolext(tr, kiso, temp, density, Z, permol = 1)   (extinction.c:282)
 * batched over nv independent thermodynamic states -- what calcopacity()
 * (opacity.c:387-403) loops over (layer x temperature) to fill an opacity grid.
 * iso_slot[i] = output row of isotope i (isotopes of one molecule share a row and
 * must be contiguous); out is [nv][nslot][wn_hi-wn_lo], extinction per unit
 * density (no density factor, extinction.c:472), thresholded per molecule. */
int  trx_sweep_permol(trx_handle *h, int32_t nv, const double *temp /* [nv] */,
                      const double *density /* [nmol][nv] */, const double *zpart /* [niso][nv] */,
                      double ethresh, int32_t nslot, const int32_t *iso_slot /* [niso] */, double *out);

int  trx_get_stats(const trx_handle *h, trx_stats *out);

/* Voigt table access for parity tests (reference struct opacity.profile /
 * .profsize, structures_tr.h:154-171). */
int  trx_table_info(const trx_handle *h, int64_t *profsize /* [ndop*nlor] */,
                    int64_t *offset /* [ndop*nlor] float offset of each profile */,
                    int64_t *total_floats);
int  trx_table_copy(const trx_handle *h, float *out /* [total_floats] */);
int  trx_width_grids(const trx_handle *h, double *adop /* [ndop] */, double *alor /* [nlor] */);

/* RCCL communicator for the wavenumber-sharded job (one process per GPU).
 * Rank 0 calls trx_comm_unique_id and ships the 128 bytes to the other ranks
 * by any channel (torch.distributed, MPI, a file); every rank then calls
 * trx_comm_create on its own device. */
#define TRX_COMM_ID_BYTES 128
int  trx_comm_unique_id(void *id_out /* TRX_COMM_ID_BYTES */);
int  trx_comm_create(const void *id, int nranks, int rank, int device, void **comm_out);
void trx_comm_destroy(void *comm);
/* Give a communicator up without the collective teardown (ncclCommAbort): for the error path of a
 * job in which some rank failed and the others must not wait for it. */
void trx_comm_abort(void *comm);

/* The one exchange of a wavenumber-sharded job ("one ncclAllGather of the
 * spectrum slices at the end"): every rank hands in `count` doubles in device memory (its slice,
 * padded to the same count on every rank) and receives all ranks' slices in rank order in d_all
 * (nranks * count doubles, device memory).  ncclAllGather on the handle's stream over the
 * communicator given in trx_static.comm; synchronised on return.  A handle without a
 * communicator (single rank) copies its slice.  Nothing else is exchanged between ranks: the
 * per-layer maximum line strength, the only global quantity of the path (extinction.c:399-427),
 * is computed by every rank from the same small set of candidate lines. */
int  trx_gather(trx_handle *h, const void *d_slice, void *d_all, int64_t count);
/* The same with host buffers on both sides (slice: count doubles; all: nranks * count). */
int  trx_gather_host(trx_handle *h, const double *slice, double *all, int64_t count);

const char *trx_strerror(int status);
const char *trx_last_error(const trx_handle *h);   /* detail of the last failure; h NULL: of this thread's last
                                                      trx_comm_create */

/* Messages.  The reference prints through tr_output(level, ...) filtered by the global
 * `verblevel` (transit.h:70-75, levels flags_tr.h:107-111) and exit()s on errors; the
 * library never prints or exits by itself: it hands the text to this process-wide callback
 * for levels <= max_level.  NULL = silent, except that the reason of a failed trx_create --
 * whose handle does not survive to be asked -- then goes to stderr.  Called on the thread
 * that made the API call. */
enum { TRX_LOG_ERROR = 1, TRX_LOG_WARN = 2, TRX_LOG_INFO = 3, TRX_LOG_RESULT = 4, TRX_LOG_DEBUG = 5 };
typedef void (*trx_log_fn)(int level, const char *message, void *user);
void trx_set_log(trx_log_fn fn, void *user, int max_level);

#ifdef __cplusplus
}
#endif
#endif /* TRANSIT_HIP_H */
