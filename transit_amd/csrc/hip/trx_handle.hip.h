// trx_handle.hip.h -- what a handle is: the buffers that own device and pinned memory, the sets a caller installs on a
// handle (bands, pixels, the observed set and what belongs to it), what a run is asked to make behind its spectrum, the
// test switches, trx_handle itself, and the helpers every stage goes through: the log, fail, HIPCHK, ensure*, upload*.
// Part of the one translation unit trx_api.hip, which includes it behind the kernel and host headers it rests on.
#pragma once

namespace {

struct DevBuf {
  void *p = nullptr; size_t bytes = 0;
  ~DevBuf() { release(); }
  void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
  template <class T> T *as() const { return (T *)p; }
};

// pinned host memory the device reads and writes in place (dev: its address there, asked for once per allocation, not per run)
struct PinnedBuf {
  void *p = nullptr, *dev = nullptr; size_t bytes = 0;
  ~PinnedBuf() { release(); }
  void release() { if (p) { (void)hipHostFree(p); p = dev = nullptr; bytes = 0; } }
};

// view into another allocation (same accessors as DevBuf, owns nothing)
struct DevView {
  void *p = nullptr;
  template <class T> T *as() const { return (T *)p; }
};

// a band set installed by trx_set_bands (trx_bands.hip.h), as this handle's shard sees it
struct BandSet {
  int32_t nbands = 0; int64_t npieces = 0;
  DevBuf d_bands, d_pieces, d_w, d_part;             // BandDev[nbands], BandPiece[npieces], WEIGHTS' in-shard weights, [npieces][2]
  PinnedBuf h_out;                                   // [nbands][2]: k_band_sums stores the run's sums here
};

// a pixel set installed by trx_set_pixels (trx_pixels.hip.h): the arrays as given -- ranges and weights are made on the device, per run
struct PixelSet {
  int64_t npix = 0; double cut = 0;
  DevBuf d_centre, d_fwhm;                           // [npix] each
};
// an observed set installed by trx_set_observed over the pixel set (trx_moments.hip.h): the arrays as given
struct ObservedSet {
  int32_t nexp = 0, nseg = 0; int64_t npix = 0;
  DevBuf d_seg, d_gain;                              // [nseg + 1], [npix] or none
  std::vector<int64_t> seg;                          // [nseg + 1] on the host: trx_set_filter cuts its tiles from it
  int64_t ndead = 0;                                 // entries whose weight as installed is not > 0 (none without weights)
  // the data [nexp][npix] and the weights, the same or none (all 1), in force (.now) and as trx_set_observed installed them
  // (.raw(), ../trx_launch.h).  trx_detrend_observed (trx_sysrem.hip.h) adopts a call's residuals as the data and its undo
  // restores them; trx_weigh_observed (trx_scatter.hip.h) adopts a call's weights, and its undo and every successful
  // trx_detrend_observed restore them.  The data have a third level (../trx_hpdata.h): trx_highpass_observed covers what is
  // in force with its high-passed version, its undo uncovers it, and every successful trx_detrend_observed discards it
  DataInForce<DevBuf> d_data; InForce<DevBuf> d_weight;
};
// a filter installed by trx_set_filter over the observed set (trx_filter.hip.h): the matrices zero-padded to npad
// components and exposure-major, and the tiles of the observed set's segments
struct FilterSet {
  int32_t ncomp = 0, npad = 0, nexp = 0, nseg = 0; int64_t npix = 0, ntiles = 0;
  DevBuf d_fwd, d_back, d_tiles;                     // [nseg][nexp][npad] each, FilterTile[ntiles]
  // a weighted filter (trx_set_weighted_filter, trx_wfilter.hip.h): its padded basis in d_back (d_fwd stays empty), and
  // every column's factor [nfac][npix] and pivot flag [npix], made by k_wfilter_factor when it was installed
  bool weighted = false; int32_t nfac = 0;
  DevBuf d_fac, d_live;
};
// a high-pass installed by trx_set_highpass over the observed set (trx_highpass.hip.h): the taps, their full-window sum and
// the tiles of the observed set's segments; obs: that set (it goes when the set does), whose gains the kernel reads
struct HighPassSet {
  int32_t half = 0, nseg = 0; int64_t npix = 0, ntiles = 0; double den_full = 0; const ObservedSet *obs = nullptr;
  DevBuf d_taps, d_tiles;                            // [half + 1], HpTile[ntiles]
};
// an exposure table installed by trx_set_exposures over the observed set (trx_pixels.hip.h, ../trx_exposures.h): the two
// arrays as given, on the host -- a run uploads them with its shifts (an array the caller left out is empty)
struct ExposureSet {
  int32_t nexp = 0;
  std::vector<double> scale, smear;                  // [nexp] each, or empty
};
// a pixel run (trx_run_pixels): the set and the run's shifts, already in h->d_pixshift; obs: a moment run (trx_run_moments);
// filt: with the filter between the pairs and the moments (trx_run_filtered_moments); trail: the shifts are the lags of a
// trail (trx_run_trail) -- every exposure of obs against every one of them (trx_trail.hip.h), never with a filter; ext: the
// extents of its buffers (../trx_products.h), which pixel_run works out, grows them to and leaves here for the guards and copies;
// hp: with the high-pass between the pairs and whatever reads them (pixel_run sets it for every run with obs on a handle that
// has one; trx_run_highpassed itself), hpx the extents of that; ex: the rows are exposures and take the handle's exposure
// table (trx_run_exposed, and trx_run_moments and trx_run_filtered_moments on a handle with one), already in h->d_exscale
// and h->d_exsmear; ex_rows: ex is the call's own set of one entry per ROW of a map under the table (trx_run_exposed_map:
// nexp = nshift rows, each a lag at an exposure), not the handle's
struct PixelRun {
  const PixelSet *set; int32_t nshift; const ObservedSet *obs = nullptr; const FilterSet *filt = nullptr; bool trail = false; PixelExtents ext{};
  const HighPassSet *hp = nullptr; HighpassExtents hpx{};
  const ExposureSet *ex = nullptr; bool ex_rows = false;
};
// a broadening installed by trx_set_broadening (trx_broaden.hip.h): two scalars, and the half-width of the grid's last bin --
// the largest -- which sizes the kernel's tile
struct Broadening { double beta = 0, limb = 0; int hmax = 0; };
// what a run makes behind its spectrum (run_once, Run): nothing (trx_run, trx_run_device), or
struct Products {
  // a band run (trx_run_bands) -- the spectrum goes to h->d_spec like trx_run_device's, the band kernels follow the
  // spectrum kernel on its queue, and the host copy of the spectrum (when asked for) is the plain copy command
  const BandSet *bs = nullptr;
  // a contribution run (trx_run_contrib) -- the kernels of trx_contrib.hip.h follow the band kernels
  bool contrib = false;
  // a pixel run (trx_run_pixels) -- the spectrum stays on the device as for bs, the kernel of trx_pixels.hip.h follows it,
  // and (px->obs: trx_run_moments) the kernel of trx_moments.hip.h follows that -- or (px->trail: trx_run_trail) the one of
  // trx_trail.hip.h
  const PixelRun *px = nullptr;
  // the broadening of a broadened run (trx_run_broadened) or of a pixel run on a handle with one installed -- the spectrum
  // stays on the device as for bs, the kernel of trx_broaden.hip.h follows it, and the pixel kernel reads what that one wrote
  const Broadening *br = nullptr;
};

// The handle's test switches: environment variables read at trx_create -- ALL of them, by read_switches
// alone, before any stage.  Each selects between two forms of the same computation that give the same
// bits (the tests named compare them side by side); none is needed in production, none changes a result.
// (The A/B switches of forms that lost -- run graphs, the range size, tile-size tuning beyond what a
// test forces -- are gone with those forms.)
struct Switches {
  bool no_row_copy = false;         // TRX_NO_ROW_COPY: wide frames without the walk's row copy (test_gpu_properties)
  bool no_rows32 = false;           // TRX_NO_ROWS32: k_line_walk_lanes<8> on the 64-byte rows (test_gpu_lanes)
  bool row_staging = true;          // osamp == 1: wide profiles through k_accumulate_rows (TRX_NO_ROW_STAGING: k_accumulate_wide; test_gpu_rows)
  long long row_m8_from = 768;      // ... profile width (bins) from which a layer's tiles are 512 bins (TRX_ROWS_M8_FROM: test_gpu_rows, measurements)
  bool packed_walk = true; int packed_max_layers = 10;   // steps of few layers walk several ranges per wave (TRX_NO_PACKED_WALK: never; TRX_PACKED_MAX_LAYERS: up to N layers, 1..32; test_gpu_packed)
  int xcd_map = 1;                  // TRX_XCD_MAP: blocks -> ranges by XCD (xcd_block): bit 0 k_line_walk_lanes, bit 1 k_line_walk (measured: slower there)
  bool no_binrec = false;           // TRX_NO_BINREC: k_ray_tail finds a bin's records through the ranges' numbers (A/B, tests)
  // steps of at most 32 layers with frames of 8+ bins: lanes = lines for the strengths (trx_lanes.hip.h)
  bool lanes_walk = true, lanes_force = false;      // TRX_LANES_WALK=0: the one-range / packed forms; =2: also on sparse lists (test_gpu_lanes)
  int lanes_parts_most = 4;         // TRX_LANES_PARTS: k_line_walk_lanes with at most 2, 3 or 4 lanes per layer in phase 2 (test_gpu_lanes_parts)
  bool ray_tail = true;             // hinted eclipse runs end in k_ray_tail (TRX_RAY_TAIL=0: the step kernels; test_gpu_tail, measurements)
  bool cia_sums = true;             // the CIA splines' second derivatives as sums per row (TRX_CIA_SUMS=0: the sweeps of k_cia_layers; tests)
  bool cia_segments = true;         // k_cia_layers in pieces of 128 rows (TRX_CIA_SEGMENTS=0: one sweep per table; test_gpu_cia_window)
  bool cia_window = true;           // the CIA spline solved for the table rows a run needs (TRX_CIA_WINDOW=0: the whole table; test_gpu_cia_window)
  bool two_queues = true;           // the second walk of a hinted run on a queue of its own, next to the first (TRX_TWO_QUEUES=0: behind it; A/B, tests)
  bool tail_direct = true;          // ... which writes spectrum and flags straight into pinned host memory (TRX_TAIL_DIRECT=0: copy commands)
  bool range_reach = true;          // k_line_walk tests a group's reach against its RANGE's widest profile and leaves a range out of all reach with zeros at its start (TRX_RANGE_REACH=0: the step's bound, every range walked; needs TablePlan::psize_mono; test_gpu_walk_reach, A/B)
  bool shard_frames = true;         // frames sized for the Doppler indices the lines in reach can take (TRX_SHARD_FRAMES=0: for the isotope's whole wavenumber range; test_gpu_shard_frames)
};

}  // namespace

struct trx_handle {
  int device = 0;
  hipStream_t stream = nullptr, stream2 = nullptr;   // stream2: CIA kernels, overlapped with the first sweep step
  // stream4: the line sweep of step c+1 runs while `stream` integrates the optical depth of
  // step c; ev_ac[c] = extinction of step c complete
  hipStream_t stream4 = nullptr;
  std::vector<hipEvent_t> ev_ac, ev_cb;      // ev_cb[c] = partial records of step c consumed
  hipEvent_t ev_walk1 = nullptr;                     // the first walk of a two-queue run (and the CIA kernels) are done
  hipEvent_t ev_inputs = nullptr, ev_cia = nullptr, ev_join = nullptr, ev_run_a = nullptr, ev_run_b = nullptr;
  std::string err;

  // grids
  double wn_i = 0, wn_d = 0, odwn = 0; int64_t nwn = 0, nown = 0, lo = 0, hi = 0, nsh = 0; int osamp = 1;
  // isotopes / molecules (host copies)
  int niso = 0, nmol = 0;
  std::vector<double> iso_mass, iso_ratio, mol_mass, mol_radius, mol_pol;
  std::vector<double> pair_csd, pair_sqrt;          // [niso][nmol]: r_mol + r_iso's molecule, sqrt(1/m_iso + 1/m_mol) (extinction.c:376-380)
  std::vector<int32_t> iso_imol, mol_is_h2;
  std::vector<double> iso_wmin, iso_wmax;          // anchor wavenumber range per isotope
  // Voigt table
  int ndop = 0, nlor = 0;
  std::vector<double> adop, alor;                   // +1 sentinel
  std::vector<int32_t> psizeT; bool psize_mono = false;   // psize as [nlor][ndop] (prep_layers); no profile narrower than the one a Doppler index below it
  std::vector<double> dopthr;                       // steps of the nearest-index function on adop (build_table; dop_index)
  std::vector<double> lorthr;                       // the same on alor (empty: the grid did not pass the check -- nearest_index is called)
  std::vector<int> guess_dop, guess_lor, guess_a0, guess_a1;      // [niso] where prep_layers found the layer above (its walks start there)
  std::vector<long> guess_npre;                     // [niso] and the layer above's count of groups at or above the refresh cut
  std::vector<double> iso_sqrtm;                    // sqrt(iso_mass)
  std::vector<double> dens_over_m;                  // [nmol] scratch of prep_layers
  std::vector<int32_t> psize; std::vector<long long> poff; int64_t tab_n = 0;
  DevBuf d_adop, d_dopthr, d_e2tab, d_psize, d_poff, d_tab, d_tabT, d_poffT, d_gimod, d_gidiv;
  // both tables carry kTabPad zero floats in front and behind: k_accumulate_wide reads whole
  // 4-float lane segments around a profile row and masks what lies outside the row
  float *tab = nullptr; const float *tabT = nullptr; const long long *poffT = nullptr;
  // the walk's copy: phase-major rows of whole cache lines (walk_row_layout), one WalkProfile per table entry
  DevBuf d_tabW, d_walkprof; const float *tabW = nullptr; bool tabw_ok = false;
  DevBuf d_tabW32, d_wp32; const float *tabW32 = nullptr; unsigned slab32 = 0;      // compact 32-byte rows for frames of 8 bins (k_table_rows32)
  std::vector<std::pair<double, double>> recip_ok;     // divisors whose reciprocal quotient_rn may use (checked_reciprocal)
  int max_gcount = 0; DevBuf d_linebase, d_rinfo;      // the largest co-added group; what k_line_walk_lanes reads per line and per range (trx_lanes.hip.h)
  Switches sw;
  // lines
  int64_t nlines = 0, ngroups = 0, nadd = 0, ninrange = 0;
  DevBuf d_lgroup, d_wavn, d_elow, d_gf, d_iso, d_inr, d_gfirst, d_gcount, d_giown, d_giso, d_gwavn, d_gblock, d_cntge, d_cntsub;
  int sub_f = 1;                        // sub-buckets per coarse cell of d_cntsub (1: it is d_cntge)
  LinesDev L{};
  HostBuf<double> h_gwavn; std::vector<int32_t> h_gblock; HostBuf<int32_t> h_cntge, h_gfirst, h_gcount;   // host copies for the per-run prologue
  void *comm = nullptr; int nranks = 1, rank = 0;          // RCCL communicator: only trx_gather uses it
  bool windowed() const { return lo > 0 || hi < nwn; }    // a shard sweeps only the lines that can reach it
  // candidates for the layer maximum (k_cand_*): indices into the line arrays; -1 = use every line
  DevBuf d_cand, d_candrec; int64_t ncand = -1;             // candidate line indices / their packed line data
  DevBuf d_kmax;                                            // [2][layer] (runs alternate; k_layer_max) / [layer][nmx] (per-molecule sweeps)
  int kmax_parity = 0, kmax_nr = 0; bool kmax_clean = false;   // clean: the half the next run will use is zero
  // the walk (k_line_walk): one record per line, line ranges of ngw groups, plans per profile reach
  DevBuf d_walk, d_wbase, d_part[2];   // partial records: consecutive steps alternate
  std::vector<int32_t> h_wbase; int nwaves = 0, ngw = 0; bool walk_ok = false;
  bool walk_temp_ok = true;         // this run's layers are all warmer than kWalkMinTemp
  struct Plan { bool built = false; DevBuf blo, bhi, off, binw, binrec; int64_t records = 0; };
  Plan plan[4];                                             // NB = 2, 4, 8, 16 bins per frame
  // CIA (host copies)
  struct Cia { int nspec; int mol[2]; std::vector<double> wn, temp, cs, zt, uw, ruw, rh, wf, wb; DevBuf d_wn, d_temp, d_cs, d_zt, d_uw, d_ruw, d_rh, d_wf, d_wb; };      // wf, wb: weights of k_cia_v / k_cia_z (empty: the sweeps)
  std::vector<Cia> cia;
  DevBuf d_cia_ws;
  // per-run workspaces (grown on demand)
  DevBuf d_SG, d_idop8, d_sticky, d_part3;
  // per-run inputs: packed into ONE pinned host block and copied with ONE transfer
  // (layer scalars, ray geometry, impact parameters, CIA density products)
  DevBuf d_in; PinnedBuf h_in;
  DevBuf d_pm_f64, d_pm_i32;         // the same scalars of a per-molecule sweep (trx_sweep_permol)
  // what the host reads back after a run, in ONE device block and one pinned host block:
  // flags (8 ints, byte 0), status (4 ints, byte 64), counters (3 per layer, byte 128)
  DevBuf d_xf;                        // scattering / cloud wavenumber factors [2][nsh] + 3 constants
  DevBuf d_small; DevView d_flags, d_status, d_counters; PinnedBuf h_small;
  DevBuf d_e, d_ecs, d_er, d_tau, d_last, d_intens, d_spec, d_acc, d_geom;
  // opacity grid (optional)
  bool has_grid = false; long og_nmol = 0, og_ntemp = 0, og_nlayer = 0, og_nwave = 0;
  std::vector<double> og_temp; std::vector<int32_t> og_molidx; DevBuf d_og_o, d_og_layer, d_og_itemp, d_iso_mx, d_pm;
  trx_stats stats{};
  std::vector<double> run_f64, run_geom, run_ipv; std::vector<int32_t> run_i32;      // per-run host arrays (kept: no allocation per run)
  std::vector<int> run_frame; std::vector<unsigned char> run_wide;      // [layer] walk_frame_bins, and the plan's "very wide" mark (trx_plan.h)
  std::vector<PlanStep> run_plan;                                        // the steps of the pass being queued
  std::vector<QueueOp> run_sched;                                        // ... and its schedule (trx_schedule.h), issued op by op
  std::vector<double> run_og_layer; std::vector<int> run_og_itemp;       // opacity grid: the layers' weights and temperature brackets (Run::grid_weights)
  int hint_layers = 0;       // layers the previous run needed (deepest toomuch crossing + 1)
  DevBuf d_e_saved; std::vector<uint8_t> saved;          // trx_restore_extinction: [nlayer][nsh] and the flags (empty: none)
  PinnedBuf h_spec;          // staging of the spectrum (trx_run hands over pageable memory)
  PinnedBuf h_tailblk;       // what each block of k_ray_tail adds to the run's flags (vertical rays: the host adds them up)
  std::unique_ptr<BandSet> bands;                      // trx_set_bands (null: none)
  // trx_run_contrib (trx_contrib.hip.h): sub-piece rows [npieces * kContribSplit][nlayer] and the pinned result [nbands][nlayer], sized on
  // first use and when the set or nlayer grows
  DevBuf d_cpart; PinnedBuf h_contrib;
  std::unique_ptr<PixelSet> pixels;                    // trx_set_pixels (null: none)
  DevBuf d_pixshift, d_pixout;                         // trx_run_pixels: the run's shifts [nshift] and its pairs [nshift][npix][2], grown on demand
  std::unique_ptr<ObservedSet> observed;               // trx_set_observed (null: none); belongs to `pixels`
  DevBuf d_mom;                                        // trx_run_moments: [nexp][nseg][TRX_NMOMENT], grown on demand
  DevBuf d_trail;                                      // trx_run_trail: [nlag][nexp][nseg][TRX_NMOMENT], grown on demand
  // trx_run_velocity_map (trx_vmap.hip.h), grown on demand: the call's arrays lag_kms, kp, vsys, orbit, offset end to end (their
  // host copy: vm_in), the statistic [nlag][nexp] followed by its transpose [nexp][nlag], the map [nkp][nvsys]
  DevBuf d_vm_in, d_vm_per, d_vm_map; std::vector<double> vm_in;
  // trx_run_filtered_map (trx_cellmap.hip.h), grown on demand: the call's arrays in d_vm_in as above, the nearest-lag table
  // [nkp * nvsys][nexp] int32, one chunk's filtered values [chunk][nexp][npix] and moments [chunk][nexp][nseg][TRX_NMOMENT],
  // the map [nkp][nvsys]
  DevBuf d_cm_index, d_cm_val, d_cm_mom, d_cm_map;
  // trx_run_exposed_map (trx_expmap.hip.h), grown on demand: the spans [nexp][2] int32 of the call's exposures (their host
  // copy: em_span), the first row [nexp] int64 of each, the row table [nkp * nvsys][nexp] int32 beside the lag table
  DevBuf d_em_span, d_em_base, d_em_row; std::vector<int32_t> em_span;
  std::unique_ptr<FilterSet> filter;                   // trx_set_filter (null: none); belongs to `observed`
  DevBuf d_pixval;                                     // trx_run_filtered_moments: the filtered values [nexp][npix], grown on demand
  std::unique_ptr<HighPassSet> highpass;               // trx_set_highpass (null: none); belongs to `observed`
  // the high-passed pairs [nshift][npix][2] of a run with a high-pass, (g', 1) or (0, 0), grown on demand: what the filter, the
  // moments and the trail then read in place of d_pixout; trx_run_highpassed copies them to h_pixhp whole
  DevBuf d_pixhp; PinnedBuf h_pixhp;
  bool broad_on = false; Broadening broad;             // trx_set_broadening (broad_on false: none); independent of the sets above
  DevBuf d_broad;                                      // the broadened spectrum [nwn] of a broadened or pixel run, grown on demand
  std::unique_ptr<ExposureSet> exposures;              // trx_set_exposures (null: none); belongs to `observed`
  DevBuf d_exscale, d_exsmear;                         // the table's arrays [nexp] each, uploaded by every run that takes it, grown on demand
  // trx_detrend_observed (trx_sysrem.hip.h), grown on demand: the residuals [nexp][npix] a call builds (swapped with the
  // observed set's data when it succeeds), the time vector [nseg][nexp], the column vector [npix], coef [ncomp][npix],
  // U [nseg][nexp][ncomp] (its host copy: sr_basis) and the tiles of the set's segments
  DevBuf d_sr_r, d_sr_a, d_sr_c, d_sr_coef, d_sr_basis, d_sr_tiles; std::vector<double> sr_basis;
  // trx_pca_observed (trx_pca.hip.h), grown on demand beside the detrend's residuals, coef, U and tiles, which it shares: the
  // live flags [nseg][nexp] and the whole flags [npix] (int32), the Gram matrices and the transposed eigenvector matrices
  // [nseg][nexp][nexp] each, eigen [nseg][ncomp], offdiag [nseg] and nwhole [nseg] (int64)
  DevBuf d_pc_live, d_pc_whole, d_pc_g, d_pc_v, d_pc_eigen, d_pc_off, d_pc_nwhole;
  bool pc_lds_raised = false;                          // k_pca_jacobi's limit of dynamic LDS has been raised on this handle's device
  // trx_weigh_observed (trx_scatter.hip.h), grown on demand: the weights [nexp][npix] a call builds (swapped with the observed
  // set's when it succeeds), the variances [npix], the medians [nseg], the columns' flags [npix] and the tiles; the factor
  // and the pivot flags a call makes for the installed weighted filter (swapped with the filter's)
  DevBuf d_sc_w, d_sc_var, d_sc_med, d_sc_flag, d_sc_tiles, d_sc_fac, d_sc_live;
  // trx_highpass_observed (trx_highpass.hip.h), grown on demand: the high-passed data [nexp][npix] a call builds (swapped
  // with the observed set's data when it succeeds; the previous call's, or an undone one, waits here for the next)
  DevBuf d_hp_r;
  // trx_set_normalise (trx_normalise.hip.h): the recipe of step 1b of the detrending calls (norm_on false: none); belongs to
  // `observed`.  Grown on demand: the row scales [nexp][nseg], the centres [npix], the columns' two counts [2][npix] (int32;
  // their host copy: nm_count) and the tiles (their staging vector: nm_tiles, which outlives the upload)
  bool norm_on = false; trx_normalise norm{};
  DevBuf d_nm_scale, d_nm_centre, d_nm_count, d_nm_tiles; std::vector<int32_t> nm_count; std::vector<FilterTile> nm_tiles;
};

namespace {

// process-wide message sink (trx_set_log): the reference's tr_output()/verblevel pair
struct LogSink { trx_log_fn fn = nullptr; void *user = nullptr; int max_level = 0; };
LogSink &log_sink() { static LogSink s; return s; }
void log_msg(int level, const std::string &msg)
{
  const LogSink s = log_sink();
  if (s.fn && level <= s.max_level) s.fn(level, msg.c_str(), s.user);
}

// stage timer of trx_create: logs "create: <stage> x.xx ms" at TRX_LOG_DEBUG
struct StageTimer {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char *what) {
    const auto n = std::chrono::steady_clock::now();
    if (log_sink().fn && log_sink().max_level >= TRX_LOG_DEBUG) {
      char b[128]; std::snprintf(b, sizeof b, "create: %-28s %8.2f ms", what, std::chrono::duration<double, std::milli>(n - t).count());
      log_msg(TRX_LOG_DEBUG, b);
    }
    t = n;
  }
};

int fail(trx_handle *h, int code, const std::string &msg)
{ if (h) h->err = msg; log_msg(TRX_LOG_ERROR, msg); return code; }

#define HIPCHK(h, call)                                                              \
  do { hipError_t e_ = (call);                                                       \
       if (e_ != hipSuccess)                                                         \
         return fail(h, e_ == hipErrorOutOfMemory ? TRX_E_NOMEM : TRX_E_HIP,         \
                     std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

int ensure(trx_handle *h, DevBuf &b, size_t bytes)
{
  if (bytes == 0) bytes = 8;
  if (b.bytes >= bytes) return TRX_OK;
  b.release();
  HIPCHK(h, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return TRX_OK;
}

// grow-only, with exactly the size asked for
int ensure_pinned(trx_handle *h, PinnedBuf &b, size_t bytes)
{
  if (b.bytes >= bytes) return TRX_OK;
  b.release();
  HIPCHK(h, hipHostMalloc(&b.p, bytes, hipHostMallocDefault));
  b.bytes = bytes;
  HIPCHK(h, hipHostGetDevicePointer(&b.dev, b.p, 0));
  return TRX_OK;
}

// the small read-back block for nlay layers (device + pinned host mirror)
int ensure_small(trx_handle *h, int nlay)
{
  const size_t bytes = 128 + 24 * (size_t)nlay;
  if (const int rc = ensure(h, h->d_small, bytes)) return rc;
  char *base = (char *)h->d_small.p;
  h->d_flags.p = base; h->d_status.p = base + 64; h->d_counters.p = base + 128;
  return ensure_pinned(h, h->h_small, bytes);
}

template <class T>
int upload_raw(trx_handle *h, DevBuf &b, const T *p, size_t n)
{
  int rc = ensure(h, b, n * sizeof(T));
  if (rc) return rc;
  if (n) HIPCHK(h, hipMemcpyAsync(b.p, p, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return TRX_OK;
}

template <class T>
int upload(trx_handle *h, DevBuf &b, const std::vector<T> &v)
{
  int rc = ensure(h, b, v.size() * sizeof(T));
  if (rc) return rc;
  if (!v.empty()) HIPCHK(h, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return TRX_OK;
}

template <class T>
int upload(trx_handle *h, DevBuf &b, const HostBuf<T> &v) { return upload_raw(h, b, v.data(), v.size()); }

}  // namespace
