// trx_api_sweep.hip.h -- one step of the line sweep as kernel launches: the walk (walk_chunk: the range plan, the record
// buffer, the arguments, the shard's window, the form, the launch; launch_combine: its combine) and the two-kernel form (sweep_chunk:
// strengths, accumulation, the wide layers' kernels), the per-kernel timing of a profiled run (Spans), and the layer
// maxima and sticky indices that leave the per-step chain.  What a launch DECIDES -- frames, windows, line counts, forms,
// masks -- is ../trx_sweep.h's, plain C++ that tests/sweep_check.cpp runs on the CPU; here it is launched.  Part of the
// one translation unit trx_api.hip, which includes it inside its anonymous namespace between the layer prologue and the
// C ABI.
#pragma once

// ---- per-kernel timing of a profiled run: (start, end) event pairs on the stream of the kernel ----
struct Spans {
  enum Kind { kSweep = 0, kWalk = 1, kAccum = 2, kTau = 3, kWalkLanes = 4, kWalkPacked = 5, kKinds = 6 };      // (kWalk: k_line_walk itself; the three walk forms add up to trx_stats.ms_k_walk)
  struct Span { hipEvent_t a, b; int kind; };
  std::vector<Span> v;
  int begin(int kind, hipStream_t st) {
    Span sp{nullptr, nullptr, kind};
    if (hipEventCreate(&sp.a) != hipSuccess || hipEventCreate(&sp.b) != hipSuccess) return -1;
    v.push_back(sp);
    return hipEventRecord(sp.a, st) == hipSuccess ? 0 : -1;
  }
  int end(hipStream_t st) { return hipEventRecord(v.back().b, st) == hipSuccess ? 0 : -1; }
  void sum(double out[kKinds]) const {
    for (const Span &sp : v) { float t = 0; if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess) out[sp.kind] += t; }
  }
  static bool is_walk(int k) { return k == kWalk || k == kWalkLanes || k == kWalkPacked; }
  // first walk's start to last walk's end (the walks of one run may share the device on two queues)
  double walk_span() const {
    double best = 0;
    for (const Span &x : v) if (is_walk(x.kind))
      for (const Span &y : v) if (is_walk(y.kind)) { float t = 0; if (hipEventElapsedTime(&t, x.a, y.b) == hipSuccess && t > best) best = t; }
    return best;
  }
  ~Spans() { for (Span &sp : v) { if (sp.a) (void)hipEventDestroy(sp.a); if (sp.b) (void)hipEventDestroy(sp.b); } }
};

// ---- one step of the line sweep ------------------------------------------------------------
struct SweepMode {
  bool eager = false, prof = false, skip_done = false, permol = false;
  double ethresh = 0;
  int nmx = 1; const int32_t *d_iso_mx = nullptr;   // output slot per isotope (per-molecule sweeps)
  double *d_e = nullptr;                             // [layer][nmx][nsh]
  const double *d_kmax = nullptr;                    // [layer][nmx] (k_layer_max)
  const int *d_sticky = nullptr;                     // [layer][iso] (k_sticky_index)
  hipStream_t st = nullptr;                          // null: the handle's stream
};

// the host's group tables as the launch decisions read them (trx_sweep.h)
GroupView group_view(const trx_handle *h)
{
  GroupView G;
  G.niso = h->niso; G.gblock = h->h_gblock.data(); G.cntge = h->h_cntge.data(); G.wbase = h->h_wbase.data();
  G.gfirst = h->h_gfirst.data(); G.gcount = h->h_gcount.data();
  G.ngw = h->ngw; G.nwn = h->nwn; G.lo = h->lo; G.hi = h->hi; G.osamp = h->osamp; G.windowed = h->windowed();
  return G;
}

// per layer: the walk's frame (0: the two-kernel form) and the plan's "very wide" mark (null: not wanted); true
// when some layer needs the two-kernel form
bool layer_frames(const trx_handle *h, const int32_t *psmax, int nv, int *frame, unsigned char *wide)
{
  const GroupView G = group_view(h);
  bool any_wide = false;
  for (int r = 0; r < nv; r++) {
    const long long psm = layer_psmax(G, psmax, r);
    frame[r] = walk_frame_bins(h->walk_ok, h->walk_temp_ok, psm, h->osamp);
    if (wide) wide[r] = very_wide(psm, h->osamp);
    any_wide = any_wide || frame[r] == 0;
  }
  return any_wide;
}

// plan of the line ranges for a frame of nb bins (built once per handle and frame size)
int walk_plan(trx_handle *h, int nb, hipStream_t st, WalkPlan &P, trx_handle::Plan *&pl)
{
  const int v = nb == 2 ? 0 : nb == 4 ? 1 : nb == 8 ? 2 : 3;
  pl = &h->plan[v];
  int rc;
  if (!pl->built) {
    const size_t nw = (size_t)std::max(h->nwaves, 1);
    if ((rc = ensure(h, pl->blo, 4 * nw)) || (rc = ensure(h, pl->bhi, 4 * nw)) || (rc = ensure(h, pl->off, 8 * (nw + 1)))) return rc;
  }
  P.nwaves = h->nwaves; P.ngw = h->ngw; P.wbase = h->d_wbase.as<int32_t>();
  P.blo = pl->blo.as<int32_t>(); P.bhi = pl->bhi.as<int32_t>(); P.off = pl->off.as<int64_t>();
  // (the per-bin range table: 8 bytes per bin and isotope; above 2^24 entries the combine searches instead)
  const long long nbinw = (long long)h->nsh * h->niso;
  const bool with_binw = nbinw > 0 && nbinw <= (1LL << 24);
  if (!pl->built && with_binw && (rc = ensure(h, pl->binw, 8 * (size_t)nbinw))) return rc;
  P.binw = with_binw ? pl->binw.as<int32_t>() : nullptr;
  // (and the bin's record in each of its first 64 ranges, for k_ray_tail: 256 bytes per bin and isotope, small shards only)
  const bool with_binrec = with_binw && nbinw <= (1LL << 17) && !h->sw.no_binrec;
  if (!pl->built && with_binrec && (rc = ensure(h, pl->binrec, 256 * (size_t)nbinw))) return rc;
  P.binrec = with_binrec ? pl->binrec.as<int32_t>() : nullptr;
  if (!pl->built) {
    hipLaunchKernelGGL(k_wave_plan, dim3(1), dim3(256), 0, st, P, h->niso, h->d_gblock.as<int32_t>(), h->d_gidiv.as<int32_t>(),
                       nb / 2 - 1, (long long)h->lo, (long long)h->hi);
    if (with_binw)
      hipLaunchKernelGGL(k_bin_ranges, dim3((unsigned)((nbinw + 255) / 256)), dim3(256), 0, st, P, h->niso, (long long)h->lo, (long long)h->nsh);
    int64_t total = 0;
    HIPCHK(h, hipMemcpyAsync(&total, P.off + h->nwaves, sizeof total, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));                 // once per handle and frame size
    pl->records = total; pl->built = true;
  }
  if (pl->records >= (1LL << 31)) P.binrec = nullptr;      // (32-bit record numbers)
  return TRX_OK;
}

template <int NB>
void launch_walk(const WalkArgs &A, bool prof, unsigned nwaves, hipStream_t st)
{
  const dim3 grid((nwaves + kWalkWaves - 1) / kWalkWaves), block(64 * kWalkWaves);
  if (prof) hipLaunchKernelGGL((k_line_walk<NB, true>), grid, block, 0, st, A);
  else if constexpr (NB >= 8) {      // steps of at most 32 layers: two lanes per layer (trx_walk.hip.h)
    if (A.nc <= 32) hipLaunchKernelGGL((k_line_walk<NB, false, 2>), grid, block, 0, st, A);
    else            hipLaunchKernelGGL((k_line_walk<NB, false>), grid, block, 0, st, A);
  }
  else      hipLaunchKernelGGL((k_line_walk<NB, false>), grid, block, 0, st, A);
}

// the combine of a walk's partial sums, on the queue its optical depth follows on
int launch_combine(trx_handle *h, const CombineArgs &C, hipStream_t q, Spans *sp)
{
  if (sp && sp->begin(Spans::kAccum, q)) return fail(h, TRX_E_HIP, "event");
  hipLaunchKernelGGL(k_walk_combine, dim3((unsigned)((h->nsh + kCombineBins - 1) / kCombineBins)), dim3(64 * kCombineBins), 0, q, C);
  if (sp && sp->end(q)) return fail(h, TRX_E_HIP, "event");
  return TRX_OK;
}

// What a walk step (walk_chunk) hands back.
struct WalkResult {
  CombineArgs C{};                     // its combine, for the caller to launch (launch_combine) or to hand to the ray tail
  int form = -1;                       // which kernel the production run takes for the step (trx_sweep.h: WalkKind)
};

// the step's record buffer, large enough for the plan's records
int record_buffer(trx_handle *h, const trx_handle::Plan &pl, int parity, hipStream_t st, DevBuf *&part)
{
  part = &h->d_part[parity & 1];
  const size_t pbytes = sizeof(double) * kWalkLayers * (size_t)std::max<int64_t>(pl.records, 1);
  if (part->bytes >= pbytes) return TRX_OK;
  HIPCHK(h, hipStreamSynchronize(st));                 // an earlier step may still be using the old buffer
  HIPCHK(h, hipStreamSynchronize(h->stream4));          // (combines of earlier steps run there)
  return ensure(h, *part, pbytes);
}

// the walk kernels' arguments but for the window: the handle's tables, the step and the mode
WalkArgs walk_args(const trx_handle *h, const LayerDev &Y, const double *d_wcut, const PlanStep &s, const SweepMode &M,
                   const WalkPlan &P, double *part)
{
  WalkArgs A{};
  A.lines = h->d_walk.as<WalkLine>(); A.rinfo = h->d_rinfo.as<RangeInfo>(); A.gfirst = h->d_gfirst.as<int32_t>(); A.gcount = h->d_gcount.as<int32_t>();
  A.gblock = h->d_gblock.as<int32_t>(); A.P = P;
  A.niso = h->niso; A.nlor = h->nlor; A.ndop = h->ndop; A.osamp = h->osamp; A.lo = h->lo; A.hi = h->hi;
  A.wn_i = h->wn_i; A.odwn = h->odwn; A.range_reach = h->sw.range_reach && h->psize_mono;      // (a table whose profiles narrow somewhere as the Doppler index rises keeps the step's bound)
  A.r_top = s.r_top; A.nc = s.nc; A.Y = Y; A.wcut = d_wcut; A.kmax = M.d_kmax; A.ethresh = M.ethresh;
  A.nmx = M.nmx; A.iso_mx = M.d_iso_mx; A.permol = M.permol; A.sticky_idop = M.d_sticky;
  A.dthr = h->d_dopthr.as<double>(); A.e2tab = h->d_e2tab.as<double>();
  A.psize = h->d_psize.as<int32_t>(); A.poff = h->d_poff.as<long long>();
  A.table = h->tab; A.zero_index = h->tab_n;
  A.tabw = h->tabW; A.walkprof = h->d_walkprof.as<WalkProfile>();
  A.tabw32 = h->tabW32; A.wp32 = h->tabW32 ? h->d_wp32.as<uint32_t>() : nullptr; A.slab32 = h->slab32;
  A.xcd_map = h->sw.xcd_map & 2;                        // (bit 1: k_line_walk, bit 0: k_line_walk_lanes)
  A.part = part; A.counters = M.prof ? h->d_counters.as<unsigned long long>() : nullptr;
  A.flags = h->d_flags.as<int>(); A.last = M.skip_done ? h->d_last.as<int>() : nullptr; A.eager = M.eager;
  return A;
}

// the kernel of the form decided (trx_sweep.h: walk_form) over the window's nw waves
void launch_walk_form(const trx_handle *h, WalkArgs &A, const WalkForm &F, unsigned nw, int nb, hipStream_t st)
{
  const int nc = A.nc;
  if (F.launched == kFormLanes) {
    // one range per wave (round 4 measured 2, 3, 4 ranges per wave at the demo size: 0.257 / 0.283 / 0.276 ms for the
    // spectrum's two walks against 0.239 -- the last lines of a range already get lanes = (line, 4 or 8 layer sets);
    // the kernel no longer has that form)
    LanesExtra X{h->d_linebase.as<double>()};
    A.xcd_map = h->sw.xcd_map & 1;
    if (log_sink().fn && log_sink().max_level >= TRX_LOG_DEBUG)
      log_msg(TRX_LOG_DEBUG, "walk: lanes = lines, " + std::to_string(nc) + " layers, " + std::to_string(nb) + "-bin frames, " +
                             std::to_string(F.parts) + " lanes per layer");
    const dim3 grid((nw + kLanesWaves - 1) / kLanesWaves), block(64 * kLanesWaves);
    const size_t lds = lanes_lds_bytes(nc, h->ndop);
    // (blocks of 5 groups at 8 bins: a batch's ~28 are 6 blocks, an even number; 4: 102.2 us, 5: 101.2, 6: 103.6, round 5.
    // Blocks of 2 at 16 bins -- with two lanes per layer 8 floats per group and lane, 112 registers: 169.5 us; 3 / 4:
    // 130 / 150 registers, 171.0 / 172.6, round 5.)  Lanes per layer in phase 2: lanes_parts
    if (nb == 8) switch (F.parts) {
      case 4:  hipLaunchKernelGGL((k_line_walk_lanes<8, 5, 4>), grid, block, lds, st, A, X); break;
      case 3:  hipLaunchKernelGGL((k_line_walk_lanes<8, 5, 3>), grid, block, lds, st, A, X); break;
      default: hipLaunchKernelGGL((k_line_walk_lanes<8, 5, 2>), grid, block, lds, st, A, X);
    }
    else switch (F.parts) {
      case 4:  hipLaunchKernelGGL((k_line_walk_lanes<16, 2, 4>), grid, block, lds, st, A, X); break;
      case 3:  hipLaunchKernelGGL((k_line_walk_lanes<16, 2, 3>), grid, block, lds, st, A, X); break;
      default: hipLaunchKernelGGL((k_line_walk_lanes<16, 2, 2>), grid, block, lds, st, A, X);
    }
  }
  else if (F.launched == kFormPacked) {
    const unsigned pw = (nw + (unsigned)F.S - 1) / (unsigned)F.S;
    const dim3 grid((pw + kWalkWaves - 1) / kWalkWaves), block(64 * kWalkWaves);
    switch (F.packed_nb) {
      case 4:  hipLaunchKernelGGL(k_line_walk_packed<4>, grid, block, 0, st, A, F.S); break;
      case 8:  hipLaunchKernelGGL(k_line_walk_packed<8>, grid, block, 0, st, A, F.S); break;
      default: hipLaunchKernelGGL(k_line_walk_packed<16>, grid, block, 0, st, A, F.S);
    }
  }
  else if (nw > 0) switch (nb) {
    case 2:  launch_walk<2>(A, F.per_bin, nw, st); break;
    case 4:  launch_walk<4>(A, F.per_bin, nw, st); break;
    case 8:  launch_walk<8>(A, F.per_bin, nw, st); break;
    default: launch_walk<16>(A, F.per_bin, nw, st);
  }
}

// the arguments of the combine of a walk's partial sums
CombineArgs combine_of(const trx_handle *h, const WalkArgs &A, const SweepMode &M)
{
  CombineArgs C{};
  C.P = A.P; C.niso = h->niso; C.gblock = h->d_gblock.as<int32_t>(); C.lo = h->lo; C.nsh = h->nsh; C.r_top = A.r_top; C.nc = A.nc;
  C.nmx = M.nmx; C.iso_mx = M.d_iso_mx; C.part = A.part; C.e = M.d_e;
  C.flags = h->d_flags.as<int>(); C.last = A.last; C.eager = M.eager;
  return C;
}

// what walk_form (trx_sweep.h) reads of the handle and the step
WalkFormIn walk_form_in(const trx_handle *h, const PlanStep &s, unsigned nw, bool prof)
{
  WalkFormIn in;
  in.nw = nw; in.row_copy = h->tabW != nullptr; in.nb = s.nb; in.nc = s.nc; in.prof = prof;
  in.lanes_walk = h->sw.lanes_walk; in.lanes_force = h->sw.lanes_force;
  in.packed_walk = h->sw.packed_walk; in.packed_max_layers = h->sw.packed_max_layers;
  in.max_gcount = h->max_gcount; in.ngroups = h->ngroups; in.nwn = h->nwn;
  in.lanes_parts = lanes_parts(s.nc, h->sw.lanes_parts_most);
  return in;
}

// The walk: layers s.r_top .. s.r_top-s.nc+1 (nc <= 64) in one kernel on M.st, into record buffer `parity`; the
// combine of its partial sums is handed back (R.C).  Consecutive steps alternate between two record buffers, so that
// the next step's walk does not wait for this step's combine.
int walk_chunk(trx_handle *h, const LayerDev &Y, const double *d_wcut, const PlanStep &s, const SweepMode &M, Spans *sp,
               int parity, WalkResult &R)
{
  static_assert(kSweepSegs == kWalkSegs, "trx_sweep.h sizes the window for the kernels' segment count");
  constexpr WalkCaps kCaps{kLanesMaxLayers, kLanesMaxGroup, kWalkRowsFrom};
  hipStream_t st = M.st ? M.st : h->stream;
  WalkPlan P{}; trx_handle::Plan *pl = nullptr; DevBuf *part = nullptr;
  int rc = walk_plan(h, s.nb, st, P, pl);
  if (rc) return rc;
  // (trx_stats describes the last trx_run: a per-molecule sweep (trx_sweep_permol) walks too but is not counted)
  if (!M.permol) { h->stats.walk_steps++; h->stats.walk_records += pl->records; h->stats.walk_record_lanes += pl->records * s.nc; }
  if ((rc = record_buffer(h, *pl, parity, st, part))) return rc;
  WalkArgs A = walk_args(h, Y, d_wcut, s, M, P, part->as<double>());
  const WalkWindow W = walk_window(group_view(h), s.nb, h->nwaves);
  A.nseg = W.nseg; std::copy(W.seg_w0, W.seg_w0 + kWalkSegs, A.seg_w0); std::copy(W.seg_cum, W.seg_cum + kWalkSegs + 1, A.seg_cum);
  const WalkForm F = walk_form(walk_form_in(h, s, W.nw, M.prof), kCaps);
  R.form = F.prod;
  if (!M.permol) { h->stats.walk_form_steps[F.prod]++; h->stats.walk_form_layers[F.prod] += s.nc; h->stats.walk_form_record_lanes[F.prod] += pl->records * s.nc; }
  if (sp && sp->begin(F.launched == kFormLanes ? Spans::kWalkLanes : F.launched == kFormPacked ? Spans::kWalkPacked : Spans::kWalk, st)) return fail(h, TRX_E_HIP, "event");
  launch_walk_form(h, A, F, W.nw, s.nb, st);
  if (sp && sp->end(st)) return fail(h, TRX_E_HIP, "event");
  R.C = combine_of(h, A, M);
  return TRX_OK;
}

// the accumulation kernels' arguments: the handle's tables, the step and the mode
AccumArgs accum_args(const trx_handle *h, const LayerDev &Y, const PlanStep &s, const SweepMode &M, int ntiles, unsigned tblocks)
{
  AccumArgs A{};
  A.L = h->L; A.Y = Y; A.niso = h->niso; A.nlor = h->nlor; A.ndop = h->ndop; A.osamp = h->osamp;
  A.nwn = h->nwn; A.lo = h->lo; A.nsh = h->nsh; A.r_top = s.r_top; A.nc = s.nc; A.ntiles = ntiles;
  A.SG = h->d_SG.as<double>(); A.idop8 = h->d_idop8.as<uint8_t>(); A.sticky_idop = M.d_sticky;
  A.kmaxc = M.d_kmax; A.ethresh = M.ethresh; A.nmx = M.nmx; A.iso_mx = M.d_iso_mx; A.permol = M.permol;
  A.psize = h->d_psize.as<int32_t>(); A.poff = h->d_poff.as<long long>();
  A.table = h->tab; A.e = M.d_e;
  // (profiled runs count every group in the tile of its own coarse cell: whole-cell windows)
  A.sub_f = M.prof ? 1 : h->sub_f; A.cnt_sub = A.sub_f > 1 ? h->d_cntsub.as<int32_t>() : h->d_cntge.as<int32_t>();
  A.part = M.prof ? h->d_part3.as<unsigned long long>() : nullptr; A.part_stride = (int)tblocks;
  A.flags = h->d_flags.as<int>(); A.eager = M.eager;
  A.last = M.skip_done ? h->d_last.as<int>() : nullptr;
  return A;
}

// the very wide layers of a two-kernel step (trx_sweep.h: wide_masks): the lanes-own-bins kernels
void launch_wide(const trx_handle *h, const AccumArgs &A, const WideMasks &K, bool prof, hipStream_t st)
{
  const unsigned nc = (unsigned)A.nc;
  WideArgs W{}; W.A = A; W.tabT = h->tabT; W.poffT = h->poffT;
  W.gimod = h->d_gimod.as<int32_t>(); W.gidiv = h->d_gidiv.as<int32_t>(); W.layer_mask = K.wide;
  if (!(h->osamp == 1 && h->sw.row_staging)) {
    const unsigned wtiles = (unsigned)((A.nsh + 64 * kWideM - 1) / (64 * kWideM));
    hipLaunchKernelGGL(k_accumulate_wide, dim3((wtiles + 3) / 4, nc), dim3(256), 0, st, W);
    return;
  }
  // no oversampling: every group of a profile reads the same row -- staged in LDS (trx_rows.hip.h);
  // layers whose profiles are much wider than a tile take tiles of 512 bins, the others of 256
  auto launch = [&](unsigned mask, int m) {
    if (!mask) return;
    W.layer_mask = mask;
    const unsigned tiles = (unsigned)((A.nsh + 64 * m - 1) / (64 * m));
    const dim3 grid((tiles + 3) / 4, nc);
    const size_t lds = rows_lds_bytes(h->ndop, m);
    if (prof) hipLaunchKernelGGL((k_accumulate_rows<true, 4>), grid, dim3(256), lds, st, W);      // (counting runs: one tile size)
    else if (m == 8) hipLaunchKernelGGL((k_accumulate_rows<false, 8>), grid, dim3(256), lds, st, W);
    else hipLaunchKernelGGL((k_accumulate_rows<false, 4>), grid, dim3(256), lds, st, W);
  };
  if (prof) launch(K.wide, 4);
  else { launch(K.wide & ~K.m8, 4); launch(K.m8, 8); }
}

// The two-kernel form (profiles wider than the walk's largest frame): strengths, accumulation.
// nc_max: layers the counting run's per-tile counters are sized for.
int sweep_chunk(trx_handle *h, const LayerDev &Y, const double *d_wcut, const int32_t *psmax,
                const PlanStep &s, int nc_max, const SweepMode &M, Spans *sp)
{
  hipStream_t st = M.st ? M.st : h->stream;
  const int niso = h->niso, r_top = s.r_top, nc = s.nc;
  const int ntiles = (int)((h->nsh + kTileBins - 1) / kTileBins);
  const GroupView G = group_view(h);
  // lines whose profiles can reach this shard in any layer of the step (contiguous per isotope block):
  // their number here, for the launch; the runs themselves are found by the kernel (SweepWindow)
  SweepWindow Wn{};
  Wn.windowed = h->windowed() ? 1 : 0; Wn.osamp = h->osamp; Wn.lo = h->lo; Wn.hi = h->hi; Wn.nwn = h->nwn;
  const long long seg_lines = sweep_window_lines(G, psmax, r_top, nc);
  constexpr unsigned kSpan = kXcds * kAccumXcdGroup;
  const unsigned tblocks = (unsigned)(((ntiles + 3) / 4 + kSpan - 1) / kSpan * kSpan);   // multiple of 8*G: xcd_grouped_x()
  if (sp && sp->begin(Spans::kSweep, st)) return fail(h, TRX_E_HIP, "event");
  if (seg_lines > 0) {
    hipLaunchKernelGGL(k_group_sweep, dim3((unsigned)((seg_lines + 255) / 256)), dim3(256), sizeof(long long) * (2 * (size_t)niso + 1), st,
                       h->L, Y, Wn, niso, r_top, nc, h->d_dopthr.as<double>(), h->ndop, h->d_e2tab.as<double>(), d_wcut,
                       h->d_SG.as<double>(), h->d_idop8.as<uint8_t>(), h->d_flags.as<int>(), (int)M.eager);
  }
  if (sp && (sp->end(st) || sp->begin(Spans::kAccum, st))) return fail(h, TRX_E_HIP, "event");
  if (h->ngroups > 0) {
    AccumArgs A = accum_args(h, Y, s, M, ntiles, tblocks);
    // layers whose profiles span >= 64 coarse bins go to the lanes-own-bins kernels
    const WideMasks K = wide_masks(G, psmax, r_top, nc, h->sw.row_m8_from);
    A.skip_mask = K.wide;
    if (M.prof) HIPCHK(h, hipMemsetAsync(h->d_part3.p, 0, 24 * (size_t)nc_max * tblocks, st));
    if (!K.all_wide) hipLaunchKernelGGL(k_accumulate, dim3(tblocks, (unsigned)nc), dim3(256), 0, st, A);
    if (K.wide) launch_wide(h, A, K, M.prof, st);
  }
  if (sp && sp->end(st)) return fail(h, TRX_E_HIP, "event");
  if (M.prof && h->ngroups > 0) {      // counters (profiling runs only; gated like the sweep itself)
    for (int k = 0; k < 3; k++)
      hipLaunchKernelGGL(k_sum_parts_gated, dim3((unsigned)nc), dim3(256), 0, st, h->d_part3.as<unsigned long long>(),
                         (int)tblocks, 3, k, h->d_counters.as<unsigned long long>(), 3, r_top, h->d_flags.as<int>(), (int)M.eager);
  }
  return TRX_OK;
}

// Strongest single line and sticky Doppler index of ALL nv layers (states) at once: both depend
// on the inputs only, not on how far the rays get, so they leave the per-step chain.
// kmax: [nv][nmx], zero on entry.  init: the run's small buffers, initialised by an extra row of
// blocks of the first launch (null: none); *init_done tells whether that happened.
// Two launches, each usable on its own: trx_run queues the maxima BEFORE the rest of its host prologue
// (they need -c/T and the strength factors only, which it hands over in pinned host memory).
int launch_layer_max(trx_handle *h, const LayerDev &Y, int nv, const double *temp_k, int nmx, const int32_t *d_iso_mx,
                     hipStream_t st, double *kmax, const RunInit *init = nullptr, bool *init_done = nullptr)
{
  if (init_done) *init_done = false;
  if (h->ngroups == 0) return TRX_OK;
  // the pruning argument needs c*nu/T well above the rounding of 1 - exp(-c*nu/T) (trx_walk.hip.h)
  bool pruned = h->ncand > 0;
  for (int r = 0; r < nv && pruned; r++) if (kExpCte * kTliEfct * h->wn_i / temp_k[r] < 1e-5) pruned = false;
  const long long n = pruned ? h->ncand : h->nlines;
  for (int r0 = 0; r0 < nv; r0 += 32768) {
    const int nr = std::min(32768, nv - r0);
    LayerDev Yr = Y; Yr.negc_over_t += r0; Yr.strength_f += (size_t)r0 * h->niso;
    const unsigned ny = (unsigned)((nr + kLayerMaxGroup - 1) / kLayerMaxGroup);
    const bool with_init = init && r0 == 0;
    RunInit R{}; R.nsh = -1;
    if (with_init) { R = *init; *init_done = true; }
    // (at most kLayerMaxWaves waves per group of layers: beyond that a wave takes several chunks of candidates)
    const int xwaves = (int)std::min<long long>((n + 64 * kLayerMaxLines - 1) / (64 * kLayerMaxLines), kLayerMaxWaves);
    hipLaunchKernelGGL(k_layer_max, dim3((unsigned)((xwaves + kLayerMaxBlock - 1) / kLayerMaxBlock), ny + (with_init ? 1u : 0u)), dim3(64 * kLayerMaxBlock), sizeof(double) * (size_t)kLayerMaxGroup * (size_t)std::max(h->niso, 1), st,
                       h->L, Yr, h->niso, nr, pruned ? h->d_candrec.as<CandLine>() : nullptr, n, h->d_e2tab.as<double>(), nmx, d_iso_mx,
                       (unsigned long long *)(kmax + (size_t)r0 * nmx), R, with_init ? (int)ny : -1, xwaves);
  }
  return TRX_OK;
}

// (copy_*: the run's input block from pinned host memory into device memory, by extra blocks of the first launch)
int launch_sticky(trx_handle *h, const LayerDev &Y, const int32_t *d_npre, int nv, int nmx, const int32_t *d_iso_mx, double ethresh,
                  hipStream_t st, const double *kmax, const void *copy_src = nullptr, void *copy_dst = nullptr, size_t copy_bytes = 0)
{
  const long long n16 = (long long)(copy_bytes / 16);
  if (h->ngroups == 0 && n16 == 0) return TRX_OK;
  bool copied = n16 == 0;
  for (int r0 = 0; r0 < nv || !copied; r0 += 4096) {               // one wave per (layer, isotope)
    const int nr = h->ngroups == 0 ? 0 : std::max(0, std::min(4096, nv - r0));
    const int nst = nr * h->niso;
    const int ncp = copied ? 0 : (int)std::min<long long>((n16 + 63) / 64, 64);
    if (nst + ncp == 0) break;
    hipLaunchKernelGGL(k_sticky_index, dim3((unsigned)(nst + ncp)), dim3(64), 0, st,
                       h->L, Y, h->niso, r0 + nr - 1, nr, kmax, nmx, d_iso_mx, ethresh, h->d_dopthr.as<double>(), h->ndop,
                       h->d_e2tab.as<double>(), d_npre, h->d_sticky.as<int>(), h->d_flags.as<int>(), 1,
                       copied ? nullptr : (const uint4 *)copy_src, copied ? nullptr : (uint4 *)copy_dst, copied ? 0LL : n16, nst);
    copied = true;
  }
  HIPCHK(h, hipGetLastError());
  return TRX_OK;
}

int layer_maxima_and_sticky(trx_handle *h, const LayerDev &Y, const int32_t *d_npre, int nv, const double *temp_k,
                            int nmx, const int32_t *d_iso_mx, double ethresh, hipStream_t st, double *kmax,
                            const RunInit *init = nullptr, bool *init_done = nullptr)
{
  int rc;
  if (init_done) *init_done = false;
  if ((rc = ensure(h, h->d_sticky, sizeof(int) * (size_t)nv * std::max(h->niso, 1)))) return rc;
  if (h->ngroups == 0) return TRX_OK;
  if ((rc = launch_layer_max(h, Y, nv, temp_k, nmx, d_iso_mx, st, kmax, init, init_done))) return rc;
  return launch_sticky(h, Y, d_npre, nv, nmx, d_iso_mx, ethresh, st, kmax);
}
