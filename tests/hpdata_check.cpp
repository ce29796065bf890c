// hpdata_check.cpp -- high-passing the observed set itself (trx_highpass_observed) without a device: the staging rule and the
// window walk of transit_amd/csrc/trx_highpass.h, walked over tiles, waves and lanes exactly as k_data_highpass walks them,
// and the checks, the extents, the launch guard and the three levels of the data of transit_amd/csrc/trx_hpdata.h.
// Stand-alone (tests/test_hpdata_host.py builds it under -ffp-contract=off -fsanitize=address,undefined); every array handed
// to the headers is a heap allocation of exactly the stated length, so a read past an extent is a sanitizer report.
//
//   hpdata_check                 the refusal table, the extents, the guard, the buffer transitions; prints "ok <checks>"
//   hpdata_check values IN OUT   IN: int64 nexp, npix, nseg, half, has_weight; int64 seg_first[nseg + 1]; double
//                                taps[half + 1]; double weight[nexp][npix] (has_weight); double data[nexp][npix].
//                                OUT: double values[nexp][npix], +0 = dead -- by the kernel's walk, after holding every
//                                value against the literal definition (terms skipped, not added as zeros); prints ndead
//                                and the share of waves that took the full-window path
#include <cmath>
#include <cstring>
#include <vector>

#include "transit_hip.h"
#include "trx_hpdata.h"
#include "check_common.h"

using namespace trx;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- one row the way k_data_highpass takes it: tile by tile, staged from the data and the weights into arrays of exactly
// count + 2 half entries, wave by wave (the ballot over the wave's windows), lane by lane (kHpOuts outputs each)
static void row_by_tiles(const HighpassLayout &L, const double *r /* [npix] */, const double *w /* [npix] or null */, double *values /* [npix] */,
                         int64_t &waves, int64_t &full_waves)
{
  const int half = L.half;
  for (const HpTile &T : L.tiles) {
    const int count = T.count, n = count + 2 * half;
    Heap<double> g((size_t)n), m((size_t)n);
    for (int i = 0; i < n; i++) {
      const int64_t q = T.first - half + i;
      const bool inside = q >= T.seg_first && q < T.seg_last;
      highpass_stage_datum(inside ? r[q] : 0.0, inside && w ? w[q] : 1.0, inside, g[(size_t)i], m[(size_t)i]);
    }
    for (int w0 = 0; w0 < kHpBlock && w0 < count; w0 += 64) {
      bool full = true;
      for (int j = 0; j < kHpOuts; j++) {
        const int o = w0 + j * kHpBlock;
        const int end = o < count ? std::min(o + 64, count) + 2 * half : 0;
        for (int i = o; i < end; i++) full = full && m[(size_t)i] != 0.0;
      }
      waves++; full_waves += full ? 1 : 0;
      for (int lane = 0; lane < 64; lane++) {
        int at[kHpOuts]; double v[kHpOuts];
        for (int j = 0; j < kHpOuts; j++) at[j] = half + std::min(w0 + j * kHpBlock + lane, count - 1);
        highpass_values<kHpOuts>(g.get(), m.get(), at, half, L.taps.data(), full, L.den_full, v);
        for (int j = 0; j < kHpOuts; j++) {
          const int p = w0 + j * kHpBlock + lane;
          if (p < count) values[T.first + p] = m[(size_t)at[j]] != 0.0 ? v[j] : 0.0;
        }
      }
    }
  }
}

// ---- the literal definition: one entry at a time, a term outside the segment or not live SKIPPED
static void row_literal(int32_t nseg, const int64_t *seg, int half, const double *taps, const double *r, const double *w, double *values)
{
  for (int32_t s = 0; s < nseg; s++)
    for (int64_t p = seg[s]; p < seg[s + 1]; p++) {
      if (w && !(w[p] > 0.0)) { values[p] = 0.0; continue; }
      double num = 0.0, den = 0.0;
      for (int k = -half; k <= half; k++) {
        const int64_t q = p + k;
        if (q < seg[s] || q >= seg[s + 1] || (w && !(w[q] > 0.0))) continue;
        const double t = taps[k < 0 ? -k : k];
        num += t * r[q]; den += t;
      }
      values[p] = r[p] - num / den;
    }
}

static int values_mode(const char *in_path, const char *out_path)
{
  std::FILE *f = std::fopen(in_path, "rb");
  if (!f) { std::printf("cannot read %s\n", in_path); return 2; }
  int64_t head[5];
  if (std::fread(head, sizeof(int64_t), 5, f) != 5) return 2;
  const int64_t nexp = head[0], npix = head[1], nseg = head[2], half = head[3]; const bool has_w = head[4] != 0;
  Heap<int64_t> seg((size_t)nseg + 1); Heap<double> taps((size_t)half + 1), w(has_w ? (size_t)(nexp * npix) : 0), r((size_t)(nexp * npix));
  if (std::fread(seg.get(), sizeof(int64_t), seg.n, f) != seg.n || std::fread(taps.get(), sizeof(double), taps.n, f) != taps.n ||
      std::fread(w.get(), sizeof(double), w.n, f) != w.n || std::fread(r.get(), sizeof(double), r.n, f) != r.n) return 2;
  std::fclose(f);
  ProductState S; S.npix = npix; S.nexp = (int32_t)nexp; S.nseg = (int32_t)nseg; S.seg = seg.get(); S.highpass = true;
  trx_highpass hp{(int32_t)half, 0, taps.get()};
  std::string msg; HighpassLayout L;
  if (hpdata_checks(S, 1, msg) || highpass_set_checks(S, &hp, msg) || highpass_layout(S, &hp, L, msg)) { std::printf("refused: %s\n", msg.c_str()); return 2; }
  const HpDataExtents X = hpdata_extents(npix, (int32_t)nexp, (int64_t)L.tiles.size(), (int32_t)half);
  if (hpdata_launch_checks(X, msg)) { std::printf("refused: %s\n", msg.c_str()); return 2; }
  Heap<double> out((size_t)(nexp * npix), -1.0), lit((size_t)npix, -1.0);
  if (X.r_bytes != sizeof(double) * out.n || X.blocks != nexp * (int64_t)L.tiles.size()) return 2;
  int64_t differ = 0, ndead = 0, waves = 0, full_waves = 0;
  for (int64_t v = 0; v < nexp; v++) {
    const double *const row = r.get() + v * npix, *const wrow = has_w ? w.get() + v * npix : nullptr;
    row_by_tiles(L, row, wrow, out.get() + v * npix, waves, full_waves);
    row_literal((int32_t)nseg, seg.get(), (int)half, taps.get(), row, wrow, lit.get());
    for (int64_t p = 0; p < npix; p++) {
      if (wrow && !(wrow[p] > 0.0)) ndead++;
      if (!same_bits(out[(size_t)(v * npix + p)], lit[(size_t)p])) {
        if (differ++ < 10) std::printf("FAILED row %lld pixel %lld: tiles %a, literal %a\n", (long long)v, (long long)p, out[(size_t)(v * npix + p)], lit[(size_t)p]);
      }
    }
  }
  f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(out.get(), sizeof(double), out.n, f) != out.n) return 2;
  std::fclose(f);
  std::printf("values %lld rows %lld pixels %zu tiles, %lld differ from the literal definition\n", (long long)nexp, (long long)npix, L.tiles.size(), (long long)differ);
  std::printf("ndead %lld\nwaves %lld full %lld\n", (long long)ndead, (long long)waves, (long long)full_waves);
  return differ ? 1 : 0;
}

// ---- the staging rule ---------------------------------------------------------------------------------------
static void staging()
{
  double g = -1, m = -1;
  highpass_stage_datum(2.5, 1.0, true, g, m); CHECK(g == 2.5 && m == 1.0);
  highpass_stage_datum(-2.5, 1e-300, true, g, m); CHECK(g == -2.5 && m == 1.0);                    // (any weight above 0 is live: the flag is 1, not the weight)
  highpass_stage_datum(2.5, 0.0, true, g, m); CHECK(g == 0.0 && !std::signbit(g) && m == 0.0 && !std::signbit(m));
  highpass_stage_datum(-2.5, -0.0, true, g, m); CHECK(g == 0.0 && !std::signbit(g) && m == 0.0);
  highpass_stage_datum(2.5, kNaN, true, g, m); CHECK(g == 0.0 && m == 0.0);                         // (NaN > 0 is false)
  highpass_stage_datum(2.5, 1.0, false, g, m); CHECK(g == 0.0 && !std::signbit(g) && m == 0.0);     // (outside the segment)
  highpass_stage_datum(-0.0, 1.0, true, g, m); CHECK(g == 0.0 && std::signbit(g) && m == 1.0);      // (the datum as it is)
}

// ---- the refusal table, the extents, the guard ------------------------------------------------------------
struct Installed {
  Heap<int64_t> seg{0, 2, 6};
  ProductState S;
  Installed() { S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.lo = 0; S.hi = 5000; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get(); S.highpass = true; }
};

static void refusals()
{
  const Installed I; const std::string who = "trx_highpass_observed: ";
  ACCEPTED(hpdata_checks(I.S, 1, msg));
  ACCEPTED(hpdata_checks(I.S, 0, msg));
  CHECK(hpdata_is_undo(0) && !hpdata_is_undo(1));
  ProductState N = I.S; N.seg = nullptr;
  ProductState Z = I.S; Z.npix = 0;
  ProductState H = I.S; H.highpass = false;
  ProductState W = I.S; W.windowed = true; W.lo = 10;
  const std::string no_set = who + "no observed set installed (trx_set_observed)", bad = who + "apply must be 0 (undo) or 1",
                    no_hp = who + "no high-pass installed (trx_set_highpass)",
                    shard = who + "this handle's shard is not the whole grid; high-pass on the host (xcor.highpass_observed_reference)";
  for (int32_t apply : {0, 1, 2, -1}) {
    REFUSED(hpdata_checks(N, apply, msg), TRX_E_ARG, no_set.c_str());
    REFUSED(hpdata_checks(Z, apply, msg), TRX_E_ARG, no_set.c_str());
  }
  for (int32_t apply : {2, -1, 7, INT32_MIN, INT32_MAX}) {
    REFUSED(hpdata_checks(I.S, apply, msg), TRX_E_ARG, bad.c_str());
    REFUSED(hpdata_checks(H, apply, msg), TRX_E_ARG, bad.c_str());                                    // (ahead of the missing high-pass)
    REFUSED(hpdata_checks(W, apply, msg), TRX_E_ARG, bad.c_str());                                    // (and of the shard)
  }
  REFUSED(hpdata_checks(H, 1, msg), TRX_E_ARG, no_hp.c_str());
  ACCEPTED(hpdata_checks(H, 0, msg));                                                                 // (the undo needs no high-pass)
  REFUSED(hpdata_checks(W, 1, msg), TRX_E_UNSUPPORTED, shard.c_str());
  REFUSED(hpdata_checks(W, 0, msg), TRX_E_UNSUPPORTED, shard.c_str());
  { ProductState HW = W; HW.highpass = false; REFUSED(hpdata_checks(HW, 1, msg), TRX_E_ARG, no_hp.c_str()); }
  { ProductState NW = W; NW.seg = nullptr; REFUSED(hpdata_checks(NW, 1, msg), TRX_E_ARG, no_set.c_str()); }
}

static void extents_and_guard()
{
  const HpDataExtents X = hpdata_extents(800, 7, 13, 70);
  CHECK(X.cells == 5600 && X.blocks == 91 && X.r_bytes == 44800 && X.lds_bytes == 16 * (size_t)(kHpTile + 140));
  const HighpassExtents M = highpass_extents(800, 7, 13, 70);
  CHECK(X.lds_bytes == M.lds_bytes && X.blocks == M.blocks && X.r_bytes == M.val_bytes);             // (the model kernel's tile, one double an entry)
  const HpDataExtents Y = hpdata_extents(81920, 100, 160, TRX_HIGHPASS_MAX_HALF);
  CHECK(Y.cells == 8192000 && Y.blocks == 16000 && Y.r_bytes == 65536000 && Y.lds_bytes == 16 * (size_t)(kHpTile + 2048) && Y.lds_bytes <= 65536);
  const HpDataExtents Z = hpdata_extents(3000000000LL, 3, 1, 0);                                     // (past 2^31 entries: 64-bit throughout)
  CHECK(Z.cells == 9000000000LL && Z.r_bytes == 72000000000ULL && Z.blocks == 3 && Z.lds_bytes == 16 * (size_t)kHpTile);
  ACCEPTED(hpdata_launch_checks(X, msg));
  ACCEPTED(hpdata_launch_checks(Y, msg));
  { const HpDataExtents E = hpdata_extents(1, 7, 0, 3); REFUSED(hpdata_launch_checks(E, msg), TRX_E_ARG, "trx_highpass_observed: the observed set has no pixel in any segment"); }
  // the grid: nexp * ntiles up to 2^31 - 1 and no further
  { const HpDataExtents E = hpdata_extents(8, 0x7fffffff, 1, 0); CHECK(E.blocks == 0x7fffffffLL); ACCEPTED(hpdata_launch_checks(E, msg)); }
  { const HpDataExtents E = hpdata_extents(8, 0x7fffffff, 2, 0); CHECK(E.blocks == 0xfffffffeLL);
    REFUSED(hpdata_launch_checks(E, msg), TRX_E_ARG, "trx_highpass_observed: nexp * ntiles above what one launch takes"); }
  { const HpDataExtents E = hpdata_extents(8, 65536, 32768, 0); CHECK(E.blocks == 0x80000000LL);
    REFUSED(hpdata_launch_checks(E, msg), TRX_E_ARG, "trx_highpass_observed: nexp * ntiles above what one launch takes"); }
}

// ---- the three levels of the data ---------------------------------------------------------------------------
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

static void data_levels()
{
  auto empty = [](const CountedBuf &b) { return !b.p && b.bytes == 0; };
  {  // the raw set: cover, cover, uncover -- F under, the two calls' buffers swap, F back and the r' into the spare
    DataInForce<CountedBuf> S; CountedBuf raw(8), one(16), two(24);
    const void *const F = raw.p, *const A = one.p, *const B = two.p;
    exchange_buf(S.now, raw);
    CHECK(S.base().p == F && S.raw().p == F && !S.covered && !S.adopted);
    S.cover(one);
    CHECK(S.now.p == A && S.base().p == F && S.raw().p == F && S.covered && !S.adopted && empty(one));
    S.cover(two);                                                         // (the second call read base(): F, never A)
    CHECK(S.now.p == B && S.base().p == F && S.raw().p == F && two.p == A && two.bytes == 16);
    CountedBuf spare;
    S.uncover(spare);
    CHECK(S.now.p == F && S.now.bytes == 8 && !S.covered && empty(S.under) && spare.p == B && S.base().p == F && S.raw().p == F);
    S.uncover(spare);                                                     // (twice: nothing moves)
    CHECK(S.now.p == F && !S.covered && spare.p == B);
    CHECK(CountedBuf::live == 3 && CountedBuf::released == 0);
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 3);
  {  // detrend, high-pass, detrend as trx_detrend_observed does it: uncover into the high-pass's spare, then adopt
    DataInForce<CountedBuf> S; CountedBuf raw(8), r1(16), hp1(24), r2(32), hp_spare;
    const void *const F = raw.p, *const R1 = r1.p, *const H1 = hp1.p, *const R2 = r2.p;
    exchange_buf(S.now, raw);
    S.adopt(r1);
    CHECK(S.now.p == R1 && S.raw().p == F && S.base().p == R1 && S.adopted && !S.covered);
    S.cover(hp1);
    CHECK(S.now.p == H1 && S.base().p == R1 && S.raw().p == F && S.adopted && S.covered);   // (under is a residual: adopted says so)
    S.uncover(hp_spare); S.adopt(r2);
    CHECK(S.now.p == R2 && S.raw().p == F && S.base().p == R2 && !S.covered && S.adopted && r2.p == R1 && hp_spare.p == H1);
    // high-pass again from the spare, then the detrend's undo
    S.cover(hp_spare);
    CHECK(S.now.p == H1 && S.base().p == R2 && empty(hp_spare));
    CountedBuf sr_spare;
    S.uncover(hp_spare); S.restore(sr_spare);
    CHECK(S.now.p == F && S.raw().p == F && S.base().p == F && !S.covered && !S.adopted && sr_spare.p == R2 && hp_spare.p == H1 && empty(S.aside) && empty(S.under));
    CHECK(CountedBuf::live == 4 && CountedBuf::released == 3);
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 7);
  {  // adopt and restore on covered data without the uncover: the r' is discarded, nothing leaks, F is never lost
    DataInForce<CountedBuf> S; CountedBuf raw(8), hp1(24), r1(16), hp2(24), spare;
    const void *const F = raw.p, *const R1 = r1.p, *const H2 = hp2.p;
    exchange_buf(S.now, raw);
    S.cover(hp1);
    S.adopt(r1);                                                          // (r' over F released; F aside)
    CHECK(S.now.p == R1 && S.raw().p == F && !S.covered && S.adopted && CountedBuf::released == 8);
    S.cover(hp2);
    S.restore(spare);                                                     // (r' over r released; r into the spare; F in force)
    CHECK(S.now.p == F && S.raw().p == F && !S.covered && !S.adopted && spare.p == R1 && CountedBuf::released == 9);
    (void)H2;
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 11);
  {  // uncover with a spare that is taken: the r' is released, not leaked; high-pass over the raw set, then the detrend's undo
    DataInForce<CountedBuf> S; CountedBuf raw(8), hp1(24), spare(32), sr;
    const void *const F = raw.p, *const D = spare.p;
    exchange_buf(S.now, raw);
    S.cover(hp1);
    S.uncover(spare);
    CHECK(S.now.p == F && !S.covered && spare.p == D && spare.bytes == 32 && CountedBuf::released == 12);
    S.cover(spare);
    S.uncover(spare); S.restore(sr);                                      // (detrend_observed(0) on a set that was never detrended)
    CHECK(S.now.p == F && S.raw().p == F && !S.covered && !S.adopted && spare.p == D && empty(sr));
  }
  CHECK(CountedBuf::live == 0 && CountedBuf::released == 14);
}

int main(int argc, char **argv)
{
  if (argc == 4 && !std::strcmp(argv[1], "values")) return values_mode(argv[2], argv[3]);
  staging();
  refusals();
  extents_and_guard();
  data_levels();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
