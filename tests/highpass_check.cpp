// highpass_check.cpp -- the host side of the high-pass along the pixel axis without a device: the arithmetic of
// transit_amd/csrc/trx_highpass.h, walked over tiles, waves and lanes exactly as k_pixel_highpass walks it, and the checks,
// layout and extents of transit_amd/csrc/trx_products.h.  Stand-alone (tests/test_highpass_host.py builds it under
// -ffp-contract=off -fsanitize=address,undefined); every array handed to the headers is a heap allocation of exactly the
// stated length, so a read past an extent is a sanitizer report.
//
//   highpass_check                 the refusal table, the layout's invariants, the extents; prints "ok <checks>"
//   highpass_check values IN OUT   IN: int64 nrow, npix, nseg, half, has_gain; int64 seg_first[nseg + 1]; double
//                                  taps[half + 1]; double gain[npix] (has_gain); double pairs[nrow][npix][2].
//                                  OUT: double values[nrow][npix], NaN = dead -- by the kernel's walk, after holding
//                                  every value against the literal definition (terms skipped, not added as zeros)
#include <cmath>
#include <cstring>
#include <vector>

#include "transit_hip.h"
#include "trx_products.h"
#include "check_common.h"

using namespace trx;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

// ---- one row the way k_pixel_highpass takes it: tile by tile, staged into arrays of exactly count + 2 half entries, wave by
// wave (the ballot over the wave's windows), lane by lane (kHpOuts outputs each)
static void row_by_tiles(const HighpassLayout &L, const double *pairs /* [npix][2] */, const double *gain, double *values /* [npix] */)
{
  const int half = L.half;
  for (const HpTile &T : L.tiles) {
    const int count = T.count, n = count + 2 * half;
    Heap<double> g((size_t)n), m((size_t)n);
    for (int i = 0; i < n; i++) {
      const int64_t q = T.first - half + i;
      const bool inside = q >= T.seg_first && q < T.seg_last;
      highpass_stage(inside ? pairs[2 * q] : 0.0, inside ? pairs[2 * q + 1] : 0.0, inside && gain ? gain[q] : 1.0, inside, g[(size_t)i], m[(size_t)i]);
    }
    for (int w0 = 0; w0 < kHpBlock && w0 < count; w0 += 64) {
      bool full = true;
      for (int j = 0; j < kHpOuts; j++) {
        const int o = w0 + j * kHpBlock;
        const int end = o < count ? std::min(o + 64, count) + 2 * half : 0;
        for (int i = o; i < end; i++) full = full && m[(size_t)i] != 0.0;
      }
      for (int lane = 0; lane < 64; lane++) {
        int at[kHpOuts]; double v[kHpOuts];
        for (int j = 0; j < kHpOuts; j++) at[j] = half + std::min(w0 + j * kHpBlock + lane, count - 1);
        highpass_values<kHpOuts>(g.get(), m.get(), at, half, L.taps.data(), full, L.den_full, v);
        for (int j = 0; j < kHpOuts; j++) {
          const int p = w0 + j * kHpBlock + lane;
          if (p < count) values[T.first + p] = m[(size_t)at[j]] != 0.0 ? v[j] : kNaN;
        }
      }
    }
  }
}

// ---- the literal definition: one pixel at a time, a term outside the segment or not live SKIPPED
static void row_literal(int32_t nseg, const int64_t *seg, int half, const double *taps, const double *pairs, const double *gain, double *values)
{
  for (int32_t s = 0; s < nseg; s++)
    for (int64_t p = seg[s]; p < seg[s + 1]; p++) {
      if (!(pairs[2 * p + 1] > 0.0)) { values[p] = kNaN; continue; }
      double num = 0.0, den = 0.0;
      for (int k = -half; k <= half; k++) {
        const int64_t q = p + k;
        if (q < seg[s] || q >= seg[s + 1] || !(pairs[2 * q + 1] > 0.0)) continue;
        const double t = taps[k < 0 ? -k : k];
        const double gq = (gain ? gain[q] : 1.0) * (pairs[2 * q] / pairs[2 * q + 1]);
        num += t * gq; den += t;
      }
      const double gp = (gain ? gain[p] : 1.0) * (pairs[2 * p] / pairs[2 * p + 1]);
      values[p] = gp - num / den;
    }
}

static int values_mode(const char *in_path, const char *out_path)
{
  std::FILE *f = std::fopen(in_path, "rb");
  if (!f) { std::printf("cannot read %s\n", in_path); return 2; }
  int64_t head[5];
  if (std::fread(head, sizeof(int64_t), 5, f) != 5) return 2;
  const int64_t nrow = head[0], npix = head[1], nseg = head[2], half = head[3]; const bool has_gain = head[4] != 0;
  Heap<int64_t> seg((size_t)nseg + 1); Heap<double> taps((size_t)half + 1), gain(has_gain ? (size_t)npix : 0), pairs((size_t)(nrow * npix * 2));
  if (std::fread(seg.get(), sizeof(int64_t), seg.n, f) != seg.n || std::fread(taps.get(), sizeof(double), taps.n, f) != taps.n ||
      std::fread(gain.get(), sizeof(double), gain.n, f) != gain.n || std::fread(pairs.get(), sizeof(double), pairs.n, f) != pairs.n) return 2;
  std::fclose(f);
  ProductState S; S.npix = npix; S.nexp = 1; S.nseg = (int32_t)nseg; S.seg = seg.get();
  trx_highpass hp{(int32_t)half, 0, taps.get()};
  std::string msg; HighpassLayout L;
  if (highpass_set_checks(S, &hp, msg) || highpass_layout(S, &hp, L, msg)) { std::printf("refused: %s\n", msg.c_str()); return 2; }
  Heap<double> out((size_t)(nrow * npix), -1.0), lit((size_t)npix, -1.0);
  int64_t differ = 0;
  for (int64_t r = 0; r < nrow; r++) {
    const double *const row = pairs.get() + r * npix * 2;
    row_by_tiles(L, row, has_gain ? gain.get() : nullptr, out.get() + r * npix);
    row_literal((int32_t)nseg, seg.get(), (int)half, taps.get(), row, has_gain ? gain.get() : nullptr, lit.get());
    for (int64_t p = 0; p < npix; p++)
      if (!same_bits(out[(size_t)(r * npix + p)], lit[(size_t)p])) {
        if (differ++ < 10) std::printf("FAILED row %lld pixel %lld: tiles %a, literal %a\n", (long long)r, (long long)p, out[(size_t)(r * npix + p)], lit[(size_t)p]);
      }
  }
  f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(out.get(), sizeof(double), out.n, f) != out.n) return 2;
  std::fclose(f);
  std::printf("values %lld rows %lld pixels %zu tiles, %lld differ from the literal definition\n", (long long)nrow, (long long)npix, L.tiles.size(), (long long)differ);
  return differ ? 1 : 0;
}

// ---- the refusal table, the layout, the extents --------------------------------------------------------
struct Installed {
  Heap<int64_t> seg{0, 2, 6};
  ProductState S;
  Installed() { S.wn_i = 2000.0; S.wn_d = 0.1; S.nwn = 5000; S.lo = 0; S.hi = 5000; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get(); S.highpass = true; }
};

static void set_refusals()
{
  const Installed I;
  Heap<double> t3{1.0, 0.5, 0.0};
  auto with = [&](int32_t half, const double *taps, std::string &msg) { trx_highpass hp{half, 0, taps}; return highpass_set_checks(I.S, &hp, msg); };
  ACCEPTED(with(2, t3.get(), msg));
  ACCEPTED(with(0, t3.get(), msg));
  { ProductState N = I.S; N.seg = nullptr; trx_highpass hp{2, 0, t3.get()}; REFUSED(highpass_set_checks(N, &hp, msg), TRX_E_ARG, "highpass: no observed set installed (trx_set_observed)"); }
  { ProductState N = I.S; N.npix = 0; trx_highpass hp{2, 0, t3.get()}; REFUSED(highpass_set_checks(N, &hp, msg), TRX_E_ARG, "highpass: no observed set installed (trx_set_observed)"); }
  REFUSED(with(-1, t3.get(), msg), TRX_E_ARG, "highpass: half < 0");
  REFUSED(with(TRX_HIGHPASS_MAX_HALF + 1, t3.get(), msg), TRX_E_ARG, "highpass: half above TRX_HIGHPASS_MAX_HALF (1024)");      // (before any tap is read)
  { Heap<double> big((size_t)TRX_HIGHPASS_MAX_HALF + 1, 1.0); ACCEPTED(with(TRX_HIGHPASS_MAX_HALF, big.get(), msg)); }
  for (double bad : {kNaN, kInf, -kInf, -1.0, -0.5}) {
    Heap<double> t{1.0, bad, 1.0};
    REFUSED(with(2, t.get(), msg), TRX_E_ARG, "highpass: tap 1 must be finite and >= 0");
    Heap<double> t0{bad, 1.0};
    REFUSED(with(1, t0.get(), msg), TRX_E_ARG, "highpass: tap 0 must be finite and >= 0");
  }
  { Heap<double> t{1.0, 1.0, -1e-300}; REFUSED(with(2, t.get(), msg), TRX_E_ARG, "highpass: tap 2 must be finite and >= 0"); }
  { Heap<double> t{0.0, 1.0}; REFUSED(with(1, t.get(), msg), TRX_E_ARG, "highpass: tap 0 must be > 0"); }
  { Heap<double> t{0.0}; REFUSED(with(0, t.get(), msg), TRX_E_ARG, "highpass: tap 0 must be > 0"); }
}

static void run_refusals()
{
  const Installed I; const char *who = "trx_run_highpassed";
  Heap<double> sh{1.0, 1.0}, out(12);
  auto run = [&](const ProductState &S, int32_t n, const void *in, const void *o, std::string &msg) { return observed_run_checks(S, who, ObservedRun::Highpassed, n, in, o, "values", msg); };
  ACCEPTED(run(I.S, 2, sh.get(), out.get(), msg));
  ACCEPTED(run(I.S, 1, sh.get(), out.get(), msg));            // (any number of rows, not the set's nexp)
  ACCEPTED(run(I.S, 7, sh.get(), out.get(), msg));
  { ProductState W = I.S; W.windowed = true; W.lo = 10;
    REFUSED(run(W, 2, sh.get(), out.get(), msg), TRX_E_UNSUPPORTED,
            "trx_run_highpassed: this handle's shard is not the whole grid; take trx_run_pixels, add the ranks' pairs (trx_gather_host) and high-pass them on the host"); }
  { ProductState N = I.S; N.seg = nullptr; REFUSED(run(N, 2, sh.get(), out.get(), msg), TRX_E_ARG, "trx_run_highpassed: no observed set installed (trx_set_observed)"); }
  { ProductState N = I.S; N.highpass = false; REFUSED(run(N, 2, sh.get(), out.get(), msg), TRX_E_ARG, "trx_run_highpassed: no high-pass installed (trx_set_highpass)"); }
  REFUSED(run(I.S, 0, sh.get(), out.get(), msg), TRX_E_ARG, "trx_run_highpassed: nshift < 1");
  REFUSED(run(I.S, -3, sh.get(), out.get(), msg), TRX_E_ARG, "trx_run_highpassed: nshift < 1");
  REFUSED(run(I.S, 2, nullptr, out.get(), msg), TRX_E_ARG, "trx_run_highpassed: shift is NULL");
  REFUSED(run(I.S, 2, sh.get(), nullptr, msg), TRX_E_ARG, "trx_run_highpassed: values is NULL");
  // the shifts themselves and the launch's size: pixel_run_checks, as for every pixel run
  for (double bad : {kNaN, kInf, 0.0, -1.0}) {
    Heap<double> s{1.0, bad};
    REFUSED(pixel_run_checks(who, 2, 6, s.get(), msg), TRX_E_ARG, "trx_run_highpassed: shift 1 must be finite and > 0");
  }
  { Heap<double> s((size_t)3, 1.0); REFUSED(pixel_run_checks(who, 3, 0x7fffffffLL * kPixBlock / 3 + 1, s.get(), msg), TRX_E_ARG, "trx_run_highpassed: nshift * npix above what one launch takes"); }
  // the other kinds are what they were: a moment run still wants one shift per exposure, a trail at least one lag
  REFUSED(observed_run_checks(I.S, "trx_run_moments", ObservedRun::Moments, 2, sh.get(), out.get(), "mom", msg), TRX_E_ARG, "trx_run_moments: nshift 2 is not the observed set's nexp 3");
  REFUSED(observed_run_checks(I.S, "trx_run_trail", ObservedRun::Trail, 0, sh.get(), out.get(), "trail", msg), TRX_E_ARG, "trx_run_trail: nlag < 1");
}

static void layouts_and_extents()
{
  static_assert(kHpTile == kHpBlock * kHpOuts && kHpBlock % 64 == 0 && kHpTile >= 256 && kHpTile <= 1024, "the tile the kernel takes");
  const int64_t T = kHpTile;
  Heap<int64_t> seg{0, 1, 1, 1 + T, 2 + 2 * T, 2 + 2 * T, 19 + 4 * T};      // lengths 1, 0, T, T + 1, 0, 2 T + 17
  ProductState S; S.npix = seg[6]; S.nexp = 2; S.nseg = 6; S.seg = seg.get();
  Heap<double> taps{2.0, 1.0, 0.5, 0.25};
  trx_highpass hp{3, 0, taps.get()};
  std::string msg; HighpassLayout L;
  CHECK(highpass_layout(S, &hp, L, msg) == TRX_OK);
  CHECK(L.half == 3 && L.taps.size() == 4 && L.taps[3] == 0.25);
  CHECK(L.den_full == ((((((0.25 + 0.5) + 1.0) + 2.0) + 1.0) + 0.5) + 0.25));
  CHECK(L.tiles.size() == 1 + 1 + 2 + 3);
  // the tiles cover every segment exactly, in pixel order, and never cross one
  size_t t = 0;
  for (int32_t s = 0; s < S.nseg; s++) {
    int64_t p = seg[(size_t)s];
    while (p < seg[(size_t)s + 1]) {
      CHECK(t < L.tiles.size());
      if (t >= L.tiles.size()) return;
      const HpTile &X = L.tiles[t++];
      CHECK(X.first == p && X.seg_first == seg[(size_t)s] && X.seg_last == seg[(size_t)s + 1]);
      CHECK(X.count >= 1 && X.count <= kHpTile && X.first + X.count <= X.seg_last);
      CHECK(X.count == kHpTile || X.first + X.count == X.seg_last);      // (only a segment's last tile is short)
      p += X.count;
    }
    CHECK(p == seg[(size_t)s + 1]);
  }
  CHECK(t == L.tiles.size());
  CHECK(L.tiles.back().count == 17);
  // a set of empty segments only: no tile
  { Heap<int64_t> none{0, 0, 0}; ProductState E; E.npix = 1; E.nseg = 2; E.seg = none.get(); HighpassLayout M; CHECK(highpass_layout(E, &hp, M, msg) == TRX_OK && M.tiles.empty()); }
  // half = 0: one tap, den its value
  { trx_highpass h0{0, 0, taps.get()}; HighpassLayout M; CHECK(highpass_layout(S, &h0, M, msg) == TRX_OK && M.taps.size() == 1 && M.den_full == 2.0); }
  // extents at their exact sizes
  const HighpassExtents X = highpass_extents(800, 7, 13, 70);
  CHECK(X.pairs == 5600 && X.blocks == 91 && X.pair_bytes == 89600 && X.val_bytes == 44800 && X.lds_bytes == 16 * (size_t)(kHpTile + 140));
  const HighpassExtents Y = highpass_extents(81920, 201, 160, TRX_HIGHPASS_MAX_HALF);
  CHECK(Y.pairs == 16465920 && Y.blocks == 32160 && Y.pair_bytes == 263454720 && Y.lds_bytes == 16 * (size_t)(kHpTile + 2048) && Y.lds_bytes <= 65536);
  const HighpassExtents Z = highpass_extents(3000000000LL, 3, 1, 0);        // (past 2^31 pairs: 64-bit throughout)
  CHECK(Z.pairs == 9000000000LL && Z.pair_bytes == 144000000000ULL && Z.val_bytes == 72000000000ULL && Z.lds_bytes == 16 * (size_t)kHpTile);
}

int main(int argc, char **argv)
{
  if (argc == 4 && !std::strcmp(argv[1], "values")) return values_mode(argv[2], argv[3]);
  set_refusals();
  run_refusals();
  layouts_and_extents();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
