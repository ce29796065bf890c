// pca_check.cpp -- the host side and the arithmetic of the principal-component detrend of the observed set
// (trx_pca_observed) on the CPU: the refusals, the extents, the tournament schedule, the Gram tiles and the arithmetic
// functions of transit_amd/csrc/trx_pca.h.  The same source the library compiles; every buffer is a heap block of EXACTLY
// its extent, addressed the way the kernels of hip/trx_pca.hip.h address theirs (row by row and lane by lane for the live
// kernel, tile by tile for the column kernels, Gram tile by Gram tile with the lane sums through the butterfly, item by item
// for the Jacobi block's phases over a block of LDS of the extents' size), so that an index outside one is an error under
// -fsanitize=address here and not a fault on the device.
//
//   pca_check                     the program's own checks: the refusal table in the header's order, the extents, the
//                                 schedule, the Gram tiles, sets whose result is known; prints "ok N" (N checks) or FAILED lines
//   pca_check set FILE            FILE: "nexp ncomp nsweep nseg hasw", the nseg + 1 segment bounds, then the doubles (C99 hex)
//                                 of the data [nexp][npix] and, with hasw = 1, the weights [nexp][npix].  Runs the call's step
//                                 2 over the whole set the way the device walks it and prints "U" and its [nseg][nexp][ncomp]
//                                 entries, "coef" [ncomp][npix], "r" [nexp][npix], "eigen" [nseg][ncomp], "offdiag" [nseg] as
//                                 C99 hex and "nwhole" [nseg] as integers
#include <cstdint>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "trx_pca.h"
#include "check_common.h"

using namespace trx;

constexpr int kElemBlock = 256, kTileWaves = 4, kRowWaves = 4;      // kPixBlock, kFiltWaves, kMomWaves

// ---- the refusal table, in the header's order --------------------------------------------------------
static void refusals()
{
  Heap<int64_t> seg{0, 2, 6};
  ProductState S; S.npix = 6; S.nexp = 3; S.nseg = 2; S.seg = seg.get();
  const int atm = 0, opts = 0;                           // (the checks look at the addresses only)
  Heap<double> shift{1.0, 1.0, 1.0};
  trx_pca D{2, 8, 0, 0, 0.0, 0.0};
  ACCEPTED(pca_checks(S, &D, nullptr, nullptr, 0, nullptr, msg));
  ACCEPTED(pca_checks(S, nullptr, nullptr, nullptr, 0, nullptr, msg));                     // the undo
  trx_pca I{3, TRX_PCA_MAX_SWEEP, 1, 0, 1e-3, 1.0};
  ACCEPTED(pca_checks(S, &I, &atm, &opts, 3, shift.get(), msg));
  CHECK(pca_is_undo(nullptr) && !pca_is_undo(&D));
  // every later fault at once: the first in the order is the one named
  trx_pca bad{-1, 0, 2, 1, kNaN, kInf};
  ProductState N = S; N.seg = nullptr; N.nexp = N.nseg = 0; N.windowed = true;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: no observed set installed (trx_set_observed)");
  REFUSED(pca_checks(N, nullptr, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: no observed set installed (trx_set_observed)");
  N = S; N.npix = 0;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: no observed set installed (trx_set_observed)");
  N = S; N.windowed = true; N.nexp = TRX_PCA_MAX_EXP + 1;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: the observed set's nexp 129 is above TRX_PCA_MAX_EXP (128)");
  bad.ncomp = 0;                                         // the undo of a set too long for the fit is the undo
  ACCEPTED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg));
  bad.ncomp = -1; N.nexp = TRX_PCA_MAX_EXP;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: ncomp < 0");
  bad.ncomp = TRX_FILTER_MAX + 1;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: ncomp above TRX_FILTER_MAX (16)");
  N.nexp = 3; bad.ncomp = 4;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: ncomp 4 is above the observed set's nexp 3");
  bad.ncomp = 0;                                         // the undo: nothing else is looked at
  ACCEPTED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg));
  CHECK(pca_is_undo(&bad));
  bad.ncomp = 3;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: nsweep < 1");
  bad.nsweep = TRX_PCA_MAX_SWEEP + 1;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: nsweep above TRX_PCA_MAX_SWEEP (32)");
  bad.nsweep = 1;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: inject must be 0 or 1");
  bad.inject = 1;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: pad must be 0");
  bad.pad = 0;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: p0 must be finite");
  bad.p0 = 0.5;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: p1 must be finite");
  bad.p1 = 1.0;
  REFUSED(pca_checks(N, &bad, nullptr, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: a is NULL");
  REFUSED(pca_checks(N, &bad, &atm, nullptr, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: o is NULL");
  REFUSED(pca_checks(N, &bad, &atm, &opts, 0, nullptr, msg), TRX_E_ARG, "trx_pca_observed: shift is NULL");
  REFUSED(pca_checks(N, &bad, &atm, &opts, 4, shift.get(), msg), TRX_E_ARG, "trx_pca_observed: nshift 4 is not the observed set's nexp 3");
  shift[2] = -1.0;
  REFUSED(pca_checks(N, &bad, &atm, &opts, 3, shift.get(), msg), TRX_E_ARG, "trx_pca_observed: shift 2 must be finite and > 0");
  shift[2] = 1.0;
  // the last: a shard of the grid, with and without an injection
  REFUSED(pca_checks(N, &bad, &atm, &opts, 3, shift.get(), msg), TRX_E_UNSUPPORTED,
          "trx_pca_observed: this handle's shard is not the whole grid; detrend on the host (xcor.pca_reference)");
  REFUSED(pca_checks(N, &D, nullptr, nullptr, 0, nullptr, msg), TRX_E_UNSUPPORTED,
          "trx_pca_observed: this handle's shard is not the whole grid; detrend on the host (xcor.pca_reference)");
  ACCEPTED(pca_checks(S, &bad, &atm, &opts, 3, shift.get(), msg));
  // without an injection a, o, shift and the p's are not looked at
  trx_pca plain{1, 1, 0, 0, kNaN, kInf};
  ACCEPTED(pca_checks(S, &plain, nullptr, nullptr, -5, nullptr, msg));
  // the non-finite component names this call
  Heap<double> U(2 * 3 * 2, 0.25);
  ACCEPTED(sysrem_basis_check(U.get(), 2, 3, 2, msg, "trx_pca_observed"));
  U[10] = kNaN;
  REFUSED(sysrem_basis_check(U.get(), 2, 3, 2, msg, "trx_pca_observed"), TRX_E_ARG, "trx_pca_observed: component 0 of segment 1 is not finite");
}

// ---- the extents -----------------------------------------------------------------------------------------
static void extents()
{
  PcaExtents X = pca_extents(800, 1, 8, 1, 16, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.cells == 800 && X.rows == 8 && X.elem_blocks == 4 && X.row_blocks == 2 && X.tile_blocks == 4 && X.gram_tiles == 8 && X.gram_blocks == 2);
  CHECK(X.stride == 1 && X.npairs == 1 && X.nrounds == 1 && X.jacobi_blocks == 8 && X.g_bytes == 8u * 8 && X.grid_ok);
  CHECK(X.lds_bytes == 8u * (1 + 2 + 2 + 16) + 8u);
  X = pca_extents(800, 2, 8, 2, 16, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.stride == 3 && X.npairs == 1 && X.nrounds == 1 && X.gram_tiles == 8 && X.lds_bytes == 8u * (6 + 2 + 4 + 16) + 8u && X.grid_ok);
  X = pca_extents(800, 7, 8, 3, 16, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.cells == 5600 && X.rows == 56 && X.elem_blocks == 22 && X.row_blocks == 14 && X.tile_blocks == 4 && X.gram_tiles == 3 * 8 && X.gram_blocks == 6);
  CHECK(X.stride == 7 && X.npairs == 4 && X.nrounds == 7 && X.lds_bytes == 8u * (49 + 8 + 14 + 16) + 32u && X.grid_ok);
  CHECK(X.r_bytes == 8u * 5600 && X.c_bytes == 8u * 800 && X.coef_bytes == 8u * 3 * 800 && X.basis_bytes == 8u * 56 * 3 && X.g_bytes == 8u * 56 * 7);
  CHECK(X.live_bytes == 4u * 56 && X.whole_bytes == 4u * 800 && X.eigen_bytes == 8u * 8 * 3 && X.offdiag_bytes == 8u * 8 && X.nwhole_bytes == 8u * 8);
  X = pca_extents(81920, 128, 40, 16, 1280, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.stride == 129 && X.npairs == 64 && X.nrounds == 127 && X.gram_tiles == 528 * 40 && X.gram_blocks == 5280 && X.jacobi_blocks == 40);
  CHECK(X.lds_bytes == 8u * (128 * 129 + 128 + 256 + 16) + 512u && X.lds_bytes <= kPcaLdsMost && X.grid_ok);
  CHECK(X.g_bytes == (size_t)8 * 40 * 128 * 128);
  // one exposure past the cap: the Jacobi block's LDS still fits, the refusal is pca_checks'
  X = pca_extents(81920, 129, 40, 16, 1280, kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.stride == 129 && X.npairs == 65 && X.nrounds == 129 && X.lds_bytes == 8u * (129 * 129 + 130 + 258 + 16) + 520u);
  // a grid above what a launch takes
  X = pca_extents(0x7fffffffLL * 300, 100, 1, 5, 10, kElemBlock, kTileWaves, kRowWaves);
  CHECK(!X.grid_ok);
}

// ---- the schedule and the Gram tiles --------------------------------------------------------------------
static void schedule()
{
  for (const int nexp : {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 64, 65, 127, 128}) {
    std::set<std::pair<int, int>> seen; bool ok = true; int64_t n = 0;
    for (int t = 0; t < pca_rounds(nexp); t++) {
      std::vector<int> used((size_t)nexp, 0);
      for (int k = 0; k < pca_pairs(nexp); k++) {
        int p, q;
        const bool in = pca_pair(nexp, t, k, p, q);
        ok = ok && p >= 0 && p < q && q <= pca_even(nexp) - 1 && in == (q < nexp);
        if (!in) continue;
        ok = ok && !used[(size_t)p] && !used[(size_t)q] && seen.insert({p, q}).second;      // disjoint in the round, once a sweep
        used[(size_t)p] = used[(size_t)q] = 1; n++;
      }
    }
    CHECK(ok && n == (int64_t)nexp * (nexp - 1) / 2 && (int64_t)seen.size() == n);
    // the Gram tiles: every (bv <= bu) once, in order
    const int nb = pca_gram_blocks(nexp); int k = 0; bool tiles_ok = nb == (nexp + 3) / 4;
    for (int bv = 0; bv < nb; bv++)
      for (int bu = bv; bu < nb; bu++, k++) { int a, b; pca_gram_tile(nb, k, a, b); tiles_ok = tiles_ok && a == bv && b == bu; }
    CHECK(tiles_ok && k == pca_gram_tiles(nexp));
  }
  // the rotation: a skipped pair, a known angle (app = aqq: theta = 0, t = 1, c = s = 1 / sqrt 2), the rotation itself
  double c, s;
  CHECK(!pca_rotation(1.0, 2.0, 0.0, c, s) && !pca_rotation(1.0, 2.0, -0.0, c, s));
  CHECK(pca_rotation(3.0, 3.0, 0.5, c, s) && c == 1.0 / std::sqrt(2.0) && s == c);
  CHECK(pca_rotation(3.0, 3.0, -0.5, c, s) && s == c);                                      // (theta = -0: >= 0)
  CHECK(pca_rotation(1.0, 0.0, 1e-300, c, s) && c == 1.0 && s == 0.0 - 0.0);               // (theta overflows: t = 0)
  double x = 1.0, y = 2.0;
  pca_rotate(x, y, 0.5, 0.25);
  CHECK(x == 0.0 && y == 1.25);
  // rank and sign
  CHECK(pca_valid(1e-300) && !pca_valid(0.0) && !pca_valid(-1.0) && !pca_valid(kInf) && !pca_valid(kNaN));
  CHECK(pca_ahead(2.0, 3, 1.0, 0) && !pca_ahead(1.0, 0, 2.0, 3) && pca_ahead(1.0, 0, 1.0, 1) && !pca_ahead(1.0, 1, 1.0, 0) && !pca_ahead(1.0, 1, 1.0, 1));
  CHECK(pca_ahead(1e-9, 5, -3.0, 0) && pca_ahead(kNaN, 0, -1.0, 1) && !pca_ahead(kNaN, 1, -1.0, 0) && !pca_ahead(kInf, 1, 1.0, 0));
  Heap<double> col{0.5, -2.0, 2.0, -1.0};
  CHECK(pca_largest(col.get(), 4, 1) == 1 && pca_largest(col.get(), 2, 2) == 1 && pca_largest(col.get(), 1, 1) == 0);
  CHECK(pca_absmax(0.0, -3.0) == 3.0 && pca_absmax(4.0, -3.0) == 4.0 && pca_absmax(4.0, kNaN) == 4.0);
}

// ---- the whole set, the way the device walks it ---------------------------------------------------------
struct SetResult { Heap<double> U, coef, r, eigen, offdiag; Heap<int64_t> nwhole; };

static SetResult run_set(const ProductState &S, int ncomp, int nsweep, const double *data, const double *weight)
{
  std::string msg;
  std::vector<FilterTile> tiles;
  CHECK(sysrem_tiles(S, tiles, msg) == TRX_OK);
  const PcaExtents X = pca_extents(S.npix, S.nexp, S.nseg, ncomp, (int64_t)tiles.size(), kElemBlock, kTileWaves, kRowWaves);
  CHECK(X.grid_ok);
  const int64_t npix = S.npix; const int nexp = S.nexp, nseg = S.nseg;
  SetResult R{Heap<double>(X.basis_bytes / 8, -7.0), Heap<double>(X.coef_bytes / 8, -7.0), Heap<double>(X.r_bytes / 8), Heap<double>(X.eigen_bytes / 8, -7.0),
              Heap<double>(X.offdiag_bytes / 8, -7.0), Heap<int64_t>(X.nwhole_bytes / 8, -7)};
  Heap<int32_t> live(X.live_bytes / 4, -7), whole(X.whole_bytes / 4, -7);
  Heap<double> G(X.g_bytes / 8, -7.0), Vt(X.g_bytes / 8, -7.0);
  double *const r = R.r.get();
  for (int64_t k = 0; k < X.cells; k++) r[k] = data[k];
  // k_pca_live: one wave per (v, s), trips of 64 pixels
  for (int64_t row = 0; row < X.rows; row++) {
    const int64_t v = row / nseg, s = row - v * nseg, first = S.seg[s], last = S.seg[s + 1];
    bool any = false;
    if (!weight) any = last > first;
    else
      for (int64_t p0 = first; p0 < last && !any; p0 += 64)
        for (int lane = 0; lane < 64; lane++) { const int64_t q = p0 + lane; if (q < last && weight[v * npix + q] > 0.0) any = true; }
    live[(size_t)(s * nexp + v)] = any ? 1 : 0;
  }
  // k_pca_whole: one lane per column of a tile
  for (const FilterTile &T : tiles)
    for (int lane = 0; lane < T.count; lane++) {
      const int64_t p = T.first + lane;
      whole[(size_t)p] = pca_whole_column(live.get() + (int64_t)T.seg * nexp, weight ? weight + p : nullptr, weight != nullptr, npix, nexp) ? 1 : 0;
    }
  // k_pca_gram: one wave per tile of 4 x 4 entries, the lanes' sums through the butterfly
  const int nb = pca_gram_blocks(nexp), per = pca_gram_tiles(nexp);
  for (int64_t tile = 0; tile < X.gram_tiles; tile++) {
    const int64_t s = tile / per, first = S.seg[s], last = S.seg[s + 1];
    int bv, bu;
    pca_gram_tile(nb, (int)(tile - s * per), bv, bu);
    for (int a = 0; a < kPcaGramTile; a++)
      for (int b = 0; b < kPcaGramTile; b++) {
        const int v = bv * kPcaGramTile + a, u = bu * kPcaGramTile + b;
        const int vr = std::min(v, nexp - 1), ur = std::min(u, nexp - 1);      // (a row past the end reads the last one again)
        double acc[64];
        for (int lane = 0; lane < 64; lane++) {
          acc[lane] = 0.0;
          for (int64_t p = first + lane; p < last; p += 64) {
            const bool w = whole[(size_t)p] != 0;
            const double xv = w && live[(size_t)(s * nexp + vr)] ? r[(int64_t)vr * npix + p] : 0.0;
            const double xu = w && live[(size_t)(s * nexp + ur)] ? r[(int64_t)ur * npix + p] : 0.0;
            const double m = xv * xu;
            acc[lane] = acc[lane] + m;
          }
        }
        const double g = sysrem_wave_sum_host(acc);
        if (u >= v && u < nexp) { G[(size_t)((s * nexp + v) * nexp + u)] = g; G[(size_t)((s * nexp + u) * nexp + v)] = g; }
      }
  }
  // k_pca_jacobi: one block per segment over its LDS, the phases item by item
  const int stride = X.stride, npairs = X.npairs, items = npairs * nexp;
  for (int64_t s = 0; s < nseg; s++) {
    Heap<double> lds(X.lds_bytes / 8, -7.0);             // (the pairs' integers are the last npairs doubles' bytes)
    double *const M = lds.get(), *const cs = M + (size_t)nexp * stride, *const lam = cs + 2 * npairs, *const rowmax = lam + nexp;
    int *const pq = (int *)(rowmax + nexp + kPcaBlock / 64);
    const double *const Gs = G.get() + s * nexp * nexp;
    double *const V = Vt.get() + s * nexp * nexp;
    for (int w = 0; w < nexp * nexp; w++) { const int i = w / nexp, j = w - i * nexp; M[i * stride + j] = Gs[w]; V[w] = i == j ? 1.0 : 0.0; }
    int64_t n = 0;
    for (int64_t p = S.seg[s]; p < S.seg[s + 1]; p++) n += whole[(size_t)p] != 0;
    R.nwhole[(size_t)s] = n;
    for (int sweep = 0; sweep < nsweep; sweep++)
      for (int t = 0; t < X.nrounds; t++) {
        for (int k = 0; k < npairs; k++) {
          int p, q; double c = 0.0, sn = 0.0;
          if (pca_pair(nexp, t, k, p, q)) { if (!pca_rotation(M[p * stride + p], M[q * stride + q], M[p * stride + q], c, sn)) c = 0.0; }
          else p = q = 0;
          pq[2 * k] = p; pq[2 * k + 1] = q; cs[2 * k] = c; cs[2 * k + 1] = sn;
        }
        for (int w = 0; w < items; w++) {
          const int k = w / nexp, i = w - k * nexp;
          const double c = cs[2 * k], sn = cs[2 * k + 1];
          if (c == 0.0) continue;
          const int p = pq[2 * k], q = pq[2 * k + 1];
          pca_rotate(M[i * stride + p], M[i * stride + q], c, sn);
          pca_rotate(V[p * nexp + i], V[q * nexp + i], c, sn);
        }
        for (int w = 0; w < items; w++) {
          const int k = w / nexp, j = w - k * nexp;
          const double c = cs[2 * k], sn = cs[2 * k + 1];
          if (c == 0.0) continue;
          const int p = pq[2 * k], q = pq[2 * k + 1];
          double x = M[p * stride + j], y = M[q * stride + j];
          pca_rotate(x, y, c, sn);
          M[p * stride + j] = j == q ? 0.0 : x; M[q * stride + j] = j == p ? 0.0 : y;
        }
      }
    for (int i = 0; i < nexp; i++) {
      lam[i] = M[i * stride + i];
      double mx = 0.0;
      for (int q = i + 1; q < nexp; q++) mx = pca_absmax(mx, M[i * stride + q]);
      rowmax[i] = mx;
    }
    double mx = 0.0;
    for (int i = 0; i < nexp; i++) mx = pca_absmax(mx, rowmax[i]);
    R.offdiag[(size_t)s] = mx;
    for (int j = 0; j < nexp; j++) {
      int rank = 0;
      for (int k = 0; k < nexp; k++) rank += pca_ahead(lam[k], k, lam[j], j) ? 1 : 0;
      if (rank >= ncomp) continue;
      const double *const col = V + j * nexp;
      const bool valid = pca_valid(lam[j]);
      const bool neg = valid && col[pca_largest(col, nexp, 1)] < 0.0;
      for (int v = 0; v < nexp; v++) R.U[(size_t)((s * nexp + v) * ncomp + rank)] = !valid ? 0.0 : neg ? pca_flip(col[v]) : col[v];
      R.eigen[(size_t)(s * ncomp + rank)] = valid ? lam[j] : 0.0;
    }
  }
  // k_pca_project: one lane per column of a tile
  for (const FilterTile &T : tiles)
    for (int lane = 0; lane < T.count; lane++) {
      const int64_t p = T.first + lane;
      pca_project_column(r + p, weight ? weight + p : nullptr, weight != nullptr, R.U.get() + (int64_t)T.seg * nexp * ncomp, R.coef.get() + p, npix, nexp, ncomp);
    }
  return R;
}

// ---- results known exactly or nearly ----------------------------------------------------------------------
static bool plus_zero(double x) { return x == 0.0 && !std::signbit(x); }

static void known()
{
  // one segment, four equal rows (2, 4, 8): G = 84 everywhere, one eigenvalue 336 with the vector (1/2, 1/2, 1/2, 1/2)
  Heap<int64_t> seg{0, 3};
  ProductState S; S.npix = 3; S.nexp = 4; S.nseg = 1; S.seg = seg.get();
  Heap<double> data{2.0, 4.0, 8.0,  2.0, 4.0, 8.0,  2.0, 4.0, 8.0,  2.0, 4.0, 8.0};
  SetResult R = run_set(S, 2, 8, data.get(), nullptr);
  CHECK(R.nwhole[0] == 3 && std::fabs(R.eigen[0] - 336.0) < 1e-11 && R.offdiag[0] < 1e-11);
  bool half = true, small = true;
  for (int v = 0; v < 4; v++) half = half && std::fabs(R.U[(size_t)(2 * v)] - 0.5) < 1e-14;
  for (size_t k = 0; k < R.r.n; k++) small = small && std::fabs(R.r[k]) < 1e-13;
  CHECK(half && small && std::fabs(R.coef[0] - 4.0) < 1e-13 && std::fabs(R.coef[2] - 16.0) < 1e-13);
  // masked everywhere: no live exposure, no whole column, zero vectors, the data as they were
  Heap<double> w0(12, 0.0);
  SetResult R0 = run_set(S, 2, 2, data.get(), w0.get());
  bool same = true, zero = true;
  for (size_t k = 0; k < R0.r.n; k++) same = same && R0.r[k] == data[k];
  for (size_t k = 0; k < R0.U.n; k++) zero = zero && plus_zero(R0.U[k]);
  for (size_t k = 0; k < R0.coef.n; k++) zero = zero && R0.coef[k] == 0.0;
  CHECK(same && zero && R0.nwhole[0] == 0 && plus_zero(R0.eigen[0]) && plus_zero(R0.eigen[1]) && plus_zero(R0.offdiag[0]));
  // an exposure masked over the whole segment: its row of every vector is +0, its residuals are its data; the others as without it
  Heap<double> w1{1.0, 1.0, 1.0,  0.0, 0.0, 0.0,  1.0, 1.0, 1.0,  1.0, 1.0, 1.0};
  Heap<double> d1{2.0, 4.0, 8.0,  5.0, 6.0, 7.0,  2.0, 4.0, 8.0,  2.0, 4.0, 8.0};
  SetResult R1 = run_set(S, 2, 8, d1.get(), w1.get());
  CHECK(R1.nwhole[0] == 3 && plus_zero(R1.U[2]) && plus_zero(R1.U[3]) && R1.r[3] == 5.0 && R1.r[4] == 6.0 && R1.r[5] == 7.0);
  CHECK(std::fabs(R1.U[0] - 1.0 / std::sqrt(3.0)) < 1e-14 && std::fabs(R1.eigen[0] - 252.0) < 1e-11);
  // every column with a hole: nothing is whole, zero vectors, the data stay
  Heap<double> w2{0.0, 1.0, 1.0,  1.0, 0.0, 1.0,  1.0, 1.0, 0.0,  1.0, 1.0, 1.0};
  SetResult R2 = run_set(S, 2, 4, data.get(), w2.get());
  zero = same = true;
  for (size_t k = 0; k < R2.U.n; k++) zero = zero && plus_zero(R2.U[k]);
  for (size_t k = 0; k < R2.r.n; k++) same = same && R2.r[k] == data[k];
  CHECK(R2.nwhole[0] == 0 && zero && same);
  // a masked column beside whole ones: its coefficient is +0 and it keeps its data
  Heap<double> w3{1.0, 0.0, 1.0,  1.0, 0.0, 1.0,  1.0, 0.0, 1.0,  1.0, 0.0, 1.0};
  SetResult R3 = run_set(S, 1, 8, data.get(), w3.get());
  CHECK(R3.nwhole[0] == 2 && R3.coef[1] == 0.0 && R3.r[1] == 4.0 && R3.r[10] == 4.0 && std::fabs(R3.eigen[0] - 272.0) < 1e-11);
  // an empty segment between two: zero vectors, nothing of it read or written; one exposure alone
  Heap<int64_t> seg3{0, 3, 3, 6};
  ProductState E; E.npix = 6; E.nexp = 4; E.nseg = 3; E.seg = seg3.get();
  Heap<double> d3(24);
  for (int v = 0; v < 4; v++) for (int p = 0; p < 6; p++) d3[(size_t)(v * 6 + p)] = data[(size_t)(v * 3 + p % 3)];
  SetResult R4 = run_set(E, 1, 8, d3.get(), nullptr);
  CHECK(std::fabs(R4.U[0] - 0.5) < 1e-14 && plus_zero(R4.U[4]) && plus_zero(R4.U[7]) && std::fabs(R4.U[8] - 0.5) < 1e-14 && R4.nwhole[1] == 0 && plus_zero(R4.eigen[1]));
  ProductState One; One.npix = 3; One.nexp = 1; One.nseg = 1; One.seg = seg.get();
  SetResult R5 = run_set(One, 1, 1, data.get(), nullptr);
  CHECK(R5.U[0] == 1.0 && R5.eigen[0] == 84.0 && R5.coef[0] == 2.0 && R5.r[0] == 0.0 && R5.r[2] == 0.0 && plus_zero(R5.offdiag[0]));
}

int main(int argc, char **argv)
{
  if (argc == 3 && !std::strcmp(argv[1], "set")) {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) { std::perror(argv[2]); return 2; }
    int nexp, ncomp, nsweep, nseg, hasw;
    if (std::fscanf(f, "%d %d %d %d %d", &nexp, &ncomp, &nsweep, &nseg, &hasw) != 5 || nexp < 1 || nseg < 1) {
      std::fprintf(stderr, "pca_check: bad header\n"); return 2;
    }
    Heap<int64_t> seg((size_t)nseg + 1);
    for (int s = 0; s <= nseg; s++) {
      long long x;
      if (std::fscanf(f, "%lld", &x) != 1) { std::fprintf(stderr, "pca_check: bad segment bounds\n"); return 2; }
      seg[(size_t)s] = x;
    }
    const size_t npix = (size_t)seg[(size_t)nseg];
    const auto data = read_doubles(f, (size_t)nexp * npix);
    std::unique_ptr<double[]> w;
    if (hasw) w = read_doubles(f, (size_t)nexp * npix);
    std::fclose(f);
    ProductState S; S.npix = (int64_t)npix; S.nexp = nexp; S.nseg = nseg; S.seg = seg.get();
    const trx_pca D{ncomp, nsweep, 0, 0, 0.0, 0.0};
    std::string msg;
    if (pca_checks(S, &D, nullptr, nullptr, 0, nullptr, msg) != TRX_OK || ncomp < 1) { std::fprintf(stderr, "pca_check: %s\n", msg.c_str()); return 2; }
    const SetResult R = run_set(S, ncomp, nsweep, data.get(), w.get());
    print_doubles("U", R.U); print_doubles("coef", R.coef); print_doubles("r", R.r); print_doubles("eigen", R.eigen); print_doubles("offdiag", R.offdiag);
    std::printf("nwhole");
    for (size_t k = 0; k < R.nwhole.n; k++) std::printf(" %lld", (long long)R.nwhole[k]);
    std::printf("\n");
    if (g_bad) return 1;
    return 0;
  }
  if (argc != 1) { std::fprintf(stderr, "usage: pca_check [set FILE]\n"); return 2; }
  refusals();
  extents();
  schedule();
  known();
  if (g_bad) { std::printf("FAILED %d of %d checks\n", g_bad, g_checks); return 1; }
  std::printf("ok %d\n", g_checks);
  return 0;
}
