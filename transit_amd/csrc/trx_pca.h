// trx_pca.h -- the host side and the arithmetic of the principal-component detrend of the observed set on the device
// (trx_pca_observed, include/transit_hip.h): what the call refuses, the tournament schedule of its Jacobi sweeps, the
// rotation, the rank and sign rules, the tiles of the Gram kernel and the extents of its buffers, launches and LDS.  Plain
// C++ (no HIP): the kernels of hip/trx_pca.hip.h call the functions per lane, tests/pca_check.cpp runs the same source on
// the CPU over exact-size arrays.  Every operation is an IEEE double operation rounded once -- no fused multiply-add -- in
// the order transit_amd/xcor.py (pca_reference) writes it.
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>

#include "transit_hip.h"
#include "trx_numerics.h"
#include "trx_products.h"
#include "trx_sysrem.h"

namespace trx {

constexpr int kPcaBlock = 1024;                       // threads of the Jacobi block (one block per segment)
constexpr int kPcaGramTile = 4;                       // exposures a side of a Gram tile: 4 x 4 accumulators per lane
constexpr int kPcaGramWaves = 4;                      // Gram tiles per block, one wave each
constexpr size_t kPcaLdsMost = 160u * 1024u;          // what one workgroup may take of a CU's LDS

// ---- the call: checks --------------------------------------------------------------------------------
// Whether the call is the undo (pc NULL or ncomp = 0): trx_detrend_observed's undo.
inline bool pca_is_undo(const trx_pca *pc) { return !pc || pc->ncomp == 0; }

// What trx_pca_observed refuses, in the header's order.  The undo is checked for the observed set (and ncomp's sign) alone.
inline int pca_checks(const ProductState &S, const trx_pca *pc, const void *a, const void *o, int32_t nshift, const double *shift, std::string &msg)
{
  const char *const who = "trx_pca_observed";
  auto no = [&](int code, const std::string &what) { return refuse(msg, code, std::string(who) + ": " + what); };
  if (S.npix < 1 || !S.seg) return no(TRX_E_ARG, "no observed set installed (trx_set_observed)");
  if (!pc) return TRX_OK;
  if (pc->ncomp != 0 && S.nexp > TRX_PCA_MAX_EXP)
    return no(TRX_E_ARG, "the observed set's nexp " + std::to_string(S.nexp) + " is above TRX_PCA_MAX_EXP (" + std::to_string(TRX_PCA_MAX_EXP) + ")");
  if (pc->ncomp < 0) return no(TRX_E_ARG, "ncomp < 0");
  if (pc->ncomp > TRX_FILTER_MAX) return no(TRX_E_ARG, "ncomp above TRX_FILTER_MAX (" + std::to_string(TRX_FILTER_MAX) + ")");
  if (pc->ncomp > S.nexp) return no(TRX_E_ARG, "ncomp " + std::to_string(pc->ncomp) + " is above the observed set's nexp " + std::to_string(S.nexp));
  if (pc->ncomp == 0) return TRX_OK;
  if (pc->nsweep < 1) return no(TRX_E_ARG, "nsweep < 1");
  if (pc->nsweep > TRX_PCA_MAX_SWEEP) return no(TRX_E_ARG, "nsweep above TRX_PCA_MAX_SWEEP (" + std::to_string(TRX_PCA_MAX_SWEEP) + ")");
  return detrend_inject_checks(who, "xcor.pca_reference", S, pc->inject, pc->pad, pc->p0, pc->p1, a, o, nshift, shift, msg);
}

// ---- the schedule ------------------------------------------------------------------------------------
// m: nexp rounded up to even; a sweep has m - 1 rounds of m / 2 pairs
TRX_HD int pca_even(int nexp) { return nexp + (nexp & 1); }
TRX_HD int pca_rounds(int nexp) { return pca_even(nexp) - 1; }
TRX_HD int pca_pairs(int nexp) { return pca_even(nexp) / 2; }

// pair k = 0 .. m/2-1 of round t = 0 .. m-2 of the circle tournament: (m-1, t) for k = 0, ((t+k) mod (m-1), (t-k) mod (m-1))
// otherwise, ordered p < q; false where q is the dummy (q >= nexp): the pair is dropped
TRX_HD bool pca_pair(int nexp, int t, int k, int &p, int &q)
{
  const int m = pca_even(nexp), n1 = m - 1;
  const int a = k == 0 ? n1 : (t + k) % n1, b = k == 0 ? t : (t - k + n1) % n1;
  p = a < b ? a : b; q = a < b ? b : a;
  return q < nexp;
}

// ---- the rotation ------------------------------------------------------------------------------------
// (c, s) of the pair whose entries of A are app, aqq and apq; false where apq == 0: the pair is skipped
TRX_HD bool pca_rotation(double app, double aqq, double apq, double &c, double &s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  c = 1.0; s = 0.0;
  if (apq == 0.0) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
  c = 1.0 / std::sqrt(t * t + 1.0);
  s = t * c;
  return true;
}

// x <- c x - s y, y <- s x + c y, both old values read first; each product rounded, then the sum or difference
TRX_HD void pca_rotate(double &x, double &y, double c, double s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x0 = x, y0 = y;
  const double cx = c * x0, sy = s * y0, sx = s * x0, cy = c * y0;
  x = cx - sy;
  y = sx + cy;
}

// ---- after the last sweep ----------------------------------------------------------------------------
// the larger of m and x, a NaN x passed over: the fold of offdiag from +0 (a max: order-free)
TRX_HD double pca_absmax(double m, double x) { const double ax = std::fabs(x); return ax > m ? ax : m; }

// an eigenvalue that gives a component: > 0 and finite; the key it is ranked by: itself, or +0.  An INVALID eigenvalue --
// <= 0, +-inf or NaN -- therefore ranks as 0, behind every valid one: it gives the zero vector and eigen +0 wherever it
// stands, so the order of the invalid ones among themselves shows nowhere, and a NaN cannot make the count ambiguous.  This
// differs from a plain descending order only for +inf (last, not first), where V is non-finite and the call refuses anyway.
TRX_HD bool pca_valid(double lam) { return lam > 0.0 && lam <= 1.79769313486231570815e+308; }
TRX_HD double pca_key(double lam) { return pca_valid(lam) ? lam : 0.0; }
// whether eigenvalue k stands ahead of eigenvalue j: descending key, ties by ascending index (counted, as k_scatter_median)
TRX_HD bool pca_ahead(double lamk, int k, double lamj, int j)
{
  const double a = pca_key(lamk), b = pca_key(lamj);
  return a > b || (a == b && k < j);
}
// the index of the entry of largest magnitude of x [n] (stride apart), the first on ties: the one made positive
TRX_HD int pca_largest(const double *x, int n, int64_t stride)
{
  int at = 0; double best = -1.0;
  for (int v = 0; v < n; v++) {
    const double ax = std::fabs(x[(int64_t)v * stride]);
    if (ax > best) { best = ax; at = v; }
  }
  return at;
}

// an entry of a negated column: 0 - x, so that a zero entry stays +0
TRX_HD double pca_flip(double x) { return 0.0 - x; }

// ---- the Gram tiles ----------------------------------------------------------------------------------
// nb blocks of kPcaGramTile exposures; the nb (nb + 1) / 2 tiles (bv <= bu) in row-major order of bv
TRX_HD int pca_gram_blocks(int nexp) { return (nexp + kPcaGramTile - 1) / kPcaGramTile; }
TRX_HD int pca_gram_tiles(int nexp) { const int nb = pca_gram_blocks(nexp); return nb * (nb + 1) / 2; }
TRX_HD void pca_gram_tile(int nb, int k, int &bv, int &bu)
{
  bv = 0;
  while (k >= nb - bv) { k -= nb - bv; bv++; }
  bu = bv + k;
}

// ---- coefficients and residuals ----------------------------------------------------------------------
// one exposure's term of a coefficient: c += u * y
TRX_HD void pca_coef_term(double u, double y, double &c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m = u * y;
  c = c + m;
}

// ---- one column ---------------------------------------------------------------------------------------
// Whether a column is whole: its segment has a live exposure (live [nexp]) and the column's weight is > 0 at every live one.
// w: the column's weights (entry v at w[v * stride]), read only where hasw: the set has weights -- one answer for the whole
// launch; without: every w is 1.
TRX_HD bool pca_whole_column(const int32_t *live, const double *w, bool hasw, int64_t stride, int nexp)
{
  bool any = false, all = true;
  for (int v = 0; v < nexp; v++) {
    if (!live[v]) continue;
    any = true;
    if (hasw && !(w[(int64_t)v * stride] > 0.0)) all = false;
  }
  return any && all;
}

// The projection of one column on its segment's ncomp components U [nexp][ncomp]: the coefficients of all components (v
// ascending; a masked entry counts as +0) to coef[i * stride], then the residuals in place in r (entry v at r[v * stride]; i
// ascending per entry).  w, hasw: as above.
TRX_HD void pca_project_column(double *r, const double *w, bool hasw, const double *U, double *coef, int64_t stride, int nexp, int ncomp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double c[TRX_FILTER_MAX];
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < TRX_FILTER_MAX; i++) c[i] = 0.0;
  for (int v = 0; v < nexp; v++) {
    const double f = r[(int64_t)v * stride];
    const double y = !hasw || w[(int64_t)v * stride] > 0.0 ? f : 0.0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < TRX_FILTER_MAX; i++)
      if (i < ncomp) pca_coef_term(U[(int64_t)v * ncomp + i], y, c[i]);
  }
#if defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < TRX_FILTER_MAX; i++)
    if (i < ncomp) coef[(int64_t)i * stride] = c[i];
  for (int v = 0; v < nexp; v++) {
    double x = r[(int64_t)v * stride];
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < TRX_FILTER_MAX; i++)
      if (i < ncomp) x = sysrem_subtract(x, U[(int64_t)v * ncomp + i], c[i]);
    r[(int64_t)v * stride] = x;
  }
}

// ---- extents -----------------------------------------------------------------------------------------
// The extents of a call of ncomp components over nexp exposures, nseg segments, npix pixels and ntiles tiles: the
// residuals r [nexp][npix], coef [ncomp][npix], U [nseg][nexp][ncomp], the Gram matrices G and the transposed eigenvector
// matrices Vt [nseg][nexp][nexp] each, the live flags [nseg][nexp] and the whole flags [npix] (int32), eigen [nseg][ncomp],
// offdiag [nseg], nwhole [nseg] (int64); the blocks of the element-wise kernel, of the live kernel (rows_per_block rows
// (v, s) each), of the tile kernels (tiles_per_block each), of the Gram kernel (kPcaGramWaves tiles each) and of the Jacobi
// kernel (one per segment); the row stride of A in LDS (odd: a column's entries fall on different banks) and the LDS bytes
// of the Jacobi block: A, the round's (c, s), the eigenvalues and the rows' maxima, the waves' counts, the round's pairs.
struct PcaExtents {
  int64_t cells = 0, rows = 0, elem_blocks = 0, row_blocks = 0, tile_blocks = 0, gram_tiles = 0, gram_blocks = 0, jacobi_blocks = 0;
  int32_t stride = 0, npairs = 0, nrounds = 0;
  size_t r_bytes = 0, c_bytes = 0, coef_bytes = 0, basis_bytes = 0, g_bytes = 0, live_bytes = 0, whole_bytes = 0, eigen_bytes = 0, offdiag_bytes = 0,
         nwhole_bytes = 0, lds_bytes = 0;
  bool grid_ok = false;
};
inline PcaExtents pca_extents(int64_t npix, int32_t nexp, int32_t nseg, int32_t ncomp, int64_t ntiles, int elem_block, int tiles_per_block, int rows_per_block)
{
  PcaExtents X;
  const FillExtents F = fill_extents(npix, nexp, elem_block);
  X.cells = F.cells; X.elem_blocks = F.elem_blocks; X.r_bytes = F.r_bytes; X.c_bytes = F.c_bytes;
  X.rows = (int64_t)nexp * nseg;
  X.row_blocks = (X.rows + rows_per_block - 1) / rows_per_block;
  X.tile_blocks = (ntiles + tiles_per_block - 1) / tiles_per_block;
  X.gram_tiles = (int64_t)pca_gram_tiles(nexp) * nseg;
  X.gram_blocks = (X.gram_tiles + kPcaGramWaves - 1) / kPcaGramWaves;
  X.jacobi_blocks = nseg;
  X.stride = nexp | 1; X.npairs = pca_pairs(nexp); X.nrounds = pca_rounds(nexp);
  X.coef_bytes = sizeof(double) * (size_t)ncomp * (size_t)npix;
  X.basis_bytes = sizeof(double) * (size_t)X.rows * (size_t)ncomp;
  X.g_bytes = sizeof(double) * (size_t)X.rows * (size_t)nexp;
  X.live_bytes = sizeof(int32_t) * (size_t)X.rows;
  X.whole_bytes = sizeof(int32_t) * (size_t)npix;
  X.eigen_bytes = sizeof(double) * (size_t)nseg * (size_t)ncomp;
  X.offdiag_bytes = sizeof(double) * (size_t)nseg;
  X.nwhole_bytes = sizeof(int64_t) * (size_t)nseg;
  X.lds_bytes = sizeof(double) * ((size_t)nexp * (size_t)X.stride + 2 * (size_t)X.npairs + 2 * (size_t)nexp + (size_t)(kPcaBlock / 64)) +
                sizeof(int32_t) * 2 * (size_t)X.npairs;
  auto ok = [](int64_t b) { return b >= 1 && b <= 0x7fffffffLL; };
  X.grid_ok = ok(X.elem_blocks) && ok(X.row_blocks) && ok(X.tile_blocks) && ok(X.gram_blocks) && ok(X.jacobi_blocks) && X.lds_bytes <= kPcaLdsMost;
  return X;
}

}  // namespace trx
