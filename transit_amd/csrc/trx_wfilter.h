// trx_wfilter.h -- the host side and the arithmetic of the weighted detrending filter (trx_set_weighted_filter,
// include/transit_hip.h): what the call refuses, the layout the device gets, the extents of its buffers, and the per-column
// arithmetic -- the normal matrix, its factor and the solve -- as plain host/device functions.  Plain C++ (no HIP): the
// kernels of hip/trx_wfilter.hip.h call the functions per lane, tests/wfilter_check.cpp runs the same source on the CPU over
// exact-size arrays.  Every operation is an IEEE double operation rounded once -- no fused multiply-add -- in the order
// transit_amd/xcor.py (weighted_factor, weighted_filter_reference) writes it.
//
// A column's factor is the L D L^T factor of its normal matrix N = U^T diag(w) U of the REAL ncomp components, kept as
// nfac = ncomp (ncomp + 1) / 2 doubles: entry wfilter_at(j, k) is L_jk for k < j and D_j for k = j.  The device keeps the
// factors component-major, [nfac][npix]: entry e of column p at fac[e * npix + p], so that a wave's loads are coalesced;
// here a column's factor is addressed as fac[e * stride].  The functions are templates over the padded component count NC
// (4, 8 or 16) so that a kernel's arrays stay in registers; a padded component j >= n is never read from the factor,
// takes no part in a pivot and gets the coefficient +0.
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "transit_hip.h"
#include "trx_columns.h"
#include "trx_numerics.h"
#include "trx_products.h"

namespace trx {

// ---- the set: checks, layout, extents --------------------------------------------------------------
// a weighted filter that is not a clearing call (f non-null, ncomp != 0)
inline int wfilter_set_checks(const ProductState &S, const trx_wfilter *f, std::string &msg)
{
  if (S.npix < 1 || !S.seg) return refuse(msg, TRX_E_ARG, "weighted filter: no observed set installed (trx_set_observed)");
  if (f->ncomp < 0) return refuse(msg, TRX_E_ARG, "weighted filter: ncomp < 0");
  if (f->ncomp > TRX_FILTER_MAX) return refuse(msg, TRX_E_ARG, "weighted filter: ncomp above TRX_FILTER_MAX (" + std::to_string(TRX_FILTER_MAX) + ")");
  if (!f->basis) return refuse(msg, TRX_E_ARG, "weighted filter: NULL basis array");
  const size_t per = (size_t)f->ncomp * (size_t)S.nexp;
  for (int32_t s = 0; s < S.nseg; s++)
    for (size_t k = 0; k < per; k++)
      if (!std::isfinite(f->basis[(size_t)s * per + k])) return refuse(msg, TRX_E_ARG, "weighted filter: segment " + std::to_string(s) + ": basis entry must be finite");
  return TRX_OK;
}

// What the device gets of a checked weighted filter over the observed set of S: the basis exposure-major [nseg][nexp][npad],
// zero-padded to the kernel's 4, 8 or 16 components, and the tiles of the set's segments.  Both are filter_layout's: the
// basis has the layout of a plain filter's `back`, and the tiles are the plain filter's tiles.
struct WfilterLayout { int32_t npad = 0; std::vector<double> basis; std::vector<FilterTile> tiles; };
inline int wfilter_layout(const ProductState &S, const trx_wfilter *f, WfilterLayout &L, std::string &msg)
{
  // (filter_layout reads fwd as [nseg][ncomp][nexp]: as many entries as the basis has; what it makes of them is dropped)
  const trx_filter plain{f->ncomp, 0, f->basis, f->basis};
  FilterLayout P;
  if (const int rc = filter_layout(S, &plain, P, msg)) return refuse(msg, rc, "weighted filter: out of host memory");
  L.npad = P.npad; L.basis = std::move(P.back); L.tiles = std::move(P.tiles);
  return TRX_OK;
}

// The extents of a weighted filter of ncomp components (padded to npad) over nseg segments, nexp exposures, npix pixels and
// ntiles tiles: the padded basis, the factors [nfac][npix], the live flags [npix] (int32: 1 no pivot was singular, 0 one was)
// and the blocks of the factor kernel (kFiltWaves tiles each).
struct WfilterExtents { int32_t nfac = 0; int64_t blocks = 0; size_t basis_bytes = 0, fac_bytes = 0, live_bytes = 0; };
inline WfilterExtents wfilter_extents(int64_t npix, int32_t nexp, int32_t nseg, int32_t ncomp, int32_t npad, int64_t ntiles, int tiles_per_block)
{
  WfilterExtents X;
  X.nfac = ncomp * (ncomp + 1) / 2;
  X.blocks = (ntiles + tiles_per_block - 1) / tiles_per_block;
  X.basis_bytes = sizeof(double) * (size_t)nseg * (size_t)nexp * (size_t)npad;
  X.fac_bytes = sizeof(double) * (size_t)X.nfac * (size_t)npix;
  X.live_bytes = sizeof(int32_t) * (size_t)npix;
  return X;
}

// ---- the arithmetic of one column ------------------------------------------------------------------
// the place of L_jk (k < j) or D_j (k = j) among a column's nfac factor entries
TRX_HD int wfilter_at(int j, int k) { return j * (j + 1) / 2 + k; }

// one exposure's term of row j of the normal matrix: N_jk += (U[v][j] * w[v]) * U[v][k] for k = 0 .. j; Uv = U[v][0 .. NC-1]
template <int NC>
TRX_HD void wfilter_normal_term(const double *Uv, double w, int j, double (&Nrow)[NC])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#pragma unroll
#endif
  for (int k = 0; k < NC; k++)
    if (k <= j) Nrow[k] += (Uv[j] * w) * Uv[k];
}

// Row j of the factor from row j of the normal matrix (Nrow[0 .. j]): reads the rows below j of the column's factor,
// writes row j, and returns whether pivot j is good: D_j > TRX_WFILTER_PIVOT * N_jj (false for N_jj = 0 and for NaN).
//   for k = 0 .. j-1:  s = N_jk;  for m = 0 .. k-1: s = s - T_jm * L_km;   T_jk = s;  L_jk = s / D_k
//   D_j = N_jj;        for k = 0 .. j-1: D_j = D_j - T_jk * L_jk
template <int NC>
TRX_HD bool wfilter_factor_row(int j, const double (&Nrow)[NC], double *fac, int64_t stride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double T[NC], Lr[NC], njj = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < NC; k++) {
    T[k] = 0.0; Lr[k] = 0.0;
    if (k == j) njj = Nrow[k];
  }
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < NC; k++)
    if (k < j) {
      double s = Nrow[k];
#if defined(__clang__)
#pragma unroll
#endif
      for (int m = 0; m < NC; m++)
        if (m < k) s = s - T[m] * fac[(int64_t)wfilter_at(k, m) * stride];
      T[k] = s;
      Lr[k] = s / fac[(int64_t)wfilter_at(k, k) * stride];
      fac[(int64_t)wfilter_at(j, k) * stride] = Lr[k];
    }
  double d = njj;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < NC; k++)
    if (k < j) d = d - T[k] * Lr[k];
  fac[(int64_t)wfilter_at(j, j) * stride] = d;
  return d > TRX_WFILTER_PIVOT * njj;
}

// The factor of one column of n components: U its segment's padded vectors [nexp][NC], w the column's weights (entry v at
// w[v * stride], read only where hasw: the set has weights -- one answer for the whole launch, never a test of a lane's own
// pointer; without: every w is 1), fac its factor out (entry e at fac[e * stride]).  For row j = 0 .. n-1 one pass over the
// exposures, in exposure_trips' trips of kFiltTrips, adds row j of the normal matrix; then row j of the factor is made from it
// and from the rows below j.  Returns whether no pivot was singular.
template <int NC>
TRX_HD bool wfilter_factor_column(const double *U, const double *w, bool hasw, double *fac, int64_t stride, int nexp, int n)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool good = true;
  for (int j = 0; j < n; j++) {
    double Nrow[NC];
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < NC; k++) Nrow[k] = 0.0;
    exposure_trips<kFiltTrips>(
        nexp, [&](int v) { return hasw ? w[(int64_t)v * stride] : 1.0; },
        [&](int v, double wv) { wfilter_normal_term<NC>(U + (int64_t)v * NC, wv, j, Nrow); });
    good = wfilter_factor_row<NC>(j, Nrow, fac, stride) && good;
  }
  return good;
}

// The coefficients c from y (in place) by the column's factor of n components:
//   z_j = y_j - sum over k < j, k ascending, of L_jk * z_k;   q_j = z_j / D_j
//   c_j = q_j - sum over k > j, k ascending, of L_kj * c_k,   j descending
// each sum started from +0.  c_j = +0 for the padded components j >= n.
template <int NC>
TRX_HD void wfilter_solve(int n, double (&y)[NC], const double *fac, int64_t stride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#pragma unroll
#endif
  for (int j = 0; j < NC; j++)
    if (j < n) {
      double t = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
      for (int k = 0; k < NC; k++)
        if (k < j) t += fac[(int64_t)wfilter_at(j, k) * stride] * y[k];
      y[j] = y[j] - t;
    }
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < NC; j++)
    if (j < n) y[j] = y[j] / fac[(int64_t)wfilter_at(j, j) * stride];
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = NC - 1; j >= 0; j--)
    if (j < n) {
      double t = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
      for (int k = 0; k < NC; k++)
        if (k > j && k < n) t += fac[(int64_t)wfilter_at(k, j) * stride] * y[k];
      y[j] = y[j] - t;
    } else y[j] = 0.0;
}

// one exposure's term of y: y_j += (U[v][j] * w[v]) * g[v], every j of the padded basis (a padded U is 0)
template <int NC>
TRX_HD void wfilter_rhs_term(const double *Uv, double w, double g, double (&y)[NC])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#pragma unroll
#endif
  for (int j = 0; j < NC; j++) y[j] += (Uv[j] * w) * g;
}

// r_v = sum over j, ascending from +0, of U[v][j] * c_j (a padded component adds an exact +0), and g' = g - r_v
template <int NC>
TRX_HD double wfilter_value(const double *Uv, const double (&c)[NC], double g)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double r = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < NC; j++) r += Uv[j] * c[j];
  return g - r;
}

}  // namespace trx
