// broaden_check.cpp -- the rotational broadening's per-bin arithmetic (transit_amd/csrc/trx_broaden.h) on the CPU, the
// way k_broaden runs it: block by block, every block over a heap buffer of EXACTLY the tile it would stage, so that a
// tile one bin short is an out-of-bounds read under -fsanitize=address here and not a fault on the device.
//
//   broaden_check [nwn]      (default 6001: the grid 2500 cm-1 + i * 0.01 of the GPU tests)
//
// For every beta of the GPU tests and three limb coefficients: each block's bins by broaden_bin over its tile, compared
// with a long-double evaluation of the definition inside tol_i = A_i (2 h_i + 17) 2^-52 + E_i (transit_hip.h's
// definition; the bound of transit_amd/broaden.py); the half-widths must not decrease; the halo of the first and the
// last block is printed.  Exit status 1 when a bin is outside its bound or a half-width decreases.
// -DBROADEN_TILE_SHORT=1 stages every tile with a halo one bin too narrow (the planted mistake the test looks for).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "trx_broaden.h"

#ifndef BROADEN_TILE_SHORT
#define BROADEN_TILE_SHORT 0
#endif

using namespace trx;

// the definition in long double: the double x, weights and sums in long double; also the bound's two terms
static void reference(const std::vector<double> &S, double wn_i, double wn_d, double beta, double limb, int64_t i,
                      long double &B, double &tol)
{
  const int64_t n = (int64_t)S.size();
  double d;
  const int h = (int)broaden_half(wn_i, wn_d, beta, i, d);
  const BroadWeights W = broaden_weights(limb);
  if (h == 0) { B = S[(size_t)i]; tol = std::fabs(S[(size_t)i]) * 17.0 * 0x1p-52; return; }
  const long double w0 = (long double)W.c1 + (long double)W.c2;
  long double num = w0 * S[(size_t)i], den = w0, absnum = w0 * std::fabs(S[(size_t)i]);
  for (int k = 1; k <= h; k++) {
    const double x = ((double)k * wn_d) / d;
    long double t = 1.0L - (long double)x * x;
    if (t < 0) t = 0;
    const long double w = W.c1 * sqrtl(t) + W.c2 * t;
    if (i - k >= 0) { num += w * S[(size_t)(i - k)]; den += w; absnum += w * std::fabs(S[(size_t)(i - k)]); }
    if (i + k < n)  { num += w * S[(size_t)(i + k)]; den += w; absnum += w * std::fabs(S[(size_t)(i + k)]); }
  }
  B = num / den;
  const double e = 8.0 * 0x1p-52;
  long double E = 0;
  for (int k = 1; k <= h; k++) {
    const double x = ((double)k * wn_d) / d;
    double t = 1.0 - x * x;
    if (t < 0) t = 0;
    const double slope = W.c1 * (t > 0 ? std::fmin(std::sqrt(e), e / std::sqrt(t)) : std::sqrt(e));
    if (i - k >= 0) E += slope * fabsl(S[(size_t)(i - k)] - B);
    if (i + k < n)  E += slope * fabsl(S[(size_t)(i + k)] - B);
  }
  tol = (double)(absnum / den * (2.0 * h + 17.0) * 0x1p-52 + E / den);
}

int main(int argc, char **argv)
{
  const int64_t nwn = argc > 1 ? std::atoll(argv[1]) : 6001;
  const double wn_i = 2500.0, wn_d = 0.01;
  std::vector<double> S((size_t)nwn);
  std::mt19937_64 rng(20240607);
  std::normal_distribution<double> g(0.0, 1.0);
  for (double &s : S) s = std::exp(g(rng));
  const double betas[4] = {1.037e-4, 1.3037e-3, 3.95e-6, 2e-6}, limbs[3] = {0.0, 0.6, 1.0};
  long long bins = 0, outside = 0, decreasing = 0;
  for (double beta : betas) {
    double d;
    const int hmax = (int)broaden_half(wn_i, wn_d, beta, nwn - 1, d), hmin = (int)broaden_half(wn_i, wn_d, beta, 0, d);
    double prev = 0;
    for (int64_t i = 0; i < nwn; i++) { const double hh = broaden_half(wn_i, wn_d, beta, i, d); if (hh < prev) decreasing++; prev = hh; }
    const int64_t blocks = (nwn + kBroadBlock - 1) / kBroadBlock;
    double worst = 0, worst_rel = 0; int64_t copies = 0;
    for (double limb : limbs) {
      const BroadWeights W = broaden_weights(limb);
      for (int64_t blk = 0; blk < blocks; blk++) {
        // ---- what k_broaden does with block blk
        const int64_t i0 = blk * kBroadBlock, i1 = std::min<int64_t>(i0 + kBroadBlock - 1, nwn - 1);
        const int H = std::min((int)broaden_half(wn_i, wn_d, beta, i1, d), hmax);
        int64_t t0, t1;
        broaden_tile(i0, i1, std::max(H - BROADEN_TILE_SHORT, 0), nwn, t0, t1);
        if (t1 - t0 + 1 > kBroadBlock + 2 * (int64_t)hmax) { std::printf("block %lld: tile of %lld bins above the launch's %lld\n", (long long)blk, (long long)(t1 - t0 + 1), (long long)(kBroadBlock + 2 * (int64_t)hmax)); return 1; }
        double *tile = new double[(size_t)(t1 - t0 + 1)];            // exact size: the sanitizer guards both ends
        for (int64_t j = t0; j <= t1; j++) tile[j - t0] = S[(size_t)j];
        if (limb == limbs[0] && (blk == 0 || blk == blocks - 1))
          std::printf("beta %g: block %lld bins [%lld, %lld] H %d stages [%lld, %lld]\n", beta, (long long)blk, (long long)i0, (long long)i1, H, (long long)t0, (long long)t1);
        for (int64_t i = i0; i <= i1; i++) {
          const int h = std::min((int)broaden_half(wn_i, wn_d, beta, i, d), H);
          const double got = broaden_bin(tile, t0, nwn, i, h, d, wn_d, W);
          long double B; double tol;
          reference(S, wn_i, wn_d, beta, limb, i, B, tol);
          const double err = (double)fabsl(got - B);
          bins++;
          if (h == 0) { copies++; if (got != S[(size_t)i]) outside++; continue; }
          if (!(err <= tol)) outside++;
          worst = std::max(worst, err / tol); worst_rel = std::max(worst_rel, err / (double)fabsl(B));
        }
        delete[] tile;
      }
    }
    std::printf("beta %g: h %d..%d, %lld blocks, %lld copied bins, largest err/tol %.4f, largest relative error %.3e\n",
                beta, hmin, hmax, (long long)blocks, (long long)copies, worst, worst_rel);
  }
  std::printf("%lld bins, %lld outside their bound, %lld decreasing half-widths\n", bins, outside, decreasing);
  return outside || decreasing ? 1 : 0;
}
