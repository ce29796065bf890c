// vmap_check.cpp -- the detection map's arithmetic (transit_amd/csrc/trx_vmap.h) on the CPU, the way k_trail_stat and
// k_velocity_map (hip/trx_vmap.hip.h) run it: the same functions, the same order of the two sums, the same buffers --
// the trail rows, the statistic lag-major and exposure-major, the call's arrays -- each a heap block of EXACTLY its size,
// so that an index outside one is an error under -fsanitize=address here and not a fault on the device.
//
//   vmap_check FILE
//
// FILE: "stat p0 p1 nlag nexp nseg nkp nvsys has_offset", then the doubles (C99 hex, nan, inf) of trail
// [nlag][nexp][nseg][7], lag_kms [nlag], kp [nkp], vsys [nvsys], orbit [nexp] and, with has_offset, offset [nexp].
// Prints "per" and nlag * nexp doubles in hex, one per line, then "map" and nkp * nvsys.
#include <cstdint>

#include "trx_vmap.h"
#include "check_common.h"

using namespace trx;

int main(int argc, char **argv)
{
  if (argc != 2) { std::fprintf(stderr, "usage: vmap_check FILE\n"); return 2; }
  FILE *f = std::fopen(argv[1], "r");
  if (!f) { std::perror(argv[1]); return 2; }
  int stat, nlag, nexp, nseg, nkp, nvsys, has_offset;
  char w0[64], w1[64];
  if (std::fscanf(f, "%d %63s %63s %d %d %d %d %d %d", &stat, w0, w1, &nlag, &nexp, &nseg, &nkp, &nvsys, &has_offset) != 9 ||
      nlag < 1 || nexp < 1 || nseg < 1 || nkp < 1 || nvsys < 1) { std::fprintf(stderr, "vmap_check: bad header\n"); return 2; }
  const double p0 = std::strtod(w0, nullptr), p1 = std::strtod(w1, nullptr);
  const size_t rows = (size_t)nlag * (size_t)nexp, cells = (size_t)nkp * (size_t)nvsys;
  const auto trail = read_doubles(f, rows * (size_t)nseg * 7), kms = read_doubles(f, (size_t)nlag), kp = read_doubles(f, (size_t)nkp);
  const auto vsys = read_doubles(f, (size_t)nvsys), orbit = read_doubles(f, (size_t)nexp);
  const auto offset = has_offset ? read_doubles(f, (size_t)nexp) : nullptr;
  std::fclose(f);

  // ---- k_trail_stat: a row's statistics in trips of 64 segments, added in segment order, NaN skipped
  std::unique_ptr<double[]> per_lv(new double[rows]), per_vl(new double[rows]);
  for (size_t row = 0; row < rows; row++) {
    const double *m0 = trail.get() + row * (size_t)nseg * 7;
    double acc = 0.0;
    for (int s0 = 0; s0 < nseg; s0 += 64) {
      double st[64];
      const int count = nseg - s0 < 64 ? nseg - s0 : 64;
      for (int lane = 0; lane < count; lane++) st[lane] = vmap_stat(m0 + (size_t)(s0 + lane) * 7, stat, p0, p1);
      for (int j = 0; j < count; j++) acc = vmap_add_stat(acc, st[j]);
    }
    const size_t l = row / (size_t)nexp, v = row % (size_t)nexp;
    per_lv[row] = acc;
    per_vl[v * (size_t)nlag + l] = acc;
  }
  // ---- k_velocity_map: a cell's terms in trips of 64 exposures, added in exposure order
  std::unique_ptr<double[]> map(new double[cells]);
  for (size_t cell = 0; cell < cells; cell++) {
    const double k_p = kp[cell / (size_t)nvsys], v_sys = vsys[cell % (size_t)nvsys];
    double acc = 0.0;
    bool outside = false;
    for (int v0 = 0; v0 < nexp; v0 += 64) {
      double term[64];
      const int count = nexp - v0 < 64 ? nexp - v0 : 64;
      for (int lane = 0; lane < count; lane++) {
        const int v = v0 + lane;
        int32_t k; double t;
        if (!vmap_locate(kms.get(), nlag, vmap_track(k_p, v_sys, orbit[(size_t)v], offset.get(), v), k, t)) outside = true;
        const double *p = per_vl.get() + (size_t)v * (size_t)nlag;
        term[lane] = nlag < 2 ? p[0] : vmap_term(p[k], p[k + 1], t);
      }
      for (int j = 0; j < count; j++) acc = acc + term[j];
    }
    map[cell] = outside ? vmap_nan() : acc;
  }
  std::printf("per\n");
  for (size_t k = 0; k < rows; k++) std::printf("%a\n", per_lv[k]);
  std::printf("map\n");
  for (size_t k = 0; k < cells; k++) std::printf("%a\n", map[k]);
  return 0;
}
