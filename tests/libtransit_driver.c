/* libtransit_driver.c -- test driver of libtransit.so through include/transit_lib.h only.
 *
 *     libtransit_driver <script> <out_prefix>
 *
 * Reads the script line by line (the grammar of the reentry_inputs.txt files of tests/golden/reentry* plus a
 * few control words):
 *     <numbers>               run_transit(numbers, n, out, nout); out goes to <out_prefix><k>.dat
 *                             at %.17g, one value per line (k counts the runs from 1)
 *     radius <r> | cloudtop <c> | scattering <flag> <x>     the setters
 *     init <cfg> [args...]    transit_init("transit", "-c", cfg, args...)
 *     init -<option> ...      transit_init("transit", "-<option>", ...)
 *     free                    free_memory()
 *     size <n>                nout of the following runs (0, the default: get_no_samples(), or 4
 *                             when that is 0)
 *     probe                   prints transit_status(), get_no_samples(), the first three values of
 *                             get_waveno_arr() and the first value of the last run's out
 * Before every run, out is filled with the sentinel -12345.5.  After every call that can fail the
 * driver prints "status <code> <call>: <transit_error()>" when the status is not 0.  It goes on
 * after failures and exits with 0 at the end of the script.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "transit_lib.h"

#define SENTINEL (-12345.5)

static void report(const char *call)
{
  if (transit_status() != 0) printf("status %d %s: %s\n", transit_status(), call, transit_error());
}

int main(int argc, char **argv)
{
  if (argc < 3) { fprintf(stderr, "usage: %s script out_prefix\n", argv[0]); return 2; }
  FILE *in = fopen(argv[1], "r");
  if (!in) { perror(argv[1]); return 2; }
  const size_t cap = (size_t)1 << 22;
  char *line = malloc(cap);
  double *out = NULL, last_first = 0;
  int nrun = 0, size = 0;
  while (line && fgets(line, (int)cap, in)) {
    char word[64] = {0}, arg[4096] = {0};
    double a = 0, b = 0;
    if (sscanf(line, " %63s", word) != 1) continue;
    if (strcmp(word, "init") == 0) {
      char *targv[64] = {"transit", "-c"};
      char *tok = strtok(line + strspn(line, " \t") + 4, " \t\r\n");
      int targc = tok && tok[0] == '-' ? 1 : 2;
      while (tok && targc < 63) { targv[targc++] = tok; tok = strtok(NULL, " \t\r\n"); }
      targv[targc] = NULL;
      transit_init(targc, targv);
      report("transit_init");
    } else if (strcmp(word, "free") == 0) {
      free_memory();
      report("free_memory");
    } else if (sscanf(line, " size %d", &size) == 1) {
    } else if (strcmp(word, "probe") == 0) {
      const int st = transit_status();
      const int n = get_no_samples();
      double wn[3];
      get_waveno_arr(wn, 3);
      printf("probe status %d samples %d wn %.17g %.17g %.17g out %.17g\n", st, n, wn[0], wn[1], wn[2], last_first);
    } else if (sscanf(line, " radius %lf", &a) == 1) {
      set_radius(a); report("set_radius");
    } else if (sscanf(line, " cloudtop %lf", &a) == 1) {
      set_cloudtop(a); report("set_cloudtop");
    } else if (sscanf(line, " scattering %lf %lf", &a, &b) == 2) {
      set_scattering((int)a, b); report("set_scattering");
    } else if (sscanf(line, " %4095s", arg) == 1) {
      size_t n = 0, room = 1024;
      double *v = malloc(sizeof(double) * room);
      char *p = line, *e;
      for (;;) {
        const double x = strtod(p, &e);
        if (e == p) break;
        if (n == room) { room *= 2; v = realloc(v, sizeof(double) * room); }
        v[n++] = x; p = e;
      }
      if (n == 0) { free(v); fprintf(stderr, "unknown script line: %s", line); continue; }
      int nout = size > 0 ? size : get_no_samples();
      if (nout <= 0) nout = 4;
      out = realloc(out, sizeof(double) * (size_t)nout);
      for (int i = 0; i < nout; i++) out[i] = SENTINEL;
      run_transit(v, (int)n, out, nout);
      report("run_transit");
      last_first = out[0];
      char name[4096];
      snprintf(name, sizeof name, "%s%d.dat", argv[2], ++nrun);
      FILE *o = fopen(name, "w");
      if (!o) { perror(name); return 2; }
      for (int i = 0; i < nout; i++) fprintf(o, "%.17g\n", out[i]);
      fclose(o);
      free(v);
    }
  }
  fclose(in);
  free(line);
  free(out);
  printf("done %d runs\n", nrun);
  return 0;
}
