// transit_outputs.h -- the per-spectrum host code that the CLI (transit_main.cpp) and the
// library (transit_lib.cpp) share: the host side's messages, the opacity-grid build, the
// choice of trx_debug buffers a run needs for the files it writes, and the writers after the
// run.  What the reference does around one do_transit() (transit.c:125-207) besides the
// spectrum itself.  Internal to this repository's binaries: not an installed header.
#ifndef TRANSIT_OUTPUTS_H
#define TRANSIT_OUTPUTS_H

#include <cstdint>
#include <string>
#include <vector>

#include "transit_hip.h"
#include "transit_host.h"

namespace trr {

// the `verb` option (default 2, argum.c)
int verb_level(const trh_problem *P);

// The host side's warnings ("W: ...") at verb >= 2 and notes ("I: ...") at verb >= 3, one line
// each to stderr as "<prog>: warning: ..." (TOUT_WARN is level 2, TOUT_INFO level 3, flags_tr.h:181-185).
void print_messages(const trh_problem *P, int verblevel, const char *prog);

// --opacityfile names a file that does not exist yet: build the grid on one GPU (calcopacity,
// opacity.c:282-427) with a handle of its own, write it and switch P to grid mode, as the reference
// goes on with the grid it just made.  No-op when there is nothing to build.  On failure returns the
// trx_status and a message in err.
int build_opacity_grid(trh_problem *P, int verblevel, std::string &err);

// What the output options ask of a run.
struct Plan {
  bool toomuch = false, dumps = false, intens = false, saveext = false;
  bool det_tau = false, det_ext = false, det_cia = false;
  bool need_tau = false, need_e = false, need_ecs = false;
  int64_t nwn = 0;
  int nr = 0, nang = 0;
};
Plan plan_outputs(const trh_problem *P);

// --saveext: the extinction an earlier run left in the file (restfile_extinct, tau.c:155-156),
// whole grid, [nr][nwn]; restored = the file held a valid record.
struct Saved {
  bool restored = false;
  std::vector<double> e;
  std::vector<uint8_t> flags;
};

// Before a spectrum: the saveext file in, and with `savefiles yes` the samplings file out
// (makeipsample -> outsample, makesample.c:598-599), with their messages.
void before_spectrum(trh_problem *P, const Plan &plan, int verblevel, const char *prog, Saved &saved);

// The debug arrays of one run over n coarse bins, in the trx_debug layouts.
struct Buffers {
  std::vector<double> tau, e, ecs, intens, er, es, ec;
  std::vector<int64_t> last;
  std::vector<uint8_t> comp;
  // size the arrays the plan needs (n bins), point dbg at them and set opts.eager for the
  // `savefiles` dumps (their writers redo the reference's laziness from `last`).  Returns whether
  // dbg is needed at all.
  bool attach(const Plan &plan, int64_t n, trx_debug &dbg, trx_opts &opts);
};

// After the spectrum: every file the options name, from the spectrum and the debug arrays of the
// whole grid (full.comp: 1 for a layer every part of the run swept).  Writes the saveext file, gives
// the rows below the deepest ray their zeros, then toomuch, intensities, dumps, detail files and
// last the spectrum.  Returns the spectrum writer's status; the others' failures are reported on
// stderr only, as before.
int write_outputs(trh_problem *P, const Plan &plan, const Saved &saved, const double *spectrum, Buffers &full,
                  const char *prog);

}  // namespace trr

#endif
