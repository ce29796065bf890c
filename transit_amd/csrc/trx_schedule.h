// trx_schedule.h -- the queues and events of one pass of a run, as a value: whether the pass ends in the ray tail
// (tail_choice), and the pass itself as a flat list of QueueOp in the order the host issues them (schedule_pass) --
// which queue each kernel goes to, which event it waits for, which event is recorded behind it.  Plain C++ (no HIP,
// no handle): shared by hip/trx_api.hip, whose Run::issue launches one op at a time, and by tests/schedule_check.cpp,
// which holds every schedule against a transcription of the control flow it replaced and against the ordering rules
// stated there (every consumer behind its producer), on the CPU.  The kernels' caps arrive as arguments (ScheduleCaps)
// because their headers are HIP.  The functions are static: none of them becomes a symbol of the library.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "trx_plan.h"

#ifndef SCHEDULE_MUTATION
#define SCHEDULE_MUTATION 0      // tests/schedule_check.cpp: 1..6 state one piece WRONGLY (7: its caps do), and the rules must catch each
#endif

namespace trx {

struct ScheduleCaps {
  long long emis_rows_above;      // kEmisRowsAbove: grids above it take the row kernels, which the tail has no form of
  int tail_rays, tail_steps;      // kTailRays, kTailSteps
  long long tail_max_rays;        // 65536: the tail's one-block-per-CU shape holds for small shards only
  int max_chunk, tau_h;           // kMaxChunk, kTauH: layers per optical-depth sub-step (vertical / slant rays)
};

// ---- the tail decision: a hinted run whose plan is 1 .. tail_steps walk steps from the top ends in ONE kernel behind its walks
struct TailIn {
  bool ray_tail = false, tail_direct = false, two_queues = false;      // the handle's switches
  bool stop_at_hint_ok = false, count = false, has_lines = false, no_saved = true, pipelined = false;
  int64_t nsh = 0, nwn = 0;
  const std::vector<PlanStep> *pass = nullptr;                         // the first pass as planned
  bool host_spectrum = false, any_product = false;                     // the caller wants the spectrum in host memory / a product behind it
};
struct TailChoice {
  bool tail_mode = false;        // the pass ends in k_ray_tail
  bool tail_direct = false;      // ... which stores the flags into the pinned block the host reads
  bool tail_spec = false;        // ... and the spectrum into pinned memory too
  bool two_queues = false;       // its second walk goes to the side queue, the tail behind it (tail_direct: nothing behind the tail on the main queue)
};

static inline TailChoice tail_choice(const TailIn &in, const ScheduleCaps &caps)
{
  TailChoice t;
  t.tail_mode = in.ray_tail && in.stop_at_hint_ok && !in.count && in.has_lines && in.no_saved &&      // (profile 1: the same plan with events around its kernels)
                in.nsh <= caps.tail_max_rays && in.nwn <= caps.emis_rows_above && in.nsh < 0x7fffffffLL / caps.tail_rays &&
                plan_is_tail(*in.pass, caps.tail_steps);
  t.tail_direct = t.tail_mode && in.tail_direct;
  t.tail_spec = t.tail_direct && in.host_spectrum && !in.any_product;
  t.two_queues = in.two_queues && t.tail_direct && in.pipelined;
  return t;
}

// ---- the schedule
enum OpKind : uint8_t { kOpWalk, kOpSweep, kOpGrid, kOpCombine, kOpCia, kOpRestore, kOpTau, kOpTail, kOpSpectrum, kOpWait, kOpRecord };
// Main: the front end, the walks and everything behind the plan's LAST walk -- that chain is the critical path, and a
// hop between queues costs it ~30 us of signalling.  Side: the combines and optical depths of the earlier steps, under
// the next step's walk; the second walk of a two-queue tail and the tail behind it.  Cia: the CIA group, which only the
// first optical depth (or the tail) needs.
enum Queue : uint8_t { kQMain, kQSide, kQCia };
enum Event : uint8_t {
  kEvNone,
  kEvInputs,           // recorded by the front end: the main queue's place behind which the inputs are in device memory
  kEvCia,              // the CIA group is done
  kEvJoin,             // the side queue's work so far
  kEvWalk1,            // the main queue's walk of a two-queue tail and the CIA group are done
  kEvStepDone,         // [idx = step of the run] the step's extinction (a sweep) or records (a walk) are complete
  kEvRecordsFree       // [idx = walk of the run] the walk's records have been combined: its buffer may be refilled
};

struct QueueOp {
  OpKind kind; Queue q; Event ev = kEvNone;
  uint8_t parity = 0;                  // walk, combine: which of the two record buffers
  bool opens = false, closes = false;  // optical-depth sub-step: the first / last of its step (a profiled run's bracket)
  int step = 0;                        // the plan step it belongs to
  int idx = 0;                         // kEvStepDone, kEvRecordsFree: which event
  int r_top = 0, nc = 0;               // optical-depth sub-step: its layers r_top .. r_top-nc+1
};

struct ScheduleIn {
  bool pipelined = false, has_grid = false, vertical = false, has_lines = false;
  TailChoice tail;
  const uint8_t *saved = nullptr;      // [nr] layers restored from an earlier run (null: none)
  int nr = 0;
};
// what survives from the first pass into the resumed one
struct ScheduleState {
  int steps = 0, walks = 0;                               // queued so far: they number the step and record events
  bool cia_queued = false, side_behind_inputs = false;    // (side_behind_inputs: by its side work; a tail's side walk waits on its own)
};
struct PassEnd { Queue spectrum_q = kQMain; bool sync_side = false; };      // the host synchronises the side queue (where asked), then the main queue

// One pass: the planned steps from the top down, the spectrum of what they swept.
//   * A walk step's side work -- its combine, the CIA group ahead of the run's first optical depth, the optical depth --
//     goes to the side queue for every step but the plan's last, and is ISSUED only behind the next step's walk: the walks
//     then sit back to back on the main queue however long the host takes over the rest.  A two-kernel step's side work is
//     issued at once (the later queueing of its optical depth delays the stop information the next step's tiles read).
//   * The walks alternate between two record buffers: walk w waits for records_free[w - 2].
//   * Tail mode: no combine, no optical depth; the CIA group behind the first walk.  With two queues the main queue waits
//     for it there and records walk1 -- ONE event for the tail to wait for -- and the second walk goes to the side queue
//     behind the inputs, the tail behind it there (same queue: no signal between them).  Two walks of one run do not
//     depend on each other, and a walk alone leaves a third of the device idle for the last third of its time: waves of
//     one launch start together and end apart, and the kernel behind it on the queue cannot start before the last wave
//     has ended (in-kernel clocks, round 5: 7168 waves in flight for the first 60 us of k_line_walk<2>, then 5000, 3900,
//     3000, 2200, 1200, 370 at 5 us steps); the second walk fills what the first one leaves.  Demo: 0.269 -> 0.251 ms, the
//     same bits.  walk1 covers every walk of the main queue only while the side queue takes every walk but the first:
//     caps.tail_steps == 2 (tests/schedule_check.cpp shows what 3 would lose).
//   * join: the main queue waits for the side queue's work where it goes on with it -- the last step's optical depth,
//     the spectrum kernel -- and only when some is outstanding.
static inline PassEnd schedule_pass(const std::vector<PlanStep> &plan, const ScheduleIn &in, const ScheduleCaps &caps,
                                    ScheduleState &state, std::vector<QueueOp> &out)
{
  out.clear();
  PassEnd end;
  auto op = [&](OpKind kind, Queue q, int step) -> QueueOp & { out.push_back(QueueOp{kind, q}); out.back().step = step; return out.back(); };
  auto wait = [&](Queue q, Event ev, int step, int idx = 0) { QueueOp &w = op(kOpWait, q, step); w.ev = ev; w.idx = idx; };
  auto record = [&](Queue q, Event ev, int step, int idx = 0) { QueueOp &r = op(kOpRecord, q, step); r.ev = ev; r.idx = idx; };
  auto cia = [&](int step) {
    wait(kQCia, kEvInputs, step); op(kOpCia, kQCia, step); record(kQCia, kEvCia, step);
    state.cia_queued = true;
  };
  bool side_dirty = false;             // work on the side queue that the main queue has not waited for
  auto join = [&](int step) {
    if (!side_dirty || SCHEDULE_MUTATION == 4) return;
    record(kQSide, kEvJoin, step); wait(kQMain, kEvJoin, step);
    side_dirty = false;
  };
  // the rest of a step behind its extinction
  struct Side { int step = -1, run_step = 0, walk = -1; Queue q = kQMain; } pending;      // (walk: the one whose records the combine reads; -1: none)
  auto side_work = [&](const Side &S) {
    const PlanStep &s = plan[(size_t)S.step];
    // The side queue's first work of a run waits for the inputs explicitly, whatever else it waits for.
    if (S.q == kQSide && !state.side_behind_inputs) { if (SCHEDULE_MUTATION != 1) wait(kQSide, kEvInputs, S.step); state.side_behind_inputs = true; }
    if (S.walk >= 0) {
      if (S.q == kQSide) wait(kQSide, kEvStepDone, S.step, S.run_step);
      op(kOpCombine, S.q, S.step).parity = (uint8_t)(S.walk & 1);
      if (S.q == kQSide) record(kQSide, kEvRecordsFree, S.step, S.walk);
    }
    if (S.run_step == 0) { cia(S.step); if (SCHEDULE_MUTATION != 3) wait(S.q, kEvCia, S.step); }
    if (S.q == kQMain) join(S.step); else side_dirty = true;
    bool restore = false;
    for (int c = 0; c < s.nc && in.saved && !restore; c++) restore = in.saved[s.r_top - c] != 0;
    if (restore) op(kOpRestore, S.q, S.step);
    // optical depth in sub-steps of at most tau_cap layers; the run's first holds the 2- and 3-point rays
    const int tau_cap = in.vertical ? caps.max_chunk : caps.tau_h;
    for (int done = 0; done < s.nc; ) {
      int nt = std::min(tau_cap, s.nc - done);
      if (s.r_top == in.nr - 1 && done == 0) nt = std::min(s.nc, std::max(nt, 3));
      QueueOp &t = op(kOpTau, S.q, S.step);
      t.r_top = s.r_top - done; t.nc = nt; t.opens = done == 0; t.closes = done + nt == s.nc;
      done += nt;
    }
  };

  const TailChoice &tail = in.tail;
  for (int k = 0; k < (int)plan.size(); k++, state.steps++) {
    const PlanStep &s = plan[(size_t)k];
    Side S; S.step = k; S.run_step = state.steps;
    S.q = in.pipelined && !s.last_step ? kQSide : kQMain;
    bool walked = false;
    if (in.has_grid) op(kOpGrid, kQMain, k);
    else {
      bool all_saved = in.saved != nullptr;      // a step whose layers are all restored sweeps nothing
      for (int c = 0; c < s.nc && all_saved; c++) all_saved = in.saved[s.r_top - c] != 0;
      if (in.has_lines && !all_saved) {
        if (s.nb && tail.tail_mode) {      // (no combine of its own: its records wait for the tail, each step in its own buffer)
          const bool side_walk = tail.two_queues && S.run_step == 1;
          if (side_walk) { if (SCHEDULE_MUTATION != 1) wait(kQSide, kEvInputs, k); end.spectrum_q = kQSide; end.sync_side = true; }
          op(kOpWalk, side_walk ? kQSide : kQMain, k).parity = (uint8_t)(state.walks & 1);
          state.walks++;
        } else if (s.nb) {
          if (in.pipelined && state.walks >= 2 && SCHEDULE_MUTATION != 2) wait(kQMain, kEvRecordsFree, k, state.walks - 2);
          op(kOpWalk, kQMain, k).parity = (uint8_t)(state.walks & 1);
          if (S.q == kQSide) record(kQMain, kEvStepDone, k, S.run_step);
          S.walk = state.walks++;
        } else op(kOpSweep, kQMain, k);
        walked = s.nb != 0;
      }
      if (S.q == kQSide && !walked) { record(kQMain, kEvStepDone, k, S.run_step); wait(kQSide, kEvStepDone, k, S.run_step); }      // the optical depth of this step follows its extinction
    }
    if (tail.tail_mode) {
      // the CIA group behind the first walk (what the device is waiting for) -- ahead of a second walk on the side queue
      // too: next to TWO walks its kernels take three times as long
      if (!state.cia_queued) {
        cia(k);
        if (tail.two_queues && !s.last_step) {
          if (SCHEDULE_MUTATION == 6) record(kQMain, kEvWalk1, k);
          wait(kQMain, kEvCia, k);
          if (SCHEDULE_MUTATION != 6) record(kQMain, kEvWalk1, k);
        }
      }
    } else {
      if (pending.step >= 0) { side_work(pending); pending.step = -1; }
      if (S.q == kQSide && walked) pending = S; else side_work(S);
    }
  }
  if (pending.step >= 0) side_work(pending);      // (no plan of today leaves one: its last step's side work is issued at once)
  const int last = (int)plan.size() - 1;
  join(last);
  if (tail.tail_mode) {
    if (end.spectrum_q == kQSide) { if (SCHEDULE_MUTATION != 5) wait(kQSide, kEvWalk1, last); }
    else { if (!state.cia_queued) cia(last); wait(kQMain, kEvCia, last); }
    op(kOpTail, end.spectrum_q, last);
  } else op(kOpSpectrum, kQMain, last);
  return end;
}

}  // namespace trx
