// schedule_check -- the queues and events of a pass (transit_amd/csrc/trx_schedule.h) on plan_check's seeded cases (layer
// profiles, depth hints, layer_chunk values, eager and opacity-grid modes), crossed with the tail switches (ray tail, two
// queues, direct tail), pipelined or not, vertical or slant rays, and saved-layer patterns (none, some, a whole step, all);
// behind every first pass that stops at a hint, the pass of a run that resumed below it.
//
// (a) Equality.  Parent below is a transcription of the control flow that issued a pass before the schedule was a value:
//     Run::step / line_step / side_work / join_early / queue_cia / ray_tail / spectrum_kernel with their mutable members
//     (early_dirty, early_behind_inputs, cia_queued, tail_on_side, pending, nwalks, nchunks), walk_chunk's and
//     launch_combine's waits and records, each hipStreamWaitEvent / hipEventRecord / launch emitting one QueueOp.
//     schedule_pass must equal it op for op: the same order, the same queues, the same events.  tail_choice is held
//     against the four expressions of plan_first_pass in the same way.
//
// (b) Ordering rules, checked by a happens-before walk over the op list: a clock per queue, an op advances its queue's, a
//     record keeps the queue's clock in its event, a wait joins the event's clock in, a host synchronise joins the
//     synchronised queues' clocks into every queue's.  The main queue starts behind the front end, which records `inputs`.
//      1. every kernel or copy of a pass is behind the `inputs` mark, on whichever queue it is;
//      2. a combine, or the tail, reads a record buffer behind the walk that filled it;
//      3. a walk that refills a record buffer is behind that buffer's last reader -- the combine two walks earlier, or the
//         tail (a host synchronise in between counts) -- and the buffer HAS been read;
//      4. an optical-depth sub-step is behind the combine, sweep, grid step and restore of every layer it integrates and
//         behind the sub-step above it, and the sub-steps tile the layers from the top;
//      5. the first sub-step of a run, every sub-step of a resumed pass, and the tail are behind the CIA group;
//      6. the spectrum kernel is behind every sub-step of its pass;
//      7. the tail is behind every walk of its pass;
//      8. at the end of a pass every op is ordered before one of the host's synchronises;
//      9. step and record events stay inside the nr + 1 that the run creates;
//     10. a run that is not pipelined names no side-queue op and no step or record event.
//     Not a rule: the sweeps' reads of flags and last (skip_done) are advisory by design -- a walk runs beside the previous
//     step's optical depth and may or may not see what it published.
//
// (c) -DSCHEDULE_MUTATION=n states the schedule WRONGLY, and the rules of (b) alone must report each: 1 the side queue's
//     waits for `inputs` dropped; 2 the walk's wait for records_free dropped; 3 the wait for `cia` ahead of the first
//     optical depth dropped; 4 the join dropped (ahead of the spectrum kernel AND ahead of the last step's optical depth:
//     the plan's last step always integrates on the main queue and joins there, so the spectrum kernel's own join finds
//     nothing outstanding in any schedule of today); 5 the side tail's wait for walk1 dropped; 6 walk1 recorded ahead of the
//     main queue's wait for `cia`; 7 tail_steps = 3 in the caps under "the side queue takes the second walk only": the
//     third walk lands on the main queue behind walk1 and the tail is unordered against it (equality still holds: the
//     transcription does the same).
// Prints "<cases> cases, <bad> differ", "rules: <checked> checked, <violated> violated", what the draws covered, "ok <checks>".
#include <algorithm>
#include <random>
#include <vector>
#include "check_common.h"
#include "trx_schedule.h"

using namespace trx;

static int cases = 0, differ = 0;
static long rule_checks = 0, rule_bad = 0;
static const ScheduleCaps kCaps{65536, 10, SCHEDULE_MUTATION == 7 ? 3 : 2, 65536, 32, 32};

// ---- (a) the parent's control flow, emitting QueueOps --------------------------------------------------
struct Parent {
  // what the run is given
  const std::vector<PlanStep> *plan = nullptr;
  bool pipelined = false, has_grid = false, vertical = false, has_lines = false;
  const uint8_t *saved = nullptr; int nr = 0;
  bool tail_mode = false, two_queues = false;
  // the members that steered it
  bool early_dirty = false, early_behind_inputs = false, cia_queued = false, tail_on_side = false;
  int nchunks = 0, nwalks = 0; Queue tst = kQMain;
  struct PendingCombine { bool valid = false; Queue sc = kQMain; int ev_walk = -1, ev_done = -1, parity = 0; bool cross = false; };
  struct SideWork { bool active = false, first = false; int r_top = 0, nc = 0, swept = 0, step = 0; Queue st_tau = kQMain; PendingCombine pc; } pending;
  struct WalkQueue { int parity = 0; bool st_comb = false; Queue q_comb = kQMain; int ev_walk = -1, ev_reuse = -1, ev_done = -1; };
  std::vector<QueueOp> *out = nullptr;

  Queue st_early() const { return pipelined ? kQSide : kQMain; }
  QueueOp &emit(OpKind kind, Queue q, int step) { out->push_back(QueueOp{kind, q}); out->back().step = step; return out->back(); }
  void wait(Queue q, Event ev, int step, int idx = 0) { QueueOp &o = emit(kOpWait, q, step); o.ev = ev; o.idx = idx; }
  void record(Queue q, Event ev, int step, int idx = 0) { QueueOp &o = emit(kOpRecord, q, step); o.ev = ev; o.idx = idx; }

  void join_early(int step) {
    if (!early_dirty) return;
    record(st_early(), kEvJoin, step); wait(kQMain, kEvJoin, step);
    early_dirty = false;
  }
  void queue_cia(int step) {
    wait(kQCia, kEvInputs, step);
    emit(kOpCia, kQCia, step);
    record(kQCia, kEvCia, step);
    cia_queued = true;
  }
  void launch_combine(PendingCombine &pc, int step) {
    if (!pc.valid) return;
    pc.valid = false;
    if (pc.cross) wait(pc.sc, kEvStepDone, step, pc.ev_walk);
    emit(kOpCombine, pc.sc, step).parity = (uint8_t)(pc.parity & 1);
    if (pc.cross && pc.ev_done >= 0) record(pc.sc, kEvRecordsFree, step, pc.ev_done);
  }
  // walk_chunk: the wait for the buffer, the walk on st, the record behind it; the combine handed back (every caller deferred it)
  PendingCombine walk_chunk(Queue st, const WalkQueue &Q, int step) {
    if (Q.ev_reuse >= 0) wait(st, kEvRecordsFree, step, Q.ev_reuse);
    emit(kOpWalk, st, step).parity = (uint8_t)(Q.parity & 1);
    PendingCombine pc;
    pc.valid = true; pc.sc = Q.st_comb ? Q.q_comb : st; pc.cross = Q.st_comb && Q.ev_walk >= 0;
    pc.ev_walk = Q.ev_walk; pc.ev_done = Q.ev_done; pc.parity = Q.parity;
    if (pc.cross) record(st, kEvStepDone, step, Q.ev_walk);
    return pc;
  }
  void side_work(SideWork &S) {
    if (S.st_tau != kQMain && !early_behind_inputs) { wait(S.st_tau, kEvInputs, S.step); early_behind_inputs = true; }
    launch_combine(S.pc, S.step);
    if (S.first) { queue_cia(S.step); wait(S.st_tau, kEvCia, S.step); }
    if (S.st_tau == kQMain) join_early(S.step);
    else early_dirty = true;
    if (saved) {
      bool any = false;      // (one op for the step's copies)
      for (int c = 0; c < S.nc; c++) any = any || saved[S.r_top - c];
      if (any) emit(kOpRestore, S.st_tau, S.step);
    }
    const int tau_cap = vertical ? kCaps.max_chunk : kCaps.tau_h;
    for (int done = 0; done < S.nc; ) {
      int nt = std::min(tau_cap, S.nc - done);
      if (S.swept == 0 && done == 0) nt = std::min(S.nc, std::max(nt, 3));
      QueueOp &t = emit(kOpTau, S.st_tau, S.step);
      t.r_top = S.r_top - done; t.nc = nt; t.opens = done == 0; t.closes = done + nt == S.nc;
      done += nt;
    }
  }
  void line_step(const PlanStep &s, SideWork &S, bool &walked) {
    Queue st = kQMain;
    bool all_saved = saved != nullptr;
    for (int c = 0; c < s.nc && all_saved; c++) all_saved = saved[s.r_top - c] != 0;
    if (has_lines && !all_saved) {
      if (s.nb && tail_mode) {
        const bool side_walk = two_queues && nchunks == 1;
        if (side_walk) { wait(kQSide, kEvInputs, S.step); st = kQSide; tail_on_side = true; }
        WalkQueue Q;
        Q.parity = nwalks;
        walk_chunk(st, Q, S.step);
        nwalks++;
      }
      else if (s.nb) {
        WalkQueue Q;
        Q.parity = nwalks;
        if (S.st_tau != kQMain) { Q.st_comb = true; Q.q_comb = S.st_tau; }
        Q.ev_walk = nchunks;
        // (the parent indexed ev_cb here whatever the mode; the events exist in pipelined runs only, and every run with
        // lines is pipelined: a line run that is not has no such wait to make)
        if (nwalks >= 2 && pipelined) Q.ev_reuse = nwalks - 2;
        Q.ev_done = nwalks;
        S.pc = walk_chunk(st, Q, S.step);
        nwalks++;
      }
      else emit(kOpSweep, st, S.step);
      walked = s.nb != 0;
    }
    if (S.st_tau != kQMain && !walked) { record(kQMain, kEvStepDone, S.step, nchunks); wait(S.st_tau, kEvStepDone, S.step, nchunks); }
  }
  void step(const PlanStep &s, int k) {
    SideWork S; bool walked = false;
    S.first = nchunks == 0; S.r_top = s.r_top; S.nc = s.nc; S.swept = nr - 1 - s.r_top; S.step = k;
    S.st_tau = (pipelined && !s.last_step) ? st_early() : kQMain;
    if (has_grid) emit(kOpGrid, kQMain, k); else line_step(s, S, walked);
    if (tail_mode) {
      if (!cia_queued) {
        queue_cia(k);
        if (two_queues && !s.last_step) { wait(kQMain, kEvCia, k); record(kQMain, kEvWalk1, k); }
      }
    } else {
      if (pending.active) { side_work(pending); pending.active = false; }
      S.active = true;
      if (S.st_tau != kQMain && walked) pending = S;
      else side_work(S);
    }
    nchunks++;
  }
  void ray_tail(int step) {
    if (tail_on_side) { tst = kQSide; wait(tst, kEvWalk1, step); }
    else {
      if (!cia_queued) queue_cia(step);
      wait(kQMain, kEvCia, step);
    }
    emit(kOpTail, tst, step);
  }
  void spectrum_kernel(int step) {
    join_early(step);
    tst = kQMain;
    if (tail_mode) ray_tail(step);
    else emit(kOpSpectrum, kQMain, step);
  }
  PassEnd pass() {
    out->clear();
    for (int k = 0; k < (int)plan->size(); k++) step((*plan)[(size_t)k], k);
    const int last = (int)plan->size() - 1;
    if (pending.active) { side_work(pending); pending.active = false; }
    spectrum_kernel(last);
    PassEnd e; e.spectrum_q = tst; e.sync_side = tail_on_side;      // results(): the side queue where the tail ran there, then the main queue
    return e;
  }
  void resume() { tail_mode = tail_on_side = false; }
};

static bool same(const QueueOp &a, const QueueOp &b)
{
  return a.kind == b.kind && a.q == b.q && a.ev == b.ev && a.parity == b.parity && a.opens == b.opens && a.closes == b.closes &&
         a.step == b.step && a.idx == b.idx && a.r_top == b.r_top && a.nc == b.nc;
}

// ---- (b) the rules --------------------------------------------------------------------------------------
struct Clock { int c[3] = {0, 0, 0}; void join(const Clock &o) { for (int i = 0; i < 3; i++) c[i] = std::max(c[i], o.c[i]); } };
struct Ref { int q = -1, seq = 0; bool valid() const { return q >= 0; } };
struct Snap { bool valid = false; Clock at; };

struct Rules {
  int nr; bool pipelined, has_grid, has_lines; const uint8_t *saved;
  Clock now[3]; int seq[3] = {1, 0, 0};      // the main queue's op 1: the front end, which records `inputs`
  Snap fixed[5]; std::vector<Snap> step_done, records_free;
  Ref cia, fill[2], reader[2], prev_tau; std::vector<Ref> writer, restorer;
  std::vector<Ref> walks_pass, taus_pass; int walk_parity_pass[2] = {0, 0};
  int next_layer; bool resumed = false;

  Rules(int nr_, bool pipelined_, bool has_grid_, bool has_lines_, const uint8_t *saved_)
    : nr(nr_), pipelined(pipelined_), has_grid(has_grid_), has_lines(has_lines_), saved(saved_), step_done((size_t)nr_ + 1),
      records_free((size_t)nr_ + 1), writer((size_t)nr_), restorer((size_t)nr_), next_layer(nr_ - 1)
  {
    now[kQMain].c[kQMain] = 1;
    fixed[kEvInputs].valid = true; fixed[kEvInputs].at = now[kQMain];
  }
  void rule(bool ok, const char *what, const QueueOp &op) {
    rule_checks++;
    if (!ok && rule_bad++ < 20) std::printf("case %d: rule violated: %s (op kind %d, queue %d, step %d)\n", cases, what, (int)op.kind, (int)op.q, op.step);
  }
  bool behind(const Ref &a, const Clock &c) const { return a.valid() && c.c[a.q] >= a.seq; }
  Snap *event(const QueueOp &op) {
    if (op.ev == kEvStepDone || op.ev == kEvRecordsFree) {
      rule(op.idx >= 0 && op.idx <= nr, "9: a step or record event inside the nr + 1 created", op);
      rule(pipelined, "10: no step or record event in a run that is not pipelined", op);
      if (op.idx < 0 || op.idx > nr) return nullptr;
      return op.ev == kEvStepDone ? &step_done[(size_t)op.idx] : &records_free[(size_t)op.idx];
    }
    return &fixed[op.ev];
  }
  void pass(const std::vector<PlanStep> &plan, const std::vector<QueueOp> &ops, const PassEnd &end) {
    for (const QueueOp &op : ops) {
      if (op.q == kQSide) rule(pipelined, "10: no side-queue op in a run that is not pipelined", op);
      if (op.kind == kOpWait) { const Snap *e = event(op); if (e && e->valid) now[op.q].join(e->at); continue; }      // (an event never recorded: nothing to wait for)
      if (op.kind == kOpRecord) { Snap *e = event(op); if (e) { e->valid = true; e->at = now[op.q]; } continue; }
      Ref me; me.q = op.q; me.seq = ++seq[op.q];
      now[op.q].c[op.q] = me.seq;
      const Clock &at = now[op.q];
      rule(at.c[kQMain] >= 1, "1: behind the inputs mark", op);
      const PlanStep &s = plan[(size_t)op.step];
      switch (op.kind) {
        case kOpWalk:
          if (fill[op.parity].valid()) rule(behind(reader[op.parity], at), "3: a refilled record buffer has been read, and the walk is behind its reader", op);
          fill[op.parity] = me; reader[op.parity] = Ref(); walks_pass.push_back(me); walk_parity_pass[op.parity] = 1;
          break;
        case kOpCombine:
          rule(behind(fill[op.parity], at), "2: the combine behind the walk that filled its buffer", op);
          reader[op.parity] = me;
          for (int c = 0; c < s.nc; c++) writer[(size_t)(s.r_top - c)] = me;
          break;
        case kOpSweep: case kOpGrid:
          for (int c = 0; c < s.nc; c++) writer[(size_t)(s.r_top - c)] = me;
          break;
        case kOpRestore:
          for (int c = 0; c < s.nc; c++) if (saved && saved[s.r_top - c]) {
            if (writer[(size_t)(s.r_top - c)].valid()) rule(behind(writer[(size_t)(s.r_top - c)], at), "4: a restored row behind the step's own extinction", op);
            restorer[(size_t)(s.r_top - c)] = me;
          }
          break;
        case kOpCia: cia = me; break;
        case kOpTau: {
          rule(op.r_top == next_layer && op.nc >= 1 && op.r_top - op.nc >= -1, "4: the sub-steps tile the layers from the top", op);
          bool all_saved = saved != nullptr;
          for (int c = 0; c < s.nc && all_saved; c++) all_saved = saved[s.r_top - c] != 0;
          for (int c = 0; c < op.nc && op.r_top - c >= 0 && op.r_top - c < nr; c++) {
            const size_t r = (size_t)(op.r_top - c);
            if (has_grid || (has_lines && !all_saved)) rule(behind(writer[r], at), "4: the sub-step behind its layers' combine, sweep or grid step", op);
            if (saved && saved[r]) rule(behind(restorer[r], at), "4: the sub-step behind its layers' restore", op);
          }
          if (prev_tau.valid()) rule(behind(prev_tau, at), "4: the sub-step behind the sub-step above it", op);
          if (!prev_tau.valid() || resumed) rule(behind(cia, at), "5: the run's first sub-step, and a resumed pass's, behind the CIA group", op);
          prev_tau = me; taus_pass.push_back(me); next_layer = op.r_top - op.nc;
          break;
        }
        case kOpTail:
          for (const Ref &w : walks_pass) rule(behind(w, at), "7: the tail behind every walk of its pass", op);
          for (int p = 0; p < 2; p++) if (walk_parity_pass[p]) { rule(behind(fill[p], at), "2: the tail behind the walk that filled a buffer", op); reader[p] = me; }
          rule(behind(cia, at), "5: the tail behind the CIA group", op);
          prev_tau = me;
          for (const PlanStep &t : plan) next_layer -= t.nc;
          break;
        case kOpSpectrum:
          for (const Ref &t : taus_pass) rule(behind(t, at), "6: the spectrum kernel behind every sub-step of its pass", op);
          break;
        default: break;
      }
    }
    // the host's synchronises: the side queue where the schedule asks for it, then the main queue
    Clock joined = now[kQMain];
    if (end.sync_side) joined.join(now[kQSide]);
    QueueOp none{kOpSpectrum, kQMain};
    for (int q = 0; q < 3; q++) rule(joined.c[q] >= seq[q], "8: every op of the pass before one of the host's synchronises", none);      // (a queue's last op stands for those ahead of it)
    for (int q = 0; q < 3; q++) now[q].join(joined);
    walks_pass.clear(); taus_pass.clear(); walk_parity_pass[0] = walk_parity_pass[1] = 0;
    resumed = true;
  }
};

// ---- the cases ------------------------------------------------------------------------------------------
static long n_tail1 = 0, n_tail2q = 0, n_tail1q = 0, n_deferred = 0, n_between = 0, n_grid = 0, n_saved_step = 0, n_res1 = 0, n_res2q = 0, n_res1q = 0;

static void compare(const std::vector<QueueOp> &got, const std::vector<QueueOp> &want, const PassEnd &ge, const PassEnd &we, const char *which)
{
  bool ok = got.size() == want.size() && ge.spectrum_q == we.spectrum_q && ge.sync_side == we.sync_side;
  size_t at = 0;
  for (; ok && at < got.size(); at++) ok = same(got[at], want[at]);
  g_checks++;
  if (!ok && differ++ < 20) std::printf("case %d (%s): the schedule differs from the transcription at op %zu of %zu / %zu\n", cases, which, at, got.size(), want.size());
}

int main(int argc, char **argv)
{
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 20000;
  const int kWalkCap = 64, kChunkCap = 32;
  std::mt19937_64 rng(20261), rng_x(20264);      // (plan_check's cases from plan_check's generator; the crosses from one of their own)
  std::vector<QueueOp> got, want;
  for (int r = 0; r < rounds; r++) {
    const int nr = 3 + (int)(rng() % (r % 7 == 0 ? 300 : 120));
    std::vector<int> frame((size_t)nr); std::vector<unsigned char> wide((size_t)nr);
    const int shape = (int)(rng() % 4);
    const int kinds[5] = {2, 4, 8, 16, 0};
    int level = (int)(rng() % 5);
    const bool wide_all = rng() % 2;
    for (int i = nr - 1; i >= 0; i--) {
      if (shape == 0) level = (int)(rng() % 5);
      else if (shape == 1) { if (rng() % 12 == 0 && level < 4) level++; }
      else if (shape == 2) { if (rng() % 40 == 0) level = (int)(rng() % 5); }
      else level = (rng() % 3 == 0) ? 4 : (int)(rng() % 4);
      frame[(size_t)i] = kinds[level];
      wide[(size_t)i] = frame[(size_t)i] == 0 && (wide_all || rng() % 3 == 0);
    }
    PlanInput in;
    in.frame = frame.data(); in.very_wide = wide.data(); in.nr = nr;
    in.has_grid = r % 11 == 0; in.eager = r % 5 == 0;
    in.user_chunk = (rng() % 3 == 0) ? 3 + (int)(rng() % 70) : 0;
    in.hint_layers = (rng() % 4 == 0) ? 0 : 1 + (int)(rng() % (nr + 5));
    in.stop_at_hint_ok = !in.has_grid && !in.eager && in.hint_layers > 0 && in.hint_layers <= nr;
    bool any_wide = false;
    for (int i = 0; i < nr; i++) any_wide = any_wide || frame[(size_t)i] == 0;
    in.sg_layers = any_wide ? (in.user_chunk ? std::min(in.user_chunk, kChunkCap) : kChunkCap) : 1;
    in.walk_cap = kWalkCap; in.chunk_cap = kChunkCap;

    // the first pass, and the pass of a run that resumed below the hint
    std::vector<PlanStep> first, second;
    plan_pass(in, nr - 1, in.stop_at_hint_ok, first);
    if (in.stop_at_hint_ok && in.hint_layers < nr) {
      const int start = first.back().r_top - first.back().nc;
      PlanInput q = in; q.hint_layers = 0;
      if (start >= 0) plan_pass(q, start, false, second);
    }
    bool between = false;      // a two-kernel step with a walk step above and below it
    for (size_t i = 0; i + 2 < first.size(); i++)
      if (first[i].nb) for (size_t j = i + 1; j + 1 < first.size(); j++) if (!first[j].nb) for (size_t k = j + 1; k < first.size(); k++) if (first[k].nb) between = true;

    // every setting of the switches without saved layers; each saved-layer pattern (which rules the tail out) under one drawn setting
    for (int combo = 0; combo < (in.has_grid ? 8 : 11); combo++, cases++) {
      const int pattern = combo < 8 ? 0 : combo - 7, sw = combo < 8 ? combo : (int)(rng_x() % 8);
      // saved layers: none, some, a whole step (and some), all
      Heap<uint8_t> saved((size_t)nr, 0);
      if (pattern == 1 || pattern == 2) for (int i = 0; i < nr; i++) saved[(size_t)i] = rng_x() % 4 == 0;
      if (pattern == 2) { const PlanStep &s = first[rng_x() % first.size()]; for (int c = 0; c < s.nc; c++) saved[(size_t)(s.r_top - c)] = 1; }
      if (pattern == 3) for (int i = 0; i < nr; i++) saved[(size_t)i] = 1;
      const uint8_t *sv = pattern ? saved.get() : nullptr;
      const unsigned long long bits = rng_x();
      const bool pipelined = !in.has_grid && (bits & 3) != 0, vertical = bits & 4, has_lines = in.has_grid ? (bits & 8) != 0 : (bits & 0x38) != 0;

      TailIn ti;
      ti.ray_tail = sw & 1; ti.two_queues = sw & 2; ti.tail_direct = sw & 4;
      ti.stop_at_hint_ok = in.stop_at_hint_ok; ti.count = (bits >> 6) % 8 == 0; ti.has_lines = has_lines; ti.no_saved = sv == nullptr; ti.pipelined = pipelined;
      ti.nsh = (bits >> 9) % 16 == 0 ? 65537 : (bits >> 9) % 16 == 1 ? 65536 : 1000; ti.nwn = (bits >> 13) % 16 == 0 ? 65537 : 4000;
      ti.pass = &first; ti.host_spectrum = (bits >> 17) & 1; ti.any_product = (bits >> 18) % 4 == 0;
      const TailChoice tail = tail_choice(ti, kCaps);
      {   // plan_first_pass's four expressions
        const bool tail_mode = ti.ray_tail && ti.stop_at_hint_ok && !ti.count && has_lines && sv == nullptr &&
                               ti.nsh <= 65536 && ti.nwn <= kCaps.emis_rows_above && ti.nsh < 0x7fffffffLL / kCaps.tail_rays && plan_is_tail(first, kCaps.tail_steps);
        const bool tail_direct = tail_mode && ti.tail_direct, tail_spec = tail_direct && ti.host_spectrum && !ti.any_product;
        const bool two_queues = ti.two_queues && tail_direct && pipelined;
        g_checks++;
        if (!(tail.tail_mode == tail_mode && tail.tail_direct == tail_direct && tail.tail_spec == tail_spec && tail.two_queues == two_queues) && differ++ < 20)
          std::printf("case %d: tail_choice differs from the four expressions\n", cases);
      }

      ScheduleIn si;
      si.pipelined = pipelined; si.has_grid = in.has_grid; si.vertical = vertical; si.has_lines = has_lines; si.tail = tail; si.saved = sv; si.nr = nr;
      ScheduleState state;
      Parent par;
      par.plan = &first; par.pipelined = pipelined; par.has_grid = in.has_grid; par.vertical = vertical; par.has_lines = has_lines;
      par.saved = sv; par.nr = nr; par.tail_mode = tail.tail_mode; par.two_queues = tail.two_queues; par.out = &want;
      Rules rules(nr, pipelined, in.has_grid, has_lines, sv);

      const PassEnd ge = schedule_pass(first, si, kCaps, state, got);
      const PassEnd we = par.pass();
      compare(got, want, ge, we, "first pass");
      rules.pass(first, got, ge);

      // what the draws are there for
      const int form = !tail.tail_mode ? 0 : first.size() == 1 ? 1 : tail.two_queues ? 2 : 3;
      n_tail1 += form == 1; n_tail2q += form == 2 && first.size() == 2; n_tail1q += form == 3 && first.size() == 2;
      bool deferred = false, saved_step = false;
      for (const PlanStep &s : first) {
        bool all = sv != nullptr;
        for (int c = 0; c < s.nc && all; c++) all = sv[s.r_top - c] != 0;
        saved_step = saved_step || all;
        deferred = deferred || (!tail.tail_mode && !in.has_grid && pipelined && has_lines && s.nb && !s.last_step && !all);
      }
      n_deferred += deferred; n_saved_step += saved_step && pattern != 3; n_grid += in.has_grid;
      n_between += between && !tail.tail_mode && !in.has_grid && has_lines && pipelined && pattern == 0;

      if (!second.empty()) {
        si.tail = TailChoice{};
        par.plan = &second; par.resume();
        const PassEnd ge2 = schedule_pass(second, si, kCaps, state, got);
        const PassEnd we2 = par.pass();
        compare(got, want, ge2, we2, "resumed pass");
        rules.pass(second, got, ge2);
        n_res1 += form == 1; n_res2q += form == 2 && first.size() == 2; n_res1q += form == 3 && first.size() == 2;
      }
    }
  }
  std::printf("%d cases, %d differ\n", cases, differ);
  std::printf("rules: %ld checked, %ld violated\n", rule_checks, rule_bad);
  std::printf("(tails: %ld of one step, %ld of two steps on two queues, %ld of two steps on one queue; %ld passes with deferred side work, "
              "%ld with a two-kernel step between walks, %ld grid passes, %ld with a wholly saved step; resumed behind a tail: %ld, %ld, %ld)\n",
              n_tail1, n_tail2q, n_tail1q, n_deferred, n_between, n_grid, n_saved_step, n_res1, n_res2q, n_res1q);
  g_bad += differ;
  if (!differ && !rule_bad) std::printf("ok %ld\n", g_checks + rule_checks);
  return differ || rule_bad ? 1 : 0;
}
