// plan_check -- the step plan of a run (transit_amd/csrc/trx_plan.h) on seeded random layer profiles,
// depth hints, layer_chunk values, eager and opacity-grid modes: what every consumer of a plan relies on.
//   * the steps of a pass tile the layers from the top, no gap, no overlap, and stop at the bottom or the hint;
//   * a walk step holds walkable layers only and its frame is the widest of theirs; a two-kernel step
//     holds two-kernel layers only (but for a first step widened to its three layers);
//   * layers per step: within the form's cap, layer_chunk and the strength buffers;
//   * the first step has three layers (the 2- and 3-point rays);
//   * last_step marks the pass's last step and no other;
//   * a pass planned whole is the pass planned step by step;
//   * the tail predicate == one or two walk steps to the hint, counted here the plain way;
//   * the per-molecule sweep's steps (plan_sweep_step) tile nv-1 .. 0, each of one kind, within its cap (walk_cap or the
//     strength buffers' layers), its frame the widest of its layers: equal to the plain per-layer restatement.
// Prints "<cases> cases, <bad> differ".
#include <cstdio>
#include <cstdlib>
#include <random>
#include "trx_plan.h"

using namespace trx;

static int bad = 0;
#define EXPECT(cond)                                                                              \
  do { if (!(cond)) { if (bad++ < 20) std::printf("case %d step %d: %s\n", cases, (int)k, #cond); } } while (0)

int main(int argc, char **argv)
{
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 20000;
  const int kWalkCap = 64, kChunkCap = 32, kTailSteps = 2;
  std::mt19937_64 rng(20261), rng_sweep(20262);      // (the sweep's caps from a generator of their own: the runs' cases stay as they were)
  int cases = 0;
  for (int r = 0; r < rounds; r++, cases++) {
    const int nr = 3 + (int)(rng() % (r % 7 == 0 ? 300 : 120));
    // frames per layer (index 0 = bottom): widening with depth as real atmospheres do, or at random
    std::vector<int> frame((size_t)nr); std::vector<unsigned char> wide((size_t)nr);
    const int shape = (int)(rng() % 4);
    const int kinds[5] = {2, 4, 8, 16, 0};
    int level = (int)(rng() % 5);
    const bool wide_all = rng() % 2;             // every two-kernel layer is "very wide"
    for (int i = nr - 1; i >= 0; i--) {
      if (shape == 0) level = (int)(rng() % 5);
      else if (shape == 1) { if (rng() % 12 == 0 && level < 4) level++; }
      else if (shape == 2) { if (rng() % 40 == 0) level = (int)(rng() % 5); }
      else level = (rng() % 3 == 0) ? 4 : (int)(rng() % 4);
      frame[i] = kinds[level];
      wide[i] = frame[i] == 0 && (wide_all || rng() % 3 == 0);
    }
    PlanInput in;
    in.frame = frame.data(); in.very_wide = wide.data(); in.nr = nr;
    in.has_grid = r % 11 == 0; in.eager = r % 5 == 0;
    in.user_chunk = (rng() % 3 == 0) ? 3 + (int)(rng() % 70) : 0;
    in.hint_layers = (rng() % 4 == 0) ? 0 : 1 + (int)(rng() % (nr + 5));
    in.stop_at_hint_ok = !in.has_grid && !in.eager && in.hint_layers > 0 && in.hint_layers <= nr;
    bool any_wide = false;
    for (int i = 0; i < nr; i++) any_wide = any_wide || frame[i] == 0;
    in.sg_layers = any_wide ? (in.user_chunk ? std::min(in.user_chunk, kChunkCap) : kChunkCap) : 1;
    in.walk_cap = kWalkCap; in.chunk_cap = kChunkCap;

    // the per-molecule sweep's steps against the plain per-layer restatement: a step takes layers while they are of
    // r_top's kind and it is under its cap, and its frame is the widest met on the way
    {
      const int sg = 1 + (int)(rng_sweep() % 32), wcap = r % 3 == 0 ? 1 + (int)(rng_sweep() % kWalkCap) : kWalkCap;
      size_t k = 0;
      int at = nr - 1;
      std::vector<unsigned char> taken((size_t)nr, 0);
      for (; at >= 0; k++) {
        const PlanStep s = plan_sweep_step(frame.data(), at, wcap, sg);
        const bool walk = frame[at] != 0;
        int nc = 0, widest = 0;
        for (int i = at; i >= 0 && (frame[i] != 0) == walk && nc < (walk ? wcap : sg); i--) { nc++; widest = std::max(widest, frame[i]); }
        EXPECT(s.r_top == at && s.nc == nc && s.nb == (walk ? widest : 0));
        EXPECT(s.nc >= 1 && s.nc <= (s.nb ? wcap : sg) && s.r_top - s.nc >= -1);
        for (int c = 0; c < s.nc && s.r_top - c >= 0; c++) {
          EXPECT((frame[s.r_top - c] != 0) == (s.nb != 0) && frame[s.r_top - c] <= s.nb);      // one kind; the frame holds every layer's
          EXPECT(!taken[(size_t)(s.r_top - c)]);
          taken[(size_t)(s.r_top - c)] = 1;
        }
        EXPECT(s.last_step == (s.r_top - s.nc < 0));
        if (s.nc < 1) break;
        at -= s.nc;
      }
      k = 0;
      for (int i = 0; i < nr; i++) EXPECT(taken[(size_t)i]);                                   // the steps tile nr-1 .. 0
    }

    // a first pass (to the hint where the run stops there), and the pass of a run that resumed below the hint
    for (int second = 0; second < 2; second++) {
      const bool stop = second ? false : in.stop_at_hint_ok;
      int start = nr - 1;
      PlanInput q = in;
      if (second) {
        if (!in.stop_at_hint_ok || in.hint_layers >= nr) break;
        std::vector<PlanStep> first;
        plan_pass(in, nr - 1, true, first);
        start = first.back().r_top - first.back().nc;
        if (start < 0) break;
        q.hint_layers = 0;
      }
      std::vector<PlanStep> pass;
      plan_pass(q, start, stop, pass);
      size_t k = 0;
      EXPECT(!pass.empty());
      int at = start;
      for (k = 0; k < pass.size(); k++) {
        const PlanStep &s = pass[k];
        const PlanStep one = plan_step(q, at, stop);
        EXPECT(one.r_top == s.r_top && one.nc == s.nc && one.nb == s.nb && one.last_step == s.last_step);
        EXPECT(s.r_top == at && s.nc >= 1 && s.r_top - s.nc >= -1);
        const int swept = nr - 1 - s.r_top, after = swept + s.nc;
        const bool first_step = swept == 0;
        if (first_step) EXPECT(s.nc >= 3);
        int widest = 0; bool all_walk = true, all_two = true;
        for (int c = 0; c < s.nc; c++) {
          const int f = frame[s.r_top - c];
          widest = std::max(widest, f); all_walk = all_walk && f != 0; all_two = all_two && f == 0;
        }
        if (q.has_grid) {
          EXPECT(s.nb == 0);
          EXPECT(s.nc <= (q.user_chunk ? q.user_chunk : kChunkCap));
        } else if (s.nb) {
          EXPECT(all_walk && s.nb == widest);
          EXPECT(s.nc <= kWalkCap && (!q.user_chunk || s.nc <= q.user_chunk));
        } else {
          EXPECT(all_two || (first_step && s.nc == 3));
          EXPECT(s.nc <= kChunkCap && s.nc <= q.sg_layers && (!q.user_chunk || s.nc <= q.user_chunk));
          if (!q.user_chunk && !q.stop_at_hint_ok) EXPECT(s.nc <= 12);
          if (wide_all && all_two) EXPECT(s.nc <= 8);
          // a step of two-kernel layers alone, no layer_chunk: the run of such layers from r_top down (as far as the pass
          // goes) in equal parts under its cap -- 8 where the run's DEEPEST layer is "very wide", 12 with the depth unknown
          if (all_two && !q.user_chunk) {
            int togo = s.r_top + 1;
            if (!q.eager && q.hint_layers > swept) togo = std::min(togo, q.hint_layers - swept);
            int run = 1;
            while (run < togo && frame[s.r_top - run] == 0) run++;
            int cap = wide[s.r_top - run + 1] ? 8 : kChunkCap;
            if (!q.stop_at_hint_ok) cap = std::min(cap, 12);
            const int parts = (run + cap - 1) / cap;
            int want = (run + parts - 1) / parts;
            if (first_step) want = std::max(want, 3);
            EXPECT(s.nc == std::min(want, s.r_top + 1));
          }
        }
        // nothing below the hint in a pass that stops there (but for the first step's three layers)
        if (stop) EXPECT(after <= std::max(q.hint_layers, 3));
        const bool ends = s.r_top - s.nc < 0 || (stop && after >= q.hint_layers);
        EXPECT(s.last_step == ends);
        EXPECT(s.last_step == (k + 1 == pass.size()));
        at -= s.nc;
      }
      // the tail predicate against the plain count: steps from the top to the hint, all of them walks
      if (!second && in.stop_at_hint_ok) {
        int rr = nr - 1, steps = 0; bool ok = true;
        while (rr >= 0 && ok) {
          const PlanStep s = plan_step(in, rr, true);
          if (!s.nb || ++steps > kTailSteps) ok = false;
          rr -= s.nc;
          if (nr - 1 - rr >= in.hint_layers) break;
        }
        k = 0;
        EXPECT(plan_is_tail(pass, kTailSteps) == (ok && steps >= 1));
        if (plan_is_tail(pass, kTailSteps)) for (const PlanStep &s : pass) EXPECT(s.nb != 0 && s.nc <= kWalkCap);
      }
    }
  }
  std::printf("%d cases, %d differ\n", cases, bad);
  return bad ? 1 : 0;
}
