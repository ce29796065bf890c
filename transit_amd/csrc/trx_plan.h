// trx_plan.h -- the step plan of a run: which layers each top-down step takes, and in which form.
// Plain C++ (no HIP): shared by trx_api.hip and by tests/plan_check.cpp.  The plan depends on the
// layers' frames, the depth hint and the options alone -- on nothing the device produces -- so a
// pass is planned whole before its first step is queued.
#pragma once
#include <algorithm>
#include <vector>

namespace trx {

struct PlanInput {
  const int *frame = nullptr;                 // [nr] the walk's frame (bins) per layer, 0 = two-kernel form (walk_frame_bins)
  const unsigned char *very_wide = nullptr;   // [nr] profiles of 64+ cells: steps of such layers are capped at 8
  // hint_layers: layers the previous run needed (0: unknown); user_chunk: the caller's cap on layers per step (0: none);
  // sg_layers: layers the two-kernel form's strength buffers hold
  int nr = 0, hint_layers = 0, user_chunk = 0, sg_layers = 1;
  bool eager = false, has_grid = false, stop_at_hint_ok = false;      // (stop_at_hint_ok: the run plans its steps to end at the hint)
  int walk_cap = 64, chunk_cap = 32, blind_cap = 12;                   // kWalkLayers, kMaxChunk; two-kernel steps of a run that does not know its depth
};

struct PlanStep { int r_top, nc, nb; bool last_step; };      // layers r_top .. r_top-nc+1; nb: frame bins (0: grid / two-kernel)

// Layers still to go: down to the previous spectrum's depth when it is known (retrieval loops
// re-run near-identical atmospheres), else to the bottom.  The step takes the layers of ONE kind
// from r_top down -- walk or two-kernel form -- up to that kind's cap, in equal parts when more
// than one step is needed.
inline PlanStep plan_step(const PlanInput &in, int r_top, bool stop_at_hint)
{
  const int *fr = in.frame;
  const int swept = in.nr - 1 - r_top;
  int togo = r_top + 1;
  if (!in.eager && in.hint_layers > swept) togo = std::min(togo, in.hint_layers - swept);
  int nb = 0, nc;
  if (in.has_grid) nc = std::min(togo, in.user_chunk ? in.user_chunk : in.chunk_cap);
  else {
    nb = fr[r_top];
    int run = 1;                                 // consecutive layers of the same kind below r_top
    while (run < togo && (fr[r_top - run] == 0) == (nb == 0)) run++;
    int cap = nb ? in.walk_cap : in.chunk_cap;
    if (!nb && in.very_wide[std::max(0, r_top - run + 1)]) cap = 8;     // (a tile only learns between steps that its rays stopped)
    if (in.user_chunk) cap = std::min(cap, in.user_chunk);
    else if (!nb && !in.stop_at_hint_ok) cap = std::min(cap, in.blind_cap);      // depth unknown, expensive layers: small steps
    const int steps = (run + cap - 1) / cap;
    nc = (run + steps - 1) / steps;
    if (nb && steps > 1 && !in.user_chunk) {
      // A walk step costs what its WIDEST layer's frame costs, whatever the number of layers
      // (<= 64, one per lane), and frames grow with depth.  So this step takes the layers it
      // cannot leave to the later steps, and then as many more as share their frame: the wide
      // frames further down are paid for by as few lanes as possible.
      const int must = run - (steps - 1) * cap;
      int f = 0;
      for (int c = 0; c < must; c++) f = std::max(f, fr[r_top - c]);
      nc = must;
      while (nc < cap && nc < run && fr[r_top - nc] <= f) nc++;
    }
    if (nb) for (int c = 1; c < nc; c++) nb = std::max(nb, fr[r_top - c]);
  }
  if (swept == 0) nc = std::max(nc, 3);          // the first step holds the 2- and 3-point rays (eclipse.c:65-80)
  nc = std::min(nc, r_top + 1);
  if (nb && swept == 0) for (int c = 1; c < nc; c++) {          // (a widened first step stays one kind)
    if (fr[r_top - c] == 0) { nb = 0; break; }
    nb = std::max(nb, fr[r_top - c]);
  }
  if (!nb && !in.has_grid && nc > in.sg_layers) nc = in.sg_layers;
  // the plan's last step (bottom reached, or the depth the previous spectrum needed): its
  // combine and optical depth stay on the walk's queue
  const bool last = r_top - nc < 0 || (stop_at_hint && in.nr - 1 - (r_top - nc) >= in.hint_layers);
  return PlanStep{r_top, nc, nb, last};
}

// the steps of one pass from r_top down to its last step (out is reused: no allocation per run)
inline void plan_pass(const PlanInput &in, int r_top, bool stop_at_hint, std::vector<PlanStep> &out)
{
  out.clear();
  while (r_top >= 0) {
    out.push_back(plan_step(in, r_top, stop_at_hint));
    if (out.back().last_step) break;
    r_top -= out.back().nc;
  }
}

// The step of a per-molecule sweep (trx_sweep_permol): no hint, no first-step rule, every state to the bottom.
// The states of ONE kind from r_top down -- walk or two-kernel form -- up to that kind's cap; a walk step's
// frame is the widest of its states'.  frame: [nv] as PlanInput::frame.  (static: no new symbol of the library)
static inline PlanStep plan_sweep_step(const int *frame, int r_top, int walk_cap, int sg_layers)
{
  int nb = frame[r_top], nc = 1;
  const int cap = nb ? walk_cap : sg_layers;
  while (nc < cap && nc <= r_top && (frame[r_top - nc] == 0) == (nb == 0)) nc++;
  if (nb) for (int c = 1; c < nc; c++) nb = std::max(nb, frame[r_top - c]);
  return PlanStep{r_top, nc, nb, r_top - nc < 0};
}

// a pass to the hint that the ray tail can end (trx_tail.hip.h): 1 to tail_steps steps, every one a walk
inline bool plan_is_tail(const std::vector<PlanStep> &pass, int tail_steps)
{
  return !pass.empty() && (int)pass.size() <= tail_steps && std::all_of(pass.begin(), pass.end(), [](const PlanStep &s) { return s.nb != 0; });
}

}  // namespace trx
