// sampler_stages.h -- the stage list of the sampler loops' ODE solvers: which time-table row, which time and which step
// size each stage of step i takes, and the one walk over the stages of a call.  The only place that knows the row
// convention and the two time formulas.  Plain C++ (no HIP types): tests/test_sampler_stages_cpu.py compiles it alone
// into a host program.
#pragma once

// solvers of the sampler loops (include/rgfm.h: RGFM_SOLVER_*)
constexpr int SOLVER_EULER = 0, SOLVER_MIDPOINT = 1;

struct Stage {
  // The stage's index within the call, 0 .. loop_stages - 1 in the order the stages run: its time-table row
  // (launch_stage_table), its diagnostics record (DiagSink::at) and its entry of a Strength's per-stage scale.
  int row;
  double t;    // the stage's own time: a stage is guided iff t > 1e-3
  float dts;   // out = base + dts * F(in, t); base is always the step's state
  bool reads_mid, writes_mid;  // in / out is the loop's mid-state buffer instead of the state
  int step;    // the global step index step_begin + i: what the stochastic step's noise is keyed by (sampler_host.h, Sde)
};

// stages of a call over `ns` steps
inline int loop_stages(int solver, int ns) { return ns * (solver == SOLVER_MIDPOINT ? 2 : 1); }

// The stages of step i of a call over [step_begin, ...) of num_steps.  Returns their number.
//   Euler:    one stage, row i, t = (step_begin + i) dt, in place.
//   Midpoint: mid = state + (dt / 2) F(state, t1) on row 2i, then state += dt F(mid, t1 + dt / 2) on row 2i + 1.
inline int step_stages(int solver, int num_steps, int step_begin, int i, Stage out[2]) {
  const double dtd = 1.0 / (double)num_steps;
  const double t1 = (double)(step_begin + i) * dtd;
  if (solver != SOLVER_MIDPOINT) {
    out[0] = {i, t1, (float)dtd, false, false, step_begin + i};
    return 1;
  }
  out[0] = {2 * i, t1, (float)(0.5 * dtd), false, true, step_begin + i};
  out[1] = {2 * i + 1, ((double)(step_begin + i) + 0.5) * dtd, (float)dtd, true, false, step_begin + i};
  return 2;
}

// The walk of every loop: f(const Stage&) -> int for the loop_stages(solver, ns) stages of a call over `ns` steps from
// step_begin, in order.  Stops at the first nonzero return and returns it; 0 after the last stage.
template <class F>
inline int for_each_stage(int solver, int num_steps, int step_begin, int ns, F&& f) {
  for (int i = 0; i < ns; ++i) {
    Stage st[2];
    const int n = step_stages(solver, num_steps, step_begin, i, st);
    for (int k = 0; k < n; ++k)
      if (int rc = f(st[k])) return rc;
  }
  return 0;
}
