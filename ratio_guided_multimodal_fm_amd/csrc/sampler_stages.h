// sampler_stages.h -- the stage list of the sampler loops' ODE solvers: which time-table row, which time and which step
// size each stage of step i takes.  The only place that knows the row convention and the two time formulas.  Plain C++
// (no HIP types): tests/test_sampler_stages_cpu.py compiles it alone into a host program.
#pragma once

// solvers of the sampler loops (include/rgfm.h: RGFM_SOLVER_*)
constexpr int SOLVER_EULER = 0, SOLVER_MIDPOINT = 1;

struct Stage {
  int row;     // time-table row of the stage (launch_stage_table)
  double t;    // the stage's own time: a stage is guided iff t > 1e-3
  float dts;   // out = base + dts * F(in, t); base is always the step's state
  bool reads_mid, writes_mid;  // in / out is the loop's mid-state buffer instead of the state
};

// The stages of step i of a call over [step_begin, ...) of num_steps.  Returns their number.
//   Euler:    one stage, row i, t = (step_begin + i) dt, in place.
//   Midpoint: mid = state + (dt / 2) F(state, t1) on row 2i, then state += dt F(mid, t1 + dt / 2) on row 2i + 1.
inline int step_stages(int solver, int num_steps, int step_begin, int i, Stage out[2]) {
  const double dtd = 1.0 / (double)num_steps;
  const double t1 = (double)(step_begin + i) * dtd;
  if (solver != SOLVER_MIDPOINT) {
    out[0] = {i, t1, (float)dtd, false, false};
    return 1;
  }
  out[0] = {2 * i, t1, (float)(0.5 * dtd), false, true};
  out[1] = {2 * i + 1, ((double)(step_begin + i) + 0.5) * dtd, (float)dtd, true, false};
  return 2;
}
