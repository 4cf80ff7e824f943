// Prints the stage list of the sampler loops (csrc/sampler_stages.h) for tests/test_sampler_stages_cpu.py.  Host-only.
// Per case (solver num_steps step_begin), over the steps step_begin .. num_steps - 1:
//   "S solver num_steps step_begin i k row t dts reads_mid writes_mid"  step_stages, one line per stage
//   "W solver num_steps step_begin visit row t dts reads_mid writes_mid" for_each_stage, one line per visit, in order
//   "C solver num_steps step_begin visits loop_stages ret"               the walk's count, loop_stages and return value
// and once "E visits ret": a midpoint walk over 3 steps whose f returns 7 at its third stage.  t and dts as hex floats.
#include <cstdio>
#include <cstdlib>

#include "sampler_stages.h"

int main(int argc, char** argv) {
  for (int a = 1; a + 2 < argc; a += 3) {
    const int solver = atoi(argv[a]), num_steps = atoi(argv[a + 1]), step_begin = atoi(argv[a + 2]);
    const int ns = num_steps - step_begin;
    for (int i = 0; i < ns; ++i) {
      Stage st[2];
      const int n = step_stages(solver, num_steps, step_begin, i, st);
      for (int k = 0; k < n; ++k)
        printf("S %d %d %d %d %d %d %a %a %d %d\n", solver, num_steps, step_begin, i, k, st[k].row, st[k].t,
               (double)st[k].dts, (int)st[k].reads_mid, (int)st[k].writes_mid);
    }
    int visits = 0;
    const int ret = for_each_stage(solver, num_steps, step_begin, ns, [&](const Stage& g) {
      printf("W %d %d %d %d %d %a %a %d %d\n", solver, num_steps, step_begin, visits++, g.row, g.t, (double)g.dts,
             (int)g.reads_mid, (int)g.writes_mid);
      return 0;
    });
    printf("C %d %d %d %d %d %d\n", solver, num_steps, step_begin, visits, loop_stages(solver, ns), ret);
  }
  int visits = 0;
  const int ret = for_each_stage(SOLVER_MIDPOINT, 3, 0, 3, [&](const Stage&) { return ++visits == 3 ? 7 : 0; });
  printf("E %d %d\n", visits, ret);
  return 0;
}
