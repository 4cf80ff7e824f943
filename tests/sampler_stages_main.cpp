// Prints the stage list of the sampler loops (csrc/sampler_stages.h) for tests/test_sampler_stages_cpu.py: one line per
// stage, "solver num_steps step_begin i k row t dts reads_mid writes_mid", t and dts as hex floats.  Host-only.
#include <cstdio>
#include <cstdlib>

#include "sampler_stages.h"

int main(int argc, char** argv) {
  for (int a = 1; a + 2 < argc; a += 3) {
    const int solver = atoi(argv[a]), num_steps = atoi(argv[a + 1]), step_begin = atoi(argv[a + 2]);
    for (int i = 0; i < num_steps - step_begin; ++i) {
      Stage st[2];
      const int n = step_stages(solver, num_steps, step_begin, i, st);
      for (int k = 0; k < n; ++k)
        printf("%d %d %d %d %d %d %a %a %d %d\n", solver, num_steps, step_begin, i, k, st[k].row, st[k].t, (double)st[k].dts,
               (int)st[k].reads_mid, (int)st[k].writes_mid);
    }
  }
  return 0;
}
