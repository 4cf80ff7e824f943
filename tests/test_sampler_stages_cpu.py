"""The stage list of the sampler loops (csrc/sampler_stages.h: step_stages, and the loops' one walk over it,
for_each_stage) on the CPU: compiled with the host compiler and -fsanitize=address,undefined into a stand-alone program
(tests/sampler_stages_main.cpp), run for both solvers, and compared EXACTLY with the same quantities computed here:

  Euler:    row i,           t = (step_begin + i) / num_steps,        dts = float(1 / num_steps)
  Midpoint: rows 2i, 2i + 1, t = t1 and (step_begin + i + 0.5) / num_steps, dts = float(0.5 / num_steps), float(1 / num_steps)

num_steps in {1, 3, 2048}, step_begin in {0, 1, num_steps - 1}, every i of the range.

The walk visits exactly those stages in that order, a stage's row is its index in the walk -- 0, 1, ..., loop_stages - 1
-- and loop_stages is their count; a walk whose callback returns nonzero at its third stage returns that value having
visited exactly three.

A quotient k / num_steps above is formed the way every loop has always formed it, k * (1.0 / num_steps) in float64: that
product is what the guidance scalars and the `t > 1e-3` test are made of, so it is what "exact" has to mean here.  The
correctly rounded quotient is not always the same double (num_steps = 3: 2.5 / 3 = 0x1.aaaaaaaaaaaabp-1, the loops'
2.5 * (1.0 / 3) = 0x1.aaaaaaaaaaaaap-1); the test also asserts that the two never differ by more than one ulp.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ratio_guided_multimodal_fm_amd", "csrc")
EULER, MIDPOINT = 0, 1
CASES = [(solver, n, b) for solver in (EULER, MIDPOINT) for n in (1, 3, 2048) for b in sorted({0, 1, n - 1}) if b < n]


@pytest.fixture(scope="module")
def stage_lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the stage-list check needs the host g++"
    exe = str(tmp_path_factory.mktemp("stages") / "sampler_stages")
    # (both sanitizer runtimes linked statically: the program does not depend on what the environment preloads)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "sampler_stages_main.cpp"), "-o", exe])
    args = [str(v) for case in CASES for v in case]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True)
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    table, walks, counts, early = {}, {}, {}, []

    def stage(f):
        return (int(f[0]), float.fromhex(f[1]), float.fromhex(f[2]), int(f[3]), int(f[4]))
    for line in out.stdout.splitlines():
        kind, *f = line.split()
        if kind == "S":  # step_stages: (solver, n, b, i, k) -> stage
            key = tuple(int(v) for v in f[:5])
            assert key not in table
            table[key] = stage(f[5:])
        elif kind == "W":  # for_each_stage: (solver, n, b) -> its visits, in order
            visits = walks.setdefault(tuple(int(v) for v in f[:3]), [])
            assert int(f[3]) == len(visits)
            visits.append(stage(f[4:]))
        elif kind == "C":  # (solver, n, b) -> (visits, loop_stages, return value)
            counts[tuple(int(v) for v in f[:3])] = tuple(int(v) for v in f[3:])
        else:
            assert kind == "E", line
            early.append(tuple(int(v) for v in f))
    assert early == [(3, 7)]  # stopped at the third of six stages, and returned what the callback returned
    return table, walks, counts


def f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize("solver,n,b", CASES)
def test_stage_list_is_the_loops_formulas_exactly(stage_lines, solver, n, b):
    steps = range(n - b)
    want = {}
    for i in steps:
        t1, t2 = (b + i) * (1.0 / n), (b + i + 0.5) * (1.0 / n)
        assert abs(t1 - (b + i) / n) <= np.spacing(t1) and abs(t2 - (b + i + 0.5) / n) <= np.spacing(t2)
        if solver == EULER:
            want[(solver, n, b, i, 0)] = (i, t1, f32(1 / n), 0, 0)
        else:
            want[(solver, n, b, i, 0)] = (2 * i, t1, f32(0.5 / n), 0, 1)
            want[(solver, n, b, i, 1)] = (2 * i + 1, t2, f32(1 / n), 1, 0)
    table, walks, counts = stage_lines
    got = {k: v for k, v in table.items() if k[:3] == (solver, n, b)}
    assert len(want) == (1 + solver) * len(steps) and got == want
    # the walk: the same stages in (i, k) order, row = index, loop_stages = their count, 0 returned at the end
    walk = walks.get((solver, n, b), [])
    assert walk == [want[k] for k in sorted(want)]
    assert [g[0] for g in walk] == list(range(len(walk)))
    assert counts[(solver, n, b)] == (len(walk), len(walk), 0)
