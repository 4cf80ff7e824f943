"""float64 yardstick of a guidance strength per sample and per stage (tests/test_strength_cpu.py, test_gpu_strength.py).

Nothing is restated: the loops are COMPOSED from pinned pieces -- ode_ref64.integrate64 (the stepping rule) and its F_*
builders (the guided velocities).  The contract (include/rgfm.h): row b, stage k runs with gamma = float64(gamma_b) * s_k,
gamma_b an fp32 number; a stage with s_k == 0 runs unguided.

    per stage   F is built with gamma * s(t): integrate64 evaluates F at the stage's own time, which names the stage
                (the times are utils.diagnostics.stage_times, the formulas integrate64 uses)
    per row     each row is integrated on its own, with its own gamma, over the shared MC set

`make_F(gamma, row)` returns the F of the one-row state of row `row` (a builder of ode_ref64 with that row's ratio row
or condition), `unguided_F(row)` the loop's unguided F.
"""
import numpy as np

import ode_ref64 as O
from ratio_guided_multimodal_fm_amd.utils.diagnostics import stage_times
from ratio_guided_multimodal_fm_amd.utils.guidance_schedule import as_schedule


def scale_by_time(schedule, num_steps, solver, step_begin=0, step_end=None):
    """{stage time: s_k} of a call's stages; schedule None: 1 everywhere."""
    ts = stage_times(num_steps, solver, step_begin, step_end)
    vals = [1.0] * len(ts) if schedule is None else as_schedule(schedule).stage_values(num_steps, solver, step_begin, step_end)
    assert len(set(ts)) == len(ts)
    return dict(zip(ts, vals))


def scheduled(make_F, unguided_F, gamma, s_of):
    """F(state, t) = make_F(gamma * s(t))(state, t), the unguided F where s(t) == 0."""
    built = {}

    def F(s, t):
        k = s_of[t]
        if k == 0.0:
            return unguided_F(s, t)
        g = gamma * k
        if g not in built:
            built[g] = make_F(g)
        return built[g](s, t)
    return F


def integrate_rows64(make_F, unguided_F, state, gammas, num_steps, solver="euler", schedule=None, step_begin=0, step_end=None):
    """End state (tuple of float64 arrays, rows in order) of the loop with a strength per row and a scale per stage."""
    s_of = scale_by_time(schedule, num_steps, solver, step_begin, step_end)
    rows = []
    for b, g in enumerate(gammas):
        g64 = float(np.float32(g))  # gamma_b is an fp32 number, widened
        F = scheduled(lambda gg, b=b: make_F(gg, b), unguided_F(b), g64, s_of)
        rows.append(O.integrate64(F, tuple(np.asarray(a, np.float64)[b:b + 1] for a in state), num_steps, solver, step_begin, step_end))
    return tuple(np.concatenate([r[m] for r in rows]) for m in range(len(state)))


# ---- the four loops the builders of ode_ref64 cover (cross pairing has none there: it is pinned bitwise on the GPU)
def pair_mc(velx, vely, mx, my, r):
    """(make_F, unguided_F) of the paired MC loop over the shared MC set (mx [N, dx], my [N, dy], r [N], float64)."""
    return (lambda g, b: O.F_pair_mc(velx, vely, mx, my, r, g)), (lambda b: O.F_pair_mc(velx, vely, None, None, None, 0.0))


def cond_mc(vel, m, R):
    """... of the one-sided MC loop: row b weighs the MC set with its own ratio row R[b]."""
    return (lambda g, b: O.F_cond_mc(vel, m, R[b:b + 1], g)), (lambda b: O.F_single(vel))


def pair_grad(velx, vely, rr):
    return (lambda g, b: O.F_pair_grad(velx, vely, rr, g)), (lambda b: O.F_pair_mc(velx, vely, None, None, None, 0.0))


def cond_grad(vel, rr, cond, given):
    return (lambda g, b: O.F_cond_grad(vel, rr, cond[b:b + 1], given, g)), (lambda b: O.F_single(vel))
