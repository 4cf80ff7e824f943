#!/usr/bin/env python3
"""What a midpoint step costs beside an Euler step: the mc_feng paired loop of the MNIST32 + SVHN presets, Euler at
--steps steps beside midpoint at --steps / 2 steps (the same number of network evaluations), in one process.

    python tools/bench_solver.py [--batch 512] [--n_mc 256] [--steps 100] [--reps 5] [--out profiles/ode/bench_solver.json]

Synthetic weights (timing does not depend on the values); the MC set is integrated and its ratios are evaluated once,
outside the timed region: what is timed is rgfm_sample_pair (Euler) and rgfm_sample_pair_ode (midpoint) on fresh noise.
Protocol of tools/bench_cond.py: a host clock around work that ends in a device synchronise, one untimed warm-up of
each, the two timed in turn (a, b, a, b, ...), the median of --reps with min and max.  "Network evaluation" = one stage
of the loop: both velocity nets once plus, on a guided stage, the guidance block -- an Euler step is one, a midpoint
step two.  Prints one JSON line and writes it to --out.  Says nothing about sample quality.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from ratio_guided_multimodal_fm_amd import _engine  # noqa: E402
from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.synth import load_synth  # noqa: E402


def timed_alternating(fa, fb, reps):
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, out in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--n_mc", type=int, default=256)
    p.add_argument("--steps", type=int, default=100, help="Euler steps; midpoint runs half as many")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ode", "bench_solver.json"))
    a = p.parse_args()
    if a.steps % 2:
        p.error("--steps must be even")
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    fm = load_synth(M.FlowMatchingUNetMNIST(32), 13).eval().to(dev)
    fs = load_synth(M.FlowMatchingUNetSVHN(), 14).eval().to(dev)
    rr = load_synth(M.RatioEstimatorMNISTSVHN(), 16).eval().to(dev)
    B, N, S = a.batch, a.n_mc, a.steps
    mx, my = torch.randn(N, 1, 32, 32, device=dev), torch.randn(N, 3, 32, 32, device=dev)
    _engine.sample_two_streams(fm, mx, fs, my, S)
    r = rr._engine.eval(mx, my, "ratio")

    def loop(steps, solver):
        x, y = torch.randn(B, 1, 32, 32, device=dev), torch.randn(B, 3, 32, 32, device=dev)
        _engine.sample_pair(fm, fs, x, y, mx, my, r, steps, 1.0, solver=solver)

    (em, e0, e1), (mm, m0, m1) = timed_alternating(lambda: loop(S, "euler"), lambda: loop(S // 2, "midpoint"), a.reps)
    res = {"batch": B, "n_mc": N, "guidance": "mc_feng", "gamma": 1.0, "reps": a.reps,
           "euler_steps": S, "euler_ms": em, "euler_ms_min_max": [round(e0, 3), round(e1, 3)], "euler_ms_per_net_eval": em / S,
           "midpoint_steps": S // 2, "midpoint_ms": mm, "midpoint_ms_min_max": [round(m0, 3), round(m1, 3)],
           "midpoint_ms_per_net_eval": mm / S, "midpoint_step_over_euler_step": (mm / (S // 2)) / (em / S),
           "range_fallbacks": _engine.range_fallbacks}
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
