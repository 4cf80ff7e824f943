#!/usr/bin/env python3
"""What the stochastic step costs: the mc_feng paired loop of the MNIST32 + SVHN presets with sde_eta = 1 beside the same
loop with sde_eta = 0 (the ODE), in one process; and the step's pre-update kernel alone against its copy-rate bound.

    python tools/bench_sde.py [--batch 512] [--n_mc 256] [--steps 100] [--reps 5] [--out profiles/sde/bench_sde.json]

Protocol of tools/bench_solver.py: synthetic weights (timing does not depend on the values); the MC set is integrated
and its ratios are evaluated once, outside the timed region; a host clock around work that ends in a device synchronise,
one untimed warm-up of each, the two timed in turn (a, b, a, b, ...), the median of --reps with min and max.  The
eta = 0 loop runs as it does by default (hipGraph replay included when RGFM_GRAPH has it on); the eta = 1 loop runs
kernel by kernel, so the overhead printed here is the pre-update kernels plus whatever the lost replay costs.

The kernel alone (rgfm_ubench_sde_pre: 200 launches between two device events): it moves 8 bytes per element, so its
bound is 8 n bytes over the measured HBM copy rate (rgfm_ubench_hbm_copy, read + written bytes); timed at the loop's
own size, batch x (1 + 3) x 1024 floats -- where the state fits the on-die cache, so the "fraction of the bound" can
exceed 1 -- and at 2^28 floats, where it cannot.  Prints one JSON line and writes it to --out.  Says nothing about sample
quality.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from ratio_guided_multimodal_fm_amd import _engine, _lib  # noqa: E402
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


def kernel_alone(n):
    gb, us = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().rgfm_ubench_sde_pre(n, ctypes.byref(gb), ctypes.byref(us)))
    return gb.value, us.value


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--n_mc", type=int, default=256)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--eta", type=float, default=1.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde", "bench_sde.json"))
    a = p.parse_args()
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

    def loop(eta):
        x, y = torch.randn(B, 1, 32, 32, device=dev), torch.randn(B, 3, 32, 32, device=dev)
        _engine.sample_pair(fm, fs, x, y, mx, my, r, S, 1.0, sde_eta=eta, sde_seed=1)

    (om, o0, o1), (sm, s0, s1) = timed_alternating(lambda: loop(0.0), lambda: loop(a.eta), a.reps)
    gb = ctypes.c_double()
    _lib.check(_lib.lib().rgfm_ubench_hbm_copy(1 << 30, ctypes.byref(gb)))
    copy_gbps = gb.value
    n_loop, n_big = B * 4 * 1024, 1 << 28
    (loop_gbps, loop_us), (big_gbps, big_us) = kernel_alone(n_loop), kernel_alone(n_big)
    res = {"batch": B, "n_mc": N, "guidance": "mc_feng", "gamma": 1.0, "steps": S, "reps": a.reps, "eta": a.eta,
           "graph_env": os.environ.get("RGFM_GRAPH", ""),
           "ode_ms": om, "ode_ms_min_max": [round(o0, 3), round(o1, 3)], "ode_ms_per_step": om / S,
           "sde_ms": sm, "sde_ms_min_max": [round(s0, 3), round(s1, 3)], "sde_ms_per_step": sm / S,
           "sde_over_ode": sm / om, "overhead_us_per_step": (sm - om) / S * 1e3,
           "hbm_copy_gbps": copy_gbps,
           "pre_update_floats_per_step": n_loop, "pre_update_bytes_per_step": 8 * n_loop,
           "pre_update_us_at_loop_size": loop_us, "pre_update_gbps_at_loop_size": loop_gbps,
           "pre_update_bound_us_at_loop_size": 8 * n_loop / (copy_gbps * 1e9) * 1e6,
           "pre_update_fraction_of_copy_rate_at_loop_size": loop_gbps / copy_gbps,
           "pre_update_us_at_2p28": big_us, "pre_update_gbps_at_2p28": big_gbps,
           "pre_update_fraction_of_copy_rate_at_2p28": big_gbps / copy_gbps,
           "range_fallbacks": _engine.range_fallbacks}
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
