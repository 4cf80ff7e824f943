#!/usr/bin/env python3
"""First numbers of class-conditional sampling and classifier-free guidance on the svhn preset.

    python tools/bench_cfg.py [--batch 512] [--steps 100] [--reps 3] [--classes 10]

Synthetic weights (timing does not depend on the values).  The three loops are timed in turn -- a, b, c, a, b, c, ... --
with a host clock around one call that ends in a device synchronise, after one untimed warm-up of each, so that a drift
of the machine during the window falls on all three alike; medians and (min, max) of --reps repetitions are reported.
Prints one JSON line:
  plain_ms        (a) rgfm_sample_single on the labelled net WITHOUT labels: today's single loop (the null row)
  cond_ms         (b) labels with cfg_scale = 1: one evaluation per stage + one gather of the rows' time table
  cfg_ms          (c) labels with cfg_scale = 3: two evaluations per stage + the blend kernel
  cond_over_plain, cfg_over_plain   the two ratios (expected near 1 and near 2)
  blend_gbps, blend_us              (d) the blend kernel alone over the state of one stage (batch x 3 x 32 x 32 floats),
                                    200 launches back to back (rgfm_ubench_cfg_blend): GB/s of the 16 bytes per element
  blend_big_gbps                    ... over 64 Mi floats, where the launch is long enough to show a rate
  hbm_copy_gbps                     the measured float4 copy rate of the device (rgfm_ubench_hbm_copy, 1 GiB)
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


def timed_in_turn(fns, reps):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for fn, ts in zip(fns, out):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(ts), min(ts), max(ts)) for ts in out]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--classes", type=int, default=10)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    B, S, K = a.batch, a.steps, a.classes
    net = load_synth(M.FlowMatchingUNetSVHN(num_classes=K), 14).eval().to(dev)
    labels = (torch.arange(B) % K).to(dev)
    x0 = torch.randn(B, 3, 32, 32, device=dev)
    loops = [lambda: _engine.sample_single(net, x0.clone(), S),
             lambda: _engine.sample_single(net, x0.clone(), S, labels=labels, cfg_scale=1.0),
             lambda: _engine.sample_single(net, x0.clone(), S, labels=labels, cfg_scale=3.0)]
    (pm, p0, p1), (cm, c0, c1), (gm, g0, g1) = timed_in_turn(loops, a.reps)
    res = {"preset": "svhn", "batch": B, "steps": S, "classes": K, "reps": a.reps,
           "plain_ms": pm, "plain_ms_min_max": [round(p0, 2), round(p1, 2)],
           "cond_ms": cm, "cond_ms_min_max": [round(c0, 2), round(c1, 2)],
           "cfg_ms": gm, "cfg_ms_min_max": [round(g0, 2), round(g1, 2)],
           "cond_over_plain": cm / pm, "cfg_over_plain": gm / pm}
    L = _lib.lib()
    gb, us = ctypes.c_double(), ctypes.c_double()
    _lib.check(L.rgfm_ubench_cfg_blend(B * 3 * 32 * 32, ctypes.byref(gb), ctypes.byref(us)))
    res["blend_gbps"], res["blend_us"] = gb.value, us.value
    _lib.check(L.rgfm_ubench_cfg_blend(64 << 20, ctypes.byref(gb), ctypes.byref(us)))
    res["blend_big_gbps"] = gb.value
    _lib.check(L.rgfm_ubench_hbm_copy(1 << 30, ctypes.byref(gb)))
    res["hbm_copy_gbps"] = gb.value
    res["range_fallbacks"] = _engine.range_fallbacks
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
