#!/usr/bin/env python3
"""What guidance diagnostics cost: the paired MC loop at BASELINE configs[2] (MNIST32 + SVHN, mc_feng, gamma 0.5,
100 Euler steps, batch 512, an MC set of 256) with and without a diagnostics sink, in one process.

    python tools/bench_diag.py [--batch 512] [--n_mc 256] [--steps 100] [--reps 5] [--out profiles/diag/bench_diag.json]

Synthetic weights, one MC set and ratio vector prepared once (the pre-phase is not part of either window).  A window is
one rgfm_sample_pair call from fresh noise -- the default path replays its hipGraph, the one with diagnostics runs
kernel by kernel and adds the statistics launches and one more guided-velocity GEMM per step -- timed with a host
clock around work that ends in a device synchronise.  The two are timed in turn (off, on, off, on, ...) after one
warm-up of each; the medians and (min, max) of --reps windows are reported, and the states of the two paths are
compared bitwise once.  Prints one JSON line and writes it to --out:
  off_ms, on_ms             medians of a whole loop call;  *_min_max the spread
  on_over_off               on_ms / off_ms
  extra_ms_per_step         (on_ms - off_ms) / steps
  same_bits                 the state with diagnostics on equals the state with them off
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
from ratio_guided_multimodal_fm_amd.utils.diagnostics import GuidanceDiagnostics  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--n_mc", type=int, default=256)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--gamma", type=float, default=0.5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag", "bench_diag.json"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    fm = load_synth(M.FlowMatchingUNetMNIST(32), 13).eval().to(dev)
    fs = load_synth(M.FlowMatchingUNetSVHN(), 14).eval().to(dev)
    rr = load_synth(M.RatioEstimatorMNISTSVHN(), 16).eval().to(dev)
    B, N, S = a.batch, a.n_mc, a.steps
    g = torch.Generator(device=dev).manual_seed(5)
    mx, my = torch.randn(N, 1, 32, 32, device=dev, generator=g), torch.randn(N, 3, 32, 32, device=dev, generator=g)
    _engine.sample_two_streams(fm, mx, fs, my, S)
    r = rr._engine.eval(mx, my, "ratio")
    x0, y0 = torch.randn(B, 1, 32, 32, device=dev, generator=g), torch.randn(B, 3, 32, 32, device=dev, generator=g)
    diag = GuidanceDiagnostics()

    def run(on):
        x, y = x0.clone(), y0.clone()
        rec = diag._begin("mc_feng", "euler", S, B, dev) if on else None
        _engine.sample_pair(fm, fs, x, y, mx, my, r, S, a.gamma, diag=rec)
        return x, y

    (xa, ya), (xb, yb) = run(False), run(True)  # warm-up of both paths
    torch.cuda.synchronize()
    same = bool(torch.equal(xa, xb) and torch.equal(ya, yb))
    t = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(on)
            torch.cuda.synchronize()
            t[on].append((time.perf_counter() - t0) * 1e3)
    off, on = statistics.median(t[False]), statistics.median(t[True])
    s = diag.summary(diag.stage_of_step(int(0.3 * S)))
    res = {"batch": B, "n_mc": N, "steps": S, "gamma": a.gamma, "reps": a.reps,
           "off_ms": off, "off_ms_min_max": [min(t[False]), max(t[False])],
           "on_ms": on, "on_ms_min_max": [min(t[True]), max(t[True])],
           "on_over_off": on / off, "extra_ms_per_step": (on - off) / S, "same_bits": same,
           "ess_mean_at_step_30pct": s["ess_mean"], "range_fallbacks": _engine.range_fallbacks,
           "device": torch.cuda.get_device_name(0)}
    res = {k: (round(v, 4) if isinstance(v, float) else [round(u, 4) for u in v] if isinstance(v, list) else v)
           for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
