#!/usr/bin/env python3
"""First numbers of conditional sampling (SVHN given MNIST32 images), beside the paired call in the same process.

    python tools/bench_cond.py [--batch 512] [--n_mc 256] [--steps 100] [--reps 3]

Synthetic weights and synthetic condition images (timing does not depend on the values).  Each phase is timed with a
host clock around work that ends in a device synchronise, after one untimed warm-up of the same shapes; the median of
--reps repetitions is reported.  Prints one JSON line:
  cross_ms       rgfm_ratio_eval_cross, batch x n_mc, RatioEstimatorMNISTSVHN
  prephase_ms    the MC pre-phase: n_mc rows of the target net, --steps unguided steps
  loop_ms        rgfm_sample_cond: batch rows, --steps steps
  cond_ms        a whole sample_conditional call (pre-phase + cross matrix + loop + noise); cond_images_per_s = batch / it
  pair_ms        a whole sample_bimodal_guided_mnist_svhn call at the same batch, n_mc, steps; pair_images_per_s

    python tools/bench_cond.py --guidance grad_log_ratio [--given mnist|svhn] [--batch 512] [--steps 100] [--reps 3]

times the gradient log-ratio conditional loop instead, per step, beside the same loop composed from the entry points
that existed before rgfm_sample_cond_grad.  Prints one JSON line:
  prepare_ms          rgfm_ratio_cond_prepare, batch condition images (once per call, outside the loop)
  loop_ms_per_step    rgfm_sample_cond_grad, batch rows, --steps steps in one call, divided by --steps
  base_ms_per_step    the baseline: per step the two-sided rgfm_ratio_grad_log_ratio at the current state with the
                      condition passed in again, one step of rgfm_sample_single (s += v dt, in place) and the axpy
                      s += gamma dt g in torch -- the same update from entry points older than the conditional one
  grad_cond_ms        one rgfm_ratio_grad_log_ratio_cond call (context prepared);  grad_both_ms  one two-sided call
  speedup_per_step    base_ms_per_step / loop_ms_per_step (medians; the two are timed in turn, *_min_max give the spread)
The baseline's host work between launches (two library calls and one torch kernel per step, a time table per call) is
part of what the one-call loop removes and is included.
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
from ratio_guided_multimodal_fm_amd.sample_mnist_svhn import sample_bimodal_guided_mnist_svhn  # noqa: E402
from ratio_guided_multimodal_fm_amd.synth import load_synth  # noqa: E402
from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up: code objects, workspaces, handles
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def timed_alternating(fa, fb, reps):
    """Medians and (min, max) of two callables timed in turn -- a, b, a, b, ... -- after one warm-up of each, so that a
    drift of the machine during the window falls on both alike."""
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


def bench_grad(a, fm, fs, rr, dev):
    B, S, gamma = a.batch, a.steps, 1.0
    given, target = ("x", fs) if a.given == "mnist" else ("y", fm)
    cshape, tshape = ((1, 32, 32), (3, 32, 32)) if given == "x" else ((3, 32, 32), (1, 32, 32))
    cond = torch.randn(B, *cshape, device=dev)
    eng = rr._engine
    ctx = eng.cond_prepare(cond, given)
    dt = 1.0 / S

    def baseline():
        s = torch.randn(B, *tshape, device=dev)
        for i in range(S):
            gx, gy, _ = eng.grad_log_ratio(*((cond, s) if given == "x" else (s, cond)))
            _engine.sample_single(target, s, S, i, i + 1)
            s.add_(gy if given == "x" else gx, alpha=gamma * dt)
        return s

    res = {"guidance": "grad_log_ratio", "given": a.given, "batch": B, "steps": S}
    res["prepare_ms"] = timed(lambda: eng.cond_prepare(cond, given), a.reps)
    s1 = torch.randn(B, *tshape, device=dev)
    res["grad_cond_ms"] = timed(lambda: eng.grad_log_ratio_cond(ctx, given, s1), a.reps)
    res["grad_both_ms"] = timed(lambda: eng.grad_log_ratio(*((cond, s1) if given == "x" else (s1, cond))), a.reps)
    loop = lambda: _engine.sample_cond_grad(target, rr, torch.randn(B, *tshape, device=dev), ctx, given, S, gamma)
    (lm, l0, l1), (bm, b0, b1) = timed_alternating(loop, baseline, a.reps)
    res["loop_ms_per_step"], res["loop_ms_per_step_min_max"] = lm / S, [round(l0 / S, 4), round(l1 / S, 4)]
    res["base_ms_per_step"], res["base_ms_per_step_min_max"] = bm / S, [round(b0 / S, 4), round(b1 / S, 4)]
    res["speedup_per_step"] = res["base_ms_per_step"] / res["loop_ms_per_step"]
    res["range_fallbacks"] = _engine.range_fallbacks
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--n_mc", type=int, default=256)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--guidance", default="mc_feng", choices=["mc_feng", "grad_log_ratio"])
    p.add_argument("--given", default="mnist", choices=["mnist", "svhn"], help="--guidance grad_log_ratio: the observed modality")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    fm = load_synth(M.FlowMatchingUNetMNIST(32), 13).eval().to(dev)
    fs = load_synth(M.FlowMatchingUNetSVHN(), 14).eval().to(dev)
    rr = load_synth(M.RatioEstimatorMNISTSVHN(), 16).eval().to(dev)
    B, N, S = a.batch, a.n_mc, a.steps
    if a.guidance == "grad_log_ratio":
        return bench_grad(a, fm, fs, rr, dev)
    cond = torch.randn(B, 1, 32, 32, device=dev)
    mc = torch.randn(N, 3, 32, 32, device=dev)
    _engine.sample_single(fs, mc, S)
    ratios = rr.cross_log_ratio(cond, mc).exp()
    res = {"batch": B, "n_mc": N, "steps": S}
    res["cross_ms"] = timed(lambda: rr.cross_log_ratio(cond, mc), a.reps)
    res["prephase_ms"] = timed(lambda: _engine.sample_single(fs, torch.randn(N, 3, 32, 32, device=dev), S), a.reps)
    res["loop_ms"] = timed(lambda: _engine.sample_cond(fs, torch.randn(B, 3, 32, 32, device=dev), mc, ratios, S, 1.0), a.reps)
    res["cond_ms"] = timed(lambda: sample_conditional(fs, rr, cond, "x", S, 1.0, N), a.reps)
    res["pair_ms"] = timed(lambda: sample_bimodal_guided_mnist_svhn(fm, fs, rr, "mc_feng", 1.0, B, S, dev, N), a.reps)
    res["cond_images_per_s"] = B / (res["cond_ms"] * 1e-3)
    res["pair_images_per_s"] = B / (res["pair_ms"] * 1e-3)
    res["cross_share_of_cond"] = res["cross_ms"] / res["cond_ms"]
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
