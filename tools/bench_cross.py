#!/usr/bin/env python3
"""What cross pairing of the MC set costs: the paired MC loop at the benchmark shape (MNIST32 + SVHN, mc_feng, gamma
0.5, 100 Euler steps, batch 512, an MC set of 256) with the n_mc pairs (x1_i, y1_i) against all n_mc^2 pairs
(x1_i, y1_j), in one process.

    python tools/bench_cross.py [--batch 512] [--n_mc 256] [--steps 100] [--reps 3] [--diagnostics]
                                [--out profiles/cross/bench_cross.json]

Synthetic weights; one MC set, prepared once (the pre-phase is the same for both pairings and is not timed).  Two
pairs of windows, each timed with a host clock around work that ends in a device synchronise, alternating (paired,
cross, paired, cross, ...) after one warm-up of each, medians of --reps windows:

  ratio stage   RatioEngine.eval (the n_mc ratios of the pairs) against RatioEngine.eval_cross (the n_mc x n_mc matrix,
                each encoder run once per image)
  loop          one rgfm_sample_pair call from fresh noise against one rgfm_sample_pair_cross call.  The paired loop
                runs as it does by default (hipGraph replay of the guided step); the cross loop runs kernel by kernel
                and adds three launches per guided stage (a/b, the [B, N] x [N, N] products, the marginal weights).

Prints one JSON line and writes it to --out:
  ratio_vector_ms, ratio_matrix_ms        medians of the ratio stage;  *_min_max the spread
  paired_ms, cross_ms                     medians of a whole loop call;  *_min_max the spread
  paired_ms_per_stage, cross_ms_per_stage   the same divided by the number of stages (Euler: steps)
  cross_over_paired                       cross_ms / paired_ms
--diagnostics adds, from one more (untimed) call of each loop with a diagnostics sink, the median over the batch of the
effective sample size at a few stages: ess_paired (1 .. n_mc) and ess_cross (the joint one, 1 .. n_mc^2).  With
synthetic weights the ratios carry no coherence: the figures show the range, not a gain.
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


def alternate(fns, reps):
    """Median and (min, max) in ms of each of `fns`, timed in turn `reps` times after one warm-up of each."""
    for f in fns:
        f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(v), [min(v), max(v)]) for v in t]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--n_mc", type=int, default=256)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--gamma", type=float, default=0.5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--diagnostics", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross", "bench_cross.json"))
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
    x0, y0 = torch.randn(B, 1, 32, 32, device=dev, generator=g), torch.randn(B, 3, 32, 32, device=dev, generator=g)

    (rv, rv_mm), (rm, rm_mm) = alternate([lambda: rr._engine.eval(mx, my, "ratio"),
                                          lambda: rr._engine.eval_cross(mx, my, "ratio")], a.reps)
    r, R = rr._engine.eval(mx, my, "ratio"), rr._engine.eval_cross(mx, my, "ratio")

    def loop(ratios, rec=None):
        x, y = x0.clone(), y0.clone()
        _engine.sample_pair(fm, fs, x, y, mx, my, ratios, S, a.gamma, diag=rec)
        return x, y

    (tp, tp_mm), (tc, tc_mm) = alternate([lambda: loop(r), lambda: loop(R)], a.reps)
    res = {"batch": B, "n_mc": N, "steps": S, "gamma": a.gamma, "reps": a.reps,
           "ratio_vector_ms": rv, "ratio_vector_ms_min_max": rv_mm, "ratio_matrix_ms": rm, "ratio_matrix_ms_min_max": rm_mm,
           "paired_ms": tp, "paired_ms_min_max": tp_mm, "cross_ms": tc, "cross_ms_min_max": tc_mm,
           "paired_ms_per_stage": tp / S, "cross_ms_per_stage": tc / S, "cross_over_paired": tc / tp}
    if a.diagnostics:
        dp, dc = GuidanceDiagnostics(), GuidanceDiagnostics()
        loop(r, dp._begin("mc_feng", "euler", S, B, dev))
        loop(R, dc._begin("mc_feng", "euler", S, B, dev))
        stages = sorted({max(1, int(f * S)) for f in (0.1, 0.3, 0.6, 0.9)} & set(range(S)))
        res["ess_stages"] = stages
        res["ess_paired"] = [float(dp.ess()[k].median()) for k in stages]
        res["ess_cross"] = [float(dc.ess()[k].median()) for k in stages]
    res["range_fallbacks"] = _engine.range_fallbacks
    res["device"] = torch.cuda.get_device_name(0)
    res = {k: (round(v, 4) if isinstance(v, float) else [round(u, 4) if isinstance(u, float) else u for u in v]
               if isinstance(v, list) else v) for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
