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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--n_mc", type=int, default=256)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--reps", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    fm = load_synth(M.FlowMatchingUNetMNIST(32), 13).eval().to(dev)
    fs = load_synth(M.FlowMatchingUNetSVHN(), 14).eval().to(dev)
    rr = load_synth(M.RatioEstimatorMNISTSVHN(), 16).eval().to(dev)
    B, N, S = a.batch, a.n_mc, a.steps
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
