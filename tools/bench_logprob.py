#!/usr/bin/env python3
"""What one stage of the likelihood loop costs: forward + K reverse walks to x + the state update, at the SVHN and
MNIST-32 presets -- the data-only walk (rgfm_unet_divergence) beside the same stage composed from the training entry
points, `forward_train(x, t)` followed by `torch.autograd.grad(v, x, eps)`, which runs the whole rgfm_unet_backward
(every weight, bias, norm and time-path gradient) to get at dL/dx.

    python tools/bench_logprob.py [--batch 128] [--n_probes 1] [--stages 10] [--reps 11] [--out profiles/logprob/bench_logprob.jsonl]

Synthetic weights and N(0, 1) inputs (timing does not depend on the values).  The composed stage pays one forward and
one backward per probe (its saved state is released by the backward); the new one pays one forward per stage.
Protocol: a host clock around --stages stages that end in a device synchronise, one untimed warm-up of each route, the
two routes timed in turn (a, b, a, b, ...), the median of --reps windows with min and max.  Before timing, the two
routes are compared on the same inputs: v and J^T eps must agree to the bit, the per-row dot products to fp32 rounding.
Appends one JSON line per preset to --out.  Says nothing about likelihoods of trained checkpoints.
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

from ratio_guided_multimodal_fm_amd import _lib  # noqa: E402
from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.synth import load_synth  # noqa: E402

PRESETS = {"svhn": (lambda: M.FlowMatchingUNetSVHN(), 14, (3, 32, 32)),
           "mnist32": (lambda: M.FlowMatchingUNetMNIST(32), 13, (1, 32, 32))}


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
    return ta, tb


def stats(ts, stages):
    return {"ms_per_stage": statistics.median(ts) / stages, "min": min(ts) / stages, "max": max(ts) / stages}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=128)
    p.add_argument("--n_probes", type=int, default=1)
    p.add_argument("--stages", type=int, default=10, help="stages per timed window")
    p.add_argument("--reps", type=int, default=11)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprob", "bench_logprob.jsonl"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    B, K, dt = a.batch, a.n_probes, 0.01
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, (ctor, seed, shape) in PRESETS.items():
        m = load_synth(ctor(), seed).eval().to(dev)
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(B, *shape, device=dev, generator=g)
        t = torch.full((1,), 0.5, device=dev)
        eps = torch.randint(0, 2, (K, B, *shape), device=dev, generator=g).float() * 2 - 1

        def vjp_stage(x):
            v, div = m.divergence(x, t, eps)
            return x - dt * v, div

        def composed_stage(x):
            div = torch.zeros(B, device=dev)
            for k in range(K):
                xg = x.detach().requires_grad_(True)
                v = m.forward_train(xg, t)
                (gk,) = torch.autograd.grad(v, xg, eps[k])
                div += (eps[k] * gk).flatten(1).sum(1)
            return x - dt * v.detach(), div / K

        def run(stage):
            s = x
            for _ in range(a.stages):
                s, _ = stage(s)

        # same inputs, both routes: v and J^T eps to the bit, the dot products to rounding
        xn_a, div_a = vjp_stage(x)
        xn_b, div_b = composed_stage(x)
        xg = x.detach().requires_grad_(True)
        (g_b,) = torch.autograd.grad(m.forward_train(xg, t), xg, eps[0])
        same_bits = bool(torch.equal(xn_a, xn_b) and torch.equal(m.vjp(x, t, eps[0]), g_b))
        div_diff = float((div_a - div_b).abs().max())
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib().rgfm_unet_log_prob_workspace_bytes(m._engine.handle(dev), B, _lib.SOLVERS["midpoint"], K,
                                                                 ctypes.byref(nbytes)))
        ta, tb = timed_alternating(lambda: run(vjp_stage), lambda: run(composed_stage), a.reps)
        sa, sb = stats(ta, a.stages), stats(tb, a.stages)
        res = {"preset": name, "batch": B, "n_probes": K, "stages_per_window": a.stages, "reps": a.reps,
               "vjp_stage_ms": sa["ms_per_stage"], "vjp_stage_ms_min_max": [round(sa["min"], 3), round(sa["max"], 3)],
               "composed_stage_ms": sb["ms_per_stage"], "composed_stage_ms_min_max": [round(sb["min"], 3), round(sb["max"], 3)],
               "composed_over_vjp": sb["ms_per_stage"] / sa["ms_per_stage"],
               "v_and_vjp_bit_equal": same_bits, "div_max_abs_diff": div_diff, "div_max_abs": float(div_a.abs().max()),
               "log_prob_workspace_mib_midpoint": nbytes.value / 2 ** 20}
        line = json.dumps({k: (float(f"{v:.5g}") if isinstance(v, float) else v) for k, v in res.items()})
        print(line)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
