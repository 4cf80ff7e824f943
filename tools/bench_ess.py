#!/usr/bin/env python3
"""What the effective-sample-size floor costs: the mc_feng paired loop of the MNIST32 + SVHN presets with ess_floor = 8
beside the same loop without it, in one process; and the two weights kernels (guid_weights_kernel,
guid_weights_ess_kernel) through the block that launches them.

    python tools/bench_ess.py [--batch 512] [--n_mc 256] [--steps 100] [--reps 5] [--floor 8] [--out profiles/ess/bench_ess.json]

Protocol of tools/bench_sde.py: synthetic weights (timing does not depend on the values); the MC set is integrated and
its ratios are evaluated once, outside the timed region; a host clock around work that ends in a device synchronise, one
untimed warm-up of each, the two timed in turn (a, b, a, b, ...), the median of --reps with min and max.  The loop
without a floor runs as it does by default (hipGraph replay included when RGFM_GRAPH has it on); the loop with one runs
kernel by kernel.  With synthetic weights the states stay far from the MC set and every row of every guided stage is
collapsed: each pays the 40 bisection steps, the floor's worst case.

The weights kernels: the block rgfm_guidance_apply_rows / rgfm_guidance_apply_ess at [batch, n_mc] with the smallest
flattened sizes (8 + 4), where the distance and apply launches are a few microseconds each -- 200 calls between two
device events, with every row collapsed (rows on an MC sample at t = 0.99: 40 bisection steps each) and with no row
below the floor (t = 0.2, a tight MC set: the sibling's extra work is one ESS and one logf per sample).  The difference
of two block times is the difference of the two weights kernels; the block times themselves include three launches.
Prints one JSON line and writes it to --out.  Says nothing about sample quality.
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


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def block_us(B, N, t, collapsed, floor, dev, calls=200):
    """Microseconds per block call without and with the floor, and the fraction of rows the floor tempered."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    dx, dy = 8, 4
    if collapsed:
        m = 0.5 * torch.randn(N, dx + dy, generator=g)
        x = t * m[torch.randint(0, N, (B,), generator=g)] + 1e-4 * torch.randn(B, dx + dy, generator=g)
    else:
        sigma = 1 - t + 1e-3
        c0 = torch.randn(dx + dy, generator=g)
        m = c0 + 0.5 * sigma / (t * (dx + dy) ** 0.5) * torch.randn(N, dx + dy, generator=g)
        x = t * c0 + 0.25 * sigma / (dx + dy) ** 0.5 * torch.randn(B, dx + dy, generator=g)
    d = {"x": x[:, :dx], "y": x[:, dx:], "mx": m[:, :dx], "my": m[:, dx:], "vx": torch.randn(B, dx, generator=g),
         "vy": torch.randn(B, dy, generator=g), "r": torch.exp(0.2 * torch.randn(N, generator=g))}
    d = {k: v.contiguous().to(dev) for k, v in d.items()}
    rows = torch.full((B,), 0.5, device=dev)
    tau = torch.zeros(B, device=dev)
    nb = ctypes.c_size_t()
    _lib.check(L.rgfm_guidance_workspace_bytes(B, N, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (_p(d["x"]), _p(d["y"]), _p(d["vx"]), _p(d["vy"]), _p(d["mx"]), _p(d["my"]), _p(d["r"]), B, N, dx, dy, float(t), _p(rows),
            None)

    def plain():
        _lib.check(L.rgfm_guidance_apply_rows(*head, _p(ws), nb.value, s))

    def floored():
        _lib.check(L.rgfm_guidance_apply_ess(*head, float(floor), _p(tau), _p(ws), nb.value, s))

    out = []
    for fn in (plain, floored):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return out[0], out[1], float((tau < 1).float().mean())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--n_mc", type=int, default=256)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--floor", type=float, default=8.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ess", "bench_ess.json"))
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
    tau = torch.zeros(S, B, device=dev)

    def loop(floor):
        x, y = torch.randn(B, 1, 32, 32, device=dev), torch.randn(B, 3, 32, 32, device=dev)
        _engine.sample_pair(fm, fs, x, y, mx, my, r, S, 1.0, ess_floor=floor, tau=tau if floor else None)

    (pm, p0, p1), (em, e0, e1) = timed_alternating(lambda: loop(None), lambda: loop(a.floor), a.reps)
    tempered = float((tau[1:] < 1).float().mean())
    kc_plain, kc_ess, kc_frac = block_us(B, N, 0.99, True, a.floor, dev)
    kh_plain, kh_ess, kh_frac = block_us(B, N, 0.2, False, a.floor, dev)
    res = {"batch": B, "n_mc": N, "guidance": "mc_feng", "gamma": 1.0, "steps": S, "reps": a.reps, "ess_floor": a.floor,
           "graph_env": os.environ.get("RGFM_GRAPH", ""),
           "plain_ms": pm, "plain_ms_min_max": [round(p0, 3), round(p1, 3)], "plain_ms_per_step": pm / S,
           "floor_ms": em, "floor_ms_min_max": [round(e0, 3), round(e1, 3)], "floor_ms_per_step": em / S,
           "floor_over_plain": em / pm, "overhead_us_per_step": (em - pm) / S * 1e3,
           "rows_tempered_in_the_loop": tempered,
           "block_us_all_rows_collapsed": {"plain": kc_plain, "floor": kc_ess, "weights_kernel_difference": kc_ess - kc_plain,
                                           "rows_tempered": kc_frac},
           "block_us_no_row_below_the_floor": {"plain": kh_plain, "floor": kh_ess, "weights_kernel_difference": kh_ess - kh_plain,
                                               "rows_tempered": kh_frac},
           "range_fallbacks": _engine.range_fallbacks}

    def rnd(v):
        return round(v, 4) if isinstance(v, float) else {k: rnd(x) for k, x in v.items()} if isinstance(v, dict) else v
    line = json.dumps({k: rnd(v) for k, v in res.items()})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
