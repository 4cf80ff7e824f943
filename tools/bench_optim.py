#!/usr/bin/env python3
"""The optimizer step on its own: torch's pieces against the fused HIP step, per parameter list.

    python tools/bench_optim.py [--nets mnist32 svhn original clf_svhn ratio_ms] [--steps 200] [--warmup 20]
                                [--repeats 5] [--out profiles/train/bench_optim.jsonl]

For the parameter list of each net it times (a) `torch.optim.Adam` (its default, the foreach implementation) +
`torch.nn.utils.clip_grad_norm_(max_norm=1)` + a `torch._foreach_lerp_` EMA and (b) `utils.optim.Adam` with the same
settings (clip 1.0, EMA 0.999) -- both in one process, on gradients laid out as the training bridge returns them: views
into one blob in state_dict order, the buffers' slots dropped.  No forward or backward runs: a window is `--steps`
optimizer steps between two device events, enqueued without waiting, so it measures whichever of host and device is
the slower.  The two sides alternate, `--repeats` windows each; a line carries the median and the spread (min, max).
`floor_us` is the bytes the fused step has to move (p, m, v, ema read and written, g read twice: 40 bytes per element)
over the measured 6.29 TB/s HBM copy rate.  One JSON line per net, also written to --out.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.models.svhn_classifier import SVHNClassifier  # noqa: E402
from ratio_guided_multimodal_fm_amd.utils.optim import Adam  # noqa: E402

NETS = {"mnist32": lambda: M.FlowMatchingUNetMNIST(32), "svhn": M.FlowMatchingUNetSVHN, "original": M.FlowMatchingModel,
        "clf_svhn": SVHNClassifier, "ratio_ms": M.RatioEstimatorMNISTSVHN}
HBM_COPY_BYTES_PER_S = 6.29e12
BYTES_PER_ELEMENT = 40
MAX_NORM, DECAY = 1.0, 0.999


def bridge_grads(model):
    """Gradients as _TrainFn.backward hands them out: views of one blob in state_dict order, the buffers' slots dropped."""
    named = {id(p) for p in model.parameters()}
    layout = [(v.numel(), id(v) in named) for v in model.state_dict(keep_vars=True).values()]
    dev = next(model.parameters()).device
    blob = torch.randn(sum(k for k, _ in layout), device=dev) * 0.01
    chunks = torch.split(blob, [k for k, _ in layout])
    return [c.view(p.shape) for c, p in zip([c for c, (_, is_p) in zip(chunks, layout) if is_p], model.parameters())]


def window(step, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps * 1e3  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=list(NETS), choices=list(NETS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "bench_optim.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optim.py needs a HIP device: a time taken without one says nothing")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for net in args.nets:
        sides = {}
        for side in ("torch", "hip"):
            model = NETS[net]().to(dev)
            params = list(model.parameters())
            for p, g in zip(params, bridge_grads(model)):
                p.grad = g
            if side == "torch":
                opt = torch.optim.Adam(params, lr=1e-4)
                ema = [p.detach().clone() for p in params]

                def step(opt=opt, params=params, ema=ema):
                    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                    opt.step()
                    with torch.no_grad():
                        torch._foreach_lerp_(ema, params, 1 - DECAY)
            else:
                opt = Adam(params, lr=1e-4, max_grad_norm=MAX_NORM, ema_decay=DECAY)
                step = opt.step
            sides[side] = (step, model, opt)
        for step, _, _ in sides.values():
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        times = {side: [] for side in sides}
        for _ in range(args.repeats):
            for side, (step, _, _) in sides.items():
                times[side].append(window(step, args.steps))
        params = list(sides["hip"][1].parameters())
        numel = sum(p.numel() for p in params)
        res = {"net": net, "tensors": len(params), "elements": numel, "steps": args.steps, "repeats": args.repeats,
               "floor_us": round(numel * BYTES_PER_ELEMENT / HBM_COPY_BYTES_PER_S * 1e6, 2)}
        for side, ts in times.items():
            res.update({f"{side}_us": round(statistics.median(ts), 2), f"{side}_us_min": round(min(ts), 2),
                        f"{side}_us_max": round(max(ts), 2)})
        res["torch_over_hip"] = round(res["torch_us"] / res["hip_us"], 3)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
