#!/usr/bin/env python3
"""Training throughput of the evaluation classifiers: one optimizer step (forward, cross-entropy, backward, Adam) at
batch 128.

    python tools/bench_train_clf.py [--kinds mnist28 mnist32 svhn] [--batch 128] [--steps 100] [--warmup 10]
                                    [--repeats 3] [--only hip|miopen] [--out profiles/train/bench_train_clf.jsonl]

For each kind it times (a) the HIP step (forward_train, the fused cross-entropy kernel, the library's backward, Adam)
and (b) the same step of the same module through its plain torch forward on the same GPU (MIOpen convs, rocBLAS
Linears, PyTorch autograd), both in training mode with the module's Dropout, and prints one JSON line per kind:
samples/s of both and their ratio.  A step ends in loss.item(), so the window between the two device events holds
finished work.  The two sides are timed in alternating windows, `--repeats` of each; the line carries the median
window and the spread (min, max) beside it.  The lines are also written to --out.  `--only hip` is the form to put
behind `rocprofv3 --kernel-trace --stats --` for the per-kernel table.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from ratio_guided_multimodal_fm_amd.models.classifier import MNISTClassifier  # noqa: E402
from ratio_guided_multimodal_fm_amd.models.svhn_classifier import MNISTClassifier32, SVHNClassifier  # noqa: E402
from ratio_guided_multimodal_fm_amd.utils.trainer import ClassifierTrainer  # noqa: E402

KINDS = {"mnist28": (MNISTClassifier, (1, 28, 28)), "mnist32": (MNISTClassifier32, (1, 32, 32)),
         "svhn": (SVHNClassifier, (3, 32, 32))}


def window(step, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["hip", "miopen"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "bench_train_clf.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_clf.py needs a HIP device: a time taken without one says nothing")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for kind in args.kinds:
        ctor, shape = KINDS[kind]
        B = args.batch
        x = torch.rand(B, *shape, device=dev) * 2 - 1
        labels = torch.arange(B, device=dev) % 10
        steps = {}
        if args.only != "miopen":
            hip = ctor().to(dev).train()
            trainer = ClassifierTrainer(hip, torch.optim.Adam(hip.parameters(), lr=1e-3), dev)
            steps["hip"] = lambda trainer=trainer: trainer.train_step(x, labels)[0].item()
        if args.only != "hip":
            ref = ctor().to(dev).train()
            opt = torch.optim.Adam(ref.parameters(), lr=1e-3)

            def step_ref(ref=ref, opt=opt):
                loss = F.cross_entropy(ref(x), labels)
                opt.zero_grad()
                loss.backward()
                opt.step()
                loss.item()
            steps["miopen"] = step_ref
        for step in steps.values():
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        times = {name: [] for name in steps}
        for _ in range(args.repeats):
            for name, step in steps.items():
                times[name].append(window(step, args.steps))
        res = {"kind": kind, "batch": B, "steps": args.steps, "repeats": args.repeats}
        for name, ts in times.items():
            ms = statistics.median(ts)
            res.update({f"{name}_ms": round(ms, 3), f"{name}_ms_min": round(min(ts), 3), f"{name}_ms_max": round(max(ts), 3),
                        f"{name}_samples_per_s": round(B / ms * 1e3, 1)})
        if "hip_ms" in res and "miopen_ms" in res:
            res["hip_over_miopen"] = round(res["miopen_ms"] / res["hip_ms"], 3)
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
