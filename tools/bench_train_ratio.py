#!/usr/bin/env python3
"""Training throughput of the ratio estimators: one optimizer step (forward, loss, backward, Adam) at batch 128.

    python tools/bench_train_ratio.py [--kinds mnist_svhn mnist28 flexible] [--batch 128] [--steps 20] [--warmup 5]

For each kind it times (a) the HIP step (forward_train + the library's backward) and (b) the same step on a plain
torch.nn build of the same architecture on the same GPU (MIOpen convs, PyTorch autograd), both in training mode with
Dropout(0.1) and the discriminator loss on alternating real / fake rows, and prints one JSON line per kind: samples/s
of both and their ratio.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402

# kind: (HIP module, x shape, y shape, per encoder (in_ch, [(channels, pool_after)]), BatchNorm?, hidden widths / 512)
KINDS = {
    "mnist_svhn": (M.RatioEstimatorMNISTSVHN, (1, 32, 32), (3, 32, 32),
                   ((1, [(32, 1), (64, 1), (128, 1), (128, 0)]),
                    (3, [(64, 0), (64, 1), (128, 0), (128, 1), (256, 0), (256, 1), (256, 0), (256, 1)])), True, (512, 512, 256)),
    "mnist28": (M.RatioEstimator, (1, 28, 28), (1, 28, 28),
                ((1, [(32, 1), (64, 1), (128, 1), (128, 0)]), (1, [(32, 1), (64, 1), (128, 1), (128, 0)])), False, (512, 256)),
    # FlexibleRatioEstimator at the MNIST-SVHN shapes (the reference's RatioEstimatorMNISTSVHN_old preset)
    "flexible": (M.RatioEstimatorMNISTSVHN_old, (1, 32, 32), (3, 32, 32),
                 ((1, [(32, 1), (64, 1), (128, 1), (128, 0)]), (3, [(32, 1), (64, 1), (128, 1), (128, 0)])), False, (512, 256)),
}


class TorchEncoder(nn.Module):
    def __init__(self, in_ch, plan, batchnorm, feature_dim=256):
        super().__init__()
        layers, c = [], in_ch
        for cout, pool in plan:
            layers += [nn.Conv2d(c, cout, 3, padding=1), nn.BatchNorm2d(cout) if batchnorm else nn.GroupNorm(8, cout), nn.SiLU()]
            if pool:
                layers.append(nn.MaxPool2d(2))
            c = cout
        self.body = nn.Sequential(*layers)
        self.fc = nn.Linear(c, feature_dim)

    def forward(self, x):
        return self.fc(self.body(x).mean((2, 3)))


class TorchRatio(nn.Module):
    """The estimator as plain torch.nn layers (the MIOpen baseline)."""

    def __init__(self, encoders, batchnorm, widths, feature_dim=256):
        super().__init__()
        self.ex = TorchEncoder(*encoders[0], batchnorm, feature_dim)
        self.ey = TorchEncoder(*encoders[1], batchnorm, feature_dim)
        layers, c = [], 2 * feature_dim
        for i, w in enumerate(widths):
            layers += [nn.Linear(c, w), nn.LayerNorm(w), nn.SiLU()] + ([nn.Dropout(0.1)] if i < 2 else [])
            c = w
        self.score = nn.Sequential(*layers, nn.Linear(c, 1))

    def forward(self, x, y):
        return self.score(torch.cat([self.ex(x), self.ey(y)], 1)).squeeze(-1)


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", nargs="+", default=list(KINDS))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for kind in args.kinds:
        ctor, sx, sy, encoders, batchnorm, widths = KINDS[kind]
        B = args.batch
        x, y = torch.rand(B, *sx, device=dev) * 2 - 1, torch.rand(B, *sy, device=dev) * 2 - 1
        real = torch.arange(B, device=dev) % 2 == 0
        res = {"kind": kind, "batch": B, "steps": args.steps}
        for name, model, fwd in (("hip", ctor().to(dev), lambda m: m.forward_train),
                                 ("miopen", TorchRatio(encoders, batchnorm, widths).to(dev), lambda m: m)):
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)

            def step(model=model, opt=opt, f=fwd(model)):
                scores = f(x, y)
                loss = F.softplus(-scores[real]).mean() + F.softplus(scores[~real]).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
                loss.item()
            ms = time_steps(step, args.steps, args.warmup)
            res.update({f"{name}_ms": round(ms, 3), f"{name}_samples_per_s": round(B / ms * 1e3, 1)})
        res["hip_over_miopen"] = round(res["miopen_ms"] / res["hip_ms"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
