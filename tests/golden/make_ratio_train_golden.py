#!/usr/bin/env python3
"""Generate tests/golden/ratio_train_grad.npz from the reference's own autograd.

Run in the build container only (the reference never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ratio_train_golden.py

Cases: the reference RatioEstimatorMNISTSVHN in training and in eval mode and the reference RatioEstimator in training
mode, filled with this repo's synthetic parameters (ratio_guided_multimodal_fm_amd/synth.py, the seeds of
tests/helpers.py), every Dropout at p = 0, seeded Gaussian x and y, the discriminator loss on real = (arange(B) % 2 == 0),
loss.backward() in fp32.  Stored per case: the loss, the scores, dx and dy in full, the BatchNorm buffers after the
call and, per parameter tensor (named_parameters order), max |grad| and the gradient at 64 seeded probe positions.

A max-pool whose two largest window elements nearly tie may route differently in another fp32 implementation, which is
a discontinuity and not an error.  So the data seed of a case is the first one >= 900 whose smallest pool gap (largest
minus second-largest window element, float64 run) is at least ten times the largest fp32-vs-float64 deviation of any
pre-pool tensor in the reference's own run; both measured values and the seed are stored.  If no seed below 1000
qualifies at B = 4 the batch drops to 2, and the stored batch says so.  Where that still finds none (measured: the
MNIST-SVHN estimator, ~45 000 windows per sample, reaches a ratio of 6.6 in training and 2.6 in eval mode at best),
the B = 2 seed with the largest ratio is taken and the stored `rule` says 'best_ratio' instead of 'ten_times'
(search()).  Data only, no reference source.
"""
import copy
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ratio_guided_multimodal_fm_amd.synth import synth_state_dict  # noqa: E402
from src.models.ratio_estimator import RatioEstimator as RefRatio28  # noqa: E402
from src.models.ratio_flexible import RatioEstimatorMNISTSVHN as RefRatioMS  # noqa: E402

N_PROBE = 64
# case: (constructor, synthetic-weight seed of tests/helpers.py, x shape, y shape, training)
CASES = {
    "ms_train": (RefRatioMS, 16, (1, 32, 32), (3, 32, 32), True),
    "ms_eval": (RefRatioMS, 16, (1, 32, 32), (3, 32, 32), False),
    "r28_train": (RefRatio28, 15, (1, 28, 28), (1, 28, 28), True),
}

_pool_inputs = []
_max_pool2d = F.max_pool2d


def _recording_max_pool2d(inp, *a, **k):
    _pool_inputs.append(inp.detach())
    return _max_pool2d(inp, *a, **k)


F.max_pool2d = _recording_max_pool2d


def inputs(seed, batch, sx, sy):  # must match tests/test_gpu_ratio_train.py (golden_inputs)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, *sx, generator=g), torch.randn(batch, *sy, generator=g)


def probes(numel, i):
    return torch.randint(0, numel, (N_PROBE,), generator=torch.Generator().manual_seed(7000 + i)).numpy()


def disc_loss(scores):
    real = torch.arange(scores.shape[0]) % 2 == 0
    return (F.binary_cross_entropy_with_logits(scores[real], torch.ones_like(scores[real]))
            + F.binary_cross_entropy_with_logits(scores[~real], torch.zeros_like(scores[~real])))


def build(ctor, wseed, training, dtype):
    m = ctor()
    m.load_state_dict(synth_state_dict(m, wseed))
    for l in m.modules():
        if isinstance(l, torch.nn.Dropout):
            l.p = 0.0
    return m.to(dtype).train(training)


def pool_inputs_of(m, x, y):
    _pool_inputs.clear()
    with torch.no_grad():
        copy.deepcopy(m)(x, y)  # (a copy: training mode updates the buffers)
    return list(_pool_inputs)


def measure(ctor, wseed, training, x, y):
    """Per max-pool (forward order, x encoder first): (smallest gap in float64, largest fp32-vs-float64 deviation of its input)."""
    p32 = pool_inputs_of(build(ctor, wseed, training, torch.float32), x, y)
    p64 = pool_inputs_of(build(ctor, wseed, training, torch.float64), x.double(), y.double())
    res = []
    for a, t in zip(p32, p64):
        B, C, H, W = t.shape
        w = t[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        top = w.topk(2, dim=1).values
        res.append((float((top[:, 0] - top[:, 1]).min()), float((a.double() - t).abs().max())))
    return res


def search(ctor, wseed, training, sx, sy):
    """(seed, batch, rule, per-pool measurements).  Rule 'ten_times' is the stated condition.  Where no seed in
    [900, 1000) meets it at B = 4 or at B = 2, rule 'best_ratio' takes the B = 2 seed with the largest ratio of
    smallest gap to largest deviation, and the stored values say how far below ten it is."""
    best = None
    for batch in (4, 2):
        for seed in range(900, 1000):
            r = measure(ctor, wseed, training, *inputs(seed, batch, sx, sy))
            ratio = min(g for g, _ in r) / max(d for _, d in r)
            if ratio >= 10:
                return seed, batch, "ten_times", r
            if batch == 2 and (best is None or ratio > best[0]):
                best = (ratio, seed, r)
    return best[1], 2, "best_ratio", best[2]


def main():
    out = {}
    for tag, (ctor, wseed, sx, sy, training) in CASES.items():
        seed, batch, rule, per_pool = search(ctor, wseed, training, sx, sy)
        gap, dev = min(g for g, _ in per_pool), max(d for _, d in per_pool)
        print(f"{tag}: seed {seed} batch {batch} rule {rule} min pool gap {gap:.3e} max pre-pool fp32 deviation {dev:.3e}")
        out[f"{tag}_rule"] = np.array(rule)
        out[f"{tag}_pool_gap_dev"] = np.array(per_pool, np.float64)  # [pools][2] = (smallest gap, input deviation)
        m = build(ctor, wseed, training, torch.float32)
        x, y = inputs(seed, batch, sx, sy)
        x.requires_grad_(True), y.requires_grad_(True)
        scores = m(x, y)
        loss = disc_loss(scores)
        loss.backward()
        out[f"{tag}_seed"], out[f"{tag}_batch"] = np.int64(seed), np.int64(batch)
        out[f"{tag}_min_pool_gap"], out[f"{tag}_max_prepool_dev"] = np.float64(gap), np.float64(dev)
        out[f"{tag}_loss"] = np.float32(loss.item())
        out[f"{tag}_scores"] = scores.detach().numpy()
        out[f"{tag}_dx"], out[f"{tag}_dy"] = x.grad.numpy(), y.grad.numpy()
        for k, v in m.named_buffers():
            out[f"{tag}_buf_{k}"] = v.numpy()
        for i, (k, p) in enumerate(m.named_parameters()):
            gr = p.grad.reshape(-1)
            out[f"{tag}_amax_{i}"] = np.float32(gr.abs().max().item())
            out[f"{tag}_probe_{i}"] = gr[probes(gr.numel(), i)].numpy()
    np.savez_compressed(os.path.join(HERE, "ratio_train_grad.npz"), **out)


if __name__ == "__main__":
    main()
