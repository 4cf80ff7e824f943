#!/usr/bin/env python3
"""Generate tests/golden/clf_train_grad.npz from the reference's own autograd.

Run in the build container only (the reference never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_clf_golden.py

Cases: the reference MNISTClassifier, MNISTClassifier32 and SVHNClassifier in training mode and the SVHNClassifier in
eval mode too, filled with this repo's synthetic parameters (ratio_guided_multimodal_fm_amd/synth.py, the seeds of
tests/helpers.py), Dropout at p = 0, B = 4 seeded Gaussian images, labels (arange(B) * 3 + 1) % 10, F.cross_entropy,
loss.backward() in fp32.  Stored per case: the loss, the logits and dx in full, the BatchNorm buffers after the call,
per parameter tensor (named_parameters order) max |grad| and the gradient at 64 seeded probe positions, and the
decisions the reference took -- per max-pool the window element (0..3, from max_pool2d's own indices) and per ReLU the
gate (bit-packed; a conv block's on its output raster, behind a pool the gate of the element taken).  The SVHN net has
2.3 M parameters: full gradients would not fit in a fixture.

A max-pool whose two largest window elements nearly tie, or a pre-activation next to zero, may be decided differently
by another fp32 implementation, which is a discontinuity and not an error.  So the data seed of a case is the first one
in [900, 1000) for which the smallest pool gap (largest minus second-largest element of a window whose maximum is
positive, float64 run) and the smallest |pre-activation| are each at least ten times the largest fp32-vs-float64
deviation of any pre-activation in the reference's own run (rule 'ten_times').  Where no seed qualifies (measured:
the SVHN net in training mode, 7.2 at best) the seed with the largest ratio is taken and the stored `rule` says
'best_ratio'; the measured values are stored either way.  Data only, no reference source.
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
from src.models.classifier import MNISTClassifier as RefMnist28  # noqa: E402
from src.models.svhn_classifier import MNISTClassifier32 as RefMnist32, SVHNClassifier as RefSvhn  # noqa: E402

N_PROBE = 64
BATCH = 4
# case: (constructor, synthetic-weight seed of tests/helpers.py, image shape, training)
CASES = {
    "mnist28_train": (RefMnist28, 21, (1, 28, 28), True),
    "mnist32_train": (RefMnist32, 17, (1, 32, 32), True),
    "svhn_train": (RefSvhn, 18, (3, 32, 32), True),
    "svhn_eval": (RefSvhn, 18, (3, 32, 32), False),
}

_relu_inputs, _pool_inputs = [], []
_relu, _max_pool2d = F.relu, F.max_pool2d


def _recording_relu(inp, *a, **k):
    _relu_inputs.append(inp.detach())
    return _relu(inp, *a, **k)


def _recording_max_pool2d(inp, *a, **k):
    _pool_inputs.append(inp.detach())
    return _max_pool2d(inp, *a, **k)


F.relu, F.max_pool2d = _recording_relu, _recording_max_pool2d


def inputs(seed, shape):  # must match tests/test_clf_train_cpu.py and tests/test_gpu_clf_train.py (golden_inputs)
    return torch.randn(BATCH, *shape, generator=torch.Generator().manual_seed(seed))


def labels():
    return (torch.arange(BATCH) * 3 + 1) % 10


def probes(numel, i):
    return torch.randint(0, numel, (N_PROBE,), generator=torch.Generator().manual_seed(7000 + i)).numpy()


def build(ctor, wseed, training, dtype):
    m = ctor()
    m.load_state_dict(synth_state_dict(m, wseed))
    m.dropout.p = 0.0
    return m.to(dtype).train(training)


def recorded(m, x):
    _relu_inputs.clear(), _pool_inputs.clear()
    with torch.no_grad():
        copy.deepcopy(m)(x)  # (a copy: training mode updates the buffers)
    return list(_relu_inputs), list(_pool_inputs)


def windows(t):
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)


def measure(ctor, wseed, training, x):
    """(smallest pool gap, smallest |pre-activation|, largest fp32-vs-float64 deviation of a pre-activation)."""
    r32, _ = recorded(build(ctor, wseed, training, torch.float32), x)
    r64, p64 = recorded(build(ctor, wseed, training, torch.float64), x.double())
    gap = float("inf")
    for t in p64:
        top = windows(t).topk(2, dim=1).values
        live = top[:, 0] > 0
        gap = min(gap, float((top[live, 0] - top[live, 1]).min()))
    small = min(float(t.abs().min()) for t in r64)
    dev = max(float((a.double() - t).abs().max()) for a, t in zip(r32, r64))
    return gap, small, dev


def search(ctor, wseed, training, shape):
    best = None
    for seed in range(900, 1000):
        gap, small, dev = measure(ctor, wseed, training, inputs(seed, shape))
        ratio = min(gap, small) / dev
        if ratio >= 10:
            return seed, "ten_times", (gap, small, dev)
        if best is None or ratio > best[0]:
            best = (ratio, seed, (gap, small, dev))
    return best[1], "best_ratio", best[2]


def decisions(m, x):
    """The reference's own decisions in its fp32 run: per ReLU the gate on the layer's output raster, per conv block
    the pool's choice (None without a pool).  The pools follow the first ReLUs, one each."""
    relu_in, pool_in = recorded(m, x)
    gates, choices = [], []
    for i, y in enumerate(relu_in):
        if i < len(pool_in):
            W = y.shape[-1]
            _, idx = _max_pool2d(pool_in[i], 2, return_indices=True)
            choices.append(((idx // W) % 2 * 2 + (idx % W) % 2).to(torch.uint8))
            taken = y.flatten(2).gather(2, idx.flatten(2)).view_as(idx)
            gates.append(taken > 0)
        else:
            choices.append(None)
            gates.append(y > 0)
    return gates, choices[:-1]  # (the last ReLU is fc1's)


def main():
    out = {}
    for tag, (ctor, wseed, shape, training) in CASES.items():
        seed, rule, (gap, small, dev) = search(ctor, wseed, training, shape)
        print(f"{tag}: seed {seed} rule {rule} min pool gap {gap:.3e} min |pre-activation| {small:.3e} "
              f"max fp32 deviation {dev:.3e}")
        out[f"{tag}_rule"], out[f"{tag}_seed"] = np.array(rule), np.int64(seed)
        out[f"{tag}_min_pool_gap"], out[f"{tag}_min_abs_pre"] = np.float64(gap), np.float64(small)
        out[f"{tag}_max_pre_dev"] = np.float64(dev)
        m = build(ctor, wseed, training, torch.float32)
        x = inputs(seed, shape)
        gates, choices = decisions(m, x)
        for i, g in enumerate(gates):
            out[f"{tag}_gate_{i}"] = np.packbits(g.numpy().reshape(-1))
        for i, c in enumerate(choices):
            if c is not None:
                out[f"{tag}_choice_{i}"] = c.numpy()
        x.requires_grad_(True)
        logits = m(x)
        loss = F.cross_entropy(logits, labels())
        loss.backward()
        out[f"{tag}_loss"] = np.float32(loss.item())
        out[f"{tag}_logits"] = logits.detach().numpy()
        out[f"{tag}_dx"] = x.grad.numpy()
        for k, v in m.named_buffers():
            out[f"{tag}_buf_{k}"] = v.numpy()
        for i, (k, p) in enumerate(m.named_parameters()):
            gr = p.grad.reshape(-1)
            out[f"{tag}_amax_{i}"] = np.float32(gr.abs().max().item())
            out[f"{tag}_probe_{i}"] = gr[probes(gr.numel(), i)].numpy()
    np.savez_compressed(os.path.join(HERE, "clf_train_grad.npz"), **out)


if __name__ == "__main__":
    main()
