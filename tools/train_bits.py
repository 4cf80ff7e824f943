#!/usr/bin/env python3
"""Bits and workspace sizes of the training passes that run on the shared conv-block kernels (the ratio estimators and
the evaluation classifiers), for a same-box A/B of two trees: one line per case -- name, *_train_workspace_bytes, SHA-256
of every output.  Only the package's public functions, a raw C-ABI size query and the case builders of
tests/test_gpu_ratio_train.py, tests/test_gpu_clf_train.py and tests/test_gpu_ratio_flex.py, so the same file runs
unchanged in a worktree of an earlier commit:

    python3 tools/train_bits.py > new.txt
    (cd ../parent && python3 tools/train_bits.py) > parent.txt
    diff parent.txt new.txt

Outputs per case, in this order: score or logits; the image gradient(s); every parameter gradient as one blob
(state_dict order); the BatchNorm buffers behind the call (what bn_stats_out turned them into; no BatchNorm: the hash of
nothing); every pool's choice map; for the classifiers every gate.

Cases: each in training and in eval mode, with dropout at 0 and at 0.1 under a fixed seed.
  classifiers, B in {2, 3, 17} and 1 in eval mode (17: more samples than BatchNorm slices, slices of 2 with a last of 1)
    mnist28   no norm, 28 -> 14 -> 7: rows that are no multiple of 8, the one-float pool and unpool
    mnist32   no norm, the four-float pool; a last block without a pool, gated on its own
    svhn      BatchNorm, four floats; two BatchNorm blocks without a pool, whose backward applies the gate
  ratio estimators, B in {2, 5, 17} and 1 in eval mode
    ratio_ms  BatchNorm, 32 x 32
    ratio28   GroupNorm, 28 -> 14 -> 7 -> 3: the odd raster whose last row and column lie in no pool window
    flex_2x12_4x12  12 -> 6 -> 3
    flex_1x8_1x8
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import test_gpu_clf_train as CT  # noqa: E402
import test_gpu_ratio_flex as FX  # noqa: E402
import test_gpu_ratio_train as RT  # noqa: E402
from helpers import make_module  # noqa: E402
from ratio_guided_multimodal_fm_amd import _lib  # noqa: E402
from ratio_guided_multimodal_fm_amd.utils.losses import cross_entropy  # noqa: E402

SEED = 99
MODES = [(training, p) for training in (True, False) for p in (0.0, 0.1)]


def sha(tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def ws_bytes(engine, dev, n):
    nb = ctypes.c_size_t()
    _lib.check(engine._fn("train_workspace_bytes")(engine.handle(dev), n, ctypes.byref(nb)))
    return nb.value


def buffers(m):
    return [v for k, v in m.state_dict().items() if "running" in k]


def line(name, m, dev, n, out, dins, rest):
    grads = [p.grad for p in m.parameters()]
    print(name, ws_bytes(m._engine, dev, n), sha([out]), *[sha([d]) for d in dins], sha(grads), sha(buffers(m)),
          *[sha([t]) for t in rest], flush=True)


def batches(training, sizes):
    return sizes if training else (1,) + sizes


def classifier(kind, dev):
    for training, p in MODES:
        for B in batches(training, (2, 3, 17)):
            m = make_module(CT.TAGS[kind], dev)
            m.dropout.p = p
            x, labels = CT.inputs(kind, B)
            m.train(training)
            xg = x.to(dev).requires_grad_(True)
            torch.cuda.manual_seed(SEED)
            logits = m.forward_train(xg)
            choices = [c for c in m._engine.pool_choices() if c is not None]
            gates = m._engine.gates()
            cross_entropy(logits, labels.to(dev))[0].backward()
            line(f"clf_{kind}/{'train' if training else 'eval'}/p{p}/B{B}", m, dev, B, logits, [xg.grad], choices + gates)


def ratio(name, make, inputs, dev):
    for training, p in MODES:
        for B in batches(training, (2, 5, 17)):
            m = make()
            RT.set_dropout(m, p)
            x, y = inputs(B)
            m.train(training)
            xg, yg = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
            torch.cuda.manual_seed(SEED)
            scores = m.forward_train(xg, yg)
            choices = [c for enc in m._engine.pool_choices() for c in enc]
            RT.loss_of(scores, RT.real_mask(B), "disc").backward()
            line(f"{name}/{'train' if training else 'eval'}/p{p}/B{B}", m, dev, B, scores, [xg.grad, yg.grad], choices)


def flex_inputs(ci):
    (xc, xs), (yc, ys) = FX.CASES[ci]

    def inputs(B):
        g = torch.Generator().manual_seed(7300 + 100 * ci + B)
        return torch.randn(B, xc, xs, xs, generator=g), torch.randn(B, yc, ys, ys, generator=g)
    return inputs


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    _lib.lib()
    for kind in ("mnist28", "mnist32", "svhn"):
        classifier(kind, dev)
    for tag in ("ratio_ms", "ratio28"):
        ratio(tag, lambda tag=tag: make_module(tag, dev), lambda B, tag=tag: RT.inputs(tag, B), dev)
    for name, ci in (("flex_2x12_4x12", 1), ("flex_1x8_1x8", 0)):
        assert FX.CASES[ci] == {1: ((2, 12), (4, 12)), 0: ((1, 8), (1, 8))}[ci]
        ratio(name, lambda ci=ci: FX.module(ci, dev), flex_inputs(ci), dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
