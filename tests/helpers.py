"""Shared test plumbing: synthetic-weight modules, oracle descriptors, fixtures."""
import functools
import os

import numpy as np
import torch

from oracle import oracle as O
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth, paired_noise  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# must match tests/golden/make_golden.py
SEED_W = {"unet28": 11, "unet28_y": 12, "mnist32": 13, "svhn": 14, "ratio28": 15, "ratio_ms": 16,
          "clf_mnist": 17, "clf_svhn": 18, "fm_original": 19, "fm_original_y": 20, "clf_mnist28": 21}
N_PROBE = 256

_CTORS = {
    "unet28": lambda: M.FlowMatchingUNet(),
    "unet28_y": lambda: M.FlowMatchingUNet(),
    "mnist32": lambda: M.FlowMatchingUNetMNIST(32),
    "svhn": lambda: M.FlowMatchingUNetSVHN(),
    "ratio28": lambda: M.RatioEstimator(),
    "ratio_ms": lambda: M.RatioEstimatorMNISTSVHN(),
    "fm_original": lambda: M.FlowMatchingModel(),
    "fm_original_y": lambda: M.FlowMatchingModel(),
    "clf_mnist28": lambda: __import__("ratio_guided_multimodal_fm_amd.models.classifier", fromlist=["x"]).MNISTClassifier(),
    "clf_mnist": lambda: __import__("ratio_guided_multimodal_fm_amd.models.svhn_classifier", fromlist=["x"]).MNISTClassifier32(),
    "clf_svhn": lambda: __import__("ratio_guided_multimodal_fm_amd.models.svhn_classifier", fromlist=["x"]).SVHNClassifier(),
}


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def make_module(tag, device=None):
    m = load_synth(_CTORS[tag](), SEED_W[tag]).eval()
    return m.to(device) if device is not None else m


@functools.lru_cache(maxsize=None)
def oracle_net(tag):
    """(descriptor-or-kind, fp32 parameter blob) for the CPU oracle."""
    m = make_module(tag)
    blob = O.blob_of(m)
    if tag.startswith("ratio"):
        return ("mnist_svhn" if tag == "ratio_ms" else "mnist28"), blob
    return O.desc_of(m), blob


def probe_idx(numel, salt):
    g = torch.Generator().manual_seed(900 + salt)
    return torch.randint(0, numel, (N_PROBE,), generator=g).numpy()


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def oracle_fm_pair(blob_x, blob_y, ratio_blob, noise, guided, gamma, steps):
    """paired_sampler with two FlowMatchingModel nets, composed from oracle pieces
    (reference src/utils/flow_utils.py:186-278 as driven by src/sample.py --model original)."""
    x, y, mx, my = (None if a is None else a.numpy().copy() for a in noise)
    dt = np.float32(1.0 / steps)
    r = None
    if guided:
        for s in range(steps):
            t = np.array([s * (1.0 / steps)], np.float32)
            mx = mx + O.fm_forward(blob_x, mx, t) * dt
            my = my + O.fm_forward(blob_y, my, t) * dt
        r = O.ratio_eval("mnist28", ratio_blob, mx, my, "ratio", "disc")
    for s in range(steps):
        t = s * (1.0 / steps)
        tv = np.array([t], np.float32)
        vx, vy = O.fm_forward(blob_x, x, tv), O.fm_forward(blob_y, y, tv)
        if guided and t > 1e-3:
            vx, vy = O.guidance_apply(x, y, vx, vy, mx, my, r, t, gamma)[:2]
        x, y = x + vx * dt, y + vy * dt
    return x, y


# must match tests/golden/make_golden.py
GENERIC_UNETS = {
    "g24": dict(in_channels=3, img_size=24, model_channels=32, channel_mult=(1, 2, 4), num_res_blocks=1),
    "g16": dict(in_channels=1, img_size=16, model_channels=64, channel_mult=(1, 1, 2, 2), num_res_blocks=3),
    "g40": dict(in_channels=3, img_size=40, model_channels=32, channel_mult=(2, 2), num_res_blocks=2),
}


def make_generic_unet(tag, device=None):
    i = list(GENERIC_UNETS).index(tag)
    m = load_synth(M.FlexibleUNet(**GENERIC_UNETS[tag]), 70 + i).eval()
    x = torch.randn(5, GENERIC_UNETS[tag]["in_channels"], GENERIC_UNETS[tag]["img_size"], GENERIC_UNETS[tag]["img_size"],
                    generator=torch.Generator().manual_seed(300 + i))
    t = torch.tensor([0.0, 0.2, 0.5, 0.8, 0.99])
    return (m.to(device) if device is not None else m), x, t


# FlexibleUNet descriptors chosen to reach the shape-dependent branches of the conv dispatch (launch_conv's routes,
# NT = 1 / 2 channel blocks, P-format hand-over, parity-class Upsample, fused / separate GroupNorm finalize) that the
# presets and GENERIC_UNETS leave out.  Fixed: nothing is drawn at run time.
ARCH_SWEEP = {
    # Cout 96 (NT = 1 over three 32-channel blocks) and 192 (NT = 2, no PAIRN); concat 384 and 288 (> 256: separate
    # gn_finalize + table path); 20 -> 10
    "a96": dict(in_channels=1, img_size=20, model_channels=96, channel_mult=(1, 2), num_res_blocks=2),
    # one level: no Downsample, no Upsample; Cout 160; concat 320; one 144-pixel tile per sample
    "a160": dict(in_channels=3, img_size=12, model_channels=160, channel_mult=(1,), num_res_blocks=2),
    # Cout 96 and 224; 10 -> 5 (odd 5x5 bottom, four samples per tile); Upsample 5 -> 10
    "a224": dict(in_channels=1, img_size=10, model_channels=32, channel_mult=(3, 7), num_res_blocks=2),
    # time MLP width 1024 (time_embed_kernel's LDS exactly full); concat 512 (gn_finalize's s_mean[512] exactly full)
    "a256": dict(in_channels=3, img_size=8, model_channels=256, channel_mult=(1,), num_res_blocks=1),
    # 64x64: 64 statistics parts (no producer-side finalize), 64 -> 32 -> 16 -> 8, Upsample 32 -> 64 in the nine-tap
    # form (up_parts_match(32) is false) while 8 -> 16 and 16 -> 32 take the parity classes
    "a64": dict(in_channels=3, img_size=64, model_channels=32, channel_mult=(1, 2, 4, 8), num_res_blocks=1),
    # 48x48 (tiles of 5 rows, 40 parts) and 24x24
    "a48": dict(in_channels=1, img_size=48, model_channels=64, channel_mult=(1, 2), num_res_blocks=2),
    # 56 -> 28 -> 14 -> 7: an odd bottom map reached by three Downsamples
    "a56": dict(in_channels=1, img_size=56, model_channels=32, channel_mult=(1, 1, 2, 2), num_res_blocks=1),
    # 12 -> 6 -> 3 (3x3 bottom, 9-pixel samples); Cout 192 at 3x3
    "a12": dict(in_channels=3, img_size=12, model_channels=64, channel_mult=(1, 2, 3), num_res_blocks=1),
    # the minimum image: 4 -> 2
    "a4": dict(in_channels=1, img_size=4, model_channels=32, channel_mult=(1, 2), num_res_blocks=1),
    # 36x36 (24 parts); Cout 96 and 192 at 36 and 18
    "a36": dict(in_channels=3, img_size=36, model_channels=96, channel_mult=(1, 2), num_res_blocks=1),
    # num_res_blocks at its maximum: 4 x 9 = 36 decoder blocks
    "deep": dict(in_channels=1, img_size=16, model_channels=32, channel_mult=(1, 1, 1, 1), num_res_blocks=8),
}


def make_sweep_unet(tag, batch, device=None):
    """(module, x, t) of ARCH_SWEEP[tag]: synthetic weights under the entry's own seed, `batch` rows of N(0, 1) input
    and t spread over [0, 0.99] (both ends included once batch >= 2)."""
    i = list(ARCH_SWEEP).index(tag)
    cfg = ARCH_SWEEP[tag]
    m = load_synth(M.FlexibleUNet(**cfg), 80 + i).eval()
    x = torch.randn(batch, cfg["in_channels"], cfg["img_size"], cfg["img_size"],
                    generator=torch.Generator().manual_seed(400 + i))
    t = torch.linspace(0.0, 0.99, batch) if batch > 1 else torch.tensor([0.99])
    return (m.to(device) if device is not None else m), x, t


# ------------------------------------------------------------------ conv routing fixture (tests/golden/conv_routes.json)
# Small descriptors whose per-route conv launch counts (rgfm_unet_conv_routes) are recorded by
# tests/golden/make_conv_routes.py on the commit BEFORE a change of the conv dispatch and compared by
# tests/test_gpu_configs.py after it.  Batch 1 and 4: under-filled launches (four-wave workgroups, 64-channel halves of
# a 128-channel block); 4: exactly one tile of the rasters that put four samples into a tile; 130: a tile count that is
# no multiple of the two-tile cut (and 32.5 four-sample tiles).
def conv_route_cases():
    """(key, FlexibleUNet kwargs, weight seed, batches) per descriptor of the grid."""
    i = 0
    for mc in (32, 64):
        for size in (8, 16, 32):
            for mult in ((1,), (1, 2), (1, 2, 2)):
                cfg = dict(in_channels=1, img_size=size, model_channels=mc, channel_mult=mult, num_res_blocks=1)
                yield f"mc{mc}_s{size}_m{'-'.join(map(str, mult))}", cfg, 300 + i, (1, 4, 130)
                i += 1


def conv_route_run(m, cfg, batch, device):
    """One eval forward of `m` on seeded input: (output, {route: launches}, x, t)."""
    g = torch.Generator().manual_seed(700 + batch)
    x = torch.randn(batch, cfg["in_channels"], cfg["img_size"], cfg["img_size"], generator=g).to(device)
    t = torch.rand(batch, generator=g).to(device)
    with torch.no_grad():
        out = m(x, t)
    torch.cuda.synchronize()
    return out, m._engine.conv_routes(device), x, t
