"""FlexibleUNet over the descriptors of helpers.ARCH_SWEEP -- channel counts that are not powers of two, concatenated
inputs above 256 channels, model_channels 256, one level, odd 3x3 / 5x5 / 7x7 bottoms, 36..64-pixel rasters, the 4x4
minimum and 8 ResBlocks per level -- on the GPU against the float64 restatement (tests/unet_ref64.py): every layer of
the forward under each conv arithmetic, the training pass's output and gradients, and a census of which conv kernel
each architecture actually ran (rgfm_unet_conv_routes)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import ARCH_SWEEP, make_module, make_sweep_unet, maxdiff
from unet_ref64 import cfg_of, forward64, params64
from test_gpu_train import assert_close, ref64_grads, train_case
from ratio_guided_multimodal_fm_amd import _engine, _lib

pytestmark = pytest.mark.gpu

TOL_EVAL = 1e-5

# rows per forward: ragged (3 or 5), one architecture at a single row and one at 66 (partial tiles of four samples)
BATCH = dict(a96=5, a160=1, a224=3, a256=3, a64=3, a48=3, a56=3, a12=5, a4=66, a36=3, deep=5)
MODES = {"default": {}, "bx3": {"RGFM_CONV": "bx3"}, "f32": {"RGFM_CONV": "f32"}, "wino": {"RGFM_WINO": "1"},
         "table": {"RGFM_GN": "table"}}
# one launch of bench size: conv_mfma_hx2q.hip is chosen by launch size (>= 1024 workgroups), not by shape alone
BIG = {"a64": 256}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def ref_trace(tag):
    """float64 (v, activations) of the sweep case, as numpy (computed once, shared by every mode)."""
    m, x, t = make_sweep_unet(tag, BATCH[tag])
    with torch.no_grad():
        v, acts = forward64(cfg_of(m), params64(m, requires_grad=False), x, t, trace=True)
    return v.numpy(), [a.numpy() for a in acts]


def run_forward(tag, mode, dev, monkeypatch, trace=True, batch=None):
    """(out, activations or None, routes) of one forward of the sweep case under MODES[mode]; asserts that no call was
    repeated on a fallback arithmetic and that the handle's range flag is clear."""
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    m, x, t = make_sweep_unet(tag, batch or BATCH[tag], dev)
    x, t = x.to(dev), t.to(dev)
    fallbacks = _engine.range_fallbacks
    if trace:
        out, acts = m._engine.forward_trace(x, t)
    else:
        out, acts = m(x, t), None
    torch.cuda.synchronize()
    assert _engine.range_fallbacks == fallbacks, (tag, mode, _engine.last_range_flags)
    assert m._engine.read_range_flag(dev, reset=False) == 0, (tag, mode)
    return out, acts, m._engine.conv_routes(dev)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("tag", list(ARCH_SWEEP))
def test_layers_vs_float64(dev, tag, mode, monkeypatch):
    out, acts, routes = run_forward(tag, mode, dev, monkeypatch)
    v64, acts64 = ref_trace(tag)
    assert len(acts) == len(acts64)
    for i, (a, r) in enumerate(zip(acts, acts64)):
        assert tuple(a.shape) == r.shape, (tag, mode, i)
        d = maxdiff(a.cpu().numpy(), r)
        assert d < TOL_EVAL * max(1.0, float(np.abs(r).max())), (tag, mode, i, d)
    assert maxdiff(out.cpu().numpy(), v64) < TOL_EVAL, (tag, mode)
    assert sum(routes[r] for r in _lib.ROUTES) > 0


@pytest.mark.parametrize("tag,B", [("a96", 512), ("a64", BIG["a64"])])
def test_rows_do_not_depend_on_the_launch_shape(dev, tag, B):
    """Bitwise: a row's result is the same in a full launch and in an under-filled one (other workgroup shapes; at
    a64's 256 rows the 32x32 and 16x16 layers take conv_mfma_hx2q.hip, which only launches of >= 1024 workgroups
    reach), and the full launch's first rows are float64's."""
    m, _, _ = make_sweep_unet(tag, 1, dev)
    cfg = ARCH_SWEEP[tag]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, cfg["in_channels"], cfg["img_size"], cfg["img_size"], generator=g)
    t = torch.rand(B, generator=g)
    fallbacks = _engine.range_fallbacks
    full = m(x.to(dev), t.to(dev))
    torch.cuda.synchronize()
    assert _engine.range_fallbacks == fallbacks
    if tag in BIG:
        assert m._engine.conv_routes(dev)["hx2q"] > 0
    with torch.no_grad():
        v64 = forward64(cfg_of(m), params64(m, requires_grad=False), x[:3], t[:3])
    assert maxdiff(full[:3].cpu().numpy(), v64.numpy()) < TOL_EVAL
    x, t = x.to(dev), t.to(dev)
    for lo, hi in ((0, 8), (B // 2 - 5, B // 2 + 8), (B - 3, B)):
        part = m(x[lo:hi].contiguous(), t[lo:hi].contiguous())
        assert torch.equal(part, full[lo:hi]), (tag, lo, hi, float((part - full[lo:hi]).abs().max()))


def _census(dev, monkeypatch):
    census = {}
    for mode in MODES:
        with monkeypatch.context() as mp:
            for tag in ARCH_SWEEP:
                census[tag, mode] = run_forward(tag, mode, dev, mp, trace=False)[2]
    for tag, b in BIG.items():
        census[f"{tag}@{b}", "default"] = run_forward(tag, "default", dev, monkeypatch, trace=False, batch=b)[2]
    return census


# Routes the default modes take for the layers named in ARCH_SWEEP's comments (one forward at BATCH rows).  hx2s
# (conv_mfma_hx2s.hip) takes only Downsamples to 16x16 or 8x8 maps, every other Downsample runs on conv_mfma_hx2.hip; the
# parity-class Upsample (t2) needs the output raster's 64-pixel statistics parts to be the input raster's four times
# over, part for part (up_parts_match: here 8 -> 16, 14 -> 28 and 16 -> 32); the 8x8 level runs on hx2c and hands
# conv1 -> conv2 over in P format (hx2d).
EXPECT = {
    "a96": dict(hx2s=0, hx2=1, t2=0),             # 20 -> 10 Downsample; 10 -> 20 Upsample in nine taps
    "a160": dict(hx2s=0, hx2=0, t2=0),            # one level: every conv on hx2p
    "a224": dict(hx2s=0, hx2=1, t2=0),            # 10 -> 5; 5 -> 10 in nine taps
    "a256": dict(hx2s=0, hx2=0, t2=0, hx2c=3, hx2d=3),
    "a64": dict(hx2s=2, hx2=1, t2=2, hx2c=3, hx2d=3),  # 64 -> 32 on hx2; 32 -> 64 in nine taps
    "a48": dict(hx2s=0, hx2=1, t2=0),
    "a56": dict(hx2s=0, hx2=3, t2=1),             # 56 -> 28 -> 14 -> 7; 14 -> 28 as parity classes, 7 -> 14 and 28 -> 56 not
    "a12": dict(hx2s=0, hx2=2, t2=0),             # 12 -> 6 -> 3
    "a4": dict(hx2s=0, hx2=1, t2=0),              # 4 -> 2
    "a36": dict(hx2s=0, hx2=1, t2=0),
    "deep": dict(hx2s=1, hx2=2, t2=1),            # 16 -> 8 on hx2s; 8 -> 4 -> 2 on hx2; only 8 -> 16 as parity classes
}


def test_route_census(dev, monkeypatch):
    """Every conv route and the parity-class Upsample form are reached by the sweep, and the architectures that were
    chosen for a route take it."""
    census = _census(dev, monkeypatch)
    keys = _lib.ROUTES + ("t2",)
    print("\nconv launches per route (one forward)\n" + "arch  mode     " + " ".join(f"{k:>5}" for k in keys))
    for (tag, mode), r in census.items():
        print(f"{tag:<5} {mode:<8} " + " ".join(f"{r[k]:>5}" for k in keys))
    total = {k: sum(r[k] for r in census.values()) for k in keys}
    for k in keys:
        assert total[k] > 0, (k, total)
    # RGFM_CONV=f32: every conv on the exact fp32 kernel; bx3: no fp16 kernel
    for tag in ARCH_SWEEP:
        f32 = census[tag, "f32"]
        assert all(f32[k] == 0 for k in keys if k != "f32"), (tag, f32)
        assert all(census[tag, "bx3"][k] == 0 for k in keys if k not in ("bx3", "f32")), tag
    for tag, want in EXPECT.items():
        got = census[tag, "default"]
        assert {k: got[k] for k in want} == want, (tag, got)
    # RGFM_WINO=1: the long-K layers (>= 128 input channels, Cout % 64 == 0) at 32x32 / 16x16 -- a64's only; a96's
    # 192-channel level is 10x10, which the Winograd kernel does not tile
    assert census["a64", "wino"]["hx2w"] > 0 and census["a96", "wino"]["hx2w"] == 0
    assert census["a64@256", "default"]["hx2q"] > 0


def _train_pass(m, x, t, target, train=False):
    m.train(train)
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    v = m.forward_train(xg, t)
    loss = F.mse_loss(v, target)
    loss.backward()
    m.eval()
    return v.detach(), loss.item(), xg.grad, [p.grad for p in m.parameters()]


def _check_train(m, x, t, target, masks=None, p_drop=0.0):
    dev = next(m.parameters()).device
    v, loss, dx, grads = _train_pass(m, x.to(dev), t.to(dev), target.to(dev), train=masks is not None)
    with torch.no_grad():
        v64 = forward64(cfg_of(m), params64(m, requires_grad=False), x, t, masks, p_drop)
    assert maxdiff(v.cpu().numpy(), v64.numpy()) < TOL_EVAL
    loss64, dx64, grads64 = ref64_grads(m, x, t, target, masks, p_drop)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert_close(dx, dx64, "dx")
    for (name, _), g, g64 in zip(m.state_dict().items(), grads, grads64):
        assert_close(g, g64, name)


@pytest.mark.parametrize("tag", list(ARCH_SWEEP))
def test_training_pass_vs_float64(dev, tag):
    m = make_sweep_unet(tag, 1, dev)[0]
    x, t, target = train_case(tag, 3, ARCH_SWEEP[tag])
    _check_train(m, x, t, target)


def test_training_pass_single_t(dev):
    """One t for every row (t_count == 1: the broadcast branch of ug_sincos_kernel)."""
    m = make_sweep_unet("a224", 1, dev)[0]
    x, _, target = train_case("a224", 4, ARCH_SWEEP["a224"])
    _check_train(m, x, torch.tensor([0.63]), target)


def test_training_pass_with_dropout(dev):
    """p = 0.1 on a 96 / 192-channel net, the float64 side fed the library's keep masks (seed drawn as forward_train
    draws it)."""
    m = make_sweep_unet("a96", 1, dev)[0]
    p = m.dropout_p()
    assert p == pytest.approx(0.1)
    B = 3
    x, t, target = train_case("a96", B, ARCH_SWEEP["a96"])
    torch.cuda.manual_seed(41)
    seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())
    masks = [m._engine.dropout_mask(b, seed, p, B, dev).cpu() for b in range(len(m.resblock_geometry()))]
    assert all(0.0 < float(k.mean()) < 1.0 for k in masks)
    torch.cuda.manual_seed(41)
    _check_train(m, x, t, target, masks, p)


def test_training_pass_at_the_bench_batch(dev):
    """mnist32 at the training bench's batch of 128: the weight-gradient K-split counts the bench runs."""
    m = make_module("mnist32", dev)
    x, t, target = train_case("mnist32", 128, cfg_of(m))
    _check_train(m, x, t, target)
