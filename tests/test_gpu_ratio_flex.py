"""FlexibleRatioEstimator on the GPU (kind RGFM_RATIO_FLEXIBLE): evaluation, the gradient of log r, the training pass,
optimiser steps and guided sampling across pairs of image shapes, against the float64 restatement
(tests/ratio_flex_ref64.py) and the reference's own results (tests/golden/ratio_flex.npz).

Shapes: (x, y) pairs of (channels, size).  1x8 + 1x8 reaches conv4 at 1x1 (the average over one pixel); 2x12 + 4x12 runs
the 2- and 4-channel input convs and a 3 -> 1 max-pool that drops a row and a column; 1x28 + 1x28 is the geometry of
the fixed RatioEstimator kind; 3x20 + 1x32 has unequal sizes and a 5 -> 2 pool; 3x32 + 3x32.  B in {1, 5}: one sample
of a four-sample tile, and more than one tile.

Data seeds.  A max-pool whose two largest window elements nearly tie may route differently in another fp32
arithmetic or in float64: a discontinuity of the function, not an arithmetic error.  SEEDS was searched on the CPU
with the fp32 torch.nn module of the architecture (same synthetic weights) against its float64 copy: for every seed
listed the fp32 module picks the float64 argmax in EVERY window (100 % >= the 99.9 % the choice check asks for), and
the seed is the first from 1000 + 100 * case whose smallest float64 pool gap is >= 10 x the largest fp32-vs-float64
deviation of a pre-pool tensor -- or, where 60 seeds hold none (the three larger shapes at B = 5, ~50 k windows), the
one of those 60 with the largest such ratio (5.1 .. 6.3).

Bounds.  Evaluation: 1e-5 absolute, the bound tests/test_gpu_parity.py applies to the two fixed estimators.  The fp32
torch.nn module itself is within 5.2e-7 of float64 on these shapes and seeds (|score| <= 1), so 4 x that is inside
the bound and no shape needs another.  Gradient of log r: 1e-4 max |g64| per tensor (tests/test_gpu_configs.py).
Training gradients: 1e-4 max |g64| per tensor.  Samplers: 1e-4 (TOL_SAMPLER)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, make_module, maxdiff
from ratio_flex_ref64 import forward64, log_ratio64, params64
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth, paired_noise
from ratio_guided_multimodal_fm_amd.utils.losses import get_ratio_loss

pytestmark = pytest.mark.gpu

TOL_EVAL, TOL_GRAD, TOL_TRAIN, TOL_SAMPLER = 1e-5, 1e-4, 1e-4, 1e-4
W_SEED, FEAT, HID = 31, 64, 128
CASES = [((1, 8), (1, 8)), ((2, 12), (4, 12)), ((1, 28), (1, 28)), ((3, 20), (1, 32)), ((3, 32), (3, 32))]
SEEDS = {(0, 1): 1000, (0, 5): 1000, (1, 1): 1100, (1, 5): 1101, (2, 1): 1220, (2, 5): 1237, (3, 1): 1302, (3, 5): 1325,
         (4, 1): 1417, (4, 5): 1459}
GRID = [(ci, B) for ci in range(len(CASES)) for B in (1, 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def module(ci, dev, loss_type="disc"):
    (xc, _), (yc, _) = CASES[ci]
    return load_synth(M.FlexibleRatioEstimator(xc, yc, FEAT, HID, loss_type), W_SEED).eval().to(dev)


def inputs(ci, B):
    (xc, xs), (yc, ys) = CASES[ci]
    g = torch.Generator().manual_seed(SEEDS[(ci, B)])
    return torch.randn(B, xc, xs, xs, generator=g), torch.randn(B, yc, ys, ys, generator=g)


_ref = {}


def ref_eval(ci, B):
    """float64 scores, log-ratios and gradients of log_ratio.sum() of a case: computed once, shared, never modified."""
    if (ci, B) not in _ref:
        x, y = inputs(ci, B)
        sd = params64(module(ci, "cpu"), requires_grad=False)
        r = {"score": forward64(sd, x, y)}
        for lt in ("disc", "rulsif"):
            x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
            lr = log_ratio64(sd, x64, y64, lt)
            r["gx_" + lt], r["gy_" + lt] = torch.autograd.grad(lr.sum(), (x64, y64))
            r["lr_" + lt] = lr.detach()
        _ref[(ci, B)] = r
    return _ref[(ci, B)]


def assert_close(g, g64, what, tol):
    scale = float(g64.abs().max())
    err = float((g.detach().cpu().double() - g64).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / max(scale, 1e-300):.3e}")
    assert err <= tol * max(scale, 1e-30), (what, err, scale)


# ------------------------------------------------------------------ 1. evaluation
@pytest.mark.parametrize("ci,B", GRID)
def test_eval_vs_float64(dev, ci, B):
    x, y = inputs(ci, B)
    ref = ref_eval(ci, B)
    m = module(ci, dev)
    xd, yd = x.to(dev), y.to(dev)
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        s, lr = m(xd, yd), m.log_ratio(xd, yd)
        r = m._engine.eval(xd, yd, "ratio")
        assert s.shape == lr.shape == r.shape == (B,)
        for name, got, want in (("score", s, ref["score"]), ("log_ratio", lr, ref["lr_" + lt]), ("ratio", r, ref["lr_" + lt].exp())):
            err = float((got.cpu().double() - want).abs().max())
            print(f"case {ci} B {B} {lt} {name}: err {err:.3e}")
            assert err < TOL_EVAL, (lt, name, err)
    m.loss_type = "bogus"
    with pytest.raises(ValueError):
        m.log_ratio(xd, yd)


def test_eval_vs_reference_fixture(dev):
    g = golden("ratio_flex")
    B, xc, yc, xs, ys, feat, hid = (int(v) for v in g["dims"])
    m = load_synth(M.FlexibleRatioEstimator(xc, yc, feat, hid), int(g["w_seed"])).eval().to(dev)
    gen = torch.Generator().manual_seed(int(g["data_seed"]))
    x, y = torch.randn(B, xc, xs, xs, generator=gen).to(dev), torch.randn(B, yc, ys, ys, generator=gen).to(dev)
    assert maxdiff(m(x, y).cpu().numpy(), g["forward"]) < TOL_EVAL
    for row, lt in enumerate(("disc", "rulsif")):
        m.loss_type = lt
        assert maxdiff(m.log_ratio(x, y).cpu().numpy(), g["log_ratio_" + lt]) < TOL_EVAL
        for k, gr in enumerate(m.grad_log_ratio(x, y)):
            amax = float(g["grad_xy_max"][2 * row + k])
            idx = torch.randint(0, gr.numel(), (g["grad_xy_probe"].shape[1],), generator=torch.Generator().manual_seed(7000 + k))
            assert abs(float(gr.abs().max()) - amax) <= TOL_GRAD * amax
            assert np.abs(gr.cpu().reshape(-1)[idx].numpy() - g["grad_xy_probe"][2 * row + k]).max() <= TOL_GRAD * amax


@pytest.mark.parametrize("B", [1, 5])
def test_28x28_is_the_fixed_kind_bitwise(dev, B):
    """At 1x28x28 + 1x28x28 the flexible handle plans the rasters, tilings and kernels of RGFM_RATIO_MNIST28 (every conv
    on the fp32 matrix-core kernel in both): the same weights, mapped key for key, give the same bits."""
    flex = module(2, dev)
    fixed = M.RatioEstimator(FEAT, HID).eval().to(dev)
    fixed.load_state_dict(flex.state_dict(), strict=True)
    x, y = (t.to(dev) for t in inputs(2, B))
    for lt in ("disc", "rulsif"):
        flex.loss_type = fixed.loss_type = lt
        assert torch.equal(flex(x, y), fixed(x, y))
        assert torch.equal(flex.log_ratio(x, y), fixed.log_ratio(x, y))
        for a, b in zip(flex.grad_log_ratio(x, y), fixed.grad_log_ratio(x, y)):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ 2. gradient of log r
@pytest.mark.parametrize("ci,B", GRID)
def test_grad_log_ratio_vs_float64_autograd(dev, ci, B):
    x, y = inputs(ci, B)
    ref = ref_eval(ci, B)
    m = module(ci, dev)
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        gx, gy = m.grad_log_ratio(x.to(dev), y.to(dev))
        assert gx.shape == x.shape and gy.shape == y.shape
        assert_close(gx, ref["gx_" + lt], f"case {ci} B {B} {lt} gx", TOL_GRAD)
        assert_close(gy, ref["gy_" + lt], f"case {ci} B {B} {lt} gy", TOL_GRAD)
        _, _, lr = m._engine.grad_log_ratio(x.to(dev), y.to(dev))
        assert float((lr.cpu().double() - ref["lr_" + lt]).abs().max()) < TOL_EVAL


# ------------------------------------------------------------------ 3. training
def loss_of(scores, real, loss_type):
    """The trainers' loss: the ratio loss, or BCE on the one class present (B = 1)."""
    real = real.to(scores.device)
    if real.all():
        return F.binary_cross_entropy_with_logits(scores, torch.ones_like(scores))
    return get_ratio_loss(loss_type)(scores[real], scores[~real])[0]


def check_choices(choices, wins):
    """Every choice is a near-argmax in float64, and the exact float64 argmax in >= 99.9 % of windows (tests/test_gpu_ratio_train.py)."""
    exact = total = 0
    for enc_c, enc_w in zip(choices, wins):
        assert len(enc_c) == len(enc_w) == 3
        for c, w in zip(enc_c, enc_w):
            k = c.to(torch.int64)
            assert k.shape == w.shape[:-1] and int(k.min()) >= 0 and int(k.max()) <= 3
            chosen = w.gather(-1, k[..., None])[..., 0]
            assert bool((chosen >= w.max(-1).values - 1e-5 * float(w.abs().max())).all())
            exact += int((k == w.argmax(-1)).sum())
            total += k.numel()
    print(f"pool choices: {exact} / {total} are the float64 argmax")
    assert exact >= 0.999 * total, (exact, total)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("ci,B", GRID)
def test_training_gradients_vs_float64(dev, ci, B, training):
    lt = "disc" if B == 5 else "rulsif"  # (the loss type only shapes dL/dscore here; both are covered)
    m = module(ci, dev, lt)
    x, y = inputs(ci, B)
    real = torch.arange(B) % 2 == 0
    sd = params64(m)
    eng, p = m._engine, m.dropout_p()
    masks = None
    if training:  # the keep masks of the seed forward_train is about to draw
        torch.cuda.manual_seed(99)
        seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())
        eng.bind(x.to(dev), y.to(dev))
        masks = [eng.dropout_mask(b, seed, p, B, dev).cpu() for b in (0, 1)]
        assert masks[0].shape == (B, HID) and masks[1].shape == (B, HID // 2)
        torch.cuda.manual_seed(99)
    m.train(training)
    xg, yg = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    scores = m.forward_train(xg, yg)
    choices = [[c.cpu() for c in enc] for enc in eng.pool_choices()]
    loss_of(scores, real, lt).backward()
    m.eval()
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    out = {}
    s64 = forward64(sd, x64, y64, choices, masks, p if training else 0.0, out)
    loss_of(s64, real, lt).backward()
    assert float((scores.detach().cpu().double() - s64.detach()).abs().max()) <= TOL_EVAL
    check_choices(choices, out["windows"])
    assert_close(xg.grad, x64.grad, "dx", TOL_TRAIN)
    assert_close(yg.grad, y64.grad, "dy", TOL_TRAIN)
    for k, q in m.named_parameters():
        assert_close(q.grad, sd[k].grad, k, TOL_TRAIN)


# ------------------------------------------------------------------ 4. optimiser steps, the handle cache
def test_adam_steps_then_eval_equals_a_fresh_module(dev):
    m = module(1, dev)
    x, y = (t.to(dev) for t in inputs(1, 5))
    m.eval()
    m.log_ratio(x, y)
    h0 = m._engine.handle(dev).value
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = m.log_ratio(x, y).clone()
    for _ in range(2):
        m.train()
        opt.zero_grad()
        loss_of(m.forward_train(x, y), torch.arange(5) % 2 == 0, "disc").backward()
        opt.step()
    m.eval()
    after = m.log_ratio(x, y)
    assert m._engine.handle(dev).value == h0  # refreshed in place (rgfm_ratio_update_params), not re-created
    assert not torch.equal(before, after)
    fresh = M.FlexibleRatioEstimator(2, 4, FEAT, HID).eval().to(dev)
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(after, fresh.log_ratio(x, y)) and torch.equal(m(x, y), fresh(x, y))
    for a, b in zip(m.grad_log_ratio(x, y), fresh.grad_log_ratio(x, y)):
        assert torch.equal(a, b)


def test_one_handle_per_pair_of_sizes(dev):
    """The module is size-agnostic; alternating between two pairs of sizes re-creates no handle, and each pair's
    results do not depend on what ran in between."""
    m = module(0, dev)
    g = torch.Generator().manual_seed(5)
    a = (torch.randn(3, 1, 8, 8, generator=g).to(dev), torch.randn(3, 1, 8, 8, generator=g).to(dev))
    b = (torch.randn(2, 1, 16, 16, generator=g).to(dev), torch.randn(2, 1, 12, 12, generator=g).to(dev))
    ra, ha = m(*a), m._engine.handle(dev).value
    rb, hb = m(*b), m._engine.handle(dev).value
    assert ha != hb
    for _ in range(2):
        assert torch.equal(m(*a), ra) and m._engine.handle(dev).value == ha
        assert torch.equal(m(*b), rb) and m._engine.handle(dev).value == hb
    sd = params64(m, requires_grad=False)
    assert float((rb.cpu().double() - forward64(sd, b[0].cpu(), b[1].cpu())).abs().max()) < TOL_EVAL
    with torch.no_grad():  # an in-place edit reaches every cached handle
        m.score_net[8].bias.add_(0.25)
    assert float((m(*a) - ra - 0.25).abs().max()) < 1e-6 and float((m(*b) - rb - 0.25).abs().max()) < 1e-6
    assert m._engine.handle(dev).value == hb
    for bad in ((torch.zeros(1, 2, 8, 8, device=dev), a[1][:1]), (torch.zeros(1, 1, 8, 10, device=dev), a[1][:1]),
                (torch.zeros(1, 1, 6, 6, device=dev), a[1][:1])):
        with pytest.raises(_lib.RgfmError):
            m(*bad)


# ------------------------------------------------------------------ 5. guided sampling
def nets(dev):
    fx = load_synth(M.FlexibleUNet(3, 16, 32, (1, 2), 2), 41).eval().to(dev)
    fy = load_synth(M.FlexibleUNet(1, 16, 32, (1, 2), 2), 42).eval().to(dev)
    rr = load_synth(M.FlexibleRatioEstimator(3, 1, FEAT, HID), W_SEED).eval().to(dev)
    return fx, fy, rr


def test_sample_pair_grad_equals_the_python_loop(dev):
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler
    fx, fy, rr = nets(dev)
    B, S, gamma = 4, 4, 0.5
    noise = paired_noise(23, B, 0, (3, 16, 16), (1, 16, 16))
    xs, ys = paired_sampler(fx, fy, rr, "grad_log_ratio", gamma, B, S, dev, 0, (3, 16, 16), (1, 16, 16), noise=noise, verbose=False)
    x, y = noise[0].to(dev), noise[1].to(dev)
    dt = 1.0 / S
    for s in range(S):
        t = torch.full((B,), s * dt, device=dev)
        vx, vy = fx(x, t), fy(y, t)
        gx, gy = rr.grad_log_ratio(x, y)
        x, y = x + (vx + gamma * gx) * dt, y + (vy + gamma * gy) * dt
    assert xs.shape == (B, 3, 16, 16) and ys.shape == (B, 1, 16, 16)
    assert maxdiff(xs.cpu().numpy(), x.cpu().numpy()) < TOL_SAMPLER and maxdiff(ys.cpu().numpy(), y.cpu().numpy()) < TOL_SAMPLER
    x0, y0 = paired_sampler(fx, fy, rr, "none", 0.0, B, S, dev, 0, (3, 16, 16), (1, 16, 16), noise=noise, verbose=False)
    assert maxdiff(xs.cpu().numpy(), x0.cpu().numpy()) > 1e-3  # the guidance term is not nothing


def test_mc_feng_through_paired_sampler(dev):
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler
    fx, fy, rr = nets(dev)
    B, N, S, gamma = 4, 8, 4, 0.5
    noise = paired_noise(29, B, N, (3, 16, 16), (1, 16, 16))
    xs, ys = paired_sampler(fx, fy, rr, "mc_feng", gamma, B, S, dev, N, (3, 16, 16), (1, 16, 16), noise=noise, verbose=False)
    x, y, mx, my = (t.to(dev) for t in noise)
    dt = 1.0 / S
    for s in range(S):
        t = torch.full((N,), s * dt, device=dev)
        mx, my = mx + fx(mx, t) * dt, my + fy(my, t) * dt
    ratios = rr._engine.eval(mx, my, "ratio")
    sd = params64(rr, requires_grad=False)
    assert float((ratios.cpu().double() - log_ratio64(sd, mx.cpu(), my.cpu(), "disc").exp()).abs().max()) < TOL_EVAL
    for s in range(S):
        t = s * dt
        tv = torch.full((B,), t, device=dev)
        vx, vy = fx(x, tv).contiguous(), fy(y, tv).contiguous()
        if t > 1e-3:
            _engine.guidance_apply(x, y, vx, vy, mx, my, ratios, t, gamma)
        x, y = x + vx * dt, y + vy * dt
    assert maxdiff(xs.cpu().numpy(), x.cpu().numpy()) < TOL_SAMPLER and maxdiff(ys.cpu().numpy(), y.cpu().numpy()) < TOL_SAMPLER


def test_mismatched_pair_is_an_error_not_a_fault(dev):
    fx, fy, rr = nets(dev)
    eng = rr._engine
    eng.bind(torch.zeros(1, 3, 12, 12, device=dev), torch.zeros(1, 1, 12, 12, device=dev))
    hr = eng.handle(dev)  # built for 3x12x12 + 1x12x12; the U-Nets are 3x16x16 + 1x16x16
    hx, hy = fx._engine.handle(dev), fy._engine.handle(dev)
    L = _lib.lib()
    nb = ctypes.c_size_t()
    with pytest.raises(_lib.RgfmError, match="3x12x12"):
        _lib.check(L.rgfm_sample_pair_grad_workspace_bytes(hx, hy, hr, 2, ctypes.byref(nb)))
    x, y = torch.zeros(2, 3, 16, 16, device=dev), torch.zeros(2, 1, 16, 16, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.RgfmError, match="3x12x12"):
        _lib.check(L.rgfm_sample_pair_grad(hx, hy, hr, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), 2, 4, 0.5,
                                           0, 4, ctypes.c_void_p(ws.data_ptr()), ws.numel(), None))
    assert not x.any() and not y.any()
    # a flexible estimator whose channels do not fit the pair: refused on the Python side
    bad = load_synth(M.FlexibleRatioEstimator(1, 1, FEAT, HID), W_SEED).eval().to(dev)
    with pytest.raises(_lib.RgfmError):
        _engine.sample_pair_grad(fx, fy, bad, x, y, 4, 0.5)


# ------------------------------------------------------------------ 6. the fixed kinds did not move
PARENT = "e48eff1"  # the commit these bit patterns were recorded from (same device, same inputs)
PARENT_BITS = {
    "ratio_ms": {
        "score": [-1088967609, -1089174165, -1088489804, -1088595422],
        "log_ratio": [-1088967609, -1089174164, -1088489804, -1088595422],
        "gx_head": [982428075, 958298798, -1159282509, -1165554925, -1158377088, 994595031, -1155648553, 990410310],
        "gy_head": [-1218474269, -1246126175, 945511321, 926154707, 944792453, 957293498, 935104995, -1209711739],
    },
    "ratio28": {
        "score": [1039940100, 1054226641, 1040918133, 993330616],
        "log_ratio": [1039940104, 1054226642, 1040918132, 993330688],
        "gx_head": [-1170486130, 1003313431, 995040244, -1175627685, 999841652, 995919748, -1156905940, 972994462],
        "gy_head": [-1149072329, 979619191, 1006151380, 965808415, -1183663815, 976247180, 973356786, -1181298226],
    },
}


@pytest.mark.parametrize("tag,sx,sy", [("ratio_ms", (1, 32, 32), (3, 32, 32)), ("ratio28", (1, 28, 28), (1, 28, 28))])
def test_fixed_kinds_are_bit_identical_to_the_parent_commit(dev, tag, sx, sy):
    m = make_module(tag, dev)
    g = torch.Generator().manual_seed(4242)
    x, y = torch.randn(4, *sx, generator=g).to(dev), torch.randn(4, *sy, generator=g).to(dev)
    got = {"score": m(x, y), "log_ratio": m.log_ratio(x, y)}
    gx, gy = m.grad_log_ratio(x, y)
    got["gx_head"], got["gy_head"] = gx.reshape(-1)[:8], gy.reshape(-1)[:8]
    for k, v in got.items():
        bits = v.cpu().contiguous().view(torch.int32).tolist()
        print(tag, k, bits)
        assert bits == PARENT_BITS[tag][k], (tag, k)


# ------------------------------------------------------------------ 7. the training CLI
def test_train_cli_flexible_one_epoch(dev, tmp_path, monkeypatch):
    """train_ratio --kind flexible in-process on a 3x16 + 2x12 toy set: sizes from the data file, the checkpoint loads back."""
    from ratio_guided_multimodal_fm_amd import train_ratio
    from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(3)
    label = torch.arange(24) % 3
    x = torch.randn(24, 3, 16, 16, generator=g) + label[:, None, None, None].float()
    y = torch.randn(24, 2, 12, 12, generator=g) - label[:, None, None, None].float()
    np.savez("pairs.npz", x=x.numpy(), y=y.numpy(), label=label.numpy())
    best = train_ratio.main(["--kind", "flexible", "--data", "pairs.npz", "--x_channels", "3", "--y_channels", "2",
                             "--epochs", "1", "--batch_size", "8", "--device", "cuda:0"])
    assert np.isfinite(best)
    ckpt = torch.load("checkpoints/ratio_disc_flexible_best.pth", map_location="cpu")
    m = M.FlexibleRatioEstimator(ckpt["x_channels"], ckpt["y_channels"], ckpt["feature_dim"], ckpt["hidden_dim"], ckpt["loss_type"])
    assert load_checkpoint(m, "checkpoints/ratio_disc_flexible_best.pth")["epoch"] == 1
    m = m.eval().to(dev)
    s = m(x[:5].to(dev), y[:5].to(dev))
    sd = params64(m, requires_grad=False)
    assert float((s.cpu().double() - forward64(sd, x[:5], y[:5])).abs().max()) < TOL_EVAL
