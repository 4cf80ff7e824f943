"""Training pass of FlexibleUNet on the GPU (rgfm_unet_forward_train / rgfm_unet_backward / update_params):
gradients against the reference's autograd (tests/golden/unet_train_grad.npz) and against a float64 restatement
(tests/unet_ref64.py), dropout, determinism, the CFM training loop, the hand-back to sampling and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GENERIC_UNETS, golden, make_generic_unet, make_module
from unet_ref64 import cfg_of, forward64, params64
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
from ratio_guided_multimodal_fm_amd.utils.flow_utils import CFMSchedule, train_flow_matching_epoch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL_GRAD = 1e-4  # max |g - g64| <= TOL_GRAD * max |g64| per tensor


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def train_case(tag, batch, cfg):  # must match tests/golden/make_train_golden.py
    g = torch.Generator().manual_seed(500 + sum(map(ord, tag)) + batch)
    S, C = cfg["img_size"], cfg["in_channels"]
    return (torch.randn(batch, C, S, S, generator=g), torch.rand(batch, generator=g),
            torch.randn(batch, C, S, S, generator=g))


def module_of(tag, dev):
    if tag in GENERIC_UNETS:
        return make_generic_unet(tag, dev)[0]
    return make_module(tag, dev)


def hip_grads(m, x, t, target, train=False):
    m.train(train)
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    loss = F.mse_loss(m.forward_train(xg, t), target)
    loss.backward()
    m.eval()
    return loss.item(), xg.grad, [p.grad for p in m.parameters()]


def ref64_grads(m, x, t, target, masks=None, p_drop=0.0):
    sd = params64(m)
    x64 = x.detach().cpu().double().requires_grad_(True)
    v = forward64(cfg_of(m), sd, x64, t.cpu(), masks, p_drop)
    loss = F.mse_loss(v, target.cpu().double())
    loss.backward()
    return loss.item(), x64.grad, [sd[k].grad for k in m.state_dict()]


def assert_close(g, g64, what):
    g = g.detach().cpu().double()
    scale = float(g64.abs().max())
    err = float((g - g64).abs().max())
    assert err <= TOL_GRAD * max(scale, 1e-30), (what, err, scale)


CASES = [("unet28", 37), ("mnist32", 5), ("svhn", 5), ("g24", 37), ("g16", 1), ("g40", 5)]


@pytest.mark.parametrize("tag,batch", CASES)
def test_gradients_vs_float64(dev, tag, batch):
    m = module_of(tag, dev)
    x, t, target = train_case(tag, batch, cfg_of(m))
    loss, dx, grads = hip_grads(m, x.to(dev), t.to(dev), target.to(dev))
    loss64, dx64, grads64 = ref64_grads(m, x, t, target)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert_close(dx, dx64, "dx")
    for (name, _), g, g64 in zip(m.state_dict().items(), grads, grads64):
        assert_close(g, g64, name)


@pytest.mark.parametrize("tag", ["g16", "mnist32"])
def test_gradients_vs_reference_autograd(dev, tag):
    gold = golden("unet_train_grad")
    m = module_of(tag, dev)
    x, t, target = train_case(tag, 2, cfg_of(m))
    loss, dx, grads = hip_grads(m, x.to(dev), t.to(dev), target.to(dev))
    assert abs(loss - float(gold[f"{tag}_loss"])) <= 1e-5 * abs(float(gold[f"{tag}_loss"]))
    r = gold[f"{tag}_dx"]
    assert np.abs(dx.cpu().numpy() - r).max() <= TOL_GRAD * np.abs(r).max()
    for i, g in enumerate(grads):
        gf = g.reshape(-1).cpu()
        idx = torch.randint(0, gf.numel(), (64,), generator=torch.Generator().manual_seed(7000 + i))
        amax = float(gold[f"{tag}_amax_{i}"])
        assert abs(float(gf.abs().max()) - amax) <= TOL_GRAD * amax, i
        assert np.abs(gf[idx].numpy() - gold[f"{tag}_probe_{i}"]).max() <= TOL_GRAD * amax, i


def test_dropout_mask_and_gradients(dev):
    m = make_module("mnist32", dev)
    p = m.dropout_p()
    assert p == pytest.approx(0.1)
    eng = m._engine
    geo = m.resblock_geometry()
    for block in (0, len(geo) - 1):
        mask = eng.dropout_mask(block, 1234, p, 8, dev)
        n = mask.numel()
        kept = float(mask.sum()) / n
        assert abs(kept - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (block, kept)
        assert set(torch.unique(mask).tolist()) <= {0.0, 1.0}
    assert not torch.equal(eng.dropout_mask(0, 1234, p, 8, dev), eng.dropout_mask(0, 1235, p, 8, dev))
    # gradients with p = 0.1 against the float64 restatement fed the library's masks (seed drawn like forward_train)
    B = 5
    x, t, target = train_case("mnist32", B, cfg_of(m))
    torch.cuda.manual_seed(99)
    seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())
    masks = [eng.dropout_mask(b, seed, p, B, dev).cpu() for b in range(len(geo))]
    torch.cuda.manual_seed(99)
    loss, dx, grads = hip_grads(m, x.to(dev), t.to(dev), target.to(dev), train=True)
    loss64, dx64, grads64 = ref64_grads(m, x, t, target, masks, p)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert_close(dx, dx64, "dx")
    for (name, _), g, g64 in zip(m.state_dict().items(), grads, grads64):
        assert_close(g, g64, name)
    # same seed: bitwise-equal outputs and gradients; another seed: another output
    runs = []
    for s in (99, 99, 100):
        torch.cuda.manual_seed(s)
        m.train()
        xg = x.to(dev).requires_grad_(True)
        v = m.forward_train(xg, t.to(dev))
        m.zero_grad(set_to_none=True)
        F.mse_loss(v, target.to(dev)).backward()
        runs.append((v.detach().clone(), xg.grad.clone(), [q.grad.clone() for q in m.parameters()]))
    m.eval()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    assert not torch.equal(runs[0][0], runs[2][0])


def test_backward_is_deterministic(dev):
    m = make_module("svhn", dev)
    x, t, target = train_case("svhn", 37, cfg_of(m))
    a = hip_grads(m, x.to(dev), t.to(dev), target.to(dev))
    b = hip_grads(m, x.to(dev), t.to(dev), target.to(dev))
    assert torch.equal(a[1], b[1])
    assert all(torch.equal(u, v) for u, v in zip(a[2], b[2]))


def test_training_mode_forward_still_raises(dev):
    m = make_module("mnist32", dev).train()
    with pytest.raises(_lib.RgfmError, match="forward_train"):
        m(torch.zeros(2, 1, 32, 32, device=dev), torch.zeros(2, device=dev))
    m.eval()


def test_sgd_steps_match_float64(dev):
    m = make_module("mnist32", dev)
    for b in m._resblocks():
        b.dropout.p = 0.0
    g = torch.Generator().manual_seed(5)
    data = torch.randn(6, 1, 32, 32, generator=g)
    lr = 0.05
    sd64 = params64(m, requires_grad=False)
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    sched = CFMSchedule()
    cfg = cfg_of(m)
    for step in range(5):
        # the loop's draws (t, then x_0) replayed for the float64 side
        state = torch.cuda.get_rng_state(dev)
        train_flow_matching_epoch(m, [{"x": data}], opt, sched, dev)
        torch.cuda.set_rng_state(state, dev)
        t = torch.rand(6, device=dev)
        x0 = torch.randn(6, 1, 32, 32, device=dev)
        tt = t.view(-1, 1, 1, 1)
        xt, u = ((1 - tt) * x0 + tt * data.to(dev)), data.to(dev) - x0
        p64 = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
        loss = F.mse_loss(forward64(cfg, p64, xt.cpu(), t.cpu()), u.cpu().double())
        loss.backward()
        sd64 = {k: (v - lr * v.grad).detach() for k, v in p64.items()}
    for k, v in m.state_dict().items():
        r = sd64[k]
        assert float((v.cpu().double() - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-12), k


def test_adam_halves_the_loss(dev):
    torch.manual_seed(0)
    m = make_module("mnist32", dev)
    g = torch.Generator().manual_seed(6)
    # 64 fixed images: smooth blobs (a learnable velocity target)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, 32), torch.linspace(-1, 1, 32), indexing="ij")
    c = torch.rand(64, 2, generator=g) - 0.5
    data = torch.exp(-((xx - c[:, 0, None, None]) ** 2 + (yy - c[:, 1, None, None]) ** 2) / 0.1)[:, None] * 2 - 1
    data = data.to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sched = CFMSchedule()
    torch.cuda.manual_seed(1)
    losses = [train_flow_matching_epoch(m, [{"x": data}], opt, sched, dev) for _ in range(200)]
    assert np.mean(losses[-10:]) < 0.5 * np.mean(losses[:3]), (losses[:3], losses[-10:])


def test_hand_back_to_sampling(dev):
    m = make_module("unet28", dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    data = torch.randn(8, 1, 28, 28, generator=torch.Generator().manual_seed(8)).to(dev)
    x = torch.randn(4, 1, 28, 28, device=dev)
    t = torch.full((4,), 0.4, device=dev)
    m.eval()
    h0 = m._engine.handle(dev).value
    v_before = m(x, t).clone()
    for _ in range(3):
        train_flow_matching_epoch(m, [{"x": data}], opt, CFMSchedule(), dev)
    m.eval()
    v = m(x, t)
    assert m._engine.handle(dev).value == h0  # refreshed in place (rgfm_unet_update_params), not re-created
    assert not torch.equal(v, v_before)
    fresh = make_module("unet28", dev)
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(v, fresh(x, t))
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    s1 = CFMSchedule().sample(m, 4, num_steps=5, device=dev)
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    s2 = CFMSchedule().sample(fresh, 4, num_steps=5, device=dev)
    assert torch.equal(s1, s2)


def test_cli_end_to_end(dev, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    rng = np.random.default_rng(0)
    out = tmp_path / "checkpoints"
    for preset, shape in (("mnist32", (1, 32, 32)), ("svhn", (3, 32, 32))):
        np.save(tmp_path / f"{preset}.npy", rng.uniform(-1, 1, (6, *shape)).astype(np.float32))
        r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.train_flow", "--preset", preset,
                            "--data", str(tmp_path / f"{preset}.npy"), "--epochs", "2", "--batch_size", "4",
                            "--save_every", "2", "--out_dir", str(out)],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        stem = "flow_" + preset
        for name in (f"{stem}_best.pth", f"{stem}_epoch2.pth"):
            ck = torch.load(out / name, map_location="cpu")
            assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_loss"}
    from ratio_guided_multimodal_fm_amd.models import FlowMatchingUNetMNIST
    m = FlowMatchingUNetMNIST(32).to(dev)
    info = load_checkpoint(m, str(out / "flow_mnist32_best.pth"), dev)
    assert info["epoch"] >= 1
    m.eval()
    assert torch.isfinite(m(torch.randn(2, 1, 32, 32, device=dev), torch.full((2,), 0.5, device=dev))).all()
    # the sampler CLI loads both under the reference's checkpoint names
    r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.sample_mnist_svhn", "--num_samples", "2",
                        "--num_steps", "2", "--guidance_method", "none"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Loaded checkpoints/flow_mnist32_best.pth" in r.stdout and "Loaded checkpoints/flow_svhn_best.pth" in r.stdout
