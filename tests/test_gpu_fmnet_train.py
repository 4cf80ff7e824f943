"""Training pass of FlowMatchingModel on the GPU (rgfm_fmnet_forward_train / _backward / _update_params): gradients
against a float64 restatement (tests/fmnet_ref64.py) and against the reference's autograd
(tests/golden/fmnet_train_grad.npz), determinism, the no-dx path, the CFM training loop, the hand-back to sampling
and the CLI.

Tolerance: max |g - g64| <= 1e-4 * max |g64| per tensor, the project's training tolerance (tests/test_gpu_train.py,
tests/test_gpu_ratio_train.py).  The reference's own fp32 autograd differs from float64 by at most 3.8e-6 of a
tensor's max over these cases (`ref32_err` of the fixture, asserted to be within a third of the tolerance in
tests/test_fmnet_train_cpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fmnet_ref64 import forward64, params64
from helpers import golden, make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth
from ratio_guided_multimodal_fm_amd.utils.flow_utils import CFMSchedule, train_flow_matching_epoch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL_GRAD = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def train_case(F_dim, T_dim, batch):  # must match tests/golden/make_fmnet_train_golden.py
    g = torch.Generator().manual_seed(900 + F_dim + T_dim + batch)
    return (torch.randn(batch, 1, 28, 28, generator=g), torch.rand(batch, generator=g),
            torch.randn(batch, 1, 28, 28, generator=g))


def module_of(F_dim, T_dim, dev):
    return load_synth(M.FlowMatchingModel(1, F_dim, T_dim), 19).eval().to(dev)


def hip_grads(m, x, t, target, need_dx=True):
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(need_dx)
    v = m.forward_train(xg, t)
    loss = F.mse_loss(v, target)
    loss.backward()
    return loss.item(), xg.grad, [p.grad for p in m.parameters()], v.detach()


def ref64_grads(m, x, t, target):
    sd = params64(m)
    x64 = x.detach().cpu().double().requires_grad_(True)
    loss = F.mse_loss(forward64(sd, x64, t.cpu()), target.cpu().double())
    loss.backward()
    return loss.item(), x64.grad, [sd[k].grad for k in m.state_dict()]


def assert_close(g, g64, what):
    g = g.detach().cpu().double()
    scale = float(g64.abs().max())
    err = float((g - g64).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} rel {err / max(scale, 1e-30):.3e}")
    assert err <= TOL_GRAD * max(scale, 1e-30), (what, err, scale)


# (feature_dim, time_emb_dim, batch, one shared t): batch 37 -> pixel counts 37 * 784 / 196 / 49, none a multiple of
# 64; batch 5 -> the Linear weight gradients' K below one staging chunk; (64, 16): the smallest descriptor; (320, 48):
# F + T = 368, no multiple of 64; batch 1
CASES = [(256, 128, 37, False), (64, 16, 5, True), (320, 48, 1, False)]


@pytest.mark.parametrize("F_dim,T_dim,batch,shared_t", CASES)
def test_gradients_vs_float64(dev, F_dim, T_dim, batch, shared_t):
    m = module_of(F_dim, T_dim, dev)
    x, t, target = train_case(F_dim, T_dim, batch)
    if shared_t:
        t = t[:1]  # t_count == 1
    loss, dx, grads, _ = hip_grads(m, x.to(dev), t.to(dev), target.to(dev))
    loss64, dx64, grads64 = ref64_grads(m, x, t, target)
    print(f"loss {loss:.8e} loss64 {loss64:.8e}")
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert_close(dx, dx64, "dx")
    for (name, _), g, g64 in zip(m.state_dict().items(), grads, grads64):
        assert_close(g, g64, name)


def test_gradients_vs_reference_autograd(dev):
    gold = golden("fmnet_train_grad")
    m = make_module("fm_original", dev)
    x, t, target = train_case(256, 128, 2)
    loss, dx, grads, _ = hip_grads(m, x.to(dev), t.to(dev), target.to(dev))
    assert abs(loss - float(gold["loss"])) <= 1e-5 * abs(float(gold["loss"]))
    r = gold["dx"]
    assert np.abs(dx.cpu().numpy() - r).max() <= TOL_GRAD * np.abs(r).max()
    for i, g in enumerate(grads):
        gf = g.reshape(-1).cpu()
        idx = torch.randint(0, gf.numel(), (64,), generator=torch.Generator().manual_seed(7000 + i))
        amax = float(gold[f"amax_{i}"])
        assert abs(float(gf.abs().max()) - amax) <= TOL_GRAD * amax, i
        assert np.abs(gf[idx].numpy() - gold[f"probe_{i}"]).max() <= TOL_GRAD * amax, i


def test_backward_is_deterministic_and_dx_is_optional(dev):
    m = make_module("fm_original", dev)
    x, t, target = (a.to(dev) for a in train_case(256, 128, 37))
    a = hip_grads(m, x, t, target)
    b = hip_grads(m, x, t, target)
    assert torch.equal(a[3], b[3]) and torch.equal(a[1], b[1])
    assert all(torch.equal(u, v) for u, v in zip(a[2], b[2]))
    # x not requiring grad: dx_out is null, the parameter gradients are bitwise the same
    c = hip_grads(m, x, t, target, need_dx=False)
    assert c[1] is None
    assert torch.equal(a[3], c[3])
    assert all(torch.equal(u, v) for u, v in zip(a[2], c[2]))


def test_empty_batch(dev):
    m = make_module("fm_original", dev)
    x = torch.zeros(0, 1, 28, 28, device=dev, requires_grad=True)
    v = m.forward_train(x, torch.zeros(0, device=dev))
    assert v.shape == (0, 1, 28, 28)
    v.sum().backward()
    assert x.grad.shape == x.shape
    assert all(p.grad is not None and not p.grad.any() for p in m.parameters())


def test_training_mode_forward_still_raises(dev):
    m = make_module("fm_original", dev).train()
    with pytest.raises(_lib.RgfmError, match="forward_train"):
        m(torch.zeros(2, 1, 28, 28, device=dev), torch.zeros(2, device=dev))
    m.eval()


def test_sgd_steps_match_float64(dev):
    m = make_module("fm_original", dev)
    data = torch.randn(6, 1, 28, 28, generator=torch.Generator().manual_seed(5))
    lr = 0.05
    sd64 = params64(m, requires_grad=False)
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    sched = CFMSchedule()
    for step in range(5):
        # the loop's draws (t, then x_0) replayed for the float64 side
        state = torch.cuda.get_rng_state(dev)
        train_flow_matching_epoch(m, [{"x": data}], opt, sched, dev)
        torch.cuda.set_rng_state(state, dev)
        t = torch.rand(6, device=dev)
        x0 = torch.randn(6, 1, 28, 28, device=dev)
        tt = t.view(-1, 1, 1, 1)
        xt, u = ((1 - tt) * x0 + tt * data.to(dev)), data.to(dev) - x0
        p64 = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
        loss = F.mse_loss(forward64(p64, xt.cpu(), t.cpu()), u.cpu().double())
        loss.backward()
        sd64 = {k: (v - lr * v.grad).detach() for k, v in p64.items()}
    for k, v in m.state_dict().items():
        r = sd64[k]
        err = float((v.cpu().double() - r).abs().max())
        assert err <= 1e-4 * max(float(r.abs().max()), 1e-12), (k, err)


def test_hand_back_to_sampling(dev):
    m = make_module("fm_original", dev)
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
    assert m._engine.handle(dev).value == h0  # repacked in place (rgfm_fmnet_update_params), not re-created
    assert not torch.equal(v, v_before)
    fresh = M.FlowMatchingModel().to(dev).eval()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(v, fresh(x, t))
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    s1 = CFMSchedule().sample(m, 4, num_steps=5, device=dev)
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    s2 = CFMSchedule().sample(fresh, 4, num_steps=5, device=dev)
    assert torch.equal(s1, s2)
    # the split-bf16 images were refreshed too
    for e in (m._engine, fresh._engine):
        e.set_conv_mode(dev, _engine.CONV_BX3)
    try:
        assert torch.equal(m(x, t), fresh(x, t))
    finally:
        for e in (m._engine, fresh._engine):
            e.set_conv_mode(dev, _engine.CONV_DEFAULT)


def test_cli_end_to_end(dev, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    rng = np.random.default_rng(0)
    out = tmp_path / "checkpoints"
    for modality, stem in (("x", "flow_x"), ("y", "flow_y_rotate90")):
        np.save(tmp_path / f"{modality}.npy", rng.uniform(-1, 1, (6, 1, 28, 28)).astype(np.float32))
        r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.train_flow", "--preset", "original",
                            "--modality", modality, "--data", str(tmp_path / f"{modality}.npy"), "--epochs", "2",
                            "--batch_size", "4", "--save_every", "2", "--out_dir", str(out)],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        for name in (f"{stem}_best.pth", f"{stem}_epoch2.pth"):
            ck = torch.load(out / name, map_location="cpu")
            assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_loss"}
    r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.sample", "--model", "original",
                        "--num_samples", "2", "--num_steps", "2", "--guidance_method", "none"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checkpoints/flow_x_best.pth" in r.stdout and "checkpoints/flow_y_rotate90_best.pth" in r.stdout
