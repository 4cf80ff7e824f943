"""The HIP optimizer step (utils/optim.py: rgfm_adam_grad_norm + rgfm_adam_step) on the GPU: parity with the float64
restatement (tests/optim_ref64.py) measured against torch's own fp32 Adam, the gradient norm, determinism, stream
order, the handle cache (version counters, EMA swap) and train_flow end to end."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import make_generic_unet
from optim_ref64 import RefAdam64
from ratio_guided_multimodal_fm_amd import _lib, train_flow
from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
from ratio_guided_multimodal_fm_amd.utils.optim import Adam

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHUNK = 1024  # ADAM_CHUNK of csrc/rgfm_kernels.h (test_chunk_constant pins it)
# the gradients are consecutive views of one blob: offsets 0, 1024, 1025, 1028, 1033, 1097, 1354, 2379 -- 0, 0, 1, 0, 1,
# 1, 2, 3 mod 4 -- so both the 16-byte path (tensors 0 and 3) and every dword misalignment are taken
SIZES = [CHUNK, 1, 3, 5, 64, 257, CHUNK + 1, 2 * CHUNK + 3]
MISALIGNED_PARAM = 5  # this parameter is itself a view one float into its allocation
STEPS = 5
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def test_chunk_constant():
    src = open(os.path.join(ROOT, "ratio_guided_multimodal_fm_amd", "csrc", "rgfm_kernels.h")).read()
    assert int(re.search(r"constexpr int ADAM_CHUNK = (\d+);", src).group(1)) == CHUNK


def initial_params(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in sizes]


def step_blob(sizes, seed, step):
    return torch.randn(sum(sizes), generator=torch.Generator().manual_seed(seed * 100 + step))


def device_params(init, dev, misaligned=None):
    out = []
    for i, v in enumerate(init):
        if i == misaligned:
            base = torch.empty(v.numel() + 1, device=dev)
            p = base[1:]
            p.copy_(v)
            assert p.data_ptr() % 16 == 4
        else:
            p = v.to(dev).clone()
        out.append(p.requires_grad_(True))
    return out


VARIANTS = {
    "plain": dict(),
    "coupled_wd": dict(weight_decay=0.05),
    "decoupled_wd": dict(weight_decay=0.05, decoupled=True),
    "clip_active": dict(max_grad_norm=0.5),     # (the norm of ~5500 N(0, 1) values is ~74)
    "clip_inactive": dict(max_grad_norm=1e4),
    "ema": dict(ema_decay=0.9),
    "grad_none": dict(ema_decay=0.9, max_grad_norm=0.5, none_at={4: (1, 2)}),  # parameter 4 has no gradient at steps 2-3
    "two_groups": dict(lrs=(1e-2, 1e-3), max_grad_norm=0.5, ema_decay=0.9),
}


def groups_of(params, cfg):
    lrs = cfg.get("lrs", (3e-3,))
    cut = len(params) // 2 if len(lrs) == 2 else len(params)
    parts = [params[:cut], params[cut:]] if len(lrs) == 2 else [params]
    return [dict(params=ps, lr=lr) for ps, lr in zip(parts, lrs)]


def has_grad(cfg, i, step):
    return step not in cfg.get("none_at", {}).get(i, ())


def run_hip(cfg, dev, seed=11, sync_between=False):
    """STEPS steps of utils.optim.Adam; returns (params, exp_avg, exp_avg_sq, ema or None, grad_norm or None)."""
    params = device_params(initial_params(SIZES, seed), dev, MISALIGNED_PARAM)
    opt = Adam(groups_of(params, cfg), weight_decay=cfg.get("weight_decay", 0.0), decoupled=cfg.get("decoupled", False),
               max_grad_norm=cfg.get("max_grad_norm"), ema_decay=cfg.get("ema_decay"))
    blobs = [step_blob(SIZES, seed, s).to(dev) for s in range(STEPS)]  # a fresh allocation per step
    for s in range(STEPS):
        for i, (p, g) in enumerate(zip(params, torch.split(blobs[s], SIZES))):
            p.grad = g if has_grad(cfg, i, s) else None
        before = [g.clone() for g in torch.split(blobs[s], SIZES)]
        opt.step()
        if sync_between:
            torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, torch.split(blobs[s], SIZES)))  # p.grad stays unscaled
    st = [opt.state[p] for p in params]
    return ([p.detach() for p in params], [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st],
            [s["ema"] for s in st] if opt.ema_decay is not None else None, opt.grad_norm)


def run_torch(cfg, dev, seed=11):
    """The same steps through torch.optim.Adam(foreach=False) + clip_grad_norm_ + lerp, fp32 on the same device."""
    params = device_params(initial_params(SIZES, seed), dev)
    wd, decay = cfg.get("weight_decay", 0.0), cfg.get("ema_decay")
    cls = torch.optim.AdamW if cfg.get("decoupled") else torch.optim.Adam
    opt = cls(groups_of(params, cfg), weight_decay=wd, foreach=False)
    ema = [p.detach().clone() for p in params]
    for s in range(STEPS):
        blob = step_blob(SIZES, seed, s).to(dev)
        for i, (p, g) in enumerate(zip(params, torch.split(blob, SIZES))):
            p.grad = g.clone() if has_grad(cfg, i, s) else None
        if cfg.get("max_grad_norm") is not None:
            torch.nn.utils.clip_grad_norm_(params, cfg["max_grad_norm"], foreach=False)
        opt.step()
        if decay is not None:
            with torch.no_grad():
                for e, p in zip(ema, params):
                    if p.grad is not None:
                        e.lerp_(p, 1 - decay)
    st = [opt.state[p] for p in params]
    return ([p.detach() for p in params], [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st],
            ema if decay is not None else None)


def run_ref64(cfg, seed=11):
    init = initial_params(SIZES, seed)
    groups = [dict(g, weight_decay=cfg.get("weight_decay", 0.0), decoupled=cfg.get("decoupled", False))
              for g in groups_of(init, cfg)]
    ref = RefAdam64(groups, max_grad_norm=cfg.get("max_grad_norm"), ema_decay=cfg.get("ema_decay"))
    cut = len(groups[0]["params"])
    for s in range(STEPS):
        gs = [g if has_grad(cfg, i, s) else None for i, g in enumerate(torch.split(step_blob(SIZES, seed, s), SIZES))]
        ref.step([gs[:cut], gs[cut:]] if len(groups) == 2 else [gs])
    return ref.params, ref.exp_avg, ref.exp_avg_sq, ref.ema, ref.grad_norm


@pytest.mark.parametrize("name", list(VARIANTS))
def test_parity_with_float64(dev, name):
    """Per tensor and per quantity: err_hip <= 2 err_torch + 2^-23 max|ref64|, err = max |x - ref64| -- torch's own fp32
    Adam on the same device and inputs is the yardstick; the factor 2 allows another, equally valid fp32 operation
    order, the floor is one fp32 ulp of the tensor's scale (for tensors where torch happens to round exactly)."""
    cfg = VARIANTS[name]
    hip, tch, ref = run_hip(cfg, dev), run_torch(cfg, dev), run_ref64(cfg)
    worst = {}
    failures = []
    for q, what in enumerate(("p", "exp_avg", "exp_avg_sq", "ema")):
        if hip[q] is None:
            assert what == "ema" and cfg.get("ema_decay") is None
            continue
        for i, n in enumerate(SIZES):
            r = ref[q][i]
            e_hip = float((hip[q][i].cpu().double() - r).abs().max())
            e_tch = float((tch[q][i].cpu().double() - r).abs().max())
            scale = float(r.abs().max())
            bound = 2 * e_tch + ULP * scale
            print(f"{name} {what}[{i}] n={n}: err_hip={e_hip:.3e} err_torch={e_tch:.3e} ulp*scale={ULP * scale:.3e} "
                  f"err_hip/bound={e_hip / bound if bound else 0.0:.3f}")
            worst[what] = max(worst.get(what, 0.0), e_hip / bound if bound else 0.0)
            if not e_hip <= bound:
                failures.append((what, i, n, e_hip, e_tch, scale))
    print(f"{name}: worst err_hip / bound per quantity: " + ", ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    if cfg.get("max_grad_norm") is not None:
        norm = float(hip[4].item())
        print(f"{name}: grad_norm={norm!r} norm64={ref[4]!r}")
        assert abs(norm - ref[4]) <= 1e-6 * ref[4]
    else:
        assert hip[4] is None
    assert not failures, failures


def test_grad_norm_over_many_small_tensors(dev):
    """300 tensors of 1..7 elements and one of two chunks: |norm - norm64| <= 1e-6 norm64 (float64 accumulation leaves
    only the final fp32 rounding)."""
    sizes = [1 + i % 7 for i in range(300)] + [2 * CHUNK]
    init = initial_params(sizes, 21)
    params = device_params(init, dev)
    blob = step_blob(sizes, 21, 0)
    for p, g in zip(params, torch.split(blob.to(dev), sizes)):
        p.grad = g
    opt = Adam(params, lr=1e-3, max_grad_norm=float("inf"))
    opt.step()
    norm, norm64 = float(opt.grad_norm.item()), float(blob.double().pow(2).sum().sqrt())
    print(f"grad_norm={norm!r} norm64={norm64!r} rel={abs(norm - norm64) / norm64:.3e}")
    assert abs(norm - norm64) <= 1e-6 * norm64
    # infinity reports without clipping: the update is the unclipped one
    ref = RefAdam64([dict(params=init, lr=1e-3)])
    ref.step([list(torch.split(blob, sizes))])
    for i, p in enumerate(params):
        r = ref.params[i]
        assert float((p.detach().cpu().double() - r).abs().max()) <= 4 * ULP * max(float(r.abs().max()), 1e-3), i


def flat(result):
    return [t for part in result[:4] if part is not None for t in part] + ([result[4]] if result[4] is not None else [])


def test_two_runs_are_bitwise_equal(dev):
    cfg = VARIANTS["two_groups"]
    a, b = flat(run_hip(cfg, dev)), flat(run_hip(cfg, dev))
    assert len(a) == len(b) == 4 * len(SIZES) + 1
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_back_to_back_steps_equal_synchronised_steps(dev):
    """Steps enqueued without waiting (each with its gradients in another allocation, so each uploads a new table while
    the previous one may still be in flight) equal the same steps with a synchronisation after each, bitwise."""
    cfg = VARIANTS["grad_none"]
    a, b = flat(run_hip(cfg, dev)), flat(run_hip(cfg, dev, sync_between=True))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_handle_sees_the_step_and_the_ema_swap(dev):
    """g40: the smallest FlexibleUNet of tests/test_gpu_train.py by parameter count."""
    m, x, t = make_generic_unet("g40", dev)
    x, t = x[:2].to(dev), t[:2].to(dev)
    target = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    opt = Adam(m.parameters(), lr=1e-3, ema_decay=0.5)
    v0 = m(x, t).clone()
    h0 = m._engine.handle(dev).value
    loss = F.mse_loss(m.forward_train(x, t), target)
    opt.zero_grad()
    loss.backward()
    opt.step()
    v1 = m(x, t).clone()
    assert m._engine.handle(dev).value == h0  # re-packed in place, not re-created
    assert not torch.equal(v1, v0)
    fresh = make_generic_unet("g40", dev)[0]
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(v1, fresh(x, t))  # (fails if the step does not raise the parameters' version counters)
    averaged = make_generic_unet("g40", dev)[0]
    averaged.load_state_dict(opt.ema_state_dict(m))
    v_avg = averaged(x, t).clone()
    assert not torch.equal(v_avg, v1) and not torch.equal(v_avg, v0)
    with opt.swap_ema(m):
        assert torch.equal(m(x, t), v_avg)
    assert torch.equal(m(x, t), v1)
    assert m._engine.handle(dev).value == h0


def test_train_flow_writes_the_averaged_weights(dev, tmp_path):
    rng = np.random.default_rng(0)
    np.save(tmp_path / "d.npy", rng.uniform(-1, 1, (16, 1, 32, 32)).astype(np.float32))
    common = ["--preset", "mnist32", "--data", str(tmp_path / "d.npy"), "--epochs", "2", "--batch_size", "8",
              "--save_every", "2"]
    train_flow.main(common + ["--out_dir", str(tmp_path / "hip"), "--optimizer", "hip", "--ema_decay", "0"])
    from ratio_guided_multimodal_fm_amd.models import FlowMatchingUNetMNIST
    m = FlowMatchingUNetMNIST(32)
    for name in ("flow_mnist32_best.pth", "flow_mnist32_epoch2.pth"):
        ck = torch.load(tmp_path / "hip" / name, map_location="cpu")
        assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_loss", "ema_state_dict"}
        assert list(ck["ema_state_dict"]) == list(m.state_dict())
        # decay 0: ema = 0 ema + 1 p is exact, so the average is the weights themselves
        for k, v in ck["model_state_dict"].items():
            assert torch.equal(ck["ema_state_dict"][k], v), k
    info = load_checkpoint(m, str(tmp_path / "hip" / "flow_mnist32_epoch2.pth"), ema=True)  # (a strict load)
    assert info["epoch"] == 2
    for k, v in m.state_dict().items():
        assert torch.equal(v, ck["ema_state_dict"][k]), k
    train_flow.main(common + ["--out_dir", str(tmp_path / "torch"), "--optimizer", "torch"])
    ck = torch.load(tmp_path / "torch" / "flow_mnist32_epoch2.pth", map_location="cpu")
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_loss"}
    with pytest.raises(KeyError, match="ema_state_dict"):
        load_checkpoint(m, str(tmp_path / "torch" / "flow_mnist32_epoch2.pth"), ema=True)
