"""Training pass of the ratio estimators on the GPU (rgfm_ratio_forward_train / rgfm_ratio_backward /
rgfm_ratio_update_params): gradients against a float64 restatement fed the library's pool choices and dropout masks
(tests/ratio_ref64.py) and against the reference's autograd (tests/golden/ratio_train_grad.npz), BatchNorm buffers,
dropout, determinism, row coupling, optimiser steps, the hand-back to evaluation / sampling and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, make_module
from ratio_ref64 import forward64, kind_of, params64
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd.utils.losses import get_ratio_loss

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL_GRAD = 1e-4   # max |g - g64| <= TOL_GRAD * max |g64| per tensor (tests/test_gpu_train.py)
TOL_LOSS = 1e-5   # relative
TOL_SCORE = 1e-5  # absolute
TOL_STATS = 1e-5  # of the tensor's maximum
SHAPES = {"ratio_ms": ((1, 32, 32), (3, 32, 32)), "ratio28": ((1, 28, 28), (1, 28, 28))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def inputs(tag, B, salt=0):
    g = torch.Generator().manual_seed(900 + B + 1000 * salt + (0 if tag == "ratio_ms" else 7))
    return torch.randn(B, *SHAPES[tag][0], generator=g), torch.randn(B, *SHAPES[tag][1], generator=g)


def real_mask(B, all_real=False):
    return torch.ones(B, dtype=torch.bool) if all_real else torch.arange(B) % 2 == 0


def loss_of(scores, real, loss_type):
    """The trainers' loss: the ratio loss, or BCE on the one class present (train_ratio.train_epoch_mnist_svhn)."""
    real = real.to(scores.device)
    if real.all():
        return F.binary_cross_entropy_with_logits(scores, torch.ones_like(scores))
    return get_ratio_loss(loss_type)(scores[real], scores[~real])[0]


def set_dropout(m, p):
    for l in m.score_net:
        if isinstance(l, torch.nn.Dropout):
            l.p = p


def hip_run(m, x, y, real, loss_type, training, dev):
    """One forward_train + backward; returns what the float64 side needs to follow it."""
    m.train(training)
    m.zero_grad(set_to_none=True)
    xg, yg = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    scores = m.forward_train(xg, yg)
    choices = [[c.cpu() for c in enc] for enc in m._engine.pool_choices()]
    loss = loss_of(scores, real, loss_type)
    loss.backward()
    m.eval()
    return dict(scores=scores.detach().cpu(), loss=loss.item(), dx=xg.grad.cpu(), dy=yg.grad.cpu(), choices=choices,
                grads={k: p.grad.cpu() for k, p in m.named_parameters()})


def ref_run(kind, sd, x, y, real, loss_type, training, choices, masks=None, p_drop=0.0):
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    out = {}
    scores = forward64(kind, sd, x64, y64, training, choices, masks, p_drop, out)
    loss = loss_of(scores, real, loss_type)
    loss.backward()
    return dict(scores=scores.detach(), loss=loss.item(), dx=x64.grad, dy=y64.grad, out=out,
                grads={k: v.grad for k, v in sd.items() if v.requires_grad})


def assert_close(g, g64, what, tol=TOL_GRAD):
    scale = float(g64.abs().max())
    err = float((g.double() - g64).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / max(scale, 1e-300):.3e}")
    assert err <= tol * max(scale, 1e-30), (what, err, scale)


def check_choices(choices, wins):
    """Every choice the library made is a near-argmax in float64, and the exact float64 argmax in >= 99.9 % of windows."""
    exact = total = 0
    for enc_c, enc_w in zip(choices, wins):
        assert len(enc_c) == len(enc_w)
        for c, w in zip(enc_c, enc_w):
            k = c.to(torch.int64)
            assert int(k.min()) >= 0 and int(k.max()) <= 3
            chosen = w.gather(-1, k[..., None])[..., 0]
            assert bool((chosen >= w.max(-1).values - 1e-5 * float(w.abs().max())).all())
            exact += int((k == w.argmax(-1)).sum())
            total += k.numel()
    print(f"pool choices: {exact} / {total} are the float64 argmax")
    assert exact >= 0.999 * total, (exact, total)


def compare(m, kind, hip, ref, training, sd_before):
    assert float((hip["scores"].double() - ref["scores"]).abs().max()) <= TOL_SCORE
    assert abs(hip["loss"] - ref["loss"]) <= TOL_LOSS * abs(ref["loss"])
    check_choices(hip["choices"], ref["out"]["windows"])
    assert_close(hip["dx"], ref["dx"], "dx")
    assert_close(hip["dy"], ref["dy"], "dy")
    for k, g in hip["grads"].items():
        bn_conv = kind == "mnist_svhn" and training and ".conv" in k and k.endswith(".bias")
        if bn_conv:  # analytically zero: bounded against the scale of that conv's weight gradient
            wscale = float(ref["grads"][k[:-4] + "weight"].abs().max())
            print(f"{k}: max |g| {float(g.abs().max()):.3e} weight-gradient scale {wscale:.3e}")
            assert float(g.abs().max()) <= TOL_GRAD * wscale, k
        else:
            assert_close(g, ref["grads"][k], k)
    now = m.state_dict()
    for k, v0 in sd_before.items():
        if "running" not in k and "num_batches" not in k:
            continue
        if training:
            r = ref["out"]["buffers"][k]
            if "num_batches" in k:
                assert int(now[k]) == int(v0) + 1 == int(r), k
            else:
                assert float((now[k].cpu().double() - r).abs().max()) <= TOL_STATS * float(r.abs().max()), k
        else:
            assert torch.equal(now[k].cpu(), v0), k  # eval mode leaves the buffers alone, bitwise


GRAD_CASES = [(tag, lt, B, False) for tag in ("ratio_ms", "ratio28") for lt in ("disc", "rulsif") for B in (2, 5, 37, 128)]
GRAD_CASES.append(("ratio_ms", "disc", 5, True))  # an all-real batch: the BCE fallback of the MNIST-SVHN trainer


def run_case(dev, tag, loss_type, B, all_real, training):
    m = make_module(tag, dev)
    set_dropout(m, 0.0)
    kind = kind_of(m)
    x, y = inputs(tag, B)
    real = real_mask(B, all_real)
    sd = params64(m)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    hip = hip_run(m, x, y, real, loss_type, training, dev)
    ref = ref_run(kind, sd, x, y, real, loss_type, training, hip["choices"])
    compare(m, kind, hip, ref, training, before)


@pytest.mark.parametrize("tag,loss_type,B,all_real", GRAD_CASES)
def test_gradients_vs_float64_training_mode(dev, tag, loss_type, B, all_real):
    run_case(dev, tag, loss_type, B, all_real, True)


@pytest.mark.parametrize("tag,loss_type,B,all_real", GRAD_CASES)
def test_gradients_vs_float64_eval_mode(dev, tag, loss_type, B, all_real):
    run_case(dev, tag, loss_type, B, all_real, False)


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
def test_dropout_mask_and_gradients(dev, tag):
    m = make_module(tag, dev)
    p = m.dropout_p()
    assert p == pytest.approx(0.1)
    eng = m._engine
    for block in (0, 1):
        mask = eng.dropout_mask(block, 1234, p, 64, dev)
        n = mask.numel()
        kept = float(mask.sum()) / n
        assert abs(kept - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (block, kept)
        assert set(torch.unique(mask).tolist()) <= {0.0, 1.0}
    assert not torch.equal(eng.dropout_mask(0, 1234, p, 64, dev), eng.dropout_mask(0, 1235, p, 64, dev))
    assert not torch.equal(eng.dropout_mask(0, 1234, p, 64, dev)[:, :256], eng.dropout_mask(1, 1234, p, 64, dev)[:, :256])
    B, kind = 6, kind_of(m)
    x, y = inputs(tag, B, salt=1)
    real = real_mask(B)
    sd = params64(m)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    torch.cuda.manual_seed(99)
    seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())  # drawn like forward_train
    masks = [eng.dropout_mask(b, seed, p, B, dev).cpu() for b in (0, 1)]
    torch.cuda.manual_seed(99)
    hip = hip_run(m, x, y, real, "disc", True, dev)
    ref = ref_run(kind, sd, x, y, real, "disc", True, hip["choices"], masks, p)
    compare(m, kind, hip, ref, True, before)
    # same seed: bitwise-equal scores and gradients; another seed: other scores
    runs = []
    for s in (99, 99, 100):
        m.load_state_dict(before)
        torch.cuda.manual_seed(s)
        r = hip_run(m, x, y, real, "disc", True, dev)
        runs.append(r)
    assert torch.equal(runs[0]["scores"], runs[1]["scores"]) and torch.equal(runs[0]["dx"], runs[1]["dx"])
    assert torch.equal(runs[0]["dy"], runs[1]["dy"])
    assert all(torch.equal(runs[0]["grads"][k], runs[1]["grads"][k]) for k in runs[0]["grads"])
    assert not torch.equal(runs[0]["scores"], runs[2]["scores"])


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
def test_backward_is_deterministic(dev, tag):
    m = make_module(tag, dev)
    set_dropout(m, 0.0)
    x, y = inputs(tag, 37)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    a = hip_run(m, x, y, real_mask(37), "disc", True, dev)
    m.load_state_dict(before)
    b = hip_run(m, x, y, real_mask(37), "disc", True, dev)
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["dy"], b["dy"])
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


def golden_inputs(seed, batch, tag):  # must match tests/golden/make_ratio_train_golden.py (inputs)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, *SHAPES[tag][0], generator=g), torch.randn(batch, *SHAPES[tag][1], generator=g)


@pytest.mark.parametrize("case,tag,training", [("ms_train", "ratio_ms", True), ("ms_eval", "ratio_ms", False),
                                               ("r28_train", "ratio28", True)])
def test_gradients_vs_reference_autograd(dev, case, tag, training):
    gold = golden("ratio_train_grad")
    B = int(gold[f"{case}_batch"])
    m = make_module(tag, dev)
    set_dropout(m, 0.0)
    x, y = golden_inputs(int(gold[f"{case}_seed"]), B, tag)
    hip = hip_run(m, x, y, real_mask(B), "disc", training, dev)
    assert abs(hip["loss"] - float(gold[f"{case}_loss"])) <= TOL_LOSS * abs(float(gold[f"{case}_loss"]))
    assert np.abs(hip["scores"].numpy() - gold[f"{case}_scores"]).max() <= TOL_SCORE
    for name in ("dx", "dy"):
        r = gold[f"{case}_{name}"]
        assert np.abs(hip[name].numpy() - r).max() <= TOL_GRAD * np.abs(r).max(), name
    for k, v in m.state_dict().items():
        if "running" in k:
            r = gold[f"{case}_buf_{k}"]
            assert np.abs(v.cpu().numpy() - r).max() <= TOL_STATS * np.abs(r).max(), k
        elif "num_batches" in k:
            assert int(v) == int(gold[f"{case}_buf_{k}"]), k
    for i, (k, g) in enumerate(hip["grads"].items()):
        gf = g.reshape(-1)
        idx = torch.randint(0, gf.numel(), (64,), generator=torch.Generator().manual_seed(7000 + i))
        amax = float(gold[f"{case}_amax_{i}"])
        if tag == "ratio_ms" and training and ".conv" in k and k.endswith(".bias"):
            # analytically zero, rounding noise on both sides: bounded against that conv's weight gradient (index i - 1)
            assert float(gf.abs().max()) <= TOL_GRAD * float(gold[f"{case}_amax_{i - 1}"]), k
            continue
        assert abs(float(gf.abs().max()) - amax) <= TOL_GRAD * amax, k
        assert np.abs(gf[idx].numpy() - gold[f"{case}_probe_{i}"]).max() <= TOL_GRAD * amax, k


@pytest.mark.parametrize("tag", ["ratio_ms"])
def test_row_coupling_is_real(dev, tag):
    m = make_module(tag, dev)
    set_dropout(m, 0.0)
    x, y = inputs(tag, 4)
    x2 = x.clone()
    x2[1] = x2[1] + 1.0
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out = {}
    for training in (True, False):
        for name, xx in (("a", x), ("b", x2)):
            m.load_state_dict(before)
            m.train(training)
            with torch.no_grad():
                out[training, name] = m.forward_train(xx.to(dev), y.to(dev)).cpu()
    m.eval()
    assert out[True, "a"][0] != out[True, "b"][0]   # batch statistics couple the rows
    assert torch.equal(out[False, "a"][[0, 2, 3]], out[False, "b"][[0, 2, 3]])  # running statistics do not
    assert out[False, "a"][1] != out[False, "b"][1]


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
def test_sgd_steps_match_float64(dev, tag):
    m = make_module(tag, dev)
    set_dropout(m, 0.0)
    kind, B, lr = kind_of(m), 6, 0.05
    x, y = inputs(tag, B, salt=2)
    real = real_mask(B)
    sd64 = params64(m, requires_grad=False)
    names = {k for k, _ in m.named_parameters()}
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    for step in range(5):
        m.train()
        opt.zero_grad()
        scores = m.forward_train(x.to(dev), y.to(dev))
        choices = [[c.cpu() for c in enc] for enc in m._engine.pool_choices()]
        loss_of(scores, real, "disc").backward()
        opt.step()
        p64 = {k: v.clone().requires_grad_(k in names) for k, v in sd64.items()}
        out = {}
        loss_of(forward64(kind, p64, x, y, True, choices, out=out), real, "disc").backward()
        sd64 = {k: (v - lr * v.grad).detach() if k in names else out["buffers"].get(k, v).detach() for k, v in p64.items()}
    m.eval()
    for k, v in m.state_dict().items():
        r = sd64[k].double()
        assert float((v.cpu().double() - r).abs().max()) <= 1e-4 * max(float(r.abs().max()), 1e-12), k


def blob_pairs(n, tag, seed):
    """n pairs: x is a blob in quadrant i % 4 of the image (centre jittered); the real y is a fixed function of x's
    blob position (a blob at the mirrored position in every channel), the fake y is shuffled: it belongs to the next
    item, whose blob sits in another quadrant."""
    g = torch.Generator().manual_seed(seed)
    sx, sy = SHAPES[tag]
    S = sx[1]
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    quad = torch.tensor([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]])[torch.arange(n) % 4]
    c = quad + (torch.rand(n, 2, generator=g) - 0.5) * 0.2
    blob = lambda cx, cy: torch.exp(-((xx - cx[:, None, None]) ** 2 + (yy - cy[:, None, None]) ** 2) / 0.08) * 2 - 1  # noqa: E731
    x = blob(c[:, 0], c[:, 1])[:, None]
    y = blob(-c[:, 0], -c[:, 1])[:, None].expand(n, sy[0], S, S).contiguous()
    real = torch.arange(n) % 2 == 0
    y = torch.where(real[:, None, None, None], y, y[torch.roll(torch.arange(n), -1)])
    return x, y, real


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
def test_adam_learns_a_synthetic_task(dev, tag):
    torch.manual_seed(0)
    m = make_module(tag, dev)
    x, y, real = blob_pairs(64, tag, 6)
    x, y = x.to(dev), y.to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    torch.cuda.manual_seed(1)
    losses = []
    for _ in range(200):
        m.train()
        opt.zero_grad()
        loss = loss_of(m.forward_train(x, y), real, "disc")
        loss.backward()
        opt.step()
        losses.append(loss.item())
    m.eval()
    acc = float(((m(x, y) > 0).cpu() == real).float().mean())
    print(f"first 3 {losses[:3]} last 10 mean {np.mean(losses[-10:]):.4f} eval accuracy {acc:.3f}")
    assert np.mean(losses[-10:]) < 0.5 * np.mean(losses[:3]), (losses[:3], losses[-10:])
    assert acc > 0.9, acc


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
def test_hand_back_to_evaluation_and_sampling(dev, tag):
    from ratio_guided_multimodal_fm_amd._engine import sample_pair_grad
    m = make_module(tag, dev)
    x, y, real = blob_pairs(8, tag, 8)
    x, y = x.to(dev), y.to(dev)
    h0 = m._engine.handle(dev).value
    s_before = m(x, y).clone()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    for _ in range(3):
        m.train()
        opt.zero_grad()
        loss_of(m.forward_train(x, y), real, "disc").backward()
        opt.step()
    m.eval()
    s = m(x, y)
    assert m._engine.handle(dev).value == h0  # refreshed in place (rgfm_ratio_update_params), not re-created
    assert not torch.equal(s, s_before)
    fresh = make_module(tag, dev)
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(s, fresh(x, y))
    assert torch.equal(m.log_ratio(x, y), fresh.log_ratio(x, y))
    for a, b in zip(m.grad_log_ratio(x, y), fresh.grad_log_ratio(x, y)):
        assert torch.equal(a, b)
    # a gradient-guided sampler call on the trained estimator
    fx, fy = (make_module("mnist32", dev), make_module("svhn", dev)) if tag == "ratio_ms" else \
             (make_module("unet28", dev), make_module("unet28_y", dev))
    g = torch.Generator().manual_seed(9)
    xs = torch.randn(2, *SHAPES[tag][0], generator=g).to(dev)
    ys = torch.randn(2, *SHAPES[tag][1], generator=g).to(dev)
    x0 = xs.clone()
    sample_pair_grad(fx, fy, m, xs, ys, 2, 0.5)
    assert torch.isfinite(xs).all() and torch.isfinite(ys).all() and not torch.equal(xs, x0)


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
def test_training_mode_forward_still_raises(dev, tag):
    m = make_module(tag, dev).train()
    x, y = inputs(tag, 2)
    with pytest.raises(_lib.RgfmError, match="training mode"):
        m(x.to(dev), y.to(dev))
    with pytest.raises(_lib.RgfmError, match="forward_train"):
        m.log_ratio(x.to(dev), y.to(dev))
    m.eval()


def test_cli_end_to_end(dev, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    rng = np.random.default_rng(0)
    label = np.array([0, 1, 2, 0, 1, 2])
    for kind, tag in (("mnist_svhn", "ratio_ms"), ("mnist28", "ratio28")):
        sx, sy = SHAPES[tag]
        np.savez(tmp_path / f"{kind}.npz", x=rng.uniform(-1, 1, (6, *sx)).astype(np.float32),
                 y=rng.uniform(-1, 1, (6, *sy)).astype(np.float32), label=label)
        r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.train_ratio", "--kind", kind, "--data",
                            str(tmp_path / f"{kind}.npz"), "--epochs", "2", "--batch_size", "4"],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    for name in ("ratio_disc_mnist_svhn_best.pth", "ratio_disc_rotate90_best.pth"):
        ck = torch.load(tmp_path / "checkpoints" / name, map_location="cpu")
        assert all(torch.is_tensor(v) for v in ck.values()) and "score_net.0.weight" in ck
    # the sampler CLI loads the ratio checkpoint beside flow checkpoints written by train_flow
    for preset, shape in (("mnist32", (1, 32, 32)), ("svhn", (3, 32, 32))):
        np.save(tmp_path / f"{preset}.npy", rng.uniform(-1, 1, (6, *shape)).astype(np.float32))
        r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.train_flow", "--preset", preset, "--data",
                            str(tmp_path / f"{preset}.npy"), "--epochs", "1", "--batch_size", "4"],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.sample_mnist_svhn", "--num_samples", "2",
                        "--num_steps", "2", "--guidance_method", "mc_feng"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Loaded ratio estimator from: checkpoints/ratio_disc_mnist_svhn_best.pth" in r.stdout
