"""Likelihood path of the U-Net on the GPU (rgfm_unet_vjp / rgfm_unet_divergence / rgfm_unet_log_prob and the Python
layers above them) against the float64 yardstick tests/logprob_ref64.py.

Bounds.  J^T u: max|g - g64| <= 1e-4 max|g64| (TOL_GRAD of test_gpu_train.py).  Divergence, from that: per row
|div - div64| <= 1e-4 max_k(max|g64_k| sum|eps_k|).  log_prob, 4 steps: z within 1e-4 absolute (the 4-step sampler
tolerance of the project); logp within TOL_LOGP, which is 10 x the largest |logp - logp64| measured over the eight
cases below on an MI355X (DESIGN.md section 13 lists them; largest 1.22e-4, g24 Euler, where logp is -2732 and an fp32
ulp 2.4e-4) and is checked against the cap sum_stages dt (divergence bound) + 1e-4 sum|z64| that the other bounds already
allow (0.07 to 0.6 for these cases).
"""
import copy
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logprob_ref64 as R
from helpers import make_generic_unet, make_module
from unet_ref64 import cfg_of, forward64, params64
from ratio_guided_multimodal_fm_amd import CFMSchedule, _lib, bits_per_dim, joint_log_prob
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd._engine import _ptr, _stream
from ratio_guided_multimodal_fm_amd.synth import load_synth

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL_GRAD = 1e-4
TOL_Z = 1e-4
TOL_LOGP = 1.22e-3
B = 3
TINY = dict(in_channels=1, img_size=8, model_channels=32, channel_mult=(1, 2), num_res_blocks=1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(tag):
    """(CPU module, x [B, C, H, W], t [B]) -- fixed, shared, never modified."""
    if tag == "tiny":
        net = load_synth(M.FlexibleUNet(**TINY), 60).eval()
        g = torch.Generator().manual_seed(61)
        return net, torch.randn(B, 1, 8, 8, generator=g), torch.tensor([0.1, 0.5, 0.9])
    net, x, t = make_generic_unet(tag)
    return net, x[:B].clone(), t[:B].clone()


@functools.lru_cache(maxsize=None)
def on_dev(tag):
    return copy.deepcopy(case(tag)[0]).to("cuda:0")


@functools.lru_cache(maxsize=None)
def cotangents(tag):
    g = torch.Generator().manual_seed(640 + len(tag))
    x = case(tag)[1]
    return torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g)


@functools.lru_cache(maxsize=None)
def rademacher(tag, K, n=B):
    g = torch.Generator().manual_seed(650 + K)
    x = case(tag)[1]
    return torch.randint(0, 2, (K, n, *x.shape[1:]), generator=g).float() * 2 - 1


@functools.lru_cache(maxsize=None)
def vjp_ref(tag, shared_t, which):
    net, x, t = case(tag)
    return R.vjp64(net, x, t[1:2] if shared_t else t, cotangents(tag)[which])[1]


# ------------------------------------------------------------------ 1. rgfm_unet_vjp
@pytest.mark.parametrize("shared_t", [False, True], ids=["t_per_row", "t_shared"])
@pytest.mark.parametrize("tag", ["g16", "g24"])
def test_vjp_vs_float64_and_backward_bits(dev, tag, shared_t):
    m = on_dev(tag)
    _, x, t = case(tag)
    t = t[1:2] if shared_t else t
    xd, td = x.to(dev), t.to(dev)
    u0, u1 = (u.to(dev) for u in cotangents(tag))
    lin = m.linearize(xd, td)
    got = [lin.vjp(u0), lin.vjp(u1), lin.vjp(u0)]  # a second walk on the same saved state, then the first again
    for which, g in ((0, got[0]), (1, got[1])):
        g64 = vjp_ref(tag, shared_t, which)
        err, scale = float((g.cpu().double() - g64).abs().max()), float(g64.abs().max())
        print(f"vjp {tag} shared_t={shared_t} u{which}: err {err:.3e} scale {scale:.3e} ratio {err / scale:.3e}")
        assert err <= TOL_GRAD * scale, (tag, which, err, scale)
    assert torch.equal(got[0], got[2])
    # the bits of rgfm_unet_backward's dx for the same cotangent, and of the one-call form
    for u, g in ((u0, got[0]), (u1, got[1])):
        xg = xd.clone().requires_grad_(True)
        v = m.forward_train(xg, td)
        v.backward(u)
        assert torch.equal(xg.grad, g)
        assert torch.equal(v.detach(), lin.v)
    assert torch.equal(m.vjp(xd, td, u1), got[1])


# ------------------------------------------------------------------ 2. rgfm_unet_divergence
def div_bound(g64, eps):
    """per row: 1e-4 max_k(max|g64_k| sum|eps_k|)"""
    K, n = eps.shape[:2]
    gmax = g64.reshape(K, n, -1).abs().max(2).values
    return TOL_GRAD * (gmax * eps.double().reshape(K, n, -1).abs().sum(2)).max(0).values


def test_divergence_exact_trace_on_the_tiny_net(dev):
    net, x, t = case("tiny")
    d = 64
    eps = (math.sqrt(d) * torch.eye(d)).reshape(d, 1, 1, 8, 8).expand(d, B, 1, 8, 8).contiguous()
    cfg, sd = cfg_of(net), params64(net, requires_grad=False)
    trace, bound = [], []
    for b in range(B):
        J = torch.autograd.functional.jacobian(lambda a: forward64(cfg, sd, a, t[b:b + 1].double()), x[b:b + 1].double())
        J = J.reshape(d, d)
        trace.append(float(torch.trace(J)))
        bound.append(TOL_GRAD * float((math.sqrt(d) * J).abs().max(1).values.max() * math.sqrt(d)))  # g64_k = 8 J[k, :]
    v, div = on_dev("tiny").divergence(x.to(dev), t.to(dev), eps.to(dev))
    for b in range(B):
        err = abs(float(div[b]) - trace[b])
        print(f"div tiny row {b}: trace {trace[b]:+.6e} err {err:.3e} bound {bound[b]:.3e}")
        assert err <= bound[b], (b, err, bound[b])
    v64 = forward64(cfg, sd, x.double(), t.double())
    assert float((v.cpu().double() - v64).abs().max()) <= 1e-5 * float(v64.abs().max())


def test_divergence_rademacher_g24_and_no_probes(dev):
    net, x, t = case("g24")
    m = on_dev("g24")
    eps = rademacher("g24", 3)
    v64, div64, g64 = R.divergence64(net, x, t, eps, with_g=True)
    bound = div_bound(g64, eps)
    xd, td = x.to(dev), t.to(dev)
    v, div = m.divergence(xd, td, eps.to(dev))
    err = (div.cpu().double() - div64).abs()
    print(f"div g24 K=3: div64 {div64.tolist()} err {err.tolist()} bound {bound.tolist()}")
    assert bool((err <= bound).all()), (err, bound)
    # n_probes = 0: a plain exact-fp32 forward, div_out untouched
    sentinel = torch.full((B,), -777.0, device=dev)
    v0, d0 = m._engine.divergence(xd, td, eps[:0].to(dev), div_out=sentinel)
    assert d0 is sentinel and bool((sentinel == -777.0).all())
    vt = m.forward_train(xd, td)
    assert torch.equal(v0, vt) and torch.equal(v, vt)
    assert float((v.cpu().double() - v64).abs().max()) <= 1e-5 * float(v64.abs().max())


# ------------------------------------------------------------------ 3. rgfm_unet_log_prob
STEPS, K_LOGP = 4, 2
SOLVERS = ("euler", "midpoint")


@functools.lru_cache(maxsize=None)
def logp_ref(tag, solver):
    """(logp64 [B], z64, cap [B]): float64 result and the error the other bounds allow,
    sum_stages dt (divergence bound of the stage) + 1e-4 sum|z64|."""
    net, x, _ = case(tag)
    eps = rademacher(tag, K_LOGP)
    stages = []
    logp, z = R.log_prob64(net, x, eps, STEPS, solver, stages)
    assert len(stages) == STEPS
    cap = sum(div_bound(torch.from_numpy(g), eps) for g in stages).numpy() / STEPS
    cap = cap + TOL_Z * np.abs(z).reshape(B, -1).sum(1)
    return logp, z, cap


def raw_log_prob(m, x, eps, K, steps, sid, z_out, logp_out, dev, short=0, ws_solver=None):
    """rgfm_unet_log_prob as the C ABI takes it: the return code, nothing checked on the Python side."""
    L = _lib.lib()
    with torch.cuda.device(dev):
        h = m._engine.handle(dev)
        n = ctypes.c_size_t()
        _lib.check(L.rgfm_unet_log_prob_workspace_bytes(h, x.shape[0], sid if ws_solver is None else ws_solver, max(K, 0),
                                                        ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
        rc = L.rgfm_unet_log_prob(h, _ptr(x), _ptr(eps), K, steps, sid, _ptr(z_out), _ptr(logp_out), x.shape[0], _ptr(ws),
                                  n.value - short, _stream(dev))
        torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("tag", ["g16", "g24"])
def test_log_prob_vs_float64(dev, tag, solver):
    m = on_dev(tag)
    x = case(tag)[1].to(dev)
    eps = rademacher(tag, K_LOGP).to(dev)
    logp64, z64, cap = logp_ref(tag, solver)
    logp, z = m._engine.log_prob(x, eps, STEPS, solver)
    ez = float(np.abs(z.cpu().double().numpy() - z64).max())
    el = np.abs(logp.cpu().double().numpy() - logp64)
    print(f"log_prob {tag} {solver}: logp64 {logp64.tolist()} |dlogp| {el.tolist()} cap {cap.tolist()} max|dz| {ez:.3e}")
    assert TOL_LOGP <= cap.min()  # the bound in force is inside what the bounds of J^T u and z already allow
    assert ez <= TOL_Z
    assert bool((el <= TOL_LOGP).all()), (el, TOL_LOGP)
    # the encoder: the same z bits, logp_out untouched
    z0 = torch.full_like(x, -5.0)
    sentinel = torch.full((B,), -777.0, device=dev)
    assert raw_log_prob(m, x, None, 0, STEPS, _lib.solver_id(solver), z0, sentinel, dev) == 0
    assert torch.equal(z0, z) and bool((sentinel == -777.0).all())
    assert torch.equal(m._engine.log_prob(x, None, STEPS, solver)[1], z)


# ------------------------------------------------------------------ 4. determinism and rows
@pytest.mark.parametrize("solver", SOLVERS)
def test_log_prob_is_deterministic_and_row_local(dev, solver):
    m = on_dev("g24")
    x = case("g24")[1].to(dev)
    eps = rademacher("g24", K_LOGP).to(dev)
    a = m._engine.log_prob(x, eps, STEPS, solver)
    b = m._engine.log_prob(x, eps, STEPS, solver)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    one = m._engine.log_prob(x[1:2], eps[:, 1:2].contiguous(), STEPS, solver)
    assert float((one[1] - a[1][1:2]).abs().max()) <= TOL_Z
    assert abs(float(one[0][0]) - float(a[0][1])) <= TOL_LOGP


# ------------------------------------------------------------------ 5. Python layer
def test_schedule_log_prob_chunks_and_encode(dev):
    m = on_dev("tiny")
    x = torch.randn(5, 1, 8, 8, generator=torch.Generator().manual_seed(66)).to(dev)
    s = CFMSchedule()
    runs = []
    for bs in (2, 5):
        gen = torch.Generator(device=dev).manual_seed(123)
        runs.append(s.log_prob(m, x, num_steps=2, solver="midpoint", n_probes=2, generator=gen, batch_size=bs))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][0].shape == (5,) and bool(torch.isfinite(runs[0][0]).all())
    assert torch.equal(s.encode(m, x, num_steps=2, solver="midpoint", batch_size=3), runs[0][1])
    # the probes are Rademacher draws of the generator for the whole batch: the engine call on them gives the same bits
    gen = torch.Generator(device=dev).manual_seed(123)
    eps = torch.randint(0, 2, (2, *x.shape), generator=gen, device=dev).float() * 2 - 1
    assert torch.equal(m._engine.log_prob(x, eps, 2, "midpoint")[0], runs[0][0])
    # another seed: other probes, another estimate, the same latents; a CPU generator is accepted too
    other = s.log_prob(m, x, num_steps=2, n_probes=2, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(other[0], runs[0][0]) and torch.equal(other[1], runs[0][1])


def test_joint_log_prob_is_the_sum_of_its_parts(dev):
    fx, fy, rr = make_module("mnist32", dev), make_module("svhn", dev), make_module("ratio_ms", dev)
    g = torch.Generator().manual_seed(67)
    x, y = torch.randn(2, 1, 32, 32, generator=g).to(dev), torch.randn(2, 3, 32, 32, generator=g).to(dev)
    kw = dict(num_steps=2, solver="euler", n_probes=1)
    joint, lx, ly, lr = joint_log_prob(fx, fy, rr, x, y, generator=torch.Generator(device=dev).manual_seed(9), **kw)
    gen = torch.Generator(device=dev).manual_seed(9)
    s = CFMSchedule()
    assert torch.equal(lx, s.log_prob(fx, x, generator=gen, **kw)[0])
    assert torch.equal(ly, s.log_prob(fy, y, generator=gen, **kw)[0])
    assert torch.equal(lr, rr.log_ratio(x, y).reshape(-1))
    assert torch.equal(joint, lx + ly + lr) and joint.shape == (2,) and bool(torch.isfinite(joint).all())


def test_flow_matching_model_has_no_likelihood(dev):
    m = make_module("fm_original", dev)
    x = torch.zeros(2, 1, 28, 28, device=dev)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        CFMSchedule().log_prob(m, x, num_steps=2)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        CFMSchedule().encode(m, x, num_steps=2)


# ------------------------------------------------------------------ 6. errors
def test_argument_errors_leave_the_outputs_untouched(dev):
    m = on_dev("tiny")
    x = case("tiny")[1].to(dev)
    eps = rademacher("tiny", 2).to(dev)
    z = torch.full_like(x, -5.0)
    logp = torch.full((B,), -777.0, device=dev)
    EINVAL, ENOMEM = -1, -2
    assert raw_log_prob(m, x, eps, 2, 2, 7, z, logp, dev, ws_solver=1) == EINVAL        # unknown solver
    assert raw_log_prob(m, x, eps, -1, 2, 1, z, logp, dev) == EINVAL                    # n_probes = -1
    assert raw_log_prob(m, x, eps, 2, 2049, 1, z, logp, dev) == EINVAL                  # 2049 midpoint steps
    assert raw_log_prob(m, x, eps, 2, 4097, 0, z, logp, dev) == EINVAL                  # 4097 Euler steps
    assert raw_log_prob(m, x, eps, 2, 0, 0, z, logp, dev) == EINVAL                     # num_steps = 0
    assert raw_log_prob(m, x, eps, 2, 2, 1, None, logp, dev) == EINVAL                  # null z_out
    assert raw_log_prob(m, x, None, 2, 2, 1, z, logp, dev) == EINVAL                    # probes wanted, none given
    assert raw_log_prob(m, x, eps, 2, 2, 1, z, logp, dev, short=1) == ENOMEM            # one byte short
    assert b"workspace" in _lib.lib().rgfm_last_error()
    assert raw_log_prob(m, x, eps, 2, 2, 1, z, logp, dev, ws_solver=0) == ENOMEM        # sized for Euler
    assert bool((z == -5.0).all()) and bool((logp == -777.0).all())
    L = _lib.lib()
    n = ctypes.c_size_t()
    h = m._engine.handle(dev)
    assert L.rgfm_unet_log_prob_workspace_bytes(h, B, 7, 2, ctypes.byref(n)) == EINVAL
    assert L.rgfm_unet_log_prob_workspace_bytes(h, 0, 1, 2, ctypes.byref(n)) == EINVAL
    # and the same call with good arguments works
    assert raw_log_prob(m, x, eps, 2, 2, 1, z, logp, dev) == 0
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(logp).all()) and not bool((logp == -777.0).any())


# ------------------------------------------------------------------ 7. CLI
def test_cli_end_to_end(dev, tmp_path):
    m = make_module("mnist32", dev)
    ck = tmp_path / "flow_mnist32_best.pth"
    torch.save({"epoch": 1, "model_state_dict": m.state_dict(), "best_loss": 0.5}, ck)
    data = np.random.default_rng(68).uniform(-1, 1, (4, 1, 32, 32)).astype(np.float32)
    np.save(tmp_path / "x.npy", data)
    r = subprocess.run([sys.executable, "-m", "ratio_guided_multimodal_fm_amd.log_prob", "--preset", "mnist32",
                        "--checkpoint", str(ck), "--data", str(tmp_path / "x.npy"), "--num_steps", "2", "--n_probes", "2",
                        "--seed", "31", "--batch_size", "3"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.load(open(tmp_path / "flow_mnist32_best_logprob.json"))
    logp, _ = CFMSchedule().log_prob(m, torch.from_numpy(data).to(dev), num_steps=2, solver="midpoint", n_probes=2,
                                     generator=torch.Generator(device=dev).manual_seed(31), batch_size=4)
    lp = logp.double().cpu()
    bpd = bits_per_dim(lp, 1024)
    assert out["num_images"] == 4 and out["dims"] == 1024
    assert out["logp_mean"] == float(lp.mean()) and out["logp_sem"] == float(lp.std()) / 2.0
    assert out["bits_per_dim_mean"] == float(bpd.mean()) and out["bits_per_dim_sem"] == float(bpd.std()) / 2.0
    assert out["bits_per_dim_mean"] == pytest.approx(7.0 - out["logp_mean"] / (1024 * math.log(2.0)), abs=1e-9)
    st = out["settings"]
    assert (st["preset"], st["num_steps"], st["solver"], st["n_probes"], st["seed"], st["batch_size"]) == \
        ("mnist32", 2, "midpoint", 2, 31, 3)
    assert f"{out['logp_mean']:.4f}" in r.stdout and "bits/dim" in r.stdout
