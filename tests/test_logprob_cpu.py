"""The float64 likelihood yardstick (tests/logprob_ref64.py) against closed forms, bits_per_dim on hand-computed values
and the Python layer's argument checks that run before any device call.  No GPU."""
import math

import numpy as np
import pytest
import torch

import logprob_ref64 as R
from helpers import make_module
from unet_ref64 import cfg_of, forward64, params64
from ratio_guided_multimodal_fm_amd import CFMSchedule, bits_per_dim, joint_log_prob
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd._lib import RgfmError
from ratio_guided_multimodal_fm_amd.synth import load_synth

TINY = dict(in_channels=1, img_size=8, model_channels=32, channel_mult=(1, 2), num_res_blocks=1)


def tiny_net():
    return load_synth(M.FlexibleUNet(**TINY), 60).eval()


def test_scaled_basis_probes_give_the_exact_trace():
    net = tiny_net()
    g = torch.Generator().manual_seed(61)
    x = torch.randn(1, 1, 8, 8, generator=g, dtype=torch.float64)
    t = torch.tensor([0.3], dtype=torch.float64)
    d = 64
    eps = (math.sqrt(d) * torch.eye(d, dtype=torch.float64)).reshape(d, 1, 1, 8, 8)
    _, div = R.divergence64(net, x, t, eps)
    cfg, sd = cfg_of(net), params64(net, requires_grad=False)
    J = torch.autograd.functional.jacobian(lambda a: forward64(cfg, sd, a, t), x).reshape(d, d)
    trace = float(torch.trace(J))
    assert abs(trace) > 1e-3  # a net whose divergence is not trivially zero
    assert abs(float(div[0]) - trace) <= 1e-10 * abs(trace)


def test_vjp64_is_the_jacobian_transposed():
    net = tiny_net()
    g = torch.Generator().manual_seed(62)
    x = torch.randn(1, 1, 8, 8, generator=g, dtype=torch.float64)
    u = torch.randn(1, 1, 8, 8, generator=g, dtype=torch.float64)
    t = torch.tensor([0.7], dtype=torch.float64)
    cfg, sd = cfg_of(net), params64(net, requires_grad=False)
    J = torch.autograd.functional.jacobian(lambda a: forward64(cfg, sd, a, t), x).reshape(64, 64)
    _, gu = R.vjp64(net, x, t, u)
    want = J.T @ u.reshape(-1)
    assert float((gu.reshape(-1) - want).abs().max()) <= 1e-12 * float(want.abs().max())


def linear_field(a):
    """v(x, t) = a * x elementwise: x(0) = x(1) exp(-a), div v = sum a."""
    return lambda x, t, need_div: (a * x, np.full(x.shape[0], a.sum()) if need_div else None)


@pytest.mark.parametrize("solver,ratio", [("euler", 2.0), ("midpoint", 4.0)])
def test_integrator_order_on_a_linear_field(solver, ratio):
    rng = np.random.default_rng(63)
    a = rng.uniform(-0.8, 0.8, (1, 2, 3, 3))
    x = rng.standard_normal((4, 2, 3, 3))
    d = 18
    z_true = x * np.exp(-a)
    logp_true = -0.5 * (z_true.reshape(4, -1) ** 2).sum(1) - 0.5 * d * math.log(2 * math.pi) - a.sum()
    errs_z, errs_l = [], []
    for N in (16, 32, 64):
        logp, z = R.integrate_logp64(linear_field(a), x, N, solver)
        errs_z.append(np.abs(z - z_true).max())
        errs_l.append(np.abs(logp - logp_true).max())
    for e in (errs_z, errs_l):
        for coarse, fine in zip(e, e[1:]):
            assert 0.8 * ratio <= coarse / fine <= 1.25 * ratio, (solver, e)
    # the divergence of a linear field is constant: its integral is exact at any N
    A = -(logp + 0.5 * (z.reshape(4, -1) ** 2).sum(1) + 0.5 * d * math.log(2 * math.pi))
    assert np.abs(A - a.sum()).max() <= 1e-12


def test_integrator_rejects_an_unknown_solver():
    with pytest.raises(ValueError, match="solver"):
        R.integrate_logp64(linear_field(np.ones((1, 1, 2, 2))), np.zeros((1, 1, 2, 2)), 2, "rk4")


def test_bits_per_dim_hand_values():
    # logp = 0 nats: only the discretisation term, log2(256 / 2) = 7 bits
    assert bits_per_dim(0.0, 10) == pytest.approx(7.0, abs=1e-15)
    # -d ln 2 nats over d dims is exactly one more bit per dim
    assert bits_per_dim(-3072 * math.log(2.0), 3072) == pytest.approx(8.0, abs=1e-12)
    # data on [0, 1], 256 levels: log2(256) = 8; logp = +d ln 4 takes two bits off
    assert bits_per_dim(784 * math.log(4.0), 784, data_range=1.0) == pytest.approx(6.0, abs=1e-12)
    # tensors pass through elementwise
    out = bits_per_dim(torch.tensor([0.0, -math.log(2.0)], dtype=torch.float64), 1, data_range=2.0, levels=2)
    assert torch.allclose(out, torch.tensor([0.0, 1.0], dtype=torch.float64), atol=1e-15)
    with pytest.raises(ValueError):
        bits_per_dim(0.0, 0)
    with pytest.raises(ValueError):
        bits_per_dim(0.0, 4, data_range=0.0)


def test_python_argument_checks_run_before_any_device_call():
    # CPU modules and CPU tensors: every error below must come from the argument checks, none from a device call
    m = make_module("mnist32")
    x = torch.zeros(2, 1, 32, 32)
    s = CFMSchedule()
    with pytest.raises(ValueError, match="solver"):
        s.log_prob(m, x, solver="rk4")
    with pytest.raises(ValueError, match="num_steps"):
        s.log_prob(m, x, num_steps=0)
    with pytest.raises(ValueError, match="num_steps"):
        s.log_prob(m, x, num_steps=2049, solver="midpoint")
    with pytest.raises(ValueError, match="num_steps"):
        s.log_prob(m, x, num_steps=4097, solver="euler")
    with pytest.raises(ValueError, match="n_probes"):
        s.log_prob(m, x, n_probes=0)
    with pytest.raises(ValueError, match="n_probes"):
        s.log_prob(m, x, n_probes=-1)
    with pytest.raises(ValueError, match="batch_size"):
        s.log_prob(m, x, batch_size=0)
    with pytest.raises(ValueError, match="shape"):
        s.log_prob(m, torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="solver"):
        s.encode(m, x, solver="heun")
    with pytest.raises(ValueError, match="num_steps"):
        s.encode(m, x, num_steps=-3)
    with pytest.raises(RgfmError, match="U-Net"):
        s.log_prob(make_module("fm_original"), torch.zeros(2, 1, 28, 28))
    with pytest.raises(RgfmError, match="U-Net"):
        s.encode(make_module("fm_original"), torch.zeros(2, 1, 28, 28))
    with pytest.raises(ValueError, match="pair up"):
        joint_log_prob(m, m, make_module("ratio_ms"), x, torch.zeros(3, 1, 32, 32))
    # valid arguments on the CPU: the loud no-CPU-path error, as everywhere in the package
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.log_prob(m, x, num_steps=2)
    with pytest.raises(RgfmError, match="HIP device|no CPU path"):
        m.vjp(x, torch.zeros(2), x)
    with pytest.raises(RgfmError, match="HIP device|no CPU path"):
        m.divergence(x, torch.zeros(2), x[None])
