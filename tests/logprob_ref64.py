"""float64 likelihood of images under a velocity U-Net: the yardstick of tests/test_logprob_cpu.py and
tests/test_gpu_logprob.py.

Nothing new is restated here: velocity and J^T u come from the pinned float64 forward (unet_ref64.forward64) and
torch.autograd through it; `integrate_logp64` adds the stepping rule of rgfm_unet_log_prob (include/rgfm.h):

    dt = 1 / N; for i = N - 1 ... 0, t_hi = (i + 1) dt
    euler:     k = v(x, t_hi), D = div(x, t_hi);                                  x -= dt k,  A += dt D
    midpoint:  k1 = v(x, t_hi), x_mid = x - (dt / 2) k1, t_m = t_hi - dt / 2,
               k2 = v(x_mid, t_m), D = div(x_mid, t_m);                           x -= dt k2, A += dt D
    logp[b] = -|z_b|^2 / 2 - (d / 2) log(2 pi) - A[b]

with div[b] = (1 / K) sum_k <eps_k[b], J^T eps_k[b]> for the caller's probes eps [K, B, C, H, W].
"""
import math

import numpy as np
import torch

import unet_ref64 as U

SOLVERS = ("euler", "midpoint")


def _net64(net):
    return U.cfg_of(net), U.params64(net, requires_grad=False)


def _t64(t, B):
    t = torch.as_tensor(t, dtype=torch.float64).reshape(-1)
    return t.expand(B) if t.numel() == 1 else t


def vjp64(net, x, t, u):
    """(v, J^T u) in float64: torch.autograd.grad through forward64 with x.requires_grad_()."""
    cfg, sd = _net64(net)
    x64 = torch.as_tensor(x).detach().cpu().double().clone().requires_grad_(True)
    v = U.forward64(cfg, sd, x64, _t64(t, x64.shape[0]))
    (g,) = torch.autograd.grad(v, x64, torch.as_tensor(u).detach().cpu().double())
    return v.detach(), g


def divergence64(net, x, t, eps, with_g=False):
    """(v [B, C, H, W], div [B]) in float64 for probes eps [K, B, C, H, W]; one forward, K reverse passes.
    with_g: (v, div, g [K, B, C, H, W]) with g_k = J^T eps_k (the error bounds of the GPU tests are stated in them)."""
    cfg, sd = _net64(net)
    x64 = torch.as_tensor(x).detach().cpu().double().clone().requires_grad_(True)
    eps64 = torch.as_tensor(eps).detach().cpu().double()
    B, K = x64.shape[0], eps64.shape[0]
    v = U.forward64(cfg, sd, x64, _t64(t, B))
    div = torch.zeros(B, dtype=torch.float64)
    gs = []
    for k in range(K):
        (g,) = torch.autograd.grad(v, x64, eps64[k], retain_graph=k + 1 < K)
        div += (eps64[k] * g).reshape(B, -1).sum(1)
        gs.append(g)
    div = div / max(K, 1)
    return (v.detach(), div, torch.stack(gs) if gs else eps64) if with_g else (v.detach(), div)


def integrate_logp64(vel_div, x, num_steps, solver):
    """(logp [B], z) of the stepping rule above; vel_div(x, t, need_div) -> (v, div [B] or None); float64 numpy arrays.
    Stage 1 of a midpoint step asks for the velocity alone."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be 'euler' or 'midpoint', got {solver!r}")
    x = np.asarray(x, np.float64).copy()
    B = x.shape[0]
    A = np.zeros(B)
    dt = 1.0 / num_steps
    for i in range(num_steps - 1, -1, -1):
        t_hi = (i + 1) * dt
        if solver == "euler":
            k, D = vel_div(x, t_hi, True)
        else:
            k1, _ = vel_div(x, t_hi, False)
            k, D = vel_div(x - (dt / 2) * k1, t_hi - dt / 2, True)
        x = x - dt * k
        A = A + dt * D
    d = x[0].size
    logp = -0.5 * (x.reshape(B, -1) ** 2).sum(1) - 0.5 * d * math.log(2 * math.pi) - A
    return logp, x


def log_prob64(net, x, eps, num_steps, solver, stages=None):
    """(logp [B], z [B, C, H, W]) of `net` in float64 for data x and probes eps [K, B, C, H, W] (numpy float64).
    stages: a list that receives, per divergence stage, g [K, B, C, H, W] = J^T eps_k at that stage (numpy)."""
    eps64 = torch.as_tensor(eps).detach().cpu().double()

    def vel_div(xs, t, need_div):
        xt = torch.from_numpy(np.ascontiguousarray(xs))
        if not need_div:
            return divergence64(net, xt, t, eps64[:0])[0].numpy(), None
        v, div, g = divergence64(net, xt, t, eps64, with_g=True)
        if stages is not None:
            stages.append(g.numpy())
        return v.numpy(), div.numpy()
    return integrate_logp64(vel_div, torch.as_tensor(x).detach().cpu().double().numpy(), num_steps, solver)
