"""float64 sampler loops with a choice of solver: the yardstick of tests/test_ode_cpu.py and tests/test_gpu_ode.py.

Nothing new is restated here: the loops are COMPOSED from the float64 pieces that are already pinned --
unet_ref64.forward64 (velocity), guidance_ref64.guidance64 (paired MC block), cond_ref64.cond64 (one-sided MC block),
cond_grad_ref64.grad_both64 / grad_given64 (gradient of the log-ratio) -- and `integrate64` adds the stepping rule:

    euler:     s <- s + dt F(s, t1)                                   t1 = i dt
    midpoint:  s_mid = s + (dt / 2) F(s, t1);  s <- s + dt F(s_mid, t2)   t2 = (i + 0.5) dt

with F the loop's whole guided velocity at the stage's own state and time; the MC blocks guide a stage iff its own
t > 1e-3.  With solver='euler' the loops are the existing Euler references (cond_ref64.sample_cond64,
cond_grad_ref64.sample_cond_grad64), which tests/test_ode_cpu.py asserts.

States are tuples of float64 numpy arrays (one per modality), F returns a tuple of the same shapes.
"""
import functools

import numpy as np
import torch

import cond_grad_ref64 as CG
import cond_ref64 as C
import guidance_ref64 as G
import unet_ref64 as U

EPS = G.EPS
SOLVERS = ("euler", "midpoint")


def integrate64(F, state, num_steps, solver="euler", step_begin=0, step_end=None):
    """The end state of steps [step_begin, step_end) of `num_steps`; F(state, t) -> tuple of velocities."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be 'euler' or 'midpoint', got {solver!r}")
    s = tuple(np.asarray(a, np.float64).copy() for a in state)
    dt = 1.0 / num_steps
    for i in range(step_begin, num_steps if step_end is None else step_end):
        t1 = i * dt
        if solver == "euler":
            s = tuple(a + v * dt for a, v in zip(s, F(s, t1)))
        else:
            mid = tuple(a + (dt / 2) * k for a, k in zip(s, F(s, t1)))
            s = tuple(a + dt * k for a, k in zip(s, F(mid, (i + 0.5) * dt)))
    return s


def velocity_of(net):
    """v(x [B, C, H, W] float64 numpy, t) of a FlexibleUNet module in float64."""
    cfg, sd = U.cfg_of(net), U.params64(net, requires_grad=False)
    return lambda x, t: U.forward64(cfg, sd, torch.from_numpy(np.ascontiguousarray(x)), torch.tensor([t])).numpy()


def guided_after_eps(t):
    return t > EPS


def F_single(vel):
    return lambda s, t: (np.asarray(vel(s[0], t), np.float64),)


def F_pair_mc(velx, vely, mx, my, r, gamma, guide=guided_after_eps):
    """Paired loop with the MC block; n_mc = 0 (mx None): two independent nets.  `guide(t)`: is a stage at t guided."""
    def F(s, t):
        x, y = s
        vx, vy = np.asarray(velx(x, t), np.float64), np.asarray(vely(y, t), np.float64)
        if mx is not None and guide(t):
            B = x.shape[0]
            gx, gy = G.guidance64(x.reshape(B, -1), y.reshape(B, -1), vx.reshape(B, -1), vy.reshape(B, -1), mx, my, r, t, gamma)[:2]
            vx, vy = gx.reshape(x.shape), gy.reshape(y.shape)
        return vx, vy
    return F


def F_cond_mc(vel, m, R, gamma, guide=guided_after_eps):
    def F(s, t):
        v = np.asarray(vel(s[0], t), np.float64)
        if guide(t):
            shape = s[0].shape
            v = C.cond64(s[0], v.reshape(shape[0], -1), m, R, t, gamma)[0].reshape(shape)
        return (v,)
    return F


def F_pair_grad(velx, vely, rr, gamma, loss_type="disc"):
    """v + gamma grad log r(x, y) for both modalities (rr: a ratio estimator module)."""
    kind, sd = CG.kind_of(rr), CG.params64(rr)

    def F(s, t):
        x, y = s
        gx, gy, _ = CG.grad_both64(kind, sd, torch.from_numpy(x), torch.from_numpy(y), loss_type)
        return velx(x, t) + gamma * gx.numpy(), vely(y, t) + gamma * gy.numpy()
    return F


def F_cond_grad(vel, rr, cond, given, gamma, loss_type="disc"):
    kind, sd = CG.kind_of(rr), CG.params64(rr)

    def F(s, t):
        g = CG.grad_given64(kind, sd, cond, torch.from_numpy(s[0]), given, loss_type)[0]
        return (vel(s[0], t) + gamma * g.numpy(),)
    return F


# ------------------------------------------------------------------ the truncation-order case (CPU and GPU tests share it)
@functools.lru_cache(maxsize=None)
def g16_case():
    """(module, x0 [3, 1, 16, 16] fp32 numpy): the generic U-Net g16 and the first 3 rows of its fixture input."""
    from helpers import make_generic_unet
    net, x, _ = make_generic_unet("g16")
    return net, x[:3].numpy().copy()


@functools.lru_cache(maxsize=None)
def g16_unguided(solver, num_steps):
    """float64 end state of the unguided loop of g16_case: computed once per (solver, N), shared, read-only."""
    net, x0 = g16_case()
    out = integrate64(F_single(velocity_of(net)), (x0,), num_steps, solver)[0]
    out.setflags(write=False)
    return out
