"""float64 restatement of the stochastic sampler step (include/rgfm.h, "Stochastic sampling"): the yardstick of
tests/test_sde_cpu.py and tests/test_gpu_sde.py.

The noise: the integer part (splitmix64 finaliser over uint64, the two 24-bit uniforms) is exact; Box-Muller is
evaluated in float64.  `noise(seed, m, k, n)` is xi[0..n) of stream m at global step k.

The step, over the F_* builders of tests/ode_ref64.py (F the loop's whole velocity at the stage):

    base = (1 - eta dt) x + sigma_k xi_k          sigma_k = sqrt(2 eta (1 - t) dt),  t = k dt,  dt = 1 / num_steps
    x    = base + ((1 + eta t) dt) F(x, t)

xi_k of modality m of the state tuple is noise(seed, m, k, x.size) in the state's flat [batch][D] order.  With eta = 0
integrate_sde64 runs ode_ref64.integrate64(..., 'euler') itself.
"""
import numpy as np

import ode_ref64 as O

GOLD = np.uint64(0x9E3779B97F4A7C15)
MASK24 = np.uint64(0xFFFFFF)


def fin(z):
    """The splitmix64 finaliser (documented for rgfm_unet_dropout_mask) on uint64 arrays, arithmetic mod 2^64."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def key_of(seed, m, k):
    c = (int(m) << 32 | int(k)) + 1
    return fin(np.uint64((int(seed) + 0x9E3779B97F4A7C15 * c) % (1 << 64)))


def uniforms(seed, m, k, pairs):
    """(u1 in (0, 1], u2 in [0, 1)) of pairs 0 .. pairs - 1: exact multiples of 2^-24."""
    p = np.arange(pairs, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = fin(key_of(seed, m, k) + GOLD * (p + np.uint64(1)))
    u1 = ((z >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((z >> np.uint64(8)) & MASK24).astype(np.float64) * 2.0 ** -24
    return u1, u2


def noise(seed, m, k, n):
    """xi[0..n) of (seed, stream m, global step k) in float64; an odd n ends on a cosine."""
    u1, u2 = uniforms(seed, m, k, (n + 1) // 2)
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty(2 * u1.size, np.float64)
    out[0::2], out[1::2] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return out[:n]


def integrate_sde64(F, state, num_steps, eta, seed, step_begin=0, step_end=None):
    """The end state of Euler-Maruyama steps [step_begin, step_end) of `num_steps`; F(state, t) -> tuple of velocities."""
    if eta == 0:
        return O.integrate64(F, state, num_steps, "euler", step_begin, step_end)
    s = tuple(np.asarray(a, np.float64).copy() for a in state)
    dt = 1.0 / num_steps
    for k in range(step_begin, num_steps if step_end is None else step_end):
        t = k * dt
        sigma = np.sqrt(2.0 * eta * (1.0 - t) * dt)
        v = F(s, t)
        base = tuple((1.0 - eta * dt) * a + sigma * noise(seed, m, k, a.size).reshape(a.shape) for m, a in enumerate(s))
        s = tuple(b + ((1.0 + eta * t) * dt) * f for b, f in zip(base, v))
    return s
