"""float64 numpy restatement of the ONE-SIDED MC guidance block of conditional sampling (rgfm_sample_cond,
rgfm_guidance_apply_cond) and the inputs its tests run on: the yardstick of tests/test_cond_ref64_cpu.py and
tests/test_gpu_cond.py.

The block is the reference's MC guidance (src/sample_mnist_svhn.py:124-171) with one side observed: the observed
side's Gaussian factor does not depend on the MC index and drops out of the row-normalised weights, and the shared
ratio vector becomes a ratio row R[b] = r(condition_b, m_.) per sample.  cond64 is written out on its own, statement by
statement, in float64 with Python-double scalars; tests/test_cond_ref64_cpu.py ties it to guidance_ref64.guidance64
(itself pinned by the reference project's goldens) on the equivalent paired problem.

spread_case follows guidance_ref64.spread_case with D = dim: m_j = centre c0 + (sigma / (t sqrt D)) u_j and
s_b = t centre c0 + 0.5 (sigma / sqrt D) n_b, so every MC sample carries about 1 / N of every row, and EVERY ROW has
its own ratio row exp(0.5 N(0, 1)): a kernel that reads the wrong row of R moves every weight by tens of per cent.
"""
import functools

import numpy as np

import guidance_ref64 as G

EPS = G.EPS
# (B, N, dim): a one-row .. two-tile batch; N = 70 (not a multiple of 32, a 6-sample tail), 257 (lane runs start past
# N), 1 (everything minimal); dim = 784 (a slice tail), 3072 (six slices, 24 column blocks), 1024 (two full slices)
CASES = [(5, 7, 784), (33, 70, 3072), (3, 257, 1024), (2, 1, 784)]
STEPS = G.STEPS
CENTRES = G.CENTRES


def cond64(s, v, m, R, t, gamma):
    """(v', w, l, g) in float64; s, v [B, d], m [N, d], R [B, N]."""
    s, v, m, R = (np.asarray(a, np.float64) for a in (s, v, m, R))
    s, v, m = (a.reshape(a.shape[0], -1) for a in (s, v, m))
    B, N = s.shape[0], m.shape[0]
    t, gamma = float(t), float(gamma)
    sigma = 1 - t + EPS
    l = np.empty((B, N))
    for b in range(B):
        l[b] = -0.5 * ((s[b] - t * m) ** 2).sum(-1) / sigma ** 2
    p = np.exp(l - l.max(1, keepdims=True))
    pbar = p.mean(1, keepdims=True) + 1e-10
    zbar = (R * p).mean(1, keepdims=True) + 1e-10
    w = (R / zbar) * (p / pbar)
    w = w / (w.sum(1, keepdims=True) + 1e-10)
    g = np.empty_like(s)
    for b in range(B):
        g[b] = (w[b][:, None] * ((m - s[b]) / (1 - t + EPS))).sum(0)
    return (1 - gamma) * v + gamma * g, w, l, g


def spread_case(B, N, dim, t, seed, centre):
    """{s, v, m, R}: fp32 arrays, s / v [B, dim], m [N, dim], R [B, N] (a distinct ratio row per sample)."""
    g = np.random.default_rng(seed)
    sigma = 1 - t + EPS
    c0 = g.standard_normal(dim)
    u = g.standard_normal((N, dim))
    n = g.standard_normal((B, dim))
    m = centre * c0 + (sigma / (t * np.sqrt(dim))) * u
    s = t * centre * c0 + 0.5 * (sigma / np.sqrt(dim)) * n
    R = np.exp(0.5 * g.standard_normal((B, N)))
    v = g.standard_normal((B, dim))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"s": f(s), "v": f(v), "m": f(m), "R": f(R)}


def seed_of(ci, si, centre):
    return 5000 + 100 * ci + 10 * si + int(centre)


def reference_of(inp, t, gamma):
    v, w, l, g = cond64(inp["s"], inp["v"], inp["m"], inp["R"], t, gamma)
    ref = {"v": v, "w": w, "l": l, "g": g}
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def case(ci, si, centre):
    """(inputs, float64 reference) of CASES[ci] at STEPS[si]: built once per process and shared, read-only."""
    B, N, dim = CASES[ci]
    t, gamma = STEPS[si]
    inp = spread_case(B, N, dim, t, seed_of(ci, si, centre), centre)
    for a in inp.values():
        a.setflags(write=False)
    return inp, reference_of(inp, t, gamma)


def velocity_bound(inp, ref, N, t, gamma, tw):
    """guidance_ref64.velocity_bound, unchanged, on the one modality there is (it takes the max over two)."""
    return G.velocity_bound({"mx": inp["m"], "my": inp["m"]}, {"gx": ref["g"], "gy": ref["g"], "vx": ref["v"], "vy": ref["v"]},
                            N, t, gamma, tw)


def sample_cond64(velocity, s, m, R, num_steps, gamma, step_begin=0, step_end=None):
    """The one-net guided Euler loop in float64: velocity(s, t) -> [B, ...] float64 array; returns the final state."""
    s = np.asarray(s, np.float64).copy()
    shape = s.shape
    dt = 1.0 / num_steps
    for step in range(step_begin, num_steps if step_end is None else step_end):
        t = step * dt
        v = np.asarray(velocity(s, t), np.float64)
        if t > EPS:
            v = cond64(s, v.reshape(shape[0], -1), m, R, t, gamma)[0].reshape(shape)
        s = s + v * dt
    return s
