"""float64 numpy restatement of the MC guidance block (reference src/sample_mnist_svhn.py:124-171) and the inputs the
guidance tests run it on: the yardstick of tests/test_guidance_ref64_cpu.py and tests/test_gpu_guidance.py.

guidance64 is the reference's statements in their order, in float64 throughout, the step's scalars Python doubles.

spread_case builds inputs whose importance weights are SPREAD over the whole MC set (independent N(0,1) images make
each row one-hot: a kernel that drops or mis-indexes a sample then goes unnoticed unless that sample is the heavy
one).  With D = dx + dy and sigma = 1 - t + 1e-3

    m_i = centre c0 + (sigma / (t sqrt D)) u_i        x_b = t centre c0 + 0.5 (sigma / sqrt D) n_b

so x_b - t m_i = (sigma / sqrt D) (0.5 n_b - u_i): |.|^2 / sigma^2 is 1.25 +- O(1 / sqrt D) for every pair, l is
O(1), and every sample carries about 1 / N of a row.  centre = 1 puts the MC set around a common image as real
sampling does (sum w m and x sum w cancel); centre = 0 leaves |m|max of the order of |m - x|, where one sample's
term is a visible share of g.
"""
import functools

import numpy as np

EPS = 1e-3

# (B, N, dx, dy): what each one reaches is tabulated in test_gpu_guidance.py
CASES = [(33, 70, 784, 784), (65, 32, 64, 192), (40, 288, 132, 128), (37, 544, 68, 4), (5, 257, 520, 48),
         (2, 33, 2052, 2052), (1, 1, 4, 4), (3, 4096, 8, 4)]
STEPS = [(0.05, 0.5), (0.5, 1.0), (0.9, 2.0), (0.99, 5.0)]  # (t, gamma)
CENTRES = [1.0, 0.0]

# max over CASES of the fp32 oracle's relative weight deviation from float64, max |w32 - w64| / w64, per (t, centre):
# measured by test_guidance_ref64_cpu.py (its docstring has the table), rounded up to two digits.  The weights
# tolerance of the GPU test is 4x this: a different expf and wave-order instead of sequential sums.
ORACLE_DW = {
    (0.05, 1.0): 1.2e-6, (0.5, 1.0): 1.2e-6, (0.9, 1.0): 2.8e-6, (0.99, 1.0): 1.7e-5,
    (0.05, 0.0): 1.1e-6, (0.5, 0.0): 2.6e-6, (0.9, 0.0): 2.0e-6, (0.99, 0.0): 1.6e-6,
}
K_GEMM = 2.1  # test_guidance_late_time_concentrated_weights: 4e-6 |m|max / c at N = 256 = 2.1 sqrt(N) 2^-23 |m|max / c


def tol_w(t, centre):
    return 4.0 * ORACLE_DW[(t, centre)]


def guidance64(x, y, vx, vy, mx, my, r, t, gamma):
    """(vx', vy', w, l) in float64; x, y, v [B, d], m [N, d], r [N]."""
    x, y, vx, vy, mx, my, r = (np.asarray(a, np.float64) for a in (x, y, vx, vy, mx, my, r))
    B, N = x.shape[0], mx.shape[0]
    x, y, vx, vy, mx, my = (a.reshape(a.shape[0], -1) for a in (x, y, vx, vy, mx, my))
    t, gamma = float(t), float(gamma)
    sigma_t = 1 - t + EPS
    s2 = sigma_t ** 2
    c = 1 - t + EPS
    l = np.empty((B, N))
    for b in range(B):  # (row by row: [N, d] temporaries, not [B, N, d])
        l[b] = -0.5 * ((x[b] - t * mx) ** 2).sum(-1) / s2 + -0.5 * ((y[b] - t * my) ** 2).sum(-1) / s2
    p = np.exp(l - l.max(1, keepdims=True))
    p_bar = p.mean(1, keepdims=True) + 1e-10
    z_bar = (r[None] * p).mean(1, keepdims=True) + 1e-10
    w = (r[None] / z_bar) * (p / p_bar)
    w = w / (w.sum(1, keepdims=True) + 1e-10)
    gx, gy = np.empty_like(x), np.empty_like(y)
    for b in range(B):
        gx[b] = (w[b][:, None] * ((mx - x[b]) / c)).sum(0)
        gy[b] = (w[b][:, None] * ((my - y[b]) / c)).sum(0)
    return (1 - gamma) * vx + gamma * gx, (1 - gamma) * vy + gamma * gy, w, l


def spread_case(B, N, dx, dy, t, seed, centre):
    """{x, y, vx, vy, mx, my, r}: fp32 arrays, x / y / v [B, d], m [N, d], r [N]."""
    g = np.random.default_rng(seed)
    D = dx + dy
    sigma = 1 - t + EPS
    c0 = g.standard_normal(D)
    u = g.standard_normal((N, D))
    n = g.standard_normal((B, D))
    m = centre * c0 + (sigma / (t * np.sqrt(D))) * u
    x = t * centre * c0 + 0.5 * (sigma / np.sqrt(D)) * n
    r = np.exp(0.5 * g.standard_normal(N))
    v = g.standard_normal((B, D))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"x": f(x[:, :dx]), "y": f(x[:, dx:]), "vx": f(v[:, :dx]), "vy": f(v[:, dx:]), "mx": f(m[:, :dx]),
            "my": f(m[:, dx:]), "r": f(r)}


def seed_of(ci, si, centre):
    return 1000 + 100 * ci + 10 * si + int(centre)


def velocity_bound(inp, ref, N, t, gamma, tw):
    """The section's bound on max |dv|: the fp32 GEMM's accumulation error ~ K sqrt(N) ulp(|m|max) / c on g, the
    weights' tolerance carried into g, and two roundings of the blend."""
    c = 1 - t + EPS
    mmax = float(max(np.abs(inp["mx"]).max(), np.abs(inp["my"]).max()))
    gmax = float(max(np.abs(ref["gx"]).max(), np.abs(ref["gy"]).max()))
    vmax = float(max(np.abs(ref["vx"]).max(), np.abs(ref["vy"]).max()))
    return gamma * (K_GEMM * np.sqrt(N) * 2.0 ** -23 * mmax / c + tw * gmax) + 2.0 ** -22 * vmax


def reference_of(inp, t, gamma):
    """float64 answer of guidance64 as a dict, g recovered from the blend's inputs (gamma > 0)."""
    vx, vy, w, l = guidance64(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], inp["r"], t, gamma)
    gx = (vx - (1 - gamma) * inp["vx"].astype(np.float64)) / gamma
    gy = (vy - (1 - gamma) * inp["vy"].astype(np.float64)) / gamma
    ref = {"vx": vx, "vy": vy, "w": w, "l": l, "gx": gx, "gy": gy}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _copy(inp):
    return {k: v.copy() for k, v in inp.items()}


def _top_two_gap(l):
    s = np.sort(l, axis=1)
    return s[:, -1] - s[:, -2]


@functools.lru_cache(maxsize=None)
def ratio_edge(si, k, value):
    """CASES[0] at STEPS[si], centre 0, with mc_ratios[k] = value: (inputs, float64 reference)."""
    inp = _copy(case(0, si, 0.0)[0])
    inp["r"][k] = value
    return inp, reference_of(inp, *STEPS[si])


@functools.lru_cache(maxsize=None)
def shifted_row():
    """CASES[0] at t = 0.99, centre 0, one row of (x, y) moved by +3 per element: its l ~ -9 D / (2 sigma^2) = -6e7
    with a spread of ~ 3 / sigma = 270 between samples, so exp(l - max) of every sample but the nearest underflows or
    nearly so.  The row is the one whose float64 top-two gap in l is largest.  (inputs, reference, row, gap)."""
    si = 3
    base = case(0, si, 0.0)[0]
    every = _copy(base)
    every["x"] += 3.0
    every["y"] += 3.0
    gaps = _top_two_gap(reference_of(every, *STEPS[si])["l"])
    row = int(np.argmax(gaps))
    inp = _copy(base)
    inp["x"][row] += 3.0
    inp["y"][row] += 3.0
    ref = reference_of(inp, *STEPS[si])
    return inp, ref, row, float(_top_two_gap(ref["l"])[row])


@functools.lru_cache(maxsize=None)
def case(ci, si, centre):
    """(inputs, float64 reference) of CASES[ci] at STEPS[si]: built once per process and shared, read-only."""
    B, N, dx, dy = CASES[ci]
    t, gamma = STEPS[si]
    inp = spread_case(B, N, dx, dy, t, seed_of(ci, si, centre), centre)
    for a in inp.values():
        a.setflags(write=False)
    return inp, reference_of(inp, t, gamma)
