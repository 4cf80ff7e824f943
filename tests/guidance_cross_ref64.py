"""float64 numpy yardstick of the MC guidance block under cross pairing (all N x N pairs (x1_i, y1_j) of the MC set,
R_ij = r(x1_i, y1_j)): what tests/test_guidance_cross_cpu.py and tests/test_gpu_guidance_cross.py compare against.

Cross pairing is the reference block (src/utils/flow_utils.py:273-369, src/sample_mnist_svhn.py:124-171) on the MC list
of N^2 pairs.  The Gaussian factor of pair (i, j) splits into a_i b_j, so cross64 states it through the weights'
marginals, in float64 throughout, with sigma = 1 - t + 1e-3:

    lx_i = -0.5 |x - t x1_i|^2 / sigma^2,  ly_j likewise;   a_i = exp(lx_i - max lx),  b_j = exp(ly_j - max ly)
    u = R b,  s = R^T a
    p_bar = (sum a)(sum b) / N^2 + 1e-10          Z_bar = a^T R b / N^2 + 1e-10
    w_ij  = (R_ij / Z_bar)(a_i b_j / p_bar), normalised by (sum_ij w_ij + 1e-10)
    wx_i  = sum_j w_ij ~ a_i u_i                  wy_j  = sum_i w_ij ~ b_j s_j
    g_x   = sum_i wx_i (x1_i - x) / (1 - t + 1e-3),  g_y likewise;   v = (1 - gamma) v + gamma g
    joint ESS = (sum_ij w_ij)^2 / sum_ij w_ij^2 = (a^T R b)^2 / ((a^2)^T (R o R) (b^2))

tests/test_guidance_cross_cpu.py pins this to guidance_ref64.guidance64 run on the materialised list (mx repeated, my
tiled, r = R.reshape(-1)) to 1e-12.

Inputs: guidance_ref64.spread_case plus R = exp(0.5 N(0, 1)) [N, N] from the case's seed -- asymmetric, so a
transposed read of R is far outside every tolerance.  STEPS, CENTRES and velocity_bound are guidance_ref64's.

cross32 is a plain sequential fp32 restatement (every sum a running fp32 sum in index order).  The weights tolerance of
the GPU test is 4x its largest relative deviation from cross64 over CASES, per (t, centre): the rule and the reason of
guidance_ref64.ORACLE_DW (another expf, wave-order instead of sequential sums).  CROSS32_DW holds the measured figures
rounded up to two digits; test_guidance_cross_cpu.py reproduces them.  Nothing here comes from the HIP result.
"""
import functools

import numpy as np

import guidance_ref64 as G

EPS = G.EPS
STEPS, CENTRES, velocity_bound = G.STEPS, G.CENTRES, G.velocity_bound

# (B, N, dx, dy)
CASES = [
    (1, 1, 4, 4),        # smallest possible shape
    (5, 8, 64, 192),
    (33, 33, 68, 4),     # ragged B and N, dy of one float4
    (65, 32, 64, 192),
    (2, 64, 520, 48),    # N^2 = 4096, the largest the paired block takes
    (3, 257, 8, 4),      # one past a 256 tile
    (2, 1024, 8, 4),     # the maximum N, with a 4 MB R
]

# max over CASES of max(|wx32 - wx64| / wx64, |wy32 - wy64| / wy64), cross32 against cross64, per (t, centre): measured
# by test_guidance_cross_cpu.py (its docstring has the table), rounded up to two digits
CROSS32_DW = {
    (0.05, 1.0): 2.4e-6, (0.5, 1.0): 2.4e-6, (0.9, 1.0): 3.1e-6, (0.99, 1.0): 9.6e-6,
    (0.05, 0.0): 2.6e-6, (0.5, 0.0): 2.3e-6, (0.9, 0.0): 2.1e-6, (0.99, 0.0): 2.0e-6,
}


def tol_w_cross(t, centre):
    return 4.0 * CROSS32_DW[(t, centre)]


def _flat64(*arrays):
    return tuple(np.asarray(a, np.float64).reshape(a.shape[0], -1) for a in arrays)


def cross64(x, y, vx, vy, mx, my, R, t, gamma):
    """(vx', vy', wx [B, N], wy [B, N], ess [B], z_bar [B]) in float64; x, y, v [B, d], m [N, d], R [N, N]."""
    x, y, vx, vy, mx, my = _flat64(x, y, vx, vy, mx, my)
    R = np.asarray(R, np.float64)
    B, N = x.shape[0], mx.shape[0]
    assert R.shape == (N, N), R.shape
    t, gamma = float(t), float(gamma)
    sigma_t = 1 - t + EPS
    s2 = sigma_t ** 2
    c = 1 - t + EPS
    lx, ly = np.empty((B, N)), np.empty((B, N))
    for k in range(B):
        lx[k] = -0.5 * ((x[k] - t * mx) ** 2).sum(-1) / s2
        ly[k] = -0.5 * ((y[k] - t * my) ** 2).sum(-1) / s2
    a = np.exp(lx - lx.max(1, keepdims=True))
    b = np.exp(ly - ly.max(1, keepdims=True))
    u = b @ R.T                                    # u_i = sum_j R_ij b_j
    s = a @ R                                      # s_j = sum_i R_ij a_i
    e = (a * u).sum(1, keepdims=True)              # a^T R b
    p_bar = a.sum(1, keepdims=True) * b.sum(1, keepdims=True) / N ** 2 + 1e-10
    z_bar = e / N ** 2 + 1e-10
    scale = 1.0 / (z_bar * p_bar)
    total = e * scale + 1e-10                      # sum_ij w_ij before the normalisation, + its epsilon
    wx = a * u * scale / total
    wy = b * s * scale / total
    q = ((a * a) * ((b * b) @ (R * R).T)).sum(1)   # (a^2)^T (R o R) (b^2)
    ess = e[:, 0] ** 2 / q
    gx, gy = np.empty_like(x), np.empty_like(y)
    for k in range(B):
        gx[k] = (wx[k][:, None] * ((mx - x[k]) / c)).sum(0)
        gy[k] = (wy[k][:, None] * ((my - y[k]) / c)).sum(0)
    return (1 - gamma) * vx + gamma * gx, (1 - gamma) * vy + gamma * gy, wx, wy, ess, z_bar[:, 0]


def _seq(a):
    """Sequential fp32 sum over the last axis."""
    return np.cumsum(a, axis=-1, dtype=np.float32)[..., -1]


def cross32(x, y, vx, vy, mx, my, R, t, gamma):
    """cross64's statements in fp32, every sum sequential; the step's scalars rounded to fp32 where a tensor op takes them."""
    f = np.float32
    x, y, vx, vy, mx, my = (np.asarray(a, f).reshape(a.shape[0], -1) for a in (x, y, vx, vy, mx, my))
    R = np.asarray(R, f)
    B, N = x.shape[0], mx.shape[0]
    sigma_t = 1 - float(t) + EPS
    tf, s2, c = f(t), f(sigma_t ** 2), f(1 - float(t) + EPS)
    g1, g2 = f(1 - float(gamma)), f(gamma)

    def logp(z, m):
        mu = tf * m
        out = np.empty((B, N), f)
        for k in range(B):
            d = z[k] - mu
            out[k] = f(-0.5) * _seq(d * d) / s2
        return out
    lx, ly = logp(x, mx), logp(y, my)
    a = np.exp(lx - lx.max(1, keepdims=True))
    b = np.exp(ly - ly.max(1, keepdims=True))
    u = _seq(R[None] * b[:, None, :])
    s = _seq(R.T[None] * a[:, None, :])
    e = _seq(a * u)[:, None]
    nn = f(N) * f(N)
    p_bar = _seq(a)[:, None] * _seq(b)[:, None] / nn + f(1e-10)
    z_bar = e / nn + f(1e-10)
    wx = (u / z_bar) * (a / p_bar)
    wy = (s / z_bar) * (b / p_bar)
    wx = wx / (_seq(wx)[:, None] + f(1e-10))
    wy = wy / (_seq(wy)[:, None] + f(1e-10))
    q = _seq((a * a) * _seq((R * R)[None] * (b * b)[:, None, :]))
    ess = e[:, 0] ** 2 / q
    gx, gy = np.empty_like(x), np.empty_like(y)
    for k in range(B):
        gx[k] = _seq((wx[k][:, None] * ((mx - x[k]) / c)).T)
        gy[k] = _seq((wy[k][:, None] * ((my - y[k]) / c)).T)
    out = (g1 * vx + g2 * gx, g1 * vy + g2 * gy, wx, wy, ess, z_bar[:, 0])
    assert all(o.dtype == f for o in out)
    return out


def materialised(inp):
    """The MC list of N^2 pairs the paired block takes: pair i N + j is (mx_i, my_j) with ratio R_ij."""
    N = inp["mx"].shape[0]
    return {**{k: inp[k] for k in ("x", "y", "vx", "vy")}, "mx": np.repeat(inp["mx"], N, axis=0),
            "my": np.tile(inp["my"], (N, 1)), "r": np.ascontiguousarray(inp["R"].reshape(-1))}


def ratio_matrix(N, seed):
    """R = exp(0.5 N(0, 1)) [N, N], fp32."""
    z = np.random.default_rng(7000 + seed).standard_normal((N, N))
    return np.ascontiguousarray(np.exp(0.5 * z), dtype=np.float32)


def cross_case(B, N, dx, dy, t, seed, centre):
    """{x, y, vx, vy, mx, my, R}: guidance_ref64.spread_case's arrays, the ratio vector replaced by the matrix."""
    inp = G.spread_case(B, N, dx, dy, t, seed, centre)
    del inp["r"]
    inp["R"] = ratio_matrix(N, seed)
    return inp


def reference_of(inp, t, gamma):
    """cross64's answer as a dict (the keys guidance_ref64.velocity_bound reads among them), g recovered from the blend."""
    vx, vy, wx, wy, ess, z_bar = cross64(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], inp["R"], t, gamma)
    B = vx.shape[0]
    gx = (vx - (1 - gamma) * inp["vx"].reshape(B, -1).astype(np.float64)) / gamma
    gy = (vy - (1 - gamma) * inp["vy"].reshape(B, -1).astype(np.float64)) / gamma
    ref = {"vx": vx, "vy": vy, "wx": wx, "wy": wy, "ess": ess, "z_bar": z_bar, "gx": gx, "gy": gy}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def diag_of(inp, t):
    """The diagnostics records of a cross call in float64, in diag_ref64's layout: {"rec" [B, 8], "gx", "gy", "vx", "vy"}
    ("vx" / "vy" are g, the names velocity_bound reads).  ess: the joint one; w_max / w_min: over the 2N marginals."""
    ref = reference_of(inp, t, 1.0)
    B = ref["gx"].shape[0]
    norm = lambda v: np.sqrt((np.asarray(v, np.float64).reshape(B, -1) ** 2).sum(1))
    w = np.concatenate([ref["wx"], ref["wy"]], 1)
    rec = np.stack([ref["ess"], w.max(1), w.min(1), ref["z_bar"], norm(inp["vx"]), norm(inp["vy"]), norm(ref["gx"]),
                    norm(ref["gy"])], 1)
    rec.setflags(write=False)
    return {"rec": rec, "wx": ref["wx"], "wy": ref["wy"], "gx": ref["gx"], "gy": ref["gy"], "vx": ref["gx"], "vy": ref["gy"]}


def seed_of(ci, si, centre):
    return 20000 + 100 * ci + 10 * si + int(centre)


def _frozen(inp):
    for v in inp.values():
        v.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def case(ci, si, centre):
    """(inputs, float64 reference) of CASES[ci] at STEPS[si]: built once per process and shared, read-only."""
    t, gamma = STEPS[si]
    inp = _frozen(cross_case(*CASES[ci], t, seed_of(ci, si, centre), centre))
    return inp, reference_of(inp, t, gamma)


def _copy(inp):
    return {k: v.copy() for k, v in inp.items()}


EDGE_CASE = 2  # (33, 33, 68, 4)
SHIFT = 20.0


@functools.lru_cache(maxsize=None)
def ratio_edge(si, kind):
    """CASES[EDGE_CASE] at STEPS[si], centre 0, with R edited: 'zero' -- row 5 and column 9 zero; 'big' -- entry (3, 7)
    1e4 x its value.  (inputs, float64 reference)."""
    inp = _copy(case(EDGE_CASE, si, 0.0)[0])
    if kind == "zero":
        inp["R"][5, :] = 0.0
        inp["R"][:, 9] = 0.0
    else:
        inp["R"][3, 7] *= 1e4
    return _frozen(inp), reference_of(inp, *STEPS[si])


@functools.lru_cache(maxsize=None)
def shifted_row():
    """CASES[EDGE_CASE] at t = 0.99, centre 0, one row of (x, y) moved by +SHIFT per element (guidance_ref64.shifted_row's
    construction, with a shift that takes the top-two gap of lx past 104 = ln 2^150, where fp32's exp is 0): all but
    one a_i of that row underflow.  The row is the one whose float64 top-two gap in lx is largest.
    (inputs, reference, row, gap)."""
    si = 3
    t = STEPS[si][0]
    base = case(EDGE_CASE, si, 0.0)[0]

    def lx_gap(inp):
        x, mx = _flat64(inp["x"], inp["mx"])
        lx = np.stack([-0.5 * ((x[k] - t * mx) ** 2).sum(-1) / (1 - t + EPS) ** 2 for k in range(x.shape[0])])
        srt = np.sort(lx, axis=1)
        return srt[:, -1] - srt[:, -2]
    every = _copy(base)
    every["x"] += SHIFT
    every["y"] += SHIFT
    row = int(np.argmax(lx_gap(every)))
    inp = _copy(base)
    inp["x"][row] += SHIFT
    inp["y"][row] += SHIFT
    return _frozen(inp), reference_of(inp, *STEPS[si]), row, float(lx_gap(inp)[row])
