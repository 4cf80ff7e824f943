"""float64 numpy restatement of the effective-sample-size floor of the MC importance weights (include/rgfm.h,
"Effective-sample-size floor"): the yardstick of tests/test_ess_cpu.py and tests/test_gpu_ess.py.

The rule, for one row with log-density terms l [N], ratios r [N] and a floor ess_min (1 <= ess_min <= N):

    w      the weights of the block without a floor (guidance_ref64.guidance64 / cond_ref64.cond64: the reference's
           statements with their epsilons), ESS_1 = (sum w)^2 / sum w^2
    P      {i : r_i > 0}, n_pos = |P|; samples outside P are masked and have weight exactly 0 for every tau
    E*     min(ess_min, n_pos); n_pos = 0: the all-zero row w, tau = 1
    ESS_1 >= E* (or E* <= 1, which every row meets):  w is kept as it is, tau = 1 (the tempered formula is not
                  evaluated at tau = 1)
    otherwise     L_i = l_i + log r_i, d_i = L_i - max_P L, ESS(tau) = (sum_P e^{tau d})^2 / sum_P e^{2 tau d};
                  bisection from lo = 0, hi = 1: BISECT times mid = 0.5 (lo + hi), lo = mid if ESS(mid) >= E* else
                  hi = mid; tau = lo, w_i = e^{tau d_i} / sum_P e^{tau d_j}

BISECT = 40 is the device's count.  The device's tau is an fp32 number, so its bisection stops moving after about 24
halvings below the leading bit of tau; in float64 40 steps leave |hi - lo| = 2^-40, and with |d ESS / d tau| <= 2 N max|d|
that is far from the 1e-9 the CPU test asks of the achieved ESS at late t (|d| ~ 1e4).  `temper_row(..., iters=)` takes
more steps for that test; the GPU tests compare against the default.

The blocks and loops below are COMPOSED from the pinned float64 pieces: guidance64 / cond64 give l and the untempered
w, the guided velocity is g = sum_i w_i (m_i - x) / (1 - t + 1e-3), blended as (1 - gamma) v + gamma g; the F_* builders
are ode_ref64's with the tempered block in the plain one's place, for ode_ref64.integrate64 / sde_ref64.integrate_sde64.
"""
import numpy as np

import cond_ref64 as C
import guidance_ref64 as G

EPS = G.EPS
BISECT = 40


def ess_of(w):
    """(sum w)^2 / sum w^2 along the last axis in float64; 0 for an all-zero row."""
    w = np.asarray(w, np.float64)
    s, q = w.sum(-1), (w * w).sum(-1)
    return np.where(q > 0, s * s / np.where(q > 0, q, 1.0), 0.0)


def ess_tau(d, tau):
    """ESS(tau) of the row with d = L - max L over its unmasked samples (d <= 0, one entry 0)."""
    e = np.exp(tau * d)
    return e.sum() ** 2 / (e * e).sum()


def temper_row(l, r, w, ess_min, iters=BISECT):
    """(w' [N], tau) of one row: l, r, w [N] float64 (w: the row's weights without a floor)."""
    l, r, w = (np.asarray(a, np.float64) for a in (l, r, w))
    pos = r > 0
    n_pos = int(pos.sum())
    target = min(float(ess_min), float(n_pos))
    if n_pos == 0 or target <= 1.0 or ess_of(w) >= target:  # (E* <= 1: met by every row)
        return w.copy(), 1.0
    L = l[pos] + np.log(r[pos])
    d = L - L.max()
    lo, hi = 0.0, 1.0
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if ess_tau(d, mid) >= target:
            lo = mid
        else:
            hi = mid
    e = np.exp(lo * d)
    out = np.zeros_like(w)  # (masked samples: exactly 0)
    out[pos] = e / e.sum()
    return out, lo


def temper(l, r, w, ess_min, iters=BISECT):
    """(w' [B, N], tau [B]); r [N] (shared) or [B, N] (a row per sample)."""
    l, w = np.asarray(l, np.float64), np.asarray(w, np.float64)
    r = np.broadcast_to(np.asarray(r, np.float64), l.shape)
    out, tau = np.empty_like(w), np.empty(l.shape[0])
    for b in range(l.shape[0]):
        out[b], tau[b] = temper_row(l[b], r[b], w[b], ess_min, iters)
    return out, tau


def target_of(r, shape, ess_min):
    """E* [B] = min(ess_min, n_pos)."""
    r = np.broadcast_to(np.asarray(r, np.float64), shape)
    return np.minimum(float(ess_min), (r > 0).sum(-1).astype(np.float64))


def _col(gamma):
    g = np.asarray(gamma, np.float64)
    return g[:, None] if g.ndim else float(g)


def guidance_ess64(x, y, vx, vy, mx, my, r, t, gamma, ess_min):
    """The paired block held to the floor: (vx', vy', w, tau); gamma a double or a vector [B]."""
    x, y, vx, vy, mx, my, r = (np.asarray(a, np.float64) for a in (x, y, vx, vy, mx, my, r))
    x, y, vx, vy, mx, my = (a.reshape(a.shape[0], -1) for a in (x, y, vx, vy, mx, my))
    _, _, w0, l = G.guidance64(x, y, vx, vy, mx, my, r, t, 1.0)
    w, tau = temper(l, r, w0, ess_min)
    c = 1 - float(t) + EPS
    gx, gy = np.empty_like(x), np.empty_like(y)
    for b in range(x.shape[0]):
        gx[b] = (w[b][:, None] * ((mx - x[b]) / c)).sum(0)
        gy[b] = (w[b][:, None] * ((my - y[b]) / c)).sum(0)
    g = _col(gamma)
    return (1 - g) * vx + g * gx, (1 - g) * vy + g * gy, w, tau


def cond_ess64(s, v, m, R, t, gamma, ess_min):
    """The one-sided block held to the floor: (v', w, tau)."""
    s, v, m, R = (np.asarray(a, np.float64) for a in (s, v, m, R))
    s, v, m = (a.reshape(a.shape[0], -1) for a in (s, v, m))
    _, w0, l, _ = C.cond64(s, v, m, R, t, 1.0)
    w, tau = temper(l, R, w0, ess_min)
    c = 1 - float(t) + EPS
    gd = np.empty_like(s)
    for b in range(s.shape[0]):
        gd[b] = (w[b][:, None] * ((m - s[b]) / c)).sum(0)
    g = _col(gamma)
    return (1 - g) * v + g * gd, w, tau


def F_pair_ess(velx, vely, mx, my, r, gamma_of, ess_min, guide, taus=None):
    """ode_ref64.F_pair_mc with the tempered block.  gamma_of(t): the stage's strength (a double or [B]); guide(t): is
    the stage guided; taus: a list that receives (t, tau [B]) per guided evaluation."""
    def F(s, t):
        x, y = s
        vx, vy = np.asarray(velx(x, t), np.float64), np.asarray(vely(y, t), np.float64)
        if guide(t):
            B = x.shape[0]
            gx, gy, _, tau = guidance_ess64(x, y, vx, vy, mx, my, r, t, gamma_of(t), ess_min)
            vx, vy = gx.reshape(x.shape), gy.reshape(y.shape)
            if taus is not None:
                taus.append((t, tau))
        return vx, vy
    return F


def F_cond_ess(vel, m, R, gamma_of, ess_min, guide, taus=None):
    def F(s, t):
        v = np.asarray(vel(s[0], t), np.float64)
        if guide(t):
            shape = s[0].shape
            out, _, tau = cond_ess64(s[0], v, m, R, t, gamma_of(t), ess_min)
            v = out.reshape(shape)
            if taus is not None:
                taus.append((t, tau))
        return (v,)
    return F


# ------------------------------------------------------------------ the rule once more in fp32 (the tolerance's source)
def logl32(x, m, t):
    """One modality's log-density term as the device forms it: mu = t m and the differences in fp32, the sum of squares
    wide, then -0.5 S / sigma_t^2 rounded to fp32 operation by operation.  x [B, d], m [N, d] fp32 -> [B, N] fp32."""
    f = np.float32
    tf, s2 = f(t), f((1 - float(t) + EPS) ** 2)
    mu = (tf * m.astype(f)).astype(f)
    out = np.empty((x.shape[0], m.shape[0]), f)
    for b in range(x.shape[0]):
        d = (x[b].astype(f)[None] - mu).astype(f)
        S = (d.astype(np.float64) ** 2).sum(-1).astype(f)
        out[b] = ((f(-0.5) * S).astype(f) / s2).astype(f)
    return out


def temper_row32(l, r, ess_min, iters=BISECT):
    """(w [N], tau) of one row with every operation of the rule rounded to fp32 (sequential sums): what an fp32
    implementation may differ from float64 by.  l, r fp32."""
    f = np.float32
    l, r = l.astype(f), r.astype(f)
    N = l.size
    p = np.exp((l - l.max()).astype(f)).astype(f)
    pbar = f(f(p.sum(dtype=f) / f(N)) + f(1e-10))
    zbar = f(f((r * p).astype(f).sum(dtype=f) / f(N)) + f(1e-10))
    w = ((r / zbar).astype(f) * (p / pbar).astype(f)).astype(f)
    w = (w / f(w.sum(dtype=f) + f(1e-10))).astype(f)
    pos = r > 0
    target = f(min(float(ess_min), float(pos.sum())))
    s, q = w.sum(dtype=f), (w * w).astype(f).sum(dtype=f)
    ess1 = f(s * s / q) if q > 0 else f(0)
    if not pos.any() or target <= 1 or ess1 >= target:
        return w, f(1)
    L = (l[pos] + np.log(r[pos]).astype(f)).astype(f)
    d = (L - L.max()).astype(f)
    lo, hi = f(0), f(1)
    for _ in range(iters):
        mid = f(f(0.5) * f(lo + hi))
        e = np.exp((mid * d).astype(f)).astype(f)
        s1, s2 = e.sum(dtype=f), (e * e).astype(f).sum(dtype=f)
        if f(s1 * s1) / s2 >= target:
            lo = mid
        else:
            hi = mid
    e = np.exp((lo * d).astype(f)).astype(f)
    out = np.zeros(N, f)
    out[pos] = (e / e.sum(dtype=f)).astype(f)
    return out, lo


# ------------------------------------------------------------------ inputs of the block tests (tests/test_gpu_ess.py)
DX, DY = 8, 4  # the smallest flattened sizes of the existing block tests (guidance_ref64.CASES[7])


def floor_of(N):
    """The floor the block tests ask for at N samples: 4, or what N leaves room for."""
    return {1: 1.0, 2: 1.5}.get(N, 4.0)


def cluster_case(B, N, t, seed, far_rows=(), spread=0.5, far=200.0):
    """guidance_ref64.spread_case with a knob per kind of row: {x, y, vx, vy, mx, my, r, R} fp32, R [B, N] the ratio
    rows of the one-sided block (whose state, velocity and MC set are x, vx, mx).  The MC set is a cluster of width
    spread * sigma / (t sqrt D) around a centre; a row amid it sees every sample at about the same distance (ESS_1
    about 0.95 N at spread 0.5; larger spreads collapse it); a row of `far_rows` sits far * sigma away from the cluster
    in a direction of its own, where the samples' log-weights differ by tens: ESS_1 is 1 to a few percent."""
    g = np.random.default_rng(seed)
    D = DX + DY
    sigma = 1 - t + EPS
    c0 = g.standard_normal(D)
    u = g.standard_normal((N, D))
    n = g.standard_normal((B, D))
    e = g.standard_normal((B, D))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    m = c0 + spread * (sigma / (t * np.sqrt(D))) * u
    x = t * c0 + 0.5 * spread * (sigma / np.sqrt(D)) * n
    for b in far_rows:
        x[b] += far * sigma * e[b]
    r = np.exp(0.2 * g.standard_normal(N))
    R = np.exp(0.2 * g.standard_normal((B, N)))
    v = g.standard_normal((B, D))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"x": f(x[:, :DX]), "y": f(x[:, DX:]), "vx": f(v[:, :DX]), "vy": f(v[:, DX:]), "mx": f(m[:, :DX]), "my": f(m[:, DX:]),
            "r": f(r), "R": f(R)}


def late_case(B, N, seed, t=0.99):
    """Rows placed ON an MC sample of a wide MC set (0.5 N(0, 1) images) at late t: the neighbours' log-weights are 1e4
    to 1e5 below the row's own sample, ESS_1 = 1, and a floor needs tau of the order of 1e-4."""
    g = np.random.default_rng(seed)
    D = DX + DY
    m = 0.5 * g.standard_normal((N, D))
    k = g.integers(0, N, B)
    x = t * m[k] + 1e-4 * g.standard_normal((B, D))
    r = np.exp(0.2 * g.standard_normal(N))
    R = np.exp(0.2 * g.standard_normal((B, N)))
    v = g.standard_normal((B, D))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"x": f(x[:, :DX]), "y": f(x[:, DX:]), "vx": f(v[:, :DX]), "vy": f(v[:, DX:]), "mx": f(m[:, :DX]), "my": f(m[:, DX:]),
            "r": f(r), "R": f(R)}


def moderate_case(B, N, t, seed):
    """cluster_case at the first spread of 3, 3.5, ... at which every row's ESS_1 (paired and one-sided, float64) is in
    [1, 4]: the moderately collapsed regime of the weights comparison."""
    for k in range(40):
        inp = cluster_case(B, N, t, seed, spread=3.0 + 0.5 * k)
        top = max(float(ess_of(pair64(inp, t, 0.5, None)["w0"]).max()), float(ess_of(cond64(inp, t, 0.5, None)["w0"]).max()))
        if top <= 4.0:
            return inp
    raise AssertionError("no spread collapses this case")


def pair64(inp, t, gamma, ess_min):
    """float64 answer of the paired block: {vx, vy, w, tau, w0, l} (ess_min None: the block without a floor, tau 1)."""
    a = {k: np.asarray(v, np.float64) for k, v in inp.items()}
    gx, gy, w0, l = G.guidance64(a["x"], a["y"], a["vx"], a["vy"], a["mx"], a["my"], a["r"], t, 1.0)  # (gamma 1: g itself)
    if ess_min is None:
        g = _col(gamma)
        return {"vx": (1 - g) * a["vx"] + g * gx, "vy": (1 - g) * a["vy"] + g * gy, "w": w0, "tau": np.ones(w0.shape[0]), "w0": w0,
                "l": l}
    vx, vy, w, tau = guidance_ess64(a["x"], a["y"], a["vx"], a["vy"], a["mx"], a["my"], a["r"], t, gamma, ess_min)
    return {"vx": vx, "vy": vy, "w": w, "tau": tau, "w0": w0, "l": l}


def cond64(inp, t, gamma, ess_min):
    """float64 answer of the one-sided block on (x, vx, mx, R): {v, w, tau, w0, l}."""
    a = {k: np.asarray(v, np.float64) for k, v in inp.items()}
    _, w0, l, g0 = C.cond64(a["x"], a["vx"], a["mx"], a["R"], t, 1.0)
    if ess_min is None:
        g = _col(gamma)
        return {"v": (1 - g) * a["vx"] + g * g0, "w": w0, "tau": np.ones(w0.shape[0]), "w0": w0, "l": l}
    v, w, tau = cond_ess64(a["x"], a["vx"], a["mx"], a["R"], t, gamma, ess_min)
    return {"v": v, "w": w, "tau": tau, "w0": w0, "l": l}


def oracle32(inp, t, ess_min, one_sided=False):
    """(w [B, N], tau [B]) of the fp32 restatement on the case's inputs."""
    l = logl32(inp["x"], inp["mx"], t)
    if not one_sided:
        l = (l + logl32(inp["y"], inp["my"], t)).astype(np.float32)
    B, N = l.shape
    R = inp["R"] if one_sided else np.broadcast_to(inp["r"], (B, N))
    rows = [temper_row32(l[b], R[b], ess_min) for b in range(B)]
    return np.stack([a[0] for a in rows]), np.array([a[1] for a in rows])


# ------------------------------------------------------------------ the tolerance of the tempered weights
# The untempered weights' tolerance (guidance_ref64.tol_w: relative error per element <= 4x the fp32 oracle's own) does
# not carry over to a tempered row as it stands: w_i ~ e^{tau d_i}, so an error of tau enters element i multiplied by
# |tau d_i| -- up to 30 at N = 63, 120 at N = 1024 in the moderate cases -- and elements below the fp32 range
# (e^{-88}) are flushed.  The fp32 restatement above (oracle32) shows it: its tau is within ORACLE_DTAU of float64's
# relatively (max over the moderate cases N in {2, 63, 64, 65, 256, 1024}, B in {1, 5, 33}, paired and one-sided,
# rounded up to two digits), and its weights miss guidance_ref64.tol_w on the small elements by up to 4x.  So:
#   tau:      |tau / tau64 - 1| <= tol_tau(t) = 4 ORACLE_DTAU[t]    (4x as guidance_ref64.tol_w: another expf, wave-order sums)
#   weights:  |w_i / w64_i - 1| <= tol_w(t, centre = 1) + |tau64 d64_i| tol_tau(t)   where w64_i >= W_FLOOR,
#             |w_i - w64_i| <= W_FLOOR                                              below it
# -- the existing tolerance plus what the exponent's own tolerance does to element i.
ORACLE_DTAU = {0.5: 5.4e-7, 0.9: 1.1e-6}
W_FLOOR = 2.0 ** -100


def tol_tau(t):
    return 4.0 * ORACLE_DTAU[t]


def weights_check(w, tau, ref, t, tempered_only=True):
    """Worst ratio (error / tolerance) of the weights and of tau over the rows with tau64 < 1; > 1 fails."""
    w = np.asarray(w, np.float64)
    worst_w = worst_t = 0.0
    for b in np.nonzero(ref["tau"] < 1)[0]:
        w64, t64 = ref["w"][b], ref["tau"][b]
        big = w64 >= W_FLOOR
        d = np.log(np.where(big, w64, 1.0))  # tau d_i - log sum: |tau d_i| <= |log w64_i| + log N
        tol = G.tol_w(t, 1.0) + (np.abs(d) + np.log(w64.size)) * tol_tau(t)
        worst_w = max(worst_w, float((np.abs(w[b] / np.where(big, w64, 1.0) - 1)[big] / tol[big]).max()))
        if (~big).any():
            worst_w = max(worst_w, float(np.abs(w[b] - w64)[~big].max() / W_FLOOR))
        worst_t = max(worst_t, abs(float(tau[b]) / t64 - 1) / tol_tau(t))
    return worst_w, worst_t
