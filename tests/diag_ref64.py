"""float64 numpy restatement of the guidance diagnostics (include/rgfm.h, RGFM_DIAG_*): the yardstick of
tests/test_diag_cpu.py and tests/test_gpu_diag.py.

Nothing of the guidance block is restated: the weights w and log-densities l come from guidance_ref64.guidance64 (the
paired block) and cond_ref64.cond64 (the one-sided block); z_bar and g are the reference's own statements
(src/utils/flow_utils.py:305-306, :315, :340-341) over them, and the record is

    ess = (sum_i w_i)^2 / sum_i w_i^2,  w_max,  w_min,  z_bar,  |v_x|, |v_y|,  |g_x|, |g_y|      per row.

paired() / one_sided(): the spread cases of guidance_ref64 / cond_ref64 keep ess near N.  The same cases with the ratios replaced
by r_i = exp(s z_i), z ~ N(0, 1) seeded, s in GRADES, run ess from about N down to about 1 (test_diag_cpu.py asserts
the span).  The grading goes through the ratios, not the distances: distances that put |l| in the thousands lose the
weights to the fp32 rounding of l in the reference too.
"""
import functools

import numpy as np

import cond_ref64 as C
import guidance_ref64 as G

FIELDS = ("ess", "w_max", "w_min", "z_bar", "v_norm_x", "v_norm_y", "g_norm_x", "g_norm_y")
GRADES = (0.0, 2.0, 6.0)  # 0: the case's own ratios exp(0.5 N(0, 1))
U24 = 2.0 ** -24
FLT_MIN = 2.0 ** -126


def stats64(w):
    """(ess, w_max, w_min) of the rows of w [B, N]."""
    w = np.asarray(w, np.float64)
    return w.sum(1) ** 2 / (w ** 2).sum(1), w.max(1), w.min(1)


def _norm(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).sum(1))


def _record(w, zbar, vx, vy, gx, gy):
    rec = np.zeros((w.shape[0], len(FIELDS)))
    rec[:, 0], rec[:, 1], rec[:, 2] = stats64(w)
    rec[:, 3] = zbar
    rec[:, 4], rec[:, 6] = _norm(vx), _norm(gx)
    if vy is not None and vy.shape[1]:
        rec[:, 5], rec[:, 7] = _norm(vy), _norm(gy)
    return rec


def diag64(inp, t):
    """The paired block's records at time t for inp = {x, y, vx, vy, mx, my, r} (guidance_ref64.spread_case's layout):
    {"rec" [B, 8], "w", "gx", "gy", "vx", "vy"} in float64; "vx" / "vy" are the blend at gamma = 1, i.e. g, the names
    guidance_ref64.velocity_bound reads."""
    gx, gy, w, l = G.guidance64(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], inp["r"], t, 1.0)
    p = np.exp(l - l.max(1, keepdims=True))                                                # reference :305-306
    zbar = (np.asarray(inp["r"], np.float64)[None] * p).mean(1) + 1e-10                    # reference :315
    B = w.shape[0]
    vx, vy = (np.asarray(inp[k], np.float64).reshape(B, -1) for k in ("vx", "vy"))
    return {"rec": _record(w, zbar, vx, vy, gx, gy), "w": w, "gx": gx, "gy": gy, "vx": gx, "vy": gy}


def diag_cond64(inp, t):
    """The one-sided block's records for inp = {s, v, m, R} (cond_ref64.spread_case's layout); the _y entries 0."""
    _, w, l, g = C.cond64(inp["s"], inp["v"], inp["m"], inp["R"], t, 1.0)
    p = np.exp(l - l.max(1, keepdims=True))
    zbar = (np.asarray(inp["R"], np.float64) * p).mean(1) + 1e-10
    B = w.shape[0]
    v = np.asarray(inp["v"], np.float64).reshape(B, -1)
    zero = np.zeros((B, 1))  # (a modality that is not there: what velocity_bound's maxima read)
    return {"rec": _record(w, zbar, v, None, g, None), "w": w, "gx": g, "gy": zero, "vx": g, "vy": zero}


def grade_ratios(shape, s, seed):
    """fp32 ratios exp(s z), z ~ N(0, 1)."""
    z = np.random.default_rng(seed).standard_normal(shape)
    return np.ascontiguousarray(np.exp(s * z), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def paired(ci, si, centre, s):
    """(inputs, diag64 of them) of guidance_ref64.CASES[ci] at STEPS[si] with ratios of grade s; shared, read-only."""
    inp = dict(G.case(ci, si, centre)[0])
    if s:
        inp["r"] = grade_ratios(inp["r"].shape, s, 9000 + G.seed_of(ci, si, centre) + int(s))
        inp["r"].setflags(write=False)
    ref = diag64(inp, G.STEPS[si][0])
    for a in ref.values():
        a.setflags(write=False)
    return inp, ref


@functools.lru_cache(maxsize=None)
def one_sided(ci, si, centre, s):
    inp = dict(C.case(ci, si, centre)[0])
    if s:
        inp["R"] = grade_ratios(inp["R"].shape, s, 9500 + C.seed_of(ci, si, centre) + int(s))
        inp["R"].setflags(write=False)
    ref = diag_cond64(inp, C.STEPS[si][0])
    for a in ref.values():
        a.setflags(write=False)
    return inp, ref


def bounds(inp_m, ref, N, dims, t, tw, v_extra=(0.0, 0.0)):
    """Per-field (kind, bound [B]) against float64, kind 'rel' or 'abs'.  tw: the relative weight tolerance
    guidance_ref64.tol_w(t, centre).  inp_m: {"mx", "my"} (what velocity_bound reads of the inputs); dims: (dx, dy).

      w_max, w_min, z_bar   relative tw (as tests/test_gpu_guidance.py holds the weights); a weight below fp32's smallest
                            normal number 2^-126 (rows that are one-hot to 1e-100 in float64: the loops' own inputs) has
                            no fp32 digits to be relative to -- there the bound is 2^-126 absolute
      ess                   relative 4 tw + 2 N 2^-24: a relative tw on every weight through (sum w)^2 / sum w^2 to first
                            order, plus the worst case of two fp32 sums of N terms
      v_norm_*              relative D 2^-24 (one fp32 sum of D squares; the square root halves it, the bound keeps the
                            whole) + v_extra absolute (loop level: the net's own tolerance)
      g_norm_*              absolute sqrt(D) velocity_bound(gamma = 1) + D 2^-24 |g64|: the per-element bound through the
                            triangle inequality
    """
    rec = ref["rec"]
    B = rec.shape[0]
    one = np.ones(B)
    out = {"ess": ("rel", (4 * tw + 2 * N * U24) * one), "w_max": ("rel", tw * one), "w_min": ("rel", tw * one),
           "z_bar": ("rel", tw * one)}
    vb = G.velocity_bound(inp_m, ref, N, t, 1.0, tw)
    for k, (D, xe) in enumerate(zip(dims, v_extra)):
        sfx = "xy"[k]
        out[f"v_norm_{sfx}"] = ("abs", D * U24 * rec[:, 4 + k] + xe)
        out[f"g_norm_{sfx}"] = ("abs", np.sqrt(D) * vb + D * U24 * rec[:, 6 + k])
    return out


def check(got, ref, bnd, what, fields=FIELDS):
    """Asserts got [B, 8] against ref["rec"] field by field; prints each field's worst ratio error / bound first."""
    rec = ref["rec"]
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    worst = {}
    for k, name in enumerate(FIELDS):
        if name not in fields:
            continue
        if name not in bnd:  # (a modality that is not there: exact zeros)
            assert not got[:, k].any() and not rec[:, k].any(), (what, name)
            continue
        kind, b = bnd[name]
        err = np.abs(got[:, k] - rec[:, k])
        lim = np.maximum(b * np.abs(rec[:, k]), FLT_MIN if name in ("w_max", "w_min") else 0.0) if kind == "rel" else b
        worst[name] = float((err / np.maximum(lim, 1e-300)).max())
    print(f"{what}: " + "  ".join(f"{n} {v:.2f}" for n, v in worst.items()))
    bad = {n: v for n, v in worst.items() if not v <= 1.0}
    assert not bad, (what, bad)
