"""MC guidance over all N x N pairs of the MC set (cross pairing) on the GPU: the cross-weights kernels of
csrc/guidance.hip (guid_cross_ab_kernel, guid_cross_prod_kernel, guid_cross_fin_kernel) with guid_logp_kernel in front
and guid_apply_mfma_kernel behind them, the block-level entry points, the U-Net pair loop and the Python samplers.

The yardstick is tests/guidance_cross_ref64.py: cross64 (float64, pinned on the CPU to guidance_ref64.guidance64 on the
materialised list of N^2 pairs by tests/test_guidance_cross_cpu.py), its cases and the weights tolerance tol_w_cross =
4 x the fp32 restatement's own deviation from float64.  Velocities: guidance_ref64.velocity_bound at that tolerance.
Loops: a float64 loop of unet_ref64.forward64 + cross64 within TOL_SAMPLER = 1e-4, the tolerance of the existing
sampler tests.

Measured on an MI355X (max over the seven cases; dw: relative error of the 2N marginal weights; worst dv / bound):

    t       centre = 1: dw / tol_w      dv / bound     centre = 0: dw / tol_w      dv / bound
    0.05    1.84e-6 / 9.6e-6            0.02           1.94e-6 / 1.0e-5            0.02
    0.5     1.66e-6 / 9.6e-6            0.03           1.91e-6 / 9.2e-6            0.01
    0.9     1.92e-6 / 1.2e-5            0.05           1.81e-6 / 8.4e-6            0.03
    0.99    9.53e-6 / 3.8e-5            0.12           2.00e-6 / 8.0e-6            0.06

(|sum wx - 1|, |sum wy - 1| <= 8.1e-8.)  Diagnostics records, worst error / bound over the 56 block configurations: ess 0.01,
w_max 0.12, w_min 0.14, z_bar 0.16, v_norm 0.37, g_norm 0.02.  Loops (unet28 + rgb32, B 5, N 7, 6 steps) against float64:
gamma 0.7 Euler 3.6e-6, midpoint 3.7e-7; gamma 0 Euler 9.1e-7, midpoint 1.7e-6.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cond_grad_ref64 as CG
import diag_ref64 as D
import guidance_cross_ref64 as X
import ode_ref64 as O
from helpers import make_generic_unet, make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
PAD = 256  # floats kept on each side of an output
TOL_SAMPLER = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to(dev, inp, rows=None):
    """The inputs on the device (fresh tensors; vx / vy are overwritten by the call); rows: a sub-batch."""
    d = {k: torch.tensor(v, device=dev) for k, v in inp.items()}
    if rows is not None:
        for k in ("x", "y", "vx", "vy"):
            d[k] = d[k][rows].clone()
    return d


def _apply(d, t, gamma):
    wx, wy = _engine.guidance_apply_cross(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"], d["R"], t, gamma, True)
    return wx, wy, d["vx"], d["vy"]


def _apply64(dev, inp, t, gamma):
    return tuple(a.cpu().numpy().astype(np.float64) for a in _apply(_to(dev, inp), t, gamma))


def _workspace_bytes(B, N, dx, dy):
    nb = ctypes.c_size_t()
    _lib.check(_lib.lib().rgfm_guidance_cross_workspace_bytes(B, N, dx, dy, ctypes.byref(nb)))
    return nb.value


def _raw(d, t, gamma, wx, wy, ws, ws_bytes):
    """rgfm_guidance_apply_cross with the caller's own weight buffers and workspace."""
    B, N = d["x"].shape[0], d["mx"].shape[0]
    with torch.cuda.device(d["x"].device):
        _lib.check(_lib.lib().rgfm_guidance_apply_cross(_p(d["x"]), _p(d["y"]), _p(d["vx"]), _p(d["vy"]), _p(d["mx"]),
                                                        _p(d["my"]), _p(d["R"]), B, N, d["x"].shape[1], d["y"].shape[1],
                                                        float(t), float(gamma), _p(wx), _p(wy), _p(ws), ws_bytes, _stream()))


def _rel_dw(w, w64):
    keep = w64 > 0
    return float((np.abs(w - w64)[keep] / w64[keep]).max()) if keep.any() else 0.0


def _check_block(got, inp, ref, N, t, gamma, centre, what):
    wx, wy, vx, vy = got
    tw = X.tol_w_cross(t, centre)
    bound = X.velocity_bound(inp, ref, N, t, gamma, tw)
    dw = max(_rel_dw(wx, ref["wx"]), _rel_dw(wy, ref["wy"]))
    dv = max(float(np.abs(vx - ref["vx"]).max()), float(np.abs(vy - ref["vy"]).max()))
    dsum = max(float(np.abs(wx.sum(1) - 1).max()), float(np.abs(wy.sum(1) - 1).max()))
    print(f"cross64 {what} t={t} centre={centre}: dw {dw:.2e} / tol_w {tw:.1e} = {dw / tw:.2f}   "
          f"dv {dv:.2e} / bound {bound:.2e} = {dv / bound:.2f}   |sum w - 1| {dsum:.1e}")
    assert all(np.isfinite(a).all() for a in got)
    assert dw <= tw, (dw, tw)
    assert dsum < 1e-5, dsum
    assert dv <= bound, (dv, bound)


# ------------------------------------------------------------------ 1. the block
@pytest.mark.parametrize("centre", X.CENTRES)
@pytest.mark.parametrize("si", range(len(X.STEPS)))
@pytest.mark.parametrize("ci", range(len(X.CASES)))
def test_marginal_weights_and_velocity_vs_float64(dev, ci, si, centre):
    N = X.CASES[ci][1]
    t, gamma = X.STEPS[si]
    inp, ref = X.case(ci, si, centre)
    _check_block(_apply64(dev, inp, t, gamma), inp, ref, N, t, gamma, centre, str(X.CASES[ci]))


@pytest.mark.parametrize("si", range(len(X.STEPS)))
@pytest.mark.parametrize("ci", [ci for ci, c in enumerate(X.CASES) if c[1] <= 64])
def test_cross_block_vs_the_paired_block_on_the_materialised_list(dev, ci, si):
    """The existing paired block on the N^2 pairs (mx repeated, my tiled, r = R.reshape(-1)) computes the same guided
    velocity: within twice the float64 bound (each side is within one bound of float64)."""
    N = X.CASES[ci][1]
    t, gamma = X.STEPS[si]
    for centre in X.CENTRES:
        inp, ref = X.case(ci, si, centre)
        _, _, vx, vy = _apply(_to(dev, inp), t, gamma)
        m = {k: torch.tensor(v, device=dev) for k, v in X.materialised(inp).items()}
        _engine.guidance_apply(m["x"], m["y"], m["vx"], m["vy"], m["mx"], m["my"], m["r"], t, gamma)
        bound = X.velocity_bound(inp, ref, N, t, gamma, X.tol_w_cross(t, centre))
        dv = max(float((vx - m["vx"]).abs().max()), float((vy - m["vy"]).abs().max()))
        print(f"cross vs paired-on-N^2 {X.CASES[ci]} t={t} centre={centre}: dv {dv:.2e} / 2 bound {2 * bound:.2e}")
        assert dv <= 2 * bound, (dv, bound)


@pytest.mark.parametrize("ci", [2, 5])
def test_rows_do_not_depend_on_the_batch(dev, ci):
    """A row alone, or in a batch of another size, has the same bits (weights and velocities)."""
    B = X.CASES[ci][0]
    for si, (t, gamma) in enumerate(X.STEPS):
        inp = X.case(ci, si, 0.0)[0]
        full = _apply(_to(dev, inp), t, gamma)
        for rows in (slice(0, 1), slice(B - 1, B), slice(max(B - 7, 1), B)):
            part = _apply(_to(dev, inp, rows), t, gamma)
            for name, f, p in zip(("wx", "wy", "vx", "vy"), full, part):
                assert torch.equal(f[rows], p), (name, t, rows)


@pytest.mark.parametrize("ci", [2, 4])
def test_scratch_is_written_before_it_is_read(dev, ci):
    """Whatever the caller's workspace holds -- NaN or zeros -- and whether it is exactly
    rgfm_guidance_cross_workspace_bytes or 4 KB more, the outputs are the same bits; one byte short is an error."""
    B, N, dx, dy = X.CASES[ci]
    si = 2
    t, gamma = X.STEPS[si]
    inp = X.case(ci, si, 1.0)[0]
    need = _workspace_bytes(B, N, dx, dy)
    assert need % 4 == 0
    outs = []
    for fill in (float("nan"), 0.0):
        for extra in (0, 4096):
            d = _to(dev, inp)
            wx, wy = torch.full((B, N), SENTINEL, device=dev), torch.full((B, N), SENTINEL, device=dev)
            ws = torch.full(((need + extra) // 4,), fill, device=dev)
            _raw(d, t, gamma, wx, wy, ws, need + extra)
            outs.append((wx, wy, d["vx"], d["vy"]))
    for o in outs:
        for a, b in zip(outs[0], o):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    d = _to(dev, inp)
    wx = torch.full((B, N), SENTINEL, device=dev)
    ws = torch.zeros(need // 4, device=dev)
    with pytest.raises(_lib.RgfmError):
        _raw(d, t, gamma, wx, wx, ws, need - 1)
    torch.cuda.synchronize()
    assert bool((wx == SENTINEL).all()) and torch.equal(d["vx"], torch.tensor(inp["vx"], device=dev))


@pytest.mark.parametrize("ci", [0, 2, 5])
def test_outputs_stay_inside_their_buffers(dev, ci):
    """vx, vy and both weight outputs as views into the middle of larger buffers: 256 floats on each side keep their
    sentinel, the inputs keep their bits, and the results are those of a plain call."""
    B, N, dx, dy = X.CASES[ci]
    si = 1
    t, gamma = X.STEPS[si]
    inp = X.case(ci, si, 1.0)[0]
    plain = _apply(_to(dev, inp), t, gamma)
    d = _to(dev, inp)
    kept = {k: d[k].clone() for k in ("x", "y", "mx", "my", "R")}
    big = {name: torch.full((PAD + n + PAD,), SENTINEL, device=dev)
           for name, n in (("vx", B * dx), ("vy", B * dy), ("wx", B * N), ("wy", B * N))}
    view = lambda name, shape: big[name][PAD:-PAD].view(shape)
    view("vx", (B, dx)).copy_(d["vx"])
    view("vy", (B, dy)).copy_(d["vy"])
    d["vx"], d["vy"] = view("vx", (B, dx)), view("vy", (B, dy))
    need = _workspace_bytes(B, N, dx, dy)
    _raw(d, t, gamma, view("wx", (B, N)), view("wy", (B, N)), torch.empty(need // 4, device=dev), need)
    torch.cuda.synchronize()
    for name in big:
        assert bool((big[name][:PAD] == SENTINEL).all()) and bool((big[name][-PAD:] == SENTINEL).all()), name
    for k, v in kept.items():
        assert torch.equal(d[k], v), k
    for p, name, shape in zip(plain, ("wx", "wy", "vx", "vy"), ((B, N), (B, N), (B, dx), (B, dy))):
        assert torch.equal(p, view(name, shape)), name
    # the weight outputs are optional
    d2 = _to(dev, inp)
    assert _engine.guidance_apply_cross(d2["x"], d2["y"], d2["vx"], d2["vy"], d2["mx"], d2["my"], d2["R"], t, gamma) is None
    assert torch.equal(d2["vx"], plain[2]) and torch.equal(d2["vy"], plain[3])


def test_ratio_and_underflow_edges(dev):
    """A zero row and a zero column of R give exactly zero wx_i / wy_j, the other weights match float64 as before; one
    entry 1e4 x the rest stays within tolerance.  A row of (x, y) moved by +20 per element, so that all but one a_i
    underflow: finite, and within 1e-6 absolute of float64."""
    N = X.CASES[X.EDGE_CASE][1]
    for si, (t, gamma) in enumerate(X.STEPS):
        for kind in ("zero", "big"):
            inp, ref = X.ratio_edge(si, kind)
            got = _apply64(dev, inp, t, gamma)
            if kind == "zero":
                assert (got[0][:, 5] == 0).all() and (got[1][:, 9] == 0).all()
                assert (ref["wx"][:, 5] == 0).all() and (ref["wy"][:, 9] == 0).all()
            _check_block(got, inp, ref, N, t, gamma, 0.0, f"R edge '{kind}'")
    inp, ref, row, gap = X.shifted_row()
    assert gap >= 104, gap  # the precondition: exp(-gap) < 2^-150, every other a_i of the row is 0 in fp32
    t, gamma = X.STEPS[3]
    wx, wy, vx, vy = _apply64(dev, inp, t, gamma)
    assert all(np.isfinite(a).all() for a in (wx, wy, vx, vy))
    assert abs(wx[row].sum() - 1) < 1e-6 and abs(wy[row].sum() - 1) < 1e-6
    assert np.abs(wx[row] - ref["wx"][row]).max() < 1e-6 and np.abs(wy[row] - ref["wy"][row]).max() < 1e-6
    others = np.arange(wx.shape[0]) != row
    tw = X.tol_w_cross(t, 0.0)
    assert _rel_dw(wx[others], ref["wx"][others]) <= tw and _rel_dw(wy[others], ref["wy"][others]) <= tw


def test_block_argument_errors(dev):
    """Null pointers, n_mc outside 1 .. 1024, a flattened size that is no multiple of 4 and a ratio vector in the
    matrix's place are errors, and the outputs are not touched."""
    L = _lib.lib()
    nb = ctypes.c_size_t()
    for args in ((2, 0, 4, 4), (2, 1025, 4, 4), (2, 3, 6, 4), (2, 3, 4, 6), (0, 3, 4, 4), (2, 3, 4, 0)):
        assert L.rgfm_guidance_cross_workspace_bytes(*args, ctypes.byref(nb)) == -1, args
    assert L.rgfm_guidance_cross_workspace_bytes(2, 3, 4, 4, None) == -1
    g = torch.Generator().manual_seed(5)
    B, N, dx, dy = 2, 3, 4, 8
    d = {"x": torch.randn(B, dx, generator=g), "y": torch.randn(B, dy, generator=g), "mx": torch.randn(N, dx, generator=g),
         "my": torch.randn(N, dy, generator=g), "R": torch.ones(N, N)}
    d = {k: v.to(dev) for k, v in d.items()}
    d["vx"], d["vy"] = torch.full((B, dx), SENTINEL, device=dev), torch.full((B, dy), SENTINEL, device=dev)
    need = _workspace_bytes(B, N, dx, dy)
    ws = torch.zeros(need // 4, device=dev)
    order = ("x", "y", "vx", "vy", "mx", "my", "R")
    for missing in order + ("ws",):
        ptrs = [None if k == missing else _p(d[k]) for k in order]
        rc = L.rgfm_guidance_apply_cross(*ptrs, B, N, dx, dy, 0.5, 1.0, None, None, None if missing == "ws" else _p(ws), need, _stream())
        assert rc == -1 and b"null" in L.rgfm_last_error(), missing
    for n_bad in (0, 1025):
        assert L.rgfm_guidance_apply_cross(*[_p(d[k]) for k in order], B, n_bad, dx, dy, 0.5, 1.0, None, None, _p(ws), need, _stream()) == -1
    out = torch.full((B, _lib.DIAG_FLOATS), SENTINEL, device=dev)
    assert L.rgfm_guidance_diag_cross(*[_p(d[k]) for k in order], B, N, dx, dy, 0.5, None, _p(ws), need, _stream()) == -1
    assert L.rgfm_guidance_diag_cross(*[_p(d[k]) for k in order], B, N, dx, dy, 0.5, _p(out), _p(ws), need - 1, _stream()) == -2
    with pytest.raises(_lib.RgfmError, match=r"\[N, N\]"):
        _engine.guidance_apply_cross(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"], d["R"][0], 0.5, 1.0)
    with pytest.raises(_lib.RgfmError, match=r"\[N, N\]"):
        _engine.guidance_diag_cross(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"][:2], d["R"], 0.5)
    torch.cuda.synchronize()
    for a in (d["vx"], d["vy"], out):
        assert bool((a == SENTINEL).all())


# ------------------------------------------------------------------ 2. the block's diagnostics
@pytest.mark.parametrize("centre", X.CENTRES)
@pytest.mark.parametrize("si", range(len(X.STEPS)))
@pytest.mark.parametrize("ci", range(len(X.CASES)))
def test_diag_cross_vs_float64(dev, ci, si, centre):
    B, N, dx, dy = X.CASES[ci]
    t = X.STEPS[si][0]
    inp = X.case(ci, si, centre)[0]
    ref = X.diag_of(inp, t)
    d = _to(dev, inp)
    v0 = d["vx"].clone(), d["vy"].clone()
    got = _engine.guidance_diag_cross(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"], d["R"], t).cpu().numpy()
    assert torch.equal(d["vx"], v0[0]) and torch.equal(d["vy"], v0[1])  # v is only read
    D.check(got, ref, D.bounds(inp, ref, N, (dx, dy), t, X.tol_w_cross(t, centre)), f"diag cross {X.CASES[ci]} t={t} centre={centre}")
    ess = got[:, 0].astype(np.float64)
    assert (ess >= 1 - 1e-5).all() and (ess <= N * N * (1 + 1e-5)).all(), (ess.min(), ess.max(), N * N)


# ------------------------------------------------------------------ 3. the U-Net pair loop
B_L, N_L, STEPS_L = 5, 7, 6
NETS = {"unet28": lambda: make_module("unet28"),
        "rgb32": lambda: load_synth(M.FlexibleUNet(3, 32, 32, (1, 2), 1), 51).eval()}
SOLVERS = ("euler", "midpoint")


@functools.lru_cache(maxsize=None)
def loop_nets():
    return NETS["unet28"](), NETS["rgb32"]()


@functools.lru_cache(maxsize=None)
def loop_inputs():
    """(x0, y0, mc_x, mc_y, R) on the CPU: shared, never modified."""
    fx, fy = loop_nets()
    sx, sy = (fx.in_channels, fx.img_size, fx.img_size), (fy.in_channels, fy.img_size, fy.img_size)
    g = torch.Generator().manual_seed(4100)
    x0, y0 = torch.randn(B_L, *sx, generator=g), torch.randn(B_L, *sy, generator=g)
    mx, my = 0.5 * torch.randn(N_L, *sx, generator=g), 0.5 * torch.randn(N_L, *sy, generator=g)
    R = torch.exp(0.5 * torch.randn(N_L, N_L, generator=g))
    return x0, y0, mx, my, R


@functools.lru_cache(maxsize=None)
def loop64(gamma, solver):
    """float64 end state of the cross loop: unet_ref64.forward64 + cross64, composed by ode_ref64.integrate64."""
    fx, fy = NETS["unet28"](), NETS["rgb32"]()  # (fresh CPU modules: loop_nets() live on the device)
    x0, y0, mx, my, R = (t.numpy().astype(np.float64) for t in loop_inputs())
    velx, vely = O.velocity_of(fx), O.velocity_of(fy)
    mxf, myf = mx.reshape(N_L, -1), my.reshape(N_L, -1)

    def F(s, t):
        x, y = s
        vx, vy = np.asarray(velx(x, t), np.float64), np.asarray(vely(y, t), np.float64)
        if O.guided_after_eps(t):
            gx, gy = X.cross64(x.reshape(B_L, -1), y.reshape(B_L, -1), vx.reshape(B_L, -1), vy.reshape(B_L, -1), mxf, myf, R, t, gamma)[:2]
            vx, vy = gx.reshape(x.shape), gy.reshape(y.shape)
        return vx, vy
    out = O.integrate64(F, (x0, y0), STEPS_L, solver)
    for a in out:
        a.setflags(write=False)
    return out


def run_cross(dev, gamma, solver, ranges=((0, STEPS_L),), rows=slice(None), R=None, diag=None):
    fx, fy = (n.to(dev) for n in loop_nets())
    x0, y0, mx, my, R0 = loop_inputs()
    x, y = x0[rows].to(dev).clone(), y0[rows].to(dev).clone()
    for b, e in ranges:
        _engine.sample_pair(fx, fy, x, y, mx.to(dev), my.to(dev), (R0 if R is None else R).to(dev), STEPS_L, gamma, b, e,
                            solver=solver, diag=diag)
    return x, y


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("gamma", [0.0, 0.7])
def test_loop_vs_float64_split_and_rows(dev, gamma, solver):
    x, y = run_cross(dev, gamma, solver)
    wx, wy = loop64(gamma, solver)
    ex = float(np.abs(x.cpu().numpy().astype(np.float64) - wx).max())
    ey = float(np.abs(y.cpu().numpy().astype(np.float64) - wy).max())
    print(f"cross loop gamma={gamma} {solver}: err vs float64 x {ex:.3e} y {ey:.3e}")
    assert ex <= TOL_SAMPLER and ey <= TOL_SAMPLER, (ex, ey)
    # splitting the integration at step boundaries changes no bit
    sx, sy = run_cross(dev, gamma, solver, ((0, 2), (2, 5), (5, STEPS_L)))
    assert torch.equal(sx, x) and torch.equal(sy, y)
    # a row alone: the same bits
    for b in (0, B_L - 1):
        rx, ry = run_cross(dev, gamma, solver, rows=slice(b, b + 1))
        assert torch.equal(rx, x[b:b + 1]) and torch.equal(ry, y[b:b + 1]), b
    # gamma = 0 is the unguided loop; gamma = 0.7 is not
    fx, fy = (n.to(dev) for n in loop_nets())
    x0, y0 = loop_inputs()[:2]
    ux, uy = _engine.sample_pair(fx, fy, x0.to(dev).clone(), y0.to(dev).clone(), None, None, None, STEPS_L, 0.0, solver=solver)
    diff = max(float((x - ux).abs().max()), float((y - uy).abs().max()))
    print(f"cross loop gamma={gamma} {solver}: max |guided - unguided| {diff:.3e}")
    if gamma == 0.0:
        assert diff <= 1e-6, diff
    else:
        assert diff > 1e-3, diff


@pytest.mark.parametrize("solver", SOLVERS)
def test_loop_constant_ratio_matrix_is_the_all_ones_matrix(dev, solver):
    """The weights are normalised: R = c 1 1^T guides as R = 1 1^T does (c = 2.5: every u / Z_bar rounds on its own, so
    equal to fp32 rounding through six steps, not bitwise), and neither is the unguided loop."""
    ones = torch.ones(N_L, N_L)
    a = run_cross(dev, 0.7, solver, R=ones)
    b = run_cross(dev, 0.7, solver, R=2.5 * ones)
    c = run_cross(dev, 0.7, solver)
    diff = max(float((p - q).abs().max()) for p, q in zip(a, b))
    moved = max(float((p - q).abs().max()) for p, q in zip(a, c))
    print(f"cross loop {solver}: R = 2.5 vs R = 1: {diff:.3e}; R = 1 vs the case's R: {moved:.3e}")
    assert diff <= 1e-5, diff
    assert moved > 1e-3, moved


@pytest.mark.parametrize("solver", SOLVERS)
def test_loop_diagnostics_keep_the_bits_and_match_the_block(dev, solver):
    per = 2 if solver == "midpoint" else 1
    plain = run_cross(dev, 0.7, solver)
    rec = torch.full((STEPS_L * per, B_L, _lib.DIAG_FLOATS), SENTINEL, device=dev)
    with_diag = run_cross(dev, 0.7, solver, diag=rec)
    assert torch.equal(plain[0], with_diag[0]) and torch.equal(plain[1], with_diag[1])
    assert not bool(rec[0].any())  # the stage at t = 0 runs unguided: an all-zero record
    ess = rec[1:, :, 0]
    assert bool((ess >= 1 - 1e-5).all()) and bool((ess <= N_L * N_L * (1 + 1e-5)).all())
    # the first stage of step K, recorded by a call of that step alone, against the block at that stage's state
    K = 3
    x, y = run_cross(dev, 0.7, solver, ((0, K),))
    one = torch.full((per, B_L, _lib.DIAG_FLOATS), SENTINEL, device=dev)
    fx, fy = (n.to(dev) for n in loop_nets())
    _, _, mx, my, R = (t.to(dev) for t in loop_inputs())
    xs, ys = x.clone(), y.clone()
    _engine.sample_pair(fx, fy, xs, ys, mx, my, R, STEPS_L, 0.7, K, K + 1, solver=solver, diag=one)
    assert torch.equal(one, rec[K * per:(K + 1) * per])
    t = K * (1.0 / STEPS_L)
    tt = torch.full((B_L,), t, device=dev)
    vx, vy = fx(x, tt).reshape(B_L, -1), fy(y, tt).reshape(B_L, -1)
    blk = _engine.guidance_diag_cross(x.reshape(B_L, -1), y.reshape(B_L, -1), vx, vy, mx.reshape(N_L, -1), my.reshape(N_L, -1), R, t)
    # the weights' entries and |g| depend on the state and the MC set alone: the same kernels, the same bits
    for k in (0, 1, 2, 3, 6, 7):
        assert torch.equal(one[0, :, k], blk[:, k]), D.FIELDS[k]
    # |v|: the loop's own net evaluation against the module's forward
    for k in (4, 5):
        assert torch.allclose(one[0, :, k], blk[:, k], rtol=1e-4, atol=0), D.FIELDS[k]


def test_loop_argument_errors(dev):
    fx, fy = (n.to(dev) for n in loop_nets())
    x0, y0, mx, my, R = (t.to(dev) for t in loop_inputs())
    x, y = x0.clone(), y0.clone()
    L = _lib.lib()
    hx, hy = fx._engine.handle(dev), fy._engine.handle(dev)
    nb = ctypes.c_size_t()
    assert L.rgfm_sample_pair_cross_workspace_bytes(hx, hy, B_L, 1025, 0, ctypes.byref(nb)) == -1
    assert L.rgfm_sample_pair_cross_workspace_bytes(hx, hy, B_L, N_L, 7, ctypes.byref(nb)) == -1
    assert L.rgfm_sample_pair_cross_workspace_bytes(None, hy, B_L, N_L, 0, ctypes.byref(nb)) == -1
    _lib.check(L.rgfm_sample_pair_cross_workspace_bytes(hx, hy, B_L, N_L, 1, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    rec = torch.full((2 * STEPS_L, B_L, _lib.DIAG_FLOATS), SENTINEL, device=dev)

    def call(n=N_L, solver=1, ratios=R, d=None, records=0, nbytes=nb.value, xs=x):
        return L.rgfm_sample_pair_cross(hx, hy, _p(xs) if xs is not None else None, _p(y), _p(mx), _p(my),
                                        _p(ratios) if ratios is not None else None, n, B_L, STEPS_L, 0.7, 0, STEPS_L, solver,
                                        _p(d) if d is not None else None, records, _p(ws), nbytes, _stream())
    assert call(n=1025) == -1 and b"n_mc" in L.rgfm_last_error()
    assert call(n=-1) == -1
    assert call(ratios=None) == -1
    assert call(xs=None) == -1
    assert call(solver=5) == -1
    assert call(nbytes=nb.value - 1) == -2
    assert call(d=rec, records=2 * STEPS_L * B_L - 1) == -1 and b"diag_records" in L.rgfm_last_error()
    assert call(d=rec, records=0) == -1 and call(d=None, records=4) == -1
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(y, y0) and bool((rec == SENTINEL).all())
    assert call(d=rec, records=2 * STEPS_L * B_L) == 0
    # n_mc = 0: the unguided loop
    x2, y2 = x0.clone(), y0.clone()
    assert L.rgfm_sample_pair_cross(hx, hy, _p(x2), _p(y2), None, None, None, 0, B_L, STEPS_L, 0.7, 0, STEPS_L, 0, None, 0,
                                    _p(ws), nb.value, _stream()) == 0
    ux, uy = _engine.sample_pair(fx, fy, x0.clone(), y0.clone(), None, None, None, STEPS_L, 0.0)
    assert torch.equal(x2, ux) and torch.equal(y2, uy)
    with pytest.raises(_lib.RgfmError, match=r"\[N, N\]"):  # a matrix of the wrong size
        _engine.sample_pair(fx, fy, x0.clone(), y0.clone(), mx, my, R[:, :3].contiguous(), STEPS_L, 0.7)


# ------------------------------------------------------------------ 4. the Python surface
@functools.lru_cache(maxsize=None)
def small_models():
    """g16 (x: 1x16x16), g24 (y: 3x24x24) and a FlexibleRatioEstimator for that pair."""
    fx, fy = make_generic_unet("g16")[0], make_generic_unet("g24")[0]
    rr = load_synth(M.FlexibleRatioEstimator(1, 3, CG.FEAT, CG.HID), CG.W_SEED).eval()
    return fx, fy, rr


def _shape(n):
    return (n.in_channels, n.img_size, n.img_size)


@pytest.mark.parametrize("solver", SOLVERS)
def test_paired_sampler_cross_is_the_direct_engine_calls(dev, solver, capsys):
    from ratio_guided_multimodal_fm_amd.synth import paired_noise
    from ratio_guided_multimodal_fm_amd.utils.diagnostics import GuidanceDiagnostics
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler
    fx, fy, rr = (m.to(dev) for m in small_models())
    B, N, steps, gamma = 4, 6, 4, 0.7
    noise = paired_noise(31, B, N, _shape(fx), _shape(fy))
    args = (fx, fy, rr, "mc_feng", gamma, B, steps, dev, N, _shape(fx), _shape(fy))
    xs, ys = paired_sampler(*args, noise=noise, verbose=True, solver=solver, mc_pairing="cross")
    out = capsys.readouterr().out
    assert "MC ratio matrix [6 x 6]: min=" in out and "its diagonal (the paired ratios): min=" in out and "mean=" in out
    x, y, mx, my = (t.to(dev, copy=True).contiguous() for t in noise)
    _engine.sample_two_streams(fx, mx, fy, my, steps, solver=solver)
    R = rr._engine.eval_cross(mx, my, "ratio")
    assert tuple(R.shape) == (N, N)
    _engine.sample_pair(fx, fy, x, y, mx, my, R, steps, gamma, solver=solver)
    assert torch.equal(xs, x) and torch.equal(ys, y)
    # the paired call on the same noise is another result; the default is the paired call
    px, py = paired_sampler(*args, noise=noise, verbose=False, solver=solver, mc_pairing="paired")
    dx, dy = paired_sampler(*args, noise=noise, verbose=False, solver=solver)
    assert torch.equal(px, dx) and torch.equal(py, dy) and not torch.equal(px, xs)
    # diagnostics: the same samples, the joint ESS in 1 .. N^2
    d = GuidanceDiagnostics()
    qx, qy = paired_sampler(*args, noise=noise, verbose=False, solver=solver, mc_pairing="cross", diagnostics=d)
    assert torch.equal(qx, xs) and torch.equal(qy, ys)
    ess = d.ess()[1:]
    assert bool((ess >= 1 - 1e-5).all()) and bool((ess <= N * N * (1 + 1e-5)).all()) and "Z_bar" in d.reference_block(1)


def test_paired_default_passes_the_same_arguments_as_before(dev, monkeypatch):
    """mc_pairing='paired' (and no mc_pairing at all) calls _engine.sample_pair exactly as the sampler did before the
    keyword existed: the same positional arguments, a ratio VECTOR from RatioEngine.eval, the same keywords."""
    from ratio_guided_multimodal_fm_amd.synth import paired_noise
    from ratio_guided_multimodal_fm_amd.utils import flow_utils
    fx, fy, rr = (m.to(dev) for m in small_models())
    B, N, steps, gamma = 3, 5, 3, 0.7
    noise = paired_noise(32, B, N, _shape(fx), _shape(fy))
    calls = []
    real = _engine.sample_pair

    def spy(*a, **k):
        calls.append((a, dict(k)))
        return real(*a, **k)
    monkeypatch.setattr(flow_utils._engine, "sample_pair", spy)
    args = (fx, fy, rr, "mc_feng", gamma, B, steps, dev, N, _shape(fx), _shape(fy))
    a = flow_utils.paired_sampler(*args, noise=noise, verbose=False)
    b = flow_utils.paired_sampler(*args, noise=noise, verbose=False, mc_pairing="paired")
    c = flow_utils.paired_sampler(*args, noise=noise, verbose=False, mc_pairing="cross")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    (a0, k0), (a1, k1), (a2, k2) = calls
    assert len(a0) == len(a1) == len(a2) == 9 and k0 == k1 == k2 == {"solver": "euler", "diag": None}
    assert a0[0] is fx and a0[1] is fy and a0[7:] == (steps, gamma) and a1[7:] == (steps, gamma)
    assert tuple(a0[6].shape) == (N,) and tuple(a1[6].shape) == (N,) and tuple(a2[6].shape) == (N, N)
    for p, q in zip(a0[4:7], a1[4:7]):
        assert torch.equal(p, q)
    assert torch.equal(a0[6], rr._engine.eval(a0[4], a0[5], "ratio"))
    assert torch.allclose(a2[6].diagonal(), a0[6], rtol=1e-4)  # (the matrix's diagonal: the paired ratios, from another kernel)


def test_flow_matching_model_pairs_and_sharded_launches_raise(dev):
    from ratio_guided_multimodal_fm_amd.distributed import make_sharded_sampler, sharded_paired_sampler
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_bimodal_guided
    fm_x, fm_y, rr = make_module("fm_original", dev), make_module("fm_original_y", dev), make_module("ratio28", dev)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        sample_bimodal_guided(fm_x, fm_y, rr, "mc_feng", 0.5, 2, 2, dev, 4, mc_pairing="cross")
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 1, 28, 28, generator=g).to(dev), torch.randn(2, 1, 28, 28, generator=g).to(dev)
    mx, my = torch.randn(4, 1, 28, 28, generator=g).to(dev), torch.randn(4, 1, 28, 28, generator=g).to(dev)
    x0 = x.clone()
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        _engine.sample_pair(fm_x, fm_y, x, y, mx, my, torch.ones(4, 4, device=dev), 2, 0.5)
    assert torch.equal(x, x0)
    # (the paired loop of the FlowMatchingModel pair is still there)
    assert sample_bimodal_guided(fm_x, fm_y, rr, "mc_feng", 0.5, 2, 2, dev, 4)[0].shape == (2, 1, 28, 28)
    ux, uy = make_module("unet28", dev), make_module("unet28", dev)
    noise = tuple(t.cpu() for t in (x, y, mx, my))
    with pytest.raises(_lib.RgfmError, match="sharded"):
        sharded_paired_sampler(ux, uy, rr, "mc_feng", 0.5, 2, noise, dev, mc_pairing="cross")
    with pytest.raises(_lib.RgfmError, match="sharded"):
        make_sharded_sampler((1, 28, 28), (1, 28, 28))(ux, uy, rr, "mc_feng", 0.5, 2, 2, dev, 4, mc_pairing="cross")
    with pytest.raises(ValueError):
        sample_bimodal_guided(ux, uy, rr, "grad_log_ratio", 0.5, 2, 2, dev, 4, mc_pairing="cross")
    with pytest.raises(ValueError):
        sample_bimodal_guided(ux, uy, rr, "mc_feng", 0.5, 2, 2, dev, 4, mc_pairing="all")


def test_cli_mc_pairing_cross_equals_the_direct_call(dev, tmp_path, monkeypatch):
    import ratio_guided_multimodal_fm_amd as R
    from ratio_guided_multimodal_fm_amd import sample_mnist_svhn
    ck = tmp_path / "checkpoints"
    ck.mkdir()
    fm, fs, rr = make_module("mnist32"), make_module("svhn"), make_module("ratio_ms")
    torch.save({"epoch": 1, "model_state_dict": fm.state_dict(), "best_loss": 0.5}, ck / "flow_mnist32_best.pth")
    torch.save({"epoch": 1, "model_state_dict": fs.state_dict(), "best_loss": 0.5}, ck / "flow_svhn_best.pth")
    torch.save(rr.state_dict(), ck / "ratio_disc_mnist_svhn_best.pth")
    monkeypatch.chdir(tmp_path)
    argv = ["--guidance_method", "mc_feng", "--guidance_strength", "0.5", "--num_steps", "3", "--num_samples", "3",
            "--mc_batch_size", "5", "--seed", "9"]
    assert sample_mnist_svhn.main(argv + ["--mc_pairing", "cross"]) == 0
    saved = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_mc_feng_gamma0.5.pt")
    R.utils.set_seed(9)
    xs, ys = sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(fm.to(dev), fs.to(dev), rr.to(dev), "mc_feng", 0.5, 3, 3, dev, 5,
                                                                mc_pairing="cross")
    assert torch.equal(saved["mnist"], xs.cpu()) and torch.equal(saved["svhn"], ys.cpu())
    R.utils.set_seed(9)
    px, _ = sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(fm.to(dev), fs.to(dev), rr.to(dev), "mc_feng", 0.5, 3, 3, dev, 5)
    assert not torch.equal(px, xs)
