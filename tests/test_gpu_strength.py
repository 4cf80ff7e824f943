"""Guidance strength per sample and per stage on the GPU (include/rgfm.h, "Guidance strength per sample and per stage"):
the *_rows blocks and the *_gs loops against today's scalar entry points (bitwise: torch.equal) and against float64
(tests/strength_ref64.py, guidance_ref64.py).

Nets and inputs are those of tests/test_gpu_ode.py: the generic U-Nets g16 (1x16x16) and g24 (3x24x24), the
FlexibleRatioEstimator of that pair, seeded start states, MC sets and ratios.  B = 37 in the bitwise tests: two 32-row
tiles of guid_apply_mfma_kernel, the second with 5 rows (not a multiple of 4) -- what a wrong row index in the epilogue
cannot survive.  ROWS cycles through 0, 0.5, 1, 2, 5 and -0.5: off, inside (0, 1), the pure guided velocity,
extrapolation, and a negative strength (values are not clamped).

Tolerances: none of its own.  Blocks: guidance_ref64.velocity_bound at the row's own strength (|gamma| for the negative
one: the bound's first term is the error of g times the size of its coefficient).  Loops: TOL_SAMPLER = 1e-4, the
project's sampler tolerance.
"""
import copy
import ctypes
import json

import numpy as np
import pytest
import torch

import guidance_ref64 as R
import ode_ref64 as O
import strength_ref64 as S
import test_gpu_ode as T
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd.utils.guidance_schedule import GuidanceSchedule

pytestmark = pytest.mark.gpu

TOL_SAMPLER = 1e-4
EINVAL, ENOMEM = -1, -2
ROWS = (0.0, 0.5, 1.0, 2.0, 5.0, -0.5)
B37, N_MC, STEPS = 37, 7, 4
KINDS = ("pair", "cross", "cond", "pair_grad", "cond_grad")
SOLVERS = ("euler", "midpoint")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def cycle(B, dev=None):
    g = torch.tensor([ROWS[b % len(ROWS)] for b in range(B)], dtype=torch.float32)
    return g if dev is None else g.to(dev)


# ------------------------------------------------------------------ 1, 2. the blocks
BLOCK_CASES = [0, 3, 4, 6]  # guidance_ref64.CASES (33, 70, 784, 784), (37, 544, 68, 4), (5, 257, 520, 48), (1, 1, 4, 4)
BLOCK_STEPS = [1, 3]        # guidance_ref64.STEPS at t = 0.5 and t = 0.99


def _dev_inputs(dev, inp):
    return {k: torch.tensor(v, device=dev) for k, v in inp.items()}


@pytest.mark.parametrize("si", BLOCK_STEPS)
@pytest.mark.parametrize("ci", BLOCK_CASES)
def test_block_rows_are_the_scalar_block_bitwise_and_meet_float64(dev, ci, si):
    B, N, dx, dy = R.CASES[ci]
    t = R.STEPS[si][0]
    inp, ref = R.case(ci, si, 1.0)
    rows = cycle(B, dev)
    d = _dev_inputs(dev, inp)
    w = _engine.guidance_apply(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"], d["r"], t, rows, True)
    for j, gamma in enumerate(ROWS[:min(B, len(ROWS))]):
        s = _dev_inputs(dev, inp)
        ws = _engine.guidance_apply(s["x"], s["y"], s["vx"], s["vy"], s["mx"], s["my"], s["r"], t, gamma, True)
        pick = slice(j, B, len(ROWS))
        assert torch.equal(d["vx"][pick], s["vx"][pick]) and torch.equal(d["vy"][pick], s["vy"][pick]), (ci, si, gamma)
        assert torch.equal(w, ws)  # (the weights do not depend on the strength)
    # float64: each row against guidance64's blend at its own strength, under the existing bound evaluated there
    vx, vy = d["vx"].cpu().numpy().astype(np.float64), d["vy"].cpu().numpy().astype(np.float64)
    tw = R.tol_w(t, 1.0)
    worst = 0.0
    for b in range(B):
        g = float(rows[b])
        wx = (1 - g) * inp["vx"][b].astype(np.float64) + g * ref["gx"][b]
        wy = (1 - g) * inp["vy"][b].astype(np.float64) + g * ref["gy"][b]
        row_ref = {"gx": ref["gx"][b], "gy": ref["gy"][b], "vx": wx, "vy": wy}
        bound = R.velocity_bound(inp, row_ref, N, t, abs(g), tw)
        dv = max(float(np.abs(vx[b] - wx).max()), float(np.abs(vy[b] - wy).max()))
        worst = max(worst, dv / bound)
        assert dv <= bound, (ci, si, b, g, dv, bound)
    print(f"block rows {R.CASES[ci]} t={t}: worst dv / bound over the rows {worst:.3f}")


def test_one_sided_and_cross_block_rows_are_the_scalar_blocks_bitwise(dev):
    B, N, dx, dy = R.CASES[3]  # (37, 544, 68, 4)
    assert B == B37
    t = 0.5
    inp, _ = R.case(3, 1, 1.0)
    rows = cycle(B, dev)
    g = torch.Generator().manual_seed(4242)
    Rrows = torch.exp(0.5 * torch.randn(B, N, generator=g)).to(dev)
    Rmat = torch.exp(0.5 * torch.randn(N, N, generator=g)).to(dev)
    d = _dev_inputs(dev, inp)
    w = _engine.guidance_apply_cond(d["x"], d["vx"], d["mx"], Rrows, t, rows, True)
    c = _dev_inputs(dev, inp)
    wx, wy = _engine.guidance_apply_cross(c["x"], c["y"], c["vx"], c["vy"], c["mx"], c["my"], Rmat, t, rows, True)
    for j, gamma in enumerate(ROWS):
        pick = slice(j, B, len(ROWS))
        s = _dev_inputs(dev, inp)
        ws = _engine.guidance_apply_cond(s["x"], s["vx"], s["mx"], Rrows, t, gamma, True)
        assert torch.equal(d["vx"][pick], s["vx"][pick]) and torch.equal(w, ws), gamma
        s = _dev_inputs(dev, inp)
        sx, sy = _engine.guidance_apply_cross(s["x"], s["y"], s["vx"], s["vy"], s["mx"], s["my"], Rmat, t, gamma, True)
        assert torch.equal(c["vx"][pick], s["vx"][pick]) and torch.equal(c["vy"][pick], s["vy"][pick]), gamma
        assert torch.equal(wx, sx) and torch.equal(wy, sy)
    assert not torch.equal(d["vx"], torch.tensor(inp["vx"], device=dev))


# ------------------------------------------------------------------ the five loops through _engine
class Loop:
    """One guided loop on fresh device copies of the shared start state: run() through _engine (the scalar entry points
    of today, or the *_gs twins with gamma_rows / stage_scale), unguided() the unguided loop over a step range."""

    def __init__(self, kind, B, dev):
        self.kind, self.B, self.dev = kind, B, dev
        self.nx, self.ny = T.net("g16").to(dev), T.net("g24").to(dev)
        if kind in ("pair", "cross", "pair_grad"):
            self.state = [T.start("g16", B).to(dev).clone(), T.start("g24", B).to(dev).clone()]
        elif kind == "cond":
            self.state = [T.start("g24", B).to(dev).clone()]
        else:
            self.state = [T.start("g16", B).to(dev).clone()]
        if kind in ("pair", "cross"):
            self.mx, self.my = T.mc_set("g16", N_MC).to(dev), T.mc_set("g24", N_MC).to(dev)
            self.r = (T.ratios(N_MC, N_MC) if kind == "cross" else T.ratios(N_MC)).to(dev)
        elif kind == "cond":
            self.m, self.R = T.mc_set("g24", N_MC).to(dev), T.ratios(B, N_MC).to(dev)
        elif kind == "pair_grad":
            self.rr = T.flex().to(dev)
        else:  # the 3x24x24 side observed as the estimator's x, the target g16 its y
            rr, tnet, _, _ = T.cond_grad_case("x")
            self.rr, self.tnet = rr.to(dev), tnet.to(dev)
            cond = T.start("g24", B, salt=1).to(dev)
            self.ctx = self.rr._engine.cond_prepare(cond, "x", tuple(self.state[0].shape[1:]))

    def run(self, gamma, steps=STEPS, b=0, e=None, solver="euler", **kw):
        s = self.state
        if self.kind in ("pair", "cross"):
            _engine.sample_pair(self.nx, self.ny, s[0], s[1], self.mx, self.my, self.r, steps, gamma, b, e, solver=solver, **kw)
        elif self.kind == "cond":
            _engine.sample_cond(self.ny, s[0], self.m, self.R, steps, gamma, b, e, solver=solver, **kw)
        elif self.kind == "pair_grad":
            _engine.sample_pair_grad(self.nx, self.ny, self.rr, s[0], s[1], steps, gamma, b, e, solver=solver, **kw)
        else:
            _engine.sample_cond_grad(self.tnet, self.rr, s[0], self.ctx, "x", steps, gamma, b, e, solver=solver, **kw)
        return self

    def unguided(self, steps=STEPS, b=0, e=None, solver="euler"):
        s = self.state
        if len(s) == 2:  # the pair loop with n_mc = 0
            _engine.sample_pair(self.nx, self.ny, s[0], s[1], None, None, None, steps, 0.0, b, e, solver=solver)
        else:
            _engine.sample_single(self.ny if self.kind == "cond" else self.tnet, s[0], steps, b, e, solver=solver)
        return self

    def same(self, other, rows=slice(None)):
        torch.cuda.synchronize()
        return all(torch.equal(a[rows], b[rows]) and bool(torch.isfinite(a).all()) for a, b in zip(self.state, other.state))


# ------------------------------------------------------------------ 3. bitwise against today's entry points
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("kind", KINDS)
def test_loop_rows_are_the_scalar_calls_row_by_row(dev, kind, solver):
    rows = cycle(B37, dev)
    n_stages = STEPS * (2 if solver == "midpoint" else 1)
    mixed = Loop(kind, B37, dev).run(0.0, solver=solver, gamma_rows=rows)
    ones = Loop(kind, B37, dev).run(123.0, solver=solver, gamma_rows=rows, stage_scale=[1.0] * n_stages)
    assert mixed.same(ones)  # (with gamma_rows the call's scalar is not read)
    scalar = {}
    for j, gamma in enumerate(ROWS):
        scalar[gamma] = Loop(kind, B37, dev).run(gamma, solver=solver)
        assert mixed.same(scalar[gamma], slice(j, B37, len(ROWS))), (kind, solver, gamma)
    assert not mixed.same(scalar[0.5])  # (the rows do differ)
    # all rows equal, s = 1: the scalar call
    equal = Loop(kind, B37, dev).run(0.0, solver=solver, gamma_rows=torch.full((B37,), 0.5, device=dev),
                                     stage_scale=[1.0] * n_stages)
    assert equal.same(scalar[0.5])
    # the scalar strength with a scale of ones, too
    assert Loop(kind, B37, dev).run(2.0, solver=solver, stage_scale=[1.0] * n_stages).same(scalar[2.0])


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("kind", KINDS)
def test_gs_entry_point_with_both_null_is_its_namesake(dev, kind, solver, monkeypatch):
    want = Loop(kind, 5, dev).run(0.7, solver=solver)
    # (the *_gs twin with null gamma_rows, null stage_scale and n_stage_scale 0: what _run_loop sends for (None, None))
    monkeypatch.setattr(_engine, "_check_strength", lambda *a: (None, None))
    sent = []
    real = _engine._run_loop
    monkeypatch.setattr(_engine, "_run_loop", lambda *a, **k: (sent.append(k.get("strength")), real(*a, **k))[1])
    got = Loop(kind, 5, dev).run(0.7, solver=solver)
    assert sent and all(s == (None, None) for s in sent)
    assert got.same(want)
    if kind != "cond_grad":
        diag_w, diag_g = (torch.zeros(STEPS * (2 if solver == "midpoint" else 1), 5, 8, device=dev) for _ in range(2))
        monkeypatch.undo()
        Loop(kind, 5, dev).run(0.7, solver=solver, diag=diag_w)
        monkeypatch.setattr(_engine, "_check_strength", lambda *a: (None, None))
        assert Loop(kind, 5, dev).run(0.7, solver=solver, diag=diag_g).same(want)
        assert torch.equal(diag_w, diag_g) and bool(diag_w.any())


# ------------------------------------------------------------------ 4. a window is three chained calls (Euler)
@pytest.mark.parametrize("kind", KINDS)
def test_window_is_unguided_guided_unguided_chained(dev, kind):
    steps, k1, k2, gamma = 6, 2, 4, 0.7
    scale = [1.0 if k1 <= k < k2 else 0.0 for k in range(steps)]
    win = Loop(kind, B37, dev).run(gamma, steps, stage_scale=scale)
    chain = Loop(kind, B37, dev).unguided(steps, 0, k1).run(gamma, steps, k1, k2).unguided(steps, k2, steps)
    assert win.same(chain), kind
    # ... with a strength per row inside the window
    rows = cycle(B37, dev)
    win = Loop(kind, B37, dev).run(0.0, steps, gamma_rows=rows, stage_scale=scale)
    chain = Loop(kind, B37, dev).unguided(steps, 0, k1).run(0.0, steps, k1, k2, gamma_rows=rows).unguided(steps, k2, steps)
    assert win.same(chain), kind
    plain = Loop(kind, B37, dev).unguided(steps)
    assert not win.same(plain)
    # s = 0 everywhere: the unguided call
    assert Loop(kind, B37, dev).run(gamma, steps, stage_scale=[0.0] * steps).same(plain)
    assert Loop(kind, B37, dev).run(gamma, steps, gamma_rows=rows, stage_scale=[0.0] * steps).same(plain)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("kind", ["pair_grad", "cond_grad"])
def test_a_zero_scale_enqueues_no_ratio_pass(dev, kind, solver):
    """By result: with every parameter of the ratio estimator NaN, a loop whose scale is 0 everywhere still has the bits
    of the unguided loop -- no kernel of the estimator ran into the state.  (One guided stage puts NaN there.)"""
    plain = Loop(kind, 5, dev).unguided(solver=solver)
    loop = Loop(kind, 5, dev)
    loop.rr = copy.deepcopy(loop.rr)
    if kind == "cond_grad":  # (the copy's engine binds the condition's image size as the original's did; the context is kept)
        loop.rr._engine.cond_prepare(T.start("g24", 5, salt=1).to(dev), "x", tuple(loop.state[0].shape[1:]))
    with torch.no_grad():
        for p in loop.rr.parameters():
            p.fill_(float("nan"))
    n = STEPS * (2 if solver == "midpoint" else 1)
    assert loop.run(0.7, solver=solver, stage_scale=[0.0] * n).same(plain)
    one = [0.0] * n
    one[-1] = 1.0
    loop.run(0.7, solver=solver, stage_scale=one)
    torch.cuda.synchronize()
    assert bool(torch.isnan(loop.state[0]).any())  # (the NaN estimator is the one the loop runs)


# ------------------------------------------------------------------ 5. midpoint, a boundary inside a step, vs float64
def _ref64(kind, B, gammas, schedule, solver="midpoint"):
    vx, vy = O.velocity_of(T.net("g16")), O.velocity_of(T.net("g24"))
    f = T.f64
    if kind == "pair":
        mk = S.pair_mc(vx, vy, f(T.mc_set("g16", N_MC)).reshape(N_MC, -1), f(T.mc_set("g24", N_MC)).reshape(N_MC, -1), f(T.ratios(N_MC)))
        state = (f(T.start("g16", B)), f(T.start("g24", B)))
    elif kind == "cond":
        mk = S.cond_mc(vy, f(T.mc_set("g24", N_MC)).reshape(N_MC, -1), f(T.ratios(B, N_MC)))
        state = (f(T.start("g24", B)),)
    elif kind == "pair_grad":
        mk = S.pair_grad(vx, vy, T.flex())
        state = (f(T.start("g16", B)), f(T.start("g24", B)))
    else:
        rr, tnet, _, _ = T.cond_grad_case("x")
        mk = S.cond_grad(O.velocity_of(tnet), rr, T.start("g24", B, salt=1).double(), "x")
        state = (f(T.start("g16", B)),)
    return S.integrate_rows64(*mk, state, gammas, STEPS, solver, schedule)


MID_ROWS = (0.35, 0.7, 1.4)  # half, once and twice the strength the midpoint loops are pinned at (test_gpu_ode.GAMMA)


@pytest.mark.parametrize("pattern", ["on_off_off_on", "linear"])
@pytest.mark.parametrize("kind", ["pair", "cond", "pair_grad", "cond_grad"])
def test_midpoint_with_a_boundary_inside_a_step_vs_float64(dev, kind, pattern):
    B = 3
    if pattern == "linear":
        sched = GuidanceSchedule.linear()
    else:  # step i: stage 1 guided and stage 2 not, then the other way round
        sched = GuidanceSchedule.from_values([1.0, 0.0, 0.0, 1.0] * (STEPS // 2))
    scale = sched.stage_values(STEPS, "midpoint")
    rows = torch.tensor(MID_ROWS, dtype=torch.float32)
    got = Loop(kind, B, dev).run(0.0, solver="midpoint", gamma_rows=rows.to(dev), stage_scale=scale)
    torch.cuda.synchronize()
    want = _ref64(kind, B, MID_ROWS, sched)
    errs = [T.err64(g, w) for g, w in zip(got.state, want)]
    plain = _ref64(kind, B, MID_ROWS, GuidanceSchedule.from_values([0.0] * len(scale)))
    full = _ref64(kind, B, MID_ROWS, None)
    moved = max(float(np.abs(a - b).max()) for a, b in zip(want, plain))
    apart = max(float(np.abs(a - b).max()) for a, b in zip(want, full))
    print(f"{kind} midpoint {pattern}: err vs float64 {' '.join(f'{e:.3e}' for e in errs)}; float64 |scheduled - unguided| "
          f"{moved:.3e}, |scheduled - unscheduled| {apart:.3e}")
    assert moved > 10 * TOL_SAMPLER and apart > 10 * TOL_SAMPLER  # (the schedule is visible at this tolerance)
    assert max(errs) <= TOL_SAMPLER, errs


# ------------------------------------------------------------------ 6. diagnostics
@pytest.mark.parametrize("kind", ["pair", "cross", "cond", "pair_grad", "cond_grad"])
def test_diagnostics_records_of_scheduled_and_mixed_calls(dev, kind):
    B = 5
    rec = lambda: torch.full((STEPS, B, 8), -1.0, device=dev)
    scalar, mixed, win = rec(), rec(), rec()
    s = Loop(kind, B, dev).run(0.5, diag=scalar)
    rows = torch.full((B,), 0.5, device=dev)
    m = Loop(kind, B, dev).run(0.0, diag=mixed, gamma_rows=rows)
    assert m.same(s) and torch.equal(scalar, mixed)
    # stages 0, 1 guided as in the scalar call (the same trajectory so far), stages 2, 3 off: all-zero records
    w = Loop(kind, B, dev).run(0.5, diag=win, stage_scale=[1.0, 1.0, 0.0, 0.0])
    torch.cuda.synchronize()
    assert torch.equal(win[:2], scalar[:2]) and bool(scalar[1].any()) and not bool(win[2:].any())
    assert bool(scalar[2:].any()) and not w.same(s)
    # the records do not depend on gamma: another strength at the first guided stage, the same numbers
    other = rec()
    first = 1 if kind in ("pair", "cross", "cond") else 0  # (the MC loops' stage at t = 0 is unguided)
    Loop(kind, B, dev).run(2.0, diag=other, gamma_rows=cycle(B, dev))
    assert torch.equal(other[first], scalar[first])


# ------------------------------------------------------------------ 7. errors
def _gs_call(raw, kind, rows, scale, n_scale, b, e, solver, ws, ws_bytes):
    fn = getattr(_lib.lib(), f"rgfm_sample_{kind}_gs")
    return fn(*raw.args, T._p(rows), scale, n_scale, b, e, solver, None, 0, T._p(ws), ws_bytes, T._stream())


@pytest.mark.parametrize("kind", ["pair", "cond", "pair_grad", "cond_grad"])
def test_argument_errors_touch_nothing_and_guard_bands_stay_intact(dev, kind):
    L = _lib.lib()
    B = 5 if kind != "cond_grad" else 3  # (test_gpu_ode's cond_grad case has its own batch of 3)
    raw = T.make_raw(kind, B, dev)
    before = [s.clone() for s in raw.state]
    rc, nb = raw.ws_bytes(T.EULER)
    assert rc == 0
    GUARD, MARK = 256, -7777.0
    ws = torch.full((nb + 4 * GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    rows_buf = torch.full((B + GUARD,), MARK, device=dev)
    rows_buf[:B] = cycle(B, dev)
    ones = (ctypes.c_double * STEPS)(*([1.0] * STEPS))
    nan = (ctypes.c_double * STEPS)(1.0, float("nan"), 1.0, 1.0)
    inf = (ctypes.c_double * STEPS)(1.0, 1.0, float("inf"), 1.0)
    eight = (ctypes.c_double * (2 * STEPS))(*([1.0] * (2 * STEPS)))

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(a, c) for a, c in zip(raw.state, before))
    bad = [
        ("n_stage_scale", (ones, STEPS - 1, 0, STEPS, T.EULER), EINVAL),
        ("n_stage_scale", (ones, STEPS, 0, STEPS, T.MIDPOINT), EINVAL),  # midpoint has 2 x 4 stages
        ("n_stage_scale", (eight, 2 * STEPS, 0, STEPS, T.EULER), EINVAL),
        ("n_stage_scale", (ones, STEPS, 1, STEPS, T.EULER), EINVAL),  # the CALL's own stages: 3
        ("n_stage_scale", (None, STEPS, 0, STEPS, T.EULER), EINVAL),
        ("finite", (nan, STEPS, 0, STEPS, T.EULER), EINVAL),
        ("finite", (inf, STEPS, 0, STEPS, T.EULER), EINVAL),
    ]
    for word, (scale, n, b, e, solver), code in bad:
        assert _gs_call(raw, kind, rows_buf, scale, n, b, e, solver, ws, nb) == code, (word, n, b, e, solver)
        assert word.encode() in L.rgfm_last_error(), L.rgfm_last_error()
        assert untouched()
    assert _gs_call(raw, kind, rows_buf, ones, STEPS, 0, STEPS, T.EULER, ws, nb - 1) == ENOMEM
    assert b"workspace" in L.rgfm_last_error() and untouched()
    # null state pointers
    args = list(raw.args)
    state_at = {"pair": 2, "cond": 1, "pair_grad": 3, "cond_grad": 2}[kind]
    args[state_at] = ctypes.c_void_p(0)
    fn = getattr(L, f"rgfm_sample_{kind}_gs")
    assert fn(*args, T._p(rows_buf), ones, STEPS, 0, STEPS, T.EULER, None, 0, T._p(ws), nb, T._stream()) == EINVAL
    assert b"null" in L.rgfm_last_error() and untouched()
    assert bool((ws == 0x5A).all())  # nothing was enqueued by any of the refused calls
    # a good call: the state moves, the bands behind gamma_rows and behind the workspace stay as they were
    assert _gs_call(raw, kind, rows_buf, ones, STEPS, 0, STEPS, T.EULER, ws, nb) == 0
    torch.cuda.synchronize()
    assert not untouched() and all(bool(torch.isfinite(s).all()) for s in raw.state)
    assert bool((rows_buf[B:] == MARK).all()) and torch.equal(rows_buf[:B], cycle(B, dev))
    assert bool((ws[nb:] == 0x5A).all())


def test_block_rows_argument_errors(dev):
    L = _lib.lib()
    inp, _ = R.case(6, 1, 1.0)  # (1, 1, 4, 4)
    d = _dev_inputs(dev, inp)
    v0 = d["vx"].clone()
    nb = ctypes.c_size_t()
    assert L.rgfm_guidance_workspace_bytes(1, 1, ctypes.byref(nb)) == 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    p = T._p
    head = (p(d["x"]), p(d["y"]), p(d["vx"]), p(d["vy"]), p(d["mx"]), p(d["my"]), p(d["r"]), 1, 1, 4, 4, 0.5)
    assert L.rgfm_guidance_apply_rows(*head, None, None, p(ws), nb.value, T._stream()) == EINVAL
    assert b"null" in L.rgfm_last_error()
    assert L.rgfm_guidance_apply_rows(*head, p(cycle(1, dev)), None, p(ws), nb.value - 1, T._stream()) == ENOMEM
    torch.cuda.synchronize()
    assert torch.equal(d["vx"], v0)
    with pytest.raises(ValueError, match="gamma"):
        _engine.guidance_apply(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"], d["r"], 0.5, torch.ones(2, device=dev))


# ------------------------------------------------------------------ 8. the Python surface
def _small_models(dev):
    return T.net("g16").to(dev), T.net("g24").to(dev), T.flex().to(dev)


def _shape(n):
    return (n.in_channels, n.img_size, n.img_size)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("method", ["mc_feng", "grad_log_ratio"])
def test_paired_sampler_is_the_direct_engine_calls(dev, method, solver):
    from ratio_guided_multimodal_fm_amd.synth import paired_noise
    from ratio_guided_multimodal_fm_amd.utils.diagnostics import GuidanceDiagnostics
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler
    fx, fy, rr = _small_models(dev)
    B, N, steps = 5, 5, 4
    noise = paired_noise(41, B, N, _shape(fx), _shape(fy))
    gam = [0.0, 0.5, 1.0, 2.0, -0.5]
    sched = GuidanceSchedule.window(0.25, 0.6)
    diag = GuidanceDiagnostics()
    xs, ys = paired_sampler(fx, fy, rr, method, gam, B, steps, dev, N, _shape(fx), _shape(fy), noise=noise, verbose=False,
                            solver=solver, guidance_schedule=sched, diagnostics=diag)
    x, y = noise[0].to(dev).clone(), noise[1].to(dev).clone()
    rows, scale = torch.tensor(gam, device=dev), sched.stage_values(steps, solver)
    if method == "mc_feng":
        mx, my = noise[2].to(dev).clone(), noise[3].to(dev).clone()
        _engine.sample_two_streams(fx, mx, fy, my, steps, solver=solver)
        r = rr._engine.eval(mx, my, "ratio")
        _engine.sample_pair(fx, fy, x, y, mx, my, r, steps, 0.0, solver=solver, gamma_rows=rows, stage_scale=scale)
    else:
        _engine.sample_pair_grad(fx, fy, rr, x, y, steps, 0.0, solver=solver, gamma_rows=rows, stage_scale=scale)
    assert torch.equal(xs, x) and torch.equal(ys, y)
    off = torch.tensor([v == 0.0 for v in scale])
    assert bool(off.any()) and not bool(diag.guided[off].any()) and not bool(diag.records[off.to(dev)].any())
    # a tensor strength, a callable schedule; and the default keeps today's bits
    a = paired_sampler(fx, fy, rr, method, torch.tensor(gam), B, steps, dev, N, _shape(fx), _shape(fy), noise=noise,
                       verbose=False, solver=solver, guidance_schedule=lambda t: 1.0 if 0.25 <= t <= 0.6 else 0.0)
    assert torch.equal(a[0], xs) and torch.equal(a[1], ys)
    p = paired_sampler(fx, fy, rr, method, 0.5, B, steps, dev, N, _shape(fx), _shape(fy), noise=noise, verbose=False, solver=solver)
    q = paired_sampler(fx, fy, rr, method, [0.5] * B, B, steps, dev, N, _shape(fx), _shape(fy), noise=noise, verbose=False,
                       solver=solver, guidance_schedule=GuidanceSchedule.constant())
    assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])


@pytest.mark.parametrize("method", ["mc_feng", "grad_log_ratio"])
def test_sample_conditional_is_the_direct_engine_calls(dev, method):
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional
    fx, fy, rr = _small_models(dev)
    B, N, steps = 3, 5, 4
    cond = T.start("g24", B, salt=2).to(dev)
    gam, sched = [0.3, 1.0, 2.0], GuidanceSchedule.cosine()
    torch.manual_seed(77)
    got = sample_conditional(fx, rr, cond, "y", steps, gam, N, guidance_method=method, guidance_schedule=sched)
    torch.manual_seed(77)
    rows, scale = torch.tensor(gam, device=dev), sched.stage_values(steps)
    if method == "mc_feng":
        mc = torch.randn(N, *_shape(fx), device=dev)
        _engine.sample_single(fx, mc, steps)
        s = torch.randn(B, *_shape(fx), device=dev)
        ratios = rr.cross_log_ratio(mc, cond).exp().T.contiguous()
        _engine.sample_cond(fx, s, mc, ratios, steps, 0.0, gamma_rows=rows, stage_scale=scale)
    else:
        s = torch.randn(B, *_shape(fx), device=dev)
        ctx = rr._engine.cond_prepare(cond, "y", _shape(fx))
        _engine.sample_cond_grad(fx, rr, s, ctx, "y", steps, 0.0, gamma_rows=rows, stage_scale=scale)
    assert torch.equal(got, s)


def _checkpoints(tmp_path):
    from helpers import make_module
    ck = tmp_path / "checkpoints"
    ck.mkdir()
    fm, fs, rr = make_module("mnist32"), make_module("svhn"), make_module("ratio_ms")
    torch.save({"epoch": 1, "model_state_dict": fm.state_dict(), "best_loss": 0.5}, ck / "flow_mnist32_best.pth")
    torch.save({"epoch": 1, "model_state_dict": fs.state_dict(), "best_loss": 0.5}, ck / "flow_svhn_best.pth")
    torch.save(rr.state_dict(), ck / "ratio_disc_mnist_svhn_best.pth")
    return fm, fs, rr


def test_cli_window_is_the_sampler_call(dev, tmp_path, monkeypatch, capsys):
    from ratio_guided_multimodal_fm_amd import sample_mnist_svhn
    from ratio_guided_multimodal_fm_amd.utils import set_seed
    fm, fs, rr = _checkpoints(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--guidance_method", "mc_feng", "--guidance_strength", "0.5", "--num_steps", "4", "--num_samples", "3",
            "--mc_batch_size", "5", "--seed", "9"]
    assert sample_mnist_svhn.main(argv + ["--guidance_window", "0.2", "0.6", "--diagnostics"]) == 0
    assert "Diagnostics" in capsys.readouterr().out
    got = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_mc_feng_gamma0.5.pt")
    set_seed(9)
    xs, ys = sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(fm.to(dev), fs.to(dev), rr.to(dev), "mc_feng", 0.5, 3, 4, dev, 5,
                                                                guidance_schedule=GuidanceSchedule.window(0.2, 0.6))
    assert torch.equal(got["mnist"], xs.cpu()) and torch.equal(got["svhn"], ys.cpu())
    assert sample_mnist_svhn.main(argv) == 0
    plain = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_mc_feng_gamma0.5.pt")
    assert not torch.equal(plain["mnist"], got["mnist"])
    capsys.readouterr()


def test_shared_mc_sweep_is_three_engine_calls_on_one_mc_set(dev, monkeypatch, capsys):
    from helpers import make_module
    from ratio_guided_multimodal_fm_amd import evaluate_mnist_svhn
    fm, fs, rr = make_module("mnist32", dev), make_module("svhn", dev), make_module("ratio_ms", dev)
    cm, cs = make_module("clf_mnist", dev), make_module("clf_svhn", dev)
    strengths, n, N, steps = [0.0, 0.5, 2.0], 5, 5, 2
    kept, draws = [], []
    real_eval, real_randn = evaluate_mnist_svhn.evaluate_coherence, torch.randn
    monkeypatch.setattr(evaluate_mnist_svhn, "evaluate_coherence", lambda xs, ys, *a: (kept.append((xs.clone(), ys.clone())), real_eval(xs, ys, *a))[1])
    monkeypatch.setattr(torch, "randn", lambda *a, **k: (draws.append(tuple(a)), real_randn(*a, **k))[1])
    torch.manual_seed(123)
    res = evaluate_mnist_svhn.run_sweep(fm, fs, lambda: rr, cm, cs, ["mc_feng"], strengths, n, steps, dev, N, shared_mc=True)
    monkeypatch.undo()
    capsys.readouterr()
    # the noise is drawn once, in the order of one ordinary call
    assert draws == [(n, 1, 32, 32), (n, 3, 32, 32), (N, 1, 32, 32), (N, 3, 32, 32)]
    assert [r["guidance_strength"] for r in res] == strengths and all(r["shared_mc"] is True and r["num_samples"] == n for r in res)
    json.dumps(res)
    torch.manual_seed(123)
    x0, y0 = torch.randn(n, 1, 32, 32, device=dev), torch.randn(n, 3, 32, 32, device=dev)
    mx, my = torch.randn(N, 1, 32, 32, device=dev), torch.randn(N, 3, 32, 32, device=dev)
    _engine.sample_two_streams(fm, mx, fs, my, steps)
    r = rr._engine.eval(mx, my, "ratio")
    for (xs, ys), gamma in zip(kept, strengths):
        x, y = x0.clone(), y0.clone()
        _engine.sample_pair(fm, fs, x, y, mx, my, r, steps, gamma)
        assert torch.equal(xs, x) and torch.equal(ys, y), gamma
    assert not torch.equal(kept[0][0], kept[2][0])
