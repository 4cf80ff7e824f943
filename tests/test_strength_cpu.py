"""Guidance strength per sample and per stage, without a GPU: the float64 yardstick (tests/strength_ref64.py) against the
pinned loops of ode_ref64, GuidanceSchedule against closed forms, the eight new exports, and the argument checks of
every Python entry point, all of which run before any device work."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import ode_ref64 as O
import strength_ref64 as S
from helpers import make_generic_unet, make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd.utils.diagnostics import stage_times
from ratio_guided_multimodal_fm_amd.utils.guidance_schedule import GuidanceSchedule, as_schedule, from_cli, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPS = ("rgfm_sample_pair_gs", "rgfm_sample_pair_cross_gs", "rgfm_sample_cond_gs", "rgfm_sample_pair_grad_gs",
         "rgfm_sample_cond_grad_gs")
BLOCKS = ("rgfm_guidance_apply_rows", "rgfm_guidance_apply_cond_rows", "rgfm_guidance_apply_cross_rows")


# ------------------------------------------------------------------ the float64 yardstick
@functools.lru_cache(maxsize=None)
def g16():
    return make_generic_unet("g16")[0]


@functools.lru_cache(maxsize=None)
def case(B=3, N=5):
    g = torch.Generator().manual_seed(9100)
    f = lambda *s: torch.randn(*s, generator=g).numpy().astype(np.float64)
    x, y = f(B, 1, 16, 16), f(B, 1, 16, 16)
    mx, my = 0.5 * f(N, 256), 0.5 * f(N, 256)
    r, R = np.exp(0.5 * f(N)), np.exp(0.5 * f(B, N))
    return x, y, mx, my, r, R


@pytest.mark.parametrize("solver", O.SOLVERS)
def test_constant_schedule_and_equal_rows_are_the_existing_loops(solver):
    x, y, mx, my, r, R = case()
    vel = O.velocity_of(g16())
    gamma, steps = 0.75, 2  # (0.75 is an fp32 number: float64(float32(gamma)) == gamma)
    want = O.integrate64(O.F_pair_mc(vel, vel, mx, my, r, gamma), (x, y), steps, solver)
    for sched in (None, GuidanceSchedule.constant()):
        got = S.integrate_rows64(*S.pair_mc(vel, vel, mx, my, r), (x, y), [gamma] * len(x), steps, solver, sched)
        err = max(float(np.abs(a - b).max()) for a, b in zip(got, want))
        print(f"pair_mc {solver} schedule={sched}: |rows - batch| {err:.3e}")
        assert err <= 1e-13
    want = O.integrate64(O.F_cond_mc(vel, mx, R, gamma), (x,), steps, solver)[0]
    got = S.integrate_rows64(*S.cond_mc(vel, mx, R), (x,), [gamma] * len(x), steps, solver, GuidanceSchedule.constant())[0]
    assert float(np.abs(got - want).max()) <= 1e-13


def test_a_zero_scale_is_the_unguided_loop_and_a_window_is_three_legs():
    x, y, mx, my, r, _ = case()
    vel = O.velocity_of(g16())
    mk = S.pair_mc(vel, vel, mx, my, r)
    steps, gam = 4, [0.5, 1.0, 2.0]
    off = S.integrate_rows64(*mk, (x, y), gam, steps, "euler", GuidanceSchedule.from_values([0.0] * steps))
    plain = O.integrate64(O.F_pair_mc(vel, vel, None, None, None, 0.0), (x, y), steps, "euler")
    assert max(float(np.abs(a - b).max()) for a, b in zip(off, plain)) <= 1e-13
    # s = 1 on steps [1, 3): unguided [0, 1), guided [1, 3), unguided [3, 4), chained
    win = S.integrate_rows64(*mk, (x, y), gam, steps, "euler", GuidanceSchedule.from_values([0.0, 1.0, 1.0, 0.0]))
    leg = O.integrate64(O.F_pair_mc(vel, vel, None, None, None, 0.0), (x, y), steps, "euler", 0, 1)
    leg = S.integrate_rows64(*mk, leg, gam, steps, "euler", None, 1, 3)
    leg = O.integrate64(O.F_pair_mc(vel, vel, None, None, None, 0.0), leg, steps, "euler", 3, 4)
    assert max(float(np.abs(a - b).max()) for a, b in zip(win, leg)) <= 1e-13
    assert max(float(np.abs(a - b).max()) for a, b in zip(win, plain)) > 1e-3  # (the window is not nothing)


def test_rows_carry_their_own_strength():
    """Row b of a mixed call is row b of the scalar loop at gamma_b (float32, widened), and gamma_b * s(t) per stage."""
    x, y, mx, my, r, _ = case()
    vel = O.velocity_of(g16())
    gam = [0.0, 0.3, 2.0]
    got = S.integrate_rows64(*S.pair_mc(vel, vel, mx, my, r), (x, y), gam, 2, "midpoint", GuidanceSchedule.linear())
    s_of = S.scale_by_time(GuidanceSchedule.linear(), 2, "midpoint")
    for b, g in enumerate(gam):
        g64 = float(np.float32(g))

        def F(s, t, g64=g64):
            return O.F_pair_mc(vel, vel, mx, my, r, g64 * s_of[t])(s, t)
        want = O.integrate64(F, (x[b:b + 1], y[b:b + 1]), 2, "midpoint")
        assert max(float(np.abs(a[b:b + 1] - w).max()) for a, w in zip(got, want)) <= 1e-13


# ------------------------------------------------------------------ GuidanceSchedule
@pytest.mark.parametrize("solver", ["euler", "midpoint"])
@pytest.mark.parametrize("rng", [(0, None), (2, 5), (7, 7)])
def test_stage_values_against_closed_forms(solver, rng):
    n, (b, e) = 7, rng
    ts = stage_times(n, solver, b, e)
    assert len(ts) == ((n if e is None else e) - b) * (2 if solver == "midpoint" else 1)
    sv = lambda s: s.stage_values(n, solver, b, e)
    assert sv(GuidanceSchedule.constant()) == [1.0] * len(ts)
    assert sv(GuidanceSchedule.linear()) == [1.0 + (0.0 - 1.0) * t for t in ts]
    assert sv(GuidanceSchedule.linear(2.0, 0.5)) == [2.0 + (0.5 - 2.0) * t for t in ts]
    got = sv(GuidanceSchedule.cosine(1.5, 0.25))
    assert got == pytest.approx([0.25 + 1.25 * 0.5 * (1 + math.cos(math.pi * t)) for t in ts], abs=1e-15)
    assert sv(GuidanceSchedule.window(0.2, 0.8)) == [1.0 if 0.2 <= t <= 0.8 else 0.0 for t in ts]
    assert sv(GuidanceSchedule.from_callable(lambda t: t * t)) == [t * t for t in ts]
    assert sv(as_schedule(lambda t: 3 * t)) == [3 * t for t in ts]
    vals = [0.1 * k for k in range(len(ts))]
    assert sv(GuidanceSchedule.from_values(vals)) == vals and sv(as_schedule(torch.tensor(vals, dtype=torch.float64))) == vals
    assert all(type(v) is float for v in got)


def test_schedule_ends_window_edges_and_wrong_lengths():
    assert GuidanceSchedule.cosine().stage_values(4)[0] == 1.0 and GuidanceSchedule.linear().stage_values(4)[0] == 1.0
    assert GuidanceSchedule.cosine(1.0, 0.0)._fn(1.0) == pytest.approx(0.0, abs=1e-16)
    # the edges are inclusive: the stage times 0.25 and 0.75 themselves are guided
    assert GuidanceSchedule.window(0.25, 0.75).stage_values(4) == [0.0, 1.0, 1.0, 1.0]
    assert GuidanceSchedule.window(0.25, 0.75).stage_values(4, "midpoint") == [0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0]
    assert GuidanceSchedule.window(0.5, 0.5).stage_values(4) == [0.0, 0.0, 1.0, 0.0]
    with pytest.raises(ValueError, match="t_lo"):
        GuidanceSchedule.window(0.8, 0.2)
    for n, solver in ((3, "euler"), (5, "euler"), (4, "midpoint")):
        with pytest.raises(ValueError, match="stages"):
            GuidanceSchedule.from_values([1.0] * 4).stage_values(n, solver)
    assert GuidanceSchedule.from_values([1.0] * 4).stage_values(2, "midpoint") == [1.0] * 4
    assert GuidanceSchedule.from_values([1.0, 0.0]).stage_values(6, "euler", 2, 4) == [1.0, 0.0]
    with pytest.raises(TypeError):
        as_schedule("linear")
    with pytest.raises(TypeError):
        GuidanceSchedule.from_callable(3.0)
    assert as_schedule(None) is None


def test_cli_flags_make_the_schedule():
    import argparse
    from ratio_guided_multimodal_fm_amd.utils.guidance_schedule import add_cli_args
    p = argparse.ArgumentParser()
    add_cli_args(p)
    ts = stage_times(5)
    assert from_cli(p.parse_args([])) is None
    assert from_cli(p.parse_args(["--guidance_schedule", "linear"])).stage_values(5) == [1.0 - t for t in ts]
    assert from_cli(p.parse_args(["--guidance_window", "0.2", "0.7"])).stage_values(5) == [0.0, 1.0, 1.0, 1.0, 0.0]
    both = from_cli(p.parse_args(["--guidance_schedule", "linear", "--guidance_window", "0.2", "0.7"])).stage_values(5)
    assert both == [0.0, 1.0 - ts[1], 1.0 - ts[2], 1.0 - ts[3], 0.0]
    with pytest.raises(SystemExit):
        p.parse_args(["--guidance_schedule", "quadratic"])


# ------------------------------------------------------------------ the C ABI
def _args_of(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_bindings_and_library_list_the_eight_exports():
    header = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    assert re.search(r"#define\s+RGFM_ABI_VERSION\s+3\b", header) and _lib.ABI_VERSION == 3
    assert _lib.SOLVERS == {"euler": 0, "midpoint": 1}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    SIG = _lib.SIGNATURES
    for name in LOOPS + BLOCKS:
        assert name in SIG and hasattr(handle, name), name
    extra = ["const float* gamma_rows", "const double* stage_scale", "int n_stage_scale"]
    extra_t = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    for name in LOOPS:
        base = "rgfm_sample_pair_cross" if name == "rgfm_sample_pair_cross_gs" else name[:-3] + "_diag"
        old, new = _args_of(header, base), _args_of(header, name)
        k = old.index("double gamma") + 1  # the three arguments sit right behind gamma
        assert new == old[:k] + extra + old[k:], name
        assert SIG[name][1] == SIG[base][1][:k] + extra_t + SIG[base][1][k:], name
        assert SIG[name][1][k - 1] is ctypes.c_double
    for name in BLOCKS:
        base = name[:-5]
        old, new = _args_of(header, base), _args_of(header, name)
        k = old.index("double gamma")  # gamma_rows in gamma's place
        assert new == old[:k] + ["const float* gamma_rows"] + old[k + 1:], name
        assert SIG[name][1] == SIG[base][1][:k] + [ctypes.c_void_p] + SIG[base][1][k + 1:], name


def test_native_argument_errors_need_no_device():
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    assert L.rgfm_guidance_apply_rows(*[null] * 7, 3, 7, 4, 4, 0.5, null, null, null, 0, null) == -1
    assert L.rgfm_guidance_apply_cond_rows(*[null] * 4, 3, 7, 4, 0.5, null, null, null, 0, null) == -1
    assert L.rgfm_guidance_apply_cross_rows(*[null] * 7, 3, 7, 4, 4, 0.5, null, null, null, null, 0, null) == -1
    one = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    assert L.rgfm_sample_pair_gs(*[null] * 7, 7, 3, 4, 0.5, null, one, 4, 0, 4, 0, null, 0, null, 0, null) == -1
    assert L.rgfm_sample_pair_cross_gs(*[null] * 7, 7, 3, 4, 0.5, null, one, 4, 0, 4, 0, null, 0, null, 0, null) == -1
    assert L.rgfm_sample_cond_gs(*[null] * 4, 7, 3, 4, 0.5, null, one, 4, 0, 4, 0, null, 0, null, 0, null) == -1
    assert L.rgfm_sample_pair_grad_gs(*[null] * 5, 3, 4, 0.5, null, one, 4, 0, 4, 0, null, 0, null, 0, null) == -1
    assert L.rgfm_sample_cond_grad_gs(*[null] * 4, 0, 3, 4, 0.5, null, one, 4, 0, 4, 0, null, 0, null, 0, null) == -1
    assert L.rgfm_last_error()


# ------------------------------------------------------------------ the Python surface: checks before any device work
def test_resolve_strength_and_schedule():
    g, vec, scale = resolve(0.7, None, 5, 4, "euler")
    assert g == 0.7 and vec is None and scale is None
    g, vec, scale = resolve([0.0, 0.5, 1.0], GuidanceSchedule.linear(), 3, 2, "midpoint")
    assert vec.dtype == torch.float32 and vec.tolist() == [0.0, 0.5, 1.0] and scale == [1.0, 0.75, 0.5, 0.25]
    assert resolve(torch.tensor([1.0, 2.0], dtype=torch.float64), None, 2, 4, "euler")[1].dtype == torch.float32
    for bad in ([0.5] * 4, torch.ones(2), torch.ones(3, 1), torch.ones(1, 3), [[0.5] * 3]):
        with pytest.raises(ValueError, match="guidance_strength"):
            resolve(bad, None, 3, 4, "euler")
    with pytest.raises(ValueError, match="guidance_strength"):
        resolve(torch.ones(3, dtype=torch.complex64), None, 3, 4, "euler")


def test_python_entry_points_check_strength_and_schedule_before_any_device_work():
    """No HIP device is in sight here: whatever is wrong with the strength or the schedule is reported before the device
    is asked for; a well-formed call reaches the device check ('no CPU path')."""
    from ratio_guided_multimodal_fm_amd.distributed import make_sharded_sampler
    from ratio_guided_multimodal_fm_amd.sample_mnist_svhn import sample_bimodal_guided_mnist_svhn
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler, sample_bimodal_guided, sample_conditional
    fx, fy, rr = make_module("unet28"), make_module("unet28_y"), make_module("ratio28")
    ms = (make_module("mnist32"), make_module("svhn"), make_module("ratio_ms"))
    calls = [
        lambda **kw: paired_sampler(fx, fy, rr, "mc_feng", kw.pop("g", 1.0), 3, 4, "cpu", 3, (1, 28, 28), (1, 28, 28), **kw),
        lambda **kw: sample_bimodal_guided(fx, fy, rr, "mc_feng", kw.pop("g", 1.0), 3, 4, "cpu", 3, **kw),
        lambda **kw: sample_bimodal_guided(fx, fy, rr, "grad_log_ratio", kw.pop("g", 1.0), 3, 4, "cpu", 3, **kw),
        lambda **kw: sample_bimodal_guided_mnist_svhn(*ms, "mc_feng", kw.pop("g", 1.0), 3, 4, "cpu", 3, **kw),
        lambda **kw: sample_conditional(ms[1], ms[2], torch.zeros(3, 1, 32, 32), "x", 4, kw.pop("g", 1.0), 3, device="cpu", **kw),
        lambda **kw: sample_conditional(ms[1], ms[2], torch.zeros(3, 1, 32, 32), "x", 4, kw.pop("g", 1.0), 3, device="cpu",
                                        guidance_method="grad_log_ratio", **kw),
    ]
    for call in calls:
        for bad in ([0.5, 1.0], torch.ones(4), torch.ones(3, 1), torch.ones(1, 3)):  # wrong length, 2-D
            with pytest.raises(ValueError, match="guidance_strength"):
                call(g=bad)
        with pytest.raises(ValueError, match="stages"):
            call(guidance_schedule=[1.0] * 3)
        with pytest.raises(ValueError, match="stages"):
            call(guidance_schedule=GuidanceSchedule.from_values([1.0] * 4), solver="midpoint")
        with pytest.raises(TypeError, match="guidance_schedule"):
            call(guidance_schedule="linear")
        for kw in ({}, {"g": [0.0, 0.5, 1.0]}, {"guidance_schedule": GuidanceSchedule.window(0.2, 0.8)},
                   {"g": torch.tensor([0.0, 0.5, 1.0]), "guidance_schedule": lambda t: 1 - t, "solver": "midpoint"}):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(**kw)
    # FlowMatchingModel pairs and sharded launches take a scalar strength only
    ox, oy = make_module("fm_original"), make_module("fm_original_y")
    for kw in ({"guidance_schedule": GuidanceSchedule.linear()}, {"guidance_strength": [0.5, 1.0]}):
        with pytest.raises(_lib.RgfmError, match="U-Net"):
            sample_bimodal_guided(ox, oy, rr, "mc_feng", num_samples=2, num_steps=4, device="cpu", mc_batch_size=3,
                                  **{"guidance_strength": 1.0, **kw})
    sharded = make_sharded_sampler((1, 28, 28), (1, 28, 28))
    with pytest.raises(_lib.RgfmError, match="sharded"):
        sharded(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 3, guidance_schedule=GuidanceSchedule.linear())
    with pytest.raises(_lib.RgfmError, match="sharded"):
        sharded(fx, fy, rr, "mc_feng", [1.0, 0.5], 2, 4, "cpu", 3)


def test_engine_calls_check_gamma_rows_and_stage_scale_first():
    fx, fy = make_module("unet28"), make_module("unet28_y")
    x, y = torch.zeros(3, 1, 28, 28), torch.zeros(3, 1, 28, 28)
    chk = lambda rows, scale, sid=0, steps=(0, 4), models=(fx, fy): _engine._check_strength(rows, scale, 3, 4, steps, sid, models)
    assert chk(None, None) is None
    for bad in (torch.ones(4), torch.ones(3, 1), [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="gamma_rows"):
            chk(bad, None)
    with pytest.raises(ValueError, match="float32"):
        chk(torch.ones(3, dtype=torch.float64), None)
    for n, sid, steps in ((3, 0, (0, 4)), (4, 1, (0, 4)), (4, 0, (1, 4))):
        with pytest.raises(ValueError, match="stage_scale"):
            chk(None, [1.0] * n, sid, steps)
    rows, arr = chk(torch.ones(3), [1.0, 0.0] * 4, 1)
    assert arr.n == 8 and list(arr) == [1.0, 0.0] * 4 and rows.shape == (3,)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        chk(None, [1.0] * 4, models=(make_module("fm_original"), make_module("fm_original_y")))
    # ... and through the entry points: the checks come before the device check of the tensors
    with pytest.raises(ValueError, match="gamma_rows"):
        _engine.sample_pair(fx, fy, x, y, None, None, None, 4, 0.5, gamma_rows=torch.ones(2))
    with pytest.raises(ValueError, match="stage_scale"):
        _engine.sample_pair(fx, fy, x, y, None, None, None, 4, 0.5, stage_scale=[1.0] * 4, solver="midpoint")
    rr = make_module("ratio28")
    with pytest.raises(ValueError, match="stage_scale"):
        _engine.sample_pair_grad(fx, fy, rr, x, y, 4, 0.5, stage_scale=[1.0] * 5)
    with pytest.raises(ValueError, match="gamma_rows"):
        _engine.sample_cond(fx, x, x, torch.ones(3, 3), 4, 0.5, gamma_rows=torch.ones(3, 1))
    with pytest.raises(ValueError, match="stage_scale"):
        _engine.sample_cond_grad(fx, rr, x, torch.zeros(3, 4), "x", 4, 0.5, stage_scale=[1.0])


def test_the_default_path_passes_the_same_arguments_as_before(monkeypatch):
    """A float strength and no schedule: the samplers call _engine.sample_pair / sample_pair_grad / sample_cond /
    sample_cond_grad with the positional arguments and keywords they always did -- no gamma_rows, no stage_scale --
    and a vector strength / a schedule add exactly those two keywords."""
    from ratio_guided_multimodal_fm_amd.utils import flow_utils
    fx, fy, rr = make_module("unet28"), make_module("unet28_y"), make_module("ratio28")
    calls = []

    def spy(name, ret):
        def f(*a, **k):
            calls.append((name, a, dict(k)))
            return ret(a)
        return f
    cpu = torch.device("cpu")
    monkeypatch.setattr(flow_utils, "_device", lambda d: cpu)
    monkeypatch.setattr(flow_utils._engine, "sample_pair", spy("pair", lambda a: (a[2], a[3])))
    monkeypatch.setattr(flow_utils._engine, "sample_pair_grad", spy("pair_grad", lambda a: (a[3], a[4])))
    monkeypatch.setattr(flow_utils._engine, "sample_cond", spy("cond", lambda a: a[1]))
    monkeypatch.setattr(flow_utils._engine, "sample_cond_grad", spy("cond_grad", lambda a: a[2]))
    monkeypatch.setattr(flow_utils._engine, "sample_two_streams", lambda *a, **k: None)
    monkeypatch.setattr(flow_utils._engine, "sample_single", lambda m, x, *a, **k: x)
    monkeypatch.setattr(type(rr._engine), "eval", lambda self, x, y, what: torch.ones(x.shape[0]))
    monkeypatch.setattr(type(rr._engine), "cond_prepare", lambda self, c, given, shape: torch.zeros(c.shape[0], 4))
    monkeypatch.setattr(type(rr), "cross_log_ratio", lambda self, a, b: torch.zeros(a.shape[0], b.shape[0]))
    B, N, steps, gamma = 3, 5, 4, 0.7
    cond = torch.zeros(B, 1, 28, 28)
    run = {
        "pair": lambda **kw: flow_utils.sample_bimodal_guided(fx, fy, rr, "mc_feng", kw.pop("g", gamma), B, steps, "cuda", N, **kw),
        "pair_grad": lambda **kw: flow_utils.sample_bimodal_guided(fx, fy, rr, "grad_log_ratio", kw.pop("g", gamma), B, steps, "cuda", N, **kw),
        "cond": lambda **kw: flow_utils.sample_conditional(fy, rr, cond, "x", steps, kw.pop("g", gamma), N, device="cuda", **kw),
        "cond_grad": lambda **kw: flow_utils.sample_conditional(fy, rr, cond, "x", steps, kw.pop("g", gamma), N, device="cuda",
                                                                guidance_method="grad_log_ratio", **kw),
    }
    gpos = {"pair": 8, "pair_grad": 6, "cond": 5, "cond_grad": 6}
    for name, call in run.items():
        calls.clear()
        call()
        call(guidance_schedule=None)
        call(g=[0.0, 0.5, 1.0], guidance_schedule=GuidanceSchedule.window(0.25, 0.5))
        call(guidance_schedule=lambda t: 1.0 - t, solver="midpoint")
        assert [c[0] for c in calls] == [name] * 4
        (_, a0, k0), (_, a1, k1), (_, a2, k2), (_, a3, k3) = calls
        assert k0 == k1 == {"solver": "euler", "diag": None}, (name, k0)
        assert len(a0) == len(a1) == len(a2) == gpos[name] + 1 and a0[gpos[name]] == gamma and a0[gpos[name] - 1] == steps
        assert set(k2) == {"solver", "diag", "gamma_rows", "stage_scale"} and a2[gpos[name]] == 0.0
        assert k2["gamma_rows"].dtype == torch.float32 and k2["gamma_rows"].tolist() == [0.0, 0.5, 1.0]
        assert k2["stage_scale"] == [0.0, 1.0, 1.0, 0.0]
        assert set(k3) == {"solver", "diag", "stage_scale"} and a3[gpos[name]] == gamma
        assert k3["stage_scale"] == [1.0 - t for t in stage_times(steps, "midpoint")]


def test_schedule_flags_parse_on_all_four_clis(monkeypatch, tmp_path, capsys):
    from ratio_guided_multimodal_fm_amd import evaluate, evaluate_mnist_svhn, sample, sample_mnist_svhn

    def parses(module, argv):
        monkeypatch.chdir(tmp_path)
        try:
            return module.main(argv)
        except RuntimeError as e:
            assert "HIP device" in str(e) or "no CPU path" in str(e), e
            return 1
    for module in (sample, sample_mnist_svhn, evaluate, evaluate_mnist_svhn):
        for kind in ("constant", "linear", "cosine"):
            assert parses(module, ["--guidance_schedule", kind]) == 1
        assert parses(module, ["--guidance_window", "0.2", "0.8", "--diagnostics"]) == 1
        assert parses(module, ["--guidance_schedule", "cosine", "--guidance_window", "0.2", "0.8"]) == 1
        with pytest.raises(SystemExit):
            module.main(["--guidance_schedule", "step"])
        with pytest.raises(SystemExit):
            module.main(["--guidance_window", "0.2"])
    for module in (evaluate, evaluate_mnist_svhn):
        assert parses(module, ["--shared_mc"]) == 1
    with pytest.raises(SystemExit):
        evaluate_mnist_svhn.main(["--shared_mc", "--sharded"])
    with pytest.raises(SystemExit):
        sample_mnist_svhn.main(["--guidance_schedule", "linear", "--sharded"])
    with pytest.raises(SystemExit):
        sample.main(["--guidance_schedule", "linear", "--model", "original"])
    capsys.readouterr()


def test_sweep_rows_gain_shared_mc_only_with_the_flag(monkeypatch):
    from helpers import golden
    from ratio_guided_multimodal_fm_amd import evaluate_mnist_svhn
    g = golden("sampler_pair_ms")
    xs = torch.from_numpy(np.concatenate([g[f"c{i}_x"] for i in range(6)]))
    ys = torch.from_numpy(np.concatenate([g[f"c{i}_y"] for i in range(6)]))
    n = 4
    seen = []

    def shared(fm_x, fm_y, ratio, method, strengths, num_samples, *a, **kw):
        seen.append((method, list(strengths), num_samples))
        return [(xs[:num_samples], ys[:num_samples]) for _ in strengths]
    monkeypatch.setattr(evaluate_mnist_svhn, "shared_mc_sweep", shared)
    monkeypatch.setattr(evaluate_mnist_svhn, "sample_bimodal_guided_mnist_svhn", lambda *a, **kw: (xs[:n], ys[:n]))
    cm, cs = make_module("clf_mnist"), make_module("clf_svhn")
    base = {"method", "guidance_strength", "experiment", "coherence_acc", "num_samples"}
    sweep = lambda **kw: evaluate_mnist_svhn.run_sweep(None, None, lambda: object(), cm, cs, ["none", "mc_feng"], [0.0, 0.5, 2.0], n,
                                                       20, "cpu", 16, sampler=evaluate_mnist_svhn.sample_bimodal_guided_mnist_svhn, **kw)
    res = sweep(shared_mc=True)
    assert seen == [("mc_feng", [0.0, 0.5, 2.0], n)]  # ONE call for the three strengths
    assert [(r["method"], r["guidance_strength"]) for r in res] == [("none", 0.0), ("mc_feng", 0.0), ("mc_feng", 0.5), ("mc_feng", 2.0)]
    assert all(set(r) == base | {"shared_mc"} and r["shared_mc"] is True for r in res)
    for kw in ({}, {"shared_mc": False}):
        assert all(set(r) == base for r in sweep(**kw))
    with pytest.raises(ValueError, match="shared_mc"):
        evaluate_mnist_svhn.run_sweep(None, None, lambda: object(), cm, cs, ["mc_feng"], [0.5], n, 20, "cpu", 16,
                                      sampler=lambda *a, **kw: (xs[:n], ys[:n]), shared_mc=True)
