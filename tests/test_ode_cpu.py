"""The ODE solver choice without a GPU: the C ABI's new entry points are declared, bound and exported; the float64
loops of tests/ode_ref64.py are the existing Euler references under solver='euler' and show second-order truncation
under solver='midpoint'; an unknown solver name is a ValueError on every Python entry point before any device work.

Truncation table re-measured by test_midpoint_truncation_order (float64, g16, first 3 rows of its fixture input,
unguided, max |s - s_ref| with s_ref = 64 midpoint steps): printed by the test, recorded in DESIGN.md.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cond_grad_ref64 as CG
import cond_ref64 as C
import ode_ref64 as O
from ratio_guided_multimodal_fm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPS = ("single", "pair", "cond", "pair_grad", "cond_grad")
NEW = [f"rgfm_sample_{k}_ode{suffix}" for k in LOOPS for suffix in ("", "_workspace_bytes")]


def test_header_bindings_and_library_list_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    assert re.search(r"#define\s+RGFM_SOLVER_EULER\s+0\b", header) and re.search(r"#define\s+RGFM_SOLVER_MIDPOINT\s+1\b", header)
    assert re.search(r"#define\s+RGFM_ABI_VERSION\s+3\b", header) and _lib.ABI_VERSION == 3
    assert _lib.SOLVERS == {"euler": 0, "midpoint": 1}
    assert len(NEW) == 10
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    # each *_ode signature is the Euler one with one int (the solver) in front of ws / bytes
    for k in LOOPS:
        old, new = _lib.SIGNATURES[f"rgfm_sample_{k}"][1], _lib.SIGNATURES[f"rgfm_sample_{k}_ode"][1]
        assert new == old[:-3] + [ctypes.c_int] + old[-3:], k
        old, new = _lib.SIGNATURES[f"rgfm_sample_{k}_workspace_bytes"][1], _lib.SIGNATURES[f"rgfm_sample_{k}_ode_workspace_bytes"][1]
        assert new == old[:-1] + [ctypes.c_int] + old[-1:], k


def test_midpoint_truncation_order():
    ref = O.g16_unguided("midpoint", 64)
    err = lambda solver, n: float(np.abs(O.g16_unguided(solver, n) - ref).max())
    e16, m8 = err("euler", 16), err("midpoint", 8)
    print(f"g16 float64, max|s_ref| {np.abs(ref).max():.3f}: euler N=4 {err('euler', 4):.3e}  N=8 {err('euler', 8):.3e}  N=16 {e16:.3e}  "
          f"N=32 {err('euler', 32):.3e} | midpoint N=4 {err('midpoint', 4):.3e}  N=8 {m8:.3e}  N=16 {err('midpoint', 16):.3e}")
    assert 4.0 * m8 <= e16, (m8, e16)
    # the fixture tests/test_gpu_ode.py reads instead of recomputing the 64-step reference
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "ode_g16_midpoint64.npz"))["s"]
    assert fixture.dtype == np.float64 and float(np.abs(fixture - ref).max()) <= 1e-12
    gap = float(np.abs(O.g16_unguided("midpoint", 4) - O.g16_unguided("euler", 4)).max())
    print(f"max |midpoint N=4 - euler N=4| {gap:.3e}")
    assert gap > 1e-2, gap


def test_euler_loops_are_the_existing_references():
    # the one-sided MC loop against cond_ref64.sample_cond64
    net, x0 = O.g16_case()
    vel = O.velocity_of(net)
    g = np.random.default_rng(5)
    m, R = 0.5 * g.standard_normal((7, 256)), np.exp(0.5 * g.standard_normal((3, 7)))
    want = C.sample_cond64(vel, x0, m, R, 4, 0.7)
    got = O.integrate64(O.F_cond_mc(vel, m, R, 0.7), (x0,), 4, "euler")[0]
    assert float(np.abs(got - want).max()) <= 1e-13
    # splitting at a step boundary, both solvers
    for solver in O.SOLVERS:
        whole = O.integrate64(O.F_cond_mc(vel, m, R, 0.7), (x0,), 4, solver)[0]
        half = O.integrate64(O.F_cond_mc(vel, m, R, 0.7), (x0,), 4, solver, 0, 2)
        assert np.array_equal(O.integrate64(O.F_cond_mc(vel, m, R, 0.7), half, 4, solver, 2, 4)[0], whole)
    # the one-sided gradient loop against cond_grad_ref64's
    rr, tnet, cond, s0 = CG.sampler_case("x")
    want = CG.sampler_loop64("x", CG.GAMMA_S).numpy()
    got = O.integrate64(O.F_cond_grad(O.velocity_of(tnet), rr, cond, "x", CG.GAMMA_S), (s0.numpy(),), CG.STEPS_S, "euler")[0]
    assert float(np.abs(got - want).max()) <= 1e-13
    with pytest.raises(ValueError):
        O.integrate64(O.F_single(vel), (x0,), 4, "heun")


class _Net:  # stands in for a module: the solver name is checked before anything touches it
    pass


def test_unknown_solver_is_a_value_error_before_any_device_work():
    from ratio_guided_multimodal_fm_amd import _engine, distributed, evaluate, evaluate_mnist_svhn, sample_mnist_svhn
    from ratio_guided_multimodal_fm_amd.utils import flow_utils as FU
    n, x = _Net(), torch.zeros(1, 1, 28, 28)
    calls = [
        lambda: FU.CFMSchedule().sample(n, 1, 2, "cuda", solver="bogus"),
        lambda: FU.paired_sampler(n, n, None, "none", 0.0, 1, 2, "cuda", 0, (1, 28, 28), (1, 28, 28), solver="bogus"),
        lambda: FU.sample_bimodal_guided(n, n, solver="bogus"),
        lambda: sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(n, n, solver="bogus"),
        lambda: FU.sample_conditional(n, n, x, "x", solver="bogus"),
        lambda: FU.sample_conditional(n, n, x, "x", guidance_method="grad_log_ratio", solver="bogus"),
        lambda: evaluate_mnist_svhn.evaluate_conditional_coherence(x, None, "mnist", n, n, "cuda", fm_target=n, ratio_estimator=n, solver="bogus"),
        lambda: evaluate.run_sweep(n, n, lambda: None, n, ["none"], [0.0], 1, 2, "cuda", 0, "rotate90", solver="bogus"),
        lambda: evaluate_mnist_svhn.run_sweep(n, n, lambda: None, n, n, ["none"], [0.0], 1, 2, "cuda", 0, solver="bogus"),
        lambda: distributed.sharded_paired_sampler(n, n, None, "none", 0.0, 2, (x, x, None, None), "cpu", solver="bogus"),
        lambda: _engine.sample_single(n, x, 2, solver="bogus"),
        lambda: _engine.sample_two_streams(n, x, n, x, 2, solver="bogus"),
        lambda: _engine.sample_pair(n, n, x, x, None, None, None, 2, 0.0, solver="bogus"),
        lambda: _engine.sample_pair_grad(n, n, n, x, x, 2, 0.0, solver="bogus"),
        lambda: _engine.sample_cond(n, x, x, x, 2, 0.0, solver="bogus"),
        lambda: _engine.sample_cond_grad(n, n, x, x, "x", 2, 0.0, solver="bogus"),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="solver"):
            call()
    for bad in (None, 1, "Midpoint"):
        with pytest.raises(ValueError):
            _lib.solver_id(bad)
    for mod in (sample_mnist_svhn, evaluate_mnist_svhn):  # the CLIs: argparse rejects it
        with pytest.raises(SystemExit):
            mod.main(["--solver", "bogus"])
