"""The effective-sample-size floor without a GPU: the float64 rule of tests/ess_ref64.py (the yardstick of
tests/test_gpu_ess.py) and the argument checks of the Python surface, which all run before any device work.

Rows.  `row(N, spread, seed)`: l ~ spread * N(0, 1) and log r ~ 0.5 N(0, 1): spread 5 is a moderately collapsed row,
spread 3e4 a late-time one (the log-weights of neighbouring samples differ by 1e4 to 1e5 at t = 0.99).
The bisection's answer: 40 halvings leave |hi - lo| = 2^-40, and the achieved ESS misses E* by at most that times
|d ESS / d tau|, which grows with the spread of d.  At spread 5 the 40 steps of the device reach E* to 1e-9; at the
late-time spread the float64 rule needs more steps for that figure (iters=80), which the test says aloud.
"""
import ctypes

import numpy as np
import pytest
import torch

import ess_cases  # noqa: F401  (registers the stream cases of the new exports: its docstring)
import ess_ref64 as E
import stream_cases
from helpers import make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd.utils.diagnostics import GuidanceDiagnostics


def row(N, spread, seed, zeros=0):
    g = np.random.default_rng(seed)
    l = spread * g.standard_normal(N) - 3.0 * spread
    r = np.exp(0.5 * g.standard_normal(N))
    if zeros:
        r[g.choice(N, zeros, replace=False)] = 0.0
    p = np.exp(l - l.max())
    w = (r / ((r * p).mean() + 1e-10)) * (p / (p.mean() + 1e-10))
    return l, r, w / (w.sum() + 1e-10)


@pytest.mark.parametrize("N,spread", [(2, 5.0), (7, 5.0), (64, 5.0), (257, 50.0), (1024, 3e4)])
def test_ess_of_tau_is_non_increasing_from_n_pos(N, spread):
    for seed in range(5):
        l, r, _ = row(N, spread, seed, zeros=N // 4)
        pos = r > 0
        L = l[pos] + np.log(r[pos])
        d = L - L.max()
        taus = np.concatenate([[0.0], np.geomspace(1e-7, 1.0, 200)])
        ess = np.array([E.ess_tau(d, t) for t in taus])
        assert ess[0] == pos.sum()
        assert (np.diff(ess) <= 1e-9 * ess[:-1]).all(), (N, spread, seed)
        assert 1.0 <= ess[-1] <= ess[0]


@pytest.mark.parametrize("N,spread,iters", [(7, 5.0, E.BISECT), (64, 5.0, E.BISECT), (256, 5.0, E.BISECT), (1024, 5.0, E.BISECT),
                                             (256, 3e4, 80), (1024, 3e4, 80)])
def test_bisection_reaches_the_target(N, spread, iters):
    worst = 0.0
    for seed in range(5):
        l, r, w = row(N, spread, 10 + seed)
        for ess_min in (1.5, 2.0, 4.0, min(8.0, N)):
            if E.ess_of(w) >= ess_min:
                continue
            out, tau = E.temper_row(l, r, w, ess_min, iters)
            assert 0.0 < tau < 1.0 and abs(out.sum() - 1.0) < 1e-12
            worst = max(worst, abs(float(E.ess_of(out)) - ess_min))
    print(f"N={N} spread={spread:g} iters={iters}: worst |ESS - E*| {worst:.3e}")
    assert 0.0 < worst <= 1e-9 or worst == 0.0, worst


def test_healthy_rows_are_returned_as_they_are():
    l, r, w = row(64, 0.3, 3)
    assert E.ess_of(w) > 8
    out, tau = E.temper_row(l, r, w, 8.0)
    assert tau == 1.0 and np.array_equal(out, w)


def test_masked_samples_stay_exactly_zero():
    for spread in (5.0, 3e4):
        l, r, w = row(64, spread, 4, zeros=20)
        # (the heaviest sample masked too: the maximum is taken over the unmasked ones)
        r[np.argmax(l)] = 0.0
        l2, r2, w2 = l, r, row_weights(l, r)
        out, tau = E.temper_row(l2, r2, w2, 6.0)
        assert tau < 1.0 and np.isfinite(out).all()
        assert (out[r2 == 0] == 0.0).all() and (out[r2 > 0] > 0.0).any()
        assert abs(float(E.ess_of(out)) - 6.0) < 1e-6


def row_weights(l, r):
    p = np.exp(l - l.max())
    w = (r / ((r * p).mean() + 1e-10)) * (p / (p.mean() + 1e-10))
    return w / (w.sum() + 1e-10)


def test_fewer_positive_ratios_than_the_floor_gives_uniform_weights_over_them():
    l, r, _ = row(32, 3e4, 5)
    r[3:] = 0.0  # n_pos = 3 < ess_min = 8: E* = 3 is reached at tau = 0 alone
    out, tau = E.temper_row(l, r, row_weights(l, r), 8.0)
    assert tau == 0.0
    assert np.array_equal(out[:3], np.full(3, 1.0 / 3.0)) and (out[3:] == 0.0).all()
    assert E.target_of(r, (1, 32), 8.0)[0] == 3.0
    # all ratios zero: the all-zero row of the block without a floor
    r[:] = 0.0
    w0 = row_weights(l, r)
    out, tau = E.temper_row(l, r, w0, 8.0)
    assert tau == 1.0 and not out.any()


def test_one_sample():
    out, tau = E.temper_row(np.array([-1e5]), np.array([0.7]), np.array([1.0]), 1.0)
    assert tau == 1.0 and out[0] == 1.0
    w, taus = E.temper(np.array([[-3.0]]), np.array([2.0]), np.array([[1.0]]), 1.0)
    assert taus[0] == 1.0 and w[0, 0] == 1.0


def test_batched_form_is_row_by_row_and_takes_both_ratio_layouts():
    rows = [row(33, 5.0, 20 + b) for b in range(4)]
    l, w = np.stack([a[0] for a in rows]), np.stack([a[2] for a in rows])
    R = np.stack([a[1] for a in rows])
    out, tau = E.temper(l, R, w, 4.0)
    for b in range(4):
        ob, tb = E.temper_row(l[b], R[b], w[b], 4.0)
        assert np.array_equal(out[b], ob) and tau[b] == tb
    w0 = np.stack([row_weights(l[b], R[0]) for b in range(4)])
    out, _ = E.temper(l, R[0], w0, 4.0)  # (one shared ratio vector)
    assert np.array_equal(out[2], E.temper_row(l[2], R[0], w0[2], 4.0)[0])


# ------------------------------------------------------------------ the Python surface: checks before any device work
def test_check_ess_values():
    u = make_module("unet28")
    assert _engine.check_ess(None, 8, (u,)) is None
    assert _engine.check_ess(4, 8, (u,)) == 4.0 and _engine.check_ess(8.0, 8, (u,)) == 8.0 and _engine.check_ess(1, 8, (u,)) == 1.0
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf"), 8.5):
        with pytest.raises(ValueError, match="ess_floor"):
            _engine.check_ess(bad, 8, (u,))
    with pytest.raises(_lib.RgfmError, match="cross"):
        _engine.check_ess(4, 8, (u,), cross=True)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        _engine.check_ess(4, 8, (make_module("fm_original"),))


def test_unsupported_combinations_raise_before_any_draw():
    from ratio_guided_multimodal_fm_amd.distributed import make_sharded_sampler, sharded_paired_sampler
    from ratio_guided_multimodal_fm_amd.evaluate import run_sweep
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import (paired_sampler, sample_bimodal_guided, sample_conditional,
                                                                 shared_mc_sweep)
    u, fm, fy, rr = make_module("unet28"), make_module("fm_original"), make_module("fm_original_y"), make_module("ratio28")
    state = torch.random.get_rng_state()  # (behind the modules: their constructors draw the initial weights)
    shapes = ((1, 28, 28), (1, 28, 28))
    with pytest.raises(_lib.RgfmError, match="cross"):
        paired_sampler(u, u, None, "mc_feng", 0.5, 2, 2, "cuda", 8, *shapes, mc_pairing="cross", ess_floor=4)
    with pytest.raises(_lib.RgfmError, match="no weights"):
        paired_sampler(u, u, None, "grad_log_ratio", 0.5, 2, 2, "cuda", 8, *shapes, ess_floor=4)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        sample_bimodal_guided(fm, fy, None, "mc_feng", 0.5, 2, 2, "cuda", 8, ess_floor=4)
    with pytest.raises(ValueError, match="ess_floor"):
        sample_bimodal_guided(u, u, None, "mc_feng", 0.5, 2, 2, "cuda", 8, ess_floor=9)
    with pytest.raises(ValueError, match="ess_floor"):
        sample_bimodal_guided(u, u, None, "mc_feng", 0.5, 2, 2, "cuda", 8, ess_floor=0.5)
    with pytest.raises(_lib.RgfmError, match="no weights"):
        shared_mc_sweep(u, u, object(), "grad_log_ratio", [0.5], 2, 2, "cuda", 8, *shapes, ess_floor=4)
    with pytest.raises(_lib.RgfmError, match="no weights"):
        sample_conditional(u, rr, torch.zeros(2, 1, 28, 28), "x", 2, 0.5, 8, guidance_method="grad_log_ratio",
                           ess_floor=4)
    with pytest.raises(ValueError, match="ess_floor"):
        sample_conditional(u, rr, torch.zeros(2, 1, 28, 28), "x", 2, 0.5, 8, ess_floor=9)
    with pytest.raises(_lib.RgfmError, match="sharded"):
        make_sharded_sampler(*shapes)(u, u, None, "mc_feng", 0.5, 2, 2, "cuda", 8, ess_floor=4)
    with pytest.raises(_lib.RgfmError, match="sharded"):
        sharded_paired_sampler(u, u, None, "mc_feng", 0.5, 2, (None,) * 4, "cuda", ess_floor=4)
    with pytest.raises(_lib.RgfmError, match="no weights"):
        run_sweep(u, u, lambda: None, None, ["mc_feng", "grad_log_ratio"], [0.5], 2, 2, "cuda", 8, "identity", ess_floor=4)
    with pytest.raises(_lib.RgfmError, match="sharded"):
        run_sweep(u, u, lambda: None, None, ["mc_feng"], [0.5], 2, 2, "cuda", 8, "identity", sampler=make_sharded_sampler(*shapes),
                  ess_floor=4)
    assert torch.equal(state, torch.random.get_rng_state())  # (nothing was drawn)


def test_cli_flag_and_diagnostics_field():
    import argparse
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import add_ess_arg, ess_from_cli
    p = argparse.ArgumentParser()
    add_ess_arg(p)
    assert ess_from_cli(p.parse_args([])) == {} and ess_from_cli(p.parse_args([]), sharded=True) == {}
    assert ess_from_cli(p.parse_args(["--ess_floor", "8"])) == {"ess_floor": 8.0}
    with pytest.raises(_lib.RgfmError, match="sharded"):
        ess_from_cli(p.parse_args(["--ess_floor", "8"]), sharded=True)
    d = GuidanceDiagnostics()
    assert d.tau is None
    d._begin("mc_feng", "midpoint", 3, 5, "cpu")
    assert d.tau is None
    tau = d._begin_tau()
    assert tau is d.tau and tuple(tau.shape) == (6, 5) and tau.dtype == torch.float32 and not tau.any()
    d._begin("mc_feng", "euler", 3, 5, "cpu")
    assert d.tau is None  # (a later call without a floor leaves no stale exponents)


def test_abi_table_and_stream_cases_name_the_new_exports():
    names = ("rgfm_sample_pair_ess", "rgfm_sample_cond_ess", "rgfm_guidance_apply_ess", "rgfm_guidance_apply_cond_ess")
    L = _lib.lib()
    covered = {e for c in stream_cases.CASES for e in c.exports}
    for n in names:
        assert hasattr(L, n) and n in covered, n
    assert ctypes.sizeof(_lib.Ess) == 24
    # null handles: the argument prelude answers before the floor is looked at
    null = ctypes.c_void_p(0)
    assert L.rgfm_guidance_apply_ess(*[null] * 7, 3, 7, 4, 4, 0.5, null, null, 4.0, null, null, 0, null) == -1
    assert L.rgfm_guidance_apply_cond_ess(*[null] * 4, 3, 7, 4, 0.5, null, null, 4.0, null, null, 0, null) == -1


# ------------------------------------------------------------------ what the floor does to the estimator: the toy
def test_toy_velocity_error_with_and_without_the_floor():
    """The toy of tests/test_guidance_cross_cpu.py (4 clusters per modality in 4 dimensions, matched clusters have ratio
    4, the others 1e-3; B = 8 query points on matched paths; N = 32 MC pairs, 100 MC sets) at late t: the guided
    velocity of the plain and the tempered weights against the large-N limit (200 000 pairs, plain weights), as
    mean-squared error = bias^2 + variance over the MC sets.  Tempering BIASES the estimator -- its own large-N limit is
    not the target -- and buys a smaller variance; which one wins depends on t, N and the floor, and the figures below
    (printed; DESIGN.md section 20 has them) say nothing about trained checkpoints."""
    import guidance_ref64 as G
    K, DIM, STD, B, N, SEEDS, NBIG = 4, 4, 0.3, 8, 32, 100, 200000
    centres = 2.0 * np.eye(K, DIM)

    def draw(rng, n):
        k = rng.integers(0, K, n)
        return centres[k] + STD * rng.standard_normal((n, DIM)), k
    rng = np.random.default_rng(1)
    x1, kx = draw(rng, B)
    y1 = centres[kx] + STD * rng.standard_normal((B, DIM))
    x0, y0 = rng.standard_normal((B, DIM)), rng.standard_normal((B, DIM))
    bx, bkx = draw(rng, NBIG)
    by, bky = draw(rng, NBIG)
    br = np.where(bkx == bky, 4.0, 1e-3)
    zero = np.zeros((B, DIM))
    for t in (0.8, 0.9, 0.95, 0.98):
        x, y = (1 - t) * x0 + t * x1, (1 - t) * y0 + t * y1
        gx, gy = G.guidance64(x, y, zero, zero, bx, by, br, t, 1.0)[:2]
        want = np.concatenate([gx, gy], 1)
        got = {None: [], 4.0: [], 8.0: []}
        ess1, taus = [], []
        for s in range(SEEDS):
            r2 = np.random.default_rng(100 + s)
            mx, kmx = draw(r2, N)
            my, kmy = draw(r2, N)
            r = np.where(kmx == kmy, 4.0, 1e-3)
            px, py, w0, _ = G.guidance64(x, y, zero, zero, mx, my, r, t, 1.0)
            got[None].append(np.concatenate([px, py], 1))
            ess1.append(E.ess_of(w0))
            for floor in (4.0, 8.0):
                ex, ey, _, tau = E.guidance_ess64(x, y, zero, zero, mx, my, r, t, 1.0, floor)
                got[floor].append(np.concatenate([ex, ey], 1))
                if floor == 4.0:
                    taus.append(tau)
        line = [f"toy t={t}: mean ESS_1 {np.mean(ess1):.2f}, mean tau (floor 4) {np.mean(taus):.3f};"]
        mse = {}
        for floor, runs in got.items():
            a = np.stack(runs)
            bias2 = float(((a.mean(0) - want) ** 2).sum())
            var = float(((a - a.mean(0)) ** 2).sum(axis=(1, 2)).mean())
            mse[floor] = float(((a - want) ** 2).sum(axis=(1, 2)).mean())
            line.append(f"floor {floor}: MSE {mse[floor]:.1f} = bias^2 {bias2:.1f} + var {var:.1f};")
            assert np.isfinite(a).all()
        print(" ".join(line))


# ------------------------------------------------------------------ the source of the GPU test's weights tolerance
def test_fp32_restatement_deviates_from_float64_by_the_recorded_figures():
    """ess_ref64.ORACLE_DTAU (the relative deviation of the fp32 restatement's tau from float64's, which
    tests/test_gpu_ess.py turns into the tolerance of the tempered weights) recomputed on a subset of the moderate cases
    -- B = 5, N in {2, 63, 65, 256}, paired and one-sided: no more than the recorded maximum over all cases, and not an
    order of magnitude less (the constant would then have drifted from what it stands for).  The restatement itself
    meets the tolerance made of it with the factor 4 to spare."""
    for t in (0.5, 0.9):
        worst = ratio_w = ratio_t = 0.0
        for N in (2, 63, 65, 256):
            inp = E.moderate_case(5, N, t, 300 + N + 5)
            floor = 1.5 if N == 2 else 8.0
            for one_sided in (False, True):
                ref = (E.cond64 if one_sided else E.pair64)(inp, t, 0.5, floor)
                w32, t32 = E.oracle32(inp, t, floor, one_sided)
                tempered = ref["tau"] < 1
                assert tempered.any() and ((t32 < 1) == tempered).all()
                worst = max(worst, float(np.abs(t32[tempered] / ref["tau"][tempered] - 1).max()))
                a, b = E.weights_check(w32, t32, ref, t)
                ratio_w, ratio_t = max(ratio_w, a), max(ratio_t, b)
        print(f"t={t}: fp32 restatement |tau / tau64 - 1| {worst:.2e} (recorded {E.ORACLE_DTAU[t]:.1e}); "
              f"its error / tolerance: weights {ratio_w:.3f}, tau {ratio_t:.3f}")
        assert 0.1 * E.ORACLE_DTAU[t] <= worst <= E.ORACLE_DTAU[t], (t, worst)
        assert ratio_w <= 0.3 and ratio_t <= 0.26, (ratio_w, ratio_t)
