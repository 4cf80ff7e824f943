"""CPU side of tests/test_gpu_fmnet_eval.py: what the float64 yardstick (tests/fmnet_ref64.py) is worth.

- the reference's own fp32 forward (tests/golden/fmnet_eval.npz, written by tests/golden/make_fmnet_eval_golden.py from
  the reference's module class) agrees with forward64 and sits within a third of the GPU test's tolerance on every
  case; so does torch's fp32 CPU evaluation of the restatement itself, computed here;
- the two embedding mistakes the GPU test is meant to catch -- the U-Net's divisor `half` for `half - 1`, the time
  columns one place off in the concat -- each move the float64 difference v(x, ta) - v(x, tb) by at least ten
  tolerances;
- guidance applied one step early (at t = 0.001, which `t > 1e-3` leaves unguided) moves the 1000-step window's result
  by more than ten sampler tolerances;
- euler64 / pair64 are the loops they claim to be.

Every figure is printed (pytest -s)."""
import numpy as np
import pytest
import torch

import fmnet_ref64 as R
from helpers import golden, maxdiff

TOL_EVAL = 1e-5
TOL_SAMPLER = 1e-4


def eval_tol(ci):  # as tests/test_gpu_fmnet_eval.py
    return TOL_EVAL * R.eval_scale(ci)


def test_fixture_is_of_these_cases():
    g = golden("fmnet_eval")
    assert g["cases"].tolist() == [[f, t, b, int(s)] for f, t, b, s in R.EVAL_CASES]
    assert int(g["seed"]) == R.SEED_W
    for ci in range(len(R.EVAL_CASES)):
        x, t = R.eval_inputs(ci)
        assert np.array_equal(g[f"x_fp_{ci}"], x.reshape(-1)[:8].numpy())
        assert np.array_equal(g[f"t_{ci}"], t.numpy())


@pytest.mark.parametrize("ci", range(len(R.EVAL_CASES)))
def test_reference_fp32_error_leaves_room_for_the_tolerance(ci):
    """max |v32 - v64| < tolerance / 3 for the reference module's fp32 forward (fixture: its output at 256 seeded
    positions, its error over the whole output) and for the fp32 evaluation of the restatement."""
    g = golden("fmnet_eval")
    F_dim, T_dim, B, shared = R.EVAL_CASES[ci]
    v64 = R.eval_ref(ci)
    idx = g[f"probe_idx_{ci}"]
    probe_err = maxdiff(g[f"probe_v32_{ci}"], v64.reshape(-1)[idx])
    ref32_err = float(g["ref32_err_cases"][ci])
    x, t = R.eval_inputs(ci)
    with torch.no_grad():
        v32 = R.forward64(R.params_of(R.module_cpu(F_dim, T_dim), torch.float32), x, t)
    assert v32.dtype == torch.float32
    own32_err = maxdiff(v32.numpy(), v64)
    tol = eval_tol(ci)
    print(f"\nF={F_dim} T={T_dim} B={B} shared_t={shared}: max|v64| {np.abs(v64).max():.3f}  reference-fp32 err "
          f"{ref32_err:.3e} (at the probes {probe_err:.3e})  restatement-fp32 err {own32_err:.3e}  tol/3 {tol / 3:.3e}")
    assert probe_err <= ref32_err < tol / 3
    assert own32_err < tol / 3


def test_time_values_cover_both_ends():
    ts = torch.cat([R.eval_inputs(ci)[1] for ci in range(len(R.EVAL_CASES))])
    assert (ts == 0.0).any() and (ts == np.float32(R.T_LATE)).any()
    assert ((ts > 0.0) & (ts < np.float32(R.T_LATE))).sum() > 50
    for ci, (_, _, B, shared) in enumerate(R.EVAL_CASES):
        assert R.eval_inputs(ci)[1].numel() == (1 if shared or B == 1 else B)


@pytest.mark.parametrize("F_dim,T_dim", R.EMBED_DIMS)
def test_embedding_mistakes_move_the_difference(F_dim, T_dim):
    """v(x, ta) - v(x, tb) in float64 with a wrong embedding against the right one.  The shifted columns move every
    pair's difference by >= 10 TOL_EVAL.  The wrong divisor changes frequency i by the factor 1e4^(i / (half (half -
    1))): over the three short pairs, whose arguments move by <= 1e-3 f_i, that is 7e-7 .. 2.6e-5 of output -- no teeth
    at any seed -- and the pair (0, 1) is there for it: >= 10 TOL_EVAL at every dims."""
    d = R.embed_ref(F_dim, T_dim)
    n = len(R.EMBED_PAIRS)
    moved = {name: np.abs(R.embed_diff64(F_dim, T_dim, emb) - d).reshape(n, -1).max(1)
             for name, emb in (("half", R.embedding_divided_by_half), ("shift", R.embedding_shifted_one_column))}
    print(f"\nF={F_dim} T={T_dim}")
    for p, pair in enumerate(R.EMBED_PAIRS):
        print(f"  t pair {pair}: max|d| {np.abs(d[p]).max():.3e}  moved by divisor `half` {moved['half'][p]:.3e}  "
              f"by a one-column shift {moved['shift'][p]:.3e}")
    assert (moved["shift"] >= 10 * TOL_EVAL).all()
    assert R.EMBED_PAIRS[-1] == (0.0, 1.0) and moved["half"][-1] >= 10 * TOL_EVAL


def test_embedding_is_the_formula():
    """sin half first, f_i = 1e4^(-i / (half - 1)): f_0 = 1, f_last = 1e-4."""
    e = R.time_embedding64(torch.tensor([0.0, 1.0], dtype=torch.float64), 16)
    assert e.shape == (2, 16)
    assert torch.equal(e[0], torch.tensor([0.0] * 8 + [1.0] * 8, dtype=torch.float64))
    assert abs(float(e[1, 0]) - np.sin(1.0)) < 1e-15 and abs(float(e[1, 7]) - np.sin(1e-4)) < 1e-15
    assert abs(float(e[1, 8]) - np.cos(1.0)) < 1e-15 and abs(float(e[1, 9]) - np.cos(1e4 ** (-1 / 7))) < 1e-15


def test_euler64_is_the_loop_and_its_windows_chain():
    F_dim, T_dim = R.SINGLE_DIMS[0]
    sd, x0 = R.sd64(F_dim, T_dim), R.single_inputs(F_dim, T_dim)
    with torch.no_grad():
        x = x0.double()
        for step in range(3):
            x = x + R.forward64(sd, x, torch.tensor([step * (1.0 / 3)], dtype=torch.float64)) * (1.0 / 3)
        assert torch.equal(R.euler64(sd, x0, 3), x)
        assert np.array_equal(R.euler64(sd, R.euler64(sd, x0, 7, 0, 3), 7, 3, 7).numpy(), R.single_ref(F_dim, T_dim, 7))
        assert torch.equal(R.euler64(sd, x0, 7, 4, 4), x0.double())


def test_unguided_pair_is_two_single_loops():
    sdx, sdy = R.pair_sds()
    x0, y0 = R.pair_inputs(0)[:2]
    x, y = R.pair_ref(0, 0.5, 6, 0, 6)
    with torch.no_grad():
        assert np.array_equal(x, R.euler64(sdx, x0, 6).numpy()) and np.array_equal(y, R.euler64(sdy, y0, 6).numpy())
    assert np.array_equal(R.pair_ref(0, 2.0, 6, 0, 6)[0], x)  # gamma is not read without an MC set


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_guidance_threshold_case_has_teeth(gamma):
    """The first four steps of 1000: t = 0, 0.001, 0.002, 0.003.  `t > 1e-3` guides steps 2 and 3 only; guiding step 1
    as well (a `>=`, a threshold compared in fp32, a step index off by one) must move the float64 result by more
    than 10 TOL_SAMPLER, and guiding none by more still."""
    x, y = R.pair_ref(9, gamma, 1000, 0, 4)
    xe, ye = R.pair_ref(9, gamma, 1000, 0, 4, threshold=0.5e-3)
    xn, yn = R.pair_ref(0, gamma, 1000, 0, 4)
    early = max(maxdiff(xe, x), maxdiff(ye, y))
    none = max(maxdiff(xn, x), maxdiff(yn, y))
    print(f"\ngamma {gamma}: guided one step early moves (x, y) by {early:.3e}, never guided by {none:.3e} "
          f"(10 TOL_SAMPLER = {10 * TOL_SAMPLER:.0e})")
    assert early > 10 * TOL_SAMPLER and none > 10 * TOL_SAMPLER
    assert 1 * (1.0 / 1000) == 1e-3 and not 1 * (1.0 / 1000) > 1e-3 and 2 * (1.0 / 1000) > 1e-3


def test_sampler_references_in_fp32():
    """The loops evaluated in fp32 on the CPU stay within a third of TOL_SAMPLER of float64 (printed: the margin the
    GPU samplers are given)."""
    worst = 0.0
    with torch.no_grad():
        for F_dim, T_dim in R.SINGLE_DIMS:
            sd32 = R.params_of(R.module_cpu(F_dim, T_dim), torch.float32)
            x = R.single_inputs(F_dim, T_dim)
            for step in range(7):
                x = x + R.forward64(sd32, x, torch.tensor([step * (1.0 / 7)])) * np.float32(1.0 / 7)
            err = maxdiff(x.numpy(), R.single_ref(F_dim, T_dim, 7))
            print(f"\nsingle F={F_dim} T={T_dim}, 7 steps: fp32 loop err {err:.3e}")
            worst = max(worst, err)
    assert worst < TOL_SAMPLER / 3
