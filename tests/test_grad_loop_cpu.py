"""The float64 side of the in-loop gradient tests (tests/grad_loop_ref64.py) on the CPU, from the reference alone: the
committed single-row seeds meet the seed rule, head scaling scales the gradient exactly, every case is admissible, the
extraction recovers a gradient through fp32 rounding within rho, and the shared assertion sees an error confined to one
receptive field."""
import pytest
import torch

import cond_grad_ref64 as CG
import grad_loop_ref64 as GL
import ratio_sweep_seeds as S
from helpers import RATIO_ROW_SEEDS, RATIO_SWEEP, make_sweep_ratio, sweep_ratio_inputs, sweep_ratio_kind

ALL_CASES = list(GL.PAIR_CASES) + list(GL.COND_CASES)


@pytest.mark.parametrize("tag", list(RATIO_ROW_SEEDS))
def test_committed_rows_meet_the_seed_rule(tag):
    """Every row of helpers.RATIO_ROW_SEEDS, alone and on the tag's own module: the fp32 encoders take the float64
    argmax in every window and the smallest gap is at least FLOOR x the largest deviation (none of the 1000 candidates
    reaches 10 x; see the table's comment).  A stacked batch measures as its worst row: the rows are independent."""
    m = make_sweep_ratio(tag)
    sd32, sd64 = S.state(m, torch.float32), S.state(m, torch.float64)
    kind = sweep_ratio_kind(tag)
    assert RATIO_ROW_SEEDS[tag][0] == RATIO_SWEEP[tag][7] and len(set(RATIO_ROW_SEEDS[tag])) == len(RATIO_ROW_SEEDS[tag])
    worst = float("inf")
    with torch.no_grad():
        for seed in RATIO_ROW_SEEDS[tag]:
            x, y, _, _ = sweep_ratio_inputs(tag, 1, seed)
            w, gap, dev, agree = S.measure_pair(kind, sd32, sd64, x, y)
            print(S.row(tag, seed, 1, dict(windows=w, gap=gap, dev=dev, ratio=gap / dev, agree=agree)))
            assert agree and gap >= S.FLOOR * dev, (tag, seed, gap, dev, agree)
            worst = min(worst, gap)
        x, y = GL._inputs(tag, 7)
        w, gap, dev, agree = S.measure_pair(kind, sd32, sd64, x, y)
    # (the same gap up to the float64 conv's summation order at another batch size)
    assert agree and abs(gap - worst) <= 1e-6 * worst and gap >= S.FLOOR * dev, (gap, worst, dev, agree)


def test_head_scaling_scales_the_float64_gradient_bit_for_bit():
    base = GL.pair_case("ms_64-disc-j0-B2")
    for j in GL.HEAD_J:
        c = GL.pair_case(f"ms_64-disc-j{j}-B2")
        for g0, g in zip(base["g64"], c["g64"]):
            assert torch.equal(g, g0 * 2.0 ** j), j
        assert all(torch.equal(a, b) for a, b in zip(base["v64"], c["v64"]))
    for given, side in (("x", 1), ("y", 0)):
        c0, c = (GL.cond_case(f"ms_64-disc-j{j}-B2-given_{given}") for j in (0, -20))
        assert torch.equal(c["g64"][0], c0["g64"][0] * 2.0 ** -20)
        # (one-sided = that side of the two-sided gradient, up to float64 rounding)
        assert float((c0["g64"][0] - base["g64"][side]).abs().max()) <= 1e-12 * float(base["g64"][side].abs().max())
    # the magnitudes the head scaling spans
    top = [max(float(g.abs().max()) for g in GL.pair_case(f"ms_64-disc-j{j}-B2")["g64"]) for j in GL.HEAD_J]
    low = min(float(g.abs().max()) for g in GL.pair_case("ms_64-disc-j-20-B2")["g64"])
    print("max|g64| per j:", top, "smallest side:", low)
    assert low < 1e-9 and top[-1] > 1.0


def test_the_case_tables_are_what_the_gpu_tests_rest_on():
    assert GL.S == 128 and GL.K == 10 and GL.DT == 2.0 ** -7 and GL.TOL_GRAD == 1e-4
    assert {c[3] for n, c in GL.PAIR_CASES.items() if n.startswith("ms_64")} == {1, GL.B_MAIN, 5, 7}
    assert GL.B_MAIN == min(len(v) for v in RATIO_ROW_SEEDS.values())
    assert {c[2] for c in GL.PAIR_CASES.values() if c[1] == "rulsif"} == {0}
    assert {c[2] for c in GL.COND_CASES.values() if c[1] == "rulsif"} == {0}
    x, y = GL.pair_case("ms_64-disc-j0-B7")["s0"]
    assert torch.equal(x[0], x[2]) and torch.equal(y[1], y[5]) and not torch.equal(x[0], x[1])
    assert torch.equal(GL.pair_case(GL.ALONE_CASE)["s0"][0], GL.pair_case(GL.BASE_CASE)["s0"][0][:1])
    # one G for both sides, as first planned, is the larger side's own G: that side's run is the planned one
    c = GL.pair_case(GL.BASE_CASE)
    assert GL.gamma_of(max(float(g.abs().max()) for g in c["g64"])) == min(c["gamma"]) == c["gamma"][0]
    joint_rho_y = GL.rho_of(c["s0"][1], c["v64"][1], c["g64"][1], min(c["gamma"]))
    assert joint_rho_y > GL.ADMISSIBLE * GL.TOL_GRAD * float(c["g64"][1].abs().max())  # (why G is taken per side)


@pytest.mark.parametrize("name", ALL_CASES)
def test_case_is_admissible_and_extraction_recovers_the_gradient(name):
    """rho <= 0.1 TOL_GRAD max|g64_side| on every side, G a power of two with G dt max|g64_side| in (1/2, 1]; and the
    extraction itself: float64 v and g rounded to fp32, the Euler update of euler_grad_kernel in fp32 (the fma formed in
    float64 and rounded once), ghat against the fp32-rounded g within rho."""
    c = GL.case(name)
    for side, (s0, v64, g64, gamma, rho) in enumerate(zip(c["s0"], c["v64"], c["g64"], c["gamma"], c["rho"])):
        gmax = float(g64.abs().max())
        assert torch.frexp(torch.tensor(gamma, dtype=torch.float64))[0] == 0.5
        assert 0.5 < gamma * GL.DT * gmax <= 1.0
        limit = GL.ADMISSIBLE * GL.TOL_GRAD * gmax
        print(f"{name} side {side}: G 2^{torch.frexp(torch.tensor(gamma))[1].item() - 1} max|g64| {gmax:.3e} rho {rho:.3e} "
              f"= {rho / gmax:.2e} max|g64| (admissible up to {limit:.3e})")
        assert rho <= limit, (name, side, rho, limit)
        v32, g32, dt = v64.float(), g64.float(), torch.tensor(GL.DT, dtype=torch.float32)
        runs = []
        for gm in (0.0, gamma):
            inner = (gm * g32.double() + v32.double()).float()  # fmaf(gamma, g, v)
            runs.append(s0 + inner * dt)                         # __fadd_rn(s, __fmul_rn(., dt))
        assert runs[0].dtype == torch.float32
        ghat = GL.extract(runs[1], runs[0], gamma)
        err = float((ghat - g32.double()).abs().max())
        print(f"{name} side {side}: extraction error {err:.3e} = {err / rho:.2f} rho")
        assert 0.0 < err <= rho, (name, side, err, rho)


def test_assert_grad_close_sees_one_receptive_field():
    """A g64 off by 3 TOL_GRAD max|g64| on one 8x8 patch of one row and one side is rejected; the exact one passes; an
    error of rho alone passes."""
    c = GL.pair_case("ms_64-disc-j0-B5")
    ghat = tuple(g.float().double() for g in c["g64"])  # (fp32 rounding: far inside the bound)
    GL.assert_grad_close(ghat, c["g64"], c["rho"], "exact")
    GL.assert_grad_close(tuple(g + r for g, r in zip(ghat, c["rho"])), c["g64"], c["rho"], "off by rho")
    for side in (0, 1):
        for row, ch in ((3, 0), (4, c["g64"][side].shape[1] - 1)):
            bad = [g.clone() for g in c["g64"]]
            bad[side][row, ch, 16:24, 8:16] += 3 * GL.TOL_GRAD * float(c["g64"][side].abs().max())
            with pytest.raises(AssertionError):
                GL.assert_grad_close(ghat, tuple(bad), c["rho"], f"perturbed side {side} row {row}")
    g, _ = CG.grad_given64("mnist_svhn", CG.params64(c["rr"]), c["s0"][0], c["s0"][1], "x", "disc")
    with pytest.raises(AssertionError):  # (a one-sided case: 1-tuples)
        bad = g.clone()
        bad[0, 1, :8, :8] -= 3 * GL.TOL_GRAD * float(g.abs().max())
        GL.assert_grad_close((g,), (bad,), (0.0,), "perturbed one-sided")
