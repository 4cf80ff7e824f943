"""The yardstick of tests/test_gpu_guidance.py checked on the CPU: that the GPU test CAN fail.

guidance_ref64.guidance64 (float64 numpy restatement of reference src/sample_mnist_svhn.py:124-171) against the fp32
oracle on guidance_ref64.spread_case inputs, over every case, step and centre the GPU test runs.

Measured deviations of the fp32 oracle from float64 (max over the eight CASES; relative weight deviation
max |w32 - w64| / w64, and max |dv|; |v|max grows from ~3 at t = 0.05 to ~28 at t = 0.99):

    t       centre = 1               centre = 0
    0.05    dw 1.14e-6   dv 1.5e-6   dw 1.03e-6   dv 2.7e-7
    0.5     dw 1.12e-6   dv 3.9e-6   dw 2.57e-6   dv 8.4e-7
    0.9     dw 2.77e-6   dv 6.6e-6   dw 1.93e-6   dv 1.7e-6
    0.99    dw 1.66e-5   dv 1.5e-5   dw 1.55e-6   dv 2.3e-6

(dw is largest at N = 4096, where the oracle's sequential fp32 sums are longest; at centre = 1 and t = 0.99 the fp32
rounding of mu = t m, |m| ~ 3, is a visible share of x - mu ~ sigma / sqrt D.)  guidance_ref64.ORACLE_DW holds the dw
column rounded up; the GPU test's weights tolerance is 4x it and its velocity bound is guidance_ref64.velocity_bound.
The oracle stays inside both (asserted below), on the ratio and underflow edges too.

Conditions on the reference, asserted for every row: effective sample size 1 / sum w^2 >= N / 2 (measured 0.61 N to
N), min w N >= 0.05 (measured >= 0.07), max |l| < 10 (measured <= 2.2): the float64 answer is well-conditioned and no
sample is negligible.

Drop-one sensitivity, centre = 0 and N <= 544: omitting any single sample k moves some velocity element of EVERY row
by at least 10x the velocity bound (measured, worst row, sample and t: 18x at N = 544, 47x at N = 288, 58x at N = 257,
253x at N = 70, 624x at N = 33), so a GEMM that drops, duplicates or mis-indexes one k cannot pass the GPU test.  At N = 4096 this
cannot hold: one sample carries 1 / 4096 of the sum (measured 0.7x to 0.85x).  There the per-element weights check
carries the weights stage and the velocity check is a bound on the GEMM, not a per-sample detector.
"""
import numpy as np
import pytest

import guidance_ref64 as R
from oracle import oracle as O

CONFIGS = [(ci, si, centre) for ci in range(len(R.CASES)) for si in range(len(R.STEPS)) for centre in R.CENTRES]


def _oracle(inp, t, gamma):
    return O.guidance_apply(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], inp["r"], t, gamma, True)


def _dv(ovx, ovy, ref):
    return max(float(np.abs(ovx - ref["vx"]).max()), float(np.abs(ovy - ref["vy"]).max()))


@pytest.mark.parametrize("ci,si,centre", CONFIGS)
def test_oracle_within_the_gpu_bounds_and_reference_conditions(ci, si, centre):
    B, N, dx, dy = R.CASES[ci]
    t, gamma = R.STEPS[si]
    inp, ref = R.case(ci, si, centre)
    w = ref["w"]
    # the reference is well-conditioned and every sample counts
    ess = 1.0 / (w ** 2).sum(1)
    assert ess.min() >= N / 2, (ess.min(), N)
    assert w.min() * N >= 0.05, w.min() * N
    assert np.abs(ref["l"]).max() < 10
    assert np.abs(w.sum(1) - 1).max() < 1e-9
    # the fp32 oracle against it
    ovx, ovy, ow = _oracle(inp, t, gamma)
    dw = float((np.abs(ow - w) / w).max())
    dv = _dv(ovx, ovy, ref)
    bound = R.velocity_bound(inp, ref, N, t, gamma, R.tol_w(t, centre))
    print(f"{R.CASES[ci]} t={t} centre={centre}: oracle dw {dw:.2e} (recorded {R.ORACLE_DW[(t, centre)]:.1e})  "
          f"dv {dv:.2e}  bound {bound:.2e}  ess/N {ess.min() / N:.2f}  min w N {w.min() * N:.2f}")
    assert dw <= R.ORACLE_DW[(t, centre)], (dw, R.ORACLE_DW[(t, centre)])  # the recorded figure covers this case
    assert dv <= bound, (dv, bound)


@pytest.mark.parametrize("ci,si", [(ci, si) for ci in range(len(R.CASES)) for si in range(len(R.STEPS))
                                   if R.CASES[ci][1] <= 544])
def test_dropping_any_one_sample_exceeds_the_velocity_bound_tenfold(ci, si):
    B, N, dx, dy = R.CASES[ci]
    t, gamma = R.STEPS[si]
    inp, ref = R.case(ci, si, 0.0)
    c = 1 - t + R.EPS
    x = np.concatenate([inp["x"], inp["y"]], 1).astype(np.float64)
    m = np.concatenate([inp["mx"], inp["my"]], 1).astype(np.float64)
    eff = np.empty((B, N))  # the velocity error of omitting sample k from row b
    for b in range(B):
        eff[b] = gamma * np.abs(ref["w"][b][:, None] * (m - x[b]) / c).max(1)
    worst = float(eff.min())  # (every sample, the row where it matters least)
    bound = R.velocity_bound(inp, ref, N, t, gamma, R.tol_w(t, 0.0))
    print(f"{R.CASES[ci]} t={t}: drop-one {worst:.2e} = {worst / bound:.0f} x bound {bound:.2e}")
    assert worst >= 10 * bound, (worst, bound)


@pytest.mark.parametrize("si", range(len(R.STEPS)))
def test_oracle_on_the_ratio_edges(si):
    t, gamma = R.STEPS[si]
    N = R.CASES[0][1]
    for k, value in ((67, 0.0), (3, 1e6)):
        inp, ref = R.ratio_edge(si, k, value)
        ovx, ovy, ow = _oracle(inp, t, gamma)
        keep = ref["w"] > 0
        assert (keep.sum(1) == N - (value == 0.0)).all()
        assert (ow[~keep] == 0).all()
        dw = float((np.abs(ow - ref["w"])[keep] / ref["w"][keep]).max())
        assert dw <= R.ORACLE_DW[(t, 0.0)], (value, dw)
        assert _dv(ovx, ovy, ref) <= R.velocity_bound(inp, ref, N, t, gamma, R.tol_w(t, 0.0))


def test_oracle_on_the_underflowing_row():
    inp, ref, row, gap = R.shifted_row()
    t, gamma = R.STEPS[3]
    assert gap >= 50, gap
    assert ref["w"][row].max() > 1 - 1e-9  # one-hot in float64
    ow = _oracle(inp, t, gamma)[2]
    assert np.isfinite(ow).all() and abs(float(ow[row].sum()) - 1) < 1e-6
    assert np.abs(ow[row] - ref["w"][row]).max() < 1e-6
    others = np.arange(ow.shape[0]) != row
    assert (np.abs(ow - ref["w"])[others] / ref["w"][others]).max() <= R.ORACLE_DW[(t, 0.0)]
