"""The yardstick of tests/test_gpu_cond.py checked on the CPU.

1. cond_ref64.cond64 IS guidance_ref64.guidance64 on the equivalent paired problem.  Take row b alone, give the paired
   block an x modality whose MC rows are all one image m0 and whose state is x = t m0: the x term of l is exactly zero
   for every sample (x - t m0 is computed by the same float64 operation on both sides), so the paired weights are the
   one-sided ones with r = R[b].  Weights and the y velocity agree to 1e-12 relative.  This ties the new reference to
   the one the reference project's goldens pin.

2. The GPU cases have SPREAD weights: every row of every case with t <= 0.9 has at least two float64 weights above
   1e-3, and evaluating a row with ANOTHER row's ratios moves its weights by more than 100 tol_w.  A one-hot row would let a
   broken ratio stride pass: whatever ratio the heavy sample is given, it normalises to 1.  The case N = 1 is the one
   exception by arithmetic, not by construction -- a row of one weight is [1.0] -- and is asserted to be exactly that;
   it is in the GPU set for the kernels' minimal tiling, not for the ratio stride.
"""
import numpy as np
import pytest

import cond_ref64 as C
import guidance_ref64 as G

CONFIGS = [(ci, si, centre) for ci in range(len(C.CASES)) for si in range(len(C.STEPS)) for centre in C.CENTRES]


@pytest.mark.parametrize("ci,si,centre", CONFIGS)
def test_cond64_is_guidance64_with_one_side_observed(ci, si, centre):
    B, N, dim = C.CASES[ci]
    t, gamma = C.STEPS[si]
    inp, ref = C.case(ci, si, centre)
    g = np.random.default_rng(77 + ci)
    m0 = g.standard_normal(12)
    mx = np.tile(m0, (N, 1))
    for b in range(B):
        x = (float(t) * mx)[:1]  # (the operation guidance64 performs: the difference is exactly zero)
        vx = g.standard_normal((1, 12))
        _, vy, w, l = G.guidance64(x, inp["s"][b:b + 1], vx, inp["v"][b:b + 1], mx, inp["m"], inp["R"][b], t, gamma)
        assert np.abs(w[0] - ref["w"][b]).max() <= 1e-12 * ref["w"][b].max()
        assert np.abs(vy[0] - ref["v"][b]).max() <= 1e-12 * np.abs(ref["v"][b]).max()
        assert np.array_equal(l[0], ref["l"][b])


@pytest.mark.parametrize("ci,si,centre", CONFIGS)
def test_gpu_cases_have_spread_weights(ci, si, centre):
    B, N, dim = C.CASES[ci]
    t, _ = C.STEPS[si]
    w = C.case(ci, si, centre)[1]["w"]
    assert np.abs(w.sum(1) - 1).max() < 1e-9
    if N == 1:
        assert np.abs(w - 1).max() < 1e-9
        return
    if t <= 0.9:
        assert ((w > 1e-3).sum(1) >= 2).all(), (w > 1e-3).sum(1)
        # and the ratio rows matter: with row 0's ratios every other row's weights move by more than 100x the tolerance
        if B > 1:
            inp = C.case(ci, si, centre)[0]
            wrong = C.cond64(inp["s"], inp["v"], inp["m"], np.tile(inp["R"][:1], (B, 1)), t, 1.0)[1]
            rel = np.abs(wrong[1:] - w[1:]) / w[1:]
            assert rel.max(1).min() > 100 * G.tol_w(t, centre), rel.max(1).min()


def test_one_hot_ratio_row_gives_a_one_hot_weight_row():
    """What the GPU ratio-stride check relies on: a ratio row that is 1 at k and 0 elsewhere makes that row's float64
    weights the one-hot at k, and leaves every other row's weights as they were."""
    ci, si, centre = 1, 1, 0.0
    t, gamma = C.STEPS[si]
    inp, ref = C.case(ci, si, centre)
    R = inp["R"].copy()
    row, k = 17, 41
    R[row] = 0
    R[row, k] = 1
    w = C.cond64(inp["s"], inp["v"], inp["m"], R, t, gamma)[1]
    onehot = np.zeros(R.shape[1])
    onehot[k] = 1
    assert np.abs(w[row] - onehot).max() < 1e-9
    others = np.arange(R.shape[0]) != row
    assert np.array_equal(w[others], ref["w"][others])
