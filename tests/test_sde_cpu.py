"""The stochastic sampler step without a GPU: the specification of include/rgfm.h ("Stochastic sampling") as restated in
tests/sde_ref64.py is pinned here, so that the GPU tests compare against something known to be sound; and the binding's
new symbols.

Generator: moments, range, correlations and the prefix property of the float64 restatement.  z-scores are against the
sampling distribution of each statistic under N(0, 1): the mean has standard error 1 / sqrt(n), the variance
sqrt(2 / n), the kurtosis sqrt(24 / n); |z| <= 4 each.
Step: a 1-D two-component Gaussian mixture with its analytic velocity, 200 000 samples, 100 steps; the end mean within 4
standard errors of the data mean and the end variance within 1 % of the data variance (the ODE's Euler loop at the same
step count is off by 0.94 %).
"""
import ctypes

import numpy as np
import pytest

import ode_ref64 as O
import sde_cases  # noqa: F401  (registers the stream cases of the new exports: its docstring)
import sde_ref64 as S
import stream_cases
from ratio_guided_multimodal_fm_amd import _lib


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize("n", [4096, 65536, 1 << 20])
def test_moments_and_range(n):
    worst = [0.0, 0.0, 0.0, 0.0]
    for seed in range(1234, 1242):
        for k in range(4):
            xi = S.noise(seed, 1, k, n)
            m, c = xi.mean(), xi - xi.mean()
            var = (c ** 2).mean()
            kurt = (c ** 4).mean() / var ** 2
            z = (np.sqrt(n) * m, np.sqrt(n / 2) * (var - 1.0), np.sqrt(n / 24) * (kurt - 3.0), np.abs(xi).max())
            worst = [max(w, abs(v)) for w, v in zip(worst, z)]
    print(f"n={n}: worst |z| mean {worst[0]:.2f} var {worst[1]:.2f} kurt {worst[2]:.2f}; max |xi| {worst[3]:.3f}")
    assert worst[0] <= 4 and worst[1] <= 4 and worst[2] <= 4, worst
    assert worst[3] <= 5.78, worst[3]


def test_the_largest_magnitude_is_the_stated_bound():
    # u1 = 2^-24 is the smallest value: r = sqrt(48 ln 2)
    assert abs(np.sqrt(-2.0 * np.log(2.0 ** -24)) - np.sqrt(48 * np.log(2))) < 1e-12 and np.sqrt(48 * np.log(2)) < 5.78


def test_correlations():
    n = 65536
    a = S.noise(5, 0, 0, n)
    corr = lambda u, v: float(np.corrcoef(u, v)[0, 1]) * np.sqrt(len(u))  # noqa: E731  (in units of 1 / sqrt(n))
    got = {"stages": corr(a, S.noise(5, 0, 1, n)), "streams": corr(a, S.noise(5, 1, 0, n)), "seeds": corr(a, S.noise(6, 0, 0, n)),
           "lag1": corr(a[:-1], a[1:]), "pair halves": corr(a[0::2], a[1::2])}
    print({k: round(v, 2) for k, v in got.items()})
    for k, v in got.items():
        assert abs(v) <= 4, (k, v)


def test_prefix_property_and_odd_lengths():
    full = S.noise(2024, 1, 3, 4099)
    for m in (1, 2, 3, 255):
        assert np.array_equal(full[:m], S.noise(2024, 1, 3, m))
    # an odd length ends on the cosine of its last pair
    u1, u2 = S.uniforms(2024, 1, 3, 2)
    assert S.noise(2024, 1, 3, 3)[2] == np.sqrt(-2 * np.log(u1[1])) * np.cos(2 * np.pi * u2[1])


def test_uniforms_are_exact_24_bit_fractions_in_their_ranges():
    u1, u2 = S.uniforms(2 ** 64 - 1, 1, 4095, 1 << 16)
    assert (u1 > 0).all() and (u1 <= 1).all() and (u2 >= 0).all() and (u2 < 1).all()
    for u in (u1, u2):
        assert np.array_equal(u * 2 ** 24, np.round(u * 2 ** 24)) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    # the key and the hash wrap mod 2^64 without an error, and differ by seed, stream and step
    keys = {int(S.key_of(s, m, k)) for s in (0, 2 ** 63 + 5, 2 ** 64 - 1) for m in (0, 1) for k in (0, 1, 4095)}
    assert len(keys) == 18
    # fin against the constants written out by hand for one word
    z = 0x0123456789ABCDEF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert int(S.fin(np.uint64(0x0123456789ABCDEF))) == z ^ (z >> 31)


# ------------------------------------------------------------------ the step
MU, SD = np.array([-1.0, 1.5]), np.array([0.2, 0.3])


def mixture_velocity(s, t):
    """E[x1 - x0 | x_t = x] of x_t = (1 - t) x0 + t x1, x0 ~ N(0, 1), x1 ~ the equal-weight mixture N(MU_j, SD_j^2)."""
    x = s[0][:, None]
    var = (1 - t) ** 2 + (t * SD) ** 2
    logw = -0.5 * (x - t * MU) ** 2 / var - 0.5 * np.log(var)
    w = np.exp(logw - logw.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    u = MU + (t * SD ** 2 - (1 - t)) / var * (x - t * MU)
    return ((w * u).sum(axis=1),)


DATA_MEAN, DATA_VAR = 0.25, 1.6275


def test_the_data_moments():
    assert abs(MU.mean() - DATA_MEAN) < 1e-15 and abs((SD ** 2 + MU ** 2).mean() - DATA_MEAN ** 2 - DATA_VAR) < 1e-12


@pytest.mark.parametrize("eta", [1.0, 4.0])
def test_toy_mixture_keeps_the_data_marginal(eta):
    B, N = 200000, 100
    x0 = S.noise(11, 0, 4095, B)
    x = S.integrate_sde64(mixture_velocity, (x0,), N, eta, 2024)[0]
    mean, var = x.mean(), x.var()
    print(f"eta={eta}: mean {mean:.4f} (data {DATA_MEAN}), var {var:.4f} (data {DATA_VAR}, deviation {var / DATA_VAR - 1:+.4f})")
    assert abs(mean - DATA_MEAN) <= 0.012, mean
    assert abs(var / DATA_VAR - 1) <= 0.01, var


def test_eta_zero_is_the_euler_loop_exactly_and_split_ranges_compose():
    x0 = S.noise(3, 0, 0, 1000)
    want = O.integrate64(mixture_velocity, (x0,), 10, "euler")[0]
    assert np.array_equal(S.integrate_sde64(mixture_velocity, (x0,), 10, 0.0, 99)[0], want)
    whole = S.integrate_sde64(mixture_velocity, (x0,), 10, 0.8, 7)[0]
    half = S.integrate_sde64(mixture_velocity, (x0,), 10, 0.8, 7, 0, 4)
    assert np.array_equal(S.integrate_sde64(mixture_velocity, half, 10, 0.8, 7, 4, 10)[0], whole)
    assert not np.array_equal(whole, want) and not np.array_equal(whole, S.integrate_sde64(mixture_velocity, (x0,), 10, 0.8, 8)[0])


def test_zero_velocity_is_the_linear_recursion_in_the_noise():
    x0, N, eta, seed = S.noise(4, 0, 0, 77), 4, 0.8, 21
    got = S.integrate_sde64(lambda s, t: (np.zeros_like(s[0]),), (x0,), N, eta, seed)[0]
    x, dt = x0.copy(), 1.0 / N
    for k in range(N):
        x = (1 - eta * dt) * x + np.sqrt(2 * eta * (1 - k * dt) * dt) * S.noise(seed, 0, k, 77)
    assert np.array_equal(got, x)


# ------------------------------------------------------------------ the binding
LOOPS = {"single": "rgfm_sample_single_ode", "pair": "rgfm_sample_pair_gs", "pair_cross": "rgfm_sample_pair_cross_gs",
         "cond": "rgfm_sample_cond_gs", "pair_grad": "rgfm_sample_pair_grad_gs", "cond_grad": "rgfm_sample_cond_grad_gs"}


def test_new_symbols_are_the_namesakes_plus_the_argument():
    L = _lib.lib()
    for name in ("rgfm_sde_noise", "rgfm_sde_scratch_bytes"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    for kind, twin in LOOPS.items():
        name = f"rgfm_sample_{kind}_sde"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        old, new = _lib.SIGNATURES[twin][1], _lib.SIGNATURES[name][1]
        assert new == old[:-3] + [ctypes.POINTER(_lib.Sde)] + old[-3:], name  # directly in front of (ws, ws_bytes, stream)
    assert ctypes.sizeof(_lib.Sde) == 16 and _lib.Sde.eta.offset == 0 and _lib.Sde.seed.offset == 8
    assert _lib.ABI_VERSION == 3  # added functions only


def test_scratch_bytes_is_one_buffer_per_modality():
    L, nb = _lib.lib(), ctypes.c_size_t()
    up = lambda n: (4 * n + 255) // 256 * 256  # noqa: E731  (the workspace carve's 256-byte granules)
    assert L.rgfm_sde_scratch_bytes(3, 256, 1728, ctypes.byref(nb)) == 0 and nb.value == up(3 * 256) + up(3 * 1728)
    assert L.rgfm_sde_scratch_bytes(3, 1728, 0, ctypes.byref(nb)) == 0 and nb.value == up(3 * 1728)
    assert L.rgfm_sde_scratch_bytes(0, 256, 0, ctypes.byref(nb)) == -1
    assert L.rgfm_sde_scratch_bytes(3, 256, 0, None) == -1
    assert L.rgfm_sde_noise(1, 2, 0, 4, None, None) == -1


def test_every_new_stream_export_has_a_stream_case():
    covered = {e for c in stream_cases.CASES for e in c.exports}
    for name, (_, args) in _lib.SIGNATURES.items():
        if name.endswith("_sde") or name == "rgfm_sde_noise":
            assert name in covered, name
    ids = [c.id for c in stream_cases.CASES]
    assert len(ids) == len(set(ids)) and stream_cases.BY_ID.keys() == set(ids)
