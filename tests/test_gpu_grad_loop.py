"""The guidance term INSIDE the gradient-guided sampler loops (rgfm_sample_pair_grad[_ode], rgfm_sample_cond_grad[_ode])
against float64.

The stand-alone gradients run the estimator on the exact fp32 MFMA and are pinned to float64 elsewhere.  Inside the loops
the same pass runs on other arithmetic for RatioEstimatorMNISTSVHN: forward convs on the U-Net handle's two fp16 planes
with the folded-BatchNorm epilogue, reverse convs on the two planes behind a tensor-wide power-of-two pre-scale
(ConvArgs::in_amax).  The loops return states; tests/grad_loop_ref64.py reads the gradient out of one Euler step
(step 10 of 128, gamma 0 against a power-of-two gamma chosen from float64) and states the bound

    max|ghat - g64| <= 1e-4 max|g64_side| + rho        (per side; rho: the rounding of the two Euler updates),

the stand-alone gradient's tolerance.  tests/test_grad_loop_cpu.py checks the float64 side on its own: seeds, the exact
head scaling that moves the gradient's magnitude from 1e-9 to 10 without touching the max-pool routing, admissibility
of every case, the extraction, and that the assertion sees one receptive field.

The GroupNorm kinds (RatioEstimator, FlexibleRatioEstimator) run the stand-alone's arithmetic in the loop too; their
cases pin the loops' plumbing (feature stride and columns, context, output buffers).

Data seeds were fixed by the CPU rule (tests/ratio_sweep_seeds.py) before the first GPU run.  Measured on an MI355X:
DESIGN.md section 11."""
import pytest
import torch

import grad_loop_ref64 as GL
from ratio_guided_multimodal_fm_amd import _engine, _lib

pytestmark = pytest.mark.gpu

SWITCHES = (("RGFM_CONV", "f32"), ("RGFM_CONV", "bx3"), ("RGFM_REV_HX2", "0"), ("RGFM_OVERLAP", "0"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def run_loop(c, gamma, dev):
    """End states (one per side) of the single step [K, K + 1) of S from the case's s0 at `gamma`."""
    rr = c["rr"].to(dev)
    nets = [n.to(dev) for n in c["nets"]]
    s = [t.to(dev).clone() for t in c["s0"]]
    if len(s) == 2:
        _engine.sample_pair_grad(nets[0], nets[1], rr, s[0], s[1], GL.S, gamma, GL.K, GL.K + 1)
    else:
        ctx = rr._engine.cond_prepare(c["cond"].to(dev), c["given"], tuple(s[0].shape[1:]))
        _engine.sample_cond_grad(nets[0], rr, s[0], ctx, c["given"], GL.S, gamma, GL.K, GL.K + 1)
    torch.cuda.synchronize()
    return s


def extract(c, dev):
    """ghat per side: gamma 0, then one run per distinct gamma of the sides."""
    zero = run_loop(c, 0.0, dev)
    runs = {g: run_loop(c, g, dev) for g in sorted(set(c["gamma"]))}
    return tuple(GL.extract(runs[g][i], zero[i], g) for i, g in enumerate(c["gamma"]))


_ghat = {}


def check(name, dev, mode="default"):
    """Extract the case's in-loop gradient in the current arithmetic mode and hold it to the bound; kept per (case,
    mode) for the tests that compare runs."""
    c = GL.case(name)
    before = _engine.range_fallbacks
    ghat = extract(c, dev)
    gammas = " ".join(f"2^{int(torch.tensor(g).log2())}" for g in c["gamma"])
    GL.assert_grad_close(ghat, c["g64"], c["rho"], f"{name} [{mode}] G {gammas}")
    if mode == "default":
        assert _engine.range_fallbacks == before, (name, _engine.last_range_flags)
    _ghat[(name, mode)] = ghat
    return ghat


@pytest.mark.parametrize("name", list(GL.PAIR_CASES))
def test_pair_loop_gradient_vs_float64(dev, name):
    check(name, dev)


@pytest.mark.parametrize("name", list(GL.COND_CASES))
def test_cond_loop_gradient_vs_float64(dev, name):
    check(name, dev)


def test_arithmetic_switches_meet_the_same_bound(dev, monkeypatch):
    """RGFM_CONV=f32 / bx3, RGFM_REV_HX2=0 and RGFM_OVERLAP=0 on the base case; the default run raises no range fallback
    (check) and differs from the RGFM_REV_HX2=0 run: the two-plane reverse convs are what ran."""
    default = _ghat.get((GL.BASE_CASE, "default")) or check(GL.BASE_CASE, dev)
    for key, value in SWITCHES:
        monkeypatch.setenv(key, value)
        check(GL.BASE_CASE, dev, f"{key}={value}")
        monkeypatch.delenv(key)
    rev32 = _ghat[(GL.BASE_CASE, "RGFM_REV_HX2=0")]
    c = GL.case(GL.BASE_CASE)
    for side, a, b, g in zip("xy", default, rev32, c["g64"]):
        print(f"default vs RGFM_REV_HX2=0 side {side}: {float((a - b).abs().max()) / float(g.abs().max()):.3e} max|g64|")
    assert any(not torch.equal(a, b) for a, b in zip(default, rev32))
    serial = _ghat[(GL.BASE_CASE, "RGFM_OVERLAP=0")]
    assert all(torch.equal(a, b) for a, b in zip(default, serial))  # (the streams change the order of launches, no bit)


def test_a_row_alone_and_inside_a_batch(dev):
    """Row 0 alone (B = 1) and inside the batches of 2 and 5: each run meets the bound; the difference is printed, not
    asserted -- the pre-scale is one exponent per tensor, so a row's bits may depend on its batch by design."""
    alone = _ghat.get((GL.ALONE_CASE, "default")) or check(GL.ALONE_CASE, dev)
    g64 = GL.case(GL.ALONE_CASE)["g64"]
    for name in (GL.BASE_CASE, "ms_64-disc-j0-B5"):
        batch = _ghat.get((name, "default")) or check(name, dev)
        for side, a, b, g in zip("xy", alone, batch, g64):
            d = float((a[0] - b[0]).abs().max())
            print(f"row 0 alone vs inside {name} side {side}: {d:.3e} = {d / float(g.abs().max()):.3e} max|g64| "
                  f"({'bitwise equal' if d == 0.0 else 'bits differ'})")
