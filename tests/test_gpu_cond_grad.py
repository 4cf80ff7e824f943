"""Conditional sampling with gradient log-ratio guidance on the GPU: the context of the observed side
(rgfm_ratio_cond_prepare), the one-sided gradient (rgfm_ratio_grad_log_ratio_cond), the one-net loop
(rgfm_sample_cond_grad) and the Python surface (grad_log_ratio_given, sample_conditional(guidance_method=
'grad_log_ratio'), the --given / --condition / --guidance_method CLI), each against float64.

Yardstick: tests/cond_grad_ref64.py -- ratio_ref64 / ratio_flex_ref64 under torch.autograd.grad with only the target
requiring grad, unet_ref64 for the velocity.  tests/test_cond_grad_cpu.py ties its factorised form to the two-sided
gradient (1e-12) and shows the sampler cases' guidance term in float64 alone.

Bounds: the project's existing ones.  Gradients: max |g - g64| <= 1e-4 max |g64| (TOL_GRAD); log-ratio 1e-5; sampler
state 1e-4 (TOL_SAMPLER).  One-sided against two-sided: each is within TOL_GRAD of float64, so 2 x TOL_GRAD.

Data seeds.  A max-pool whose two largest window elements nearly tie may route differently in another arithmetic: a
discontinuity of the function, not an arithmetic error (tests/test_gpu_ratio_flex.py).  The flexible cases reuse that
file's searched SEEDS (the encoders' synthetic weights do not depend on hidden_dim, so they hold at 384 and 1024 too).
The two fixed-kind seeds are, of 24 tried each, the ones with the largest ratio of the smallest float64 window gap to
the largest fp32-vs-float64 deviation of a pre-pool map (fp32 torch on the CPU: 1.6 and 0.7; the fp32 encoders pick the
float64 argmax in every one of the 308 k and 781 k windows).  The sampler seeds: cond_grad_ref64.SAMPLER_CASES.

Measured on an MI355X: see DESIGN.md section 11."""
import ctypes

import numpy as np
import pytest
import torch

import cond_grad_ref64 as CG
import test_gpu_ratio_flex as TF
import unet_ref64 as U
from helpers import make_generic_unet, make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth
from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional

pytestmark = pytest.mark.gpu

TOL_EVAL, TOL_GRAD, TOL_SAMPLER = 1e-5, 1e-4, 1e-4
FEAT, W_SEED = TF.FEAT, TF.W_SEED
SENTINEL, PAD = -7777.0, 256
FIXED = {"ratio_ms": ("mnist_svhn", (1, 32, 32), (3, 32, 32), 7, 6007), "ratio28": ("mnist28", (1, 28, 28), (1, 28, 28), 37, 6113)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def flex_module(ci, hid, dev):
    (xc, _), (yc, _) = TF.CASES[ci]
    return load_synth(M.FlexibleRatioEstimator(xc, yc, FEAT, hid), W_SEED).eval().to(dev)


def fixed_inputs(tag):
    _, sx, sy, B, seed = FIXED[tag]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, *sx, generator=g), torch.randn(B, *sy, generator=g)


_ref = {}


def ref64(key, m, x, y):
    """float64 one-sided gradients and log-ratios of a case, {(given, loss): (g, lr)}: computed once, shared, never modified."""
    if key not in _ref:
        kind, sd = CG.kind_of(m), CG.params64(m)
        _ref[key] = {(given, lt): CG.grad_given64(kind, sd, *((x, y) if given == "x" else (y, x)), given, lt)
                     for given in ("x", "y") for lt in ("disc", "rulsif")}
    return _ref[key]


def one_sided(m, cond, target, given):
    eng = m._engine
    ctx = eng.cond_prepare(cond, given, tuple(target.shape[1:]))
    return eng.grad_log_ratio_cond(ctx, given, target)


def check_case(m, x, y, ref, what, dev):
    xd, yd = x.to(dev), y.to(dev)
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        for given, cond, target in (("x", xd, yd), ("y", yd, xd)):
            g, lr = one_sided(m, cond, target, given)
            g64, lr64 = ref[(given, lt)]
            assert g.shape == target.shape and lr.shape == (x.shape[0],)
            TF.assert_close(g, g64, f"{what} {lt} given={given} g_target", TOL_GRAD)
            elr = float((lr.cpu().double() - lr64).abs().max())
            print(f"{what} {lt} given={given} log_ratio: err {elr:.3e}")
            assert elr <= TOL_EVAL, elr
            assert torch.equal(m.grad_log_ratio_given(cond, target, given), g)  # the module-level API
    m.loss_type = "disc"


# ------------------------------------------------------------------ 1. the one-sided gradient against float64
@pytest.mark.parametrize("ci,B", [(ci, B) for ci in (0, 1, 3) for B in (1, 5)])
def test_flexible_one_sided_gradient_vs_float64(dev, ci, B):
    x, y = TF.inputs(ci, B)
    m = flex_module(ci, TF.HID, dev)
    check_case(m, x, y, ref64(("flex", ci, B, TF.HID), m, x, y), f"flexible case {ci} B {B}", dev)


@pytest.mark.parametrize("ci,hid", [(1, 384), (3, 1024)])
def test_flexible_wide_hidden_layers_vs_float64(dev, ci, hid):
    """hidden_dim 384: 96 float4 per row, the second group of 64 lanes half filled; 1024: all four groups full (128, the
    other cases, leaves half a wave idle)."""
    x, y = TF.inputs(ci, 5)
    m = flex_module(ci, hid, dev)
    check_case(m, x, y, ref64(("flex", ci, 5, hid), m, x, y), f"flexible case {ci} hidden {hid}", dev)


@pytest.mark.parametrize("tag", list(FIXED))
def test_fixed_kinds_one_sided_gradient_vs_float64(dev, tag):
    x, y = fixed_inputs(tag)
    check_case(make_module(tag, dev), x, y, ref64((tag,), make_module(tag), x, y), f"{tag} B {x.shape[0]}", dev)


# ------------------------------------------------------------------ 2. agreement with the two-sided gradient
@pytest.mark.parametrize("case", ["flex3", "ratio_ms", "ratio28"])
def test_one_sided_agrees_with_two_sided_and_is_deterministic(dev, case):
    if case == "flex3":
        x, y = TF.inputs(3, 5)
        m, key = flex_module(3, TF.HID, dev), ("flex", 3, 5, TF.HID)
    else:
        x, y = fixed_inputs(case)
        m, key = make_module(case, dev), (case,)
    ref = ref64(key, flex_module(3, TF.HID, "cpu") if case == "flex3" else make_module(case), x, y)
    xd, yd = x.to(dev), y.to(dev)
    gx, gy = m.grad_log_ratio(xd, yd)
    for given, cond, target, two in (("x", xd, yd, gy), ("y", yd, xd, gx)):
        g, lr = one_sided(m, cond, target, given)
        scale = float(ref[(given, "disc")][0].abs().max())
        diff = float((g - two).abs().max())
        print(f"{case} given={given}: |one-sided - two-sided| {diff:.3e} = {diff / scale:.3e} max|g64|, bitwise {torch.equal(g, two)}")
        assert diff <= 2 * TOL_GRAD * scale, (diff, scale)
        g2, lr2 = one_sided(m, cond, target, given)
        assert torch.equal(g, g2) and torch.equal(lr, lr2)


def test_raw_calls_bounds_and_argument_errors(dev):
    """The raw entry points into the middle of larger buffers with the workspace exactly as asked for: nothing outside
    is written; a workspace one byte short is RGFM_ENOMEM, given = 2 and n = 0 are RGFM_EINVAL."""
    ci, B = 1, 5
    x, y = (t.to(dev) for t in TF.inputs(ci, B))
    m = flex_module(ci, TF.HID, dev)
    m(x, y)  # binds the sizes
    L, h = _lib.lib(), m._engine.handle(dev)
    nb = ctypes.c_size_t()
    assert L.rgfm_ratio_cond_prepare_workspace_bytes(h, 2, B, ctypes.byref(nb)) == -1
    assert L.rgfm_ratio_cond_prepare_workspace_bytes(h, 0, 0, ctypes.byref(nb)) == -1
    assert L.rgfm_ratio_grad_cond_workspace_bytes(h, -1, B, ctypes.byref(nb)) == -1
    _lib.check(L.rgfm_ratio_cond_prepare_workspace_bytes(h, 0, B, ctypes.byref(nb)))
    ws = torch.full((nb.value // 4,), float("nan"), device=dev)
    big = torch.full((PAD + B * TF.HID + PAD,), SENTINEL, device=dev)
    assert L.rgfm_ratio_cond_prepare(h, _p(x), 0, B, _p(big[PAD:]), _p(ws), nb.value - 1, _stream()) == -2
    _lib.check(L.rgfm_ratio_cond_prepare(h, _p(x), 0, B, _p(big[PAD:]), _p(ws), nb.value, _stream()))
    torch.cuda.synchronize()
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all())
    ctx = big[PAD:-PAD].view(B, TF.HID).clone()
    assert torch.equal(ctx, m._engine.cond_prepare(x, "x", tuple(y.shape[1:])))
    _lib.check(L.rgfm_ratio_grad_cond_workspace_bytes(h, 0, B, ctypes.byref(nb)))
    ws = torch.full((nb.value // 4,), float("nan"), device=dev)
    gbig = torch.full((PAD + y.numel() + PAD,), SENTINEL, device=dev)
    call = lambda nbytes, lr: L.rgfm_ratio_grad_log_ratio_cond(h, _p(ctx), 0, _p(y), _p(gbig[PAD:]), lr, B, _p(ws), nbytes, _stream())
    assert call(nb.value - 1, None) == -2
    _lib.check(call(nb.value, None))  # log_ratio_out is optional
    torch.cuda.synchronize()
    assert bool((gbig[:PAD] == SENTINEL).all()) and bool((gbig[-PAD:] == SENTINEL).all())
    assert torch.equal(gbig[PAD:-PAD].view_as(y), m._engine.grad_log_ratio_cond(ctx, "x", y)[0])


# ------------------------------------------------------------------ 3. parameter update
def test_context_follows_an_in_place_parameter_update(dev):
    """rgfm_ratio_update_params refreshes the column slices cond_prepare reads: after an in-place edit of the first score
    Linear the same handle prepares the float64 context of the new weights; the context prepared before is stale."""
    ci, B = 1, 5
    x, y = TF.inputs(ci, B)
    m = flex_module(ci, TF.HID, dev)
    xd, yd = x.to(dev), y.to(dev)
    before = {g: m._engine.cond_prepare(c, g, tuple(t.shape[1:])).clone() for g, c, t in (("x", xd, yd), ("y", yd, xd))}
    h0 = m._engine.handle(dev).value
    with torch.no_grad():
        m.score_net[0].weight.mul_(0.5)
        m.score_net[0].weight[:, FEAT:].add_(0.01)
        m.score_net[0].bias.add_(0.02)
    sd = CG.params64(m)
    for given, c, t, c64 in (("x", xd, yd, x), ("y", yd, xd, y)):
        after = m._engine.cond_prepare(c, given, tuple(t.shape[1:]))
        assert m._engine.handle(dev).value == h0
        want = CG.context64("flexible", sd, c64.double(), given)
        err, moved = float((after.cpu().double() - want).abs().max()), float((before[given].cpu().double() - want).abs().max())
        print(f"update given={given}: new context err {err:.3e}, the old context is off by {moved:.3e}")
        assert err <= TOL_EVAL, err
        assert moved > 1e-3, moved
        g, _ = m._engine.grad_log_ratio_cond(after, given, t)
        TF.assert_close(g, CG.grad_given64("flexible", sd, c64, t.cpu(), given, "disc")[0], f"update given={given} g_target", TOL_GRAD)


# ------------------------------------------------------------------ 4. the sampler loop
def run_loop(net, rr, cond, s0, given, gamma, dev, ranges=((0, CG.STEPS_S),)):
    s = s0.to(dev).clone()
    ctx = rr._engine.cond_prepare(cond.to(dev), given, tuple(s0.shape[1:]))
    for b, e in ranges:
        _engine.sample_cond_grad(net, rr, s, ctx, given, CG.STEPS_S, gamma, b, e)
    return s


@pytest.mark.parametrize("given", ["x", "y"])
def test_sample_cond_grad_vs_float64_split_and_gamma(dev, given):
    rr, net, cond, s0 = CG.sampler_case(given)
    rr, net = rr.to(dev), net.to(dev)
    got = run_loop(net, rr, cond, s0, given, CG.GAMMA_S, dev)
    err = float((got.cpu().double() - CG.sampler_loop64(given, CG.GAMMA_S)).abs().max())
    print(f"sample_cond_grad given={given} gamma={CG.GAMMA_S}: err vs float64 {err:.3e}")
    assert err <= TOL_SAMPLER, err
    # splitting the integration at a step boundary changes no bit
    assert torch.equal(run_loop(net, rr, cond, s0, given, CG.GAMMA_S, dev, ((0, 2), (2, CG.STEPS_S))), got)
    unguided = _engine.sample_single(net, s0.to(dev).clone(), CG.STEPS_S)
    zero = run_loop(net, rr, cond, s0, given, 0.0, dev)
    e0 = float((zero.cpu().double() - CG.sampler_loop64(given, 0.0)).abs().max())
    d0, scale = float((zero - unguided).abs().max()), float(unguided.abs().max())
    dist = float((got - unguided).abs().max())
    print(f"sample_cond_grad given={given}: gamma 0 err vs float64 {e0:.3e}, |gamma 0 - sample_single| {d0:.3e} = {d0 / scale:.3e} max|s|, "
          f"|gamma {CG.GAMMA_S} - sample_single| {dist:.3e}")
    assert e0 <= TOL_SAMPLER, e0
    assert d0 <= 1e-6 * scale, (d0, scale)
    assert dist > 100 * TOL_SAMPLER, dist  # (a missing guidance term does not pass)


def test_sample_cond_grad_wrong_target_shape_is_an_error_not_a_fault(dev):
    rr, net, cond, s0 = CG.sampler_case("x")  # the estimator's y is 1x16x16
    rr, net = rr.to(dev), net.to(dev)
    ctx = rr._engine.cond_prepare(cond.to(dev), "x", tuple(s0.shape[1:]))
    hr = rr._engine.handle(dev)  # built for 3x24x24 + 1x16x16
    wrong = make_generic_unet("g24", dev)[0]  # 3x24x24
    s = torch.zeros(CG.B_S, 3, 24, 24, device=dev)
    L, nb = _lib.lib(), ctypes.c_size_t()
    with pytest.raises(_lib.RgfmError, match="1x16x16"):
        _lib.check(L.rgfm_sample_cond_grad_workspace_bytes(wrong._engine.handle(dev), hr, 0, CG.B_S, ctypes.byref(nb)))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.RgfmError, match="1x16x16"):
        _lib.check(L.rgfm_sample_cond_grad(wrong._engine.handle(dev), hr, _p(s), _p(ctx), 0, CG.B_S, 4, 0.7, 0, 4, _p(ws), ws.numel(), None))
    torch.cuda.synchronize()
    assert not s.any()
    with pytest.raises(_lib.RgfmError):  # the Python side: the estimator's y has one channel
        _engine.sample_cond_grad(wrong, rr, s, ctx, "x", 4, 0.7)
    with pytest.raises(_lib.RgfmError):  # a fixed kind with a U-Net of another size
        r28 = make_module("ratio28", dev)
        c28 = r28._engine.cond_prepare(torch.zeros(CG.B_S, 1, 28, 28, device=dev), "x")
        _engine.sample_cond_grad(net, r28, s0.to(dev).clone(), c28, "x", 4, 0.7)
    # the step-range checks of rgfm_sample_pair_grad
    h = net._engine.handle(dev)
    sd_ = s0.to(dev).clone()
    _lib.check(L.rgfm_sample_cond_grad_workspace_bytes(h, hr, 0, CG.B_S, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    call = lambda steps, b, e, nbytes: L.rgfm_sample_cond_grad(h, hr, _p(sd_), _p(ctx), 0, CG.B_S, steps, 0.7, b, e, _p(ws), nbytes, _stream())
    assert call(4, 2, 1, nb.value) == -1 and call(4, 0, 5, nb.value) == -1 and call(5000, 0, 4097, nb.value) == -1
    assert call(4, 0, 4, nb.value - 1) == -2
    torch.cuda.synchronize()
    assert torch.equal(sd_, s0.to(dev))


# ------------------------------------------------------------------ 5. Python end to end
@pytest.mark.parametrize("given", ["x", "y"])
def test_sample_conditional_grad_log_ratio_vs_float64_composition(dev, given):
    fx, fy, rr = TF.nets(dev)  # 3x16x16 + 1x16x16
    target = fy if given == "x" else fx
    cshape, tshape = ((3, 16, 16), (1, 16, 16)) if given == "x" else ((1, 16, 16), (3, 16, 16))
    B, S, gamma = 4, 4, 0.7
    cond = torch.randn(B, *cshape, generator=torch.Generator().manual_seed(61))
    torch.cuda.manual_seed(123)
    s0 = torch.randn(B, *tshape, device=dev)  # the first draw of the seeded generator: no MC noise comes before it
    torch.cuda.manual_seed(123)
    out = sample_conditional(target, rr, cond.to(dev), given, S, gamma, mc_batch_size=7, guidance_method="grad_log_ratio")
    assert out.shape == (B, *tshape)
    after = torch.randn(3, device=dev)
    torch.cuda.manual_seed(123)
    torch.randn(B, *tshape, device=dev)
    assert torch.equal(after, torch.randn(3, device=dev))  # ... and none after it
    cfg, usd, sdr = U.cfg_of(target), U.params64(target, requires_grad=False), CG.params64(rr)
    vel = lambda s, t: U.forward64(cfg, usd, s, torch.tensor([t]))
    grad = lambda s: CG.grad_given64("flexible", sdr, cond, s, given, "disc")[0]
    want = CG.sample_cond_grad64(vel, grad, s0.cpu(), S, gamma)
    err = float((out.cpu().double() - want).abs().max())
    print(f"sample_conditional grad_log_ratio given={given}: err vs float64 {err:.3e}")
    assert err <= TOL_SAMPLER, err
    # mc_batch_size and mc_samples are ignored
    torch.cuda.manual_seed(123)
    again = sample_conditional(target, rr, cond.to(dev), given, S, gamma, mc_batch_size=2, mc_samples=torch.zeros(2, *tshape),
                               guidance_method="grad_log_ratio")
    assert torch.equal(again, out)


def test_default_method_is_mc_feng_bit_for_bit(dev):
    fx, fy, rr = TF.nets(dev)
    cond = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(62)).to(dev)
    torch.cuda.manual_seed(5)
    a = sample_conditional(fy, rr, cond, "x", 4, 0.7, 6)
    torch.cuda.manual_seed(5)
    b = sample_conditional(fy, rr, cond, "x", 4, 0.7, 6, guidance_method="mc_feng")
    torch.cuda.manual_seed(5)
    c = sample_conditional(fy, rr, cond, "x", 4, 0.7, 6, guidance_method="grad_log_ratio")
    assert torch.equal(a, b) and not torch.equal(a, c)
    with pytest.raises(ValueError, match="guidance_method"):
        sample_conditional(fy, rr, cond, "x", 4, 0.7, 6, guidance_method="none")
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        sample_conditional(make_module("fm_original", dev), make_module("ratio28", dev), torch.zeros(2, 1, 28, 28, device=dev), "x", 2,
                           0.5, 3, guidance_method="grad_log_ratio")


# ------------------------------------------------------------------ 6. the CLI
def test_cli_given_mnist_grad_log_ratio_equals_the_direct_call(dev, tmp_path, monkeypatch):
    import ratio_guided_multimodal_fm_amd as R
    from ratio_guided_multimodal_fm_amd import sample_mnist_svhn
    ck = tmp_path / "checkpoints"
    ck.mkdir()
    fm, fs, rr = make_module("mnist32"), make_module("svhn"), make_module("ratio_ms")
    torch.save({"epoch": 1, "model_state_dict": fm.state_dict(), "best_loss": 0.5}, ck / "flow_mnist32_best.pth")
    torch.save({"epoch": 1, "model_state_dict": fs.state_dict(), "best_loss": 0.5}, ck / "flow_svhn_best.pth")
    torch.save(rr.state_dict(), ck / "ratio_disc_mnist_svhn_best.pth")
    cond = torch.randn(3, 1, 32, 32, generator=torch.Generator().manual_seed(8))
    np.save(tmp_path / "cond.npy", cond.numpy())
    monkeypatch.chdir(tmp_path)
    assert sample_mnist_svhn.main(["--given", "mnist", "--condition", "cond.npy", "--guidance_method", "grad_log_ratio",
                                   "--guidance_strength", "0.5", "--num_steps", "4", "--seed", "9"]) == 0
    saved = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_given_mnist_grad_log_ratio_gamma0.5.pt")
    R.utils.set_seed(9)
    want = sample_conditional(fs.to(dev), rr.to(dev), cond.to(dev), "x", 4, 0.5, device=dev, guidance_method="grad_log_ratio")
    assert saved["svhn"].shape == (3, 3, 32, 32)
    assert torch.equal(saved["svhn"], want.cpu()) and torch.equal(saved["mnist"], cond)
    R.utils.set_seed(9)
    mc = sample_conditional(fs.to(dev), rr.to(dev), cond.to(dev), "x", 4, 0.5, 5, device=dev)
    assert not torch.equal(mc, want)  # (the MC route is another sampler)
