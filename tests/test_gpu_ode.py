"""The midpoint solver of the U-Net sampler loops on the GPU (rgfm_sample_*_ode), against the float64 loops of
tests/ode_ref64.py, and its compatibility with the Euler entry points.

Nets: the generic U-Nets g16 (1x16x16, d = 256) and g24 (3x24x24, d = 1728: 13.5 column tiles of guid_apply), a few
steps each.  Bounds: TOL = 1e-4 absolute, the bound of the project's 4-step sampler tests (tests/test_gpu_cond.py,
test_gpu_cond_grad.py, test_gpu_ratio_flex.py: TOL_SAMPLER); the Euler loops measure about 1e-6 there.  Everything
"equal" is torch.equal: the same bits.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import cond_grad_ref64 as CG
import ode_ref64 as O
from helpers import GOLDEN, make_generic_unet, make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth

pytestmark = pytest.mark.gpu

TOL = 1e-4
EULER, MIDPOINT = 0, 1
STEPS, GAMMA = 4, 0.7
EINVAL, ENOMEM = -1, -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def net(tag):
    return make_generic_unet(tag)[0]


def shape_of(tag):
    n = net(tag)
    return (n.in_channels, n.img_size, n.img_size)


@functools.lru_cache(maxsize=None)
def start(tag, B, salt=0):
    """Seeded N(0, 1) start state [B, C, S, S] (fp32, CPU): shared, never modified."""
    return torch.randn(B, *shape_of(tag), generator=torch.Generator().manual_seed(7100 + 10 * B + salt))


@functools.lru_cache(maxsize=None)
def mc_set(tag, N, salt=0):
    return 0.5 * torch.randn(N, *shape_of(tag), generator=torch.Generator().manual_seed(7300 + 10 * N + salt))


@functools.lru_cache(maxsize=None)
def ratios(*shape):
    return torch.exp(0.5 * torch.randn(*shape, generator=torch.Generator().manual_seed(7500 + sum(shape))))


def err64(got, want):
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())


def f64(t):
    return t.numpy().astype(np.float64)


# ------------------------------------------------------------------ raw calls of the ten new entry points
class Raw:
    """One sampler loop through the C ABI: `ws_args` / `args` are the arguments in front of (solver, bytes) and of
    (step range, solver, ws); `old` calls the Euler entry point of the same loop."""

    def __init__(self, kind, ws_args, args, state):
        self.kind, self.ws_args, self.args, self.state = kind, ws_args, args, state
        self.L = _lib.lib()

    def ws_bytes(self, solver=None):
        nb = ctypes.c_size_t()
        if solver is None:
            rc = getattr(self.L, f"rgfm_sample_{self.kind}_workspace_bytes")(*self.ws_args, ctypes.byref(nb))
        else:
            rc = getattr(self.L, f"rgfm_sample_{self.kind}_ode_workspace_bytes")(*self.ws_args, solver, ctypes.byref(nb))
        return rc, nb.value

    def run(self, solver, b, e, ws_solver="same", dev=None):
        """rc of the call on steps [b, e); solver None: the old Euler entry point.  The workspace is sized by the query
        of `ws_solver` (default: the call's own)."""
        rc, nb = self.ws_bytes(solver if ws_solver == "same" else ws_solver)
        assert rc == 0
        ws = torch.empty(nb, dtype=torch.uint8, device=self.state[0].device)
        if solver is None:
            return getattr(self.L, f"rgfm_sample_{self.kind}")(*self.args, b, e, _p(ws), nb, _stream())
        return getattr(self.L, f"rgfm_sample_{self.kind}_ode")(*self.args, b, e, solver, _p(ws), nb, _stream())


def raw_single(tag, x, steps, dev):
    h = net(tag).to(dev)._engine.handle(dev)
    return Raw("single", (h, x.shape[0]), (h, _p(x), x.shape[0], steps), [x])


def raw_pair(x, y, mx, my, r, steps, gamma, dev):
    hx, hy = net("g16").to(dev)._engine.handle(dev), net("g24").to(dev)._engine.handle(dev)
    n = 0 if mx is None else mx.shape[0]
    r_ = Raw("pair", (hx, hy, x.shape[0], n), (hx, hy, _p(x), _p(y), _p(mx), _p(my), _p(r), n, x.shape[0], steps, gamma), [x, y])
    r_.keep = (mx, my, r)
    return r_


def raw_cond(tag, s, m, R, steps, gamma, dev):
    h = net(tag).to(dev)._engine.handle(dev)
    r_ = Raw("cond", (h, s.shape[0], m.shape[0]), (h, _p(s), _p(m), _p(R), m.shape[0], s.shape[0], steps, gamma), [s])
    r_.keep = (m, R)
    return r_


FEAT, HID, W_SEED = CG.FEAT, CG.HID, CG.W_SEED


@functools.lru_cache(maxsize=None)
def flex():
    """FlexibleRatioEstimator for x = 1x16x16 (g16), y = 3x24x24 (g24)."""
    return load_synth(M.FlexibleRatioEstimator(1, 3, FEAT, HID), W_SEED).eval()


def raw_pair_grad(x, y, steps, gamma, dev):
    rr = flex().to(dev)
    rr._engine.bind(x, y)
    hx, hy, hr = net("g16").to(dev)._engine.handle(dev), net("g24").to(dev)._engine.handle(dev), rr._engine.handle(dev)
    return Raw("pair_grad", (hx, hy, hr, x.shape[0]), (hx, hy, hr, _p(x), _p(y), x.shape[0], steps, gamma), [x, y])


@functools.lru_cache(maxsize=None)
def cond_grad_case(given):
    """cond_grad_ref64.sampler_case: (estimator, target U-Net g16, condition [3, 3, 24, 24], start state [3, 1, 16, 16]) --
    the pair (1, 16) + (3, 24) with the 3x24x24 side observed, as the estimator's x (given='x') or its y (given='y')."""
    return CG.sampler_case(given)


def raw_cond_grad(given, steps, gamma, dev):
    rr, tnet, cond, s0 = cond_grad_case(given)
    rr, tnet, s = rr.to(dev), tnet.to(dev), s0.to(dev).clone()
    ctx = rr._engine.cond_prepare(cond.to(dev), given, tuple(s0.shape[1:]))
    gi = 0 if given == "x" else 1
    rr._engine._bind_target(gi, s)
    h, hr = tnet._engine.handle(dev), rr._engine.handle(dev)
    r_ = Raw("cond_grad", (h, hr, gi, s.shape[0]), (h, hr, _p(s), _p(ctx), gi, s.shape[0], steps, gamma), [s])
    r_.keep = (ctx,)
    return r_


def pair_inputs(B, N, dev):
    x, y = start("g16", B).to(dev).clone(), start("g24", B).to(dev).clone()
    if N == 0:
        return x, y, None, None, None
    return x, y, mc_set("g16", N).to(dev), mc_set("g24", N).to(dev), ratios(N).to(dev)


def make_raw(kind, B, dev, steps=STEPS):
    """A Raw of every loop on fresh device copies of its shared start state."""
    if kind == "single":
        return raw_single("g24", start("g24", B).to(dev).clone(), steps, dev)
    if kind == "pair":
        return raw_pair(*pair_inputs(B, 7, dev), steps, GAMMA, dev)
    if kind == "cond":
        return raw_cond("g24", start("g24", B).to(dev).clone(), mc_set("g24", 7).to(dev), ratios(5, 7)[:B].contiguous().to(dev), steps, GAMMA, dev)
    if kind == "pair_grad":
        return raw_pair_grad(start("g16", B).to(dev).clone(), start("g24", B).to(dev).clone(), steps, GAMMA, dev)
    return raw_cond_grad("x", steps, GAMMA, dev)  # (its own batch of 3)


KINDS = ("single", "pair", "cond", "pair_grad", "cond_grad")


# ------------------------------------------------------------------ 4. the unguided single loop
@functools.lru_cache(maxsize=None)
def single64(tag, B, solver, steps=STEPS):
    out = O.integrate64(O.F_single(O.velocity_of(net(tag))), (f64(start(tag, B)),), steps, solver)[0]
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("tag,B", [("g16", 3), ("g24", 33)])
def test_single_midpoint_vs_float64(dev, tag, B):
    m = net(tag).to(dev)
    got = _engine.sample_single(m, start(tag, B).to(dev).clone(), STEPS, solver="midpoint")
    err = err64(got, single64(tag, B, "midpoint"))
    euler = _engine.sample_single(m, start(tag, B).to(dev).clone(), STEPS)
    gap = float((got - euler).abs().max())
    print(f"single midpoint {tag} B={B}: err vs float64 {err:.3e}  max |midpoint - euler| {gap:.3e}")
    assert err <= TOL, err
    assert gap > 1e-2, gap  # (a loop that silently runs Euler fails here)


# ------------------------------------------------------------------ 5. Euler compatibility and bit-stability
@pytest.mark.parametrize("kind", KINDS)
def test_euler_through_the_new_entry_point_is_the_old_entry_point_bitwise(dev, kind):
    old, new = make_raw(kind, 5, dev), make_raw(kind, 5, dev)
    assert old.ws_bytes(None) == new.ws_bytes(EULER)  # (the same workspace size)
    assert old.run(None, 0, STEPS) == 0 and new.run(EULER, 0, STEPS) == 0
    torch.cuda.synchronize()
    for a, b in zip(old.state, new.state):
        assert torch.equal(a, b) and torch.isfinite(a).all()


@pytest.mark.parametrize("kind", KINDS)
def test_midpoint_split_ranges_and_single_rows_are_bitwise_stable(dev, kind):
    B = 5
    whole, split = make_raw(kind, B, dev), make_raw(kind, B, dev)
    assert whole.run(MIDPOINT, 0, STEPS) == 0
    assert split.run(MIDPOINT, 0, 2) == 0 and split.run(MIDPOINT, 2, STEPS) == 0
    torch.cuda.synchronize()
    for a, b in zip(whole.state, split.state):
        assert torch.equal(a, b)
    # a row run alone (with its own ratio row / context row) has the bits it has inside the batch
    for row in (0, B - 1):
        if kind == "single":
            one = raw_single("g24", start("g24", B)[row:row + 1].to(dev).clone(), STEPS, dev)
        elif kind == "pair":
            x, y, mx, my, r = pair_inputs(B, 7, dev)
            one = raw_pair(x[row:row + 1].clone(), y[row:row + 1].clone(), mx, my, r, STEPS, GAMMA, dev)
        elif kind == "cond":
            one = raw_cond("g24", start("g24", B)[row:row + 1].to(dev).clone(), mc_set("g24", 7).to(dev),
                           ratios(5, 7)[row:row + 1].contiguous().to(dev), STEPS, GAMMA, dev)
        elif kind == "pair_grad":
            one = raw_pair_grad(start("g16", B)[row:row + 1].to(dev).clone(), start("g24", B)[row:row + 1].to(dev).clone(), STEPS, GAMMA, dev)
        else:
            continue  # (the context of a one-row batch is prepared from another condition batch: covered by the loops above)
        assert one.run(MIDPOINT, 0, STEPS) == 0
        torch.cuda.synchronize()
        for a, b in zip(whole.state, one.state):
            assert torch.equal(a[row:row + 1], b), (kind, row)


# ------------------------------------------------------------------ 6. the paired loops
@functools.lru_cache(maxsize=None)
def pair64(B, N, steps=STEPS, rng=None, guide_all=False, gamma=GAMMA):
    vx, vy = O.velocity_of(net("g16")), O.velocity_of(net("g24"))
    mx = my = r = None
    if N:
        mx, my, r = f64(mc_set("g16", N)).reshape(N, -1), f64(mc_set("g24", N)).reshape(N, -1), f64(ratios(N))
    guide = (lambda t: t > 8e-4) if guide_all else O.guided_after_eps
    b, e = rng or (0, steps)
    out = O.integrate64(O.F_pair_mc(vx, vy, mx, my, r, gamma, guide), (f64(start("g16", B)), f64(start("g24", B))), steps, "midpoint", b, e)
    for a in out:
        a.setflags(write=False)
    return out


def test_pair_without_mc_set_is_two_single_loops(dev):
    B = 3
    x, y, _, _, _ = pair_inputs(B, 0, dev)
    _engine.sample_pair(net("g16").to(dev), net("g24").to(dev), x, y, None, None, None, STEPS, 0.0, solver="midpoint")
    ex, ey = err64(x, single64("g16", B, "midpoint")), err64(y, pair64(B, 0)[1])
    print(f"pair n_mc=0: err vs float64 x {ex:.3e} y {ey:.3e}")
    assert ex <= TOL and ey <= TOL
    sx = _engine.sample_single(net("g16").to(dev), start("g16", B).to(dev).clone(), STEPS, solver="midpoint")
    sy = _engine.sample_single(net("g24").to(dev), start("g24", B).to(dev).clone(), STEPS, solver="midpoint")
    assert torch.equal(sx, x) and torch.equal(sy, y)


# (5, 7): one row tile, a ragged MC set (W4 = false); (33, 70): two row tiles, N % 32 != 0 with a 6-sample tail;
# (5, 64): N % 32 == 0, the float4 weight loads (W4 = true).  y = g24: the last column tile of guid_apply is half full.
@pytest.mark.parametrize("B,N", [(5, 7), (33, 70), (5, 64)])
def test_pair_mc_feng_midpoint_vs_float64(dev, B, N):
    x, y, mx, my, r = pair_inputs(B, N, dev)
    _engine.sample_pair(net("g16").to(dev), net("g24").to(dev), x, y, mx, my, r, STEPS, GAMMA, solver="midpoint")
    wx, wy = pair64(B, N)
    ex, ey = err64(x, wx), err64(y, wy)
    ux, uy = pair64(B, 0)
    moved = max(float(np.abs(wx - ux).max()), float(np.abs(wy - uy).max()))
    print(f"pair mc_feng midpoint B={B} N={N}: err vs float64 x {ex:.3e} y {ey:.3e}; float64 guided - unguided {moved:.3e}")
    assert moved > 100 * TOL  # (the guidance is not nothing)
    assert ex <= TOL and ey <= TOL, (ex, ey)


# ------------------------------------------------------------------ 7. the guidance threshold is per stage
def test_stage_time_threshold(dev):
    B, N, steps = 5, 7, 600
    # float64 first: guiding stage 2 of step 0 (t = 0.5 / 600 = 8.3e-4 <= 1e-3) would move the result by far more than TOL
    want, wrong = pair64(B, N, steps, (0, 2)), pair64(B, N, steps, (0, 2), guide_all=True)
    sep = max(float(np.abs(a - b).max()) for a, b in zip(want, wrong))
    unguided = pair64(B, 0, steps, (0, 2))
    moved = max(float(np.abs(a - b).max()) for a, b in zip(want, unguided))
    print(f"threshold: float64 |right - stage-2-of-step-0 guided| {sep:.3e}; |right - never guided| {moved:.3e}")
    assert sep > 10 * TOL and moved > 10 * TOL
    x, y, mx, my, r = pair_inputs(B, N, dev)
    _engine.sample_pair(net("g16").to(dev), net("g24").to(dev), x, y, mx, my, r, steps, GAMMA, 0, 2, solver="midpoint")
    ex, ey = err64(x, want[0]), err64(y, want[1])
    print(f"threshold: err vs float64 x {ex:.3e} y {ey:.3e}")
    assert ex <= TOL and ey <= TOL, (ex, ey)


# ------------------------------------------------------------------ 8. conditional and gradient loops
@functools.lru_cache(maxsize=None)
def cond64(tag, B, N, gamma):
    out = O.integrate64(O.F_cond_mc(O.velocity_of(net(tag)), f64(mc_set(tag, N)).reshape(N, -1), f64(ratios(B, N)), gamma),
                        (f64(start(tag, B)),), STEPS, "midpoint")[0]
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("tag,B,N", [("g16", 5, 7), ("g24", 33, 70)])
def test_cond_midpoint_vs_float64(dev, tag, B, N):
    m = net(tag).to(dev)
    run = lambda gamma: _engine.sample_cond(m, start(tag, B).to(dev).clone(), mc_set(tag, N).to(dev), ratios(B, N).to(dev),
                                            STEPS, gamma, solver="midpoint")
    got = run(GAMMA)
    err = err64(got, cond64(tag, B, N, GAMMA))
    print(f"cond midpoint {tag} B={B} N={N}: err vs float64 {err:.3e}")
    assert err <= TOL, err
    unguided = _engine.sample_single(m, start(tag, B).to(dev).clone(), STEPS, solver="midpoint")
    d0 = float((run(0.0) - unguided).abs().max())
    assert d0 <= 1e-6 * float(unguided.abs().max()), d0
    assert float((got - unguided).abs().max()) > 100 * TOL


@pytest.mark.parametrize("given", ["x", "y"])
def test_cond_grad_midpoint_vs_float64(dev, given):
    rr64, net64, cond, s0 = cond_grad_case(given)
    want = O.integrate64(O.F_cond_grad(O.velocity_of(net64), rr64, cond, given, GAMMA), (f64(s0),), STEPS, "midpoint")[0]
    m, rr = net64.to(dev), rr64.to(dev)

    def run(gamma):
        ctx = rr._engine.cond_prepare(cond.to(dev), given, tuple(s0.shape[1:]))
        return _engine.sample_cond_grad(m, rr, s0.to(dev).clone(), ctx, given, STEPS, gamma, solver="midpoint")
    got = run(GAMMA)
    err = err64(got, want)
    unguided = _engine.sample_single(m, s0.to(dev).clone(), STEPS, solver="midpoint")
    d0, moved = float((run(0.0) - unguided).abs().max()), float((got - unguided).abs().max())
    print(f"cond_grad midpoint given={given}: err vs float64 {err:.3e}; gamma=0 vs single {d0:.3e}; guided - unguided {moved:.3e}")
    assert err <= TOL, err
    assert d0 <= 1e-6 * float(unguided.abs().max()), d0
    assert moved > 10 * TOL, moved


def test_pair_grad_midpoint_vs_float64(dev):
    B = 3
    fx, fy, rr = net("g16").to(dev), net("g24").to(dev), flex().to(dev)
    run = lambda gamma: _engine.sample_pair_grad(fx, fy, rr, start("g16", B).to(dev).clone(), start("g24", B).to(dev).clone(), STEPS,
                                                 gamma, solver="midpoint")
    x, y = run(GAMMA)
    wx, wy = O.integrate64(O.F_pair_grad(O.velocity_of(net("g16")), O.velocity_of(net("g24")), flex(), GAMMA),
                           (f64(start("g16", B)), f64(start("g24", B))), STEPS, "midpoint")
    ex, ey = err64(x, wx), err64(y, wy)
    x0, y0 = run(0.0)
    ux = _engine.sample_single(fx, start("g16", B).to(dev).clone(), STEPS, solver="midpoint")
    uy = _engine.sample_single(fy, start("g24", B).to(dev).clone(), STEPS, solver="midpoint")
    d0 = max(float((x0 - ux).abs().max()) / float(ux.abs().max()), float((y0 - uy).abs().max()) / float(uy.abs().max()))
    moved = max(float((x - ux).abs().max()), float((y - uy).abs().max()))
    print(f"pair_grad midpoint: err vs float64 x {ex:.3e} y {ey:.3e}; gamma=0 vs single (relative) {d0:.3e}; guided - unguided {moved:.3e}")
    assert ex <= TOL and ey <= TOL, (ex, ey)
    assert d0 <= 1e-6, d0
    assert moved > 10 * TOL, moved


# ------------------------------------------------------------------ 9. truncation order on the GPU
def test_truncation_order_on_the_gpu(dev):
    ref = np.load(os.path.join(GOLDEN, "ode_g16_midpoint64.npz"))["s"][:2]  # (tests/test_ode_cpu.py recomputes it)
    m, x0 = net("g16").to(dev), torch.from_numpy(O.g16_case()[1][:2])
    mid8 = err64(_engine.sample_single(m, x0.to(dev).clone(), 8, solver="midpoint"), ref)
    eul16 = err64(_engine.sample_single(m, x0.to(dev).clone(), 16), ref)
    print(f"g16 B=2 vs float64 64-step midpoint: GPU midpoint N=8 {mid8:.3e}  GPU euler N=16 {eul16:.3e}  ratio {eul16 / mid8:.1f}")
    assert 4.0 * mid8 <= eul16, (mid8, eul16)


# ------------------------------------------------------------------ 10. errors
@pytest.mark.parametrize("kind", KINDS)
def test_unknown_solver_step_cap_and_euler_sized_workspace(dev, kind):
    r = make_raw(kind, 5, dev, steps=2100)
    before = [s.clone() for s in r.state]
    assert r.ws_bytes(2)[0] == EINVAL
    assert r.run(2, 0, 2, ws_solver=MIDPOINT) == EINVAL and b"solver" in r.L.rgfm_last_error()
    assert r.run(MIDPOINT, 0, 2049) == EINVAL and b"2048" in r.L.rgfm_last_error()  # (two table rows per step: 2048 steps per call)
    assert r.ws_bytes(EULER)[1] < r.ws_bytes(MIDPOINT)[1]
    assert r.run(MIDPOINT, 0, 2, ws_solver=EULER) == ENOMEM
    torch.cuda.synchronize()
    for a, b in zip(r.state, before):
        assert torch.equal(a, b)
    assert r.run(MIDPOINT, 0, 0) == 0  # (an empty range is fine)


# ------------------------------------------------------------------ 11. the Python surface
def test_paired_sampler_midpoint_is_the_direct_engine_calls(dev):
    from ratio_guided_multimodal_fm_amd.synth import paired_noise
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler
    fx, fy, rr = net("g16").to(dev), net("g24").to(dev), flex().to(dev)
    B, N = 4, 6
    noise = paired_noise(31, B, N, shape_of("g16"), shape_of("g24"))
    args = (fx, fy, rr, "mc_feng", GAMMA, B, STEPS, dev, N, shape_of("g16"), shape_of("g24"))
    xs, ys = paired_sampler(*args, noise=noise, verbose=False, solver="midpoint")
    x, y, mx, my = (t.to(dev, copy=True).contiguous() for t in noise)
    _engine.sample_two_streams(fx, mx, fy, my, STEPS, solver="midpoint")
    r = rr._engine.eval(mx, my, "ratio")
    _engine.sample_pair(fx, fy, x, y, mx, my, r, STEPS, GAMMA, solver="midpoint")
    assert torch.equal(xs, x) and torch.equal(ys, y)
    ex, ey = paired_sampler(*args, noise=noise, verbose=False, solver="euler")
    dx, dy = paired_sampler(*args, noise=noise, verbose=False)
    assert torch.equal(ex, dx) and torch.equal(ey, dy) and not torch.equal(ex, xs)
    gx, gy = paired_sampler(fx, fy, rr, "grad_log_ratio", GAMMA, B, STEPS, dev, 0, shape_of("g16"), shape_of("g24"), noise=noise,
                            verbose=False, solver="midpoint")
    x, y = noise[0].to(dev, copy=True).contiguous(), noise[1].to(dev, copy=True).contiguous()
    _engine.sample_pair_grad(fx, fy, rr, x, y, STEPS, GAMMA, solver="midpoint")
    assert torch.equal(gx, x) and torch.equal(gy, y)


@pytest.mark.parametrize("method", ["mc_feng", "grad_log_ratio"])
def test_sample_conditional_midpoint_is_the_direct_engine_calls(dev, method):
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional
    target, rr = net("g24").to(dev), flex().to(dev)
    B, N = 3, 6
    cond = start("g16", B, salt=9).to(dev)
    torch.cuda.manual_seed(77)
    out = sample_conditional(target, rr, cond, "x", STEPS, GAMMA, N, guidance_method=method, solver="midpoint")
    torch.cuda.manual_seed(77)
    if method == "mc_feng":  # the documented draw order: MC noise, then the start noise
        mc = torch.randn(N, *shape_of("g24"), device=dev)
        _engine.sample_single(target, mc, STEPS, solver="midpoint")
        s = torch.randn(B, *shape_of("g24"), device=dev)
        R = rr.cross_log_ratio(cond, mc).exp()
        _engine.sample_cond(target, s, mc, R, STEPS, GAMMA, solver="midpoint")
    else:
        s = torch.randn(B, *shape_of("g24"), device=dev)
        ctx = rr._engine.cond_prepare(cond, "x", shape_of("g24"))
        _engine.sample_cond_grad(target, rr, s, ctx, "x", STEPS, GAMMA, solver="midpoint")
    assert torch.equal(out, s)
    torch.cuda.manual_seed(77)
    a = sample_conditional(target, rr, cond, "x", STEPS, GAMMA, N, guidance_method=method)
    torch.cuda.manual_seed(77)
    b = sample_conditional(target, rr, cond, "x", STEPS, GAMMA, N, guidance_method=method, solver="euler")
    assert torch.equal(a, b) and not torch.equal(a, out)


def test_schedule_sample_and_flow_matching_model(dev):
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import CFMSchedule, sample_bimodal_guided
    m = make_module("unet28", dev)
    torch.cuda.manual_seed(5)
    got = CFMSchedule().sample(m, 3, STEPS, dev, solver="midpoint")
    torch.cuda.manual_seed(5)
    x = torch.randn(3, 1, 28, 28, device=dev)
    assert torch.equal(got, _engine.sample_single(m, x.clone(), STEPS, solver="midpoint"))
    torch.cuda.manual_seed(5)
    a = CFMSchedule().sample(m, 3, STEPS, dev)
    torch.cuda.manual_seed(5)
    b = CFMSchedule().sample(m, 3, STEPS, dev, solver="euler")
    assert torch.equal(a, b) and torch.equal(a, _engine.sample_single(m, x.clone(), STEPS)) and not torch.equal(a, got)
    fm = make_module("fm_original", dev)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        CFMSchedule().sample(fm, 2, 2, dev, solver="midpoint")
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        sample_bimodal_guided(fm, make_module("fm_original_y", dev), None, "none", 0.0, 2, 2, dev, 4, solver="midpoint")
    assert CFMSchedule().sample(fm, 2, 2, dev).shape == (2, 1, 28, 28)  # (Euler is still there)


def test_cli_solver_midpoint_equals_the_direct_call(dev, tmp_path, monkeypatch):
    import ratio_guided_multimodal_fm_amd as R
    from ratio_guided_multimodal_fm_amd import sample_mnist_svhn
    ck = tmp_path / "checkpoints"
    ck.mkdir()
    fm, fs, rr = make_module("mnist32"), make_module("svhn"), make_module("ratio_ms")
    torch.save({"epoch": 1, "model_state_dict": fm.state_dict(), "best_loss": 0.5}, ck / "flow_mnist32_best.pth")
    torch.save({"epoch": 1, "model_state_dict": fs.state_dict(), "best_loss": 0.5}, ck / "flow_svhn_best.pth")
    torch.save(rr.state_dict(), ck / "ratio_disc_mnist_svhn_best.pth")
    monkeypatch.chdir(tmp_path)
    assert sample_mnist_svhn.main(["--guidance_method", "mc_feng", "--guidance_strength", "0.5", "--num_steps", "3", "--num_samples", "3",
                                   "--mc_batch_size", "5", "--seed", "9", "--solver", "midpoint"]) == 0
    saved = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_mc_feng_gamma0.5.pt")
    R.utils.set_seed(9)
    xs, ys = sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(fm.to(dev), fs.to(dev), rr.to(dev), "mc_feng", 0.5, 3, 3, dev, 5,
                                                                solver="midpoint")
    assert torch.equal(saved["mnist"], xs.cpu()) and torch.equal(saved["svhn"], ys.cpu())
    R.utils.set_seed(9)
    ex, _ = sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(fm.to(dev), fs.to(dev), rr.to(dev), "mc_feng", 0.5, 3, 3, dev, 5)
    assert not torch.equal(ex, xs)
