"""The stochastic sampler step on the GPU (include/rgfm.h, "Stochastic sampling"; rgfm_sample_*_sde, rgfm_sde_noise)
against the float64 restatement of tests/sde_ref64.py, which tests/test_sde_cpu.py pins.

Nets and shapes: those of tests/test_gpu_ode.py -- the generic U-Nets g16 (1x16x16, D = 256) and g24 (3x24x24,
D = 1728), B = 3, 4 steps; the raw callers are tests/sde_cases.py.

Bounds.  Noise: 1e-5 absolute (about 29 fp32 ulps of the largest magnitude, 5.77: the integer part and u1, u2 are exact
in fp32, what remains is a few ulps each of logf, sqrtf, sincospif and the product).  Loops: TOL = 1e-4 absolute, the
bound of the project's 4-step sampler tests (TOL_SAMPLER).  The closed form (a net whose velocity is 0): 1e-5.
Everything "equal" is torch.equal: the same bits.
Measured on one MI355X: noise worst 7.8e-7 (n = 2^20 + 3), loops worst 2.1e-6 (the single loop at eta = 4), closed form
3.2e-7.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import cond_grad_ref64 as CG
import diag_ref64 as D
import guidance_cross_ref64 as X
import guidance_ref64 as G
import ode_ref64 as O
import sde_cases as C
import sde_ref64 as S
import test_gpu_ode as T
from helpers import make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib

pytestmark = pytest.mark.gpu

TOL, TOL_NOISE, TOL_CLOSED = 1e-4, 1e-5, 1e-5
EULER, MIDPOINT = 0, 1
STEPS, GAMMA, B, N = T.STEPS, T.GAMMA, 3, C.N_MC
ETA, SEED = 0.8, 2024
EINVAL, ENOMEM = -1, -2
f64, err64, net = T.f64, T.err64, T.net


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def sync_states(*raws):
    torch.cuda.synchronize()
    return [[s.clone() for s in r.state] for r in raws]


# ------------------------------------------------------------------ 1. the noise
def gpu_noise(seed, m, k, n, dev, out=None):
    out = torch.full((n,), float("nan"), device=dev) if out is None else out
    assert _lib.lib().rgfm_sde_noise(seed % (1 << 64), m, k, n, C._p(out), T._stream()) == 0
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 7, 63, 64, 65, 255, 257, 4099, (1 << 20) + 3])
def test_noise_vs_float64(dev, n):
    worst = 0.0
    for seed in (0, 2024, 2 ** 63 + 5, 2 ** 64 - 1):
        for m in (0, 1):
            for k in (0, 1, 4095):
                got = gpu_noise(seed, m, k, n, dev)
                assert torch.isfinite(got).all(), (seed, m, k)
                worst = max(worst, float(np.abs(got.cpu().numpy().astype(np.float64) - S.noise(seed, m, k, n)).max()))
    print(f"rgfm_sde_noise n={n}: worst |err| vs float64 {worst:.3e}")
    assert worst <= TOL_NOISE, worst


def test_noise_prefix_alignment_and_bounds(dev):
    full = gpu_noise(2024, 1, 3, 4099, dev)
    for m in (1, 2, 3, 255):
        assert torch.equal(full[:m], gpu_noise(2024, 1, 3, m, dev)), m
    # a buffer that is not 16-byte aligned takes the element-wise path: the same bits, and nothing outside [0, n)
    buf = torch.full((4099 + 9,), -7.0, device=dev)
    gpu_noise(2024, 1, 3, 4099, dev, out=buf[5:5 + 4099])
    assert torch.equal(buf[5:5 + 4099], full) and bool((buf[:5] == -7.0).all()) and bool((buf[5 + 4099:] == -7.0).all())
    buf = torch.full((64 + 8,), -7.0, device=dev)
    gpu_noise(2024, 1, 3, 63, dev, out=buf[4:4 + 63])  # (16-byte aligned, a tail of 7)
    assert torch.equal(buf[4:4 + 63], full[:63]) and bool((buf[:4] == -7.0).all()) and bool((buf[4 + 63:] == -7.0).all())
    assert float(full.abs().max()) <= 5.78
    assert not torch.equal(full, gpu_noise(2024, 0, 3, 4099, dev)) and not torch.equal(full, gpu_noise(2024, 1, 2, 4099, dev))
    L = _lib.lib()
    assert L.rgfm_sde_noise(1, 2, 0, 4, C._p(full), T._stream()) == EINVAL and L.rgfm_sde_noise(1, 0, -1, 4, C._p(full), T._stream()) == EINVAL


# ------------------------------------------------------------------ 2. the off-switch
@pytest.mark.parametrize("kind", C.KINDS)
def test_null_and_eta_zero_are_the_namesake_bitwise(dev, kind):
    old, null, zero = (C.make(kind, B, dev) for _ in range(3))
    assert old.run(0, STEPS, namesake=True) == 0
    assert null.run(0, STEPS, None) == 0       # (in the namesake's workspace: nothing more is asked for)
    assert zero.run(0, STEPS, (0.0, 99)) == 0
    a, b, c = sync_states(old, null, zero)
    start = sync_states(C.make(kind, B, dev))[0]
    for s0, u, v, w in zip(start, a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w) and torch.isfinite(u).all() and not torch.equal(u, s0)


# ------------------------------------------------------------------ 3. each loop against float64
def vel(tag):
    return O.velocity_of(net(tag))


def mc64(n=N, cross=False):
    mx, my = f64(T.mc_set("g16", n)).reshape(n, -1), f64(T.mc_set("g24", n)).reshape(n, -1)
    return mx, my, f64(T.ratios(n, n) if cross else T.ratios(n))


def F_pair_cross(velx, vely, mx, my, R, gamma):
    def F(s, t):
        x, y = s
        vx, vy = np.asarray(velx(x, t), np.float64), np.asarray(vely(y, t), np.float64)
        if O.guided_after_eps(t):
            n = x.shape[0]
            gx, gy = X.cross64(x.reshape(n, -1), y.reshape(n, -1), vx.reshape(n, -1), vy.reshape(n, -1), mx, my, R, t, gamma)[:2]
            vx, vy = gx.reshape(x.shape), gy.reshape(y.shape)
        return vx, vy
    return F


def F_of(kind):
    if kind == "single":
        return O.F_single(vel("g24")), ("g24",)
    if kind == "pair":
        return O.F_pair_mc(vel("g16"), vel("g24"), *mc64(), GAMMA), ("g16", "g24")
    if kind == "pair_n0":
        return O.F_pair_mc(vel("g16"), vel("g24"), None, None, None, GAMMA), ("g16", "g24")
    if kind == "pair_cross":
        return F_pair_cross(vel("g16"), vel("g24"), *mc64(cross=True), GAMMA), ("g16", "g24")
    if kind == "cond":
        return O.F_cond_mc(vel("g24"), f64(T.mc_set("g24", N)).reshape(N, -1), f64(T.ratios(5, N)[:B]), GAMMA), ("g24",)
    assert kind == "pair_grad"
    return O.F_pair_grad(vel("g16"), vel("g24"), T.flex(), GAMMA), ("g16", "g24")


@functools.lru_cache(maxsize=None)
def want64(kind, eta, seed=SEED, rng=(0, STEPS)):
    """float64 end state of the loop `kind` from test_gpu_ode's shared start states: computed once, shared, read-only."""
    if kind == "cond_grad":
        rr64, net64, cond, s0 = T.cond_grad_case("x")
        F, state = O.F_cond_grad(O.velocity_of(net64), rr64, cond, "x", GAMMA), (f64(s0),)
    else:
        F, tags = F_of(kind)
        state = tuple(f64(T.start(tag, B)) for tag in tags)
    out = S.integrate_sde64(F, state, STEPS, eta, seed, *rng)
    for a in out:
        a.setflags(write=False)
    return out


CASES3 = [("single", ETA), ("single", 4.0), ("pair", ETA), ("pair_n0", ETA), ("pair_cross", ETA), ("cond", ETA), ("pair_grad", ETA),
          ("cond_grad", ETA)]


@pytest.mark.parametrize("kind,eta", CASES3)
def test_loop_vs_float64(dev, kind, eta):
    raw = C.make("pair", B, dev, n_mc=0) if kind == "pair_n0" else C.make(kind, B, dev)
    assert raw.run(0, STEPS, (eta, SEED)) == 0
    torch.cuda.synchronize()
    want, ode = want64(kind, eta), want64(kind, 0.0)
    errs = [err64(a, w) for a, w in zip(raw.state, want)]
    moved = max(float(np.abs(w - o).max()) for w, o in zip(want, ode))
    print(f"{kind} eta={eta}: err vs float64 {' '.join(f'{e:.3e}' for e in errs)}; float64 |sde - ode| {moved:.3e}")
    assert moved > 1000 * TOL  # (the noise is not nothing)
    assert max(errs) <= TOL, errs


def test_pair_grad_with_gamma_rows_and_a_stage_switched_off_vs_float64(dev):
    rows64, scale = np.array([0.3, 1.0, 1.6]), [1.0, 0.0, 0.5, 1.5]
    rr = T.flex()
    kind, sd = CG.kind_of(rr), CG.params64(rr)

    def F(s, t):
        k = int(round(t * STEPS))
        x, y = s
        vx, vy = vel("g16")(x, t), vel("g24")(y, t)
        if scale[k] == 0.0:
            return vx, vy
        gx, gy, _ = CG.grad_both64(kind, sd, torch.from_numpy(x), torch.from_numpy(y), "disc")
        g = (np.float32(rows64).astype(np.float64) * scale[k])[:, None, None, None]
        return vx + g * gx.numpy(), vy + g * gy.numpy()
    want = S.integrate_sde64(F, (f64(T.start("g16", B)), f64(T.start("g24", B))), STEPS, ETA, SEED)
    raw = C.make("pair_grad", B, dev)
    rows = torch.tensor(rows64, dtype=torch.float32, device=dev)
    assert raw.run(0, STEPS, (ETA, SEED), rows=rows, scale=scale) == 0
    errs = [err64(a, w) for a, w in zip(raw.state, want)]
    plain = want64("pair_grad", ETA)
    moved = max(float(np.abs(w - p).max()) for w, p in zip(want, plain))
    print(f"pair_grad rows + scale, eta={ETA}: err vs float64 {errs[0]:.3e} {errs[1]:.3e}; float64 |rows - scalar| {moved:.3e}")
    assert moved > 10 * TOL and max(errs) <= TOL, errs


def test_cond_with_diagnostics_keeps_the_bits_and_records_the_float64_stage(dev):
    """The one-sided MC loop with the sink: the samples keep their bits, and the record of stage 2 is the float64
    record at the fp32 state in front of it (the guidance is evaluated at the old state, whatever the pre-update),
    within the bounds of tests/test_gpu_diag.py's own stage test."""
    plain, diag = C.make("cond", B, dev), C.make("cond", B, dev)
    rec = torch.full((STEPS, B, 8), -7777.0, device=dev)
    assert plain.run(0, STEPS, (ETA, SEED)) == 0 and diag.run(0, STEPS, (ETA, SEED), diag=rec) == 0
    torch.cuda.synchronize()
    assert torch.equal(plain.state[0], diag.state[0])
    assert not rec[0].any() and bool((rec[1:, :, 0] >= 1.0).all())  # (stage 0 is unguided: a zero record; then 1 <= ess)
    step = C.make("cond", B, dev)
    assert step.run(0, 2, (ETA, SEED)) == 0
    torch.cuda.synchronize()
    s = step.state[0].clone()
    one = torch.full((1, B, 8), -7777.0, device=dev)
    assert step.run(2, 3, (ETA, SEED), diag=one) == 0
    torch.cuda.synchronize()
    assert torch.equal(one[0], rec[2])
    t = 2 * (1.0 / STEPS)
    s64 = f64(s.cpu())
    v = vel("g24")(s64, t)
    m, R = step.keep
    inp = {"s": s64.reshape(B, -1), "v": v.reshape(B, -1), "m": f64(m.cpu()).reshape(N, -1), "R": f64(R.cpu())}
    ref = D.diag_cond64(inp, t)
    tw = min(G.tol_w(0.5, c) for c in G.CENTRES)
    v_extra = np.sqrt(1728) * 1e-5 * max(1.0, float(np.abs(v).max()))
    bnd = D.bounds({"mx": inp["m"], "my": np.zeros(1)}, ref, N, (1728,), t, tw, (v_extra,))
    D.check(one[0].cpu().numpy(), ref, bnd, "cond sde loop, step 2")


# ------------------------------------------------------------------ 4. composition and determinism
@pytest.mark.parametrize("kind", C.KINDS)
def test_split_ranges_same_seed_and_other_seed(dev, kind):
    whole, split, again, other = (C.make(kind, B, dev) for _ in range(4))
    assert whole.run(0, STEPS, (ETA, 1)) == 0
    assert split.run(0, 2, (ETA, 1)) == 0 and split.run(2, STEPS, (ETA, 1)) == 0
    assert again.run(0, STEPS, (ETA, 1)) == 0 and other.run(0, STEPS, (ETA, 2)) == 0
    a, b, c, d = sync_states(whole, split, again, other)
    for u, v, w, z in zip(a, b, c, d):
        assert torch.equal(u, v) and torch.equal(u, w)
        assert bool((u != z).flatten(1).any(dim=1).all())  # (seeds 1 and 2 differ in every sample)


def test_the_two_modalities_draw_different_noise(dev):
    """Two nets of equal shape and weights from equal start states: equal ends without noise, different ends with it."""
    m0, m1 = net("g16").to(dev), copy.deepcopy(net("g16")).to(dev)
    h0, h1 = m0._engine.handle(dev), m1._engine.handle(dev)
    assert h0.value != h1.value
    ends = {}
    for eta in (0.0, ETA):
        x, y = T.start("g16", B).to(dev).clone(), T.start("g16", B).to(dev).clone()
        raw = T.Raw("pair", (h0, h1, B, 0), (h0, h1, C._p(x), C._p(y), None, None, None, 0, B, STEPS, GAMMA), [x, y])
        assert C.RawSde("pair", raw).run(0, STEPS, (eta, SEED)) == 0
        torch.cuda.synchronize()
        ends[eta] = (x, y)
    assert torch.equal(*ends[0.0])
    x, y = ends[ETA]
    assert bool((x != y).flatten(1).any(dim=1).all())
    # x is the single loop's stream 0
    one = C.RawSde("single", T.raw_single("g16", T.start("g16", B).to(dev).clone(), STEPS, dev))
    assert one.run(0, STEPS, (ETA, SEED)) == 0
    torch.cuda.synchronize()
    assert torch.equal(one.state[0], x)


# ------------------------------------------------------------------ 5. closed form
def test_zero_velocity_is_the_linear_recursion_in_the_noise(dev):
    m = copy.deepcopy(net("g16"))
    with torch.no_grad():
        m.out_conv.weight.zero_()
        m.out_conv.bias.zero_()
    m = m.to(dev)
    x0 = T.start("g16", B)
    x = x0.to(dev).clone()
    h = m._engine.handle(dev)
    raw = C.RawSde("single", T.Raw("single", (h, B), (h, C._p(x), B, STEPS), [x]))
    assert raw.run(0, STEPS, (ETA, SEED)) == 0
    w, dt = f64(x0).reshape(-1), 1.0 / STEPS
    for k in range(STEPS):
        w = (1 - ETA * dt) * w + np.sqrt(2 * ETA * (1 - k * dt) * dt) * S.noise(SEED, 0, k, w.size)
    err = err64(x.reshape(-1), w)
    print(f"closed form, F = 0: err vs float64 {err:.3e}")
    assert err <= TOL_CLOSED, err


# ------------------------------------------------------------------ 6. errors
@pytest.mark.parametrize("kind", C.KINDS)
def test_errors_come_back_before_any_launch(dev, kind):
    r = C.make(kind, B, dev)
    before = sync_states(r)[0]
    assert r.run(0, STEPS, (-1.0, 1)) == EINVAL and b"eta" in r.L.rgfm_last_error()
    assert r.run(0, STEPS, (float("nan"), 1)) == EINVAL
    assert r.run(0, STEPS, (float("inf"), 1)) == EINVAL
    assert r.run(0, STEPS, (ETA, 1), solver=MIDPOINT) == EINVAL and b"midpoint" in r.L.rgfm_last_error().lower()
    assert r.run(0, STEPS, (ETA, 1), short=1) == ENOMEM
    after = sync_states(r)[0]
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert r.run(0, 0, (ETA, 1)) == 0                      # (an empty range is fine)
    assert r.run(0, STEPS, (0.0, 1), solver=MIDPOINT) == 0  # (eta = 0 with midpoint: the namesake)


# ------------------------------------------------------------------ 7. a caller's busy stream
def test_pair_loop_on_a_busy_stream_is_the_null_stream_call(dev):
    import stream_cases as SC
    case = SC.BY_ID["sde_sample_pair"]
    SC.null_stream_run(case, dev)
    want, wall_ms = SC.null_stream_run(case, dev)
    run = SC.late_stream_run(case, dev, SC.delay_for(wall_ms))
    assert run.delay_pending, "the delay had ended when the call returned: this run has shown nothing"
    assert len(run.clones) == len(want) == 2
    for a, b in zip(run.clones, want):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 8. the Python surface
def test_engine_calls_are_the_raw_calls(dev):
    raw = C.make("single", B, dev)
    assert raw.run(0, STEPS, (ETA, 7)) == 0
    got = _engine.sample_single(net("g24").to(dev), T.start("g24", B).to(dev).clone(), STEPS, sde_eta=ETA, sde_seed=7)
    assert torch.equal(got, raw.state[0])
    for kind in ("pair", "pair_cross"):
        raw = C.make(kind, B, dev)
        assert raw.run(0, STEPS, (ETA, 7)) == 0
        x, y, mx, my, r = C.pair_inputs(B, N, dev, kind == "pair_cross")
        _engine.sample_pair(net("g16").to(dev), net("g24").to(dev), x, y, mx, my, r, STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
        assert torch.equal(x, raw.state[0]) and torch.equal(y, raw.state[1]), kind
    raw = C.make("cond", B, dev)
    assert raw.run(0, STEPS, (ETA, 7)) == 0
    got = _engine.sample_cond(net("g24").to(dev), T.start("g24", B).to(dev).clone(), T.mc_set("g24", N).to(dev),
                              T.ratios(5, N)[:B].contiguous().to(dev), STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
    assert torch.equal(got, raw.state[0])
    raw = C.make("pair_grad", B, dev)
    assert raw.run(0, STEPS, (ETA, 7)) == 0
    x, y = _engine.sample_pair_grad(net("g16").to(dev), net("g24").to(dev), T.flex().to(dev), T.start("g16", B).to(dev).clone(),
                                    T.start("g24", B).to(dev).clone(), STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
    assert torch.equal(x, raw.state[0]) and torch.equal(y, raw.state[1])
    raw = C.make("cond_grad", B, dev)
    assert raw.run(0, STEPS, (ETA, 7)) == 0
    rr, tnet, cond, s0 = T.cond_grad_case("x")
    ctx = rr.to(dev)._engine.cond_prepare(cond.to(dev), "x", tuple(s0.shape[1:]))
    got = _engine.sample_cond_grad(tnet.to(dev), rr.to(dev), s0.to(dev).clone(), ctx, "x", STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
    assert torch.equal(got, raw.state[0])


@pytest.mark.parametrize("pairing", ["paired", "cross"])
def test_paired_sampler_is_the_direct_engine_calls(dev, pairing):
    from ratio_guided_multimodal_fm_amd.synth import paired_noise
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler
    fx, fy, rr = net("g16").to(dev), net("g24").to(dev), T.flex().to(dev)
    n, n_mc = 4, 6
    noise = paired_noise(31, n, n_mc, T.shape_of("g16"), T.shape_of("g24"))
    args = (fx, fy, rr, "mc_feng", GAMMA, n, STEPS, dev, n_mc, T.shape_of("g16"), T.shape_of("g24"))
    xs, ys = paired_sampler(*args, noise=noise, verbose=False, mc_pairing=pairing, sde_eta=ETA, sde_seed=7)
    x, y, mx, my = (t.to(dev, copy=True).contiguous() for t in noise)
    _engine.sample_two_streams(fx, mx, fy, my, STEPS)  # (the pre-phase stays deterministic)
    r = rr._engine.eval_cross(mx, my, "ratio") if pairing == "cross" else rr._engine.eval(mx, my, "ratio")
    _engine.sample_pair(fx, fy, x, y, mx, my, r, STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
    assert torch.equal(xs, x) and torch.equal(ys, y)
    zx, zy = paired_sampler(*args, noise=noise, verbose=False, mc_pairing=pairing, sde_eta=0.0, sde_seed=7)
    dx, dy = paired_sampler(*args, noise=noise, verbose=False, mc_pairing=pairing)
    assert torch.equal(zx, dx) and torch.equal(zy, dy) and not torch.equal(zx, xs)
    # sde_seed=None: one draw from torch's CPU generator, after the call's other draws
    torch.manual_seed(5)
    ax, ay = paired_sampler(*args, noise=noise, verbose=False, mc_pairing=pairing, sde_eta=ETA)
    torch.manual_seed(5)
    bx, by = paired_sampler(*args, noise=noise, verbose=False, mc_pairing=pairing, sde_eta=ETA)
    torch.manual_seed(5)
    cx, cy = paired_sampler(*args, noise=noise, verbose=False, mc_pairing=pairing, sde_eta=ETA, sde_seed=_engine.draw_sde_seed())
    assert torch.equal(ax, bx) and torch.equal(ay, by) and torch.equal(ax, cx) and torch.equal(ay, cy) and not torch.equal(ax, xs)
    if pairing == "paired":
        gx, gy = paired_sampler(fx, fy, rr, "grad_log_ratio", GAMMA, n, STEPS, dev, 0, T.shape_of("g16"), T.shape_of("g24"),
                                noise=noise, verbose=False, sde_eta=ETA, sde_seed=7)
        x, y = noise[0].to(dev, copy=True).contiguous(), noise[1].to(dev, copy=True).contiguous()
        _engine.sample_pair_grad(fx, fy, rr, x, y, STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
        assert torch.equal(gx, x) and torch.equal(gy, y)


@pytest.mark.parametrize("method", ["mc_feng", "grad_log_ratio"])
def test_sample_conditional_is_the_direct_engine_calls(dev, method):
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional
    target, rr = net("g24").to(dev), T.flex().to(dev)
    n, n_mc = 3, 6
    cond = T.start("g16", n, salt=9).to(dev)
    torch.manual_seed(77)
    out = sample_conditional(target, rr, cond, "x", STEPS, GAMMA, n_mc, guidance_method=method, sde_eta=ETA, sde_seed=7)
    torch.manual_seed(77)
    none = sample_conditional(target, rr, cond, "x", STEPS, GAMMA, n_mc, guidance_method=method, sde_eta=ETA)
    torch.manual_seed(77)
    if method == "mc_feng":  # the documented draw order: MC noise, then the start noise -- those of the eta = 0 call
        mc = torch.randn(n_mc, *T.shape_of("g24"), device=dev)
        _engine.sample_single(target, mc, STEPS)
        s = torch.randn(n, *T.shape_of("g24"), device=dev)
        R = rr.cross_log_ratio(cond, mc).exp()
        seed = _engine.draw_sde_seed()  # (then the seed, from the CPU generator)
        s2 = s.clone()
        _engine.sample_cond(target, s, mc, R, STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
        _engine.sample_cond(target, s2, mc, R, STEPS, GAMMA, sde_eta=ETA, sde_seed=seed)
    else:
        s = torch.randn(n, *T.shape_of("g24"), device=dev)
        ctx = rr._engine.cond_prepare(cond, "x", T.shape_of("g24"))
        seed = _engine.draw_sde_seed()
        s2 = s.clone()
        _engine.sample_cond_grad(target, rr, s, ctx, "x", STEPS, GAMMA, sde_eta=ETA, sde_seed=7)
        _engine.sample_cond_grad(target, rr, s2, ctx, "x", STEPS, GAMMA, sde_eta=ETA, sde_seed=seed)
    assert torch.equal(out, s) and torch.equal(none, s2) and not torch.equal(s, s2)
    torch.manual_seed(77)
    a = sample_conditional(target, rr, cond, "x", STEPS, GAMMA, n_mc, guidance_method=method)
    torch.manual_seed(77)
    b = sample_conditional(target, rr, cond, "x", STEPS, GAMMA, n_mc, guidance_method=method, sde_eta=0.0, sde_seed=7)
    assert torch.equal(a, b) and not torch.equal(a, out)


def test_schedule_sample_seeding_and_refusals(dev):
    from ratio_guided_multimodal_fm_amd.distributed import make_sharded_sampler
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import CFMSchedule, sample_bimodal_guided, sample_conditional
    m = make_module("unet28", dev)
    torch.manual_seed(5)
    got = CFMSchedule().sample(m, 3, STEPS, dev, sde_eta=ETA, sde_seed=7)
    torch.manual_seed(5)
    again = CFMSchedule().sample(m, 3, STEPS, dev, sde_eta=ETA)
    torch.manual_seed(5)
    twice = CFMSchedule().sample(m, 3, STEPS, dev, sde_eta=ETA)
    torch.manual_seed(5)
    x = torch.randn(3, 1, 28, 28, device=dev)  # (the start noise of the eta = 0 call)
    seed = _engine.draw_sde_seed()
    assert torch.equal(got, _engine.sample_single(m, x.clone(), STEPS, sde_eta=ETA, sde_seed=7))
    assert torch.equal(again, twice) and torch.equal(again, _engine.sample_single(m, x.clone(), STEPS, sde_eta=ETA, sde_seed=seed))
    assert not torch.equal(got, again)
    torch.manual_seed(5)
    a = CFMSchedule().sample(m, 3, STEPS, dev)
    torch.manual_seed(5)
    b = CFMSchedule().sample(m, 3, STEPS, dev, sde_eta=0.0, sde_seed=7)
    assert torch.equal(a, b) and torch.equal(a, _engine.sample_single(m, x.clone(), STEPS)) and not torch.equal(a, got)
    with pytest.raises(_lib.RgfmError, match="euler"):
        CFMSchedule().sample(m, 2, 2, dev, solver="midpoint", sde_eta=ETA)
    with pytest.raises(ValueError, match="sde_eta"):
        CFMSchedule().sample(m, 2, 2, dev, sde_eta=-1.0)
    fm = make_module("fm_original", dev)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        CFMSchedule().sample(fm, 2, 2, dev, sde_eta=ETA)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        sample_bimodal_guided(fm, make_module("fm_original_y", dev), None, "none", 0.0, 2, 2, dev, 4, sde_eta=ETA)
    with pytest.raises(_lib.RgfmError, match="euler"):
        sample_conditional(net("g24").to(dev), T.flex().to(dev), T.start("g16", 2).to(dev), "x", 2, GAMMA, 4, solver="midpoint",
                           sde_eta=ETA)
    with pytest.raises(_lib.RgfmError, match="sharded"):
        make_sharded_sampler((1, 28, 28), (1, 28, 28))(m, m, None, "none", 0.0, 2, 2, dev, 4, sde_eta=ETA)
    assert CFMSchedule().sample(fm, 2, 2, dev).shape == (2, 1, 28, 28)  # (the deterministic loop is still there)


def test_cli_sde_eta_equals_the_direct_call(dev, tmp_path, monkeypatch):
    import ratio_guided_multimodal_fm_amd as R
    from ratio_guided_multimodal_fm_amd import sample_mnist_svhn
    ck = tmp_path / "checkpoints"
    ck.mkdir()
    fm, fs, rr = make_module("mnist32"), make_module("svhn"), make_module("ratio_ms")
    torch.save({"epoch": 1, "model_state_dict": fm.state_dict(), "best_loss": 0.5}, ck / "flow_mnist32_best.pth")
    torch.save({"epoch": 1, "model_state_dict": fs.state_dict(), "best_loss": 0.5}, ck / "flow_svhn_best.pth")
    torch.save(rr.state_dict(), ck / "ratio_disc_mnist_svhn_best.pth")
    monkeypatch.chdir(tmp_path)
    base = ["--guidance_method", "mc_feng", "--guidance_strength", "0.5", "--num_steps", "3", "--num_samples", "3",
            "--mc_batch_size", "5", "--seed", "9"]
    assert sample_mnist_svhn.main(base + ["--sde_eta", "0.8", "--sde_seed", "11"]) == 0
    saved = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_mc_feng_gamma0.5.pt")
    R.utils.set_seed(9)
    xs, ys = sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(fm.to(dev), fs.to(dev), rr.to(dev), "mc_feng", 0.5, 3, 3, dev, 5,
                                                                sde_eta=0.8, sde_seed=11)
    assert torch.equal(saved["mnist"], xs.cpu()) and torch.equal(saved["svhn"], ys.cpu())
    R.utils.set_seed(9)
    ex, _ = sample_mnist_svhn.sample_bimodal_guided_mnist_svhn(fm.to(dev), fs.to(dev), rr.to(dev), "mc_feng", 0.5, 3, 3, dev, 5)
    assert not torch.equal(ex, xs)
    with pytest.raises(_lib.RgfmError, match="sharded"):
        sample_mnist_svhn.main(base + ["--sde_eta", "0.8", "--sharded"])
