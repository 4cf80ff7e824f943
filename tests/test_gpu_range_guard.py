"""The fp16 range guard on every conv route and every guarded loop, against float64 on the same
edited weights.  Cases: tests/range_cases.py (a scale pair puts ONE stretch of the residual stream outside the window;
tests/test_range_cases_cpu.py checks the magnitudes on the CPU).  The bound of a single evaluation is the existing
range tests' 1e-5 max|v64|; of a 4-step loop TOL_SAMPLER = 1e-4 (tests/test_gpu_ode.py, test_gpu_fmnet_eval.py); of an
in-loop gradient grad_loop_ref64.assert_grad_close.

Part A, cell by cell.  `route` is the launch whose check must raise the bit: the stager of the raw tensor (high side)
or its producer (low side).  With RGFM_RANGE_CHECK=0 the flag word must read exactly that bit, and the census of the
forward (rgfm_unet_conv_routes) must show the route and, for the other routes, the counts of range_cases.ROUTES.

  hit, and no launch of another route touches the stretch
    high: fused 1x1 skip on hx2p (a96, 20 px), on hx2d with SKIP (r16, 8x8), on hx2q (r32 at 256 rows, 32 px: a64's
          32-px skip launches have 64 channels and stay on hx2p at any batch, conv_hx2q_supported);
          Upsample in nine taps (a224, 5 -> 10); Upsample as parity classes (r16, 8 -> 16)
    low:  conv2 of a skip block on hx2p over full tiles (r32, 32 px) and over a ragged raster (r28, 28 px), on hx2d
          behind the P-format hand-over (r16, 8x8), on hx2q (r32 at 256 rows); Downsample on hx2 (a224) and on hx2s
          (r16); Upsample in nine taps (a224) and as parity classes (r16); input_conv with 1 and with 3 channels;
          a conv2 routed to bx3 at create (r28, weights x 2^-45)
  hit, not isolated
    high: Downsample on hx2 (a224, 10 -> 5) and on hx2s (r16, 16 -> 8).  A Downsample reads an encoder block's output,
          and every encoder tensor is also stored for the decoder, whose fused skip stages the same tensor on hx2p:
          both launches see it, both raise the same bit.
  cannot be reached by the default dispatch
    high: a fused 1x1 skip on hx2c -- conv_hx2c_supported leaves res_mode 2 to hx2p / hx2d (ConvTuning::hx2c_all is a
          kbench switch with no environment variable), so conv_mfma_hx2c.hip never stages a raw tensor.  Part B's
          "hx2c" runs the 8x8 level's raw stager, hx2d with SKIP, instead.
    low:  conv2 on hx2c and conv2 on hx2w -- both kernels take conv2 only with an identity skip (res_mode 1), whose
          output is h + conv2(...): it is small only where h is, and then h's producer has raised the bit already.

The Winograd cell (RGFM_WINO=1, a raw-free hx2w conv whose check is 4 max against the direct kernels' max) has a test
of its own below: a GroupNorm just under norm_params_ok's ceiling, the same weights with and without RGFM_WINO.

"The raw output is finite" (step 1) holds where it can: a raw value a is staged as S_A a = 16 a on fp16 planes, whose
largest number is 65504, so from |a| = 4094 on the unguarded planes hold inf and the unguarded result is inf / NaN by
construction -- the flag is all there is, which is what RGFM_RANGE_CHECK=0 gives up.  Part A's high side asks for
max >= 8192, beyond that; its unguarded results are printed, not asserted finite.  The low side and part B's
just-outside cases (3584: 16 a = 57344) are asserted finite.
"""
import copy

import numpy as np
import pytest
import torch

import grad_loop_ref64 as GL
import range_cases as R
from ratio_guided_multimodal_fm_amd import _engine, _lib

pytestmark = pytest.mark.gpu

TOL_EVAL = 1e-5
TOL_SAMPLER = 1e-4
FALLBACK_ENV = {R.HIGH: "bx3", R.LOW: "f32"}
S_A, FP16_MAX = 16.0, 65504.0  # conv_hx2_common.h: a raw value a is staged as S_A a on two fp16 planes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def on(m, dev):
    """A copy of a shared CPU module on the device (the engine is per copy: a fresh handle)."""
    return copy.deepcopy(m).to(dev).eval()


def rel(out, v64):
    return float(np.abs(out.detach().cpu().numpy().astype(np.float64) - v64).max() / np.abs(v64).max())


def flags_clear(dev, *modules):
    return all(m._engine.read_range_flag(dev, reset=False) == 0 for m in modules)


def guarded(fn, bit):
    """fn() under the guard: exactly one fallback with exactly `bit` (0: none).  Returns fn's result."""
    before = _engine.range_fallbacks
    out = fn()
    torch.cuda.synchronize()
    rose = _engine.range_fallbacks - before
    assert rose == (1 if bit else 0), (rose, _engine.last_range_flags)
    if bit:
        assert _engine.last_range_flags == bit, _engine.last_range_flags
    return out


# ================================================================== parts A and B: one forward
def check_routes(name, c, routes):
    want = c["routes"] if c["routes"] is not None else R.ROUTES[c["net"]]
    got = {k: routes[k] for k in want}
    print(f"{name}: routes " + " ".join(f"{k}={routes[k]}" for k in _lib.ROUTES + ("t2",)))
    assert got == want, (name, routes)
    if c["route"]:
        assert routes[c["route"]] > 0, (name, c["route"], routes)


def forward_case(name, c, dev, monkeypatch, expect_bit):
    """Steps 1 and 2 of the issue on one case; expect_bit 0: no flag, no fallback; None: either, printed."""
    cpu, x, t, targeted, readers, v64, acts64 = R.unet_case(name)
    staged_max = S_A * max(float(np.abs(acts64[k]).max()) for k in targeted)
    m = on(cpu, dev)
    xd, td = x.to(dev), t.to(dev)
    rows = R.ROWS_256 if c["rows"] == 256 else slice(None)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    # 1. unguarded: the flag word itself, the census, a finite result
    monkeypatch.setenv("RGFM_RANGE_CHECK", "0")
    raw = m(xd, td)
    torch.cuda.synchronize()
    routes = m._engine.conv_routes(dev)
    flag = m._engine.read_range_flag(dev)
    monkeypatch.delenv("RGFM_RANGE_CHECK")
    print(f"{name}: flag word {flag} with the guard off; error of the unguarded result {rel(raw[rows], v64):.3e}")
    if expect_bit is not None:
        assert flag == expect_bit, (name, flag)
    if staged_max < FP16_MAX:  # (see the docstring: beyond it the unguarded result is inf / NaN by construction)
        assert torch.isfinite(raw).all()
    check_routes(name, c, routes)
    # 2. guarded
    if expect_bit is None:
        before = _engine.range_fallbacks
        out = m(xd, td)
        print(f"{name}: fell back: {_engine.range_fallbacks - before} (flags {_engine.last_range_flags if _engine.range_fallbacks > before else 0})")
    else:
        out = guarded(lambda: m(xd, td), expect_bit)
    assert flags_clear(dev, m)
    err = rel(out[rows], v64)
    print(f"{name}: error / tolerance {err / TOL_EVAL:.3f}")
    assert err <= TOL_EVAL, (name, err)
    # an unedited net of the same shape right behind it: no fallback
    plain = on(R.make_unet(c["net"], 1)[0], dev)
    guarded(lambda: plain(xd[:3].contiguous(), td[:3].contiguous()), 0)
    assert flags_clear(dev, plain)


@pytest.mark.parametrize("name", list(R.A_CASES))
def test_part_a_every_route_raises_the_flag_itself(dev, name, monkeypatch):
    c = R.A_CASES[name]
    forward_case(name, c, dev, monkeypatch, c["bit"])


@pytest.mark.parametrize("name", list(R.B_CASES))
def test_part_b_edges_of_the_window(dev, name, monkeypatch):
    c = R.B_CASES[name]
    fb = c["falls_back"]
    forward_case(name, c, dev, monkeypatch, None if fb is None else (c["bit"] if fb else 0))


@pytest.mark.parametrize("name", list(R.ROW_CASES))
def test_part_b_one_row_out_of_range(dev, name):
    """One row of a batch out of range: the bound per row against float64; the large row must cause a fallback, for the
    tiny one the bound is the contract (a block maximum hiding a small sample would show here)."""
    cpu, x, t, row, v64, _ = R.row_case(name)
    m = on(cpu, dev)
    high = R.ROW_CASES[name][3] > 0
    before = _engine.range_fallbacks
    out = m(x.to(dev), t.to(dev)).cpu().numpy().astype(np.float64)
    rose = _engine.range_fallbacks - before
    per_row = np.abs(out - v64).reshape(len(v64), -1).max(1) / np.abs(v64).reshape(len(v64), -1).max(1)
    print(f"{name}: fallbacks {rose} (flags {_engine.last_range_flags if rose else 0}); worst row error / tolerance "
          f"{per_row.max() / TOL_EVAL:.3f}, row {row}: {per_row[row] / TOL_EVAL:.3f}")
    if high:
        assert rose == 1 and _engine.last_range_flags == R.HIGH
    assert flags_clear(dev, m)
    assert per_row.max() <= TOL_EVAL, (name, int(per_row.argmax()), float(per_row.max()))


def test_part_a_winograd_conv_tests_four_times_the_maximum(dev, monkeypatch):
    """norm1 of a64's decoder_blocks.2 just under norm_params_ok's ceiling (range_cases.wino_case): staged values of
    ~9000, under the direct kernels' limit and over a quarter of it.  Default dispatch: no flag.  RGFM_WINO=1: that conv
    runs on hx2w, whose input transform adds up to four staged values -- it must raise bit 1, and the repeat on bx3
    must meet the bound."""
    cpu, x, t, v64, _, _ = R.wino_case()
    xd, td = x.to(dev), t.to(dev)
    m = on(cpu, dev)
    out = guarded(lambda: m(xd, td), 0)
    plain_routes = m._engine.conv_routes(dev)
    assert plain_routes["hx2w"] == 0 and plain_routes["bx3"] == 0 and flags_clear(dev, m)
    print(f"wino cell, default dispatch: error / tolerance {rel(out, v64) / TOL_EVAL:.3f}")
    assert rel(out, v64) <= TOL_EVAL
    monkeypatch.setenv("RGFM_WINO", "1")
    w = on(cpu, dev)
    monkeypatch.setenv("RGFM_RANGE_CHECK", "0")
    raw = w(xd, td)
    torch.cuda.synchronize()
    routes, flag = w._engine.conv_routes(dev), w._engine.read_range_flag(dev)
    monkeypatch.delenv("RGFM_RANGE_CHECK")
    print("wino cell: routes " + " ".join(f"{k}={routes[k]}" for k in _lib.ROUTES + ("t2",)) + f"; flag word {flag}")
    assert routes["hx2w"] > 0 and routes["bx3"] == 0 and flag == R.HIGH and torch.isfinite(raw).all()
    out = guarded(lambda: w(xd, td), R.HIGH)
    assert flags_clear(dev, w)
    print(f"wino cell, RGFM_WINO=1: error / tolerance {rel(out, v64) / TOL_EVAL:.3f}")
    assert rel(out, v64) <= TOL_EVAL
    # the unedited net under RGFM_WINO=1 raises nothing
    plain = on(R.make_unet(R.WINO_NET, 1)[0], dev)
    guarded(lambda: plain(xd, td), 0)
    assert plain._engine.conv_routes(dev)["hx2w"] == routes["hx2w"]


# ================================================================== part C: the GroupNorm gate of a U-Net conv
def norm_run(m, x, t, dev):
    out = guarded(lambda: m(x, t), 0)  # (the gate acts at create: never a fallback)
    assert flags_clear(dev, m)
    return out, m._engine.conv_routes(dev)


@pytest.mark.parametrize("name", list(R.NORM_CASES))
def test_part_c_norm_gate_at_create(dev, name):
    inside = R.NORM_CASES[name][3]
    cpu, x, t, v64, _ = R.norm_case(name)
    xd, td = x.to(dev), t.to(dev)
    _, base = norm_run(on(R.make_unet(R.NORM_NET, 1)[0], dev), xd, td, dev)
    assert {k: base[k] for k in R.ROUTES[R.NORM_NET]} == R.ROUTES[R.NORM_NET], base
    out, routes = norm_run(on(cpu, dev), xd, td, dev)
    err = rel(out, v64)
    print(f"norm gate {name}: bx3 launches {base['bx3']} -> {routes['bx3']}; error / tolerance {err / TOL_EVAL:.3f}")
    assert err <= TOL_EVAL, (name, err)
    assert routes["bx3"] == base["bx3"] + (0 if inside else 1), (name, routes)  # (that block's conv2, nothing else)
    assert sum(routes[k] for k in _lib.ROUTES) == sum(base[k] for k in _lib.ROUTES)


@pytest.mark.parametrize("name", ["hi-outside", "lo-outside"])
def test_part_c_norm_gate_through_update_params(dev, name):
    """The edit applied in place to a live handle (rgfm_unet_update_params): the conv is demoted; with the parameters
    put back it is promoted again and the forward has its first bits."""
    cpu, x, t, v64, _ = R.norm_case(name)
    xd, td = x.to(dev), t.to(dev)
    m = on(R.make_unet(R.NORM_NET, 1)[0], dev)
    saved = {k: v.clone() for k, v in m.state_dict().items()}
    first, base = norm_run(m, xd, td, dev)
    handle = m._engine.handle(dev)
    R.apply_norm_edit(m, name)
    out, routes = norm_run(m, xd, td, dev)
    assert m._engine.owns(handle) and m._engine.handle(dev) is handle  # (re-packed in place, not re-created)
    assert routes["bx3"] == base["bx3"] + 1, routes
    assert rel(out, v64) <= TOL_EVAL
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(saved[k])
    again, routes = norm_run(m, xd, td, dev)
    assert m._engine.handle(dev) is handle
    assert routes == base and torch.equal(again, first)


# ================================================================== part F: FlowMatchingModel, both sides
@pytest.mark.parametrize("bit", [R.HIGH, R.LOW])
def test_part_f_fmnet_forward(dev, bit, monkeypatch):
    i = R.fm_inputs()
    m = on(R.fm_net(bit), dev)
    x, t = i["x"].to(dev), i["t"].to(dev)
    monkeypatch.setenv("RGFM_RANGE_CHECK", "0")
    raw = m(x, t)
    flag = m._engine.read_range_flag(dev)
    monkeypatch.delenv("RGFM_RANGE_CHECK")
    assert flag == bit, flag
    assert bit == R.HIGH or torch.isfinite(raw).all()  # (high side: S_A 2.5e4 is beyond fp16, see the docstring)
    out = guarded(lambda: m(x, t), bit)
    assert flags_clear(dev, m)
    err = rel(out, R.fm_want("forward", bit)[0])
    print(f"FlowMatchingModel forward bit {bit}: error / tolerance {err / TOL_EVAL:.3f}")
    assert err <= TOL_EVAL, err
    plain = on(R.fm_net("x"), dev)
    guarded(lambda: plain(x, t), 0)


# ================================================================== part D: every guarded entry point
class Loop:
    """One part D entry on device copies of the shared nets: run(solver) starts from fresh copies of the start state
    and returns (states, records or None)."""

    def __init__(self, entry, bit, dev):
        self.entry, self.dev = entry, dev
        self.i = {k: v.to(dev) for k, v in R.d_inputs().items()}
        self.X, self.Y = on(R.d_net(bit), dev), on(R.d_net("y"), dev)
        self.rr = None
        if entry == "pair-grad":
            self.rr = on(R.d_flex(), dev)
        elif entry == "cond-grad":
            import cond_grad_ref64 as CG
            self.rr = on(CG.sampler_case("x")[0], dev)
        self.nets = {"single": [self.X], "two": [self.Y, self.X], "two-same": [self.X], "cond": [self.X],
                     "cond-grad": [self.X]}.get(entry, [self.X, self.Y])

    def run(self, solver):
        i, X, Y, E, S, G = self.i, self.X, self.Y, _engine, R.D_STEPS, R.D_GAMMA
        x, y, rec = i["x0"].clone(), i["y0"].clone(), None
        e = self.entry
        if e == "single":
            return [E.sample_single(X, x, S, solver=solver)], None
        if e == "two":
            return list(E.sample_two_streams(Y, y, X, x, S, solver=solver)), None
        if e == "two-same":
            return list(E.sample_two_streams(X, x, X, i["x1"].clone(), S, solver=solver)), None
        if e == "pair":
            return list(E.sample_pair(X, Y, x, y, None, None, None, S, 0.0, solver=solver)), None
        if e in ("pair-mc", "pair-graph"):
            return list(E.sample_pair(X, Y, x, y, i["mx7"], i["my7"], i["r7"], S, G, solver=solver)), None
        if e == "pair-cross":
            return list(E.sample_pair(X, Y, x, y, i["mx5"], i["my5"], i["R5"], S, G, solver=solver)), None
        if e == "pair-gs":
            return list(E.sample_pair(X, Y, x, y, i["mx7"], i["my7"], i["r7"], S, 0.0, solver=solver, gamma_rows=i["rows"],
                                      stage_scale=list(R.D_STAGE_SCALE[solver]))), None
        if e == "pair-diag":
            rec = torch.full((S * (2 if solver == "midpoint" else 1), R.D_B, _lib.DIAG_FLOATS), -7.0, device=self.dev)
            return list(E.sample_pair(X, Y, x, y, i["mx7"], i["my7"], i["r7"], S, G, solver=solver, diag=rec)), rec
        if e == "pair-grad":
            return list(E.sample_pair_grad(X, Y, self.rr, x, y, S, G, solver=solver)), None
        if e == "cond":
            return [E.sample_cond(X, x, i["mx7"], i["Rc"], S, G, solver=solver)], None
        if e == "cond-grad":
            s = i["s0"].clone()
            ctx = self.rr._engine.cond_prepare(i["cond"], "x", tuple(s.shape[1:]))
            return [E.sample_cond_grad(X, self.rr, s, ctx, "x", S, G, solver=solver)], None
        raise KeyError(e)


def check_restored_handles(loop, bit, solver, first):
    """Both engines are back on CONV_DEFAULT: the unedited net's next ordinary call has the bits of a fresh handle's,
    and the edited net's next call trips the guard again (a handle left on the fallback would not) with the same bits."""
    dev, i = loop.dev, loop.i
    if loop.Y in loop.nets:
        used = guarded(lambda: _engine.sample_single(loop.Y, i["y0"].clone(), R.D_STEPS, solver=solver), 0)
        fresh = _engine.sample_single(on(R.d_net("y"), dev), i["y0"].clone(), R.D_STEPS, solver=solver)
        assert torch.equal(used, fresh)
    again, rec = guarded(lambda: loop.run(solver), bit)
    assert all(torch.equal(a, b) for a, b in zip(again, first))
    assert flags_clear(dev, *loop.nets)


D_GRID = [(e, bit, s) for e, solvers in R.D_ENTRIES.items() for bit in (R.HIGH, R.LOW) for s in solvers
          if not (e == "pair-graph" and bit == R.LOW)]


@pytest.mark.parametrize("entry,bit,solver", D_GRID)
def test_part_d_entry_repeats_correctly(dev, entry, bit, solver, monkeypatch):
    if entry == "pair-graph":
        monkeypatch.setenv("RGFM_GRAPH", "1")
    loop = Loop(entry, bit, dev)
    states, rec = guarded(lambda: loop.run(solver), bit)
    assert flags_clear(dev, *loop.nets)
    want = R.d_want(entry, bit, solver)
    errs = [float(np.abs(s.cpu().numpy().astype(np.float64) - w).max()) for s, w in zip(states, want)]
    print(f"part D {entry} bit {bit} {solver}: error / tolerance " + " ".join(f"{e / TOL_SAMPLER:.3f}" for e in errs))
    assert len(states) == len(want) and max(errs) <= TOL_SAMPLER, errs
    # the same call with the fallback arithmetic chosen up front, on fresh handles: the same bits (this pins the restore)
    monkeypatch.setenv("RGFM_CONV", FALLBACK_ENV[bit])
    front = Loop(entry, bit, dev)
    fstates, frec = guarded(lambda: front.run(solver), 0)
    monkeypatch.delenv("RGFM_CONV")
    for a, b in zip(states, fstates):
        assert torch.equal(a, b), (entry, float((a - b).abs().max()))
    if rec is not None:
        assert torch.equal(rec, frec) and not bool((rec == -7.0).any())
    check_restored_handles(loop, bit, solver, states)


@pytest.mark.parametrize("what", ["single", "pair"])
def test_part_d_fmnet_loops(dev, what, monkeypatch):
    """FlowMatchingModel sample_single / sample_pair with one net's fc1 x 2^-16 (bit 2; the Euler loops)."""
    i = {k: v.to(dev) for k, v in R.fm_inputs().items()}

    def run(fx, fy):
        x, y = i["x"].clone(), i["y"].clone()
        if what == "single":
            return [_engine.sample_single(fx, x, R.D_STEPS)]
        return list(_engine.sample_pair(fx, fy, x, y, i["mx"], i["my"], i["r"], R.D_STEPS, R.D_GAMMA))
    fx, fy = on(R.fm_net(R.LOW), dev), on(R.fm_net("y"), dev)
    states = guarded(lambda: run(fx, fy), R.LOW)
    assert flags_clear(dev, fx, fy)
    errs = [float(np.abs(s.cpu().numpy().astype(np.float64) - w).max()) for s, w in zip(states, R.fm_want(what, R.LOW))]
    print(f"part D FlowMatchingModel {what}: error / tolerance " + " ".join(f"{e / TOL_SAMPLER:.3f}" for e in errs))
    assert max(errs) <= TOL_SAMPLER, errs
    monkeypatch.setenv("RGFM_CONV", "f32")
    front = guarded(lambda: run(on(R.fm_net(R.LOW), dev), on(R.fm_net("y"), dev)), 0)
    monkeypatch.delenv("RGFM_CONV")
    assert all(torch.equal(a, b) for a, b in zip(states, front))
    if what == "pair":  # the partner's handle is back on the default arithmetic
        used = guarded(lambda: _engine.sample_single(fy, i["y"].clone(), R.D_STEPS), 0)
        assert torch.equal(used, _engine.sample_single(on(R.fm_net("y"), dev), i["y"].clone(), R.D_STEPS))
    again = guarded(lambda: run(fx, fy), R.LOW)
    assert all(torch.equal(a, b) for a, b in zip(states, again))


@pytest.mark.parametrize("bit", [R.HIGH, R.LOW])
def test_part_d_an_exception_inside_the_repeat_leaves_the_default_arithmetic(dev, bit, monkeypatch):
    """_run_loop raises on its second call -- the repeat: the `finally` of _range_guarded must still put both handles
    back on CONV_DEFAULT."""
    loop = Loop("pair-mc", bit, dev)
    real, calls = _engine._run_loop, []

    def flaky(*a, **k):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("second call")
        return real(*a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(_engine, "_run_loop", flaky)
        before = _engine.range_fallbacks
        with pytest.raises(RuntimeError, match="second call"):
            loop.run("euler")
        assert len(calls) == 2 and _engine.range_fallbacks == before + 1 and _engine.last_range_flags == bit
    torch.cuda.synchronize()
    assert flags_clear(dev, loop.X, loop.Y)
    states, _ = guarded(lambda: loop.run("euler"), bit)
    want = R.d_want("pair-mc", bit, "euler")
    assert max(float(np.abs(s.cpu().numpy().astype(np.float64) - w).max()) for s, w in zip(states, want)) <= TOL_SAMPLER
    check_restored_handles(loop, bit, "euler", states)


# ================================================================== part E: the estimator raises the velocity net's flag
def e_loop(c, gamma, dev, nets, rr):
    s = [t.to(dev).clone() for t in c["s0"]]
    if len(s) == 2:
        _engine.sample_pair_grad(nets[0], nets[1], rr, s[0], s[1], GL.S, gamma, GL.K, GL.K + 1)
    else:
        ctx = rr._engine.cond_prepare(c["cond"].to(dev), c["given"], tuple(s[0].shape[1:]))
        _engine.sample_cond_grad(nets[0], rr, s[0], ctx, c["given"], GL.S, gamma, GL.K, GL.K + 1)
    torch.cuda.synchronize()
    return s


@pytest.mark.parametrize("kind,loop,bit", R.E_CASES)
def test_part_e_estimator_inside_the_gradient_loops(dev, kind, loop, bit, monkeypatch):
    """The in-loop gradient (read out of one Euler step, grad_loop_ref64) on an estimator whose one layer is staged out
    of the window.  BatchNorm kind: the estimator's forward convs run on the U-Net handle's two fp16 planes and must
    raise ITS flag -- bit 1 for the large layer; for the small layer the contract is the gradient bound.  GroupNorm
    kinds: exact fp32 convs in the loop, so no flag and the bound.

    The small-layer cases are the ones that failed first: no flag, and the target side's gradient off by 1.37e-2 of its
    maximum (bound 1e-4) in both loops.  pack_ratio's create-time gate on the BatchNorm parameters (demote_by_batchnorms)
    takes conv2b off the fp16 path; measured after it: 2.0e-6."""
    c = R.e_case(kind, loop, bit)
    rr, nets = on(c["rr"], dev), [on(n, dev) for n in c["nets"]]
    # the flag word itself, with the guard off: read through the x net's handle (the target's in the cond loop)
    monkeypatch.setenv("RGFM_RANGE_CHECK", "0")
    e_loop(c, c["gamma"][0], dev, nets, rr)
    words = [n._engine.read_range_flag(dev) for n in nets]
    monkeypatch.delenv("RGFM_RANGE_CHECK")
    before = _engine.range_fallbacks
    zero = e_loop(c, 0.0, dev, nets, rr)
    runs = {g: e_loop(c, g, dev, nets, rr) for g in sorted(set(c["gamma"]))}
    rose = _engine.range_fallbacks - before
    print(f"part E {kind} {loop} bit {bit}: flag words with the guard off {words}; fallbacks in {1 + len(runs)} guarded calls: {rose}")
    ghat = tuple(GL.extract(runs[g][k], zero[k], g) for k, g in enumerate(c["gamma"]))
    if kind == "ms" and bit == R.HIGH:
        assert words[0] == R.HIGH and all(w == 0 for w in words[1:]), words
        # (every guided call falls back; the gamma = 0 call too if the loop runs the estimator at gamma 0)
        assert rose in (len(runs), 1 + len(runs)) and _engine.last_range_flags == R.HIGH
    elif kind != "ms":
        assert words == [0] * len(nets) and rose == 0, (words, rose)
    assert flags_clear(dev, *nets)
    GL.assert_grad_close(ghat, c["g64"], c["rho"], f"part E {kind} {loop} bit {bit}")
