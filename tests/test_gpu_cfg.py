"""Class-conditional U-Nets and classifier-free guidance on the GPU, against float64 (tests/cfg_ref64.py: composed from
the pinned unet_ref64.forward64 / ode_ref64.integrate64 / sde_ref64.integrate_sde64).

Bounds (the project's own; the CFG factor is derived: the blend v_u + w (v_c - v_u) = w v_c + (1 - w) v_u combines two
evaluations' errors with the weights |w| and |1 - w|):
    one evaluation         |v - v64| <= TOL_EVAL * max(1, max |v64|),   TOL_EVAL = 1e-5     (test_gpu_arch_sweep.py)
    gradients              |g - g64| <= TOL_GRAD * max |g64| per tensor, TOL_GRAD = 1e-4    (test_gpu_train.py)
    a 4-step loop          |x - x64| <= TOL_SAMPLER * (|w| + |1 - w|),  TOL_SAMPLER = 1e-4  (1e-4 at w = 1, 5e-4 at w = 3)
Measured worst cases on one MI355X (every test prints its own: pytest -s; profiles/cfg/test_gpu_cfg.txt):
    forward                6.1e-6 (k10w under RGFM_CONV=f32; 3.0e-6 default; mnist32 batch 66: 2.7e-6 .. 3.9e-6)   bound 1e-5 x max|v64| (1.6 .. 4.1)
    training pass          v 2.7e-6; worst gradient error / max |g64| 2.5e-6 (k3);  after one Adam step v 5.1e-6
    4-step loops, w = 1    1.1e-6 (mnist32 Euler);  w = 3: 4.1e-6 (mnist32, sde_eta = 1)                          bounds 1e-4 / 5e-4
    unguided pair          5.6e-6 (k10w, w = 3, midpoint);  two labelled nets without labels under mc_feng: 3.2e-7
    margins                |w=3 - w=1| 0.22 (k3) / 0.45 (mnist32), |labelled - unlabelled| 0.11 / 0.23            needed: > 0.05
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cfg_cases as C
import cfg_ref64 as R
import ode_ref64 as O
import sde_ref64 as S
import stream_cases as SC
import unet_ref64 as U
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth
from ratio_guided_multimodal_fm_amd.utils import flow_utils as FU

pytestmark = pytest.mark.gpu

TOL_EVAL, TOL_GRAD, TOL_SAMPLER = 1e-5, 1e-4, 1e-4
STEPS = C.STEPS
EINVAL, ENOMEM = -1, -2
MODES = {"default": {}, "bx3": {"RGFM_CONV": "bx3"}, "f32": {"RGFM_CONV": "f32"}}
LOOP_ROWS = 5  # rows of the sampler-loop cases


def bound(w):
    return TOL_SAMPLER * (abs(w) + abs(1.0 - w))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def err64(got, want):
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - np.asarray(want)).max())


def f64(t):
    return t.numpy().astype(np.float64)


# ------------------------------------------------------------------ shared float64 references (computed once, read-only)
@functools.lru_cache(maxsize=None)
def forward64(tag):
    m = C.net(tag)
    y = C.labels_of(tag)
    x, t = C.inputs(tag, len(y))
    with torch.no_grad():
        return R.forward_labels64(U.cfg_of(m), R.params64(m, requires_grad=False), x, t, y).numpy()


def loop_labels(tag):
    return C.labels_of(tag, LOOP_ROWS)


@functools.lru_cache(maxsize=None)
def loop64(tag, w, solver="euler", eta=0.0, labelled=True, rng=(0, STEPS), steps=STEPS):
    m = C.net(tag)
    x0 = f64(C.inputs(tag, LOOP_ROWS)[0])
    Fv = R.F_cfg(m, loop_labels(tag) if labelled else None, w)
    if eta:
        out = S.integrate_sde64(Fv, (x0,), steps, eta, 2024, *rng)[0]
    else:
        out = O.integrate64(Fv, (x0,), steps, solver, *rng)[0]
    out.setflags(write=False)
    return out


def start(tag, dev, rows=LOOP_ROWS):
    return C.inputs(tag, LOOP_ROWS)[0][:rows].to(dev).clone()


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("tag", list(C.NETS))
def test_forward_vs_float64(dev, monkeypatch, tag, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    m = C.net(tag).to(dev)
    y = C.labels_of(tag)
    x, t = (v.to(dev) for v in C.inputs(tag, len(y)))
    fallbacks = _engine.range_fallbacks
    v = m(x, t, y.to(dev))
    torch.cuda.synchronize()
    assert _engine.range_fallbacks == fallbacks, (tag, mode, _engine.last_range_flags)
    want = forward64(tag)
    e = err64(v, want)
    print(f"forward {tag} [{mode}] B={len(y)}: |v - v64| {e:.3e} (max |v64| {np.abs(want).max():.3f})")
    assert e <= TOL_EVAL * max(1.0, float(np.abs(want).max())), (tag, mode, e)
    # y = None is the null label in every row, bitwise; and it is not the labelled output
    K = C.classes(tag)
    none = m(x, t)
    assert torch.equal(none, m(x, t, torch.full((len(y),), K, device=dev)))
    with torch.no_grad():
        null64 = R.forward_labels64(U.cfg_of(C.net(tag)), R.params64(C.net(tag), requires_grad=False), x[:3].cpu(), t[:3].cpu(), None)
    assert err64(none[:3], null64.numpy()) <= TOL_EVAL * max(1.0, float(null64.abs().max()))
    assert float((none - v).abs().max()) > 100 * TOL_EVAL


# ------------------------------------------------------------------ 2. rows do not depend on the batch
@pytest.mark.parametrize("tag", ["k3", "mnist32"])
def test_rows_do_not_depend_on_the_batch(dev, tag):
    m = C.net(tag).to(dev)
    y = C.labels_of(tag).to(dev)
    x, t = (v.to(dev) for v in C.inputs(tag, len(y)))
    full = m(x, t, y)
    for i in sorted({0, 1, len(y) // 2, len(y) - 1}):
        assert torch.equal(full[i:i + 1], m(x[i:i + 1].contiguous(), t[i:i + 1].contiguous(), y[i:i + 1].contiguous())), (tag, i)
    # a 4-step cfg_scale = 3 loop
    yl = loop_labels(tag).to(dev)
    s = start(tag, dev)
    _engine.sample_single(m, s, STEPS, labels=yl, cfg_scale=3.0)
    for i in (0, LOOP_ROWS - 1):
        one = start(tag, dev)[i:i + 1].contiguous()
        _engine.sample_single(m, one, STEPS, labels=yl[i:i + 1].contiguous(), cfg_scale=3.0)
        assert torch.equal(one, s[i:i + 1]), (tag, i)


# ------------------------------------------------------------------ 3. training pass
TRAIN_LABELS = {"k3": [0, 2, 3, 2, 0, 0], "mnist32": [0, 1, 2, 10, 4, 5]}  # batch 6: class 1 / 3 absent, one null label


def _hip_train(m, x, t, y, target):
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    v = m.forward_train(xg, t, y)
    loss = F.mse_loss(v, target)
    loss.backward()
    return v.detach(), loss.item(), xg.grad, [p.grad.clone() for p in m.parameters()]


@pytest.mark.parametrize("tag", ["k3", "mnist32"])
def test_training_pass_vs_float64(dev, tag):
    m = load_synth(C.NETS[tag][0](), C.NETS[tag][2]).to(dev).eval()  # (its own module: the step below moves the weights)
    K = C.classes(tag)
    y = torch.tensor(TRAIN_LABELS[tag])
    absent = sorted(set(range(K + 1)) - set(y.tolist()))
    assert absent and K in y.tolist()
    g = torch.Generator().manual_seed(900 + K)
    x, t = torch.randn(6, *C.shape_of(tag), generator=g), torch.rand(6, generator=g)
    target = torch.randn(6, *C.shape_of(tag), generator=g)
    v, loss, dx, grads = _hip_train(m, x.to(dev), t.to(dev), y.to(dev), target.to(dev))
    sd = R.params64(m)
    x64 = x.double().requires_grad_(True)
    v64 = R.forward_labels64(U.cfg_of(m), sd, x64, t, y)
    loss64 = F.mse_loss(v64, target.double())
    loss64.backward()
    ev = err64(v, v64.detach().numpy())
    assert ev <= TOL_EVAL * max(1.0, float(v64.detach().abs().max())), ev
    assert abs(loss - loss64.item()) <= 1e-5 * abs(loss64.item())
    worst = 0.0
    for name, got, want in [("dx", dx, x64.grad)] + [(k, a, sd[k].grad) for k, a in zip(m.state_dict(), grads)]:
        scale = float(want.abs().max())
        e = float((got.detach().cpu().double() - want).abs().max())
        worst = max(worst, e / max(scale, 1e-30))
        assert e <= TOL_GRAD * max(scale, 1e-30), (name, e, scale)
    dE = grads[-1]
    assert list(m.state_dict())[-1] == R.EMB and tuple(dE.shape) == (K + 1, 4 * m.model_channels)
    for c in absent:
        assert bool((dE[c] == 0).all()), c
    assert all(float(dE[c].abs().max()) > 0 for c in set(y.tolist()))
    print(f"train {tag}: |v - v64| {ev:.3e}, worst gradient error / max |g64| {worst:.3e}")
    # two backward calls: identical bits
    again = _hip_train(m, x.to(dev), t.to(dev), y.to(dev), target.to(dev))
    assert torch.equal(again[0], v) and torch.equal(again[2], dx) and all(torch.equal(a, b) for a, b in zip(again[3], grads))
    # without labels: the null row takes every row's gradient
    none = _hip_train(m, x.to(dev), t.to(dev), None, target.to(dev))
    assert bool((none[3][-1][:K] == 0).all()) and float(none[3][-1][K].abs().max()) > 0
    # one Adam step, then the eval forward: the handle's repack picks up label_emb (float64: the same step)
    lr = 1e-4
    before = m(x.to(dev), t.to(dev), y.to(dev)).clone()
    _hip_train(m, x.to(dev), t.to(dev), y.to(dev), target.to(dev))
    e_before = m.label_emb.weight.detach().clone()
    torch.optim.Adam(m.parameters(), lr=lr).step()
    leaves = [sd[k] for k in m.state_dict()]
    torch.optim.Adam(leaves, lr=lr).step()
    after = m(x.to(dev), t.to(dev), y.to(dev))
    with torch.no_grad():
        after64 = R.forward_labels64(U.cfg_of(m), {k: q.detach() for k, q in sd.items()}, x, t, y)
    ea, moved = err64(after, after64.numpy()), float((after - before).abs().max())
    print(f"train {tag}: after one Adam step |v - v64| {ea:.3e}; the step moved v by {moved:.3e}")
    assert not torch.equal(m.label_emb.weight.detach(), e_before) and moved > 100 * TOL_EVAL
    # (the step's own rounding: an fp32 Adam update lr g / (|g| + eps) differs from the float64 one by up to lr * (relative
    # error of g), far below the bound of one evaluation at lr = 1e-4)
    assert ea <= TOL_EVAL * max(1.0, float(after64.abs().max())), ea


# ------------------------------------------------------------------ 4. sampler loops
def _schedule_sample(m, dev, labels, w, seed=77, **kw):
    """CFMSchedule.sample from a seeded device generator, and the start noise it drew."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    out = FU.CFMSchedule().sample(m, len(labels), num_steps=STEPS, device=dev, labels=labels, cfg_scale=w, **kw)
    torch.cuda.manual_seed(seed)
    x0 = torch.randn(len(labels), m.in_channels, m.img_size, m.img_size, device=dev)
    return out, x0


@pytest.mark.parametrize("w", [1.0, 3.0])
@pytest.mark.parametrize("solver,eta", [("euler", 0.0), ("midpoint", 0.0), ("euler", 1.0)])
@pytest.mark.parametrize("tag", ["k3", "mnist32"])
def test_loops_vs_float64(dev, tag, solver, eta, w):
    m = C.net(tag).to(dev)
    y = loop_labels(tag).to(dev)
    x = start(tag, dev)
    _engine.sample_single(m, x, STEPS, solver=solver, labels=y, cfg_scale=w, sde_eta=eta, sde_seed=2024)
    e = err64(x, loop64(tag, w, solver, eta))
    print(f"loop {tag} {solver} eta={eta} w={w}: |x - x64| {e:.3e} (bound {bound(w):.1e})")
    assert e <= bound(w), (tag, solver, eta, w, e)
    # CFMSchedule.sample is that loop on its own start noise
    out, x0 = _schedule_sample(m, dev, y, w, solver=solver, sde_eta=eta, sde_seed=2024)
    direct = x0.clone()
    _engine.sample_single(m, direct, STEPS, solver=solver, labels=y, cfg_scale=w, sde_eta=eta, sde_seed=2024)
    assert torch.equal(out, direct) and tuple(out.shape) == (LOOP_ROWS, *C.shape_of(tag))


@pytest.mark.parametrize("tag", ["k3", "mnist32"])
def test_scale_zero_split_calls_and_margins(dev, tag):
    m = C.net(tag).to(dev)
    y = loop_labels(tag).to(dev)
    runs = {}
    for w in (0.0, 1.0, 3.0):
        runs[w] = start(tag, dev)
        _engine.sample_single(m, runs[w], STEPS, labels=y, cfg_scale=w)
    plain = start(tag, dev)
    _engine.sample_single(m, plain, STEPS)
    assert torch.equal(runs[0.0], plain)  # cfg_scale = 0 with labels: the call without labels, bitwise
    assert err64(plain, loop64(tag, 1.0, labelled=False)) <= TOL_SAMPLER  # ... which is the null row, against float64
    for solver in ("euler", "midpoint"):
        one, two = start(tag, dev), start(tag, dev)
        _engine.sample_single(m, one, STEPS, solver=solver, labels=y, cfg_scale=3.0)
        _engine.sample_single(m, two, STEPS, 0, 2, solver=solver, labels=y, cfg_scale=3.0)
        _engine.sample_single(m, two, STEPS, 2, 4, solver=solver, labels=y, cfg_scale=3.0)
        assert torch.equal(one, two), solver
    d31, d1u = float((runs[3.0] - runs[1.0]).abs().max()), float((runs[1.0] - plain).abs().max())
    print(f"margins {tag}: |w=3 - w=1| {d31:.3e}, |labelled - unlabelled| {d1u:.3e} (100 x bound: {100 * bound(3.0):.1e})")
    assert d31 > 100 * bound(3.0)  # a loop that ignores the scale fails here
    assert d1u > 100 * bound(3.0)  # ... and one that ignores the labels here


def test_unguided_pair_vs_two_float64_loops(dev):
    mx, my = C.net("k3").to(dev), C.net("k10w").to(dev)
    B = 3
    x0, y0 = C.inputs("k3", B)[0], C.inputs("k10w", B)[0]
    same = torch.tensor([0, 3, 2])
    lx, ly = torch.tensor([1, 0, 3]), torch.tensor([9, 10, 4])
    for labels, scale, want in ((same, 3.0, (same, same, 3.0, 3.0)), ((lx, ly), (3.0, 1.0), (lx, ly, 3.0, 1.0)),
                                ((lx, None), (0.5, 1.0), (lx, None, 0.5, 1.0))):
        a, b, wa, wb = want
        xs, ys = FU.paired_sampler(mx, my, None, "none", 0.0, B, STEPS, dev, 4, C.shape_of("k3"), C.shape_of("k10w"),
                                   noise=(x0, y0, None, None), verbose=False, solver="midpoint", labels=labels, cfg_scale=scale)
        rx = O.integrate64(R.F_cfg(C.net("k3"), a, wa), (f64(x0),), STEPS, "midpoint")[0]
        ry = O.integrate64(R.F_cfg(C.net("k10w"), b, wb), (f64(y0),), STEPS, "midpoint")[0]
        ex, ey = err64(xs, rx), err64(ys, ry)
        print(f"pair labels {['same', 'two', 'x only'][[3.0, (3.0, 1.0), (0.5, 1.0)].index(scale)]}: |x - x64| {ex:.3e}, |y - y64| {ey:.3e}")
        assert ex <= bound(wa) and ey <= bound(wb), (ex, ey)
        # each chain is the single labelled loop of its net, bitwise
        sx = x0.to(dev).clone()
        _engine.sample_single(mx, sx, STEPS, solver="midpoint", labels=a, cfg_scale=wa)
        assert torch.equal(xs, sx)


def test_more_steps_than_the_class_table_holds(dev):
    m = C.net("k10w").to(dev)           # K + 1 = 11 classes: 372 Euler steps per call
    steps, B = 380, 2
    y = torch.tensor([3, 10], dtype=torch.int32, device=dev)
    auto = start("k10w", dev, B)
    _engine.sample_single(m, auto, steps, labels=y, cfg_scale=1.0)  # (the Python layer splits)
    raw = C.RawSingleCfg(C.net("k10w"), start("k10w", dev, B), y, dev)
    before = raw.x.clone()
    assert raw.run(1.0, steps, 0, steps) == EINVAL and b"rows" in _lib.lib().rgfm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(raw.x, before)
    for b, e in ((0, 100), (100, 372), (372, 380)):
        assert raw.run(1.0, steps, b, e) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw.x, auto) and torch.isfinite(auto).all()
    # without labels the call holds 4096 steps, as it always did
    assert C.RawSingleCfg(C.net("k10w"), start("k10w", dev, B), None, dev).run(1.0, steps, 0, steps) == 0
    # midpoint: two stages per step
    assert raw.run(1.0, steps, 0, 187, C.MIDPOINT) == EINVAL and raw.run(1.0, steps, 379, 380, C.MIDPOINT) == 0


def test_c_abi_errors_come_back_before_any_launch(dev):
    L = _lib.lib()
    y = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    raw = C.RawSingleCfg(C.net("k3"), start("k3", dev, 2), y, dev)
    before = raw.x.clone()
    assert raw.run(3.0, STEPS, 0, STEPS, short=1) == ENOMEM
    assert raw.run(float("nan"), STEPS, 0, STEPS) == EINVAL
    assert raw.run(3.0, STEPS, 0, STEPS, C.MIDPOINT, sde=(1.0, 5)) == EINVAL
    plain = load_synth(M.FlexibleUNet(1, 8, 32, (1, 2), 1), 41).to(dev).eval()
    unl = C.RawSingleCfg(plain, raw.x, y, dev)
    assert unl.run(1.0, STEPS, 0, STEPS) == EINVAL and b"without classes" in L.rgfm_last_error()
    nb = ctypes.c_size_t()
    h = plain._engine.handle(dev)
    assert L.rgfm_unet_workspace_bytes(h, 2, ctypes.byref(nb)) == 0
    ws, t, out = torch.empty(nb.value, dtype=torch.uint8, device=dev), torch.zeros(2, device=dev), torch.empty_like(raw.x)
    assert L.rgfm_unet_forward_labels(h, C._p(raw.x), C._p(t), 2, C._p(y), C._p(out), 2, C._p(ws), nb.value, C._stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(raw.x, before)
    # a label outside 0..K read on the device is the null label: no address leaves the table
    wild = torch.tensor([7, -5], dtype=torch.int32, device=dev)
    a = C.RawSingleCfg(C.net("k3"), start("k3", dev, 2), wild, dev)
    b = C.RawSingleCfg(C.net("k3"), start("k3", dev, 2), torch.tensor([3, 3], dtype=torch.int32, device=dev), dev)
    assert a.run(1.0, STEPS, 0, STEPS) == 0 and b.run(1.0, STEPS, 0, STEPS) == 0
    torch.cuda.synchronize()
    assert torch.equal(a.x, b.x)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_state_untouched(dev):
    m, my = C.net("k3").to(dev), C.net("k10w").to(dev)
    plain = load_synth(M.FlexibleUNet(1, 8, 32, (1, 2), 1), 41).to(dev).eval()
    y = torch.tensor([0, 1, 2], device=dev)
    x, t = start("k3", dev, 3), torch.zeros(3, device=dev)
    x0, y0 = C.inputs("k3", 3)[0], C.inputs("k10w", 3)[0]
    keep = x.clone()
    pair = lambda method, **kw: FU.paired_sampler(m, my, None, method, 1.0, 3, STEPS, dev, 4, C.shape_of("k3"), C.shape_of("k10w"),
                                                  noise=(x0, y0, x0, y0), verbose=False, **kw)
    calls = {
        "mc_feng": lambda: pair("mc_feng", labels=y),
        "grad_log_ratio": lambda: pair("grad_log_ratio", labels=y),
        "sample_conditional": lambda: FU.sample_conditional(m, None, x, labels=y),
        "log_prob": lambda: FU.CFMSchedule().log_prob(m, x, 4, labels=y),
        "vjp": lambda: m.vjp(x, t, x, y=y),
        "divergence": lambda: m.divergence(x, t, x[None], y=y),
        "unlabelled net": lambda: _engine.sample_single(plain, x, STEPS, labels=y),
        "unlabelled forward": lambda: plain(x, t, y),
        "K + 1": lambda: _engine.sample_single(m, x, STEPS, labels=torch.tensor([0, 4, 1], device=dev)),
        "-1": lambda: _engine.sample_single(m, x, STEPS, labels=torch.tensor([0, -1, 1], device=dev)),
        "forward K + 1": lambda: m(x, t, torch.tensor([0, 4, 1], device=dev)),
        "train -1": lambda: m.forward_train(x, t, torch.tensor([0, -1, 1], device=dev)),
        "shape": lambda: _engine.sample_single(m, x, STEPS, labels=y[:2]),
        "scale without labels": lambda: _engine.sample_single(m, x, STEPS, cfg_scale=3.0),
        "FlowMatchingModel": lambda: FU.CFMSchedule().sample(M.FlowMatchingModel().to(dev), 3, 2, dev, labels=y),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.RgfmError):
            call()
        torch.cuda.synchronize()
        assert torch.equal(x, keep), name
    # ... and in each of them the net stays usable without labels
    assert torch.isfinite(FU.CFMSchedule().log_prob(m, x, 2)[0]).all()


def test_labelled_nets_inside_an_mc_feng_loop_run_as_their_null_row(dev):
    mx, my = C.net("k3").to(dev), C.net("k10w").to(dev)
    B, N, gamma = 3, 5, 0.7
    g = torch.Generator().manual_seed(31)
    mcx, mcy = 0.5 * torch.randn(N, *C.shape_of("k3"), generator=g), 0.5 * torch.randn(N, *C.shape_of("k10w"), generator=g)
    r = torch.exp(0.5 * torch.randn(N, generator=g))
    x0, y0 = C.inputs("k3", B)[0], C.inputs("k10w", B)[0]
    x, y = x0.to(dev).clone(), y0.to(dev).clone()
    _engine.sample_pair(mx, my, x, y, mcx.to(dev), mcy.to(dev), r.to(dev), STEPS, gamma)
    Fp = O.F_pair_mc(R.velocity_labels_of(C.net("k3"), None), R.velocity_labels_of(C.net("k10w"), None),
                     f64(mcx).reshape(N, -1), f64(mcy).reshape(N, -1), f64(r), gamma)
    wx, wy = O.integrate64(Fp, (f64(x0), f64(y0)), STEPS)
    ex, ey = err64(x, wx), err64(y, wy)
    print(f"mc_feng over two labelled nets without labels: |x - x64| {ex:.3e}, |y - y64| {ey:.3e}")
    assert ex <= TOL_SAMPLER and ey <= TOL_SAMPLER


# ------------------------------------------------------------------ 6. a caller's stream
@pytest.mark.parametrize("cid", ["cfg_forward_labels", "cfg_forward_train_labels", "cfg_sample_single[euler+sde]",
                                 "cfg_sample_single[midpoint]", "cfg_sample_two"])
def test_on_a_late_stream_is_the_null_stream_run_bitwise(dev, monkeypatch, cid):
    for k in ("RGFM_RANGE_CHECK", "RGFM_OVERLAP", "RGFM_CONV", "RGFM_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    case = SC.BY_ID[cid]
    warm, _ = SC.null_stream_run(case, dev)
    want, wall_ms = SC.null_stream_run(case, dev)
    assert all(torch.equal(a, b) for a, b in zip(want, warm)) and len(want) > 0
    run = SC.late_stream_run(case, dev, SC.delay_for(wall_ms))
    assert run.delay_pending, f"{cid}: the delay kernel had ended when the call returned: this run has shown nothing"
    assert len(run.clones) == len(want)
    for i, (a, b) in enumerate(zip(run.clones, want)):
        assert torch.equal(a, b), f"{cid}: tensor {i} differs from the null-stream run"
