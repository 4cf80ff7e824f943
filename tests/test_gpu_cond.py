"""Conditional sampling on the GPU: the cross evaluation of the ratio estimators (rgfm_ratio_eval_cross), the one-sided
MC guidance block (rgfm_guidance_apply_cond), the one-net guided loop (rgfm_sample_cond) and the Python surface
(sample_conditional, the --given / --condition CLI), each against float64.

Yardsticks: tests/ratio_ref64.py and tests/ratio_flex_ref64.py on the explicitly tiled pairs for the cross matrix;
tests/cond_ref64.py (tied to guidance_ref64.guidance64 by tests/test_cond_ref64_cpu.py) for the block; cond_ref64's loop
over tests/unet_ref64.py for the samplers.

Bounds.  Cross matrix: 1e-5 absolute on score and log-ratio (TOL_EVAL of tests/test_gpu_ratio_flex.py); the ratio output
as |log(out) - l64| <= 1e-5.  Block: guidance_ref64.tol_w and velocity_bound, unchanged -- the block is the paired one
with one distance term fewer.  Samplers: 1e-4 (TOL_SAMPLER of the existing sampler tests)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cond_ref64 as C
import guidance_ref64 as G
import ratio_flex_ref64 as RF
import ratio_ref64 as RR
import unet_ref64 as U
from helpers import make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth
from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional

pytestmark = pytest.mark.gpu

TOL_EVAL, TOL_SAMPLER = 1e-5, 1e-4
FEAT, HID, W_SEED = 64, 128, 31
SENTINEL = -7777.0
PAD = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ 1. cross evaluation
def tiled(x, y):
    """The nx * ny explicit pairs in the matrix's row-major order: (x_i, y_j) at i * ny + j."""
    return x.repeat_interleave(y.shape[0], 0), y.repeat(x.shape[0], *([1] * (y.dim() - 1)))


def log_ratio_of(s, loss_type):
    return F.logsigmoid(s) - F.logsigmoid(-s) if loss_type == "disc" else torch.log(F.softplus(s) + 1e-8)


def flex_module(dev):
    return load_synth(M.FlexibleRatioEstimator(1, 3, FEAT, HID), W_SEED).eval().to(dev)


def flex_inputs(nx, ny):
    g = torch.Generator().manual_seed(2000 + 100 * nx + ny)
    return torch.randn(nx, 1, 8, 8, generator=g), torch.randn(ny, 3, 12, 12, generator=g)


_score64 = {}


def flex_score64(nx, ny):
    """float64 scores [nx, ny] of the flexible case: computed once, shared, never modified."""
    if (nx, ny) not in _score64:
        x, y = flex_inputs(nx, ny)
        sd = RF.params64(flex_module("cpu"), requires_grad=False)
        _score64[(nx, ny)] = RF.forward64(sd, *tiled(x, y)).reshape(nx, ny)
    return _score64[(nx, ny)]


def check_cross(m, xd, yd, s64, tag):
    nx, ny = s64.shape
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        l64 = log_ratio_of(s64, lt)
        s, lr = m.forward_cross(xd, yd), m.cross_log_ratio(xd, yd)
        r = m._engine.eval_cross(xd, yd, "ratio")
        assert s.shape == lr.shape == r.shape == (nx, ny)
        errs = {"score": float((s.cpu().double() - s64).abs().max()),
                "log_ratio": float((lr.cpu().double() - l64).abs().max()),
                "ratio": float((r.cpu().double().log() - l64).abs().max())}
        print(f"cross {tag} {nx}x{ny} {lt}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= TOL_EVAL, (tag, lt, k, v)
    m.loss_type = "disc"


@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 5), (13, 11)])
def test_cross_flexible_vs_float64(dev, nx, ny):
    x, y = flex_inputs(nx, ny)
    check_cross(flex_module(dev), x.to(dev), y.to(dev), flex_score64(nx, ny), "flexible")


@pytest.mark.parametrize("tag,kind,sx,sy,nx,ny", [("ratio_ms", "mnist_svhn", (1, 32, 32), (3, 32, 32), 3, 5),
                                                   ("ratio28", "mnist28", (1, 28, 28), (1, 28, 28), 4, 3)])
def test_cross_fixed_kinds_vs_float64(dev, tag, kind, sx, sy, nx, ny):
    g = torch.Generator().manual_seed(2100 + nx)
    x, y = torch.randn(nx, *sx, generator=g), torch.randn(ny, *sy, generator=g)
    sd = RR.params64(make_module(tag), requires_grad=False)
    s64 = RR.forward64(kind, sd, *tiled(x, y), training=False).reshape(nx, ny)
    check_cross(make_module(tag, dev), x.to(dev), y.to(dev), s64, tag)


def test_cross_chunks_ragged_and_inside_matrix_rows(dev, monkeypatch):
    """13 x 11 = 143 pairs in chunks of 32: four full chunks and one of 15, every boundary inside a matrix row (11 does
    not divide 32).  Within the bound, bitwise equal to the default chunking (a pair's arithmetic does not depend on
    the chunk it falls into), and nothing is written outside the matrix."""
    nx, ny = 13, 11
    x, y = (t.to(dev) for t in flex_inputs(nx, ny))
    m = flex_module(dev)
    plain = {w: m._engine.eval_cross(x, y, w).clone() for w in ("score", "log_ratio", "ratio")}
    monkeypatch.setenv("RGFM_CROSS_ROWS", "32")
    check_cross(m, x, y, flex_score64(nx, ny), "flexible, RGFM_CROSS_ROWS=32")
    for w, want in plain.items():
        got = m._engine.eval_cross(x, y, w)
        print(f"chunked vs default {w}: bitwise equal {torch.equal(got, want)}, max diff {float((got - want).abs().max()):.1e}")
        assert torch.equal(got, want), w
    # the raw call into the middle of a larger buffer, workspace exactly as asked for
    L = _lib.lib()
    h = m._engine.handle(dev)
    nb = ctypes.c_size_t()
    _lib.check(L.rgfm_ratio_cross_workspace_bytes(h, nx, ny, ctypes.byref(nb)))
    ws = torch.full((nb.value // 4,), float("nan"), device=dev)
    big = torch.full((PAD + nx * ny + PAD,), SENTINEL, device=dev)
    _lib.check(L.rgfm_ratio_eval_cross(h, _p(x), nx, _p(y), ny, _p(big[PAD:]), 0, _p(ws), nb.value, _stream()))
    torch.cuda.synchronize()
    assert bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all())
    assert torch.equal(big[PAD:-PAD].view(nx, ny), plain["score"])
    assert L.rgfm_ratio_eval_cross(h, _p(x), nx, _p(y), ny, _p(big[PAD:]), 0, _p(ws), nb.value - 1, _stream()) == -2
    assert L.rgfm_ratio_cross_workspace_bytes(h, 0, ny, ctypes.byref(nb)) == -1
    assert L.rgfm_ratio_cross_workspace_bytes(h, nx, 0, ctypes.byref(nb)) == -1


def test_cross_swapping_two_x_images_swaps_two_rows(dev):
    nx, ny = 13, 11
    x, y = flex_inputs(nx, ny)
    perm = list(range(nx))
    perm[2], perm[9] = perm[9], perm[2]
    m = flex_module(dev)
    s = m.forward_cross(x[perm].to(dev), y.to(dev)).cpu().double()
    err = float((s - flex_score64(nx, ny)[perm]).abs().max())
    print(f"swapped rows: err {err:.3e}")
    assert err <= TOL_EVAL
    assert float((s[2] - flex_score64(nx, ny)[9]).abs().max()) <= TOL_EVAL


def test_cross_follows_an_in_place_parameter_update(dev):
    """rgfm_ratio_update_params repacks the cross path's weight slices: after an in-place edit of the first score Linear
    the same handle gives the float64 answer of the new parameters."""
    nx, ny = 3, 5
    x, y = flex_inputs(nx, ny)
    m = flex_module(dev)
    before = m.forward_cross(x.to(dev), y.to(dev)).clone()
    h0 = m._engine.handle(dev).value
    with torch.no_grad():
        m.score_net[0].weight.mul_(0.5)
        m.score_net[0].weight[:, FEAT:].add_(0.01)
    after = m.forward_cross(x.to(dev), y.to(dev))
    assert m._engine.handle(dev).value == h0
    s64 = RF.forward64(RF.params64(m, requires_grad=False), *tiled(x, y)).reshape(nx, ny)
    assert float((after.cpu().double() - s64).abs().max()) <= TOL_EVAL
    assert float((after - before).abs().max()) > 1e-3


# ------------------------------------------------------------------ 2. the one-sided guidance block
def _to(dev, inp, rows=None):
    d = {k: torch.tensor(v, device=dev) for k, v in inp.items()}
    if rows is not None:
        for k in ("s", "v", "R"):
            d[k] = d[k][rows].clone()
    return d


def _apply(d, t, gamma):
    w = _engine.guidance_apply_cond(d["s"], d["v"], d["m"], d["R"], t, gamma, True)
    return w, d["v"]


def _rel_dw(w, w64):
    keep = w64 > 0
    return float((np.abs(w - w64)[keep] / w64[keep]).max())


@pytest.mark.parametrize("centre", C.CENTRES)
@pytest.mark.parametrize("si", range(len(C.STEPS)))
@pytest.mark.parametrize("ci", range(len(C.CASES)))
def test_block_weights_and_velocity_vs_float64(dev, ci, si, centre):
    B, N, dim = C.CASES[ci]
    t, gamma = C.STEPS[si]
    inp, ref = C.case(ci, si, centre)
    w, v = (a.cpu().numpy().astype(np.float64) for a in _apply(_to(dev, inp), t, gamma))
    tw = G.tol_w(t, centre)
    bound = C.velocity_bound(inp, ref, N, t, gamma, tw)
    dw, dv = _rel_dw(w, ref["w"]), float(np.abs(v - ref["v"]).max())
    dsum = float(np.abs(w.sum(1) - 1).max())
    print(f"cond64 {C.CASES[ci]} t={t} centre={centre}: dw {dw:.2e} / tol_w {tw:.1e} = {dw / tw:.2f}   "
          f"dv {dv:.2e} / bound {bound:.2e} = {dv / bound:.2f}   |sum w - 1| {dsum:.1e}")
    assert np.isfinite(w).all() and np.isfinite(v).all()
    assert dw <= tw, (dw, tw)
    assert dsum < 1e-5, dsum
    assert dv <= bound, (dv, bound)


def test_block_reads_each_rows_own_ratio_row(dev):
    """Every row has a distinct ratio row; one row's ratios become a one-hot: that row's weights are the one-hot within
    1e-6, and every other row keeps its bits.  A kernel with a wrong row stride fails both."""
    ci, si, centre = 1, 1, 0.0
    B, N, dim = C.CASES[ci]
    t, gamma = C.STEPS[si]
    inp = C.case(ci, si, centre)[0]
    base_w, base_v = _apply(_to(dev, inp), t, gamma)
    row, k = 17, 41
    d = _to(dev, inp)
    d["R"][row] = 0
    d["R"][row, k] = 1
    w, v = _apply(d, t, gamma)
    onehot = torch.zeros(N, device=dev)
    onehot[k] = 1
    assert float((w[row] - onehot).abs().max()) <= 1e-6
    others = torch.arange(B, device=dev) != row
    assert torch.equal(w[others], base_w[others]) and torch.equal(v[others], base_v[others])
    assert not torch.equal(v[row], base_v[row])


def test_block_rows_do_not_depend_on_the_batch(dev):
    ci, si = 1, 2
    B = C.CASES[ci][0]
    t, gamma = C.STEPS[si]
    inp = C.case(ci, si, 0.0)[0]
    full = _apply(_to(dev, inp), t, gamma)
    for rows in (slice(0, 1), slice(B - 1, B), slice(B - 7, B)):
        part = _apply(_to(dev, inp, rows), t, gamma)
        for f, p in zip(full, part):
            assert torch.equal(f[rows], p), rows


def test_block_argument_errors(dev):
    """n_mc = 0 is RGFM_EINVAL and a workspace one byte short is RGFM_ENOMEM; v is not touched."""
    inp = C.case(0, 1, 1.0)[0]
    B, N, dim = C.CASES[0]
    d = _to(dev, inp)
    v0 = d["v"].clone()
    L = _lib.lib()
    nb = ctypes.c_size_t()
    _lib.check(L.rgfm_guidance_workspace_bytes(B, N, ctypes.byref(nb)))
    ws = torch.zeros(nb.value // 4, device=dev)
    call = lambda n, nbytes: L.rgfm_guidance_apply_cond(_p(d["s"]), _p(d["v"]), _p(d["m"]), _p(d["R"]), B, n, dim, 0.5, 1.0, None,
                                                        _p(ws), nbytes, _stream())
    assert call(0, nb.value) == -1
    assert call(N, nb.value - 1) == -2
    torch.cuda.synchronize()
    assert torch.equal(d["v"], v0)
    assert call(N, nb.value) == 0


# ------------------------------------------------------------------ 3. the one-net guided loop
B_S, N_S, STEPS_S = 5, 7, 6
NETS = {"unet28": lambda: make_module("unet28"),
        "rgb32": lambda: load_synth(M.FlexibleUNet(3, 32, 32, (1, 2), 1), 51).eval()}


def sampler_inputs(tag):
    net = NETS[tag]()
    shape = (net.in_channels, net.img_size, net.img_size)
    g = torch.Generator().manual_seed(3000 + len(tag))
    s0 = torch.randn(B_S, *shape, generator=g)
    mc = 0.5 * torch.randn(N_S, *shape, generator=g)
    R = torch.exp(0.5 * torch.randn(B_S, N_S, generator=g))
    return net, s0, mc, R


_loop64 = {}


def loop64(tag, gamma):
    """float64 result of the guided loop: computed once per (net, gamma), shared, never modified."""
    if (tag, gamma) not in _loop64:
        net, s0, mc, R = sampler_inputs(tag)
        cfg, sd = U.cfg_of(net), U.params64(net, requires_grad=False)
        vel = lambda s, t: U.forward64(cfg, sd, torch.from_numpy(s), torch.tensor([t])).numpy()
        _loop64[(tag, gamma)] = C.sample_cond64(vel, s0.numpy(), mc.reshape(N_S, -1).numpy(), R.numpy(), STEPS_S, gamma)
    return _loop64[(tag, gamma)]


def run_cond(net, s0, mc, R, gamma, dev, ranges=((0, STEPS_S),)):
    s = s0.to(dev).clone()
    for b, e in ranges:
        _engine.sample_cond(net, s, mc.to(dev), R.to(dev), STEPS_S, gamma, b, e)
    return s


@pytest.mark.parametrize("gamma", [0.0, 0.7])
@pytest.mark.parametrize("tag", list(NETS))
def test_sample_cond_vs_float64_split_and_rows(dev, tag, gamma):
    net, s0, mc, R = sampler_inputs(tag)
    net = net.to(dev)
    got = run_cond(net, s0, mc, R, gamma, dev)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - loop64(tag, gamma)).max())
    print(f"sample_cond {tag} gamma={gamma}: err vs float64 {err:.3e}")
    assert err <= TOL_SAMPLER, err
    # splitting the integration at a step boundary changes no bit
    assert torch.equal(run_cond(net, s0, mc, R, gamma, dev, ((0, 2), (2, 5), (5, STEPS_S))), got)
    # a row run alone with its own ratio row: the same bits
    for b in (0, B_S - 1):
        assert torch.equal(run_cond(net, s0[b:b + 1], mc, R[b:b + 1], gamma, dev), got[b:b + 1]), b
    unguided = _engine.sample_single(net, s0.to(dev).clone(), STEPS_S)
    diff = float((got - unguided).abs().max())
    print(f"sample_cond {tag} gamma={gamma}: max |guided - unguided| {diff:.3e}")
    if gamma == 0.0:
        assert diff <= 1e-6, diff
    else:
        assert diff > 1e-3, diff


def test_sample_cond_argument_errors(dev):
    net, s0, mc, R = sampler_inputs("unet28")
    net = net.to(dev)
    s, mcd, Rd = s0.to(dev).clone(), mc.to(dev), R.to(dev)
    L = _lib.lib()
    h = net._engine.handle(dev)
    nb = ctypes.c_size_t()
    assert L.rgfm_sample_cond_workspace_bytes(h, B_S, 0, ctypes.byref(nb)) == -1
    _lib.check(L.rgfm_sample_cond_workspace_bytes(h, B_S, N_S, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    call = lambda n, nbytes: L.rgfm_sample_cond(h, _p(s), _p(mcd), _p(Rd), n, B_S, STEPS_S, 0.7, 0, STEPS_S, _p(ws), nbytes, _stream())
    assert call(0, nb.value) == -1 and b"n_mc" in L.rgfm_last_error()
    assert call(4097, nb.value) == -1
    assert call(N_S, nb.value - 1) == -2
    torch.cuda.synchronize()
    assert torch.equal(s, s0.to(dev))
    with pytest.raises(_lib.RgfmError):  # a ratio vector instead of a row per sample
        _engine.sample_cond(net, s, mcd, Rd[0], STEPS_S, 0.7)


# ------------------------------------------------------------------ 4. Python end to end
def e2e_nets(dev):
    fx = load_synth(M.FlexibleUNet(3, 16, 32, (1, 2), 2), 41).eval().to(dev)
    fy = load_synth(M.FlexibleUNet(1, 16, 32, (1, 2), 2), 42).eval().to(dev)
    rr = load_synth(M.FlexibleRatioEstimator(3, 1, FEAT, HID), W_SEED).eval().to(dev)
    return fx, fy, rr


@pytest.mark.parametrize("given", ["x", "y"])
def test_sample_conditional_vs_float64_composition(dev, given):
    fx, fy, rr = e2e_nets(dev)
    target = fy if given == "x" else fx
    cshape, tshape = ((3, 16, 16), (1, 16, 16)) if given == "x" else ((1, 16, 16), (3, 16, 16))
    B, N, S, gamma = 4, 6, 4, 0.7
    cond = torch.randn(B, *cshape, generator=torch.Generator().manual_seed(61))
    # the documented draw order: MC noise, then the start noise
    torch.cuda.manual_seed(123)
    mc0, s0 = torch.randn(N, *tshape, device=dev), torch.randn(B, *tshape, device=dev)
    torch.cuda.manual_seed(123)
    out = sample_conditional(target, rr, cond.to(dev), given, S, gamma, N)
    assert out.shape == (B, *tshape)
    cfg, sd = U.cfg_of(target), U.params64(target, requires_grad=False)
    vel = lambda s, t: U.forward64(cfg, sd, torch.from_numpy(s), torch.tensor([t])).numpy()
    mc = mc0.cpu().double().numpy()
    for step in range(S):
        mc = mc + vel(mc, step / S) / S
    sdr = RF.params64(rr, requires_grad=False)
    mct = torch.from_numpy(mc)
    if given == "x":
        lr = RF.log_ratio64(sdr, *tiled(cond, mct), "disc").reshape(B, N)
    else:
        lr = RF.log_ratio64(sdr, *tiled(mct, cond), "disc").reshape(N, B).T
    want = C.sample_cond64(vel, s0.cpu().numpy(), mc.reshape(N, -1), lr.exp().numpy(), S, gamma)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    print(f"sample_conditional given={given}: err vs float64 {err:.3e}")
    assert err <= TOL_SAMPLER, err
    # mc_samples: the terminal MC set of that call, and the generator where the call left it after the MC draw
    torch.cuda.manual_seed(123)
    mc1 = torch.randn(N, *tshape, device=dev)
    _engine.sample_single(target, mc1, S)
    again = sample_conditional(target, rr, cond.to(dev), given, S, gamma, N, mc_samples=mc1)
    assert torch.equal(again, out)


def test_flow_matching_model_target_raises(dev):
    rr = make_module("ratio28", dev)
    cond = torch.zeros(2, 1, 28, 28, device=dev)
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        sample_conditional(make_module("fm_original", dev), rr, cond, "x", 2, 0.5, 3)
    with pytest.raises(ValueError):
        sample_conditional(make_module("unet28", dev), rr, cond, "z", 2, 0.5, 3)


def test_cli_given_mnist_equals_the_direct_call(dev, tmp_path, monkeypatch):
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
    assert sample_mnist_svhn.main(["--given", "mnist", "--condition", "cond.npy", "--guidance_strength", "0.5", "--num_steps", "4",
                                   "--mc_batch_size", "5", "--seed", "9"]) == 0
    saved = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_given_mnist_gamma0.5.pt")
    R.utils.set_seed(9)
    want = sample_conditional(fs.to(dev), rr.to(dev), cond.to(dev), "x", 4, 0.5, 5, device=dev)
    assert saved["svhn"].shape == (3, 3, 32, 32)
    assert torch.equal(saved["svhn"], want.cpu()) and torch.equal(saved["mnist"], cond)
    with pytest.raises(SystemExit):
        sample_mnist_svhn.main(["--given", "mnist"])
