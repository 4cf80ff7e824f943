"""FlowMatchingModel's eval and sampling path (rgfm_fmnet_forward / _sample_single / _sample_pair, the in-place
rgfm_fmnet_update_params) on the GPU against the float64 restatement (tests/fmnet_ref64.py) across what check_fm_desc
accepts: the smallest and the largest descriptor (64, 16) and (1024, 1024) -- the float64 side of the latter takes
0.7 s on the CPU, so nothing was trimmed -- F + T no multiple of 64, T >> F, ragged batches, t = 0 and t = 1 - 1/1000,
under each conv / GroupNorm mode; the time embedding isolated as v(x, ta) - v(x, tb); rows independent of the launch
shape at B = 512; both sampler loops against a float64 Euler loop written out in fmnet_ref64; the in-place refresh.

Tolerances are the suite's own: TOL_EVAL = 1e-5 on an output (absolute; times max(1, max |v64|), the U-Net sweep's
rule, for the two descriptors above 320 -- fmnet_ref64.eval_scale), TOL_SAMPLER = 1e-4 on a sampler state.  The
reference's own fp32 CPU forward differs from float64 by at most 2.9e-6 over the cases (1.8e-6 .. 2.9e-6,
tests/test_fmnet_eval_cpu.py, which asserts it to be within a third of the tolerance), and the two embedding mistakes
and the guidance-threshold mistake this module is meant to catch are shown there to move the float64 answers by at
least ten tolerances."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import fmnet_ref64 as R
from helpers import maxdiff
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd._engine import _ptr, _stream

pytestmark = pytest.mark.gpu

TOL_EVAL = 1e-5
TOL_SAMPLER = 1e-4

MODES = {"default": {}, "bx3": {"RGFM_CONV": "bx3"}, "f32": {"RGFM_CONV": "f32"}, "table": {"RGFM_GN": "table"},
         "table_nofuse": {"RGFM_GN": "table", "RGFM_FUSE_FIN": "0"}, "hx2s0": {"RGFM_HX2S": "0"},
         "hx2p0": {"RGFM_HX2P": "0"}}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


_modules = {}


def module_of(F_dim, T_dim, dev, seed=R.SEED_W):
    """load_synth(M.FlowMatchingModel(1, F, T), seed).eval() on the device; one per (F, T, seed), shared by the tests
    that do not edit it (the modes are read per call, a handle serves them all)."""
    key = (F_dim, T_dim, seed)
    if key not in _modules:
        _modules[key] = new_module(F_dim, T_dim, dev, seed)
    return _modules[key]


def new_module(F_dim, T_dim, dev, seed=R.SEED_W):
    return copy.deepcopy(R.module_cpu(F_dim, T_dim, seed)).to(dev)


def set_mode(mode, monkeypatch):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def checked_forward(m, x, t, dev, what):
    """m(x, t) with the two assertions every forward of this module makes: no call was repeated on a fallback
    arithmetic and the handle's range flag is clear (or the fp16 modes would be testing the bf16 / fp32 kernels)."""
    fallbacks = _engine.range_fallbacks
    out = m(x.to(dev), t.to(dev))
    torch.cuda.synchronize()
    assert _engine.range_fallbacks == fallbacks, (what, _engine.last_range_flags)
    assert m._engine.read_range_flag(dev, reset=False) == 0, what
    return out


# ------------------------------------------------------------------ 1. forward across descriptor, batch, arithmetic
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("ci", range(len(R.EVAL_CASES)))
def test_forward_vs_float64(dev, ci, mode, monkeypatch):
    F_dim, T_dim, B, shared = R.EVAL_CASES[ci]
    set_mode(mode, monkeypatch)
    x, t = R.eval_inputs(ci)
    out = checked_forward(module_of(F_dim, T_dim, dev), x, t, dev, (ci, mode))
    v64 = R.eval_ref(ci)
    err, tol = maxdiff(out.cpu().numpy(), v64), TOL_EVAL * R.eval_scale(ci)
    print(f"\nforward F={F_dim} T={T_dim} B={B} shared_t={shared} mode={mode}: err {err:.3e} (tol {tol:.3e}, "
          f"max|v64| {np.abs(v64).max():.3f})")
    assert err < tol, (ci, mode, err)


# ------------------------------------------------------------------ 2. the time embedding alone
@pytest.mark.parametrize("F_dim,T_dim", R.EMBED_DIMS)
def test_time_embedding_through_output_differences(dev, F_dim, T_dim):
    """v(x, ta) - v(x, tb) at a fixed x depends on t through the embedding columns of the concat only: against float64
    for the t pairs of fmnet_ref64.EMBED_PAIRS, all pairs in one launch per side (per-row t)."""
    m = module_of(F_dim, T_dim, dev)
    x, ta, tb = R.embed_inputs(F_dim, T_dim)
    P = len(R.EMBED_PAIRS)
    X = x.repeat(P, 1, 1, 1)  # row 2 p + j: x[j] at pair p
    va = checked_forward(m, X, ta.repeat_interleave(2), dev, "ta")
    vb = checked_forward(m, X, tb.repeat_interleave(2), dev, "tb")
    d = (va.double() - vb.double()).cpu().numpy().reshape(P, 2, -1)
    d64 = R.embed_ref(F_dim, T_dim)
    errs = np.abs(d - d64).reshape(P, -1).max(1)
    for pair, e, r in zip(R.EMBED_PAIRS, errs, d64):
        print(f"\nembedding F={F_dim} T={T_dim} t pair {pair}: err {e:.3e} of max|d64| {np.abs(r).max():.3e}")
    assert (errs < TOL_EVAL).all(), errs
    # one shared t (t_count == 1) is the same embedding row for every sample
    v1 = checked_forward(m, x, tb[-1:], dev, "shared")
    assert torch.equal(v1, vb[-2:])


# ------------------------------------------------------------------ 3. rows do not depend on the launch shape
@pytest.mark.parametrize("mode", ["default", "bx3"])
@pytest.mark.parametrize("F_dim,T_dim", [(256, 128), (64, 16)])
def test_rows_do_not_depend_on_the_launch_shape(dev, F_dim, T_dim, mode, monkeypatch):
    """Bitwise: a row's result is the same in a launch of 512 rows and in an under-filled one (other workgroup shapes
    in the convs, other row-tile counts in the Linears, whose split-K order is fixed), and the full launch's first
    rows are float64's."""
    set_mode(mode, monkeypatch)
    B = 512
    m = module_of(F_dim, T_dim, dev)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 1, 28, 28, generator=g)
    t = torch.rand(B, generator=g)
    full = checked_forward(m, x, t, dev, (F_dim, mode))
    with torch.no_grad():
        v64 = R.forward64(R.sd64(F_dim, T_dim), x[:3], t[:3]).numpy()
    err = maxdiff(full[:3].cpu().numpy(), v64)
    print(f"\nrows F={F_dim} T={T_dim} B={B} mode={mode}: first rows err {err:.3e}")
    assert err < TOL_EVAL
    x, t = x.to(dev), t.to(dev)
    for lo, hi in ((0, 8), (250, 263), (509, 512)):
        part = checked_forward(m, x[lo:hi].contiguous(), t[lo:hi].contiguous(), dev, (lo, hi))
        assert torch.equal(part, full[lo:hi]), (F_dim, mode, lo, hi, float((part - full[lo:hi]).abs().max()))


# ------------------------------------------------------------------ 4. samplers vs a float64 Euler loop
def checked_sampler(engines, dev, fn):
    fallbacks = _engine.range_fallbacks
    out = fn()
    torch.cuda.synchronize()
    assert _engine.range_fallbacks == fallbacks, _engine.last_range_flags
    for e in engines:
        assert e.read_range_flag(dev, reset=False) == 0
    return out


@pytest.mark.parametrize("F_dim,T_dim", R.SINGLE_DIMS)
def test_sample_single_vs_float64(dev, F_dim, T_dim):
    m = module_of(F_dim, T_dim, dev)
    x0 = R.single_inputs(F_dim, T_dim).to(dev)
    run = lambda x, *a: checked_sampler([m._engine], dev, lambda: _engine.sample_single(m, x, *a))
    for num_steps in (1, 7):  # 1: a single step at t = 0 with dt = 1
        xs = run(x0.clone(), num_steps)
        err = maxdiff(xs.cpu().numpy(), R.single_ref(F_dim, T_dim, num_steps))
        print(f"\nsample_single F={F_dim} T={T_dim} num_steps={num_steps}: err {err:.3e}")
        assert err < TOL_SAMPLER
    x1 = x0.clone()
    run(x1, 7, 0, 3)
    assert not torch.equal(x1, xs) and not torch.equal(x1, x0)
    run(x1, 7, 3, 7)
    assert torch.equal(x1, xs)  # [0, 3) then [3, 7) is the single call, bitwise
    x2 = x0.clone()
    run(x2, 7, 4, 4)
    assert torch.equal(x2, x0)  # the empty window


def run_pair(fx, fy, dev, n_mc, gamma, num_steps, begin, end):
    x, y, mx, my, r = (None if a is None else a.to(dev) for a in R.pair_inputs(n_mc))
    checked_sampler([fx._engine, fy._engine], dev,
                    lambda: _engine.sample_pair(fx, fy, x, y, mx, my, r, num_steps, gamma, begin, end))
    return x, y


@pytest.mark.parametrize("n_mc,gamma,num_steps,begin,end", R.PAIR_CASES)
def test_sample_pair_vs_float64(dev, n_mc, gamma, num_steps, begin, end, monkeypatch):
    """Two handles of different dims in one loop, (256, 128) for x and (64, 16) for y, against pair64 (the float64 loop
    with guidance_ref64.guidance64).  The 1000-step window [0, 4) holds the threshold: step 1 (t = 0.001 exactly)
    unguided, step 2 the first guided one."""
    (fxd, txd), (fyd, tyd) = R.PAIR_DIMS
    fx, fy = module_of(fxd, txd, dev), module_of(fyd, tyd, dev, R.PAIR_SEED_Y)
    x, y = run_pair(fx, fy, dev, n_mc, gamma, num_steps, begin, end)
    x64, y64 = R.pair_ref(n_mc, gamma, num_steps, begin, end)
    ex, ey = maxdiff(x.cpu().numpy(), x64), maxdiff(y.cpu().numpy(), y64)
    print(f"\nsample_pair n_mc={n_mc} gamma={gamma} steps [{begin},{end}) of {num_steps}: err x {ex:.3e} y {ey:.3e}")
    assert ex < TOL_SAMPLER and ey < TOL_SAMPLER
    if num_steps == 1000:  # the two nets one after the other on one stream: the same numbers
        monkeypatch.setenv("RGFM_OVERLAP", "0")
        xs, ys = run_pair(fx, fy, dev, n_mc, gamma, num_steps, begin, end)
        assert torch.equal(xs, x) and torch.equal(ys, y)


def test_sampler_argument_errors(dev):
    """Bad step ranges, a workspace one byte short and a t_count that is neither 1 nor B come back as RgfmError; the
    state is untouched and the handles go on working."""
    fx, fy = module_of(64, 16, dev), module_of(64, 16, dev, R.PAIR_SEED_Y)
    B = R.SAMPLER_B
    x0 = R.single_inputs(64, 16).to(dev)
    x, y = x0.clone(), x0.clone()
    for begin, end in ((0, 8), (5, 4)):  # step_end > num_steps; step_begin > step_end
        with pytest.raises(_lib.RgfmError, match="bad step range"):
            _engine.sample_single(fx, x, 7, begin, end)
        with pytest.raises(_lib.RgfmError, match="bad step range"):
            _engine.sample_pair(fx, fy, x, y, None, None, None, 7, 0.5, begin, end)
    L = _lib.lib()
    with torch.cuda.device(dev):
        h, hy = fx._engine.handle(dev), fy._engine.handle(dev)
        n = ctypes.c_size_t()
        _lib.check(L.rgfm_fmnet_workspace_bytes(h, B, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
        with pytest.raises(_lib.RgfmError, match="workspace too small"):
            _lib.check(L.rgfm_fmnet_sample_single(h, _ptr(x), B, 7, 0, 7, _ptr(ws), n.value - 1, _stream(dev)))
        t, out = torch.zeros(B, device=dev), torch.empty_like(x)
        with pytest.raises(_lib.RgfmError, match="workspace too small"):
            _lib.check(L.rgfm_fmnet_forward(h, _ptr(x), _ptr(t), B, _ptr(out), B, _ptr(ws), n.value - 1, _stream(dev)))
        for t_count in (0, 2, B + 1):
            with pytest.raises(_lib.RgfmError, match="t_count"):
                _lib.check(L.rgfm_fmnet_forward(h, _ptr(x), _ptr(t), t_count, _ptr(out), B, _ptr(ws), n.value,
                                                _stream(dev)))
        _lib.check(L.rgfm_fmnet_sample_pair_workspace_bytes(h, hy, B, 0, ctypes.byref(n)))
        ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
        with pytest.raises(_lib.RgfmError, match="workspace too small"):
            _lib.check(L.rgfm_fmnet_sample_pair(h, hy, _ptr(x), _ptr(y), None, None, None, 0, B, 7, 0.5, 0, 7, _ptr(ws),
                                                n.value - 1, _stream(dev)))
    with pytest.raises(_lib.RgfmError, match="1 or 5 elements"):
        fx(x, torch.zeros(2, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(y, x0)
    _engine.sample_single(fx, x, 7)
    assert maxdiff(x.cpu().numpy(), R.single_ref(64, 16, 7)) < TOL_SAMPLER


# ------------------------------------------------------------------ 5. in-place refresh at other dims
def fresh_copy(m, dev):
    f = M.FlowMatchingModel(1, m.feature_dim, m.time_emb_dim).to(dev).eval()
    f.load_state_dict(m.state_dict())
    return f


@pytest.mark.parametrize("mode", ["default", "bx3"])
def test_in_place_refresh(dev, mode, monkeypatch):
    """(320, 48): after an in-place edit of every parameter the SAME handle serves the next forward
    (rgfm_fmnet_update_params) and computes, bitwise, what a module created from those values does -- also across a
    GroupNorm whose parameters leave the fp16 window (norm_params_ok: 8 |gamma| + |beta| >= 1024 demotes the conv
    behind it) and back."""
    set_mode(mode, monkeypatch)
    F_dim, T_dim = 320, 48
    m = new_module(F_dim, T_dim, dev)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(5, 1, 28, 28, generator=g).to(dev)
    t = torch.tensor([0.0, 0.3, 0.6, 0.9, R.T_LATE]).to(dev)
    h0 = m._engine.handle(dev).value
    v0 = checked_forward(m, x, t, dev, "before").clone()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.0 + 0.01 * torch.randn(p.shape, generator=g).to(dev))
    v = checked_forward(m, x, t, dev, "edited").clone()
    assert m._engine.handle(dev).value == h0
    assert not torch.equal(v, v0)
    assert torch.equal(v, checked_forward(fresh_copy(m, dev), x, t, dev, "fresh"))
    with torch.no_grad():
        v64 = R.forward64(R.params64(m, requires_grad=False), x.cpu(), t.cpu()).numpy()
    err = maxdiff(v.cpu().numpy(), v64)
    print(f"\nrefresh F={F_dim} T={T_dim} mode={mode}: err {err:.3e}")
    assert err < TOL_EVAL
    # decoder.gn1 out of the window: 8 max|gamma| = 2048
    gn = m.decoder.gn1
    scale = 2048.0 / (8.0 * float(gn.weight.abs().max()))
    with torch.no_grad():
        gn.weight.mul_(scale)
    assert 8.0 * float(gn.weight.abs().max()) + float(gn.bias.abs().max()) >= 1024.0
    vs = m(x, t).clone()
    assert m._engine.handle(dev).value == h0
    assert torch.isfinite(vs).all() and not torch.equal(vs, v)
    assert torch.equal(vs, fresh_copy(m, dev)(x, t))  # both demoted deconv2 or neither did
    with torch.no_grad():
        gn.weight.mul_(1.0 / scale)
    assert 8.0 * float(gn.weight.abs().max()) + float(gn.bias.abs().max()) < 1024.0
    vb = checked_forward(m, x, t, dev, "back").clone()
    assert m._engine.handle(dev).value == h0
    assert torch.equal(vb, checked_forward(fresh_copy(m, dev), x, t, dev, "fresh, back"))
    with torch.no_grad():  # (gamma scale / scale is gamma to an ulp or two: its own float64 answer)
        v64b = R.forward64(R.params64(m, requires_grad=False), x.cpu(), t.cpu()).numpy()
    assert maxdiff(vb.cpu().numpy(), v64b) < TOL_EVAL
