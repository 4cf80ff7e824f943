"""The MC guidance kernels (csrc/guidance.hip: guid_logp_kernel, guid_weights_kernel, guid_apply_mfma_kernel) through
the parity hook against float64, on inputs where EVERY MC sample carries a visible share of every row.

The yardstick is tests/guidance_ref64.py (guidance64: numpy float64 of reference src/sample_mnist_svhn.py:124-171;
spread_case: importance weights spread over the whole MC set, effective sample size >= N / 2); that the checks below
can fail -- the tolerances against the fp32 oracle's own deviation, the drop-one sensitivity -- is asserted on the CPU
by tests/test_guidance_ref64_cpu.py.

Cases (B, N, dx, dy), KH = ceil(N / 8) samples per (wave, lane half) of the apply kernel, U = 16 per register group:

    (33, 70, 784, 784)    one-row tail in the second 32-row tile; 6-sample tail in the second 64-sample tile; KH = 9,
                          not W4; 784 = 512 + 272: a slice tail of four chunks + 16; 16-column tail of the apply tile
    (65, 32, 64, 192)     smallest W4 (KH = 4); three row tiles; dx exactly one chunk
    (40, 288, 132, 128)   W4, KH = 36 = 2U + 4: the third group load is partial; dx one column block + 4; dy one block
    (37, 544, 68, 4)      W4, KH = 68 > 4U: two full loop trips + a tail; dx one chunk + 4; dy = 4
    (5, 257, 520, 48)     not W4, KH = 33
    (2, 33, 2052, 2052)   5 + 5 > 8 slices: slice_len 1024 with a last slice of 4 elements; KH = 5, the last lane half
                          starts past N
    (1, 1, 4, 4)          everything minimal
    (3, 4096, 8, 4)       largest accepted N (the LDS limit of guid_weights_kernel); 64 sample tiles; KH = 512

each at (t, gamma) = (0.05, 0.5), (0.5, 1.0), (0.9, 2.0), (0.99, 5.0) and centre 1 (sum w m and x sum w cancel as in
real sampling) and 0 (|m|max ~ |m - x|: one sample's term is 18x .. 600x the velocity bound at N <= 544).

Tolerances.  Weights: relative error per element <= 4x the fp32 oracle's own deviation from float64 at that t and
centre (guidance_ref64.ORACLE_DW; 4x for another expf and wave-order sums).  Velocity: max |dv| <=
gamma (K sqrt(N) 2^-23 |m|max / c + tol_w max |g64|) + 2^-22 max |v64| with K = 2.1, the constant of
test_guidance_late_time_concentrated_weights.  At N = 4096 one sample is 0.7x .. 0.85x that bound: the weights check
carries the weights stage there and the velocity check is bound-only.

Measured on an MI355X (max over the eight cases; dw relative, max |dv|, and the worst dv / bound):

    t       centre = 1: dw / tol_w       dv        dv / bound     centre = 0: dw / tol_w       dv        dv / bound
    0.05    3.8e-7 / 4.8e-6              5.0e-7    0.03           4.0e-7 / 4.4e-6              2.7e-7    0.03
    0.5     3.4e-7 / 4.8e-6              1.4e-6    0.04           3.2e-7 / 1.0e-5              4.1e-8    0.01
    0.9     1.7e-6 / 1.1e-5              1.4e-5    0.07           3.7e-7 / 8.0e-6              2.6e-7    0.07
    0.99    1.65e-5 / 6.8e-5             4.9e-4    0.07           3.4e-7 / 6.4e-6              9.6e-7    0.09

(|sum w - 1| <= 1.4e-7.  The kernels' weights are closer to float64 than the oracle's wherever summation order
matters -- wave-order against sequential fp32 sums; at t = 0.99, centre = 1 both carry the same fp32 rounding of
mu = t m.)  With the last sample of every (wave, lane half) run left out of guid_apply_mfma_kernel's GEMM -- a
throwaway mutation, `s < KH - 1` -- the velocity check fails in all 64 configurations, by 11x the bound at the least.
"""
import ctypes

import numpy as np
import pytest
import torch

import guidance_ref64 as R
from ratio_guided_multimodal_fm_amd import _engine, _lib

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
PAD = 256  # floats kept on each side of an output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _to(dev, inp, rows=None):
    """The inputs on the device (fresh tensors; vx / vy are overwritten by the call); rows: a sub-batch."""
    d = {k: torch.tensor(v, device=dev) for k, v in inp.items()}
    if rows is not None:
        for k in ("x", "y", "vx", "vy"):
            d[k] = d[k][rows].clone()
    return d


def _apply(d, t, gamma, want_weights=True):
    w = _engine.guidance_apply(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"], d["r"], t, gamma, want_weights)
    return w, d["vx"], d["vy"]


def _raw(d, t, gamma, w, ws, ws_bytes):
    """rgfm_guidance_apply with the caller's own weights buffer and workspace."""
    B, N = d["x"].shape[0], d["mx"].shape[0]
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    with torch.cuda.device(d["x"].device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().rgfm_guidance_apply(p(d["x"]), p(d["y"]), p(d["vx"]), p(d["vy"]), p(d["mx"]), p(d["my"]),
                                                  p(d["r"]), B, N, d["x"].shape[1], d["y"].shape[1], float(t),
                                                  float(gamma), p(w), p(ws), ws_bytes, stream))


def _workspace_bytes(B, N):
    nb = ctypes.c_size_t()
    _lib.check(_lib.lib().rgfm_guidance_workspace_bytes(B, N, ctypes.byref(nb)))
    return nb.value


def _rel_dw(w, w64):
    keep = w64 > 0
    return float((np.abs(w - w64)[keep] / w64[keep]).max())


@pytest.mark.parametrize("centre", R.CENTRES)
@pytest.mark.parametrize("si", range(len(R.STEPS)))
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_weights_and_velocity_vs_float64(dev, ci, si, centre):
    B, N, dx, dy = R.CASES[ci]
    t, gamma = R.STEPS[si]
    inp, ref = R.case(ci, si, centre)
    w, vx, vy = (a.cpu().numpy().astype(np.float64) for a in _apply(_to(dev, inp), t, gamma))
    tw = R.tol_w(t, centre)
    bound = R.velocity_bound(inp, ref, N, t, gamma, tw)
    dw = _rel_dw(w, ref["w"])
    dv = max(float(np.abs(vx - ref["vx"]).max()), float(np.abs(vy - ref["vy"]).max()))
    dsum = float(np.abs(w.sum(1) - 1).max())
    print(f"guidance64 {R.CASES[ci]} t={t} centre={centre}: dw {dw:.2e} / tol_w {tw:.1e} = {dw / tw:.2f}   "
          f"dv {dv:.2e} / bound {bound:.2e} = {dv / bound:.2f}   |sum w - 1| {dsum:.1e}")
    assert np.isfinite(w).all() and np.isfinite(vx).all() and np.isfinite(vy).all()
    assert dw <= tw, (dw, tw)
    assert dsum < 1e-5, dsum
    assert dv <= bound, (dv, bound)


@pytest.mark.parametrize("ci", [0, 2])
def test_rows_do_not_depend_on_the_batch(dev, ci):
    """guidance.hip: "a row's result depends on its own weights and the MC set only, in an order fixed by N:
    independent of the batch it is in" -- bitwise, for the first row, the last row and a batch of the last seven."""
    B = R.CASES[ci][0]
    for si, (t, gamma) in enumerate(R.STEPS):
        inp = R.case(ci, si, 0.0)[0]
        full = _apply(_to(dev, inp), t, gamma)
        for rows in (slice(0, 1), slice(B - 1, B), slice(B - 7, B)):
            part = _apply(_to(dev, inp, rows), t, gamma)
            for name, f, p in zip(("weights", "vx", "vy"), full, part):
                assert torch.equal(f[rows], p), (name, t, rows)


@pytest.mark.parametrize("ci", [0, 5])
def test_scratch_is_written_before_it_is_read(dev, ci):
    """Whatever the caller's workspace holds -- NaN or zeros -- and whether it is exactly
    rgfm_guidance_workspace_bytes or 4 KB more, the outputs are the same bits; one byte short is an error."""
    B, N, dx, dy = R.CASES[ci]
    si = 2
    t, gamma = R.STEPS[si]
    inp = R.case(ci, si, 1.0)[0]
    need = _workspace_bytes(B, N)
    assert need % 4 == 0
    outs = []
    for fill in (float("nan"), 0.0):
        for extra in (0, 4096):
            d = _to(dev, inp)
            w = torch.full((B, N), SENTINEL, device=dev)
            ws = torch.full(((need + extra) // 4,), fill, device=dev)
            _raw(d, t, gamma, w, ws, need + extra)
            outs.append((w, d["vx"], d["vy"]))
    for o in outs:
        for a, b in zip(outs[0], o):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    d = _to(dev, inp)
    w = torch.full((B, N), SENTINEL, device=dev)
    ws = torch.zeros(need // 4, device=dev)
    with pytest.raises(_lib.RgfmError):
        _raw(d, t, gamma, w, ws, need - 1)
    torch.cuda.synchronize()
    assert bool((w == SENTINEL).all()) and torch.equal(d["vx"], torch.tensor(inp["vx"], device=dev))


@pytest.mark.parametrize("ci", [0, 4, 6])
def test_outputs_stay_inside_their_buffers(dev, ci):
    """vx, vy and the weights as views into the middle of larger buffers: 256 floats on each side keep their
    sentinel, the inputs keep their bits, and the results are those of a plain call."""
    B, N, dx, dy = R.CASES[ci]
    si = 1
    t, gamma = R.STEPS[si]
    inp = R.case(ci, si, 1.0)[0]
    plain = _apply(_to(dev, inp), t, gamma)
    d = _to(dev, inp)
    kept = {k: d[k].clone() for k in ("x", "y", "mx", "my", "r")}
    big = {}
    for name, n in (("vx", B * dx), ("vy", B * dy), ("w", B * N)):
        big[name] = torch.full((PAD + n + PAD,), SENTINEL, device=dev)
    view = lambda name, shape: big[name][PAD:-PAD].view(shape)
    view("vx", (B, dx)).copy_(d["vx"])
    view("vy", (B, dy)).copy_(d["vy"])
    d["vx"], d["vy"] = view("vx", (B, dx)), view("vy", (B, dy))
    need = _workspace_bytes(B, N)
    _raw(d, t, gamma, view("w", (B, N)), torch.empty(need // 4, device=dev), need)
    torch.cuda.synchronize()
    for name in big:
        assert bool((big[name][:PAD] == SENTINEL).all()) and bool((big[name][-PAD:] == SENTINEL).all()), name
    for k, v in kept.items():
        assert torch.equal(d[k], v), k
    for p, name, shape in zip(plain, ("w", "vx", "vy"), ((B, N), (B, dx), (B, dy))):
        assert torch.equal(p, view(name, shape)), name


def test_ratio_and_underflow_edges(dev):
    """mc_ratios[k] = 0 gives a weight of exactly 0, mc_ratios[k] = 1e6 a row dominated by k: the other weights match
    float64 as before.  A row moved by +3 per element (l ~ -6e7, float64 top-two gap >= 50): every exp(l - max) but
    one underflows or nearly so; the row stays finite, sums to 1 and is the float64 one-hot row."""
    N = R.CASES[0][1]
    for si, (t, gamma) in enumerate(R.STEPS):
        for k, value in ((67, 0.0), (3, 1e6)):
            inp, ref = R.ratio_edge(si, k, value)
            w, vx, vy = (a.cpu().numpy().astype(np.float64) for a in _apply(_to(dev, inp), t, gamma))
            tw = R.tol_w(t, 0.0)
            if value == 0.0:
                assert (w[:, k] == 0).all()
            assert _rel_dw(w, ref["w"]) <= tw, (t, value, _rel_dw(w, ref["w"]))
            assert np.abs(w.sum(1) - 1).max() < 1e-5
            bound = R.velocity_bound(inp, ref, N, t, gamma, tw)
            assert max(np.abs(vx - ref["vx"]).max(), np.abs(vy - ref["vy"]).max()) <= bound
    inp, ref, row, gap = R.shifted_row()
    assert gap >= 50, gap  # the precondition: float64 itself is one-hot to 2e-22
    t, gamma = R.STEPS[3]
    w, vx, vy = (a.cpu().numpy().astype(np.float64) for a in _apply(_to(dev, inp), t, gamma))
    assert np.isfinite(w).all() and np.isfinite(vx).all() and np.isfinite(vy).all()
    assert abs(w[row].sum() - 1) < 1e-6
    assert np.abs(w[row] - ref["w"][row]).max() < 1e-6
    others = np.arange(w.shape[0]) != row
    assert _rel_dw(w[others], ref["w"][others]) <= R.tol_w(t, 0.0)


def test_argument_errors(dev):
    """A flattened image size that is no multiple of 4 and an MC set above 4096 are errors, and the outputs are not
    touched."""
    g = torch.Generator().manual_seed(5)
    for B, N, dx, dy in ((2, 3, 6, 4), (2, 4097, 4, 4)):
        d = {"x": torch.randn(B, dx, generator=g), "y": torch.randn(B, dy, generator=g),
             "mx": torch.randn(N, dx, generator=g), "my": torch.randn(N, dy, generator=g),
             "r": torch.ones(N)}
        d = {k: v.to(dev) for k, v in d.items()}
        d["vx"], d["vy"] = torch.full((B, dx), SENTINEL, device=dev), torch.full((B, dy), SENTINEL, device=dev)
        w = torch.full((B, N), SENTINEL, device=dev)
        need = _workspace_bytes(B, N)
        ws = torch.zeros(need // 4, device=dev)
        with pytest.raises(_lib.RgfmError):
            _raw(d, 0.5, 1.0, w, ws, need)
        with pytest.raises(_lib.RgfmError):
            _apply(d, 0.5, 1.0)
        torch.cuda.synchronize()
        for a in (d["vx"], d["vy"], w):
            assert bool((a == SENTINEL).all())
