"""Guidance diagnostics without a GPU: the float64 yardstick tests/diag_ref64.py (identities of the effective sample
size, the span of its graded inputs, the bounds of tests/test_gpu_diag.py held against the reference's own statements
in fp32), the GuidanceDiagnostics object (schedule, accessors, the reference's print), the argument checks of the
samplers' `diagnostics=` and the C ABI's declarations.

Reference arithmetic in fp32 (numpy, the statements of diag_ref64 with every array float32) against float64, worst
error / bound over the cases this file runs (all (t, centre), grades 0, 2, 6): printed by
test_fp32_reference_arithmetic_is_inside_the_bounds.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cond_ref64 as C
import diag_ref64 as D
import guidance_ref64 as G
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd.utils import diagnostics as UD
from ratio_guided_multimodal_fm_amd.utils.diagnostics import GuidanceDiagnostics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOPS = ("rgfm_sample_pair", "rgfm_sample_cond", "rgfm_sample_pair_grad", "rgfm_sample_cond_grad", "rgfm_fmnet_sample_pair")


# ------------------------------------------------------------------ the effective sample size
def test_ess_identities():
    for N in (1, 7, 64, 4096):
        ess, wmax, wmin = D.stats64(np.full((3, N), 1.0 / N))
        assert np.allclose(ess, N, rtol=1e-12) and np.allclose(wmax, 1.0 / N) and np.allclose(wmin, 1.0 / N)
        hot = np.zeros((2, N))
        hot[0, 0] = hot[1, N - 1] = 1.0
        ess, wmax, wmin = D.stats64(hot)
        assert (ess == 1).all() and (wmax == 1).all() and (wmin == (1.0 if N == 1 else 0.0)).all()
    ess, wmax, wmin = D.stats64(np.ones((5, 1)))
    assert (ess == 1).all() and (wmax == 1).all() and (wmin == 1).all()
    # the block itself at N = 1: the one weight is 1 up to the epsilons of the normalisation
    for si in range(len(G.STEPS)):
        rec = D.paired(6, si, 1.0, 0.0)[1]["rec"]
        assert np.allclose(rec[:, :3], 1.0, rtol=1e-9)


@pytest.mark.parametrize("ci", range(len(G.CASES)))
def test_graded_inputs_span_the_ess_range_paired(ci):
    N = G.CASES[ci][1]
    ess = np.concatenate([D.paired(ci, si, c, s)[1]["rec"][:, 0] for si in range(len(G.STEPS)) for c in G.CENTRES
                          for s in D.GRADES])
    print(f"paired {G.CASES[ci]}: ess64 {ess.min():.2f} .. {ess.max():.2f}")
    assert (ess >= 1 - 1e-9).all() and (ess <= N + 1e-9).all()
    assert ess.min() < 4 and ess.max() > N / 2


@pytest.mark.parametrize("ci", range(len(C.CASES)))
def test_graded_inputs_span_the_ess_range_one_sided(ci):
    N = C.CASES[ci][1]
    ess = np.concatenate([D.one_sided(ci, si, c, s)[1]["rec"][:, 0] for si in range(len(C.STEPS)) for c in C.CENTRES
                          for s in D.GRADES])
    print(f"one-sided {C.CASES[ci]}: ess64 {ess.min():.2f} .. {ess.max():.2f}")
    assert ess.min() < 4 and ess.max() > N / 2


def _diag32(inp, t):
    """diag_ref64.diag64's statements with every array float32 (numpy keeps fp32 through them): the reference's own
    arithmetic, as torch fp32 on the CPU would run it."""
    f = np.float32
    x, y, vx, vy, mx, my, r = (np.asarray(inp[k], f).reshape(inp[k].shape[0], -1) if inp[k].ndim > 1 else np.asarray(inp[k], f)
                               for k in ("x", "y", "vx", "vy", "mx", "my", "r"))
    t32, s2, c = f(t), f((1 - t + G.EPS) ** 2), f(1 - t + G.EPS)
    B, N = x.shape[0], mx.shape[0]
    l = np.empty((B, N), f)
    for b in range(B):
        l[b] = f(-0.5) * ((x[b] - t32 * mx) ** 2).sum(-1) / s2 + f(-0.5) * ((y[b] - t32 * my) ** 2).sum(-1) / s2
    p = np.exp(l - l.max(1, keepdims=True))
    pbar = p.mean(1, keepdims=True) + f(1e-10)
    zbar = (r[None] * p).mean(1, keepdims=True) + f(1e-10)
    w = (r[None] / zbar) * (p / pbar)
    w = w / (w.sum(1, keepdims=True) + f(1e-10))
    assert w.dtype == f
    gx = np.stack([(w[b][:, None] * ((mx - x[b]) / c)).sum(0) for b in range(B)])
    gy = np.stack([(w[b][:, None] * ((my - y[b]) / c)).sum(0) for b in range(B)])
    rec = np.zeros((B, 8), f)
    rec[:, 0] = w.sum(1) ** 2 / (w ** 2).sum(1)
    rec[:, 1], rec[:, 2], rec[:, 3] = w.max(1), w.min(1), zbar[:, 0]
    for k, a in ((4, vx), (5, vy), (6, gx), (7, gy)):
        rec[:, k] = np.sqrt((a ** 2).sum(1))
    return rec


@pytest.mark.parametrize("ci", [0, 1, 4, 6])
def test_fp32_reference_arithmetic_is_inside_the_bounds(ci):
    """The bounds of tests/test_gpu_diag.py are not vacuous and not out of reach: the reference's statements in fp32
    sit inside every one of them."""
    B, N, dx, dy = G.CASES[ci]
    for si, (t, _) in enumerate(G.STEPS):
        for centre in G.CENTRES:
            for s in D.GRADES:
                inp, ref = D.paired(ci, si, centre, s)
                bnd = D.bounds(inp, ref, N, (dx, dy), t, G.tol_w(t, centre))
                D.check(_diag32(inp, t), ref, bnd, f"fp32 reference {G.CASES[ci]} t={t} centre={centre} s={s}")


def test_the_check_can_fail():
    """A dropped MC sample, a wrong row sum and a norm over D - 4 elements are all outside the bounds."""
    ci, si, centre = 0, 1, 1.0
    B, N, dx, dy = G.CASES[ci]
    t = G.STEPS[si][0]
    inp, ref = D.paired(ci, si, centre, 2.0)
    bnd = D.bounds(inp, ref, N, (dx, dy), t, G.tol_w(t, centre))
    w = ref["w"].copy()
    w[:, -1] = 0  # the last sample of every row left out of the statistics
    bad = ref["rec"].copy()
    bad[:, 0], bad[:, 1], bad[:, 2] = D.stats64(w)
    with pytest.raises(AssertionError):
        D.check(bad, ref, bnd, "dropped sample", fields=("ess", "w_min"))
    bad = ref["rec"].copy()
    bad[:, 4] = np.sqrt((inp["vx"].astype(np.float64)[:, :-4] ** 2).sum(1))
    with pytest.raises(AssertionError):
        D.check(bad, ref, bnd, "short norm", fields=("v_norm_x",))
    bad = ref["rec"].copy()
    bad[:, 6] = np.sqrt((ref["gx"][:, :-4] ** 2).sum(1))
    with pytest.raises(AssertionError):
        D.check(bad, ref, bnd, "short g norm", fields=("g_norm_x",))


# ------------------------------------------------------------------ the object
def test_schedule_follows_the_loops_stage_formulas():
    assert UD.stage_times(4) == [0.0, 0.25, 0.5, 0.75]
    assert UD.stage_times(4, "midpoint") == [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875]
    assert UD.stage_times(7, "midpoint", 2, 4) == [2 * (1.0 / 7), 2.5 * (1.0 / 7), 3 * (1.0 / 7), 3.5 * (1.0 / 7)]
    assert UD.stage_times(1000, "euler", 0, 3) == [0.0, 1.0 * (1.0 / 1000), 2.0 * (1.0 / 1000)]
    d = GuidanceDiagnostics.from_records(np.zeros((3, 2, 8), np.float32), "mc_feng", "euler", 1000, 0, 3)
    assert d.guided.tolist() == [False, False, True]  # t = 0.001 exactly is unguided (`t > eps`)
    assert torch.allclose(d.sigma_t, 1 - d.t + 1e-3) and d.t.dtype == torch.float64
    d = GuidanceDiagnostics.from_records(np.zeros((8, 2, 8), np.float32), "mc_feng", "midpoint", 4)
    assert d.guided.tolist() == [False] + [True] * 7 and d.stage_of_step(2) == 4
    d = GuidanceDiagnostics.from_records(np.zeros((4, 2, 8), np.float32), "grad_log_ratio", "euler", 4)
    assert d.guided.all()
    d = GuidanceDiagnostics.from_records(np.zeros((4, 2, 8), np.float32), "none", "euler", 4)
    assert not d.guided.any()
    d = GuidanceDiagnostics.from_records(np.zeros((4, 2, 8), np.float32), "mc_feng", "euler", 4, has_mc=False)
    assert not d.guided.any()


def _filled():
    rec = np.random.default_rng(3).random((4, 5, 8)).astype(np.float32) + 0.5
    rec[0] = 0
    return rec, GuidanceDiagnostics.from_records(rec, "mc_feng", "euler", 4)


def test_accessors_and_summary():
    rec, d = _filled()
    for k, name in enumerate(UD.FIELDS):
        assert torch.equal(getattr(d, name)(), torch.from_numpy(rec[..., k]))
    s = d.summary(2)
    r = rec[2].astype(np.float64)
    assert s["t"] == 0.5 and s["sigma_t"] == 1 - 0.5 + 1e-3 and s["guided"] is True
    assert s["ess_mean"] == pytest.approx(r[:, 0].mean()) and s["ess_min"] == r[:, 0].min()
    assert s["w_max"] == r[:, 1].max() and s["w_min"] == r[:, 2].min() and s["z_bar"] == pytest.approx(r[:, 3].mean())
    for k in range(4, 8):
        assert s[UD.FIELDS[k]] == pytest.approx(r[:, k].mean())
    assert d.summary(0)["guided"] is False and d.summary(0)["ess_mean"] == 0


def test_reference_block_is_the_references_print():
    """The f-strings of the reference (src/utils/flow_utils.py:357-362), line by line."""
    rec, d = _filled()
    text = d.reference_block(1)
    pat = (r"\n\[MC Guidance Diagnostics at t=(\d\.\d{2})\]\n"
           r"  sigma_t=(\d+\.\d{4})\n"
           r"  \|\|v_x\|\|=(\d+\.\d{4}), \|\|v_y\|\|=(\d+\.\d{4})\n"
           r"  \|\|g_x\|\|=(\d+\.\d{4}), \|\|g_y\|\|=(\d+\.\d{4})\n"
           r"  weights: min=(\d+\.\d{6}), max=(\d+\.\d{6})\n"
           r"  Z_bar: (\d+\.\d{4})")
    m = re.fullmatch(pat, text)
    assert m, text
    r = rec[1].astype(np.float64)
    want = [0.25, 1 - 0.25 + 1e-3, r[:, 4].mean(), r[:, 5].mean(), r[:, 6].mean(), r[:, 7].mean(), r[:, 2].min(),
            r[:, 1].max(), r[:, 3].mean()]
    digits = [2, 4, 4, 4, 4, 4, 6, 6, 4]
    for got, w, nd in zip(m.groups(), want, digits):
        assert got == f"{w:.{nd}f}"
    assert d.reference_block(0) == ""  # step 0 is unguided: the reference prints from inside its guided branch
    with pytest.raises(IndexError):
        d.reference_block(4)
    g = GuidanceDiagnostics.from_records(rec, "grad_log_ratio", "euler", 4)
    with pytest.raises(ValueError, match="mc_feng"):
        g.reference_block(1)


def test_save_writes_the_arrays(tmp_path):
    rec, d = _filled()
    path = str(tmp_path / "diag.npz")
    d.save(path)
    z = np.load(path)
    assert (z["records"] == rec).all() and z["t"].tolist() == [0.0, 0.25, 0.5, 0.75]
    assert np.allclose(z["sigma_t"], 1 - z["t"] + 1e-3) and z["guided"].tolist() == [False, True, True, True]


def test_argument_checks():
    with pytest.raises(ValueError, match="solver"):
        UD.stage_times(4, "rk4")
    with pytest.raises(ValueError, match="num_steps"):
        UD.stage_times(0)
    with pytest.raises(ValueError, match="step range"):
        UD.stage_times(4, "euler", 3, 2)
    with pytest.raises(ValueError, match="guidance method"):
        GuidanceDiagnostics.from_records(np.zeros((4, 2, 8), np.float32), "mc", "euler", 4)
    with pytest.raises(ValueError, match="records of shape"):
        GuidanceDiagnostics.from_records(np.zeros((4, 2, 7), np.float32), "mc_feng", "euler", 4)
    with pytest.raises(ValueError, match="records of shape"):
        GuidanceDiagnostics.from_records(np.zeros((4, 2, 8), np.float32), "mc_feng", "midpoint", 4)
    with pytest.raises(RuntimeError, match="no records yet"):
        GuidanceDiagnostics().ess()
    with pytest.raises(RuntimeError, match="no records yet"):
        GuidanceDiagnostics().summary(0)
    assert UD.check(None) is None
    with pytest.raises(TypeError, match="GuidanceDiagnostics"):
        UD.check({})


def test_samplers_check_diagnostics_before_any_device_work():
    """A wrong `diagnostics=` is a TypeError and a CPU device the "no CPU path" error, with no HIP device in sight."""
    from helpers import make_module
    from ratio_guided_multimodal_fm_amd.sample_mnist_svhn import sample_bimodal_guided_mnist_svhn
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler, sample_bimodal_guided, sample_conditional
    fx, fy, rr = make_module("unet28"), make_module("unet28_y"), make_module("ratio28")
    with pytest.raises(TypeError, match="GuidanceDiagnostics"):
        sample_bimodal_guided(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 3, diagnostics=True)
    with pytest.raises(TypeError, match="GuidanceDiagnostics"):
        paired_sampler(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 3, (1, 28, 28), (1, 28, 28), diagnostics="yes")
    with pytest.raises(TypeError, match="GuidanceDiagnostics"):
        sample_conditional(fx, rr, torch.zeros(2, 1, 28, 28), "y", 4, diagnostics=1)
    d = GuidanceDiagnostics()
    with pytest.raises(RuntimeError, match="no CPU path"):
        sample_bimodal_guided(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 3, diagnostics=d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sample_bimodal_guided_mnist_svhn(make_module("mnist32"), make_module("svhn"), make_module("ratio_ms"), "mc_feng",
                                         1.0, 2, 4, "cpu", 3, diagnostics=d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sample_conditional(fx, rr, torch.zeros(2, 1, 28, 28), "y", 4, device="cpu", diagnostics=d)
    assert d.records is None


# ------------------------------------------------------------------ the C ABI
def test_header_bindings_and_library_list_the_diag_entry_points():
    header = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    assert re.search(r"#define\s+RGFM_ABI_VERSION\s+3\b", header)
    assert re.search(r"#define\s+RGFM_DIAG_FLOATS\s+8\b", header) and _lib.DIAG_FLOATS == 8 == UD.DIAG_FLOATS
    for k, name in enumerate(UD.FIELDS):
        assert re.search(r"#define\s+RGFM_DIAG_%s\s+%d\b" % (name.upper(), k), header), name
    handle = ctypes.CDLL(_lib.LIB_PATH)
    new = [f"{stem}_diag{tail}" for stem in LOOPS for tail in ("", "_workspace_bytes")]
    new += ["rgfm_guidance_diag", "rgfm_guidance_diag_cond", "rgfm_guidance_diag_workspace_bytes"]
    for name in new:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
    # each *_diag loop: its *_ode twin (the FlowMatchingModel pair: its Euler loop) with (diag_out, diag_records) in
    # front of ws; its workspace query: the twin's
    for stem in LOOPS:
        twin = stem if "fmnet" in stem else stem + "_ode"
        old, got = _lib.SIGNATURES[twin][1], _lib.SIGNATURES[stem + "_diag"][1]
        assert got == old[:-3] + [ctypes.c_void_p, ctypes.c_size_t] + old[-3:], stem
        assert _lib.SIGNATURES[twin + "_workspace_bytes"][1] == _lib.SIGNATURES[stem + "_diag_workspace_bytes"][1], stem
    # the blocks: the parity hooks without gamma and weights_out, diag_out in front of ws
    old, got = _lib.SIGNATURES["rgfm_guidance_apply"][1], _lib.SIGNATURES["rgfm_guidance_diag"][1]
    assert got == old[:12] + [ctypes.c_void_p] + old[-3:]
    old, got = _lib.SIGNATURES["rgfm_guidance_apply_cond"][1], _lib.SIGNATURES["rgfm_guidance_diag_cond"][1]
    assert got == old[:8] + [ctypes.c_void_p] + old[-3:]
    from ratio_guided_multimodal_fm_amd import _engine
    # the Python layer's export table: every guided loop has a row, which names the twin, its query and their *_diag pair
    rows = {row.fn: row for row in _engine._GUIDED_LOOPS}
    assert len(rows) == len(LOOPS)
    for stem in LOOPS:
        twin = stem if "fmnet" in stem else stem + "_ode"
        assert rows[twin][:4] == (twin, twin + "_workspace_bytes", stem + "_diag", stem + "_diag_workspace_bytes"), stem


def test_block_level_argument_errors_need_no_device():
    """The workspace query's checks (descriptor-only, like rgfm_guidance_workspace_bytes)."""
    L = _lib.lib()
    n = ctypes.c_size_t()
    assert L.rgfm_guidance_diag_workspace_bytes(3, 7, 784, 784, ctypes.byref(n)) == 0
    base = ctypes.c_size_t()
    assert L.rgfm_guidance_workspace_bytes(3, 7, ctypes.byref(base)) == 0
    assert n.value >= base.value + 4 * 3 * (784 + 784)  # the block's workspace + the two scratch velocities
    for bad in ((0, 7, 784, 784), (3, 0, 784, 784), (3, 7, 0, 784), (3, 7, 6, 4), (3, 7, 8, -4)):
        assert L.rgfm_guidance_diag_workspace_bytes(*bad, ctypes.byref(n)) == -1, bad
    assert L.rgfm_guidance_diag_workspace_bytes(3, 7, 784, 0, ctypes.byref(n)) == 0  # the one-sided block


# ------------------------------------------------------------------ the evaluation sweeps
def test_sweep_rows_gain_the_three_keys_only_with_diagnostics():
    """run_sweep(diagnostics=True) hands every guided call a fresh GuidanceDiagnostics and adds ess_mean, ess_min and
    w_max at step int(0.3 * num_steps) to that row; 'none' rows and sweeps without the flag keep exactly their keys."""
    from helpers import golden, make_module
    from ratio_guided_multimodal_fm_amd import evaluate, evaluate_mnist_svhn
    g = golden("sampler_pair_ms")
    xs = torch.from_numpy(np.concatenate([g[f"c{i}_x"] for i in range(6)]))
    ys = torch.from_numpy(np.concatenate([g[f"c{i}_y"] for i in range(6)]))
    steps, seen = 20, []

    def fake_sampler(fm_m, fm_s, ratio, method, strength, n, num_steps, device, mc, diagnostics=None):
        seen.append((method, diagnostics))
        if diagnostics is not None:
            rec = np.zeros((num_steps, n, 8), np.float32)
            rec[1:, :, 0] = np.arange(1, n + 1)          # ess per row: 1 .. n
            rec[1:, :, 1] = 0.5 + 0.01 * np.arange(n)    # w_max per row
            diagnostics._schedule(method, "euler", num_steps)
            diagnostics.records = torch.from_numpy(rec)
        return xs[:n], ys[:n]

    cm, cs = make_module("clf_mnist"), make_module("clf_svhn")
    base = {"method", "guidance_strength", "experiment", "coherence_acc", "num_samples"}
    res = evaluate_mnist_svhn.run_sweep(None, None, lambda: object(), cm, cs, ["none", "mc_feng"], [0.0, 0.5], 8, steps,
                                        "cpu", 16, sampler=fake_sampler, diagnostics=True)
    assert [m for m, _ in seen] == ["none", "mc_feng", "mc_feng"]
    assert seen[0][1] is None and isinstance(seen[1][1], GuidanceDiagnostics) and seen[1][1] is not seen[2][1]
    assert set(res[0]) == base and all(set(r) == base | {"ess_mean", "ess_min", "w_max"} for r in res[1:])
    assert res[1]["ess_mean"] == 4.5 and res[1]["ess_min"] == 1.0 and res[1]["w_max"] == pytest.approx(0.57)
    seen.clear()

    def plain_sampler(fm_m, fm_s, ratio, method, strength, n, num_steps, device, mc):  # (no diagnostics keyword at all)
        return xs[:n], ys[:n]

    res = evaluate_mnist_svhn.run_sweep(None, None, lambda: object(), cm, cs, ["none", "mc_feng"], [0.0, 0.5], 8, steps,
                                        "cpu", 16, sampler=plain_sampler)
    assert all(set(r) == base for r in res)
    # the 28x28 harness: the same rule
    g28 = golden("sampler_pair28")
    x28 = torch.from_numpy(np.concatenate([g28[f"c{i}_x"] for i in range(3)]))
    y28 = torch.from_numpy(np.concatenate([g28[f"c{i}_y"] for i in range(3)]))
    n28 = min(8, len(x28))

    def fake28(fx, fy, ratio, method, strength, n, num_steps, device, mc, diagnostics=None):
        if diagnostics is not None:
            diagnostics._schedule(method, "euler", num_steps)
            diagnostics.records = torch.ones(num_steps, n, 8)
        return x28[:n], y28[:n]

    res = evaluate.run_sweep(None, None, lambda: object(), make_module("clf_mnist28"), ["none", "mc_feng"], [0.0, 1.0], n28,
                             steps, "cpu", 16, "none", sampler=fake28, diagnostics=True)
    base28 = {"method", "guidance_strength", "transform_type", "coherence_acc", "num_samples"}
    assert set(res[0]) == base28 and set(res[1]) == base28 | {"ess_mean", "ess_min", "w_max"} and res[1]["ess_mean"] == 1.0
