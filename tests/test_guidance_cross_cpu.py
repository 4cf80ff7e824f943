"""Cross pairing of the MC set without a GPU: the float64 yardstick tests/guidance_cross_ref64.py against the paired
yardstick on the materialised list, its conditioning, the fp32 restatement behind the GPU test's weights tolerance,
closed forms, the variance toy, the C ABI's declarations and argument checks, and the Python / CLI argument checks.

cross32 against cross64, max over guidance_cross_ref64.CASES of the relative deviation of the 2N marginal weights
(printed by test_cross32_table_reproduces; CROSS32_DW holds it rounded up to two digits; the N = 1024 case sets it):

    t       centre = 1   centre = 0
    0.05    2.39e-6      2.55e-6
    0.5     2.37e-6      2.29e-6
    0.9     3.10e-6      2.04e-6
    0.99    9.58e-6      2.00e-6

Conditioning of the float64 answer over all cases: every marginal weight >= 0.29 / N, joint ESS >= 0.70 N^2.

The toy (test_cross_estimator_has_at_most_half_the_paired_error): 4 clusters per modality in 4 dimensions (centres
2 e_k, spread 0.3), r = 4 on matching clusters and 1e-3 elsewhere, N = 32, 100 seeds, 8 query points on matched paths,
error of the guided velocity g against a paired estimate with N = 200 000: paired MSE / cross MSE = 4.7 at t = 0.3,
9.2 at t = 0.6, 5.0 at t = 0.9.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import guidance_cross_ref64 as X
import guidance_ref64 as G
from ratio_guided_multimodal_fm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(ci, si, centre) for ci in range(len(X.CASES)) for si in range(len(X.STEPS)) for centre in X.CENTRES]
NEW = ("rgfm_guidance_cross_workspace_bytes", "rgfm_guidance_apply_cross", "rgfm_guidance_diag_cross",
       "rgfm_sample_pair_cross_workspace_bytes", "rgfm_sample_pair_cross")


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("ci,si,centre", [c for c in CONFIGS if X.CASES[c[0]][1] <= 64])
def test_cross64_is_guidance64_on_the_materialised_list(ci, si, centre):
    B, N, dx, dy = X.CASES[ci]
    t, gamma = X.STEPS[si]
    inp, ref = X.case(ci, si, centre)
    m = X.materialised(inp)
    assert m["mx"].shape == (N * N, dx) and m["my"].shape == (N * N, dy) and m["r"].shape == (N * N,)
    vx, vy, w, _ = G.guidance64(m["x"], m["y"], m["vx"], m["vy"], m["mx"], m["my"], m["r"], t, gamma)
    w = w.reshape(B, N, N)
    ess = w.sum((1, 2)) ** 2 / (w ** 2).sum((1, 2))
    errs = {"vx": _rel(ref["vx"], vx), "vy": _rel(ref["vy"], vy),
            "wx": float((np.abs(ref["wx"] - w.sum(2)) / w.sum(2)).max()), "wy": float((np.abs(ref["wy"] - w.sum(1)) / w.sum(1)).max()),
            "ess": float((np.abs(ref["ess"] - ess) / ess).max())}
    print(f"{X.CASES[ci]} t={t} centre={centre}: " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12, errs


def test_a_transposed_ratio_matrix_is_far_outside_the_tolerance():
    """R is asymmetric: reading it transposed moves the marginal weights by far more than tol_w_cross."""
    for ci in (1, 2, 5):
        for si, (t, gamma) in enumerate(X.STEPS):
            inp, ref = X.case(ci, si, 0.0)
            wx = X.cross64(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], inp["R"].T, t, gamma)[2]
            assert float((np.abs(wx - ref["wx"]) / ref["wx"]).max()) > 1e3 * X.tol_w_cross(t, 0.0)


@pytest.mark.parametrize("ci,si,centre", CONFIGS)
def test_every_marginal_weight_counts(ci, si, centre):
    N = X.CASES[ci][1]
    ref = X.case(ci, si, centre)[1]
    wmin = min(ref["wx"].min(), ref["wy"].min()) * N
    print(f"{X.CASES[ci]} t={X.STEPS[si][0]} centre={centre}: min w N {wmin:.2f}  joint ESS / N^2 {ref['ess'].min() / N ** 2:.2f}")
    assert wmin >= 0.25, wmin
    assert np.abs(ref["wx"].sum(1) - 1).max() < 1e-9 and np.abs(ref["wy"].sum(1) - 1).max() < 1e-9
    assert (ref["ess"] >= 1 - 1e-9).all() and (ref["ess"] <= N * N * (1 + 1e-9)).all()


_table = {}


@pytest.mark.parametrize("ci,si,centre", CONFIGS)
def test_cross32_is_inside_the_recorded_figure_and_the_velocity_bound(ci, si, centre):
    N = X.CASES[ci][1]
    t, gamma = X.STEPS[si]
    inp, ref = X.case(ci, si, centre)
    vx, vy, wx, wy, ess, z = X.cross32(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], inp["R"], t, gamma)
    dw = max(float((np.abs(wx - ref["wx"]) / ref["wx"]).max()), float((np.abs(wy - ref["wy"]) / ref["wy"]).max()))
    _table[(ci, t, centre)] = dw
    dv = max(float(np.abs(vx - ref["vx"]).max()), float(np.abs(vy - ref["vy"]).max()))
    bound = X.velocity_bound(inp, ref, N, t, gamma, X.tol_w_cross(t, centre))
    print(f"{X.CASES[ci]} t={t} centre={centre}: cross32 dw {dw:.2e} (recorded {X.CROSS32_DW[(t, centre)]:.1e})  dv {dv:.2e}  bound {bound:.2e}")
    assert dw <= X.CROSS32_DW[(t, centre)], (dw, X.CROSS32_DW[(t, centre)])
    assert dv <= bound, (dv, bound)
    assert float((np.abs(ess - ref["ess"]) / ref["ess"]).max()) <= 4 * X.tol_w_cross(t, centre) + 2 * N * 2.0 ** -24
    assert float((np.abs(z - ref["z_bar"]) / ref["z_bar"]).max()) <= X.tol_w_cross(t, centre)


def test_cross32_table_reproduces():
    """CROSS32_DW is the measured maximum rounded UP to two digits: not below it, and not more than one step above."""
    if len(_table) < len(CONFIGS):  # (run alone: fill the table)
        for ci, si, centre in CONFIGS:
            test_cross32_is_inside_the_recorded_figure_and_the_velocity_bound(ci, si, centre)
    for (t, centre), rec in X.CROSS32_DW.items():
        worst = max(v for (ci, tt, c), v in _table.items() if tt == t and c == centre)
        step = 10.0 ** (np.floor(np.log10(worst)) - 1)
        print(f"t={t} centre={centre}: measured {worst:.3e}, recorded {rec:.1e}")
        assert worst <= rec <= worst + 1.001 * step, (t, centre, worst, rec)


# ------------------------------------------------------------------ closed forms
def _ab(inp, t):
    x, y, mx, my = (np.asarray(inp[k], np.float64) for k in ("x", "y", "mx", "my"))
    s2 = (1 - t + X.EPS) ** 2
    lx = np.stack([-0.5 * ((x[k] - t * mx) ** 2).sum(-1) / s2 for k in range(x.shape[0])])
    ly = np.stack([-0.5 * ((y[k] - t * my) ** 2).sum(-1) / s2 for k in range(y.shape[0])])
    return np.exp(lx - lx.max(1, keepdims=True)), np.exp(ly - ly.max(1, keepdims=True))


@pytest.mark.parametrize("ci", [1, 2, 5])
def test_closed_forms(ci):
    N = X.CASES[ci][1]
    for si, (t, gamma) in enumerate(X.STEPS):
        inp = X.case(ci, si, 0.0)[0]
        a, b = _ab(inp, t)
        run = lambda R: X.cross64(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], R, t, gamma)
        # R = 1: the two modalities decouple, each marginal is its own softmax
        _, _, wx, wy, ess, z = run(np.ones((N, N)))
        assert np.allclose(wx, a / a.sum(1, keepdims=True), rtol=1e-9, atol=0)
        assert np.allclose(wy, b / b.sum(1, keepdims=True), rtol=1e-9, atol=0)
        assert np.allclose(ess, (a.sum(1) ** 2 / (a ** 2).sum(1)) * (b.sum(1) ** 2 / (b ** 2).sum(1)), rtol=1e-9)
        # R_ij = f_i: y is untouched, x is reweighted by f
        f = np.exp(0.7 * np.random.default_rng(ci).standard_normal(N))
        _, _, wx, wy, _, _ = run(np.repeat(f[:, None], N, 1))
        assert np.allclose(wy, b / b.sum(1, keepdims=True), rtol=1e-9, atol=0)
        assert np.allclose(wx, a * f / (a * f).sum(1, keepdims=True), rtol=1e-9, atol=0)
        # a constant factor cancels
        assert np.allclose(run(2.5 * inp["R"].astype(np.float64))[2], run(inp["R"])[2], rtol=1e-9, atol=0)


def test_edge_inputs_of_the_gpu_test():
    """The R edges and the underflowing row the GPU test runs: float64 is what the test's docstring says it is."""
    for si in range(len(X.STEPS)):
        ref = X.ratio_edge(si, "zero")[1]
        assert (ref["wx"][:, 5] == 0).all() and (ref["wy"][:, 9] == 0).all()
        assert (np.delete(ref["wx"], 5, 1) > 0).all() and (np.delete(ref["wy"], 9, 1) > 0).all()
        big = X.ratio_edge(si, "big")[1]
        assert big["wx"][:, 3].min() > 10 * X.case(X.EDGE_CASE, si, 0.0)[1]["wx"][:, 3].max()
    inp, ref, row, gap = X.shifted_row()
    assert gap >= 104 and ref["wx"][row].max() >= 1 - 1e-12 and np.isfinite(ref["vx"]).all()
    o = X.cross32(inp["x"], inp["y"], inp["vx"], inp["vy"], inp["mx"], inp["my"], inp["R"], *X.STEPS[3])
    assert all(np.isfinite(a).all() for a in o)
    assert np.abs(o[2][row] - ref["wx"][row]).max() < 1e-6 and np.abs(o[3][row] - ref["wy"][row]).max() < 1e-6


# ------------------------------------------------------------------ why: the variance toy
def test_cross_estimator_has_at_most_half_the_paired_error():
    K, DIM, STD, B, N, SEEDS, NBIG = 4, 4, 0.3, 8, 32, 100, 200000
    centres = 2.0 * np.eye(K, DIM)

    def draw(rng, n):
        k = rng.integers(0, K, n)
        return centres[k] + STD * rng.standard_normal((n, DIM)), k
    rng = np.random.default_rng(1)
    x1, kx = draw(rng, B)
    y1 = centres[kx] + STD * rng.standard_normal((B, DIM))  # the query points lie on matched paths
    x0, y0 = rng.standard_normal((B, DIM)), rng.standard_normal((B, DIM))
    bx, bkx = draw(rng, NBIG)
    by, bky = draw(rng, NBIG)
    br = np.where(bkx == bky, 4.0, 1e-3)
    zero = np.zeros((B, DIM))
    for t in (0.3, 0.6, 0.9):
        x, y = (1 - t) * x0 + t * x1, (1 - t) * y0 + t * y1
        gx, gy = G.guidance64(x, y, zero, zero, bx, by, br, t, 1.0)[:2]
        ep = ec = 0.0
        for s in range(SEEDS):
            r2 = np.random.default_rng(100 + s)
            mx, kmx = draw(r2, N)
            my, kmy = draw(r2, N)
            R = np.where(kmx[:, None] == kmy[None, :], 4.0, 1e-3)
            px, py = G.guidance64(x, y, zero, zero, mx, my, np.diag(R).copy(), t, 1.0)[:2]
            cx, cy = X.cross64(x, y, zero, zero, mx, my, R, t, 1.0)[:2]
            ep += ((px - gx) ** 2).sum() + ((py - gy) ** 2).sum()
            ec += ((cx - gx) ** 2).sum() + ((cy - gy) ** 2).sum()
        print(f"toy t={t}: paired MSE / cross MSE = {ep / ec:.2f}")
        assert ec <= 0.5 * ep, (t, ep, ec)


# ------------------------------------------------------------------ the C ABI
def test_header_bindings_and_library_list_the_cross_entry_points():
    header = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    assert re.search(r"#define\s+RGFM_ABI_VERSION\s+3\b", header) and _lib.ABI_VERSION == 3
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
    S = _lib.SIGNATURES
    # the block: rgfm_guidance_apply with a second weights output; its diagnostics twin: rgfm_guidance_diag's arguments
    old = S["rgfm_guidance_apply"][1]
    assert S["rgfm_guidance_apply_cross"][1] == old[:14] + [ctypes.c_void_p] + old[14:]
    assert S["rgfm_guidance_diag_cross"][1] == S["rgfm_guidance_diag"][1]
    assert S["rgfm_guidance_cross_workspace_bytes"][1] == S["rgfm_guidance_diag_workspace_bytes"][1]
    # the loop: rgfm_sample_pair_diag's arguments, the matrix in the vector's place
    assert S["rgfm_sample_pair_cross"][1] == S["rgfm_sample_pair_diag"][1]
    assert S["rgfm_sample_pair_cross_workspace_bytes"][1] == S["rgfm_sample_pair_diag_workspace_bytes"][1]


def test_block_level_argument_errors_need_no_device():
    L = _lib.lib()
    n, base = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.rgfm_guidance_cross_workspace_bytes(3, 7, 784, 3072, ctypes.byref(n)) == 0
    assert L.rgfm_guidance_workspace_bytes(3, 7, ctypes.byref(base)) == 0
    # the paired block's workspace + six more [B][N] rows + the two scratch velocities
    assert n.value >= base.value + 4 * 6 * 3 * 7 + 4 * 3 * (784 + 3072) and n.value % 256 == 0
    assert L.rgfm_guidance_cross_workspace_bytes(1, 1024, 4, 4, ctypes.byref(n)) == 0
    for bad in ((0, 7, 784, 784), (3, 0, 784, 784), (3, 1025, 784, 784), (3, 7, 0, 784), (3, 7, 784, 0), (3, 7, 6, 4), (3, 7, 8, -4)):
        assert L.rgfm_guidance_cross_workspace_bytes(*bad, ctypes.byref(n)) == -1, bad
    assert L.rgfm_guidance_cross_workspace_bytes(3, 7, 784, 784, None) == -1
    assert b"n_mc" in (L.rgfm_guidance_cross_workspace_bytes(3, 1025, 4, 4, ctypes.byref(n)), L.rgfm_last_error())[1]
    # null pointers and a null handle come back before any device call
    null = ctypes.c_void_p(0)
    assert L.rgfm_guidance_apply_cross(*[null] * 7, 3, 7, 4, 4, 0.5, 1.0, null, null, null, 0, null) == -1
    assert L.rgfm_guidance_diag_cross(*[null] * 7, 3, 7, 4, 4, 0.5, null, null, 0, null) == -1
    assert L.rgfm_sample_pair_cross_workspace_bytes(null, null, 3, 7, 0, ctypes.byref(n)) == -1
    assert L.rgfm_sample_pair_cross(null, null, null, null, null, null, null, 7, 3, 4, 0.5, 0, 4, 0, null, 0, null, 0, null) == -1


# ------------------------------------------------------------------ the Python surface
def test_mc_pairing_argument_checks():
    """Unknown pairings, 'cross' with another guidance method, FlowMatchingModel nets, too large an MC set and sharded
    launches are refused before any device work (there is no HIP device in sight here); the default reaches the
    device check like before."""
    from helpers import make_module
    from ratio_guided_multimodal_fm_amd.distributed import make_sharded_sampler, sharded_paired_sampler
    from ratio_guided_multimodal_fm_amd.sample_mnist_svhn import sample_bimodal_guided_mnist_svhn
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import check_pairing, paired_sampler, sample_bimodal_guided
    fx, fy, rr = make_module("unet28"), make_module("unet28_y"), make_module("ratio28")
    assert check_pairing("paired") == "paired" and check_pairing("cross") == "cross" and check_pairing("paired", "none") == "paired"
    for bad in ("all", "", None, 1):
        with pytest.raises(ValueError, match="mc_pairing"):
            sample_bimodal_guided(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 3, mc_pairing=bad)
    for method in ("none", "grad_log_ratio"):
        with pytest.raises(ValueError, match="mc_feng"):
            sample_bimodal_guided(fx, fy, rr, method, 1.0, 2, 4, "cpu", 3, mc_pairing="cross")
        with pytest.raises(ValueError, match="mc_feng"):
            paired_sampler(fx, fy, rr, method, 1.0, 2, 4, "cpu", 3, (1, 28, 28), (1, 28, 28), mc_pairing="cross")
    with pytest.raises(_lib.RgfmError, match="U-Net"):
        sample_bimodal_guided(make_module("fm_original"), make_module("fm_original_y"), rr, "mc_feng", 1.0, 2, 4, "cpu", 3,
                              mc_pairing="cross")
    with pytest.raises(_lib.RgfmError, match="1024"):
        sample_bimodal_guided(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 1025, mc_pairing="cross")
    for kw in ({}, {"mc_pairing": "paired"}, {"mc_pairing": "cross"}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            sample_bimodal_guided(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 3, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sample_bimodal_guided_mnist_svhn(make_module("mnist32"), make_module("svhn"), make_module("ratio_ms"), "mc_feng",
                                         1.0, 2, 4, "cpu", 3, mc_pairing="cross")
    noise = tuple(torch.zeros(2, 1, 28, 28) for _ in range(4))
    with pytest.raises(_lib.RgfmError, match="sharded"):
        sharded_paired_sampler(fx, fy, rr, "mc_feng", 1.0, 4, noise, torch.device("cpu"), mc_pairing="cross")
    with pytest.raises(_lib.RgfmError, match="sharded"):
        make_sharded_sampler((1, 28, 28), (1, 28, 28))(fx, fy, rr, "mc_feng", 1.0, 2, 4, "cpu", 3, mc_pairing="cross")
    with pytest.raises(ValueError, match="mc_pairing"):
        sharded_paired_sampler(fx, fy, rr, "mc_feng", 1.0, 4, noise, torch.device("cpu"), mc_pairing="both")


def _parses(module, argv, monkeypatch, tmp_path):
    """main(argv) gets past the parser: it ends at the missing-checkpoint message (1) or at the device check."""
    monkeypatch.chdir(tmp_path)
    try:
        return module.main(argv)
    except RuntimeError as e:
        assert "HIP device" in str(e) or "no CPU path" in str(e), e
        return 1


def test_mc_pairing_parses_on_all_four_clis(monkeypatch, tmp_path, capsys):
    from ratio_guided_multimodal_fm_amd import evaluate, evaluate_mnist_svhn, sample, sample_mnist_svhn
    for module in (sample, sample_mnist_svhn):
        for pairing in ("paired", "cross"):
            assert _parses(module, ["--guidance_method", "mc_feng", "--mc_pairing", pairing], monkeypatch, tmp_path) == 1
        with pytest.raises(SystemExit):
            module.main(["--guidance_method", "mc_feng", "--mc_pairing", "all"])
        with pytest.raises(SystemExit):  # 'cross' pairs up the MC set of mc_feng
            module.main(["--guidance_method", "none", "--mc_pairing", "cross"])
    with pytest.raises(SystemExit):
        sample.main(["--guidance_method", "mc_feng", "--mc_pairing", "cross", "--model", "original"])
    with pytest.raises(SystemExit):
        sample_mnist_svhn.main(["--guidance_method", "mc_feng", "--mc_pairing", "cross", "--sharded"])
    for module in (evaluate, evaluate_mnist_svhn):
        for pairing in ("paired", "cross"):
            assert _parses(module, ["--mc_pairing", pairing], monkeypatch, tmp_path) == 1
        with pytest.raises(SystemExit):
            module.main(["--mc_pairing", "all"])
    with pytest.raises(SystemExit):
        evaluate_mnist_svhn.main(["--mc_pairing", "cross", "--sharded"])
    capsys.readouterr()


def test_sweep_rows_record_the_pairing_only_when_it_is_cross():
    from helpers import golden, make_module
    from ratio_guided_multimodal_fm_amd import evaluate, evaluate_mnist_svhn
    g = golden("sampler_pair_ms")
    xs = torch.from_numpy(np.concatenate([g[f"c{i}_x"] for i in range(6)]))
    ys = torch.from_numpy(np.concatenate([g[f"c{i}_y"] for i in range(6)]))
    seen = []

    def sampler(fm_m, fm_s, ratio, method, strength, n, num_steps, device, mc, **kw):
        seen.append((method, kw))
        return xs[:n], ys[:n]

    def old_sampler(fm_m, fm_s, ratio, method, strength, n, num_steps, device, mc):  # (no mc_pairing keyword at all)
        return xs[:n], ys[:n]
    cm, cs = make_module("clf_mnist"), make_module("clf_svhn")
    base = {"method", "guidance_strength", "experiment", "coherence_acc", "num_samples"}
    sweep = lambda **kw: evaluate_mnist_svhn.run_sweep(None, None, lambda: object(), cm, cs, ["none", "mc_feng"], [0.0, 0.5], 8, 20,
                                                       "cpu", 16, **kw)
    res = sweep(sampler=sampler, mc_pairing="cross")
    assert seen == [("none", {}), ("mc_feng", {"mc_pairing": "cross"}), ("mc_feng", {"mc_pairing": "cross"})]
    assert set(res[0]) == base and all(set(r) == base | {"mc_pairing"} and r["mc_pairing"] == "cross" for r in res[1:])
    for kw in ({}, {"mc_pairing": "paired"}):
        assert all(set(r) == base for r in sweep(sampler=old_sampler, **kw))
    with pytest.raises(ValueError, match="mc_pairing"):
        sweep(sampler=sampler, mc_pairing="all")
    g28 = golden("sampler_pair28")
    x28 = torch.from_numpy(np.concatenate([g28[f"c{i}_x"] for i in range(3)]))
    y28 = torch.from_numpy(np.concatenate([g28[f"c{i}_y"] for i in range(3)]))
    n28 = min(8, len(x28))
    res = evaluate.run_sweep(None, None, lambda: object(), make_module("clf_mnist28"), ["none", "mc_feng"], [0.0, 1.0], n28, 20,
                             "cpu", 16, "none", sampler=lambda *a, **kw: (x28[:n28], y28[:n28]), mc_pairing="cross")
    base28 = {"method", "guidance_strength", "transform_type", "coherence_acc", "num_samples"}
    assert set(res[0]) == base28 and set(res[1]) == base28 | {"mc_pairing"}
