"""Guidance diagnostics on the GPU (include/rgfm.h, RGFM_DIAG_*; csrc/guidance.hip: guid_diag_wstats_kernel,
guid_diag_rownorm_kernel) against the float64 yardstick tests/diag_ref64.py.

Block level: rgfm_guidance_diag on guidance_ref64.CASES and rgfm_guidance_diag_cond on cond_ref64.CASES, every
(t, centre), the case's own ratios and the graded ones r = exp(s z), s = 2 and 6 (effective sample size from about N
down to about 1; tests/test_diag_cpu.py asserts that span).  Bounds: diag_ref64.bounds (its docstring derives them from
guidance_ref64.tol_w, the fp32 sums and guidance_ref64.velocity_bound); tests/test_diag_cpu.py holds the reference's
own fp32 arithmetic inside them.

Loop level: the five guided loops on the generic nets g16 (1x16x16) and g24 (3x24x24) and the flexible estimator of
tests/test_gpu_ode.py (B = 3, N = 7, 4 steps; the FlowMatchingModel pair on its own fixtures, B = 5, N = 9, 6 steps):
diagnostics change no bit of the state; the records of one call are those of step-by-step calls; one guided stage per
loop against float64 from the fp32 state in front of it.  Everything "equal" is torch.equal.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import cond_grad_ref64 as CG
import cond_ref64 as C
import diag_ref64 as D
import fmnet_ref64 as FM
import guidance_ref64 as G
import ode_ref64 as O
import test_gpu_ode as T
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd.utils.diagnostics import GuidanceDiagnostics

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM = -1, -2
EULER, MIDPOINT = 0, 1
SENTINEL = -7777.0
STEPS = T.STEPS  # 4
B_LOOP = 3
_p, _stream = T._p, T._stream


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def _dev(inp, dev):
    return {k: torch.tensor(v, device=dev) for k, v in inp.items()}


# ================================================================== block level
@pytest.mark.parametrize("centre", G.CENTRES)
@pytest.mark.parametrize("si", range(len(G.STEPS)))
@pytest.mark.parametrize("ci", range(len(G.CASES)))
def test_paired_block_vs_float64(dev, ci, si, centre):
    B, N, dx, dy = G.CASES[ci]
    t = G.STEPS[si][0]
    tw = G.tol_w(t, centre)
    for s in D.GRADES:
        inp, ref = D.paired(ci, si, centre, s)
        d = _dev(inp, dev)
        got = _engine.guidance_diag(d["x"], d["y"], d["vx"], d["vy"], d["mx"], d["my"], d["r"], t).cpu().numpy()
        D.check(got, ref, D.bounds(inp, ref, N, (dx, dy), t, tw), f"diag {G.CASES[ci]} t={t} centre={centre} s={s}")
        assert (got[:, 0] >= 1 - 1e-5).all() and (got[:, 0] <= N * (1 + 1e-5)).all()


@pytest.mark.parametrize("centre", C.CENTRES)
@pytest.mark.parametrize("si", range(len(C.STEPS)))
@pytest.mark.parametrize("ci", range(len(C.CASES)))
def test_one_sided_block_vs_float64(dev, ci, si, centre):
    B, N, dim = C.CASES[ci]
    t = C.STEPS[si][0]
    tw = G.tol_w(t, centre)
    for s in D.GRADES:
        inp, ref = D.one_sided(ci, si, centre, s)
        d = _dev(inp, dev)
        got = _engine.guidance_diag_cond(d["s"], d["v"], d["m"], d["R"], t).cpu().numpy()
        bnd = D.bounds({"mx": inp["m"], "my": np.zeros(1)}, ref, N, (dim,), t, tw)
        D.check(got, ref, bnd, f"diag_cond {C.CASES[ci]} t={t} centre={centre} s={s}")
        assert not got[:, 5].any() and not got[:, 7].any()  # dy = 0: the y entries stay 0


def _block_raw(d, t, out, ws, ws_bytes):
    B, N = d["x"].shape[0], d["mx"].shape[0]
    return _lib.lib().rgfm_guidance_diag(_p(d["x"]), _p(d["y"]), _p(d["vx"]), _p(d["vy"]), _p(d["mx"]), _p(d["my"]), _p(d["r"]),
                                         B, N, d["x"].shape[1], d["y"].shape[1], float(t), _p(out), _p(ws), ws_bytes, _stream())


def _block_bytes(B, N, dx, dy):
    nb = ctypes.c_size_t()
    assert _lib.lib().rgfm_guidance_diag_workspace_bytes(B, N, dx, dy, ctypes.byref(nb)) == 0
    return nb.value


@pytest.mark.parametrize("ci", [0, 5])
def test_block_writes_the_records_and_nothing_else(dev, ci):
    """Whatever the workspace holds (NaN or zeros, exact size or 4 KB more) the records are the same bits, the inputs --
    the velocities too -- keep theirs, 256 floats on each side of the records keep their sentinel; the records do not
    depend on the batch a row is in."""
    B, N, dx, dy = G.CASES[ci]
    si = 2
    t = G.STEPS[si][0]
    inp = D.paired(ci, si, 1.0, 2.0)[0]
    need = _block_bytes(B, N, dx, dy)
    outs = []
    for fill in (float("nan"), 0.0):
        for extra in (0, 4096):
            d = _dev(inp, dev)
            big = torch.full((256 + B * 8 + 256,), SENTINEL, device=dev)
            ws = torch.full(((need + extra) // 4,), fill, device=dev)
            assert _block_raw(d, t, big[256:-256], ws, need + extra) == 0
            torch.cuda.synchronize()
            assert bool((big[:256] == SENTINEL).all()) and bool((big[-256:] == SENTINEL).all())
            for k, v in inp.items():
                assert torch.equal(d[k], torch.tensor(v, device=dev)), k
            outs.append(big[256:-256].clone())
    for o in outs:
        assert bool(torch.isfinite(o).all()) and torch.equal(o, outs[0])
    full = outs[0].view(B, 8)
    for rows in (slice(0, 1), slice(B - 1, B)):
        d = _dev(inp, dev)
        part = _engine.guidance_diag(d["x"][rows], d["y"][rows], d["vx"][rows], d["vy"][rows], d["mx"], d["my"], d["r"], t)
        assert torch.equal(part, full[rows])


def test_block_argument_errors_come_back_before_any_launch(dev):
    ci, si = 0, 1
    B, N, dx, dy = G.CASES[ci]
    t = G.STEPS[si][0]
    d = _dev(D.paired(ci, si, 1.0, 0.0)[0], dev)
    need = _block_bytes(B, N, dx, dy)
    out = torch.full((B * 8,), SENTINEL, device=dev)
    ws = torch.full((need // 4,), SENTINEL, device=dev)
    assert _block_raw(d, t, None, ws, need) == EINVAL            # null diag_out
    assert _block_raw(d, t, out, ws, need - 1) == ENOMEM         # a workspace one byte short
    assert _block_raw(d, t, out, None, need) == EINVAL
    L = _lib.lib()
    assert L.rgfm_guidance_diag_cond(_p(d["x"]), _p(d["vx"]), _p(d["mx"]), _p(d["r"]), B, 4097, dx, float(t), _p(out), _p(ws),
                                     need, _stream()) == EINVAL  # n_mc above 4096
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())


# ================================================================== loop level
class FmRaw:
    """The FlowMatchingModel pair (rgfm_fmnet_sample_pair) with the interface of test_gpu_ode.Raw; Euler only."""
    kind, N_MC, STEPS, GAMMA = "fmnet", 9, 6, 0.5

    def __init__(self, dev):
        self.fx, self.fy = _fm_modules(dev)
        x, y, mx, my, r = (a.to(dev).clone() for a in FM.pair_inputs(self.N_MC))
        self.state, self.keep = [x, y], (mx, my, r)
        hx, hy = self.fx._engine.handle(dev), self.fy._engine.handle(dev)
        B = x.shape[0]
        self.ws_args = (hx, hy, B, self.N_MC)
        self.args = (hx, hy, _p(x), _p(y), _p(mx), _p(my), _p(r), self.N_MC, B, self.STEPS, self.GAMMA)
        self.L = _lib.lib()

    def run(self, solver, b, e):
        nb = ctypes.c_size_t()
        assert self.L.rgfm_fmnet_sample_pair_workspace_bytes(*self.ws_args, ctypes.byref(nb)) == 0
        ws = torch.empty(nb.value, dtype=torch.uint8, device=self.state[0].device)
        return self.L.rgfm_fmnet_sample_pair(*self.args, b, e, _p(ws), nb.value, _stream())


@functools.lru_cache(maxsize=None)
def _fm_modules(dev):
    (fxd, txd), (fyd, tyd) = FM.PAIR_DIMS
    return (copy.deepcopy(FM.module_cpu(fxd, txd)).to(dev), copy.deepcopy(FM.module_cpu(fyd, tyd, FM.PAIR_SEED_Y)).to(dev))


KINDS = ("pair", "cond", "pair_grad", "cond_grad", "fmnet")
MC_KINDS = ("pair", "cond", "fmnet")


def make(kind, dev):
    """A fresh loop on fresh copies of its start state: test_gpu_ode's raw loops at B = 3 (N = 7), or the fmnet pair."""
    return FmRaw(dev) if kind == "fmnet" else T.make_raw(kind, B_LOOP, dev)


def steps_of(raw):
    return raw.STEPS if raw.kind == "fmnet" else STEPS


def batch_of(raw):
    return raw.state[0].shape[0]


def stages(solver, ns):
    return ns * (2 if solver == MIDPOINT else 1)


def diag_bytes(raw, solver):
    nb = ctypes.c_size_t()
    if raw.kind == "fmnet":
        rc = raw.L.rgfm_fmnet_sample_pair_diag_workspace_bytes(*raw.ws_args, ctypes.byref(nb))
    else:
        rc = getattr(raw.L, f"rgfm_sample_{raw.kind}_diag_workspace_bytes")(*raw.ws_args, solver, ctypes.byref(nb))
    assert rc == 0
    return nb.value


def diag_run(raw, solver, b, e, rec, records="all", short=0, ws_fill=None):
    """rc of the *_diag loop over steps [b, e) into `rec` ([n_stages, B, 8] or None) with capacity `records`."""
    nb = diag_bytes(raw, solver)
    ws = torch.empty(nb, dtype=torch.uint8, device=raw.state[0].device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    raw.last_ws = ws
    cap = (0 if rec is None else rec.shape[0] * rec.shape[1]) if records == "all" else records
    if raw.kind == "fmnet":
        return raw.L.rgfm_fmnet_sample_pair_diag(*raw.args, b, e, _p(rec), cap, _p(ws), nb - short, _stream())
    return getattr(raw.L, f"rgfm_sample_{raw.kind}_diag")(*raw.args, b, e, solver, _p(rec), cap, _p(ws), nb - short, _stream())


def new_records(raw, solver, ns, dev):
    return torch.full((stages(solver, ns), batch_of(raw), 8), SENTINEL, device=dev)


def solvers_of(kind):
    return (EULER,) if kind == "fmnet" else (EULER, MIDPOINT)


@pytest.mark.parametrize("kind", KINDS)
def test_state_with_diagnostics_is_the_state_without(dev, kind):
    """RGFM_GRAPH at its default: the plain paired Euler loop replays a hipGraph, the one with diagnostics runs kernel by
    kernel -- the same bits.  A null sink through the *_diag entry point is the plain loop too."""
    for solver in solvers_of(kind):
        plain, diag, null = make(kind, dev), make(kind, dev), make(kind, dev)
        ns = steps_of(plain)
        assert plain.run(solver, 0, ns) == 0
        rec = new_records(diag, solver, ns, dev)
        assert diag_run(diag, solver, 0, ns, rec) == 0
        assert diag_run(null, solver, 0, ns, None) == 0
        torch.cuda.synchronize()
        for a, b, c in zip(plain.state, diag.state, null.state):
            assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c), (kind, solver)
        assert bool(torch.isfinite(rec).all()) and not bool((rec == SENTINEL).any())


@pytest.mark.parametrize("kind", KINDS)
def test_records_of_one_call_are_those_of_step_by_step_calls(dev, kind):
    """Stage order, the step offset and the unguided first stage: records [0, ns) == cat of the calls [i, i + 1)."""
    for solver in solvers_of(kind):
        whole, split = make(kind, dev), make(kind, dev)
        ns = steps_of(whole)
        rec = new_records(whole, solver, ns, dev)
        assert diag_run(whole, solver, 0, ns, rec, ws_fill=0xA5) == 0  # (the byte pattern of test_gpu_sampler_ws.py)
        parts = []
        for i in range(ns):
            parts.append(new_records(split, solver, 1, dev))
            assert diag_run(split, solver, i, i + 1, parts[-1]) == 0
        torch.cuda.synchronize()
        assert torch.equal(rec, torch.cat(parts)), (kind, solver)
        for a, b in zip(whole.state, split.state):
            assert torch.equal(a, b)
        d = GuidanceDiagnostics.from_records(rec, "mc_feng" if kind in MC_KINDS else "grad_log_ratio",
                                             "midpoint" if solver else "euler", ns)
        if kind in MC_KINDS:
            assert not d.guided[0] and bool(d.guided[1:].all())
            assert not bool(rec[0].any())                       # t = 0: an all-zero record
            ess = d.ess()[1:]
            N = whole.N_MC if kind == "fmnet" else 7
            assert bool((ess >= 1 - 1e-5).all()) and bool((ess <= N * (1 + 1e-5)).all())
            assert bool((rec[1:, :, 1] >= rec[1:, :, 2]).all()) and bool((rec[1:, :, 3] > 0).all())
            assert bool((rec[1:, :, 4] > 0).all()) and bool((rec[1:, :, 6] > 0).all())
            assert bool((rec[1:, :, 5] > 0).all()) == (kind != "cond") and bool((rec[1:, :, 7] > 0).all()) == (kind != "cond")
        else:
            assert not bool(rec[..., :4].any())                 # ess == 0: not MC-guided
            assert bool((rec[..., 4] > 0).all()) and bool((rec[..., 6] > 0).all())
            assert bool((rec[..., 5] > 0).all()) == (kind == "pair_grad") and bool((rec[..., 7] > 0).all()) == (kind == "pair_grad")


@pytest.mark.parametrize("kind", KINDS)
def test_loop_argument_errors_come_back_before_any_launch(dev, kind):
    raw = make(kind, dev)
    ns, solver = steps_of(raw), EULER
    before = [a.clone() for a in raw.state]
    rec = new_records(raw, solver, ns, dev)
    full = rec.shape[0] * rec.shape[1]
    assert diag_run(raw, solver, 0, ns, None, records=full) == EINVAL      # null diag_out with a capacity
    assert diag_run(raw, solver, 0, ns, rec, records=0) == EINVAL          # ... and the reverse
    assert diag_run(raw, solver, 0, ns, rec, records=full - 1) == EINVAL   # one record short
    if kind != "fmnet":
        assert diag_run(raw, MIDPOINT, 0, ns, rec, records=full) == EINVAL  # (twice the stages)
    rc = diag_run(raw, solver, 0, ns, rec, short=1, ws_fill=0x5A)          # a workspace one byte short
    assert rc == ENOMEM
    torch.cuda.synchronize()
    assert bool((raw.last_ws == 0x5A).all()) and bool((rec == SENTINEL).all())
    for a, b in zip(raw.state, before):
        assert torch.equal(a, b)
    # the diag query is the plain one plus the scratch velocities of the MC loops, and nothing for the gradient loops
    if kind != "fmnet":
        plain = raw.ws_bytes(solver)[1]
        extra = diag_bytes(raw, solver) - plain
        dims = {"pair": 256 + 1728, "cond": 1728}.get(kind, 0)
        assert extra >= 4 * B_LOOP * dims and (extra == 0) == (kind in ("pair_grad", "cond_grad"))


# ---- one guided stage per loop against float64
STAGE = 2  # Euler step 2 of 4: t = 0.5, a key of guidance_ref64.ORACLE_DW
TW_LOOP = min(G.tol_w(0.5, c) for c in G.CENTRES)  # (the loops' inputs are neither centre: the tighter of the two)


def _state_before_and_record(raw, dev, step):
    """The fp32 state the chunked run hands back in front of Euler step `step`, and that step's records."""
    for i in range(step):
        assert diag_run(raw, EULER, i, i + 1, new_records(raw, EULER, 1, dev)) == 0
    torch.cuda.synchronize()
    before = [a.clone() for a in raw.state]
    rec = new_records(raw, EULER, 1, dev)
    assert diag_run(raw, EULER, step, step + 1, rec) == 0
    torch.cuda.synchronize()
    return before, rec[0].cpu().numpy()


def _v_extra(D_, v64):
    """sqrt(D) 1e-5 max(1, max |v64|): the net's own tolerance (TOL_EVAL) carried into a row norm."""
    return np.sqrt(D_) * 1e-5 * max(1.0, float(np.abs(v64).max()))


def test_pair_stage_vs_float64(dev):
    raw = make("pair", dev)
    (x, y), got = _state_before_and_record(raw, dev, STAGE)
    t = STAGE * (1.0 / STEPS)
    B = x.shape[0]
    x64, y64 = T.f64(x.cpu()), T.f64(y.cpu())
    vx, vy = O.velocity_of(T.net("g16"))(x64, t), O.velocity_of(T.net("g24"))(y64, t)
    mx, my, r = raw.keep
    inp = {"x": x64.reshape(B, -1), "y": y64.reshape(B, -1), "vx": vx.reshape(B, -1), "vy": vy.reshape(B, -1),
           "mx": T.f64(mx.cpu()).reshape(7, -1), "my": T.f64(my.cpu()).reshape(7, -1), "r": T.f64(r.cpu())}
    ref = D.diag64(inp, t)
    bnd = D.bounds(inp, ref, 7, (256, 1728), t, TW_LOOP, (_v_extra(256, vx), _v_extra(1728, vy)))
    D.check(got, ref, bnd, "pair loop, step 2")


def test_cond_stage_vs_float64(dev):
    raw = make("cond", dev)
    (s,), got = _state_before_and_record(raw, dev, STAGE)
    t = STAGE * (1.0 / STEPS)
    B = s.shape[0]
    s64 = T.f64(s.cpu())
    v = O.velocity_of(T.net("g24"))(s64, t)
    m, R = raw.keep
    inp = {"s": s64.reshape(B, -1), "v": v.reshape(B, -1), "m": T.f64(m.cpu()).reshape(7, -1), "R": T.f64(R.cpu())}
    ref = D.diag_cond64(inp, t)
    bnd = D.bounds({"mx": inp["m"], "my": np.zeros(1)}, ref, 7, (1728,), t, TW_LOOP, (_v_extra(1728, v),))
    D.check(got, ref, bnd, "cond loop, step 2")


def test_fmnet_pair_stage_vs_float64(dev):
    raw = make("fmnet", dev)
    step = 3  # of 6: t = 0.5
    (x, y), got = _state_before_and_record(raw, dev, step)
    t = step * (1.0 / raw.STEPS)
    assert t == 0.5
    B, N = x.shape[0], raw.N_MC
    sdx, sdy = FM.pair_sds()
    with torch.no_grad():
        tt = torch.tensor([t], dtype=torch.float64)
        vx, vy = FM.forward64(sdx, x.cpu().double(), tt).numpy(), FM.forward64(sdy, y.cpu().double(), tt).numpy()
    mx, my, r = raw.keep
    inp = {"x": T.f64(x.cpu()).reshape(B, -1), "y": T.f64(y.cpu()).reshape(B, -1), "vx": vx.reshape(B, -1), "vy": vy.reshape(B, -1),
           "mx": T.f64(mx.cpu()).reshape(N, -1), "my": T.f64(my.cpu()).reshape(N, -1), "r": T.f64(r.cpu())}
    ref = D.diag64(inp, t)
    bnd = D.bounds(inp, ref, N, (784, 784), t, TW_LOOP, (_v_extra(784, vx), _v_extra(784, vy)))
    D.check(got, ref, bnd, "fmnet pair loop, step 3 of 6")


def _check_grad_record(got, v64s, g64s, what):
    """Gradient loops: v norms as the MC loops'; g norms within sqrt(D) 1e-4 max |g64| (the project's gradient
    tolerance, per element, through the triangle inequality); the first four entries 0."""
    assert not got[:, :4].any(), what
    for k, (v64, g64) in enumerate(zip(v64s, g64s)):
        B = v64.shape[0]
        v64, g64 = v64.reshape(B, -1), g64.reshape(B, -1)
        D_ = v64.shape[1]
        vn, gn = np.sqrt((v64 ** 2).sum(1)), np.sqrt((g64 ** 2).sum(1))
        ev, eg = np.abs(got[:, 4 + k] - vn), np.abs(got[:, 6 + k] - gn)
        bv, bg = D_ * D.U24 * vn + _v_extra(D_, v64), np.sqrt(D_) * 1e-4 * float(np.abs(g64).max())
        print(f"{what} modality {k}: |v| err / bound {float((ev / bv).max()):.2f}   |g| err / bound {float((eg / bg).max()):.2f}   "
              f"|g| {gn.min():.3e} .. {gn.max():.3e}")
        assert (ev <= bv).all() and (eg <= bg).all(), (what, k)
    if len(v64s) == 1:
        assert not got[:, 5].any() and not got[:, 7].any(), what


def test_pair_grad_stage_vs_float64(dev):
    raw = make("pair_grad", dev)
    (x, y), got = _state_before_and_record(raw, dev, STAGE)
    t = STAGE * (1.0 / STEPS)
    x64, y64 = T.f64(x.cpu()), T.f64(y.cpu())
    vx, vy = O.velocity_of(T.net("g16"))(x64, t), O.velocity_of(T.net("g24"))(y64, t)
    rr = T.flex()
    gx, gy, _ = CG.grad_both64(CG.kind_of(rr), CG.params64(rr), x.cpu(), y.cpu(), "disc")
    _check_grad_record(got, (vx, vy), (gx.numpy(), gy.numpy()), "pair_grad loop, step 2")


def test_cond_grad_stage_vs_float64(dev):
    raw = make("cond_grad", dev)
    (s,), got = _state_before_and_record(raw, dev, STAGE)
    t = STAGE * (1.0 / STEPS)
    rr, tnet, cond, _ = T.cond_grad_case("x")
    v = O.velocity_of(tnet)(T.f64(s.cpu()), t)
    g = CG.grad_given64(CG.kind_of(rr), CG.params64(rr), cond, s.cpu(), "x", "disc")[0]
    _check_grad_record(got, (v,), (g.numpy(),), "cond_grad loop, step 2")


# ================================================================== Python
def test_python_samplers_fill_the_object(dev):
    from ratio_guided_multimodal_fm_amd.utils.flow_utils import paired_sampler, sample_conditional
    fx, fy, rr = T.net("g16").to(dev), T.net("g24").to(dev), T.flex().to(dev)
    sx, sy = T.shape_of("g16"), T.shape_of("g24")
    for method in ("mc_feng", "grad_log_ratio"):
        for solver in ("euler", "midpoint"):
            outs = []
            for diag in (None, GuidanceDiagnostics(), GuidanceDiagnostics()):
                torch.manual_seed(31)
                xs, ys = paired_sampler(fx, fy, rr, method, 0.7, B_LOOP, STEPS, dev, 7, sx, sy, verbose=False, solver=solver,
                                        diagnostics=diag)
                outs.append((xs, ys, diag))
            n = STEPS * (2 if solver == "midpoint" else 1)
            (x0, y0, _), (x1, y1, d1), (x2, y2, d2) = outs
            assert torch.equal(x0, x1) and torch.equal(y0, y1) and torch.equal(x0, x2)
            assert tuple(d1.records.shape) == (n, B_LOOP, 8) and d1.records.is_cuda and torch.equal(d1.records, d2.records)
            assert d1.t.shape == (n,) and torch.allclose(d1.sigma_t, 1 - d1.t + 1e-3)
            if method == "mc_feng":
                assert d1.guided.tolist() == [False] + [True] * (n - 1) and not bool(d1.records[0].any())
                assert bool((d1.ess()[1:] >= 1 - 1e-5).all()) and "sigma_t=" in d1.reference_block(1)
                assert d1.summary(1)["ess_min"] >= 1 - 1e-5
            else:
                assert bool(d1.guided.all()) and not bool(d1.ess().any()) and bool((d1.g_norm_y() > 0).all())
            # a one-sided run: the target's fields in the x entries
            torch.manual_seed(32)
            cond = T.start("g24", B_LOOP).to(dev)
            dc = GuidanceDiagnostics()
            torch.manual_seed(33)
            a = sample_conditional(fx, rr, cond, "y", STEPS, 0.7, 7, guidance_method=method, solver=solver, diagnostics=dc)
            torch.manual_seed(33)
            b = sample_conditional(fx, rr, cond, "y", STEPS, 0.7, 7, guidance_method=method, solver=solver)
            assert torch.equal(a, b) and tuple(dc.records.shape) == (n, B_LOOP, 8)
            first = 1 if method == "mc_feng" else 0  # (the MC loops' stage at t = 0 is unguided: an all-zero record)
            assert not bool(dc.v_norm_y().any()) and not bool(dc.g_norm_y().any())
            assert bool((dc.v_norm_x()[first:] > 0).all()) and bool((dc.g_norm_x()[first:] > 0).all())
            assert bool((dc.ess()[1:] >= 1 - 1e-5).all()) == (method == "mc_feng")


def test_cli_diagnostics_out_writes_the_arrays(dev, tmp_path, monkeypatch, capsys):
    from helpers import make_module
    from ratio_guided_multimodal_fm_amd import sample_mnist_svhn
    ck = tmp_path / "checkpoints"
    ck.mkdir()
    fm, fs, rr = make_module("mnist32"), make_module("svhn"), make_module("ratio_ms")
    torch.save({"epoch": 1, "model_state_dict": fm.state_dict(), "best_loss": 0.5}, ck / "flow_mnist32_best.pth")
    torch.save({"epoch": 1, "model_state_dict": fs.state_dict(), "best_loss": 0.5}, ck / "flow_svhn_best.pth")
    torch.save(rr.state_dict(), ck / "ratio_disc_mnist_svhn_best.pth")
    monkeypatch.chdir(tmp_path)
    argv = ["--guidance_method", "mc_feng", "--guidance_strength", "0.5", "--num_steps", "4", "--num_samples", "3",
            "--mc_batch_size", "5", "--seed", "9"]
    assert sample_mnist_svhn.main(argv) == 0
    plain = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_mc_feng_gamma0.5.pt")
    assert "Diagnostics" not in capsys.readouterr().out
    assert sample_mnist_svhn.main(argv + ["--diagnostics", "--diagnostics_out", "diag.npz"]) == 0
    out = capsys.readouterr().out
    assert "[MC Guidance Diagnostics at t=0.25]" in out and "Z_bar:" in out and "ESS: mean=" in out  # step int(0.3 * 4) = 1
    again = torch.load(tmp_path / "outputs" / "mnist_svhn" / "samples_mc_feng_gamma0.5.pt")
    assert torch.equal(plain["mnist"], again["mnist"]) and torch.equal(plain["svhn"], again["svhn"])
    z = np.load(tmp_path / "diag.npz")
    assert z["records"].shape == (4, 3, 8) and z["records"].dtype == np.float32
    assert z["t"].tolist() == [0.0, 0.25, 0.5, 0.75] and np.allclose(z["sigma_t"], 1 - z["t"] + 1e-3)
    assert not z["records"][0].any() and (z["records"][1:, :, 0] >= 1 - 1e-5).all() and (z["records"][1:, :, 0] <= 5 + 1e-4).all()
