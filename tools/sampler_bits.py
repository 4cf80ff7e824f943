#!/usr/bin/env python3
"""Bits of every sampler loop, for a same-box A/B of two trees: one line per case -- name, workspace bytes, SHA-256 of
every state tensor.  Only the package's public functions and raw C-ABI calls, and the case builders of
tests/test_gpu_ode.py, so the same file runs unchanged in a worktree of an earlier commit:

    python3 tools/sampler_bits.py > new.txt
    (cd ../parent && python3 tools/sampler_bits.py) > parent.txt
    diff parent.txt new.txt

Run it as one process per environment (default, RGFM_GRAPH=1 / 0, RGFM_OVERLAP=0, RGFM_PREPHASE_PRIO=0): the switches are
read per call, but a process per setting keeps the runs independent.  Cases: the five U-Net loops x {Euler entry point,
_ode Euler, _ode midpoint} x {steps 0..4, 0..2 + 2..4}; rgfm_sample_two through sample_two_streams at 5 / 3 rows; the pair
loop at 6 steps (the graph-replay path under RGFM_GRAPH=1); the two FlowMatchingModel loops; the Python sample_* surface.
Then the guided calls' other arguments, through the Python surface, for both solvers and both step ranges: every guided
loop with a diagnostics tensor (its records are hashed behind the state, its size is the *_diag query's), the pair loop
over a ratio matrix [N, N] with and without records, every guided U-Net loop with gamma_rows, with a stage_scale that
holds a 0 and with both, the cross loop with both; and the nine guidance-block calls at one t (guidance_apply, _cond,
_cross with a scalar and with a row tensor; guidance_diag, _cond, _cross): vx, vy and the returned weights or records.
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import test_gpu_ode as T  # noqa: E402
from helpers import make_module  # noqa: E402
from ratio_guided_multimodal_fm_amd import _engine, _lib  # noqa: E402

STEPS, GAMMA, B, N = T.STEPS, T.GAMMA, 5, 7


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def line(name, nbytes, states):
    print(name, nbytes, *[sha(s) for s in states], flush=True)


def raw_cases(dev):
    for kind in T.KINDS:
        for tag, solver in (("old", None), ("ode_euler", T.EULER), ("ode_midpoint", T.MIDPOINT)):
            for rname, ranges in (("whole", [(0, STEPS)]), ("split", [(0, 2), (2, STEPS)])):
                r = T.make_raw(kind, B, dev)
                for b, e in ranges:
                    assert r.run(solver, b, e) == 0, _lib.lib().rgfm_last_error()
                line(f"raw/{kind}/{tag}/{rname}", r.ws_bytes(solver)[1], r.state)
    for tag, solver in (("old", None), ("ode_euler", T.EULER), ("ode_midpoint", T.MIDPOINT)):
        r = T.make_raw("pair", B, dev, steps=6)
        assert r.run(solver, 0, 6) == 0, _lib.lib().rgfm_last_error()
        line(f"raw/pair6/{tag}", r.ws_bytes(solver)[1], r.state)


def two_cases(dev):
    L = _lib.lib()
    fx, fy = T.net("g16").to(dev), T.net("g24").to(dev)
    for solver, sid in (("euler", 0), ("midpoint", 1)):
        x, y = T.start("g16", 5).to(dev).clone(), T.start("g24", 3).to(dev).clone()
        _engine.sample_two_streams(fx, x, fy, y, STEPS, solver=solver)
        nb = ctypes.c_size_t()
        _lib.check(L.rgfm_sample_two_workspace_bytes(fx._engine.handle(dev), fy._engine.handle(dev), 5, 3, sid, ctypes.byref(nb)))
        line(f"two/{solver}", nb.value, [x, y])


def fm_start(salt, n, dev):
    return torch.randn(n, 1, 28, 28, generator=torch.Generator().manual_seed(8100 + salt)).to(dev)


def fmnet_cases(dev):
    L = _lib.lib()
    mx_, my_ = make_module("fm_original", dev), make_module("fm_original_y", dev)
    hx, hy = mx_._engine.handle(dev), my_._engine.handle(dev)
    p, st = T._p, T._stream
    for rname, ranges in (("whole", [(0, STEPS)]), ("split", [(0, 2), (2, STEPS)])):
        x = fm_start(0, B, dev)
        nb = ctypes.c_size_t()
        _lib.check(L.rgfm_fmnet_workspace_bytes(hx, B, ctypes.byref(nb)))
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        for b, e in ranges:
            _lib.check(L.rgfm_fmnet_sample_single(hx, p(x), B, STEPS, b, e, p(ws), nb.value, st()))
        line(f"fmnet/single/{rname}", nb.value, [x])
        x, y = fm_start(0, B, dev), fm_start(1, B, dev)
        mx, my, r = 0.5 * fm_start(2, N, dev), 0.5 * fm_start(3, N, dev), T.ratios(N).to(dev)
        _lib.check(L.rgfm_fmnet_sample_pair_workspace_bytes(hx, hy, B, N, ctypes.byref(nb)))
        ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        for b, e in ranges:
            _lib.check(L.rgfm_fmnet_sample_pair(hx, hy, p(x), p(y), p(mx), p(my), p(r), N, B, STEPS, GAMMA, b, e, p(ws),
                                                nb.value, st()))
        line(f"fmnet/pair/{rname}", nb.value, [x, y])
    x, y = fm_start(0, B, dev), fm_start(1, B, dev)
    _engine.sample_single(mx_, x, STEPS)
    line("py/fmnet_single/euler", "-", [x])
    x = fm_start(0, B, dev)
    _engine.sample_pair(mx_, my_, x, y, 0.5 * fm_start(2, N, dev), 0.5 * fm_start(3, N, dev), T.ratios(N).to(dev), STEPS, GAMMA)
    line("py/fmnet_pair/euler", "-", [x, y])


def python_surface(dev):
    g16, g24, rr = T.net("g16").to(dev), T.net("g24").to(dev), T.flex().to(dev)
    for solver in ("euler", "midpoint"):
        for rname, ranges in (("whole", [(0, STEPS)]), ("split", [(0, 2), (2, STEPS)])):
            tag = f"{solver}/{rname}"
            x = T.start("g24", B).to(dev).clone()
            for b, e in ranges:
                _engine.sample_single(g24, x, STEPS, b, e, solver=solver)
            line(f"py/single/{tag}", "-", [x])
            x, y, mx, my, r = T.pair_inputs(B, N, dev)
            for b, e in ranges:
                _engine.sample_pair(g16, g24, x, y, mx, my, r, STEPS, GAMMA, b, e, solver=solver)
            line(f"py/pair/{tag}", "-", [x, y])
            s = T.start("g24", B).to(dev).clone()
            for b, e in ranges:
                _engine.sample_cond(g24, s, T.mc_set("g24", N).to(dev), T.ratios(B, N).to(dev), STEPS, GAMMA, b, e, solver=solver)
            line(f"py/cond/{tag}", "-", [s])
            x, y = T.start("g16", B).to(dev).clone(), T.start("g24", B).to(dev).clone()
            for b, e in ranges:
                _engine.sample_pair_grad(g16, g24, rr, x, y, STEPS, GAMMA, b, e, solver=solver)
            line(f"py/pair_grad/{tag}", "-", [x, y])
            er, tnet, cond, s0 = T.cond_grad_case("x")
            er, tnet, s = er.to(dev), tnet.to(dev), s0.to(dev).clone()
            ctx = er._engine.cond_prepare(cond.to(dev), "x", tuple(s0.shape[1:]))
            for b, e in ranges:
                _engine.sample_cond_grad(tnet, er, s, ctx, "x", STEPS, GAMMA, b, e, solver=solver)
            line(f"py/cond_grad/{tag}", "-", [s])


def guided_loops(dev):
    """name -> (batch, build): build() makes fresh inputs and returns (states, run(b, e, solver, **kw), size(sid)) -- the
    _engine call on steps [b, e) and the loop's *_diag (cross: *_cross) workspace query."""
    L = _lib.lib()
    g16, g24, rr = T.net("g16").to(dev), T.net("g24").to(dev), T.flex().to(dev)
    fmx, fmy = make_module("fm_original", dev), make_module("fm_original_y", dev)

    def query(name, *args):
        nb = ctypes.c_size_t()
        _lib.check(getattr(L, name)(*args, ctypes.byref(nb)))
        return nb.value

    def pair(matrix=False):
        def build():
            x, y, mx, my, r = T.pair_inputs(B, N, dev)
            r = T.ratios(N, N).to(dev) if matrix else r
            hx, hy = g16._engine.handle(dev), g24._engine.handle(dev)
            q = "rgfm_sample_pair_cross_workspace_bytes" if matrix else "rgfm_sample_pair_diag_workspace_bytes"
            return ([x, y], lambda b, e, solver, **k: _engine.sample_pair(g16, g24, x, y, mx, my, r, STEPS, GAMMA, b, e,
                                                                          solver=solver, **k),
                    lambda sid: query(q, hx, hy, B, N, sid))
        return build

    def cond():
        s, m, R = T.start("g24", B).to(dev).clone(), T.mc_set("g24", N).to(dev), T.ratios(B, N).to(dev)
        h = g24._engine.handle(dev)
        return ([s], lambda b, e, solver, **k: _engine.sample_cond(g24, s, m, R, STEPS, GAMMA, b, e, solver=solver, **k),
                lambda sid: query("rgfm_sample_cond_diag_workspace_bytes", h, B, N, sid))

    def pair_grad():
        x, y = T.start("g16", B).to(dev).clone(), T.start("g24", B).to(dev).clone()
        rr._engine.bind(x, y)
        hx, hy, hr = g16._engine.handle(dev), g24._engine.handle(dev), rr._engine.handle(dev)
        return ([x, y], lambda b, e, solver, **k: _engine.sample_pair_grad(g16, g24, rr, x, y, STEPS, GAMMA, b, e,
                                                                           solver=solver, **k),
                lambda sid: query("rgfm_sample_pair_grad_diag_workspace_bytes", hx, hy, hr, B, sid))

    def cond_grad():
        er, tnet, cond_, s0 = T.cond_grad_case("x")
        er, tnet, s = er.to(dev), tnet.to(dev), s0.to(dev).clone()
        ctx = er._engine.cond_prepare(cond_.to(dev), "x", tuple(s0.shape[1:]))
        h, hr = tnet._engine.handle(dev), er._engine.handle(dev)
        return ([s], lambda b, e, solver, **k: _engine.sample_cond_grad(tnet, er, s, ctx, "x", STEPS, GAMMA, b, e,
                                                                        solver=solver, **k),
                lambda sid: query("rgfm_sample_cond_grad_diag_workspace_bytes", h, hr, 0, s.shape[0], sid))

    def fm_pair():
        x, y = fm_start(0, B, dev), fm_start(1, B, dev)
        mx, my, r = 0.5 * fm_start(2, N, dev), 0.5 * fm_start(3, N, dev), T.ratios(N).to(dev)
        hx, hy = fmx._engine.handle(dev), fmy._engine.handle(dev)
        return ([x, y], lambda b, e, solver, **k: _engine.sample_pair(fmx, fmy, x, y, mx, my, r, STEPS, GAMMA, b, e,
                                                                      solver=solver, **k),
                lambda sid: query("rgfm_fmnet_sample_pair_diag_workspace_bytes", hx, hy, B, N))
    return {"pair": (B, pair()), "cross": (B, pair(True)), "cond": (B, cond), "pair_grad": (B, pair_grad),
            "cond_grad": (T.cond_grad_case("x")[3].shape[0], cond_grad), "fm_pair": (B, fm_pair)}


SCALE = (1.0, 0.0, 0.5, 1.5, 0.0, 1.0, 2.0, 0.25)  # a scale per stage of the whole integration (midpoint: 2 x STEPS)


def guided_cases(dev):
    loops = guided_loops(dev)
    # (what a line adds to the plain call: diag = a records tensor, rows = gamma_rows, scale = stage_scale)
    variants = [(k, v) for k in ("pair", "cond", "pair_grad", "cond_grad")
                for v in ("diag", "rows", "scale", "rows+scale")]
    variants += [("fm_pair", "diag"), ("cross", ""), ("cross", "diag"), ("cross", "rows+scale")]
    for solver, sid, per in (("euler", T.EULER, 1), ("midpoint", T.MIDPOINT, 2)):
        for rname, ranges in (("whole", [(0, STEPS)]), ("split", [(0, 2), (2, STEPS)])):
            for kind, variant in variants:
                if kind == "fm_pair" and sid:
                    continue  # (the FlowMatchingModel loops are Euler only)
                batch, build = loops[kind]
                states, run, size = build()
                records = []
                for b, e in ranges:
                    kw = {}
                    if "diag" in variant:
                        records.append(torch.zeros((e - b) * per, batch, _lib.DIAG_FLOATS, device=dev))
                        kw["diag"] = records[-1]
                    if "rows" in variant:
                        kw["gamma_rows"] = torch.linspace(0.2, 1.2, batch, device=dev)
                    if "scale" in variant:
                        kw["stage_scale"] = list(SCALE[b * per:e * per])
                    run(b, e, solver, **kw)
                line(f"guided/{kind}/{variant or 'plain'}/{solver}/{rname}", size(sid) if records or kind == "cross" else "-",
                     states + records)


def block_cases(dev):
    t = 0.5
    x, y, mx, my, r = T.pair_inputs(B, N, dev)
    matrix, rows = T.ratios(N, N).to(dev), torch.linspace(0.2, 1.2, B, device=dev)
    s, m, R = T.start("g24", B).to(dev), T.mc_set("g24", N).to(dev), T.ratios(B, N).to(dev)

    def v():  # fresh velocities: the apply blocks overwrite them
        return T.start("g16", B, 1).to(dev).clone(), T.start("g24", B, 1).to(dev).clone()
    for gname, gamma in (("scalar", GAMMA), ("rows", rows)):
        vx, vy = v()
        w = _engine.guidance_apply(x, y, vx, vy, mx, my, r, t, gamma, want_weights=True)
        line(f"block/apply/{gname}", "-", [vx, vy, w])
        _, vs = v()
        w = _engine.guidance_apply_cond(s, vs, m, R, t, gamma, want_weights=True)
        line(f"block/apply_cond/{gname}", "-", [vs, w])
        vx, vy = v()
        wx, wy = _engine.guidance_apply_cross(x, y, vx, vy, mx, my, matrix, t, gamma, want_weights=True)
        line(f"block/apply_cross/{gname}", "-", [vx, vy, wx, wy])
    vx, vy = v()
    line("block/diag", "-", [vx, vy, _engine.guidance_diag(x, y, vx, vy, mx, my, r, t)])
    line("block/diag_cond", "-", [vy, _engine.guidance_diag_cond(s, vy, m, R, t)])
    line("block/diag_cross", "-", [vx, vy, _engine.guidance_diag_cross(x, y, vx, vy, mx, my, matrix, t)])


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    _lib.lib()
    raw_cases(dev)
    two_cases(dev)
    fmnet_cases(dev)
    python_surface(dev)
    guided_cases(dev)
    block_cases(dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
