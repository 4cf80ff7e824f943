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


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    _lib.lib()
    raw_cases(dev)
    two_cases(dev)
    fmnet_cases(dev)
    python_surface(dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
