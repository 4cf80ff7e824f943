#!/usr/bin/env python3
"""Bits and workspace sizes of the ratio estimators' inference and gradient entry points, for a same-box A/B of two
trees: one line per case -- name, *_workspace_bytes, SHA-256 of every output tensor.  Only the package's public
functions, raw C-ABI size queries and the case builders of tests/helpers.py, tests/test_gpu_ode.py and
tests/grad_loop_ref64.py, so the same file runs unchanged in a worktree of an earlier commit:

    python3 tools/ratio_bits.py > new.txt
    (cd ../parent && python3 tools/ratio_bits.py) > parent.txt
    diff parent.txt new.txt

Run it as one process per environment (default, RGFM_CONV=f32 / bx3, RGFM_REV_HX2=0, RGFM_OVERLAP=0).  Cases, at batch 1
and 5 of each kind -- RatioEstimatorMNISTSVHN (BatchNorm; convs feeding convs, a max-pool in front of the average pool),
RatioEstimator (GroupNorm, 28 -> 14 -> 7 -> 3), FlexibleRatioEstimator at 2x12 + 4x12 (odd levels) and at 1x8 + 1x8
(conv4 on one pixel, four samples per tile): eval for the three outputs, eval_cross at 3 x 2 by default and in chunks
of 4 pairs (RGFM_CROSS_ROWS), grad_log_ratio, cond_prepare + grad_log_ratio_cond for both sides.  Then sample_pair_grad
and sample_cond_grad, Euler and midpoint, 2 steps: on the "ms_64" estimator of grad_loop_ref64.py with the mnist32 / svhn
nets (the kind whose in-loop pass leaves the fp32 route) and on the flexible case of test_gpu_ode.py.
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import grad_loop_ref64 as G  # noqa: E402
import test_gpu_ode as T  # noqa: E402
from helpers import make_module, make_sweep_ratio  # noqa: E402
from ratio_guided_multimodal_fm_amd import _engine, _lib  # noqa: E402
from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.synth import load_synth  # noqa: E402

STEPS = 2
# name -> (module, x shape, y shape)
KINDS = {
    "ratio_ms": (lambda: make_module("ratio_ms"), (1, 32, 32), (3, 32, 32)),
    "ratio28": (lambda: make_module("ratio28"), (1, 28, 28), (1, 28, 28)),
    "flex_2x12_4x12": (lambda: load_synth(M.FlexibleRatioEstimator(2, 4, 64, 128), 31).eval(), (2, 12, 12), (4, 12, 12)),
    "flex_1x8_1x8": (lambda: make_sweep_ratio("w192"), (1, 8, 8), (1, 8, 8)),
}


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def line(name, nbytes, outs):
    print(name, nbytes, *[sha(o) for o in outs], flush=True)


def query(fn, *args):
    nb = ctypes.c_size_t()
    _lib.check(getattr(_lib.lib(), fn)(*args, ctypes.byref(nb)))
    return nb.value


def images(shape, n, seed, dev):
    return torch.randn(n, *shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def entry_points(name, dev):
    make, sx, sy = KINDS[name]
    m = make().to(dev)
    e = m._engine
    for B in (1, 5):
        x, y = images(sx, B, 9100 + B, dev), images(sy, B, 9200 + B, dev)
        for what in ("score", "log_ratio", "ratio"):
            out = e.eval(x, y, what)
            line(f"{name}/B{B}/eval/{what}", query("rgfm_ratio_workspace_bytes", e.handle(dev), B), [out])
        gx, gy, lr = e.grad_log_ratio(x, y)
        line(f"{name}/B{B}/grad_log_ratio", query("rgfm_ratio_grad_workspace_bytes", e.handle(dev), B), [gx, gy, lr])
        for given, cond, target in (("x", x, y), ("y", y, x)):
            gi = 0 if given == "x" else 1
            ctx = e.cond_prepare(cond, given, tuple(target.shape[1:]))
            line(f"{name}/B{B}/cond_prepare/given_{given}",
                 query("rgfm_ratio_cond_prepare_workspace_bytes", e.handle(dev), gi, B), [ctx])
            g, lr = e.grad_log_ratio_cond(ctx, given, target)
            line(f"{name}/B{B}/grad_log_ratio_cond/given_{given}",
                 query("rgfm_ratio_grad_cond_workspace_bytes", e.handle(dev), gi, B), [g, lr])
    cx, cy = images(sx, 3, 9300, dev), images(sy, 2, 9400, dev)
    for rows in (None, "4"):
        if rows:
            os.environ["RGFM_CROSS_ROWS"] = rows
        try:
            for what in ("score", "log_ratio", "ratio"):
                out = e.eval_cross(cx, cy, what)
                line(f"{name}/cross3x2/rows_{rows or 'default'}/{what}",
                     query("rgfm_ratio_cross_workspace_bytes", e.handle(dev), 3, 2), [out])
        finally:
            os.environ.pop("RGFM_CROSS_ROWS", None)


def loops(name, rr, fx, fy, x0, y0, gamma, dev):
    """The two gradient-guided loops of one estimator and its U-Net pair from the states (x0, y0), CPU tensors."""
    rr, fx, fy = rr.to(dev), fx.to(dev), fy.to(dev)
    B = x0.shape[0]
    for solver, sid in (("euler", 0), ("midpoint", 1)):
        x, y = x0.to(dev).clone(), y0.to(dev).clone()
        _engine.sample_pair_grad(fx, fy, rr, x, y, STEPS, gamma, solver=solver)
        nb = query("rgfm_sample_pair_grad_ode_workspace_bytes", fx._engine.handle(dev), fy._engine.handle(dev),
                   rr._engine.handle(dev), B, sid)
        line(f"{name}/pair_grad/{solver}", nb, [x, y])
        for given, cond, s0, net in (("x", x0, y0, fy), ("y", y0, x0, fx)):
            gi = 0 if given == "x" else 1
            s = s0.to(dev).clone()
            ctx = rr._engine.cond_prepare(cond.to(dev), given, tuple(s0.shape[1:]))
            _engine.sample_cond_grad(net, rr, s, ctx, given, STEPS, gamma, solver=solver)
            nb = query("rgfm_sample_cond_grad_ode_workspace_bytes", net._engine.handle(dev), rr._engine.handle(dev), gi, B, sid)
            line(f"{name}/cond_grad/given_{given}/{solver}", nb, [s])


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    _lib.lib()
    for name in KINDS:
        entry_points(name, dev)
    x0, y0 = G._inputs("ms_64", G.B_MAIN)
    loops("loop_ms_64", G.estimator("ms_64", "disc", 0), G.unet("mnist32"), G.unet("svhn"), x0, y0, 64.0, dev)
    loops("loop_flex", T.flex(), T.net("g16"), T.net("g24"), T.start("g16", 5), T.start("g24", 5), T.GAMMA, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
