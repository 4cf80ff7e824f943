"""Workspace honesty of the sampler loops: every *_workspace_bytes figure is the end of the carve the call itself walks
(csrc/sampler_host.h), so a call handed EXACTLY that many bytes must stay inside them.

Per case: (a) the queried size plus a 4 KB tail of a byte pattern is allocated and ws_bytes = the queried size is passed:
the tail is intact afterwards; (b) the states are the same bits as a run with a workspace 4 KB larger; (c) a call with
one byte less returns RGFM_ENOMEM and leaves the states untouched.  The guard tail is inside the allocation.

Cases: single, pair, cond, pair_grad, cond_grad under Euler and midpoint; two at 5 / 3 rows; the two FlowMatchingModel
loops.  Nets g16 (1x16x16) and g24 (3x24x24), the FlexibleRatioEstimator of test_gpu_ode.py, the synthetic
FlowMatchingModel pair; batch 5, an MC set of 7, 2 steps -- the pair case 6 steps under RGFM_GRAPH=1 and RGFM_GRAPH=0, so
that the graph-replay path (Euler, >= 4 guided steps) runs on the shared chain too.
"""
import ctypes
import functools

import pytest
import torch

from helpers import make_module
from ratio_guided_multimodal_fm_amd import _lib
from test_gpu_ode import EULER, GAMMA, MIDPOINT, _p, _stream, flex, make_raw, net, ratios, start

pytestmark = pytest.mark.gpu

ENOMEM = -2
B, N_MC, TAIL, PATTERN = 5, 7, 4096, 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


class Case:
    """One loop on fresh copies of its start state: `states`, the queried size, and call(ws, ws_bytes) -> rc."""

    def __init__(self, states, query, call, keep=()):
        self.states, self.call, self.keep = states, call, keep
        nb = ctypes.c_size_t()
        assert query(ctypes.byref(nb)) == 0
        self.bytes = nb.value


def ode_case(kind, solver, steps, dev):
    if kind == "cond_grad":  # (test_gpu_ode's case has its own batch of 3: here batch 5, the 3x24x24 side observed)
        rr, tnet, s = flex().to(dev), net("g16").to(dev), start("g16", B).to(dev).clone()
        ctx = rr._engine.cond_prepare(start("g24", B, salt=3).to(dev), "y", tuple(s.shape[1:]))
        rr._engine._bind_target(1, s)
        h, hr = tnet._engine.handle(dev), rr._engine.handle(dev)
        ws_args, args, states, keep = (h, hr, 1, B), (h, hr, _p(s), _p(ctx), 1, B, steps, GAMMA), [s], (ctx,)
    else:
        r = make_raw(kind, B, dev, steps)
        ws_args, args, states, keep = r.ws_args, r.args, r.state, (r,)
    L = _lib.lib()
    return Case(states, lambda out: getattr(L, f"rgfm_sample_{kind}_ode_workspace_bytes")(*ws_args, solver, out),
                lambda ws, nb: getattr(L, f"rgfm_sample_{kind}_ode")(*args, 0, steps, solver, _p(ws), nb, _stream()), keep)


def two_case(solver, steps, dev):
    hx, hy = net("g16").to(dev)._engine.handle(dev), net("g24").to(dev)._engine.handle(dev)
    x, y = start("g16", 5).to(dev).clone(), start("g24", 3).to(dev).clone()
    L = _lib.lib()
    return Case([x, y], lambda out: L.rgfm_sample_two_workspace_bytes(hx, hy, 5, 3, solver, out),
                lambda ws, nb: L.rgfm_sample_two(hx, hy, _p(x), _p(y), 5, 3, steps, 0, steps, solver, _p(ws), nb, _stream()))


@functools.lru_cache(maxsize=None)
def fm_module(tag, dev):
    """The synthetic FlowMatchingModel of tests/helpers.py on the device (kept: its engine owns the native handle)."""
    return make_module(tag, dev)


def fm_start(salt, n, dev):
    return torch.randn(n, 1, 28, 28, generator=torch.Generator().manual_seed(8100 + salt)).to(dev)


def fmnet_case(kind, steps, dev):
    L = _lib.lib()
    hx = fm_module("fm_original", dev)._engine.handle(dev)
    x = fm_start(0, B, dev)
    if kind == "single":
        return Case([x], lambda out: L.rgfm_fmnet_workspace_bytes(hx, B, out),
                    lambda ws, nb: L.rgfm_fmnet_sample_single(hx, _p(x), B, steps, 0, steps, _p(ws), nb, _stream()))
    hy = fm_module("fm_original_y", dev)._engine.handle(dev)
    y, mx, my, r = fm_start(1, B, dev), 0.5 * fm_start(2, N_MC, dev), 0.5 * fm_start(3, N_MC, dev), ratios(N_MC).to(dev)
    return Case([x, y], lambda out: L.rgfm_fmnet_sample_pair_workspace_bytes(hx, hy, B, N_MC, out),
                lambda ws, nb: L.rgfm_fmnet_sample_pair(hx, hy, _p(x), _p(y), _p(mx), _p(my), _p(r), N_MC, B, steps, GAMMA,
                                                        0, steps, _p(ws), nb, _stream()), (mx, my, r))


def check(make, dev):
    exact, roomy, short = make(), make(), make()
    nb = exact.bytes
    assert nb > 0 and roomy.bytes == nb and short.bytes == nb
    ws = torch.full((nb + TAIL,), PATTERN, dtype=torch.uint8, device=dev)
    assert exact.call(ws, nb) == 0
    torch.cuda.synchronize()
    assert bool((ws[nb:] == PATTERN).all()), "the call wrote past the size its own query returned"
    assert roomy.call(torch.empty(nb + TAIL, dtype=torch.uint8, device=dev), nb + TAIL) == 0
    torch.cuda.synchronize()
    for a, b in zip(exact.states, roomy.states):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    before = [s.clone() for s in short.states]
    assert not any(torch.equal(a, b) for a, b in zip(exact.states, before))  # (the loop moved its state)
    assert short.call(torch.empty(nb, dtype=torch.uint8, device=dev), nb - 1) == ENOMEM
    torch.cuda.synchronize()
    for a, b in zip(short.states, before):
        assert torch.equal(a, b)


@pytest.mark.parametrize("solver", [EULER, MIDPOINT])
@pytest.mark.parametrize("kind", ["single", "cond", "pair_grad", "cond_grad"])
def test_loop_stays_inside_its_queried_workspace(dev, kind, solver):
    check(lambda: ode_case(kind, solver, 2, dev), dev)


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("solver", [EULER, MIDPOINT])
def test_pair_stays_inside_its_queried_workspace(dev, monkeypatch, solver, graph):
    monkeypatch.setenv("RGFM_GRAPH", graph)
    check(lambda: ode_case("pair", solver, 6, dev), dev)


@pytest.mark.parametrize("solver", [EULER, MIDPOINT])
def test_two_stays_inside_its_queried_workspace(dev, solver):
    check(lambda: two_case(solver, 2, dev), dev)
    # the sum of the two single sizes (the second chain starts where the first one's single-loop layout ends)
    L, nb = _lib.lib(), [ctypes.c_size_t() for _ in range(3)]
    hx, hy = net("g16").to(dev)._engine.handle(dev), net("g24").to(dev)._engine.handle(dev)
    assert L.rgfm_sample_two_workspace_bytes(hx, hy, 5, 3, solver, ctypes.byref(nb[0])) == 0
    assert L.rgfm_sample_single_ode_workspace_bytes(hx, 5, solver, ctypes.byref(nb[1])) == 0
    assert L.rgfm_sample_single_ode_workspace_bytes(hy, 3, solver, ctypes.byref(nb[2])) == 0
    assert nb[0].value == nb[1].value + nb[2].value


@pytest.mark.parametrize("kind", ["single", "pair"])
def test_fmnet_loop_stays_inside_its_queried_workspace(dev, kind):
    check(lambda: fmnet_case(kind, 2, dev), dev)
