"""Scheduling of the two-net unguided entry (sample_two_streams -> rgfm_sample_two: the MC pre-phase) changes no bits.

The chains are enqueued step by step and the lighter one is paced by the heavier (RGFM_PREPHASE_PRIO=0: one whole
chain after the other, unpaced).  Each chain enqueues the launches of sample_single, so every
comparison is torch.equal against sample_single of each net alone on the same noise.  Nets: the synthetic MNIST32 and
SVHN presets (conv work 1 : 2.8 per row); rows 5 / 3 (unequal), 1 and 33 (one row; more than a 32-row tile), 1 to 4 steps.
"""
import functools

import pytest
import torch

from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth

pytestmark = pytest.mark.gpu

SHAPES = {"mnist": (1, 32, 32), "svhn": (3, 32, 32)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def net(tag):
    m = load_synth(M.FlowMatchingUNetMNIST(32), 13) if tag == "mnist" else load_synth(M.FlowMatchingUNetSVHN(), 14)
    return m.eval().to("cuda:0")


@functools.lru_cache(maxsize=None)
def noise(tag, rows):
    """Seeded N(0, 1) start state (CPU): shared, never modified."""
    return torch.randn(rows, *SHAPES[tag], generator=torch.Generator().manual_seed(9100 + 10 * rows + len(tag)))


@functools.lru_cache(maxsize=None)
def alone(tag, rows, steps, solver="euler"):
    """sample_single of one net alone: the reference of every test below (computed once, never modified)."""
    x = noise(tag, rows).to("cuda:0", copy=True)
    _engine.sample_single(net(tag), x, steps, solver=solver)
    torch.cuda.synchronize()
    return x


def two(tag_x, rows_x, tag_y, rows_y, steps, solver="euler"):
    x, y = noise(tag_x, rows_x).to("cuda:0", copy=True), noise(tag_y, rows_y).to("cuda:0", copy=True)
    _engine.sample_two_streams(net(tag_x), x, net(tag_y), y, steps, solver=solver)
    torch.cuda.synchronize()
    return x, y


def check(tag_x, rows_x, tag_y, rows_y, steps, solver="euler"):
    x, y = two(tag_x, rows_x, tag_y, rows_y, steps, solver)
    assert torch.equal(x, alone(tag_x, rows_x, steps, solver))
    assert torch.equal(y, alone(tag_y, rows_y, steps, solver))


@pytest.mark.parametrize("switch", [None, "0"])
def test_two_nets_are_two_single_calls(dev, monkeypatch, switch):
    """5 rows of MNIST32 beside 3 rows of SVHN, 4 Euler steps: the new schedule and the switch off."""
    if switch is None:
        monkeypatch.delenv("RGFM_PREPHASE_PRIO", raising=False)
    else:
        monkeypatch.setenv("RGFM_PREPHASE_PRIO", switch)
    check("mnist", 5, "svhn", 3, 4)


@pytest.mark.parametrize("switch", [None, "0"])
def test_heavier_net_first_or_second(dev, monkeypatch, switch):
    """The nets swapped: which chain is the long one comes from the descriptors, not from the argument position."""
    if switch is not None:
        monkeypatch.setenv("RGFM_PREPHASE_PRIO", switch)
    check("svhn", 5, "mnist", 3, 4)
    # rows decide too: 33 rows of the light net are more work per step than one row of the heavy net
    check("mnist", 33, "svhn", 1, 3)


def test_same_net_on_both_sides(dev):
    """Equal work: no pacing, both chains of ONE handle side by side (two workspaces), nothing waits for ever."""
    x, y = noise("mnist", 5).to(dev, copy=True), noise("mnist", 3).to(dev, copy=True)
    _engine.sample_two_streams(net("mnist"), x, net("mnist"), y, 4)
    torch.cuda.synchronize()
    assert torch.equal(x, alone("mnist", 5, 4)) and torch.equal(y, alone("mnist", 3, 4))


@pytest.mark.parametrize("rows", [1, 33])
def test_rows_around_the_tile_and_few_steps(dev, rows):
    """One row and 33 rows per net at 3 steps; one step only: the short chain never waits on a step that does not exist."""
    check("mnist", rows, "svhn", rows, 3)
    check("mnist", rows, "svhn", rows, 1)


def test_midpoint(dev):
    check("mnist", 5, "svhn", 3, 3, solver="midpoint")


def test_caller_stream_is_joined(dev):
    """Work enqueued on the caller's stream right after the call sees both results (no synchronisation in between)."""
    side = torch.cuda.Stream(dev)
    x, y = noise("mnist", 5).to(dev, copy=True), noise("svhn", 3).to(dev, copy=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _engine.sample_two_streams(net("mnist"), x, net("svhn"), y, 4)
        cx, cy = x.clone(), y.clone()
    side.synchronize()
    assert torch.equal(cx, alone("mnist", 5, 4)) and torch.equal(cy, alone("svhn", 3, 4))


def test_guided_loop_does_not_see_the_switch(dev, monkeypatch):
    """sample_pair at 4 rows, N_mc = 4, 3 steps: the same bits with the switch on and off."""
    gen = torch.Generator().manual_seed(9300)
    mx, my = 0.5 * torch.randn(4, *SHAPES["mnist"], generator=gen), 0.5 * torch.randn(4, *SHAPES["svhn"], generator=gen)
    r = torch.exp(0.5 * torch.randn(4, generator=gen))
    outs = []
    for switch in (None, "0"):
        if switch is not None:
            monkeypatch.setenv("RGFM_PREPHASE_PRIO", switch)
        x, y = noise("mnist", 4).to(dev, copy=True), noise("svhn", 4).to(dev, copy=True)
        _engine.sample_pair(net("mnist"), net("svhn"), x, y, mx.to(dev), my.to(dev), r.to(dev), 3, 0.5)
        torch.cuda.synchronize()
        outs.append((x, y))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], noise("mnist", 4).to(dev))
