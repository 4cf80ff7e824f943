"""Every stream-taking entry point on a caller's stream that is not the null stream (tests/stream_cases.py).

A. controls of the harness itself (pure torch): a missing entry edge IS seen.
B/C. every case of the table, bitwise: the null-stream run against late_stream_run, with the range guard on and off for
     the guarded Python entry points and RGFM_OVERLAP 1 and 0 for the calls that fork a side stream and every sampler loop.
D. graph replay (RGFM_GRAPH=1) captured directly on a caller's stream, twice on the same stream.
E. one engine (one workspace) on two streams with no host synchronisation in between.
"""
import copy
import time

import pytest
import torch

import stream_cases as S
from ratio_guided_multimodal_fm_amd import _engine, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def set_env(monkeypatch, guard=None, overlap=None, **more):
    for k in ("RGFM_RANGE_CHECK", "RGFM_OVERLAP", "RGFM_CONV", "RGFM_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    if guard == "off":
        monkeypatch.setenv("RGFM_RANGE_CHECK", "0")
    if overlap is not None:
        monkeypatch.setenv("RGFM_OVERLAP", str(overlap))
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def assert_same(got, want, what):
    assert len(got) == len(want) and len(got) > 0, what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        assert torch.equal(a, b), f"{what}: tensor {i} of {len(got)} differs from the null-stream run"


def assert_delay_outlasted_the_call(run, what):
    assert run.delay_pending, (f"{what}: the delay kernel ({run.delay_ms:.1f} ms) had ended when the call returned -- "
                               "either the call synchronised, or the delay was too short: this run has shown nothing")


# ------------------------------------------------------------------ A. the harness can fail
def _control(dev, second_stream_waits):
    """Poison -> (delay, copy of the real values) on stream 1; a clone on stream 1 and a clone on stream 2."""
    g = torch.Generator().manual_seed(1)
    real, poison = torch.randn(4096, generator=g).to(dev), torch.randn(4096, generator=g).to(dev)
    buf = poison.clone()
    cycles = S.delay_cycles(S.DELAY_FLOOR_MS)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        torch.cuda._sleep(cycles)
        buf.copy_(real, non_blocking=True)
        same = buf.clone()
    if second_stream_waits:
        s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        other = buf.clone()
    s2.synchronize()
    s1.synchronize()
    return real, poison, same, other


def test_control_a_second_stream_that_does_not_wait_reads_the_poison(dev):
    """The device has fewer hardware queues than the process has streams, and two streams that share a queue run in
    order without any edge between them: such a pair cannot show a missing wait (and hides none that matters).  So
    the control takes fresh stream pairs, at most 8, until one does not share a queue; every pair's same-stream clone
    must hold the real values, and a second stream never holds anything but the poison or the real values."""
    seen = []
    for _ in range(8):
        real, poison, same, other = _control(dev, second_stream_waits=False)
        assert torch.equal(same, real)
        assert torch.equal(other, poison) or torch.equal(other, real)
        seen.append(torch.equal(other, poison))
        if seen[-1]:
            break
    assert seen[-1], f"no second stream out of {len(seen)} read the poison: the harness cannot see a missing entry edge"


def test_control_the_same_stream_and_a_waiting_stream_read_the_real_values(dev):
    real, _, same, other = _control(dev, second_stream_waits=True)
    assert torch.equal(same, real) and torch.equal(other, real)


# ------------------------------------------------------------------ B / C. every case, bitwise
def cells():
    out = []
    for c in S.CASES:
        for guard in (("on", "off") if c.kind == "guarded" else (None,)):
            for overlap in ((1, 0) if c.forks else (None,)):
                name = c.id + (f"-guard_{guard}" if guard else "") + (f"-overlap{overlap}" if overlap is not None else "")
                out.append(pytest.param(c.id, guard, overlap, id=name))
    return out


@pytest.mark.parametrize("cid,guard,overlap", cells())
def test_case_on_a_late_stream_is_the_null_stream_run_bitwise(dev, monkeypatch, cid, guard, overlap):
    case = S.BY_ID[cid]
    set_env(monkeypatch, guard, overlap)
    warm, _ = S.null_stream_run(case, dev)       # creates and warms the handles and workspaces
    want, wall_ms = S.null_stream_run(case, dev)
    assert_same(want, warm, f"{cid}: two null-stream runs")
    run = S.late_stream_run(case, dev, S.delay_for(wall_ms))
    print(f"{cid}: null-stream call {wall_ms:.2f} ms, delay {run.delay_ms:.1f} ms, pending at return: {run.delay_pending}")
    if case.kind in ("raw", "plain") or guard == "off":  # the call does not synchronise
        assert_delay_outlasted_the_call(run, cid)
    assert_same(run.clones, want, cid)
    if case.fresh is not None:  # update_params: as a newly built module with the same weights
        fresh = [t.clone() for t in case.fresh(dev, case.draw(0))]
        torch.cuda.synchronize()
        assert_same(run.clones, fresh, f"{cid} against a fresh module")


# ------------------------------------------------------------------ D. graph replay on a caller's stream
def test_graph_replay_on_a_callers_stream_twice(dev, monkeypatch):
    """sample_pair, 4 Euler steps (ns >= 4: the guided step is captured), RGFM_GRAPH=1: the capture happens directly on
    the caller's stream with the side stream pulled in.  Bit-equal to the eager null-stream run; the second call on the
    same stream releases the first call's graph behind graph_done."""
    case = S.BY_ID["sample_pair[euler]"]
    set_env(monkeypatch, guard="off")
    S.null_stream_run(case, dev)
    want, wall_ms = S.null_stream_run(case, dev)  # eager
    set_env(monkeypatch, guard="off", RGFM_GRAPH="1")
    s = torch.cuda.Stream(dev)
    for n in (1, 2):
        run = S.late_stream_run(case, dev, S.delay_for(wall_ms), stream=s)
        assert_delay_outlasted_the_call(run, f"graph replay, call {n}")
        assert_same(run.clones, want, f"graph replay, call {n}")
    set_env(monkeypatch)
    assert not torch.equal(want[0], case.draw(0)["x"].to(dev))  # (the loop moved the state)


# ------------------------------------------------------------------ E. one engine, two streams, no host synchronisation
def _forward(m, x, t):
    return lambda: (m(x, t),)


def _two_streams(dev, call_a, call_b, wall_ms):
    """Stream A: delay, call_a, event; stream B: call_b at once, event.  Returns (clones of a, clones of b, eA, eB)."""
    cycles = S.delay_cycles(S.delay_for(wall_ms))
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    behind_delay = torch.cuda.Event()
    with torch.cuda.stream(sa):
        torch.cuda._sleep(cycles)
        behind_delay.record()
        a = [t.clone() for t in call_a()]
        ea.record()
    with torch.cuda.stream(sb):
        b = [t.clone() for t in call_b()]
        eb.record()
    pending = not behind_delay.query()
    sa.synchronize()
    sb.synchronize()
    assert pending, ("two streams: the delay on stream A had ended before both calls were enqueued: this run has shown "
                     "nothing")
    return a, b, ea, eb


def _serial(dev, call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [t.clone() for t in call()]
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def _uploads_then(dev, case):
    """The case built ahead (its inputs uploaded on the null stream); the returned call only makes the call."""
    built = case.build(dev, case.draw(0))

    def call():
        built.call()
        return built.state
    return call


E_ENVS = {"range_check_0": dict(guard="off"), "conv_bx3": dict(RGFM_CONV="bx3")}


@pytest.mark.parametrize("env", list(E_ENVS))
@pytest.mark.parametrize("combo", ["same_forward", "pair_and_cond", "grow"])
def test_one_engine_two_streams_without_host_synchronisation(dev, monkeypatch, env, combo):
    set_env(monkeypatch, **E_ENVS[env])
    g = torch.Generator().manual_seed(77)
    shape = S.SX
    if combo == "pair_and_cond":
        pair, cond = S.BY_ID["sample_pair[euler]"], S.BY_ID["sample_cond[euler]"]
        serial = lambda c: _serial(dev, _uploads_then(dev, c))  # noqa: E731
        serial(pair), serial(cond)  # warm
        (want_a, wall_ms), (want_b, _) = serial(pair), serial(cond)
        call_a, call_b = _uploads_then(dev, pair), _uploads_then(dev, cond)
        assert _engine._sampler_ws.buf is not None
    else:
        big = 40 if combo == "grow" else S.ROWS
        xa, ta = torch.randn(S.ROWS, *shape, generator=g).to(dev), torch.rand(S.ROWS, generator=g).to(dev)
        xb, tb = torch.randn(big, *shape, generator=g).to(dev), torch.rand(big, generator=g).to(dev)
        base = S.unet("g16", dev)
        _serial(dev, _forward(base, xa, ta))
        (want_a, wall_ms), (want_b, _) = _serial(dev, _forward(base, xa, ta)), _serial(dev, _forward(base, xb, tb))
        m = base
        if combo == "grow":  # a module of its own, whose workspace has seen the small batch only
            m = copy.deepcopy(base)
            _serial(dev, _forward(m, xa, ta))
            assert m._engine is not base._engine
        before = m._engine._ws.buf
        call_a, call_b = _forward(m, xa, ta), _forward(m, xb, tb)
    got_a, got_b, ea, eb = _two_streams(dev, call_a, call_b, wall_ms)
    if combo == "grow":
        assert m._engine._ws.buf is not before and m._engine._ws.buf.numel() > before.numel()
    assert_same(got_a, want_a, f"{combo}: the call on stream A")
    assert_same(got_b, want_b, f"{combo}: the call on stream B")
    # structural: B took the workspace behind A, so B's event cannot complete before A's
    assert ea.elapsed_time(eb) >= 0.0, (combo, ea.elapsed_time(eb))


def test_a_caller_on_one_stream_waits_for_nothing(dev, monkeypatch):
    """The workspace's cross-stream wait is for a change of stream only: calls that stay on one stream enqueue no wait."""
    set_env(monkeypatch, guard="off")
    m = S.unet("g16", dev)
    g = torch.Generator().manual_seed(78)
    x, t = torch.randn(S.ROWS, *S.SX, generator=g).to(dev), torch.rand(S.ROWS, generator=g).to(dev)
    s = torch.cuda.Stream(dev)
    waits = []
    monkeypatch.setattr(torch.cuda.Stream, "wait_stream", lambda self, other: waits.append((self, other)))
    with torch.cuda.stream(s):
        m(x, t)       # (the stream changed: this one may wait)
        waits.clear()
        m(x, t)
        m(x, t)
    s.synchronize()
    assert waits == []
