"""Case table and harness of the stream contract: every export of include/rgfm.h that takes an rgfm_stream_t is
"ordered with respect to `stream` on entry and on return".  Importable without a GPU (tests/test_stream_cases_cpu.py
reads the table; tests/test_gpu_streams.py runs it).

A case (one row of CASES) names the exports it drives and holds two functions:

    draws(d)          the tensors the CALLER writes (inputs, and state the call updates in place), drawn on the CPU from
                      the seeded Draw `d`.  Draw 0 holds the real values, draw 1 the POISON: a second draw of the same
                      distribution and scale -- finite and inside the fp16 window of the default conv path, so no range
                      flag can rise and no NaN can mask a comparison.
    build(dev, vals)  uploads `vals` (one of the two draws) and returns a Built: `targets` (name -> the device tensor the
                      caller writes), `state` (tensors the call updates in place), `call` (makes the call on the current
                      stream and returns the tuple of its output tensors).

The calls are the package's own entry points (_engine, the modules, utils.optim.Adam) and, for the Euler entry points
that the Python layer no longer routes through, the raw ctypes callers of tests/test_gpu_ode.py; both name
torch.cuda.current_stream(), so they follow a stream context as they are.

late_stream_run builds a case on POISON, synchronises the device, and then on a fresh non-blocking stream enqueues a
delay kernel, copies the real values over the poison, makes the call and clones every output and state tensor -- with no
host synchronisation anywhere in between.  While the host enqueues the call the device still sits in the delay, so

  * a launch, copy or memset of the call that is not ordered behind the caller's stream on ENTRY (wrong stream, a fork
    without its edge, a wait on a stale event) reads the poison, and
  * a call whose work is not joined back on RETURN is cloned before it has run;

either way the clones differ from the null-stream run of the same case, which test_gpu_streams.py requires to be
torch.equal.

The delay.  torch.cuda._sleep(cycles), never a fixed cycle count: `cycles_per_ms` times one _sleep of 2^24 cycles with
two timing events, once per session (after a warm-up launch), and `delay_cycles(ms)` converts.  The rule for the
length: twice the wall time of the same call on the null stream -- enqueue plus torch.cuda.synchronize(), measured in
the same test on warmed handles (null_stream_run returns it) -- with a floor of 20 ms.  That wall time is an upper bound
of the host's enqueue time, which is all the delay has to outlast.  A call that does not synchronise must return while
the delay is still running: LateRun.delay_pending is the `query()` of an event recorded right behind the delay kernel,
read when the call returns; a run whose delay ended early has shown nothing and the test fails it by name.

Test hooks without a stream argument (rgfm_*_dropout_mask, rgfm_*_pool_choice, rgfm_clf_gate, ...) are documented as
null-stream calls and take no rgfm_stream_t: they need no entry here.  EXEMPT lists the stream-taking exports without a
case, each with its reason.
"""
import collections
import ctypes
import functools
import re
import time
import zlib

import torch

import test_gpu_ode as T
from helpers import GENERIC_UNETS, make_module
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.models.classifier import MNISTClassifier
from ratio_guided_multimodal_fm_amd.synth import synth_state_dict
from ratio_guided_multimodal_fm_amd.utils.optim import Adam

ROWS, STEPS, N_MC, GAMMA = 3, 4, 5, 0.7
SOLVERS = ("euler", "midpoint")
FP16_WINDOW = 2048.0  # |activation| bound of the two-plane fp16 convs (_engine.py, "range guard")
DELAY_FLOOR_MS = 20.0

# stream-taking exports without a case
EXEMPT = {
    "rgfm_unet_create": "synchronises `stream` by contract (the blob may be freed on return)",
    "rgfm_ratio_create": "synchronises `stream` by contract, as rgfm_unet_create",
    "rgfm_ratio_flex_create": "synchronises `stream` by contract, as rgfm_unet_create",
    "rgfm_fmnet_create": "synchronises `stream` by contract, as rgfm_unet_create",
    "rgfm_clf_create": "synchronises `stream` by contract, as rgfm_unet_create",
    "rgfm_unet_range_flag": "waits for `stream` by contract: it is the range guard's read-back",
    "rgfm_fmnet_range_flag": "waits for `stream` by contract: it is the range guard's read-back",
}


def stream_exports(header_text):
    """Names of the exports of include/rgfm.h whose parameter list has an rgfm_stream_t, in the header's order."""
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return [m.group(1) for m in re.finditer(r"\b(rgfm_\w+)\s*\(([^;{}()]*)\)\s*;", text)
            if "rgfm_stream_t" in m.group(2)]


class Draw:
    """Seeded CPU draws of one case: `which` 0 = the real values, 1 = the poison."""

    def __init__(self, case_id, which):
        self.which = which
        self.g = torch.Generator().manual_seed(2 * zlib.crc32(case_id.encode()) + which)

    def normal(self, *shape, scale=1.0):
        return scale * torch.randn(*shape, generator=self.g)

    def ratios(self, *shape):
        return torch.exp(0.5 * torch.randn(*shape, generator=self.g))

    def uniform(self, *shape, lo=0.0, hi=1.0):
        return lo + (hi - lo) * torch.rand(*shape, generator=self.g)

    def labels(self, n, classes):
        return torch.randint(0, classes, (n,), generator=self.g)


Built = collections.namedtuple("Built", "targets state call")
LateRun = collections.namedtuple("LateRun", "clones delay_pending delay_ms")


class Case:
    """kind: 'raw' -- a C ABI call, never synchronises; 'plain' -- a Python entry point outside the range guard, never
    synchronises; 'guarded' -- a Python entry point under _range_guarded: synchronises at its end unless
    RGFM_RANGE_CHECK=0 (or RGFM_CONV names another arithmetic), so it runs with the guard on and off; 'syncs' -- the
    call synchronises `stream` by contract (update_params of the U-Net, ratio and FlowMatchingModel handles).
    forks: the case runs with RGFM_OVERLAP 1 and 0 -- the calls that fork a library-owned side stream (the paired loops,
    rgfm_sample_two, the ratio estimator's two encoders) and, with them, every other sampler loop.
    fresh(dev, vals): for the update_params cases, the outputs of a newly built module that was loaded with the real
    weights."""

    def __init__(self, id, exports, draws, build, kind="plain", forks=False, fresh=None):
        assert kind in ("raw", "plain", "guarded", "syncs")
        self.id, self.exports, self._draws, self.build = id, tuple(exports), draws, build
        self.kind, self.forks, self.fresh = kind, forks, fresh

    def draw(self, which):
        return self._draws(Draw(self.id, which))

    def __repr__(self):
        return f"Case({self.id})"


# ------------------------------------------------------------------ the harness
_cycles_per_ms = None


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond on this device: one timed _sleep, once per session."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        n = 1 << 24
        torch.cuda._sleep(1 << 16)  # (the first launch loads the kernel)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, f"torch.cuda._sleep({n}) took {ms} ms: the delay kernel cannot be calibrated"
        _cycles_per_ms = n / ms
    return _cycles_per_ms


def delay_cycles(ms):
    return int(ms * cycles_per_ms())


def delay_for(wall_ms):
    """The rule: twice the null-stream wall time of the call, at least DELAY_FLOOR_MS."""
    return max(2.0 * wall_ms, DELAY_FLOOR_MS)


def _upload(vals, dev):
    return {k: v.to(dev) for k, v in vals.items()}


def _clones(outs, built):
    return [t.clone() for t in (*outs, *built.state) if t is not None]


def null_stream_run(case, dev):
    """The case on the null stream with full synchronisation: (clones of its outputs and state, wall time in ms of the
    call -- enqueue plus synchronize)."""
    real = case.draw(0)
    built = case.build(dev, real)
    src = _upload(real, dev)
    for k, t in built.targets.items():  # (the same writes as the late run makes: the real values over themselves)
        t.copy_(src[k])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = built.call()
    torch.cuda.synchronize()
    wall_ms = 1e3 * (time.perf_counter() - t0)
    clones = _clones(outs, built)
    torch.cuda.synchronize()
    return clones, wall_ms


def late_stream_run(case, dev, delay_ms=DELAY_FLOOR_MS, stream=None):
    """The case on a caller's stream that is still busy when the call is enqueued (module docstring): a LateRun with the
    clones of every output and state tensor, taken on that stream right behind the call.  `stream`: run on this stream
    instead of a fresh one."""
    real, poison = case.draw(0), case.draw(1)
    built = case.build(dev, poison)
    src = _upload(real, dev)
    cycles = delay_cycles(delay_ms)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev) if stream is None else stream
    behind_delay = torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        behind_delay.record()
        for k, t in built.targets.items():
            t.copy_(src[k], non_blocking=True)
        outs = built.call()
        pending = not behind_delay.query()
        clones = _clones(outs, built)
    s.synchronize()
    return LateRun(clones, pending, delay_ms)


# ------------------------------------------------------------------ modules (built once, moved to the device on use)
def unet(tag, dev):
    return T.net(tag).to(dev)


@functools.lru_cache(maxsize=None)
def _module(tag):
    return make_module(tag)


def module(tag, dev):
    return _module(tag).to(dev)


def flex(dev):
    """FlexibleRatioEstimator for x = 1x16x16 (g16) and y = 3x24x24 (g24), bound to that pair."""
    rr = T.flex().to(dev)
    rr._engine.bind(torch.empty(0, 1, 16, 16, device="meta"), torch.empty(0, 3, 24, 24, device="meta"))
    return rr


SX, SY = (1, 16, 16), (3, 24, 24)  # image shapes of "g16" and "g24"
FM = (1, 28, 28)                   # FlowMatchingModel, RatioEstimator


def n_stages(solver):
    return STEPS * (2 if solver == "midpoint" else 1)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


CASES = []


def case(id, exports, draws, kind="plain", forks=False, fresh=None):
    def add(build):
        CASES.append(Case(id, exports, draws, build, kind, forks, fresh))
        return build
    return add


def simple(fn, state=()):
    """A build function for the common form: upload everything, `fn(dev, t)` is the call, `state` names the in-place
    tensors."""
    def build(dev, vals):
        t = _upload(vals, dev)
        return Built(t, [t[k] for k in state], lambda: fn(dev, t))
    return build


def _tup(v):
    if v is None:
        return ()
    return tuple(v) if isinstance(v, (tuple, list)) else (v,)


# ------------------------------------------------------------------ forwards
def _xt(shape):
    return lambda d: {"x": d.normal(ROWS, *shape), "t": d.uniform(ROWS, hi=0.99)}


case("unet_forward", ["rgfm_unet_forward"], _xt(SY), kind="guarded")(
    simple(lambda dev, t: _tup(unet("g24", dev)(t["x"], t["t"]))))
case("unet_time_embedding", ["rgfm_unet_time_embedding"], lambda d: {"t": d.uniform(ROWS, hi=0.99)})(
    simple(lambda dev, t: _tup(unet("g16", dev)._engine.time_embedding(t["t"]))))


def _forward_trace(dev, t):
    out, acts = unet("g16", dev)._engine.forward_trace(t["x"], t["t"])
    return (out, *acts)


case("unet_forward_trace", ["rgfm_unet_forward", "rgfm_unet_read_activation"], _xt(SX), kind="guarded")(
    simple(_forward_trace))
case("fmnet_forward", ["rgfm_fmnet_forward"], _xt(FM), kind="guarded")(
    simple(lambda dev, t: _tup(module("fm_original", dev)(t["x"], t["t"]))))


def _clf_forward(dev, t):
    with torch.no_grad():
        return _tup(module("clf_mnist28", dev).forward_train(t["x"]))


case("clf_forward", ["rgfm_clf_forward_train"], lambda d: {"x": d.normal(ROWS, *FM)})(simple(_clf_forward))


# ------------------------------------------------------------------ ratio estimator (the two encoders fork)
def _xy(d):
    return {"x": d.normal(ROWS, *SX), "y": d.normal(ROWS, *SY)}


case("ratio_eval", ["rgfm_ratio_eval"], _xy, forks=True)(
    simple(lambda dev, t: _tup(flex(dev)._engine.eval(t["x"], t["y"], "log_ratio"))))
case("ratio_eval_bn", ["rgfm_ratio_eval"], lambda d: {"x": d.normal(ROWS, 1, 32, 32), "y": d.normal(ROWS, 3, 32, 32)},
     forks=True)(simple(lambda dev, t: _tup(module("ratio_ms", dev)._engine.eval(t["x"], t["y"], "score"))))
case("ratio_eval_cross", ["rgfm_ratio_eval_cross"],
     lambda d: {"x": d.normal(ROWS, *SX), "y": d.normal(ROWS + 2, *SY)}, forks=True)(
    simple(lambda dev, t: _tup(flex(dev)._engine.eval_cross(t["x"], t["y"], "ratio"))))
case("ratio_grad_log_ratio", ["rgfm_ratio_grad_log_ratio"], _xy, forks=True)(
    simple(lambda dev, t: _tup(flex(dev)._engine.grad_log_ratio(t["x"], t["y"]))))
case("ratio_cond_prepare", ["rgfm_ratio_cond_prepare"], lambda d: {"cond": d.normal(ROWS, *SY)}, forks=True)(
    simple(lambda dev, t: _tup(flex(dev)._engine.cond_prepare(t["cond"], "y", SX))))
case("ratio_grad_log_ratio_cond", ["rgfm_ratio_grad_log_ratio_cond"],
     lambda d: {"ctx": d.normal(ROWS, T.HID), "target": d.normal(ROWS, *SX)}, forks=True)(
    simple(lambda dev, t: _tup(flex(dev)._engine.grad_log_ratio_cond(t["ctx"], "y", t["target"]))))


# ------------------------------------------------------------------ guidance blocks
def _block(d):
    return {"x": d.normal(ROWS, *SX), "y": d.normal(ROWS, *SY), "vx": d.normal(ROWS, *SX), "vy": d.normal(ROWS, *SY),
            "mx": d.normal(N_MC, *SX, scale=0.5), "my": d.normal(N_MC, *SY, scale=0.5), "r": d.ratios(N_MC),
            "R": d.ratios(N_MC, N_MC), "rows": d.ratios(ROWS, N_MC), "g": d.uniform(ROWS, hi=2.0)}


def _pick(draws, *names):
    return lambda d: {k: v for k, v in draws(d).items() if k in names}


PAIRED = ("x", "y", "vx", "vy", "mx", "my")
for rows in (False, True):
    sfx, gam = ("_rows", lambda t: t["g"]) if rows else ("", lambda t: GAMMA)
    more = ("g",) if rows else ()
    case("guidance_apply" + sfx, ["rgfm_guidance_apply" + sfx], _pick(_block, *PAIRED, "r", *more))(
        simple(lambda dev, t, gam=gam: _tup(_engine.guidance_apply(
            t["x"], t["y"], t["vx"], t["vy"], t["mx"], t["my"], t["r"], 0.5, gam(t), want_weights=True)),
            state=("vx", "vy")))
    case("guidance_apply_cond" + sfx, ["rgfm_guidance_apply_cond" + sfx], _pick(_block, "y", "vy", "my", "rows", *more))(
        simple(lambda dev, t, gam=gam: _tup(_engine.guidance_apply_cond(
            t["y"], t["vy"], t["my"], t["rows"], 0.5, gam(t), want_weights=True)), state=("vy",)))
    case("guidance_apply_cross" + sfx, ["rgfm_guidance_apply_cross" + sfx], _pick(_block, *PAIRED, "R", *more))(
        simple(lambda dev, t, gam=gam: _tup(_engine.guidance_apply_cross(
            t["x"], t["y"], t["vx"], t["vy"], t["mx"], t["my"], t["R"], 0.5, gam(t), want_weights=True)),
            state=("vx", "vy")))
case("guidance_diag", ["rgfm_guidance_diag"], _pick(_block, *PAIRED, "r"))(
    simple(lambda dev, t: _tup(_engine.guidance_diag(t["x"], t["y"], t["vx"], t["vy"], t["mx"], t["my"], t["r"], 0.5))))
case("guidance_diag_cond", ["rgfm_guidance_diag_cond"], _pick(_block, "y", "vy", "my", "rows"))(
    simple(lambda dev, t: _tup(_engine.guidance_diag_cond(t["y"], t["vy"], t["my"], t["rows"], 0.5))))
case("guidance_diag_cross", ["rgfm_guidance_diag_cross"], _pick(_block, *PAIRED, "R"))(
    simple(lambda dev, t: _tup(_engine.guidance_diag_cross(t["x"], t["y"], t["vx"], t["vy"], t["mx"], t["my"], t["R"],
                                                           0.5))))


# ------------------------------------------------------------------ sampler loops
def _loop(d):
    return {"x": d.normal(ROWS, *SX), "y": d.normal(ROWS, *SY), "mx": d.normal(N_MC, *SX, scale=0.5),
            "my": d.normal(N_MC, *SY, scale=0.5), "r": d.ratios(N_MC), "R": d.ratios(N_MC, N_MC),
            "rows": d.ratios(ROWS, N_MC), "ctx": d.normal(ROWS, T.HID), "g": d.uniform(ROWS, hi=2.0)}


def _loop_build(fn, state, diag_rows=None):
    """build of a loop: `fn(dev, t, extra)`; diag_rows = n_stages: a zeroed records tensor goes in as extra['diag'] and
    comes back as state."""
    def build(dev, vals):
        t = _upload(vals, dev)
        extra = {}
        st = [t[k] for k in state]
        if diag_rows:
            extra["diag"] = torch.zeros(diag_rows, ROWS, _lib.DIAG_FLOATS, device=dev)
            st.append(extra["diag"])

        def call():
            fn(dev, t, extra)  # (in place: what it returns is the state)
            return ()
        return Built(t, st, call)
    return build


def _strength(solver):
    return [1.0, 0.5, 0.0, 1.5, 1.0, 0.25, 2.0, 1.0][:n_stages(solver)]


def _loop_cases(solver):
    ode = solver == "midpoint"  # (the Euler loops of the Python layer run through the *_ode entry points too)
    tag = f"[{solver}]"
    ns = n_stages(solver)

    def kw(extra, gs=False, t=None):
        k = dict(solver=solver, **extra)
        if gs:
            k.update(gamma_rows=t["g"], stage_scale=_strength(solver))
        return k

    case("sample_single" + tag, ["rgfm_sample_single_ode"], _pick(_loop, "y"), kind="guarded", forks=True)(_loop_build(
        lambda dev, t, e: _engine.sample_single(unet("g24", dev), t["y"], STEPS, solver=solver), ("y",)))
    case("sample_two" + tag, ["rgfm_sample_two"], _pick(_loop, "x", "y"), kind="guarded", forks=True)(_loop_build(
        lambda dev, t, e: _engine.sample_two_streams(unet("g16", dev), t["x"], unet("g24", dev), t["y"], STEPS,
                                                                solver=solver), ("x", "y")))
    for diag, gs in ((False, False), (True, False), (False, True)):
        sfx = "_diag" if diag else "_gs" if gs else ""
        exp = (lambda stem: [f"rgfm_sample_{stem}{sfx}"]) if sfx else (lambda stem: [f"rgfm_sample_{stem}_ode"])
        more = ("g",) if gs else ()
        rows = ns if diag else None
        case(f"sample_pair{sfx}{tag}", exp("pair"), _pick(_loop, "x", "y", "mx", "my", "r", *more), kind="guarded",
             forks=True)(_loop_build(lambda dev, t, e, gs=gs: _engine.sample_pair(
                 unet("g16", dev), unet("g24", dev), t["x"], t["y"], t["mx"], t["my"], t["r"], STEPS, GAMMA,
                 **kw(e, gs, t)), ("x", "y"), rows))
        case(f"sample_cond{sfx}{tag}", exp("cond"), _pick(_loop, "y", "my", "rows", *more), kind="guarded",
             forks=True)(
            _loop_build(lambda dev, t, e, gs=gs: _engine.sample_cond(
                unet("g24", dev), t["y"], t["my"], t["rows"], STEPS, GAMMA, **kw(e, gs, t)), ("y",), rows))
        case(f"sample_pair_grad{sfx}{tag}", exp("pair_grad"), _pick(_loop, "x", "y", *more), kind="guarded", forks=True)(
            _loop_build(lambda dev, t, e, gs=gs: _engine.sample_pair_grad(
                unet("g16", dev), unet("g24", dev), flex(dev), t["x"], t["y"], STEPS, GAMMA, **kw(e, gs, t)),
                ("x", "y"), rows))
        case(f"sample_cond_grad{sfx}{tag}", exp("cond_grad"), _pick(_loop, "x", "ctx", *more), kind="guarded",
             forks=True)(
            _loop_build(lambda dev, t, e, gs=gs: _engine.sample_cond_grad(
                unet("g16", dev), flex(dev), t["x"], t["ctx"], "y", STEPS, GAMMA, **kw(e, gs, t)), ("x",), rows))
    # cross pairing: one entry point with and without records, and its strength twin
    for diag, gs in ((False, False), (True, False), (False, True)):
        sfx = "_diag" if diag else "_gs" if gs else ""
        more = ("g",) if gs else ()
        case(f"sample_pair_cross{sfx}{tag}", ["rgfm_sample_pair_cross_gs" if gs else "rgfm_sample_pair_cross"],
             _pick(_loop, "x", "y", "mx", "my", "R", *more), kind="guarded", forks=True)(
            _loop_build(lambda dev, t, e, gs=gs: _engine.sample_pair(
                unet("g16", dev), unet("g24", dev), t["x"], t["y"], t["mx"], t["my"], t["R"], STEPS, GAMMA,
                **kw(e, gs, t)), ("x", "y"), ns if diag else None))


for _solver in SOLVERS:
    _loop_cases(_solver)


# the Euler entry points without a solver argument: the raw callers of tests/test_gpu_ode.py
def _raw_build(make, state):
    def build(dev, vals):
        t = _upload(vals, dev)
        raw = make(dev, t)

        def call():
            assert raw.run(None, 0, STEPS) == 0
            return ()
        return Built(t, [t[k] for k in state], call)
    return build


def _raw_cond_grad(dev, t):
    rr, net = flex(dev), unet("g16", dev)
    h, hr = net._engine.handle(dev), rr._engine.handle(dev)
    raw = T.Raw("cond_grad", (h, hr, 1, ROWS), (h, hr, _p(t["x"]), _p(t["ctx"]), 1, ROWS, STEPS, GAMMA), [t["x"]])
    raw.keep = (t["ctx"],)
    return raw


case("raw_sample_single", ["rgfm_sample_single"], _pick(_loop, "y"), kind="raw", forks=True)(
    _raw_build(lambda dev, t: T.raw_single("g24", t["y"], STEPS, dev), ("y",)))
case("raw_sample_pair", ["rgfm_sample_pair"], _pick(_loop, "x", "y", "mx", "my", "r"), kind="raw", forks=True)(
    _raw_build(lambda dev, t: T.raw_pair(t["x"], t["y"], t["mx"], t["my"], t["r"], STEPS, GAMMA, dev), ("x", "y")))
case("raw_sample_cond", ["rgfm_sample_cond"], _pick(_loop, "y", "my", "rows"), kind="raw", forks=True)(
    _raw_build(lambda dev, t: T.raw_cond("g24", t["y"], t["my"], t["rows"], STEPS, GAMMA, dev), ("y",)))
case("raw_sample_pair_grad", ["rgfm_sample_pair_grad"], _pick(_loop, "x", "y"), kind="raw", forks=True)(
    _raw_build(lambda dev, t: T.raw_pair_grad(t["x"], t["y"], STEPS, GAMMA, dev), ("x", "y")))
case("raw_sample_cond_grad", ["rgfm_sample_cond_grad"], _pick(_loop, "x", "ctx"), kind="raw", forks=True)(
    _raw_build(_raw_cond_grad, ("x",)))


# FlowMatchingModel loops (Euler only)
def _fm_loop(d):
    return {"x": d.normal(ROWS, *FM), "y": d.normal(ROWS, *FM), "mx": d.normal(N_MC, *FM, scale=0.5),
            "my": d.normal(N_MC, *FM, scale=0.5), "r": d.ratios(N_MC)}


case("fmnet_sample_single", ["rgfm_fmnet_sample_single"], _pick(_fm_loop, "x"), kind="guarded", forks=True)(_loop_build(
    lambda dev, t, e: _engine.sample_single(module("fm_original", dev), t["x"], STEPS), ("x",)))
for _diag in (False, True):
    case("fmnet_sample_pair" + ("_diag" if _diag else ""), ["rgfm_fmnet_sample_pair" + ("_diag" if _diag else "")], _fm_loop,
         kind="guarded", forks=True)(_loop_build(lambda dev, t, e: _engine.sample_pair(
             module("fm_original", dev), module("fm_original_y", dev), t["x"], t["y"], t["mx"], t["my"], t["r"], STEPS,
             GAMMA, **e), ("x", "y"), STEPS if _diag else None))


# ------------------------------------------------------------------ likelihood
def _vjp(dev, t):
    lin = unet("g16", dev).linearize(t["x"], t["t"])
    return lin.v, lin.vjp(t["u"])


case("unet_vjp", ["rgfm_unet_forward_train", "rgfm_unet_vjp"],
     lambda d: {"x": d.normal(ROWS, *SX), "t": d.uniform(ROWS, hi=0.99), "u": d.normal(ROWS, *SX)})(simple(_vjp))
case("unet_divergence", ["rgfm_unet_divergence"],
     lambda d: {"x": d.normal(ROWS, *SX), "t": d.uniform(ROWS, hi=0.99), "eps": d.normal(2, ROWS, *SX)})(
    simple(lambda dev, t: _tup(unet("g16", dev).divergence(t["x"], t["t"], t["eps"]))))
for _solver in SOLVERS:
    case(f"unet_log_prob[{_solver}]", ["rgfm_unet_log_prob"],
         lambda d: {"x": d.normal(ROWS, *SX), "eps": d.normal(2, ROWS, *SX)})(
        simple(lambda dev, t, solver=_solver: _tup(unet("g16", dev)._engine.log_prob(t["x"], t["eps"], 3, solver))))


# ------------------------------------------------------------------ training passes (forward + backward through autograd)
def _train_call(m, inputs, loss_of):
    """Forward and backward of module `m` on the current stream: (output, input gradients, every parameter gradient)."""
    m.zero_grad(set_to_none=True)
    leaves = [v.detach().requires_grad_(True) for v in inputs]
    out = loss_of(leaves)
    out[0].backward()
    return (*[o.detach() for o in out], *[v.grad for v in leaves], *[q.grad for q in m.parameters()])


def _unet_train(dev, t):
    m = unet("g16", dev)
    return _train_call(m, [t["x"]], lambda v: [(m.forward_train(v[0], t["t"]) * t["w"]).sum()])


def _fmnet_train(dev, t):
    m = module("fm_original", dev)
    return _train_call(m, [t["x"]], lambda v: [(m.forward_train(v[0], t["t"]) * t["w"]).sum()])


def _ratio_train(dev, t):
    m = flex(dev)
    return _train_call(m, [t["x"], t["y"]], lambda v: [(m.forward_train(v[0], v[1]) * t["w"]).sum()])


def _clf_train(dev, t):
    m = module("clf_mnist28", dev)

    def loss_of(v):
        loss, pred, rows = _engine.cross_entropy(m.forward_train(v[0]), t["labels"])
        return [loss, pred, rows]
    return _train_call(m, [t["x"]], loss_of)


case("unet_train", ["rgfm_unet_forward_train", "rgfm_unet_backward"],
     lambda d: {"x": d.normal(ROWS, *SX), "t": d.uniform(ROWS, hi=0.99), "w": d.normal(ROWS, *SX)})(simple(_unet_train))
case("fmnet_train", ["rgfm_fmnet_forward_train", "rgfm_fmnet_backward"],
     lambda d: {"x": d.normal(ROWS, *FM), "t": d.uniform(ROWS, hi=0.99), "w": d.normal(ROWS, *FM)})(simple(_fmnet_train))
case("ratio_train", ["rgfm_ratio_forward_train", "rgfm_ratio_backward"],
     lambda d: {"x": d.normal(ROWS, *SX), "y": d.normal(ROWS, *SY), "w": d.normal(ROWS)})(simple(_ratio_train))
case("clf_train", ["rgfm_clf_forward_train", "rgfm_clf_backward", "rgfm_clf_xent"],
     lambda d: {"x": d.normal(ROWS, *FM), "labels": d.labels(ROWS, 10)})(simple(_clf_train))


# ------------------------------------------------------------------ the optimizer step
ADAM_SIZES = (1025, 5, 257)  # (more than one 1024-float chunk; tiny; no multiple of 4)


def _adam_draws(d):
    out = {}
    for i, n in enumerate(ADAM_SIZES):
        out[f"p{i}"], out[f"g{i}"], out[f"ema{i}"] = d.normal(n), d.normal(n), d.normal(n)
        out[f"m{i}"], out[f"v{i}"] = d.normal(n, scale=0.1), d.uniform(n, hi=0.1)
    return out


@case("adam_step", ["rgfm_adam_grad_norm", "rgfm_adam_step"], _adam_draws)
def _adam_build(dev, vals):
    t = _upload(vals, dev)
    params = [torch.nn.Parameter(t[f"p{i}"]) for i in range(len(ADAM_SIZES))]
    for i, q in enumerate(params):
        q.grad = t[f"g{i}"]
    opt = Adam(params, lr=1e-2, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9)
    targets = dict(t)
    state = []
    for i, q in enumerate(params):  # the moments and the average are the caller's state too: written late like the rest
        st = opt.state[q]
        targets[f"m{i}"], targets[f"v{i}"], targets[f"ema{i}"] = st["exp_avg"], st["exp_avg_sq"], st["ema"]
        state += [q.detach(), st["exp_avg"], st["exp_avg_sq"], st["ema"]]

    opt.step()  # (a first step allocates the pinned table slot and the norm; every value it moved is written again late)

    def call():
        opt.step()
        return (opt.grad_norm,)
    return Built(targets, state, call)


# ------------------------------------------------------------------ update_params: the weights are written late
def _update_case(id, export, ctor, inputs, forward, kind="syncs"):
    """`ctor()`: a new module of the family; the real / poison weights are two draws of the synthetic-weight recipe.
    The handle is created by a first forward under the weights the build was given; the
    late write moves the parameters' version counters, so the next forward re-packs the handle in place
    (rgfm_<family>_update_params) on the caller's stream."""
    def draws(d):
        sd = synth_state_dict(ctor(), 900 + d.which)
        out = {f"w{i}": v for i, v in enumerate(sd.values()) if v.is_floating_point()}
        out.update(inputs(d))
        return out

    def load(dev, vals):
        m = ctor().eval()
        sd = m.state_dict()
        ws = [v for k, v in vals.items() if k.startswith("w")]
        m.load_state_dict({k: (ws.pop(0) if v.is_floating_point() else v) for k, v in sd.items()})
        return m.to(dev)

    def build(dev, vals):
        m = load(dev, vals)
        t = _upload({k: v for k, v in vals.items() if not k.startswith("w")}, dev)
        forward(m, t)  # creates the handle (under the weights of this build)
        targets = dict(t)
        floats = [v for v in m.state_dict(keep_vars=True).values() if v.is_floating_point()]
        targets.update({f"w{i}": v.detach() for i, v in enumerate(floats)})  # (detach() shares the version counter)
        return Built(targets, [], lambda: _tup(forward(m, t)))

    def fresh(dev, vals):
        m = load(dev, vals)
        return _tup(forward(m, _upload({k: v for k, v in vals.items() if not k.startswith("w")}, dev)))
    CASES.append(Case(id, [export], draws, build, kind=kind, fresh=fresh))


def _clf_eval_forward(m, t):
    with torch.no_grad():
        return m.forward_train(t["x"])


_update_case("unet_update_params", "rgfm_unet_update_params", lambda: M.FlexibleUNet(**GENERIC_UNETS["g16"]),
             _xt(SX), lambda m, t: m(t["x"], t["t"]))
_update_case("fmnet_update_params", "rgfm_fmnet_update_params", lambda: M.FlowMatchingModel(),
             _xt(FM), lambda m, t: m(t["x"], t["t"]))
_update_case("ratio_update_params", "rgfm_ratio_update_params", lambda: M.RatioEstimator(64, 128),
             lambda d: {"x": d.normal(ROWS, *FM), "y": d.normal(ROWS, *FM)}, lambda m, t: m(t["x"], t["y"]))
_update_case("clf_update_params", "rgfm_clf_update_params", lambda: MNISTClassifier(),
             lambda d: {"x": d.normal(ROWS, *FM)}, _clf_eval_forward, kind="plain")
# (the classifier's re-pack is one asynchronous copy: it does not synchronise)

BY_ID = {c.id: c for c in CASES}
