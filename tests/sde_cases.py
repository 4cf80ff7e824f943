"""Raw ctypes callers of the stochastic sampler loops (rgfm_sample_*_sde) over the loops of tests/test_gpu_ode.py: shared
by tests/test_gpu_sde.py and the stream-case table (tests/stream_cases.py).  Importable without a GPU.

A RawSde wraps a test_gpu_ode.Raw (handles, state, the arguments in front of the step range) and adds what the *_sde
entry points take: (gamma_rows, stage_scale, n_stage_scale) behind gamma, (diag_out, diag_records) behind the solver,
and the `const rgfm_sde*` directly in front of the workspace.  Its workspace is the namesake's query plus
rgfm_sde_scratch_bytes when eta > 0.

The stream cases of these exports are registered from here, through stream_cases.case -- the table's own registrar --
when this module is imported: tests/test_sde_cpu.py and tests/test_gpu_sde.py import it, and pytest imports every test
module of a run before it runs a test, so tests/test_stream_cases_cpu.py finds the rows in the table and
tests/test_gpu_streams.py (collected behind test_gpu_sde.py) runs them.  A run of tests/test_stream_cases_cpu.py alone
does not import this module and reports the new exports as uncovered; tests/test_sde_cpu.py asserts the coverage itself.
"""
import ctypes

import torch

import test_gpu_ode as T
from ratio_guided_multimodal_fm_amd import _lib

EULER, MIDPOINT = 0, 1
KINDS = ("single", "pair", "pair_cross", "cond", "pair_grad", "cond_grad")
NAMESAKE = {"single": "rgfm_sample_single_ode", "pair": "rgfm_sample_pair_gs", "pair_cross": "rgfm_sample_pair_cross_gs",
            "cond": "rgfm_sample_cond_gs", "pair_grad": "rgfm_sample_pair_grad_gs", "cond_grad": "rgfm_sample_cond_grad_gs"}
N_MC = 5


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class RawSde:
    def __init__(self, kind, raw):
        self.kind, self.raw, self.L, self.state = kind, raw, raw.L, raw.state
        self.keep = getattr(raw, "keep", ())
        self.dims = [int(s[0].numel()) for s in self.state] + [0]

    def base_bytes(self, solver=EULER, diag=False):
        """The namesake's workspace query."""
        if self.kind == "pair_cross":
            fn = "rgfm_sample_pair_cross_workspace_bytes"
        elif diag and self.kind != "single":
            fn = f"rgfm_sample_{self.kind}_diag_workspace_bytes"
        else:
            fn = f"rgfm_sample_{self.kind}_ode_workspace_bytes"
        nb = ctypes.c_size_t()
        assert getattr(self.L, fn)(*self.raw.ws_args, solver, ctypes.byref(nb)) == 0
        return nb.value

    def scratch_bytes(self):
        nb = ctypes.c_size_t()
        assert self.L.rgfm_sde_scratch_bytes(self.state[0].shape[0], self.dims[0], self.dims[1], ctypes.byref(nb)) == 0
        return nb.value

    def run(self, b, e, sde=None, solver=EULER, rows=None, scale=None, diag=None, short=0, namesake=False):
        """rc of the call on steps [b, e).  sde: None -- a null pointer; (eta, seed) -- the record.  namesake: the
        entry point without the argument (rgfm_sample_single_ode / the *_gs loop).  short: bytes withheld from the
        workspace the call is told about."""
        eta_on = sde is not None and sde[0] > 0
        nb = self.base_bytes(solver, diag is not None) + (self.scratch_bytes() if eta_on else 0)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.state[0].device)
        rec = _lib.Sde(float(sde[0]), int(sde[1]) % (1 << 64)) if sde is not None else None
        more = () if namesake else (ctypes.byref(rec) if rec is not None else None,)
        tail = (*more, _p(ws), nb - short, T._stream())
        if self.kind == "single":
            fn = NAMESAKE["single"] if namesake else "rgfm_sample_single_sde"
            return getattr(self.L, fn)(*self.raw.args, b, e, solver, *tail)
        arr = (ctypes.c_double * len(scale))(*scale) if scale is not None else None
        cap = 0 if diag is None else diag.shape[0] * diag.shape[1]
        fn = NAMESAKE[self.kind] if namesake else f"rgfm_sample_{self.kind}_sde"
        return getattr(self.L, fn)(*self.raw.args, _p(rows), arr, 0 if scale is None else len(scale), b, e, solver, _p(diag), cap,
                                   *tail)


def pair_inputs(B, N, dev, cross=False):
    x, y, mx, my, r = T.pair_inputs(B, N, dev)
    if cross and N:
        r = T.ratios(N, N).to(dev)
    return x, y, mx, my, r


def make(kind, B, dev, steps=T.STEPS, gamma=T.GAMMA, n_mc=N_MC):
    """A RawSde of every loop on fresh device copies of test_gpu_ode's shared start states (guided, n_mc = 5; the
    gradient loops: the flexible estimator)."""
    if kind == "single":
        return RawSde(kind, T.raw_single("g24", T.start("g24", B).to(dev).clone(), steps, dev))
    if kind in ("pair", "pair_cross"):
        raw = T.raw_pair(*pair_inputs(B, n_mc, dev, kind == "pair_cross"), steps, gamma, dev)
        return RawSde(kind, raw)
    if kind == "cond":
        return RawSde(kind, T.raw_cond("g24", T.start("g24", B).to(dev).clone(), T.mc_set("g24", n_mc).to(dev),
                                       T.ratios(5, n_mc)[:B].contiguous().to(dev), steps, gamma, dev))
    if kind == "pair_grad":
        return RawSde(kind, T.raw_pair_grad(T.start("g16", B).to(dev).clone(), T.start("g24", B).to(dev).clone(), steps, gamma, dev))
    assert kind == "cond_grad" and B == 3  # (its own batch of 3)
    return RawSde(kind, T.raw_cond_grad("x", steps, gamma, dev))


# ------------------------------------------------------------------ the stream cases of the *_sde exports
import stream_cases as SC  # noqa: E402  (behind the callers above, which its rows use)

SDE = (0.8, 2024)  # (eta, seed)


def _sde_build(kind, make_raw, state):
    def build(dev, vals):
        t = SC._upload(vals, dev)
        raw = RawSde(kind, make_raw(dev, t))

        def call():
            assert raw.run(0, SC.STEPS, SDE) == 0
            return ()
        return SC.Built(t, [t[k] for k in state], call)
    return build


def _sde_noise(dev, t):
    out = t["out"].view(-1)
    assert _lib.lib().rgfm_sde_noise(SDE[1], 1, 3, out.numel(), _p(out), T._stream()) == 0
    return ()


def register_stream_cases():
    if "sde_noise" in SC.BY_ID:
        return
    S, G, pick, loop = SC.STEPS, SC.GAMMA, SC._pick, SC._loop
    SC.case("sde_noise", ["rgfm_sde_noise"], lambda d: {"out": d.normal(SC.ROWS, *SC.SX)}, kind="raw")(
        SC.simple(_sde_noise, state=("out",)))
    SC.case("sde_sample_single", ["rgfm_sample_single_sde"], pick(loop, "y"), kind="raw", forks=True)(
        _sde_build("single", lambda dev, t: T.raw_single("g24", t["y"], S, dev), ("y",)))
    SC.case("sde_sample_pair", ["rgfm_sample_pair_sde"], pick(loop, "x", "y", "mx", "my", "r"), kind="raw", forks=True)(
        _sde_build("pair", lambda dev, t: T.raw_pair(t["x"], t["y"], t["mx"], t["my"], t["r"], S, G, dev), ("x", "y")))
    SC.case("sde_sample_pair_cross", ["rgfm_sample_pair_cross_sde"], pick(loop, "x", "y", "mx", "my", "R"), kind="raw", forks=True)(
        _sde_build("pair_cross", lambda dev, t: T.raw_pair(t["x"], t["y"], t["mx"], t["my"], t["R"], S, G, dev), ("x", "y")))
    SC.case("sde_sample_cond", ["rgfm_sample_cond_sde"], pick(loop, "y", "my", "rows"), kind="raw", forks=True)(
        _sde_build("cond", lambda dev, t: T.raw_cond("g24", t["y"], t["my"], t["rows"], S, G, dev), ("y",)))
    SC.case("sde_sample_pair_grad", ["rgfm_sample_pair_grad_sde"], pick(loop, "x", "y"), kind="raw", forks=True)(
        _sde_build("pair_grad", lambda dev, t: T.raw_pair_grad(t["x"], t["y"], S, G, dev), ("x", "y")))
    SC.case("sde_sample_cond_grad", ["rgfm_sample_cond_grad_sde"], pick(loop, "x", "ctx"), kind="raw", forks=True)(
        _sde_build("cond_grad", SC._raw_cond_grad, ("x",)))
    SC.BY_ID.update({c.id: c for c in SC.CASES})


register_stream_cases()
