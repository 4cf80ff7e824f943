"""Raw ctypes callers of the effective-sample-size floor's exports (include/rgfm.h, "Effective-sample-size floor"):
the blocks rgfm_guidance_apply_ess / rgfm_guidance_apply_cond_ess and the loops rgfm_sample_pair_ess /
rgfm_sample_cond_ess over the loops of tests/test_gpu_ode.py.  Shared by tests/test_gpu_ess.py and the stream-case table
(tests/stream_cases.py); importable without a GPU.

The stream cases of the four exports are registered from here when this module is imported, as tests/sde_cases.py does
for the *_sde exports: tests/test_ess_cpu.py and tests/test_gpu_ess.py import it, and pytest imports every test module
of a run before it runs a test, so tests/test_stream_cases_cpu.py finds the rows and tests/test_gpu_streams.py runs them.
tests/test_ess_cpu.py asserts the coverage itself.
"""
import ctypes

import torch

import sde_cases as C
import test_gpu_ode as T
from ratio_guided_multimodal_fm_amd import _lib

EULER, MIDPOINT = 0, 1
_p = C._p


def ws_block(B, N, dev):
    nb = ctypes.c_size_t()
    assert _lib.lib().rgfm_guidance_workspace_bytes(B, N, ctypes.byref(nb)) == 0
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


def block_pair(d, t, rows, ess_min, tau=None, weights=None, rows_namesake=False):
    """rc of rgfm_guidance_apply_ess on the device tensors d = {x, y, vx, vy, mx, my, r} (vx, vy in place);
    rows_namesake: rgfm_guidance_apply_rows on the same arguments."""
    L = _lib.lib()
    B, N = d["x"].shape[0], d["mx"].shape[0]
    dx, dy = d["x"][0].numel(), d["y"][0].numel()
    ws, nb = ws_block(B, N, d["x"].device)
    head = (_p(d["x"]), _p(d["y"]), _p(d["vx"]), _p(d["vy"]), _p(d["mx"]), _p(d["my"]), _p(d["r"]), B, N, dx, dy, float(t), _p(rows),
            _p(weights))
    if rows_namesake:
        return L.rgfm_guidance_apply_rows(*head, _p(ws), nb, T._stream())
    return L.rgfm_guidance_apply_ess(*head, float(ess_min), _p(tau), _p(ws), nb, T._stream())


def block_cond(d, t, rows, ess_min, tau=None, weights=None, rows_namesake=False):
    """rc of rgfm_guidance_apply_cond_ess on d = {s, v, m, R} (v in place)."""
    L = _lib.lib()
    B, N = d["s"].shape[0], d["m"].shape[0]
    ws, nb = ws_block(B, N, d["s"].device)
    head = (_p(d["s"]), _p(d["v"]), _p(d["m"]), _p(d["R"]), B, N, d["s"][0].numel(), float(t), _p(rows), _p(weights))
    if rows_namesake:
        return L.rgfm_guidance_apply_cond_rows(*head, _p(ws), nb, T._stream())
    return L.rgfm_guidance_apply_cond_ess(*head, float(ess_min), _p(tau), _p(ws), nb, T._stream())


class RawEss(C.RawSde):
    """A sde_cases.RawSde of the pair or the one-sided MC loop with the `const rgfm_ess*` behind the `const rgfm_sde*`.
    The workspace is RawSde's: the floor asks for none of its own."""

    def run(self, b, e, ess=None, sde=None, solver=EULER, rows=None, scale=None, diag=None, short=0, namesake=False,
            tau_records=None):
        """rc of the call on steps [b, e).  ess: None -- a null pointer; (ess_min, tau tensor or None) -- the record.
        namesake: the *_sde entry point on the same arguments.  tau_records: what the record claims (default: the
        tensor's size)."""
        if namesake:
            return super().run(b, e, sde, solver, rows, scale, diag, short)
        eta_on = sde is not None and sde[0] > 0
        nb = self.base_bytes(solver, diag is not None) + (self.scratch_bytes() if eta_on else 0)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.state[0].device)
        srec = _lib.Sde(float(sde[0]), int(sde[1]) % (1 << 64)) if sde is not None else None
        erec = None
        if ess is not None:
            tau = ess[1]
            n = (0 if tau is None else tau.numel()) if tau_records is None else tau_records
            erec = _lib.Ess(float(ess[0]), _p(tau), n)
        arr = (ctypes.c_double * len(scale))(*scale) if scale is not None else None
        cap = 0 if diag is None else diag.shape[0] * diag.shape[1]
        return getattr(self.L, f"rgfm_sample_{self.kind}_ess")(
            *self.raw.args, _p(rows), arr, 0 if scale is None else len(scale), b, e, solver, _p(diag), cap,
            ctypes.byref(srec) if srec is not None else None, ctypes.byref(erec) if erec is not None else None,
            _p(ws), nb - short, T._stream())


def make(kind, B, dev, n_mc=8, steps=T.STEPS, gamma=T.GAMMA):
    """A RawEss of the pair or the one-sided loop on fresh device copies of test_gpu_ode's shared start states."""
    assert kind in ("pair", "cond")
    if kind == "pair":
        return RawEss(kind, T.raw_pair(*T.pair_inputs(B, n_mc, dev), steps, gamma, dev))
    return RawEss(kind, T.raw_cond("g24", T.start("g24", B).to(dev).clone(), T.mc_set("g24", n_mc).to(dev),
                                   T.ratios(5, n_mc)[:B].contiguous().to(dev), steps, gamma, dev))


# ------------------------------------------------------------------ the stream cases of the *_ess exports
import stream_cases as SC  # noqa: E402  (behind the callers above, which its rows use)

ESS_MIN = 3.0


def _ess_build(kind, make_raw, state):
    def build(dev, vals):
        t = SC._upload(vals, dev)
        raw = RawEss(kind, make_raw(dev, t))
        tau = torch.zeros(SC.STEPS, SC.ROWS, device=dev)

        def call():
            assert raw.run(0, SC.STEPS, (ESS_MIN, tau)) == 0
            return ()
        return SC.Built(t, [t[k] for k in state] + [tau], call)
    return build


def _block_pair(dev, t):
    tau = torch.zeros(SC.ROWS, device=dev)
    w = torch.zeros(SC.ROWS, SC.N_MC, device=dev)
    d = {k: t[k].flatten(1) for k in ("x", "y", "vx", "vy", "mx", "my")}
    assert block_pair({**d, "r": t["r"]}, 0.9, t["g"], ESS_MIN, tau, w) == 0
    return (tau, w)


def _block_cond(dev, t):
    tau = torch.zeros(SC.ROWS, device=dev)
    w = torch.zeros(SC.ROWS, SC.N_MC, device=dev)
    assert block_cond({"s": t["y"].flatten(1), "v": t["vy"].flatten(1), "m": t["my"].flatten(1), "R": t["rows"]}, 0.9, t["g"],
                      ESS_MIN, tau, w) == 0
    return (tau, w)


def register_stream_cases():
    if "ess_sample_pair" in SC.BY_ID:
        return
    S, G, pick, loop, block = SC.STEPS, SC.GAMMA, SC._pick, SC._loop, SC._block
    SC.case("ess_guidance_apply", ["rgfm_guidance_apply_ess"], pick(block, *SC.PAIRED, "r", "g"), kind="raw")(
        SC.simple(_block_pair, state=("vx", "vy")))
    SC.case("ess_guidance_apply_cond", ["rgfm_guidance_apply_cond_ess"], pick(block, "y", "vy", "my", "rows", "g"), kind="raw")(
        SC.simple(_block_cond, state=("vy",)))
    SC.case("ess_sample_pair", ["rgfm_sample_pair_ess"], pick(loop, "x", "y", "mx", "my", "r"), kind="raw", forks=True)(
        _ess_build("pair", lambda dev, t: T.raw_pair(t["x"], t["y"], t["mx"], t["my"], t["r"], S, G, dev), ("x", "y")))
    SC.case("ess_sample_cond", ["rgfm_sample_cond_ess"], pick(loop, "y", "my", "rows"), kind="raw", forks=True)(
        _ess_build("cond", lambda dev, t: T.raw_cond("g24", t["y"], t["my"], t["rows"], S, G, dev), ("y",)))
    SC.BY_ID.update({c.id: c for c in SC.CASES})


register_stream_cases()
