"""Shared pieces of the class-conditioning tests (tests/test_cfg_cpu.py, tests/test_gpu_cfg.py): the three labelled nets,
their seeded inputs, raw callers of the new entry points, and the stream cases of the new stream-taking exports.

The stream cases are registered in tests/stream_cases.py's table when this module is imported, as tests/sde_cases.py and
tests/ess_cases.py do: both test files import it, and pytest imports every test module before it runs a test, so
tests/test_stream_cases_cpu.py sees the complete table in any session that collects tests/.  rgfm_unet_labeled_create
synchronises `stream` by contract, as rgfm_unet_create does: it joins the exemptions, with that reason.
"""
import ctypes
import functools

import torch

from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth

EULER, MIDPOINT = 0, 1
STEPS = 4
TABLE_ROWS = 4096

# tag: (constructor, K, weight seed)
NETS = {
    # the first net of the issue: two levels, a Downsample and an Upsample
    "k3": (lambda: M.FlexibleUNet(in_channels=1, img_size=8, model_channels=32, channel_mult=(1, 2), num_res_blocks=1,
                                  num_classes=3), 3, 41),
    # time width 4 * 256 = 1024: the LDS edge of the time-table kernels
    "k10w": (lambda: M.FlexibleUNet(in_channels=3, img_size=8, model_channels=256, channel_mult=(1,), num_res_blocks=1,
                                    num_classes=10), 10, 42),
    "mnist32": (lambda: M.FlowMatchingUNetMNIST(32, num_classes=10), 10, 43),
}
LABELS = {  # the forward's batches
    "k3": [0, 3, 2, 3, 1],                       # 3 is the null row
    "k10w": [7, 10, 0],
    "mnist32": [(5 * i + 3) % 11 for i in range(66)],  # every label 0..10 present; 66 rows: partial tiles of four samples
}


@functools.lru_cache(maxsize=None)
def net(tag):
    ctor, _, seed = NETS[tag]
    return load_synth(ctor(), seed).eval()


def classes(tag):
    return NETS[tag][1]


def shape_of(tag):
    n = net(tag)
    return (n.in_channels, n.img_size, n.img_size)


@functools.lru_cache(maxsize=None)
def inputs(tag, B, salt=0):
    """Seeded (x [B, C, S, S] ~ N(0, 1), t [B] ~ U(0, 1)) on the CPU: shared, never modified."""
    g = torch.Generator().manual_seed(8100 + 10 * B + salt + sum(map(ord, tag)))
    return torch.randn(B, *shape_of(tag), generator=g), torch.rand(B, generator=g)


def labels_of(tag, B=None):
    y = torch.tensor(LABELS[tag])
    return y if B is None else y[:B]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class RawSingleCfg:
    """rgfm_sample_single_cfg through the C ABI on the state `x` (device, in place) with device int32 labels (or None)."""

    def __init__(self, m, x, labels, dev):
        self.L, self.h, self.x, self.labels, self.dev = _lib.lib(), m.to(dev)._engine.handle(dev), x, labels, dev
        self.state = [x]

    def bytes(self, solver=EULER, sde=None):
        nb, more = ctypes.c_size_t(), ctypes.c_size_t()
        assert self.L.rgfm_sample_single_cfg_workspace_bytes(self.h, self.x.shape[0], solver, ctypes.byref(nb)) == 0
        if sde is not None and sde[0] > 0:
            assert self.L.rgfm_sde_scratch_bytes(self.x.shape[0], int(self.x[0].numel()), 0, ctypes.byref(more)) == 0
        return nb.value + more.value

    def run(self, w, steps, b, e, solver=EULER, sde=None, short=0):
        nb = self.bytes(solver, sde)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.dev)
        rec = _lib.Sde(float(sde[0]), int(sde[1])) if sde is not None else None
        return self.L.rgfm_sample_single_cfg(self.h, _p(self.x), _p(self.labels), float(w), self.x.shape[0], steps, b, e, solver,
                                             ctypes.byref(rec) if rec is not None else None, _p(ws), nb - short, _stream())


# ------------------------------------------------------------------ the stream cases of the new exports
import stream_cases as SC  # noqa: E402

W = 3.0


def _labels(d, tag, n):
    return d.labels(n, classes(tag) + 1).int()


def _forward_labels(dev, t):
    m = net("k3").to(dev)
    L, h, B = _lib.lib(), m._engine.handle(dev), t["x"].shape[0]
    nb = ctypes.c_size_t()
    assert L.rgfm_unet_workspace_bytes(h, B, ctypes.byref(nb)) == 0
    ws, out = torch.empty(nb.value, dtype=torch.uint8, device=dev), torch.empty_like(t["x"])
    assert L.rgfm_unet_forward_labels(h, _p(t["x"]), _p(t["t"]), B, _p(t["labels"]), _p(out), B, _p(ws), nb.value, _stream()) == 0
    return (out,)


def _train_labels(dev, t):
    m = net("k3").to(dev)
    L, h, B = _lib.lib(), m._engine.handle(dev), t["x"].shape[0]
    nb = ctypes.c_size_t()
    assert L.rgfm_unet_train_workspace_bytes(h, B, ctypes.byref(nb)) == 0
    ws, v, dx = torch.empty(nb.value, dtype=torch.uint8, device=dev), torch.empty_like(t["x"]), torch.empty_like(t["x"])
    dp = torch.empty(sum(q.numel() for q in m.state_dict().values()), device=dev)
    assert L.rgfm_unet_forward_train_labels(h, _p(t["x"]), _p(t["t"]), B, _p(t["labels"]), _p(v), B, 0.0, 0, _p(ws), nb.value,
                                            _stream()) == 0
    assert L.rgfm_unet_backward(h, _p(t["w"]), _p(dx), _p(dp), B, _p(ws), nb.value, _stream()) == 0
    return (v, dx, dp)


def _single_cfg_build(solver, sde):
    def build(dev, vals):
        t = SC._upload(vals, dev)
        raw = RawSingleCfg(net("k3"), t["x"], t["labels"], dev)

        def call():
            assert raw.run(W, SC.STEPS, 0, SC.STEPS, solver, sde) == 0
            return ()
        return SC.Built(t, [t["x"]], call)
    return build


def _two_cfg(dev, t):
    mx, my = net("k3").to(dev), net("k10w").to(dev)
    L, hx, hy, B = _lib.lib(), mx._engine.handle(dev), my._engine.handle(dev), t["x"].shape[0]
    nb = ctypes.c_size_t()
    assert L.rgfm_sample_two_cfg_workspace_bytes(hx, hy, B, B, MIDPOINT, ctypes.byref(nb)) == 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    assert L.rgfm_sample_two_cfg(hx, hy, _p(t["x"]), _p(t["y"]), _p(t["labels"]), _p(t["labels_y"]), W, 1.0, B, B, SC.STEPS, 0,
                                 SC.STEPS, MIDPOINT, _p(ws), nb.value, _stream()) == 0
    return ()


def register_stream_cases():
    if "cfg_forward_labels" in SC.BY_ID:
        return
    R = SC.ROWS
    SC.EXEMPT["rgfm_unet_labeled_create"] = "synchronises `stream` by contract, as rgfm_unet_create"
    xt = lambda d: {"x": d.normal(R, *shape_of("k3")), "t": d.uniform(R, hi=0.99), "labels": _labels(d, "k3", R)}
    SC.case("cfg_forward_labels", ["rgfm_unet_forward_labels"], xt, kind="raw")(SC.simple(_forward_labels))
    SC.case("cfg_forward_train_labels", ["rgfm_unet_forward_train_labels"],
            lambda d: {**xt(d), "w": d.normal(R, *shape_of("k3"))}, kind="raw")(SC.simple(_train_labels))
    xl = lambda d: {"x": d.normal(R, *shape_of("k3")), "labels": _labels(d, "k3", R)}
    SC.case("cfg_sample_single[euler+sde]", ["rgfm_sample_single_cfg"], xl, kind="raw", forks=True)(
        _single_cfg_build(EULER, (0.8, 2024)))
    SC.case("cfg_sample_single[midpoint]", ["rgfm_sample_single_cfg"], xl, kind="raw", forks=True)(
        _single_cfg_build(MIDPOINT, None))
    SC.case("cfg_sample_two", ["rgfm_sample_two_cfg"],
            lambda d: {**xl(d), "y": d.normal(R, *shape_of("k10w")), "labels_y": _labels(d, "k10w", R)}, kind="raw", forks=True)(
        SC.simple(_two_cfg, state=("x", "y")))
    SC.BY_ID.update({c.id: c for c in SC.CASES})


register_stream_cases()
