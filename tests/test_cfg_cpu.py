"""Class-conditional U-Nets and classifier-free guidance, the parts that need no GPU: the state_dict layout, the
checkpoint round trip, the command-line flags, the label dropout's draws, the Python-side label checks, and the
float64 yardstick's composition (tests/cfg_ref64.py) against a direct restatement."""
import argparse
import ctypes

import pytest
import torch

import cfg_cases  # noqa: F401  (registers the stream cases of the new exports: tests/stream_cases.py's table)
import cfg_ref64 as R
import unet_ref64 as U
from ratio_guided_multimodal_fm_amd import _engine, _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd import train_flow
from ratio_guided_multimodal_fm_amd.synth import load_synth
from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
from ratio_guided_multimodal_fm_amd.utils import flow_utils as FU


def tiny(K=3, **kw):
    cfg = dict(in_channels=1, img_size=8, model_channels=32, channel_mult=(1, 2), num_res_blocks=1)
    cfg.update(kw)
    return M.FlexibleUNet(**cfg, num_classes=K)


def test_state_dict_layout():
    for K, m in ((10, M.FlowMatchingUNetMNIST(32, num_classes=10)), (10, M.FlowMatchingUNetSVHN(num_classes=10)), (3, tiny(3))):
        sd = m.state_dict()
        assert list(sd)[-1] == "label_emb.weight"
        assert tuple(sd["label_emb.weight"].shape) == (K + 1, 4 * m.model_channels)
        plain = type(m)(32) if isinstance(m, M.FlowMatchingUNetMNIST) else (type(m)() if isinstance(m, M.FlowMatchingUNetSVHN) else
                                                                           M.FlexibleUNet(1, 8, 32, (1, 2), 1))
        assert list(sd)[:-1] == list(plain.state_dict())  # every existing entry keeps its place
        assert [tuple(v.shape) for v in list(sd.values())[:-1]] == [tuple(v.shape) for v in plain.state_dict().values()]
    assert len(M.FlowMatchingUNetMNIST(32).state_dict()) == 148
    assert len(M.FlowMatchingUNetSVHN().state_dict()) == 208
    assert M.FlowMatchingUNetMNIST(32).num_classes is None and not hasattr(M.FlowMatchingUNetMNIST(32), "label_emb")
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_classes"):
            M.FlexibleUNet(num_classes=bad)


def test_library_counts_the_label_table():
    m = M.FlowMatchingUNetSVHN(num_classes=10)
    d = m._engine.desc()
    n, n0 = ctypes.c_size_t(), ctypes.c_size_t()
    L = _lib.lib()
    assert L.rgfm_unet_param_floats(ctypes.byref(d), ctypes.byref(n0)) == 0
    assert L.rgfm_unet_labeled_param_floats(ctypes.byref(d), 10, ctypes.byref(n)) == 0
    assert n.value == n0.value + 11 * 256 == sum(v.numel() for v in m.state_dict().values())
    assert L.rgfm_unet_labeled_param_floats(ctypes.byref(d), 0, ctypes.byref(n)) == -1
    assert m._engine._create_variant() == ("rgfm_unet_labeled", (10,)) and M.FlowMatchingUNetSVHN()._engine._create_variant() == (None, ())


def test_checkpoint_round_trip(tmp_path):
    m = load_synth(tiny(3), 5)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    ck = train_flow.checkpoint(7, m, opt, 0.25)
    assert ck["num_classes"] == 3
    path = str(tmp_path / "flow.pth")
    torch.save(ck, path)
    m2 = tiny(3)
    info = load_checkpoint(m2, path)
    assert info == {"epoch": 7, "best_loss": 0.25, "num_classes": 3}
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    for other in (tiny(4), M.FlexibleUNet(1, 8, 32, (1, 2), 1)):
        with pytest.raises(ValueError, match="num_classes"):
            load_checkpoint(other, path)
    # an unlabelled net's checkpoint keeps exactly its keys
    plain = M.FlexibleUNet(1, 8, 32, (1, 2), 1)
    assert set(train_flow.checkpoint(1, plain, torch.optim.Adam(plain.parameters()), 1.0)) == \
        {"epoch", "model_state_dict", "optimizer_state_dict", "best_loss"}


def test_cli_flags():
    a = train_flow.parse_args(["--preset", "svhn", "--data", "d.npz", "--num_classes", "10", "--p_uncond", "0.2"])
    assert a.num_classes == 10 and a.p_uncond == 0.2
    a = train_flow.parse_args(["--preset", "svhn", "--data", "d.npy"])
    assert a.num_classes is None and a.p_uncond == 0.1
    with pytest.raises(SystemExit):
        train_flow.parse_args(["--preset", "original", "--modality", "x", "--data", "d.npz", "--num_classes", "10"])
    p = argparse.ArgumentParser()
    FU.add_label_args(p)
    a = p.parse_args([])
    assert (a.num_classes, a.labels, a.cfg_scale) == (None, None, 1.0) and FU.labels_from_cli(a, 4) == {}
    a = p.parse_args(["--num_classes", "10", "--labels", "cycle", "--cfg_scale", "3"])
    kw = FU.labels_from_cli(a, 12)
    assert kw["cfg_scale"] == 3.0 and kw["labels"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 1]
    assert FU.labels_from_cli(p.parse_args(["--num_classes", "10", "--labels", "7"]), 3)["labels"].tolist() == [7, 7, 7]
    torch.manual_seed(0)
    r = FU.labels_from_cli(p.parse_args(["--num_classes", "4", "--labels", "random"]), 64)["labels"]
    assert r.shape == (64,) and 0 <= int(r.min()) and int(r.max()) <= 3
    for argv, kw in ((["--labels", "3"], {}), (["--num_classes", "10", "--labels", "11"], {}), (["--num_classes", "10", "--labels", "x"], {}),
                     (["--cfg_scale", "2"], {}), (["--num_classes", "10", "--labels", "3"], {"sharded": True}),
                     (["--num_classes", "10", "--labels", "3"], {"guided": True}), (["--num_classes", "10", "--labels", "3"], {"unet": False})):
        with pytest.raises(_lib.RgfmError):
            FU.labels_from_cli(p.parse_args(argv), 4, **kw)
    # the four samplers / evaluators build their parsers in main(): the flags are the helper's
    import inspect
    from ratio_guided_multimodal_fm_amd import evaluate, evaluate_mnist_svhn, sample, sample_mnist_svhn
    for mod in (evaluate, evaluate_mnist_svhn, sample, sample_mnist_svhn):
        src = inspect.getsource(mod.main)
        assert "add_label_args(p)" in src and "labels_from_cli(args" in src, mod.__name__
    for fn in (evaluate.run_sweep, evaluate_mnist_svhn.run_sweep, FU.paired_sampler, FU.sample_bimodal_guided,
               sample_mnist_svhn.sample_bimodal_guided_mnist_svhn):
        sig = inspect.signature(fn).parameters
        assert sig["labels"].default is None and sig["cfg_scale"].default == 1.0


def test_label_dropout_draws():
    g = torch.Generator().manual_seed(3)
    y = torch.arange(1000) % 10
    out = FU.drop_labels(y, 10, 0.1, generator=g)
    dropped = out == 10
    assert 50 < int(dropped.sum()) < 150 and torch.equal(out[~dropped], y[~dropped])
    g.manual_seed(3)
    assert torch.equal(torch.rand(1000, generator=g) < 0.1, dropped)  # the draw: one rand per label
    assert torch.equal(FU.drop_labels(y, 10, 0.0), y) and bool((FU.drop_labels(y, 10, 1.0) == 10).all())
    with pytest.raises(ValueError):
        FU.drop_labels(y, 10, 1.5)


class _Recorder(torch.nn.Module):
    """A stand-in net: records what the epoch feeds it; its output depends on a parameter so that backward runs."""

    def __init__(self, num_classes=None):
        super().__init__()
        self.num_classes = num_classes
        self.w = torch.nn.Parameter(torch.ones(()))
        self.calls = []

    def forward_train(self, x, t, y=None):
        self.calls.append((x.detach().clone(), t.detach().clone(), None if y is None else y.detach().clone()))
        return x * self.w


def _epoch(monkeypatch, net, batches, **kw):
    monkeypatch.setattr(FU, "_device", lambda d: torch.device("cpu"))
    torch.manual_seed(11)
    FU.train_flow_matching_epoch(net, batches, torch.optim.SGD(net.parameters(), lr=0.0), FU.CFMSchedule(), "cpu", **kw)
    return net.calls, torch.rand(3)  # (and where the generator stands after the epoch)


def test_epoch_draws_with_and_without_labels(monkeypatch):
    data = [torch.randn(4, 1, 8, 8, generator=torch.Generator().manual_seed(i)) for i in range(2)]
    lab = [torch.tensor([0, 1, 2, 1]), torch.tensor([2, 2, 0, 1])]
    # an unlabelled epoch draws t, then x_0, per batch and nothing else -- on a plain net and on a net with classes
    torch.manual_seed(11)
    want = []
    for x1 in data:
        t = torch.rand(4)
        x0 = torch.randn_like(x1)
        tt = t.view(4, 1, 1, 1)
        want.append(((1 - tt) * x0 + tt * x1, t))
    after = torch.rand(3)
    for net in (_Recorder(), _Recorder(3)):
        calls, tail = _epoch(monkeypatch, net, [{"x": d} for d in data])
        assert all(torch.equal(c[0], w[0]) and torch.equal(c[1], w[1]) and c[2] is None for c, w in zip(calls, want))
        assert torch.equal(tail, after)
    # labels: the same t and x_0 draws, then one rand per label; p_uncond = 0 keeps every label
    calls, _ = _epoch(monkeypatch, _Recorder(3), list(zip(data, lab)), p_uncond=0.0)
    assert torch.equal(calls[0][0], want[0][0]) and torch.equal(calls[0][1], want[0][1]) and torch.equal(calls[0][2], lab[0])
    calls, _ = _epoch(monkeypatch, _Recorder(3), list(zip(data, lab)), p_uncond=1.0)
    assert all(bool((c[2] == 3).all()) for c in calls)
    calls, _ = _epoch(monkeypatch, _Recorder(3), [{"x": d, "label": y} for d, y in zip(data, lab)], p_uncond=0.0)
    assert torch.equal(calls[1][2], lab[1])
    with pytest.raises(TypeError, match="num_classes"):
        _epoch(monkeypatch, _Recorder(), list(zip(data, lab)))


def test_label_validation():
    m = tiny(3)
    eng = m._engine
    assert eng.check_labels(None, 5, "cpu") is None
    y = eng.check_labels(torch.tensor([0, 3, 2, 3, 1]), 5, "cpu")
    assert y.dtype == torch.int32 and y.tolist() == [0, 3, 2, 3, 1]
    for bad in (torch.tensor([0, 1, 2, 3, 4]), torch.tensor([0, -1, 2, 3, 1]), torch.tensor([0, 1]), torch.zeros(5),
                torch.zeros(5, 1, dtype=torch.long), [0, 1, 2, 3, 1], torch.zeros(5, dtype=torch.bool)):
        with pytest.raises(_lib.RgfmError, match="label"):
            eng.check_labels(bad, 5, "cpu")
    plain = M.FlexibleUNet(1, 8, 32, (1, 2), 1)
    with pytest.raises(_lib.RgfmError, match="num_classes"):
        plain._engine.check_labels(torch.zeros(5, dtype=torch.long), 5, "cpu")
    with pytest.raises(_lib.RgfmError, match="no class labels"):
        M.FlowMatchingModel()._engine.check_labels(torch.zeros(5, dtype=torch.long), 5, "cpu")
    assert _engine.check_cfg(None, 1.0, 5, m) is None
    lab, w = _engine.check_cfg(torch.tensor([0, 3, 2, 3, 1]), 3, 5, m)
    assert w == 3.0 and lab.dtype == torch.int32
    with pytest.raises(_lib.RgfmError, match="cfg_scale needs labels"):
        _engine.check_cfg(None, 3.0, 5, m)
    with pytest.raises(ValueError, match="finite"):
        _engine.check_cfg(torch.zeros(5, dtype=torch.long), float("nan"), 5, m)
    # the entry points without a labelled form refuse before they touch a device
    x, t = torch.zeros(2, 1, 8, 8), torch.zeros(2)
    yy = torch.zeros(2, dtype=torch.long)
    for call in (lambda: m.vjp(x, t, x, y=yy), lambda: m.divergence(x, t, x[None], y=yy), lambda: m.linearize(x, t, y=yy),
                 lambda: FU.CFMSchedule().log_prob(m, x, 4, labels=yy),
                 lambda: FU.sample_conditional(m, None, x, labels=yy),
                 lambda: FU.paired_sampler(m, tiny(3), None, "mc_feng", 1.0, 2, 4, "cuda", 4, (1, 8, 8), (1, 8, 8), labels=yy),
                 lambda: FU.paired_sampler(m, tiny(3), None, "grad_log_ratio", 1.0, 2, 4, "cuda", 4, (1, 8, 8), (1, 8, 8), labels=yy),
                 lambda: FU.paired_sampler(m, M.FlowMatchingModel(), None, "none", 0.0, 2, 4, "cuda", 4, (1, 8, 8), (1, 28, 28), labels=yy)):
        with pytest.raises(_lib.RgfmError):
            call()
    from ratio_guided_multimodal_fm_amd.distributed import make_sharded_sampler
    from ratio_guided_multimodal_fm_amd.evaluate_mnist_svhn import run_sweep
    with pytest.raises(_lib.RgfmError, match="sharded"):
        make_sharded_sampler((1, 8, 8), (1, 8, 8))(m, m, None, "none", 0.0, 2, 2, "cuda", 4, labels=yy)
    with pytest.raises(_lib.RgfmError, match="sharded"):
        run_sweep(m, m, lambda: None, None, None, ["none"], [0.0], 2, 2, "cuda", 4, sampler=make_sharded_sampler((1, 8, 8), (1, 8, 8)),
                  labels=yy)
    with pytest.raises(_lib.RgfmError, match="guided"):
        run_sweep(m, m, lambda: None, None, None, ["none", "mc_feng"], [0.0], 2, 2, "cuda", 4, labels=yy)
    assert _engine._cfg_chunks((M.FlowMatchingUNetSVHN(num_classes=10),), 0, 0, 1000) == [(0, 372), (372, 744), (744, 1000)]
    assert _engine._cfg_chunks((M.FlowMatchingUNetSVHN(num_classes=10),), 1, 3, 200) == [(3, 189), (189, 200)]


def test_ref64_composition_vs_direct_restatement():
    m = load_synth(M.FlexibleUNet(in_channels=3, img_size=8, model_channels=32, channel_mult=(1,), num_res_blocks=1, num_classes=4), 21)
    sd = R.params64(m, requires_grad=False)
    g = torch.Generator().manual_seed(2)
    x, t = torch.randn(6, 3, 8, 8, generator=g).double(), torch.rand(6, generator=g).double()
    y = torch.tensor([4, 0, 2, 2, 4, 1])
    a = R.forward_labels64(U.cfg_of(m), sd, x, t, y)
    b = R.direct64(sd, x, t, y)
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    # y = None is the null label; a label changes the output
    assert torch.equal(R.forward_labels64(U.cfg_of(m), sd, x, t, None), R.forward_labels64(U.cfg_of(m), sd, x, t, torch.full((6,), 4)))
    assert float((a - R.forward_labels64(U.cfg_of(m), sd, x, t, None)).abs().max()) > 1e-3
    # the gradient of the embedding through the composition: that of the direct form, zero rows for absent classes
    grads = []
    for fwd in (lambda p: R.forward_labels64(U.cfg_of(m), p, x, t, y), lambda p: R.direct64(p, x, t, y)):
        p = R.params64(m)
        fwd(p).square().sum().backward()
        grads.append(p[R.EMB].grad)
    assert float((grads[0] - grads[1]).abs().max()) <= 1e-10 * float(grads[1].abs().max())
    assert bool((grads[0][3] == 0).all()) and float(grads[0][4].abs().max()) > 0
    # the CFG loop: integrate64 over v_u + w (v_c - v_u), written out once for two Euler steps
    x0 = x.numpy()
    w = 3.0
    s = x0.copy()
    for i in range(2):
        tt = torch.tensor([i / 2.0])
        c = R.direct64(sd, torch.from_numpy(s), tt, y).numpy()
        u = R.direct64(sd, torch.from_numpy(s), tt, torch.full((6,), 4)).numpy()
        s = s + 0.5 * (u + w * (c - u))
    got = R.sample_cfg64(m, x0, y, w, 2)
    assert abs(got - s).max() <= 1e-12 * max(1.0, abs(s).max())
