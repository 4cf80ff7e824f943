"""CPU-only checks of FlexibleRatioEstimator: the classes and their state_dict layout against the reference's
(tests/golden/ratio_flex.npz, written by tests/golden/make_ratio_flex_golden.py), the C ABI's parameter count and
descriptor rules, and the float64 restatement the GPU tests measure against (tests/ratio_flex_ref64.py) against the
reference's own outputs and autograd gradients."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden
from ratio_flex_ref64 import forward64, log_ratio64, params64
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd.synth import load_synth

# The fixture's values are the reference's fp32 results; the restatement is float64.  Measured fp32-vs-float64 error of
# the reference at these shapes: 5e-7 on the scores (|score| <= 1.2), 2e-6 relative on the gradients.  The bounds are
# the suite's: 1e-5 absolute on an evaluation (tests/test_gpu_parity.py), 1e-4 of the tensor's maximum on a gradient.
TOL_EVAL, TOL_GRAD = 1e-5, 1e-4


def classes():
    from ratio_guided_multimodal_fm_amd.models.ratio_flexible import (FlexibleRatioEstimator, RatioEstimatorMNIST,
                                                                      RatioEstimatorMNISTSVHN_old)
    return FlexibleRatioEstimator, RatioEstimatorMNIST, RatioEstimatorMNISTSVHN_old


def fixture_module():
    g = golden("ratio_flex")
    B, xc, yc, xs, ys, feat, hid = (int(v) for v in g["dims"])
    m = load_synth(classes()[0](xc, yc, feat, hid), int(g["w_seed"])).eval()
    gen = torch.Generator().manual_seed(int(g["data_seed"]))
    x, y = torch.randn(B, xc, xs, xs, generator=gen), torch.randn(B, yc, ys, ys, generator=gen)
    return g, m, x, y


def probe_idx(numel, salt, n):  # must match tests/golden/make_ratio_flex_golden.py
    return torch.randint(0, numel, (n,), generator=torch.Generator().manual_seed(7000 + salt))


def test_classes_import_with_the_reference_surface():
    Flex, Mnist, Old = classes()
    from ratio_guided_multimodal_fm_amd import models as M
    assert M.FlexibleRatioEstimator is Flex and M.RatioEstimatorMNIST is Mnist and M.RatioEstimatorMNISTSVHN_old is Old
    m = Flex()
    assert (m.x_channels, m.y_channels, m.feature_dim, m.hidden_dim, m.loss_type) == (1, 1, 256, 512, "disc")
    a, b = Mnist("rulsif"), Old()
    assert (a.x_channels, a.y_channels, a.feature_dim, a.hidden_dim, a.loss_type) == (1, 1, 256, 512, "rulsif")
    assert (b.x_channels, b.y_channels, b.feature_dim, b.hidden_dim, b.loss_type) == (1, 3, 256, 512, "disc")
    assert issubclass(Mnist, Flex) and issubclass(Old, Flex)
    for name in ("forward", "forward_train", "log_ratio", "grad_log_ratio", "dropout_p"):
        assert callable(getattr(m, name)), name
    assert m.dropout_p() == pytest.approx(0.1)
    assert b.encoder_y.conv1.weight.shape == (32, 3, 3, 3)
    with pytest.raises(_lib.RgfmError, match="HIP device"):  # no CPU path
        m.eval()(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))


def test_state_dict_layout_is_the_reference_one():
    g, m, x, y = fixture_module()
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    for v, shape, s in zip(sd.values(), g["shapes"], g["weight_sums"]):
        assert list(v.shape) == [int(d) for d in shape[:v.dim()]] and not shape[v.dim():].any()
        assert float(v.double().sum()) == pytest.approx(float(s), rel=1e-12, abs=1e-12)  # the seeded recipe reproduces
    assert float(x.double().sum()) == float(g["input_sums"][0]) and float(y.double().sum()) == float(g["input_sums"][1])
    # a checkpoint of the reference's presets loads strictly: same keys, same shapes
    for cls in classes()[1:]:
        keys = list(cls().state_dict())
        assert keys == [str(k) for k in g["keys"]]


@pytest.mark.parametrize("xc,yc", [(1, 1), (1, 3), (4, 2)])
def test_param_floats(xc, yc):
    m = classes()[0](xc, yc, 64, 128)
    d = _lib.RatioFlexDesc(64, 128, 0, xc, yc, 12, 20)
    n = ctypes.c_size_t()
    assert _lib.lib().rgfm_ratio_flex_param_floats(ctypes.byref(d), ctypes.byref(n)) == 0
    assert n.value == sum(v.numel() for v in m.state_dict().values())
    d.x_size, d.y_size = 64, 8  # the count does not depend on the sizes
    n2 = ctypes.c_size_t()
    assert _lib.lib().rgfm_ratio_flex_param_floats(ctypes.byref(d), ctypes.byref(n2)) == 0 and n2.value == n.value


@pytest.mark.parametrize("geom,field", [((0, 1, 12, 12), b"x_channels"), ((5, 1, 12, 12), b"x_channels"),
                                        ((1, 0, 12, 12), b"y_channels"), ((1, 5, 12, 12), b"y_channels"),
                                        ((1, 1, 7, 12), b"x_size"), ((1, 1, 12, 7), b"y_size"),
                                        ((1, 1, 300, 12), b"x_size"), ((1, 1, 12, 96), b"y_size")])
def test_bad_descriptor_is_einval_and_names_the_field(geom, field):
    L = _lib.lib()
    d = _lib.RatioFlexDesc(64, 128, 0, *geom)
    n = ctypes.c_size_t()
    assert L.rgfm_ratio_flex_param_floats(ctypes.byref(d), ctypes.byref(n)) == -1  # RGFM_EINVAL
    assert field in L.rgfm_last_error()
    h = ctypes.c_void_p()
    assert L.rgfm_ratio_flex_create(ctypes.byref(d), ctypes.c_void_p(16), 1, None, ctypes.byref(h)) == -1
    assert field in L.rgfm_last_error() and not h.value


def test_fixed_kinds_keep_their_descriptor():
    """The two fixed kinds still go through rgfm_ratio_desc; the flexible kind has no geometry there and is refused."""
    L = _lib.lib()
    n = ctypes.c_size_t()
    d = _lib.RatioDesc(2, 256, 512, 0)
    assert L.rgfm_ratio_param_floats(ctypes.byref(d), ctypes.byref(n)) == -1
    assert b"rgfm_ratio_flex_create" in L.rgfm_last_error()
    d28, f28 = _lib.RatioDesc(1, 256, 512, 0), _lib.RatioFlexDesc(256, 512, 0, 1, 1, 28, 28)
    n28 = ctypes.c_size_t()
    assert L.rgfm_ratio_param_floats(ctypes.byref(d28), ctypes.byref(n28)) == 0
    assert L.rgfm_ratio_flex_param_floats(ctypes.byref(f28), ctypes.byref(n)) == 0 and n.value == n28.value


def test_float64_restatement_reproduces_the_reference():
    g, m, x, y = fixture_module()
    sd = params64(m, requires_grad=False)
    with torch.no_grad():
        s = forward64(sd, x, y)
        assert np.abs(s.numpy() - g["forward"]).max() < TOL_EVAL
        for lt in ("disc", "rulsif"):
            assert np.abs(log_ratio64(sd, x, y, lt).numpy() - g["log_ratio_" + lt]).max() < TOL_EVAL
    row = 0
    for lt in ("disc", "rulsif"):
        x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
        grads = torch.autograd.grad(log_ratio64(sd, x64, y64, lt).sum(), (x64, y64))
        for salt, gr in enumerate(grads):
            amax = float(g["grad_xy_max"][row])
            assert abs(float(gr.abs().max()) - amax) <= TOL_GRAD * amax
            probe = gr.reshape(-1)[probe_idx(gr.numel(), salt, g["grad_xy_probe"].shape[1])].numpy()
            assert np.abs(probe - g["grad_xy_probe"][row]).max() <= TOL_GRAD * amax, (lt, salt)
            row += 1


def test_float64_parameter_gradients_reproduce_the_reference():
    g, m, x, y = fixture_module()
    sd = params64(m)
    real = (torch.arange(x.shape[0]) % 2 == 0).double()
    loss = F.binary_cross_entropy_with_logits(forward64(sd, x, y), real)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    for i, (k, v) in enumerate(sd.items()):
        amax = float(g["grad_param_max"][i])
        assert abs(float(v.grad.abs().max()) - amax) <= TOL_GRAD * amax, k
        probe = v.grad.reshape(-1)[probe_idx(v.numel(), 100 + i, g["grad_param_probe"].shape[1])].numpy()
        assert np.abs(probe - g["grad_param_probe"][i]).max() <= TOL_GRAD * amax, k


def test_dropped_row_and_column_get_no_gradient_in_float64():
    """The 3 -> 1 and 5 -> 2 pools of the fixture's shapes drop a row and a column: their gradient is exactly zero."""
    g, m, x, y = fixture_module()
    sd = params64(m)
    out = {}
    forward64(sd, x.double().requires_grad_(True), y.double().requires_grad_(True), out=out).sum().backward()
    seen = 0
    for enc in out["pooled_in"]:
        for a in enc:
            if a.shape[-1] % 2:
                assert not a.grad[:, :, -1, :].any() and not a.grad[:, :, :, -1].any()
                assert a.grad[:, :, :-1, :-1].any()
                seen += 1
    assert seen == 2  # x: 3x3 in front of pool3; y: 5x5 in front of pool3


def test_train_cli_flexible_arguments_and_checkpoint_format(tmp_path, monkeypatch):
    import os
    from ratio_guided_multimodal_fm_amd import train_ratio
    from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
    a = train_ratio.parse_args(["--kind", "flexible", "--data", "d.npz", "--x_channels", "3", "--y_channels", "2",
                                "--loss_type", "rulsif"])
    assert (a.x_channels, a.y_channels) == (3, 2)
    monkeypatch.chdir(tmp_path)
    path = train_ratio.checkpoint_path(a, "best")
    assert path == "checkpoints/ratio_rulsif_flexible_best.pth" and os.path.isdir("checkpoints")
    # sizes come from the data file: any square image of the stated channels
    np.savez("ok.npz", x=np.zeros((4, 3, 16, 16), np.float32), y=np.zeros((4, 2, 12, 12), np.float32), label=np.arange(4) % 2)
    x, y, _ = train_ratio.load_pairs("ok.npz", (3, None, None), (2, None, None))
    assert x.shape == (4, 3, 16, 16) and y.shape == (4, 2, 12, 12)
    with pytest.raises(ValueError):
        train_ratio.load_pairs("ok.npz", (1, None, None), (2, None, None))
    np.savez("rect.npz", x=np.zeros((4, 3, 16, 12), np.float32), y=np.zeros((4, 2, 12, 12), np.float32), label=np.arange(4) % 2)
    with pytest.raises(ValueError):
        train_ratio.load_pairs("rect.npz", (3, None, None), (2, None, None))
    m = load_synth(classes()[0](3, 2, 64, 128, "rulsif"), 5)
    train_ratio.save_checkpoint(m, a, path, 7, 0.25)
    ckpt = torch.load(path)
    assert {k: ckpt[k] for k in ("x_channels", "y_channels", "feature_dim", "hidden_dim", "loss_type")} == \
        {"x_channels": 3, "y_channels": 2, "feature_dim": 64, "hidden_dim": 128, "loss_type": "rulsif"}
    again = classes()[0](ckpt["x_channels"], ckpt["y_channels"], ckpt["feature_dim"], ckpt["hidden_dim"], ckpt["loss_type"])
    assert load_checkpoint(again, path) == {"epoch": 7, "best_loss": 0.25}
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in m.state_dict().items())
