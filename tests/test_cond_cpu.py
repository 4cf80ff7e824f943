"""Conditional sampling, the parts that need no GPU: the public surface exists on every estimator, the argument checks
of sample_conditional and of the CLI fire before any device work, and evaluate_conditional_coherence is
evaluate_coherence with the two modalities put in their places."""
import pytest
import torch

from helpers import make_module
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.evaluate_mnist_svhn import evaluate_coherence, evaluate_conditional_coherence
from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional


def test_every_estimator_has_the_cross_methods():
    from ratio_guided_multimodal_fm_amd.models.ratio_flexible import RatioEstimatorMNIST, RatioEstimatorMNISTSVHN_old
    for cls in (M.RatioEstimatorMNISTSVHN, M.RatioEstimator, M.FlexibleRatioEstimator, RatioEstimatorMNIST,
                RatioEstimatorMNISTSVHN_old):
        assert callable(getattr(cls, "forward_cross")) and callable(getattr(cls, "cross_log_ratio")), cls
    for name in ("rgfm_ratio_cross_workspace_bytes", "rgfm_ratio_eval_cross", "rgfm_guidance_apply_cond",
                 "rgfm_sample_cond_workspace_bytes", "rgfm_sample_cond"):
        assert hasattr(_lib.lib(), name), name


def test_cross_methods_have_no_cpu_path_and_check_the_loss_type():
    m = make_module("ratio28")
    x = torch.zeros(2, 1, 28, 28)
    with pytest.raises(_lib.RgfmError, match="HIP device"):
        m.forward_cross(x, x)
    m.loss_type = "bogus"
    with pytest.raises(ValueError):
        m.cross_log_ratio(x, x)


def test_sample_conditional_argument_checks():
    rr = make_module("ratio28")
    cond = torch.zeros(2, 1, 28, 28)
    with pytest.raises(_lib.RgfmError, match="U-Net"):  # a FlowMatchingModel target has no conditional sampler
        sample_conditional(make_module("fm_original"), rr, cond, "x", 2, 0.5, 3)
    with pytest.raises(ValueError, match="given"):
        sample_conditional(make_module("unet28"), rr, cond, "mnist", 2, 0.5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sample_conditional(make_module("unet28"), rr, cond, "x", 2, 0.5, 3)


def test_cli_given_and_condition_go_together(capsys):
    from ratio_guided_multimodal_fm_amd import sample_mnist_svhn
    for argv in (["--given", "mnist"], ["--condition", "c.npy"], ["--given", "svhn", "--condition", "c.npy", "--sharded"],
                 ["--given", "fashion", "--condition", "c.npy"]):
        with pytest.raises(SystemExit):
            sample_mnist_svhn.main(argv)
    capsys.readouterr()
    with pytest.raises(ValueError, match="--condition"):
        p = "bad.npy"
        import numpy as np
        import os
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            np.save(os.path.join(d, p), np.zeros((2, 3, 32, 32), np.float32))
            sample_mnist_svhn.load_condition(os.path.join(d, p), (1, 32, 32))


def test_evaluate_conditional_coherence():
    cm, cs = make_module("clf_mnist"), make_module("clf_svhn")
    g = torch.Generator().manual_seed(4)
    xm, ys = torch.randn(16, 1, 32, 32, generator=g), torch.randn(16, 3, 32, 32, generator=g)
    want = evaluate_coherence(xm, ys, cm, cs, "cpu")["coherence_acc"]
    assert 0.0 <= want <= 1.0
    assert evaluate_conditional_coherence(xm, ys, "mnist", cm, cs, "cpu") == want
    assert evaluate_conditional_coherence(ys, xm, "svhn", cm, cs, "cpu") == want
    with pytest.raises(ValueError):
        evaluate_conditional_coherence(xm, ys[:3], "mnist", cm, cs, "cpu")
    with pytest.raises(ValueError):
        evaluate_conditional_coherence(xm, ys, "x", cm, cs, "cpu")
