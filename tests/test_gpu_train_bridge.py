"""The host bridge the four training passes share (_engine._TrainFn on _EngineBase.handle): a backward that has lost its
saved state or its handle is an error in every family, and an optimizer step repacks the handle instead of re-creating it."""
import pytest
import torch

from helpers import make_generic_unet, make_module
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth

pytestmark = pytest.mark.gpu

B = 2
FAMILIES = ["unet", "fmnet", "ratio", "ratio_flex", "clf"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def case(family, dev):
    """(module in training mode, one tuple of forward_train inputs per geometry the module is driven at)."""
    g = torch.Generator().manual_seed(77)

    def randn(*shape):
        return torch.randn(*shape, generator=g).to(dev)
    if family == "unet":
        m, calls = make_generic_unet("g24", dev)[0], [(randn(B, 3, 24, 24), torch.rand(B, generator=g).to(dev))]
    elif family == "fmnet":
        m, calls = make_module("fm_original", dev), [(randn(B, 1, 28, 28), torch.rand(B, generator=g).to(dev))]
    elif family == "ratio":
        m, calls = make_module("ratio_ms", dev), [(randn(B, 1, 32, 32), randn(B, 3, 32, 32))]
    elif family == "ratio_flex":  # two pairs of sizes, the second with odd rasters (12 -> 6 -> 3, 20 -> 10 -> 5)
        m = load_synth(M.FlexibleRatioEstimator(1, 1, 64, 128, "disc"), 31).to(dev)
        calls = [(randn(B, 1, 8, 8), randn(B, 1, 8, 8)), (randn(B, 1, 12, 12), randn(B, 1, 20, 20))]
    else:
        m, calls = make_module("clf_svhn", dev), [(randn(B, 3, 32, 32),)]
    return m.train(), calls


def loss_of(m, call):
    return m.forward_train(*call).square().mean()


@pytest.mark.parametrize("family", FAMILIES)
def test_second_backward_is_an_error(dev, family):
    m, calls = case(family, dev)
    loss = loss_of(m, calls[-1])
    loss.backward(retain_graph=True)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    with pytest.raises(_lib.RgfmError, match="saved state of this forward_train call is gone"):
        loss.backward()


@pytest.mark.parametrize("family", FAMILIES)
def test_backward_after_the_handle_was_rebuilt_is_an_error(dev, family):
    m, calls = case(family, dev)
    loss = loss_of(m, calls[-1])
    name, p = next(iter(m.named_parameters()))
    owner, _, leaf = name.rpartition(".")
    setattr(m.get_submodule(owner), leaf, torch.nn.Parameter(p.detach().clone()))
    loss_of(m, calls[-1])  # the module's tensors are not the packed ones any more: a new handle
    with pytest.raises(_lib.RgfmError, match="re-created"):
        loss.backward()


@pytest.mark.parametrize("family", FAMILIES)
def test_optimizer_steps_keep_the_handle(dev, family):
    m, calls = case(family, dev)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    seen = [set() for _ in calls]
    for _ in range(3):
        for handles, call in zip(seen, calls):
            opt.zero_grad(set_to_none=True)
            loss = loss_of(m, call)
            handles.add(m._engine._handle.value)
            loss.backward()
            opt.step()
    assert all(len(handles) == 1 for handles in seen), seen
    assert len(set.union(*seen)) == len(calls)  # one handle per geometry, alternating re-creates none
