"""The Upsample kernel that computes all four parity classes of an input tile from one staged halo
(conv_mfma_hx2u.hip) against the kernel it replaces (conv_mfma_hx2p_kernel<*, CONV_T2, *>, a workgroup per class:
RGFM_HX2U=0).  Same summation order per output element, so everything here is torch.equal; the hook
rgfm_unet_up_merged says which of the two a walk really took.

The Upsample rasters are fixed by the presets (svhn: 8 -> 16 and 16 -> 32 with 128 channels; mnist32: 16 -> 32 with 64),
so the batch is the only size knob: 1, 2, 3 and 11 rows give a lone sample in a two-sample 8x8 tile, a full one, an odd
tail, and several tiles with a partly filled last one.  A workgroup of the kernel WALKS tiles when a launch has more of
them than the device has CUs; RGFM_HX2U_WGS=n caps the workgroups so that 11 rows reach that loop too."""
import pytest
import torch

import range_cases as R
from oracle import oracle as O
from helpers import make_module, make_sweep_unet, maxdiff, oracle_net
from ratio_guided_multimodal_fm_amd import _engine, _lib

pytestmark = pytest.mark.gpu

TOL_EVAL = 1e-5
SHAPES = {"unet28": (1, 28, 28), "mnist32": (1, 32, 32), "svhn": (3, 32, 32)}
MERGED = {"mnist32": 1, "svhn": 2}  # Upsample convs of the preset inside the kernel's scope


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def inputs(tag, B):
    x = torch.randn(B, *SHAPES[tag], generator=torch.Generator().manual_seed(41))
    t = torch.rand(B, generator=torch.Generator().manual_seed(42))
    return x, t


def both(m, x, t, dev, monkeypatch):
    """(output on the new kernel, convs it took, output with RGFM_HX2U=0, convs it took then)."""
    new = m(x.to(dev), t.to(dev))
    n_new = m._engine.up_merged(dev)
    with monkeypatch.context() as mp:
        mp.setenv("RGFM_HX2U", "0")
        old = m(x.to(dev), t.to(dev))
        n_old = m._engine.up_merged(dev)
    return new, n_new, old, n_old


@pytest.mark.parametrize("tag", ["mnist32", "svhn"])
def test_bitwise_against_the_kernel_it_replaces(dev, tag, monkeypatch):
    m = make_module(tag, dev)
    for B in (1, 2, 3, 11):
        x, t = inputs(tag, B)
        new, n_new, old, n_old = both(m, x, t, dev, monkeypatch)
        assert (n_new, n_old) == (MERGED[tag], 0), (tag, B, n_new, n_old)
        assert torch.equal(new, old), (tag, B, float((new - old).abs().max()))
        routes = m._engine.conv_routes(dev)
        assert routes["t2"] == MERGED[tag]  # (counted as the launches it replaces: route hx2p, slot t2)


@pytest.mark.parametrize("tag", ["mnist32", "svhn"])
@pytest.mark.parametrize("wgs", ["1", "2", "3"])
def test_tile_walk_gives_the_same_bits(dev, tag, wgs, monkeypatch):
    """11 rows over 1, 2 or 3 workgroups along the tiles (svhn: two channel groups, so wgs = 1 is one workgroup per group
    too): each workgroup walks several tiles, the last ones fewer than the first."""
    m = make_module(tag, dev)
    x, t = inputs(tag, 11)
    base = m(x.to(dev), t.to(dev))
    monkeypatch.setenv("RGFM_HX2U_WGS", wgs)
    out = m(x.to(dev), t.to(dev))
    assert m._engine.up_merged(dev) == MERGED[tag]
    assert torch.equal(out, base)


@pytest.mark.parametrize("tag", ["mnist32", "svhn"])
def test_rows_do_not_depend_on_the_batch_and_match_the_oracle(dev, tag):
    m = make_module(tag, dev)
    desc, blob = oracle_net(tag)
    x, t = inputs(tag, 11)
    out = m(x.to(dev), t.to(dev))
    assert m._engine.up_merged(dev) > 0
    part = m(x[2:6].to(dev), t[2:6].to(dev))
    assert torch.equal(out[2:6], part)
    ro = O.unet_forward(desc, blob, x.numpy(), t.numpy())
    d = maxdiff(out.cpu().numpy(), ro)
    print(f"{tag}: 11 rows on the new kernel against the oracle: max|diff| {d:.2e}")
    assert d < TOL_EVAL


def test_shapes_it_declines(dev, monkeypatch):
    """An Upsample with 32 output channels ("deep": 8 -> 16, 32 channels) and a 14 <- 7 / 28 <- 14 net stay where they were."""
    cases = [("deep",) + make_sweep_unet("deep", 3, dev), ("unet28", make_module("unet28", dev)) + inputs("unet28", 3)]
    for name, m, x, t in cases:
        new, n_new, old, n_old = both(m, x, t, dev, monkeypatch)
        assert (n_new, n_old) == (0, 0), (name, n_new, n_old)
        assert torch.equal(new, old), name


@pytest.mark.parametrize("env", [{"RGFM_GN": "table"}, {"RGFM_GN": "table", "RGFM_FUSE_FIN": "0"}], ids=["table", "table-nofuse"])
@pytest.mark.parametrize("tag", ["mnist32", "svhn"])
def test_the_other_plumbings(dev, tag, env, monkeypatch):
    """RGFM_GN=table: the GroupNorm behind an Upsample is finalized by the last wave of the producing launch
    (fin_arrive, which the kernel implements) or, with RGFM_FUSE_FIN=0, by a gn_finalize launch."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = make_module(tag, dev)
    x, t = inputs(tag, 11)
    new, n_new, old, n_old = both(m, x, t, dev, monkeypatch)
    print(f"{tag} {env}: {n_new} Upsample conv(s) on the new kernel" + (" (it declined)" if n_new == 0 else ""))
    assert n_old == 0
    assert torch.equal(new, old)


@pytest.mark.parametrize("name", ["hi-up-t2", "lo-up-t2"])
def test_range_guard_on_the_new_kernel(dev, name, monkeypatch):
    """tests/range_cases.py's Upsample cases: the staged values' high side / the output's low side must raise the same
    flag word on the new kernel, and the guarded call must return the same result."""
    import copy
    cpu, x, t = R.unet_case(name)[:3]
    seen = {}
    for sw in ("1", "0"):
        m = copy.deepcopy(cpu).to(dev).eval()
        with monkeypatch.context() as mp:
            mp.setenv("RGFM_HX2U", sw)
            mp.setenv("RGFM_RANGE_CHECK", "0")
            m(x.to(dev), t.to(dev))
            torch.cuda.synchronize()
            merged, flag = m._engine.up_merged(dev), m._engine.read_range_flag(dev)
            mp.delenv("RGFM_RANGE_CHECK")
            before = _engine.range_fallbacks
            out = m(x.to(dev), t.to(dev))
            torch.cuda.synchronize()
            seen[sw] = (merged, flag, _engine.range_fallbacks - before, out)
    assert seen["1"][0] > 0 and seen["0"][0] == 0, (seen["1"][0], seen["0"][0])
    assert seen["1"][1] == seen["0"][1] == R.A_CASES[name]["bit"], (seen["1"][1], seen["0"][1])
    assert seen["1"][2] == seen["0"][2] == 1
    assert torch.equal(seen["1"][3], seen["0"][3])
