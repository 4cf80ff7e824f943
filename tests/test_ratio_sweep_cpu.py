"""helpers.RATIO_SWEEP on the CPU: every entry is inside the domain the library accepts, the table covers the widths
and rasters it is there for, and every committed data seed meets the rule of tests/ratio_sweep_seeds.py -- the fp32
restatement of the encoders takes the float64 argmax in EVERY max-pool window, and the smallest float64 window gap is
at least 5 x the largest fp32-vs-float64 deviation of a pre-pool tensor (the conditions are the table's own, not a
tolerance of the code under test)."""
import ctypes

import pytest
import torch

import ratio_sweep_seeds as S
from helpers import RATIO_SWEEP, RATIO_SWEEP_TRAIN, make_sweep_ratio, sweep_ratio_inputs, sweep_ratio_kind
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd.synth import synth_state_dict


@pytest.mark.parametrize("tag,training", [(t, False) for t in RATIO_SWEEP] + [(t, True) for t in RATIO_SWEEP_TRAIN])
def test_committed_seed_meets_the_rule(tag, training):
    r = S.measure(tag, training=training)
    batch, seed = RATIO_SWEEP_TRAIN[tag] if training else RATIO_SWEEP[tag][6:]
    print(S.row(tag, seed, batch, r))
    assert r["agree"], (tag, r)
    assert r["ratio"] >= S.FLOOR, (tag, r)


def test_every_entry_is_accepted_by_the_library():
    """rgfm_ratio[_flex]_param_floats checks the descriptor (no device needed) and counts what the module holds."""
    L = _lib.lib()
    for tag, (xc, xs, yc, ys, feat, hid, batch, _) in RATIO_SWEEP.items():
        m = make_sweep_ratio(tag)
        n = ctypes.c_size_t()
        if sweep_ratio_kind(tag) == "flexible":
            d = _lib.RatioFlexDesc(feat, hid, 0, xc, yc, xs, ys)
            _lib.check(L.rgfm_ratio_flex_param_floats(ctypes.byref(d), ctypes.byref(n)))
        else:
            d = _lib.RatioDesc(0 if tag.startswith("ms_") else 1, feat, hid, 0)
            _lib.check(L.rgfm_ratio_param_floats(ctypes.byref(d), ctypes.byref(n)))
            shapes = m._engine.image_shapes()
            assert shapes == ((xc, xs, xs), (yc, ys, ys)), tag
        assert n.value == sum(v.numel() for v in m.state_dict().values()), tag
        x, y, cx, cy = sweep_ratio_inputs(tag)
        assert x.shape == (batch, xc, xs, xs) and y.shape == (batch, yc, ys, ys)
        assert cx.shape == (3, xc, xs, xs) and cy.shape == (2, yc, ys, ys)


def test_the_table_covers_the_widths_and_rasters():
    feats = {e[4] for e in RATIO_SWEEP.values()}
    hids = {e[5] for e in RATIO_SWEEP.values()}
    assert {64, 192, 320, 512} <= feats and {128, 384, 640, 1024} <= hids
    flex = {t: e for t, e in RATIO_SWEEP.items() if sweep_ratio_kind(t) == "flexible"}
    assert flex["y64"][4:6] != (64, 128)
    assert {e[4:6] for t, e in flex.items() if max(e[1], e[3]) > 32} != {(64, 128)}
    sizes = {s for e in flex.values() for s in (e[1], e[3])}
    assert {64, 63, 56, 48, 40, 36, 33, 25, 17, 15, 9, 8} <= sizes
    assert any(e[1] == 64 for e in flex.values()) and any(e[3] == 64 for e in flex.values())  # on either encoder
    levels = [{s >> l for s in sizes} for l in range(4)]
    assert any(17 <= s <= 32 for s in levels[1])  # a multi-tile level-2 raster
    assert any(9 <= s <= 16 for s in levels[2])   # a level-3 raster of one-sample tiles
    assert any(5 <= s <= 8 for s in levels[3])    # conv4 on more than 16 pixels
    assert {t: e[4:6] for t, e in RATIO_SWEEP.items() if sweep_ratio_kind(t) != "flexible"} == \
        {"ms_64": (64, 128), "ms_192": (192, 640), "ms_512": (512, 1024), "r28_512": (512, 1024)}
    assert {e[6] for t, e in flex.items() if max(e[1], e[3]) == 8} == {5}
    assert set(RATIO_SWEEP_TRAIN) == {t for t in RATIO_SWEEP if sweep_ratio_kind(t) == "mnist_svhn"}


def test_encoder_weights_do_not_depend_on_the_widths():
    """load_synth draws a tensor from (seed, position, shape) alone, and only the encoders' Linear has a shape that
    depends on feature_dim: everything in front of the max-pools is bitwise the same at every width, which is why the
    three "ms_" entries share their searched seeds."""
    a, b = (synth_state_dict(make_sweep_ratio(t), 16) for t in ("ms_64", "ms_512"))
    keys = [k for k in a if k.startswith("encoder") and ".fc." not in k]
    assert len(keys) == 12 * 7 and all(torch.equal(a[k], b[k]) for k in keys)
    assert a["encoder_mnist.fc.weight"].shape != b["encoder_mnist.fc.weight"].shape
