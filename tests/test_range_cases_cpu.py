"""The cases of tests/range_cases.py on the CPU, from float64 alone: each edit puts the tensors it targets outside the
fp16 window by the margin its GPU test relies on (or just inside / just outside it), and leaves every other recorded
tensor of the net, and the output, ordinary -- so that on the GPU only the launches that touch the targeted stretch can
raise the range flag."""
import numpy as np
import pytest
import torch

import range_cases as R

WINDOW = (2.0 ** -4, 128.0)  # every tensor that is NOT targeted: its (sample, 32-channel block) maxima


def check_others(acts, targeted, what):
    for i, a in enumerate(acts[:-1]):  # (the last entry is v)
        if i in targeted:
            continue
        bm = R.block_maxima(a)
        assert WINDOW[0] <= bm.min() and bm.max() <= WINDOW[1], (what, i, float(bm.min()), float(bm.max()))


def check_output(v, what):
    assert np.isfinite(v).all() and 2.0 ** -4 <= np.abs(v).max() <= 16.0, (what, float(np.abs(v).max()))


def test_topology_is_the_trace_order():
    """The trace indices scale_pair hands out are forward64's: a scaled producer scales exactly the activation it
    names and nothing in front of it."""
    m0, x, t = R.make_unet("r16", 3)
    _, acts0 = R.trace64(m0, x, t)
    for name, kind, ins, out, act in R.topology(m0):
        if kind == "res" and not isinstance(m0.get_submodule(name).skip, torch.nn.Conv2d):
            continue  # (an identity block adds its unscaled input back)
        m, _, _ = R.make_unet("r16", 3)
        targeted, readers = R.scale_pair(m, name, 4.0)
        assert targeted[0] == act and (readers or name == "decoder_blocks.3"), name  # (only out_norm reads the last block)
        _, acts = R.trace64(m, x, t)
        np.testing.assert_allclose(acts[act], 4.0 * acts0[act], rtol=1e-12)
        for i in range(act):  # (nothing in front of the producer moves)
            assert np.array_equal(acts[i], acts0[i]), (name, i)
        if name == "decoder_blocks.2":
            # its only reader is decoder_blocks.3, whose norm1 groups do not straddle the concat (32 + 32 channels in
            # groups of 8): behind the compensated skip slice the net is the unedited one again (up to the norm's eps)
            for i in range(act + 1, len(acts)):
                np.testing.assert_allclose(acts[i], acts0[i], rtol=1e-4, atol=1e-4, err_msg=f"{name} {i}")
    assert len(acts0) == R.topology(m0)[-1][4] + 2  # (the last block's output, then v)


def test_an_identity_block_cannot_be_made_small():
    m, _, _ = R.make_unet("r16", 3)
    with pytest.raises(ValueError):
        R.scale_pair(m, "middle_block1", 2.0 ** -15)


@pytest.mark.parametrize("name", list(R.A_CASES))
def test_part_a_case(name):
    c = R.A_CASES[name]
    m, x, t, targeted, readers, v, acts = R.unet_case(name)
    assert readers, name
    for i in targeted:
        bm = R.block_maxima(acts[i])
        print(f"{name}: targeted tensor {i} block maxima [{bm.min():.3g}, {bm.max():.3g}]")
        if c["bit"] == R.HIGH:
            assert bm.max() >= 8192.0, (name, i, float(bm.max()))
        else:
            assert 0.0 < bm.min() and bm.max() <= 2.0 ** -10, (name, i, float(bm.min()), float(bm.max()))
    check_others(acts, targeted, name)
    check_output(v, name)
    if c["routes"] is None:
        assert c["net"] in R.ROUTES


@pytest.mark.parametrize("name", list(R.B_CASES))
def test_part_b_case(name):
    c = R.B_CASES[name]
    m, x, t, targeted, readers, v, acts = R.unet_case(name)
    lo, hi = c["window"]
    for i in targeted:
        bm = R.block_maxima(acts[i])
        print(f"{name}: targeted tensor {i} block maxima [{bm.min():.3g}, {bm.max():.3g}]")
        if c["bit"] == R.HIGH:
            assert lo <= bm.max() <= hi, (name, i, float(bm.max()))
        else:
            assert lo <= bm.min() and bm.max() <= hi, (name, i, float(bm.min()), float(bm.max()))
    check_others(acts, targeted, name)
    check_output(v, name)


@pytest.mark.parametrize("name", list(R.ROW_CASES))
def test_row_case(name):
    m, x, t, row, v, h0 = R.row_case(name)
    lg = R.ROW_CASES[name][3]
    assert float(m.input_conv.bias.detach().abs().max()) == 0.0
    bm = R.block_maxima(h0)
    others = np.delete(bm, row, axis=0)
    print(f"{name}: first-level stream of row {row} [{bm[row].min():.3g}, {bm[row].max():.3g}], of the others "
          f"[{others.min():.3g}, {others.max():.3g}]")
    if lg > 0:
        assert bm[row].max() >= 8192.0
    else:
        assert 0.0 < bm[row].min() and bm[row].max() <= 2.0 ** -10
    assert WINDOW[0] <= others.min() and others.max() <= WINDOW[1]
    assert np.isfinite(v).all()
    per_row = np.abs(v).reshape(v.shape[0], -1).max(axis=1)
    assert 2.0 ** -4 <= per_row.min() and per_row.max() <= 16.0, (float(per_row.min()), float(per_row.max()))


@pytest.mark.parametrize("name", list(R.NORM_CASES))
def test_norm_case(name):
    gamma, beta, _, inside = R.NORM_CASES[name]
    g, b = np.float32(gamma), np.float32(beta)
    hi, lo = np.float32(8.0) * abs(g) + abs(b), max(abs(g), abs(b))  # norm_params_ok, in its fp32
    assert bool(hi < np.float32(1024.0) and lo >= np.float32(0.015625)) == inside, (name, hi, lo)
    if name.startswith("hi"):
        assert abs(float(hi) - 1024.0) <= 0.11 and lo >= 0.015625  # just under / just over the ceiling, the floor untouched
    else:
        assert float(lo) in (2.0 ** -6, 2.0 ** -7) and hi < 1024.0
    m, x, t, v, acts = R.norm_case(name)
    blk = m.get_submodule(R.NORM_BLOCK)
    w = blk.norm2.weight.detach()
    assert float(w.min()) == float(w.max()) == float(g)
    check_others(acts, (), name)
    check_output(v, name)


def test_wino_case():
    """The Winograd cell: norm1's parameters pass norm_params_ok, the staged maximum S_A max stays under the fp16 limit
    the direct kernels test, 4 S_A max is over it; conv1's output and everything else stay ordinary."""
    m, x, t, v, acts, staged = R.wino_case()
    hi = np.float32(8.0) * np.float32(R.WINO_GAMMA) + np.float32(R.WINO_BETA)
    assert hi < np.float32(1024.0) and max(R.WINO_GAMMA, R.WINO_BETA) >= 0.015625
    smax = 16.0 * float(np.abs(staged).max())
    print(f"wino: staged S_A silu(norm1) max {smax:.4g}, 4 x {4 * smax:.4g} (limit 32760)")
    assert 1.25 * smax < 32760.0 < 4.0 * smax / 1.25
    check_others(acts, (), "wino")
    check_output(v, "wino")


# ------------------------------------------------------------------ part D: the edited loop net
@pytest.mark.parametrize("bit", [R.HIGH, R.LOW])
def test_part_d_net(bit):
    """The edited g16 at the loops' start state and at three times: the targeted tensor outside the window, the rest
    ordinary; and the producer's only raw reader is the next decoder block."""
    from helpers import make_generic_unet
    m = make_generic_unet("g16")[0]
    targeted, readers = R.scale_pair(m, R.D_PRODUCER, 2.0 ** R.D_LG[bit])
    assert readers == ["decoder_blocks.14"] and len(targeted) == 1
    x0 = R.d_inputs()["x0"]
    for tv in R.D_TRACE_T:
        v, acts = R.trace64(R.d_net(bit), x0, torch.tensor([tv]))
        bm = R.block_maxima(acts[targeted[0]])
        print(f"part D bit {bit} t = {tv}: targeted block maxima [{bm.min():.3g}, {bm.max():.3g}]")
        if bit == R.HIGH:
            assert bm.max() >= 8192.0
        else:
            assert 0.0 < bm.min() and bm.max() <= 2.0 ** -10
        check_others(acts, targeted, ("D", bit, tv))
        check_output(v, ("D", bit, tv))


def test_part_d_tables():
    assert set(R.D_STAGE_SCALE) == {"euler", "midpoint"}
    assert len(R.D_STAGE_SCALE["euler"]) == R.D_STEPS and len(R.D_STAGE_SCALE["midpoint"]) == 2 * R.D_STEPS
    assert all(0.0 in s[1:] for s in R.D_STAGE_SCALE.values())  # (a zero stage behind t = 0, which is unguided anyway)
    assert len(R.D_GAMMA_ROWS) == R.D_B == R.d_inputs()["x0"].shape[0]
    # the float64 loops see the edit: the guided end states differ from the unguided ones, the edited net's from g16's
    for bit in (R.HIGH, R.LOW):
        a, b = R.d_want("pair-mc", bit, "euler"), R.d_want("pair", bit, "euler")
        assert max(float(np.abs(p - q).max()) for p, q in zip(a, b)) > 1e-2
        assert all(np.isfinite(p).all() for p in a)


# ------------------------------------------------------------------ parts D and F: FlowMatchingModel
@pytest.mark.parametrize("bit", [R.HIGH, R.LOW])
def test_fm_case(bit):
    i = R.fm_inputs()
    bm = R.block_maxima(R.fm_map64(R.fm_net(bit), i["x"], i["t"]))
    base = R.block_maxima(R.fm_map64(R.fm_net("x"), i["x"], i["t"]))
    print(f"FlowMatchingModel bit {bit}: fc1 map block maxima [{bm.min():.3g}, {bm.max():.3g}] (unedited [{base.min():.3g}, {base.max():.3g}])")
    assert WINDOW[0] <= base.min() and base.max() <= WINDOW[1]
    if bit == R.HIGH:
        assert bm.min() >= 8192.0  # (every block, not only the largest)
    else:
        assert 0.0 < bm.min() and bm.max() <= 2.0 ** -10
    check_output(R.fm_want("forward", bit)[0], ("fm", bit))


# ------------------------------------------------------------------ part E: the edited estimators
@pytest.mark.parametrize("bit", [R.HIGH, R.LOW])
def test_part_e_rows_meet_the_seed_rule_on_the_edited_module(bit):
    """As tests/test_grad_loop_cpu.py does for the committed rows: every row alone, on the EDITED BatchNorm estimator."""
    import ratio_sweep_seeds as S
    from helpers import sweep_ratio_inputs
    rr = R.e_case("ms", "pair", bit)["rr"]
    sd32, sd64 = S.state(rr, torch.float32), S.state(rr, torch.float64)
    with torch.no_grad():
        for seed in R.E_MS_SEEDS[bit]:
            x, y, _, _ = sweep_ratio_inputs("ms_64", 1, seed)
            w, gap, dev, agree = S.measure_pair("mnist_svhn", sd32, sd64, x, y)
            print(f"part E bit {bit} seed {seed}: windows {w} gap {gap:.3e} dev {dev:.3e} gap / dev {gap / dev:.2f}")
            assert agree and gap >= S.FLOOR * dev, (seed, gap, dev, agree)
    z = np.abs(R.e_staged64(bit))
    bm = R.block_maxima(z)
    print(f"part E bit {bit}: the layer conv2b stages, block maxima [{bm.min():.3g}, {bm.max():.3g}]")
    if bit == R.HIGH:
        assert bm.max() >= 8192.0  # (silu(z) ~ z up there: S_A silu(z) is far beyond fp16)
    else:
        assert 0.0 < bm.max() <= 2.0 ** -13  # (silu(z) ~ z / 2: staged below 2^-10 of the two-plane floor's reach)


@pytest.mark.parametrize("kind", ["r28", "flex"])
def test_part_e_groupnorm_edits_leave_the_pools_alone(kind):
    """gn4 is behind every pool: the edited module has the pre-pool maps, bit for bit, of the unedited one, whose rows
    tests/test_ratio_sweep_cpu.py and tests/test_cond_grad_cpu.py hold to the seed rule."""
    import cond_grad_ref64 as CG
    import grad_loop_ref64 as GL
    import ratio_sweep_seeds as S
    for bit in (R.HIGH, R.LOW):
        c = R.e_case(kind, "pair" if kind == "r28" else "cond", bit)
        base = GL.estimator("r28_512", "disc", 0) if kind == "r28" else CG.sampler_case("x")[0]
        rkind = "mnist28" if kind == "r28" else "flexible"
        side = 0 if kind == "r28" else 1
        img = c["s0"][0]
        with torch.no_grad():
            a = S.encoder_prepool(rkind, S.state(c["rr"], torch.float64), img, side)
            b = S.encoder_prepool(rkind, S.state(base, torch.float64), img, side)
        assert len(a) == 3 and all(torch.equal(p, q) for p, q in zip(a, b))
        assert not torch.equal(getattr(c["rr"], R.E_GN_EDIT[kind][0]).gn4.weight, getattr(base, R.E_GN_EDIT[kind][0]).gn4.weight)


@pytest.mark.parametrize("kind,loop,bit", R.E_CASES)
def test_part_e_case_is_admissible(kind, loop, bit):
    """grad_loop_ref64's condition on the inputs: rho <= 0.1 TOL_GRAD max|g64_side|, G a power of two."""
    import grad_loop_ref64 as GL
    c = R.e_case(kind, loop, bit)
    for (rho, limit), gamma, g in zip(GL.admissible(c), c["gamma"], c["g64"]):
        gmax = float(g.abs().max())
        print(f"part E {kind} {loop} bit {bit}: max|g64| {gmax:.3e} G {gamma:g} rho {rho:.3e} (admissible up to {limit:.3e})")
        assert 0.5 < gamma * GL.DT * gmax <= 1.0 and rho <= limit, (rho, limit)
