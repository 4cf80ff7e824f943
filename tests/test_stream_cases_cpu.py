"""The stream-case table (tests/stream_cases.py) against include/rgfm.h, without a GPU.

Every export whose parameter list has an rgfm_stream_t must be named by a row of the table or be listed in EXEMPT with
a one-line reason, so a new export fails here until it gets a stream case.  The test hooks (rgfm_*_dropout_mask,
rgfm_*_pool_choice, rgfm_clf_gate, rgfm_unet_conv_routes, ...) are documented as null-stream calls and take no
rgfm_stream_t: the parse does not see them and they need no entry."""
import os

import torch

import stream_cases as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def header_exports():
    with open(os.path.join(ROOT, "include", "rgfm.h")) as f:
        return S.stream_exports(f.read())


def test_the_parse_sees_the_header():
    ex = header_exports()
    assert len(ex) == len(set(ex)) and len(ex) >= 67
    for name in ("rgfm_unet_create", "rgfm_unet_forward", "rgfm_sample_pair", "rgfm_sample_two", "rgfm_sample_pair_cross_gs",
                 "rgfm_adam_step", "rgfm_clf_xent", "rgfm_fmnet_range_flag", "rgfm_guidance_apply_cross_rows"):
        assert name in ex, name
    # exports without a stream stay out: size queries, null-stream test hooks, handle settings
    for name in ("rgfm_unet_workspace_bytes", "rgfm_unet_dropout_mask", "rgfm_ratio_pool_choice", "rgfm_unet_set_conv_mode"):
        assert name not in ex, name


def test_every_stream_export_has_a_case_or_a_reason():
    ex = header_exports()
    covered = {e for c in S.CASES for e in c.exports}
    missing = [e for e in ex if e not in covered and e not in S.EXEMPT]
    assert not missing, f"stream-taking exports without a stream case (tests/stream_cases.py): {missing}"
    unknown = sorted((covered | set(S.EXEMPT)) - set(ex))
    assert not unknown, f"the table names exports that include/rgfm.h does not declare with a stream: {unknown}"
    both = sorted(covered & set(S.EXEMPT))
    assert not both, f"exempt and covered at once: {both}"
    for name, reason in S.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name
    # the exemptions are the calls that synchronise by contract, nothing else
    assert all(n.endswith("_create") or n.endswith("_range_flag") for n in S.EXEMPT)


def test_ids_are_unique_and_rows_are_well_formed():
    ids = [c.id for c in S.CASES]
    assert len(ids) == len(set(ids))
    assert S.BY_ID.keys() == set(ids)
    for c in S.CASES:
        assert c.exports and callable(c.build), c.id
        assert (c.fresh is not None) == c.id.endswith("_update_params"), c.id
        assert c.kind != "syncs" or c.fresh is not None, c.id


def test_poison_and_real_draws_differ_and_stay_inside_the_fp16_window():
    for c in S.CASES:
        real, again, poison = c.draw(0), c.draw(0), c.draw(1)
        assert list(real) == list(poison) and real, c.id
        for k, v in real.items():
            p = poison[k]
            assert torch.equal(v, again[k]), (c.id, k)  # (seeded: the null-stream run and the late run see the same values)
            assert v.shape == p.shape and v.dtype == p.dtype, (c.id, k)
            assert not torch.equal(v, p), (c.id, k)
            for t in (v, p):
                if t.is_floating_point():
                    assert torch.isfinite(t).all() and float(t.abs().max()) < S.FP16_WINDOW, (c.id, k)
            if v.is_floating_point() and v.numel() >= 64:  # same distribution and scale: the spreads agree
                assert 0.5 < float(v.std() / p.std()) < 2.0, (c.id, k)


def test_delay_rule():
    assert S.delay_for(0.0) == S.DELAY_FLOOR_MS == 20.0
    assert S.delay_for(35.0) == 70.0
