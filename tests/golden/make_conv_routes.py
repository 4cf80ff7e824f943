#!/usr/bin/env python3
"""Generate tests/golden/conv_routes.json: which conv kernel every launch of one eval forward goes to
(rgfm_unet_conv_routes), for the grid of small descriptors of tests/helpers.py (conv_route_cases).

Run on an MI355X with the library of the commit BEFORE a change of the conv dispatch -- check that commit out and build
it, or point RGFM_LIB at a build of it -- so that the fixture never comes from the code it then tests:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_conv_routes.py

Default run-time switches (the script refuses to run with an RGFM_* routing switch set).  The counts depend on the
device's CU count (launches with fewer workgroups than CUs are cut finer, which moves no launch to another route today,
but the file records the count it was made with).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

import torch  # noqa: E402

from helpers import conv_route_cases, conv_route_run  # noqa: E402
from ratio_guided_multimodal_fm_amd import _engine, models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.synth import load_synth  # noqa: E402


def main():
    set_ = sorted(k for k in os.environ if k.startswith("RGFM_") and k != "RGFM_LIB")
    assert not set_, f"unset {set_} first"
    dev = torch.device("cuda:0")
    cases = {}
    for key, cfg, seed, batches in conv_route_cases():
        m = load_synth(M.FlexibleUNet(**cfg), seed).eval().to(dev)
        for b in batches:
            before = _engine.range_fallbacks
            routes = conv_route_run(m, cfg, b, dev)[1]
            assert _engine.range_fallbacks == before, (key, b)  # (the default arithmetic's routes, not a fallback's)
            cases[f"{key}_b{b}"] = routes
            print(f"{key}_b{b}", {k: v for k, v in routes.items() if v})
    doc = {"compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "cases": cases}
    with open(os.path.join(HERE, "conv_routes.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
