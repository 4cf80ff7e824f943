#!/usr/bin/env python3
"""Generate tests/golden/fmnet_eval.npz from the reference's own fp32 forward.

Run where a checkout of the reference project is at hand (it never travels with this repository):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fmnet_eval_golden.py REFERENCE_DIR

For every case of tests/fmnet_ref64.py:EVAL_CASES -- the reference FlowMatchingModel at the case's (feature_dim,
time_emb_dim), filled with this repo's synthetic parameters (ratio_guided_multimodal_fm_amd/synth.py, seed SEED_W), on
the case's seeded x and t -- the fp32 CPU output of the reference module at 256 seeded positions (`probe_idx_i`,
`probe_v32_i`) and its largest deviation from the float64 restatement over the whole output (`ref32_err_cases[i]`): the
reference's own fp32 error, which the tolerance of tests/test_gpu_fmnet_eval.py is weighed against.  Also the cases,
the seed and a fingerprint of each case's inputs, so that a fixture of other cases is noticed.  Data only, no reference
source.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fmnet_ref64 as R  # noqa: E402
from ratio_guided_multimodal_fm_amd.synth import synth_state_dict  # noqa: E402
from src.models.flow_matching import FlowMatchingModel as RefFlowMatchingModel  # noqa: E402

N_PROBE = 256


def main():
    out = {"cases": np.asarray([[f, t, b, int(s)] for f, t, b, s in R.EVAL_CASES], np.int64),
           "seed": np.int64(R.SEED_W)}
    errs = []
    for ci, (F_dim, T_dim, B, _) in enumerate(R.EVAL_CASES):
        m = RefFlowMatchingModel(1, F_dim, T_dim)
        m.load_state_dict(synth_state_dict(m, R.SEED_W))
        m.eval()
        x, t = R.eval_inputs(ci)
        with torch.no_grad():
            v32 = m(x, t.expand(B)).numpy()
        err = float(np.abs(v32.astype(np.float64) - R.eval_ref(ci)).max())
        errs.append(err)
        print(f"F={F_dim} T={T_dim} B={B}: ref32_err = {err:.3e}")
        idx = torch.randint(0, v32.size, (N_PROBE,), generator=torch.Generator().manual_seed(7100 + ci)).numpy()
        out[f"probe_idx_{ci}"] = idx
        out[f"probe_v32_{ci}"] = v32.reshape(-1)[idx]
        out[f"x_fp_{ci}"] = x.reshape(-1)[:8].numpy()
        out[f"t_{ci}"] = t.numpy()
    out["ref32_err_cases"] = np.asarray(errs, np.float64)
    np.savez_compressed(os.path.join(HERE, "fmnet_eval.npz"), **out)


if __name__ == "__main__":
    main()
