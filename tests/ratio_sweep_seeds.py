"""Data seeds of helpers.RATIO_SWEEP: the rule, the search and the measured table.

    python tests/ratio_sweep_seeds.py                 # the table of the committed seeds
    python tests/ratio_sweep_seeds.py --search [tag]  # run the search again (every entry, or one)
    python tests/ratio_sweep_seeds.py --collect tag N # the first N single-row seeds of an entry (helpers.RATIO_ROW_SEEDS)

A max-pool whose two largest window elements nearly tie may route differently in another fp32 arithmetic or in float64:
a discontinuity of the function's gradient, not an arithmetic error (tests/test_gpu_ratio_flex.py,
tests/golden/make_ratio_train_golden.py).  This module restates the encoders of the three estimator kinds in plain
torch.nn.functional over the module's own state_dict, in the dtype of the tensors it is handed, and runs the restatement
in fp32 against the same in float64.  measure() returns, for an entry and a seed,

    windows    the number of 2x2 max-pool windows of the entry's batch (both encoders, every pool),
    gap        the smallest float64 gap between the two largest elements of a window,
    dev        the largest fp32-vs-float64 deviation of a pre-pool tensor,
    agree      whether the fp32 run takes the float64 argmax in every window.

The rule.  An entry's seed is the first of BASE[tag] .. BASE[tag] + 999 with agree and gap >= 10 dev; where none of the
1000 qualifies, the one with the largest gap / dev among those that agree, which must reach 5 (the weakest seed the
existing flexible tests rest on has 5.1) -- otherwise the entry's batch goes down by one and the search starts again.
RatioEstimatorMNISTSVHN normalises with batch statistics in training mode, so its pre-pool tensors differ between the
modes and the rule is applied to each mode on its own: helpers.RATIO_SWEEP has the batch and seed of an "ms_" entry in
eval mode (evaluation, cross matrix, both gradients, the eval-mode training pass), helpers.RATIO_SWEEP_TRAIN those of
its training-mode pass.  One seed for both modes does not exist among the candidates: the smaller of a candidate's two
ratios stays below 4.4 at batch 1 and below 3.1 at batch 2.  The GroupNorm kinds have one mode.

load_synth draws every tensor from (seed, position in state_dict) and its own shape, and the encoders' Linear is the
only encoder tensor whose shape depends on feature_dim: the conv and norm tensors in front of the pools are the same at
every (feature_dim, hidden_dim).  The three "ms_" entries therefore share one search per mode (BASE is the same), and
tests/test_ratio_sweep_cpu.py still recomputes every entry on its own module.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import ratio_ref64 as RR  # noqa: E402
from helpers import RATIO_SWEEP, RATIO_SWEEP_TRAIN, make_sweep_ratio, sweep_ratio_inputs, sweep_ratio_kind  # noqa: E402

EPS = 1e-5
CANDIDATES, TEN, FLOOR = 1000, 10.0, 5.0
# first candidate per entry
BASE = {"s64": 2000, "s63": 2100, "s48": 2200, "s56": 2300, "s36": 2400, "y64": 2500, "w192": 2600, "w320": 2700,
        "w512": 2800, "w64h": 2900, "w512n": 3000, "ms_64": 3100, "ms_192": 3100, "ms_512": 3100, "r28_512": 3400}


def encoder_prepool(kind, sd, img, side, training=False):
    """The activated maps in front of the max-pools of one encoder (side 0 = x, 1 = y), in the dtype of `sd`; the pools
    take the true maximum of that dtype.  Layer tables: ratio_ref64.ENCODERS (the flexible kind has the GroupNorm
    encoders of "mnist28" under the same keys)."""
    prefix, layers = RR.ENCODERS["mnist28" if kind == "flexible" else kind][side]
    h = img.to(sd[f"{prefix}.fc.weight"].dtype)
    pre = []
    for conv, norm, pool in layers:
        z = F.conv2d(h, sd[f"{prefix}.{conv}.weight"], sd[f"{prefix}.{conv}.bias"], padding=1)
        g, b = sd[f"{prefix}.{norm}.weight"], sd[f"{prefix}.{norm}.bias"]
        if kind == "mnist_svhn":
            if training:
                mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
            else:
                mean, var = sd[f"{prefix}.{norm}.running_mean"], sd[f"{prefix}.{norm}.running_var"]
            zn = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
            zn = zn * g[None, :, None, None] + b[None, :, None, None]
        else:
            zn = F.group_norm(z, 8, g, b, eps=EPS)
        h = F.silu(zn)
        if pool:
            pre.append(h)
            h = RR.windows(h).max(-1).values
    return pre


def state(module, dtype):
    return {k: v.detach().to("cpu", dtype) for k, v in module.state_dict().items() if v.is_floating_point()}


def measure_pair(kind, sd32, sd64, x, y, training=False):
    """(windows, gap, dev, agree) of one batch in one mode."""
    windows, gap, dev, agree = 0, float("inf"), 0.0, True
    for side, img in enumerate((x, y)):
        p32 = encoder_prepool(kind, sd32, img, side, training)
        p64 = encoder_prepool(kind, sd64, img, side, training)
        for a, t in zip(p32, p64):
            w64, w32 = RR.windows(t), RR.windows(a)
            top = w64.topk(2, dim=-1).values
            windows += top[..., 0].numel()
            gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
            dev = max(dev, float((a.double() - t).abs().max()))
            agree = agree and bool((w32.argmax(-1) == w64.argmax(-1)).all())
    return windows, gap, dev, agree


_states = {}


def measure(tag, seed=None, batch=None, training=False):
    """dict(windows, gap, dev, ratio, agree) of RATIO_SWEEP[tag] at `seed` and `batch` (default: the committed ones of
    that mode); `training` matters for the BatchNorm kind only."""
    kind = sweep_ratio_kind(tag)
    if tag not in _states:
        m = make_sweep_ratio(tag)
        _states[tag] = state(m, torch.float32), state(m, torch.float64)
    sd32, sd64 = _states[tag]
    if training and seed is None:
        batch, seed = RATIO_SWEEP_TRAIN[tag]
    x, y, _, _ = sweep_ratio_inputs(tag, batch, seed)
    with torch.no_grad():
        w, gap, dev, agree = measure_pair(kind, sd32, sd64, x, y, training)
    return dict(windows=w, gap=gap, dev=dev, ratio=gap / dev, agree=agree)


def search(tag, batch, training=False):
    """(seed, measurement, rule) at `batch`: rule 'ten_times' or 'best_ratio'; seed None where no candidate agrees and
    reaches FLOOR."""
    best = None
    for seed in range(BASE[tag], BASE[tag] + CANDIDATES):
        r = measure(tag, seed, batch, training)
        if not r["agree"]:
            continue
        if r["ratio"] >= TEN:
            return seed, r, "ten_times"
        if best is None or r["ratio"] > best[1]["ratio"]:
            best = (seed, r)
    if best is None or best[1]["ratio"] < FLOOR:
        return None, best[1] if best else None, "none"
    return best[0], best[1], "best_ratio"


def collect(tag, count, training=False):
    """[(seed, measurement, rule)]: the first `count` candidates of BASE[tag] .. BASE[tag] + 999 that satisfy the rule at
    batch 1 (agree and gap >= 10 dev), in candidate order; where fewer do, filled up with the agreeing candidates of the
    largest gap / dev that reach FLOOR ('best_ratio'), so the list may stay shorter than `count`.  The rows of an
    eval-mode RatioEstimatorMNISTSVHN are independent, so a batch stacked from such single-row seeds
    (helpers.RATIO_ROW_SEEDS, helpers.stacked_ratio_inputs) keeps every row's margin."""
    ten, rest = [], []
    for seed in range(BASE[tag], BASE[tag] + CANDIDATES):
        r = measure(tag, seed, 1, training)
        if not r["agree"]:
            continue
        if r["ratio"] >= TEN:
            ten.append((seed, r, "ten_times"))
            if len(ten) == count:
                return ten
        elif r["ratio"] >= FLOOR:
            rest.append((seed, r, "best_ratio"))
    rest.sort(key=lambda c: -c[1]["ratio"])
    return ten + rest[:count - len(ten)]


def row(tag, seed, batch, r, note=""):
    return (f"{tag:18s} seed {seed} batch {batch} windows {r['windows']:7d} gap {r['gap']:.3e} dev {r['dev']:.3e} "
            f"ratio {r['ratio']:5.1f} agree {r['agree']} {note}")


def main(argv):
    torch.set_num_threads(int(os.environ.get("RATIO_SWEEP_THREADS", "4")))
    if argv and argv[0] == "--search":
        jobs = [(tag, False, RATIO_SWEEP[tag][6]) for tag in (argv[1:] or list(RATIO_SWEEP))]
        jobs += [(tag, True, RATIO_SWEEP_TRAIN[tag][0]) for tag, _, _ in jobs if tag in RATIO_SWEEP_TRAIN]
        for tag, training, batch in jobs:
            name = tag + (" (training)" if training else "")
            batch = int(os.environ.get("RATIO_SWEEP_BATCH", batch))  # (where to start going down from)
            while batch >= 1:
                seed, r, rule = search(tag, batch, training)
                if seed is not None:
                    print(row(name, seed, batch, r, rule), flush=True)
                    break
                print(f"{name:18s} batch {batch}: no candidate reaches {FLOOR} (best {r['ratio'] if r else float('nan'):.1f})", flush=True)
                batch -= 1
        return 0
    if argv and argv[0] == "--collect":
        for seed, r, rule in collect(argv[1], int(argv[2])):
            print(row(argv[1], seed, 1, r, rule), flush=True)
        return 0
    for tag, e in RATIO_SWEEP.items():
        print(row(tag, e[7], e[6], measure(tag)))
    for tag, (batch, seed) in RATIO_SWEEP_TRAIN.items():
        print(row(tag + " (training)", seed, batch, measure(tag, training=True)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
