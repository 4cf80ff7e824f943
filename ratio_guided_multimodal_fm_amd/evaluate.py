"""Coherence evaluation of generated 28x28 pairs (reference ``src/evaluate.py``).

``get_inverse_transform`` (``:31-54``), ``evaluate_coherence`` (``:57-96``) and the sweep of ``main``
(``:99-240``) with its flags, skip rule and JSON schema
(``method, guidance_strength, transform_type, coherence_acc, num_samples``).

The reference un-rotates y with ``torchvision.transforms.functional.rotate`` (nearest, about the
image centre); for the multiples of 90 degrees it uses on a square image that is the exact pixel
permutation ``torch.rot90`` (counter-clockwise for positive angles), which is what is used here --
torchvision is not a dependency of this package.  Sampling runs on the HIP path, the classifier once
per configuration in PyTorch-ROCm.
"""
import argparse
import json
import os

import torch

from .models.classifier import MNISTClassifier
from .models.ratio_estimator import RatioEstimator
from .sample import add_common_args, build_flow_models
from .utils import load_checkpoint, set_seed
from .utils.diagnostics import GuidanceDiagnostics, add_cli_args as add_diagnostics_args, row_metrics
from .utils.flow_utils import (add_ess_arg, add_label_args, add_sde_args, ess_from_cli, labels_from_cli, sde_from_cli, add_pairing_arg,
                               sample_bimodal_guided, shared_mc_sweep)
from .utils.guidance_schedule import add_cli_args as add_schedule_args, from_cli as schedule_from_cli
from .utils.path_utils import get_checkpoint_path


def get_inverse_transform(transform_type):
    """Function undoing the y-modality transform; unknown names are the identity (reference :53-54)."""
    table = {
        'rotate90': lambda img: torch.rot90(img, 1, (-2, -1)),    # TF.rotate(img, 90)
        'rotate180': lambda img: torch.rot90(img, 2, (-2, -1)),   # TF.rotate(img, 180)
        'rotate270': lambda img: torch.rot90(img, -1, (-2, -1)),  # TF.rotate(img, -90)
        'invert': lambda img: -img,
        'flip_h': lambda img: torch.flip(img, (-1,)),
        'flip_v': lambda img: torch.flip(img, (-2,)),
    }
    return table.get(transform_type, lambda img: img)


def evaluate_coherence(samples_x, samples_y, classifier, device, transform_type='rotate90'):
    """P(argmax clf(x) == argmax clf(inverse_transform(y))); returns the reference's dict."""
    classifier.eval()
    y_inv = get_inverse_transform(transform_type)(samples_y)
    with torch.no_grad():
        pred_x = classifier(samples_x.to(device)).argmax(dim=1)
        pred_y = classifier(y_inv.to(device)).argmax(dim=1)
    acc = (pred_x == pred_y).float().mean().item() if len(samples_x) else float('nan')
    return {'coherence_acc': float(acc), 'num_samples': len(samples_x)}


def label_accuracy(samples, classifier, labels, device, num_classes=None):
    """Share of the rows whose class the classifier predicts as the requested label; rows with the null label
    (`num_classes`) are left out.  nan without rows."""
    classifier.eval()
    labels = torch.as_tensor(labels).to(device).reshape(-1)
    with torch.no_grad():
        pred = classifier(samples.to(device)).argmax(dim=1)
    keep = labels != num_classes if num_classes is not None else torch.ones_like(labels, dtype=torch.bool)
    return float((pred[keep] == labels[keep]).float().mean().item()) if int(keep.sum()) else float('nan')


def run_sweep(fm_x, fm_y, make_ratio, classifier, methods, strengths, num_samples, num_steps, device,
              mc_batch_size, transform_type, sampler=sample_bimodal_guided, solver='euler', diagnostics=False,
              mc_pairing='paired', shared_mc=False, guidance_schedule=None, sde_eta=0.0, sde_seed=None, ess_floor=None,
              labels=None, cfg_scale=1.0):
    """The reference's nested loop (:165-222). `make_ratio()` returns a fresh ratio estimator or None.
    `solver` ('euler' | 'midpoint') goes to `sampler` as a keyword when it is not the default.
    `diagnostics`: every guided row also gets ess_mean, ess_min and w_max of the importance weights at step
    int(0.3 * num_steps) (utils/diagnostics.py); without it the rows keep exactly their keys.
    `mc_pairing` = 'cross': the 'mc_feng' configurations guide over all mc_batch_size ** 2 pairs of the MC set (the
    sampler's `mc_pairing` keyword) and their rows record ``"mc_pairing": "cross"``; 'paired' rows keep their keys.
    `guidance_schedule` (utils/guidance_schedule.py) goes to `sampler` as a keyword when it is given.
    `shared_mc`: all strengths of a guided method run as ONE sampler call of ``len(strengths) * num_samples`` rows,
    row block j carrying strength j, over one MC set, one pre-phase and one start-noise set repeated per block
    (``utils.flow_utils.shared_mc_sweep``): the strengths' numbers then differ by the strength alone.  Every row of
    the result gains ``"shared_mc": true``.  The default sampler only (no sharded form).
    `sde_eta` > 0: every sampler call takes Euler-Maruyama steps (``paired_sampler``; `sde_seed` None: each call draws its
    own seed after its other draws); the keywords go to `sampler` only then, and every row gains ``"sde_eta"``.
    `ess_floor`: the 'mc_feng' configurations hold their importance weights to this effective sample size
    (``paired_sampler``; the sampler's `ess_floor` keyword) and their rows record ``"ess_floor"``; it goes with no
    gradient method among `methods` (they have no weights: ``RgfmError``) and has no sharded form.  None: nothing changes.
    `labels` (an integer tensor [num_samples]) with `cfg_scale`: the class-conditional baseline.  The 'none' configuration
    samples both nets with these labels (``paired_sampler``) and its row gains ``"labelled": true``, ``"cfg_scale"`` and
    ``label_accuracy_x`` / ``label_accuracy_y`` -- the classifier's prediction on x and on the inverse-transformed y against the requested label (null-label
    rows left out) -- beside the coherence.  It goes with no guided method among `methods` and has no sharded form
    (``RgfmError``).  None: nothing changes."""
    from ._lib import solver_id
    from .utils.flow_utils import check_pairing
    solver_id(solver)
    check_pairing(mc_pairing)
    kw = {'solver': solver} if solver != 'euler' else {}
    if guidance_schedule is not None:
        kw['guidance_schedule'] = guidance_schedule
    sde = {'sde_eta': float(sde_eta), 'sde_seed': sde_seed} if sde_eta else {}
    sde_row = {'sde_eta': float(sde_eta)} if sde_eta else {}
    kw.update(sde)
    if ess_floor is not None:
        from ._lib import RgfmError
        if any(m not in ('none', 'mc_feng') for m in methods):
            raise RgfmError(f"ess_floor tempers the importance weights of 'mc_feng'; {list(methods)} holds a gradient method, "
                            "which has no weights: sweep it in a run of its own")
        if sampler is not sample_bimodal_guided:
            raise RgfmError("ess_floor has no sharded form: run the tempered sampler on one device")
    if shared_mc and sampler is not sample_bimodal_guided:
        raise ValueError("shared_mc runs the default sampler: it has no sharded form")
    if labels is not None:
        from ._lib import RgfmError
        if any(m != 'none' for m in methods):
            raise RgfmError(f"labels go with the 'none' method alone (the supervised baseline); {list(methods)} holds a guided "
                            "method: sweep it without labels, in a run of its own")
        if sampler is not sample_bimodal_guided:
            raise RgfmError("labels have no sharded form: run the labelled sampler on one device")
    lab_kw = {'labels': labels, 'cfg_scale': float(cfg_scale)} if labels is not None else {}
    results = []
    for method in methods:
        # `extra` (below): what an 'mc_feng' configuration adds, to the sampler's keywords and to its result rows alike
        if shared_mc and method != 'none':
            ratio = make_ratio()
            if ratio is None:
                continue
            diag = GuidanceDiagnostics() if diagnostics else None
            extra = {'mc_pairing': 'cross'} if mc_pairing == 'cross' and method == 'mc_feng' else {}
            if ess_floor is not None and method == 'mc_feng':
                extra['ess_floor'] = float(ess_floor)
            blocks = shared_mc_sweep(fm_x, fm_y, ratio, method, strengths, num_samples, num_steps, device, mc_batch_size,
                                     (1, 28, 28), (1, 28, 28), solver=solver, diagnostics=diag,
                                     guidance_schedule=guidance_schedule, **extra, **sde)
            for j, (strength, (xs, ys)) in enumerate(zip(strengths, blocks)):
                metrics = evaluate_coherence(xs, ys, classifier, device, transform_type)
                if diag is not None and diag.records is not None:
                    part = GuidanceDiagnostics.from_records(diag.records[:, j * num_samples:(j + 1) * num_samples], method,
                                                            solver, num_steps)
                    metrics = {**metrics, **row_metrics(part, num_steps)}
                results.append({'method': method, 'guidance_strength': strength, 'transform_type': transform_type,
                                **metrics, **extra, **sde_row, 'shared_mc': True})
                print(f"  method={method} gamma={strength} -> coherence accuracy {metrics['coherence_acc']:.3f}")
            continue
        for strength in strengths:
            if method == 'none' and strength > 0:
                continue
            ratio = make_ratio() if method != 'none' else None
            if method != 'none' and ratio is None:
                continue
            diag = GuidanceDiagnostics() if diagnostics and method != 'none' else None
            extra = {'mc_pairing': 'cross'} if mc_pairing == 'cross' and method == 'mc_feng' else {}
            if ess_floor is not None and method == 'mc_feng':
                extra['ess_floor'] = float(ess_floor)
            xs, ys = sampler(fm_x, fm_y, ratio, method, strength, num_samples, num_steps, device, mc_batch_size, **kw,
                             **({'diagnostics': diag} if diag is not None else {}), **extra, **lab_kw)
            metrics = evaluate_coherence(xs, ys, classifier, device, transform_type)
            if lab_kw:
                K = getattr(fm_x, 'num_classes', None)
                metrics = {**metrics, 'labelled': True, 'cfg_scale': float(cfg_scale),
                           'label_accuracy_x': label_accuracy(xs, classifier, labels, device, K),
                           'label_accuracy_y': label_accuracy(get_inverse_transform(transform_type)(ys), classifier, labels,
                                                              device, K)}
            if diag is not None and diag.records is not None:
                metrics = {**metrics, **row_metrics(diag, num_steps)}
            if shared_mc:
                metrics = {**metrics, 'shared_mc': True}
            results.append({'method': method, 'guidance_strength': strength, 'transform_type': transform_type,
                            **metrics, **extra, **sde_row})
            print(f"  method={method} gamma={strength} -> coherence accuracy {metrics['coherence_acc']:.3f}")
    return results


def main(argv=None):
    p = argparse.ArgumentParser(description='Evaluate guided sampling (MI355X)')
    p.add_argument('--guidance_methods', nargs='+', default=['none', 'mc_feng'])
    p.add_argument('--guidance_strengths', nargs='+', type=float, default=[0.0, 0.5, 1.0])
    p.add_argument('--num_samples', type=int, default=500)
    add_common_args(p, mc_default=256)
    add_diagnostics_args(p, sampling=False)
    add_pairing_arg(p)
    add_schedule_args(p)
    add_sde_args(p)
    add_ess_arg(p)
    add_label_args(p)
    p.add_argument('--shared_mc', action='store_true',
                   help='run all strengths of a guided method as one sampler call over one MC set, one pre-phase and one '
                        'start-noise set (a strength per row): the strengths then differ by the strength alone; --model unet')
    args = p.parse_args(argv)
    schedule = schedule_from_cli(args)
    sde_kw = {**sde_from_cli(args), **ess_from_cli(args)}
    if (schedule is not None or args.shared_mc) and args.model != 'unet':
        p.error('--guidance_schedule / --guidance_window / --shared_mc go with --model unet')

    set_seed(args.seed)
    lab_kw = labels_from_cli(args, args.num_samples, guided=bool(args.labels) and any(m != 'none' for m in args.guidance_methods),
                             unet=args.model == 'unet')
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; the sampler has no CPU path")
    device = torch.device(args.device)

    clf_path = 'checkpoints/mnist_classifier.pth'
    path_x = get_checkpoint_path('flow', 'x', None, 'best')
    path_y = get_checkpoint_path('flow', 'y', args.transform_type, 'best')
    for path in (clf_path, path_x, path_y):
        if not os.path.exists(path):
            print(f"ERROR: checkpoint not found: {path} (train it with the reference scripts)")
            return 1
    classifier = MNISTClassifier().to(device)
    classifier.load_state_dict(torch.load(clf_path, map_location=device))
    fm_x, fm_y = build_flow_models(args.model, device, args.num_classes)
    load_checkpoint(fm_x, path_x, device, ema=args.ema)
    load_checkpoint(fm_y, path_y, device, ema=args.ema)

    def make_ratio():
        path = get_checkpoint_path('ratio', args.loss_type, args.transform_type, 'best')
        if not os.path.exists(path):
            print(f"ERROR: Ratio estimator not found: {path}")
            return None
        r = RatioEstimator(loss_type=args.loss_type).to(device)
        load_checkpoint(r, path, device)
        return r

    results = run_sweep(fm_x, fm_y, make_ratio, classifier, args.guidance_methods, args.guidance_strengths,
                        args.num_samples, args.num_steps, device, args.mc_batch_size, args.transform_type, solver=args.solver,
                        diagnostics=args.diagnostics, mc_pairing=args.mc_pairing, shared_mc=args.shared_mc,
                        guidance_schedule=schedule, **sde_kw, **lab_kw)
    os.makedirs('outputs', exist_ok=True)
    out = 'outputs/evaluation_results.json'
    with open(out, 'w') as f:
        json.dump(results, f, indent=2)
    print(f"Results saved to: {out}")
    for r in results:
        print(f"  {r['method']:20s} gamma={r['guidance_strength']:.1f} -> coherence={r['coherence_acc']:.3f}")
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
