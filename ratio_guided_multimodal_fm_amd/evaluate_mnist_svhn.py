"""Coherence evaluation of generated MNIST-SVHN pairs (reference ``src/evaluate_mnist_svhn.py``).

``evaluate_coherence`` (``:28-57``) and the method x strength sweep of ``main`` (``:60-199``) with the
reference's flags, skip rule (``none`` with gamma > 0), single ``set_seed`` before the sweep (so each
configuration's noise depends on sweep order, as in the reference) and JSON schema
(``method, guidance_strength, experiment, coherence_acc, num_samples``).  Sampling runs on the HIP
path; the two classifiers run once per configuration in PyTorch-ROCm.

Multi-GPU (new; the reference is single-device): launched under ``torch.distributed.run`` with ``--sharded``,
e.g. BASELINE configs[4]

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m ratio_guided_multimodal_fm_amd.evaluate_mnist_svhn --sharded --num_samples 8192 --num_steps 200 \
        --guidance_strengths 0 0.5 1 2 5

every rank loads the checkpoints, integrates its rows of each configuration (distributed.py: sharded MC
pre-phase, one RCCL all_gather of the MC set, one all_gather of the outputs) and rank 0 classifies and writes
the JSON.
"""
import argparse
import json
import os

import torch

from .models.ratio_flexible import RatioEstimatorMNISTSVHN
from .models.svhn_classifier import MNISTClassifier32, SVHNClassifier
from .models.unet_flexible import FlowMatchingUNetMNIST, FlowMatchingUNetSVHN
from .sample_mnist_svhn import sample_bimodal_guided_mnist_svhn
from .utils import load_checkpoint, set_seed
from .utils.diagnostics import GuidanceDiagnostics, add_cli_args as add_diagnostics_args, row_metrics
from .utils.flow_utils import (add_ess_arg, add_label_args, add_sde_args, ess_from_cli, labels_from_cli, sde_from_cli, add_pairing_arg,
                               shared_mc_sweep)
from .utils.guidance_schedule import add_cli_args as add_schedule_args, from_cli as schedule_from_cli


def evaluate_coherence(samples_mnist, samples_svhn, mnist_classifier, svhn_classifier, device):
    """P(argmax clf_mnist(x) == argmax clf_svhn(y)) over the pairs; returns the reference's dict."""
    mnist_classifier.eval()
    svhn_classifier.eval()
    with torch.no_grad():
        pred_m = mnist_classifier(samples_mnist.to(device)).argmax(dim=1)
        pred_s = svhn_classifier(samples_svhn.to(device)).argmax(dim=1)
    acc = (pred_m == pred_s).float().mean().item() if len(samples_mnist) else float('nan')
    return {'coherence_acc': float(acc), 'num_samples': len(samples_mnist)}


def label_accuracy(samples, classifier, labels, device, num_classes=None):
    """Share of the rows whose class the classifier predicts as the requested label; rows with the null label
    (`num_classes`) are left out.  nan without rows."""
    classifier.eval()
    labels = torch.as_tensor(labels).to(device).reshape(-1)
    with torch.no_grad():
        pred = classifier(samples.to(device)).argmax(dim=1)
    keep = labels != num_classes if num_classes is not None else torch.ones_like(labels, dtype=torch.bool)
    return float((pred[keep] == labels[keep]).float().mean().item()) if int(keep.sum()) else float('nan')


def evaluate_conditional_coherence(condition, samples, given, mnist_classifier, svhn_classifier, device,
                                   fm_target=None, ratio_estimator=None, guidance_method='mc_feng', **sampler_kwargs):
    """Share of rows where the classifier of the condition's modality and the classifier of the generated modality
    agree: `condition` [B, ...] are the images `samples` [B, ...] were generated for (``sample_conditional``), `given`
    ('mnist' or 'svhn') names the condition's modality.  With ``samples=None`` they are generated here:
    ``sample_conditional(fm_target, ratio_estimator, condition, given, guidance_method=guidance_method,
    **sampler_kwargs)`` ('mc_feng' or 'grad_log_ratio'; num_steps, guidance_strength, mc_batch_size, solver as keywords)."""
    from ._lib import solver_id
    solver_id(sampler_kwargs.get('solver', 'euler'))
    if given not in ('mnist', 'svhn'):
        raise ValueError(f"given must be 'mnist' or 'svhn', got {given!r}")
    if samples is None:
        if fm_target is None or ratio_estimator is None:
            raise ValueError("samples=None needs fm_target and ratio_estimator to generate them")
        from .utils.flow_utils import sample_conditional
        samples = sample_conditional(fm_target, ratio_estimator, condition, 'x' if given == 'mnist' else 'y',
                                     guidance_method=guidance_method, device=device, **sampler_kwargs)
    if len(condition) != len(samples):
        raise ValueError(f"{len(condition)} condition images for {len(samples)} samples")
    mnist, svhn = (condition, samples) if given == 'mnist' else (samples, condition)
    return evaluate_coherence(mnist, svhn, mnist_classifier, svhn_classifier, device)['coherence_acc']


def run_sweep(fm_mnist, fm_svhn, make_ratio, mnist_classifier, svhn_classifier, methods, strengths,
              num_samples, num_steps, device, mc_batch_size, sampler=sample_bimodal_guided_mnist_svhn, solver='euler', diagnostics=False,
              mc_pairing='paired', shared_mc=False, guidance_schedule=None, sde_eta=0.0, sde_seed=None, ess_floor=None,
              labels=None, cfg_scale=1.0):
    """The reference's nested loop (:130-183). `make_ratio()` returns a fresh ratio estimator or None.
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
    ``label_accuracy_x`` / ``label_accuracy_y`` -- each classifier's prediction against the requested label (null-label
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
        if sampler is not sample_bimodal_guided_mnist_svhn:
            raise RgfmError("ess_floor has no sharded form: run the tempered sampler on one device")
    if shared_mc and sampler is not sample_bimodal_guided_mnist_svhn:
        raise ValueError("shared_mc runs the default sampler: it has no sharded form")
    if labels is not None:
        from ._lib import RgfmError
        if any(m != 'none' for m in methods):
            raise RgfmError(f"labels go with the 'none' method alone (the supervised baseline); {list(methods)} holds a guided "
                            "method: sweep it without labels, in a run of its own")
        if sampler is not sample_bimodal_guided_mnist_svhn:
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
            blocks = shared_mc_sweep(fm_mnist, fm_svhn, ratio, method, strengths, num_samples, num_steps, device,
                                     mc_batch_size, (1, 32, 32), (3, 32, 32), solver=solver, diagnostics=diag,
                                     guidance_schedule=guidance_schedule, **extra, **sde)
            for j, (strength, (xs, ys)) in enumerate(zip(strengths, blocks)):
                metrics = evaluate_coherence(xs, ys, mnist_classifier, svhn_classifier, device)
                if diag is not None and diag.records is not None:
                    part = GuidanceDiagnostics.from_records(diag.records[:, j * num_samples:(j + 1) * num_samples], method,
                                                            solver, num_steps)
                    metrics = {**metrics, **row_metrics(part, num_steps)}
                results.append({'method': method, 'guidance_strength': strength, 'experiment': 'mnist_svhn',
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
            xs, ys = sampler(fm_mnist, fm_svhn, ratio, method, strength, num_samples, num_steps, device,
                             mc_batch_size, **kw, **({'diagnostics': diag} if diag is not None else {}), **extra, **lab_kw)
            metrics = evaluate_coherence(xs, ys, mnist_classifier, svhn_classifier, device)
            if lab_kw:
                K = getattr(fm_mnist, 'num_classes', None)
                metrics = {**metrics, 'labelled': True, 'cfg_scale': float(cfg_scale),
                           'label_accuracy_x': label_accuracy(xs, mnist_classifier, labels, device, K),
                           'label_accuracy_y': label_accuracy(ys, svhn_classifier, labels, device, K)}
            if diag is not None and diag.records is not None:
                metrics = {**metrics, **row_metrics(diag, num_steps)}
            if shared_mc:
                metrics = {**metrics, 'shared_mc': True}
            results.append({'method': method, 'guidance_strength': strength, 'experiment': 'mnist_svhn',
                            **metrics, **extra, **sde_row})
            print(f"  method={method} gamma={strength} -> coherence accuracy {metrics['coherence_acc']:.3f}")
    return results


def main(argv=None):
    from . import distributed  # noqa: F401  (first: it puts HSA_ENABLE_IPC_MODE_LEGACY=0 in place before any HIP call of this process)
    p = argparse.ArgumentParser(description='Evaluate MNIST-SVHN guided sampling (MI355X)')
    p.add_argument('--guidance_methods', nargs='+', default=['none', 'mc_feng'])
    p.add_argument('--guidance_strengths', nargs='+', type=float, default=[0.0, 0.5, 1.0])
    p.add_argument('--mc_batch_size', type=int, default=256)
    p.add_argument('--loss_type', type=str, default='disc')
    p.add_argument('--num_samples', type=int, default=500)
    p.add_argument('--num_steps', type=int, default=100)
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--ema', action='store_true', help="load the averaged weights ('ema_state_dict') of the flow checkpoints (train_flow --optimizer hip --ema_decay ...)")
    p.add_argument('--solver', type=str, default='euler', choices=['euler', 'midpoint'],
                   help="ODE solver of every sampler loop: 'midpoint' (explicit midpoint rule, second order) takes two network evaluations per step")
    p.add_argument('--sharded', action='store_true',
                   help='rows sharded over the ranks of a torch.distributed.run launch (one process per GPU, RCCL)')
    add_diagnostics_args(p, sampling=False)
    add_pairing_arg(p)
    add_schedule_args(p)
    add_sde_args(p)
    add_ess_arg(p)
    add_label_args(p)
    p.add_argument('--shared_mc', action='store_true',
                   help='run all strengths of a guided method as one sampler call over one MC set, one pre-phase and one '
                        'start-noise set (a strength per row): the strengths then differ by the strength alone; not with '
                        '--sharded')
    args = p.parse_args(argv)
    schedule = schedule_from_cli(args)
    sde_kw = {**sde_from_cli(args, args.sharded), **ess_from_cli(args, args.sharded)}
    if args.shared_mc and args.sharded:
        p.error('--shared_mc has no --sharded form')
    if schedule is not None and args.sharded:
        p.error('--guidance_schedule / --guidance_window have no --sharded form')
    if args.diagnostics and args.sharded:
        p.error('--diagnostics has no --sharded form')
    if args.mc_pairing == 'cross' and args.sharded:
        p.error('--mc_pairing cross has no --sharded form')

    set_seed(args.seed)  # (every rank alike: the sharded sampler slices ONE noise set)
    lab_kw = labels_from_cli(args, args.num_samples, sharded=args.sharded,
                             guided=bool(args.labels) and any(m != 'none' for m in args.guidance_methods))
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; the sampler has no CPU path")
    rank, sampler = 0, sample_bimodal_guided_mnist_svhn
    if args.sharded:
        from .distributed import init_from_env, make_sharded_sampler
        rank, world, device = init_from_env("nccl")
        sampler = make_sharded_sampler((1, 32, 32), (3, 32, 32), gather="all")
        print(f"rank {rank} of {world} on {device}")
    else:
        device = torch.device(args.device)

    paths = {'mnist_clf': 'checkpoints/mnist32_classifier.pth', 'svhn_clf': 'checkpoints/svhn_classifier.pth',
             'fm_mnist': 'checkpoints/flow_mnist32_best.pth', 'fm_svhn': 'checkpoints/flow_svhn_best.pth'}
    for k, v in paths.items():
        if not os.path.exists(v):
            print(f"ERROR: checkpoint not found: {v} (train it with the reference scripts)")
            return 1
    mnist_clf = MNISTClassifier32().to(device)
    svhn_clf = SVHNClassifier().to(device)
    mnist_clf.load_state_dict(torch.load(paths['mnist_clf'], map_location=device))
    svhn_clf.load_state_dict(torch.load(paths['svhn_clf'], map_location=device))
    fm_mnist = FlowMatchingUNetMNIST(img_size=32, num_classes=args.num_classes).to(device)
    fm_svhn = FlowMatchingUNetSVHN(num_classes=args.num_classes).to(device)
    load_checkpoint(fm_mnist, paths['fm_mnist'], device, ema=args.ema)
    load_checkpoint(fm_svhn, paths['fm_svhn'], device, ema=args.ema)

    def make_ratio():
        path = f'checkpoints/ratio_{args.loss_type}_mnist_svhn_best.pth'
        if not os.path.exists(path):
            print(f"ERROR: Ratio estimator not found: {path}")
            return None
        r = RatioEstimatorMNISTSVHN(loss_type=args.loss_type).to(device)
        r.load_state_dict(torch.load(path, map_location=device))
        return r

    results = run_sweep(fm_mnist, fm_svhn, make_ratio, mnist_clf, svhn_clf, args.guidance_methods,
                        args.guidance_strengths, args.num_samples, args.num_steps, device, args.mc_batch_size,
                        sampler=sampler, solver=args.solver, diagnostics=args.diagnostics, mc_pairing=args.mc_pairing,
                        shared_mc=args.shared_mc, guidance_schedule=schedule, **sde_kw, **lab_kw)
    if args.sharded:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
        if rank != 0:
            return 0
    os.makedirs('outputs/mnist_svhn', exist_ok=True)
    out = 'outputs/mnist_svhn/evaluation_results.json'
    with open(out, 'w') as f:
        json.dump(results, f, indent=2)
    print(f"Results saved to: {out}")
    for r in results:
        print(f"  {r['method']:20s} gamma={r['guidance_strength']:.1f} -> coherence={r['coherence_acc']:.3f}")
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
