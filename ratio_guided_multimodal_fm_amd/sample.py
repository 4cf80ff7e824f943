"""28x28 paired sampler CLI (reference ``src/sample.py``).

Flags and defaults of the reference ``main`` (``:117-137``), its checkpoint naming
(``get_checkpoint_path('flow','x',None,'best')`` etc., ``:156-157,:182``) and both ``--model``
choices: ``unet`` (``FlowMatchingUNet``) and ``original`` (``FlowMatchingModel``).  Sampling is
``utils.flow_utils.sample_bimodal_guided`` on the HIP path.  The matplotlib grid of
``visualize_pairs`` (``:33-114``) is out of scope: samples are saved as a ``.pt`` file.
"""
import argparse
import os

import torch

from .models.flow_matching import FlowMatchingModel
from .models.ratio_estimator import RatioEstimator
from .models.unet import FlowMatchingUNet
from .utils import load_checkpoint, set_seed
from .utils.diagnostics import GuidanceDiagnostics, add_cli_args as add_diagnostics_args, report_diagnostics
from .utils.flow_utils import (add_ess_arg, add_label_args, add_pairing_arg, add_sde_args, ess_from_cli, labels_from_cli,
                               sample_bimodal_guided, sde_from_cli)
from .utils.guidance_schedule import add_cli_args as add_schedule_args, from_cli as schedule_from_cli
from .utils.path_utils import get_checkpoint_path


def build_flow_models(model, device, num_classes=None):
    """The reference's ``--model`` switch (:149-154); `num_classes`: class-conditional U-Nets (--num_classes)."""
    if model == 'unet':
        return FlowMatchingUNet(num_classes=num_classes).to(device), FlowMatchingUNet(num_classes=num_classes).to(device)
    if num_classes is not None:
        raise ValueError("--num_classes goes with --model unet")
    if model == 'original':
        return FlowMatchingModel().to(device), FlowMatchingModel().to(device)
    raise ValueError(f"unknown --model {model!r} (choices: unet, original)")


def add_common_args(p, mc_default):
    p.add_argument('--transform_type', type=str, default='rotate90')
    p.add_argument('--mc_batch_size', type=int, default=mc_default)
    p.add_argument('--loss_type', type=str, default='disc')
    p.add_argument('--num_steps', type=int, default=100)
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--model', type=str, default='unet', choices=['unet', 'original'])
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--ema', action='store_true', help="load the averaged weights ('ema_state_dict') of the flow checkpoints (train_flow --optimizer hip --ema_decay ...)")
    p.add_argument('--solver', type=str, default='euler', choices=['euler', 'midpoint'],
                   help="ODE solver of every sampler loop: 'midpoint' (explicit midpoint rule, second order) takes two network evaluations per step (U-Net nets: not with --model original)")


def main(argv=None):
    p = argparse.ArgumentParser(description='Sample bimodal pairs (MI355X)')
    p.add_argument('--guidance_method', type=str, default='none', choices=['none', 'mc_feng'])
    p.add_argument('--guidance_strength', type=float, default=0.5)
    p.add_argument('--num_samples', type=int, default=64)
    add_common_args(p, mc_default=128)
    add_diagnostics_args(p)
    add_pairing_arg(p)
    add_schedule_args(p)
    add_sde_args(p)
    add_ess_arg(p)
    add_label_args(p)
    args = p.parse_args(argv)
    schedule = schedule_from_cli(args)
    sde_kw = {**sde_from_cli(args), **ess_from_cli(args)}
    if schedule is not None and args.model != 'unet':
        p.error('--guidance_schedule / --guidance_window go with --model unet')
    if args.mc_pairing == 'cross' and (args.guidance_method != 'mc_feng' or args.model != 'unet'):
        p.error('--mc_pairing cross goes with --guidance_method mc_feng and --model unet')
    diag = GuidanceDiagnostics() if args.diagnostics or args.diagnostics_out else None

    set_seed(args.seed)
    lab_kw = labels_from_cli(args, args.num_samples, guided=args.guidance_method != 'none', unet=args.model == 'unet')
    print(f"Random seed: {args.seed}")
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; this sampler has no CPU path")
    device = torch.device(args.device)
    print(f"Using device: {device}")

    fm_x, fm_y = build_flow_models(args.model, device, args.num_classes)
    path_x = get_checkpoint_path('flow', 'x', None, 'best')
    path_y = get_checkpoint_path('flow', 'y', args.transform_type, 'best')
    preset = 'original' if args.model == 'original' else 'unet28'
    for path, flags in ((path_x, '--modality x'), (path_y, f'--modality y --transform_type {args.transform_type}')):
        if not os.path.exists(path):
            print(f"ERROR: FM checkpoint not found: {path} (train it: python -m ratio_guided_multimodal_fm_amd.train_flow "
                  f"--preset {preset} {flags} --data <images.npy>)")
            return 1
    load_checkpoint(fm_x, path_x, device, ema=args.ema)
    load_checkpoint(fm_y, path_y, device, ema=args.ema)
    print(f"  Loaded FM_x from: {path_x}\n  Loaded FM_y from: {path_y}")

    ratio = None
    if args.guidance_method != 'none':
        ratio = RatioEstimator(loss_type=args.loss_type).to(device)
        path_ratio = get_checkpoint_path('ratio', args.loss_type, args.transform_type, 'best')
        if not os.path.exists(path_ratio):
            print(f"ERROR: Ratio estimator checkpoint not found: {path_ratio}")
            return 1
        load_checkpoint(ratio, path_ratio, device)
        print(f"  Loaded ratio estimator from: {path_ratio}")

    print(f"\nSampling {args.num_samples} pairs...")
    xs, ys = sample_bimodal_guided(fm_x, fm_y, ratio, args.guidance_method, args.guidance_strength,
                                   args.num_samples, args.num_steps, device, args.mc_batch_size, solver=args.solver,
                                   diagnostics=diag, mc_pairing=args.mc_pairing,
                                   **({'guidance_schedule': schedule} if schedule is not None else {}), **sde_kw, **lab_kw)
    report_diagnostics(diag, args.num_steps, args.diagnostics, args.diagnostics_out)
    os.makedirs('outputs', exist_ok=True)
    out = f"outputs/samples_{args.guidance_method}_gamma{args.guidance_strength}_{args.transform_type}.pt"
    torch.save({'x': xs.cpu(), 'y': ys.cpu()}, out)
    print(f"Saved samples: {out}")
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
