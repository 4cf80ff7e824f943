"""MNIST32 + SVHN paired sampler (reference ``src/sample_mnist_svhn.py``).

``sample_bimodal_guided_mnist_svhn`` keeps the reference signature
(``:39-49``) and semantics (``:68-177``); the CLI mirrors ``main`` (``:247-337``)
minus the matplotlib grid, which is out of scope: samples are saved as a
``.pt`` file instead.
"""
import argparse
import os

import torch

from .models.ratio_flexible import RatioEstimatorMNISTSVHN
from .models.unet_flexible import FlowMatchingUNetMNIST, FlowMatchingUNetSVHN
from .utils import load_checkpoint, set_seed
from .utils.diagnostics import GuidanceDiagnostics, add_cli_args as add_diagnostics_args, report_diagnostics
from .utils.flow_utils import (add_ess_arg, add_label_args, add_pairing_arg, add_sde_args, ess_from_cli, labels_from_cli, paired_sampler,
                               sample_conditional, sde_from_cli)
from .utils.guidance_schedule import add_cli_args as add_schedule_args, from_cli as schedule_from_cli


def sample_bimodal_guided_mnist_svhn(fm_mnist, fm_svhn, ratio_estimator=None, guidance_method='none',
                                     guidance_strength=0.0, num_samples=16, num_steps=100,
                                     device='cuda', mc_batch_size=64, solver='euler', diagnostics=None,
                                     mc_pairing='paired', guidance_schedule=None, sde_eta=0.0, sde_seed=None,
                                     ess_floor=None, labels=None, cfg_scale=1.0):
    """Returns ``(samples_mnist [n,1,32,32], samples_svhn [n,3,32,32])`` on `device`.  `diagnostics`: a
    ``utils.diagnostics.GuidanceDiagnostics`` to fill; `mc_pairing`: 'paired' | 'cross'; `guidance_strength`: a float or
    one strength per sample; `guidance_schedule`: a scale of it per stage; `sde_eta`, `sde_seed`: the stochastic sampler;
    `ess_floor`: the effective-sample-size floor of the importance weights; `labels`, `cfg_scale`
    (``guidance_method='none'``): the class-conditional pair (all: ``paired_sampler``)."""
    return paired_sampler(fm_mnist, fm_svhn, ratio_estimator, guidance_method, guidance_strength,
                          num_samples, num_steps, device, mc_batch_size, (1, 32, 32), (3, 32, 32), solver=solver,
                          diagnostics=diagnostics, mc_pairing=mc_pairing, guidance_schedule=guidance_schedule,
                          sde_eta=sde_eta, sde_seed=sde_seed, ess_floor=ess_floor, labels=labels, cfg_scale=cfg_scale)


def load_condition(path, shape):
    """Condition images [B, *shape] from a ``.npy`` array or a ``.pt`` tensor."""
    import numpy as np
    t = torch.from_numpy(np.load(path)) if path.endswith('.npy') else torch.load(path, map_location='cpu')
    t = torch.as_tensor(t, dtype=torch.float32)
    if t.dim() != 4 or tuple(t.shape[1:]) != shape:
        raise ValueError(f"--condition: expected images of shape [B,{shape[0]},{shape[1]},{shape[2]}], got {tuple(t.shape)}")
    return t


def main(argv=None):
    from . import distributed  # noqa: F401  (first: it puts HSA_ENABLE_IPC_MODE_LEGACY=0 in place before any HIP call of this process)
    p = argparse.ArgumentParser(description='Sample MNIST-SVHN pairs (MI355X)')
    p.add_argument('--guidance_method', type=str, default='none', choices=['none', 'mc_feng', 'grad_log_ratio'],
                   help="'grad_log_ratio' (v + gamma * grad log r, reference README.md:159-164) is this build's extension: "
                        "the reference CLI accepts 'none' and 'mc_feng' only")
    p.add_argument('--guidance_strength', type=float, default=0.5)
    p.add_argument('--mc_batch_size', type=int, default=256)
    p.add_argument('--loss_type', type=str, default='disc')
    p.add_argument('--num_samples', type=int, default=32)
    p.add_argument('--num_steps', type=int, default=100)
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--ema', action='store_true', help="load the averaged weights ('ema_state_dict') of the flow checkpoints (train_flow --optimizer hip --ema_decay ...)")
    p.add_argument('--solver', type=str, default='euler', choices=['euler', 'midpoint'],
                   help="ODE solver of every sampler loop: 'midpoint' (explicit midpoint rule, second order) takes two network evaluations per step")
    p.add_argument('--sharded', action='store_true',
                   help='rows sharded over the ranks of a torch.distributed.run launch (one process per GPU, RCCL); '
                        'e.g. BASELINE configs[3]: --nproc-per-node 8 ... --sharded --num_samples 4096 '
                        '--guidance_method mc_feng --guidance_strength 1.0')
    p.add_argument('--given', type=str, default=None, choices=['mnist', 'svhn'],
                   help="conditional sampling (this build's extension): the modality of --condition; the other one is "
                        "generated, one sample per condition image (MC guidance with --guidance_strength and "
                        "--mc_batch_size; with --guidance_method grad_log_ratio the one-sided gradient guidance, no MC set)")
    p.add_argument('--condition', type=str, default=None, metavar='FILE.npy|.pt',
                   help='condition images [B,1,32,32] (--given mnist) or [B,3,32,32] (--given svhn)')
    add_diagnostics_args(p)
    add_pairing_arg(p)
    add_schedule_args(p)
    add_sde_args(p)
    add_ess_arg(p)
    add_label_args(p)
    args = p.parse_args(argv)
    schedule = schedule_from_cli(args)
    sde_kw = {**sde_from_cli(args, args.sharded), **ess_from_cli(args, args.sharded)}
    if schedule is not None and args.sharded:
        p.error('--guidance_schedule / --guidance_window have no --sharded form')
    if args.mc_pairing == 'cross' and (args.guidance_method != 'mc_feng' or args.given or args.sharded):
        p.error('--mc_pairing cross goes with --guidance_method mc_feng; it has no --given and no --sharded form')
    if (args.diagnostics or args.diagnostics_out) and args.sharded:
        p.error('--diagnostics / --diagnostics_out have no --sharded form')
    diag = GuidanceDiagnostics() if args.diagnostics or args.diagnostics_out else None
    if (args.given is None) != (args.condition is None):
        p.error('--given and --condition go together')
    if args.given and args.sharded:
        p.error('conditional sampling has no --sharded form')

    set_seed(args.seed)  # (every rank alike: the sharded sampler slices ONE noise set)
    lab_kw = labels_from_cli(args, args.num_samples, sharded=args.sharded,
                             guided=args.guidance_method != 'none' or bool(args.given))
    print(f"Random seed: {args.seed}")
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible; this sampler has no CPU path")
    rank, sampler = 0, sample_bimodal_guided_mnist_svhn
    if args.sharded:
        from .distributed import init_from_env, make_sharded_sampler
        rank, world, device = init_from_env("nccl")
        sampler = make_sharded_sampler((1, 32, 32), (3, 32, 32), gather="rank0")
        print(f"rank {rank} of {world}")
    else:
        device = torch.device(args.device)
    print(f"Using device: {device}")

    fm_mnist = FlowMatchingUNetMNIST(img_size=32, num_classes=args.num_classes).to(device)
    fm_svhn = FlowMatchingUNetSVHN(num_classes=args.num_classes).to(device)
    for model, path, hint in ((fm_mnist, 'checkpoints/flow_mnist32_best.pth', 'train_flow_mnist32.py'),
                              (fm_svhn, 'checkpoints/flow_svhn_best.pth', 'train_flow_svhn.py')):
        if not os.path.exists(path):
            print(f"ERROR: checkpoint not found: {path}")
            print(f"Please train first with the reference: python src/{hint}")
            return 1
        load_checkpoint(model, path, device, ema=args.ema)
        print(f"  Loaded {path}")

    ratio = None
    if args.guidance_method != 'none' or args.given:
        ratio = RatioEstimatorMNISTSVHN(loss_type=args.loss_type).to(device)
        path = f'checkpoints/ratio_{args.loss_type}_mnist_svhn_best.pth'
        if not os.path.exists(path):
            print(f"ERROR: Ratio estimator not found: {path}")
            return 1
        ratio.load_state_dict(torch.load(path, map_location=device))
        print(f"  Loaded ratio estimator from: {path}")

    if args.given:
        shape = (1, 32, 32) if args.given == 'mnist' else (3, 32, 32)
        condition = load_condition(args.condition, shape)
        target, name = (fm_svhn, 'svhn') if args.given == 'mnist' else (fm_mnist, 'mnist')
        print(f"\nSampling {len(condition)} {name} images given {args.given}...")
        # ('none' and 'mc_feng' both mean the MC guidance here: a conditional sampler without guidance ignores --condition)
        method = 'grad_log_ratio' if args.guidance_method == 'grad_log_ratio' else 'mc_feng'
        out_t = sample_conditional(target, ratio, condition.to(device), 'x' if args.given == 'mnist' else 'y',
                                   args.num_steps, args.guidance_strength, args.mc_batch_size, device=device,
                                   guidance_method=method, solver=args.solver, diagnostics=diag,
                                   **({'guidance_schedule': schedule} if schedule is not None else {}), **sde_kw)
        report_diagnostics(diag, args.num_steps, args.diagnostics, args.diagnostics_out)
        os.makedirs('outputs/mnist_svhn', exist_ok=True)
        tag = '_grad_log_ratio' if method == 'grad_log_ratio' else ''
        out = f"outputs/mnist_svhn/samples_given_{args.given}{tag}_gamma{args.guidance_strength}.pt"
        torch.save({args.given: condition, name: out_t.cpu()}, out)
        print(f"Saved samples: {out}")
        return 0

    print(f"\nSampling {args.num_samples} pairs...")
    xs, ys = sampler(fm_mnist, fm_svhn, ratio, args.guidance_method, args.guidance_strength, args.num_samples,
                     args.num_steps, device, args.mc_batch_size, **({'solver': args.solver} if args.solver != 'euler' else {}),
                     **({'diagnostics': diag} if diag is not None else {}),
                     **({'mc_pairing': args.mc_pairing} if args.mc_pairing != 'paired' else {}),
                     **({'guidance_schedule': schedule} if schedule is not None else {}), **sde_kw, **lab_kw)
    report_diagnostics(diag, args.num_steps, args.diagnostics, args.diagnostics_out)
    if args.sharded:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
        if rank != 0:
            return 0
    os.makedirs('outputs/mnist_svhn', exist_ok=True)
    out = f"outputs/mnist_svhn/samples_{args.guidance_method}_gamma{args.guidance_strength}.pt"
    torch.save({'mnist': xs.cpu(), 'svhn': ys.cpu()}, out)
    print(f"Saved samples: {out}")
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
