"""Log-likelihood and bits per dimension of images under a trained velocity U-Net.

    python -m ratio_guided_multimodal_fm_amd.log_prob --preset svhn --checkpoint checkpoints/flow_svhn_best.pth --data svhn_test.npy
    python -m ratio_guided_multimodal_fm_amd.log_prob --preset mnist32 --checkpoint checkpoints/flow_mnist32_best.pth --data mnist_test.npy \\
        --preset_y svhn --checkpoint_y checkpoints/flow_svhn_best.pth --data_y svhn_test.npy --ratio_checkpoint checkpoints/ratio_mnist_svhn_best.pth

The images (one tensor [N, C, H, W] in a .npy or .pt file, in the value range the net was trained on) are integrated
backwards along the flow with the divergence of v accumulated on the way (CFMSchedule.log_prob; Hutchinson's estimate
with --n_probes Rademacher probes per image, drawn from a generator seeded with --seed).  Prints, and writes as JSON
next to the checkpoint (<checkpoint stem>_logprob.json), the mean and the standard error of log p and of bits/dim,
the number of images and the settings.  With the four joint arguments the pairs (x_i, y_i) are scored under
p(x) p(y) r(x, y) as well (utils.flow_utils.joint_log_prob; the ratio estimator is unnormalised, so is that term).
The reference has no likelihood evaluation; U-Net presets only.
"""
import argparse
import json
import os

import torch

from .models import (FlowMatchingUNet, FlowMatchingUNetMNIST, FlowMatchingUNetSVHN, RatioEstimator,
                     RatioEstimatorMNISTSVHN)
from .train_flow import load_data
from .utils import load_checkpoint
from .utils.flow_utils import CFMSchedule, bits_per_dim, joint_log_prob

PRESETS = {
    'mnist32': (lambda: FlowMatchingUNetMNIST(32), (1, 32, 32)),
    'svhn': (FlowMatchingUNetSVHN, (3, 32, 32)),
    'unet28': (FlowMatchingUNet, (1, 28, 28)),
}
# the ratio estimator of a pair of presets (x, y)
RATIO_OF = {('mnist32', 'svhn'): RatioEstimatorMNISTSVHN, ('unet28', 'unet28'): RatioEstimator}
JOINT_ARGS = ('ratio_checkpoint', 'data_y', 'preset_y', 'checkpoint_y')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--preset', choices=sorted(PRESETS), required=True)
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--data', required=True, help='.npy / .pt tensor [N, C, H, W]')
    p.add_argument('--num_steps', type=int, default=100)
    p.add_argument('--solver', choices=['euler', 'midpoint'], default='midpoint')
    p.add_argument('--ema', action='store_true', help="load the averaged weights ('ema_state_dict') of the flow checkpoints (train_flow --optimizer hip --ema_decay ...)")
    p.add_argument('--n_probes', type=int, default=1, help='Hutchinson probes per image')
    p.add_argument('--seed', type=int, default=42, help='seed of the probe generator')
    p.add_argument('--batch_size', type=int, default=128)
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--data_range', type=float, default=2.0, help='length of the interval the pixel values were scaled to')
    p.add_argument('--levels', type=int, default=256, help='quantisation levels of the source images')
    p.add_argument('--ratio_checkpoint', default=None, help='joint term: the ratio estimator of the pair')
    p.add_argument('--data_y', default=None, help='joint term: the partner images, paired by index')
    p.add_argument('--preset_y', choices=sorted(PRESETS), default=None)
    p.add_argument('--checkpoint_y', default=None)
    p.add_argument('--loss_type', choices=['disc', 'rulsif'], default='disc', help='of the ratio estimator')
    args = p.parse_args(argv)
    given = [a for a in JOINT_ARGS if getattr(args, a) is not None]
    if given and len(given) != len(JOINT_ARGS):
        p.error('the joint term needs all of ' + ', '.join('--' + a for a in JOINT_ARGS))
    args.joint = bool(given)
    if args.joint and (args.preset, args.preset_y) not in RATIO_OF:
        p.error('ratio estimators exist for the preset pairs ' + ', '.join(f'{a}+{b}' for a, b in RATIO_OF))
    return args


def load_net(preset, path, device, ema=False):
    model = PRESETS[preset][0]().to(device)
    load_checkpoint(model, path, device, ema=ema)
    return model.eval()


def mean_sem(v):
    """(mean, standard error of the mean) of a 1-D tensor, in double."""
    v = v.detach().double().cpu()
    n = v.numel()
    return float(v.mean()), (float(v.std(unbiased=True)) / n ** 0.5 if n > 1 else 0.0)


def summarise(logp, dims, data_range, levels):
    bpd = bits_per_dim(logp.double(), dims, data_range, levels)
    (lm, ls), (bm, bs) = mean_sem(logp), mean_sem(bpd)
    return {'logp_mean': lm, 'logp_sem': ls, 'bits_per_dim_mean': bm, 'bits_per_dim_sem': bs}


def main(argv=None):
    args = parse_args(argv)
    device = torch.device(args.device)
    shape = PRESETS[args.preset][1]
    x = load_data(args.data, shape).to(device)
    model = load_net(args.preset, args.checkpoint, device, args.ema)
    gen = torch.Generator(device=device).manual_seed(args.seed)
    kw = dict(num_steps=args.num_steps, solver=args.solver, n_probes=args.n_probes, generator=gen,
              batch_size=args.batch_size)
    settings = {k: getattr(args, k) for k in ('preset', 'checkpoint', 'data', 'num_steps', 'solver', 'n_probes', 'seed',
                                              'batch_size', 'data_range', 'levels')}
    if args.ema:
        settings['ema'] = True
    dims = shape[0] * shape[1] * shape[2]
    result = {'num_images': int(x.shape[0]), 'dims': dims, 'settings': settings}
    if args.joint:
        shape_y = PRESETS[args.preset_y][1]
        y = load_data(args.data_y, shape_y).to(device)
        model_y = load_net(args.preset_y, args.checkpoint_y, device, args.ema)
        ratio = RATIO_OF[(args.preset, args.preset_y)](loss_type=args.loss_type).to(device)
        load_checkpoint(ratio, args.ratio_checkpoint, device)
        joint, logp, logp_y, log_r = joint_log_prob(model, model_y, ratio.eval(), x, y, **kw)
        dims_y = shape_y[0] * shape_y[1] * shape_y[2]
        result.update(summarise(logp, dims, args.data_range, args.levels))
        result['y'] = dict(summarise(logp_y, dims_y, args.data_range, args.levels), dims=dims_y)
        result['log_ratio_mean'], result['log_ratio_sem'] = mean_sem(log_r)
        result['joint_logp_mean'], result['joint_logp_sem'] = mean_sem(joint)
        settings.update({a: getattr(args, a) for a in JOINT_ARGS + ('loss_type',)})
    else:
        logp, _ = CFMSchedule().log_prob(model, x, **kw)
        result.update(summarise(logp, dims, args.data_range, args.levels))
    out = os.path.splitext(args.checkpoint)[0] + '_logprob.json'
    with open(out, 'w') as f:
        json.dump(result, f, indent=2)
    print(f"{result['num_images']} images, {args.solver} x {args.num_steps} steps, {args.n_probes} probe(s):")
    print(f"  log p     = {result['logp_mean']:.4f} +- {result['logp_sem']:.4f} nats")
    print(f"  bits/dim  = {result['bits_per_dim_mean']:.5f} +- {result['bits_per_dim_sem']:.5f}")
    if args.joint:
        print(f"  log p(y)  = {result['y']['logp_mean']:.4f} +- {result['y']['logp_sem']:.4f} nats")
        print(f"  log r     = {result['log_ratio_mean']:.4f} +- {result['log_ratio_sem']:.4f}")
        print(f"  joint     = {result['joint_logp_mean']:.4f} +- {result['joint_logp_sem']:.4f} nats")
    print(f"Wrote {out}")
    return result


if __name__ == '__main__':
    main()
