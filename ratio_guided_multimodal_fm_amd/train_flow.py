"""Train a velocity net with conditional flow matching on the HIP backward.

    python -m ratio_guided_multimodal_fm_amd.train_flow --preset svhn --data svhn_train.npy
    python -m ratio_guided_multimodal_fm_amd.train_flow --preset original --modality x --data mnist_x.npy

Mirrors the reference trainers (src/train_flow_svhn.py, src/train_flow_mnist32.py, src/train_flow.py): same
arguments and defaults, Adam (--optimizer hip: the fused HIP step of utils/optim.py, with --ema_decay,
--max_grad_norm, --weight_decay), best / every-N checkpoints {'epoch', 'model_state_dict', 'optimizer_state_dict',
'best_loss'} under the reference's names, early stopping.  The data is one tensor [N, C, H, W] in a .npy or .pt
file, already in the reference's value range (no dataset download here).

The 28x28 presets (``original``: FlowMatchingModel, the reference's ``--model original``; ``unet28``) take the
reference's ``--modality {x,y}`` and ``--transform_type``: they only select the checkpoint stem, as the reference's
``get_checkpoint_path('flow', modality, transform, ...)`` does -- ``flow_x_*`` / ``flow_y_<transform>_*``, the names
sample.py and evaluate.py load.  ``original`` requires ``--modality``; without it ``unet28`` writes ``flow_unet28_*``.
"""
import argparse
import os

import numpy as np
import torch

from .models import FlowMatchingModel, FlowMatchingUNet, FlowMatchingUNetMNIST, FlowMatchingUNetSVHN
from .utils import set_seed
from .utils.flow_utils import CFMSchedule, train_flow_matching_epoch
from .utils.optim import add_optimizer_args, build_optimizer, check_optimizer_args

PRESETS = {
    # preset: (constructor, image shape, checkpoint stem) -- the stems sample_mnist_svhn.py / sample.py load
    # (the U-Net constructors take num_classes: --num_classes)
    'mnist32': (lambda **kw: FlowMatchingUNetMNIST(32, **kw), (1, 32, 32), 'flow_mnist32'),
    'svhn': (FlowMatchingUNetSVHN, (3, 32, 32), 'flow_svhn'),
    'unet28': (FlowMatchingUNet, (1, 28, 28), 'flow_unet28'),
    'original': (FlowMatchingModel, (1, 28, 28), None),  # (stem from --modality: checkpoint_stem)
}
MODALITY_PRESETS = ('original', 'unet28')


def checkpoint_stem(preset, modality=None, transform_type='rotate90'):
    """Checkpoint stem of a run: the preset's own, or -- 28x28 presets with --modality -- the reference's
    get_checkpoint_path('flow', modality, transform): 'flow_x' / 'flow_y_<transform>'."""
    if modality is None:
        return PRESETS[preset][2]
    return 'flow_x' if modality == 'x' else f'flow_y_{transform_type}'


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--preset', choices=sorted(PRESETS), required=True)
    p.add_argument('--data', required=True, help='.npy / .pt tensor [N, C, H, W]')
    p.add_argument('--epochs', type=int, default=50)
    p.add_argument('--batch_size', type=int, default=128)
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--save_every', type=int, default=10, help='Save checkpoint every N epochs')
    p.add_argument('--patience', type=int, default=10, help='Early stopping patience')
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--resume', type=str, default=None, help='checkpoint to resume from')
    p.add_argument('--out_dir', type=str, default='checkpoints')
    p.add_argument('--modality', type=str, default=None, choices=['x', 'y'],
                   help='28x28 presets: which modality the data is (selects the checkpoint name)')
    p.add_argument('--transform_type', type=str, default='rotate90', help='names the y checkpoint')
    p.add_argument('--num_classes', type=int, default=None,
                   help="train a class-conditional net (U-Net presets): --data is then a .npz / .pt with 'x' [N,C,H,W] and "
                        "'label' [N] in 0..num_classes-1, as train_classifier reads; stored in the checkpoint")
    p.add_argument('--p_uncond', type=float, default=0.1,
                   help='--num_classes: probability that a label is replaced by the null label (classifier-free training)')
    add_optimizer_args(p)
    args = p.parse_args(argv)
    check_optimizer_args(p, args)
    if args.num_classes is not None and (args.num_classes < 1 or args.preset == 'original'):
        p.error("--num_classes: an integer >= 1, for the U-Net presets (mnist32, svhn, unet28)")
    if not 0.0 <= args.p_uncond <= 1.0:
        p.error("--p_uncond is a probability")
    if args.modality is not None and args.preset not in MODALITY_PRESETS:
        p.error(f"--modality applies to the presets {', '.join(MODALITY_PRESETS)}")
    if args.preset == 'original' and args.modality is None:
        p.error("--preset original requires --modality {x,y}")
    args.stem = checkpoint_stem(args.preset, args.modality, args.transform_type)
    return args


def load_data(path, shape):
    data = torch.load(path, map_location='cpu') if path.endswith('.pt') else torch.from_numpy(np.load(path))
    data = torch.as_tensor(data, dtype=torch.float32).contiguous()
    if data.dim() != 4 or tuple(data.shape[1:]) != shape:
        raise ValueError(f"{path}: expected a tensor [N, {shape[0]}, {shape[1]}, {shape[2]}], got {tuple(data.shape)}")
    return data


def load_labelled(path, shape, num_classes):
    """(x, label) of a .npz / .pt data file with 'x' [N, C, H, W] and 'label' [N] in 0..num_classes-1."""
    d = torch.load(path, map_location='cpu') if path.endswith('.pt') else np.load(path)
    for key in ('x', 'label'):
        if key not in d:
            raise ValueError(f"{path}: --num_classes needs a file with 'x' and 'label' (missing {key!r})")
    x = torch.as_tensor(np.asarray(d['x']), dtype=torch.float32).contiguous()
    label = torch.as_tensor(np.asarray(d['label'])).long().reshape(-1)
    if x.dim() != 4 or tuple(x.shape[1:]) != shape:
        raise ValueError(f"{path}: expected x [N, {shape[0]}, {shape[1]}, {shape[2]}], got {tuple(x.shape)}")
    if x.shape[0] != label.shape[0] or x.shape[0] == 0:
        raise ValueError(f"{path}: x and label must have the same, non-zero length")
    if int(label.min()) < 0 or int(label.max()) >= num_classes:
        raise ValueError(f"{path}: labels must be in 0..{num_classes - 1}")
    return x, label


def batches(data, batch_size, gen, label=None):
    """The reference loaders' shuffle=True, drop_last=False epoch order; with `label`, (x, label) batches."""
    perm = torch.randperm(data.shape[0], generator=gen)
    for i in range(0, data.shape[0], batch_size):
        if label is not None:
            yield data[perm[i:i + batch_size]], label[perm[i:i + batch_size]]
        else:
            yield {'x': data[perm[i:i + batch_size]]}


def checkpoint(epoch, model, optimizer, best_loss):
    """The reference's checkpoint dict; with an optimizer that keeps an EMA of the weights (--optimizer hip --ema_decay)
    also 'ema_state_dict', the averaged weights under the model's keys (load_checkpoint(..., ema=True))."""
    ck = {'epoch': epoch, 'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(),
          'best_loss': best_loss}
    if getattr(model, 'num_classes', None) is not None:  # (a class-conditional net: load_checkpoint checks it)
        ck['num_classes'] = model.num_classes
    if getattr(optimizer, 'ema_decay', None) is not None:
        ck['ema_state_dict'] = optimizer.ema_state_dict(model)
    return ck


def main(argv=None):
    args = parse_args(argv)
    set_seed(args.seed)
    ctor, shape, _ = PRESETS[args.preset]
    stem = args.stem
    device = torch.device(args.device)
    label = None
    if args.num_classes is not None:
        data, label = load_labelled(args.data, shape, args.num_classes)
        model = ctor(num_classes=args.num_classes).to(device)
    else:
        data = load_data(args.data, shape)
        model = ctor().to(device)
    optimizer = build_optimizer(args, model.parameters())
    schedule = CFMSchedule()
    start_epoch, best_loss = 0, float('inf')
    if args.resume:
        ckpt = torch.load(args.resume, map_location=device)
        if isinstance(ckpt, dict) and 'model_state_dict' in ckpt:
            model.load_state_dict(ckpt['model_state_dict'])
            if 'optimizer_state_dict' in ckpt:
                optimizer.load_state_dict(ckpt['optimizer_state_dict'])
            start_epoch = ckpt.get('epoch', 0)
            best_loss = ckpt.get('best_loss', best_loss)
        else:
            model.load_state_dict(ckpt)
        print(f"Resumed from {args.resume}: epoch {start_epoch}, best_loss={best_loss:.4f}")
    os.makedirs(args.out_dir, exist_ok=True)
    gen = torch.Generator().manual_seed(args.seed)
    patience_counter = 0
    for epoch in range(start_epoch, args.epochs):
        avg_loss = train_flow_matching_epoch(model, batches(data, args.batch_size, gen, label), optimizer, schedule, device,
                                             p_uncond=args.p_uncond)
        print(f"Epoch {epoch + 1}/{args.epochs} - Loss: {avg_loss:.4f}")
        if avg_loss < best_loss:
            best_loss, patience_counter = avg_loss, 0
            path = os.path.join(args.out_dir, f'{stem}_best.pth')
            torch.save(checkpoint(epoch + 1, model, optimizer, best_loss), path)
            print(f"  -> Saved best model: {path}")
        else:
            patience_counter += 1
        if (epoch + 1) % args.save_every == 0:
            path = os.path.join(args.out_dir, f'{stem}_epoch{epoch + 1}.pth')
            torch.save(checkpoint(epoch + 1, model, optimizer, best_loss), path)
            print(f"  -> Saved checkpoint: {path}")
        if patience_counter >= args.patience:
            print(f"\nEarly stopping after {epoch + 1} epochs")
            break
    print(f"\nTraining complete! Best loss: {best_loss:.4f}")
    return best_loss


if __name__ == '__main__':
    main()
