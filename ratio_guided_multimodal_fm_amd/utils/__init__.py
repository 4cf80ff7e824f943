"""Seeding and checkpoint ingestion (reference ``src/utils/__init__.py``)."""
import random

import numpy as np
import torch


def set_seed(seed: int = 42):
    """Seed python / numpy / torch generators (reference :7-22).

    The samplers draw their noise from the global torch generator of the
    target device in the reference order x0, y0, mc_x0, mc_y0.
    """
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)


def load_checkpoint(model, path, device='cpu', ema=False):
    """Load either checkpoint format the reference writes (reference :25-51).

    ``{'model_state_dict': ..., 'epoch': ..., 'best_loss': ...}`` dicts
    (train_flow_mnist32.py / train_flow_svhn.py) or a raw ``state_dict``
    (train_flow.py, ratio and classifier trainers).  Returns
    ``{'epoch', 'best_loss'}`` for the dict format, ``{}`` otherwise.

    ``ema=True`` loads the averaged weights instead: the ``'ema_state_dict'`` a dict checkpoint of
    ``train_flow --optimizer hip --ema_decay ...`` carries; a file without one is an error.

    A dict checkpoint of a class-conditional net (``train_flow --num_classes K``) carries ``'num_classes'``: it must be
    the model's (``ValueError`` otherwise, before any tensor is loaded) and is returned with the other entries.
    """
    ckpt = torch.load(path, map_location=device)
    extra = {}
    if isinstance(ckpt, dict) and ckpt.get('num_classes') is not None:
        if ckpt['num_classes'] != getattr(model, 'num_classes', None):
            raise ValueError(f"{path} holds a net with num_classes={ckpt['num_classes']}, the model was built with "
                             f"num_classes={getattr(model, 'num_classes', None)} (--num_classes)")
        extra = {'num_classes': ckpt['num_classes']}
    if ema:
        if not (isinstance(ckpt, dict) and 'ema_state_dict' in ckpt):
            raise KeyError(f"{path} has no 'ema_state_dict': it was not trained with --optimizer hip --ema_decay "
                           "(the ratio and classifier trainers write the averaged weights to <name>_ema.pth instead)")
        model.load_state_dict(ckpt['ema_state_dict'])
        return {'epoch': ckpt.get('epoch', 0), 'best_loss': ckpt.get('best_loss', float('inf')), **extra}
    if isinstance(ckpt, dict) and 'model_state_dict' in ckpt:
        model.load_state_dict(ckpt['model_state_dict'])
        return {'epoch': ckpt.get('epoch', 0), 'best_loss': ckpt.get('best_loss', float('inf')), **extra}
    model.load_state_dict(ckpt)
    return {}
