"""The optimizer step on the HIP kernels of csrc/optim.hip: Adam / AdamW, global-norm clipping and a weight EMA.

``Adam`` is a ``torch.optim.Optimizer``: ``zero_grad``, ``param_groups`` and the lr schedulers work as with
``torch.optim.Adam``, whose update it computes (``amsgrad=False, maximize=False``; ``decoupled=True`` is AdamW).  One
``step()`` is a table upload and two launches -- the norm of all gradients, then clip + update + EMA in one pass per
parameter group -- on the current stream, with no read-back and no wait on the device.

What differs from the torch pieces it replaces:

* the clip (``max_grad_norm``) is ``torch.nn.utils.clip_grad_norm_``'s formula, applied inside the update:
  ``p.grad`` is left UNSCALED.  ``grad_norm`` is a device tensor with the latest norm before clipping
  (``max_grad_norm=float('inf')`` reports it without clipping);
* the state lives in three flat buffers (``exp_avg``, ``exp_avg_sq``, ``ema``); ``state[p]`` holds views into them,
  and ``load_state_dict`` copies INTO them instead of replacing them;
* ``state[p]['step']`` is brought up to date by ``state_dict()`` (the step itself counts in a host array);
* there is no CPU path: ``step()`` on CPU parameters raises ``RgfmError``.

The EMA (``ema_decay``) starts as a copy of the parameters at construction.  ``ema_state_dict(model)`` is the
checkpoint to sample from; ``swap_ema(model)`` evaluates with the averaged weights in place.
"""
import contextlib
import ctypes
import os
from itertools import chain

import numpy as np
import torch

from .. import _lib

_ENTRY = np.dtype([("param", "<u8"), ("grad", "<u8"), ("offset", "<u8"), ("numel", "<u8"), ("bc1", "<f8"), ("bc2", "<f8")])
assert _ENTRY.itemsize == ctypes.sizeof(_lib.AdamEntry)


class _TableSlot:
    """One upload of the table: pinned staging memory, its device copy and the event behind the copy.  The host may
    rewrite the staging memory only once the event has completed -- the asynchronous copy reads it when the stream gets
    there, not when it is enqueued."""

    def __init__(self, nbytes, device):
        self.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.event = None

    def free(self):
        return self.event is None or self.event.query()


class Adam(torch.optim.Optimizer):
    """Adam / AdamW + global-norm clip + weight EMA in two HIP launches (rgfm_adam_grad_norm, rgfm_adam_step)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                 max_grad_norm=None, ema_decay=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("lr must be a number (it is read on the host at every step)")
        if not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not eps >= 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not weight_decay >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 or None, got {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError(f"ema_decay must be in [0, 1] or None, got {ema_decay}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.grad_norm = None  # device scalar: the latest norm before clipping (set by the first step that takes one)
        self._flat = None
        # (torch's name for the AdamW switch, so that a torch.optim.Adam loading this state_dict follows it)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled)))
        self._allocate()

    # ---- state ---------------------------------------------------------
    def _params(self):
        return list(chain.from_iterable(g["params"] for g in self.param_groups))

    def add_param_group(self, param_group):
        if self._flat is not None:  # (the flat state is laid out once, over the groups given to the constructor)
            raise _lib.RgfmError("parameter groups cannot be added after construction: pass every group to Adam(...)")
        super().add_param_group(param_group)

    def _buffers(self):
        return ("exp_avg", "exp_avg_sq") + (("ema",) if self.ema_decay is not None else ())

    def _allocate(self):
        """The flat buffers (every tensor's slot padded to 4 floats) and the per-parameter views into them."""
        params = self._params()
        devices = {p.device for p in params}
        if len(devices) > 1:
            raise _lib.RgfmError(f"all parameters must be on one device, got {sorted(map(str, devices))}")
        for p in params:
            if p.dtype != torch.float32 or p.is_sparse:
                raise _lib.RgfmError(f"dense fp32 parameters expected, got {p.dtype}")
        self._order = params
        self._index = {p: i for i, p in enumerate(params)}
        self._numel = np.array([p.numel() for p in params], dtype=np.uint64)
        padded = (self._numel + np.uint64(3)) // np.uint64(4) * np.uint64(4)
        self._offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.uint64)
        self._total = int(padded.sum())
        self._steps = np.zeros(len(params), dtype=np.int64)
        device = params[0].device
        self._flat = {k: torch.zeros(max(self._total, 4), dtype=torch.float32, device=device) for k in self._buffers()}
        for i, p in enumerate(params):
            o, n = int(self._offset[i]), int(self._numel[i])
            st = self.state[p]
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            for k, buf in self._flat.items():
                st[k] = buf[o:o + n].view(p.shape)
            if self.ema_decay is not None:
                st["ema"].copy_(p.detach())
        self._key, self._table, self._slots, self._ws = None, None, [], None

    def _sync_steps(self):
        for i, p in enumerate(self._order):
            self.state[p]["step"] = torch.tensor(float(self._steps[i]), dtype=torch.float32)

    def state_dict(self):
        """torch.optim.Adam's format -- per parameter 'step', 'exp_avg', 'exp_avg_sq' -- plus 'ema' when one is kept:
        torch.optim.Adam loads it and ignores the extra key."""
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Loads a state written by this class or by torch.optim.Adam (the EMA then starts from the parameters).  The
        values are copied INTO the flat buffers: state[p] keeps aliasing them.  A parameter the state does not mention
        starts from zero moments."""
        groups, saved = self.param_groups, state_dict["param_groups"]
        if len(groups) != len(saved):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(g["params"]) != len(s["params"]) for g, s in zip(groups, saved)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        id_map = dict(zip(chain.from_iterable(s["params"] for s in saved), self._params()))
        loaded = {id_map[k]: v for k, v in state_dict["state"].items() if k in id_map}
        with torch.no_grad():
            for i, p in enumerate(self._order):
                st, src = self.state[p], loaded.get(p, {})
                step = src.get("step", 0)
                self._steps[i] = int(round(float(step)))
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in src:
                        st[k].copy_(src[k])
                    else:
                        st[k].zero_()
                if self.ema_decay is not None:
                    st["ema"].copy_(src["ema"] if "ema" in src else p.detach())
        for g, s in zip(groups, saved):
            g.update({k: v for k, v in s.items() if k not in ("params", "param_names")})
        self._sync_steps()
        self._key = None

    # ---- the step ------------------------------------------------------
    def _slot(self, nbytes, device):
        for s in self._slots:
            if s.host.numel() >= nbytes and s.free():
                return s
        self._slots = [s for s in self._slots if not s.free()]  # (outgrown or still in flight: those stay until done)
        self._slots.append(_TableSlot(max(nbytes, 4096), device))
        return self._slots[-1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        idx, grads = [], []
        for p in self._order:
            g = p.grad
            if g is None:
                continue
            if not p.is_cuda or not g.is_cuda:
                raise _lib.RgfmError(f"this optimizer runs only on a HIP device (MI355X): got a parameter on '{p.device}'. "
                                     "There is no CPU path; move the model to 'cuda' before building the optimizer.")
            if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                raise _lib.RgfmError(f"dense fp32 gradients on {p.device} expected, got {g.dtype} on {g.device}")
            if not p.is_contiguous():
                raise _lib.RgfmError("parameters must be contiguous")
            idx.append(self._index[p])
            grads.append(g if g.is_contiguous() else g.contiguous())  # (a copy lives until the launches are enqueued)
        if not idx:
            return loss
        device = self._order[idx[0]].device
        key = tuple(chain(idx, (self._order[i].data_ptr() for i in idx), (g.data_ptr() for g in grads)))
        if key != self._key:  # a pointer moved (or another set of parameters has gradients): gather the table again
            ii = np.asarray(idx)
            t = np.zeros(len(idx), dtype=_ENTRY)
            t["param"] = [self._order[i].data_ptr() for i in idx]
            t["grad"] = [g.data_ptr() for g in grads]
            t["offset"], t["numel"] = self._offset[ii], self._numel[ii]
            # per group: (first entry, number of entries, span) -- a group's entries are consecutive
            bounds = []
            pos = {i: k for k, i in enumerate(idx)}
            for group in self.param_groups:
                ks = [pos[self._index[p]] for p in group["params"] if self._index[p] in pos]
                if ks:
                    end = int(t["offset"][ks[-1]] + (t["numel"][ks[-1]] + np.uint64(3)) // np.uint64(4) * np.uint64(4))
                    bounds.append((group, ks[0], len(ks), int(t["offset"][ks[0]]), end))
            self._key, self._table, self._ii, self._bounds = key, t, ii, bounds
        t, ii = self._table, self._ii
        self._steps[ii] += 1
        steps = self._steps[ii].astype(np.float64)
        # (a table spans groups with their own betas: the bias corrections are taken per group below)
        L = _lib.lib()
        with torch.cuda.device(device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            for group, k0, n, _, _ in self._bounds:
                b1, b2 = group["betas"]
                t["bc1"][k0:k0 + n] = 1.0 - np.power(float(b1), steps[k0:k0 + n])
                t["bc2"][k0:k0 + n] = 1.0 - np.power(float(b2), steps[k0:k0 + n])
            nbytes = t.nbytes
            slot = self._slot(nbytes, device)
            slot.host[:nbytes].numpy()[:] = t.view(np.uint8)
            slot.dev[:nbytes].copy_(slot.host[:nbytes], non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record()
            if self._ws is None:
                nb = ctypes.c_size_t()
                _lib.check(L.rgfm_adam_workspace_bytes(ctypes.byref(nb)))
                self._ws = torch.empty(nb.value, dtype=torch.uint8, device=device)
            want_norm = self.max_grad_norm is not None
            if want_norm:
                if self.grad_norm is None:
                    self.grad_norm = torch.zeros((), dtype=torch.float32, device=device)
                _lib.check(L.rgfm_adam_grad_norm(slot.dev.data_ptr(), len(idx), self._bounds[0][3], self._bounds[-1][4],
                                                 self._ws.data_ptr(), self._ws.numel(), stream))
            ema = self._flat.get("ema")
            for group, k0, n, begin, end in self._bounds:
                d = _lib.AdamDesc()
                d.lr = float(group["lr"])
                d.betas[0], d.betas[1] = map(float, group["betas"])
                d.eps, d.weight_decay = float(group["eps"]), float(group["weight_decay"])
                d.decoupled = 1 if group.get("decoupled_weight_decay", False) else 0
                d.max_grad_norm = self.max_grad_norm if want_norm else 0.0
                d.ema_decay = self.ema_decay if ema is not None else -1.0
                _lib.check(L.rgfm_adam_step(
                    ctypes.byref(d), slot.dev.data_ptr() + k0 * _ENTRY.itemsize, n, begin, end,
                    self._flat["exp_avg"].data_ptr(), self._flat["exp_avg_sq"].data_ptr(),
                    ema.data_ptr() if ema is not None else None,
                    self.grad_norm.data_ptr() if want_norm else None,
                    self._ws.data_ptr() if want_norm else None, self._ws.numel() if want_norm else 0, stream))
        # the kernels wrote through raw pointers: tell autograd -- and with it the engines' handle caches, which key on
        # the version counters -- that the values moved
        torch.autograd.graph.increment_version([self._order[i] for i in idx])
        return loss

    # ---- EMA -----------------------------------------------------------
    def _require_ema(self):
        if self.ema_decay is None:
            raise _lib.RgfmError("this optimizer keeps no EMA: build it with ema_decay=...")

    def ema_state_dict(self, model):
        """model.state_dict() with every parameter this optimizer averages replaced by its average (a copy); buffers
        -- the BatchNorm running statistics -- and other parameters are copied as they are."""
        self._require_ema()
        named = dict(model.named_parameters(remove_duplicate=False))
        out = type(sd := model.state_dict())()
        for k, v in sd.items():
            p = named.get(k)
            out[k] = (self.state[p]["ema"] if p is not None and p in self._index else v).detach().clone()
        return out

    @contextlib.contextmanager
    def swap_ema(self, model):
        """Evaluate `model` with the averaged weights: inside the block the parameters hold the EMA (and the EMA buffer
        the live weights), afterwards they are swapped back.  Both swaps are in-place copies that raise the
        parameters' version counters, so the engines re-pack their handles.  Do not step inside the block."""
        self._require_ema()
        mine = [p for p in model.parameters() if p in self._index]

        def swap():
            with torch.no_grad():
                for p in mine:
                    e = self.state[p]["ema"]
                    tmp = p.detach().clone()
                    p.copy_(e)
                    e.copy_(tmp)
        swap()
        try:
            yield model
        finally:
            swap()


# ---- the trainers' command lines ------------------------------------------------------------------------------------
def add_optimizer_args(parser):
    """--optimizer {torch,hip} and the three options only the HIP optimizer has (check_optimizer_args enforces that)."""
    parser.add_argument('--optimizer', choices=['torch', 'hip'], default='torch',
                        help="torch: torch.optim.Adam; hip: this package's fused Adam + clip + EMA step")
    parser.add_argument('--ema_decay', type=float, default=None, help='--optimizer hip: keep an EMA of the weights')
    parser.add_argument('--max_grad_norm', type=float, default=None, help='--optimizer hip: clip the global gradient norm')
    parser.add_argument('--weight_decay', type=float, default=None, help='--optimizer hip: decoupled (AdamW) weight decay')


def check_optimizer_args(parser, args):
    if args.optimizer != 'hip':
        for name in ('ema_decay', 'max_grad_norm', 'weight_decay'):
            if getattr(args, name) is not None:
                parser.error(f"--{name} needs --optimizer hip")


def build_optimizer(args, params, default_max_grad_norm=None):
    """The optimizer the command line asks for: torch.optim.Adam(lr) as before, or Adam of this module."""
    if args.optimizer != 'hip':
        return torch.optim.Adam(params, lr=args.lr)
    clip = args.max_grad_norm if args.max_grad_norm is not None else default_max_grad_norm
    wd = args.weight_decay or 0.0
    return Adam(params, lr=args.lr, weight_decay=wd, decoupled=wd > 0.0, max_grad_norm=clip, ema_decay=args.ema_decay)


def ema_path(path):
    """<name>_ema.pth beside <name>.pth: where the trainers that write raw state_dicts put the averaged weights."""
    stem, ext = os.path.splitext(path)
    return f"{stem}_ema{ext}"
