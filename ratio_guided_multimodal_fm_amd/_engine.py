"""Host plumbing between the nn.Module parameter containers and the C ABI.

PyTorch is used for what it is good at here: owning device memory (parameter
blob, workspace, I/O tensors) and naming the stream.  All arithmetic happens
inside librgfm_hip.so.
"""
import collections
import ctypes
import math
import os
import weakref

import torch

from . import _lib

_LOSS = {"disc": 0, "rulsif": 1}
_RATIO_KIND = {"mnist_svhn": 0, "mnist28": 1, "flexible": 2}
_RATIO_OUT = {"score": 0, "log_ratio": 1, "ratio": 2}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_hip(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.RgfmError(
                "this package runs only on a HIP device (MI355X): got a tensor on "
                f"'{t.device}'. There is no CPU path; move the model and inputs to 'cuda'.")
        if t.dtype != torch.float32:
            raise _lib.RgfmError(f"fp32 tensors expected, got {t.dtype}")


class _Workspace:
    """Grow-only byte buffer per device, shared by every call that goes through it.

    The calls are ordered by the stream they run on.  When the current stream is not the one that took the buffer
    last, it is made to wait for the streams that used the buffer since the last such hand-over -- a call on another
    stream then starts behind the work that is still pending in the scratch (also when it grows the buffer: one rule).
    A caller that stays on one stream enqueues nothing."""

    def __init__(self):
        self.buf = None
        self.streams = set()
        self.last = None  # the stream of the latest get

    def get(self, nbytes, device):
        cur = torch.cuda.current_stream(device)
        waited = False
        if self.last is not None and cur != self.last and self.buf is not None and self.buf.device == device:
            for st in self.streams:
                if st != cur:
                    cur.wait_stream(st)
            waited = True
        self.last = cur
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            old = self.buf
            self.buf = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
            if old is not None:
                # work already enqueued on other streams may still use the old buffer: keep the
                # caching allocator from handing its memory out before those streams get there
                for st in self.streams:
                    old.record_stream(st)
            self.streams = set()
        elif waited:
            # everything those streams enqueued now precedes `cur`: from here on `cur` stands for them
            self.streams = set()
        self.streams.add(cur)
        return self.buf


def engine_property(factory):
    """Class attribute `_engine = engine_property(factory)`: the module's engine, built on first use.

    The engine is a per-module cache (device handle, packed weights, workspace) kept out of
    state_dict, deepcopy and pickling: a copied / unpickled module simply builds its own.
    """
    def get(module):
        e = module.__dict__.get("_engine_obj")
        if e is None or e._module() is not module:
            e = factory(module)
            module.__dict__["_engine_obj"] = e
        return e
    return property(get)


# ---- range guard of the default fp16 conv path -------------------------------------------------
# The fp16 two-plane convs (conv_mfma_hx2*.hip) emulate fp32 products inside a window: activations
# below 2048, and residual-stream tensors (consumed without a GroupNorm in front) not smaller than
# 2^-8 per 64-pixel block.  Outside it a launch raises the range flag of ITS HANDLE instead of
# returning degraded numbers.  Every public compute entry point below runs under _range_guarded:
# if a flag of one of the engines involved is up after the call, the in-place state is restored
# and the call is repeated with those handles switched to the split-bf16 convs (too large: fp32 exponent
# range) or the exact fp32 matrix-core convs (too small) -- rgfm_*_set_conv_mode, a handle setting,
# nothing process-wide is touched.  RGFM_RANGE_CHECK=0
# disables the check (and its end-of-call synchronisation), e.g. for stream capture.
CONV_DEFAULT, CONV_HX2, CONV_BX3, CONV_F32 = -1, 0, 1, 2


def _hx2_active():
    return os.environ.get("RGFM_CONV", "hx2") == "hx2" and os.environ.get("RGFM_RANGE_CHECK", "1") != "0"


range_fallbacks = 0  # number of calls repeated on the bf16 path (tests read it)
last_range_flags = 0  # OR of the flag bits that caused the latest fallback (1: too large, 2: too small)


def _range_guarded(device, state, fn, engines):
    """fn() with the fp16-range check; `state` = tensors fn updates in place, `engines` = the
    velocity-net engines whose handles fn launches on."""
    global range_fallbacks, last_range_flags
    engines = [e for i, e in enumerate(engines) if e is not None and all(e is not o for o in engines[:i])]
    if not _hx2_active() or not engines:
        return fn()
    saved = [t.clone() for t in state]
    out = fn()
    bits = 0
    with torch.cuda.device(device):
        for e in engines:
            bits |= e.read_range_flag(device)
    if bits:
        range_fallbacks += 1
        last_range_flags = bits
        for t, t0 in zip(state, saved):
            t.copy_(t0)
        # too large (bit 0): the split-bf16 convs have fp32's exponent range at the top; too small (bit 1): the repeat
        # runs on the exact fp32 matrix-core convs, which ARE the reference's arithmetic at any magnitude
        fallback = CONV_F32 if bits & 2 else CONV_BX3
        with torch.cuda.device(device):
            for e in engines:
                e.set_conv_mode(device, fallback)
            try:
                out = fn()
            finally:
                for e in engines:
                    e.set_conv_mode(device, CONV_DEFAULT)
    return out


def _same_tensors(key, old):
    """Two _state_key tuples that differ at most in the tensors' version counters."""
    return [(k, p, d) for k, p, _, d in key] == [(k, p, d) for k, p, _, d in old]


class _EngineBase:
    """Per-module cache of the device handle; subclasses name the ABI family and describe the architecture."""
    PREFIX = None       # rgfm_<family>_{update_params,destroy,...}
    DESC_PREFIX = None  # rgfm_<family>_{param_floats,create}, where the descriptor has a family of its own

    def __init__(self, module):
        self._module = weakref.ref(module)
        self._handle = None
        self._key = None
        self._blob = None
        self._layout = None      # per state_dict entry: (numel, is it a parameter?), as of the latest create
        self._last_train = None  # (weakref of the workspace, batch, handle, family's extra) of the latest forward_train
        self._ws = _Workspace()

    # engines are per-module caches: never copied or pickled with the module (engine_property rebuilds them)
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())

    def _fn(self, name, prefix=None):
        return getattr(_lib.lib(), f"{prefix or self.PREFIX}_{name}")

    def desc(self):
        raise NotImplementedError

    def _key_extra(self):
        """What the handle depends on besides the module's tensors."""
        return None

    def _create_variant(self):
        """(prefix of the param_floats / create entry points, their arguments behind the descriptor)."""
        return self.DESC_PREFIX, ()

    def _state_key(self, sd):
        return tuple((k, v.data_ptr(), v._version, str(v.device)) for k, v in sd.items())

    def handle(self, device):
        """The module's device handle: the cached one while nothing moved, the same one re-packed in place when only
        the values of the same tensors moved (an optimizer step, the running statistics), a new one otherwise."""
        m = self._module()
        sd = m.state_dict()
        key, extra = self._state_key(sd), self._key_extra()
        if self._handle is not None and (key, extra) == self._key:
            return self._handle
        blob = self._blob_from(sd, device)
        if self._handle is not None and extra == self._key[1] and _same_tensors(key, self._key[0]):
            with torch.cuda.device(device):
                _lib.check(self._fn("update_params")(self._handle, _ptr(blob), blob.numel(), _stream(device)))
            self._key, self._blob = (key, extra), blob
            return self._handle
        if self._handle is not None:
            self._destroy()
        d = self.desc()
        n = ctypes.c_size_t()
        prefix, more = self._create_variant()
        _lib.check(self._fn("param_floats", prefix)(ctypes.byref(d), *more, ctypes.byref(n)))
        if blob.numel() != n.value:
            raise _lib.RgfmError(f"parameter blob has {blob.numel()} floats, library expects {n.value}")
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(self._fn("create", prefix)(ctypes.byref(d), *more, _ptr(blob), blob.numel(), _stream(device),
                                                  ctypes.byref(h)))
        self._handle, self._key, self._blob = h, (key, extra), blob
        named = {id(q) for q in m.parameters()}
        self._layout = [(v.numel(), id(v) in named) for v in m.state_dict(keep_vars=True).values()]
        return h

    def _destroy(self):
        self._fn("destroy")(self._handle)
        self._handle = None

    def owns(self, handle):
        """Is `handle` (as handle() returned it) still alive in this engine?"""
        return self._handle is handle

    def _saved(self):
        """(workspace, batch, handle, the family's extra) of the latest forward_train, until its backward has run."""
        ws = self._last_train[0]() if self._last_train else None
        if ws is None:
            raise _lib.RgfmError("no saved state: call this between forward_train and its backward")
        _, n, h, extra = self._last_train
        if not self.owns(h):
            raise _lib.RgfmError("the module's handle was re-created since that forward_train")
        return ws, n, h, extra

    def __del__(self):
        try:
            if self._handle is not None:
                self._destroy()
        except Exception:
            pass

    def _blob_from(self, sd, device):
        parts = [v.detach().reshape(-1).to(device=device, dtype=torch.float32) for v in sd.values()]
        return torch.cat(parts).contiguous()

    def _check_eval(self, module):
        if module.training:
            raise _lib.RgfmError(
                f"{type(module).__name__} is in training mode; the HIP path implements eval-mode "
                "semantics only (Dropout = identity, BatchNorm = running statistics). Call .eval().")


class _TrainSpec:
    """What one family contributes to _TrainFn: how many tensors are inputs and how many of them (the leading ones) can
    get a gradient, the output shape, the arguments of rgfm_<family>_forward_train between the handle and the
    workspace, whether the pass has dropout, whether it takes the `training` flag and reports BatchNorm statistics,
    and what it leaves in engine._last_train."""

    def __init__(self, inputs, grads, out_shape, args, dropout=False, batchnorm=False, last=None, fn="forward_train"):
        self.inputs, self.grads, self.out_shape, self.args = inputs, grads, out_shape, args
        self.dropout, self.batchnorm, self.last = dropout, batchnorm, last
        self.fn = fn  # the forward's entry point, rgfm_<family>_<fn>; the backward is the family's one


class _TrainFn(torch.autograd.Function):
    """Training forward / backward of every family through rgfm_<family>_forward_train / rgfm_<family>_backward.

    Inputs: the family's _TrainSpec, the engine, p_drop, the input tensors and the module's parameters (state_dict
    order), so that autograd hands back the input gradients and every dL/dparam.  Each call owns its saved-state buffer
    and runs its backward on the handle of its forward; the dropout seed is drawn from the device's torch generator.
    While a module with BatchNorm trains, its buffers are updated from the batch statistics the library reports."""

    @staticmethod
    def forward(ctx, spec, engine, p_drop, *tensors):
        m = engine._module()
        inputs = [v.contiguous() for v in tensors[:spec.inputs]]
        dev, n = inputs[0].device, inputs[0].shape[0]
        out = torch.empty(spec.out_shape(*inputs), device=dev)
        ctx.spec, ctx.engine, ctx.n, ctx.ws, ctx.nbytes, ctx.h = spec, engine, n, None, 0, None
        ctx.save_for_backward(*tensors[spec.inputs:])
        ctx.shapes = [v.shape for v in inputs[:spec.grads]]
        if n == 0:
            return out
        training = spec.batchnorm and bool(m.training)
        seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item()) if p_drop > 0 else 0
        bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)] if training else []
        stats = torch.empty(2 * sum(b.num_features for b in bns), device=dev) if bns else None
        with torch.cuda.device(dev):
            h = engine.handle(dev)
            nb = ctypes.c_size_t()
            _lib.check(engine._fn("train_workspace_bytes")(h, n, ctypes.byref(nb)))
            ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
            _lib.check(engine._fn(spec.fn)(
                h, *spec.args(*inputs, out, n, 1 if training else 0, p_drop, seed, _ptr(stats)), _ptr(ws), nb.value,
                _stream(dev)))
        off = 0
        for b in bns:  # nn.BatchNorm2d's update: momentum 0.1, unbiased batch variance
            st = stats[off:off + 2 * b.num_features].view(-1, 2)
            off += 2 * b.num_features
            mom = b.momentum
            b.running_mean.mul_(1 - mom).add_(st[:, 0], alpha=mom)
            b.running_var.mul_(1 - mom).add_(st[:, 1], alpha=mom)
            b.num_batches_tracked.add_(1)
        ctx.ws, ctx.nbytes, ctx.h, ctx.layout = ws, nb.value, h, engine._layout
        engine._last_train = (weakref.ref(ws), n, h, spec.last(engine, seed, p_drop) if spec.last else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        spec, params, dev = ctx.spec, ctx.saved_tensors, dout.device
        need = ctx.needs_input_grad[3:3 + spec.grads]
        rest = (None,) * (spec.inputs - spec.grads)
        if ctx.n == 0:
            dins = [torch.zeros(sh, device=dev) if nd else None for sh, nd in zip(ctx.shapes, need)]
            return (None, None, None, *dins, *rest, *[torch.zeros_like(q) for q in params])
        if ctx.ws is None:
            raise _lib.RgfmError("the saved state of this forward_train call is gone (backward ran twice?)")
        if not ctx.engine.owns(ctx.h):
            raise _lib.RgfmError("the module's handle was re-created between forward_train and backward")
        dout = dout.to(torch.float32).contiguous()
        dparams = torch.empty(sum(k for k, _ in ctx.layout), device=dev)
        dins = [torch.empty(sh, device=dev) if nd else None for sh, nd in zip(ctx.shapes, need)]
        with torch.cuda.device(dev):
            _lib.check(ctx.engine._fn("backward")(ctx.h, _ptr(dout), *map(_ptr, dins), _ptr(dparams), ctx.n, _ptr(ctx.ws),
                                                  ctx.nbytes, _stream(dev)))
        ctx.ws = None
        chunks = torch.split(dparams, [k for k, _ in ctx.layout])  # the buffers' slots are dropped
        grads = [g.view(q.shape) for g, q in zip([c for c, (_, is_p) in zip(chunks, ctx.layout) if is_p], params)]
        return (None, None, None, *dins, *rest, *grads)


# The exports of a sampler loop, one row each: the entry point and its workspace query, their *_diag pair, the *_gs entry
# point (a strength per row / per stage; no query of its own), and for the U-Net pair the cross-pairing entry points (one
# query for calls with and without records), and the *_sde entry points (the stochastic step; workspace: the query the
# call would use without it plus rgfm_sde_scratch_bytes), and the *_ess entry point (the effective-sample-size floor of the
# MC loops; no workspace of its own).  None: the loop has no such export.  _run_loop picks from the row.
_Loop = collections.namedtuple("_Loop", "fn ws diag diag_ws gs cross cross_ws cross_gs sde cross_sde ess", defaults=(None,) * 9)
_SINGLE = _Loop("rgfm_sample_single_ode", "rgfm_sample_single_ode_workspace_bytes", sde="rgfm_sample_single_sde")
_TWO = _Loop("rgfm_sample_two", "rgfm_sample_two_workspace_bytes")
_PAIR = _Loop("rgfm_sample_pair_ode", "rgfm_sample_pair_ode_workspace_bytes",
              "rgfm_sample_pair_diag", "rgfm_sample_pair_diag_workspace_bytes", "rgfm_sample_pair_gs",
              "rgfm_sample_pair_cross", "rgfm_sample_pair_cross_workspace_bytes", "rgfm_sample_pair_cross_gs",
              "rgfm_sample_pair_sde", "rgfm_sample_pair_cross_sde", ess="rgfm_sample_pair_ess")
_PAIR_GRAD = _Loop("rgfm_sample_pair_grad_ode", "rgfm_sample_pair_grad_ode_workspace_bytes",
                   "rgfm_sample_pair_grad_diag", "rgfm_sample_pair_grad_diag_workspace_bytes", "rgfm_sample_pair_grad_gs",
                   sde="rgfm_sample_pair_grad_sde")
_COND = _Loop("rgfm_sample_cond_ode", "rgfm_sample_cond_ode_workspace_bytes",
              "rgfm_sample_cond_diag", "rgfm_sample_cond_diag_workspace_bytes", "rgfm_sample_cond_gs",
              sde="rgfm_sample_cond_sde", ess="rgfm_sample_cond_ess")
_COND_GRAD = _Loop("rgfm_sample_cond_grad_ode", "rgfm_sample_cond_grad_ode_workspace_bytes",
                   "rgfm_sample_cond_grad_diag", "rgfm_sample_cond_grad_diag_workspace_bytes", "rgfm_sample_cond_grad_gs",
                   sde="rgfm_sample_cond_grad_sde")
_FM_SINGLE = _Loop("rgfm_fmnet_sample_single", "rgfm_fmnet_workspace_bytes")
_FM_PAIR = _Loop("rgfm_fmnet_sample_pair", "rgfm_fmnet_sample_pair_workspace_bytes",
                 "rgfm_fmnet_sample_pair_diag", "rgfm_fmnet_sample_pair_diag_workspace_bytes")
_GUIDED_LOOPS = (_PAIR, _PAIR_GRAD, _COND, _COND_GRAD, _FM_PAIR)


class _VelocityEngine(_EngineBase):
    """Shared handle cache / forward of the velocity nets; subclasses name the ABI family."""
    SINGLE = PAIR = None  # the family's _Loop rows
    TRAIN = None  # the family's _TrainSpec

    def _check_input(self, m, x):
        raise NotImplementedError

    def _check_xt(self, x, t):
        """x checked against the module, t flattened to its 1 or B elements; both contiguous."""
        _require_hip(x, t)
        self._check_input(self._module(), x)
        t = t.reshape(-1)
        if t.numel() not in (1, x.shape[0]):
            raise _lib.RgfmError(f"t must have 1 or {x.shape[0]} elements, got {t.numel()}")
        return x.contiguous(), t.contiguous()

    def check_labels(self, y, batch, device):
        """The labels of a call as the library takes them: None for `y` None, else a contiguous int32 tensor [batch] on
        `device`.  Every check runs here, before the library enqueues anything: the family has labels at all, the net
        was built with num_classes, `y` is an integer tensor [batch] with values in 0..num_classes."""
        if y is None:
            return None
        raise _lib.RgfmError(f"{type(self._module()).__name__} has no class labels (FlexibleUNet and its presets take "
                             "num_classes)")

    def forward_train(self, x, t, y=None):
        """v = model(x, t) on the exact-fp32 training path, differentiable w.r.t. x and the parameters (_TrainFn).  A
        net with Dropout applies it while the module trains; neither net has batch statistics.  `y`: labels
        (check_labels; U-Nets built with num_classes)."""
        m = self._module()
        x, t = self._check_xt(x, t)
        y = self.check_labels(y, x.shape[0], x.device)
        p = m.dropout_p() if self.TRAIN.dropout and m.training else 0.0
        if y is not None:
            return _TrainFn.apply(self.TRAIN_LABELS, self, float(p), x, t, y, *m.parameters())
        return _TrainFn.apply(self.TRAIN, self, float(p), x, t, *m.parameters())

    def workspace(self, fn_name, batch, device):
        L = _lib.lib()
        n = ctypes.c_size_t()
        _lib.check(getattr(L, fn_name)(self.handle(device), int(batch), ctypes.byref(n)))
        return self._ws.get(n.value, device), n.value

    def read_range_flag(self, device, reset=True):
        """Flag bits raised by this engine's launches since the last reset (waits for the current stream)."""
        flag = ctypes.c_int()
        _lib.check(self._fn("range_flag")(self.handle(device), ctypes.byref(flag), 1 if reset else 0, _stream(device)))
        return flag.value

    def set_conv_mode(self, device, mode):
        """Conv arithmetic of this engine's handle: CONV_DEFAULT (RGFM_CONV), CONV_HX2, CONV_BX3, CONV_F32."""
        _lib.check(self._fn("set_conv_mode")(self.handle(device), int(mode)))

    def forward(self, x, t, y=None):
        self._check_eval(self._module())
        x, t = self._check_xt(x, t)
        B = x.shape[0]
        y = self.check_labels(y, B, x.device)
        out = torch.empty_like(x)
        if B == 0:
            return out
        dev = x.device

        def run():
            with torch.cuda.device(dev):
                h = self.handle(dev)
                ws, nb = self.workspace(f"{self.PREFIX}_workspace_bytes", B, dev)
                if y is not None:
                    _lib.check(self._fn("forward_labels")(h, _ptr(x), _ptr(t), t.numel(), _ptr(y), _ptr(out), B, _ptr(ws),
                                                          nb, _stream(dev)))
                    return out
                _lib.check(self._fn("forward")(h, _ptr(x), _ptr(t), t.numel(), _ptr(out), B, _ptr(ws), nb,
                                               _stream(dev)))
            return out
        return _range_guarded(dev, [], run, [self])


class FmNetEngine(_VelocityEngine):
    """FlowMatchingModel ('--model original', reference src/models/flow_matching.py:127-173)."""
    PREFIX = "rgfm_fmnet"
    SINGLE, PAIR = _FM_SINGLE, _FM_PAIR
    TRAIN = _TrainSpec(inputs=2, grads=1, out_shape=lambda x, t: x.shape,
                       args=lambda x, t, out, n, training, p, seed, stats: (_ptr(x), _ptr(t), t.numel(), _ptr(out), n))

    def _check_eval(self, module):
        if module.training:
            raise _lib.RgfmError(
                f"{type(module).__name__} is in training mode; model(x, t) and the samplers are the eval path. Train "
                "through model.forward_train(x, t) (HIP backward), or call .eval() to evaluate / sample.")

    def desc(self):
        m = self._module()
        d = _lib.FmNetDesc()
        d.img_channels, d.feature_dim, d.time_emb_dim = m.img_channels, m.feature_dim, m.time_emb_dim
        return d

    def _check_input(self, m, x):
        if x.dim() != 4 or tuple(x.shape[1:]) != (m.img_channels, 28, 28):
            raise _lib.RgfmError(f"expected x of shape [B,{m.img_channels},28,28], got {tuple(x.shape)}")


class UNetEngine(_VelocityEngine):
    PREFIX = "rgfm_unet"
    # (the *_ode entry points take the solver id; with RGFM_SOLVER_EULER they are the Euler loops, bit for bit)
    SINGLE, PAIR = _SINGLE, _PAIR
    TRAIN = _TrainSpec(inputs=2, grads=1, out_shape=lambda x, t: x.shape, dropout=True,
                       args=lambda x, t, out, n, training, p, seed, stats: (_ptr(x), _ptr(t), t.numel(), _ptr(out), n, p, seed))
    # (with labels: rgfm_unet_forward_train_labels, the int32 labels a third input without a gradient)
    TRAIN_LABELS = _TrainSpec(inputs=3, grads=1, out_shape=lambda x, t, y: x.shape, dropout=True, fn="forward_train_labels",
                              args=lambda x, t, y, out, n, training, p, seed, stats: (_ptr(x), _ptr(t), t.numel(), _ptr(y),
                                                                                      _ptr(out), n, p, seed))

    def num_classes(self):
        """K of a class-conditional net (label_emb.weight: [K + 1, 4 model_channels]), or 0."""
        return int(getattr(self._module(), "num_classes", None) or 0)

    def _key_extra(self):
        return self.num_classes()

    def _create_variant(self):
        K = self.num_classes()
        return ("rgfm_unet_labeled", (K,)) if K else (self.DESC_PREFIX, ())

    def check_labels(self, y, batch, device):
        if y is None:
            return None
        K = self.num_classes()
        if not K:
            raise _lib.RgfmError(f"labels on a {type(self._module()).__name__} built without num_classes: the net is unconditional")
        if not isinstance(y, torch.Tensor) or y.dtype.is_floating_point or y.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise _lib.RgfmError(f"labels: an integer tensor [{batch}] expected, got {type(y).__name__}"
                                 f"{' of ' + str(y.dtype) if isinstance(y, torch.Tensor) else ''}")
        if y.dim() != 1 or y.shape[0] != batch:
            raise _lib.RgfmError(f"labels: one label per row ([{batch}]) expected, got {tuple(y.shape)}")
        if batch:
            lo, hi = int(y.min()), int(y.max())
            if lo < 0 or hi > K:
                raise _lib.RgfmError(f"labels must lie in 0..{K} ({K} is the null label), got values in {lo}..{hi}")
        return y.to(device=device, dtype=torch.int32).contiguous()

    def no_labels(self, y, what):
        """The refusal of the entry points that have no labelled form."""
        if y is not None:
            raise _lib.RgfmError(f"{what} has no labelled form; without labels a class-conditional net runs as its "
                                 "unconditional branch (the null label in every row)")

    def _check_eval(self, module):
        if module.training:
            raise _lib.RgfmError(
                f"{type(module).__name__} is in training mode; model(x, t) implements eval-mode semantics only "
                "(Dropout = identity). Train through model.forward_train(x, t) (HIP backward, dropout), or call "
                ".eval() to evaluate / sample.")

    # ---- likelihood: J^T u, divergence, log p(x) -------------------------
    def _check_probes(self, x, eps):
        _require_hip(eps)
        if eps.dim() != 5 or tuple(eps.shape[1:]) != tuple(x.shape) or eps.device != x.device:
            raise _lib.RgfmError(f"probes of shape [K,{','.join(map(str, x.shape))}] on {x.device} expected, got "
                                 f"{tuple(eps.shape)} on {eps.device}")
        return eps.contiguous()

    def linearize(self, x, t):
        """One exact-fp32 forward (no dropout, whatever the module's mode) that keeps its state: an object with `.v`
        = model(x, t) and `.vjp(u)` = J^T u, J = dv/dx, as often as wanted (rgfm_unet_forward_train / rgfm_unet_vjp)."""
        x, t = self._check_xt(x, t)
        return _Linearization(self, x, t)

    def divergence(self, x, t, eps, div_out=None):
        """(v, div): v = model(x, t) on the exact-fp32 forward and div[b] = mean_k <eps_k[b], J^T eps_k[b]> for the probes
        eps [K, B, C, H, W] (rgfm_unet_divergence).  K = 0: a plain forward, div (or the given `div_out`) untouched."""
        x, t = self._check_xt(x, t)
        eps = self._check_probes(x, eps)
        B, K, dev = x.shape[0], eps.shape[0], x.device
        v = torch.empty_like(x)
        div = torch.zeros(B, device=dev) if div_out is None else div_out
        if B == 0:
            return v, div
        L = _lib.lib()
        with torch.cuda.device(dev):
            h = self.handle(dev)
            ws, nb = self.workspace("rgfm_unet_divergence_workspace_bytes", B, dev)
            _lib.check(L.rgfm_unet_divergence(h, _ptr(x), _ptr(t), t.numel(), _ptr(eps), K, _ptr(v), _ptr(div), B,
                                              _ptr(ws), nb, _stream(dev)))
        return v, div

    def log_prob(self, x, eps, num_steps, solver):
        """(logp [B], z [B, C, H, W]) of rgfm_unet_log_prob for data x and probes eps [K, B, C, H, W]; eps None or K = 0:
        the encoder, (None, z)."""
        sid = _lib.solver_id(solver)
        m = self._module()
        _require_hip(x)
        self._check_input(m, x)
        x = x.contiguous()
        B, dev = x.shape[0], x.device
        K = 0 if eps is None else eps.shape[0]
        if K:
            eps = self._check_probes(x, eps)
        z = torch.empty_like(x)
        logp = torch.empty(B, device=dev) if K else None
        if B == 0:
            return logp, z
        L = _lib.lib()
        with torch.cuda.device(dev):
            h = self.handle(dev)
            n = ctypes.c_size_t()
            _lib.check(L.rgfm_unet_log_prob_workspace_bytes(h, B, sid, K, ctypes.byref(n)))
            ws = self._ws.get(n.value, dev)
            _lib.check(L.rgfm_unet_log_prob(h, _ptr(x), _ptr(eps if K else None), K, int(num_steps), sid, _ptr(z),
                                            _ptr(logp), B, _ptr(ws), n.value, _stream(dev)))
        return logp, z

    def dropout_mask(self, block, seed, p, batch, device):
        """Keep decisions (1 / 0) of ResBlock `block` for `batch` rows: [batch, cout, H, W] (rgfm_unet_dropout_mask)."""
        m = self._module()
        S, C = m.resblock_geometry()[block]
        out = torch.empty(batch, C, S, S, device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().rgfm_unet_dropout_mask(self.handle(device), int(block), int(seed), float(p),
                                                         int(batch), _ptr(out)))
        return out

    def _check_input(self, m, x):
        if x.dim() != 4 or x.shape[1] != m.in_channels or x.shape[2] != m.img_size or x.shape[3] != m.img_size:
            raise _lib.RgfmError(f"expected x of shape [B,{m.in_channels},{m.img_size},{m.img_size}], got {tuple(x.shape)}")

    def desc(self):
        m = self._module()
        d = _lib.UNetDesc()
        d.in_channels, d.img_size, d.model_channels = m.in_channels, m.img_size, m.model_channels
        d.num_levels = len(m.channel_mult)
        if d.num_levels > 4:
            raise _lib.RgfmError("at most 4 resolution levels are supported")
        for i, c in enumerate(m.channel_mult):
            d.channel_mult[i] = c
        d.num_res_blocks = m.num_res_blocks
        return d

    # ---- parity hooks -------------------------------------------------
    def time_embedding(self, t):
        """timestep_embedding(t, model_channels) as the device evaluates it (rgfm_unet_time_embedding)."""
        _require_hip(t)
        t = t.reshape(-1).contiguous()
        dev = t.device
        out = torch.empty(t.numel(), self._module().model_channels, device=dev)
        with torch.cuda.device(dev):
            h = self.handle(dev)
            ws, nb = self.workspace("rgfm_unet_workspace_bytes", t.numel(), dev)
            _lib.check(_lib.lib().rgfm_unet_time_embedding(h, _ptr(t), t.numel(), _ptr(out), _ptr(ws), nb, _stream(dev)))
        return out

    def conv_routes(self, device):
        """{route name: conv launches} of the handle's latest walk (rgfm_unet_conv_routes); key "t2": CONV_T2 launches."""
        counts = (ctypes.c_int * (_lib.ROUTE_T2 + 1))()
        _lib.check(_lib.lib().rgfm_unet_conv_routes(self.handle(device), counts, len(counts)))
        return dict(zip(_lib.ROUTES + ("t2",), counts))

    def up_merged(self, device):
        """Convs of the handle's latest walk that ran on the merged-parity-class Upsample kernel (rgfm_unet_up_merged)."""
        n = ctypes.c_int(0)
        _lib.check(_lib.lib().rgfm_unet_up_merged(self.handle(device), ctypes.byref(n)))
        return n.value

    def forward_trace(self, x, t):
        """Forward in trace mode; returns (out, [activation tensors, NCHW])."""
        dev = x.device
        L = _lib.lib()
        with torch.cuda.device(dev):
            h = self.handle(dev)
            _lib.check(L.rgfm_unet_set_trace(h, 1))
            try:
                out = self.forward(x, t)
                ws, _ = self.workspace("rgfm_unet_workspace_bytes", x.shape[0], dev)
                n = ctypes.c_int()
                _lib.check(L.rgfm_unet_num_activations(h, ctypes.byref(n)))
                acts = []
                for i in range(n.value):
                    c, hh, ww = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                    _lib.check(L.rgfm_unet_activation_shape(h, i, ctypes.byref(c), ctypes.byref(hh),
                                                            ctypes.byref(ww)))
                    a = torch.empty(x.shape[0], c.value, hh.value, ww.value, device=dev)
                    _lib.check(L.rgfm_unet_read_activation(h, i, x.shape[0], _ptr(ws), _ptr(a),
                                                           _stream(dev)))
                    acts.append(a)
            finally:
                _lib.check(L.rgfm_unet_set_trace(h, 0))
        return out, acts


class _Linearization:
    """The saved state of one exact-fp32 U-Net forward at (x, t) (UNetEngine.linearize).  It owns its workspace and
    belongs to the parameters of its forward: take a new one after the module's parameters change."""

    def __init__(self, engine, x, t):
        dev = x.device
        self.engine, self.shape, self.B = engine, x.shape, x.shape[0]
        self.v = torch.empty_like(x)
        self.ws, self.nbytes = None, 0
        if self.B == 0:
            return
        L = _lib.lib()
        with torch.cuda.device(dev):
            h = engine.handle(dev)
            n = ctypes.c_size_t()
            _lib.check(L.rgfm_unet_train_workspace_bytes(h, self.B, ctypes.byref(n)))
            self.ws, self.nbytes = torch.empty(n.value, dtype=torch.uint8, device=dev), n.value
            _lib.check(L.rgfm_unet_forward_train(h, _ptr(x), _ptr(t), t.numel(), _ptr(self.v), self.B, 0.0, 0,
                                                 _ptr(self.ws), n.value, _stream(dev)))
        self.handle = h.value

    def vjp(self, u):
        """J^T u [B, C, H, W]: the data-only reverse walk (rgfm_unet_vjp)."""
        _require_hip(u)
        if tuple(u.shape) != tuple(self.shape) or u.device != self.v.device:
            raise _lib.RgfmError(f"u of shape {tuple(self.shape)} on {self.v.device} expected, got {tuple(u.shape)} on {u.device}")
        u = u.contiguous()
        g = torch.empty_like(u)
        if self.B == 0:
            return g
        dev = u.device
        with torch.cuda.device(dev):
            h = self.engine.handle(dev)
            if h.value != self.handle:
                raise _lib.RgfmError("the module was rebuilt since this forward; call linearize again")
            _lib.check(_lib.lib().rgfm_unet_vjp(h, _ptr(u), _ptr(g), self.B, _ptr(self.ws), self.nbytes, _stream(dev)))
        return g


class RatioEngine(_EngineBase):
    PREFIX = "rgfm_ratio"
    TRAIN = _TrainSpec(inputs=2, grads=2, out_shape=lambda x, y: x.shape[:1], dropout=True, batchnorm=True,
                       args=lambda x, y, out, n, training, p, seed, stats: (_ptr(x), _ptr(y), _ptr(out), n, training, p,
                                                                            seed, stats),
                       last=lambda engine, seed, p: engine.pool_geometry())

    def __init__(self, module, kind):
        super().__init__(module)
        self.kind = kind

    def desc(self):
        m = self._module()
        d = _lib.RatioDesc()
        d.kind = _RATIO_KIND[self.kind]
        d.feature_dim, d.hidden_dim = m.feature_dim, m.hidden_dim
        d.loss_type = _LOSS.get(m.loss_type, 0)
        return d

    def _check_eval(self, module):
        if module.training:
            raise _lib.RgfmError(
                f"{type(module).__name__} is in training mode; model(x, y), log_ratio and grad_log_ratio implement "
                "eval-mode semantics only (Dropout = identity, BatchNorm = running statistics). Train through "
                "model.forward_train(x, y) (HIP backward, batch statistics, dropout), or call .eval().")

    def _key_extra(self):
        return self._module().loss_type

    def bind(self, x, y):
        """Select the handle that serves this pair of inputs (one geometry per fixed kind: nothing to select)."""

    # ---- training -----------------------------------------------------
    def image_shapes(self):
        return ((1, 32, 32), (3, 32, 32)) if self.kind == "mnist_svhn" else ((1, 28, 28), (1, 28, 28))

    def pool_geometry(self):
        """Per encoder (x, y), per max-pool in forward order: (channels, output size)."""
        if self.kind == "mnist_svhn":
            return [(32, 16), (64, 8), (128, 4)], [(64, 16), (128, 8), (256, 4), (256, 2)]
        return [(32, 14), (64, 7), (128, 3)], [(32, 14), (64, 7), (128, 3)]

    def _check_shapes(self, x, y, rows=("B", "B"), paired=False):
        """x and y are batches of the bound handle's images (`paired`: of one size); `rows` names their row counts."""
        sx, sy = self.image_shapes()
        if (x.dim() != 4 or y.dim() != 4 or tuple(x.shape[1:]) != sx or tuple(y.shape[1:]) != sy
                or (paired and x.shape[0] != y.shape[0])):
            raise _lib.RgfmError(f"expected x of shape [{rows[0]},{sx[0]},{sx[1]},{sx[2]}] and y of shape "
                                 f"[{rows[1]},{sy[0]},{sy[1]},{sy[2]}], got {tuple(x.shape)} and {tuple(y.shape)}")

    def _check_pair(self, x, y):
        _require_hip(x, y)
        self.bind(x, y)
        self._check_shapes(x, y, paired=True)

    def _checked(self, *tensors):
        """What every eval-mode call starts with; returns the module."""
        m = self._module()
        self._check_eval(m)
        _require_hip(*tensors)
        return m

    def _check_xy(self, x, y, rows=None, paired=True):
        """_checked, equal batch sizes (`paired`), the handle bound, and with `rows` the image shapes."""
        self._checked(x, y)
        if paired and x.shape[0] != y.shape[0]:
            raise _lib.RgfmError("x and y must have the same batch size")
        self.bind(x, y)
        if rows:
            self._check_shapes(x, y, rows)

    def _call(self, dev, ws_fn, ws_args, fn, *args):
        """One native call in exactly the workspace it asks for: the size query `ws_fn`(handle, *ws_args), then
        `fn`(handle, *args, workspace, its size, stream)."""
        L = _lib.lib()
        with torch.cuda.device(dev):
            h = self.handle(dev)
            nb = ctypes.c_size_t()
            _lib.check(getattr(L, ws_fn)(h, *ws_args, ctypes.byref(nb)))
            ws = self._ws.get(nb.value, dev)
            _lib.check(getattr(L, fn)(h, *args, _ptr(ws), nb.value, _stream(dev)))

    def forward_train(self, x, y):
        """scores = model(x, y) in the module's current mode, differentiable w.r.t. x, y and the parameters
        (_TrainFn).  In training mode: batch statistics, dropout, and the BatchNorm buffers are updated."""
        m = self._module()
        self._check_pair(x, y)
        p = m.dropout_p() if m.training else 0.0
        return _TrainFn.apply(self.TRAIN, self, float(p), x, y, *m.parameters())

    def dropout_mask(self, block, seed, p, batch, device):
        """Keep decisions (1 / 0) of Dropout layer `block` of the score MLP: [batch, width] (rgfm_ratio_dropout_mask)."""
        m = self._module()
        width = [l.out_features for l in m.score_net if isinstance(l, torch.nn.Linear)][block]
        out = torch.empty(batch, width, device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().rgfm_ratio_dropout_mask(self.handle(device), int(block), int(seed), float(p),
                                                          int(batch), _ptr(out)))
        return out

    def pool_choices(self):
        """The window elements (0..3, row-major) the max-pools of the latest forward_train chose, per encoder (x, y) a
        list of [B, C, Ho, Wo] tensors (rgfm_ratio_pool_choice).  Valid until that call's backward has run."""
        ws, n, h, geometry = self._saved()
        dev = ws.device
        out = []
        with torch.cuda.device(dev):
            for e, geo in enumerate(geometry):
                out.append([])
                for i, (C, S) in enumerate(geo):
                    t = torch.empty(n, C, S, S, device=dev)
                    _lib.check(_lib.lib().rgfm_ratio_pool_choice(h, _ptr(ws), e, i, n, _ptr(t)))
                    out[-1].append(t)
        return out

    def eval(self, x, y, what):
        self._check_xy(x, y)
        n = x.shape[0]
        x, y = x.contiguous(), y.contiguous()
        out = torch.empty(n, device=x.device, dtype=torch.float32)
        if n:
            self._call(x.device, "rgfm_ratio_workspace_bytes", (n,),
                       "rgfm_ratio_eval", _ptr(x), _ptr(y), _ptr(out), n, _RATIO_OUT[what])
        return out

    def eval_cross(self, x, y, what):
        """[nx, ny]: `what` of every pair (x_i, y_j) (rgfm_ratio_eval_cross): each encoder runs once per image."""
        self._check_xy(x, y, rows=("nx", "ny"), paired=False)
        nx, ny = x.shape[0], y.shape[0]
        x, y = x.contiguous(), y.contiguous()
        out = torch.empty(nx, ny, device=x.device, dtype=torch.float32)
        if nx and ny:
            self._call(x.device, "rgfm_ratio_cross_workspace_bytes", (nx, ny),
                       "rgfm_ratio_eval_cross", _ptr(x), nx, _ptr(y), ny, _ptr(out), _RATIO_OUT[what])
        return out

    def grad_log_ratio(self, x, y):
        """(d log_ratio/dx, d log_ratio/dy, log_ratio): rgfm_ratio_grad_log_ratio (either estimator)."""
        self._check_xy(x, y, rows=("B", "B"))
        n = x.shape[0]
        x, y = x.contiguous(), y.contiguous()
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        lr = torch.empty(n, device=x.device, dtype=torch.float32)
        if n:
            self._call(x.device, "rgfm_ratio_grad_workspace_bytes", (n,),
                       "rgfm_ratio_grad_log_ratio", _ptr(x), _ptr(y), _ptr(gx), _ptr(gy), _ptr(lr), n)
        return gx, gy, lr

    # ---- one side given (conditional sampling) ------------------------
    @staticmethod
    def _given_index(given):
        if given not in ('x', 'y'):
            raise ValueError(f"given must be 'x' or 'y', got {given!r}")
        return 0 if given == 'x' else 1

    def _bind_given(self, given, cond, target_shape):
        """Select the handle for a condition batch and a target of shape (C, S, S); returns (given as 0 / 1, the
        estimator's image shapes as (condition's, target's))."""
        gi = self._given_index(given)
        if cond.dim() != 4:
            raise _lib.RgfmError(f"expected condition images [B,C,S,S], got {tuple(cond.shape)}")
        if target_shape is None:
            target_shape = self._default_target_shape(gi)
        probe = torch.empty(0, *target_shape, device='meta')
        self.bind(*((cond, probe) if gi == 0 else (probe, cond)))
        shapes = self.image_shapes()
        sc, st = shapes[gi], shapes[1 - gi]
        if tuple(cond.shape[1:]) != sc or tuple(target_shape) != st:
            raise _lib.RgfmError(f"given={given!r}: expected the condition of shape [B,{sc[0]},{sc[1]},{sc[2]}] and the target of "
                                 f"shape [B,{st[0]},{st[1]},{st[2]}], got {tuple(cond.shape)} and [B,{','.join(map(str, target_shape))}]")
        return gi, (sc, st)

    def _default_target_shape(self, gi):
        return self.image_shapes()[1 - gi]

    def cond_prepare(self, cond, given, target_shape=None):
        """ctx [B, hidden_dim] = W1[:, given slice] f_given(cond) + b1 (rgfm_ratio_cond_prepare): the condition's encoder
        and its half of the first score Linear, once.  `target_shape` (C, S, S) selects the handle of the flexible kind
        (default: the sizes bound by the latest call); the context itself does not depend on it."""
        m = self._checked(cond)
        gi, _ = self._bind_given(given, cond, target_shape)
        n, dev = cond.shape[0], cond.device
        cond = cond.to(torch.float32).contiguous()
        ctx = torch.empty(n, m.hidden_dim, device=dev, dtype=torch.float32)
        if n:
            self._call(dev, "rgfm_ratio_cond_prepare_workspace_bytes", (gi, n),
                       "rgfm_ratio_cond_prepare", _ptr(cond), gi, n, _ptr(ctx))
        return ctx

    def grad_log_ratio_cond(self, ctx, given, target):
        """(d log_ratio/d target, log_ratio) with row b pairing ctx[b] (cond_prepare) and target[b]
        (rgfm_ratio_grad_log_ratio_cond): only the target's encoder runs."""
        m = self._checked(ctx, target)
        gi = self._given_index(given)
        if target.dim() != 4:
            raise _lib.RgfmError(f"expected target images [B,C,S,S], got {tuple(target.shape)}")
        self._bind_target(gi, target)
        st = self.image_shapes()[1 - gi]
        n = target.shape[0]
        if tuple(target.shape[1:]) != st or tuple(ctx.shape) != (n, m.hidden_dim):
            raise _lib.RgfmError(f"given={given!r}: expected the target of shape [B,{st[0]},{st[1]},{st[2]}] and ctx of shape "
                                 f"[B,{m.hidden_dim}], got {tuple(target.shape)} and {tuple(ctx.shape)}")
        target, ctx = target.contiguous(), ctx.contiguous()
        g = torch.empty_like(target)
        lr = torch.empty(n, device=target.device, dtype=torch.float32)
        if n:
            self._call(target.device, "rgfm_ratio_grad_cond_workspace_bytes", (gi, n),
                       "rgfm_ratio_grad_log_ratio_cond", _ptr(ctx), gi, _ptr(target), _ptr(g), _ptr(lr), n)
        return g, lr

    def _bind_target(self, gi, target):
        """Select the handle that serves a target batch (one geometry per fixed kind: nothing to select)."""


class FlexibleRatioEngine(RatioEngine):
    """RatioEngine of FlexibleRatioEstimator.  The module is size-agnostic, a device handle is not (its rasters, tilings
    and workspaces follow from the image sizes): bind() reads (x_size, y_size) from the inputs of a call and handle()
    serves the handle of the bound pair, keeping one per pair seen -- alternating between sizes re-creates nothing."""
    DESC_PREFIX = "rgfm_ratio_flex"

    def __init__(self, module):
        super().__init__(module, "flexible")
        self._sizes = None
        self._cache = {}  # (x_size, y_size) -> (handle, key, blob) of every pair but the bound one

    def bind(self, x, y):
        m = self._module()
        for name, t, c in (("x", x, m.x_channels), ("y", y, m.y_channels)):
            if t.dim() != 4 or t.shape[1] != c or t.shape[2] != t.shape[3]:
                raise _lib.RgfmError(f"expected {name} of shape [B,{c},S,S] (square images), got {tuple(t.shape)}")
        sizes = (int(x.shape[2]), int(y.shape[2]))
        if sizes != self._sizes:
            if self._sizes is not None and self._handle is not None:
                self._cache[self._sizes] = (self._handle, self._key, self._blob)
            self._handle, self._key, self._blob = self._cache.pop(sizes, (None, None, None))
            self._sizes = sizes
        return sizes

    def _default_target_shape(self, gi):
        if self._sizes is None:
            raise _lib.RgfmError("FlexibleRatioEstimator: pass target_shape (C, S, S); no image sizes are bound yet")
        m = self._module()
        c, sz = ((m.y_channels, self._sizes[1]) if gi == 0 else (m.x_channels, self._sizes[0]))
        return (c, sz, sz)

    def _bind_target(self, gi, target):
        # the context carries no image size: the given side keeps the size bound by cond_prepare
        if self._sizes is None:
            raise _lib.RgfmError("FlexibleRatioEstimator: call cond_prepare first (it binds the condition's image size)")
        m = self._module()
        sg = self._sizes[gi]
        probe = torch.empty(0, m.x_channels if gi == 0 else m.y_channels, sg, sg, device='meta')
        self.bind(*((probe, target) if gi == 0 else (target, probe)))

    def desc(self):
        if self._sizes is None:
            raise _lib.RgfmError("FlexibleRatioEstimator: no image sizes yet (they are read from the inputs of a call)")
        m = self._module()
        d = _lib.RatioFlexDesc()
        d.feature_dim, d.hidden_dim, d.loss_type = m.feature_dim, m.hidden_dim, _LOSS.get(m.loss_type, 0)
        d.x_channels, d.y_channels = m.x_channels, m.y_channels
        d.x_size, d.y_size = self._sizes
        return d

    def owns(self, handle):
        return self._handle is handle or any(h is handle for h, _, _ in self._cache.values())

    def _destroy(self):
        # (called for the bound handle when the module's tensors were replaced: the other sizes' handles are as stale)
        handles = [self._handle] + [h for h, _, _ in self._cache.values()]
        self._cache = {}
        self._handle = None
        for h in handles:
            if h is not None:
                _lib.lib().rgfm_ratio_destroy(h)

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def image_shapes(self):
        m = self._module()
        sx, sy = self._sizes
        return (m.x_channels, sx, sx), (m.y_channels, sy, sy)

    def pool_geometry(self):
        sx, sy = self._sizes
        return tuple([(32, s // 2), (64, s // 4), (128, s // 8)] for s in (sx, sy))


_CLF_KIND = {"mnist28": 0, "mnist32": 1, "svhn": 2}
# kind: (image shape, per conv block (channels, output size, max-pool behind it), fc1 width)
_CLF_GEOMETRY = {
    "mnist28": ((1, 28, 28), [(32, 14, True), (64, 7, True)], 128),
    "mnist32": ((1, 32, 32), [(32, 16, True), (64, 8, True), (64, 8, False)], 128),
    "svhn": ((3, 32, 32), [(32, 16, True), (64, 8, True), (128, 8, False), (128, 8, False)], 256),
}


class ClassifierEngine(_EngineBase):
    """Training pass of the evaluation classifiers (rgfm_clf_*): one handle per module, re-packed in place when
    only the values of its parameters moved."""

    PREFIX = "rgfm_clf"
    TRAIN = _TrainSpec(inputs=1, grads=1, out_shape=lambda x: (x.shape[0], 10), dropout=True, batchnorm=True,
                       args=lambda x, out, n, training, p, seed, stats: (_ptr(x), _ptr(out), n, training, seed, p, stats),
                       last=lambda engine, seed, p: (seed, p))

    def __init__(self, module, kind):
        super().__init__(module)
        self.kind = kind

    def desc(self):
        d = _lib.ClfDesc()
        d.kind = _CLF_KIND[self.kind]
        return d

    def image_shape(self):
        return _CLF_GEOMETRY[self.kind][0]

    def layer_shapes(self):
        """Per layer with a ReLU, in forward order: the shape (without the batch) of its gate -- the conv blocks on
        their output raster, then fc1 -- and whether a max-pool sits behind it."""
        _, blocks, hidden = _CLF_GEOMETRY[self.kind]
        return [((c, s, s), pool) for c, s, pool in blocks] + [((hidden,), False)]

    def forward_train(self, x):
        """logits = model(x) in the module's current mode, differentiable w.r.t. x and the parameters (_TrainFn).
        In training mode: batch statistics, dropout, and the BatchNorm buffers are updated."""
        m = self._module()
        _require_hip(x)
        c, s, _ = self.image_shape()
        if x.dim() != 4 or tuple(x.shape[1:]) != (c, s, s):
            raise _lib.RgfmError(f"expected images of shape [B,{c},{s},{s}], got {tuple(x.shape)}")
        p = m.dropout_p() if m.training else 0.0
        return _TrainFn.apply(self.TRAIN, self, float(p), x, *m.parameters())

    def pool_choices(self):
        """The window elements (0..3, row-major) the max-pools of the latest forward_train chose: per conv block a
        [B, C, Ho, Wo] tensor, or None where no pool follows (rgfm_clf_pool_choice).  Valid until that call's backward."""
        ws, n, h, _ = self._saved()
        out = []
        with torch.cuda.device(ws.device):
            for i, (shape, pool) in enumerate(self.layer_shapes()[:-1]):
                t = torch.empty(n, *shape, device=ws.device) if pool else None
                if pool:
                    _lib.check(_lib.lib().rgfm_clf_pool_choice(h, _ptr(ws), i, n, _ptr(t)))
                out.append(t)
        return out

    def gates(self):
        """1.0 where the ReLU of the latest forward_train passed: per conv block on its output raster (behind a pool:
        the gate of the element taken), then fc1's [B, hidden] before the dropout (rgfm_clf_gate)."""
        ws, n, h, _ = self._saved()
        out = []
        with torch.cuda.device(ws.device):
            for i, (shape, _) in enumerate(self.layer_shapes()):
                t = torch.empty(n, *shape, device=ws.device)
                _lib.check(_lib.lib().rgfm_clf_gate(h, _ptr(ws), i, n, _ptr(t)))
                out.append(t)
        return out

    def last_dropout(self):
        """(seed, p) of the latest forward_train's dropout."""
        if not self._last_train:
            raise _lib.RgfmError("no forward_train call yet")
        return self._last_train[3]

    def dropout_mask(self, seed, p, batch, device):
        """Keep decisions (1 / 0) of the Dropout layer behind fc1: [batch, hidden] (rgfm_clf_dropout_mask)."""
        out = torch.empty(batch, _CLF_GEOMETRY[self.kind][2], device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().rgfm_clf_dropout_mask(self.handle(device), int(seed), float(p), int(batch), _ptr(out)))
        return out


class _XentFn(torch.autograd.Function):
    """Mean softmax cross-entropy through rgfm_clf_xent: the forward computes dlogits = (softmax - onehot) / n with
    the loss rows, the backward scales it by the incoming gradient."""

    @staticmethod
    def forward(ctx, logits, labels):
        _require_hip(logits)
        if logits.dim() != 2 or not 1 <= logits.shape[1] <= 32:
            raise _lib.RgfmError(f"expected logits of shape [B, classes <= 32], got {tuple(logits.shape)}")
        if labels.shape != logits.shape[:1]:
            raise _lib.RgfmError(f"expected {logits.shape[0]} labels, got {tuple(labels.shape)}")
        dev = logits.device
        n, classes = logits.shape
        if n == 0:
            raise _lib.RgfmError("cross_entropy of an empty batch")
        logits = logits.contiguous()
        labels = labels.to(device=dev, dtype=torch.int32).contiguous()
        rows = torch.empty(n, dtype=torch.float64, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev)
        dlogits = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rgfm_clf_xent(_ptr(logits), _ptr(labels), n, classes, 1.0 / n, _ptr(rows), _ptr(dlogits),
                                                _ptr(pred), _stream(dev)))
        ctx.dlogits = dlogits
        ctx.mark_non_differentiable(rows)
        return (rows.sum() / n).to(torch.float32), pred.long(), rows

    @staticmethod
    def backward(ctx, dloss, _dpred, _drows):
        return ctx.dlogits * dloss, None


def cross_entropy(logits, labels):
    """(mean loss, predicted classes [B], per-row losses [B] in fp64) of the fused softmax cross-entropy kernel."""
    return _XentFn.apply(logits, labels)


# ---- sampler entry points ------------------------------------------------

_sampler_ws = _Workspace()


def _solver(solver, *models):
    """RGFM_SOLVER_* of `solver` ('euler' | 'midpoint'; anything else: ValueError before any device work).  The
    midpoint loops exist for U-Net nets only: a FlowMatchingModel net with 'midpoint' raises RgfmError."""
    sid = _lib.solver_id(solver)
    if sid:
        for m in models:
            if not isinstance(m._engine, UNetEngine):
                raise _lib.RgfmError(f"solver={solver!r} needs U-Net velocity nets (FlexibleUNet and its presets); "
                                     f"{type(m).__name__} has the Euler loop only")
    return sid


def _check_strength(gamma_rows, stage_scale, batch, num_steps, steps, sid, models):
    """Argument checks of a call with a strength per row (`gamma_rows`: fp32 device tensor [batch]) and / or a scale per
    stage (`stage_scale`: floats, one per stage of the call), before any device work.  Returns what _run_loop takes as
    `strength`: None when both are None (the call is then today's), else (gamma_rows, ctypes double array or None)."""
    if gamma_rows is None and stage_scale is None:
        return None
    for m in models:
        if not isinstance(m._engine, UNetEngine):
            raise _lib.RgfmError("a guidance strength per sample or per stage needs U-Net velocity nets (FlexibleUNet and "
                                 f"its presets); {type(m).__name__} takes a scalar strength only")
    if gamma_rows is not None:
        if not isinstance(gamma_rows, torch.Tensor) or gamma_rows.dim() != 1 or gamma_rows.shape[0] != batch:
            shape = tuple(gamma_rows.shape) if isinstance(gamma_rows, torch.Tensor) else type(gamma_rows).__name__
            raise ValueError(f"gamma_rows: a 1-D tensor with one strength per row ([{batch}]) expected, got {shape}")
        if gamma_rows.dtype != torch.float32:
            raise ValueError(f"gamma_rows must be float32, got {gamma_rows.dtype}")
    arr = None
    if stage_scale is not None:
        n = (int(steps[1]) - int(steps[0])) * (2 if sid else 1)
        vals = [float(v) for v in stage_scale]
        if len(vals) != n:
            raise ValueError(f"stage_scale holds {len(vals)} values, the call has {n} stages")
        arr = (ctypes.c_double * max(n, 1))(*vals)
        arr.n = n
    return gamma_rows, arr


def draw_sde_seed():
    """The noise seed of a stochastic sampler call that names none: one 62-bit integer from torch's CPU default
    generator (torch.manual_seed fixes it; no device read-back)."""
    return int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item())


def check_sde(sde_eta, solver, models):
    """Argument checks of a stochastic sampler call, before any draw and any device work; returns sde_eta as a float
    (0.0: off).  sde_eta must be finite and >= 0 (ValueError); sde_eta > 0 needs solver='euler' and U-Net velocity nets
    (RgfmError)."""
    eta = float(sde_eta)
    if not (eta >= 0.0 and math.isfinite(eta)):
        raise ValueError(f"sde_eta must be finite and >= 0, got {sde_eta!r}")
    if eta == 0.0:
        return eta
    if _lib.solver_id(solver):
        raise _lib.RgfmError("sde_eta > 0 needs solver='euler': there is no stochastic midpoint rule")
    for m in models:
        if not isinstance(m._engine, UNetEngine):
            raise _lib.RgfmError("stochastic sampling (sde_eta > 0) needs U-Net velocity nets (FlexibleUNet and its "
                                 f"presets); {type(m).__name__} has the deterministic Euler loop only")
    return eta


def _sde(sde_eta, sde_seed, sid, models, *states):
    """The stochastic step of a loop call (include/rgfm.h, "Stochastic sampling"), before any device work: None for
    sde_eta = 0 (the call is then today's), else what _run_loop takes as `sde`.  The checks: check_sde; sde_seed None:
    draw_sde_seed().  `states`: the loop's state tensors."""
    eta = check_sde(sde_eta, 'midpoint' if sid else 'euler', models)
    if eta == 0.0:
        return None
    seed = draw_sde_seed() if sde_seed is None else int(sde_seed) % (1 << 64)
    B = states[0].shape[0]
    dims = [int(t[0].numel()) if B else 0 for t in states] + [0]
    return _lib.Sde(eta, seed), B, dims[0], dims[1]


def check_ess(ess_floor, n_mc, models, cross=False):
    """Argument checks of an effective-sample-size floor (include/rgfm.h, "Effective-sample-size floor"), before any
    draw and any device work; returns the floor as a float, or None for ess_floor=None (the call is then today's).
    The floor must be finite with 1 <= ess_floor <= n_mc (ValueError); it needs U-Net velocity nets and the paired
    (not the cross) pairing (RgfmError)."""
    if ess_floor is None:
        return None
    floor = float(ess_floor)
    if not math.isfinite(floor) or floor < 1.0:
        raise ValueError(f"ess_floor must be finite and >= 1 (an effective sample size), got {ess_floor!r}")
    if floor > n_mc:
        raise ValueError(f"ess_floor {floor:g} is above the {n_mc} MC samples: no exponent can reach it")
    if cross:
        raise _lib.RgfmError("ess_floor does not go with mc_pairing='cross': an exponent per row makes the ratio matrix "
                             "row-dependent, and the two [B,N] x [N,N] products of the cross weights no longer exist")
    for m in models:
        if not isinstance(m._engine, UNetEngine):
            raise _lib.RgfmError("ess_floor needs U-Net velocity nets (FlexibleUNet and its presets); "
                                 f"{type(m).__name__}'s loop has the plain importance weights only")
    return floor


def _ess(ess_floor, n_mc, models, cross, tau, n_stages, batch):
    """The floor of a loop call, before any device work: None for ess_floor=None, else what _run_loop takes as `ess` --
    the rgfm_ess record and the tensor it points into.  `tau`: a zeroed fp32 device tensor [n_stages, batch], or None."""
    floor = check_ess(ess_floor, n_mc, models, cross)
    if floor is None:
        return None
    if tau is not None and not (tau.is_cuda and tau.dtype == torch.float32 and tau.is_contiguous()
                                and tuple(tau.shape) == (n_stages, batch)):
        raise _lib.RgfmError(f"tau: a contiguous fp32 device tensor [{n_stages}, {batch}] expected, got "
                             f"{tuple(tau.shape)} {tau.dtype} on {tau.device}")
    return _lib.Ess(floor, _ptr(tau), 0 if tau is None else tau.numel()), tau


def _run_loop(loop, ws_args, args, steps, sid, dev, ws=None, diag=None, cross=False, strength=None, sde=None, ess=None):
    """One native sampler loop (`loop`: its _Loop row): the size query (*ws_args[, sid]), the workspace (`ws`: a
    _Workspace; default the samplers' shared one), then the entry point (*args, *steps[, sid], workspace, stream).
    `steps`: (step_begin, step_end).  sid None: entry points without a solver argument (the FlowMatchingModel loops).
    `diag`: a records tensor [n_stages, B, RGFM_DIAG_FLOATS] -- the loop's *_diag pair runs and fills it (guided loops
    only).  `cross`: the U-Net pair loop over all pairs of the MC set (one entry point with and without records).
    `strength`: what _check_strength returns -- not None: the loop's *_gs entry point runs (U-Net loops), the *_diag
    arguments with (gamma_rows, stage_scale, n_stage_scale) behind gamma, in the workspace chosen above.
    `sde`: what _sde returns -- not None: the loop's *_sde entry point runs (the *_gs arguments, or the single loop's own,
    with the rgfm_sde in front of the workspace), in the workspace chosen above plus rgfm_sde_scratch_bytes.
    `ess`: what _ess returns -- not None: the loop's *_ess entry point runs (the *_sde arguments with the rgfm_ess behind
    the rgfm_sde, which is null without `sde`), in the workspace chosen above."""
    L = _lib.lib()
    tail = () if sid is None else (sid,)
    fn, ws_fn, sink = loop.fn, loop.ws, ()
    if diag is not None:
        if not (diag.is_cuda and diag.dtype == torch.float32 and diag.is_contiguous() and diag.dim() == 3
                and diag.shape[2] == _lib.DIAG_FLOATS):
            raise _lib.RgfmError(f"diagnostics records: a contiguous fp32 device tensor [n_stages, B, {_lib.DIAG_FLOATS}] "
                                 f"expected, got {tuple(diag.shape)} {diag.dtype} on {diag.device}")
        fn, ws_fn = loop.diag, loop.diag_ws
        sink = (_ptr(diag), diag.shape[0] * diag.shape[1])
    if cross:
        fn, ws_fn = loop.cross, loop.cross_ws
    if strength is not None:
        rows, scale = strength
        if rows is not None and not (rows.is_cuda and rows.is_contiguous() and rows.device == dev):
            raise _lib.RgfmError(f"gamma_rows must be a contiguous tensor on {dev}, got one on {rows.device}")
        fn = loop.cross_gs if cross else loop.gs
        args = (*args, _ptr(rows), scale, scale.n if scale is not None else 0)
    if cross or strength is not None:  # (these entry points always take the sink's two arguments)
        sink = sink or (None, 0)
    nb, more = ctypes.c_size_t(), ()
    _lib.check(getattr(L, ws_fn)(*ws_args, *tail, ctypes.byref(nb)))
    nbytes = nb.value
    if sde is not None:
        rec, batch, dim_x, dim_y = sde
        fn = loop.cross_sde if cross else loop.sde
        if fn is None:
            raise _lib.RgfmError("this sampler loop has no stochastic step")
        if loop.gs is not None:  # (the guided loops: the *_gs arguments)
            if strength is None:
                args = (*args, None, None, 0)
            sink = sink or (None, 0)
        _lib.check(L.rgfm_sde_scratch_bytes(batch, dim_x, dim_y, ctypes.byref(nb)))
        nbytes, more = nbytes + nb.value, (ctypes.byref(rec),)
    if ess is not None:
        if loop.ess is None or cross:
            raise _lib.RgfmError("this sampler loop has no effective-sample-size floor")
        fn = loop.ess
        if sde is None:
            if strength is None:
                args = (*args, None, None, 0)
            sink, more = sink or (None, 0), (None,)
        more = (*more, ctypes.byref(ess[0]))
    buf = (ws or _sampler_ws).get(nbytes, dev)
    _lib.check(getattr(L, fn)(*args, int(steps[0]), int(steps[1]), *tail, *sink, *more, _ptr(buf), nbytes, _stream(dev)))


def _solver_arg(engine, sid):
    return sid if isinstance(engine, UNetEngine) else None


TABLE_ROWS = 4096  # (stage, class) rows of a labelled sampler call's time table (csrc/sampler_host.h)


def check_cfg(labels, cfg_scale, batch, model, device=None):
    """Argument checks of a labelled sampler call for one net, before any draw and any device work.  Returns None when
    the call has neither labels nor a scale other than 1 (it is then today's), else (labels as int32 [batch] on
    `device`, cfg_scale as a float).  A scale other than 1 needs labels: without them v_c and v_u are the same."""
    w = float(cfg_scale)
    if not math.isfinite(w):
        raise ValueError(f"cfg_scale must be finite, got {cfg_scale!r}")
    if labels is None:
        if w != 1.0:
            raise _lib.RgfmError("cfg_scale needs labels: without them the net's conditional and unconditional "
                                 "velocities are the same")
        return None
    return model._engine.check_labels(labels, batch, device), w


def _cfg_chunks(nets, sid, step_begin, step_end):
    """The step ranges a labelled call is split into so that stages x (K + 1) of every labelled net fits TABLE_ROWS.
    Split calls reproduce one call bit for bit."""
    K = max(m._engine.num_classes() for m in nets)
    cap = max(1, TABLE_ROWS // ((K + 1) * (2 if sid else 1)))
    return [(b, min(b + cap, step_end)) for b in range(step_begin, step_end, cap)] or [(step_begin, step_end)]


def sample_single(model, x, num_steps, step_begin=0, step_end=None, solver='euler', sde_eta=0.0, sde_seed=None,
                  labels=None, cfg_scale=1.0):
    """In-place unguided integration of `x` (rgfm_sample_single; solver='midpoint': rgfm_sample_single_ode).
    `sde_eta` > 0: Euler-Maruyama steps of that strength (rgfm_sample_single_sde; U-Net nets, solver='euler'), the
    noise seeded by `sde_seed` (None: draw_sde_seed()); 0: the call above, unchanged.  The loops below take the two the
    same way.
    `labels` (an integer tensor [B], values 0..K of a net built with num_classes=K) and `cfg_scale` = w: every stage
    advances by v_u + w (v_c - v_u) (rgfm_sample_single_cfg); neither: the call above, unchanged."""
    cfg = check_cfg(labels, cfg_scale, x.shape[0], model, x.device)
    sde = _sde(sde_eta, sde_seed, _solver(solver, model), (model,), x)
    if cfg is not None:
        if x.is_cuda and x.shape[0]:
            return _range_guarded(x.device, [x], lambda: _sample_single_cfg(model, x, num_steps, step_begin, step_end, solver,
                                                                            sde, cfg), [model._engine])
        return _sample_single_cfg(model, x, num_steps, step_begin, step_end, solver, sde, cfg)
    if x.is_cuda and x.shape[0]:
        return _range_guarded(x.device, [x], lambda: _sample_single(model, x, num_steps, step_begin, step_end, solver, sde),
                              [model._engine])
    return _sample_single(model, x, num_steps, step_begin, step_end, solver, sde)


def _sample_single(model, x, num_steps, step_begin=0, step_end=None, solver='euler', sde=None):
    sid = _solver(solver, model)
    eng = model._engine
    eng._check_eval(model)
    _require_hip(x)
    if not x.is_contiguous():
        raise _lib.RgfmError("x must be contiguous (it is updated in place)")
    if step_end is None:
        step_end = num_steps
    B, dev = x.shape[0], x.device
    if B == 0:
        return x
    with torch.cuda.device(dev):
        h = eng.handle(dev)
        _run_loop(eng.SINGLE, (h, B), (h, _ptr(x), B, int(num_steps)), (step_begin, step_end),
                  _solver_arg(eng, sid), dev, ws=eng._ws, sde=sde)
    return x


def _sample_single_cfg(model, x, num_steps, step_begin, step_end, solver, sde, cfg):
    """The labelled single loop: rgfm_sample_single_cfg over the chunks of _cfg_chunks, in the engine's workspace."""
    sid = _solver(solver, model)
    eng = model._engine
    eng._check_eval(model)
    _require_hip(x)
    if not x.is_contiguous():
        raise _lib.RgfmError("x must be contiguous (it is updated in place)")
    if step_end is None:
        step_end = num_steps
    B, dev = x.shape[0], x.device
    if B == 0:
        return x
    labels, w = cfg
    L = _lib.lib()
    with torch.cuda.device(dev):
        h = eng.handle(dev)
        nb = ctypes.c_size_t()
        _lib.check(L.rgfm_sample_single_cfg_workspace_bytes(h, B, sid, ctypes.byref(nb)))
        nbytes, rec = nb.value, None
        if sde is not None:
            rec, batch, dim_x, dim_y = sde
            _lib.check(L.rgfm_sde_scratch_bytes(batch, dim_x, dim_y, ctypes.byref(nb)))
            nbytes += nb.value
        buf = eng._ws.get(nbytes, dev)
        for b, e in _cfg_chunks((model,), sid, int(step_begin), int(step_end)):
            _lib.check(L.rgfm_sample_single_cfg(h, _ptr(x), _ptr(labels), w, B, int(num_steps), b, e, sid,
                                                ctypes.byref(rec) if rec is not None else None, _ptr(buf), nbytes,
                                                _stream(dev)))
    return x


def sample_two_cfg(fm_x, x, fm_y, y, num_steps, solver='euler', labels_x=None, labels_y=None, cfg_scale_x=1.0, cfg_scale_y=1.0):
    """Two independent labelled integrations at once, in place (rgfm_sample_two_cfg: rgfm_sample_two with labels and a
    scale per net): the unguided pair of two class-conditional nets.  Either net may go without labels."""
    cx = check_cfg(labels_x, cfg_scale_x, x.shape[0], fm_x, x.device) or (None, 1.0)
    cy = check_cfg(labels_y, cfg_scale_y, y.shape[0], fm_y, y.device) or (None, 1.0)
    sid = _solver(solver, fm_x, fm_y)
    for m in (fm_x, fm_y):
        if not isinstance(m._engine, UNetEngine):
            raise _lib.RgfmError(f"labelled sampling needs U-Net velocity nets; {type(m).__name__} has no class labels")
        m._engine._check_eval(m)
    _require_hip(x, y)
    if not (x.is_contiguous() and y.is_contiguous()):
        raise _lib.RgfmError("x and y must be contiguous (they are updated in place)")
    if x.data_ptr() == y.data_ptr() or fm_x._engine is fm_y._engine:
        raise _lib.RgfmError("the labelled pair needs two nets and two state tensors")
    dev = x.device
    if x.shape[0] == 0 or y.shape[0] == 0:
        return x, y
    L = _lib.lib()

    def run():
        with torch.cuda.device(dev):
            hx, hy = fm_x._engine.handle(dev), fm_y._engine.handle(dev)
            nb = ctypes.c_size_t()
            _lib.check(L.rgfm_sample_two_cfg_workspace_bytes(hx, hy, x.shape[0], y.shape[0], sid, ctypes.byref(nb)))
            buf = _sampler_ws.get(nb.value, dev)
            for b, e in _cfg_chunks((fm_x, fm_y), sid, 0, int(num_steps)):
                _lib.check(L.rgfm_sample_two_cfg(hx, hy, _ptr(x), _ptr(y), _ptr(cx[0]), _ptr(cy[0]), cx[1], cy[1], x.shape[0],
                                                 y.shape[0], int(num_steps), b, e, sid, _ptr(buf), nb.value, _stream(dev)))
        return x, y
    return _range_guarded(dev, [x, y], run, [fm_x._engine, fm_y._engine])


_side_streams = {}


def _sample_two(fm_x, x, fm_y, y, num_steps, solver):
    sid = _solver(solver, fm_x, fm_y)
    for m in (fm_x, fm_y):
        m._engine._check_eval(m)
    _require_hip(x, y)
    if not (x.is_contiguous() and y.is_contiguous()):
        raise _lib.RgfmError("x and y must be contiguous (they are updated in place)")
    dev = x.device
    with torch.cuda.device(dev):
        hx, hy = fm_x._engine.handle(dev), fm_y._engine.handle(dev)
        _run_loop(_TWO, (hx, hy, x.shape[0], y.shape[0]),
                  (hx, hy, _ptr(x), _ptr(y), x.shape[0], y.shape[0], int(num_steps)), (0, num_steps), sid, dev)
    return x, y


def sample_two_streams(fm_x, x, fm_y, y, num_steps, solver='euler'):
    """Two independent unguided integrations (the MC pre-phase) on two HIP streams.

    Same arithmetic as two sample_single calls; the second net runs on a side stream that
    forks from / joins back into the current stream, so callers keep stream-ordered semantics.
    """
    dev = x.device
    _solver(solver, fm_x, fm_y)

    def run():
        # two U-Nets: one native call that schedules both chains (rgfm_sample_two; RGFM_OVERLAP, RGFM_PREPHASE_PRIO)
        if isinstance(fm_x._engine, UNetEngine) and isinstance(fm_y._engine, UNetEngine) and x.is_cuda and y.is_cuda \
                and x.shape[0] and y.shape[0] and x.data_ptr() != y.data_ptr():
            return _sample_two(fm_x, x, fm_y, y, num_steps, solver)
        # one module passed for both modalities (legal in the reference) has ONE engine workspace:
        # its two integrations must not run concurrently
        if os.environ.get("RGFM_OVERLAP", "1") == "0" or fm_x._engine is fm_y._engine:
            _sample_single(fm_x, x, num_steps, solver=solver)
            _sample_single(fm_y, y, num_steps, solver=solver)
            return x, y
        cur = torch.cuda.current_stream(dev)
        side = _side_streams.get(dev)
        if side is None:
            side = _side_streams[dev] = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            _sample_single(fm_y, y, num_steps, solver=solver)
        _sample_single(fm_x, x, num_steps, solver=solver)
        cur.wait_stream(side)
        return x, y
    if x.is_cuda and y.is_cuda:
        return _range_guarded(dev, [x, y], run, [fm_x._engine, fm_y._engine])
    return run()


def sample_pair(fm_x, fm_y, x, y, mc_x1, mc_y1, mc_ratios, num_steps, gamma, step_begin=0,
                step_end=None, solver='euler', diag=None, gamma_rows=None, stage_scale=None, sde_eta=0.0, sde_seed=None,
                ess_floor=None, tau=None):
    """In-place paired loop with optional MC guidance (rgfm_sample_pair; solver='midpoint': rgfm_sample_pair_ode).
    `diag`: a records tensor [n_stages, B, 8] to fill (rgfm_sample_pair_diag / rgfm_fmnet_sample_pair_diag; the state
    keeps its bits); the other guided loops below take it the same way.

    `mc_ratios` [N]: the ratios of the N pairs (mc_x1[i], mc_y1[i]).  `mc_ratios` [N, N] (x index first, what
    RatioEngine.eval_cross returns): cross pairing, the guidance over all N x N pairs (mc_x1[i], mc_y1[j])
    (rgfm_sample_pair_cross; U-Net nets, N <= 1024).

    `gamma_rows` (fp32 device tensor [B]: a strength per row, in `gamma`'s place) and `stage_scale` (floats, one per
    stage of the call: a scale of the strength per stage; 0 = the stage runs unguided): rgfm_sample_pair_gs /
    rgfm_sample_pair_cross_gs (U-Net nets).  Both None: the call above, unchanged.  The other guided loops below take
    them the same way.

    `ess_floor` (a float in [1, N]): every guided stage tempers the rows whose effective sample size is below it
    (rgfm_sample_pair_ess); `tau`: a zeroed fp32 device tensor [n_stages, B] that receives the rows' exponents.  None:
    the call above, unchanged.  sample_cond takes them the same way."""
    sid = _solver(solver, fm_x, fm_y)
    strength = _check_strength(gamma_rows, stage_scale, x.shape[0], num_steps,
                               (step_begin, num_steps if step_end is None else step_end), sid, (fm_x, fm_y))
    sde = _sde(sde_eta, sde_seed, sid, (fm_x, fm_y), x, y)
    for m in (fm_x, fm_y):
        m._engine._check_eval(m)
    ex = fm_x._engine
    if type(ex) is not type(fm_y._engine):
        raise _lib.RgfmError("paired sampling needs two velocity nets of the same family "
                             f"(got {type(fm_x).__name__} and {type(fm_y).__name__})")
    _require_hip(x, y, mc_x1, mc_y1, mc_ratios)
    if not (x.is_contiguous() and y.is_contiguous()):
        raise _lib.RgfmError("x and y must be contiguous (they are updated in place)")
    if step_end is None:
        step_end = num_steps
    B, dev = x.shape[0], x.device
    if B == 0:
        return x, y
    n_mc = 0 if mc_x1 is None else mc_x1.shape[0]
    cross = bool(n_mc) and mc_ratios.dim() == 2
    if cross:
        _check_cross(mc_ratios.shape, n_mc, mc_y1.shape[0], fm_x, fm_y)
    ess = _ess(ess_floor, n_mc, (fm_x, fm_y), cross, tau, (step_end - step_begin) * (2 if sid else 1), B)
    if n_mc:
        mc_x1, mc_y1, mc_ratios = mc_x1.contiguous(), mc_y1.contiguous(), mc_ratios.contiguous()

    def run():
        with torch.cuda.device(dev):
            hx, hy = fm_x._engine.handle(dev), fm_y._engine.handle(dev)
            _run_loop(ex.PAIR, (hx, hy, B, n_mc),
                      (hx, hy, _ptr(x), _ptr(y), _ptr(mc_x1 if n_mc else None), _ptr(mc_y1 if n_mc else None),
                       _ptr(mc_ratios if n_mc else None), n_mc, B, int(num_steps), float(gamma)),
                      (step_begin, step_end), _solver_arg(ex, sid), dev, diag=diag, cross=cross, strength=strength,
                      sde=sde, ess=ess)
        return x, y
    return _range_guarded(dev, [x, y], run, [fm_x._engine, fm_y._engine])


def sample_pair_grad(fm_x, fm_y, ratio_estimator, x, y, num_steps, gamma, step_begin=0, step_end=None, solver='euler',
                     diag=None, gamma_rows=None, stage_scale=None, sde_eta=0.0, sde_seed=None):
    """In-place paired loop with gradient log-ratio guidance (rgfm_sample_pair_grad; solver='midpoint':
    rgfm_sample_pair_grad_ode)."""
    sid = _lib.solver_id(solver)
    strength = _check_strength(gamma_rows, stage_scale, x.shape[0], num_steps,
                               (step_begin, num_steps if step_end is None else step_end), sid, (fm_x, fm_y))
    for m in (fm_x, fm_y, ratio_estimator):
        m._engine._check_eval(m)
    if not (isinstance(fm_x._engine, UNetEngine) and isinstance(fm_y._engine, UNetEngine)):
        raise _lib.RgfmError("gradient log-ratio guidance needs two U-Net velocity nets")
    sde = _sde(sde_eta, sde_seed, sid, (fm_x, fm_y), x, y)
    _require_hip(x, y)
    ratio_estimator._engine.bind(x, y)
    if not (x.is_contiguous() and y.is_contiguous()):
        raise _lib.RgfmError("x and y must be contiguous (they are updated in place)")
    if step_end is None:
        step_end = num_steps
    B, dev = x.shape[0], x.device
    if B == 0:
        return x, y

    def run():
        with torch.cuda.device(dev):
            hx, hy, hr = fm_x._engine.handle(dev), fm_y._engine.handle(dev), ratio_estimator._engine.handle(dev)
            _run_loop(_PAIR_GRAD, (hx, hy, hr, B),
                      (hx, hy, hr, _ptr(x), _ptr(y), B, int(num_steps), float(gamma)), (step_begin, step_end), sid, dev,
                      diag=diag, strength=strength, sde=sde)
        return x, y
    return _range_guarded(dev, [x, y], run, [fm_x._engine, fm_y._engine])


def _block_gamma(gamma, batch, dev, name):
    """(entry point, its gamma argument) of a guidance block: a number is the scalar block `name`; an fp32 device tensor
    [batch] -- a strength per row -- its *_rows twin."""
    if not isinstance(gamma, torch.Tensor):
        return name, float(gamma)
    if gamma.dim() != 1 or gamma.shape[0] != batch or gamma.dtype != torch.float32:
        raise ValueError(f"gamma: a number or a float32 tensor [{batch}] (a strength per row) expected, got "
                         f"{tuple(gamma.shape)} {gamma.dtype}")
    if not (gamma.is_cuda and gamma.device == dev and gamma.is_contiguous()):
        raise _lib.RgfmError(f"gamma must be a contiguous tensor on {dev}")
    return name + "_rows", _ptr(gamma)


def _block(dev, ws_fn, ws_args, fn, *args):
    """One guidance-block call: the size query `ws_fn`(*ws_args), a buffer of the samplers' workspace, then
    `fn`(*args, workspace, stream).  A tensor among `args` is an input: it is passed contiguous.  What the block writes
    comes as the pointer of the caller's own tensor."""
    L = _lib.lib()
    with torch.cuda.device(dev):
        nb = ctypes.c_size_t()
        _lib.check(getattr(L, ws_fn)(*ws_args, ctypes.byref(nb)))
        ws = _sampler_ws.get(nb.value, dev)
        args = [_ptr(a.contiguous()) if isinstance(a, torch.Tensor) else a for a in args]
        _lib.check(getattr(L, fn)(*args, _ptr(ws), nb.value, _stream(dev)))


def guidance_apply(x, y, vx, vy, mc_x1, mc_y1, mc_ratios, t, gamma, want_weights=False):
    """One guidance evaluation (parity hook): overwrites vx, vy; returns weights or None.  `gamma`: a number, or an
    fp32 device tensor [B] with a strength per row (rgfm_guidance_apply_rows); the other blocks take it the same way."""
    _require_hip(x, y, vx, vy, mc_x1, mc_y1, mc_ratios)
    B, N, dev = x.shape[0], mc_x1.shape[0], x.device
    dx, dy = x[0].numel(), y[0].numel()
    w = torch.empty(B, N, device=dev) if want_weights else None
    fn, g = _block_gamma(gamma, B, dev, "rgfm_guidance_apply")
    _block(dev, "rgfm_guidance_workspace_bytes", (B, N), fn, x, y, _ptr(vx), _ptr(vy), mc_x1, mc_y1, mc_ratios, B, N, dx, dy,
           float(t), g, _ptr(w))
    return w


CROSS_MAX_N = 1024  # GUID_CROSS_MAX_N of csrc/rgfm_host.h


def _check_cross(shape, n_x, n_y, *models):
    """Argument checks of a cross-pairing call, before any device work."""
    for m in models:
        if not isinstance(m._engine, UNetEngine):
            raise _lib.RgfmError("cross pairing (a ratio matrix over all pairs of the MC set) needs U-Net velocity nets "
                                 f"(FlexibleUNet and its presets); {type(m).__name__} has the paired loop only")
    if n_x != n_y or tuple(shape) != (n_x, n_x):
        raise _lib.RgfmError(f"cross pairing needs equal MC counts and a ratio matrix [N, N] (x index first); got "
                             f"{n_x} x samples, {n_y} y samples and ratios of shape {tuple(shape)}")
    if not 1 <= n_x <= CROSS_MAX_N:
        raise _lib.RgfmError(f"cross pairing takes 1 <= N <= {CROSS_MAX_N} MC samples per modality, got {n_x}")


def guidance_apply_cross(x, y, vx, vy, mc_x1, mc_y1, ratio_matrix, t, gamma, want_weights=False):
    """One guidance evaluation over all N x N pairs of the MC set (rgfm_guidance_apply_cross; parity hook): overwrites
    vx, vy; returns the marginal weights (wx [B, N], wy [B, N]) or None.  ratio_matrix [N, N]: r(mc_x1[i], mc_y1[j])."""
    _require_hip(x, y, vx, vy, mc_x1, mc_y1, ratio_matrix)
    B, N, dev = x.shape[0], mc_x1.shape[0], x.device
    _check_cross(ratio_matrix.shape, N, mc_y1.shape[0])
    dx, dy = x[0].numel(), y[0].numel()
    wx, wy = (torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)) if want_weights else (None, None)
    fn, g = _block_gamma(gamma, B, dev, "rgfm_guidance_apply_cross")
    _block(dev, "rgfm_guidance_cross_workspace_bytes", (B, N, dx, dy), fn, x, y, _ptr(vx), _ptr(vy), mc_x1, mc_y1,
           ratio_matrix, B, N, dx, dy, float(t), g, _ptr(wx), _ptr(wy))
    return (wx, wy) if want_weights else None


def guidance_diag_cross(x, y, vx, vy, mc_x1, mc_y1, ratio_matrix, t):
    """Diagnostics of one evaluation of the cross-pairing block (rgfm_guidance_diag_cross): records [B, 8] -- the joint
    ESS (1 .. N^2), the range over the 2N marginal weights, Z_bar, the four norms; nothing else is written."""
    _require_hip(x, y, vx, vy, mc_x1, mc_y1, ratio_matrix)
    B, N, dev = x.shape[0], mc_x1.shape[0], x.device
    _check_cross(ratio_matrix.shape, N, mc_y1.shape[0])
    dx, dy = x[0].numel(), y[0].numel()
    out = torch.empty(B, _lib.DIAG_FLOATS, device=dev)
    _block(dev, "rgfm_guidance_cross_workspace_bytes", (B, N, dx, dy), "rgfm_guidance_diag_cross", x, y, vx, vy, mc_x1,
           mc_y1, ratio_matrix, B, N, dx, dy, float(t), _ptr(out))
    return out


def guidance_diag(x, y, vx, vy, mc_x1, mc_y1, mc_ratios, t):
    """Diagnostics of one evaluation of the paired guidance block (rgfm_guidance_diag): records [B, 8]
    (utils.diagnostics.FIELDS); nothing else is written."""
    _require_hip(x, y, vx, vy, mc_x1, mc_y1, mc_ratios)
    B, N, dev = x.shape[0], mc_x1.shape[0], x.device
    dx, dy = x[0].numel(), y[0].numel()
    out = torch.empty(B, _lib.DIAG_FLOATS, device=dev)
    _block(dev, "rgfm_guidance_diag_workspace_bytes", (B, N, dx, dy), "rgfm_guidance_diag", x, y, vx, vy, mc_x1, mc_y1,
           mc_ratios, B, N, dx, dy, float(t), _ptr(out))
    return out


def guidance_diag_cond(s, v, mc_set, ratios, t):
    """Diagnostics of one evaluation of the one-sided guidance block (rgfm_guidance_diag_cond): records [B, 8], the _y
    fields 0."""
    _require_hip(s, v, mc_set, ratios)
    B, N, dev = s.shape[0], mc_set.shape[0], s.device
    out = torch.empty(B, _lib.DIAG_FLOATS, device=dev)
    _block(dev, "rgfm_guidance_diag_workspace_bytes", (B, N, s[0].numel(), 0), "rgfm_guidance_diag_cond", s, v, mc_set,
           ratios, B, N, s[0].numel(), float(t), _ptr(out))
    return out


def sample_cond(model, s, mc_set, ratios, num_steps, gamma, step_begin=0, step_end=None, solver='euler', diag=None,
                gamma_rows=None, stage_scale=None, sde_eta=0.0, sde_seed=None, ess_floor=None, tau=None):
    """In-place loop of one U-Net with one-sided MC guidance (rgfm_sample_cond; solver='midpoint':
    rgfm_sample_cond_ode): s [B, C, H, W], mc_set [N, C, H, W], ratios [B, N]."""
    sid = _lib.solver_id(solver)
    strength = _check_strength(gamma_rows, stage_scale, s.shape[0], num_steps,
                               (step_begin, num_steps if step_end is None else step_end), sid, (model,))
    eng = model._engine
    eng._check_eval(model)
    if not isinstance(eng, UNetEngine):
        raise _lib.RgfmError(f"conditional sampling needs a U-Net target (FlexibleUNet and its presets), got "
                             f"{type(model).__name__}")
    sde = _sde(sde_eta, sde_seed, sid, (model,), s)
    _require_hip(s, mc_set, ratios)
    if not s.is_contiguous():
        raise _lib.RgfmError("s must be contiguous (it is updated in place)")
    eng._check_input(model, s)
    eng._check_input(model, mc_set)
    B, N, dev = s.shape[0], mc_set.shape[0], s.device
    if tuple(ratios.shape) != (B, N):
        raise _lib.RgfmError(f"expected ratios of shape [{B},{N}] (a row per sample), got {tuple(ratios.shape)}")
    if step_end is None:
        step_end = num_steps
    if B == 0:
        return s
    ess = _ess(ess_floor, N, (model,), False, tau, (step_end - step_begin) * (2 if sid else 1), B)
    mc_set, ratios = mc_set.contiguous(), ratios.contiguous()

    def run():
        with torch.cuda.device(dev):
            h = eng.handle(dev)
            _run_loop(_COND, (h, B, N),
                      (h, _ptr(s), _ptr(mc_set), _ptr(ratios), N, B, int(num_steps), float(gamma)),
                      (step_begin, step_end), sid, dev, diag=diag, strength=strength, sde=sde, ess=ess)
        return s
    return _range_guarded(dev, [s], run, [eng])


def sample_cond_grad(model, ratio_estimator, s, ctx, given, num_steps, gamma, step_begin=0, step_end=None, solver='euler',
                     diag=None, gamma_rows=None, stage_scale=None, sde_eta=0.0, sde_seed=None):
    """In-place loop of one U-Net with one-sided gradient log-ratio guidance (rgfm_sample_cond_grad; solver='midpoint':
    rgfm_sample_cond_grad_ode): s [B, C, H, W], ctx [B, hidden_dim] from ratio_estimator._engine.cond_prepare(condition,
    given)."""
    sid = _lib.solver_id(solver)
    strength = _check_strength(gamma_rows, stage_scale, s.shape[0], num_steps,
                               (step_begin, num_steps if step_end is None else step_end), sid, (model,))
    eng, re = model._engine, ratio_estimator._engine
    eng._check_eval(model)
    re._check_eval(ratio_estimator)
    if not isinstance(eng, UNetEngine):
        raise _lib.RgfmError(f"conditional sampling needs a U-Net target (FlexibleUNet and its presets), got "
                             f"{type(model).__name__}")
    if given not in ('x', 'y'):
        raise ValueError(f"given must be 'x' or 'y', got {given!r}")
    gi = 0 if given == 'x' else 1
    sde = _sde(sde_eta, sde_seed, sid, (model,), s)
    _require_hip(s, ctx)
    if not s.is_contiguous():
        raise _lib.RgfmError("s must be contiguous (it is updated in place)")
    eng._check_input(model, s)
    re._bind_target(gi, s)
    B, dev = s.shape[0], s.device
    if tuple(ctx.shape) != (B, ratio_estimator.hidden_dim):
        raise _lib.RgfmError(f"expected ctx of shape [{B},{ratio_estimator.hidden_dim}] (a row per sample), got {tuple(ctx.shape)}")
    if step_end is None:
        step_end = num_steps
    if B == 0:
        return s
    ctx = ctx.contiguous()

    def run():
        with torch.cuda.device(dev):
            h, hr = eng.handle(dev), re.handle(dev)
            _run_loop(_COND_GRAD, (h, hr, gi, B),
                      (h, hr, _ptr(s), _ptr(ctx), gi, B, int(num_steps), float(gamma)), (step_begin, step_end), sid, dev,
                      diag=diag, strength=strength, sde=sde)
        return s
    return _range_guarded(dev, [s], run, [eng])


def guidance_apply_cond(s, v, mc_set, ratios, t, gamma, want_weights=False):
    """One evaluation of the one-sided guidance block (parity hook): overwrites v; returns weights or None."""
    _require_hip(s, v, mc_set, ratios)
    B, N, dev = s.shape[0], mc_set.shape[0], s.device
    w = torch.empty(B, N, device=dev) if want_weights else None
    fn, g = _block_gamma(gamma, B, dev, "rgfm_guidance_apply_cond")
    _block(dev, "rgfm_guidance_workspace_bytes", (B, N), fn, s, _ptr(v), mc_set, ratios, B, N, s[0].numel(),
           float(t), g, _ptr(w))
    return w


def profile(enable=None, reset=False, reserve=None):
    L = _lib.lib()
    if reserve is not None:
        _lib.check(L.rgfm_profile_reserve(int(reserve)))
    if enable is not None:
        _lib.check(L.rgfm_profile_enable(1 if enable else 0))
    if reset:
        _lib.check(L.rgfm_profile_reset())


def profile_read(kclass):
    """(busy_ms [union of launch intervals], sum_ms, launches, flops) of a kernel class."""
    busy, tot, n, fl = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    _lib.check(_lib.lib().rgfm_profile_read(kclass, ctypes.byref(busy), ctypes.byref(tot), ctypes.byref(n),
                                            ctypes.byref(fl)))
    return busy.value, tot.value, n.value, fl.value


def profile_span(kclass):
    """(start of the first launch, end of the last launch) of a kernel class, ms since the first timed launch."""
    lo, hi = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().rgfm_profile_span(kclass, ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value
