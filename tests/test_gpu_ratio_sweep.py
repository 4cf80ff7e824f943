"""The ratio estimators on the GPU across the sizes and widths they accept (helpers.RATIO_SWEEP): evaluation, the cross
matrix, the gradient of log r, the one-sided gradient and the training pass of every entry against float64
(tests/ratio_flex_ref64.py, tests/ratio_ref64.py, tests/cond_grad_ref64.py), the workspace carve of the raw entry
points, and the independence of a row from its batch.

What each entry reaches is said beside it in tests/helpers.py: rasters of 9 .. 64 pixels a side on either encoder (16
tiles, ragged last tiles, odd rasters at every level, multi-tile level-2 rasters, one-sample and four-sample tiles at
levels 2 .. 4), feature_dim in {64, 192, 320, 512} and hidden_dim in {128, 384, 640, 1024} including both maxima, and the
two fixed kinds away from (256, 512).

Data seeds.  A max-pool whose two largest window elements nearly tie may route differently in another arithmetic: a
discontinuity of the gradient, not an arithmetic error.  Every entry's seed was searched on the CPU by the rule of
tests/ratio_sweep_seeds.py (fp32 takes the float64 argmax in every window and smallest float64 gap >= 10 x the largest
fp32-vs-float64 deviation of a pre-pool tensor, the first such of 1000 candidates; else the best of the 1000, which
must reach 5), and tests/test_ratio_sweep_cpu.py recomputes it.  `python tests/ratio_sweep_seeds.py` printed:

    s64                seed 2910 batch 2 windows  116480 gap 2.450e-05 dev 1.927e-06 ratio  12.7 agree True
    s63                seed 2918 batch 2 windows  131520 gap 1.336e-05 dev 2.092e-06 ratio   6.4 agree True
    s48                seed 2320 batch 2 windows  109312 gap 1.799e-05 dev 2.038e-06 ratio   8.8 agree True
    s56                seed 2509 batch 2 windows   94976 gap 2.607e-05 dev 2.241e-06 ratio  11.6 agree True
    s36                seed 2422 batch 2 windows   51328 gap 2.130e-05 dev 1.915e-06 ratio  11.1 agree True
    y64                seed 3215 batch 2 windows  119232 gap 2.247e-05 dev 2.097e-06 ratio  10.7 agree True
    w192               seed 2600 batch 5 windows    8960 gap 4.595e-05 dev 1.800e-06 ratio  25.5 agree True
    w320               seed 2700 batch 5 windows    8960 gap 1.161e-04 dev 1.678e-06 ratio  69.2 agree True
    w512               seed 2803 batch 5 windows    8960 gap 1.195e-04 dev 1.800e-06 ratio  66.4 agree True
    w64h               seed 2900 batch 5 windows    8960 gap 3.497e-05 dev 1.481e-06 ratio  23.6 agree True
    w512n              seed 3000 batch 5 windows    8960 gap 9.045e-05 dev 2.368e-06 ratio  38.2 agree True
    ms_64              seed 3197 batch 1 windows   44032 gap 1.867e-05 dev 3.141e-06 ratio   5.9 agree True
    ms_192             seed 3197 batch 1 windows   44032 gap 1.867e-05 dev 3.141e-06 ratio   5.9 agree True
    ms_512             seed 3197 batch 1 windows   44032 gap 1.867e-05 dev 3.141e-06 ratio   5.9 agree True
    r28_512            seed 3828 batch 5 windows  105600 gap 2.515e-05 dev 2.645e-06 ratio   9.5 agree True
    ms_64 (training)   seed 3939 batch 2 windows   88064 gap 4.264e-05 dev 7.458e-06 ratio   5.7 agree True
    ms_192 (training)  seed 3939 batch 2 windows   88064 gap 4.264e-05 dev 7.458e-06 ratio   5.7 agree True
    ms_512 (training)  seed 3939 batch 2 windows   88064 gap 4.264e-05 dev 7.458e-06 ratio   5.7 agree True

The six geometry entries hold the rule at batch 2.  RatioEstimatorMNISTSVHN (44 032 windows per sample) does not at the
batches 2 and 5: in eval mode the best of 1000 candidates has 3.6 at batch 2, so the "ms_" entries evaluate one pair
(5.9); under batch statistics the maps differ and batch 2 holds it with a seed of its own (5.7,
helpers.RATIO_SWEEP_TRAIN); no single seed serves both modes (best 4.3 at batch 1, 3.0 at batch 2).

The cross matrix runs on 3 + 2 further images of the same seed: a max-pool is continuous, so evaluation does not need
a searched seed, and the training pass is fed the library's own pool choices.

Bounds: the project's.  Evaluation and cross matrix 1e-5 absolute (TOL_EVAL); gradients, one-sided gradients and
training gradients 1e-4 max |g64| per tensor; training scores 1e-5; BatchNorm buffers 1e-5 of the tensor's maximum and
the analytically zero conv-bias gradients under batch statistics against that conv's weight-gradient scale, both as
tests/test_gpu_ratio_train.py has them.  No entry needed another bound.  Measured on an MI355X: evaluation within 3.3e-6,
cross matrix 1.5e-6, both gradients 2.4e-6 of the tensor's maximum, training scores 1.8e-6 and training gradients
1.9e-5 of the tensor's maximum; all 1 942 784 pool choices the float64 argmax.

Mutations each tried once on a scratch build, never committed: the 1024 zeros of the bias-free reverse Linears cut to
512 (the other 512 set to one) fails the cross matrix at hidden_dim 1024 and both gradients at feature_dim 512
("w512", "w512n", "y64", "ms_512", "r28_512"); launch_grad_act_gn without its memset for odd maps fails both gradients
at "s63", "s36", "y64" and the raw-call test at "s63"; `c < n4` as `c < 128` in cross_ln_silu_kernel fails the cross
matrix at hidden_dim 640 and 1024 ("w320", "w512", "y64", "s63") and the chunked case."""
import ctypes

import pytest
import torch

import cond_grad_ref64 as CG
import ratio_flex_ref64 as RF
import ratio_ref64 as RR
from helpers import RATIO_SWEEP, RATIO_SWEEP_TRAIN, make_sweep_ratio, sweep_ratio_inputs, sweep_ratio_kind
from test_gpu_cond import check_cross, tiled
from test_gpu_ratio_flex import assert_close
from test_gpu_ratio_train import check_choices, loss_of
from ratio_guided_multimodal_fm_amd import _lib

pytestmark = pytest.mark.gpu

TOL_EVAL, TOL_GRAD, TOL_TRAIN, TOL_STATS = 1e-5, 1e-4, 1e-4, 1e-5
TAGS = list(RATIO_SWEEP)
PAD = 1 << 20       # bytes of sentinel on each side of a raw call's workspace
SENTINEL = 0xFF     # byte; four of them are a NaN: workspace that is read before it is written poisons the result


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_modules, _ref = {}, {}


def module(tag, dev):
    """The entry's estimator on the device, shared by the evaluation-mode tests (they leave its parameters alone)."""
    if tag not in _modules:
        _modules[tag] = make_sweep_ratio(tag, dev)
    m = _modules[tag]
    m.loss_type = "disc"
    return m.eval()


def score64(kind, sd, x, y):
    return RF.forward64(sd, x, y) if kind == "flexible" else RR.forward64(kind, sd, x, y, training=False)


def ref(tag):
    """float64 side of an entry in eval mode: scores, log-ratios, two-sided and one-sided gradients under both losses and
    the cross matrix's scores.  Computed once, shared, never modified."""
    if tag not in _ref:
        kind, m = sweep_ratio_kind(tag), make_sweep_ratio(tag)
        x, y, cx, cy = sweep_ratio_inputs(tag)
        sd = CG.params64(m)
        r = {"score": score64(kind, sd, x, y), "cross": score64(kind, sd, *tiled(cx, cy)).reshape(cx.shape[0], cy.shape[0])}
        for lt in ("disc", "rulsif"):
            r["gx_" + lt], r["gy_" + lt], r["lr_" + lt] = CG.grad_both64(kind, sd, x, y, lt)
            r["given_x_" + lt] = CG.grad_given64(kind, sd, x, y, "x", lt)
            r["given_y_" + lt] = CG.grad_given64(kind, sd, y, x, "y", lt)
        _ref[tag] = r
    return _ref[tag]


# ------------------------------------------------------------------ 1. evaluation
@pytest.mark.parametrize("tag", TAGS)
def test_eval_vs_float64(dev, tag):
    x, y, _, _ = sweep_ratio_inputs(tag)
    r = ref(tag)
    m = module(tag, dev)
    xd, yd = x.to(dev), y.to(dev)
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        s, lr = m(xd, yd), m.log_ratio(xd, yd)
        ratio = m._engine.eval(xd, yd, "ratio")
        assert s.shape == lr.shape == ratio.shape == (x.shape[0],)
        for name, got, want in (("score", s, r["score"]), ("log_ratio", lr, r["lr_" + lt]), ("ratio", ratio, r["lr_" + lt].exp())):
            err = float((got.cpu().double() - want).abs().max())
            print(f"{tag} {lt} {name}: err {err:.3e} (max |{name}| {float(want.abs().max()):.3e})")
            assert err < TOL_EVAL, (tag, lt, name, err)


# ------------------------------------------------------------------ 2. the cross matrix
@pytest.mark.parametrize("tag", TAGS)
def test_cross_vs_float64(dev, tag):
    _, _, cx, cy = sweep_ratio_inputs(tag)
    assert cx.shape[0] == 3 and cy.shape[0] == 2
    check_cross(module(tag, dev), cx.to(dev), cy.to(dev), ref(tag)["cross"], tag)


def test_cross_chunks_inside_matrix_rows_at_hidden_1024(dev, monkeypatch):
    """5 x 3 = 15 pairs of "w512" in chunks of 4: the chunks begin at pairs 4, 8 and 12 -- inside matrix rows 1 and 2 and
    at the head of row 4 -- and the last has 3 pairs; each row of cross_ln_silu_kernel holds 1024 values.  Within the
    bound, and bitwise equal to the default chunking."""
    tag = "w512"
    x, y, _, _ = sweep_ratio_inputs(tag)
    x, y = x[:5], y[:3]
    m = module(tag, dev)
    xd, yd = x.to(dev), y.to(dev)
    plain = {w: m._engine.eval_cross(xd, yd, w).clone() for w in ("score", "log_ratio", "ratio")}
    sd = CG.params64(make_sweep_ratio(tag))
    s64 = score64("flexible", sd, *tiled(x, y)).reshape(5, 3)
    monkeypatch.setenv("RGFM_CROSS_ROWS", "4")
    check_cross(m, xd, yd, s64, "w512, RGFM_CROSS_ROWS=4")
    for w, want in plain.items():
        assert torch.equal(m._engine.eval_cross(xd, yd, w), want), w


# ------------------------------------------------------------------ 3. gradient of log r
@pytest.mark.parametrize("tag", TAGS)
def test_grad_log_ratio_vs_float64_autograd(dev, tag):
    x, y, _, _ = sweep_ratio_inputs(tag)
    r = ref(tag)
    m = module(tag, dev)
    xd, yd = x.to(dev), y.to(dev)
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        gx, gy, lr = m._engine.grad_log_ratio(xd, yd)
        assert gx.shape == x.shape and gy.shape == y.shape
        assert_close(gx, r["gx_" + lt], f"{tag} {lt} gx", TOL_GRAD)
        assert_close(gy, r["gy_" + lt], f"{tag} {lt} gy", TOL_GRAD)
        err = float((lr.cpu().double() - r["lr_" + lt]).abs().max())
        print(f"{tag} {lt} log_ratio: err {err:.3e}")
        assert err < TOL_EVAL, (tag, lt, err)


# ------------------------------------------------------------------ 4. the one-sided gradient
@pytest.mark.parametrize("tag", TAGS)
def test_one_sided_gradient_vs_float64(dev, tag):
    x, y, _, _ = sweep_ratio_inputs(tag)
    r = ref(tag)
    m = module(tag, dev)
    xd, yd = x.to(dev), y.to(dev)
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        for given, cond, target in (("x", xd, yd), ("y", yd, xd)):
            g64, lr64 = r[f"given_{given}_{lt}"]
            ctx = m._engine.cond_prepare(cond, given, tuple(target.shape[1:]))
            g, lr = m._engine.grad_log_ratio_cond(ctx, given, target)
            assert g.shape == target.shape and lr.shape == (x.shape[0],)
            assert_close(g, g64, f"{tag} {lt} given={given} g_target", TOL_GRAD)
            err = float((lr.cpu().double() - lr64).abs().max())
            print(f"{tag} {lt} given={given} log_ratio: err {err:.3e}")
            assert err <= TOL_EVAL, (tag, lt, given, err)
            assert torch.equal(m.grad_log_ratio_given(cond, target, given), g)  # the module-level API


# ------------------------------------------------------------------ 5. the training pass
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("tag", TAGS)
def test_training_pass_vs_float64(dev, tag, training):
    """forward_train + backward in training mode (dropout; batch statistics in the BatchNorm kind) and in eval mode; the
    float64 side is fed the library's pool choices and dropout masks.

    Both sides are handed ONE dL/dscore: that of the float64 loss, rounded to fp32.  The backward is linear in it and the
    library receives it as an input; taken from torch's fp32 loss on the device it would differ from the float64 one by
    fp32 rounding of terms of size 0.5, while their sum over the batch -- the gradient of the head's bias, a tensor of
    one element -- cancels under a two-class loss on scores near zero (float64: to 1.4e-3 at "y64"), so that
    1e-4 max |g64| of that tensor (1.4e-7) would bound the loss's rounding and not a kernel."""
    kind = sweep_ratio_kind(tag)
    lt = "disc" if TAGS.index(tag) % 2 == 0 else "rulsif"  # (the loss type only shapes dL/dscore here; both are covered)
    m = make_sweep_ratio(tag, dev, lt)  # its own module: training mode moves the BatchNorm buffers
    # (the BatchNorm kind's maps in front of the pools are others under batch statistics: that mode has its own seed)
    x, y, _, _ = sweep_ratio_inputs(tag, *RATIO_SWEEP_TRAIN[tag]) if training and tag in RATIO_SWEEP_TRAIN else sweep_ratio_inputs(tag)
    B = x.shape[0]
    real = torch.arange(B) % 2 == 0
    sd = RF.params64(m) if kind == "flexible" else RR.params64(m)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    eng, p = m._engine, m.dropout_p()
    xd, yd = x.to(dev), y.to(dev)
    masks = None
    if training:  # the keep masks of the seed forward_train is about to draw
        torch.cuda.manual_seed(99)
        seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())
        eng.bind(xd, yd)
        masks = [eng.dropout_mask(b, seed, p, B, dev).cpu() for b in (0, 1)]
        widths = [l.out_features for l in m.score_net if isinstance(l, torch.nn.Linear)][:2]
        assert [tuple(k.shape) for k in masks] == [(B, w) for w in widths]
        assert all(set(torch.unique(k).tolist()) <= {0.0, 1.0} for k in masks)
        torch.cuda.manual_seed(99)
    m.train(training)
    xg, yg = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    scores = m.forward_train(xg, yg)
    choices = [[c.cpu() for c in enc] for enc in eng.pool_choices()]
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    out = {}
    if kind == "flexible":
        s64 = RF.forward64(sd, x64, y64, choices, masks, p if training else 0.0, out)
    else:
        s64 = RR.forward64(kind, sd, x64, y64, training, choices, masks, p if training else 0.0, out)
    (d64,) = torch.autograd.grad(loss_of(s64, real, lt), s64, retain_graph=True)
    dscore = d64.float()
    assert float(dscore.abs().min()) > 0
    scores.backward(dscore.to(dev))
    s64.backward(dscore.double())
    m.eval()
    err = float((scores.detach().cpu().double() - s64.detach()).abs().max())
    print(f"{tag} training={training} scores: err {err:.3e}")
    assert err <= TOL_EVAL, (tag, err)
    check_choices(choices, out["windows"])
    assert_close(xg.grad, x64.grad, f"{tag} dx", TOL_TRAIN)
    assert_close(yg.grad, y64.grad, f"{tag} dy", TOL_TRAIN)
    for k, q in m.named_parameters():
        if kind == "mnist_svhn" and training and ".conv" in k and k.endswith(".bias"):
            # analytically zero under batch statistics: bounded against the scale of that conv's weight gradient
            wscale = float(sd[k[:-4] + "weight"].grad.abs().max())
            print(f"{k}: max |g| {float(q.grad.abs().max()):.3e} weight-gradient scale {wscale:.3e}")
            assert float(q.grad.abs().max()) <= TOL_TRAIN * wscale, k
        else:
            assert_close(q.grad, sd[k].grad, f"{tag} {k}", TOL_TRAIN)
    now = m.state_dict()
    for k, v0 in before.items():
        if "running" not in k and "num_batches" not in k:
            continue
        if not training:
            assert torch.equal(now[k].cpu(), v0), k  # eval mode leaves the buffers alone, bitwise
        elif "num_batches" in k:
            assert int(now[k]) == int(v0) + 1 == int(out["buffers"][k]), k
        else:
            r = out["buffers"][k]
            assert float((now[k].cpu().double() - r).abs().max()) <= TOL_STATS * float(r.abs().max()), k


# ------------------------------------------------------------------ 6. the workspace carve of the raw entry points
def _padded(nbytes, dev):
    """(whole buffer, the nbytes in its middle): PAD sentinel bytes on each side, so that an overrun of the carve lands
    in memory this test owns."""
    big = torch.full((PAD + nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    return big, big[PAD:PAD + nbytes]


def _intact(big, nbytes):
    return bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + nbytes:] == SENTINEL).all())


def _untouched(*tensors):
    return all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in tensors)


def _sentinel_like(t):
    """A float tensor of t's shape whose every byte is the sentinel."""
    return torch.full((t.numel() * 4,), SENTINEL, dtype=torch.uint8, device=t.device).view(torch.float32).view(t.shape)


@pytest.mark.parametrize("tag", ["s63", "s64", "w512"])
def test_raw_calls_with_the_exact_workspace(dev, tag):
    """rgfm_ratio_eval, _eval_cross, _grad_log_ratio, _grad_log_ratio_cond and _forward_train + _backward through ctypes
    with a workspace of exactly *_workspace_bytes, taken from the middle of a larger sentinel-filled buffer: the padding
    stays bitwise intact, the results equal the Python path's bitwise, and one byte less is RGFM_ENOMEM with nothing
    written."""
    x, y, cx, cy = (t.to(dev) for t in sweep_ratio_inputs(tag))
    n, nx, ny = x.shape[0], cx.shape[0], cy.shape[0]
    m = module(tag, dev)
    eng = m._engine
    want = {"score": m(x, y), "cross": m.forward_cross(cx, cy)}
    want["gx"], want["gy"], want["lr"] = eng.grad_log_ratio(x, y)
    ctx = eng.cond_prepare(x, "x", tuple(y.shape[1:]))
    want["g_cond"], want["lr_cond"] = eng.grad_log_ratio_cond(ctx, "x", y)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    s = m.forward_train(xg, yg)  # eval mode: no dropout
    s.sum().backward()
    want["train_score"], want["dx"], want["dy"] = s.detach(), xg.grad, yg.grad
    want["dparams"] = torch.cat([q.grad.reshape(-1) for q in m.parameters()])  # (no buffers: state_dict order)
    m.zero_grad(set_to_none=True)
    eng.bind(x, y)
    L, h, nb, st = _lib.lib(), eng.handle(dev), ctypes.c_size_t(), _stream()

    def run(size_fn, size_args, call, outs, names):
        _lib.check(size_fn(h, *size_args, ctypes.byref(nb)))
        big, ws = _padded(nb.value, dev)
        assert call(ws, nb.value - 1) == -2
        torch.cuda.synchronize()
        assert _untouched(big, *outs), names
        _lib.check(call(ws, nb.value))
        torch.cuda.synchronize()
        assert _intact(big, nb.value), names
        for o, k in zip(outs, names):
            assert torch.equal(o, want[k]), (tag, k, float((o - want[k]).abs().max()))
        return big, ws

    o = _sentinel_like(want["score"])
    run(L.rgfm_ratio_workspace_bytes, (n,), lambda ws, b: L.rgfm_ratio_eval(h, _p(x), _p(y), _p(o), n, 0, _p(ws), b, st),
        [o], ["score"])
    o = _sentinel_like(want["cross"])
    run(L.rgfm_ratio_cross_workspace_bytes, (nx, ny),
        lambda ws, b: L.rgfm_ratio_eval_cross(h, _p(cx), nx, _p(cy), ny, _p(o), 0, _p(ws), b, st), [o], ["cross"])
    gx, gy, lr = _sentinel_like(x), _sentinel_like(y), _sentinel_like(want["lr"])
    run(L.rgfm_ratio_grad_workspace_bytes, (n,),
        lambda ws, b: L.rgfm_ratio_grad_log_ratio(h, _p(x), _p(y), _p(gx), _p(gy), _p(lr), n, _p(ws), b, st),
        [gx, gy, lr], ["gx", "gy", "lr"])
    g, lr = _sentinel_like(y), _sentinel_like(want["lr_cond"])
    run(L.rgfm_ratio_grad_cond_workspace_bytes, (0, n),
        lambda ws, b: L.rgfm_ratio_grad_log_ratio_cond(h, _p(ctx), 0, _p(y), _p(g), _p(lr), n, _p(ws), b, st),
        [g, lr], ["g_cond", "lr_cond"])
    sc = _sentinel_like(want["train_score"])
    big, ws = run(L.rgfm_ratio_train_workspace_bytes, (n,),
                  lambda ws, b: L.rgfm_ratio_forward_train(h, _p(x), _p(y), _p(sc), n, 0, 0.0, 0, None, _p(ws), b, st),
                  [sc], ["train_score"])
    dscore = torch.ones(n, device=dev)
    dx, dy, dp = _sentinel_like(x), _sentinel_like(y), _sentinel_like(want["dparams"])
    call = lambda b: L.rgfm_ratio_backward(h, _p(dscore), _p(dx), _p(dy), _p(dp), n, _p(ws), b, st)  # noqa: E731
    assert call(nb.value - 1) == -2
    torch.cuda.synchronize()
    assert _untouched(dx, dy, dp)
    _lib.check(call(nb.value))
    torch.cuda.synchronize()
    assert _intact(big, nb.value)
    for got, k in ((dx, "dx"), (dy, "dy"), (dp, "dparams")):
        assert torch.equal(got, want[k]), (tag, k, float((got - want[k]).abs().max()))


# ------------------------------------------------------------------ 7. rows do not depend on the batch
@pytest.mark.parametrize("tag", ["s48", "w320"])
def test_rows_do_not_depend_on_the_batch(dev, tag):
    """Row b of a batch-5 evaluation equals the batch-1 evaluation of that row bitwise: one sample of a four-sample tile
    against a full tile, one row of a Linear's row block against five."""
    x, y, _, _ = (t.to(dev) for t in sweep_ratio_inputs(tag, batch=5))
    m = module(tag, dev)
    for lt in ("disc", "rulsif"):
        m.loss_type = lt
        full = {w: m._engine.eval(x, y, w) for w in ("score", "log_ratio", "ratio")}
        for b in range(5):
            for w, f in full.items():
                one = m._engine.eval(x[b:b + 1], y[b:b + 1], w)
                assert torch.equal(one, f[b:b + 1]), (tag, lt, w, b, float(one - f[b]))
