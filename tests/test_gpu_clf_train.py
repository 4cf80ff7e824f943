"""Training pass of the evaluation classifiers on the GPU (rgfm_clf_*): gradients against a float64 restatement fed the
library's pool choices, ReLU gates and dropout masks (tests/clf_ref64.py) and against the reference's autograd
(tests/golden/clf_train_grad.npz), BatchNorm buffers, dropout, the fused cross-entropy kernel, determinism, row
independence, optimiser steps, the hand-back of the parameters, the CLI and the error paths."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, make_module
from clf_ref64 import NETS, first_argmax, forward64, params64
from ratio_guided_multimodal_fm_amd import _engine, _lib, evaluate, evaluate_mnist_svhn, train_classifier
from ratio_guided_multimodal_fm_amd.utils.losses import cross_entropy
from ratio_guided_multimodal_fm_amd.utils.trainer import ClassifierTrainer

pytestmark = pytest.mark.gpu

TAGS = {"mnist28": "clf_mnist28", "mnist32": "clf_mnist", "svhn": "clf_svhn"}
TOL_GRAD = 1e-4    # max |g - g64| <= TOL_GRAD * max |g64| per tensor (tests/test_gpu_ratio_train.py)
TOL_LOSS = 1e-5    # relative
TOL_LOGIT = 1e-5   # of max(1, max |logits64|)
TOL_STATS = 1e-5   # of the tensor's maximum
TOL_DECIDE = 1e-5  # a gate / choice is a near-sign / near-argmax within this share of the tensor's maximum


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.lib()
    return torch.device("cuda:0")


def inputs(kind, B, salt=0):
    """Seeded Gaussian images and labels that walk through the classes.  For these seeds the modules' own fp32 torch
    forward on the CPU takes the float64 decision at every pool choice and at every gate but one (measured over every
    case below: 1 gate of 1 880 320 at B = 65, SVHN, training mode), far inside the 99.9 % the tests ask of the
    library."""
    g = torch.Generator().manual_seed(1900 + B + 1000 * salt + 7 * sorted(TAGS).index(kind))
    return torch.randn(B, *NETS[kind][0], generator=g), (torch.arange(B) * 3 + 1) % 10


def hip_run(m, x, labels, training, dev):
    """One forward_train + fused cross-entropy + backward; returns what the float64 side needs to follow it."""
    m.train(training)
    m.zero_grad(set_to_none=True)
    xg = x.to(dev).requires_grad_(True)
    logits = m.forward_train(xg)
    eng = m._engine
    choices = [None if c is None else c.cpu() for c in eng.pool_choices()]
    gates = [g.cpu() for g in eng.gates()]
    seed, p = eng.last_dropout()
    loss, pred = cross_entropy(logits, labels.to(dev))
    loss.backward()
    m.eval()
    return dict(logits=logits.detach().cpu(), loss=loss.item(), pred=pred.cpu(), dx=xg.grad.cpu(), choices=choices,
                gates=gates, seed=seed, p=p, grads={k: q.grad.cpu() for k, q in m.named_parameters()})


def ref_run(kind, sd, x, labels, training, choices, gates, mask=None, p_drop=0.0):
    x64 = x.double().requires_grad_(True)
    out = {}
    logits = forward64(kind, sd, x64, training, choices, gates, mask, p_drop, out)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    return dict(logits=logits.detach(), loss=loss.item(), dx=x64.grad, out=out,
                grads={k: v.grad for k, v in sd.items() if v.requires_grad})


def assert_close(g, g64, what, tol=TOL_GRAD):
    scale = float(g64.abs().max())
    err = float((g.double() - g64).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / max(scale, 1e-300):.3e}")
    assert err <= tol * max(scale, 1e-30), (what, err, scale)


def check_decisions(choices, gates, out):
    """Every choice the library made is a near-argmax and every gate a near-sign in float64, and each equals the float64
    decision in >= 99.9 % of positions."""
    c_exact = c_total = g_exact = g_total = 0
    for i, pre in enumerate(out["pre"]):
        tol = TOL_DECIDE * float(pre.abs().max())
        if i < len(choices) and choices[i] is not None:
            k = choices[i].to(torch.int64)
            assert int(k.min()) >= 0 and int(k.max()) <= 3
            rw = F.relu(pre)
            assert bool((rw.gather(-1, k[..., None])[..., 0] >= rw.max(-1).values - tol).all()), i
            c_exact += int((k == first_argmax(rw)).sum())
            c_total += k.numel()
            y = pre.gather(-1, k[..., None])[..., 0]
        else:
            y = pre
        g = gates[i]
        assert set(torch.unique(g).tolist()) <= {0.0, 1.0} and g.shape == y.shape, i
        assert bool((y[g == 1] > -tol).all()) and bool((y[g == 0] < tol).all()), i
        g_exact += int(((y > 0) == (g == 1)).sum())
        g_total += g.numel()
    print(f"pool choices: {c_exact} / {c_total} are the float64 argmax; gates: {g_exact} / {g_total} are the float64 sign")
    assert c_exact >= 0.999 * c_total and g_exact >= 0.999 * g_total, (c_exact, c_total, g_exact, g_total)


def compare(m, kind, hip, ref, training, sd_before):
    scale = max(1.0, float(ref["logits"].abs().max()))
    err = float((hip["logits"].double() - ref["logits"]).abs().max())
    print(f"logits: err {err:.3e} scale {scale:.3e}; loss {hip['loss']:.8f} vs {ref['loss']:.8f}")
    assert err <= TOL_LOGIT * scale
    assert abs(hip["loss"] - ref["loss"]) <= TOL_LOSS * abs(ref["loss"])
    check_decisions(hip["choices"], hip["gates"], ref["out"])
    assert_close(hip["dx"], ref["dx"], "dx")
    for k, g in hip["grads"].items():
        if kind == "svhn" and training and k.startswith("conv") and k.endswith(".bias"):
            # in front of a training-mode BatchNorm: analytically zero, bounded against that conv's weight gradient
            wscale = float(ref["grads"][k[:-4] + "weight"].abs().max())
            print(f"{k}: max |g| {float(g.abs().max()):.3e} weight-gradient scale {wscale:.3e}")
            assert float(g.abs().max()) <= TOL_GRAD * wscale, k
        else:
            assert_close(g, ref["grads"][k], k)
    now = m.state_dict()
    for k, v0 in sd_before.items():
        if "running" not in k and "num_batches" not in k:
            continue
        if training:
            r = ref["out"]["buffers"][k]
            if "num_batches" in k:
                assert int(now[k]) == int(v0) + 1 == int(r), k
            else:
                assert float((now[k].cpu().double() - r).abs().max()) <= TOL_STATS * float(r.abs().max()), k
        else:
            assert torch.equal(now[k].cpu(), v0), k  # eval mode leaves the buffers alone, bitwise


def run_case(dev, kind, B, training, p=0.0):
    m = make_module(TAGS[kind], dev)
    m.dropout.p = p
    x, labels = inputs(kind, B)
    sd = params64(m)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    hip = hip_run(m, x, labels, training, dev)
    ref = ref_run(kind, sd, x, labels, training, hip["choices"], hip["gates"])
    assert torch.equal(hip["pred"], hip["logits"].argmax(1))
    compare(m, kind, hip, ref, training, before)


# B = 17: BatchNorm slices of 2 samples with a ragged last slice; 65: past the GEMMs' 64-row tile and the wgrad K
# split; 2 and 3: multiples of nothing
@pytest.mark.parametrize("B", [2, 3, 17, 65])
@pytest.mark.parametrize("kind", sorted(TAGS))
def test_gradients_vs_float64_training_mode(dev, kind, B):
    run_case(dev, kind, B, True)


@pytest.mark.parametrize("B", [1, 2, 3, 17, 65])
@pytest.mark.parametrize("kind", sorted(TAGS))
def test_gradients_vs_float64_eval_mode(dev, kind, B):
    run_case(dev, kind, B, False)


@pytest.mark.parametrize("case,kind,training", [("mnist28_train", "mnist28", True), ("mnist32_train", "mnist32", True),
                                                ("svhn_train", "svhn", True), ("svhn_eval", "svhn", False)])
def test_gradients_vs_reference_autograd(dev, case, kind, training):
    gold = golden("clf_train_grad")
    m = make_module(TAGS[kind], dev)
    m.dropout.p = 0.0
    x = torch.randn(4, *NETS[kind][0], generator=torch.Generator().manual_seed(int(gold[f"{case}_seed"])))
    hip = hip_run(m, x, (torch.arange(4) * 3 + 1) % 10, training, dev)  # (tests/golden/make_clf_golden.py: inputs, labels)
    r = gold[f"{case}_logits"]
    assert np.abs(hip["logits"].numpy() - r).max() <= TOL_LOGIT * max(1.0, np.abs(r).max())
    assert abs(hip["loss"] - float(gold[f"{case}_loss"])) <= TOL_LOSS * abs(float(gold[f"{case}_loss"]))
    r = gold[f"{case}_dx"]
    assert np.abs(hip["dx"].numpy() - r).max() <= TOL_GRAD * np.abs(r).max()
    for k, v in m.state_dict().items():
        if "running" in k:
            r = gold[f"{case}_buf_{k}"]
            assert np.abs(v.cpu().numpy() - r).max() <= TOL_STATS * np.abs(r).max(), k
        elif "num_batches" in k:
            assert int(v) == int(gold[f"{case}_buf_{k}"]), k
    for i, (k, g) in enumerate(hip["grads"].items()):
        gf = g.reshape(-1)
        idx = torch.randint(0, gf.numel(), (64,), generator=torch.Generator().manual_seed(7000 + i))
        amax = float(gold[f"{case}_amax_{i}"])
        if kind == "svhn" and training and k.startswith("conv") and k.endswith(".bias"):
            assert float(gf.abs().max()) <= TOL_GRAD * float(gold[f"{case}_amax_{i - 1}"]), k
            continue
        assert abs(float(gf.abs().max()) - amax) <= TOL_GRAD * amax, k
        assert np.abs(gf[idx].numpy() - gold[f"{case}_probe_{i}"]).max() <= TOL_GRAD * amax, k


@pytest.mark.parametrize("kind", sorted(TAGS))
def test_dropout_mask_and_gradients(dev, kind):
    m = make_module(TAGS[kind], dev)
    p = m.dropout_p()
    assert p == pytest.approx(0.3 if kind == "svhn" else 0.25)
    eng = m._engine
    B = 65
    x, labels = inputs(kind, B, salt=1)
    sd = params64(m)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    torch.cuda.manual_seed(99)
    seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())  # drawn like forward_train
    mask = eng.dropout_mask(seed, p, B, dev).cpu()
    assert set(torch.unique(mask).tolist()) <= {0.0, 1.0}
    # the keep fraction over 65 x 256 units (130 rows of the 128-wide nets): 4 binomial standard deviations
    units = eng.dropout_mask(seed, p, B * 256 // mask.shape[1], dev)
    n = units.numel()
    assert n == 65 * 256
    kept = float(units.sum()) / n
    print(f"kept {kept:.4f} of {n} units, p = {p}")
    assert abs(kept - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n), kept
    torch.cuda.manual_seed(99)
    hip = hip_run(m, x, labels, True, dev)
    assert (hip["seed"], hip["p"]) == (seed, pytest.approx(p))  # the mask above is the mask that forward used
    ref = ref_run(kind, sd, x, labels, True, hip["choices"], hip["gates"], mask, p)
    compare(m, kind, hip, ref, True, before)
    # the same generator seed: the same mask, bitwise-equal results; the next call draws another
    runs = []
    for s in (99, 99, None):
        m.load_state_dict(before)
        if s is not None:
            torch.cuda.manual_seed(s)
        runs.append(hip_run(m, x, labels, True, dev))
    assert torch.equal(runs[0]["logits"], runs[1]["logits"]) and torch.equal(runs[0]["dx"], runs[1]["dx"])
    assert all(torch.equal(runs[0]["grads"][k], runs[1]["grads"][k]) for k in runs[0]["grads"])
    assert runs[2]["seed"] != runs[0]["seed"] and not torch.equal(runs[0]["logits"], runs[2]["logits"])
    # p = 0 is the identity; so is eval mode at any p
    assert bool((eng.dropout_mask(seed, 0.0, B, dev) == 1).all())
    m.load_state_dict(before)
    ev = hip_run(m, x, labels, False, dev)
    m.dropout.p = 0.0
    ev0 = hip_run(m, x, labels, False, dev)
    assert torch.equal(ev["logits"], ev0["logits"]) and torch.equal(ev["dx"], ev0["dx"])
    if kind != "svhn":  # (no batch statistics: training mode at p = 0 is eval mode)
        assert torch.equal(hip_run(m, x, labels, True, dev)["logits"], ev0["logits"])


@pytest.mark.parametrize("n", [1, 3, 257])
def test_cross_entropy_kernel_vs_float64(dev, n):
    """Logits of N(0, 1) x 80: exp of an unshifted logit would overflow fp32.  The row losses come back in fp64."""
    g = torch.Generator().manual_seed(40 + n)
    logits = (torch.randn(n, 10, generator=g) * 80).to(dev)
    assert float(logits.max()) > 89  # exp(89) overflows fp32
    assert int(torch.topk(logits, 2, dim=1).values.diff(dim=1).abs().min() > 0)  # no ties
    for off in range(10 if n < 10 else 1):  # every class is a label
        labels = (torch.arange(n) + off) % 10
        lg = logits.clone().requires_grad_(True)
        loss, pred, rows = _engine.cross_entropy(lg, labels.to(dev))
        loss.backward()
        l64 = logits.detach().cpu().double().requires_grad_(True)
        rows64 = F.cross_entropy(l64, labels, reduction="none")
        rows64.mean().backward()
        assert rows.dtype == torch.float64 and loss.dtype == torch.float32
        err_rows = float((rows.cpu() - rows64.detach()).abs().max())
        err_d = float((lg.grad.cpu().double() - l64.grad).abs().max())
        print(f"n {n} off {off}: rows err {err_rows:.3e} (max {float(rows64.detach().max()):.1f}) dlogits err {err_d:.3e}")
        assert err_rows <= 1e-6 and err_d <= 1e-6
        assert abs(float(loss.detach()) - float(rows64.detach().mean())) <= 1e-6 * max(1.0, float(rows64.detach().mean()))
        assert torch.equal(pred.cpu(), logits.cpu().argmax(1))
        loss2, pred2, rows2 = _engine.cross_entropy(logits, labels.to(dev))
        assert torch.equal(loss2, loss.detach()) and torch.equal(rows2, rows) and torch.equal(pred2, pred)
    lo, pr = cross_entropy(logits, ((torch.arange(n)) % 10).to(dev))  # the public two-value form
    assert lo.shape == () and pr.dtype == torch.int64 and pr.shape == (n,)


@pytest.mark.parametrize("kind", sorted(TAGS))
def test_determinism_and_row_independence(dev, kind):
    """Two identical training calls agree bitwise.  In eval mode row b of a B = 5 call equals the B = 1 call on that row
    BITWISE: every output element of every kernel of the forward is one fixed-order sum over its own row's data -- the
    convs' K loop runs over (input channel, tap) of one output pixel, fc1's split-K ranges are chosen from the row-tile
    count (one tile for B = 1 and B = 5 alike) and an MFMA accumulates each output element independently of the other
    rows of its tile, fc2 is a per-output loop -- and the eval-mode BatchNorm uses constants."""
    m = make_module(TAGS[kind], dev)
    m.dropout.p = 0.0
    x, labels = inputs(kind, 17, salt=2)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    a = hip_run(m, x, labels, True, dev)
    bufs_a = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.load_state_dict(before)
    b = hip_run(m, x, labels, True, dev)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["dx"], b["dx"]) and a["loss"] == b["loss"]
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
    assert all(torch.equal(v, bufs_a[k]) for k, v in m.state_dict().items())
    m.load_state_dict(before)
    m.eval()
    x5 = x[:5].to(dev)
    with torch.no_grad():
        all5 = m.forward_train(x5)
        for r in range(5):
            one = m.forward_train(x5[r:r + 1])
            assert torch.equal(one[0], all5[r]), (r, float((one[0] - all5[r]).abs().max()))


def spy_on_forward_train(m, log):
    """Records the decisions of every forward_train call of `m` (they are readable until its backward)."""
    orig = m.forward_train

    def spy(x):
        out = orig(x)
        eng = m._engine
        log.append(([None if c is None else c.cpu() for c in eng.pool_choices()], [g.cpu() for g in eng.gates()],
                    eng.last_dropout()))
        return out
    m.forward_train = spy


@pytest.mark.parametrize("kind", sorted(TAGS))
def test_sgd_steps_match_float64_and_hand_back(dev, kind):
    m = make_module(TAGS[kind], dev)
    p, B, lr = m.dropout_p(), 17, 0.05
    x, labels = inputs(kind, B, salt=3)
    sd64 = params64(m, requires_grad=False)
    names = {k for k, _ in m.named_parameters()}
    log = []
    spy_on_forward_train(m, log)
    trainer = ClassifierTrainer(m, torch.optim.SGD(m.parameters(), lr=lr), dev)
    torch.cuda.manual_seed(5)
    h0 = None
    for step in range(3):
        m.train()
        trainer.train_step(x, labels)
        h0 = h0 or m._engine._handle.value
        choices, gates, (seed, pd) = log[-1]
        mask = m._engine.dropout_mask(seed, pd, B, dev).cpu()
        p64 = {k: v.clone().requires_grad_(k in names) for k, v in sd64.items()}
        out = {}
        F.cross_entropy(forward64(kind, p64, x, True, choices, gates, mask, pd, out), labels).backward()
        sd64 = {k: (v - lr * v.grad).detach() if k in names else out["buffers"].get(k, v).detach() for k, v in p64.items()}
    assert len(log) == 3 and pd == pytest.approx(p)
    del m.forward_train  # (the spy: without autograd nothing keeps a call's saved state)
    m.eval()
    for k, v in m.state_dict().items():
        r = sd64[k].double()
        err = float((v.cpu().double() - r).abs().max())
        print(f"{k}: err {err:.3e} scale {float(r.abs().max()):.3e}")
        assert err <= 1e-4 * max(float(r.abs().max()), 1e-12), k
    # the eval-mode device forward sees the stepped parameters: the module's own torch forward, float64 on the CPU
    with torch.no_grad():
        got = m.forward_train(x.to(dev)).cpu().double()
    assert m._engine._handle.value == h0  # refreshed in place (rgfm_clf_update_params), not re-created
    m64 = type(m)().double().eval()
    m64.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        want = m64(x.double())
    err = float((got - want).abs().max())
    print(f"hand-back: err {err:.3e} scale {float(want.abs().max()):.3e}")
    assert err <= 1e-5 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("kind", sorted(TAGS))
def test_adam_steps_decrease_the_loss(dev, kind):
    m = make_module(TAGS[kind], dev)
    m.dropout.p = 0.0
    x, labels = inputs(kind, 17, salt=4)
    trainer = ClassifierTrainer(m, torch.optim.Adam(m.parameters(), lr=1e-3), dev)
    m.train()
    losses = [float(trainer.train_step(x, labels)[0]) for _ in range(4)]
    m.eval()
    print(f"losses {losses}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def pattern_dataset(shape, seed=0, per_class=64, noise=0.5):
    """10 classes x per_class images: class c is a low-frequency plane wave whose direction and frequency depend on
    c, in every channel, plus Gaussian noise; shuffled, so that the held-out tail holds every class."""
    g = torch.Generator().manual_seed(seed)
    C, S, _ = shape
    yy, xx = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
    label = torch.arange(10).repeat_interleave(per_class)
    ang = label.float() * (np.pi / 10)
    freq = 1.0 + (label % 3).float()
    phase = 2 * np.pi * freq[:, None, None] * (torch.cos(ang)[:, None, None] * xx + torch.sin(ang)[:, None, None] * yy)
    x = 0.7 * torch.cos(phase)[:, None].expand(-1, C, -1, -1) + noise * torch.randn(label.numel(), C, S, S, generator=g)
    perm = torch.randperm(label.numel(), generator=g)
    return x[perm].clamp(-1, 1).contiguous(), label[perm]


@pytest.mark.parametrize("kind", sorted(TAGS))
def test_cli_end_to_end(dev, kind, tmp_path, monkeypatch):
    """train_classifier.main for 2 epochs at batch 32 on pattern_dataset, then the coherence evaluation on the
    checkpoint it wrote.  The same loop (same split, Adam 1e-3, 2 epochs, batch 32, seed 42) on the plain torch
    module on the CPU reaches a held-out accuracy of 1.000 (mnist28), 1.000 (mnist32) and 1.000 (svhn); the HIP run
    must reach 0.90: the 0.05 below the 0.95 asked of the CPU loop is for the other dropout stream and summation order."""
    monkeypatch.chdir(tmp_path)
    shape = NETS[kind][0]
    x, label = pattern_dataset(shape)
    np.savez(tmp_path / "data.npz", x=x.numpy(), label=label.numpy())
    best = train_classifier.main(["--kind", kind, "--data", "data.npz", "--epochs", "2", "--batch_size", "32"])
    print(f"{kind}: held-out accuracy {best:.4f}")
    assert best >= 0.90
    path = tmp_path / train_classifier.checkpoint_path(kind)
    assert path.exists()
    clf = type(make_module(TAGS[kind]))().to(dev)
    clf.load_state_dict(torch.load(path, map_location=dev), strict=True)
    xt, lt = x[-64:], label[-64:]
    if kind == "mnist28":
        met = evaluate.evaluate_coherence(xt, torch.rot90(xt, 1, (2, 3)), clf, dev, "rotate90")
    else:
        other = make_module(TAGS["svhn" if kind == "mnist32" else "mnist32"], dev)
        xo = pattern_dataset(NETS["svhn" if kind == "mnist32" else "mnist32"][0])[0][-64:]
        pair = (xt, xo, clf, other) if kind == "mnist32" else (xo, xt, other, clf)
        met = evaluate_mnist_svhn.evaluate_coherence(*pair, dev)
    print(met)
    assert 0.0 <= met["coherence_acc"] <= 1.0
    with torch.no_grad():  # the plain torch forward of the checkpoint on the held-out tail
        acc = float((clf.eval()(xt.to(dev)).argmax(1).cpu() == lt).float().mean())
    print(f"{kind}: the checkpoint's torch forward: {acc:.4f}")
    assert acc >= 0.90 and acc <= best + 1.0 / 64 + 1e-6


def test_errors(dev):
    m = make_module("clf_mnist", dev)
    L = _lib.lib()
    h = m._engine.handle(dev)
    nb = ctypes.c_size_t()
    assert L.rgfm_clf_train_workspace_bytes(h, 3, ctypes.byref(nb)) == 0
    x = torch.zeros(3, 1, 32, 32, device=dev)
    out = torch.full((3, 10), 7.0, device=dev)
    ws = torch.zeros(nb.value, dtype=torch.uint8, device=dev)
    short = L.rgfm_clf_forward_train(h, x.data_ptr(), out.data_ptr(), 3, 0, 0, 0.0, None, ws.data_ptr(), nb.value - 1, None)
    assert short == -2 and b"too small" in L.rgfm_last_error()
    assert L.rgfm_clf_backward(h, out.data_ptr(), None, out.data_ptr(), 3, ws.data_ptr(), nb.value - 1, None) == -2
    assert L.rgfm_clf_forward_train(h, x.data_ptr(), out.data_ptr(), 0, 0, 0, 0.0, None, ws.data_ptr(), nb.value, None) == -1
    assert L.rgfm_clf_forward_train(h, None, out.data_ptr(), 3, 0, 0, 0.0, None, ws.data_ptr(), nb.value, None) == -1
    assert L.rgfm_clf_pool_choice(h, ws.data_ptr(), 2, 3, out.data_ptr()) == -1  # conv3 has no pool behind it
    assert L.rgfm_clf_gate(h, ws.data_ptr(), 4, 3, out.data_ptr()) == -1
    assert L.rgfm_clf_xent(out.data_ptr(), ws.data_ptr(), 3, 33, 1.0, ws.data_ptr(), None, None, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not ws.any()  # nothing was touched
    with pytest.raises(_lib.RgfmError, match=r"\[B,1,32,32\]"):
        m.forward_train(torch.zeros(2, 1, 28, 28, device=dev))
    with pytest.raises(_lib.RgfmError, match=r"\[B,3,32,32\]"):
        make_module("clf_svhn", dev).forward_train(torch.zeros(2, 1, 32, 32, device=dev))
    with pytest.raises(_lib.RgfmError, match="no saved state"):  # the message of the ratio engine
        m._engine.pool_choices()
    logits = m.forward_train(x.requires_grad_(True))
    logits.sum().backward(retain_graph=True)
    with pytest.raises(_lib.RgfmError, match="saved state of this forward_train call is gone"):
        logits.sum().backward()
