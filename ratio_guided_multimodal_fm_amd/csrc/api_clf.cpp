// api_clf.cpp -- the evaluation classifiers' handle and training pass: create / destroy / update_params, the forward
// that keeps what the backward needs (BatchNorm on batch statistics, dropout behind fc1), the backward to the image and
// to every parameter, the fused softmax cross-entropy and the three test hooks (C ABI: include/rgfm.h; kernels:
// block_train.hip behind the convs, clf_train.hip, the convs and the 10-way head of unet_grad.hip and the GEMM of
// fmnet_grad.hip for fc1).
//
// The walk is the reference MNISTClassifier.forward (src/models/classifier.py:38-52), MNISTClassifier32.forward
// (src/models/svhn_classifier.py:101-116) or SVHNClassifier.forward (:49-71) over NCHW tensors in the caller's
// workspace, laid out by plan_ct: first the SAVED state (header, the image, per conv block its BatchNorm input z and
// (mean, rstd) pairs where it has a BatchNorm, the activated (and pooled) map with the pool's choices, fc1's output u
// and its activated, dropped-out map), then the SCRATCH of the backward (the forward keeps a conv output that no
// BatchNorm needs again there too).  The flatten is NCHW order, so fc1 consumes the last map in place.
#include "train_host.h"

struct rgfm_clf {
  rgfm_clf_desc d;
  float* params = nullptr;  // device copy of the state_dict-order blob
  size_t n_params = 0;
  bool bn = false;
  int in_ch = 1, size = 28, hidden = 128, flat = 0;
  struct Conv {
    size_t w, b;            // offsets into the blob
    size_t nw, nb, rm, rv;  // BatchNorm weight, bias, running_mean, running_var (bn only)
    int cin, cout;
    bool pool_after;
  };
  std::vector<Conv> convs;
  size_t f1w, f1b, f2w, f2b;
};

namespace {

constexpr int CLF_CLASSES = 10;

int check_clf_desc(const rgfm_clf_desc* d) {
  if (!d) return fail(RGFM_EINVAL, "null descriptor");
  if (d->kind != RGFM_CLF_MNIST28 && d->kind != RGFM_CLF_MNIST32 && d->kind != RGFM_CLF_SVHN)
    return fail(RGFM_EINVAL, "unknown classifier kind %d", d->kind);
  return RGFM_OK;
}

// Walks the parameter registration order of the module's __init__ and records blob offsets; returns the float count.
size_t plan_clf(const rgfm_clf_desc& d, rgfm_clf* h) {
  rgfm_clf tmp;
  rgfm_clf& o = h ? *h : tmp;
  o.d = d;
  o.bn = d.kind == RGFM_CLF_SVHN;
  o.in_ch = d.kind == RGFM_CLF_SVHN ? 3 : 1;
  o.size = d.kind == RGFM_CLF_MNIST28 ? 28 : 32;
  o.hidden = d.kind == RGFM_CLF_SVHN ? 256 : 128;
  std::vector<std::pair<int, bool>> blocks;  // (channels, max-pool behind)
  if (d.kind == RGFM_CLF_MNIST28) blocks = {{32, true}, {64, true}};
  else if (d.kind == RGFM_CLF_MNIST32) blocks = {{32, true}, {64, true}, {64, false}};
  else blocks = {{32, true}, {64, true}, {128, false}, {128, false}};
  Cursor c;
  o.convs.clear();
  int cin = o.in_ch, S = o.size;
  for (const auto& b : blocks) {
    rgfm_clf::Conv cv{};
    cv.cin = cin, cv.cout = b.first, cv.pool_after = b.second;
    cv.w = c.take((size_t)cv.cout * cin * 9), cv.b = c.take(cv.cout);
    if (o.bn) {
      cv.nw = c.take(cv.cout), cv.nb = c.take(cv.cout), cv.rm = c.take(cv.cout), cv.rv = c.take(cv.cout);
      c.take(1);  // num_batches_tracked
    }
    o.convs.push_back(cv);
    cin = cv.cout;
    if (cv.pool_after) S /= 2;
  }
  o.flat = cin * S * S;
  o.f1w = c.take((size_t)o.hidden * o.flat), o.f1b = c.take(o.hidden);
  o.f2w = c.take((size_t)CLF_CLASSES * o.hidden), o.f2b = c.take(CLF_CLASSES);
  o.n_params = c.off;
  return c.off;
}

struct CPlan {
  std::vector<TrainBlock> convs;
  size_t hdr, img, u, a1, saved;
  size_t G0, G1, part, bnpart, m12, dA;
  size_t total;  // floats
};

// the three GEMMs of fc1
FgGemm fc1_fwd(const rgfm_clf* h, int n) { return fg_gemm_of(n, h->hidden, h->flat, h->flat, h->flat, h->hidden, true); }
FgGemm fc1_dgrad(const rgfm_clf* h, int n) { return fg_gemm_of(n, h->flat, h->hidden, h->hidden, h->flat, h->flat, false); }
FgGemm fc1_wgrad(const rgfm_clf* h, int n) { return fg_gemm_of(h->hidden, h->flat, n, h->hidden, h->flat, h->flat, false); }

int norm_kind(const rgfm_clf* h) { return h->bn ? NORM_BATCH : NORM_NONE; }  // the conv blocks' norm (train_host.h)

// every region starts on a 16-byte boundary of the workspace (the 16-byte accesses of block_train.hip, clf_train.hip and fg_gemm_kernel)
CPlan plan_ct(const rgfm_clf* h, int n) {
  CPlan p;
  Cursor c;
  auto take = [&](size_t k) { return c.take((k + 3) & ~(size_t)3); };
  TrainBlockMax m;
  p.hdr = take(64);
  p.img = take((size_t)n * h->in_ch * h->size * h->size);
  for (const rgfm_clf::Conv& cv : h->convs) {
    TrainBlock r{};
    r.w = cv.w, r.b = cv.b, r.nw = cv.nw, r.nb = cv.nb, r.rm = cv.rm, r.rv = cv.rv, r.C = cv.cout, r.pool = cv.pool_after;
    p.convs.push_back(r);
  }
  p.convs[0].Cin = h->in_ch, p.convs[0].S = h->size, p.convs[0].in = p.img;
  plan_blocks(p.convs, n, take, norm_kind(h), m);
  p.u = take((size_t)n * h->hidden), p.a1 = take((size_t)n * h->hidden);
  p.saved = c.off;
  p.G0 = take(m.mx), p.G1 = take(m.mx);
  const FgGemm g = fc1_fwd(h, n);
  p.part = take(std::max(m.mx_part, (size_t)g.splits * g.M * g.N));
  p.bnpart = take(m.mxC * BT_BN_SLICES * 3);
  p.m12 = take(m.mxC * 2);
  p.dA = take((size_t)n * h->hidden);
  p.total = c.off;
  return p;
}

int check_ct(const rgfm_clf* h, int n, const void* ws, size_t ws_bytes) {
  if (!h || n < 1) return fail(RGFM_EINVAL, "bad argument");
  return check_train_ws(plan_ct(h, n).total * sizeof(float), ws, ws_bytes, 16);
}

}  // namespace

extern "C" int rgfm_clf_param_floats(const rgfm_clf_desc* desc, size_t* n_floats) {
  if (int rc = check_clf_desc(desc)) return rc;
  if (!n_floats) return fail(RGFM_EINVAL, "null output");
  *n_floats = plan_clf(*desc, nullptr);
  return RGFM_OK;
}

extern "C" int rgfm_clf_create(const rgfm_clf_desc* desc, const float* params_dev, size_t n_floats, rgfm_stream_t stream,
                               rgfm_clf** out) {
  if (int rc = check_clf_desc(desc)) return rc;
  if (!params_dev || !out) return fail(RGFM_EINVAL, "null argument");
  if (int rc = ensure_init()) return rc;
  rgfm_clf* h = new rgfm_clf();
  if (plan_clf(*desc, h) != n_floats) {
    const size_t want = h->n_params;
    delete h;
    return fail(RGFM_EINVAL, "parameter blob has %zu floats, architecture needs %zu", n_floats, want);
  }
  if (hipMalloc(&h->params, h->n_params * sizeof(float)) != hipSuccess) {
    delete h;
    return fail(RGFM_ENOMEM, "hipMalloc(params)");
  }
  if (hipMemcpyAsync(h->params, params_dev, n_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
    rgfm_clf_destroy(h);
    return fail(RGFM_EHIP, "hipMemcpyAsync(params)");
  }
  *out = h;
  return RGFM_OK;
}

extern "C" void rgfm_clf_destroy(rgfm_clf* h) {
  if (!h) return;
  if (h->params) (void)hipFree(h->params);
  delete h;
}

extern "C" int rgfm_clf_update_params(rgfm_clf* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream) {
  if (!h || !params_dev) return fail(RGFM_EINVAL, "null argument");
  if (n_floats != h->n_params) return fail(RGFM_EINVAL, "parameter blob has %zu floats, the handle has %zu", n_floats, h->n_params);
  HIP_TRY(hipMemcpyAsync(h->params, params_dev, n_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RGFM_OK;
}

extern "C" int rgfm_clf_train_workspace_bytes(const rgfm_clf* h, int n, size_t* bytes) {
  if (!h || !bytes || n < 1) return fail(RGFM_EINVAL, "bad argument");
  *bytes = plan_ct(h, n).total * sizeof(float);
  return RGFM_OK;
}

extern "C" int rgfm_clf_forward_train(rgfm_clf* h, const float* x, float* logits_out, int n, int training, uint64_t seed,
                                      float p_drop, float* bn_stats_out, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_ct(h, n, ws, ws_bytes)) return rc;
  if (!x || !logits_out) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = check_p_drop(p_drop)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const CPlan p = plan_ct(h, n);
  float* W = (float*)ws;
  const float* P = h->params;
  unsigned* hdr = (unsigned*)(W + p.hdr);
  if (int rc = write_train_header(hdr, training, p_drop, seed, s)) return rc;
  HIP_TRY(hipMemcpyAsync(W + p.img, x, (size_t)n * h->in_ch * h->size * h->size * sizeof(float), hipMemcpyDeviceToDevice, s));
  for (const TrainBlock& r : p.convs) {
    float* z = W + (h->bn ? r.z : p.G0);
    run_fwd(conv_of(P, r, n), W + r.in, z, nullptr, nullptr, s);
    block_tail(BT_RELU, r, norm_kind(h), n, training, z, P, W, p.bnpart, bn_stats_out, s);
  }
  FgGemm g = fc1_fwd(h, n);
  g.a = W + p.convs.back().a, g.b = P + h->f1w, g.bias = P + h->f1b, g.c = W + p.u, g.part = W + p.part;
  launch_fg_gemm(g, false, false, s);
  launch_ct_relu_drop(W + p.u, (size_t)n * h->hidden, hdr, W + p.a1, s);
  launch_ug_linear(W + p.a1, P + h->f2w, P + h->f2b, logits_out, n, h->hidden, CLF_CLASSES, 0, s);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_clf_backward(rgfm_clf* h, const float* dlogits, float* dx_out, float* dparams_out, int n, void* ws,
                                 size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_ct(h, n, ws, ws_bytes)) return rc;
  if (!dlogits || !dparams_out) return fail(RGFM_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const CPlan p = plan_ct(h, n);
  float* W = (float*)ws;
  const float* P = h->params;
  float* D = dparams_out;
  const unsigned* hdr = (const unsigned*)(W + p.hdr);
  if (h->bn) HIP_TRY(hipMemsetAsync(D, 0, h->n_params * sizeof(float), s));  // (the BatchNorm buffers' slots stay zero)
  // fc2, the ReLU + dropout in front of it, fc1
  launch_ug_linear_wgrad(dlogits, W + p.a1, n, h->hidden, CLF_CLASSES, 0, D + h->f2w, D + h->f2b, s);
  launch_ug_linear_dgrad(dlogits, P + h->f2w, n, h->hidden, CLF_CLASSES, W + p.dA, 0, s);
  launch_ct_relu_drop_bwd(W + p.u, W + p.dA, (size_t)n * h->hidden, hdr, s);  // dA = d u
  const float* last = W + p.convs.back().a;
  FgGemm g = fc1_wgrad(h, n);
  g.a = W + p.dA, g.b = last, g.c = D + h->f1w;
  launch_fg_gemm(g, true, true, s);
  launch_ug_colsum(W + p.dA, n, h->hidden, D + h->f1b, s);
  float *cur = W + p.G0, *other = W + p.G1;
  g = fc1_dgrad(h, n);
  g.a = W + p.dA, g.b = P + h->f1w, g.c = cur;
  launch_fg_gemm(g, false, true, s);
  // the conv blocks, backwards.  cur: gradient of the block's output
  for (int i = (int)p.convs.size() - 1; i >= 0; --i) {
    const TrainBlock& r = p.convs[i];
    const float* gate = W + r.a;  // the gate the BatchNorm backward still has to apply, or null
    if (r.pool) {
      launch_bt_unpool(BT_RELU, cur, (const unsigned char*)(W + r.choice), gate, other, n * r.C, r.S, r.S, s);
      std::swap(cur, other);
      gate = nullptr;
    } else if (!h->bn) {
      launch_ct_gate(cur, W + r.a, (size_t)n * r.C * r.S * r.S, s);
    }
    if (h->bn)
      launch_bt_bn_bwd(BT_RELU, norm_act_of(r, NORM_BATCH, n, W + r.z, P, W), cur, gate, hdr + HDR_TRAINING, W + p.bnpart,
                       W + p.m12, D + r.nw, D + r.nb, s);
    block_grads(conv_of(P, r, n), r, W, p.part, D, cur, other, i > 0 ? other : dx_out, s);
  }
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_clf_xent(const float* logits, const int32_t* labels, int n, int classes, float scale,
                             double* loss_rows_out, float* dlogits_out, int32_t* pred_out, rgfm_stream_t stream) {
  if (!logits || !labels || !loss_rows_out || n < 1) return fail(RGFM_EINVAL, "bad argument");
  if (classes < 1 || classes > CT_MAX_CLASSES) return fail(RGFM_EINVAL, "classes must be in 1..%d", CT_MAX_CLASSES);
  if (!cur_dev())  // (the first call on a device: is it a gfx950?)
    if (int rc = ensure_init()) return rc;
  launch_ct_xent(logits, labels, n, classes, scale, loss_rows_out, dlogits_out, pred_out, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_clf_pool_choice(rgfm_clf* h, const void* ws, int layer, int n, float* out) {
  if (!h || !ws || !out || n < 1) return fail(RGFM_EINVAL, "bad argument");
  if (layer < 0 || layer >= (int)h->convs.size() || !h->convs[layer].pool_after)
    return fail(RGFM_EINVAL, "conv block %d has no max-pool", layer);
  const CPlan p = plan_ct(h, n);
  const TrainBlock& r = p.convs[layer];
  launch_bt_choice((const unsigned char*)((const float*)ws + r.choice), (size_t)n * r.C * r.So * r.So, out, nullptr);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_clf_gate(rgfm_clf* h, const void* ws, int layer, int n, float* out) {
  if (!h || !ws || !out || n < 1) return fail(RGFM_EINVAL, "bad argument");
  const int nconv = (int)h->convs.size();
  if (layer < 0 || layer > nconv) return fail(RGFM_EINVAL, "layer %d out of range (%d conv blocks, then fc1)", layer, nconv);
  const CPlan p = plan_ct(h, n);
  const float* W = (const float*)ws;
  if (layer == nconv) launch_ct_gate_out(W + p.u, (size_t)n * h->hidden, out, nullptr);
  else launch_ct_gate_out(W + p.convs[layer].a, (size_t)n * p.convs[layer].C * p.convs[layer].So * p.convs[layer].So, out, nullptr);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_clf_dropout_mask(rgfm_clf* h, uint64_t seed, float p_drop, int n, float* out) {
  if (!h || !out || n < 1) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = check_p_drop(p_drop)) return rc;
  launch_ug_mask(out, (size_t)n * h->hidden, seed, 0, p_drop, nullptr);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
