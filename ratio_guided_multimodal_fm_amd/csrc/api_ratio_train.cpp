// api_ratio_train.cpp -- training pass of the ratio-estimator handle: the forward that keeps what the backward needs
// (BatchNorm on batch statistics, dropout in the score MLP), the backward to both images and to every parameter, and
// the two test hooks (C ABI: include/rgfm.h; kernels: block_train.hip behind the encoders' convs, ratio_train.hip, and
// the conv / Linear kernels of unet_grad.hip).
//
// The walk is the reference RatioEstimatorMNISTSVHN.forward (src/models/ratio_flexible.py:211-364),
// RatioEstimator.forward (src/models/ratio_estimator.py:67-135) or FlexibleRatioEstimator.forward
// (src/models/ratio_flexible.py:42-66, :116-133; the rasters follow the handle's sizes) over NCHW tensors in the caller's workspace, laid out
// by plan_rt: first the SAVED state (header, both images, per conv its input, its output z, the norm's (mean, rstd)
// pairs, the activated (and pooled) map with the pool's choices, the score MLP's pre-norm tensors and row statistics),
// then the backward's SCRATCH.
#include "train_host.h"

namespace {

struct REnc {
  const rgfm_ratio::Encoder* e;
  std::vector<TrainBlock> convs;
  size_t img, pooled, feat;
  int C, S;  // of the last block's output
};
struct RDense {
  const rgfm_ratio::Dense* d;
  size_t in, u, mr, a;
  int block;  // index of the Dropout layer behind it, or -1
};
struct RPlan {
  REnc enc[2];
  std::vector<RDense> dense;
  size_t hdr, cat, saved;
  size_t G0, G1, part, bnpart, m12, pg, pb, dA, dU, dcat, dfeat[2], gpool;
  size_t total;  // floats
};

int norm_kind(const rgfm_ratio* h) { return h->gn_encoders() ? 8 : NORM_BATCH; }  // the encoders' norm (train_host.h)

RPlan plan_rt(const rgfm_ratio* h, int n) {
  RPlan p;
  Cursor c;
  const int F = h->d.feature_dim;
  auto take = [&](size_t k) { return c.take(k); };
  TrainBlockMax m;
  p.hdr = c.take(64);
  const rgfm_ratio::Encoder* encs[2] = {&h->ex, &h->ey};
  for (int k = 0; k < 2; ++k) {
    REnc& e = p.enc[k];
    e.e = encs[k];
    e.img = c.take((size_t)n * e.e->in_ch * e.e->size * e.e->size);
    for (const rgfm_ratio::Conv& cv : e.e->convs) {
      TrainBlock r{};
      r.w = cv.w.w_raw, r.b = cv.w.b, r.nw = cv.nw, r.nb = cv.nb, r.rm = cv.rm, r.rv = cv.rv, r.C = cv.w.cout;
      r.pool = cv.pool_after;
      e.convs.push_back(r);
    }
    e.convs[0].Cin = e.e->in_ch, e.convs[0].S = e.e->size, e.convs[0].in = e.img;
    plan_blocks(e.convs, n, take, norm_kind(h), m);
    e.C = e.convs.back().C, e.S = e.convs.back().So;
    e.pooled = c.take((size_t)n * e.C);
    e.feat = c.take((size_t)n * F);
  }
  p.cat = c.take((size_t)n * 2 * F);
  size_t in = p.cat, width = 2 * (size_t)F;
  for (size_t l = 0; l < h->hidden.size(); ++l) {
    RDense dn{};
    dn.d = &h->hidden[l], dn.in = in, dn.block = l < 2 ? (int)l : -1;  // both estimators: Dropout behind the first two
    dn.u = c.take((size_t)n * dn.d->out);
    dn.mr = c.take((size_t)n * 2);
    dn.a = c.take((size_t)n * dn.d->out);
    width = std::max(width, (size_t)dn.d->out);
    p.dense.push_back(dn);
    in = dn.a;
  }
  p.saved = c.off;
  const size_t mxC = m.mxC;
  p.G0 = c.take(m.mx), p.G1 = c.take(m.mx);
  p.part = c.take(m.mx_part);
  p.bnpart = c.take(mxC * BT_BN_SLICES * 3);
  p.m12 = c.take(mxC * 2);
  p.pg = c.take((size_t)n * std::max(mxC, width)), p.pb = c.take((size_t)n * std::max(mxC, width));
  p.dA = c.take((size_t)n * width), p.dU = c.take((size_t)n * width);
  p.dcat = c.take((size_t)n * 2 * F);
  p.dfeat[0] = c.take((size_t)n * F), p.dfeat[1] = c.take((size_t)n * F);
  p.gpool = c.take((size_t)n * mxC);
  p.total = c.off;
  return p;
}

int check_rt(const rgfm_ratio* h, int n, void* ws, size_t ws_bytes) {
  if (!h || n < 1) return fail(RGFM_EINVAL, "bad argument");
  return check_train_ws(plan_rt(h, n).total * sizeof(float), ws, ws_bytes);
}

}  // namespace

extern "C" int rgfm_ratio_train_workspace_bytes(const rgfm_ratio* h, int n, size_t* bytes) {
  if (!h || !bytes || n < 1) return fail(RGFM_EINVAL, "bad argument");
  *bytes = plan_rt(h, n).total * sizeof(float);
  return RGFM_OK;
}

extern "C" int rgfm_ratio_forward_train(rgfm_ratio* h, const float* x, const float* y, float* score_out, int n,
                                        int training, float p_drop, uint64_t seed, float* bn_stats_out, void* ws,
                                        size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_rt(h, n, ws, ws_bytes)) return rc;
  if (!x || !y || !score_out) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = check_p_drop(p_drop)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const RPlan p = plan_rt(h, n);
  const int F = h->d.feature_dim;
  float* W = (float*)ws;
  const float* P = h->params;
  unsigned* hdr = (unsigned*)(W + p.hdr);
  if (int rc = write_train_header(hdr, training, p_drop, seed, s)) return rc;
  const float* img[2] = {x, y};
  for (int k = 0; k < 2; ++k) {
    const REnc& e = p.enc[k];
    HIP_TRY(hipMemcpyAsync(W + e.img, img[k], (size_t)n * e.e->in_ch * e.e->size * e.e->size * sizeof(float),
                           hipMemcpyDeviceToDevice, s));
    for (const TrainBlock& r : e.convs) {
      run_fwd(conv_of(P, r, n), W + r.in, W + r.z, nullptr, nullptr, s);
      block_tail(BT_SILU, r, norm_kind(h), n, training, W + r.z, P, W, p.bnpart, bn_stats_out, s);
    }
    launch_rt_avgpool(W + e.convs.back().a, n * e.C, e.S * e.S, W + e.pooled, s);
    launch_ug_linear(W + e.pooled, P + e.e->fcw, P + e.e->fcb, W + e.feat, n, e.C, F, 0, s);
  }
  {
    UgAct cat{};  // torch.cat([feat_x, feat_y], dim=1)
    cat.s0 = W + p.enc[0].feat, cat.s1 = W + p.enc[1].feat, cat.C0 = cat.C1 = F, cat.B = n, cat.HW = 1, cat.groups = 1;
    cat.block = -1, cat.out = W + p.cat;
    launch_ug_gn_act(cat, s);
  }
  for (const RDense& dn : p.dense) {
    const auto& d = *dn.d;
    launch_ug_linear(W + dn.in, P + d.w, P + d.b, W + dn.u, n, d.in, d.out, 0, s);
    launch_rt_ln_act(W + dn.u, P + d.lw, P + d.lb, n, d.out, hdr, dn.block, W + dn.mr, W + dn.a, s);
  }
  launch_ug_linear(W + p.dense.back().a, P + h->headw, P + h->headb, score_out, n, h->head_in, 1, 0, s);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_ratio_backward(rgfm_ratio* h, const float* dscore, float* dx_out, float* dy_out, float* dparams_out,
                                   int n, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_rt(h, n, ws, ws_bytes)) return rc;
  if (!dscore || !dparams_out) return fail(RGFM_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const RPlan p = plan_rt(h, n);
  const int F = h->d.feature_dim;
  float* W = (float*)ws;
  const float* P = h->params;
  float* D = dparams_out;
  const unsigned* hdr = (const unsigned*)(W + p.hdr);
  HIP_TRY(hipMemsetAsync(D, 0, h->n_params * sizeof(float), s));  // (the BatchNorm buffers' slots stay zero)
  // score MLP
  launch_ug_linear_wgrad(dscore, W + p.dense.back().a, n, h->head_in, 1, 0, D + h->headw, D + h->headb, s);
  launch_ug_linear_dgrad(dscore, P + h->headw, n, h->head_in, 1, W + p.dA, 0, s);
  for (int l = (int)p.dense.size() - 1; l >= 0; --l) {
    const RDense& dn = p.dense[l];
    const auto& d = *dn.d;
    launch_rt_ln_act_bwd(W + dn.u, W + p.dA, P + d.lw, P + d.lb, n, d.out, hdr, dn.block, W + dn.mr, W + p.dU, W + p.pg,
                         W + p.pb, s);
    launch_ug_colsum(W + p.pg, n, d.out, D + d.lw, s);
    launch_ug_colsum(W + p.pb, n, d.out, D + d.lb, s);
    launch_ug_linear_wgrad(W + p.dU, W + dn.in, n, d.in, d.out, 0, D + d.w, D + d.b, s);
    launch_ug_linear_dgrad(W + p.dU, P + d.w, n, d.in, d.out, W + (l ? p.dA : p.dcat), 0, s);
  }
  HIP_TRY(hipMemsetAsync(W + p.dfeat[0], 0, (size_t)2 * n * F * sizeof(float), s));  // dfeat[0], dfeat[1] are adjacent
  launch_ug_split_add(W + p.dcat, W + p.dfeat[0], W + p.dfeat[1], n, F, F, 1, s);
  float* dimg[2] = {dx_out, dy_out};
  for (int k = 0; k < 2; ++k) {
    const REnc& e = p.enc[k];
    launch_ug_linear_wgrad(W + p.dfeat[k], W + e.pooled, n, e.C, F, 0, D + e.e->fcw, D + e.e->fcb, s);
    launch_ug_linear_dgrad(W + p.dfeat[k], P + e.e->fcw, n, e.C, F, W + p.gpool, 0, s);
    float *cur = W + p.G0, *other = W + p.G1;
    launch_rt_avgpool_bwd(W + p.gpool, n * e.C, e.S * e.S, cur, s);
    for (int i = (int)e.convs.size() - 1; i >= 0; --i) {
      const TrainBlock& r = e.convs[i];
      if (r.pool) {
        launch_bt_unpool(BT_SILU, cur, (const unsigned char*)(W + r.choice), nullptr, other, n * r.C, r.S, r.S, s);
        std::swap(cur, other);
      }
      // cur: gradient of silu(norm(z)) on the conv's raster -> gradient of z
      const BtBlock a = norm_act_of(r, norm_kind(h), n, W + r.z, P, W);
      if (a.groups == 0) {
        launch_bt_bn_bwd(BT_SILU, a, cur, nullptr, hdr + HDR_TRAINING, W + p.bnpart, W + p.m12, D + r.nw, D + r.nb, s);
      } else {
        UgAct g{};
        g.s0 = a.z, g.C0 = r.C, g.B = n, g.HW = r.S * r.S, g.groups = a.groups, g.mr = a.mr, g.gamma = a.gamma, g.beta = a.beta;
        g.block = -1;
        launch_ug_gn_act_bwd(g, cur, other, nullptr, 0, 0, W + p.pg, W + p.pb, s);
        launch_ug_colsum(W + p.pg, n, r.C, D + r.nw, s);
        launch_ug_colsum(W + p.pb, n, r.C, D + r.nb, s);
        std::swap(cur, other);
      }
      block_grads(conv_of(P, r, n), r, W, p.part, D, cur, other, i > 0 ? other : dimg[k], s);
    }
  }
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_ratio_pool_choice(rgfm_ratio* h, const void* ws, int encoder, int pool, int n, float* out) {
  if (!h || !ws || !out || n < 1 || encoder < 0 || encoder > 1 || pool < 0) return fail(RGFM_EINVAL, "bad argument");
  const RPlan p = plan_rt(h, n);
  int seen = 0;
  for (const TrainBlock& r : p.enc[encoder].convs)
    if (r.pool && seen++ == pool) {
      launch_bt_choice((const unsigned char*)((const float*)ws + r.choice), (size_t)n * r.C * r.So * r.So, out, nullptr);
      HIP_TRY(hipGetLastError());
      return RGFM_OK;
    }
  return fail(RGFM_EINVAL, "pool %d out of range (the encoder has %d max-pools)", pool, seen);
}

extern "C" int rgfm_ratio_dropout_mask(rgfm_ratio* h, int block, uint64_t seed, float p_drop, int n, float* out) {
  if (!h || !out || n < 1) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = check_p_drop(p_drop)) return rc;
  if (block < 0 || block > 1) return fail(RGFM_EINVAL, "block %d out of range (the score MLP has 2 Dropout layers)", block);
  launch_ug_mask(out, (size_t)n * h->hidden[block].out, seed, block, p_drop, nullptr);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
