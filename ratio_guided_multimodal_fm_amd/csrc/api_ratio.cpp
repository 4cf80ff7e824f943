// api_ratio.cpp -- ratio estimators: evaluation, gradient of log r, and the gradient-guided paired sampler (C ABI: include/rgfm.h).
#include <optional>

#include "sampler_host.h"

namespace {

// Parameter order of RatioEstimatorMNISTSVHN (src/models/ratio_flexible.py:191-208,
// :241-269, :327-345), RatioEstimator (src/models/ratio_estimator.py:43-65, :121-135) and FlexibleRatioEstimator
// (src/models/ratio_flexible.py:22-40, :100-114; `geom` gives its channels and sizes, unused by the other kinds).
size_t plan_ratio(const rgfm_ratio_desc& d, const rgfm_ratio_flex_desc& geom, rgfm_ratio* h) {
  Planner P;
  Cursor &c = P.raw, &pk = P.pk, bn, gw;
  const int F = d.feature_dim, Hd = d.hidden_dim;
  auto encoder = [&](int in_ch, int size, const std::vector<int>& chans, const std::vector<int>& pools, bool batchnorm) {
    rgfm_ratio::Encoder e;
    e.in_ch = in_ch, e.size = size;
    int ci = in_ch;
    for (size_t i = 0; i < chans.size(); ++i) {
      rgfm_ratio::Conv cv;
      cv.w.cin = ci, cv.w.cout = chans[i], cv.w.taps = 9;
      cv.w.w_raw = c.take((size_t)chans[i] * ci * 9);
      cv.w.b = c.take(chans[i]);
      if (i > 0) {
        cv.w.w_pk = pk.take((size_t)chans[i] * ci * 9);
        cv.wt_pk = gw.take((size_t)chans[i] * ci * 9);
        cv.w.hx = P.image((size_t)chans[i] * ci * 9 * 2);
        cv.wt_h = P.image((size_t)chans[i] * ci * 9 * 2);
      }
      cv.nw = c.take(chans[i]);
      cv.nb = c.take(chans[i]);
      if (batchnorm) {
        cv.rm = c.take(chans[i]);
        cv.rv = c.take(chans[i]);
        c.take(1);  // num_batches_tracked
        cv.bn_scale = bn.take(chans[i]);
        cv.bn_shift = bn.take(chans[i]);
      }
      cv.pool_after = pools[i] != 0;
      e.convs.push_back(cv);
      ci = chans[i];
    }
    e.fc_in = ci;
    e.fcw = c.take((size_t)F * ci);
    e.fcb = c.take(F);
    e.fcw_t = gw.take((size_t)F * ci);
    return e;
  };
  rgfm_ratio::Encoder ex, ey;
  std::vector<int> dims;
  if (d.kind == RGFM_RATIO_MNIST_SVHN) {
    ex = encoder(1, 32, {32, 64, 128, 128}, {1, 1, 1, 0}, true);
    ey = encoder(3, 32, {64, 64, 128, 128, 256, 256, 256, 256}, {0, 1, 0, 1, 0, 1, 0, 1}, true);
    dims = {2 * F, Hd, Hd, Hd / 2};
  } else if (d.kind == RGFM_RATIO_FLEXIBLE) {
    ex = encoder(geom.x_channels, geom.x_size, {32, 64, 128, 128}, {1, 1, 1, 0}, false);
    ey = encoder(geom.y_channels, geom.y_size, {32, 64, 128, 128}, {1, 1, 1, 0}, false);
    dims = {2 * F, Hd, Hd / 2};
  } else {
    ex = encoder(1, 28, {32, 64, 128, 128}, {1, 1, 1, 0}, false);
    ey = encoder(1, 28, {32, 64, 128, 128}, {1, 1, 1, 0}, false);
    dims = {2 * F, Hd, Hd / 2};
  }
  std::vector<rgfm_ratio::Dense> hidden;
  for (size_t l = 0; l + 1 < dims.size(); ++l) {
    rgfm_ratio::Dense dn;
    dn.in = dims[l], dn.out = dims[l + 1];
    dn.w = c.take((size_t)dn.in * dn.out), dn.b = c.take(dn.out);
    dn.w_t = gw.take((size_t)dn.in * dn.out);
    dn.lw = c.take(dn.out), dn.lb = c.take(dn.out);
    hidden.push_back(dn);
  }
  const size_t headw = c.take(dims.back()), headb = c.take(1);
  if (h) {
    h->ex = ex, h->ey = ey, h->hidden = hidden, h->headw = headw, h->headb = headb, h->head_in = dims.back();
    static_cast<WeightLayout&>(*h) = P.layout();
    h->n_bn = bn.off;
    h->w1x = gw.take((size_t)Hd * F), h->w1y = gw.take((size_t)Hd * F);
    h->g_zeros = gw.take(1024);
    h->n_gradw = gw.off;
    h->max_c = 0, h->n_wtmp = 1;
    for (const auto* e : {&h->ex, &h->ey})
      for (size_t i = 0; i < e->convs.size(); ++i) {
        const ConvW& w = e->convs[i].w;
        h->max_c = std::max(h->max_c, w.cout);
        if (i > 0) h->n_wtmp = std::max(h->n_wtmp, (size_t)w.cout * w.cin * 9);
      }
  }
  return c.off;
}

int check_ratio_dims(const rgfm_ratio_desc* d) {
  if (d->feature_dim % 64 || d->hidden_dim % 128 || d->feature_dim > 512 || d->hidden_dim > 1024)
    return fail(RGFM_EINVAL, "feature_dim must be a multiple of 64 (<=512), hidden_dim of 128 (<=1024)");
  if (d->loss_type != RGFM_LOSS_DISC && d->loss_type != RGFM_LOSS_RULSIF) return fail(RGFM_EINVAL, "unknown loss_type");
  return RGFM_OK;
}

int check_ratio_desc(const rgfm_ratio_desc* d) {
  if (!d) return fail(RGFM_EINVAL, "null descriptor");
  if (d->kind == RGFM_RATIO_FLEXIBLE)
    return fail(RGFM_EINVAL, "RGFM_RATIO_FLEXIBLE takes its geometry from rgfm_ratio_flex_desc: use rgfm_ratio_flex_create");
  if (d->kind != RGFM_RATIO_MNIST_SVHN && d->kind != RGFM_RATIO_MNIST28) return fail(RGFM_EINVAL, "unknown ratio kind");
  return check_ratio_dims(d);
}

// Geometry rules of the flexible kind.  Channels 1..4: conv_in stages one float4 per pixel.  Size >= 8: three floor
// 2x2 max-pools must leave a pixel for conv4.  Size <= 64: every raster S, S/2, S/4, S/8 must tile -- make_geom cuts a
// raster into 256-pixel tiles of whole rows, and the convs hold a tile's zero-padded halo (at most 448 pixels) in LDS.
int check_ratio_flex_desc(const rgfm_ratio_flex_desc* f, rgfm_ratio_desc* d) {
  if (!f) return fail(RGFM_EINVAL, "null descriptor");
  d->kind = RGFM_RATIO_FLEXIBLE, d->feature_dim = f->feature_dim, d->hidden_dim = f->hidden_dim, d->loss_type = f->loss_type;
  if (int rc = check_ratio_dims(d)) return rc;
  const int chans[2] = {f->x_channels, f->y_channels}, sizes[2] = {f->x_size, f->y_size};
  const char* cn[2] = {"x_channels", "y_channels"};
  const char* sn[2] = {"x_size", "y_size"};
  for (int k = 0; k < 2; ++k) {
    if (chans[k] < 1 || chans[k] > 4) return fail(RGFM_EINVAL, "%s must be in 1..4, got %d", cn[k], chans[k]);
    if (sizes[k] < 8) return fail(RGFM_EINVAL, "%s must be at least 8 (three 2x2 max-pools), got %d", sn[k], sizes[k]);
    if (sizes[k] > 64) return fail(RGFM_EINVAL, "%s = %d cannot be tiled: at most 64", sn[k], sizes[k]);
    for (int S = sizes[k], l = 0; l < 4; ++l, S /= 2) {
      const TileGeom g = make_geom(S, S);
      if (g.spt * (g.th + 2) * (g.W + 2) > 448)
        return fail(RGFM_EINVAL, "%s = %d cannot be tiled: the %dx%d raster's halo exceeds a tile", sn[k], sizes[k], S, S);
    }
  }
  return RGFM_OK;
}

// BatchNorm encoders inside a gradient-guided sampler loop: conv i stages S_A silu(z) of layer i - 1 raw on the two fp16
// planes (RatioPass::encode), z = gamma (c - mean) / sqrt(var + eps) + beta.  The staging path covers the high side (the
// x net's range flag), but nothing on this path looks at the low side: the producer's epilogue is the BatchNorm, not a
// ConvArgs::small_check.  So, as norm_params_ok does for a GroupNorm in front of a U-Net conv: a layer whose gamma AND
// beta are all below 2^-6 -- its output would sit under the two-plane floor -- takes its reader off the fp16 path here,
// at create / update_params (after read_hx_flags, which recomputes every verdict); that conv then runs the exact fp32
// kernel in the loops.  Only the low side: a large layer is left to the range flag, whose fallback covers the whole call.
// One stream-ordered read of the norm parameters (weight and bias are adjacent in the blob), nothing per launch.
int demote_by_batchnorms(rgfm_ratio* h, hipStream_t s) {
  std::vector<std::vector<float>> host;
  std::vector<HxImage*> readers;
  for (auto* e : {&h->ex, &h->ey})
    for (size_t i = 1; i < e->convs.size(); ++i) {
      const auto& prev = e->convs[i - 1];
      if (prev.nb != prev.nw + (size_t)prev.w.cout) return fail(RGFM_EINVAL, "BatchNorm weight and bias are not adjacent");
      host.emplace_back((size_t)2 * prev.w.cout);
      readers.push_back(&e->convs[i].w.hx);
    }
  size_t k = 0;
  for (auto* e : {&h->ex, &h->ey})
    for (size_t i = 1; i < e->convs.size(); ++i, ++k)
      if (hipMemcpyAsync(host[k].data(), h->params + e->convs[i - 1].nw, host[k].size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess)
        return fail(RGFM_EHIP, "reading the BatchNorm parameters back failed");
  if (hipStreamSynchronize(s) != hipSuccess) return fail(RGFM_EHIP, "reading the BatchNorm parameters back failed");
  for (k = 0; k < host.size(); ++k) {
    float lo = 0.f;
    for (float v : host[k]) lo = std::max(lo, std::fabs(v));
    if (!(lo >= 0.015625f)) readers[k]->ok = false;  // (NaN parameters too)
  }
  return RGFM_OK;
}

// Every derived image of the handle from h->params: the fp32-packed and two-plane conv weights, the folded BatchNorm
// scale/shift, and the transposed weights of the gradient path (dL/d(in) of a 3x3 conv is the conv of dL/d(out) with
// the weights transposed and the taps flipped; of a Linear, the Linear with W^T); then which convs may run on the fp16
// path (synchronises once).  Used by rgfm_ratio_create and, in place, by rgfm_ratio_update_params.
int pack_ratio(rgfm_ratio* h, hipStream_t s) {
  for (const auto* e : {&h->ex, &h->ey})
    for (size_t i = 0; i < e->convs.size(); ++i) {
      const auto& cv = e->convs[i];
      if (i > 0) launch_pack_conv(h->params + cv.w.w_raw, h->packed + cv.w.w_pk, cv.w.cout, cv.w.cin, 9, nt32_of(cv.w.cout), s);
      if (!h->gn_encoders())
        launch_bn_fold(h->params + cv.nw, h->params + cv.nb, h->params + cv.rm, h->params + cv.rv,
                       h->bn + cv.bn_scale, h->bn + cv.bn_shift, cv.w.cout, s);
    }
  for (const auto* e : {&h->ex, &h->ey}) {
    for (size_t i = 1; i < e->convs.size(); ++i) {
      const auto& cv = e->convs[i];
      launch_conv_weight_transpose(h->params + cv.w.w_raw, h->wtmp, cv.w.cout, cv.w.cin, s);
      launch_pack_conv(h->wtmp, h->gradw + cv.wt_pk, cv.w.cin, cv.w.cout, 9, nt32_of(cv.w.cin), s);
      launch_pack_conv_hx2(h->wtmp, h->packedh + cv.wt_h.off, h->hq + 4 * cv.wt_h.hq, cv.w.cin, cv.w.cout, 9, CONV_S1, s);
    }
    launch_transpose2d(h->params + e->fcw, h->gradw + e->fcw_t, h->d.feature_dim, e->fc_in, s);
  }
  for (const auto& dn : h->hidden) launch_transpose2d(h->params + dn.w, h->gradw + dn.w_t, dn.out, dn.in, s);
  {  // the cross path's column slices W[:, :F] and W[:, F:] of the first score Linear, each made contiguous
    const size_t F = (size_t)h->d.feature_dim, Hd = (size_t)h->hidden[0].out;
    const float* w1 = h->params + h->hidden[0].w;
    HIP_TRY(hipMemcpy2DAsync(h->gradw + h->w1x, F * 4, w1, 2 * F * 4, F * 4, Hd, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpy2DAsync(h->gradw + h->w1y, F * 4, w1 + F, 2 * F * 4, F * 4, Hd, hipMemcpyDeviceToDevice, s));
  }
  launch_fill(h->gradw + h->g_zeros, 0.f, 1024, s);
  std::vector<HxImage*> images;
  for (auto* e : {&h->ex, &h->ey})
    for (size_t i = 1; i < e->convs.size(); ++i) {
      ConvW& w = e->convs[i].w;
      launch_pack_conv_hx2(h->params + w.w_raw, h->packedh + w.hx.off, h->hq + 4 * w.hx.hq, w.cout, w.cin, 9, CONV_S1, s);
      images.push_back(&w.hx);
      images.push_back(&e->convs[i].wt_h);
    }
  if (int rc = read_hx_flags(*h, images, s)) return rc;
  return h->gn_encoders() ? RGFM_OK : demote_by_batchnorms(h, s);
}

// pairs per chunk of the cross evaluation: 32 MB of first-layer activations at hidden_dim 512, 64 MB at the largest, 1024
constexpr long long RGFM_CROSS_ROWS_DEFAULT = 16384;
inline long long cross_rows() {  // RGFM_CROSS_ROWS: test hook, read on entry of the two cross entry points
  const char* e = getenv("RGFM_CROSS_ROWS");
  const long long v = e ? atoll(e) : 0;
  return v >= 1 && v <= (1 << 20) ? v : RGFM_CROSS_ROWS_DEFAULT;
}

// what a conv of the encoder walk leaves for the reverse pass
struct Kept {
  float* z;  // its pre-activation (GroupNorm kinds: the conv output; BatchNorm kind: the BatchNorm output)
  int C, S;
  bool pooled;
  float* ab = nullptr;  // GroupNorm encoders: the samples' scale/shift pairs [n][C][2] ...
  float* mr = nullptr;  // ... and (mean, rstd) of every group [n][8][2]
};

// One pass over an estimator handle: n rows, buffers carved from `ws`, launches on `s`; dry = carve only.  Every entry
// point is a member, run dry for its *_workspace_bytes figure and live for the call (ratio_call below, and the carves
// of the two gradient-guided loops).
struct RatioPass {
  rgfm_ratio* h;
  int n;
  Bump* ws;
  hipStream_t s;
  bool dry;
  // the range-flag word of the U-Net handle whose sampler loop this pass belongs to, or null (stand-alone gradient:
  // exact fp32 convs).  With it the encoders' forward convs follow that handle's conv arithmetic (g_modes, set by the
  // caller's ModeScope) and raise ITS flag, so that the sampler's range guard and fallback cover them.
  unsigned* flag = nullptr;
  float* ab1 = nullptr;  // [n][max_c][2] identity scale/shift: "SiLU on load"
  unsigned* amax = nullptr;  // one word per reverse conv: bits of max |gradient| of its input (ConvArgs::in_amax); zeroed per call
  int amax_used = 0;

  RatioPass rows(int m) const {  // the same pass over m rows
    RatioPass p = *this;
    p.n = m;
    return p;
  }

  // One encoder forward (the ImageEncoder of ratio_estimator.py:67-93 / ratio_flexible.py:42-66 and the two BatchNorm
  // encoders of RatioEstimatorMNISTSVHN): image NCHW -> features written at feat[:, col0 : col0+F] (row stride `stride`).
  // kept == null, inference: a GroupNorm conv writes its partial statistics, gn_finalize turns them into the scale/shift
  // pairs that the max-pool / average pool behind it applies with SiLU; a BatchNorm conv applies the folded scale/shift
  // and SiLU in its epilogue.
  // kept != null, the forward of a gradient pass: the same launches with every pre-activation kept, one Kept per conv.
  // GroupNorm: the finalize also writes (mean, rstd).  BatchNorm: the epilogue stores z instead of silu(z) (ep_nosilu)
  // and whoever reads z applies SiLU on load through the identity pairs ab1 (begin_grad); inside a sampler loop (`flag`)
  // these convs are offered the two-plane fp16 image of their weights.
  void encode(const rgfm_ratio::Encoder& e, const float* img, float* feat, int col0, int stride, std::vector<Kept>* kept) {
    const bool gn = h->gn_encoders(), keep_z = kept && !gn;
    const int F = h->d.feature_dim;
    int S = e.size, curC = e.in_ch;
    const float* cur = nullptr;  // input of the next conv
    const float* act = nullptr;  // ... and the scale/shift pairs its reader applies with SiLU, or null: `cur` is final
    for (size_t i = 0; i < e.convs.size(); ++i) {
      const rgfm_ratio::Conv& cv = e.convs[i];
      const TileGeom g = make_geom(S, S);
      const int C = cv.w.cout;
      float* z = ws->f((size_t)n * S * S * C);
      float* stats = gn ? ws->f((size_t)n * g.nparts * C * 2) : nullptr;
      float* ab = gn ? ws->f((size_t)n * C * 2) : nullptr;
      float* mr = gn && kept ? ws->f((size_t)n * 8 * 2) : nullptr;
      if (!dry) {
        const float* es = gn ? nullptr : h->bn + cv.bn_scale;
        const float* eh = gn ? nullptr : h->bn + cv.bn_shift;
        if (i == 0) {
          ConvInArgs ci{};
          ci.x = img, ci.w = h->params + cv.w.w_raw, ci.bias = h->params + cv.w.b;
          ci.ep_scale = es, ci.ep_shift = eh, ci.ep_nosilu = keep_z;
          ci.out = z, ci.stats_out = stats, ci.B = n, ci.C0 = C, ci.g = g;
          ProfScope p(RGFM_KCLASS_OTHER, 0, s);
          launch_conv_in(ci, e.in_ch, s);
        } else {
          ConvArgs c{};
          c.in0 = cur, c.C0 = curC, c.Hin = c.Win = S, c.ab = act;
          c.wpk = h->packed + cv.w.w_pk, c.bias = h->params + cv.w.b;
          c.ep_scale = es, c.ep_shift = eh, c.ep_nosilu = keep_z;
          c.out = z, c.stats_out = stats, c.B = n, c.Cout = C, c.g = g;
          c.halo_px = g.spt * (g.th + 2) * (g.W + 2);
          // (fp16 two-plane conv with the BatchNorm epilogue, any of its pipelined forms; without the image conv_route
          // ends at the fp32 MFMA kernel)
          if (keep_z && flag && g_modes.conv == CONV_ARITH_HX2 && cv.w.hx.ok)
            c.wpkh = h->packedh + cv.w.hx.off, c.hq = h->hq + 4 * cv.w.hx.hq, c.range_flag = flag;
          ProfScope p(RGFM_KCLASS_CONV_MFMA, conv_flops(n, S * S, C, 9 * curC), s);
          launch_conv(c, CONV_S1, s);
        }
        if (gn) {
          GnFinalizeArgs f{};
          f.stats0 = stats, f.C0 = C, f.groups = 8;
          f.gamma = h->params + cv.nw, f.beta = h->params + cv.nb, f.ab = ab, f.mr = mr, f.B = n, f.g = g;
          ProfScope p(RGFM_KCLASS_OTHER, 0, s);
          launch_gn_finalize(f, s);
        }
      }
      if (kept) kept->push_back({z, C, S, cv.pool_after, ab, mr});
      cur = z, curC = C, act = gn ? ab : keep_z ? ab1 : nullptr;
      if (cv.pool_after) {
        float* pl = ws->f((size_t)n * (S / 2) * (S / 2) * C);
        if (!dry) {
          ProfScope p(RGFM_KCLASS_OTHER, 0, s);
          launch_pool2(z, act, pl, n, S, S, C, s);
        }
        cur = pl, act = nullptr, S /= 2;
      }
    }
    float* pooled = ws->f((size_t)n * curC);
    if (!dry) {
      ProfScope p(RGFM_KCLASS_OTHER, 0, s);
      launch_avgpool(cur, act, pooled, n, S * S, curC, s);
      launch_linear_mfma(pooled, h->params + e.fcw, h->params + e.fcb, feat + col0, n, curC, F, curC, stride, s);
    }
  }

  // reverse pass of one encoder: gfeat [n][stride] (columns col0 .. col0+F) -> gimg NCHW
  void encode_bwd(const rgfm_ratio::Encoder& e, const std::vector<Kept>& kept, const float* gfeat, int col0, int stride, float* gimg) {
    const int F = h->d.feature_dim;
    const float* zeros = h->gradw + h->g_zeros;
    const Kept& last = kept.back();
    float* g = ws->f((size_t)n * last.C);  // gradient of the average-pooled vector
    if (!dry) launch_linear_mfma(gfeat + col0, h->gradw + e.fcw_t, zeros, g, n, F, last.C, stride, last.C, s);
    int mode = 2;  // first step: g is [n][C] behind the global average pool
    for (int i = (int)kept.size() - 1; i >= 0; --i) {
      const Kept& k = kept[i];
      const rgfm_ratio::Conv& cv = e.convs[i];
      if (i != (int)kept.size() - 1) mode = k.pooled ? 1 : 0;
      else mode = k.pooled ? 3 : 2;  // (SVHN encoder: a max-pool sits between the last conv and the average pool)
      float* gz = ws->f((size_t)n * k.S * k.S * k.C);
      unsigned* am = nullptr;
      if (!dry) {
        if (k.ab) {  // GroupNorm encoder: SiLU' (and the max-pool routing) at u = a z + b, then the norm's backward in place
          launch_grad_act_gn(g, k.z, k.ab, gz, n, k.S, k.C, mode, s);
          launch_gn_bwd(gz, k.z, h->params + cv.nw, k.mr, n, k.S * k.S, k.C, 8, s);
        } else {
          // (inside the sampler the next conv runs on the two-plane arithmetic: it needs the tensor's magnitude)
          am = (flag && i > 0 && amax && g_modes.conv == CONV_ARITH_HX2 && g_modes.rev_hx2 && cv.wt_h.ok) ? amax + amax_used++ : nullptr;
          launch_grad_act(g, k.z, h->bn + cv.bn_scale, gz, n, k.S, k.C, mode, s, am);
        }
      }
      if (i == 0) {
        if (!dry) launch_conv_bwd_img(gz, h->params + cv.w.w_raw, gimg, n, k.S, k.C, e.in_ch, s);
      } else {
        float* gin = ws->f((size_t)n * k.S * k.S * cv.w.cin);
        if (!dry) {
          ConvArgs c{};
          c.in0 = gz, c.C0 = k.C, c.Hin = c.Win = k.S;
          c.wpk = h->gradw + cv.wt_pk, c.bias = zeros;
          c.out = gin, c.stats_out = nullptr, c.B = n, c.Cout = cv.w.cin;
          c.g = make_geom(k.S, k.S);
          c.halo_px = c.g.spt * (c.g.th + 2) * (c.g.W + 2);
          // Inside the gradient-guided sampler (flag set): the data gradient on the two-plane fp16 arithmetic.  Gradients
          // are far from 1 in magnitude -- typically 1e-3 ... 1e-6, below the raw staging window -- so the conv stages
          // them x 2^-e for the tensor's measured maximum f 2^e (grad_act wrote its bits) and scales its outputs back;
          // the staged values are then <= 16 and the x net's range flag covers the rest.  The pre-scale is a power of
          // two, so the result scales exactly with the gradient: tests/test_gpu_grad_loop.py holds the in-loop
          // gradient to 1e-4 of its maximum against float64 for image gradients of 6.5e-10 ... 17 in magnitude (the same
          // relative error at every magnitude).  Otherwise (stand-alone gradient, fallback modes,
          // weights outside the fp16 window): the exact fp32 matrix-core conv.
          bool hx = false;
          if (am) {
            c.wpkh = h->packedh + cv.wt_h.off, c.hq = h->hq + 4 * cv.wt_h.hq, c.range_flag = flag, c.in_amax = am;
            hx = conv_hx2_supported(c, CONV_S1);
          }
          if (hx) launch_conv_hx2(c, CONV_S1, s);
          else launch_conv_mfma(c, CONV_S1, s);
        }
        g = gin;
      }
    }
  }

  // Hidden layers first .. last of the score MLP forward from `cur`: buffers of n rows, launches over rows <= n of them.
  // us == null: Linear, then LayerNorm + SiLU in place (`scoped`: under the launch timers, one scope per layer).
  // us != null, the forward of a gradient pass: each Linear's output u is kept (appended to *us) and a copy normalised.
  // Returns the last activation.
  float* mlp_fwd(size_t first, float* cur, int rows, std::vector<float*>* us, bool scoped = false) {
    for (size_t l = first; l < h->hidden.size(); ++l) {
      const auto& dn = h->hidden[l];
      float* u = ws->f((size_t)n * dn.out);
      float* a = us ? ws->f((size_t)n * dn.out) : u;
      if (!dry) {
        std::optional<ProfScope> p;
        if (scoped) p.emplace(RGFM_KCLASS_OTHER, 0, s);
        launch_linear_mfma(cur, h->params + dn.w, h->params + dn.b, u, rows, dn.in, dn.out, dn.in, dn.out, s);
        if (us) (void)hipMemcpyAsync(a, u, (size_t)rows * dn.out * sizeof(float), hipMemcpyDeviceToDevice, s);
        launch_layernorm_silu(a, h->params + dn.lw, h->params + dn.lb, rows, dn.out, s);
      }
      if (us) us->push_back(u);
      cur = a;
    }
    return cur;
  }

  void head(const float* a, float* out, int rows, int what) {
    launch_ratio_head(a, h->params + h->headw, h->params + h->headb, out, rows, h->head_in, h->d.loss_type, what, s);
  }

  // The head on the last activation `a`, its backward (writes log_ratio when asked) and the hidden layers in reverse
  // over their kept outputs `us`.  Layer 0 gives the gradient of `in0` of its input columns, those whose rows of the
  // transposed weight start at row `row0` (rows of W^T are contiguous): all 2F from 0, or one side's F.  Returns it, [n][in0].
  float* mlp_bwd(const float* a, const std::vector<float*>& us, int in0, int row0, float* log_ratio) {
    const float* zeros = h->gradw + h->g_zeros;
    float* score = ws->f(n);
    float* g = ws->f((size_t)n * h->head_in);
    if (!dry) {
      head(a, score, n, 0);
      launch_ratio_head_bwd(score, h->params + h->headw, g, log_ratio, n, h->head_in, h->d.loss_type, s);
    }
    for (int l = (int)h->hidden.size() - 1; l >= 0; --l) {
      const auto& dn = h->hidden[l];
      const int in = l ? dn.in : in0;
      const float* wt = h->gradw + dn.w_t + (l ? 0 : (size_t)row0 * dn.out);
      float* gu = ws->f((size_t)n * dn.out);
      float* gi = ws->f((size_t)n * in);
      if (!dry) {
        launch_layernorm_silu_bwd(us[l], g, h->params + dn.lw, h->params + dn.lb, gu, n, dn.out, s);
        launch_linear_mfma(gu, wt, zeros, gi, n, dn.out, in, dn.out, in, s);
      }
      g = gi;
    }
    return g;
  }

  // ---- the entry points
  void eval(const float* x, const float* y, float* out, int what) {
    const int F = h->d.feature_dim;
    float* feat = ws->f((size_t)n * 2 * F);
    encode(h->ex, x, feat, 0, 2 * F, nullptr);
    encode(h->ey, y, feat, F, 2 * F, nullptr);
    const float* a = mlp_fwd(0, feat, n, nullptr, true);
    if (!dry) {
      ProfScope p(RGFM_KCLASS_OTHER, 0, s);
      head(a, out, n, what);
    }
  }

  // Cross evaluation: `what` of every pair (x_i, y_j), out[nx][ny].  Each encoder runs once over its own images; the
  // first score Linear is factorised over the concatenation (cross_ln_silu_kernel) and the rest of the MLP runs over the
  // nx * ny pairs in chunks of `chunk` pair indices, so the scratch does not grow with the matrix.
  void cross(const float* x, int nx, const float* y, int ny, float* out, int what, long long chunk) {
    const int F = h->d.feature_dim;
    const auto& d0 = h->hidden[0];
    float* fx = ws->f((size_t)nx * F);
    float* fy = ws->f((size_t)ny * F);
    float* ux = ws->f((size_t)nx * d0.out);
    float* uy = ws->f((size_t)ny * d0.out);
    // the encoders' scratch is dead once the features are written: the two walks and the MLP chunk share one region
    const size_t mark = ws->off;
    size_t peak = mark;
    rows(nx).encode(h->ex, x, fx, 0, F, nullptr);
    peak = std::max(peak, ws->off), ws->off = mark;
    rows(ny).encode(h->ey, y, fy, 0, F, nullptr);
    peak = std::max(peak, ws->off), ws->off = mark;
    const long long total = (long long)nx * ny;
    RatioPass mlp = rows((int)std::min(total, chunk));
    std::optional<ProfScope> p;
    if (!dry) {
      p.emplace(RGFM_KCLASS_OTHER, 0, s);
      const float* zeros = h->gradw + h->g_zeros;
      launch_linear_mfma(fx, h->gradw + h->w1x, zeros, ux, nx, F, d0.out, F, d0.out, s);
      launch_linear_mfma(fy, h->gradw + h->w1y, zeros, uy, ny, F, d0.out, F, d0.out, s);
    }
    for (long long r0 = 0; r0 < total; r0 += chunk) {
      const int m = (int)std::min(chunk, total - r0);
      ws->off = mark;  // (every chunk in the buffers of the first, the largest)
      float* a0 = ws->f((size_t)mlp.n * d0.out);
      if (!dry) launch_cross_ln_silu(ux, uy, h->params + d0.b, h->params + d0.lw, h->params + d0.lb, a0, r0, m, ny, d0.out, s);
      const float* a = mlp.mlp_fwd(1, a0, m, nullptr);
      if (dry) break;
      head(a, out + r0, m, what);
    }
    ws->off = std::max(peak, ws->off);
  }

  // ctx [n][Hd] = W[:, given slice] f_given(cond) + b of the first score Linear: the given side's encoder once (as the
  // cross path runs it) and one linear_mfma on the contiguous column slice pack_ratio keeps.
  void cond_prepare(const float* cond, int given, float* ctx) {
    const int F = h->d.feature_dim;
    const auto& d0 = h->hidden[0];
    float* feat = ws->f((size_t)n * F);
    encode(given ? h->ey : h->ex, cond, feat, 0, F, nullptr);
    if (dry) return;
    ProfScope p(RGFM_KCLASS_OTHER, 0, s);
    launch_linear_mfma(feat, h->gradw + (given ? h->w1y : h->w1x), h->params + d0.b, ctx, n, F, d0.out, F, d0.out, s);
  }

  // ---- gradient of log r.  The forward with every pre-activation kept (encode with `kept`, mlp_fwd
  // with `us`: same kernels as inference), then the reverse pass down to the images: ratio_grad.hip, linear_mfma with
  // W^T, conv_mfma with the transposed weights (dL/d(in) of a 3x3 conv: pack_ratio).
  void begin_grad() {
    ab1 = ws->f((size_t)n * h->max_c * 2);
    amax = ws->u(64);
    amax_used = 0;
    if (!dry) {
      launch_fill_ab_identity(ab1, (size_t)n * h->max_c, s);
      (void)hipMemsetAsync(amax, 0, 64 * sizeof(unsigned), s);
    }
  }

  void grad(const float* x, const float* y, float* gx, float* gy, float* log_ratio) {
    const int F = h->d.feature_dim;
    begin_grad();
    float* feat = ws->f((size_t)n * 2 * F);
    std::vector<Kept> kx, ky;
    encode(h->ex, x, feat, 0, 2 * F, &kx);
    encode(h->ey, y, feat, F, 2 * F, &ky);
    std::vector<float*> us;
    const float* a = mlp_fwd(0, feat, n, &us);
    const float* g = mlp_bwd(a, us, 2 * F, 0, log_ratio);
    encode_bwd(h->ex, kx, g, 0, 2 * F, gx);
    encode_bwd(h->ey, ky, g, F, 2 * F, gy);
  }

  // One side only (conditional sampling): d log_ratio / d target with the other side's share of the first score Linear,
  // ctx [n][Hd] = W[:, given slice] f_given + b (cond_prepare), held fixed.  Only the target's encoder runs, forward
  // and reverse; the first hidden layer is u = ctx + W[:, target slice] f_target (cond_ln_silu_kernel), and its input
  // gradient is taken for the target's F columns alone.
  void grad_cond(const float* ctx, int given, const float* target, float* g_target, float* log_ratio) {
    const int F = h->d.feature_dim;
    const auto& d0 = h->hidden[0];
    begin_grad();
    const rgfm_ratio::Encoder& e = given ? h->ex : h->ey;
    float* feat = ws->f((size_t)n * F);
    std::vector<Kept> kt;
    encode(e, target, feat, 0, F, &kt);
    float* u = ws->f((size_t)n * d0.out);
    float* a0 = ws->f((size_t)n * d0.out);
    float* ut = ws->f((size_t)n * d0.out);
    if (!dry) {
      launch_linear_mfma(feat, h->gradw + (given ? h->w1x : h->w1y), h->gradw + h->g_zeros, ut, n, F, d0.out, F, d0.out, s);
      launch_cond_ln_silu(ctx, ut, h->params + d0.lw, h->params + d0.lb, u, a0, n, d0.out, s);
    }
    std::vector<float*> us{u};
    const float* a = mlp_fwd(1, a0, n, &us);
    const float* g = mlp_bwd(a, us, F, given ? 0 : F, log_ratio);
    encode_bwd(e, kt, g, 0, F, g_target);
  }
};

// A stand-alone entry point is its own argument checks and one of these around its body, a member call on the pass.
// Run dry over an empty Bump, the body's end offset is the *_workspace_bytes figure; the call computes the same figure,
// refuses a smaller workspace before anything is launched, and runs the same body over the caller's workspace.
template <class Body>
size_t ratio_bytes(const rgfm_ratio* h, int n, Body&& body) {
  Bump b;
  RatioPass p{const_cast<rgfm_ratio*>(h), n, &b, nullptr, true};
  body(p);
  return b.off;
}
template <class Body>
int ratio_call(rgfm_ratio* h, int n, void* ws, size_t ws_bytes, rgfm_stream_t stream, Body&& body) {
  const size_t need = ratio_bytes(h, n, body);
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  refresh_modes();
  Bump b(ws, ws_bytes);
  RatioPass p{h, n, &b, (hipStream_t)stream, false};
  body(p);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

}  // namespace

extern "C" int rgfm_ratio_param_floats(const rgfm_ratio_desc* desc, size_t* n_floats) {
  int rc = check_ratio_desc(desc);
  if (rc) return rc;
  if (!n_floats) return fail(RGFM_EINVAL, "null output");
  *n_floats = plan_ratio(*desc, rgfm_ratio_flex_desc{}, nullptr);
  return RGFM_OK;
}

extern "C" int rgfm_ratio_flex_param_floats(const rgfm_ratio_flex_desc* desc, size_t* n_floats) {
  rgfm_ratio_desc d{};
  int rc = check_ratio_flex_desc(desc, &d);
  if (rc) return rc;
  if (!n_floats) return fail(RGFM_EINVAL, "null output");
  *n_floats = plan_ratio(d, *desc, nullptr);
  return RGFM_OK;
}

namespace {
int create_ratio(const rgfm_ratio_desc& d, const rgfm_ratio_flex_desc& geom, const float* params_dev, size_t n_floats,
                 rgfm_stream_t stream, rgfm_ratio** out) {
  int rc;
  if (!params_dev || !out) return fail(RGFM_EINVAL, "null argument");
  if ((rc = ensure_init())) return rc;
  hipStream_t s = (hipStream_t)stream;
  rgfm_ratio* h = new rgfm_ratio();
  h->d = d, h->geom = geom;
  if (plan_ratio(d, geom, h) != n_floats) {
    const size_t want = h->n_params;
    delete h;
    return fail(RGFM_EINVAL, "parameter blob has %zu floats, architecture needs %zu", n_floats, want);
  }
  auto bail = [&](int code, const char* what) {
    rgfm_ratio_destroy(h);
    return fail(code, "%s", what);
  };
  if ((rc = h->alloc(params_dev, false, s))) return rgfm_ratio_destroy(h), rc;
  if (hipMalloc(&h->bn, (h->n_bn + 4) * sizeof(float)) != hipSuccess) return bail(RGFM_ENOMEM, "hipMalloc(bn)");
  if (hipMalloc(&h->gradw, (h->n_gradw + 4) * sizeof(float)) != hipSuccess) return bail(RGFM_ENOMEM, "hipMalloc(gradw)");
  if (hipMalloc(&h->wtmp, h->n_wtmp * sizeof(float)) != hipSuccess) return bail(RGFM_ENOMEM, "hipMalloc(tmp)");
  if ((rc = pack_ratio(h, s))) return rgfm_ratio_destroy(h), rc;
  *out = h;
  return RGFM_OK;
}
}  // namespace

extern "C" int rgfm_ratio_create(const rgfm_ratio_desc* desc, const float* params_dev, size_t n_floats,
                                 rgfm_stream_t stream, rgfm_ratio** out) {
  if (int rc = check_ratio_desc(desc)) return rc;
  return create_ratio(*desc, rgfm_ratio_flex_desc{}, params_dev, n_floats, stream, out);
}

extern "C" int rgfm_ratio_flex_create(const rgfm_ratio_flex_desc* desc, const float* params_dev, size_t n_floats,
                                      rgfm_stream_t stream, rgfm_ratio** out) {
  rgfm_ratio_desc d{};
  if (int rc = check_ratio_flex_desc(desc, &d)) return rc;
  return create_ratio(d, *desc, params_dev, n_floats, stream, out);
}

extern "C" void rgfm_ratio_destroy(rgfm_ratio* h) {
  if (!h) return;
  h->free();
  if (h->bn) (void)hipFree(h->bn);
  if (h->gradw) (void)hipFree(h->gradw);
  if (h->wtmp) (void)hipFree(h->wtmp);
  delete h;
}

extern "C" int rgfm_ratio_update_params(rgfm_ratio* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream) {
  if (!h || !params_dev) return fail(RGFM_EINVAL, "null argument");
  if (n_floats != h->n_params) return fail(RGFM_EINVAL, "parameter blob has %zu floats, the handle has %zu", n_floats, h->n_params);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(h->params, params_dev, n_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
  return pack_ratio(h, s);
}

namespace {
int bad_unless(bool ok) { return ok ? RGFM_OK : fail(RGFM_EINVAL, "bad argument"); }
int check_what(int what) { return what >= 0 && what <= 2 ? RGFM_OK : fail(RGFM_EINVAL, "bad output selector"); }
int check_given(int given) { return given == 0 || given == 1 ? RGFM_OK : fail(RGFM_EINVAL, "given must be 0 (the condition is x) or 1 (y)"); }
}  // namespace

extern "C" int rgfm_ratio_workspace_bytes(const rgfm_ratio* h, int n, size_t* bytes) {
  if (int rc = bad_unless(h && bytes && n >= 1)) return rc;
  *bytes = ratio_bytes(h, n, [](RatioPass& p) { p.eval(nullptr, nullptr, nullptr, 0); });
  return RGFM_OK;
}

extern "C" int rgfm_ratio_eval(rgfm_ratio* h, const float* x, const float* y, float* out, int n, int what,
                               void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!h || !x || !y || !out || !ws) return fail(RGFM_EINVAL, "null argument");
  int rc = check_what(what);
  if (rc || (rc = bad_unless(n >= 1))) return rc;
  return ratio_call(h, n, ws, ws_bytes, stream, [&](RatioPass& p) { p.eval(x, y, out, what); });
}

extern "C" int rgfm_ratio_cross_workspace_bytes(const rgfm_ratio* h, int nx, int ny, size_t* bytes) {
  const long long chunk = cross_rows();
  if (int rc = bad_unless(h && bytes && nx >= 1 && ny >= 1)) return rc;
  *bytes = ratio_bytes(h, 0, [&](RatioPass& p) { p.cross(nullptr, nx, nullptr, ny, nullptr, 0, chunk); });
  return RGFM_OK;
}

extern "C" int rgfm_ratio_eval_cross(rgfm_ratio* h, const float* x, int nx, const float* y, int ny, float* out, int what,
                                     void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  const long long chunk = cross_rows();
  if (!h || !x || !y || !out || !ws) return fail(RGFM_EINVAL, "null argument");
  int rc = check_what(what);
  if (rc || (rc = bad_unless(nx >= 1 && ny >= 1))) return rc;
  return ratio_call(h, 0, ws, ws_bytes, stream, [&](RatioPass& p) { p.cross(x, nx, y, ny, out, what, chunk); });
}

extern "C" int rgfm_ratio_grad_workspace_bytes(const rgfm_ratio* h, int n, size_t* bytes) {
  if (int rc = bad_unless(h && bytes && n >= 1)) return rc;
  *bytes = ratio_bytes(h, n, [](RatioPass& p) { p.grad(nullptr, nullptr, nullptr, nullptr, nullptr); });
  return RGFM_OK;
}

extern "C" int rgfm_ratio_grad_log_ratio(rgfm_ratio* h, const float* x, const float* y, float* gx, float* gy,
                                         float* log_ratio_out, int n, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!h || !x || !y || !gx || !gy || !ws) return fail(RGFM_EINVAL, "null argument");
  if (int rc = bad_unless(n >= 1)) return rc;
  return ratio_call(h, n, ws, ws_bytes, stream, [&](RatioPass& p) { p.grad(x, y, gx, gy, log_ratio_out); });
}

// the one-sided forms (conditional sampling): the given side's context once, then the gradient for the other side
extern "C" int rgfm_ratio_cond_prepare_workspace_bytes(const rgfm_ratio* h, int given, int n, size_t* bytes) {
  int rc = bad_unless(h && bytes && n >= 1);
  if (rc || (rc = check_given(given))) return rc;
  *bytes = ratio_bytes(h, n, [&](RatioPass& p) { p.cond_prepare(nullptr, given, nullptr); });
  return RGFM_OK;
}

extern "C" int rgfm_ratio_cond_prepare(rgfm_ratio* h, const float* cond, int given, int n, float* ctx_out, void* ws,
                                       size_t ws_bytes, rgfm_stream_t stream) {
  if (!h || !cond || !ctx_out || !ws) return fail(RGFM_EINVAL, "null argument");
  int rc = bad_unless(n >= 1);
  if (rc || (rc = check_given(given))) return rc;
  return ratio_call(h, n, ws, ws_bytes, stream, [&](RatioPass& p) { p.cond_prepare(cond, given, ctx_out); });
}

extern "C" int rgfm_ratio_grad_cond_workspace_bytes(const rgfm_ratio* h, int given, int n, size_t* bytes) {
  int rc = bad_unless(h && bytes && n >= 1);
  if (rc || (rc = check_given(given))) return rc;
  *bytes = ratio_bytes(h, n, [&](RatioPass& p) { p.grad_cond(nullptr, given, nullptr, nullptr, nullptr); });
  return RGFM_OK;
}

extern "C" int rgfm_ratio_grad_log_ratio_cond(rgfm_ratio* h, const float* ctx, int given, const float* target, float* g_target,
                                              float* log_ratio_out, int n, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!h || !ctx || !target || !g_target || !ws) return fail(RGFM_EINVAL, "null argument");
  int rc = bad_unless(n >= 1);
  if (rc || (rc = check_given(given))) return rc;
  return ratio_call(h, n, ws, ws_bytes, stream, [&](RatioPass& p) { p.grad_cond(ctx, given, target, g_target, log_ratio_out); });
}

namespace {

// (channels, size) of the estimator's x (side 0) or y (side 1) images
void ratio_side_shape(const rgfm_ratio* hr, int side, int* c, int* sz) {
  if (hr->d.kind == RGFM_RATIO_FLEXIBLE) *c = side ? hr->geom.y_channels : hr->geom.x_channels, *sz = side ? hr->geom.y_size : hr->geom.x_size;
  else if (hr->d.kind == RGFM_RATIO_MNIST_SVHN) *c = side ? 3 : 1, *sz = 32;
  else *c = 1, *sz = 28;
}
bool is_side(const rgfm_unet* hu, const rgfm_ratio* hr, int side, int* c, int* sz) {
  ratio_side_shape(hr, side, c, sz);
  return hu->d.in_channels == *c && hu->d.img_size == *sz;
}

// the U-Net pair must be the one the estimator handle was built for
int check_grad_pair(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr) {
  int cx = 0, sx = 0, cy = 0, sy = 0;
  const bool okx = is_side(hx, hr, 0, &cx, &sx), oky = is_side(hy, hr, 1, &cy, &sy);
  if (okx && oky) return RGFM_OK;
  return fail(RGFM_EINVAL, "gradient guidance: the estimator handle is built for %dx%dx%d + %dx%dx%d, the U-Nets are %dx%dx%d + %dx%dx%d",
              cx, sx, sx, cy, sy, sy, hx->d.in_channels, hx->d.img_size, hx->d.img_size, hy->d.in_channels, hy->d.img_size, hy->d.img_size);
}

// ... and for one side: the target U-Net must be the estimator's shape for the side that is NOT given
int check_grad_side(const rgfm_unet* hu, const rgfm_ratio* hr, int given) {
  int c = 0, sz = 0;
  if (is_side(hu, hr, given ? 0 : 1, &c, &sz)) return RGFM_OK;
  return fail(RGFM_EINVAL, "conditional gradient guidance: given the estimator's %s, its %s is %dx%dx%d; the target U-Net is %dx%dx%d",
              given ? "y" : "x", given ? "x" : "y", c, sz, sz, hu->d.in_channels, hu->d.img_size, hu->d.img_size);
}

}  // namespace

// Paired loop with gradient log-ratio guidance (reference README.md:159-164: v_guided = v_ind + gamma *
// grad log r(x_t, y_t); the reference ships no code for it): x <- x + (v_x + gamma dlogr/dx) dt, every Euler step.
// Midpoint: both modalities advance stage by stage -- (x_mid, y_mid) = (x, y) + (dt / 2) F(x, y, t1), then
// (x, y) += dt F(x_mid, y_mid, t1 + dt / 2), the gradient taken at the stage's state.
namespace {

// the loop's workspace, in order: the two chains, the velocities, the gradients, then one region per concurrent pass
struct PairGradWs {
  NetChain cx, cy;
  float *vx, *vy, *gx, *gy;
  size_t mark_r;
};
void carve_pair_grad(Bump& b, PairGradWs& w, rgfm_ratio* hr) {
  const int batch = w.cx.batch;
  w.cx.carve(b), w.cy.carve(b);
  w.vx = b.f((size_t)batch * w.cx.image_floats());
  w.vy = b.f((size_t)batch * w.cy.image_floats());
  w.gx = b.f((size_t)batch * w.cx.image_floats());
  w.gy = b.f((size_t)batch * w.cy.image_floats());
  w.cx.carve_eval(), w.cy.carve_eval();
  w.mark_r = b.off;
  RatioPass{hr, batch, &b, nullptr, true}.grad(nullptr, nullptr, nullptr, nullptr, nullptr);
}

int pair_grad_bytes(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr, int batch, int solver, size_t* bytes) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!hx || !hy || !hr || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  if (hr->d.kind == RGFM_RATIO_FLEXIBLE)  // (the fixed kinds: checked by the sampler call)
    if (int rc = check_grad_pair(hx, hy, hr)) return rc;
  Bump b;
  PairGradWs w{{const_cast<rgfm_unet*>(hx), batch, solver}, {const_cast<rgfm_unet*>(hy), batch, solver}};
  carve_pair_grad(b, w, const_cast<rgfm_ratio*>(hr));
  *bytes = b.off;
  return RGFM_OK;
}

// x = base + (v + gamma g) dt over [batch][dim] with the stage's strength: the scalar kernel, or the per-row one
void euler_grad_update(float* x, const float* v, const float* g, int batch, size_t dim, const StageStrength& gamma, float dt,
                       hipStream_t s, const float* base) {
  if (gamma.rows) launch_euler_grad_rows(x, v, g, (size_t)batch * dim, (int)dim, gamma.rows, gamma.scale, dt, s, base);
  else launch_euler_grad(x, v, g, (size_t)batch * dim, (float)gamma.gamma, dt, s, base);
}

int pair_grad_loop(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout, const LoopCall& c) {
  const int batch = c.batch;
  int ns = 0;
  DiagSink sink;  // (the gradient loops need no scratch: v and grad log r are both in the workspace already)
  if (int rc = open_loop(c, hx && hy && hr && x_inout && y_inout, &ns, &sink)) return rc;
  if (int rc = check_grad_pair(hx, hy, hr)) return rc;
  Bump b(c.ws, c.ws_bytes);
  PairGradWs w{{hx, batch, c.solver}, {hy, batch, c.solver}};
  carve_pair_grad(b, w, hr);
  Sde sde = c.sde;
  if (sde.on()) sde.carve(b, batch, w.cx.image_floats(), w.cy.image_floats());
  if (int rc = check_workspace(b, c.ws_bytes)) return rc;
  if (ns == 0) return RGFM_OK;
  DevState* ds = cur_dev();
  if (!ds) return fail(RGFM_EINVAL, "no handle has been created on the current device");
  hipStream_t s = (hipStream_t)c.stream;
  const size_t dx = w.cx.image_floats(), dy = w.cy.image_floats();
  if (int rc = w.cx.begin(s, c.num_steps, c.step_begin, ns)) return rc;
  if (int rc = w.cy.begin(s, c.num_steps, c.step_begin, ns)) return rc;
  if (sink.on())
    if (int rc = sink.begin(s, 0, 0)) return rc;
  const bool overlap = g_modes.overlap;
  // one stage: (xout, yout) = (xb, yb) + (v(in, row's t) + gamma grad log r(xin, yin)) dts; xb / yb null: in place
  // A stage whose scale is 0 runs unguided -- both nets with the fused Euler epilogue on the two streams, as pair_loop's
  // unguided stage, and no ratio pass; its diagnostics record stays zero.
  auto stage = [&](const Stage& g) -> int {
    float *xin = g.reads_mid ? w.cx.mid : x_inout, *yin = g.reads_mid ? w.cy.mid : y_inout;
    float *xout = g.writes_mid ? w.cx.mid : x_inout, *yout = g.writes_mid ? w.cy.mid : y_inout;
    const float *xb = g.writes_mid ? x_inout : nullptr, *yb = g.writes_mid ? y_inout : nullptr;
    float dts = g.dts;
    // (the stochastic step: both pre-updates on `s`, in front of the fork; then xb / yb are its buffers)
    if (int rc = sde.stage(g, c.num_steps, 0, x_inout, (size_t)batch * dx, s, xb, &xb, &dts)) return rc;
    if (int rc = sde.stage(g, c.num_steps, 1, y_inout, (size_t)batch * dy, s, yb, &yb, &dts)) return rc;
    hipStream_t sy = overlap ? ds->side : s;
    if (overlap) {
      HIP_TRY(hipEventRecord(ds->fork, s));
      HIP_TRY(hipStreamWaitEvent(ds->side, ds->fork, 0));
    }
    if (c.strength.off(g.row)) {
      if (int rc = w.cy.eval(g.row, sy, yin, nullptr, yout, yb ? yb : y_inout, dts)) return rc;
      if (overlap) HIP_TRY(hipEventRecord(ds->join, ds->side));
      if (int rc = w.cx.eval(g.row, s, xin, nullptr, xout, xb ? xb : x_inout, dts)) return rc;
      if (overlap) HIP_TRY(hipStreamWaitEvent(s, ds->join, 0));
      return RGFM_OK;
    }
    if (int rc = w.cy.eval(g.row, sy, yin, w.vy, nullptr, nullptr, 0.f)) return rc;
    if (overlap) HIP_TRY(hipEventRecord(ds->join, ds->side));
    if (int rc = w.cx.eval(g.row, s, xin, w.vx, nullptr, nullptr, 0.f)) return rc;
    {
      b.off = w.mark_r;
      RatioPass r{hr, batch, &b, s, false, hx->range_flag};
      ModeScope ratio_mode(hx->conv_mode);  // (the estimator's forward convs follow the x net's handle)
      r.grad(xin, yin, w.gx, w.gy, nullptr);
    }
    if (overlap) HIP_TRY(hipStreamWaitEvent(s, ds->join, 0));
    if (sink.on()) {  // |v| and |grad log r| (before gamma) per row and modality
      float* rec = sink.at(g.row).rec;
      launch_diag_rownorm(w.vx, batch, (int)dx, rec, RGFM_DIAG_V_NORM_X, s);
      launch_diag_rownorm(w.vy, batch, (int)dy, rec, RGFM_DIAG_V_NORM_Y, s);
      launch_diag_rownorm(w.gx, batch, (int)dx, rec, RGFM_DIAG_G_NORM_X, s);
      launch_diag_rownorm(w.gy, batch, (int)dy, rec, RGFM_DIAG_G_NORM_Y, s);
    }
    const StageStrength gamma = c.strength.stage(g.row);
    euler_grad_update(xout, w.vx, w.gx, batch, dx, gamma, dts, s, xb);
    euler_grad_update(yout, w.vy, w.gy, batch, dy, gamma, dts, s, yb);
    return RGFM_OK;
  };
  if (int rc = for_each_stage(c.solver, c.num_steps, c.step_begin, ns, stage)) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

}  // namespace

extern "C" int rgfm_sample_pair_grad_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr, int batch,
                                                     size_t* bytes) {
  return pair_grad_bytes(hx, hy, hr, batch, SOLVER_EULER, bytes);
}
extern "C" int rgfm_sample_pair_grad_ode_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr,
                                                         int batch, int solver, size_t* bytes) {
  return pair_grad_bytes(hx, hy, hr, batch, solver, bytes);
}
extern "C" int rgfm_sample_pair_grad(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout, int batch,
                                     int num_steps, double gamma, int step_begin, int step_end, void* ws, size_t ws_bytes,
                                     rgfm_stream_t stream) {
  return pair_grad_loop(hx, hy, hr, x_inout, y_inout,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .strength = gamma, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
extern "C" int rgfm_sample_pair_grad_ode(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout,
                                         int batch, int num_steps, double gamma, int step_begin, int step_end, int solver,
                                         void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return pair_grad_loop(hx, hy, hr, x_inout, y_inout,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = gamma, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}

// One net with gradient log-ratio guidance, the other side observed: s <- s + (v(s, t) + gamma dlogr/ds) dt, every step
// (midpoint: s_mid = s + (dt / 2) F(s, t1), s += dt F(s_mid, t1 + dt / 2)).
// The velocity net and the estimator's one-sided pass run one after the other on `stream` and share one scratch region.
namespace {

// the loop's workspace, in order: the chain, the velocity, the gradient, then ONE region for the net and the ratio pass
struct CondGradWs {
  NetChain c;
  float *v, *g;
};
CondGradWs carve_cond_grad(Bump& b, rgfm_unet* h, rgfm_ratio* hr, int given, int batch, int solver) {
  CondGradWs w{{h, batch, solver}, nullptr, nullptr};
  w.c.carve(b);
  w.v = b.f((size_t)batch * w.c.image_floats());
  w.g = b.f((size_t)batch * w.c.image_floats());
  w.c.carve_eval();
  const size_t net_end = b.off;
  b.off = w.c.mark;
  RatioPass{hr, batch, &b, nullptr, true}.grad_cond(nullptr, given, nullptr, nullptr, nullptr);
  b.off = std::max(b.off, net_end);
  return w;
}

int cond_grad_bytes(const rgfm_unet* h, const rgfm_ratio* hr, int given, int batch, int solver, size_t* bytes) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!h || !hr || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  int rc = check_given(given);
  if (rc || (rc = check_grad_side(h, hr, given))) return rc;
  Bump b;
  carve_cond_grad(b, const_cast<rgfm_unet*>(h), const_cast<rgfm_ratio*>(hr), given, batch, solver);
  *bytes = b.off;
  return RGFM_OK;
}

int cond_grad_loop(rgfm_unet* h, rgfm_ratio* hr, float* s_inout, const float* ctx, int given, const LoopCall& c) {
  const int batch = c.batch;
  int ns = 0;
  DiagSink sink;
  int rc = open_loop(c, h && hr && s_inout && ctx, &ns, &sink);
  if (rc || (rc = check_given(given)) || (rc = check_grad_side(h, hr, given))) return rc;
  Bump b(c.ws, c.ws_bytes);
  CondGradWs w = carve_cond_grad(b, h, hr, given, batch, c.solver);
  Sde sde = c.sde;
  if (sde.on()) sde.carve(b, batch, w.c.image_floats(), 0);
  if ((rc = check_workspace(b, c.ws_bytes))) return rc;
  if (ns == 0) return RGFM_OK;
  hipStream_t s = (hipStream_t)c.stream;
  const size_t d = w.c.image_floats();
  if ((rc = w.c.begin(s, c.num_steps, c.step_begin, ns))) return rc;
  if (sink.on() && (rc = sink.begin(s, 0, 0))) return rc;
  // one stage: out = base + (v(in, row's t) + gamma grad log r(in)) dts; base null: in place on out
  auto stage = [&](const Stage& g) -> int {
    float *in = g.reads_mid ? w.c.mid : s_inout, *out = g.writes_mid ? w.c.mid : s_inout;
    const float* base = g.writes_mid ? s_inout : nullptr;
    float dts = g.dts;
    if (int rc = sde.stage(g, c.num_steps, 0, s_inout, (size_t)batch * d, s, base, &base, &dts)) return rc;
    // scale 0: the unguided stage (NetChain::step's evaluation), no ratio pass, a zero record
    if (c.strength.off(g.row)) return w.c.eval(g.row, s, in, nullptr, out, base ? base : s_inout, dts);
    if (int rc = w.c.eval(g.row, s, in, w.v, nullptr, nullptr, 0.f)) return rc;
    {
      b.off = w.c.mark;
      RatioPass r{hr, batch, &b, s, false, h->range_flag};
      ModeScope ratio_mode(h->conv_mode);  // (the estimator's convs follow the target net's handle)
      r.grad_cond(ctx, given, in, w.g, nullptr);
    }
    if (sink.on()) {  // (one-sided: the target's norms in the x entries, whichever side of the estimator it is)
      float* rec = sink.at(g.row).rec;
      launch_diag_rownorm(w.v, batch, (int)d, rec, RGFM_DIAG_V_NORM_X, s);
      launch_diag_rownorm(w.g, batch, (int)d, rec, RGFM_DIAG_G_NORM_X, s);
    }
    euler_grad_update(out, w.v, w.g, batch, d, c.strength.stage(g.row), dts, s, base);
    return RGFM_OK;
  };
  if ((rc = for_each_stage(c.solver, c.num_steps, c.step_begin, ns, stage))) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

}  // namespace

extern "C" int rgfm_sample_cond_grad_workspace_bytes(const rgfm_unet* h, const rgfm_ratio* hr, int given, int batch, size_t* bytes) {
  return cond_grad_bytes(h, hr, given, batch, SOLVER_EULER, bytes);
}
extern "C" int rgfm_sample_cond_grad_ode_workspace_bytes(const rgfm_unet* h, const rgfm_ratio* hr, int given, int batch, int solver,
                                                         size_t* bytes) {
  return cond_grad_bytes(h, hr, given, batch, solver, bytes);
}
extern "C" int rgfm_sample_cond_grad(rgfm_unet* h, rgfm_ratio* hr, float* s_inout, const float* ctx, int given, int batch,
                                     int num_steps, double gamma, int step_begin, int step_end, void* ws, size_t ws_bytes,
                                     rgfm_stream_t stream) {
  return cond_grad_loop(h, hr, s_inout, ctx, given,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .strength = gamma, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
extern "C" int rgfm_sample_cond_grad_ode(rgfm_unet* h, rgfm_ratio* hr, float* s_inout, const float* ctx, int given, int batch,
                                         int num_steps, double gamma, int step_begin, int step_end, int solver, void* ws,
                                         size_t ws_bytes, rgfm_stream_t stream) {
  return cond_grad_loop(h, hr, s_inout, ctx, given,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = gamma, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}

// ---- the gradient-guided loops with the diagnostics sink (include/rgfm.h, "Guidance diagnostics"): no extra workspace
extern "C" int rgfm_sample_pair_grad_diag_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr,
                                                          int batch, int solver, size_t* bytes) {
  return pair_grad_bytes(hx, hy, hr, batch, solver, bytes);
}
extern "C" int rgfm_sample_pair_grad_diag(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout,
                                          int batch, int num_steps, double gamma, int step_begin, int step_end, int solver,
                                          float* diag_out, size_t diag_records, void* ws, size_t ws_bytes,
                                          rgfm_stream_t stream) {
  return pair_grad_loop(hx, hy, hr, x_inout, y_inout,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = gamma, .diag_out = diag_out, .diag_records = diag_records, .ws = ws,
                         .ws_bytes = ws_bytes, .stream = stream});
}
extern "C" int rgfm_sample_cond_grad_diag_workspace_bytes(const rgfm_unet* h, const rgfm_ratio* hr, int given, int batch,
                                                          int solver, size_t* bytes) {
  return cond_grad_bytes(h, hr, given, batch, solver, bytes);
}
extern "C" int rgfm_sample_cond_grad_diag(rgfm_unet* h, rgfm_ratio* hr, float* s_inout, const float* ctx, int given, int batch,
                                          int num_steps, double gamma, int step_begin, int step_end, int solver,
                                          float* diag_out, size_t diag_records, void* ws, size_t ws_bytes,
                                          rgfm_stream_t stream) {
  return cond_grad_loop(h, hr, s_inout, ctx, given,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = gamma, .diag_out = diag_out, .diag_records = diag_records, .ws = ws,
                         .ws_bytes = ws_bytes, .stream = stream});
}

// ---- guidance strength as data (include/rgfm.h, "Guidance strength per sample and per stage"): each loop is its *_diag
// namesake with (gamma_rows, stage_scale, n_stage_scale) behind gamma
extern "C" int rgfm_sample_pair_grad_gs(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout, int batch,
                                        int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                                        int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                                        size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return pair_grad_loop(hx, hy, hr, x_inout, y_inout,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale),
                         .diag_out = diag_out, .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
extern "C" int rgfm_sample_cond_grad_gs(rgfm_unet* h, rgfm_ratio* hr, float* s_inout, const float* ctx, int given, int batch,
                                        int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                                        int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                                        size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return cond_grad_loop(h, hr, s_inout, ctx, given,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale),
                         .diag_out = diag_out, .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}

// ---- the stochastic step (include/rgfm.h, "Stochastic sampling"): the *_gs loops with `const rgfm_sde* sde` in front of ws
extern "C" int rgfm_sample_pair_grad_sde(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout, int batch,
                                         int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                                         int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                                         size_t diag_records, const rgfm_sde* sde, void* ws, size_t ws_bytes,
                                         rgfm_stream_t stream) {
  return pair_grad_loop(hx, hy, hr, x_inout, y_inout,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale),
                         .diag_out = diag_out, .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream,
                         .sde = sde});
}
extern "C" int rgfm_sample_cond_grad_sde(rgfm_unet* h, rgfm_ratio* hr, float* s_inout, const float* ctx, int given, int batch,
                                         int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                                         int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                                         size_t diag_records, const rgfm_sde* sde, void* ws, size_t ws_bytes,
                                         rgfm_stream_t stream) {
  return cond_grad_loop(h, hr, s_inout, ctx, given,
                        {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end,
                         .solver = solver, .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale),
                         .diag_out = diag_out, .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream,
                         .sde = sde});
}
