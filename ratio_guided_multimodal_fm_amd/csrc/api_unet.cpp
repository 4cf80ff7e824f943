// api_unet.cpp -- the U-Net handle: parameter ingestion / packing, forward, trace hooks (C ABI: include/rgfm.h).  The
// network's topology is the op list of unet_plan.h (plan_unet); the inference walk over it is UNetRun (rgfm_host.h).
#include "rgfm_host.h"

extern "C" int rgfm_unet_param_floats(const rgfm_unet_desc* desc, size_t* n_floats) {
  int rc = check_desc(desc);
  if (rc) return rc;
  if (!n_floats) return fail(RGFM_EINVAL, "null output");
  *n_floats = plan_unet(*desc).layout.n_params;
  return RGFM_OK;
}

// Every derived weight image of the handle from h->params: the fp32-packed, two-plane and bf16 images, the stride-2
// phase order, the Upsample parity-class sums, the Winograd images and the output conv's layout; then which convs may
// run on the fp16 path (synchronises once).  Used by rgfm_unet_create and, in place, by rgfm_unet_update_params.
static int pack_weights(rgfm_unet* h, hipStream_t s) {
  std::vector<HxImage*> images;
  std::vector<NormGate> gates;
  std::vector<ConvW*> res_convs;
  for (ResW& r : h->res) {
    res_convs.push_back(&r.c1), res_convs.push_back(&r.c2);
    if (r.has_skip) res_convs.push_back(&r.sk);
    gates.push_back({r.n1w, r.n1b, r.cin, &r.c1.hx}), gates.push_back({r.n2w, r.n2b, r.cout, &r.c2.hx});
  }
  for (ConvW* w : res_convs) pack_one(h, *w, CONV_S1, s), images.push_back(&w->hx);
  for (ConvW& w : h->down) {  // stride-2 convs: phase-ordered weights, and once more in plain tap order
    pack_one(h, w, CONV_S2, s), images.push_back(&w.hx);
    launch_pack_conv_hx2(h->params + w.w_raw, h->packedh + w.hx9.off, h->hq + 4 * w.hx9.hq, w.cout, w.cin, 9, CONV_S1, s);
    images.push_back(&w.hx9);
  }
  // the Upsample convs once more as ConvTranspose2d(4, 2, 1) weights (summed taps), packed in parity-class order; the
  // ResBlock convs once more as Winograd images (one scratch array serves both)
  for (ConvW& w : h->up) {
    pack_one(h, w, CONV_S1, s), images.push_back(&w.hx);
    launch_up2_as_deconv(h->params + w.w_raw, h->wtmp, w.cout, w.cin, s);
    launch_pack_conv_hx2(h->wtmp, h->packedh + w.t2.off, h->hq + 4 * w.t2.hq, w.cout, w.cin, 16, CONV_T2, s);
    images.push_back(&w.t2);
  }
  for (ConvW* w : res_convs)
    if (w->wino.present) {
      launch_pack_conv_hx2w(h->params + w->w_raw, h->packedh + w->wino.off, h->hq + 4 * w->wino.hq, h->wtmp, w->cout, w->cin, s);
      images.push_back(&w->wino);
    }
  launch_pack_conv_out(h->params + h->ocw, h->packed + h->ocw_pk, h->d.in_channels, h->final_ch, s);
  if (int rc = read_hx_flags(*h, images, s)) return rc;
  return demote_by_norms(*h, gates, s);
}

// label_emb.weight [K + 1][temb] of a class-conditional net, in floats (K = 0: none)
static size_t label_floats(const rgfm_unet_desc& d, int num_classes) {
  return num_classes ? (size_t)(num_classes + 1) * (size_t)(4 * d.model_channels) : 0;
}
static int check_classes(int num_classes) {
  // (a sampler call's class table holds 4096 rows, sampler_host.h: one stage of K + 1 classes must fit)
  if (num_classes < 1 || num_classes >= 4096) return fail(RGFM_EINVAL, "num_classes must be in [1, 4096), got %d", num_classes);
  return RGFM_OK;
}

extern "C" int rgfm_unet_labeled_param_floats(const rgfm_unet_desc* desc, int num_classes, size_t* n_floats) {
  if (int rc = rgfm_unet_param_floats(desc, n_floats)) return rc;
  if (int rc = check_classes(num_classes)) return rc;
  *n_floats += label_floats(*desc, num_classes);
  return RGFM_OK;
}

// num_classes 0: the unlabelled handle of rgfm_unet_create
static int create_unet(const rgfm_unet_desc* desc, int num_classes, const float* params_dev, size_t n_floats,
                       rgfm_stream_t stream, rgfm_unet** out) {
  int rc = check_desc(desc);
  if (rc) return rc;
  if (!params_dev || !out) return fail(RGFM_EINVAL, "null argument");
  if ((rc = ensure_init())) return rc;
  hipStream_t s = (hipStream_t)stream;
  rgfm_unet* h = new rgfm_unet();
  h->d = *desc;
  static_cast<UNetPlan&>(*h) = plan_unet(*desc);
  static_cast<WeightLayout&>(*h) = h->layout;
  h->num_classes = num_classes, h->lemb = h->n_params;
  h->n_params += label_floats(*desc, num_classes);  // (the store's count: alloc, update_params and the backward's blob follow it)
  if (h->n_params != n_floats) {
    const size_t want = h->n_params;
    delete h;
    return fail(RGFM_EINVAL, "parameter blob has %zu floats, architecture needs %zu", n_floats, want);
  }
  for (const ResW& r : h->res)
    if (r.cin % KC || r.cout % 32) {
      delete h;
      return fail(RGFM_EINVAL, "channel counts must be multiples of 16 (in) / 32 (out)");
    }
  auto bail = [&](int code, const char* what) {
    rgfm_unet_destroy(h);
    return fail(code, "%s", what);
  };
  if ((rc = h->alloc(params_dev, true, s))) return rgfm_unet_destroy(h), rc;
  {
    size_t mx = 0;
    for (const ConvW& w : h->up) mx = std::max(mx, (size_t)w.cin * w.cout * 16);
    for (const ResW& r : h->res) {
      if (r.c1.wino.present) mx = std::max(mx, (size_t)r.c1.cin * r.c1.cout * 16);
      if (r.c2.wino.present) mx = std::max(mx, (size_t)r.c2.cin * r.c2.cout * 16);
    }
    if (mx && hipMalloc(&h->wtmp, mx * sizeof(float)) != hipSuccess) return bail(RGFM_ENOMEM, "hipMalloc(upsample weights)");
  }
  if ((rc = pack_weights(h, s))) return bail(rc, "packing the weights failed");
  // frequency table exp(-ln(1e4) * i / half) in fp32, as torch evaluates it (unet_flexible.py:28-31)
  const int half = h->mc / 2;
  std::vector<float> fr(half);
  const float neg_log = (float)(-std::log(10000.0));
  for (int i = 0; i < half; ++i) fr[i] = std::exp(((float)i * neg_log) / (float)half);
  std::vector<TimeLinear> lin;
  for (const ResW& r : h->res) lin.push_back({(int)r.tw, (int)r.tb, r.cout, r.temb_off});
  h->nlin = (int)lin.size();
  if (hipMalloc(&h->freqs, half * sizeof(float)) != hipSuccess) return bail(RGFM_ENOMEM, "hipMalloc(freqs)");
  if (hipMalloc(&h->lin_dev, lin.size() * sizeof(TimeLinear)) != hipSuccess) return bail(RGFM_ENOMEM, "hipMalloc(lin)");
  if (hipMemcpy(h->freqs, fr.data(), half * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->lin_dev, lin.data(), lin.size() * sizeof(TimeLinear), hipMemcpyHostToDevice) != hipSuccess)
    return bail(RGFM_EHIP, "hipMemcpy(tables)");
  *out = h;
  return RGFM_OK;
}

extern "C" int rgfm_unet_create(const rgfm_unet_desc* desc, const float* params_dev, size_t n_floats,
                                rgfm_stream_t stream, rgfm_unet** out) {
  return create_unet(desc, 0, params_dev, n_floats, stream, out);
}
extern "C" int rgfm_unet_labeled_create(const rgfm_unet_desc* desc, int num_classes, const float* params_dev, size_t n_floats,
                                        rgfm_stream_t stream, rgfm_unet** out) {
  if (int rc = check_desc(desc)) return rc;
  if (int rc = check_classes(num_classes)) return rc;
  return create_unet(desc, num_classes, params_dev, n_floats, stream, out);
}

extern "C" void rgfm_unet_destroy(rgfm_unet* h) {
  if (!h) return;
  h->free();
  if (h->freqs) (void)hipFree(h->freqs);
  if (h->lin_dev) (void)hipFree(h->lin_dev);
  if (h->wtmp) (void)hipFree(h->wtmp);
  delete h;
}

extern "C" int rgfm_unet_update_params(rgfm_unet* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream) {
  if (!h || !params_dev) return fail(RGFM_EINVAL, "null argument");
  if (n_floats != h->n_params) return fail(RGFM_EINVAL, "parameter blob has %zu floats, the handle has %zu", n_floats, h->n_params);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(h->params, params_dev, n_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
  return pack_weights(h, s);
}

extern "C" int rgfm_unet_set_conv_mode(rgfm_unet* h, int mode) {
  if (!h) return fail(RGFM_EINVAL, "null handle");
  if (int rc = check_conv_mode(mode)) return rc;
  h->conv_mode = mode;
  return RGFM_OK;
}
extern "C" int rgfm_unet_range_flag(rgfm_unet* h, int* flagged, int reset, rgfm_stream_t stream) {
  if (!h) return fail(RGFM_EINVAL, "null handle");
  return read_flag_word(h->range_flag, flagged, reset, (hipStream_t)stream);
}

extern "C" int rgfm_unet_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes) {
  if (!h || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  *bytes = unet_eval_bytes(const_cast<rgfm_unet*>(h), batch) + table_bytes(h, batch) + counter_bytes(batch);
  return RGFM_OK;
}

// labels (device int32 [batch]) non-null: the labelled forward -- a [batch]-row time table, row b of (t_b, label_b)
static int unet_forward(rgfm_unet* h, const float* x, const float* t_dev, int t_count, const int* labels, float* v_out,
                        int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  refresh_modes();
  if (!h || !x || !t_dev || !v_out || !ws) return fail(RGFM_EINVAL, "null argument");
  if (batch < 1 || (t_count != 1 && t_count != batch)) return fail(RGFM_EINVAL, "t_count must be 1 or batch");
  if (labels && !h->num_classes) return fail(RGFM_EINVAL, "labels on a handle without classes (rgfm_unet_labeled_create makes one)");
  hipStream_t s = (hipStream_t)stream;
  Bump b(ws, ws_bytes);
  size_t need = 0;
  rgfm_unet_workspace_bytes(h, batch, &need);
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  const int rows = labels ? batch : t_count;
  float* table = b.f((size_t)rows * h->temb_total);
  unsigned* cnt = b.u(batch);
  HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)batch * sizeof(unsigned), s));
  if (labels) launch_class_table(h, t_dev, t_count == 1, labels, 1, 0, rows, table, s);
  else launch_time_table(h, t_dev, 1, 0, t_count, table, s);
  UNetRun r{h, batch, &b, s, table, rows == batch ? 1 : 0, false};
  r.fin_counter = cnt;
  int rc = r.run(x, v_out, nullptr, 0.f);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_unet_forward(rgfm_unet* h, const float* x, const float* t_dev, int t_count, float* v_out,
                                 int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return unet_forward(h, x, t_dev, t_count, nullptr, v_out, batch, ws, ws_bytes, stream);
}
extern "C" int rgfm_unet_forward_labels(rgfm_unet* h, const float* x, const float* t_dev, int t_count, const int32_t* labels_dev,
                                        float* v_out, int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return unet_forward(h, x, t_dev, t_count, labels_dev, v_out, batch, ws, ws_bytes, stream);
}

extern "C" int rgfm_unet_time_embedding(rgfm_unet* h, const float* t_dev, int t_count, float* emb_out, void* ws,
                                        size_t ws_bytes, rgfm_stream_t stream) {
  if (!h || !t_dev || !emb_out || !ws || t_count < 1) return fail(RGFM_EINVAL, "bad argument");
  if (table_bytes(h, t_count) > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small");
  TimeEmbedArgs a = time_embed_args(h, t_dev, 1, 0, reinterpret_cast<float*>(ws));
  a.emb_out = emb_out;
  launch_time_embed(a, t_count, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_unet_set_trace(rgfm_unet* h, int enable) {
  if (!h) return fail(RGFM_EINVAL, "null handle");
  h->trace = enable != 0;
  h->acts.clear();
  return RGFM_OK;
}

extern "C" int rgfm_unet_p_handovers(const rgfm_unet* h, int* blocks) {
  if (!h || !blocks) return fail(RGFM_EINVAL, "null argument");
  *blocks = h->p_handovers;
  return RGFM_OK;
}
extern "C" int rgfm_unet_wino_convs(const rgfm_unet* h, int* convs) {
  if (!h || !convs) return fail(RGFM_EINVAL, "null argument");
  *convs = h->wino_convs;
  return RGFM_OK;
}
extern "C" int rgfm_unet_up_merged(const rgfm_unet* h, int* convs) {
  if (!h || !convs) return fail(RGFM_EINVAL, "null argument");
  *convs = h->up_merged;
  return RGFM_OK;
}
extern "C" int rgfm_unet_conv_routes(const rgfm_unet* h, int* counts, int n) {
  if (!h || !counts || n < 0) return fail(RGFM_EINVAL, "null argument or negative count");
  for (int i = 0; i < n && i < RGFM_ROUTE_SLOTS; ++i) counts[i] = h->routes[i];
  return RGFM_OK;
}

extern "C" int rgfm_unet_num_activations(const rgfm_unet* h, int* n) {
  if (!h || !n) return fail(RGFM_EINVAL, "null argument");
  *n = (int)unet_trace_table(*h).size();
  return RGFM_OK;
}

extern "C" int rgfm_unet_activation_shape(const rgfm_unet* h, int index, int* channels, int* height, int* width) {
  if (!h) return fail(RGFM_EINVAL, "null handle");
  const std::vector<UTensor> t = unet_trace_table(*h);
  if (index < 0 || index >= (int)t.size()) return fail(RGFM_EINVAL, "activation index out of range");
  *channels = t[index].C;
  *height = *width = t[index].S;
  return RGFM_OK;
}

extern "C" int rgfm_unet_read_activation(rgfm_unet* h, int index, int batch, const void* ws, float* out_dev,
                                         rgfm_stream_t stream) {
  (void)ws;
  if (!h || !out_dev) return fail(RGFM_EINVAL, "null argument");
  if (index < 0 || index >= (int)h->acts.size()) return fail(RGFM_EINVAL, "no traced activation %d (run a forward in trace mode first)", index);
  const auto& a = h->acts[index];
  hipStream_t s = (hipStream_t)stream;
  if (a.nchw) HIP_TRY(hipMemcpyAsync(out_dev, a.data, (size_t)batch * a.C * a.S * a.S * sizeof(float), hipMemcpyDeviceToDevice, s));
  else launch_nhwc_to_nchw(a.data, out_dev, batch, a.C, a.S * a.S, s);
  return RGFM_OK;
}
