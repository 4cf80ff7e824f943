// api_train.cpp -- training pass of the U-Net handle: the forward that keeps what the backward needs, the backward to
// dx and to every parameter, and the dropout mask hook (C ABI: include/rgfm.h; kernels: unet_grad.hip).
//
// The walk is the reference FlexibleUNet.forward (src/models/unet_flexible.py:203-261) over NCHW tensors in the
// caller's workspace, laid out by plan_train: first the SAVED state (dropout header, x, the time path, every tensor
// the walk produces, and per ResBlock the group statistics of both norms, the time projection and conv1's output),
// then the backward's SCRATCH (one gradient buffer per produced tensor and a few transient maps).
#include "rgfm_host.h"

namespace {

struct TTensor {  // a produced tensor: float offset into the workspace, channels, square size
  size_t off;
  int C, S;
};

enum { OP_IN, OP_RES, OP_DOWN, OP_UP, OP_OUT };

struct TOp {
  int kind;
  const ResW* r = nullptr;
  const ConvW* cw = nullptr;  // Downsample / Upsample conv (the input and output convs: TrainPlan)
  int in0 = -1, in1 = -1, out = -1;
  int S = 0;       // spatial size of the input
  int block = -1;  // ResBlock index in walk order (the dropout mask's block id)
  size_t mr1 = 0, temb = 0, h1 = 0, mr2 = 0;
};

struct TrainPlan {
  std::vector<TTensor> T;
  std::vector<TOp> ops;
  std::vector<size_t> dT;  // gradient buffer of T[i]
  size_t hdr, x0, emb0, e1, emb, mro, saved;
  size_t dT_begin, dT_end, A, R, G, DH, part, pg, pb, dtemb, dsemb, de1;
  size_t total;  // floats
  ConvW in_conv, out_conv;
  int nblocks = 0;
};

int groups_of(int C) { return std::min(8, C); }

TrainPlan plan_train(const rgfm_unet* h, int B) {
  TrainPlan p;
  Cursor c;
  const rgfm_unet_desc& d = h->d;
  const int mc = h->mc, temb = h->temb, S0 = d.img_size;
  size_t mx = 1, mxC = 1, mx_part = 1;
  auto big = [&](int C, int S) { mx = std::max(mx, (size_t)B * C * S * S); };
  p.hdr = c.take(64);
  p.x0 = c.take((size_t)B * d.in_channels * S0 * S0);
  p.emb0 = c.take((size_t)B * mc);
  p.e1 = c.take((size_t)B * temb);
  p.emb = c.take((size_t)B * temb);
  auto tensor = [&](int C, int S) {
    p.T.push_back({c.take((size_t)B * C * S * S), C, S});
    big(C, S);
    return (int)p.T.size() - 1;
  };
  auto part_of = [&](int Cout, int Cin, int taps, int So) {
    UgConv u{};
    u.Cout = Cout, u.Cin = Cin, u.taps = taps, u.B = B, u.Ho = u.Wo = So;
    wgrad_split(u);
    mx_part = std::max(mx_part, (size_t)u.splits * Cout * Cin * taps);
  };
  p.in_conv.w_raw = h->icw, p.in_conv.b = h->icb, p.in_conv.cin = d.in_channels, p.in_conv.cout = mc;
  p.out_conv.w_raw = h->ocw, p.out_conv.b = h->ocb, p.out_conv.cin = h->final_ch, p.out_conv.cout = d.in_channels;
  int S = S0;
  TOp in{OP_IN};
  in.S = S, in.out = tensor(mc, S);
  p.ops.push_back(in);
  part_of(mc, d.in_channels, 9, S);
  int cur = in.out;
  std::vector<int> skips{cur};
  auto res = [&](const ResW& r, int a, int b) {
    TOp o{OP_RES};
    o.r = &r, o.in0 = a, o.in1 = b, o.S = S, o.block = p.nblocks++;
    const int cin = r.cin, cout = r.cout;
    o.mr1 = c.take((size_t)B * groups_of(cin) * 2);
    o.temb = c.take((size_t)B * cout);
    o.h1 = c.take((size_t)B * cout * S * S);
    o.mr2 = c.take((size_t)B * groups_of(cout) * 2);
    o.out = tensor(cout, S);
    big(cin, S);
    mxC = std::max(mxC, (size_t)cin);
    part_of(cout, cin, 9, S);
    part_of(cout, cout, 9, S);
    if (r.has_skip) part_of(cout, cin, 1, S);
    p.ops.push_back(o);
    return o.out;
  };
  size_t ei = 0, di = 0, ui = 0;
  for (int l = 0; l < d.num_levels; ++l) {
    for (int i = 0; i < d.num_res_blocks; ++i) {
      cur = res(h->enc[ei++], cur, -1);
      skips.push_back(cur);
    }
    if (l < d.num_levels - 1) {
      TOp o{OP_DOWN};
      o.cw = &h->down[l], o.in0 = cur, o.S = S, o.out = tensor(o.cw->cout, S / 2);
      part_of(o.cw->cout, o.cw->cin, 9, S / 2);
      p.ops.push_back(o);
      cur = o.out, S /= 2;
      skips.push_back(cur);
    }
  }
  cur = res(h->mid[0], cur, -1);
  cur = res(h->mid[1], cur, -1);
  for (int l = d.num_levels - 1; l >= 0; --l) {
    for (int i = 0; i < d.num_res_blocks + 1; ++i) {
      cur = res(h->dec[di++], cur, skips.back());
      skips.pop_back();
    }
    if (l > 0) {
      TOp o{OP_UP};
      o.cw = &h->up[ui++], o.in0 = cur, o.S = S, o.out = tensor(o.cw->cout, 2 * S);
      big(o.cw->cout, 2 * S);
      part_of(o.cw->cout, o.cw->cin, 9, 2 * S);
      p.ops.push_back(o);
      cur = o.out, S *= 2;
    }
  }
  TOp out{OP_OUT};
  out.in0 = cur, out.S = S;
  p.ops.push_back(out);
  part_of(d.in_channels, h->final_ch, 9, S);
  mxC = std::max(mxC, (size_t)h->final_ch);
  p.mro = c.take((size_t)B * groups_of(h->final_ch) * 2);
  p.saved = c.off;
  p.dT_begin = c.off;
  for (const TTensor& t : p.T) p.dT.push_back(c.take((size_t)B * t.C * t.S * t.S));
  p.dT_end = c.off;
  p.A = c.take(mx), p.R = c.take(mx), p.G = c.take(mx), p.DH = c.take(mx);
  p.part = c.take(mx_part);
  p.pg = c.take((size_t)B * mxC), p.pb = c.take((size_t)B * mxC);
  p.dtemb = c.take((size_t)B * mxC);
  p.dsemb = c.take((size_t)B * temb), p.de1 = c.take((size_t)B * temb);
  p.total = c.off;
  return p;
}

// conv description: mode 0 stride 1, 1 stride 2 (Downsample), 2 nearest x 2 then stride 1 (Upsample); S = source size
UgConv conv_of(const rgfm_unet* h, const ConvW& w, int B, int S, int mode) {
  UgConv c{};
  c.w = h->params + w.w_raw, c.bias = h->params + w.b;
  c.B = B, c.Cin = w.cin, c.Cout = w.cout, c.taps = w.taps;
  c.stride = mode == 1 ? 2 : 1, c.up = mode == 2;
  c.Hs = c.Ws = S;
  c.Hc = c.Wc = mode == 2 ? 2 * S : S;
  c.Ho = c.Wo = mode == 1 ? S / 2 : c.Hc;
  c.C0 = w.cin;
  c.splits = 1;
  return c;
}

UgAct act_of(const float* s0, const float* s1, int C0, int C1, int B, int HW, const float* mr, const float* gamma,
             const float* beta, const unsigned* hdr, int block, float* out) {
  UgAct a{};
  a.s0 = s0, a.s1 = s1, a.C0 = C0, a.C1 = C1, a.B = B, a.HW = HW, a.groups = mr ? groups_of(C0 + C1) : 1;
  a.mr = mr, a.gamma = gamma, a.beta = beta, a.drop_hdr = hdr, a.block = block, a.out = out;
  return a;
}

int check_train(const rgfm_unet* h, int batch, void* ws, size_t ws_bytes, size_t* need) {
  if (!h || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  *need = plan_train(h, batch).total * sizeof(float);
  if (!ws || ws_bytes < *need) return fail(RGFM_ENOMEM, "training workspace too small: %zu < %zu bytes", ws_bytes, *need);
  return RGFM_OK;
}

}  // namespace

extern "C" int rgfm_unet_train_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes) {
  if (!h || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  *bytes = plan_train(h, batch).total * sizeof(float);
  return RGFM_OK;
}

extern "C" int rgfm_unet_forward_train(rgfm_unet* h, const float* x, const float* t_dev, int t_count, float* v_out,
                                       int batch, float p_drop, uint64_t seed, void* ws, size_t ws_bytes,
                                       rgfm_stream_t stream) {
  size_t need = 0;
  if (int rc = check_train(h, batch, ws, ws_bytes, &need)) return rc;
  if (!x || !t_dev || !v_out || (t_count != 1 && t_count != batch)) return fail(RGFM_EINVAL, "bad argument");
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(RGFM_EINVAL, "p_drop must be in [0, 1)");
  hipStream_t s = (hipStream_t)stream;
  const TrainPlan p = plan_train(h, batch);
  const int B = batch, mc = h->mc, temb = h->temb;
  float* W = (float*)ws;
  const float* P = h->params;
  unsigned* hdr = (unsigned*)(W + p.hdr);
  launch_ug_header(hdr, p_drop, seed, s);
  HIP_TRY(hipMemcpyAsync(W + p.x0, x, (size_t)B * h->d.in_channels * h->d.img_size * h->d.img_size * sizeof(float),
                         hipMemcpyDeviceToDevice, s));
  launch_ug_sincos(t_dev, t_count, h->freqs, B, mc, W + p.emb0, s);
  launch_ug_linear(W + p.emb0, P + h->te0w, P + h->te0b, W + p.e1, B, mc, temb, 0, s);
  launch_ug_linear(W + p.e1, P + h->te2w, P + h->te2b, W + p.emb, B, temb, temb, 1, s);
  for (const TOp& o : p.ops) {
    const int S = o.S, HW = S * S;
    switch (o.kind) {
      case OP_IN:
        run_fwd(conv_of(h, p.in_conv, B, S, 0), W + p.x0, W + p.T[o.out].off, nullptr, nullptr, s);
        break;
      case OP_DOWN:
        run_fwd(conv_of(h, *o.cw, B, S, 1), W + p.T[o.in0].off, W + p.T[o.out].off, nullptr, nullptr, s);
        break;
      case OP_UP:
        run_fwd(conv_of(h, *o.cw, B, S, 2), W + p.T[o.in0].off, W + p.T[o.out].off, nullptr, nullptr, s);
        break;
      case OP_OUT: {
        const TTensor& t = p.T[o.in0];
        launch_ug_gn_stats(W + t.off, nullptr, t.C, 0, B, HW, groups_of(t.C), W + p.mro, s);
        launch_ug_gn_act(act_of(W + t.off, nullptr, t.C, 0, B, HW, W + p.mro, P + h->onw, P + h->onb, nullptr, -1,
                                W + p.A), s);
        run_fwd(conv_of(h, p.out_conv, B, S, 0), W + p.A, v_out, nullptr, nullptr, s);
        break;
      }
      case OP_RES: {
        const ResW& r = *o.r;
        const float* s0 = W + p.T[o.in0].off;
        const float* s1 = o.in1 >= 0 ? W + p.T[o.in1].off : nullptr;
        const int C0 = p.T[o.in0].C, C1 = o.in1 >= 0 ? p.T[o.in1].C : 0;
        float* out = W + p.T[o.out].off;
        launch_ug_gn_stats(s0, s1, C0, C1, B, HW, groups_of(r.cin), W + o.mr1, s);
        launch_ug_gn_act(act_of(s0, s1, C0, C1, B, HW, W + o.mr1, P + r.n1w, P + r.n1b, nullptr, o.block, W + p.A), s);
        launch_ug_linear(W + p.emb, P + r.tw, P + r.tb, W + o.temb, B, temb, r.cout, 1, s);
        run_fwd(conv_of(h, r.c1, B, S, 0), W + p.A, W + o.h1, W + o.temb, nullptr, s);
        launch_ug_gn_stats(W + o.h1, nullptr, r.cout, 0, B, HW, groups_of(r.cout), W + o.mr2, s);
        launch_ug_gn_act(act_of(W + o.h1, nullptr, r.cout, 0, B, HW, W + o.mr2, P + r.n2w, P + r.n2b, hdr, o.block,
                                W + p.A), s);
        const float* xr = s0;  // the block input as the skip path sees it (raw)
        if (C1) {
          launch_ug_gn_act(act_of(s0, s1, C0, C1, B, HW, nullptr, nullptr, nullptr, nullptr, -1, W + p.R), s);
          xr = W + p.R;
        }
        if (r.has_skip) {
          run_fwd(conv_of(h, r.sk, B, S, 0), xr, out, nullptr, nullptr, s);
          run_fwd(conv_of(h, r.c2, B, S, 0), W + p.A, out, nullptr, out, s);
        } else {
          run_fwd(conv_of(h, r.c2, B, S, 0), W + p.A, out, nullptr, xr, s);
        }
        break;
      }
    }
  }
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_unet_backward(rgfm_unet* h, const float* dv, float* dx_out, float* dparams_out, int batch,
                                  void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  size_t need = 0;
  if (int rc = check_train(h, batch, ws, ws_bytes, &need)) return rc;
  if (!dv || !dparams_out) return fail(RGFM_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const TrainPlan p = plan_train(h, batch);
  const int B = batch, mc = h->mc, temb = h->temb;
  float* W = (float*)ws;
  const float* P = h->params;
  float* D = dparams_out;
  const unsigned* hdr = (const unsigned*)(W + p.hdr);
  HIP_TRY(hipMemsetAsync(D, 0, h->n_params * sizeof(float), s));
  HIP_TRY(hipMemsetAsync(W + p.dT_begin, 0, (p.dT_end - p.dT_begin) * sizeof(float), s));
  HIP_TRY(hipMemsetAsync(W + p.dsemb, 0, (size_t)B * temb * sizeof(float), s));
  // dgamma / dbeta of a norm from the per-sample partials
  auto norm_grads = [&](int C, size_t gw, size_t gb) {
    launch_ug_colsum(W + p.pg, B, C, D + gw, s);
    launch_ug_colsum(W + p.pb, B, C, D + gb, s);
  };
  for (auto it = p.ops.rbegin(); it != p.ops.rend(); ++it) {
    const TOp& o = *it;
    const int S = o.S, HW = S * S;
    switch (o.kind) {
      case OP_OUT: {
        const TTensor& t = p.T[o.in0];
        const UgAct a = act_of(W + t.off, nullptr, t.C, 0, B, HW, W + p.mro, P + h->onw, P + h->onb, nullptr, -1,
                               W + p.A);
        launch_ug_gn_act(a, s);
        const UgConv c = conv_of(h, p.out_conv, B, S, 0);
        run_wgrad(c, dv, W + p.A, W + p.part, D + h->ocw, D + h->ocb, s);
        run_dgrad(c, dv, W + p.G, nullptr, t.C, 0, s);
        launch_ug_gn_act_bwd(a, W + p.G, W + p.dT[o.in0], nullptr, 1, 0, W + p.pg, W + p.pb, s);
        norm_grads(t.C, h->onw, h->onb);
        break;
      }
      case OP_UP: {
        const UgConv c = conv_of(h, *o.cw, B, S, 2);
        const float* dy = W + p.dT[o.out];
        run_wgrad(c, dy, W + p.T[o.in0].off, W + p.part, D + o.cw->w_raw, D + o.cw->b, s);
        run_dgrad(c, dy, W + p.G, nullptr, c.Cin, 0, s);  // gradient of the upsampled map (2S x 2S)
        launch_ug_pool2_add(W + p.G, W + p.dT[o.in0], B * c.Cin, S, S, s);
        break;
      }
      case OP_DOWN: {
        const UgConv c = conv_of(h, *o.cw, B, S, 1);
        const float* dy = W + p.dT[o.out];
        run_wgrad(c, dy, W + p.T[o.in0].off, W + p.part, D + o.cw->w_raw, D + o.cw->b, s);
        run_dgrad(c, dy, W + p.dT[o.in0], nullptr, c.Cin, 1, s);
        break;
      }
      case OP_IN: {
        const UgConv c = conv_of(h, p.in_conv, B, S, 0);
        const float* dy = W + p.dT[o.out];
        run_wgrad(c, dy, W + p.x0, W + p.part, D + h->icw, D + h->icb, s);
        if (dx_out) run_dgrad(c, dy, dx_out, nullptr, c.Cin, 0, s);
        break;
      }
      case OP_RES: {
        const ResW& r = *o.r;
        const float* s0 = W + p.T[o.in0].off;
        const float* s1 = o.in1 >= 0 ? W + p.T[o.in1].off : nullptr;
        float* d0 = W + p.dT[o.in0];
        float* d1 = o.in1 >= 0 ? W + p.dT[o.in1] : nullptr;
        const int C0 = p.T[o.in0].C, C1 = o.in1 >= 0 ? p.T[o.in1].C : 0;
        const float* dout = W + p.dT[o.out];
        // conv2 and norm2 (+ dropout)
        const UgAct a2 = act_of(W + o.h1, nullptr, r.cout, 0, B, HW, W + o.mr2, P + r.n2w, P + r.n2b, hdr, o.block,
                                W + p.A);
        launch_ug_gn_act(a2, s);
        const UgConv c2 = conv_of(h, r.c2, B, S, 0);
        run_wgrad(c2, dout, W + p.A, W + p.part, D + r.c2.w_raw, D + r.c2.b, s);
        run_dgrad(c2, dout, W + p.G, nullptr, r.cout, 0, s);
        launch_ug_gn_act_bwd(a2, W + p.G, W + p.DH, nullptr, 0, 0, W + p.pg, W + p.pb, s);
        norm_grads(r.cout, r.n2w, r.n2b);
        // time projection: d temb_out = sum over the pixels of d h1
        launch_ug_rowsum(W + p.DH, B * r.cout, HW, W + p.dtemb, s);
        launch_ug_linear_wgrad(W + p.dtemb, W + p.emb, B, temb, r.cout, 1, D + r.tw, D + r.tb, s);
        launch_ug_linear_dgrad(W + p.dtemb, P + r.tw, B, temb, r.cout, W + p.dsemb, 1, s);
        // conv1 and norm1
        const UgAct a1 = act_of(s0, s1, C0, C1, B, HW, W + o.mr1, P + r.n1w, P + r.n1b, nullptr, o.block, W + p.A);
        launch_ug_gn_act(a1, s);
        const UgConv c1 = conv_of(h, r.c1, B, S, 0);
        run_wgrad(c1, W + p.DH, W + p.A, W + p.part, D + r.c1.w_raw, D + r.c1.b, s);
        run_dgrad(c1, W + p.DH, W + p.G, nullptr, r.cin, 0, s);
        launch_ug_gn_act_bwd(a1, W + p.G, d0, d1, 1, 1, W + p.pg, W + p.pb, s);
        norm_grads(r.cin, r.n1w, r.n1b);
        // skip path
        if (r.has_skip) {
          const float* xr = s0;
          if (C1) {
            launch_ug_gn_act(act_of(s0, s1, C0, C1, B, HW, nullptr, nullptr, nullptr, nullptr, -1, W + p.R), s);
            xr = W + p.R;
          }
          const UgConv ck = conv_of(h, r.sk, B, S, 0);
          run_wgrad(ck, dout, xr, W + p.part, D + r.sk.w_raw, D + r.sk.b, s);
          run_dgrad(ck, dout, d0, d1, C0, 1, s);
        } else {
          launch_ug_split_add(dout, d0, d1, B, C0, C1, HW, s);
        }
        break;
      }
    }
  }
  // time_embed: Linear(mc, temb) -> SiLU -> Linear(temb, temb); every ResBlock's time_mlp starts with SiLU(emb)
  launch_ug_dsilu(W + p.dsemb, W + p.emb, B * temb, s);
  launch_ug_linear_wgrad(W + p.dsemb, W + p.e1, B, temb, temb, 1, D + h->te2w, D + h->te2b, s);
  launch_ug_linear_dgrad(W + p.dsemb, P + h->te2w, B, temb, temb, W + p.de1, 0, s);
  launch_ug_dsilu(W + p.de1, W + p.e1, B * temb, s);
  launch_ug_linear_wgrad(W + p.de1, W + p.emb0, B, mc, temb, 0, D + h->te0w, D + h->te0b, s);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_unet_dropout_mask(rgfm_unet* h, int block, uint64_t seed, float p_drop, int batch, float* out) {
  if (!h || !out || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(RGFM_EINVAL, "p_drop must be in [0, 1)");
  const TrainPlan p = plan_train(h, batch);
  for (const TOp& o : p.ops)
    if (o.kind == OP_RES && o.block == block) {
      launch_ug_mask(out, (size_t)batch * o.r->cout * o.S * o.S, seed, block, p_drop, nullptr);
      HIP_TRY(hipGetLastError());
      return RGFM_OK;
    }
  return fail(RGFM_EINVAL, "block %d out of range (the net has %d ResBlocks)", block, p.nblocks);
}
