// api_train.cpp -- training pass of the U-Net handle: the forward that keeps what the backward needs, the backward to
// dx and to every parameter, and the dropout mask hook (C ABI: include/rgfm.h; kernels: unet_grad.hip); and, on the
// same two walks, the likelihood path: J^T u by the data-only reverse walk (rgfm_unet_vjp), the Hutchinson divergence
// (rgfm_unet_divergence) and the reverse-time augmented ODE loop (rgfm_unet_log_prob; kernels: unet_logp.hip).
//
// The walk is the op list of the handle's plan (unet_plan.h: the reference FlexibleUNet.forward,
// src/models/unet_flexible.py:203-261) over NCHW tensors in the caller's workspace, laid out by plan_train, which adds
// to each op only what the training pass owns: first the SAVED state (dropout header, x, the time path, every tensor
// the walk produces, and per ResBlock the group statistics of both norms, the time projection and conv1's output),
// then the backward's SCRATCH (one gradient buffer per produced tensor and a few transient maps).
#include "sampler_host.h"
#include "train_host.h"

namespace {

struct TTensor {  // a produced tensor: float offset into the workspace, channels, square size
  size_t off;
  int C, S;
};

struct TOp {  // an op of the plan + (ResBlocks) the workspace offsets of what the forward saves for the backward
  const UOp* u;
  size_t mr1 = 0, temb = 0, h1 = 0, mr2 = 0;
};

struct TrainPlan {
  std::vector<TTensor> T;  // by the plan's tensor ids
  std::vector<TOp> ops;
  std::vector<size_t> dT;  // gradient buffer of T[i]
  size_t hdr, x0, emb0, e1, emb, mro, saved;
  size_t labels = 0;  // class-conditional handles: the rows' labels as the forward used them (int32 [B])
  size_t dT_begin, dT_end, A, R, G, DH, part, pg, pb, dtemb, dsemb, de1;
  size_t total;  // floats
  ConvW in_conv, out_conv;
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
  if (h->num_classes) p.labels = c.take((size_t)B);  // (an unlabelled handle's layout stays what it was)
  auto part_of = [&](const ConvW& w, int So) {
    UgConv u{};
    u.Cout = w.cout, u.Cin = w.cin, u.taps = w.taps, u.B = B, u.Ho = u.Wo = So;
    wgrad_split(u);
    mx_part = std::max(mx_part, (size_t)u.splits * w.cout * w.cin * w.taps);
  };
  p.in_conv.w_raw = h->icw, p.in_conv.b = h->icb, p.in_conv.cin = d.in_channels, p.in_conv.cout = mc;
  p.out_conv.w_raw = h->ocw, p.out_conv.b = h->ocb, p.out_conv.cin = h->final_ch, p.out_conv.cout = d.in_channels;
  for (const UOp& u : h->ops) {
    TOp o{&u};
    const int S = u.S;
    if (u.kind == UOP_RES) {
      const ResW& r = h->res[u.idx];
      o.mr1 = c.take((size_t)B * groups_of(r.cin) * 2);
      o.temb = c.take((size_t)B * r.cout);
      o.h1 = c.take((size_t)B * r.cout * S * S);
      o.mr2 = c.take((size_t)B * groups_of(r.cout) * 2);
      big(r.cin, S);
      mxC = std::max(mxC, (size_t)r.cin);
      part_of(r.c1, S), part_of(r.c2, S);
      if (r.has_skip) part_of(r.sk, S);
    }
    if (u.out >= 0) {  // (the ops produce the plan's tensors in id order)
      const UTensor& t = h->tensors[u.out];
      p.T.push_back({c.take((size_t)B * t.C * t.S * t.S), t.C, t.S});
      big(t.C, t.S);
    }
    if (u.kind == UOP_IN) part_of(p.in_conv, S);
    if (u.kind == UOP_DOWN) part_of(h->down[u.idx], S / 2);
    if (u.kind == UOP_UP) part_of(h->up[u.idx], 2 * S);
    if (u.kind == UOP_OUT) part_of(p.out_conv, S);
    p.ops.push_back(o);
  }
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

int check_train(const rgfm_unet* h, int batch, void* ws, size_t ws_bytes) {
  if (!h || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  return check_train_ws(plan_train(h, batch).total * sizeof(float), ws, ws_bytes);
}

// The training forward over the planned workspace W.  keep_x: copy x into the saved state (the weight gradient of the
// input conv reads it); the data-only users pass false and the input conv reads the caller's x.
// labels (device int32 [batch], class-conditional handles): emb[b] += label_emb[labels[b]]; null: every row the null label.
int forward_walk(rgfm_unet* h, const float* x, bool keep_x, const float* t_dev, int t_count, float* v_out, int batch,
                 float p_drop, uint64_t seed, float* W, const TrainPlan& p, hipStream_t s, const int* labels = nullptr) {
  const int B = batch, mc = h->mc, temb = h->temb;
  const float* P = h->params;
  unsigned* hdr = (unsigned*)(W + p.hdr);
  launch_ug_header(hdr, p_drop, seed, s);
  const float* x_in = x;
  if (keep_x) {
    HIP_TRY(hipMemcpyAsync(W + p.x0, x, (size_t)B * h->d.in_channels * h->d.img_size * h->d.img_size * sizeof(float),
                           hipMemcpyDeviceToDevice, s));
    x_in = W + p.x0;
  }
  launch_ug_sincos(t_dev, t_count, h->freqs, B, mc, W + p.emb0, s);
  launch_ug_linear(W + p.emb0, P + h->te0w, P + h->te0b, W + p.e1, B, mc, temb, 0, s);
  launch_ug_linear(W + p.e1, P + h->te2w, P + h->te2b, W + p.emb, B, temb, temb, 1, s);
  if (h->num_classes) launch_cfg_label_add(W + p.emb, P + h->lemb, labels, h->num_classes, B, temb, (int*)(W + p.labels), s);
  for (const TOp& o : p.ops) {
    const UOp& u = *o.u;
    const int S = u.S, HW = S * S;
    switch (u.kind) {
      case UOP_IN:
        run_fwd(conv_of(h, p.in_conv, B, S, 0), x_in, W + p.T[u.out].off, nullptr, nullptr, s);
        break;
      case UOP_DOWN:
        run_fwd(conv_of(h, h->down[u.idx], B, S, 1), W + p.T[u.in0].off, W + p.T[u.out].off, nullptr, nullptr, s);
        break;
      case UOP_UP:
        run_fwd(conv_of(h, h->up[u.idx], B, S, 2), W + p.T[u.in0].off, W + p.T[u.out].off, nullptr, nullptr, s);
        break;
      case UOP_OUT: {
        const TTensor& t = p.T[u.in0];
        launch_ug_gn_stats(W + t.off, nullptr, t.C, 0, B, HW, groups_of(t.C), W + p.mro, s);
        launch_ug_gn_act(act_of(W + t.off, nullptr, t.C, 0, B, HW, W + p.mro, P + h->onw, P + h->onb, nullptr, -1,
                                W + p.A), s);
        run_fwd(conv_of(h, p.out_conv, B, S, 0), W + p.A, v_out, nullptr, nullptr, s);
        break;
      }
      case UOP_RES: {
        const ResW& r = h->res[u.idx];
        const float* s0 = W + p.T[u.in0].off;
        const float* s1 = u.in1 >= 0 ? W + p.T[u.in1].off : nullptr;
        const int C0 = p.T[u.in0].C, C1 = u.in1 >= 0 ? p.T[u.in1].C : 0;
        float* out = W + p.T[u.out].off;
        launch_ug_gn_stats(s0, s1, C0, C1, B, HW, groups_of(r.cin), W + o.mr1, s);
        launch_ug_gn_act(act_of(s0, s1, C0, C1, B, HW, W + o.mr1, P + r.n1w, P + r.n1b, nullptr, u.block, W + p.A), s);
        launch_ug_linear(W + p.emb, P + r.tw, P + r.tb, W + o.temb, B, temb, r.cout, 1, s);
        run_fwd(conv_of(h, r.c1, B, S, 0), W + p.A, W + o.h1, W + o.temb, nullptr, s);
        launch_ug_gn_stats(W + o.h1, nullptr, r.cout, 0, B, HW, groups_of(r.cout), W + o.mr2, s);
        launch_ug_gn_act(act_of(W + o.h1, nullptr, r.cout, 0, B, HW, W + o.mr2, P + r.n2w, P + r.n2b, hdr, u.block,
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

// The reverse walk over the state a forward_walk left in W: dv = dL/dv_out -> dL/dx (dx_out, optional).  With D (the
// parameter-gradient blob, state_dict order) it is the whole backward.  D null: the DATA-ONLY walk of rgfm_unet_vjp --
// the same launches on the path to x with the same arguments (so the same dx bits), and nothing else: no weight-gradient
// GEMMs and split reductions, no bias / norm-parameter / time-path gradients, none of the activation recomputes that only
// the weight gradients read.  It leaves the saved state untouched: any number of walks may follow one forward.
int backward_walk(rgfm_unet* h, const float* dv, float* dx_out, float* D, int batch, float* W, const TrainPlan& p,
                  hipStream_t s) {
  const int B = batch, mc = h->mc, temb = h->temb;
  const float* P = h->params;
  const unsigned* hdr = (const unsigned*)(W + p.hdr);
  const bool full = D != nullptr;
  float* pg = full ? W + p.pg : nullptr;
  float* pb = full ? W + p.pb : nullptr;
  if (full) HIP_TRY(hipMemsetAsync(D, 0, h->n_params * sizeof(float), s));
  HIP_TRY(hipMemsetAsync(W + p.dT_begin, 0, (p.dT_end - p.dT_begin) * sizeof(float), s));
  if (full) HIP_TRY(hipMemsetAsync(W + p.dsemb, 0, (size_t)B * temb * sizeof(float), s));
  // dgamma / dbeta of a norm from the per-sample partials
  auto norm_grads = [&](int C, size_t gw, size_t gb) {
    if (!full) return;
    launch_ug_colsum(pg, B, C, D + gw, s);
    launch_ug_colsum(pb, B, C, D + gb, s);
  };
  // weight and bias gradient of a conv; x_act: its input
  auto wgrad = [&](const UgConv& c, const float* dy, const float* x_act, size_t gw, size_t gb) {
    if (full) run_wgrad(c, dy, x_act, W + p.part, D + gw, D + gb, s);
  };
  // the activation a conv consumed, recomputed into its transient buffer: read by that conv's weight gradient alone
  auto recompute = [&](const UgAct& a) {
    if (full) launch_ug_gn_act(a, s);
  };
  for (auto it = p.ops.rbegin(); it != p.ops.rend(); ++it) {
    const TOp& o = *it;
    const UOp& u = *o.u;
    const int S = u.S, HW = S * S;
    switch (u.kind) {
      case UOP_OUT: {
        const TTensor& t = p.T[u.in0];
        const UgAct a = act_of(W + t.off, nullptr, t.C, 0, B, HW, W + p.mro, P + h->onw, P + h->onb, nullptr, -1,
                               W + p.A);
        recompute(a);
        const UgConv c = conv_of(h, p.out_conv, B, S, 0);
        wgrad(c, dv, W + p.A, h->ocw, h->ocb);
        run_dgrad(c, dv, W + p.G, nullptr, t.C, 0, s);
        launch_ug_gn_act_bwd(a, W + p.G, W + p.dT[u.in0], nullptr, 1, 0, pg, pb, s);
        norm_grads(t.C, h->onw, h->onb);
        break;
      }
      case UOP_UP: {
        const ConvW& w = h->up[u.idx];
        const UgConv c = conv_of(h, w, B, S, 2);
        const float* dy = W + p.dT[u.out];
        wgrad(c, dy, W + p.T[u.in0].off, w.w_raw, w.b);
        run_dgrad(c, dy, W + p.G, nullptr, c.Cin, 0, s);  // gradient of the upsampled map (2S x 2S)
        launch_ug_pool2_add(W + p.G, W + p.dT[u.in0], B * c.Cin, S, S, s);
        break;
      }
      case UOP_DOWN: {
        const ConvW& w = h->down[u.idx];
        const UgConv c = conv_of(h, w, B, S, 1);
        const float* dy = W + p.dT[u.out];
        wgrad(c, dy, W + p.T[u.in0].off, w.w_raw, w.b);
        run_dgrad(c, dy, W + p.dT[u.in0], nullptr, c.Cin, 1, s);
        break;
      }
      case UOP_IN: {
        const UgConv c = conv_of(h, p.in_conv, B, S, 0);
        const float* dy = W + p.dT[u.out];
        wgrad(c, dy, W + p.x0, h->icw, h->icb);
        if (dx_out) run_dgrad(c, dy, dx_out, nullptr, c.Cin, 0, s);
        break;
      }
      case UOP_RES: {
        const ResW& r = h->res[u.idx];
        const float* s0 = W + p.T[u.in0].off;
        const float* s1 = u.in1 >= 0 ? W + p.T[u.in1].off : nullptr;
        float* d0 = W + p.dT[u.in0];
        float* d1 = u.in1 >= 0 ? W + p.dT[u.in1] : nullptr;
        const int C0 = p.T[u.in0].C, C1 = u.in1 >= 0 ? p.T[u.in1].C : 0;
        const float* dout = W + p.dT[u.out];
        // conv2 and norm2 (+ dropout)
        const UgAct a2 = act_of(W + o.h1, nullptr, r.cout, 0, B, HW, W + o.mr2, P + r.n2w, P + r.n2b, hdr, u.block,
                                W + p.A);
        recompute(a2);
        const UgConv c2 = conv_of(h, r.c2, B, S, 0);
        wgrad(c2, dout, W + p.A, r.c2.w_raw, r.c2.b);
        run_dgrad(c2, dout, W + p.G, nullptr, r.cout, 0, s);
        launch_ug_gn_act_bwd(a2, W + p.G, W + p.DH, nullptr, 0, 0, pg, pb, s);
        norm_grads(r.cout, r.n2w, r.n2b);
        if (full) {  // time projection: d temb_out = sum over the pixels of d h1
          launch_ug_rowsum(W + p.DH, B * r.cout, HW, W + p.dtemb, s);
          launch_ug_linear_wgrad(W + p.dtemb, W + p.emb, B, temb, r.cout, 1, D + r.tw, D + r.tb, s);
          launch_ug_linear_dgrad(W + p.dtemb, P + r.tw, B, temb, r.cout, W + p.dsemb, 1, s);
        }
        // conv1 and norm1
        const UgAct a1 = act_of(s0, s1, C0, C1, B, HW, W + o.mr1, P + r.n1w, P + r.n1b, nullptr, u.block, W + p.A);
        recompute(a1);
        const UgConv c1 = conv_of(h, r.c1, B, S, 0);
        wgrad(c1, W + p.DH, W + p.A, r.c1.w_raw, r.c1.b);
        run_dgrad(c1, W + p.DH, W + p.G, nullptr, r.cin, 0, s);
        launch_ug_gn_act_bwd(a1, W + p.G, d0, d1, 1, 1, pg, pb, s);
        norm_grads(r.cin, r.n1w, r.n1b);
        // skip path
        if (r.has_skip) {
          const float* xr = s0;
          if (C1 && full) {  // the concatenated block input: the skip conv's weight gradient reads it
            launch_ug_gn_act(act_of(s0, s1, C0, C1, B, HW, nullptr, nullptr, nullptr, nullptr, -1, W + p.R), s);
            xr = W + p.R;
          }
          const UgConv ck = conv_of(h, r.sk, B, S, 0);
          wgrad(ck, dout, xr, r.sk.w_raw, r.sk.b);
          run_dgrad(ck, dout, d0, d1, C0, 1, s);
        } else {
          launch_ug_split_add(dout, d0, d1, B, C0, C1, HW, s);
        }
        break;
      }
    }
  }
  if (full) {
    // time_embed: Linear(mc, temb) -> SiLU -> Linear(temb, temb); every ResBlock's time_mlp starts with SiLU(emb)
    launch_ug_dsilu(W + p.dsemb, W + p.emb, B * temb, s);
    // label_emb: emb[b] = time_embed(..)[b] + E[y_b], so dE[c] collects the rows of d emb whose label is c
    if (h->num_classes)
      launch_cfg_label_grad(W + p.dsemb, (const int*)(W + p.labels), h->num_classes, B, temb, D + h->lemb, s);
    launch_ug_linear_wgrad(W + p.dsemb, W + p.e1, B, temb, temb, 1, D + h->te2w, D + h->te2b, s);
    launch_ug_linear_dgrad(W + p.dsemb, P + h->te2w, B, temb, temb, W + p.de1, 0, s);
    launch_ug_dsilu(W + p.de1, W + p.e1, B * temb, s);
    launch_ug_linear_wgrad(W + p.de1, W + p.emb0, B, mc, temb, 0, D + h->te0w, D + h->te0b, s);
  }
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

size_t image_floats(const rgfm_unet* h) { return (size_t)h->d.in_channels * h->d.img_size * h->d.img_size; }

// ------------------------------------------------------------------ likelihood path
// One stage of the augmented ODE on the planned training workspace W: v = model(x, t) by the exact-fp32 forward, then
// per probe k one data-only reverse walk g = J^T eps_k and acc[b] (+)= scale <eps_k[b], g[b]>  (g: [B][d] scratch).
// first_overwrites: probe 0 overwrites acc (rgfm_unet_divergence) instead of adding to it (the loop's integral).
int divergence_stage(rgfm_unet* h, const float* x, const float* t_dev, int t_count, const float* eps, int n_probes,
                     float* v_out, float* acc, float scale, bool first_overwrites, int batch, float* W,
                     const TrainPlan& p, float* g, hipStream_t s) {
  if (int rc = forward_walk(h, x, false, t_dev, t_count, v_out, batch, 0.f, 0, W, p, s)) return rc;
  const size_t n = (size_t)batch * image_floats(h);
  for (int k = 0; k < n_probes; ++k) {
    const float* e = eps + (size_t)k * n;
    if (int rc = backward_walk(h, e, g, nullptr, batch, W, p, s)) return rc;
    launch_ul_rowdot(e, g, batch, (int)image_floats(h), scale, !(first_overwrites && k == 0), acc, s);
  }
  return RGFM_OK;
}

// workspace of rgfm_unet_divergence: the training plan, then g [B][d] and a v [B][d] for a caller without v_out
size_t divergence_floats(const rgfm_unet* h, int batch) {
  return plan_train(h, batch).total + 2 * (size_t)batch * image_floats(h);
}

// workspace of rgfm_unet_log_prob, in floats
struct LogpPlan {
  size_t tt, A, xa, xb, xm, k, g, train, total;
};
LogpPlan plan_logp(const rgfm_unet* h, int batch, int solver, int n_probes) {
  LogpPlan q{};
  Cursor c;
  const size_t n = (size_t)batch * image_floats(h);
  q.tt = c.take(4096);  // the time table of a call, as in the sampler loops: one row per Euler step, two per midpoint step
  q.A = c.take(((size_t)batch + 63) & ~(size_t)63);
  q.xa = c.take(n), q.xb = c.take(n);
  q.xm = solver == SOLVER_MIDPOINT ? c.take(n) : 0;
  q.k = c.take(n);
  q.g = n_probes > 0 ? c.take(n) : 0;
  q.train = c.take(plan_train(h, batch).total);
  q.total = c.off;
  return q;
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
  if (int rc = check_train(h, batch, ws, ws_bytes)) return rc;
  if (!x || !t_dev || !v_out || (t_count != 1 && t_count != batch)) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = check_p_drop(p_drop)) return rc;
  return forward_walk(h, x, true, t_dev, t_count, v_out, batch, p_drop, seed, (float*)ws, plan_train(h, batch),
                      (hipStream_t)stream);
}

extern "C" int rgfm_unet_forward_train_labels(rgfm_unet* h, const float* x, const float* t_dev, int t_count,
                                              const int32_t* labels_dev, float* v_out, int batch, float p_drop, uint64_t seed,
                                              void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_train(h, batch, ws, ws_bytes)) return rc;
  if (!x || !t_dev || !v_out || (t_count != 1 && t_count != batch)) return fail(RGFM_EINVAL, "bad argument");
  if (labels_dev && !h->num_classes) return fail(RGFM_EINVAL, "labels on a handle without classes (rgfm_unet_labeled_create makes one)");
  if (int rc = check_p_drop(p_drop)) return rc;
  return forward_walk(h, x, true, t_dev, t_count, v_out, batch, p_drop, seed, (float*)ws, plan_train(h, batch),
                      (hipStream_t)stream, labels_dev);
}

extern "C" int rgfm_unet_backward(rgfm_unet* h, const float* dv, float* dx_out, float* dparams_out, int batch,
                                  void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_train(h, batch, ws, ws_bytes)) return rc;
  if (!dv || !dparams_out) return fail(RGFM_EINVAL, "bad argument");
  return backward_walk(h, dv, dx_out, dparams_out, batch, (float*)ws, plan_train(h, batch), (hipStream_t)stream);
}

extern "C" int rgfm_unet_vjp(rgfm_unet* h, const float* u, float* dx_out, int batch, void* ws, size_t ws_bytes,
                             rgfm_stream_t stream) {
  if (int rc = check_train(h, batch, ws, ws_bytes)) return rc;
  if (!u || !dx_out) return fail(RGFM_EINVAL, "bad argument");
  return backward_walk(h, u, dx_out, nullptr, batch, (float*)ws, plan_train(h, batch), (hipStream_t)stream);
}

extern "C" int rgfm_unet_divergence_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes) {
  if (!h || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  *bytes = divergence_floats(h, batch) * sizeof(float);
  return RGFM_OK;
}

extern "C" int rgfm_unet_divergence(rgfm_unet* h, const float* x, const float* t_dev, int t_count, const float* eps,
                                    int n_probes, float* v_out, float* div_out, int batch, void* ws, size_t ws_bytes,
                                    rgfm_stream_t stream) {
  if (!h || !x || !t_dev || !ws || batch < 1 || n_probes < 0 || (t_count != 1 && t_count != batch))
    return fail(RGFM_EINVAL, "bad argument");
  if (n_probes > 0 && (!eps || !div_out)) return fail(RGFM_EINVAL, "eps and div_out are needed with n_probes > 0");
  const size_t need = divergence_floats(h, batch) * sizeof(float);
  if (ws_bytes < need) return fail(RGFM_ENOMEM, "divergence workspace too small: %zu < %zu bytes", ws_bytes, need);
  const TrainPlan p = plan_train(h, batch);
  float* W = (float*)ws;
  float* g = W + p.total;
  float* v = v_out ? v_out : g + (size_t)batch * image_floats(h);
  return divergence_stage(h, x, t_dev, t_count, eps, n_probes, v, div_out, (float)(1.0 / std::max(n_probes, 1)), true,
                          batch, W, p, g, (hipStream_t)stream);
}

extern "C" int rgfm_unet_log_prob_workspace_bytes(const rgfm_unet* h, int batch, int solver, int n_probes,
                                                  size_t* bytes) {
  if (!h || !bytes || batch < 1 || n_probes < 0) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = check_solver(solver, 0, 1)) return rc;
  *bytes = plan_logp(h, batch, solver, n_probes).total * sizeof(float);
  return RGFM_OK;
}

extern "C" int rgfm_unet_log_prob(rgfm_unet* h, const float* x, const float* eps, int n_probes, int num_steps,
                                  int solver, float* z_out, float* logp_out, int batch, void* ws, size_t ws_bytes,
                                  rgfm_stream_t stream) {
  if (!h || !x || !z_out || !ws || batch < 1 || n_probes < 0 || num_steps < 1) return fail(RGFM_EINVAL, "bad argument");
  if (n_probes > 0 && (!eps || !logp_out)) return fail(RGFM_EINVAL, "eps and logp_out are needed with n_probes > 0");
  if (int rc = check_solver(solver, num_steps, num_steps)) return rc;
  const LogpPlan q = plan_logp(h, batch, solver, n_probes);
  if (ws_bytes < q.total * sizeof(float))
    return fail(RGFM_ENOMEM, "log_prob workspace too small: %zu < %zu bytes", ws_bytes, q.total * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  const TrainPlan p = plan_train(h, batch);
  const int B = batch, N = num_steps, K = n_probes;
  const size_t n = (size_t)B * image_floats(h);
  float* Q = (float*)ws;
  float* W = Q + q.train;
  float* A = Q + q.A;
  float* k = Q + q.k;
  float* g = Q + q.g;
  const bool mid = solver == SOLVER_MIDPOINT;
  launch_ul_times(Q + q.tt, N, mid, s);
  if (K > 0) HIP_TRY(hipMemsetAsync(A, 0, (size_t)B * sizeof(float), s));
  const double dtd = 1.0 / (double)N;
  const float dt = (float)dtd, dth = (float)(0.5 * dtd);
  const float wdiv = (float)(dtd / (double)std::max(K, 1));  // A += dt (1 / K) sum_k <eps_k, J^T eps_k>
  // the state is read from one buffer and written to another: x on the first step, z_out on the last, the two
  // ping-pong buffers between them
  const float* cur = x;
  for (int j = 0; j < N; ++j) {  // step i = N - 1 - j
    float* nxt = j == N - 1 ? z_out : (j & 1 ? Q + q.xb : Q + q.xa);
    const float* at = cur;
    const float* t = Q + q.tt + (mid ? 2 * j : j);
    if (mid) {  // stage 1: a forward without a reverse walk
      if (int rc = forward_walk(h, cur, false, t, 1, k, B, 0.f, 0, W, p, s)) return rc;
      launch_ul_step(cur, k, dth, n, Q + q.xm, s);
      at = Q + q.xm, t += 1;
    }
    if (int rc = divergence_stage(h, at, t, 1, eps, K, k, A, wdiv, false, B, W, p, g, s)) return rc;
    launch_ul_step(cur, k, dt, n, nxt, s);
    cur = nxt;
  }
  if (K > 0) launch_ul_gauss_logp(z_out, A, B, (int)image_floats(h), logp_out, s);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_unet_dropout_mask(rgfm_unet* h, int block, uint64_t seed, float p_drop, int batch, float* out) {
  if (!h || !out || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = check_p_drop(p_drop)) return rc;
  for (const UOp& o : h->ops)
    if (o.kind == UOP_RES && o.block == block) {
      launch_ug_mask(out, (size_t)batch * h->res[o.idx].cout * o.S * o.S, seed, block, p_drop, nullptr);
      HIP_TRY(hipGetLastError());
      return RGFM_OK;
    }
  return fail(RGFM_EINVAL, "block %d out of range (the net has %d ResBlocks)", block, (int)h->res.size());
}
