// api_fmnet_train.cpp -- training pass of the FlowMatchingModel handle: the forward that keeps what the backward needs,
// the backward to dx and to every parameter, and the in-place parameter refresh (C ABI: include/rgfm.h; kernels:
// unet_grad.hip for the convs, transposed convs and GroupNorm, fmnet_grad.hip for the two wide Linears).
//
// The walk is the reference FlowMatchingModel.forward (src/models/flow_matching.py:153-173) over NCHW tensors in the
// caller's workspace, laid out by plan_train: first the SAVED state -- x, every layer's raw output (the pre-norm maps
// z1..z4 and u1..u3, and fc1's map, which deconv1 consumes without a norm), the group (mean, rstd) pairs of the seven
// GroupNorms and the [features | t_emb] concat -- then the backward's SCRATCH.  GroupNorm + SiLU is re-applied into a
// transient buffer right before its consumer, in the backward too.
//
// ConvTranspose2d(k 4, s 2, p 1) with weight [Cin][Cout][4][4] is the data gradient of the 4x4 stride-2 pad-1 conv
// E: [Cout][2S][2S] -> [Cin][S][S] whose weight [E.Cout = Cin][E.Cin = Cout][16] is the same array.  So on
// ug_igemm_kernel: its forward is E's op 1 (fed the layer's input as `dy`, plus the bias), its data gradient E's op 0
// (fed the output gradient as `x`), its weight gradient E's op 2 with the two exchanged.
#include "train_host.h"

namespace {

struct FmTrainPlan {
  size_t x0, z[4], mre[4], comb, d0, u[3], mrd[3], saved;
  size_t A, G, DZ, dfeat, part, pg, pb;
  size_t total;  // floats
};

// the eight convs of the net as ug_igemm_kernel sees them
struct FmConvs {
  UgConv c1, ec[3], d1, d2, c3, co;
};

UgConv fm_conv(const rgfm_fmnet* h, size_t w, size_t b, int cin, int cout, int B, int S, int stride) {
  UgConv c{};
  c.w = h->params + w, c.bias = h->params + b;
  c.B = B, c.Cin = cin, c.Cout = cout, c.taps = 9, c.stride = stride;
  c.Hs = c.Ws = c.Hc = c.Wc = S;
  c.Ho = c.Wo = S / stride;
  c.C0 = cin, c.splits = 1;
  return c;
}
// the conv E of a transposed conv `w` whose input is S x S (see the head of this file); no bias of its own
UgConv fm_deconv(const rgfm_fmnet* h, const ConvW& w, int B, int S) {
  UgConv c{};
  c.w = h->params + w.w_raw;
  c.B = B, c.Cin = w.cout, c.Cout = w.cin, c.taps = 16, c.stride = 2;
  c.Hs = c.Ws = c.Hc = c.Wc = 2 * S;
  c.Ho = c.Wo = S;
  c.C0 = c.Cin, c.splits = 1;
  return c;
}
FmConvs fm_convs(const rgfm_fmnet* h, int B) {
  FmConvs v;
  v.c1 = fm_conv(h, h->c1w, h->c1b, h->d.img_channels, 32, B, FM_S, 1);
  v.ec[0] = fm_conv(h, h->ec[0].w_raw, h->ec[0].b, 32, 64, B, 28, 2);
  v.ec[1] = fm_conv(h, h->ec[1].w_raw, h->ec[1].b, 64, 128, B, 14, 2);
  v.ec[2] = fm_conv(h, h->ec[2].w_raw, h->ec[2].b, 128, 256, B, 7, 1);
  v.d1 = fm_deconv(h, h->d1, B, 7);
  v.d2 = fm_deconv(h, h->d2, B, 14);
  v.c3 = fm_conv(h, h->c3.w_raw, h->c3.b, 64, 32, B, FM_S, 1);
  v.co = fm_conv(h, h->cow, h->cob, 32, h->d.img_channels, B, FM_S, 1);
  return v;
}

// the six GEMMs of the two Linears
constexpr int FM_FLAT = FM_CF * FM_P;  // 12544
FgGemm fc_fwd(int B, int F, int T) { return fg_gemm_of(B, F, FM_FLAT, FM_FLAT, FM_FLAT, F + T, true); }
FgGemm fc_dgrad(int B, int F) { return fg_gemm_of(B, FM_FLAT, F, F, FM_FLAT, FM_FLAT, false); }
FgGemm fc_wgrad(int B, int F) { return fg_gemm_of(F, FM_FLAT, B, F, FM_FLAT, FM_FLAT, false); }
FgGemm fc1_fwd(int B, int F, int T) { return fg_gemm_of(B, FM_FLAT, F + T, F + T, F + T, FM_FLAT, false); }
// (only the first F columns of the concat's gradient exist: t has none)
FgGemm fc1_dgrad(int B, int F, int T) { return fg_gemm_of(B, F, FM_FLAT, FM_FLAT, F + T, F, true); }
FgGemm fc1_wgrad(int B, int F, int T) { return fg_gemm_of(FM_FLAT, F + T, B, FM_FLAT, F + T, F + T, false); }

FmTrainPlan plan_train(const rgfm_fmnet* h, int B) {
  FmTrainPlan p;
  Cursor c;
  auto take = [&](size_t n) { return c.take((n + 3) & ~(size_t)3); };  // (16-byte rows for fg_gemm_kernel's loads)
  const int F = h->d.feature_dim, T = h->d.time_emb_dim;
  const size_t zc[4] = {32 * 784, 64 * 196, 128 * 49, 256 * 49}, uc[3] = {128 * 196, 64 * 784, 32 * 784};
  p.x0 = take((size_t)B * h->d.img_channels * 784);
  for (int i = 0; i < 4; ++i) p.z[i] = take(B * zc[i]), p.mre[i] = take((size_t)B * 16);
  p.comb = take((size_t)B * (F + T));
  p.d0 = take((size_t)B * FM_FLAT);
  for (int i = 0; i < 3; ++i) p.u[i] = take(B * uc[i]), p.mrd[i] = take((size_t)B * 16);
  p.saved = c.off;
  const size_t mx = (size_t)B * 64 * 784;  // the largest map (u2)
  p.A = take(mx), p.G = take(mx), p.DZ = take(mx);
  p.dfeat = take((size_t)B * F);
  size_t mx_part = 1;
  FmConvs v = fm_convs(h, B);
  for (UgConv* u : {&v.c1, &v.ec[0], &v.ec[1], &v.ec[2], &v.d1, &v.d2, &v.c3, &v.co}) {
    wgrad_split(*u);
    mx_part = std::max(mx_part, (size_t)u->splits * u->Cout * u->Cin * u->taps);
  }
  for (const FgGemm& g : {fc_fwd(B, F, T), fc1_dgrad(B, F, T)}) mx_part = std::max(mx_part, (size_t)g.splits * g.M * g.N);
  p.part = take(mx_part);
  p.pg = take((size_t)B * 256), p.pb = take((size_t)B * 256);
  p.total = c.off;
  return p;
}

UgAct act_of(const float* z, int C, int B, int HW, const float* mr, const float* gamma, const float* beta, float* out) {
  UgAct a{};
  a.s0 = z, a.C0 = C, a.B = B, a.HW = HW, a.groups = 8;
  a.mr = mr, a.gamma = gamma, a.beta = beta, a.block = -1, a.out = out;
  return a;
}

int check_train(const rgfm_fmnet* h, int batch, void* ws, size_t ws_bytes) {
  if (!h || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  return check_train_ws(plan_train(h, batch).total * sizeof(float), ws, ws_bytes);
}

// weight gradient of a transposed conv: E's op 2 with the layer's input as `dy` and the output gradient as `x`; the
// bias gradient sums the output gradient
void run_deconv_wgrad(UgConv e, const float* in, const float* dout, float* part, float* dw, float* db, hipStream_t s) {
  e.dy = in, e.x = dout, e.part = part;
  wgrad_split(e);
  launch_ug_conv(e, 2, s);
  launch_ug_reduce(part, e.splits, (size_t)e.Cout * e.Cin * e.taps, dw, s);
  launch_ug_bias_grad(dout, e.B, e.Cin, e.Hc * e.Wc, db, s);
}

}  // namespace

extern "C" int rgfm_fmnet_train_workspace_bytes(const rgfm_fmnet* h, int batch, size_t* bytes) {
  if (!h || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  *bytes = plan_train(h, batch).total * sizeof(float);
  return RGFM_OK;
}

extern "C" int rgfm_fmnet_forward_train(rgfm_fmnet* h, const float* x, const float* t_dev, int t_count, float* v_out,
                                        int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_train(h, batch, ws, ws_bytes)) return rc;
  if (!x || !t_dev || !v_out || (t_count != 1 && t_count != batch)) return fail(RGFM_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const FmTrainPlan p = plan_train(h, batch);
  const FmConvs cv = fm_convs(h, batch);
  const int B = batch, F = h->d.feature_dim, T = h->d.time_emb_dim;
  float* W = (float*)ws;
  const float* P = h->params;
  HIP_TRY(hipMemcpyAsync(W + p.x0, x, (size_t)B * h->d.img_channels * 784 * sizeof(float), hipMemcpyDeviceToDevice, s));
  // ImageEncoder.forward (:56-72)
  const int ech[4] = {32, 64, 128, 256}, ehw[4] = {784, 196, 49, 49};
  run_fwd(cv.c1, W + p.x0, W + p.z[0], nullptr, nullptr, s);
  for (int i = 0; i < 4; ++i) {
    launch_ug_gn_stats(W + p.z[i], nullptr, ech[i], 0, B, ehw[i], 8, W + p.mre[i], s);
    launch_ug_gn_act(act_of(W + p.z[i], ech[i], B, ehw[i], W + p.mre[i], P + h->egw[i], P + h->egb[i], W + p.A), s);
    if (i < 3) run_fwd(cv.ec[i], W + p.A, W + p.z[i + 1], nullptr, nullptr, s);
  }
  FgGemm g = fc_fwd(B, F, T);  // features into the first F columns of the concat (:110)
  g.a = W + p.A, g.b = P + h->fcw, g.bias = P + h->fcb, g.c = W + p.comb, g.part = W + p.part;
  launch_fg_gemm(g, false, false, s);
  launch_fm_time_embed(t_dev, t_count, 1, 0, h->freqs, W + p.comb, B, T, F + T, F, s);
  // VelocityDecoder.forward (:100-124)
  g = fc1_fwd(B, F, T);
  g.a = W + p.comb, g.b = P + h->f1w, g.bias = P + h->f1b, g.c = W + p.d0;
  launch_fg_gemm(g, false, false, s);
  UgConv e = cv.d1;
  e.dbias = P + h->d1.b;
  run_dgrad(e, W + p.d0, W + p.u[0], nullptr, e.Cin, 0, s);
  launch_ug_gn_stats(W + p.u[0], nullptr, 128, 0, B, 196, 8, W + p.mrd[0], s);
  launch_ug_gn_act(act_of(W + p.u[0], 128, B, 196, W + p.mrd[0], P + h->dgw[0], P + h->dgb[0], W + p.A), s);
  e = cv.d2;
  e.dbias = P + h->d2.b;
  run_dgrad(e, W + p.A, W + p.u[1], nullptr, e.Cin, 0, s);
  launch_ug_gn_stats(W + p.u[1], nullptr, 64, 0, B, 784, 8, W + p.mrd[1], s);
  launch_ug_gn_act(act_of(W + p.u[1], 64, B, 784, W + p.mrd[1], P + h->dgw[1], P + h->dgb[1], W + p.A), s);
  run_fwd(cv.c3, W + p.A, W + p.u[2], nullptr, nullptr, s);
  launch_ug_gn_stats(W + p.u[2], nullptr, 32, 0, B, 784, 8, W + p.mrd[2], s);
  launch_ug_gn_act(act_of(W + p.u[2], 32, B, 784, W + p.mrd[2], P + h->dgw[2], P + h->dgb[2], W + p.A), s);
  run_fwd(cv.co, W + p.A, v_out, nullptr, nullptr, s);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_fmnet_backward(rgfm_fmnet* h, const float* dv, float* dx_out, float* dparams_out, int batch,
                                   void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_train(h, batch, ws, ws_bytes)) return rc;
  if (!dv || !dparams_out) return fail(RGFM_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const FmTrainPlan p = plan_train(h, batch);
  const FmConvs cv = fm_convs(h, batch);
  const int B = batch, F = h->d.feature_dim, T = h->d.time_emb_dim;
  float* W = (float*)ws;
  const float* P = h->params;
  float* D = dparams_out;  // (every slot is written below: nothing to clear)
  // the norm in front of a consumer: re-applied into A; then, given the consumer's input gradient in G, the gradient
  // of the norm's input into DZ and dgamma / dbeta from the per-sample partials
  auto norm_bwd = [&](const UgAct& a, size_t gw, size_t gb) {
    launch_ug_gn_act_bwd(a, W + p.G, W + p.DZ, nullptr, 0, 0, W + p.pg, W + p.pb, s);
    launch_ug_colsum(W + p.pg, B, a.C0, D + gw, s);
    launch_ug_colsum(W + p.pb, B, a.C0, D + gb, s);
  };
  // ---- VelocityDecoder, backwards
  UgAct a = act_of(W + p.u[2], 32, B, 784, W + p.mrd[2], P + h->dgw[2], P + h->dgb[2], W + p.A);
  launch_ug_gn_act(a, s);
  run_wgrad(cv.co, dv, W + p.A, W + p.part, D + h->cow, D + h->cob, s);
  run_dgrad(cv.co, dv, W + p.G, nullptr, 32, 0, s);
  norm_bwd(a, h->dgw[2], h->dgb[2]);  // DZ = d u3
  a = act_of(W + p.u[1], 64, B, 784, W + p.mrd[1], P + h->dgw[1], P + h->dgb[1], W + p.A);
  launch_ug_gn_act(a, s);
  run_wgrad(cv.c3, W + p.DZ, W + p.A, W + p.part, D + h->c3.w_raw, D + h->c3.b, s);
  run_dgrad(cv.c3, W + p.DZ, W + p.G, nullptr, 64, 0, s);
  norm_bwd(a, h->dgw[1], h->dgb[1]);  // DZ = d u2
  a = act_of(W + p.u[0], 128, B, 196, W + p.mrd[0], P + h->dgw[0], P + h->dgb[0], W + p.A);
  launch_ug_gn_act(a, s);
  run_deconv_wgrad(cv.d2, W + p.A, W + p.DZ, W + p.part, D + h->d2.w_raw, D + h->d2.b, s);
  run_fwd(cv.d2, W + p.DZ, W + p.G, nullptr, nullptr, s);
  norm_bwd(a, h->dgw[0], h->dgb[0]);  // DZ = d u1
  run_deconv_wgrad(cv.d1, W + p.d0, W + p.DZ, W + p.part, D + h->d1.w_raw, D + h->d1.b, s);
  run_fwd(cv.d1, W + p.DZ, W + p.G, nullptr, nullptr, s);  // G = d (fc1 output) [B][12544]
  FgGemm g = fc1_wgrad(B, F, T);
  g.a = W + p.G, g.b = W + p.comb, g.c = D + h->f1w;
  launch_fg_gemm(g, true, true, s);
  launch_ug_colsum(W + p.G, B, FM_FLAT, D + h->f1b, s);
  g = fc1_dgrad(B, F, T);
  g.a = W + p.G, g.b = P + h->f1w, g.c = W + p.dfeat, g.part = W + p.part;
  launch_fg_gemm(g, false, true, s);
  // ---- ImageEncoder, backwards
  const int ech[4] = {32, 64, 128, 256}, ehw[4] = {784, 196, 49, 49};
  a = act_of(W + p.z[3], 256, B, 49, W + p.mre[3], P + h->egw[3], P + h->egb[3], W + p.A);
  launch_ug_gn_act(a, s);
  g = fc_wgrad(B, F);
  g.a = W + p.dfeat, g.b = W + p.A, g.c = D + h->fcw;
  launch_fg_gemm(g, true, true, s);
  launch_ug_colsum(W + p.dfeat, B, F, D + h->fcb, s);
  g = fc_dgrad(B, F);
  g.a = W + p.dfeat, g.b = P + h->fcw, g.c = W + p.G;
  launch_fg_gemm(g, false, true, s);
  norm_bwd(a, h->egw[3], h->egb[3]);  // DZ = d z4
  for (int i = 2; i >= 0; --i) {
    a = act_of(W + p.z[i], ech[i], B, ehw[i], W + p.mre[i], P + h->egw[i], P + h->egb[i], W + p.A);
    launch_ug_gn_act(a, s);
    run_wgrad(cv.ec[i], W + p.DZ, W + p.A, W + p.part, D + h->ec[i].w_raw, D + h->ec[i].b, s);
    run_dgrad(cv.ec[i], W + p.DZ, W + p.G, nullptr, ech[i], 0, s);
    norm_bwd(a, h->egw[i], h->egb[i]);  // DZ = d z(i+1)
  }
  run_wgrad(cv.c1, W + p.DZ, W + p.x0, W + p.part, D + h->c1w, D + h->c1b, s);
  if (dx_out) run_dgrad(cv.c1, W + p.DZ, dx_out, nullptr, cv.c1.Cin, 0, s);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_fmnet_update_params(rgfm_fmnet* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream) {
  if (!h || !params_dev) return fail(RGFM_EINVAL, "null argument");
  if (n_floats != h->n_params) return fail(RGFM_EINVAL, "parameter blob has %zu floats, the handle has %zu", n_floats, h->n_params);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(h->params, params_dev, n_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
  return fm_pack_weights(h, s);
}
