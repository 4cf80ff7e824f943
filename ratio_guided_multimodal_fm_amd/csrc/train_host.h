// train_host.h -- host-side pieces the four training passes share (api_train.cpp, api_fmnet_train.cpp,
// api_ratio_train.cpp, api_clf.cpp): the argument checks, the saved state's header, the dense-layer descriptor, and the
// plan of a stack of conv blocks (conv -> norm -> activation -> optional 2x2 max-pool) with the tail of a block's forward
// (block_train.hip) and of its backward.
#pragma once
#include "rgfm_host.h"

// align 0: a null workspace counts as too small; otherwise null and misaligned workspaces are errors of their own
inline int check_train_ws(size_t need, const void* ws, size_t ws_bytes, size_t align = 0) {
  if (align && !ws) return fail(RGFM_EINVAL, "null workspace");
  if (!ws || ws_bytes < need) return fail(RGFM_ENOMEM, "training workspace too small: %zu < %zu bytes", ws_bytes, need);
  if (align && reinterpret_cast<uintptr_t>(ws) % align != 0)
    return fail(RGFM_EINVAL, "the training workspace must be %zu-byte aligned", align);
  return RGFM_OK;
}

inline int check_p_drop(float p) {
  return p >= 0.f && p < 1.f ? RGFM_OK : fail(RGFM_EINVAL, "p_drop must be in [0, 1)");
}

// header words: {p_drop bits, seed lo, seed hi, 0, training}
constexpr int HDR_TRAINING = 4;
inline int write_train_header(unsigned* hdr, int training, float p_drop, uint64_t seed, hipStream_t s) {
  launch_ug_header(hdr, training ? p_drop : 0.f, seed, s);
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(hdr + HDR_TRAINING), training ? 1 : 0, 1, s));
  return RGFM_OK;
}

// one dense layer on fg_gemm_kernel (fmnet_grad.hip); pointers are filled in by the caller
inline FgGemm fg_gemm_of(int M, int N, int K, int lda, int ldb, int ldc, bool split) {
  FgGemm g{};
  g.M = M, g.N = N, g.K = K, g.lda = lda, g.ldb = ldb, g.ldc = ldc;
  g.splits = 1, g.kps = (K + 15) / 16 * 16;
  if (split) fg_split(g);
  return g;
}

// ---- conv blocks of the ratio estimators' encoders and the classifiers
struct TrainBlock {
  size_t w, b;            // blob offsets: conv weight and bias,
  size_t nw, nb, rm, rv;  // the norm's weight and bias, BatchNorm's running_mean and running_var
  bool pool;              // a max-pool behind the activation
  int Cin, C, S, So;      // So: raster of the block's output (S / 2 behind a pool)
  size_t in, z, mr, a, choice;
  size_t stats;  // floats before this layer's pairs in bn_stats_out
};
struct TrainBlockMax {  // running over every stack of a plan: what its scratch regions are sized by
  size_t mx = 1, mxC = 1, mx_part = 1, stats = 0;
};
constexpr int NORM_NONE = -1, NORM_BATCH = 0;  // a positive value: GroupNorm with that many groups

inline UgConv conv_of(const float* params, const TrainBlock& r, int n) {
  UgConv c{};
  c.w = params + r.w, c.bias = params + r.b;
  c.B = n, c.Cin = r.Cin, c.Cout = r.C, c.taps = 9, c.stride = 1, c.up = 0;
  c.Hs = c.Ws = c.Hc = c.Wc = c.Ho = c.Wo = r.S;
  c.C0 = r.Cin;
  c.splits = 1;
  return c;
}

// Lays out a stack of blocks for batch n.  They arrive with their blob offsets, C and pool set, the first one with Cin,
// S and in (its input tensor) as well; take(k) carves k floats of the workspace.  z and the (mean, rstd) pairs mr are
// kept only in front of a norm.
template <class Take>
void plan_blocks(std::vector<TrainBlock>& blocks, int n, Take take, int norm, TrainBlockMax& m) {
  for (size_t i = 0; i < blocks.size(); ++i) {
    TrainBlock& r = blocks[i];
    if (i) r.in = blocks[i - 1].a, r.Cin = blocks[i - 1].C, r.S = blocks[i - 1].So;
    r.So = r.pool ? r.S / 2 : r.S;
    if (norm != NORM_NONE) {
      r.z = take((size_t)n * r.C * r.S * r.S);
      r.mr = take(norm == NORM_BATCH ? (size_t)r.C * 2 : (size_t)n * norm * 2);
    }
    r.a = take((size_t)n * r.C * r.So * r.So);
    r.choice = r.pool ? take(((size_t)n * r.C * r.So * r.So + 3) / 4) : 0;
    r.stats = m.stats;
    m.stats += (size_t)r.C * 2;
    m.mx = std::max(m.mx, (size_t)n * r.C * r.S * r.S);
    m.mxC = std::max(m.mxC, (size_t)r.C);
    UgConv u{};  // (the split follows from the shape alone)
    u.B = n, u.Cin = r.Cin, u.Cout = r.C, u.taps = 9, u.Ho = u.Wo = r.S;
    wgrad_split(u);
    m.mx_part = std::max(m.mx_part, (size_t)u.splits * r.C * r.Cin * 9);
  }
}

// z (the conv's output) in front of the block's norm and activation
inline BtBlock norm_act_of(const TrainBlock& r, int norm, int n, const float* z, const float* params, const float* W) {
  BtBlock a{};
  a.z = z, a.B = n, a.C = r.C, a.H = a.W = r.S, a.groups = std::max(norm, 0);
  if (norm != NORM_NONE) a.mr = W + r.mr, a.gamma = params + r.nw, a.beta = params + r.nb;
  return a;
}

// The tail of a block's forward behind the conv: the norm's (mean, rstd) pairs -- of the batch (BatchNorm in training
// mode, through bnpart, with the pairs bn_stats_out asks for), of the running statistics, or per (sample, group) -- then
// the activation, with the pool where the block has one.
inline void block_tail(BtActKind act, const TrainBlock& r, int norm, int n, bool training, const float* z, const float* params,
                       float* W, size_t bnpart, float* bn_stats_out, hipStream_t s) {
  if (norm > 0) launch_ug_gn_stats(z, nullptr, r.C, 0, n, r.S * r.S, norm, W + r.mr, s);
  else if (norm == NORM_BATCH && training)
    launch_bt_bn_stats(z, n, r.C, r.S * r.S, W + bnpart, W + r.mr, bn_stats_out ? bn_stats_out + r.stats : nullptr, s);
  else if (norm == NORM_BATCH) launch_bt_bn_running(params + r.rm, params + r.rv, r.C, W + r.mr, s);
  launch_bt_act(act, norm_act_of(r, norm, n, z, params, W), W + r.a, r.pool ? (unsigned char*)(W + r.choice) : nullptr, s);
}

// The tail of a block's backward.  cur: the gradient of the conv's output.  The weight and bias gradients go into D; the
// data gradient into dst when there is one -- `other`, which then becomes cur, or the caller's image gradient.
inline void block_grads(const UgConv& c, const TrainBlock& r, float* W, size_t part, float* D, float*& cur, float*& other,
                        float* dst, hipStream_t s) {
  run_wgrad(c, cur, W + r.in, W + part, D + r.w, D + r.b, s);
  if (dst) run_dgrad(c, cur, dst, nullptr, r.Cin, 0, s);
  if (dst == other) std::swap(cur, other);
}
