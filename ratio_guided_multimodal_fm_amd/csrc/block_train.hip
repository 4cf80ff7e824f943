// block_train.hip -- the tail of a training conv block, conv -> (BatchNorm | GroupNorm | nothing) -> activation ->
// optional 2x2 max-pool, and its backward: what the ratio estimators' encoders (SiLU; api_ratio_train.cpp) and the
// evaluation classifiers (ReLU; api_clf.cpp) share behind their convs.
//
//   BatchNorm in training mode: per-channel (count, mean, M2) partials over B*H*W, one per (channel, batch slice),
//     Chan-combined in fp64 in slice order (bt_bn_part_kernel / bt_bn_finalize_kernel); eval mode: bt_bn_running_kernel.
//   y = gamma xhat + beta (or y = z), the activation, and with a pool behind it the 2x2 maximum with the window element
//     taken recorded, one byte per output: bt_act_kernel, bt_act_pool_kernel.  The pool's backward routes the pooled
//     gradient to the recorded element (bt_unpool_kernel), never through a recomputed maximum.
//   BatchNorm + activation backward as a two-pass pair (bt_bn_bwd_part_kernel -> bt_bn_bwd_finalize_kernel ->
//     bt_bn_bwd_apply_kernel).
//
// The activation is a policy type (BtSilu, BtRelu).  ReLU's gate is `stored activation > 0`, as in torch: a value of
// exactly 0 gets no gradient, and behind a pool the gate of the chosen element is `pooled value > 0`.
//
// All tensors are NCHW fp32.  No float atomics: every reduction is a fixed-order loop, an LDS tree or an ordered
// combine of per-workgroup partials, so two calls on the same inputs agree bitwise.  The kernels are memory-bound:
// a thread moves V = 4 consecutive floats with one 16-byte access where the raster allows (rows of 32, 16 and 8;
// 28, 14 and 7 take the V = 1 instantiation), in grid-stride loops capped at 4096 workgroups.  bt_width picks V; the
// instantiations are SiLU at V = 1 and ReLU at V = 1 and 4 (bt_dispatch).
#include <type_traits>

#include "train_device.h"

namespace rgfm {

// fwd: the activation of y.  dy: the gradient of y from the gradient `dout` of the activation; `saved` points at the
// stored activation of the element, or is null when dout is the gradient of y already.
struct BtSilu {
  static __device__ __forceinline__ float fwd(float y) { return ug_silu(y); }
  static __device__ __forceinline__ float dy(float dout, float y, const float*) { return dout * ug_dsilu(y); }
};
struct BtRelu {
  static __device__ __forceinline__ float fwd(float y) { return y > 0.f ? y : 0.f; }
  static __device__ __forceinline__ float dy(float dout, float, const float* saved) {
    return !saved || *saved > 0.f ? dout : 0.f;
  }
};

// V = 4 needs a raster that keeps a thread's floats in one row (`raster`) and 16-byte aligned tensors.  The SiLU side
// stays at 1: the ratio plan does not align its regions, and the part kernel's per-thread summation order -- the bits
// of dgamma, dbeta and dz -- depends on V.  Vectorising it is this line plus that plan change.
static int bt_width(BtActKind act, bool raster, std::initializer_list<const void*> ps) {
  return act != BT_SILU && raster && vec_aligned(ps) ? 4 : 1;
}
// f(activation policy, integral_constant V) for the (activation, width) pairs that exist
template <class F>
static void bt_dispatch(BtActKind act, int V, F f) {
  if (act == BT_SILU) f(BtSilu{}, std::integral_constant<int, 1>{});
  else if (V == 4) f(BtRelu{}, std::integral_constant<int, 4>{});
  else f(BtRelu{}, std::integral_constant<int, 1>{});
}

// (mean, rstd, gamma, beta) of element (b, c): BatchNorm keeps one pair per channel, GroupNorm one per (sample, group);
// the identity without a norm
struct BtAffine {
  float mean, rstd, g, b;
  __device__ __forceinline__ float xhat(float z) const { return (z - mean) * rstd; }
  __device__ __forceinline__ float y(float z) const { return g * xhat(z) + b; }
};
__device__ __forceinline__ BtAffine bt_affine(const BtBlock& a, int b, int c) {
  if (!a.mr) return {0.f, 1.f, 1.f, 0.f};
  const float* m = a.mr + 2 * (a.groups ? b * a.groups + c / (a.C / a.groups) : c);
  return {m[0], m[1], a.gamma[c], a.beta[c]};
}

// ------------------------------------------------------------------ BatchNorm statistics
// part[c][slice] = (count, mean, M2) of channel c over the samples [slice * bper, (slice + 1) * bper); two passes
__global__ __launch_bounds__(256) void bt_bn_part_kernel(const float* z, int B, int C, int HW, int bper, float* part) {
  __shared__ float red[256];
  const int c = blockIdx.x, b0 = blockIdx.y * bper;
  const int n = (min(B, b0 + bper) - b0) * HW;
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) v += z[((size_t)(b0 + i / HW) * C + c) * HW + i % HW];
  const float mean = ug_block_sum(v, red) / (float)n;
  v = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = z[((size_t)(b0 + i / HW) * C + c) * HW + i % HW] - mean;
    v += d * d;
  }
  const float m2 = ug_block_sum(v, red);
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)c * gridDim.y + blockIdx.y) * 3;
    o[0] = (float)n, o[1] = mean, o[2] = m2;
  }
}
// mr[c] = (mean, rstd) with the biased variance (eps 1e-5); stats[c] = (mean, unbiased variance) when asked for
__global__ void bt_bn_finalize_kernel(const float* part, int C, int slices, float* mr, float* stats) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int s = 0; s < slices; ++s) {
    const float* p = part + ((size_t)c * slices + s) * 3;
    const double nb = p[0], delta = (double)p[1] - mean, tot = n + nb;
    mean += delta * nb / tot;
    m2 += (double)p[2] + delta * delta * n * nb / tot;
    n = tot;
  }
  mr[2 * c] = (float)mean, mr[2 * c + 1] = (float)(1.0 / sqrt(m2 / n + 1e-5));
  if (stats) stats[2 * c] = (float)mean, stats[2 * c + 1] = (float)(m2 / (n - 1.0));
}
void launch_bt_bn_stats(const float* z, int B, int C, int HW, float* part, float* mr, float* stats, hipStream_t s) {
  const int bper = (B + BT_BN_SLICES - 1) / BT_BN_SLICES, slices = (B + bper - 1) / bper;
  hipLaunchKernelGGL(bt_bn_part_kernel, dim3(C, slices), dim3(256), 0, s, z, B, C, HW, bper, part);
  hipLaunchKernelGGL(bt_bn_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, s, part, C, slices, mr, stats);
}
// eval mode: mr[c] = (running_mean, 1 / sqrt(running_var + eps))
__global__ void bt_bn_running_kernel(const float* rm, const float* rv, int C, float* mr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) mr[2 * c] = rm[c], mr[2 * c + 1] = 1.0f / sqrtf(rv[c] + 1e-5f);
}
void launch_bt_bn_running(const float* rm, const float* rv, int C, float* mr, hipStream_t s) {
  hipLaunchKernelGGL(bt_bn_running_kernel, dim3((C + 63) / 64), dim3(64), 0, s, rm, rv, C, mr);
}

// ------------------------------------------------------------------ norm + activation (+ max-pool)
// out = act(y), y = z or gamma xhat + beta
template <class Act, int V>
__global__ void bt_act_kernel(BtBlock a, float* out) {
  const int HW = a.H * a.W;
  const size_t groups = (size_t)a.B * a.C * HW / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * V, r = e / HW;
    const BtAffine f = bt_affine(a, (int)(r / a.C), (int)(r % a.C));
    float v[V];
    vec_load<V>(a.z + e, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = Act::fwd(f.y(v[j]));
    vec_store<V>(out + e, v);
  }
}
// out[b][c][yo][xo] = max over the 2x2 window of act(y), floor division of odd rasters; choice = the window element
// taken (row-major 0..3; ties: the first).  A thread owns V consecutive outputs of one row: 2 V inputs of two rows.
template <class Act, int V>
__global__ void bt_act_pool_kernel(BtBlock a, float* out, unsigned char* choice) {
  const int Ho = a.H / 2, Wo = a.W / 2;
  const size_t groups = (size_t)a.B * a.C * Ho * Wo / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = i * V;
    const int xo = (int)(o % Wo);
    size_t r = o / Wo;
    const int yo = (int)(r % Ho);
    r /= Ho;  // b * C + c
    const BtAffine f = bt_affine(a, (int)(r / a.C), (int)(r % a.C));
    const float* zp = a.z + (r * a.H + 2 * yo) * a.W + 2 * xo;
    float top[2 * V], bot[2 * V];
    if constexpr (V == 4) {
      float t[4];
      vec_load<4>(zp, t), top[0] = t[0], top[1] = t[1], top[2] = t[2], top[3] = t[3];
      vec_load<4>(zp + 4, t), top[4] = t[0], top[5] = t[1], top[6] = t[2], top[7] = t[3];
      vec_load<4>(zp + a.W, t), bot[0] = t[0], bot[1] = t[1], bot[2] = t[2], bot[3] = t[3];
      vec_load<4>(zp + a.W + 4, t), bot[4] = t[0], bot[5] = t[1], bot[6] = t[2], bot[7] = t[3];
    } else {
      top[0] = zp[0], top[1] = zp[1], bot[0] = zp[a.W], bot[1] = zp[a.W + 1];
    }
    float best[V];
    unsigned ks = 0u;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float w[4] = {Act::fwd(f.y(top[2 * j])), Act::fwd(f.y(top[2 * j + 1])), Act::fwd(f.y(bot[2 * j])),
                          Act::fwd(f.y(bot[2 * j + 1]))};
      unsigned k = 0u;
      float m = w[0];
#pragma unroll
      for (unsigned q = 1; q < 4; ++q)
        if (w[q] > m) m = w[q], k = q;
      best[j] = m;
      ks |= k << (8 * j);
    }
    vec_store<V>(out + o, best);
    if constexpr (V == 4) *reinterpret_cast<unsigned*>(choice + o) = ks;
    else choice[o] = (unsigned char)ks;
  }
}
void launch_bt_act(BtActKind act, const BtBlock& a, float* out, unsigned char* choice, hipStream_t s) {
  if (choice) {
    const size_t total = (size_t)a.B * a.C * (a.H / 2) * (a.W / 2);
    bt_dispatch(act, bt_width(act, a.W % 8 == 0, {a.z, out, choice}), [&](auto A, auto v) {
      hipLaunchKernelGGL((bt_act_pool_kernel<decltype(A), v.value>), vec_grid(total / v.value), dim3(256), 0, s, a, out, choice);
    });
  } else {
    const size_t total = (size_t)a.B * a.C * a.H * a.W;
    bt_dispatch(act, bt_width(act, (a.H * a.W) % 4 == 0, {a.z, out}), [&](auto A, auto v) {
      hipLaunchKernelGGL((bt_act_kernel<decltype(A), v.value>), vec_grid(total / v.value), dim3(256), 0, s, a, out);
    });
  }
}

// ------------------------------------------------------------------ backward of the max-pool
// full[b][c][y][x] = g[b][c][y / 2][x / 2] where (y, x) is the chosen element -- and, with a gate, the pooled activation
// gate[b][c][y / 2][x / 2] > 0 -- else 0 (the last row / column of an odd raster lies in no window).
// V = 4 (even H, W % 8 == 0): a thread owns 4 consecutive pooled outputs and writes their two rows of 8.
template <int V>
__global__ void bt_unpool_kernel(const float* g, const unsigned char* choice, const float* gate, float* full, int BC,
                                 int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  if constexpr (V == 4) {
    const size_t groups = (size_t)BC * Ho * Wo / 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
      const size_t o = i * 4;
      const int xo = (int)(o % Wo);
      const size_t r = o / Wo;  // bc * Ho + yo
      float gv[4], av[4];
      vec_load<4>(g + o, gv);
      if (gate) vec_load<4>(gate + o, av);
      const unsigned ks = *reinterpret_cast<const unsigned*>(choice + o);
      float row[2][8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned k = (ks >> (8 * j)) & 0xffu;
        const float v = !gate || av[j] > 0.f ? gv[j] : 0.f;
#pragma unroll
        for (unsigned q = 0; q < 4; ++q) row[q >> 1][2 * j + (q & 1)] = k == q ? v : 0.f;
      }
      float* fp = full + 2 * r * W + 2 * xo;  // ((bc * H + 2 yo) * W + 2 xo), H = 2 Ho
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        *reinterpret_cast<f32x4*>(fp + q * W) = f32x4{row[q][0], row[q][1], row[q][2], row[q][3]};
        *reinterpret_cast<f32x4*>(fp + q * W + 4) = f32x4{row[q][4], row[q][5], row[q][6], row[q][7]};
      }
    }
  } else {
    const size_t total = (size_t)BC * H * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
      const int x = (int)(i % W);
      const size_t r = i / W;
      const int y = (int)(r % H);
      const size_t bc = r / H;
      float v = 0.f;
      if (y < 2 * Ho && x < 2 * Wo) {
        const size_t o = (bc * Ho + (y >> 1)) * Wo + (x >> 1);
        if (choice[o] == (unsigned char)((y & 1) * 2 + (x & 1)) && (!gate || gate[o] > 0.f)) v = g[o];
      }
      full[i] = v;
    }
  }
}
void launch_bt_unpool(BtActKind act, const float* g, const unsigned char* choice, const float* gate, float* full, int BC,
                      int H, int W, hipStream_t s) {
  if (bt_width(act, H % 2 == 0 && W % 8 == 0, {g, choice, gate, full}) == 4)
    hipLaunchKernelGGL(bt_unpool_kernel<4>, vec_grid((size_t)BC * (H / 2) * (W / 2) / 4), dim3(256), 0, s, g, choice, gate,
                       full, BC, H, W);
  else
    hipLaunchKernelGGL(bt_unpool_kernel<1>, vec_grid((size_t)BC * H * W), dim3(256), 0, s, g, choice, gate, full, BC, H, W);
}
// out[i] = choice[i] as a float (rgfm_ratio_pool_choice, rgfm_clf_pool_choice)
__global__ void bt_choice_kernel(const unsigned char* choice, size_t n, float* out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (float)choice[i];
}
void launch_bt_choice(const unsigned char* choice, size_t n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(bt_choice_kernel, vec_grid(n), dim3(256), 0, s, choice, n, out);
}

// ------------------------------------------------------------------ BatchNorm + activation backward
// With dy = Act::dy(dout, y, saved), the gradient of y = gamma xhat + beta:  dgamma = sum dy xhat,  dbeta = sum dy  over
// (b, pixel), and
//   training:  dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat))      eval:  dz = gamma rstd dy
__device__ __forceinline__ BtAffine bt_bn_affine(const BtBlock& a, int c) {
  return {a.mr[2 * c], a.mr[2 * c + 1], a.gamma[c], a.beta[c]};
}
// pass 1: part[c][slice] = (sum dy, sum dy xhat) over a batch slice
template <class Act, int V>
__global__ __launch_bounds__(256) void bt_bn_bwd_part_kernel(BtBlock a, const float* dout, const float* saved, int bper,
                                                             float* part) {
  __shared__ float red[256];
  const int c = blockIdx.x, b0 = blockIdx.y * bper, HW = a.H * a.W;
  const int n = (min(a.B, b0 + bper) - b0) * HW / V;
  const BtAffine f = bt_bn_affine(a, c);
  float sb = 0.f, sg = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int e = i * V;
    const size_t o = ((size_t)(b0 + e / HW) * a.C + c) * HW + e % HW;
    float zv[V], dv[V], sv[V];
    vec_load<V>(a.z + o, zv), vec_load<V>(dout + o, dv);
    if (saved) vec_load<V>(saved + o, sv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xh = f.xhat(zv[j]);
      const float dy = Act::dy(dv[j], f.g * xh + f.b, saved ? sv + j : nullptr);
      sb += dy, sg += dy * xh;
    }
  }
  sb = ug_block_sum(sb, red);
  sg = ug_block_sum(sg, red);
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)c * gridDim.y + blockIdx.y) * 2;
    o[0] = sb, o[1] = sg;
  }
}
// slices added in order in fp64: dgamma, dbeta, and m12[c] = (mean(dy), mean(dy xhat)) (zeros in eval mode: the
// forward left its mode in a word of the saved state)
__global__ void bt_bn_bwd_finalize_kernel(const float* part, int C, int slices, float inv_n, const unsigned* training_flag,
                                          float* dgamma, float* dbeta, float* m12) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const bool training = *training_flag != 0u;
  double sb = 0.0, sg = 0.0;
  for (int s = 0; s < slices; ++s) sb += part[((size_t)c * slices + s) * 2], sg += part[((size_t)c * slices + s) * 2 + 1];
  dgamma[c] = (float)sg, dbeta[c] = (float)sb;
  m12[2 * c] = training ? (float)sb * inv_n : 0.f, m12[2 * c + 1] = training ? (float)sg * inv_n : 0.f;
}
// pass 2, in place: dout <- dz
template <class Act, int V>
__global__ void bt_bn_bwd_apply_kernel(BtBlock a, float* dout, const float* saved, const float* m12) {
  const int HW = a.H * a.W;
  const size_t groups = (size_t)a.B * a.C * HW / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * V;
    const int c = (int)((e / HW) % a.C);
    const BtAffine f = bt_bn_affine(a, c);
    const float m1 = m12[2 * c], m2 = m12[2 * c + 1];
    float zv[V], dv[V], sv[V];
    vec_load<V>(a.z + e, zv), vec_load<V>(dout + e, dv);
    if (saved) vec_load<V>(saved + e, sv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xh = f.xhat(zv[j]);
      const float dy = Act::dy(dv[j], f.g * xh + f.b, saved ? sv + j : nullptr);
      dv[j] = f.g * f.rstd * (dy - m1 - xh * m2);
    }
    vec_store<V>(dout + e, dv);
  }
}
void launch_bt_bn_bwd(BtActKind act, const BtBlock& a, float* dout, const float* saved, const unsigned* training, float* part,
                      float* m12, float* dgamma, float* dbeta, hipStream_t s) {
  const int bper = (a.B + BT_BN_SLICES - 1) / BT_BN_SLICES, slices = (a.B + bper - 1) / bper;
  const size_t total = (size_t)a.B * a.C * a.H * a.W;
  bt_dispatch(act, bt_width(act, (a.H * a.W) % 4 == 0, {a.z, dout, saved}), [&](auto A, auto v) {
    hipLaunchKernelGGL((bt_bn_bwd_part_kernel<decltype(A), v.value>), dim3(a.C, slices), dim3(256), 0, s, a, dout, saved, bper,
                       part);
    hipLaunchKernelGGL(bt_bn_bwd_finalize_kernel, dim3((a.C + 63) / 64), dim3(64), 0, s, part, a.C, slices,
                       1.0f / (float)((size_t)a.B * a.H * a.W), training, dgamma, dbeta, m12);
    hipLaunchKernelGGL((bt_bn_bwd_apply_kernel<decltype(A), v.value>), vec_grid(total / v.value), dim3(256), 0, s, a, dout, saved,
                       m12);
  });
}

}  // namespace rgfm
