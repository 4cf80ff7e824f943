// clf_train.hip -- training pass of the evaluation classifiers (reference src/models/classifier.py:9-52,
// src/models/svhn_classifier.py:11-116): what the other training kernels do not cover.
//
//   ReLU (behind an optional BatchNorm) with an optional 2x2 max-pool that records the window element taken, one byte
//     per output: ct_act_kernel, ct_act_pool_kernel; their backward -- the pooled gradient routed to the chosen element
//     and multiplied by the gate -- ct_unpool_gate_kernel, ct_gate_kernel.  The gate is `value > 0`, as in torch: a
//     value of exactly 0 gets no gradient.  Behind a pool the gate of the chosen element is `pooled value > 0`.
//   BatchNorm + ReLU backward as a two-pass pair (ct_bn_bwd_part_kernel -> rt_bn_bwd_finalize_kernel of ratio_train.hip
//     -> ct_bn_bwd_apply_kernel): the formulas of ratio_train.hip with the ReLU gate in place of silu'.
//   ReLU + dropout behind fc1 and its backward (the counter hash ug_keep, Dropout layer 0).
//   Softmax cross-entropy with its gradient and the predicted class: ct_xent_kernel, one lane per row.
//
// All tensors are NCHW fp32.  No float atomics: every reduction is a fixed-order loop, an LDS tree or an ordered
// combine of per-workgroup partials, so two calls on the same inputs agree bitwise.  The kernels are memory-bound:
// a thread moves V = 4 consecutive floats with one 16-byte access where the raster allows (rows of 32, 16 and 8;
// 28, 14 and 7 take the V = 1 instantiation), in grid-stride loops capped at 4096 workgroups.  The convs, the Linear
// layers and the BatchNorm statistics run on the kernels of unet_grad.hip, fmnet_grad.hip and ratio_train.hip.
#include <initializer_list>

#include "train_device.h"

namespace rgfm {

template <int V>
__device__ __forceinline__ void ct_load(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void ct_store(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}
__device__ __forceinline__ float ct_relu(float v) { return v > 0.f ? v : 0.f; }

static bool ct_aligned(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}
static dim3 ct_grid(size_t groups) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((groups + 255) / 256, 4096))); }

// (mean, rstd, gamma, beta) of channel c; the identity without a norm
struct CtAffine {
  float mean, rstd, g, b;
  __device__ __forceinline__ float xhat(float z) const { return (z - mean) * rstd; }
  __device__ __forceinline__ float y(float z) const { return g * xhat(z) + b; }
};
__device__ __forceinline__ CtAffine ct_affine(const CtAct& a, int c) {
  if (!a.mr) return {0.f, 1.f, 1.f, 0.f};
  return {a.mr[2 * c], a.mr[2 * c + 1], a.gamma[c], a.beta[c]};
}

// ------------------------------------------------------------------ ReLU (+ BatchNorm) (+ max-pool)
// out = relu(y), y = z or gamma xhat + beta
template <int V>
__global__ void ct_act_kernel(CtAct a, float* out) {
  const int HW = a.H * a.W;
  const size_t groups = (size_t)a.B * a.C * HW / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * V;
    const CtAffine f = ct_affine(a, (int)((e / HW) % a.C));
    float v[V];
    ct_load<V>(a.z + e, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = ct_relu(f.y(v[j]));
    ct_store<V>(out + e, v);
  }
}
void launch_ct_act(const CtAct& a, float* out, hipStream_t s) {
  const size_t total = (size_t)a.B * a.C * a.H * a.W;
  if ((a.H * a.W) % 4 == 0 && ct_aligned({a.z, out}))
    hipLaunchKernelGGL(ct_act_kernel<4>, ct_grid(total / 4), dim3(256), 0, s, a, out);
  else hipLaunchKernelGGL(ct_act_kernel<1>, ct_grid(total), dim3(256), 0, s, a, out);
}
// out[b][c][yo][xo] = max over the 2x2 window of relu(y), floor division of odd rasters; choice = the window element
// taken (row-major 0..3; ties: the first).  A thread owns V consecutive outputs of one row: 2 V inputs of two rows.
template <int V>
__global__ void ct_act_pool_kernel(CtAct a, float* out, unsigned char* choice) {
  const int Ho = a.H / 2, Wo = a.W / 2;
  const size_t groups = (size_t)a.B * a.C * Ho * Wo / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = i * V;
    const int xo = (int)(o % Wo);
    size_t r = o / Wo;
    const int yo = (int)(r % Ho);
    r /= Ho;  // b * C + c
    const CtAffine f = ct_affine(a, (int)(r % a.C));
    const float* zp = a.z + (r * a.H + 2 * yo) * a.W + 2 * xo;
    float top[2 * V], bot[2 * V];
    if constexpr (V == 4) {
      float t[4];
      ct_load<4>(zp, t), top[0] = t[0], top[1] = t[1], top[2] = t[2], top[3] = t[3];
      ct_load<4>(zp + 4, t), top[4] = t[0], top[5] = t[1], top[6] = t[2], top[7] = t[3];
      ct_load<4>(zp + a.W, t), bot[0] = t[0], bot[1] = t[1], bot[2] = t[2], bot[3] = t[3];
      ct_load<4>(zp + a.W + 4, t), bot[4] = t[0], bot[5] = t[1], bot[6] = t[2], bot[7] = t[3];
    } else {
      top[0] = zp[0], top[1] = zp[1], bot[0] = zp[a.W], bot[1] = zp[a.W + 1];
    }
    float best[V];
    unsigned ks = 0u;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float w[4] = {ct_relu(f.y(top[2 * j])), ct_relu(f.y(top[2 * j + 1])), ct_relu(f.y(bot[2 * j])),
                          ct_relu(f.y(bot[2 * j + 1]))};
      unsigned k = 0u;
      float m = w[0];
#pragma unroll
      for (unsigned q = 1; q < 4; ++q)
        if (w[q] > m) m = w[q], k = q;
      best[j] = m;
      ks |= k << (8 * j);
    }
    ct_store<V>(out + o, best);
    if constexpr (V == 4) *reinterpret_cast<unsigned*>(choice + o) = ks;
    else choice[o] = (unsigned char)ks;
  }
}
void launch_ct_act_pool(const CtAct& a, float* out, unsigned char* choice, hipStream_t s) {
  const size_t total = (size_t)a.B * a.C * (a.H / 2) * (a.W / 2);
  if (a.W % 8 == 0 && ct_aligned({a.z, out, choice}))
    hipLaunchKernelGGL(ct_act_pool_kernel<4>, ct_grid(total / 4), dim3(256), 0, s, a, out, choice);
  else hipLaunchKernelGGL(ct_act_pool_kernel<1>, ct_grid(total), dim3(256), 0, s, a, out, choice);
}

// ------------------------------------------------------------------ backward of ReLU (+ max-pool)
// full[b][c][y][x] = g[b][c][y / 2][x / 2] where (y, x) is the chosen element and the pooled activation passed the
// ReLU, else 0 (the last row / column of an odd raster lies in no window): the gradient of y on the conv's raster.
// V = 4 (even H, W % 8 == 0): a thread owns 4 consecutive pooled outputs and writes their two rows of 8.
template <int V>
__global__ void ct_unpool_gate_kernel(const float* g, const unsigned char* choice, const float* act, float* full, int BC,
                                      int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  if constexpr (V == 4) {
    const size_t groups = (size_t)BC * Ho * Wo / 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
      const size_t o = i * 4;
      const int xo = (int)(o % Wo);
      const size_t r = o / Wo;  // bc * Ho + yo
      float gv[4], av[4];
      ct_load<4>(g + o, gv), ct_load<4>(act + o, av);
      const unsigned ks = *reinterpret_cast<const unsigned*>(choice + o);
      float row[2][8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned k = (ks >> (8 * j)) & 0xffu;
        const float v = av[j] > 0.f ? gv[j] : 0.f;
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
        if (choice[o] == (unsigned char)((y & 1) * 2 + (x & 1)) && act[o] > 0.f) v = g[o];
      }
      full[i] = v;
    }
  }
}
void launch_ct_unpool_gate(const float* g, const unsigned char* choice, const float* act, float* full, int BC, int H,
                           int W, hipStream_t s) {
  if (H % 2 == 0 && W % 8 == 0 && ct_aligned({g, choice, act, full}))
    hipLaunchKernelGGL(ct_unpool_gate_kernel<4>, ct_grid((size_t)BC * (H / 2) * (W / 2) / 4), dim3(256), 0, s, g, choice,
                       act, full, BC, H, W);
  else
    hipLaunchKernelGGL(ct_unpool_gate_kernel<1>, ct_grid((size_t)BC * H * W), dim3(256), 0, s, g, choice, act, full, BC,
                       H, W);
}
// in place: g <- g where act > 0, else 0
template <int V>
__global__ void ct_gate_kernel(float* g, const float* act, size_t n) {
  const size_t groups = n / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    float gv[V], av[V];
    ct_load<V>(g + i * V, gv), ct_load<V>(act + i * V, av);
#pragma unroll
    for (int j = 0; j < V; ++j) gv[j] = av[j] > 0.f ? gv[j] : 0.f;
    ct_store<V>(g + i * V, gv);
  }
}
void launch_ct_gate(float* g, const float* act, size_t n, hipStream_t s) {
  if (n % 4 == 0 && ct_aligned({g, act})) hipLaunchKernelGGL(ct_gate_kernel<4>, ct_grid(n / 4), dim3(256), 0, s, g, act, n);
  else hipLaunchKernelGGL(ct_gate_kernel<1>, ct_grid(n), dim3(256), 0, s, g, act, n);
}
// out[i] = 1.0 where act[i] > 0, else 0.0 (rgfm_clf_gate)
__global__ void ct_gate_out_kernel(const float* act, size_t n, float* out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = act[i] > 0.f ? 1.f : 0.f;
}
void launch_ct_gate_out(const float* act, size_t n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ct_gate_out_kernel, ct_grid(n), dim3(256), 0, s, act, n, out);
}

// ------------------------------------------------------------------ BatchNorm + ReLU backward
// With dy = the gradient of y = gamma xhat + beta (dout where `act` = relu(y) > 0; `act` null: dout is dy already, the
// pool's routing has applied the gate):  dgamma = sum dy xhat,  dbeta = sum dy  over (b, pixel), and
//   training:  dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat))      eval:  dz = gamma rstd dy
// pass 1: part[c][slice] = (sum dy, sum dy xhat) over a batch slice
template <int V>
__global__ __launch_bounds__(256) void ct_bn_bwd_part_kernel(CtAct a, const float* dout, const float* act, int bper,
                                                             float* part) {
  __shared__ float red[256];
  const int c = blockIdx.x, b0 = blockIdx.y * bper, HW = a.H * a.W;
  const int n = (min(a.B, b0 + bper) - b0) * HW / V;
  const CtAffine f = ct_affine(a, c);
  float sb = 0.f, sg = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int e = i * V;
    const size_t o = ((size_t)(b0 + e / HW) * a.C + c) * HW + e % HW;
    float zv[V], dv[V], av[V];
    ct_load<V>(a.z + o, zv), ct_load<V>(dout + o, dv);
    if (act) ct_load<V>(act + o, av);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float dy = !act || av[j] > 0.f ? dv[j] : 0.f;
      sb += dy, sg += dy * f.xhat(zv[j]);
    }
  }
  sb = ug_block_sum(sb, red);
  sg = ug_block_sum(sg, red);
  if (threadIdx.x == 0) {
    float* o = part + ((size_t)c * gridDim.y + blockIdx.y) * 2;
    o[0] = sb, o[1] = sg;
  }
}
// (between the passes: launch_rt_bn_bwd_finalize of ratio_train.hip adds the slices in order in fp64 -- dgamma, dbeta and
// m12[c] = (mean(dy), mean(dy xhat)), zeros in eval mode: the forward left its mode in a word of the saved state)
// pass 2, in place: dout <- dz
template <int V>
__global__ void ct_bn_bwd_apply_kernel(CtAct a, float* dout, const float* act, const float* m12) {
  const int HW = a.H * a.W;
  const size_t groups = (size_t)a.B * a.C * HW / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * V;
    const int c = (int)((e / HW) % a.C);
    const CtAffine f = ct_affine(a, c);
    const float m1 = m12[2 * c], m2 = m12[2 * c + 1];
    float zv[V], dv[V], av[V];
    ct_load<V>(a.z + e, zv), ct_load<V>(dout + e, dv);
    if (act) ct_load<V>(act + e, av);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float dy = !act || av[j] > 0.f ? dv[j] : 0.f;
      dv[j] = f.g * f.rstd * (dy - m1 - f.xhat(zv[j]) * m2);
    }
    ct_store<V>(dout + e, dv);
  }
}
void launch_ct_bn_bwd(const CtAct& a, float* dout, const float* act, const unsigned* training, float* part, float* m12,
                      float* dgamma, float* dbeta, hipStream_t s) {
  const int bper = (a.B + RT_BN_SLICES - 1) / RT_BN_SLICES, slices = (a.B + bper - 1) / bper;
  const size_t total = (size_t)a.B * a.C * a.H * a.W;
  const bool vec = (a.H * a.W) % 4 == 0 && ct_aligned({a.z, dout, act});
  if (vec) hipLaunchKernelGGL(ct_bn_bwd_part_kernel<4>, dim3(a.C, slices), dim3(256), 0, s, a, dout, act, bper, part);
  else hipLaunchKernelGGL(ct_bn_bwd_part_kernel<1>, dim3(a.C, slices), dim3(256), 0, s, a, dout, act, bper, part);
  launch_rt_bn_bwd_finalize(part, a.C, slices, 1.0f / (float)((size_t)a.B * a.H * a.W), training, dgamma, dbeta, m12, s);
  if (vec) hipLaunchKernelGGL(ct_bn_bwd_apply_kernel<4>, ct_grid(total / 4), dim3(256), 0, s, a, dout, act, m12);
  else hipLaunchKernelGGL(ct_bn_bwd_apply_kernel<1>, ct_grid(total), dim3(256), 0, s, a, dout, act, m12);
}

// ------------------------------------------------------------------ ReLU + dropout behind fc1
// out = drop(relu(u)): Dropout layer 0, the keep decision of element i by ug_keep, kept values scaled by 1 / (1 - p)
template <int V>
__global__ void ct_relu_drop_kernel(const float* u, size_t n, const unsigned* hdr, float* out) {
  float p;
  uint64_t seed;
  ug_drop_params(hdr, p, seed);
  const float keep_scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  const size_t groups = n / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    float v[V];
    ct_load<V>(u + i * V, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      v[j] = ct_relu(v[j]);
      if (p > 0.f) v[j] = ug_keep(seed, 0, (uint32_t)(i * V + j), p) ? v[j] * keep_scale : 0.f;
    }
    ct_store<V>(out + i * V, v);
  }
}
void launch_ct_relu_drop(const float* u, size_t n, const unsigned* hdr, float* out, hipStream_t s) {
  if (n % 4 == 0 && ct_aligned({u, out})) hipLaunchKernelGGL(ct_relu_drop_kernel<4>, ct_grid(n / 4), dim3(256), 0, s, u, n, hdr, out);
  else hipLaunchKernelGGL(ct_relu_drop_kernel<1>, ct_grid(n), dim3(256), 0, s, u, n, hdr, out);
}
// in place: g <- drop(g) where u > 0, else 0
template <int V>
__global__ void ct_relu_drop_bwd_kernel(const float* u, float* g, size_t n, const unsigned* hdr) {
  float p;
  uint64_t seed;
  ug_drop_params(hdr, p, seed);
  const float keep_scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  const size_t groups = n / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    float uv[V], gv[V];
    ct_load<V>(u + i * V, uv), ct_load<V>(g + i * V, gv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (p > 0.f) gv[j] = ug_keep(seed, 0, (uint32_t)(i * V + j), p) ? gv[j] * keep_scale : 0.f;
      gv[j] = uv[j] > 0.f ? gv[j] : 0.f;
    }
    ct_store<V>(g + i * V, gv);
  }
}
void launch_ct_relu_drop_bwd(const float* u, float* g, size_t n, const unsigned* hdr, hipStream_t s) {
  if (n % 4 == 0 && ct_aligned({u, g})) hipLaunchKernelGGL(ct_relu_drop_bwd_kernel<4>, ct_grid(n / 4), dim3(256), 0, s, u, g, n, hdr);
  else hipLaunchKernelGGL(ct_relu_drop_bwd_kernel<1>, ct_grid(n), dim3(256), 0, s, u, g, n, hdr);
}

// ------------------------------------------------------------------ softmax cross-entropy
// One lane per row of logits[n][classes], classes <= CT_MAX_CLASSES.  The row's maximum m (the first index on a tie is
// the predicted class) is subtracted before the exponential; the exponentials, their ascending sum and the logarithm
// are taken in fp64, so that loss[r] = log(sum_j exp(x_j - m)) + (m - x_label) carries no fp32 rounding of a sum of
// large logits.  dlogits = (softmax - onehot) scale.  No reduction across rows: the mean is the caller's `scale` and
// its own fixed-order sum of loss[].
__global__ void ct_xent_kernel(const float* logits, const int* labels, int n, int classes, float scale, double* loss,
                               float* dlogits, int* pred) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float* x = logits + (size_t)r * classes;
  float v[CT_MAX_CLASSES];
#pragma unroll
  for (int j = 0; j < CT_MAX_CLASSES; ++j) v[j] = j < classes ? x[j] : -INFINITY;
  float m = v[0];
  int k = 0;
#pragma unroll
  for (int j = 1; j < CT_MAX_CLASSES; ++j)
    if (v[j] > m) m = v[j], k = j;
  const int label = labels[r];
  double sum = 0.0, xl = 0.0;
#pragma unroll
  for (int j = 0; j < CT_MAX_CLASSES; ++j) {
    if (j < classes) sum += exp((double)v[j] - (double)m);
    if (j == label) xl = (double)v[j];
  }
  loss[r] = log(sum) + ((double)m - xl);
  if (pred) pred[r] = k;
  if (dlogits) {
    const double inv = 1.0 / sum;
#pragma unroll
    for (int j = 0; j < CT_MAX_CLASSES; ++j)
      if (j < classes)
        dlogits[(size_t)r * classes + j] = (float)(exp((double)v[j] - (double)m) * inv - (j == label ? 1.0 : 0.0)) * scale;
  }
}
void launch_ct_xent(const float* logits, const int* labels, int n, int classes, float scale, double* loss,
                    float* dlogits, int* pred, hipStream_t s) {
  hipLaunchKernelGGL(ct_xent_kernel, dim3((n + 63) / 64), dim3(64), 0, s, logits, labels, n, classes, scale, loss,
                     dlogits, pred);
}

}  // namespace rgfm
