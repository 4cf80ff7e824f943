// clf_train.hip -- training pass of the evaluation classifiers (reference src/models/classifier.py:9-52,
// src/models/svhn_classifier.py:11-116): what the other training kernels do not cover.
//
//   The ReLU gate of a conv block that has neither a max-pool nor a BatchNorm behind it (ct_gate_kernel) and the gate
//     as a test hook (ct_gate_out_kernel).  The gate is `value > 0`, as in torch: a value of exactly 0 gets no gradient.
//   ReLU + dropout behind fc1 and its backward (the counter hash ug_keep, Dropout layer 0).
//   Softmax cross-entropy with its gradient and the predicted class: ct_xent_kernel, one lane per row.
//
// All tensors are NCHW fp32; the elementwise kernels move V = 4 floats per thread where size and alignment allow
// (train_device.h).  The conv blocks' BatchNorm, ReLU and max-pool with their backward run on block_train.hip, the
// convs and the Linear layers on the kernels of unet_grad.hip and fmnet_grad.hip.
#include "train_device.h"

namespace rgfm {

__device__ __forceinline__ float ct_relu(float v) { return v > 0.f ? v : 0.f; }

// ------------------------------------------------------------------ the ReLU gate
// in place: g <- g where act > 0, else 0
template <int V>
__global__ void ct_gate_kernel(float* g, const float* act, size_t n) {
  const size_t groups = n / V;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    float gv[V], av[V];
    vec_load<V>(g + i * V, gv), vec_load<V>(act + i * V, av);
#pragma unroll
    for (int j = 0; j < V; ++j) gv[j] = av[j] > 0.f ? gv[j] : 0.f;
    vec_store<V>(g + i * V, gv);
  }
}
void launch_ct_gate(float* g, const float* act, size_t n, hipStream_t s) {
  if (n % 4 == 0 && vec_aligned({g, act})) hipLaunchKernelGGL(ct_gate_kernel<4>, vec_grid(n / 4), dim3(256), 0, s, g, act, n);
  else hipLaunchKernelGGL(ct_gate_kernel<1>, vec_grid(n), dim3(256), 0, s, g, act, n);
}
// out[i] = 1.0 where act[i] > 0, else 0.0 (rgfm_clf_gate)
__global__ void ct_gate_out_kernel(const float* act, size_t n, float* out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = act[i] > 0.f ? 1.f : 0.f;
}
void launch_ct_gate_out(const float* act, size_t n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ct_gate_out_kernel, vec_grid(n), dim3(256), 0, s, act, n, out);
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
    vec_load<V>(u + i * V, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      v[j] = ct_relu(v[j]);
      if (p > 0.f) v[j] = ug_keep(seed, 0, (uint32_t)(i * V + j), p) ? v[j] * keep_scale : 0.f;
    }
    vec_store<V>(out + i * V, v);
  }
}
void launch_ct_relu_drop(const float* u, size_t n, const unsigned* hdr, float* out, hipStream_t s) {
  if (n % 4 == 0 && vec_aligned({u, out})) hipLaunchKernelGGL(ct_relu_drop_kernel<4>, vec_grid(n / 4), dim3(256), 0, s, u, n, hdr, out);
  else hipLaunchKernelGGL(ct_relu_drop_kernel<1>, vec_grid(n), dim3(256), 0, s, u, n, hdr, out);
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
    vec_load<V>(u + i * V, uv), vec_load<V>(g + i * V, gv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (p > 0.f) gv[j] = ug_keep(seed, 0, (uint32_t)(i * V + j), p) ? gv[j] * keep_scale : 0.f;
      gv[j] = uv[j] > 0.f ? gv[j] : 0.f;
    }
    vec_store<V>(g + i * V, gv);
  }
}
void launch_ct_relu_drop_bwd(const float* u, float* g, size_t n, const unsigned* hdr, hipStream_t s) {
  if (n % 4 == 0 && vec_aligned({u, g})) hipLaunchKernelGGL(ct_relu_drop_bwd_kernel<4>, vec_grid(n / 4), dim3(256), 0, s, u, g, n, hdr);
  else hipLaunchKernelGGL(ct_relu_drop_bwd_kernel<1>, vec_grid(n), dim3(256), 0, s, u, g, n, hdr);
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
