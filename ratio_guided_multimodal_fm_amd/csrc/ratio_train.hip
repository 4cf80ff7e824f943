// ratio_train.hip -- training pass of the ratio estimators (reference src/models/ratio_flexible.py:185-364,
// src/models/ratio_estimator.py:34-135): what the other training kernels do not cover.
//
//   global average pool and its backward; LayerNorm + SiLU + dropout of the score MLP and its backward.
//
// All tensors are fp32.  No float atomics: every reduction is a fixed-order loop or an LDS tree, so two calls on the
// same inputs agree bitwise.  The encoders' norm, SiLU and max-pool with their backward run on block_train.hip, the
// convs and the Linear layers on the kernels of unet_grad.hip.
#include "train_device.h"

namespace rgfm {

// ------------------------------------------------------------------ global average pool
// out[r] = mean over p (ascending) of in[r][p]
__global__ void rt_avgpool_kernel(const float* in, int rows, int n, float* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float v = 0.f;
  for (int p = 0; p < n; ++p) v += in[(size_t)r * n + p];
  out[r] = v / (float)n;
}
void launch_rt_avgpool(const float* in, int rows, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(rt_avgpool_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, in, rows, n, out);
}
// din[r][p] = g[r] / n
__global__ void rt_avgpool_bwd_kernel(const float* g, size_t total, int n, float* din) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    din[i] = g[i / n] / (float)n;
}
void launch_rt_avgpool_bwd(const float* g, int rows, int n, float* din, hipStream_t s) {
  const size_t total = (size_t)rows * n;
  hipLaunchKernelGGL(rt_avgpool_bwd_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s,
                     g, total, n, din);
}

// ------------------------------------------------------------------ LayerNorm + SiLU + dropout of the score MLP
// One workgroup per row.  Forward: mr[r] = (mean, rstd) (biased variance, eps 1e-5), out = drop(silu(gamma xhat + beta)),
// dropout layer `block` (< 0: none) with the keep decisions of element r * width + j.
__global__ __launch_bounds__(256) void rt_ln_act_kernel(const float* u, const float* gamma, const float* beta, int width,
                                                        const unsigned* hdr, int block, float* mr, float* out) {
  __shared__ float red[256];
  const int r = blockIdx.x;
  const float* x = u + (size_t)r * width;
  float v = 0.f;
  for (int j = threadIdx.x; j < width; j += 256) v += x[j];
  const float mean = ug_block_sum(v, red) / (float)width;
  v = 0.f;
  for (int j = threadIdx.x; j < width; j += 256) v += (x[j] - mean) * (x[j] - mean);
  const float rstd = 1.0f / sqrtf(ug_block_sum(v, red) / (float)width + 1e-5f);
  if (threadIdx.x == 0) mr[2 * r] = mean, mr[2 * r + 1] = rstd;
  float drop_p;
  uint64_t seed;
  ug_drop_params(block >= 0 ? hdr : nullptr, drop_p, seed);
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  for (int j = threadIdx.x; j < width; j += 256) {
    float a = ug_silu(gamma[j] * ((x[j] - mean) * rstd) + beta[j]);
    if (drop_p > 0.f) a = ug_keep(seed, block, (uint32_t)(r * width + j), drop_p) ? a * keep_scale : 0.f;
    out[(size_t)r * width + j] = a;
  }
}
void launch_rt_ln_act(const float* u, const float* gamma, const float* beta, int rows, int width, const unsigned* hdr,
                      int block, float* mr, float* out, hipStream_t s) {
  hipLaunchKernelGGL(rt_ln_act_kernel, dim3(rows), dim3(256), 0, s, u, gamma, beta, width, hdr, block, mr, out);
}
// Backward: dy = drop(g) silu'(gamma xhat + beta); du = rstd (dy gamma - mean_j(dy gamma) - xhat mean_j(dy gamma xhat));
// pg / pb [rows][width] = dy xhat / dy (dgamma / dbeta are their column sums)
__global__ __launch_bounds__(256) void rt_ln_act_bwd_kernel(const float* u, const float* g, const float* gamma,
                                                            const float* beta, int width, const unsigned* hdr, int block,
                                                            const float* mr, float* du, float* pg, float* pb) {
  __shared__ float red[256];
  const int r = blockIdx.x;
  const float mean = mr[2 * r], rstd = mr[2 * r + 1];
  float drop_p;
  uint64_t seed;
  ug_drop_params(block >= 0 ? hdr : nullptr, drop_p, seed);
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  float s1 = 0.f, s2 = 0.f;
  for (int j = threadIdx.x; j < width; j += 256) {
    const size_t i = (size_t)r * width + j;
    const float xh = (u[i] - mean) * rstd;
    float go = g[i];
    if (drop_p > 0.f) go = ug_keep(seed, block, (uint32_t)i, drop_p) ? go * keep_scale : 0.f;
    const float dy = go * ug_dsilu(gamma[j] * xh + beta[j]);
    pg[i] = dy * xh, pb[i] = dy;
    s1 += dy * gamma[j], s2 += dy * gamma[j] * xh;
  }
  const float m1 = ug_block_sum(s1, red) / (float)width;
  const float m2 = ug_block_sum(s2, red) / (float)width;
  for (int j = threadIdx.x; j < width; j += 256) {
    const size_t i = (size_t)r * width + j;
    du[i] = rstd * (pb[i] * gamma[j] - m1 - (u[i] - mean) * rstd * m2);
  }
}
void launch_rt_ln_act_bwd(const float* u, const float* g, const float* gamma, const float* beta, int rows, int width,
                          const unsigned* hdr, int block, const float* mr, float* du, float* pg, float* pb,
                          hipStream_t s) {
  hipLaunchKernelGGL(rt_ln_act_bwd_kernel, dim3(rows), dim3(256), 0, s, u, g, gamma, beta, width, hdr, block, mr, du, pg,
                     pb);
}

}  // namespace rgfm
