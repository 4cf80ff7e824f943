// ratio_train.hip -- training pass of the ratio estimators (reference src/models/ratio_flexible.py:185-364,
// src/models/ratio_estimator.py:34-135): what the U-Net training kernels (unet_grad.hip) do not cover.
//
//   BatchNorm in training mode: per-channel (count, mean, M2) partials over B*H*W, one per (channel, batch slice),
//     Chan-combined in fp64 in slice order (rt_bn_part_kernel / rt_bn_finalize_kernel); its backward as a two-pass pair
//     (rt_bn_bwd_part_kernel -> rt_bn_bwd_finalize_kernel -> rt_bn_bwd_apply_kernel).
//   norm + SiLU (+ 2x2 max-pool with the chosen window element recorded, one byte per output): rt_norm_act_kernel,
//     rt_norm_act_pool_kernel; the pool's gradient routing: rt_unpool_kernel.
//   global average pool and its backward; LayerNorm + SiLU + dropout of the score MLP and its backward.
//
// All tensors are NCHW fp32.  No float atomics: every reduction is a fixed-order loop, an LDS tree or an ordered
// combine of per-workgroup partials, so two calls on the same inputs agree bitwise.  The convs and the Linear layers
// run on the kernels of unet_grad.hip.
#include "train_device.h"

namespace rgfm {

// (mean, rstd) of element (b, c): BatchNorm keeps one pair per channel, GroupNorm one per (sample, group)
__device__ __forceinline__ const float* rt_mr(const float* mr, int groups, int C, int b, int c) {
  return mr + 2 * (groups ? b * groups + c / (C / groups) : c);
}

// ------------------------------------------------------------------ BatchNorm statistics
// part[c][slice] = (count, mean, M2) of channel c over the samples [slice * bper, (slice + 1) * bper); two passes
__global__ __launch_bounds__(256) void rt_bn_part_kernel(const float* z, int B, int C, int HW, int bper, float* part) {
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
__global__ void rt_bn_finalize_kernel(const float* part, int C, int slices, float* mr, float* stats) {
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
void launch_rt_bn_stats(const float* z, int B, int C, int HW, float* part, float* mr, float* stats, hipStream_t s) {
  const int bper = (B + RT_BN_SLICES - 1) / RT_BN_SLICES, slices = (B + bper - 1) / bper;
  hipLaunchKernelGGL(rt_bn_part_kernel, dim3(C, slices), dim3(256), 0, s, z, B, C, HW, bper, part);
  hipLaunchKernelGGL(rt_bn_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, s, part, C, slices, mr, stats);
}
// eval mode: mr[c] = (running_mean, 1 / sqrt(running_var + eps))
__global__ void rt_bn_running_kernel(const float* rm, const float* rv, int C, float* mr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) mr[2 * c] = rm[c], mr[2 * c + 1] = 1.0f / sqrtf(rv[c] + 1e-5f);
}
void launch_rt_bn_running(const float* rm, const float* rv, int C, float* mr, hipStream_t s) {
  hipLaunchKernelGGL(rt_bn_running_kernel, dim3((C + 63) / 64), dim3(64), 0, s, rm, rv, C, mr);
}

// ------------------------------------------------------------------ norm + SiLU (+ max-pool)
__device__ __forceinline__ float rt_act(float v, const float* m, float gamma, float beta) {
  return ug_silu(gamma * ((v - m[0]) * m[1]) + beta);
}
// out = silu(gamma xhat + beta)
__global__ void rt_norm_act_kernel(RtNorm a, float* out) {
  const size_t total = (size_t)a.B * a.C * a.H * a.W;
  const int HW = a.H * a.W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / HW;
    const int c = r % a.C, b = r / a.C;
    out[i] = rt_act(a.z[i], rt_mr(a.mr, a.groups, a.C, b, c), a.gamma[c], a.beta[c]);
  }
}
void launch_rt_norm_act(const RtNorm& a, float* out, hipStream_t s) {
  const size_t total = (size_t)a.B * a.C * a.H * a.W;
  hipLaunchKernelGGL(rt_norm_act_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, a,
                     out);
}
// out[b][c][yo][xo] = max over the 2x2 window of silu(gamma xhat + beta), floor division of odd rasters;
// choice = the window element taken (row-major 0..3; ties: the first)
__global__ void rt_norm_act_pool_kernel(RtNorm a, float* out, unsigned char* choice) {
  const int Ho = a.H / 2, Wo = a.W / 2;
  const size_t total = (size_t)a.B * a.C * Ho * Wo;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xo = i % Wo;
    size_t r = i / Wo;
    const int yo = r % Ho;
    r /= Ho;
    const int c = r % a.C, b = r / a.C;
    const float* m = rt_mr(a.mr, a.groups, a.C, b, c);
    const float* zp = a.z + (r * a.H + 2 * yo) * a.W + 2 * xo;
    const float g = a.gamma[c], be = a.beta[c];
    const float v[4] = {rt_act(zp[0], m, g, be), rt_act(zp[1], m, g, be), rt_act(zp[a.W], m, g, be),
                        rt_act(zp[a.W + 1], m, g, be)};
    int k = 0;
    float best = v[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (v[j] > best) best = v[j], k = j;
    out[i] = best;
    choice[i] = (unsigned char)k;
  }
}
void launch_rt_norm_act_pool(const RtNorm& a, float* out, unsigned char* choice, hipStream_t s) {
  const size_t total = (size_t)a.B * a.C * (a.H / 2) * (a.W / 2);
  hipLaunchKernelGGL(rt_norm_act_pool_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0,
                     s, a, out, choice);
}
// gradient routing of the max-pool: full[b][c][y][x] = g[b][c][y / 2][x / 2] where (y, x) is the chosen element, else 0
// (the last row / column of an odd raster lies in no window)
__global__ void rt_unpool_kernel(const float* g, const unsigned char* choice, float* full, int BC, int H, int W) {
  const int Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)BC * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    const size_t r = i / W;
    const int y = r % H;
    const size_t bc = r / H;
    float v = 0.f;
    if (y < 2 * Ho && x < 2 * Wo) {
      const size_t o = (bc * Ho + (y >> 1)) * Wo + (x >> 1);
      if (choice[o] == (unsigned char)((y & 1) * 2 + (x & 1))) v = g[o];
    }
    full[i] = v;
  }
}
void launch_rt_unpool(const float* g, const unsigned char* choice, float* full, int BC, int H, int W, hipStream_t s) {
  const size_t total = (size_t)BC * H * W;
  hipLaunchKernelGGL(rt_unpool_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, g,
                     choice, full, BC, H, W);
}
// out[i] = choice[i] as a float (rgfm_ratio_pool_choice)
__global__ void rt_choice_kernel(const unsigned char* choice, size_t n, float* out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = (float)choice[i];
}
void launch_rt_choice(const unsigned char* choice, size_t n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(rt_choice_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, choice,
                     n, out);
}

// ------------------------------------------------------------------ BatchNorm + SiLU backward
// With dy = dout silu'(gamma xhat + beta):  dgamma = sum dy xhat,  dbeta = sum dy  over (b, pixel), and
//   training:  dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat))      eval:  dz = gamma rstd dy
// pass 1: part[c][slice] = (sum dy, sum dy xhat) over a batch slice
__global__ __launch_bounds__(256) void rt_bn_bwd_part_kernel(RtNorm a, const float* dout, int bper, float* part) {
  __shared__ float red[256];
  const int c = blockIdx.x, b0 = blockIdx.y * bper, HW = a.H * a.W;
  const int n = (min(a.B, b0 + bper) - b0) * HW;
  const float mean = a.mr[2 * c], rstd = a.mr[2 * c + 1], g = a.gamma[c], be = a.beta[c];
  float sb = 0.f, sg = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const size_t o = ((size_t)(b0 + i / HW) * a.C + c) * HW + i % HW;
    const float xh = (a.z[o] - mean) * rstd;
    const float dy = dout[o] * ug_dsilu(g * xh + be);
    sb += dy, sg += dy * xh;
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
__global__ void rt_bn_bwd_finalize_kernel(const float* part, int C, int slices, float inv_n, const unsigned* training_flag,
                                          float* dgamma, float* dbeta, float* m12) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const bool training = *training_flag != 0u;
  double sb = 0.0, sg = 0.0;
  for (int s = 0; s < slices; ++s) sb += part[((size_t)c * slices + s) * 2], sg += part[((size_t)c * slices + s) * 2 + 1];
  dgamma[c] = (float)sg, dbeta[c] = (float)sb;
  m12[2 * c] = training ? (float)sb * inv_n : 0.f, m12[2 * c + 1] = training ? (float)sg * inv_n : 0.f;
}
void launch_rt_bn_bwd_finalize(const float* part, int C, int slices, float inv_n, const unsigned* training, float* dgamma,
                               float* dbeta, float* m12, hipStream_t s) {
  hipLaunchKernelGGL(rt_bn_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, s, part, C, slices, inv_n, training,
                     dgamma, dbeta, m12);
}
// pass 2, in place: dout <- dz
__global__ void rt_bn_bwd_apply_kernel(RtNorm a, float* dout, const float* m12) {
  const size_t total = (size_t)a.B * a.C * a.H * a.W;
  const int HW = a.H * a.W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (i / HW) % a.C;
    const float rstd = a.mr[2 * c + 1], g = a.gamma[c];
    const float xh = (a.z[i] - a.mr[2 * c]) * rstd;
    const float dy = dout[i] * ug_dsilu(g * xh + a.beta[c]);
    dout[i] = g * rstd * (dy - m12[2 * c] - xh * m12[2 * c + 1]);
  }
}
void launch_rt_bn_bwd(const RtNorm& a, float* dout, const unsigned* training, float* part, float* m12, float* dgamma, float* dbeta,
                      hipStream_t s) {
  const int bper = (a.B + RT_BN_SLICES - 1) / RT_BN_SLICES, slices = (a.B + bper - 1) / bper;
  const size_t total = (size_t)a.B * a.C * a.H * a.W;
  hipLaunchKernelGGL(rt_bn_bwd_part_kernel, dim3(a.C, slices), dim3(256), 0, s, a, dout, bper, part);
  launch_rt_bn_bwd_finalize(part, a.C, slices, 1.0f / (float)((size_t)a.B * a.H * a.W), training, dgamma, dbeta, m12, s);
  hipLaunchKernelGGL(rt_bn_bwd_apply_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0,
                     s, a, dout, m12);
}

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
