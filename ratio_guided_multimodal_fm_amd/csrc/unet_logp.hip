// unet_logp.hip -- the small kernels of the likelihood path (api_train.cpp: rgfm_unet_divergence, rgfm_unet_log_prob;
// DESIGN.md section 13): the per-row dot product of the Hutchinson estimate, the state update of the reverse-time ODE
// loop, its time table and the Gaussian log-density that finishes log p.  The network itself -- the exact-fp32 forward
// and the data-only reverse walk -- is unet_grad.hip's.
//
// Every reduction is a fixed-order per-thread loop followed by a fixed-order LDS tree: no float atomics, two calls on
// the same inputs give the same bits, and a row's result depends on that row only.
#include "rgfm_device.h"
#include "train_device.h"

namespace rgfm {

// acc[b] = (accumulate ? acc[b] : 0) + scale <a[b, :], g[b, :]>; one workgroup per row, any d >= 1
__global__ __launch_bounds__(256) void ul_rowdot_kernel(const float* a, const float* g, int d, float scale,
                                                        int accumulate, float* acc) {
  __shared__ float red[256];
  const size_t base = (size_t)blockIdx.x * d;
  float v = 0.f;
  for (int i = threadIdx.x; i < d; i += 256) v += a[base + i] * g[base + i];
  v = ug_block_sum(v, red);
  if (threadIdx.x == 0) acc[blockIdx.x] = (accumulate ? acc[blockIdx.x] : 0.f) + scale * v;
}
void launch_ul_rowdot(const float* a, const float* g, int B, int d, float scale, int accumulate, float* acc,
                      hipStream_t s) {
  hipLaunchKernelGGL(ul_rowdot_kernel, dim3(B), dim3(256), 0, s, a, g, d, scale, accumulate, acc);
}

// dst = src - c k  (two roundings, as the Euler epilogues of the samplers); dst may be src
__global__ void ul_step_kernel(const float* src, const float* k, float c, size_t n, float* dst) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = __fsub_rn(src[i], __fmul_rn(c, k[i]));
}
void launch_ul_step(const float* src, const float* k, float c, size_t n, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(ul_step_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, src, k,
                     c, n, dst);
}

// The stage times of the reverse loop over steps i = N - 1 ... 0, in the order the loop takes them, scalars in double and
// rounded once: Euler row j = t_hi of step N - 1 - j; midpoint rows 2j, 2j + 1 = (t_hi, t_hi - dt / 2).
__global__ void ul_times_kernel(float* tt, int num_steps, int midpoint) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= num_steps) return;
  const double dt = 1.0 / (double)num_steps;
  const double t_hi = (double)(num_steps - j) * dt;
  if (midpoint) tt[2 * j] = (float)t_hi, tt[2 * j + 1] = (float)(t_hi - 0.5 * dt);
  else tt[j] = (float)t_hi;
}
void launch_ul_times(float* tt, int num_steps, int midpoint, hipStream_t s) {
  hipLaunchKernelGGL(ul_times_kernel, dim3((num_steps + 255) / 256), dim3(256), 0, s, tt, num_steps, midpoint);
}

// logp[b] = -|z_b|^2 / 2 - (d / 2) log(2 pi) - A[b]; one workgroup per row.  |z|^2 and the three-term sum are taken
// in double (d / 2 log(2 pi) is 2823 at d = 3072, where an fp32 ulp is 2.4e-4) and rounded once.
__global__ __launch_bounds__(256) void ul_gauss_logp_kernel(const float* z, const float* A, int d, float* logp) {
  __shared__ double red[256];
  const size_t base = (size_t)blockIdx.x * d;
  const int t = threadIdx.x;
  double v = 0.0;
  for (int i = t; i < d; i += 256) v += (double)z[base + i] * (double)z[base + i];
  red[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) logp[blockIdx.x] = (float)(-0.5 * red[0] - 0.5 * (double)d * 1.8378770664093453 - (double)A[blockIdx.x]);
}
void launch_ul_gauss_logp(const float* z, const float* A, int B, int d, float* logp, hipStream_t s) {
  hipLaunchKernelGGL(ul_gauss_logp_kernel, dim3(B), dim3(256), 0, s, z, A, d, logp);
}

}  // namespace rgfm
