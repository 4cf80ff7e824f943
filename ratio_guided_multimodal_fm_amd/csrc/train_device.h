// train_device.h -- device helpers shared by the training kernels (unet_grad.hip, ratio_train.hip).
#pragma once
#include <cstdint>

#include "rgfm_device.h"

namespace rgfm {

__device__ __forceinline__ float ug_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float ug_silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float ug_dsilu(float v) {
  const float s = ug_sigmoid(v);
  return s * (1.0f + v * (1.0f - s));
}

// Dropout keep decision of element `idx` of ResBlock `block` (rgfm.h: rgfm_unet_dropout_mask).
__host__ __device__ inline bool ug_keep(uint64_t seed, int block, uint32_t idx, float p) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((((uint64_t)(uint32_t)block) << 32 | idx) + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u = (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f);
  return u >= p;
}

// 256-thread LDS tree (fixed order)
__device__ __forceinline__ float ug_block_sum(float v, float* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// the saved state's dropout header {p_drop bits, seed lo, seed hi} (launch_ug_header)
__device__ __forceinline__ void ug_drop_params(const unsigned* hdr, float& p, uint64_t& seed) {
  p = 0.f, seed = 0;
  if (hdr) p = __uint_as_float(hdr[0]), seed = (uint64_t)hdr[1] | ((uint64_t)hdr[2] << 32);
}

}  // namespace rgfm
