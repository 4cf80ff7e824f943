// train_device.h -- helpers shared by the training kernels (unet_grad.hip, fmnet_grad.hip, block_train.hip,
// ratio_train.hip, clf_train.hip): SiLU, the MFMA GEMM core, the dropout hash, the block sum, and the V = 1 / 4 access
// of the memory-bound elementwise kernels with the host-side checks their launchers make.
#pragma once
#include <cstdint>
#include <initializer_list>

#include "rgfm_device.h"

namespace rgfm {

__device__ __forceinline__ float ug_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float ug_silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float ug_dsilu(float v) {
  const float s = ug_sigmoid(v);
  return s * (1.0f + v * (1.0f - s));
}

// The GEMM core of every training kernel: one staged K-chunk (KC = 16) of a 64 (M) x 64 (N) block tile.  Every thread
// hands over 4 consecutive k -- quarter qa / qb -- of ONE row of A and ONE row (column) of B; the four waves then take
// eight v_mfma_f32_32x32x2_f32 steps on their 32 x 32 accumulator (same LDS layout and k permutation as
// linear_mfma_kernel).  sA / sB: 64 * LDP floats each.
__device__ __forceinline__ void ug_mfma_chunk(float* sA, float* sB, int rowa, int qa, const float (&va)[4], int rowb,
                                              int qb, const float (&vb)[4], int wm, int wn, int l31, int h,
                                              f32x16& acc) {
  __syncthreads();
  *reinterpret_cast<f32x4*>(sA + rowa * LDP + qa * 4) = f32x4{va[0], va[1], va[2], va[3]};
  *reinterpret_cast<f32x4*>(sB + rowb * LDP + qb * 4) = f32x4{vb[0], vb[1], vb[2], vb[3]};
  __syncthreads();
  const float* ap = sA + (wm * 32 + l31) * LDP + h * 8;
  const float* bp = sB + (wn * 32 + l31) * LDP + h * 8;
  const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc, 0, 0, 0);
}
// row of the accumulator's element r (C/D layout of the 32x32 MFMA: column = lane & 31, h = lane >> 5)
__device__ __forceinline__ int ug_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

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

// V consecutive floats per thread: one 16-byte access at V = 4
template <int V>
__device__ __forceinline__ void vec_load(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void vec_store(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}
static bool vec_aligned(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  return true;
}
// grid-stride launch of 256-thread workgroups over `groups` work items, capped at 4096 workgroups
static dim3 vec_grid(size_t groups) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((groups + 255) / 256, 4096))); }

}  // namespace rgfm
