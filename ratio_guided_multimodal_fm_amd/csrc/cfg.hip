// cfg.hip -- class conditioning and classifier-free guidance around the U-Net (include/rgfm.h, "Class conditioning").
//
// The label enters the net in one place, emb = time_embed(t) + E[y] (time_embed_labels_kernel, unet_kernels.hip, for the
// eval path's time tables).  What is left is data movement:
//   cfg_gather_kernel      a stage's per-row time table [B][total], row b copied from the call's [stages][K + 1][total]
//                          class table by its label: the convs read it through ConvArgs::temb_per_row
//   cfg_blend_kernel       state = base + (v_u + w (v_c - v_u)) dts, the update of a guided stage from the two raw
//                          velocities: 12 bytes read and 4 written per element, float4 wide, nothing reused
//   cfg_label_add_kernel   training: emb[b] += E[y_b], and the labels as used go into the saved state
//   cfg_label_grad_kernel  training: dE[c] = sum of the rows of d emb whose label is c, in ascending row order -- one
//                          workgroup per class and one thread per column, so two calls give the same bits, and a class
//                          without a row gets exact zeros
// A label is user data: every kernel reads `(unsigned)y > K ? K : y`, so no value of it addresses outside a table.
#include "rgfm_device.h"

namespace rgfm {

__device__ __forceinline__ int cfg_label(const int* labels, int b, int K) {
  if (!labels) return K;
  const int c = labels[b];
  return (unsigned)c > (unsigned)K ? K : c;
}

__global__ __launch_bounds__(256) void cfg_gather_kernel(const float* __restrict__ table, const int* __restrict__ labels, int K,
                                                         int stage, int total4, float* __restrict__ rows) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= total4) return;
  const size_t src = ((size_t)stage * (K + 1) + cfg_label(labels, b, K)) * total4 + j;
  reinterpret_cast<float4*>(rows)[(size_t)b * total4 + j] = reinterpret_cast<const float4*>(table)[src];
}

void launch_cfg_gather(const float* table, const int* labels, int K, int stage, int B, int total, float* rows, hipStream_t s) {
  const int total4 = total / 4;
  hipLaunchKernelGGL(cfg_gather_kernel, dim3((total4 + 255) / 256, B), dim3(256), 0, s, table, labels, K, stage, total4, rows);
}

__device__ __forceinline__ float cfg_blend(float base, float vc, float vu, float w, float dts) {
  return base + (vu + w * (vc - vu)) * dts;
}

template <bool VEC>
__global__ __launch_bounds__(256) void cfg_blend_kernel(const float* base, const float* __restrict__ vc, const float* __restrict__ vu,
                                                        float w, float dts, size_t n, float* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (VEC) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n / 4; i += stride) {
      const float4 b = reinterpret_cast<const float4*>(base)[i];
      const float4 c = reinterpret_cast<const float4*>(vc)[i], u = reinterpret_cast<const float4*>(vu)[i];
      reinterpret_cast<float4*>(out)[i] = make_float4(cfg_blend(b.x, c.x, u.x, w, dts), cfg_blend(b.y, c.y, u.y, w, dts),
                                                      cfg_blend(b.z, c.z, u.z, w, dts), cfg_blend(b.w, c.w, u.w, w, dts));
    }
  } else {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) out[i] = cfg_blend(base[i], vc[i], vu[i], w, dts);
  }
}

void launch_cfg_blend(const float* base, const float* vc, const float* vu, float w, float dts, size_t n, float* out, hipStream_t s) {
  if (n == 0) return;
  const bool vec = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(vc) | reinterpret_cast<uintptr_t>(vu) |
                                   reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const size_t threads = vec ? n / 4 : n;
  const int blocks = (int)((threads + 255) / 256 < 4096 ? (threads + 255) / 256 : 4096);
  if (vec) hipLaunchKernelGGL((cfg_blend_kernel<true>), dim3(blocks), dim3(256), 0, s, base, vc, vu, w, dts, n, out);
  else hipLaunchKernelGGL((cfg_blend_kernel<false>), dim3(blocks), dim3(256), 0, s, base, vc, vu, w, dts, n, out);
}

__global__ __launch_bounds__(256) void cfg_label_add_kernel(float* emb, const float* __restrict__ E, const int* __restrict__ labels,
                                                            int K, int temb, int* saved) {
  const int b = blockIdx.x;
  const int c = cfg_label(labels, b, K);
  for (int j = threadIdx.x; j < temb; j += blockDim.x) emb[(size_t)b * temb + j] += E[(size_t)c * temb + j];
  if (threadIdx.x == 0) saved[b] = c;
}

void launch_cfg_label_add(float* emb, const float* E, const int* labels, int K, int B, int temb, int* saved, hipStream_t s) {
  hipLaunchKernelGGL(cfg_label_add_kernel, dim3(B), dim3(256), 0, s, emb, E, labels, K, temb, saved);
}

__global__ __launch_bounds__(256) void cfg_label_grad_kernel(const float* __restrict__ g, const int* __restrict__ saved, int B,
                                                             int temb, float* __restrict__ dE) {
  const int c = blockIdx.x;
  for (int j = threadIdx.x; j < temb; j += blockDim.x) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b)
      if (saved[b] == c) acc += g[(size_t)b * temb + j];
    dE[(size_t)c * temb + j] = acc;
  }
}

void launch_cfg_label_grad(const float* g, const int* saved, int K, int B, int temb, float* dE, hipStream_t s) {
  hipLaunchKernelGGL(cfg_label_grad_kernel, dim3(K + 1), dim3(256), 0, s, g, saved, B, temb, dE);
}

}  // namespace rgfm
