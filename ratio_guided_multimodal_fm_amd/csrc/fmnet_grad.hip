// fmnet_grad.hip -- the dense layers of FlowMatchingModel's training pass (reference src/models/flow_matching.py:53,
// :85: encoder.fc 12544 -> F and decoder.fc1 F + T -> 12544) as GEMMs on v_mfma_f32_32x32x2_f32.
//
// Everything else of that pass runs on unet_grad.hip: the 3x3 convs and -- as the data gradient / forward / weight
// gradient of a 4x4 stride-2 conv -- both ConvTranspose2d layers on ug_igemm_kernel, GroupNorm + SiLU on ug_gn_*.
// This kernel shares their GEMM core (ug_mfma_chunk, train_device.h): block tile 64 x 64, K staged 16 at a time.
// The six GEMMs of the two layers differ only in which operand is contiguous along k:
//   forward   y[b][o]  = sum_i x[b][i] W[o][i]      A = x row-major,  B = W row-major   (fc: K = 12544, split-K)
//   dgrad     dx[b][i] = sum_o dy[b][o] W[o][i]     A = dy row-major, B = W K-major     (fc1: K = 12544, split-K)
//   wgrad     dW[o][i] = sum_b dy[b][o] x[b][i]     A = dy K-major,   B = x K-major     (K = batch: one short pass
//             per tile of a 12544-wide output grid, no split)
// A row-major operand is staged like ug_igemm_kernel's (a thread owns 4 consecutive k of one row, one 16-byte load
// where alignment allows); a K-major operand with the thread mapping turned (64 consecutive rows per k), so that
// either way a wave's loads are contiguous.  Split-K writes partial slices that fg_reduce_kernel adds in split order:
// no float atomics, bitwise-reproducible results.
#include "rgfm_device.h"
#include "train_device.h"

namespace rgfm {

// 4 consecutive k (from k) of row r of an operand; zero beyond the row count R or kend
template <bool KMAJOR>
__device__ __forceinline__ void fg_load4(const float* p, int ld, int r, int R, int k, int kend, int vec, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (r >= R) return;
  if (KMAJOR) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j < kend) v[j] = p[(size_t)(k + j) * ld + r];
  } else if (vec && k + 3 < kend) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + (size_t)r * ld + k);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j < kend) v[j] = p[(size_t)r * ld + k + j];
  }
}

template <bool AK, bool BK>
__global__ __launch_bounds__(256) void fg_gemm_kernel(FgGemm g) {
  __shared__ __attribute__((aligned(16))) float sA[64 * LDP];
  __shared__ __attribute__((aligned(16))) float sB[64 * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int rowa = AK ? tid & 63 : tid >> 2, qa = AK ? tid >> 6 : tid & 3;
  const int rowb = BK ? tid & 63 : tid >> 2, qb = BK ? tid >> 6 : tid & 3;
  const int kbeg = blockIdx.z * g.kps;
  const int kend = min(g.K, kbeg + g.kps);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = kbeg; k0 < kend; k0 += KC) {
    float va[4], vb[4];
    fg_load4<AK>(g.a, g.lda, m0 + rowa, g.M, k0 + qa * 4, kend, g.veca, va);
    fg_load4<BK>(g.b, g.ldb, n0 + rowb, g.N, k0 + qb * 4, kend, g.vecb, vb);
    ug_mfma_chunk(sA, sB, rowa, qa, va, rowb, qb, vb, wm, wn, l31, h, acc);
  }
  const int n = n0 + wn * 32 + l31;
  if (n >= g.N) return;
  if (g.splits > 1) {
    float* out = g.part + (size_t)blockIdx.z * g.M * g.N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + ug_acc_row(r, h);
      if (m < g.M) out[(size_t)m * g.N + n] = acc[r];
    }
    return;
  }
  const float bias = g.bias ? g.bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + ug_acc_row(r, h);
    if (m < g.M) g.c[(size_t)m * g.ldc + n] = acc[r] + bias;
  }
}

// c[m][n] = bias[n] + sum over z (ascending) of part[z][m][n]
__global__ void fg_reduce_kernel(const float* part, int splits, int M, int N, const float* bias, float* c, int ldc) {
  const size_t total = (size_t)M * N;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += part[(size_t)z * total + i];
    c[(size_t)m * ldc + n] = bias ? v + bias[n] : v;
  }
}

void launch_fg_gemm(FgGemm g, bool a_kmajor, bool b_kmajor, hipStream_t s) {
  // 16-byte loads of a row-major operand: every row start and every chunk start (multiples of 4 floats) aligned
  g.veca = !a_kmajor && g.lda % 4 == 0 && reinterpret_cast<uintptr_t>(g.a) % 16 == 0;
  g.vecb = !b_kmajor && g.ldb % 4 == 0 && reinterpret_cast<uintptr_t>(g.b) % 16 == 0;
  const dim3 grid((g.N + 63) / 64, (g.M + 63) / 64, g.splits);
  if (a_kmajor && b_kmajor) hipLaunchKernelGGL((fg_gemm_kernel<true, true>), grid, dim3(256), 0, s, g);
  else if (b_kmajor) hipLaunchKernelGGL((fg_gemm_kernel<false, true>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((fg_gemm_kernel<false, false>), grid, dim3(256), 0, s, g);
  if (g.splits > 1) {
    const size_t total = (size_t)g.M * g.N;
    hipLaunchKernelGGL(fg_reduce_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 2048)), dim3(256), 0, s,
                       g.part, g.splits, g.M, g.N, g.bias, g.c, g.ldc);
  }
}

}  // namespace rgfm
