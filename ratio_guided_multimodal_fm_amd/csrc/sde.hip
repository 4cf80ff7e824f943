// sde.hip -- the state pre-update of the stochastic sampler step (include/rgfm.h, "Stochastic sampling") and its noise.
//
//   base[e] = a x[e] + sigma xi[e],      a = (float)(1 - eta dt),  sigma = (float)sqrt(2 eta (1 - t) dt)
//
// over the flat [batch][D] state, one pass: 4 bytes read and 4 written per element, xi generated in registers.  xi is a
// counter-based Gaussian: pair p = e / 2 hashes (key, p) with the splitmix64 finaliser of the dropout masks into one
// 64-bit word, whose two 24-bit fields are the uniforms of one Box-Muller pair (cosine to 2p, sine to 2p + 1).  The key
// -- fin(seed, stream, step) -- is formed once per launch on the host (sde_key, rgfm_host.h).  Nothing depends on the
// grid, the batch size or the call's step range: element e of (seed, stream, step) has one value.
//
// A thread owns 8 consecutive elements (4 pairs): two 16-byte loads, two 16-byte stores when both pointers are 16-byte
// aligned, the same 8 elements one by one otherwise; the last n % 8 elements go pair by pair to one more thread.  The
// arithmetic per element is the same on every path (sde_pair, then one fma), so the path does not change a bit.
#include "rgfm_device.h"

namespace rgfm {

__device__ __forceinline__ uint64_t sde_fin(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the Gaussian pair p of `key`: u1 in (0, 1] and u2 in [0, 1) are exact fp32 values, 2 u2 is an exact argument of
// sincospif (no rounding of 2 pi u2), logf is the precise one
__device__ __forceinline__ void sde_pair(uint64_t key, uint64_t p, float& c, float& s) {
  const uint64_t z = sde_fin(key + 0x9E3779B97F4A7C15ull * (p + 1ull));
  const float u1 = (float)((uint32_t)(z >> 40) + 1u) * (1.0f / 16777216.0f);
  const float u2 = (float)((uint32_t)(z >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);
  c = r * cs, s = r * sn;
}

// STATE: out = a x + sigma xi; else out = xi (the test hook: x is not read)
template <bool STATE>
__device__ __forceinline__ float sde_elem(float x, float xi, float a, float sigma) {
  return STATE ? fmaf(a, x, sigma * xi) : xi;
}

template <bool STATE, bool VEC>
__global__ void sde_pre_kernel(const float* __restrict__ x, float* __restrict__ out, size_t n, uint64_t key, float a, float sigma) {
  const size_t groups = n / 8;  // whole groups of 8 elements; thread `groups` (of the grid-stride order) takes the tail
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g <= groups; g += (size_t)gridDim.x * blockDim.x) {
    const size_t e0 = g * 8;
    if (g < groups) {
      float xv[8], xi[8];
      if (STATE) {
        if (VEC) {
          const float4 lo = *reinterpret_cast<const float4*>(x + e0), hi = *reinterpret_cast<const float4*>(x + e0 + 4);
          xv[0] = lo.x, xv[1] = lo.y, xv[2] = lo.z, xv[3] = lo.w, xv[4] = hi.x, xv[5] = hi.y, xv[6] = hi.z, xv[7] = hi.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) xv[j] = x[e0 + j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) sde_pair(key, g * 4 + j, xi[2 * j], xi[2 * j + 1]);
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = sde_elem<STATE>(STATE ? xv[j] : 0.f, xi[j], a, sigma);
      if (VEC) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(out + e0 + 4) = make_float4(o[4], o[5], o[6], o[7]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) out[e0 + j] = o[j];
      }
    } else {  // the last n % 8 elements (none: nothing to do); an odd n ends on a cosine
      for (size_t e = e0; e < n; e += 2) {
        float c, s;
        sde_pair(key, e / 2, c, s);
        out[e] = sde_elem<STATE>(STATE ? x[e] : 0.f, c, a, sigma);
        if (e + 1 < n) out[e + 1] = sde_elem<STATE>(STATE ? x[e + 1] : 0.f, s, a, sigma);
      }
    }
  }
}

template <bool STATE>
static void launch_sde(const float* x, float* out, size_t n, uint64_t key, float a, float sigma, hipStream_t s) {
  if (n == 0) return;
  const size_t threads = n / 8 + 1;
  const int blocks = (int)((threads + 255) / 256 < 2048 ? (threads + 255) / 256 : 2048);
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (vec) hipLaunchKernelGGL((sde_pre_kernel<STATE, true>), dim3(blocks), dim3(256), 0, s, x, out, n, key, a, sigma);
  else hipLaunchKernelGGL((sde_pre_kernel<STATE, false>), dim3(blocks), dim3(256), 0, s, x, out, n, key, a, sigma);
}

void launch_sde_pre(const float* x, float* base, size_t n, uint64_t key, float a, float sigma, hipStream_t s) {
  launch_sde<true>(x, base, n, key, a, sigma, s);
}
void launch_sde_noise(float* out, size_t n, uint64_t key, hipStream_t s) { launch_sde<false>(nullptr, out, n, key, 0.f, 0.f, s); }

}  // namespace rgfm
