// conv_mfma_hx2.hip -- the implicit-GEMM convolution of conv_mfma_bx3.hip with fp32 operands carried as
// TWO fp16 planes and the product formed on the f16 matrix cores (v_mfma_f32_32x32x16_f16, fp32 accumulate):
//     a' = S_A a,  a' ~= a_h + a_l,  a_h = f16(a'), a_l = f16(a' - a_h)      (round-to-nearest-even both times)
//     w' = s_w w,  w' ~= w_h + w_l   (s_w: a per-conv power of two that puts max|w| in [2^13, 2^14))
//     a'w' ~= a_l*w_h + a_h*w_l + a_h*w_h                                     (3 MFMAs, small terms first)
// Each plane carries 11 significand bits plus the sign of the residual, so a_h + a_l represents a' to
// 2^-24 |a'| (half an fp32 ulp) as long as a_l is a normal fp16, i.e. |a'| >= 2^-2; below that the
// absolute error is <= 2^-25 (|a| error <= 2^-29 at S_A = 16).  Every f16 x f16 product is exact in fp32
// and the dropped term a_l*w_l is < 2^-24 |a'w'|: per product the error is <= 3 * 2^-24 relative -- the
// class of conv_mfma_bx3.hip's 2^-23 -- at HALF its MFMA count.  The accumulators hold q = S_A s_w times
// the true sums (bias / time embedding / residual enter multiplied by q; the epilogue multiplies by 1/q;
// powers of two, exact).  Range: fp16 overflows at 65504, so |activation| must stay below 2048 (S_A = 16;
// GroupNorm+SiLU outputs are O(10)); the staging path raises ConvArgs::range_flag when it sees
// |a'| >= 32768 and the host re-runs the call on the split-bf16 kernel (fp32 range); convs whose
// weights fall outside [2^-40, 2^40] are never routed here (launch_pack_conv_hx2 reports it).
//
// Same fusion set, tiling, prologue (consumer-side GroupNorm) and epilogue as conv_mfma_bx3w_kernel.
// LDS records are 2 planes x 16 fp16 = 64 B; the four 16-byte slots of a record are XOR-swizzled with
// (record >> 2) & 3, so 16 consecutive records cover all 16 slot columns of the 256-byte bank row
// (conflict-free ds_read_b128).  DESIGN.md section 4 has the measurements.
//
// The kernel body, the weight packers and the host helpers are conv_planes.h's, shared with conv_mfma_bx3.hip; this file
// is the two-plane format (PlanesF16), the kernel's instantiations and the fp16-only conditions of its route.
// The stride-1 / upsampling convs run on conv_mfma_hx2p.hip's pipelined version of this kernel; this one keeps the
// stride-2 and transposed modes and the external scale/shift array path.
#include <stdlib.h>

#include "conv_planes.h"

namespace rgfm {

#ifdef RGFM_HX2_PROF
__device__ unsigned long long g_hx2_prof[10];  // (slots: conv_planes.h)
#endif

// Two scaled fp16 planes: 64-byte records (conv_hx2_common.h: HRW) whose four 16-byte slots are XOR-swizzled (hswz); plane
// l of a slot sits at its byte offset ^ 32; three products (hx_mma3).
struct PlanesF16 {
  static constexpr bool SCALED = true;
  static constexpr bool SMALL_EARLY = true;
  static constexpr int NPL = 2, RW = HRW;
  typedef f16x8 frag;
  static __device__ __forceinline__ int slot(int rec, int half) { return hswz(rec, 0, half); }
  static __device__ __forceinline__ int plane(int off, int p) { return p ? off ^ 32 : off; }
  static __device__ __forceinline__ int wfrag_base(int rec, int) { return rec * HRW; }
  static __device__ __forceinline__ int wfrag_sw(int rec) { return (rec >> 2) & 3; }
  static __device__ __forceinline__ int wfrag_slot(int sw, int hp) { return ((hp ^ sw) & 3) * 16; }
  static __device__ __forceinline__ void load(f16x8 (&f)[2], const char* base, int o0) {
    f[0] = *reinterpret_cast<const f16x8*>(base + o0);
    f[1] = *reinterpret_cast<const f16x8*>(base + (o0 ^ 32));
  }
  static __device__ __forceinline__ void split2(float a, float b, unsigned (&p)[2]) { hsplit2(a, b, p[0], p[1]); }
  template <int NT>
  static __device__ __forceinline__ void mma(f32x16 (&acc)[2][NT], const f16x8 (&af)[2][2], const f16x8 (&bf)[NT][2]) { hx_mma3<NT>(acc, af, bf); }
  static __device__ __forceinline__ const void* wmain(const ConvArgs& a) { return a.wpkh; }
  static __device__ __forceinline__ const void* wskip(const ConvArgs& a) { return a.wskiph; }
#ifdef RGFM_HX2_PROF
  static constexpr bool PROF = true;
  static __device__ __forceinline__ unsigned long long* prof() { return g_hx2_prof; }
#else
  static constexpr bool PROF = false;
  static __device__ __forceinline__ unsigned long long* prof() { return nullptr; }
#endif
};

template <int NT, int MODE, bool PAIRN>
__global__ __launch_bounds__(512, 2) void conv_mfma_hx2_kernel(const ConvArgs a, const int num_tiles) {
  conv_planes_body<PlanesF16, NT, MODE, PAIRN>(a, num_tiles);
}
struct Hx2Kernel {
  template <int NT, int MODE, bool PAIRN>
  static auto get() { return &conv_mfma_hx2_kernel<NT, MODE, PAIRN>; }
};

// ---------------------------------------------------------------- weight packing (scaled 2-way fp16 split)
// Per-conv scale: hq[0] = q = S_A s_w, hq[1] = 1 / q, hq[2] = s_w, hq[3] = 1 when the conv may run on this
// kernel (finite weights with max|w| in [2^-40, 2^40]; an all-zero tensor counts as in range, s_w = 1).
__global__ void hx2_scale_kernel(const float* w, size_t n, float* hq) {
  __shared__ float red[256];
  float m = 0.f;
  bool bad = false;
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
    const float v = fabsf(w[i]);
    if (!(v <= 3.0e38f)) bad = true;  // inf / nan
    m = fmaxf(m, v);
  }
  red[threadIdx.x] = bad ? __builtin_inff() : m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float mx = red[0];
    float sw = 1.f, ok = 1.f;
    if (mx > 0.f) {
      if (!(mx <= 3.0e38f)) {
        ok = 0.f;
      } else {
        const int e = ilogbf(mx);  // 2^e <= mx < 2^(e+1)
        if (e < -40 || e > 40) ok = 0.f;
        else sw = ldexpf(1.f, 13 - e);  // mx s_w in [2^13, 2^14)
      }
    }
    hq[0] = HX_SA * sw, hq[1] = 1.f / (HX_SA * sw), hq[2] = sw, hq[3] = ok;
  }
}

void hx2_scale_launch(const float* w, size_t n, float* hq, hipStream_t s) {  // (for conv_mfma_hx2w.hip's transformed weights)
  hipLaunchKernelGGL(hx2_scale_kernel, dim3(1), dim3(256), 0, s, w, n, hq);
}

// scale record first, then the image (conv_planes.h: launch_pack_planes; the kernels read s_w = hq[2] on the stream)
void launch_pack_conv_hx2(const float* w, void* out, float* hq, int Cout, int Cin, int taps, int mode, hipStream_t s) {
  const size_t n = (size_t)Cout * Cin * (mode == CONV_T2 ? 16 : taps);
  hipLaunchKernelGGL(hx2_scale_kernel, dim3(1), dim3(256), 0, s, w, n, hq);
  launch_pack_planes<PlanesF16>(w, out, hq, Cout, Cin, taps, mode, s);
}

bool conv_hx2_supported(const ConvArgs& a, int mode) {
  if (!a.wpkh || !a.hq || !a.range_flag) return false;
  if (a.res_mode == 2 && (!a.wskiph || !a.hq_skip)) return false;
  return conv_planes_shape_ok<PlanesF16>(a, mode);
}
bool conv_hx2_gn_supported(const ConvArgs& a, int mode) { return conv_planes_gn_ok(a) && conv_hx2_supported(a, mode); }

int conv_hx2_init() { return conv_planes_init<Hx2Kernel>(); }
bool launch_conv_hx2(const ConvArgs& a, int mode, hipStream_t s) { return launch_conv_planes<PlanesF16, Hx2Kernel>(a, mode, s); }

}  // namespace rgfm
