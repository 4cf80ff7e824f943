// conv_mfma_bx3.hip -- the implicit-GEMM convolution of conv_mfma.hip with fp32 operands carried as
// three bf16 planes (a = a_h + a_m + a_l, an EXACT decomposition of the 24-bit significand) and the
// product formed on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulate) as
//     a*b ~= a_l*b_h + a_h*b_l + a_m*b_m + a_m*b_h + a_h*b_m + a_h*b_h        (6 MFMAs, small terms first)
// Every bf16 x bf16 product is exact in fp32; the dropped terms (a_m*b_l, a_l*b_m, a_l*b_l) are
// < 2^-23 |a*b|, i.e. below the rounding of a single fp32 multiply.  The bf16 pipe runs 16x the
// fp32-MFMA rate, so six passes still leave ~2.7x of MFMA headroom over v_mfma_f32_32x32x2_f32.
//
// Same fusion set, register tile, prefetch structure and epilogue as conv_mfma_pf_kernel (see conv_mfma.hip), plus:
// stride-2 convs (four input parity phases), the consumer-side GroupNorm (scale/shift derived in the prologue from
// the producers' partial statistics) and the producer-side finalize (rgfm_device.h).  Differences in the data path:
// LDS records are 3 planes x 16 bf16 = 96 B, unpadded, halves swapped on odd groups of 8 records (conflict-free
// ds_read_b128); the staging path splits the (GroupNorm+SiLU-transformed) activations; weights arrive pre-split, as
// the byte image of the LDS tile, from launch_pack_conv_bx3 / _s2 / launch_pack_deconv_bx3; one 512-thread
// workgroup per CU (two waves per SIMD, 100-155 KB of LDS).  DESIGN.md section 4 has the measurements.
//
// The kernel body, the weight packers and the host helpers are conv_planes.h's, shared with conv_mfma_hx2.hip; this file
// is the three-plane format (PlanesBf16), the kernel's instantiations and the conditions of its route.
#include <stdlib.h>

#include "conv_planes.h"

namespace rgfm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// exact 3-way bf16 split of two floats: planes h, m, l as packed bf16 pairs
__device__ __forceinline__ void split2(float a, float b, unsigned& ph, unsigned& pm, unsigned& pl) {
  f32x2 v = {a, b};
  ph = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  f32x2 hf = {__builtin_bit_cast(float, ph << 16), __builtin_bit_cast(float, ph & 0xffff0000u)};
  v = v - hf;
  pm = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  f32x2 mf = {__builtin_bit_cast(float, pm << 16), __builtin_bit_cast(float, pm & 0xffff0000u)};
  v = v - mf;
  pl = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

#ifdef RGFM_BX3_PROF
__device__ unsigned long long g_bx3_prof[10];  // (slots: conv_planes.h)
#endif

// Three exact bf16 planes: 96-byte records [h | m | l] x 16 bf16, the two 16-byte halves of every plane swapped on odd
// groups of 8 records; six products, small terms first.  No scaling: fp32 range.
struct PlanesBf16 {
  static constexpr bool SCALED = false;
  static constexpr bool SMALL_EARLY = false;
  static constexpr int NPL = 3, RW = 96;
  typedef bf16x8 frag;
  static __device__ __forceinline__ int slot(int rec, int half) { return ((half ^ (rec >> 3)) & 1) * 16; }
  static __device__ __forceinline__ int plane(int off, int p) { return off + 32 * p; }
  static __device__ __forceinline__ int wfrag_base(int rec, int hp) { return rec * 96 + slot(rec, hp); }
  static __device__ __forceinline__ int wfrag_sw(int) { return 0; }
  static __device__ __forceinline__ int wfrag_slot(int, int) { return 0; }
  static __device__ __forceinline__ void load(bf16x8 (&f)[3], const char* base, int o0) {
#pragma unroll
    for (int p = 0; p < 3; ++p) f[p] = *reinterpret_cast<const bf16x8*>(base + o0 + p * 32);
  }
  static __device__ __forceinline__ void split2(float a, float b, unsigned (&p)[3]) { rgfm::split2(a, b, p[0], p[1], p[2]); }
  template <int NT>
  static __device__ __forceinline__ void mma(f32x16 (&acc)[2][NT], const bf16x8 (&af)[2][3], const bf16x8 (&bf)[NT][3]) {
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt][PA[q]], bf[nt][PB[q]], acc[mt][nt], 0, 0, 0);
  }
  static __device__ __forceinline__ const void* wmain(const ConvArgs& a) { return a.wpk3; }
  static __device__ __forceinline__ const void* wskip(const ConvArgs& a) { return a.wskip3; }
#ifdef RGFM_BX3_PROF
  static constexpr bool PROF = true;
  static __device__ __forceinline__ unsigned long long* prof() { return g_bx3_prof; }
#else
  static constexpr bool PROF = false;
  static __device__ __forceinline__ unsigned long long* prof() { return nullptr; }
#endif
};

template <int NT, int MODE, bool PAIRN>
__global__ __launch_bounds__(512, 2) void conv_mfma_bx3w_kernel(const ConvArgs a, const int num_tiles) {
  conv_planes_body<PlanesBf16, NT, MODE, PAIRN>(a, num_tiles);
}
struct Bx3Kernel {
  template <int NT, int MODE, bool PAIRN>
  static auto get() { return &conv_mfma_bx3w_kernel<NT, MODE, PAIRN>; }
};

void launch_pack_conv_bx3(const float* w, void* out, int Cout, int Cin, int taps, hipStream_t s) {
  launch_pack_planes<PlanesBf16>(w, out, nullptr, Cout, Cin, taps, CONV_S1, s);
}
void launch_pack_conv_bx3_s2(const float* w, void* out, int Cout, int Cin, hipStream_t s) {
  launch_pack_planes<PlanesBf16>(w, out, nullptr, Cout, Cin, 9, CONV_S2, s);
}
void launch_pack_deconv_bx3(const float* w, void* out, int Cin, int Cout, hipStream_t s) {
  launch_pack_planes<PlanesBf16>(w, out, nullptr, Cout, Cin, 16, CONV_T2, s);
}

bool conv_bx3_supported(const ConvArgs& a, int mode) {
  if (!a.wpk3 || a.ep_scale) return false;  // (the BatchNorm+SiLU epilogue of the ratio nets stays on conv_mfma.hip)
  if (a.res_mode == 2 && !a.wskip3) return false;
  if (mode == CONV_S2 && g_conv_tuning.s2_f32) return false;  // (RGFM_S2_F32, A/B switch: stride-2 convs on the fp32 kernel)
  return conv_planes_shape_ok<PlanesBf16>(a, mode);
}
bool conv_bx3_gn_supported(const ConvArgs& a, int mode) { return conv_planes_gn_ok(a) && conv_bx3_supported(a, mode); }

int conv_bx3_init() { return conv_planes_init<Bx3Kernel>(); }
bool launch_conv_bx3(const ConvArgs& a, int mode, hipStream_t s) { return launch_conv_planes<PlanesBf16, Bx3Kernel>(a, mode, s); }

}  // namespace rgfm
