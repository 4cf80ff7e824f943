// conv_hx2_common.h -- device helpers shared by the two-plane fp16 conv kernels (conv_mfma_hx2{,p,q,s,c,d,w}.hip): the
// split, the LDS record layout, the P format, and the blocks every kernel of the family runs the same way -- table rows
// and zero row of the consumer-side GroupNorm (over rgfm_device.h: gn_table_row), chunk descriptors, the three-product
// MFMA step (hx_mma3, HxFrag), accumulator set-up (hx_acc_init), low-range scan and 64-pixel statistics of the epilogue.
// See the header comment of conv_mfma_hx2.hip for the arithmetic.
#pragma once
#include "rgfm_device.h"

namespace rgfm {

typedef __attribute__((address_space(1))) f32x4 hx_gf32x4;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float hx_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned hx_u32x2 __attribute__((ext_vector_type(2)));

constexpr float HX_SA = 16.f;         // activation scale S_A
constexpr float HX_LIMIT = 32768.f;   // |a'| at or above this raises the range flag

// 2-way fp16 split of two (already scaled) floats: planes h, l as packed fp16 pairs.  h = v_cvt_pk_f16_f32 (RNE); the
// remainder a - float(h) in ONE v_fma_mix_f32 per value (the fp16 half is an operand: no v_cvt_f32_f16, and no packed
// v_pk_add_f32, which hipcc makes of the vector form and which is an anti-lever beside MFMAs); exact either way, so the
// planes are bit for bit those of the conversion + subtraction form.  The staging path is VALU-issue-bound in the MFMA
// shadow (tools/ubench/mfma_valu_overlap.hip: ~5.5 vector instructions per MFMA slot from the other waves of a SIMD):
// every instruction per item counts.
__device__ __forceinline__ void hsplit2(float a, float b, unsigned& ph, unsigned& pl) {
  hx_f32x2 v = {a, b};
  const f16x2 h = __builtin_convertvector(v, f16x2);
  ph = __builtin_bit_cast(unsigned, h);
  float la, lb;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(la) : "v"(ph), "v"(a));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(lb) : "v"(ph), "v"(b));
  const hx_f32x2 lv = {la, lb};
  pl = __builtin_bit_cast(unsigned, __builtin_convertvector(lv, f16x2));
}

// High side of the staging path: plane h = fp16(S_A a) reaches 32768 (fp16's top binade, where the remainder plane stops
// being exact -- and 65520 rounds to inf) from |S_A a| >= 32760 (round to nearest even).  The running max is taken on
// the fp32 values before the split: v_max3_f32 with |.| source modifiers, one instruction per two values.  A NaN is not
// caught here and need not be: it propagates into every output it touches, as in the reference.
constexpr float HX_BIG = 32760.f;
__device__ __forceinline__ float hx_absmax3(float a, float b, float m) {
  return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a), __builtin_fabsf(b)), m);
}

// S_A silu(z) from z' = S_A z (v_exp_f32 + v_rcp_f32 as silu_fast)
__device__ __forceinline__ float silu_scaled(float zs) {
  const float e = __builtin_amdgcn_exp2f(zs * (-1.44269504088896341f / HX_SA));
  return zs * __builtin_amdgcn_rcpf(1.0f + e);
}

// (HX_SMALL / hx_small_flag, the low side of the raw staging path, live in rgfm_device.h: the bf16x3 and fp32 kernels
// check it too when they produce a tensor that a two-plane conv stages raw)

// ---- "P format": an activation ALREADY normalised, activated and split, as the consumer's MFMAs read it
// (conv_mfma_hx2d.hip stages it by LDS-DMA only).  One (pixel, 16-channel chunk) = 64 B:
//   [plane h: channels 0 .. 15 | plane l: channels 0 .. 15]  fp16 of S_A silu(scale x + shift),   [B][H][W][C / 16][64 B]
// -- the bytes of the fp32 map it replaces.  Written by the producing conv's epilogue where a workgroup owns whole
// (sample, GroupNorm group) sets (ConvArgs::pout), or by launch_hx_presplit.

// exchange between the two lanes of a channel pair (2 k, 2 k + 1): DPP quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float hx_swap1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}

// GroupNorm scale / shift (x S_A) of this lane's channel from its (mean, M2) over n pixels, when all `cpg` channels of
// its group sit in consecutive lanes of ONE wave (cpg a power of two <= 32; both lane halves hold the same values).
// gn_table_row's formula (rgfm_device.h; fp64: N, sum n mean, sum M2 + n mean^2 -> mean, var), here with one channel per
// lane and a butterfly over the group's lanes.
// (hx_group_affine_s: from the channel's sums s1 = sum n_p mean_p, s2 = sum M2_p + n_p mean_p^2 over its parts, n pixels in all)
__device__ __forceinline__ void hx_group_affine_s(double s1, double s2, double n, int cpg, float gamma, float beta, float& sc, float& sh) {
  for (int o = 1; o < cpg; o <<= 1) s1 += __shfl_xor(s1, o), s2 += __shfl_xor(s2, o);
  const double N = n * (double)cpg, mean = s1 / N, var = s2 / N - mean * mean;
  const float rstd = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + 1e-5));
  const float a = rstd * gamma;
  sc = HX_SA * a;
  sh = HX_SA * (beta - (float)mean * a);
}
__device__ __forceinline__ void hx_group_affine(float mean_c, float m2_c, float n, int cpg, float gamma, float beta, float& sc, float& sh) {
  double s1 = (double)n * (double)mean_c, s2 = (double)m2_c + (double)n * (double)mean_c * (double)mean_c;
  for (int o = 1; o < cpg; o <<= 1) s1 += __shfl_xor(s1, o), s2 += __shfl_xor(s2, o);
  const double N = (double)n * (double)cpg, mean = s1 / N, var = s2 / N - mean * mean;
  const float rstd = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + 1e-5));
  const float a = rstd * gamma;
  sc = HX_SA * a;
  sh = HX_SA * (beta - (float)mean * a);
}

// One wave's 64 pixels x 32 channels (accumulator layout: channel = lane & 31, acc<mt>[r] = pixel 32 mt + (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5) of the block) as P records: S_A silu(sc x + sh), split, two channels per lane -- the lanes of a
// channel pair trade one value of every pixel pair, so each holds (2 k, 2 k + 1) of ONE pixel -- and one 4-byte store per
// plane.  rec0: the record of (pixel 0 of the block, this lane's chunk); pstride: bytes per pixel (C / 16 x 64).
// Returns the largest |S_A silu(.)| seen (the caller raises range-flag bit 0 on >= HX_BIG, as the staging paths do).
__device__ __forceinline__ float hx_p_emit(const f32x16& acc0, const f32x16& acc1, float sc, float sh, char* rec0, unsigned pstride, int l31, int hp) {
  const bool odd = (l31 & 1) != 0;
  char* const base = rec0 + ((l31 & 15) >> 1) * 4 + (size_t)(4 * hp + (odd ? 1 : 0)) * pstride;
  float m = 0.f;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const f32x16& am = mt ? acc1 : acc0;
      const float o0 = silu_scaled(fmaf(sc, am[r], sh)), o1 = silu_scaled(fmaf(sc, am[r + 1], sh));
      const float recv = hx_swap1(odd ? o0 : o1);
      const float lo = odd ? recv : o0, hi = odd ? o1 : recv;
      m = hx_absmax3(lo, hi, m);
      unsigned ph, pl;
      hsplit2(lo, hi, ph, pl);
      char* const q = base + (size_t)(32 * mt + (r & 3) + 8 * (r >> 2)) * pstride;
      *reinterpret_cast<unsigned*>(q) = ph;
      *reinterpret_cast<unsigned*>(q + 32) = pl;
    }
  return m;
}

constexpr int HRW = 64;  // bytes per LDS record: [plane h | plane l] x 16 fp16
// byte offset of 16-byte slot (plane, half) inside record `rec`
__device__ __forceinline__ int hswz(int rec, int plane, int half) { return (((2 * plane + half) ^ (rec >> 2)) & 3) * 16; }

// ---- prologue blocks of the kernels that keep a [rows + 1][cin][2] scale/shift table and chunk descriptors in LDS

// The table rows of a workgroup's `rows` (1, 2 or 4) consecutive samples b_first, b_first + 1, ... in one shot: rows side
// by side on the waves, 2^wsh waves per row -- gn_waves_log2(cin / 8) of them, but no more than 2^wsh_max (what the
// workgroup's wave count leaves per row).  Rows of samples past the batch are not written (never read: their items
// take the zero row).
__device__ __forceinline__ void hx_gn_table_rows(const ConvArgs& a, int rows, int wsh_max, int b_first, float* sTab, int cin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpg = cin >> 3, need = gn_waves_log2(cpg);
  const GnLane L(wave, lane, wsh_max < need ? wsh_max : need, cpg);
  const int b = b_first + L.row;
  if (L.row < rows && b < a.B) gn_table_row(a, L, b, true, sTab + (size_t)L.row * cin * 2, HX_SA);
}
// the all-zero row behind the table: out-of-image / out-of-batch items point at it, so silu(0 x + 0) = 0 is the padding
__device__ __forceinline__ void hx_tab_zero_row(float* sTab, int rows, int cin, int nthr) {
  for (int i = threadIdx.x; i < 2 * cin; i += nthr) sTab[rows * cin * 2 + i] = 0.f;
}

// chunk descriptors: which tensor a 16-channel chunk comes from (input / concat partner / 1x1-skip sources), one
// 16-byte record per chunk: {pointer to the chunk's first channel (lo, hi), channel stride of that source, -}
typedef unsigned hx_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void hx_store_chunk_desc(const ConvArgs& a, char* sDesc, int nmain, int ntot) {
  const int tid = threadIdx.x;
  if (tid < ntot) {
    const bool skip = tid >= nmain;
    const int c = (skip ? tid - nmain : tid) * KC;
    const float* src;
    int cs, cc;
    if (!skip) {
      if (c < a.C0) src = a.in0, cs = a.C0, cc = c;
      else src = a.in1, cs = a.C1, cc = c - a.C0;
    } else {
      if (c < a.R0) src = a.res0, cs = a.R0, cc = c;
      else src = a.res1, cs = a.R1, cc = c - a.R0;
    }
    const unsigned long long pv = reinterpret_cast<unsigned long long>(src + cc);
    const hx_u32x4 d = {(unsigned)pv, (unsigned)(pv >> 32), (unsigned)cs, 0u};
    *reinterpret_cast<hx_u32x4*>(sDesc + tid * 16) = d;
  }
}

// ---- the three f16 products of one fp32 product, for a wave tile of 2 pixel tiles x NT channel tiles:
// a_l w_h, a_h w_l, a_h w_h (small terms first).  af[mt][plane], bf[nt][plane]; plane 0 = h, 1 = l.
template <int NT>
__device__ __forceinline__ void hx_mma3(f32x16 (&acc)[2][NT], const f16x8 (&af)[2][2], const f16x8 (&bf)[NT][2]) {
  constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[mt][PA[q]], bf[nt][PB[q]], acc[mt][nt], 0, 0, 0);
}
// One tap's fragments of a 64-pixel x 32 NT-channel wave tile whose second pixel tile sits mt_off bytes behind the first:
// 4 + 2 NT reads (plane l of a record is plane h's slot ^ 2, i.e. the byte offset ^ 32), then hx_mma3
template <int NT = 1>
struct HxFrag {
  f16x8 a[2][2], b[NT][2];
  __device__ __forceinline__ void load(const char* sArow, int o0, int mt_off, const char* sBt, const int (&bofs)[NT]) {
    const int o1 = o0 ^ 32;
    a[0][0] = *reinterpret_cast<const f16x8*>(sArow + o0);
    a[0][1] = *reinterpret_cast<const f16x8*>(sArow + o1);
    a[1][0] = *reinterpret_cast<const f16x8*>(sArow + o0 + mt_off);
    a[1][1] = *reinterpret_cast<const f16x8*>(sArow + o1 + mt_off);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      b[nt][0] = *reinterpret_cast<const f16x8*>(sBt + bofs[nt]);
      b[nt][1] = *reinterpret_cast<const f16x8*>(sBt + (bofs[nt] ^ 32));
    }
  }
  __device__ __forceinline__ void load(const char* sArow, int o0, int mt_off, const char* sBt, int bofs) {
    static_assert(NT == 1, "one weight offset: one channel column");
    const int bo[1] = {bofs};
    load(sArow, o0, mt_off, sBt, bo);
  }
  __device__ __forceinline__ void mma(f32x16 (&acc)[2][NT]) const { hx_mma3<NT>(acc, a, b); }
};

// ---- accumulator set-up of a wave tile whose 64 pixels are consecutive in the output (the 8x8 / 16x16 kernels): bias
// (+ skip bias + time term of `sample`), scaled by q -- the accumulators hold q x the true sums; an identity residual
// (its 64 pixels start at pixel pixr; channel ch0 + 32 nt) enters as fma(res, q, .)
template <bool SKIP, int NT>
__device__ __forceinline__ void hx_acc_init(f32x16 (&acc)[2][NT], const ConvArgs& a, int sample, size_t pixr, int ch0, int hp, float qmain) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int ch = ch0 + 32 * nt;
    float v = a.bias[ch];
    if (SKIP) v += a.skip_bias[ch];
    if (a.temb) v += a.temb[((size_t)(a.temb_per_row ? (sample < a.B ? sample : 0) : 0) + (a.step_ptr ? (size_t)*a.step_ptr : 0)) * a.temb_stride + ch];
    const float add0 = v * qmain;
    if (!SKIP && a.res_mode == 1) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = a.res0[(pixr + hx_acc_pixel(mt, r, hp)) * a.Cout + ch];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = fmaf(acc[mt][nt][r], qmain, add0);
    } else {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = add0;
    }
  }
}

// ---- epilogue blocks

// ConvArgs::small_check, every pixel valid: largest |output| of the wave's block -> range-flag bit 1 (hx_small_flag)
template <int NT>
__device__ __forceinline__ void hx_small_scan(unsigned* flag, const f32x16 (&acc)[2][NT]) {
  float m = 0.f;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; r += 2) m = hx_absmax3(acc[mt][nt][r], acc[mt][nt][r + 1], m);
  hx_small_flag(flag, m);
}
// (mean, M2) of column nt over the wave's 64 valid pixels (both lane halves get the same pair)
template <int NT>
__device__ __forceinline__ void hx_stats64(const f32x16 (&acc)[2][NT], int nt, float& mean_out, float& m2_out) {
  float s = 0.f;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[mt][nt][r];
  s += __shfl_xor(s, 32);
  const float mean = s / 64.f;
  float m2 = 0.f;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = acc[mt][nt][r] - mean;
      m2 += d * d;
    }
  m2 += __shfl_xor(m2, 32);
  mean_out = mean, m2_out = m2;
}

}  // namespace rgfm
