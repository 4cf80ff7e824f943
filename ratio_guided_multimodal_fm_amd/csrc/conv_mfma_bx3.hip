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
#include <stdlib.h>

#include <type_traits>

#include "rgfm_device.h"

namespace rgfm {

typedef __attribute__((address_space(1))) f32x4 bx_gf32x4;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

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

// ------------------------------------------------------------------------------------
// Workgroup = 512 threads = 2 waves per SIMD (one wave alone cannot keep the bf16 MFMA pipe issuing
// back to back), built as TWO of conv_mfma_pf_kernel's 4-wave tiles sharing one operand in LDS:
//   PAIRN  (Cout % (64 NT) == 0): one 256-pixel tile x two adjacent 32NT-channel groups -- the
//          activation halo (the expensive GroupNorm+SiLU+split staging) is staged once for both;
//   !PAIRN: two consecutive 256-pixel tiles x one channel group -- the weights are staged once.
// LDS records are unpadded (96 B) with the two 16-byte halves of a plane swapped on odd groups of
// 8 records, which keeps ds_read_b128 conflict-free for 16 consecutive records.
// ------------------------------------------------------------------------------------
#ifdef RGFM_BX3_PROF
__device__ unsigned long long g_bx3_prof[10];  // prologue, issue, mfma, commit-wait, commit-A, commit-B, epilogue, blocks, [8] shader clk, [9] 100 MHz ticks
#define PROF_T(var) const long long var = clock64()
#define PROF_ADD(slot, t0, t1) prof_acc[slot] += (t1) - (t0)
#else
#define PROF_T(var)
#define PROF_ADD(slot, t0, t1)
#endif

constexpr int RW = 96;
__device__ __forceinline__ int swz(int rec, int half) { return ((half ^ (rec >> 3)) & 1) * 16; }

template <int NT, int MODE, bool PAIRN>
__global__ __launch_bounds__(512, 2) void conv_mfma_bx3w_kernel(const ConvArgs a, const int num_tiles) {
  // CONV_S2 (3x3, stride 2, pad 1): the input is read as its four pixel-parity phases (a, b) = (row & 1, col & 1),
  // each a plane of the OUTPUT's size; output (r, x) takes phase (a, b) at plane offsets dr in {-1 (a = 1 only), 0},
  // dx likewise, i.e. 1 / 2 / 2 / 4 taps for phases (0,0) / (0,1) / (1,0) / (1,1) -- 9 in all, nothing multiplied by
  // zero.  The K loop runs over (phase, 16-channel chunk); a halo tile is one phase plane, staged like CONV_S1.
  constexpr int NTAPS = (MODE == CONV_T2 || MODE == CONV_S2) ? 4 : 9;  // weight taps resident in LDS
  constexpr int NG = PAIRN ? 2 : 1;            // channel groups per block
  constexpr int NA = PAIRN ? 1 : 2;            // pixel tiles per block
  constexpr int NBLK = 32 * NT;                // channels per group
  constexpr int NBIG = NTAPS * NBLK * 6;       // 16-byte weight items per chunk and group
  constexpr int NB = (NBIG * NG + 511) / 512;
  constexpr int MAXIT = (NA * 448 * 4 + 511) / 512;
  extern __shared__ __attribute__((aligned(16))) char smem3[];
#ifdef RGFM_BX3_PROF
  long long prof_acc[7] = {0, 0, 0, 0, 0, 0, 0};
  const long long wall0 = wall_clock64();
#endif
  PROF_T(tp0);
  char* sA = smem3;
  char* sB = smem3 + NA * a.halo_px * RW;
  float* sAB = reinterpret_cast<float*>(sB + NTAPS * NBLK * NG * RW);  // [NA * spt][16][2]   (external `ab` path)
  float* sG = sAB + 256;                                                // [NA * spt][8][2] group (mean, rstd)
  float* sTab = sG + 128;                                               // [NA * spt][cin][2] (consumer-side GroupNorm)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave >> 2, seg = wave & 3;
  const int l31p = lane & 31, hp_ = lane >> 5;
  const TileGeom g = a.g;
  const int W = g.W, H = g.H, HW = g.HW;

  // tile origins of the block's one or two pixel tiles (block-uniform: scalar registers)
  auto tile_origin = [&](int tile, int& b0, int& row0) {
    if (tile >= num_tiles) {
      b0 = a.B, row0 = 0;  // idle half of the last block: every sample index is out of range
    } else if (g.spt == 1) {
      b0 = tile / g.tps;
      row0 = (tile - b0 * g.tps) * g.th;
    } else {
      b0 = tile * g.spt;
      row0 = 0;
    }
  };
  int tb0_[2], trow0_[2];
  tile_origin(PAIRN ? (int)blockIdx.x : (int)blockIdx.x * 2, tb0_[0], trow0_[0]);
  tile_origin(PAIRN ? (int)blockIdx.x : (int)blockIdx.x * 2 + 1, tb0_[1], trow0_[1]);
  const int ga_w = PAIRN ? 0 : grp;
  const int my_tile = PAIRN ? (int)blockIdx.x : (int)blockIdx.x * 2 + grp;
  const int my_cb = PAIRN ? (int)blockIdx.y * 2 + grp : (int)blockIdx.y;
  const int b0 = ga_w ? tb0_[1] : tb0_[0], row0 = ga_w ? trow0_[1] : trow0_[0];
  // exact n / d for 0 <= n < 2048 as (n * m) >> 16 with m = ceil(65536 / d): full-rate 24-bit multiplies
  // instead of the emulated 32-bit division (n (d - 1) < 65536 holds: n <= 1791, d <= 34)
  const unsigned mW = (65536u + (unsigned)g.W - 1u) / (unsigned)g.W;
  const unsigned mWR = (65536u + (unsigned)g.W + 1u) / (unsigned)(g.W + 2);
  const unsigned mPER = (65536u + (unsigned)((g.th + 2) * (g.W + 2)) - 1u) / (unsigned)((g.th + 2) * (g.W + 2));
  const int n0 = my_cb * NBLK;
  const int pc = (MODE == CONV_T2) ? (int)blockIdx.z : 0, py = pc >> 1, px = pc & 1;
  const int HR = g.th + 2, WR = W + 2;
  int rows_valid = H - row0;
  if (rows_valid > g.th) rows_valid = g.th;
  const int nvalid = rows_valid * W;

  int arec[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int p = 64 * seg + 32 * mt + l31p;
    int s, q;
    if (g.spt == 1) {
      s = 0;
      q = p < nvalid ? p : nvalid - 1;
    } else {
      s = seg;
      q = (p & 63) < HW ? (p & 63) : HW - 1;
    }
    const int r = (int)(__umul24((unsigned)q, mW) >> 16), x = q - r * W;
    arec[mt] = (PAIRN ? 0 : grp) * a.halo_px + (s * HR + r) * WR + x;
  }
  int bbase[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int rec = (PAIRN ? grp : 0) * NBLK + nt * 32 + l31p;
    bbase[nt] = rec * RW + swz(rec, hp_);  // NBLK * NG is a multiple of 16: the swap bit does not depend on the tap
  }

  const int bw = (g.spt == 1) ? b0 : b0 + seg;
  const bool sample_ok = bw < a.B;
  const size_t pix0 = (g.spt == 1) ? (size_t)b0 * HW + (size_t)row0 * W : (size_t)bw * HW;
  f32x16 acc[2][NT];
  {
    float add0[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int c = n0 + nt * 32 + l31p;
      float v = a.bias[c];
      if (a.res_mode == 2) v += a.skip_bias[c];
      if (a.temb && sample_ok) v += a.temb[((size_t)(a.temb_per_row ? bw : 0) + (a.step_ptr ? (size_t)*a.step_ptr : 0)) * a.temb_stride + c];
      add0[nt] = v;
    }
    if (a.res_mode == 1) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int pl = hx_acc_pixel(mt, r, hp_);
          const int p = 64 * seg + pl;
          const bool valid = (g.spt == 1) ? (sample_ok && p < nvalid) : (sample_ok && pl < HW);
          const unsigned pix = valid ? (unsigned)pix0 + (unsigned)((g.spt == 1) ? p : pl) : 0u;
          const float* rp = a.res0 + (size_t)(__umul24(pix, (unsigned)a.Cout) + (unsigned)(n0 + l31p));
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mt][nt][r] = rp[nt * 32];
        }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mt][nt][r] += add0[nt];
    } else {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mt][nt][r] = add0[nt];
    }
  }

  // ---- per-item decode, once: source pixel offset, LDS destination, validity bit, scale/shift slot
  const int q4 = tid & 3;
  const int nA = a.halo_px * 4;
  int poff[MAXIT], adst[MAXIT];
  unsigned okmask = 0u, inmask = 0u, smask = 0u;
  {
    const int per = HR * WR;
#pragma unroll
    for (int j = 0; j < MAXIT; ++j) {
      const int it = tid + 512 * j;
      poff[j] = 0, adst[j] = 0;
      if (it < NA * nA) {
        const int ga = (NA == 2 && it >= nA) ? 1 : 0;
        const int ita = it - ga * nA;
        const int tb0 = ga ? tb0_[1] : tb0_[0], trow0 = ga ? trow0_[1] : trow0_[0];
        const int hp = ita >> 2;
        // hp < 448; per = HR * WR >= 81 when spt == 4 (hp (per - 1) < 65536 needs hp <= 448: per <= 146 there)
        const int s = (g.spt == 1) ? 0 : (int)(__umul24((unsigned)hp, mPER) >> 16);
        const int rem = hp - s * per;
        const int hy = (int)(__umul24((unsigned)rem, mWR) >> 16), hx = rem - hy * WR;
        const int b = tb0 + s;
        int y, x;
        bool ok;
        if (MODE == CONV_S1 || MODE == CONV_T2) {
          y = trow0 + hy - 1, x = hx - 1;
          ok = (y >= 0) && (y < H) && (x >= 0) && (x < W);
        } else if (MODE == CONV_S2) {
          const int pi = trow0 + hy - 1, pj = hx - 1;  // phase-plane coordinates; phase (0,0) pixel = (2 pi, 2 pj)
          ok = (pi >= 0) && (pi < H) && (pj >= 0) && (pj < W);
          y = 2 * pi, x = 2 * pj;
        } else {
          const int yu = trow0 + hy - 1, xu = hx - 1;
          ok = (yu >= 0) && (yu < H) && (xu >= 0) && (xu < W);
          y = yu >> 1, x = xu >> 1;
        }
        ok = ok && (b < a.B);
        const int rec = ga * a.halo_px + hp;
        adst[j] = (int)__umul24((unsigned)rec, RW) + swz(rec, q4 >> 1) + (q4 & 1) * 8;
        inmask |= 1u << j;
        if (ok) {
          poff[j] = (int)__umul24(__umul24((unsigned)b, (unsigned)a.Hin) + (unsigned)y, (unsigned)a.Win) + x;  // < 2^24 pixels
          okmask |= 1u << j;
          smask |= (unsigned)(ga * 4 + s) << (3 * j);
        }
      }
    }
  }
  // scale/shift table slot of this thread (tid < NA * spt * 8): sample and channel pair
  int ab_b = -1;
  if (tid < NA * g.spt * 8) {
    const int slot = tid >> 3;
    const int ga = (g.spt == 1) ? slot : (slot >> 2), s = (g.spt == 1) ? 0 : (slot & 3);
    const int tb0 = ga ? tb0_[1] : tb0_[0];
    if (tb0 + s < a.B) ab_b = tb0 + s;
  }
  const int ab_slot = (NA == 2 && g.spt == 1) ? (tid >> 3) * 4 : (tid >> 3);  // table index ga * 4 + s

  const int cin = a.C0 + a.C1;
  const int nch_in = cin / KC;                                   // 16-channel chunks of the input
  const int nch_main = (MODE == CONV_S2) ? 4 * nch_in : nch_in;  // K chunks (x 4 phases for stride 2)
  const int nch_skip = (a.res_mode == 2) ? (a.R0 + a.R1) / KC : 0;
  const int ntot = nch_main + nch_skip;
  const char* wpk3 = reinterpret_cast<const char*>(a.wpk3);
  const char* wskip3 = reinterpret_cast<const char*>(a.wskip3);

  f32x4 ra[MAXIT], rb[NB], rab;
  rab = f32x4{1.f, 0.f, 1.f, 0.f};

  auto issue = [&](int ch) {
    const bool skip = ch >= nch_main;
    const float* src;
    int cs, cc, c;
    int ph = 0;  // CONV_S2: phase of the chunk
    if (!skip) {
      if (MODE == CONV_S2) ph = ch / nch_in;
      c = (ch - ph * nch_in) * KC;
      if (c < a.C0) src = a.in0, cs = a.C0, cc = c;
      else src = a.in1, cs = a.C1, cc = c - a.C0;
    } else {
      c = (ch - nch_main) * KC;
      if (c < a.R0) src = a.res0, cs = a.R0, cc = c;
      else src = a.res1, cs = a.R1, cc = c - a.R0;
    }
    {
      const unsigned pshift = (MODE == CONV_S2) ? (unsigned)((ph >> 1) * a.Win + (ph & 1)) : 0u;  // phase pixel offset
#pragma unroll
      for (int j = 0; j < MAXIT; ++j)
        ra[j] = *(const bx_gf32x4*)(src + (size_t)(__umul24((unsigned)poff[j] + pshift, (unsigned)cs) + (unsigned)(cc + q4 * 4)));
    }
    // packed weights: the chunk's LDS image ([tap][NG groups][NBLK channels] records of 96 B, halves
    // pre-swapped) is contiguous in global memory (launch_pack_conv_bx3 with nb = NBLK * NG)
    int nbit = skip ? NBLK * NG * 6 : NBIG * NG;
    const char* w0 = skip ? wskip3 + ((size_t)(blockIdx.y * nch_skip + (ch - nch_main))) * (NBLK * NG * 96)
                          : wpk3 + ((size_t)((pc * gridDim.y + blockIdx.y) * nch_main + ch) * NTAPS) * (NBLK * NG * 96);
    if (MODE == CONV_S2) {
      // packed [channel block][phase][chunk][taps of the phase][nb]: 0 / 1 / 3 / 5 taps precede phases 0..3
      const int ntp = ((ph >> 1) + 1) * ((ph & 1) + 1), tbefore = (ph == 0) ? 0 : (ph == 1 ? 1 : (ph == 2 ? 3 : 5));
      nbit = ntp * NBLK * NG * 6;
      w0 = wpk3 + ((size_t)blockIdx.y * 9 * nch_in + (size_t)tbefore * nch_in + (size_t)(ch - ph * nch_in) * ntp) * (NBLK * NG * 96);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int it = tid + 512 * j;
      rb[j] = *(const bx_gf32x4*)(w0 + (size_t)(it < nbit ? it : 0) * 16);
    }
    if (!skip && a.ab && !a.gn_stats0) {
      const size_t o = ab_b >= 0 ? ((size_t)ab_b * cin + c + 2 * (tid & 7)) * 2 : 0;
      rab = *(const bx_gf32x4*)(a.ab + o);
    }
  };

  auto commit = [&](int ch) {
    const bool skip = ch >= nch_main;
    const int phc = (MODE == CONV_S2 && !skip) ? ch / nch_in : 0;
    const int chc = (ch - phc * nch_in) * KC;  // first channel of the chunk in the concatenated input
    const bool gnk = a.gn_stats0 != nullptr;
    const bool xform = !skip && (a.ab != nullptr || gnk);
    PROF_T(tc0);
    if (xform && !gnk && tid < NA * g.spt * 8) *reinterpret_cast<f32x4*>(sAB + (ab_slot * 8 + (tid & 7)) * 4) = rab;
    __syncthreads();
    PROF_T(tc1);
    PROF_ADD(3, tc0, tc1);
#pragma unroll
    for (int j = 0; j < MAXIT; ++j) {
      if ((inmask >> j) & 1u) {
        f32x4 v = ra[j];
        const bool okj = (okmask >> j) & 1u;
        if (!okj) v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (xform && okj) {
          const int s = (smask >> (3 * j)) & 7u;
          // scale/shift of the item's 4 channels: this chunk's slice of the block-lifetime table (consumer-side
          // GroupNorm; slot = (s >> 2) * spt + (s & 3)) or the per-chunk sAB copy of the external `ab`
          const float* ep = gnk ? sTab + ((((s >> 2) * g.spt + (s & 3)) * cin + chc + q4 * 4) * 2) : sAB + (s * 16 + q4 * 4) * 2;
          const f32x4 e0 = *reinterpret_cast<const f32x4*>(ep);
          const f32x4 e1 = *reinterpret_cast<const f32x4*>(ep + 4);
          v.x = silu_fast(e0.x * v.x + e0.y);
          v.y = silu_fast(e0.z * v.y + e0.w);
          v.z = silu_fast(e1.x * v.z + e1.y);
          v.w = silu_fast(e1.z * v.w + e1.w);
        }
        unsigned h0, m0, l0, h1, m1, l1;
        split2(v.x, v.y, h0, m0, l0);
        split2(v.z, v.w, h1, m1, l1);
        const u32x2 ph = {h0, h1}, pm = {m0, m1}, pl = {l0, l1};
        char* dst = sA + adst[j];
        *reinterpret_cast<u32x2*>(dst) = ph;
        *reinterpret_cast<u32x2*>(dst + 32) = pm;
        *reinterpret_cast<u32x2*>(dst + 64) = pl;
      }
    }
    PROF_T(tc2);
    PROF_ADD(4, tc1, tc2);
    int nbit = skip ? NBLK * NG * 6 : NBIG * NG;
    if (MODE == CONV_S2) nbit = ((phc >> 1) + 1) * ((phc & 1) + 1) * NBLK * NG * 6;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int it = tid + 512 * j;
      if (it < nbit) *reinterpret_cast<f32x4*>(sB + it * 16) = rb[j];
    }
    __syncthreads();
    PROF_T(tc3);
    PROF_ADD(5, tc2, tc3);
  };

  PROF_T(tp1);
  PROF_ADD(0, tp0, tp1);
  if (a.gn_stats0) {
    // ---- consumer-side GroupNorm: scale/shift of this block's sample(s) from the producers' partial statistics,
    // before chunk 0's prefetch registers come alive (with them the partials would spill).  Wave w owns table row
    // w (= ga * spt + s, the slot of smask), one wave per row (rgfm_device.h: gn_table_row)
    if (wave < NA * g.spt) {
      const int ga = (g.spt == 1) ? wave : (wave >> 2), sl = (g.spt == 1) ? 0 : (wave & 3);
      const int b = (ga ? tb0_[1] : tb0_[0]) + sl;
      gn_table_row(a, GnLane(wave, lane, 0, cin >> 3), b, b < a.B, sTab + (size_t)wave * cin * 2, 1.f);
    }
    // (visible to every wave after the barrier that opens commit(0))
  }
  issue(0);
  commit(0);
  for (int ch = 0; ch < ntot; ++ch) {
    const bool skip = ch >= nch_main;
    PROF_T(ti0);
    if (ch + 1 < ntot) issue(ch + 1);
    PROF_T(ti1);
    PROF_ADD(1, ti0, ti1);
    const int phm = (MODE == CONV_S2) ? ch / nch_in : 0, pa = phm >> 1, pb = phm & 1;
    const int tap_lo = skip ? 4 : 0, tap_hi = skip ? 5 : (MODE == CONV_S2 ? (pa + 1) * (pb + 1) : NTAPS);
#pragma unroll 1
    for (int tap = tap_lo; tap < tap_hi; ++tap) {
      int ky, kx;
      if (MODE == CONV_T2) {
        ky = py + (tap >> 1), kx = px + (tap & 1);
      } else if (MODE == CONV_S2) {
        // halo rows are plane rows r - 1 (ky = 0) and r (ky = 1): phase a = 0 uses r only; a = 1 uses r - 1 then r
        const int ty = pb ? (tap >> 1) : tap, tx = pb ? (tap & 1) : 0;
        ky = pa ? ty : 1, kx = pb ? tx : 1;
      } else {
        ky = tap / 3, kx = tap - 3 * ky;
      }
      const int toff = ky * WR + kx;
      const int boff = (skip ? 0 : tap) * (NBLK * NG * RW);
      bf16x8 af[2][3], bf[NT][3];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int rec = arec[mt] + toff;
        const char* pa = sA + rec * RW + swz(rec, hp_);
#pragma unroll
        for (int p = 0; p < 3; ++p) af[mt][p] = *reinterpret_cast<const bf16x8*>(pa + p * 32);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int p = 0; p < 3; ++p) bf[nt][p] = *reinterpret_cast<const bf16x8*>(sB + bbase[nt] + boff + p * 32);
      constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt][PA[q]], bf[nt][PB[q]], acc[mt][nt], 0, 0, 0);
    }
    PROF_T(tm1);
    PROF_ADD(2, ti1, tm1);
    if (ch + 1 < ntot) commit(ch + 1);
  }
  PROF_T(te0);

  // ---------------------------------------------------------------- epilogue (as conv_mfma_pf_kernel)
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int l31 = lane_e & 31, h = lane_e >> 5;
  // Two instantiations of the same epilogue: FULL (every pixel of this wave's 64-pixel segment is valid -- all
  // waves of all interior tiles) has no per-element predicates, which are a third of its instructions.
  auto epilogue = [&](auto full_tag) {
    constexpr bool FULL = decltype(full_tag)::value;
    unsigned vmask[2] = {0u, 0u};
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pl = hx_acc_pixel(mt, r, h);
        const int p = 64 * seg + pl;
        const bool valid = FULL || ((g.spt == 1) ? (sample_ok && p < nvalid) : (sample_ok && pl < HW));
        if (!FULL && valid) vmask[mt] |= 1u << r;
        unsigned pix = (unsigned)pix0 + (unsigned)((g.spt == 1) ? p : pl);
        if (MODE == CONV_T2) {
          const int pp = (g.spt == 1) ? row0 * W + p : pl;
          const int rr = (int)(__umul24((unsigned)pp, mW) >> 16), xx = pp - rr * W;
          pix = (unsigned)((bw * (2 * H) + 2 * rr + py) * (2 * W) + 2 * xx + px);
        }
        float* op = a.out + (size_t)(__umul24(pix, (unsigned)a.Cout) + (unsigned)(n0 + l31));
        if (valid) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) op[nt * 32] = acc[mt][nt][r];
        }
      }
    // ConvArgs::small_check (set in two-plane mode only): this conv was routed here at create (weights or norm parameters
    // outside the fp16 window) but its output is still staged RAW by a two-plane conv downstream -- the low side of that
    // representation is this producer's to check, whichever kernel it runs on
    if (a.small_check && a.range_flag) {
      float m = 0.f;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (FULL || (vmask[mt] & (1u << r))) m = fmaxf(m, fabsf(acc[mt][nt][r]));
      hx_small_flag(a.range_flag, m);
    }
    if (a.stats_out) {
      int nw;
      if (FULL) {
        nw = 64;
      } else if (g.spt == 1) {
        nw = nvalid - 64 * seg;
        nw = nw < 0 ? 0 : (nw > 64 ? 64 : nw);
        if (!sample_ok) nw = 0;
      } else {
        nw = sample_ok ? HW : 0;
      }
      const int nparts = (MODE == CONV_T2) ? 4 * g.nparts : g.nparts;
      const int part = ((g.spt == 1) ? (my_tile - b0 * g.tps) * 4 + seg : 0) + pc * g.nparts;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float s = 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (FULL || (vmask[mt] & (1u << r))) s += acc[mt][nt][r];
        s += __shfl_xor(s, 32);
        const float mean = nw > 0 ? s / (float)nw : 0.f;
        float m2 = 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (FULL || (vmask[mt] & (1u << r))) {
              const float d = acc[mt][nt][r] - mean;
              m2 += d * d;
            }
        m2 += __shfl_xor(m2, 32);
        if (h == 0 && sample_ok) {
          const int c = n0 + nt * 32 + l31;
          store_stats(a, a.stats_out + (((size_t)bw * nparts + part) * a.Cout + c) * 2, mean, m2);
        }
      }
      if (a.fin_ab && sample_ok) fin_arrive(a, bw, lane_e, nparts, MODE == CONV_T2);
    }
  };
  const bool full_seg = sample_ok && ((g.spt == 1) ? (nvalid - 64 * seg >= 64) : (HW == 64));  // wave-uniform
  if (full_seg) epilogue(std::true_type{});
  else epilogue(std::false_type{});
#ifdef RGFM_BX3_PROF
  PROF_T(te1);
  PROF_ADD(6, te0, te1);
  if (threadIdx.x == 0) {
    for (int i = 0; i < 7; ++i) atomicAdd(&g_bx3_prof[i], (unsigned long long)prof_acc[i]);
    atomicAdd(&g_bx3_prof[7], 1ull);
    atomicAdd(&g_bx3_prof[8], (unsigned long long)(te1 - tp0));
    atomicAdd(&g_bx3_prof[9], (unsigned long long)(wall_clock64() - wall0));
  }
#endif
}

// ---------------------------------------------------------------- weight packing (exact 3-way split)
__device__ __forceinline__ void split1(float v, unsigned short& h, unsigned short& m, unsigned short& l) {
  unsigned ph, pm, pl;
  split2(v, 0.f, ph, pm, pl);
  h = (unsigned short)(ph & 0xffffu), m = (unsigned short)(pm & 0xffffu), l = (unsigned short)(pl & 0xffffu);
}

// [Cout][Cin][taps] fp32 -> [Cout/nb][Cin/16][taps][nb][3][16] bf16, nb = channels of one workgroup
// (conv_block_channels): each [taps][nb] slab is the byte image of the kernel's LDS weight tile
__global__ void pack_conv_bx3_kernel(const float* w, unsigned short* out, int Cout, int Cin, int taps, int nb) {
  const size_t total = (size_t)Cout * Cin * taps;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int kk = i % 16;
    size_t r = i / 16;
    const int n = r % nb;
    r /= nb;
    const int tap = r % taps;
    r /= taps;
    const int nch = Cin / 16;
    const int ch = r % nch;
    const int blk = (int)(r / nch);
    const int co = blk * nb + n, ci = ch * 16 + kk;
    unsigned short h, m, l;
    split1(w[((size_t)co * Cin + ci) * taps + tap], h, m, l);
    // record index inside the chunk's LDS image = tap * nb + n; odd groups of 8 records hold their halves swapped
    const int kq = kk ^ ((((tap * nb + n) >> 3) & 1) << 3);
    unsigned short* rec = out + (i / 16) * 48;
    rec[kq] = h, rec[16 + kq] = m, rec[32 + kq] = l;
  }
}

// ConvTranspose2d [Cin][Cout][4][4] -> [4 parity][Cout/nb][Cin/16][4 taps][nb][3][16] bf16 (see pack_deconv_kernel)
__global__ void pack_deconv_bx3_kernel(const float* w, unsigned short* out, int Cin, int Cout, int nb) {
  const size_t per = (size_t)Cout * Cin * 4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < 4 * per; i += (size_t)gridDim.x * blockDim.x) {
    const int pc = (int)(i / per);
    size_t r = i - (size_t)pc * per;
    const int kk = r % 16;
    r /= 16;
    const int n = r % nb;
    r /= nb;
    const int tap = r % 4;
    r /= 4;
    const int nch = Cin / 16;
    const int ch = r % nch;
    const int blk = (int)(r / nch);
    const int co = blk * nb + n, ci = ch * 16 + kk;
    const int ky = 3 - (pc >> 1) - 2 * (tap >> 1), kx = 3 - (pc & 1) - 2 * (tap & 1);
    unsigned short h, m, l;
    split1(w[(((size_t)ci * Cout + co) * 4 + ky) * 4 + kx], h, m, l);
    const int kq = kk ^ ((((tap * nb + n) >> 3) & 1) << 3);
    unsigned short* rec = out + (i / 16) * 48;
    rec[kq] = h, rec[16 + kq] = m, rec[32 + kq] = l;
  }
}

// stride-2 3x3 conv: [Cout][Cin][3][3] -> [Cout/nb][4 phases][Cin/16][taps of the phase][nb][3][16] bf16.
// Phase (a, b), tap (ty, tx): kernel row = a ? 2 * ty : 1 (plane row r - 1 is input row 2r - 1 = kernel row 0,
// plane row r of phase a = 1 is input row 2r + 1 = kernel row 2; phase a = 0 is input row 2r = kernel row 1).
__global__ void pack_conv_bx3_s2_kernel(const float* w, unsigned short* out, int Cout, int Cin, int nb) {
  const int nch = Cin / 16;
  const size_t total = (size_t)Cout * Cin * 9;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int kk = i % 16;
    size_t r = i / 16;                      // record index
    const size_t per_blk = (size_t)9 * nch * nb;
    const int blk = (int)(r / per_blk);
    size_t q = r - (size_t)blk * per_blk;   // record within the channel block
    int ph = 0, tbefore = 0;
    for (int p = 0; p < 4; ++p) {
      const int ntp = ((p >> 1) + 1) * ((p & 1) + 1);
      if (q < (size_t)ntp * nch * nb) { ph = p; break; }
      q -= (size_t)ntp * nch * nb;
      tbefore += ntp;
    }
    const int pa = ph >> 1, pb = ph & 1, ntp = (pa + 1) * (pb + 1);
    const int ch = (int)(q / ((size_t)ntp * nb));
    const int rem = (int)(q - (size_t)ch * ntp * nb);
    const int tap = rem / nb, n = rem - tap * nb;
    const int ty = pb ? (tap >> 1) : tap, tx = pb ? (tap & 1) : 0;
    const int kyo = pa ? 2 * ty : 1, kxo = pb ? 2 * tx : 1;
    const int co = blk * nb + n, ci = ch * 16 + kk;
    unsigned short h, m, l;
    split1(w[((size_t)co * Cin + ci) * 9 + kyo * 3 + kxo], h, m, l);
    const int kq = kk ^ ((((tap * nb + n) >> 3) & 1) << 3);
    unsigned short* rec = out + r * 48;
    rec[kq] = h, rec[16 + kq] = m, rec[32 + kq] = l;
    (void)tbefore;
  }
}

void launch_pack_conv_bx3(const float* w, void* out, int Cout, int Cin, int taps, hipStream_t s) {
  hipLaunchKernelGGL(pack_conv_bx3_kernel, dim3(256), dim3(256), 0, s, w, (unsigned short*)out, Cout, Cin, taps,
                     conv_block_channels(Cout));
}
void launch_pack_conv_bx3_s2(const float* w, void* out, int Cout, int Cin, hipStream_t s) {
  hipLaunchKernelGGL(pack_conv_bx3_s2_kernel, dim3(256), dim3(256), 0, s, w, (unsigned short*)out, Cout, Cin,
                     conv_block_channels(Cout));
}
void launch_pack_deconv_bx3(const float* w, void* out, int Cin, int Cout, hipStream_t s) {
  hipLaunchKernelGGL(pack_deconv_bx3_kernel, dim3(256), dim3(256), 0, s, w, (unsigned short*)out, Cin, Cout,
                     conv_block_channels(Cout));
}

static bool bx3_pairn(const ConvArgs& a) {
  const int nt = (a.Cout % 64 == 0) ? 2 : 1;
  return a.Cout % (64 * nt) == 0;
}
static size_t bx3w_lds_bytes(const ConvArgs& a, int mode) {
  const int nt = (a.Cout % 64 == 0) ? 2 : 1;
  const int ntaps = (mode == CONV_T2 || mode == CONV_S2) ? 4 : 9;
  const bool pn = bx3_pairn(a);
  size_t bytes = (size_t)((pn ? 1 : 2) * conv_halo_px(a) + ntaps * 32 * nt * (pn ? 2 : 1)) * RW + (256 + 128) * sizeof(float);
  if (a.gn_stats0) bytes += (size_t)(pn ? 1 : 2) * a.g.spt * (a.C0 + a.C1) * 2 * sizeof(float);  // scale/shift table
  return bytes;
}
bool conv_bx3_supported(const ConvArgs& a, int mode) {
  if (!a.wpk3 || a.ep_scale) return false;  // (the BatchNorm+SiLU epilogue of the ratio nets stays on conv_mfma.hip)
  if (a.res_mode == 2 && !a.wskip3) return false;
  // 24-bit pixel indices and 32-bit element offsets inside the kernel (B = 8192 rows of 32x32x256 still fit)
  const size_t px_in = (size_t)a.B * a.Hin * a.Win, px_out = (size_t)a.B * a.g.HW * (mode == CONV_T2 ? 4 : 1);
  const size_t cmax = (size_t)(a.C0 > a.C1 ? a.C0 : a.C1) > (size_t)a.Cout ? (size_t)(a.C0 > a.C1 ? a.C0 : a.C1) : (size_t)a.Cout;
  if (px_in >= (1u << 24) || px_out >= (1u << 24) || (px_in > px_out ? px_in : px_out) * cmax >= (1ull << 32)) return false;
  if (mode == CONV_S2 && g_conv_tuning.s2_f32) return false;  // (RGFM_S2_F32, A/B switch: stride-2 convs on the fp32 kernel)
  if (mode == CONV_S2 && (a.Hin != 2 * a.g.H || a.Win != 2 * a.g.W || a.C1 != 0 || a.res_mode != 0)) return false;
  return conv_halo_px(a) <= 448 && bx3w_lds_bytes(a, mode) <= 160 * 1024;
}

bool conv_bx3_gn_supported(const ConvArgs& a, int mode) {
  const int cin = a.C0 + a.C1;
  if (!a.gn_stats0 || cin < 32 || cin % 8 != 0 || cin > 256) return false;  // <= 4 channels per lane in the prologue
  if (a.gn_nparts0 > 16 || a.gn_g.nparts > 16) return false;  // the prologue holds <= 16 partials per channel
  return conv_bx3_supported(a, mode);                         // (its LDS check includes the table)
}

int conv_fin_expected(const ConvArgs& a, int mode) {
  const int groups = a.Cout / (32 * ((a.Cout % 64 == 0) ? 2 : 1));  // 4-wave groups along the channels
  return (a.g.spt == 1 ? 4 * a.g.tps : 1) * groups * (mode == CONV_T2 ? 4 : 1);
}

// Every instantiation: X(NT, MODE, PAIRN).  conv_bx3_init and launch_conv_bx3 both expand this list.
#define BX3_FOR_ALL(X)                                                                       \
  X(1, CONV_S1, false) X(1, CONV_UP2, false) X(1, CONV_T2, false) X(1, CONV_S2, false) \
  X(2, CONV_S1, false) X(2, CONV_UP2, false) X(2, CONV_T2, false) X(2, CONV_S2, false) \
  X(2, CONV_S1, true) X(2, CONV_UP2, true) X(2, CONV_T2, true) X(2, CONV_S2, true)

int conv_bx3_init() {
  int rc = 0;
#define RAISEW(NTV, M, P) rc |= raise_lds_limit(&conv_mfma_bx3w_kernel<NTV, M, P>, 160 * 1024);
  BX3_FOR_ALL(RAISEW)
#undef RAISEW
  return rc;
}

bool launch_conv_bx3(const ConvArgs& a_in, int mode, hipStream_t s) {
  ConvArgs a = a_in;
  a.halo_px = conv_halo_px(a_in);
  const int nt = (a.Cout % 64 == 0) ? 2 : 1;
  const int tiles = geom_num_tiles(a.g, a.B);
  const bool pn = bx3_pairn(a);  // nt == 2 and Cout % 128 == 0
  dim3 grid(pn ? tiles : (tiles + 1) / 2, pn ? a.Cout / 128 : a.Cout / (32 * nt), mode == CONV_T2 ? 4 : 1);
  const size_t lds = bx3w_lds_bytes(a, mode);
#define LAUNCHW(NTV, M, P) \
  if (nt == (NTV) && mode == (M) && pn == (P)) { hipLaunchKernelGGL((conv_mfma_bx3w_kernel<NTV, M, P>), grid, dim3(512), lds, s, a, tiles); return true; }
  BX3_FOR_ALL(LAUNCHW)
#undef LAUNCHW
  return false;
}
#undef BX3_FOR_ALL

}  // namespace rgfm
