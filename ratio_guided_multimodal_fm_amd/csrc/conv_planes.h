// conv_planes.h -- the split-precision implicit-GEMM convolution, written once for both plane formats: fp32 operands
// carried as 16-bit planes in LDS and multiplied on the 16-bit matrix cores (fp32 accumulate).  conv_mfma_hx2.hip (two
// scaled fp16 planes, three products) and conv_mfma_bx3.hip (three exact bf16 planes, six products) each supply a
// format policy F and instantiate the kernel body, the weight packers and the host helpers below.
//
// A policy owns only how an fp32 value sits in planes:
//   SCALED        the fp16 arithmetic: activations x S_A, weights x s_w (ConvArgs::hq), in_amax pre-scale, running |a'|
//                 maximum -> range-flag bit 0, 1 / q at the end, and the folded BatchNorm epilogue (ep_scale) that only
//                 the fp16 route is given.  !SCALED: none of these (scale 1, fp32 range)
//   NPL, RW       planes; bytes per LDS record = NPL x 16 elements (RW / 16 16-byte items per packed weight record)
//   frag          eight 16-bit elements: one MFMA operand
//   slot(rec, half)    byte offset, inside record rec, of the 16-byte half `half` of plane 0 (the bank swizzle)
//   plane(off, p)      byte offset of plane p's copy of the slot at byte offset off (record base included)
//   load(f[], base, o0)  the NPL fragments of the slot at byte offset o0 behind base
//   wfrag_base(rec, hp), wfrag_sw(rec), wfrag_slot(sw, hp)   a weight fragment's (base, o0), cut into what the tap loop
//                      keeps per channel column and what it forms per read (each format's own cut: the loop's
//                      instruction stream depends on it)
//   split2(a, b, p[])  two floats -> NPL packed pairs
//   mma(acc, af, bf)   the products of one tap for a wave tile of 2 pixel tiles x NT channel tiles
//   wmain(a), wskip(a) the packed weight images of this format in ConvArgs
//   SMALL_EARLY        where the epilogue scans ConvArgs::small_check (see there)
//   PROF, prof()       the format's cycle-counter switch (-DRGFM_HX2_PROF / -DRGFM_BX3_PROF) and its counter array
// Everything else -- tiling, halo decode, stride-2 phase walk, scale/shift paths, chunk loop, epilogue -- is shared.
#pragma once
#include <type_traits>

#include "conv_hx2_common.h"

namespace rgfm {

typedef __attribute__((address_space(1))) f32x4 pl_gf32x4;
typedef unsigned pl_u32x2 __attribute__((ext_vector_type(2)));

#define PL_T(var) const long long var = F::PROF ? clock64() : 0
#define PL_ADD(slot, t0, t1) \
  if constexpr (F::PROF) prof_acc[slot] += (t1) - (t0)

// ------------------------------------------------------------------------------------
// Workgroup = 512 threads = 2 waves per SIMD (one wave alone cannot keep the 16-bit MFMA pipe issuing
// back to back), built as TWO of conv_mfma_pf_kernel's 4-wave tiles sharing one operand in LDS:
//   PAIRN  (Cout % (64 NT) == 0): one 256-pixel tile x two adjacent 32NT-channel groups -- the
//          activation halo (the expensive GroupNorm+SiLU+split staging) is staged once for both;
//   !PAIRN: two consecutive 256-pixel tiles x one channel group -- the weights are staged once.
// LDS records are unpadded; F::slot swizzles their 16-byte slots so that ds_read_b128 is conflict-free for 16
// consecutive records.
// ------------------------------------------------------------------------------------
template <class F, int NT, int MODE, bool PAIRN>
__device__ __forceinline__ void conv_planes_body(const ConvArgs& a, const int num_tiles) {
  // CONV_S2 (3x3, stride 2, pad 1): the input is read as its four pixel-parity phases (a, b) = (row & 1, col & 1),
  // each a plane of the OUTPUT's size; output (r, x) takes phase (a, b) at plane offsets dr in {-1 (a = 1 only), 0},
  // dx likewise, i.e. 1 / 2 / 2 / 4 taps for phases (0,0) / (0,1) / (1,0) / (1,1) -- 9 in all, nothing multiplied by
  // zero.  The K loop runs over (phase, 16-channel chunk); a halo tile is one phase plane, staged like CONV_S1.
  constexpr int NTAPS = (MODE == CONV_T2 || MODE == CONV_S2) ? 4 : 9;  // weight taps resident in LDS
  constexpr int NG = PAIRN ? 2 : 1;            // channel groups per block
  constexpr int NA = PAIRN ? 1 : 2;            // pixel tiles per block
  constexpr int NBLK = 32 * NT;                // channels per group
  constexpr int RW = F::RW, NPL = F::NPL;
  constexpr int WIT = RW / 16;                 // 16-byte items per weight record
  constexpr int NBIG = NTAPS * NBLK * WIT;     // 16-byte weight items per chunk and group
  constexpr int NB = (NBIG * NG + 511) / 512;
  constexpr int MAXIT = (NA * 448 * 4 + 511) / 512;
  extern __shared__ __attribute__((aligned(16))) char smem_planes[];
  long long prof_acc[7] = {0, 0, 0, 0, 0, 0, 0};
  const long long wall0 = F::PROF ? wall_clock64() : 0;
  PL_T(tp0);
  char* sA = smem_planes;
  char* sB = smem_planes + NA * a.halo_px * RW;
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
  int bbase[NT], bsw[NT];  // this lane's records in tap 0's weight tile (F::wfrag_base / _sw / _slot: each format's own split
                           // of the fragment address into a part fixed here and a part formed per tap)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int rec = (PAIRN ? grp : 0) * NBLK + nt * 32 + l31p;
    bbase[nt] = F::wfrag_base(rec, hp_);  // NBLK * NG is a multiple of 16, so the swizzle does not depend on the tap
    bsw[nt] = F::wfrag_sw(rec);
  }

  const int bw = (g.spt == 1) ? b0 : b0 + seg;
  const bool sample_ok = bw < a.B;
  const size_t pix0 = (g.spt == 1) ? (size_t)b0 * HW + (size_t)row0 * W : (size_t)bw * HW;
  // SCALED: the accumulators hold q x the true sums; sa_raw scales a raw input, out_sc undoes in_amax's pre-scale
  float out_sc = 1.f, sa_raw = 1.f, qmain = 1.f;
  if constexpr (F::SCALED) {
    // ConvArgs::in_amax: power-of-two pre-scale of a raw input tensor whose magnitude is far from 1 (the gradients of the
    // ratio estimator's reverse pass): max = f 2^e, f in [0.5, 1) -> the values are staged x 2^-e, the outputs x 2^e
    float in_sc = 1.f;
    if (a.in_amax) {
      const float m = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)*a.in_amax));
      if (m > 0.f && m < 3.0e38f) {
        int e;
        (void)frexpf(m, &e);
        in_sc = ldexpf(1.f, -e), out_sc = ldexpf(1.f, e);
      }
      in_sc = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(in_sc)));
      out_sc = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(out_sc)));
    }
    sa_raw = HX_SA * in_sc;
    qmain = a.hq[0] * in_sc;
  }
  f32x16 acc[2][NT];
  {
    float add0[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int c = n0 + nt * 32 + l31p;
      float v = a.bias[c];
      if (a.res_mode == 2) v += a.skip_bias[c];
      if (a.temb && sample_ok) v += a.temb[((size_t)(a.temb_per_row ? bw : 0) + (a.step_ptr ? (size_t)*a.step_ptr : 0)) * a.temb_stride + c];
      add0[nt] = F::SCALED ? v * qmain : v;
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
          for (int r = 0; r < 16; ++r) acc[mt][nt][r] = F::SCALED ? fmaf(acc[mt][nt][r], qmain, add0[nt]) : acc[mt][nt][r] + add0[nt];
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
        adst[j] = (int)__umul24((unsigned)rec, RW) + F::slot(rec, q4 >> 1) + (q4 & 1) * 8;  // plane 0
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
  const char* wmain = reinterpret_cast<const char*>(F::wmain(a));
  const char* wskip = reinterpret_cast<const char*>(F::wskip(a));

  f32x4 ra[MAXIT], rb[NB], rab;
  float amax = 0.f;  // SCALED: max |a'| this thread has staged (range flag)
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
        ra[j] = *(const pl_gf32x4*)(src + (size_t)(__umul24((unsigned)poff[j] + pshift, (unsigned)cs) + (unsigned)(cc + q4 * 4)));
    }
    // packed weights: the chunk's LDS image ([tap][NG groups][NBLK channels] records of RW bytes, slots already
    // swizzled) is contiguous in global memory (the format's pack_conv_planes_kernel with nb = NBLK * NG)
    int nbit = skip ? NBLK * NG * WIT : NBIG * NG;
    const char* w0 = skip ? wskip + ((size_t)(blockIdx.y * nch_skip + (ch - nch_main))) * (NBLK * NG * RW)
                          : wmain + ((size_t)((pc * gridDim.y + blockIdx.y) * nch_main + ch) * NTAPS) * (NBLK * NG * RW);
    if (MODE == CONV_S2) {
      // packed [channel block][phase][chunk][taps of the phase][nb]: 0 / 1 / 3 / 5 taps precede phases 0..3
      const int ntp = ((ph >> 1) + 1) * ((ph & 1) + 1), tbefore = (ph == 0) ? 0 : (ph == 1 ? 1 : (ph == 2 ? 3 : 5));
      nbit = ntp * NBLK * NG * WIT;
      w0 = wmain + ((size_t)blockIdx.y * 9 * nch_in + (size_t)tbefore * nch_in + (size_t)(ch - ph * nch_in) * ntp) * (NBLK * NG * RW);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int it = tid + 512 * j;
      rb[j] = *(const pl_gf32x4*)(w0 + (size_t)(it < nbit ? it : 0) * 16);
    }
    if (!skip && a.ab && !a.gn_stats0) {
      const size_t o = ab_b >= 0 ? ((size_t)ab_b * cin + c + 2 * (tid & 7)) * 2 : 0;
      rab = *(const pl_gf32x4*)(a.ab + o);
    }
  };

  auto commit = [&](int ch) {
    const bool skip = ch >= nch_main;
    const int phc = (MODE == CONV_S2 && !skip) ? ch / nch_in : 0;
    const int chc = (ch - phc * nch_in) * KC;  // first channel of the chunk in the concatenated input
    const bool gnk = a.gn_stats0 != nullptr;
    const bool xform = !skip && (a.ab != nullptr || gnk);
    PL_T(tc0);
    if (xform && !gnk && tid < NA * g.spt * 8) *reinterpret_cast<f32x4*>(sAB + (ab_slot * 8 + (tid & 7)) * 4) = rab;
    __syncthreads();
    PL_T(tc1);
    PL_ADD(3, tc0, tc1);
    // SCALED: the table path holds S_A x (scale, shift): z' = S_A z, silu' = z' / (1 + exp(-z' / S_A)) = S_A silu(z)
    const float ks = (F::SCALED && !gnk) ? HX_SA : 1.f;
    auto act = [&](float z) {
      if constexpr (F::SCALED) return silu_scaled(ks * z);
      else return silu_fast(z);
    };
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
          v.x = act(e0.x * v.x + e0.y);
          v.y = act(e0.z * v.y + e0.w);
          v.z = act(e1.x * v.z + e1.y);
          v.w = act(e1.z * v.w + e1.w);
        } else if constexpr (F::SCALED) {
          v = v * sa_raw;
        }
        if constexpr (F::SCALED) amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        unsigned p0[NPL], p1[NPL];
        F::split2(v.x, v.y, p0);
        F::split2(v.z, v.w, p1);
#pragma unroll
        for (int p = 0; p < NPL; ++p) *reinterpret_cast<pl_u32x2*>(sA + F::plane(adst[j], p)) = pl_u32x2{p0[p], p1[p]};
      }
    }
    PL_T(tc2);
    PL_ADD(4, tc1, tc2);
    int nbit = skip ? NBLK * NG * WIT : NBIG * NG;
    if (MODE == CONV_S2) nbit = ((phc >> 1) + 1) * ((phc & 1) + 1) * NBLK * NG * WIT;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int it = tid + 512 * j;
      if (it < nbit) *reinterpret_cast<f32x4*>(sB + it * 16) = rb[j];
    }
    __syncthreads();
    PL_T(tc3);
    PL_ADD(5, tc2, tc3);
  };

  PL_T(tp1);
  PL_ADD(0, tp0, tp1);
  if (a.gn_stats0) {
    // ---- consumer-side GroupNorm: scale/shift of this block's sample(s) from the producers' partial statistics,
    // before chunk 0's prefetch registers come alive (with them the partials would spill).  Wave w owns table row
    // w (= ga * spt + s, the slot of smask), one wave per row (rgfm_device.h: gn_table_row)
    if (wave < NA * g.spt) {
      const int ga = (g.spt == 1) ? wave : (wave >> 2), sl = (g.spt == 1) ? 0 : (wave & 3);
      const int b = (ga ? tb0_[1] : tb0_[0]) + sl;
      gn_table_row(a, GnLane(wave, lane, 0, cin >> 3), b, b < a.B, sTab + (size_t)wave * cin * 2, F::SCALED ? HX_SA : 1.f);
    }
    // (visible to every wave after the barrier that opens commit(0))
  }
  issue(0);
  commit(0);
  for (int ch = 0; ch < ntot; ++ch) {
    const bool skip = ch >= nch_main;
    if constexpr (F::SCALED) {
      if (nch_skip && ch == nch_main) {  // the 1x1 skip weights carry their own scale: q_main -> q_skip
        const float rs = a.hq_skip[0] * a.hq[1];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = acc[mt][nt] * rs;
      }
    }
    PL_T(ti0);
    if (ch + 1 < ntot) issue(ch + 1);
    PL_T(ti1);
    PL_ADD(1, ti0, ti1);
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
      typename F::frag af[2][NPL], bf[NT][NPL];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int rec = arec[mt] + toff;
        const char* pa = sA + rec * RW;
        const int o0 = F::slot(rec, hp_);
        F::load(af[mt], pa, o0);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) F::load(bf[nt], sB + bbase[nt] + boff, F::wfrag_slot(bsw[nt], hp_));
      F::template mma<NT>(acc, af, bf);
    }
    PL_T(tm1);
    PL_ADD(2, ti1, tm1);
    if (ch + 1 < ntot) commit(ch + 1);
  }
  PL_T(te0);
  if constexpr (F::SCALED) {
    const float qinv = (nch_skip ? a.hq_skip[1] : a.hq[1]) * out_sc;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = acc[mt][nt] * qinv;
    if (!(amax < HX_LIMIT)) atomicOr(a.range_flag, 1u);  // (rare) an activation left the fp16 range: the host re-runs on bx3
  }

  // ---------------------------------------------------------------- epilogue (as conv_mfma_pf_kernel)
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int l31 = lane_e & 31, h = lane_e >> 5;
  if constexpr (F::SCALED) {
    // folded eval-mode BatchNorm (+ SiLU) of the ratio estimators' encoders, as conv_mfma.hip (once, in front of the two
    // instantiations of the epilogue: conv_mfma_hx2p.hip)
    if (a.ep_scale) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float es = a.ep_scale[n0 + nt * 32 + l31], eh = a.ep_shift[n0 + nt * 32 + l31];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = acc[mt][nt][r] * es + eh;
            acc[mt][nt][r] = a.ep_nosilu ? v : silu_f(v);
          }
      }
    }
  }
  // Two instantiations of the same epilogue: FULL (every pixel of this wave's 64-pixel segment is valid -- all
  // waves of all interior tiles) has no per-element predicates, which are a third of its instructions.
  auto epilogue = [&](auto full_tag) {
    constexpr bool FULL = decltype(full_tag)::value;
    unsigned vmask[2] = {0u, 0u};
    // ConvArgs::small_check: the output's low range, for a two-plane conv downstream that stages this output RAW -- the
    // producer's to check, whichever format it runs on.  SMALL_EARLY (fp16): full segments HERE, while nothing but the
    // accumulators is live (behind the stores and the statistics it costs registers: conv_mfma_hx2q.hip), edge segments
    // masked at the end.  !SMALL_EARLY (bf16): one masked scan between the stores and the statistics -- the early scan
    // costs that kernel 10 to 16 registers in CONV_T2 and 0.1 % of its time at 128 channels
    if (F::SMALL_EARLY && FULL && a.small_check && a.range_flag) hx_small_scan(a.range_flag, acc);
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
    if (!F::SMALL_EARLY && a.small_check && a.range_flag) {
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
    if (F::SMALL_EARLY && !FULL && a.small_check && a.range_flag) {  // (edge tiles: only the valid pixels count)
      float m = 0.f;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (vmask[mt] & (1u << r)) m = fmaxf(m, fabsf(acc[mt][nt][r]));
      hx_small_flag(a.range_flag, m);
    }
  };
  const bool full_seg = sample_ok && ((g.spt == 1) ? (nvalid - 64 * seg >= 64) : (HW == 64));  // wave-uniform
  if (full_seg) epilogue(std::true_type{});
  else epilogue(std::false_type{});
  if constexpr (F::PROF) {  // prologue, issue, mfma, commit-wait, commit-A, commit-B, epilogue, blocks, [8] shader clk, [9] 100 MHz ticks
    PL_T(te1);
    PL_ADD(6, te0, te1);
    if (threadIdx.x == 0) {
      unsigned long long* const gp = F::prof();
      for (int i = 0; i < 7; ++i) atomicAdd(&gp[i], (unsigned long long)prof_acc[i]);
      atomicAdd(&gp[7], 1ull);
      atomicAdd(&gp[8], (unsigned long long)(te1 - tp0));
      atomicAdd(&gp[9], (unsigned long long)(wall_clock64() - wall0));
    }
  }
}
#undef PL_T
#undef PL_ADD

// ---------------------------------------------------------------- weight packing
// One packed record per (tap, output channel) and 16-channel chunk: NPL planes x 16 elements, laid out as the kernel's
// LDS record `rec` = tap * nb + n of the chunk's weight tile (F::slot / F::plane), so a [taps][nb] slab is the byte image
// of that tile.  nb = channels of one workgroup (conv_block_channels).  SCALED: x s_w = hq[2] before the split.
template <class F>
__device__ __forceinline__ void pack_planes_store(unsigned short* rp, int rec, int kk, float v) {
  unsigned p[F::NPL];
  F::split2(v, 0.f, p);
#pragma unroll
  for (int q = 0; q < F::NPL; ++q) rp[(F::plane(F::slot(rec, kk >> 3), q) >> 1) + (kk & 7)] = (unsigned short)(p[q] & 0xffffu);
}

// [Cout][Cin][taps] fp32 -> [Cout/nb][Cin/16][taps][nb][NPL][16]
template <class F>
__global__ void pack_conv_planes_kernel(const float* w, unsigned short* out, const float* hq, int Cout, int Cin, int taps, int nb) {
  const float sw = F::SCALED ? hq[2] : 1.f;
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
    pack_planes_store<F>(out + (i / 16) * (F::RW / 2), tap * nb + n, kk, sw * w[((size_t)co * Cin + ci) * taps + tap]);
  }
}

// ConvTranspose2d [Cin][Cout][4][4] -> [4 parity][Cout/nb][Cin/16][4 taps][nb][NPL][16] (see pack_deconv_kernel)
template <class F>
__global__ void pack_deconv_planes_kernel(const float* w, unsigned short* out, const float* hq, int Cin, int Cout, int nb) {
  const float sw = F::SCALED ? hq[2] : 1.f;
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
    pack_planes_store<F>(out + (i / 16) * (F::RW / 2), tap * nb + n, kk, sw * w[(((size_t)ci * Cout + co) * 4 + ky) * 4 + kx]);
  }
}

// stride-2 3x3 conv: [Cout][Cin][3][3] -> [Cout/nb][4 phases][Cin/16][taps of the phase][nb][NPL][16].
// Phase (a, b), tap (ty, tx): kernel row = a ? 2 * ty : 1 (plane row r - 1 is input row 2r - 1 = kernel row 0,
// plane row r of phase a = 1 is input row 2r + 1 = kernel row 2; phase a = 0 is input row 2r = kernel row 1).
template <class F>
__global__ void pack_conv_planes_s2_kernel(const float* w, unsigned short* out, const float* hq, int Cout, int Cin, int nb) {
  const float sw = F::SCALED ? hq[2] : 1.f;
  const int nch = Cin / 16;
  const size_t total = (size_t)Cout * Cin * 9;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int kk = i % 16;
    size_t r = i / 16;                      // record index
    const size_t per_blk = (size_t)9 * nch * nb;
    const int blk = (int)(r / per_blk);
    size_t q = r - (size_t)blk * per_blk;   // record within the channel block
    int ph = 0;
    for (int p = 0; p < 4; ++p) {
      const int ntp = ((p >> 1) + 1) * ((p & 1) + 1);
      if (q < (size_t)ntp * nch * nb) { ph = p; break; }
      q -= (size_t)ntp * nch * nb;
    }
    const int pa = ph >> 1, pb = ph & 1, ntp = (pa + 1) * (pb + 1);
    const int ch = (int)(q / ((size_t)ntp * nb));
    const int rem = (int)(q - (size_t)ch * ntp * nb);
    const int tap = rem / nb, n = rem - tap * nb;
    const int ty = pb ? (tap >> 1) : tap, tx = pb ? (tap & 1) : 0;
    const int kyo = pa ? 2 * ty : 1, kxo = pb ? 2 * tx : 1;
    const int co = blk * nb + n, ci = ch * 16 + kk;
    pack_planes_store<F>(out + r * (F::RW / 2), tap * nb + n, kk, sw * w[((size_t)co * Cin + ci) * 9 + kyo * 3 + kxo]);
  }
}

// mode: CONV_S1 (also CONV_UP2 and 1x1: plain [taps] order), CONV_S2 (phase-major), CONV_T2 (w is a ConvTranspose2d
// weight [Cin][Cout][4][4]).  hq: the conv's scale record (SCALED) or null.
template <class F>
void launch_pack_planes(const float* w, void* out, const float* hq, int Cout, int Cin, int taps, int mode, hipStream_t s) {
  unsigned short* o = (unsigned short*)out;
  const int nb = conv_block_channels(Cout);
  if (mode == CONV_S2) hipLaunchKernelGGL(pack_conv_planes_s2_kernel<F>, dim3(256), dim3(256), 0, s, w, o, hq, Cout, Cin, nb);
  else if (mode == CONV_T2) hipLaunchKernelGGL(pack_deconv_planes_kernel<F>, dim3(256), dim3(256), 0, s, w, o, hq, Cin, Cout, nb);
  else hipLaunchKernelGGL(pack_conv_planes_kernel<F>, dim3(256), dim3(256), 0, s, w, o, hq, Cout, Cin, taps, nb);
}

// ---------------------------------------------------------------- host side
inline int conv_planes_nt(const ConvArgs& a) { return (a.Cout % 64 == 0) ? 2 : 1; }
inline bool conv_planes_pairn(const ConvArgs& a) { return a.Cout % (64 * conv_planes_nt(a)) == 0; }  // nt == 2 and Cout % 128 == 0

template <class F>
size_t conv_planes_lds_bytes(const ConvArgs& a, int mode) {
  const int nt = conv_planes_nt(a);
  const int ntaps = (mode == CONV_T2 || mode == CONV_S2) ? 4 : 9;
  const bool pn = conv_planes_pairn(a);
  size_t bytes = (size_t)((pn ? 1 : 2) * conv_halo_px(a) + ntaps * 32 * nt * (pn ? 2 : 1)) * F::RW + (256 + 128) * sizeof(float);
  if (a.gn_stats0) bytes += (size_t)(pn ? 1 : 2) * a.g.spt * (a.C0 + a.C1) * 2 * sizeof(float);  // scale/shift table
  return bytes;
}
// what both formats ask of a shape (each format's conv_*_supported adds its own pointers and switches)
template <class F>
bool conv_planes_shape_ok(const ConvArgs& a, int mode) {
  // 24-bit pixel indices and 32-bit element offsets inside the kernel (B = 8192 rows of 32x32x256 still fit)
  const size_t px_in = (size_t)a.B * a.Hin * a.Win, px_out = (size_t)a.B * a.g.HW * (mode == CONV_T2 ? 4 : 1);
  const size_t cmax = (size_t)(a.C0 > a.C1 ? a.C0 : a.C1) > (size_t)a.Cout ? (size_t)(a.C0 > a.C1 ? a.C0 : a.C1) : (size_t)a.Cout;
  if (px_in >= (1u << 24) || px_out >= (1u << 24) || (px_in > px_out ? px_in : px_out) * cmax >= (1ull << 32)) return false;
  if (mode == CONV_S2 && (a.Hin != 2 * a.g.H || a.Win != 2 * a.g.W || a.C1 != 0 || a.res_mode != 0)) return false;
  return conv_halo_px(a) <= 448 && conv_planes_lds_bytes<F>(a, mode) <= 160 * 1024;
}
// the consumer-side GroupNorm prologue (the caller adds conv_*_supported, whose LDS check includes the table)
inline bool conv_planes_gn_ok(const ConvArgs& a) {
  const int cin = a.C0 + a.C1;
  if (!a.gn_stats0 || cin < 32 || cin % 8 != 0 || cin > 256) return false;  // <= 4 channels per lane in the prologue
  return a.gn_nparts0 <= 16 && a.gn_g.nparts <= 16;                         // the prologue holds <= 16 partials per channel
}

// Every instantiation: X(NT, MODE, PAIRN).  conv_planes_init and launch_conv_planes both expand this list.
// K: the format's kernel, as K::get<NT, MODE, PAIRN>().
#define CONV_PLANES_FOR_ALL(X)                                                           \
  X(1, CONV_S1, false) X(1, CONV_UP2, false) X(1, CONV_T2, false) X(1, CONV_S2, false) \
  X(2, CONV_S1, false) X(2, CONV_UP2, false) X(2, CONV_T2, false) X(2, CONV_S2, false) \
  X(2, CONV_S1, true) X(2, CONV_UP2, true) X(2, CONV_T2, true) X(2, CONV_S2, true)

template <class K>
int conv_planes_init() {
  int rc = 0;
#define RAISEW(NTV, M, P) rc |= raise_lds_limit(K::template get<NTV, M, P>(), 160 * 1024);
  CONV_PLANES_FOR_ALL(RAISEW)
#undef RAISEW
  return rc;
}

template <class F, class K>
bool launch_conv_planes(const ConvArgs& a_in, int mode, hipStream_t s) {
  ConvArgs a = a_in;
  a.halo_px = conv_halo_px(a_in);
  const int nt = conv_planes_nt(a);
  const int tiles = geom_num_tiles(a.g, a.B);
  const bool pn = conv_planes_pairn(a);
  dim3 grid(pn ? tiles : (tiles + 1) / 2, pn ? a.Cout / 128 : a.Cout / (32 * nt), mode == CONV_T2 ? 4 : 1);
  const size_t lds = conv_planes_lds_bytes<F>(a, mode);
#define LAUNCHW(NTV, M, P) \
  if (nt == (NTV) && mode == (M) && pn == (P)) { hipLaunchKernelGGL((K::template get<NTV, M, P>()), grid, dim3(512), lds, s, a, tiles); return true; }
  CONV_PLANES_FOR_ALL(LAUNCHW)
#undef LAUNCHW
  return false;
}

}  // namespace rgfm
