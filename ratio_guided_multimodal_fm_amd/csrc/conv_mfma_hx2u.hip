// conv_mfma_hx2u.hip -- the convs of the U-Nets' Upsample (reference src/models/unet_flexible.py:100-108: nearest x 2,
// then Conv2d(ch, ch, 3, padding=1) on the un-normalised residual stream) in their ConvTranspose2d(4, 2, 1) form
// (CONV_T2: four 2x2-tap parity classes over the INPUT raster, rgfm_host.h) on the two-plane fp16 arithmetic
// (conv_hx2_common.h), one K iteration and ONE barrier per 16-channel chunk.
//
// conv_mfma_hx2p_kernel<*, CONV_T2, *> gives every parity class a workgroup of its own (blockIdx.z): the same
// (th + 2) x (W + 2) halo is fetched, split and stored four times, for four taps each.  Here ONE workgroup computes all
// four classes of a 128-pixel input tile (8 rows of a 16-wide raster, or two 8x8 samples) x 64 output channels from one
// staged halo: wave = (parity class, 64-pixel half), i.e. the 64 pixels x 64 channels of ONE class that a wave of the
// general kernel holds, so accumulators, summation order, statistics parts and range checks are that kernel's and the
// results are its results bit for bit.  Per chunk the 10 x 18 (2 x 10 x 10) halo records are split once (the next chunk's
// raw values wait in registers), the 16 (class, tap) weight slabs arrive by LDS-DMA in the other weight buffer, and the 16
// products run between two barriers; halo and weights are double-buffered, and the staging instructions of the next chunk
// sit between the MFMAs of this one.  The input is raw (an Upsample has no norm in front): no scale/shift table, no chunk
// descriptors, no per-lane predicates in the K loop.
//
// A workgroup WALKS tiles (blockIdx.x, + gridDim.x, ...: one workgroup per CU on a full launch, LDS allows no more) as one
// continuous stream of (tile, chunk) positions: the first chunk of the next tile is fetched and staged under the last
// chunk of this one, so only the first tile of a workgroup pays a fetch round trip and the decode.  (Tried on top: a tile's
// output stores leaving from a COPY of its accumulators under the next tile's first chunks -- 256 registers and 100 - 300
// bytes of scratch per lane beside two accumulator sets; not kept.)
//
// Scope (conv_hx2u_supported): mode CONV_T2, raw single-source input, no residual / time term / epilogue activation / P
// output, input rasters of 16x16 or 8x8, Cin % 16 == 0, Cout % 64 == 0.  Weights: the T2 image of
// pack_deconv_planes_kernel ([class][channel block][chunk][tap] slabs; a workgroup reads a 64-channel block or its half of
// a 128-channel block).  Everything else stays on conv_mfma_hx2p_kernel.
#include <type_traits>

#include "conv_hx2_common.h"

namespace rgfm {

template <int WL2>
__global__ __launch_bounds__(512, 1) void conv_mfma_hx2u_kernel(const ConvArgs a, const int num_tiles) {
  constexpr int W = 1 << WL2, H = W, SPT = (W == 16) ? 1 : 2;  // input raster W x W; samples per 128-pixel tile
  static_assert(W == 16 || W == 8, "16x16 or 8x8 input rasters");
  constexpr int TH = 128 / (W * SPT);                      // raster rows of a sample in the tile: 8
  constexpr int WR = W + 2, HR = TH + 2, PREC = HR * WR;   // halo of one sample's rows
  constexpr int NREC = SPT * PREC;                         // 180 / 200 records
  constexpr int ABYTES = (NREC + 1) * HRW;                 // + a pad record (the store target of lanes past the end)
  constexpr int NTHR = 512, NW = 8;
  constexpr int TAPB = 64 * HRW;     // one (class, tap) weight slab of this workgroup's 64 channels
  constexpr int CHB = 16 * TAPB;     // one chunk's weights
  constexpr int NPW = CHB / 1024 / NW;                     // 1-KB DMA pieces per wave and chunk: 8
  constexpr int NIT = (NREC * 4 + NTHR - 1) / NTHR;        // (pixel, 4 channels) items per thread and chunk: 2
  constexpr int MT_OFF = (32 / W) * WR * HRW;              // pixel p + 32 of a wave: 2 (W = 16) or 4 (W = 8) halo rows down
  extern __shared__ __attribute__((aligned(16))) char smu[];
  char* const sA = smu;               // two halo buffers
  char* const sB = smu + 2 * ABYTES;  // two chunk-sized weight buffers

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pc = wave & 3, half = wave >> 2, py = pc >> 1, px = pc & 1;  // this wave's parity class and 64-pixel half
  const int l31 = lane & 31, hp = lane >> 5;
  const int cb = blockIdx.y;
  const int cin = a.C0, nch = cin / KC;
  // this workgroup's tiles: blockIdx.x, + gridDim.x, ... (gridDim.x <= num_tiles: at least one)
  const int njobs = (num_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;

  // ---- per-item decode, once per tile: source offset (floats) of the item's four channels in chunk 0 and validity; the
  // LDS destination does not depend on the tile
  const int q4 = tid & 3;
  unsigned poff[NIT];
  int adst[NIT];
  unsigned okm = 0u;
#pragma unroll
  for (int j = 0; j < NIT; ++j) {
    const int it = tid + NTHR * j;
    adst[j] = NREC * HRW + (q4 >> 1) * 16 + (q4 & 1) * 8;
    if (it < NREC * 4) {
      const int rec = it >> 2, hc = (rec % PREC) % WR;
      // the four 16-byte slots of a record rotate with its halo column >> 1: conflict-free fragment reads on 18- and
      // 10-wide halo rows (conv_mfma_hx2p.hip: swz, tools/lds_swizzle.py)
      adst[j] = rec * HRW + ((((q4 >> 1) ^ (hc >> 1)) & 3) * 16) + (q4 & 1) * 8;  // plane l: ^ 32
    }
  }
  auto decode = [&](int tile) {
    const int b0 = SPT == 1 ? tile >> 1 : tile * 2;   // first sample of the tile
    const int row0 = SPT == 1 ? (tile & 1) * TH : 0;  // its first raster row
    okm = 0u;
    // (an opaque copy of the thread index: what the decode derives from it is worked out per tile, not kept in registers
    // -- or in scratch -- across the K loops)
    int tid_o = tid;
    asm volatile("" : "+v"(tid_o));
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int it = tid_o + NTHR * j;
      poff[j] = 0u;
      if (it < NREC * 4) {
        const int rec = it >> 2;
        const int s = rec / PREC, rr = rec - s * PREC;
        const int hr = rr / WR, hc = rr - hr * WR;
        const int iy = row0 + hr - 1, ix = hc - 1;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W && b0 + s < a.B) {
          okm |= 1u << j;
          poff[j] = (unsigned)(((b0 + s) * H + iy) * W + ix) * (unsigned)cin + (unsigned)((tid_o & 3) * 4);
        }
      }
    }
  };

  // ---- fragment offsets: this lane's pixel 64 half + l31 (+ 32: MT_OFF) of the tile; tap (ty, tx) of class (py, px) reads
  // halo row r + py + ty, column x + px + tx
  int aofs[2];
  {
    const int p = 64 * half + l31;
    const int s = SPT == 1 ? 0 : half, pp = SPT == 1 ? p : l31;  // (8x8: a half is a sample)
    const int r = pp >> WL2, x = pp & (W - 1);
    const int arec = s * PREC + (r + py) * WR + x + px;
#pragma unroll
    for (int tx = 0; tx < 2; ++tx) aofs[tx] = (arec + tx) * HRW + ((hp ^ ((x + px + tx) >> 1)) & 3) * 16;
  }
  int bofs[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int rec = nt * 32 + l31;
    bofs[nt] = rec * HRW + ((hp ^ (rec >> 2)) & 3) * 16;
  }

  // ---- weights: [class][channel block][chunk][tap] slabs; a workgroup of a 128-channel block takes its 64-channel half
  const bool nb128 = (a.Cout & 127) == 0;
  const int TAPS = nb128 ? 2 * TAPB : TAPB;
  const int wblk = nb128 ? cb >> 1 : cb, whalf = nb128 ? (cb & 1) * TAPB : 0;
  const int wblocks = nb128 ? (int)gridDim.y >> 1 : (int)gridDim.y;
  const size_t wclass = (size_t)wblocks * nch * 4 * TAPS;  // bytes of one class's image
  const char* const wpk = reinterpret_cast<const char*>(a.wpkh) + (size_t)wblk * nch * 4 * TAPS + whalf;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const unsigned sB_lds = (unsigned)(size_t)sB;
  // chunk ch -> weight buffer buf: slab 4 class + tap; a wave copies NPW of the chunk's 64 1-KB pieces, this is its j-th
  auto wdma1 = [&](int ch, int buf, int j) {
    const int slab = 2 * j + (wave_s >> 2);
    const char* gsrc = wpk + (size_t)ch * 4 * TAPS + (wave_s & 3) * 1024 + lane * 16 + (size_t)(slab >> 2) * wclass + (slab & 3) * TAPS;
    const unsigned dst = sB_lds + (unsigned)(buf * CHB + slab * TAPB + (wave_s & 3) * 1024);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(dst)
                 : "memory");
  };
  auto wdma = [&](int ch, int buf) {
#pragma unroll
    for (int j = 0; j < NPW; ++j) wdma1(ch, buf, j);
  };

  f32x4 ra[NIT];
  float hmax = 0.f;
  auto issue = [&](int ch) {
#pragma unroll
    for (int j = 0; j < NIT; ++j) ra[j] = *(const hx_gf32x4*)(a.in0 + (size_t)(poff[j] + (unsigned)(ch * KC)));
  };
  auto commit = [&](char* sAc) {  // raw values -> S_A x value in two fp16 planes (zero where the halo leaves the image)
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const float sa = ((okm >> j) & 1u) ? HX_SA : 0.f;
      const f32x4 v = ra[j] * sa;
      unsigned h0, l0, h1, l1;
      hsplit2(v.x, v.y, h0, l0);
      hsplit2(v.z, v.w, h1, l1);
      hmax = hx_absmax3(v.x, v.y, hmax);
      hmax = hx_absmax3(v.z, v.w, hmax);
      const hx_u32x2 ph = {h0, h1}, pl = {l0, l1};
      *reinterpret_cast<hx_u32x2*>(sAc + adst[j]) = ph;
      *reinterpret_cast<hx_u32x2*>(sAc + (adst[j] ^ 32)) = pl;
    }
  };

  const float qmain = a.hq[0], qinv = a.hq[1];
  const int ch0 = cb * 64 + l31;  // this lane's output channel (+ 32 nt)
  const float add0[2] = {a.bias[ch0] * qmain, a.bias[ch0 + 32] * qmain};  // (the accumulators hold q x the true sums)

  // ---- the stream of (tile, chunk) positions; position p uses halo buffer and weight buffer p & 1.  While chunk p is
  // multiplied, the halo of position p + 1 waits in registers and its weights arrive in the other buffer (both requested
  // behind barrier p: every wave is past its reads of position p - 1, the last user of those buffers).
  // One straight-line body per position: the 8 weight pieces of the next position are issued BETWEEN the MFMAs of the first
  // two taps and its halo is split and stored between those of the last two, so a wave's memory instructions issue while
  // its own MFMAs occupy the matrix pipe (issued in a block behind the barrier, by both waves of a SIMD at once, they cost
  // these layers 5 - 12 %: DESIGN.md).  The position behind the last one is staged too (chunk 0 of the last tile again, into
  // the buffers nobody reads): no branch in the body.
  int tile = blockIdx.x, pos = 0;
  decode(tile);
  issue(0);
  wdma(0, 0);
  commit(sA);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  f32x16 acc[2][2];
  // tap T's 12 MFMAs (hx_mma3's order); with DMA: a weight piece of (chunk chn -> buffer bufn) behind each of the first four pairs
  auto mma_dma = [&](const HxFrag<2>& f, auto dma_tag, int chn, int bufn, int j0) {
    constexpr bool DMA = decltype(dma_tag)::value;
    constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[mt][PA[q]], f.b[nt][PB[q]], acc[mt][nt], 0, 0, 0);
        if (DMA && 2 * q + mt < 4) {
          wdma1(chn, bufn, j0 + 2 * q + mt);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
  };
#pragma unroll 1
  for (int k = 0; k < njobs; ++k) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = add0[nt];
#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch, ++pos) {
      const bool last = ch + 1 == nch;
      const int chn = last ? 0 : ch + 1, bufn = (pos + 1) & 1;
      if (last && k + 1 < njobs) decode(tile + (int)gridDim.x);  // the next tile's first chunk
      const char* sAc = sA + (pos & 1) * ABYTES;
      const char* sBc = sB + (pos & 1) * CHB + pc * 4 * TAPB;
      HxFrag<2> f0, f1;  // the class's taps in (ty, tx) order
      f0.load(sAc, aofs[0], MT_OFF, sBc, bofs);
      issue(chn);
      f1.load(sAc, aofs[1], MT_OFF, sBc + TAPB, bofs);
      __builtin_amdgcn_sched_barrier(0);
      mma_dma(f0, std::true_type{}, chn, bufn, 0);
      f0.load(sAc + WR * HRW, aofs[0], MT_OFF, sBc + 2 * TAPB, bofs);
      __builtin_amdgcn_sched_barrier(0);
      mma_dma(f1, std::true_type{}, chn, bufn, 4);
      f1.load(sAc + WR * HRW, aofs[1], MT_OFF, sBc + 3 * TAPB, bofs);
      __builtin_amdgcn_sched_barrier(0);
      mma_dma(f0, std::false_type{}, 0, 0, 0);
      commit(sA + bufn * ABYTES);
      mma_dma(f1, std::false_type{}, 0, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's weight pieces of the next position have landed
      __syncthreads();  // the next position is staged; every wave is past its reads of this one
    }

    // ---- tile end (the next tile's first chunk is already on its way): x 1/q, low-range scan, scatter to (2r + py, 2x + px),
    // statistics -- a wave's 64 pixels are one part of its class; every pixel of a sample that exists is valid
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = acc[mt][nt] * qinv;
    // (an opaque copy of the tile index: the 32 store addresses are worked out here, not kept across the K loop)
    int tile_o = tile;
    asm volatile("" : "+s"(tile_o));
    const int sample = SPT == 1 ? tile_o >> 1 : tile_o * 2 + half;
    if (sample < a.B) {  // (wave-uniform.  8x8: the second half of the last tile of an odd batch is empty)
      if (a.small_check && a.range_flag) hx_small_scan(a.range_flag, acc);  // (ConvArgs::small_check: the output's low range)
      const int pbase = SPT == 1 ? (tile_o & 1) * TH * W + 64 * half : 0;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int pp = pbase + hx_acc_pixel(mt, r, hp);  // pixel of the sample's input raster
          const int rr = pp >> WL2, xx = pp & (W - 1);
          const unsigned pix = (unsigned)((sample * (2 * H) + 2 * rr + py) * (2 * W) + 2 * xx + px);
          float* op = a.out + (size_t)(pix * (unsigned)a.Cout + (unsigned)ch0);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) op[nt * 32] = acc[mt][nt][r];
        }
      if (a.stats_out) {
        constexpr int NP_IN = SPT == 1 ? 4 : 1;  // parts of the input raster (TileGeom::nparts); the output has four classes of them
        const int part = pc * NP_IN + (SPT == 1 ? (tile_o & 1) * 2 + half : 0);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          float mean, m2;
          hx_stats64(acc, nt, mean, m2);
          if (hp == 0) store_stats(a, a.stats_out + (((size_t)sample * (4 * NP_IN) + part) * a.Cout + ch0 + 32 * nt) * 2, mean, m2);
        }
        if (a.fin_ab) fin_arrive(a, sample, lane, 4 * NP_IN, true);
      }
    }
    tile += (int)gridDim.x;
  }
  if (!(hmax < HX_BIG)) atomicOr(a.range_flag, 1u);  // (rare) plane h would be >= 32768 (or inf)
}

// ---------------------------------------------------------------- host side
static size_t hx2u_lds_bytes(const ConvArgs& a) {
  const int nrec = a.g.W == 16 ? 10 * 18 : 2 * 10 * 10;
  return (size_t)2 * (nrec + 1) * HRW + (size_t)2 * 16 * 64 * HRW;
}

bool conv_hx2u_supported(const ConvArgs& a, int mode) {
  if (mode != CONV_T2) return false;
  if (!a.wpkh || !a.hq || !a.range_flag) return false;
  if (a.C1 != 0 || a.ab || a.gn_stats0 || a.in_amax || a.pin0 || a.pout || a.res_mode != 0 || a.temb || a.ep_scale) return false;
  const TileGeom& g = a.g;  // (the INPUT raster)
  if (!((g.W == 16 && g.H == 16 && g.spt == 1 && g.tps == 1) || (g.W == 8 && g.H == 8 && g.spt == 4))) return false;
  if (a.Hin != g.H || a.Win != g.W) return false;
  if (a.C0 % KC != 0 || a.Cout % 64 != 0) return false;
  // 32-bit element offsets inside the kernel
  if ((size_t)a.B * g.HW * a.C0 >= (1ull << 32) || (size_t)a.B * 4 * g.HW * a.Cout >= (1ull << 32)) return false;
  return hx2u_lds_bytes(a) <= 160 * 1024;
}

// Every instantiation: X(log2 of the input raster's width).  conv_hx2u_init and launch_conv_hx2u both expand this list.
#define HX2U_FOR_ALL(X) X(4) X(3)

int conv_hx2u_init() {
  int rc = 0;
#define RAISEU(WL) rc |= raise_lds_limit(&conv_mfma_hx2u_kernel<WL>, 160 * 1024);
  HX2U_FOR_ALL(RAISEU)
#undef RAISEU
  return rc;
}

bool launch_conv_hx2u(const ConvArgs& a, int mode, hipStream_t s) {
  if (mode != CONV_T2) return false;
  const int wl = a.g.W == 16 ? 4 : 3;
  const int tiles = wl == 4 ? 2 * a.B : (a.B + 1) / 2;  // 128 input pixels each
  // One workgroup fills a CU (LDS): at most hx2u_wgs of them (the device's CU count), each walking its share of the tiles.
  // Which workgroup takes a tile changes no bit of it.
  const int groups = a.Cout / 64;
  int gx = (g_conv_tuning.hx2u_wgs_env > 0 ? g_conv_tuning.hx2u_wgs_env : g_conv_tuning.hx2u_wgs) / groups;
  gx = gx < 1 ? 1 : (gx > tiles ? tiles : gx);
  const dim3 grid(gx, groups);
  const size_t lds = hx2u_lds_bytes(a);
#define LAUNCHU(WL) \
  if (wl == (WL)) { hipLaunchKernelGGL((conv_mfma_hx2u_kernel<WL>), grid, dim3(512), lds, s, a, tiles); return true; }
  HX2U_FOR_ALL(LAUNCHU)
#undef LAUNCHU
  return false;
}
#undef HX2U_FOR_ALL

}  // namespace rgfm
