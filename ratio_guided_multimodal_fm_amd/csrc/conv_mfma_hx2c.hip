// conv_mfma_hx2c.hip -- the stride-1 3x3 convs of the 8x8 level on the two-plane fp16 arithmetic, one K iteration and ONE
// barrier per 16-channel chunk.
//
// At 8x8 a 256-pixel tile is four whole samples and a launch has 128 tiles at B = 512: fewer workgroups than CUs, so a
// launch lasts as long as ONE workgroup's serial chain, whatever the batch (conv_mfma_hx2p_kernel: 128 -> 128 takes 41 us at
// 512 rows and 33 us at 32 rows -- 4 us per chunk: three units of barrier + weight wait + three taps each, where the
// chunk's matrix work is 1.45 us).  This kernel is cut for that chain: a workgroup is one tile x 64 channels (two per
// tile at Cout = 128: 256 workgroups), the halo and the weights of a WHOLE chunk are double-buffered in LDS (25 + 37 KB
// each; one workgroup per CU anyway), all nine taps run between two barriers, and while they run the next chunk is
// transformed + stored into the other halo buffer, its weights arrive by LDS-DMA and the chunk after that is fetched
// into registers.  Same arithmetic, LDS record layout, tap and product order as the other hx2 kernels (a fused 1x1 skip
// runs as one-tap chunks behind the main chunks, under its own weight scale, as there).
//
// Scope (conv_hx2c_supported): stride 1, 8x8 rasters (TileGeom::spt == 4), consumer-side GroupNorm on the input
// (ConvArgs::gn_stats0), Cout a multiple of 64, identity residual or fused 1x1 skip or none, optional time term; no
// producer-side finalize, no epilogue activation.  Weights: the packed fp16 images of conv_mfma_hx2p_kernel (a workgroup
// reads one 64-channel block or its half of a 128-channel block).
#include <type_traits>

#include "conv_hx2_common.h"

namespace rgfm {

template <bool SKIP>
__global__ __launch_bounds__(512, 1) void conv_mfma_hx2c_kernel(const ConvArgs a, const int num_tiles) {
  constexpr int W = 8, SPT = 4, WR = W + 2, PREC = WR * WR, HALO = SPT * PREC;
  constexpr int ABYTES = (HALO + 1) * HRW;  // + a pad record (the store target of lanes past the halo)
  constexpr int NTHR = 512, NW = 8, CB = 64;
  constexpr int TAPB = CB * HRW, CHB = 9 * TAPB, PPT = TAPB / 1024;
  constexpr int NIT = (HALO * 4 + NTHR - 1) / NTHR;  // 4
  constexpr int MT_OFF = 4 * WR * HRW;               // pixel p + 32 of a sample: four halo rows down
  // The four 16-byte slots of a halo record are rotated with its halo column so that the 16 lanes of a ds_read_b128 phase
  // (the guide's lane groups) hit 64 distinct banks.  The rotation key (hx >> 2) of the 32-wide rasters leaves the
  // fragment reads of an 8-wide raster two-way conflicted (8 consecutive pixels, then a row stride of 10 records: only
  // two of the four slots in use per bank group); hx >> 1 is conflict-free here (tools/lds_swizzle.py).
  constexpr int SWZ = 1;
  extern __shared__ __attribute__((aligned(16))) char smc[];
  char* const sA = smc;
  char* const sB = smc + 2 * ABYTES;
  float* const sTab = reinterpret_cast<float*>(sB + 2 * CHB);  // [SPT + 1][cin][2]: S_A x (scale, shift) per sample, and a zero row
  const int cin = a.C0 + a.C1;
  char* const sDesc = reinterpret_cast<char*>(sTab) + (SPT + 1) * cin * 8;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = wave >> 2, seg = wave & 3;
  const int l31 = lane & 31, hp = lane >> 5;
  const int tile = blockIdx.x, cb = blockIdx.y;
  const int b0 = tile * SPT;

  // ---- consumer-side GroupNorm: scale/shift of the tile's four samples from the producers' partial statistics
  // (rows side by side on the waves, two waves per row: 8 waves / 4 rows)
  hx_gn_table_rows(a, SPT, 1, b0, sTab, cin);
  hx_tab_zero_row(sTab, SPT, cin, NTHR);

  const int nmain = cin / KC;
  const int nskip = SKIP ? (a.R0 + a.R1) / KC : 0;
  const int ntot = nmain + nskip;
  typedef hx_u32x4 u32x4;
  hx_store_chunk_desc(a, sDesc, nmain, ntot);

  // ---- per-item decode, once: source PIXEL index, LDS destination, table row (the sample inside the tile; SPT: invalid)
  const int q4 = tid & 3;
  unsigned ppix[NIT];
  int adst[NIT], trow[NIT];
#pragma unroll
  for (int j = 0; j < NIT; ++j) {
    const int it = tid + NTHR * j;
    ppix[j] = 0u, trow[j] = SPT, adst[j] = HALO * HRW + (q4 >> 1) * 16 + (q4 & 1) * 8;
    if (it < HALO * 4) {
      const int rec = it >> 2;
      const int s = rec / PREC, rr = rec - s * PREC;
      const int hy = rr / WR, hx = rr - hy * WR;
      const int y = hy - 1, x = hx - 1;
      adst[j] = rec * HRW + ((((q4 >> 1) ^ (hx >> SWZ)) & 3) * 16) + (q4 & 1) * 8;  // plane l: ^ 32
      if (y >= 0 && y < W && x >= 0 && x < W && b0 + s < a.B) {
        trow[j] = s;
        ppix[j] = (unsigned)(((b0 + s) * W + y) * W + x);
      }
    }
  }

  // ---- fragment offsets: this lane's pixel l31 (+ 32: MT_OFF) of sample seg at tap column kx
  int aofs[3];
  {
    const int r = l31 >> 3, x = l31 & 7;
    const int arec = seg * PREC + r * WR + x;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) aofs[kx] = (arec + kx) * HRW + ((hp ^ (((x + kx) >> SWZ) & 3)) & 3) * 16;
  }
  int bofs;
  {
    const int rec = grp * 32 + l31;
    bofs = rec * HRW + ((hp ^ (rec >> 2)) & 3) * 16;
  }

  // ---- weights: [channel block][chunk][tap] slabs; a workgroup of a 128-channel block takes its 64-channel half
  const bool nb128 = (a.Cout & 127) == 0;
  const int TAPS = nb128 ? 2 * TAPB : TAPB;
  const int wblk = nb128 ? cb >> 1 : cb, whalf = nb128 ? (cb & 1) * TAPB : 0;
  const char* const wpk = reinterpret_cast<const char*>(a.wpkh) + (size_t)wblk * nmain * 9 * TAPS + whalf;
  const char* const wsk = reinterpret_cast<const char*>(SKIP ? a.wskiph : a.wpkh) + (size_t)wblk * nskip * TAPS + whalf;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const unsigned sB_lds = (unsigned)(size_t)sB;
  // position c (main chunk c, or skip chunk c - nmain: one tap) -> weight buffer c & 1.  Main: 36 one-KB pieces, five per
  // wave (the surplus ones repeat a piece); skip: four pieces, one per wave of the first four... every wave issues the
  // same count, so the hand-counted wait below holds for all of them.
  constexpr int NPW = 5;
  auto wdma = [&](int c) {
    const bool main = !SKIP || c < nmain;
    const char* src = wpk + (size_t)c * 9 * TAPS;
    if (SKIP && !main) src = wsk + (size_t)(c - nmain) * TAPS;
    const int npc = main ? 9 * PPT : PPT;
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
      const int pq = wave_s + NW * j;
      const int pc = main ? (pq < npc ? pq : pq - npc) : (pq & (PPT - 1));
      const char* gsrc = src + (pc / PPT) * TAPS + (pc % PPT) * 1024 + lane * 16;
      const unsigned dst = sB_lds + (unsigned)((c & 1) * CHB + pc * 1024);
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(gsrc), "s"(dst)
                   : "memory");
    }
  };

  // raw values of the positions in flight: TWO sets -- a position is fetched two iterations before it is stored (one
  // iteration, 2.7 - 3.9 us, does not cover the fetches' round trip: with one set the loop ran at the memory latency,
  // whatever its barrier / unit structure)
  f32x4 ra0[NIT], ra1[NIT];
  float hmax = 0.f;
  auto issue = [&](f32x4 (&ra)[NIT], int c) {
    const u32x4 d = *reinterpret_cast<const u32x4*>(sDesc + c * 16);
    const float* src = reinterpret_cast<const float*>(((unsigned long long)d.y << 32) | (unsigned long long)d.x);
#pragma unroll
    for (int j = 0; j < NIT; ++j) ra[j] = *(const hx_gf32x4*)(src + (size_t)(__umul24(ppix[j], d.z) + (unsigned)(q4 * 4)));
  };
  // GroupNorm + SiLU (main chunks) or the plain scale (skip chunks) + split + store of position c into halo buffer c & 1
  auto commit = [&](const f32x4 (&ra)[NIT], int c) {
    char* base = sA + (c & 1) * ABYTES;
    const bool xf = !SKIP || c < nmain;
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const f32x4 v = ra[j];
      f32x4 o;
      if (xf) {
        const char* ep = reinterpret_cast<const char*>(sTab) + (trow[j] * cin + c * KC + 4 * q4) * 8;
        const f32x4 e0 = *reinterpret_cast<const f32x4*>(ep), e1 = *reinterpret_cast<const f32x4*>(ep + 16);
        o.x = silu_scaled(fmaf(e0.x, v.x, e0.y));
        o.y = silu_scaled(fmaf(e0.z, v.y, e0.w));
        o.z = silu_scaled(fmaf(e1.x, v.z, e1.y));
        o.w = silu_scaled(fmaf(e1.z, v.w, e1.w));
      } else {
        const float sa = trow[j] < SPT ? HX_SA : 0.f;
        o.x = v.x * sa, o.y = v.y * sa, o.z = v.z * sa, o.w = v.w * sa;
      }
      unsigned h0, l0, h1, l1;
      hsplit2(o.x, o.y, h0, l0);
      hsplit2(o.z, o.w, h1, l1);
      hmax = hx_absmax3(o.x, o.y, hmax);
      hmax = hx_absmax3(o.z, o.w, hmax);
      const hx_u32x2 ph = {h0, h1}, pl = {l0, l1};
      *reinterpret_cast<hx_u32x2*>(base + adst[j]) = ph;
      *reinterpret_cast<hx_u32x2*>(base + (adst[j] ^ 32)) = pl;
    }
  };
#define HX2C_VM_WAIT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")

  __syncthreads();  // the scale/shift table and the chunk descriptors are complete

  // ---- pipeline fill: chunk 0 in halo buffer 0 / weight buffer 0, chunk 1 in registers
  issue(ra0, 0);
  wdma(0);
  commit(ra0, 0);
  if (ntot > 1) issue(ra1, 1);
  if (ntot > 2) issue(ra0, 2);

  // ---- accumulators: bias (+ skip bias + time term), scaled by q (they hold q x the true sums); an identity residual
  // enters as fma(res, q, .)
  const float qmain = a.hq[0];
  const int sample = b0 + seg;  // this wave's sample
  const int ch0 = cb * CB + grp * 32 + l31;
  f32x16 acc[2][1];
  hx_acc_init<SKIP>(acc, a, sample, (size_t)(sample < a.B ? sample : 0) * (W * W), ch0, hp, qmain);

  // one tap: 6 fragment reads, 6 MFMAs (a_l w_h, a_h w_l, a_h w_h per tile).  The reads of tap t + 1 are issued BEFORE the
  // MFMAs of tap t (two fragment sets, pinned with sched_barrier): left to itself hipcc emits read x 6, wait, MFMA x 6
  // per tap, and every tap of a wave then waits out an LDS round trip in front of its MFMAs (with two waves per SIMD
  // that was half of a chunk's time: 3.0 us per chunk against 1.45 us of matrix work)
  typedef HxFrag<> Frag;
  auto ldf = [&](Frag& f, const char* sArow, const char* sBt, int o0) { f.load(sArow, o0, MT_OFF, sBt, bofs); };
  auto mma = [&](const Frag& f) { f.mma(acc); };

  // ---- K loop: one barrier per position.  Behind it the next position is transformed + stored (the other halo buffer),
  // its weights requested (the other weight buffer), the position after that fetched, and this position multiplied
  // one iteration; `ra` is the register set of position c + 1 (stored here; refilled with position c + 3)
  auto iteration = [&](f32x4 (&ra)[NIT], int c) {
    // this wave's weight pieces of position c have landed (the NIT fetches of position c + 2 issued behind them stay in
    // flight; those of position c + 1, older, are due now anyway)
    if (c + 2 < ntot) HX2C_VM_WAIT(4);
    else HX2C_VM_WAIT(0);
    static_assert(NIT == 4, "the hand-counted wait above");
    __syncthreads();
    // The two waves of a SIMD (a workgroup's waves w and w + 4: the two channel groups) take the two halves of the
    // iteration in OPPOSITE order -- group 0 stages the next position and then multiplies, group 1 multiplies and then
    // stages -- so that one wave's MFMAs run beside the other's transform + store.  In the same order both staged at once
    // and both multiplied at once: 3.0 us per chunk = 1.45 us of MFMAs + 1.0 us of staging + 0.5 us of DMA issue, summed.
    auto stage_next = [&]() {
      if (c + 1 < ntot) {
        commit(ra, c + 1);
        if (grp == 0) wdma(c + 1);
        if (c + 3 < ntot) issue(ra, c + 3);
      }
    };
    auto multiply = [&]() {
      const char* sAc = sA + (c & 1) * ABYTES;
      const char* sBc = sB + (c & 1) * CHB;
      if (!SKIP || c < nmain) {
        Frag f0, f1;
        // tap t = 3 ky + kx: halo row ky, column offset aofs[kx], weight slab t
#define HX2C_LDF(F, T) ldf(F, sAc + ((T) / 3) * WR * HRW, sBc + (T) * TAPB, aofs[(T) % 3])
#define HX2C_STEP(FN, FC, T)               \
  do {                                     \
      HX2C_LDF(FN, (T) + 1);                 \
      __builtin_amdgcn_sched_barrier(0);     \
      mma(FC);                               \
      __builtin_amdgcn_sched_barrier(0);     \
  } while (0)
        HX2C_LDF(f0, 0);
        HX2C_STEP(f1, f0, 0);
        HX2C_STEP(f0, f1, 1);
        HX2C_STEP(f1, f0, 2);
        HX2C_STEP(f0, f1, 3);
        HX2C_STEP(f1, f0, 4);
        HX2C_STEP(f0, f1, 5);
        HX2C_STEP(f1, f0, 6);
        HX2C_STEP(f0, f1, 7);
        mma(f0);
#undef HX2C_STEP
#undef HX2C_LDF
        if (SKIP && c == nmain - 1) {  // the 1x1 skip weights carry their own scale: q_main -> q_skip
          const float rs = a.hq_skip[0] * a.hq[1];
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) acc[mt][0] = acc[mt][0] * rs;
        }
      } else {
        Frag f;
        ldf(f, sAc + WR * HRW, sBc, aofs[1]);  // (the centre tap)
        mma(f);
      }
    };
    if (grp == 0) {
      stage_next();
      multiply();
    } else {
      if (c + 1 < ntot) wdma(c + 1);  // (requested first: a chunk of MFMAs for it to arrive)
      multiply();
      stage_next();
    }
  };
#pragma unroll 1
  for (int c = 0; c < ntot; c += 2) {
    iteration(ra1, c);
    if (c + 1 < ntot) iteration(ra0, c + 1);
  }
#undef HX2C_VM_WAIT
  if (!(hmax < HX_BIG)) atomicOr(a.range_flag, 1u);  // (rare) plane h would be >= 32768 (or inf)

  // ---- epilogue: a wave's 64 pixels are one whole sample
  {
    const float qinv = SKIP ? a.hq_skip[1] : a.hq[1];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[mt][0] = acc[mt][0] * qinv;
  }
  if (sample >= a.B) return;  // (wave-uniform; no barrier follows)
  if (a.small_check && a.range_flag) hx_small_scan(a.range_flag, acc);  // (ConvArgs::small_check: the output's low range)
  const size_t pix0 = (size_t)sample * (W * W);
  if (a.out) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        a.out[(pix0 + hx_acc_pixel(mt, r, hp)) * a.Cout + ch0] = acc[mt][0][r];
      }
  }
  if (a.stats_out || a.pout) {
    float mean, m2;
    hx_stats64(acc, 0, mean, m2);
    if (a.stats_out && hp == 0) store_stats(a, a.stats_out + ((size_t)sample * a.g.nparts * a.Cout + ch0) * 2, mean, m2);
    if (a.pout) {
      // P format for the norm that consumes this output (ConvArgs::pout): a wave holds a whole sample x 32 channels, i.e.
      // whole GroupNorm groups (Cout / 8 = 8, 16 or 32 channels), so the norm's statistics are finished right here
      float sc, sh;
      hx_group_affine(mean, m2, 64.f, a.Cout >> 3, a.pn_gamma[ch0], a.pn_beta[ch0], sc, sh);
      const unsigned pstride = (unsigned)a.Cout * 4u;
      char* const rec0 = reinterpret_cast<char*>(a.pout) + pix0 * pstride + (size_t)(ch0 >> 4) * 64;
      const float pm = hx_p_emit(acc[0][0], acc[1][0], sc, sh, rec0, pstride, l31, hp);
      if (!(pm < HX_BIG)) atomicOr(a.range_flag, 1u);
    }
  }
}

// ---------------------------------------------------------------- host side
static size_t hx2c_lds_bytes(const ConvArgs& a) {
  const int cin = a.C0 + a.C1, nch = cin / KC + (a.res_mode == 2 ? (a.R0 + a.R1) / KC : 0);
  return (size_t)2 * (4 * 100 + 1) * HRW + (size_t)2 * 9 * 64 * HRW + (size_t)5 * cin * 8 + (size_t)nch * 16;
}

bool conv_hx2c_supported(const ConvArgs& a, int mode) {
  if (!g_conv_tuning.hx2c_on || mode != CONV_S1) return false;
  if (!a.gn_stats0 || a.ab) return false;  // convs of raw inputs stay on conv_mfma_hx2p_kernel
  if (!conv_hx2_supported(a, mode) || !conv_hx2_gn_supported(a, mode)) return false;
  const TileGeom& g = a.g;
  if (g.W != 8 || g.H != 8 || g.spt != 4 || a.Hin != 8 || a.Win != 8) return false;
  if (a.Cout % 64 != 0 || (a.C0 + a.C1) % KC != 0) return false;
  if (a.res_mode == 2 && (a.R0 + a.R1) % KC != 0) return false;
  if (a.res_mode == 1 && a.R0 != a.Cout) return false;
  if (a.ep_scale || a.fin_ab) return false;
  if (a.pout && (a.Cout != 64 && a.Cout != 128 && a.Cout != 256)) return false;  // (whole power-of-two groups per wave)
  if (hx2c_lds_bytes(a) > 160 * 1024) return false;
  // Where it pays (tools/kbench/scripts/q23.sh, q24.sh): 128 -> 128 and 256 -> 128 without a fused skip -3 ... -8 % against
  // conv_mfma_hx2p_kernel at 32 ... 512 rows; with the 1x1 skip (16 one-tap chunks, each behind a whole chunk of staging)
  // +7 %: those stay on hx2p.  ConvTuning::hx2c_all (kbench) lifts the restriction.
  return g_conv_tuning.hx2c_all || a.res_mode != 2;
}

// Every instantiation: X(fused 1x1 skip).  conv_hx2c_init and launch_conv_hx2c both expand this list.
#define HX2C_FOR_ALL(X) X(false) X(true)

int conv_hx2c_init() {
  int rc = 0;
#define RAISEC(SK) rc |= raise_lds_limit(&conv_mfma_hx2c_kernel<SK>, 160 * 1024);
  HX2C_FOR_ALL(RAISEC)
#undef RAISEC
  return rc;
}

bool launch_conv_hx2c(const ConvArgs& a, int mode, hipStream_t s) {
  if (mode != CONV_S1) return false;
  const int tiles = geom_num_tiles(a.g, a.B);
  const dim3 grid(tiles, a.Cout / 64);
  const size_t lds = hx2c_lds_bytes(a);
  const bool skip = a.res_mode == 2;
#define LAUNCHC(SK) \
  if (skip == (SK)) { hipLaunchKernelGGL(conv_mfma_hx2c_kernel<SK>, grid, dim3(512), lds, s, a, tiles); return true; }
  HX2C_FOR_ALL(LAUNCHC)
#undef LAUNCHC
  return false;
}
#undef HX2C_FOR_ALL

}  // namespace rgfm
