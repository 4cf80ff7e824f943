// rgfm_kernels.h -- internal interface between the C-ABI host code (rgfm_host.h, api_*.cpp)
// and the gfx950 kernels.  Not part of the public ABI (that is include/rgfm.h).
//
// HBM data layout (DESIGN.md "Data layout"):
//   * boundary tensors (x_t, v, MC set): NCHW fp32, as the reference passes them;
//   * every internal activation: NHWC fp32  [B][H][W][C]  (channels contiguous:
//     the implicit-GEMM K axis), produced once and consumed in place -- channel
//     concat, nearest-upsample, GroupNorm-apply and SiLU are folded into the
//     consumer's load path, never materialised;
//   * GroupNorm statistics: per (sample, 64-pixel wave segment, channel) partial
//     (mean, M2) pairs written by the producer's epilogue:
//     stats[B][nparts][C][2]; combined (Chan) by gn_finalize into per
//     (sample, channel) scale/shift  ab[B][C][2].
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rgfm.h"  // RGFM_ROUTE_*

namespace rgfm {

constexpr int KC = 16;   // input channels per K-chunk of the MFMA conv
constexpr int LDP = 20;  // LDS row length (floats) of a 16-channel record: 16 + 4 pad,
                         // conflict-free for ds_read_b128 (stride 80 B)

// Output tiling of a [B, H, W] raster into 256-pixel workgroup tiles made of
// four 64-pixel wave segments.
struct TileGeom {
  int H, W, HW;
  int spt;     // samples per tile: 4 when HW <= 64 (one sample per wave segment), else 1
  int th;      // output rows per tile (spt == 1)
  int tps;     // tiles per sample (spt == 1)
  int nparts;  // statistics parts per sample
};

__host__ __device__ inline TileGeom make_geom(int H, int W) {
  TileGeom g;
  g.H = H;
  g.W = W;
  g.HW = H * W;
  if (g.HW <= 64) {
    g.spt = 4;
    g.th = H;
    g.tps = 1;
    g.nparts = 1;
  } else {
    g.spt = 1;
    const int thmax = 256 / W;
    const int nt = (H + thmax - 1) / thmax;
    g.th = (H + nt - 1) / nt;
    g.tps = nt;
    g.nparts = nt * 4;
  }
  return g;
}

__host__ __device__ inline int geom_num_tiles(const TileGeom& g, int B) {
  return g.spt == 1 ? B * g.tps : (B + g.spt - 1) / g.spt;
}

// valid pixels of statistics part `part` of a sample
__host__ __device__ inline int geom_part_count(const TileGeom& g, int part) {
  if (g.spt != 1) return g.HW;
  const int tile = part >> 2, w = part & 3;
  int rows = g.H - tile * g.th;
  if (rows > g.th) rows = g.th;
  int n = rows * g.W - 64 * w;
  return n < 0 ? 0 : (n > 64 ? 64 : n);
}

// CONV_T2: ConvTranspose2d(k=4, s=2, p=1) as four 2x2-tap parity-class convs over the INPUT raster
// (ConvArgs::g describes that raster; the output is [B][2H][2W][Cout]); weights from launch_pack_deconv.
enum ConvMode { CONV_S1 = 0, CONV_S2 = 1, CONV_UP2 = 2, CONV_T2 = 3 };

struct ConvArgs {
  // input: up to two NHWC sources concatenated along C (torch.cat([h, skip], 1))
  const float* in0;
  const float* in1;
  int C0, C1;        // channels of in0 / in1 (C1 = 0: single source)
  int Hin, Win;      // spatial size of the sources
  const float* ab;   // [B][C0+C1][2] GroupNorm scale/shift (then SiLU) applied on load; null = raw
  // Consumer-side GroupNorm (conv_mfma_bx3.hip): instead of `ab`, the partial statistics of the input map(s)
  // themselves -- every workgroup derives the scale/shift of its own sample(s) in its prologue, so no finalize
  // launch (or producer-side finalize) sits between two convs.
  const float* gn_stats0;  // [B][gn_nparts0][C0][2] statistics of in0 (null: use `ab`)
  const float* gn_stats1;  // [B][gn_g.nparts][C1][2] statistics of in1 or null
  const float* gn_gamma;   // [C0 + C1]
  const float* gn_beta;
  int gn_nparts0;          // parts of in0: gn_g.nparts, or 4 x that when in0 was written by a CONV_T2 launch
  TileGeom gn_g;           // tiling of the raster the parts refer to (part sizes)
  // conv_mfma_hx2d.hip: the input ALREADY normalised, activated and split ("P format": [pixel][C0/16][h ch 0-7 | h ch
  // 8-15 | l ch 0-7 | l ch 8-15] fp16, 64 B per (pixel, 16-channel chunk), written by the producing conv's epilogue or
  // by launch_hx_presplit) -- staged by LDS-DMA only; `zeros` = 64 zero bytes on the device (the padding records' source)
  // raw inputs far from unit scale (the gradients of the reverse pass, 1e-3 ... 1e-6): when set, *in_amax holds the bits
  // of max |input| over the tensor (its producer's launch_grad_act wrote them) and the kernel stages 2^-e x the values
  // (max = f 2^e, f in [0.5, 1)) and multiplies its outputs by 2^e -- the two-plane representation then keeps its 22 bits
  // below the tensor's maximum.  conv_mfma_hx2_kernel (launch_conv_hx2), raw inputs without residual / skip only.
  const unsigned* in_amax;
  const void* pin0;
  const void* zeros;
  // ... and the producing side: when set, the epilogue ALSO (out != null) or ONLY (out == null) writes the output in P
  // format for the ONE norm that consumes it (8 groups over Cout channels, parameters pn_gamma / pn_beta [Cout]):
  // kernels whose workgroups own whole (sample, group) sets (rgfm_host.h: p_producer_ok)
  void* pout;
  const float* pn_gamma;
  const float* pn_beta;
  const float* wpk;  // packed 3x3 weights  [Cout/(32NT)][Cin/16][9][32NT][16]
  const void* wpk3;  // the same weights as three bf16 planes [..][9][32NT][3][16] (conv_mfma_bx3.hip) or null
  const void* wskip3;
  // conv_mfma_hx2.hip: the same weights as two scaled fp16 planes [..][9][32NT][2][16] + their scale record
  // hq = {q = S_A s_w, 1 / q, s_w, eligible} (launch_pack_conv_hx2), and the device word the kernel ORs 1 into
  // when a staged activation leaves the fp16 range (the host then repeats the call on the split-bf16 kernel)
  const void* wpkh;
  const void* wskiph;
  const void* wpkh9;  // stride-2 convs: the weights once more as the plain nine-tap image (conv_mfma_hx2s.hip), or null
  const float* hq;
  const float* hq_skip;
  unsigned* range_flag;
  // 1: a later conv stages this output RAW (no GroupNorm: the fused 1x1 skip, Downsample, Upsample -- reference
  // unet_flexible.py:85,96,107-108), i.e. as S_A x value in two fp16 planes.  The epilogue then checks the low side of
  // that representation: a wave block (64 pixels x its channels) whose largest |value| is below HX_SMALL (and not 0)
  // ORs 2 into *range_flag, and the caller repeats the call on the split-bf16 kernels (fp32 exponent range).
  int small_check;
  const float* bias; // [Cout]
  const float* temb; // time-embedding add: temb[(per_row ? b : 0) * temb_stride + c]; null = none
  int temb_stride;
  int temb_per_row;
  const int* step_ptr;  // optional device word: the row of the time table is *step_ptr (+ b when temb_per_row): lets
                        // one captured launch sequence (hipGraph) serve every Euler step
  // residual: res_mode 0 none; 1 identity (res0 NHWC [.., Cout]); 2 fused 1x1 conv over cat(res0, res1)
  int res_mode;
  const float* res0;
  const float* res1;
  int R0, R1;
  const float* wskip;      // packed 1x1 weights [Cout/(32NT)][(R0+R1)/16][1][32NT][16]
  const float* skip_bias;  // [Cout]
  // epilogue activation (ratio-net BatchNorm folded to scale/shift, then SiLU); null = none
  const float* ep_scale;
  const float* ep_shift;
  int ep_nosilu;     // 1: store ep_scale * acc + ep_shift itself (the gradient path keeps the pre-activation)
  float* out;        // NHWC [B][H][W][Cout]
  float* stats_out;  // [B][nparts][Cout][2] or null
  // Producer-side GroupNorm finalize (rgfm_device.h: fin_arrive): when fin_ab is set, the LAST wave to deliver
  // statistics of a sample (arrival counter) computes the scale/shift of the norm that consumes this
  // output -- cat(this output, fin_stats1's tensor) -- instead of a separate gn_finalize launch.
  float* fin_ab;             // [B][Cout + fin_C1][2] or null
  unsigned* fin_counter;     // [B], zero between launches (the finishing wave resets its entry)
  int fin_expected;          // arrivals per sample
  const float* fin_stats1;   // partner statistics [B][nparts][fin_C1][2] (same spatial size as the output) or null
  int fin_C1;
  const float* fin_gamma;    // [Cout + fin_C1]
  const float* fin_beta;
  // Winograd F(2x2, 3x3) image of the same 3x3 weights (conv_mfma_hx2w.hip: launch_pack_conv_hx2w) and its scale record, or null
  const void* wpkw;
  const float* hqw;
  int B, Cout;
  TileGeom g;        // OUTPUT raster tiling
  int halo_px;       // pixels of the staged input tile
};

// ---- host-side helpers shared by the conv kernels' launch code
// pixels of the staged input tile of the split-plane kernels (they set ConvArgs::halo_px to it): (th + 2) x (W + 2)
// plane pixels per sample of the tile in every mode (the fp32 kernel's own halo differs for stride 2)
inline int conv_halo_px(const ConvArgs& a) { return a.g.spt * (a.g.th + 2) * (a.g.W + 2); }
// output channels per block of the packed split-plane weight images (bf16x3 and two-plane fp16 alike) = channels one
// workgroup covers: 128 when Cout % 128 == 0 (two 64-channel groups), else 64 or 32
inline int conv_block_channels(int Cout) { return Cout % 128 == 0 ? 128 : (Cout % 64 == 0 ? 64 : 32); }
// ConvArgs::fin_expected: waves that arrive per sample in the producer-side finalize (rgfm_device.h: fin_arrive), the
// same for every conv_mfma* kernel -- one per 64-pixel segment and 4-wave channel group (and CONV_T2 parity class)
inline int conv_fin_expected(const ConvArgs& a, int mode) {
  const int groups = a.Cout / (32 * ((a.Cout % 64 == 0) ? 2 : 1));  // 4-wave groups along the channels
  return (a.g.spt == 1 ? 4 * a.g.tps : 1) * groups * (mode == CONV_T2 ? 4 : 1);
}
// raises a kernel's dynamic-LDS limit (the default is 64 KB); returns the hipError_t as an int, 0 = success
template <class Kernel>
inline int raise_lds_limit(Kernel* kernel, int bytes) {
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

struct ConvInArgs {  // first conv of a net: NCHW image -> NHWC features
  const float* x;    // [B][CIN][H][W]
  const float* w;    // [C0][CIN][3][3] (reference layout)
  const float* bias;
  const float* ep_scale;  // optional BatchNorm scale/shift + SiLU epilogue (ratio nets)
  const float* ep_shift;
  int ep_nosilu;          // 1: no SiLU (see ConvArgs::ep_nosilu)
  float* out;        // NHWC [B][H][W][C0]
  float* stats_out;  // or null
  int B, C0;
  TileGeom g;
  unsigned* range_flag;  // with small_check (see ConvArgs::small_check): the first conv's output feeds raw consumers too
  int small_check;
};

struct ConvOutArgs {  // out_conv(silu(out_norm(h))) -> NCHW velocity, optional fused Euler
  const float* in;    // NHWC [B][H][W][Cin]
  const float* ab;    // [B][Cin][2]
  const float* w;     // [Cin/16][9][CIMG][16] (launch_pack_conv_out)
  const float* bias;
  float* v_out;       // NCHW velocity or null
  float* x_state;     // NCHW state for the fused Euler update or null
  const float* x_base;  // x_state = x_base + v dt (out of place: a midpoint stage); null: x_state += v dt
  float dt;
  int B, Cin;
  TileGeom g;
  int halo_px;
};

struct GnFinalizeArgs {
  const float* stats0;  // [B][nparts][C0][2]
  const float* stats1;  // [B][nparts][C1][2] or null
  int C0, C1, groups;
  const float* gamma;   // [C0+C1]
  const float* beta;
  float* ab;            // [B][C0+C1][2]
  int B;
  TileGeom g;
  int rep;              // 0/1: stats0 has g.nparts parts; 4: output of a CONV_T2 launch (4 x g.nparts parts of a 4*HW-pixel map)
  float* mr;            // optional [B][groups][2]: (mean, rstd) of every group (the norm's backward: launch_gn_bwd)
};

struct TimeLinear {  // one ResBlock time_mlp Linear: rows [out_off, out_off+cout) of the table
  int w_off, b_off, cout, out_off;
};

struct TimeEmbedArgs {
  const float* params;     // state_dict-order blob (device copy)
  const float* freqs;      // [mc/2]
  int mc, temb;
  int te0w, te0b, te2w, te2b;  // offsets into params
  const TimeLinear* lin;   // device array
  int nlin;
  int total;               // table row length
  // time values: either explicit t_dev[nt] or step index based: t = (float)((step_begin + i) * (1.0/num_steps))
  const float* t_dev;
  int num_steps, step_begin;
  float* table;            // [nt][total]
  float* emb_out;          // optional [nt][mc]: the sinusoidal embedding itself (parity hook)
  // class-conditional nets (time_embed_labels_kernel); label_emb null: an unlabelled net, nothing below is read
  const float* label_emb;  // [num_classes + 1][temb]; row num_classes is the null label
  const int* labels;       // optional [nt]: the class of each row (outside 0..num_classes: the null label)
  int num_classes;
  int ncls;                // rows per time value: 1, or num_classes + 1 (row i: time i / ncls, class i % ncls without labels)
  int t_shared;            // 1: every row reads t_dev[0]
};

// ---- the conv kernels (conv_mfma*.hip), one group per kernel.  Each file lists its instantiations ONCE (*_FOR_ALL):
// conv_*_init() expands the list to raise every instantiation's dynamic-LDS limit (0 = success), launch_conv_*() to launch
// the one whose key matches (ConvArgs, mode, ConvTuning) -- false, and no launch, when none does.  conv_*_supported() is
// the kernel's line of the predicate chain conv_route (the fp32 kernel takes everything).

// Process-wide tuning of the conv kernels' host side: with Modes (rgfm_host.h), everything that can change which kernel
// -- or which cut of one -- a launch takes.  The library writes hx2p_half (ensure_init: per device, the last one wins)
// and the four environment fields (refresh_modes: once per API call); the rest keep their defaults unless tools/kbench
// sets them.  Not thread_local: whoever sets a field sets it for every thread that launches.  Every cut of a kernel
// gives the same bits, so none of these changes a result.
struct ConvTuning {
  int hx2p_half = 256;     // conv_mfma_hx2p.hip: launches with fewer workgroups than this are cut finer -- 64-channel halves,
                           // four-wave workgroups (0: never).  The device's CU count, or RGFM_HX2P_HALF=n (A/B of the threshold)
  int hx2p_w4 = 0;         // kbench: 1 = four-wave workgroups forced where Cout % 128 != 0, 2 = wherever two fit on a CU
  int hx2q_min = 1024;     // conv_mfma_hx2q.hip: launches with fewer (tile, channel block) pairs stay on hx2p (0: never runs) -- at
                           // two workgroups per CU the stream needs >= 2 tiles per workgroup to pay (kbench: B = 128 rows lose)
  int hx2q_target = 512;   // workgroups a launch is cut into when it has the tiles: two per CU (> 0)
  int hx2q_tpw = 0;        // kbench: force the tiles per workgroup (0: hx2q_tiles_per_wg)
  int hx2q_cut = 0;        // kbench: force the workgroup cut, 10 NG + NT (0: hx2q_cut)
  int hx2q_all = 0;        // kbench: 1 = every supported shape, not only those where it is the faster kernel
  int hx2s_on = 1;         // conv_mfma_hx2s.hip: 0 = never (Modes::s2 is the per-call switch)
  int hx2u_wgs = 256;      // conv_mfma_hx2u.hip: workgroups a launch is cut into at most, each walking its share of the tiles: the
                           // device's CU count (one workgroup fills a CU)
  int hx2u_wgs_env = 0;    // RGFM_HX2U_WGS=n: that number instead (> 0; A/B of the tile walk, and how a test reaches it with few rows)
  int hx2c_on = 1;         // conv_mfma_hx2c.hip: 0 = never (Modes::c8 is the per-call switch)
  int hx2c_all = 0;        // kbench: 1 = every supported shape, also the fused-skip layers where hx2p is faster
  int hx2d_cut = 3;        // conv_mfma_hx2d.hip: 0 off, 1 the eight-wave kernel everywhere, 2 the four-wave kernel everywhere,
                           // 3 by layer shape.  RGFM_HX2D=1|2 (A/B; RGFM_HX2D=0 is Modes::pfmt)
  int wino_w32 = 0;        // RGFM_WINO_W32=1: with RGFM_WINO=1, the Winograd form for the 32x32 layers only (A/B)
  bool s2_f32 = false;     // RGFM_S2_F32 set: stride-2 convs off conv_mfma_bx3.hip, i.e. on the fp32 kernel (A/B)
  bool f32_simple = false; // RGFM_CONV_SIMPLE set: conv_mfma.hip's non-prefetching kernel wherever it exists (debug)
};
inline ConvTuning g_conv_tuning;

// conv_mfma.hip: exact fp32 MFMA, every shape
int conv_mfma_init();
bool launch_conv_mfma(const ConvArgs& a, int mode, hipStream_t s);
size_t conv_mfma_lds_bytes(const ConvArgs& a);

// conv_mfma_bx3.hip: fp32 conv with operands split into three bf16 planes, on the bf16 matrix cores
bool conv_bx3_supported(const ConvArgs& a, int mode);
bool conv_bx3_gn_supported(const ConvArgs& a, int mode);  // a.gn_* filled: can the kernel take the norm itself?
int conv_bx3_init();
bool launch_conv_bx3(const ConvArgs& a, int mode, hipStream_t s);
void launch_pack_conv_bx3(const float* w, void* out, int Cout, int Cin, int taps, hipStream_t s);
void launch_pack_deconv_bx3(const float* w, void* out, int Cin, int Cout, hipStream_t s);
void launch_pack_conv_bx3_s2(const float* w, void* out, int Cout, int Cin, hipStream_t s);  // weights of a stride-2 3x3 conv

// conv_mfma_hx2.hip: fp32 conv with operands split into two scaled fp16 planes, on the f16 matrix cores
bool conv_hx2_supported(const ConvArgs& a, int mode);
bool conv_hx2_gn_supported(const ConvArgs& a, int mode);
int conv_hx2_init();
bool launch_conv_hx2(const ConvArgs& a, int mode, hipStream_t s);
// packs w (mode CONV_S1: [Cout][Cin][taps]; CONV_S2: the phase-major stride-2 order; CONV_T2: a ConvTranspose2d
// weight [Cin][Cout][4][4], taps ignored) and writes the scale record hq[4] (device)
void launch_pack_conv_hx2(const float* w, void* out, float* hq, int Cout, int Cin, int taps, int mode, hipStream_t s);
// w [Cout][Cin][3][3] of "nearest-upsample x 2, then 3x3 conv" -> the ConvTranspose2d(4, 2, 1) weight K [Cin][Cout][4][4] of
// the same linear map: K[ky][kx] = sum of w[i][j] over i in A(ky), j in A(kx), A = {2}, {1, 2}, {0, 1}, {0} (unet_kernels.hip)
void launch_up2_as_deconv(const float* w, float* k, int Cout, int Cin, hipStream_t s);

// conv_mfma_hx2p.hip: producer / consumer pipelined version for CONV_S1 / CONV_UP2 / CONV_T2; same arguments
bool conv_hx2p_supported(const ConvArgs& a, int mode);
int conv_hx2p_init();
bool launch_conv_hx2p(const ConvArgs& a, int mode, hipStream_t s);

// conv_mfma_hx2q.hip: four-waves-per-SIMD version (one tile x 64 channels at a time, two workgroups per CU, several
// tiles per workgroup behind one continuous staging stream) for full stride-1 launches over 16- / 32-pixel-wide
// rasters with Cout % 64 == 0 and a consumer-side input norm; bit-identical results
bool conv_hx2q_supported(const ConvArgs& a, int mode);
int conv_hx2q_init();
bool launch_conv_hx2q(const ConvArgs& a, int mode, hipStream_t s);

// conv_mfma_hx2s.hip: the Downsample convs (stride 2, raw input) with a chunk's four parity planes staged together
bool conv_hx2s_supported(const ConvArgs& a, int mode);
int conv_hx2s_init();
bool launch_conv_hx2s(const ConvArgs& a, int mode, hipStream_t s);

// conv_mfma_hx2u.hip: the Upsample convs (CONV_T2 over a 16x16 / 8x8 raster, raw input) with one staged halo for all four
// parity classes -- a cut of route RGFM_ROUTE_HX2P (launch_conv, rgfm_host.h), not a route of its own; bit-identical results
bool conv_hx2u_supported(const ConvArgs& a, int mode);
int conv_hx2u_init();
bool launch_conv_hx2u(const ConvArgs& a, int mode, hipStream_t s);

// conv_mfma_hx2c.hip: the stride-1 convs of the 8x8 level, one barrier per chunk (cut for the workgroup's serial chain)
bool conv_hx2c_supported(const ConvArgs& a, int mode);
int conv_hx2c_init();
bool launch_conv_hx2c(const ConvArgs& a, int mode, hipStream_t s);

// conv_mfma_hx2d.hip: stride-1 convs of the 16x16 / 8x8 levels over a P-format input (ConvArgs::pin0), staged by LDS-DMA only
bool conv_hx2d_supported(const ConvArgs& a, int mode);
int conv_hx2d_init();
bool launch_conv_hx2d(const ConvArgs& a, int mode, hipStream_t s);
// P format of silu(scale x + shift) from an fp32 NHWC map and per-(sample, channel) pairs ab[B][C][2]
void launch_hx_presplit(const float* in, const float* ab, void* pout, int B, int HW, int C, hipStream_t s);

// conv_mfma_hx2w.hip: Winograd F(2x2, 3x3) form of the stride-1 3x3 conv on the two-plane arithmetic; its own packed weights
bool conv_hx2w_supported(const ConvArgs& a, int mode);
int conv_hx2w_init();
bool launch_conv_hx2w(const ConvArgs& a, int mode, hipStream_t s);
void hx2_scale_launch(const float* w, size_t n, float* hq, hipStream_t s);
void launch_pack_conv_hx2w(const float* w, void* out, float* hq, float* tmp, int Cout, int Cin, hipStream_t s);

// The conv kernels by route (RGFM_ROUTE_* of include/rgfm.h, whose names these are: _lib.ROUTES spells them the same).
// ensure_init loops over it, launch_conv_on indexes it; WHICH route a launch takes is conv_route's chain (rgfm_host.h).
struct ConvKernel {
  const char* name;
  int (*init)();
  bool (*launch)(const ConvArgs& a, int mode, hipStream_t s);
};
inline constexpr ConvKernel CONV_KERNELS[RGFM_ROUTE_COUNT] = {
    {"hx2d", conv_hx2d_init, launch_conv_hx2d},  // RGFM_ROUTE_HX2D
    {"hx2w", conv_hx2w_init, launch_conv_hx2w},  // RGFM_ROUTE_HX2W
    {"hx2s", conv_hx2s_init, launch_conv_hx2s},  // RGFM_ROUTE_HX2S
    {"hx2c", conv_hx2c_init, launch_conv_hx2c},  // RGFM_ROUTE_HX2C
    {"hx2q", conv_hx2q_init, launch_conv_hx2q},  // RGFM_ROUTE_HX2Q
    {"hx2p", conv_hx2p_init, launch_conv_hx2p},  // RGFM_ROUTE_HX2P
    {"hx2", conv_hx2_init, launch_conv_hx2},     // RGFM_ROUTE_HX2
    {"bx3", conv_bx3_init, launch_conv_bx3},     // RGFM_ROUTE_BX3
    {"f32", conv_mfma_init, launch_conv_mfma},   // RGFM_ROUTE_F32
};
static_assert(RGFM_ROUTE_HX2D == 0 && RGFM_ROUTE_HX2W == 1 && RGFM_ROUTE_HX2S == 2 && RGFM_ROUTE_HX2C == 3 && RGFM_ROUTE_HX2Q == 4 &&
                  RGFM_ROUTE_HX2P == 5 && RGFM_ROUTE_HX2 == 6 && RGFM_ROUTE_BX3 == 7 && RGFM_ROUTE_F32 == 8,
              "CONV_KERNELS is written in RGFM_ROUTE_* order");

void launch_conv_in(const ConvInArgs& a, int cin, hipStream_t s);
void launch_conv_out(const ConvOutArgs& a, int cimg, hipStream_t s);
void launch_pack_conv_out(const float* w, float* out, int cimg, int Cin, hipStream_t s);
void launch_gn_finalize(const GnFinalizeArgs& a, hipStream_t s);
void launch_time_embed(const TimeEmbedArgs& a, int nt, hipStream_t s);
void launch_pack_conv(const float* w, float* out, int Cout, int Cin, int taps, int nt32, hipStream_t s);
// ConvTranspose2d weight [Cin][Cout][4][4] -> [4 parity][Cout/(32 nt32)][Cin/16][4 taps][32 nt32][16]
void launch_pack_deconv(const float* w, float* out, int Cin, int Cout, int nt32, hipStream_t s);
// out[o][p*C + c] = w[o][c*P + p]  (Linear consuming an NCHW-flattened map, re-indexed for NHWC)
void launch_permute_cols(const float* w, float* out, int rows, int C, int P, hipStream_t s);
// out[(p*C + c)][k] = w[(c*P + p)][k], bias likewise  (Linear producing an NCHW-flattened map)
void launch_permute_rows(const float* w, const float* b, float* wout, float* bout, int C, int P, int K, hipStream_t s);
// SinusoidalPositionEmbeddings (flow_matching.py:17-31) into out[b*stride + col0 + 0..dim)
void launch_fm_time_embed(const float* t_dev, int t_count, int num_steps, int step, const float* freqs, float* out,
                          int B, int dim, int stride, int col0, hipStream_t s);
void launch_nhwc_to_nchw(const float* in, float* out, int B, int C, int HW, hipStream_t s);
// ORs 2 into *flag when a (sample, 32-channel) block of the NHWC map is non-zero but below HX_SMALL (see ConvArgs::small_check)
void launch_range_low_check(const float* in, int B, int HW, int C, unsigned* flag, hipStream_t s);

// ---- ratio-estimator helpers
void launch_pool2(const float* in, const float* ab, float* out, int B, int H, int W, int C, hipStream_t s);
void launch_avgpool(const float* in, const float* ab, float* out, int B, int HW, int C, hipStream_t s);
void launch_linear_mfma(const float* x, const float* w, const float* b, float* y, int rows, int in,
                        int out, int x_stride, int y_stride, hipStream_t s);
// split-K variant with GroupNorm-apply + SiLU on the x load (x is an NHWC map flattened per row,
// ab[row][k % C][2]); `part` holds splits x rows x out floats
void launch_linear_mfma_splitk(const float* x, const float* ab, int C, const float* w, const float* b, float* y,
                               float* part, int splits, int rows, int in, int out, int y_stride, hipStream_t s);
void launch_layernorm_silu(float* x, const float* w, const float* b, int rows, int n, hipStream_t s);
// Cross evaluation, first hidden layer: out[r - row0][n] = silu(LayerNorm(ux[r / ny] + uy[r % ny] + bias)) for the `rows`
// pair indices r = row0 .. row0 + rows - 1 of the row-major [nx][ny] matrix (n % 4 == 0, n <= 1024)
void launch_cross_ln_silu(const float* ux, const float* uy, const float* bias, const float* w, const float* b, float* out,
                          long long row0, int rows, int ny, int n, hipStream_t s);
// One-sided gradient, first hidden layer for matched rows: u[r] = ctx[r] + ut[r] (stored: layernorm_silu_bwd reads it) and
// a[r] = silu(LayerNorm(u[r])) in one pass (n % 4 == 0, n <= 1024); ctx, ut, u, a are [rows][n], u and a distinct from the inputs
void launch_cond_ln_silu(const float* ctx, const float* ut, const float* w, const float* b, float* u, float* a, int rows, int n,
                         hipStream_t s);
void launch_ratio_head(const float* x, const float* w, const float* b, float* out, int rows, int n,
                       int loss, int what, hipStream_t s);
void launch_bn_fold(const float* w, const float* b, const float* rm, const float* rv, float* scale,
                    float* shift, int C, hipStream_t s);

// ---- gradient of log r (ratio_grad.hip)
// [Co][Ci][9] -> [Ci][Co][9] with the taps flipped: the weights of the conv that maps dL/d(out) to dL/d(in)
void launch_conv_weight_transpose(const float* w, float* wt, int Co, int Ci, hipStream_t s);
void launch_transpose2d(const float* w, float* wt, int rows, int cols, hipStream_t s);  // [rows][cols] -> [cols][rows]
void launch_fill(float* p, float v, size_t n, hipStream_t s);
void launch_fill_ab_identity(float* ab, size_t n_pairs, hipStream_t s);  // (scale, shift) = (1, 0)
// gz[b,y,x,c] = route * silu'(z) * scale[c].  mode 0: g has z's shape; 1: g is the 2x2-max-pooled map's gradient
// (routed to the first maximum of silu(z) in each window); 2: g is [B][C], the gradient of the global average of
// silu(z); 3: g is [B][C], the gradient of the global average of the 2x2-max-pooled map (modes 2 then 1 in one)
// amax (optional): device word that receives (atomic max) the bits of the largest |gz| -- zero it before the launch
void launch_grad_act(const float* g, const float* z, const float* scale, float* gz, int B, int S, int C, int mode, hipStream_t s,
                     unsigned* amax = nullptr);
// the GroupNorm encoders (RatioEstimator, 28x28): activation backward with per-sample scale/shift pairs, then the norm's own
void launch_grad_act_gn(const float* g, const float* z, const float* ab, float* gu, int B, int S, int C, int mode, hipStream_t s);
void launch_gn_bwd(float* gu, const float* z, const float* gamma, const float* mr, int B, int HW, int C, int groups, hipStream_t s);
// first conv of an encoder, input gradient as an NCHW image: gimg[b,c,y,x] = sum_co,k w[co,c,k] gz[b, y-ky+1, x-kx+1, co]
void launch_conv_bwd_img(const float* gz, const float* w, float* gimg, int B, int S, int Co, int cimg, hipStream_t s);
// y = silu(LayerNorm(u)): gu from gy (wave per row); u is the Linear output kept by the forward
void launch_layernorm_silu_bwd(const float* u, const float* gy, const float* w, const float* b, float* gu, int rows, int n, hipStream_t s);
// gh[row][k] = d log_ratio / d score (score[row]) * w[k]; log_ratio (optional) [rows]
void launch_ratio_head_bwd(const float* score, const float* w, float* gh, float* log_ratio, int rows, int n, int loss, hipStream_t s);
// x <- base + (v + gamma g) dt; base null: x <- x + (v + gamma g) dt
void launch_euler_grad(float* x, const float* v, const float* g, size_t n, float gamma, float dt, hipStream_t s,
                       const float* base = nullptr);
// ... with a strength per row: element i takes (float)((double)gamma_rows[i / dim] * scale) as its gamma (n = rows x dim)
void launch_euler_grad_rows(float* x, const float* v, const float* g, size_t n, int dim, const float* gamma_rows, double scale,
                            float dt, hipStream_t s, const float* base = nullptr);

// ---- guidance / Euler
struct GuidanceArgs {
  const float* x;  // [B][dx]
  const float* y;  // [B][dy]
  float* vx;       // in: model velocity, out: blended velocity (when x_state null)
  float* vy;
  const float* mc_x1;
  const float* mc_y1;
  const float* mc_ratios;
  int ratio_stride;  // row b reads mc_ratios[b * ratio_stride + i]: 0 = one vector shared by every row (the paired block), N = a ratio row per sample (the one-sided block)
  int B, N, dx, dy;  // dy = 0 (with nsy = 0; y, vy, mc_y1 unused): a block with one modality
  float tf, s2, cden, g1, g2;
  double* dist;        // [nsx + nsy][B][N] scratch: sliced squared distances (guid_logp -> guid_apply)
  int slice_len, nsx, nsy;  // D-slices per modality (<= RGFM_GUID_SLICES in all)
  // optional (hipGraph replay): the step's scalars {tf, s2, cden, -} come from sched[4 * *step_ptr] instead of the fields
  const float* sched;
  const int* step_ptr;
  float* weights_out;  // optional [B][N]
  float* wbuf;         // [B][N] importance weights of the step (scratch: behind the distance slices)
  float* wsum;         // [B] their row sums (scratch: behind wbuf)
  // cross pairing (all N x N pairs of the MC set; mc_ratios is then the matrix R [N][N], x index first; ratio_stride
  // unused): wbuf / wsum hold the x marginal weights, wbuf_y / wsum_y the y ones, which guid_apply's y column blocks read.
  // Null wbuf_y: one weight row for both modalities.
  float* wbuf_y;
  float* wsum_y;
  float* weights_out_y;  // optional [B][N] (weights_out: the x marginals)
  float *ca, *cb, *cu, *cs, *cq;  // scratch [B][N] each: a, b, u = R b, s = R^T a, q = (R o R) b^2 (read with diag_rec only)
  float* diag_rec;     // optional [B][RGFM_DIAG_FLOATS] diagnostics records: guid_weights writes each row's Z_bar into its slot
  float* x_state;      // optional fused Euler: x_state += dt * blended
  float* y_state;
  // optional: x_state = x_base + dt * blended, with x still the point the guidance is evaluated at (the second stage of
  // a midpoint step evaluates at the mid state and moves the step's start state); null: the base is x
  const float* x_base;
  const float* y_base;
  float dt;
  // optional per-row strength (include/rgfm.h, "Guidance strength per sample and per stage"): row b blends with
  // gamma = (double)gamma_rows[b] * gamma_scale, g1 = (float)(1 - gamma), g2 = (float)gamma -- the host's rule for the
  // scalar fields, per row; null: g1 / g2 above for every row
  const float* gamma_rows;
  double gamma_scale;
  // optional effective-sample-size floor (include/rgfm.h, "Effective-sample-size floor"; read by guid_weights_ess_kernel
  // alone): ess_min >= 1 as fp32, and the row's exponent tau goes to tau_out[b] when that is not null
  float ess_min;
  float* tau_out;
};
constexpr int RGFM_GUID_SLICES = 8;
void launch_guid_logp(const GuidanceArgs& a, hipStream_t s);   // distances -> GuidanceArgs::dist
void launch_guid_weights(const GuidanceArgs& a, hipStream_t s);  // distances + ratios -> importance weights (GuidanceArgs::wbuf, wsum)
// ... held to the floor GuidanceArgs::ess_min (a sibling kernel: twice the LDS, [4][N] log-weights beside the [4][N] weights)
void launch_guid_weights_ess(const GuidanceArgs& a, hipStream_t s);
void launch_guid_cross_weights(const GuidanceArgs& a, hipStream_t s);  // cross pairing: distances + R -> marginal weights (wbuf, wbuf_y and their sums; the diagnostics' weight entries)
void launch_guid_apply(const GuidanceArgs& a, hipStream_t s);  // guided velocity (the [B,N] x [N,D] GEMM), blend (+ Euler)
int guid_apply_init();                                         // (once per process: the GEMM kernel's LDS size)
void launch_euler(float* x, const float* v, size_t n, float dt, hipStream_t s);
void launch_step_inc(int* step, hipStream_t s);  // *step += 1
// the stochastic step's pre-update (sde.hip): base = a x + sigma xi over n floats, xi the Gaussian noise of `key`
// (sde_key, sampler_host.h); launch_sde_noise writes xi alone
void launch_sde_pre(const float* x, float* base, size_t n, uint64_t key, float a, float sigma, hipStream_t s);
void launch_sde_noise(float* out, size_t n, uint64_t key, hipStream_t s);
void launch_guid_schedule(float* sched, int step_begin, int ns, int num_steps, hipStream_t s);  // [ns][4] = {tf, s2, cden, 0}
// class conditioning and classifier-free guidance (cfg.hip); a label outside 0..K reads as K on every path
// rows[b][:] = table[stage][label_b][:], table [stages][K + 1][total] (total % 4 == 0): the per-row time table of a stage
void launch_cfg_gather(const float* table, const int* labels, int K, int stage, int B, int total, float* rows, hipStream_t s);
// out = base + (vu + w (vc - vu)) dts over n floats (out may be base)
void launch_cfg_blend(const float* base, const float* vc, const float* vu, float w, float dts, size_t n, float* out, hipStream_t s);
// training: emb[b][:] += E[label_b][:] (labels null: every row K), saved[b] = the label as used
void launch_cfg_label_add(float* emb, const float* E, const int* labels, int K, int B, int temb, int* saved, hipStream_t s);
// training: dE[c][:] = sum over rows b with saved[b] == c of g[b][:], in ascending b (one workgroup per class, no atomics)
void launch_cfg_label_grad(const float* g, const int* saved, int K, int B, int temb, float* dE, hipStream_t s);
// diagnostics (opt-in; rec: [B][RGFM_DIAG_FLOATS] records, include/rgfm.h)
void launch_diag_wstats(const float* w, int B, int N, float* rec, hipStream_t s);  // ess, w_max, w_min of the rows of w [B][N]
void launch_diag_rownorm(const float* v, int B, int D, float* rec, int slot, hipStream_t s);  // rec[b][slot] = |v[b]|_2, v [B][D], D % 4 == 0

// ---- training pass of the U-Net (unet_grad.hip; all tensors NCHW fp32)
// One conv for ug_igemm_kernel.  op 0: out = conv(x) + bias (+ temb[b][co]) (+ res), op 1: data gradient of the conv's
// input (conv-input raster Hc x Wc) from dy, routed by channel to out ([B][C0]) / out1 ([B][Cin - C0]), each added to
// (acc0 / acc1) or overwritten; op 2: weight gradient partials part[split][Cout][Cin * taps] from dy and x.
// The conv input raster is Hc x Wc; with `up` it is the nearest-x2 image of the Hs x Ws source, else Hs = Hc.
struct UgConv {
  const float* x;   // input [B][Cin][Hs][Ws]
  const float* w;   // [Cout][Cin][taps]; taps 1, 9 (3x3, pad 1) or 16 (4x4, pad 1)
  const float* dy;  // output gradient [B][Cout][Ho][Wo]
  const float* bias;  // op 0: [Cout] or null
  const float* temb;  // [B][Cout] or null
  const float* res;   // [B][Cout][Ho][Wo] or null (may alias out)
  float* out;
  float* out1;
  float* part;
  int C0, acc0, acc1;
  int B, Cin, Cout, taps, stride, up;
  int Hs, Ws, Hc, Wc, Ho, Wo;
  int splits, kps;  // op 2: K split into `splits` ranges of kps (multiple of 16); else splits = 1, kps = K
  const float* dbias;  // op 1: added per row m of the result (a transposed conv's bias), or null
};
// out = cat(s0, s1) [B][C0 + C1][HW]; with mr: silu(gamma (v - mean) rstd + beta) per group, then (drop_hdr set and
// its p > 0) dropout with the keep decisions of ResBlock `block`
struct UgAct {
  const float* s0;
  const float* s1;
  int C0, C1, B, HW, groups;
  const float* mr;  // [B][groups][2] (mean, rstd) or null
  const float* gamma;
  const float* beta;
  const unsigned* drop_hdr;  // {p_drop bits, seed lo, seed hi} on the device, or null
  int block;
  float* out;
};
void launch_ug_conv(const UgConv& c, int op, hipStream_t s);
void launch_ug_reduce(const float* part, int splits, size_t n, float* out, hipStream_t s);
void launch_ug_bias_grad(const float* dy, int B, int C, int HW, float* db, hipStream_t s);
void launch_ug_gn_stats(const float* s0, const float* s1, int C0, int C1, int B, int HW, int groups, float* mr,
                        hipStream_t s);
void launch_ug_gn_act(const UgAct& a, hipStream_t s);
void launch_ug_gn_act_bwd(const UgAct& a, const float* dout, float* d0, float* d1, int acc0, int acc1, float* pg,
                          float* pb, hipStream_t s);
void launch_ug_colsum(const float* in, int rows, int cols, float* out, hipStream_t s);
void launch_ug_rowsum(const float* in, int rows, int n, float* out, hipStream_t s);
void launch_ug_linear(const float* x, const float* w, const float* b, float* y, int rows, int in, int out, int silu_in,
                      hipStream_t s);
void launch_ug_linear_wgrad(const float* dy, const float* x, int rows, int in, int out, int silu_in, float* dw,
                            float* db, hipStream_t s);
void launch_ug_linear_dgrad(const float* dy, const float* w, int rows, int in, int out, float* dx, int acc,
                            hipStream_t s);
void launch_ug_dsilu(float* g, const float* x, int n, hipStream_t s);
void launch_ug_sincos(const float* t, int t_count, const float* freqs, int B, int mc, float* emb, hipStream_t s);
void launch_ug_pool2_add(const float* du, float* dx, int BC, int H, int W, hipStream_t s);
void launch_ug_split_add(const float* src, float* d0, float* d1, int B, int C0, int C1, int HW, hipStream_t s);
void launch_ug_mask(float* out, size_t n, uint64_t seed, int block, float p, hipStream_t s);
void launch_ug_header(unsigned* hdr, float p, uint64_t seed, hipStream_t s);

// ---- likelihood path of the U-Net (unet_logp.hip; fixed-order reductions, one workgroup per row)
// acc[b] = (accumulate ? acc[b] : 0) + scale <a[b, :], g[b, :]>, rows of d floats
void launch_ul_rowdot(const float* a, const float* g, int B, int d, float scale, int accumulate, float* acc,
                      hipStream_t s);
void launch_ul_step(const float* src, const float* k, float c, size_t n, float* dst, hipStream_t s);  // dst = src - c k
// stage times of the reverse loop in the order it takes them: Euler tt[j] = (N - j) / N, midpoint also tt[2j + 1] = t_hi - dt / 2
void launch_ul_times(float* tt, int num_steps, int midpoint, hipStream_t s);
void launch_ul_gauss_logp(const float* z, const float* A, int B, int d, float* logp, hipStream_t s);  // log N(z_b; 0, I) - A[b]

// ---- the tail of a training conv block (block_train.hip; NCHW fp32): norm, activation, optional 2x2 max-pool
// A conv output z [B][C][H][W] in front of an activation, with a norm in between when mr, its (mean, rstd) pairs, is set:
// y = gamma (z - mean) rstd + beta -- groups == 0: one pair per channel (BatchNorm), mr[C][2]; groups > 0: GroupNorm,
// mr[B][groups][2] -- else y = z.
struct BtBlock {
  const float* z;
  const float* mr;  // or null
  const float* gamma;
  const float* beta;
  int B, C, H, W, groups;
};
enum BtActKind { BT_SILU, BT_RELU };  // the ratio estimators' encoders / the classifiers
constexpr int BT_BN_SLICES = 16;  // batch slices of a per-channel BatchNorm reduction (partials per channel)
// part: [C][BT_BN_SLICES][3] floats; stats (optional): [C][2] = (batch mean, unbiased batch variance)
void launch_bt_bn_stats(const float* z, int B, int C, int HW, float* part, float* mr, float* stats, hipStream_t s);
void launch_bt_bn_running(const float* rm, const float* rv, int C, float* mr, hipStream_t s);
// out = act(y); with `choice` its 2x2 max-pool (floor division of odd rasters) and the window element taken per output
void launch_bt_act(BtActKind act, const BtBlock& a, float* out, unsigned char* choice, hipStream_t s);
// full (the conv's raster) = g (pooled raster) at the chosen element -- where `gate`, the pooled activation, is > 0 when
// there is one -- else 0
void launch_bt_unpool(BtActKind act, const float* g, const unsigned char* choice, const float* gate, float* full, int BC,
                      int H, int W, hipStream_t s);
void launch_bt_choice(const unsigned char* choice, size_t n, float* out, hipStream_t s);  // out = (float)choice
// BatchNorm: dout (gradient of act(y) on the full raster; `saved` = the stored act(y) where the activation's gradient needs
// it, null for SiLU and when dout is the gradient of y already) is replaced by dz; part: [C][BT_BN_SLICES][2], m12: [C][2];
// training: a device word, non-zero = batch statistics (their dependence on z is differentiated), zero = constants
void launch_bt_bn_bwd(BtActKind act, const BtBlock& a, float* dout, const float* saved, const unsigned* training, float* part,
                      float* m12, float* dgamma, float* dbeta, hipStream_t s);

// ---- training pass of the ratio estimators (ratio_train.hip; NCHW fp32): what block_train.hip does not cover
void launch_rt_avgpool(const float* in, int rows, int n, float* out, hipStream_t s);
void launch_rt_avgpool_bwd(const float* g, int rows, int n, float* din, hipStream_t s);
void launch_rt_ln_act(const float* u, const float* gamma, const float* beta, int rows, int width, const unsigned* hdr,
                      int block, float* mr, float* out, hipStream_t s);
void launch_rt_ln_act_bwd(const float* u, const float* g, const float* gamma, const float* beta, int rows, int width,
                          const unsigned* hdr, int block, const float* mr, float* du, float* pg, float* pb,
                          hipStream_t s);

// ---- training pass of FlowMatchingModel (fmnet_grad.hip): the wide Linears as fp32-MFMA GEMMs
// C[m][n] = bias[n] + sum_k A(m, k) B(n, k).  An operand is ROW-major (element (r, k) at p[r * ld + k]) or K-major
// (p[k * ld + r]): which one is the launch's a_kmajor / b_kmajor.  splits > 1: workgroup z covers k in
// [z kps, (z + 1) kps) and writes part[z][M][N]; launch_fg_gemm then adds the slices in split order (+ bias).
struct FgGemm {
  const float* a;
  const float* b;
  const float* bias;  // [N] or null
  float* c;           // [M][ldc]
  float* part;        // [splits][M][N] (splits > 1)
  int M, N, K, lda, ldb, ldc;
  int splits, kps;    // kps: a multiple of 16 (splits == 1: kps >= K)
  int veca, vecb;     // a row-major operand may be read 16 bytes at a time (set by launch_fg_gemm)
};
void launch_fg_gemm(FgGemm g, bool a_kmajor, bool b_kmajor, hipStream_t s);

// ---- training pass of the evaluation classifiers (clf_train.hip; NCHW fp32): what block_train.hip does not cover
constexpr int CT_MAX_CLASSES = 32;
void launch_ct_gate(float* g, const float* act, size_t n, hipStream_t s);          // in place: g where act > 0, else 0
void launch_ct_gate_out(const float* act, size_t n, float* out, hipStream_t s);    // out = act > 0 ? 1 : 0
// out = drop(relu(u)) / in place g <- drop(g) where u > 0: Dropout layer 0 of the header hdr (launch_ug_header)
void launch_ct_relu_drop(const float* u, size_t n, const unsigned* hdr, float* out, hipStream_t s);
void launch_ct_relu_drop_bwd(const float* u, float* g, size_t n, const unsigned* hdr, hipStream_t s);
// rows of logits[n][classes <= CT_MAX_CLASSES]: loss[n] (fp64), optional dlogits = (softmax - onehot) scale, optional pred
void launch_ct_xent(const float* logits, const int* labels, int n, int classes, float scale, double* loss,
                    float* dlogits, int* pred, hipStream_t s);

// ---- optimizer step (optim.hip): gradient norm, clip, Adam / AdamW, weight EMA over a table of rgfm_adam_entry
constexpr int ADAM_CHUNK = 1024;     // floats of the flat state range per chunk (a quad per lane of a 256-thread workgroup)
constexpr int ADAM_PARTIALS = 1024;  // float64 partial sums of g^2: the norm launch's grid cap; the step sums all of them
constexpr int ADAM_MAX_GRID = 2048;  // the step launch's grid cap (beyond it a workgroup walks a run of consecutive chunks)
struct AdamStepArgs {
  const rgfm_adam_entry* tab;  // device table, sorted by offset
  int n;
  uint64_t span_begin, n_chunks;  // first float of the flat range the table covers; its chunks (set by launch_adam_step)
  float *exp_avg, *exp_avg_sq, *ema;  // ema null: no average kept
  const double* partials;             // [ADAM_PARTIALS] of launch_adam_norm, or null: no norm, coef = 1
  float* grad_norm_out;               // optional
  double lr, beta1, one_minus_beta1, beta2, one_minus_beta2, wd, decay_mul, max_norm, ema_decay, one_minus_ema_decay;
  float eps;
  int decoupled;
};
void launch_adam_norm(const rgfm_adam_entry* tab, int n, uint64_t span_begin, uint64_t span_end, double* partials,
                      hipStream_t s);
void launch_adam_step(AdamStepArgs a, uint64_t span_end, hipStream_t s);

}  // namespace rgfm
