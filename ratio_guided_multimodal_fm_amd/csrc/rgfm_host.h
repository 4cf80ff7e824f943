// rgfm_host.h -- host-side internals shared by the translation units of the C ABI (api_*.cpp): error text, the
// hipEvent kernel-class timers, workspace carving, the per-thread run-time switches (Modes; with the process-wide
// ConvTuning of rgfm_kernels.h the only two places that can change conv routing), per-device state, conv dispatch,
// the U-Net handle and its inference walk over the plan's op list (unet_plan.h: the one place that knows the network's
// topology; the walk is used by the samplers and the gradient-guided loop too) and the guidance launch.
// (What only the sampler loops share is in sampler_host.h.)  Not part of the public ABI (that is include/rgfm.h);
// everything here is `inline` / C++17 inline variables, so every unit sees ONE definition.
//
//   api_core.cpp     rgfm_last_error, rgfm_abi_version, rgfm_profile_*
//   api_unet.cpp     rgfm_unet_*            (create / forward / trace hooks)
//   api_sampler.cpp  rgfm_sample_single, rgfm_guidance_*, rgfm_sample_pair
//   api_ratio.cpp    rgfm_ratio_*, gradient of log r, rgfm_sample_pair_grad
//   api_train.cpp    rgfm_unet_forward_train / _backward (U-Net training pass)
//   api_ratio_train.cpp  rgfm_ratio_forward_train / _backward (ratio estimators' training pass)
//   api_fmnet.cpp    rgfm_fmnet_*           (FlowMatchingModel)
//   api_fmnet_train.cpp  rgfm_fmnet_forward_train / _backward / _update_params (FlowMatchingModel's training pass)
//   api_clf.cpp      rgfm_clf_*             (the evaluation classifiers: handle, training pass, cross-entropy)
//   api_optim.cpp    rgfm_adam_*            (the optimizer step: gradient norm, clip, Adam / AdamW, weight EMA)
//
// No PyTorch types, no allocation and no synchronisation inside forward / sample calls (everything is carved from the
// caller's workspace, stream-ordered).
#pragma once
#include "../../include/rgfm.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rgfm_kernels.h"
#include "unet_plan.h"  // the weight-plan types (Cursor .. ResW) and the U-Net's plan: parameter offsets + op list

using namespace rgfm;

static_assert(UNET_KC == KC, "unet_plan.h states the conv kernels' K chunk for the Winograd-image condition");

// ------------------------------------------------------------------ errors
inline thread_local std::string g_err;

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return fail(RGFM_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)


// ------------------------------------------------------------------ profiling (bench support)
struct Prof {
  bool on = false;
  std::vector<hipEvent_t> ev;  // pairs
  std::vector<int> cls;
  size_t used = 0;
  double flops[RGFM_KCLASS_COUNT] = {};  // algorithmic FLOPs (conv class) or algorithmic HBM bytes (the others)
  double sum_ms[RGFM_KCLASS_COUNT] = {};
  int64_t launches[RGFM_KCLASS_COUNT] = {};
  std::vector<std::pair<double, double>> iv[RGFM_KCLASS_COUNT];  // [start, stop] ms since the first event
  hipEvent_t base = nullptr;
  bool have_base = false;
};
inline Prof g_prof;

struct ProfScope {
  bool active = false;
  size_t idx = 0;
  hipStream_t s;
  ProfScope(int kclass, double flops, hipStream_t stream) : s(stream) {
    if (!g_prof.on) return;
    if (g_prof.used + 2 > g_prof.ev.size()) {
      for (int i = 0; i < 4096; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        g_prof.ev.push_back(e);
      }
      g_prof.cls.resize(g_prof.ev.size() / 2);
    }
    if (!g_prof.have_base) {
      if (!g_prof.base && hipEventCreate(&g_prof.base) != hipSuccess) return;
      (void)hipEventRecord(g_prof.base, s);
      g_prof.have_base = true;
    }
    idx = g_prof.used;
    g_prof.used += 2;
    g_prof.cls[idx / 2] = kclass;
    g_prof.flops[kclass] += flops;
    g_prof.launches[kclass] += 1;
    (void)hipEventRecord(g_prof.ev[idx], s);
    active = true;
  }
  ~ProfScope() {
    if (active) (void)hipEventRecord(g_prof.ev[idx + 1], s);
  }
};

inline int prof_collect() {
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    HIP_TRY(hipEventSynchronize(g_prof.ev[i + 1]));
    float t0 = 0.f, t1 = 0.f;
    HIP_TRY(hipEventElapsedTime(&t0, g_prof.base, g_prof.ev[i]));
    HIP_TRY(hipEventElapsedTime(&t1, g_prof.base, g_prof.ev[i + 1]));
    const int k = g_prof.cls[i / 2];
    g_prof.sum_ms[k] += (double)t1 - (double)t0;
    g_prof.iv[k].push_back({(double)t0, (double)t1});
  }
  g_prof.used = 0;
  return RGFM_OK;
}

inline double prof_union_ms(int k) {
  auto v = g_prof.iv[k];
  std::sort(v.begin(), v.end());
  double total = 0.0, lo = 0.0, hi = -1.0;
  for (const auto& p : v) {
    if (p.first > hi) {
      if (hi >= lo) total += hi - lo;
      lo = p.first, hi = p.second;
    } else if (p.second > hi) {
      hi = p.second;
    }
  }
  if (hi >= lo) total += hi - lo;
  return total;
}


// ------------------------------------------------------------------ small helpers

struct Bump {  // workspace carving; dry = size-only pass
  char* base = nullptr;
  size_t off = 0;
  size_t cap = 0;
  bool dry = true;
  bool overflow = false;
  Bump() = default;
  Bump(void* ws, size_t ws_bytes) : base((char*)ws), cap(ws_bytes), dry(false) {}  // the live pass over a caller's workspace
  unsigned* u(size_t n) { return reinterpret_cast<unsigned*>(f(n)); }  // n 32-bit words (arrival counters)
  float* f(size_t nfloats) {
    const size_t bytes = (nfloats * sizeof(float) + 255) & ~(size_t)255;
    const size_t o = off;
    off += bytes;
    if (dry) return nullptr;
    if (off > cap) {
      overflow = true;
      return reinterpret_cast<float*>(base);  // never dereferenced: caller checks overflow first
    }
    return reinterpret_cast<float*>(base + o);
  }
};

struct Tensor {  // NHWC activation + its GroupNorm partial statistics
  float* data = nullptr;
  float* stats = nullptr;
  int C = 0, S = 0;
  void* p = nullptr;     // the same map in P format (ConvArgs::pout / pin0), when its producer wrote it
  bool p_valid = false;
};

inline int nt32_of(int cout) { return (cout % 64 == 0) ? 2 : 1; }

inline bool on_gfx950() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
  return strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

// Run-time switches, read from the environment ONCE per API call (refresh_modes), never on the launch path.  What can
// change conv routing is described in exactly two places: Modes (per host thread: which kernels are eligible) and
// ConvTuning (rgfm_kernels.h; process-wide: thresholds and cuts inside the kernels' own supported() / launch code).
// refresh_modes fills both -- ConvTuning's RGFM_HX2D cut, RGFM_WINO_W32, RGFM_S2_F32 and RGFM_CONV_SIMPLE -- except
// RGFM_HX2P_HALF, which belongs to the device's CU count and is read with it (ensure_init).
//   RGFM_CONV = hx2 (default: conv_mfma_hx2.hip, fp32 operands as two scaled fp16 planes, three f16-MFMA products
//               per fp32 product) | bx3 (conv_mfma_bx3.hip: three exact bf16 planes, six products; fp32 range)
//               | f32 (conv_mfma.hip: v_mfma_f32_32x32x2_f32 everywhere);
//   RGFM_OVERLAP=0   both velocity nets of a step on the caller's stream;
//   RGFM_FUSE_FIN=0  separate gn_finalize launches instead of the producer-side finalize;
//   RGFM_GN=table    every GroupNorm finalized into a scale/shift array instead of the consumer-side prologue;
//   RGFM_HX2P=0, RGFM_HX2Q=0, RGFM_HX2S=0, RGFM_HX2C=0, RGFM_HX2D=0, RGFM_GRAPH=1: A/B switches of the pipelined fp16
//               kernel, its four-waves-per-SIMD version, the stride-2 kernel, the 8x8-level kernel, the P-format hand-over
//               between a ResBlock's two convs (conv_mfma_hx2d.hip) and the hipGraph replay;
//   RGFM_HX2U=0      the Upsample convs on conv_mfma_hx2p_kernel<*, CONV_T2, *>, a workgroup per parity class (A/B switch, bit-identical).
enum { CONV_ARITH_HX2 = 0, CONV_ARITH_BX3 = 1, CONV_ARITH_F32 = 2 };
struct Modes {
  int conv = CONV_ARITH_HX2;
  bool overlap = true, fuse_fin = true, gn_consumer = true;
  bool pipelined = true;  // RGFM_HX2P=0: the fp16 convs on conv_mfma_hx2_kernel only (A/B switch)
  bool quad = true;       // RGFM_HX2Q=0: no four-waves-per-SIMD workgroups (conv_mfma_hx2q.hip; A/B switch, bit-identical)
  bool c8 = true;         // RGFM_HX2C=0: the 8x8 level on conv_mfma_hx2p_kernel (A/B switch)
  bool s2 = true;         // RGFM_HX2S=0: the Downsample convs on conv_mfma_hx2_kernel<*, CONV_S2, *> (A/B switch; same to 1e-6)
  bool pfmt = true;       // RGFM_HX2D=0: no P-format hand-over conv1 -> conv2 at the 16x16 / 8x8 levels (A/B switch)
  bool wino = false;      // RGFM_WINO=1: the Winograd form of the long-K stride-1 convs (conv_mfma_hx2w.hip) -- opt-in: faster per
                          // layer in isolation at 32x32, slower on the whole bench
  bool up_t2 = true;      // RGFM_UP_T2=0: the Upsample convs as nine taps over the upsampled raster instead of four parity classes (A/B switch)
  bool up_merged = true;  // RGFM_HX2U=0: the parity-class Upsample convs on conv_mfma_hx2p_kernel instead of conv_mfma_hx2u_kernel (A/B switch, bit-identical)
  bool rev_hx2 = true;    // RGFM_REV_HX2=0: the reverse convs of the gradient-guided sampler on the exact fp32 MFMA (A/B switch)
  bool prephase = true;   // RGFM_PREPHASE_PRIO=0: the two-net unguided entry (rgfm_sample_two) with its earlier schedule -- one chain
                          // enqueued after the other, unpaced -- instead of step by step with the lighter chain paced (A/B switch)
  bool graph = false;     // RGFM_GRAPH=1: the guided steps of the paired U-Net loop replayed from one captured hipGraph
                          // (bit-identical; measured 0.995-1.002x of the kernel-by-kernel path: the host is not the bottleneck)
};
inline thread_local Modes g_modes;  // per host thread: a handle's own conv arithmetic (rgfm_*_set_conv_mode) overrides it per network walk
inline void refresh_modes() {
  Modes m;
  const char* e = getenv("RGFM_CONV");
  if (e && strcmp(e, "bx3") == 0) m.conv = CONV_ARITH_BX3;
  else if (e && strcmp(e, "f32") == 0) m.conv = CONV_ARITH_F32;
  e = getenv("RGFM_OVERLAP");
  m.overlap = !(e && e[0] == '0');
  e = getenv("RGFM_FUSE_FIN");
  m.fuse_fin = !(e && e[0] == '0');
  e = getenv("RGFM_GN");
  m.gn_consumer = !(e && strcmp(e, "table") == 0);
  e = getenv("RGFM_HX2P");
  m.pipelined = !(e && e[0] == '0');
  e = getenv("RGFM_HX2Q");
  m.quad = !(e && e[0] == '0');
  e = getenv("RGFM_HX2S");
  m.s2 = !(e && e[0] == '0');
  e = getenv("RGFM_HX2C");
  m.c8 = !(e && e[0] == '0');
  e = getenv("RGFM_HX2D");
  m.pfmt = !(e && e[0] == '0');
  g_conv_tuning.hx2d_cut = e && e[0] == '1' ? 1 : (e && e[0] == '2' ? 2 : 3);
  e = getenv("RGFM_WINO");
  m.wino = e && e[0] == '1';
  e = getenv("RGFM_UP_T2");
  m.up_t2 = !(e && e[0] == '0');
  e = getenv("RGFM_HX2U");
  m.up_merged = !(e && e[0] == '0');
  e = getenv("RGFM_REV_HX2");
  m.rev_hx2 = !(e && e[0] == '0');
  e = getenv("RGFM_GRAPH");
  m.graph = e && e[0] == '1';
  e = getenv("RGFM_PREPHASE_PRIO");
  m.prephase = !(e && e[0] == '0');
  g_modes = m;
  e = getenv("RGFM_WINO_W32");
  g_conv_tuning.wino_w32 = e ? atoi(e) : 0;
  e = getenv("RGFM_HX2U_WGS");
  g_conv_tuning.hx2u_wgs_env = e ? atoi(e) : 0;
  g_conv_tuning.s2_f32 = getenv("RGFM_S2_F32") != nullptr;
  g_conv_tuning.f32_simple = getenv("RGFM_CONV_SIMPLE") != nullptr;
}

// A handle's own conv arithmetic (rgfm_unet_set_conv_mode / rgfm_fmnet_set_conv_mode; -1: the environment's) for the
// duration of one network walk.
struct ModeScope {
  int saved;
  explicit ModeScope(int handle_mode) : saved(g_modes.conv) {
    if (handle_mode >= 0) g_modes.conv = handle_mode;
  }
  ~ModeScope() { g_modes.conv = saved; }
};

// Per-device state, created by the first rgfm_*_create on that device (never inside forward / sample calls):
// raised dynamic-LDS limits (a per-device function attribute), the side stream + fork/join events of the paired
// sampler, and the range-flag word of conv_mfma_hx2.hip.
constexpr int MAX_DEVICES = 16;
struct DevState {
  bool init = false;
  int num_cus = 256;
  hipStream_t side = nullptr;
  void* zeros = nullptr;  // 256 zero bytes: the source of the padding records of conv_mfma_hx2d_kernel's halo DMA
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t pre_pace = nullptr;  // the two-net unguided entry (two_loop, api_sampler.cpp): paces the lighter chain
  // the legacy default stream cannot be captured: a caller on it has its graph-replayed loop run on `main`,
  // forked from / joined back into the default stream with these events
  hipStream_t main = nullptr;
  hipEvent_t main_fork = nullptr, main_join = nullptr;
  // hipGraphs of earlier sampler calls that may still be executing: destroyed once `graph_done` (recorded behind the
  // latest replay) has completed
  hipEvent_t graph_done = nullptr;
  std::vector<std::pair<hipGraphExec_t, hipGraph_t>> graphs;
};
inline DevState g_dev[MAX_DEVICES];

inline DevState* cur_dev() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
  return g_dev[dev].init ? &g_dev[dev] : nullptr;
}

inline int ensure_init() {
  if (!on_gfx950()) return fail(RGFM_ENODEVICE, "librgfm_hip needs a gfx950 (MI355X) device; none is current");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= MAX_DEVICES) return fail(RGFM_EINVAL, "device ordinal %d out of range (max %d)", dev, MAX_DEVICES - 1);
  DevState& d = g_dev[dev];
  if (!d.init) {
    int rc = guid_apply_init();
    for (const ConvKernel& k : CONV_KERNELS) rc |= k.init();
    rc |= conv_hx2u_init();  // (a cut of route hx2p: launch_conv)
    if (rc != 0) return fail(RGFM_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) == hipSuccess) d.num_cus = p.multiProcessorCount;
    const char* e = getenv("RGFM_HX2P_HALF");
    g_conv_tuning.hx2p_half = e ? atoi(e) : d.num_cus;  // launches with fewer 128-channel workgroups than CUs take 64-channel workgroups
    g_conv_tuning.hx2u_wgs = d.num_cus;                 // a tile-walking workgroup per CU (conv_mfma_hx2u.hip)
    HIP_TRY(hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&d.zeros, 256));
    HIP_TRY(hipMemset(d.zeros, 0, 256));
    HIP_TRY(hipEventCreateWithFlags(&d.fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d.join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d.graph_done, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&d.main, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&d.main_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d.main_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d.pre_pace, hipEventDisableTiming));
    d.init = true;
  }
  return RGFM_OK;
}

// Where the Winograd form is the faster kernel (tools/kbench, B = 512, profiles/r04_kbench/hx2w_vs_direct.txt): its K loop
// costs less per chunk than the direct kernels', its epilogue (the output transform through LDS) more -- so the long-K
// layers: 128 or more input channels.  By layer shape only, never by batch.
inline bool hx2w_pays(const ConvArgs& c) {
  return c.wpkw != nullptr && c.C0 + c.C1 >= 128 && (!g_conv_tuning.wino_w32 || c.g.W == 32);
}

// Which kernel launch_conv sends this launch to (RGFM_ROUTE_*): the one place the predicate chain is written.
inline int conv_route(const ConvArgs& c, int mode) {
  if (c.pin0) return RGFM_ROUTE_HX2D;  // (P-format input: only conv_mfma_hx2d_kernel reads it; the walk has checked conv_hx2d_supported)
  const bool hx2 = g_modes.conv == CONV_ARITH_HX2, pipe = hx2 && g_modes.pipelined;
  if (pipe && g_modes.wino && hx2w_pays(c) && conv_hx2w_supported(c, mode)) return RGFM_ROUTE_HX2W;
  if (pipe && g_modes.s2 && conv_hx2s_supported(c, mode)) return RGFM_ROUTE_HX2S;
  if (pipe && g_modes.c8 && conv_hx2c_supported(c, mode)) return RGFM_ROUTE_HX2C;
  if (pipe && g_modes.quad && conv_hx2q_supported(c, mode)) return RGFM_ROUTE_HX2Q;
  if (pipe && conv_hx2p_supported(c, mode)) return RGFM_ROUTE_HX2P;
  if (hx2 && conv_hx2_supported(c, mode)) return RGFM_ROUTE_HX2;
  if (g_modes.conv != CONV_ARITH_F32 && conv_bx3_supported(c, mode)) return RGFM_ROUTE_BX3;
  return RGFM_ROUTE_F32;
}

// Would launch_conv send this launch to a kernel that can write ConvArgs::pout (the P-format hand-over)?  Asked with
// pout already set, which conv_hx2w_supported rejects: the Winograd line of conv_route cannot fire here.
inline bool p_producer_ok(const ConvArgs& c, int mode) {
  if (!g_modes.pfmt) return false;
  const int route = conv_route(c, mode);
  if (route == RGFM_ROUTE_HX2C) return true;
  // conv_mfma_hx2p_kernel: 16x16 rasters (a tile = one whole sample), whole power-of-two groups per 32-channel wave block
  return route == RGFM_ROUTE_HX2P && mode == CONV_S1 && c.g.W == 16 && c.g.H == 16 && c.g.spt == 1 && c.g.tps == 1 &&
         (c.Cout == 64 || c.Cout == 128 || c.Cout == 256) && !c.ep_scale && !c.fin_ab;
}

// A launch whose key matches no instantiation of its kernel launches nothing: the error text says so (rgfm_last_error).
inline bool launch_conv_on(int route, const ConvArgs& c, int mode, hipStream_t s) {
  const ConvKernel& k = CONV_KERNELS[route];
  if (k.launch(c, mode, s)) return true;
  fail(RGFM_EINVAL, "no %s instantiation for mode %d, Cout %d, %d x %d raster, res_mode %d", k.name, mode, c.Cout, c.g.H, c.g.W, c.res_mode);
  return false;
}

// routes: the handle's per-route launch counts (RGFM_ROUTE_SLOTS entries), or null
// up_merged: the handle's count of launches that took conv_mfma_hx2u_kernel, or null.  That kernel is a cut of route hx2p
// (an Upsample's parity classes from one staged halo), chosen by layer shape only: it counts as hx2p in `routes`.
inline void launch_conv(const ConvArgs& c, int mode, hipStream_t s, int* routes = nullptr, int* up_merged = nullptr) {
  const int route = conv_route(c, mode);
  if (routes) {
    routes[route] += 1;
    if (mode == CONV_T2) routes[RGFM_ROUTE_T2] += 1;
  }
  if (route == RGFM_ROUTE_HX2P && g_modes.up_merged && conv_hx2u_supported(c, mode)) {
    if (up_merged) *up_merged += 1;
    if (!launch_conv_hx2u(c, mode, s)) fail(RGFM_EINVAL, "no hx2u instantiation for a %d x %d raster", c.g.H, c.g.W);
    return;
  }
  launch_conv_on(route, c, mode, s);
}



// ------------------------------------------------------------------ fp16-path range flag
// Every U-Net / FlowMatchingModel handle owns one device word.  conv_mfma_hx2*.hip OR into it: bit 0 when a staged
// activation reaches |S_A a| >= 32768 (fp16 would overflow), bit 1 when an output that a later conv stages raw is too
// small for the two-plane representation (ConvArgs::small_check).  Either way the results of the handle's calls since
// the last reset are not fp32-class and the caller repeats them with the handle switched to RGFM_CONV_BX3 (bit 0: fp32's
// exponent range at the top) or to RGFM_CONV_F32 (bit 1: the exact fp32 matrix-core convs, the reference's arithmetic
// at any magnitude) -- what _engine._range_guarded and INTEGRATION.md section B do.  Per handle, so that two threads /
// two engines on one device cannot consume each other's flag.
inline int read_flag_word(unsigned* word, int* flagged, int reset, hipStream_t s) {
  if (!flagged) return fail(RGFM_EINVAL, "null output");
  *flagged = 0;
  if (!word) return RGFM_OK;
  unsigned v = 0;
  HIP_TRY(hipMemcpyAsync(&v, word, sizeof(v), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *flagged = (int)v;
  if (reset && v) HIP_TRY(hipMemsetAsync(word, 0, sizeof(v), s));
  return RGFM_OK;
}
inline int alloc_flag_word(unsigned** word) {
  HIP_TRY(hipMalloc(word, 256));
  HIP_TRY(hipMemset(*word, 0, 256));
  return RGFM_OK;
}
inline int check_conv_mode(int mode) {
  if (mode < -1 || mode > CONV_ARITH_F32) return fail(RGFM_EINVAL, "conv mode must be RGFM_CONV_DEFAULT, _HX2, _BX3 or _F32");
  return RGFM_OK;
}


// ------------------------------------------------------------------ weight store
// The device buffers every handle owns, sized by its plan's WeightLayout.
struct WeightStore : WeightLayout {
  float* params = nullptr;            // device copy of the state_dict-order blob
  float* packed = nullptr;            // packed fp32 conv weights (+ whatever else the handle re-lays out)
  unsigned short* packed3 = nullptr;  // 3-plane bf16 weights (conv_mfma_bx3.hip); null when the plan has none
  unsigned short* packedh = nullptr;  // 2-plane scaled fp16 weights (conv_mfma_hx2.hip)
  float* hq = nullptr;                // [n_hq][4] scale records of packedh
  unsigned* range_flag = nullptr;     // this handle's range-flag word (the velocity nets)
  int conv_mode = -1;                 // rgfm_*_set_conv_mode: -1 = RGFM_CONV from the environment

  // allocates the buffers of the layout and copies the caller's blob in (stream-ordered)
  int alloc(const float* params_dev, bool with_range_flag, hipStream_t s) {
    if (hipMalloc(&params, n_params * sizeof(float)) != hipSuccess) return fail(RGFM_ENOMEM, "hipMalloc(params)");
    if (hipMalloc(&packed, (n_packed + 4) * sizeof(float)) != hipSuccess) return fail(RGFM_ENOMEM, "hipMalloc(packed)");
    if (hipMalloc(&packedh, (n_packedh + 8) * sizeof(unsigned short)) != hipSuccess) return fail(RGFM_ENOMEM, "hipMalloc(packedh)");
    if (hipMalloc(&hq, ((size_t)n_hq * 4 + 4) * sizeof(float)) != hipSuccess) return fail(RGFM_ENOMEM, "hipMalloc(hq)");
    if (with_range_flag && alloc_flag_word(&range_flag) != RGFM_OK) return fail(RGFM_ENOMEM, "hipMalloc(range flag)");
    if (n_packed3 && hipMalloc(&packed3, (n_packed3 + 8) * sizeof(unsigned short)) != hipSuccess)
      return fail(RGFM_ENOMEM, "hipMalloc(packed3)");
    if (hipMemcpyAsync(params, params_dev, n_params * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(RGFM_EHIP, "hipMemcpyAsync(params)");
    return RGFM_OK;
  }
  void free() {
    for (void* p : {(void*)params, (void*)packed, (void*)packed3, (void*)packedh, (void*)hq, (void*)range_flag})
      if (p) (void)hipFree(p);
  }
};

// after the pack launches: which images may run on the fp16 path, from their scale records (one synchronising copy)
inline int read_hx_flags(const WeightStore& st, const std::vector<HxImage*>& images, hipStream_t s) {
  std::vector<float> host((size_t)st.n_hq * 4);
  if (hipMemcpyAsync(host.data(), st.hq, host.size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(RGFM_EHIP, "reading the fp16 scale records failed");
  for (HxImage* i : images) i->ok = host[(size_t)i->hq * 4 + 3] != 0.f;
  return RGFM_OK;
}

// The normalised inputs of the fp16 path are S_A silu(gamma xhat + beta): in range for every trained net the reference
// can produce, but a conv whose norm parameters are tiny (the activation would sit in the fp16 subnormals) or huge is
// routed to the split-bf16 kernel, like a conv with out-of-window weights.  `host` = the parameter blob.
inline bool norm_params_ok(const std::vector<float>& host, size_t gw, size_t gb, int C) {
  float mg = 0.f, mb = 0.f;
  for (int i = 0; i < C; ++i) mg = std::max(mg, std::fabs(host[gw + i])), mb = std::max(mb, std::fabs(host[gb + i]));
  if (!(mg <= 3.0e38f) || !(mb <= 3.0e38f)) return false;
  const float hi = 8.f * mg + mb, lo = std::max(mg, mb);  // |gamma xhat + beta| for |xhat| <= 8; the activation's scale
  return hi < 1024.f && lo >= 0.015625f;
}

struct NormGate {  // a GroupNorm (blob offsets, channels) in front of the conv that owns `image`
  size_t gamma, beta;
  int C;
  HxImage* image;
};

// after read_hx_flags (which recomputes every verdict): convs behind a GroupNorm with out-of-window parameters leave
// the fp16 path (one synchronising read of the blob)
inline int demote_by_norms(const WeightStore& st, const std::vector<NormGate>& gates, hipStream_t s) {
  std::vector<float> host(st.n_params);
  if (hipMemcpyAsync(host.data(), st.params, host.size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(RGFM_EHIP, "reading the parameters back failed");
  for (const NormGate& g : gates)
    if (!norm_params_ok(host, g.gamma, g.beta, g.C)) g.image->ok = false;
  return RGFM_OK;
}


// ================================================================== U-Net
struct rgfm_unet : WeightStore, UNetPlan {  // (the plan: unet_plan.h; its `layout` is also the store's WeightLayout)
  rgfm_unet_desc d;
  float* freqs = nullptr;
  TimeLinear* lin_dev = nullptr;
  float* wtmp = nullptr;  // scratch of the Upsample / Winograd weight images (kept for rgfm_unet_update_params)
  int nlin = 0;
  // class conditioning (rgfm_unet_labeled_create): K classes, label_emb.weight [K + 1][temb] at `lemb`, behind the
  // unlabelled blob (n_params counts it); 0: an unlabelled net
  int num_classes = 0;
  size_t lemb = 0;
  bool trace = false;
  int wino_convs = 0;   // convs of the latest walk described for the Winograd kernel (rgfm_unet_wino_convs)
  int up_merged = 0;    // convs of the latest walk that ran on conv_mfma_hx2u_kernel (rgfm_unet_up_merged)
  int p_handovers = 0;  // ResBlocks of the latest walk whose conv1 -> conv2 hand-over took the P format (rgfm_unet_p_handovers)
  int routes[RGFM_ROUTE_SLOTS] = {};  // conv launches of the latest walk per route, + CONV_T2 launches (rgfm_unet_conv_routes)
  struct Act {
    float* data;
    int C, S;
    bool nchw;
  };
  std::vector<Act> acts;  // filled by the last (non-dry) run in trace mode
};


inline int check_desc(const rgfm_unet_desc* d) {
  if (!d) return fail(RGFM_EINVAL, "null descriptor");
  if (d->in_channels != 1 && d->in_channels != 3) return fail(RGFM_EINVAL, "in_channels must be 1 or 3");
  if (d->num_levels < 1 || d->num_levels > RGFM_MAX_LEVELS) return fail(RGFM_EINVAL, "1..4 levels supported");
  if (d->model_channels % 32 != 0 || d->model_channels > 256) return fail(RGFM_EINVAL, "model_channels must be a multiple of 32, <= 256");
  if (d->num_res_blocks < 1 || d->num_res_blocks > 8) return fail(RGFM_EINVAL, "num_res_blocks out of range");
  if (d->img_size < 4 || d->img_size > 64) return fail(RGFM_EINVAL, "img_size must be in 4..64");
  int s = d->img_size;
  for (int l = 0; l < d->num_levels; ++l) {
    if (d->channel_mult[l] < 1) return fail(RGFM_EINVAL, "channel_mult must be >= 1");
    if (d->model_channels * d->channel_mult[l] > 256) return fail(RGFM_EINVAL, "at most 256 channels per level");
    if (l < d->num_levels - 1) {
      if (s % 2) return fail(RGFM_EINVAL, "odd resolution before a downsample is not supported");
      s /= 2;
    }
  }
  return RGFM_OK;
}

inline void pack_one(const rgfm_unet* h, const ConvW& w, int mode, hipStream_t s) {
  launch_pack_conv(h->params + w.w_raw, h->packed + w.w_pk, w.cout, w.cin, w.taps, nt32_of(w.cout), s);
  if (mode == CONV_S2) launch_pack_conv_bx3_s2(h->params + w.w_raw, h->packed3 + w.w_bx3, w.cout, w.cin, s);
  else launch_pack_conv_bx3(h->params + w.w_raw, h->packed3 + w.w_bx3, w.cout, w.cin, w.taps, s);
  launch_pack_conv_hx2(h->params + w.w_raw, h->packedh + w.hx.off, h->hq + 4 * w.hx.hq, w.cout, w.cin, w.taps, mode, s);
}

// fills the fp16-path fields of a conv launch (main conv `w`, optional fused 1x1 skip `sk`)
inline void fill_hx2(ConvArgs& c, const WeightStore& st, const ConvW& w, const ConvW* sk) {
  if (!w.hx.usable() || (sk && !sk->hx.usable())) return;
  c.wpkh = st.packedh + w.hx.off, c.hq = st.hq + 4 * w.hx.hq, c.range_flag = st.range_flag;
  if (w.hx9.usable()) c.wpkh9 = st.packedh + w.hx9.off;
  if (w.wino.usable() && !sk) c.wpkw = st.packedh + w.wino.off, c.hqw = st.hq + 4 * w.wino.hq;
  if (sk) c.wskiph = st.packedh + sk->hx.off, c.hq_skip = st.hq + 4 * sk->hx.hq;
}

inline double conv_flops(int B, int HW, int cout, int kprod) { return 2.0 * B * HW * (double)cout * kprod; }

// True when the statistics of a map written by a CONV_T2 launch over an S x S raster (4 parity classes x that raster's
// parts) are indistinguishable, part for part, from those of a plain 2S x 2S map: same number of parts, same pixel
// counts.  (32 <- 16 and 16 <- 8: 64-pixel parts on both sides.)
inline bool up_parts_match(int S) {
  const TileGeom gl = make_geom(S, S), gf = make_geom(2 * S, 2 * S);
  if (gf.nparts != 4 * gl.nparts || gf.nparts > 16) return false;
  for (int p = 0; p < gf.nparts; ++p)
    if (geom_part_count(gf, p) != geom_part_count(gl, p % gl.nparts)) return false;
  return true;
}

// A conv that has been described but not launched yet: if the next thing the walk asks for is the
// GroupNorm finalize of its output, the finalize is attached to it (ConvArgs::fin_*: the last wave per
// sample computes the scale/shift) and no gn_finalize launch happens -- each such launch is a full
// drain-and-refill bubble between two convs (measured: 18 % of the sampling call).
struct PendingConv {
  bool valid = false;
  ConvArgs c{};
  int mode = 0;
  double flops = 0.0;
};

inline void flush_conv(PendingConv& p, hipStream_t s, int* routes = nullptr, int* up_merged = nullptr) {
  if (!p.valid) return;
  p.valid = false;
  ProfScope ps(RGFM_KCLASS_CONV_MFMA, p.flops, s);
  launch_conv(p.c, p.mode, s, routes, up_merged);
}

// true when `p` can take the finalize of cat(its output, partner) itself
inline bool try_fuse_finalize(PendingConv& p, const float* first_data, const float* stats1, int C1, const float* gamma,
                       const float* beta, float* ab, unsigned* counter) {
  if (!g_modes.fuse_fin || !p.valid || !counter || p.c.out != first_data || !p.c.stats_out) return false;
  if (p.c.pin0) return false;  // (conv_mfma_hx2d_kernel has no producer-side finalize: a gn_finalize launch follows)
  if ((p.c.Cout + C1) % 8 != 0 || p.c.Cout + C1 < 32 || p.c.Cout + C1 > 256) return false;  // <= 4 channels per lane
  if (p.c.g.nparts * (p.mode == CONV_T2 ? 4 : 1) > 16) return false;  // the finalizing wave holds <= 16 partials per channel
  p.c.fin_ab = ab, p.c.fin_counter = counter, p.c.fin_expected = conv_fin_expected(p.c, p.mode);
  p.c.fin_stats1 = stats1, p.c.fin_C1 = C1, p.c.fin_gamma = gamma, p.c.fin_beta = beta;
  return true;
}

// Consumer-side GroupNorm (default): the split-operand conv derives the scale/shift in its own prologue from the
// partial statistics (ConvArgs::gn_*); the table path (RGFM_GN=table) remains for the kernels that cannot
// (conv_out, RGFM_CONV=f32).  On failure the gn_* fields are cleared and the caller supplies `ab`.
inline bool try_consumer_gn(ConvArgs& c, int mode, const float* stats0, const float* stats1, int nparts0, const TileGeom& gg,
                     const float* gamma, const float* beta) {
  c.gn_stats0 = stats0, c.gn_stats1 = stats1, c.gn_gamma = gamma, c.gn_beta = beta, c.gn_nparts0 = nparts0, c.gn_g = gg;
  bool ok = false;
  if (g_modes.gn_consumer) {
    if (g_modes.conv == CONV_ARITH_HX2 && conv_hx2_supported(c, mode)) ok = conv_hx2_gn_supported(c, mode);
    else if (g_modes.conv != CONV_ARITH_F32) ok = conv_bx3_gn_supported(c, mode);
  }
  if (!ok) c.gn_stats0 = c.gn_stats1 = c.gn_gamma = c.gn_beta = nullptr;
  return ok;
}

struct NormRef {  // a GroupNorm in front of a conv: parameters (offsets into the blob)
  size_t gamma, beta;
};

struct UNetRun {
  rgfm_unet* h;
  int B;
  Bump* ws;
  hipStream_t s;
  const float* temb_row;  // table row(s) for this evaluation
  int temb_per_row;
  bool dry;
  unsigned* fin_counter = nullptr;  // [B] arrival counters (zero between launches) or null: separate gn_finalize
  const int* step_ptr = nullptr;    // device-side step counter: temb_row is then the table's first row (ConvArgs::step_ptr)
  PendingConv pend{};

  Tensor new_tensor(int C, int S) {
    Tensor t;
    t.C = C, t.S = S;
    const TileGeom g = make_geom(S, S);
    t.data = ws->f((size_t)B * S * S * C);
    t.stats = ws->f((size_t)B * g.nparts * C * 2);
    return t;
  }
  void record(const Tensor& t) {
    if (!dry && h->trace) h->acts.push_back({t.data, t.C, t.S, false});
  }
  float* finalize(const Tensor& a, const Tensor* b, size_t gamma, size_t beta, float* ab = nullptr) {
    const int C = a.C + (b ? b->C : 0);
    if (!ab) ab = ws->f((size_t)B * C * 2);
    if (dry) return ab;
    const bool fused = try_fuse_finalize(pend, a.data, b ? b->stats : nullptr, b ? b->C : 0, h->params + gamma,
                                         h->params + beta, ab, fin_counter);
    flush_conv(pend, s, h->routes, &h->up_merged);
    if (fused) return ab;
    GnFinalizeArgs f{};
    f.stats0 = a.stats, f.stats1 = b ? b->stats : nullptr;
    f.C0 = a.C, f.C1 = b ? b->C : 0;
    f.groups = C < 8 ? C : 8;
    f.gamma = h->params + gamma, f.beta = h->params + beta;
    f.ab = ab, f.B = B, f.g = make_geom(a.S, a.S);
    ProfScope p(RGFM_KCLASS_OTHER, 0, s);
    launch_gn_finalize(f, s);
    return ab;
  }
  // generic 3x3 conv launch
  // raw_consumed: a later conv stages this output without a GroupNorm in front (ConvArgs::small_check)
  Tensor conv(const Tensor& a, const Tensor* b, const NormRef* norm, const ConvW& w, int mode, const float* temb,
              int res_mode, const Tensor* r0, const Tensor* r1, const ConvW* sk, bool raw_consumed) {
    const int So = mode == CONV_S2 ? a.S / 2 : (mode == CONV_UP2 ? a.S * 2 : a.S);
    Tensor o = new_tensor(w.cout, So);
    float* ab_buf = norm ? ws->f((size_t)B * (a.C + (b ? b->C : 0)) * 2) : nullptr;  // used by the table path only
    if (dry) return o;
    const float* ab = nullptr;
    ConvArgs c{};
    c.in0 = a.data, c.in1 = b ? b->data : nullptr;
    c.C0 = a.C, c.C1 = b ? b->C : 0;
    c.Hin = c.Win = a.S;
    c.ab = ab;
    c.wpk = h->packed + w.w_pk;
    c.wpk3 = h->packed3 + w.w_bx3;
    c.bias = h->params + w.b;
    c.temb = temb, c.temb_stride = h->temb_total, c.temb_per_row = temb_per_row;
    c.step_ptr = temb ? step_ptr : nullptr;
    c.res_mode = res_mode;
    if (res_mode) {
      c.res0 = r0->data, c.res1 = r1 ? r1->data : nullptr;
      c.R0 = r0->C, c.R1 = r1 ? r1->C : 0;
    }
    if (res_mode == 2) c.wskip = h->packed + sk->w_pk, c.wskip3 = h->packed3 + sk->w_bx3, c.skip_bias = h->params + sk->b;
    c.out = o.data, c.stats_out = o.stats;
    c.B = B, c.Cout = w.cout;
    c.g = make_geom(So, So);
    c.halo_px = mode == CONV_S2 ? c.g.spt * (2 * c.g.th + 1) * (2 * c.g.W + 1) : c.g.spt * (c.g.th + 2) * (c.g.W + 2);
    const int kprod = 9 * w.cin + (res_mode == 2 ? sk->cin : 0);
    fill_hx2(c, *h, w, res_mode == 2 ? sk : nullptr);
    if (g_modes.conv == CONV_ARITH_HX2) c.range_flag = h->range_flag, c.small_check = raw_consumed ? 1 : 0;
    if (mode == CONV_UP2 && g_modes.conv == CONV_ARITH_HX2 && g_modes.up_t2 && w.t2.usable() && up_parts_match(a.S)) {
      // nearest x 2 + 3x3 == ConvTranspose2d(4, 2, 1) with summed taps: the parity-class form over the INPUT raster
      // (4 / 9 of the matrix work, a quarter of the halo per output).  Its statistics parts -- four classes x the input
      // raster's parts -- have the sizes of the output raster's parts (up_parts_match), so readers see a plain map.
      ConvArgs ct = c;
      ct.g = make_geom(a.S, a.S);
      ct.halo_px = ct.g.spt * (ct.g.th + 2) * (ct.g.W + 2);
      ct.wpkh = h->packedh + w.t2.off, ct.hq = h->hq + 4 * w.t2.hq;
      if (conv_hx2_supported(ct, CONV_T2)) c = ct, mode = CONV_T2;
    }
    bool p_in = false;
    if (norm && a.p_valid && !b) {
      // the producer (still pending) can hand this input over in P format: take it if conv_mfma_hx2d_kernel can run this
      // conv, otherwise the producer goes back to the fp32 map + statistics
      ConvArgs cp = c;
      DevState* ds = cur_dev();
      cp.pin0 = a.p, cp.zeros = ds ? ds->zeros : nullptr;
      if (pend.valid && pend.c.pout == a.p && conv_hx2d_supported(cp, mode)) {
        c = cp, p_in = true;
        h->p_handovers += 1;
        if (!h->trace) pend.c.out = nullptr, pend.c.stats_out = nullptr;  // (nothing else reads the fp32 map)
      } else if (pend.valid && pend.c.pout == a.p) {
        pend.c.pout = nullptr;
      }
    }
    if (norm && !p_in) {
      const TileGeom gg = make_geom(a.S, a.S);
      if (!try_consumer_gn(c, mode, a.stats, b ? b->stats : nullptr, gg.nparts, gg, h->params + norm->gamma,
                           h->params + norm->beta))
        c.ab = finalize(a, b, norm->gamma, norm->beta, ab_buf);  // (may attach itself to the pending producer)
    }
    flush_conv(pend, s, h->routes, &h->up_merged);
    if (conv_route(c, mode) == RGFM_ROUTE_HX2W) h->wino_convs += 1;  // (as described: a finalize or pout attached later moves it)
    pend.valid = true, pend.c = c, pend.mode = mode;
    pend.flops = conv_flops(B, So * So, w.cout, kprod);
    return o;
  }
  // ResBlock.forward (unet_flexible.py:71-85)
  Tensor resblock(const ResW& r, const Tensor& a, const Tensor* b) {
    const NormRef n1{r.n1w, r.n1b}, n2{r.n2w, r.n2b};
    Tensor h1 = conv(a, b, &n1, r.c1, CONV_S1, dry ? nullptr : temb_row + r.temb_off, 0, nullptr, nullptr, nullptr, false);
    // P-format hand-over (conv_mfma_hx2d.hip): at the 16x16 / 8x8 levels conv1's workgroups own whole (sample, group) sets
    // of h1, whose only reader is conv2 through norm2 + SiLU (unet_flexible.py:79-81) -- conv1 writes silu(norm2(h1))
    // already split, conv2 stages it by LDS-DMA.  The buffer is carved whenever the SHAPE allows it (dry and real walks
    // alike); whether the two launches take the hand-over is decided from the kernels they are dispatched to.
    // Where it pays (tools/kbench, profiles/r04_kbench/p_producer_overhead.txt + hx2d_cuts.txt, B = 512): writing the P
    // format costs the producer 2.2 us at 8x8 (of 36), 3.5 us at 16x16 / 64 channels, 6.5 us at 16x16 / 128 channels (its
    // epilogue is vector-ALU-bound: SiLU + split of every output); the consumer gains 6.7 / 5.5 - 6.5 / 3.6 - 4.4 us.  So:
    // the 8x8 level and 64-channel 16x16 layers; 128-channel 16x16 layers keep the fp32 hand-over.
    if ((a.S == 8 || (a.S == 16 && r.cout == 64)) && r.cout % 64 == 0) {
      h1.p = ws->f((size_t)B * a.S * a.S * r.cout);
      if (!dry && pend.valid && pend.c.out == h1.data && r.c1.hx.ok && r.c2.hx.ok && (!r.has_skip || r.sk.hx.ok)) {
        pend.c.pout = h1.p, pend.c.pn_gamma = h->params + r.n2w, pend.c.pn_beta = h->params + r.n2b;
        if (p_producer_ok(pend.c, pend.mode)) h1.p_valid = true;
        else pend.c.pout = nullptr;
      }
    }
    record(h1);
    // (a ResBlock's output is the residual stream: the next block's 1x1 skip, a Downsample or an Upsample reads it raw)
    Tensor o = conv(h1, nullptr, &n2, r.c2, CONV_S1, nullptr, r.has_skip ? 2 : 1, &a, b, r.has_skip ? &r.sk : nullptr, true);
    record(o);
    return o;
  }

  // FlexibleUNet.forward (unet_flexible.py:203-261), op by op of the handle's plan.  Exactly one of v_out / x_state
  // may be non-null... both allowed: v_out receives the velocity, x_state the Euler update.
  // x_base (with x_state): x_state = x_base + v dt, a midpoint stage that starts from another buffer than it writes;
  // null or x_state itself: the in-place update.
  int run(const float* x, float* v_out, float* x_state, float dt, const float* x_base = nullptr) {
    const rgfm_unet_desc& d = h->d;
    ModeScope mode_scope(h->conv_mode);
    if (!dry && h->trace) h->acts.clear();
    if (!dry) h->p_handovers = 0, h->wino_convs = 0, h->up_merged = 0, std::fill(h->routes, h->routes + RGFM_ROUTE_SLOTS, 0);
    std::vector<Tensor> T(h->tensors.size());  // the maps of this run, by the plan's tensor ids
    for (const UOp& o : h->ops) {
      switch (o.kind) {
        case UOP_IN: {
          const int S = o.S;
          const Tensor& cur = T[o.out] = new_tensor(h->mc, S);
          if (!dry) {
            ConvInArgs ci{};
            ci.x = x, ci.w = h->params + h->icw, ci.bias = h->params + h->icb;
            ci.out = cur.data, ci.stats_out = cur.stats, ci.B = B, ci.C0 = h->mc, ci.g = make_geom(S, S);
            ci.range_flag = h->range_flag, ci.small_check = g_modes.conv == CONV_ARITH_HX2 ? 1 : 0;  // (the last decoder block's skip reads it raw)
            // algorithmic bytes: the NCHW image in, the NHWC map (+ its statistics) out
            const TileGeom g0 = make_geom(S, S);
            ProfScope p(d.in_channels == 1 ? RGFM_KCLASS_CONV_IN1 : RGFM_KCLASS_CONV_IN3,
                        4.0 * B * ((double)S * S * (d.in_channels + h->mc) + 2.0 * g0.nparts * h->mc), s);
            launch_conv_in(ci, d.in_channels, s);
          }
          record(cur);
          break;
        }
        case UOP_RES:
          T[o.out] = resblock(h->res[o.idx], T[o.in0], o.in1 >= 0 ? &T[o.in1] : nullptr);
          break;
        case UOP_DOWN:
          T[o.out] = conv(T[o.in0], nullptr, nullptr, h->down[o.idx], CONV_S2, nullptr, 0, nullptr, nullptr, nullptr, true);
          record(T[o.out]);
          break;
        case UOP_UP:
          T[o.out] = conv(T[o.in0], nullptr, nullptr, h->up[o.idx], CONV_UP2, nullptr, 0, nullptr, nullptr, nullptr, true);
          record(T[o.out]);
          break;
        case UOP_OUT: {
          const Tensor& cur = T[o.in0];
          float* ab = finalize(cur, nullptr, h->onw, h->onb);
          if (dry) break;
          flush_conv(pend, s, h->routes, &h->up_merged);
          ConvOutArgs co{};
          co.in = cur.data, co.ab = ab, co.w = h->packed + h->ocw_pk, co.bias = h->params + h->ocb;
          co.v_out = v_out, co.x_state = x_state, co.dt = dt, co.B = B, co.Cin = cur.C;
          co.x_base = x_base == x_state ? nullptr : x_base;
          co.g = make_geom(cur.S, cur.S);
          co.halo_px = co.g.spt * (co.g.th + 2) * (co.g.W + 2);
          // algorithmic bytes: the NHWC map + its scale/shift in, the NCHW velocity out (fused Euler: state in and out)
          const double px = (double)B * cur.S * cur.S;
          ProfScope p(d.in_channels == 1 ? RGFM_KCLASS_CONV_OUT1 : RGFM_KCLASS_CONV_OUT3,
                      4.0 * (px * cur.C + 2.0 * B * cur.C + px * d.in_channels * ((v_out ? 1 : 0) + (x_state ? 2 : 0))), s);
          launch_conv_out(co, d.in_channels, s);
          if (h->trace && v_out) h->acts.push_back({v_out, d.in_channels, cur.S, true});
          break;
        }
      }
    }
    return RGFM_OK;
  }
};

inline size_t counter_bytes(int B) { return (((size_t)B * sizeof(unsigned)) + 255) & ~(size_t)255; }

inline size_t unet_eval_bytes(rgfm_unet* h, int B) {
  Bump b;
  UNetRun r{h, B, &b, nullptr, nullptr, 0, true};
  r.run(nullptr, nullptr, nullptr, 0.f);
  return b.off;
}

inline TimeEmbedArgs time_embed_args(const rgfm_unet* h, const float* t_dev, int num_steps, int step_begin, float* table) {
  TimeEmbedArgs a{};
  a.params = h->params, a.freqs = h->freqs, a.mc = h->mc, a.temb = h->temb;
  a.te0w = (int)h->te0w, a.te0b = (int)h->te0b, a.te2w = (int)h->te2w, a.te2b = (int)h->te2b;
  a.lin = h->lin_dev, a.nlin = h->nlin, a.total = h->temb_total;
  a.t_dev = t_dev, a.num_steps = num_steps, a.step_begin = step_begin, a.table = table;
  // a class-conditional net without labels is its own unconditional branch: every row takes the null label
  if (h->num_classes) a.label_emb = h->params + h->lemb, a.num_classes = h->num_classes, a.ncls = 1;
  return a;
}

// The time table of a labelled evaluation.  `labels` (device, one per row): row i is (t_dev[i] or t_dev[0], labels[i]),
// the forward's per-row table.  Null: rows (stage, class) of a sampler call, [nt / (K + 1)][K + 1][total].
inline int launch_class_table(rgfm_unet* h, const float* t_dev, int t_shared, const int* labels, int num_steps, int step_begin,
                              int nt, float* table, hipStream_t s) {
  ProfScope p(RGFM_KCLASS_OTHER, 0, s);
  TimeEmbedArgs a = time_embed_args(h, t_dev, num_steps, step_begin, table);
  a.labels = labels, a.t_shared = t_shared, a.ncls = labels ? 1 : h->num_classes + 1;
  launch_time_embed(a, nt, s);
  return RGFM_OK;
}

inline int launch_time_table(rgfm_unet* h, const float* t_dev, int num_steps, int step_begin, int nt, float* table,
                      hipStream_t s) {
  ProfScope p(RGFM_KCLASS_OTHER, 0, s);
  launch_time_embed(time_embed_args(h, t_dev, num_steps, step_begin, table), nt, s);
  return RGFM_OK;
}

inline size_t table_bytes(const rgfm_unet* h, int rows) {
  return (((size_t)rows * h->temb_total * sizeof(float)) + 255) & ~(size_t)255;
}


inline size_t guid_dist_bytes(int batch, int n_mc) {  // sliced fp64 distances, RGFM_GUID_SLICES slices at most
  return (((size_t)RGFM_GUID_SLICES * batch * (n_mc > 0 ? n_mc : 1) * sizeof(double)) + 255) & ~(size_t)255;
}
inline size_t guid_wbuf_bytes(int batch, int n_mc) {  // the step's importance weights [B][N]
  return (((size_t)batch * (n_mc > 0 ? n_mc : 1) * sizeof(float)) + 255) & ~(size_t)255;
}
inline size_t guid_wsum_bytes(int batch) { return ((size_t)batch * sizeof(float) + 255) & ~(size_t)255; }
inline size_t guid_scratch_bytes(int batch, int n_mc) {  // + the weights and their row sums [B]
  return guid_dist_bytes(batch, n_mc) + guid_wbuf_bytes(batch, n_mc) + guid_wsum_bytes(batch);
}
// Cross pairing (PAIRING_CROSS: all N x N pairs of the MC set): the paired block's scratch -- its weight rows are the x
// marginals -- then the y marginals and their row sums, then five [B][N] rows of the weights stage (a, b, u, s, q).
constexpr int PAIRING_PAIRED = 0, PAIRING_CROSS = 1;
constexpr int GUID_CROSS_MAX_N = 1024;
inline size_t guid_cross_scratch_bytes(int batch, int n_mc) {
  return guid_scratch_bytes(batch, n_mc) + guid_wbuf_bytes(batch, n_mc) + guid_wsum_bytes(batch) + 5 * guid_wbuf_bytes(batch, n_mc);
}
inline size_t guid_scratch_bytes(int batch, int n_mc, int pairing) {
  return pairing == PAIRING_CROSS ? guid_cross_scratch_bytes(batch, n_mc) : guid_scratch_bytes(batch, n_mc);
}


// The step's scalars of the guidance block: Python-double arithmetic of the reference
// (sample_mnist_svhn.py:115,127,135,159,170), rounded to fp32 where a tensor op consumes it.
inline void guidance_scalars(double t, float* tf, float* s2, float* cden) {
  const double eps = 1e-3;
  const double sigma_t = 1.0 - t + eps;
  *tf = (float)t, *s2 = (float)(sigma_t * sigma_t), *cden = (float)(1.0 - t + eps);
}

// Diagnostics of one evaluation of the block (include/rgfm.h, RGFM_DIAG_*).  rec: its [B][RGFM_DIAG_FLOATS] records,
// zeroed by the caller (the entries of a modality that is not there stay 0).  gx / gy: scratch velocities [B][dx] /
// [B][dy] holding finite values (zeroed once by the caller): they receive the pure guided velocity g -- one more
// launch_guid_apply with the blend (1 - gamma, gamma) = (0, 1) and no state update, the bits of the g inside the real one.
struct GuidDiag {
  float *rec, *gx, *gy;
};

// Guidance strength as data (include/rgfm.h, "Guidance strength per sample and per stage").
// Strength: what a loop is called with -- the scalar gamma, optionally a device vector of per-row strengths (fp32
// [batch]; null: gamma for every row) and a HOST array of per-stage scales (null: 1 for every stage), read while the
// call enqueues and not kept.  A plain double converts to the scalar-only strength, which is every existing entry point.
// StageStrength: one stage of it, what a GuidanceCall and the gradient loops' update take -- with `rows` null the blend
// is the scalar rule on `gamma` (already multiplied by the stage's scale, in double), otherwise row b has
// (double)rows[b] * scale, formed on the device.
struct StageStrength {
  double gamma = 0.0;
  const float* rows = nullptr;
  double scale = 1.0;
  StageStrength(double g) : gamma(g) {}
  StageStrength(double g, const float* r, double s) : gamma(g), rows(r), scale(s) {}
};
struct Strength {
  double gamma = 0.0;
  const float* rows = nullptr;
  const double* scale = nullptr;
  int n_scale = 0;
  Strength(double g) : gamma(g) {}
  Strength(double g, const float* r, const double* s, int n) : gamma(g), rows(r), scale(s), n_scale(n) {}
  bool is_data() const { return rows || scale; }  // (a call with either runs kernel by kernel: no graph replay)
  // before anything is enqueued: the scale array's length against the call's stage count, and finite entries
  int check(int n_stages) const {
    if (!scale) return n_scale == 0 ? RGFM_OK : fail(RGFM_EINVAL, "stage_scale null with n_stage_scale %d (null goes with 0)", n_scale);
    if (n_scale != n_stages) return fail(RGFM_EINVAL, "n_stage_scale %d != %d stages of the call", n_scale, n_stages);
    for (int k = 0; k < n_scale; ++k)
      if (!std::isfinite(scale[k])) return fail(RGFM_EINVAL, "stage_scale[%d] is not finite", k);
    return RGFM_OK;
  }
  double s(int k) const { return scale ? scale[k] : 1.0; }
  bool off(int k) const { return scale && scale[k] == 0.0; }  // the stage runs unguided
  StageStrength stage(int k) const { return rows ? StageStrength(gamma, rows, s(k)) : StageStrength(scale ? gamma * scale[k] : gamma); }
};

// What of the block a call of guidance_launch enqueues.
enum class GuidPhase {
  All,          // the whole block
  Weights,      // distances + importance weights only: they need the step's (x_t, y_t) and the MC set, not the velocities
  Apply,        // the rest (needs v, and the weights of an earlier Weights call in the scratch)
  WeightsDiag,  // (with diag) the weights and the diagnostics, no apply: v is only read
};
// One call of the MC guidance block, by field name; what a caller leaves out is off.
struct GuidanceCall {
  // the state the block is evaluated at, [B][dx] / [B][dy], and the velocities it reads and overwrites.
  // One-sided block (conditional sampling): dy = 0 with y, vy, my, ys null and ratio_stride = N.  The kernels take the
  // second modality's slices and column blocks from dy, so none is launched; the observed side's Gaussian factor is
  // constant in the MC index and cancels in the normalised weights.
  const float *x = nullptr, *y = nullptr;
  float *vx = nullptr, *vy = nullptr;
  const float *mx = nullptr, *my = nullptr;  // the MC set, [N][dx] / [N][dy]
  // ratios of the MC set.  ratio_stride 0: r is [N], one ratio per MC pair; ratio_stride = N (the one-sided block): r is
  // [B][N], a ratio row per sample.  pairing = PAIRING_CROSS: r is the ratio matrix [N][N] (x index first) of all pairs
  // (x1_i, y1_j), the weights stage writes one marginal weight row per modality (weights_out: x, weights_out_y: y) and
  // `scratch` is guid_cross_scratch_bytes.
  const float* r = nullptr;
  int ratio_stride = 0;
  int B = 0, N = 0, dx = 0, dy = 0;
  double t = 0.0;
  StageStrength strength{0.0};
  float* scratch = nullptr;  // the block's whole scratch: guid_scratch_bytes(B, N, pairing)
  float *weights_out = nullptr, *weights_out_y = nullptr;  // [B][N] copies of the normalised weights, or null
  // xs / ys: the state the apply stage moves, xs = xb + dt * blended; null: the blended velocity goes to vx / vy only.
  // xb / yb: the state the update starts from while the block is evaluated at x / y (second stage of a midpoint
  // step); null or x / y themselves: xs = x + dt * blended.
  float *xs = nullptr, *ys = nullptr;
  const float *xb = nullptr, *yb = nullptr;
  float dt = 0.f;
  hipStream_t stream = nullptr;
  // graph replay: the per-step scalars and the device-side step counter that picks them (pair_loop)
  const float* sched = nullptr;
  const int* step_ptr = nullptr;
  GuidDiag diag{};  // rec null: no diagnostics
  int pairing = PAIRING_PAIRED;
  GuidPhase phase = GuidPhase::All;
  // effective-sample-size floor (include/rgfm.h): ess_min > 0 swaps the weights kernel for its tempering sibling, which
  // writes the rows' exponents to tau_out [B] (or nowhere: null); 0: off.  Paired and one-sided blocks only.
  double ess_min = 0.0;
  float* tau_out = nullptr;
};

inline int guidance_launch(const GuidanceCall& c) {
  const float *x = c.x, *y = c.y, *xb = c.xb, *yb = c.yb;
  float *vx = c.vx, *vy = c.vy, *scratch = c.scratch;
  const int B = c.B, N = c.N, dx = c.dx, dy = c.dy;
  const GuidPhase phase = c.phase;
  const GuidDiag& diag = c.diag;
  hipStream_t s = c.stream;
  if (dx % 4 || dy % 4) return fail(RGFM_EINVAL, "flattened image sizes must be multiples of 4");
  if ((size_t)4 * N * sizeof(float) > 64 * 1024) return fail(RGFM_EINVAL, "n_mc too large (max 4096)");
  const bool cross = c.pairing == PAIRING_CROSS;
  if (cross && (N < 1 || N > GUID_CROSS_MAX_N || dy < 1))
    return fail(RGFM_EINVAL, "cross pairing needs two modalities and 1 <= n_mc <= %d (got %d)", GUID_CROSS_MAX_N, N);
  if (cross && c.ess_min > 0.0) return fail(RGFM_EINVAL, "the effective-sample-size floor does not go with cross pairing");
  // Python-double scalar arithmetic of the reference (sample_mnist_svhn.py:115,127,135,159,170),
  // rounded to fp32 where a tensor op consumes it.
  GuidanceArgs a{};
  a.x = x, a.y = y, a.vx = vx, a.vy = vy, a.mc_x1 = c.mx, a.mc_y1 = c.my, a.mc_ratios = c.r;
  a.ratio_stride = c.ratio_stride;
  a.B = B, a.N = N, a.dx = dx, a.dy = dy;
  guidance_scalars(c.t, &a.tf, &a.s2, &a.cden);
  a.sched = c.sched, a.step_ptr = c.sched ? c.step_ptr : nullptr;
  a.g1 = (float)(1.0 - c.strength.gamma), a.g2 = (float)c.strength.gamma;
  a.gamma_rows = c.strength.rows, a.gamma_scale = c.strength.scale;
  a.dist = reinterpret_cast<double*>(scratch), a.weights_out = c.weights_out, a.x_state = c.xs, a.y_state = c.ys, a.dt = c.dt;
  a.diag_rec = diag.rec;
  a.ess_min = (float)c.ess_min, a.tau_out = c.tau_out;
  a.x_base = xb == x ? nullptr : xb, a.y_base = yb == y ? nullptr : yb;
  a.wbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + guid_dist_bytes(B, N));
  a.wsum = reinterpret_cast<float*>(reinterpret_cast<char*>(a.wbuf) + guid_wbuf_bytes(B, N));
  if (cross) {
    float* p = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + guid_scratch_bytes(B, N));
    const size_t row = guid_wbuf_bytes(B, N) / sizeof(float), sum = guid_wsum_bytes(B) / sizeof(float);
    a.wbuf_y = p, a.wsum_y = p + row, p += row + sum;
    a.ca = p, a.cb = p + row, a.cu = p + 2 * row, a.cs = p + 3 * row, a.cq = p + 4 * row;
    a.weights_out_y = c.weights_out_y;
  }
  a.slice_len = 512;  // 512-element slices (8 x 16 x 4 = 512 workgroups at the benchmark shape) unless that needs more than RGFM_GUID_SLICES of them
  while ((dx + a.slice_len - 1) / a.slice_len + (dy + a.slice_len - 1) / a.slice_len > RGFM_GUID_SLICES) a.slice_len *= 2;
  a.nsx = (dx + a.slice_len - 1) / a.slice_len, a.nsy = (dy + a.slice_len - 1) / a.slice_len;
  // algorithmic bytes.  logp: rows of x, y and the MC set in, the sliced fp64 distances out.  apply: the
  // distances, x, y, v and the MC set in, the new state (or velocity) out.
  const double D = (double)dx + dy, dist_b = 8.0 * (a.nsx + a.nsy) * (double)B * N;
  if (phase != GuidPhase::Apply) {  // (timer class "guid_logp": the distances AND the importance weights made of them)
    ProfScope p(RGFM_KCLASS_GUID_LOGP, 4.0 * (B + N) * D + dist_b, s);
    launch_guid_logp(a, s);
    if (cross) launch_guid_cross_weights(a, s);  // (with diag: the joint ESS, the marginals' range and Z_bar too)
    else if (c.ess_min > 0.0) launch_guid_weights_ess(a, s);
    else launch_guid_weights(a, s);
  }
  if (phase != GuidPhase::Apply && diag.rec && !cross) launch_diag_wstats(a.wbuf, B, N, diag.rec, s);
  if (phase != GuidPhase::Weights && diag.rec) {  // before the real apply: in a loop that one moves the state g is taken at
    launch_diag_rownorm(vx, B, dx, diag.rec, RGFM_DIAG_V_NORM_X, s);
    if (dy) launch_diag_rownorm(vy, B, dy, diag.rec, RGFM_DIAG_V_NORM_Y, s);
    GuidanceArgs d = a;
    d.vx = diag.gx, d.vy = diag.gy, d.g1 = 0.f, d.g2 = 1.f, d.gamma_rows = nullptr;
    d.x_state = d.y_state = nullptr, d.x_base = d.y_base = nullptr, d.weights_out = nullptr;
    launch_guid_apply(d, s);
    launch_diag_rownorm(diag.gx, B, dx, diag.rec, RGFM_DIAG_G_NORM_X, s);
    if (dy) launch_diag_rownorm(diag.gy, B, dy, diag.rec, RGFM_DIAG_G_NORM_Y, s);
  }
  if (phase == GuidPhase::All || phase == GuidPhase::Apply) {
    ProfScope p(RGFM_KCLASS_GUID_APPLY, 4.0 * B * N + 4.0 * N * D + 4.0 * B * D * 3.0, s);
    launch_guid_apply(a, s);
  }
  return RGFM_OK;
}


// ================================================================== ratio estimators
// (packedh / hq: the encoders' 3x3 convs once more as two scaled fp16 planes (conv_mfma_hx2*.hip) -- the forward half of
// the gradient-guided sampler's per-step ratio pass runs on the default arithmetic of the U-Nets it guides; no bf16 image,
// no range flag of its own)
struct rgfm_ratio : WeightStore {
  rgfm_ratio_desc d;
  rgfm_ratio_flex_desc geom{};  // kind RGFM_RATIO_FLEXIBLE: the descriptor the handle was built from
  // GroupNorm(8) encoders (per-sample statistics, gn_finalize, gn_bwd) rather than folded BatchNorm ones
  bool gn_encoders() const { return d.kind != RGFM_RATIO_MNIST_SVHN; }
  int max_c = 0;       // widest conv output of either encoder (sizes the identity scale/shift scratch)
  size_t n_wtmp = 0;   // floats of `wtmp`: the largest conv weight after an encoder's first
  float* bn = nullptr;  // folded BatchNorm scale/shift pairs
  // gradient path (kind RGFM_RATIO_MNIST_SVHN): transposed weights, built at create time
  float* gradw = nullptr;  // [packed W^T of every conv after the first | fc W^T | dense W^T | zeros]
  size_t n_gradw = 0, g_zeros = 0, n_bn = 0;
  float* wtmp = nullptr;  // scratch of the transposed conv weights (kept for rgfm_ratio_update_params)
  struct Conv {
    size_t wt_pk = 0;  // packed transposed weights (offset into gradw), convs after the first
    HxImage wt_h;      // the same transposed weights as two scaled fp16 planes: the reverse pass inside the
                       // gradient-guided sampler runs on the U-Nets' default arithmetic (round 4)
    ConvW w;           // (no bf16 image; the first conv of an encoder has no packed images at all)
    size_t nw = 0, nb = 0;                 // GroupNorm weight/bias (mnist28) or BatchNorm w/b
    size_t rm = 0, rv = 0;                 // BatchNorm running stats
    size_t bn_scale = 0, bn_shift = 0;     // offsets into `bn`
    bool pool_after = false;
  };
  struct Encoder {
    int in_ch = 1, size = 32;
    std::vector<Conv> convs;
    size_t fcw = 0, fcb = 0;
    size_t fcw_t = 0;  // fc weight transposed [fc_in][F] (offset into gradw)
    int fc_in = 0;
  };
  Encoder ex, ey;
  struct Dense {
    size_t w, b, lw, lb;
    size_t w_t = 0;  // weight transposed [in][out] (offset into gradw)
    int in, out;
  };
  std::vector<Dense> hidden;
  size_t headw = 0, headb = 0;
  int head_in = 0;
  // cross evaluation (rgfm_ratio_eval_cross): the first Linear's weight [Hd][2F] as its two column slices, each a
  // contiguous [Hd][F] matrix (offsets into gradw; copied by pack_ratio, so rgfm_ratio_update_params refreshes them)
  size_t w1x = 0, w1y = 0;
};


// ================================================================== FlowMatchingModel ("--model original")
constexpr int FM_S = 28, FM_P = 49, FM_CF = 256;  // image size; 7x7 bottleneck pixels x 256 channels
struct FmPlan {  // what plan_fmnet produces: blob / packed offsets of every layer
  size_t c1w = 0, c1b = 0;           // encoder.conv1 (reference layout, conv_in kernel)
  size_t egw[4], egb[4];             // encoder.gn1..4
  ConvW ec[3];                       // encoder.conv2..4
  size_t fcw = 0, fcb = 0, fc_pk = 0;
  size_t f1w = 0, f1b = 0, f1w_pk = 0, f1b_pk = 0;
  ConvW d1, d2;                      // decoder.deconv1/2 (taps = 16 raw, packed per parity)
  size_t dgw[3], dgb[3];             // decoder.gn1..3
  ConvW c3;                          // decoder.conv3
  size_t cow = 0, cob = 0, cow_pk = 0;  // decoder.conv_out (raw; re-laid out for conv_out_kernel in `packed`)
};
struct rgfm_fmnet : WeightStore, FmPlan {  // (`packed` also holds the re-indexed Linear weights)
  rgfm_fmnet_desc d;
  float* freqs = nullptr;
};
// every derived weight image of the handle from h->params (api_fmnet.cpp; create and update_params)
int fm_pack_weights(rgfm_fmnet* h, hipStream_t s);


// ================================================================== training passes (api_train.cpp, api_ratio_train.cpp, api_fmnet_train.cpp)
// One conv on ug_igemm_kernel (unet_grad.hip): forward, data gradient, weight gradient with its ordered split-K reduce.
inline void wgrad_split(UgConv& c) {
  const int M = c.Cout, N = c.Cin * c.taps, K = c.B * c.Ho * c.Wo;
  const int base = ((M + 63) / 64) * ((N + 63) / 64);
  int splits = std::max(1, std::min((1024 + base - 1) / base, (K + 255) / 256));
  const int kps = ((K + splits - 1) / splits + 15) / 16 * 16;
  c.splits = (K + kps - 1) / kps;
  c.kps = kps;
}

inline void run_fwd(UgConv c, const float* x, float* out, const float* temb, const float* res, hipStream_t s) {
  c.x = x, c.out = out, c.temb = temb, c.res = res, c.kps = c.Cin * c.taps;
  launch_ug_conv(c, 0, s);
}
// input gradient of the conv input raster Hc x Wc into d0 (+ d1 beyond channel C0); acc: add instead of overwrite
inline void run_dgrad(UgConv c, const float* dy, float* d0, float* d1, int C0, int acc, hipStream_t s) {
  c.dy = dy, c.out = d0, c.out1 = d1, c.C0 = C0, c.acc0 = c.acc1 = acc, c.kps = c.Cout * c.taps;
  launch_ug_conv(c, 1, s);
}
inline void run_wgrad(UgConv c, const float* dy, const float* x, float* part, float* dw, float* db, hipStream_t s) {
  c.dy = dy, c.x = x, c.part = part;
  wgrad_split(c);
  launch_ug_conv(c, 2, s);
  launch_ug_reduce(part, c.splits, (size_t)c.Cout * c.Cin * c.taps, dw, s);
  launch_ug_bias_grad(dy, c.B, c.Cout, c.Ho * c.Wo, db, s);
}

// One dense layer on fg_gemm_kernel (fmnet_grad.hip): K split into ranges of kps (a multiple of 16) over gridDim.z when
// the output tile grid alone would leave the device idle (K = 12544 against a [batch][F] output); by shape only, so
// the reduction order -- partial slices added in split order -- is the same on every call.
inline void fg_split(FgGemm& g) {
  const int tiles = ((g.M + 63) / 64) * ((g.N + 63) / 64);
  const int want = std::max(1, std::min((512 + tiles - 1) / tiles, (g.K + 255) / 256));
  g.kps = ((g.K + want - 1) / want + 15) / 16 * 16;
  g.splits = (g.K + g.kps - 1) / g.kps;
}
