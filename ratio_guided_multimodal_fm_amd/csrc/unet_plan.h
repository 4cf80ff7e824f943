// unet_plan.h -- the weight-plan types every handle's plan is made of, and the plan of the U-Net handle: parameter
// offsets, weight images and the op list of FlexibleUNet.forward.  plan_unet is the only place that runs the level nest
// and the skip stack; the inference walk (UNetRun::run), the training plan (plan_train), the trace table and the
// per-row FLOPs read its op list.  Plain C++ (no HIP types): tests/test_unet_plan_cpu.py compiles it alone into a host
// program.
#pragma once
#include "../../include/rgfm.h"

#include <cstddef>
#include <vector>

struct Cursor {
  size_t off = 0;
  size_t take(size_t n) {
    const size_t r = off;
    off += n;
    return r;
  }
};

// One two-plane fp16 weight image (conv_mfma_hx2*.hip) of a conv.
struct HxImage {
  size_t off = 0;        // offset (fp16 elements) into the packedh buffer
  int hq = 0;            // index of its scale record {q, 1/q, s_w, eligible} in the hq array
  bool present = false;  // the plan carved it
  bool ok = false;       // weights inside the fp16 path's range (read_hx_flags, after packing)
  bool usable() const { return present && ok; }
};

struct ConvW {  // one packed conv
  size_t w_raw = 0, b = 0;  // offsets into the params blob
  size_t w_pk = 0;          // offset into the packed buffer
  size_t w_bx3 = 0;         // offset (bf16 elements) into the 3-plane bf16 buffer of conv_mfma_bx3.hip
  int cin = 0, cout = 0, taps = 9;
  HxImage hx;    // the image every conv has, in the order of its mode (stride-2 convs: phase-major)
  HxImage hx9;   // stride-2 convs once more in plain nine-tap order (conv_mfma_hx2s.hip): same weights, hx's scale record
  HxImage wino;  // ResBlock convs with Cout % 64 == 0 once more as Winograd F(2x2, 3x3) images (conv_mfma_hx2w.hip)
  // Upsample convs (nearest x 2, then 3x3: unet_flexible.py:107-108) once more as the EQUIVALENT ConvTranspose2d(4, 2, 1)
  // -- four 2x2-tap parity classes over the INPUT raster, 16 instead of 36 tap products per input pixel (launch_up2_as_deconv)
  HxImage t2;
};

// What a plan hands to the weight store: element counts of the buffers every handle owns.
struct WeightLayout {
  size_t n_params = 0, n_packed = 0, n_packed3 = 0, n_packedh = 0;
  int n_hq = 0;
};

// The cursors of one plan: the state_dict-order blob, the fp32-packed, bf16 and fp16 buffers and the scale records.
struct Planner {
  Cursor raw, pk, p3, ph;
  int nhq = 0;
  // a two-plane image of n_fp16 elements; `same_scale`: an image of the same weights, whose scale record this one shares
  HxImage image(size_t n_fp16, const HxImage* same_scale = nullptr) {
    HxImage i;
    i.off = ph.take(n_fp16), i.hq = same_scale ? same_scale->hq : nhq++, i.present = true;
    return i;
  }
  ConvW conv(int cin, int cout, int taps) {
    ConvW w;
    w.cin = cin, w.cout = cout, w.taps = taps;
    w.w_raw = raw.take((size_t)cout * cin * taps);
    w.b = raw.take(cout);
    w.w_pk = pk.take((size_t)cout * cin * taps);
    w.w_bx3 = p3.take((size_t)cout * cin * taps * 3);
    w.hx = image((size_t)cout * cin * taps * 2);
    return w;
  }
  WeightLayout layout() const { return {raw.off, pk.off, p3.off, ph.off, nhq}; }
};

struct ResW {
  int cin = 0, cout = 0;
  size_t n1w, n1b, n2w, n2b, tw, tb;
  ConvW c1, c2, sk;
  bool has_skip = false;
  int temb_off = 0;
};


// ================================================================== U-Net plan
constexpr int UNET_KC = 16;  // the conv kernels' K chunk (KC of rgfm_kernels.h; rgfm_host.h asserts the two agree)

struct UTensor {  // a map the forward produces: channels, square size
  int C, S;
};

enum { UOP_IN, UOP_RES, UOP_DOWN, UOP_UP, UOP_OUT };

struct UOp {  // one step of FlexibleUNet.forward
  int kind;
  int idx = -1;    // RES: into UNetPlan::res; DOWN / UP: into down / up
  int in0 = -1, in1 = -1, out = -1;  // tensor ids, -1: none (in1: the skip a decoder block pops; OUT writes the caller's v)
  int S = 0;       // spatial size of the input
  int block = -1;  // ResBlock number in walk order (the dropout mask's block id)
};

struct UNetPlan {
  int in_channels = 0, mc = 0, temb = 0, final_ch = 0, temb_total = 0;
  size_t te0w = 0, te0b = 0, te2w = 0, te2b = 0, icw = 0, icb = 0, onw = 0, onb = 0, ocw = 0, ocb = 0;
  size_t ocw_pk = 0;  // out_conv weights re-laid out for conv_out_kernel (offset into `packed`)
  WeightLayout layout;
  std::vector<ResW> res;  // every ResBlock in forward order (= registration order: encoder, middle, decoder)
  std::vector<ConvW> down, up;
  std::vector<UTensor> tensors;
  std::vector<UOp> ops;  // forward order
};

// FlexibleUNet.forward (reference src/models/unet_flexible.py:203-261) as an op list, and the blob offsets of every
// parameter in the registration order of FlexibleUNet.__init__ (unet_flexible.py:146-201; UNetMNIST, src/models/unet.py:
// 155-214, is identical): the encoder blocks, the Downsample convs, the middle blocks, the decoder blocks, the Upsample
// convs.  The ResBlocks are registered in the order the forward runs them, the Downsample / Upsample convs behind the
// blocks of their half: those are carved from the ops once their half is listed.
inline UNetPlan plan_unet(const rgfm_unet_desc& d) {
  UNetPlan p;
  Planner P;
  Cursor& c = P.raw;
  const int mc = d.model_channels, temb = 4 * mc;
  p.in_channels = d.in_channels, p.mc = mc, p.temb = temb;
  auto emit = [&](int kind, int idx, int in0, int in1, int C, int So) {
    UOp o{kind};
    o.idx = idx, o.in0 = in0, o.in1 = in1, o.S = in0 >= 0 ? p.tensors[in0].S : So;
    if (kind == UOP_RES) o.block = idx;
    if (kind != UOP_OUT) p.tensors.push_back({C, So}), o.out = (int)p.tensors.size() - 1;
    p.ops.push_back(o);
    return o.out;
  };
  auto res = [&](int a, int b, int cout) {  // a ResBlock on tensor a (+ the popped skip b)
    ResW r;
    const int cin = p.tensors[a].C + (b >= 0 ? p.tensors[b].C : 0);
    r.cin = cin, r.cout = cout;
    r.n1w = c.take(cin), r.n1b = c.take(cin);
    r.c1 = P.conv(cin, cout, 9);
    r.tw = c.take((size_t)cout * temb), r.tb = c.take(cout);
    r.n2w = c.take(cout), r.n2b = c.take(cout);
    r.c2 = P.conv(cout, cout, 9);
    if (cout % 64 == 0 && cin % UNET_KC == 0) {  // the Winograd images (16 positions instead of 9 taps)
      r.c1.wino = P.image((size_t)cout * cin * 16 * 2);
      r.c2.wino = P.image((size_t)cout * cout * 16 * 2);
    }
    r.has_skip = cin != cout;
    if (r.has_skip) r.sk = P.conv(cin, cout, 1);
    r.temb_off = p.temb_total;
    p.temb_total += cout;
    p.res.push_back(r);
    return emit(UOP_RES, (int)p.res.size() - 1, a, b, cout, p.tensors[a].S);
  };
  p.te0w = c.take((size_t)temb * mc), p.te0b = c.take(temb);
  p.te2w = c.take((size_t)temb * temb), p.te2b = c.take(temb);
  p.icw = c.take((size_t)mc * d.in_channels * 9), p.icb = c.take(mc);
  int cur = emit(UOP_IN, -1, -1, -1, mc, d.img_size), ndown = 0, nup = 0;
  std::vector<int> skips{cur};
  for (int l = 0; l < d.num_levels; ++l) {
    for (int r = 0; r < d.num_res_blocks; ++r) skips.push_back(cur = res(cur, -1, mc * d.channel_mult[l]));
    if (l < d.num_levels - 1)
      skips.push_back(cur = emit(UOP_DOWN, ndown++, cur, -1, p.tensors[cur].C, p.tensors[cur].S / 2));
  }
  for (const UOp& o : p.ops)
    if (o.kind == UOP_DOWN) {
      const int dc = p.tensors[o.in0].C;
      ConvW w = P.conv(dc, dc, 9);
      w.hx9 = P.image((size_t)dc * dc * 9 * 2, &w.hx);  // (the Downsample convs twice: phase-major and plain)
      p.down.push_back(w);
    }
  cur = res(cur, -1, p.tensors[cur].C);
  cur = res(cur, -1, p.tensors[cur].C);
  for (int l = d.num_levels - 1; l >= 0; --l) {
    for (int i = 0; i < d.num_res_blocks + 1; ++i) {
      cur = res(cur, skips.back(), mc * d.channel_mult[l]);
      skips.pop_back();
    }
    if (l > 0) cur = emit(UOP_UP, nup++, cur, -1, p.tensors[cur].C, p.tensors[cur].S * 2);
  }
  for (const UOp& o : p.ops)
    if (o.kind == UOP_UP) {
      const int uc = p.tensors[o.in0].C;
      ConvW w = P.conv(uc, uc, 9);
      w.t2 = P.image((size_t)uc * uc * 16 * 2);  // (the Upsample convs twice: nine taps, and the parity-class form)
      p.up.push_back(w);
    }
  const int ch = p.final_ch = p.tensors[cur].C;
  p.onw = c.take(ch), p.onb = c.take(ch);
  p.ocw = c.take((size_t)d.in_channels * ch * 9), p.ocb = c.take(d.in_channels);
  p.ocw_pk = P.pk.take((size_t)d.in_channels * ch * 9);
  emit(UOP_OUT, -1, cur, -1, 0, 0);
  p.layout = P.layout();
  return p;
}

// The (C, S) table of the trace hooks, in the order a traced forward records: the input conv's map; per ResBlock conv1 +
// the time term, then the block's output; every Downsample / Upsample output; the velocity last.
inline std::vector<UTensor> unet_trace_table(const UNetPlan& p) {
  std::vector<UTensor> t;
  for (const UOp& o : p.ops) {
    if (o.kind == UOP_OUT) t.push_back({p.in_channels, o.S});
    else t.push_back(p.tensors[o.out]);
    if (o.kind == UOP_RES) t.push_back(p.tensors[o.out]);
  }
  return t;
}

// Conv FLOPs of one evaluation of one row (what paces the MC pre-phase: two_loop, api_sampler.cpp).
inline double unet_row_flops(const UNetPlan& p) {
  const int S0 = p.ops.front().S;
  double f = 2.0 * S0 * S0 * 9.0 * p.in_channels * (p.mc + p.final_ch);
  for (const UOp& o : p.ops) {
    if (o.kind == UOP_RES) {
      const ResW& r = p.res[o.idx];
      f += 2.0 * o.S * o.S * r.cout * (9.0 * r.cin + 9.0 * r.cout + (r.has_skip ? r.cin : 0));
    } else if (o.kind == UOP_DOWN || o.kind == UOP_UP) {
      const ConvW& w = o.kind == UOP_DOWN ? p.down[o.idx] : p.up[o.idx];
      const int So = p.tensors[o.out].S;
      f += 2.0 * So * So * 9.0 * w.cin * w.cout;
    }
  }
  return f;
}
