// Prints the U-Net plan (csrc/unet_plan.h) for tests/test_unet_plan_cpu.py.  Arguments: nine integers per descriptor --
// in_channels img_size model_channels num_levels mult0 mult1 mult2 mult3 num_res_blocks.  Per descriptor i, lines
// that begin with i:
//   total N | tensor id C S | op n kind idx in0 in1 out S block | trace C S | flops <hex float>
//   param n name offset count   (n: the op the parameter belongs to, -1 for the time MLP; name: the state_dict key of the
//                                time MLP, input conv and output head, else the key below its module)
// Host-only.
#include <cstdio>
#include <cstdlib>

#include "unet_plan.h"

static int g_desc = 0;

static void param(int op, const char* name, size_t off, size_t count) {
  printf("%d param %d %s %zu %zu\n", g_desc, op, name, off, count);
}

static void conv(int op, const char* w, const char* b, const ConvW& c) {
  param(op, w, c.w_raw, (size_t)c.cout * c.cin * c.taps);
  param(op, b, c.b, c.cout);
}

int main(int argc, char** argv) {
  static const char* kinds[] = {"IN", "RES", "DOWN", "UP", "OUT"};
  for (int a = 1; a + 8 < argc; a += 9, ++g_desc) {
    rgfm_unet_desc d{};
    d.in_channels = atoi(argv[a]), d.img_size = atoi(argv[a + 1]), d.model_channels = atoi(argv[a + 2]);
    d.num_levels = atoi(argv[a + 3]);
    for (int l = 0; l < 4; ++l) d.channel_mult[l] = atoi(argv[a + 4 + l]);
    d.num_res_blocks = atoi(argv[a + 8]);
    const UNetPlan p = plan_unet(d);
    const int i = g_desc;
    printf("%d total %zu\n", i, p.layout.n_params);
    for (size_t t = 0; t < p.tensors.size(); ++t) printf("%d tensor %zu %d %d\n", i, t, p.tensors[t].C, p.tensors[t].S);
    const size_t temb = p.temb;
    param(-1, "time_embed.0.weight", p.te0w, temb * p.mc), param(-1, "time_embed.0.bias", p.te0b, temb);
    param(-1, "time_embed.2.weight", p.te2w, temb * temb), param(-1, "time_embed.2.bias", p.te2b, temb);
    for (size_t n = 0; n < p.ops.size(); ++n) {
      const UOp& o = p.ops[n];
      printf("%d op %zu %s %d %d %d %d %d %d\n", i, n, kinds[o.kind], o.idx, o.in0, o.in1, o.out, o.S, o.block);
      const int op = (int)n;
      if (o.kind == UOP_IN) {
        param(op, "input_conv.weight", p.icw, (size_t)p.mc * d.in_channels * 9), param(op, "input_conv.bias", p.icb, p.mc);
      } else if (o.kind == UOP_RES) {
        const ResW& r = p.res[o.idx];
        param(op, "norm1.weight", r.n1w, r.cin), param(op, "norm1.bias", r.n1b, r.cin);
        conv(op, "conv1.weight", "conv1.bias", r.c1);
        param(op, "time_mlp.1.weight", r.tw, (size_t)r.cout * temb), param(op, "time_mlp.1.bias", r.tb, r.cout);
        param(op, "norm2.weight", r.n2w, r.cout), param(op, "norm2.bias", r.n2b, r.cout);
        conv(op, "conv2.weight", "conv2.bias", r.c2);
        if (r.has_skip) conv(op, "skip.weight", "skip.bias", r.sk);
      } else if (o.kind == UOP_DOWN || o.kind == UOP_UP) {
        conv(op, "conv.weight", "conv.bias", o.kind == UOP_DOWN ? p.down[o.idx] : p.up[o.idx]);
      } else {
        param(op, "out_norm.weight", p.onw, p.final_ch), param(op, "out_norm.bias", p.onb, p.final_ch);
        param(op, "out_conv.weight", p.ocw, (size_t)d.in_channels * p.final_ch * 9);
        param(op, "out_conv.bias", p.ocb, d.in_channels);
      }
    }
    for (const UTensor& t : unet_trace_table(p)) printf("%d trace %d %d\n", i, t.C, t.S);
    printf("%d flops %a\n", i, unet_row_flops(p));
  }
  return 0;
}
