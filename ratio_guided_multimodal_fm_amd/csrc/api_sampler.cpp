// api_sampler.cpp -- the Euler / midpoint samplers over U-Net handles and the stand-alone guidance block (C ABI: include/rgfm.h).
#include "sampler_host.h"

// ================================================================== samplers
// Every loop below is shared by its Euler entry point (the `solver` = RGFM_SOLVER_EULER case) and its *_ode twin.  A loop
// is: check_loop, its carve over the caller's workspace (the same function, run dry, is its *_workspace_bytes), a
// NetChain per U-Net, and the stages of the call from for_each_stage (sampler_stages.h).  A guided loop takes its own
// operands and the call's LoopCall record, which its extern "C" wrapper fills by field name.
namespace {

// ---- carves: each loop's buffers, in the order they lie in its workspace
void carve_single(Bump& b, NetChain& c) {
  c.carve(b);
  c.carve_eval();
}

struct CondWs {
  NetChain c;
  float *v, *scratch;
};
CondWs carve_cond(Bump& b, rgfm_unet* h, int batch, int n_mc, int solver) {
  CondWs w{{h, batch, solver}, nullptr, nullptr};
  w.c.carve(b);
  w.v = b.f((size_t)batch * w.c.image_floats());
  w.scratch = b.f(guid_scratch_bytes(batch, n_mc) / sizeof(float));
  w.c.carve_eval();
  return w;
}

struct PairWs {
  NetChain cx, cy;
  float *vx, *vy, *scratch, *gstate;
};
void carve_pair(Bump& b, PairWs& w, int n_mc, int pairing) {
  const int batch = w.cx.batch;
  w.cx.carve(b), w.cy.carve(b);
  w.vx = b.f((size_t)batch * w.cx.image_floats());
  w.vy = b.f((size_t)batch * w.cy.image_floats());
  w.scratch = b.f(guid_scratch_bytes(batch, n_mc, pairing) / sizeof(float));
  w.gstate = b.f(64 + (size_t)TABLE_ROWS * 4);  // step counter + per-step guidance scalars (graph replay)
  w.cx.carve_eval(), w.cy.carve_eval();         // the two nets run concurrently: disjoint regions
}

int single_bytes(const rgfm_unet* h, int batch, int solver, size_t* bytes, bool cfg = false) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!h || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  Bump b;
  NetChain c{const_cast<rgfm_unet*>(h), batch, solver};
  c.cfg_ws = cfg;
  carve_single(b, c);
  *bytes = b.off;
  return RGFM_OK;
}

// The labels and scale of a *_cfg entry point (include/rgfm.h, "Class conditioning"); the other entry points pass none.
struct Cfg {
  bool on = false;
  const int* labels = nullptr;
  double scale = 1.0;
};

int single_loop(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin, int step_end, int solver, void* ws,
                size_t ws_bytes, rgfm_stream_t stream, Sde sde = Sde(), Cfg cfg = Cfg()) {
  refresh_modes();
  int ns = 0;
  if (int rc = check_loop(solver, h && x_inout && ws, batch, num_steps, step_begin, step_end, &ns)) return rc;
  if (int rc = sde.check(solver)) return rc;
  Bump b(ws, ws_bytes);
  NetChain c{h, batch, solver, x_inout};
  if (cfg.on)
    if (int rc = c.check_cfg(cfg.labels, cfg.scale, ns)) return rc;
  carve_single(b, c);
  if (sde.on()) sde.carve(b, batch, c.image_floats(), 0);
  if (int rc = check_workspace(b, ws_bytes)) return rc;
  if (ns == 0) return RGFM_OK;
  if (int rc = c.begin((hipStream_t)stream, num_steps, step_begin, ns)) return rc;
  for (int i = 0; i < ns; ++i)
    if (int rc = c.step(i, sde)) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

// ---- two unguided integrations at once (the MC pre-phase of the paired sampler)
// The workspace: the first net's single-loop layout, then the second's (its size: the sum of the two single sizes).
// The two chains are independent and carry unequal work (the benchmark's pair: 1 : 2.8).  x runs on the caller's stream,
// y on the device's side stream, forked from and joined back into the caller's.  Enqueued one whole chain after the
// other, the second chain starts only when the host has got through the first one's launches, and from then on the two
// drift: whichever ends first leaves the other alone on the chip, with nothing to cover its launch heads and tails and
// its small grids.  So ("MC pre-phase") the chains are enqueued step by step, and step i + 1 of the lighter
// chain -- by conv FLOPs per step x rows, from the descriptors -- waits for step i of the heavier one (hipStreamWaitEvent,
// no host synchronisation): every step of the heavier chain has the lighter chain's step beside it, as a step of the
// guided loop has, and both end within a step of each other.  Chains of equal work are not paced.
// RGFM_PREPHASE_PRIO=0: the earlier schedule.  Same launches and arguments per chain either way: a row's bits do not
// depend on the schedule.
int two_loop(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, int batch_x, int batch_y, int num_steps,
             int step_begin, int step_end, int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream, Cfg cfg_x = Cfg(),
             Cfg cfg_y = Cfg()) {
  refresh_modes();
  int ns = 0;
  if (int rc = check_loop(solver, hx && hy && x_inout && y_inout && ws, batch_x, num_steps, step_begin, step_end, &ns))
    return rc;
  if (x_inout == y_inout) return fail(RGFM_EINVAL, "the two states must be different buffers");
  if (batch_y < 1) return fail(RGFM_EINVAL, "bad argument");
  Bump b(ws, ws_bytes);
  // each net's chain is cut into steps so that the two can be enqueued side by side
  NetChain cx{hx, batch_x, solver, x_inout}, cy{hy, batch_y, solver, y_inout};
  if (cfg_x.on)
    if (int rc = cx.check_cfg(cfg_x.labels, cfg_x.scale, ns)) return rc;
  if (cfg_y.on)
    if (int rc = cy.check_cfg(cfg_y.labels, cfg_y.scale, ns)) return rc;
  carve_single(b, cx), carve_single(b, cy);
  if (int rc = check_workspace(b, ws_bytes)) return rc;
  if (ns == 0) return RGFM_OK;
  DevState* ds = cur_dev();
  if (!ds) return fail(RGFM_EINVAL, "no handle has been created on the current device");
  hipStream_t caller = (hipStream_t)stream;
  const bool overlap = g_modes.overlap;  // (RGFM_OVERLAP=0: both chains on the caller's stream)
  // (conv FLOPs of one evaluation of one row, from each plan's op list: unet_plan.h)
  const double wx = unet_row_flops(*hx) * batch_x, wy = unet_row_flops(*hy) * batch_y;
  hipStream_t sy = overlap ? ds->side : caller;
  NetChain &lng = wx > wy ? cx : cy, &sht = wx > wy ? cy : cx;
  // Whatever has been enqueued on the side stream must be joined into the caller's on every exit path.
  struct Join {
    DevState* ds;
    hipStream_t caller, side;
    ~Join() {
      if (side != caller) (void)hipEventRecord(ds->join, side), (void)hipStreamWaitEvent(caller, ds->join, 0);
    }
  } join{ds, caller, sy};
  if (overlap) {
    HIP_TRY(hipEventRecord(ds->fork, caller));
    HIP_TRY(hipStreamWaitEvent(sy, ds->fork, 0));
  }
  if (int rc = cx.begin(caller, num_steps, step_begin, ns)) return rc;
  if (int rc = cy.begin(sy, num_steps, step_begin, ns)) return rc;
  if (!overlap || !g_modes.prephase) {  // the earlier order: the second net's whole chain, then the first's
    for (NetChain* c : {&cy, &cx})
      for (int i = 0; i < ns; ++i)
        if (int rc = c->step(i)) return rc;
  } else {
    const bool pace = wx != wy;
    for (int i = 0; i < ns; ++i) {
      if (int rc = lng.step(i)) return rc;
      if (pace && i + 1 < ns) HIP_TRY(hipEventRecord(ds->pre_pace, lng.s));
      if (int rc = sht.step(i)) return rc;
      if (pace && i + 1 < ns) HIP_TRY(hipStreamWaitEvent(sht.s, ds->pre_pace, 0));
    }
  }
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

}  // namespace

extern "C" int rgfm_sample_two_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch_x, int batch_y, int solver,
                                               size_t* bytes) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!hx || !hy || !bytes || batch_x < 1 || batch_y < 1) return fail(RGFM_EINVAL, "bad argument");
  Bump b;
  NetChain cx{const_cast<rgfm_unet*>(hx), batch_x, solver}, cy{const_cast<rgfm_unet*>(hy), batch_y, solver};
  carve_single(b, cx), carve_single(b, cy);
  *bytes = b.off;
  return RGFM_OK;
}
extern "C" int rgfm_sample_two(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, int batch_x, int batch_y,
                               int num_steps, int step_begin, int step_end, int solver, void* ws, size_t ws_bytes,
                               rgfm_stream_t stream) {
  return two_loop(hx, hy, x_inout, y_inout, batch_x, batch_y, num_steps, step_begin, step_end, solver, ws, ws_bytes, stream);
}

extern "C" int rgfm_sample_single_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes) {
  return single_bytes(h, batch, SOLVER_EULER, bytes);
}
extern "C" int rgfm_sample_single_ode_workspace_bytes(const rgfm_unet* h, int batch, int solver, size_t* bytes) {
  return single_bytes(h, batch, solver, bytes);
}
extern "C" int rgfm_sample_single(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin,
                                  int step_end, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return single_loop(h, x_inout, batch, num_steps, step_begin, step_end, SOLVER_EULER, ws, ws_bytes, stream);
}
extern "C" int rgfm_sample_single_ode(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin, int step_end,
                                      int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return single_loop(h, x_inout, batch, num_steps, step_begin, step_end, solver, ws, ws_bytes, stream);
}

extern "C" int rgfm_guidance_workspace_bytes(int batch, int n_mc, size_t* bytes) {
  if (!bytes || batch < 1 || n_mc < 1) return fail(RGFM_EINVAL, "bad argument");
  *bytes = guid_scratch_bytes(batch, n_mc);
  return RGFM_OK;
}

// (the blocks below: `gamma` is the scalar of the existing entry points, or the per-row vector of their *_rows twins)
namespace {
int guidance_block(const float* x, const float* y, float* vx, float* vy, const float* mc_x1, const float* mc_y1,
                   const float* mc_ratios, int batch, int n_mc, int dim_x, int dim_y, double t, const StageStrength& gamma,
                   float* weights_out, void* ws, size_t ws_bytes, rgfm_stream_t stream, double ess_min = 0.0,
                   float* tau_out = nullptr) {
  if (!x || !y || !vx || !vy || !mc_x1 || !mc_y1 || !mc_ratios || !ws) return fail(RGFM_EINVAL, "null argument");
  size_t need = 0;
  int rc = rgfm_guidance_workspace_bytes(batch, n_mc, &need);
  if (rc) return rc;
  if (!(ess_min <= 0.0) && (rc = Ess::check_min(ess_min, n_mc))) return rc;  // (<= 0: off, the *_rows block)
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if ((rc = ensure_init())) return rc;
  rc = guidance_launch({.x = x, .y = y, .vx = vx, .vy = vy, .mx = mc_x1, .my = mc_y1, .r = mc_ratios, .B = batch, .N = n_mc,
                        .dx = dim_x, .dy = dim_y, .t = t, .strength = gamma, .scratch = (float*)ws,
                        .weights_out = weights_out, .stream = (hipStream_t)stream, .ess_min = ess_min, .tau_out = tau_out});
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

// The one-sided block: the paired block with dy = 0 and a ratio row per sample (GuidanceCall).
int guidance_block_cond(const float* s, float* v, const float* mc_set, const float* ratios, int batch, int n_mc, int dim,
                        double t, const StageStrength& gamma, float* weights_out, void* ws, size_t ws_bytes,
                        rgfm_stream_t stream, double ess_min = 0.0, float* tau_out = nullptr) {
  if (!s || !v || !mc_set || !ratios || !ws) return fail(RGFM_EINVAL, "null argument");
  if (dim < 1) return fail(RGFM_EINVAL, "bad argument");
  size_t need = 0;
  int rc = rgfm_guidance_workspace_bytes(batch, n_mc, &need);
  if (rc) return rc;
  if (!(ess_min <= 0.0) && (rc = Ess::check_min(ess_min, n_mc))) return rc;  // (<= 0: off, the *_rows block)
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if ((rc = ensure_init())) return rc;
  rc = guidance_launch({.x = s, .vx = v, .mx = mc_set, .r = ratios, .ratio_stride = n_mc, .B = batch, .N = n_mc, .dx = dim,
                        .t = t, .strength = gamma, .scratch = (float*)ws, .weights_out = weights_out,
                        .stream = (hipStream_t)stream, .ess_min = ess_min, .tau_out = tau_out});
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
}  // namespace

extern "C" int rgfm_guidance_apply(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                                   const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x,
                                   int dim_y, double t, double gamma, float* weights_out, void* ws,
                                   size_t ws_bytes, rgfm_stream_t stream) {
  return guidance_block(x, y, vx, vy, mc_x1, mc_y1, mc_ratios, batch, n_mc, dim_x, dim_y, t, gamma, weights_out, ws, ws_bytes,
                        stream);
}
extern "C" int rgfm_guidance_apply_cond(const float* s, float* v, const float* mc_set, const float* ratios, int batch, int n_mc,
                                        int dim, double t, double gamma, float* weights_out, void* ws, size_t ws_bytes,
                                        rgfm_stream_t stream) {
  return guidance_block_cond(s, v, mc_set, ratios, batch, n_mc, dim, t, gamma, weights_out, ws, ws_bytes, stream);
}
// ... with a strength per row (include/rgfm.h, "Guidance strength per sample and per stage")
extern "C" int rgfm_guidance_apply_rows(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                                        const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x, int dim_y,
                                        double t, const float* gamma_rows, float* weights_out, void* ws, size_t ws_bytes,
                                        rgfm_stream_t stream) {
  if (!gamma_rows) return fail(RGFM_EINVAL, "null argument");
  return guidance_block(x, y, vx, vy, mc_x1, mc_y1, mc_ratios, batch, n_mc, dim_x, dim_y, t, StageStrength(0.0, gamma_rows, 1.0),
                        weights_out, ws, ws_bytes, stream);
}
extern "C" int rgfm_guidance_apply_cond_rows(const float* s, float* v, const float* mc_set, const float* ratios, int batch,
                                             int n_mc, int dim, double t, const float* gamma_rows, float* weights_out, void* ws,
                                             size_t ws_bytes, rgfm_stream_t stream) {
  if (!gamma_rows) return fail(RGFM_EINVAL, "null argument");
  return guidance_block_cond(s, v, mc_set, ratios, batch, n_mc, dim, t, StageStrength(0.0, gamma_rows, 1.0), weights_out, ws,
                             ws_bytes, stream);
}
// ... held to an effective-sample-size floor (include/rgfm.h, "Effective-sample-size floor"): the *_rows blocks plus
// (ess_min, tau_out); ess_min 0 is the *_rows block itself
extern "C" int rgfm_guidance_apply_ess(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                                       const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x, int dim_y,
                                       double t, const float* gamma_rows, float* weights_out, double ess_min, float* tau_out,
                                       void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!gamma_rows) return fail(RGFM_EINVAL, "null argument");
  return guidance_block(x, y, vx, vy, mc_x1, mc_y1, mc_ratios, batch, n_mc, dim_x, dim_y, t, StageStrength(0.0, gamma_rows, 1.0),
                        weights_out, ws, ws_bytes, stream, ess_min, tau_out);
}
extern "C" int rgfm_guidance_apply_cond_ess(const float* s, float* v, const float* mc_set, const float* ratios, int batch,
                                            int n_mc, int dim, double t, const float* gamma_rows, float* weights_out,
                                            double ess_min, float* tau_out, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!gamma_rows) return fail(RGFM_EINVAL, "null argument");
  return guidance_block_cond(s, v, mc_set, ratios, batch, n_mc, dim, t, StageStrength(0.0, gamma_rows, 1.0), weights_out, ws,
                             ws_bytes, stream, ess_min, tau_out);
}

// ---- diagnostics of one evaluation of the block (include/rgfm.h, "Guidance diagnostics")
// workspace: the block's, then the two scratch velocities of GuidDiag
namespace {
// `c`: the block's inputs by name (state, MC set, ratios, shape, t, stream, pairing); v is only read
int guidance_diag(GuidanceCall c, const float* vx, const float* vy, float* diag_out, void* ws, size_t ws_bytes) {
  size_t need = 0;
  int rc = c.pairing == PAIRING_CROSS ? rgfm_guidance_cross_workspace_bytes(c.B, c.N, c.dx, c.dy, &need)
                                      : rgfm_guidance_diag_workspace_bytes(c.B, c.N, c.dx, c.dy, &need);
  if (rc) return rc;
  if (c.N > 4096) return fail(RGFM_EINVAL, "n_mc too large (max 4096)");
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if ((rc = ensure_init())) return rc;
  Bump b(ws, ws_bytes);
  c.scratch = b.f(guid_scratch_bytes(c.B, c.N, c.pairing) / sizeof(float));
  DiagSink sink;
  if ((rc = sink.check(diag_out, (size_t)c.B, c.B, 1, SOLVER_EULER))) return rc;
  sink.carve(b, c.dx, c.dy);
  if ((rc = sink.begin(c.stream, c.dx, c.dy))) return rc;
  // (WeightsDiag reads v and writes none of the block's outputs: the casts drop a const that is kept)
  c.vx = const_cast<float*>(vx), c.vy = const_cast<float*>(vy);
  c.diag = sink.at(0), c.phase = GuidPhase::WeightsDiag;  // (one evaluation, one record)
  if ((rc = guidance_launch(c))) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
}  // namespace

extern "C" int rgfm_guidance_diag_workspace_bytes(int batch, int n_mc, int dim_x, int dim_y, size_t* bytes) {
  if (!bytes || batch < 1 || n_mc < 1 || dim_x < 1 || dim_y < 0) return fail(RGFM_EINVAL, "bad argument");
  if (dim_x % 4 || dim_y % 4) return fail(RGFM_EINVAL, "flattened image sizes must be multiples of 4");
  *bytes = guid_scratch_bytes(batch, n_mc) + diag_scratch_bytes(batch, dim_x, dim_y);
  return RGFM_OK;
}
extern "C" int rgfm_guidance_diag(const float* x, const float* y, const float* vx, const float* vy, const float* mc_x1,
                                  const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x, int dim_y,
                                  double t, float* diag_out, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!x || !y || !vx || !vy || !mc_x1 || !mc_y1 || !mc_ratios || !diag_out || !ws) return fail(RGFM_EINVAL, "null argument");
  if (dim_y < 1) return fail(RGFM_EINVAL, "bad argument");
  return guidance_diag({.x = x, .y = y, .mx = mc_x1, .my = mc_y1, .r = mc_ratios, .B = batch, .N = n_mc, .dx = dim_x, .dy = dim_y,
                        .t = t, .stream = (hipStream_t)stream},
                       vx, vy, diag_out, ws, ws_bytes);
}
extern "C" int rgfm_guidance_diag_cond(const float* s, const float* v, const float* mc_set, const float* ratios, int batch,
                                       int n_mc, int dim, double t, float* diag_out, void* ws, size_t ws_bytes,
                                       rgfm_stream_t stream) {
  if (!s || !v || !mc_set || !ratios || !diag_out || !ws) return fail(RGFM_EINVAL, "null argument");
  const float* no_vy = nullptr;  // (the one-sided block: GuidanceCall)
  return guidance_diag({.x = s, .mx = mc_set, .r = ratios, .ratio_stride = n_mc, .B = batch, .N = n_mc, .dx = dim, .t = t,
                        .stream = (hipStream_t)stream},
                       v, no_vy, diag_out, ws, ws_bytes);
}

namespace {

int cond_bytes(const rgfm_unet* h, int batch, int n_mc, int solver, size_t* bytes, bool diag = false) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!h || !bytes || batch < 1 || n_mc < 1) return fail(RGFM_EINVAL, "bad argument");
  Bump b;
  const CondWs w = carve_cond(b, const_cast<rgfm_unet*>(h), batch, n_mc, solver);
  *bytes = b.off + (diag ? diag_scratch_bytes(batch, w.c.image_floats(), 0) : 0);
  return RGFM_OK;
}

// One net, guided by the one-sided block: kernel by kernel on the caller's stream (nothing to overlap, no graph).
int cond_loop(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, const LoopCall& c) {
  int ns = 0;
  DiagSink sink;
  if (int rc = open_loop(c, h && s_inout && mc_set && ratios, &ns, &sink)) return rc;
  if (n_mc < 1) return fail(RGFM_EINVAL, "conditional sampling needs an MC set (n_mc >= 1)");
  const int d = h->d.in_channels * h->d.img_size * h->d.img_size;
  if (d % 4) return fail(RGFM_EINVAL, "flattened image sizes must be multiples of 4");
  if (n_mc > 4096) return fail(RGFM_EINVAL, "n_mc too large (max 4096)");
  if (int rc = c.ess.check(n_mc, loop_stages(c.solver, ns), c.batch)) return rc;
  Bump b(c.ws, c.ws_bytes);
  CondWs w = carve_cond(b, h, c.batch, n_mc, c.solver);
  if (sink.on()) sink.carve(b, d, 0);
  Sde sde = c.sde;
  if (sde.on()) sde.carve(b, c.batch, d, 0);
  if (int rc = check_workspace(b, c.ws_bytes)) return rc;
  if (ns == 0) return RGFM_OK;
  hipStream_t s = (hipStream_t)c.stream;
  if (int rc = w.c.begin(s, c.num_steps, c.step_begin, ns)) return rc;
  if (sink.on())
    if (int rc = sink.begin(s, d, 0)) return rc;
  if (int rc = c.ess.begin(s, loop_stages(c.solver, ns), c.batch)) return rc;
  // one stage: out = s + F(in, t) dts; guided iff the stage's own t > eps (`t > eps` test of the reference, :124)
  // and its scale is not 0
  auto stage = [&](const Stage& g) -> int {
    float *in = g.reads_mid ? w.c.mid : s_inout, *out = g.writes_mid ? w.c.mid : s_inout;
    const float* base = nullptr;
    float dts = 0.f;
    if (int rc = sde.stage(g, c.num_steps, 0, s_inout, (size_t)c.batch * d, s, s_inout, &base, &dts)) return rc;
    // unguided: the fused Euler epilogue
    if (g.t <= 1e-3 || c.strength.off(g.row)) return w.c.eval(g.row, s, in, nullptr, out, base, dts);
    // guided: the raw velocity, and the (one-sided) guidance block moves the state
    if (int rc = w.c.eval(g.row, s, in, w.v, nullptr, nullptr, dts)) return rc;
    return guidance_launch({.x = in, .vx = w.v, .mx = mc_set, .r = ratios, .ratio_stride = n_mc, .B = c.batch, .N = n_mc,
                            .dx = d, .t = g.t, .strength = c.strength.stage(g.row), .scratch = w.scratch, .xs = out,
                            .xb = base, .dt = dts, .stream = s, .diag = sink.at(g.row), .ess_min = c.ess.floor(),
                            .tau_out = c.ess.at(g.row, c.batch)});
  };
  if (int rc = for_each_stage(c.solver, c.num_steps, c.step_begin, ns, stage)) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

int pair_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver, size_t* bytes, bool diag = false,
               int pairing = PAIRING_PAIRED) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!hx || !hy || !bytes || batch < 1 || n_mc < 0) return fail(RGFM_EINVAL, "bad argument");
  Bump b;
  PairWs w{{const_cast<rgfm_unet*>(hx), batch, solver}, {const_cast<rgfm_unet*>(hy), batch, solver}};
  carve_pair(b, w, n_mc, pairing);
  *bytes = b.off + (diag ? diag_scratch_bytes(batch, w.cx.image_floats(), w.cy.image_floats()) : 0);
  return RGFM_OK;
}

int pair_sample(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1, const float* mc_y1,
                const float* mc_ratios, int n_mc, const LoopCall& c) {
  int ns = 0;
  DiagSink sink;
  if (int rc = open_loop(c, hx && hy && x_inout && y_inout, &ns, &sink)) return rc;
  if (n_mc < 0 || (n_mc > 0 && (!mc_x1 || !mc_y1 || !mc_ratios))) return fail(RGFM_EINVAL, "MC set missing");
  if (c.ess.on() && c.pairing == PAIRING_CROSS) return fail(RGFM_EINVAL, "the effective-sample-size floor does not go with cross pairing");
  if (int rc = c.ess.check(n_mc, loop_stages(c.solver, ns), c.batch)) return rc;
  if (c.pairing == PAIRING_CROSS) {  // (what guidance_launch would refuse at the first guided stage, before anything is enqueued)
    if (n_mc > GUID_CROSS_MAX_N) return fail(RGFM_EINVAL, "cross pairing: n_mc %d too large (max %d)", n_mc, GUID_CROSS_MAX_N);
    for (const rgfm_unet* h : {hx, hy})
      if ((h->d.in_channels * h->d.img_size * h->d.img_size) % 4) return fail(RGFM_EINVAL, "flattened image sizes must be multiples of 4");
  }
  Bump b(c.ws, c.ws_bytes);
  PairWs w{{hx, c.batch, c.solver}, {hy, c.batch, c.solver}};
  carve_pair(b, w, n_mc, c.pairing);
  if (sink.on()) sink.carve(b, w.cx.image_floats(), w.cy.image_floats());
  else if (c.pairing == PAIRING_CROSS)  // (one workspace query for calls with and without records: the same carve)
    (void)b.f((size_t)c.batch * w.cx.image_floats()), (void)b.f((size_t)c.batch * w.cy.image_floats());
  LoopCall cc = c;  // (the call with the stochastic step's buffers carved)
  if (cc.sde.on()) cc.sde.carve(b, c.batch, w.cx.image_floats(), w.cy.image_floats());
  if (int rc = check_workspace(b, c.ws_bytes)) return rc;
  if (ns == 0) return RGFM_OK;
  hipStream_t s = (hipStream_t)c.stream;
  if (int rc = w.cx.begin(s, c.num_steps, c.step_begin, ns)) return rc;
  if (int rc = w.cy.begin(s, c.num_steps, c.step_begin, ns)) return rc;
  if (sink.on())
    if (int rc = sink.begin(s, w.cx.image_floats(), w.cy.image_floats())) return rc;
  if (int rc = c.ess.begin(s, loop_stages(c.solver, ns), c.batch)) return rc;
  auto net = [](NetChain& n) { return [&n](auto... a) { return n.eval(a...); }; };  // pair_loop's eval: NetChain::eval
  return pair_loop(net(w.cx), net(w.cy),
                   {.x = x_inout, .y = y_inout, .mc_x1 = mc_x1, .mc_y1 = mc_y1, .mc_ratios = mc_ratios, .n_mc = n_mc,
                    .dx = (int)w.cx.image_floats(), .dy = (int)w.cy.image_floats(), .vx = w.vx, .vy = w.vy, .scratch = w.scratch,
                    .gstate = w.gstate, .x_mid = w.cx.mid, .y_mid = w.cy.mid},
                   cc, ns, sink);
}

}  // namespace

extern "C" int rgfm_sample_cond_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, size_t* bytes) {
  return cond_bytes(h, batch, n_mc, SOLVER_EULER, bytes);
}
extern "C" int rgfm_sample_cond_ode_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, int solver, size_t* bytes) {
  return cond_bytes(h, batch, n_mc, solver, bytes);
}
extern "C" int rgfm_sample_cond(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                int num_steps, double gamma, int step_begin, int step_end, void* ws, size_t ws_bytes,
                                rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc,
                   {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .strength = gamma,
                    .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
extern "C" int rgfm_sample_cond_ode(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                    int num_steps, double gamma, int step_begin, int step_end, int solver, void* ws,
                                    size_t ws_bytes, rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc,
                   {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                    .strength = gamma, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}

extern "C" int rgfm_sample_pair_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc,
                                                size_t* bytes) {
  return pair_bytes(hx, hy, batch, n_mc, SOLVER_EULER, bytes);
}
extern "C" int rgfm_sample_pair_ode_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver,
                                                    size_t* bytes) {
  return pair_bytes(hx, hy, batch, n_mc, solver, bytes);
}
extern "C" int rgfm_sample_pair(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps,
                                double gamma, int step_begin, int step_end, void* ws, size_t ws_bytes,
                                rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .strength = gamma,
                      .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
extern "C" int rgfm_sample_pair_ode(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                    const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps,
                                    double gamma, int step_begin, int step_end, int solver, void* ws, size_t ws_bytes,
                                    rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = gamma, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}

// ---- the same loops with the diagnostics sink (include/rgfm.h, "Guidance diagnostics")
extern "C" int rgfm_sample_cond_diag_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, int solver, size_t* bytes) {
  return cond_bytes(h, batch, n_mc, solver, bytes, true);
}
extern "C" int rgfm_sample_cond_diag(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                     int num_steps, double gamma, int step_begin, int step_end, int solver, float* diag_out,
                                     size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc,
                   {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                    .strength = gamma, .diag_out = diag_out, .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes,
                    .stream = stream});
}
extern "C" int rgfm_sample_pair_diag_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver,
                                                     size_t* bytes) {
  return pair_bytes(hx, hy, batch, n_mc, solver, bytes, true);
}
extern "C" int rgfm_sample_pair_diag(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                     const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps,
                                     double gamma, int step_begin, int step_end, int solver, float* diag_out,
                                     size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = gamma, .diag_out = diag_out, .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes,
                      .stream = stream});
}

// ---- cross pairing: all n_mc x n_mc pairs of the MC set (include/rgfm.h, "Cross pairing of the MC set")
// workspace of the block: the cross scratch (rgfm_host.h), then the two scratch velocities of the diagnostics call
extern "C" int rgfm_guidance_cross_workspace_bytes(int batch, int n_mc, int dim_x, int dim_y, size_t* bytes) {
  if (!bytes || batch < 1 || dim_x < 1 || dim_y < 1) return fail(RGFM_EINVAL, "bad argument");
  if (n_mc < 1 || n_mc > GUID_CROSS_MAX_N) return fail(RGFM_EINVAL, "cross pairing: 1 <= n_mc <= %d (got %d)", GUID_CROSS_MAX_N, n_mc);
  if (dim_x % 4 || dim_y % 4) return fail(RGFM_EINVAL, "flattened image sizes must be multiples of 4");
  *bytes = guid_cross_scratch_bytes(batch, n_mc) + diag_scratch_bytes(batch, dim_x, dim_y);
  return RGFM_OK;
}
namespace {
int guidance_block_cross(const float* x, const float* y, float* vx, float* vy, const float* mc_x1, const float* mc_y1,
                         const float* ratio_matrix, int batch, int n_mc, int dim_x, int dim_y, double t,
                         const StageStrength& gamma, float* wx_out, float* wy_out, void* ws, size_t ws_bytes,
                         rgfm_stream_t stream) {
  if (!x || !y || !vx || !vy || !mc_x1 || !mc_y1 || !ratio_matrix || !ws) return fail(RGFM_EINVAL, "null argument");
  size_t need = 0;
  int rc = rgfm_guidance_cross_workspace_bytes(batch, n_mc, dim_x, dim_y, &need);
  if (rc) return rc;
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if ((rc = ensure_init())) return rc;
  rc = guidance_launch({.x = x, .y = y, .vx = vx, .vy = vy, .mx = mc_x1, .my = mc_y1, .r = ratio_matrix, .B = batch, .N = n_mc,
                        .dx = dim_x, .dy = dim_y, .t = t, .strength = gamma, .scratch = (float*)ws, .weights_out = wx_out,
                        .weights_out_y = wy_out, .stream = (hipStream_t)stream, .pairing = PAIRING_CROSS});
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
}  // namespace
extern "C" int rgfm_guidance_apply_cross(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                                         const float* mc_y1, const float* ratio_matrix, int batch, int n_mc, int dim_x,
                                         int dim_y, double t, double gamma, float* wx_out, float* wy_out, void* ws,
                                         size_t ws_bytes, rgfm_stream_t stream) {
  return guidance_block_cross(x, y, vx, vy, mc_x1, mc_y1, ratio_matrix, batch, n_mc, dim_x, dim_y, t, gamma, wx_out, wy_out, ws,
                              ws_bytes, stream);
}
extern "C" int rgfm_guidance_apply_cross_rows(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                                              const float* mc_y1, const float* ratio_matrix, int batch, int n_mc, int dim_x,
                                              int dim_y, double t, const float* gamma_rows, float* wx_out, float* wy_out,
                                              void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!gamma_rows) return fail(RGFM_EINVAL, "null argument");
  return guidance_block_cross(x, y, vx, vy, mc_x1, mc_y1, ratio_matrix, batch, n_mc, dim_x, dim_y, t,
                              StageStrength(0.0, gamma_rows, 1.0), wx_out, wy_out, ws, ws_bytes, stream);
}
extern "C" int rgfm_guidance_diag_cross(const float* x, const float* y, const float* vx, const float* vy, const float* mc_x1,
                                        const float* mc_y1, const float* ratio_matrix, int batch, int n_mc, int dim_x,
                                        int dim_y, double t, float* diag_out, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!x || !y || !vx || !vy || !mc_x1 || !mc_y1 || !ratio_matrix || !diag_out || !ws) return fail(RGFM_EINVAL, "null argument");
  return guidance_diag({.x = x, .y = y, .mx = mc_x1, .my = mc_y1, .r = ratio_matrix, .B = batch, .N = n_mc, .dx = dim_x,
                        .dy = dim_y, .t = t, .stream = (hipStream_t)stream, .pairing = PAIRING_CROSS},
                       vx, vy, diag_out, ws, ws_bytes);
}
// (one query for calls with and without diagnostics: the scratch velocities are always counted)
extern "C" int rgfm_sample_pair_cross_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver,
                                                      size_t* bytes) {
  if (n_mc > GUID_CROSS_MAX_N) return fail(RGFM_EINVAL, "cross pairing: n_mc %d too large (max %d)", n_mc, GUID_CROSS_MAX_N);
  return pair_bytes(hx, hy, batch, n_mc, solver, bytes, true, PAIRING_CROSS);
}
extern "C" int rgfm_sample_pair_cross(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                      const float* mc_y1, const float* ratio_matrix, int n_mc, int batch, int num_steps,
                                      double gamma, int step_begin, int step_end, int solver, float* diag_out,
                                      size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, ratio_matrix, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = gamma, .diag_out = diag_out, .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes,
                      .stream = stream, .pairing = PAIRING_CROSS});
}

// ---- guidance strength as data (include/rgfm.h, "Guidance strength per sample and per stage"): each loop is its
// *_diag / *_cross namesake with (gamma_rows, stage_scale, n_stage_scale) behind gamma
extern "C" int rgfm_sample_pair_gs(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                   const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                                   const float* gamma_rows, const double* stage_scale, int n_stage_scale, int step_begin,
                                   int step_end, int solver, float* diag_out, size_t diag_records, void* ws, size_t ws_bytes,
                                   rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                      .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
extern "C" int rgfm_sample_pair_cross_gs(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                         const float* mc_y1, const float* ratio_matrix, int n_mc, int batch, int num_steps,
                                         double gamma, const float* gamma_rows, const double* stage_scale, int n_stage_scale,
                                         int step_begin, int step_end, int solver, float* diag_out, size_t diag_records,
                                         void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, ratio_matrix, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                      .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream,
                      .pairing = PAIRING_CROSS});
}
extern "C" int rgfm_sample_cond_gs(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                   int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                                   int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                                   size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc,
                   {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                    .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                    .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}

// ---- the stochastic step (include/rgfm.h, "Stochastic sampling"): each loop is its *_ode / *_gs namesake with
// `const rgfm_sde* sde` in front of ws; null or eta = 0: the namesake
extern "C" int rgfm_sde_scratch_bytes(int batch, int dim_x, int dim_y, size_t* bytes) {
  if (!bytes || batch < 1 || dim_x < 1 || dim_y < 0) return fail(RGFM_EINVAL, "bad argument");
  *bytes = sde_scratch_bytes(batch, (size_t)dim_x, (size_t)dim_y);
  return RGFM_OK;
}
extern "C" int rgfm_sde_noise(uint64_t seed, int stream_id, int k, size_t n, float* out, rgfm_stream_t stream) {
  if (!out || stream_id < 0 || stream_id > 1 || k < 0) return fail(RGFM_EINVAL, "bad argument");
  if (int rc = ensure_init()) return rc;
  launch_sde_noise(out, n, sde_key(seed, stream_id, k), (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
extern "C" int rgfm_sample_single_sde(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin, int step_end,
                                      int solver, const rgfm_sde* sde, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return single_loop(h, x_inout, batch, num_steps, step_begin, step_end, solver, ws, ws_bytes, stream, sde);
}
// ---- class labels and classifier-free guidance (include/rgfm.h, "Class conditioning"): rgfm_sample_single_sde and
// rgfm_sample_two with labels and a scale per net; null labels: the namesake's launches in the *_cfg workspace
extern "C" int rgfm_sample_single_cfg_workspace_bytes(const rgfm_unet* h, int batch, int solver, size_t* bytes) {
  return single_bytes(h, batch, solver, bytes, true);
}
extern "C" int rgfm_sample_single_cfg(rgfm_unet* h, float* x_inout, const int32_t* labels_dev, double cfg_scale, int batch,
                                      int num_steps, int step_begin, int step_end, int solver, const rgfm_sde* sde, void* ws,
                                      size_t ws_bytes, rgfm_stream_t stream) {
  return single_loop(h, x_inout, batch, num_steps, step_begin, step_end, solver, ws, ws_bytes, stream, sde,
                     {true, labels_dev, cfg_scale});
}
extern "C" int rgfm_sample_two_cfg_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch_x, int batch_y, int solver,
                                                   size_t* bytes) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!hx || !hy || !bytes || batch_x < 1 || batch_y < 1) return fail(RGFM_EINVAL, "bad argument");
  Bump b;
  NetChain cx{const_cast<rgfm_unet*>(hx), batch_x, solver}, cy{const_cast<rgfm_unet*>(hy), batch_y, solver};
  cx.cfg_ws = cy.cfg_ws = true;
  carve_single(b, cx), carve_single(b, cy);
  *bytes = b.off;
  return RGFM_OK;
}
extern "C" int rgfm_sample_two_cfg(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const int32_t* labels_x,
                                   const int32_t* labels_y, double cfg_scale_x, double cfg_scale_y, int batch_x, int batch_y,
                                   int num_steps, int step_begin, int step_end, int solver, void* ws, size_t ws_bytes,
                                   rgfm_stream_t stream) {
  return two_loop(hx, hy, x_inout, y_inout, batch_x, batch_y, num_steps, step_begin, step_end, solver, ws, ws_bytes, stream,
                  {true, labels_x, cfg_scale_x}, {true, labels_y, cfg_scale_y});
}

extern "C" int rgfm_sample_pair_sde(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                    const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                                    const float* gamma_rows, const double* stage_scale, int n_stage_scale, int step_begin,
                                    int step_end, int solver, float* diag_out, size_t diag_records, const rgfm_sde* sde, void* ws,
                                    size_t ws_bytes, rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                      .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream, .sde = sde});
}
extern "C" int rgfm_sample_pair_cross_sde(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                          const float* mc_y1, const float* ratio_matrix, int n_mc, int batch, int num_steps,
                                          double gamma, const float* gamma_rows, const double* stage_scale, int n_stage_scale,
                                          int step_begin, int step_end, int solver, float* diag_out, size_t diag_records,
                                          const rgfm_sde* sde, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, ratio_matrix, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                      .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream,
                      .pairing = PAIRING_CROSS, .sde = sde});
}
extern "C" int rgfm_sample_cond_sde(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                    int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                                    int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                                    size_t diag_records, const rgfm_sde* sde, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc,
                   {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                    .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                    .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream, .sde = sde});
}

// ---- the effective-sample-size floor (include/rgfm.h, "Effective-sample-size floor"): each loop is its *_sde namesake
// with `const rgfm_ess* ess` in front of ws; null or ess_min <= 0: the namesake
extern "C" int rgfm_sample_pair_ess(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                    const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                                    const float* gamma_rows, const double* stage_scale, int n_stage_scale, int step_begin,
                                    int step_end, int solver, float* diag_out, size_t diag_records, const rgfm_sde* sde,
                                    const rgfm_ess* ess, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc,
                     {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                      .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                      .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream, .sde = sde, .ess = ess});
}
extern "C" int rgfm_sample_cond_ess(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                    int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                                    int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                                    size_t diag_records, const rgfm_sde* sde, const rgfm_ess* ess, void* ws, size_t ws_bytes,
                                    rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc,
                   {.batch = batch, .num_steps = num_steps, .step_begin = step_begin, .step_end = step_end, .solver = solver,
                    .strength = Strength(gamma, gamma_rows, stage_scale, n_stage_scale), .diag_out = diag_out,
                    .diag_records = diag_records, .ws = ws, .ws_bytes = ws_bytes, .stream = stream, .sde = sde, .ess = ess});
}
