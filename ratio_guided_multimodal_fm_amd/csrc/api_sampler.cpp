// api_sampler.cpp -- the Euler / midpoint samplers over U-Net handles and the stand-alone guidance block (C ABI: include/rgfm.h).
#include "rgfm_host.h"

// ================================================================== samplers
// Every loop below is shared by its Euler entry point (the `solver` = RGFM_SOLVER_EULER case: the launches, arguments and
// workspace layout of before) and its *_ode twin.  Midpoint: a mid-state buffer per modality behind the Euler layout's
// fixed part, two time-table rows per step (launch_stage_table), two stages per step.
namespace {

int check_range(int batch, int num_steps, int step_begin, int step_end) {
  if (batch < 1 || num_steps < 1 || step_begin < 0 || step_end > num_steps || step_begin > step_end)
    return fail(RGFM_EINVAL, "bad step range [%d,%d) of %d", step_begin, step_end, num_steps);
  return RGFM_OK;
}
int check_solver_id(int solver) {
  return solver == SOLVER_EULER || solver == SOLVER_MIDPOINT ? RGFM_OK : fail(RGFM_EINVAL, "unknown solver %d (RGFM_SOLVER_EULER, RGFM_SOLVER_MIDPOINT)", solver);
}
size_t image_floats(const rgfm_unet* h) { return (size_t)h->d.in_channels * h->d.img_size * h->d.img_size; }

int single_bytes(const rgfm_unet* h, int batch, int solver, size_t* bytes) {
  if (!h || !bytes || batch < 1) return fail(RGFM_EINVAL, "bad argument");
  // the time table is sized for up to 4096 rows per call
  *bytes = unet_eval_bytes(const_cast<rgfm_unet*>(h), batch) + table_bytes(h, 4096) + counter_bytes(batch) +
           (solver == SOLVER_MIDPOINT ? state_bytes(batch, image_floats(h)) : 0);
  return RGFM_OK;
}

int single_loop(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin, int step_end, int solver, void* ws,
                size_t ws_bytes, rgfm_stream_t stream) {
  refresh_modes();
  if (int rc = check_solver_id(solver)) return rc;
  if (!h || !x_inout || !ws) return fail(RGFM_EINVAL, "null argument");
  if (int rc = check_range(batch, num_steps, step_begin, step_end)) return rc;
  const int ns = step_end - step_begin;
  if (int rc = check_solver(solver, ns, num_steps)) return rc;
  size_t need = 0;
  single_bytes(h, batch, solver, &need);
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if (ns == 0) return RGFM_OK;
  hipStream_t s = (hipStream_t)stream;
  Bump b;
  b.base = (char*)ws, b.cap = ws_bytes, b.dry = false;
  float* table = b.f((size_t)4096 * h->temb_total);
  unsigned* cnt = reinterpret_cast<unsigned*>(b.f(batch));
  float* mid = solver == SOLVER_MIDPOINT ? b.f((size_t)batch * image_floats(h)) : nullptr;
  HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)batch * sizeof(unsigned), s));
  launch_stage_table(h, solver, num_steps, step_begin, ns, table, s);
  const size_t mark = b.off;
  const double dtd = 1.0 / (double)num_steps;
  const float dt = (float)dtd, dth = (float)(0.5 * dtd);
  // one stage: out = base + v(in, row's t) dts, fused into the out-conv
  auto stage = [&](int row, const float* in, float* out, const float* base, float dts) {
    b.off = mark;
    UNetRun r{h, batch, &b, s, table + (size_t)row * h->temb_total, 0, false};
    r.fin_counter = cnt;
    return r.run(in, nullptr, out, dts, base);
  };
  for (int i = 0; i < ns; ++i) {
    int rc;
    if (solver == SOLVER_MIDPOINT) {
      if ((rc = stage(2 * i, x_inout, mid, x_inout, dth))) return rc;
      rc = stage(2 * i + 1, mid, x_inout, x_inout, dt);
    } else {
      rc = stage(i, x_inout, x_inout, x_inout, dt);
    }
    if (rc) return rc;
  }
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

// ---- two unguided integrations at once (the MC pre-phase of the paired sampler)
// One net's chain of launches as single_loop runs it, cut into steps so that two chains can be enqueued side by side.
struct Chain {
  rgfm_unet* h;
  float* x;
  int batch, solver;
  hipStream_t s;
  Bump b;
  float *table = nullptr, *mid = nullptr;
  unsigned* cnt = nullptr;
  size_t mark = 0;
  float dt = 0.f, dth = 0.f;

  int begin(void* ws, size_t bytes, int num_steps, int step_begin, int ns) {
    b.base = (char*)ws, b.cap = bytes, b.dry = false;
    table = b.f((size_t)4096 * h->temb_total);
    cnt = reinterpret_cast<unsigned*>(b.f(batch));
    mid = solver == SOLVER_MIDPOINT ? b.f((size_t)batch * image_floats(h)) : nullptr;
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)batch * sizeof(unsigned), s));
    launch_stage_table(h, solver, num_steps, step_begin, ns, table, s);
    mark = b.off;
    const double dtd = 1.0 / (double)num_steps;
    dt = (float)dtd, dth = (float)(0.5 * dtd);
    return RGFM_OK;
  }
  int stage(int row, const float* in, float* out, const float* base, float dts) {
    b.off = mark;
    UNetRun r{h, batch, &b, s, table + (size_t)row * h->temb_total, 0, false};
    r.fin_counter = cnt;
    return r.run(in, nullptr, out, dts, base);
  }
  int step(int i) {
    if (solver != SOLVER_MIDPOINT) return stage(i, x, x, x, dt);
    if (int rc = stage(2 * i, x, mid, x, dth)) return rc;
    return stage(2 * i + 1, mid, x, x, dt);
  }
};

// Conv FLOPs of one evaluation of one row, from the descriptor's layer list (the walk of UNetRun::run).
double row_flops(const rgfm_unet* h) {
  const rgfm_unet_desc& d = h->d;
  auto res = [](const ResW& r, int S) {
    return 2.0 * S * S * r.cout * (9.0 * r.cin + 9.0 * r.cout + (r.has_skip ? r.cin : 0));
  };
  int S = d.img_size;
  double f = 2.0 * S * S * 9.0 * d.in_channels * (h->mc + h->final_ch);
  size_t e = 0, di = 0;
  for (int l = 0; l < d.num_levels; ++l) {
    for (int r = 0; r < d.num_res_blocks; ++r) f += res(h->enc[e++], S);
    if (l < d.num_levels - 1) S /= 2, f += 2.0 * S * S * 9.0 * h->down[l].cin * h->down[l].cout;
  }
  f += res(h->mid[0], S) + res(h->mid[1], S);
  for (int l = d.num_levels - 1; l >= 0; --l) {
    for (int i = 0; i < d.num_res_blocks + 1; ++i) f += res(h->dec[di++], S);
    if (l > 0) S *= 2, f += 2.0 * S * S * 9.0 * h->up[d.num_levels - 1 - l].cin * h->up[d.num_levels - 1 - l].cout;
  }
  return f;
}

int two_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch_x, int batch_y, int solver, size_t* bytes) {
  size_t nx = 0, ny = 0;
  if (int rc = single_bytes(hx, batch_x, solver, &nx)) return rc;
  if (int rc = single_bytes(hy, batch_y, solver, &ny)) return rc;
  *bytes = nx + ny;
  return RGFM_OK;
}

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
             int step_begin, int step_end, int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  refresh_modes();
  if (int rc = check_solver_id(solver)) return rc;
  if (!hx || !hy || !x_inout || !y_inout || !ws) return fail(RGFM_EINVAL, "null argument");
  if (x_inout == y_inout) return fail(RGFM_EINVAL, "the two states must be different buffers");
  if (int rc = check_range(batch_x, num_steps, step_begin, step_end)) return rc;
  if (batch_y < 1) return fail(RGFM_EINVAL, "bad argument");
  const int ns = step_end - step_begin;
  if (int rc = check_solver(solver, ns, num_steps)) return rc;
  size_t nx = 0, ny = 0;
  single_bytes(hx, batch_x, solver, &nx);
  single_bytes(hy, batch_y, solver, &ny);
  if (nx + ny > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, nx + ny);
  if (ns == 0) return RGFM_OK;
  DevState* ds = cur_dev();
  if (!ds) return fail(RGFM_EINVAL, "no handle has been created on the current device");
  hipStream_t caller = (hipStream_t)stream;
  const bool overlap = g_modes.overlap;  // (RGFM_OVERLAP=0: both chains on the caller's stream)
  const double wx = row_flops(hx) * batch_x, wy = row_flops(hy) * batch_y;
  Chain cx{hx, x_inout, batch_x, solver, caller}, cy{hy, y_inout, batch_y, solver, overlap ? ds->side : caller};
  Chain &lng = wx > wy ? cx : cy, &sht = wx > wy ? cy : cx;
  // Whatever has been enqueued on the side stream must be joined into the caller's on every exit path.
  struct Join {
    DevState* ds;
    hipStream_t caller, side;
    ~Join() {
      if (side != caller) (void)hipEventRecord(ds->join, side), (void)hipStreamWaitEvent(caller, ds->join, 0);
    }
  } join{ds, caller, cy.s};
  if (overlap) {
    HIP_TRY(hipEventRecord(ds->fork, caller));
    HIP_TRY(hipStreamWaitEvent(cy.s, ds->fork, 0));
  }
  if (int rc = cx.begin(ws, nx, num_steps, step_begin, ns)) return rc;
  if (int rc = cy.begin((char*)ws + nx, ny, num_steps, step_begin, ns)) return rc;
  if (!overlap || !g_modes.prephase) {  // the earlier order: the second net's whole chain, then the first's
    for (Chain* c : {&cy, &cx})
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
  return two_bytes(hx, hy, batch_x, batch_y, solver, bytes);
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
  if (int rc = check_solver_id(solver)) return rc;
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

extern "C" int rgfm_guidance_apply(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                                   const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x,
                                   int dim_y, double t, double gamma, float* weights_out, void* ws,
                                   size_t ws_bytes, rgfm_stream_t stream) {
  if (!x || !y || !vx || !vy || !mc_x1 || !mc_y1 || !mc_ratios || !ws) return fail(RGFM_EINVAL, "null argument");
  size_t need = 0;
  int rc = rgfm_guidance_workspace_bytes(batch, n_mc, &need);
  if (rc) return rc;
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if ((rc = ensure_init())) return rc;
  rc = guidance_launch(x, y, vx, vy, mc_x1, mc_y1, mc_ratios, batch, n_mc, dim_x, dim_y, t, gamma, (float*)ws,
                       weights_out, nullptr, nullptr, 0.f, (hipStream_t)stream);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

// The one-sided block: the paired block with dy = 0 and a ratio row per sample (guidance_launch).
extern "C" int rgfm_guidance_apply_cond(const float* s, float* v, const float* mc_set, const float* ratios, int batch, int n_mc,
                                        int dim, double t, double gamma, float* weights_out, void* ws, size_t ws_bytes,
                                        rgfm_stream_t stream) {
  if (!s || !v || !mc_set || !ratios || !ws) return fail(RGFM_EINVAL, "null argument");
  if (dim < 1) return fail(RGFM_EINVAL, "bad argument");
  size_t need = 0;
  int rc = rgfm_guidance_workspace_bytes(batch, n_mc, &need);
  if (rc) return rc;
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if ((rc = ensure_init())) return rc;
  rc = guidance_launch(s, nullptr, v, nullptr, mc_set, nullptr, ratios, batch, n_mc, dim, 0, t, gamma, (float*)ws, weights_out,
                       nullptr, nullptr, 0.f, (hipStream_t)stream, nullptr, nullptr, 0, n_mc);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

namespace {

int cond_bytes(const rgfm_unet* h, int batch, int n_mc, int solver, size_t* bytes) {
  if (!h || !bytes || batch < 1 || n_mc < 1) return fail(RGFM_EINVAL, "bad argument");
  const size_t d = image_floats(h);
  *bytes = unet_eval_bytes(const_cast<rgfm_unet*>(h), batch) + table_bytes(h, 4096) + counter_bytes(batch) +
           ((batch * d * 4 + 255) & ~(size_t)255) + guid_scratch_bytes(batch, n_mc) +
           (solver == SOLVER_MIDPOINT ? state_bytes(batch, d) : 0);
  return RGFM_OK;
}

// One net, guided by the one-sided block: kernel by kernel on the caller's stream (nothing to overlap, no graph).
int cond_loop(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch, int num_steps,
              double gamma, int step_begin, int step_end, int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  refresh_modes();
  if (int rc = check_solver_id(solver)) return rc;
  if (!h || !s_inout || !mc_set || !ratios || !ws) return fail(RGFM_EINVAL, "null argument");
  if (n_mc < 1) return fail(RGFM_EINVAL, "conditional sampling needs an MC set (n_mc >= 1)");
  if (int rc = check_range(batch, num_steps, step_begin, step_end)) return rc;
  const int ns = step_end - step_begin;
  if (int rc = check_solver(solver, ns, num_steps)) return rc;
  const int d = h->d.in_channels * h->d.img_size * h->d.img_size;
  if (d % 4) return fail(RGFM_EINVAL, "flattened image sizes must be multiples of 4");
  if (n_mc > 4096) return fail(RGFM_EINVAL, "n_mc too large (max 4096)");
  size_t need = 0;
  int rc = cond_bytes(h, batch, n_mc, solver, &need);
  if (rc) return rc;
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if (ns == 0) return RGFM_OK;
  hipStream_t s = (hipStream_t)stream;
  Bump b;
  b.base = (char*)ws, b.cap = ws_bytes, b.dry = false;
  float* table = b.f((size_t)4096 * h->temb_total);
  unsigned* cnt = reinterpret_cast<unsigned*>(b.f(batch));
  float* v = b.f((size_t)batch * d);
  float* scratch = b.f(guid_scratch_bytes(batch, n_mc) / sizeof(float));
  float* mid = solver == SOLVER_MIDPOINT ? b.f((size_t)batch * d) : nullptr;
  HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)batch * sizeof(unsigned), s));
  launch_stage_table(h, solver, num_steps, step_begin, ns, table, s);
  const size_t mark = b.off;
  const double dtd = 1.0 / (double)num_steps;
  const float dt = (float)dtd, dth = (float)(0.5 * dtd);
  // one stage: out = base + F(in, t) dts; guided iff the stage's own t > eps (`t > eps` test of the reference, :124)
  auto stage = [&](int row, double t, float* in, float* out, const float* base, float dts) -> int {
    const bool guided = t > 1e-3;
    b.off = mark;
    UNetRun r{h, batch, &b, s, table + (size_t)row * h->temb_total, 0, false};
    r.fin_counter = cnt;
    // unguided: the fused Euler epilogue; guided: the raw velocity, and the guidance block moves the state
    if (int rc = guided ? r.run(in, v, nullptr, dts) : r.run(in, nullptr, out, dts, base)) return rc;
    if (!guided) return RGFM_OK;
    return guidance_launch(in, nullptr, v, nullptr, mc_set, nullptr, ratios, batch, n_mc, d, 0, t, gamma, scratch, nullptr,
                           out, nullptr, dts, s, nullptr, nullptr, 0, n_mc, base, nullptr);
  };
  for (int i = 0; i < ns; ++i) {
    const double t = (double)(step_begin + i) * dtd;
    if (solver == SOLVER_MIDPOINT) {
      if ((rc = stage(2 * i, t, s_inout, mid, s_inout, dth))) return rc;
      rc = stage(2 * i + 1, ((double)(step_begin + i) + 0.5) * dtd, mid, s_inout, s_inout, dt);
    } else {
      rc = stage(i, t, s_inout, s_inout, s_inout, dt);
    }
    if (rc) return rc;
  }
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

int pair_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver, size_t* bytes) {
  if (!hx || !hy || !bytes || batch < 1 || n_mc < 0) return fail(RGFM_EINVAL, "bad argument");
  const size_t ex = unet_eval_bytes(const_cast<rgfm_unet*>(hx), batch);
  const size_t ey = unet_eval_bytes(const_cast<rgfm_unet*>(hy), batch);
  const size_t dx = image_floats(hx), dy = image_floats(hy);
  size_t total = table_bytes(hx, 4096) + table_bytes(hy, 4096) + ex + ey + 2 * counter_bytes(batch);  // the two nets run concurrently
  total += ((batch * dx * 4 + 255) & ~(size_t)255) + ((batch * dy * 4 + 255) & ~(size_t)255);
  total += guid_scratch_bytes(batch, n_mc);
  total += 256 + (size_t)4096 * 4 * sizeof(float);  // step counter + per-step guidance scalars (graph replay)
  if (solver == SOLVER_MIDPOINT) total += state_bytes(batch, dx) + state_bytes(batch, dy);
  *bytes = total;
  return RGFM_OK;
}

int pair_sample(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1, const float* mc_y1,
                const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma, int step_begin, int step_end,
                int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  refresh_modes();
  if (int rc = check_solver_id(solver)) return rc;
  if (!hx || !hy || !x_inout || !y_inout || !ws) return fail(RGFM_EINVAL, "null argument");
  if (n_mc < 0 || (n_mc > 0 && (!mc_x1 || !mc_y1 || !mc_ratios))) return fail(RGFM_EINVAL, "MC set missing");
  if (int rc = check_range(batch, num_steps, step_begin, step_end)) return rc;
  const int ns = step_end - step_begin;
  if (int rc = check_solver(solver, ns, num_steps)) return rc;
  size_t need = 0;
  pair_bytes(hx, hy, batch, n_mc, solver, &need);
  if (need > ws_bytes) return fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, need);
  if (ns == 0) return RGFM_OK;
  hipStream_t s = (hipStream_t)stream;
  const int dx = hx->d.in_channels * hx->d.img_size * hx->d.img_size;
  const int dy = hy->d.in_channels * hy->d.img_size * hy->d.img_size;
  Bump b;
  b.base = (char*)ws, b.cap = ws_bytes, b.dry = false;
  float* tx = b.f((size_t)4096 * hx->temb_total);
  float* ty = b.f((size_t)4096 * hy->temb_total);
  float* vx = b.f((size_t)batch * dx);
  float* vy = b.f((size_t)batch * dy);
  float* logp = b.f(guid_scratch_bytes(batch, n_mc) / sizeof(float));
  unsigned* cnt_x = reinterpret_cast<unsigned*>(b.f(batch));
  unsigned* cnt_y = reinterpret_cast<unsigned*>(b.f(batch));
  float* gstate = b.f(64 + (size_t)4096 * 4);
  float* x_mid = solver == SOLVER_MIDPOINT ? b.f((size_t)batch * dx) : nullptr;
  float* y_mid = solver == SOLVER_MIDPOINT ? b.f((size_t)batch * dy) : nullptr;
  HIP_TRY(hipMemsetAsync(cnt_x, 0, (size_t)batch * sizeof(unsigned), s));
  HIP_TRY(hipMemsetAsync(cnt_y, 0, (size_t)batch * sizeof(unsigned), s));
  launch_stage_table(hx, solver, num_steps, step_begin, ns, tx, s);
  launch_stage_table(hy, solver, num_steps, step_begin, ns, ty, s);
  const size_t mark_x = b.off;
  const size_t mark_y = mark_x + unet_eval_bytes(hx, batch);
  // (step: the device-side step counter of the graph-replay path -- the time-table row is then chosen on the device)
  auto eval_x = [&](int row, hipStream_t st, const float* in, float* v_out, float* x_state, const float* base, float dt,
                    const int* step) {
    b.off = mark_x;
    UNetRun r{hx, batch, &b, st, step ? tx : tx + (size_t)row * hx->temb_total, 0, false};
    r.fin_counter = cnt_x, r.step_ptr = step;
    return r.run(in, v_out, x_state, dt, base);
  };
  auto eval_y = [&](int row, hipStream_t st, const float* in, float* v_out, float* y_state, const float* base, float dt,
                    const int* step) {
    b.off = mark_y;
    UNetRun r{hy, batch, &b, st, step ? ty : ty + (size_t)row * hy->temb_total, 0, false};
    r.fin_counter = cnt_y, r.step_ptr = step;
    return r.run(in, v_out, y_state, dt, base);
  };
  return pair_loop(eval_x, eval_y, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc, batch, num_steps, gamma,
                   step_begin, ns, dx, dy, vx, vy, logp, s, gstate, solver, x_mid, y_mid);
}

}  // namespace

extern "C" int rgfm_sample_cond_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, size_t* bytes) {
  return cond_bytes(h, batch, n_mc, SOLVER_EULER, bytes);
}
extern "C" int rgfm_sample_cond_ode_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, int solver, size_t* bytes) {
  if (int rc = check_solver_id(solver)) return rc;
  return cond_bytes(h, batch, n_mc, solver, bytes);
}
extern "C" int rgfm_sample_cond(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                int num_steps, double gamma, int step_begin, int step_end, void* ws, size_t ws_bytes,
                                rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc, batch, num_steps, gamma, step_begin, step_end, SOLVER_EULER, ws, ws_bytes,
                   stream);
}
extern "C" int rgfm_sample_cond_ode(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                                    int num_steps, double gamma, int step_begin, int step_end, int solver, void* ws,
                                    size_t ws_bytes, rgfm_stream_t stream) {
  return cond_loop(h, s_inout, mc_set, ratios, n_mc, batch, num_steps, gamma, step_begin, step_end, solver, ws, ws_bytes, stream);
}

extern "C" int rgfm_sample_pair_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc,
                                                size_t* bytes) {
  return pair_bytes(hx, hy, batch, n_mc, SOLVER_EULER, bytes);
}
extern "C" int rgfm_sample_pair_ode_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver,
                                                    size_t* bytes) {
  if (int rc = check_solver_id(solver)) return rc;
  return pair_bytes(hx, hy, batch, n_mc, solver, bytes);
}
extern "C" int rgfm_sample_pair(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps,
                                double gamma, int step_begin, int step_end, void* ws, size_t ws_bytes,
                                rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc, batch, num_steps, gamma, step_begin, step_end,
                     SOLVER_EULER, ws, ws_bytes, stream);
}
extern "C" int rgfm_sample_pair_ode(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                    const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps,
                                    double gamma, int step_begin, int step_end, int solver, void* ws, size_t ws_bytes,
                                    rgfm_stream_t stream) {
  return pair_sample(hx, hy, x_inout, y_inout, mc_x1, mc_y1, mc_ratios, n_mc, batch, num_steps, gamma, step_begin, step_end,
                     solver, ws, ws_bytes, stream);
}
