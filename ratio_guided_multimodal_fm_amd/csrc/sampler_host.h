// sampler_host.h -- what the sampler loops share (api_sampler.cpp, api_ratio.cpp, api_fmnet.cpp; api_train.cpp for the
// solver checks): the argument prelude, the stage list (sampler_stages.h), one U-Net's integration state (NetChain) and
// the paired guided loop.  A loop's workspace is described once, by a carve over a Bump: the *_workspace_bytes query is
// that carve's end offset, the call checks the same figure against ws_bytes before it launches anything.
#pragma once
#include "rgfm_host.h"
#include "sampler_stages.h"

constexpr int TABLE_ROWS = 4096;  // rows of a call's time table: one per Euler step, two per midpoint step
constexpr int MAX_STEPS_EULER = TABLE_ROWS, MAX_STEPS_MIDPOINT = TABLE_ROWS / 2;
inline int check_solver(int solver, int ns, int num_steps) {
  if (solver != SOLVER_EULER && solver != SOLVER_MIDPOINT) return fail(RGFM_EINVAL, "unknown solver %d (RGFM_SOLVER_EULER, RGFM_SOLVER_MIDPOINT)", solver);
  if (solver == SOLVER_EULER && ns > MAX_STEPS_EULER) return fail(RGFM_EINVAL, "at most 4096 steps per call");
  if (solver == SOLVER_MIDPOINT && ns > MAX_STEPS_MIDPOINT) return fail(RGFM_EINVAL, "midpoint: at most 2048 steps per call (two time-table rows per step)");
  if (solver == SOLVER_MIDPOINT && num_steps > (1 << 30)) return fail(RGFM_EINVAL, "midpoint: num_steps too large");
  return RGFM_OK;
}
inline int check_solver_id(int solver) { return check_solver(solver, 0, 0); }  // (what a *_workspace_bytes query can check)

// The prelude of every loop, in this order: solver id, null arguments (`have_args`: the loop's own pointers), step range,
// step caps.  `time_table` = false (the FlowMatchingModel loops embed t per evaluation): no cap on the steps of a call.
inline int check_loop(int solver, bool have_args, int batch, int num_steps, int step_begin, int step_end, int* ns,
                      bool time_table = true) {
  if (int rc = check_solver_id(solver)) return rc;
  if (!have_args) return fail(RGFM_EINVAL, "null argument");
  if (batch < 1 || num_steps < 1 || step_begin < 0 || step_end > num_steps || step_begin > step_end)
    return fail(RGFM_EINVAL, "bad step range [%d,%d) of %d", step_begin, step_end, num_steps);
  *ns = step_end - step_begin;
  return time_table ? check_solver(solver, *ns, num_steps) : RGFM_OK;
}
// ... and its last line: the carve's end against what the caller brought
inline int check_workspace(const Bump& carved, size_t ws_bytes) {
  return carved.off > ws_bytes ? fail(RGFM_ENOMEM, "workspace too small: %zu < %zu", ws_bytes, carved.off) : RGFM_OK;
}

// The diagnostics sink of a loop (include/rgfm.h, "Guidance diagnostics"): null `out` = off, and every loop then enqueues
// what it enqueues without one.  On: one [batch][RGFM_DIAG_FLOATS] block of `out` per stage, block Stage::row the
// stage's; `begin` zeroes all of them (an unguided stage's record, and the entries a loop does not fill, stay 0), the
// guided stages' kernels fill theirs.  gx / gy: the MC loops' scratch velocities for the pure guided velocity
// (GuidDiag), carved behind the loop's own workspace.
struct DiagSink {
  float* out = nullptr;
  size_t records = 0;
  int batch = 0, n_stages = 0;
  float *gx = nullptr, *gy = nullptr;
  bool on() const { return out != nullptr; }
  // the argument check of every *_diag entry point, before anything is carved or enqueued
  int check(float* diag_out, size_t diag_records, int batch_, int ns, int solver) {
    if (!diag_out && !diag_records) return RGFM_OK;
    if (!diag_out || !diag_records) return fail(RGFM_EINVAL, "diag_out and diag_records go together (both, or null and 0)");
    out = diag_out, records = diag_records, batch = batch_, n_stages = loop_stages(solver, ns);
    if (records < (size_t)n_stages * batch)
      return fail(RGFM_EINVAL, "diag_records %zu < %d stages x %d samples", records, n_stages, batch);
    return RGFM_OK;
  }
  void carve(Bump& b, size_t dx, size_t dy) { gx = b.f((size_t)batch * dx), gy = b.f((size_t)batch * dy); }
  int begin(hipStream_t s, size_t dx, size_t dy) {
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_stages * batch * RGFM_DIAG_FLOATS * sizeof(float), s));
    if (gx && dx) HIP_TRY(hipMemsetAsync(gx, 0, (size_t)batch * dx * sizeof(float), s));
    if (gy && dy) HIP_TRY(hipMemsetAsync(gy, 0, (size_t)batch * dy * sizeof(float), s));
    return RGFM_OK;
  }
  // the records of stage `row` (Stage::row; the one evaluation of a block: 0), for a GuidanceCall; off: none
  GuidDiag at(int row) const { return on() ? GuidDiag{out + (size_t)row * batch * RGFM_DIAG_FLOATS, gx, gy} : GuidDiag{}; }
};
// bytes a loop's workspace grows by with diagnostics on (the *_diag_workspace_bytes queries): DiagSink::carve
inline size_t diag_scratch_bytes(int batch, size_t dx, size_t dy) {
  Bump b;
  DiagSink d;
  d.batch = batch, d.carve(b, dx, dy);
  return b.off;
}

// The stochastic step of a loop (include/rgfm.h, "Stochastic sampling"; Euler-Maruyama): eta = 0 -- or no rgfm_sde -- is
// off, and every loop then enqueues what it enqueues without the argument.  On, step k of num_steps is
//   base = (1 - eta dt) state + sigma_k xi_k,   sigma_k = sqrt(2 eta (1 - t) dt),   state = base + ((1 + eta t) dt) F(state, t):
// `stage` enqueues the first line into the loop's extra [batch][D] buffer of the modality (carved behind the loop's
// own buffers, as the diagnostics' scratch) and hands back the second line's base and dts for the loop's fused update,
// which reads the old state and stays as it is.  The noise of stream m (0: the loop's first or only state, 1: the
// second) at step k depends on (seed, m, k, element) alone: sde_key, and sde.hip.
inline uint64_t sde_fin(uint64_t z) {  // (the splitmix64 finaliser of the dropout masks)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline uint64_t sde_key(uint64_t seed, int stream_id, int k) {
  return sde_fin(seed + 0x9E3779B97F4A7C15ull * ((((uint64_t)(uint32_t)stream_id << 32) | (uint32_t)k) + 1ull));
}
struct Sde {
  double eta = 0.0;
  uint64_t seed = 0;
  float* buf[2] = {nullptr, nullptr};  // the pre-updated state of stream 0 / 1
  Sde() = default;
  Sde(const rgfm_sde* a) {  // (null: off)
    if (a) eta = a->eta, seed = a->seed;
  }
  bool on() const { return eta > 0.0; }
  // the argument check of every *_sde entry point, before anything is carved or enqueued
  int check(int solver) const {
    if (!(eta >= 0.0) || !std::isfinite(eta)) return fail(RGFM_EINVAL, "sde: eta must be finite and >= 0 (got %g)", eta);
    if (on() && solver == SOLVER_MIDPOINT) return fail(RGFM_EINVAL, "sde: eta > 0 needs RGFM_SOLVER_EULER (no stochastic midpoint rule)");
    return RGFM_OK;
  }
  void carve(Bump& b, int batch, size_t dx, size_t dy) {
    buf[0] = b.f((size_t)batch * dx);
    if (dy) buf[1] = b.f((size_t)batch * dy);
  }
  // Stage g of a loop over num_steps, state `x` ([batch][D] = n floats) of stream m, on s: enqueues the pre-update and
  // returns the stage's base and dts.  Off: nothing is enqueued, and (base_off, g.dts) -- the loop's own -- come back.
  int stage(const Stage& g, int num_steps, int m, const float* x, size_t n, hipStream_t s, const float* base_off, const float** base,
            float* dts) const {
    *base = base_off, *dts = g.dts;
    if (!on()) return RGFM_OK;
    const double dt = 1.0 / (double)num_steps;
    launch_sde_pre(x, buf[m], n, sde_key(seed, m, g.step), (float)(1.0 - eta * dt), (float)std::sqrt(2.0 * eta * (1.0 - g.t) * dt), s);
    *base = buf[m], *dts = (float)((1.0 + eta * g.t) * dt);
    return RGFM_OK;
  }
};
// bytes a loop's workspace grows by with eta > 0 (rgfm_sde_scratch_bytes): Sde::carve
inline size_t sde_scratch_bytes(int batch, size_t dx, size_t dy) {
  Bump b;
  Sde().carve(b, batch, dx, dy);
  return b.off;
}

// The effective-sample-size floor of an MC loop (include/rgfm.h, "Effective-sample-size floor"): no rgfm_ess, or
// ess_min <= 0, is off, and every loop then enqueues what it enqueues without the argument.  On, each guided stage's
// weights kernel is guid_weights_ess_kernel, and block Stage::row of tau_out ([stages][batch], or null) receives the
// rows' exponents; `begin` zeroes the blocks, so an unguided stage's stay 0.
struct Ess {
  double ess_min = 0.0;
  float* tau_out = nullptr;
  size_t tau_records = 0;
  Ess() = default;
  Ess(const rgfm_ess* a) {  // (null: off)
    if (a) ess_min = a->ess_min, tau_out = a->tau_out, tau_records = a->tau_records;
  }
  bool on() const { return !(ess_min <= 0.0); }  // (NaN counts as on, and fails the check)
  // the argument check of every *_ess entry point, before anything is carved or enqueued
  static int check_min(double ess_min, int n_mc) {
    if (!std::isfinite(ess_min)) return fail(RGFM_EINVAL, "ess: ess_min must be finite (got %g)", ess_min);
    if (ess_min < 1.0) return fail(RGFM_EINVAL, "ess: ess_min %g in (0, 1): an effective sample size is at least 1", ess_min);
    if (ess_min > (double)n_mc) return fail(RGFM_EINVAL, "ess: ess_min %g > n_mc %d", ess_min, n_mc);
    return RGFM_OK;
  }
  int check(int n_mc, int n_stages, int batch) const {
    if (!on()) return RGFM_OK;
    if (int rc = check_min(ess_min, n_mc)) return rc;
    if (tau_out && tau_records < (size_t)n_stages * batch)
      return fail(RGFM_EINVAL, "ess: tau_records %zu < %d stages x %d samples", tau_records, n_stages, batch);
    return RGFM_OK;
  }
  int begin(hipStream_t s, int n_stages, int batch) const {
    if (on() && tau_out) HIP_TRY(hipMemsetAsync(tau_out, 0, (size_t)n_stages * batch * sizeof(float), s));
    return RGFM_OK;
  }
  float* at(int row, int batch) const { return on() && tau_out ? tau_out + (size_t)row * batch : nullptr; }
  double floor() const { return on() ? ess_min : 0.0; }
};

// The call-level arguments of a sampler loop, filled by field name in its extern "C" wrapper; the loop's own operands
// (handles, states, MC set) travel beside it.  What an entry point has no argument for keeps its default.
struct LoopCall {
  int batch = 0, num_steps = 0, step_begin = 0, step_end = 0, solver = SOLVER_EULER;
  Strength strength{0.0};
  float* diag_out = nullptr;  // the diagnostics sink (DiagSink): both, or null and 0
  size_t diag_records = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  rgfm_stream_t stream = nullptr;
  int pairing = PAIRING_PAIRED;  // (the U-Net pair loop)
  Sde sde;                       // (the *_sde entry points)
  Ess ess;                       // (the *_ess entry points)
};
// The head of every guided loop, in this order: the switches, check_loop (`have_args`: the loop's own pointers), the
// stochastic step's arguments, the sink's, the strength's.  The loop's own argument checks follow it, then its carve and check_workspace.
inline int open_loop(const LoopCall& c, bool have_args, int* ns, DiagSink* sink, bool time_table = true) {
  refresh_modes();
  if (int rc = check_loop(c.solver, have_args && c.ws, c.batch, c.num_steps, c.step_begin, c.step_end, ns, time_table)) return rc;
  if (int rc = c.sde.check(c.solver)) return rc;
  if (int rc = sink->check(c.diag_out, c.diag_records, c.batch, *ns, c.solver)) return rc;
  return c.strength.check(loop_stages(c.solver, *ns));
}

// Time-table rows of a loop's stages.  Euler: row i is t = (step_begin + i) / num_steps.  Midpoint: row 2i is the step's
// t1 = (step_begin + i) dt and row 2i + 1 its t2 = (step_begin + i + 0.5) dt -- the table of the 2 num_steps half-steps:
// (2k + j) * (1.0 / (2 N)) and (k + j / 2) * (1.0 / N) are the same double (a factor two moves no rounding).
inline int launch_stage_table(rgfm_unet* h, int solver, int num_steps, int step_begin, int ns, float* table, hipStream_t s) {
  if (solver == SOLVER_MIDPOINT) return launch_time_table(h, nullptr, 2 * num_steps, 2 * step_begin, 2 * ns, table, s);
  return launch_time_table(h, nullptr, num_steps, step_begin, ns, table, s);
}

// One U-Net's integration state inside a loop's workspace: the time table, the [batch] arrival counters of the
// producer-side GroupNorm finalize, the mid state of the midpoint solver and the region its evaluations carve their
// activations from.  The Bump is the loop's: nets that run concurrently carve disjoint regions of it (carve_eval one
// after the other), a pass that runs after the net on the same stream may reuse the region from `mark`.
struct NetChain {
  rgfm_unet* h = nullptr;
  int batch = 0, solver = SOLVER_EULER;
  float* x = nullptr;  // the state `step` advances (the unguided loops; the guided loops pass their own pointers to eval)
  hipStream_t s = nullptr;  // ... and its stream, from begin
  Bump* b = nullptr;
  float *table = nullptr, *mid = nullptr;
  unsigned* cnt = nullptr;
  size_t mark = 0;
  int num_steps = 1, step_begin = 0;
  // Class labels and classifier-free guidance (the *_cfg entry points; include/rgfm.h, "Class conditioning").  `cfg_ws`:
  // the carve holds the labelled call's buffers, so that one query serves every scale.  With `labels` (device int32
  // [batch]) the table is [stages][K + 1][temb_total], a stage's conditional evaluation reads `rowtab`, its rows gathered
  // by label, and its unconditional one the stage's null row -- today's launch.  Without: nothing below is touched.
  bool cfg_ws = false;
  const int* labels = nullptr;
  float cfg_scale = 1.f;
  float *rowtab = nullptr, *vc = nullptr, *vu = nullptr;

  size_t image_floats() const { return (size_t)h->d.in_channels * h->d.img_size * h->d.img_size; }
  int classes() const { return labels ? h->num_classes + 1 : 1; }  // table rows per stage
  void carve(Bump& bump) {
    b = &bump;
    table = bump.f((size_t)TABLE_ROWS * h->temb_total);
    cnt = bump.u(batch);
    mid = solver == SOLVER_MIDPOINT ? bump.f((size_t)batch * image_floats()) : nullptr;
    if (cfg_ws) {
      rowtab = bump.f((size_t)batch * h->temb_total);
      vc = bump.f((size_t)batch * image_floats()), vu = bump.f((size_t)batch * image_floats());
    }
  }
  // the argument check of the *_cfg entry points, before anything is carved or enqueued (ns: the call's steps)
  int check_cfg(const int* labels_dev, double scale, int ns) {
    cfg_ws = true, labels = labels_dev, cfg_scale = (float)scale;
    if (!std::isfinite(scale)) return fail(RGFM_EINVAL, "cfg_scale must be finite (got %g)", scale);
    if (!labels) return RGFM_OK;
    if (!h->num_classes) return fail(RGFM_EINVAL, "labels on a handle without classes (rgfm_unet_labeled_create makes one)");
    if ((long long)loop_stages(solver, ns) * classes() > TABLE_ROWS)
      return fail(RGFM_EINVAL, "a labelled call holds at most %d (stage, class) rows: %d stages x %d classes; split the steps", TABLE_ROWS,
                  loop_stages(solver, ns), classes());
    return RGFM_OK;
  }
  void carve_eval() {  // one evaluation's activations, from the Bump's current offset (the walk of UNetRun, run dry)
    mark = b->off;
    UNetRun r{h, batch, b, nullptr, nullptr, 0, true};
    r.run(nullptr, nullptr, nullptr, 0.f);
  }
  int begin(hipStream_t stream, int num_steps_, int step_begin_, int ns) {
    s = stream, num_steps = num_steps_, step_begin = step_begin_;
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)batch * sizeof(unsigned), s));
    if (labels) {  // the class table: one row per (stage, class), the stages' times as launch_stage_table lays them out
      const int f = solver == SOLVER_MIDPOINT ? 2 : 1;
      return launch_class_table(h, nullptr, 0, nullptr, f * num_steps, f * step_begin, f * ns * classes(), table, s);
    }
    return launch_stage_table(h, solver, num_steps, step_begin, ns, table, s);
  }
  // The net at `in` with time-table row `row` on `s`: v_out receives the raw velocity, state_out = base + v dts (the fused
  // epilogue of the out-conv).  step_ptr: the device-side step counter of the graph-replay path, which picks the row.
  int eval(int row, hipStream_t s, const float* in, float* v_out, float* state_out, const float* base, float dts,
           const int* step_ptr = nullptr) {
    b->off = mark;
    // (a labelled call: the stage's null row, last of its K + 1 -- the unconditional evaluation)
    const size_t trow = labels ? (size_t)row * classes() + h->num_classes : (size_t)row;
    UNetRun r{h, batch, b, s, step_ptr ? table : table + trow * h->temb_total, 0, false};
    r.fin_counter = cnt, r.step_ptr = step_ptr;
    return r.run(in, v_out, state_out, dts, base);
  }
  // The conditional evaluation of a labelled call's stage: the rows' time table gathered by label, then eval's walk with a
  // row of the table per sample (ConvArgs::temb_per_row).
  int eval_cond(int row, hipStream_t s, const float* in, float* v_out, float* state_out, const float* base, float dts) {
    b->off = mark;
    launch_cfg_gather(table, labels, h->num_classes, row, batch, h->temb_total, rowtab, s);
    UNetRun r{h, batch, b, s, rowtab, 1, false};
    r.fin_counter = cnt;
    return r.run(in, v_out, state_out, dts, base);
  }
  // One stage of a *_cfg call: state_out = base + (v_u + w (v_c - v_u)) dts.  w = 1: the conditional evaluation alone
  // and w = 0 (or no labels): the unconditional one alone, each with the out-conv's fused update; else both raw
  // velocities and the blend kernel, which takes the same (base, dts).
  int eval_cfg(int row, hipStream_t s, const float* in, float* state_out, const float* base, float dts) {
    if (!labels || cfg_scale == 0.f) return eval(row, s, in, nullptr, state_out, base, dts);
    if (cfg_scale == 1.f) return eval_cond(row, s, in, nullptr, state_out, base, dts);
    if (int rc = eval_cond(row, s, in, vc, nullptr, nullptr, dts)) return rc;
    if (int rc = eval(row, s, in, vu, nullptr, nullptr, dts)) return rc;
    launch_cfg_blend(base, vc, vu, cfg_scale, dts, (size_t)batch * image_floats(), state_out, s);
    return RGFM_OK;
  }
  // one unguided step of `x` on `s`: every stage's update fused into the out-conv; `sde`: the stochastic step (stream 0)
  int step(int i, const Sde& sde = Sde()) {
    Stage st[2];
    const int n = step_stages(solver, num_steps, step_begin, i, st);
    for (int k = 0; k < n; ++k) {
      const float* base = nullptr;
      float dts = 0.f;
      if (int rc = sde.stage(st[k], num_steps, 0, x, (size_t)batch * image_floats(), s, x, &base, &dts)) return rc;
      if (int rc = eval_cfg(st[k].row, s, st[k].reads_mid ? mid : x, st[k].writes_mid ? mid : x, base, dts)) return rc;
    }
    return RGFM_OK;
  }
};

// what pair_loop works on beside the call record: the two states, the MC set, and its buffers in the caller's workspace
struct PairOperands {
  float *x = nullptr, *y = nullptr;  // the states, advanced in place
  // the MC set; pairing = PAIRING_CROSS: mc_ratios is the [n_mc][n_mc] ratio matrix and `scratch` guid_cross_scratch_bytes
  const float *mc_x1 = nullptr, *mc_y1 = nullptr, *mc_ratios = nullptr;
  int n_mc = 0, dx = 0, dy = 0;
  float *vx = nullptr, *vy = nullptr;  // the guided stages' raw velocities
  float* scratch = nullptr;            // the guidance block's (GuidanceCall::scratch)
  float* gstate = nullptr;             // graph-replay state, or null: never replay
  float *x_mid = nullptr, *y_mid = nullptr;  // midpoint: one mid-state buffer per modality
};

// Shared loop of paired_sampler (src/utils/flow_utils.py:186-278 with the guidance of
// src/sample_mnist_svhn.py:117-175): eval_x / eval_y enqueue one velocity-net evaluation of a stage
// on the given stream, writing the raw velocity (guided stages) or the fused Euler update.
// eval(row, stream, in, v_out, state_out, base, dt, step): the net at `in` with time-table row `row`; state_out = base + v dt.
// The stages come from for_each_stage.  Midpoint (x_mid / y_mid: one mid-state buffer per modality):
//   (x_mid, y_mid) = (x, y) + (dt / 2) F(x, y, t1),   (x, y) = (x, y) + dt F(x_mid, y_mid, t2),   t2 = t1 + dt / 2,
// F the whole guided velocity at the stage's own state and time; a stage is guided iff its own t > 1e-3.  Each stage
// forks and joins the side stream as an Euler step does.
// Graph replay (U-Net pairs, RGFM_GRAPH=1; never with active kernel timers): every guided step enqueues the
// same ~135 launches with the same arguments except the time-table row and three guidance scalars.  Euler only: a midpoint
// call runs kernel by kernel.  Those are read
// on the device through a step counter (`gstate`: [0] the counter, [64..] the per-step scalars), so the first guided
// step is captured once -- both streams, fork and join included -- into a hipGraph and every guided step is one
// hipGraphLaunch.  Results are bit-identical to the kernel-by-kernel path (same kernels, same arguments).
template <class EvalX, class EvalY>
int pair_loop(EvalX&& eval_x, EvalY&& eval_y, const PairOperands& p, const LoopCall& c, int ns, const DiagSink& sink) {
  const int n_mc = p.n_mc, num_steps = c.num_steps, step_begin = c.step_begin, solver = c.solver;
  const Strength& strength = c.strength;
  // The two velocity nets of a step are independent (reference :119-121): the second one runs on a
  // side stream forked from / joined back into the caller's stream every step, which fills the CUs
  // that one net's small-grid launches (8x8 level, kernel tails) leave idle.
  // (the stream and its fork/join events belong to the device's DevState, created with the first handle)
  DevState* ds = cur_dev();
  if (!ds) return fail(RGFM_EINVAL, "no handle has been created on the current device");
  const bool overlap = g_modes.overlap;
  hipStream_t side = ds->side;
  hipEvent_t ev_fork = ds->fork, ev_join = ds->join;
  // (diagnostics: kernel by kernel -- each stage writes its own records, a replayed graph would write one stage's)
  // (cross pairing: kernel by kernel as well)
  const bool use_graph = p.gstate && g_modes.graph && !g_prof.on && n_mc > 0 && ns >= 4 && solver == SOLVER_EULER && !sink.on() && c.pairing == PAIRING_PAIRED && !strength.is_data() && !c.sde.on() && !c.ess.on();
  // (a strength that is data -- per row or per stage -- runs kernel by kernel: the replayed graph holds one stage's scalars)
  // (the stochastic step: kernel by kernel as well -- its noise key and scalars are launch arguments of the step)
  // (the effective-sample-size floor: kernel by kernel as well -- each stage writes its own block of tau_out)
  const hipStream_t caller = (hipStream_t)c.stream;
  hipStream_t s = caller;
  if (use_graph && caller == nullptr) {  // (see DevState::main)
    s = ds->main;
    HIP_TRY(hipEventRecord(ds->main_fork, caller));
    HIP_TRY(hipStreamWaitEvent(s, ds->main_fork, 0));
  }
  int* step_dev = nullptr;
  float* sched_dev = nullptr;
  if (use_graph) {
    // graphs of earlier calls: release them once the device is past their last replay
    if (!ds->graphs.empty() && hipEventQuery(ds->graph_done) == hipSuccess) {
      for (auto& g : ds->graphs) (void)hipGraphExecDestroy(g.first), (void)hipGraphDestroy(g.second);
      ds->graphs.clear();
    }
    step_dev = reinterpret_cast<int*>(p.gstate);
    sched_dev = p.gstate + 64;
    HIP_TRY(hipMemsetAsync(step_dev, 0, 256, s));
    launch_guid_schedule(sched_dev, step_begin, ns, num_steps, s);
  }
  // one stage: (xout, yout) = (x, y) + dts * F(xin, yin, t), the nets reading time-table row `row`
  auto one_stage = [&](const Stage& g, bool guided) -> int {
    float *xin = g.reads_mid ? p.x_mid : p.x, *yin = g.reads_mid ? p.y_mid : p.y;
    float *xout = g.writes_mid ? p.x_mid : p.x, *yout = g.writes_mid ? p.y_mid : p.y;
    float *vx = p.vx, *vy = p.vy;
    const float *xb = p.x, *yb = p.y;
    float dts = g.dts;
    // (the stochastic step: both pre-updates on `s`, in front of the fork)
    if (int rc = c.sde.stage(g, num_steps, 0, p.x, (size_t)c.batch * p.dx, s, p.x, &xb, &dts)) return rc;
    if (int rc = c.sde.stage(g, num_steps, 1, p.y, (size_t)c.batch * p.dy, s, p.y, &yb, &dts)) return rc;
    hipStream_t sy = overlap ? side : s;
    GuidanceCall gc{.x = xin, .y = yin, .vx = vx, .vy = vy, .mx = p.mc_x1, .my = p.mc_y1, .r = p.mc_ratios,
                    .B = c.batch, .N = n_mc, .dx = p.dx, .dy = p.dy, .t = g.t, .strength = strength.stage(g.row),
                    .scratch = p.scratch, .xs = xout, .ys = yout, .xb = xb, .yb = yb, .dt = dts, .stream = s,
                    .sched = sched_dev, .step_ptr = step_dev, .diag = sink.at(g.row), .pairing = c.pairing,
                    .ess_min = c.ess.floor(), .tau_out = c.ess.at(g.row, c.batch)};
    if (overlap) {
      HIP_TRY(hipEventRecord(ev_fork, s));
      HIP_TRY(hipStreamWaitEvent(side, ev_fork, 0));
    }
    int rc = eval_y(g.row, sy, yin, guided ? vy : nullptr, guided ? nullptr : yout, yb, dts, step_dev);
    if (rc) return rc;
    if (overlap) HIP_TRY(hipEventRecord(ev_join, side));
    rc = eval_x(g.row, s, xin, guided ? vx : nullptr, guided ? nullptr : xout, xb, dts, step_dev);
    if (rc) return rc;
    // The distances to the MC set and the importance weights depend on (x_t, y_t) only (sample_mnist_svhn.py:130-156; a
    // guided step's nets write velocities, the state moves in guid_apply): they go on this stream BEFORE it waits for the
    // other net -- the x net of a pair is the quicker one, so they run in its shadow instead of on the step's critical path
    if (guided && overlap) {
      gc.phase = GuidPhase::Weights;
      if ((rc = guidance_launch(gc))) return rc;
    }
    if (overlap) HIP_TRY(hipStreamWaitEvent(s, ev_join, 0));
    if (guided) {
      gc.phase = overlap ? GuidPhase::Apply : GuidPhase::All;
      if ((rc = guidance_launch(gc))) return rc;
    }
    if (step_dev) launch_step_inc(step_dev, s);
    return RGFM_OK;
  };
  hipGraphExec_t exec = nullptr;
  // On EVERY exit path -- also the error returns inside the loop -- the work already enqueued must stay ordered: the
  // event that guards the destruction of this call's graph is recorded behind its last launch, and the caller's
  // stream is joined behind whatever ran on the device's `main` stream (a stale graph_done could let the
  // next call destroy a graph that is still executing).
  struct ExitGuard {
    DevState* ds;
    hipStream_t s, caller;
    hipGraphExec_t* exec;
    ~ExitGuard() {
      if (*exec) (void)hipEventRecord(ds->graph_done, s);
      if (s != caller) {
        (void)hipEventRecord(ds->main_join, s);
        (void)hipStreamWaitEvent(caller, ds->main_join, 0);
      }
    }
  } exit_guard{ds, s, caller, &exec};
  // (Measured and rejected in round 4, profiles/r04_ab_decoupled_loop.txt: the loop WITHOUT the per-step join -- each
  // modality a chain net -> its half of the guided update on its own stream, coupled only through two events per step
  // around the importance weights, the x net up to one evaluation ahead -- is bit-identical and 0.5 - 0.9 % SLOWER
  // (469 - 471 vs 473 paired images/s, same box, alternating): the join costs nothing the chains could use.)
  const int rc = for_each_stage(solver, num_steps, step_begin, ns, [&](const Stage& st) -> int {
    // `t > eps` test of the reference (:124); a stage whose scale is 0 runs as the unguided stage
    const bool guided = n_mc > 0 && st.t > 1e-3 && !strength.off(st.row);
    if (!(use_graph && guided)) return one_stage(st, guided);
    if (!exec) {  // (Euler: the step's one stage)
      hipGraph_t graph = nullptr;
      HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
      const int rc = one_stage(st, true);
      const hipError_t ce = hipStreamEndCapture(s, &graph);
      if (rc) {  // (a captured graph that will never run: nothing refers to it)
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (ce != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        return fail(RGFM_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
      }
      const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (ie != hipSuccess) {
        exec = nullptr;
        (void)hipGraphDestroy(graph);
        return fail(RGFM_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
      }
      ds->graphs.push_back({exec, graph});
    }
    HIP_TRY(hipGraphLaunch(exec, s));
    return RGFM_OK;
  });
  if (rc) return rc;
  // (the guard's destructor records graph_done and joins `main` into the caller's stream -- on this path too, so that a
  // failing record cannot skip the join)
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
