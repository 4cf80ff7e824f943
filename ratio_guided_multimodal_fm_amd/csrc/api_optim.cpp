// api_optim.cpp -- the optimizer step's host glue: rgfm_adam_workspace_bytes, rgfm_adam_grad_norm, rgfm_adam_step (C ABI:
// include/rgfm.h; kernels: optim.hip).  No handle and no state of its own: the table, the three flat state buffers and
// the workspace (the partial sums of g^2) are the caller's; both calls only validate and enqueue one launch.
#include "train_host.h"

namespace {

constexpr size_t ADAM_WS_BYTES = (size_t)ADAM_PARTIALS * sizeof(double);

int check_table(const rgfm_adam_entry* table_dev, int n_entries, uint64_t span_begin, uint64_t span_end) {
  if (!table_dev) return fail(RGFM_EINVAL, "null table");
  if (n_entries < 1) return fail(RGFM_EINVAL, "the table needs at least one entry, got %d", n_entries);
  if (span_end <= span_begin || span_begin % 4 || span_end % 4)
    return fail(RGFM_EINVAL, "the span [%llu, %llu) must be non-empty and made of whole quads of 4 floats",
                (unsigned long long)span_begin, (unsigned long long)span_end);
  return RGFM_OK;
}

int check_ws(const void* ws, size_t ws_bytes) { return check_train_ws(ADAM_WS_BYTES, ws, ws_bytes, 16); }

int check_device() {  // (the first call on a device: is it a gfx950?)
  return cur_dev() ? RGFM_OK : ensure_init();
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int rgfm_adam_workspace_bytes(size_t* bytes) {
  if (!bytes) return fail(RGFM_EINVAL, "null output");
  *bytes = ADAM_WS_BYTES;
  return RGFM_OK;
}

extern "C" int rgfm_adam_grad_norm(const rgfm_adam_entry* table_dev, int n_entries, uint64_t span_begin, uint64_t span_end,
                                   void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (int rc = check_table(table_dev, n_entries, span_begin, span_end)) return rc;
  if (int rc = check_ws(ws, ws_bytes)) return rc;
  if (int rc = check_device()) return rc;
  launch_adam_norm(table_dev, n_entries, span_begin, span_end, (double*)ws, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}

extern "C" int rgfm_adam_step(const rgfm_adam_desc* d, const rgfm_adam_entry* table_dev, int n_entries, uint64_t span_begin,
                              uint64_t span_end, float* exp_avg, float* exp_avg_sq, float* ema, float* grad_norm_out,
                              void* ws, size_t ws_bytes, rgfm_stream_t stream) {
  if (!d) return fail(RGFM_EINVAL, "null descriptor");
  if (int rc = check_table(table_dev, n_entries, span_begin, span_end)) return rc;
  if (!exp_avg || !exp_avg_sq) return fail(RGFM_EINVAL, "null state buffer");
  if (!aligned16(exp_avg) || !aligned16(exp_avg_sq) || !aligned16(ema))
    return fail(RGFM_EINVAL, "the state buffers must be 16-byte aligned");
  if (!(d->lr >= 0.0) || !std::isfinite(d->lr)) return fail(RGFM_EINVAL, "lr must be finite and >= 0");
  for (double b : d->betas)
    if (!(b >= 0.0 && b < 1.0)) return fail(RGFM_EINVAL, "betas must be in [0, 1)");
  if (!(d->eps >= 0.0)) return fail(RGFM_EINVAL, "eps must be >= 0");
  if (!(d->weight_decay >= 0.0)) return fail(RGFM_EINVAL, "weight_decay must be >= 0");
  if (std::isnan(d->max_grad_norm) || std::isnan(d->ema_decay)) return fail(RGFM_EINVAL, "max_grad_norm / ema_decay is NaN");
  if (d->ema_decay > 1.0) return fail(RGFM_EINVAL, "ema_decay must be <= 1 (negative: no EMA)");
  if ((d->ema_decay >= 0.0) != (ema != nullptr))
    return fail(RGFM_EINVAL, "the ema buffer must be given exactly when ema_decay >= 0");
  const bool need_norm = d->max_grad_norm > 0.0 || grad_norm_out;
  if (need_norm)
    if (int rc = check_ws(ws, ws_bytes)) return rc;
  if (int rc = check_device()) return rc;
  AdamStepArgs a{};
  a.tab = table_dev, a.n = n_entries, a.span_begin = span_begin;
  a.exp_avg = exp_avg, a.exp_avg_sq = exp_avg_sq, a.ema = ema;
  a.partials = need_norm ? (const double*)ws : nullptr, a.grad_norm_out = grad_norm_out;
  a.lr = d->lr;
  a.beta1 = d->betas[0], a.one_minus_beta1 = 1.0 - d->betas[0];
  a.beta2 = d->betas[1], a.one_minus_beta2 = 1.0 - d->betas[1];
  a.decoupled = d->decoupled != 0 && d->weight_decay != 0.0;
  a.wd = d->weight_decay, a.decay_mul = 1.0 - d->lr * d->weight_decay;
  a.max_norm = d->max_grad_norm;
  a.ema_decay = d->ema_decay, a.one_minus_ema_decay = 1.0 - d->ema_decay;
  a.eps = (float)d->eps;
  launch_adam_step(a, span_end, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return RGFM_OK;
}
