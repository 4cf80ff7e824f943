/*
 * rgfm.h -- C ABI of librgfm_hip.so: the MI355X (gfx950) implementation of the
 * ratio-guided flow-matching SAMPLER of foubari/ratio_guided_Multimodal_FM.
 *
 * The reference has no FFI; its boundary for this path is a Python module API.
 * Each entry point below replaces the reference call cited next to it, and is
 * what a ctypes / cffi / pybind stub on the reference side would bind
 * (INTEGRATION.md shows that stub).
 *
 * Conventions
 *   - every pointer named *_dev / x / y / out / ws is a raw DEVICE pointer to
 *     contiguous fp32 data that the CALLER owns (PyTorch: tensor.data_ptr());
 *     the library owns only what *_create allocates and frees it in *_destroy;
 *   - image tensors are NCHW fp32, exactly as the reference passes them;
 *   - `stream` is a hipStream_t (PyTorch: torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it; forward/sample calls neither synchronise nor
 *     allocate nor create streams/events (per-device resources are created by the
 *     first *_create on that device; rgfm_profile_reserve pre-creates the bench
 *     timers' events) and read the RGFM_* environment switches once on entry;
 *   - return value: 0 on success, a negative RGFM_E* code otherwise; nothing is
 *     thrown across the ABI; rgfm_last_error() returns text for the calling
 *     thread's last failure;
 *   - one host thread per handle; distinct handles are independent;
 *   - arithmetic: fp32 tensors, fp32 accumulation.  By default (RGFM_CONV_HX2) the 3x3 /
 *     transposed convolutions EMULATE each fp32 product on the f16 matrix cores: both
 *     (power-of-two scaled) operands are held as two fp16 planes -- 22 significant bits -- and
 *     three of the four plane products are accumulated in fp32 (product
 *     error measured 2^-24.8 median, 2^-20.3 at the 99.9th percentile; one whole U-Net
 *     evaluation against float64: 2.6e-6, the reference's own fp32 run 1.7e-6).  The
 *     representation has a window: activations 2^-8 <= max|a| per wave block and |a| < 2048,
 *     GroupNorm parameters and weights of ordinary magnitude.  Convs whose weights or norm
 *     parameters are outside it are routed to the split-bf16 kernel when the handle is
 *     created; activations outside it raise the handle's range flag (rgfm_unet_range_flag:
 *     bit 0 too large, bit 1 too small), on which the caller repeats the call with the handle
 *     set to RGFM_CONV_BX3 / RGFM_CONV_F32 (rgfm_unet_set_conv_mode) -- the Python host does both.
 *     RGFM_CONV_BX3: exact three-way bf16 split, six products, fp32 exponent range.
 *     RGFM_CONV_F32: v_mfma_f32_32x32x2_f32 for every convolution.
 */
#ifndef RGFM_H_
#define RGFM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGFM_ABI_VERSION 3

#define RGFM_OK 0
#define RGFM_EINVAL (-1)    /* bad argument / unsupported shape          */
#define RGFM_ENOMEM (-2)    /* hipMalloc failed or workspace too small   */
#define RGFM_EHIP (-3)      /* a HIP runtime call failed                 */
#define RGFM_ENODEVICE (-4) /* no gfx950 device visible                  */

#define RGFM_MAX_LEVELS 4

typedef void* rgfm_stream_t; /* hipStream_t */

/* ------------------------------------------------------------------------
 * Velocity U-Net.  Replaces FlexibleUNet / FlowMatchingUNetMNIST /
 * FlowMatchingUNetSVHN (reference src/models/unet_flexible.py:111-291) and
 * UNetMNIST / FlowMatchingUNet (src/models/unet.py:122-305): same
 * architecture parameters, same parameter tensors.
 * ---------------------------------------------------------------------- */
typedef struct rgfm_unet_desc {
  int32_t in_channels;    /* 1 (MNIST) or 3 (SVHN)                                 */
  int32_t img_size;       /* 28 or 32 (square)                                     */
  int32_t model_channels; /* 32 / 64                                               */
  int32_t num_levels;     /* len(channel_mult)                                     */
  int32_t channel_mult[RGFM_MAX_LEVELS];
  int32_t num_res_blocks; /* 2                                                     */
} rgfm_unet_desc;

typedef struct rgfm_unet rgfm_unet;

/* Number of fp32 values in the parameter blob for `desc`: the tensors of the
 * reference module's state_dict(), in state_dict() order, each flattened
 * row-major and concatenated (unet_flexible.py:146-201 registration order). */
int rgfm_unet_param_floats(const rgfm_unet_desc* desc, size_t* n_floats);

/* Builds the device-side packed weights from the state_dict-order blob
 * (replaces module construction + load_state_dict, src/utils/__init__.py:25-51).
 * The blob may be freed once `stream` has been synchronised. */
int rgfm_unet_create(const rgfm_unet_desc* desc, const float* params_dev, size_t n_floats,
                     rgfm_stream_t stream, rgfm_unet** out);
void rgfm_unet_destroy(rgfm_unet* h);

/* Scratch bytes one forward / sample call needs for `batch` rows. */
int rgfm_unet_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes);

/* v_out[B,C,H,W] = model(x[B,C,H,W], t)   (FlexibleUNet.forward,
 * unet_flexible.py:203-261).  t_dev holds t_count in {1, batch} timesteps
 * (t_count == 1: one t shared by every row, as inside the samplers). */
int rgfm_unet_forward(rgfm_unet* h, const float* x, const float* t_dev, int t_count, float* v_out,
                      int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* Debug / parity hook: after a forward, copy activation `index` (the order the
 * tensors are produced in; see rgfm_unet_num_activations) as NCHW fp32 into
 * out_dev.  Only valid when the handle was put in trace mode, which keeps every
 * activation in its own buffer. */
int rgfm_unet_set_trace(rgfm_unet* h, int enable);
/* Parity hook: emb_out[t_count][model_channels] = timestep_embedding(t, model_channels) exactly as the
 * device evaluates it in front of the time MLPs (unet_flexible.py:16-36: cos half first, t unscaled).
 * ws: at least rgfm_unet_workspace_bytes(h, t_count) bytes. */
int rgfm_unet_time_embedding(rgfm_unet* h, const float* t_dev, int t_count, float* emb_out, void* ws,
                             size_t ws_bytes, rgfm_stream_t stream);
int rgfm_unet_num_activations(const rgfm_unet* h, int* n);
/* Debug / test hook: how many ResBlocks of the handle's LATEST network walk handed conv1's output to conv2 in the
 * pre-normalised pre-split "P format" (conv_mfma_hx2d.hip) instead of as an fp32 map.  Lets a
 * test see that the hand-over is really taken (its results are the fp32 hand-over's to the last bit or two). */
int rgfm_unet_p_handovers(const rgfm_unet* h, int* blocks);
/* Debug / test hook: how many convs of the handle's LATEST network walk were described for the Winograd F(2x2, 3x3) kernel
 * (conv_mfma_hx2w.hip; opt-in: RGFM_WINO=1). */
int rgfm_unet_wino_convs(const rgfm_unet* h, int* convs);
/* Debug / test hook: how many convs of the handle's LATEST network walk ran on the Upsample kernel that computes all four
 * parity classes from one staged input tile (conv_mfma_hx2u.hip; RGFM_HX2U=0 switches it off).  They count under route
 * RGFM_ROUTE_HX2P and in slot RGFM_ROUTE_T2 of rgfm_unet_conv_routes, as the launches they replace. */
int rgfm_unet_up_merged(const rgfm_unet* h, int* convs);
/* Debug / test hook: conv launches of the handle's LATEST network walk per kernel route (the dispatch of
 * launch_conv, csrc/rgfm_host.h), plus the launches that ran as the four parity classes of an Upsample (CONV_T2,
 * whichever route took them).  counts[i] for i < min(n, RGFM_ROUTE_SLOTS); the input / output convs are not counted. */
#define RGFM_ROUTE_HX2D 0   /* conv_mfma_hx2d.hip: P-format input                       */
#define RGFM_ROUTE_HX2W 1   /* conv_mfma_hx2w.hip: Winograd F(2x2, 3x3) (RGFM_WINO=1)   */
#define RGFM_ROUTE_HX2S 2   /* conv_mfma_hx2s.hip: stride-2 Downsample                  */
#define RGFM_ROUTE_HX2C 3   /* conv_mfma_hx2c.hip: the 8x8 level                        */
#define RGFM_ROUTE_HX2Q 4   /* conv_mfma_hx2q.hip: four waves per SIMD                  */
#define RGFM_ROUTE_HX2P 5   /* conv_mfma_hx2p.hip: pipelined fp16                       */
#define RGFM_ROUTE_HX2 6    /* conv_mfma_hx2.hip                                        */
#define RGFM_ROUTE_BX3 7    /* conv_mfma_bx3.hip: three bf16 planes                     */
#define RGFM_ROUTE_F32 8    /* conv_mfma.hip: exact fp32 MFMA                           */
#define RGFM_ROUTE_COUNT 9
#define RGFM_ROUTE_T2 9     /* (not a route) launches in the Upsample parity-class form */
#define RGFM_ROUTE_SLOTS 10
int rgfm_unet_conv_routes(const rgfm_unet* h, int* counts, int n);
int rgfm_unet_activation_shape(const rgfm_unet* h, int index, int* channels, int* height, int* width);
int rgfm_unet_read_activation(rgfm_unet* h, int index, int batch, const void* ws, float* out_dev,
                              rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Training pass of the U-Net (replaces the reference's autograd through FlexibleUNet.forward in
 * train_flow_matching_epoch, src/utils/flow_utils.py:103-156).  Exact fp32 arithmetic (v_mfma_f32_32x32x2_f32 for
 * every conv, whatever the handle's conv mode), NCHW boundary tensors, stream-ordered, no synchronisation.
 *
 * rgfm_unet_forward_train evaluates v_out = model(x, t) in TRAINING mode and leaves in `ws` (at least
 * rgfm_unet_train_workspace_bytes(h, batch) bytes, owned by the caller) everything rgfm_unet_backward needs; one ws
 * per forward that is still to be differentiated.  Dropout (every ResBlock, on conv2's input, unet_flexible.py:77-79):
 * element i of the NCHW tensor [batch][cout][H][W] in front of conv2 of ResBlock `block` (ResBlocks counted in the
 * order the forward runs them: encoder, middle, decoder, from 0) is kept, and scaled by 1 / (1 - p_drop), iff
 *     z = seed + 0x9E3779B97F4A7C15 * (((uint64)block << 32 | i) + 1)         (mod 2^64)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
 *     (float)(z >> 40) * 2^-24 >= p_drop
 * (the splitmix64 finaliser); p_drop = 0 applies none.  The backward regenerates the mask instead of storing it.
 *
 * rgfm_unet_backward: given dv = dL/dv_out, writes dL/dx to dx_out (optional, may be null) and dL/dparams to
 * dparams_out -- one blob in the parameter blob's state_dict order, overwritten (not accumulated).  Every reduction
 * has a fixed order: two calls on the same inputs give bitwise-identical results.  The handle's parameters must be
 * those of the forward.
 *
 * rgfm_unet_dropout_mask writes the keep decisions (1.0 / 0.0) of ResBlock `block` for `batch` rows,
 * out[batch][cout][H][W], on the null stream (test hook).
 *
 * rgfm_unet_update_params copies a new state_dict-order blob into the handle and repacks every derived weight image
 * in place (fp32-packed, two-plane, split-bf16, Upsample parity-class, Winograd), without reallocating: what an
 * optimizer step needs before the next eval-mode forward / sample call.  Synchronises `stream` once (as create). */
int rgfm_unet_train_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes);
int rgfm_unet_forward_train(rgfm_unet* h, const float* x, const float* t_dev, int t_count, float* v_out, int batch,
                            float p_drop, uint64_t seed, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_unet_backward(rgfm_unet* h, const float* dv, float* dx_out, float* dparams_out, int batch, void* ws,
                       size_t ws_bytes, rgfm_stream_t stream);
int rgfm_unet_dropout_mask(rgfm_unet* h, int block, uint64_t seed, float p_drop, int batch, float* out);
int rgfm_unet_update_params(rgfm_unet* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Exact log-likelihood of images under the velocity U-Net.  Added functions only: the ABI
 * version is unchanged.  All of it runs on the exact-fp32 training forward (p_drop = 0) and on the DATA-ONLY reverse
 * walk; the two-plane eval arithmetic is not used.  Stream-ordered, nothing allocated or synchronised, nothing
 * graph-captured, every reduction in a fixed order (two calls on the same inputs give the same bits, a row's result
 * depends on its own row only).
 *
 * rgfm_unet_vjp: dx_out = J^T u, J = dv/dx of the forward whose state rgfm_unet_forward_train left in `ws` (same ws,
 * same size query).  It is rgfm_unet_backward's walk restricted to what reaches x: no weight-gradient GEMMs and split-K
 * reductions, no bias / norm-parameter / time-path gradients, no dparams memset.  dx_out has the bits of
 * rgfm_unet_backward's dx_out for dv = u.  The saved state is left untouched: the call may be repeated on it.
 *
 * rgfm_unet_divergence: one forward v = model(x, t) (t_count in {1, batch}) and n_probes reverse walks;
 *     div_out[b] = (1 / K) sum_k <eps_k[b], J^T eps_k[b]>,   eps[K][B][C][H][W] supplied by the caller
 * (Hutchinson's estimate of the trace of J per row; the d probes sqrt(d) e_i give the exact trace).  v_out is optional
 * (may be null).  n_probes = 0 is a plain exact-fp32 forward: div_out is untouched (and may be null, as eps).
 *
 * rgfm_unet_log_prob: data x at t = 1 is integrated BACKWARDS to z = x(0) along dx/dt = v(x, t), and
 *     logp_out[b] = log N(z_b; 0, I) - A[b],   A = integral over [0, 1] of div v(x(t), t) dt.
 * dt = 1 / num_steps; for i = num_steps - 1 ... 0, t_hi = (i + 1) dt, scalars in double and rounded to fp32 where a
 * tensor op consumes them:
 *     RGFM_SOLVER_EULER:     k = v(x, t_hi), D = div(x, t_hi);                                x -= dt k,  A += dt D
 *     RGFM_SOLVER_MIDPOINT:  k1 = v(x, t_hi), x_mid = x - (dt / 2) k1, t_m = t_hi - dt / 2,
 *                            k2 = v(x_mid, t_m), D = div(x_mid, t_m);                         x -= dt k2, A += dt D
 * (midpoint: the divergence is taken at the second stage only; stage 1 is a forward without a reverse walk).  Velocity
 * and divergence of a stage come from ONE forward; the probes are fixed for the whole call; the library draws nothing.
 * x [B,C,H,W] is read-only, z_out [B,C,H,W] and logp_out [B] are written.  n_probes = 0 makes the call an encoder:
 * only z_out is written (the same bits as with probes), logp_out and eps may be null.  At most 4096 Euler steps or
 * 2048 midpoint steps per call.  Argument errors are reported before anything is enqueued, outputs untouched: null
 * pointers, unknown solver, n_probes < 0, num_steps < 1 or above the cap, batch < 1 -> RGFM_EINVAL; a short workspace
 * -> RGFM_ENOMEM. */
int rgfm_unet_vjp(rgfm_unet* h, const float* u, float* dx_out, int batch, void* ws, size_t ws_bytes,
                  rgfm_stream_t stream);
int rgfm_unet_divergence_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes);
int rgfm_unet_divergence(rgfm_unet* h, const float* x, const float* t_dev, int t_count, const float* eps, int n_probes,
                         float* v_out, float* div_out, int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_unet_log_prob_workspace_bytes(const rgfm_unet* h, int batch, int solver, int n_probes, size_t* bytes);
int rgfm_unet_log_prob(rgfm_unet* h, const float* x, const float* eps, int n_probes, int num_steps, int solver,
                       float* z_out, float* logp_out, int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Density-ratio estimators.  Replaces RatioEstimatorMNISTSVHN
 * (src/models/ratio_flexible.py:305-385), RatioEstimator
 * (src/models/ratio_estimator.py:96-191) and FlexibleRatioEstimator
 * (src/models/ratio_flexible.py:69-154), eval mode.
 * ---------------------------------------------------------------------- */
#define RGFM_RATIO_MNIST_SVHN 0 /* x[N,1,32,32], y[N,3,32,32], BatchNorm encoders */
#define RGFM_RATIO_MNIST28 1    /* x[N,1,28,28], y[N,1,28,28], GroupNorm encoders */
/* FlexibleRatioEstimator (rgfm_ratio_flex_desc / rgfm_ratio_flex_create): x[N,x_channels,x_size,x_size],
 * y[N,y_channels,y_size,y_size].  Two GroupNorm ImageEncoders
 * (ratio_flexible.py:13-66: convs of 32, 64, 128, 128 channels, a floor 2x2 max-pool behind the first three, a global
 * average pool, Linear(128, feature_dim)) and the two-hidden-layer score MLP; parameter blob in the order of
 * ratio_flexible.py:22-40 and :100-114.  The module itself is size-agnostic; a handle is built for ONE pair of sizes
 * (the rasters, tilings and workspaces follow from them) -- keep one handle per pair of sizes in use.  Channels 1..4;
 * sizes 8..64 (below 8 the third pool would produce an empty map; 64 is the largest raster the conv kernels tile).
 * The two sizes are independent, the images square.  Every rgfm_ratio_* entry point works on such a handle as on
 * the other kinds. */
#define RGFM_RATIO_FLEXIBLE 2

#define RGFM_LOSS_DISC 0
#define RGFM_LOSS_RULSIF 1

#define RGFM_RATIO_OUT_SCORE 0     /* forward(x, y)                      */
#define RGFM_RATIO_OUT_LOG_RATIO 1 /* log_ratio(x, y)                    */
#define RGFM_RATIO_OUT_RATIO 2     /* log_ratio(x, y).exp()  (mc_ratios) */

typedef struct rgfm_ratio_desc {
  int32_t kind;        /* RGFM_RATIO_*      */
  int32_t feature_dim; /* 256               */
  int32_t hidden_dim;  /* 512               */
  int32_t loss_type;   /* RGFM_LOSS_*       */
} rgfm_ratio_desc;

/* Descriptor of kind RGFM_RATIO_FLEXIBLE; rgfm_ratio_flex_create returns the same rgfm_ratio* as rgfm_ratio_create
 * (which rejects that kind: its descriptor has no geometry).  Added functions only: the ABI version is unchanged. */
typedef struct rgfm_ratio_flex_desc {
  int32_t feature_dim; /* multiple of 64, <= 512  */
  int32_t hidden_dim;  /* multiple of 128, <= 1024 */
  int32_t loss_type;   /* RGFM_LOSS_*       */
  int32_t x_channels;  /* 1..4              */
  int32_t y_channels;  /* 1..4              */
  int32_t x_size;      /* 8..64             */
  int32_t y_size;      /* 8..64             */
} rgfm_ratio_flex_desc;

typedef struct rgfm_ratio rgfm_ratio;

int rgfm_ratio_param_floats(const rgfm_ratio_desc* desc, size_t* n_floats);
/* Blob = state_dict() order, fp32; BatchNorm `num_batches_tracked` entries are
 * carried as one fp32 each (value ignored) so that offsets follow the keys. */
int rgfm_ratio_create(const rgfm_ratio_desc* desc, const float* params_dev, size_t n_floats,
                      rgfm_stream_t stream, rgfm_ratio** out);
int rgfm_ratio_flex_param_floats(const rgfm_ratio_flex_desc* desc, size_t* n_floats);
int rgfm_ratio_flex_create(const rgfm_ratio_flex_desc* desc, const float* params_dev, size_t n_floats,
                           rgfm_stream_t stream, rgfm_ratio** out);
void rgfm_ratio_destroy(rgfm_ratio* h);
int rgfm_ratio_workspace_bytes(const rgfm_ratio* h, int n, size_t* bytes);
/* out[n] per `what` (RGFM_RATIO_OUT_*): forward ratio_flexible.py:347-364,
 * log_ratio :366-385, and the .exp() of sample_mnist_svhn.py:110-111. */
int rgfm_ratio_eval(rgfm_ratio* h, const float* x, const float* y, float* out, int n, int what,
                    void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* Cross evaluation: out[nx][ny], row-major, is `what` (RGFM_RATIO_OUT_*) of EVERY pair (x_i, y_j) -- the matrix that
 * conditional sampling needs (each condition image against each Monte-Carlo sample), which rgfm_ratio_eval gives only
 * for the nx * ny explicitly tiled pairs.  Every kind.  Each encoder runs once (nx and ny images); the first score
 * Linear acts on the concatenation [f_x | f_y], so W [f_x | f_y] + b = W[:, :F] f_x + W[:, F:] f_y + b is two small
 * products per image and a sum per pair; the rest of the MLP runs over the pairs in chunks of a fixed number of pair
 * indices (a library constant, independent of nx and ny: the workspace is bounded by the encoders and one chunk; a
 * chunk may begin and end inside a matrix row).  RGFM_CROSS_ROWS=<pairs per chunk> overrides the constant (test hook,
 * read on entry of both functions; results do not depend on it).  nx, ny >= 1.  Results agree with rgfm_ratio_eval on
 * the tiled pairs to fp32 rounding (another summation order in the first Linear), not bitwise. */
int rgfm_ratio_cross_workspace_bytes(const rgfm_ratio* h, int nx, int ny, size_t* bytes);
int rgfm_ratio_eval_cross(rgfm_ratio* h, const float* x, int nx, const float* y, int ny, float* out, int what,
                          void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* Gradient of the log-ratio, d log_ratio(x, y) / d(x, y): what torch.autograd.grad(model.log_ratio(x, y).sum(),
 * (x, y)) returns for the reference module in eval mode (ratio_flexible.py:347-385, ratio_estimator.py:137-191;
 * hand-written reverse pass).  RGFM_RATIO_MNIST_SVHN: gx[n,1,32,32], gy[n,3,32,32]; RGFM_RATIO_MNIST28: gx, gy
 * [n,1,28,28]; RGFM_RATIO_FLEXIBLE: gx[n,x_channels,x_size,x_size], gy[n,y_channels,y_size,y_size]; log_ratio_out
 * (optional) [n]. */
int rgfm_ratio_grad_workspace_bytes(const rgfm_ratio* h, int n, size_t* bytes);
int rgfm_ratio_grad_log_ratio(rgfm_ratio* h, const float* x, const float* y, float* gx, float* gy,
                              float* log_ratio_out, int n, void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* The same gradient for ONE side with the other side held fixed (conditional sampling: the observed image never
 * moves).  `given` = 0: the condition is the estimator's x and the target its y; 1: the other way round.  Every kind.
 *
 * rgfm_ratio_cond_prepare: ctx_out[n][hidden_dim] = W1[:, given slice] f_given(cond) + b1 -- the given side's encoder,
 * once, and its half of the first score Linear (W1 acts on the concatenation [f_x | f_y]; the factorisation of
 * rgfm_ratio_eval_cross), bias folded in.  A context belongs to the parameters it was prepared with: prepare again
 * after rgfm_ratio_update_params.
 *
 * rgfm_ratio_grad_log_ratio_cond: g_target = d log_ratio(x, y) / d target, row b pairing ctx[b] with target[b]
 * (target and g_target in the target side's image shape, log_ratio_out optional [n]).  Only the target's encoder runs,
 * forward and reverse; the first hidden layer is LayerNorm + SiLU of ctx + W1[:, target slice] f_target, and its input
 * gradient is taken for the target's feature columns alone.  The sum ctx + W1[:, target slice] f_target associates
 * differently from the 2 feature_dim long dot products of rgfm_ratio_grad_log_ratio, so the two agree to fp32 rounding,
 * not bitwise.  Every reduction has a fixed order: two calls on the same inputs give identical bits.  Exact fp32 convs. */
int rgfm_ratio_cond_prepare_workspace_bytes(const rgfm_ratio* h, int given, int n, size_t* bytes);
int rgfm_ratio_cond_prepare(rgfm_ratio* h, const float* cond, int given, int n, float* ctx_out, void* ws,
                            size_t ws_bytes, rgfm_stream_t stream);
int rgfm_ratio_grad_cond_workspace_bytes(const rgfm_ratio* h, int given, int n, size_t* bytes);
int rgfm_ratio_grad_log_ratio_cond(rgfm_ratio* h, const float* ctx, int given, const float* target, float* g_target,
                                   float* log_ratio_out, int n, void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* Training pass of the ratio estimators (exact fp32 arithmetic on v_mfma_f32_32x32x2_f32, NCHW fp32 tensors,
 * stream-ordered, caller-owned workspace, nothing allocated or synchronised inside a call; every kind).
 *
 * rgfm_ratio_forward_train writes score_out[n] = forward(x, y) and leaves in `ws` what rgfm_ratio_backward needs; `ws`
 * (rgfm_ratio_train_workspace_bytes(h, n)) must stay untouched between the two calls.
 *   training != 0: BatchNorm normalises with the batch mean and the biased batch variance (eps 1e-5), and Dropout is
 *     applied behind the SiLU of the score MLP where the reference has a Dropout layer (the first two hidden layers
 *     of either estimator): element i of [n][width] of Dropout layer `block` (counted from 0) is kept by the counter
 *     hash documented for rgfm_unet_dropout_mask, kept values are scaled by 1 / (1 - p_drop), and the backward
 *     regenerates the mask.  bn_stats_out (may be null; ignored for RGFM_RATIO_MNIST28) receives per BatchNorm layer,
 *     in state_dict order, [C][2] = (batch mean, UNBIASED batch variance): what the running-statistics update needs.
 *   training == 0: running statistics, no dropout, still differentiable.
 * rgfm_ratio_backward: given dscore = dL/dscore_out, writes dL/dx and dL/dy (each optional) and dL/dparams -- one blob
 * in state_dict order, overwritten; the slots of running_mean, running_var and num_batches_tracked are zero.  Every
 * reduction has a fixed order: two calls on the same inputs give bitwise-identical results.
 * rgfm_ratio_pool_choice (test hook, null stream): for max-pool `pool` of encoder `encoder` (0 = x, 1 = y), the
 * window element (0..3, row-major) that the forward which filled `ws` chose and the backward routes to, as
 * out[n][C][Ho][Wo] floats; ties go to the first element in row-major order, as in PyTorch.
 * rgfm_ratio_dropout_mask (test hook, null stream): keep decisions (1.0 / 0.0) of Dropout layer `block`, out[n][width].
 * rgfm_ratio_update_params copies a new state_dict-order blob into the handle and repacks every derived image in
 * place (fp32-packed and two-plane conv weights, the transposed weights of rgfm_ratio_grad_log_ratio, the folded
 * BatchNorm scale/shift).  Synchronises `stream` once (as create). */
int rgfm_ratio_train_workspace_bytes(const rgfm_ratio* h, int n, size_t* bytes);
int rgfm_ratio_forward_train(rgfm_ratio* h, const float* x, const float* y, float* score_out, int n, int training,
                             float p_drop, uint64_t seed, float* bn_stats_out, void* ws, size_t ws_bytes,
                             rgfm_stream_t stream);
int rgfm_ratio_backward(rgfm_ratio* h, const float* dscore, float* dx_out, float* dy_out, float* dparams_out, int n,
                        void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_ratio_pool_choice(rgfm_ratio* h, const void* ws, int encoder, int pool, int n, float* out);
int rgfm_ratio_dropout_mask(rgfm_ratio* h, int block, uint64_t seed, float p_drop, int n, float* out);
int rgfm_ratio_update_params(rgfm_ratio* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Samplers (the Euler/ODE loops).
 * ---------------------------------------------------------------------- */

/* Unguided Euler integration of one model, in place on x_inout[B,C,H,W]:
 *   for step in [step_begin, step_end): t = step*(1/num_steps);
 *       x <- x + model(x, t) * dt
 * Replaces CFMSchedule.sample (src/utils/flow_utils.py:69-100) and each MC
 * pre-phase loop (src/sample_mnist_svhn.py:90-95, :99-104;
 * flow_utils.py:236-241, :245-250). */
int rgfm_sample_single_workspace_bytes(const rgfm_unet* h, int batch, size_t* bytes);
int rgfm_sample_single(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin,
                       int step_end, void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* Paired Euler loop with optional MC importance-weighted guidance, in place on
 * x_inout[B,Cx,H,W], y_inout[B,Cy,H,W].  Replaces the main loop of
 * sample_bimodal_guided_mnist_svhn (src/sample_mnist_svhn.py:114-175) and of
 * sample_bimodal_guided (src/utils/flow_utils.py:263-373).
 *   mc_x1[N,..], mc_y1[N,..], mc_ratios[N]: terminal MC set; pass n_mc = 0 (and
 *   null pointers) for guidance_method == 'none'.
 *   gamma = guidance_strength (not clamped).  Guidance is applied on steps with
 *   t = step/num_steps > 1e-3, as in the reference.
 *   The two networks of a step are independent; the second one is enqueued on a
 *   library-owned side stream that is forked from and joined back into `stream`
 *   with events every step (RGFM_OVERLAP=0 keeps everything on `stream`), so the
 *   call is still ordered with respect to `stream` on entry and on return. */
int rgfm_sample_pair_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc,
                                     size_t* bytes);
int rgfm_sample_pair(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout,
                     const float* mc_x1, const float* mc_y1, const float* mc_ratios, int n_mc,
                     int batch, int num_steps, double gamma, int step_begin, int step_end, void* ws,
                     size_t ws_bytes, rgfm_stream_t stream);

/* Conditional sampling: one modality given images of the other.  Euler loop of ONE net, in place on
 * s_inout[B,C,H,W], guided by the MC block of sample_mnist_svhn.py:124-171 with one side observed:
 *   mc_set[N,C,H,W]: the target net's own unguided samples (the pre-phase of :89-104);
 *   ratios[B][N]:    r(c_b, m_j) = exp(log_ratio) of condition image c_b against MC sample m_j (rgfm_ratio_eval_cross
 *                    with RGFM_RATIO_OUT_RATIO; transposed when the condition is the estimator's y argument).
 * Each step with t = step/num_steps > 1e-3: logp[b][j] = -0.5 |s_b - t m_j|^2 / sigma^2, p = exp(logp - max_j),
 * w = (R / mean_j(R p)) (p / mean_j p) row-normalised, g = sum_j w[b][j] (m_j - s_b) / (1 - t + eps),
 * v = (1 - gamma) v + gamma g, s += v dt -- the epsilons and scalar roundings of the paired block.  This IS the paired
 * block with the observed side's Gaussian factor dropped (it does not depend on j, so it cancels in the normalised
 * weights) and the shared ratio vector replaced by a ratio row per sample; the same kernels run it.
 * Conventions of rgfm_sample_pair: in place, stream-ordered, nothing allocated or synchronised, 1 <= n_mc <= 4096, at
 * most 4096 steps per call.  Steps with t <= 1e-3 use the fused Euler epilogue as rgfm_sample_single does.  Every
 * launch goes to `stream`: one net has nothing to overlap, so there is no side stream and no graph replay. */
int rgfm_sample_cond_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, size_t* bytes);
int rgfm_sample_cond(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                     int num_steps, double gamma, int step_begin, int step_end, void* ws, size_t ws_bytes,
                     rgfm_stream_t stream);

/* Paired Euler loop with GRADIENT LOG-RATIO guidance, in place: every step
 *     x <- x + (v_x(x, t) + gamma * d log r(x, y)/dx) dt,   y likewise
 * (reference README.md:159-164, "v_guided = v_ind + gamma * grad log r(x_t, y_t)").  The reference ships no code
 * for this mode, so the composition above is this library's reading of that line; the gradient itself is the
 * autograd gradient of the reference module (rgfm_ratio_grad_log_ratio).  The pair must be the estimator's:
 * 1x32x32 + 3x32x32 (RGFM_RATIO_MNIST_SVHN), 1x28x28 + 1x28x28 (RGFM_RATIO_MNIST28), or the descriptor's
 * (x_channels, x_size) + (y_channels, y_size) (RGFM_RATIO_FLEXIBLE). */
int rgfm_sample_pair_grad_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr,
                                          int batch, size_t* bytes);
int rgfm_sample_pair_grad(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout,
                          int batch, int num_steps, double gamma, int step_begin, int step_end, void* ws,
                          size_t ws_bytes, rgfm_stream_t stream);

/* Conditional sampling with GRADIENT LOG-RATIO guidance: the one-sided reading of rgfm_sample_pair_grad.  Euler loop
 * of ONE net, in place on s_inout[B,C,H,W]; every step
 *     s <- s + (v(s, t) + gamma * d log r / d s) dt
 * with the observed side entering through ctx[B][hidden_dim] (rgfm_ratio_cond_prepare, once per condition batch) and
 * the gradient that of rgfm_ratio_grad_log_ratio_cond.  No MC set, no pre-phase.  The target U-Net must have the
 * estimator's shape for the side that is NOT given.  Conventions of rgfm_sample_cond: in place, stream-ordered, nothing
 * allocated or synchronised, at most 4096 steps per call, every launch on `stream` (no side stream, no graph).  The
 * estimator's convs follow the target net's conv arithmetic and raise its range flag, as in rgfm_sample_pair_grad. */
int rgfm_sample_cond_grad_workspace_bytes(const rgfm_unet* h_unet, const rgfm_ratio* h_ratio, int given, int batch,
                                          size_t* bytes);
int rgfm_sample_cond_grad(rgfm_unet* h_unet, rgfm_ratio* h_ratio, float* s_inout, const float* ctx, int given,
                          int batch, int num_steps, double gamma, int step_begin, int step_end, void* ws,
                          size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Choice of ODE solver for the U-Net sampler loops.  Added functions only: the ABI version is unchanged.
 *
 * Each rgfm_sample_*_ode is its Euler namesake above with `int solver` in front of `ws`; each workspace query takes
 * `solver` in front of `bytes`.  RGFM_SOLVER_EULER runs the very loop of the old entry point (same launches, same
 * workspace size, same bits); the old entry points are that case.
 *
 * RGFM_SOLVER_MIDPOINT (explicit midpoint rule, second order): step i of num_steps, dt = 1.0 / num_steps,
 *     t1 = i dt          k1 = F(s, t1)       s_mid = s + (dt / 2) k1
 *     t2 = (i + 0.5) dt  k2 = F(s_mid, t2)   s     = s + dt k2
 * with F the loop's WHOLE guided velocity at the stage's own state and time, scalars in double and rounded to fp32
 * where a tensor op consumes them (as in the Euler loops):
 *   - single, and pair with n_mc = 0: F is the network output;
 *   - MC guidance (pair, cond): F = (1 - gamma) v + gamma g with the distances, importance weights, sigma_t and
 *     1 - t + eps all taken at the stage's state and time; a stage is guided iff ITS OWN time is > 1e-3 (stage 1 of
 *     step 0 never is; stage 2 of step 0 is whenever 0.5 / num_steps > 1e-3);
 *   - gradient guidance (pair_grad, cond_grad): F = v + gamma grad log r at the stage's state; in the paired loops both
 *     modalities advance stage by stage, stage 2 sees (x_mid, y_mid).
 * No stage is ever evaluated at t = 1 (where the MC guidance's 1 / (1 - t + eps) is 1000).  Two network evaluations
 * per step.  The update epilogues (out-conv, guid_apply, euler_grad) read the stage's start state from one buffer and
 * write another: no copies on the step path.
 *
 * Conventions of the Euler loops: in place on the caller's state, [step_begin, step_end) counts WHOLE steps (running
 * [0, k) then [k, n) gives the bits of [0, n)), stream-ordered, nothing allocated or synchronised, a row's result
 * depends on its own row only.  The paired loops fork and join the side stream once per STAGE.
 * Workspace: the Euler workspace plus one mid-state buffer per modality (a workspace sized by the Euler query is
 * RGFM_ENOMEM for a midpoint call).
 * Step cap: the time table of a call holds 4096 rows and a midpoint step takes two (t1 and t2: the table of the
 * 2 num_steps half-steps), so a midpoint call covers at most 2048 steps -- RGFM_EINVAL beyond that; split the range.
 * RGFM_GRAPH=1: a midpoint call runs kernel by kernel, nothing is captured or replayed (graph replay is Euler only).
 * An unknown `solver` is RGFM_EINVAL before anything is enqueued: the state is untouched.
 * The FlowMatchingModel loops (rgfm_fmnet_sample_*) are Euler only.
 * ---------------------------------------------------------------------- */
#define RGFM_SOLVER_EULER 0
#define RGFM_SOLVER_MIDPOINT 1
int rgfm_sample_single_ode_workspace_bytes(const rgfm_unet* h, int batch, int solver, size_t* bytes);
int rgfm_sample_single_ode(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin, int step_end,
                           int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_ode_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver,
                                         size_t* bytes);
int rgfm_sample_pair_ode(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                         const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                         int step_begin, int step_end, int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_ode_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, int solver, size_t* bytes);
/* Two independent unguided integrations in one call (the MC pre-phase of the paired sampler): x under hx and y under hy,
 * each with its own row count, with the bits of two rgfm_sample_single_ode calls.  The two chains run side by side, x
 * on `stream` and y on the device state's side stream (forked from and joined back into `stream`), enqueued step by
 * step; the chain with less conv work per step (by the descriptors and row counts, not by argument position) is never
 * more than one step ahead of the other (RGFM_PREPHASE_PRIO=0: one chain enqueued after the other, unpaced).  hx == hy
 * is allowed.
 * Added functions only: the ABI version is unchanged. */
int rgfm_sample_two_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch_x, int batch_y, int solver,
                                    size_t* bytes);
int rgfm_sample_two(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, int batch_x, int batch_y, int num_steps,
                    int step_begin, int step_end, int solver, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_ode(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                         int num_steps, double gamma, int step_begin, int step_end, int solver, void* ws,
                         size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_grad_ode_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr,
                                              int batch, int solver, size_t* bytes);
int rgfm_sample_pair_grad_ode(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout,
                              int batch, int num_steps, double gamma, int step_begin, int step_end, int solver,
                              void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_grad_ode_workspace_bytes(const rgfm_unet* h_unet, const rgfm_ratio* h_ratio, int given,
                                              int batch, int solver, size_t* bytes);
int rgfm_sample_cond_grad_ode(rgfm_unet* h_unet, rgfm_ratio* h_ratio, float* s_inout, const float* ctx, int given,
                              int batch, int num_steps, double gamma, int step_begin, int step_end, int solver,
                              void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------ FlowMatchingModel ("--model original")
 * The reference's encoder-decoder velocity net (src/models/flow_matching.py:127-173;
 * built by src/sample.py:152-154 and src/evaluate.py:144-146) for 1x28x28 images:
 * ImageEncoder (:34-72: four 3x3 convs, two of them stride 2, GroupNorm(8)+SiLU,
 * Linear 12544->feature_dim), SinusoidalPositionEmbeddings (:11-31) and
 * VelocityDecoder (:75-124: Linear, two ConvTranspose2d(k4,s2,p1), 3x3 convs).
 * Same conventions as rgfm_unet_*: blob = state_dict() order, NCHW boundary tensors,
 * caller-owned workspace, stream-ordered, no synchronisation. */
typedef struct rgfm_fmnet_desc {
  int32_t img_channels; /* 1   (FlowMatchingModel.__init__ argument, :138) */
  int32_t feature_dim;  /* 256 */
  int32_t time_emb_dim; /* 128 */
} rgfm_fmnet_desc;

typedef struct rgfm_fmnet rgfm_fmnet;

int rgfm_fmnet_param_floats(const rgfm_fmnet_desc* desc, size_t* n_floats);
int rgfm_fmnet_create(const rgfm_fmnet_desc* desc, const float* params_dev, size_t n_floats,
                      rgfm_stream_t stream, rgfm_fmnet** out);
void rgfm_fmnet_destroy(rgfm_fmnet* h);
/* bytes for one forward or one rgfm_fmnet_sample_single call at this batch */
int rgfm_fmnet_workspace_bytes(const rgfm_fmnet* h, int batch, size_t* bytes);
/* v_out[B,1,28,28] = model(x, t)  (FlowMatchingModel.forward, :153-173); t_count in {1, batch} */
int rgfm_fmnet_forward(rgfm_fmnet* h, const float* x, const float* t_dev, int t_count, float* v_out,
                       int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream);
/* CFMSchedule.sample / the unguided Euler loops of flow_utils.py:69-100, :186-278 with this net */
int rgfm_fmnet_sample_single(rgfm_fmnet* h, float* x_inout, int batch, int num_steps, int step_begin,
                             int step_end, void* ws, size_t ws_bytes, rgfm_stream_t stream);
/* paired_sampler (flow_utils.py:186-278) with two FlowMatchingModel nets: as rgfm_sample_pair */
int rgfm_fmnet_sample_pair_workspace_bytes(const rgfm_fmnet* hx, const rgfm_fmnet* hy, int batch,
                                           int n_mc, size_t* bytes);
int rgfm_fmnet_sample_pair(rgfm_fmnet* hx, rgfm_fmnet* hy, float* x_inout, float* y_inout,
                           const float* mc_x1, const float* mc_y1, const float* mc_ratios, int n_mc,
                           int batch, int num_steps, double gamma, int step_begin, int step_end,
                           void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* Training pass of FlowMatchingModel (replaces the reference's autograd through FlowMatchingModel.forward in
 * src/train_flow.py --model original).  Same conventions as the U-Net's training pass: exact fp32 arithmetic on
 * v_mfma_f32_32x32x2_f32 whatever the handle's conv mode, NCHW fp32 boundary tensors, stream-ordered, caller-owned
 * workspace, nothing allocated or synchronised inside forward_train / backward.  The net has no Dropout and no batch
 * statistics, so training and eval semantics coincide.
 *
 * rgfm_fmnet_forward_train writes v_out[batch,1,28,28] = model(x, t) (t_count = 1: one t for every row, or batch) and
 * leaves in `ws` (at least rgfm_fmnet_train_workspace_bytes(h, batch) bytes) what rgfm_fmnet_backward needs: x, every
 * layer's raw output, the (mean, rstd) pairs of the seven GroupNorms and the [features | t_emb] concat.  One ws per
 * forward that is still to be differentiated; it must stay untouched between the two calls.
 *
 * rgfm_fmnet_backward: given dv = dL/dv_out, writes dL/dx to dx_out (optional, may be null) and dL/dparams to
 * dparams_out -- one blob in the parameter blob's state_dict order, overwritten (not accumulated); t gets no
 * gradient.  Both ConvTranspose2d(4, 2, 1) layers and both Linears (12544 -> feature_dim, feature_dim + time_emb_dim
 * -> 12544) run on the fp32 MFMA in all three roles.  Every reduction has a fixed order (split-K partial slices added
 * in split order, no float atomics): two calls on the same inputs give bitwise-identical results.  The handle's
 * parameters must be those of the forward.
 *
 * rgfm_fmnet_update_params copies a new state_dict-order blob into the handle and repacks every derived image in
 * place -- everything rgfm_fmnet_create packs: the fp32-packed, two-plane and split-bf16 conv and transposed-conv
 * images, the Linear weights and bias re-indexed to NHWC, conv_out's layout -- without reallocating: what an optimizer
 * step needs before the next forward / sample call.  Synchronises `stream` (as create). */
int rgfm_fmnet_train_workspace_bytes(const rgfm_fmnet* h, int batch, size_t* bytes);
int rgfm_fmnet_forward_train(rgfm_fmnet* h, const float* x, const float* t_dev, int t_count, float* v_out,
                             int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_fmnet_backward(rgfm_fmnet* h, const float* dv, float* dx_out, float* dparams_out, int batch, void* ws,
                        size_t ws_bytes, rgfm_stream_t stream);
int rgfm_fmnet_update_params(rgfm_fmnet* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream);

/* ------------------------------------------------------------------ evaluation classifiers (training pass)
 * The three digit classifiers of the coherence metric (reference src/models/classifier.py:9-52: MNISTClassifier,
 * 1x28x28; src/models/svhn_classifier.py:74-116: MNISTClassifier32, 1x32x32; :11-71: SVHNClassifier, 3x32x32 with
 * BatchNorm2d behind every conv): conv3x3 (+ BatchNorm) + ReLU blocks, a 2x2 max-pool behind the first two, fc1 + ReLU
 * + Dropout, fc2 -> 10 logits.  Replaces the autograd of src/train_classifier.py and
 * src/train_classifiers_mnist_svhn.py.  Same conventions as the ratio estimators' training pass: blob = state_dict()
 * order INCLUDING the BatchNorm buffers, exact fp32 arithmetic on v_mfma_f32_32x32x2_f32 (convs, fc1), NCHW fp32
 * tensors, stream-ordered, caller-owned 16-byte aligned workspace, nothing allocated or synchronised inside a call.
 * Added functions only: the ABI version is unchanged.
 *
 * rgfm_clf_forward_train writes logits_out[n][10] = forward(x) and leaves in `ws` what rgfm_clf_backward needs; `ws`
 * (rgfm_clf_train_workspace_bytes(h, n)) must stay untouched between the two calls.
 *   training != 0: BatchNorm normalises with the batch mean and the biased batch variance (eps 1e-5); Dropout behind
 *     fc1's ReLU keeps element i of [n][hidden] by the counter hash documented for rgfm_unet_dropout_mask (Dropout
 *     layer 0), scales kept values by 1 / (1 - p_drop), and the backward regenerates the mask.  bn_stats_out (may be
 *     null; unused by the two MNIST nets) receives per BatchNorm layer, in state_dict order, [C][2] = (batch mean,
 *     UNBIASED batch variance): what the running-statistics update needs.
 *   training == 0: running statistics, no dropout, still differentiable.
 * The ReLU gate is `value > 0` (a value of exactly 0 gets no gradient) and a max-pool takes the first maximal element
 * of its window in row-major order, both as in PyTorch.
 * rgfm_clf_backward: given dlogits = dL/dlogits_out, writes dL/dx (optional) and dL/dparams -- one blob in state_dict
 * order, overwritten; the slots of running_mean, running_var and num_batches_tracked are zero.  Every reduction has a
 * fixed order: two calls on the same inputs give bitwise-identical results.
 * rgfm_clf_xent: softmax cross-entropy of logits[n][classes] (classes <= 32) against int32 labels, every row shifted
 * by its own maximum: loss_rows_out[n] (DOUBLES: at logits of magnitude 10^2 an fp32 row loss could not hold the
 * accuracy of the softmax itself), dlogits_out[n][classes] = (softmax - onehot) * scale (optional) and pred_out[n] =
 * argmax, the first index on a tie (optional).  No reduction across rows: the mean is the caller's scale = 1 / n and
 * its own sum of the rows.  Needs no handle.
 * Test hooks (null stream), for the forward that filled `ws`: rgfm_clf_pool_choice -- the window element (0..3,
 * row-major) the max-pool behind conv block `layer` (0-based) took, as out[n][C][Ho][Wo] floats; rgfm_clf_gate -- 1.0
 * where the ReLU of `layer` passed, else 0.0: for a conv block on the block's OUTPUT raster (behind a pool: the gate
 * of the element taken), for layer == number of conv blocks fc1's ReLU, out[n][hidden], before the dropout;
 * rgfm_clf_dropout_mask -- the keep decisions (1.0 / 0.0) of the Dropout layer, out[n][hidden].
 * Errors touch no state: n < 1, a null pointer or an unknown kind -> RGFM_EINVAL; a workspace one byte short ->
 * RGFM_ENOMEM; no gfx950 device -> RGFM_ENODEVICE (create, xent). */
#define RGFM_CLF_MNIST28 0
#define RGFM_CLF_MNIST32 1
#define RGFM_CLF_SVHN 2
typedef struct rgfm_clf_desc {
  int32_t kind; /* RGFM_CLF_* */
} rgfm_clf_desc;

typedef struct rgfm_clf rgfm_clf;

int rgfm_clf_param_floats(const rgfm_clf_desc* desc, size_t* n_floats);
int rgfm_clf_create(const rgfm_clf_desc* desc, const float* params_dev, size_t n_floats, rgfm_stream_t stream,
                    rgfm_clf** out);
void rgfm_clf_destroy(rgfm_clf* h);
int rgfm_clf_update_params(rgfm_clf* h, const float* params_dev, size_t n_floats, rgfm_stream_t stream);
int rgfm_clf_train_workspace_bytes(const rgfm_clf* h, int n, size_t* bytes);
int rgfm_clf_forward_train(rgfm_clf* h, const float* x, float* logits_out, int n, int training, uint64_t seed,
                           float p_drop, float* bn_stats_out, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_clf_backward(rgfm_clf* h, const float* dlogits, float* dx_out, float* dparams_out, int n, void* ws,
                      size_t ws_bytes, rgfm_stream_t stream);
int rgfm_clf_xent(const float* logits, const int32_t* labels, int n, int classes, float scale, double* loss_rows_out,
                  float* dlogits_out, int32_t* pred_out, rgfm_stream_t stream);
int rgfm_clf_pool_choice(rgfm_clf* h, const void* ws, int layer, int n, float* out);
int rgfm_clf_gate(rgfm_clf* h, const void* ws, int layer, int n, float* out);
int rgfm_clf_dropout_mask(rgfm_clf* h, uint64_t seed, float p_drop, int n, float* out);

/* ------------------------------------------------------------------ optimizer step (Adam / AdamW, clip, weight EMA)
 * The step around the four training passes: torch.optim.Adam(amsgrad=False, maximize=False) -- AdamW when `decoupled`
 * -- with torch.nn.utils.clip_grad_norm_'s global-norm clip in front and an exponential moving average of the weights
 * behind, as two launches over a table of tensors.  Needs no handle.  Added functions only: the ABI version is unchanged.
 *
 * State.  The caller owns three flat fp32 device buffers, 16-byte aligned: exp_avg, exp_avg_sq and (optional) ema.
 * Tensor e owns floats [offset, offset + numel) of each; every offset is a multiple of 4 and slots do not overlap (so
 * a slot is padded to whole quads of 4 floats; the padding is read and written back unchanged: keep it inside the
 * buffers).
 *
 * Table.  `table_dev` is a DEVICE array of n_entries rgfm_adam_entry, sorted by strictly increasing offset.  param and
 * grad are contiguous fp32 device tensors of numel floats at ANY 4-byte alignment (gradients are typically views into
 * one blob): 16-byte accesses are issued only for a quad whose tensor has both base pointers 16-byte aligned, dword
 * accesses otherwise.  bc1 = 1 - beta1^t and bc2 = 1 - beta2^t are THIS tensor's bias corrections for its own step
 * count t >= 1, computed by the caller in double (a parameter without a gradient is left out of the table and keeps
 * its count).  span_begin / span_end (multiples of 4, span_begin <= the first offset, span_end >= the end of the last
 * slot) name the flat range the table covers, which the host cannot read from the device table.
 * Stream ordering: the calls READ THE TABLE ON THE STREAM, not on entry -- the caller keeps table_dev alive and
 * unmodified until the work enqueued by the call has run (a table uploaded by an asynchronous copy on the same stream
 * is fine; so is overwriting it by a later copy on that stream).
 *
 * rgfm_adam_grad_norm: leaves in `ws` (rgfm_adam_workspace_bytes; 16-byte aligned) the partial sums of g^2 over every
 * tensor of the table: squares and sums in float64, one partial per workgroup, a fixed chunk-to-workgroup assignment,
 * no atomics -- the same bits on every run.  Called ONCE over the union of all parameter groups' tensors.
 * rgfm_adam_step: then per group (each with its own lr / weight_decay; the table of a group is a sub-range of the
 * union's).  With norm = sqrt(sum of the partials) (every workgroup adds them in the same order) and
 *   coef = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6)) : 1        (clip_grad_norm_'s formula)
 * it does per element, in one pass (36 bytes per element with the EMA, 28 without):
 *   g = coef g;   coupled: g += weight_decay p;   decoupled: p *= 1 - lr weight_decay;
 *   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps);
 *   ema = ema_decay ema + (1 - ema_decay) p                                      (ema_decay >= 0)
 * Products and sums in float64, each stored value rounded to fp32 once; the square root and the quotient in fp32.  The
 * gradients are NOT modified (clip_grad_norm_ scales them in place).  `ws` is read when max_grad_norm > 0 or
 * grad_norm_out is given (the norm call must then precede on the stream) and may be null otherwise; grad_norm_out
 * (optional device float) receives the norm before clipping.  max_grad_norm = infinity reports the norm without
 * clipping.  `ema` must be given exactly when ema_decay >= 0.
 * Errors touch no state: a null descriptor, table, state buffer or needed workspace, n_entries < 1, a span that is
 * empty or not a multiple of 4, a misaligned state buffer or workspace, lr < 0, betas outside [0, 1), eps < 0,
 * weight_decay < 0, ema_decay > 1 or ema / ema_decay given one without the other -> RGFM_EINVAL; a workspace too small
 * -> RGFM_ENOMEM; no gfx950 device -> RGFM_ENODEVICE. */
typedef struct rgfm_adam_entry { /* 48 bytes */
  float* param;
  const float* grad;
  uint64_t offset; /* first float of the tensor's slot in exp_avg / exp_avg_sq / ema; a multiple of 4 */
  uint64_t numel;
  double bc1, bc2; /* 1 - beta1^t, 1 - beta2^t for this tensor's step count t */
} rgfm_adam_entry;

typedef struct rgfm_adam_desc {
  double lr;
  double betas[2];
  double eps;
  double weight_decay;
  double max_grad_norm; /* <= 0: no clipping */
  double ema_decay;     /* < 0: no EMA */
  int32_t decoupled;    /* 0: g += weight_decay p (Adam);  1: p *= 1 - lr weight_decay (AdamW) */
  int32_t reserved;     /* 0 */
} rgfm_adam_desc;

int rgfm_adam_workspace_bytes(size_t* bytes);
int rgfm_adam_grad_norm(const rgfm_adam_entry* table_dev, int n_entries, uint64_t span_begin, uint64_t span_end, void* ws,
                        size_t ws_bytes, rgfm_stream_t stream);
int rgfm_adam_step(const rgfm_adam_desc* desc, const rgfm_adam_entry* table_dev, int n_entries, uint64_t span_begin,
                   uint64_t span_end, float* exp_avg, float* exp_avg_sq, float* ema, float* grad_norm_out, void* ws,
                   size_t ws_bytes, rgfm_stream_t stream);

/* One guidance evaluation on its own (parity hook for sample_mnist_svhn.py:124-171):
 * vx/vy are overwritten with (1-gamma)*v + gamma*g at time t; weights_out[B,N]
 * (optional, may be null) receives the normalised importance weights. */
int rgfm_guidance_workspace_bytes(int batch, int n_mc, size_t* bytes);
int rgfm_guidance_apply(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                        const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x,
                        int dim_y, double t, double gamma, float* weights_out, void* ws,
                        size_t ws_bytes, rgfm_stream_t stream);

/* One evaluation of the one-sided block of rgfm_sample_cond on its own (parity hook): v[B,dim] is overwritten with
 * (1-gamma)*v + gamma*g at time t for the state s[B,dim], the MC set mc_set[N,dim] and ratios[batch][n_mc];
 * weights_out[B,N] (optional, may be null); ws as rgfm_guidance_workspace_bytes(batch, n_mc). */
int rgfm_guidance_apply_cond(const float* s, float* v, const float* mc_set, const float* ratios, int batch,
                             int n_mc, int dim, double t, double gamma, float* weights_out, void* ws,
                             size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Guidance diagnostics (opt-in).  Added functions only: the ABI version is unchanged.
 *
 * One record of RGFM_DIAG_FLOATS fp32 values per (stage, sample), written on the device, stage-major
 * [n_stages][batch][RGFM_DIAG_FLOATS]; n_stages = step_end - step_begin for RGFM_SOLVER_EULER and twice that for
 * RGFM_SOLVER_MIDPOINT (stage 1 then stage 2 of each step).  What the reference prints once per run
 * (src/utils/flow_utils.py:349-363), as per-sample curves:
 *   RGFM_DIAG_ESS      MC guidance: (sum_i w_i)^2 / sum_i w_i^2 of the row's normalised importance weights, 1 .. n_mc;
 *                      0 marks "this stage was not MC-guided" (t <= 1e-3, n_mc = 0, or a gradient-guided loop)
 *   RGFM_DIAG_W_MAX / RGFM_DIAG_W_MIN    max_i w_i, min_i w_i of the row
 *   RGFM_DIAG_Z_BAR    the row's Z_bar = mean_i r_i p_i + 1e-10 (reference :315)
 *   RGFM_DIAG_V_NORM_X / _Y    L2 norm of the net's velocity at the stage, before any blend
 *   RGFM_DIAG_G_NORM_X / _Y    MC guidance: L2 norm of the pure guided velocity g = sum_i w_i (m_i - x) / (1 - t + eps)
 *                      (reference :340-341); gradient guidance: L2 norm of d log r / dx, d log r / dy, before gamma
 * One-sided loops and blocks leave the _Y entries 0.  A stage that runs unguided is an all-zero record.
 * Gradient-guided loops fill the four norms and leave the first four entries 0.
 *
 * Block level: the inputs of the guidance block's parity hooks without gamma; v is read, nothing but diag_out
 * [batch][RGFM_DIAG_FLOATS] and the workspace is written.
 * Loop level: each *_diag loop is its *_ode namesake (the FlowMatchingModel pair: its Euler entry point) with
 * `float* diag_out, size_t diag_records` in front of `ws`; the state it computes has the bits of that entry point.
 * diag_out null with diag_records 0: exactly the existing entry point.  Otherwise both must be given and diag_records
 * (a capacity, in records) must be at least n_stages * batch: RGFM_EINVAL before anything is enqueued.  No host
 * synchronisation is added; the records are complete when the stream reaches the end of the call.  With diagnostics on
 * the paired MC loop runs kernel by kernel (no hipGraph replay: same kernels, same arguments, same bits) and each
 * guided stage adds the weight statistics (one launch), a row norm per velocity and modality (four launches, two in a
 * one-sided loop) and one more pass of the guided-velocity GEMM into a scratch velocity; the workspace grows by that
 * scratch (the *_diag_workspace_bytes queries).  The gradient-guided loops add the row norms only and need no scratch.
 * ---------------------------------------------------------------------- */
#define RGFM_DIAG_FLOATS 8
#define RGFM_DIAG_ESS 0
#define RGFM_DIAG_W_MAX 1
#define RGFM_DIAG_W_MIN 2
#define RGFM_DIAG_Z_BAR 3
#define RGFM_DIAG_V_NORM_X 4
#define RGFM_DIAG_V_NORM_Y 5
#define RGFM_DIAG_G_NORM_X 6
#define RGFM_DIAG_G_NORM_Y 7
int rgfm_guidance_diag_workspace_bytes(int batch, int n_mc, int dim_x, int dim_y, size_t* bytes);
int rgfm_guidance_diag(const float* x, const float* y, const float* vx, const float* vy, const float* mc_x1,
                       const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x, int dim_y, double t,
                       float* diag_out, void* ws, size_t ws_bytes, rgfm_stream_t stream);
/* (the one-sided block: dim_y = 0 in the workspace query) */
int rgfm_guidance_diag_cond(const float* s, const float* v, const float* mc_set, const float* ratios, int batch, int n_mc,
                            int dim, double t, float* diag_out, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_diag_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver,
                                          size_t* bytes);
int rgfm_sample_pair_diag(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                          const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                          int step_begin, int step_end, int solver, float* diag_out, size_t diag_records, void* ws,
                          size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_diag_workspace_bytes(const rgfm_unet* h, int batch, int n_mc, int solver, size_t* bytes);
int rgfm_sample_cond_diag(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                          int num_steps, double gamma, int step_begin, int step_end, int solver, float* diag_out,
                          size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_grad_diag_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, const rgfm_ratio* hr,
                                               int batch, int solver, size_t* bytes);
int rgfm_sample_pair_grad_diag(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout,
                               int batch, int num_steps, double gamma, int step_begin, int step_end, int solver,
                               float* diag_out, size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_grad_diag_workspace_bytes(const rgfm_unet* h_unet, const rgfm_ratio* h_ratio, int given,
                                               int batch, int solver, size_t* bytes);
int rgfm_sample_cond_grad_diag(rgfm_unet* h_unet, rgfm_ratio* h_ratio, float* s_inout, const float* ctx, int given,
                               int batch, int num_steps, double gamma, int step_begin, int step_end, int solver,
                               float* diag_out, size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_fmnet_sample_pair_diag_workspace_bytes(const rgfm_fmnet* hx, const rgfm_fmnet* hy, int batch, int n_mc,
                                                size_t* bytes);
int rgfm_fmnet_sample_pair_diag(rgfm_fmnet* hx, rgfm_fmnet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                                const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps,
                                double gamma, int step_begin, int step_end, float* diag_out, size_t diag_records,
                                void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Cross pairing of the MC set (U-Net pairs).  Added functions only: the ABI version is unchanged.
 *
 * The paired MC guidance uses the n_mc pairs (mc_x1[i], mc_y1[i]).  Every (mc_x1[i], mc_y1[j]) is as valid a draw
 * from the product of the marginals, so the same MC set yields n_mc^2 importance pairs.  Cross pairing is the
 * reference block (src/utils/flow_utils.py:273-369, src/sample_mnist_svhn.py:124-171) on that list of n_mc^2 pairs
 * with ratios ratio_matrix[i][j] = r(mc_x1[i], mc_y1[j]) ([n_mc][n_mc] row-major, x index first:
 * rgfm_ratio_eval_cross).  The Gaussian factor of pair (i, j) is a_i b_j, so only the marginals of the weights are
 * ever formed:
 *   a_i = exp(lx_i - max lx), b_j = exp(ly_j - max ly),  u = R b,  s = R^T a,
 *   p_bar = (sum a)(sum b) / n_mc^2 + 1e-10,  Z_bar = a^T R b / n_mc^2 + 1e-10,
 *   wx_i = sum_j w_ij ~ a_i u_i,  wy_j = sum_i w_ij ~ b_j s_j,  each summing to 1,
 *   g_x = sum_i wx_i (mc_x1[i] - x) / (1 - t + 1e-3),  g_y = sum_j wy_j (mc_y1[j] - y) / (1 - t + 1e-3).
 * 1 <= n_mc <= 1024; dim_x, dim_y multiples of 4.  wx_out / wy_out [batch][n_mc]: optional (may be null).
 *
 * Diagnostics records of a cross call: RGFM_DIAG_ESS is the JOINT effective sample size
 * (sum_ij w_ij)^2 / sum_ij w_ij^2, 1 .. n_mc^2; RGFM_DIAG_W_MAX / _W_MIN the max and min over the 2 n_mc marginal
 * weights wx, wy; RGFM_DIAG_Z_BAR the Z_bar above; the four norms as before, g from the marginal weights.
 *
 * rgfm_sample_pair_cross is rgfm_sample_pair_diag with the ratio matrix in the ratio vector's place: one entry point
 * for both solvers; diag_out null with diag_records 0 = no diagnostics; n_mc = 0 = unguided.  A cross call runs
 * kernel by kernel (no hipGraph replay).  All argument errors (null pointers, n_mc above 1024, flattened sizes that
 * are no multiples of 4, a short workspace, short diag_records) are returned before anything is enqueued.
 * ---------------------------------------------------------------------- */
int rgfm_guidance_cross_workspace_bytes(int batch, int n_mc, int dim_x, int dim_y, size_t* bytes);
int rgfm_guidance_apply_cross(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                              const float* mc_y1, const float* ratio_matrix, int batch, int n_mc, int dim_x, int dim_y,
                              double t, double gamma, float* wx_out, float* wy_out, void* ws, size_t ws_bytes,
                              rgfm_stream_t stream);
/* (v is read; nothing but diag_out [batch][RGFM_DIAG_FLOATS] and the workspace is written) */
int rgfm_guidance_diag_cross(const float* x, const float* y, const float* vx, const float* vy, const float* mc_x1,
                             const float* mc_y1, const float* ratio_matrix, int batch, int n_mc, int dim_x, int dim_y,
                             double t, float* diag_out, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_cross_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch, int n_mc, int solver,
                                           size_t* bytes);
int rgfm_sample_pair_cross(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                           const float* mc_y1, const float* ratio_matrix, int n_mc, int batch, int num_steps,
                           double gamma, int step_begin, int step_end, int solver, float* diag_out,
                           size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Guidance strength per sample and per stage (U-Net nets).  Added functions only: the ABI version is unchanged.
 *
 * For row b and stage k of a call the effective strength is gamma[b,k] = (double)gamma_b * s_k, formed in double.
 *   k        counts the call's own stages in the order of the diagnostics records: step_end - step_begin stages for
 *            RGFM_SOLVER_EULER, twice that for RGFM_SOLVER_MIDPOINT (stage 1 then stage 2 of each step).
 *   gamma_b  gamma_rows[batch], a DEVICE vector of fp32 owned by the caller; null: the call's `double gamma` for every row.
 *   s_k      stage_scale[n_stage_scale], a HOST array of doubles, read before the call returns and not retained;
 *            null (with n_stage_scale 0): 1 for every stage.
 * The MC blends (paired, cross, one-sided) use g1 = (float)(1.0 - gamma[b,k]) and g2 = (float)gamma[b,k] in
 * g1 v + g2 g; the gradient loops use (float)gamma[b,k] in x = base + fma(gamma, grad log r, v) dt -- the rules of the
 * scalar entry points.  So with s_k = 1 row b has the bits of the scalar call with gamma = (double)gamma_rows[b].
 * Values are not clamped: negative strengths and strengths above 1 are allowed.
 * A stage is guided iff it is guided in the scalar call (the MC loops: n_mc > 0 and the stage's own t > 1e-3; the
 * gradient loops: always) AND s_k != 0.  A stage with s_k == 0 runs as the loop's unguided stage: the nets with the
 * fused Euler epilogue and no guidance, ratio-estimator or update launch.  Its state has the bits of the unguided loops
 * over that range (rgfm_sample_pair_ode with n_mc = 0, rgfm_sample_single_ode) and its diagnostics record is all zero.
 * The diagnostics' norms and weights do not depend on gamma.
 * A call with gamma_rows or stage_scale runs kernel by kernel (no hipGraph replay).  With both null each *_gs loop is
 * exactly its namesake: same launches, arguments and replay.
 *
 * Loops: each *_gs entry point is its *_diag namesake (rgfm_sample_pair_cross_gs: rgfm_sample_pair_cross) with
 * `const float* gamma_rows, const double* stage_scale, int n_stage_scale` behind `gamma`; workspace: the namesake's
 * query (rgfm_sample_pair_diag_workspace_bytes with records, rgfm_sample_pair_ode_workspace_bytes without, ...).
 * Blocks: each *_rows entry point is the existing block with `const float* gamma_rows` (not null) in place of
 * `double gamma`; workspace: the existing block queries.
 * Errors are returned before anything is enqueued and touch no state: the namesake's own, and RGFM_EINVAL for
 * n_stage_scale != the call's stage count, a stage_scale entry that is not finite, or stage_scale null with
 * n_stage_scale != 0.
 * ---------------------------------------------------------------------- */
int rgfm_sample_pair_gs(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                        const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                        const float* gamma_rows, const double* stage_scale, int n_stage_scale, int step_begin,
                        int step_end, int solver, float* diag_out, size_t diag_records, void* ws, size_t ws_bytes,
                        rgfm_stream_t stream);
int rgfm_sample_pair_cross_gs(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                              const float* mc_y1, const float* ratio_matrix, int n_mc, int batch, int num_steps,
                              double gamma, const float* gamma_rows, const double* stage_scale, int n_stage_scale,
                              int step_begin, int step_end, int solver, float* diag_out, size_t diag_records, void* ws,
                              size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_gs(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                        int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                        int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                        size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_grad_gs(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout, int batch,
                             int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                             int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                             size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_grad_gs(rgfm_unet* h_unet, rgfm_ratio* h_ratio, float* s_inout, const float* ctx, int given,
                             int batch, int num_steps, double gamma, const float* gamma_rows,
                             const double* stage_scale, int n_stage_scale, int step_begin, int step_end, int solver,
                             float* diag_out, size_t diag_records, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_guidance_apply_rows(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                             const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x, int dim_y,
                             double t, const float* gamma_rows, float* weights_out, void* ws, size_t ws_bytes,
                             rgfm_stream_t stream);
int rgfm_guidance_apply_cond_rows(const float* s, float* v, const float* mc_set, const float* ratios, int batch,
                                  int n_mc, int dim, double t, const float* gamma_rows, float* weights_out, void* ws,
                                  size_t ws_bytes, rgfm_stream_t stream);
int rgfm_guidance_apply_cross_rows(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                                   const float* mc_y1, const float* ratio_matrix, int batch, int n_mc, int dim_x,
                                   int dim_y, double t, const float* gamma_rows, float* wx_out, float* wy_out, void* ws,
                                   size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Stochastic sampling: Euler-Maruyama steps in every U-Net sampler loop (added functions only: the ABI version is
 * unchanged).  For the Gaussian path x_t = (1 - t) x_0 + t x_1, x_0 ~ N(0, I), the score follows from the velocity,
 * grad log p_t(x) = (t v - x) / (1 - t), and with g(t)^2 = 2 eta (1 - t) the SDE of the ODE's marginals is
 *     dx = [F + eta (t F - x)] dt + sqrt(2 eta (1 - t)) dW          (no singularity at either end; eta = 0: the ODE)
 * with F the loop's whole velocity at the stage: the net's (unguided), the MC blend (MC loops), v + gamma grad log r
 * (gradient loops).
 *
 * 1. The step.  Step i of num_steps: dt = 1 / num_steps and t = i dt in double, k = i the GLOBAL step index (not the
 *    index within the call):
 *        base = (1 - eta dt) x + sigma_k xi_k          sigma_k = sqrt(2 eta (1 - t) dt)
 *        x    = base + ((1 + eta t) dt) F(x, t)
 *    The second line is the loop's fused update as it is: it reads the old state, its base is the new buffer, and
 *    dts = (float)((1 + eta t) dt), formed in double.  The first line is one kernel over the [batch][D] state of each
 *    modality, which generates xi itself, with a = (float)(1 - eta dt) and sigma = (float)sigma_k:
 *    base[e] = fma(a, x[e], sigma xi[e]).  Whether a stage is guided, and t, are unchanged.
 *
 * 2. The noise, bit-defined up to logf, sqrtf and sincospif.  xi_k of stream m (0: the loop's first or only state,
 *    1: the second) is a function of (seed, m, k, e) alone, e the flat element index in [batch][D].  Elements come in
 *    pairs p = e / 2; with fin the splitmix64 finaliser documented for rgfm_unet_dropout_mask, arithmetic mod 2^64:
 *        key = fin(seed + 0x9E3779B97F4A7C15 * ((((uint64)m << 32) | k) + 1))
 *        z   = fin(key  + 0x9E3779B97F4A7C15 * (p + 1))
 *        u1  = ((z >> 40) + 1) * 2^-24            in (0, 1]
 *        u2  = ((z >> 8) & 0xFFFFFF) * 2^-24      in [0, 1)
 *        r   = sqrt(-2 ln u1),   xi[2p] = r cos(2 pi u2),   xi[2p + 1] = r sin(2 pi u2)
 *    in fp32 (u1, u2 and the argument 2 u2 of sincospif are exact).  So |xi| <= sqrt(48 ln 2) = 5.77; an odd
 *    batch * D ends on a cosine; a row's noise does not depend on the batch size; and split calls reproduce the bits of
 *    one call: steps [0, a) then [a, N) equal [0, N).  rgfm_sde_noise (test hook) writes xi[0..n) of (seed,
 *    stream_id in {0, 1}, k >= 0) to out, stream-ordered.
 *
 * 3. Entry points.  rgfm_sample_single_sde is rgfm_sample_single_ode, and rgfm_sample_{pair, pair_cross, cond,
 *    pair_grad, cond_grad}_sde is its *_gs namesake, with `const rgfm_sde* sde` directly in front of ws.
 *    sde == NULL or eta == 0: the call IS its namesake -- same launches, same arguments, same graph replay, same
 *    bits, same workspace.  eta > 0: the workspace is the namesake's query plus rgfm_sde_scratch_bytes (batch, D of the
 *    first state, D of the second or 0): one [batch][D] buffer per modality, carved behind the loop's own buffers;
 *    the call runs kernel by kernel (no hipGraph replay).  rgfm_sample_two (the MC pre-phase) has no stochastic twin.
 *    Errors are returned before anything is enqueued and touch no state: the namesake's own; RGFM_EINVAL for eta < 0 or
 *    not finite, and for solver == RGFM_SOLVER_MIDPOINT with eta > 0 (a stochastic midpoint rule is out of scope);
 *    RGFM_ENOMEM for a workspace short of the sum above.
 * ---------------------------------------------------------------------- */
typedef struct rgfm_sde { double eta; uint64_t seed; } rgfm_sde;
int rgfm_sde_scratch_bytes(int batch, int dim_x, int dim_y, size_t* bytes);
int rgfm_sde_noise(uint64_t seed, int stream_id, int k, size_t n, float* out, rgfm_stream_t stream);
int rgfm_sample_single_sde(rgfm_unet* h, float* x_inout, int batch, int num_steps, int step_begin, int step_end,
                           int solver, const rgfm_sde* sde, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_sde(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                         const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                         const float* gamma_rows, const double* stage_scale, int n_stage_scale, int step_begin,
                         int step_end, int solver, float* diag_out, size_t diag_records, const rgfm_sde* sde, void* ws,
                         size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_cross_sde(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                               const float* mc_y1, const float* ratio_matrix, int n_mc, int batch, int num_steps,
                               double gamma, const float* gamma_rows, const double* stage_scale, int n_stage_scale,
                               int step_begin, int step_end, int solver, float* diag_out, size_t diag_records,
                               const rgfm_sde* sde, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_sde(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                         int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                         int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                         size_t diag_records, const rgfm_sde* sde, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_pair_grad_sde(rgfm_unet* hx, rgfm_unet* hy, rgfm_ratio* hr, float* x_inout, float* y_inout, int batch,
                              int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                              int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                              size_t diag_records, const rgfm_sde* sde, void* ws, size_t ws_bytes,
                              rgfm_stream_t stream);
int rgfm_sample_cond_grad_sde(rgfm_unet* h_unet, rgfm_ratio* h_ratio, float* s_inout, const float* ctx, int given,
                              int batch, int num_steps, double gamma, const float* gamma_rows,
                              const double* stage_scale, int n_stage_scale, int step_begin, int step_end, int solver,
                              float* diag_out, size_t diag_records, const rgfm_sde* sde, void* ws, size_t ws_bytes,
                              rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Effective-sample-size floor: adaptive tempering of the MC importance weights (paired and one-sided MC loops of the
 * U-Nets).  Added functions only: the ABI version is unchanged.
 *
 * Row b of a guided stage weighs the MC set by w_i ~ r_i N(x_t; t m_i, sigma_t^2), and as t -> 1 the weights collapse
 * onto the nearest MC sample.  With a floor ess_min (a double, 1 <= ess_min <= n_mc) the row's weights are flattened by
 * an exponent tau <= 1 of its own, just enough that their effective sample size reaches the floor; rows at or above it
 * are not touched.
 *
 * 1. The rule.  l_i: the row's log-density term (the two modalities' -0.5 |.|^2 / sigma_t^2, each rounded to fp32, then
 *    added); r_i: its ratio (the shared vector, or the row's own in the one-sided loop); w_i: the weights of the call
 *    without a floor; ESS_1 = (sum w)^2 / sum w^2.
 *      P = {i : r_i > 0}, n_pos = |P|.  Samples outside P have weight exactly 0 for every tau: they are masked,
 *                 tau * (-inf) is never formed.
 *      E* = min(ess_min, n_pos).  n_pos = 0: the all-zero row of the call without a floor (tau = 1).
 *      ESS_1 >= E*, or E* <= 1 (an effective sample size is at least 1, whatever the rounding of ESS_1 says):
 *                 tau = 1, and the row's weights, weight sum and weights_out are the BITS of the call without a
 *                 floor -- the existing result is kept, the tempered formula is not evaluated at tau = 1.
 *      otherwise  L_i = l_i + log r_i,  d_i = L_i - max_P L,  ESS(tau) = (sum_P e^{tau d_i})^2 / sum_P e^{2 tau d_i},
 *                 non-increasing in tau with ESS(0) = n_pos >= E*.  Bisection from lo = 0, hi = 1, exactly 40 times
 *                 mid = 0.5 (lo + hi); lo = mid if ESS(mid) >= E*, else hi = mid.  Then tau = lo and
 *                 w_i = e^{tau d_i} / sum_P e^{tau d_j}.  No early exit and no epsilon: the largest term is 1.
 *    All in fp32, e^{2 tau d} as the square of e^{tau d}; every sum runs lane l over samples l, l + 64, ... in index
 *    order followed by the xor butterfly over the 64 lanes, so a row's result depends on its own data and n_mc only,
 *    not on the batch.  The WHOLE weight r p is tempered, not the Gaussian factor alone: with r held fixed,
 *    (sum r_i p_i^tau)^2 / sum r_i^2 p_i^{2 tau} is not monotone in tau and the target may be unreachable (at tau = 0 it
 *    is the effective sample size of r itself).  Tempering biases the estimator: it trades the collapsed weights'
 *    variance for a pull toward the ratio-free, flatter posterior mean.
 *
 * 2. Loops.  rgfm_sample_pair_ess / rgfm_sample_cond_ess: the *_sde namesake with `const rgfm_ess* ess` directly in
 *    front of ws.  ess == NULL or ess_min <= 0: the call IS its namesake -- launches, graph replay, bits, workspace.
 *    Otherwise the workspace is still the namesake's query (the kernel needs LDS only, no memory of the caller's), every
 *    guided stage enqueues the tempering weights kernel in the place of the plain one and nothing else changes, and the
 *    call runs kernel by kernel (no hipGraph replay).  tau_out: a DEVICE array [stages][batch] of fp32, or null; it
 *    receives tau per row in the diagnostics records' stage order (tau_records >= stages x batch floats), 0 for an
 *    unguided stage.  Composes with both solvers, gamma_rows / stage_scale, sde and diagnostics: RGFM_DIAG_ESS, _W_MAX
 *    and _W_MIN are then those of the tempered weights, RGFM_DIAG_Z_BAR stays the untempered value.
 *    Blocks: rgfm_guidance_apply_ess / rgfm_guidance_apply_cond_ess are the *_rows blocks with
 *    `double ess_min, float* tau_out` (tau_out [batch] or null) behind weights_out; ess_min <= 0: the *_rows block.
 *    n_mc: 1 .. 4096 as everywhere (two [4][n_mc] fp32 arrays in LDS: 128 KB of the CU's 160 at n_mc = 4096).
 *    Errors are returned before anything is enqueued: the namesake's own, and RGFM_EINVAL for ess_min not finite, in
 *    (0, 1) or above n_mc, and for tau_out with tau_records short of the call's stages x batch.  There is no cross
 *    twin: a per-row exponent makes the ratio matrix row-dependent, and the two [B,N] x [N,N] products are gone.
 * ---------------------------------------------------------------------- */
typedef struct rgfm_ess { double ess_min; float* tau_out; size_t tau_records; } rgfm_ess;
int rgfm_sample_pair_ess(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const float* mc_x1,
                         const float* mc_y1, const float* mc_ratios, int n_mc, int batch, int num_steps, double gamma,
                         const float* gamma_rows, const double* stage_scale, int n_stage_scale, int step_begin,
                         int step_end, int solver, float* diag_out, size_t diag_records, const rgfm_sde* sde,
                         const rgfm_ess* ess, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_cond_ess(rgfm_unet* h, float* s_inout, const float* mc_set, const float* ratios, int n_mc, int batch,
                         int num_steps, double gamma, const float* gamma_rows, const double* stage_scale,
                         int n_stage_scale, int step_begin, int step_end, int solver, float* diag_out,
                         size_t diag_records, const rgfm_sde* sde, const rgfm_ess* ess, void* ws, size_t ws_bytes,
                         rgfm_stream_t stream);
int rgfm_guidance_apply_ess(const float* x, const float* y, float* vx, float* vy, const float* mc_x1,
                            const float* mc_y1, const float* mc_ratios, int batch, int n_mc, int dim_x, int dim_y,
                            double t, const float* gamma_rows, float* weights_out, double ess_min, float* tau_out,
                            void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_guidance_apply_cond_ess(const float* s, float* v, const float* mc_set, const float* ratios, int batch,
                                 int n_mc, int dim, double t, const float* gamma_rows, float* weights_out,
                                 double ess_min, float* tau_out, void* ws, size_t ws_bytes, rgfm_stream_t stream);

/* ------------------------------------------------------------------------
 * Class conditioning and classifier-free guidance (an extension: the reference's nets are unconditional).
 * Added functions only: rgfm_unet_desc and RGFM_ABI_VERSION are unchanged.
 *
 * 1. The model.  A class-conditional U-Net with K = num_classes classes owns one more tensor, label_emb.weight
 *    [K + 1][4 model_channels], the LAST entry of its blob: the unlabelled blob, then that table.  Row K is the null
 *    label, the net's unconditional branch.  The function is the ADM form
 *        emb = time_embed(timestep_embedding(t)) + label_emb[y],   then every ResBlock: Linear(SiLU(emb)) as before.
 *    rgfm_unet_labeled_param_floats / rgfm_unet_labeled_create: the counterparts of rgfm_unet_param_floats / _create,
 *    1 <= num_classes < 4096.  Every function that takes an rgfm_unet* takes such a handle: rgfm_unet_update_params
 *    the longer blob, rgfm_unet_backward writes dparams_out with d label_emb.weight [K + 1][temb] at its end, and every
 *    entry point WITHOUT a labels argument (forward, the sampler loops, the likelihood path, training) evaluates the
 *    net with the null label in every row.
 * 2. Labels are device int32, one per row, values 0 .. K.  A value outside that range is READ AS K on the device (an
 *    index taken from user data never addresses outside the table); callers that want an error check on the host.
 *    Labels on a handle without classes: RGFM_EINVAL.  A null labels pointer: the namesake without labels.
 * 3. rgfm_unet_forward_labels / rgfm_unet_forward_train_labels: rgfm_unet_forward / rgfm_unet_forward_train with
 *    labels_dev behind t_count; same workspaces.  The training forward saves the labels in ws;
 *    dE[c] = sum of d emb[b] over the rows b with y_b == c, added in ascending b by one workgroup per class (no
 *    atomics: two backward calls give the same bits), exact zeros for a class without a row.
 * 4. rgfm_sample_single_cfg is rgfm_sample_single_sde, rgfm_sample_two_cfg is rgfm_sample_two, with labels and a
 *    guidance scale w per net: every stage advances by  F = v_u + w (v_c - v_u),  v_c the net at the rows' labels, v_u
 *    at the null label.  w == 1 evaluates v_c alone and w == 0 v_u alone (one evaluation per stage, the out-conv's fused
 *    update; w == 0 has the bits of the call without labels); any other w evaluates both and one elementwise kernel
 *    writes state = base + F dts with the stage's own (base, dts), so midpoint stages and the stochastic step compose.
 *    A call builds its time table once, [stages][K + 1][temb_total], and hands each conditional evaluation the rows
 *    gathered by label.  The table holds 4096 rows: stages x (K + 1) beyond that is RGFM_EINVAL -- split the call with
 *    step_begin / step_end (split calls reproduce one call bit for bit).  Workspace: the *_cfg_workspace_bytes
 *    queries (one size for every scale; rgfm_sample_single_cfg with eta > 0 adds rgfm_sde_scratch_bytes).
 *    Errors are returned before anything is enqueued: the namesake's own, RGFM_EINVAL for labels on a handle without
 *    classes or a cfg_scale that is not finite, RGFM_ENOMEM for a short workspace.
 * ---------------------------------------------------------------------- */
int rgfm_unet_labeled_param_floats(const rgfm_unet_desc* desc, int num_classes, size_t* n_floats);
int rgfm_unet_labeled_create(const rgfm_unet_desc* desc, int num_classes, const float* params_dev, size_t n_floats,
                             rgfm_stream_t stream, rgfm_unet** out);
int rgfm_unet_forward_labels(rgfm_unet* h, const float* x, const float* t_dev, int t_count, const int32_t* labels_dev,
                             float* v_out, int batch, void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_unet_forward_train_labels(rgfm_unet* h, const float* x, const float* t_dev, int t_count,
                                   const int32_t* labels_dev, float* v_out, int batch, float p_drop, uint64_t seed,
                                   void* ws, size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_single_cfg_workspace_bytes(const rgfm_unet* h, int batch, int solver, size_t* bytes);
int rgfm_sample_single_cfg(rgfm_unet* h, float* x_inout, const int32_t* labels_dev, double cfg_scale, int batch,
                           int num_steps, int step_begin, int step_end, int solver, const rgfm_sde* sde, void* ws,
                           size_t ws_bytes, rgfm_stream_t stream);
int rgfm_sample_two_cfg_workspace_bytes(const rgfm_unet* hx, const rgfm_unet* hy, int batch_x, int batch_y, int solver,
                                        size_t* bytes);
int rgfm_sample_two_cfg(rgfm_unet* hx, rgfm_unet* hy, float* x_inout, float* y_inout, const int32_t* labels_x,
                        const int32_t* labels_y, double cfg_scale_x, double cfg_scale_y, int batch_x, int batch_y,
                        int num_steps, int step_begin, int step_end, int solver, void* ws, size_t ws_bytes,
                        rgfm_stream_t stream);
/* The blend kernel of 4. alone over n floats, 200 launches back to back between two device events on the null stream
 * (synchronises): GB/s of the 16 bytes per element it moves, and the time of one launch in microseconds. */
int rgfm_ubench_cfg_blend(size_t n, double* gbps, double* us_per_launch);

/* ------------------------------------------------------------------------
 * Bench support: per-kernel-class device time measured with hipEvents on the
 * launch stream (bench.py's roofline line).  Timing is off by default.
 * ---------------------------------------------------------------------- */
#define RGFM_KCLASS_CONV_MFMA 0  /* conv3x3/1x1 implicit GEMM on the matrix cores: work = FLOPs (2*MAC)      */
#define RGFM_KCLASS_OTHER 1      /* everything not listed here (work = 0)                                     */
/* HBM-bound kernels of the U-Net pair step: work = ALGORITHMIC HBM bytes of the launch */
#define RGFM_KCLASS_CONV_IN1 2   /* input_conv, 1-channel image (conv_in_kernel<1>)                          */
#define RGFM_KCLASS_CONV_IN3 3   /* input_conv, 3-channel image (conv_in_kernel<3>)                          */
#define RGFM_KCLASS_CONV_OUT1 4  /* out_norm + SiLU + out_conv (+ fused Euler), 1 channel                    */
#define RGFM_KCLASS_CONV_OUT3 5  /* ... 3 channels                                                           */
#define RGFM_KCLASS_GUID_LOGP 6  /* guidance: squared distances to the MC set (guid_logp_kernel)             */
#define RGFM_KCLASS_GUID_APPLY 7 /* guidance: weights, weighted velocity, blend, Euler (guid_apply_kernel x2) */
#define RGFM_KCLASS_COUNT 8
int rgfm_profile_enable(int enable);
int rgfm_profile_reset(void);
/* Waits for the recorded events, then returns for the class, since the last reset:
 *   busy_ms  = length of the UNION of the launches' [start, stop] intervals (the two velocity nets
 *              of a step run on two streams, so launches of one class may overlap in time);
 *   sum_ms   = plain sum of the launch durations (== busy_ms when nothing overlaps);
 *   launches, flops = launch count and the class's algorithmic work (FLOPs or bytes, see RGFM_KCLASS_*). */
int rgfm_profile_read(int kclass, double* busy_ms, double* sum_ms, int64_t* launches, double* flops);
/* Start of the class's first timed launch and end of its last one, in ms since the first timed launch after the latest
 * reset (both 0 when the class has none).  The in- and out-conv classes are per modality (1 / 3 channels), so their
 * spans tell when each net of a two-net call started and ended.  Added function only: the ABI version is unchanged. */
int rgfm_profile_span(int kclass, double* first_start_ms, double* last_end_ms);

/* Pre-creates the hipEvents of `launches` timed launches, so that none is created inside a timed region. */
int rgfm_profile_reserve(int64_t launches);

/* Measured ceilings of the current device, for the roofline line (each call takes ~0.2-0.5 s and synchronises):
 *   rgfm_ubench_mfma_f16: sustained dense f16 MFMA rate (v_mfma_f32_32x32x16_f16, operands in registers, random
 *     data, two waves per SIMD on every CU, >= 0.2 s) in TFLOP/s -- what the chip holds under DVFS, as opposed to
 *     the 2500 TFLOP/s nominal peak;
 *   rgfm_ubench_hbm_copy: float4 copy of `bytes` (>= 256 MiB recommended) in GB/s of read + written bytes. */
int rgfm_ubench_mfma_f16(double* tflops);
int rgfm_ubench_hbm_copy(size_t bytes, double* gbps);
/* The stochastic step's pre-update kernel ("Stochastic sampling", 1.) alone over n floats, 200 launches back to back
 * between two device events on the null stream (synchronises): GB/s of the 8 bytes per element it moves, and the time
 * of one launch in microseconds.  Added function only. */
int rgfm_ubench_sde_pre(size_t n, double* gbps, double* us_per_launch);

/* Conv arithmetic of ONE handle (see "arithmetic" above); RGFM_CONV_DEFAULT follows the RGFM_CONV environment
 * variable (hx2 | bx3 | f32, read once per API call; unset = hx2).  A handle setting, not process state: two host
 * threads driving two handles never change each other's arithmetic. */
#define RGFM_CONV_DEFAULT (-1)
#define RGFM_CONV_HX2 0
#define RGFM_CONV_BX3 1
#define RGFM_CONV_F32 2
int rgfm_unet_set_conv_mode(rgfm_unet* h, int mode);
int rgfm_fmnet_set_conv_mode(rgfm_fmnet* h, int mode);

/* Range flag of the default fp16 conv path, one word per handle: waits for `stream`, then *flagged = the bits raised
 * by the handle's launches since the last reset -- 1: a staged activation reached |a| >= 2048 (fp16 overflow);
 * 2: an output that a later conv stages without a GroupNorm in front (the residual stream: reference
 * src/models/unet_flexible.py:85,96,107-108 consume it in fp32 at any magnitude) had a 64-pixel wave block whose
 * largest |value| was below 2^-8, where the two fp16 planes lose bits.  Non-zero: the results of those calls are not
 * fp32-class; repeat them with rgfm_*_set_conv_mode(h, RGFM_CONV_BX3) (bit 0) or RGFM_CONV_F32 (bit 1: the exact fp32
 * convs are the reference's arithmetic at any magnitude).  reset != 0 clears the word. */
int rgfm_unet_range_flag(rgfm_unet* h, int* flagged, int reset, rgfm_stream_t stream);
int rgfm_fmnet_range_flag(rgfm_fmnet* h, int* flagged, int reset, rgfm_stream_t stream);

int rgfm_abi_version(void);
const char* rgfm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RGFM_H_ */
