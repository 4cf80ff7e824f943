"""ctypes binding of csrc/librgfm_hip.so (C ABI: include/rgfm.h).

Loading is lazy and LOUD: there is no fallback implementation, so a missing
or stale library raises with the build command instead of degrading.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RGFM_LIB: another build of the same ABI (A/B measurements of two library versions inside one run)
LIB_PATH = os.environ.get("RGFM_LIB") or os.path.join(_HERE, "csrc", "librgfm_hip.so")
ABI_VERSION = 3

_lib = None

c_void_p, c_int, c_size_t, c_double = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
c_int32, c_int64, c_uint64, c_float = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float
P = ctypes.POINTER


class UNetDesc(ctypes.Structure):
    _fields_ = [("in_channels", c_int32), ("img_size", c_int32), ("model_channels", c_int32),
                ("num_levels", c_int32), ("channel_mult", c_int32 * 4), ("num_res_blocks", c_int32)]


class RatioDesc(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("feature_dim", c_int32), ("hidden_dim", c_int32),
                ("loss_type", c_int32)]


class RatioFlexDesc(ctypes.Structure):
    _fields_ = [("feature_dim", c_int32), ("hidden_dim", c_int32), ("loss_type", c_int32),
                ("x_channels", c_int32), ("y_channels", c_int32), ("x_size", c_int32), ("y_size", c_int32)]


class FmNetDesc(ctypes.Structure):
    _fields_ = [("img_channels", c_int32), ("feature_dim", c_int32), ("time_emb_dim", c_int32)]


class ClfDesc(ctypes.Structure):
    _fields_ = [("kind", c_int32)]


class AdamEntry(ctypes.Structure):  # rgfm_adam_entry: one tensor of the optimizer step's device table (48 bytes)
    _fields_ = [("param", c_uint64), ("grad", c_uint64), ("offset", c_uint64), ("numel", c_uint64),
                ("bc1", c_double), ("bc2", c_double)]


class AdamDesc(ctypes.Structure):
    _fields_ = [("lr", c_double), ("betas", c_double * 2), ("eps", c_double), ("weight_decay", c_double),
                ("max_grad_norm", c_double), ("ema_decay", c_double), ("decoupled", c_int32), ("reserved", c_int32)]


class Sde(ctypes.Structure):  # rgfm_sde: the stochastic step's strength and noise seed
    _fields_ = [("eta", c_double), ("seed", c_uint64)]


class Ess(ctypes.Structure):  # rgfm_ess: the effective-sample-size floor and the per-row exponents' sink
    _fields_ = [("ess_min", c_double), ("tau_out", c_void_p), ("tau_records", c_size_t)]


# name -> (restype, argtypes); every symbol include/rgfm.h declares.
SIGNATURES = {
    "rgfm_unet_param_floats": (c_int, [P(UNetDesc), P(c_size_t)]),
    "rgfm_unet_create": (c_int, [P(UNetDesc), c_void_p, c_size_t, c_void_p, P(c_void_p)]),
    "rgfm_unet_destroy": (None, [c_void_p]),
    "rgfm_unet_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_unet_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                  c_size_t, c_void_p]),
    "rgfm_unet_set_trace": (c_int, [c_void_p, c_int]),
    "rgfm_unet_p_handovers": (c_int, [c_void_p, P(c_int)]),
    "rgfm_unet_wino_convs": (c_int, [c_void_p, P(c_int)]),
    "rgfm_unet_up_merged": (c_int, [c_void_p, P(c_int)]),
    "rgfm_unet_conv_routes": (c_int, [c_void_p, P(c_int), c_int]),
    "rgfm_unet_time_embedding": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_unet_num_activations": (c_int, [c_void_p, P(c_int)]),
    "rgfm_unet_activation_shape": (c_int, [c_void_p, c_int, P(c_int), P(c_int), P(c_int)]),
    "rgfm_unet_read_activation": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "rgfm_unet_train_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_unet_forward_train": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, c_uint64,
                                        c_void_p, c_size_t, c_void_p]),
    "rgfm_unet_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_unet_vjp": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_unet_divergence_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_unet_divergence": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                     c_void_p, c_size_t, c_void_p]),
    "rgfm_unet_log_prob_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_unet_log_prob": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                   c_void_p, c_size_t, c_void_p]),
    "rgfm_unet_dropout_mask": (c_int, [c_void_p, c_int, c_uint64, c_float, c_int, c_void_p]),
    "rgfm_unet_update_params": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_ratio_param_floats": (c_int, [P(RatioDesc), P(c_size_t)]),
    "rgfm_ratio_create": (c_int, [P(RatioDesc), c_void_p, c_size_t, c_void_p, P(c_void_p)]),
    "rgfm_ratio_flex_param_floats": (c_int, [P(RatioFlexDesc), P(c_size_t)]),
    "rgfm_ratio_flex_create": (c_int, [P(RatioFlexDesc), c_void_p, c_size_t, c_void_p, P(c_void_p)]),
    "rgfm_ratio_destroy": (None, [c_void_p]),
    "rgfm_ratio_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_ratio_eval": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                c_size_t, c_void_p]),
    "rgfm_ratio_cross_workspace_bytes": (c_int, [c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_ratio_eval_cross": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                      c_size_t, c_void_p]),
    "rgfm_ratio_grad_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_ratio_grad_log_ratio": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                          c_void_p, c_size_t, c_void_p]),
    "rgfm_ratio_cond_prepare_workspace_bytes": (c_int, [c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_ratio_cond_prepare": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_ratio_grad_cond_workspace_bytes": (c_int, [c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_ratio_grad_log_ratio_cond": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                               c_size_t, c_void_p]),
    "rgfm_ratio_train_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_ratio_forward_train": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_uint64,
                                         c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_ratio_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                                    c_void_p]),
    "rgfm_ratio_pool_choice": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "rgfm_ratio_dropout_mask": (c_int, [c_void_p, c_int, c_uint64, c_float, c_int, c_void_p]),
    "rgfm_ratio_update_params": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_grad_workspace_bytes": (c_int, [c_void_p, c_void_p, c_void_p, c_int, P(c_size_t)]),
    "rgfm_sample_pair_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double,
                                      c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_single_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_sample_single": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                   c_size_t, c_void_p]),
    "rgfm_sample_cond_workspace_bytes": (c_int, [c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_cond": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_int,
                                 c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_cond_grad_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_cond_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_int,
                                      c_void_p, c_size_t, c_void_p]),
    "rgfm_guidance_apply_cond": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double,
                                         c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_pair": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_int, c_int, c_int, c_double, c_int, c_int, c_void_p,
                                 c_size_t, c_void_p]),
    # the sampler loops with a choice of solver (SOLVER_*): the Euler signatures with `solver` in front of ws / bytes
    "rgfm_sample_single_ode_workspace_bytes": (c_int, [c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_single_ode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                       c_void_p]),
    "rgfm_sample_pair_ode_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_pair_ode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     c_int, c_double, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_two_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_two": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                c_size_t, c_void_p]),
    "rgfm_sample_cond_ode_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_cond_ode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_int,
                                     c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_grad_ode_workspace_bytes": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_pair_grad_ode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double,
                                          c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_cond_grad_ode_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_cond_grad_ode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int,
                                          c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_fmnet_param_floats": (c_int, [P(FmNetDesc), P(c_size_t)]),
    "rgfm_fmnet_create": (c_int, [P(FmNetDesc), c_void_p, c_size_t, c_void_p, P(c_void_p)]),
    "rgfm_fmnet_destroy": (None, [c_void_p]),
    "rgfm_fmnet_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_fmnet_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                   c_size_t, c_void_p]),
    "rgfm_fmnet_sample_single": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                         c_size_t, c_void_p]),
    "rgfm_fmnet_sample_pair_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_fmnet_sample_pair": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int, c_int, c_int, c_double, c_int, c_int, c_void_p,
                                       c_size_t, c_void_p]),
    "rgfm_guidance_workspace_bytes": (c_int, [c_int, c_int, P(c_size_t)]),
    "rgfm_guidance_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_int, c_int, c_int, c_int, c_double, c_double,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    # guidance diagnostics: the block's inputs without gamma + diag_out; the *_ode loops (the FlowMatchingModel pair: its
    # Euler loop) with (diag_out, diag_records) in front of ws
    "rgfm_guidance_diag_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_guidance_diag": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                   c_int, c_int, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_guidance_diag_cond": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p,
                                        c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_diag_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_pair_diag": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                      c_int, c_double, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t,
                                      c_void_p]),
    "rgfm_sample_cond_diag_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_cond_diag": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int, c_int,
                                      c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_grad_diag_workspace_bytes": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_pair_grad_diag": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double,
                                           c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_cond_grad_diag_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_cond_grad_diag": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_int,
                                           c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "rgfm_fmnet_sample_pair_diag_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_fmnet_sample_pair_diag": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                            c_int, c_int, c_double, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t,
                                            c_void_p]),
    # cross pairing of the MC set: the ratio matrix [n_mc][n_mc] in the ratio vector's place; two optional weight outputs
    "rgfm_guidance_cross_workspace_bytes": (c_int, [c_int, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_guidance_apply_cross": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                          c_int, c_int, c_double, c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_guidance_diag_cross": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                         c_int, c_int, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_cross_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_pair_cross": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_int, c_double, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t,
                                       c_void_p]),
    # guidance strength as data: the *_diag loops (cross: rgfm_sample_pair_cross) with (gamma_rows [device fp32],
    # stage_scale [host doubles], n_stage_scale) behind gamma; the blocks with gamma_rows in gamma's place
    "rgfm_sample_pair_gs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                    c_int, c_double, c_void_p, P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                    c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_cross_gs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                          c_int, c_double, c_void_p, P(c_double), c_int, c_int, c_int, c_int, c_void_p,
                                          c_size_t, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_cond_gs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p,
                                    P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t,
                                    c_void_p]),
    "rgfm_sample_pair_grad_gs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_void_p,
                                         P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t,
                                         c_void_p]),
    "rgfm_sample_cond_grad_gs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p,
                                         P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t,
                                         c_void_p]),
    "rgfm_guidance_apply_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                         c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_guidance_apply_cond_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double,
                                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_guidance_apply_cross_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                               c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_size_t, c_void_p]),
    # the stochastic step: rgfm_sample_single_ode / the *_gs loops with `const rgfm_sde*` in front of ws
    "rgfm_sde_scratch_bytes": (c_int, [c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sde_noise": (c_int, [c_uint64, c_int, c_int, c_size_t, c_void_p, c_void_p]),
    "rgfm_sample_single_sde": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, P(Sde), c_void_p, c_size_t,
                                       c_void_p]),
    "rgfm_sample_pair_sde": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     c_int, c_double, c_void_p, P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                     P(Sde), c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_pair_cross_sde": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                           c_int, c_double, c_void_p, P(c_double), c_int, c_int, c_int, c_int, c_void_p,
                                           c_size_t, P(Sde), c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_cond_sde": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p,
                                     P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t, P(Sde), c_void_p, c_size_t,
                                     c_void_p]),
    "rgfm_sample_pair_grad_sde": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_void_p,
                                          P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t, P(Sde), c_void_p,
                                          c_size_t, c_void_p]),
    "rgfm_sample_cond_grad_sde": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p,
                                          P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t, P(Sde), c_void_p,
                                          c_size_t, c_void_p]),
    # the effective-sample-size floor: the *_sde MC loops with `const rgfm_ess*` in front of ws; the *_rows blocks with
    # (ess_min, tau_out) behind weights_out
    "rgfm_sample_pair_ess": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     c_int, c_double, c_void_p, P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                     P(Sde), P(Ess), c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_cond_ess": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p,
                                     P(c_double), c_int, c_int, c_int, c_int, c_void_p, c_size_t, P(Sde), P(Ess), c_void_p,
                                     c_size_t, c_void_p]),
    "rgfm_guidance_apply_ess": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                        c_int, c_int, c_double, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_size_t,
                                        c_void_p]),
    "rgfm_guidance_apply_cond_ess": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double,
                                             c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    # class conditioning and classifier-free guidance: the namesakes with num_classes behind the descriptor, labels
    # (device int32) behind t_count / the states, and a scale per net
    "rgfm_unet_labeled_param_floats": (c_int, [P(UNetDesc), c_int, P(c_size_t)]),
    "rgfm_unet_labeled_create": (c_int, [P(UNetDesc), c_int, c_void_p, c_size_t, c_void_p, P(c_void_p)]),
    "rgfm_unet_forward_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                         c_size_t, c_void_p]),
    "rgfm_unet_forward_train_labels": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_float,
                                               c_uint64, c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_single_cfg_workspace_bytes": (c_int, [c_void_p, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_single_cfg": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_int, c_int, c_int, c_int, c_int, P(Sde),
                                       c_void_p, c_size_t, c_void_p]),
    "rgfm_sample_two_cfg_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, P(c_size_t)]),
    "rgfm_sample_two_cfg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_int,
                                    c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_ubench_cfg_blend": (c_int, [c_size_t, P(c_double), P(c_double)]),
    "rgfm_profile_enable": (c_int, [c_int]),
    "rgfm_profile_reset": (c_int, []),
    "rgfm_profile_read": (c_int, [c_int, P(c_double), P(c_double), P(c_int64), P(c_double)]),
    "rgfm_profile_reserve": (c_int, [c_int64]),
    "rgfm_profile_span": (c_int, [c_int, P(c_double), P(c_double)]),
    "rgfm_ubench_mfma_f16": (c_int, [P(c_double)]),
    "rgfm_fmnet_train_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_fmnet_forward_train": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t,
                                         c_void_p]),
    "rgfm_fmnet_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_fmnet_update_params": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_clf_param_floats": (c_int, [P(ClfDesc), P(c_size_t)]),
    "rgfm_clf_create": (c_int, [P(ClfDesc), c_void_p, c_size_t, c_void_p, P(c_void_p)]),
    "rgfm_clf_destroy": (None, [c_void_p]),
    "rgfm_clf_update_params": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "rgfm_clf_train_workspace_bytes": (c_int, [c_void_p, c_int, P(c_size_t)]),
    "rgfm_clf_forward_train": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint64, c_float, c_void_p,
                                       c_void_p, c_size_t, c_void_p]),
    "rgfm_clf_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "rgfm_clf_xent": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rgfm_clf_pool_choice": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rgfm_clf_gate": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "rgfm_clf_dropout_mask": (c_int, [c_void_p, c_uint64, c_float, c_int, c_void_p]),
    "rgfm_adam_workspace_bytes": (c_int, [P(c_size_t)]),
    "rgfm_adam_grad_norm": (c_int, [c_void_p, c_int, c_uint64, c_uint64, c_void_p, c_size_t, c_void_p]),
    "rgfm_adam_step": (c_int, [P(AdamDesc), c_void_p, c_int, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_size_t, c_void_p]),
    "rgfm_ubench_hbm_copy": (c_int, [c_size_t, P(c_double)]),
    "rgfm_ubench_sde_pre": (c_int, [c_size_t, P(c_double), P(c_double)]),
    "rgfm_unet_set_conv_mode": (c_int, [c_void_p, c_int]),
    "rgfm_fmnet_set_conv_mode": (c_int, [c_void_p, c_int]),
    "rgfm_unet_range_flag": (c_int, [c_void_p, P(c_int), c_int, c_void_p]),
    "rgfm_fmnet_range_flag": (c_int, [c_void_p, P(c_int), c_int, c_void_p]),
    "rgfm_abi_version": (c_int, []),
    "rgfm_last_error": (ctypes.c_char_p, []),
}


# RGFM_DIAG_FLOATS of include/rgfm.h: fp32 values of one guidance-diagnostics record (utils/diagnostics.py names them)
DIAG_FLOATS = 8

# RGFM_SOLVER_* of include/rgfm.h by the name the Python samplers and the CLIs take
SOLVERS = {"euler": 0, "midpoint": 1}


def solver_id(solver):
    """RGFM_SOLVER_* of a solver name; any other value is a ValueError (raised before any device work)."""
    if not isinstance(solver, str) or solver not in SOLVERS:
        raise ValueError(f"solver must be 'euler' or 'midpoint', got {solver!r}")
    return SOLVERS[solver]


# RGFM_ROUTE_* of include/rgfm.h, in index order (rgfm_unet_conv_routes); slot ROUTE_T2 counts the CONV_T2 launches
ROUTES = ("hx2d", "hx2w", "hx2s", "hx2c", "hx2q", "hx2p", "hx2", "bx3", "f32")
ROUTE_T2 = len(ROUTES)


class RgfmError(RuntimeError):
    pass


def lib():
    """Return the loaded library, loading it on first use."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RgfmError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or "
            "`make -C ratio_guided_multimodal_fm_amd/csrc`). There is no CPU fallback.")
    handle = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if the library is stale
        fn.restype, fn.argtypes = res, args
    got = handle.rgfm_abi_version()
    if got != ABI_VERSION:
        raise RgfmError(f"librgfm_hip.so ABI {got} != expected {ABI_VERSION}; rebuild it")
    _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().rgfm_last_error()
        raise RgfmError(f"librgfm_hip error {rc}: {msg.decode() if msg else '?'}")
