"""ctypes binding of libcaldhip.so (include/cald_hip.h).

This is the thin FFI shim of the drop-in boundary: every symbol declared in include/cald_hip.h is
bound here with its exact C signature.  There is NO fallback: if the library is missing, or no
MI355X is visible when a compute call is made, the call raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcaldhip.so")
_lib = None

c_f = C.POINTER(C.c_float)
c_i = C.POINTER(C.c_int)
c_i64 = C.POINTER(C.c_int64)
c_d = C.POINTER(C.c_double)
c_u8 = C.POINTER(C.c_uint8)
c_i8 = C.POINTER(C.c_int8)


class ModelCfg(C.Structure):
    _fields_ = [("arch", C.c_int), ("depth", C.c_int), ("num_classes", C.c_int), ("min_size", C.c_int),
                ("max_size", C.c_int), ("box_score_thresh", C.c_float), ("box_nms_thresh", C.c_float),
                ("detections_per_img", C.c_int), ("rpn_pre_nms_top_n", C.c_int), ("rpn_post_nms_top_n", C.c_int),
                ("rpn_nms_thresh", C.c_float), ("precision", C.c_int)]


PRECISION = {"fp32": 0, "f16x3": 1}


class View(C.Structure):
    _fields_ = [("image_dev", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("flip", C.c_int), ("nrect", C.c_int),
                ("rects", C.c_int * 16), ("noise_dev", C.c_void_p)]


class Dets(C.Structure):
    _fields_ = [("boxes_dev", C.c_void_p), ("scores_dev", C.c_void_p), ("labels_dev", C.c_void_p),
                ("props_dev", C.c_void_p), ("prob_max_dev", C.c_void_p), ("scores_cls_dev", C.c_void_p),
                ("count_dev", C.c_void_p), ("cap", C.c_int)]


MAX_AUGS = 32
N_MARGINS = 16          # CALD_N_MARGINS
EVAL_MAX_DT, EVAL_MAX_GT = 128, 256     # CALD_EVAL_MAX_DT / CALD_EVAL_MAX_GT: per-segment caps of cald_op_coco_match / cald_op_voc_match
MARGIN_NAMES = ['rpn_topk', 'rpn_iou', 'rpn_order', 'rpn_trunc', 'rpn_small', 'roi_level', 'roi_edge', 'post_thr', 'post_iou', 'post_order',
                'post_cap', 'ref_subsample', 'argmax', 'zero_row', 'cutout', 'post_small']
# Rounding noise of precision="f16x3" against the exact mode on each margin's scale, calibrated on 1 536 configs[1] images
# (tools/cascade_margins.py, profiles/r5_cascade_margins.txt): about the 90th percentile of |margin_exact - margin_f16x3|.
MARGIN_NOISE_F16X3 = [2e-5, 2e-6, 2e-5, 2e-5, 1e-5, 1e-6, 1e-4, 5e-6, 2e-6, 5e-6, 5e-6, 5e-6, 2e-6, 5e-6, 2e-6, 0.0]
# The same for a RetinaNet (sigmoid scores, boxes from the regression head; 0.0 where the kind cannot occur), measured on plain forwards of
# 256 pool-seed-1 images, not on the audit's own output (tools/retina_f16x3_noise.py, profiles/retina_f16x3_noise.json): the 90th percentile
# of |delta score| (7, 9, 10, 11, 13), of |delta IoU| between neighbouring same-class detections (8, 12) and of |delta box coordinate| on
# the resized image (15); slot 14 is host arithmetic and keeps the row above's value.
MARGIN_NOISE_F16X3_RETINA = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 6.3e-07, 4.6e-07, 6.3e-07, 6.3e-07, 6.3e-07, 4.6e-07, 6.3e-07, 2e-06, 0.00012]
AUG_FLIP, AUG_GAUSS, AUG_COLOR_ADJUST, AUG_COLOR_SWAP, AUG_SALT_PEPPER, AUG_CUTOUT, AUG_RESIZE, AUG_ROTATE = range(1, 9)
MAX_NOISE_SEG = 16    # CALD_MAX_NOISE_SEG: GaussianNoise / SaltPepperNoise views drawn from one generator


class AugSpec(C.Structure):
    _fields_ = [("kind", C.c_int), ("param", C.c_double)]


class PackJob(C.Structure):
    """cald_pack_job of include/cald_hip.h: the arguments of one cald_train_pack_conv call (device pointers)."""
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p),
                ("Cout", C.c_int), ("Cin", C.c_int), ("KH", C.c_int), ("KW", C.c_int), ("CinK", C.c_int), ("mode", C.c_int),
                ("packed", C.c_void_p), ("w16", C.c_void_p), ("w16_S", C.c_int)]


class LLCfg(C.Structure):
    """cald_ll_cfg of include/cald_hip.h."""
    _fields_ = [("batch_views", C.c_int), ("levels", C.c_int * 4)]


class VaalCfg(C.Structure):
    """cald_vaal_cfg of include/cald_hip.h."""
    _fields_ = [("bn_mode", C.c_int), ("batch_images", C.c_int)]


VAAL_BN_BATCH, VAAL_BN_RUNNING = 0, 1


class LossNetTensors(C.Structure):
    """cald_lossnet_tensors of include/cald_hip.h: LossNet's parameters (or gradients) as device pointers in state_dict() layout."""
    _fields_ = [("fc_w", C.c_void_p * 4), ("fc_b", C.c_void_p * 4), ("lin_w", C.c_void_p), ("lin_b", C.c_void_p)]


class SweepCfg(C.Structure):
    _fields_ = [("base_seed", C.c_uint64), ("bp", C.c_float), ("batch_images", C.c_int), ("n_augs", C.c_int),
                ("augs", AugSpec * MAX_AUGS)]


PROBE_MAX_VIEWS = 8
PROBE_MAX_RECTS = 8


class ConvProbe(C.Structure):
    """cald_conv_probe (include/cald_hip.h): one conv launch for cald_op_conv_probe."""
    _fields_ = [("V", C.c_int), ("in_hw", (C.c_int * 2) * PROBE_MAX_VIEWS), ("up_hw", (C.c_int * 2) * PROBE_MAX_VIEWS),
                ("dyn_rows", C.c_int * PROBE_MAX_VIEWS), ("has_dyn", C.c_int), ("gather", C.c_int), ("nrect", C.c_int * PROBE_MAX_VIEWS),
                ("rect", ((C.c_int * 4) * PROBE_MAX_RECTS) * PROBE_MAX_VIEWS),
                ("Cin", C.c_int), ("Cout", C.c_int), ("KH", C.c_int), ("KW", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
                ("relu", C.c_int), ("in_relu", C.c_int), ("out_ld", C.c_int), ("cin_true", C.c_int),
                ("weight", c_f), ("bias", c_f), ("bn_scale", c_f), ("bn_shift", c_f), ("in_", c_f), ("in16", C.POINTER(C.c_uint32)),
                ("residual", c_f), ("up", c_f), ("ex16", C.c_int), ("mask", c_f), ("row_map", c_i),
                ("out", c_f), ("out_n", C.c_int64), ("out16", C.POINTER(C.c_uint32)), ("out16_n", C.c_int64),
                ("energy4", c_f), ("energy4_n", C.c_int64),
                ("head_w", c_f), ("head_b", c_f), ("head_out", c_f), ("head_out_n", C.c_int64), ("head_ld", C.c_int),
                ("row_packing", C.c_int)]      # 0 auto (the product's choice), 1 per-view row tiles, 2 packed row tiles


PRUNE_PROBE_MAX_VIEWS = 8


class RpnPruneProbe(C.Structure):
    """cald_rpn_prune_probe (include/cald_hip.h): the arguments and results of cald_op_rpn_prune."""
    _fields_ = [("V", C.c_int), ("guard", C.c_int), ("hw", ((C.c_int * 2) * PRUNE_PROBE_MAX_VIEWS) * 2),
                ("pre_n", C.c_int), ("head_ld", C.c_int), ("c1", C.c_float * 3), ("c0", C.c_float * 3),
                ("energy", c_f * 2), ("exact", c_f * 2), ("head", c_f * 2), ("pnorm", c_f * 2),
                ("tau_key", C.POINTER(C.c_uint32)), ("row_map", (c_i * 2) * 2), ("nsel", c_i * 2),
                ("check", C.c_float * 2), ("stat", C.c_uint64 * 4)]


class ScoreProbe(C.Structure):
    """cald_score_probe (include/cald_hip.h): one sweep batch for cald_op_score_batch."""
    _fields_ = [("V", C.c_int), ("cap", C.c_int), ("C", C.c_int), ("n_img", C.c_int), ("P", C.c_int), ("bp", C.c_float),
                ("boxes", c_f), ("props", c_f), ("scores", c_f), ("labels", c_i64), ("scores_cls", c_f), ("prob_max", c_f), ("count", c_i),
                ("view_img", c_i), ("view_isref", c_i), ("ref_sel", c_i), ("ref_n", c_i),
                ("ref_view", c_i), ("aug_view", c_i), ("pair_img", c_i), ("aug_kind", c_i), ("aug_param", c_f),
                ("cons", c_f), ("cls_corr", c_f), ("pair_audit", c_f), ("max_iou", c_f), ("lt", c_f)]


class WgradPlan(C.Structure):
    """cald_wgrad_plan (include/cald_hip.h): what cald_train_wgrad_plan answers."""
    _fields_ = [("variant", C.c_int), ("reduce", C.c_int), ("MT", C.c_int), ("JT", C.c_int), ("S", C.c_longlong), ("chunk", C.c_longlong),
                ("csplit", C.c_longlong), ("rows_per_block", C.c_longlong), ("scratch_bytes", C.c_longlong),
                ("kernel", C.c_char * 48), ("reduce_kernel", C.c_char * 32)]


# cald_ssm_pick_fn of include/cald_hip.h.  The entry points that take one declare it c_void_p, so that a Python callback
# (C.cast(PICK_FN(f), C.c_void_p)) and a C function of the library (C.cast(lib().cald_ssm_pick_mt19937, C.c_void_p)) both pass.
PICK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, c_i, c_i, c_i)
SSM_RETINA_TAKE = 500    # CALD_SSM_RETINA_TAKE

# name -> (restype, argtypes): must list every symbol of include/cald_hip.h
SIGNATURES = {
    "cald_last_error": (C.c_char_p, []),
    "cald_version": (C.c_int, []),
    "cald_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cald_ctx_destroy": (C.c_int, [C.c_void_p]),
    "cald_ctx_sync": (C.c_int, [C.c_void_p]),
    "cald_model_create": (C.c_int, [C.c_void_p, C.POINTER(ModelCfg), C.POINTER(C.c_void_p)]),
    "cald_model_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, c_f, c_i64, C.c_int]),
    "cald_model_finalize": (C.c_int, [C.c_void_p]),
    "cald_model_set_rpn_prune": (C.c_int, [C.c_void_p, C.c_int, c_i]),
    "cald_model_set_rpn_prune_capture": (C.c_int, [C.c_void_p, C.c_int]),
    "cald_model_rpn_prune_bound": (C.c_int, [C.c_void_p, c_f, c_f]),
    "cald_model_set_rpn_prune_bound": (C.c_int, [C.c_void_p, c_f, c_f]),
    "cald_profile_prune_fallbacks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "cald_model_destroy": (C.c_int, [C.c_void_p]),
    "cald_forward": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(View), C.POINTER(Dets)]),
    "cald_debug_cutout_forward": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(View), C.POINTER(Dets), C.c_int]),
    "cald_sweep": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, c_i64, C.POINTER(SweepCfg), c_d, c_d]),
    "cald_sweep_audit": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, c_i64, C.POINTER(SweepCfg), c_d, c_d, c_f]),
    "cald_sweep_ltc": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, C.c_int, c_d]),
    "cald_sweep_ssm": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, C.c_int, C.c_int64, c_i, c_i, c_f, c_f, c_i8, c_i64]),
    "cald_ssm_pick_mt19937": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_i, c_i, c_i]),
    "cald_sweep_ssm_retina": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, c_i, c_i, c_f, c_f,
                                        c_i8, c_i64]),
    "cald_sweep_lsc": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, c_i64, C.c_uint64, C.c_int, c_d]),
    "cald_lossnet_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cald_lossnet_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, c_f, c_i64, C.c_int]),
    "cald_lossnet_finalize": (C.c_int, [C.c_void_p]),
    "cald_lossnet_destroy": (C.c_int, [C.c_void_p]),
    "cald_sweep_ll": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, c_i, C.POINTER(LLCfg), c_d, c_f]),
    "cald_vaal_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cald_vaal_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, c_f, c_i64, C.c_int]),
    "cald_vaal_finalize": (C.c_int, [C.c_void_p]),
    "cald_vaal_destroy": (C.c_int, [C.c_void_p]),
    "cald_sweep_vaal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, c_i, C.POINTER(VaalCfg), c_f, c_f]),
    "cald_op_vaal_resize": (C.c_int, [C.c_void_p, c_u8, C.c_int, C.c_int, c_f]),
    "cald_op_vaal_bn_relu": (C.c_int, [C.c_void_p, c_f, C.c_longlong, C.c_int, C.c_int, C.c_int, c_f, c_f, c_f]),
    "cald_op_vaal_fc_mu": (C.c_int, [C.c_void_p, C.c_int, c_f, c_f]),
    "cald_op_vaal_head": (C.c_int, [C.c_void_p, C.c_int, c_f, c_f]),
    "cald_train_gap": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, C.c_void_p]),
    "cald_lossnet_train_fwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(LossNetTensors), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cald_lossnet_train_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(LossNetTensors), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(LossNetTensors), C.c_int, C.c_void_p]),
    "cald_loss_pred_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cald_op_gap": (C.c_int, [C.c_void_p, c_f, C.c_int, C.c_int, C.c_int, c_f]),
    "cald_op_lossnet": (C.c_int, [C.c_void_p, C.c_int, c_f, c_f]),
    "cald_op_consistency": (C.c_int, [C.c_void_p, C.c_int, c_f, c_f, c_f, C.c_int, c_f, c_f, c_f, C.c_int, C.c_float, c_f]),
    "cald_op_cls_corr": (C.c_int, [C.c_void_p, C.c_int, c_f, c_i64, C.c_int, c_f]),
    "cald_op_score_batch": (C.c_int, [C.c_void_p, C.POINTER(ScoreProbe)]),
    "cald_op_pair_params": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, c_f]),
    "cald_op_ls_tail": (C.c_int, [C.c_int, c_f, C.c_int, c_f, c_i, c_i, c_d]),
    "cald_op_coco_match": (C.c_int, [C.c_void_p, C.c_int, c_i64, c_i64, c_d, c_d, c_d, c_d, c_u8, c_u8, C.c_int, c_d, C.c_int, c_d,
                                     C.POINTER(C.c_int32), c_u8, c_u8]),
    "cald_op_voc_match": (C.c_int, [C.c_void_p, C.c_int, c_i64, c_i64, c_d, c_u8, c_d, c_i64, C.c_int, c_d, C.c_int64, c_d, c_i64, c_u8, c_u8]),
    "cald_op_pil_resize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "cald_op_cutout_rects": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, c_f, C.c_int, c_i, c_i]),
    "cald_op_cutout_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_i, C.c_int, c_i, c_i]),
    "cald_op_augment": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_int, c_f,
                                  C.c_void_p, c_f, c_i]),
    "cald_op_noise_stream": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_int, c_i, c_d, C.POINTER(C.c_void_p)]),
    "cald_op_frcnn_postprocess": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_f, c_f, c_f, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                            C.c_int, c_f, c_f, c_i64, c_f, c_f, c_f, c_i]),
    "cald_op_frcnn_postprocess_min": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_f, c_f, c_f, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                                C.c_int, C.c_float, c_f, c_f, c_i64, c_f, c_f, c_f, c_i]),
    "cald_op_ssm_postprocess": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_f, c_f, c_f, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                          c_i, c_i, c_f, c_f, c_i8]),
    "cald_op_retina_postprocess": (C.c_int, [C.c_void_p, C.POINTER(c_f), C.POINTER(c_f), c_i, C.c_int, C.c_int, c_f] + [C.c_int] * 6
                                   + [C.c_float, C.c_float, C.c_int, c_f, c_f, c_i64, c_f, c_f, c_i]),
    "cald_op_retina_audit": (C.c_int, [C.c_void_p, C.POINTER(c_f), C.POINTER(c_f), c_i, C.c_int, C.c_int, c_f] + [C.c_int] * 6
                             + [C.c_float, C.c_float, C.c_int, c_i, c_f]),
    "cald_op_retina_ssm_postprocess": (C.c_int, [C.c_void_p, C.POINTER(c_f), C.POINTER(c_f), c_i, C.c_int, C.c_int, c_f] + [C.c_int] * 6
                                       + [C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, c_i, c_i, c_i, c_f, c_f, c_i8]),
    "cald_op_rpn_prune": (C.c_int, [C.c_void_p, C.POINTER(RpnPruneProbe)]),
    "cald_op_roi_align": (C.c_int, [C.c_void_p, C.POINTER(c_f), c_i, C.c_int, C.c_int, c_f, c_f]),
    "cald_op_roi_align_views": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(c_f), c_i, c_i, c_f, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_uint32), c_i]),
    "cald_op_conv2d": (C.c_int, [C.c_void_p, c_f, C.c_int, C.c_int, C.c_int, c_f, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, c_f, c_f, c_f, c_f, C.c_int, c_f]),
    "cald_op_conv_probe": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ConvProbe), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "cald_op_mfma_f16": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64]),
    "cald_op_conv2d_f16x3": (C.c_int, [C.c_void_p, c_f, C.c_int, C.c_int, C.c_int, c_f, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, c_f, c_f, c_f, c_f, C.c_int, c_f]),
    "cald_op_conv_bench": (C.c_int, [C.c_void_p] + [C.c_int] * 12 + [c_d, c_d]),
    "cald_op_row_pack_lookup": (C.c_int, [C.c_int, c_i, c_i, C.c_int, C.c_int, C.c_int64, c_i64, c_i, c_i64, c_i64]),
    "cald_op_transform_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, c_i, c_i, c_i, c_i]),
    "cald_debug_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, c_f, C.c_int64, c_i64]),
    "cald_jpeg_info": (C.c_int, [C.c_void_p, C.c_size_t, c_i, c_i, c_i]),
    "cald_jpeg_decode_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)]),
    "cald_jpeg_probe": (C.c_int, [C.c_void_p, C.c_size_t, c_i, c_i, c_i, c_i]),
    "cald_jpeg_decode_batch_any": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)]),
    "cald_jpeg_decode_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "cald_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "cald_profile_read": (C.c_int, [C.c_void_p, c_d, c_d, c_i64, c_d]),
    "cald_profile_prune": (C.c_int, [C.c_void_p, c_d, c_d, c_d, c_d, c_d]),
    "cald_profile_roi_rows": (C.c_int, [C.c_void_p, c_d, c_i64]),
    "cald_profile_cutout": (C.c_int, [C.c_void_p, c_d, c_d, c_i64, c_i64]),
    "cald_model_set_cutout_reuse": (C.c_int, [C.c_void_p, C.c_int, c_i]),
    "cald_profile_cutout_stages": (C.c_int, [C.c_void_p, c_d, c_d, c_d, c_d, c_i64]),
    "cald_model_set_cutout_retention_cap": (C.c_int, [C.c_void_p, C.c_int64, c_i64]),
    "cald_op_cutout_fpn_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_i, C.c_int, c_i, c_i]),
    "cald_model_set_look_fuse": (C.c_int, [C.c_void_p, C.c_int, c_i]),
    "cald_model_set_row_packing": (C.c_int, [C.c_void_p, C.c_int, c_i]),
    "cald_model_set_box_min_size": (C.c_int, [C.c_void_p, C.c_float, c_f]),
    "cald_profile_dump": (C.c_int, [C.c_void_p, C.c_char_p]),
    # training step (device pointers as c_void_p)
    "cald_train_packed_floats": (C.c_int, [C.c_int] * 6 + [c_i64]),
    "cald_train_pack_conv": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p]),
    "cald_train_packed16_bytes": (C.c_int, [C.c_int] * 6 + [c_i64]),
    "cald_train_f16x3_scale": (C.c_int, [C.c_float, c_i, c_f]),
    "cald_train_pack_conv16": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_int]),
    "cald_train_pack_plan_scratch_floats": (C.c_int, [C.c_int, C.POINTER(PackJob), c_i64]),
    "cald_train_pack_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(PackJob), C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "cald_train_pack_plan_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cald_train_pack_plan_destroy": (C.c_int, [C.c_void_p]),
    "cald_train_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 8
                        + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "cald_train_conv_group": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_i, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)] + [C.c_int] * 8
                              + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]),
    "cald_train_conv_f16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 8
                              + [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
                              + [C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_char_p)]),
    "cald_train_conv_group_f16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_i, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)] + [C.c_int] * 8
                                    + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]
                                    + [C.POINTER(C.c_void_p), c_f, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)]),
    "cald_train_packed_grad16_bytes": (C.c_int, [C.c_int] * 6 + [c_i64]),
    "cald_train_f16x3_grad_scale": (C.c_int, [C.c_float, c_i, c_f]),
    "cald_train_conv_dgrad_f16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 6
                                    + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_char_p)]),
    "cald_train_conv_dgrad_group_f16x3": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_i, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)] + [C.c_int] * 6
                                          + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), c_f, c_f, C.POINTER(C.c_char_p)]),
    "cald_train_conv_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "cald_train_linear_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_int]),
    "cald_train_wgrad_plan": (C.c_int, [C.c_longlong] + [C.c_int] * 12 + [C.POINTER(WgradPlan)]),
    "cald_train_relu_bwd": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cald_train_add": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cald_train_dilate": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p]),
    "cald_train_upsample_bwd": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "cald_train_rpn_proposals": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_i, C.POINTER(C.c_void_p), c_i, C.c_int, C.c_int, C.c_int,
                                           C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "cald_train_roi_sample_host": (C.c_int, [C.c_int, c_i, c_i, c_i, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i, c_i, c_i]),
    "cald_train_roi_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_void_p, C.c_void_p]),
    "cald_train_anchors": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_i, C.c_void_p]),
    "cald_train_match": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "cald_train_box_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "cald_train_roi_align": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), c_i, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cald_train_roi_align_bwd": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_i, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cald_train_softmax_ce": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "cald_train_smooth_l1": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_float,
                                       C.c_void_p, C.c_void_p]),
    "cald_train_focal_loss": (C.c_int, [C.c_void_p, C.c_int, c_i, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "cald_train_bce_logits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "cald_train_softmax_ce_seg": (C.c_int, [C.c_void_p, C.c_int, c_i, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cald_train_smooth_l1_seg": (C.c_int, [C.c_void_p, C.c_int, c_i, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, c_f, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "cald_train_bce_logits_seg": (C.c_int, [C.c_void_p, C.c_int, c_i, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cald_train_focal_loss_seg": (C.c_int, [C.c_void_p, C.c_int, c_i, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            c_f, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cald_train_seg_mean": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cald_train_add_bcast": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]),
    "cald_train_preprocess": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i, C.c_int, C.c_int, C.c_void_p]),
    "cald_train_maxpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cald_train_subsample2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cald_train_sgd": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int]),
    "cald_train_seg_cache_size": (C.c_int, []),
    "cald_comm_unique_id": (C.c_int, [C.c_void_p]),
    "cald_comm_init_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "cald_comm_adopt": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cald_comm_info": (C.c_int, [C.c_void_p, c_i, c_i]),
    "cald_comm_destroy": (C.c_int, [C.c_void_p]),
    "cald_allgather_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
}


def lib():
    """Loads libcaldhip.so.  torch is imported first so that both share one HIP runtime
    (torch's bundled libamdhip64.so.7 satisfies the library's NEEDED entry)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libcaldhip.so is not built (%s missing): run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` or `make -C cald_amd/csrc`; there is no CPU fallback" % LIB_PATH)
        import torch  # noqa: F401  (loads the HIP runtime)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


ERR_UNSUPPORTED = -5


def check(rc):
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError("libcaldhip: %s (code %d)" % (lib().cald_last_error().decode(), rc))
    if rc != 0:
        raise RuntimeError("libcaldhip: %s (code %d)" % (lib().cald_last_error().decode(), rc))


def ptr(a, t=c_f):
    return a.ctypes.data_as(t) if a is not None else None
