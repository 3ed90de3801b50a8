"""ctypes binding of the C-ABI in include/s2i_hip.h (libs2i_hip.so, built by csrc/Makefile).

There is no CPU fallback: if the shared library is missing, or a call is made on a tensor that
is not resident on a gfx950 device, this module raises.  torch must be imported first so that the
library's libamdhip64 dependency resolves to the HIP runtime torch already loaded.
"""
import ctypes
import os

import torch  # noqa: F401  (loads the HIP runtime the kernels attach to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libs2i_hip.so")

# enums of include/s2i_hip.h
CONV_K1, CONV_K3S1, CONV_K4S2, TCONV_K4S2, CONV_1D = 0, 1, 2, 3, 4
ACT_NONE, ACT_GLU, ACT_LRELU, ACT_TANH, ACT_RELU = 0, 1, 2, 3, 4
PACK_PLAIN, PACK_UPFOLD = 0, 1
DT_F32, DT_BF16 = 0, 1
POOL_MAX3S2, POOL_AVG3S1, POOL_GLOBAL = 0, 1, 2
POOL_THEN_LRN, LRN_THEN_POOL = 0, 1
LOGMEL_BFT, LOGMEL_NHWC = 0, 1
ENC_LOSS_JEL, ENC_LOSS_L1, ENC_LOSS_DISTILL = 1, 2, 4
LOGMEL_TILE_FRAMES = 64
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = 0, 1, 2, 3, 4, 5
RESAMPLE_TILE = 1024
RESAMPLE_MAX_WINDOW = 13826
TOPK_MAX = 64
RANK_GATHER, RANK_COUNT = 0, 1      # s2i_rank_rows modes (S2I_RANK_*)
DIFFAUG_COLOR, DIFFAUG_TRANSLATION, DIFFAUG_CUTOUT = 1, 2, 4
GRAD_CHUNK, GRAD_STATS_HEAD = 4096, 16      # S2I_GRAD_CHUNK, S2I_GRAD_STATS_HEAD
ABI_VERSION = 7
# s2i_wgrad_plan_query: the WgKernel values of csrc/s2i_igemm.h in order, and the twelve outputs
WGRAD_KERNELS = ("f32-128x128", "f32-128x64", "f32-128x32", "f32-64x64", "f32-256x128", "f32-256x256", "f32-96x64", "f32-96x32",
                 "f32in-128x128", "b16-128x128", "b16-128x64", "b16-128x32", "b16-64x64", "b16-256x128", "b16-256x256",
                 "b16d1-64x64", "split-128x128", "split-128x64", "split-128x32", "split-64x64", "rows3-32x64", "rows3-32x32",
                 "rows3-64x128", "rows3-64x64", "rows3-64x32", "smalln-16", "smalln-32", "smalln-64")
WGRAD_PLAN_FIELDS = ("kernel", "bm", "bn", "threads", "gx", "gy", "gz", "stage", "slabs", "ws_slabs", "K", "M")
# s2i_conv_plan_query: the FwdKernel values of csrc/s2i_igemm.h in order, the fifteen outputs and its reduction kinds
FWD_KERNELS = ("f32-128x128", "f32-128x64", "f32-128x32", "f32-96x128", "f32in-128x128", "f32in-128x64", "f32in-128x32",
               "f32in-96x128", "split-128x128", "split-128x64", "split-128x32", "smalln-4", "smalln-8", "smalln-16",
               "tconv-n4-64", "conv3-n4-16", "conv3-n4-32", "rgb-out-4", "rgb-out-8", "rgb-out-9", "rgb-out-16", "rgb-out-18",
               "rgb-out-36", "rgb-in-1x3", "rgb-in-2x3", "rgb-in-1x4", "rgb-in-2x4", "thin-out", "thin-in-16", "thin-in-32")
FWD_PLAN_FIELDS = ("kernel", "bm", "bn", "threads", "gx", "gy", "gz", "splitk", "cps", "nchunks", "prep_elems", "reduce",
                   "ws_bytes", "M", "K")
FWD_REDUCE_NONE, FWD_REDUCE_PLAIN, FWD_REDUCE_COLSTATS, FWD_REDUCE_STATS = 0, 1, 2, 3
# s2i_conv_bf16_plan_query: the B16Kernel values of csrc/s2i_bf16.h in order (kind-BNxCK of the 128-pixel kernel, then the
# 256-pixel forms) and the twenty-one outputs
B16_KERNELS = ("b16-k3s1-128x16", "b16-k3s1-64x32", "b16-k3s1-32x64", "b16-k3s1-32x32", "b16-k4s2-128x32", "b16-k4s2-128x16",
               "b16-k4s2-64x32", "b16-k4s2-32x32", "b16-tconv-128x32", "b16-tconv-64x64", "b16-tconv-32x64", "b16-tconv-32x32",
               "b16v2-k3s1", "b16v2-tconv", "b16v2-k4s2-pw66", "b16v2-k4s2")
B16_PLAN_FIELDS = ("kernel", "pixels", "bn", "ck", "threads", "gx", "gy", "gz", "tw", "th", "tb", "tiles", "splitk", "cps",
                   "nchunks", "parts", "npad", "w_elems", "smem", "ws_bytes", "rows")

c_int, c_float, c_void_p, c_size_t, c_ll = (ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_longlong)


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("kind", "B", "H", "W", "Cx", "Cc", "N", "wmode", "flip", "wR",
                                     "ldw", "act", "stats", "ldy", "groups", "nosplit", "kw", "stride", "pad",
                                     "tile_rows", "in_act", "in_groups")]


class Conv2dDesc(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("B", "H", "W", "C", "ldx", "N", "kh", "kw", "sh", "sw", "ph", "pw", "Ho", "Wo",
                                     "ldy", "coff", "relu", "tile")]


class WgradDesc(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("kind", "B", "H", "W", "Ca", "Cc", "N", "ldg", "swap", "fold",
                                     "O", "I", "KH", "KW", "accumulate", "i_off", "I_total", "a_act", "a_groups")]


class PackItem(ctypes.Structure):
    _fields_ = [("w", c_void_p), ("packed", c_void_p)] + [(n, c_int) for n in ("O", "I", "KH", "KW", "Ip", "mode", "gx",
                                                                               "block0")]


class Pack16Item(ctypes.Structure):
    _fields_ = [("P", c_void_p), ("out", c_void_p)] + [(n, c_int) for n in (
        "R", "C", "kind", "flip", "transpose", "T", "nphase", "Nn", "Npad", "Kk", "CK", "gx", "gy", "block0")]


P = c_void_p
_SIGNATURES = {
    "s2i_last_error": (ctypes.c_char_p, []),
    "s2i_version": (c_int, []),
    "s2i_check_device": (c_int, []),
    "s2i_set_tuning": (c_int, [ctypes.c_char_p, c_int]),
    "s2i_get_tuning": (c_int, [ctypes.c_char_p, ctypes.POINTER(c_int)]),
    "s2i_conv_workspace_bytes": (c_size_t, [ctypes.POINTER(ConvDesc)]),
    "s2i_conv_stat_parts": (c_int, [ctypes.POINTER(ConvDesc)]),
    "s2i_conv_plan_query": (c_int, [ctypes.POINTER(ConvDesc), c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int * 15)]),
    "s2i_conv_forward": (c_int, [ctypes.POINTER(ConvDesc), P, P, P, P, P, P, P, c_size_t, P]),
    "s2i_conv_forward_cls": (c_int, [ctypes.POINTER(ConvDesc), P, P, P, P, P, P, P, P, c_size_t, P]),
    "s2i_conv_forward_in": (c_int, [ctypes.POINTER(ConvDesc), P, P, P, P, P, P, c_size_t, P]),
    "s2i_conv_wgrad_in_eligible": (c_int, [ctypes.POINTER(WgradDesc)]),
    "s2i_conv_wgrad_in": (c_int, [ctypes.POINTER(WgradDesc), P, P, P, P, P, c_size_t, P]),
    "s2i_conv_split_eligible": (c_int, [ctypes.POINTER(ConvDesc)]),
    "s2i_conv_forward_split": (c_int, [ctypes.POINTER(ConvDesc), P, P, P, c_int, c_int, c_int, P, P, P, P, P, c_size_t, P]),
    "s2i_split_packed_weight": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P]),
    "s2i_wgrad_workspace_bytes_split": (c_size_t, [ctypes.POINTER(WgradDesc), c_int]),
    "s2i_conv_wgrad_split": (c_int, [ctypes.POINTER(WgradDesc), c_int, P, P, P, P, P, c_size_t, P]),
    "s2i_conv_bf16_plan_query": (c_int, [ctypes.POINTER(ConvDesc), ctypes.POINTER(c_ll * 21)]),
    "s2i_pack16_item_fill": (c_int, [ctypes.POINTER(ConvDesc), P, c_int, c_int, P, ctypes.POINTER(Pack16Item)]),
    "s2i_pack_conv_weights_bf16_batched": (c_int, [P, c_int, c_int, P]),
    "s2i_pack_conv_weight_bf16": (c_int, [ctypes.POINTER(ConvDesc), P, c_int, c_int, P, P]),
    "s2i_conv_forward_bf16": (c_int, [ctypes.POINTER(ConvDesc), P, P, P, P, P, P, c_size_t, P]),
    "s2i_conv_forward_dt": (c_int, [ctypes.POINTER(ConvDesc), P, c_int, P, P, P, P, P, c_int, P, P, c_size_t, P]),
    "s2i_wgrad_workspace_bytes_dt": (c_size_t, [ctypes.POINTER(WgradDesc), c_int, c_int]),
    "s2i_conv_wgrad_dt": (c_int, [ctypes.POINTER(WgradDesc), P, c_int, P, P, c_int, P, P, c_size_t, P]),
    "s2i_wgrad_plan_query": (c_int, [ctypes.POINTER(WgradDesc), c_int, c_int, c_int, c_int, ctypes.POINTER(c_int * 12)]),
    "s2i_bn_act_forward_dt": (c_int, [c_int, P, c_ll, c_int, c_int, P, c_int, P, P, P]),
    "s2i_bn_act_bwd_reduce_dt": (c_int, [c_int, P, P, c_int, c_ll, c_int, c_int, P, c_int, P, c_int, P]),
    "s2i_bn_act_bwd_apply_dt": (c_int, [c_int, P, P, c_int, c_ll, c_int, c_int, P, P, c_int, P, P]),
    "s2i_act_backward_dt": (c_int, [c_int, P, P, c_int, c_ll, c_int, c_int, P, P]),
    "s2i_nchw_to_nhwc_dt": (c_int, [c_int, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "s2i_nhwc_to_nchw_dt": (c_int, [c_int, P, c_int, P, c_int, c_int, c_int, c_int, P]),
    "s2i_spatial_sum_dt": (c_int, [c_int, P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "s2i_tap_sums_dt": (c_int, [c_int, P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "s2i_cast": (c_int, [P, c_int, P, c_int, c_ll, P]),
    "s2i_cvec_bias_table": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "s2i_border_sums_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "s2i_tap_sums": (c_int, [P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "s2i_cvec_grads": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P]),
    "s2i_wgrad_workspace_bytes": (c_size_t, [ctypes.POINTER(WgradDesc)]),
    "s2i_conv_wgrad": (c_int, [ctypes.POINTER(WgradDesc), P, P, P, P, P, c_size_t, P]),
    "s2i_pack_conv_weight": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "s2i_pack_conv_weights_batched": (c_int, [P, c_int, c_int, c_int, P]),
    "s2i_bn_finalize": (c_int, [P, c_int, c_int, c_int, c_ll, P, P, P, P, P, c_float, c_float, P, P]),
    "s2i_bn_eval_coeffs": (c_int, [c_int, P, P, P, P, c_float, P, P]),
    "s2i_bn_act_forward": (c_int, [P, c_ll, c_int, c_int, P, c_int, P, P, P]),
    "s2i_colstats": (c_int, [P, c_ll, c_int, c_int, P, c_int, P]),
    "s2i_bn_act_bwd_reduce": (c_int, [P, P, c_int, c_ll, c_int, c_int, P, c_int, P, c_int, P]),
    "s2i_bn_bwd_finalize": (c_int, [P, c_int, c_int, c_int, c_ll, P, P, c_int, P, P]),
    "s2i_bn_act_bwd_apply": (c_int, [P, P, c_int, c_ll, c_int, c_int, P, P, c_int, P, P]),
    "s2i_act_backward": (c_int, [P, P, c_int, c_ll, c_int, c_int, P, P]),
    "s2i_glu_forward": (c_int, [P, c_ll, c_int, P, P]),
    "s2i_glu_backward": (c_int, [P, P, c_ll, c_int, P, P]),
    "s2i_nchw_to_nhwc": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "s2i_nhwc_to_nchw": (c_int, [P, c_int, P, c_int, c_int, c_int, c_int, P]),
    "s2i_image_to_u8": (c_int, [P, c_int, P, c_ll, P]),
    "s2i_u8_to_image": (c_int, [P, P, c_int, c_int, c_int, P]),
    "s2i_image_batch": (c_int, [P, c_ll, P, P, c_int, P, c_int, c_int, c_int, P, P, P, P, P, P]),
    "s2i_image_grid_workspace_bytes": (c_size_t, []),
    "s2i_image_grid_u8": (c_int, [P, c_int, c_int, c_int, c_ll, c_ll, c_ll, c_ll, c_int, c_int, P, P, P]),
    "s2i_spatial_sum": (c_int, [P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    "s2i_spatial_sum_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "s2i_diffaug_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "s2i_diffaug_forward": (c_int, [P, P, c_int, P, c_int, c_int, c_int, P, c_size_t, P]),
    "s2i_diffaug_backward": (c_int, [c_int, P, c_int, P, c_int, P, c_int, c_int, c_int, P, c_size_t, P]),
    "s2i_specaug_workspace_bytes": (c_size_t, [c_int]),
    "s2i_specaug": (c_int, [P, P, c_int, c_int, P, c_int, c_int, c_int, c_int, c_float, ctypes.c_ulonglong,
                            ctypes.c_ulonglong, P, c_size_t, P]),
    "s2i_wave_mix_workspace_bytes": (c_size_t, [c_int, c_int]),
    "s2i_wave_mix": (c_int, [P, P, P, c_int, c_int, P, P, ctypes.c_ulonglong, ctypes.c_ulonglong, P, c_size_t, P]),
    "s2i_reverb_rir": (c_int, [P, c_int, c_int, P, ctypes.c_ulonglong, ctypes.c_ulonglong, P]),
    "s2i_reverb": (c_int, [P, P, P, c_int, c_int, P, P, c_int, P, P]),
    "s2i_stretch_basis_elems": (c_size_t, []),
    "s2i_time_stretch_workspace_bytes": (c_size_t, [c_int, c_ll, c_ll]),
    "s2i_time_stretch": (c_int, [P, P, P, c_int, c_int, P, P, P, P, c_int, c_ll, c_ll, P, c_size_t, P]),
    "s2i_reparam_forward": (c_int, [P, P, c_int, c_int, P, P]),
    "s2i_reparam_backward": (c_int, [P, P, P, P, P, c_int, c_int, P, P]),
    "s2i_kl_forward": (c_int, [P, c_int, P, c_int, c_int, c_int, P, P]),
    "s2i_kl_backward": (c_int, [P, c_int, P, c_int, c_int, c_int, P, P, P, P]),
    "s2i_logit_forward": (c_int, [P, P, P, c_int, c_int, P, P]),
    "s2i_logit_backward": (c_int, [P, P, P, P, c_int, c_int, P, c_int, P, P, c_int, P]),
    "s2i_bce_forward": (c_int, [P, c_float, c_int, c_float, P, c_int, P]),
    "s2i_bce_backward": (c_int, [P, c_float, c_int, c_float, P, P, P]),
    "s2i_bce_multi_forward": (c_int, [P, P, P, c_int, c_int, c_int, P, P]),
    "s2i_bce_multi_backward": (c_int, [P, P, P, c_int, c_int, c_int, P, P, P]),
    "s2i_cal_loss": (c_int, [P, P, c_int, c_int, P, c_int, P, P]),
    "s2i_maxpool_w3s2": (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    "s2i_lstm_cell": (c_int, [P, c_int, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int, P]),
    "s2i_lstm_step": (c_int, [P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, c_int, P]),
    "s2i_time_mean": (c_int, [P, c_int, c_int, c_int, P, P]),
    "s2i_lstm_train_step": (c_int, [P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, c_int, P, P, P, P]),
    "s2i_lstm_train_cell": (c_int, [P, c_int, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int, P, P, P, P]),
    "s2i_lstm_bwd_step": (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P]),
    "s2i_lstm_bwd_cell": (c_int, [P, P, c_int, P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P]),
    "s2i_lstm_bias_grad": (c_int, [P, c_ll, c_int, P, P]),
    "s2i_encoder_loss_workspace_bytes": (c_size_t, [c_int]),
    "s2i_encoder_loss": (c_int, [P, P, P, c_int, c_int, c_float, c_float, c_int, c_float, c_float, c_float, P, c_size_t, P,
                                 P, P]),
    "s2i_conv1d_dgrad": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "s2i_conv1d_wgrad_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "s2i_conv1d_wgrad": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    "s2i_bn_relu_forward": (c_int, [P, c_ll, c_int, P, P, P]),
    "s2i_bn_relu_bwd_reduce": (c_int, [P, P, P, c_ll, c_int, P, P, c_int, P]),
    "s2i_bn_relu_bwd_apply": (c_int, [P, P, P, c_ll, c_int, P, P, P, P]),
    "s2i_maxpool_w3s2_backward": (c_int, [P, P, c_int, c_int, c_int, c_int, P, P]),
    "s2i_bn1_stats": (c_int, [P, c_ll, P, c_int, P]),
    "s2i_bn1_finalize": (c_int, [P, c_int, c_ll, P, P, P, P, P, c_float, c_float, P, P]),
    "s2i_bn1_bwd_reduce": (c_int, [P, P, c_ll, P, P, c_int, P]),
    "s2i_bn1_bwd_finalize": (c_int, [P, c_int, c_ll, P, P, P, P]),
    "s2i_adam_step": (c_int, [P, P, P, P, c_ll, c_float, c_float, c_float, c_float, c_int, P, c_float, P]),
    "s2i_adam_l2_step": (c_int, [P, P, P, P, c_ll, c_float, c_float, c_float, c_float, c_float, c_int, P, c_float, P]),
    "s2i_increment": (c_int, [P, P]),
    "s2i_grad_sumsq": (c_int, [P, c_ll, P, P, P, c_int, c_ll, P, P]),
    "s2i_grad_clip_scale": (c_int, [P, P, c_int, ctypes.c_double, ctypes.c_double, P, P, P, P, P]),
    "s2i_adam_step_dev": (c_int, [P, P, P, P, c_ll, c_float, c_float, c_float, c_float, P, P, P, P]),
    "s2i_adam_l2_step_dev": (c_int, [P, P, P, P, c_ll, c_float, c_float, c_float, c_float, c_float, P, P, P, P]),
    "s2i_ema_update": (c_int, [P, P, c_ll, c_float, P]),
    "s2i_scale_dev": (c_int, [P, P, c_ll, P, P]),
    "s2i_axpby": (c_int, [P, P, c_ll, c_float, c_float, P]),
    "s2i_plan_create": (c_int, [P, ctypes.POINTER(P), ctypes.POINTER(c_int)]),
    "s2i_plan_replay": (c_int, [P, P]),
    "s2i_plan_destroy": (c_int, [P]),
    "s2i_conv2d_plan": (c_int, [ctypes.POINTER(Conv2dDesc)]),
    "s2i_conv2d_weight_elems": (c_size_t, [ctypes.POINTER(Conv2dDesc)]),
    "s2i_conv2d_forward": (c_int, [ctypes.POINTER(Conv2dDesc), P, P, P, P, P]),
    "s2i_pool2d": (c_int, [c_int, P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, P]),
    "s2i_inception_prep": (c_int, [P, c_int, c_int, c_int, c_ll, c_ll, c_ll, c_ll, P, c_int, c_int, P]),
    "s2i_softmax_rows": (c_int, [P, c_int, c_int, c_int, P, c_int, P]),
    "s2i_googlenet_prep": (c_int, [P, c_ll, P, P, P, c_int, c_float, c_float, c_float, P, P]),
    "s2i_maxpool3": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, P]),
    "s2i_lrn_maxpool3": (c_int, [c_int, P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int, c_float, c_float,
                                 c_float, P]),
    "s2i_logmel_basis_elems": (c_size_t, []),
    "s2i_signal_mean": (c_int, [P, P, P, c_int, P, P, P]),
    "s2i_logmel_power": (c_int, [P, P, P, c_int, P, P, P, P, P, c_int, c_int, P, P, P]),
    "s2i_logmel_finish": (c_int, [P, P, P, c_int, c_int, c_int, P, P]),
    "s2i_logmel_gather": (c_int, [P, P, P, c_int, c_int, P, P]),
    "s2i_pcm_resample": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P, P, P]),
    "s2i_moments_accumulate": (c_int, [P, c_int, c_int, c_ll, P, P, P]),
    "s2i_topk_rows": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P]),
    "s2i_rank_rows": (c_int, [P, c_int, c_int, c_int, c_int, P, P, P, c_int, P, P, P, c_int, P]),
    "s2i_polykernel_rows": (c_int, [P, c_int, c_int, c_int, c_int, c_int, ctypes.c_double, P, P]),
    "s2i_sqdist_rows": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P]),
    "s2i_ball_rows": (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, P, P, P]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_device_checked = False


class S2IError(RuntimeError):
    pass


def load():
    """Load libs2i_hip.so (once) and declare every entry point of include/s2i_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise S2IError(
            "libs2i_hip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C %s/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback."
            % (LIB_PATH, _HERE))
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.s2i_version() != ABI_VERSION:
        raise S2IError("libs2i_hip.so ABI version %d, expected %d: rebuild it (make -C csrc)" % (lib.s2i_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().s2i_last_error()
        raise S2IError("%s failed: %s" % (what, msg.decode() if msg else "unknown error"))


class tuning:
    """`with tuning(fwd_bm=96): ...` sets integer knobs of the launch planners (s2i_set_tuning) for the body and restores
    them: tools and tests use it to force a kernel variant; nothing on a launch path reads the environment."""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        lib = load()
        self.old = {}
        for k, v in self.knobs.items():
            cur = c_int(0)
            check(lib.s2i_get_tuning(k.encode(), ctypes.byref(cur)), "s2i_get_tuning")
            self.old[k] = cur.value
            check(lib.s2i_set_tuning(k.encode(), int(v)), "s2i_set_tuning")
        return self

    def __exit__(self, *exc):
        lib = load()
        for k, v in self.old.items():
            check(lib.s2i_set_tuning(k.encode(), v), "s2i_set_tuning")
        return False


def wgrad_plan(d, a_dtype=DT_F32, g_dtype=DT_F32, planes=0, in_act=0):
    """What the weight gradient of WgradDesc d launches in this operand mode (s2i_wgrad_plan_query, host only): a dict of
    WGRAD_PLAN_FIELDS with the kernel as its WGRAD_KERNELS name, or None where the plan refuses (s2i_last_error says why)."""
    out = (c_int * 12)()
    if load().s2i_wgrad_plan_query(ctypes.byref(d), a_dtype, g_dtype, planes, in_act, ctypes.byref(out)):
        return None
    plan = dict(zip(WGRAD_PLAN_FIELDS, out))
    plan["kernel"] = WGRAD_KERNELS[plan["kernel"]]
    return plan


def conv_plan(d, x_dtype=DT_F32, y_dtype=DT_F32, planes=0, bias=False, cls_bias=False):
    """What the forward convolution of ConvDesc d launches with these operands (s2i_conv_plan_query, host only; d.in_act
    says apply-on-load): a dict of FWD_PLAN_FIELDS with the kernel as its FWD_KERNELS name, or None where the plan refuses
    (s2i_last_error says why)."""
    out = (c_int * 15)()
    if load().s2i_conv_plan_query(ctypes.byref(d), x_dtype, y_dtype, planes, int(bool(bias)), int(bool(cls_bias)), ctypes.byref(out)):
        return None
    plan = dict(zip(FWD_PLAN_FIELDS, out))
    plan["kernel"] = FWD_KERNELS[plan["kernel"]]
    return plan


def conv_bf16_plan(d):
    """What s2i_conv_forward_bf16 launches for ConvDesc d (s2i_conv_bf16_plan_query, host only): a dict of B16_PLAN_FIELDS
    with the kernel as its B16_KERNELS name, None for a tile the kernel is not instantiated for (the layer is not eligible);
    or None where the plan refuses the descriptor (s2i_last_error says why).  The weight layout key is ck | npad << 8."""
    out = (c_ll * 21)()
    if load().s2i_conv_bf16_plan_query(ctypes.byref(d), ctypes.byref(out)):
        return None
    plan = dict(zip(B16_PLAN_FIELDS, out))
    plan["kernel"] = B16_KERNELS[plan["kernel"]] if plan["kernel"] >= 0 else None
    return plan


def require_device():
    """Raise unless the current device is a gfx950 GPU the kernels were compiled for."""
    global _device_checked
    if _device_checked:
        return
    if not torch.cuda.is_available():
        raise S2IError("no HIP device visible: the MI355X kernels have no CPU fallback")
    check(load().s2i_check_device(), "s2i_check_device")
    _device_checked = True


def ptr(t):
    """Device pointer of a contiguous fp32/int32 CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise S2IError("tensor is not on a HIP device; the MI355X path has no CPU fallback")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_dev = torch.cuda.current_device


def stream():
    """Raw hipStream_t of torch's current stream.  `torch.cuda.current_stream().cuda_stream` builds a Stream object per
    call (8 us; 1 600 calls per train step = 2.6 ms of host time, tools/host_profile.py); the raw query is ~0.3 us."""
    if _raw_stream is not None:
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream
