"""ctypes binding of libmmtpsm.so (include/mmtpsm.h) -- the ONLY compute backend of this package.

There is no CPU or eager-PyTorch fallback: if the shared library is missing, or a tensor that reaches
an op is not a CUDA/HIP tensor, the call raises.  PyTorch is used for device memory, streams and
autograd bookkeeping only; tensors cross the boundary as raw device pointers.
"""
import ctypes
import gc as _gc
import math
import weakref
import os
import threading as _threading
from collections import namedtuple as _namedtuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libmmtpsm.so")

c_void_p, c_int, c_float, c_double, c_int64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int64


class Pyramid(ctypes.Structure):
    _fields_ = [("feat", c_void_p * 4), ("grad_feat", c_void_p * 4), ("H", c_int * 4), ("W", c_int * 4),
                ("scale", c_float * 4), ("num_levels", c_int), ("N", c_int), ("C", c_int)]


class RoiMaps(ctypes.Structure):   # include/mmtpsm.h: mmt_roi_maps
    _fields_ = [("feat", c_void_p * 4), ("grad_feat", c_void_p * 4), ("H", c_int * 4), ("W", c_int * 4), ("C", c_int * 4),
                ("c_off", c_int * 4), ("scale", c_float * 4), ("num_maps", c_int), ("N", c_int), ("out_C", c_int)]


class ConvArgs(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("scale", c_void_p), ("shift", c_void_p), ("res", c_void_p),
                ("mask", c_void_p), ("mul", c_void_p), ("y", c_void_p),
                ("N", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int), ("Cout", c_int), ("KH", c_int),
                ("KW", c_int), ("stride", c_int), ("pad", c_int), ("Ho", c_int), ("Wo", c_int),
                ("relu", c_int), ("res_mode", c_int), ("out_stride", c_int), ("out_H", c_int), ("out_W", c_int),
                ("mask_scale", c_float), ("w_planes", c_void_p), ("w_plane_stride", ctypes.c_long),
                ("x_planes", c_void_p), ("x_plane_stride", ctypes.c_long),
                ("y_planes", c_void_p), ("y_plane_stride", ctypes.c_long), ("io_bf16", c_int), ("y_amax", c_void_p),
                ("f16_x_amax", c_void_p), ("f16_dy_amax", c_void_p), ("y_amax_stats", c_int),
                ("f16_guard_x", c_void_p), ("f16_guard_dy", c_void_p), ("w_src", c_void_p), ("w_src_scale", c_void_p),
                ("x_planes_layout", c_int),
                ("y_rb", c_void_p), ("y_rb_stride", ctypes.c_long), ("y_rb_scale", c_void_p), ("y_amax_next", c_void_p),
                ("x_planes_lag", c_int), ("y_rb_rows", c_int)]


IO_X, IO_Y, IO_RES, IO_MASK, IO_DY = 1, 2, 4, 8, 16  # include/mmtpsm.h: mmt_conv_args.io_bf16


class ConvRoute(ctypes.Structure):   # include/mmtpsm.h: mmt_conv_route_t
    _fields_ = [(n, c_int) for n in ("family", "tag", "bm", "bn", "kgroups", "panels", "ksplit", "strip_tw", "strip_ksplit", "strip_korder",
                                     "pg_rows", "pg_ksplit", "wanted", "x_form", "writes_rb", "switches")]


ENTRY_LIB, ENTRY_F16 = 0, 1                                                        # mmt_conv_route: entry
ASSUME_X, ASSUME_W, ASSUME_W_PLANES, ASSUME_X_PLANES, ASSUME_F16_SCALARS = 1, 2, 4, 8, 16   # ... assume
ROUTE_NONE, ROUTE_STRIP, ROUTE_PG = 0, 6, 7                                        # ... family (the ones the host side tells apart)


class WgradRoute(ctypes.Structure):   # include/mmtpsm.h: mmt_conv_wgrad_route_t
    _fields_ = ([(n, c_int) for n in ("family", "terms", "decode", "vec4", "bf", "splits", "mps")] + [("ws_floats", ctypes.c_long)] +
                [(n, c_int) for n in ("lds_bytes", "dbias_in_kernel", "group_kind", "group_splits", "group_mps", "switches")])


WG_HAVE_MAXIMA, WG_HAVE_PLANES = 1, 2                  # mmt_conv_wgrad_route: have
WGRAD_NONE, WGRAD_PLANES_1, WGRAD_PLANES_3 = 0, 6, 7   # ... family (the ones the host side tells apart)


class WgradJob(ctypes.Structure):   # include/mmtpsm.h: mmt_wgrad_job
    _fields_ = [("a", ConvArgs), ("dy", c_void_p), ("rowscale", c_void_p), ("dw", c_void_p), ("dbias", c_void_p),
                ("x_planes", c_void_p), ("x_plane_stride", ctypes.c_long), ("dy_planes", c_void_p), ("dy_plane_stride", ctypes.c_long),
                ("s_x", c_void_p), ("s_dy", c_void_p)]


class RpnLevel(ctypes.Structure):
    _fields_ = [("head", c_void_p), ("anchors", c_void_p), ("topk", c_void_p), ("HW", c_int), ("k", c_int),
                ("out_off", c_int), ("pad", c_int)]


class RpnTopkLevel(ctypes.Structure):
    _fields_ = [("head", c_void_p), ("topk", c_void_p), ("HW", c_int), ("k", c_int)]


class RpnSelectArgs(ctypes.Structure):
    _fields_ = [("lv", RpnLevel * 8), ("L", c_int), ("N", c_int), ("A", c_int), ("C", c_int), ("sumk", c_int),
                ("clipv", c_float), ("lim", c_void_p), ("boxes", c_void_p), ("scores", c_void_p), ("idx", c_void_p),
                ("box_reg", c_void_p)]


class RpnPostArgs(ctypes.Structure):
    _fields_ = [("boxes", c_void_p), ("scores", c_void_p), ("idx", c_void_p), ("box_reg", c_void_p), ("keep", c_void_p),
                ("keep_cnt", c_void_p), ("seg_off", c_int * 9), ("own_pre", c_int * 8), ("L", c_int), ("N", c_int),
                ("sumk", c_int), ("kmax", c_int), ("post_n", c_int), ("fpn_post_n", c_int), ("training", c_int),
                ("cap", c_int), ("min_size_filter", c_int), ("pad", c_int), ("gt", c_void_p), ("gt_off", c_void_p),
                ("out_boxes", c_void_p), ("out_scores", c_void_p),
                ("out_idx", c_void_p), ("out_reg", c_void_p), ("out_level", c_void_p), ("out_cnt", c_void_p),
                ("key_scratch", c_void_p)]


class MgdTeachers(ctypes.Structure):
    _fields_ = [("t", c_void_p * 8), ("flip", c_int * 8), ("nt", c_int)]


class MgdStudents(ctypes.Structure):
    _fields_ = [("s", c_void_p * 4), ("mirror", c_int * 4), ("ns", c_int)]


_SIGS = {
    "mmt_version": [],
    "mmt_roi_align_forward": [ctypes.POINTER(Pyramid), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_roi_align_forward_bf16": [ctypes.POINTER(Pyramid), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_roi_align_backward": [ctypes.POINTER(Pyramid), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_roi_align_backward_dense": [ctypes.POINTER(Pyramid), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_roi_align_maps_forward": [ctypes.POINTER(RoiMaps), c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_roi_align_maps_backward": [ctypes.POINTER(RoiMaps), c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_nms_batched": [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_soft_nms_batched": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p,
                             c_void_p],
    "mmt_resample_u8": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p],
    "mmt_aug_views": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(c_float),
                      c_void_p, ctypes.c_long, c_int, c_int, c_void_p],
    "mmt_aug_erase": [c_void_p, ctypes.c_long, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(c_float),
                      c_void_p],
    "mmt_roi_format_levels": [c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_relation_reg_labels": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_float), c_int, c_void_p, c_void_p],
    "mmt_match_targets": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                          c_float, c_int, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p],
    "mmt_conv_forward": [ctypes.POINTER(ConvArgs), c_void_p],
    "mmt_conv_route": [ctypes.POINTER(ConvArgs), c_int, c_int, c_void_p],
    "mmt_conv_switches": [],
    "mmt_set_conv_precision": [ctypes.c_int],
    "mmt_get_conv_precision": [],
    "mmt_pack_weight": [c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_void_p],
    "mmt_rpn_topk": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_rpn_gather_decode": [ctypes.POINTER(RpnSelectArgs), c_void_p],
    "mmt_rpn_post_select": [ctypes.POINTER(RpnPostArgs), c_void_p],
    "mmt_sample_fg_bg": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_box_decode": [c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_int,
                       c_void_p, c_void_p],
    "mmt_split_planes": [c_void_p, c_void_p, ctypes.c_long, ctypes.c_long, c_void_p],
    "mmt_pack_weights": [c_void_p, c_void_p, ctypes.c_long, c_void_p, c_void_p, c_int, c_void_p],
    "mmt_pack_weights_flipped": [c_void_p, c_void_p, c_int, c_void_p],
    "mmt_pack_weights_f16": [c_void_p, c_void_p, ctypes.c_long, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
    "mmt_pack_weights_flipped_f16": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
    "mmt_pack_weight_flipped": [c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_conv_wgrad_route": [ctypes.POINTER(ConvArgs), c_int, ctypes.POINTER(WgradRoute)],
    "mmt_conv_wgrad": [ctypes.POINTER(ConvArgs), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_colsum": [c_void_p, c_int, c_int, c_void_p, c_void_p],
    "mmt_weight_flip_transpose": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_maxpool3x3s2": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_amax": [c_void_p, ctypes.c_long, c_void_p, ctypes.c_long, c_int, c_void_p, c_void_p],
    "mmt_amax_stats": [c_void_p, ctypes.c_long, c_void_p, c_void_p],
    "mmt_det_postprocess": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_int, c_void_p,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_det_postprocess_soft": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_float, c_float,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_position_embedding": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_sample_fg_bg_wide": [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p],
    "mmt_rpn_loss": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_long, c_float, c_void_p, c_void_p, c_void_p,
                     c_void_p, c_void_p],
    "mmt_box_loss": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_box_loss_rows": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_relation_attention_fwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                   c_void_p, c_void_p, c_void_p],
    "mmt_relation_attention_bwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_ciam_fwd": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_ciam_bwd": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                     c_void_p, c_void_p, c_void_p],
    "mmt_stats_combine": [c_void_p, c_int, c_void_p, c_void_p],
    "mmt_sum_stats": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_long, c_void_p, c_void_p],
    "mmt_split_planes_f16": [c_void_p, c_void_p, ctypes.c_long, ctypes.c_long, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_split_planes_f16_rb": [c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_replay": [c_void_p, c_int, c_void_p],
    "mmt_conv_wgrad_group_workspace": [c_void_p, c_int, ctypes.POINTER(ctypes.c_long)],
    "mmt_conv_wgrad_group": [c_void_p, c_int, c_void_p, ctypes.c_long, c_void_p],
    "mmt_sum_stats_rb": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.c_long, c_void_p,
                         c_void_p, c_void_p],
    "mmt_rb_scales_update": [c_void_p, c_int, c_void_p],
    "mmt_conv_wgrad_planes": [ctypes.POINTER(ConvArgs), c_void_p, c_void_p, ctypes.c_long, c_void_p, ctypes.c_long, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_pack_weight_f16": [c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p],
    "mmt_pack_weight_flipped_f16": [c_void_p, c_void_p, c_void_p, ctypes.c_long, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_conv3x3_strip_f16x2": [ctypes.POINTER(ConvArgs), c_void_p, c_void_p, c_void_p],
    "mmt_conv_forward_f16x2": [ctypes.POINTER(ConvArgs), c_void_p, c_void_p, c_void_p],
    "mmt_conv_forward_pg": [ctypes.POINTER(ConvArgs), c_void_p, c_void_p, c_int, c_int, c_void_p],
    "mmt_stem_fused": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_void_p],
    "mmt_c64_conv3_fused": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, ctypes.c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, ctypes.c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                            c_void_p, c_void_p, c_void_p, ctypes.c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p],
    "mmt_maxpool3x3s2_bf16": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_gconv3x3_forward": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_gconv3x3_dgrad": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_gconv3x3_wgrad": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_maxpool3x3s2_backward": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "mmt_stem_wgrad": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    "mmt_mask_bce": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p],
    "mmt_mgd_level_forward": [c_void_p, ctypes.POINTER(MgdTeachers), c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_mgd_level_backward": [c_void_p, ctypes.POINTER(MgdTeachers), c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_mgd_views_forward": [ctypes.POINTER(MgdStudents), ctypes.POINTER(MgdTeachers), c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                              c_void_p],
    "mmt_mgd_views_backward": [ctypes.POINTER(MgdStudents), ctypes.POINTER(MgdTeachers), c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                               c_void_p, c_void_p],
    "mmt_mask_pool": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_psm_rows": [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_psm_variance": [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_ema_update": [c_void_p, c_void_p, c_int64, c_double, c_void_p],
    "mmt_sgd_momentum": [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_int, c_void_p],
    "mmt_grad_guard": [c_void_p, c_int64, c_void_p, c_void_p, c_float, c_void_p],
    "mmt_sgd_momentum_guarded": [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_int, c_void_p, c_void_p],
    "mmt_paste_masks": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p],
    "mmt_paste_mask_stack": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p],
    "mmt_polygon_targets": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_mask_pack": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_paste_mask_words": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p],
    "mmt_mask_expand": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_mask_transition_counts": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_mask_transition_positions": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_mask_pair_intersections": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_mask_nms_workspace": [c_int, c_void_p],
    "mmt_mask_nms": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p,
                     c_void_p, c_void_p],
    "mmt_polygon_mask_words_workspace": [c_int, c_int, c_int, c_void_p],
    "mmt_polygon_mask_words": [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p,
                               c_void_p],
    "mmt_mask_words_integral": [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p],
    "mmt_mask_words_resample": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                c_void_p],
    "mmt_mask_words_targets": [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p],
    "mmt_set_deterministic": [c_int],
    "mmt_get_deterministic": [],
    "mmt_roi_align_backward_ordered": [ctypes.POINTER(Pyramid), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p],
    "mmt_colsum_ordered": [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_stem_wgrad_ordered": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, ctypes.c_long, c_void_p],
    "mmt_mask_bce_ordered": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_mgd_level_forward_ordered": [c_void_p, ctypes.POINTER(MgdTeachers), c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_mgd_views_forward_ordered": [ctypes.POINTER(MgdStudents), ctypes.POINTER(MgdTeachers), c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                      c_void_p, c_void_p],
    "mmt_box_loss_ordered": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_ciam_bwd_ordered": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_ciam_norm_fwd": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_ciam_norm_bwd": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_void_p, c_void_p],
    "mmt_ciam_norm_bwd_ordered": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p],
    "mmt_tta_merge_box": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "mmt_tta_merge_mask": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
}
# the entry points that return `long` (sizes in floats; include/mmtpsm.h), bound like _SIGS with that result type
_SIGS_LONG = {
    "mmt_stem_wgrad_ws_floats": [c_int, c_int, c_int],
    "mmt_ciam_norm_lds_bytes": [c_int, c_int, c_int],
    "mmt_ciam_norm_saved_floats": [c_int, c_int],
    "mmt_ciam_norm_ws_floats": [c_int, c_int],
}

_lib = None
# bench.py sets this to a list: every launch of the dominant conv kernel (128x128 tiles) is then bracketed by a pair
# of events on the launch stream and recorded as (algorithmic FLOPs, start, stop, shape key).  PROFILE_ALL (tuning
# tool only) extends that to every conv / wgrad launch.
PROFILE = None
PROFILE_ALL = False
# bf16 STORAGE of the ResNet body's activations and activation gradients (BASELINE configs[4] "bf16 MFMA path"): only with
# the bf16 arithmetic (mode 1).  The producers in layers/fused.py ask `bf16_storage()`; every consumer goes by the dtype
# of the tensor it is handed.
_BF16_STORAGE = os.environ.get("MMT_BF16_STORAGE", "0") != "0"


# DEFAULT arithmetic of mode 3 since round 3 (MMT_F16X2=0 / set_f16x2(False) selects the 3-term bf16 split, which is also the
# per-tensor fall-back): convolutions take a TWO-term fp16 split of both operands (3 matrix products per
# multiply instead of 6), each tensor scaled by a power of two derived on the device from its largest magnitude.  Error
# against fp64 no larger than the 3-term bf16 split's (tools/bench_f16x2.py, profiles/r03_precision_f16x2.txt).
F16X2_DEFAULT = os.environ.get("MMT_F16X2", "1") != "0"
F16X2 = F16X2_DEFAULT
F16X2_TILED = True   # (constant, read by bench.py: the tiled kernel -- 1x1, small-map 3x3, fc -- runs on the fp16 split like the strip kernel)
F16_STATS = {"wgrad": 0, "conv": 0, "tiled": 0, "pg": 0, "amax_pass": 0, "fallback": 0, "weight_pack": 0}   # launches that took the fp16 path (tools, tests)
WGRAD_F16_MIN_ELEMS = 1 << 22


def set_f16x2(on):
    """True / False; None restores the process default (MMT_F16X2, on unless set to 0)"""
    global F16X2
    F16X2 = F16X2_DEFAULT if on is None else bool(on)
    _PLAN_EPOCH[0] += 1
    _PLAN.clear()
    LOOSE.forget()
    _F16SITE.clear()
    _SITES.clear()
    rb_reset()


# ---- per-tensor statistics of the fp16 split: every producing launch records max |y| AND sum |y| of its output in a slot of
# a device pool (mmt_conv_args.y_amax / y_amax_stats; tensors that come from elsewhere take one mmt_amax_stats pass).  The
# maximum gives the consumer its power-of-two scale on the device, with no host round trip.  max / mean -- the crest factor
# -- tells whether fp16's 5 exponent bits can hold the tensor at all: when one element is 10^8 x the rest, everything else
# falls below the range of the low term (outputs built only from such values then carry 2e-5 instead of 2e-6 of sum |a||b|,
# profiles/r02_precision_f16x2.txt).  That decision needs the host (it picks the kernel), so it is LAGGED: a full pool is
# copied to pinned memory asynchronously, each consuming site (a weight, forward or data-gradient form) looks at the
# statistics of one of its recent input tensors when they have arrived, and falls back to the 3-term bf16 split -- exact
# for any dynamic range -- from then on, until the crest factor is back below F16_CREST_LO.  No call ever waits.
STAT_W = 40            # floats per slot: [0] max |x|, [1..16] sums of |x| over a sample, [17..32] the sample's counts, padding
_POOL_SLOTS = 2048     # ~6 steps of the detector
F16_CREST_HI, F16_CREST_LO = 2.0 ** 17, 2.0 ** 15


class _StatPool(object):
    __slots__ = ("dev", "host", "event", "next", "gen", "host_gen", "base")
    travels = True   # its statistics reach the host (retire); a pool of slots says so, _site_ok queues a slot only where they do

    def __init__(self, device):
        self.dev = torch.zeros((_POOL_SLOTS, STAT_W), dtype=torch.float32, device=device)
        self.host = torch.zeros((_POOL_SLOTS, STAT_W), dtype=torch.float32).pin_memory()
        self.event, self.next, self.gen, self.host_gen = None, 0, 0, -1
        self.base = self.dev.data_ptr()

    def retire(self):
        """full: its statistics travel to the host (asynchronously, on the stream that filled it)"""
        self.host.copy_(self.dev, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        self.host_gen = self.gen

    def reuse(self):
        if self.event is not None:
            self.event.synchronize()   # two rotations later: long done
        self.dev.zero_()
        self.gen += 1
        self.next = 0


_AMAX_POOL = {}   # (device, stream) -> [ring of 3 pools, index of the current one]
_SITES = {}       # consuming site -> [fp16 split allowed, pending (pool, generation, slot, numel) or None]


class _Slot(object):
    """one zeroed statistics slot of a pool (a _StatPool or a launch plan: `base`, `gen`, `travels`): what a launch is handed as y_amax
    and what `tensor._mmt_amax[0]` holds (anything with a data_ptr() works there: tests attach plain one-element tensors)"""
    __slots__ = ("ptr", "pool", "gen", "idx")

    def __init__(self, pool, idx):
        self.pool, self.gen, self.idx = pool, pool.gen, idx
        self.ptr = pool.base + idx * (4 * STAT_W)

    def data_ptr(self):
        return self.ptr


def _amax_slot(device):
    """-> a zeroed statistics slot of the current pool of this (device, stream)"""
    rec = getattr(_TLS, "rec", None)
    if rec is not None:   # a launch plan is being recorded: a slot of its own block (zeroed before every replay)
        i = rec.slot_next
        if i >= _LP_SLOTS:
            raise RuntimeError("launch plan: statistics slots exhausted")
        rec.slot_next = i + 1
        return _Slot(rec, i)
    key = (device.index, _stream())   # (the device's ordinal: str(device) costs a microsecond per launch)
    ent = _AMAX_POOL.get(key)
    if ent is None:
        ent = _AMAX_POOL[key] = [[_StatPool(device)], 0]
    pool = ent[0][ent[1]]
    if pool.next >= _POOL_SLOTS:
        pool.retire()
        ent[1] = (ent[1] + 1) % 3
        if ent[1] >= len(ent[0]):
            ent[0].append(_StatPool(device))
        pool = ent[0][ent[1]]
        if pool.next:
            pool.reuse()
    i = pool.next
    pool.next = i + 1
    return _Slot(pool, i)


def f16_flush_stats():
    """tests / tools: send the statistics recorded so far to the host now (a pool normally travels when it is full)"""
    torch.cuda.synchronize()
    for ent in _AMAX_POOL.values():
        pool = ent[0][ent[1]]
        if pool.next:
            pool.retire()
            pool.next = _POOL_SLOTS   # nothing more goes into this generation
    torch.cuda.synchronize()


# ---- what a producer leaves on a tensor object (plain attributes; each carries the tensor's version counter at the time and is
# void once the tensor has been modified):
#   _mmt_amax   (statistics slot -- anything with a data_ptr() --, version)           written by _record,        read by _recorded
#   _mmt_rb     _Rb(row-blocked fp16 planes, device view of their scale, version,     written by _rb_attach,     read by _rb_of
#                   "epi" | "split", images covered or None = all)
#   _mmt_planes (bf16 planes of the 3-term split, version)                            written by _planes_attach, read by planes_of
# Nobody else in this module assigns them (drop voids all three).  _stat_ptrs turns a statistics record into the addresses a launch
# is handed, _full_slot tells a pool's slot from a bare maximum, _Rb answers what consumers ask of planes (covers, lagged).
def _record(x, slot):   # attach a statistics slot to x at its current version -> the record
    am = x._mmt_amax = (slot, x._version)
    return am


def _recorded(x):
    """the current (statistics slot, version) of x, or None"""
    am = getattr(x, "_mmt_amax", None)
    return am if am is not None and am[1] == x._version else None


def _full_slot(s):   # a slot of a pool (max, sampled sums and counts), not the bare maximum that tests attach as a one-element tensor?
    return type(s) is _Slot


def _stat_ptrs(am):
    """what a launch needs of a current statistics record -> (the address of the maximum, the address of the full slot for the
    kernels' on-device range test or None when only a maximum was recorded)"""
    return (am[0].ptr, am[0].ptr) if _full_slot(am[0]) else (am[0].data_ptr(), None)


class _Rb(_namedtuple("_Rb", "planes scale version kind images")):
    """kind "epi": written by the epilogue of the launch that produced the tensor, with the site's scale of the step before; "split":
    by a pass over it.  images: planes for the first n images of the batch only"""
    __slots__ = ()

    def covers(self, n=None):   # planes for the first n images (None: for the whole batch)?
        return self.images is None or (n is not None and n <= self.images)

    def lagged(self):   # was the scale fixed before the values existed?  (a consumer's guard then tests it)
        return self.kind == "epi"


def _rb_of(x):
    """the current row-blocked planes record of x, or None"""
    rb = getattr(x, "_mmt_rb", None)
    return rb if rb is not None and rb.version == x._version else None


def _rb_attach(x, planes, scale, kind, images=None):
    x._mmt_rb = tuple.__new__(_Rb, (planes, scale, x._version, kind, images))   # (_Rb(...) without the generated __new__: per launch)


def _planes_attach(x, planes):
    x._mmt_planes = (planes, x._version)


def planes_of(x):
    """the bf16 planes a producing convolution attached to this very tensor object (still valid: not modified since)"""
    t = getattr(x, "_mmt_planes", None)
    return t[0] if t is not None and t[1] == x._version and t[0].shape[1] == x.numel() else None


def carry(src, dst, rb=True, planes=True, images=None):
    """dst holds the same values as src (a view, an alias) or, images=(lo, hi), is that batch slice of it: what the producer of src
    left on it goes along -- the statistics always (a maximum over more elements is an upper bound: all the fp16 split's scale
    needs), the planes unless switched off (a reshaped or subsampled tensor has another plane order)"""
    carry_stats(src, dst)
    if planes:
        pl = planes_of(src)
        if pl is not None:
            if images is not None:
                per = src.numel() // src.shape[0]
                pl = pl[:, images[0] * per:images[1] * per]
            _planes_attach(dst, pl)
    if rb:
        r = _rb_of(src)
        if r is not None:
            if images is None:
                _rb_attach(dst, r.planes, r.scale, r.kind, r.images)
            elif r.covers(images[1]):   # (image-major planes: a batch slice is a slice, also inside planes of the leading images)
                per = src.numel() // src.shape[0]
                _rb_attach(dst, r.planes[:, images[0] * per:images[1] * per], r.scale, r.kind)


def carry_stats(src, dst):
    """the statistics alone: dst is a reshaped view of src, or holds a subset / the window maxima of its non-negative values"""
    am = _recorded(src)
    if am is not None:
        _record(dst, am[0])


def drop(x):
    """x was modified through raw pointers: what its producer recorded about it no longer holds"""
    for a in ("_mmt_amax", "_mmt_rb", "_mmt_planes"):
        if getattr(x, a, None) is not None:
            setattr(x, a, None)


def _site_ok(site, x, count=True):
    """may the consumer `site` take `x` on the two-term fp16 split?  (lagged crest-factor test, see above)"""
    ent = _SITES.get(site)
    if ent is None:
        ent = _SITES[site] = [True, None]
    if _DET:
        # deterministic mode: WHEN a pool's statistics reach the host is a matter of timing, and the answer picks the kernel -- the
        # site keeps the state it has, nothing is polled or queued; the kernels' on-device range guard covers accuracy alone
        if not ent[0] and count:
            F16_STATS["fallback"] = F16_STATS.get("fallback", 0) + 1
        return ent[0]
    pend = ent[1]
    if pend is not None:
        pool, gen = pend.pool, pend.gen
        if pool.host_gen == gen:
            if pool.event.query():
                row = pool.host[pend.idx]
                amax, tot, cnt = float(row[0]), float(row[1:17].sum()), float(row[17:33].sum())
                if tot > 0.0:
                    crest = amax * cnt / tot if amax == amax and amax != float("inf") else float("inf")
                    if crest > F16_CREST_HI:
                        ent[0] = False
                    elif crest < F16_CREST_LO:
                        ent[0] = True
                ent[1] = None
        elif pool.gen > gen + 1:
            ent[1] = None    # overwritten before anybody looked
    if ent[1] is None:
        am = _recorded(x)
        if am is not None and _full_slot(am[0]) and am[0].pool.travels:
            ent[1] = am[0]   # (a launch plan's slots never travel to the host: they would sit here for ever and switch the lagged
                             # test off for the site -- replayed passes rely on the kernels' device-side guard alone)
    if not ent[0] and count:
        F16_STATS["fallback"] = F16_STATS.get("fallback", 0) + 1
    return ent[0]


def _amax_of(x):
    """the recorded (statistics slot, version) of x, taking one reduction pass when nobody recorded it"""
    am = _recorded(x)
    if am is None:
        F16_STATS["amax_pass"] += 1
        if AMAX_LOG is not None:   # tools/f16_stats.py: who needed a reduction pass of its own
            import sys
            f = sys._getframe(1)
            chain = []
            while f is not None and len(chain) < 5:
                chain.append("%s:%d" % (f.f_code.co_name, f.f_lineno))
                f = f.f_back
            AMAX_LOG.append((tuple(x.shape), " < ".join(chain)))
        slot = _amax_slot(x.device)
        _check(lib().mmt_amax_stats(x.data_ptr(), x.numel(), slot.ptr, _stream()), "mmt_amax_stats")
        am = _record(x, slot)
    return am


def stats_of_convex_combination(out, sources):
    """attach to `out` -- a tensor whose elements are convex combinations of elements of `sources` (ROIAlign of pyramid levels) --
    a statistics slot derived from theirs (include/mmtpsm.h: mmt_stats_combine): one 64-thread launch instead of a reduction pass
    over `out`; the (at most 8) slot addresses are kernel arguments.  Nothing happens unless every source carries a recorded slot."""
    slots = []
    for t in sources:
        am = _recorded(t)
        if am is None or not _full_slot(am[0]):
            return
        slots.append(am[0].ptr)
    if not slots or len(slots) > 8:
        return
    arr = (c_void_p * len(slots))(*slots)
    slot = _amax_slot(out.device)
    _check(lib().mmt_stats_combine(arr, len(slots), slot.ptr, _stream()), "mmt_stats_combine")
    _record(out, slot)


def sum_stats(ts, rb_site=None):
    """sum of 2..4 equally shaped dense fp32 tensors (same memory order) in one launch; the statistics of the sum are recorded
    (the consumers of the result then need no reduction pass: fp16-split scale, crest-factor test).  rb_site (round 6): the sum is an
    NHWC activation gradient that a plane-fed data-gradient launch consumes -- the same launch leaves its row-blocked fp16 planes
    (include/mmtpsm.h: mmt_sum_stats_rb; the site's scale as in _rb_produce)"""
    a = ts[0]
    if not (2 <= len(ts) <= 4) or any(t.shape != a.shape or t.stride() != a.stride() or t.dtype != torch.float32 for t in ts):
        raise RuntimeError("sum_stats: 2..4 fp32 tensors of one shape and memory order")
    _dev(a)
    n = a.numel()
    if n == 0 or (n & 3):
        y = ts[0] + ts[1]
        for t in ts[2:]:
            y = y + t
        return y
    y = torch.empty_like(a)
    if y.stride() != a.stride():
        raise RuntimeError("sum_stats: dense tensors only")
    slot = _amax_slot(a.device)
    p = [t.data_ptr() for t in ts] + [None] * (4 - len(ts))
    if (rb_site is not None and RB_EPI and PG_RB and a.dim() == 4 and a.shape[1] % 16 == 0 and n < (1 << 30)
            and a.is_contiguous(memory_format=torch.channels_last)):
        s = _rb_site(rb_site, a.device)
        if s is not None:
            nxt = s.produce()
            N, C, Hh, W = a.shape
            # no scale yet: the sum alone (planes NULL); its maximum becomes the site's first pending maximum
            pl = torch.empty((2, n), dtype=torch.float16, device=a.device) if s.ready else None
            _check(lib().mmt_sum_stats_rb(p[0], p[1], p[2], p[3], y.data_ptr(), N * Hh, W, C, slot.ptr, _p(pl), 0 if pl is None else n,
                                          s.scale, nxt, _stream()), "mmt_sum_stats_rb")
            _record(y, slot)
            if pl is not None:
                _rb_attach(y, pl, s.scale_view, "epi")
            return y
    _check(lib().mmt_sum_stats(p[0], p[1], p[2], p[3], y.data_ptr(), n, slot.ptr, _stream()), "mmt_sum_stats")
    _record(y, slot)
    return y


_F16SITE = {}   # role of a tensor (consumer weight address, flipped) -> [device state (scale, a0, a1, a2), calls so far]


def f16_split(x, site=None):
    """x (dense fp32) -> ((2, numel) fp16 planes of x * s, device tensor holding s at [0]), no host sync.
    Without `site`: one reduction pass for max |x|, one split pass.  With `site` (a key naming the ROLE of x: the weight that
    consumes it): delayed scaling -- call k scales by the maximum of the tensor of call k-1 (slot (k-1) % 3), records its own
    in slot k % 3 and clears slot (k+1) % 3: one pass; the first tensor of a role takes the two-pass route.  A power-of-two
    scale does not change the represented value unless a term leaves the fp16 range: 4x headroom above the previous maximum,
    saturating beyond."""
    n = x.numel()
    xp = torch.empty((2, n), dtype=torch.float16, device=x.device)
    am = _recorded(x)
    if am is None and site is None:
        am = _amax_of(x)   # one reduction pass; other consumers of this tensor (its weight gradient) then need none of their own
    if am is not None:
        # (recorded: the convolution that produced x left max |x| from its epilogue, mmt_conv_args.y_amax) the split pass alone
        st = torch.empty((1,), dtype=torch.float32, device=x.device)
        _check(lib().mmt_split_planes_f16(x.data_ptr(), xp.data_ptr(), xp.stride(0), n, 1.0, _stat_ptrs(am)[0], st.data_ptr(),
                                          None, None, _stream()), "mmt_split_planes_f16")
        return xp, st
    ent = _F16SITE.get(site)
    if ent is None:
        F16_STATS["amax_pass"] += 1
        st = torch.zeros((4,), dtype=torch.float32, device=x.device)
        _check(lib().mmt_amax(x.data_ptr(), n, None, 0, 0, st.data_ptr() + 4, _stream()), "mmt_amax")
        _check(lib().mmt_split_planes_f16(x.data_ptr(), xp.data_ptr(), xp.stride(0), n, 1.0, st.data_ptr() + 4, st.data_ptr(),
                                          None, None, _stream()), "mmt_split_planes_f16")
        _F16SITE[site] = [st, 1]
        return xp, st
    st, k = ent
    base = st.data_ptr() + 4
    _check(lib().mmt_split_planes_f16(x.data_ptr(), xp.data_ptr(), xp.stride(0), n, 1.0, base + 4 * ((k - 1) % 3), st.data_ptr(),
                                      base + 4 * (k % 3), base + 4 * ((k + 1) % 3), _stream()), "mmt_split_planes_f16")
    ent[1] = k + 1
    return xp, st


# weight gradients from the row-blocked planes of both operands.  A test hook (MMT_WGRAD_PLANES=0 at import): off, the planes are not
# OFFERED to the weight gradient's route; whether an offered layer runs plane-fed is the route's answer (mmt_conv_wgrad_route)
WG_PLANES = os.environ.get("MMT_WGRAD_PLANES", "1") != "0"
PG_RB = os.environ.get("MMT_PG_RB", "1") != "0"   # input planes of the plane-fed and tap-strip kernels in the row-blocked order (A/B timing: 0)


# ---- round 6: planes out of the PRODUCERS' epilogues.  A plane-fed consumer (tap-strip kernel, plane-fed GEMM, the
# plane-fed weight gradient) used to run one mmt_split_planes_f16_rb pass over its input first: 92 launches and 6.7 GB of traffic per
# step.  The launch that PRODUCES the tensor now writes the row-blocked planes from its epilogue (mmt_conv_args.y_rb).  The scale it
# needs before the values exist is the producing SITE's: the largest |y| any call of the site recorded during the previous step, with
# 2 x head-room (one device word per site, folded once per step by mmt_rb_scales_update: `rb_scales_update`, called by the trainer
# after the optimiser step).  A consumer tests that scale against the statistics the producer recorded in the SAME launch
# (x_planes_lag: max |x| s inside the fp16 range, sampled mean above the low term's) and computes the launch with exact fp32 products
# when it fails -- so a tensor that outgrows the head-room costs time, never accuracy.  A site's first step (no scale yet) and shapes
# whose producing kernel has no plane store keep the split pass.
RB_EPI = os.environ.get("MMT_RB_EPI", "1") != "0"
_RB_MAX = 2048
_RB = {}            # device ordinal -> _RbTable
_RB_LOCK = _threading.Lock()
_RB_EPOCH = [0]     # bumped when a site becomes ready (launch plans recorded before that are re-recorded)


class _RbTable(object):
    __slots__ = ("state", "base", "sites")

    def __init__(self, device):
        self.state = torch.zeros((_RB_MAX, 2), dtype=torch.float32, device=device)   # [site] = (scale, pending max |y| of this step)
        self.state[:, 0] = 1.0
        # base: what mmt_rb_scales_update folds, with the number of sites; sites: key -> _RbSite, in the order of their rows
        self.base, self.sites = self.state.data_ptr(), {}


# one producing site: its row of the table.  THE place that knows the row's layout (include/mmtpsm.h: mmt_rb_scales_update)
class _RbSite(object):
    __slots__ = ("index", "state", "scale_view", "scale", "pending", "produced", "ready", "ok")

    def __init__(self, table, index):
        self.index = index
        self.state = table.state[index]       # device view of both words: [0] the scale, [1] the pending max |y| of this step
        self.scale_view = self.state[0:1]     # (what the planes records of tensors carry)
        self.scale = table.base + 8 * index   # their addresses, as launches are handed them
        self.pending = self.scale + 4
        # produced: a launch of this step recorded a maximum here; ready: has a scale (from the rb_scales_update after the step that
        # produced here first); ok (_rb_produce): launch shape -> does the kernel it takes write planes?
        self.produced, self.ready, self.ok = False, False, {}

    def produce(self):   # a launch of this step records max |y| here -> the address it records it at
        self.produced = True
        return self.pending


def _rb_site(key, device):
    """-> the _RbSite of the producing site `key` (a weight's address and role), the same object every time; None: table full"""
    t = _RB.get(device.index)
    s = t.sites.get(key) if t is not None else None
    if s is None:
        with _RB_LOCK:   # (asked again under the lock: the teacher's thread creates tables and sites too)
            t = _RB.get(device.index)
            if t is None:
                t = _RB[device.index] = _RbTable(device)
            s = t.sites.get(key)
            if s is None and len(t.sites) < _RB_MAX:
                s = t.sites[key] = _RbSite(t, len(t.sites))
    return s


class RbLead(int):
    """last element of a producing site's key: planes for the first n images of the batch only"""


def _rb_produce(a, y, key):
    """the producing half, called with the launch's argument block filled: the site's pending maximum always (y_amax_next); the planes
    when the site has a scale and the kernel this launch takes writes them -> (planes, scale view, images covered or None) or None.
    key = any hashable tuple naming the site; (..., RbLead(n)): planes for the first n images of the batch only (the teacher's view 0)"""
    if not RB_EPI:
        return None
    images = None
    if type(key[-1]) is RbLead:
        images = int(key[-1]) if 0 < int(key[-1]) < y.shape[0] else None
        key = key[:-1]
    s = _rb_site(key, y.device)
    if s is None:
        return None
    a.y_amax_next = s.produce()
    if not s.ready:
        return None
    okk = (a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.stride, a.res_mode, a.mask is not None)
    ok = s.ok.get(okk)
    if ok is None:
        ok = s.ok[okk] = conv_route(a, ENTRY_F16, ASSUME_F16_SCALARS).writes_rb == 1
    if not ok:
        return None
    n = y.numel() if images is None else (y.numel() // y.shape[0]) * images
    pl = torch.empty((2, n), dtype=torch.float16, device=y.device)
    a.y_rb, a.y_rb_stride, a.y_rb_scale = pl.data_ptr(), n, s.scale
    a.y_rb_rows = 0 if images is None else images * y.shape[2] * y.shape[3]
    return pl, s.scale_view, images


def rb_scales_update():
    """once per step, when every launch of the step has been issued and ordered in front of the current stream: the sites' pending
    maxima become their scales for the next step (include/mmtpsm.h: mmt_rb_scales_update); sites that produced for the first time
    are ready from now on"""
    for t in list(_RB.values()):
        produced = [s for s in list(t.sites.values()) if s.produced]
        if not produced:
            continue
        _check(lib().mmt_rb_scales_update(t.base, len(t.sites), _stream()), "mmt_rb_scales_update")
        if not all(s.ready for s in produced):
            _RB_EPOCH[0] += 1
        for s in produced:
            s.produced, s.ready = False, True


def rb_reset():
    """forget every site (tests; an arithmetic switch)"""
    with _RB_LOCK:
        _RB.clear()
    _RB_EPOCH[0] += 1


def f16_split_pg(x):
    """x (dense NHWC fp32) -> (planes, scale tensor, layout, lag) for the plane-fed kernels: the two fp16 planes of x * s in the
    row-blocked order [N H][C / 16][W][16] (layout 1) -- runs of up to 1 KiB per copy instruction of the kernel instead of 32-byte
    pieces.  Planes the PRODUCER of x wrote from its epilogue are taken as they are (lag 1: their scale was fixed before the tensor
    existed, the consumer's guard tests it); else one mmt_split_planes_f16_rb pass, or, MMT_PG_RB=0, planes indexed like x (layout
    0: f16_split).  The same values either way."""
    if not PG_RB:
        xp, st = f16_split(x)
        return xp, st, 0, 0
    rb = _rb_of(x)
    if rb is not None and rb.lagged() and rb.covers(x.shape[0]):
        F16_STATS["rb_epi"] = F16_STATS.get("rb_epi", 0) + 1
        return rb.planes, rb.scale, 1, 1
    F16_STATS["rb_split"] = F16_STATS.get("rb_split", 0) + 1
    # (no reuse of planes an earlier consumer left on the tensor: a launch plan's replay rewrites its result tensors in place without
    # touching their version counters -- the teacher's pyramid levels -- and planes made from the previous step's values would pass)
    N, C, Hh, W = x.shape
    if x.numel() >= (1 << 30) or C % 16:
        # (beyond the row-blocked pass's 32-bit offsets -- planes indexed like x, which the kernels take as layout 0)
        xp, st = f16_split(x)
        return xp, st, 0, 0
    amax = _stat_ptrs(_amax_of(x))[0]
    xp = torch.empty((2, x.numel()), dtype=torch.float16, device=x.device)
    st = torch.empty((1,), dtype=torch.float32, device=x.device)
    _check(lib().mmt_split_planes_f16_rb(x.data_ptr(), xp.data_ptr(), xp.stride(0), N * Hh, W, C, amax, st.data_ptr(), _stream()),
           "mmt_split_planes_f16_rb")
    # the planes stay with the tensor: the weight gradient of the same layer takes BOTH operands from planes (conv_wgrad: the input's
    # from the forward launch, the gradient's from the data-gradient launch) -- alive as long as the tensor is.  (ADVICE r5 asked to
    # keep them only where a weight gradient can follow; a backward pass runs with autograd's grad mode OFF like the teacher's forward,
    # so that test would drop the gradients' planes too -- the RPN head's weight gradients would fall back to the slower kernel.  Since
    # round 6 few tensors are split here at all: 10 per step, 0.57 GB)
    _rb_attach(x, xp, st, "split")
    return xp, st, 1, 0


def _pack_f16(w, scale, flipped, pl, am):
    """the per-call pack of one weight's fp16 form: reduction launch (am[0] = max |w scale|) + packing launch (am[1] = scale word)"""
    Cout, Cin, KH, KW = w.shape
    F16_STATS["weight_pack"] = F16_STATS.get("weight_pack", 0) + 1
    _check(lib().mmt_amax(w.data_ptr(), w.numel(), _p(scale) if flipped else None, Cin * KH * KW, Cout, am.data_ptr(), _stream()), "mmt_amax")
    if flipped:
        _check(lib().mmt_pack_weight_flipped_f16(w.data_ptr(), _p(scale), pl.data_ptr(), pl.stride(0), Cout, KH, KW, Cin,
                                                 am.data_ptr(), am.data_ptr() + 4, _stream()), "mmt_pack_weight_flipped_f16")
    else:
        _check(lib().mmt_pack_weight_f16(w.data_ptr(), pl.data_ptr(), pl.stride(0), Cout, Cin * KH * KW, 1.0, am.data_ptr(),
                                         am.data_ptr() + 4, _stream()), "mmt_pack_weight_f16")


def f16_weight_planes(w, flip_scale=None, flipped=False):
    """packed fp16 planes + a one-element device view holding their scale, of a forward weight or of its data-gradient form
    (taps flipped, transposed, rows scaled by flip_scale).  Parameters of a flattened model (engine/flat.py) are packed in
    bulk after every SGD / EMA step (raw-pointer updates that no version counter sees) and only looked up here; anything else
    is packed per call and kept until the tensor (or the scale vector) is modified."""
    form = "f16_dgrad" if flipped else "f16"
    flat, hit = _flat_form(w, form, flip_scale)
    if hit is not None:
        return hit
    stamp = _loose_stamp(w, flip_scale, w)
    hit = LOOSE.get(w, form, stamp, flip_scale)
    if hit is not None:
        return hit
    Cout, Cin, KH, KW = w.shape
    am = torch.zeros((2,), dtype=torch.float32, device=w.device)
    pl = torch.empty((2, packed_elems(Cin, KH * KW * Cout) if flipped else packed_elems(Cout, Cin * KH * KW)), dtype=torch.float16,
                     device=w.device)
    _pack_f16(w, flip_scale, flipped, pl, am)
    if flipped and flat is not None and flat.register(form, w, flip_scale, pl, am):
        return pl, am[1:2]   # (served by the buffer from now on)
    return LOOSE.put(w, form, stamp, flip_scale, (pl, am[1:2]), w, am)


def set_bf16_storage(on):
    global _BF16_STORAGE
    if on and _DET:
        raise NotImplementedError("bf16 activation storage is not offered in deterministic mode (its kernels' summation orders were "
                                  "never examined): set_deterministic(False)")
    _BF16_STORAGE = bool(on)


def bf16_storage():
    return _BF16_STORAGE and get_conv_precision() == 1


# ---- deterministic mode (include/mmtpsm.h: mmt_set_deterministic).  Process-wide and opt-in: with it, the same seed,
# build, weights and batches give bit-identical training state run to run on one device.  Every sum whose order the default kernels
# leave to timing goes through a fixed-order form (ROIAlign backward, bias gradients, loss scalars, CIAM's gamma, the stem's weight
# gradient), the lagged host-side site test is frozen, torch's own deterministic algorithms are switched on, and what has no ordered
# form yet refuses (the grouped 3x3 weight gradient of ResNeXt, the CSPN mask head's multi-map ROIAlign backward; bf16 activation
# storage).  Off: nothing here is consulted beyond one boolean per call.
_DET = os.environ.get("MMT_DETERMINISTIC", "0") != "0"
_DET_TORCH = None   # torch's switches as set_deterministic(True) found them: (deterministic algorithms, warn only, fill uninitialised memory)
COLSUM_MAX_BLOCKS, MASK_BCE_WS, MGD_MAX_BLOCKS, RPN_LOSS_MAX_BLOCKS, BOX_LOSS_MAX_BLOCKS = 256, 2048, 4096, 1024, 256   # include/mmtpsm.h


def _det_torch(on):
    global _DET_TORCH
    from torch.utils import deterministic as td
    if on:
        if _DET_TORCH is None:
            _DET_TORCH = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                          td.fill_uninitialized_memory)
        torch.use_deterministic_algorithms(True)
        # (every buffer handed to a kernel here is fully written by it; filling each torch.empty first would add a launch per call)
        td.fill_uninitialized_memory = False
    elif _DET_TORCH is not None:
        torch.use_deterministic_algorithms(_DET_TORCH[0], warn_only=_DET_TORCH[1])
        td.fill_uninitialized_memory = _DET_TORCH[2]
        _DET_TORCH = None


def set_deterministic(on):
    """True: deterministic mode (also torch.use_deterministic_algorithms(True)); False: the default kernels, and torch's switches back
    to what set_deterministic(True) found.  MMT_DETERMINISTIC=1 in the environment switches it on at import."""
    global _DET
    on = bool(on)
    if on and _BF16_STORAGE:
        raise NotImplementedError("deterministic mode is not offered with bf16 activation storage (its kernels' summation orders were "
                                  "never examined): set_bf16_storage(False)")
    _det_torch(on)
    _DET = on
    if _lib is not None or os.path.exists(LIB_PATH):
        if lib().mmt_set_deterministic(1 if on else 0) != 0:   # (a switch, not work: not counted among the launches)
            raise RuntimeError("mmt_set_deterministic failed")


def get_deterministic():
    return _DET


def reset_adaptive_state():
    """forget what earlier launches taught the host side about tensors' ranges -- the sites' fp16 / bf16 states, the delayed scales of
    f16_split, the producers' plane scales: the state a fresh process starts from (MTtrainer calls this when it is built in
    deterministic mode, so that a second trainer of a process repeats the first, after a checkpoint is written in that mode and when a
    run is resumed: a checkpoint is a restart point).  rb_reset moves _RB_EPOCH, which is part of a launch plan's key:
    no plan recorded before, with a site's scale address in it, is replayed afterwards"""
    _F16SITE.clear()
    _SITES.clear()
    rb_reset()


if _DET:
    if _BF16_STORAGE:
        raise NotImplementedError("MMT_DETERMINISTIC=1 with MMT_BF16_STORAGE=1: deterministic mode is not offered with bf16 activation storage")
    _det_torch(True)


def _refuse_unordered(kernel, what):
    if _DET:
        raise NotImplementedError("%s is not offered in deterministic mode: %s adds into its destination with float atomics and has "
                                  "no ordered form yet; set_deterministic(False)" % (what, kernel))


def lib():
    """Loads libmmtpsm.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmmtpsm.so not found at %s: build it with `make -C mmt-psm_amd/csrc` "
                "(or python -c 'import __graft_entry__ as g; g.build()'); there is no fallback path" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, args in _SIGS.items():
            f = getattr(L, name)
            f.restype = c_int
            f.argtypes = args
        for name, args in _SIGS_LONG.items():
            f = getattr(L, name)
            f.restype = ctypes.c_long
            f.argtypes = args
        if _DET:
            L.mmt_set_deterministic(1)
        _lib = _LibProxy(L)
    return _lib


def _lib_raw():
    """the CDLL itself (calls through it are never recorded by a launch plan)"""
    return lib()._L


# ---- launch plans (round 5).  The step is bound by the interpreter time of its two launch-issuing threads under one GIL (DESIGN.md
# section 5: the student's head phases are host-bound while the teacher thread issues its backbone).  A no-grad backbone pass over a
# batch of a fixed shape issues the SAME launches every step -- same kernels, same weight / plane / workspace addresses, outputs of
# the same sizes --, so the pass is RECORDED once (every C-ABI call with its arguments; its tensors allocated from a private memory
# pool, which keeps their addresses for the plan's life; its statistics slots from a block of the plan's own) and REPLAYED from then
# on: ~70 ctypes calls instead of the Python that derives them (a manual graph: hipGraph replays of the two models serialise in
# this runtime).  Only the input's address is patched.  Queries are not recorded.
_NO_RECORD = frozenset(("mmt_polygon_mask_words_workspace", "mmt_mask_nms_workspace", "mmt_conv_route", "mmt_conv_switches", "mmt_conv_wgrad_group_workspace",
                        "mmt_conv_wgrad_route", "mmt_get_conv_precision", "mmt_packed_weight_elems", "mmt_set_conv_precision", "mmt_set_deterministic", "mmt_get_deterministic",
                        "mmt_stem_wgrad_ws_floats", "mmt_ciam_norm_lds_bytes", "mmt_ciam_norm_saved_floats", "mmt_ciam_norm_ws_floats"))
LAYOUT_EPOCH = [0]    # bumped when a flat model (re)allocates its plane buffers (engine/flat.py)
LAUNCH_PLANS = os.environ.get("MMT_LAUNCH_PLANS", "1") != "0"
_LP_SLOTS = 512
_LP_MAX = 4           # plans kept (least recently used first out)
_LAUNCH_PLANS = {}    # insertion-ordered: the least recently used plan first
_LP_LOCK = _threading.Lock()


class _LibProxy(object):
    """the loaded library; every entry point is handed out through a thin wrapper that also notes the call when this thread records"""

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if name in _NO_RECORD:
            w = f
        else:
            def w(*args, _f=f):
                rec = getattr(_TLS, "rec", None)
                if rec is not None:
                    rec.calls.append((_f, args))
                return _f(*args)
        self.__dict__[name] = w
        return w


class _Call(ctypes.Structure):   # include/mmtpsm.h: mmt_call
    _fields_ = [("fn", c_void_p), ("a", ctypes.c_long * 16)]


C_REPLAY = os.environ.get("MMT_C_REPLAY", "1") != "0"   # a plan's runs of C-ABI calls replayed by ONE library call (mmt_replay), the lock released


def _compile_plan(plan):
    """plan.calls -> segments: ("c", array of mmt_call, n, [(index, argument) positions holding the recorded input pointer]) for runs of
    recorded library calls with integer / pointer arguments, ("py", f, args) for everything else (record_torch closures, entry
    points with a floating-point parameter)"""
    segs, run = [], []

    def flush():
        if run:
            arr = (_Call * len(run))()
            patch = []
            for i, (addr, vals) in enumerate(run):
                arr[i].fn = addr
                for j, v in enumerate(vals):
                    arr[i].a[j] = v
                    if v == plan.in_ptr:
                        patch.append((i, j))
            segs.append(("c", arr, len(run), patch))
            run.clear()
    for f, args in plan.calls:
        enc = None
        at = getattr(f, "argtypes", None)
        if at is not None and len(args) <= 16 and len(at) == len(args) and not any(t in (c_float, ctypes.c_double) for t in at):
            enc = []
            for a in args:
                if a is None:
                    enc.append(0)
                elif isinstance(a, int):
                    enc.append(a)
                elif hasattr(a, "_obj"):                      # ctypes.byref(structure): the structure stays alive with the plan's argument tuple
                    enc.append(ctypes.addressof(a._obj))
                elif isinstance(a, ctypes.Array) or isinstance(a, ctypes.Structure):
                    enc = None                                # (by-value aggregates: not through the integer prototype)
                    break
                else:
                    enc = None
                    break
        if enc is None:
            flush()
            segs.append(("py", f, args))
        else:
            run.append((ctypes.cast(f, c_void_p).value, enc))
    flush()
    return segs


class LaunchPlan(object):
    __slots__ = ("calls", "result", "in_ptr", "slot_buf", "slot_next", "pool", "base", "gen", "seen", "segs", "dead")
    travels = False   # the pool of its own statistics slots (_Slot: base, gen): zeroed before every replay, never copied to the host

    def __init__(self, device):
        self.calls, self.result, self.in_ptr, self.seen, self.dead = [], None, None, 0, False
        self.slot_buf = torch.zeros((_LP_SLOTS, STAT_W), dtype=torch.float32, device=device)
        self.slot_next = 0
        self.pool = torch.cuda.MemPool()
        self.base, self.gen = self.slot_buf.data_ptr(), 0

    def __del__(self):
        # A plan sits in a reference cycle (its result tensors carry statistics slots whose pool it is), so it dies in the cyclic
        # collector -- at ANY allocation, also in the middle of another plan's recording, i.e. inside torch.cuda.use_mem_pool(): a
        # MemPool destroyed there aborts the process in the caching allocator (seen once in ~10 runs of the GPU suite, "Fatal Python
        # error: Aborted / Garbage-collecting" under planned()).  The pool is handed to a graveyard instead and destroyed at the next
        # safe point: the entry of planned(), outside every pool context (_drain_pools).
        try:
            p = self.pool
            if p is not None:
                self.pool = None
                _POOL_GRAVE.append(p)
        except Exception:   # (interpreter shutdown: the module's globals may be gone)
            pass


_POOL_GRAVE = []   # MemPool objects of dead plans, destroyed by _drain_pools
_POOL_CTX = [0, False]   # threads inside torch.cuda.use_mem_pool right now, and whether the cyclic collector is to be switched on again


class _no_gc_in_pool(object):
    """around torch.cuda.use_mem_pool: the cyclic collector stays off while ANY thread records a plan.  The graveyard above covers a
    dead plan's MemPool and the collector of the recording thread; the teacher's thread records its plans while the step's thread
    allocates, and a collection THERE -- the launch plans, streams and pooled tensors of a trainer that died -- aborted the process
    the same way ("Fatal Python error: Aborted", the step's thread "Garbage-collecting", the teacher's inside this context;
    tests/test_deterministic_backbones_gpu.py, two trainers in one process).  A recording is one backbone pass per plan: the
    collector misses a few milliseconds; reference counting frees as ever."""

    def __enter__(self):
        with _LP_LOCK:
            if _POOL_CTX[0] == 0:
                _POOL_CTX[1] = _gc.isenabled()
                _gc.disable()
            _POOL_CTX[0] += 1

    def __exit__(self, *exc):
        with _LP_LOCK:
            _POOL_CTX[0] -= 1
            if _POOL_CTX[0] == 0 and _POOL_CTX[1]:
                _gc.enable()
        return False


def _drain_pools():
    """destroy the memory pools of plans that died since the last call (never inside a pool context: see LaunchPlan.__del__)"""
    while _POOL_GRAVE:
        try:
            _POOL_GRAVE.pop()
        except IndexError:   # (another thread drained it)
            break


def record_torch(fn):
    """inside a pass that may be recorded: `fn()` -- a library (ATen) operation on tensors of the pass, already executed by the
    caller -- is to be repeated by every replay (a plan sees C-ABI calls only).  fn must read and write the SAME tensor objects."""
    rec = getattr(_TLS, "rec", None)
    if rec is not None:
        def w(_fn=fn):
            _fn()
            return 0
        rec.calls.append((w, ()))


def planned(tag, fn, x):
    """fn(x) -- a no-grad pass that issues nothing but C-ABI launches and tensor allocations (a backbone pass) -- through a launch
    plan: the first call of a (tag, shape, stream, arithmetic) runs as it is (caches warm up: weight planes, folded BN), the second
    is recorded, later ones are replayed.  -> fn's result (replays return the SAME tensor objects, refilled)."""
    # (the library's per-call switches -- A/B timing, parity tests -- choose kernels: part of the key)
    key = (tag, tuple(x.shape), x.dtype, _stream(), _PLAN_EPOCH[0], PLANES_EPOCH, LAYOUT_EPOCH[0], F16X2, _PREC, _BF16_STORAGE, _RB_EPOCH[0], _DET,
           lib().mmt_conv_switches())
    if getattr(_TLS, "rec", None) is None and _POOL_GRAVE:
        with _LP_LOCK:
            if _POOL_CTX[0] == 0:   # (no thread inside a pool context, and none enters one while the pools go: it takes this lock)
                _drain_pools()
    with _LP_LOCK:
        plan = _LAUNCH_PLANS.pop(key, None)
        if plan is None:
            # a small LRU: every plan pins the activations of a whole pass in a private memory pool, and batches of
            # varying shape would otherwise pile up one footprint per shape; eviction is per key, never a blanket clear under
            # another thread's replay
            while len(_LAUNCH_PLANS) >= _LP_MAX:
                _LAUNCH_PLANS.pop(next(iter(_LAUNCH_PLANS)))
            plan = LaunchPlan(x.device)
        _LAUNCH_PLANS[key] = plan   # (re-inserted at the recent end)
    plan.seen += 1
    if plan.seen == 1 or plan.dead or getattr(_TLS, "rec", None) is not None:
        return fn(x)
    if plan.seen == 2:
        _TLS.rec = plan
        try:
            with _no_gc_in_pool(), torch.cuda.use_mem_pool(plan.pool):
                plan.result = fn(x)
        except BaseException:
            with _LP_LOCK:
                _LAUNCH_PLANS.pop(key, None)
            raise
        finally:
            _TLS.rec = None
        plan.in_ptr = x.data_ptr()
        # the input must have reached the recorded launches as a direct pointer argument -- the only thing a replay patches.  A pass
        # that read it through a tensor operation or an argument block would replay the recorded batch for ever: never replayed
        if not any(type(a) is int and a == plan.in_ptr for _f, args in plan.calls for a in args):
            dead_pool, plan.pool = plan.pool, None
            plan.dead, plan.calls = True, []
            del dead_pool   # (outside the pool context: destroyed here and now)
        return plan.result
    plan.slot_buf.zero_()
    old, new = plan.in_ptr, x.data_ptr()
    if C_REPLAY:
        segs = getattr(plan, "segs", None)
        if segs is None:
            segs = plan.segs = _compile_plan(plan)
        replay = _lib_raw().mmt_replay
        for sg in segs:
            if sg[0] == "c":
                for i, j in sg[3]:
                    sg[1][i].a[j] = new
                if replay(sg[1], sg[2], None):
                    raise RuntimeError("a replayed launch failed")
            elif sg[1](*[new if (type(a) is int and a == old) else a for a in sg[2]]):
                raise RuntimeError("a replayed launch failed")
        C_CALLS[0] += len(plan.calls)
        return plan.result
    if old == new:
        for f, args in plan.calls:
            if f(*args):
                raise RuntimeError("a replayed launch failed")
    else:
        for f, args in plan.calls:
            if f(*[new if (type(a) is int and a == old) else a for a in args]):
                raise RuntimeError("a replayed launch failed")
    C_CALLS[0] += len(plan.calls)
    return plan.result


def exported_symbols():
    return sorted(_SIGS)


C_CALLS = [0]   # interpreter -> library calls that issue work (every one passes through _check); bench.py reports them per step


def _check(code, what):
    C_CALLS[0] += 1
    if code != 0:
        raise RuntimeError("%s failed with code %d" % (what, code))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_dev = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device   # (the C call, without torch.cuda's lazy-init wrapper: ~700 calls per step)


_TLS = _threading.local()   # .stream: raw handle that replaces the current stream for the launches of this thread (side-stream weight gradients)


def _stream():
    """raw hipStream_t of torch's current stream on the current device (per thread: the teacher thread has its own)"""
    ov = getattr(_TLS, "stream", None)
    if ov is not None:
        return ov
    if _raw_stream is not None:  # one C call instead of building a torch.cuda.Stream object (~9 us, ~230 calls per step)
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("%s must be a GPU tensor: the MI355X HIP library is the only backend" % name)
    return t


def _p(t):
    return None if t is None else t.data_ptr()


def nhwc(x):
    """(N,C,H,W)-shaped tensor -> same tensor guaranteed dense in NHWC memory order."""
    _dev(x)
    if x.dim() != 4:
        raise RuntimeError("expected a 4-D activation")
    if x.dtype != torch.float32 and x.dtype != torch.bfloat16:
        raise RuntimeError("fp32 (or, with bf16 storage, bf16) activations only")
    if x.is_contiguous(memory_format=torch.channels_last):   # (one call; size-1 dimensions are ignored by both tests)
        return x
    if not x.permute(0, 2, 3, 1).is_contiguous():
        x = x.contiguous(memory_format=torch.channels_last)
        if not x.permute(0, 2, 3, 1).is_contiguous():  # C==1 / H==W==1 corner cases of torch's format logic
            x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x


def empty_nhwc(n, c, h, w, device, zero=False, dtype=torch.float32):
    if zero:
        return torch.zeros((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)   # one call


# ------------------------------------------------------------------------------------------ ROIAlign
def _pyramid(feats, scales, grads=None):
    p = Pyramid()
    p.num_levels = len(feats)
    p.N, p.C = feats[0].shape[0], feats[0].shape[1]
    for i, f in enumerate(feats):
        p.feat[i] = f.data_ptr()
        p.grad_feat[i] = grads[i].data_ptr() if grads is not None else None
        p.H[i], p.W[i] = f.shape[2], f.shape[3]
        p.scale[i] = float(scales[i])
    return p


def roi_align_forward(feats, scales, rois, levels, ph, pw, sr):
    """feats: list of (N,C,H,W) NHWC-dense tensors; rois (K,5) fp32; levels (K,) int32 -> (K,C,ph,pw) NHWC-dense"""
    feats = [nhwc(f) for f in feats]
    rois = _dev(rois).float().contiguous()
    levels = _dev(levels).to(torch.int32).contiguous()
    K = rois.shape[0]
    out = empty_nhwc(K, feats[0].shape[1], ph, pw, rois.device)
    if K:
        p = _pyramid(feats, scales)
        if feats[0].dtype == torch.bfloat16:  # bf16 activation storage: levels as stored, pooled output fp32
            if any(f.dtype != torch.bfloat16 for f in feats):
                raise RuntimeError("roi_align_forward: pyramid levels of mixed storage types")
            _check(lib().mmt_roi_align_forward_bf16(ctypes.byref(p), _p(rois), _p(levels), K, ph, pw, sr, _p(out), _stream()),
                   "mmt_roi_align_forward_bf16")
        else:
            _check(lib().mmt_roi_align_forward(ctypes.byref(p), _p(rois), _p(levels), K, ph, pw, sr, _p(out), _stream()),
                   "mmt_roi_align_forward")
    return out


def roi_align_backward(grad_out, shapes, scales, rois, levels, ph, pw, sr, into=None):
    """-> list of zero-initialised-then-accumulated gradients, one per level (N,C,H,W) NHWC-dense
    into: per level an existing fp32 gradient tensor of that shape to accumulate into (the atomics add to what is there), or None"""
    g = nhwc(grad_out)
    rois = _dev(rois).float().contiguous()
    levels = _dev(levels).to(torch.int32).contiguous()
    K = rois.shape[0]
    if into is not None and not any(t is not None for t in into):
        into = None
    if _DET:
        return _roi_align_backward_ordered(g, shapes, scales, rois, levels, K, ph, pw, sr, into)
    if into is None and g.is_cuda and g.dtype == torch.float32 and os.environ.get("MMT_ROI_BWD_DENSE", "0") != "0":
        # opt-in: the tile-gather form writes every element of every level once -- no clear, no atomics, repeatable (csrc/roi_align.hip)
        grads = [empty_nhwc(s[0], s[1], s[2], s[3], g.device) for s in shapes]
        p = _pyramid(grads, scales, grads)
        rc = lib().mmt_roi_align_backward_dense(ctypes.byref(p), _p(rois), _p(levels), K, ph, pw, sr, _p(g), _stream())
        if rc == 0:
            return grads
        if rc != 1:
            _check(rc, "mmt_roi_align_backward_dense")
    grads = [into[i] if (into is not None and into[i] is not None) else empty_nhwc(s[0], s[1], s[2], s[3], g.device, zero=True)
             for i, s in enumerate(shapes)]
    if into is not None:
        for t, s in zip(grads, shapes):
            if tuple(t.shape) != tuple(s) or t.dtype != torch.float32 or not t.is_contiguous(memory_format=torch.channels_last):
                raise RuntimeError("roi_align_backward: `into` must hold dense NHWC fp32 tensors of the levels' shapes")
    if K:
        p = _pyramid(grads, scales, grads)
        _check(lib().mmt_roi_align_backward(ctypes.byref(p), _p(rois), _p(levels), K, ph, pw, sr, _p(g), _stream()),
               "mmt_roi_align_backward")
    return grads


def _roi_align_backward_ordered(g, shapes, scales, rois, levels, K, ph, pw, sr, into):
    """deterministic mode: the tile-gather form (include/mmtpsm.h: mmt_roi_align_backward_ordered) -- a level given in `into` gets
    grad = grad + (the tile's fixed-order sum), the others are written, zeros included; a call the kernel does not take raises"""
    _dev(g, "grad_out")
    if g.dtype != torch.float32:
        raise NotImplementedError("roi_align_backward in deterministic mode: fp32 gradients only")
    grads, mask = [], 0
    for i, s in enumerate(shapes):
        t = into[i] if into is not None else None
        if t is not None:
            if tuple(t.shape) != tuple(s) or t.dtype != torch.float32 or not t.is_contiguous(memory_format=torch.channels_last):
                raise RuntimeError("roi_align_backward: `into` must hold dense NHWC fp32 tensors of the levels' shapes")
            mask |= 1 << i
        else:
            t = empty_nhwc(s[0], s[1], s[2], s[3], g.device)
        grads.append(t)
    p = _pyramid(grads, scales, grads)
    rc = lib().mmt_roi_align_backward_ordered(ctypes.byref(p), _p(rois), _p(levels), K, ph, pw, sr, _p(g), mask, _stream())
    if rc == 1:
        raise NotImplementedError("roi_align_backward in deterministic mode: roi_align_bwd_tiles_kernel takes sampling_ratio 2, "
                                  "C %% 64 == 0, C <= 256 and K <= 8192 (got sampling_ratio %d, C %d, K %d), and the scatter kernel adds "
                                  "with float atomics; set_deterministic(False)" % (sr, shapes[0][1], K))
    _check(rc, "mmt_roi_align_backward_ordered")
    return grads


def _roi_maps(shapes, scales, c_off, out_C, feats=None, grads=None):
    """mmt_roi_maps of 1..4 maps of the shapes (N, C, H, W); c_off None: the maps side by side in the order given"""
    n = len(shapes)
    if not 1 <= n <= 4 or len(scales) != n or (c_off is not None and len(c_off) != n):
        raise RuntimeError("roi_align_maps: 1..4 maps with one scale (and one channel offset) each, got %d" % n)
    if any(len(s) != 4 or s[0] != shapes[0][0] for s in shapes):
        raise RuntimeError("roi_align_maps: maps are (N, C, H, W) tensors of one batch size")
    if c_off is None:
        c_off = [sum(s[1] for s in shapes[:i]) for i in range(n)]
    p = RoiMaps()
    p.num_maps, p.N = n, shapes[0][0]
    p.out_C = int(out_C) if out_C is not None else sum(s[1] for s in shapes)
    for i, s in enumerate(shapes):
        p.feat[i] = feats[i].data_ptr() if feats is not None else None
        p.grad_feat[i] = grads[i].data_ptr() if grads is not None else None
        p.C[i], p.H[i], p.W[i] = s[1], s[2], s[3]
        p.c_off[i], p.scale[i] = int(c_off[i]), float(scales[i])
    return p


def roi_align_maps_forward(feats, scales, rois, ph, pw, sr, c_off=None, out=None):
    """include/mmtpsm.h: mmt_roi_align_maps_forward.  feats: 1..4 fp32 (N, C_m, H_m, W_m) NHWC-dense maps; rois (K, 5) fp32; every ROI
    is pooled from every map -> (K, sum C_m, ph, pw) NHWC-dense, map m at channels c_off[m] .. c_off[m] + C_m (default: side by
    side).  out: an NHWC-dense fp32 (K, out_C, ph, pw) tensor to write the slices of (channels no map owns stay as they are)"""
    feats = [nhwc(_dev(f, "feats")) for f in feats]
    if any(f.dtype != torch.float32 for f in feats):
        raise RuntimeError("roi_align_maps_forward: fp32 maps only")
    rois = _dev(rois, "rois").float().contiguous()
    K = rois.shape[0]
    if out is None:
        out = empty_nhwc(K, sum(f.shape[1] for f in feats), ph, pw, rois.device)
    elif (not out.is_cuda or out.dtype != torch.float32 or out.dim() != 4 or (out.shape[0], out.shape[2], out.shape[3]) != (K, ph, pw)
          or nhwc(out) is not out):
        raise RuntimeError("roi_align_maps_forward: `out` is an NHWC-dense fp32 GPU tensor (K, out_C, ph, pw)")
    p = _roi_maps([tuple(f.shape) for f in feats], scales, c_off, out.shape[1], feats=feats)
    _check(lib().mmt_roi_align_maps_forward(ctypes.byref(p), _p(rois), K, ph, pw, sr, _p(out), _stream()), "mmt_roi_align_maps_forward")
    return out


def roi_align_maps_backward(grad_out, shapes, scales, rois, ph, pw, sr, c_off=None):
    """include/mmtpsm.h: mmt_roi_align_maps_backward.  grad_out (K, out_C, ph, pw) -> one zero-initialised-then-accumulated (fp32
    atomics) gradient per map, (N, C_m, H_m, W_m) NHWC-dense"""
    g = nhwc(_dev(grad_out, "grad_out"))
    if g.dtype != torch.float32:
        raise RuntimeError("roi_align_maps_backward: fp32 gradients only")
    rois = _dev(rois, "rois").float().contiguous()
    K = rois.shape[0]
    if (g.shape[0], g.shape[2], g.shape[3]) != (K, ph, pw):
        raise RuntimeError("roi_align_maps_backward: grad_out is (K, out_C, ph, pw)")
    _refuse_unordered("roi_align_maps_kernel", "the CSPN mask head (MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR PRCNNFeatureExtractor)")
    shapes = [tuple(s) for s in shapes]
    p = _roi_maps(shapes, scales, c_off, g.shape[1])
    grads = [empty_nhwc(s[0], s[1], s[2], s[3], g.device, zero=True) for s in shapes]
    for i, t in enumerate(grads):
        p.grad_feat[i] = t.data_ptr()
    _check(lib().mmt_roi_align_maps_backward(ctypes.byref(p), _p(rois), K, ph, pw, sr, _p(g), _stream()), "mmt_roi_align_maps_backward")
    return grads


# ------------------------------------------------------------------------------------------ NMS
def nms_batched(boxes, seg_off, max_n, thr):
    """boxes (T,4) score-sorted within each segment; seg_off int32 (B+1) on device.
    -> keep (B,max_n) int32 positions within the segment, cnt (B,) int32"""
    boxes = _dev(boxes).float().contiguous()
    seg_off = _dev(seg_off).to(torch.int32).contiguous()
    B = seg_off.numel() - 1
    words = (max_n + 63) // 64
    ws = torch.empty((B * max_n * words,), dtype=torch.int64, device=boxes.device)
    keep = torch.empty((B, max_n), dtype=torch.int32, device=boxes.device)
    cnt = torch.zeros((B,), dtype=torch.int32, device=boxes.device)
    if B and max_n:
        _check(lib().mmt_nms_batched(_p(boxes), _p(seg_off), B, max_n, float(thr), _p(ws), _p(keep), _p(cnt), _stream()),
               "mmt_nms_batched")
    return keep, cnt


SOFT_NMS_MAX = 2048                              # candidates of one segment (csrc/softnms.hip)
SOFT_NMS_METHODS = {"linear": 0, "gaussian": 1}  # s *= 1 - ov where ov >= thr, or s *= exp(-ov^2 / sigma) everywhere


def _soft_nms_args(what, method, nms_thresh, sigma, min_score):
    """what mmt_soft_nms_batched refuses, refused here before any launch -> the method's number"""
    if method not in SOFT_NMS_METHODS:
        raise ValueError("%s: method %r is not one of %s" % (what, method, sorted(SOFT_NMS_METHODS)))
    sigma, min_score, nms_thresh = float(sigma), float(min_score), float(nms_thresh)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError("%s: sigma %r is not a positive finite number" % (what, sigma))
    if not 0.0 < min_score <= 1.0:
        raise ValueError("%s: min_score %r is outside (0, 1]" % (what, min_score))
    if not 0.0 < nms_thresh <= 1.0:
        raise ValueError("%s: nms_thresh %r is outside (0, 1]" % (what, nms_thresh))
    return SOFT_NMS_METHODS[method]


def soft_nms_batched(boxes, scores, seg_off, max_n, method="linear", nms_thresh=0.5, sigma=0.5, min_score=0.001):
    """Soft-NMS of B pre-sorted segments in one launch (include/mmtpsm.h: mmt_soft_nms_batched).  boxes (T, 4) and scores (T,)
    sorted by descending score within each segment; seg_off int32 (B + 1) on the device
    -> picked (B, max_n) int32 positions within the segment in pick order, cnt (B,) int32, scores (T,) decayed -- or None when
    max_n > 2048"""
    m = _soft_nms_args("soft_nms_batched", method, nms_thresh, sigma, min_score)
    if max_n < 0:
        raise ValueError("soft_nms_batched: max_n %d" % max_n)
    if max_n > SOFT_NMS_MAX:
        return None
    boxes = _dev(boxes).float().contiguous()
    scores = _dev(scores).float().contiguous()
    seg_off = _dev(seg_off).to(torch.int32).contiguous()
    if boxes.dim() != 2 or boxes.shape[1] != 4 or scores.dim() != 1 or scores.shape[0] != boxes.shape[0]:
        raise ValueError("soft_nms_batched: boxes (T, 4) and scores (T,), not %s and %s" % (tuple(boxes.shape), tuple(scores.shape)))
    B = seg_off.numel() - 1
    picked = torch.empty((B, max_n), dtype=torch.int32, device=boxes.device)
    cnt = torch.zeros((B,), dtype=torch.int32, device=boxes.device)
    out = scores.clone()
    if B > 0:
        _check(lib().mmt_soft_nms_batched(_p(boxes), _p(scores), _p(seg_off), B, max_n, m, float(nms_thresh), float(sigma),
                                          float(min_score), _p(picked), _p(cnt), _p(out), _stream()), "mmt_soft_nms_batched")
    return picked, cnt, out


def det_postprocess(prob, dec, per, score_thresh, nms_thresh, detections_per_img, zero_tails=False, soft=None):
    """PostProcessor.filter_results for a batch (prob (R, nc), dec (R, nc * 4), per = rows per image) on the device:
    -> boxes (N, cap, 4), scores (N, cap), labels int64 (N, cap), counts int32 (N,) -- or None when an image has more than
    2048 rows / nc > 64 (the caller's tensor formulation takes those).  `soft`: (method number, sigma, min_score) of
    det_postprocess_soft, which is this function with mmt_det_postprocess_soft as its entry"""
    N, nc = len(per), prob.shape[1]
    if N == 0 or nc < 2 or nc > 64 or max(per) > 2048 or prob.dtype != torch.float32:
        return None
    prob = _dev(prob).contiguous()
    dec = _dev(dec).float().contiguous()
    offs = [0]
    for n_ in per:
        offs.append(offs[-1] + int(n_))
    host = (ctypes.c_int32 * (N + 1))(*offs)
    dev = prob.device
    row_off = torch.tensor(offs, dtype=torch.int32).to(dev, non_blocking=True)
    cap = max(max(per) * (nc - 1), 1)
    fn = lib().mmt_det_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_long, [c_int, c_int, c_int]
    nb = fn(offs[-1], N, nc)
    if nb < 0:
        return None
    ws = torch.empty((nb // 16 + 1, 4), dtype=torch.float32, device=dev)
    alloc = torch.zeros if zero_tails else torch.empty   # zero_tails: rows behind an image's count are read by the caller
    ob = alloc((N, cap, 4), dtype=torch.float32, device=dev)
    os_ = alloc((N, cap), dtype=torch.float32, device=dev)
    ol = alloc((N, cap), dtype=torch.int64, device=dev)
    oc = torch.empty((N,), dtype=torch.int32, device=dev)
    if soft is None:
        _check(lib().mmt_det_postprocess(_p(prob), _p(dec), _p(row_off), ctypes.cast(host, c_void_p), N, nc, float(score_thresh),
                                         float(nms_thresh), int(detections_per_img), _p(ws), _p(ob), _p(os_), _p(ol), _p(oc),
                                         _stream()), "mmt_det_postprocess")
    else:
        _check(lib().mmt_det_postprocess_soft(_p(prob), _p(dec), _p(row_off), ctypes.cast(host, c_void_p), N, nc, float(score_thresh),
                                              float(nms_thresh), int(detections_per_img), soft[0], float(soft[1]), float(soft[2]),
                                              _p(ws), _p(ob), _p(os_), _p(ol), _p(oc), _stream()), "mmt_det_postprocess_soft")
    return ob, os_, ol, oc


def det_postprocess_soft(prob, dec, per, score_thresh, nms_thresh, detections_per_img, method="linear", sigma=0.5, min_score=0.001,
                         zero_tails=False):
    """det_postprocess with Soft-NMS (mmt_det_postprocess_soft): the same outputs with DECAYED scores, the same None-when-out-of-
    range contract; a method, sigma, min_score or nms_thresh that the library refuses raises ValueError before any launch"""
    m = _soft_nms_args("det_postprocess_soft", method, nms_thresh, sigma, min_score)
    return det_postprocess(prob, dec, per, score_thresh, nms_thresh, detections_per_img, zero_tails=zero_tails,
                           soft=(m, sigma, min_score))


# ------------------------------------------------------------------------------------------ test-time augmentation
TTA_MAX_VIEWS = 8   # csrc/tta.hip: the bits of flip_mask (the teacher's slot count)


def _tta_flip_mask(flips, V):
    flips = [bool(f) for f in flips]
    if len(flips) != V:
        raise ValueError("one flip flag per view: %d flags for %d views" % (len(flips), V))
    if not 1 <= V <= TTA_MAX_VIEWS:
        raise ValueError("1 to %d views, not %d" % (TTA_MAX_VIEWS, V))
    return sum(1 << v for v, f in enumerate(flips) if f)


def tta_merge_box(logits, reg, flips):
    """logits (V, R, C), reg (V, R, 4C) of the same R proposals on V views, flips[v]: view v is a mirror image
    -> prob (R, C) = mean over views of the row softmax, reg (R, 4C) = mean with dx negated for mirrored views (one launch)"""
    logits, reg = _dev(logits, "logits"), _dev(reg, "reg")
    if logits.dim() != 3 or reg.dim() != 3 or logits.dtype != torch.float32 or reg.dtype != torch.float32:
        raise ValueError("tta_merge_box: fp32 logits (V, R, C) and reg (V, R, 4C)")
    V, R, C = logits.shape
    if tuple(reg.shape) != (V, R, 4 * C):
        raise ValueError("tta_merge_box: reg %s does not go with logits %s" % (tuple(reg.shape), tuple(logits.shape)))
    mask = _tta_flip_mask(flips, V)
    logits, reg = logits.contiguous(), reg.contiguous()
    prob = torch.empty((R, C), dtype=torch.float32, device=logits.device)
    out = torch.empty((R, 4 * C), dtype=torch.float32, device=logits.device)
    _check(lib().mmt_tta_merge_box(_p(logits), _p(reg), V, R, C, mask, _p(prob), _p(out), _stream()), "mmt_tta_merge_box")
    return prob, out


def tta_merge_mask(logits, labels, flips):
    """logits (V, D, C, M, M) of the same D detections on V views, labels (D,) int64 -> (D, 1, M, M): the mean over views of the
    predicted class's sigmoid, mirrored views read right to left (one launch)"""
    logits, labels = _dev(logits, "logits"), _dev(labels, "labels")
    if logits.dim() != 5 or logits.shape[3] != logits.shape[4] or logits.dtype != torch.float32:
        raise ValueError("tta_merge_mask: fp32 logits (V, D, C, M, M)")
    V, D, C, M, _ = logits.shape
    if labels.dtype != torch.int64 or tuple(labels.shape) != (D,):
        raise ValueError("tta_merge_mask: int64 labels (D,)")
    mask = _tta_flip_mask(flips, V)
    logits, labels = logits.contiguous(), labels.contiguous()
    prob = torch.empty((D, 1, M, M), dtype=torch.float32, device=logits.device)
    _check(lib().mmt_tta_merge_mask(_p(logits), _p(labels), V, D, C, M, mask, _p(prob), _stream()), "mmt_tta_merge_mask")
    return prob


# ------------------------------------------------------------------------------------------ input augmentation
def resample_u8(img, out_size, horizontal, bounds, coeffs):
    """img uint8 (H,W,3) on the device -> resampled along one axis (Pillow 8-bit bilinear); bounds/coeffs: device int32"""
    _dev(img, "img")
    Hh, Ww = img.shape[0], img.shape[1]
    out = torch.empty((Hh, out_size, 3) if horizontal else (out_size, Ww, 3), dtype=torch.uint8, device=img.device)
    _check(lib().mmt_resample_u8(_p(img), _p(out), Hh, Ww, out_size, 1 if horizontal else 0, _p(bounds), _p(coeffs),
                                 coeffs.shape[1], _stream()), "mmt_resample_u8")
    return out


def aug_views(img, flip, brightness, contrast, hue_shift, mean3, out):
    """img uint8 (H,W,3); per-view device tensors brightness/contrast (float32 [V]), hue_shift (int32 [V], < 0: no colour
    chain); out: zero-initialised fp32 (V, Hp, Wp, C>=3) NHWC batch -> the H x W corner of every view filled in place"""
    _dev(img, "img")
    V, Hp, Wp, C = out.shape
    m = (c_float * 3)(*[float(x) for x in mean3])
    ws = torch.empty((V,), dtype=torch.int64, device=img.device)
    _check(lib().mmt_aug_views(_p(img), img.shape[0], img.shape[1], 1 if flip else 0, _p(brightness), _p(contrast),
                               _p(hue_shift), _p(ws), V, m, _p(out), Hp * Wp * C, Wp, C, _stream()), "mmt_aug_views")
    return out


def aug_erase(out, rects, fill_off, fills, mean3):
    """RandomErasing rectangles {view, top, left, h, w} (int32 [R,5]) filled with the RGB bytes fills[fill_off[r]:...];
    rectangles of ONE call must not overlap inside a view (the caller serialises overlapping ones)"""
    V, Hp, Wp, C = out.shape
    m = (c_float * 3)(*[float(x) for x in mean3])
    _check(lib().mmt_aug_erase(_p(out), Hp * Wp * C, Wp, C, _p(rects), _p(fill_off), _p(fills), rects.shape[0], m, _stream()),
           "mmt_aug_erase")
    return out


def match_targets(cand, cand_off, gt, gt_off, n_images, high, low, allow_low_quality=False, gt_labels=None,
                  visible=None, shared_cand=False, rpn_labels=False, box_labels=False, weights=None):
    """ground-truth assignment for all images of a batch in one launch (include/mmtpsm.h: mmt_match_targets).
    cand (A,4) [shared_cand: one anchor grid for all images] / (A_total,4); cand_off, gt_off: device int32 [N+1].
    -> matches int32 (A_total,), labels (float for the RPN / int64 for the box head / None), regression targets or None"""
    cand = _dev(cand, "cand").float().contiguous()
    gt = _dev(gt, "gt").float().contiguous()
    A_total = cand.shape[0] * (n_images if shared_cand else 1)
    dev = cand.device
    matches = torch.empty((A_total,), dtype=torch.int32, device=dev)
    lf = torch.empty((A_total,), dtype=torch.float32, device=dev) if rpn_labels else None
    li = torch.empty((A_total,), dtype=torch.int64, device=dev) if box_labels else None
    reg = torch.empty((A_total, 4), dtype=torch.float32, device=dev) if weights is not None else None
    top = torch.empty((max(gt.shape[0], 1),), dtype=torch.int32, device=dev) if allow_low_quality else None
    wx, wy, ww, wh = weights if weights is not None else (1.0, 1.0, 1.0, 1.0)
    vis = None
    if visible is not None:
        vis = visible.to(torch.uint8) if visible.dtype != torch.uint8 else visible
    gl = gt_labels.to(torch.int64).contiguous() if gt_labels is not None else None
    _check(lib().mmt_match_targets(_p(cand), _p(cand_off), _p(gt), _p(gt_off), _p(gl), _p(vis), n_images, A_total, gt.shape[0],
                                   1 if shared_cand else 0, float(high), float(low), 1 if allow_low_quality else 0, float(wx),
                                   float(wy), float(ww), float(wh), _p(top), _p(matches), _p(lf), _p(li), _p(reg), _stream()),
           "mmt_match_targets")
    return matches, (lf if rpn_labels else li), reg


def roi_format_levels(boxes, s0=None, lvl0=None, eps=None, k_min=0, k_max=0):
    """boxes: per-image (n_i, 4) xyxy tensors -> rois (K, 5) = (image, box) and, with a level mapper's constants, the FPN
    level of every roi as int32 (include/mmtpsm.h: mmt_roi_format_levels); one launch"""
    n = len(boxes)
    if n > 32:
        raise RuntimeError("roi_format_levels: at most 32 images per call")
    bs = [_dev(b, "boxes") if (b.is_contiguous() and b.dtype == torch.float32 and not (b.data_ptr() & 15)) else
          _dev(b, "boxes").float().contiguous().clone() for b in boxes]
    K = sum(b.shape[0] for b in bs)
    dev = bs[0].device
    rois = torch.empty((K, 5), dtype=torch.float32, device=dev)
    levels = torch.empty((K,), dtype=torch.int32, device=dev) if s0 is not None else None
    if K == 0:
        return rois, levels
    ptrs = (c_void_p * n)(*[b.data_ptr() if b.shape[0] else None for b in bs])
    cnts = (c_int * n)(*[b.shape[0] for b in bs])
    _check(lib().mmt_roi_format_levels(ptrs, cnts, n, float(s0 or 1.0), float(lvl0 or 0.0), float(eps or 0.0), int(k_min), int(k_max),
                                       _p(rois), _p(levels), _stream()), "mmt_roi_format_levels")
    return rois, levels


AMAX_LOG = None
_TOPK_WS = {}   # (device, stream) -> workspace of mmt_rpn_topk (kernels of a stream run in order and may share it)


def rpn_topk(heads, ks, A):
    """heads[l]: fused RPN head output of level l, (N, 5A, H, W) NHWC-dense -> [topk indices (N, k_l) int64 per level]:
    torch.topk(logits, k_l, sorted=True)[1] of every (image, level) in five launches (include/mmtpsm.h: mmt_rpn_topk)"""
    L, N = len(heads), heads[0].shape[0]
    dev = heads[0].device
    lv = (RpnTopkLevel * L)()
    outs, keep, total = [], [], 0
    for l, (h, k) in enumerate(zip(heads, ks)):
        h = nhwc(h)
        if h.shape[1] != 5 * A or h.dtype != torch.float32:
            raise RuntimeError("rpn_topk: the fused fp32 head output (A logits + 4A deltas per pixel) is expected")
        o = torch.empty((N, k), dtype=torch.int64, device=dev)
        lv[l].head, lv[l].topk, lv[l].HW, lv[l].k = h.data_ptr(), o.data_ptr(), h.shape[2] * h.shape[3], k
        total += h.shape[2] * h.shape[3] * A
        outs.append(o)
        keep.append(h)
    fn = lib().mmt_rpn_topk_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_long, [c_int, c_int, ctypes.c_long]
    need = fn(N, L, total)
    key = (str(dev), _stream())
    ws = _TOPK_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _TOPK_WS[key] = torch.empty((need,), dtype=torch.uint8, device=dev)
    _check(lib().mmt_rpn_topk(ctypes.addressof(lv), L, N, A, ws.data_ptr(), _stream()), "mmt_rpn_topk")
    return outs


def relation_reg_labels(sorted_boxes, sorted_score, gt, gt_labels, thresholds):
    """IR-Net relation NMS label preparation of one image in one launch (include/mmtpsm.h: mmt_relation_reg_labels) or None
    when the shapes are beyond the kernel's LDS matrix (the caller keeps its tensor formulation)"""
    n, fg = sorted_score.shape
    G, T = gt.shape[0], len(thresholds)
    if T > 4 or G > 256 or n > 128 or n * max(G, 1) > 8192:   # (n <= 128: the per-box LDS arrays of the kernel)
        return None
    b = _dev(sorted_boxes, "boxes").float().contiguous()
    sc = sorted_score.float().contiguous()
    out = torch.empty((n, fg, T), dtype=torch.float32, device=b.device)
    th = (c_float * T)(*[float(t) for t in thresholds])
    g, gl = gt.float().contiguous(), gt_labels.to(torch.int64).contiguous()
    _check(lib().mmt_relation_reg_labels(_p(b), _p(sc), _p(g) if G else None, _p(gl) if G else None, n, fg, G, th, T, _p(out), _stream()),
           "mmt_relation_reg_labels")
    return out


def position_embedding(boxes, dim_g, freq):
    """IR-Net geometric embedding of all ordered box pairs per class: boxes (n, C, 4) -> (C, n, n, dim_g), one launch
    (include/mmtpsm.h: mmt_position_embedding); freq = the dim_g / 8 wave-length factors (device)"""
    b = _dev(boxes, "boxes").float().contiguous()
    n, C = b.shape[0], b.shape[1]
    out = torch.empty((C, n, n, dim_g), dtype=torch.float32, device=b.device)
    _check(lib().mmt_position_embedding(_p(b), n, C, int(dim_g), _p(freq), _p(out), _stream()), "mmt_position_embedding")
    return out


RELATION_ATTENTION_MAX_N = 128   # csrc/relation.hip: RA_MAXN
CIAM_MAX_N = 512                 # csrc/relation.hip: CI_MAXG (the whole batch is used as the bound of a group's size)


def relation_attention_fits(N, G, DQ, DV):
    return 1 <= N <= RELATION_ATTENTION_MAX_N and DQ <= 128 and DV <= 16


def relation_attention_fwd(q, k, wg, v, bias, C, N, G, topk, scale):
    """include/mmtpsm.h: mmt_relation_attention_fwd.  q, k (C*N, G*DQ), wg (C*N*N, G), v (C*N, G*DV), bias (G*DV)
    -> out (N, C, G*DV), P (C, G, N, N)"""
    DQ, DV = q.shape[1] // G, v.shape[1] // G
    out = torch.empty((N, C, G * DV), dtype=torch.float32, device=q.device)
    P = torch.empty((C, G, N, N), dtype=torch.float32, device=q.device)
    _check(lib().mmt_relation_attention_fwd(_p(q), _p(k), _p(wg), _p(v), _p(bias), C, N, G, DQ, DV, int(topk), float(scale), _p(P),
                                            _p(out), _stream()), "mmt_relation_attention_fwd")
    return out, P


def relation_attention_bwd(q, k, wg, v, P, dout, C, N, G, scale):
    DQ, DV = q.shape[1] // G, v.shape[1] // G
    dq, dk, dwg, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(wg), torch.empty_like(v)
    dS = torch.empty_like(P)
    _check(lib().mmt_relation_attention_bwd(_p(q), _p(k), _p(wg), _p(v), _p(P), _p(dout), C, N, G, DQ, DV, float(scale), _p(dS), _p(dq),
                                            _p(dk), _p(dwg), _p(dv), _stream()), "mmt_relation_attention_bwd")
    return dq, dk, dwg, dv


def ciam_fwd(x, group, gamma):
    """include/mmtpsm.h: mmt_ciam_fwd.  x (n, C, H, W) NCHW-dense fp32, group (n,) int64 with equal ids contiguous, gamma (1,)
    -> out like x, A (n, n), J (C, n) int32"""
    n, C = x.shape[0], x.shape[1]
    HW = x.shape[2] * x.shape[3]
    out = torch.empty((n, C, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
    A = torch.empty((n, n), dtype=torch.float32, device=x.device)
    J = torch.empty((C, n), dtype=torch.int32, device=x.device)
    _check(lib().mmt_ciam_fwd(_p(x), _p(group), n, C, HW, n, _p(gamma), _p(A), _p(J), _p(out), _stream()), "mmt_ciam_fwd")
    return out, A, J


def ciam_bwd(x, group, gamma, A, J, dout):
    n, C = x.shape[0], x.shape[1]
    HW = x.shape[2] * x.shape[3]
    dx = torch.empty((n, C, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
    ws = torch.empty((n * n + n,), dtype=torch.float32, device=x.device)
    dgamma = torch.empty((1,), dtype=torch.float32, device=x.device)
    if _DET:   # the rows' shares of dgamma added in row order
        part = torch.empty((n,), dtype=torch.float32, device=x.device)
        _check(lib().mmt_ciam_bwd_ordered(_p(x), _p(group), n, C, HW, n, _p(gamma), _p(A), _p(J), _p(dout), _p(ws), ws.data_ptr() + 4 * n * n,
                                          _p(dx), _p(dgamma), _p(part), _stream()), "mmt_ciam_bwd_ordered")
        return dx, dgamma
    _check(lib().mmt_ciam_bwd(_p(x), _p(group), n, C, HW, n, _p(gamma), _p(A), _p(J), _p(dout), _p(ws), ws.data_ptr() + 4 * n * n, _p(dx),
                              _p(dgamma), _stream()), "mmt_ciam_bwd")
    return dx, dgamma


def ciam_norm_kind(norm):
    """MODEL.RELATION_MASK.NORM as the kernels read it: 1 ("sum channel"), 2 ("L2 norm"), anything else 0 (none: the reference's
    else branch takes every other value)"""
    return int(norm) if norm in (1, 2) else 0


def ciam_norm_fits(n, C, HW):
    """the capacity of mmt_ciam_norm_fwd / _bwd, by the library's own expression (include/mmtpsm.h: mmt_ciam_norm_lds_bytes)"""
    return 0 < n <= CIAM_MAX_N and 0 < C <= 16 and 0 < HW and 0 < lib().mmt_ciam_norm_lds_bytes(n, C, HW) <= 65536


def ciam_norm_fwd(x, group, gamma, norm, pre_norm):
    """include/mmtpsm.h: mmt_ciam_norm_fwd.  x, group, gamma as ciam_fwd; norm 1 / 2 / other, pre_norm bool
    -> out like x, A (n, n), J (C, n) int32, saved (the energies and the normalisation's sums, for ciam_norm_bwd)"""
    n, C = x.shape[0], x.shape[1]
    HW = x.shape[2] * x.shape[3]
    if not ciam_norm_fits(n, C, HW):
        raise RuntimeError("mmt_ciam_norm_fwd: n = %d, C = %d, HW = %d is beyond 1..%d instances, 16 channels or 64 KiB of LDS "
                           "(mmt_ciam_norm_lds_bytes)" % (n, C, HW, CIAM_MAX_N))
    out = torch.empty((n, C, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
    A = torch.empty((n, n), dtype=torch.float32, device=x.device)
    J = torch.empty((C, n), dtype=torch.int32, device=x.device)
    saved = torch.empty((lib().mmt_ciam_norm_saved_floats(n, C),), dtype=torch.float32, device=x.device)
    _check(lib().mmt_ciam_norm_fwd(_p(x), _p(group), n, C, HW, ciam_norm_kind(norm), int(bool(pre_norm)), _p(gamma), _p(saved), _p(A),
                                   _p(J), _p(out), _stream()), "mmt_ciam_norm_fwd")
    return out, A, J, saved


def ciam_norm_bwd(x, group, gamma, norm, pre_norm, saved, A, J, dout):
    """include/mmtpsm.h: mmt_ciam_norm_bwd; in deterministic mode mmt_ciam_norm_bwd_ordered -> dx, dgamma"""
    n, C = x.shape[0], x.shape[1]
    HW = x.shape[2] * x.shape[3]
    if not ciam_norm_fits(n, C, HW):
        raise RuntimeError("mmt_ciam_norm_bwd: n = %d, C = %d, HW = %d is beyond the kernels' capacity" % (n, C, HW))
    dx = torch.empty((n, C, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
    ws = torch.empty((lib().mmt_ciam_norm_ws_floats(n, C),), dtype=torch.float32, device=x.device)
    dgamma = torch.empty((1,), dtype=torch.float32, device=x.device)
    f, what = (lib().mmt_ciam_norm_bwd_ordered, "mmt_ciam_norm_bwd_ordered") if _DET else (lib().mmt_ciam_norm_bwd, "mmt_ciam_norm_bwd")
    _check(f(_p(x), _p(group), n, C, HW, ciam_norm_kind(norm), int(bool(pre_norm)), _p(gamma), _p(saved), _p(A), _p(J), _p(dout), _p(ws),
             _p(dx), _p(dgamma), _stream()), what)
    return dx, dgamma


def rpn_gather_decode(heads, anchors, topks, A, clip, lim):
    """heads[l]: the fused RPN head output of level l, (N, 5A, H, W) NHWC-dense (A logits, then 4A deltas); anchors[l]
    (H*W*A, 4); topks[l] (N, k_l) int64 indices into H*W*A -> boxes (N, sumk, 4), scores (N, sumk), idx (N, sumk),
    box_reg (N, sumk, 4), level offsets (include/mmtpsm.h: mmt_rpn_gather_decode)"""
    a = RpnSelectArgs()
    L, N = len(heads), heads[0].shape[0]
    offs, keep = [0], []
    for l, (h, an, tk) in enumerate(zip(heads, anchors, topks)):
        h = nhwc(h)
        tk = tk.contiguous()
        keep += [h, tk]
        lv = a.lv[l]
        lv.head, lv.anchors, lv.topk = h.data_ptr(), an.data_ptr(), tk.data_ptr()
        lv.HW, lv.k, lv.out_off = h.shape[2] * h.shape[3], tk.shape[1], offs[-1]
        if h.shape[1] != 5 * A or an.shape[0] != lv.HW * A:
            raise RuntimeError("rpn_gather_decode: head / anchor shapes do not match A")
        offs.append(offs[-1] + tk.shape[1])
    sumk, dev = offs[-1], heads[0].device
    boxes = torch.empty((N, sumk, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((N, sumk), dtype=torch.float32, device=dev)
    idx = torch.empty((N, sumk), dtype=torch.int64, device=dev)
    reg = torch.empty((N, sumk, 4), dtype=torch.float32, device=dev)
    a.L, a.N, a.A, a.C, a.sumk, a.clipv, a.lim = L, N, A, 5 * A, sumk, float(clip), lim.data_ptr()
    a.boxes, a.scores, a.idx, a.box_reg = boxes.data_ptr(), scores.data_ptr(), idx.data_ptr(), reg.data_ptr()
    _check(lib().mmt_rpn_gather_decode(ctypes.byref(a), _stream()), "mmt_rpn_gather_decode")
    return boxes, scores, idx, reg, offs


def rpn_post_select(boxes, scores, idx, reg, keep, keep_cnt, level_off, own_pre, post_n, fpn_post_n, training, cap,
                    gt=None, gt_off=None, min_size_filter=False, zero_tails=False):
    """include/mmtpsm.h: mmt_rpn_post_select -> (out_boxes (N,cap,4), out_scores, out_idx, out_reg, out_level, out_cnt (N,))"""
    N, sumk = scores.shape
    L = len(level_off) - 1
    dev = boxes.device
    a = RpnPostArgs()
    a.boxes, a.scores, a.idx, a.box_reg = boxes.data_ptr(), scores.data_ptr(), idx.data_ptr(), reg.data_ptr()
    a.keep, a.keep_cnt = keep.data_ptr(), keep_cnt.data_ptr()
    for l in range(L + 1):
        a.seg_off[l] = level_off[l]
    for l in range(L):
        a.own_pre[l] = own_pre[l]
    a.L, a.N, a.sumk, a.kmax = L, N, sumk, keep.shape[1]
    a.post_n, a.fpn_post_n, a.training, a.cap = int(post_n), int(fpn_post_n), 1 if training else 0, int(cap)
    a.min_size_filter = 1 if min_size_filter else 0
    if gt is not None:
        a.gt, a.gt_off = gt.data_ptr(), gt_off.data_ptr()
    ob = (torch.zeros if zero_tails else torch.empty)((N, cap, 4), dtype=torch.float32, device=dev)
    osc = (torch.zeros if zero_tails else torch.empty)((N, cap), dtype=torch.float32, device=dev)
    oi = torch.empty((N, cap), dtype=torch.int64, device=dev)
    orr = torch.empty((N, cap, 4), dtype=torch.float32, device=dev)
    ol = torch.empty((N, cap), dtype=torch.int32, device=dev)
    oc = torch.empty((N,), dtype=torch.int32, device=dev)
    a.out_boxes, a.out_scores, a.out_idx, a.out_reg = ob.data_ptr(), osc.data_ptr(), oi.data_ptr(), orr.data_ptr()
    a.out_level, a.out_cnt = ol.data_ptr(), oc.data_ptr()
    scratch = torch.empty((N * L * (keep.shape[1] + 1),), dtype=torch.int64, device=dev)
    a.key_scratch = scratch.data_ptr()
    _check(lib().mmt_rpn_post_select(ctypes.byref(a), _stream()), "mmt_rpn_post_select")
    return ob, osc, oi, orr, ol, oc


SAMPLE_WIDE = True            # long label vectors (the RPN's 262 k anchors per image) take the many-blocks-wide form of the sampler,
SAMPLE_WIDE_MIN = 32768       # short ones (the box head's proposals) the one-block-per-image kernel: same masks bit for bit (tests)
_SAMPLE_WS = {}


def _sample_ws_bytes(n_img):
    b = _SAMPLE_WS.get(n_img)
    if b is None:
        fn = lib().mmt_sample_fg_bg_workspace_bytes
        fn.restype, fn.argtypes = ctypes.c_long, [c_int]
        b = _SAMPLE_WS[n_img] = int(fn(n_img))
    return b


def sample_fg_bg(labels, keys, off, batch_size_per_image, max_pos):
    """labels (float32 or int64, concatenated over images), keys (float32 uniform), off int32 (n_images + 1,) ->
    pos_mask, neg_mask (bool), counts (n_images, 2) int32 (include/mmtpsm.h: mmt_sample_fg_bg)"""
    _dev(labels, "labels")
    n_img = off.numel() - 1
    if labels.dtype not in (torch.float32, torch.int64):
        raise RuntimeError("sample_fg_bg: labels must be float32 or int64")
    labels, keys = labels.contiguous(), keys.contiguous()
    pm = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    nm = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    cnt = torch.empty((n_img, 2), dtype=torch.int32, device=labels.device)
    if SAMPLE_WIDE and labels.numel() >= SAMPLE_WIDE_MIN * n_img and n_img <= 64:
        # long vectors (the RPN's anchors): the streaming passes many blocks wide, the exact select per image (four launches,
        # same result bit for bit); labels.numel() bounds every image's length
        ws = torch.empty((_sample_ws_bytes(n_img) // 8,), dtype=torch.int64, device=labels.device)
        _check(lib().mmt_sample_fg_bg_wide(_p(labels), 1 if labels.dtype == torch.float32 else 0, _p(keys), _p(off), n_img,
                                           labels.numel(), int(batch_size_per_image), int(max_pos), _p(pm), _p(nm), _p(cnt), _p(ws),
                                           _stream()), "mmt_sample_fg_bg_wide")
        return pm.view(torch.bool), nm.view(torch.bool), cnt
    _check(lib().mmt_sample_fg_bg(_p(labels), 1 if labels.dtype == torch.float32 else 0, _p(keys), _p(off), n_img,
                                  int(batch_size_per_image), int(max_pos), _p(pm), _p(nm), _p(cnt), _stream()), "mmt_sample_fg_bg")
    return pm.view(torch.bool), nm.view(torch.bool), cnt


def box_decode(codes, boxes, weights, clip, row_off=None, lim=None):
    """BoxCoder.decode (+ clip_to_image when row_off / lim are given) in one launch; codes (R, ncls*4), boxes (R, 4)"""
    _dev(codes, "codes")
    codes, boxes = codes.contiguous(), boxes.contiguous().to(torch.float32)
    R, ncls = codes.shape[0], codes.shape[1] // 4
    out = torch.empty_like(codes)
    n_img = 0 if lim is None else lim.shape[0]
    _check(lib().mmt_box_decode(_p(codes), _p(boxes), R, ncls, float(weights[0]), float(weights[1]), float(weights[2]),
                                float(weights[3]), float(clip), _p(row_off), _p(lim), n_img, _p(out), _stream()), "mmt_box_decode")
    return out


# ------------------------------------------------------------------------------------------ conv
def _conv_out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def _conv_shape(a, N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo):
    """the shape half of a mmt_conv_args (everything else in a fresh block is null / zero)"""
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW = N, H, W, Cin, Cout, KH, KW
    a.stride, a.pad, a.Ho, a.Wo = stride, pad, Ho, Wo
    a.out_stride, a.mask_scale = 1, 1.0
    return a


def _weight_dims(Cin, w_shape):
    Cout, Cin_w, KH, KW = w_shape
    if Cin_w != Cin:
        raise RuntimeError("conv channel mismatch: x has %d, w has %d" % (Cin, Cin_w))
    return Cout, KH, KW


def split_planes(x, out=None):
    """x (dense fp32, numel % 8 == 0) -> (3, numel) bf16 planes with x = p0 + p1 + p2 (include/mmtpsm.h: mmt_split_planes)"""
    n = x.numel()
    if out is None:
        out = torch.empty((3, n), dtype=torch.bfloat16, device=x.device)
    _check(lib().mmt_split_planes(x.data_ptr(), out.data_ptr(), out.stride(0), n, _stream()), "mmt_split_planes")
    return out


def conv_route(a, entry, assume=0):
    """which kernel the library runs the call with the argument block `a` on, and its plan (include/mmtpsm.h: mmt_conv_route): entry =
    ENTRY_LIB (mmt_conv_forward's dispatch in the current mode) or ENTRY_F16 (the two-term fp16 split's three launches); assume: ASSUME_*
    bits for operands the block lacks and the caller supplies before the launch.  A query: not counted, not recorded."""
    r = ConvRoute()
    code = lib().mmt_conv_route(ctypes.byref(a), entry, assume, ctypes.byref(r))
    if code != 0:
        raise RuntimeError("mmt_conv_route failed with code %d" % code)
    return r


def planes_wanted_3x3(N, C, H, W, Cout):
    """would a 3x3 / stride 1 / pad 1 convolution (C -> Cout) over an (N, C, H, W) tensor run on the all-planes kernel?
    (asked by the PRODUCER of that tensor, which then writes the planes from its epilogue: conv_forward(want_planes=True))"""
    if get_conv_precision() != 3 or F16X2:   # (on the fp16 split no epilogue writes bf16 planes: consumers scale
        return False                                              # the tensor themselves, conv_forward ignores the request)
    a = _conv_shape(ConvArgs(), N, H, W, C, Cout, 3, 3, 1, 1, H, W)
    return conv_route(a, ENTRY_LIB, ASSUME_X | ASSUME_W_PLANES | ASSUME_X_PLANES).family == ROUTE_STRIP


# ---- launch plans of the default arithmetic.  The step is bound by the interpreter time of its launch-issuing threads
# (DESIGN.md section 5), and most of conv_forward's is spent re-deriving what never changes for a call site: shapes, the kernel
# family, the static half of mmt_conv_args.  The first call of a (weight, input shape, epilogue form) on the fp16 split leaves
# a PLAN -- the filled argument block and the path taken; later calls copy the block, patch the pointers and launch.  Anything
# unusual (profiling, bf16 storage, explicit planes / outputs, a site that fell back to the 3-term bf16 split) takes the
# general path below; a plan is tied to the weight OBJECT (addresses are re-used) and to the mode epoch.
_PLAN = {}
_WPLAN = {}   # weight gradient: (shapes, stride, pad, dtypes, what the caller holds, arithmetic, switch mask) -> (shape half of mmt_conv_args, route)
_PLAN_EPOCH = [0]
FAST_PLANS = True
# the path of a convolution call: the library's own dispatch (fp32 MFMA, bf16, the bf16 splits), or the two-term fp16 split on the
# tiled / row-resident kernels (x split in registers), on the tap-strip kernel, on the plane-fed implicit GEMM (x as fp16 planes)
K_LIB, K_TILED, K_STRIP, K_PG = -1, 0, 1, 2
_F16_STAT = {K_TILED: "tiled", K_STRIP: "conv", K_PG: "pg"}
_KIND_OF = {ROUTE_STRIP: K_STRIP, ROUTE_PG: K_PG}   # the route's family -> the kind (every other family: K_TILED)


def _conv_kind(a, x, w, f16_src, io, y_out, prec):
    """which path the call with the argument block `a` (x, the weight or its planes, the shape, the output stride and `mul` filled in)
    takes -> (kind, is the shape one of the tap-strip kernel's, the fp16 split's weight source (tensor, flipped?, row scale) or None).
    ONE question to the library's route (planes of x and the fp16 scalars promised: they are made once the kind is known) answers
    everything about shapes, strides and epilogue forms; what only this side knows is the arithmetic (F16X2, bf16 storage, the mode),
    an explicit output tensor, a missing weight source and the site's verdict: a site whose input defeats fp16 (lagged crest-factor
    test, counted in F16_STATS["fallback"]) stays on the library's 3-term bf16 split."""
    if F16X2 and not io and prec == 3 and y_out is None and (w is not None or f16_src is not None):
        r = conv_route(a, ENTRY_F16, ASSUME_X_PLANES | ASSUME_F16_SCALARS)
        strip = r.strip_tw != 0
        if r.family != ROUTE_NONE:
            src = (w, False, None) if w is not None else (nhwc(f16_src[0]), True, f16_src[1])
            if _site_ok((src[0].data_ptr(), src[1]), x):
                return _KIND_OF.get(r.family, K_TILED), strip, src
        return K_LIB, strip, None
    # would the library's own dispatch run this call on the tap-strip kernel, given planes of x?  (mode 3, fp32 tensors)
    strip = prec == 3 and not io and conv_route(a, ENTRY_LIB, ASSUME_X_PLANES).family == ROUTE_STRIP
    return K_LIB, strip, None


def _ev():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _profiled(a, e0, tag, ksplit, pre, ebytes):
    """closes the bracket e0 = _ev() opened around a launch of the block `a`: one PROFILE record (bench.py, tools/conv_table.py) --
    (algorithmic FLOPs, start, stop, (tag, shape ...), K split, the event pair around the launch's pre-pass or None, the bytes of the
    fused epilogue's operands)"""
    PROFILE.append((2.0 * a.N * a.Ho * a.Wo * a.Cout * a.Cin * a.KH * a.KW, e0, _ev(),
                    (tag, a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.stride, a.out_stride), ksplit, pre, ebytes))


def _conv_f16(a, kind, x, src, y, slot, rb_site, tile_rows=0, ksplit=0, xp=None, prof=None, counted=True):
    """THE launch of the two-term fp16 split: `a` holds the shape, x, y and the epilogue; src = (weight, flipped?, row scale) names the
    weight planes; slot: the statistics slot y's maximum goes to (a.y_amax) or None; rb_site: None, or the producing site whose
    row-blocked planes of y this launch's epilogue writes (_rb_produce, asked with the block filled: the weight pointer, the mask and
    the residual mode decide whether the kernel the launch takes has the plane store); tile_rows /
    ksplit / xp = (planes, scale[, layout, lag]): conv_forward_pg's overrides; prof: None, or the fused epilogue's bytes -- the
    launch is bracketed for PROFILE (the strip and plane-fed kinds with their input pass in a bracket of its own; the tiled kind
    only where it runs the dominant 128 x 128 kernel, unless PROFILE_ALL); counted: F16_STATS counts what the DISPATCHER sent to a
    kind (conv_forward and its plans), not the explicit conv_forward_pg of tools and tests"""
    wsrc, flipped, fscale = src
    e0 = _ev() if prof is not None and kind != K_TILED else None
    amax, a.f16_guard_x = _stat_ptrs(_amax_of(x))
    # the fp32 weights for the kernels' slow, exact path (a tensor whose range defeats fp16: decided per block on the device)
    if flipped:
        a.w_src, a.w_src_scale = wsrc.data_ptr(), _p(fscale)
    else:
        a.w = wsrc.data_ptr()
    wp16, sw = f16_weight_planes(wsrc, fscale, flipped)
    a.w_planes, a.w_plane_stride = wp16.data_ptr(), wp16.stride(0)
    yrb = _rb_produce(a, y, rb_site) if rb_site is not None else None
    if counted:
        F16_STATS[_F16_STAT[kind]] += 1
    if kind == K_TILED:   # x is split in registers, its recorded maximum gives the scale
        pre = None
        if prof is not None:
            r = conv_route(a, ENTRY_F16, ASSUME_F16_SCALARS)
            if PROFILE_ALL or r.tag == 1:
                tag, ks, e0 = "fwd%d" % r.tag, r.ksplit, _ev()
        _check(lib().mmt_conv_forward_f16x2(ctypes.byref(a), amax, sw.data_ptr(), _stream()), "mmt_conv_forward_f16x2")
    else:                 # x's planes (its producer's, or one split pass), then the launch
        xp16, sx, a.x_planes_layout, a.x_planes_lag = f16_split_pg(x) if xp is None else (tuple(xp) + (0, 0))[:4]
        a.x_planes, a.x_plane_stride = xp16.data_ptr(), xp16.stride(0)
        if e0 is not None:
            pre, tag, ks, e0 = (e0, _ev()), "fwd5" if kind == K_PG else "fwd4", 1, _ev()
        if kind == K_PG:
            _check(lib().mmt_conv_forward_pg(ctypes.byref(a), sx.data_ptr(), sw.data_ptr(), tile_rows, ksplit, _stream()),
                   "mmt_conv_forward_pg")
        else:
            _check(lib().mmt_conv3x3_strip_f16x2(ctypes.byref(a), sx.data_ptr(), sw.data_ptr(), _stream()), "mmt_conv3x3_strip_f16x2")
    if e0 is not None:
        _profiled(a, e0, tag, ks, pre, prof)
    if slot is not None:
        _record(y, slot)
    if yrb is not None:   # (y's row-blocked planes came out of this launch's epilogue)
        _rb_attach(y, yrb[0], yrb[1], "epi", yrb[2])
    return y


def _plan_key(x, w, f16_src, stride, pad, relu, res, res_mode, mask):
    src = w if w is not None else (f16_src[0] if f16_src is not None else None)
    if src is None:
        return None, None, None
    base = src._base   # a reshaped view of a parameter (Linear: a fresh (O, K, 1, 1) view per call) stands for the parameter
    return ((src.data_ptr(), w is None, x.shape, stride, pad, relu, res_mode, res is not None, mask is not None, src.shape,
             _PLAN_EPOCH[0]), src, src if base is None else base)


def _conv_fast(x, w, scale, shift, stride, pad, relu, res, res_mode, mask, mask_scale, f16_src, rb_site=None):
    key, src, owner = _plan_key(x, w, f16_src, stride, pad, relu, res, res_mode, mask)
    plan = _PLAN.get(key) if key is not None else None
    if plan is None:
        return None
    tmpl, kind, Cout, Ho, Wo, wref = plan
    if wref() is not owner or x.dtype != torch.float32 or (res is not None and res.dtype != torch.float32) or (
            mask is not None and mask.dtype != torch.float32):
        return None
    x = nhwc(x)
    flipped = w is None
    wsrc = nhwc(src)
    if not _site_ok((wsrc.data_ptr(), flipped), x, count=False):
        return None   # (the general path asks again, counts the fall-back and runs the 3-term bf16 split for this site)
    a = ConvArgs.from_buffer_copy(tmpl)
    y = torch.empty((x.shape[0], Cout, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    a.x, a.y = x.data_ptr(), y.data_ptr()
    a.scale, a.shift = _p(scale), _p(shift)
    if res is not None:
        a.res = nhwc(res).data_ptr()
    if mask is not None:
        a.mask, a.mask_scale = nhwc(mask).data_ptr(), float(mask_scale)
    if a.KH == 3:
        # the library's choice between the strip, plane-fed and tiled kernels can be switched per call (MMT_STRIP, MMT_PG): the
        # question _conv_kind asked (the weight planes are made for the launch below)
        r = conv_route(a, ENTRY_F16, ASSUME_W_PLANES | ASSUME_X_PLANES | ASSUME_F16_SCALARS)
        if _KIND_OF.get(r.family, K_TILED) != kind:
            return None   # re-plan
    slot = _amax_slot(x.device)
    a.y_amax = slot.ptr
    return _conv_f16(a, kind, x, (wsrc, flipped, f16_src[1] if flipped else None), y, slot, rb_site)


def _plan_record(x, w, f16_src, stride, pad, relu, res, res_mode, mask, a, kind, Cout, Ho, Wo):
    key, src, owner = _plan_key(x, w, f16_src, stride, pad, relu, res, res_mode, mask)
    if key is None:
        return
    t = ConvArgs.from_buffer_copy(a)
    # every pointer is cleared in the template (a stale one must never survive into a launch), and what a call sets with them
    for name, typ in ConvArgs._fields_:
        if typ is c_void_p:
            setattr(t, name, None)
    t.w_plane_stride = t.x_plane_stride = t.y_plane_stride = t.x_planes_layout = t.y_rb_stride = t.x_planes_lag = t.y_rb_rows = 0
    t.mask_scale, t.io_bf16, t.y_amax_stats = 1.0, 0, 1
    if len(_PLAN) > 4096:
        _PLAN.clear()
    _PLAN[key] = (bytes(t), kind, Cout, Ho, Wo, weakref.ref(owner))


def _epilogue_bytes(y, res, res_mode, mask, mul):
    """HBM bytes of the operands a fused epilogue reads besides the convolution's own input / weights (profiling records: the
    algorithmic traffic of a launch is input + weights + output + THESE, each once): the residual (same pixels, the coarser map of
    the FPN top-down add, or the four finer pixels of its gradient), the ReLU mask of a data gradient, the dropout multiplier"""
    n = 0
    if res is not None:
        n += res.numel() * res.element_size() if res_mode in (1, 2, 3) else 0
    if mask is not None:
        n += y.numel() * mask.element_size()
    if mul is not None:
        n += mul.numel() * mul.element_size()
    return n


def conv_forward(x, w, scale=None, shift=None, stride=1, pad=0, relu=False, res=None, res_mode=0,
                 mask=None, mask_scale=1.0, mul=None, out_stride=1, out_hw=None, y_out=None, y_offset=0,
                 w_shape=None, planes=None, out_size=None, x_planes=None, want_planes=False, out_dtype=None, f16_src=None,
                 rb_site=None):
    """x (N,Cin,H,W) NHWC-dense; w (Cout,Cin,KH,KW) channels_last-dense ([Cout][KH][KW][Cin] memory).
    y_out/y_offset (elements): write into an existing NHWC tensor at a shifted base (transposed-conv taps).
    w=None with w_shape + planes: the weight exists only as packed bf16 planes (pack_weight_flipped).
    out_size=(Ho, Wo): fewer output rows / columns than `pad` on both sides would give, i.e. a smaller pad at the
    bottom / right (taps that fall outside the input read zeros either way).
    bf16 storage (mode 1): a bf16 `x`, `res`, `mask` is taken as it is; out_dtype=torch.bfloat16 makes y a bf16 tensor."""
    fast_ok = (FAST_PLANS and F16X2 and PROFILE is None and y_out is None and mul is None and out_stride == 1 and x_planes is None
               and out_size is None and (out_dtype is None or out_dtype is torch.float32) and _PREC == 3)
    if fast_ok:
        y = _conv_fast(x, w, scale, shift, stride, pad, relu, res, res_mode, mask, mask_scale, f16_src, rb_site)
        if y is not None:
            return y
    if x_planes is None:
        x_planes = planes_of(x)
    x = nhwc(x)
    N, Cin, H, W = x.shape
    io = IO_X if x.dtype == torch.bfloat16 else 0
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if y_out is not None:
        out_dtype = y_out.dtype
    if out_dtype == torch.bfloat16:
        io |= IO_Y
    esz = 2 if out_dtype == torch.bfloat16 else 4
    if w is not None:
        w = nhwc(w)
    Cout, KH, KW = _weight_dims(Cin, w_shape if w is None else w.shape)
    Ho, Wo = _conv_out_hw(H, W, KH, KW, stride, pad)
    if out_size is not None and w is not None:
        if out_size[0] > Ho or out_size[1] > Wo or out_stride > 1:
            raise RuntimeError("conv_forward: out_size can only trim the output")
        Ho, Wo = out_size
    a = _conv_shape(ConvArgs(), N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo)
    a.x = x.data_ptr()
    if w is None:
        a.w_planes, a.w_plane_stride = planes.data_ptr(), planes.stride(0)
        # data-gradient planes of a flat model's weight: deferred like the forward planes
        planes_owner = _flat_form(f16_src[0], None)[0] if f16_src is not None else None
    else:
        a.w = w.data_ptr()
        _keep, planes_owner = _weight_planes(w, a)  # noqa: F841  (keeps a per-call plane buffer alive until the launch is queued)
    if out_stride > 1:
        oh, ow = out_hw
        y = y_out if y_out is not None else empty_nhwc(N, Cout, oh, ow, x.device, zero=True, dtype=out_dtype)
        a.out_stride, a.out_H, a.out_W = out_stride, oh, ow
    else:
        y = y_out if y_out is not None else empty_nhwc(N, Cout, Ho, Wo, x.device, dtype=out_dtype)
    a.y = y.data_ptr() + esz * int(y_offset)
    prec = get_conv_precision()
    io_xy = io   # (bf16 storage of x / y: what the arithmetic goes by)
    want_amax = bool(F16X2 and not io_xy and prec == 3)
    a.scale, a.shift = _p(scale), _p(shift)
    a.relu = 1 if relu else 0
    if res is not None:
        res = nhwc(res)
        a.res, a.res_mode = res.data_ptr(), res_mode
        if res.dtype == torch.bfloat16:
            io |= IO_RES
    if mask is not None:
        mask = nhwc(mask)
        a.mask, a.mask_scale = mask.data_ptr() + mask.element_size() * int(y_offset), float(mask_scale)
        if mask.dtype == torch.bfloat16:
            io |= IO_MASK
    a.io_bf16 = io
    if mul is not None:
        mul = nhwc(mul)
        a.mul = mul.data_ptr()
    kind, strip, src = _conv_kind(a, x, w, f16_src, io_xy, y_out, prec)
    if want_amax:
        want_planes = False   # consumers on the fp16 split scale y themselves: no bf16 planes from this epilogue, max |y| recorded on the way
    if kind != K_LIB:
        x_planes = None       # (the fp16 kinds split x in registers or read fp16 planes of their own)
    y_planes = None
    if want_planes and out_stride == 1 and y_out is None and Cout % 4 == 0 and not io_xy:
        y_planes = torch.empty((3, y.numel()), dtype=torch.bfloat16, device=x.device)
        a.y_planes, a.y_plane_stride = y_planes.data_ptr(), y_planes.stride(0)
    auto_split = x_planes is None and strip and kind == K_LIB
    if auto_split:
        # one pass over x; the 3x3 kernel then reads bf16 planes (9 taps x Cout/128 re-reads).  Allocated here, filled
        # below INSIDE the profiling bracket: the pass is part of this convolution's cost
        x_planes = torch.empty((3, x.numel()), dtype=torch.bfloat16, device=x.device)
    if x_planes is not None:
        a.x_planes, a.x_plane_stride = x_planes.data_ptr(), x_planes.stride(0)
    amax_slot = None
    if want_amax and not io and y_out is None and out_stride == 1:
        amax_slot = _amax_slot(x.device)
        a.y_amax, a.y_amax_stats = amax_slot.ptr, 1
    ebytes = _epilogue_bytes(y, res, res_mode, mask, mul) if PROFILE is not None else None
    if kind != K_LIB:
        if fast_ok and not io:
            _plan_record(x, w, f16_src, stride, pad, relu, res, res_mode, mask, a, kind, Cout, Ho, Wo)
        if amax_slot is None or mul is not None:
            rb_site = None   # (y's row-blocked planes come out of an epilogue that also records max |y|, see f16_split_pg)
        # (a, kind, x, src, y, slot, rb_site, tile_rows, ksplit, xp, prof = the epilogue's bytes when PROFILE is on)
        return _conv_f16(a, kind, x, src, y, amax_slot, rb_site, 0, 0, None, ebytes)
    r = conv_route(a, ENTRY_LIB) if ebytes is not None else None
    rec = r is not None and (r.tag in (1, 4) or PROFILE_ALL)
    pre = None
    if auto_split:   # the plane-split pass of the input (when no producer wrote the planes): its own bracket
        p0 = _ev() if rec else None
        split_planes(x, x_planes)
        if rec:
            pre = (p0, _ev())
    e0 = _ev() if rec else None
    if planes_owner is not None:
        planes_owner.ensure_bf16()
    _check(lib().mmt_conv_forward(ctypes.byref(a), _stream()), "mmt_conv_forward")
    if rec:
        _profiled(a, e0, "fwd%d" % r.tag, 1 if r.tag == 4 else r.ksplit, pre, ebytes)   # (K ranges of the tiled kernels, as ever)
    if y_planes is not None:
        _planes_attach(y, y_planes)
    if amax_slot is not None:
        _record(y, amax_slot)
    return y


def conv_forward_pg(x, w, scale=None, shift=None, stride=1, pad=0, relu=False, res=None, mask=None, mask_scale=1.0, w_shape=None,
                    f16_src=None, tile_rows=0, ksplit=0, xp=None):
    """the plane-fed implicit GEMM of the default arithmetic (include/mmtpsm.h: mmt_conv_forward_pg; csrc/conv_pgemm.hip): x is split
    into its two fp16 planes by one pass (or `xp` = (planes, scale) from an earlier call on the same tensor), the weight planes are
    the packed fp16 planes of `w` -- or, `w` None with `w_shape` and `f16_src` = (forward weight, row scale), of its data-gradient
    form.  tile_rows / ksplit: 0 = the library's choice.  Raises for shapes the kernel does not take."""
    x = nhwc(x)
    N, Cin, H, W = x.shape
    src = (nhwc(w), False, None) if w is not None else (nhwc(f16_src[0]), True, f16_src[1])
    Cout, KH, KW = _weight_dims(Cin, src[0].shape if w is not None else w_shape)
    Ho, Wo = _conv_out_hw(H, W, KH, KW, stride, pad)
    a = _conv_shape(ConvArgs(), N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo)
    a.x = x.data_ptr()
    y = empty_nhwc(N, Cout, Ho, Wo, x.device)
    a.y = y.data_ptr()
    a.scale, a.shift, a.relu = _p(scale), _p(shift), 1 if relu else 0
    if res is not None:
        a.res, a.res_mode = nhwc(res).data_ptr(), 1
    if mask is not None:
        a.mask, a.mask_scale = nhwc(mask).data_ptr(), float(mask_scale)
    slot = _amax_slot(x.device)
    a.y_amax, a.y_amax_stats = slot.ptr, 1
    # (a, kind, x, src, y, slot, rb_site, tile_rows, ksplit, xp, prof, counted)
    return _conv_f16(a, K_PG, x, src, y, slot, None, int(tile_rows), int(ksplit), xp, None, False)


def stem_fused(x, w_s2d, scale, shift):
    """conv 7x7 / 2 + FrozenBN + ReLU + max pool 3x3 / 2 of the ResNet stem in one launch (include/mmtpsm.h: mmt_stem_fused).
    x (N, 3, H, W) fp32 NCHW-contiguous with H, W multiples of 4; w_s2d the (64, 16, 4, 4) channels_last space-to-depth filter
    (modeling/backbone/backbone.py: StemWithFixedBatchNorm._s2d_weight).  -> (N, 64, H / 4, W / 4) channels_last, statistics attached."""
    _dev(x)
    N, C, Hh, W = x.shape
    if C != 3 or not x.is_contiguous() or x.dtype != torch.float32 or (Hh & 3) or (W & 3) or tuple(w_s2d.shape) != (64, 16, 4, 4):
        raise RuntimeError("stem_fused: (N, 3, H, W) fp32 NCHW with H, W % 4 == 0 and the 64 x 16 x 4 x 4 space-to-depth filter")
    w = nhwc(w_s2d)
    am = _amax_of(x)
    if not _full_slot(am[0]):
        raise RuntimeError("stem_fused: the input needs a full statistics slot")
    wp16, sw = f16_weight_planes(w)
    y = empty_nhwc(N, 64, Hh // 4, W // 4, x.device)
    slot = _amax_slot(x.device)
    _check(lib().mmt_stem_fused(x.data_ptr(), N, Hh, W, w.data_ptr(), wp16.data_ptr(), wp16.stride(0), sw.data_ptr(), _p(scale), _p(shift),
                                am[0].ptr, y.data_ptr(), slot.ptr, _stream()), "mmt_stem_fused")
    _record(y, slot)
    return y


C64_FUSE = os.environ.get("MMT_C64_FUSE", "1") != "0"   # a frozen layer1 block's conv2 + conv3 as one launch (A/B timing, parity tests: 0)


def o2_site(w3):
    """the producing site of a layer1 block's o2 (conv2's output): keyed by the weight that consumes it"""
    return ("o2", w3.data_ptr())


def c64_fuse_enabled():
    """do the process's switches and arithmetic allow the fused launch at all?  (Only then does conv2 of a frozen layer1 block record
    o2's maximum at its site on the two-launch path: a site that becomes ready with the fused launch switched off -- MMT_C64=0, a
    profiling leg -- would make conv2 write planes of o2 that nobody reads)"""
    return bool(C64_FUSE and F16X2 and RB_EPI and PROFILE is None and os.environ.get("MMT_C64") != "0" and get_conv_precision() == 3)


def out_site(w1_next):
    """the site of a layer1 block's `out` in its role as the operand of the NEXT block's conv1: keyed by that weight"""
    return ("out1", w1_next.data_ptr())


def c64_conv3_fused(x, w2, scale2, shift2, w3, scale3, shift3, res, o2_amax=None, nxt=None, out_amax=None):
    """conv2 (3x3, 64 -> 64, FrozenBN, ReLU) and conv3 (1x1, 64 -> 256, FrozenBN, + res, ReLU) of a layer1 bottleneck in one launch
    (include/mmtpsm.h: mmt_c64_conv3_fused); o2 never reaches memory.  -> out with its statistics attached, or None when this is not
    a call for the fused launch -- other shapes / arithmetic, a site without a scale yet (its first step: the two launches record the
    maximum the scale is folded from, `rb_site=o2_site(w3)` on conv2) -- and the caller takes the two launches.
    nxt = (w1, scale1, shift1) of the NEXT block (256 -> 64, stride 1): its conv1 runs behind conv3 in the same launch -> (out, o1_next);
    o1_next is None while the site of `out` as that operand has no scale yet (this launch then records the maximum it is folded from).
    o2_amax / out_amax (tests): device maxima of |o2| / |out| to derive the scales from, as the un-fused chain does, instead of the
    sites' lagged scales."""
    if not c64_fuse_enabled():
        return None
    N, C, Hh, W = x.shape
    if (C != 64 or tuple(w2.shape) != (64, 64, 3, 3) or tuple(w3.shape) != (256, 64, 1, 1) or tuple(res.shape) != (N, 256, Hh, W)
            or x.dtype != torch.float32 or res.dtype != torch.float32 or N * Hh * W >= (1 << 21) or N * Hh * W == 0):
        return None
    if nxt is not None and tuple(nxt[0].shape) != (64, 256, 1, 1):
        return None
    site = o2_site(w3)
    x, res, w2, w3 = nhwc(x), nhwc(res), nhwc(w2), nhwc(w3)
    if not _site_ok((w2.data_ptr(), False), x, count=False):
        return None   # (the lagged crest-factor test sent conv2's site to the 3-term bf16 split)
    pend = None
    if o2_amax is None:
        s = _rb_site(site, x.device)
        if s is None or not s.ready:
            return None
        sc, pend = s.scale, s.produce()
    else:
        sc = o2_amax.data_ptr()
    am = _amax_of(x)
    if not _full_slot(am[0]):
        return None
    wp2, sw2 = f16_weight_planes(w2)
    wp3, sw3 = f16_weight_planes(w3)
    out = empty_nhwc(N, 256, Hh, W, x.device)
    slot = _amax_slot(x.device)
    # the next block's conv1: its operand's site must have a scale (else this launch only records max |out| there)
    nx = [None] * 10   # out_amax_next, w1, w1_planes, stride, s_w1, scale1, shift1, out_scale, o1_next, o1_next_slot
    nx[3] = 0
    o1n = nslot = None
    if nxt is not None:
        w1 = nhwc(nxt[0])
        go = True
        if out_amax is None:
            s1 = _rb_site(out_site(nxt[0]), x.device)
            go = s1 is not None and o2_amax is None
            if go:
                nx[0] = s1.produce()
                go, osc = s1.ready, s1.scale
        else:
            go, osc = o2_amax is not None, out_amax.data_ptr()
        ent = _SITES.get((w1.data_ptr(), False))   # (the host's lagged crest-factor verdict on the next conv1's site, if any)
        if go and (ent is None or ent[0]):
            wp1, sw1 = f16_weight_planes(w1)
            o1n = empty_nhwc(N, 64, Hh, W, x.device)
            nslot = _amax_slot(x.device)
            nx[1:] = [w1.data_ptr(), wp1.data_ptr(), wp1.stride(0), sw1.data_ptr(), _p(nxt[1]), _p(nxt[2]), osc, o1n.data_ptr(), nslot.ptr]
            F16_STATS["c64_fused_next"] = F16_STATS.get("c64_fused_next", 0) + 1
    F16_STATS["c64_fused"] = F16_STATS.get("c64_fused", 0) + 1
    _check(lib().mmt_c64_conv3_fused(x.data_ptr(), N, Hh, W, w2.data_ptr(), wp2.data_ptr(), wp2.stride(0), sw2.data_ptr(), _p(scale2),
                                     _p(shift2), am[0].ptr, w3.data_ptr(), wp3.data_ptr(), wp3.stride(0), sw3.data_ptr(), _p(scale3),
                                     _p(shift3), res.data_ptr(), out.data_ptr(), slot.ptr, sc, 0 if o2_amax is None else 1, pend,
                                     *nx, _stream()), "mmt_c64_conv3_fused")
    _record(out, slot)
    if nxt is None:
        return out
    if o1n is not None:
        _record(o1n, nslot)
    return out, o1n


def conv_pg_plan(N, Cin, H, W, Cout, KH, KW, stride, pad):
    """(tile rows, K ranges) the library would run this shape with on the plane-fed kernel; (0, 0): not one of its shapes"""
    Ho, Wo = _conv_out_hw(H, W, KH, KW, stride, pad)
    a = _conv_shape(ConvArgs(), N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo)
    r = conv_route(a, ENTRY_F16, ASSUME_X | ASSUME_W_PLANES | ASSUME_X_PLANES | ASSUME_F16_SCALARS)
    return (r.pg_rows, r.pg_ksplit) if N * Ho * Wo > 0 else (0, 0)


# ---- who owns the derived forms of a weight (what a convolution reads instead of the weight: packed bf16 / fp16 planes of the
# forward and the data-gradient matrix, the flipped fp32 tensor).  A parameter of a flattened model: its FlatParams, found by the
# weight's address -- a Linear weight arrives as a fresh view every call, a backward pass sees new objects -- in FLATS, whose
# values are weak: an entry goes when its owner dies; FlatParams.form alone decides what is current (the invariants are stated
# there).  Anything else -- also a flat model's parameter written through torch since the last refresh -- : LOOSE, by the identity of
# the tensor object.  An entry holds a weak reference to its owner, is removed when the owner dies and is served only to that very
# object: neither an id nor an address that comes back can hit.  One validity rule: `_loose_stamp` and the identity of the scale
# vector.  Raw-pointer writes (sgd_momentum, ema_update) announce their bytes: `forget`.
FLATS = weakref.WeakValueDictionary()   # address of a packed weight matrix -> the FlatParams that holds it (engine/flat.py puts them)
GRAD_SLOTS = {}  # address of a parameter's slot in a flat gradient buffer -> (weakref FlatParams, parameter name); engine/flat.py
PLANES_EPOCH = 0  # THE counter of the arithmetic mode, bumped by set_conv_precision: nothing packed before a mode switch is trusted
                  # afterwards (steps taken in mode 0 do not refresh the planes)


def _flat_form(w, form, scale=None):
    """-> (the live FlatParams whose buffer holds the packed matrix `w`, or None; what it serves for `w` in `form`, or None)"""
    flat = FLATS.get(w.data_ptr())
    return flat, (flat.form(w, form, scale) if flat is not None and form is not None else None)


class _LooseEntry(object):
    __slots__ = ("ref", "stamp", "scale", "served", "lo", "hi", "keep")


class LooseForms(object):
    """derived forms ("f16", "f16_dgrad", "f32_dgrad") of weights no flat buffer vouches for, keyed by (id(owner), form)"""

    def __init__(self):
        self.entries = {}

    def get(self, owner, form, stamp, scale):
        e = self.entries.get((id(owner), form))
        return e.served if e is not None and e.stamp == stamp and e.scale is scale and e.ref() is owner else None

    def put(self, owner, form, stamp, scale, served, src, keep=None):
        """keep `served` for (owner, form); src: the tensor it was derived from (its bytes are what `forget` compares) -> served"""
        key = (id(owner), form)
        e = self.entries.get(key)
        if e is None or e.ref() is not owner:
            # ONE entry and one finalizer per live owner and form: `forget` empties the entry and leaves it in place, so that the
            # next put finds it (a finalizer holds its entry until the owner dies: a popped entry would pin what it served)
            e = self.entries[key] = _LooseEntry()
            e.ref = weakref.ref(owner)
            weakref.finalize(owner, self._drop, key, e)
        e.stamp, e.scale, e.served, e.keep, e.lo = stamp, scale, served, keep, src.data_ptr()
        e.hi = e.lo + src.numel() * src.element_size()
        return served

    def _drop(self, key, e):
        if self.entries.get(key) is e:
            self.entries.pop(key, None)

    def forget(self, t=None):
        """the bytes of `t` were rewritten through raw pointers (no version counter moved): what was derived from them is let go
        (t None: everything)"""
        lo, hi = (0, 1 << 64) if t is None else (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
        # (list of the values: one C call that allocates nothing the collector tracks, so neither the teacher's thread nor a
        # finalizer can change the dict under it)
        for e in list(self.entries.values()):
            if e.lo < hi and lo < e.hi:
                e.stamp = e.scale = e.served = e.keep = None

    def refresh(self, w):
        """`w` -- a weight that is not a parameter of a flattened model -- was rewritten in place: its fp16 planes are re-packed into
        the SAME plane and scale tensors (a recorded launch plan holds their addresses).  Nothing kept for it: nothing to do."""
        e = self.entries.get((id(w), "f16"))
        if e is not None and e.served is not None and e.ref() is w:
            e.keep.zero_()
            _pack_f16(w, None, False, e.served[0], e.keep)
            e.stamp = _loose_stamp(w, None, w)


LOOSE = LooseForms()
refresh_f16_weight_planes = LOOSE.refresh


def _loose_stamp(w, scale, owner, stream=None):
    """what a loose form was packed from and under"""
    # the tensor's version and dimensions, the scale vector's version, the arithmetic counter, the plane generation of the flat buffer
    # its owner is a parameter of (raw-pointer updates of the buffer; engine/flat.py marks every parameter, also those it packs no
    # planes for), and -- the fp32 form only, a plain tensor handed to the next launch; the fp16 planes' addresses sit in recorded
    # plans and stay -- the stream
    ref = getattr(owner, "_flat_ref", None)
    flat = ref() if ref is not None else None
    return (w._version, tuple(w.shape), None if scale is None else scale._version, PLANES_EPOCH,
            None if flat is None else flat.plane_gen, stream)


def packed_elems(cout, k):
    """elements per packed bf16 plane of a [cout][k] weight matrix (include/mmtpsm.h: mmt_packed_weight_elems)"""
    return (k // 16) * ((cout + 31) // 32) * 512


def pack_weight(w):
    """dense fp32 weight (Cout, ...) with K = numel/Cout, K % 16 == 0 -> packed bf16 planes [3, elems]"""
    cout = w.shape[0]
    k = w.numel() // cout
    planes = torch.empty((3, packed_elems(cout, k)), dtype=torch.bfloat16, device=w.device)
    _check(lib().mmt_pack_weight(w.data_ptr(), planes.data_ptr(), planes.stride(0), cout, k, _stream()), "mmt_pack_weight")
    return planes


def pack_weight_flipped(w, scale=None):
    """packed planes of the data-gradient weights of conv(x, w) (* scale[co]) -- or None when the data gradient does not
    run on the DMA-fed kernels (then the caller materialises them with weight_flip_transpose)"""
    Cout, Cin, KH, KW = w.shape
    if get_conv_precision() == 0 or (Cout & 15) or Cin <= 32:
        return None
    w = nhwc(w)
    # A weight is used by several backward passes between two optimiser steps (labeled and unlabeled student pass, the RPN
    # head on five levels): packed once per parameter generation of its flat buffer (engine/flat.py: refresh_planes).
    flat, planes = _flat_form(w, "bf16_dgrad", scale)
    if planes is None:
        planes = torch.empty((3, packed_elems(Cin, KH * KW * Cout)), dtype=torch.bfloat16, device=w.device)
        _check(lib().mmt_pack_weight_flipped(w.data_ptr(), _p(scale), planes.data_ptr(), planes.stride(0), Cout, KH, KW, Cin,
                                             _stream()), "mmt_pack_weight_flipped")
        if flat is not None:
            flat.register("bf16_dgrad", w, scale, planes)
    return planes


def pack_weights(base, planes, descs, unit_desc, n_units):
    _check(lib().mmt_pack_weights(base.data_ptr(), planes.data_ptr(), planes.stride(0), descs.data_ptr(),
                                  unit_desc.data_ptr(), n_units, _stream()), "mmt_pack_weights")


def _weight_planes(w, a):
    """fill a.w_planes / a.w_plane_stride for a dense weight tensor when a split-bf16 mode is on -> (the planes, kept alive until the
    launch is queued; the FlatParams that serves them or None: conv_forward calls its ensure_bf16 before a launch that reads them)"""
    if get_conv_precision() == 0 or (w.shape[1] & 15) or w.shape[0] <= 32:
        return None, None
    flat, pl = _flat_form(w, "bf16")
    if pl is None:
        flat, pl = None, pack_weight(w)
    a.w_planes, a.w_plane_stride = pl.data_ptr(), pl.stride(0)
    return pl, flat


_PREC = None   # the library's mode, mirrored here (asked several times per launch)


def set_conv_precision(mode):
    """0 fp32 MFMA | 1 bf16 | 2 bf16x2 split | 3 bf16x3 split (include/mmtpsm.h: mmt_set_conv_precision)"""
    global PLANES_EPOCH, _PREC
    _check(lib().mmt_set_conv_precision(int(mode)), "mmt_set_conv_precision")
    _PREC = lib().mmt_get_conv_precision()
    PLANES_EPOCH += 1
    _PLAN_EPOCH[0] += 1
    _PLAN.clear()


def get_conv_precision():
    global _PREC
    if _PREC is None:
        _PREC = lib().mmt_get_conv_precision()
    return _PREC


def wgrad_prepare(x, dy):
    """the reduction passes conv_wgrad would take for large operands without a recorded maximum, taken on the CURRENT stream
    (layers/fused.py launches the weight gradient itself on a side stream; a maximum recorded there would race with the
    data-gradient launch that reads it here)"""
    if F16X2 and x.dtype == torch.float32 and dy.dtype == torch.float32 and x.numel() >= WGRAD_F16_MIN_ELEMS and get_conv_precision() == 3:
        _amax_of(nhwc(x))
        _amax_of(nhwc(dy))


def _wgrad_stats(x, dy, dw):
    """the recorded statistics (slot, version) of both operands of a weight gradient on the two-term fp16 split (3 products instead of
    6), or None: not eligible -- an operand nobody recorded a maximum of (big operands, where the saving pays for it, take a
    reduction pass here), or a site whose range defeats fp16 (lagged crest-factor test)"""
    ax, ad = _recorded(x), _recorded(dy)
    if x.numel() >= WGRAD_F16_MIN_ELEMS:
        if ax is None:
            ax = _amax_of(x)
        if ad is None:
            ad = _amax_of(dy)
    if ax is None or ad is None or not (_site_ok(("wgx", dw.data_ptr()), x) and _site_ok(("wgd", dw.data_ptr()), dy)):
        return None
    return ax, ad


def _wgrad_planes(x, dy, guarded):
    """the row-blocked fp16 planes both operands carry for the whole batch -> (x's record, dy's record, lag bits), or None.  Planes a
    producer's epilogue wrote carry a scale fixed beforehand: the kernel's guard tests it (bit 0: x, bit 1: dy), so both guards of the
    operands' statistics must be there (`guarded`)"""
    xr, dr = _rb_of(x), _rb_of(dy)
    if xr is None or dr is None or not (xr.covers() and dr.covers()):
        return None
    lag = (1 if xr.lagged() else 0) | (2 if dr.lagged() else 0)
    if lag and not guarded:
        return None
    return xr, dr, lag


def _wgrad_job(x, dy, w_shape, stride, pad, dw, rowscale, dbias, sw):
    """THE preparation of a weight gradient (x, dy dense NHWC; sw: mmt_conv_switches() of this call or batch) -> (j, r, f16, alive):
    j the filled mmt_wgrad_job (argument block, statistics and guards, the planes when both operands carry them for the whole batch,
    with the lag bits), r its route as a launch of its own, f16: on the two-term fp16 split (the arithmetic the grouped launches
    take), alive: the plane tensors j points to.
    Both operands' maxima make it an fp16-split job (big operands nobody recorded take their reduction pass here); row-blocked
    planes of both are offered to the route on top (whoever attaches _mmt_rb has recorded _mmt_amax at the same version -- sum_stats,
    f16_split_pg, _conv_f16, carry --, so planes never exist without maxima and asking for the maxima first costs no pass).
    Cout % 4 != 0: no kernel of the fp16 split takes the layer, and no pass is spent on it."""
    st = pl = None
    if F16X2 and _PREC == 3 and x.dtype == torch.float32 and dy.dtype == torch.float32 and w_shape[0] % 4 == 0:
        st = _wgrad_stats(x, dy, dw)
        if st is not None:
            st = _stat_ptrs(st[0]) + _stat_ptrs(st[1])   # (x's maximum, its guard, dy's maximum, its guard)
            if WG_PLANES:
                pl = _wgrad_planes(x, dy, st[1] is not None and st[3] is not None)
    have = (WG_HAVE_MAXIMA if st is not None else 0) | (WG_HAVE_PLANES if pl is not None else 0)
    # the shape half of the job and its route depend on these only: kept after the first call
    key = (x.shape, dy.shape, w_shape, stride, pad, x.dtype, dy.dtype, have, _PREC, sw)
    plan = _WPLAN.get(key)
    if plan is None:
        Cout, Cin, KH, KW = w_shape
        j = WgradJob()
        _conv_shape(j.a, x.shape[0], x.shape[2], x.shape[3], Cin, Cout, KH, KW, stride, pad, dy.shape[2], dy.shape[3])
        j.a.io_bf16 = (IO_X if x.dtype == torch.bfloat16 else 0) | (IO_DY if dy.dtype == torch.bfloat16 else 0)
        r = WgradRoute()
        if lib().mmt_conv_wgrad_route(ctypes.byref(j.a), have, ctypes.byref(r)) != 0:
            r = WgradRoute(splits=1)   # (a block the library refuses: the launch reports it)
        if len(_WPLAN) > 4096:
            _WPLAN.clear()
        plan = _WPLAN[key] = (bytes(j), r)
    j = WgradJob.from_buffer_copy(plan[0])
    a = j.a
    a.x = x.data_ptr()
    j.dy, j.rowscale, j.dw, j.dbias = dy.data_ptr(), _p(rowscale), dw.data_ptr(), _p(dbias)
    if st is not None:
        a.f16_x_amax, a.f16_guard_x, a.f16_dy_amax, a.f16_guard_dy = st
    if pl is None:
        return j, plan[1], st is not None, ()
    xr, dr, a.x_planes_lag = pl
    j.x_planes, j.x_plane_stride = xr.planes.data_ptr(), xr.planes.stride(0)
    j.dy_planes, j.dy_plane_stride = dr.planes.data_ptr(), dr.planes.stride(0)
    j.s_x, j.s_dy = xr.scale.data_ptr(), dr.scale.data_ptr()
    return j, plan[1], True, (xr.planes, dr.planes)


def _wgrad_launch(j, r, f16, device):
    """a prepared weight gradient as a launch of its own, on the kernel its route names -> the split-K workspace it allocated (the
    caller keeps it alive or records the side stream) or None"""
    ws = torch.empty((r.ws_floats,), dtype=torch.float32, device=device) if r.ws_floats > 0 else None
    if r.family in (WGRAD_PLANES_1, WGRAD_PLANES_3):
        _check(lib().mmt_conv_wgrad_planes(ctypes.byref(j.a), j.dy, j.x_planes, j.x_plane_stride, j.dy_planes, j.dy_plane_stride, j.s_x, j.s_dy,
                                           j.rowscale, j.dw, j.dbias, _p(ws), _stream()), "mmt_conv_wgrad_planes")
        F16_STATS["wgrad_pl"] = F16_STATS.get("wgrad_pl", 0) + 1
        return ws
    if f16:   # both operands carry their recorded maximum: two-term fp16 split
        F16_STATS["wgrad"] += 1
    e0 = _ev() if PROFILE is not None and PROFILE_ALL else None
    _check(lib().mmt_conv_wgrad(ctypes.byref(j.a), j.dy, j.rowscale, j.dw, j.dbias, _p(ws), _stream()), "mmt_conv_wgrad")
    if e0 is not None:
        _profiled(j.a, e0, "wgrad", r.splits, None, 0)
    return ws


def _hand_over(ws, side, keep):
    """a workspace a side-stream launch reads: kept by the caller until it has joined the stream, or recorded on the stream"""
    if ws is not None:
        if keep is not None:
            keep.append(ws)
        else:
            ws.record_stream(side)


def conv_wgrad(x, dy, w_shape, stride, pad, dw, rowscale=None, dbias=None, side=None, keep=None):
    """accumulates into dw (same memory layout as the weight) and dbias.  `side`: a torch stream to launch on instead of the
    current one (the caller orders it against the producers of x / dy and joins it later) -- cheaper than entering a stream
    context per call; the split-K workspace is handed to it with record_stream, or -- `keep`, a list -- simply kept alive by
    the caller until it has joined the side stream."""
    if side is not None:
        _TLS.stream = side.cuda_stream
        ws = None
        try:
            ws = _conv_wgrad(x, dy, w_shape, stride, pad, dw, rowscale, dbias)
        finally:
            _TLS.stream = None
            _hand_over(ws, side, keep)
            _drain_det_ws(side, keep)
    else:
        _conv_wgrad(x, dy, w_shape, stride, pad, dw, rowscale, dbias)


def _conv_wgrad(x, dy, w_shape, stride, pad, dw, rowscale, dbias):
    """conv_wgrad on the stream in force -> the split-K workspace the launch reads, or None"""
    x = nhwc(x)
    dy = nhwc(dy)
    bias_to = None
    if _DET and dbias is not None:
        if dy.dtype != torch.float32:
            raise NotImplementedError("deterministic mode: the ordered bias gradient reads fp32 gradients")
        bias_to, dbias = dbias, None   # the weight-gradient kernels' bias epilogues use float atomics: an ordered column sum instead
    get_conv_precision()
    j, r, f16, _ = _wgrad_job(x, dy, w_shape, stride, pad, dw, rowscale, dbias, lib().mmt_conv_switches())
    ws = _wgrad_launch(j, r, f16, x.device)
    if bias_to is not None:
        _bias_ordered(dy, bias_to)
    return ws


def _bias_ordered(dy, out):
    """deterministic mode: out[c] += sum_m dy[m, c] in a fixed order (include/mmtpsm.h: mmt_colsum_ordered), on the stream of the
    launch it belongs to; dy dense fp32 whose memory is [M][C] row-major"""
    C = out.numel()
    M = dy.numel() // C
    ws = torch.empty((COLSUM_MAX_BLOCKS * C,), dtype=torch.float32, device=dy.device)
    _check(lib().mmt_colsum_ordered(_p(dy), M, C, _p(out), _p(ws), _stream()), "mmt_colsum_ordered")
    _keep_det_ws(ws)


def _keep_det_ws(ws):
    """a deterministic-mode workspace just handed to a launch.  On the current stream the caching allocator orders its reuse behind
    the launch (inside a recorded launch plan it comes from the plan's pool and lives with the plan); on a side stream it lives until
    the caller that set the stream has dealt with it (_drain_det_ws)"""
    if getattr(_TLS, "stream", None) is not None:
        kept = getattr(_TLS, "det_ws", None)
        if kept is None:
            kept = _TLS.det_ws = []
        kept.append(ws)


def _drain_det_ws(side, keep):
    kept = getattr(_TLS, "det_ws", None)
    if kept:
        for ws in kept:
            _hand_over(ws, side, keep)
        kept.clear()


# a batch of weight gradients as grouped launches (mmt_conv_wgrad_group): -0.5 ... -0.75 ms per step with every job cut into a quarter
# of the pixel ranges it would use alone (profiles/r06_history.md section 7; MMT_WGRAD_GROUP=0: one launch per layer as before)
WGRAD_GROUP = os.environ.get("MMT_WGRAD_GROUP", "1") != "0"


def conv_wgrad_group(jobs, side=None, keep=None):
    """the weight gradients of a batch of layers -- jobs: (x, dy, w_shape, stride, pad, dw, rowscale, dbias) -- through
    mmt_conv_wgrad_group (include/mmtpsm.h: grouped launches); jobs of another arithmetic (bf16 storage, an operand without a recorded
    maximum, a site on the bf16 fall-back, a shape no kernel of the fp16 split takes) go out as conv_wgrad launches them, in order.
    `side`, `keep` as in conv_wgrad.  WGRAD_GROUP off (a test hook; MMT_WGRAD_GROUP=0 at import): nothing is offered to the grouped
    entry point -- which reads the same variable per call and then launches every job singly."""
    wss = []   # the launches' workspaces
    if side is not None:
        _TLS.stream = side.cuda_stream
    try:
        _conv_wgrad_group(jobs, keep if keep is not None else [], wss)
    finally:
        if side is not None:
            _TLS.stream = None
            for ws in wss:
                _hand_over(ws, side, keep)
            _drain_det_ws(side, keep)
        elif keep is not None:
            keep.extend(wss)
        # (on the current stream without `keep`: the caching allocator orders the buffers' reuse behind the launches)


def _conv_wgrad_group(jobs, keep, wss):
    """conv_wgrad_group on the stream in force.  keep: a list for the operands and planes the grouped launches read; wss: a list
    for the workspaces allocated here"""
    get_conv_precision()
    grouped, single, biases = [], [], []   # biases: deterministic mode, (dy, dbias) of the grouped jobs -- ordered column sums behind the launches
    if WGRAD_GROUP and not (PROFILE is not None and PROFILE_ALL):
        sw = lib().mmt_conv_switches()
        for job in jobs:
            x, dy, w_shape, stride, pad, dw, rowscale, dbias = job
            x, dy = nhwc(x), nhwc(dy)
            j, r, f16, alive = _wgrad_job(x, dy, w_shape, stride, pad, dw, rowscale, None if _DET else dbias, sw)
            if not f16 or r.family == WGRAD_NONE:
                single.append(job)
            else:
                grouped.append(j)
                keep.extend(alive + (x, dy))
                if _DET and dbias is not None:
                    biases.append((dy, dbias))
    else:
        single = jobs
    for c0 in range(0, len(grouped), 96):
        chunk = grouped[c0:c0 + 96]
        arr = (WgradJob * len(chunk))(*chunk)
        need_c = ctypes.c_long(0)
        if lib().mmt_conv_wgrad_group_workspace(ctypes.addressof(arr), len(chunk), ctypes.byref(need_c)) != 0:
            raise RuntimeError("mmt_conv_wgrad_group_workspace failed")
        need = need_c.value
        ws = torch.empty((need,), dtype=torch.float32, device=torch.device("cuda", _cur_dev())) if need > 0 else None
        _check(lib().mmt_conv_wgrad_group(ctypes.addressof(arr), len(chunk), _p(ws), need, _stream()), "mmt_conv_wgrad_group")
        F16_STATS["wgrad_grouped"] = F16_STATS.get("wgrad_grouped", 0) + len(chunk)
        if ws is not None:
            wss.append(ws)
    for dy, dbias in biases:
        _bias_ordered(dy, dbias)
    for job in single:
        ws = _conv_wgrad(*job)
        if ws is not None:
            wss.append(ws)


def colsum(dy2d, out):
    """out[c] += sum_m dy2d[m, c]; dy2d any dense tensor whose memory is [M][C] row-major"""
    if _DET:
        return _bias_ordered(dy2d, out)
    C = out.numel()
    M = dy2d.numel() // C
    _check(lib().mmt_colsum(_p(dy2d), M, C, _p(out), _stream()), "mmt_colsum")


def weight_flip_transpose(w, scale=None, owner=None):
    """w (Cout,Cin,KH,KW) channels_last-dense -> (Cin,Cout,KH,KW) channels_last-dense, taps flipped, rows scaled
    owner: the tensor object the forward pass was given as `w` (a backward pass sees its saved tensors as new Python objects; the
    node keeps the forward's): with it the result is kept for the next launch with the same object, version and parameter generation"""
    w0, w = (w if owner is None else owner), nhwc(w)
    Cout, Cin, KH, KW = w.shape
    # the RPN predictors' data gradient runs once per pyramid level with the same weights: flipped once per version and stream
    # (identity of the Parameter object, not its address: a freed tensor's address comes back with another tensor's values)
    stamp = _loose_stamp(w, scale, w0, _stream())
    hit = LOOSE.get(w0, "f32_dgrad", stamp, scale)
    if hit is not None:
        return hit
    wd = empty_nhwc(Cin, Cout, KH, KW, w.device)
    _check(lib().mmt_weight_flip_transpose(_p(w), _p(scale), _p(wd), Cout, KH, KW, Cin, _stream()),
           "mmt_weight_flip_transpose")
    if scale is None and owner is not None and w0.data_ptr() == w.data_ptr() and w0._version == w._version:
        LOOSE.put(w0, "f32_dgrad", stamp, scale, wd, w)
    return wd


def maxpool3x3s2(x):
    x = nhwc(x)
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = empty_nhwc(N, C, Ho, Wo, x.device, dtype=x.dtype)
    if x.dtype == torch.bfloat16:
        _check(lib().mmt_maxpool3x3s2_bf16(_p(x), _p(y), N, H, W, C, Ho, Wo, _stream()), "mmt_maxpool3x3s2_bf16")
    else:
        _check(lib().mmt_maxpool3x3s2(_p(x), _p(y), N, H, W, C, Ho, Wo, _stream()), "mmt_maxpool3x3s2")
    return y


def refuse_trainable_stem_bf16():
    """a stem that records gradients, asked before its forward launches (modeling/backbone/backbone.py): its backward reads the
    un-pooled output as fp32"""
    if bf16_storage():
        raise NotImplementedError("MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0 (a trainable stem) is not offered with bf16 activation "
                                  "storage: set_bf16_storage(False)")


def maxpool3x3s2_backward(y, g, out=None):
    """include/mmtpsm.h: mmt_maxpool3x3s2_backward.  y (N, C, H, W) the pool's input (a ReLU output), g the gradient of
    maxpool3x3s2(y) -> (y > 0) * the pool's gradient, ATen's first-maximum rule; every element is written (out: a destination to fill)"""
    y, g = nhwc(_dev(y, "y")), nhwc(_dev(g, "g"))
    N, C, H, W = y.shape
    if (y.dtype != torch.float32 or g.dtype != torch.float32 or C % 4
            or tuple(g.shape) != (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)):
        raise RuntimeError("max-pool backward: fp32 y (N, C, H, W) with C %% 4 == 0 and g of the pooled shape; got y %s, g %s"
                           % (tuple(y.shape), tuple(g.shape)))
    if out is None:
        out = empty_nhwc(N, C, H, W, y.device)
    elif tuple(out.shape) != (N, C, H, W) or out.dtype != torch.float32 or not out.is_cuda or nhwc(out) is not out:
        raise RuntimeError("max-pool backward: `out` is an NHWC-dense fp32 GPU tensor of y's shape")
    _check(lib().mmt_maxpool3x3s2_backward(_p(y), _p(g), _p(out), N, H, W, C, _stream()), "mmt_maxpool3x3s2_backward")
    return out


def _stem_wgrad_args(x, dy, dw, rowscale):
    """checked (dy NHWC-dense, N, H, W) of a stem weight-gradient call"""
    _dev(x, "x")
    dy = nhwc(_dev(dy, "dy"))
    N, C, H, W = x.shape
    if (C != 3 or x.dtype != torch.float32 or not x.is_contiguous() or dy.dtype != torch.float32
            or tuple(dy.shape) != (N, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1)):
        raise RuntimeError("stem weight gradient: fp32 NCHW-contiguous x (N, 3, H, W) and dy (N, 64, Ho, Wo); got x %s, dy %s"
                           % (tuple(x.shape), tuple(dy.shape)))
    _dev(dw, "dw")
    if dw.dtype != torch.float32 or dw.numel() != 64 * 147 or (dw.dim() == 4 and (tuple(dw.shape) != (64, 3, 7, 7) or nhwc(dw) is not dw)) \
            or (dw.dim() != 4 and not dw.is_contiguous()):
        raise RuntimeError("stem weight gradient: dw is a dense fp32 tensor in the weight's layout (64, 3, 7, 7 channels-last)")
    if rowscale is not None and not (rowscale.is_cuda and rowscale.dtype == torch.float32 and rowscale.numel() == 64 and rowscale.is_contiguous()):
        raise RuntimeError("stem weight gradient: rowscale is a dense fp32 GPU vector of 64 elements")
    return dy, N, H, W


def stem_wgrad(x, dy, dw, rowscale=None):
    """include/mmtpsm.h: mmt_stem_wgrad.  x (N, 3, H, W) fp32 NCHW-contiguous (the image), dy (N, 64, Ho, Wo) the gradient of the
    7x7 / stride 2 / pad 3 convolution's output; dw (64, 3, 7, 7 in the weight's channels-last layout) += rowscale[co] * the
    weight gradient, the blocks' sums added with float atomics.  This form stays refused in deterministic mode
    (tests/test_deterministic_kernels_gpu.py); the mode's callers take stem_wgrad_ordered (layers/fused.py::StemFn.backward)"""
    dy, N, H, W = _stem_wgrad_args(x, dy, dw, rowscale)
    if _DET:
        raise NotImplementedError("stem_wgrad is not offered in deterministic mode: stem_wgrad_kernel adds into its destination with "
                                  "float atomics here; call stem_wgrad_ordered, or set_deterministic(False)")
    _check(lib().mmt_stem_wgrad(_p(x), _p(dy), _p(rowscale), _p(dw), N, H, W, _stream()), "mmt_stem_wgrad")
    return dw


def stem_wgrad_ordered(x, dy, dw, rowscale=None):
    """include/mmtpsm.h: mmt_stem_wgrad_ordered.  stem_wgrad's arguments and result with the blocks' sums stored to a workspace and
    added in block order: the same bits run to run, in either mode"""
    dy, N, H, W = _stem_wgrad_args(x, dy, dw, rowscale)
    ws = _wgrad_ordered_ws(lib().mmt_stem_wgrad_ws_floats(N, H, W), x.device, "mmt_stem_wgrad_ws_floats")
    _check(lib().mmt_stem_wgrad_ordered(_p(x), _p(dy), _p(rowscale), _p(dw), N, H, W, _p(ws), ws.numel(), _stream()),
           "mmt_stem_wgrad_ordered")
    _keep_det_ws(ws)
    return dw


def _wgrad_ordered_ws(floats, device, what):
    """the workspace of an ordered weight gradient, sized by the library's query (nothing in it needs clearing: every partial the
    finish reads is written by stage one)"""
    if floats <= 0:
        raise RuntimeError("%s refused the shape (%d)" % (what, floats))
    return torch.empty((floats,), dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------ grouped 3x3 convolution (ResNeXt conv2)
GCONV_WIDTHS = (8, 16, 32, 64)   # channels per group csrc/conv_group.hip takes


def _gconv_args(x, w, stride):
    """checked (x, w, N, C, H, W, Cg) of a grouped 3x3 call: x (N, C, H, W), w (C, Cg, 3, 3), both fp32"""
    if bf16_storage():
        raise NotImplementedError("grouped 3x3 convolutions (ResNeXt) are not offered with bf16 activation storage: "
                                  "set_bf16_storage(False)")
    x, w = nhwc(_dev(x)), nhwc(_dev(w, "weight"))
    if x.dtype != torch.float32 or w.dtype != torch.float32:
        raise RuntimeError("grouped 3x3 convolution: fp32 tensors only")
    N, C, H, W = x.shape
    Cg = w.shape[1]
    if tuple(w.shape) != (C, Cg, 3, 3) or Cg not in GCONV_WIDTHS or C % Cg or C % 32 or stride not in (1, 2):
        raise RuntimeError("grouped 3x3 convolution: weight (C, Cg, 3, 3) with Cg in %s, C %% 32 == 0, stride 1 or 2; got x %s, w %s, "
                           "stride %s" % (GCONV_WIDTHS, tuple(x.shape), tuple(w.shape), stride))
    return x, w, N, C, H, W, Cg


def _gconv_vec(t, C, name):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float32 and t.numel() == C and t.is_contiguous()):
        raise RuntimeError("grouped 3x3 convolution: %s is a dense fp32 GPU vector of C elements" % name)
    return t


def gconv3x3_forward(x, w, scale=None, shift=None, stride=1, relu=False):
    """include/mmtpsm.h: mmt_gconv3x3_forward.  y = relu?(conv(x, w, pad 1, stride, groups = C / Cg) * scale[co] + shift[co])"""
    x, w, N, C, H, W, Cg = _gconv_args(x, w, stride)
    y = empty_nhwc(N, C, (H - 1) // stride + 1, (W - 1) // stride + 1, x.device)
    _check(lib().mmt_gconv3x3_forward(_p(x), _p(w), _p(_gconv_vec(scale, C, "scale")), _p(_gconv_vec(shift, C, "shift")), _p(y),
                                      N, H, W, C, Cg, stride, 1 if relu else 0, _stream()), "mmt_gconv3x3_forward")
    return y


def gconv3x3_dgrad(dy, w, x_hw, stride=1, scale=None, mask=None, out=None):
    """include/mmtpsm.h: mmt_gconv3x3_dgrad.  The gradient w.r.t. the (H, W) = x_hw input of gconv3x3_forward for the output gradient
    dy, times scale[co] on the way in and (mask > 0) on the way out; every element is written (out: a destination to fill)"""
    dy, w, N, C, Ho, Wo, Cg = _gconv_args(dy, w, stride)
    H, W = int(x_hw[0]), int(x_hw[1])
    if ((H - 1) // stride + 1, (W - 1) // stride + 1) != (Ho, Wo):
        raise RuntimeError("grouped 3x3 data gradient: dy %s is not the output of a stride-%d convolution over %s" % (tuple(dy.shape), stride, (H, W)))
    if mask is not None:
        mask = nhwc(_dev(mask, "mask"))
        if tuple(mask.shape) != (N, C, H, W) or mask.dtype != torch.float32:
            raise RuntimeError("grouped 3x3 data gradient: the mask has the shape and type of dx")
    if out is None:
        out = empty_nhwc(N, C, H, W, dy.device)
    elif tuple(out.shape) != (N, C, H, W) or out.dtype != torch.float32 or not out.is_cuda or nhwc(out) is not out:
        raise RuntimeError("grouped 3x3 data gradient: `out` is an NHWC-dense fp32 GPU tensor of dx's shape")
    wt = torch.empty((C * 9 * Cg,), dtype=torch.float32, device=dy.device)   # (stream-ordered allocator: alive for the launch)
    _check(lib().mmt_gconv3x3_dgrad(_p(dy), _p(w), _p(_gconv_vec(scale, C, "scale")), _p(mask), _p(wt), _p(out), N, H, W, C, Cg, stride,
                                    _stream()), "mmt_gconv3x3_dgrad")
    return out


def gconv3x3_wgrad(x, dy, w_shape, stride, dw, rowscale=None):
    """include/mmtpsm.h: mmt_gconv3x3_wgrad.  dw (C, Cg, 3, 3 in the weight's layout) += rowscale[co] * the weight gradient"""
    _refuse_unordered("gconv_wgrad_kernel", "the weight gradient of a grouped 3x3 convolution (ResNeXt conv2)")
    if bf16_storage():
        raise NotImplementedError("grouped 3x3 convolutions (ResNeXt) are not offered with bf16 activation storage: "
                                  "set_bf16_storage(False)")
    x, dy = nhwc(_dev(x)), nhwc(_dev(dy, "dy"))
    N, C, H, W = x.shape
    Cg = int(w_shape[1])
    if (tuple(w_shape) != (C, Cg, 3, 3) or Cg not in GCONV_WIDTHS or C % Cg or C % 32 or stride not in (1, 2)
            or tuple(dy.shape) != (N, C, (H - 1) // stride + 1, (W - 1) // stride + 1)
            or x.dtype != torch.float32 or dy.dtype != torch.float32):
        raise RuntimeError("grouped 3x3 weight gradient: fp32 x (N, C, H, W), dy of the stride-%s output, weight (C, Cg, 3, 3) with Cg in "
                           "%s; got x %s, dy %s, w %s" % (stride, GCONV_WIDTHS, tuple(x.shape), tuple(dy.shape), tuple(w_shape)))
    _dev(dw, "dw")
    if dw.dtype != torch.float32 or dw.numel() != C * Cg * 9 or (dw.dim() == 4 and nhwc(dw) is not dw) or (dw.dim() != 4 and not dw.is_contiguous()):
        raise RuntimeError("grouped 3x3 weight gradient: dw is a dense fp32 tensor in the weight's layout")
    _check(lib().mmt_gconv3x3_wgrad(_p(x), _p(dy), _p(_gconv_vec(rowscale, C, "rowscale")), _p(dw), N, H, W, C, Cg, stride, _stream()),
           "mmt_gconv3x3_wgrad")
    return dw


# ------------------------------------------------------------------------------------------ losses
def rpn_loss(obj, reg, labels, regt, pos, neg, beta):
    """include/mmtpsm.h: mmt_rpn_loss.  obj (R,), reg / regt (R, 4), labels (R,) float, pos / neg (R,) bool
    -> out (2,) = (objectness loss, box loss), d out[0] / d obj (R,), d out[1] / d reg (R, 4)"""
    obj, reg = _dev(obj, "obj").float().contiguous(), _dev(reg, "reg").float().contiguous()
    labels, regt = labels.float().contiguous(), regt.float().contiguous()
    pos, neg = pos.contiguous(), neg.contiguous()
    if pos.dtype != torch.bool or neg.dtype != torch.bool:
        raise RuntimeError("rpn_loss: the sampler masks are bool tensors")
    R = obj.numel()
    # sums [0:3], out [4:6]; deterministic mode: the library's block partials behind them
    ws = torch.empty((8 + 3 * RPN_LOSS_MAX_BLOCKS if _DET else 8,), dtype=torch.float32, device=obj.device)
    dobj, dreg = torch.empty_like(obj), torch.empty_like(reg)
    _check(lib().mmt_rpn_loss(_p(obj), _p(reg), _p(labels), _p(regt), _p(pos), _p(neg), R, float(beta), _p(ws), ws.data_ptr() + 16,
                              _p(dobj), _p(dreg), _stream()), "mmt_rpn_loss")
    return ws[4:6], dobj, dreg


def box_loss(logits, breg, labels, regt, n_rows=None):
    """include/mmtpsm.h: mmt_box_loss / mmt_box_loss_rows.  logits (R, NC), breg (R, 4 NC), labels (R,) int64, regt (R, 4)
    -> out (2,) = (classification loss, box loss), d out[0] / d logits, d out[1] / d breg.  n_rows (device int64 scalar): the batch
    is a fixed-capacity one -- rows labelled -1 are skipped, the means run over n_rows"""
    logits, breg = _dev(logits, "logits").float().contiguous(), _dev(breg, "breg").float().contiguous()
    labels, regt = labels.to(torch.int64).contiguous(), regt.float().contiguous()
    R, NC = logits.shape
    out = torch.empty((2,), dtype=torch.float32, device=logits.device)
    dl, db = torch.empty_like(logits), torch.empty_like(breg)
    if _DET:
        ws = torch.empty((2 * BOX_LOSS_MAX_BLOCKS,), dtype=torch.float32, device=logits.device)
        _check(lib().mmt_box_loss_ordered(_p(logits), _p(breg), _p(labels), _p(regt), R, NC,
                                          None if n_rows is None else _p(n_rows.to(torch.int64)), _p(out), _p(dl), _p(db), _p(ws),
                                          _stream()), "mmt_box_loss_ordered")
        return out, dl, db
    if n_rows is not None:
        _check(lib().mmt_box_loss_rows(_p(logits), _p(breg), _p(labels), _p(regt), R, NC, _p(n_rows.to(torch.int64)), _p(out), _p(dl),
                                       _p(db), _stream()), "mmt_box_loss_rows")
        return out, dl, db
    _check(lib().mmt_box_loss(_p(logits), _p(breg), _p(labels), _p(regt), R, NC, _p(out), _p(dl), _p(db), _stream()), "mmt_box_loss")
    return out, dl, db


def mask_bce(logits, labels, targets, grad_scale=1.0):
    """logits (P,NC,M,M) NHWC-dense, labels (P,) int, targets (P,M,M) -> (loss scalar tensor, grad like logits)"""
    logits = nhwc(logits)
    P, NC, M, _ = logits.shape
    labels = _dev(labels).to(torch.int32).contiguous()
    targets = _dev(targets).float().contiguous()
    loss = torch.zeros((), dtype=torch.float32, device=logits.device)
    grad = empty_nhwc(P, NC, M, M, logits.device)
    if _DET:
        ws = torch.empty((MASK_BCE_WS,), dtype=torch.float32, device=logits.device)
        _check(lib().mmt_mask_bce_ordered(_p(logits), _p(labels), _p(targets), P, M * M, NC, float(grad_scale), _p(loss), _p(grad),
                                          _p(ws), _stream()), "mmt_mask_bce_ordered")
        return loss, grad
    _check(lib().mmt_mask_bce(_p(logits), _p(labels), _p(targets), P, M * M, NC, float(grad_scale), _p(loss), _p(grad),
                              _stream()), "mmt_mask_bce")
    return loss, grad


def _teachers(ts, flips):
    if not 1 <= len(ts) <= MGD_MAX_TEACHERS or len(flips) != len(ts):
        raise RuntimeError("MGD: %d teacher views with %d flips; the kernels take 1 to %d views, one flip each"
                           % (len(ts), len(flips), MGD_MAX_TEACHERS))
    T = MgdTeachers()
    T.nt = len(ts)
    for i, (t, f) in enumerate(zip(ts, flips)):
        T.t[i] = t.data_ptr()
        T.flip[i] = 1 if f else 0
    return T


def mgd_level_forward(s, ts, flips, m, acc=None):
    """-> acc (nt+1,) = [num_i..., msum]; `acc`: a zeroed row to accumulate into (one tensor for all levels of a call)"""
    s = nhwc(s)
    ts = [nhwc(t) for t in ts]
    N, C, H, W = s.shape
    if acc is None:
        acc = torch.zeros((len(ts) + 1,), dtype=torch.float32, device=s.device)
    T = _teachers(ts, flips)
    if _DET:
        ws = torch.empty((MGD_MAX_BLOCKS * (len(ts) + 1),), dtype=torch.float32, device=s.device)
        _check(lib().mmt_mgd_level_forward_ordered(_p(s), ctypes.byref(T), _p(m), N, H, W, C, _p(acc), _p(ws), _stream()),
               "mmt_mgd_level_forward_ordered")
        return acc
    _check(lib().mmt_mgd_level_forward(_p(s), ctypes.byref(T), _p(m), N, H, W, C, _p(acc), _stream()),
           "mmt_mgd_level_forward")
    return acc


def mgd_level_backward(s, ts, flips, m, coef):
    s = nhwc(s)
    ts = [nhwc(t) for t in ts]
    N, C, H, W = s.shape
    g = empty_nhwc(N, C, H, W, s.device)
    T = _teachers(ts, flips)
    if coef.dtype != torch.float32 or not coef.is_contiguous():
        coef = coef.float().contiguous()
    _check(lib().mmt_mgd_level_backward(_p(s), ctypes.byref(T), _p(m), N, H, W, C, _p(coef), _p(g), _stream()),
           "mmt_mgd_level_backward")
    return g


MGD_MAX_STUDENTS, MGD_MAX_TEACHERS, MGD_MAX_TERMS = 4, 8, 16   # the register budget of mmt_mgd_views_* (include/mmtpsm.h)


def mgd_views_supported(ns, nt):
    return 1 <= ns <= MGD_MAX_STUDENTS and 1 <= nt <= MGD_MAX_TEACHERS and ns * nt <= MGD_MAX_TERMS


def _students(ss, mirrors):
    S = MgdStudents()
    S.ns = len(ss)
    for j, (s, f) in enumerate(zip(ss, mirrors)):
        S.s[j] = s.data_ptr()
        S.mirror[j] = 1 if f else 0
    return S


def _views_check(ss, ts):
    if not mgd_views_supported(len(ss), len(ts)):
        raise RuntimeError("MGD over student views: %d students x %d teacher views is beyond the kernel's register budget "
                           "(at most %d students, %d teachers, %d pairs)" % (len(ss), len(ts), MGD_MAX_STUDENTS, MGD_MAX_TEACHERS,
                                                                            MGD_MAX_TERMS))
    for t in list(ss) + list(ts):
        if t.shape != ss[0].shape or t.dtype != torch.float32:
            raise RuntimeError("MGD over student views: every student and teacher embedding of a level is fp32 and has the same shape")


def mgd_views_forward(ss, mirrors, ts, flips, m, acc=None):
    """-> acc (ns*nt+1,) = [num(j, i) at j*nt + i ..., msum] of one level, all student views x all teacher views in ONE launch;
    `acc`: a zeroed row to accumulate into"""
    ss = [nhwc(s) for s in ss]
    ts = [nhwc(t) for t in ts]
    _views_check(ss, ts)
    N, C, Hh, W = ss[0].shape
    if acc is None:
        acc = torch.zeros((len(ss) * len(ts) + 1,), dtype=torch.float32, device=ss[0].device)
    S, T = _students(ss, mirrors), _teachers(ts, flips)
    if _DET:
        ws = torch.empty((MGD_MAX_BLOCKS * (len(ss) * len(ts) + 1),), dtype=torch.float32, device=ss[0].device)
        _check(lib().mmt_mgd_views_forward_ordered(ctypes.byref(S), ctypes.byref(T), _p(m), N, Hh, W, C, _p(acc), _p(ws), _stream()),
               "mmt_mgd_views_forward_ordered")
        return acc
    _check(lib().mmt_mgd_views_forward(ctypes.byref(S), ctypes.byref(T), _p(m), N, Hh, W, C, _p(acc), _stream()),
           "mmt_mgd_views_forward")
    return acc


def mgd_views_backward(ss, mirrors, ts, flips, m, coef):
    """-> [gradient of student j, in view j's own frame] (NHWC views of one [ns, N, H, W, C] buffer); coef (ns*nt,) at j*nt + i"""
    ss = [nhwc(s) for s in ss]
    ts = [nhwc(t) for t in ts]
    _views_check(ss, ts)
    N, C, Hh, W = ss[0].shape
    g = empty_nhwc(len(ss) * N, C, Hh, W, ss[0].device)
    S, T = _students(ss, mirrors), _teachers(ts, flips)
    if coef.dtype != torch.float32 or not coef.is_contiguous():
        coef = coef.float().contiguous()
    _check(lib().mmt_mgd_views_backward(ctypes.byref(S), ctypes.byref(T), _p(m), N, Hh, W, C, _p(coef), _p(g), _stream()),
           "mmt_mgd_views_backward")
    return [g[j * N:(j + 1) * N] for j in range(len(ss))]


def mask_pool(seg, H, W):
    """seg (N,IH,IW) int32 -> (N,H,W) float {0,1}"""
    seg = _dev(seg).to(torch.int32).contiguous()
    N, IH, IW = seg.shape
    m = torch.empty((N, H, W), dtype=torch.float32, device=seg.device)
    _check(lib().mmt_mask_pool(_p(seg), N, IH, IW, H, W, _p(m), _stream()), "mmt_mask_pool")
    return m


def psm_rows(teacher, student, roww, temp, sharpen, kind):
    teacher = _dev(teacher).float().contiguous()
    student = _dev(student).float().contiguous()
    roww = _dev(roww).float().contiguous()
    K, R, NC = teacher.shape
    rl = torch.empty((R,), dtype=torch.float32, device=teacher.device)
    rg = torch.empty((R, NC), dtype=torch.float32, device=teacher.device)
    _check(lib().mmt_psm_rows(_p(teacher), K, _p(student), R, NC, _p(roww), float(temp), int(sharpen), int(kind),
                              _p(rl), _p(rg), _stream()), "mmt_psm_rows")
    return rl, rg


def psm_variance(teacher, use_softmax=True):
    teacher = _dev(teacher).float().contiguous()
    K, R, NC = teacher.shape
    v = torch.empty((R,), dtype=torch.float32, device=teacher.device)
    _check(lib().mmt_psm_variance(_p(teacher), K, R, NC, 1 if use_softmax else 0, _p(v), _stream()), "mmt_psm_variance")
    return v


# ------------------------------------------------------------------------------------------ optimiser / EMA
def ema_update(teacher_flat, student_flat, alpha):
    _dev(teacher_flat)
    _dev(student_flat)
    assert teacher_flat.numel() == student_flat.numel() and teacher_flat.is_contiguous() and student_flat.is_contiguous()
    LOOSE.forget(teacher_flat)
    _check(lib().mmt_ema_update(_p(teacher_flat), _p(student_flat), teacher_flat.numel(), float(alpha), _stream()),
           "mmt_ema_update")


def sgd_momentum(p, g, buf, lr, wd, momentum, first):
    _dev(p)
    LOOSE.forget(p)
    _check(lib().mmt_sgd_momentum(_p(p), _p(g), _p(buf), p.numel(), float(lr), float(wd), float(momentum),
                                  1 if first else 0, _stream()), "mmt_sgd_momentum")


# ---- the guarded step (include/mmtpsm.h: mmt_grad_guard; solver/build.py: FlatSGD.enable_guard)
GRAD_GUARD_WS, GRAD_GUARD_STATE_WORDS = 4096, 8   # include/mmtpsm.h
GUARD_COEF, GUARD_NORM, GUARD_SKIP, GUARD_SEEN, GUARD_SKIPPED, GUARD_CLIPPED, GUARD_CONSECUTIVE = range(7)   # the state words


def grad_guard_buffers(device):
    """-> (state, ws) as mmt_grad_guard takes them: state = GRAD_GUARD_STATE_WORDS zeroed fp32 words (words 2..6 hold int32 values:
    read them through `state.view(torch.int32)`), ws = GRAD_GUARD_WS doubles"""
    return (torch.zeros((GRAD_GUARD_STATE_WORDS,), dtype=torch.float32, device=device),
            torch.empty((GRAD_GUARD_WS,), dtype=torch.float64, device=device))


def _guard_state(state):
    _dev(state, "state")
    if state.dtype != torch.float32 or state.numel() != GRAD_GUARD_STATE_WORDS or not state.is_contiguous() or state.data_ptr() & 15:
        raise RuntimeError("grad guard: state must be %d contiguous, 16-byte aligned fp32 words (grad_guard_buffers), got %s of %d"
                           % (GRAD_GUARD_STATE_WORDS, state.dtype, state.numel()))
    return state


def _flat_f32(t, name):
    _dev(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() & 15:
        raise RuntimeError("%s must be a dense fp32 tensor on the 16-byte grid, got %s%s" % (name, t.dtype, "" if t.is_contiguous() else
                                                                                           " (not contiguous)"))
    return t


def grad_guard(g, state, ws, max_norm):
    """the L2 norm of g in fp64 and the step's verdict, into `state` on the device (two launches, no read-back): skip when g holds
    a non-finite value; max_norm > 0: clip coefficient of torch.nn.utils.clip_grad_norm_; max_norm 0: observe only"""
    _flat_f32(g, "g")
    _guard_state(state)
    _dev(ws, "ws")
    if ws.dtype != torch.float64 or ws.numel() < GRAD_GUARD_WS or not ws.is_contiguous() or ws.data_ptr() & 15:
        raise RuntimeError("grad guard: ws must be %d contiguous, 16-byte aligned doubles (grad_guard_buffers), got %s of %d"
                           % (GRAD_GUARD_WS, ws.dtype, ws.numel()))
    if g.device != state.device or g.device != ws.device:
        raise RuntimeError("grad guard: g, state and ws live on different devices")
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError("grad guard: max_norm must be >= 0 (0: no clipping), got %r" % (max_norm,))
    _check(lib().mmt_grad_guard(_p(g), g.numel(), _p(ws), _p(state), max_norm, _stream()), "mmt_grad_guard")


def sgd_momentum_guarded(p, g, buf, lr, wd, momentum, first, state):
    """`sgd_momentum` on g * state[coef], or nothing at all when `grad_guard` set the skip flag; g is left as it is"""
    _flat_f32(p, "p")
    _flat_f32(g, "g")
    _flat_f32(buf, "buf")
    _guard_state(state)
    if not (p.numel() == g.numel() == buf.numel()):
        raise RuntimeError("sgd_momentum_guarded: p, g and buf differ in size (%d, %d, %d)" % (p.numel(), g.numel(), buf.numel()))
    LOOSE.forget(p)
    _check(lib().mmt_sgd_momentum_guarded(_p(p), _p(g), _p(buf), p.numel(), float(lr), float(wd), float(momentum),
                                          1 if first else 0, _p(state), _stream()), "mmt_sgd_momentum_guarded")


# ------------------------------------------------------------------------------------------ masks
def paste_masks(logits, labels, boxes, img, N, IH, IW, thresh):
    """logits (D,NC,M,M) NHWC-dense -> seg (N,IH,IW) int32"""
    logits = nhwc(logits)
    D, NC, M, _ = logits.shape
    labels = _dev(labels).to(torch.int32).contiguous()
    boxes = _dev(boxes).float().contiguous()
    img = _dev(img).to(torch.int32).contiguous()
    seg = torch.zeros((N, IH, IW), dtype=torch.int32, device=logits.device)
    _check(lib().mmt_paste_masks(_p(logits), _p(labels), _p(boxes), _p(img), D, M, NC, IH, IW, float(thresh), _p(seg),
                                 _stream()), "mmt_paste_masks")
    return seg


def paste_mask_stack(prob, boxes, IH, IW, thresh):
    """prob (D,1,M,M) or (D,M,M) probabilities of the predicted class, boxes (D,4) -> uint8 (D,1,IH,IW): one pasted binary mask
    per detection (include/mmtpsm.h: mmt_paste_mask_stack)"""
    prob = _dev(prob, "prob").float().contiguous()
    D, M = prob.shape[0], prob.shape[-1]
    boxes = _dev(boxes, "boxes").float().contiguous()
    out = torch.zeros((D, 1, IH, IW), dtype=torch.uint8, device=prob.device)
    _check(lib().mmt_paste_mask_stack(_p(prob), _p(boxes), D, M, IH, IW, float(thresh), _p(out), _stream()), "mmt_paste_mask_stack")
    return out


def polygon_targets(poly_xy, poly_off, roi_poly, boxes, M):
    poly_xy = _dev(poly_xy).float().contiguous()
    poly_off = _dev(poly_off).to(torch.int32).contiguous()
    roi_poly = _dev(roi_poly).to(torch.int32).contiguous()
    boxes = _dev(boxes).float().contiguous()
    P = boxes.shape[0]
    out = torch.empty((P, M, M), dtype=torch.float32, device=boxes.device)
    ovf = torch.zeros((1,), dtype=torch.int32, device=boxes.device)
    _check(lib().mmt_polygon_targets(_p(poly_xy), _p(poly_off), _p(roi_poly), _p(boxes), P, M, _p(out), _p(ovf), _stream()),
           "mmt_polygon_targets")
    return out, ovf


# ---- mask work of the PAP evaluator (include/mmtpsm.h: mmt_mask_*; csrc/maskeval.hip).  A stack of masks on the device is
# (words int64 [n, ceil(H*W/64)] -- the 64-bit words of the codec's column-major flattening --, records int32 [n, 8]).
MASK_REC = 8   # MMT_MASK_REC_INTS


def _mask_buffers(n, H, W, device):
    if H <= 0 or W <= 0 or H * W >= (1 << 31):
        raise RuntimeError("masks of %d x %d: 0 < H * W < 2^31 only" % (H, W))
    return (torch.empty((n, (H * W + 63) // 64), dtype=torch.int64, device=device),
            torch.empty((n, MASK_REC), dtype=torch.int32, device=device))


def mask_pack(masks):
    """masks uint8 (n, H, W), non-zero = set -> (words, records) (mmt_mask_pack)"""
    masks = _dev(masks, "masks")
    if masks.dtype != torch.uint8 or masks.dim() != 3:
        raise RuntimeError("mask_pack: a uint8 (n, H, W) stack")
    masks = masks.contiguous()
    n, H, W = masks.shape
    words, rec = _mask_buffers(n, H, W, masks.device)
    _check(lib().mmt_mask_pack(_p(masks), n, H, W, _p(words), _p(rec), _stream()), "mmt_mask_pack")
    return words, rec


def paste_mask_words(prob, boxes, IH, IW, thresh):
    """prob (D,1,M,M) or (D,M,M) probabilities of the predicted class, boxes (D,4) -> (words, records): what
    mask_pack(paste_mask_stack(...)[:, 0]) gives, bit for bit, without the (D, IH, IW) bytes (mmt_paste_mask_words)"""
    prob = _dev(prob, "prob").float().contiguous()
    D, M = prob.shape[0], prob.shape[-1]
    boxes = _dev(boxes, "boxes").float().contiguous()
    words, rec = _mask_buffers(D, IH, IW, prob.device)
    _check(lib().mmt_paste_mask_words(_p(prob), _p(boxes), D, M, IH, IW, float(thresh), _p(words), _p(rec), _stream()),
           "mmt_paste_mask_words")
    return words, rec


def mask_expand(ends, off, H, W):
    """ends int32: the concatenated inclusive prefix sums of every mask's run lengths, off int64 (n + 1) -> (words, records)
    (mmt_mask_expand)"""
    ends, off = _dev(ends, "ends"), _dev(off, "off")
    if ends.dtype != torch.int32 or off.dtype != torch.int64 or off.numel() < 1:
        raise RuntimeError("mask_expand: int32 prefix sums and int64 offsets")
    n = off.numel() - 1
    words, rec = _mask_buffers(n, H, W, ends.device)
    _check(lib().mmt_mask_expand(_p(ends.contiguous()), _p(off.contiguous()), n, H, W, _p(words), _p(rec), _stream()), "mmt_mask_expand")
    return words, rec


def mask_transitions(words, H, W):
    """-> (counts int64 (n,) on the HOST, positions int32 on the HOST, concatenated mask after mask): where bit(k) != bit(k - 1)
    in each mask, ascending (mmt_mask_transition_counts / _positions).  The only data that crosses to the host."""
    words = _dev(words, "words")
    n = words.shape[0]
    counts = torch.empty((n,), dtype=torch.int32, device=words.device)
    _check(lib().mmt_mask_transition_counts(_p(words), n, H, W, _p(counts), _stream()), "mmt_mask_transition_counts")
    counts = counts.cpu().to(torch.int64)
    off = torch.zeros((n + 1,), dtype=torch.int64)
    torch.cumsum(counts, 0, out=off[1:])
    pos = torch.empty((max(int(off[-1]), 1),), dtype=torch.int32, device=words.device)
    off_d = off.to(words.device)
    _check(lib().mmt_mask_transition_positions(_p(words), n, H, W, _p(off_d), _p(pos), _stream()), "mmt_mask_transition_positions")
    return counts, pos[:int(off[-1])].cpu()


def mask_pair_intersections(dwords, drec, gwords, grec, H, W):
    """-> int32 (m, n) on the device: popcount(D_d & G_g), -1 where the two boxes do not overlap (mmt_mask_pair_intersections)"""
    m, n = _dev(dwords, "dwords").shape[0], _dev(gwords, "gwords").shape[0]
    out = torch.empty((m, n), dtype=torch.int32, device=dwords.device)
    _check(lib().mmt_mask_pair_intersections(_p(dwords), _p(drec), m, _p(gwords), _p(grec), n, H, W, _p(out), _stream()),
           "mmt_mask_pair_intersections")
    return out


# ---- mask NMS at inference (include/mmtpsm.h: mmt_mask_nms; csrc/masknms.hip)
MASK_NMS_MAX = 1024                         # detections of one call
MASK_NMS_MEASURES = {"iou": 0, "iomin": 1}  # the denominator: area_i + area_j - inter, or min(area_i, area_j)


def mask_nms_threshold_q20(thresh):
    """a threshold in (0, 1] as the library takes it: round(t * 2^20), halves up (0.3 acts as 314573 / 2^20)"""
    t = float(thresh)
    if not 0.0 < t <= 1.0:
        raise RuntimeError("mask_nms: a threshold in (0, 1], not %r" % (thresh,))
    q = int(math.floor(t * (1 << 20) + 0.5))   # (t * 2^20 is exact in binary floating point)
    if q < 1:
        raise RuntimeError("mask_nms: the threshold %r is below 2^-21 and quantises to zero" % (thresh,))
    return q


def mask_nms(words, rec, scores, labels, H, W, thresh, measure="iou", class_agnostic=False):
    """greedy mask NMS over the D masks (words, rec) of one H x W image (mmt_mask_nms): walk the detections by descending score
    (equal scores in row order); one is dropped when an earlier kept one of the same label (any label with class_agnostic)
    overlaps it -- popcount(mask_i & mask_j) * 2^20 >= round(thresh * 2^20) * den, den = the union (measure "iou") or the smaller
    area ("iomin"), all in integers.  -> (keep uint8 (D,) in row order, count int32 (1,)), both on the device; nothing is read
    back.  What the library refuses raises RuntimeError here, before any launch"""
    words, rec = _dev(words, "words"), _dev(rec, "rec")
    scores, labels = _dev(scores, "scores"), _dev(labels, "labels")
    H, W = int(H), int(W)
    D = words.shape[0]
    if measure not in MASK_NMS_MEASURES:
        raise RuntimeError("mask_nms: measure %r is not one of %s" % (measure, sorted(MASK_NMS_MEASURES)))
    tq = mask_nms_threshold_q20(thresh)
    if D > MASK_NMS_MAX:
        raise RuntimeError("mask_nms: %d detections, at most %d per call" % (D, MASK_NMS_MAX))
    if H <= 0 or W <= 0 or H * W >= (1 << 31):
        raise RuntimeError("masks of %d x %d: 0 < H * W < 2^31 only" % (H, W))
    if (words.dtype != torch.int64 or words.dim() != 2 or words.shape[1] != (H * W + 63) // 64 or rec.dtype != torch.int32
            or tuple(rec.shape) != (D, MASK_REC) or scores.numel() != D or labels.numel() != D):
        raise RuntimeError("mask_nms: words int64 (D, ceil(H*W/64)), records int32 (D, %d), D scores and D labels" % MASK_REC)
    order = torch.sort(scores.reshape(-1), descending=True, stable=True)[1].to(torch.int32)
    labels = labels.reshape(-1).to(torch.int32).contiguous()
    need = ctypes.c_int64(0)
    if lib().mmt_mask_nms_workspace(D, ctypes.byref(need)) != 0:
        raise RuntimeError("mmt_mask_nms_workspace refused %d detections" % D)
    ws = torch.empty((max(int(need.value), 1),), dtype=torch.uint8, device=words.device)
    keep = torch.empty((D,), dtype=torch.uint8, device=words.device)
    count = torch.empty((1,), dtype=torch.int32, device=words.device)
    _check(lib().mmt_mask_nms(_p(words.contiguous()), _p(rec.contiguous()), _p(order), _p(labels), D, H, W, tq,
                              MASK_NMS_MEASURES[measure], 1 if class_agnostic else 0, _p(ws), int(need.value), _p(keep), _p(count),
                              _stream()), "mmt_mask_nms")
    return keep, count


# ---- polygons at image size (include/mmtpsm.h: mmt_polygon_mask_words, mmt_mask_words_integral; csrc/polyfill.hip)
POLYGON_WS_WORDS = 1 << 25   # toggle workspace of one call, in 64-bit words (256 MiB); more polygons than fit go in several calls


def polygon_workspace_words(NP, H, W):
    """64-bit words of toggle workspace that mmt_polygon_mask_words wants for NP polygons in an H x W image (a query: no launch)"""
    n = ctypes.c_int64(0)
    if lib().mmt_polygon_mask_words_workspace(int(NP), int(H), int(W), ctypes.byref(n)) != 0:
        raise RuntimeError("polygon masks of %d x %d, %d polygons: 0 < H * W < 2^31 and NP >= 0 only" % (H, W, NP))
    return int(n.value)


def polygon_mask_words(xy, poly_off, inst_poly, H, W):
    """xy float32 vertices (x, y interleaved), poly_off int32 (NP + 1,), inst_poly int32 (G, 2): instance g is the union of
    polygons inst_poly[g, 0] .. inst_poly[g, 1] - 1 -> (words, records) of the G masks in an H x W image: what
    mask_pack(pycocotools' decode(merge(frPyObjects(...)))) gives, bit for bit (mmt_polygon_mask_words).  The toggle workspace of
    one call holds POLYGON_WS_WORDS words; instances whose polygons need more are rasterised in several calls"""
    xy = _dev(xy, "xy").float().contiguous()
    poly_off = _dev(poly_off, "poly_off").to(torch.int32).contiguous()
    inst_poly = _dev(inst_poly, "inst_poly").to(torch.int32).contiguous().reshape(-1, 2)
    H, W = int(H), int(W)
    G, NP = inst_poly.shape[0], poly_off.numel() - 1
    if NP < 0:
        raise RuntimeError("polygon_mask_words: poly_off holds NP + 1 offsets")
    words, rec = _mask_buffers(G, H, W, xy.device)
    if G == 0:
        return words, rec
    L = lib()

    def run(off, n_poly, rng, w, r, need):
        ws = torch.empty((max(need, 1),), dtype=torch.int64, device=xy.device)
        _check(L.mmt_polygon_mask_words(_p(xy), _p(off), n_poly, _p(rng), rng.shape[0], H, W, _p(ws), need, _p(w), _p(r), _stream()),
               "mmt_polygon_mask_words")

    need = polygon_workspace_words(NP, H, W)
    if need <= POLYGON_WS_WORDS:
        run(poly_off, NP, inst_poly, words, rec, need)
        return words, rec
    # consecutive instances whose polygons span a range that fits; an instance that does not fit alone gets what it needs
    host = inst_poly.cpu().tolist()
    if any(s < 0 or e < 0 or s > NP or e > NP for s, e in host):
        raise RuntimeError("polygon_mask_words: an inst_poly range outside [0, %d]" % NP)
    g0 = 0
    while g0 < G:
        lo = hi = None
        g1 = g0
        while g1 < G:
            s, e = host[g1]
            nlo, nhi = (lo, hi) if e <= s else ((s, e) if lo is None else (min(lo, s), max(hi, e)))
            if g1 > g0 and nlo is not None and polygon_workspace_words(nhi - nlo, H, W) > POLYGON_WS_WORDS:
                break
            lo, hi = nlo, nhi
            g1 += 1
        if lo is None:
            lo = hi = 0
        # (poly_off holds vertex positions in xy, so a slice of it serves as it is; the ranges move with it)
        part = inst_poly[g0:g1]
        full = (part[:, 1:2] > part[:, 0:1]).expand(-1, 2)          # an empty range may lie anywhere: it becomes [0, 0)
        rng = torch.where(full, part - lo, torch.zeros_like(part)).contiguous()
        run(poly_off[lo:hi + 1], hi - lo, rng, words[g0:g1], rec[g0:g1], polygon_workspace_words(hi - lo, H, W))
        g0 = g1
    return words, rec


def mask_words_integral(words, img_off, H, W):
    """words (G, ceil(H * W / 64)) of G masks in an H x W image, img_off: N + 1 host integers, image n owns masks
    img_off[n] .. img_off[n + 1] - 1 -> seg int32 (N, H, W) on the device, the number of masks that cover each pixel
    (mmt_mask_words_integral); what mask_pool reads"""
    words = _dev(words, "words")
    H, W = int(H), int(W)
    off = [int(v) for v in (img_off.tolist() if isinstance(img_off, torch.Tensor) else img_off)]
    if words.dtype != torch.int64 or words.dim() != 2 or words.shape[1] != (H * W + 63) // 64 or not words.is_contiguous():
        raise RuntimeError("mask_words_integral: contiguous int64 words (G, ceil(H * W / 64))")
    if len(off) < 1 or off[0] < 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] > words.shape[0]:
        raise RuntimeError("mask_words_integral: img_off must rise from a non-negative start and end within the %d masks" % words.shape[0])
    N = len(off) - 1
    seg = torch.empty((N, H, W), dtype=torch.int32, device=words.device)
    if N:
        arr = (ctypes.c_int32 * (N + 1))(*off)
        _check(lib().mmt_mask_words_integral(_p(words), ctypes.cast(arr, c_void_p), N, H, W, _p(seg), _stream()),
               "mmt_mask_words_integral")
    return seg


# ---- bitmap ground truth: geometry on mask words (include/mmtpsm.h: mmt_mask_words_resample / _targets; csrc/bitmasks.hip)
MASK_WORDS_MAX_SIDE, MASK_WORDS_MAX_AREA = 16384, 1 << 26


def _mask_words_of(words, H, W, what):
    words = _dev(words, "words")
    if words.dtype != torch.int64 or words.dim() != 2 or words.shape[1] != (H * W + 63) // 64 or not words.is_contiguous():
        raise RuntimeError("%s: contiguous int64 words (G, ceil(H * W / 64))" % what)
    return words


def mask_words_resample(words, H, W, window, flip, OH, OW):
    """words (G, ceil(H * W / 64)) of G masks in an H x W image, window (x0, y0, w, h) inside it, flip bit 0 left-right, bit 1
    top-bottom -> (words, records) of the window resampled to OH x OW by the integer bilinear rule of include/mmtpsm.h
    (mmt_mask_words_resample).  Sides up to 16384, areas up to 2^26; a refused call raises"""
    H, W, OH, OW, flip = int(H), int(W), int(OH), int(OW), int(flip)
    x0, y0, w, h = (int(v) for v in window)
    words = _mask_words_of(words, H, W, "mask_words_resample")
    G = words.shape[0]
    for a, b in ((H, W), (OH, OW)):
        if not (0 < a <= MASK_WORDS_MAX_SIDE and 0 < b <= MASK_WORDS_MAX_SIDE and a * b <= MASK_WORDS_MAX_AREA):
            raise RuntimeError("mask_words_resample: masks of %d x %d; sides up to %d and areas up to 2^26 only" % (a, b, MASK_WORDS_MAX_SIDE))
    out, rec = _mask_buffers(G, OH, OW, words.device)
    _check(lib().mmt_mask_words_resample(_p(words), G, H, W, x0, y0, w, h, flip, OH, OW, _p(out), _p(rec), _stream()),
           "mmt_mask_words_resample")
    return out, rec


def mask_words_targets(words, roi_inst, boxes, H, W, M):
    """words (G, ceil(H * W / 64)), roi_inst int32 (P,): the instance of each ROI, anything outside [0, G) -- -1 by convention -- for
    a ROI without one, boxes float32 (P, 4) xyxy -> float32 (P, M, M) in {0, 1}: the instance cropped to the box's window and
    resampled to M x M (mmt_mask_words_targets); zeros for a ROI without an instance or with a non-finite box.  Nothing is read
    back"""
    H, W, M = int(H), int(W), int(M)
    words = _mask_words_of(words, H, W, "mask_words_targets")
    roi_inst = _dev(roi_inst, "roi_inst")
    boxes = _dev(boxes, "boxes")
    if roi_inst.dtype != torch.int32 or roi_inst.dim() != 1:
        raise RuntimeError("mask_words_targets: roi_inst is int32 (P,)")
    if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] != roi_inst.shape[0]:
        raise RuntimeError("mask_words_targets: boxes are float32 (P, 4), one per roi_inst")
    roi_inst, boxes = roi_inst.contiguous(), boxes.contiguous()
    G, P = words.shape[0], boxes.shape[0]
    out = (torch.empty if G and P else torch.zeros)((P, M, M), dtype=torch.float32, device=boxes.device)
    _check(lib().mmt_mask_words_targets(_p(words), G, H, W, _p(roi_inst), _p(boxes), P, M, _p(out), _stream()),
           "mmt_mask_words_targets")
    return out
