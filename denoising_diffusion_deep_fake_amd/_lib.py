"""ctypes binding of libd3f_hip.so (include/d3f_hip.h).

The library is the product path: there is no CPU / eager fallback.  If it cannot be loaded
the import of any op raises, loudly.
"""
import ctypes as C
import os
import re
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["D3F_LIB"]) if os.environ.get("D3F_LIB") else _HERE / "csrc" / "libd3f_hip.so"  # D3F_LIB: profiling builds
HEADER_PATH = _HERE.parent / "include" / "d3f_hip.h"

F32, BF16, F32X3 = 0, 1, 2  # F32X3: fp32 tensors, contractions on the bf16 matrix pipe (exact 3-way split)
AUGMENT_NONE = -1  # D3F_AUGMENT_NONE: the `kind` of d3f_pool_batch_balanced_rng that warps nothing


# D3F_ACT_*: the head activation codes, by the canonical names Unet.activation holds
ACT_IDENTITY, ACT_SIGMOID, ACT_TANH, ACT_SOFTMAX, ACT_LOGSOFTMAX, ACT_CLAMP = range(6)
HEAD_ACTIVATIONS = {None: ACT_IDENTITY, "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH, "softmax2d": ACT_SOFTMAX,
                    "logsoftmax": ACT_LOGSOFTMAX, "clamp": ACT_CLAMP}


RESAMPLE_CUBIC, RESAMPLE_CUBIC_AA = 0, 1  # D3F_RESAMPLE_*: how the frame entries resize the crop to the network's size
COLOR_NONE, COLOR_MEANSTD = 0, 1  # D3F_COLOR_*: whether the full-frame entry matches the fake's colour before it pastes
COLOR_MATCH_MODES = {None: COLOR_NONE, "none": COLOR_NONE, "meanstd": COLOR_MEANSTD}


def color_match_mode(color_match):
    """the D3F_COLOR_* code of None / "none" / "meanstd"; anything else is a ValueError"""
    if not (color_match is None or isinstance(color_match, str)) or color_match not in COLOR_MATCH_MODES:
        raise ValueError(f"color_match is None, 'none' or 'meanstd', not {color_match!r}")
    return COLOR_MATCH_MODES[color_match]


BLEND_FEATHER, BLEND_MULTIBAND = 0, 1  # D3F_BLEND_*: how the full-frame entry blends the fake into the frame
BLEND_MODES = {None: BLEND_FEATHER, "feather": BLEND_FEATHER, "multiband": BLEND_MULTIBAND}
MULTIBAND_MAX_LEVELS = 6  # D3F_MULTIBAND_MAX_LEVELS


def blend_mode(blend):
    """the D3F_BLEND_* code of None / "feather" / "multiband"; anything else is a ValueError"""
    if not (blend is None or isinstance(blend, str)) or blend not in BLEND_MODES:
        raise ValueError(f"blend is None, 'feather' or 'multiband', not {blend!r}")
    return BLEND_MODES[blend]


def blend_levels(levels):
    """the levels of a multiband blend as an int; anything but an integer in 1..D3F_MULTIBAND_MAX_LEVELS is a ValueError"""
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MULTIBAND_MAX_LEVELS:
        raise ValueError(f"blend levels: an integer in 1..{MULTIBAND_MAX_LEVELS}, not {levels!r}")
    return levels


TEMPORAL_STRENGTH, TEMPORAL_THRESHOLD = 0.75, 8  # D3F_TEMPORAL_*: design choices, not measurements
# D3F_TRACK_*: the template tracker's limits, and its defaults (design choices, not measurements)
TRACK_MAX_SIDE, TRACK_MAX_SEARCH, TRACK_MAX_STRIDE, TRACK_MIN_SIDE = 64, 64, 32, 4
TRACK_TEMPLATE_SIDE, TRACK_SEARCH, TRACK_ADAPT, TRACK_LOST = 48, 16, 1, 16
TRACK_RELOST = 8  # D3F_TRACK_RELOST: the whole-frame search's threshold, half of TRACK_LOST (a design choice too)
TRACK_SCALE_PENALTY, TRACK_MAX_SCALE_PENALTY = 512, 65535  # D3F_TRACK_SCALE_PENALTY, in 1/4096 grey levels
# D3F_TRACK_ROT_*: the rotation search's step in hundredths of a degree, its range in degrees, its penalty, the largest index
TRACK_ROT_STEP, TRACK_ROT_MAX, TRACK_ROT_PENALTY, TRACK_ROT_MAX_INDEX = 200, 60, 512, 64


def temporal_setting(temporal, threshold=None):
    """(strength, threshold) of temporal = None (off: strength 0) / a strength / (strength, threshold); the strength as the
    float32 the handle will hold.  A strength outside [0, 1) or NaN, a threshold outside 1..255 and anything else are a
    ValueError.  threshold: what a bare strength gets (None: D3F_TEMPORAL_THRESHOLD)."""
    import struct
    thr = TEMPORAL_THRESHOLD if threshold is None else threshold
    if temporal is None:
        strength = 0.0
    elif isinstance(temporal, (tuple, list)):
        if len(temporal) != 2:
            raise ValueError(f"temporal is None, a strength or (strength, threshold), not {temporal!r}")
        strength, thr = temporal
    else:
        strength = temporal
    if isinstance(strength, bool) or not isinstance(strength, (int, float)):
        raise ValueError(f"temporal: the strength is a number in [0, 1), not {strength!r}")
    if isinstance(thr, bool) or not isinstance(thr, int) or not 1 <= thr <= 255:
        raise ValueError(f"temporal: the threshold is an integer in 1..255, not {thr!r}")
    if 0.0 <= strength < 1.0:  # (0.99999999 rounds to 1.0f: the second look refuses it)
        strength = struct.unpack("f", struct.pack("f", float(strength)))[0]
    if not 0.0 <= strength < 1.0:
        raise ValueError(f"temporal: the strength is a number in [0, 1), not {strength!r}")
    return (strength + 0.0, int(thr))



class D3FError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("B", "H", "W", "C0", "C1", "upsample0", "Cout", "KH", "KW", "stride", "pad", "CinReal")]


class BnDesc(C.Structure):
    """d3f_bn_desc: one BatchNorm layer as the engine describes it"""
    _fields_ = [("dtype", C.c_int32), ("C", C.c_int32), ("Cpad", C.c_int32), ("rows", C.c_int64),
                ("apply", C.c_int32), ("relu", C.c_int32), ("res", C.c_int32), ("mask", C.c_int32),
                ("fwd_rows", C.c_int32), ("fused_rows", C.c_int32), ("allow_fused", C.c_int32), ("plan_nets", C.c_int32)]


class BnPlan(C.Structure):
    """d3f_bn_plan: what bn_layer_plan made of a BnDesc"""
    _fields_ = [("fwd_fused", C.c_int32), ("bwd_fused", C.c_int32), ("reduce_blocks", C.c_int32), ("bwd_rows", C.c_int32),
                ("rows_per_block", C.c_int64), ("stat_floats", C.c_uint64), ("part_floats", C.c_uint64)]


class ConvLaunchPlan(C.Structure):
    """d3f_conv_launch_plan: the kernel form of one forward / data-gradient launch"""
    _fields_ = [(n, C.c_int32) for n in
                ("planned", "patch", "tile_bm", "tile_bn", "tiles_m", "tiles_n", "splitk", "par", "nz", "small_c",
                 "fast_addr", "sum2", "stat_rows")]


class ConvWgradPlan(C.Structure):
    """d3f_conv_wgrad_plan: one pass of a layer's weight gradient"""
    _fields_ = [(n, C.c_int32) for n in ("part", "cls", "patch", "splits", "chunks_per_split", "tile", "tiles")]


class ConvPlan(C.Structure):
    """d3f_conv_plan: what conv_layer_plan made of a ConvDesc"""
    _fields_ = [("upfold", C.c_int32), ("parity", C.c_int32), ("wino", C.c_int32), ("wino_rows", C.c_int32),
                ("fwd", ConvLaunchPlan), ("dgrad", ConvLaunchPlan), ("dgrad_lo", ConvLaunchPlan),
                ("wgrad_parts", C.c_int32), ("wgrad", ConvWgradPlan * 2)]


BN_COEF_ROWS = 7  # D3F_BN_COEF_ROWS: mean invstd scale shift k0 k1 k2

_p, _i, _i64, _f, _sz, _dbl = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t, C.c_double
_u64, _u32p, _i32p = C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
_desc = C.POINTER(ConvDesc)
_bnd, _bnp = C.POINTER(BnDesc), C.POINTER(BnPlan)
_cvp = C.POINTER(ConvPlan)

# name -> (restype, argtypes); must list every symbol include/d3f_hip.h declares
PROTOTYPES = {
    "d3f_version": (_i, []),
    "d3f_last_error": (C.c_char_p, []),
    "d3f_source_digest": (C.c_char_p, []),
    "d3f_profile_enable": (_i, [_i]),
    "d3f_profile_classes": (_i, [_i]),
    "d3f_profile_collect": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "d3f_unet_create": (_i, [C.c_char_p, _i, _i, _i, _i, _i, _i, C.POINTER(_p)]),
    "d3f_unet_destroy": (_i, [_p]),
    "d3f_unet_create_nets": (_i, [C.c_char_p, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_p)]),
    "d3f_unet_nets": (_i, [_p]),
    "d3f_unet_net_workspace_stride": (_sz, [_p]),
    "d3f_unet_pair_pack_weights": (_i, [_p, C.POINTER(_p), _p, _p]),
    "d3f_unet_pair_forward": (_i, [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_p), C.POINTER(_p), _p, _p]),
    "d3f_unet_pair_backward": (_i, [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_p), _p, _i, _i, _i, _p]),
    "d3f_unet_set_head_activation": (_i, [_p, _i]),
    "d3f_unet_head_activation": (_i, [_p]),
    "d3f_unet_set_frame_resample": (_i, [_p, _i]),
    "d3f_unet_frame_resample": (_i, [_p]),
    "d3f_unet_set_frame_color_match": (_i, [_p, _i]),
    "d3f_unet_frame_color_match": (_i, [_p]),
    "d3f_unet_set_frame_temporal": (_i, [_p, _f, _i]),
    "d3f_unet_frame_temporal": (_i, [_p, C.POINTER(_f), C.POINTER(_i)]),
    "d3f_unet_frame_temporal_reset": (_i, [_p, _p]),
    "d3f_unet_set_frame_blend": (_i, [_p, _i, _i]),
    "d3f_unet_frame_blend": (_i, [_p, C.POINTER(_i)]),
    "d3f_unet_num_params": (_i, [_p]),
    "d3f_unet_param_info": (_i, [_p, _i, C.c_char_p, _i, C.POINTER(C.c_int32), C.POINTER(_i), C.POINTER(_i64)]),
    "d3f_unet_param_floats": (_i64, [_p]),
    "d3f_unet_num_bn": (_i, [_p]),
    "d3f_unet_bn_info": (_i, [_p, _i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(_i64), C.POINTER(_i64)]),
    "d3f_unet_bnstat_floats": (_i64, [_p]),
    "d3f_unet_workspace_bytes": (_sz, [_p]),
    "d3f_unet_forward_flops": (_dbl, [_p]),
    "d3f_unet_backward_flops": (_dbl, [_p]),
    "d3f_unet_pack_weights": (_i, [_p, _p, _p, _p]),
    "d3f_unet_forward": (_i, [_p, _p, _p, _p, _p, _p, _i, _p]),
    "d3f_unet_forward_graph": (_i, [_p, _p, _p, _p, _p, _p, _p]),
    "d3f_noise_blend_fixed": (_i, [_p, _p, _p, _p, _i, _i64, _p]),
    "d3f_l1_per_image_workspace_bytes": (_sz, [_i]),
    "d3f_l1_per_image": (_i, [_p, _p, _p, _p, _i, _i64, _p]),
    "d3f_l1_per_image_scatter": (_i, [_p, _p, _p, _p, _i, _p, _i, _i64, _p]),
    "d3f_quality_per_image_workspace_bytes": (_sz, [_i, _i, _i]),
    "d3f_quality_per_image_scatter": (_i, [_p, _p, _f, _f, _p, _p, _i, _p, _i, _i, _i, _p]),
    "d3f_difficulty_classes_workspace_bytes": (_sz, [_i]),
    "d3f_difficulty_classes": (_i, [_p, _i, _i, _p, _p, _p, _p, _p]),
    "d3f_difficulty_histogram_u8_workspace_bytes": (_sz, [_i]),
    "d3f_difficulty_histogram_u8": (_i, [_p, _i, _i, _p, _p, _p, _i, _i, _p, _p]),
    "d3f_affine_warp": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "d3f_u8rgb_normalise": (_i, [_p, _p, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _p]),
    "d3f_unet_predict_u8": (_i, [_p, _p, _p, _p, _p, C.POINTER(_f), C.POINTER(_f), _p, _i, _p]),
    "d3f_unet_predict_frames_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, C.POINTER(_f), C.POINTER(_f), _p, _i, _p]),
    "d3f_crop_resize_cubic_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _p, _i, _i, _i64, _p]),
    "d3f_crop_resize_cubic_aa_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _p, _i, _i, _i64, _p]),
    "d3f_paste_resize_cubic_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p]),
    "d3f_channel_sums_u8": (_i, [_p, _i, _i, _i, _i64, _p, _p]),
    "d3f_color_match_coef": (_i, [_p, _p, _i, _i64, _p, _p]),
    "d3f_paste_resize_cubic_color_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "d3f_paste_multiband_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "d3f_paste_multiband_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p, _i64, _p, _p]),
    "d3f_paste_multiband_color_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _i64, _p, _p]),
    "d3f_paste_multiband_boxes_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, C.POINTER(C.c_int32), _i, _i, _p, _i64, _p, _p]),
    "d3f_paste_multiband_color_boxes_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, C.POINTER(C.c_int32), _i, _i, _p, _p, _i64, _p,
                                                _p]),
    "d3f_temporal_filter_u8": (_i, [_p, _i64, _p, _i64, _i, _i, _i, _p, _p, _p, _f, _i, _p]),
    "d3f_color_coef_smooth": (_i, [_p, _p, _i, _i64, _f, _p, _p, _p, _p]),
    "d3f_temporal_flag_set": (_i, [_p, _i, _p]),
    "d3f_unet_predict_frames_full_u8": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p, C.POINTER(_f), C.POINTER(_f),
                                             _p, _i, _p]),
    # a box per frame: boxes is HOST memory, [B][4] int32
    "d3f_crop_resize_cubic_boxes_u8": (_i, [_p, _i, _i, _i, C.POINTER(C.c_int32), _p, _i, _i, _i64, _p]),
    "d3f_crop_resize_cubic_aa_boxes_u8": (_i, [_p, _i, _i, _i, C.POINTER(C.c_int32), _p, _i, _i, _i64, _p]),
    "d3f_paste_resize_cubic_boxes_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, C.POINTER(C.c_int32), _i, _p, _p]),
    "d3f_paste_resize_cubic_color_boxes_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, C.POINTER(C.c_int32), _i, _p, _p, _p]),
    "d3f_unet_predict_frames_boxes_u8": (_i, [_p, _p, _p, _p, _i, _i, C.POINTER(C.c_int32), _p, C.POINTER(_f), C.POINTER(_f),
                                              _p, _i, _p]),
    "d3f_unet_predict_frames_full_boxes_u8": (_i, [_p, _p, _p, _p, _i, _i, C.POINTER(C.c_int32), _i, _p, _p, C.POINTER(_f),
                                                   C.POINTER(_f), _p, _i, _p]),
    # ... and a rotation per frame: rot is HOST memory, [B][2] int32 (c16, s16)
    "d3f_crop_resize_cubic_rboxes_u8": (_i, [_p, _i, _i, _i, _i32p, _i32p, _p, _i, _i, _i64, _p]),
    "d3f_crop_resize_cubic_rboxes_u8_nhwc": (_i, [_i, _p, _i, _i, _i, _i32p, _i32p, _p, _i, _i, _i64, _p, _i, C.POINTER(_f),
                                                  C.POINTER(_f), _p]),
    "d3f_paste_resize_cubic_rboxes_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, _i32p, _i32p, _i, _p, _p]),
    "d3f_paste_resize_cubic_color_rboxes_u8": (_i, [_p, _i, _i, _i, _i64, _p, _i, _i, _i32p, _i32p, _i, _p, _p, _p]),
    "d3f_unet_predict_frames_rboxes_u8": (_i, [_p, _p, _p, _p, _i, _i, _i32p, _i32p, _p, C.POINTER(_f), C.POINTER(_f), _p, _i,
                                               _p]),
    "d3f_unet_predict_frames_full_rboxes_u8": (_i, [_p, _p, _p, _p, _i, _i, _i32p, _i32p, _i, _p, _p, C.POINTER(_f),
                                                    C.POINTER(_f), _p, _i, _p]),
    "d3f_gray_decimate_u8": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "d3f_track_seed_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "d3f_track_search_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "d3f_track_template_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    # keys: uint64 [B] on the device
    "d3f_track_global_u8": (_i, [_p, _i, _i, _i, _i, _i, _p, _p, _p]),
    "d3f_track_search_reacq_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "d3f_track_template_reacq_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "d3f_track_seed_scale_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "d3f_track_search_scale_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p]),
    "d3f_track_template_scale_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    # table is HOST memory, [2 amax + 1][2] int32
    "d3f_track_seed_rot_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _p]),
    "d3f_track_search_rot_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i32p, _p, _p, _p, _p]),
    "d3f_track_template_rot_u8": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i32p, _p, _p, _p, _p, _p]),
    "d3f_image_grid_shape": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_int32)]),
    "d3f_image_grid_u8": (_i, [C.POINTER(_p), _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _p, _p]),
    "d3f_unet_num_segments": (_i, [_p]),
    "d3f_unet_plan_counts": (_i, [_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "d3f_unet_segment_range": (_i, [_p, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "d3f_unet_backward": (_i, [_p, _p, _p, _p, _p, _i, _i, _p]),
    "d3f_unet_backward_nojoin": (_i, [_p, _p, _p, _p, _p, _i, _i, _p]),
    "d3f_unet_side_stream": (_i, [_p, C.POINTER(_p)]),
    "d3f_unet_backward_join": (_i, [_p, _p]),
    "d3f_adam_coefficients": (_i, [_f, _f, _f, _f, _i, _f, C.POINTER(_f)]),
    "d3f_unet_train_step": (_i, [_p, _p, _f, _f, _f, _p, _i, _p]),
    "d3f_unet_set_bn_sync": (_i, [_p, _p, _p, _i]),
    "d3f_unet_export": (_i, [_p, C.c_char_p, _p, _p, _p]),
    "d3f_unet_export_shape": (_i, [_p, C.c_char_p, C.POINTER(C.c_int32)]),
    "d3f_conv_upsample_folded": (_i, [_i, _p]),
    "d3f_conv_upsample_summed": (_i, [_i, _p]),
    "d3f_conv_packed_bytes": (_sz, [_i, _desc, _i]),
    "d3f_conv_pack_weights": (_i, [_i, _desc, _p, _p, _p, _p]),
    "d3f_conv_workspace_bytes": (_sz, [_i, _desc, _i]),
    "d3f_conv_stats_floats": (_sz, [_i, _desc, _i, C.POINTER(_i)]),
    "d3f_conv_forward": (_i, [_i, _desc, _p, _p, _p, _p, _p, _p, _p]),
    "d3f_conv_winograd_applies": (_i, [_i, _desc]),
    "d3f_conv_winograd_filter_bytes": (_sz, [_desc]),
    "d3f_conv_winograd_stats_floats": (_sz, [_desc, C.POINTER(_i)]),
    "d3f_conv_winograd_pack": (_i, [_desc, _p, _p, _p]),
    "d3f_conv_winograd_forward": (_i, [_desc, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
    "d3f_conv_backward_data": (_i, [_i, _desc, _p, _p, _p, _p, _i, _i, _p, _p]),
    "d3f_conv_backward_weight_workspace_bytes": (_sz, [_i, _desc]),
    "d3f_conv_backward_weight": (_i, [_i, _desc, _p, _p, _p, _p, _p, _p]),
    "d3f_conv_layer_plan": (_i, [_i, _desc, _i, _cvp]),
    "d3f_unet_num_conv_layers": (_i, [_p]),
    "d3f_unet_conv_layer": (_i, [_p, _i, _desc, _cvp]),
    "d3f_bn_finalize": (_i, [_p, _i, _i, _i64, _p, _p, _p, _p, _p, _p]),
    "d3f_bn_apply": (_i, [_i, _p, _p, _i, _i64, _p, _i, _p, _p]),
    "d3f_bn_backward_workspace_bytes": (_sz, [_i, _i, _i64]),
    "d3f_bn_backward": (_i, [_i, _p, _p, _p, _p, _p, _i, _i64, _p, _p, _p, _p, _p, _p]),
    "d3f_bn_layer_plan": (_i, [_bnd, _bnp]),
    "d3f_bn_layer_forward": (_i, [_bnd, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "d3f_bn_layer_backward": (_i, [_bnd, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p]),
    "d3f_unet_bn_layer": (_i, [_p, _i, _bnd, _bnp]),
    "d3f_head_activation_forward": (_i, [_i, _p, _p, _i, _i, _i, _i, _p]),
    "d3f_head_activation_backward": (_i, [_i, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "d3f_maxpool3x3s2_forward": (_i, [_i, _p, _p, _p, _i, _i, _i, _i, _p]),
    "d3f_maxpool3x3s2_backward": (_i, [_i, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "d3f_upsample2x_backward": (_i, [_i, _p, _p, _i, _i, _i, _i, _p]),
    "d3f_nchw_to_nhwc": (_i, [_i, _p, _p, _i, _i, _i, _i, _i, _p]),
    "d3f_nhwc_to_nchw": (_i, [_i, _p, _p, _i, _i, _i, _i, _i, _p]),
    "d3f_noise_blend": (_i, [_p, _p, _p, _f, _p, _p, _i, _i64, _p]),
    "d3f_mse_ssim_loss_workspace_bytes": (_sz, [_i, _i, _i]),
    "d3f_mse_ssim_loss": (_i, [_p, _p, _f, _f, _p, _p, _p, _i, _i, _i, _p]),
    "d3f_adam_step": (_i, [_p, _p, _p, _p, _i64, _f, _f, _f, _f, _i, _f, _p]),
    "d3f_ema_lerp": (_i, [_p, _p, _i64, _f, _p]),
    "d3f_philox4x32_10": (_i, [_u32p, _u32p, _u32p]),
    "d3f_noise_blend_rng": (_i, [_p, _u64, _u64, _f, _p, _p, _i, _i64, _p]),
    "d3f_noise_blend_fixed_rng": (_i, [_p, _u64, _u64, _p, _p, _i, _i64, _p]),
    "d3f_noise_blend_fixed_index_rng": (_i, [_p, _u64, _u64, _p, _p, _p, _i, _i64, _p]),
    "d3f_noise_draw": (_i, [_u64, _u64, _p, _p, _i, _i64, _p]),
    "d3f_affine_warp_rng": (_i, [_p, _p, _u64, _u64, _i, C.POINTER(_f), _i, _i, _i, _i, _p]),
    "d3f_affine_theta_draw": (_i, [_u64, _u64, _i, C.POINTER(_f), _p, _p, _i, _i, _i, _p]),
    "d3f_pool_batch": (_i, [_p, _i64, _p, _p, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _p, _p, _p]),
    "d3f_pool_batch_rng": (_i, [_p, _i64, _p, _p, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _u64, _u64, _i, C.POINTER(_f), _p]),
    "d3f_pool_batch_balanced_rng": (_i, [_p, _i64, _p, _p, _i, _p, _p, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _u64, _u64, _i,
                                         C.POINTER(_f), _p]),
    "d3f_balanced_index_draw": (_i, [_p, _p, _i, _u64, _u64, _p, _i, _p]),
}

# d3f_allreduce_fn: int (*)(void* ctx, float* data, int64_t count, void* stream)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)

_lib = None


def header_symbols():
    """Function names declared in include/d3f_hip.h."""
    text = HEADER_PATH.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(d3f_[a-z0-9_]+)\s*\(", text)))


def sources_present():
    """are the kernel sources and the public header the digest covers next to the library?"""
    return HEADER_PATH.exists() and any((_HERE / "csrc").glob("*.hip"))


def source_digest():
    """sha256 (first 16 hex digits) over the kernel sources csrc/*.hip, csrc/*.h and the public header -- ties a
    counter file under profiles/ to the code it was collected on (the GPU box has no .git to ask)."""
    import hashlib
    h = hashlib.sha256()
    files = sorted((_HERE / "csrc").glob("*.hip")) + sorted((_HERE / "csrc").glob("*.h")) + [HEADER_PATH]
    for f in files:
        h.update(f.name.encode())
        h.update(f.read_bytes())
    return h.hexdigest()[:16]


def lib():
    """Load (once) and return the ctypes handle; raises D3FError if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise D3FError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {LIB_PATH.parent}` (hipcc, gfx950). There is no CPU fallback.")
    handle = C.CDLL(str(LIB_PATH))
    for name, (res, args) in PROTOTYPES.items():
        if os.environ.get("D3F_LIB") and not hasattr(handle, name):
            continue  # an older profiling / A-B build given explicitly: calling the missing entry point fails loudly
        fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if not os.environ.get("D3F_LIB") and sources_present():
        # (a layout without the sources next to the library -- a non-editable install that ships only the .so -- has
        # nothing to compare against: the library is taken as built)
        built, here = handle.d3f_source_digest().decode(), source_digest()
        if built != here:
            raise D3FError(
                f"{LIB_PATH} was built from other sources (digest {built}) than the ones next to it ({here}): "
                f"rebuild it with `make -C {LIB_PATH.parent}`, or name a variant build explicitly through D3F_LIB")
    _lib = handle
    return _lib


def built_digest():
    """Digest baked into the loaded library (equals source_digest() unless D3F_LIB names a variant build)."""
    handle = lib()
    return handle.d3f_source_digest().decode() if hasattr(handle, "d3f_source_digest") else None


def check(rc):
    if rc != 0:
        raise D3FError(lib().d3f_last_error().decode("utf-8", "replace"))


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def ptr2(a, b):
    """the `T* const x[2]` argument of the pair entry points: the two networks' buffers"""
    return (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
