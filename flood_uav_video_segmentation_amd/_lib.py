"""ctypes binding of libfloodseg.so (the C ABI declared in include/floodseg.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, importing
the ops raises.  torch is imported first on purpose -- torch ships its own libamdhip64 (same
soname), and device pointers / streams are only interchangeable inside ONE HIP runtime instance.
"""
import collections
import ctypes
import functools
import os

import torch  # noqa: F401  (must precede CDLL so both share torch's HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfloodseg.so")

c_float_p = ctypes.POINTER(ctypes.c_float)
c_void = ctypes.c_void_p
c_int = ctypes.c_int
c_i64 = ctypes.c_int64
c_f32 = ctypes.c_float


class FsConfig(ctypes.Structure):
    _fields_ = [("arch", c_int), ("layers", c_int), ("classes", c_int), ("patch", c_int), ("d_model", c_int),
                ("n_layers", c_int), ("dec_layers", c_int), ("image_size", c_int), ("flags", c_int), ("winograd_tile", c_int)]


ARCH_PSPNET = 0
ARCH_DEEPLABV3 = 1
ARCH_SEGMENTER = 2
OPT_NO_WINOGRAD = 1      # FS_OPT_NO_WINOGRAD
OPT_NO_FUSED_HEAD = 2    # FS_OPT_NO_FUSED_HEAD
OPT_NO_FUSED_SHORTCUT = 4  # FS_OPT_NO_FUSED_SHORTCUT
OPT_NO_FUSED_WINOGRAD = 8  # FS_OPT_NO_FUSED_WINOGRAD
OPT_NO_SPLIT_BF16 = 16  # FS_OPT_NO_SPLIT_BF16
OPT_NO_RES_TOUCH = 128  # FS_OPT_NO_RES_TOUCH
OPT_NO_FUSED_POOL = 256  # FS_OPT_NO_FUSED_POOL
OPT_NO_FUSED_QKV = 1024  # FS_OPT_NO_FUSED_QKV
CONV_CHUNK_MAJOR = 0x400  # FS_CONV_CHUNK_MAJOR

# name -> (restype, argtypes); must list every symbol of include/floodseg.h (+ fs_test_hooks of include/floodseg_test.h)
_SIGNATURES = {
    "fs_version": (c_int, []),
    "fs_last_error": (ctypes.c_char_p, []),
    "fs_create": (c_int, [ctypes.POINTER(FsConfig), ctypes.POINTER(c_void)]),
    "fs_destroy": (c_int, [c_void]),
    "fs_load_weight": (c_int, [c_void, ctypes.c_char_p, c_void, ctypes.POINTER(c_i64), c_int, c_int, c_void]),
    "fs_finalize": (c_int, [c_void, c_void]),
    "fs_feature_shape": (c_int, [c_void, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "fs_workspace_bytes": (ctypes.c_size_t, [c_void, c_int, c_int, c_int]),
    "fs_reserve": (c_int, [c_void, c_int, c_int, c_int, c_void]),
    "fs_reserved_bytes": (ctypes.c_size_t, [c_void]),
    "fs_encoder_forward": (c_int, [c_void, c_void, c_int, c_int, c_int, c_void, c_void]),
    "fs_decoder_forward": (c_int, [c_void, c_void, c_int, c_int, c_int, c_void, c_void]),
    "fs_segment_forward": (c_int, [c_void, c_void, c_int, c_int, c_int, c_void, c_void]),
    "fs_encoder_forward2": (c_int, [c_void, c_void, c_int, c_void, c_int, c_int, c_int, c_void, c_void]),
    "fs_segment_forward2": (c_int, [c_void, c_void, c_int, c_void, c_int, c_int, c_int, c_void, c_void]),
    "fs_segment_crops": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int, c_int,
                                 c_void, c_void]),
    "fs_profile_enable": (c_int, [c_void, c_int]),
    "fs_profile_dump": (c_int, [c_void, ctypes.c_char_p, ctypes.c_size_t]),
    "fs_grid_sample_nchw": (c_int, [c_void, c_int, c_int, c_int, c_int, c_void, c_int, c_int, c_void, c_int, c_void]),
    "fs_grid_sample_nhwc": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_int, c_int, c_void, c_int, c_int, c_void]),
    "fs_resize_bilinear_nchw": (c_int, [c_void, c_int, c_int, c_int, c_void, c_int, c_int, c_int, c_void]),
    "fs_resize_bilinear_nhwc": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_int, c_int, c_int, c_int, c_void]),
    "fs_blend": (c_int, [c_void, c_f32, c_void, c_f32, c_void, c_i64, c_void]),
    "fs_seg_tail": (c_int, [c_void, c_void, ctypes.POINTER(c_void), ctypes.POINTER(c_void), c_int, c_int, c_int, c_int, c_int,
                            c_int, c_int, c_int, c_int, c_void, c_void, c_void, c_void]),
    "fs_feat_tail": (c_int, [c_void, c_void, c_int, c_int, c_int, ctypes.POINTER(c_void), ctypes.POINTER(c_void), c_int, c_int, c_void, c_int, c_int,
                             c_int, c_int, c_void, c_void, c_void]),
    "fs_seg_tail_accumulate": (c_int, [c_void, c_void, ctypes.POINTER(c_void), ctypes.POINTER(c_void), c_int, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_int, c_int, c_void, c_void, c_int, c_int, c_int, c_int, c_void, c_void]),
    "fs_canvas_resize_argmax": (c_int, [c_void, c_int, c_int, c_int, c_int, c_void, c_int, c_int, c_void]),
    "fs_crop_grids": (c_int, [ctypes.POINTER(c_void), c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                              c_int, c_int, c_void, c_void]),
    "fs_crops_fuse": (c_int, [c_void, c_void, c_void, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)] + [c_int] * 9 + [c_void, c_void, c_int, c_int,
                              c_void, c_void]),
    "fs_argmax_u8": (c_int, [c_void, c_int, c_int, c_i64, c_void, c_void]),
    "fs_resize_crop": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void, c_void, c_int, c_int, c_void]),
    "fs_resize_argmax_u8": (c_int, [c_void, c_int, c_int, c_int, c_int, c_void, c_int, c_int, c_void]),
    "fs_iou_hist": (c_int, [c_void, c_void, c_i64, c_int, c_int, c_void, c_void]),
    "fs_colorize": (c_int, [c_void, c_void, c_int, c_void, c_i64, c_void]),
    "fs_mv_to_grids": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void, c_void, c_void, c_void]),
    "fs_softmax_accumulate": (c_int, [c_void, c_int, c_int, c_int, c_int, c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    "fs_canvas_finish": (c_int, [c_void, c_void, c_int, c_int, c_i64, c_void, c_void]),
    "fs_ms_prepare": (c_int, [c_void] + [c_int] * 6 + [c_float_p, c_float_p, c_void, c_int, c_void]),
    "fs_ms_fuse": (c_int, [c_void, c_void, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)] + [c_int] * 9 + [c_void, c_void] + [c_int] * 4
                   + [c_void, c_void]),
    "fs_test_hooks": (c_void, []),
}

# members of fs_test_api (include/floodseg_test.h), in declaration order after `size`: name -> (restype, argtypes).  Reached as
# load().fs_<name>(...) like any exported function -- tests and tools do not care that they come from the table fs_test_hooks() returns.
_HOOKS = [
    ("pack_conv_weight", c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    ("conv2d_nhwc", c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_int, c_void, c_int] + [c_int] * 12 + [c_void]),
    ("split_bf16x3", c_int, [c_void, c_i64, c_void, c_void]),
    ("conv2d_nhwc_split", c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_int, c_void, c_int] + [c_int] * 12 + [c_void]),
    ("attention_workspace_floats", ctypes.c_size_t, [c_int] * 4),
    ("attention", c_int, [c_void, c_void, c_int, c_int, c_int, c_f32, c_int, c_void, c_void]),
    ("winograd_workspace_floats", ctypes.c_size_t, [c_int] * 7),
    ("conv3x3_winograd_nhwc", c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_int] + [c_int] * 8 + [c_void, c_void]),
    ("winograd_fused_workspace_floats", ctypes.c_size_t, [c_int, c_int]),
    ("conv3x3_winograd_fused_nhwc", c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_int] + [c_int] * 7 + [c_void, c_void]),
    ("conv3x3_winograd_fused_pool_nhwc", c_int, [c_void, c_int, c_void, c_void, c_void, c_void] + [c_int] * 5 + [c_void, c_void]),
    ("stem_conv_nchw", c_int, [c_void, c_void, c_void, c_void, c_void] + [c_int] * 8 + [c_void]),
    ("stem_conv_nchw_split", c_int, [c_void, c_void, c_void, c_void, c_void] + [c_int] * 8 + [c_void]),
    ("maxpool3x3s2_nhwc", c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    ("adaptive_avgpool_nhwc", c_int, [c_void, c_int, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    ("nchw_to_nhwc", c_int, [c_void, c_void, c_int, c_int, c_int, c_void]),
    ("nhwc_to_nchw", c_int, [c_void, c_void, c_int, c_int, c_int, c_void]),
    ("layernorm", c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    ("linear_splits", c_int, [c_int] * 5),
    ("linear", c_int, [c_void] * 6 + [c_int] * 6 + [c_void] * 4 + [c_void]),
    ("qkv_attention_workspace_floats", ctypes.c_size_t, [c_int] * 3),
    ("qkv_attention", c_int, [c_void] * 4 + [c_int] * 3 + [c_void, c_void, c_int, c_void, c_void]),
    ("mask_head", c_int, [c_void] * 5 + [c_int] * 4 + [c_void]),
    ("patchify", c_int, [c_void, c_void, c_int, c_void, c_int, c_int, c_int, c_int, c_void]),
    ("vit_assemble", c_int, [c_void] * 4 + [c_int] * 3 + [c_void]),
    ("dec_assemble", c_int, [c_void] * 3 + [c_int] * 4 + [c_void]),
    ("concat_scaled_filters", c_int, [c_void, c_void, c_void, c_int, c_void, c_void, c_void, c_int, c_void, c_void, c_int, c_void]),
    ("pack_slice_tap_major", c_int, [c_void, c_void] + [c_int] * 5 + [c_void]),
    ("dual_conv", c_int, [c_void, c_int, c_void, c_int, c_void, c_void, c_void, c_void] + [c_int] * 12 + [c_void]),
    ("pyramid_pool", c_int, [c_void, c_int, c_void] + [c_int] * 4 + [c_void]),
    ("rowdot_batch", c_int, [c_int] + [c_void] * 6 + [c_int] * 5 + [c_void]),
    ("upsample_into", c_int, [c_void, c_int, c_int, c_void] + [c_int] * 6 + [c_void]),
    ("classifier_nchw", c_int, [c_void, c_int, c_void, c_void, c_void] + [c_int] * 4 + [c_void]),
    ("ppm_term_scratch_floats", ctypes.c_size_t, [c_int] * 3),
    ("ppm_term_classify", c_int, [c_void, c_int] + [c_void] * 7 + [c_int] * 5 + [c_void] * 3 + [c_int, c_void, c_void]),
    ("ppm_head_workspace_floats", ctypes.c_size_t, [c_int] * 3),
    ("ppm_head", c_int, [c_void, c_int, c_void, c_int] + [c_void] * 5 + [c_int] * 5 + [c_void] * 3 + [c_int, c_void, c_void]),
    ("block_match", c_int, [c_void, c_void] + [c_int] * 5 + [c_void, c_void, c_void]),
]

# members of fs_ext_api (include/floodseg_test.h), the append-only extension table the library places right behind the frozen
# fs_test_api, in declaration order after `magic` and `size`; reached as load().fs_<name>(...) like the hooks above
_EXT_HOOKS = [
    ("frame_prepare", c_int, [c_void, c_void, c_void] + [c_int] * 5 + [c_void, c_void, c_void, c_int, c_int, c_void]),
    ("frame_compose", c_int, [c_void, c_int, c_int, c_void, c_int, c_void, c_void, c_void] + [c_int] * 5 + [c_void, c_void, c_void] + [c_int] * 3 + [c_void]),
]
EXT_MAGIC = 0x4653455854414231  # FS_EXT_MAGIC

# members of fs_ext2_api, the third table (append-only, behind the two frozen ones), in declaration order after `magic` and `size`
_EXT2_HOOKS = [
    ("block_match_modes", c_int, [c_void, c_void] + [c_int] * 7 + [c_void, c_void, c_void, c_void, c_void]),
    ("window_weights", c_int, [c_int, ctypes.POINTER(c_void), c_void, c_void, c_void]),
    ("seg_tail_weighted", c_int, [c_void, c_void, ctypes.POINTER(c_void), ctypes.POINTER(c_void)] + [c_int] * 9 + [c_void] * 4 + [c_int] * 4
     + [c_void, c_void, c_void]),
    ("crops_fuse_weighted", c_int, [c_void, c_void, c_void, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)] + [c_int] * 9
     + [c_void, c_void, c_int, c_int, c_void, c_void, c_void]),
    ("feat_tail_weighted", c_int, [c_void, c_void, c_int, c_int, c_int, ctypes.POINTER(c_void), ctypes.POINTER(c_void), c_int, c_int, c_void, c_int,
                                   c_int, c_int, c_int, c_void, c_void, c_void, c_void]),
    ("mask_confidence", c_int, [c_void] + [c_int] * 4 + [c_void, c_void, c_int, c_int, c_void]),
    ("canvas_confidence", c_int, [c_void] + [c_int] * 4 + [c_void, c_void, c_int, c_int, c_void]),
    ("frame_report", c_int, [c_void, c_void] + [c_int] * 5 + [c_void, c_void]),
    ("mask_regions", c_int, [c_void] + [c_int] * 5 + [c_void, c_void]),
    ("region_table", c_int, [c_void, c_void, c_void] + [c_int] * 6 + [c_void] * 5),
    ("region_filter", c_int, [c_void, c_void, c_void] + [c_int] * 6 + [c_void, c_void, c_void]),
    ("region_links", c_int, [c_void] * 6 + [c_int] * 6 + [c_void] * 5),
    ("region_tracks", c_int, [c_void] * 4 + [c_int] * 2 + [c_void] * 3),
    ("region_links_mc", c_int, [c_void] * 8 + [c_int] * 8 + [c_void] * 5),
]
EXT2_MAGIC = 0x4653455854414232  # FS_EXT2_MAGIC

# members of fs_ext3_api, the fourth table (append-only, behind the three frozen ones), in declaration order after `magic` and `size`
_EXT3_HOOKS = [
    ("region_outlines", c_int, [c_void] + [c_int] * 7 + [c_void] * 6),
]
EXT3_MAGIC = 0x4653455854414233  # FS_EXT3_MAGIC

# members of fs_ext4_api, the fifth table (append-only, behind the four frozen ones), in declaration order after `magic` and `size`
_EXT4_HOOKS = [
    ("outline_simplify", c_int, [c_void] * 3 + [c_int] * 5 + [c_void] * 5),
]
EXT4_MAGIC = 0x4653455854414234  # FS_EXT4_MAGIC

# members of fs_ext5_api, the sixth table (append-only, behind the five frozen ones), in declaration order after `magic` and `size`
_EXT5_HOOKS = [
    ("frame_compose_regions", c_int, [c_void, c_int, c_int, c_void, c_int, c_void, c_void, c_void] + [c_int] * 5 + [c_void, c_void, c_void] + [c_int] * 3
     + [c_void] * 4 + [c_int, c_void, c_int, c_void, c_int, c_int, c_i64, ctypes.c_uint32, ctypes.c_uint32, c_void, c_void]),
]
EXT5_MAGIC = 0x4653455854414235  # FS_EXT5_MAGIC

# members of fs_ext6_api, the seventh table (append-only, behind the six frozen ones), in declaration order after `magic` and `size`
_EXT6_HOOKS = [
    ("mask_stabilize", c_int, [c_void] * 4 + [c_int] * 9 + [c_void] * 5),
]
EXT6_MAGIC = 0x4653455854414236  # FS_EXT6_MAGIC

# members of fs_ext7_api, the eighth table (append-only, behind the seven frozen ones), in declaration order after `magic` and `size`
_EXT7_HOOKS = [
    ("mask_distance", c_int, [c_void] + [c_int] * 3 + [ctypes.c_uint32, c_int] + [c_void] * 4),
    ("region_proximity", c_int, [c_void] * 5 + [c_int] * 5 + [ctypes.c_uint32, c_void, c_int] + [c_void] * 3),
]
EXT7_MAGIC = 0x4653455854414237  # FS_EXT7_MAGIC

# members of fs_ext8_api, the ninth table (append-only, behind the eight frozen ones), in declaration order after `magic` and `size`
_EXT8_HOOKS = [
    ("global_motion", c_int, [c_void] * 3 + [ctypes.c_uint32] + [c_int] * 6 + [ctypes.c_int64, c_int, c_void, c_void]),
    ("pose_chain", c_int, [c_void] * 3 + [c_int] * 8 + [c_void]),
    ("mosaic_accumulate", c_int, [c_void] * 2 + [c_int] * 8 + [c_void] * 2),
    ("mosaic_resolve", c_int, [c_void] + [c_int] * 3 + [c_void] * 5),
]
EXT8_MAGIC = 0x4653455854414238  # FS_EXT8_MAGIC

# members of fs_ext9_api, the tenth table (append-only, behind the nine frozen ones), in declaration order after `magic` and `size`
_EXT9_HOOKS = [
    ("ortho_accumulate", c_int, [c_void] * 3 + [c_int] * 5 + [c_void, ctypes.c_uint32] + [c_int] * 7 + [c_void] * 3),
    ("ortho_compose", c_int, [c_void] * 3 + [c_int, ctypes.c_uint32, ctypes.c_uint32, c_int, c_int, c_void, c_void]),
]
EXT9_MAGIC = 0x4653455854414239  # FS_EXT9_MAGIC

# members of fs_ext10_api, the eleventh table (append-only, behind the ten frozen ones), in declaration order after `magic` and `size`
_EXT10_HOOKS = [
    ("map_view", c_int, [c_void] * 3 + [c_int] * 5 + [c_void, ctypes.c_uint32] + [c_int] * 6 + [c_void] * 2 + [c_int] + [c_void] * 4),
    ("map_gate", c_int, [c_void, c_int, c_void, c_int, c_int, c_void]),
    ("pose_correct", c_int, [c_void] * 3 + [c_int] * 6 + [c_void] * 2),
]
EXT10_MAGIC = 0x4653455854413130  # FS_EXT10_MAGIC

# members of fs_ext11_api, the twelfth table (append-only, behind the eleven frozen ones), in declaration order after `magic` and `size`
_EXT11_HOOKS = [
    ("guide_vectors", c_int, [c_void] * 2 + [c_int] * 4 + [ctypes.c_int64] + [c_void] * 2 + [c_int, c_void, c_int, c_int] + [c_void] * 3),
]
EXT11_MAGIC = 0x4653455854413131  # FS_EXT11_MAGIC

# members of fs_ext12_api, the thirteenth table (append-only, behind the twelve frozen ones), in declaration order after `magic` and `size`
_EXT12_HOOKS = [
    ("map_coarse", c_int, [c_void] + [c_int] * 3 + [c_void] * 3),
    ("map_patch", c_int, [c_void] * 3 + [c_int] * 5 + [c_void] + [c_int] * 7 + [c_void] * 4),
    ("map_locate", c_int, [c_void] * 2 + [c_int] * 2 + [c_void] * 3 + [c_int] * 2 + [c_void] * 3),
    ("pose_relocate", c_int, [c_void] * 4 + [c_int] * 9 + [c_void]),
    ("relocate_commit", c_int, [c_void] * 6 + [c_int] + [c_void] * 2),
]
EXT12_MAGIC = 0x4653455854413132  # FS_EXT12_MAGIC

# members of fs_ext13_api, the fourteenth table (append-only, behind the thirteen frozen ones), in declaration order after `magic` and `size`
_EXT13_HOOKS = [
    ("merge_view", c_int, [c_void] + [c_int] * 4 + [c_void] + [c_int] * 4 + [c_void] + [c_int] * 4 + [c_void] * 5),
    ("merge_gate", c_int, [c_void] + [c_int] + [c_void] * 2 + [c_int] * 2 + [c_void]),
    ("link_correct", c_int, [c_void] * 2 + [c_int] * 6 + [c_void] * 2),
    ("mosaic_merge", c_int, [c_void] + [c_int] * 4 + [c_void] + [c_int] * 5 + [c_void] * 5 + [ctypes.c_uint32] + [c_int] + [c_void] * 2),
    ("merge_patch", c_int, [c_void] + [c_int] * 4 + [c_void] + [c_int] * 9 + [c_void] * 4),
    ("link_place", c_int, [c_void] * 2 + [c_int] * 3 + [c_void] * 3),
]
EXT13_MAGIC = 0x4653455854413133  # FS_EXT13_MAGIC

# members of fs_ext14_api, the fifteenth table (append-only, behind the fourteen frozen ones), in declaration order after `magic` and `size`
_EXT14_HOOKS = [
    ("mosaic_change", c_int, [c_void] + [c_int] * 4 + [c_void] + [c_int] * 5 + [c_void] + [c_int] * 3 + [ctypes.c_uint32] + [c_void] * 6),
]
EXT14_MAGIC = 0x4653455854413134  # FS_EXT14_MAGIC

# members of fs_ext15_api, the sixteenth table (append-only, behind the fifteen frozen ones), in declaration order after `magic` and `size`
_EXT15_HOOKS = [
    ("mask_access", c_int, [c_void] * 2 + [c_int] * 3 + [c_void] + [ctypes.c_uint32] + [c_int] + [ctypes.c_uint32] + [c_int] * 2 + [c_void] * 5),
    ("region_access", c_int, [c_void] * 5 + [c_int] * 5 + [c_void] * 3),
]
EXT15_MAGIC = 0x4653455854413135  # FS_EXT15_MAGIC

# members of fs_ext16_api, the seventeenth table (append-only, behind the sixteen frozen ones), in declaration order after `magic` and `size`
_EXT16_HOOKS = [
    ("ground_area", c_int, [c_void] + [c_int] * 4 + [c_void] + [c_int] + [c_void] + [c_int] + [c_void] * 4),
    ("ground_rectify", c_int, [c_void] + [c_int] * 7 + [ctypes.c_int64] * 2 + [c_int] + [c_void] * 4 + [c_int] + [ctypes.c_uint32] + [c_void]),
    ("ground_points", c_int, [c_void] + [c_int] + [c_void] + [c_int] * 2 + [c_void] * 2),
]
EXT16_MAGIC = 0x4653455854413136  # FS_EXT16_MAGIC


def _struct(name, *fields):
    return type(name, (ctypes.Structure,), {"_fields_": list(fields)})


def _members(hooks):
    return [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in hooks]


# the tables and the nested structs the library lays them out in (include/floodseg_test.h): every fs_hook_tablesN is the one before it
# with one more table directly behind
_EXT_HEAD = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)]
FsTestApi = _struct("FsTestApi", ("size", ctypes.c_size_t), *_members(_HOOKS))
FsExtApi = _struct("FsExtApi", *_EXT_HEAD, *_members(_EXT_HOOKS))
FsHookTables = _struct("FsHookTables", ("test", FsTestApi), ("ext", FsExtApi))
FsExt2Api = _struct("FsExt2Api", *_EXT_HEAD, *_members(_EXT2_HOOKS))
FsHookTables2 = _struct("FsHookTables2", ("base", FsHookTables), ("ext2", FsExt2Api))
FsExt3Api = _struct("FsExt3Api", *_EXT_HEAD, *_members(_EXT3_HOOKS))
FsHookTables3 = _struct("FsHookTables3", ("base2", FsHookTables2), ("ext3", FsExt3Api))
FsExt4Api = _struct("FsExt4Api", *_EXT_HEAD, *_members(_EXT4_HOOKS))
FsHookTables4 = _struct("FsHookTables4", ("base3", FsHookTables3), ("ext4", FsExt4Api))
FsExt5Api = _struct("FsExt5Api", *_EXT_HEAD, *_members(_EXT5_HOOKS))
FsHookTables5 = _struct("FsHookTables5", ("base4", FsHookTables4), ("ext5", FsExt5Api))
FsExt6Api = _struct("FsExt6Api", *_EXT_HEAD, *_members(_EXT6_HOOKS))
FsHookTables6 = _struct("FsHookTables6", ("base5", FsHookTables5), ("ext6", FsExt6Api))
FsExt7Api = _struct("FsExt7Api", *_EXT_HEAD, *_members(_EXT7_HOOKS))
FsHookTables7 = _struct("FsHookTables7", ("base6", FsHookTables6), ("ext7", FsExt7Api))
FsExt8Api = _struct("FsExt8Api", *_EXT_HEAD, *_members(_EXT8_HOOKS))
FsHookTables8 = _struct("FsHookTables8", ("base7", FsHookTables7), ("ext8", FsExt8Api))
FsExt9Api = _struct("FsExt9Api", *_EXT_HEAD, *_members(_EXT9_HOOKS))
FsHookTables9 = _struct("FsHookTables9", ("base8", FsHookTables8), ("ext9", FsExt9Api))
FsExt10Api = _struct("FsExt10Api", *_EXT_HEAD, *_members(_EXT10_HOOKS))
FsHookTables10 = _struct("FsHookTables10", ("base9", FsHookTables9), ("ext10", FsExt10Api))
FsExt11Api = _struct("FsExt11Api", *_EXT_HEAD, *_members(_EXT11_HOOKS))
FsHookTables11 = _struct("FsHookTables11", ("base10", FsHookTables10), ("ext11", FsExt11Api))
FsExt12Api = _struct("FsExt12Api", *_EXT_HEAD, *_members(_EXT12_HOOKS))
FsHookTables12 = _struct("FsHookTables12", ("base11", FsHookTables11), ("ext12", FsExt12Api))
FsExt13Api = _struct("FsExt13Api", *_EXT_HEAD, *_members(_EXT13_HOOKS))
FsHookTables13 = _struct("FsHookTables13", ("base12", FsHookTables12), ("ext13", FsExt13Api))
FsExt14Api = _struct("FsExt14Api", *_EXT_HEAD, *_members(_EXT14_HOOKS))
FsHookTables14 = _struct("FsHookTables14", ("base13", FsHookTables13), ("ext14", FsExt14Api))
FsExt15Api = _struct("FsExt15Api", *_EXT_HEAD, *_members(_EXT15_HOOKS))
FsHookTables15 = _struct("FsHookTables15", ("base14", FsHookTables14), ("ext15", FsExt15Api))
FsExt16Api = _struct("FsExt16Api", *_EXT_HEAD, *_members(_EXT16_HOOKS))
FsHookTables16 = _struct("FsHookTables16", ("base15", FsHookTables15), ("ext16", FsExt16Api))

# One row per hook table, in the library's order.  count / nth: the words the error messages use for the tables in front of it and for
# the table itself; magic: the NAME of its module global, read when a lookup happens; api: the table's struct; outer: the struct that
# ends with it, member: its name in there.
# Adding a table: its _EXTn_HOOKS, EXTn_MAGIC, FsExtnApi and FsHookTablesn above, one row here, and extn_hook_names below.
_Table = collections.namedtuple("_Table", "count nth hooks magic api outer member")
_TABLES = [
    _Table(None, None, _HOOKS, None, FsTestApi, FsHookTables, "test"),
    _Table("one", "first", _EXT_HOOKS, "EXT_MAGIC", FsExtApi, FsHookTables, "ext"),
    _Table("two", "second", _EXT2_HOOKS, "EXT2_MAGIC", FsExt2Api, FsHookTables2, "ext2"),
    _Table("three", "third", _EXT3_HOOKS, "EXT3_MAGIC", FsExt3Api, FsHookTables3, "ext3"),
    _Table("four", "fourth", _EXT4_HOOKS, "EXT4_MAGIC", FsExt4Api, FsHookTables4, "ext4"),
    _Table("five", "fifth", _EXT5_HOOKS, "EXT5_MAGIC", FsExt5Api, FsHookTables5, "ext5"),
    _Table("six", "sixth", _EXT6_HOOKS, "EXT6_MAGIC", FsExt6Api, FsHookTables6, "ext6"),
    _Table("seven", "seventh", _EXT7_HOOKS, "EXT7_MAGIC", FsExt7Api, FsHookTables7, "ext7"),
    _Table("eight", "eighth", _EXT8_HOOKS, "EXT8_MAGIC", FsExt8Api, FsHookTables8, "ext8"),
    _Table("nine", "ninth", _EXT9_HOOKS, "EXT9_MAGIC", FsExt9Api, FsHookTables9, "ext9"),
    _Table("ten", "tenth", _EXT10_HOOKS, "EXT10_MAGIC", FsExt10Api, FsHookTables10, "ext10"),
    _Table("eleven", "eleventh", _EXT11_HOOKS, "EXT11_MAGIC", FsExt11Api, FsHookTables11, "ext11"),
    _Table("twelve", "twelfth", _EXT12_HOOKS, "EXT12_MAGIC", FsExt12Api, FsHookTables12, "ext12"),
    _Table("thirteen", "thirteenth", _EXT13_HOOKS, "EXT13_MAGIC", FsExt13Api, FsHookTables13, "ext13"),
    _Table("fourteen", "fourteenth", _EXT14_HOOKS, "EXT14_MAGIC", FsExt14Api, FsHookTables14, "ext14"),
    _Table("fifteen", "fifteenth", _EXT15_HOOKS, "EXT15_MAGIC", FsExt15Api, FsHookTables15, "ext15"),
    _Table("sixteen", "sixteenth", _EXT16_HOOKS, "EXT16_MAGIC", FsExt16Api, FsHookTables16, "ext16"),
]
_TABLE_OF = {"fs_" + h[0]: n for n, t in enumerate(_TABLES) for h in t.hooks}


class _Library:
    """The loaded library: exported functions as attributes (ctypes), and the op-level test hooks of fs_test_hooks() under the names
    fs_<member> (so `lib.fs_conv2d_nhwc(...)` works whether a symbol is exported or lives in a table)."""

    def __init__(self, cdll):
        self._cdll = cdll
        self._tables = {}  # table number -> that table in the library, once its checks have passed

    def __getattr__(self, name):
        n = _TABLE_OF.get(name)
        if n is None:
            return getattr(self._cdll, name)  # an exported symbol, fs_test_hooks itself among them
        want = _TABLES[n]
        if n not in self._tables:
            # Every table in front of table n must be the one this binding knows, to the byte, or table n is not where `outer` puts it; table
            # n itself needs its magic and may be longer, since it grows at its end.  The two oldest tables accept any size from their own
            # on and keep their own messages.
            for t in _TABLES[:n + 1]:
                table = getattr(ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(t.outer)).contents, t.member)
                known = t.magic is None or table.magic == globals()[t.magic]
                if t is not want:
                    known = known and table.size == ctypes.sizeof(t.api)
                elif n < 2:
                    known = known and table.size >= ctypes.sizeof(t.api)
                if known:
                    continue
                if n == 0:
                    raise RuntimeError(f"floodseg: the library's test-hook table ({table.size} B) is older than this binding ({ctypes.sizeof(t.api)} B)")
                if n == 1:
                    raise RuntimeError(f"floodseg: the library has no extension table, or an older one than this binding ({name} is missing)")
                if t is not want:
                    raise RuntimeError(f"floodseg: the library's first {want.count} hook tables are not the ones this binding knows ({name} is missing)")
                raise RuntimeError(f"floodseg: the library has no {want.nth} extension table ({name} is missing)")
            self._tables[n] = table
        member = getattr(want.api, name[3:])  # an older library holds the members up to its table's `size`
        if n >= 2 and self._tables[n].size < member.offset + member.size:
            raise RuntimeError(f"floodseg: the library's {want.nth} extension table is older than this binding ({name} is missing)")
        fn = getattr(self._tables[n], name[3:])
        setattr(self, name, fn)
        return fn


_lib = None
ALLOW_MISSING = False  # development A/B against an OLDER build only (bench.py --lib): symbols it lacks are skipped, not an error


def load():
    """Load libfloodseg.so once; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback for this path")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        if ALLOW_MISSING and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = _Library(lib)
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


def _hook_names(n):
    """Members of table n after `size` (an extension table: after `magic` and `size`), in declaration order."""
    return [h[0] for h in _TABLES[n].hooks]


(hook_names, ext_hook_names, ext2_hook_names, ext3_hook_names, ext4_hook_names, ext5_hook_names, ext6_hook_names, ext7_hook_names,
 ext8_hook_names, ext9_hook_names, ext10_hook_names, ext11_hook_names, ext12_hook_names, ext13_hook_names,
 ext14_hook_names, ext15_hook_names, ext16_hook_names) = (functools.partial(_hook_names, n) for n in range(len(_TABLES)))


def check(rc):
    if rc != 0:
        msg = load().fs_last_error()
        raise RuntimeError("floodseg: " + (msg.decode() if msg else f"error {rc}"))


def stream_ptr(device=None):
    """Current HIP stream of `device` (default: the current device) as the void* the C ABI takes."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def one_device(*tensors, handle_device=None, what="floodseg"):
    """All tensors (None entries skipped) must live on ONE HIP device -- and on the handle's, when given.  Returns it.
    The library launches on the calling thread's current device, so every wrapper runs its call under
    `with torch.cuda.device(dev)`: a cuda:1 tensor while cuda:0 is current must never reach a device-0 launch."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{what}: tensors must live on the GPU (no CPU fallback exists)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"{what}: tensors on different devices ({dev} and {t.device})")
    if dev is None:
        raise RuntimeError(f"{what}: no device tensor given")
    if handle_device is not None and dev != handle_device:
        raise RuntimeError(f"{what}: tensor on {dev} but the network's weights live on {handle_device}")
    return dev


def ptr(t):
    """Device (or host) pointer of a tensor; None -> NULL."""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())
