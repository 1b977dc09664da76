"""ctypes binding of libfloodseg.so (the C ABI declared in include/floodseg.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, importing
the ops raises.  torch is imported first on purpose -- torch ships its own libamdhip64 (same
soname), and device pointers / streams are only interchangeable inside ONE HIP runtime instance.
"""
import ctypes
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


class FsTestApi(ctypes.Structure):
    _fields_ = [("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _HOOKS]


class FsExtApi(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT_HOOKS]


class FsHookTables(ctypes.Structure):
    _fields_ = [("test", FsTestApi), ("ext", FsExtApi)]


class FsExt2Api(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT2_HOOKS]


class FsHookTables2(ctypes.Structure):
    _fields_ = [("base", FsHookTables), ("ext2", FsExt2Api)]


class FsExt3Api(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT3_HOOKS]


class FsHookTables3(ctypes.Structure):
    _fields_ = [("base2", FsHookTables2), ("ext3", FsExt3Api)]


class FsExt4Api(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT4_HOOKS]


class FsHookTables4(ctypes.Structure):
    _fields_ = [("base3", FsHookTables3), ("ext4", FsExt4Api)]


class FsExt5Api(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT5_HOOKS]


class FsHookTables5(ctypes.Structure):
    _fields_ = [("base4", FsHookTables4), ("ext5", FsExt5Api)]


class FsExt6Api(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT6_HOOKS]


class FsHookTables6(ctypes.Structure):
    _fields_ = [("base5", FsHookTables5), ("ext6", FsExt6Api)]


class FsExt7Api(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT7_HOOKS]


class FsHookTables7(ctypes.Structure):
    _fields_ = [("base6", FsHookTables6), ("ext7", FsExt7Api)]


class FsExt8Api(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint64), ("size", ctypes.c_size_t)] + [(name, ctypes.CFUNCTYPE(res, *args)) for name, res, args in _EXT8_HOOKS]


class FsHookTables8(ctypes.Structure):
    _fields_ = [("base7", FsHookTables7), ("ext8", FsExt8Api)]


class _Library:
    """The loaded library: exported functions as attributes (ctypes), and the op-level test hooks of fs_test_hooks() under the names
    fs_<member> (so `lib.fs_conv2d_nhwc(...)` works whether a symbol is exported or lives in the table)."""

    def __init__(self, cdll):
        self._cdll = cdll
        self._hooks = None
        self._ext = None
        self._ext2 = None
        self._ext3 = None
        self._ext4 = None
        self._ext5 = None
        self._ext6 = None
        self._ext7 = None
        self._ext8 = None

    def __getattr__(self, name):
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT8_HOOKS):
            if self._ext8 is None:
                all7 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables7)).contents
                all5 = all7.base6.base5
                all2 = all5.base4.base3.base2
                if (all2.base.test.size != ctypes.sizeof(FsTestApi) or all2.base.ext.magic != EXT_MAGIC or all2.base.ext.size != ctypes.sizeof(FsExtApi)
                        or all2.ext2.magic != EXT2_MAGIC or all2.ext2.size != ctypes.sizeof(FsExt2Api)
                        or all5.base4.base3.ext3.magic != EXT3_MAGIC or all5.base4.base3.ext3.size != ctypes.sizeof(FsExt3Api)
                        or all5.base4.ext4.magic != EXT4_MAGIC or all5.base4.ext4.size != ctypes.sizeof(FsExt4Api)
                        or all5.ext5.magic != EXT5_MAGIC or all5.ext5.size != ctypes.sizeof(FsExt5Api)
                        or all7.base6.ext6.magic != EXT6_MAGIC or all7.base6.ext6.size != ctypes.sizeof(FsExt6Api)
                        or all7.ext7.magic != EXT7_MAGIC or all7.ext7.size != ctypes.sizeof(FsExt7Api)):
                    raise RuntimeError(f"floodseg: the library's first eight hook tables are not the ones this binding knows ({name} is missing)")
                ext8 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables8)).contents.ext8
                if ext8.magic != EXT8_MAGIC:
                    raise RuntimeError(f"floodseg: the library has no eighth extension table ({name} is missing)")
                self._ext8 = ext8
            member = getattr(FsExt8Api, name[3:])  # the table grows at its end: an older library holds the members up to its `size`
            if self._ext8.size < member.offset + member.size:
                raise RuntimeError(f"floodseg: the library's eighth extension table is older than this binding ({name} is missing)")
            fn = getattr(self._ext8, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT7_HOOKS):
            if self._ext7 is None:
                all6 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables6)).contents
                all5 = all6.base5
                all2 = all5.base4.base3.base2
                if (all2.base.test.size != ctypes.sizeof(FsTestApi) or all2.base.ext.magic != EXT_MAGIC or all2.base.ext.size != ctypes.sizeof(FsExtApi)
                        or all2.ext2.magic != EXT2_MAGIC or all2.ext2.size != ctypes.sizeof(FsExt2Api)
                        or all5.base4.base3.ext3.magic != EXT3_MAGIC or all5.base4.base3.ext3.size != ctypes.sizeof(FsExt3Api)
                        or all5.base4.ext4.magic != EXT4_MAGIC or all5.base4.ext4.size != ctypes.sizeof(FsExt4Api)
                        or all5.ext5.magic != EXT5_MAGIC or all5.ext5.size != ctypes.sizeof(FsExt5Api)
                        or all6.ext6.magic != EXT6_MAGIC or all6.ext6.size != ctypes.sizeof(FsExt6Api)):
                    raise RuntimeError(f"floodseg: the library's first seven hook tables are not the ones this binding knows ({name} is missing)")
                ext7 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables7)).contents.ext7
                if ext7.magic != EXT7_MAGIC:
                    raise RuntimeError(f"floodseg: the library has no seventh extension table ({name} is missing)")
                self._ext7 = ext7
            member = getattr(FsExt7Api, name[3:])  # the table grows at its end: an older library holds the members up to its `size`
            if self._ext7.size < member.offset + member.size:
                raise RuntimeError(f"floodseg: the library's seventh extension table is older than this binding ({name} is missing)")
            fn = getattr(self._ext7, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT6_HOOKS):
            if self._ext6 is None:
                all5 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables5)).contents
                all2 = all5.base4.base3.base2
                if (all2.base.test.size != ctypes.sizeof(FsTestApi) or all2.base.ext.magic != EXT_MAGIC or all2.base.ext.size != ctypes.sizeof(FsExtApi)
                        or all2.ext2.magic != EXT2_MAGIC or all2.ext2.size != ctypes.sizeof(FsExt2Api)
                        or all5.base4.base3.ext3.magic != EXT3_MAGIC or all5.base4.base3.ext3.size != ctypes.sizeof(FsExt3Api)
                        or all5.base4.ext4.magic != EXT4_MAGIC or all5.base4.ext4.size != ctypes.sizeof(FsExt4Api)
                        or all5.ext5.magic != EXT5_MAGIC or all5.ext5.size != ctypes.sizeof(FsExt5Api)):
                    raise RuntimeError(f"floodseg: the library's first six hook tables are not the ones this binding knows ({name} is missing)")
                ext6 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables6)).contents.ext6
                if ext6.magic != EXT6_MAGIC:
                    raise RuntimeError(f"floodseg: the library has no sixth extension table ({name} is missing)")
                self._ext6 = ext6
            member = getattr(FsExt6Api, name[3:])  # the table grows at its end: an older library holds the members up to its `size`
            if self._ext6.size < member.offset + member.size:
                raise RuntimeError(f"floodseg: the library's sixth extension table is older than this binding ({name} is missing)")
            fn = getattr(self._ext6, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT5_HOOKS):
            if self._ext5 is None:
                all4 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables4)).contents
                all2 = all4.base3.base2
                if (all2.base.test.size != ctypes.sizeof(FsTestApi) or all2.base.ext.magic != EXT_MAGIC or all2.base.ext.size != ctypes.sizeof(FsExtApi)
                        or all2.ext2.magic != EXT2_MAGIC or all2.ext2.size != ctypes.sizeof(FsExt2Api)
                        or all4.base3.ext3.magic != EXT3_MAGIC or all4.base3.ext3.size != ctypes.sizeof(FsExt3Api)
                        or all4.ext4.magic != EXT4_MAGIC or all4.ext4.size != ctypes.sizeof(FsExt4Api)):
                    raise RuntimeError(f"floodseg: the library's first five hook tables are not the ones this binding knows ({name} is missing)")
                ext5 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables5)).contents.ext5
                if ext5.magic != EXT5_MAGIC:
                    raise RuntimeError(f"floodseg: the library has no fifth extension table ({name} is missing)")
                self._ext5 = ext5
            member = getattr(FsExt5Api, name[3:])  # the table grows at its end: an older library holds the members up to its `size`
            if self._ext5.size < member.offset + member.size:
                raise RuntimeError(f"floodseg: the library's fifth extension table is older than this binding ({name} is missing)")
            fn = getattr(self._ext5, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT4_HOOKS):
            if self._ext4 is None:
                all3 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables3)).contents
                all2 = all3.base2
                if (all2.base.test.size != ctypes.sizeof(FsTestApi) or all2.base.ext.magic != EXT_MAGIC or all2.base.ext.size != ctypes.sizeof(FsExtApi)
                        or all2.ext2.magic != EXT2_MAGIC or all2.ext2.size != ctypes.sizeof(FsExt2Api)
                        or all3.ext3.magic != EXT3_MAGIC or all3.ext3.size != ctypes.sizeof(FsExt3Api)):
                    raise RuntimeError(f"floodseg: the library's first four hook tables are not the ones this binding knows ({name} is missing)")
                ext4 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables4)).contents.ext4
                if ext4.magic != EXT4_MAGIC:
                    raise RuntimeError(f"floodseg: the library has no fourth extension table ({name} is missing)")
                self._ext4 = ext4
            member = getattr(FsExt4Api, name[3:])  # the table grows at its end: an older library holds the members up to its `size`
            if self._ext4.size < member.offset + member.size:
                raise RuntimeError(f"floodseg: the library's fourth extension table is older than this binding ({name} is missing)")
            fn = getattr(self._ext4, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT3_HOOKS):
            if self._ext3 is None:
                all2 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables2)).contents
                if (all2.base.test.size != ctypes.sizeof(FsTestApi) or all2.base.ext.magic != EXT_MAGIC or all2.base.ext.size != ctypes.sizeof(FsExtApi)
                        or all2.ext2.magic != EXT2_MAGIC or all2.ext2.size != ctypes.sizeof(FsExt2Api)):
                    raise RuntimeError(f"floodseg: the library's first three hook tables are not the ones this binding knows ({name} is missing)")
                ext3 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables3)).contents.ext3
                if ext3.magic != EXT3_MAGIC:
                    raise RuntimeError(f"floodseg: the library has no third extension table ({name} is missing)")
                self._ext3 = ext3
            member = getattr(FsExt3Api, name[3:])  # the table grows at its end: an older library holds the members up to its `size`
            if self._ext3.size < member.offset + member.size:
                raise RuntimeError(f"floodseg: the library's third extension table is older than this binding ({name} is missing)")
            fn = getattr(self._ext3, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT2_HOOKS):
            if self._ext2 is None:
                base = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables)).contents
                if base.test.size != ctypes.sizeof(FsTestApi) or base.ext.magic != EXT_MAGIC or base.ext.size != ctypes.sizeof(FsExtApi):
                    raise RuntimeError(f"floodseg: the library's first two hook tables are not the ones this binding knows ({name} is missing)")
                ext2 = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables2)).contents.ext2
                if ext2.magic != EXT2_MAGIC:
                    raise RuntimeError(f"floodseg: the library has no second extension table ({name} is missing)")
                self._ext2 = ext2
            member = getattr(FsExt2Api, name[3:])  # the table grows at its end: an older library holds the members up to its `size`
            if self._ext2.size < member.offset + member.size:
                raise RuntimeError(f"floodseg: the library's second extension table is older than this binding ({name} is missing)")
            fn = getattr(self._ext2, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and any(name == "fs_" + h[0] for h in _EXT_HOOKS):
            if self._ext is None:
                tables = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsHookTables)).contents
                if tables.test.size != ctypes.sizeof(FsTestApi) or tables.ext.magic != EXT_MAGIC or tables.ext.size < ctypes.sizeof(FsExtApi):
                    raise RuntimeError(f"floodseg: the library has no extension table, or an older one than this binding ({name} is missing)")
                self._ext = tables.ext
            fn = getattr(self._ext, name[3:])
            setattr(self, name, fn)
            return fn
        if name.startswith("fs_") and name != "fs_test_hooks" and any(name == "fs_" + h[0] for h in _HOOKS):
            if self._hooks is None:
                table = ctypes.cast(self._cdll.fs_test_hooks(), ctypes.POINTER(FsTestApi)).contents
                if table.size < ctypes.sizeof(FsTestApi):
                    raise RuntimeError(f"floodseg: the library's test-hook table ({table.size} B) is older than this binding ({ctypes.sizeof(FsTestApi)} B)")
                self._hooks = table
            fn = getattr(self._hooks, name[3:])
            setattr(self, name, fn)
            return fn
        return getattr(self._cdll, name)


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


def hook_names():
    """Members of fs_test_api after `size`, in declaration order."""
    return [h[0] for h in _HOOKS]


def ext_hook_names():
    """Members of fs_ext_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT_HOOKS]


def ext2_hook_names():
    """Members of fs_ext2_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT2_HOOKS]


def ext3_hook_names():
    """Members of fs_ext3_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT3_HOOKS]


def ext4_hook_names():
    """Members of fs_ext4_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT4_HOOKS]


def ext5_hook_names():
    """Members of fs_ext5_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT5_HOOKS]


def ext6_hook_names():
    """Members of fs_ext6_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT6_HOOKS]


def ext7_hook_names():
    """Members of fs_ext7_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT7_HOOKS]


def ext8_hook_names():
    """Members of fs_ext8_api after `magic` and `size`, in declaration order."""
    return [h[0] for h in _EXT8_HOOKS]


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
