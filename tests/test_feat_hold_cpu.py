"""Holding a key frame across a scene cut in the FEATURE tail, the parts that need no GPU: the fifth member of the third hook table
(feat_tail_weighted), what fs_feat_tail / feat_tail_weighted refuse before any launch, and the refusals of the Python surface."""
import ctypes
import os
import re

import pytest
import torch

from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow.model import FlowModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "feat_tail_weighted"


def test_feat_tail_weighted_is_the_fifth_member_in_header_initialiser_and_binding():
    ext2 = _lib.ext2_hook_names()
    assert ext2[4] == NAME and ext2[:4] == ["block_match_modes", "window_weights", "seg_tail_weighted", "crops_fuse_weighted"]
    assert getattr(_lib.FsExt2Api, NAME).offset == 16 + 8 * 4 == 48
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext2_api {"):text.index("} fs_ext2_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body)[:5] == ext2[:5]
    src = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read()
    init = src[src.index("static const fs_hook_tables2 all"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M)[:5] == ["fs_" + n for n in ext2[:5]]
    # the weighted entry takes fs_feat_tail's arguments with the weights pointer before the stream
    plain = _lib._SIGNATURES["fs_feat_tail"][1]
    weighted = dict((n, a) for n, _, a in _lib._EXT2_HOOKS)[NAME]
    assert weighted == plain[:-1] + [_lib.c_void, plain[-1]]
    decl = re.sub(r"\s+", " ", body[body.index("(*" + NAME + ")"):]).split(";")[0]
    assert decl.endswith("float* stack, float* scratch, const float* weights, fs_stream stream)")


def test_table_size_exports_and_version():
    lib = _lib.load()
    all3 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables2)).contents
    assert all3.ext2.magic == _lib.EXT2_MAGIC and all3.ext2.size >= 16 + 8 * 5          # from below only: the table grows at its end
    assert ctypes.cast(getattr(all3.ext2, NAME), ctypes.c_void_p).value and lib.fs_feat_tail_weighted is not None
    assert len(_lib.exported_symbols()) == 40 and "fs_" + NAME not in _lib.exported_symbols()
    assert lib.fs_version() == 600
    with pytest.raises(AttributeError):
        getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + NAME)                                 # a table member, not an exported symbol


def grid_array(entries):
    arr = (ctypes.c_void_p * len(entries))()
    for i, e in enumerate(entries):
        arr[i] = e
    return arr


@pytest.mark.parametrize("weighted", [False, True])
def test_feat_tail_arguments_are_refused_before_a_launch(weighted):
    """Fake non-null pointers: a call that got as far as a launch would fail with another message (or fault on a GPU)."""
    lib = _lib.load()
    fake, odd = 0x1000, 0x1004
    ok2 = grid_array([fake, fake])

    def call(f_prev=fake, f_next=fake, C=64, fh=8, fw=8, gl=ok2, gr=ok2, n=3, no_warp=0, stack=fake, scratch=fake):
        args = [f_prev, f_next, C, fh, fw, gl, gr, 4, 4, fake, 3, 3, n, no_warp, stack, scratch]
        if weighted:
            return lib.fs_feat_tail_weighted(*args, fake, None)
        return lib.fs_feat_tail(*args, None)

    cases = [
        (dict(gl=grid_array([fake, None])), b"null pointer"),          # a NULL entry among the n-1 grids of either direction
        (dict(gr=grid_array([None, fake])), b"null pointer"),
        (dict(f_prev=odd), b"16-byte aligned"),
        (dict(f_next=odd, no_warp=1), b"16-byte aligned"),
        (dict(stack=odd), b"16-byte aligned"),
        (dict(scratch=odd), b"16-byte aligned"),
        (dict(C=6), b"C % 4 == 0"),
        (dict(C=2), b"C % 4 == 0"),
        (dict(n=0), b"n must be >= 1"),
        (dict(n=-2, no_warp=1), b"n must be >= 1"),
        (dict(C=256, fh=4096, fw=4096), b"2^32"),                      # fh * fw * C == 2^32: the key map's 32-bit tap offsets
        (dict(C=4, fh=32768, fw=32768), b"2^32"),
    ]
    for kw, word in cases:
        assert call(**kw) != 0, kw
        msg = lib.fs_last_error()
        assert word in msg and b"feat_tail" in msg, (kw, msg)


def test_ops_feat_tail_refuses_bad_weights():
    f = torch.zeros(1, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    for w in (torch.zeros(3, 2), torch.zeros(4, 2), torch.zeros(3, 2, dtype=torch.float64), torch.zeros(6)):
        with pytest.raises(RuntimeError):
            ops.feat_tail(f, f, [], [], 3, True, weights=w)
    # the check itself, as feat_tail calls it (the tensors of a real call live on a GPU)
    dev = torch.device("cuda", 0)
    for w, word in ((torch.zeros(3, 2), "device"), (torch.zeros(3, 2, dtype=torch.float64), "device")):
        with pytest.raises(RuntimeError, match=word):
            ops._window_weights_arg(w, 3, dev, "floodseg.feat_tail")
    assert ops._window_weights_arg(None, 3, dev, "floodseg.feat_tail") is None


class MirrorThatMustNotRun(torch.nn.Module):
    """Looks like a HIP mirror (offers encode_frames); fails the test if the encoder is reached."""

    def encode_frames(self, *frames):
        pytest.fail("the refusal must come before the encoder runs")

    encoder = decoder = encode_frames


def test_predict_feature_with_weights_is_refused_off_the_fused_route():
    x, w = torch.zeros(1, 3, 9, 9), torch.zeros(1, 2)
    fm = FlowModel(torch.nn.Identity(), feature_based=True, no_warp=True)               # a foreign network: no encode_frames
    assert fm.fused_feature_tail is True
    with pytest.raises(NotImplementedError, match="segmentation tails"):
        fm.predict_feature(x, x, [], [], 1, weights=w)
    fm = FlowModel(MirrorThatMustNotRun(), feature_based=True, no_warp=True)
    fm.fused_feature_tail = False                                                        # the op-by-op route has no weighted form
    for call in (fm.predict_feature, fm.predict):
        with pytest.raises(NotImplementedError, match="segmentation tails.*fused feature tail"):
            call(x, x, [], [], 1, weights=w)
