"""Holding one key frame across a scene cut, the parts that need no GPU: the definition of the window weights (tests/cut_ref.py against
hand-written cases), the three new members of the third hook table, and the refusals of the Python surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cut_ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import motion
from flood_uav_video_segmentation_amd.flow.dataset import PredictWindows, RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["window_weights", "seg_tail_weighted", "crops_fuse_weighted"]


def f32(x):
    return np.float32(x)


def test_window_weights_definition_by_hand():
    # no cut, n = 5: the linear blend, each weight the float of the double quotient
    w, s = cut_ref.window_weights([0, None, 0, 0, 0], 5)
    assert w.dtype == np.float32 and s.dtype == np.int32
    assert w.tolist() == [[1.0, 0.0], [f32(0.8), f32(0.2)], [f32(0.6), f32(0.4)], [f32(0.4), f32(0.6)], [f32(0.2), f32(0.8)]]
    assert w[1, 0] == f32(4.0 / 5.0) and w[3, 1] == f32(3.0 / 5.0) and s.tolist() == [0] * 5
    # a cut at pair 1: only the key frame itself is on the previous key frame's side
    w, s = cut_ref.window_weights([1, 0, 0, 0, 0], 5)
    assert w.tolist() == [[1, 0], [0, 1], [0, 1], [0, 1], [0, 1]] and s.tolist() == [1, 2, 2, 2, 2]
    # a cut at pair n (the closing pair): every emitted frame is held from the previous key frame
    w, s = cut_ref.window_weights([0, 0, 0, 0, 1], 5)
    assert w.tolist() == [[1, 0]] * 5 and s.tolist() == [1] * 5
    # a cut inside
    w, s = cut_ref.window_weights([0, 0, 1, 0, 0], 5)
    assert w.tolist() == [[1, 0], [1, 0], [1, 0], [0, 1], [0, 1]] and s.tolist() == [1, 1, 1, 2, 2]
    # two cuts, pairs 2 and 4 of 5: frames 2 and 3 show a scene neither key frame has; 2 f <= n goes to the previous key frame
    w, s = cut_ref.window_weights([0, 1, 0, 1, 0], 5)
    assert w.tolist() == [[1, 0], [1, 0], [1, 0], [0, 1], [0, 1]] and s.tolist() == [1, 1, 3, 3, 2]
    w, s = cut_ref.window_weights([1, 0, 0, 1], 4)      # 2 f == n is still the previous key frame's
    assert w.tolist() == [[1, 0], [1, 0], [1, 0], [0, 1]] and s.tolist() == [1, 3, 3, 3]
    # n = 1: the window emits the key frame only
    assert [x.tolist() for x in cut_ref.window_weights([0], 1)] == [[[1, 0]], [0]]
    assert [x.tolist() for x in cut_ref.window_weights([1], 1)] == [[[1, 0]], [1]]
    assert [x.tolist() for x in cut_ref.window_weights([None], 1)] == [[[1, 0]], [0]]


def test_new_members_follow_block_match_modes_in_header_initialiser_and_binding():
    ext2 = _lib.ext2_hook_names()
    assert ext2[0] == "block_match_modes" and ext2[1:4] == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext2_api {"):text.index("} fs_ext2_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == ext2
    for i, name in enumerate(NEW, start=1):
        assert getattr(_lib.FsExt2Api, name).offset == 16 + 8 * i
    assert len(_lib.exported_symbols()) == 40 and not any("fs_" + n in _lib.exported_symbols() for n in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    all3 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables2)).contents
    assert all3.ext2.size >= 16 + 8 * 4
    for name in NEW:
        assert ctypes.cast(getattr(all3.ext2, name), ctypes.c_void_p).value and getattr(lib, "fs_" + name) is not None


def test_window_weights_arguments_are_refused_before_a_launch():
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    arr = (ctypes.c_void_p * 64)()
    for n, weights, source, word in ((0, fake, fake, b"1..64"), (65, fake, fake, b"1..64"), (-3, fake, fake, b"1..64"),
                                     (5, None, fake, b"null"), (5, fake, None, b"null")):
        assert lib.fs_window_weights(n, arr, weights, source, None) != 0
        assert word in lib.fs_last_error() and b"fs_window_weights" in lib.fs_last_error(), lib.fs_last_error()
    with pytest.raises(RuntimeError, match="1..64"):
        ops.window_weights([None] * 65, 65)
    with pytest.raises(RuntimeError, match="per frame pair"):
        ops.window_weights([None] * 4, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.window_weights([torch.zeros(4, dtype=torch.int32)], 1)


def test_hold_cuts_without_scene_cut_raises(tmp_path):
    with pytest.raises(ValueError, match="hold_cuts"):
        PredictWindows(str(tmp_path), "v", grids="estimate", intra_bias=0, hold_cuts=True)
    with pytest.raises(ValueError, match="hold_cuts"):
        PredictWindows(str(tmp_path), "v", grids="files", scene_cut=0.5, hold_cuts=True)
    with pytest.raises(ValueError, match="hold_cuts"):
        RawVideoWindows(str(tmp_path / "none.rgb"), 1072, 1920, "rgb24", grids="estimate", intra_bias=0, hold_cuts=True)
    with pytest.raises(ValueError, match="hold_cuts"):
        RawVideoWindows(str(tmp_path / "none.rgb"), 1072, 1920, "rgb24", no_warp=True, hold_cuts=True)
    assert PredictWindows.hold_cuts is False


def test_window_stats_without_decisions_or_frames_is_all_none():
    est = motion.GridEstimator()
    assert est.window_stats(5, 5, lambda i: pytest.fail("no frame is needed when both decisions are off")) == [None] * 5
    est = motion.GridEstimator(intra_bias=0, scene_cut=0.5)
    assert est.window_stats(0, 3, lambda i: None) == [None] * 3     # no frame exists: every pair is "no cut"


def test_predict_feature_refuses_weights():
    fm = FlowModel(torch.nn.Identity(), feature_based=True, no_warp=True)
    x = torch.zeros(1, 3, 9, 9)
    with pytest.raises(NotImplementedError, match="segmentation tails"):
        fm.predict_feature(x, x, [], [], 1, weights=torch.zeros(1, 2))
    with pytest.raises(NotImplementedError, match="segmentation tails"):
        fm.predict(x, x, [], [], 1, weights=torch.zeros(1, 2))
