"""Intra blocks and scene cuts of the block-motion estimator without a GPU: the third hook table the op enters by, its argument
refusals, and self-checks of the numpy restatement (tests/motion_modes_ref.py) on the synthetic scenes the GPU tests use -- so that
"GPU == restatement" there is not an equality of two tables without a single void row."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import motion_modes_ref as modes_ref
import motion_ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import motion
from flood_uav_video_segmentation_amd.flow.model import get_default_grid
from oracle.crops_oracle import motion_vectors_to_grids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ library surface
def test_block_match_modes_is_the_first_member_of_the_third_table():
    """The same name in the same position in the header, in the library's initialiser and in the binding; the member's POSITION is
    pinned (first, offset 16) and the table's size only from below, so the next extension op is appended without editing this."""
    ext2 = _lib.ext2_hook_names()
    index = ext2.index("block_match_modes")
    assert index == 0
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext2_api {"):text.index("} fs_ext2_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == ext2
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables;") < text.index("typedef struct fs_ext2_api {") < text.index("typedef struct fs_hook_tables2 {")
    tables2 = text[text.index("typedef struct fs_hook_tables2 {"):text.index("} fs_hook_tables2;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables2) == [("fs_hook_tables", "base"), ("fs_ext2_api", "ext2")]
    assert int(re.search(r"#define FS_EXT2_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT2_MAGIC == int.from_bytes(b"FSEXTAB2", "big")
    src = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read()
    init = src[src.index("static const fs_hook_tables2 all = {tables, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + n for n in ext2]
    assert "FS_EXT2_MAGIC," in init and "sizeof(fs_ext2_api)," in init
    # the two older tables and the export list are what they were
    assert _lib.hook_names()[-1] == "block_match" and len(_lib.hook_names()) == 38
    assert _lib.ext_hook_names() == ["frame_prepare", "frame_compose"]
    assert len(_lib.exported_symbols()) == 40 and "fs_block_match_modes" not in _lib.exported_symbols()
    assert "block_match_modes" not in open(os.path.join(ROOT, "include", "floodseg.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    lib = _lib.load()
    assert lib.fs_version() == 600
    all3 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables2)).contents
    assert all3.base.test.size == ctypes.sizeof(_lib.FsTestApi) == ctypes.sizeof(ctypes.c_size_t) + 38 * ctypes.sizeof(ctypes.c_void_p)
    assert all3.base.ext.magic == _lib.EXT_MAGIC and all3.base.ext.size == ctypes.sizeof(_lib.FsExtApi) == 32
    assert _lib.FsHookTables2.ext2.offset == ctypes.sizeof(_lib.FsHookTables)           # directly behind, no padding
    assert all3.ext2.magic == _lib.EXT2_MAGIC                                           # checked before the table is used
    assert _lib.FsExt2Api.block_match_modes.offset == 16 + 8 * index == 16
    assert all3.ext2.size >= 16 + 8 * (index + 1) and all3.ext2.size >= ctypes.sizeof(_lib.FsExt2Api)
    assert ctypes.cast(all3.ext2.block_match_modes, ctypes.c_void_p).value
    # the first two tables of the object are the frozen ones, member for member
    two = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables)).contents
    for name in _lib.hook_names():
        assert ctypes.cast(getattr(two.test, name), ctypes.c_void_p).value == ctypes.cast(getattr(all3.base.test, name), ctypes.c_void_p).value
    assert lib.fs_block_match_modes is not None and lib.fs_block_match is not None and lib.fs_frame_prepare is not None


def test_header_with_the_third_table_is_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "floodseg_test.h"\n'
                   "int main(void) { const fs_hook_tables2* t = (const fs_hook_tables2*)fs_test_hooks();\n"
                   "  return t->ext2.magic == FS_EXT2_MAGIC && (const void*)&t->base.test == (const void*)t ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_errors_are_refused_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    good = dict(cur=fake, ref=fake, H=64, W=64, channels=1, search=16, penalty=0, intra_bias=0, cut_permille=500, mv=fake)
    cases = [(dict(cur=None), b"null"), (dict(ref=None), b"null"), (dict(mv=None), b"null"),
             (dict(channels=4), b"channels"), (dict(channels=0), b"channels"), (dict(H=15), b"smaller"), (dict(W=15), b"smaller"),
             (dict(search=0), b"search"), (dict(search=33), b"search"), (dict(penalty=-1), b"penalty"), (dict(penalty=256), b"penalty"),
             (dict(H=1 << 15, W=1 << 15, channels=3), b"too large"),
             (dict(intra_bias=-1), b"intra_bias"), (dict(intra_bias=65536), b"intra_bias"),
             (dict(cut_permille=-1), b"cut_permille"), (dict(cut_permille=1001), b"cut_permille")]
    for change, word in cases:
        a = dict(good, **change)
        rc = lib.fs_block_match_modes(a["cur"], a["ref"], a["H"], a["W"], a["channels"], a["search"], a["penalty"], a["intra_bias"],
                                      a["cut_permille"], a["mv"], None, None, None, None)
        assert rc != 0 and word in lib.fs_last_error() and b"fs_block_match_modes" in lib.fs_last_error(), (change, lib.fs_last_error())


def test_python_surface_refuses_bad_arguments_without_a_gpu():
    a = torch.zeros(64, 64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.block_match_modes(a, a.clone(), intra_bias=0)
    with pytest.raises(ValueError, match="intra_bias"):
        motion.GridEstimator(intra_bias=65536)
    with pytest.raises(ValueError, match="scene_cut"):
        motion.GridEstimator(scene_cut=1.5)
    with pytest.warns(UserWarning, match="never detects a cut"):      # the cut rule counts intra blocks: alone it cannot fire
        motion.GridEstimator(scene_cut=0.5)
    est = motion.GridEstimator(intra_bias=0, scene_cut=0.5)
    assert est.intra_bias == 0 and est.scene_cut == 0.5 and est.stats_for(3) is None
    off = motion.GridEstimator()
    assert off.intra_bias is None and off.scene_cut is None
    assert ops.VOID_ROW == modes_ref.VOID_ROW and [modes_ref.permille(x) for x in (None, 0.0, 0.5, 1.0, 0.0004, 0.0006)] == [1000, 0, 500, 1000, 0, 1]


# ------------------------------------------------------------------------------------------------ the restatement on hand-checked blocks
def test_activity_of_hand_checked_blocks():
    flat = np.full((16, 16), 200, dtype=np.uint8)
    assert modes_ref.block_activity(flat).tolist() == [0]
    half = flat.copy()
    half[:, 8:] = 0                      # S = 128 * 200 = 25600, m = (25600 + 128) >> 8 = 100: every pixel is 100 away
    assert modes_ref.block_activity(half).tolist() == [25600]
    board = ((np.indices((16, 16)).sum(axis=0) % 2) * 255).astype(np.uint8)   # S = 32640, m = (32640 + 128) >> 8 = 128: 128 * 128 + 128 * 127
    assert modes_ref.block_activity(board).tolist() == [32640]
    one = np.zeros((16, 16), dtype=np.uint8)
    one[0, 0] = 255                      # S = 255, m = 383 >> 8 = 1: 254 + 255 * 1
    assert modes_ref.block_activity(one).tolist() == [509]
    rgb = np.stack([half, half, half], axis=-1)                               # luma of (200, 200, 200) = (51200 + 128) >> 8 = 200
    assert modes_ref.block_activity(rgb).tolist() == [25600]
    # a remainder strip owns no block
    assert modes_ref.block_activity(np.zeros((40, 50), dtype=np.uint8)).shape == (6,)


def test_the_rule_on_saturated_and_flat_frames():
    """0 against 255: sad = 65280 and activity = 0, so every block is intra up to bias 65279 and none from 65280 on; the penalty is
    taken out of the cost before the comparison."""
    zero, full = np.zeros((48, 64), dtype=np.uint8), np.full((48, 64), 255, dtype=np.uint8)
    for penalty in (0, 255):
        for bias, n in ((0, 12), (65279, 12), (65280, 0), (65535, 0)):
            table, cost, act, stats = modes_ref.block_match_modes(zero, full, 16, penalty, bias, 1000)
            assert stats.tolist() == [12, n, 0, 0] and (cost == 65280).all() and not act.any()
            assert modes_ref.is_void(table).sum() == n
    table, cost, act, stats = modes_ref.block_match_modes(zero, zero.copy(), 16, 4, 0, 0)
    assert stats.tolist() == [12, 0, 0, 0] and not modes_ref.is_void(table).any()        # 0 > 0 is false: permille 0 cuts on ONE intra block
    table, _, _, stats = modes_ref.block_match_modes(zero, full, 16, 0, 0, 999)
    assert stats.tolist() == [12, 12, 1, 0] and modes_ref.is_void(table).all()
    table, _, _, stats = modes_ref.block_match_modes(zero, full, 16, 0, 0, 1000)
    assert stats.tolist() == [12, 12, 0, 0]                                               # 1000 can never cut


# ------------------------------------------------------------------------------------------------ the scenes of the GPU tests
H, W = 104, 168   # 6 x 10 blocks and a remainder strip of 8 on both axes: at (5, 3) every block's true match is a candidate


@pytest.mark.parametrize("channels", [1, 3])
def test_a_translated_textured_frame_has_no_intra_block_at_bias_0(channels):
    cur, ref = modes_ref.translated_pair(H, W, 5, 3, seed=11, channels=channels)
    table, cost, act, stats = modes_ref.block_match_modes(cur, ref, 8, 0, 0, 500)
    want, want_cost = motion_ref.block_match(cur, ref, 8, 0)
    assert stats.tolist() == [60, 0, 0, 0] and np.array_equal(table, want) and np.array_equal(cost, want_cost)
    dx, dy = motion_ref.vectors(table)
    assert (dx == 5).all() and (dy == 3).all() and not cost.any() and act.min() > 1000


@pytest.mark.parametrize("channels", [1, 3])
def test_an_occluded_rectangle_is_intra_and_the_rest_inter_without_a_cut(channels):
    cur, ref = modes_ref.occluded_pair(H, W, 5, 3, seed=12, channels=channels, rect=(32, 48, 64, 96))
    table, cost, act, stats = modes_ref.block_match_modes(cur, ref, 8, 0, 0, 500)
    void = modes_ref.is_void(table)
    assert stats[0] == 60 and stats[1] == void.sum() and stats[2] == 0
    assert void.any() and not void.all() and void.sum() * 1000 <= 500 * 60
    inside = np.zeros((6, 10), dtype=bool)
    inside[2:4, 3:6] = True                                # the replaced rectangle: rows 32..64, columns 48..96
    assert void[inside.reshape(-1)].all() and not void[~inside.reshape(-1)].any()
    want, _ = motion_ref.block_match(cur, ref, 8, 0)
    assert np.array_equal(table[~void], want[~void]) and (cost[void] > act[void]).all()
    # through the grid oracle: the cells of the intra blocks are identity cells, the others moved (dx = 5 stays in the block: use the table)
    grid, inv = motion_vectors_to_grids(table, H, W, default_like(H, W))
    ident = default_like(H, W)
    assert np.array_equal(grid.reshape(-1, 2)[void], ident.reshape(-1, 2)[void])
    # the same scene at a bias no SAD can pass: the old table
    table2, _, _, stats2 = modes_ref.block_match_modes(cur, ref, 8, 0, 65535, 0)
    assert np.array_equal(table2, want) and stats2.tolist() == [60, 0, 0, 0]


@pytest.mark.parametrize("channels", [1, 3])
def test_two_unrelated_textured_frames_are_a_cut(channels):
    cur, ref = modes_ref.unrelated_pair(H, W, seed=13, channels=channels)
    table, cost, act, stats = modes_ref.block_match_modes(cur, ref, 8, 0, 0, 500)
    assert stats[0] == 60 and stats[1] * 1000 > 500 * 60 and stats[2] == 1 and modes_ref.is_void(table).all()
    grid, inv = motion_vectors_to_grids(table, H, W, default_like(H, W))
    assert np.array_equal(grid, default_like(H, W)) and np.array_equal(inv, default_like(H, W))
    # without the cut rule only the intra blocks are void, and cost / activity do not depend on either rule
    table1, cost1, act1, stats1 = modes_ref.block_match_modes(cur, ref, 8, 0, 0, 1000)
    assert stats1.tolist() == [60, int(stats[1]), 0, 0] and modes_ref.is_void(table1).sum() == stats[1]
    assert np.array_equal(cost1, cost) and np.array_equal(act1, act)


def default_like(h, w):
    """The identity grid of an h x w frame's blocks, built as flow/model.py builds the 67 x 120 one."""
    hb, wb = h // 16, w // 16
    xs = (np.arange(wb) * 16 + 8) / (wb * 16) * 2 - 1
    ys = (np.arange(hb) * 16 + 8) / (hb * 16) * 2 - 1
    return np.stack(np.meshgrid(xs, ys), axis=-1).astype(np.float64)


def test_default_like_is_the_default_grid_at_the_product_geometry():
    assert np.array_equal(default_like(1072, 1920), get_default_grid())
