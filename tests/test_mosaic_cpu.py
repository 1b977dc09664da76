"""The flood-extent mosaic, the parts that need no GPU: the definition in numpy (tests/mosaic_ref.py) in its vectorised form against the
literal loops; csrc/mosaic_defs.h run on the CPU by a stand-alone sanitized host program; hand-computed canvases; the ninth hook table,
the refusals, FlowPredictor's argument checks and the CSV writer; and the end-to-end property of the definition on a synthetic
flight."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mosaic_ref as mref
import motion_ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import predict
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["global_motion", "pose_chain", "mosaic_accumulate", "mosaic_resolve"]
ONE = mref.ONE
IDENT = mref.IDENTITY


def small_tables():
    """(name, table, frame size, mask or None, exclude_set, pair_stats row or None) on 4 x 6 and 8 x 12 block grids."""
    out = []
    for hb, wb in ((4, 6), (8, 12)):
        size = (hb * 16, wb * 16)
        clean = mref.grid_table(hb, wb, mref.affine_vectors(hb, wb, degrees=2.0, zoom=1.03, shift=(7, -3)))
        out.append((f"affine{hb}", clean, size, None, 0, None))
        out.append((f"outliers{hb}", mref.with_outliers(clean, 0.3, 5), size, None, 0, None))
        void = clean.copy()
        void[::3] = mref.VOID_ROW
        out.append((f"void{hb}", void, size, None, 0, None))
        far = clean.copy()
        far[1::2, 3] += 40                                                   # |dx| > 32: not usable
        out.append((f"far{hb}", far, size, None, 0, None))
        mask = (np.add.outer(np.arange(size[0]), np.arange(size[1])) // 23 % 3).astype(np.uint8)
        mask[:5, :7] = 40                                                    # an id >= 32 is never excluded
        out.append((f"masked{hb}", clean, size, mask, 0b110, None))
        out.append((f"cut{hb}", clean, size, None, 0, [hb * wb, 0, 1, 0]))
        out.append((f"allvoid{hb}", np.tile(np.array(mref.VOID_ROW, np.int32), (hb * wb, 1)), size, None, 0, None))
        out.append((f"shift{hb}", mref.grid_table(hb, wb, lambda cx, cy: (np.full_like(cx, -5), np.full_like(cy, 9))), size, None, 0, None))
    one_row = mref.grid_table(1, 12, mref.affine_vectors(1, 12))                # a single block row: q is constant, the system singular
    out.append(("onerow", one_row, (16, 192), None, 0, None))
    return out


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("rounds", [0, 1, 4])
def test_vectorised_global_motion_equals_the_loop(rounds):
    statuses = set()
    for name, table, size, mask, exclude, stats in small_tables():
        kw = dict(rounds=rounds, tol=ONE, min_inliers=6, mask=None if mask is None else mask[None], exclude_set=exclude,
                  pair_stats=None if stats is None else np.array([stats], np.int32))
        for mask_size in (size, (37, 53)) if mask is None else (size,):
            a = mref.global_motion([table], size, mask_size, **kw)
            b = mref.global_motion_loop([table], size, mask_size, **kw)
            assert np.array_equal(a, b), (name, mask_size)
            statuses.add(int(a[0, 12]))
            if a[0, 12] != 0:
                assert a[0, :12].tolist() == IDENT + IDENT, name
    assert statuses == ({0, 1, 2} if rounds == 0 else {0, 1, 2, 3})              # the single block row is degenerate once a round solves


def test_global_motion_by_hand():
    hb, wb = 4, 6
    shift = mref.grid_table(hb, wb, lambda cx, cy: (np.full_like(cx, -5), np.full_like(cy, 9)))
    for rounds in (0, 1, 4):
        row = mref.global_motion([shift], (64, 96), (64, 96), rounds=rounds, tol=ONE, min_inliers=6)[0].tolist()
        assert row == [ONE, 0, -5 * ONE, 0, ONE, 9 * ONE] + [ONE, 0, 5 * ONE, 0, ONE, -9 * ONE] + [0, 24, 24, rounds]
    # a mask of half the frame's size: the translation halves, exactly
    row = mref.global_motion([shift], (64, 96), (32, 48), rounds=2, tol=ONE, min_inliers=6)[0].tolist()
    assert row[:6] == [ONE, 0, -5 * ONE // 2, 0, ONE, 9 * ONE // 2]
    # the mode's order: two translations with 12 rows each -- the smaller |dx| + |dy| wins; at equal magnitude the smaller dy, then dx
    for (a, b), want in ((((3, 0), (-2, 0)), (-2, 0)), (((0, 2), (0, -2)), (0, -2)), (((2, 0), (0, 2)), (2, 0)), (((2, 0), (-2, 0)), (-2, 0))):
        t = mref.grid_table(hb, wb, lambda cx, cy: (np.where(np.arange(24) % 2 == 0, a[0], b[0]), np.where(np.arange(24) % 2 == 0, a[1], b[1])))
        row = mref.global_motion([t], (64, 96), (64, 96), rounds=0, min_inliers=6)[0].tolist()
        assert (row[2], row[5], row[13], row[14]) == (want[0] * ONE, want[1] * ONE, 24, 12), (a, b)
    # too few: 5 usable rows against min_inliers = 6; a later round that runs short keeps the model of the round before
    few = np.tile(np.array(mref.VOID_ROW, np.int32), (24, 1))
    few[:5] = shift[:5]
    assert mref.global_motion([few], (64, 96), (64, 96), rounds=4, min_inliers=6)[0, 12:].tolist() == [2, 5, 5, 0]
    # an implausible model: a zoom of 1.5 between two frames
    zoom = mref.grid_table(8, 12, lambda cx, cy: (np.rint(0.3 * (cx - 96)).astype(np.int64), np.rint(0.3 * (cy - 64)).astype(np.int64)))
    row = mref.global_motion([zoom], (128, 192), (128, 192), rounds=4, tol=8 * ONE, min_inliers=6)[0].tolist()
    assert row[12] == 3 and row[:12] == IDENT + IDENT and row[15] >= 1
    # the tolerance doubles per round back from the last and is capped at 64 pixels
    assert [mref.round_tolerance(ONE, 4, r) for r in range(4)] == [8 * ONE, 4 * ONE, 2 * ONE, ONE]
    assert mref.round_tolerance(40 * ONE, 8, 0) == 64 * ONE and mref.round_tolerance(0, 8, 0) == 0


def small_canvases():
    """(mask [n, H, W], poses, K, canvas, origin): identity, shifts, a rotation, zooms, a lost frame, ids >= K."""
    rng = np.random.RandomState(11)
    mask = rng.randint(0, 4, size=(4, 9, 13)).astype(np.uint8)
    mask[:, 2, 3] = 7                                                        # >= K: votes nowhere
    c, s = np.cos(np.radians(30)), np.sin(np.radians(30))
    pairs = [mref.affine_pose(1, 0, 0, 1, 0, 0), mref.affine_pose(1, 0, 0, 1, -4.5, 3.25), mref.affine_pose(c, -s, s, c, 6, -2),
             mref.affine_pose(2, 0, 0, 2, -3, -3)]
    poses = mref.pose_rows(pairs, status=[0, 1, 2, 0])
    return [(mask, poses, 4, (16, 20), (3, 2)), (mask[:2], mref.pose_rows([mref.affine_pose(0.5, 0, 0, 0.5, 0, 0), pairs[2]]), 5, (11, 7), (-2, 4))]


def test_vectorised_accumulate_and_resolve_equal_the_loops():
    for mask, poses, k, canvas, origin in small_canvases():
        start = np.random.RandomState(3).randint(0, 3, size=(k,) + canvas).astype(np.uint16)
        start[0, 0, :] = 65535
        a = mref.mosaic_accumulate(mask, poses, start.copy(), origin)
        b = mref.mosaic_accumulate_loop(mask, poses, start.copy(), origin)
        assert np.array_equal(a, b) and not np.array_equal(a, start) and (a[0, 0] == 65535).all()
        for x, y in zip(mref.mosaic_resolve(a), mref.mosaic_resolve_loop(a)):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ hand-computed canvases
def test_hand_computed_votes():
    rng = np.random.RandomState(5)
    mask = rng.randint(0, 3, size=(1, 6, 8)).astype(np.uint8)
    onehot = np.stack([mask[0] == k for k in range(3)]).astype(np.uint16)
    # an identity pose with a canvas the size of the frame: one-hot votes
    votes = mref.mosaic_accumulate(mask, mref.pose_rows([(IDENT, IDENT)]), np.zeros((3, 6, 8), np.uint16), (0, 0))
    assert np.array_equal(votes, onehot)
    # a translation pose shifts them: the frame's pixel (0, 0) lies at anchor (2, 1), the origin puts the anchor's corner at canvas (1, 3)
    pose = mref.affine_pose(1, 0, 0, 1, 2, 1)
    votes = mref.mosaic_accumulate(mask, mref.pose_rows([pose]), np.zeros((3, 10, 14), np.uint16), (1, 3))
    want = np.zeros((3, 10, 14), np.uint16)
    want[:, 2:8, 5:13] = onehot
    assert np.array_equal(votes, want)
    # a zoom of 2 fills without holes: every canvas pixel of the 12 x 16 footprint holds the vote of the frame pixel it halves to
    pose = mref.affine_pose(2, 0, 0, 2, 0, 0)
    votes = mref.mosaic_accumulate(mask, mref.pose_rows([pose]), np.zeros((3, 12, 16), np.uint16), (0, 0))
    assert np.array_equal(votes, np.repeat(np.repeat(onehot, 2, axis=1), 2, axis=2)) and (votes.sum(0) == 1).all()
    # saturation: 65534 + 1 = 65535, and it stays there
    full = np.full((3, 6, 8), 65534, np.uint16)
    twice = mref.pose_rows([(IDENT, IDENT), (IDENT, IDENT)])
    votes = mref.mosaic_accumulate(np.repeat(mask, 2, 0), twice, full, (0, 0))
    assert np.array_equal(votes, np.where(onehot == 1, 65535, 65534))
    # a lost frame votes nowhere, whatever its matrices say
    votes = mref.mosaic_accumulate(mask, mref.pose_rows([(IDENT, IDENT)], status=[2]), np.zeros((3, 6, 8), np.uint16), (0, 0))
    assert not votes.any()


def test_hand_computed_resolve():
    votes = np.zeros((3, 1, 5), np.uint16)
    votes[:, 0, 0] = (2, 2, 1)          # a tie: the lower id
    votes[:, 0, 1] = (0, 1, 3)
    votes[:, 0, 2] = (0, 0, 0)          # unseen
    votes[:, 0, 3] = (65535, 65535, 65535)
    votes[:, 0, 4] = (0, 7, 0)
    cls, conf, seen, totals = mref.mosaic_resolve(votes)
    assert cls.tolist() == [[0, 2, 255, 0, 1]] and seen.tolist() == [[5, 4, 0, 196605, 7]]
    assert conf.tolist() == [[(255 * 2 + 2) // 5, (255 * 3 + 2) // 4, 0, 85, 255]]
    assert totals.tolist() == [[2, 2 + 65535], [1, 2 + 1 + 65535 + 7], [1, 1 + 3 + 65535]]


def test_pose_chain_by_hand():
    shift = lambda dx, dy, status=0: [ONE, 0, dx * ONE, 0, ONE, dy * ONE, ONE, 0, -dx * ONE, 0, ONE, -dy * ONE, status, 20, 18, 4]  # noqa: E731
    failed = IDENT + IDENT + [2, 3, 3, 0]
    model = np.array([shift(99, 99), shift(3, -2), failed, failed, shift(1, 1), failed, failed, failed, shift(5, 5)], np.int64)
    poses, state = mref.pose_chain(model, np.zeros(32, np.int64), (40, 60), (100, 100), (10, 20), max_bridge=2)
    assert poses[:, 12].tolist() == [0, 0, 1, 1, 0, 1, 1, 2, 2]                 # two bridged, a good pair, two bridged, the third is one too many
    assert poses[:, [2, 5]].tolist()[:7] == [[0, 0], [3 * ONE, -2 * ONE], [6 * ONE, -4 * ONE], [9 * ONE, -6 * ONE], [10 * ONE, -5 * ONE],
                                             [11 * ONE, -4 * ONE], [12 * ONE, -3 * ONE]]
    assert poses[0, 14:].tolist() == [0, 0] and poses[1, 14:].tolist() == [18, 20]    # the anchor's own row is ignored
    assert poses[7].tolist() == IDENT + IDENT + [2, 0, 3, 3] and state[24:28].tolist() == [2, 9, 2, 2]
    # the same in pieces
    st = np.zeros(32, np.int64)
    parts = []
    for piece in (model[:3], model[3:5], model[5:]):
        got, st = mref.pose_chain(piece, st, (40, 60), (100, 100), (10, 20), max_bridge=2)
        parts.append(got)
    assert np.array_equal(np.concatenate(parts), poses) and np.array_equal(st, state)
    # a cut loses the chain at once; clipping at each edge; the translation bound
    poses, _ = mref.pose_chain(np.array([shift(0, 0), shift(1, 1), shift(0, 0, 1), shift(1, 1)], np.int64), np.zeros(32, np.int64), (40, 60), (100, 100), (0, 0))
    assert poses[:, 12].tolist() == [0, 0, 2, 2]
    for dx, dy, origin, clipped in ((0, 0, (10, 20), 0), (-21, 0, (10, 20), 1), (21, 0, (10, 20), 1), (20, 0, (10, 20), 0), (0, -11, (10, 20), 1),
                                    (0, 51, (10, 20), 1), (0, 50, (10, 20), 0)):
        poses, _ = mref.pose_chain(np.array([shift(0, 0), shift(dx, dy)], np.int64), np.zeros(32, np.int64), (40, 60), (100, 100), origin)
        assert poses[1, 13] == clipped, (dx, dy)
    big = np.array([shift(0, 0)] + [shift(4000, 0)] * 5, np.int64)
    poses, _ = mref.pose_chain(big, np.zeros(32, np.int64), (40, 60), (100, 100), (0, 0))
    assert poses[:, 12].tolist() == [0, 0, 0, 0, 0, 2] and poses[4, 2] == 16000 * ONE   # 20000 >= 2^14: lost


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def clip_cases():
    """(to_anchor, clipped) for a 40 x 60 frame on a 100 x 100 canvas with its anchor at (20, 10): the header tests the corners' bounding
    box, the reference corner by corner.  Each edge of the canvas in turn: the extreme corner exactly ON it (inside), and one Q20 unit
    beyond it (clipped); upright, and turned by 30 degrees, where each of the four extrema comes from another corner."""
    (h, w), (ch, cw), (oy, ox) = (40, 60), (100, 100), (10, 20)
    c, s = np.cos(np.radians(30)), np.sin(np.radians(30))
    cases = []
    for lin in ([ONE, 0, 0, ONE], [int(round(v * ONE)) for v in (c, -s, s, c)]):
        corners = ((0, 0), (w, 0), (0, h), (w, h))
        xs, ys = [lin[0] * x + lin[1] * y for x, y in corners], [lin[2] * x + lin[3] * y for x, y in corners]
        if lin[1]:
            assert len({xs.index(min(xs)), xs.index(max(xs)), ys.index(min(ys)), ys.index(max(ys))}) == 4
        left, right = -min(xs) - ox * ONE, cw * ONE - max(xs) - ox * ONE      # the translations that put the box's edge on the canvas's
        top, bottom = -min(ys) - oy * ONE, ch * ONE - max(ys) - oy * ONE
        assert left < right and top < bottom                                  # the box fits: between the two the frame is inside
        for tx, ty, clipped in ((left, top, 0), (right, bottom, 0), (left - 1, top + ONE, 1), (right + 1, top + ONE, 1), (left + ONE, top - 1, 1),
                                (left + ONE, bottom + 1, 1), (left + ONE, top + ONE, 0)):
            cases.append(([lin[0], lin[1], tx, lin[2], lin[3], ty], clipped))
    return cases


def host_commands():
    """(commands, expected output lines) for tests/mosaic_host_check.cpp, from the numpy reference and from arithmetic."""
    rng = np.random.RandomState(17)
    cmds, want = [], []

    def add(cmd, out):
        cmds.append(" ".join(str(int(v)) if not isinstance(v, str) else v for v in cmd))
        want.append(" ".join(str(int(v)) for v in out))

    for v in (0, 1, -1, (1 << 19) - 1, 1 << 19, -(1 << 19), -(1 << 19) - 1, 3 * ONE // 2, -3 * ONE // 2, -5 * ONE // 2, (1 << 62) - 1, -(1 << 62)):
        add(["rshr", v], [(v + (1 << 19)) // ONE])                           # floor division: what an arithmetic shift does
    for _ in range(40):
        a = [int(v) for v in rng.randint(-(1 << 23), 1 << 23, size=6)]
        b = [int(v) for v in rng.randint(-(1 << 21), 1 << 21, size=6)]
        a[2], a[5], b[2], b[5] = (int(v) for v in rng.randint(-(1 << 33), 1 << 33, size=4))
        add(["compose"] + a + b, mref.compose(a, b))
    for count, dx, dy in ((0, 0, 0), (7, -32, 32), (7, 32, -32), (1 << 20, 5, -9), (3, 0, -1)):
        bin_ = (dy + 32) * 65 + dx + 32
        key = int(mref.mode_key(np.array([count]), np.array([bin_]))[0])
        add(["key", count, bin_], [key, count, dx, dy])
    for tol, rounds, r in ((ONE, 4, 0), (ONE, 4, 3), (40 * ONE, 8, 0), (64 * ONE, 8, 0), (0, 1, 0), (3, 8, 0)):
        add(["tol", tol, rounds, r], [mref.round_tolerance(tol, rounds, r)])
    sums = []
    for name, table, size, mask, exclude, stats in small_tables():
        if stats is not None:
            continue
        p, q, dx, dy = mref.usable_rows(table, size[0], size[1], mask, size[0], size[1], exclude)
        sums.append([int(v) for v in (len(p), p.sum(), q.sum(), (p * p).sum(), (p * q).sum(), (q * q).sum(), dx.sum(), (p * dx).sum(), (q * dx).sum(), dy.sum(),
                                      (p * dy).sum(), (q * dy).sum())])
        for rounds in (0, 1, 4):
            for mask_size in (size, (37, 53)) if mask is None else (size,):
                row = mref.global_motion([table], size, mask_size, rounds=rounds, tol=ONE, min_inliers=6, mask=None if mask is None else mask[None],
                                         exclude_set=exclude)[0]
                add(["motion", size[0], size[1], mask_size[0], mask_size[1], rounds, ONE, 6, exclude, int(mask is not None), len(table)]
                    + table.reshape(-1).tolist() + ([] if mask is None else mask.reshape(-1).tolist()), row)
    sums.append([0] * 12)
    sums.append([10, 0, 0, 40, 0, 0, 5, 3, 0, 1, 2, 0])                        # q constant: the determinant is 0
    for s in sums:
        got = mref.gm_solve(s)
        add(["solve"] + s, [0] * 7 if got is None else [1] + got)
    models = [[0] * 6, [7 * ONE, ONE // 16, -ONE // 32, -3 * ONE, ONE // 64, ONE // 16], [ONE, 3 * ONE, 0, 0, 0, 0], [0, 0, 0, 0, 0, -2 * ONE - 1]]
    models += [[int(v) for v in rng.randint(-ONE // 2, ONE // 2, size=6)] for _ in range(12)]
    for model in models:
        for fh, fw, h, w in ((128, 192, 128, 192), (1072, 1920, 268, 480), (144, 176, 37, 53)):
            got = mref.gm_finish(model, fh, fw, h, w)
            add(["finish"] + model + [fh, fw, h, w], [0] + IDENT + IDENT if got is None else [1] + got[0] + got[1])
    shift = lambda dx, dy, status=0: [ONE, 0, dx * ONE, 0, ONE, dy * ONE, ONE, 0, -dx * ONE, 0, ONE, -dy * ONE, status, 20, 18, 4]  # noqa: E731
    wild = [1 << 40] * 12 + [0, 1, 1, 1]                                     # status ok, entries out of the pair bounds: counts as degenerate
    state = np.zeros(32, np.int64)
    for row in [shift(9, 9), shift(3, -2), IDENT + IDENT + [3, 0, 0, 0], wild, shift(-40, 7), IDENT + IDENT + [7, 0, 0, 0], shift(20000, 0), shift(1, 1),
                shift(0, 0, 1), shift(1, 1)]:
        poses, after = mref.pose_chain(np.array([row], np.int64), state, (40, 60), (100, 100), (10, 20), max_bridge=2)
        add(["pose"] + state.tolist() + row + [40, 60, 100, 100, 20, 10, 2], poses[0].tolist() + after.tolist())
        state = after
        if after[24] == 2:
            state = np.zeros(32, np.int64)                                   # lost is sticky: go on from a fresh state
    for to, clipped in clip_cases():                                         # a tracking chain that stands at `to`, and a pair that moves nothing
        state = np.zeros(32, np.int64)
        state[0:6], state[6:12], state[12:18], state[18:24], state[24] = to, IDENT, IDENT, IDENT, 1
        row = IDENT + IDENT + [0, 20, 18, 4]
        poses, after = mref.pose_chain(np.array([row], np.int64), state, (40, 60), (100, 100), (10, 20), max_bridge=2)
        assert poses[0, :6].tolist() == to and poses[0, 12] == 0 and poses[0, 13] == int(clipped), (to, poses[0])   # the reference first
        add(["pose"] + state.tolist() + row + [40, 60, 100, 100, 20, 10, 2], poses[0].tolist() + after.tolist())
    c, s = np.cos(np.radians(30)), np.sin(np.radians(30))
    for back in (IDENT, mref.affine_pose(c, -s, s, c, 6, -2)[1], mref.affine_pose(0.5, 0, 0, 0.5, -100.25, 3)[1], mref.affine_pose(2, 0, 0, 2, 1, 1)[1]):
        for X, Y, ox, oy in ((0, 0, 0, 0), (5, 7, 3, -2), (16383, 0, -16384, 16384), (0, 16383, 16384, -16384)):
            ax, ay = (2 * (X - ox) + 1) << 19, (2 * (Y - oy) + 1) << 19
            add(["pixel"] + back + [X, Y, ox, oy], [(mref.rshr(back[0] * ax + back[1] * ay) + back[2]) >> 20, (mref.rshr(back[3] * ax + back[4] * ay) + back[5]) >> 20])
    for tile, touch in (((0, 0, 64, 16), 1), ((64, 0, 128, 16), 0), ((54, 0, 64, 16), 1), ((0, 48, 64, 64), 0), ((0, 41, 64, 57), 1), ((61, 41, 125, 57), 1)):
        add(["touch"] + IDENT + list(tile) + [0, 0, 40, 60], [touch])        # a 40 x 60 frame at the origin, one pixel of slack
    for v, more, out in ((0, 1, 1), (65534, 1, 65535), (65535, 1, 65535), (65000, 64, 65064), (65500, 64, 65535)):
        add(["vote", v, more], [out])
    for most, total in ((0, 0), (2, 5), (3, 4), (65535, 196605), (7, 7), (1, 2097120)):
        add(["conf", most, total], [0 if total == 0 else (255 * most + total // 2) // total])
    return cmds, want


def test_the_headers_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/mosaic_defs.h is plain __host__ __device__ C++: tests/mosaic_host_check.cpp runs rshr with negative operands, compose, the
    mode key, the tolerance, gm_solve, gm_finish with its inverse, whole pair fits, the pose step, the gather's rounding, the tile test,
    saturation and the confidence code as a stand-alone program built with -fsanitize=address,undefined and without fused
    multiply-adds; every line it prints is the reference's."""
    makefile = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "mosaic_host_check"), str(tmp_path / "commands.txt")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc"), os.path.join(ROOT, "tests", "mosaic_host_check.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):   # the runtimes linked in where the compiler can
        build = subprocess.run(base + static, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    cmds, want = host_commands()
    with open(data, "w") as fh:
        fh.write("\n".join(cmds) + "\n")
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(want) and len(want) > 200
    for cmd, g, w in zip(cmds, got, want):
        assert g == w, (cmd[:200], g, w)


def test_the_solve_is_within_one_unit_of_an_independent_solver():
    """np.linalg.solve (LU with pivoting) on the same normal equations: the float64 solve of these small systems is good to about 1e-7
    units of Q20, so only a tie can flip a rounding -- within 1 unit everywhere; pure translations come out exactly, slopes exactly 0."""
    checked = 0
    for name, table, size, mask, exclude, stats in small_tables():
        p, q, dx, dy = mref.usable_rows(table, size[0], size[1], mask, size[0], size[1], exclude)
        s = [int(v) for v in (len(p), p.sum(), q.sum(), (p * p).sum(), (p * q).sum(), (q * q).sum(), dx.sum(), (p * dx).sum(), (q * dx).sum(), dy.sum(),
                              (p * dy).sum(), (q * dy).sum())]
        got = mref.gm_solve(s)
        if got is None:
            continue
        m = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]], np.float64)
        want = np.concatenate([np.linalg.solve(m, np.array(s[6:9], np.float64)), np.linalg.solve(m, np.array(s[9:12], np.float64))]) * ONE
        assert np.abs(np.array(got) - want).max() <= 1.0, name
        if name.startswith("shift"):
            assert got == [-5 * ONE, 0, 0, 9 * ONE, 0, 0]
        checked += 1
    assert checked >= 10


# ------------------------------------------------------------------------------------------------ library surface
def test_the_ninth_table_in_header_initialiser_and_binding():
    assert _lib.ext8_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext8_api {"):text.index("} fs_ext8_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == _lib.ext8_hook_names()
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables7;") < text.index("typedef struct fs_ext8_api {") < text.index("typedef struct fs_hook_tables8 {")
    tables8 = text[text.index("typedef struct fs_hook_tables8 {"):text.index("} fs_hook_tables8;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables8) == [("fs_hook_tables7", "base7"), ("fs_ext8_api", "ext8")]
    assert int(re.search(r"#define FS_EXT8_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT8_MAGIC == int.from_bytes(b"FSEXTAB8", "big")
    assert int(re.search(r"#define FS_POSE_FRAC (\d+)", text).group(1)) == mref.FRAC and ops.POSE_ONE == ONE
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables8 all8 = {all7, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT8_MAGIC," in init and "sizeof(fs_ext8_api)," in init
    assert re.search(r"const fs_hook_tables7& all7 = all8\.base7;\s+const fs_hook_tables6& all6 = all7\.base6;\s+return all6\.base5;", src)
    kernels = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "kernels.h")).read()
    assert all("launch_" + name in kernels for name in NEW)
    # the eight older tables and the export list are what they were: ext7 still holds its two members
    assert [len(_lib.hook_names()), len(_lib.ext_hook_names()), len(_lib.ext2_hook_names()), len(_lib.ext3_hook_names()), len(_lib.ext4_hook_names()),
            len(_lib.ext5_hook_names()), len(_lib.ext6_hook_names()), len(_lib.ext7_hook_names())] == [38, 2, 14, 1, 1, 1, 1, 2]
    assert [ctypes.sizeof(t) for t in (_lib.FsExtApi, _lib.FsExt2Api, _lib.FsExt3Api, _lib.FsExt4Api, _lib.FsExt5Api, _lib.FsExt6Api, _lib.FsExt7Api)] == \
        [32, 128, 24, 24, 24, 24, 32]
    assert _lib.ext7_hook_names() == ["mask_distance", "region_proximity"]
    assert not any("fs_" + name in _lib.exported_symbols() for name in NEW) and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    public = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(name in public for name in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables8.ext8.offset == ctypes.sizeof(_lib.FsHookTables7)                           # directly behind, no padding
    assert [getattr(_lib.FsExt8Api, name).offset for name in NEW] == [16, 24, 32, 40] and ctypes.sizeof(_lib.FsExt8Api) == 48
    all8 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables8)).contents
    assert all8.base7.ext7.magic == _lib.EXT7_MAGIC and all8.base7.ext7.size == 32
    assert all8.base7.base6.ext6.magic == _lib.EXT6_MAGIC and all8.base7.base6.base5.ext5.magic == _lib.EXT5_MAGIC
    assert all8.ext8.magic == _lib.EXT8_MAGIC and all8.ext8.size >= 48                                   # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all8.ext8, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                                            # a table member, not an exported symbol
    assert ctypes.cast(all8.base7.ext7.mask_distance, ctypes.c_void_p).value == ctypes.cast(lib.fs_mask_distance, ctypes.c_void_p).value
    # the header's constants are the reference's
    defs = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "mosaic_defs.h")).read()
    assert "constexpr int FRAC = 20;" in defs and "constexpr int MAX_VECTOR = 32;" in defs and "constexpr int64_t PLAUSIBLE = ONE / 4;" in defs
    assert "POSE_SHIFT_LIMIT = ((int64_t)1 << 14) * ONE" in defs and mref.POSE_SHIFT_LIMIT == (1 << 14) * ONE


def test_the_magic_is_checked_before_use(monkeypatch):
    """A binding that expects another magic finds no ninth table in this library and says so, instead of calling through it."""
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT8_MAGIC", _lib.EXT8_MAGIC + 1)
    with pytest.raises(RuntimeError, match="eighth extension table"):
        fresh.fs_global_motion
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT7_MAGIC", _lib.EXT7_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first eight hook tables"):
        fresh.fs_mosaic_resolve
    monkeypatch.undo()
    assert all(getattr(fresh, "fs_" + name) is not None for name in NEW) and fresh.fs_mask_distance is not None


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    assert len(mref.refusal_cases()) >= 50
    for op, kw, word in mref.refusal_cases():
        assert mref.call_mosaic_op(lib, op, **kw) != 0, (op, kw)
        msg = lib.fs_last_error()
        assert msg.startswith(op.encode() + b":") and word in msg, (op, kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
def test_ops_refuse_with_the_offending_value():
    tables = torch.zeros((2, 24, 7), dtype=torch.int32)
    good = dict(tables=tables, frame_size=(64, 96), mask_size=(64, 96))
    for kw, word in ((dict(rounds=9), "9"), (dict(tol=65.0), "65.0"), (dict(tol=-1), "-1"), (dict(min_inliers=2), "2"), (dict(exclude=(32,)), "32"),
                     (dict(frame_size=(8, 96)), "(8, 96)"), (dict(mask_size=(0, 5)), "(0, 5)"), (dict(tables=tables[:, :5]), "(2, 5, 7)"),
                     (dict(tables=tables.long()), "int64"), (dict(mask=torch.zeros((2, 64, 95), dtype=torch.uint8)), "(2, 64, 95)"),
                     (dict(pair_stats=torch.zeros((1, 4), dtype=torch.int32)), "(1, 4)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.global_motion(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.global_motion: tensors must live on the GPU"):
        ops.global_motion(**good)
    model, state = torch.zeros((3, 16), dtype=torch.int64), torch.zeros((32,), dtype=torch.int64)
    good = dict(model=model, state=state, mask_size=(64, 96), canvas_size=(100, 100), origin=(0, 0))
    for kw, word in ((dict(max_bridge=65), "65"), (dict(canvas_size=(0, 9)), "(0, 9)"), (dict(origin=(20000, 0)), "20000"), (dict(model=model[:, :8]), "(3, 8)"),
                     (dict(state=state[:16]), "(16,)"), (dict(mask_size=(64, 16385)), "16385")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.pose_chain(**{**good, **kw})
    mask, votes = torch.zeros((3, 8, 8), dtype=torch.uint8), torch.zeros((5, 9, 9), dtype=torch.uint16)
    for kw, word in ((dict(mask=mask.int()), "int32"), (dict(poses=model[:2]), "(2, 16)"), (dict(votes=votes.to(torch.int16)), "int16"),
                     (dict(votes=torch.zeros((33, 2, 2), dtype=torch.uint16)), "(33, 2, 2)"), (dict(origin=(0, -16385)), "-16385")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.mosaic_accumulate(**{**dict(mask=mask, poses=model, votes=votes, origin=(0, 0)), **kw})
    with pytest.raises(ValueError, match="uint8"):
        ops.mosaic_resolve(votes.to(torch.uint8))
    with pytest.raises(RuntimeError, match="floodseg.mosaic_resolve: tensors must live on the GPU"):
        ops.mosaic_resolve(votes)


def test_predictor_argument_checks():
    ident = torch.nn.Identity()
    p = FlowPredictor(ident)
    assert p.mosaic is None and p.mosaic_builder.votes is None
    cls, conf, seen, totals, poses = p.mosaic_report()
    assert cls.shape == (0, 0) and totals.shape == (5, 2) and poses.shape == (0, 16)
    assert p._link_inputs(3, None, None, None) is None                       # off: no vectors are asked for
    on = FlowPredictor(ident, mosaic=(300, 400))                                # it does not need regions=True
    assert on.mosaic == (300, 400) and on.mosaic_builder.classes == 5 and on.mosaic_builder.exclude == (1,) and on.mosaic_builder.bridge == 2 and on.mosaic_builder.origin is None
    assert (on.mosaic_builder.rounds, on.mosaic_builder.tol, on.mosaic_builder.min_inliers) == (4, 1.0, 12)
    cls, conf, seen, totals, poses = on.mosaic_report()
    assert cls.shape == (300, 400) and (cls == 255).all() and not conf.any() and not seen.any() and poses.shape == (0, 16)
    with pytest.raises(ValueError, match="mosaic=\\(CH, CW\\) needs link_mvs and link_frame_size"):
        on._link_inputs(3, None, None, None)
    for kw, word in ((dict(mosaic=(0, 5)), "(0, 5)"), (dict(mosaic=(5, 16385)), "16385"), (dict(mosaic=(5,)), "(5,)"), (dict(mosaic_classes=33), "33"),
                     (dict(mosaic_rounds=9), "9"), (dict(mosaic_tol=100), "100"), (dict(mosaic_min_inliers=2), "2"), (dict(mosaic_exclude=(40,)), "40"),
                     (dict(mosaic_bridge=-1), "-1"), (dict(mosaic_origin=(1, 2, 3)), "(1, 2, 3)"), (dict(mosaic_origin=(0, 20000)), "20000")):
        with pytest.raises(ValueError, match=re.escape(word)):
            FlowPredictor(ident, **{**dict(mosaic=(300, 400)), **kw})
    assert FlowPredictor(ident, mosaic=(9, 9), mosaic_classes=32, mosaic_exclude=(), mosaic_origin=(-3, 4)).mosaic_builder.origin == (-3, 4)


def test_the_mosaic_csv(tmp_path):
    shift = lambda dx, dy, status, clipped: [ONE, 0, dx * ONE, 0, ONE, dy * ONE, ONE, 0, -dx * ONE, 0, ONE, -dy * ONE, status, clipped, 18, 20]  # noqa: E731
    poses = np.array([shift(0, 0, 0, 0), [ONE + ONE // 4, -ONE // 8, 3 * ONE // 2, 0, ONE, -7 * ONE] + IDENT + [1, 1, 3, 9], IDENT + IDENT + [2, 0, 0, 0]], np.int64)
    totals = np.array([[30, 100], [10, 50], [0, 0]], np.int64)
    path = str(tmp_path / "m.csv")
    predict.write_mosaic_csv(path, [7, 8, 9], poses, totals)
    assert open(path).read().split("\n") == [
        "frame,status,clipped,inliers,usable,m00,m01,m02,m10,m11,m12",
        "7,ok,0,18,20,1.000000,0.000000,0.000000,0.000000,1.000000,0.000000",
        "8,bridged,1,3,9,1.250000,-0.125000,1.500000,0.000000,1.000000,-7.000000",
        "9,lost,0,0,0,,,,,,",
        "",
        "class,pixels,share,votes",
        "0,30,0.750000,100",
        "1,10,0.250000,50",
        "2,0,0.000000,0",
        ""]
    predict.write_mosaic_csv(path, [], np.zeros((0, 16), np.int64), np.zeros((2, 2), np.int64))
    assert open(path).read().split("\n")[2:] == ["class,pixels,share,votes", "0,0,0.000000,0", "1,0,0.000000,0", ""]
    with pytest.raises(ValueError, match="poses must be"):
        predict.write_mosaic_csv(path, [7], poses, totals)


def test_tool_refuses_a_mosaic_without_vectors(capsys):
    spec = importlib.util.spec_from_file_location("predict_video_tool_mosaic", os.path.join(ROOT, "tools", "predict_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw = ["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights"]
    a = tool.parse_args(raw + ["--mosaic", "m.png"])
    assert a.mosaic == "m.png" and a.grids == "estimate" and a.mosaic_size is None and a.mosaic_exclude == [1]
    assert (a.mosaic_rounds, a.mosaic_tol, a.mosaic_report) == (4, 1.0, None) and tool.parse_args(raw).mosaic is None
    a = tool.parse_args(["--data-root", "d", "--synthetic-weights", "--grids", "estimate", "--mosaic", "m.png", "--mosaic-size", "300", "400", "--mosaic-exclude",
                         "--mosaic-rounds", "0", "--mosaic-tol", "2.5", "--mosaic-report", "m.csv"])
    assert (a.mosaic_size, a.mosaic_exclude, a.mosaic_rounds, a.mosaic_tol, a.mosaic_report) == ([300, 400], [], 0, 2.5, "m.csv")
    capsys.readouterr()
    for bad, word in ((["--data-root", "d", "--synthetic-weights", "--mosaic", "m.png"], "hold grids"),
                      (["--data-root", "d", "--synthetic-weights", "--grids", "files", "--mosaic", "m.png"], "hold grids"),
                      (raw + ["--no-warp", "--mosaic", "m.png"], "--no-warp estimates none"),
                      (raw + ["--mosaic-report", "m.csv"], "need --mosaic"), (raw + ["--mosaic-size", "9", "9"], "need --mosaic"),
                      (raw + ["--mosaic", "m.png", "--mosaic-size", "0", "9"], "1..16384"), (raw + ["--mosaic", "m.png", "--mosaic-rounds", "9"], "0..8"),
                      (raw + ["--mosaic", "m.png", "--mosaic-tol", "65"], "0..64"), (raw + ["--mosaic", "m.png", "--mosaic-exclude", "32"], "0..31")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert word in capsys.readouterr().err, bad


# ------------------------------------------------------------------------------------------------ the definition end to end
def test_a_synthetic_flight_is_mosaicked_without_a_single_wrong_pixel():
    """Six 128 x 192 views of a 256 x 384 textured world with a four-class label map, the tables from the block matcher's reference: every
    pair model is its exact integer translation with zero slopes, `seen` is the analytic coverage count, and the mosaic shows the world's
    labels on all 28434 seen pixels.  Zero mismatches is the condition."""
    frames, masks, offsets, labels = mref.scene()
    tables = [motion_ref.block_match(frames[i], frames[max(i - 1, 0)], search=16)[0] for i in range(6)]
    model, poses, state, votes, (cls, conf, seen, totals) = mref.run_scene(tables, masks)
    for i, (dy, dx) in enumerate(mref.SCENE_STEPS, start=1):
        assert model[i].tolist()[:13] == [ONE, 0, dx * ONE, 0, ONE, dy * ONE, ONE, 0, -dx * ONE, 0, ONE, -dy * ONE, 0], i   # frame i -> frame i - 1
        assert model[i, 13] == 96 and model[i, 14] >= 60 and model[i, 15] == 4
    assert poses[:, 12].tolist() == [0] * 6 and poses[:, 13].tolist() == [0] * 6
    assert poses[:, [5, 2]].tolist() == [[(y - offsets[0][0]) * ONE, (x - offsets[0][1]) * ONE] for y, x in offsets]
    want_seen, want_cls = mref.scene_expectation()
    assert np.array_equal(seen, want_seen) and seen.max() == 6 and int((seen > 0).sum()) == 28434
    assert int((cls != want_cls).sum()) == 0
    assert (conf[seen > 0] == 255).all() and totals[:, 0].sum() == 28434 and totals[:, 1].sum() == 6 * 128 * 192
    assert len(np.unique(cls[seen > 0])) == 4 and state[24:28].tolist() == [1, 6, 0, 0]
    # the loop form of the fit agrees on this scene too
    assert np.array_equal(mref.global_motion_loop(tables, mref.SCENE_VIEW, mref.SCENE_VIEW, **mref.SCENE_SETTINGS), model)
