"""Relocalisation against the orthophoto, the parts that need no GPU: the definition in numpy (tests/relocate_ref.py) in its vectorised form
against the literal loops; csrc/relocate_defs.h run on the CPU by a stand-alone sanitized host program; the thirteenth hook table and the
freeze of the twelfth; the library's refusals, the argument checks of the ops, FlowPredictor and the tool; and properties of the
definition run on the reference alone: a shift of 0, a shift and back, every tie rule on a constant canvas, and two synthetic flights
with a scene cut -- one onto ground mapped earlier, which is recovered to the exact poses, one onto unmapped ground, which stays lost."""
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
import placement_rows
import refine_ref as rref
import relocate_ref as lref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor, write_relocate_csv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc")
NEW = ["map_coarse", "map_patch", "map_locate", "pose_relocate", "relocate_commit"]
ONE = mref.ONE
CANVAS, ORIGIN = (100, 150), (20, 30)


def random_canvas(size=CANVAS, seed=3, holes=True):
    """A canvas of random pixels, seen everywhere but for two unseen rectangles."""
    rng = np.random.RandomState(seed)
    rgba = (rng.randint(0, 1 << 24, size=size).astype(np.uint32) | np.uint32(0xFF000000))
    if holes:
        rgba[10:23, 40:61] = 0
        rgba[70:, :17] &= np.uint32(0x00FFFFFF)
    return rgba


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("s", [4, 8, 16])
def test_vectorised_coarse_equals_the_loop(s):
    rgba = random_canvas()
    (cl, cv), (ll, lv) = lref.map_coarse(rgba, s), lref.map_coarse_loop(rgba, s)
    assert np.array_equal(cl, ll) and np.array_equal(cv, lv) and cl.shape == (100 // s, 150 // s)
    assert 0 < cv.sum() < cv.size and (cl[cv == 0] == 0).all()


@pytest.mark.parametrize("s", [4, 8])
def test_vectorised_patch_equals_the_loop(s):
    size = (36, 44)
    img = np.random.RandomState(5).randint(0, 256, size=size + (3,)).astype(np.uint8)
    status = []
    for name, state in lref.patch_states(size):
        a, b = lref.map_patch(img, state, CANVAS, ORIGIN, s), lref.map_patch_loop(img, state, CANVAS, ORIGIN, s)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        status.append(int(a[2][0]))
        if a[2][0] == 0:
            assert a[0].shape == (a[2][4], a[2][3]) and a[2][5] == a[1].sum() and (a[0][a[1] == 0] == 0).all(), name
    assert status == [0, 0, 0, 0, 1, 2, 4, 3]
    # the identity at s = 4: a 9 x 11-cell patch at the origin's cell, every cell valid; rotated: the box is larger, its corners are not valid
    tl, tv, geom = lref.map_patch(img, lref.patch_states(size)[0][1], CANVAS, ORIGIN, 4)
    if s == 4:
        assert geom.tolist() == [0, 30 // 4, 20 // 4, 12, 9, geom[5], 0, 0] and tv[:, 1:-1].all()   # x 30..74: cells 7..18, the two at the ends cut
    tl, tv, geom = lref.map_patch(img, lref.patch_states(size)[2][1], CANVAS, ORIGIN, s)
    assert tv[0, 0] == 0 and tv[-1, -1] == 0 and tv[tv.shape[0] // 2, tv.shape[1] // 2] == 1 and geom[3] * s > 44 and geom[4] * s > 36


def test_vectorised_locate_equals_the_loop_with_holes_and_nothing_seen():
    size = (32, 48)
    rgba = random_canvas((96, 160), seed=8)
    img = np.random.RandomState(6).randint(0, 256, size=size + (3,)).astype(np.uint8)
    cl, cv = lref.map_coarse(rgba, 4)
    tl, tv, geom = lref.map_patch(img, lref.patch_states(size)[1][1], (96, 160), ORIGIN, 4)
    a, b = lref.map_locate(cl, cv, tl, tv, geom, 500, 2), lref.map_locate_loop(cl, cv, tl, tv, geom, 500, 2)
    assert np.array_equal(a, b) and a[0] == lref.FOUND and a[5] == 1 and a[10] == (24 - geom[4] + 1) * (40 - geom[3] + 1) and 0 < a[11] <= a[10]
    assert np.array_equal(lref.map_locate(cl, cv, tl, tv, geom, 1000, 0), lref.map_locate_loop(cl, cv, tl, tv, geom, 1000, 0))
    nothing = lref.map_locate(cl, np.zeros_like(cv), tl, tv, geom)
    assert nothing.tolist() == [lref.FOUND_NONE] + [0] * 9 + [a[10], 0, geom[5], 0, 0, 0]
    bad = geom.copy()
    bad[3] = 41
    assert lref.map_locate(cl, cv, tl, tv, bad).tolist() == [lref.FOUND_BAD_GEOM] + [0] * 15
    assert lref.map_locate(cl, cv, tl, tv, lref.map_patch(img, lref.patch_states(size)[4][1], (96, 160), ORIGIN, 4)[2])[0] == lref.FOUND_BAD_GEOM


def test_a_constant_canvas_exercises_every_tie_rule():
    """Every placement on a canvas of one grey has the same mean.  Seen everywhere: they differ in nothing, so the smallest v, then the
    smallest u wins, and the runner-up is the first placement outside the exclusion square.  With an unseen hole the placements that
    avoid it have the larger n and win first."""
    size, s = (32, 48), 4
    img = np.full(size + (3,), 90, np.uint8)
    state = lref.patch_states(size)[0][1]
    _, rgba = lref.constant_canvas((96, 160))
    cl, cv = lref.map_coarse(rgba, s)
    tl, tv, geom = lref.map_patch(img, state, (96, 160), ORIGIN, s)
    pu0, pv0 = int(geom[1]), int(geom[2])
    found = lref.map_locate(cl, cv, tl, tv, geom, 500, 2)
    assert found[:5].tolist() == [0, -pu0, -pv0, 0, geom[5]] and found[5:10].tolist() == [1, 3 - pu0, -pv0, 0, geom[5]]     # the next u past the square, same v
    assert lref.map_locate(cl, cv, tl, tv, geom, 500, 64)[5] == 0                                                         # nothing lies beyond 64 cells
    assert np.array_equal(found, lref.map_locate_loop(cl, cv, tl, tv, geom, 500, 2))
    _, holed = lref.constant_canvas((96, 160), hole=(0, 8, 0, 8))                                                         # cells (0..1, 0..1) unseen
    cl, cv = lref.map_coarse(holed, s)
    found = lref.map_locate(cl, cv, tl, tv, geom, 500, 2)
    assert tv[:, 0].sum() == 0 and tv[:, 1].all()                                                                         # x 30..77: the patch's first column of cells is cut
    assert found[:5].tolist() == [0, 1 - pu0, -pv0, 0, geom[5]]                                                           # the larger n first: its valid columns clear the hole
    a = (0, 10, 5, 5)
    assert lref.better((0, 11, 9, 9), a) and lref.better((0, 10, 9, 4), a) and lref.better((0, 10, 4, 5), a) and not lref.better(a, a)
    assert lref.better((1, 10, 0, 0), (3, 20, 0, 0)) and not lref.better((2, 10, 9, 9), (3, 20, 0, 0)) and lref.better(a, (0, 0, 0, 0)) and not lref.better((0, 0, 0, 0), a)


def test_a_shift_of_zero_and_a_shift_and_back_are_exact():
    for to, back in (mref.affine_pose(1, 0, 0, 1, 12, -5), mref.affine_pose(1.013, -0.04, 0.05, 0.97, -333.25, 801.5)):
        state = lref.lost_state(to, back)
        cs, cp = lref.relocate_step(lref.found_row(u=0, v=0, sad=0, n=5), state, s=8, **lref.STEP_GEOMETRY)
        assert cs[28] == lref.RELOCATED and cs[:12].tolist() == state[:12].tolist() == cp[:12].tolist()              # bit for bit
        for s in (4, 8, 16):
            for u, v in ((3, -7), (-120, 55), (1, 0)):
                there = lref.translate(to, back, s * u, s * v)
                assert lref.translate(*there, -s * u, -s * v) == (to, back)
                assert there[0][2] - to[2] == s * u * ONE and there[0][0:2] == to[0:2]
                # the translated inverse still inverts the translated pose at the frame's origin, to the rounding of the pair it came from
                assert mref.compose(there[1], there[0])[2] == mref.compose(back, to)[2]


def test_the_steps_by_hand():
    names = [c[0] for c in lref.step_cases()]
    assert sorted({c[5] for c in lref.step_cases()}) == [0, 1, 2, 3, 4, 6, 7] and len(set(names)) == len(names)
    for name, found, state, max_mean, ratio, decision in lref.step_cases():
        cs, cp = lref.relocate_step(found, state, s=4, max_mean=max_mean, ratio=ratio, **lref.STEP_GEOMETRY)
        assert cs[28] == decision and np.array_equal(cs[29:], state[29:]) and np.array_equal(cs[25:27], state[25:27]), name
        if decision == lref.RELOCATED:
            assert cs[24] == 1 and cs[27] == 0 and cs[12:24].tolist() == mref.IDENTITY * 2 and cp[12] == 0 and np.array_equal(cs[:12], cp[:12]), name
            assert cs[2] == state[2] + 4 * found[1] * ONE and cs[5] == state[5] + 4 * found[2] * ONE and np.array_equal(cs[[0, 1, 3, 4]], state[[0, 1, 3, 4]]), name
        else:
            assert np.array_equal(cs[:28], state[:28]) and cp.tolist() == mref.IDENTITY * 2 + [2, 0, 0, 0], name
    seen = set()
    for name, cs, cp, co, state, pose, found, status in lref.commit_cases():
        st, p, out = lref.commit_step(cs, cp, co, state, pose, found, 4)
        seen.add(status)
        assert out[0] == status, name
        if status == lref.RELOCATED:
            assert np.array_equal(st[:28], cs[:28]) and np.array_equal(st[28:], state[28:]) and np.array_equal(p[:14], cp[:14]) and np.array_equal(p[14:], pose[14:]), name
            assert out[1:5].tolist() == [4 * found[1], 4 * found[2], found[3], found[4]], name
        else:
            assert np.array_equal(st, state) and np.array_equal(p, pose), name
    assert seen == {0, 1, 2, 3, 4, 5, 6, 7}


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def host_commands():
    """(commands, expected output lines) for tests/relocate_host_check.cpp, from the numpy reference."""
    cmds, want = [], []

    def add(cmd, out):
        cmds.append(" ".join(str(int(v)) if not isinstance(v, str) else v for v in cmd))
        want.append(" ".join(str(int(v)) for v in out))

    flat = lambda a: [int(v) for v in np.asarray(a).reshape(-1)]  # noqa: E731
    rgba = random_canvas((37, 50), seed=2)
    rgba[5:9, 12:20] = 0
    for s in (4, 8, 16):
        cl, cv = lref.map_coarse(rgba, s)
        add(["coarse", 37, 50, s] + flat(rgba), flat(cl) + flat(cv))
    size = (36, 44)
    img = np.random.RandomState(5).randint(0, 256, size=size + (3,)).astype(np.uint8)
    grey = np.repeat(img[..., :1], 3, axis=2)                            # a grey image's luma is its grey: the program takes the lumas
    for s in (4, 8, 16):
        for name, state in lref.patch_states(size):
            head = [size[0], size[1], CANVAS[0], CANVAS[1], ORIGIN[1], ORIGIN[0], s] + flat(state)
            geom = lref.patch_geometry(state, size, CANVAS, ORIGIN, s)
            add(["geometry"] + head, geom)
            tl, tv, geom = lref.map_patch(grey, state, CANVAS, ORIGIN, s)
            add(["patch"] + head + flat(grey[..., 0]), flat(geom) + flat(tl) + flat(tv))
    far = lref.lost_state(*mref.affine_pose(15.9, -15.9, 15.9, 15.9, -16383.9, 16383.9))     # the corners' products at their bounds
    add(["geometry", 16384, 16384, 16384, 16384, -16384, 16384, 4] + flat(far), lref.patch_geometry(far, (16384, 16384), (16384, 16384), (16384, -16384), 4))
    rgba = random_canvas((48, 64), seed=8, holes=False)
    rgba[0:9, 20:31] = 0
    small = np.random.RandomState(6).randint(0, 256, size=(16, 24, 3)).astype(np.uint8)
    for s, (name, state) in ((4, lref.patch_states((16, 24))[1]), (4, lref.patch_states((16, 24))[2]), (8, lref.patch_states((16, 24))[0])):
        cl, cv = lref.map_coarse(rgba, s)
        tl, tv, geom = lref.map_patch(small, state, (48, 64), (10, 14), s)
        for permille, exclude in ((500, 2), (1000, 0), (1, 64)):
            add(["locate", cl.shape[0], cl.shape[1], permille, exclude] + flat(geom) + flat(cl) + flat(cv) + flat(tl) + flat(tv),
                lref.map_locate(cl, cv, tl, tv, geom, permille, exclude))
    _, grey_canvas = lref.constant_canvas((48, 64), hole=(0, 8, 0, 8))
    cl, cv = lref.map_coarse(grey_canvas, 4)
    tl, tv, geom = lref.map_patch(np.full((16, 24, 3), 90, np.uint8), lref.patch_states((16, 24))[0][1], (48, 64), (10, 14), 4)
    add(["locate", 12, 16, 500, 2] + flat(geom) + flat(cl) + flat(cv) + flat(tl) + flat(tv), lref.map_locate(cl, cv, tl, tv, geom, 500, 2))
    add(["locate", 12, 16, 500, 2] + flat(geom) + flat(cl) + flat(np.zeros_like(cv)) + flat(tl) + flat(tv), lref.map_locate(cl, np.zeros_like(cv), tl, tv, geom, 500, 2))
    bad = geom.copy()
    bad[4] = 13
    add(["locate", 12, 16, 500, 2] + flat(bad) + flat(cl) + flat(cv), lref.map_locate(cl, cv, tl, tv, bad, 500, 2))
    big = (255 * 65536, 65536, 9, 9)
    for a, b in (((0, 10, 5, 5), (0, 10, 5, 5)), ((0, 11, 9, 9), (0, 10, 5, 5)), ((0, 10, 9, 4), (0, 10, 5, 5)), ((0, 10, 4, 5), (0, 10, 5, 5)), ((1, 10, 0, 0), (3, 20, 0, 0)),
                 ((2, 10, 0, 0), (3, 20, 0, 0)), ((0, 0, 0, 0), (9, 1, 0, 0)), ((9, 1, 0, 0), (0, 0, 0, 0)), (big, (255 * 65536 - 1, 65536, 0, 0)), ((255 * 65535, 65535, 0, 0), big)):
        add(["better"] + list(a) + list(b), [int(lref.better(a, b))])
    g = lref.STEP_GEOMETRY
    for name, found, state, max_mean, ratio, decision in lref.step_cases():
        for s in (4, 16):
            cs, cp = lref.relocate_step(found, state, s=s, max_mean=max_mean, ratio=ratio, **g)
            add(["step", *g["mask_size"], *g["canvas_size"], g["origin"][1], g["origin"][0], s, max_mean, ratio] + flat(found) + flat(state), flat(cs) + flat(cp))
    for name, cs, cp, co, state, pose, found, status in lref.commit_cases():
        st, p, out = lref.commit_step(cs, cp, co, state, pose, found, 4)
        add(["commit", 4] + flat(cs) + flat(cp) + flat(co) + flat(state) + flat(pose) + flat(found), flat(out) + flat(st) + flat(p))
    for name, state, size, s, status, cells in box_cases():
        geom = lref.patch_geometry(state, size, CANVAS, ORIGIN, s)
        assert geom[0] == status and (cells is None or tuple(geom[1:5]) == cells), (name, geom)          # the reference first: the case is what it says
        add(["geometry", size[0], size[1], CANVAS[0], CANVAS[1], ORIGIN[1], ORIGIN[0], s] + flat(state), geom)
    for name, found, (to, back), code in placement_rows.gate_rows():
        for s in (4, 16):
            cs, cp = lref.relocate_step(found, lref.lost_state(to, back), s=s, max_mean=placement_rows.MAX_MEAN, ratio=placement_rows.RATIO, **g)
            assert cs[28] == code, name
            add(["step", *g["mask_size"], *g["canvas_size"], g["origin"][1], g["origin"][0], s, placement_rows.MAX_MEAN, placement_rows.RATIO] + flat(found)
                + flat(lref.lost_state(to, back)), flat(cs) + flat(cp))
    return cmds, want


def box_cases():
    """(name, state, mask size, S, status, (pu0, pv0, tw, th) or None) where a rule on the corners' box and a rule corner by corner could part:
    on CANVAS = 100 x 150 with its anchor at (30, 20), so 37 x 25 cells of 4.  The extrema of the rotated frame come from four different
    corners; its translation is then chosen in Q20 so that an edge of the box lies exactly on a pixel's edge, and one unit beyond it."""
    (oy, ox), cases = ORIGIN, []
    flat_to = lambda tx, ty: lref.lost_state([ONE, 0, tx * ONE, 0, ONE, ty * ONE], [ONE, 0, -tx * ONE, 0, ONE, -ty * ONE])  # noqa: E731
    cases.append(("as wide as the coarse canvas", flat_to(-ox, 0), (36, 148), 4, 0, (0, 5, 37, 9)))       # x 0..148: cells 0..36
    cases.append(("one cell wider", flat_to(1 - ox, 0), (36, 148), 4, 4, None))                           # x 1..149: cells 0..37
    cases.append(("one cell higher", flat_to(0, 1 - oy), (100, 44), 4, 4, None))                          # y 1..101: cells 0..25 of 25
    cases.append(("a box of no width", lref.lost_state([0, 0, 5 * ONE, 0, ONE, 0], mref.IDENTITY), (36, 44), 4, 3, None))   # hi == lo on a pixel's edge
    cases.append(("a box of no height", lref.lost_state([ONE, 0, 0, 0, 0, -3 * ONE], mref.IDENTITY), (36, 44), 8, 3, None))
    c, s = np.cos(np.radians(30)), np.sin(np.radians(30))
    lin = [int(round(v * ONE)) for v in (c, -s, s, c)]
    h, w = 36, 44
    corners = ((0, 0), (w, 0), (0, h), (w, h))
    xs, ys = [lin[0] * x + lin[1] * y for x, y in corners], [lin[2] * x + lin[3] * y for x, y in corners]
    assert len({xs.index(min(xs)), xs.index(max(xs)), ys.index(min(ys)), ys.index(max(ys))}) == 4
    wide, high = -(-(max(xs) - min(xs)) // ONE), -(-(max(ys) - min(ys)) // ONE)                            # whole pixels the box spans when it starts on an edge
    for d in (0, -1, 1):                                                                                  # the box starts at canvas pixel (40, 24) exactly, or a unit off
        to = [lin[0], lin[1], 40 * ONE - min(xs) - ox * ONE + d, lin[2], lin[3], 24 * ONE - min(ys) - oy * ONE + d]
        X0, X1, Y0, Y1 = 40 - (d < 0), 40 + wide + (d > 0 and (max(xs) - min(xs)) % ONE == 0), 24 - (d < 0), 24 + high + (d > 0 and (max(ys) - min(ys)) % ONE == 0)
        cells = (X0 // 4, Y0 // 4, (X1 + 3) // 4 - X0 // 4, (Y1 + 3) // 4 - Y0 // 4)
        cases.append((f"rotated, {d} units off the pixel's edge", lref.lost_state(to, mref.IDENTITY), (h, w), 4, 0, cells))
    # ... and its far edge exactly on a pixel's edge: one unit more takes another pixel, and with it another cell
    to = [lin[0], lin[1], 96 * ONE - max(xs) - ox * ONE, lin[2], lin[3], 64 * ONE - max(ys) - oy * ONE]
    for d, more in ((0, 0), (1, 1)):
        moved = to[:2] + [to[2] + d] + to[3:5] + [to[5] + d]
        X0, Y0 = (96 * ONE - (max(xs) - min(xs)) + d) // ONE, (64 * ONE - (max(ys) - min(ys)) + d) // ONE
        cells = (X0 // 4, Y0 // 4, 24 + more - X0 // 4, 16 + more - Y0 // 4)
        cases.append((f"rotated, the far edge {d} units past a cell's edge", lref.lost_state(moved, mref.IDENTITY), (h, w), 4, 0, cells))
    return cases


def test_the_headers_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/relocate_defs.h is plain __host__ __device__ C++: tests/relocate_host_check.cpp runs the coarse cells on a canvas exactly as
    large as it says, the patch geometry (also with every product at its bound), whole patches cell by cell, the search placement by
    placement with the header's order, and both steps in every status, as a stand-alone program built with
    -fsanitize=address,undefined; every line it prints is the reference's."""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "relocate_host_check"), str(tmp_path / "commands.txt")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tests", "relocate_host_check.cpp"), "-o", exe]
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
    assert len(got) == len(want) and len(want) > 100
    for cmd, g, w in zip(cmds, got, want):
        assert g == w, (cmd[:200], g[:200], w[:200])


# ------------------------------------------------------------------------------------------------ library surface
def test_the_thirteenth_table_and_the_freeze_of_the_twelfth():
    assert _lib.ext12_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext12_api {"):text.index("} fs_ext12_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == NEW
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables11;") < text.index("typedef struct fs_ext12_api {") < text.index("typedef struct fs_hook_tables12 {")
    tables12 = text[text.index("typedef struct fs_hook_tables12 {"):text.index("} fs_hook_tables12;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables12) == [("fs_hook_tables11", "base11"), ("fs_ext12_api", "ext12")]
    assert int(re.search(r"#define FS_EXT12_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT12_MAGIC == int.from_bytes(b"FSEXTA12", "big")
    # fs_ext11_api is frozen: the header and the binding name the same one member, 24 bytes
    frozen = text[text.index("typedef struct fs_ext11_api {"):text.index("} fs_ext11_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", frozen) == _lib.ext11_hook_names() == ["guide_vectors"]
    assert ctypes.sizeof(_lib.FsExt11Api) == 24
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables12 all12 = {all11, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT12_MAGIC," in init and "sizeof(fs_ext12_api)," in init
    assert re.search(r"const fs_hook_tables11& all11 = all12\.base11;\s+const fs_hook_tables10& all10 = all11\.base10;", src)
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    assert all("launch_" + name in kernels for name in NEW)
    # the twelve older tables and the export list are what they were
    assert [len(names()) for names in (_lib.hook_names, _lib.ext_hook_names, _lib.ext2_hook_names, _lib.ext3_hook_names, _lib.ext4_hook_names, _lib.ext5_hook_names,
                                       _lib.ext6_hook_names, _lib.ext7_hook_names, _lib.ext8_hook_names, _lib.ext9_hook_names, _lib.ext10_hook_names,
                                       _lib.ext11_hook_names)] == [38, 2, 14, 1, 1, 1, 1, 2, 4, 2, 3, 1]
    assert not any("fs_" + name in _lib.exported_symbols() for name in NEW) and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    public = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(name in public for name in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables12.ext12.offset == ctypes.sizeof(_lib.FsHookTables11)                         # directly behind, no padding
    assert [getattr(_lib.FsExt12Api, name).offset for name in NEW] == [16, 24, 32, 40, 48] and ctypes.sizeof(_lib.FsExt12Api) == 56
    all12 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables12)).contents
    assert all12.base11.ext11.magic == _lib.EXT11_MAGIC and all12.base11.ext11.size == 24                 # frozen: exactly, not from below
    assert all12.base11.base10.ext10.magic == _lib.EXT10_MAGIC and all12.base11.base10.ext10.size == 40
    assert all12.ext12.magic == _lib.EXT12_MAGIC and all12.ext12.size >= 56                               # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all12.ext12, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                                            # a table member, not an exported symbol
    assert ctypes.cast(all12.base11.ext11.guide_vectors, ctypes.c_void_p).value == ctypes.cast(lib.fs_guide_vectors, ctypes.c_void_p).value
    # the rules' header builds on refine_defs.h and leaves it alone; the kernels take their rules from it and use no atomics
    defs = open(os.path.join(CSRC, "relocate_defs.h")).read()
    assert '#include "refine_defs.h"' in defs and all(f"mos::{fn}(" in defs for fn in ("source_pixel", "anchor_coord", "pose_in_bounds", "frame_clipped"))
    assert "refn::luma_of(" in defs and "refn::seen(" in defs
    kernel = open(os.path.join(CSRC, "relocate_ops.hip")).read()
    assert all(f"relo::{fn}(" in kernel for fn in ("coarse_cell", "patch_geometry", "patch_source", "geom_ok", "eligible", "better", "outside", "write_found",
                                                    "relocate_step", "commit_step")) and "resized1<" in kernel and "__builtin_amdgcn_sad_u8(" in kernel
    code = re.sub(r"//[^\n]*", "", kernel.split("namespace fs {")[1])
    assert "atomic" not in code and "asm" not in code
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"\$\(OBJDIR\)/relocate_ops\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", makefile) and " relocate_ops.hip " in makefile


def test_the_magic_is_checked_before_use(monkeypatch):
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT12_MAGIC", _lib.EXT12_MAGIC + 1)
    with pytest.raises(RuntimeError, match="the library has no twelfth extension table \\(fs_map_locate is missing\\)"):
        fresh.fs_map_locate
    assert fresh.fs_guide_vectors is not None                                 # the tables in front of it stay usable
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT11_MAGIC", _lib.EXT11_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first twelve hook tables are not the ones this binding knows \\(fs_map_coarse is missing\\)"):
        fresh.fs_map_coarse
    monkeypatch.undo()
    assert all(getattr(fresh, "fs_" + name) is not None for name in NEW)


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    assert len(lref.refusal_cases()) >= 70
    for op, kw, word in lref.refusal_cases():
        assert lref.call_op(lib, op, **kw) != 0, (op, kw)
        msg = lib.fs_last_error()
        assert msg.startswith(op.encode() + b":") and word in msg, (op, kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
def test_ops_refuse_with_the_offending_value():
    rgba = torch.zeros((40, 64), dtype=torch.int32)
    for kw, word in ((dict(scale=5), "5"), (dict(scale=0), "0"), (dict(rgba=rgba.long()), "int64"), (dict(rgba=rgba[None]), "(1, 40, 64)"), (dict(rgba=rgba[:7], scale=8), "no cell"),
                     (dict(rgba=torch.zeros((16385, 4), dtype=torch.int32)), "16385")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.map_coarse(**{**dict(rgba=rgba, scale=8), **kw})
    with pytest.raises(RuntimeError, match="floodseg.map_coarse: tensors must live on the GPU"):
        ops.map_coarse(rgba, 8)
    frame, state = torch.zeros((16, 32, 3), dtype=torch.uint8), torch.zeros((32,), dtype=torch.int64)
    good = dict(source=(frame, None, "rgb24", "bt601", False), state=state, mask_size=(16, 32), canvas_size=(40, 64), origin=(0, 0), scale=4)
    for kw, word in ((dict(scale=2), "2"), (dict(state=state[:31]), "(31,)"), (dict(state=state.int()), "int32"), (dict(mask_size=(0, 32)), "(0, 32)"),
                     (dict(canvas_size=(40, 16385)), "16385"), (dict(canvas_size=(40, 15), scale=16), "no cell"), (dict(origin=(20000, 0)), "20000"),
                     (dict(source=(frame, None, "bgr24", "bt601", False)), "'bgr24'"), (dict(source=(frame, None, "rgb24")), "of 3")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.map_patch(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.map_patch: tensors must live on the GPU"):
        ops.map_patch(**good)
    cl, tl, geom = torch.zeros((10, 16), dtype=torch.uint8), torch.zeros((65536,), dtype=torch.uint8), torch.zeros((8,), dtype=torch.int64)
    good = dict(cl=cl, cv=cl.clone(), tl=tl, tv=tl.clone(), geom=geom)
    for kw, word in ((dict(min_overlap_permille=0), "got 0"), (dict(min_overlap_permille=1001), "1001"), (dict(exclude=-1), "-1"), (dict(exclude=65), "65"),
                     (dict(cv=cl[:9]), "(9, 16)"), (dict(cl=cl.int()), "int32"), (dict(tl=tl[:100]), "(100,)"), (dict(tv=tl.int()), "int32"), (dict(geom=geom[:7]), "(7,)"),
                     (dict(cl=torch.zeros((4097, 1), dtype=torch.uint8), cv=torch.zeros((4097, 1), dtype=torch.uint8)), "4097")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.map_locate(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.map_locate: tensors must live on the GPU"):
        ops.map_locate(**good)
    found = torch.zeros((16,), dtype=torch.int64)
    good = dict(found=found, state=state, mask_size=(64, 96), canvas_size=(128, 192), origin=(32, 48), scale=8)
    for kw, word in ((dict(max_mean=-1), "-1"), (dict(max_mean=256), "256"), (dict(ratio_permille=0), "got 0"), (dict(ratio_permille=1001), "1001"), (dict(scale=32), "32"),
                     (dict(found=found[:15]), "(15,)"), (dict(state=state.int()), "int32"), (dict(mask_size=(64, 0)), "(64, 0)"), (dict(origin=(0, -16385)), "-16385")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.pose_relocate(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.pose_relocate: tensors must live on the GPU"):
        ops.pose_relocate(**good)
    pose, out = torch.zeros((16,), dtype=torch.int64), torch.zeros((8,), dtype=torch.int64)
    good = dict(cand_state=state.clone(), cand_pose=pose.clone(), correct_out=out, state=state, pose=pose, found=found, scale=8)
    for kw, word in ((dict(scale=3), "3"), (dict(cand_state=state[:31]), "(31,)"), (dict(cand_pose=pose.int()), "int32"), (dict(correct_out=out[:7]), "(7,)"),
                     (dict(pose=torch.zeros((2, 16), dtype=torch.int64)), "(2, 16)"), (dict(found=found[:8]), "(8,)"), (dict(state=state[::2]), "(16,)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.relocate_commit(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.relocate_commit: tensors must live on the GPU"):
        ops.relocate_commit(**good)


def test_predictor_tool_and_csv_argument_checks(tmp_path, capsys):
    ident = torch.nn.Identity()
    off = FlowPredictor(ident, mosaic=(30, 40), ortho="centre", mosaic_refine=True)
    assert off.mosaic_relocate is False and (off.mosaic_builder.relocate_scale, off.mosaic_builder.relocate_every, off.mosaic_builder.relocate_min_overlap, off.mosaic_builder.relocate_exclude, off.mosaic_builder.relocate_max_mean,
                                             off.mosaic_builder.relocate_ratio) == (8, 1, 500, 2, 16, 800)
    with pytest.raises(ValueError, match="relocate_report\\(\\) needs mosaic_relocate=True"):
        off.relocate_report()
    with pytest.raises(ValueError, match="mosaic_relocate=True needs mosaic_refine=True"):
        FlowPredictor(ident, mosaic=(30, 40), ortho="centre", mosaic_relocate=True)
    for kw, word in ((dict(relocate_scale=5), "got 5"), (dict(relocate_every=0), "got 0"), (dict(relocate_min_overlap=0.0), "got 0.0"), (dict(relocate_min_overlap=1.5), "1.5"),
                     (dict(relocate_exclude=65), "got 65"), (dict(relocate_max_mean=256), "got 256"), (dict(relocate_ratio=1.01), "1.01")):
        with pytest.raises(ValueError, match=word):
            FlowPredictor(ident, mosaic=(30, 40), ortho="centre", mosaic_refine=True, mosaic_relocate=True, **kw)
    on = FlowPredictor(ident, mosaic=(30, 40), ortho="latest", mosaic_refine=True, mosaic_relocate=True, relocate_scale=4, relocate_every=3, relocate_ratio=0.5)
    assert on.mosaic_relocate and (on.mosaic_builder.relocate_scale, on.mosaic_builder.relocate_every, on.mosaic_builder.relocate_ratio) == (4, 3, 500) and on.relocate_report().shape == (0, 8)
    rows = [list(lref.NOT_ATTEMPTED_ROW), [0, -36, 0, 0, 384, 2312, 195, 325], [4, 8, 4, 10, 5, 11, 5, 7]]
    on.mosaic_builder.relocate_outs.rows(0, 3, on.REPORT_CHUNK, "cpu")[0].copy_(torch.tensor(rows))
    on.mosaic_builder.relocate_outs.frames = 3
    assert on.relocate_report().tolist() == rows
    path = str(tmp_path / "r.csv")
    write_relocate_csv(path, [7, 8, 9], on.relocate_report())
    assert open(path).read().split("\n") == ["frame,status,shift_x,shift_y,sad,cells,sad2,cells2,eligible", "7,not_attempted,0,0,0,0,0,0,0",
                                              "8,relocated,-36,0,0,384,2312,195,325", "9,rejected_uniqueness,8,4,10,5,11,5,7", ""]
    with pytest.raises(ValueError, match="\\(2, 8\\)"):
        write_relocate_csv(path, [7, 8, 9], np.zeros((2, 8), np.int64))
    on.clear_report()
    assert on.relocate_report().shape == (0, 8)
    # the tool
    spec = importlib.util.spec_from_file_location("predict_video_tool_relocate", os.path.join(ROOT, "tools", "predict_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw = ["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights", "--mosaic", "m.png"]
    a = tool.parse_args(raw + ["--ortho", "o.png", "--mosaic-refine"])
    assert (a.mosaic_relocate, a.relocate_scale, a.relocate_every, a.relocate_min_overlap, a.relocate_max_mean, a.relocate_ratio, a.relocate_report) == (
        False, 8, 1, 0.5, 16, 0.8, None)
    a = tool.parse_args(raw + ["--ortho", "o.png", "--mosaic-refine", "--mosaic-relocate", "--relocate-scale", "16", "--relocate-every", "5", "--relocate-min-overlap", "0.25",
                               "--relocate-max-mean", "9", "--relocate-ratio", "0.7", "--relocate-report", "r.csv"])
    assert (a.mosaic_relocate, a.relocate_scale, a.relocate_every, a.relocate_min_overlap, a.relocate_max_mean, a.relocate_ratio, a.relocate_report) == (
        True, 16, 5, 0.25, 9, 0.7, "r.csv")
    capsys.readouterr()
    for bad, word in ((raw + ["--mosaic-relocate"], "need --ortho"), (raw + ["--ortho", "o.png", "--mosaic-relocate"], "need --mosaic-refine"),
                      (raw + ["--ortho", "o.png", "--mosaic-refine", "--relocate-scale", "4"], "need --mosaic-relocate"),
                      (raw + ["--ortho", "o.png", "--mosaic-refine", "--relocate-report", "r.csv"], "need --mosaic-relocate"),
                      (raw + ["--ortho", "o.png", "--mosaic-refine", "--mosaic-relocate", "--relocate-scale", "5"], "4, 8 or 16"),
                      (raw + ["--ortho", "o.png", "--mosaic-refine", "--mosaic-relocate", "--relocate-ratio", "2"], "0.001..1"),
                      (["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights", "--mosaic-relocate"], "need --ortho")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert word in capsys.readouterr().err, bad


# ------------------------------------------------------------------------------------------------ the definition end to end
def test_a_cut_onto_mapped_ground_is_recovered_to_the_exact_poses():
    """Ten 64 x 96 frames cut from a random texture, 4 px further right each; the pair of frame 10 is flagged as a scene cut and frames
    10..13 lie 40 px back (beyond the matcher's 32) on ground that frames 0..3 mapped, panning on.  Without relocation (the parent's
    behaviour) every frame from the cut on is lost.  With it (S = 4, the jump a whole number of cells, so the coarse SAD at the true
    shift is 0) the chain is relocalised at frame 10 and EVERY frame after the cut has its exact pose."""
    images, pairs, true = lref.revisit_after_cut()
    lost = lref.run_flight(images, pairs, rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN, relocate=False, **rref.FLIGHT_SETTINGS)
    assert lost[0][:lref.CUT_AT, 12].tolist() == [0] * lref.CUT_AT and lost[0][lref.CUT_AT:, 12].tolist() == [2] * 4
    assert (lost[2] == np.array(lref.NOT_ATTEMPTED_ROW)).all() and lost[3][24] == lref.LOST
    poses, outs, relocs, state, canvas = lref.run_flight(images, pairs, rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN, relocate=True, s=4, **rref.FLIGHT_SETTINGS)
    for f, (tx, ty) in enumerate(true):
        assert poses[f][:6].tolist() == [ONE, 0, tx * ONE, 0, ONE, ty * ONE] and poses[f][6:12].tolist() == [ONE, 0, -tx * ONE, 0, ONE, -ty * ONE], f
        assert poses[f][12] == 0, f
    assert relocs[:, 0].tolist() == [1] * lref.CUT_AT + [0, 1, 1, 1]
    assert relocs[lref.CUT_AT][1:5].tolist() == [-36, 0, 0, 24 * 16] and relocs[lref.CUT_AT][7] > 1        # 36 px back from the last pose, SAD 0 on all 384 cells
    assert state[24] == lref.TRACKING and np.array_equal(poses[:lref.CUT_AT], lost[0][:lref.CUT_AT])
    assert outs[lref.CUT_AT][0] == rref.NOT_TRACKING and (outs[lref.CUT_AT + 1:, 0] == rref.OK).all()       # the frame's own registration saw a lost chain
    # S = 8 finds the same frame (the jump is not a whole number of its cells: the fine registration absorbs the rest)
    again = lref.run_flight(images, pairs, rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN, relocate=True, s=8, **rref.FLIGHT_SETTINGS)
    print("S = 8:", again[2][lref.CUT_AT:].tolist(), [rref.translation_px(p) for p in again[0][lref.CUT_AT:]])


def test_a_cut_onto_unmapped_ground_stays_lost():
    images, pairs, _ = lref.unmapped_after_cut()
    lost = lref.run_flight(images, pairs, rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN, relocate=False, **rref.FLIGHT_SETTINGS)
    poses, outs, relocs, state, canvas = lref.run_flight(images, pairs, rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN, relocate=True, s=4, **rref.FLIGHT_SETTINGS)
    assert np.array_equal(poses, lost[0]) and np.array_equal(state, lost[3]) and poses[lref.CUT_AT:, 12].tolist() == [2] * 3
    assert np.array_equal(canvas[0], lost[4][0]) and np.array_equal(canvas[1], lost[4][1])                  # the same mosaic as the parent's
    assert set(relocs[lref.CUT_AT:, 0].tolist()) <= {lref.REJECTED_MEAN, lref.REJECTED_UNIQUENESS} and relocs[:lref.CUT_AT, 0].tolist() == [1] * lref.CUT_AT
    print("unmapped:", relocs[lref.CUT_AT:].tolist())
