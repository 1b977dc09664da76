"""Map-to-map registration and the merge of two mosaics, the parts that need no GPU: the definition in numpy (tests/merge_ref.py) in its
vectorised form against the literal loops; csrc/merge_defs.h run on the CPU by a stand-alone sanitized host program; the fourteenth hook
table and the freeze of the thirteenth; the library's refusals and the argument checks of the ops; and the end-to-end expectations shown
on the reference alone: a flight split in two is registered to the exact pose and merges into the single chain's planes byte for byte,
and a cut onto new ground that later pans back comes together with the coarse placement and stays apart without it."""
import ctypes
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import merge_ref as gref
import mosaic_ref as mref
import placement_rows
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow.predict import (FlowPredictor, merge_part, mosaic_part_arrays, part_seen_box, read_mosaic_part, write_merge_csv,
                                                           write_mosaic_part)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc")
NEW = ["merge_view", "merge_gate", "link_correct", "mosaic_merge", "merge_patch", "link_place"]
ONE = mref.ONE
OA, OB = gref.VIEW_ORIGIN_A, gref.VIEW_ORIGIN_B


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_vectorised_view_equals_the_loop():
    a, b = gref.view_canvases()
    seen = {}
    for name, link in gref.view_links():
        for window in gref.VIEW_WINDOWS:
            v, w = gref.merge_view(a, OA, b, OB, link, window), gref.merge_view_loop(a, OA, b, OB, link, window)
            assert all(np.array_equal(x, y) for x, y in zip(v, w)), (name, window)
            assert v[0].shape == ((96, 160) if window is None else window[2:]) and (v[1][v[3] == 0] == 0).all()
            seen[name] = int(v[3].sum())
            assert 0 < v[2].sum() < v[2].size                                   # A's holes show in valid_a whatever the link
    assert seen["outside"] == seen["no fit"] == seen["out of bounds"] == 0 and min(seen["identity"], seen["shift"], seen["rotation and zoom"]) > 1000
    # cur is the luma of whatever the word holds: the hole with colour bits under alpha 0 is not valid, and not black either
    cur, _, valid_a, _ = gref.merge_view(a, OA, b, OB, gref.view_links()[0][1])
    assert (valid_a[70:, :17] == 0).all() and cur[70:, :17].any() and (cur[10:23, 40:61] == 0).all()


def test_vectorised_gate_equals_the_loop():
    for name, table, va, vb, keep in gref.gate_cases():
        got = gref.merge_gate(table, va, vb)
        assert np.array_equal(got, gref.merge_gate_loop(table, va, vb)), name
        alive = [i for i in range(len(got)) if tuple(got[i]) != mref.VOID_ROW]
        if keep is not None:
            assert alive == keep, name
        else:
            assert 5 < len(alive) < len(got) and all(np.array_equal(got[i], table[i]) for i in alive), name


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("mode", ["centre", "latest"])
def test_vectorised_merge_equals_the_loop(k, mode):
    for name, link, merges in gref.merge_links():
        for offset in (0, 7, 0xFFFFFFFE - 25):
            va, oa, vb, ob = gref.merge_mosaics(k, mode=mode)
            v = (va.copy(), (oa[0].copy(), oa[1].copy()))
            w = (va.copy(), (oa[0].copy(), oa[1].copy()))
            cv = gref.mosaic_merge(v[0], gref.MERGE_ORIGIN_A, vb, gref.MERGE_ORIGIN_B, link, v[1], ob, offset, mode)
            cw = gref.mosaic_merge_loop(w[0], gref.MERGE_ORIGIN_A, vb, gref.MERGE_ORIGIN_B, link, w[1], ob, offset, mode)
            assert np.array_equal(cv, cw) and np.array_equal(v[0], w[0]) and np.array_equal(v[1][0], w[1][0]) and np.array_equal(v[1][1], w[1][1]), (name, offset)
            changed = not (np.array_equal(v[0], va) and np.array_equal(v[1][0], oa[0]) and np.array_equal(v[1][1], oa[1]))
            assert changed == (merges and name != "out of reach") and cv[0] == link[12], (name, offset)
            if name == "identity":
                assert cv[1] == 70 * 90 and 0 < cv[2] < cv[1] and cv[3] > cv[2] and (v[0] == 65535).sum() > (va == 65535).sum()      # both sides saturate
                assert 0 < cv[4] < cv[1]
                if offset > 7:                                                   # ordinals past 0xFFFFFFFE take nothing: every pixel taken carries one of B's first 26
                    took = v[1][0] != oa[0]
                    assert ((v[1][0][took] & np.uint64(0xFFFFFFFF)) >= np.uint64(offset)).all() and took.sum() == cv[4]
                # a second call: the votes again, the orthophoto unchanged
                r0, c0 = v[1][0].copy(), v[1][1].copy()
                again = gref.mosaic_merge(v[0], gref.MERGE_ORIGIN_A, vb, gref.MERGE_ORIGIN_B, link, v[1], ob, offset, mode)
                assert again[4] == 0 and again[3] == cv[3] and np.array_equal(v[1][0], r0) and np.array_equal(v[1][1], c0)
    # equal ranks: A keeps the pixel
    va, oa, vb, ob = gref.merge_mosaics(1, mode="centre")
    bx, by, exists = gref.b_pixels(gref.merge_links()[0][1], (0, 0) + gref.MERGE_A, gref.MERGE_ORIGIN_A, gref.MERGE_B, gref.MERGE_ORIGIN_B)
    Y, X = np.nonzero(exists)
    tie = (oa[0][Y, X] == ob[0][by[Y, X], bx[Y, X]]) & (oa[0][Y, X] != np.uint64(gref.EMPTY))
    assert tie.sum() > 3
    before = oa[1].copy()
    gref.mosaic_merge(va, gref.MERGE_ORIGIN_A, vb, gref.MERGE_ORIGIN_B, gref.merge_links()[0][1], oa, ob, 0, "centre")
    assert np.array_equal(oa[1][Y[tie], X[tie]], before[Y[tie], X[tie]])
    assert gref.shifted_rank(gref.EMPTY, 0, "centre") is None and gref.shifted_rank(5 << 32 | 0xFFFFFFFE, 1, "centre") is None
    assert gref.shifted_rank(5 << 32 | 0xFFFFFFFD, 1, "centre") == 5 << 32 | 0xFFFFFFFE and gref.shifted_rank(5 << 32 | 3, 4, "latest") == (0xFFFFFFFF - 7) << 32 | 7


@pytest.mark.parametrize("s", [4, 8])
def test_vectorised_patch_equals_the_loop_in_every_status(s):
    status = []
    for name, link, box, size_a, ob, want in gref.patch_links():
        b = gref.patch_canvas_b(name)
        v = gref.merge_patch(b, ob, link, size_a, OA, s, box)
        status.append(int(v[2][0]))
        assert v[2][0] == want, name
        if v[2][0] == 0 and v[2][3] * v[2][4] < 2000:
            w = gref.merge_patch_loop(b, ob, link, size_a, OA, s, box)
            assert all(np.array_equal(x, y) for x, y in zip(v, w)), name
            assert v[0].shape == (v[2][4], v[2][3]) and v[2][5] == v[1].sum() > 0 and (v[0][v[1] == 0] == 0).all(), name
    assert set(status) == {0, 1, 2, 3, 4}
    # the smaller box draws fewer cells than the whole canvas under the same link
    whole, part = (gref.merge_patch(gref.view_canvases()[1], OB, gref.patch_links()[1][1], gref.VIEW_A, OA, s, box)[2] for box in (None, (8, 16, 40, 81)))
    assert part[3] < whole[3] and part[4] < whole[4]


def test_the_steps_by_hand():
    seen = set()
    for name, model, link, status in gref.correct_cases():
        new, out = gref.correct_step(model, link, gref.CORRECT_WINDOW, gref.CORRECT_ORIGIN)
        seen.add(status)
        assert out[0] == status and out[1:6].tolist() == [model[13], model[14], model[15], model[2], model[5]], name
        if status == gref.OK:
            assert new[12] == 0 and new[13:].tolist() == [model[14], model[13], model[15]] and not np.array_equal(new[:12], link[:12]), name
        else:
            assert np.array_equal(new, link), name
    assert seen == {0, 2, 3, 4}
    at_edge = [c for c in gref.correct_cases() if c[0] == "exactly at the pose bound"][0]
    assert gref.correct_step(at_edge[1], at_edge[2], gref.CORRECT_WINDOW, gref.CORRECT_ORIGIN)[0][2] == (1 << 14) * ONE - 1
    # a whole-pixel shift fitted in a window away from the anchor is the same shift in anchor coordinates; a rotation is not
    shift = gref.correct_cases()[1]
    assert gref.correct_step(shift[1], shift[2], gref.CORRECT_WINDOW, gref.CORRECT_ORIGIN)[0][6:12].tolist() == [ONE, 0, 3 * ONE, 0, ONE, -2 * ONE]
    good, link = gref.correct_cases()[0][1:3]
    here, there = (gref.correct_step(good, link, w, gref.CORRECT_ORIGIN)[0] for w in (gref.CORRECT_WINDOW, (20, 30, 64, 96)))
    assert there[6:12].tolist() == mref.compose([int(v) for v in link[6:12]], [int(v) for v in good[0:6]]) and here[8] != there[8]
    codes = set()
    for name, found, link, max_mean, ratio, code in gref.place_cases():
        for s in (4, 16):
            cand, out = gref.place_step(found, link, s, max_mean, ratio)
            codes.add(code)
            assert out[0] == code, name
            if code == gref.PLACED:
                assert cand[12] == 1 and cand[13:].tolist() == [0, 0, 0] and cand[2] == link[2] + s * found[1] * ONE and cand[5] == link[5] + s * found[2] * ONE, name
                assert out[1:5].tolist() == [s * found[1], s * found[2], found[3], found[4]], name
            else:
                assert np.array_equal(cand, link), name
    assert codes == {0, 1, 2, 3, 4, 6, 7}


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def host_commands():
    """(commands, expected output lines) for tests/merge_host_check.cpp, from the numpy reference."""
    cmds, want = [], []

    def add(cmd, out):
        cmds.append(" ".join(str(int(v)) if not isinstance(v, str) else v for v in cmd))
        want.append(" ".join(str(int(v)) for v in out))

    flat = lambda a: [int(v) for v in np.asarray(a).reshape(-1)]  # noqa: E731
    halves = lambda r: [int(h) for v in np.asarray(r).reshape(-1) for h in (int(v) >> 32, int(v) & 0xFFFFFFFF)]  # noqa: E731
    a, b = gref.view_canvases()
    a, b = np.ascontiguousarray(a[:48, :80]), np.ascontiguousarray(b[:40, :64])
    for name, link in gref.view_links():
        for window in (None, (16, 32, 32, 48)):
            y0, x0, wh, ww = gref.whole_window(a.shape) if window is None else window
            add(["view", 48, 80, OA[1], OA[0], 40, 64, OB[1], OB[0], y0, x0, wh, ww] + flat(link) + flat(a) + flat(b),
                [v for p in gref.merge_view(a, OA, b, OB, link, window) for v in flat(p)])
    for name, table, va, vb, _ in gref.gate_cases():
        add(["gate", va.shape[0], va.shape[1]] + flat(table) + flat(va) + flat(vb), flat(gref.merge_gate(table, va, vb)))
    for name, model, link, _ in gref.correct_cases():
        for window, origin in ((gref.CORRECT_WINDOW, gref.CORRECT_ORIGIN), ((16368, 16368, 16, 16), (-16384, -16384))):    # s at its bound of 2^15
            new, out = gref.correct_step(model, link, window, origin)
            add(["correct", window[0], window[1], origin[1], origin[0]] + flat(model) + flat(link), flat(new) + flat(out))
    for k, mode, ortho in ((1, "centre", 1), (5, "latest", 1), (32, "centre", 0)):
        for name, link, _ in gref.merge_links():
            for offset in (3, 0xFFFFFFFE - 25):
                va, oa, vb, ob = gref.merge_mosaics(k, mode=mode)
                va, vb = np.ascontiguousarray(va[:, :40, :70]), np.ascontiguousarray(vb[:, :30, :50])
                oa, ob = tuple(np.ascontiguousarray(p[:40, :70]) for p in oa), tuple(np.ascontiguousarray(p[:30, :50]) for p in ob)
                head = ["merge", k, 40, 70, gref.MERGE_ORIGIN_A[1], gref.MERGE_ORIGIN_A[0], 30, 50, gref.MERGE_ORIGIN_B[1], gref.MERGE_ORIGIN_B[0], offset,
                        gref.oref.MODES[mode], ortho] + flat(link) + flat(va) + flat(vb) + ((halves(oa[0]) + flat(oa[1]) + halves(ob[0]) + flat(ob[1])) if ortho else [])
                counts = gref.mosaic_merge(va, gref.MERGE_ORIGIN_A, vb, gref.MERGE_ORIGIN_B, link, oa if ortho else None, ob if ortho else None, offset, mode)
                add(head, flat(counts) + flat(va) + ((halves(oa[0]) + flat(oa[1])) if ortho else []))
    for s in (4, 8, 16):
        for name, link, box, size_a, ob, _ in gref.patch_links():
            b = gref.patch_canvas_b(name)
            if s == 16 and name == "too many cells":
                continue                                                         # 60000 cells of 16 x 16: drawn, and nothing new
            y0, x0, y1, x1 = gref.whole_box(b.shape) if box is None else box
            geo = [y0, x0, y1, x1, ob[1], ob[0], size_a[0], size_a[1], OA[1], OA[0], s] + flat(link)
            add(["geometry"] + geo, gref.box_geometry(link, (y0, x0, y1, x1), ob, size_a, OA, s))
            tl, tv, geom = gref.merge_patch(b, ob, link, size_a, OA, s, box)
            add(["patch", b.shape[0], b.shape[1]] + geo + flat(b), flat(geom) + flat(tl) + flat(tv))
    far = gref.link_row(*mref.affine_pose(15.9, -15.9, 15.9, 15.9, -16383.9, 16383.9))                  # the corners' products at their bounds
    add(["geometry", 0, 0, 16384, 16384, 16384, -16384, 16384, 16384, -16384, 16384, 4] + flat(far),
        gref.box_geometry(far, (0, 0, 16384, 16384), (-16384, 16384), (16384, 16384), (16384, -16384), 4))
    for name, found, link, max_mean, ratio, _ in gref.place_cases():
        for s in (4, 16):
            cand, out = gref.place_step(found, link, s, max_mean, ratio)
            add(["place", s, max_mean, ratio] + flat(found) + flat(link), flat(cand) + flat(out))
    for name, link, box, size_a, s, status, cells in box_cases():
        geom = gref.box_geometry(link, box, OB, size_a, OA, s)
        assert geom[0] == status and (cells is None or tuple(geom[1:5]) == cells), (name, geom)          # the reference first: the case is what it says
        add(["geometry"] + list(box) + [OB[1], OB[0], size_a[0], size_a[1], OA[1], OA[0], s] + flat(link), geom)
    for name, found, (to, back), code in placement_rows.gate_rows():
        link, state = gref.link_row(to, back, status=gref.REGISTERED, tail=(7, 8, 9)), gref.lref.lost_state(to, back)
        for s in (4, 16):
            cand, out = gref.place_step(found, link, s, placement_rows.MAX_MEAN, placement_rows.RATIO)
            step = gref.lref.relocate_step(found, state, s=s, max_mean=placement_rows.MAX_MEAN, ratio=placement_rows.RATIO, **gref.lref.STEP_GEOMETRY)
            assert out[0] == code == step[0][28], name                                                    # one gate: pose_relocate draws the same code
            add(["place", s, placement_rows.MAX_MEAN, placement_rows.RATIO] + flat(found) + flat(link), flat(cand) + flat(out))
    return cmds, want


def box_cases():
    """(name, link, b_box, canvas A, S, status, (pu0, pv0, tw, th) or None) for merge_patch's geometry where a rule on the corners' box and
    a rule corner by corner could part.  Origins OA and OB; a b_box of 32 x 48 pixels of B turned by 30 degrees, so that each extremum
    comes from another corner, with the link's translation chosen in Q20 so that the box starts exactly on a pixel's edge of A, or a unit
    off it; a box exactly as wide as A's coarse canvas and one cell wider; and a link that flattens the box to no pixel."""
    (oya, oxa), (oyb, oxb), cases = OA, OB, []
    y0, x0, y1, x1 = box = (4, 8, 36, 56)
    shift = lambda tx, ty: gref.link_row([ONE, 0, tx * ONE, 0, ONE, ty * ONE], [ONE, 0, -tx * ONE, 0, ONE, -ty * ONE], status=gref.REGISTERED)  # noqa: E731
    # upright: B pixel x lands on A pixel x - oxb + tx + oxa; tx puts x0 on A's pixel 0
    tx, ty = oxb - oxa - x0, oyb - oya - y0 + 8
    cases.append(("as wide as the coarse canvas", shift(tx, ty), box, (64, 48), 4, 0, (0, 2, 12, 8)))    # x 0..48: cells 0..11 of 12
    cases.append(("one cell wider", shift(tx + 1, ty), box, (64, 48), 4, 4, None))                       # x 1..49: cells 0..12
    cases.append(("a box of no width", gref.link_row([0, 0, 5 * ONE, 0, ONE, 0], status=gref.REGISTERED), box, (64, 48), 4, 3, None))
    c, s = np.cos(np.radians(30)), np.sin(np.radians(30))
    lin = [int(round(v * ONE)) for v in (c, -s, s, c)]
    corners = [(x - oxb, y - oyb) for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
    xs, ys = [lin[0] * x + lin[1] * y for x, y in corners], [lin[2] * x + lin[3] * y for x, y in corners]
    assert len({xs.index(min(xs)), xs.index(max(xs)), ys.index(min(ys)), ys.index(max(ys))}) == 4
    wide, high = -(-(max(xs) - min(xs)) // ONE), -(-(max(ys) - min(ys)) // ONE)
    for d in (0, -1):                                                                                    # the box starts at A's pixel (40, 24), or a unit before it
        link = gref.link_row([lin[0], lin[1], 40 * ONE - min(xs) - oxa * ONE + d, lin[2], lin[3], 24 * ONE - min(ys) - oya * ONE + d], status=gref.REGISTERED)
        X0, Y0 = 40 + d, 24 + d
        cases.append((f"rotated, {d} units off the pixel's edge", link, box, (128, 192), 4, 0,
                      (X0 // 4, Y0 // 4, (40 + wide + 3) // 4 - X0 // 4, (24 + high + 3) // 4 - Y0 // 4)))
    return cases


def test_the_headers_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/merge_defs.h is plain __host__ __device__ C++: tests/merge_host_check.cpp runs the view, the gate, the correction (also with
    the window corner at its bound), the merge tile by tile as the kernel walks it (a tile that b_reaches refuses must hold no pixel of
    B), the patch cell by cell and the placement step in every status, as a stand-alone program built with -fsanitize=address,undefined;
    every line it prints is the reference's."""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "merge_host_check"), str(tmp_path / "commands.txt")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tests", "merge_host_check.cpp"), "-o", exe]
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
def test_the_fourteenth_table_and_the_freeze_of_the_thirteenth():
    assert _lib.ext13_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext13_api {"):text.index("} fs_ext13_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == NEW
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables12;") < text.index("typedef struct fs_ext13_api {") < text.index("typedef struct fs_hook_tables13 {")
    tables13 = text[text.index("typedef struct fs_hook_tables13 {"):text.index("} fs_hook_tables13;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables13) == [("fs_hook_tables12", "base12"), ("fs_ext13_api", "ext13")]
    assert int(re.search(r"#define FS_EXT13_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT13_MAGIC == int.from_bytes(b"FSEXTA13", "big")
    # fs_ext12_api is frozen: the header and the binding name the same five members, 56 bytes
    frozen = text[text.index("typedef struct fs_ext12_api {"):text.index("} fs_ext12_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", frozen) == _lib.ext12_hook_names() == ["map_coarse", "map_patch", "map_locate", "pose_relocate", "relocate_commit"]
    assert ctypes.sizeof(_lib.FsExt12Api) == 56
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables13 all13 = {all12, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT13_MAGIC," in init and "sizeof(fs_ext13_api)," in init
    assert re.search(r"const fs_hook_tables12& all12 = all13\.base12;\s+const fs_hook_tables11& all11 = all12\.base11;", src)
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    assert all("launch_" + name in kernels for name in NEW)
    # the thirteen older tables and the export list are what they were
    assert [len(names()) for names in (_lib.hook_names, _lib.ext_hook_names, _lib.ext2_hook_names, _lib.ext3_hook_names, _lib.ext4_hook_names, _lib.ext5_hook_names,
                                       _lib.ext6_hook_names, _lib.ext7_hook_names, _lib.ext8_hook_names, _lib.ext9_hook_names, _lib.ext10_hook_names,
                                       _lib.ext11_hook_names, _lib.ext12_hook_names)] == [38, 2, 14, 1, 1, 1, 1, 2, 4, 2, 3, 1, 5]
    assert not any("fs_" + name in _lib.exported_symbols() for name in NEW) and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    public = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(name in public for name in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables13.ext13.offset == ctypes.sizeof(_lib.FsHookTables12)                         # directly behind, no padding
    assert [getattr(_lib.FsExt13Api, name).offset for name in NEW] == [16, 24, 32, 40, 48, 56] and ctypes.sizeof(_lib.FsExt13Api) == 64
    all13 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables13)).contents
    assert all13.base12.ext12.magic == _lib.EXT12_MAGIC and all13.base12.ext12.size == 56                 # frozen: exactly, not from below
    assert all13.base12.base11.ext11.magic == _lib.EXT11_MAGIC and all13.base12.base11.ext11.size == 24
    assert all13.ext13.magic == _lib.EXT13_MAGIC and all13.ext13.size >= 64                               # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all13.ext13, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                                            # a table member, not an exported symbol
    assert ctypes.cast(all13.base12.ext12.map_locate, ctypes.c_void_p).value == ctypes.cast(lib.fs_map_locate, ctypes.c_void_p).value
    # the rules' header builds on the older ones: a rule two ops share is theirs, called from here; the kernels take their rules from it; no canvas takes an atomic
    defs = open(os.path.join(CSRC, "merge_defs.h")).read()
    assert '#include "relocate_defs.h"' in defs and all(f"mos::{fn}(" in defs for fn in ("source_pixel", "anchor_coord", "pose_in_bounds", "touches", "compose", "corner_box"))
    assert all(f"refn::{fn}(" in defs for fn in ("luma_of", "seen", "gate_keeps", "fit_report")) and "orth::rank_ordinal(" in defs
    assert all(f"relo::{fn}(" in defs for fn in ("box_cells", "placement_gate", "placement_report")) and "translate(" not in defs   # the move is the gate's
    assert defs.count("mos::source_pixel(") == 1                                                         # the one gather the ops share
    kernel = open(os.path.join(CSRC, "merge_ops.hip")).read()
    assert all(f"mrg::{fn}(" in kernel for fn in ("link_views", "link_merges", "gather_affine", "b_pixel", "b_reaches", "view_pixel", "correct_step", "shifted_rank",
                                                   "box_geometry", "patch_pixel", "place_step", "window_ok", "box_ok"))
    code = re.sub(r"//[^\n]*", "", kernel.split("namespace fs {")[1])
    assert "asm" not in code and "hipMemset" not in code
    atomics = re.findall(r"atomic\w*\(([^,]+),", code)
    assert atomics and all(a.strip().startswith(("&tally[", "counts +")) for a in atomics)                # the tally and counts only
    # the four headers it builds on are byte for byte what they became when the family's shared rules (the corners' box, the cells of a box,
    # the placement gate, the two report rows) were written once, in them (no git needed: a checkout may have none)
    for older, digest in (("mosaic_defs.h", "e691732e4314af07baa789dc7c3fb306ab002605536cd97ff10e48957de23d2c"),
                          ("ortho_defs.h", "7406b782e77f4778c32786c9a5363a3ff6adad4831944c0925d5b174de12a347"),
                          ("refine_defs.h", "d6167c7b09f800b4e9a07b3843c8992abd8300df18a2c1cbb0868d0d10829d45"),
                          ("relocate_defs.h", "a36b5c734d196339835b549aa37b4885f18e4bbe450006f56d677ee9eca984d8")):
        assert hashlib.sha256(open(os.path.join(CSRC, older), "rb").read().replace(b"\r\n", b"\n")).hexdigest() == digest, older   # whatever line endings a checkout made
    assert " merge_ops.hip " in open(os.path.join(CSRC, "Makefile")).read()


def test_the_magic_is_checked_before_use(monkeypatch):
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT13_MAGIC", _lib.EXT13_MAGIC + 1)
    with pytest.raises(RuntimeError, match="the library has no thirteenth extension table \\(fs_mosaic_merge is missing\\)"):
        fresh.fs_mosaic_merge
    assert fresh.fs_map_locate is not None                                    # the tables in front of it stay usable
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT12_MAGIC", _lib.EXT12_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first thirteen hook tables are not the ones this binding knows \\(fs_merge_view is missing\\)"):
        fresh.fs_merge_view
    monkeypatch.undo()
    assert all(getattr(fresh, "fs_" + name) is not None for name in NEW)


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    assert len(gref.refusal_cases()) >= 90
    for op, kw, word in gref.refusal_cases():
        assert gref.call_op(lib, op, **kw) != 0, (op, kw)
        msg = lib.fs_last_error()
        assert msg.startswith(op.encode() + b":") and word in msg, (op, kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
def test_ops_refuse_with_the_offending_value():
    rgba, small, link = torch.zeros((64, 96), dtype=torch.int32), torch.zeros((40, 48), dtype=torch.int32), torch.zeros((16,), dtype=torch.int64)
    good = dict(rgba_a=rgba, origin_a=(0, 0), rgba_b=small, origin_b=(3, 4), link=link)
    for kw, word in ((dict(window=(0, 0, 24, 32)), "(0, 0, 24, 32)"), (dict(window=(16, 0, 64, 32)), "(16, 0, 64, 32)"), (dict(window=(0, 0, 16)), "(0, 0, 16)"),
                     (dict(window=(0, -16, 16, 16)), "-16"), (dict(rgba_a=rgba.long()), "int64"), (dict(rgba_b=small[None]), "(1, 40, 48)"), (dict(link=link[:15]), "(15,)"),
                     (dict(link=link.int()), "int32"), (dict(origin_a=(20000, 0)), "20000"), (dict(origin_b=(0, -16385)), "-16385"), (dict(rgba_b=rgba), "same memory"),
                     (dict(rgba_a=torch.zeros((8, 96), dtype=torch.int32)), "(0, 0, 0, 96)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.merge_view(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.merge_view: tensors must live on the GPU"):
        ops.merge_view(**good)
    table, valid = torch.zeros((6, 7), dtype=torch.int32), torch.zeros((32, 48), dtype=torch.uint8)
    good = dict(table=table, valid_a=valid, valid_b=valid.clone())
    for kw, word in ((dict(table=table[:5]), "(5, 7)"), (dict(table=table.long()), "int64"), (dict(valid_b=valid[:16]), "(16, 48)"), (dict(valid_a=valid.int()), "int32"),
                     (dict(valid_a=valid[:8], valid_b=valid[:8]), "(8, 48)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.merge_gate(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.merge_gate: tensors must live on the GPU"):
        ops.merge_gate(**good)
    model = torch.zeros((16,), dtype=torch.int64)
    good = dict(model=model, link=link, window=(16, 32, 64, 96), origin_a=(5, 6))
    for kw, word in ((dict(model=model[:8]), "(8,)"), (dict(link=link.int()), "int32"), (dict(window=(16, 32, 60, 96)), "(16, 32, 60, 96)"), (dict(window=(16384, 0, 16, 16)), "16384"),
                     (dict(origin_a=(0, 16385)), "16385")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.link_correct(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.link_correct: tensors must live on the GPU"):
        ops.link_correct(**good)
    va, vb = torch.zeros((5, 64, 96), dtype=torch.int16).view(torch.uint16), torch.zeros((5, 40, 48), dtype=torch.int16).view(torch.uint16)
    oa, ob = (torch.zeros((64, 96), dtype=torch.int64), rgba), (torch.zeros((40, 48), dtype=torch.int64), small)
    good = dict(votes_a=va, origin_a=(0, 0), votes_b=vb, origin_b=(3, 4), link=link, ortho_a=oa, ortho_b=ob, ordinal_offset=3, mode="latest")
    for kw, word in ((dict(votes_b=vb[:4]), "5 and 4"), (dict(votes_a=va.view(torch.int16)), "int16"), (dict(mode="newest"), "'newest'"), (dict(ordinal_offset=0xFFFFFFFF), "4294967295"),
                     (dict(ordinal_offset=-1), "-1"), (dict(ortho_b=None), "go together"), (dict(ortho_a=(oa[0],)), "(rank, rgba)"), (dict(ortho_b=oa), "(64, 96)"),
                     (dict(votes_b=va, ortho_b=oa), "same memory"), (dict(link=link[:8]), "(8,)"), (dict(origin_b=(99999, 0)), "99999"),
                     (dict(ortho_a=(oa[0].int(), rgba)), "int32")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.mosaic_merge(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.mosaic_merge: tensors must live on the GPU"):
        ops.mosaic_merge(**good)
    assert "NOT IDEMPOTENT" in ops.mosaic_merge.__doc__ and "guesses, not validated on real video" in ops.register_mosaics.__doc__
    good = dict(rgba_b=small, origin_b=(3, 4), link=link, canvas_a=(64, 96), origin_a=(0, 0), scale=4)
    for kw, word in ((dict(scale=5), "5"), (dict(b_box=(0, 0, 41, 48)), "(0, 0, 41, 48)"), (dict(b_box=(8, 8, 8, 20)), "(8, 8, 8, 20)"), (dict(canvas_a=(0, 96)), "(0, 96)"),
                     (dict(canvas_a=(15, 96), scale=16), "no cell"), (dict(rgba_b=small.long()), "int64"), (dict(link=link[:3]), "(3,)"), (dict(origin_a=(0, 16385)), "16385")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.merge_patch(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.merge_patch: tensors must live on the GPU"):
        ops.merge_patch(**good)
    good = dict(found=link.clone(), link=link, scale=8)
    for kw, word in ((dict(scale=2), "2"), (dict(max_mean=256), "256"), (dict(ratio_permille=0), "got 0"), (dict(found=link[:15]), "(15,)"), (dict(link=link.int()), "int32")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.link_place(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.link_place: tensors must live on the GPU"):
        ops.link_place(**good)
    good = dict(a=(rgba, (0, 0)), b=(small, (3, 4)), link=link)
    for kw, word in ((dict(rounds=0), "got 0"), (dict(rounds=9), "got 9"), (dict(search=33), "got 33"), (dict(a=rgba), "Tensor"), (dict(place=dict(exclude=2)), "exclude"),
                     (dict(place=dict(scale=4, radius=1)), "radius"), (dict(window=(0, 0, 64, 100)), "(0, 0, 64, 100)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.register_mosaics(**{**good, **kw})
    with pytest.raises(ValueError, match="six Q20 integers"):
        ops.mosaic_link(b_to_a=[1, 2, 3])
    with pytest.raises(ValueError, match="got 4"):
        ops.mosaic_link(status=4)
    assert ops.mosaic_link().tolist() == [ONE, 0, 0, 0, ONE, 0] * 2 + [1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the definition end to end
@pytest.mark.parametrize("mode", ["centre", "latest"])
def test_a_split_flight_registers_exactly_and_merges_into_the_single_chains_planes(mode):
    """Six 64 x 96 frames 4 px apart, split after frame 3: both halves mosaicked on their own, B registered against A from the default
    initial link (A's tail, status 1: one step short of the truth), then merged with ordinal_offset = 3.  (b) the recovered b_to_a is
    frame 3's exact pose; (c) votes, rank and rgba equal the single chain's byte for byte."""
    whole, a, b, link, true = gref.split_flight(mode)
    assert link[12] == 1 and link[2] == true[2] - 4 * ONE
    merged, link, outs, counts = gref.merge_parts(a, b, link, mode)
    assert link[:6].tolist() == true and link[6:12].tolist() == [ONE, 0, -true[2], 0, ONE, 0] and link[12] == 0
    assert outs[:, 0].tolist() == [0, 0] and outs[0, 4:6].tolist() == [-4 * ONE, 0] and outs[1, 4:6].tolist() == [0, 0] and outs[0, 2] >= 12
    for plane in ("votes", "rank", "rgba"):
        assert np.array_equal(merged[plane], whole[plane]), plane
        assert not np.array_equal(a[plane], whole[plane]), plane
    assert counts[0] == 0 and counts[1] == 128 * 180 and counts[2] == 64 * 104 and counts[3] == 3 * 64 * 96 and 0 < counts[4] <= counts[2]
    # the multi-rank bookkeeping: the merged tail is compose(b_to_a, B's tail), the last frame's exact pose
    tail = mref.compose([int(v) for v in link[:6]], [int(v) for v in b["tail"][:6]])
    assert tail == [int(v) for v in whole["tail"][:6]] == [ONE, 0, 20 * ONE, 0, ONE, 0]


def test_a_cut_onto_new_ground_comes_together_with_the_placement_only():
    a, b, link, true, box = gref.cut_parts()
    apart, kept, outs, counts = gref.merge_parts(a, b, link, "centre")
    assert outs[:, 0].tolist() == [2, 2] and np.array_equal(kept, link) and counts.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert all(np.array_equal(apart[p], a[p]) for p in ("votes", "rank", "rgba"))
    for s in (4, 8):
        merged, placed, outs, counts = gref.merge_parts(a, b, link, "centre", place=dict(scale=s, b_box=box))
        assert outs[0, :4].tolist() == [0, 24, 0, 0] and outs[0, 4] >= 72 and outs[1:, 0].tolist() == [0, 0], s
        assert placed[:6].tolist() == true and placed[12] == 0 and counts[0] == 0 and counts[2] == 64 * 104 and counts[4] > 0, s
        assert (merged["votes"].sum(0) > 0).sum() > (a["votes"].sum(0) > 0).sum()


# ------------------------------------------------------------------------------------------------ part files, the predictor's checks, the CSV
def cpu_part(p, mode="centre"):
    """One of merge_ref's parts as FlowPredictor.mosaic_part() hands it out, on the CPU."""
    t = torch.from_numpy
    return dict(votes=t(p["votes"].copy()), rank=t(p["rank"].view(np.int64).copy()), rgba=t(p["rgba"].view(np.int32).copy()), state=t(p["state"].copy()),
                poses=t(p["poses"].copy()), tail=t(p["tail"].copy()), origin=gref.SPLIT_ORIGIN, mask_size=(64, 96), frames=p["frames"], mode=mode)


def test_a_part_file_round_trips_and_carries_the_seen_box(tmp_path):
    _, b, _, _, box = gref.cut_parts()
    part = cpu_part(b)
    path = str(tmp_path / "b.part000.npz")
    write_mosaic_part(path, part)
    assert os.path.exists(path) and os.path.getsize(path) < 1 << 20
    back = read_mosaic_part(path, "cpu")
    for k in ("votes", "rank", "rgba", "state", "poses", "tail"):
        assert back[k].dtype == part[k].dtype and torch.equal(back[k], part[k]), k
    assert (back["origin"], back["mask_size"], back["frames"], back["mode"]) == (gref.SPLIT_ORIGIN, (64, 96), 3, "centre")
    assert back["box"] == box == part_seen_box(b["poses"], (64, 96), gref.SPLIT_CANVAS, gref.SPLIT_ORIGIN)         # what the frames saw, from the pose rows
    seen = (b["rgba"] >> 24) != 0
    ys, xs = np.nonzero(seen)
    assert box == (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    lost = b["poses"].copy()
    lost[:, 12] = 2
    assert part_seen_box(lost, (64, 96), gref.SPLIT_CANVAS, gref.SPLIT_ORIGIN) == (0, 0) + gref.SPLIT_CANVAS      # nothing voted: the whole canvas
    votes_only = dict(part, rank=None, rgba=None, mode=None)
    write_mosaic_part(path, votes_only)
    back = read_mosaic_part(path, "cpu")
    assert back["rank"] is None and back["rgba"] is None and back["mode"] is None and torch.equal(back["votes"], part["votes"])
    with pytest.raises(ValueError, match="int16"):
        mosaic_part_arrays(dict(part, votes=part["votes"].view(torch.int16)))
    np.savez(str(tmp_path / "other.npz"), votes=b["votes"])
    with pytest.raises(ValueError, match="is no mosaic part"):
        read_mosaic_part(str(tmp_path / "other.npz"), "cpu")


def test_predictor_checks_and_the_merge_csv(tmp_path):
    pred = FlowPredictor(torch.nn.Identity(), mosaic=(30, 40), ortho="centre")
    with pytest.raises(ValueError, match="mosaic_part\\(\\) needs mosaic="):
        pred.mosaic_part()
    with pytest.raises(ValueError, match="merge_mosaic\\(\\) needs mosaic= and ortho="):
        pred.merge_mosaic(cpu_part(gref.cut_parts()[1]))
    links, outs, counts = pred.merge_report()
    assert links.shape == (0, 16) and outs == [] and counts.shape == (0, 8)
    a, b, link, _, box = gref.cut_parts()
    _, placed, rows, count = gref.merge_parts(a, b, link, "centre", place=dict(scale=4, b_box=box))
    path = str(tmp_path / "m.csv")
    write_merge_csv(path, ["b.part001.npz", "c"], (np.stack([placed, link]), [rows, rows[1:]], np.stack([count, [1, 0, 0, 0, 0, 0, 0, 0]])))
    assert open(path).read().split("\n") == ["part,link,m00,m01,m02,m10,m11,m12,inliers,usable,register,reached,voted,votes,taken",
                                              "b.part001.npz,registered,1.000000,0.000000,36.000000,0.000000,1.000000,0.000000,16,16,0/0/0,19968,6656,18432,4096",
                                              "c,initial,1.000000,0.000000,12.000000,0.000000,1.000000,0.000000,0,0,0/0,0,0,0,0", ""]
    with pytest.raises(ValueError, match="1 names for 2 links"):
        write_merge_csv(path, ["x"], (np.stack([placed, link]), [rows, rows], np.stack([count, count])))


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name.replace(".py", "_tool_merge"), os.path.join(ROOT, "tools", name))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_argument_checks(capsys):
    merge = load_tool("merge_mosaics.py")
    a = merge.parse_args(["a.npz", "b.npz", "c.npz", "--out", "m.png", "--ortho", "o.png", "--report", "r.csv", "--search-scale", "8"])
    assert (a.parts, a.out, a.ortho, a.report, a.search_scale) == (["a.npz", "b.npz", "c.npz"], "m.png", "o.png", "r.csv", 8)
    assert merge.parse_args(["a.npz", "b.npz", "--out", "m.png"]).search_scale is None
    capsys.readouterr()
    for bad, word in ((["a.npz", "--out", "m.png"], "at least two parts"), (["a.npz", "b.npz"], "--out"), (["a.npz", "b.npz", "--out", "m.png", "--search-scale", "5"], "4, 8 or 16")):
        with pytest.raises(SystemExit):
            merge.parse_args(bad)
        assert word in capsys.readouterr().err, bad
    video = load_tool("predict_video.py")
    raw = ["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights"]
    assert video.parse_args(raw + ["--mosaic", "m.png", "--ortho", "o.png", "--mosaic-part", "p.npz"]).mosaic_part == "p.npz"
    assert video.parse_args(raw + ["--mosaic", "m.png"]).mosaic_part is None
    capsys.readouterr()
    for bad in (raw + ["--mosaic-part", "p.npz"], raw + ["--mosaic", "m.png", "--mosaic-part", "p.npz"]):
        with pytest.raises(SystemExit):
            video.parse_args(bad)
        assert "--mosaic-part needs --mosaic FILE.png and --ortho FILE.png" in capsys.readouterr().err, bad


def test_a_multi_rank_launch_names_its_parts_and_needs_the_orthophoto(capsys):
    video = load_tool("predict_video.py")
    raw = ["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights"]
    assert [video.mosaic_part_path("out/flood.png", r) for r in (0, 7, 123)] == ["out/flood.part000.npz", "out/flood.part007.npz", "out/flood.part123.npz"]
    assert video.mosaic_part_path("m", 1) == "m.part001.npz"
    both, alone, none = (video.parse_args(raw + extra) for extra in (["--mosaic", "m.png", "--ortho", "o.png", "--mosaic-report", "r.csv"], ["--mosaic", "m.png"], []))
    for args, world in ((both, 1), (both, 4), (alone, 1), (none, 1), (none, 8)):
        video.check_multi_rank_mosaic(args, world)                                 # nothing to refuse
    with pytest.raises(SystemExit, match="--mosaic under a multi-rank launch needs --ortho FILE.png"):
        video.check_multi_rank_mosaic(alone, 2)
    paths = [video.mosaic_part_path(both.mosaic, r) for r in range(3)]
    assert video.merge_command(both, paths) == "python tools/merge_mosaics.py m.part000.npz m.part001.npz m.part002.npz --out m.png --ortho o.png --report r.merge.csv"
    assert video.merge_command(alone, paths[:2]) == "python tools/merge_mosaics.py m.part000.npz m.part001.npz --out m.png"
    merge = load_tool("merge_mosaics.py")                                          # the command line it prints is one the merge tool takes
    a = merge.parse_args(video.merge_command(both, paths).split()[2:])
    assert (a.parts, a.out, a.ortho, a.report) == (paths, "m.png", "o.png", "r.merge.csv")
    source = open(os.path.join(ROOT, "tools", "predict_video.py")).read()
    assert "merging the ranks' mosaics is out of scope" not in source and "merge_rank_parts(pred, args, blocks)" in source


def test_merge_part_refuses_two_modes_and_two_mask_sizes_before_anything_runs():
    a, b, _, _, _ = gref.cut_parts()
    mine, part = cpu_part(a), cpu_part(b)
    before = mine["votes"].clone()
    for change, word in ((dict(mode="latest"), "'centre' and 'latest'"), (dict(mode=None), "'centre' and None"), (dict(mask_size=(64, 80)), "(64, 96) and (64, 80)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            merge_part(mine, dict(part, **change))
    with pytest.raises(ValueError, match=re.escape("None and None")):
        merge_part(dict(mine, mode=None), dict(part, mode=None))
    assert torch.equal(mine["votes"], before) and mine["frames"] == a["frames"]
