"""The change map between two registered mosaics, the parts that need no GPU: the definition in numpy (tests/change_ref.py) in its
vectorised form against the literal loops; csrc/change_defs.h run on the CPU by a stand-alone sanitized host program; the fifteenth hook
table and the freeze of the fourteenth; the library's refusals and the argument checks of the Python layers; and the properties of the
definition shown on the reference alone: a shift of at most r pixels changes nothing, a larger one does, new water far from old water
keeps every pixel, and the degenerate parameters are a plain comparison of two resolved class planes."""
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

import change_ref as cref
import merge_ref as gref
import mosaic_ref as mref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import predict
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc")
NEW = ["mosaic_change"]
OA, OB = cref.VIEW_ORIGIN_A, cref.VIEW_ORIGIN_B
WATER = cref.class_set((1,))


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("case", [c for c in cref.op_cases() if c[0] in ("K1 r1", "K5 r0", "K5 r3", "K32 r1", "small A", "small B")], ids=lambda c: c[0])
def test_vectorised_change_equals_the_loop(case):
    name, k, size_a, size_b, r, (min_votes, min_conf), watch = case
    va, vb = cref.case_inputs(k, size_a, size_b)
    va, vb = np.ascontiguousarray(va[:, :40, :70]), np.ascontiguousarray(vb[:, :33, :66])
    codes = set()
    for lname, link, merges in cref.change_links():
        v = cref.mosaic_change(va, OA, vb, OB, link, min_votes, min_conf, r, watch)
        w = cref.mosaic_change_loop(va, OA, vb, OB, link, min_votes, min_conf, r, watch)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(v, w)), (name, lname)
        codes |= set(np.unique(v[0]).tolist())
        assert v[4][0] == link[12] and v[4][2] == v[4][3:].sum() == v[3][0].sum() and v[4][5:].sum() == v[3][1].sum(), (name, lname)
        if not merges or lname == "outside":
            assert not v[0].any() and not v[3].any() and v[4][1:].sum() == 0 and (v[2] == 255).all(), (name, lname)
    assert {0, 1} <= codes and (codes == {0, 1} if k == 1 else 3 in codes and codes & {4, 5}) and (r > 0 or 2 not in codes), (name, codes)


def test_the_cases_hold_what_they_promise():
    """change_votes: pixels without a vote, cells at 65535, ties at the top and below, totals at and below min_votes = 3, shares at and
    below min_conf = 170; the thresholds move exactly those pixels."""
    v = cref.change_votes(5, cref.VIEW_A, 3).astype(np.int64)
    total, most = v.sum(0), v.max(0)
    conf = (255 * most + total // 2) // np.maximum(total, 1)
    ties = (v == most[None]).sum(0) > 1
    assert (total == 0).sum() > 500 and (v == 65535).sum() > 200 and (ties & (most == 65535)).sum() > 100 and (ties & (most == 9)).sum() > 300
    assert (total == 3).sum() > 300 and (total == 2).sum() > 300 and ((conf == 170) & (total == 3)).sum() > 200 and (conf == 169).sum() > 200
    loose, strict = cref.decided(v.astype(np.uint16), 1, 0), cref.decided(v.astype(np.uint16), 3, 170)
    assert ((loose == 255) == (total == 0)).all()
    assert ((strict == 255) == ((total < 3) | (conf < 170))).all() and (strict[(conf == 170) & (total == 3)] != 255).all() and (strict[conf == 169] == 255).all()
    tie = ties & (total > 0)
    assert (loose[tie] == v.argmax(0)[tie]).all() and (v[loose[tie], np.nonzero(tie)[0], np.nonzero(tie)[1]] == most[tie]).all()   # the lowest id of a tie
    assert [c[1:] for c in cref.op_cases()].count((5, cref.VIEW_A, cref.VIEW_B, 8, cref.THRESHOLDS[1], (4,))) == 1


# ------------------------------------------------------------------------------------------------ the properties of the definition
def shifted(plane, d):
    """B's class plane: A's moved by d = (dx, dy) pixels, 255 where nothing moves in."""
    out = np.full_like(plane, 255)
    (dx, dy), (h, w) = d, plane.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = plane[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def inside(plane, margin):
    return plane[margin:plane.shape[0] - margin, margin:plane.shape[1] - margin] if margin else plane


@pytest.mark.parametrize("r", [1, 3, 8])
def test_a_shift_of_at_most_r_changes_nothing(r):
    a = cref.block_classes(cref.VIEW_A)
    for d in ((1, 0), (0, -1), (r, 0), (-r, r), (r, -r), (r // 2 + 1, -r)):
        m = max(abs(d[0]), abs(d[1]))
        code = cref.change_codes(a, shifted(a, d), r, WATER)
        assert (inside(code, m) <= cref.EXPLAINED).all() and (inside(code, m) >= cref.SAME).all(), (r, d)
        assert (code == cref.EXPLAINED).sum() > 500, (r, d)


@pytest.mark.parametrize("r, d", [(0, (1, 0)), (0, (0, -1)), (1, (2, 0)), (3, (4, 0)), (3, (0, -4)), (8, (9, 0))])
def test_a_shift_beyond_r_changes_pixels(r, d):
    a = cref.block_classes(cref.VIEW_A)
    code = inside(cref.change_codes(a, shifted(a, d), r, WATER), max(abs(d[0]), abs(d[1])))
    assert (code >= cref.CHANGED).sum() > 300 and {cref.GAINED, cref.LOST} <= set(np.unique(code).tolist())
    if r == 0:
        assert not (code == cref.EXPLAINED).any()


@pytest.mark.parametrize("r", [0, 3])
def test_new_water_far_from_old_keeps_every_pixel(r):
    a = cref.block_classes(cref.VIEW_A)
    b = a.copy()
    box = (slice(26, 33), slice(44, 59))                         # 7 x 15 pixels inside the block rows 24..35, columns 40..59: class 0
    assert (a[box] == 0).all()
    far = a[box[0].start - r - 1:box[0].stop + r + 1, box[1].start - r - 1:box[1].stop + r + 1]
    assert not (far == 1).any()                                  # farther than r from any water of A
    b[box] = 1
    code = cref.change_codes(a, b, r, WATER)
    assert (code[box] == cref.GAINED).all() and (code == cref.GAINED).sum() == 7 * 15 and ((code == cref.SAME) | (code == cref.GAINED)).all()
    back = cref.change_codes(b, a, r, WATER)                     # the other way round it recedes
    assert (back[box] == cref.LOST).all() and (back == cref.LOST).sum() == 7 * 15
    # a ring of water two pixels wide around water that A holds already: the stated price of the tolerance
    near = a.copy()
    ys, xs = np.nonzero(a == 1)
    grown = np.zeros(a.shape, bool)
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            grown[np.clip(ys + dy, 0, a.shape[0] - 1), np.clip(xs + dx, 0, a.shape[1] - 1)] = True
    near[grown] = 1
    ring = cref.change_codes(a, near, r, WATER)
    if r == 0:
        assert (ring == cref.GAINED).sum() == (near != a).sum() and not (ring == cref.EXPLAINED).any()
    else:
        assert 0 < (ring == cref.EXPLAINED).sum() and (ring == cref.GAINED).sum() < (near != a).sum() // 2     # partly swallowed


def test_degenerate_parameters_are_a_plain_comparison():
    va, vb = cref.case_inputs(5, cref.VIEW_A, cref.VIEW_B)
    name, link, _ = cref.change_links()[1]
    change, cls_a, cls_b, transitions, counts = cref.mosaic_change(va, OA, vb, OB, link, 1, 0, 0, (1,))
    ra, rb = mref.mosaic_resolve(va)[0], mref.mosaic_resolve(vb)[0]
    assert np.array_equal(cls_a, ra)
    bx, by, exists = gref.b_pixels(link, (0, 0) + cref.VIEW_A, OA, cref.VIEW_B, OB)
    under = np.where(exists, rb[np.clip(by, 0, cref.VIEW_B[0] - 1), np.clip(bx, 0, cref.VIEW_B[1] - 1)], 255)
    assert np.array_equal(cls_b, under) and counts[1] == exists.sum()
    both = (ra != 255) & (under != 255)
    assert np.array_equal(change != 0, both) and np.array_equal(change == 1, both & (ra == under)) and not (change == 2).any()
    assert np.array_equal(change == 4, both & (ra != 1) & (under == 1)) and np.array_equal(change == 5, both & (ra == 1) & (under != 1))
    for status, broken in ((1, None), (2, None), (3, None), (0, [16 * mref.ONE, 0, 0, 0, mref.ONE, 0])):
        bad = link.copy()
        bad[12] = status
        if broken:
            bad[0:6] = broken
        out = cref.mosaic_change(va, OA, vb, OB, bad, 1, 0, 0, (1,))
        assert not out[0].any() and not out[3].any() and out[4].tolist() == [status, 0, 0, 0, 0, 0, 0, 0] and (out[2] == 255).all() and np.array_equal(out[1], ra)


def test_two_flights_on_the_reference():
    """The end-to-end expectation, reference first: flight B registers against flight A from a link 3 px off to the exact pose; code 4
    covers exactly the painted ground; with the link one pixel off and no registration, tolerance 0 lights up the class boundaries
    and tolerance 1 leaves the painted block alone."""
    a, b, exact, (y0, x0, y1, x1) = cref.two_flights()
    ground = cref.ground_classes()
    py0, px0, py1, px1 = cref.PAINT
    assert not (ground[py0 - 3:py1 + 3, px0 - 3:px1 + 3] == cref.PAINT_CLASS).any()              # farther than the tolerances used from any water of A
    (change, cls_a, cls_b, transitions, counts), link, outs = cref.flights_change(a, b, cref.off_link(-3))
    assert np.array_equal(link[:13], exact[:13]) and outs[:, 0].tolist() == [0, 0] and outs[0, 4:6].tolist() == [-3 * mref.ONE, 0]
    painted = np.zeros(change.shape, bool)
    painted[y0:y1, x0:x1] = True
    assert np.array_equal(change == cref.GAINED, painted) and not (change == cref.LOST).any() and not (change == cref.CHANGED).any()
    assert transitions[1].sum() == transitions[1, 0, cref.PAINT_CLASS] == 7 * 15 == counts[6]
    assert counts[0] == 0 and counts[1] == 128 * 180 and counts[2] == 64 * 104 == counts[3:].sum() == transitions[0].sum()   # the overlap: ground columns 76..180
    (c0, *_, n0), _, _ = cref.flights_change(a, b, cref.off_link(1, status=0), register=False, tolerance=0)
    (c1, *_, n1), _, _ = cref.flights_change(a, b, cref.off_link(1, status=0), register=False, tolerance=1)
    assert n0[5] > 50 and n0[7] > 30 and n0[6] > 7 * 15                                          # every class boundary is "change"
    assert n1[5] == n1[7] == 0 and n1[6] == 7 * 15 and n1[4] > 100 and (c1 == cref.GAINED).sum() == 7 * 15
    assert np.array_equal(np.argwhere(c1 == cref.GAINED).min(0), [y0, x0 + 1]) and np.array_equal(np.argwhere(c1 == cref.GAINED).max(0), [y1 - 1, x1])   # where the link puts it
    (_, _, _, t2, n2), _, _ = cref.flights_change(a, b, cref.off_link(1, status=1), register=False)   # an unconfirmed link compares nothing
    assert n2.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and not t2.any()


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def host_commands():
    """(commands, expected output lines) for tests/change_host_check.cpp, from the numpy reference."""
    cmds, want = [], []
    flat = lambda a: [int(v) for v in np.asarray(a).reshape(-1)]  # noqa: E731
    for name, k, size_a, size_b, r, (min_votes, min_conf), watch in cref.op_cases():
        va, vb = cref.case_inputs(k, size_a, size_b)
        va, vb = np.ascontiguousarray(va[:, :40, :150]), np.ascontiguousarray(vb[:, :33, :66])     # three tiles a row, the last of 22 columns
        for lname, link, _ in cref.change_links():
            if k == 32 and lname not in ("shift", "no fit") or k == 1 and lname == "rotation and zoom":
                continue                                                                        # the same walk, more classes to print
            head = ["change", k, va.shape[1], va.shape[2], OA[1], OA[0], vb.shape[1], vb.shape[2], OB[1], OB[0], min_votes, min_conf, r, cref.class_set(watch)]
            cmds.append(" ".join(str(v) for v in head + flat(link) + flat(va) + flat(vb)))
            change, cls_a, cls_b, transitions, counts = cref.mosaic_change(va, OA, vb, OB, link, min_votes, min_conf, r, watch)
            want.append(" ".join(str(v) for v in flat(counts) + flat(transitions) + flat(change) + flat(cls_a) + flat(cls_b)))
    return cmds, want


def test_the_headers_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/change_defs.h is plain __host__ __device__ C++: tests/change_host_check.cpp walks the planes tile by tile as the kernels do (a
    tile that b_reaches refuses must hold no pixel of B; the apron is clipped at the canvas edge; no tally cell exceeds a tile), as a
    stand-alone program built with -fsanitize=address,undefined; every line it prints is the reference's."""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "change_host_check"), str(tmp_path / "commands.txt")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tests", "change_host_check.cpp"), "-o", exe]
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
    assert len(got) == len(want) and len(want) > 60
    for cmd, g, w in zip(cmds, got, want):
        assert g == w, (cmd[:200], g[:200], w[:200])


# ------------------------------------------------------------------------------------------------ library surface
def test_the_fifteenth_table_and_the_freeze_of_the_fourteenth():
    assert _lib.ext14_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext14_api {"):text.index("} fs_ext14_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == NEW
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables13;") < text.index("typedef struct fs_ext14_api {") < text.index("typedef struct fs_hook_tables14 {")
    tables14 = text[text.index("typedef struct fs_hook_tables14 {"):text.index("} fs_hook_tables14;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables14) == [("fs_hook_tables13", "base13"), ("fs_ext14_api", "ext14")]
    assert int(re.search(r"#define FS_EXT14_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT14_MAGIC == int.from_bytes(b"FSEXTA14", "big")
    # fs_ext13_api is frozen: the header and the binding name the same six members, 64 bytes
    frozen = text[text.index("typedef struct fs_ext13_api {"):text.index("} fs_ext13_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", frozen) == _lib.ext13_hook_names() == ["merge_view", "merge_gate", "link_correct", "mosaic_merge", "merge_patch", "link_place"]
    assert ctypes.sizeof(_lib.FsExt13Api) == 64
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables14 all14 = {all13, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT14_MAGIC," in init and "sizeof(fs_ext14_api)," in init
    assert re.search(r"const fs_hook_tables13& all13 = all14\.base13;\s+const fs_hook_tables12& all12 = all13\.base12;", src)
    assert "launch_mosaic_change" in open(os.path.join(CSRC, "kernels.h")).read()
    # the fourteen older tables and the export list are what they were
    assert [len(names()) for names in (_lib.hook_names, _lib.ext_hook_names, _lib.ext2_hook_names, _lib.ext3_hook_names, _lib.ext4_hook_names, _lib.ext5_hook_names,
                                       _lib.ext6_hook_names, _lib.ext7_hook_names, _lib.ext8_hook_names, _lib.ext9_hook_names, _lib.ext10_hook_names,
                                       _lib.ext11_hook_names, _lib.ext12_hook_names, _lib.ext13_hook_names)] == [38, 2, 14, 1, 1, 1, 1, 2, 4, 2, 3, 1, 5, 6]
    assert not any("fs_" + name in _lib.exported_symbols() for name in NEW) and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    public = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(name in public for name in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables14.ext14.offset == ctypes.sizeof(_lib.FsHookTables13)                         # directly behind, no padding
    assert [getattr(_lib.FsExt14Api, name).offset for name in NEW] == [16] and ctypes.sizeof(_lib.FsExt14Api) == 24
    all14 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables14)).contents
    assert all14.base13.ext13.magic == _lib.EXT13_MAGIC and all14.base13.ext13.size == 64                 # frozen: exactly, not from below
    assert all14.base13.base12.ext12.magic == _lib.EXT12_MAGIC and all14.base13.base12.ext12.size == 56
    assert all14.ext14.magic == _lib.EXT14_MAGIC and all14.ext14.size >= 24                               # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all14.ext14, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                                            # a table member, not an exported symbol
    assert ctypes.cast(all14.base13.ext13.mosaic_merge, ctypes.c_void_p).value == ctypes.cast(lib.fs_mosaic_merge, ctypes.c_void_p).value


def test_the_rules_sit_on_the_merge_header_and_the_kernels_take_them_from_there():
    # merge_defs.h is byte for byte what it was before this op (no git needed: a checkout may have none)
    merge = open(os.path.join(CSRC, "merge_defs.h"), "rb").read().replace(b"\r\n", b"\n")                 # whatever line endings a checkout made
    assert hashlib.sha256(merge).hexdigest() == "528e2053abeb4122d9c1dedde067412e93097f9474eec7d5c073d5be9eedbdc2"
    defs = open(os.path.join(CSRC, "change_defs.h")).read()
    assert '#include "merge_defs.h"' in defs and "mos::source_pixel(" not in defs and "mos::vote_confidence(" in defs   # the gather is called, not restated
    assert "hip" not in re.sub(r"//[^\n]*", "", defs).lower()
    kernel = open(os.path.join(CSRC, "change_ops.hip")).read()
    assert all(f"mrg::{fn}(" in kernel for fn in ("link_merges", "gather_affine", "b_pixel", "b_reaches"))
    assert all(f"chg::{fn}(" in kernel for fn in ("take_votes", "decided_class", "staged_bit", "span_or", "change_code", "transition_cell", "tally_cells", "watch_ok"))
    code = re.sub(r"//[^\n]*", "", kernel.split("namespace fs {")[1])
    assert "asm" not in code and "hipMemset" not in code
    atomics = re.findall(r"atomic\w*\(([^,]+),", code)
    assert len(atomics) >= 6 and all(a.strip().startswith(("&tally[", "counts +", "transitions +")) for a in atomics)   # the tally, counts and transitions only
    classes = code[code.index("void change_classes_kernel"):code.index("stage_row_sets")]
    assert "atomic" not in classes and "__shared__" not in classes
    assert code.count("<<<") == 4 and "change_codes_kernel<false>" in code and "change_codes_kernel<true>" in code   # clear, classes, and one of two codes kernels
    assert " change_ops.hip " in open(os.path.join(CSRC, "Makefile")).read()


def test_the_magic_is_checked_before_use(monkeypatch):
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT14_MAGIC", _lib.EXT14_MAGIC + 1)
    with pytest.raises(RuntimeError, match="the library has no fourteenth extension table \\(fs_mosaic_change is missing\\)"):
        fresh.fs_mosaic_change
    assert fresh.fs_mosaic_merge is not None                                  # the tables in front of it stay usable
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT13_MAGIC", _lib.EXT13_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first fourteen hook tables are not the ones this binding knows \\(fs_mosaic_change is missing\\)"):
        fresh.fs_mosaic_change
    monkeypatch.undo()
    assert fresh.fs_mosaic_change is not None


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    assert len(cref.refusal_cases()) >= 38
    for kw, word in cref.refusal_cases():
        assert cref.call_op(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert msg.startswith(b"mosaic_change:") and word in msg, (kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
def test_the_op_refuses_with_the_offending_value():
    va, vb = torch.zeros((5, 64, 96), dtype=torch.int16).view(torch.uint16), torch.zeros((5, 40, 48), dtype=torch.int16).view(torch.uint16)
    link = torch.zeros((16,), dtype=torch.int64)
    good = dict(votes_a=va, origin_a=(0, 0), votes_b=vb, origin_b=(3, 4), link=link)
    for kw, word in ((dict(votes_b=vb[:4]), "5 and 4"), (dict(votes_a=va.view(torch.int16)), "int16"), (dict(link=link[:8]), "(8,)"), (dict(link=link.int()), "int32"),
                     (dict(origin_b=(99999, 0)), "99999"), (dict(origin_a=(0, -16385)), "-16385"), (dict(min_votes=0), "got 0"), (dict(min_votes=65536), "65536"),
                     (dict(min_conf=256), "256"), (dict(min_conf=-1), "-1"), (dict(tolerance=9), "got 9"), (dict(tolerance=-1), "-1"), (dict(watch=(5,)), "[5]"),
                     (dict(watch=(1, 32)), "[1, 32]"), (dict(votes_b=va), "same memory")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.mosaic_change(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.mosaic_change: tensors must live on the GPU"):
        ops.mosaic_change(**good)
    with pytest.raises(RuntimeError, match="floodseg.mosaic_change: tensors must live on the GPU"):
        ops.mosaic_change(**good, watch=())                                    # an empty watch set is a comparison without water
    assert "guesses, not validated on real video" in ops.mosaic_change.__doc__ and "guesses, not validated on real video" in predict.mosaic_change.__doc__
    assert ops.CHANGE_CODES == ("not_comparable", "same", "explained", "changed", "gained", "lost") and ops.CHANGE_CLASSES == 6
    assert np.array_equal(predict.CHANGE_PALETTE, cref.PALETTE) and predict.CHANGE_PALETTE[:2, 3].tolist() == [0, 0] and (predict.CHANGE_PALETTE[2:, 3] > 0).all()


def cpu_part(p, mode="centre"):
    """One of the reference's parts as FlowPredictor.mosaic_part() hands it out, on the CPU."""
    t = torch.from_numpy
    return dict(votes=t(p["votes"].copy()), rank=t(p["rank"].view(np.int64).copy()), rgba=t(p["rgba"].view(np.int32).copy()), state=t(p["state"].copy()),
                poses=t(p["poses"].copy()), tail=t(p["tail"].copy()), origin=gref.SPLIT_ORIGIN, mask_size=(64, 96), frames=p["frames"], mode=mode)


def test_the_helper_refuses_before_anything_is_enqueued():
    a, b, exact, _ = cref.two_flights()
    mine, part = cpu_part(a), cpu_part(b)
    for kw, word in ((dict(part_b=dict(part, mask_size=(64, 80))), "(64, 96) and (64, 80)"), (dict(part_b=dict(part, votes=part["votes"][:3])), "4 and 3"),
                     (dict(part_b=dict(part, rgba=None)), "register=True reads both orthophotos"), (dict(part_a=dict(mine, rgba=None)), "register=True reads both orthophotos"),
                     (dict(register=False), "needs the link"), (dict(outlines=True), "go with regions=True"), (dict(min_region_area=5), "go with regions=True"),
                     (dict(regions=True, simplify=1.0), "goes with outlines=True"), (dict(tolerence=2), "['tolerence']"),
                     (dict(register=False, link=torch.from_numpy(exact), search=8), "['search'] go with register=True")):
        with pytest.raises(ValueError, match=re.escape(word)):
            predict.mosaic_change(**{**dict(part_a=mine, part_b=part), **kw})
    with pytest.raises(RuntimeError, match="tensors must live on the GPU"):    # past the helper's own checks: the first op refuses CPU tensors
        predict.mosaic_change(mine, part, register=False, link=torch.from_numpy(exact))
    with pytest.raises(ValueError, match="mosaic_part\\(\\) needs mosaic="):
        FlowPredictor(torch.nn.Identity(), mosaic=(30, 40), ortho="centre").change_against(part)


def test_the_change_csv(tmp_path):
    a, b, _, _ = cref.two_flights()
    (change, _, _, transitions, counts), link, outs = cref.flights_change(a, b, cref.off_link(-3))
    path = str(tmp_path / "c.csv")
    predict.write_change_csv(path, dict(counts=counts, transitions=transitions))
    lines = open(path).read().split("\n")
    assert lines == cref.change_csv_lines(transitions, counts)
    assert lines[0] == "from,to,comparable,changed" and "0,1,105,105" in lines and lines[-2] == "registered,23040,6656,6551,0,0,105,0"
    predict.write_change_csv(path, dict(counts=np.array([2, 0, 0, 0, 0, 0, 0, 0]), transitions=np.zeros((2, 4, 4), np.int64)), class_names=["bg", "water", "c", "d"])
    assert open(path).read() == "from,to,comparable,changed\n\nlink,reached,comparable,same,explained,changed,gained,lost\nno_fit,0,0,0,0,0,0,0\n"


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name.replace(".py", "_tool_change"), os.path.join(ROOT, "tools", name))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_argument_checks(capsys):
    tool = load_tool("mosaic_change.py")
    a = tool.parse_args(["a.npz", "b.npz", "--out", "c.png", "--report", "r.csv", "--regions", "g.csv", "--outlines", "o.geojson", "--min-region", "9", "--tolerance", "3",
                         "--min-votes", "2", "--min-conf", "128", "--watch", "1", "2", "--search-scale", "8"])
    assert (a.before, a.after, a.out, a.report, a.regions, a.outlines) == ("a.npz", "b.npz", "c.png", "r.csv", "g.csv", "o.geojson")
    assert (a.min_region, a.tolerance, a.min_votes, a.min_conf, a.watch, a.search_scale, a.no_register) == (9, 3, 2, 128, [1, 2], 8, False)
    d = tool.parse_args(["a.npz", "b.npz", "--out", "c.png", "--no-register"])
    assert (d.tolerance, d.min_votes, d.min_conf, d.watch, d.search_scale, d.no_register, d.min_region) == (1, 1, 0, [1], None, True, 0)
    capsys.readouterr()
    base = ["a.npz", "b.npz", "--out", "c.png"]
    for bad, word in ((["a.npz", "--out", "c.png"], "AFTER.npz"), (["a.npz", "b.npz"], "--out"), (base + ["--search-scale", "5"], "4, 8 or 16"),
                      (base + ["--tolerance", "9"], "0..8"), (base + ["--min-votes", "0"], "1..65535"), (base + ["--min-conf", "256"], "0..255"),
                      (base + ["--search-scale", "8", "--no-register"], "--no-register"), (base + ["--min-region", "-1"], "pixel count")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert word in capsys.readouterr().err, bad
