"""The distance ops, the parts that need no GPU: the definition in numpy (tests/distance_ref.py) in separable form against a brute force
that is literally the definition, hand-computed planes and scipy where it is installed; csrc/distance_defs.h run on the CPU by a
stand-alone sanitized host program; the eighth hook table, the refusals, FlowPredictor's argument checks and the CSV writers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import distance_ref as dref
import regions_ref as rref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import predict
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mask_distance", "region_proximity"]
NONE = dref.NONE
SMALL = [i for i, c in enumerate(dref.case_list()) if max(c["geometry"]) <= 24]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def plane(rows):
    return np.array(rows, np.uint8)[None]


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_the_case_list_covers_what_it_says():
    cases = dref.case_list()
    assert len(cases) == len(dref.GEOMETRIES) * len(dref.FRAME_SETS) == 48
    assert {c["mask"].shape[0] for c in cases} == {1, 2, 3}
    assert {(1, 1), (1, 9), (9, 1), (37, 301), (67, 120), (130, 257), (3, 1500), (1100, 5)} == set(dref.GEOMETRIES)
    patterns = {p for c in cases for p in c["patterns"]}
    assert patterns == {"none", "all", "corner0", "corner1", "corner2", "corner3", "corners", "row", "column", "checker", "ties", "random01", "random5",
                        "random50"}
    assert dref.FRAME_SETS[0][1] == "none"                                  # an empty frame between two full ones
    big = [c for c in cases if c["geometry"] == (130, 257) and "random5" in c["patterns"]][0]["mask"]
    assert (big == 5).any() and (big == 33).any() and (big == 200).any()    # ids that are no class, one of them 32 + a source's id
    counts = dref.is_source(big, dref.SOURCE_SETS[0]).reshape(3, -1).sum(1)
    assert counts[0] < counts[1] < counts[2]                                # frames of one call with different source counts
    assert not dref.is_source(np.array([33, 200, 32, 5], np.uint8), 0xFFFFFFFF & ~(1 << 5)).any()
    assert len(SMALL) == 3 * len(dref.FRAME_SETS)


@pytest.mark.parametrize("i", SMALL)
def test_separable_reference_equals_the_brute_force(i):
    mask = dref.case_list()[i]["mask"]
    for source_set in dref.SOURCE_SETS:
        for r in dref.RADII:
            assert same(dref.expected(i, source_set, r), dref.mask_distance_bruteforce(mask, source_set, r)), (source_set, r)
            assert same(dref.expected(i, source_set, r), dref.mask_distance(mask, source_set, r)), (source_set, r)   # capped directly, not cut


def test_reference_equals_the_brute_force_on_random_planes_with_ties():
    """24 x 24 and 13 x 22 at densities where most pixels have several nearest sources."""
    rng = np.random.default_rng(dref.SEED)
    for h, w, density in ((24, 24, 0.02), (24, 24, 0.3), (13, 22, 0.08), (22, 13, 0.08)):
        mask = (rng.random((2, h, w)) < density).astype(np.uint8)
        want = dref.mask_distance_bruteforce(mask, 2)
        assert same(dref.mask_distance(mask, 2), want)
        d2 = want[0].astype(np.int64)
        yy, xx = np.mgrid[0:h, 0:w]
        for f in range(2):                                                  # not vacuous: pixels with several minimisers exist
            src = np.argwhere(mask[f] == 1)
            minimisers = (((yy[..., None] - src[:, 0]) ** 2 + (xx[..., None] - src[:, 1]) ** 2) == d2[f][..., None]).sum(-1)
            assert minimisers.min() >= 1 and (minimisers > 1).sum() > 10


def test_hand_computed_planes():
    # a single source in each corner of a 3 x 4 frame: d2 = dy^2 + dx^2 from that corner, nearest = its raster index everywhere
    yy, xx = np.mgrid[0:3, 0:4]
    for cy, cx in ((0, 0), (0, 3), (2, 0), (2, 3)):
        m = np.zeros((1, 3, 4), np.uint8)
        m[0, cy, cx] = 1
        d2, nearest = dref.mask_distance(m, 2)
        assert np.array_equal(d2[0], (yy - cy) ** 2 + (xx - cx) ** 2) and (nearest == cy * 4 + cx).all()
    # two sources mirror-symmetric about the centre pixel of a row: the axis pixel takes the smaller raster index
    d2, nearest = dref.mask_distance(plane([[1, 0, 0, 0, 1]]), 2)
    assert d2.tolist() == [[[0, 1, 4, 1, 0]]] and nearest.tolist() == [[[0, 0, 0, 4, 4]]]
    # ... and about the centre of a column: the upper one
    d2, nearest = dref.mask_distance(plane([[1], [0], [0], [0], [1]]), 2)
    assert d2.reshape(-1).tolist() == [0, 1, 4, 1, 0] and nearest.reshape(-1).tolist() == [0, 0, 0, 4, 4]
    # four sources around a centre: all at distance 2, the winner is the smallest raster index (the upper one, not the left one)
    d2, nearest = dref.mask_distance(plane([[0, 1, 0], [1, 0, 1], [0, 1, 0]]), 2)
    assert d2[0].tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 1]] and nearest[0].tolist() == [[1, 1, 1], [3, 1, 5], [3, 7, 5]]
    # a tie between an upper-right and a lower-left source at equal distance: raster order decides, whatever the column
    d2, nearest = dref.mask_distance(plane([[0, 0, 1], [0, 0, 0], [1, 0, 0]]), 2)
    assert d2[0, 1, 1] == 2 and nearest[0, 1, 1] == 2 and nearest[0, 0, 0] == 2 and nearest[0, 2, 2] == 2 and nearest[0, 2, 1] == 6
    # one source row, one source column
    m = np.zeros((1, 5, 4), np.uint8)
    m[0, 3, :] = 1
    d2, nearest = dref.mask_distance(m, 2)
    assert np.array_equal(d2[0], np.repeat(np.array([9, 4, 1, 0, 1])[:, None], 4, 1)) and np.array_equal(nearest[0], np.tile(12 + np.arange(4), (5, 1)))
    m = np.zeros((1, 4, 5), np.uint8)
    m[0, :, 1] = 1
    d2, nearest = dref.mask_distance(m, 2)
    assert np.array_equal(d2[0], np.tile(np.array([1, 0, 1, 4, 9]), (4, 1))) and np.array_equal(nearest[0], np.repeat((5 * np.arange(4) + 1)[:, None], 5, 1))
    # no source: NONE and -1; ids >= 32 are never sources, whatever bit they would wrap to; R cuts and never changes
    d2, nearest = dref.mask_distance(plane([[0, 33, 200, 2]]), 0xFFFFFFFA)
    assert (d2 == NONE).all() and (nearest == -1).all()
    d2, nearest = dref.mask_distance(plane([[1, 0, 0, 0, 0]]), 2, 2)
    assert d2.reshape(-1).tolist() == [0, 1, 4, NONE, NONE] and nearest.reshape(-1).tolist() == [0, 0, 0, -1, -1]
    # frames never see each other's sources
    d2, _ = dref.mask_distance(np.stack([plane([[1, 0]])[0], plane([[0, 0]])[0], plane([[0, 1]])[0]]), 2)
    assert d2.reshape(3, 2).tolist() == [[0, 1], [NONE, NONE], [1, 0]]


def test_scipy_agrees_where_it_is_installed():
    ndimage = pytest.importorskip("scipy.ndimage")
    for i in SMALL + [j for j, c in enumerate(dref.case_list()) if c["geometry"] == (37, 301)]:
        mask = dref.case_list()[i]["mask"]
        d2, _ = dref.expected(i, dref.SOURCE_SETS[1])
        for f in range(mask.shape[0]):
            src = dref.is_source(mask[f], dref.SOURCE_SETS[1])
            if src.any():
                assert np.array_equal(np.rint(ndimage.distance_transform_edt(~src) ** 2).astype(np.int64), d2[f].astype(np.int64))
            else:
                assert (d2[f] == NONE).all()


def test_hand_computed_proximity():
    """Water (1) on the left, a building (3) of two pixels and a street (4): K = 5, thresholds 1 and 2."""
    mask = plane([[1, 0, 3, 3, 4],
                  [1, 0, 0, 0, 4]])
    d2, nearest = dref.mask_distance(mask, 2)
    assert d2[0].tolist() == [[0, 1, 4, 9, 16], [0, 1, 4, 9, 16]]
    table, counts, index = rref.region_table(mask, rref.mask_regions(mask, 5, 8), 5, None, 128, 8)
    assert counts.tolist() == [[4, 4]] and index[0].tolist() == [[0, 1, 2, 2, 3], [0, 1, 1, 1, 3]]
    exposure, near = dref.region_proximity(mask, d2, nearest, index, counts, 5, 8, 0b11000, (1, 2))
    assert exposure[0].tolist() == [[0, 0], [0, 0], [0, 0], [0, 1], [0, 0]]        # one building pixel within 2, no street pixel
    assert near[0, :4].tolist() == [[0, 0, 0, 0, 0, 0, 2, 0], [1, 1, 0, 0, 0, 0, 2, 0], [4, 2, 0, 0, 0, 0, 0, 0], [16, 4, 0, 0, 0, 0, 0, 0]]
    assert not near[0, 4:].any()
    capped = dref.capped(d2, nearest, 3)
    exposure, near = dref.region_proximity(mask, capped[0], None, index, counts, 5, 8, 0b11001, (1, 2))
    assert exposure[0].tolist() == [[2, 3], [0, 0], [0, 0], [0, 1], [0, 0]]        # class 0 is a target now: two pixels at 1, a third at 2
    assert near[0, :4].tolist() == [[0, 0, 0, -1, -1, -1, 2, 0], [1, 1, 0, -1, -1, -1, 2, 0], [4, 2, 0, -1, -1, -1, 0, 0], [-1, -1, -1, -1, -1, -1, 0, 0]]
    _, counts2, index2 = rref.region_table(mask, rref.mask_regions(mask, 5, 8), 5, None, 128, 2)   # a cap of two rows: the rest has no row
    exposure, near = dref.region_proximity(mask, d2, nearest, index2, counts2, 5, 2, 0b11000, (1, 2))
    assert near[0].tolist() == [[0, 0, 0, 0, 0, 0, 2, 0], [1, 1, 0, 0, 0, 0, 2, 0]] and exposure[0, 3].tolist() == [0, 1]


def test_the_cases_reach_what_they_are_for():
    """Not vacuous: rows with and without a finite distance, rows cut by the small cap, non-zero exposure, ties in the near rows."""
    finite = unreachable = cut = exposed = 0
    for i in range(len(dref.case_list())):
        exposure, near = dref.expected_proximity(i, dref.SOURCE_SETS[0], 2, dref.SMALL_CAP, dref.THRESHOLDS_1, True)
        counts = dref.region_tables(i)[dref.SMALL_CAP][1]
        cut += int((counts[:, 0] > counts[:, 1]).sum())
        for f in range(near.shape[0]):
            rows = near[f, :counts[f, 1]]
            finite += int((rows[:, 0] >= 0).sum())
            unreachable += int((rows[:, 0] < 0).sum())
        exposed += int(exposure.sum() > 0)
    assert finite > 100 and unreachable > 20 and cut > 20 and exposed > 10


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def test_the_headers_scan_and_tie_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/distance_defs.h is plain __host__ __device__ C++: tests/distance_host_check.cpp runs the chunk words, the column tie rule and
    the row scan with its stop rule, as a stand-alone program built with -fsanitize=address,undefined; d2 and nearest are the
    reference's, pixel by pixel."""
    makefile = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "distance_host_check"), str(tmp_path / "cases.bin")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc"), os.path.join(ROOT, "tests", "distance_host_check.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):   # the runtimes linked in where the compiler can
        build = subprocess.run(base + static, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    tall = [j for j, c in enumerate(dref.case_list()) if c["geometry"] == (1100, 5)]   # columns of 18 chunks: the carries
    ragged = [j for j, c in enumerate(dref.case_list()) if c["geometry"] == (67, 120)][:2]
    entries = [(i, s, r, nr) for i in SMALL + tall + ragged for s in dref.SOURCE_SETS for r, nr in ((0, 1), (2, 1), (7, 0), (0, 0))]
    want = []
    with open(data, "wb") as fh:
        fh.write(np.int32(len(entries)).tobytes())
        for j, (i, source_set, r, with_nearest) in enumerate(entries):
            mask = dref.case_list()[i]["mask"]
            fh.write(np.array(mask.shape + (source_set, r, with_nearest), np.int32).tobytes())
            fh.write(mask.tobytes())
            d2, nearest = dref.expected(i, source_set, r)
            want.append(f"case {j}")
            want.extend(f"{a} {b if with_nearest else 0}" for a, b in zip(d2.reshape(-1).tolist(), nearest.reshape(-1).tolist()))
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert run.stdout.split("\n")[:-1] == want
    assert len(want) > 200000                                               # not vacuous


# ------------------------------------------------------------------------------------------------ library surface
def test_the_eighth_table_in_header_initialiser_and_binding():
    assert _lib.ext7_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext7_api {"):text.index("} fs_ext7_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == _lib.ext7_hook_names()
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables6;") < text.index("typedef struct fs_ext7_api {") < text.index("typedef struct fs_hook_tables7 {")
    tables7 = text[text.index("typedef struct fs_hook_tables7 {"):text.index("} fs_hook_tables7;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables7) == [("fs_hook_tables6", "base6"), ("fs_ext7_api", "ext7")]
    assert int(re.search(r"#define FS_EXT7_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT7_MAGIC == int.from_bytes(b"FSEXTAB7", "big")
    assert int(re.search(r"#define FS_DIST_NONE (0x[0-9A-F]+)u", text).group(1), 16) == NONE == ops.DIST_NONE
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables7 all7 = {all6, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT7_MAGIC," in init and "sizeof(fs_ext7_api)," in init
    assert re.search(r"const fs_hook_tables6& all6 = all7\.base6;\s+return all6\.base5;", src)       # the head of the new object is handed out
    kernels = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "kernels.h")).read()
    assert "launch_mask_distance" in kernels and "launch_region_proximity" in kernels
    # the seven older tables and the export list are what they were
    assert [len(_lib.hook_names()), len(_lib.ext_hook_names()), len(_lib.ext2_hook_names()), len(_lib.ext3_hook_names()), len(_lib.ext4_hook_names()),
            len(_lib.ext5_hook_names()), len(_lib.ext6_hook_names())] == [38, 2, 14, 1, 1, 1, 1]
    assert [ctypes.sizeof(t) for t in (_lib.FsExtApi, _lib.FsExt2Api, _lib.FsExt3Api, _lib.FsExt4Api, _lib.FsExt5Api, _lib.FsExt6Api)] == [32, 128, 24, 24, 24, 24]
    assert not any("fs_" + name in _lib.exported_symbols() for name in NEW) and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    public = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(name in public for name in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables7.ext7.offset == ctypes.sizeof(_lib.FsHookTables6)                           # directly behind, no padding
    assert _lib.FsExt7Api.mask_distance.offset == 16 and _lib.FsExt7Api.region_proximity.offset == 24 and ctypes.sizeof(_lib.FsExt7Api) == 32
    all7 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables7)).contents
    assert all7.base6.ext6.magic == _lib.EXT6_MAGIC and all7.base6.ext6.size == 24
    assert all7.base6.base5.ext5.magic == _lib.EXT5_MAGIC and all7.base6.base5.base4.ext4.magic == _lib.EXT4_MAGIC
    assert all7.ext7.magic == _lib.EXT7_MAGIC and all7.ext7.size >= 32                                   # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all7.ext7, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                                            # a table member, not an exported symbol
    assert ctypes.cast(all7.base6.ext6.mask_stabilize, ctypes.c_void_p).value == ctypes.cast(lib.fs_mask_stabilize, ctypes.c_void_p).value
    macro = re.search(r"#define FS_MASK_DISTANCE_WORKSPACE_BYTES\(n, H, W\) \\\n(.*)", text).group(1)
    for n, h, w in ((1, 1, 1), (5, 1072, 1920), (3, 37, 301), (2, 64, 7), (2, 65, 7), (3, 1100, 5), (65535, 3, 5), (1, 32768, 32768)):
        got = eval(macro.replace("(size_t)", "").replace("/", "//"), dict(n=n, H=h, W=w))
        assert got == ops.mask_distance_workspace_bytes(n, h, w) == dref.workspace_bytes(n, h, w) and got % 16 == 0
        assert got >= 2 * n * h * w + 4 * n * -(-h // 64) * w


def test_the_magic_is_checked_before_use(monkeypatch):
    """A binding that expects another magic finds no eighth table in this library and says so, instead of calling through it."""
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT7_MAGIC", _lib.EXT7_MAGIC + 1)
    with pytest.raises(RuntimeError, match="seventh extension table"):
        fresh.fs_mask_distance
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT6_MAGIC", _lib.EXT6_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first seven hook tables"):
        fresh.fs_region_proximity
    monkeypatch.undo()
    assert fresh.fs_mask_distance is not None and fresh.fs_region_proximity is not None and fresh.fs_mask_stabilize is not None


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    assert len(dref.refusal_cases()) >= 46
    for op, kw, word in dref.refusal_cases():
        assert dref.call_distance_op(lib, op, **kw) != 0, (op, kw)
        msg = lib.fs_last_error()
        assert msg.startswith(op.encode() + b":") and word in msg, (op, kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
def test_ops_refuse_before_the_library_is_asked():
    mask = torch.zeros((2, 4, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="floodseg.mask_distance: tensors must live on the GPU"):
        ops.mask_distance(mask, (1,))
    assert ops.mask_distance_workspace_bytes(5, 1072, 1920) == (5 * 17 * 1920 * 4 + 5 * 1072 * 1920 * 2 + 15) // 16 * 16
    assert ops.class_set((1,), "sources", "x") == 2 and ops.class_set((1, 3, 31), "sources", "x") == 0x8000000A and ops.class_set((), "t", "x", True) == 0
    for bad in ((), (32,), (-1,)):
        with pytest.raises(ValueError, match=re.escape(str(list(bad)))):
            ops.class_set(bad, "sources", "floodseg.mask_distance")


def test_predictor_argument_checks():
    ident = torch.nn.Identity()
    p = FlowPredictor(ident)
    assert p.proximity is None and p.proximity_max == 0
    exposure, near = p.proximity_report()
    assert exposure.shape == (0, 5, 0) and exposure.dtype == np.int64 and near == []
    with pytest.raises(ValueError, match="proximity needs regions=True"):
        FlowPredictor(ident, proximity=(8,))
    on = FlowPredictor(ident, regions=True, proximity=(8, 16, 32))
    assert on.proximity == (8, 16, 32) and on.proximity_sources == (1,) and on.proximity_targets == (3, 4)
    assert on.proximity_max == 0                                            # unbounded unless asked: DESIGN §3.17 has the measured worst case
    assert on.proximity_report()[0].shape == (0, 5, 3)
    assert FlowPredictor(ident, regions=True, proximity=(8,), proximity_max=0).proximity_max == 0          # unbounded on request
    assert FlowPredictor(ident, regions=True, proximity=(8,), proximity_max=100).proximity_max == 100
    for bad in ((), (1, 1), (3, 2), (-1,), (32768,), tuple(range(9))):
        with pytest.raises(ValueError, match="proximity must be 1..8 strictly ascending"):
            FlowPredictor(ident, regions=True, proximity=bad)
    with pytest.raises(ValueError, match="proximity_sources"):
        FlowPredictor(ident, regions=True, proximity=(8,), proximity_sources=())
    with pytest.raises(ValueError, match="proximity_targets"):
        FlowPredictor(ident, regions=True, proximity=(8,), proximity_targets=(40,))
    with pytest.raises(ValueError, match="proximity_max must be"):
        FlowPredictor(ident, regions=True, proximity=(8,), proximity_max=32768)
    with pytest.raises(ValueError, match="below the largest threshold"):
        FlowPredictor(ident, regions=True, proximity=(8, 16), proximity_max=10)


# ------------------------------------------------------------------------------------------------ the CSV writers
def small_report():
    """Two frames: regions_ref's tables of a 2 x 5 scene, the reference's proximity rows, tracks made up by hand."""
    mask = np.stack([plane([[1, 0, 3, 3, 4], [1, 0, 0, 0, 4]])[0], plane([[0, 0, 3, 3, 4], [0, 0, 0, 1, 4]])[0]])
    d2, nearest = dref.capped(*dref.mask_distance(mask, 2), 3)
    table, counts, index = rref.region_table(mask, rref.mask_regions(mask, 5, 8), 5, None, 128, 8)
    exposure, near = dref.region_proximity(mask, d2, nearest, index, counts, 5, 8, 0b11000, (1, 2))
    rows = [table[f, :counts[f, 1]] for f in range(2)]
    nears = [near[f, :counts[f, 1]] for f in range(2)]
    tracks = [np.array([[10, -1, -1, 0], [11, -1, -1, 0], [12, -1, -1, 0], [13, -1, -1, 0]]), np.array([[11, -1, 1, 5], [12, -1, 2, 2], [14, 10, 0, 1], [13, -1, 3, 2]])]
    return rows, nears, tracks, exposure


def test_csv_writers_round_trip_and_are_unchanged_without_proximity(tmp_path):
    rows, nears, tracks, exposure = small_report()
    assert [len(r) for r in rows] == [4, 4]
    a, b, c = str(tmp_path / "a.csv"), str(tmp_path / "b.csv"), str(tmp_path / "c.csv")
    # proximity=None: byte for byte what the writers give without the argument, for every combination of the other columns
    for kw in (dict(), dict(tracks=tracks), dict(with_confidence=False)):
        predict.write_regions_csv(a, [7, 8], rows, **kw)
        predict.write_regions_csv(b, [7, 8], rows, proximity=None, **kw)
        assert open(a, "rb").read() == open(b, "rb").read()
        predict.write_regions_csv(c, [7, 8], rows, proximity=nears, **kw)
        plain, more = open(a).read().split("\n"), open(c).read().split("\n")
        extra = ",dist,near_px,nearest_region" + (",nearest_track" if "tracks" in kw else "")
        assert more[0] == plain[0] + extra and all(m.startswith(p + ",") for p, m in zip(plain[1:-1], more[1:-1])) and len(plain) == len(more) == 10
    lines = open(c).read().split("\n")                                      # the last loop: without confidence and tracks
    cells = [line.split(",")[-3:] for line in lines[1:-1]]
    assert cells[:4] == [["0.000", "2", "0"], ["1.000", "2", "0"], ["2.000", "0", "0"], ["", "0", "-1"]]      # the street is out of reach at R = 3
    assert cells[4:] == [["1.000", "1", "3"], ["1.000", "1", "3"], ["1.000", "1", "3"], ["0.000", "1", "3"]]     # frame 8: the water is region 3
    predict.write_regions_csv(c, [7, 8], rows, tracks=tracks, proximity=nears)
    cells = [line.split(",")[-4:] for line in open(c).read().split("\n")[1:-1]]
    assert cells[0] == ["0.000", "2", "0", "10"] and cells[3] == ["", "0", "-1", "-1"] and cells[4] == ["1.000", "1", "3", "13"]
    with pytest.raises(ValueError, match="proximity must hold one row per region"):
        predict.write_regions_csv(c, [7, 8], rows, proximity=nears[:1])
    # the tracks summary
    predict.write_tracks_csv(a, [7, 8], rows, tracks)
    predict.write_tracks_csv(b, [7, 8], rows, tracks, proximity=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    predict.write_tracks_csv(c, [7, 8], rows, tracks, proximity=nears)
    plain, more = open(a).read().split("\n"), open(c).read().split("\n")
    assert more[0] == plain[0] + ",first_dist,last_dist,min_dist" and [m[:len(p)] for p, m in zip(plain, more)] == plain
    by_track = {line.split(",")[0]: line.split(",")[-3:] for line in more[1:-1]}
    assert by_track == {"10": ["0.000", "0.000", "0.000"], "11": ["1.000", "1.000", "1.000"], "12": ["2.000", "1.000", "1.000"],
                        "13": ["", "0.000", "0.000"], "14": ["1.000", "1.000", "1.000"]}
    # the exposure table
    predict.write_exposure_csv(a, [7, 8], exposure, (1, 2), 10)
    lines = open(a).read().split("\n")
    assert lines[0].split(",")[:5] == ["frame", "within_0_1", "share_0_1", "within_0_2", "share_0_2"] and len(lines[0].split(",")) == 1 + 5 * 2 * 2
    got = np.array([[float(v) for v in line.split(",")] for line in lines[1:-1]])
    assert got[:, 0].tolist() == [7, 8] and np.array_equal(got[:, 1::2].reshape(2, 5, 2), exposure) and np.allclose(got[:, 2::2], got[:, 1::2] / 10)
    assert exposure[0, 3].tolist() == [0, 1] and exposure[1, 3].tolist() == [1, 2] and exposure[1, 4].tolist() == [1, 2]
    with pytest.raises(ValueError, match="exposure must be"):
        predict.write_exposure_csv(a, [7], exposure, (1, 2), 10)
