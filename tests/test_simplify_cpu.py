"""Outline simplification, the parts that need no GPU: the definition in numpy (tests/simplify_ref.py, recursive) against the figures
of the prototype and the properties the definition implies, csrc/simplify_defs.h run in round form on the CPU by a stand-alone
sanitized host program, the fifth hook table, the refusals, the GeoJSON writer, and the FlowPredictor plumbing on stubs."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import outlines_ref as oref
import regions_ref as rref
import simplify_ref as sref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import predict
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "outline_simplify"
CAPS = (8, 32, 256)


# ------------------------------------------------------------------------------------------------ the prototype's figures
# case: vertices, then (kept vertices, rounds, flagged unconverged) at (tol_q, cap) = (0, 256), (4, 256), (16, 256), (64, 256), (16, 8), (16, 32)
TABLE = {
    "pixel": (4, [(4, 1, 0)] * 6),
    "diagonal": (8, [(8, 3, 0), (4, 1, 0), (4, 1, 0), (4, 1, 0), (4, 1, 0), (4, 1, 0)]),
    "33x67": (2980, [(2980, 11, 0), (2570, 10, 0), (1715, 9, 0), (1475, 7, 0), (1719, 8, 1), (1715, 9, 0)]),
    "n3": (4000, [(4000, 10, 0), (3306, 9, 0), (2128, 7, 0), (1819, 5, 0), (2128, 7, 0), (2128, 7, 0)]),
    "checker": (2048, [(2048, 33, 0), (2040, 32, 0), (1804, 1, 0), (1804, 1, 0), (1804, 1, 0), (1804, 1, 0)]),
    "serpentine": (5464, [(5464, 172, 0), (5380, 171, 0), (87, 44, 0), (45, 42, 0), (4951, 8, 1), (1879, 32, 1)]),
    "comb": (260, [(260, 129, 0), (258, 128, 0), (131, 126, 0), (128, 124, 0), (253, 8, 1), (229, 32, 1)]),
    "blob": (282, [(282, 16, 0), (232, 14, 0), (51, 7, 0), (36, 4, 0), (51, 7, 0), (51, 7, 0)]),
}
COLUMNS = ((0, 256), (4, 256), (16, 256), (64, 256), (16, 8), (16, 32))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_reference_gives_the_prototypes_figures(name):
    """Connectivity 8; a batch counts as one: the vertices summed, the largest round, any flag."""
    vertices, cells = TABLE[name]
    assert int(sref.outlines_of(name, 8)["counts"][:, 2].sum()) == vertices
    for (tol_q, cap), want in zip(COLUMNS, cells):
        _, _, counts = sref.expected(name, 8, tol_q, cap)
        assert (int(counts[:, 1].sum()), int(counts[:, 2].max()), int((counts[:, 3] & 1).any())) == want, (name, tol_q, cap)
        assert not (counts[:, 3] & ~1).any()


def test_at_one_pixel_and_the_default_cap_only_serpentine_and_comb_are_flagged():
    for conn in (4, 8):
        flagged = {name for name in sref.CASES if (sref.expected(name, conn, 16, 32)[2][:, 3] & 1).any()}
        assert flagged == {"serpentine", "comb"}, conn


# ------------------------------------------------------------------------------------------------ properties
def distance2(v, idx, a, b):
    """The squared distances of the vertices v[idx] to the segments v[a] -> v[b] in float64, by projection: not the reference's key."""
    p, s, e = v[idx].astype(np.float64), v[a].astype(np.float64), v[b].astype(np.float64)
    u, w = e - s, p - s
    length2 = (u * u).sum(1)
    t = np.clip(np.divide((u * w).sum(1), length2, out=np.zeros(len(p)), where=length2 > 0), 0.0, 1.0)
    d = w - t[:, None] * u
    return (d * d).sum(1)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", sorted(sref.CASES))
def test_properties_on_every_case(name, conn):
    e = sref.outlines_of(name, conn)
    for f in range(len(e["counts"])):
        for row in e["contours"][f, :int(e["counts"][f, 1])].tolist():
            ring = np.asarray(e["vertices"][f, row[1]:row[1] + row[2]], np.int64)
            m = len(ring)
            for cap in CAPS:
                before = None
                for tol_q in sref.TOLS:
                    kept, rounds, flagged = sref.simplify_ring(ring, tol_q, cap)
                    where = (name, conn, f, row[5], tol_q, cap)
                    assert kept[0] == 0 and kept == sorted(set(kept)) and kept[-1] < m and len(kept) >= 3, where   # a subsequence from the anchor's vertex
                    assert 0 <= rounds <= cap, where
                    ends = np.array(kept + [m])
                    dropped = np.setdiff1d(np.arange(m), kept)
                    span = np.searchsorted(ends, dropped) - 1                                                       # the kept segment that spans each
                    d2 = distance2(ring, dropped, ends[span], ends[span + 1] % m)
                    assert (d2 <= tol_q / 16.0 * (1 + 1e-12) + 1e-9).all(), where                                    # cap or no cap
                    if tol_q == 0 and not flagged:
                        assert sref.area2_of(ring[kept]) == row[4], where
                    if before is not None and not before[1]:                                                         # a smaller tolerance converged:
                        assert not flagged and set(kept) <= set(before[0]), where                                    # nested, so never more vertices
                    before = (kept, flagged)


def test_the_frame_function_concatenates_the_rings():
    e = sref.outlines_of("lake", 8)
    simple, vertices, counts = sref.expected("lake", 8, 16, 32)
    rows = int(e["counts"][0, 1])
    assert counts.tolist() == [[rows, int(simple[0, :rows, 1].sum()), 1, 0]] and not simple[0, rows:].any() and not vertices[0, int(counts[0, 1]):].any()
    assert simple[0, :rows, 0].tolist() == (np.cumsum(simple[0, :rows, 1]) - simple[0, :rows, 1]).tolist()
    for k in range(rows):
        _, off, m = e["contours"][0, k, :3]
        kept, _, _ = sref.simplify_ring(e["vertices"][0, off:off + m], 16, 32)
        got = vertices[0, simple[0, k, 0]:simple[0, k, 0] + simple[0, k, 1]]
        assert np.array_equal(got, e["vertices"][0, off:off + m][kept]) and simple[0, k, 2] == sref.area2_of(got)
        assert (simple[0, k, 2] > 0) == (e["contours"][0, k, 4] > 0)                                                 # squares: nothing to drop
    assert np.array_equal(vertices[0, :int(counts[0, 1])], e["vertices"][0, :int(e["counts"][0, 2])])


# ------------------------------------------------------------------------------------------------ input handling
def test_frames_that_break_a_rule_get_nothing_and_their_flag():
    for what, c, v, n, flag in sref.broken_frames():
        simple, vertices, counts = sref.outline_simplify(c, v, n, 16, 32)
        assert counts.tolist() == [[0, 0, 0, flag]] and not simple.any() and not vertices.any(), what


def test_a_frame_with_more_contours_than_rows_is_simplified_and_flagged():
    full = sref.expected("lake", 8, 16, 32, 8, 64)
    e = sref.outlines_of("lake", 8, 4, 64)
    assert e["counts"].tolist() == [[6, 4, 24, 2]]
    simple, vertices, counts = sref.expected("lake", 8, 16, 32, 4, 64)
    assert counts.tolist() == [[4, 16, 1, 4]] and np.array_equal(simple[0], full[0][0, :4]) and np.array_equal(vertices[0, :16], full[1][0, :16])
    assert not vertices[0, 16:].any()                                                                                # contours without a row: not simplified


def test_coordinates_are_read_clamped():
    c, v, n = (np.array(sref.outlines_of("pixel", 8, 4, 16)[key]) for key in ("contours", "vertices", "counts"))
    v[0, :4] = [[-5, -5], [1 << 30, 0], [1 << 30, 1 << 30], [-(1 << 31), 1 << 20]]
    simple, vertices, counts = sref.outline_simplify(c, v, n, 16, 32)
    assert vertices[0, :4].tolist() == [[0, 0], [16384, 0], [16384, 16384], [0, 16384]] and simple[0, 0].tolist() == [0, 4, 2 * 16384 ** 2, 0]


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def rows_of(simple, counts, f):
    return simple[f, :int(counts[f, 0])].tolist()


def test_the_headers_functions_in_round_form_under_sanitizers(tmp_path):
    """csrc/simplify_defs.h is plain __host__ __device__ C++: tests/simplify_host_check.cpp runs every case through it round by round,
    as the kernels do -- cells, slots of two parities, the largest key and the smallest index among its holders -- as a stand-alone
    program built with -fsanitize=address,undefined; the rows it prints are those of the recursive reference."""
    makefile = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "simplify_host_check"), str(tmp_path / "cases.bin")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc"), os.path.join(ROOT, "tests", "simplify_host_check.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):   # the runtimes linked in where the compiler can
        build = subprocess.run(base + static, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    runs = [(name, conn, tol_q, cap, 4096, 8192) for name in sorted(sref.CASES) for conn in (4, 8) for tol_q, cap in ((0, 256), (16, 8), (16, 32), (64, 256))]
    runs += [("lake", 8, 16, 32, 4, 64), ("n3", 8, 4, 32, 4096, int(np.sort(sref.outlines_of("n3", 8)["counts"][:, 2])[1]))]  # cut rows; one frame overflows
    want = []
    with open(data, "wb") as fh:
        fh.write(np.int32(len(runs)).tobytes())
        for c, (name, conn, tol_q, cap, mc, mv) in enumerate(runs):
            e = sref.outlines_of(name, conn, mc, mv)
            simple, _, counts = sref.expected(name, conn, tol_q, cap, mc, mv)
            fh.write(np.array([len(counts), mc, mv, tol_q, cap], np.int32).tobytes())
            for key, dtype in (("contours", np.int64), ("vertices", np.int32), ("counts", np.int64)):
                fh.write(np.ascontiguousarray(e[key], dtype).tobytes())
            want.append(f"case {c}")
            for f in range(len(counts)):
                want.append(" ".join(str(v) for v in ["frame", f] + counts[f].tolist()))
                want.extend(" ".join(str(v) for v in [f, k] + row) for k, row in enumerate(rows_of(simple, counts, f)))
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert run.stdout.split("\n")[:-1] == want
    assert sum(1 for line in want if line.endswith(" 0 0 0 2")) == 1 and sum(1 for line in want if line.startswith("frame") and line.endswith(" 4")) == 1
    assert len(want) > 5000


# ------------------------------------------------------------------------------------------------ library surface
def test_the_fifth_table_in_header_initialiser_and_binding():
    assert _lib.ext4_hook_names() == [NEW]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext4_api {"):text.index("} fs_ext4_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == _lib.ext4_hook_names()
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables3;") < text.index("typedef struct fs_ext4_api {") < text.index("typedef struct fs_hook_tables4 {")
    tables4 = text[text.index("typedef struct fs_hook_tables4 {"):text.index("} fs_hook_tables4;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables4) == [("fs_hook_tables3", "base3"), ("fs_ext4_api", "ext4")]
    assert int(re.search(r"#define FS_EXT4_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT4_MAGIC == int.from_bytes(b"FSEXTAB4", "big")
    src = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read()
    assert "static const fs_hook_tables3 all3 = {all, {\n        FS_EXT3_MAGIC,\n        sizeof(fs_ext3_api),\n        fs_region_outlines,\n    }};" in src
    init = src[src.index("static const fs_hook_tables4 all4 = {all3, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + NEW]
    assert "FS_EXT4_MAGIC," in init and "sizeof(fs_ext4_api)," in init and "return &all4.base3.base2.base.test;" in src
    assert "launch_outline_simplify" in open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "kernels.h")).read()
    # the four older tables and the export list are what they were
    assert [len(_lib.hook_names()), len(_lib.ext_hook_names()), len(_lib.ext2_hook_names()), len(_lib.ext3_hook_names())] == [38, 2, 14, 1]
    assert ctypes.sizeof(_lib.FsExt2Api) == 128 and ctypes.sizeof(_lib.FsExt3Api) == 24
    assert "fs_" + NEW not in _lib.exported_symbols() and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    assert NEW not in open(os.path.join(ROOT, "include", "floodseg.h")).read()
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables4.ext4.offset == ctypes.sizeof(_lib.FsHookTables3)                           # directly behind, no padding
    assert _lib.FsExt4Api.outline_simplify.offset == 16 and ctypes.sizeof(_lib.FsExt4Api) == 24
    all4 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables4)).contents
    assert all4.base3.base2.ext2.magic == _lib.EXT2_MAGIC and all4.base3.base2.ext2.size == 128
    assert all4.base3.ext3.magic == _lib.EXT3_MAGIC and all4.base3.ext3.size == 24
    assert all4.ext4.magic == _lib.EXT4_MAGIC and all4.ext4.size >= 24                                   # from below only: the table grows at its end
    assert ctypes.cast(all4.ext4.outline_simplify, ctypes.c_void_p).value and lib.fs_outline_simplify is not None
    assert ctypes.cast(all4.base3.ext3.region_outlines, ctypes.c_void_p).value == ctypes.cast(lib.fs_region_outlines, ctypes.c_void_p).value
    with pytest.raises(AttributeError):
        getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + NEW)                                                 # a table member, not an exported symbol
    macro = " ".join(line.rstrip("\\").strip() for line in re.search(
        r"#define FS_OUTLINE_SIMPLIFY_WORKSPACE_BYTES\(n, max_contours, max_vertices\)((?:.*\\\n)*.*)", text).group(1).split("\n"))
    for n, c, v in ((1, 1, 4), (3, 4096, 32768), (5, 2 ** 20, 2 ** 22), (2, 7, 1025), (1, 8, 2049)):
        got = eval(macro.replace("(size_t)", "").replace("/", "//"), dict(n=n, max_contours=c, max_vertices=v))
        assert got == ops.outline_simplify_workspace_bytes(n, c, v) == sref.workspace_bytes(n, c, v) and got % 8 == 0
    defs = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "simplify_defs.h")).read()
    assert "HDR_INTS = HDR_SPLIT + ROUND_SLOTS;  // 524" in defs and sref.workspace_bytes(1, 1, 4) == 8 * (24 + 1 + 1 + 524 // 2)


def test_the_magic_is_checked_before_use(monkeypatch):
    """A binding that expects another magic finds no fifth table in this library and says so, instead of calling through it."""
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT4_MAGIC", _lib.EXT4_MAGIC + 1)
    with pytest.raises(RuntimeError, match="fourth extension table"):
        fresh.fs_outline_simplify
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT3_MAGIC", _lib.EXT3_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first four hook tables"):
        fresh.fs_outline_simplify
    monkeypatch.undo()
    assert fresh.fs_outline_simplify is not None and fresh.fs_region_outlines is not None


def test_library_refuses_bad_arguments_before_a_launch():
    """Fake non-null pointers: a call that got as far as a launch would fail with another message (or fault on a GPU)."""
    lib = _lib.load()
    cases = sref.refusal_cases()
    assert len(cases) == 18
    for kw, word in cases:
        assert sref.call_simplify(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert word.encode() in msg and NEW.encode() in msg, (kw, msg)


def test_ops_and_predictor_refuse_bad_arguments():
    contours, vertices, counts = torch.zeros(1, 4, 6, dtype=torch.int64), torch.zeros(1, 8, 2, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.outline_simplify(contours, vertices, counts, 1.0)
    for tol in (-0.5, 256.5, float("nan")):
        with pytest.raises(ValueError, match="tolerance"):
            ops.outline_simplify(contours, vertices, counts, tol)
    for rounds in (0, 257):
        with pytest.raises(ValueError, match="max_rounds"):
            ops.outline_simplify(contours, vertices, counts, 1.0, rounds)
    assert [ops.simplify_tol_q(t) for t in (0, 0.5, 1, 2, 256)] == [0, 4, 16, 64, 2 ** 20]
    with pytest.raises(ValueError, match="outlines=True"):
        FlowPredictor(torch.nn.Identity(), regions=True, simplify=1.0)
    with pytest.raises(ValueError, match="tolerance"):
        FlowPredictor(torch.nn.Identity(), regions=True, outlines=True, simplify=-1.0)
    with pytest.raises(ValueError, match="simplify_rounds"):
        FlowPredictor(torch.nn.Identity(), regions=True, outlines=True, simplify=1.0, simplify_rounds=0)
    p = FlowPredictor(torch.nn.Identity(), regions=True, outlines=True, simplify=1.0)
    per_frame = 8 * 32768 + 32 * 4096 + 32
    assert p.outline_chunk == 138 and p.simple_chunk == 170 and p.simple_chunk * per_frame < 64 << 20 <= (p.simple_chunk + 1) * per_frame
    assert (p.simplify, p.simplify_rounds) == (1.0, 32) and p.simple_outline_report()[0] == [] and p.simple_outline_report()[1].shape == (0, 4)
    assert FlowPredictor(torch.nn.Identity(), regions=True, outlines=True).simplify is None


# ------------------------------------------------------------------------------------------------ the writer
def reports_of(name, conn, tol_q, cap, max_contours=4096, max_vertices=32768):
    """What region_report(), outline_report() and simple_outline_report() would hand out for a case."""
    _, mask, k, regions = sref.CASES[name]
    e = sref.outlines_of(name, conn, max_contours, max_vertices)
    simple, vertices, counts = sref.expected(name, conn, tol_q, cap, max_contours, max_vertices)
    table_rows = [e["table"][f, :int(e["tcounts"][f, 1])] for f in range(len(mask))]
    frames = []
    for f in range(len(mask)):
        total = 0 if e["counts"][f, 3] & 1 else int(e["counts"][f, 2])
        frames.append((e["contours"][f, :int(e["counts"][f, 1])], e["vertices"][f, :total], e["shape"][f, :len(table_rows[f])]))
    simplified = ([(simple[f, :int(counts[f, 0])], vertices[f, :int(counts[f, 1])]) for f in range(len(mask))], np.array(counts))
    return table_rows, (frames, e["counts"][:, 3].copy()), simplified


def test_geojson_without_the_simple_report_is_byte_for_byte_the_old_file(tmp_path):
    table_rows, outlines, _ = reports_of("n3", 8, 16, 32)
    old, new = str(tmp_path / "a.geojson"), str(tmp_path / "b.geojson")
    predict.write_outlines_geojson(old, [4, 5, 6], table_rows, outlines)
    predict.write_outlines_geojson(new, [4, 5, 6], table_rows, outlines, simplified=None, tolerance=1.0)
    text = open(old).read()
    assert text == open(new).read() and text.startswith('{"type": "FeatureCollection", "overflowed_frames": [], "truncated_frames": [], "features": [{')
    assert "unconverged" not in text and "tolerance" not in text
    doc = json.loads(text)
    assert set(doc["features"][0]["properties"]) == {"frame", "region", "class", "area", "perimeter", "holes"}


def test_geojson_with_the_simple_report_writes_the_simplified_rings(tmp_path):
    path = str(tmp_path / "o.geojson")
    table_rows, outlines, simplified = reports_of("blob", 8, 16, 32)
    predict.write_outlines_geojson(path, ["f0"], table_rows, outlines, simplified=simplified, tolerance=1.0)
    with open(path) as fh:
        doc = json.load(fh)
    assert doc["unconverged_frames"] == [] and len(doc["features"]) == 1
    p, rings = doc["features"][0]["properties"], doc["features"][0]["geometry"]["coordinates"]
    assert set(p) == {"frame", "region", "class", "area", "perimeter", "holes", "tolerance", "vertices_full", "area2_simplified"}
    assert p["tolerance"] == 1.0 and p["vertices_full"] == 282 and p["holes"] == 1 and len(rings) == 2
    assert all(r[0] == r[-1] and len(r) >= 4 for r in rings) and sum(len(r) - 1 for r in rings) == 51
    area2 = [sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(r[:-1], r[1:])) for r in rings]
    assert area2[0] > 0 > area2[1] and sum(area2) == p["area2_simplified"] and abs(p["area2_simplified"] - 2 * p["area"]) < 0.02 * 2 * p["area"]
    # a frame that hit the cap is named; the overflowed one contributes nothing; tracks still add their two properties
    table_rows, outlines, simplified = reports_of("serpentine", 8, 16, 8)
    predict.write_outlines_geojson(path, [9], table_rows, outlines, simplified=simplified, tolerance=1.0)
    with open(path) as fh:
        doc = json.load(fh)
    assert doc["unconverged_frames"] == [9] and len(doc["features"][0]["geometry"]["coordinates"][0]) == 4951 + 1
    total = int(np.sort(sref.outlines_of("n3", 8)["counts"][:, 2])[1])
    table_rows, outlines, simplified = reports_of("n3", 8, 16, 32, 4096, total)
    assert sorted(simplified[1][:, 3].tolist()) == [0, 0, 2]
    tracks = [np.stack([np.arange(len(t)) + 100, np.full(len(t), -1), np.full(len(t), -1), np.zeros(len(t), np.int64)], 1) for t in table_rows]
    predict.write_outlines_geojson(path, ["a", "b", "c"], table_rows, outlines, tracks=tracks, simplified=simplified, tolerance=1.0)
    with open(path) as fh:
        doc = json.load(fh)
    bad = "abc"[simplified[1][:, 3].tolist().index(2)]
    assert doc["overflowed_frames"] == [bad] and doc["unconverged_frames"] == [] and all(f["properties"]["frame"] != bad for f in doc["features"])
    assert all(f["properties"]["track"] == f["properties"]["region"] + 100 and f["properties"]["tolerance"] == 1.0 for f in doc["features"])
    with pytest.raises(ValueError, match="tolerance"):
        predict.write_outlines_geojson(path, ["a", "b", "c"], table_rows, outlines, simplified=simplified)
    with pytest.raises(ValueError, match="one simplified outline per frame"):
        predict.write_outlines_geojson(path, ["a", "b", "c"], table_rows, outlines, simplified=(simplified[0][:2], simplified[1][:2]), tolerance=1.0)


# ------------------------------------------------------------------------------------------------ plumbing
def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class StubFlow(torch.nn.Module):
    """A flow model that returns fixed logits [n,K,H,W] (a foreign network: no fused routes)."""
    feature_based = True
    no_warp = True

    def __init__(self, k=3, hw=(6, 8)):
        super().__init__()
        self.k, self.hw, self.calls = k, hw, 0

    def predict(self, frame_prev, frame_next, mvs_left, mvs_right, n, profiler=None, **extra):
        self.calls += 1
        return {"pred": torch.randn((n, self.k) + self.hw, generator=torch.Generator().manual_seed(self.calls))}


def test_predictor_plumbing_with_a_stub_model(monkeypatch):
    """The ops are replaced by the numpy definitions: the simplified rings follow the chunk borders of their own buffers, which are not
    the outlines'; clear_report() drops them, reset() keeps them, and masks and outlines are those of simplify=None."""
    calls = []
    monkeypatch.setattr(ops, "resize_argmax_u8", lambda logits, size: logits.argmax(1).to(torch.uint8))
    monkeypatch.setattr(ops, "mask_regions", lambda mask, classes, connectivity=8: t(rref.mask_regions(mask.numpy(), classes, connectivity)))

    def table(mask, labels, classes, conf=None, low=128, max_regions=1024, out=None):
        got = rref.region_table(mask.numpy(), labels.numpy(), classes, None, low, max_regions)
        out[0].copy_(t(got[0]))
        out[1].copy_(t(got[1]))
        return out[0], out[1], t(got[2])

    def outlines(index, max_regions, connectivity=8, max_contours=4096, max_vertices=32768, out=None):
        for dst, src in zip(out, oref.region_outlines(index.numpy(), max_regions, connectivity, max_contours, max_vertices)):
            dst.copy_(t(src))
        return out

    def simplify(contours, vertices, counts, tolerance, max_rounds=32, out=None):
        calls.append(contours.shape[0])
        for dst, src in zip(out, sref.outline_simplify(contours.numpy(), vertices.numpy(), counts.numpy(), ops.simplify_tol_q(tolerance), max_rounds)):
            dst.copy_(t(src))
        return out

    monkeypatch.setattr(ops, "region_table", table)
    monkeypatch.setattr(ops, "region_outlines", outlines)
    monkeypatch.setattr(ops, "outline_simplify", simplify)
    x, grids = torch.zeros(1, 3, 6, 8), [None] * 2                                                        # windows of three frames
    kw = dict(classes=3, out_size=(6, 8), crop=None, compute_metrics=False, regions=True, connectivity=4, max_regions=20, outlines=True, max_contours=6,
              max_vertices=200)
    on = FlowPredictor(StubFlow(), simplify=0.5, simplify_rounds=3, **kw)
    on.outline_chunk, on.simple_chunk = 4, 5
    off = FlowPredictor(StubFlow(), **kw)
    off.outline_chunk = 4
    kept = [on.predict_window(x, x, grids, grids) for _ in range(3)]
    assert all(np.array_equal(a, off.predict_window(x, x, grids, grids)) for a in kept) and off.simple_outline_report()[0] == []
    assert calls == [3, 1, 1, 1, 2, 1]                                                                    # outlines 3 | 1 + 2 | 2 + 1, simple 3 | 1 + (1 + 1) | 2 + 1
    frames, flags = on.outline_report()
    want_frames, want_flags = off.outline_report()
    assert np.array_equal(flags, want_flags) and all(np.array_equal(a, b) for f, g in zip(frames, want_frames) for a, b in zip(f, g))
    simple, counts = on.simple_outline_report()
    assert len(simple) == 9 and counts.shape == (9, 4) and (counts[:, 3] & 4).any()
    for f in range(9):
        c, v = np.zeros((1, 6, 6), np.int64), np.zeros((1, 200, 2), np.int32)
        c[0, :len(frames[f][0])], v[0, :len(frames[f][1])] = frames[f][0], frames[f][1]
        n = np.array([[len(frames[f][0]) + (2 if flags[f] & 2 else 0), len(frames[f][0]), len(frames[f][1]), flags[f]]], np.int64)
        want = sref.outline_simplify(c, v, n, 4, 3)
        assert counts[f].tolist() == want[2][0].tolist() and np.array_equal(simple[f][0], want[0][0, :len(frames[f][0])])
        assert np.array_equal(simple[f][1], want[1][0, :int(want[2][0, 1])])
    on.reset()
    assert len(on.simple_outline_report()[0]) == 9                                                        # a new video keeps the report
    on.clear_report()
    assert on.simple_outline_report()[0] == [] and on.outline_report()[0] == []
    on.predict_window(x, x, grids, grids)
    assert len(on.simple_outline_report()[0]) == 3 and calls[-1] == 3


def test_tool_takes_the_two_options_and_refuses_simplify_without_outlines(capsys):
    import importlib.util

    spec = importlib.util.spec_from_file_location("predict_video_tool_simplify", os.path.join(ROOT, "tools", "predict_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw = ["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights", "--regions", "r.csv"]
    a = tool.parse_args(raw + ["--outlines", "o.geojson", "--simplify", "1.5", "--simplify-rounds", "64"])
    assert (a.simplify, a.simplify_rounds) == (1.5, 64)
    a = tool.parse_args(raw + ["--outlines", "o.geojson"])
    assert (a.simplify, a.simplify_rounds) == (None, 32)
    capsys.readouterr()
    for bad, word in ((raw + ["--simplify", "1"], "--simplify needs --outlines"),
                      (raw + ["--outlines", "o.geojson", "--simplify", "-1"], "0..256 pixels"),
                      (raw + ["--outlines", "o.geojson", "--simplify", "1", "--simplify-rounds", "0"], "--simplify-rounds")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert word in capsys.readouterr().err, bad
