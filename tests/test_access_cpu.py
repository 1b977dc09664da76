"""Dry-route reachability, the parts that need no GPU: the definition twice in tests/access_ref.py, a heap Dijkstra against a literal
relaxation; csrc/access_defs.h run on the CPU by a stand-alone sanitized host program that walks the frame tile by tile as the kernels
do; the sixteenth hook table and the freeze of the fifteenth; the library's refusals and the argument checks of the Python layers; and
the properties of the definition shown on the reference alone: a diagonal line of water is a wall, a building is never crossed, a larger
bound only adds values, and a route's moves sum to the value it starts from."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import access_ref as aref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import mosaic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc")
NEW = ["mask_access", "region_access"]
COST = [2, 0, 6, 9, 1]


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("case", aref.op_cases(), ids=lambda c: c[0])
def test_the_two_references_agree(case):
    name, m, s, cost, terminal, conn = case
    d, origin, status = aref.case_reference(name)
    for f in range(m.shape[0]):
        d2, o2, converged = aref.relax(m[f], s[f], cost, terminal, conn)
        assert converged and np.array_equal(d[f], d2) and np.array_equal(origin[f], o2), (name, f)
        assert status[f].tolist() == [1, int((d2 != aref.NONE).sum()), 0]
        ok, where = aref.real_routes(m[f], d[f], s[f], cost, terminal, conn)
        assert ok, (name, f, where)
    vals = d[d != aref.NONE]
    if vals.size > 2:
        r = int(np.median(vals))
        if r >= 1:
            dr, orr, _ = aref.case_reference(name, r)
            for f in range(m.shape[0]):
                d2, o2, converged = aref.relax(m[f], s[f], cost, terminal, conn, max_cost=r)   # pruned while it relaxes, not afterwards
                assert converged and np.array_equal(dr[f], d2) and np.array_equal(orr[f], o2), (name, f, r)


def test_the_serpentine_is_one_long_chain():
    m, s, cost, terminal = aref.serpentine()
    d, origin, status = aref.serpentine_reference()
    assert status[0].tolist() == [1, 6288, 0] and (origin[d != aref.NONE] == 0).all()
    assert d[0, 0, 0] == 0 and d[0, 0, 129] == 129 * 10 and d[0, 2, 129] == 131 * 10 and (d[0][m[0] == 1] == aref.NONE).all()
    far = d[0][d[0] != aref.NONE].max()
    assert far == 62870 and far // 10 > 48 * 129                   # every corridor from end to end
    part, _, converged = aref.relax(m[0], s[0], cost, terminal, 8, sweeps=40)
    assert not converged and ((part != aref.NONE) <= (d[0] != aref.NONE)).all() and (part[part != aref.NONE] >= d[0][part != aref.NONE]).all()
    rest, _, converged = aref.relax(m[0], s[0], cost, terminal, 8, start=aref.relax(m[0], s[0], cost, terminal, 8, sweeps=40)[:2])
    assert converged and np.array_equal(rest, d[0])                # going on from unfinished planes ends at the same fixed point


def test_the_cases_hold_what_they_promise():
    names = [c[0] for c in aref.op_cases()]
    t = aref.TILE
    assert t == ops.ACCESS_TILE == 32 and {"1x1", "1x37", "41x1", "70x150x3", "junction"} <= set(names)
    assert {f"{a}x{b}" for a in (t - 1, t, t + 1) for b in (t - 1, t, t + 1)} <= set(names)
    costs = [c[3] for c in aref.op_cases()]
    assert all(1 in c and 255 in c and c[1] == 0 for c in costs[:12])
    _, m, s, cost, terminal, _ = aref.op_cases()[names.index("70x150x3")]
    kinds = aref.pixel_kinds(m, cost, terminal)
    assert ((s[0] != 0) & ~kinds[1][0]).any() and ((s[0] != 0) & kinds[1][0]).any()                  # seeds on barriers and terminals, and valid ones
    assert (s[1] != 0).any() and not ((s[1] != 0) & kinds[1][1]).any() and kinds[1][2].all() and (s[2] != 0).sum() == 1
    assert (m[0] >= 32).any() and (m[0] == 255).any()
    for name in names:
        assert aref.case_reference(name)[2][0, 1] > 0, name


# ------------------------------------------------------------------------------------------------ the properties of the definition
def field(rows, seeds, cost=COST, terminal=(3,), conn=8, max_cost=0):
    m = np.array([[int(ch) for ch in row] for row in rows], np.uint8)
    s = np.zeros_like(m)
    for x, y in seeds:
        s[y, x] = 1
    return m, s, aref.dijkstra(m, s, cost, terminal, conn, max_cost)


def test_a_diagonal_line_of_water_is_a_wall_at_connectivity_8():
    rows = ["00001", "00010", "00100", "01000", "10000"]
    m, s, (d, origin) = field(rows, [(0, 0)])
    upper = np.array([[x + y < 4 for x in range(5)] for y in range(5)])
    assert (d[upper] != aref.NONE).all() and (d[~upper] == aref.NONE).all() and (origin[~upper] == -1).all()
    assert d[0, 1] == 5 * 4 and d[1, 1] == 7 * 4 and d[2, 1] == 7 * 4 + 5 * 4
    # one water pixel less: everything behind the line is reached through the gap, and no corner beside it is cut
    rows[2] = "00000"
    m, s, (d, origin) = field(rows, [(0, 0)])
    assert (d[m == 0] != aref.NONE).all() and d[2, 2] == 2 * 7 * 4 and d[3, 3] == 3 * 7 * 4 and d[2, 3] == d[3, 2] == d[2, 2] + 5 * 4
    below = np.array([[x + y > 4 for x in range(5)] for y in range(5)])
    assert d[below].min() == d[2, 2] + 5 * 4 and d[1, 4] == d[2, 3] + 2 * 5 * 4 > d[2, 3] + 7 * 4   # (4, 1) around the corner of the water at (3, 1), not across it
    m, s, (d4, _) = field(rows, [(0, 0)], conn=4)
    assert (d4[m == 0] != aref.NONE).all() and d4[2, 2] == 4 * 5 * 4


def test_a_building_is_arrived_at_and_never_crossed():
    rows = ["11111111111",
            "14444344441",
            "11111111111"]
    m, s, (d, origin) = field(rows, [(1, 1)])
    assert d[1, 4] == 3 * 10 and d[1, 5] == 3 * 10 + 5 * (1 + 9) and (d[1, 6:10] == aref.NONE).all()   # two streets joined only through a building stay apart
    m, s, (d, origin) = field(rows, [(5, 1)])                         # a seed on a terminal pixel is ignored
    assert (d == aref.NONE).all() and (origin == -1).all()
    m, s, (d, origin) = field(rows, [(1, 1), (9, 1)])
    assert d[1, 5] == 3 * 10 + 50 and origin[1, 5] == 1 * 11 + 1 and origin[1, 6] == 1 * 11 + 9      # reached from both sides: the lower index names it
    m, s, (d, _) = field(rows, [(1, 1)], cost=[2, 0, 6, 0, 1])        # a terminal class without a cost is a barrier
    assert d[1, 5] == aref.NONE
    m, s, (d, _) = field(rows, [(1, 1)], terminal=())                 # not terminal: crossed at its cost
    assert d[1, 6] == 30 + 50 + 50


def test_raising_the_bound_only_adds_values():
    name, m, s, cost, terminal, conn = [c for c in aref.op_cases() if c[0] == "speckle 66x97"][0]
    full = aref.case_reference(name)[0][0]
    vals = np.sort(full[full != aref.NONE])
    last = None
    for r in (1, int(vals[len(vals) // 4]), int(vals[len(vals) // 2]), int(vals[-1]), aref.MAX_COST):
        d, origin = aref.dijkstra(m[0], s[0], cost, terminal, conn, r)
        assert np.array_equal(d != aref.NONE, full <= r) and np.array_equal(d[d != aref.NONE], full[d != aref.NONE]) and ((origin == -1) == (d == aref.NONE)).all()
        if last is not None:
            assert ((last != aref.NONE) <= (d != aref.NONE)).all()
        last = d
    assert np.array_equal(last, full)


def test_a_routes_moves_sum_to_the_value_it_starts_from():
    for name in ("70x150x3", "speckle 66x97", "junction"):
        _, m, s, cost, terminal, conn = [c for c in aref.op_cases() if c[0] == name][0]
        d, origin, _ = aref.case_reference(name)
        ys, xs = np.nonzero(d[0] != aref.NONE)
        report = dict(cls=m[0], d=d[0], cost=aref.cost_table(cost), terminal=terminal, connectivity=conn, converged=True)
        for i in range(0, len(ys), max(1, len(ys) // 40)):
            x, y = int(xs[i]), int(ys[i])
            chain = aref.access_route(d[0], m[0], cost, terminal, conn, x, y)
            assert chain[0] == (x, y) and d[0][chain[-1][1], chain[-1][0]] == 0 and s[0][chain[-1][1], chain[-1][0]] != 0
            assert aref.route_cost(chain, m[0], cost) == d[0, y, x]
            assert mosaic.access_route(report, x, y) == chain         # the package's backtrack is the reference's
        nx, ny = (int(v) for v in np.argwhere(d[0] == aref.NONE)[0][::-1])
        with pytest.raises(ValueError, match="has no value"):
            mosaic.access_route(report, nx, ny)
    with pytest.raises(ValueError, match="has not converged"):
        mosaic.access_route(dict(report, converged=False), x, y)


def test_the_river_scene_on_the_reference():
    seeds = np.zeros((1,) + aref.SCENE, np.uint8)
    seeds[0, aref.SCENE_SEED[1], aref.SCENE_SEED[0]] = 1
    for cut in (False, True):
        cls = aref.scene_classes(cut)
        d, origin, _ = aref.mask_access(cls[None], seeds, aref.SCENE_COST, (3,), 8)
        for boxes, reached in ((aref.NEAR_BUILDINGS, True), (aref.FAR_BUILDINGS, not cut)):
            for y0, x0, y1, x1 in boxes:
                assert (cls[y0:y1, x0:x1] == 3).all() and (d[0, y0:y1, x0:x1] != aref.NONE).any() == reached, (cut, y0, x0)
        assert (d[0][cls == 255] == aref.NONE).all() and (d[0][cls == 1] == aref.NONE).all()
    assert (aref.scene_classes(True) != aref.scene_classes(False)).sum() == 3
    votes = aref.scene_votes()
    assert votes.dtype == np.uint16 and np.array_equal(np.where(votes.sum(0) > 0, votes.argmax(0), 255), aref.scene_classes())


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def host_commands():
    """(commands, expected output lines) for tests/access_host_check.cpp, from the reference."""
    cmds, want = [], []
    flat = lambda a: [int(v) for v in np.asarray(a).reshape(-1)]  # noqa: E731
    runs = [(c, 0, 1, 128) for c in aref.op_cases() if c[0] != "70x150x3 conn4"]
    runs += [(c, "median", 1, 128) for c in aref.op_cases() if c[0] in ("33x33", "speckle 66x97")]
    runs += [(c, 0, 0, 128) for c in aref.op_cases() if c[0] == "31x32"]
    runs.append((("serpentine",) + aref.serpentine() + (8,), 0, 1, 256))
    for (name, m, s, cost, terminal, conn), r, want_origin, rounds in runs:
        full = aref.mask_access(m, s, cost, terminal, conn)
        if r == "median":
            r = int(np.median(full[0][full[0] != aref.NONE]))
        d, origin, status = aref.mask_access(m, s, cost, terminal, conn, r) if r else full
        for f in range(m.shape[0]):
            head = ["field", m.shape[1], m.shape[2], conn, r, want_origin, rounds, aref.class_set(terminal)] + aref.cost_table(cost)
            cmds.append(" ".join(str(v) for v in head + flat(m[f]) + flat(s[f])))
            org = origin[f] if want_origin else np.where(origin[f] < 0, -1, 0)
            want.append(" ".join(str(v) for v in [1, int(status[f, 1])] + flat(d[f]) + flat(org)))
    return cmds, want


def test_the_headers_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/access_defs.h is plain __host__ __device__ C++: tests/access_host_check.cpp relaxes every case tile by tile, with the ring,
    the sweep cap and the dirty marks of the kernels, as a stand-alone program built with -fsanitize=address,undefined; every line it
    prints is the reference's, the serpentine within 256 rounds included."""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "access_host_check"), str(tmp_path / "commands.txt")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tests", "access_host_check.cpp"), "-o", exe]
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
    assert len(got) == len(want) and len(want) >= 20
    for cmd, g, w in zip(cmds, got, want):
        assert g == w, (cmd[:120], g[:200], w[:200])


def test_the_rules_are_written_once():
    defs = open(os.path.join(CSRC, "access_defs.h")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", defs).lower().replace("__hipcc__", "")
    kernel = open(os.path.join(CSRC, "access_ops.hip")).read()
    assert all(f"acc::{fn}(" in kernel for fn in ("move_cost", "offer", "better", "seed_key", "plane_key", "kind_of", "bound_of", "key_cost", "key_origin", "make_key"))
    code = re.sub(r"//[^\n]*", "", kernel.split("namespace fs {")[1])
    assert "asm" not in code and "hipMemset" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert re.search(r"for \(int sweep = 0; sweep < SWEEPS; \+\+sweep\)", code) and "while (true)" not in code and "for (;;)" not in code
    assert " access_ops.hip " in open(os.path.join(CSRC, "Makefile")).read()
    header = open(os.path.join(ROOT, "include", "floodseg_test.h")).read()
    assert int(re.search(r"#define FS_ACCESS_TILE (\d+)", header).group(1)) == ops.ACCESS_TILE == int(re.search(r"constexpr int T = (\d+);", kernel).group(1))
    assert int(re.search(r"#define FS_ACCESS_MAX_COST (0x[0-9A-Fa-f]+)u", header).group(1), 16) == ops.ACCESS_MAX_COST == aref.MAX_COST == 2 ** 31 - 4096
    assert int(re.search(r"#define FS_ACCESS_NONE (0x[0-9A-Fa-f]+)u", header).group(1), 16) == ops.ACCESS_NONE == aref.NONE
    assert mosaic.ACCESS_MOVES == aref.MOVES
    for n, h, w in ((1, 1, 1), (3, 70, 150), (2, 4096, 4096), (1, 33, 31)):
        tiles = -(-h // 32) * -(-w // 32)
        assert ops.mask_access_workspace_bytes(n, h, w) == n * h * w * 8 + n * tiles * 8 + n * 16


# ------------------------------------------------------------------------------------------------ library surface
def test_the_sixteenth_table_and_the_freeze_of_the_fifteenth():
    assert _lib.ext15_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext15_api {"):text.index("} fs_ext15_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == NEW
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables14;") < text.index("typedef struct fs_ext15_api {") < text.index("typedef struct fs_hook_tables15 {")
    tables15 = text[text.index("typedef struct fs_hook_tables15 {"):text.index("} fs_hook_tables15;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables15) == [("fs_hook_tables14", "base14"), ("fs_ext15_api", "ext15")]
    assert int(re.search(r"#define FS_EXT15_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT15_MAGIC == int.from_bytes(b"FSEXTA15", "big")
    # fs_ext14_api is frozen: the header and the binding name the same one member, 24 bytes
    frozen = text[text.index("typedef struct fs_ext14_api {"):text.index("} fs_ext14_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", frozen) == _lib.ext14_hook_names() == ["mosaic_change"]
    assert ctypes.sizeof(_lib.FsExt14Api) == 24
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables15 all15 = {all14, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT15_MAGIC," in init and "sizeof(fs_ext15_api)," in init
    assert re.search(r"const fs_hook_tables14& all14 = all15\.base14;\s+const fs_hook_tables13& all13 = all14\.base13;", src)
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    assert "launch_mask_access" in kernels and "launch_region_access" in kernels
    # the fifteen older tables and the export list are what they were
    assert [len(names()) for names in (_lib.hook_names, _lib.ext_hook_names, _lib.ext2_hook_names, _lib.ext3_hook_names, _lib.ext4_hook_names, _lib.ext5_hook_names,
                                       _lib.ext6_hook_names, _lib.ext7_hook_names, _lib.ext8_hook_names, _lib.ext9_hook_names, _lib.ext10_hook_names,
                                       _lib.ext11_hook_names, _lib.ext12_hook_names, _lib.ext13_hook_names, _lib.ext14_hook_names)] == [38, 2, 14, 1, 1, 1, 1, 2, 4, 2, 3, 1, 5, 6, 1]
    assert not any("fs_" + name in _lib.exported_symbols() for name in NEW) and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    public = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(name in public for name in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables15.ext15.offset == ctypes.sizeof(_lib.FsHookTables14)                         # directly behind, no padding
    assert [getattr(_lib.FsExt15Api, name).offset for name in NEW] == [16, 24] and ctypes.sizeof(_lib.FsExt15Api) == 32
    all15 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables15)).contents
    assert all15.base14.ext14.magic == _lib.EXT14_MAGIC and all15.base14.ext14.size == 24                 # frozen: exactly, not from below
    assert all15.base14.base13.ext13.magic == _lib.EXT13_MAGIC and all15.base14.base13.ext13.size == 64
    assert all15.ext15.magic == _lib.EXT15_MAGIC and all15.ext15.size >= 32                               # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all15.ext15, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                                            # a table member, not an exported symbol
    assert ctypes.cast(all15.base14.ext14.mosaic_change, ctypes.c_void_p).value == ctypes.cast(lib.fs_mosaic_change, ctypes.c_void_p).value


def test_the_magic_is_checked_before_use(monkeypatch):
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT15_MAGIC", _lib.EXT15_MAGIC + 1)
    with pytest.raises(RuntimeError, match="the library has no fifteenth extension table \\(fs_mask_access is missing\\)"):
        fresh.fs_mask_access
    assert fresh.fs_mosaic_change is not None                                 # the tables in front of it stay usable
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT14_MAGIC", _lib.EXT14_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first fifteen hook tables are not the ones this binding knows \\(fs_region_access is missing\\)"):
        fresh.fs_region_access
    monkeypatch.undo()
    assert fresh.fs_mask_access is not None and fresh.fs_region_access is not None


P = 0x10000  # a dummy non-null pointer, aligned to 64 KiB: every call below must be refused before anything is launched


def call_field(lib, **kw):
    a = dict(mask=P, seeds=P, n=1, H=64, W=96, cost=[2, 0, 6, 9, 1], terminal_set=8, connectivity=8, max_cost=0, rounds=4, resume=0, d=P, origin=P, status=P,
             workspace=P)
    a.update(kw)
    cost = None if a["cost"] is None else (ctypes.c_uint8 * 32)(*(list(a["cost"]) + [0] * (32 - len(a["cost"]))))
    return lib.fs_mask_access(a["mask"], a["seeds"], a["n"], a["H"], a["W"], None if cost is None else ctypes.cast(cost, ctypes.c_void_p), a["terminal_set"],
                              a["connectivity"], a["max_cost"], a["rounds"], a["resume"], a["d"], a["origin"], a["status"], a["workspace"], None)


def call_table(lib, **kw):
    a = dict(mask=P, d=P, origin=P, index=P, counts=P, n=1, H=64, W=96, K=5, max_regions=64, reach=P, rows=P)
    a.update(kw)
    return lib.fs_region_access(a["mask"], a["d"], a["origin"], a["index"], a["counts"], a["n"], a["H"], a["W"], a["K"], a["max_regions"], a["reach"], a["rows"], None)


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    field_cases = [(dict(mask=None), b"null"), (dict(seeds=None), b"null"), (dict(cost=None), b"null"), (dict(d=None), b"null"), (dict(status=None), b"null"),
                   (dict(workspace=None), b"null"), (dict(n=0), b"n=0"), (dict(n=65536), b"n=65536"), (dict(H=0), b"0x96"), (dict(W=0), b"64x0"),
                   (dict(H=32769), b"32769"), (dict(W=32769), b"32769"), (dict(H=32768, W=65536), b"2^31"), (dict(connectivity=6), b"got 6"),
                   (dict(connectivity=0), b"got 0"), (dict(max_cost=2 ** 31 - 4095), b"2147479553"), (dict(max_cost=0xFFFFFFFF), b"4294967295"),
                   (dict(rounds=0), b"rounds=0"), (dict(rounds=65536), b"rounds=65536"), (dict(resume=2), b"got 2"), (dict(d=P + 2), b"d is not aligned"),
                   (dict(origin=P + 1), b"origin is not aligned"), (dict(status=P + 2), b"status is not aligned"), (dict(workspace=P + 4), b"workspace is not aligned"),
                   (dict(cost=[0] * 32), b"all zero"), (dict(cost=[]), b"all zero")]
    for kw, word in field_cases:
        assert call_field(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert msg.startswith(b"mask_access:") and word in msg, (kw, msg)
    table_cases = [(dict(mask=None), b"null"), (dict(d=None), b"null"), (dict(index=None), b"null"), (dict(counts=None), b"null"), (dict(reach=None), b"null"),
                   (dict(rows=None), b"null"), (dict(n=0), b"n=0"), (dict(H=0), b"0x96"), (dict(W=40000), b"40000"), (dict(K=0), b"classes=0"),
                   (dict(K=256), b"classes=256"), (dict(max_regions=0), b"max_regions=0"), (dict(max_regions=65537), b"65537"), (dict(d=P + 2), b"aligned to 4"),
                   (dict(origin=P + 2), b"aligned to 4"), (dict(index=P + 1), b"aligned to 4"), (dict(counts=P + 4), b"aligned to 8"),
                   (dict(reach=P + 4), b"aligned to 8"), (dict(rows=P + 4), b"aligned to 8")]
    for kw, word in table_cases:
        assert call_table(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert msg.startswith(b"region_access:") and word in msg, (kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
def test_the_ops_refuse_with_the_offending_value():
    mask, seeds = torch.zeros((2, 40, 50), dtype=torch.uint8), torch.zeros((2, 40, 50), dtype=torch.uint8)
    good = dict(mask=mask, seeds=seeds, cost=COST)
    planes = (torch.zeros((2, 40, 50), dtype=torch.int32), torch.zeros((2, 40, 50), dtype=torch.int32))
    for kw, word in ((dict(mask=mask.int()), "int32"), (dict(mask=mask[0]), "(40, 50)"), (dict(seeds=seeds[:1]), "(1, 40, 50)"), (dict(seeds=seeds.bool()), "bool"),
                     (dict(cost=[0, 0, 0]), "all zero"), (dict(cost={5: 256}), "256"), (dict(cost={32: 1}), "32"), (dict(terminal=(32,)), "[32]"),
                     (dict(connectivity=6), "got 6"), (dict(max_cost=-1), "-1"), (dict(max_cost=2 ** 31 - 4095), "2147479553"), (dict(rounds=0), "got 0"),
                     (dict(rounds=65536), "65536"), (dict(resume=planes, out=planes), "not both"), (dict(resume=(planes[0], None)), "exactly when want_origin"),
                     (dict(out=(planes[0][:1], planes[1])), "(1, 40, 50)"), (dict(out=(planes[0].long(), planes[1])), "int64"),
                     (dict(want_origin=False, out=planes), "exactly when want_origin")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.mask_access(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.mask_access: tensors must live on the GPU"):
        ops.mask_access(**good)
    d, index, counts = planes[0], planes[1], torch.zeros((2, 2), dtype=torch.int64)
    good = dict(mask=mask, d=d, origin=planes[1], index=index, counts=counts, classes=5, max_regions=64)
    for kw, word in ((dict(mask=mask.int()), "int32"), (dict(d=d.long()), "int64"), (dict(d=None), "None"), (dict(index=index[:1]), "(1, 40, 50)"),
                     (dict(origin=planes[1][:, :3]), "(2, 3, 50)"), (dict(counts=counts[:1]), "(1, 2)"), (dict(counts=counts.int()), "int32"), (dict(classes=0), "got 0"),
                     (dict(classes=256), "256"), (dict(max_regions=0), "and 0"), (dict(max_regions=65537), "65537"),
                     (dict(out=(torch.zeros((2, 5, 4), dtype=torch.int64), torch.zeros((2, 63, 8), dtype=torch.int64))), "[2,64,8]")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.region_access(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.region_access: tensors must live on the GPU"):
        ops.region_access(**good)
    ops.region_access.__doc__ and ops.mask_access.__doc__
    assert "guess" in ops.mask_access.__doc__ and "guesses, not validated on real video" in mosaic.mosaic_access.__doc__
    assert mosaic.ACCESS_COST == aref.SCENE_COST == {4: 1, 0: 2, 2: 6, 3: 2} and mosaic.ACCESS_TERMINAL == (3,)
    assert ops.access_cost_table(mosaic.ACCESS_COST) == [2, 0, 6, 2, 1] + [0] * 27


def test_the_helper_refuses_before_anything_is_enqueued():
    part = dict(votes=torch.from_numpy(aref.scene_votes().view(np.int16).copy()).view(torch.uint16))
    for kw, word in ((dict(min_votes=0), "got 0"), (dict(cost={1: 300}), "300"), (dict(cost={}), "all zero"), (dict(terminal=(40,)), "[40]"), (dict(connectivity=5), "got 5"),
                     (dict(chunk=0), "got 0 and"), (dict(max_rounds=0), "and 0"), (dict(roundz=3), "['roundz']")):
        with pytest.raises(ValueError, match=re.escape(word)):
            mosaic.mosaic_access(part, **kw)
    with pytest.raises(RuntimeError, match="tensors must live on the GPU"):    # past the helper's own checks: the first op refuses CPU tensors
        mosaic.mosaic_access(part)
    cls = torch.from_numpy(aref.scene_classes())
    for seeds, word in (("edge", "'edge'"), ({}, "{}"), (dict(point=[(1, 1)]), "point"), (dict(points=[(160, 5)]), "(160, 5)"), (dict(points=[(5, -1)]), "(5, -1)"),
                        (dict(classes=(33,)), "[33]")):
        with pytest.raises(ValueError, match=re.escape(word)):
            mosaic.access_seeds(cls, seeds)
    plane = mosaic.access_seeds(cls, dict(points=[(5, 60)], classes=(3,), border=True))     # the seed planes are plain tensor code: they run anywhere
    assert plane.dtype == torch.uint8 and plane[60, 5] == 1 and plane[3, 2] == 1 and plane[2, 2] == 0 and bool((plane[cls == 3] == 1).all()) and plane[50, 50] == 0
    from flood_uav_video_segmentation_amd.flow.mosaic import MosaicBuilder
    with pytest.raises(ValueError, match="mosaic_part\\(\\) needs mosaic="):
        MosaicBuilder((30, 40)).access()


def reference_report(cut):
    """access_report()'s dict from the reference alone: regions by scipy-free flood fill are not needed -- one region per building box."""
    cls = aref.scene_classes(cut)
    seeds = np.zeros((1,) + aref.SCENE, np.uint8)
    seeds[0, aref.SCENE_SEED[1], aref.SCENE_SEED[0]] = 1
    d, origin, _ = aref.mask_access(cls[None], seeds, aref.SCENE_COST, (3,), 8)
    boxes = aref.NEAR_BUILDINGS + aref.FAR_BUILDINGS
    index = np.full(aref.SCENE, -1, np.int32)
    table = np.zeros((len(boxes), 10), np.int64)
    for r, (y0, x0, y1, x1) in enumerate(boxes):
        index[y0:y1, x0:x1] = r
        ys, xs = np.mgrid[y0:y1, x0:x1]
        table[r, :8] = (3, ys.size, x0, y0, x1 - 1, y1 - 1, xs.sum(), ys.sum())
    counts = np.array([[len(boxes), len(boxes)]], np.int64)
    reach, rows = aref.region_access(cls[None], d, origin, index[None], counts, 5, 16)
    return dict(cls=cls, d=d[0], origin=origin[0], status=np.array([1, 0, int((d != aref.NONE).sum()), 0], np.int32), converged=True, rounds=64, table=table,
                rows=rows[0, :len(boxes)], reach=reach[0], index=index, cost=aref.cost_table(aref.SCENE_COST), terminal=(3,), connectivity=8, classes=5)


def test_the_writers_on_the_reference(tmp_path):
    import json

    report = reference_report(cut=True)
    path = str(tmp_path / "a.csv")
    mosaic.write_access_csv(path, report, class_names=["bg", "water", "tree", "building", "street"])
    lines = open(path).read().split("\n")
    assert lines == aref.access_csv_lines(report["table"], 7, report["rows"], True, ["bg", "water", "tree", "building", "street"])
    assert lines[0] == "region,class,area,centroid_x,centroid_y,state,cost,at_x,at_y,origin_x,origin_y,origin_region"
    assert [line.split(",")[5] for line in lines[1:-1]] == ["reached"] * 3 + ["cut_off"] * 4 and lines[4].endswith("cut_off,,,,,,")
    assert lines[1].split(",")[1:5] == ["building", "96", "15.50", "13.50"] and lines[1].split(",")[9:] == ["5", "60", ""]    # the seed lies in no region
    mosaic.write_access_csv(path, dict(report, converged=False))
    assert [line.split(",")[5] for line in open(path).read().split("\n")[1:-1]] == ["reached_bound"] * 3 + ["not_reached_yet"] * 4
    mosaic.write_access_geojson(str(tmp_path / "a.geojson"), report)
    doc = json.load(open(str(tmp_path / "a.geojson")))
    assert [f["properties"]["region"] for f in doc["features"]] == [0, 1, 2] and all(f["geometry"]["type"] == "LineString" for f in doc["features"])
    for f in doc["features"]:
        line = f["geometry"]["coordinates"]
        assert line[-1] == [aref.SCENE_SEED[0] + 0.5, aref.SCENE_SEED[1] + 0.5] and line[0] == [report["rows"][f["properties"]["region"], 1] + 0.5,
                                                                                               report["rows"][f["properties"]["region"], 2] + 0.5]
    image = mosaic.access_image(report)
    assert image.shape == aref.SCENE + (3,) and image.dtype == np.uint8
    y0, x0, y1, x1 = aref.FAR_BUILDINGS[0]
    assert (image[y0:y1, x0:x1] == mosaic.ACCESS_CUT_OFF).all() and not (image[10:18, 10:22] == mosaic.ACCESS_CUT_OFF).all(-1).any()
    assert (image[0, 0] == 0).all() and tuple(image[aref.SCENE_SEED[1], aref.SCENE_SEED[0]]) == ops.FLOOD_PALETTE[4]       # unseen: the fill; the seed: its class colour
    mosaic.write_access_png(str(tmp_path / "a.png"), report)
    from PIL import Image
    assert np.array_equal(np.array(Image.open(str(tmp_path / "a.png"))), image)
    with pytest.raises(ValueError, match="has no regions"):
        mosaic.write_access_csv(path, dict(report, table=None))


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name.replace(".py", "_tool_access"), os.path.join(ROOT, "tools", name))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_argument_checks(capsys):
    tool = load_tool("mosaic_access.py")
    a = tool.parse_args(["p.npz", "--csv", "a.csv", "--png", "a.png", "--routes", "r.geojson", "--seed-point", "5", "60", "--seed-point", "7", "8", "--seed-class", "4",
                         "--cost", "4=1", "0=3", "--terminal", "3", "--min-votes", "2", "--connectivity", "4", "--max-cost", "5000", "--max-rounds", "512",
                         "--max-regions", "2048"])
    assert (a.part, a.csv, a.png, a.routes, a.seed_point, a.seed_class, a.seed_border) == ("p.npz", "a.csv", "a.png", "r.geojson", [[5, 60], [7, 8]], [4], False)
    assert (a.cost, a.terminal, a.min_votes, a.connectivity, a.max_cost, a.max_rounds, a.max_regions) == ({4: 1, 0: 3}, [3], 2, 4, 5000, 512, 2048)
    d = tool.parse_args(["p.npz", "--csv", "a.csv"])
    assert (d.seed_point, d.seed_class, d.seed_border, d.cost, d.terminal, d.connectivity, d.max_cost, d.max_rounds) == (None, None, True, None, [3], 8, 0, mosaic.ACCESS_MAX_ROUNDS)
    assert tool.seed_spec(d) == dict(border=True) and tool.seed_spec(a) == dict(points=[(5, 60), (7, 8)], classes=[4])
    capsys.readouterr()
    base = ["p.npz", "--csv", "a.csv"]
    for bad, word in ((["p.npz"], "--csv, --png or --routes"), (base + ["--connectivity", "6"], "4 or 8"), (base + ["--cost", "4:1"], "K=COST"),
                      (base + ["--cost", "4=256"], "0..255"), (base + ["--cost", "40=1"], "0..31"), (base + ["--min-votes", "0"], "1..65535"),
                      (base + ["--max-cost", "-1"], "--max-cost"), (base + ["--max-rounds", "0"], "--max-rounds"), (["--csv", "a.csv"], "PART.npz")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert word in capsys.readouterr().err, bad
