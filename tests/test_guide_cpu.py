"""The matcher's vectors guided by the camera model, the parts that need no GPU: the definition in numpy (tests/guide_ref.py) in its
vectorised form against the literal loops; csrc/guide_defs.h run on the CPU by a stand-alone sanitized host program; the four
consequences of the definition; the twelfth hook table and the freeze of the eleventh; the library's and the op's refusals; and the host
logic of GridEstimator(guide=...) and the datasets on stubs."""
import contextlib
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import guide_ref as gref
import mosaic_ref as mref
import motion_ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import dataset, motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc")
NEW = ["guide_vectors"]
ONE = gref.ONE
SIZES = [(64, 96), (70, 100), (16, 16), (176, 240)]
OUTLIERS = [None, 0, 1.0, 2.5]


def rows(models):
    return np.array(models, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("size", SIZES)
def test_vectorised_equals_the_loop_on_adversarial_tables(size):
    fh, fw = size
    seen = np.zeros(8, np.int64)
    for seed, (name, M) in enumerate(gref.models(fh, fw).items()):
        tables = np.stack([gref.adversarial_table(M, fh, fw, 10 * seed + k) for k in range(2)])
        model = rows([M, M])
        for fill_void in (0, 1):
            for outlier in OUTLIERS:
                oq = gref.outlier_q20(outlier)
                a, b = gref.guide_vectors(tables, model, fh, fw, fill_void, oq), gref.guide_vectors_loop(tables, model, fh, fw, fill_void, oq)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, fill_void, outlier)
                assert (a[1][:, 4] + a[1][:, 5] + a[1][:, 6] == a[1][:, 3]).all() and (a[1][:, 2] <= a[1][:, 1]).all()
                seen += a[1].sum(0)
    if size != (16, 16):
        assert (seen[[0, 1, 2, 3, 4, 5, 7]] > 0).all()          # every kind of row and every decision without evidence has occurred


def test_rows_of_each_class_by_hand():
    cx, cy = 40, 24
    assert gref.classify(gref.VOID_ROW, cx, cy) == (gref.ROW_VOID, 0, 0)
    assert gref.classify([-1, 16, 16, -1, 24, 40, 24], cx, cy)[0] == gref.ROW_VOID and gref.classify([-1, 16, 16, 40, 24, 40, -1], cx, cy)[0] == gref.ROW_VOID
    assert gref.classify([-1, 16, 16, 72, -8, 40, 24], cx, cy) == (gref.ROW_VECTOR, 32, -32)                # exactly +-32: a vector
    assert gref.classify([-1, 16, 16, 73, 24, 40, 24], cx, cy)[0] == gref.ROW_FOREIGN and gref.classify([-1, 16, 16, 40, -9, 40, 24], cx, cy)[0] == gref.ROW_FOREIGN
    assert gref.classify([-1, 16, 16, 56, 24, 56, 24], cx, cy)[0] == gref.ROW_FOREIGN                         # another block's row
    assert gref.classify([0, 0, 0, gref.I32_MAX, gref.I32_MIN, 0, gref.I32_MAX], cx, cy)[0] == gref.ROW_FOREIGN  # differences in 64 bits
    M = gref.shift_model(3, -2)
    assert gref.predict(M, cx, cy) == (3 * ONE, -2 * ONE, 3, -2)
    assert gref.available(3, -2, 40, 24, 64, 96) and not gref.available(3, -2, 40, 8, 64, 96) and not gref.available(33, 0, 40, 24, 640, 960)
    assert gref.available(8, 0, 88, 24, 64, 104) and not gref.available(9, 0, 88, 24, 64, 104)              # the window ends at the frame's edge
    assert not gref.pair_guides(gref.garbage_model()) and not gref.pair_guides(gref.shift_model(0, 0, status=2)) and gref.pair_guides(M)


@pytest.mark.parametrize("outlier", [0, 1.0, 2.5])
def test_a_deviation_of_exactly_the_bound_is_no_outlier_and_one_more_is(outlier):
    oq = gref.outlier_q20(outlier)
    outl, edge, table = gref.deviation_case(64, 96, oq)
    for fn in (gref.guide_vectors, gref.guide_vectors_loop):
        out, counts = fn(table[None], rows([edge]), 64, 96, 1, oq)
        assert np.array_equal(out[0], table) and counts[0].tolist() == [24, 0, 0, 0, 0, 0, 0, 0]
        out, counts = fn(table[None], rows([outl]), 64, 96, 1, oq)
        assert counts[0, 3] == 24 and counts[0, 4] + counts[0, 5] == 24 and not np.array_equal(out[0], table)


def test_vectorised_equals_the_loop_with_evidence():
    for channels, size in ((1, (64, 96)), (3, (66, 98))):
        fh, fw = size
        cur, ref = gref.evidence_scene(fh, fw, channels)
        table, cost = motion_ref.block_match(cur, ref, search=8, penalty=2)
        M = gref.shift_model(3, -2)
        for bias in (0, 700, 65535):
            a = gref.guide_vectors(table[None], rows([M]), fh, fw, 1, 0, cur[None], ref[None], cost[None], 2, bias)
            b = gref.guide_vectors_loop(table[None], rows([M]), fh, fw, 1, 0, cur[None], ref[None], cost[None], 2, bias)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[1][0, 6] == 0 and b[1][0, 4] == b[1][0, 3] - b[1][0, 5]   # at the largest bias nothing is kept by evidence


# ------------------------------------------------------------------------------------------------ the four consequences
@pytest.mark.parametrize("size", SIZES[:3])
def test_the_four_consequences(size):
    fh, fw = size
    for seed, (name, M) in enumerate(gref.models(fh, fw).items()):
        table = gref.adversarial_table(M, fh, fw, 100 + seed)[None]
        model = rows([M])
        # 1. nothing to fill and no outlier rule: a copy
        out, counts = gref.guide_vectors(table, model, fh, fw, 0, -1)
        assert np.array_equal(out, table) and counts[0, 2:7].tolist() == [0] * 5
        # 2. a model with status != 0 (or outside the pair bounds) is a copy, whatever is asked
        if not gref.pair_guides(M):
            out, counts = gref.guide_vectors(table, model, fh, fw, 1, 0)
            assert np.array_equal(out, table) and counts[0, 2:7].tolist() == [0] * 5
        # 3. without evidence the op is idempotent: a second pass changes nothing and fills nothing
        for outlier in OUTLIERS:
            oq = gref.outlier_q20(outlier)
            once, _ = gref.guide_vectors(table, model, fh, fw, 1, oq)
            twice, counts = gref.guide_vectors(once, model, fh, fw, 1, oq)
            assert np.array_equal(once, twice) and counts[0, 2] == 0 and counts[0, 5] == 0, (name, outlier)
        # 4. the rounded model vectors are no outliers from half a pixel on
        if gref.pair_guides(M):
            own = gref.model_table(M, fh, fw)[None]
            for oq in (ONE // 2, ONE, 64 * ONE):
                out, counts = gref.guide_vectors(own, model, fh, fw, 1, oq)
                assert counts[0, 3] == 0 and np.array_equal(out, own), (name, oq)


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def host_commands():
    """(commands, expected output lines) for tests/guide_host_check.cpp, from the numpy reference."""
    cmds, want = [], []

    def add(cmd, out):
        cmds.append(" ".join(str(int(v)) if not isinstance(v, str) else v for v in cmd))
        want.append(" ".join(str(int(v)) for v in out))

    fh, fw = 70, 100
    models = gref.models(fh, fw)
    big = gref.model_of([2 * ONE, -2 * ONE, (1 << 36) - 1, -2 * ONE, 2 * ONE, -(1 << 36) + 1], inv=[2 * ONE, 2 * ONE, (1 << 36) - 1, 2 * ONE, 2 * ONE, 1 - (1 << 36)])
    over = gref.model_of([2 * ONE + 1, 0, 0, 0, ONE, 0])
    for M in list(models.values()) + [big, over]:
        for cx, cy in ((8, 8), (88, 56), (16376, 16376)):
            add(["predict"] + list(M) + [cx, cy], [1] + list(gref.predict(M, cx, cy)) if gref.pair_guides(M) else [0, 0, 0, 0, 0])
    for pdx, pdy, cx, cy in ((0, 0, 8, 8), (-1, 0, 8, 8), (0, -1, 8, 8), (32, 32, 40, 24), (33, 0, 40, 24), (0, -33, 40, 40), (4, 6, 88, 56), (5, 6, 88, 56),
                             (4, 7, 88, 56), (-32, -32, 40, 40), (1 << 18, -(1 << 18), 40, 40)):
        add(["avail", pdx, pdy, cx, cy, fh, fw], [int(gref.available(pdx, pdy, cx, cy, fh, fw))])
    rng = np.random.RandomState(3)
    for name, M in models.items():
        table = gref.adversarial_table(M, fh, fw, 7)
        cx, cy = gref.centres(fh, fw)
        for i, r in enumerate(table):
            add(["class"] + list(r) + [cx[i], cy[i]], gref.classify(r, int(cx[i]), int(cy[i])))
            for fill_void, oq in ((1, ONE), (0, 0), (1, -1)):
                for has_ev in (0, 1):
                    sad, penalty, cost, bias = int(rng.randint(0, 65281)), int(rng.randint(0, 256)), int(rng.choice([0, 500, 40000, gref.I32_MAX, gref.I32_MIN])), int(
                        rng.choice([0, 300, 65535]))
                    ev = (lambda pdx, pdy: sad + penalty * (abs(pdx) + abs(pdy)) <= cost + bias) if has_ev else None
                    decision, row, outlier, cls = gref.decide_row(r, M, gref.pair_guides(M), int(cx[i]), int(cy[i]), fh, fw, fill_void, oq, ev)
                    add(["row", fh, fw, fill_void, oq, has_ev, sad, penalty, cost, bias] + list(M) + [cx[i], cy[i]] + list(r), [decision, cls, int(outlier)] + row)
    for dx, dy, gx, gy, oq in ((2, -1, 2 * ONE + 5, -ONE, 5), (2, -1, 2 * ONE + 6, -ONE, 5), (2, -1, 2 * ONE, -ONE - 6, 5), (32, -32, -(1 << 38), 1 << 38, 64 * ONE),
                               (0, 0, 1, 0, 0), (0, 0, 0, 0, 0), (5, 5, 0, 0, -1)):
        add(["outlier", dx, dy, gx, gy, oq], [int(gref.is_outlier(dx, dy, gx, gy, oq))])
    for sad, penalty, pdx, pdy, cost, bias in ((0, 0, 0, 0, 0, 0), (100, 7, -3, 2, 134, 0), (100, 7, -3, 2, 135, 0), (100, 7, -3, 2, 100, 35), (65280, 255, 32, -32, gref.I32_MAX, 65535),
                                               (0, 0, 0, 0, gref.I32_MIN, 65535)):
        cost_g = sad + penalty * (abs(pdx) + abs(pdy))
        add(["evidence", sad, penalty, pdx, pdy, cost, bias], [cost_g, int(cost_g <= cost + bias)])
    return cmds, want


def test_the_headers_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/guide_defs.h is plain __host__ __device__ C++: tests/guide_host_check.cpp runs the prediction, the availability test, the
    classification and the decision as a stand-alone program built with -fsanitize=address,undefined; every line it prints is the
    reference's."""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "guide_host_check"), str(tmp_path / "commands.txt")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tests", "guide_host_check.cpp"), "-o", exe]
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
    assert len(got) == len(want) and len(want) > 500
    for cmd, g, w in zip(cmds, got, want):
        assert g == w, (cmd[:300], g[:200], w[:200])


# ------------------------------------------------------------------------------------------------ library surface
def test_the_twelfth_table_and_the_freeze_of_the_eleventh():
    assert _lib.ext11_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext11_api {"):text.index("} fs_ext11_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == NEW
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables10;") < text.index("typedef struct fs_ext11_api {") < text.index("typedef struct fs_hook_tables11 {")
    tables11 = text[text.index("typedef struct fs_hook_tables11 {"):text.index("} fs_hook_tables11;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables11) == [("fs_hook_tables10", "base10"), ("fs_ext11_api", "ext11")]
    assert int(re.search(r"#define FS_EXT11_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT11_MAGIC == int.from_bytes(b"FSEXTA11", "big")
    # fs_ext10_api is frozen: the header and the binding name the same three members, 40 bytes
    frozen = text[text.index("typedef struct fs_ext10_api {"):text.index("} fs_ext10_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", frozen) == _lib.ext10_hook_names() == ["map_view", "map_gate", "pose_correct"]
    assert ctypes.sizeof(_lib.FsExt10Api) == 40 and len(_lib.ext10_hook_names()) == 3
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables11 all11 = {all10, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT11_MAGIC," in init and "sizeof(fs_ext11_api)," in init
    assert re.search(r"const fs_hook_tables10& all10 = all11\.base10;\s+const fs_hook_tables9& all9 = all10\.base9;", src)
    assert "launch_guide_vectors" in open(os.path.join(CSRC, "kernels.h")).read()
    # the eleven older tables and the export list are what they were
    assert [len(names()) for names in (_lib.hook_names, _lib.ext_hook_names, _lib.ext2_hook_names, _lib.ext3_hook_names, _lib.ext4_hook_names, _lib.ext5_hook_names,
                                       _lib.ext6_hook_names, _lib.ext7_hook_names, _lib.ext8_hook_names, _lib.ext9_hook_names, _lib.ext10_hook_names)] == [
        38, 2, 14, 1, 1, 1, 1, 2, 4, 2, 3]
    assert "fs_guide_vectors" not in _lib.exported_symbols() and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    assert "guide_vectors" not in open(os.path.join(ROOT, "include", "floodseg.h")).read()
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables11.ext11.offset == ctypes.sizeof(_lib.FsHookTables10)                         # directly behind, no padding
    assert _lib.FsExt11Api.guide_vectors.offset == 16 and ctypes.sizeof(_lib.FsExt11Api) == 24
    all11 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables11)).contents
    assert all11.base10.ext10.magic == _lib.EXT10_MAGIC and all11.base10.ext10.size == 40                  # frozen: exactly, not from below
    assert all11.base10.base9.ext9.magic == _lib.EXT9_MAGIC and all11.base10.base9.ext9.size == 32
    assert all11.ext11.magic == _lib.EXT11_MAGIC and all11.ext11.size >= 24                               # from below only: the table grows at its end
    assert ctypes.cast(all11.ext11.guide_vectors, ctypes.c_void_p).value == ctypes.cast(lib.fs_guide_vectors, ctypes.c_void_p).value
    with pytest.raises(AttributeError):
        ctypes.CDLL(_lib.LIB_PATH).fs_guide_vectors                                                       # a table member, not an exported symbol
    assert ctypes.cast(all11.base10.ext10.pose_correct, ctypes.c_void_p).value == ctypes.cast(lib.fs_pose_correct, ctypes.c_void_p).value
    # the kernel takes its rules from the header and its luma from the matcher: one definition of each
    kernel = open(os.path.join(CSRC, "motion_ops.hip")).read()
    assert all(f"guide::{fn}(" in kernel for fn in ("pair_guides", "predict", "available", "classify", "is_outlier", "decide", "evidence_replaces", "out_word"))
    assert len(re.findall(r"uint32_t luma_u8\(", kernel)) == 1 and len(re.findall(r"uint32_t load_luma4\(", kernel)) == 1
    assert not any("luma_u8(" in open(os.path.join(CSRC, f)).read() for f in ("guide_defs.h",))
    assert "hipMemsetAsync" not in kernel and "asm" not in kernel.split("namespace fs {")[1]


def test_the_magic_is_checked_before_use(monkeypatch):
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT11_MAGIC", _lib.EXT11_MAGIC + 1)
    with pytest.raises(RuntimeError, match="the library has no eleventh extension table \\(fs_guide_vectors is missing\\)"):
        fresh.fs_guide_vectors
    assert fresh.fs_pose_correct is not None                                  # the tables in front of it stay usable


def good_arguments():
    """The arguments of a call that passes validation (dummy non-null pointers), in the ABI's order, by name."""
    return dict(mv=64, model=64, n=3, FH=64, FW=96, fill_void=1, outlier_q20=ONE, cur=64, ref=64, channels=3, cost=64, penalty=2, guide_bias=100, out=64,
                counts=64, stream=None)


REFUSALS = [(dict(mv=None), b"null"), (dict(model=None), b"null"), (dict(out=None), b"null"), (dict(counts=None), b"null"),
            (dict(n=0), b"got 0"), (dict(n=65), b"got 65"), (dict(FH=15), b"15x96"), (dict(FW=16385), b"64x16385"), (dict(FH=16385), b"16385x96"), (dict(FW=8), b"64x8"),
            (dict(outlier_q20=-2), b"got -2"), (dict(outlier_q20=64 * ONE + 1), b"got 67108865"), (dict(penalty=-1), b"got -1"), (dict(penalty=256), b"got 256"),
            (dict(guide_bias=-1), b"got -1"), (dict(guide_bias=65536), b"got 65536"),
            (dict(cur=None), b"together"), (dict(ref=None), b"together"), (dict(cost=None), b"together"), (dict(cur=None, ref=None), b"together"),
            (dict(channels=2), b"got 2"), (dict(channels=4), b"got 4"),
            (dict(mv=66), b"aligned to 4"), (dict(out=65), b"aligned to 4"), (dict(cost=66), b"aligned to 4"), (dict(model=68), b"aligned to 8"),
            (dict(counts=68), b"aligned to 8")]


@pytest.mark.parametrize("changed,word", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_the_library_refuses_before_a_launch_and_names_the_value(changed, word):
    """Validation precedes every launch: the pointers are never dereferenced, so the refusals run without a GPU."""
    lib = _lib.load()
    args = good_arguments()
    args.update(changed)
    assert lib.fs_guide_vectors(*args.values()) != 0
    message = lib.fs_last_error()
    assert b"guide_vectors" in message and word in message, message


def test_the_op_refuses_with_a_value_error_that_names_the_value():
    tables, model = torch.zeros((2, 24, 7), dtype=torch.int32), torch.zeros((2, 16), dtype=torch.int64)
    frames, cost = torch.zeros((2, 64, 96, 3), dtype=torch.uint8), torch.zeros((2, 24), dtype=torch.int32)
    good = dict(tables=tables, model=model, frame_size=(64, 96))
    for changed, word in ((dict(frame_size=(15, 96)), r"\(15, 96\)"), (dict(frame_size=(64, 16385)), "16385"), (dict(tables=tables[:, :23]), r"\(2, 23, 7\)"),
                          (dict(tables=tables.long()), "int64"), (dict(tables=torch.zeros((65, 24, 7), dtype=torch.int32)), r"\(65, 24, 7\)"),
                          (dict(model=model[:1]), r"\(1, 16\)"), (dict(model=model.int()), "int32"), (dict(outlier=-0.5), "-0.5"), (dict(outlier=65), "65"),
                          (dict(penalty=256), "256"), (dict(guide_bias=65536), "65536"), (dict(guide_bias=-1), "-1"),
                          (dict(cur=frames), r"only \['cur'\]"), (dict(cur=frames, ref=frames), r"only \['cur', 'ref'\]"), (dict(cost=cost), r"only \['cost'\]"),
                          (dict(cur=frames[..., :2], ref=frames[..., :2], cost=cost), r"\(2, 64, 96, 2\)"), (dict(cur=frames, ref=frames, cost=cost[:, :5]), r"\(2, 5\)"),
                          (dict(cur=frames, ref=frames[:, :32], cost=cost), r"\(2, 32, 96, 3\)"), (dict(out=torch.zeros((2, 24, 6), dtype=torch.int32)), r"\(2, 24, 6\)")):
        with pytest.raises(ValueError, match=word):
            ops.guide_vectors(**{**good, **changed})
    with pytest.raises(RuntimeError, match="GPU"):
        ops.guide_vectors(**good)                                                                        # host tensors: no CPU fallback exists


# ------------------------------------------------------------------------------------------------ GridEstimator(guide=...) on stubs
def stub_ops(monkeypatch, fh=32, fw=48):
    """ops' search, fit and guide, and the table -> grid step, replaced by host stubs that record their calls; the guide stub is the
    numpy reference itself."""
    calls = dict(search=[], fit=[], guide=[], grids=[])
    blocks = (fh // 16) * (fw // 16)

    def table_of(cur, ref_):
        t = mref.grid_table(fh // 16, fw // 16, lambda x, y: (0 * x + int(cur.reshape(-1)[0]), 0 * y - int(ref_.reshape(-1)[0])))
        t[4] = gref.VOID_ROW                                                  # one void row (an inner block's) for the guide to fill
        return torch.from_numpy(t)

    def block_match(cur, ref_, search=16, penalty=0, return_cost=False):
        calls["search"].append((int(ref_.reshape(-1)[0]), int(cur.reshape(-1)[0]), "cost" if return_cost else ""))
        return (table_of(cur, ref_), torch.full((blocks,), 9, dtype=torch.int32)) if return_cost else table_of(cur, ref_)

    def block_match_modes(cur, ref_, search=16, penalty=0, intra_bias=65535, scene_cut=None, return_cost=False, return_stats=False):
        calls["search"].append((int(ref_.reshape(-1)[0]), int(cur.reshape(-1)[0]), "cost" if return_cost else ""))
        stats = torch.tensor([blocks, 1, int(cur.reshape(-1)[0]) == 3, 0], dtype=torch.int32)
        return (table_of(cur, ref_), torch.full((blocks,), 9, dtype=torch.int32), stats) if return_cost else (table_of(cur, ref_), stats)

    def global_motion(tables, frame_size, mask_size, rounds=4, tol=1.0, min_inliers=12, mask=None, exclude=(), pair_stats=None):
        calls["fit"].append((tuple(frame_size), tuple(mask_size), rounds, tol, min_inliers, None if pair_stats is None else pair_stats.tolist()))
        cut = pair_stats is not None and int(pair_stats[0, 2]) != 0
        dx, dy = int(tables[0, 0, 3] - tables[0, 0, 5]), int(tables[0, 0, 4] - tables[0, 0, 6])
        return torch.tensor([gref.shift_model(dx, dy, status=1 if cut else 0)], dtype=torch.int64)

    def guide_vectors(tables, model, frame_size, fill_void=True, outlier=None, cur=None, ref=None, cost=None, penalty=0, guide_bias=None, out=None):
        calls["guide"].append(dict(outlier=outlier, evidence=cur is not None, penalty=penalty, guide_bias=guide_bias, fill_void=fill_void))
        assert (cur is None) == (ref is None) == (cost is None) and (cur is None or (cur.shape[0] == 1 and cost.shape == (1, blocks)))
        got = gref.guide_vectors(tables.numpy(), model.numpy(), frame_size[0], frame_size[1], int(fill_void), gref.outlier_q20(outlier))
        return torch.from_numpy(got[0]), torch.from_numpy(got[1])

    def to_grids(table, h, w, validate=True):
        calls["grids"].append(table.clone())
        return table.double(), -table.double()

    monkeypatch.setattr(ops, "block_match", block_match)
    monkeypatch.setattr(ops, "block_match_modes", block_match_modes)
    monkeypatch.setattr(ops, "global_motion", global_motion)
    monkeypatch.setattr(ops, "guide_vectors", guide_vectors)
    monkeypatch.setattr(motion, "motion_vectors_to_grids", to_grids)
    monkeypatch.setattr(motion, "check_geometry", lambda h, w: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return calls, table_of


def test_grid_estimator_keeps_raw_and_guided_tables_of_one_search_per_pair(monkeypatch):
    calls, table_of = stub_ops(monkeypatch)
    frames = {i: torch.full((32, 48), i, dtype=torch.uint8) for i in range(7)}
    load = frames.get
    void = torch.tensor(gref.VOID_ROW, dtype=torch.int32)
    est = motion.GridEstimator(search=8, penalty=3, guide=True, guide_rounds=2, guide_tol=0.5, guide_min_inliers=5)
    raw2 = est.raw_table_for(2, load)                                                                     # the raw table asked first ...
    t2, g2 = est.table_for(2, load), est.grids_for(2, load)
    assert calls["search"] == [(1, 2, "")] and len(calls["fit"]) == len(calls["guide"]) == 1             # ... one search, one fit, one guide serve all three
    assert calls["fit"][0] == ((32, 48), (32, 48), 2, 0.5, 5, None) and calls["guide"][0] == dict(outlier=None, evidence=False, penalty=0, guide_bias=None, fill_void=True)
    assert torch.equal(raw2, table_of(frames[2], frames[1])) and (raw2[4] == void).all()
    assert t2[4].tolist() == [-1, 16, 16, 24 + 2, 24 - 1, 24, 24] and torch.equal(t2[[0, 1, 2, 3, 5]], raw2[[0, 1, 2, 3, 5]])  # the void row is filled, nothing else moves
    assert torch.equal(g2[0], t2.double()) and torch.equal(calls["grids"][0], t2)                         # the grids come from the GUIDED table
    assert est.guide_counts_for(2).tolist() == [6, 1, 1, 0, 0, 0, 0, 0] and est.guide_counts_for(3) is None
    g4 = est.grids_for(4, load)                                                                           # the grids asked first
    assert torch.equal(g4[0], est.table_for(4, load).double()) and (est.raw_table_for(4, load)[4] == void).all() and calls["search"] == [(1, 2, ""), (3, 4, "")]
    tables, raws = est.window_tables(2, 3, load), est.window_raw_tables(2, 3, load)
    assert calls["search"] == [(1, 2, ""), (3, 4, ""), (2, 3, "")] and tables.shape == raws.shape == (3, 6, 7)
    assert torch.equal(tables[0], t2) and torch.equal(raws[0], raw2) and (raws[:, 4] == void).all(1).all() and not (tables[:, 4] == void).all(1).any()
    assert est.guide_report()[0] == [2, 3, 4]
    # a frame without a predecessor: the void table, raw and guided, and no fit
    assert (est.table_for(0, load) == void).all() and (est.raw_table_for(0, load) == void).all() and len(calls["fit"]) == 3
    # eviction takes the raw table with the guided one; reset forgets the counts
    small = motion.GridEstimator(search=8, cache=1, guide=True)
    small.table_for(1, load), small.table_for(2, load)
    assert list(small._tables) == [2] and list(small._raw) == [2] and small.guide_report()[0] == [1, 2]
    small.reset()
    assert not small._raw and small.guide_report()[0] == [] and not small._guide_chunks
    # guide_bias asks the search for its costs and hands the frames on; a cut pair passes through untouched
    for key in calls:
        del calls[key][:]
    ev = motion.GridEstimator(search=8, penalty=3, intra_bias=0, scene_cut=0.5, guide=True, guide_outlier=1.5, guide_bias=40)
    t2, t3 = ev.table_for(2, load), ev.table_for(3, load)
    assert calls["search"] == [(1, 2, "cost"), (2, 3, "cost")] and calls["guide"][0] == dict(outlier=1.5, evidence=True, penalty=3, guide_bias=40, fill_void=True)
    assert calls["fit"][0][5] == [[6, 1, 0, 0]] and calls["fit"][1][5] == [[6, 1, 1, 0]]
    assert not (t2[4] == void).all() and torch.equal(t3, ev.raw_table_for(3, load)) and int(ev.stats_for(3)[2]) == 1
    assert ev.guide_counts_for(3).tolist() == [6, 1, 0, 0, 0, 0, 0, 0]
    # estimate_grids takes the same arguments
    del calls["search"][:], calls["guide"][:]
    grid, inv = motion.estimate_grids(frames[2], frames[1], search=8, guide=True, guide_outlier=2.0)
    assert calls["search"] == [(1, 2, "")] and calls["guide"][0]["outlier"] == 2.0 and grid[4].tolist() == [-1, 16, 16, 26, 23, 24, 24] and torch.equal(inv, -grid)
    for bad in (dict(guide_outlier=1.0), dict(guide_bias=3), dict(guide=True, guide_outlier=65), dict(guide=True, guide_bias=65536), dict(guide=True, guide_rounds=9),
                dict(guide=True, guide_min_inliers=2)):
        with pytest.raises(ValueError, match="guide"):
            motion.GridEstimator(**bad)


def test_guide_off_is_the_estimator_of_before(monkeypatch):
    calls, table_of = stub_ops(monkeypatch)
    frames = {i: torch.full((32, 48), i, dtype=torch.uint8) for i in range(5)}
    est = motion.GridEstimator(search=8)
    t2 = est.table_for(2, frames.get)
    assert est.guide is False and torch.equal(t2, table_of(frames[2], frames[1])) and est.raw_table_for(2, frames.get) is t2
    assert torch.equal(est.window_raw_tables(1, 2, frames.get), est.window_tables(1, 2, frames.get))
    assert calls["fit"] == [] and calls["guide"] == [] and est.guide_counts_for(2) is None and est.guide_report()[0] == [] and est.window_guide_counts(1, 2) is None and not est._raw
    assert torch.equal(est.grids_for(2, frames.get)[0], t2.double()) and calls["search"] == [(1, 2, ""), (0, 1, "")]
    grid, _ = motion.estimate_grids(frames[2], frames[1], search=8)
    assert torch.equal(grid, t2.double()) and calls["fit"] == [] and calls["guide"] == []


def test_datasets_pass_the_guide_arguments_on_and_carry_the_raw_tables(monkeypatch, tmp_path):
    fh, fw, delta = 32, 48, 3
    calls, _ = stub_ops(monkeypatch, fh, fw)
    path = str(tmp_path / "clip.rgb")
    np.repeat(np.arange(7, dtype=np.uint8), fh * fw * 3).tofile(path)
    monkeypatch.setattr(ops, "prepare_frame", lambda frame, size, mean, std, **kw: torch.zeros(1, 3, fh, fw))
    monkeypatch.setattr(ops, "frame_planes", lambda buf, h, w, fmt: (buf.view(h, w, 3), None))
    void = torch.tensor(gref.VOID_ROW, dtype=torch.int32)
    off = dataset.RawVideoWindows(path, fh, fw, "rgb24", frame_delta=delta, no_warp=True, device="cpu", link_vectors=True)
    item = off[1]
    assert "link_raw_mvs" not in item and "link_guide_counts" not in item and (item["link_mvs"][:, 4] == void).all() and off.estimator.guide is False
    ds = dataset.RawVideoWindows(path, fh, fw, "rgb24", frame_delta=delta, no_warp=True, device="cpu", link_vectors=True, guide=True, guide_outlier=2.0, guide_bias=7,
                                 guide_rounds=3, guide_tol=0.75, guide_min_inliers=4)
    est = ds.estimator
    assert (est.guide, est.guide_outlier, est.guide_bias, est.guide_rounds, est.guide_tol, est.guide_min_inliers) == (True, 2.0, 7, 3, 0.75, 4)
    item = ds[1]                                                                                          # emits frames 3, 4, 5
    assert item["link_mvs"].shape == item["link_raw_mvs"].shape == (delta, 6, 7) and item["link_raw_mvs"].dtype == torch.int32
    assert item["link_guide_counts"].dtype == torch.int64 and item["link_guide_counts"].tolist() == [[6, 1, 1, 0, 0, 0, 0, 0]] * delta
    assert ds[0]["link_guide_counts"].tolist() == [[0] * 8] + [[6, 1, 1, 0, 0, 0, 0, 0]] * (delta - 1)      # frame 0 has no pair: a row of zeros
    assert (item["link_raw_mvs"][:, 4] == void).all() and not (item["link_mvs"][:, 4] == void).all(1).any()
    assert torch.equal(item["link_mvs"][:, [0, 1, 2, 3, 5]], item["link_raw_mvs"][:, [0, 1, 2, 3, 5]]) and calls["guide"][0]["evidence"]
    for cls, args in ((dataset.PredictWindows, (str(tmp_path), "v")), (dataset.RawVideoWindows, (path, fh, fw, "rgb24"))):
        with pytest.raises(ValueError, match="guide"):
            cls(*args, grids="estimate", guide_outlier=1.0)                                              # needs guide=True
    with pytest.raises(ValueError, match="guide"):
        dataset.PredictWindows(str(tmp_path), "v", grids="files", guide=True)                             # the grids/ folders hold no vectors to guide


# ------------------------------------------------------------------------------------------------ the report and the tools' flags
def test_guide_report_reads_the_counts_once_and_the_csv_lists_them_per_frame(monkeypatch, tmp_path):
    from flood_uav_video_segmentation_amd.flow.predict import write_guide_csv

    stub_ops(monkeypatch)
    frames = {i: torch.full((32, 48), i, dtype=torch.uint8) for i in range(6)}
    est = motion.GridEstimator(search=8, guide=True)
    assert est.guide_report()[0] == [] and est.guide_report()[1].shape == (0, 8)
    est.table_for(4, frames.get), est.table_for(2, frames.get), est.table_for(0, frames.get)             # frame 0 has no pair
    ids, counts = est.guide_report()
    assert ids == [2, 4] and counts.dtype == np.int64 and counts.tolist() == [[6, 1, 1, 0, 0, 0, 0, 0]] * 2
    path = str(tmp_path / "guide.csv")
    write_guide_csv(path, ids, counts)
    assert open(path).read().split("\n") == ["frame," + ",".join(ops.GUIDE_COUNTS), "2,6,1,1,0,0,0,0,0", "4,6,1,1,0,0,0,0,0", ""]
    assert ops.GUIDE_COUNTS == gref.COUNTS
    assert motion.GridEstimator(search=8).guide_report()[0] == []


def test_the_tools_take_the_guide_flags(capsys):
    import importlib.util

    spec = importlib.util.spec_from_file_location("predict_video_tool_guide", os.path.join(ROOT, "tools", "predict_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw = ["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights"]
    a = tool.parse_args(raw + ["--guide", "--guide-outlier", "1.5", "--guide-bias", "64", "--guide-report", "g.csv"])
    assert (a.guide, a.guide_outlier, a.guide_bias, a.guide_report) == (True, 1.5, 64, "g.csv")
    b = tool.parse_args(raw)
    assert (b.guide, b.guide_outlier, b.guide_bias, b.guide_report) == (False, None, None, None)
    assert tool.parse_args(["--data-root", "d", "--synthetic-weights", "--grids", "estimate", "--guide"]).guide
    capsys.readouterr()
    for bad, word in ((raw + ["--guide-outlier", "1"], "need --guide"), (raw + ["--guide-report", "g.csv"], "need --guide"), (raw + ["--guide-bias", "3"], "need --guide"),
                      (raw + ["--guide", "--guide-outlier", "65"], "0..64"), (raw + ["--guide", "--guide-outlier", "1", "--guide-bias", "65536"], "0..65535"),
                      (raw + ["--guide", "--guide-bias", "3"], "needs --guide-outlier"),
                      (["--data-root", "d", "--synthetic-weights", "--guide"], "hold grids"),
                      (["--data-root", "d", "--synthetic-weights", "--grids", "files", "--guide"], "hold grids")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert word in capsys.readouterr().err, bad
    spec = importlib.util.spec_from_file_location("estimate_grids_tool_guide", os.path.join(ROOT, "tools", "estimate_grids.py"))
    grids_tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(grids_tool)
    for bad, word in ((["d", "v", "--guide-outlier", "1"], "need --guide"), (["d", "v", "--guide", "--guide-outlier", "-1"], "0..64"),
                      (["d", "v", "--guide", "--guide-bias", "3"], "needs --guide-outlier")):
        with pytest.raises(SystemExit):
            grids_tool.main(bad)
        assert word in capsys.readouterr().err, bad
