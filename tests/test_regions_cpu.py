"""Connected regions, the parts that need no GPU: the numpy definition (tests/regions_ref.py) against a flood fill and against
scipy.ndimage.label, the invariants of the table and of the filter, the three new members of the third hook table, the refusals, the
labelling passes of csrc/region_uf.h run on the CPU by a stand-alone sanitized host program, and the FlowPredictor plumbing on a stub
model."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import regions_ref as ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor, write_regions_csv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mask_regions", "region_table", "region_filter"]
ALL = [(c, p, k) for c in range(len(ref.CASES)) for p in ref.PATTERNS for k in (4, 8)]


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_equals_a_flood_fill_on_the_small_cases():
    for case in range(4):
        for pattern in ref.PATTERNS:
            for conn in (4, 8):
                e = ref.expected(case, pattern, conn)
                assert np.array_equal(e["labels"], ref.mask_regions_bfs(e["mask"], e["classes"], conn)), (case, pattern, conn)


def test_reference_equals_scipy_by_partition_per_class():
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: np.ones((3, 3), int)}
    for case, pattern, conn in ALL:
        e = ref.expected(case, pattern, conn)
        for f, m in enumerate(e["mask"]):
            for k in range(e["classes"]):
                theirs, count = ndimage.label(m == k, structure[conn])
                ours = np.where(m == k, e["labels"][f], 0)
                assert ref.partitions_equal(ours, theirs) and len(np.unique(ours[ours > 0])) == count, (case, pattern, conn, f, k)


def test_patterns_are_what_the_case_list_says():
    n, h, w = ref.CASES[4]
    assert h > 2 * ref.TILE_H and h % ref.TILE_H and w > 2 * ref.TILE_W and w % ref.TILE_W                  # 3 x 3 tiles, remainders
    n, h, w = ref.CASES[5]
    assert h > 2 * ref.TILE_H and h % ref.TILE_H and w > ref.TILE_W and w % ref.TILE_W                      # 5 x 2 tiles, remainders
    text = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "region_uf.h")).read()
    assert f"TILE_H = {ref.TILE_H}, TILE_W = {ref.TILE_W};" in text
    n, h, w = ref.CASES[6]
    assert w % 4 == 0 and h > 2 * ref.TILE_H and h % ref.TILE_H and w > 2 * ref.TILE_W and w % ref.TILE_W  # the dword-store width
    for pattern in ("percolation", "random5", "frames"):                                         # ... with pixels the filter re-classes,
        e = ref.expected(6, pattern, 8)                                                                     # at row starts and row tails too
        changed = e["filtered"][9] != e["mask"]
        assert changed.sum() > 50 and changed[:, :, :4].any() and changed[:, :, -4:].any(), pattern
    for case in (4, 5, 6):
        n, h, w = ref.CASES[case]
        for conn in (4, 8):
            spiral = ref.expected(case, "spiral", conn)
            assert (spiral["with_conf"][1][:, 0] == 2).all()                                               # the path and what it leaves
            assert spiral["with_conf"][0][0, 0, 1] > h * w // 3 and spiral["with_conf"][0][0, 0, 5] == h - 1
            comb = ref.expected(case, "comb", conn)
            assert comb["with_conf"][1][0, 0] == 1 + w // 2                                                 # the comb and its gaps
        assert ref.expected(case, "checker", 4)["with_conf"][1][0].tolist() == [h * w, h * w]
        assert ref.expected(case, "checker", 4)["overflow"][1][0].tolist() == [h * w, ref.OVERFLOW_CAP]
        assert ref.expected(case, "checker", 8)["with_conf"][1][0].tolist() == [2, 2]
        assert ref.expected(case, "uniform", 8)["with_conf"][1][0].tolist() == [1, 1]
        # the diagonal contacts on the tile corners join at 8 and stay apart at 4
        c4, c8 = ref.expected(case, "corners", 4), ref.expected(case, "corners", 8)
        corners = len(range(ref.TILE_H, h, ref.TILE_H)) * len(range(ref.TILE_W, w, ref.TILE_W))
        assert c4["with_conf"][1][0, 0] == 1 + 2 * corners and c8["with_conf"][1][0, 0] == 1 + corners
        # no region leaks from the last row of a frame into the first row of the next one
        fr = ref.expected(case, "frames", 8)
        assert fr["labels"][1, 0, 0] == 1 and fr["labels"][0, -1, 0] != 1 and (fr["mask"][0, -1] == fr["mask"][1, 0]).all()
        st = ref.expected(case, "stripes", 8)
        assert (st["labels"][st["mask"] >= 5] == 0).all() and (st["with_conf"][2][st["mask"] >= 5] == -1).all()


def test_table_and_filter_invariants():
    for case, pattern, conn in ALL:
        e = ref.expected(case, pattern, conn)
        mask, k = e["mask"], e["classes"]
        table, counts, index = e["with_conf"]
        assert (counts[:, 0] < e["cap"]).all() and (counts[:, 0] == counts[:, 1]).all()                     # the cap is large enough
        for f in range(mask.shape[0]):
            rows = int(counts[f, 1])
            assert table[f, :rows, 1].sum() == (mask[f] < k).sum() and not table[f, rows:].any()
            anchors = table[f, :rows, 3] * mask.shape[2] + table[f, :rows, 2]                               # y0 is the anchor's row ...
            first = np.array([np.flatnonzero(index[f].reshape(-1) == r)[0] for r in range(min(rows, 50))])
            assert (np.diff(first) > 0).all() and (first // mask.shape[2] == table[f, :len(first), 3]).all() and (anchors[:len(first)] <= first).all()
            assert np.array_equal(e["labels"][f].reshape(-1)[first], first + 1)
        assert not e["without"][0][..., 8:].any()
        assert np.array_equal(table[..., :8], e["without"][0][..., :8])
        over_t, over_c, over_i = e["overflow"]
        common = min(ref.OVERFLOW_CAP, e["cap"])                                                              # the smallest frames hold fewer
        assert np.array_equal(over_t[:, :common], table[:, :common]) and not over_t[:, common:].any()
        assert (over_c[:, 1] == np.minimum(counts[:, 0], ref.OVERFLOW_CAP)).all() and np.array_equal(over_c[:, 0], counts[:, 0])
        assert np.array_equal(over_i, np.where(index < ref.OVERFLOW_CAP, index, -1))
        assert np.array_equal(e["filtered"][0], mask) and np.array_equal(e["filtered"][1], mask)           # min_area <= 1: the identity
        for a in ref.MIN_AREAS:
            changed = e["filtered"][a] != mask
            area = np.where(index >= 0, np.take_along_axis(table[..., 1], np.maximum(index, 0).reshape(mask.shape[0], -1), 1).reshape(mask.shape), 0)
            assert not (changed & ~((index >= 0) & (area < a))).any()                                       # speckle pixels only
            assert (e["filtered"][a][mask >= k] == mask[mask >= k]).all()


def test_filter_on_hand_made_masks():
    m = np.zeros((1, 7, 9), np.uint8)
    m[0, 3, 4] = 2                                                            # a speckle enclosed by one region takes its class
    labels = ref.mask_regions(m, 5, 8)
    t, c, i = ref.region_table(m, labels, 5, None, 128, 16)
    assert c[0].tolist() == [2, 2] and t[0, 1].tolist() == [2, 1, 4, 3, 4, 3, 4, 3, 0, 0] and t[0, 0, 1] == 62
    assert (ref.region_filter(m, i, t, 5, 2) == 0).all()
    m[0, 3, 5] = 3                                                            # two adjacent speckles do not vote for each other
    labels = ref.mask_regions(m, 5, 8)
    t, c, i = ref.region_table(m, labels, 5, None, 128, 16)
    assert c[0, 0] == 3 and (ref.region_filter(m, i, t, 5, 2) == 0).all()
    alone = np.array([[[1, 2]]], np.uint8)                                    # only speckles: nobody votes, both stay
    t, c, i = ref.region_table(alone, ref.mask_regions(alone, 5, 4), 5, None, 128, 4)
    assert np.array_equal(ref.region_filter(alone, i, t, 5, 9), alone)
    tie = np.array([[[1, 1, 1], [0, 4, 0], [3, 3, 3]]], np.uint8)            # each pixel of the middle row: one vote for 1, one for 3
    t, c, i = ref.region_table(tie, ref.mask_regions(tie, 5, 4), 5, None, 128, 8)
    got = ref.region_filter(tie, i, t, 5, 2)
    assert got[0, 1].tolist() == [1, 1, 1] and np.array_equal(got[0, ::2], tie[0, ::2])   # the tie goes to the lowest id


# ------------------------------------------------------------------------------------------------ library surface
def test_new_members_follow_frame_report_in_header_initialiser_and_binding():
    ext2 = _lib.ext2_hook_names()
    assert ext2[7] == "frame_report" and ext2[8:11] == NEW
    assert [getattr(_lib.FsExt2Api, n).offset for n in NEW] == [80, 88, 96]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext2_api {"):text.index("} fs_ext2_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body)[:11] == ext2[:11]
    src = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read()
    init = src[src.index("static const fs_hook_tables2 all"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M)[:11] == ["fs_" + n for n in ext2[:11]]
    assert "region_ops.hip" in open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    all3 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables2)).contents
    assert all3.ext2.magic == _lib.EXT2_MAGIC and all3.ext2.size >= 104        # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all3.ext2, name), ctypes.c_void_p).value and getattr(lib, "fs_" + name) is not None
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                  # table members, not exported symbols
    assert not any("fs_" + n in _lib.exported_symbols() for n in NEW) and len(_lib.exported_symbols()) == 40
    assert lib.fs_version() == 600
    assert not any(n in open(os.path.join(ROOT, "include", "floodseg.h")).read() for n in NEW)


def test_library_refuses_bad_arguments_before_a_launch():
    """Fake non-null pointers: a call that got as far as a launch would fail with another message (or fault on a GPU)."""
    lib = _lib.load()
    for op, kw, word in ref.refusal_cases():
        assert ref.call_region_op(lib, op, **kw) != 0, (op, kw)
        msg = lib.fs_last_error()
        assert word in msg and op.encode() in msg, (op, kw, msg)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mask_regions(m, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.region_table(m, m.int(), 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.region_filter(m, m.int(), torch.zeros(1, 4, 10, dtype=torch.int64), 5, 3)
    for kw in (dict(regions=True, max_regions=0), dict(regions=True, connectivity=6), dict(min_region_area=-1)):
        with pytest.raises(ValueError):
            FlowPredictor(torch.nn.Identity(), **kw)


# ------------------------------------------------------------------------------------------------ the kernels' merge logic on the CPU
def test_union_find_header_on_the_cpu_under_sanitizers(tmp_path):
    """csrc/region_uf.h is plain __host__ __device__ C++: tests/regions_host_check.cpp runs the three labelling passes with it, tile by
    tile, in two orders, on every case, as a stand-alone program built with -fsanitize=address,undefined."""
    makefile = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "regions_host_check"), str(tmp_path / "cases.bin")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc"), os.path.join(ROOT, "tests", "regions_host_check.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):   # the runtimes linked in where the compiler can
        build = subprocess.run(base + static, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    with open(data, "wb") as fh:
        fh.write(np.int32(len(ALL)).tobytes())
        for case, pattern, conn in ALL:
            e = ref.expected(case, pattern, conn)
            n, h, w = e["mask"].shape
            fh.write(np.array([n, h, w, e["classes"], conn], np.int32).tobytes())
            fh.write(np.ascontiguousarray(e["mask"]).tobytes())
            fh.write(np.ascontiguousarray(e["labels"]).tobytes())
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert f"{len(ALL)} entries, 0 mismatching runs" in run.stdout


# ------------------------------------------------------------------------------------------------ CSV and FlowPredictor plumbing
def test_regions_csv(tmp_path):
    rows = [np.array([[1, 4, 2, 3, 3, 4, 10, 14, 510, 1]], np.int64), np.zeros((0, 10), np.int64)]
    path = str(tmp_path / "r.csv")
    write_regions_csv(path, [7, 8], rows)
    lines = open(path).read().splitlines()
    assert lines[0] == "frame,region,class,area,x0,y0,x1,y1,cx,cy,conf,low"
    assert lines[1:] == ["7,0,1,4,2,3,3,4,2.500,3.500,0.500000,0.250000"]
    write_regions_csv(path, [7, 8], rows, with_confidence=False)
    assert open(path).read().splitlines() == ["frame,region,class,area,x0,y0,x1,y1,cx,cy", "7,0,1,4,2,3,3,4,2.500,3.500"]
    with pytest.raises(ValueError):
        write_regions_csv(path, [7], rows)


class StubFlow(torch.nn.Module):
    """A flow model that returns fixed logits [n,K,H,W] (a foreign network: no fused routes)."""
    feature_based = True
    no_warp = True

    def __init__(self, k=3, hw=(6, 8)):
        super().__init__()
        self.k, self.hw, self.calls = k, hw, 0

    def predict(self, frame_prev, frame_next, mvs_left, mvs_right, n, profiler=None, **extra):
        self.calls += 1
        g = torch.Generator().manual_seed(self.calls)
        return {"pred": torch.randn((n, self.k) + self.hw, generator=g) * 2}


def test_predictor_plumbing_with_a_stub_model(monkeypatch):
    """The ops are replaced by the numpy definition (they refuse CPU tensors): which op is called with what, what is returned, and
    how the region report grows across chunk borders."""
    called = []

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    monkeypatch.setattr(ops, "resize_argmax_u8", lambda logits, size: logits.argmax(1).to(torch.uint8))
    monkeypatch.setattr(ops, "mask_regions", lambda mask, classes, connectivity=8: (called.append(("mr", connectivity)),
                                                                                     t(ref.mask_regions(mask.numpy(), classes, connectivity)))[1])

    def table(mask, labels, classes, conf=None, low=128, max_regions=1024, out=None):
        called.append(("rt", max_regions))
        got = ref.region_table(mask.numpy(), labels.numpy(), classes, None if conf is None else conf.numpy(), low, max_regions)
        if out is not None:
            out[0].copy_(t(got[0]))
            out[1].copy_(t(got[1]))
            return out[0], out[1], t(got[2])
        return tuple(t(a) for a in got)

    monkeypatch.setattr(ops, "region_table", table)
    monkeypatch.setattr(ops, "region_filter", lambda mask, index, tab, classes, min_area: (called.append(("rf", min_area)),
                        t(ref.region_filter(mask.numpy(), index.numpy(), tab.numpy(), classes, min_area)))[1])
    x = torch.zeros(1, 3, 6, 8)
    grids = [None] * 2
    kw = dict(classes=3, out_size=(6, 8), crop=None, compute_metrics=False)
    plain = FlowPredictor(StubFlow(), **kw).predict_window(x, x, grids, grids, to_host=False)
    assert called == []
    monkeypatch.setattr(FlowPredictor, "REPORT_CHUNK", 4)
    on = FlowPredictor(StubFlow(), regions=True, connectivity=4, max_regions=5, **kw)
    masks = on.predict_window(x, x, grids, grids, to_host=False)
    assert torch.equal(masks, plain) and called == [("mr", 4), ("rt", 5)]                                   # regions alone: the default masks
    kept = [masks.numpy()]
    for _ in range(2):
        kept.append(on.predict_window(x, x, grids, grids))
    rows, totals = on.region_report()
    assert len(rows) == 9 and totals.shape == (9,) and len(on._region_chunks) == 3
    for f, m in enumerate(np.concatenate(kept)):
        tab, cnt, _ = ref.region_table(m[None], ref.mask_regions(m[None], 3, 4), 3, None, 128, 5)
        assert totals[f] == cnt[0, 0] and np.array_equal(rows[f], tab[0, :cnt[0, 1]])
    on.clear_report()
    assert on.region_report()[0] == [] and on._region_chunks == []
    called.clear()
    filt = FlowPredictor(StubFlow(), regions=True, min_region_area=3, **kw)
    got = filt.predict_window(x, x, grids, grids, to_host=False)
    assert [c[0] for c in called] == ["mr", "rt", "rf", "mr", "rt"]                                       # label, filter, label again
    lab = ref.mask_regions(plain.numpy(), 3, 8)
    tab, cnt, idx = ref.region_table(plain.numpy(), lab, 3, None, 128, 1024)
    want = ref.region_filter(plain.numpy(), idx, tab, 3, 3)
    assert np.array_equal(got.numpy(), want)
    rows, totals = filt.region_report()
    tab2, cnt2, _ = ref.region_table(want, ref.mask_regions(want, 3, 8), 3, None, 128, 1024)
    assert all(np.array_equal(rows[f], tab2[f, :cnt2[f, 1]]) for f in range(3)) and np.array_equal(totals, cnt2[:, 0])
    called.clear()
    only = FlowPredictor(StubFlow(), min_region_area=3, **kw)                                             # the filter without the report
    assert np.array_equal(only.predict_window(x, x, grids, grids, to_host=False).numpy(), want) and [c[0] for c in called] == ["mr", "rt", "rf"]
    assert only.region_report()[0] == [] and np.array_equal(only.despeckle_counts(), cnt[:, 0]) and filt.despeckle_counts().shape == (3,)
    only.clear_report()
    assert only.despeckle_counts().shape == (0,)
