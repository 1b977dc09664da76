"""Motion-compensated region links, the parts that need no GPU: the numpy definition (tests/tracks_mc_ref.py) against a pixel loop, the
consequences the header states, the moving-blob scene's figures, the new member of the third hook table, the refusals, the compensated
overlap pass of csrc/track_ops.hip run serially on the CPU through csrc/track_defs.h by a stand-alone sanitized host program, and the
GridEstimator / dataset / FlowPredictor / tool plumbing on stubs."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import regions_ref as rref
import tracks_mc_ref as mc
import tracks_ref as ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import dataset, motion
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "region_links_mc"
EVERY = range(len(mc.case_list()))
KEYS = ("back", "fwd", "link_counts")


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_equals_a_pixel_loop():
    """Every table kind on the first two geometries, the garbage tables everywhere, the blobs, the matched scenes, the full and the
    overflowing pair table, and the cut."""
    names = [c["name"] for c in mc.case_list()]
    small = [i for i, n in enumerate(names) if n.startswith(("blobs", "(48, 80", "(37, 300, 48, 320) random5", "(3, 17", "pairs", "cut")) or n.endswith("garbage")]
    assert len(small) == 25
    for i in small:
        e = mc.expected(i)
        got = mc.region_links_mc_bruteforce(e["index"], e["table"], e["counts"], e["mv"], e["frame_size"], None, e["pair_stats"], e["max_pairs"], e["min_overlap"])
        assert all(np.array_equal(g, e[k]) for g, k in zip(got, KEYS)), e["name"]


def test_case_list_is_what_it_says():
    full, over, cut = (mc.expected(mc.case_by_name(n)) for n in ("pairs_full", "pairs_overflow", "cut"))
    assert full["max_pairs"] == 16 and full["link_counts"].tolist() == [[0, 0], [16, 0]] and (full["back"][1, :8, 0] >= 0).all()
    assert over["max_pairs"] == 16 and over["link_counts"].tolist() == [[0, 0], [16, 1]] and (over["back"][..., 0] == -1).all() and not over["fwd"][..., 1].any()
    assert cut["link_counts"][:, 1].tolist() == [0, 2, 0] and cut["link_counts"][1, 0] == 0 and cut["link_counts"][2, 0] > 100
    assert (cut["back"][1] == [-1, 0]).all() and (cut["fwd"][1] == [-1, 0]).all()
    h, w, fh, fw = mc.GEOMETRIES[1]
    assert w > 256 and w % 256 and w % 64 and (h, w) != (fh, fw) and fh % 16 == 0 and fw % 16 == 0      # a piece border, a ragged last wave, a ragged scale
    h, w, fh, fw = mc.GEOMETRIES[3]
    sy, sx = mc.shifts(mc.table_uniform(fh, fw, 3, -2), h, w, fh, fw)
    assert fh % 16 and fw % 16 and (sy[:48, :80] == -2).all() and (sx[:48, :80] == 3).all() and not sy[48:].any() and not sx[:, 80:].any()   # remainder strips
    for name in ("per_block", "outward", "void_mixed", "pm32", "garbage"):                                # the tables do what their names say
        e = mc.expected(mc.case_by_name(f"(48, 80, 48, 80) random5 {name}"))
        sy, sx = mc.shifts(e["mv"][1], 48, 80, 48, 80)
        row = sx[20]
        assert len(np.unique(row[:64])) > 1, name                                                        # runs break inside a wave
        if name == "outward":
            assert (sy[0] < -16).all() and (sy[-1] > 16).all() and (sx[:, 0] < -16).all() and (sx[:, -1] > 16).all()
        if name == "pm32":
            assert set(np.unique(sx)) == {-32, 32} and set(np.unique(sy)) == {-32, 32}
        if name == "void_mixed":
            assert ((e["mv"][1][:, 5] < 0).sum() > 2) and (e["mv"][1][:, 5] >= 0).sum() > 2
        if name == "garbage":
            v = e["mv"][1].astype(np.int64)
            assert (abs(v[:, 3] - v[:, 5]) > 2 ** 31).any() and ((abs(v[:, 3] - v[:, 5]) == 1024) & (v[:, 5] >= 0) & (v[:, 6] >= 0)).any()
            assert (abs(sx) <= 1024).all() and (abs(sy) <= 1024).all() and (abs(sx) == 1024).any()
    e = mc.expected(mc.case_by_name("(96, 160, 48, 80) random5 uniform"))                                 # mask twice the frame: shifts doubled
    sy, sx = mc.shifts(e["mv"][1], 96, 160, 48, 80)
    assert (sy == 2 * (int(e["mv"][1][0, 4]) - int(e["mv"][1][0, 6]))).all() and (sx == 2 * (int(e["mv"][1][0, 3]) - int(e["mv"][1][0, 5]))).all()


def test_void_and_zero_tables_give_the_in_place_links():
    for i in range(len(ref.case_list())):
        e = ref.expected(i)
        n, h, w = e["mask"].shape
        for fh, fw in ((max(h, 16), max(w, 16)), (48, 320)):
            for table in (mc.table_void(fh, fw), mc.table_uniform(fh, fw, 0, 0)):
                got = mc.region_links_mc(e["index"], e["table"], e["counts"], np.stack([table] * n), (fh, fw), None, None, e["max_pairs"], e["min_overlap"])
                assert all(np.array_equal(g, e[k]) for g, k in zip(got, KEYS)), (e["name"], fh, fw)


def test_the_shift_is_the_vector_at_equal_sizes_and_scales_to_nearest():
    rng = np.random.default_rng(5)
    for h, w in ((48, 80), (50, 90), (16, 16)):
        hb, wb = h // 16, w // 16
        vx, vy = rng.integers(-40, 41, (hb, wb)), rng.integers(-40, 41, (hb, wb))
        sy, sx = mc.shifts(mc._rows(h, w, vx, vy), h, w, h, w)
        assert np.array_equal(sy[:hb * 16, :wb * 16], np.kron(vy, np.ones((16, 16), np.int64))) and np.array_equal(sx[:hb * 16, :wb * 16], np.kron(vx, np.ones((16, 16), np.int64)))
    for v, p, f, want in ((1, 8, 16, 1), (-1, 8, 16, -1), (1, 7, 16, 0), (3, 37, 48, 2), (-13, 300, 320, -12), (5, 713, 1080, 3), (-7, 713, 1920, -3)):
        sy, sx = mc.shifts(mc.table_uniform(f, 16, 0, v), p, 1, f, 16)                                    # nearest, ties away from zero
        assert sy[0, 0] == want and not sx.any(), (v, p, f)
        sy, sx = mc.shifts(mc.table_uniform(16, f, v, 0), 1, p, 16, f)
        assert sx[0, 0] == want and not sy.any(), (v, p, f)


def test_one_frame_equals_region_links_on_a_warped_plane():
    for i in EVERY:
        e = mc.expected(i)
        if e["pair_stats"] is not None:
            continue
        for f in range(1, len(e["mask"])):
            s = slice(f, f + 1)
            prev = (e["index"][f - 1], e["table"][f - 1], e["counts"][f - 1])
            got = mc.region_links_mc(e["index"][s], e["table"][s], e["counts"][s], e["mv"][s], e["frame_size"], prev, None, e["max_pairs"], e["min_overlap"])
            warped = (mc.warp_prev(prev[0], e["mv"][f], *e["frame_size"]),) + prev[1:]
            want = ref.region_links(e["index"][s], e["table"][s], e["counts"][s], warped, e["max_pairs"], e["min_overlap"])
            assert all(np.array_equal(g, w) for g, w in zip(got, want)) and all(np.array_equal(g[0], e[k][f]) for g, k in zip(got, KEYS)), (e["name"], f)
            areas = e["table"][f][:, 1]
            assert (got[0][0, :, 1] <= areas).all()                                                      # overlap(a, b) <= area(b)
        for pieces in ([1] * len(e["mask"]), [len(e["mask"])]):
            assert all(np.array_equal(g, e[k]) for g, k in zip(mc.chained(e, pieces), KEYS + ("tracks", "state"))), (e["name"], pieces)


def test_the_blob_scene_needs_the_compensation():
    """8 x 8 blobs on a 32-pixel lattice moving (3, 12) pixels per frame on 96 x 160: in place nothing continues."""
    e = mc.expected(mc.case_by_name("blobs"))
    b = mc.BLOB_SCENE
    rows_mc, flags_mc = mc.clip_tracks(e["mask"], 5, ref.CONN, e["cap"], e["mv"], e["frame_size"], e["max_pairs"])
    rows_in, flags_in = mc.clip_tracks(e["mask"], 5, ref.CONN, e["cap"], e["mv"], e["frame_size"], e["max_pairs"], compensate=False)
    assert all(np.array_equal(r, e["tracks"][f, :len(r)]) for f, r in enumerate(rows_mc))
    cont_in, total, ids_in = mc.continued(rows_in)
    cont_mc, total_mc, ids_mc = mc.continued(rows_mc)
    print(f"in place {cont_in} of {total} continued, {ids_in} ids; compensated {cont_mc} of {total_mc}, {ids_mc} ids")
    assert total == total_mc == 48 and cont_in == 0 and ids_in == int(e["counts"][:, 1].sum()) == 63
    assert cont_mc >= 40 and ids_mc == 63 - cont_mc
    assert not flags_mc.any() and not flags_in.any() and b["step"][1] > b["size"]                        # no pair table overflows


# ------------------------------------------------------------------------------------------------ library surface
def test_new_member_follows_region_tracks_in_header_initialiser_and_binding():
    ext2 = _lib.ext2_hook_names()
    assert ext2[12] == "region_tracks" and ext2[13] == NEW and len(ext2) == 14
    assert getattr(_lib.FsExt2Api, NEW).offset == 120 and ctypes.sizeof(_lib.FsExt2Api) == 128
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext2_api {"):text.index("} fs_ext2_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == ext2
    src = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read()
    init = src[src.index("static const fs_hook_tables2 all"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + n for n in ext2]
    assert "launch_region_links_mc" in open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "kernels.h")).read()
    lib = _lib.load()
    all3 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables2)).contents
    assert all3.ext2.magic == _lib.EXT2_MAGIC and all3.ext2.size >= 128        # from below only: the table grows at its end
    assert ctypes.cast(getattr(all3.ext2, NEW), ctypes.c_void_p).value and getattr(lib, "fs_" + NEW) is not None
    with pytest.raises(AttributeError):
        getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + NEW)                       # a table member, not an exported symbol
    assert "fs_" + NEW not in _lib.exported_symbols() and len(_lib.exported_symbols()) == 40 and lib.fs_version() == 600
    assert NEW not in open(os.path.join(ROOT, "include", "floodseg.h")).read()
    macro = re.search(r"#define FS_REGION_LINKS_MC_WORKSPACE_BYTES\(n, R, max_pairs, hb, wb\) \\\n\s*(.*)", text).group(1).replace("(size_t)", "")
    base = re.search(r"#define FS_REGION_LINKS_WORKSPACE_BYTES\(n, R, max_pairs\) (.*)", text).group(1).replace("(size_t)", "")
    for n, r, p, hb, wb in ((1, 1, 16, 1, 1), (3, 1024, 4096, 67, 120), (5, 65536, 2 ** 20, 3, 5), (1, 16, 64, 3, 5)):
        env = dict(n=n, R=r, max_pairs=p, hb=hb, wb=wb)
        got = eval(macro.replace("FS_REGION_LINKS_WORKSPACE_BYTES(n, R, max_pairs)", "(" + base + ")").replace("/", "//"), env)
        assert got == ops.region_links_mc_workspace_bytes(n, r, p, hb, wb) == ops.region_links_workspace_bytes(n, r, p) + -(-n * hb * wb * 4 // 8) * 8


def test_library_refuses_bad_arguments_before_a_launch():
    """Fake non-null pointers: a call that got as far as a launch would fail with another message (or fault on a GPU)."""
    lib = _lib.load()
    cases = mc.refusal_cases()
    assert len(cases) >= len([c for c in ref.refusal_cases() if c[0] == "region_links"]) + 6
    for kw, word in cases:
        assert mc.call_links_mc(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert word in msg and NEW.encode() in msg, (kw, msg)


def test_ops_refuse_bad_arguments():
    index = torch.zeros(1, 4, 4, dtype=torch.int32)
    table, counts = torch.zeros(1, 4, 10, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64)
    mv = torch.zeros(1, 1, 7, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.region_links(index, table, counts, mv=mv, frame_size=(16, 16))
    with pytest.raises(ValueError, match="track=True"):
        FlowPredictor(torch.nn.Identity(), regions=True, compensate=True)
    with pytest.raises(ValueError, match="track=True"):
        FlowPredictor(torch.nn.Identity(), compensate=True)
    assert FlowPredictor(torch.nn.Identity(), regions=True, track=True).compensate is False
    assert ops.region_links_mc_workspace_bytes(1, 1, 16, 1, 1) == ops.region_links_workspace_bytes(1, 1, 16) + 8


# ------------------------------------------------------------------------------------------------ the kernels' integer logic on the CPU
def test_compensated_pass_on_the_cpu_under_sanitizers(tmp_path):
    """csrc/track_defs.h is plain __host__ __device__ C++: tests/tracks_mc_host_check.cpp runs a serial version of the compensated pass
    with it, in two pixel orders, on every case (the garbage tables among them), as a stand-alone program built with
    -fsanitize=address,undefined."""
    makefile = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "tracks_mc_host_check"), str(tmp_path / "cases.bin")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc"), os.path.join(ROOT, "tests", "tracks_mc_host_check.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):   # the runtimes linked in where the compiler can
        build = subprocess.run(base + static, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    assert any("garbage" in mc.case_list()[i]["name"] for i in EVERY)
    with open(data, "wb") as fh:
        fh.write(np.int32(len(EVERY)).tobytes())
        for i in EVERY:
            e = mc.expected(i)
            n, h, w = e["mask"].shape
            stats = e["pair_stats"]
            fh.write(np.array([n, h, w, e["cap"], e["max_pairs"], e["min_overlap"], e["frame_size"][0], e["frame_size"][1], stats is not None], np.int32).tobytes())
            parts = [("index", np.int32), ("table", np.int64), ("counts", np.int64), ("mv", np.int32)] + ([("pair_stats", np.int32)] if stats is not None else [])
            for key, dtype in parts + [("back", np.int32), ("fwd", np.int32), ("link_counts", np.int64)]:
                assert e[key].dtype == dtype
                fh.write(np.ascontiguousarray(e[key]).tobytes())
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert f"{len(EVERY)} entries, 0 mismatching runs" in run.stdout


# ------------------------------------------------------------------------------------------------ plumbing
def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class StubFlow(torch.nn.Module):
    """A flow model that returns fixed logits [n,K,H,W] (a foreign network: no fused routes): smooth ones, so that regions persist."""
    feature_based = True
    no_warp = True

    def __init__(self, k=3, hw=(6, 8)):
        super().__init__()
        self.k, self.hw, self.calls = k, hw, 0

    def predict(self, frame_prev, frame_next, mvs_left, mvs_right, n, profiler=None, **extra):
        self.calls += 1
        base = torch.randn((1, self.k) + self.hw, generator=torch.Generator().manual_seed(7)) * 2
        noise = torch.randn((n, self.k) + self.hw, generator=torch.Generator().manual_seed(self.calls)) * 0.7
        return {"pred": base + noise}


def test_predictor_plumbing_with_a_stub_model(monkeypatch):
    """The ops are replaced by the numpy definitions: link_mvs and link_stats sliced in step with the chunk borders, reset(), the
    flag word, and the errors."""
    called = []
    monkeypatch.setattr(ops, "resize_argmax_u8", lambda logits, size: logits.argmax(1).to(torch.uint8))
    monkeypatch.setattr(ops, "mask_regions", lambda mask, classes, connectivity=8: t(rref.mask_regions(mask.numpy(), classes, connectivity)))

    def table(mask, labels, classes, conf=None, low=128, max_regions=1024, out=None):
        got = rref.region_table(mask.numpy(), labels.numpy(), classes, None, low, max_regions)
        out[0].copy_(t(got[0]))
        out[1].copy_(t(got[1]))
        return out[0], out[1], t(got[2])

    def links(index, tab, counts, prev=None, max_pairs=None, min_overlap=1, mv=None, frame_size=None, pair_stats=None):
        called.append((index.shape[0], prev is not None, None if mv is None else tuple(mv.shape), frame_size, None if pair_stats is None else tuple(pair_stats.shape)))
        p = None if prev is None else tuple(x.numpy() for x in prev)
        if mv is None:
            return tuple(t(a) for a in ref.region_links(index.numpy(), tab.numpy(), counts.numpy(), p, max_pairs, min_overlap))
        stats = None if pair_stats is None else pair_stats.numpy()
        return tuple(t(a) for a in mc.region_links_mc(index.numpy(), tab.numpy(), counts.numpy(), mv.numpy(), frame_size, p, stats, max_pairs, min_overlap))

    def tracks(back, fwd, counts, state, prev_tracks=None, out=None):
        got, new = ref.region_tracks(back.numpy(), fwd.numpy(), counts.numpy(), state.numpy(), None if prev_tracks is None else prev_tracks.numpy())
        state.copy_(t(new))
        out.copy_(t(got))
        return out

    monkeypatch.setattr(ops, "region_table", table)
    monkeypatch.setattr(ops, "region_links", links)
    monkeypatch.setattr(ops, "region_tracks", tracks)
    monkeypatch.setattr(FlowPredictor, "REPORT_CHUNK", 4)
    x = torch.zeros(1, 3, 6, 8)
    grids = [None] * 2                                                                                   # windows of three frames
    fsize = (32, 48)
    rng = np.random.default_rng(3)
    mvs = np.stack([mc._rows(32, 48, rng.integers(-12, 13, (2, 3)), rng.integers(-12, 13, (2, 3))) for _ in range(12)])
    stats = np.zeros((12, 4), np.int32)
    stats[:, 0] = 6
    stats[[4, 6], 2] = 1                                                                                 # cuts in front of frames 4 (a chunk's first) and 6 (a window's first)
    kw = dict(classes=3, out_size=(6, 8), crop=None, compute_metrics=False, regions=True, connectivity=4, max_regions=20, min_overlap=2, max_pairs=64)
    off = FlowPredictor(StubFlow(), track=True, **kw)
    off.predict_window(x, x, grids, grids, to_host=False, link_mvs=t(mvs[:3]), link_frame_size=fsize)     # compensate=False: the keys are ignored
    assert called == [(3, False, None, None, None)]
    del called[:]
    on = FlowPredictor(StubFlow(), track=True, compensate=True, **kw)
    kept = []
    for wdw in range(3):
        s = slice(3 * wdw, 3 * wdw + 3)
        kept.append(on.predict_window(x, x, grids, grids, link_mvs=t(mvs[s]), link_frame_size=fsize, link_stats=t(stats[s])))
    # 3 | 1 + 2 | 2 + 1: the chunk borders cut the second and the third window, and the tables are cut with them
    assert called == [(3, False, (3, 6, 7), fsize, (3, 4)), (1, True, (1, 6, 7), fsize, (1, 4)), (2, True, (2, 6, 7), fsize, (2, 4)),
                      (2, True, (2, 6, 7), fsize, (2, 4)), (1, True, (1, 6, 7), fsize, (1, 4))]
    masks = np.concatenate(kept)
    want, want_flags = mc.clip_tracks(masks, 3, 4, 20, mvs, fsize, 64, 2, stats=stats)
    got, over, cuts = on.track_report(with_cuts=True)
    assert len(got) == 9 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(over, want_flags & 1) and np.array_equal(cuts, want_flags >> 1) and cuts.tolist() == [0, 0, 0, 0, 1, 0, 1, 0, 0] and not over.any()
    two = on.track_report()
    assert len(two) == 2 and np.array_equal(two[1], over)                                                # the two return values stay
    in_place, _ = mc.clip_tracks(masks, 3, 4, 20, mvs, fsize, 64, 2, compensate=False)
    assert any(not np.array_equal(g, w) for g, w in zip(got, in_place))                                   # the vectors do matter here
    assert all((g[:, 2] == -1).all() for g in (got[4], got[6])) and sum(int((g[:, 2] >= 0).sum()) for g in got) > 5
    # reset(): the next frame has no frame before it, so its vectors -- and a cut flag -- are ignored
    on.reset()
    stats[9, 2] = 1
    kept.append(on.predict_window(x, x, grids, grids, link_mvs=t(mvs[9:]), link_frame_size=fsize, link_stats=t(stats[9:])))
    want, want_flags = mc.clip_tracks(np.concatenate(kept), 3, 4, 20, mvs, fsize, 64, 2, resets=(9,), stats=stats)
    got, over, cuts = on.track_report(with_cuts=True)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and cuts[9] == 0 and want_flags[9] == 0 and (got[9][:, 1:3] == -1).all()
    # without link_stats the same windows have no cuts; without link_mvs a window raises, it is never linked in place
    plain = FlowPredictor(StubFlow(), track=True, compensate=True, **kw)
    plain.predict_window(x, x, grids, grids, link_mvs=t(mvs[:3]), link_frame_size=fsize)
    assert called[-1] == (3, False, (3, 6, 7), fsize, None)
    n_calls = len(called)
    for bad in (dict(), dict(link_mvs=t(mvs[:3])), dict(link_frame_size=fsize), dict(link_mvs=t(mvs[:2]), link_frame_size=fsize),
                dict(link_mvs=t(mvs[:3]), link_frame_size=fsize, link_stats=t(stats[:2]))):
        with pytest.raises(ValueError, match="link_"):
            plain.predict_window(x, x, grids, grids, **bad)
    assert len(called) == n_calls and len(plain.track_report()[0]) == 3
    item = dict(frame_prev=x, frame_next=x, mvs_left=grids, mvs_right=grids, link_mvs=t(mvs[3:6]), link_frame_size=fsize, link_stats=t(stats[3:6]))
    list(plain.predict_clip([item]))                                                                      # predict_clip passes the item's keys through
    assert called[n_calls:] == [(1, True, (1, 6, 7), fsize, (1, 4)), (2, True, (2, 6, 7), fsize, (2, 4))]
    with pytest.raises(ValueError, match="link_"):
        list(plain.predict_clip([dict(frame_prev=x, frame_next=x, mvs_left=grids, mvs_right=grids)]))


def test_grid_estimator_hands_out_the_tables_of_one_search_per_pair(monkeypatch):
    """ops.block_match / block_match_modes and the table -> grid step are replaced by host stubs that count their calls."""
    searches, produced = [], []
    frames = {i: torch.full((32, 48), i, dtype=torch.uint8) for i in range(7)}

    def table_of(cur, ref_):
        return torch.from_numpy(mc._rows(32, 48, int(cur[0, 0]), int(ref_[0, 0]))).clone()

    def block_match(cur, ref_, search=16, penalty=0, return_cost=False):
        searches.append((int(ref_[0, 0]), int(cur[0, 0])))
        return table_of(cur, ref_)

    def block_match_modes(cur, ref_, search=16, penalty=0, intra_bias=65535, scene_cut=None, return_stats=False):
        searches.append((int(ref_[0, 0]), int(cur[0, 0])))
        return table_of(cur, ref_), torch.tensor([6, 0, int(cur[0, 0]) == 3, 0], dtype=torch.int32)

    def to_grids(table, h, w, validate=True):
        produced.append(int(table[0, 3]) - int(table[0, 5]))
        return table.double(), -table.double()

    monkeypatch.setattr(ops, "block_match", block_match)
    monkeypatch.setattr(ops, "block_match_modes", block_match_modes)
    monkeypatch.setattr(motion, "motion_vectors_to_grids", to_grids)
    monkeypatch.setattr(motion, "check_geometry", lambda h, w: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    load = frames.get
    est = motion.GridEstimator(search=8)
    first = est.table_for(0, load)
    assert first.dtype == torch.int32 and first.shape == (6, 7) and (first == torch.tensor(mc.VOID_ROW, dtype=torch.int32)).all() and searches == []
    g2 = est.grids_for(2, load)
    t2 = est.table_for(2, load)
    assert searches == [(1, 2)] and torch.equal(t2, table_of(frames[2], frames[1])) and torch.equal(g2[0], t2.double())   # one search serves both
    t4 = est.table_for(4, load)
    assert est.grids_for(4, load)[0].equal(t4.double()) and searches == [(1, 2), (3, 4)] and est.table_for(4, load) is t4    # ... whichever is asked first
    tables = est.window_tables(2, 3, load)
    assert tables.shape == (3, 6, 7) and tables.dtype == torch.int32 and searches == [(1, 2), (3, 4), (2, 3)]
    assert torch.equal(tables[0], t2) and torch.equal(tables[1], table_of(frames[3], frames[2])) and torch.equal(tables[2], t4)
    assert est.window_link_stats(2, 3) is None and est.window_tables(0, 2, load).shape == (2, 6, 7) and searches[3:] == [(0, 1)]
    missing = dict(frames)
    del missing[4]
    est.reset()
    assert (est.table_for(5, missing.get) == torch.tensor(mc.VOID_ROW, dtype=torch.int32)).all()         # the predecessor is missing
    with pytest.raises(FileNotFoundError):
        est.table_for(9, load)
    # with the decisions on: the stats rows of the same pairs, and hold_cuts' closing pair is the next window's first pair
    del searches[:]
    cut = motion.GridEstimator(search=8, intra_bias=0, scene_cut=0.5)
    cut.grids_for(1, load), cut.grids_for(2, load)
    stats = cut.window_stats(0, 3, load)                                                                   # pairs 1, 2, 3: the closing pair is searched here
    assert searches == [(0, 1), (1, 2), (2, 3)] and [int(s[2]) for s in stats] == [0, 0, 1]
    tables = cut.window_tables(3, 3, load)                                                                 # pairs 3, 4, 5
    assert searches == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)] and torch.equal(tables[0], table_of(frames[3], frames[2]))
    assert cut.window_link_stats(3, 3)[:, 2].tolist() == [1, 0, 0] and cut.window_link_stats(3, 3).dtype == torch.int32
    first = cut.window_tables(0, 3, load)
    assert (first[0] == torch.tensor(mc.VOID_ROW, dtype=torch.int32)).all() and cut.window_link_stats(0, 3).tolist() == [[0, 0, 0, 0], [6, 0, 0, 0], [6, 0, 0, 0]]
    # estimate_grids itself is as it was: a search and the grids of its table
    del searches[:]
    grid, inv = motion.estimate_grids(frames[2], frames[1], search=8)
    assert searches == [(1, 2)] and torch.equal(grid, table_of(frames[2], frames[1]).double()) and torch.equal(inv, -grid)
    assert len(motion.estimate_grids(frames[2], frames[1], search=8, intra_bias=0, return_stats=True)) == 3


def test_datasets_carry_the_link_keys(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="vectors"):
        dataset.PredictWindows(str(tmp_path), "v", grids="files", link_vectors=True)
    fh, fw, delta = 32, 48, 3
    path = str(tmp_path / "clip.rgb")
    np.repeat(np.arange(7, dtype=np.uint8), fh * fw * 3).tofile(path)
    monkeypatch.setattr(ops, "prepare_frame", lambda frame, size, mean, std, **kw: torch.zeros(1, 3, fh, fw))
    monkeypatch.setattr(ops, "frame_planes", lambda buf, h, w, fmt: (buf.view(h, w, 3), None))
    monkeypatch.setattr(ops, "block_match", lambda cur, ref_, search=16, penalty=0, return_cost=False: torch.from_numpy(mc._rows(fh, fw, int(cur[0, 0, 0]), int(ref_[0, 0, 0]))))
    monkeypatch.setattr(ops, "block_match_modes", lambda cur, ref_, search=16, penalty=0, intra_bias=65535, scene_cut=None, return_stats=False: (
        torch.from_numpy(mc._rows(fh, fw, int(cur[0, 0, 0]), int(ref_[0, 0, 0]))), torch.tensor([6, 1, int(cur[0, 0, 0]) == 4, 0], dtype=torch.int32)))
    off = dataset.RawVideoWindows(path, fh, fw, "rgb24", frame_delta=delta, no_warp=True, device="cpu")
    assert off.link_vectors is False and not any(k.startswith("link_") for k in off[1])
    ds = dataset.RawVideoWindows(path, fh, fw, "rgb24", frame_delta=delta, no_warp=True, device="cpu", link_vectors=True)
    item = ds[1]                                                                                          # emits frames 3, 4, 5
    assert item["link_frame_size"] == (fh, fw) and item["link_mvs"].shape == (delta, 6, 7) and item["link_mvs"].dtype == torch.int32 and "link_stats" not in item
    assert [int(m[0, 3] - m[0, 5]) for m in item["link_mvs"]] == [3, 4, 5] and [int(m[0, 4] - m[0, 6]) for m in item["link_mvs"]] == [2, 3, 4]
    assert (ds[0]["link_mvs"][0] == torch.tensor(mc.VOID_ROW, dtype=torch.int32)).all()
    ds = dataset.RawVideoWindows(path, fh, fw, "rgb24", frame_delta=delta, no_warp=True, device="cpu", link_vectors=True, intra_bias=0, scene_cut=0.5)
    item = ds[1]
    assert item["link_stats"].shape == (delta, 4) and item["link_stats"][:, 2].tolist() == [0, 1, 0]


def test_tool_refuses_compensate_without_tracks_or_vectors(capsys):
    spec = importlib.util.spec_from_file_location("predict_video_tool_mc", os.path.join(ROOT, "tools", "predict_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw = ["--raw", "c.rgb", "--raw-size", "1072", "1920", "--synthetic-weights"]
    a = tool.parse_args(raw + ["--regions", "r.csv", "--tracks", "t.csv", "--compensate"])
    assert a.compensate and a.grids == "estimate" and not tool.parse_args(raw + ["--regions", "r.csv", "--tracks", "t.csv"]).compensate
    assert tool.parse_args(["--data-root", "d", "--synthetic-weights", "--grids", "estimate", "--regions", "r.csv", "--tracks", "t.csv", "--compensate"]).compensate
    capsys.readouterr()
    for bad, word in ((raw + ["--regions", "r.csv", "--compensate"], "--compensate needs --tracks"),
                      (raw + ["--compensate"], "--compensate needs --tracks"),
                      (["--data-root", "d", "--synthetic-weights", "--regions", "r.csv", "--tracks", "t.csv", "--compensate"], "hold grids"),
                      (["--data-root", "d", "--synthetic-weights", "--grids", "files", "--regions", "r.csv", "--tracks", "t.csv", "--compensate"], "hold grids")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert word in capsys.readouterr().err, bad
