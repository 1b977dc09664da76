"""The distance ops on the GPU (ops.mask_distance, ops.region_proximity) against the numpy definition of
tests/distance_ref.py, bit for bit: every shared case at every radius, with and without the nearest plane, with one and with several
source classes; the tabulation with an ample and with a too small region cap, one and eight thresholds; every buffer inside guarded
planes; one HIP-graph capture; and end to end through FlowPredictor(regions=True, track=True, proximity=...)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distance_ref as dref
import regions_ref as rref
import tracks_ref as tref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import PALETTE, FlowPredictor, write_exposure_csv, write_regions_csv, write_tracks_csv
from test_gpu_regions import DELTA, FH, FRAMES, FW, Guarded, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = range(len(dref.case_list()))
NONE = dref.NONE


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared expectations are read-only


def ids(source_set):
    return [k for k in range(32) if (source_set >> k) & 1]


def distance(mask, source_set, max_dist=0, want_nearest=True):
    """ops.mask_distance on a numpy mask -> numpy (d2 as uint32, nearest or None)."""
    d2, nearest = ops.mask_distance(dev(mask), ids(source_set), max_dist, want_nearest)
    return d2.cpu().numpy().view(np.uint32), None if nearest is None else nearest.cpu().numpy()


@pytest.mark.parametrize("i", CASES)
def test_every_case_equals_the_definition(i):
    """d2 and nearest everywhere, at every radius; a capped call equals the uncapped one wherever it is not FS_DIST_NONE."""
    mask = dref.case_list()[i]["mask"]
    for source_set in dref.SOURCE_SETS:
        free = None
        for r in dref.RADII:
            want_d2, want_nearest = dref.expected(i, source_set, r)
            d2, nearest = distance(mask, source_set, r)
            assert np.array_equal(d2, want_d2) and np.array_equal(nearest, want_nearest), (source_set, r)
            alone, nothing = distance(mask, source_set, r, want_nearest=False)
            assert nothing is None and np.array_equal(alone, want_d2), (source_set, r)
            if r == 0:
                free = (d2, nearest)
            else:
                kept = d2 != NONE
                assert np.array_equal(d2[kept], free[0][kept]) and np.array_equal(nearest[kept], free[1][kept])
                assert (nearest[~kept] == -1).all() and (free[0][~kept].astype(np.int64) > r * r).all()


def proximity(i, source_set, max_dist, cap, thresholds, with_nearest=True):
    mask = dref.case_list()[i]["mask"]
    d2, nearest = dref.expected(i, source_set, max_dist)
    index, counts = dref.region_tables(i)[cap]
    exposure, near = ops.region_proximity(dev(mask), dev(d2.view(np.int32)), dev(nearest) if with_nearest else None, dev(index), dev(counts), dref.K, cap,
                                          ids(dref.TARGET_SET & 0x1F) + [7], thresholds)
    return exposure.cpu().numpy(), near.cpu().numpy()


@pytest.mark.parametrize("i", CASES)
def test_the_tabulation_equals_the_definition(i):
    """An ample cap and one of seven rows, eight thresholds and one, a capped field and the free one, with and without nearest."""
    for source_set, max_dist, cap, thresholds, with_nearest in ((dref.SOURCE_SETS[0], 0, dref.ample_cap(i), dref.THRESHOLDS_8, True),
                                                                (dref.SOURCE_SETS[1], 7, dref.ample_cap(i), dref.THRESHOLDS_1, True),
                                                                (dref.SOURCE_SETS[1], 0, dref.SMALL_CAP, dref.THRESHOLDS_8, False),
                                                                (dref.SOURCE_SETS[0], 2, dref.SMALL_CAP, dref.THRESHOLDS_1, True)):
        want = dref.expected_proximity(i, source_set, max_dist, cap, thresholds, with_nearest)
        got = proximity(i, source_set, max_dist, cap, thresholds, with_nearest)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (source_set, max_dist, cap, thresholds, with_nearest)


@pytest.mark.parametrize("geometry", [(37, 301), (67, 120), (3, 1500)])
def test_nothing_outside_the_buffers_is_touched(geometry):
    """Every buffer inside a guarded plane, the mask at an odd byte offset, both ops through the library itself."""
    i = [j for j, c in enumerate(dref.case_list()) if c["geometry"] == geometry and c["patterns"][0] == "random01"][0]
    mask = dref.case_list()[i]["mask"]
    n, h, w = mask.shape
    cap, thresholds, source_set = dref.SMALL_CAP, dref.THRESHOLDS_8, dref.SOURCE_SETS[1]
    index_np, counts_np = dref.region_tables(i)[cap]
    lib = _lib.load()
    for with_nearest in (True, False):
        m = Guarded((n, h, w), torch.uint8, 3)
        m.view.copy_(dev(mask))
        d2, nearest, index = Guarded((n, h, w), torch.int32, 1), Guarded((n, h, w), torch.int32, 3), Guarded((n, h, w), torch.int32, 1)
        work = Guarded((ops.mask_distance_workspace_bytes(n, h, w) // 4,), torch.int32, 1)
        counts, exposure, near = Guarded((n, 2), torch.int64, 1), Guarded((n, dref.K, len(thresholds)), torch.int64, 3), Guarded((n, cap, 8), torch.int64, 1)
        index.view.copy_(dev(index_np))
        counts.view.copy_(dev(counts_np))
        host = (ctypes.c_int32 * len(thresholds))(*thresholds)
        check(lib.fs_mask_distance(ptr(m.view), n, h, w, source_set, 7, ptr(d2.view), ptr(nearest.view) if with_nearest else None, ptr(work.view),
                                   stream_ptr()))
        check(lib.fs_region_proximity(ptr(m.view), ptr(d2.view), ptr(nearest.view) if with_nearest else None, ptr(index.view), ptr(counts.view), n, h, w,
                                      dref.K, cap, dref.TARGET_SET, ctypes.cast(host, ctypes.c_void_p), len(thresholds),
                                      ptr(exposure.view), ptr(near.view), stream_ptr()))
        torch.cuda.synchronize()
        want_d2, want_nearest = dref.expected(i, source_set, 7)
        assert np.array_equal(d2.view.cpu().numpy().view(np.uint32), want_d2)
        if with_nearest:
            assert np.array_equal(nearest.view.cpu().numpy(), want_nearest)
        want = dref.expected_proximity(i, source_set, 7, cap, thresholds, with_nearest)
        assert np.array_equal(exposure.view.cpu().numpy(), want[0]) and np.array_equal(near.view.cpu().numpy(), want[1])
        assert all(g.intact() for g in (m, d2, nearest, index, work, counts, exposure, near))
        if not with_nearest:
            assert (nearest.view == nearest.guard).all()                    # a NULL plane is not written anywhere else either


def test_cpu_side_checks_of_the_arguments():
    mask = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    plane = torch.zeros((2, 8, 8), dtype=torch.int32, device=DEV)
    counts = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    for kw, word in ((dict(sources=()), "sources"), (dict(sources=(32,)), "32"), (dict(sources=(1,), max_dist=32768), "32768"),
                     (dict(sources=(1,), max_dist=-1), "-1"), (dict(sources=(1,), out=(plane[:1], plane)), "d2"),
                     (dict(sources=(1,), want_nearest=False, out=(plane, plane)), "want_nearest")):
        with pytest.raises(ValueError, match=word):
            ops.mask_distance(mask, **kw)
    with pytest.raises(ValueError, match="mask must be uint8"):
        ops.mask_distance(plane, (1,))
    good = dict(mask=mask, d2=plane, nearest=plane, index=plane, counts=counts, classes=5, max_regions=16, targets=(3,), thresholds=(1, 2))
    for kw, word in ((dict(thresholds=()), "thresholds"), (dict(thresholds=(2, 2)), "2, 2"), (dict(thresholds=(1, 40000)), "40000"),
                     (dict(thresholds=tuple(range(9))), "thresholds"), (dict(classes=0), "classes"), (dict(max_regions=65537), "65537"),
                     (dict(targets=(33,)), "33"), (dict(counts=counts[:1]), "counts"), (dict(d2=plane[:, :4]), "d2"), (dict(index=None), "index")):
        with pytest.raises(ValueError, match=word):
            ops.region_proximity(**{**good, **kw})
    d2, nearest = ops.mask_distance(mask[:0], (1,))
    assert d2.shape == (0, 8, 8) and nearest.shape == (0, 8, 8)


def test_a_captured_graph_replayed_on_new_planes_gives_each_replays_result():
    """Both ops in one graph on a single stream; the outputs are never cleared by the caller."""
    a, b = [j for j, c in enumerate(dref.case_list()) if c["geometry"] == (67, 120) and len(c["patterns"]) == 3][:2]
    ca, cb = dref.case_list()[a], dref.case_list()[b]
    n, h, w = ca["mask"].shape
    assert cb["mask"].shape == (n, h, w)
    cap, thresholds, source_set = dref.ample_cap(a), dref.THRESHOLDS_8, dref.SOURCE_SETS[0]
    lib = _lib.load()
    mask = dev(ca["mask"])
    index, counts = dev(dref.region_tables(a)[cap][0]), dev(dref.region_tables(a)[cap][1])
    d2 = torch.full((n, h, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    nearest = torch.full((n, h, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    work = torch.full((ops.mask_distance_workspace_bytes(n, h, w) // 4,), -1, dtype=torch.int32, device=DEV)
    exposure = torch.full((n, dref.K, len(thresholds)), -12345, dtype=torch.int64, device=DEV)
    near = torch.full((n, cap, 8), -12345, dtype=torch.int64, device=DEV)
    host = (ctypes.c_int32 * len(thresholds))(*thresholds)

    def launch():
        s = stream_ptr()
        check(lib.fs_mask_distance(ptr(mask), n, h, w, source_set, 0, ptr(d2), ptr(nearest), ptr(work), s))
        check(lib.fs_region_proximity(ptr(mask), ptr(d2), ptr(nearest), ptr(index), ptr(counts), n, h, w, dref.K, cap, dref.TARGET_SET,
                                      ctypes.cast(host, ctypes.c_void_p), len(thresholds), ptr(exposure), ptr(near), s))

    launch()                                                                # the kernels are loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for i in (b, a, b):
        mask.copy_(dev(dref.case_list()[i]["mask"]))
        index.copy_(dev(dref.region_tables(i)[cap][0]))
        counts.copy_(dev(dref.region_tables(i)[cap][1]))
        graph.replay()
        torch.cuda.synchronize()
        want_d2, want_nearest = dref.expected(i, source_set, 0)
        want = dref.expected_proximity(i, source_set, 0, cap, thresholds, True)
        assert np.array_equal(d2.cpu().numpy().view(np.uint32), want_d2) and np.array_equal(nearest.cpu().numpy(), want_nearest)
        assert np.array_equal(exposure.cpu().numpy(), want[0]) and np.array_equal(near.cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------------ through the predictor
def test_predictor_reports_the_definition_and_changes_nothing_else(clip):  # noqa: F811
    """Three windows of the synthetic model with regions and tracks: proximity_report() is the reference applied to the masks handed
    out; masks, region rows and tracks equal a run with proximity=None; clear_report() drops the tables, reset() keeps them."""
    size = (65, 65)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8)
    items = [ds[0], ds[1], ds[0]]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=True, cache_keyframes=False, regions=True, track=True, max_regions=64)
    args = [(i["frame_prev"], i["frame_next"], i["mvs_left"], i["mvs_right"]) for i in items]
    off = FlowPredictor(fm, proximity=None, **kw)
    plain = np.concatenate([off.predict_window(*a, to_host=False).cpu().numpy() for a in args])
    assert off.proximity_report()[1] == [] and off._proximity_chunks == []
    present = np.bincount(plain.reshape(-1), minlength=5)[:5]
    order = np.argsort(-present, kind="stable")
    assert present[order[1]] > 0, "the synthetic masks hold one class only: nothing to measure between"
    sources, targets = (int(order[1]),), tuple(int(k) for k in order if k != order[1])
    thresholds = (1, 3, 9)
    on = FlowPredictor(fm, proximity=thresholds, proximity_sources=sources, proximity_targets=targets, **kw)
    got = np.concatenate([on.predict_window(*a, to_host=False).cpu().numpy() for a in args])
    assert np.array_equal(got, plain) and torch.equal(on.hist, off.hist)
    rows, totals = on.region_report()
    rows_off, totals_off = off.region_report()
    assert all(np.array_equal(g, w_) for g, w_ in zip(rows, rows_off)) and np.array_equal(totals, totals_off)
    assert all(np.array_equal(g, w_) for g, w_ in zip(on.track_report()[0], off.track_report()[0]))
    assert on.proximity_max == 0                                                     # unbounded by default
    source_set = 1 << sources[0]
    target_set = sum(1 << k for k in targets)
    d2, nearest = dref.mask_distance(plain, source_set, on.proximity_max)
    _, counts, index = rref.region_table(plain, rref.mask_regions(plain, 5, 8), 5, None, 128, 64)
    want_exposure, want_near = dref.region_proximity(plain, d2, nearest, index, counts, 5, 64, target_set, thresholds)
    exposure, near = on.proximity_report()
    assert np.array_equal(exposure, want_exposure) and len(near) == len(plain) == len(rows)
    assert all(np.array_equal(g, want_near[f, :counts[f, 1]]) and len(g) == len(rows[f]) for f, g in enumerate(near))
    assert (d2 != NONE).any() and want_exposure.sum() > 0                            # not vacuous
    bound = FlowPredictor(fm, proximity=thresholds, proximity_sources=sources, proximity_targets=targets, proximity_max=9, **kw)
    bound.predict_window(*args[0], to_host=False)
    d2, nearest = dref.mask_distance(plain[:DELTA], source_set, 9)
    want_bound = dref.region_proximity(plain[:DELTA], d2, nearest, index[:DELTA], counts[:DELTA], 5, 64, target_set, thresholds)
    assert np.array_equal(bound.proximity_report()[0], want_bound[0]) and np.array_equal(want_bound[0], want_exposure[:DELTA])
    assert all(np.array_equal(g, want_bound[1][f, :counts[f, 1]]) for f, g in enumerate(bound.proximity_report()[1]))
    on.reset()                                                                       # a new video: the report stays
    assert len(on.proximity_report()[1]) == len(plain)
    on.clear_report()
    assert on.proximity_report()[1] == [] and on.proximity_report()[0].shape == (0, 5, 3)
    on.predict_window(*args[1], to_host=False)
    exposure, near = on.proximity_report()
    assert np.array_equal(exposure, want_exposure[DELTA:2 * DELTA]) and len(near) == DELTA


def test_predict_video_writes_the_proximity_columns_and_the_exposure_csv(clip, tmp_path):  # noqa: F811
    """The command-line tool is what this test is about: one child process, --regions --tracks --proximity --exposure on the synthetic clip;
    the three files are what the writers make of the reference applied to the masks the tool wrote."""
    size, frames = (65, 65), (FRAMES - 1) // DELTA * DELTA
    csv, tcsv, ecsv, out = str(tmp_path / "r.csv"), str(tmp_path / "t.csv"), str(tmp_path / "e.csv"), str(tmp_path / "m.rgb")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "predict_video.py"), "--raw", clip, "--raw-size", str(FH), str(FW), "--pix-fmt", "rgb24",
           "--search", "8", "--synthetic-weights", "--no-cropping", "--size", "65", "65", "--no-metrics", "--raw-out", out, "--out-pix-fmt", "rgb24",
           "--regions", csv, "--max-regions", "64", "--tracks", tcsv, "--proximity", "1", "3", "9", "--proximity-sources", "0", "1",
           "--proximity-targets", "2", "3", "4", "--proximity-max", "12", "--exposure", ecsv]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rgb = np.fromfile(out, np.uint8).reshape(frames, size[0], size[1], 3)     # opaque class colours: the masks, through the palette
    onehot = np.stack([(rgb == PALETTE[k]).all(-1) for k in range(5)], 1)
    assert (onehot.sum(1) == 1).all()
    masks = onehot.argmax(1).astype(np.uint8)
    table, counts, index = rref.region_table(masks, rref.mask_regions(masks, 5, 8), 5, None, 128, 64)
    rows = [table[f, :counts[f, 1]] for f in range(frames)]
    tracks, _ = tref.clip_tracks(masks, 5, 8, 64, None, 1)
    d2, nearest = dref.mask_distance(masks, 0b00011, 12)
    exposure, near = dref.region_proximity(masks, d2, nearest, index, counts, 5, 64, 0b11100, (1, 3, 9))
    nears = [near[f, :counts[f, 1]] for f in range(frames)]
    want, want_t, want_e = str(tmp_path / "want.csv"), str(tmp_path / "want_t.csv"), str(tmp_path / "want_e.csv")
    write_regions_csv(want, list(range(frames)), rows, with_confidence=False, tracks=tracks, proximity=nears)
    write_tracks_csv(want_t, list(range(frames)), rows, tracks, proximity=nears)
    write_exposure_csv(want_e, list(range(frames)), exposure, (1, 3, 9), size[0] * size[1])
    assert open(csv).read() == open(want).read() and open(tcsv).read() == open(want_t).read() and open(ecsv).read() == open(want_e).read()
    assert open(csv).readline().strip().endswith(",dist,near_px,nearest_region,nearest_track") and len(open(ecsv).read().splitlines()) == frames + 1
