"""ops.guide_vectors on the GPU against the numpy definition of tests/guide_ref.py, bit for bit: table-only on block grids
from one block to 67 x 120 under every kind of model, with void, foreign and garbage rows, in place and not; evidence mode on gray and
RGB frames, aligned and not, with a constant patch and a textured patch that moves against the pan; search, fit and guide from one
captured graph; GridEstimator(guide=True) end to end on a pan over textured ground with flat noisy water; FlowPredictor with the raw
tables; and the refusals."""
import functools
import gc
import os

import numpy as np
import pytest
import torch

import guide_ref as gref
import motion_ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow import motion
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor, write_guide_csv, write_mosaic_csv, write_regions_csv, write_tracks_csv
from test_gpu_regions import DELTA, FH, FRAMES, FW, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = gref.ONE
VOID = np.array(gref.VOID_ROW, np.int32)


@pytest.fixture(autouse=True)
def leave_nothing_behind():
    """Every test of this module ends with its work done and its garbage collected: predictors, estimators, graphs and their device
    memory are released HERE, not by a collection that happens to run inside a later test's stream capture."""
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ table only
@functools.lru_cache(maxsize=None)
def table_case(fh, fw, n):
    """n pairs of one geometry: the issue's models in turn, each with an adversarial table -> (tables, model), read-only."""
    names = list(gref.models(fh, fw))
    rows = [gref.models(fh, fw)[names[f % len(names)]] for f in range(n)]
    tables = np.stack([gref.adversarial_table(rows[f], fh, fw, 50 + f) for f in range(n)])
    model = np.array(rows, dtype=np.int64)
    tables.setflags(write=False), model.setflags(write=False)
    return tables, model


@pytest.mark.parametrize("size,n", [((64, 96), 1), ((64, 96), 3), ((64, 96), 64), ((70, 100), 3), ((70, 100), 64), ((16, 16), 1), ((16, 16), 64), ((1072, 1920), 1)])
def test_table_only_equals_the_reference(size, n):
    fh, fw = size
    if n == 1:                                                             # one pair at a time: every model of the issue
        cases = [(gref.adversarial_table(M, fh, fw, 9)[None], np.array([M], np.int64)) for M in gref.models(fh, fw).values()]
    else:
        cases = [table_case(fh, fw, n)]
    big = fh > 1000
    for tables, model in [cases[i] for i in (1, 3, 7)] if big else cases:     # at 8040 rows: the shift, the rotation, the garbage row
        for fill_void in (True, False):
            for outlier in ([1.0] if big else [None, 0, 1.0, 2.5]):
                want, want_counts = gref.guide_vectors(tables, model, fh, fw, int(fill_void), gref.outlier_q20(outlier))
                out, counts = ops.guide_vectors(dev(tables), dev(model), size, fill_void=fill_void, outlier=outlier)
                assert np.array_equal(host(out), want) and np.array_equal(host(counts), want_counts), (size, n, fill_void, outlier)
                t = dev(tables)                                            # out aliasing mv
                same, counts = ops.guide_vectors(t, dev(model), size, fill_void=fill_void, outlier=outlier, out=t)
                assert same is t and np.array_equal(host(t), want) and np.array_equal(host(counts), want_counts)
                poisoned = torch.full(tables.shape, -77, dtype=torch.int32, device=DEV)
                ops.guide_vectors(dev(tables), dev(model), size, fill_void=fill_void, outlier=outlier, out=poisoned)
                assert np.array_equal(host(poisoned), want)               # every row is written
    assert want_counts[:, 0].tolist() == [(fh // 16) * (fw // 16)] * len(model)


def test_the_consequences_on_the_device():
    fh, fw = 70, 100
    tables, model = table_case(fh, fw, 64)
    out, counts = ops.guide_vectors(dev(tables), dev(model), (fh, fw), fill_void=False, outlier=None)
    assert np.array_equal(host(out), tables) and (host(counts)[:, 2:7] == 0).all()                       # a copy
    out, counts = ops.guide_vectors(dev(tables), dev(model), (fh, fw), fill_void=True, outlier=0)
    failed = np.array([not gref.pair_guides(m) for m in model])
    assert failed.sum() >= 16 and np.array_equal(host(out)[failed], tables[failed]) and (host(counts)[failed][:, 2:7] == 0).all()
    again, counts2 = ops.guide_vectors(out, dev(model), (fh, fw), fill_void=True, outlier=0)
    assert torch.equal(again, out) and (host(counts2)[:, 2] == 0).all() and (host(counts2)[:, 5] == 0).all()   # idempotent, fills nothing
    M = gref.rotation_model(fh, fw)
    own = gref.model_table(M, fh, fw)[None]
    out, counts = ops.guide_vectors(dev(own), dev(np.array([M], np.int64)), (fh, fw), outlier=0.5)
    assert np.array_equal(host(out), own) and host(counts)[0, 3] == 0
    pdx = own[0, :, 3] - own[0, :, 5]
    assert pdx.min() < 0 < pdx.max()                                       # the rotation's vectors change sign across the grid


# ------------------------------------------------------------------------------------------------ evidence
@functools.lru_cache(maxsize=None)
def evidence_case(fh, fw, channels, penalty):
    """Two pairs (two seeds) of the evidence scene, searched on the CPU: (cur, ref, tables, cost, model of the pan), read-only."""
    pairs = [gref.evidence_scene(fh, fw, channels, seed=seed) for seed in (3, 4)]
    cur, ref = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    searched = [motion_ref.block_match(c, r, search=8, penalty=penalty) for c, r in pairs]
    tables, cost = np.stack([s[0] for s in searched]), np.stack([s[1] for s in searched])
    model = np.array([gref.shift_model(3, -2)] * 2, np.int64)
    for a in (cur, ref, tables, cost, model):
        a.setflags(write=False)
    return cur, ref, tables, cost, model


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [(64, 96), (66, 98)])
@pytest.mark.parametrize("penalty", [0, 7])
def test_evidence_mode(size, channels, penalty):
    fh, fw = size
    wb = fw // 16
    cur, ref, tables, cost, model = evidence_case(fh, fw, channels, penalty)
    d_cur, d_ref = dev(cur), dev(ref)
    for f in range(2):                                                     # the matcher on the device finds what the reference found
        t, c = ops.block_match(d_cur[f], d_ref[f], search=8, penalty=penalty, return_cost=True)
        assert np.array_equal(host(t), tables[f]) and np.array_equal(host(c), cost[f])
    flat, patch = 2 * wb + 1, 1 * wb + 4                                   # the constant block (2, 1) and the textured patch (1, 4)
    lc, lr = motion_ref.luma(cur[0]), motion_ref.luma(ref[0])
    cx, cy = gref.centres(fh, fw)
    sad_flat = gref.block_sad(lc, lr, int(cx[flat]), int(cy[flat]), 3, -2)
    sad_patch = gref.block_sad(lc, lr, int(cx[patch]), int(cy[patch]), 3, -2)
    assert sad_flat == 0 and cost[0, flat] == 0 and tables[0, flat].tolist() == [-1, 16, 16, cx[flat], cy[flat], cx[flat], cy[flat]]   # every SAD is 0 there
    assert tables[0, patch].tolist() == [-1, 16, 16, cx[patch] - 5, cy[patch] + 4, cx[patch], cy[patch]] and cost[0, patch] == 9 * penalty
    need_flat, need_patch = sad_flat + 5 * penalty - int(cost[0, flat]), sad_patch + 5 * penalty - int(cost[0, patch])
    assert need_flat == 5 * penalty and 10000 < need_patch <= 65535
    guide_flat = [-1, 16, 16, cx[flat] + 3, cy[flat] - 2, cx[flat], cy[flat]]
    guide_patch = [-1, 16, 16, cx[patch] + 3, cy[patch] - 2, cx[patch], cy[patch]]
    for bias in sorted({0, need_flat - 1, need_flat, need_patch - 1, need_patch, 65535} - {-1}):
        want, want_counts = gref.guide_vectors(tables, model, fh, fw, 1, 0, cur, ref, cost, penalty, bias)
        out, counts = ops.guide_vectors(dev(tables), dev(model), size, outlier=0, cur=d_cur, ref=d_ref, cost=dev(cost), penalty=penalty, guide_bias=bias)
        assert np.array_equal(host(out), want) and np.array_equal(host(counts), want_counts), (bias, host(counts), want_counts)
        got = host(out)[0]
        assert (got[flat].tolist() == guide_flat) == (bias >= need_flat) and (got[patch].tolist() == guide_patch) == (bias >= need_patch)
        assert bias >= need_flat or np.array_equal(got[flat], tables[0, flat])
        assert bias >= need_patch or np.array_equal(got[patch], tables[0, patch])                       # kept by evidence: the winner stays
        assert (want_counts[:, 4] + want_counts[:, 5] + want_counts[:, 6] == want_counts[:, 3]).all()
    assert want_counts[0, 6] == 0                                          # at the largest bias nothing is kept
    # without the frames the same outliers are replaced as they stand
    out, counts = ops.guide_vectors(dev(tables), dev(model), size, outlier=0)
    assert host(out)[0, patch].tolist() == guide_patch and host(counts)[0, 6] == 0


@pytest.mark.parametrize("channels", [1, 3])
def test_evidence_with_frame_planes_that_are_not_dword_aligned(channels):
    """FW % 4 == 0 but the planes start one byte past a dword: the other way into the byte loads of cur (and the usual one for ref)."""
    fh, fw = 64, 96
    cur, ref, tables, cost, model = evidence_case(fh, fw, channels, 7)

    def off_by_one(a):
        buf = torch.zeros(a.size + 5, dtype=torch.uint8, device=DEV)
        start = 1 + (-buf.data_ptr()) % 4                                  # one byte past a dword, wherever the buffer begins
        view = buf[start:start + a.size].view(a.shape)
        view.copy_(dev(a))
        assert view.data_ptr() % 4 == 1 and view.is_contiguous()
        return view

    d_cur, d_ref = off_by_one(cur), off_by_one(ref)
    for bias in (0, 30000, 65535):
        want, want_counts = gref.guide_vectors(tables, model, fh, fw, 1, 0, cur, ref, cost, 7, bias)
        out, counts = ops.guide_vectors(dev(tables), dev(model), (fh, fw), outlier=0, cur=d_cur, ref=d_ref, cost=dev(cost), penalty=7, guide_bias=bias)
        assert np.array_equal(host(out), want) and np.array_equal(host(counts), want_counts), bias
    assert want_counts[:, 4].sum() > 0


# ------------------------------------------------------------------------------------------------ one graph: search, fit, guide
def test_search_fit_and_guide_replay_from_one_graph():
    fh, fw = 64, 96
    blocks = 24
    lib = _lib.load()
    scenes = [gref.flat_scene(fh, fw, pan=pan, seed=seed) for pan, seed in (((20, 0), 5), ((-6, 3), 6), ((2, -9), 7))]
    cur, ref = dev(scenes[0][0]), dev(scenes[0][1])
    mv = torch.empty((1, blocks, 7), dtype=torch.int32, device=DEV)
    cost = torch.empty((1, blocks), dtype=torch.int32, device=DEV)
    stats = torch.empty((1, 4), dtype=torch.int32, device=DEV)
    model = torch.empty((1, 16), dtype=torch.int64, device=DEV)
    out = torch.empty_like(mv)
    counts = torch.empty((1, 8), dtype=torch.int64, device=DEV)

    def launch():
        s = stream_ptr()
        check(lib.fs_block_match_modes(ptr(cur), ptr(ref), fh, fw, 1, 24, 1, 0, 1000, ptr(mv), ptr(cost), None, ptr(stats), s))
        check(lib.fs_global_motion(ptr(mv), ptr(stats), None, 0, 1, fh, fw, fh, fw, 4, ONE, 6, ptr(model), s))
        check(lib.fs_guide_vectors(ptr(mv), ptr(model), 1, fh, fw, 1, ONE, ptr(cur), ptr(ref), 1, ptr(cost), 1, 0, ptr(out), ptr(counts), s))

    launch()                                                               # the kernels are loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for c, r in scenes:
        cur.copy_(dev(c)), ref.copy_(dev(r))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [host(t).copy() for t in (mv, model, out, counts)]
        for t in (mv, model, out, counts):
            t.fill_(-3)
        launch()
        torch.cuda.synchronize()
        assert all(np.array_equal(a, host(t)) for a, t in zip(replayed, (mv, model, out, counts)))
        want, want_counts = gref.guide_vectors(replayed[0], replayed[1], fh, fw, 1, ONE, c[None], r[None], host(cost), 1, 0)
        assert np.array_equal(replayed[2], want) and np.array_equal(replayed[3], want_counts) and replayed[1][0, 12] == 0 and want_counts[0, 2] > 0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("size", [(64, 96), (1072, 1920)])
def test_grid_estimator_fills_flat_water_with_the_pan(size):
    fh, fw = size
    hb, wb = fh // 16, fw // 16
    pan = (20, 0)
    cur, ref = gref.flat_scene(fh, fw, pan=pan, seed=5)
    frames = {0: dev(ref), 1: dev(cur)}
    rect = [by * wb + bx for by in (1, 2) for bx in (1, 2)]
    kw = dict(search=24, intra_bias=0)
    plain = motion.GridEstimator(**kw)
    raw = host(plain.table_for(1, frames.get))
    assert (raw[rect] == VOID).all()                                       # without guidance the water's rows are void ...
    guided = motion.GridEstimator(guide=True, guide_min_inliers=6, **kw)
    table = host(guided.table_for(1, frames.get))
    assert np.array_equal(host(guided.raw_table_for(1, frames.get)), raw)
    cx, cy = gref.centres(fh, fw)
    avail = np.array([gref.available(pan[0], pan[1], int(x), int(y), fh, fw) for x, y in zip(cx, cy)])
    want = np.tile(VOID, (hb * wb, 1))
    want[avail] = np.stack([np.full(avail.sum(), -1), np.full(avail.sum(), 16), np.full(avail.sum(), 16), cx[avail] + pan[0], cy[avail] + pan[1], cx[avail], cy[avail]], 1)
    assert avail[rect].all() and np.array_equal(table[avail], want[avail])  # ... with it every block the camera's vector can serve carries the pan
    model = host(ops.global_motion(dev(raw[None]), size, size, 4, 1.0, 6, pair_stats=guided.stats_for(1)[None]))
    assert model[0, :6].tolist() == [ONE, 0, pan[0] * ONE, 0, ONE, pan[1] * ONE] and model[0, 12] == 0
    ref_table, ref_counts = gref.guide_vectors(raw[None], model, fh, fw, 1, -1)
    assert np.array_equal(table, ref_table[0]) and np.array_equal(host(guided.guide_counts_for(1)), ref_counts[0]) and ref_counts[0, 2] >= len(rect)
    if size == (1072, 1920):                                               # the grid producer's own geometry: the grids of the guided table
        with torch.cuda.device(frames[0].device):
            g_plain, g_guided = plain.grids_for(1, frames.get), guided.grids_for(1, frames.get)
            from_pan = motion.motion_vectors_to_grids(dev(np.where(avail[:, None], want, table)), fh, fw, validate=False)
            identity = motion.motion_vectors_to_grids(dev(np.tile(VOID, (hb * wb, 1))), fh, fw, validate=False)
        assert all(torch.equal(a, b) for a, b in zip(g_guided, from_pan))
        cells = [(by, bx) for by in (1, 2) for bx in (1, 2)]
        kept = [all(torch.equal(g_plain[i][by, bx], identity[i][by, bx]) for by, bx in cells) for i in (0, 1)]
        assert any(kept)                                                   # unguided: in the grid that is indexed by the block, the water keeps the identity
        assert not any(torch.equal(g_guided[kept.index(True)][by, bx], identity[kept.index(True)][by, bx]) for by, bx in cells)


@pytest.fixture(scope="module")
def lake_clip(tmp_path_factory):
    """A raw RGB video at the grid producer's geometry: textured ground panning by (8, 0) px a frame with a flat, noisy grey lake of
    20 x 30 blocks that stays where it is in the frame: with intra_bias = 0 the lake's blocks are void rows, which guidance fills."""
    rng = np.random.RandomState(77)
    ground = rng.randint(0, 256, size=(FH, FW + 8 * FRAMES, 3)).astype(np.uint8)
    path = str(tmp_path_factory.mktemp("guide") / "lake.rgb")
    with open(path, "wb") as fh:
        for i in range(FRAMES):
            frame = np.ascontiguousarray(ground[:, 8 * i:8 * i + FW])
            frame[320:640, 480:960] = (100 + rng.randint(-3, 4, size=(320, 480)))[..., None]
            fh.write(frame.tobytes())
    return path


SIZE = (65, 65)
IDS = list(range(2 * DELTA))
WINDOWS = dict(size=SIZE, frame_delta=DELTA, grids="estimate", search=12, link_vectors=True, intra_bias=0)
EVERYTHING = dict(classes=5, out_size=SIZE, crop=None, compute_metrics=True, cache_keyframes=False, regions=True, track=True, compensate=True, stabilize=3,
                  stabilize_compensate=True, mosaic=(96, 120), mosaic_min_inliers=6, mosaic_exclude=())


def run_windows(ds, fm, folder, **kw):
    """Two windows through a predictor -> (items, masks, mosaic report, stabiliser counts, guide report, {csv name: its bytes})."""
    pred = FlowPredictor(fm, **kw)
    items = [ds[0], ds[1]]
    masks = np.concatenate([host(pred.predict_window(i["frame_prev"], i["frame_next"], i["mvs_left"], i["mvs_right"], to_host=False, link_mvs=i["link_mvs"],
                                                     link_frame_size=i["link_frame_size"], link_stats=i.get("link_stats"), link_raw_mvs=i.get("link_raw_mvs"),
                                                     link_guide_counts=i.get("link_guide_counts"))) for i in items])
    rows, _ = pred.region_report()
    tracks = pred.track_report()[0] if kw.get("track") else None
    mosaic = pred.mosaic_report()
    os.makedirs(folder, exist_ok=True)
    write_regions_csv(os.path.join(folder, "regions.csv"), IDS, rows, with_confidence=False, tracks=tracks)
    if tracks is not None:
        write_tracks_csv(os.path.join(folder, "tracks.csv"), IDS, rows, tracks)
    write_mosaic_csv(os.path.join(folder, "mosaic.csv"), IDS, mosaic[4], mosaic[3])
    write_guide_csv(os.path.join(folder, "guide.csv"), IDS[:len(pred.guide_report())], pred.guide_report())
    files = {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}
    return items, masks, mosaic, pred.stabilize_report() if kw.get("stabilize") else None, pred.guide_report(), files


def test_with_guidance_off_masks_reports_and_csvs_are_byte_identical(lake_clip, tmp_path):
    """The new arguments left out, and given as their defaults: the same items, masks, reports and CSV files, byte for byte, with
    everything that reads the tables switched on (warped grids, compensated links, compensated stabiliser, mosaic)."""
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    before = run_windows(RawVideoWindows(lake_clip, FH, FW, "rgb24", **WINDOWS), fm, str(tmp_path / "before"), **EVERYTHING)
    off = run_windows(RawVideoWindows(lake_clip, FH, FW, "rgb24", guide=False, guide_outlier=None, guide_bias=None, **WINDOWS), fm, str(tmp_path / "off"), **EVERYTHING)
    assert all(set(a) == set(b) and "link_raw_mvs" not in b and "link_guide_counts" not in b for a, b in zip(before[0], off[0]))
    assert all(torch.equal(a["link_mvs"], b["link_mvs"]) and all(torch.equal(x, y) for x, y in zip(a["mvs_left"], b["mvs_left"])) for a, b in zip(before[0], off[0]))
    assert np.array_equal(before[1], off[1]) and all(np.array_equal(a, b) for a, b in zip(before[2], off[2])) and np.array_equal(before[3], off[3])
    assert before[4].shape == off[4].shape == (0, 8)
    assert sorted(before[5]) == ["guide.csv", "mosaic.csv", "regions.csv", "tracks.csv"] and before[5] == off[5]       # the files, byte for byte
    assert len(before[5]["regions.csv"]) > 200 and len(before[5]["mosaic.csv"]) > 200 and (before[2][4][:, 12] == 0).sum() >= 2   # not vacuous


def test_with_guidance_on_the_fit_reads_the_raw_tables_and_guide_report_is_the_per_pair_counts(lake_clip, tmp_path, monkeypatch):
    """Warp mode with everything on.  The items carry the guided tables, the raw ones and the counts; tracks and stabiliser get the
    GUIDED tensor, the mosaic's fit the RAW one (the very tensors of the items); the poses are those of the run without guidance; and
    guide_report() is the reference's counts of every pair, computed from the raw table and the model fitted to it."""
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    off = run_windows(RawVideoWindows(lake_clip, FH, FW, "rgb24", **WINDOWS), fm, str(tmp_path / "off"), **EVERYTHING)
    seen = dict(fit=[], links=[], stabilize=[])
    real = dict(fit=ops.global_motion, links=ops.region_links, stabilize=ops.mask_stabilize)

    def global_motion(tables, *args, **kw):
        if kw.get("mask") is not None:                                     # the mosaic's fit (the estimator's own has no mask)
            seen["fit"].append(tables)
        return real["fit"](tables, *args, **kw)

    def region_links(*args, **kw):
        seen["links"].append(kw.get("mv"))
        return real["links"](*args, **kw)

    def mask_stabilize(*args, **kw):
        seen["stabilize"].append(kw.get("mv"))
        return real["stabilize"](*args, **kw)

    monkeypatch.setattr(ops, "global_motion", global_motion)
    monkeypatch.setattr(ops, "region_links", region_links)
    monkeypatch.setattr(ops, "mask_stabilize", mask_stabilize)
    ds = RawVideoWindows(lake_clip, FH, FW, "rgb24", guide=True, guide_outlier=1.0, **WINDOWS)
    items, masks, mosaic, _, report, files = run_windows(ds, fm, str(tmp_path / "on"), **EVERYTHING)
    monkeypatch.undo()
    assert [t is i["link_raw_mvs"] for t, i in zip(seen["fit"], items)] == [True, True]                   # the fit never feeds on rows a fit produced
    assert all(any(t is i["link_mvs"] or (t is not None and t.data_ptr() == i["link_mvs"].data_ptr()) for t in seen["links"]) for i in items)
    assert all(any(t is not None and t.data_ptr() == i["link_mvs"].data_ptr() for t in seen["stabilize"]) for i in items)
    assert all(torch.equal(a["link_raw_mvs"], b["link_mvs"]) for a, b in zip(items, off[0]))             # the raw tables are the unguided run's tables
    assert not any(torch.equal(i["link_mvs"], i["link_raw_mvs"]) for i in items)                          # guidance changed rows in both windows
    assert np.array_equal(mosaic[4], off[2][4]) and (mosaic[4][:, 12] == 0).sum() >= 2                   # the poses and their statuses, unconditionally
    # guide_report(): one row per frame, the reference's counts of the pair that ends in it (zeros for frame 0, which has no pair)
    want = np.zeros((2 * DELTA, 8), np.int64)
    blocks = (FH // 16) * (FW // 16)
    for j in range(1, 2 * DELTA):
        item, p = items[j // DELTA], j % DELTA
        raw = item["link_raw_mvs"][p:p + 1]
        stats = None if "link_stats" not in item else item["link_stats"][p:p + 1]
        model = ops.global_motion(raw, (FH, FW), (FH, FW), 4, 1.0, 12, pair_stats=stats)
        table, counts = gref.guide_vectors(host(raw), host(model), FH, FW, 1, ONE)
        want[j] = counts[0]
        assert np.array_equal(host(item["link_mvs"][p]), table[0]) and host(model)[0, 12] == 0
    assert report.dtype == np.int64 and np.array_equal(report, want) and (want[1:, 0] == blocks).all() and (want[1:, 2] >= 500).all()   # the lake is filled
    assert np.array_equal(report, np.concatenate([host(i["link_guide_counts"]) for i in items]))
    lines = files["guide.csv"].decode().split("\n")
    assert lines[0] == "frame," + ",".join(ops.GUIDE_COUNTS) and lines[2] == "1," + ",".join(str(v) for v in want[1]) and len(lines) == 2 * DELTA + 2
    pred = FlowPredictor(fm, **EVERYTHING)
    with pytest.raises(ValueError, match=r"link_guide_counts must be int64 \[5, 8\]"):
        pred.predict_window(items[0]["frame_prev"], items[0]["frame_next"], items[0]["mvs_left"], items[0]["mvs_right"], to_host=False, link_mvs=items[0]["link_mvs"],
                            link_frame_size=items[0]["link_frame_size"], link_guide_counts=items[0]["link_guide_counts"][:3])
    assert pred.guide_report().shape == (0, 8)


def test_the_mosaic_report_is_the_same_with_guidance_on_and_off(lake_clip, tmp_path):
    """Where the masks do not depend on the grids (no_warp: the key frames' blend) the whole of mosaic_report() -- classes, confidence,
    votes seen, totals, poses -- is identical with guidance on and off, although the link tables differ: the fit is on the raw tables.
    (In warp mode guided grids may change the masks, and with them the votes; there the poses are identical, see the test above.)"""
    fm = FlowModel(network(), feature_based=False, no_warp=True).eval()
    kw = dict(classes=5, out_size=SIZE, crop=None, compute_metrics=True, cache_keyframes=False, regions=True, track=True, compensate=True, mosaic=(96, 120),
              mosaic_min_inliers=6, mosaic_exclude=())
    windows = dict(WINDOWS, no_warp=True)
    off = run_windows(RawVideoWindows(lake_clip, FH, FW, "rgb24", **windows), fm, str(tmp_path / "off"), **kw)
    on = run_windows(RawVideoWindows(lake_clip, FH, FW, "rgb24", guide=True, guide_outlier=1.0, **windows), fm, str(tmp_path / "on"), **kw)
    assert not any(torch.equal(i["link_mvs"], i["link_raw_mvs"]) for i in on[0]) and np.array_equal(on[1], off[1])
    assert len(on[2]) == 5 and all(np.array_equal(a, b) for a, b in zip(on[2], off[2])) and on[5]["mosaic.csv"] == off[5]["mosaic.csv"]
    assert (on[2][4][:, 12] == 0).sum() >= 2 and on[2][2].max() >= 2                                       # frames were registered and voted
    assert on[4].shape == (2 * DELTA, 8) and off[4].shape == (0, 8)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_raises_before_a_launch_and_names_the_value():
    tables, model = table_case(64, 96, 3)
    t, m = dev(tables), dev(model)
    frames = torch.zeros((3, 64, 96, 3), dtype=torch.uint8, device=DEV)
    cost = torch.zeros((3, 24), dtype=torch.int32, device=DEV)
    before = t.clone()
    for changed, word in ((dict(frame_size=(15, 96)), r"\(15, 96\)"), (dict(frame_size=(64, 16400)), "16400"), (dict(outlier=64.5), "64.5"), (dict(outlier=-1), "-1"),
                          (dict(penalty=-1), "-1"), (dict(penalty=256), "256"), (dict(guide_bias=65536), "65536"), (dict(cur=frames), "cur"),
                          (dict(ref=frames, cost=cost), r"\['ref', 'cost'\]"), (dict(cur=frames[..., :2], ref=frames[..., :2], cost=cost), r"\(3, 64, 96, 2\)"),
                          (dict(model=m[:2]), r"\(2, 16\)"), (dict(tables=torch.zeros((65, 24, 7), dtype=torch.int32, device=DEV)), "65")):
        with pytest.raises(ValueError, match=word):
            ops.guide_vectors(**{**dict(tables=t, model=m, frame_size=(64, 96), out=t), **changed})
    lib = _lib.load()
    counts = torch.full((3, 8), -5, dtype=torch.int64, device=DEV)
    good = dict(mv=ptr(t), model=ptr(m), n=3, FH=64, FW=96, fill_void=1, outlier_q20=0, cur=ptr(frames), ref=ptr(frames), channels=3, cost=ptr(cost), penalty=0,
                guide_bias=0, out=ptr(t), counts=ptr(counts), stream=stream_ptr())
    for changed, word in ((dict(mv=None), b"null"), (dict(counts=None), b"null"), (dict(n=65), b"got 65"), (dict(FH=8), b"8x96"), (dict(outlier_q20=-2), b"got -2"),
                          (dict(penalty=300), b"got 300"), (dict(guide_bias=-4), b"got -4"), (dict(ref=None), b"together"), (dict(channels=2), b"got 2"),
                          (dict(out=ptr(t).value + 2), b"aligned to 4"), (dict(counts=ptr(counts).value + 4), b"aligned to 8")):
        assert lib.fs_guide_vectors(*{**good, **changed}.values()) != 0 and word in lib.fs_last_error()
    torch.cuda.synchronize()
    assert torch.equal(t, before) and (counts == -5).all()                 # nothing was launched: not even the clearing of counts


def test_predict_video_guides_and_writes_the_report(clip, tmp_path):  # noqa: F811
    """The command-line tool is what this test is about: one child process, --guide with its options and --mosaic (so the windows carry
    raw and guided tables) on the synthetic clip; the CSV holds one row of counts per guided frame pair."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    png, csv = str(tmp_path / "m.png"), str(tmp_path / "g.csv")
    cmd = [sys.executable, os.path.join(root, "tools", "predict_video.py"), "--raw", clip, "--raw-size", str(FH), str(FW), "--pix-fmt", "rgb24", "--search", "8",
           "--synthetic-weights", "--no-cropping", "--size", "65", "65", "--no-metrics", "--intra-bias", "0", "--guide", "--guide-outlier", "1.0", "--guide-bias", "0",
           "--guide-report", csv, "--mosaic", png, "--mosaic-size", "96", "120", "--mosaic-exclude"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--guide:" in r.stdout and "frame pairs" in r.stdout and "--mosaic:" in r.stdout
    lines = open(csv).read().split("\n")
    assert lines[0] == "frame," + ",".join(ops.GUIDE_COUNTS) and lines[-1] == "" and len(lines) > 3
    rows = np.array([[int(v) for v in line.split(",")] for line in lines[1:-1]])
    assert (np.diff(rows[:, 0]) > 0).all() and (rows[:, 1] == (FH // 16) * (FW // 16)).all()
    assert (rows[:, 5] + rows[:, 6] + rows[:, 7] == rows[:, 4]).all() and (rows[:, 3] <= rows[:, 2]).all()   # replaced + dropped + kept = outliers; filled <= void in
