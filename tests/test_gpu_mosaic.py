"""The flood-extent mosaic on the GPU (ops.global_motion, ops.pose_chain, ops.mosaic_accumulate, ops.mosaic_resolve)
against the numpy definition of tests/mosaic_ref.py, bit for bit, through the C ABI: the fit on block grids from 4 x 6 to 135 x 240 with
outliers, void rows, long vectors, cuts and exclusion masks; the chain fresh, carried, bridged, cut, clipped and out of bounds; the
gather under shifts, a rotation and zooms onto canvases off the tile size, with a poisoned tile that no frame touches; the resolve; a
synthetic flight end to end through ops.block_match; FlowPredictor(mosaic=...) over two windows; and one HIP-graph capture."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mosaic_ref as mref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import PALETTE, FlowPredictor
from test_gpu_regions import DELTA, FH, FRAMES, FW, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = mref.ONE
IDENT = mref.IDENTITY


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ global_motion
@functools.lru_cache(maxsize=None)
def pair_set(hb, wb):
    """Seven pairs of one block grid with different outcomes: a known affine (0.5 degrees, zoom 1.005, shift (7, -3)) clean and with 25 and
    40 % outlier rows, all rows void, every second vector beyond +-32, a cut, and the clean table again under an exclusion mask that
    removes most rows.  -> (tables [7, blocks, 7], pair_stats [7, 4], mask [7, H, W], exclude_set, mask size)."""
    clean = mref.grid_table(hb, wb, mref.affine_vectors(hb, wb))
    far = clean.copy()
    far[::2, 4] -= 45
    tables = np.stack([clean, mref.with_outliers(clean, 0.25, 1), mref.with_outliers(clean, 0.40, 2), np.tile(np.array(mref.VOID_ROW, np.int32), (hb * wb, 1)),
                       far, clean, clean])
    stats = np.zeros((7, 4), np.int32)
    stats[:, 0] = hb * wb
    stats[5, 2] = 1
    h, w = (hb * 16, wb * 16) if hb <= 8 else (hb * 2 + 1, wb * 2 + 1)     # a mask of the frame's size, or of an eighth of it and odd
    mask = np.zeros((7, h, w), np.uint8)
    mask[:, :, w // 3:] = 40                                                # an id >= 32 is never excluded
    mask[6] = 1
    mask[6, : h // 3, : w // 4] = 2                                         # pair 6: a twelfth of the blocks stay
    for a in (tables, stats, mask):
        a.setflags(write=False)
    return tables, stats, mask, 0b10, (h, w)


@pytest.mark.parametrize("hb,wb", [(4, 6), (8, 12), (67, 120), (135, 240)])
def test_global_motion_equals_the_definition(hb, wb):
    """135 x 240 is a 2160 x 3840 frame: 32400 rows, more than a workgroup's threads eight times over and no multiple of them."""
    tables, stats, mask, exclude, mask_size = pair_set(hb, wb)
    size = (hb * 16, wb * 16)
    for rounds, min_inliers in ((0, 6), (1, 6), (4, 12)):
        want = mref.global_motion(tables, size, mask_size, rounds, ONE, min_inliers, mask, exclude, stats)
        got = host(ops.global_motion(dev(tables), size, mask_size, rounds, 1.0, min_inliers, dev(mask), (1,), dev(stats)))
        assert np.array_equal(got, want), (rounds, got[:, 12:].tolist(), want[:, 12:].tolist())
        if hb >= 8 and rounds:
            assert want[:6, 12].tolist() == [0, 0, 0, 2, 0, 1]                  # not vacuous: fitted, too few, cut
            assert (want[:3, 0] != ONE).all() and (want[:3, 1] != 0).all()  # a real affine, not a translation
            assert 0 < want[6, 13] <= hb * wb // 10 and want[4, 13] < hb * wb * 6 // 10   # the mask and the long vectors removed rows
    one = host(ops.global_motion(dev(tables[1:2]), size, mask_size, 4, 1.0, 6))    # n = 1, no mask, no stats
    assert np.array_equal(one, mref.global_motion(tables[1:2], size, mask_size, 4, ONE, 6))
    five = host(ops.global_motion(dev(tables[:5]), size, mask_size, 4, 0.25, 6, pair_stats=dev(stats[:5])))
    assert np.array_equal(five, mref.global_motion(tables[:5], size, mask_size, 4, ONE // 4, 6, pair_stats=stats[:5]))


def test_global_motion_on_a_degenerate_grid_and_an_implausible_motion():
    one_row = mref.grid_table(1, 12, mref.affine_vectors(1, 12))                # q is constant: the normal equations are singular
    zoom = mref.grid_table(8, 12, lambda cx, cy: (np.rint(0.3 * (cx - 96)).astype(np.int64), np.rint(0.3 * (cy - 64)).astype(np.int64)))
    for table, size, tol in ((one_row, (16, 192), 1.0), (zoom, (128, 192), 8.0)):
        for rounds in (0, 2):
            want = mref.global_motion(table[None], size, size, rounds, mref.tol_q20(tol), 6)
            got = host(ops.global_motion(dev(table[None]), size, size, rounds, tol, 6))
            assert np.array_equal(got, want)
            assert want[0, 12] == (3 if rounds else 0)


# ------------------------------------------------------------------------------------------------ pose_chain
def shift(dx, dy, status=0):
    return [ONE, 0, dx * ONE, 0, ONE, dy * ONE, ONE, 0, -dx * ONE, 0, ONE, -dy * ONE, status, 20, 18, 4]


FAILED = IDENT + IDENT + [2, 3, 3, 0]


def chain(model, state, origin=(10, 20), max_bridge=2, canvas=(100, 100)):
    st = dev(state)
    poses = ops.pose_chain(dev(np.array(model, np.int64)), st, (40, 60), canvas, origin, max_bridge)
    return host(poses), host(st)


def test_pose_chain_equals_the_definition():
    c, s = 1.01 * np.cos(np.radians(1.5)), 1.01 * np.sin(np.radians(1.5))
    turn = mref.affine_pose(c, -s, s, c, 2.5, -1.25)
    turn = turn[0] + turn[1] + [0, 50, 40, 4]
    wild = [1 << 40] * 12 + [0, 1, 1, 1]
    runs = [[shift(99, 99), shift(3, -2), FAILED, FAILED, shift(1, 1), FAILED, FAILED, FAILED, shift(5, 5)],   # a bridge run of two, then one of three
            [shift(0, 0), turn, turn, FAILED, turn, wild, turn, IDENT + IDENT + [9, 0, 0, 0], turn],              # rounding, bad rows bridged
            [shift(0, 0), shift(1, 1), shift(0, 0, 1), shift(1, 1)],                                              # a cut
            [shift(0, 0)] + [shift(4000, 0)] * 5,                                                                 # the translation bound
            [shift(0, 0), FAILED]]                                                                                 # a bridge before any good pair
    fresh = np.zeros(32, np.int64)
    for model in runs:
        for max_bridge in (0, 2):
            want_poses, want_state = mref.pose_chain(np.array(model, np.int64), fresh, (40, 60), (100, 100), (10, 20), max_bridge)
            poses, state = chain(model, fresh, max_bridge=max_bridge)
            assert np.array_equal(poses, want_poses) and np.array_equal(state, want_state), max_bridge
    poses, _ = chain(runs[0], fresh)
    assert poses[:, 12].tolist() == [0, 0, 1, 1, 0, 1, 1, 2, 2]
    poses, _ = chain(runs[3], fresh, origin=(0, 0))
    assert poses[:, 12].tolist() == [0, 0, 0, 0, 0, 2]
    # two calls of 3 and 2 frames are one call of 5; the carried state goes on where it was
    whole, end = chain(runs[1][:5], fresh)
    first, mid = chain(runs[1][:3], fresh)
    second, last = chain(runs[1][3:5], mid)
    assert np.array_equal(np.concatenate([first, second]), whole) and np.array_equal(last, end) and mid[25] == 3
    # clipping at each canvas edge
    for dx, dy, clipped in ((0, 0, 0), (-21, 0, 1), (21, 0, 1), (20, 0, 0), (0, -11, 1), (0, 51, 1), (0, 50, 0)):
        poses, _ = chain([shift(0, 0), shift(dx, dy)], fresh)
        assert poses[1, 13] == clipped and np.array_equal(poses, mref.pose_chain(np.array([shift(0, 0), shift(dx, dy)], np.int64), fresh, (40, 60), (100, 100),
                                                                                 (10, 20))[0])


# ------------------------------------------------------------------------------------------------ mosaic_accumulate
def guarded_votes(start):
    """`start` uint16 [K, CH, CW] inside a larger buffer of a guard value, at an odd element offset."""
    whole = np.full(start.size + 64, 0x5A5A, np.uint16)
    whole[3:3 + start.size] = start.reshape(-1)
    buf = dev(whole)
    return buf, buf[3:3 + start.size].view(start.shape)


@functools.lru_cache(maxsize=None)
def gather_case():
    """Five 37 x 53 masks with ids up to 6, and poses: identity, a negative translation partly off the canvas, a 30 degree rotation, a lost
    frame between live ones, a zoom of 2; with the zoom 0.5 in a second set."""
    rng = np.random.RandomState(23)
    mask = rng.randint(0, 7, size=(5, 37, 53)).astype(np.uint8)
    c, s = np.cos(np.radians(30)), np.sin(np.radians(30))
    pairs = [mref.affine_pose(1, 0, 0, 1, 0, 0), mref.affine_pose(1, 0, 0, 1, -30.5, -20.25), mref.affine_pose(c, -s, s, c, 40, 10),
             mref.affine_pose(1, 0, 0, 1, 5, 5), mref.affine_pose(2, 0, 0, 2, -10, 30)]
    poses = mref.pose_rows(pairs, status=[0, 1, 0, 2, 0])
    small = mref.pose_rows([mref.affine_pose(0.5, 0, 0, 0.5, 3, 70)] + pairs[1:], status=[0, 2, 2, 2, 2])
    for a in (mask, poses, small):
        a.setflags(write=False)
    return mask, poses, small


@pytest.mark.parametrize("canvas,origin", [((128, 160), (20, 25)), ((50, 70), (-4, 9))])
@pytest.mark.parametrize("k", [1, 5, 32])
def test_accumulate_equals_the_definition(canvas, origin, k):
    """Both canvases are off the 64 x 16 tile; K = 1 drops most ids, K = 32 takes them all.  Twice in a row on a canvas that starts near
    saturation in places; nothing outside the canvas planes is written."""
    mask, poses, small = gather_case()
    start = np.zeros((k,) + canvas, np.uint16)
    start[:, ::7, ::5] = 65534
    want = start.copy()
    buf, votes = guarded_votes(start)
    for p in (poses, small, poses):
        mref.mosaic_accumulate(mask, p, want, origin)
        ops.mosaic_accumulate(dev(mask), dev(p), votes, origin)
        assert np.array_equal(host(votes), want)
    assert (want == 65535).any() and want.max() == 65535 and (want[:, 1::7, 1::5] > 0).any()
    assert (host(buf)[:3] == 0x5A5A).all() and (host(buf)[3 + start.size:] == 0x5A5A).all()


def test_a_tile_that_no_frame_touches_is_neither_read_nor_written():
    """A 37 x 53 frame at the origin of a 128 x 160 canvas touches the tiles of columns 0..63 and rows 0..47 (one pixel of slack): every
    other tile keeps the poison written into it, which a read-modify-write of its votes would have replaced with the same value -- so the
    poison is 65535 with a frame whose every pixel votes, and the count of changed cells is the frame's."""
    mask = np.zeros((1, 37, 53), np.uint8)
    want = np.full((2, 128, 160), 65535, np.uint16)
    want[:, :48, :64] = 0
    votes = dev(want)
    ops.mosaic_accumulate(dev(mask), dev(mref.pose_rows([(IDENT, IDENT)])), votes, (0, 0))
    want[0, :37, :53] = 1
    assert np.array_equal(host(votes), want)
    # the same through the definition, and a canvas that no live frame reaches at all stays as it was, poison included
    far = dev(np.full((2, 50, 70), 0x1234, np.uint16))
    ops.mosaic_accumulate(dev(mask), dev(mref.pose_rows([mref.affine_pose(1, 0, 0, 1, 500, 500)])), far, (0, 0))
    assert (host(far) == 0x1234).all()
    lost = mref.pose_rows([(IDENT, IDENT)], status=[2])
    ops.mosaic_accumulate(dev(mask), dev(lost), far, (0, 0))
    assert (host(far) == 0x1234).all()
    lost[0, 12] = 77                                                        # a status that is none of the three: tested before use
    ops.mosaic_accumulate(dev(mask), dev(lost), far, (0, 0))
    assert (host(far) == 0x1234).all()


# ------------------------------------------------------------------------------------------------ mosaic_resolve
@pytest.mark.parametrize("k,canvas", [(1, (5, 7)), (5, (50, 70)), (32, (33, 129))])
def test_resolve_equals_the_definition(k, canvas):
    rng = np.random.RandomState(k)
    votes = rng.randint(0, 4, size=(k,) + canvas).astype(np.uint16)            # small counts: ties everywhere
    votes[:, ::3, ::2] = 0                                                   # unseen pixels
    votes[:, 1, 1] = 65535                                                   # the largest total
    votes[k - 1, 2, :] = 60000
    want = mref.mosaic_resolve(votes)
    got = ops.mosaic_resolve(dev(votes))
    for g, w_ in zip(got, want):
        assert np.array_equal(host(g).astype(np.int64), w_.astype(np.int64))
    assert (want[0] == 255).any() and want[3][:, 0].sum() == (want[2] > 0).sum()
    if k > 1:
        v = votes.astype(np.int64)
        assert ((v == v.max(0)).sum(0) > 1)[want[2] > 0].any()             # not vacuous: tied winners exist


# ------------------------------------------------------------------------------------------------ end to end
def test_a_synthetic_flight_through_the_block_matcher():
    """The CPU test's scene with the tables from ops.block_match: equal to the reference run on the same tables, and to the world."""
    frames, masks, offsets, labels = mref.scene()
    d = dev(frames)
    tables = torch.stack([ops.block_match(d[i], d[max(i - 1, 0)], search=16) for i in range(6)])
    model = ops.global_motion(tables, mref.SCENE_VIEW, mref.SCENE_VIEW, 4, 1.0, 6)
    state = torch.zeros((32,), dtype=torch.int64, device=DEV)
    poses = ops.pose_chain(model, state, mref.SCENE_VIEW, mref.SCENE_CANVAS, mref.SCENE_ORIGIN)
    votes = ops.mosaic_accumulate(dev(masks), poses, dev(np.zeros((4,) + mref.SCENE_CANVAS, np.uint16)), mref.SCENE_ORIGIN)
    cls, conf, seen, totals = (host(t) for t in ops.mosaic_resolve(votes))
    w_model, w_poses, w_state, w_votes, (w_cls, w_conf, w_seen, w_totals) = mref.run_scene(list(host(tables)), masks)
    assert np.array_equal(host(model), w_model) and np.array_equal(host(poses), w_poses) and np.array_equal(host(state), w_state)
    assert np.array_equal(host(votes), w_votes) and np.array_equal(cls, w_cls) and np.array_equal(conf, w_conf) and np.array_equal(seen, w_seen)
    assert np.array_equal(totals, w_totals)
    want_seen, want_cls = mref.scene_expectation()
    assert np.array_equal(seen, want_seen) and int((seen > 0).sum()) == 28434 and int((cls != want_cls).sum()) == 0
    assert [row[:6] for row in host(model)[1:].tolist()] == [[ONE, 0, dx * ONE, 0, ONE, dy * ONE] for dy, dx in mref.SCENE_STEPS]


def test_predictor_keeps_the_mosaic_and_changes_nothing_else(clip):  # noqa: F811
    """Two windows of the synthetic network: the masks are bit-identical to mosaic=None, mosaic_report() is the reference applied to the
    masks handed out and the tables the dataset handed out; clear_report() drops canvas and state, reset() keeps them."""
    size = (65, 65)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8, link_vectors=True)
    items = [ds[0], ds[1]]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=True, cache_keyframes=False)

    def run(pred, item):
        return pred.predict_window(item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"], to_host=False, link_mvs=item["link_mvs"],
                                   link_frame_size=item["link_frame_size"], link_stats=item.get("link_stats"))

    off = FlowPredictor(fm, mosaic=None, **kw)
    plain = np.concatenate([host(run(off, i)) for i in items])
    on = FlowPredictor(fm, mosaic=(96, 120), mosaic_min_inliers=6, mosaic_exclude=(), **kw)
    got = np.concatenate([host(run(on, i)) for i in items])
    assert np.array_equal(got, plain) and torch.equal(on.hist, off.hist)
    tables = np.concatenate([host(i["link_mvs"]) for i in items])
    stats = None if items[0].get("link_stats") is None else np.concatenate([host(i["link_stats"]) for i in items])
    origin = ((96 - 65) // 2, (120 - 65) // 2)
    model = mref.global_motion(tables, (FH, FW), size, 4, ONE, 6, plain, 0, stats)
    poses, state = mref.pose_chain(model, np.zeros(32, np.int64), size, (96, 120), origin)
    votes = mref.mosaic_accumulate(plain, poses, np.zeros((5, 96, 120), np.uint16), origin)
    want = mref.mosaic_resolve(votes)
    cls, conf, seen, totals, rows = on.mosaic_report()
    assert np.array_equal(rows, poses) and np.array_equal(host(on.mosaic_builder.state), state)
    assert np.array_equal(cls, want[0]) and np.array_equal(conf, want[1]) and np.array_equal(seen, want[2].astype(np.int32)) and np.array_equal(totals, want[3])
    assert (poses[:, 12] == 0).sum() >= 2 and seen.max() >= 2 and totals[:, 1].sum() > 0     # not vacuous: frames were registered and voted
    on.reset()                                                                 # a new video: canvas and state stay
    assert on.mosaic_report()[4].shape == (2 * DELTA, 16) and on.mosaic_builder.votes is not None
    on.clear_report()
    assert on.mosaic_builder.votes is None and on.mosaic_builder.state is None and on.mosaic_report()[4].shape == (0, 16)
    run(on, items[1])                                                          # the next frame anchors a new mosaic
    rows = on.mosaic_report()[4]
    assert rows.shape == (DELTA, 16) and rows[0].tolist() == IDENT + IDENT + [0, 0, 0, 0]
    with pytest.raises(ValueError, match="needs link_mvs and link_frame_size"):
        on.predict_window(items[0]["frame_prev"], items[0]["frame_next"], items[0]["mvs_left"], items[0]["mvs_right"], to_host=False)


def test_a_captured_graph_replayed_on_new_inputs_gives_each_replays_result():
    """The three per-window ops in one graph on a single stream; state and votes carry from replay to replay as they do from call to call."""
    tables, stats, mask, exclude, mask_size = pair_set(8, 12)
    size = (128, 192)
    canvas, origin = (160, 230), (12, 17)
    lib = _lib.load()
    n = 3
    t, st, m = dev(tables[:n]), dev(stats[:n]), dev(mask[:n])
    model = torch.full((n, 16), -12345, dtype=torch.int64, device=DEV)
    poses = torch.full((n, 16), -12345, dtype=torch.int64, device=DEV)
    state = torch.zeros((32,), dtype=torch.int64, device=DEV)
    votes = dev(np.zeros((3,) + canvas, np.uint16))

    def launch():
        s = stream_ptr()
        check(lib.fs_global_motion(ptr(t), ptr(st), ptr(m), exclude, n, size[0], size[1], mask_size[0], mask_size[1], 4, ONE, 6, ptr(model), s))
        check(lib.fs_pose_chain(ptr(model), ptr(state), ptr(poses), n, mask_size[0], mask_size[1], canvas[0], canvas[1], origin[1], origin[0], 2, s))
        check(lib.fs_mosaic_accumulate(ptr(m), ptr(poses), n, mask_size[0], mask_size[1], 3, canvas[0], canvas[1], origin[1], origin[0], ptr(votes), s))

    launch()                                                                # the kernels are loaded before the capture
    torch.cuda.synchronize()
    state.zero_()
    votes.view(torch.int16).zero_()                                        # the same bits
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    state.zero_()
    votes.view(torch.int16).zero_()                                        # the same bits
    want_state, want_votes = np.zeros(32, np.int64), np.zeros((3,) + canvas, np.uint16)
    for pick in ((0, 1, 2), (2, 6, 1), (4, 0, 3)):
        idx = list(pick)
        t.copy_(dev(tables[idx]))
        st.copy_(dev(stats[idx]))
        m.copy_(dev(mask[idx]))
        graph.replay()
        torch.cuda.synchronize()
        want_model = mref.global_motion(tables[idx], size, mask_size, 4, ONE, 6, mask[idx], exclude, stats[idx])
        want_poses, want_state = mref.pose_chain(want_model, want_state, mask_size, canvas, origin)
        mref.mosaic_accumulate(mask[idx], want_poses, want_votes, origin)
        assert np.array_equal(host(model), want_model) and np.array_equal(host(poses), want_poses)
        assert np.array_equal(host(state), want_state) and np.array_equal(host(votes), want_votes)
    assert want_votes.any()


def test_predict_video_writes_the_mosaic_and_its_report(clip, tmp_path):  # noqa: F811
    """The command-line tool is what this test is about: one child process, --mosaic with its options on the synthetic clip; the PNG is
    the palette's colours of the classes the report counts, black where no frame looked, and the CSV holds one row per frame."""
    from PIL import Image                                                   # the tool's own dependency for --mosaic and --out

    frames = (FRAMES - 1) // DELTA * DELTA
    png, csv = str(tmp_path / "m.png"), str(tmp_path / "m.csv")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "predict_video.py"), "--raw", clip, "--raw-size", str(FH), str(FW), "--pix-fmt", "rgb24", "--search", "8",
           "--synthetic-weights", "--no-cropping", "--size", "65", "65", "--no-metrics", "--mosaic", png, "--mosaic-size", "96", "120", "--mosaic-exclude",
           "--mosaic-report", csv]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--mosaic:" in r.stdout and "canvas pixels seen" in r.stdout
    rgb = np.asarray(Image.open(png))
    assert rgb.shape == (96, 120, 3)
    lines = open(csv).read().split("\n")
    assert lines[0] == "frame,status,clipped,inliers,usable,m00,m01,m02,m10,m11,m12" and lines[frames + 1] == "" and lines[frames + 2] == "class,pixels,share,votes"
    rows = [line.split(",") for line in lines[1:frames + 1]]
    assert [int(row[0]) for row in rows] == list(range(frames)) and rows[0][1:5] == ["ok", "0", "0", "0"] and rows[0][5:] == ["1.000000", "0.000000", "0.000000", "0.000000", "1.000000", "0.000000"]
    assert all(row[1] in ("ok", "bridged", "lost") for row in rows)
    totals = np.array([[int(v) for v in (line.split(",")[1], line.split(",")[3])] for line in lines[frames + 3:frames + 8]])
    per_class = [int((rgb == PALETTE[k]).all(-1).sum()) for k in range(5)]
    assert 65 * 65 <= totals[:, 0].sum() <= 96 * 120 and per_class[1:] == totals[1:, 0].tolist()       # class 0 and "never seen" are both black
    assert per_class[0] == 96 * 120 - totals[1:, 0].sum() and sum(per_class) == 96 * 120
