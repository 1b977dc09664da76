"""The region overlay on the GPU (csrc/overlay_ops.hip through the sixth hook table, ops.compose_regions, FlowPredictor.window_regions and
compose_window(regions=)).

Every comparison in this file is an EQUALITY against the numpy definition tests/overlay_ref.py (or against ops.compose_frame where the
header says the two agree).  The index planes, tables and counts come from ops.mask_regions / ops.region_table, which their own tests
pin; the expected pictures are computed once per case.  Every GPU step runs once."""
import numpy as np
import pytest
import torch

import egress_ref
import outlines_ref as oref
import overlay_ref as vref
import regions_ref as rref
from flood_uav_video_segmentation_amd import ops
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows, raw_frame_bytes
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor, compose_window
from test_gpu_regions import DELTA, FH, FW, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
K = 3                                                                        # classes 0..2; oref.BG is background (index -1, class 0's colour)
PAL = np.array([[20, 40, 60, 0], [30, 95, 170, 128], [212, 98, 1, 255]], dtype=np.uint8)
LINE = np.array([[255, 255, 255, 255], [0, 0, 0, 0], [250, 20, 200, 127]], dtype=np.uint8)   # class 1 draws no outline
FILL = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240]], dtype=np.uint8)
HALO, INK = (10, 20, 30, 160), (250, 251, 252)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def first_difference(got, want):
    bad = got != want
    i = int(np.argmax(bad))
    return f"{int(bad.sum())} of {got.size} bytes differ, first at byte {i}: got {int(got[i])}, want {int(want[i])}"


def blobs(h, w, seed, cell=3):
    """A mask of connected bodies of classes 0..2 over background: a coarse random field, repeated."""
    if cell == 3:
        return oref.random_mask(1, h, w, seed, smooth=True)[0]
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 4, (-(-h // cell), -(-w // cell))).astype(np.uint8)
    coarse[coarse == 3] = oref.BG
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:h, :w])


def regions_of(mask, cap):
    """index [h,w], table [cap,10], counts [2] on the device from the region ops."""
    m = dev(mask)[None]
    table, counts, index = ops.region_table(m, ops.mask_regions(m, K, 8), K, None, 128, cap)
    return index[0].contiguous(), table[0].contiguous(), counts[0].contiguous()


def tracks_of(cap, seed):
    """int64 [cap,4]: ids small, above 10^7, and -1 (no id), as region_tracks lays a frame out."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 40, cap)
    ids[2::5] = rng.integers(10 ** 7, 2 ** 40, len(ids[2::5]))
    ids[3::7] = -1
    t = np.full((cap, 4), -1, np.int64)
    t[:, 0] = ids
    return t


def source_of(kind, hw, seed):
    """(ops arguments, the reference's background image) for a background kind: none, rgb (resized), nv12 (at the frame's size)."""
    h, w = hw
    rng = np.random.default_rng(seed)
    if kind == "none":
        return {}, None
    if kind == "rgb":
        img = rng.integers(0, 256, (h + 9, w + 13, 3)).astype(np.uint8)
        return dict(background=dev(img), fmt="rgb24"), egress_ref.background(img, size=hw)
    y = rng.integers(0, 256, (h, w)).astype(np.uint8)
    u, v = (rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2)).astype(np.uint8) for _ in range(2))
    return (dict(background=dev(y), chroma=dev(np.stack([u, v], -1)), fmt="nv12", matrix="bt709", full_range=False),
            egress_ref.background(y, (u, v), "i420", "bt709", False, hw))


def nv12_bytes(want, h, w):
    """egress_ref packs planar chroma for "i420"; NV12 interleaves the same samples."""
    n = h * w
    c = (len(want) - n) // 2
    return np.concatenate([want[:n], np.stack([want[n:n + c], want[n + c:]], axis=-1).reshape(-1)])


def expected(mask, index, out_fmt, out_matrix, out_full_range, **layers):
    want = vref.compose(mask, PAL, index, "rgb24" if out_fmt == "rgb24" else "i420", out_matrix, out_full_range, **layers)
    return nv12_bytes(want, *mask.shape) if out_fmt == "nv12" else want


# an orthogonal array over (out_fmt, background, T, s), three levels each: every pair of levels of two of them occurs; each row runs with
# (P, tracks) and with its complement, the four (P, tracks) combinations rotating, so every level also meets both values of those two
L9 = [(0, 0, 0, 0), (0, 1, 1, 1), (0, 2, 2, 2), (1, 0, 1, 2), (1, 1, 2, 0), (1, 2, 0, 1), (2, 0, 2, 1), (2, 1, 0, 2), (2, 2, 1, 0)]
OUTS = [("rgb24", "bt601", False), ("nv12", "bt709", False), ("i420", "bt601", True)]
COMBOS = [(OUTS[a], ("none", "rgb", "nv12")[b], (1, 2, 4)[c], (0, 1, 3)[d], 7 * ((i + flip) % 2), bool(((i // 2) + flip) % 2))
          for i, (a, b, c, d) in enumerate(L9) for flip in (0, 1)]


@pytest.mark.parametrize("hw", [(33, 47), (40, 64), (70, 200)])
def test_layer_combinations_equal_the_definition(hw):
    """(33, 47): odd, the byte route; (40, 64): the wide route, half a tile; (70, 200): more than one tile in both directions."""
    h, w = hw
    assert {(c[0][0], c[1]) for c in COMBOS} == {(o[0], b) for o in OUTS for b in ("none", "rgb", "nv12")}
    assert {(c[2], c[3]) for c in COMBOS} == {(t, s) for t in (1, 2, 4) for s in (0, 1, 3)} and {(c[4], c[5]) for c in COMBOS} == {(0, False), (0, True), (7, False), (7, True)}
    mask = blobs(h, w, seed=h + w)
    cap = {33: 48, 40: 400, 70: 2048}[h]                                      # 48: below the region count, regions without a row inside the picture
    index, table, counts = regions_of(mask, cap)
    tr = tracks_of(cap, seed=3)
    idx, tab, cnt = index.cpu().numpy(), table.cpu().numpy(), counts.cpu().numpy()
    assert int(cnt[1]) >= 20 and (idx < 0).any() and (idx[h // 2:, w // 2:] >= 0).any()
    m, dtr = dev(mask), dev(tr)
    sources = {kind: source_of(kind, hw, seed=7) for kind in ("none", "rgb", "nv12")}
    seen_labels = 0
    for (ofmt, omx, ofr), kind, T, s, P, with_tracks in COMBOS:
        kw, bg = sources[kind]
        layers = dict(table=tab, counts=cnt, tracks=tr if with_tracks else None, fill_palette=FILL if P else None, outline=LINE, outline_width=T,
                      label_scale=s, label_min_area=20, halo=HALO, ink=INK)
        want = expected(mask, idx, ofmt, omx, ofr, bg=bg, **layers)
        seen_labels += len(vref.labels(h, w, cap, tab, cnt, tr if with_tracks else None, s, 20))
        out = torch.empty(raw_frame_bytes(h, w, ofmt), dtype=torch.uint8, device="cuda")
        ops.compose_regions(m, PAL, index, table, counts, dtr if with_tracks else None, fill_palette=FILL if P else None, outline=LINE, outline_width=T,
                            label_scale=s, label_min_area=20, halo=HALO, ink=INK, out_fmt=ofmt, out_matrix=omx, out_full_range=ofr, out=out, **kw)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), f"{hw} out {ofmt} bg {kind} T {T} s {s} P {P} tracks {with_tracks}: {first_difference(got, want)}"
        plain = expected(mask, idx, ofmt, omx, ofr, bg=bg, outline_width=0)
        assert not np.array_equal(want, plain)                                # the layers show
    assert seen_labels > 20


def test_a_full_frame_with_every_layer_equals_the_definition():
    h, w = 1072, 1920
    mask = blobs(h, w, seed=5, cell=40)
    cap = 1024
    index, table, counts = regions_of(mask, cap)
    tr = tracks_of(cap, seed=6)
    kw, bg = source_of("nv12", (h, w), seed=8)
    want = expected(mask, index.cpu().numpy(), "nv12", "bt709", False, bg=bg, table=table.cpu().numpy(), counts=counts.cpu().numpy(), tracks=tr,
                    fill_palette=FILL, outline=LINE, outline_width=2, label_scale=2, label_min_area=256, halo=HALO, ink=INK)
    y, uv = ops.compose_regions(dev(mask), PAL, index, table, counts, dev(tr), fill_palette=FILL, outline=LINE, outline_width=2, label_scale=2,
                                label_min_area=256, halo=HALO, ink=INK, out_fmt="nv12", **kw)
    got = torch.cat([y.reshape(-1), uv.reshape(-1)]).cpu().numpy()
    assert 100 < int(counts[1]) <= cap and np.array_equal(got, want), first_difference(got, want)


def test_adversarial_planes():
    """Index values outside 0 .. R - 1 (negative and huge), ids -1 and above 10^7 and 2^32, counts[1] > R, areas below label_min_area,
    centroids far outside the frame."""
    h, w, R = 45, 83, 16
    rng = np.random.default_rng(9)
    coarse = rng.integers(-3, R + 3, (-(-h // 5), -(-w // 5)))
    index = np.repeat(np.repeat(coarse, 5, 0), 5, 1)[:h, :w].astype(np.int32)
    index[::9, ::7] = np.array([-2 ** 31, 2 ** 31 - 1, 65536, R, -1, 10 ** 9, -7], np.int32)[rng.integers(0, 7, index[::9, ::7].shape)]
    mask = rng.integers(0, 5, (h, w)).astype(np.uint8)                       # ids >= K among them
    table = np.zeros((R, 10), np.int64)
    table[:, 1] = [300, 5, 40, 10 ** 12, 39, 41, 300, 300, 300, 300, 300, 300, 300, 300, 300, 300]
    table[:, 6] = table[:, 1] * np.array([5, 40, 60, 10, 20, 80, -500, 10 ** 6, 30, 41, 42, 43, 70, 75, 3, 50])
    table[:, 7] = table[:, 1] * np.array([5, 10, 20, 40, 30, 44, 20, 20, -9, 10 ** 6, 22, 23, 10, 35, 40, 2])
    counts = np.array([99, 10 ** 6], np.int64)                               # more rows "written" than the table has
    tracks = np.full((R, 4), -1, np.int64)
    tracks[:, 0] = [0, 1, 10 ** 7 + 7, 9_999_999, 2 ** 32 + 5, -1, 2 ** 62, 12, 345, 6789, -5, 10 ** 7, 77, 2 ** 31, 2 ** 32 - 1, 3]
    for s, T, ofmt in ((1, 1, "rgb24"), (2, 4, "nv12")):
        layers = dict(fill_palette=FILL, outline=np.full((K, 4), 200, np.uint8), outline_width=T, label_scale=s, label_min_area=40, halo=HALO, ink=INK)
        want = expected(mask, index, ofmt, "bt601", False, table=table, counts=counts, tracks=tracks, **layers)
        assert len(vref.labels(h, w, R, table, counts, tracks, s, 40)) >= 8
        out = torch.empty(raw_frame_bytes(h, w, ofmt), dtype=torch.uint8, device="cuda")
        ops.compose_regions(dev(mask), PAL, dev(index), dev(table), dev(counts), dev(tracks), out_fmt=ofmt, out=out, **layers)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (s, T, ofmt, first_difference(got, want))


@pytest.mark.parametrize("hw", [(33, 47), (40, 64)])
def test_the_two_stated_consequences_against_compose_frame(hw):
    h, w = hw
    mask = blobs(h, w, seed=11)
    index, table, counts = regions_of(mask, 64)
    m = dev(mask)
    for kind in ("none", "rgb", "nv12"):
        kw, _ = source_of(kind, hw, seed=12)
        for ofmt in ("rgb24", "nv12", "i420"):
            want = torch.empty(raw_frame_bytes(h, w, ofmt), dtype=torch.uint8, device="cuda")
            ops.compose_frame(m, PAL, out_fmt=ofmt, out=want, **kw)
            # every layer off: P = 0, T = 0, s = 0 (and an outline width without outline colours)
            for off in (dict(outline_width=0), dict(outline=None, outline_width=3), dict(outline=LINE, outline_width=0, table=table, counts=counts)):
                got = torch.empty_like(want)
                ops.compose_regions(m, PAL, index, out_fmt=ofmt, out=got, **off, **kw)
                assert torch.equal(got, want), (kind, ofmt, off.keys())
            # index all -1 and no live row, whatever the options: through the overlay kernels
            none = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
            got = torch.empty_like(want)
            ops.compose_regions(m, PAL, none, torch.zeros_like(table), torch.zeros_like(counts), dev(tracks_of(64, 1)), fill_palette=FILL, outline=LINE,
                                outline_width=4, label_scale=3, label_min_area=1, out_fmt=ofmt, out=got, **kw)
            assert torch.equal(got, want), (kind, ofmt, "index -1")


@pytest.mark.parametrize("hw", [(40, 64), (33, 47)])
def test_out_slices_at_aligned_and_unaligned_offsets_leave_their_surroundings_alone(hw):
    h, w = hw
    mask = blobs(h, w, seed=13)
    index, table, counts = regions_of(mask, 64)
    tr = tracks_of(64, seed=14)
    layers = dict(fill_palette=FILL, outline=LINE, outline_width=2, label_scale=1, label_min_area=10, halo=HALO, ink=INK)
    kw, bg = source_of("rgb", hw, seed=15)
    m, dtr = dev(mask), dev(tr)
    for ofmt in ("rgb24", "nv12", "i420"):
        want = expected(mask, index.cpu().numpy(), ofmt, "bt709", False, bg=bg, table=table.cpu().numpy(), counts=counts.cpu().numpy(), tracks=tr, **layers)
        n = raw_frame_bytes(h, w, ofmt)
        big = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        for off in (0, 8, 16, 1, 3, 4, 5):
            big.fill_(0xA5)
            ops.compose_regions(m, PAL, index, table, counts, dtr, out_fmt=ofmt, out_matrix="bt709", out_full_range=False, out=big[off:off + n], **layers, **kw)
            got = big.cpu().numpy()
            assert np.array_equal(got[off:off + n], want), (ofmt, off, first_difference(got[off:off + n], want))
            assert (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all(), (ofmt, off)
    with pytest.raises(RuntimeError, match="floodseg.compose_regions:.*out"):
        ops.compose_regions(m, PAL, index, out_fmt="nv12", out=torch.empty(raw_frame_bytes(h, w, "nv12") + 1, dtype=torch.uint8, device="cuda"))


def test_two_runs_are_identical():
    h, w = 70, 200
    mask = blobs(h, w, seed=16)
    index, table, counts = regions_of(mask, 256)
    tr, m = dev(tracks_of(256, seed=17)), dev(mask)
    kw, _ = source_of("nv12", (h, w), seed=18)
    runs = [ops.compose_regions(m, PAL, index, table, counts, tr, fill_palette=FILL, outline=LINE, outline_width=4, label_scale=2, label_min_area=8,
                                out_fmt="i420", **kw) for _ in range(2)]
    (y0, (u0, v0)), (y1, (u1, v1)) = runs
    assert torch.equal(y0, y1) and torch.equal(u0, u1) and torch.equal(v0, v1)


def test_a_captured_graph_replayed_on_new_planes_gives_that_replays_picture():
    h, w, cap = 40, 64, 64
    scenes = []
    for seed in (19, 20):
        mask = blobs(h, w, seed=seed)
        index, table, counts = regions_of(mask, cap)
        scenes.append((mask, index, table, counts, tracks_of(cap, seed)))
    layers = dict(fill_palette=FILL, outline=LINE, outline_width=1, label_scale=1, label_min_area=12, halo=HALO, ink=INK)
    m, index, table, counts, tr = dev(scenes[0][0]), scenes[0][1].clone(), scenes[0][2].clone(), scenes[0][3].clone(), dev(scenes[0][4])
    out = torch.empty(raw_frame_bytes(h, w, "nv12"), dtype=torch.uint8, device="cuda")
    ops.compose_regions(m, PAL, index, table, counts, tr, out_fmt="nv12", out=out, **layers)       # the palettes are on the device from here on
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.compose_regions(m, PAL, index, table, counts, tr, out_fmt="nv12", out=out, **layers)
    for mask, i, t, c, ids in (scenes[1], scenes[0], scenes[1]):
        m.copy_(dev(mask)), index.copy_(i), table.copy_(t), counts.copy_(c), tr.copy_(dev(ids))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = expected(mask, i.cpu().numpy(), "nv12", "bt601", False, table=t.cpu().numpy(), counts=c.cpu().numpy(), tracks=ids, **layers)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), first_difference(got, want)
    assert not np.array_equal(expected(scenes[0][0], scenes[0][1].cpu().numpy(), "nv12", "bt601", False, outline_width=0),
                              expected(scenes[1][0], scenes[1][1].cpu().numpy(), "nv12", "bt601", False, outline_width=0))


def test_refusals_carry_the_package_s_message():
    m = torch.zeros((16, 20), dtype=torch.uint8, device="cuda")
    index = torch.zeros((16, 20), dtype=torch.int32, device="cuda")
    table = torch.zeros((8, 10), dtype=torch.int64, device="cuda")
    counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    tracks = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    f = torch.zeros((16, 20, 3), dtype=torch.uint8, device="cuda")
    for match, call in (
            ("GPU", lambda: ops.compose_regions(m, PAL, index.cpu())),
            ("mask", lambda: ops.compose_regions(m.float(), PAL, index)),
            ("index must be int32", lambda: ops.compose_regions(m, PAL, index.long())),
            ("index must be int32", lambda: ops.compose_regions(m, PAL, index[:8])),
            ("outline_width and label_scale", lambda: ops.compose_regions(m, PAL, index, outline_width=5)),
            ("outline_width and label_scale", lambda: ops.compose_regions(m, PAL, index, table, counts, label_scale=5)),
            ("outline_width and label_scale", lambda: ops.compose_regions(m, PAL, index, table, counts, label_scale=1, label_min_area=0)),
            ("table must be int64", lambda: ops.compose_regions(m, PAL, index, table[:, :9])),
            ("tracks must be int64", lambda: ops.compose_regions(m, PAL, index, table, counts, tracks[:7])),
            ("counts must be int64", lambda: ops.compose_regions(m, PAL, index, table, counts[None])),
            ("labels .* need table= and counts=", lambda: ops.compose_regions(m, PAL, index, label_scale=1)),
            ("fill_palette must be uint8", lambda: ops.compose_regions(m, PAL, index, fill_palette=np.zeros((257, 3), np.uint8))),
            ("fill_palette must be uint8", lambda: ops.compose_regions(m, PAL, index, fill_palette=np.zeros((4, 4), np.uint8))),
            ("outline must be uint8", lambda: ops.compose_regions(m, PAL, index, outline=np.zeros((3, 3), np.uint8))),
            ("one .* row per class", lambda: ops.compose_regions(m, PAL, index, outline=np.zeros((2, 4), np.uint8))),
            ("halo must be 4 values", lambda: ops.compose_regions(m, PAL, index, halo=(0, 0, 0))),
            ("ink must be 3 values", lambda: ops.compose_regions(m, PAL, index, ink=(0, 0, 256))),
            ("chroma", lambda: ops.compose_regions(m, PAL, index, background=m, fmt="nv12")),
            ("alpha", lambda: ops.compose_regions(m, PAL[:, :3], index, background=f)),
            ("palette", lambda: ops.compose_regions(m, np.zeros((5, 2), np.uint8), index))):
        with pytest.raises(RuntimeError, match="floodseg.compose.*" + match):
            call()


# ------------------------------------------------------------------------------------------------ end to end
def test_predictor_window_regions_into_compose_window(clip, monkeypatch):  # noqa: F811
    """One window of five frames with the report buffers cut into chunks of three: window_regions() spans two pieces.  The frames composed
    from it equal the definition fed from region_report() and track_report(); without regions= compose_window is what it was."""
    monkeypatch.setattr(FlowPredictor, "REPORT_CHUNK", 3)
    size = (65, 97)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8)
    item = ds[1]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=(65, 65), compute_metrics=False, cache_keyframes=False, connectivity=4, max_regions=64)
    args = (item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"])
    plain = FlowPredictor(fm, regions=True, track=True, **kw).predict_window(*args, to_host=False)
    pred = FlowPredictor(fm, regions=True, track=True, keep_window_regions=True, **kw)
    masks = pred.predict_window(*args, to_host=False)
    assert torch.equal(masks, plain)                                          # nothing else in the predictor changes
    regions = pred.window_regions()
    assert len(regions) == DELTA and len(pred._window_regions) == 2 and len(pred._region_chunks) == 2
    rows, _ = pred.region_report()
    tracks, _ = pred.track_report()
    pal = np.concatenate([np.array([[0, 0, 0], [30, 95, 170], [65, 117, 5], [212, 98, 1], [255, 244, 116]], np.uint8),
                          np.array([[64], [160], [160], [96], [128]], np.uint8)], axis=1)
    line = np.full((5, 4), 255, np.uint8)
    style = dict(fill_palette=FILL, outline=line, outline_width=1, label_scale=1, label_min_area=4)
    host = masks.cpu().numpy()
    index = rref.region_table(host, rref.mask_regions(host, 5, 4), 5, None, 128, 64)[2]
    got = [buf.cpu().numpy() for buf in compose_window(masks, item, pal, out_fmt="nv12", out_matrix="bt709", dataset=ds, regions=regions, style=style)]
    old = [buf.cpu().numpy() for buf in compose_window(masks, item, pal, out_fmt="nv12", out_matrix="bt709", dataset=ds)]
    labelled = 0
    for p in range(DELTA):
        idx, table, counts, tr = regions[p]
        assert np.array_equal(idx.cpu().numpy(), index[p]) and int(counts[1]) == len(rows[p]) == len(tracks[p])
        tab, trk = np.zeros((64, 10), np.int64), np.full((64, 4), -1, np.int64)
        tab[:len(rows[p])], trk[:len(rows[p])] = rows[p], tracks[p]
        frame, chroma, fmt, matrix, full_range = ds.source(item["frame_id"] + p)
        bg = egress_ref.background(frame.cpu().numpy(), size=size)
        assert fmt == "rgb24" and chroma is None
        cnt = np.array([len(rows[p]), len(rows[p])])
        want = nv12_bytes(vref.compose(host[p], pal, index[p], "i420", "bt709", False, bg=bg, table=tab, counts=cnt, tracks=trk, **style), *size)
        assert np.array_equal(got[p], want), (p, first_difference(got[p], want))
        assert np.array_equal(old[p], nv12_bytes(egress_ref.compose(host[p], pal, bg, "i420", "bt709", False), *size))
        assert not np.array_equal(got[p], old[p])
        labelled += len(vref.labels(size[0], size[1], 64, tab, cnt, trk, 1, 4))
    assert labelled >= DELTA
    mixed = [buf.cpu().numpy() for buf in compose_window(masks[:2], item, pal, out_fmt="nv12", out_matrix="bt709", dataset=ds,
                                                         regions=[None, regions[1]], style=style)]
    assert np.array_equal(mixed[0], old[0]) and np.array_equal(mixed[1], got[1])   # None: that frame without layers
