"""Motion-compensated region links on the GPU: region_links_mc (csrc/track_ops.hip through the third hook table) against the numpy
definition (tests/tracks_mc_ref.py) by integer equality, against ops.region_links itself where the two must agree, the moving-blob scene
end to end through FlowPredictor(compensate=True), and one HIP-graph capture.  The geometries are the smallest that exercise one way the
kernel can go wrong each (tracks_mc_ref.GEOMETRIES); none is the workload's own size."""
import numpy as np
import pytest
import torch

import tracks_mc_ref as mc
import tracks_ref as ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor
from test_gpu_regions import DELTA, FH, FW, Guarded, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
OUTPUTS = ("back", "fwd", "link_counts", "tracks", "state")
GROUPS = 5


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # a copy: the shared expectations are read-only


def run_guarded(e, offset, prev=None, prev_tracks=None, state=(0, 0), frames=slice(None)):
    """The two ops through the library itself, every output and the workspace inside a guarded buffer at element `offset`."""
    lib = _lib.load()
    index, table, counts, mv = (dev(e[k][frames]) for k in ("index", "table", "counts", "mv"))
    stats = dev(None if e["pair_stats"] is None else e["pair_stats"][frames])
    n, h, w = index.shape
    cap, pairs, (fh, fw) = e["cap"], e["max_pairs"], e["frame_size"]
    back, fwd = Guarded((n, cap, 2), torch.int32, offset), Guarded((n, cap, 2), torch.int32, offset)
    link_counts, tracks, st = Guarded((n, 2), torch.int64, offset), Guarded((n, cap, 4), torch.int64, offset), Guarded((2,), torch.int64, offset)
    work = Guarded((ops.region_links_mc_workspace_bytes(n, cap, pairs, fh // 16, fw // 16) // 8,), torch.int64, offset)
    st.view.copy_(torch.tensor(state, dtype=torch.int64))
    p = (None, None, None) if prev is None else prev
    check(lib.fs_region_links_mc(ptr(index), ptr(table), ptr(counts), ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(mv), ptr(stats), n, h, w, fh, fw, cap, pairs,
                                 e["min_overlap"], ptr(back.view), ptr(fwd.view), ptr(link_counts.view), ptr(work.view), stream_ptr()))
    check(lib.fs_region_tracks(ptr(back.view), ptr(fwd.view), ptr(counts), ptr(prev_tracks), n, cap, ptr(st.view), ptr(tracks.view), stream_ptr()))
    torch.cuda.synchronize()
    assert all(g.intact() for g in (back, fwd, link_counts, tracks, st, work)), (e["name"], offset)
    return back.view, fwd.view, link_counts.view, tracks.view, st.view


def links(e, frames=slice(None), prev=None):
    stats = None if e["pair_stats"] is None else dev(e["pair_stats"][frames])
    return ops.region_links(dev(e["index"][frames]), dev(e["table"][frames]), dev(e["counts"][frames]), prev, e["max_pairs"], e["min_overlap"],
                            mv=dev(e["mv"][frames]), frame_size=e["frame_size"], pair_stats=stats)


@pytest.mark.parametrize("group", range(GROUPS))
def test_every_case_equals_the_definition(group):
    """Every geometry with every table -- the garbage ones among them --, the blobs, the full and the overflowing pair table and the cut:
    through ops, and through the library with guarded outputs and workspace at element offsets 4, 1 and 3."""
    for i in range(group, len(mc.case_list()), GROUPS):
        e = mc.expected(i)
        back, fwd, link_counts = links(e)
        state = torch.zeros(2, dtype=torch.int64, device=DEV)
        tracks = ops.region_tracks(back, fwd, dev(e["counts"]), state)
        for got, key in zip((back, fwd, link_counts, tracks, state), OUTPUTS):
            assert got.dtype == dev(e[key]).dtype and torch.equal(got, dev(e[key])), (e["name"], key)
        for offset in (4, 1, 3):
            for got, key in zip(run_guarded(e, offset), OUTPUTS):
                assert torch.equal(got, dev(e[key])), (e["name"], key, offset)


@pytest.mark.parametrize("name", ["(37, 300, 48, 320) random5 per_block", "(96, 160, 48, 80) random5 garbage", "(50, 90, 50, 90) random5 pm32", "cut"])
def test_single_frames_and_chained_calls_equal_one_call(name):
    """n = 1 without and with the frame before, n = 3, and 1 + 1 + 1 against one call of 3 (through ops, and guarded with a previous frame)."""
    e = mc.expected(mc.case_by_name(name))
    want = [dev(e[k]) for k in OUTPUTS]
    index, table, counts = dev(e["index"]), dev(e["table"]), dev(e["counts"])
    for pieces in ([3], [1, 1, 1], [1, 2]):
        state = torch.zeros(2, dtype=torch.int64, device=DEV)
        got, prev, prev_tracks, at = [[], [], [], []], None, None, 0
        for n in pieces:
            s = slice(at, at + n)
            back, fwd, lc = links(e, s, prev)
            tracks = ops.region_tracks(back, fwd, counts[s], state, prev_tracks)
            for lst, t in zip(got, (back, fwd, lc, tracks)):
                lst.append(t)
            at += n
            prev, prev_tracks = (index[at - 1].contiguous(), table[at - 1].contiguous(), counts[at - 1].contiguous()), tracks[-1]
        assert all(torch.equal(torch.cat(g), w) for g, w in zip(got, want)) and torch.equal(state, want[4]), pieces
    head = mc.chained(e, [1])
    prev = (index[0].contiguous(), table[0].contiguous(), counts[0].contiguous())
    for frames in (slice(1, 2), slice(1, 3)):                                  # n = 1 and n = 2 with the frame before, guarded
        got = run_guarded(e, 1, prev, dev(head[3][0]), tuple(head[4].tolist()), frames)
        for g, key in zip(got[:4], OUTPUTS):
            assert torch.equal(g, dev(e[key][frames])), (key, frames)
    assert torch.equal(got[4], want[4])


@pytest.mark.parametrize("group", range(ref.GROUPS))
def test_void_and_zero_tables_equal_region_links_itself(group):
    """All-void and all-zero tables, on a frame of the mask's size and on another one: bit for bit ops.region_links' outputs."""
    for i in ref.cases_of(group)[::4]:
        e = ref.expected(i)
        index, table, counts = dev(e["index"]), dev(e["table"]), dev(e["counts"])
        n, h, w = index.shape
        want = ops.region_links(index, table, counts, None, e["max_pairs"], e["min_overlap"])
        assert all(torch.equal(g, dev(e[k])) for g, k in zip(want, OUTPUTS))
        for fh, fw in ((max(h, 16), max(w, 16)), (48, 320)):
            for one in (mc.table_void(fh, fw), mc.table_uniform(fh, fw, 0, 0)):
                got = ops.region_links(index, table, counts, None, e["max_pairs"], e["min_overlap"], mv=dev(np.stack([one] * n)), frame_size=(fh, fw))
                assert all(torch.equal(g, w_) for g, w_ in zip(got, want)), (e["name"], fh, fw)


@pytest.mark.parametrize("name", ["(37, 300, 48, 320) stripes per_block", "(48, 80, 48, 80) random5 outward", "(96, 160, 48, 80) random5 void_mixed",
                                  "(50, 90, 50, 90) random5 garbage"])
def test_one_frame_equals_region_links_on_a_plane_warped_beforehand(name):
    e = mc.expected(mc.case_by_name(name))
    index, table, counts = dev(e["index"]), dev(e["table"]), dev(e["counts"])
    n, h, w = index.shape
    yy, xx = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
    for f in range(1, n):
        sy, sx = (dev(a) for a in mc.shifts(e["mv"][f], h, w, *e["frame_size"]))
        ys, xs = yy + sy, xx + sx
        inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
        warped = torch.where(inside, index[f - 1][ys.clamp(0, h - 1), xs.clamp(0, w - 1)], torch.full_like(index[f - 1], -1)).contiguous()
        s = slice(f, f + 1)
        want = ops.region_links(index[s], table[s], counts[s], (warped, table[f - 1].contiguous(), counts[f - 1].contiguous()), e["max_pairs"], e["min_overlap"])
        got = links(e, s, (index[f - 1].contiguous(), table[f - 1].contiguous(), counts[f - 1].contiguous()))
        assert all(torch.equal(g, w_) for g, w_ in zip(got, want)) and all(torch.equal(g[0], dev(e[k][f])) for g, k in zip(got, OUTPUTS)), f
        assert int(got[2][0, 0]) > 50


def test_cpu_side_checks_of_the_new_arguments():
    e = mc.expected(mc.case_by_name("(48, 80, 48, 80) random5 uniform"))
    index, table, counts, mv = dev(e["index"]), dev(e["table"]), dev(e["counts"]), dev(e["mv"])
    stats = torch.zeros((3, 4), dtype=torch.int32, device=DEV)
    for bad in (dict(mv=mv), dict(frame_size=(48, 80)), dict(pair_stats=stats), dict(mv=mv, frame_size=(48, 96)), dict(mv=mv.long(), frame_size=(48, 80)),
                dict(mv=mv[:2], frame_size=(48, 80)), dict(mv=mv, frame_size=(48, 80), pair_stats=stats[:2]), dict(mv=mv, frame_size=(48, 80), pair_stats=stats.long()),
                dict(mv=mv, frame_size=(8, 80)), dict(mv=mv[:, :0], frame_size=(1, 2))):
        with pytest.raises(RuntimeError):
            ops.region_links(index, table, counts, **bad)
    got = ops.region_links(index[:0], table[:0], counts[:0], mv=mv[:0], frame_size=(48, 80))
    assert got[0].shape == (0, e["cap"], 2)


class BlobFlow(torch.nn.Module):
    """A flow model that returns the one-hot logits of the next frames of a fixed mask clip (a foreign network: no fused routes)."""
    feature_based = True
    no_warp = True

    def __init__(self, masks, channels):
        super().__init__()
        self.masks, self.channels, self.at = masks, channels, 0

    def predict(self, frame_prev, frame_next, mvs_left, mvs_right, n, profiler=None, **extra):
        m = self.masks[self.at:self.at + n].long()
        self.at += n
        return {"pred": torch.nn.functional.one_hot(m, self.channels).permute(0, 3, 1, 2).float().contiguous()}


def test_the_blob_scene_through_the_predictor():
    """Two windows of two frames: in place every region is born, compensated the definition's continuations appear."""
    e = mc.expected(mc.case_by_name("blobs"))
    masks, mv = dev(e["mask"]), dev(e["mv"])
    h, w = e["frame_size"]
    x = torch.zeros(1, 3, h, w, device=DEV)
    kw = dict(classes=5, out_size=(h, w), crop=None, compute_metrics=False, regions=True, track=True, max_regions=e["cap"])
    reports = {}
    for compensate in (False, True):
        p = FlowPredictor(BlobFlow(masks, ref.BG + 1), compensate=compensate, **kw)
        for wdw in range(2):
            s = slice(2 * wdw, 2 * wdw + 2)
            out = p.predict_window(x, x, [None], [None], to_host=False, link_mvs=mv[s], link_frame_size=(h, w))
            assert torch.equal(out, masks[s])
        reports[compensate] = p.track_report(with_cuts=True)
    for compensate, (rows, over, cuts) in reports.items():
        want, flags = mc.clip_tracks(e["mask"], 5, 8, e["cap"], e["mv"], (h, w), compensate=compensate)
        assert len(rows) == 4 and all(np.array_equal(g, w_) for g, w_ in zip(rows, want)) and not over.any() and not cuts.any() and not flags.any()
    assert all(np.array_equal(g, e["tracks"][f, :len(g)]) for f, g in enumerate(reports[True][0]))
    born, total, _ = mc.continued(reports[False][0])
    cont, _, ids = mc.continued(reports[True][0])
    assert (born, total) == (0, 48) and cont >= 40 and ids == 63 - cont


def test_windows_of_a_raw_video_are_linked_with_the_tables_the_dataset_hands_out(clip):  # noqa: F811
    """RawVideoWindows(link_vectors=True) -> predict_clip -> FlowPredictor(compensate=True): the item's tables are the matcher's, one per
    emitted frame, and the tracks are the definition's on the emitted masks with those tables."""
    size = (65, 65)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8, link_vectors=True)
    items = [ds[0], ds[1]]
    blocks = (FH // 16) * (FW // 16)
    for w, item in enumerate(items):
        assert item["link_frame_size"] == (FH, FW) and item["link_mvs"].shape == (DELTA, blocks, 7) and item["link_mvs"].dtype == torch.int32
        assert item["link_mvs"].is_cuda and "link_stats" not in item
    assert torch.equal(items[0]["link_mvs"][0], dev(mc.table_void(FH, FW)))                             # frame 0 has no frame before it
    assert torch.equal(items[1]["link_mvs"][0], ops.block_match(ds.raw_frame(DELTA), ds.raw_frame(DELTA - 1), search=8))   # the pair no grid needs
    assert torch.equal(items[1]["link_mvs"][2], ops.block_match(ds.raw_frame(DELTA + 2), ds.raw_frame(DELTA + 1), search=8))
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=False, cache_keyframes=False, regions=True, track=True, connectivity=4, min_overlap=2)
    on = FlowPredictor(fm, compensate=True, **kw)
    masks = torch.cat(list(on.predict_clip([dict(i) for i in items], to_host=False))).cpu().numpy()
    mvs = torch.cat([i["link_mvs"] for i in items]).cpu().numpy()
    want, flags = mc.clip_tracks(masks, 5, 4, 1024, mvs, (FH, FW), None, 2)
    got, over = on.track_report()
    assert len(got) == 2 * DELTA and all(np.array_equal(g, w_) for g, w_ in zip(got, want)) and np.array_equal(over, flags) and not over.any()
    assert sum(int((g[:, 2] >= 0).sum()) for g in got) > DELTA
    with pytest.raises(ValueError, match="link_"):                                                      # a window without its tables is never linked in place
        on.predict_window(items[0]["frame_prev"], items[0]["frame_next"], items[0]["mvs_left"], items[0]["mvs_right"], to_host=False)


def test_a_captured_graph_replayed_on_new_masks_and_vectors_gives_each_replays_result():
    """label -> table -> compensated links -> tracks in one graph; every replay links the masks with the vectors it finds."""
    a, b = mc.expected(mc.case_by_name("(37, 300, 48, 320) random5 per_block")), mc.expected(mc.case_by_name("(37, 300, 48, 320) stripes void_mixed"))
    k, cap, pairs, (fh, fw) = a["classes"], a["cap"], a["max_pairs"], a["frame_size"]
    assert b["cap"] == cap and b["classes"] == k and b["max_pairs"] == pairs and b["frame_size"] == (fh, fw)
    mask, mv = dev(a["mask"]), dev(a["mv"])
    n, h, w = mask.shape
    lib = _lib.load()
    labels, index = (torch.empty((n, h, w), dtype=torch.int32, device=DEV) for _ in range(2))
    table = torch.full((n, cap, 10), -12345, dtype=torch.int64, device=DEV)          # never cleared by the caller
    counts, link_counts = (torch.full((n, 2), -12345, dtype=torch.int64, device=DEV) for _ in range(2))
    work = torch.empty((n, -(-h * w // ops.REGION_RANK_CHUNK)), dtype=torch.int32, device=DEV)
    back, fwd = (torch.full((n, cap, 2), -12345, dtype=torch.int32, device=DEV) for _ in range(2))
    tracks = torch.full((n, cap, 4), -12345, dtype=torch.int64, device=DEV)
    pair_work = torch.full((ops.region_links_mc_workspace_bytes(n, cap, pairs, fh // 16, fw // 16) // 8,), -1, dtype=torch.int64, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)

    def run():
        s = stream_ptr()
        check(lib.fs_mask_regions(ptr(mask), n, h, w, k, ref.CONN, ptr(labels), s))
        check(lib.fs_region_table(ptr(mask), ptr(labels), None, n, h, w, k, 128, cap, ptr(table), ptr(counts), ptr(index), ptr(work), s))
        check(lib.fs_region_links_mc(ptr(index), ptr(table), ptr(counts), None, None, None, ptr(mv), None, n, h, w, fh, fw, cap, pairs, 1, ptr(back), ptr(fwd),
                                     ptr(link_counts), ptr(pair_work), s))
        check(lib.fs_region_tracks(ptr(back), ptr(fwd), ptr(counts), None, n, cap, ptr(state), ptr(tracks), s))

    run()
    torch.cuda.synchronize()
    assert torch.equal(tracks, dev(a["tracks"])) and torch.equal(state, dev(a["state"]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    next_id = int(a["state"][0])
    for e in (b, a, b):
        mask.copy_(dev(e["mask"]))
        mv.copy_(dev(e["mv"]))
        graph.replay()
        torch.cuda.synchronize()
        want, new = ref.region_tracks(e["back"], e["fwd"], e["counts"], np.array([next_id, 0], np.int64))
        assert int(new[0]) > next_id
        assert torch.equal(back, dev(e["back"])) and torch.equal(fwd, dev(e["fwd"])) and torch.equal(link_counts, dev(e["link_counts"]))
        assert torch.equal(tracks, dev(want)) and torch.equal(state, dev(new))
        next_id = int(new[0])
