"""The temporal mask stabiliser on the GPU (ops.mask_stabilize) against the numpy definition of tests/stabilize_ref.py,
bit for bit: the op on every shared case, chained calls (the ping-pong parity of the compensated route), void and zero tables, one
HIP-graph capture, and end to end through FlowPredictor(stabilize=N).  The geometries are tracks_mc_ref's plus three whose planes are no
multiple of four pixels (the ragged last thread, byte planes at every alignment)."""
import numpy as np
import pytest
import torch

import regions_ref as rref
import stabilize_ref as sref
import tracks_mc_ref as mc
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor
from test_gpu_regions import DELTA, FH, FW, Guarded, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = range(len(sref.case_list()))
COMBOS = [(bool(c & 1), bool(c & 2), bool(c & 4)) for c in range(8)]       # (conf, mv, pair_stats)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared expectations are read-only


def run(mask, state=None, **kw):
    """ops.mask_stabilize on numpy inputs -> numpy (out, state as uint32, counts)."""
    kw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    out, st, counts = ops.mask_stabilize(dev(mask), None if state is None else dev(np.asarray(state).view(np.int32)), **kw)
    return out.cpu().numpy(), st.cpu().numpy().view(np.uint32), counts.cpu().numpy()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("i", CASES)
def test_every_case_equals_the_definition(i):
    """n = 3..6 by case; every persistence with and without conf, mv and pair_stats: out, state and counts, bit for bit."""
    mask = sref.case_list()[i]["mask"]
    for persist in sref.PERSISTS:
        for flags in COMBOS:
            got = run(mask, **sref.case_kwargs(i, persist, *flags))
            assert same(got, sref.expected(i, persist, *flags)), (persist, flags)
            if persist == 1:
                assert np.array_equal(got[0], mask)                            # P = 1 is the identity on the masks
    c = sref.case_list()[i]
    assert np.array_equal(run(mask, conf=c["conf"], trust=0, persist=3)[0], mask)   # and so is T = 0


@pytest.mark.parametrize("i", [1, 3, 8, 10, 14, 20, 24, 27, 29])
def test_single_frames_and_chained_calls_equal_one_call(i):
    """Odd and even call lengths on both routes: on the compensated one the last frame of every call must land in the caller's plane."""
    c = sref.case_list()[i]
    mask, n = c["mask"], c["mask"].shape[0]
    for flags in ((True, True, True), (False, True, False), (True, False, True)):
        kw = sref.case_kwargs(i, 2, *flags)
        want = sref.expected(i, 2, *flags)
        for pieces in ((1,) * n, (2, n - 2), (n - 1, 1), (1, n - 1)):
            assert same(sref.chained(mask, pieces, run, **kw), want), (flags, pieces)


def test_the_state_plane_is_updated_in_place_and_nothing_else_is_touched():
    """Every output inside a guarded buffer, the byte planes at an odd offset; the state the caller passed is the one that comes back."""
    i = 25                                                                  # 37 x 301, garbage tables
    c = sref.case_list()[i]
    mask, (fh, fw) = c["mask"], c["frame_size"]
    n, h, w = mask.shape
    lib = _lib.load()
    for use_mv in (False, True):
        first = sref.mask_stabilize(mask[:1], None, c["conf"][:1], sref.K, 2, sref.TRUST)
        m, cf, out = Guarded((n - 1, h, w), torch.uint8, 1), Guarded((n - 1, h, w), torch.uint8, 3), Guarded((n - 1, h, w), torch.uint8, 1)
        m.view.copy_(dev(mask[1:]))
        cf.view.copy_(dev(c["conf"][1:]))
        state, counts = Guarded((h, w), torch.int32, 4), Guarded((n - 1, 4), torch.int64, 2)
        state.view.copy_(dev(first[1].view(np.int32)))
        hb, wb = (fh // 16, fw // 16) if use_mv else (0, 0)
        work = Guarded((max(ops.mask_stabilize_workspace_bytes(n - 1, h, w, hb, wb), 16) // 4,), torch.int32, 4)
        mv = dev(c["mv"][1:]) if use_mv else None
        check(lib.fs_mask_stabilize(ptr(m.view), ptr(cf.view), ptr(mv), None, n - 1, h, w, fh if use_mv else 0, fw if use_mv else 0, sref.K, 2, sref.TRUST, 1,
                                    ptr(state.view), ptr(out.view), ptr(counts.view), ptr(work.view) if use_mv else None, stream_ptr()))
        torch.cuda.synchronize()
        kw = dict(mv=c["mv"][1:], frame_size=(fh, fw)) if use_mv else {}
        want = sref.mask_stabilize(mask[1:], first[1], c["conf"][1:], sref.K, 2, sref.TRUST, **kw)
        assert same((out.view.cpu().numpy(), state.view.cpu().numpy().view(np.uint32), counts.view.cpu().numpy()), want)
        assert all(g.intact() for g in (m, cf, out, state, counts, work))


@pytest.mark.parametrize("i", [0, 7, 13, 19, 26])
def test_void_and_zero_tables_equal_the_uncompensated_launch(i):
    c = sref.case_list()[i]
    mask, n, (fh, fw) = c["mask"], c["mask"].shape[0], c["frame_size"]
    plain = run(mask, conf=c["conf"], trust=sref.TRUST, persist=3, pair_stats=c["pair_stats"])
    assert same(plain, sref.expected(i, 3, True, False, True))
    for table in (mc.table_void(fh, fw), mc.table_uniform(fh, fw, 0, 0)):
        got = run(mask, conf=c["conf"], trust=sref.TRUST, persist=3, pair_stats=c["pair_stats"], mv=np.stack([table] * n), frame_size=(fh, fw))
        assert same(got, plain)


def test_cpu_side_checks_of_the_arguments():
    mask = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    for kw, word in ((dict(persist=0), "persist"), (dict(persist=256), "persist"), (dict(trust=200), "needs conf"), (dict(classes=0), "classes"),
                     (dict(frame_size=(16, 16)), "goes with mv"), (dict(mv=torch.zeros((2, 1, 7), dtype=torch.int32, device=DEV)), "frame_size"),
                     (dict(mv=torch.zeros((2, 2, 7), dtype=torch.int32, device=DEV), frame_size=(16, 16)), "mv must be"),
                     (dict(state=torch.zeros((8, 8), dtype=torch.int64, device=DEV)), "state must be"),
                     (dict(pair_stats=torch.zeros((3, 4), dtype=torch.int32, device=DEV)), "pair_stats"),
                     (dict(conf=torch.zeros((2, 8, 9), dtype=torch.uint8, device=DEV)), "conf must be"),
                     (dict(out=torch.zeros((2, 8, 8), dtype=torch.int32, device=DEV)), "out must be")):
        with pytest.raises(RuntimeError, match=word):
            ops.mask_stabilize(mask, **kw)
    out, state, counts = ops.mask_stabilize(mask[:0])
    assert out.shape == (0, 8, 8) and counts.shape == (0, 4) and not state.any()


def test_a_captured_graph_replayed_on_new_masks_gives_each_replays_result():
    """Both routes in one graph on a single stream, each carrying its own state plane from replay to replay."""
    a, b = 6, 9                                                             # two cases of the (37, 300, 48, 320) geometry
    ca, cb = sref.case_list()[a], sref.case_list()[b]
    n = min(ca["mask"].shape[0], cb["mask"].shape[0])
    assert ca["mask"].shape[1:] == cb["mask"].shape[1:] and ca["frame_size"] == cb["frame_size"]
    _, h, w = ca["mask"].shape
    fh, fw = ca["frame_size"]
    lib = _lib.load()
    mask, conf, mv = dev(ca["mask"][:n]), dev(ca["conf"][:n]), dev(ca["mv"][:n])
    outs = [torch.full((n, h, w), 0xA5, dtype=torch.uint8, device=DEV) for _ in range(2)]
    states = [torch.zeros((h, w), dtype=torch.int32, device=DEV) for _ in range(2)]      # the word 0: no state
    counts = [torch.full((n, 4), -12345, dtype=torch.int64, device=DEV) for _ in range(2)]   # never cleared by the caller
    work = torch.full((ops.mask_stabilize_workspace_bytes(n, h, w, fh // 16, fw // 16) // 4,), -1, dtype=torch.int32, device=DEV)

    def launch():
        s = stream_ptr()
        check(lib.fs_mask_stabilize(ptr(mask), ptr(conf), None, None, n, h, w, 0, 0, sref.K, 2, sref.TRUST, 1, ptr(states[0]), ptr(outs[0]), ptr(counts[0]),
                                    None, s))
        check(lib.fs_mask_stabilize(ptr(mask), ptr(conf), ptr(mv), None, n, h, w, fh, fw, sref.K, 2, sref.TRUST, 1, ptr(states[1]), ptr(outs[1]),
                                    ptr(counts[1]), ptr(work), s))

    launch()                                                                # the kernels are loaded before the capture
    torch.cuda.synchronize()
    for st in states:
        st.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    want_state = [np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)]
    for c in (ca, cb, cb, ca):
        mask.copy_(dev(c["mask"][:n]))
        conf.copy_(dev(c["conf"][:n]))
        mv.copy_(dev(c["mv"][:n]))
        graph.replay()
        torch.cuda.synchronize()
        for route, kw in enumerate(({}, dict(mv=c["mv"][:n], frame_size=(fh, fw)))):
            want = sref.mask_stabilize(c["mask"][:n], want_state[route], c["conf"][:n], sref.K, 2, sref.TRUST, **kw)
            got = (outs[route].cpu().numpy(), states[route].cpu().numpy().view(np.uint32), counts[route].cpu().numpy())
            assert same(got, want), route
            want_state[route] = want[1]


# ------------------------------------------------------------------------------------------------ through the predictor
def test_predictor_stabilises_first_and_everything_downstream_sees_it(clip):  # noqa: F811
    """Three windows of the synthetic model: the returned masks are the definition applied to the masks of the stabilize=None run, the
    report is the definition's counts, reset() re-seeds, and the despeckle and the score see the stabilised masks."""
    size = (65, 65)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8)
    items = [ds[0], ds[1], ds[0]]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=True, cache_keyframes=False)
    args = [(i["frame_prev"], i["frame_next"], i["mvs_left"], i["mvs_right"]) for i in items]
    off = FlowPredictor(fm, stabilize=None, **kw)
    plain = [off.predict_window(*a, to_host=False).cpu().numpy() for a in args]
    assert off.stabilize_report().shape == (0, 4) and off._stabilize_state is None
    on = FlowPredictor(fm, stabilize=3, **kw)
    got = [on.predict_window(*a, to_host=False).cpu().numpy() for a in args]
    want = sref.mask_stabilize(np.concatenate(plain), None, None, 5, 3)
    assert np.array_equal(np.concatenate(got), want[0]) and np.array_equal(on.stabilize_report(), want[2])
    assert np.array_equal(on._stabilize_state.cpu().numpy().view(np.uint32), want[1])
    assert want[2][0, 2] == size[0] * size[1] and want[2][1:, 2].sum() == 0          # the first frame seeds, and only it
    score = FlowPredictor(fm, **kw)                                                # the temporal-consistency score of the stabilised masks
    for g in got:
        score._score(torch.from_numpy(g).to(DEV), DELTA)
    assert torch.equal(on.hist, score.hist)
    on.clear_report()                                                              # the counts go, the state stays
    assert on.stabilize_report().shape == (0, 4)
    again = on.predict_window(*args[1], to_host=False).cpu().numpy()
    chained = sref.mask_stabilize(plain[1], want[1], None, 5, 3)
    assert np.array_equal(again, chained[0]) and np.array_equal(on.stabilize_report(), chained[2])
    on.reset()                                                                     # a new video: the next frame seeds
    fresh = on.predict_window(*args[1], to_host=False).cpu().numpy()
    seeded = sref.mask_stabilize(plain[1], None, None, 5, 3)
    assert np.array_equal(fresh, seeded[0]) and np.array_equal(on.stabilize_report(), np.concatenate([chained[2], seeded[2]]))
    # trust, with the confidence plane left as computed; then the despeckle behind the stabiliser
    conf_off = FlowPredictor(fm, confidence=True, **kw)
    pm, pc = conf_off.predict_window(*args[1], to_host=False)
    tr = FlowPredictor(fm, confidence=True, stabilize=3, stabilize_trust=180, **kw)
    tm, tc = tr.predict_window(*args[1], to_host=False)
    twant = sref.mask_stabilize(pm.cpu().numpy(), None, pc.cpu().numpy(), 5, 3, 180)
    assert torch.equal(tc, pc) and np.array_equal(tm.cpu().numpy(), twant[0]) and np.array_equal(tr.stabilize_report(), twant[2])
    flt = FlowPredictor(fm, regions=True, min_region_area=9, stabilize=3, **kw)
    fgot = np.concatenate([flt.predict_window(*a, to_host=False).cpu().numpy() for a in args])
    table, counts, index = rref.region_table(want[0], rref.mask_regions(want[0], 5, 8), 5, None, 128, 1024)
    assert np.array_equal(fgot, rref.region_filter(want[0], index, table, 5, 9)) and np.array_equal(flt.despeckle_counts(), counts[:, 0])
    assert np.array_equal(np.concatenate(list(FlowPredictor(fm, stabilize=3, **kw).predict_clip([dict(i) for i in items[:2]]))), want[0][:2 * DELTA])


def test_the_compensated_route_takes_the_tables_the_dataset_hands_out(clip):  # noqa: F811
    """RawVideoWindows(link_vectors=True) -> predict_clip -> FlowPredictor(stabilize_compensate=True): the state is read along the item's
    tables; the tracks of the same predictor stay in place without compensate=True; a window without tables raises."""
    size = (65, 65)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8, link_vectors=True)
    items = [ds[0], ds[1]]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=False, cache_keyframes=False)
    plain = torch.cat(list(FlowPredictor(fm, **kw).predict_clip([dict(i) for i in items], to_host=False))).cpu().numpy()
    on = FlowPredictor(fm, stabilize=2, stabilize_compensate=True, regions=True, track=True, **kw)
    got = torch.cat(list(on.predict_clip([dict(i) for i in items], to_host=False))).cpu().numpy()
    mvs = torch.cat([i["link_mvs"] for i in items]).cpu().numpy()
    want = sref.chained(plain, (DELTA, DELTA), mv=mvs, frame_size=(FH, FW), classes=5, persist=2)
    assert np.array_equal(got, want[0]) and np.array_equal(on.stabilize_report(), want[2])
    rows, over = on.track_report()
    want_rows, flags = mc.clip_tracks(got, 5, 8, 1024, mvs, (FH, FW), compensate=False)
    assert all(np.array_equal(g, w_) for g, w_ in zip(rows, want_rows)) and np.array_equal(over, flags)
    with pytest.raises(ValueError, match="stabilize_compensate=True needs link_mvs"):
        on.predict_window(items[0]["frame_prev"], items[0]["frame_next"], items[0]["mvs_left"], items[0]["mvs_right"], to_host=False)
