"""Holding one key frame across a detected scene cut, on the GPU: ops.window_weights (csrc/motion_ops.hip), the weighted instantiations
of the two fused tails (csrc/flow_ops.hip through seg_tail_weighted / crops_fuse_weighted of the third hook table), and one window end
to end (RawVideoWindows(hold_cuts=True) -> FlowPredictor, whole frame and sliding crops).

Tolerances: the weights are compared with torch.equal (tests/cut_ref.py), and so is everything a held frame is compared with inside
the fused tails -- a held frame IS one chain's value.  The one comparison against another ROUTE (the warp chain built from
ops.grid_sample / ops.resize_bilinear) takes LOGIT_TOL of tests/test_gpu_net.py, as the other seg-tail comparisons do."""
import numpy as np
import pytest
import torch

import cut_ref
import motion_modes_ref as modes_ref
from conftest import rel_err
from flood_uav_video_segmentation_amd import ops, synth
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor
from test_gpu_net import LOGIT_TOL

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def cu(ts):
    return [t.cuda() for t in ts]


def stats_of(cuts):
    """Synthetic stats tensors as block_match_modes writes them: (blocks, intra blocks, cut, 0); None stays None."""
    return [None if c is None else torch.tensor([8040, 5000 if c else 3, int(bool(c)), 0], dtype=torch.int32, device="cuda") for c in cuts]


def weights_for(cuts):
    return ops.window_weights(stats_of(cuts), len(cuts))[0]


# ------------------------------------------------------------------------------------------------ window_weights
def cut_patterns(n):
    yield [0] * n
    for c in range(n):                                    # every single-cut position
        yield [int(j == c) for j in range(n)]
    if n >= 2:                                            # two cuts: the ends, neighbours, and every pair for the small n
        for a in range(n):
            for b in range(a + 1, n):
                yield [int(j in (a, b)) for j in range(n)]
        yield [1] * n


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_window_weights_equal_the_definition(n):
    for cuts in cut_patterns(n):
        for nulls in ((), (0,), (n - 1,), tuple(range(n))):          # null entries: "not estimated, no cut" whatever they hid
            given = [None if j in nulls else c for j, c in enumerate(cuts)]
            want_w, want_s = cut_ref.window_weights(given, n)
            w, s = ops.window_weights(stats_of(given), n)
            assert w.is_cuda and w.dtype == torch.float32 and w.shape == (n, 2) and s.dtype == torch.int32 and s.shape == (n,)
            assert torch.equal(w.cpu(), torch.from_numpy(want_w)) and torch.equal(s.cpu(), torch.from_numpy(want_s)), (given, w, s)


def test_window_weights_64_frames_and_only_the_cut_flag_counts():
    cuts = [0] * 64
    cuts[40] = 1
    w, s = ops.window_weights(stats_of(cuts), 64)
    want_w, want_s = cut_ref.window_weights(cuts, 64)
    assert torch.equal(w.cpu(), torch.from_numpy(want_w)) and torch.equal(s.cpu(), torch.from_numpy(want_s))
    many_intra = [torch.tensor([8040, 8040, 0, 7], dtype=torch.int32, device="cuda") for _ in range(5)]    # index 2 alone decides
    assert torch.equal(ops.window_weights(many_intra, 5)[1].cpu(), torch.zeros(5, dtype=torch.int32))


def test_window_weights_in_a_hip_graph_follow_the_stats_of_each_replay():
    n = 5
    stats = stats_of([0] * n)
    ops.window_weights(stats, n)                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        w, s = ops.window_weights(stats, n)
    for cuts in ([0, 0, 1, 0, 0], [0] * n, [1, 0, 0, 0, 1], [0, 0, 0, 0, 1]):
        for t, c in zip(stats, cuts):
            t[2] = c
        graph.replay()
        torch.cuda.synchronize()
        want_w, want_s = cut_ref.window_weights(cuts, n)
        assert torch.equal(w.cpu(), torch.from_numpy(want_w)) and torch.equal(s.cpu(), torch.from_numpy(want_s)), cuts


# ------------------------------------------------------------------------------------------------ the whole-frame tail
H, W, LH, LW, GH, GW = 33, 47, 9, 12, 5, 7
CASES = [(k, n, no_warp) for k in (5, 9) for n in (2, 5) for no_warp in (False, True)]


def tail_inputs(k, n, no_warp, seed=7):
    g = torch.Generator().manual_seed(seed + 100 * k + n)
    lo_p, lo_n = torch.randn(1, k, LH, LW, generator=g).cuda(), torch.randn(1, k, LH, LW, generator=g).cuda()
    mvl, mvr = synth.dummy_grids(n) if no_warp else synth.make_grids(n, GH, GW, seed=3, frame=(H, W), jitter=0.05)
    return lo_p, lo_n, cu(mvl), cu(mvr)


def all_outputs(lo_p, lo_n, mvl, mvr, n, no_warp, weights):
    """Every output mode of the seg tail: (logits, mask, canvas, count)."""
    kw = {} if weights is None else {"weights": weights}
    logits, mask = ops.seg_tail(lo_p, lo_n, mvl, mvr, n, (H, W), no_warp, want_logits=True, want_mask=True, **kw)
    only = ops.seg_tail(lo_p, lo_n, mvl, mvr, n, (H, W), no_warp, want_logits=False, want_mask=True, **kw)[1]
    assert torch.equal(only, mask)
    canvas = torch.zeros(n, lo_p.shape[1], H + 6, W + 9, dtype=torch.float64, device="cuda")
    count = torch.zeros(H + 6, W + 9, dtype=torch.float64, device="cuda")
    for y0, x0 in ((0, 0), (6, 9)):
        ops.seg_tail_accumulate(lo_p, lo_n, mvl, mvr, n, (H, W), no_warp, canvas, count, y0, x0, **kw)
    return logits, mask, canvas, count


@pytest.mark.parametrize("k,n,no_warp", CASES)
def test_no_cut_weights_give_todays_bits(k, n, no_warp):
    lo_p, lo_n, mvl, mvr = tail_inputs(k, n, no_warp)
    plain = all_outputs(lo_p, lo_n, mvl, mvr, n, no_warp, None)
    weighted = all_outputs(lo_p, lo_n, mvl, mvr, n, no_warp, weights_for([0] * n))
    for a, b in zip(plain, weighted):
        assert torch.equal(a, b)


@pytest.mark.parametrize("k,n", [(5, 2), (5, 5), (9, 2), (9, 5)])
def test_no_warp_cut_holds_each_key_frame_bit_for_bit(k, n):
    lo_p, lo_n, mvl, mvr = tail_inputs(k, n, True)
    prev0 = [t[0] for t in all_outputs(lo_p, None, [], [], 1, True, None)[:3]]       # frame 0 of either key frame: its upsampled logits
    next0 = [t[0] for t in all_outputs(lo_n, None, [], [], 1, True, None)[:3]]
    also = [t[0] for t in all_outputs(lo_n, lo_p, mvl, mvr, n, True, None)[:3]]       # "lo_next in lo_prev's place"
    assert all(torch.equal(a, b) for a, b in zip(next0, also))
    for c in range(1, n + 1):
        cuts = [int(j == c) for j in range(1, n + 1)]
        logits, mask, canvas, _ = all_outputs(lo_p, lo_n, mvl, mvr, n, True, weights_for(cuts))
        for f in range(n):
            want = prev0 if f < c else next0
            assert torch.equal(logits[f], want[0]) and torch.equal(mask[f], want[1]) and torch.equal(canvas[f], want[2]), (c, f)


def one_chain(lo, grids, steps):
    """The warp chain of one direction from the existing ops: up(lo) warped by grids[0], then each result by the next grid, every
    map upsampled to the frame (flow/model.py, predict_segmentation).  Returns the `steps` maps [K,H,W]."""
    cur = ops.resize_bilinear(lo, (H, W), align_corners=True)
    out = []
    for g in grids[:steps]:
        cur = ops.grid_sample(cur, g, align_corners=False)
        out.append(ops.resize_bilinear(cur, (H, W), align_corners=True)[0])
    return out


@pytest.mark.parametrize("k,n", [(5, 2), (5, 5), (9, 5)])
def test_warp_cut_holds_one_chain(k, n):
    lo_p, lo_n, mvl, mvr = tail_inputs(k, n, False)
    fwd, bwd = one_chain(lo_p, mvl, n - 1), one_chain(lo_n, mvr, n - 1)
    plain = ops.seg_tail(lo_p, lo_n, mvl, mvr, n, (H, W), False)[0]
    scale = float(plain.abs().max())
    for c in range(1, n + 1):
        cuts = [int(j == c) for j in range(1, n + 1)]
        logits, mask, canvas, count = all_outputs(lo_p, lo_n, mvl, mvr, n, False, weights_for(cuts))
        assert torch.equal(logits[0], plain[0])
        for f in range(1, n):
            want = fwd[f - 1] if f < c else bwd[n - f - 1]
            err = float((logits[f] - want).abs().max()) / scale
            print(f"K={k} n={n} cut at pair {c} frame {f}: held chain vs op-by-op route, max err / max|logit| = {err:.3e}")
            assert err < LOGIT_TOL, (c, f, err)
            assert torch.equal(mask[f], ops.argmax_u8(logits[f:f + 1])[0])
        # the canvas mode holds the same values: softmax of the held logits, added twice where the two placements overlap
        soft = torch.softmax(logits.double(), 1)
        assert rel_err(canvas[:, :, 6:H, 9:W].cpu(), (soft[:, :, 6:, 9:W] + soft[:, :, :H - 6, :W - 9]).cpu()) < 1e-6


@pytest.mark.parametrize("k,no_warp", [(5, False), (5, True), (9, False), (9, True)])
def test_a_non_finite_unused_key_frame_does_not_reach_a_held_frame(k, no_warp):
    n = 5
    lo_p, lo_n, mvl, mvr = tail_inputs(k, n, no_warp)
    for cuts, dirty_next in (([0, 0, 0, 0, 1], True), ([1, 0, 0, 0, 0], False), ([0, 0, 1, 0, 0], True), ([0, 0, 1, 0, 0], False)):
        w = weights_for(cuts)
        clean = all_outputs(lo_p, lo_n, mvl, mvr, n, no_warp, w)
        bad = (lo_n if dirty_next else lo_p).clone()
        bad[0, :, ::2, ::3] = float("nan")
        bad[0, :, 1::2, 1::3] = float("-inf")
        dirty = all_outputs(lo_p, bad, mvl, mvr, n, no_warp, w) if dirty_next else all_outputs(bad, lo_n, mvl, mvr, n, no_warp, w)
        first = cuts.index(1) + 1
        held = [f for f in range(n) if (f < first) == dirty_next]            # the frames that do not use the dirty key frame
        assert held and (dirty_next or 0 not in held)
        for f in held:
            for a, b in zip(clean[:3], dirty[:3]):
                assert torch.isfinite(b[f].double()).all() and torch.equal(a[f], b[f]), (cuts, dirty_next, f)


# ------------------------------------------------------------------------------------------------ sliding crops
@pytest.mark.parametrize("n,no_warp", [(2, False), (5, False), (5, True), (7, False)])
def test_crops_fuse_with_weights_equals_per_crop_accumulation(n, no_warp):
    """Two overlapping 32 x 32 crops of a 32 x 48 frame, K = 5 (n = 7: two register chunks of frames): no-cut weights give the
    unweighted call's bits; with a cut crops_fuse(weights) equals seg_tail_accumulate(weights) per crop + canvas_finish, bit for bit,
    canvas and masks, and a held frame ignores a non-finite other key frame."""
    g = torch.Generator().manual_seed(13 + n)
    k, ch, cw, fh, fw = 5, 32, 32, 32, 48
    yx = [(0, 0), (0, 16)]
    lo_p, lo_n = torch.randn(2, k, 5, 6, generator=g).cuda(), torch.randn(2, k, 5, 6, generator=g).cuda()
    grids = None
    if not no_warp:
        mvl, mvr = synth.make_grids(n, 4, 6, seed=5, frame=(fh, fw), jitter=0.04)
        grids = ops.crop_grids(cu(mvl) + cu(mvr), (fh, fw), yx, (ch, cw))

    def per_crop(weights, lo_next=lo_n):
        canvas = torch.zeros(n, k, fh, fw, dtype=torch.float64, device="cuda")
        count = torch.zeros(fh, fw, dtype=torch.float64, device="cuda")
        for c, (y0, x0) in enumerate(yx):
            gl = [grids[c, j][None] for j in range(n - 1)] if grids is not None else cu(synth.dummy_grids(n)[0])
            gr = [grids[c, n - 1 + j][None] for j in range(n - 1)] if grids is not None else cu(synth.dummy_grids(n)[1])
            ops.seg_tail_accumulate(lo_p[c:c + 1], lo_next[c:c + 1], gl, gr, n, (ch, cw), no_warp, canvas, count, y0, x0, weights=weights)
        assert float(count.max()) == 2.0 and float(count.min()) == 1.0
        return canvas, ops.canvas_finish(canvas, count, None, want_mask=True)

    plain = ops.crops_fuse(lo_p, lo_n, grids, yx, (ch, cw), n, no_warp, (fh, fw), want_canvas=True, want_mask=True)
    same = ops.crops_fuse(lo_p, lo_n, grids, yx, (ch, cw), n, no_warp, (fh, fw), want_canvas=True, want_mask=True, weights=weights_for([0] * n))
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1], same[1])
    for c in sorted({1, (n + 1) // 2, n}):
        w = weights_for([int(j == c) for j in range(1, n + 1)])
        ref_c, ref_m = per_crop(w)
        canvas, mask = ops.crops_fuse(lo_p, lo_n, grids, yx, (ch, cw), n, no_warp, (fh, fw), want_canvas=True, want_mask=True, weights=w)
        assert torch.equal(canvas, ref_c) and torch.equal(mask, ref_m), c
        none, only = ops.crops_fuse(lo_p, lo_n, grids, yx, (ch, cw), n, no_warp, (fh, fw), want_canvas=False, want_mask=True, weights=w)
        assert none is None and torch.equal(only, ref_m)
        assert torch.equal(canvas[0], plain[0][0]) and not torch.equal(canvas[1:], plain[0][1:])
        bad = lo_n.clone()
        bad[:, :, ::2, ::2] = float("nan")
        dirty = ops.crops_fuse(lo_p, bad, grids, yx, (ch, cw), n, no_warp, (fh, fw), want_canvas=True, want_mask=True, weights=w)
        assert torch.equal(dirty[0][:c], canvas[:c]) and torch.equal(dirty[1][:c], mask[:c]) and torch.isfinite(dirty[0][:c]).all()
    with pytest.raises(RuntimeError, match="weights"):
        ops.crops_fuse(lo_p, lo_n, grids, yx, (ch, cw), n, no_warp, (fh, fw), weights=torch.zeros(n + 1, 2, device="cuda"))
    with pytest.raises(RuntimeError, match="weights"):
        ops.seg_tail(lo_p[:1], lo_n[:1], [], [], n, (ch, cw), True, weights=torch.zeros(n, 2, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------------------------------------ one window, end to end
FH, FW, FRAMES, DELTA = 1072, 1920, 11, 5


@pytest.fixture(scope="module")
def scenes():
    """The scenes of tests/test_gpu_motion_modes.py's planted-cut window: a dark texture and a bright one, each panning by 8 rows a
    frame (translated: no cut inside a scene; unrelated across the two: a cut)."""
    return (modes_ref.textured_frame(FH + 8 * FRAMES, FW, seed=51, channels=3),
            modes_ref.textured_frame(FH + 8 * FRAMES, FW, seed=52, channels=3, levels=modes_ref.BRIGHT))


@pytest.fixture(scope="module")
def flow_model():
    from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

    class HP:
        layers, classes, pretrained = 50, 5, False

    net = FlowPSPNet(HP()).eval()
    net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
    return FlowModel(net, feature_based=False, no_warp=False).eval()


@pytest.mark.parametrize("cut_at,want_source", [(7, [1, 1, 2, 2, 2]), (10, [1, 1, 1, 1, 1])])
def test_window_with_a_planted_cut_holds_the_key_frame_of_each_side(tmp_path, scenes, flow_model, cut_at, want_source):
    """Window 1 (frames 5..10) of an eleven-frame 1072 x 1920 clip whose scene changes at frame `cut_at`: inside the window (pair
    6 -> 7), or on the closing pair (9 -> 10), which feeds no grid and is searched for hold_cuts alone."""
    a, b = scenes
    path = str(tmp_path / "clip.rgb")
    with open(path, "wb") as fh:
        for i in range(FRAMES):
            fh.write(np.ascontiguousarray((a if i < cut_at else b)[8 * i:8 * i + FH]).tobytes())
    common = dict(frame_delta=DELTA, grids="estimate", search=8, penalty=0, intra_bias=0, scene_cut=0.5)
    for size, crop in (((65, 65), None), ((65, 97), (65, 65))):       # the whole-frame route; two overlapping sliding crops
        ds = RawVideoWindows(path, FH, FW, "rgb24", size=size, hold_cuts=True, **common)
        off = RawVideoWindows(path, FH, FW, "rgb24", size=size, **common)
        item, plain = ds[1], off[1]
        assert "weights" not in plain and "source" not in plain and off.estimator.stats_for(10) is None     # no extra search without it
        assert ds.estimator.stats_for(10) is not None and sorted(ds.estimator.estimated_stats()) == [6, 7, 8, 9, 10]
        assert item["weights"].is_cuda and item["weights"].shape == (DELTA, 2) and item["source"].cpu().tolist() == want_source
        want_w = cut_ref.window_weights([int(j == cut_at) for j in range(6, 11)], DELTA)[0]
        assert torch.equal(item["weights"].cpu(), torch.from_numpy(want_w))
        for key in ("frame_prev", "frame_next"):
            assert torch.equal(item[key], plain[key])
        assert all(torch.equal(x, y) for key in ("mvs_left", "mvs_right") for x, y in zip(item[key], plain[key]))
        pred = FlowPredictor(flow_model, classes=5, out_size=size, crop=crop, compute_metrics=False, cache_keyframes=False)

        def run(it, frame_prev=None, frame_next=None, weights=None):
            return pred.predict_window(it["frame_prev"] if frame_prev is None else frame_prev, it["frame_next"] if frame_next is None else frame_next,
                                       it["mvs_left"], it["mvs_right"], to_host=False, weights=weights)

        held = run(item, weights=item["weights"])
        blended = run(plain)
        assert held.shape == blended.shape == (DELTA, *size) and torch.equal(held[0], blended[0])
        # hold_cuts off is the unweighted call, and so is a window item that carries no weights
        assert torch.equal(blended, run(item)) and torch.equal(blended, next(iter(pred.predict_clip([dict(plain)], to_host=False))))
        assert torch.equal(held, next(iter(pred.predict_clip([dict(item)], to_host=False))))
        garbage = torch.randn(item["frame_prev"].shape, generator=torch.Generator().manual_seed(9)).cuda() * 3
        from_prev = [f for f, s in enumerate(want_source) if s == 1]
        from_next = [f for f, s in enumerate(want_source) if s == 2]
        no_next = run(item, frame_next=garbage, weights=item["weights"])
        assert torch.equal(no_next[from_prev], held[from_prev])
        if from_next:
            no_prev = run(item, frame_prev=garbage, weights=item["weights"])
            assert torch.equal(no_prev[from_next], held[from_next])
