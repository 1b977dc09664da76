"""Holding one key frame across a detected scene cut in the FEATURE tail, on the GPU: the weighted instantiations of feat_fuse_warp_kernel /
feat_fuse_nowarp_kernel (csrc/flow_ops.hip through feat_tail_weighted of the third hook table), and one window end to end
(RawVideoWindows(hold_cuts=True) -> FlowPredictor -> FlowModel.predict_feature).

Every comparison is torch.equal: the fused feature tail is bit-identical to the op-by-op route (tests/test_gpu_ops.py), a held map IS one
chain's value, and a blended map is fadd_rn(fmul_rn(wa, va), fmul_rn(wb, vb)) -- ops.blend on the two fitted chain maps."""
import functools
import random

import numpy as np
import pytest
import torch

import cut_ref
import motion_modes_ref as modes_ref
from flood_uav_video_segmentation_amd import ops, synth
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"

GEOMS = [
    # C, fh, fw, Hg, Wg, H0, W0, n
    (64, 17, 13, 8, 6, 9, 15, 5),        # everything resized, odd sizes
    (96, 12, 12, 12, 12, 7, 9, 3),       # grids at the feature size (same_g): the copy branch
    (68, 6, 5, 3, 3, 4, 4, 2),           # last XCD slab short
    (128, 5, 6, 11, 18, 5, 6, 7),        # grid larger than the map: the run loop reloads both register sets
    (64, 1, 1, 1, 1, 1, 1, 3),
    (384, 45, 45, 44, 44, 67, 120, 5),   # the Segmenter's token map at 713^2
]


def stats_of(cuts):
    """Synthetic stats tensors as block_match_modes writes them: (blocks, intra blocks, cut, 0); None stays None."""
    return [None if c is None else torch.tensor([8040, 5000 if c else 3, int(bool(c)), 0], dtype=torch.int32, device=DEV) for c in cuts]


def weights_for(cuts):
    """window_weights on planted stats: the device tensor the tail takes, checked against the definition."""
    w = ops.window_weights(stats_of(cuts), len(cuts))[0]
    assert torch.equal(w.cpu(), torch.from_numpy(cut_ref.window_weights(cuts, len(cuts))[0]))
    return w


def cut_at(c, n):
    """Cut flags of a window whose pair (c-1 -> c) is a cut, c = 1..n."""
    return [int(j == c) for j in range(1, n + 1)]


def make_inputs(C, fh, fw, Hg, Wg, H0, W0, n, seed, scale=3.0, reach=1.3):
    g = torch.Generator().manual_seed(seed)
    f = (torch.randn(1, C, fh, fw, generator=g) * scale).to(DEV).contiguous(memory_format=torch.channels_last)
    f_next = (torch.randn(1, C, fh, fw, generator=g) * scale).to(DEV).contiguous(memory_format=torch.channels_last)
    mk = lambda: (torch.rand(1, Hg, Wg, 2, generator=g) * 2 * reach - reach).to(DEV)  # noqa: E731  (grids reach outside [-1, 1])
    mvl, mvr = [mk() for _ in range(n - 1)], [mk() for _ in range(n - 1)]
    g0 = (torch.rand(1, H0, W0, 2, generator=g) * 2.2 - 1.1).to(DEV)
    return f, f_next, mvl, mvr, g0


def chain(f, grids):
    """One direction's warp chain op by op: grid_sample steps, each map fitted to the feature size (flow/model.py:135-151)."""
    fh, fw = f.shape[2:]
    cur, out = f, []
    for m in grids:
        cur = ops.grid_sample(cur, m, align_corners=False)
        out.append(cur if cur.shape[2:] == (fh, fw) else ops.resize_bilinear(cur, (fh, fw), align_corners=True))
    return out


class Case:
    """Inputs of one geometry and everything the tests compare with, computed ONCE and never written to."""

    def __init__(self, geom, seed, f_next_given=True, **kw):
        self.geom, self.n = geom, geom[7]
        self.f, self.f_next, self.mvl, self.mvr, self.g0 = make_inputs(*geom, seed=seed, **kw)
        if not f_next_given:
            self.f_next = None
        self.fwd = chain(self.f, self.mvl) if f_next_given else []
        self.bwd = chain(self.f_next, self.mvr) if f_next_given else []
        self.plain = {no_warp: self.run(no_warp, None) for no_warp in (False, True)}

    def run(self, no_warp, weights, f=None, f_next=None):
        f = self.f if f is None else f
        f_next = self.f_next if f_next is None else f_next
        return ops.feat_tail(f, f_next, self.mvl, self.mvr, self.n, no_warp, None if no_warp else self.g0, weights=weights)

    def sides(self, p, no_warp):
        """(va, vb) of map p >= 1 as whole maps: the previous / next key frame's value."""
        return (self.f, self.f_next) if no_warp else (self.fwd[p - 1], self.bwd[self.n - p - 1])

    def check(self, got, w_host, no_warp, what=""):
        """`got` against the definition for the weights w_host (numpy [n,2])."""
        nmaps = self.n if self.f_next is not None else 1
        assert got.shape == self.plain[no_warp].shape == (nmaps, *self.f.shape[1:]) and ops.is_channels_last_dense(got)
        assert torch.equal(got[0], self.plain[no_warp][0]), (what, 0)                       # map 0 never reads its weights
        for p in range(1, nmaps):
            va, vb = self.sides(p, no_warp)
            wa, wb = float(w_host[p, 0]), float(w_host[p, 1])
            want = va if wb == 0.0 else vb if wa == 0.0 else ops.blend(va, wa, vb, wb)
            assert torch.equal(got[p:p + 1], want), (what, self.geom, no_warp, p, wa, wb)


@functools.lru_cache(maxsize=None)
def case(i):
    return Case(GEOMS[i], seed=GEOMS[i][0] + GEOMS[i][1] + GEOMS[i][7])


ALL = list(range(len(GEOMS)))


@pytest.mark.parametrize("no_warp", [False, True])
@pytest.mark.parametrize("i", ALL)
def test_no_cut_weights_give_todays_bits(i, no_warp):
    c = case(i)
    assert torch.equal(c.run(no_warp, weights_for([0] * c.n)), c.plain[no_warp])
    assert torch.equal(c.run(no_warp, weights_for([None] * c.n)), c.plain[no_warp])


@pytest.mark.parametrize("i", ALL)
def test_no_warp_cut_holds_each_key_frame_bit_for_bit(i):
    c = case(i)
    for cut in range(1, c.n + 1):
        got = c.run(True, weights_for(cut_at(cut, c.n)))
        assert torch.equal(got[0], c.plain[True][0])
        for p in range(1, c.n):
            assert torch.equal(got[p:p + 1], c.f if p < cut else c.f_next), (cut, p)


@pytest.mark.parametrize("i", ALL)
def test_warp_cut_holds_one_chain_bit_for_bit(i):
    c = case(i)
    for cut in range(1, c.n + 1):
        got = c.run(False, weights_for(cut_at(cut, c.n)))
        assert torch.equal(got[0], c.plain[False][0])
        for p in range(1, c.n):
            want = c.fwd[p - 1] if p < cut else c.bwd[c.n - p - 1]
            assert torch.equal(got[p:p + 1], want), (cut, p)


@pytest.mark.parametrize("no_warp", [False, True])
@pytest.mark.parametrize("i", ALL)
def test_general_weights_blend_like_ops_blend(i, no_warp):
    """Rows window_weights never emits, a held row between them, and weights that do not add up to 1."""
    c = case(i)
    rows = [(0.25, 0.75), (0.6, 0.4), (1.0, 0.0), (0.0, 1.0), (1.5, -0.5), (0.3, 0.3)]
    w = np.array([(1.0, 0.0)] + [rows[(p + i) % len(rows)] for p in range(1, c.n)], dtype=np.float32)
    c.check(c.run(no_warp, torch.from_numpy(w).to(DEV)), w, no_warp)


@pytest.mark.parametrize("i", [0, 1, 3, 5])
def test_two_cuts_in_a_window(i):
    c = case(i)
    n = c.n
    for a, b in {(1, 2), (1, n), (2, n), (n - 1, n), (2, n - 1)}:
        if not 1 <= a < b <= n:
            continue
        cuts = [int(j in (a, b)) for j in range(1, n + 1)]
        want_w, want_s = cut_ref.window_weights(cuts, n)
        w, s = ops.window_weights(stats_of(cuts), n)
        assert torch.equal(s.cpu(), torch.from_numpy(want_s)) and torch.equal(w.cpu(), torch.from_numpy(want_w))
        for no_warp in (False, True):
            got = c.run(no_warp, w)
            c.check(got, want_w, no_warp, (a, b))
            for p in range(1, n):                                       # ... which names one chain per map: source 1 / 2, or 3 by 2 p <= n
                va, vb = c.sides(p, no_warp)
                prev_side = want_s[p] == 1 or (want_s[p] == 3 and 2 * p <= n)
                assert torch.equal(got[p:p + 1], va if prev_side else vb), (a, b, p)


def test_seeded_sweep_of_geometries_cut_patterns_and_modes():
    """20 seeded random geometries drawn as tests/test_gpu_ops.py::test_feat_tail_on_seeded_random_geometries draws them (grids larger and
    smaller than the map, 1-pixel maps, short and empty XCD slabs, n = 1 .. 7, a missing next key frame), each with a random cut pattern."""
    rnd = random.Random(1506)
    for it in range(20):
        C = 4 * rnd.choice([16, 17, 24, 31, 32, 33, 64, 96, 130])
        fh, fw = rnd.choice([(1, 1), (1, 9), (7, 1), (5, 6), (13, 11), (23, 31)])
        Hg, Wg = rnd.choice([(1, 1), (2, 3), (fh, fw), (2 * fh + 1, 3 * fw), (9, 4)])
        H0, W0 = rnd.choice([(1, 1), (fh, fw), (3, 5), (11, 17)])
        n = rnd.choice([1, 2, 3, 5, 7])
        no_warp, single = rnd.random() < 0.25, rnd.random() < 0.2
        ncuts = rnd.choice([0, 1, 1, 1, 2])
        where = set(rnd.sample(range(1, n + 1), min(ncuts, n)))
        cuts = [int(j in where) for j in range(1, n + 1)]
        c = Case((C, fh, fw, Hg, Wg, H0, W0, n), seed=2000 + it, f_next_given=not single, scale=2.0, reach=1.2)
        c.check(c.run(no_warp, weights_for(cuts)), cut_ref.window_weights(cuts, n)[0], no_warp, (it, cuts, single))


@pytest.mark.parametrize("no_warp", [False, True])
@pytest.mark.parametrize("i", [0, 1, 3])
def test_a_non_finite_unused_key_frame_does_not_reach_a_held_map(i, no_warp):
    c = case(i)
    n = c.n
    for cut, dirty_next in ((n, True), (1, False), ((n + 1) // 2, True), ((n + 1) // 2, False)):
        w = weights_for(cut_at(cut, n))
        clean = c.run(no_warp, w)
        bad = (c.f_next if dirty_next else c.f).clone()
        bad[0, ::2, ::2, ::3] = float("nan")
        bad[0, 1::2] = float("-inf")
        dirty = c.run(no_warp, w, f_next=bad) if dirty_next else c.run(no_warp, w, f=bad)
        held = [p for p in range(n) if (p < cut) == dirty_next]          # the maps that do not use the dirty key frame
        assert held and (dirty_next or 0 not in held)
        for p in held:
            assert torch.isfinite(dirty[p]).all() and torch.equal(dirty[p], clean[p]), (cut, dirty_next, p)
        other = [p for p in range(1, n) if p not in held]
        assert all(not torch.isfinite(dirty[p]).all() for p in other)     # ... and the test's poison does reach the maps that use it


@pytest.mark.parametrize("no_warp", [False, True])
def test_weighted_feat_tail_in_a_hip_graph_follows_the_weights_of_each_replay(no_warp):
    c = case(0)
    n = c.n
    patterns = [cut_at(3, n), [0] * n, cut_at(n, n), cut_at(1, n), [0, 1, 0, 1, 0]]
    eager = [c.run(no_warp, weights_for(p)).clone() for p in patterns]
    w = weights_for([0] * n).clone()
    c.run(no_warp, w)                                                     # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = c.run(no_warp, w)
    for p, want in zip(patterns, eager):
        w.copy_(weights_for(p))                                           # in place: the captured launches read this tensor
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), p


def test_ops_feat_tail_refuses_bad_weights_on_the_device():
    c = case(2)
    for w, word in ((torch.zeros(c.n, 2), "device"), (torch.zeros(c.n + 1, 2, device=DEV), "weights must be"),
                    (torch.zeros(c.n, 2, dtype=torch.float64, device=DEV), "weights must be"),
                    (torch.zeros(2, c.n, device=DEV).t(), "weights must be")):
        for no_warp in (False, True):
            with pytest.raises(RuntimeError, match=word):
                c.run(no_warp, w)


# ------------------------------------------------------------------------------------------------ one window, end to end
FH, FW, FRAMES, DELTA, SIZE = 1072, 1920, 11, 5, (65, 65)
SOURCES = {7: [1, 1, 2, 2, 2], 10: [1, 1, 1, 1, 1]}


@pytest.fixture(scope="module")
def windows(tmp_path_factory):
    """Window 1 (frames 5..10) of the eleven-frame planted-cut clip of tests/test_gpu_cut_hold.py, cut inside the window (pair 6 -> 7) or
    on the closing pair (9 -> 10): {cut frame: (item with weights, item of the same window without hold_cuts)}."""
    a = modes_ref.textured_frame(FH + 8 * FRAMES, FW, seed=51, channels=3)
    b = modes_ref.textured_frame(FH + 8 * FRAMES, FW, seed=52, channels=3, levels=modes_ref.BRIGHT)
    common = dict(frame_delta=DELTA, grids="estimate", search=8, penalty=0, intra_bias=0, scene_cut=0.5)
    out = {}
    for cut, want_source in SOURCES.items():
        path = str(tmp_path_factory.mktemp("feat_hold") / f"clip{cut}.rgb")
        with open(path, "wb") as fh:
            for i in range(FRAMES):
                fh.write(np.ascontiguousarray((a if i < cut else b)[8 * i:8 * i + FH]).tobytes())
        item = RawVideoWindows(path, FH, FW, "rgb24", size=SIZE, hold_cuts=True, **common)[1]
        plain = RawVideoWindows(path, FH, FW, "rgb24", size=SIZE, **common)[1]
        assert "weights" not in plain and item["source"].cpu().tolist() == want_source
        assert torch.equal(item["weights"].cpu(), torch.from_numpy(cut_ref.window_weights([int(j == cut) for j in range(6, 11)], DELTA)[0]))
        out[cut] = (item, plain)
    return out


@functools.lru_cache(maxsize=None)
def feature_model(arch):
    if arch == "pspnet":
        from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

        class HP:
            layers, classes, pretrained = 50, 5, False

        net = FlowPSPNet(HP()).eval()
        net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
    else:  # the smallest Segmenter of tests/test_gpu_vit.py
        from flood_uav_video_segmentation_amd.model.vit import VITSegmentModel

        net = VITSegmentModel(5, 96, patch_size=16, d_model=384, n_layers=2, dec_layers=1).eval()
        net.load_state_dict(synth.make_vit_state(5, 96, 16, 384, 2, 1, seed=5))
    return FlowModel(net, feature_based=True, no_warp=False).eval()


@pytest.mark.parametrize("arch,cut", [("pspnet", 7), ("pspnet", 10), ("vit", 7)])
def test_feature_mode_window_with_a_planted_cut_holds_the_key_frame_of_each_side(windows, arch, cut):
    item, plain = windows[cut]
    want_source = SOURCES[cut]
    fm = feature_model(arch)
    pred = FlowPredictor(fm, classes=5, out_size=SIZE, crop=None, compute_metrics=False, cache_keyframes=False)

    def run(it, frame_prev=None, frame_next=None, weights=None):
        return pred.predict_window(it["frame_prev"] if frame_prev is None else frame_prev, it["frame_next"] if frame_next is None else frame_next,
                                   it["mvs_left"], it["mvs_right"], to_host=False, weights=weights)

    held = run(item, weights=item["weights"])
    blended = run(plain)
    assert held.shape == blended.shape == (DELTA, *SIZE) and held.dtype == torch.uint8 and torch.equal(held[0], blended[0])
    # hold_cuts off is the unweighted call, and so is a window item that carries no weights
    assert torch.equal(blended, run(item)) and torch.equal(blended, next(iter(pred.predict_clip([dict(plain)], to_host=False))))
    assert torch.equal(held, next(iter(pred.predict_clip([dict(item)], to_host=False))))
    # the logits of a held frame are those of ONE key frame's chain: replacing the other key frame changes nothing
    garbage = torch.randn(item["frame_prev"].shape, generator=torch.Generator().manual_seed(9)).cuda() * 3
    from_prev = [f for f, s in enumerate(want_source) if s == 1]
    from_next = [f for f, s in enumerate(want_source) if s == 2]
    no_next = run(item, frame_next=garbage, weights=item["weights"])
    assert torch.equal(no_next[from_prev], held[from_prev])
    if from_next:
        no_prev = run(item, frame_prev=garbage, weights=item["weights"])
        assert torch.equal(no_prev[from_next], held[from_next])
    # ... at the level of the logits too
    kw = dict(mvs_left=item["mvs_left"], mvs_right=item["mvs_right"], n=DELTA, weights=item["weights"])
    ref = fm.predict(item["frame_prev"], item["frame_next"], **kw)["pred"]
    assert torch.equal(fm.predict(item["frame_prev"], garbage, **kw)["pred"][from_prev], ref[from_prev])
    # the op-by-op route has no weighted form: refused, not blended
    fm.fused_feature_tail = False
    try:
        with pytest.raises(NotImplementedError, match="segmentation tails"):
            fm.predict(item["frame_prev"], item["frame_next"], **kw)
        assert torch.equal(run(plain), blended)                          # without weights it is the same route as ever, bit for bit
    finally:
        fm.fused_feature_tail = True
