"""Frame-to-map registration on the GPU (ops.map_view, ops.map_gate, ops.pose_correct) against the numpy restatement of the
definition (tests/refine_ref.py), bit for bit: map_view on the dword and the byte route, from an RGB24 frame at the mask's size, an NV12
frame at twice the size (four taps) and an I420 frame at equal size (the identity resize), under five poses, with and without an age
gate; map_gate on winners inside, on the edge of, outside and nowhere near valid ground; pose_correct in every status; the whole
per-frame chain on a synthetic flight whose biased pose chain it must correct to the exact poses, eagerly and from one captured HIP
graph; and FlowPredictor(mosaic_refine=...) over two windows."""
import functools
import re

import numpy as np
import pytest
import torch

import mosaic_ref as mref
import ortho_ref as oref
import refine_ref as rref
from flood_uav_video_segmentation_amd import ops
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor
from test_gpu_regions import DELTA, FH, FW, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = mref.ONE


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


def dev_source(source):
    frame, chroma, fmt, matrix, full_range = source
    chroma = None if chroma is None else tuple(dev(c) for c in chroma) if isinstance(chroma, tuple) else dev(chroma)
    return dev(frame), chroma, fmt, matrix, full_range


def dev_canvas(planes):
    return dev(planes[0].view(np.int64)), dev(planes[1].view(np.int32))


@functools.lru_cache(maxsize=None)
def sampled(mask_size, kind):
    """(the decoded frame as numpy, the uint8 image the reference samples): RGB24 at the mask's size, NV12 at twice the size (four taps),
    I420 at the mask's size (the identity resize of a YUV frame)."""
    h, w = mask_size
    fmt, frame_size = {"rgb": ("rgb24", (h, w)), "nv12x2": ("nv12", (2 * h, 2 * w)), "i420": ("i420", (h, w))}[kind]
    source = oref.make_source(frame_size[0], frame_size[1], fmt, "bt709", False, seed=60 + h)
    img = oref.image(source, mask_size)
    img.setflags(write=False)
    return source, img


@functools.lru_cache(maxsize=None)
def canvas_of(mask_size):
    planes = rref.view_canvas(mask_size)
    for a in planes:
        a.setflags(write=False)
    return planes


# ------------------------------------------------------------------------------------------------ map_view
@pytest.mark.parametrize("min_age", [0, 3])
@pytest.mark.parametrize("kind", ["rgb", "nv12x2", "i420"])
@pytest.mark.parametrize("mask_size", [(48, 64), (50, 70)])
def test_view_equals_the_definition(mask_size, kind, min_age):
    """48 x 64: dword stores; 50 x 70: bytes, with a last group of two pixels and a remainder strip for the matcher.  Poses: the identity,
    a translation that pushes half the frame off the canvas, a rotation of 3 degrees with zoom 1.02, a lost row, and an ok row whose
    to_anchor breaks the pose bounds -- the last two must give all-invalid planes (and read no canvas pixel).  The canvas was written by
    four earlier frames; the frame's ordinal is 4, so min_age = 3 leaves only the ground of frames 0 and 1."""
    source, img = sampled(mask_size, kind)
    rank, rgba = canvas_of(mask_size)
    d_source, d_rank, d_rgba = dev_source(source), *dev_canvas((rank, rgba))
    seen = []
    for i, pose in enumerate(rref.view_poses(mask_size)):
        want = rref.map_view(img, pose, 4, rank, rgba, rref.VIEW_ORIGIN, min_age)
        got = ops.map_view(d_source, dev(pose), 4, mask_size, d_rank, d_rgba, rref.VIEW_ORIGIN, min_age)
        for name, g, w in zip(("cur", "view", "valid"), got, want):
            assert g.dtype == torch.uint8 and tuple(g.shape) == mask_size and np.array_equal(host(g), w), (i, name, int((host(g) != w).sum()))
        seen.append(int(want[2].sum()))                                       # from the reference, not from the op
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and seen[3:] == [0, 0]
    assert np.array_equal(host(d_rank), rank.view(np.int64)) and np.array_equal(host(d_rgba), rgba.view(np.int32))   # the canvas is only read


# ------------------------------------------------------------------------------------------------ map_gate
def test_gate_keeps_only_the_winners_on_fully_valid_ground():
    """A 3 x 4-block table: winners fully inside valid ground, on the plane's border, touching the ground's edge, one pixel over it, one
    pixel out of the plane, on invalid ground, void already, and two rows of garbage that a 32-bit window test would let through."""
    table, valid, survivors = rref.gate_case()
    want = rref.map_gate(table, valid)
    d_table = dev(table)
    got = ops.map_gate(d_table, dev(valid))
    assert got is d_table and np.array_equal(host(got), want)
    void = (want == np.array(rref.VOID_ROW)).all(1)
    assert np.flatnonzero(~void).tolist() == survivors
    rng = np.random.RandomState(9)                                            # and a random table on a plane with a few holes
    valid = (rng.rand(48, 64) < 0.999).astype(np.uint8)
    table = mref.grid_table(3, 4, lambda cx, cy: (rng.randint(-10, 11, size=cx.shape), rng.randint(-10, 11, size=cy.shape)))
    want = rref.map_gate(table, valid)
    assert 0 < (want == np.array(rref.VOID_ROW)).all(1).sum() < 12
    assert np.array_equal(host(ops.map_gate(dev(table), dev(valid))), want)


# ------------------------------------------------------------------------------------------------ pose_correct
@pytest.mark.parametrize("case", rref.step_cases(), ids=[c[0] for c in rref.step_cases()])
def test_correct_in_every_status(case):
    name, model, state, pose, status = case
    want_state, want_pose, want_out = rref.refine_step(model, state, pose, (64, 96), (128, 192), (32, 48))
    assert want_out[0] == status
    d_state, d_pose = dev(state), dev(pose)
    out = ops.pose_correct(dev(model), d_state, d_pose, (64, 96), (128, 192), (32, 48))
    assert np.array_equal(host(out), want_out) and np.array_equal(host(d_state), want_state) and np.array_equal(host(d_pose), want_pose)
    assert np.array_equal(host(d_state)[12:], state[12:])                    # last_fwd, last_inv, the phase, the counters: never written
    if status != rref.OK:
        assert np.array_equal(host(d_state), state) and np.array_equal(host(d_pose), pose)


# ------------------------------------------------------------------------------------------------ the chain
SIZE, CANVAS, ORIGIN = rref.FLIGHT_SIZE, rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN


def chain(frames, tables, state, rank, rgba):
    """The per-frame sequence FlowPredictor runs, on static device tensors: frames uint8 [6, 64, 96, 3], tables int32 [6, 24, 7].  The
    state and the canvas are reset by device ops first, so a replay starts from a fresh mosaic.  -> (poses [6, 16], outs [6, 8])."""
    state.zero_()
    rank.fill_(-1)
    rgba.zero_()
    poses, outs = [], []
    for f in range(frames.shape[0]):
        source = (frames[f], None, "rgb24", "bt601", False)
        pair = ops.global_motion(tables[f:f + 1], SIZE, SIZE, 4, 1.0, 6)
        pose = ops.pose_chain(pair, state, SIZE, CANVAS, ORIGIN)[0]
        cur, view, valid = ops.map_view(source, pose, f, SIZE, rank, rgba, ORIGIN, 0)
        table, stats = ops.block_match_modes(cur, view, search=8, penalty=0, intra_bias=65535, return_stats=True)
        ops.map_gate(table, valid)
        fit = ops.global_motion(table[None], SIZE, SIZE, 4, 1.0, 6, pair_stats=stats[None])
        outs.append(ops.pose_correct(fit, state, pose, SIZE, CANVAS, ORIGIN))
        ops.ortho_accumulate(source, pose, f, SIZE, rank, rgba, ORIGIN)
        poses.append(pose)
    return torch.stack(poses), torch.stack(outs)


def test_the_chain_corrects_a_biased_flight_exactly_eagerly_and_from_one_graph():
    """The CPU test's scene: six frames 4 px apart, pair tables that say one pixel too many.  The eager chain equals the reference and the
    exact true poses; the same chain captured in ONE graph on one stream and replayed on fresh inputs -- the same flight, then one cut
    from another part of the ground -- equals the eager run bit for bit, canvas and state included."""
    flights = [rref.straight_flight(), rref.straight_flight(row=7)]
    wants = [rref.run_flight(images, tables, CANVAS, ORIGIN, **rref.FLIGHT_SETTINGS) for images, tables, _ in flights]
    for f, (tx, ty) in enumerate(flights[0][2]):
        assert wants[0][0][f][:6].tolist() == [ONE, 0, tx * ONE, 0, ONE, ty * ONE]           # the reference itself gives the true poses
    assert not np.array_equal(wants[0][3][1], wants[1][3][1])                                # the second flight is another picture
    inputs = [(dev(np.stack(images)), dev(np.stack(tables))) for images, tables, _ in flights]
    frames, tables = inputs[0][0].clone(), inputs[0][1].clone()
    state = torch.zeros((32,), dtype=torch.int64, device=DEV)
    rank, rgba = ops.ortho_canvas(CANVAS, DEV)

    def same(poses, outs, want):
        return (np.array_equal(host(poses), want[0]) and np.array_equal(host(outs), want[1]) and np.array_equal(host(state), want[2])
                and np.array_equal(host(rank).view(np.uint64), want[3][0]) and np.array_equal(host(rgba).view(np.uint32), want[3][1]))

    eager = chain(frames, tables, state, rank, rgba)
    assert same(*eager, wants[0]), (host(eager[0])[:, [2, 5, 12]].tolist(), host(eager[1])[:, :3].tolist())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        poses, outs = chain(frames, tables, state, rank, rgba)
    for which in (0, 1):
        frames.copy_(inputs[which][0])
        tables.copy_(inputs[which][1])
        graph.replay()
        torch.cuda.synchronize()
        assert same(poses, outs, wants[which]), which


# ------------------------------------------------------------------------------------------------ FlowPredictor
def test_predictor_registers_every_frame_and_is_todays_without_it(clip):  # noqa: F811
    """Two windows of the synthetic network.  mosaic_refine=False: every report is bit-identical to a predictor built without the
    argument.  True: the masks are what they were; mosaic_report()'s poses are the reference's corrected rows, refine_report() its out
    rows, and the orthophoto is the one those rows gather."""
    size, canvas = (65, 65), (96, 120)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8, link_vectors=True, link_sources=True)
    items = [ds[0], ds[1]]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=True, cache_keyframes=False, mosaic=canvas, mosaic_min_inliers=6, mosaic_exclude=(1,), ortho="centre")

    def run(pred):
        return np.concatenate([host(pred.predict_window(i["frame_prev"], i["frame_next"], i["mvs_left"], i["mvs_right"], to_host=False, link_mvs=i["link_mvs"],
                                                        link_frame_size=i["link_frame_size"], link_stats=i.get("link_stats"), link_sources=i["link_sources"]))
                               for i in items])

    plain, off, on = FlowPredictor(fm, **kw), FlowPredictor(fm, mosaic_refine=False, **kw), FlowPredictor(fm, mosaic_refine=True, refine_search=8, **kw)
    masks = run(plain)
    assert np.array_equal(run(off), masks) and np.array_equal(run(on), masks) and torch.equal(on.hist, plain.hist)
    for a, b in zip(off.mosaic_report() + off.ortho_report(), plain.mosaic_report() + plain.ortho_report()):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="refine_report\\(\\) needs mosaic_refine=True"):
        off.refine_report()
    # the reference: the pair models of the windows' tables, then the loop
    tables = np.concatenate([host(i["link_mvs"]) for i in items])
    stats = None if items[0].get("link_stats") is None else np.concatenate([host(i["link_stats"]) for i in items])
    pairs = mref.global_motion(tables, (FH, FW), size, 4, ONE, 6, masks, 0b10, stats)
    images = [oref.image((host(s[0]), None) + tuple(s[2:]), size) for i in items for s in i["link_sources"]]
    origin = ((96 - 65) // 2, (120 - 65) // 2)
    poses, outs, _, planes = rref.run_flight(images, None, canvas, origin, masks=masks, pairs=pairs, exclude_set=0b10, search=8, rounds=4, tol=ONE, min_inliers=6)
    print("refine status per frame", outs[:, 0].tolist(), "shift Q20", outs[:, 4:6].tolist())
    assert np.array_equal(on.mosaic_report()[4], poses) and np.array_equal(on.refine_report(), outs) and outs.shape == (2 * DELTA, 8)
    want_src, want_covered = oref.winners(planes[0])
    image, src, covered = on.ortho_report(overlay=False)
    assert np.array_equal(src, want_src) and covered == want_covered and np.array_equal(image, oref.ortho_compose(planes[1]))
    votes = mref.mosaic_accumulate(masks, poses, np.zeros((5, 96, 120), np.uint16), origin)
    assert np.array_equal(on.mosaic_report()[0], mref.mosaic_resolve(votes)[0])               # the frames vote with the corrected rows
    on.clear_report()
    assert on.refine_report().shape == (0, 8) and on.mosaic_builder.frames == 0
    # every second frame, and a frame without a source: those rows say "not attempted"
    sources = list(items[0]["link_sources"])
    sources[2] = None
    every = FlowPredictor(fm, mosaic_refine=True, refine_every=2, **kw)
    i = items[0]
    every.predict_window(i["frame_prev"], i["frame_next"], i["mvs_left"], i["mvs_right"], to_host=False, link_mvs=i["link_mvs"], link_frame_size=i["link_frame_size"],
                         link_stats=i.get("link_stats"), link_sources=sources)
    want = rref.run_flight([None if s is None else img for s, img in zip(sources, images)], None, canvas, origin, masks=masks[:DELTA], pairs=pairs[:DELTA], every=2,
                           exclude_set=0b10, search=8, rounds=4, tol=ONE, min_inliers=6)
    assert np.array_equal(every.refine_report(), want[1]) and np.array_equal(every.mosaic_report()[4], want[0])
    assert [r[0] == 1 for r in want[1].tolist()] == [False, True, True, True, False]


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_raises_before_a_launch_and_names_the_value():
    """Device tensors of valid shapes with one bad value each: the library (or the Python check in front of it) refuses, nothing is
    launched, and the outputs a launch would have written are untouched."""
    mask_size = (48, 64)
    source, _ = sampled(mask_size, "rgb")
    rank, rgba = dev_canvas(canvas_of(mask_size))
    pose = dev(rref.view_poses(mask_size)[0])
    good = dict(source=dev_source(source), pose=pose, ordinal=4, mask_size=mask_size, rank=rank, rgba=rgba, origin=rref.VIEW_ORIGIN)
    for kw, word in ((dict(min_age=-1), "-1"), (dict(ordinal=0xFFFFFFFF), "4294967295"), (dict(mask_size=(15, 64)), "(15, 64)"), (dict(origin=(0, 16385)), "16385"),
                     (dict(pose=pose[:8]), "(8,)"), (dict(rank=rank[:, :5]), "(96, 5)")):
        with pytest.raises(ValueError, match=".*".join(("map_view", re.escape(word)))):
            ops.map_view(**{**good, **kw})
    table, valid, _ = rref.gate_case()
    d_table = dev(table)
    for kw, word in ((dict(valid=dev(valid)[:15]), "(15, 64)"), (dict(table=d_table[:11]), "(11, 7)"), (dict(valid=dev(valid).int()), "int32")):
        with pytest.raises(ValueError, match=".*".join(("map_gate", re.escape(word)))):
            ops.map_gate(**{**dict(table=d_table, valid=dev(valid)), **kw})
    assert np.array_equal(host(d_table), table)
    _, model, state, row, _ = rref.step_cases()[0]
    d_state, d_row = dev(state), dev(row)
    good = dict(model=dev(model), state=d_state, pose=d_row, mask_size=(64, 96), canvas_size=(128, 192), origin=(32, 48))
    for kw, word in ((dict(mask_size=(0, 96)), "(0, 96)"), (dict(canvas_size=(128, 16385)), "16385"), (dict(origin=(-16385, 0)), "-16385"), (dict(state=d_state[:31]), "(31,)")):
        with pytest.raises(ValueError, match=".*".join(("pose_correct", re.escape(word)))):
            ops.pose_correct(**{**good, **kw})
    assert np.array_equal(host(d_state), state) and np.array_equal(host(d_row), row)
