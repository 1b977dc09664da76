"""Relocalisation against the orthophoto on the GPU (ops.map_coarse, ops.map_patch, ops.map_locate, ops.pose_relocate, ops.relocate_commit;
DESIGN §3.22) against the numpy restatement of the definition (tests/relocate_ref.py), bit for bit: the coarse canvas with unseen holes
and a remainder strip; patches under shifted, rotated and refused states from RGB24 and NV12 frames; the search on canvases with holes,
with nothing seen and of one grey (every tie rule, the runner-up against `exclude`), on shapes with one and with several workgroups and
chunks; both steps in every status; the whole sequence on a synthetic flight with a scene cut, eagerly and from ONE captured HIP graph;
and FlowPredictor(mosaic_relocate=...) on that flight."""
import functools
import re

import numpy as np
import pytest
import torch

import mosaic_ref as mref
import ortho_ref as oref
import refine_ref as rref
import relocate_ref as lref
from flood_uav_video_segmentation_amd import ops
from flood_uav_video_segmentation_amd.flow.mosaic import MosaicBuilder

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = mref.ONE
# (canvas, origin (oy, ox), mask, S, the frame): 96 x 160 whole cells; 100 x 150 a remainder strip and a CW that is no multiple of 4 S;
# 36 x 44 at S = 4 a 9 x 11-cell patch (odd, two chunks of rows); 64 x 80 at S = 8; 40 x 400 placements in two workgroups side by side;
# 16 x 272 a patch of 68 cells a row (two chunks of columns)
SCENES = {"whole": ((96, 160), (20, 30), (32, 48), 4, "rgb"), "strip": ((100, 150), (20, 30), (36, 44), 4, "nv12x2"), "eight": ((100, 150), (8, 16), (64, 80), 8, "rgb"),
          "eight whole": ((96, 160), (8, 16), (64, 80), 8, "nv12x2"), "two tiles": ((40, 400), (8, 40), (16, 24), 4, "rgb"), "two chunks": ((40, 400), (8, 40), (16, 272), 4, "rgb")}


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


def dev_source(source):
    frame, chroma, fmt, matrix, full_range = source
    chroma = None if chroma is None else tuple(dev(c) for c in chroma) if isinstance(chroma, tuple) else dev(chroma)
    return dev(frame), chroma, fmt, matrix, full_range


@functools.lru_cache(maxsize=None)
def sampled(mask_size, kind):
    """(the decoded frame as numpy, the uint8 image the reference samples): RGB24 at the mask's size, NV12 at twice the size (four taps)."""
    h, w = mask_size
    fmt, frame_size = {"rgb": ("rgb24", (h, w)), "nv12x2": ("nv12", (2 * h, 2 * w))}[kind]
    source = oref.make_source(frame_size[0], frame_size[1], fmt, "bt709", False, seed=70 + h)
    img = oref.image(source, mask_size)
    img.setflags(write=False)
    return source, img


@functools.lru_cache(maxsize=None)
def canvas_of(name, kind="holes"):
    """The scene's rgba plane: random pixels with unseen holes, the frame planted 4 cells right and 1 down of the identity ("planted"),
    nothing seen ("empty"), or one grey with an unseen corner ("grey")."""
    canvas, origin, mask, s, frame = SCENES[name]
    if kind == "empty":
        return oref.canvas(canvas)[1]
    if kind == "grey":
        return lref.constant_canvas(canvas, hole=(0, 2 * s, 0, 2 * s))[1]
    rng = np.random.RandomState(len(name))
    rgba = rng.randint(0, 1 << 24, size=canvas).astype(np.uint32) | np.uint32(0xFF000000)
    rgba[3:11, canvas[1] // 2:canvas[1] // 2 + 9] = 0
    rgba[canvas[0] - 9:, :13] &= np.uint32(0x00FFFFFF)
    if kind == "planted":
        rank = np.full(canvas, oref.EMPTY, np.uint64)
        oref.ortho_accumulate(sampled(mask, frame)[1], mref.pose_rows([mref.affine_pose(1, 0, 0, 1, 4 * s, s)])[0], 1, rank, rgba, origin, "latest")
    rgba.setflags(write=False)
    return rgba


def check_patch(got, want):
    (tl, tv, geom), (wl, wv, wgeom) = got, want
    assert tl.dtype == tv.dtype == torch.uint8 and tuple(tl.shape) == tuple(tv.shape) == (65536,) and np.array_equal(host(geom), wgeom), (host(geom), wgeom)
    cells = wl.size
    assert np.array_equal(host(tl)[:cells], wl.reshape(-1)) and np.array_equal(host(tv)[:cells], wv.reshape(-1))


# ------------------------------------------------------------------------------------------------ map_coarse
@pytest.mark.parametrize("s", [4, 8, 16])
@pytest.mark.parametrize("name", ["whole", "strip"])
def test_coarse_equals_the_definition(name, s):
    for kind in ("holes", "empty"):
        rgba = canvas_of(name, kind)
        wl, wv = lref.map_coarse(rgba, s)
        cl, cv = ops.map_coarse(dev(rgba.view(np.int32)), s)
        assert cl.dtype == cv.dtype == torch.uint8 and tuple(cl.shape) == tuple(cv.shape) == (rgba.shape[0] // s, rgba.shape[1] // s)
        assert np.array_equal(host(cl), wl) and np.array_equal(host(cv), wv), kind
        assert (0 < wv.sum() < wv.size) if kind == "holes" else wv.sum() == 0


# ------------------------------------------------------------------------------------------------ map_patch
@pytest.mark.parametrize("name", list(SCENES))
def test_patch_equals_the_definition(name):
    """Eight states: the identity; a shift off the cell grid; a rotation with zoom (the bounding box is larger than the frame and its
    corner cells are invalid); a patch partly off the canvas; and the four refusals, which write geom and nothing else."""
    canvas, origin, mask, s, frame = SCENES[name]
    source, img = sampled(mask, frame)
    d_source = dev_source(source)
    status = []
    for label, state in lref.patch_states(mask):
        want = lref.map_patch(img, state, canvas, origin, s)
        d_state = dev(state)
        check_patch(ops.map_patch(d_source, d_state, mask, canvas, origin, s), want)
        assert np.array_equal(host(d_state), state), label                    # only read
        status.append(int(want[2][0]))
    assert status[:3] == [0, 0, 0] and status[4:6] == [1, 2] and status[7] == 3
    rotated = lref.map_patch(img, lref.patch_states(mask)[2][1], canvas, origin, s)
    assert rotated[1][0, 0] == 0 and rotated[1][-1, -1] == 0 and 0 < rotated[2][5] < rotated[1].size


def shape_states(s):
    """(label, state, cells, valid cells) for a 32 x 48 frame on a canvas with its anchor at (30, 20): the frame shrunk onto exactly one
    cell; the frame on whole cells at canvas (32, 32) under a from_anchor sheared by 1/62, so that of all its pixels only the source of
    the bottom left one falls outside the frame (x = 0.5 - 31.5 / 62 < 0) and one cell is invalid; and the frame one pixel off the cell
    grid, its rim of cells invalid.  3 x 2 = 6 cells at S = 16 and 13 x 9 = 117 at S = 4: no multiple of the four a workgroup takes."""
    k = 16913                                                                 # ONE / 62 in Q20
    sheared = [ONE, -k, -2 * ONE + 12 * k, 0, ONE, -12 * ONE]                 # the inverse of the shift by (2, 12), and - y / 62 in x
    return [("one cell", lref.lost_state(*mref.affine_pose(s / 48, 0, 0, s / 32, 2, 12)), 1, 1),
            ("one pixel outside", lref.lost_state(mref.affine_pose(1, 0, 0, 1, 2, 12)[0], sheared), (48 // s) * (32 // s), (48 // s) * (32 // s) - 1),
            ("off the grid", lref.lost_state(*mref.affine_pose(1, 0, 0, 1, 3, 13)), (48 // s + 1) * (32 // s + 1), (48 // s - 1) * (32 // s - 1))]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("fmt", ["rgb24", "nv12"])
def test_the_patch_kernel_in_every_shape_and_source(fmt, mode):
    """The one cells kernel behind map_patch on every frame source it is instantiated for -- RGB24 and NV12, each resized in both
    directions (0), in height only (1) and not at all (2) -- at S = 4 (16 of a wave's 64 lanes hold a pixel) and S = 16 (four pixels a
    lane), on shape_states' patches."""
    mask, canvas, origin = (32, 48), (96, 160), (20, 30)
    source = oref.make_source(*{0: (64, 96), 1: (64, 48), 2: (32, 48)}[mode], fmt, "bt709", False, seed=90 + mode)
    img, d_source = oref.image(source, mask), dev_source(source)
    for s in (4, 16):
        for label, state, cells, valid in shape_states(s):
            want = lref.map_patch(img, state, canvas, origin, s)
            assert want[2][0] == 0 and want[2][3] * want[2][4] == cells and want[2][5] == valid, (s, label, want[2])      # the reference first
            check_patch(ops.map_patch(d_source, dev(state), mask, canvas, origin, s), want)
    X, Y = np.meshgrid(np.arange(32, 80), np.arange(32, 64))                   # "one pixel outside" means one
    x, y = lref._source(shape_states(4)[1][1][6:12].tolist(), X, Y, origin[1], origin[0])
    assert ((x < 0) | (x >= 48) | (y < 0) | (y >= 32)).sum() == 1 and x[31, 0] == -1


# ------------------------------------------------------------------------------------------------ map_locate
@pytest.mark.parametrize("name", list(SCENES))
def test_locate_equals_the_definition(name):
    canvas, origin, mask, s, frame = SCENES[name]
    source, img = sampled(mask, frame)
    d_source = dev_source(source)
    for kind in ("holes", "planted", "empty"):
        rgba = canvas_of(name, kind)
        cl, cv = lref.map_coarse(rgba, s)
        d_cl, d_cv = ops.map_coarse(dev(rgba.view(np.int32)), s)
        for label, state in lref.patch_states(mask)[:5]:
            tl, tv, geom = lref.map_patch(img, state, canvas, origin, s)
            d_patch = ops.map_patch(d_source, dev(state), mask, canvas, origin, s)
            for permille, exclude in ((500, 2), (1000, 0)) if kind != "empty" else ((1, 2),):
                want = lref.map_locate(cl, cv, tl, tv, geom, permille, exclude)
                got = ops.map_locate(d_cl, d_cv, *d_patch, permille, exclude)
                assert np.array_equal(host(got), want), (kind, label, permille, host(got).tolist(), want.tolist())
                assert want[0] == (lref.FOUND_BAD_GEOM if geom[0] != 0 else lref.FOUND_NONE if kind == "empty" or want[11] == 0 else lref.FOUND)
            if kind == "planted" and label == "identity":
                assert want[:5].tolist() == [0, 4, 1, 0, geom[5]]                    # planted (4 S, S) px away: four cells right, one down, every cell equal
    # a geom row of garbage is refused on the device
    bad = host(d_patch[2]).copy()
    bad[0], bad[3] = 0, 1 << 40
    assert host(ops.map_locate(d_cl, d_cv, d_patch[0], d_patch[1], dev(bad)))[0] == lref.FOUND_BAD_GEOM


@pytest.mark.parametrize("name", ["whole", "strip", "two tiles"])
def test_a_canvas_of_one_grey_ties_everywhere(name):
    """Every placement has mean 0: the larger n (clear of the unseen corner), then the smaller v, then the smaller u wins; the runner-up
    is the first such placement outside the exclusion square, and with exclude = 64 on these canvases there may be none."""
    canvas, origin, mask, s, frame = SCENES[name]
    rgba = canvas_of(name, "grey")
    img = np.full(mask + (3,), 90, np.uint8)
    source = (img, None, "rgb24", "bt601", False)
    cl, cv = lref.map_coarse(rgba, s)
    d_cl, d_cv = ops.map_coarse(dev(rgba.view(np.int32)), s)
    state = lref.patch_states(mask)[0][1]
    tl, tv, geom = lref.map_patch(img, state, canvas, origin, s)
    d_patch = ops.map_patch(dev_source(source), dev(state), mask, canvas, origin, s)
    check_patch(d_patch, (tl, tv, geom))
    runner = []
    for exclude in (0, 2, 64):
        want = lref.map_locate(cl, cv, tl, tv, geom, 500, exclude)
        assert np.array_equal(host(ops.map_locate(d_cl, d_cv, *d_patch, 500, exclude)), want), exclude
        assert want[0] == lref.FOUND and want[3] == 0 and want[4] == geom[5]
        runner.append(want[5:8].tolist())
    assert runner[0][0] == runner[1][0] == 1 and runner[0] != runner[1]


# ------------------------------------------------------------------------------------------------ pose_relocate, relocate_commit
@pytest.mark.parametrize("case", lref.step_cases(), ids=[c[0] for c in lref.step_cases()])
def test_relocate_in_every_status(case):
    name, found, state, max_mean, ratio, decision = case
    for s in (4, 16):
        want_state, want_pose = lref.relocate_step(found, state, s=s, max_mean=max_mean, ratio=ratio, **lref.STEP_GEOMETRY)
        assert want_state[28] == decision
        d_state = dev(state)
        cs, cp = ops.pose_relocate(dev(found), d_state, scale=s, max_mean=max_mean, ratio_permille=ratio, **lref.STEP_GEOMETRY)
        assert np.array_equal(host(cs), want_state) and np.array_equal(host(cp), want_pose) and np.array_equal(host(d_state), state)


@pytest.mark.parametrize("case", lref.commit_cases(), ids=[c[0] for c in lref.commit_cases()])
def test_commit_in_every_status(case):
    name, cs, cp, co, state, pose, found, status = case
    want_state, want_pose, want_out = lref.commit_step(cs, cp, co, state, pose, found, 4)
    assert want_out[0] == status
    d_state, d_pose, d_cs, d_cp = dev(state), dev(pose), dev(cs), dev(cp)
    out = ops.relocate_commit(d_cs, d_cp, dev(co), d_state, d_pose, dev(found), 4)
    assert np.array_equal(host(out), want_out) and np.array_equal(host(d_state), want_state) and np.array_equal(host(d_pose), want_pose)
    assert np.array_equal(host(d_cs), cs) and np.array_equal(host(d_cp), cp)
    if status != lref.RELOCATED:
        assert np.array_equal(host(d_state), state) and np.array_equal(host(d_pose), pose)     # the chain stays lost exactly as it was


# ------------------------------------------------------------------------------------------------ the flight
SIZE, CANVAS, ORIGIN = rref.FLIGHT_SIZE, rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN


def register(source, pose, state, f, rank, rgba):
    """refine_ref.refine_frame's sequence with the flight's settings, on the device."""
    cur, view, valid = ops.map_view(source, pose, f, SIZE, rank, rgba, ORIGIN, 0)
    table, stats = ops.block_match_modes(cur, view, search=8, penalty=0, intra_bias=65535, return_stats=True)
    ops.map_gate(table, valid)
    fit = ops.global_motion(table[None], SIZE, SIZE, 4, 1.0, 6, pair_stats=stats[None])
    return ops.pose_correct(fit, state, pose, SIZE, CANVAS, ORIGIN)


def chain(frames, pairs, state, rank, rgba, s=4):
    """The per-frame sequence FlowPredictor(mosaic_relocate=True) runs, on static device tensors.  The state and the canvas are reset by
    device ops first, so a replay starts from a fresh mosaic.  -> (poses [n, 16], refine outs [n, 8], relocate outs [n, 8])."""
    state.zero_()
    rank.fill_(-1)
    rgba.zero_()
    poses, outs, relocs = [], [], []
    for f in range(frames.shape[0]):
        source = (frames[f], None, "rgb24", "bt601", False)
        pose = ops.pose_chain(pairs[f:f + 1], state, SIZE, CANVAS, ORIGIN)[0]
        outs.append(register(source, pose, state, f, rank, rgba))
        cl, cv = ops.map_coarse(rgba, s)
        tl, tv, geom = ops.map_patch(source, state, SIZE, CANVAS, ORIGIN, s)
        found = ops.map_locate(cl, cv, tl, tv, geom, 500, 2)
        cand_state, cand_pose = ops.pose_relocate(found, state, SIZE, CANVAS, ORIGIN, s, 16, 800)
        correct_out = register(source, cand_pose, cand_state, f, rank, rgba)
        relocs.append(ops.relocate_commit(cand_state, cand_pose, correct_out, state, pose, found, s))
        ops.ortho_accumulate(source, pose, f, SIZE, rank, rgba, ORIGIN)
        poses.append(pose)
    return torch.stack(poses), torch.stack(outs), torch.stack(relocs)


@functools.lru_cache(maxsize=None)
def flights():
    """[(images, pairs, true)] and the reference's runs: the cut onto mapped ground, cut to 14 frames, and the cut onto unmapped ground with a
    14th frame, so that both fill the same static tensors."""
    a, b = lref.revisit_after_cut(), lref.unmapped_after_cut()
    b = (b[0] + [b[0][-1]], np.concatenate([b[1], b[1][-1:]]), b[2] + [b[2][-1]])
    wants = [lref.run_flight(f[0], f[1], CANVAS, ORIGIN, relocate=True, s=4, **rref.FLIGHT_SETTINGS) for f in (a, b)]
    return (a, b), wants


def test_the_sequence_recovers_the_cut_flight_eagerly_and_from_one_graph():
    """The CPU test's scenes.  The eager sequence equals the reference, which brings every frame after the cut back to its exact pose;
    the same sequence captured in ONE graph on one stream and replayed on fresh inputs -- that flight, then the one that jumps to
    unmapped ground and must stay lost -- equals the reference bit for bit, canvas and state included."""
    (a, b), wants = flights()
    for f, (tx, ty) in enumerate(a[2]):
        assert wants[0][0][f][:6].tolist() == [ONE, 0, tx * ONE, 0, ONE, ty * ONE] and wants[0][0][f][12] == 0     # the reference itself gives the true poses
    assert wants[0][2][:, 0].tolist() == [1] * lref.CUT_AT + [0, 1, 1, 1] and wants[1][0][lref.CUT_AT:, 12].tolist() == [2] * 4
    inputs = [(dev(np.stack(f[0])), dev(f[1])) for f in (a, b)]
    frames, pairs = inputs[0][0].clone(), inputs[0][1].clone()
    state = torch.zeros((32,), dtype=torch.int64, device=DEV)
    rank, rgba = ops.ortho_canvas(CANVAS, DEV)

    def same(got, want):
        return (np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1]) and np.array_equal(host(got[2]), want[2])
                and np.array_equal(host(state), want[3]) and np.array_equal(host(rank).view(np.uint64), want[4][0])
                and np.array_equal(host(rgba).view(np.uint32), want[4][1]))

    eager = chain(frames, pairs, state, rank, rgba)
    assert same(eager, wants[0]), (host(eager[0])[:, [2, 5, 12]].tolist(), host(eager[2]).tolist())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = chain(frames, pairs, state, rank, rgba)
    for which in (0, 1):
        frames.copy_(inputs[which][0])
        pairs.copy_(inputs[which][1])
        graph.replay()
        torch.cuda.synchronize()
        assert same(got, wants[which]), (which, host(got[2]).tolist())


# ------------------------------------------------------------------------------------------------ FlowPredictor
def test_predictor_relocalises_the_cut_flight_and_is_todays_without_it():
    """The flight handed to FlowPredictor's mosaic step, a MosaicBuilder without a predictor, in two windows of seven frames (synthesised
    tables and a stats row that flags the cut, as an estimate-mode dataset hands them out; the masks are all one class, which votes).  mosaic_relocate=True: mosaic_report()'s
    poses and relocate_report() are the reference's, the orthophoto the one those rows gather.  False: every report equals a predictor's
    built without the argument, and every frame after the cut is lost."""
    (a, _), wants = flights()
    images, _, _ = a
    offsets = [rref.FLIGHT_STEP * f for f in range(lref.CUT_AT)] + [rref.FLIGHT_STEP * f for f in range(4)]
    tables = dev(np.stack(rref.flight(offsets, bias=(0, 0))[1]))
    stats = torch.zeros((len(images), 4), dtype=torch.int32, device=DEV)
    stats[lref.CUT_AT, 2] = 1
    frames = dev(np.stack(images))
    masks = torch.zeros((len(images),) + SIZE, dtype=torch.uint8, device=DEV)
    kw = dict(classes=5, min_inliers=6, exclude=(), origin=ORIGIN, ortho="centre", refine=True, refine_search=8)

    def run(pred):
        for lo in (0, 7):
            sources = [(frames[f], None, "rgb24", "bt601", False) for f in range(lo, lo + 7)]
            pred.add(masks[lo:lo + 7], (tables[lo:lo + 7], SIZE, stats[lo:lo + 7], None), sources)
        return pred

    plain, off = run(MosaicBuilder(CANVAS, **kw)), run(MosaicBuilder(CANVAS, relocate=False, **kw))
    on = run(MosaicBuilder(CANVAS, relocate=True, relocate_scale=4, **kw))
    for x, y in zip(off.report() + off.ortho_report() + (off.refine_report(),), plain.report() + plain.ortho_report() + (plain.refine_report(),)):
        assert np.array_equal(x, y)
    assert off.report()[4][:, 12].tolist() == [0] * lref.CUT_AT + [2] * 4
    with pytest.raises(ValueError, match="relocate_report\\(\\) needs mosaic_relocate=True"):
        off.relocate_report()
    poses, outs, relocs, _, planes = wants[0]
    assert np.array_equal(on.report()[4], poses) and np.array_equal(on.relocate_report(), relocs) and np.array_equal(on.refine_report(), outs)
    want_src, want_covered = oref.winners(planes[0])
    image, src, covered = on.ortho_report(overlay=False)
    assert np.array_equal(src, want_src) and covered == want_covered and np.array_equal(image, oref.ortho_compose(planes[1]))
    votes = mref.mosaic_accumulate(host(masks), poses, np.zeros((5,) + CANVAS, np.uint16), ORIGIN)
    assert np.array_equal(on.report()[0], mref.mosaic_resolve(votes)[0])
    on.clear()
    assert on.relocate_report().shape == (0, 8)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_raises_before_a_launch_and_names_the_value():
    """Device tensors of valid shapes with one bad value each: the Python check (which mirrors the library's) refuses, nothing is
    launched, and the tensors a launch would have written are untouched."""
    canvas, origin, mask, s, frame = SCENES["whole"]
    rgba = dev(canvas_of("whole").view(np.int32))
    for kw, word in ((dict(scale=5), "5"), (dict(rgba=rgba[:3], scale=4), "no cell"), (dict(rgba=rgba.long()), "int64")):
        with pytest.raises(ValueError, match=".*".join(("map_coarse", re.escape(word)))):
            ops.map_coarse(**{**dict(rgba=rgba, scale=4), **kw})
    state = dev(lref.patch_states(mask)[0][1])
    good = dict(source=dev_source(sampled(mask, "rgb")[0]), state=state, mask_size=mask, canvas_size=canvas, origin=origin, scale=s)
    for kw, word in ((dict(scale=32), "32"), (dict(state=state[:31]), "(31,)"), (dict(mask_size=(0, 48)), "(0, 48)"), (dict(canvas_size=(96, 16385)), "16385"),
                     (dict(canvas_size=(96, 7), scale=8), "no cell"), (dict(origin=(0, 16385)), "16385")):
        with pytest.raises(ValueError, match=".*".join(("map_patch", re.escape(word)))):
            ops.map_patch(**{**good, **kw})
    cl, cv = ops.map_coarse(rgba, s)
    tl, tv, geom = ops.map_patch(**good)
    for kw, word in ((dict(min_overlap_permille=0), "got 0"), (dict(min_overlap_permille=1001), "1001"), (dict(exclude=65), "65"), (dict(exclude=-1), "-1"),
                     (dict(cv=cv[:5]), "(5, 40)"), (dict(tl=tl[:9]), "(9,)"), (dict(geom=geom[:7]), "(7,)")):
        with pytest.raises(ValueError, match=".*".join(("map_locate", re.escape(word)))):
            ops.map_locate(**{**dict(cl=cl, cv=cv, tl=tl, tv=tv, geom=geom), **kw})
    found = ops.map_locate(cl, cv, tl, tv, geom)
    good = dict(found=found, state=state, mask_size=mask, canvas_size=canvas, origin=origin, scale=s)
    for kw, word in ((dict(max_mean=256), "256"), (dict(max_mean=-1), "-1"), (dict(ratio_permille=0), "got 0"), (dict(ratio_permille=1001), "1001"), (dict(scale=2), "2"),
                     (dict(found=found[:15]), "(15,)")):
        with pytest.raises(ValueError, match=".*".join(("pose_relocate", re.escape(word)))):
            ops.pose_relocate(**{**good, **kw})
    cs, cp = ops.pose_relocate(**good)
    before = host(state).copy()
    pose = torch.zeros((16,), dtype=torch.int64, device=DEV)
    good = dict(cand_state=cs, cand_pose=cp, correct_out=torch.zeros((8,), dtype=torch.int64, device=DEV), state=state, pose=pose, found=found, scale=s)
    for kw, word in ((dict(scale=3), "3"), (dict(cand_state=cs[:31]), "(31,)"), (dict(pose=pose[:8]), "(8,)"), (dict(correct_out=pose), "(16,)")):
        with pytest.raises(ValueError, match=".*".join(("relocate_commit", re.escape(word)))):
            ops.relocate_commit(**{**good, **kw})
    assert np.array_equal(host(state), before) and not host(pose).any()
