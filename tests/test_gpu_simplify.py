"""Outline simplification on the GPU: ops.outline_simplify (csrc/simplify_ops.hip through the fifth hook table) on outlines made on the
device by ops.mask_regions, region_table and region_outlines, against the recursive definition in numpy (tests/simplify_ref.py) by
integer equality at both connectivities, and one window end to end through FlowPredictor(regions=True, outlines=True, simplify=1.0)."""
import functools
import json

import numpy as np
import pytest
import torch

import motion_modes_ref as modes_ref
import simplify_ref as sref
from flood_uav_video_segmentation_amd import _lib, ops, synth
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor, write_outlines_geojson

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
KEYS = ("simple", "simple_vertices", "simple_counts")
SENTINEL = {torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B}
PAIRS = ((0, 32), (4, 32), (16, 8), (16, 32), (64, 256))      # (tol_q, round cap)
TOLERANCE = {0: 0.0, 4: 0.5, 16: 1.0, 64: 2.0}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                            # a copy: the shared expectations are read-only


def sentinel_out(n, max_contours, max_vertices):
    """The three outputs pre-filled with a sentinel: whatever the call leaves of it shows in the comparison."""
    shapes = ((n, max_contours, 4), (n, max_vertices, 2), (n, 4))
    dtypes = (torch.int64, torch.int32, torch.int64)
    return tuple(torch.full(s, SENTINEL[d], dtype=d, device=DEV) for s, d in zip(shapes, dtypes))


@functools.lru_cache(maxsize=None)
def device_outlines(name, conn, max_contours=sref.MAX_CONTOURS, max_vertices=sref.MAX_VERTICES):
    """A case's outlines, made on the device from its mask; they are the reference's (tests/test_gpu_outlines.py checks that op)."""
    _, mask, k, cap = sref.CASES[name]
    mask = dev(mask)
    index = ops.region_table(mask, ops.mask_regions(mask, k, conn), k, None, 128, cap)[2]
    contours, vertices, _, counts = ops.region_outlines(index, cap, conn, max_contours, max_vertices)
    e = sref.outlines_of(name, conn, max_contours, max_vertices)
    assert torch.equal(contours, dev(e["contours"])) and torch.equal(vertices, dev(e["vertices"])) and torch.equal(counts, dev(e["counts"]))
    return contours, vertices, counts


def check_case(name, conn, tol_q, cap, max_contours=sref.MAX_CONTOURS, max_vertices=sref.MAX_VERTICES):
    contours, vertices, counts = device_outlines(name, conn, max_contours, max_vertices)
    want = sref.expected(name, conn, tol_q, cap, max_contours, max_vertices)
    got = ops.outline_simplify(contours, vertices, counts, TOLERANCE[tol_q], cap, out=sentinel_out(len(counts), max_contours, max_vertices))
    for g, w, key in zip(got, want, KEYS):
        assert g.dtype == (torch.int32 if key == "simple_vertices" else torch.int64) and torch.equal(g, dev(w)), (name, conn, tol_q, cap, key)
    return want


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["1x1", "1x7", "5x1", "pixel", "ring", "diagonal", "diagonal_hole", "lake", "40x300", "checker", "33x67", "n3", "capped",
                                  "blob", "serpentine", "comb"])
def test_every_shape_equals_the_definition(name, conn):
    flagged = {}
    for tol_q, cap in PAIRS:
        simple, _, counts = check_case(name, conn, tol_q, cap)
        flagged[tol_q, cap] = bool((counts[:, 3] & 1).any())
        assert not (counts[:, 3] & ~1).any() and (simple[..., 1][simple[..., 1] > 0] >= 3).all()
    if name in ("serpentine", "comb"):                                       # the cap bites; at 256 rounds they converge
        assert flagged[16, 8] and flagged[16, 32]
        _, _, counts = check_case(name, conn, 16, 256)
        assert not counts[:, 3].any() and counts[0, 2] > 32
    else:
        assert not flagged[16, 32] and not flagged[64, 256]
    if name == "n3":
        assert len({tuple(c) for c in sref.expected(name, conn, 16, 32)[2].tolist()}) == 3
    if name == "33x67":                                                      # contours across the borders of the 256- and 1024-vertex workgroups
        assert sref.outlines_of(name, conn)["counts"][0, 2] > 2048


def test_a_batch_with_an_overflowed_and_a_truncated_frame():
    name, conn = "n3", 8
    e = sref.outlines_of(name, conn)
    total = int(np.sort(e["counts"][:, 2])[1])                               # one frame of three has more vertices: it overflows
    want = check_case(name, conn, 16, 32, sref.MAX_CONTOURS, total)
    assert sorted(want[2][:, 3].tolist()) == [0, 0, 2]
    rows = int(np.sort(e["counts"][:, 0])[1])                                # one frame of three has more contours: its rows are cut
    want = check_case(name, conn, 16, 32, rows, sref.MAX_VERTICES)
    assert sorted(want[2][:, 3].tolist()) == [0, 0, 4] and want[2][:, 0].max() == rows


def test_frames_that_break_a_rule_get_nothing_and_their_flag():
    """One batch of all the broken frames of the CPU test plus a sound one in the middle: garbage rows steer nothing."""
    frames = sref.broken_frames()
    sound = tuple(np.array(sref.outlines_of("lake", 8, 8, 64)[key]) for key in ("contours", "vertices", "counts"))
    batch = [f[1:4] for f in frames[:6]] + [sound] + [f[1:4] for f in frames[6:]]
    contours, vertices, counts = (np.concatenate([b[k] for b in batch]) for k in range(3))
    want = sref.outline_simplify(contours, vertices, counts, 16, 32)
    assert want[2][:, 3].tolist() == [f[4] for f in frames[:6]] + [0] + [f[4] for f in frames[6:]] and want[2][6, 1] == 24
    got = ops.outline_simplify(dev(contours), dev(vertices), dev(counts), 1.0, 32, out=sentinel_out(len(batch), 8, 64))
    assert all(torch.equal(g, dev(w)) for g, w in zip(got, want))
    c, v, n = (np.array(a) for a in sound)                                   # coordinates out of range are read clamped
    v[0, :24:5] = [[-7, 3], [1 << 20, 2], [5, -(1 << 31)], [(1 << 31) - 1, (1 << 31) - 1], [0, 1 << 15]]
    want = sref.outline_simplify(c, v, n, 16, 32)
    got = ops.outline_simplify(dev(c), dev(v), dev(n), 1.0, 32, out=sentinel_out(1, 8, 64))
    assert all(torch.equal(g, dev(w)) for g, w in zip(got, want)) and want[1].max() == 16384 and want[1].min() == 0


def raw_call(lib, ins, n, mc, mv, tol_q, cap, outs, work):
    check(lib.fs_outline_simplify(*(ptr(t) for t in ins), n, mc, mv, tol_q, cap, *(ptr(o) for o in outs), ptr(work), stream_ptr()))


def test_a_workspace_full_of_garbage_changes_nothing_and_two_runs_are_bit_identical():
    lib = _lib.load()
    for name, conn, tol_q, cap in (("33x67", 8, 16, 8), ("n3", 4, 4, 32), ("serpentine", 8, 16, 32)):
        ins = device_outlines(name, conn)
        n, mc, mv = len(ins[2]), sref.MAX_CONTOURS, sref.MAX_VERTICES
        want = sref.expected(name, conn, tol_q, cap)
        words = ops.outline_simplify_workspace_bytes(n, mc, mv) // 8
        runs = []
        for fill in (SENTINEL[torch.int64], -1, 0x7FFFFFFF7FFFFFFF):
            outs = sentinel_out(n, mc, mv)
            raw_call(lib, ins, n, mc, mv, tol_q, cap, outs, torch.full((words,), fill, dtype=torch.int64, device=DEV))
            assert all(torch.equal(g, dev(w)) for g, w in zip(outs, want)), (name, fill)
            runs.append(outs)
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))      # the atomics do not show


def test_a_captured_graph_replayed_on_new_planes_gives_those_planes_result():
    conn, mc, mv, tol_q, cap = 8, 512, 4096, 16, 8
    lib = _lib.load()
    a_in, b_in = device_outlines("33x67", conn, mc, mv), device_outlines("blob", conn, mc, mv)
    a, b = sref.expected("33x67", conn, tol_q, cap, mc, mv), sref.expected("blob", conn, tol_q, cap, mc, mv)
    ins = tuple(t.clone() for t in a_in)
    outs = sentinel_out(1, mc, mv)                                            # never cleared by the caller
    work = torch.empty((ops.outline_simplify_workspace_bytes(1, mc, mv) // 8,), dtype=torch.int64, device=DEV)
    raw_call(lib, ins, 1, mc, mv, tol_q, cap, outs, work)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_call(lib, ins, 1, mc, mv, tol_q, cap, outs, work)
    for src, want in ((b_in, b), (a_in, a), (b_in, b)):
        for dst, t in zip(ins, src):
            dst.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(g, dev(w)) for g, w in zip(outs, want))
    assert a[2][0, 2:].tolist() == [8, 1] and b[2][0, 1:].tolist() == [51, 7, 0]


def test_refusals_launch_nothing():
    """Every refusal of the header, with real device buffers: the call fails with its message and no output changes."""
    lib = _lib.load()
    n, mc, mv = 1, 16, 64
    ins = (torch.zeros((n, mc, 6), dtype=torch.int64, device=DEV), torch.zeros((n, mv, 2), dtype=torch.int32, device=DEV),
           torch.zeros((n, 4), dtype=torch.int64, device=DEV))
    outs = sentinel_out(n, mc, mv)
    work = torch.full((ops.outline_simplify_workspace_bytes(n, mc, mv) // 8,), SENTINEL[torch.int64], dtype=torch.int64, device=DEV)
    real = dict(contours=ins[0].data_ptr(), vertices=ins[1].data_ptr(), counts=ins[2].data_ptr(), workspace=work.data_ptr(),
                **{key: o.data_ptr() for key, o in zip(KEYS, outs)})
    for kw, word in sref.refusal_cases():
        args = dict(real)
        args.update({key: (work.data_ptr() + 4 if key == "workspace" and value else value) for key, value in kw.items()})
        assert sref.call_simplify(lib, **args) != 0, kw
        msg = lib.fs_last_error()
        assert word.encode() in msg and b"outline_simplify" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL[o.dtype]).all()) for o in outs + (work,))
    for bad in (lambda: ops.outline_simplify(ins[0].int(), ins[1], ins[2], 1.0), lambda: ops.outline_simplify(ins[0], ins[1].long(), ins[2], 1.0),
                lambda: ops.outline_simplify(ins[0], ins[1], ins[2][:, :3], 1.0), lambda: ops.outline_simplify(ins[0], ins[1][:, :3], ins[2], 1.0),
                lambda: ops.outline_simplify(*ins, 1.0, out=outs[:2]), lambda: ops.outline_simplify(*ins, 1.0, out=(outs[0], outs[1][:, :8], outs[2]))):
        with pytest.raises(RuntimeError):
            bad()
    assert [tuple(t.shape) for t in ops.outline_simplify(ins[0][:0], ins[1][:0], ins[2][:0], 1.0)] == [(0, mc, 4), (0, mv, 2), (0, 4)]
    empty = ops.outline_simplify(*ins, 1.0)                                   # a frame without a contour
    assert not any(bool(t.any()) for t in empty)


# ------------------------------------------------------------------------------------------------ end to end
FH, FW, FRAMES, DELTA = 1072, 1920, 11, 5   # the grid estimator is built for 1072 / 1080 x 1920 frames; the network sees 65 x 65


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    frames = modes_ref.textured_frame(FH + 8 * FRAMES, FW, seed=51, channels=3)
    path = str(tmp_path_factory.mktemp("simplify") / "clip.rgb")
    with open(path, "wb") as fh:
        for i in range(FRAMES):
            fh.write(np.ascontiguousarray(frames[8 * i:8 * i + FH]).tobytes())
    return path


@functools.lru_cache(maxsize=None)
def network():
    from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

    class HP:
        layers, classes, pretrained = 50, 5, False

    net = FlowPSPNet(HP()).eval()
    net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
    return net


def test_predictor_with_simplified_outlines(clip, tmp_path):
    size, conn, cap, mc, mv = (65, 65), 8, 1024, 2048, 16384
    item = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8)[1]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=True, cache_keyframes=False, regions=True, connectivity=conn, max_regions=cap,
              outlines=True, max_contours=mc, max_vertices=mv)
    args = (item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"])
    off = FlowPredictor(fm, **kw)
    plain = off.predict_window(*args, to_host=False)
    on = FlowPredictor(fm, simplify=1.0, **kw)
    on.outline_chunk, on.simple_chunk = 3, 2                                 # the window crosses the borders of both sets of buffers
    masks = on.predict_window(*args, to_host=False)
    assert torch.equal(masks, plain)                                         # the masks of simplify=None bit for bit
    frames, flags = on.outline_report()
    want_frames, want_flags = off.outline_report()
    assert np.array_equal(flags, want_flags) and not flags.any() and len(frames) == DELTA
    assert all(np.array_equal(a, b) for f, g in zip(frames, want_frames) for a, b in zip(f, g))   # and its outlines
    simple, counts = on.simple_outline_report()
    assert len(simple) == DELTA and counts.shape == (DELTA, 4) and not counts[:, 3].any()
    for f in range(DELTA):
        c, v = np.zeros((1, mc, 6), np.int64), np.zeros((1, mv, 2), np.int32)
        c[0, :len(frames[f][0])], v[0, :len(frames[f][1])] = frames[f][0], frames[f][1]
        n = np.array([[len(frames[f][0]), len(frames[f][0]), len(frames[f][1]), 0]], np.int64)
        want = sref.outline_simplify(c, v, n, 16, 32)
        assert counts[f].tolist() == want[2][0].tolist() and np.array_equal(simple[f][0], want[0][0, :len(frames[f][0])])
        assert np.array_equal(simple[f][1], want[1][0, :int(want[2][0, 1])])
    print(f"window: {int(counts[:, 1].sum())} of {sum(len(f[1]) for f in frames)} vertices kept, rounds {counts[:, 2].tolist()}")
    assert counts[:, 1].sum() <= sum(len(f[1]) for f in frames) and counts[:, 2].min() >= 1
    rows, _ = on.region_report()
    path = str(tmp_path / "o.geojson")
    write_outlines_geojson(path, list(range(DELTA)), rows, (frames, flags), simplified=(simple, counts), tolerance=1.0)
    with open(path) as fh:
        doc = json.load(fh)
    assert doc["unconverged_frames"] == [] and len(doc["features"]) == sum(len(r) for r in rows)
    assert sum(len(r) - 1 for feat in doc["features"] for r in feat["geometry"]["coordinates"]) == counts[:, 1].sum()
    on.reset()
    assert len(on.simple_outline_report()[0]) == DELTA
    on.clear_report()
    assert on.simple_outline_report()[0] == []
