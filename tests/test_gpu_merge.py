"""Map-to-map registration and the merge of two mosaics on the GPU (ops.merge_view, ops.merge_gate, ops.link_correct, ops.mosaic_merge,
ops.merge_patch, ops.link_place, ops.register_mosaics) against the numpy restatement of the definition (tests/merge_ref.py),
bit for bit: views of two canvases with different origins and unseen holes under every kind of link, whole and in a sub-window; the
gate on six blocks and on sixty; the correction in every status; the merge with K = 1, 5 and 32 on tiles with remainders, saturating
votes, tied ranks, both orthophoto modes, the ordinal edge, links that do not merge, a second call, votes only; patches and placements
in every status; and end to end: a split flight registered to its exact pose and merged into the single chain's planes, a cut flight
that comes together with the coarse placement only, the register sequence from ONE captured graph."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import merge_ref as gref
import mosaic_ref as mref
import refine_ref as rref
from flood_uav_video_segmentation_amd import ops
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor, read_mosaic_part, write_mosaic_part

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = mref.ONE
OA, OB = gref.VIEW_ORIGIN_A, gref.VIEW_ORIGIN_B
MA, MB = gref.MERGE_ORIGIN_A, gref.MERGE_ORIGIN_B


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


def rgba32(a):
    return dev(a.view(np.int32))


def planes(ortho):
    return dev(ortho[0].view(np.int64)), dev(ortho[1].view(np.int32))


def same_planes(got, want):
    return np.array_equal(host(got[0]).view(np.uint64), want[0]) and np.array_equal(host(got[1]).view(np.uint32), want[1])


# ------------------------------------------------------------------------------------------------ merge_view
@pytest.mark.parametrize("window", gref.VIEW_WINDOWS)
def test_view_equals_the_reference_under_every_link(window):
    a, b = gref.view_canvases()
    d_a, d_b = rgba32(a), rgba32(b)
    for name, link in gref.view_links():
        got = ops.merge_view(d_a, OA, d_b, OB, dev(link), window)
        want = gref.merge_view(a, OA, b, OB, link, window)
        for plane, g, w in zip(("cur", "view", "valid_a", "valid_b"), got, want):
            assert np.array_equal(host(g), w), (name, plane)
    assert np.array_equal(host(d_a).view(np.uint32), a) and np.array_equal(host(d_b).view(np.uint32), b)      # only read


# ------------------------------------------------------------------------------------------------ merge_gate
def test_gate_equals_the_reference():
    for name, table, va, vb, _ in gref.gate_cases():
        got = ops.merge_gate(dev(table), dev(va), dev(vb))
        assert np.array_equal(host(got), gref.merge_gate(table, va, vb)), name


# ------------------------------------------------------------------------------------------------ link_correct
def test_correct_equals_the_reference_in_every_status():
    for name, model, link, status in gref.correct_cases():
        for window, origin in ((gref.CORRECT_WINDOW, gref.CORRECT_ORIGIN), ((0, 0, 16, 16), (0, 0))):
            d_link = dev(link)
            out = ops.link_correct(dev(model), d_link, window, origin)
            want_link, want_out = gref.correct_step(model, link, window, origin)
            assert np.array_equal(host(out), want_out) and np.array_equal(host(d_link), want_link), (name, window)
            if window == gref.CORRECT_WINDOW:
                assert host(out)[0] == status, name


# ------------------------------------------------------------------------------------------------ mosaic_merge
@pytest.mark.parametrize("k,mode", [(1, "centre"), (5, "latest"), (32, "centre")])
def test_merge_equals_the_reference(k, mode):
    """A 100 x 150 and B 70 x 90: tiles with remainders in both directions.  Every link; offsets 0, 7 and the one that pushes ordinals past
    0xFFFFFFFE; counts; A's three planes byte-identical where nothing merges; a second call adds the votes again and leaves the orthophoto."""
    va, oa, vb, ob = gref.merge_mosaics(k, mode=mode)
    d_vb, d_ob = dev(vb), planes(ob)
    for name, link, merges in gref.merge_links():
        for offset in (0, 7, 0xFFFFFFFE - 25):
            w_va, w_oa = va.copy(), (oa[0].copy(), oa[1].copy())
            want = gref.mosaic_merge(w_va, MA, vb, MB, link, w_oa, ob, offset, mode)
            d_va, d_oa, d_link = dev(va), planes(oa), dev(link)
            counts = ops.mosaic_merge(d_va, MA, d_vb, MB, d_link, d_oa, d_ob, offset, mode)
            assert np.array_equal(host(counts), want), (name, offset, host(counts).tolist(), want.tolist())
            assert np.array_equal(host(d_va), w_va) and same_planes(d_oa, w_oa), (name, offset)
            if not merges or name == "out of reach":
                assert np.array_equal(host(d_va), va) and same_planes(d_oa, oa), name
            elif offset == 7:
                again_want = gref.mosaic_merge(w_va, MA, vb, MB, link, w_oa, ob, offset, mode)
                again = ops.mosaic_merge(d_va, MA, d_vb, MB, d_link, d_oa, d_ob, offset, mode)
                assert np.array_equal(host(again), again_want) and again_want[4] == 0 and np.array_equal(host(d_va), w_va) and same_planes(d_oa, w_oa), name
    assert np.array_equal(host(d_vb), vb) and same_planes(d_ob, ob)                                          # B is only read


def test_merge_votes_only():
    va, oa, vb, ob = gref.merge_mosaics(5)
    for name, link, _ in gref.merge_links()[:3]:
        w_va = va.copy()
        want = gref.mosaic_merge(w_va, MA, vb, MB, link)
        d_va = dev(va)
        counts = ops.mosaic_merge(d_va, MA, dev(vb), MB, dev(link))
        assert np.array_equal(host(counts), want) and want[4] == 0 and np.array_equal(host(d_va), w_va), name


# ------------------------------------------------------------------------------------------------ merge_patch, link_place
@pytest.mark.parametrize("s", [4, 8])
def test_patch_equals_the_reference_in_every_status(s):
    seen = set()
    for name, link, box, size_a, ob, status in gref.patch_links():
        b = gref.patch_canvas_b(name)
        tl, tv, geom = ops.merge_patch(rgba32(b), ob, dev(link), size_a, OA, s, box)
        w_tl, w_tv, w_geom = gref.merge_patch(b, ob, link, size_a, OA, s, box)
        cells = w_tl.size
        assert np.array_equal(host(geom), w_geom) and w_geom[0] == status, (name, host(geom).tolist(), w_geom.tolist())
        assert np.array_equal(host(tl)[:cells], w_tl.reshape(-1)) and np.array_equal(host(tv)[:cells], w_tv.reshape(-1)), name
        seen.add(status)
    assert seen == {0, 1, 2, 3, 4}


def test_the_patch_kernel_on_canvas_b_in_every_shape():
    """The cells kernel that map_patch shares, with canvas B as its source, at S = 4 (16 of a wave's 64 lanes hold a pixel) and S = 16
    (four pixels a lane): a b_box that lands on exactly one cell of A, and one on 3 x 2 cells -- no multiple of the four a workgroup
    takes -- of which one holds B's only unseen pixel."""
    rng = np.random.RandomState(12)
    link = gref.link_row(*mref.affine_pose(1, 0, 0, 1, 32 - 8 + OB[1] - OA[1], 32 - 4 + OB[0] - OA[0]), status=gref.REGISTERED)   # B's (8, 4) on A's (32, 32)
    for s in (4, 16):
        b = rng.randint(0, 1 << 24, size=(64, 96)).astype(np.uint32) | np.uint32(0xFF000000)
        b[4 + s + 1, 8 + 1] = 0                                               # in the second row of cells, first column
        for box, cells, valid in (((4, 8, 4 + s, 8 + s), (1, 1), 1), ((4, 8, 4 + 2 * s, 8 + 3 * s), (3, 2), 5)):
            want = gref.merge_patch(b, OB, link, (96, 160), OA, s, box)
            assert want[2].tolist() == [0, 32 // s, 32 // s, cells[0], cells[1], valid, 0, 0], (s, box, want[2])            # the reference first
            tl, tv, geom = ops.merge_patch(rgba32(b), OB, dev(link), (96, 160), OA, s, box)
            assert np.array_equal(host(geom), want[2]), (s, box, host(geom).tolist())
            assert np.array_equal(host(tl)[:want[0].size], want[0].reshape(-1)) and np.array_equal(host(tv)[:want[1].size], want[1].reshape(-1)), (s, box)
            if valid == 5:
                assert want[1].tolist() == [[1, 1, 1], [0, 1, 1]]


def test_place_equals_the_reference_in_every_code():
    for name, found, link, max_mean, ratio, code in gref.place_cases():
        for s in (4, 8):
            d_link = dev(link)
            cand, out = ops.link_place(dev(found), d_link, s, max_mean, ratio)
            w_cand, w_out = gref.place_step(found, link, s, max_mean, ratio)
            assert np.array_equal(host(cand), w_cand) and np.array_equal(host(out), w_out) and w_out[0] == code and np.array_equal(host(d_link), link), name


# ------------------------------------------------------------------------------------------------ end to end
def gpu_merge(a, b, link, mode, origin=gref.SPLIT_ORIGIN, **register):
    """ops.register_mosaics and ops.mosaic_merge on copies of the reference's parts -> (votes, (rank, rgba), link, outs, counts) as numpy."""
    votes, ortho, d_link = dev(a["votes"]), planes((a["rank"], a["rgba"])), dev(link)
    b_ortho = planes((b["rank"], b["rgba"]))
    _, outs = ops.register_mosaics((ortho[1], origin), (b_ortho[1], origin), d_link, **register)
    counts = ops.mosaic_merge(votes, origin, dev(b["votes"]), origin, d_link, ortho, b_ortho, a["frames"], mode)
    return host(votes), (host(ortho[0]).view(np.uint64), host(ortho[1]).view(np.uint32)), host(d_link), host(outs), host(counts)


@pytest.mark.parametrize("mode", ["centre", "latest"])
def test_the_split_flight_is_the_references_and_the_single_chains(mode):
    """(a) the GPU sequence equals merge_ref; (b) the recovered b_to_a is frame 3's exact pose; (c) the merged planes equal the single
    chain's byte for byte."""
    whole, a, b, link, true = gref.split_flight(mode)
    want, w_link, w_outs, w_counts = gref.merge_parts(a, b, link, mode)
    votes, ortho, g_link, outs, counts = gpu_merge(a, b, link, mode)
    assert np.array_equal(g_link, w_link) and np.array_equal(outs, w_outs) and np.array_equal(counts, w_counts), (g_link.tolist(), outs.tolist(), counts.tolist())
    assert np.array_equal(votes, want["votes"]) and np.array_equal(ortho[0], want["rank"]) and np.array_equal(ortho[1], want["rgba"])
    assert g_link[:6].tolist() == true and g_link[12] == 0
    assert np.array_equal(votes, whole["votes"]) and np.array_equal(ortho[0], whole["rank"]) and np.array_equal(ortho[1], whole["rgba"])


def test_the_cut_flight_comes_together_with_the_placement_only():
    a, b, link, true, box = gref.cut_parts()
    votes, ortho, g_link, outs, counts = gpu_merge(a, b, link, "centre")
    assert outs[:, 0].tolist() == [2, 2] and np.array_equal(g_link, link) and counts.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(votes, a["votes"]) and np.array_equal(ortho[0], a["rank"]) and np.array_equal(ortho[1], a["rgba"])
    for s in (4, 8):
        want, w_link, w_outs, w_counts = gref.merge_parts(a, b, link, "centre", place=dict(scale=s, b_box=box))
        votes, ortho, g_link, outs, counts = gpu_merge(a, b, link, "centre", place=dict(scale=s, b_box=box))
        assert np.array_equal(g_link, w_link) and np.array_equal(outs, w_outs) and np.array_equal(counts, w_counts), (s, g_link.tolist(), outs.tolist())
        assert np.array_equal(votes, want["votes"]) and np.array_equal(ortho[0], want["rank"]) and np.array_equal(ortho[1], want["rgba"]), s
        assert g_link[:6].tolist() == true and g_link[12] == 0, s


def test_the_register_sequence_from_one_captured_graph_equals_eager():
    """Coarse placement and two fine rounds, enqueued once into ONE graph on one stream and replayed on fresh inputs: the cut flight, then
    the split flight's halves (whose placement finds the step of 4 px at S = 4)."""
    a, b, link, _, box = gref.cut_parts()
    _, a2, b2, link2, true2 = gref.split_flight("centre")
    place = dict(scale=4, b_box=box)
    inputs = [(rgba32(p["rgba"]), rgba32(q["rgba"]), dev(ln)) for p, q, ln in ((a, b, link), (a2, b2, link2))]
    wants = [gref.register_mosaics((p["rgba"], gref.SPLIT_ORIGIN), (q["rgba"], gref.SPLIT_ORIGIN), ln, place=place)[:2] for p, q, ln in ((a, b, link), (a2, b2, link2))]
    assert wants[1][0][:6].tolist() == true2
    ra, rb, ln = (t.clone() for t in inputs[0])
    _, eager = ops.register_mosaics((ra, gref.SPLIT_ORIGIN), (rb, gref.SPLIT_ORIGIN), ln, place=dict(scale=4, b_box=box))
    assert np.array_equal(host(ln), wants[0][0]) and np.array_equal(host(eager), wants[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, outs = ops.register_mosaics((ra, gref.SPLIT_ORIGIN), (rb, gref.SPLIT_ORIGIN), ln, place=dict(scale=4, b_box=box))
    for which in (0, 1, 0):
        for dst, src in zip((ra, rb, ln), inputs[which]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(ln), wants[which][0]) and np.array_equal(host(outs), wants[which][1]), (which, host(ln).tolist(), host(outs).tolist())


# ------------------------------------------------------------------------------------------------ FlowPredictor
@pytest.mark.parametrize("mode", ["centre", "latest"])
def test_predictor_merges_the_split_flight_directly_and_through_a_part_file(mode, tmp_path):
    """Three predictors mosaic frames 0..5, 0..2 and 3..5 of the split flight; the second takes the third's part -- handed over on the
    device, and read back from a part file -- with the default link: its reports are the single chain's, the recovered link is frame
    3's exact pose, the tail the last frame's, and the ordinal counter counts all six."""
    whole, a, b, link, true = gref.split_flight(mode)
    images, masks, tables = whole["inputs"]
    size = rref.FLIGHT_SIZE
    kw = dict(classes=gref.SPLIT_CLASSES, out_size=size, mosaic=gref.SPLIT_CANVAS, mosaic_classes=gref.SPLIT_CLASSES, mosaic_min_inliers=6, mosaic_exclude=(),
              mosaic_origin=gref.SPLIT_ORIGIN, ortho=mode)

    def run(lo, hi):
        pred = FlowPredictor(torch.nn.Identity(), **kw)
        sources = [(dev(images[f]), None, "rgb24", "bt601", False) for f in range(lo, hi)]
        pred.mosaic_builder.add(dev(np.stack(masks[lo:hi])), (dev(np.stack(tables[lo:hi])), size, None, None), sources)
        return pred

    single, second = run(0, 6), run(3, 6)
    path = str(tmp_path / "flight.part001.npz")
    write_mosaic_part(path, second.mosaic_part())
    for part in (second.mosaic_part(), read_mosaic_part(path, DEV)):
        first = run(0, 3)
        assert np.array_equal(host(first.mosaic_part()["votes"]), a["votes"]) and first.mosaic_part()["frames"] == 3
        first.merge_mosaic(part)
        for x, y in zip(first.mosaic_report()[:4] + first.ortho_report(overlay=False), single.mosaic_report()[:4] + single.ortho_report(overlay=False)):
            assert np.array_equal(x, y)
        links, outs, counts = first.merge_report()
        want, w_link, w_outs, w_counts = gref.merge_parts(a, b, link, mode)
        assert np.array_equal(links[0], w_link) and np.array_equal(outs[0], w_outs) and np.array_equal(counts[0], w_counts) and links[0][:6].tolist() == true
        assert first.mosaic_builder.frames == 6 and first.mosaic_part()["frames"] == 6
        assert host(first.mosaic_part()["tail"]).tolist() == whole["tail"].tolist() == host(single.mosaic_part()["tail"]).tolist()
        first.clear_report()
        assert first.merge_report()[0].shape == (0, 16)
    # rank 0 of a multi-rank launch: the parts of the ranks behind it, by their names, in rank order; a rank without windows wrote none
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("predict_video_tool_merge_gpu", os.path.join(root, "tools", "predict_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(["--raw", "c.rgb", "--raw-size", "64", "96", "--synthetic-weights", "--mosaic", str(tmp_path / "flight.png"), "--ortho", str(tmp_path / "o.png")])
    assert tool.mosaic_part_path(args.mosaic, 1) == path
    first = run(0, 3)
    assert tool.merge_rank_parts(first, args, [1, 1, 0]) == [path]
    for x, y in zip(first.mosaic_report()[:4] + first.ortho_report(overlay=False), single.mosaic_report()[:4] + single.ortho_report(overlay=False)):
        assert np.array_equal(x, y)
    # a merge that would pass the orthophoto's frame limit is refused before anything is enqueued: nothing of the predictor changes
    first = run(0, 3)
    first.mosaic_builder.MAX_FRAMES = 5
    with pytest.raises(ValueError, match="got 3 \\+ 3 with the part"):
        first.merge_mosaic(second.mosaic_part())
    assert np.array_equal(host(first.mosaic_part()["votes"]), a["votes"]) and first.mosaic_builder.frames == 3 and first.merge_report()[0].shape == (0, 16)
    assert np.array_equal(host(first.mosaic_part()["rank"]).view(np.uint64), a["rank"])


# ------------------------------------------------------------------------------------------------ the tool
def test_the_merge_tool_writes_the_single_chains_map_from_part_files(tmp_path):
    from PIL import Image

    from flood_uav_video_segmentation_amd.flow.predict import PALETTE

    whole, a, b, _, true = gref.split_flight("centre")
    paths = []
    for i, p in enumerate((a, b)):
        part = dict(votes=torch.from_numpy(p["votes"].copy()), rank=torch.from_numpy(p["rank"].view(np.int64).copy()), rgba=torch.from_numpy(p["rgba"].view(np.int32).copy()),
                    state=torch.from_numpy(p["state"].copy()), poses=torch.from_numpy(p["poses"].copy()), tail=torch.from_numpy(p["tail"].copy()),
                    origin=gref.SPLIT_ORIGIN, mask_size=rref.FLIGHT_SIZE, frames=p["frames"], mode="centre")
        paths.append(str(tmp_path / f"flight.part{i:03d}.npz"))
        write_mosaic_part(paths[-1], part)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("merge_mosaics_tool_gpu", os.path.join(root, "tools", "merge_mosaics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out, ortho, report = (str(tmp_path / n) for n in ("m.png", "o.png", "r.csv"))
    tool.main(paths + ["--out", out, "--ortho", ortho, "--report", report])
    cls = mref.mosaic_resolve(whole["votes"])[0]
    want = PALETTE[np.minimum(cls, len(PALETTE) - 1)]
    want[cls == 255] = 0
    assert np.array_equal(np.array(Image.open(out)), want)
    assert np.array_equal(np.array(Image.open(ortho)), host(ops.ortho_compose(rgba32(whole["rgba"]), dev(cls))))
    rows = open(report).read().split("\n")
    assert rows[1].startswith(f"flight.part001.npz,registered,1.000000,0.000000,{true[2] / ONE:.6f},0.000000,1.000000,0.000000,") and len(rows) == 3
