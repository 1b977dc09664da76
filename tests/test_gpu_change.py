"""ops.mosaic_change on the GPU against the numpy definition (tests/change_ref.py), bit for bit: every K, tolerance, threshold and watch set
at canvases with remainders in both directions and one smaller than a tile with its apron, under every link of merge_ref.view_links();
the inputs only read, a second call identical, A and B swapped; the three launches from ONE captured graph replayed on a second pair of
canvases; and two flights over the same ground end to end -- flow.predict.mosaic_change with and without registration, with regions,
through part files and tools/mosaic_change.py."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import change_ref as cref
import merge_ref as gref
import mosaic_ref as mref
import refine_ref as rref
from flood_uav_video_segmentation_amd import ops
from flood_uav_video_segmentation_amd.flow import predict
from flood_uav_video_segmentation_amd.flow.predict import read_mosaic_part, write_mosaic_part

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = mref.ONE
OA, OB = cref.VIEW_ORIGIN_A, cref.VIEW_ORIGIN_B
NAMES = ("change", "cls_a", "cls_b", "transitions", "counts")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)    # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = host(g)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, int((g != w).sum()), host(got[4]).tolist(), want[4].tolist())


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("case", cref.op_cases(), ids=lambda c: c[0])
def test_change_equals_the_reference_under_every_link(case):
    name, k, size_a, size_b, r, (min_votes, min_conf), watch = case
    va, vb = cref.case_inputs(k, size_a, size_b)
    d_a, d_b = dev(va), dev(vb)
    for lname, link, _ in cref.change_links():
        got = ops.mosaic_change(d_a, OA, d_b, OB, dev(link), min_votes, min_conf, r, watch)
        same(got, cref.mosaic_change(va, OA, vb, OB, link, min_votes, min_conf, r, watch), (name, lname))
    assert np.array_equal(host(d_a), va) and np.array_equal(host(d_b), vb)                      # the inputs are only read
    if k == 1:
        assert set(np.unique(host(got[0])).tolist()) <= {0, 1}
    if not watch or len(watch) == k:                                                            # no water, or nothing but water: nothing gained or lost
        counts = host(ops.mosaic_change(d_a, OA, d_b, OB, dev(cref.change_links()[0][1]), min_votes, min_conf, r, watch)[4])
        assert counts[6] == counts[7] == 0 and (counts[5] > 0 or k == 1)


def test_a_second_call_is_identical_and_the_sides_swap():
    va, vb = cref.case_inputs(5, cref.VIEW_A, cref.VIEW_B)
    link = cref.change_links()[2][1]                                                            # rotation and zoom
    d_a, d_b, d_link = dev(va), dev(vb), dev(link)
    first = ops.mosaic_change(d_a, OA, d_b, OB, d_link, 3, 170, 3, (1, 4))
    second = ops.mosaic_change(d_a, OA, d_b, OB, d_link, 3, 170, 3, (1, 4))
    want = cref.mosaic_change(va, OA, vb, OB, link, 3, 170, 3, (1, 4))
    same(first, want, "first"), same(second, want, "second")
    assert np.array_equal(host(d_link), link)
    back = np.concatenate([link[6:12], link[0:6], link[12:]])                                   # B's canvas is the one compared in
    same(ops.mosaic_change(d_b, OB, d_a, OA, dev(back), 3, 170, 3, (1, 4)), cref.mosaic_change(vb, OB, va, OA, back, 3, 170, 3, (1, 4)), "swapped")
    assert host(first[0]).shape == cref.VIEW_A


def test_the_extremes_of_the_thresholds():
    va, vb = cref.case_inputs(5, cref.VIEW_A, cref.VIEW_B)
    link = cref.change_links()[0][1]
    for min_votes, min_conf in ((65535, 0), (1, 255), (65535, 255), (9, 128)):
        got = ops.mosaic_change(dev(va), OA, dev(vb), OB, dev(link), min_votes, min_conf, 1, (1,))
        same(got, cref.mosaic_change(va, OA, vb, OB, link, min_votes, min_conf, 1, (1,)), (min_votes, min_conf))


def test_the_three_launches_from_one_captured_graph_equal_eager():
    """Enqueued once into ONE graph on one stream and replayed on a second pair of canvases and another link."""
    pairs = [cref.case_inputs(5, cref.VIEW_A, cref.VIEW_B), (cref.change_votes(5, cref.VIEW_A, 19), cref.change_votes(5, cref.VIEW_B, 23))]
    links = [cref.change_links()[1][1], cref.change_links()[2][1]]
    wants = [cref.mosaic_change(va, OA, vb, OB, ln, 3, 170, 8, (1,)) for (va, vb), ln in zip(pairs, links)]
    assert not np.array_equal(wants[0][0], wants[1][0])
    d_a, d_b, d_link = dev(pairs[0][0]), dev(pairs[0][1]), dev(links[0])
    same(ops.mosaic_change(d_a, OA, d_b, OB, d_link, 3, 170, 8, (1,)), wants[0], "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.mosaic_change(d_a, OA, d_b, OB, d_link, 3, 170, 8, (1,))
    for which in (1, 0, 1):
        d_a.copy_(dev(pairs[which][0])), d_b.copy_(dev(pairs[which][1])), d_link.copy_(dev(links[which]))
        graph.replay()
        torch.cuda.synchronize()
        same(got, wants[which], ("replay", which))


# ------------------------------------------------------------------------------------------------ end to end
def gpu_part(p, mode="centre"):
    """One of the reference's parts as FlowPredictor.mosaic_part() hands it out."""
    return dict(votes=dev(p["votes"]), rank=dev(p["rank"].view(np.int64)), rgba=dev(p["rgba"].view(np.int32)), state=dev(p["state"]), poses=dev(p["poses"]),
                tail=dev(p["tail"]), origin=gref.SPLIT_ORIGIN, mask_size=rref.FLIGHT_SIZE, frames=p["frames"], mode=mode)


def test_two_flights_register_and_the_painted_water_is_the_only_change():
    a, b, exact, (y0, x0, y1, x1) = cref.two_flights()
    want, w_link, w_outs = cref.flights_change(a, b, cref.off_link(-3))
    part_a, part_b = gpu_part(a), gpu_part(b)
    start = dev(cref.off_link(-3))
    result = predict.mosaic_change(part_a, part_b, link=start, regions=True, outlines=True, simplify=1.0)
    assert np.array_equal(host(start), cref.off_link(-3))                                       # the caller's link is not the one updated
    assert np.array_equal(host(result["link"]), w_link) and np.array_equal(host(result["outs"]), w_outs) and np.array_equal(w_link[:13], exact[:13])
    same([result[n] for n in NAMES], want, "registered")
    change, counts, transitions = host(result["change"]), host(result["counts"]), host(result["transitions"])
    painted = np.zeros(change.shape, bool)
    painted[y0:y1, x0:x1] = True
    assert np.array_equal(change == cref.GAINED, painted) and transitions[1].sum() == transitions[1, 0, cref.PAINT_CLASS] == 7 * 15
    assert counts[2] == counts[3:].sum() == transitions[0].sum() and counts[1] >= counts[2] and counts[5] == counts[7] == 0
    for p, q in ((part_a, a), (part_b, b)):
        assert np.array_equal(host(p["votes"]), q["votes"]) and np.array_equal(host(p["rgba"]).view(np.uint32), q["rgba"])   # neither mosaic is changed
    report = predict.change_report(result)
    rows = report["rows"][0]
    gained = rows[rows[:, 0] == cref.GAINED]
    assert len(gained) == 1 and gained[0, 1:6].tolist() == [7 * 15, x0, y0, x1 - 1, y1 - 1] and not (rows[:, 0] == cref.LOST).any()
    assert rows[:, 1].sum() == change.size and set(rows[:, 0].tolist()) == {0, 1, 4}
    row = int(np.nonzero(rows[:, 0] == cref.GAINED)[0][0])
    contours, vertices, shape = report["outlines"][0][0]
    assert report["outlines"][1].tolist() == [0] and shape[row, :2].tolist() == [2 * (7 + 15), 1]      # the rectangle's perimeter, one contour
    ring = contours[contours[:, 0] == row][0]
    corners = vertices[ring[1]:ring[1] + ring[2]].tolist()
    assert ring[4] == 2 * 7 * 15 and all(c in corners for c in ([x0, y0], [x1, y0], [x1, y1], [x0, y1]))
    assert report["simplified"][1][0, 3] == 0 and report["tolerance"] == 1.0
    # the default link is the identity with status 1: 12 px off, within the default search of 16
    default = predict.mosaic_change(part_a, part_b)
    assert np.array_equal(host(default["link"])[:13], exact[:13]) and np.array_equal(host(default["change"]), want[0]) and default["regions"] is None


def test_without_registration_the_tolerance_takes_the_misregistration():
    a, b, _, (y0, x0, y1, x1) = cref.two_flights()
    part_a, part_b = gpu_part(a), gpu_part(b)
    link = cref.off_link(1, status=0)
    for r in (0, 1):
        want, _, _ = cref.flights_change(a, b, link, register=False, tolerance=r)
        result = predict.mosaic_change(part_a, part_b, link=dev(link), register=False, tolerance=r)
        same([result[n] for n in NAMES], want, r)
        assert result["outs"] is None
    counts, change = host(result["counts"]), host(result["change"])
    assert counts[5] == counts[7] == 0 and counts[6] == 7 * 15 and np.array_equal(np.argwhere(change == cref.GAINED).min(0), [y0, x0 + 1])
    # small areas take their neighbours' code: at tolerance 0 the one-pixel boundary lines are areas too
    every, kept = (predict.change_report(predict.mosaic_change(part_a, part_b, link=dev(link), register=False, tolerance=0, regions=True, min_region_area=n))["rows"][0]
                   for n in (0, 4 * 64))
    assert len(kept) < len(every) and every[:, 1].min() < 4 * 64 and every[:, 1].sum() == kept[:, 1].sum() == change.size


def test_the_tool_writes_the_references_files_from_part_files(tmp_path):
    from PIL import Image

    a, b, exact, (y0, x0, y1, x1) = cref.two_flights()
    paths = []
    for name, p in (("before", a), ("after", b)):
        part = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in gpu_part(p).items()}
        paths.append(str(tmp_path / f"{name}.npz"))
        write_mosaic_part(paths[-1], part)
    back = read_mosaic_part(paths[1], DEV)
    assert np.array_equal(host(back["votes"]), b["votes"]) and back["origin"] == gref.SPLIT_ORIGIN
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mosaic_change_tool_gpu", os.path.join(root, "tools", "mosaic_change.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out, report, regions, outlines = (str(tmp_path / n) for n in ("c.png", "c.csv", "g.csv", "o.geojson"))
    tool.main(paths + ["--out", out, "--report", report, "--regions", regions, "--outlines", outlines])
    (change, _, _, transitions, counts), link, _ = cref.flights_change(a, b, gref.link_row())   # the tool's default link: the identity, status 1
    assert np.array_equal(link[:13], exact[:13])
    assert np.array_equal(np.array(Image.open(out)), cref.change_picture(change, a["rgba"]))
    assert open(report).read().split("\n") == cref.change_csv_lines(transitions, counts)
    lines = open(regions).read().split("\n")
    assert lines[0] == "frame,region,class,area,x0,y0,x1,y1,cx,cy,perimeter,holes"
    flooded = [ln.split(",") for ln in lines[1:] if ln.split(",")[2:3] == ["4"]]
    assert len(flooded) == 1 and flooded[0][2:] == ["4", "105", str(x0), str(y0), str(x1 - 1), str(y1 - 1), f"{(x0 + x1 - 1) / 2:.3f}", f"{(y0 + y1 - 1) / 2:.3f}", "44", "0"]
    doc = json.load(open(outlines))
    flooded = [f for f in doc["features"] if f["properties"]["class"] == 4]
    assert len(flooded) == 1 and flooded[0]["properties"]["area"] == 105 and len(flooded[0]["geometry"]["coordinates"][0]) == 5
    # without an orthophoto under it the change is drawn over a plain fill; --no-register compares under the identity link
    tool.main(paths + ["--out", out, "--no-register", "--tolerance", "0", "--report", report])
    ident = gref.link_row(status=gref.REGISTERED)
    (change, _, _, transitions, counts), _, _ = cref.flights_change(a, b, ident, register=False, tolerance=0)
    assert np.array_equal(np.array(Image.open(out)), cref.change_picture(change, a["rgba"])) and open(report).read().split("\n") == cref.change_csv_lines(transitions, counts)
    plain = predict.change_image(dict(change=dev(change)), None, fill=(9, 8, 7))
    assert np.array_equal(host(plain), cref.oref.ortho_compose(np.zeros(change.shape, np.uint32), change, cref.PALETTE, fill=(9, 8, 7)))
