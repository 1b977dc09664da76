"""Georeferencing the mosaic, the parts that need no GPU: the rules twice in tests/ground_ref.py, vectorised against literal loops;
csrc/ground_defs.h run on the CPU by a stand-alone sanitized host program that walks canvas and raster tile by tile as the kernels do;
the properties of the definition shown on the reference alone (pixel areas telescope to the boundary's shoelace, exactly; the flip and
the quarter turn rectify a plane to itself and to np.rot90; half the gsd repeats pixels; a mirrored model; folded pixels); the ground
model's fits; the seventeenth hook table and the freeze of the sixteenth; the library's refusals and the argument checks of the Python
layers; and the writers."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ground_ref as gref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import georef, mosaic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc")
NEW = ["ground_area", "ground_rectify", "ground_points"]
K, CAP = gref.CLASSES, gref.MAX_REGIONS


def case(name):
    return [c for c in gref.op_cases() if c[0] == name][0]


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("name", [c[0] for c in gref.op_cases()])
def test_the_two_references_agree(name):
    _, size, origin, fwd, cls, other, index, rgba, raster = case(name)
    assert gref.check_forward(fwd, size, origin) == 0, gref.REFUSALS[gref.check_forward(fwd, size, origin)]
    with_index, without, rasters, pts = gref.case_reference(name)
    for got, want in zip(with_index, gref.area_loops(cls, fwd, origin, K, index, CAP)):
        assert np.array_equal(got, want)
    for got, want in zip(without, gref.area_loops(cls, fwd, origin, K)):
        assert np.array_equal(got, want)
    assert np.array_equal(with_index[0], without[0]) and np.array_equal(with_index[2], without[2]) and without[1].size == 0
    assert np.array_equal(pts, gref.points_loops(gref.case_points(size), fwd, origin))
    if raster is not None:
        inv = gref.invert(fwd)
        assert gref.check_inverse(inv, *raster) == 0
        outs, rgb = gref.rectify_loops(inv, origin, size, raster[0], raster[1], raster[2], gref.rectify_planes(cls, other, index), rgba, gref.FILL, gref.RGB_FILL)
        assert all(np.array_equal(a, b) for a, b in zip(outs, rasters[0])) and np.array_equal(rgb, rasters[1])


def test_the_cases_hold_what_they_promise():
    names = [c[0] for c in gref.op_cases()]
    assert {"1x1", "1x37", "41x1", "37x53"} <= {n.split()[0] for n in names}
    assert {f"{h}x{w}" for h in (gref.TH - 1, gref.TH, gref.TH + 1) for w in (gref.TW - 1, gref.TW, gref.TW + 1)} <= {n.split()[0] for n in names}
    assert {"flip", "turn", "shear", "mild", "strong", "steep"} == {n.split()[1] for n in names}
    kernel = open(os.path.join(CSRC, "ground_ops.hip")).read()
    assert (gref.TW, gref.TH) == tuple(int(v) for v in re.search(r"constexpr int TW = (\d+), TH = (\d+);", kernel).groups())
    for name, size, origin, fwd, cls, other, index, rgba, raster in gref.op_cases():
        assert origin != (size[0] // 2, size[1] // 2)                                                       # off-centre
        if size[0] * size[1] > 500:
            assert (cls == 255).any() and ((cls >= K) & (cls != 255)).any() and (cls < K).any()
            assert (index < 0).any() and (index >= CAP).any() and ((rgba >> 24) == 0).any()
    # the steep model uses most of the factor of 4 the denominators may differ by; one more step of tilt is refused
    _, size, origin, fwd, *_ = case("37x53 steep")
    d = [(fwd[6] * x + fwd[7] * y) + fwd[8] for x in (-origin[1], size[1] - origin[1]) for y in (-origin[0], size[0] - origin[0])]
    assert 3.4 < max(d) / min(d) <= 4.0
    beyond = fwd.copy()
    beyond[6:8] *= 1.3
    beyond[8] = 1.0 + beyond[6] * origin[1] + beyond[7] * origin[0]
    assert gref.REFUSALS[gref.check_forward(beyond, size, origin)] == "ratio"
    # the wide rasters hold tiles wholly outside the canvas' footprint, tiles that straddle it and tiles inside
    for name in ("wide shear", "wide mild"):
        plane = gref.case_reference(name)[2][0][0] != gref.FILL
        gh, gw = plane.shape
        tiles = [plane[v:v + gref.TH, u:u + gref.TW] for v in range(0, gh, gref.TH) for u in range(0, gw, gref.TW)]
        kinds = {"out" if not t.any() else "in" if t.all() else "straddle" for t in tiles}
        assert {"out", "straddle"} <= kinds and sum(1 for t in tiles if not t.any()) > len(tiles) // 2


# ------------------------------------------------------------------------------------------------ the properties of the definition
@pytest.mark.parametrize("model", ["flip", "turn", "shear", "mild", "strong", "steep"])
def test_pixel_areas_sum_to_the_shoelace_of_the_boundary_exactly(model):
    _, size, origin, fwd, *_ = case(f"37x53 {model}")
    a = gref.pixel_area2(fwd, size, origin)
    assert (a > 0).all()
    sign = gref.orientation(fwd)
    assert sign == -1                                                                                       # north up, y down
    for seed in (1, 2):
        inside = gref.blob(size, seed)
        assert 0.3 < inside.mean() < 0.7
        assert int(a[inside].sum()) == sign * gref.boundary_shoelace(inside, fwd, origin)
    # the whole canvas: the shoelace of its border, every lattice point of it a vertex
    ch, cw = size
    border = [(x, 0) for x in range(cw)] + [(cw, y) for y in range(ch)] + [(x, ch) for x in range(cw, 0, -1)] + [(0, y) for y in range(ch, 0, -1)]
    e, n = gref.corner(fwd, np.array([p[0] for p in border]) - origin[1], np.array([p[1] for p in border]) - origin[0])
    assert int(a.sum()) == sign * gref.polygon_shoelace(e, n)
    # ... which is not the four corners' quadrilateral in general: the rounding of the border's points is in it
    whole = gref.area(np.zeros(size, np.uint8), fwd, origin, 1)
    assert whole[0][0] == a.sum() and whole[2].tolist() == [ch * cw, 0, 0, 0]


def test_the_flip_and_the_quarter_turn_rectify_a_plane_to_itself_and_to_rot90():
    rng = np.random.default_rng(3)
    size, origin, gsd = (37, 53), (5, -4), 250
    plane = rng.integers(0, 255, size).astype(np.uint8)
    rgba = (rng.integers(0, 1 << 24, size).astype(np.int64) | (0xFF << 24)).astype(np.uint32)
    flip = gref.model_flip(gsd)
    e, n = gref.corner(flip, -origin[1], -origin[0])                                                       # the canvas' top-left corner on the ground
    outs, rgb = gref.rectify(gref.invert(flip), origin, size, size, gsd, (int(e), int(n)), (plane,), rgba)
    assert np.array_equal(outs[0], plane)
    assert np.array_equal(rgb, np.stack([(rgba >> s) & 0xFF for s in (0, 8, 16)], axis=2).astype(np.uint8))   # pixel centres on pixel centres: weight 0
    turn = gref.model_turn(gsd)
    e, n = gref.corner(turn, np.array([0, size[1]]) - origin[1], np.array([0, size[0]]) - origin[0])
    outs, _ = gref.rectify(gref.invert(turn), origin, size, size[::-1], gsd, (int(e.min()), int(n.max())), (plane,))
    assert np.array_equal(outs[0], np.rot90(plane))
    # half the gsd: every canvas pixel becomes four raster pixels
    e, n = gref.corner(flip, -origin[1], -origin[0])
    outs, _ = gref.rectify(gref.invert(flip), origin, size, (2 * size[0], 2 * size[1]), gsd // 2, (int(e), int(n)), (plane,))
    assert np.array_equal(outs[0], np.repeat(np.repeat(plane, 2, axis=0), 2, axis=1))
    # one raster pixel further out on every side: a frame of fill
    outs, rgb = gref.rectify(gref.invert(flip), origin, size, (size[0] + 2, size[1] + 2), gsd, (int(e) - gsd, int(n) + gsd), (plane,), rgba, 7, (1, 2, 3))
    assert np.array_equal(outs[0][1:-1, 1:-1], plane) and (outs[0][0] == 7).all() and (outs[0][:, -1] == 7).all() and rgb[0, 0].tolist() == [1, 2, 3]


def test_a_model_and_its_mirror_give_opposite_signs_and_equal_areas():
    for name in ("37x53 flip", "37x53 shear", "37x53 mild"):
        _, size, origin, fwd, cls, _, index, _, _ = case(name)
        mirror = fwd.copy()
        mirror[:3] = -mirror[:3]                                                                            # east becomes west
        assert gref.orientation(fwd) == -1 and gref.orientation(mirror) == 1
        e, n = gref.lattice(fwd, size, origin)
        em, nm = gref.lattice(mirror, size, origin)
        twice = gref.project(fwd, *np.meshgrid(np.arange(size[1] + 1) - origin[1], np.arange(size[0] + 1) - origin[0]))[0] * 2
        ties = (twice == np.floor(twice)) & (np.floor(twice) % 2 == 1)                                      # q + 0.5 a whole number
        assert np.array_equal(nm, n) and np.array_equal(em[~ties], -e[~ties])
        if not ties.any():                                                                                  # floor(q + 0.5) rounds ties up on both sides
            for a, b in zip(gref.area(cls, fwd, origin, K, index, CAP), gref.area(cls, mirror, origin, K, index, CAP)):
                assert np.array_equal(a, b)
    assert not ties.any()


def test_folded_pixels_are_counted_beyond_the_bounds():
    """A horizon across the canvas: beyond it the orientation turns over.  The library refuses such a model; the reference, asked all the
    same, counts those pixels as folded and sums the rest."""
    size, origin = (20, 30), (0, 0)
    fwd = np.array([800.0, 0, 0, 0, -800.0, 0, -1 / 12.5, 0, 1.0])                                         # the denominator is zero at i = 12.5
    assert gref.REFUSALS[gref.check_forward(fwd, size, origin)] == "denominator"
    cls = np.zeros(size, np.uint8)
    vec, loops = gref.area(cls, fwd, origin, 1), gref.area_loops(cls, fwd, origin, 1)
    assert all(np.array_equal(a, b) for a, b in zip(vec, loops))
    assert vec[2].tolist() == [12 * 20, 18 * 20, 0, 0]                                                      # columns 0..11 lie before the horizon
    a = gref.pixel_area2(fwd, size, origin)
    assert (a[:, :12] > 0).all() and (a[:, 12:] <= 0).all() and vec[0][0] == a[:, :12].sum()
    # and inside the bounds a pixel smaller than the millimetre grid folds by rounding: every corner on one point
    tiny = np.array([0.01, 0, 0, 0, -0.01, 0, 0, 0, 1.0])
    assert gref.check_forward(tiny, size, origin) == 0
    assert gref.area(cls, tiny, origin, 1)[2].tolist() == [0, 600, 0, 0]


# ------------------------------------------------------------------------------------------------ the ground model's fits
E0 = np.array([431250.0, 5412800.0])
TRUTH = {"similarity": [[0.212, -0.071, 10.0], [-0.071, -0.212, -20.0], [0, 0, 1]],
         "affine": [[0.25, 0.03, 10.0], [0.02, -0.24, -20.0], [0, 0, 1]],
         "projective": [[0.25, 0.03, 10.0], [0.02, -0.24, -20.0], [2e-5, -1e-5, 1]]}
FIT_ORIGIN = (7, -3)


def truth_points(kind, n, seed):
    xy = np.random.default_rng(seed).random((n, 2)) * np.array([4000.0, 3000.0])
    h = np.c_[xy - np.array([FIT_ORIGIN[1], FIT_ORIGIN[0]]), np.ones(n)] @ np.array(TRUTH[kind]).T
    return xy, h[:, :2] / h[:, 2:] + E0


MEASURED_RMS = 3.9e-10   # metres: the largest RMS of the six fits below on the CPU (eastings of 5.4e6 m have an ulp of 9.3e-10 m)


@pytest.mark.parametrize("kind,n", [("similarity", 2), ("similarity", 9), ("affine", 3), ("affine", 12), ("projective", 4), ("projective", 15)])
def test_each_kind_recovers_a_synthetic_model_from_exact_points(kind, n):
    """Measured on the CPU: RMS 0 with the fewest points (the system is square), 3.2e-10 m (similarity, 9 points), 3.8e-10 m (affine,
    12) and 2.6e-11 m (projective, 15): the rounding of eastings and northings of millions of metres in float64.  The bound is ten
    times the largest of them."""
    xy, en = truth_points(kind, n, 5 + n)
    model = georef.GroundModel.fit(xy, en, kind, origin=FIT_ORIGIN, crs="EPSG:32633")
    assert model.kind == kind and model.crs == "EPSG:32633" and model.residuals.shape == (n, 2)
    print(f"{kind} {n}: rms {model.rms:.3g} m")
    assert model.rms <= 10 * MEASURED_RMS
    test, want = truth_points(kind, 50, 99)
    assert np.abs(model.to_ground(test, FIT_ORIGIN) - want).max() <= 1e-7                                   # a tenth of a micrometre, anywhere on the canvas
    assert gref.orientation(model.forward) == -1 and np.array_equal(model.inverse, np.linalg.inv(model.forward.reshape(3, 3)).reshape(-1))
    assert model.origin_en == (round(en[:, 0].mean()), round(en[:, 1].mean())) and np.abs(model.forward).max() < 1e8   # small numbers for the device
    assert gref.check_forward(model.forward, (3000, 4000), FIT_ORIGIN) == 0
    # the device's integers agree with the host's floats to the rounding
    mm = gref.points(np.array([[0, 0], [4000, 3000], [1234, 567]]), model.forward, FIT_ORIGIN)
    assert np.abs(model.mm_to_en(mm) - model.to_ground([[0, 0], [4000, 3000], [1234, 567]], FIT_ORIGIN)).max() <= 0.00051


def test_a_similarity_from_telemetry():
    model = georef.GroundModel.from_telemetry(0.05, 30.0, (431250.4, 5412800.7), (2000.0, 1500.0), origin=FIT_ORIGIN, crs="local")
    assert model.kind == "similarity" and model.rms == 0.0 and model.origin_en == (431250.0, 5412801.0)
    at = model.to_ground([[2000, 1500], [2000, 1400], [2100, 1500]], FIT_ORIGIN)
    assert np.allclose(at[0], [431250.4, 5412800.7], atol=1e-8, rtol=0)
    assert np.allclose(at[1] - at[0], [5 * math.sin(math.radians(30)), 5 * math.cos(math.radians(30))], atol=1e-8, rtol=0)   # up the image: along the heading
    assert np.allclose(at[2] - at[0], [5 * math.cos(math.radians(30)), -5 * math.sin(math.radians(30))], atol=1e-8, rtol=0)  # to the right: 90 degrees clockwise of it
    assert gref.orientation(model.forward) == -1
    xy = np.array([[0.0, 0.0], [4000.0, 0.0], [0.0, 3000.0], [4000.0, 3000.0]])
    again = georef.GroundModel.fit(xy, model.to_ground(xy, FIT_ORIGIN), "similarity", origin=FIT_ORIGIN)
    assert again.rms <= 10 * MEASURED_RMS and np.abs(again.to_ground([[1234.5, 678.25]], FIT_ORIGIN) - model.to_ground([[1234.5, 678.25]], FIT_ORIGIN)).max() <= 1e-7
    assert model.mean_gsd_mm((3000, 4000), FIT_ORIGIN) == 50
    size, gsd, (e0, ntop) = model.raster((3000, 4000), FIT_ORIGIN)
    assert gsd == 50 and e0 % 50 == 0 and ntop % 50 == 0
    f = model.footprint_mm((3000, 4000), FIT_ORIGIN)
    assert e0 <= f[:, 0].min() and e0 + size[1] * gsd >= f[:, 0].max() and ntop >= f[:, 1].max() and ntop - size[0] * gsd <= f[:, 1].min()
    assert model.world_file(50, (1000, 2000)) == [0.05, 0.0, 0.0, -0.05, 431250.0 + 1.025, 5412801.0 + 1.975]
    for kw, word in ((dict(gsd_m=0), "got 0"), (dict(gsd_m=float("nan")), "nan"), (dict(heading_deg=float("inf")), "inf")):
        with pytest.raises(ValueError, match=re.escape(word)):
            georef.GroundModel.from_telemetry(**{**dict(gsd_m=0.05, heading_deg=0.0, centre_en=(0, 0), canvas_xy=(0, 0)), **kw})


def test_degenerate_control_points_raise():
    xy, en = truth_points("affine", 6, 1)
    line = np.stack([np.linspace(0, 100, 6), np.linspace(5, 55, 6)], axis=1)
    three = np.array([[0, 0], [100, 0], [200, 0], [50, 80.0]])                                             # three of the four on a line: no unique projective model
    for args, word in (((xy[:1], en[:1], "similarity"), "needs 2 or more control points, got 1"), ((xy[:2], en[:2], "affine"), "needs 3 or more control points, got 2"),
                       ((xy[:3], en[:3], "projective"), "needs 4 or more control points, got 3"), ((line, en, "affine"), "collinear"), ((line, en, "projective"), "collinear"),
                       ((np.repeat(xy[:1], 3, axis=0), en[:3], "similarity"), "coincide"), ((xy, np.repeat(en[:1], 6, axis=0), "affine"), "coincide"),
                       ((xy, en, "spline"), "'spline'"), ((xy, en[:5], "affine"), "(6, 2) and (5, 2)"), ((xy * np.nan, en, "affine"), "not finite"),
                       ((three, np.c_[three - [FIT_ORIGIN[1], FIT_ORIGIN[0]], np.ones(4)] @ np.array(TRUTH["affine"]).T[:, :2] + E0, "projective"), "do not determine")):
        with pytest.raises(ValueError, match=re.escape(word)):
            georef.GroundModel.fit(*args)
    with pytest.raises(ValueError, match="cannot be inverted"):
        georef.GroundModel([1, 2, 3, 2, 4, 6, 0, 0, 1], (0, 0))
    with pytest.raises(ValueError, match="not finite"):
        georef.GroundModel([1, 0, 0, 0, float("inf"), 0, 0, 0, 1], (0, 0))


def test_the_control_point_file(tmp_path):
    path = str(tmp_path / "gcp.csv")
    with open(path, "w") as f:
        f.write("x,y,easting,northing\n# a comment\n10,20,431250.5,5412800.25\n\n30.5;40.5;431260;5412790\n")
    xy, en = georef.read_gcp_csv(path)
    assert xy.tolist() == [[10, 20], [30.5, 40.5]] and en.tolist() == [[431250.5, 5412800.25], [431260, 5412790]]
    assert georef.read_gcp_csv(path, indices=True)[0].tolist() == [[10.5, 20.5], [31, 41]]
    with open(path, "w") as f:
        f.write("x,y,easting,northing\n10,20,abc,1\n")
    with pytest.raises(ValueError, match="line 2 is not x,y,easting,northing"):
        georef.read_gcp_csv(path)
    with open(path, "w") as f:
        f.write("x,y,easting,northing\n")
    with pytest.raises(ValueError, match="holds no control point"):
        georef.read_gcp_csv(path)


# ------------------------------------------------------------------------------------------------ the header on the CPU
def fmt(m):
    return " ".join(float(v).hex() for v in m)


def host_commands():
    cmds, want = [], []
    for name, size, origin, fwd, cls, other, index, rgba, raster in gref.op_cases():
        if name.split()[0] in ("15x63", "15x65", "17x63", "17x65", "16x64"):
            continue                                                                                        # the other tile sizes walk the same code
        (ch, cw), (oy, ox) = size, origin
        with_index, without, rasters, pts = gref.case_reference(name)
        cmds.append(f"check {ch} {cw} {ox} {oy} {fmt(fwd)}")
        want.append(f"0 {gref.orientation(fwd)}")
        head = f"area {ch} {cw} {ox} {oy} {K}"
        cells = " ".join(str(v) for v in cls.reshape(-1).tolist())
        cmds.append(f"{head} {CAP} {fmt(fwd)} {cells} " + " ".join(str(v) for v in index.reshape(-1).tolist()))
        want.append(" ".join(str(v) for part in with_index for v in part.tolist()))
        cmds.append(f"{head} 0 {fmt(fwd)} {cells}")
        want.append(" ".join(str(v) for part in without for v in part.tolist()))
        points = gref.case_points(size)
        cmds.append(f"points {len(points)} {ox} {oy} {fmt(fwd)} " + " ".join(str(v) for v in points.reshape(-1).tolist()))
        want.append(" ".join(str(v) for v in pts.reshape(-1).tolist()))
        if raster is not None:
            (gh, gw), gsd, (e0, ntop) = raster
            inv = gref.invert(fwd)
            word = gref.RGB_FILL[0] | gref.RGB_FILL[1] << 8 | gref.RGB_FILL[2] << 16
            cmds.append(f"checkinv {gh} {gw} {gsd} {e0} {ntop} {fmt(inv)}")
            want.append("0")
            cmds.append(f"rectify {ch} {cw} {ox} {oy} {gh} {gw} {gsd} {e0} {ntop} {gref.FILL} {word} {fmt(inv)} {cells} " + " ".join(str(v) for v in rgba.reshape(-1).tolist()))
            rgb = rasters[1].astype(np.int64)
            want.append(" ".join(str(v) for v in rasters[0][0].reshape(-1).tolist() + (rgb[..., 0] | rgb[..., 1] << 8 | rgb[..., 2] << 16).reshape(-1).tolist()))
    for model, size, origin, code in REFUSED_MODELS:
        cmds.append(f"check {size[0]} {size[1]} {origin[1]} {origin[0]} {fmt(model)}")
        want.append(f"{gref.REFUSALS.index(code)} {gref.orientation(model)}")
    return cmds, want


FLIP = gref.model_flip(250).tolist()
REFUSED_MODELS = [(FLIP[:4] + [float("nan")] + FLIP[5:], (64, 96), (0, 0), "not finite"), (FLIP[:8] + [float("inf")], (64, 96), (0, 0), "not finite"),
                  ([250.0, 0, 0, 500.0, 0, 0, 0, 0, 1], (64, 96), (0, 0), "orientation"), (FLIP[:6] + [-0.02, 0, 1.0], (64, 96), (0, 0), "denominator"),
                  (FLIP[:6] + [0, 0, -1.0], (64, 96), (0, 0), "denominator"), (FLIP[:6] + [0.04, 0, 1.0], (64, 96), (0, 0), "ratio"),
                  ([250.0, 0, 2.0 ** 31, 0, -250.0, 0, 0, 0, 1], (64, 96), (0, 0), "range"), ([250.0, 0, 0, 0, -250.0, -2.0 ** 31 + 1000, 0, 0, 1], (64, 96), (0, 0), "range"),
                  ([2.0 ** 30, 0, -2.0 ** 30, 0, -250.0, 0, 0, 0, 1], (1, 1), (0, 0), "step"), ([250.0, 0, 0, 0, -2.0 ** 30, 2.0 ** 29, 0, 0, 1], (1, 1), (0, 0), "step"),
                  ([130000.0, 0, 0, 0, -130000.0, 0, 0, 0, 1], (16384, 16384), (8192, 8192), "area"), (FLIP, (16384, 16384), (8192, 8192), "ok")]


def test_the_refused_models_are_the_references():
    for model, size, origin, code in REFUSED_MODELS:
        assert gref.REFUSALS[gref.check_forward(model, size, origin)] == code, (model, code)


def test_the_headers_rules_are_the_references_under_sanitizers(tmp_path):
    """csrc/ground_defs.h is plain __host__ __device__ C++: tests/ground_host_check.cpp walks every case tile by tile with the staged
    corner array of the kernels, and the rasters with the empty-tile test, as a stand-alone program built with
    -fsanitize=address,undefined -ffp-contract=off; every line it prints is the reference's."""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "ground_host_check"), str(tmp_path / "commands.txt")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", CSRC,
            os.path.join(ROOT, "tests", "ground_host_check.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):   # the runtimes linked in where the compiler can
        build = subprocess.run(base + static, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    cmds, want = host_commands()
    with open(data, "w") as fh:
        fh.write("\n".join(cmds) + "\n")
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(want) and len(want) >= 200
    skipped = 0
    for cmd, g, w in zip(cmds, got, want):
        if cmd.startswith("rectify"):
            tiles, _, g = g.partition(" ")
            skipped += int(tiles)
        assert g.strip() == w, (cmd[:120], g[:200], w[:200])
    assert skipped > 100                                                                                    # the wide rasters' empty tiles were skipped, not sampled


def test_the_rules_are_written_once():
    defs = open(os.path.join(CSRC, "ground_defs.h")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", defs).lower().replace("__hipcc__", "")
    kernel = open(os.path.join(CSRC, "ground_ops.hip")).read()
    assert all(f"gnd::{fn}(" in kernel for fn in ("corner", "corner_checked", "area2", "folded", "orientation", "check_forward", "check_inverse", "raster_ground",
                                                   "ground_to_anchor", "nearest_pixel", "rectify_colour", "tile_outside", "project"))
    code = re.sub(r"//[^\n]*", "", kernel.split("namespace fs {")[1])
    assert "asm" not in code and "hipMemset" not in code and "hipMalloc" not in code and "Synchronize" not in code and "hipMemcpy" not in code
    assert "while (true)" not in code and "for (;;)" not in code and " / d" not in code                   # every division is the header's
    assert "ground_clear_kernel" in code                                                                    # a clearing kernel, not a memset node
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " ground_ops.hip " in makefile
    assert re.search(r"\$\(OBJDIR\)/ground_ops\.o[^\n]*: CXXFLAGS \+= -ffp-contract=off", makefile)
    header = open(os.path.join(ROOT, "include", "floodseg_test.h")).read()
    assert int(re.search(r"#define FS_GROUND_MAX_PLANES (\d+)", header).group(1)) == ops.GROUND_MAX_PLANES == int(re.search(r"MAX_PLANES = (\d+);", defs).group(1))
    assert ops.GROUND_NO_POINT == gref.NO_POINT == -2 ** 63 and "#define FS_GROUND_NO_POINT INT64_MIN" in header
    assert ops.GROUND_MAX_GSD_MM == 1 << 20 and "MAX_GSD_MM = 1 << 20;" in defs
    for word in ("2^63", "telescopes", "convex hull"):                                                      # the header says why nothing leaves 63 bits
        assert word in defs


# ------------------------------------------------------------------------------------------------ library surface
def test_the_seventeenth_table_and_the_freeze_of_the_sixteenth():
    assert _lib.ext16_hook_names() == NEW
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext16_api {"):text.index("} fs_ext16_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == NEW
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables15;") < text.index("typedef struct fs_ext16_api {") < text.index("typedef struct fs_hook_tables16 {")
    tables16 = text[text.index("typedef struct fs_hook_tables16 {"):text.index("} fs_hook_tables16;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables16) == [("fs_hook_tables15", "base15"), ("fs_ext16_api", "ext16")]
    assert int(re.search(r"#define FS_EXT16_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT16_MAGIC == int.from_bytes(b"FSEXTA16", "big")
    # fs_ext15_api is frozen: the header and the binding name the same two members, 32 bytes
    frozen = text[text.index("typedef struct fs_ext15_api {"):text.index("} fs_ext15_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", frozen) == _lib.ext15_hook_names() == ["mask_access", "region_access"]
    assert ctypes.sizeof(_lib.FsExt15Api) == 32
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables16 all16 = {all15, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + name for name in NEW]
    assert "FS_EXT16_MAGIC," in init and "sizeof(fs_ext16_api)," in init
    assert re.search(r"const fs_hook_tables15& all15 = all16\.base15;\s+const fs_hook_tables14& all14 = all15\.base14;", src)
    kernels = open(os.path.join(CSRC, "kernels.h")).read()
    assert all(f"launch_{name}" in kernels for name in NEW)
    # the sixteen older tables and the export list are what they were
    assert [len(names()) for names in (_lib.hook_names, _lib.ext_hook_names, _lib.ext2_hook_names, _lib.ext3_hook_names, _lib.ext4_hook_names, _lib.ext5_hook_names,
                                       _lib.ext6_hook_names, _lib.ext7_hook_names, _lib.ext8_hook_names, _lib.ext9_hook_names, _lib.ext10_hook_names,
                                       _lib.ext11_hook_names, _lib.ext12_hook_names, _lib.ext13_hook_names, _lib.ext14_hook_names,
                                       _lib.ext15_hook_names)] == [38, 2, 14, 1, 1, 1, 1, 2, 4, 2, 3, 1, 5, 6, 1, 2]
    assert not any("fs_" + name in _lib.exported_symbols() for name in NEW) and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    public = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(name in public for name in NEW)
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables16.ext16.offset == ctypes.sizeof(_lib.FsHookTables15)                         # directly behind, no padding
    assert [getattr(_lib.FsExt16Api, name).offset for name in NEW] == [16, 24, 32] and ctypes.sizeof(_lib.FsExt16Api) == 40
    all16 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables16)).contents
    assert all16.base15.ext15.magic == _lib.EXT15_MAGIC and all16.base15.ext15.size == 32                 # frozen: exactly, not from below
    assert all16.base15.base14.ext14.magic == _lib.EXT14_MAGIC and all16.base15.base14.ext14.size == 24
    assert all16.ext16.magic == _lib.EXT16_MAGIC and all16.ext16.size >= 40                               # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all16.ext16, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                                            # a table member, not an exported symbol
    for name in ("mask_access", "region_access"):
        assert ctypes.cast(getattr(all16.base15.ext15, name), ctypes.c_void_p).value == ctypes.cast(getattr(lib, "fs_" + name), ctypes.c_void_p).value


def test_the_magic_is_checked_before_use(monkeypatch):
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT16_MAGIC", _lib.EXT16_MAGIC + 1)
    with pytest.raises(RuntimeError, match="the library has no sixteenth extension table \\(fs_ground_area is missing\\)"):
        fresh.fs_ground_area
    assert fresh.fs_mask_access is not None                                   # the tables in front of it stay usable
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT15_MAGIC", _lib.EXT15_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first sixteen hook tables are not the ones this binding knows \\(fs_ground_points is missing\\)"):
        fresh.fs_ground_points
    monkeypatch.undo()
    assert fresh.fs_ground_area is not None and fresh.fs_ground_rectify is not None and fresh.fs_ground_points is not None


P = 0x10000  # a dummy non-null pointer, aligned to 64 KiB: every call below must be refused before anything is launched


def doubles(m):
    return None if m is None else ctypes.cast((ctypes.c_double * 9)(*m), ctypes.c_void_p)


def call_area(lib, **kw):
    a = dict(cls=P, CH=64, CW=96, ox=0, oy=0, forward=FLIP, K=5, index=P, max_regions=64, class_area2=P, region_area2=P, counts=P)
    a.update(kw)
    return lib.fs_ground_area(a["cls"], a["CH"], a["CW"], a["ox"], a["oy"], doubles(a["forward"]), a["K"], a["index"], a["max_regions"], a["class_area2"],
                              a["region_area2"], a["counts"], None)


def call_rectify(lib, **kw):
    a = dict(inverse=gref.invert(FLIP).tolist(), CH=64, CW=96, ox=0, oy=0, GH=64, GW=96, gsd_mm=250, e0=0, ntop=0, nplanes=1, planes=[P], outs=[P], rgba=P, rgb_out=P,
             fill=255, rgb_fill=0)
    a.update(kw)
    arrays = [None if a[k] is None else ctypes.cast((ctypes.c_void_p * max(len(a[k]), 1))(*a[k]), ctypes.c_void_p) for k in ("planes", "outs")]
    return lib.fs_ground_rectify(doubles(a["inverse"]), a["CH"], a["CW"], a["ox"], a["oy"], a["GH"], a["GW"], a["gsd_mm"], a["e0"], a["ntop"], a["nplanes"], arrays[0],
                                 arrays[1], a["rgba"], a["rgb_out"], a["fill"], a["rgb_fill"], None)


def call_points(lib, **kw):
    a = dict(points=P, n=10, forward=FLIP, ox=0, oy=0, out=P)
    a.update(kw)
    return lib.fs_ground_points(a["points"], a["n"], doubles(a["forward"]), a["ox"], a["oy"], a["out"], None)


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    area_cases = [(dict(cls=None), b"null"), (dict(forward=None), b"null"), (dict(class_area2=None), b"null"), (dict(counts=None), b"null"), (dict(CH=0), b"0x96"),
                  (dict(CW=16385), b"64x16385"), (dict(ox=16385), b"ox=16385"), (dict(oy=-16385), b"oy=-16385"), (dict(K=0), b"classes=0"), (dict(K=256), b"classes=256"),
                  (dict(max_regions=-1), b"max_regions=-1"), (dict(max_regions=65537), b"max_regions=65537"), (dict(index=None), b"max_regions=64"),
                  (dict(region_area2=None), b"max_regions=64"), (dict(max_regions=0), b"max_regions=0"), (dict(index=P + 2), b"index is not aligned"),
                  (dict(class_area2=P + 4), b"aligned to 8"), (dict(region_area2=P + 4), b"aligned to 8"), (dict(counts=P + 4), b"aligned to 8")]
    words = {"not finite": b"not finite", "orientation": b"determinant is zero", "denominator": b"horizon crosses", "ratio": b"factor of 4", "range": b"2^31 mm",
             "step": b"2^30 mm", "area": b"2^61 mm^2"}
    for model, size, origin, code in REFUSED_MODELS[:-1]:
        shown = b"nan" if any(v != v for v in model) else b"inf" if any(math.isinf(v) for v in model) else ("%.17g" % model[0]).encode()
        area_cases.append((dict(forward=model, CH=size[0], CW=size[1], oy=origin[0], ox=origin[1]), words[code]))
        area_cases.append((dict(forward=model, CH=size[0], CW=size[1], oy=origin[0], ox=origin[1]), shown))       # the model is named by value
    for kw, word in area_cases:
        assert call_area(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert msg.startswith(b"ground_area:") and word in msg, (kw, msg)
    inv = gref.invert(FLIP).tolist()
    rectify_cases = [(dict(inverse=None), b"null"), (dict(CH=0), b"0x96"), (dict(ox=20000), b"ox=20000"), (dict(GH=0), b"0x96"), (dict(GW=16385), b"64x16385"),
                     (dict(gsd_mm=0), b"gsd_mm=0"), (dict(gsd_mm=(1 << 20) + 1), b"gsd_mm=1048577"), (dict(e0=1 << 40), b"1099511627776"),
                     (dict(ntop=-(1 << 40)), b"-1099511627776"), (dict(nplanes=9, planes=[P] * 9, outs=[P] * 9), b"9 planes"), (dict(nplanes=-1), b"-1 planes"),
                     (dict(planes=None), b"null"), (dict(outs=None), b"null"), (dict(planes=[0]), b"plane 0 is null"), (dict(nplanes=2, planes=[P, P], outs=[P, 0]), b"plane 1 is null"),
                     (dict(rgba=None), b"go together"), (dict(rgb_out=None), b"go together"), (dict(nplanes=0, rgba=None, rgb_out=None), b"nothing to rectify"),
                     (dict(fill=256), b"fill=256"), (dict(fill=-1), b"fill=-1"), (dict(rgb_fill=1 << 24), b"0x1000000"), (dict(rgba=P + 2), b"rgba is not aligned"),
                     (dict(inverse=inv[:3] + [float("nan")] + inv[4:]), b"not finite"), (dict(inverse=inv[:6] + [-1e-4, 0, 1.0]), b"horizon crosses"),
                     (dict(inverse=inv[:6] + [0, 0, -1.0]), b"horizon crosses"), (dict(inverse=inv[:6] + [2e-4, 0, 1.0]), b"factor of 4")]
    for kw, word in rectify_cases:
        assert call_rectify(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert msg.startswith(b"ground_rectify:") and word in msg, (kw, msg)
    points_cases = [(dict(points=None), b"null"), (dict(forward=None), b"null"), (dict(out=None), b"null"), (dict(n=0), b"n=0"), (dict(n=(1 << 28) + 1), b"n=268435457"),
                    (dict(ox=-16385), b"ox=-16385"), (dict(oy=16385), b"oy=16385"), (dict(points=P + 2), b"points is not aligned"), (dict(out=P + 4), b"out is not aligned"),
                    (dict(forward=FLIP[:2] + [float("inf")] + FLIP[3:]), b"not finite"), (dict(forward=[1.0, 2, 3, 2, 4, 6, 0, 0, 1]), b"determinant is zero")]
    for kw, word in points_cases:
        assert call_points(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert msg.startswith(b"ground_points:") and word in msg, (kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
class Pair:
    forward, inverse = FLIP, gref.invert(FLIP).tolist()


def test_the_ops_refuse_with_the_offending_value():
    cls, index = torch.zeros((40, 50), dtype=torch.uint8), torch.zeros((1, 40, 50), dtype=torch.int32)
    good = dict(cls=cls, model=Pair, origin=(0, 0), classes=5, index=index, max_regions=8)
    nan = (FLIP[:4] + [float("nan")] + FLIP[5:], Pair.inverse)
    for kw, word in ((dict(cls=cls.int()), "int32"), (dict(cls=cls[None]), "(1, 40, 50)"), (dict(cls=torch.zeros((1, 16385), dtype=torch.uint8)), "(1, 16385)"),
                     (dict(model=(FLIP, FLIP[:8])), "nine float64"), (dict(model=3), "nine float64"), (dict(model=nan), "the forward model holds a value that is not finite"),
                     (dict(origin=(0, 16385)), "(0, 16385)"), (dict(classes=0), "got 0"), (dict(classes=256), "got 256"), (dict(max_regions=65537), "65537"),
                     (dict(max_regions=-1), "-1"), (dict(index=None), "max_regions=8 and index None"), (dict(max_regions=0), "max_regions=0 and index given"),
                     (dict(index=index.long()), "int64"), (dict(index=index[:, :39]), "(1, 39, 50)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.ground_area(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.ground_area: tensors must live on the GPU"):
        ops.ground_area(**good)
    rgba = torch.zeros((40, 50), dtype=torch.int32)
    good = dict(model=Pair, origin=(0, 0), raster_size=(40, 50), gsd_mm=250, top_left_mm=(0, 0), planes=(cls, cls), rgba=rgba)
    for kw, word in ((dict(model=(FLIP, [float("inf")] * 9)), "the inverse model holds a value that is not finite"), (dict(origin=(-16385, 0)), "(-16385, 0)"),
                     (dict(raster_size=(0, 50)), "(0, 50)"), (dict(raster_size=(40, 16385)), "(40, 16385)"), (dict(gsd_mm=0), "got 0"), (dict(gsd_mm=250.5), "250.5"),
                     (dict(gsd_mm=(1 << 20) + 1), "1048577"), (dict(top_left_mm=(0.5, 0)), "(0.5, 0)"), (dict(top_left_mm=(0, 2 ** 40)), "1099511627776"),
                     (dict(planes=(cls,) * 9), "got 9 planes"), (dict(planes=(), rgba=None), "got 0 planes and rgba None"), (dict(planes=(cls, cls[:39])), "plane 1"),
                     (dict(planes=(cls.int(),)), "int32"), (dict(rgba=rgba.long()), "int64"), (dict(fill=256), "got 256"), (dict(rgb_fill=(0, 0)), "(0, 0)"),
                     (dict(rgb_fill=(0, 0, 256)), "(0, 0, 256)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.ground_rectify(**{**good, **kw})
    with pytest.raises(RuntimeError, match="floodseg.ground_rectify: tensors must live on the GPU"):
        ops.ground_rectify(**good)
    points = torch.zeros((5, 2), dtype=torch.int32)
    for kw, word in ((dict(points=points.long()), "int64"), (dict(points=points[:, :1]), "(5, 1)"), (dict(points=[[0, 0]]), "list"), (dict(model=nan), "not finite"),
                     (dict(origin=(16385, 0)), "(16385, 0)")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ops.ground_points(**{**dict(points=points, model=Pair, origin=(0, 0)), **kw})
    with pytest.raises(RuntimeError, match="floodseg.ground_points: tensors must live on the GPU"):
        ops.ground_points(points, Pair, (0, 0))
    assert ops.ground_model_rows(georef.GroundModel(FLIP, (0, 0))) == [FLIP, np.linalg.inv(np.array(FLIP).reshape(3, 3)).reshape(-1).tolist()]


def test_the_layer_refuses_before_anything_is_enqueued():
    model = georef.GroundModel(FLIP, (431250.0, 5412800.0))
    part = dict(votes=torch.zeros((5, 40, 50), dtype=torch.uint16), origin=(0, 0))
    for kw, word in ((dict(model=Pair), "GroundModel"), (dict(min_votes=0), "got 0"), (dict(outlines=True), "go with regions=True"),
                     (dict(regions=True, simplify=1.0), "goes with outlines=True"), (dict(gsd=0.0001), "0.0001"), (dict(gsd=2000.0), "2000.0"), (dict(tile=3), "['tile']")):
        with pytest.raises(ValueError, match=re.escape(word)):
            mosaic.mosaic_ground(part, **{**dict(model=model), **kw})
    assert "not validated on real video" in mosaic.mosaic_ground.__doc__ and "parallax" in mosaic.mosaic_ground.__doc__
    assert mosaic.MosaicBuilder.ground.__doc__ and "§3.26" in mosaic.MosaicBuilder.ground.__doc__


# ------------------------------------------------------------------------------------------------ the writers
def reference_result(simplify=None):
    """What mosaic_ground() hands to ground_report(), put together from the reference on CPU tensors: a 20 x 30 canvas with a lake with an
    island, flip model at a quarter of a metre."""
    size, origin = (20, 30), (2, 3)
    cls = np.zeros(size, np.uint8)
    cls[4:14, 5:20] = 1
    cls[8:10, 9:12] = 2
    cls[:, 27:] = 255
    model = georef.GroundModel(gref.model_flip(250, 1000, -2000), (431250.0, 5412800.0), "similarity", crs="EPSG:32633")
    index = np.where(cls == 1, 1, np.where(cls == 2, 2, np.where(cls == 0, 0, -1))).astype(np.int32)
    class_area2, region_area2, counts = gref.area(cls, model.forward, origin, 5, index, 4)
    table = np.zeros((1, 4, 10), np.int64)
    for r in range(3):
        ys, xs = np.nonzero(index == r)
        table[0, r, :2], table[0, r, 6:8] = (r, len(ys)), (xs.sum(), ys.sum())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    # the lake's outer ring (clockwise on the screen) and its hole, the island's ring; the background's outer ring is left out
    rings = [(1, [(5, 4), (20, 4), (20, 14), (5, 14)], 300), (1, [(9, 8), (9, 10), (12, 10), (12, 8)], -12), (2, [(9, 8), (12, 8), (12, 10), (9, 10)], 12)]
    vertices = np.array([p for _, ring, _ in rings for p in ring], np.int32)
    contours = np.zeros((1, 8, 6), np.int64)
    for k, (region, ring, area2) in enumerate(rings):
        contours[0, k] = (region, 4 * k, 4, 0, area2, 0)
    outline_counts = np.array([[3, 3, 12, 0]], np.int64)
    raster_size, gsd_mm, top_left = model.raster(size, origin)
    outs, rgb = gref.rectify(model.inverse, origin, size, raster_size, gsd_mm, top_left, (cls, cls), np.full(size, 0xFF204060, np.uint32))
    return dict(model=model, origin=origin, size=size, classes=5, plane=t(cls), conf=t(cls), changed=False, regions=(t(table), t(np.array([[3, 3]], np.int64)), t(index[None])),
                outlines=(t(contours), t(vertices[None]), t(np.zeros((1, 4, 3), np.int64)), t(outline_counts)), simplified=None, tolerance=simplify,
                points=t(gref.points(vertices, model.forward, origin)), simple_points=None, class_area2=t(class_area2), region_area2=t(region_area2), counts=t(counts),
                raster=dict(size=raster_size, gsd_mm=gsd_mm, top_left_mm=top_left, plane=t(outs[0]), conf=t(outs[1]), rgb=t(rgb))), cls


def test_the_writers_parse_back_to_the_numbers_that_went_in(tmp_path):
    result, cls = reference_result()
    report = mosaic.ground_report(result)
    m2 = 0.0625                                                                                             # a pixel of a quarter of a metre
    assert [round(a / m2, 9) for _, a, _ in report["classes"]] == [(cls == k).sum() for k in range(5)]
    assert report["summed_m2"] == (cls != 255).sum() * m2 and abs(sum(s for _, _, s in report["classes"]) - 1.0) < 1e-12
    assert [(r, k, p, a) for r, k, p, a, _, _ in report["regions"]] == [(0, 0, 390, 390 * m2), (1, 1, 144, 144 * m2), (2, 2, 6, 6 * m2)]
    # the island's centroid: pixels 9..11 x 8..9, centre (10.5, 9) in continuous canvas coordinates; anchor = canvas - origin
    assert report["regions"][2][4:] == (431250.0 + 1.0 + (10.5 - 3) * 0.25, 5412800.0 - 2.0 - (9.0 - 2) * 0.25)
    csv, png, geo = str(tmp_path / "areas.csv"), str(tmp_path / "class.png"), str(tmp_path / "regions.geojson")
    mosaic.write_ground_csv(csv, report, ["background", "water", "tree", "building", "street"])
    tables = open(csv).read().split("\n\n")
    assert tables[0].split("\n")[0] == "class,area_m2,hectares,share" and tables[0].split("\n")[2].split(",")[:3] == ["water", "9.000000", "0.000900"]
    assert tables[1].split("\n")[1] == "similarity,0,0.000000,0.000000,EPSG:32633,0"
    assert tables[2].split("\n")[2] == "1,water,144,9.000000,431253.396,5412796.250"
    mosaic.write_ground_png(png, report, "class")
    from PIL import Image
    picture = np.asarray(Image.open(png))
    raster = report["raster"]
    assert picture.shape == raster["plane"].shape + (3,) and np.array_equal(picture, mosaic.ground_image(report, "class"))
    world = [float(line) for line in open(str(tmp_path / "class.pgw")).read().split("\n")[:-1]]
    assert len(world) == 6 and world[:4] == [0.25, 0.0, 0.0, -0.25]
    # the world file's numbers put raster pixel (u, v)'s centre where the model puts the canvas pixel it shows
    v, u = [int(a[0]) for a in np.nonzero(raster["plane"] == 2)]
    e, n = world[4] + u * world[0], world[5] + v * world[3]
    back = (np.array([e, n]) - np.array(result["model"].origin_en)) * 1000.0
    x, y, _ = gref.project(result["model"].inverse, back[0], back[1])
    assert cls[int(np.floor(y)) + 2, int(np.floor(x)) + 3] == 2
    assert (mosaic.ground_image(report, "ortho")[raster["plane"] != 255] == [0x60, 0x40, 0x20]).all() and mosaic.ground_image(report, "conf").shape == picture.shape
    mosaic.write_ground_geojson(geo, report)
    doc = json.load(open(geo))
    assert doc["crs"] == {"type": "name", "properties": {"name": "EPSG:32633"}} and [f["properties"]["region"] for f in doc["features"]] == [1, 2]
    lake = doc["features"][0]["geometry"]["coordinates"]
    assert len(lake) == 2 and lake[0][0] == lake[0][-1] and len(lake[0]) == 5
    east, north = lambda x: 431250.0 + 1.0 + (x - 3) * 0.25, lambda y: 5412800.0 - 2.0 - (y - 2) * 0.25  # noqa: E731
    assert lake[0][:4] == [[east(5), north(4)], [east(20), north(4)], [east(20), north(14)], [east(5), north(14)]]
    assert lake[1][:4] == [[east(9), north(8)], [east(9), north(10)], [east(12), north(10)], [east(12), north(8)]]
    # the polygon's area in map coordinates is the table's: outer ring minus hole
    ring_area = lambda ring: abs(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(ring[:-1], ring[1:]))) / 2  # noqa: E731
    assert abs(ring_area(lake[0]) - ring_area(lake[1]) - doc["features"][0]["properties"]["area_m2"]) < 1e-6
    for kw, word in ((dict(what="ortho"), None), (dict(what="depth"), "'depth'")):
        if word:
            with pytest.raises(ValueError, match=re.escape(word)):
                mosaic.ground_image(report, **kw)
    with pytest.raises(ValueError, match="no outlines"):
        mosaic.write_ground_geojson(geo, {**report, "rings": None})
    with pytest.raises(ValueError, match="no raster"):
        mosaic.ground_image({**report, "raster": None})


def test_the_tools_argument_checks(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mosaic_ground_tool", os.path.join(ROOT, "tools", "mosaic_ground.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parse_args(["part.npz", "--gcp", "g.csv", "--areas", "a.csv", "--kind", "projective", "--gsd", "0.1", "--crs", "EPSG:32633", "--gcp-indices"])
    assert args.kind == "projective" and args.gsd == 0.1 and args.crs == "EPSG:32633" and args.gcp_indices and args.simplify is None
    for argv, word in ((["part.npz", "--gcp", "g.csv"], "nothing to write"), (["part.npz", "--areas", "a.csv"], "--gcp"),
                       (["part.npz", "--gcp", "g.csv", "--areas", "a.csv", "--gsd", "0"], "--gsd takes"), (["part.npz", "--gcp", "g.csv", "--areas", "a.csv", "--simplify", "1"], "--simplify goes with"),
                       (["part.npz", "--gcp", "g.csv", "--outlines", "o.json", "--simplify", "300"], "0..256"), (["part.npz", "--gcp", "g.csv", "--areas", "a.csv", "--kind", "spline"], "invalid choice"),
                       (["part.npz", "--gcp", "g.csv", "--areas", "a.csv", "--min-votes", "0"], "--min-votes"), (["part.npz", "--gcp", "g.csv", "--areas", "a.csv", "--max-regions", "0"], "--max-regions")):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
        assert word in capsys.readouterr().err
    assert "not validated on real video" in tool.__doc__ and "`mosaic_ground.py PART.npz" in open(os.path.join(ROOT, "tools", "README.md")).read()
