"""ops.mask_access and ops.region_access on the GPU against the definition (tests/access_ref.py), bit for bit: the d and origin planes
and the status row at one-pixel frames, lines, frames of T - 1, T and T + 1 pixels a side (T = FS_ACCESS_TILE = 32), three frames of
different content sliced from a larger buffer at an odd byte offset, a frame without a valid seed, an open frame, a serpentine corridor
across dozens of tile borders, the origin's tie rule, a bound at the field's median; the contract of an unconverged call, resume and
want_origin; the tabulation through the existing region ops; and flow.mosaic.mosaic_access on a synthetic river with one bridge.

The status row's second word -- the rounds in which a value was lowered -- depends on how the tiles cut the frame and on which of two
neighbouring tiles of a round wrote first, not on the definition: it is checked for its range and against the words beside it, the
other three words exactly."""
import json

import numpy as np
import pytest
import torch

import access_ref as aref
from flood_uav_video_segmentation_amd import ops
from flood_uav_video_segmentation_amd.flow import mosaic

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROUNDS = 128   # enough for every route of the small cases: none crosses more than a few dozen tile borders


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def check_status(status, want, rounds, seeds_valid, what):
    status = host(status)
    assert status.dtype == np.int32 and status.shape == (want.shape[0], 4), what
    assert np.array_equal(status[:, [0, 2, 3]], want), (what, status.tolist(), want.tolist())
    for row, valid in zip(status.tolist(), seeds_valid):
        assert 0 <= row[1] <= rounds and (row[1] > 0) == (row[2] > valid), (what, row, valid)   # a round lowered something iff a value is not a seed's


def valid_seeds(mask, seeds, cost, terminal):
    return [int(((s != 0) & aref.pixel_kinds(m, cost, terminal)[1]).sum()) for m, s in zip(mask, seeds)]


def same_planes(got, want, what):
    d, origin = host(got[0]).view(np.uint32), host(got[1])
    assert d.shape == want[0].shape and origin.dtype == np.int32, what
    assert np.array_equal(d, want[0]), (what, "d", int((d != want[0]).sum()))
    assert np.array_equal(origin, want[1]), (what, "origin", int((origin != want[1]).sum()))


# ------------------------------------------------------------------------------------------------ the field
@pytest.mark.parametrize("case", aref.op_cases(), ids=lambda c: c[0])
def test_the_field_equals_the_reference(case):
    name, m, s, cost, terminal, conn = case
    want = aref.case_reference(name)
    if m.shape[0] == 3:   # sliced from a larger buffer at an odd byte offset
        big_m, big_s = torch.zeros(m.size + 64, dtype=torch.uint8, device=DEV), torch.zeros(m.size + 64, dtype=torch.uint8, device=DEV)
        d_m, d_s = big_m[13:13 + m.size].view(m.shape), big_s[7:7 + m.size].view(m.shape)
        d_m.copy_(dev(m)), d_s.copy_(dev(s))
        assert d_m.data_ptr() % 2 == 1 and d_s.data_ptr() % 2 == 1
        assert [row[1] for row in want[2].tolist()] == [want[2][0, 1], 0, m.shape[1] * m.shape[2]] and want[2][0, 1] > 1000   # mixed, no valid seed, all reached
    else:
        d_m, d_s = dev(m), dev(s)
    got = ops.mask_access(d_m, d_s, cost, terminal, conn, rounds=ROUNDS)
    same_planes(got, want, name)
    check_status(got[2], want[2], ROUNDS, valid_seeds(m, s, cost, terminal), name)
    assert np.array_equal(host(d_m), m) and np.array_equal(host(d_s), s)   # the inputs are only read
    if name == "junction":   # both seeds are 30 streets from the junction: everything on the side street belongs to the lower index
        origin = host(got[1])[0]
        assert set(origin[21:41, 32].tolist()) == {20 * 65 + 2} and origin[20, 33] == 20 * 65 + 62 and origin[20, 32] == 20 * 65 + 2
    # the bound at the median of the unbounded field removes the values above it and changes none
    vals = want[0][want[0] != aref.NONE]
    if vals.size > 2 and np.median(vals) >= 1:
        r = int(np.median(vals))
        bounded = ops.mask_access(d_m, d_s, cost, terminal, conn, max_cost=r, rounds=ROUNDS)
        want_r = aref.case_reference(name, r)
        same_planes(bounded, want_r, (name, r))
        assert np.array_equal(host(bounded[2])[:, [0, 2, 3]], want_r[2])
        keep = want[0] <= r
        assert np.array_equal(want_r[0][keep], want[0][keep]) and (want_r[0][~keep] == aref.NONE).all()


def test_the_serpentine_converges_within_256_rounds():
    m, s, cost, terminal = aref.serpentine()
    want = aref.serpentine_reference()
    assert want[2][0, 1] == (m == 4).sum() and want[0][want[0] != aref.NONE].max() > 60000   # every street pixel, 6288 of them, in one chain
    got = ops.mask_access(dev(m), dev(s), cost, terminal, 8, rounds=256)
    print("serpentine status", host(got[2]).tolist())
    same_planes(got, want, "serpentine")
    check_status(got[2], want[2], 256, [1], "serpentine")


def test_an_unconverged_call_holds_upper_bounds_and_resume_finishes_it():
    m, s, cost, terminal = aref.serpentine()
    want = aref.serpentine_reference()
    d_m, d_s = dev(m), dev(s)
    d, origin, status = ops.mask_access(d_m, d_s, cost, terminal, 8, rounds=1)
    st = host(status)[0].tolist()
    assert st[0] == 0 and st[1] == 1 and 1 < st[2] < want[2][0, 1] and st[3] == 0, st
    part = host(d).view(np.uint32)
    valued = part != aref.NONE
    assert valued.sum() == st[2] and (part[valued] >= want[0][valued]).all()                    # never too small
    ok, where = aref.real_routes(m[0], part[0], s[0], cost, terminal, 8)
    assert ok, where                                                                             # every value is the cost of a real route
    rounds = 1
    for _ in range(4):                                                                           # at most 4 x 64 more rounds: 257 in all
        d2, origin2, status = ops.mask_access(d_m, d_s, cost, terminal, 8, rounds=64, resume=(d, origin))
        assert d2 is d and origin2 is origin
        rounds += 64
        if host(status)[0, 0]:
            break
    assert host(status)[0, 0] == 1, rounds
    same_planes((d, origin), want, "resumed")
    assert host(status)[0, [0, 2, 3]].tolist() == want[2][0].tolist()
    before = (d.clone(), origin.clone())
    _, _, status = ops.mask_access(d_m, d_s, cost, terminal, 8, rounds=3, resume=(d, origin))   # a converged frame stays exactly as it is
    assert torch.equal(d, before[0]) and torch.equal(origin, before[1]) and host(status)[0].tolist() == [1, 0, int(want[2][0, 1]), 0]


def test_without_the_origin_plane_the_costs_are_the_same():
    name, m, s, cost, terminal, conn = [c for c in aref.op_cases() if c[0] == "70x150x3"][0]
    want = aref.case_reference(name)
    d, origin, status = ops.mask_access(dev(m), dev(s), cost, terminal, conn, rounds=ROUNDS, want_origin=False)
    assert origin is None and np.array_equal(host(d).view(np.uint32), want[0]) and np.array_equal(host(status)[:, [0, 2, 3]], want[2])
    out = (torch.empty_like(d), None)
    d2, _, _ = ops.mask_access(dev(m), dev(s), cost, terminal, conn, rounds=ROUNDS, want_origin=False, out=out)
    assert d2 is out[0] and torch.equal(d2, d)


# ------------------------------------------------------------------------------------------------ the tabulation
@pytest.mark.parametrize("name, cap", [("70x150x3", 1024), ("70x150x3", 40), ("speckle 66x97", 2048), ("33x33", 64)])
def test_the_tabulation_equals_numpy(name, cap):
    _, m, s, cost, terminal, conn = [c for c in aref.op_cases() if c[0] == name][0]
    d_m = dev(m)
    d, origin, _ = ops.mask_access(d_m, dev(s), cost, terminal, conn, rounds=ROUNDS)
    labels = ops.mask_regions(d_m, 5, conn)
    table, counts, index = ops.region_table(d_m, labels, 5, None, 128, cap)
    reach, rows = ops.region_access(d_m, d, origin, index, counts, 5, cap)
    h_d, h_o, h_i, h_c = host(d).view(np.uint32), host(origin), host(index), host(counts)
    want_reach, want_rows = aref.region_access(m, h_d, h_o, h_i, h_c, 5, cap)
    assert np.array_equal(host(reach), want_reach), (host(reach).tolist(), want_reach.tolist())
    assert np.array_equal(host(rows), want_rows), int((host(rows) != want_rows).any(-1).sum())
    written = np.minimum(h_c[:, 1], cap)
    if cap == 40:
        assert (h_c[:2, 0] > cap).all() and (written[:2] == cap).all() and written[2] == 1          # regions past max_regions have no row
    assert (want_rows[0, :written[0], 0] == -1).any() and (want_rows[0, :written[0], 0] > 0).any()   # an unreached region and a reached one
    assert all((want_rows[f, written[f]:] == 0).all() for f in range(m.shape[0]))
    reach2, rows2 = ops.region_access(d_m, d, None, index, counts, 5, cap)                        # without the origin plane
    row_written = np.arange(cap)[None, :, None] < written[:, None, None]
    want_rows[..., 3:6] = np.where(row_written & (want_rows[..., :1] >= 0), -1, want_rows[..., 3:6])
    assert torch.equal(reach2, reach) and np.array_equal(host(rows2), want_rows)


# ------------------------------------------------------------------------------------------------ the mosaic layer
def building_rows(report, boxes):
    """The region rows of the buildings whose boxes are given."""
    found = []
    for y0, x0, y1, x1 in boxes:
        hit = [r for r, t in enumerate(report["table"].tolist()) if t[0] == 3 and t[2:6] == [x0, y0, x1 - 1, y1 - 1]]
        assert len(hit) == 1, (y0, x0, hit)
        found.append(hit[0])
    return found


@pytest.mark.parametrize("cut", [False, True], ids=["dry bridge", "bridge under water"])
def test_the_far_bank_is_cut_off_when_the_bridge_floods(cut, tmp_path):
    part = dict(votes=dev(aref.scene_votes(cut)))
    result = mosaic.mosaic_access(part, seeds=dict(points=[aref.SCENE_SEED]), chunk=16)
    report = mosaic.access_report(result)
    cls = aref.scene_classes(cut)
    assert result["converged"] and report["status"][0] == 1 and np.array_equal(report["cls"], cls)
    seeds = np.zeros((1,) + aref.SCENE, np.uint8)
    seeds[0, aref.SCENE_SEED[1], aref.SCENE_SEED[0]] = 1
    want = aref.mask_access(cls[None], seeds, aref.SCENE_COST, (3,), 8)
    assert np.array_equal(report["d"], want[0][0]) and np.array_equal(report["origin"], want[1][0]) and report["status"][2] == want[2][0, 1]
    near, far = building_rows(report, aref.NEAR_BUILDINGS), building_rows(report, aref.FAR_BUILDINGS)
    assert all(report["rows"][r, 0] > 0 for r in near)
    if cut:
        assert all(report["rows"][r].tolist() == [-1, -1, -1, -1, -1, -1, 0, -1] for r in far)  # exactly the far bank's buildings
        cut_off = [r for r, (t, a) in enumerate(zip(report["table"].tolist(), report["rows"].tolist())) if t[0] == 3 and a[0] < 0]
        assert sorted(cut_off) == sorted(far)
    else:
        assert all(report["rows"][r, 0] > 0 for r in far)
    # the CSV is the reference's, from the reference's field through the numpy tabulation
    index, counts = host(result["regions"][2]), host(result["regions"][1])
    want_reach, want_rows = aref.region_access(cls[None], want[0], want[1], index, counts, 5, 1024)
    assert np.array_equal(report["reach"], want_reach[0]) and np.array_equal(report["rows"], want_rows[0, :len(report["rows"])])
    path = str(tmp_path / "a.csv")
    mosaic.write_access_csv(path, report)
    assert open(path).read().split("\n") == aref.access_csv_lines(report["table"], len(report["table"]), want_rows[0], True)
    # a route from every reached building back to the seed, the summed moves its cost
    for r in near + ([] if cut else far):
        cost, x, y = (int(v) for v in report["rows"][r, :3])
        chain = mosaic.access_route(report, x, y)
        assert chain == aref.access_route(want[0][0], cls, aref.SCENE_COST, (3,), 8, x, y)
        assert chain[0] == (x, y) and chain[-1] == aref.SCENE_SEED and aref.route_cost(chain, cls, aref.SCENE_COST) == cost
    mosaic.write_access_geojson(str(tmp_path / "a.geojson"), report)
    features = json.load(open(str(tmp_path / "a.geojson")))["features"]
    assert sorted(f["properties"]["region"] for f in features) == sorted(near + ([] if cut else far))
    mosaic.write_access_png(str(tmp_path / "a.png"), report)
    image = mosaic.access_image(report)
    y0, x0, y1, x1 = aref.FAR_BUILDINGS[0]
    assert image.shape == aref.SCENE + (3,) and (tuple(image[y0, x0]) == mosaic.ACCESS_CUT_OFF) == cut
    # too few rounds: flagged, never passed off as final
    short = mosaic.mosaic_access(part, seeds=dict(points=[aref.SCENE_SEED]), chunk=1, max_rounds=2, regions=False)
    assert not short["converged"] and short["rounds"] == 2 and host(short["status"])[0] == 0
    with pytest.raises(ValueError, match="has not converged"):
        mosaic.access_route(mosaic.access_report(short), *aref.SCENE_SEED)


def test_the_seed_planes():
    cls = dev(aref.scene_classes())
    border = host(mosaic.access_seeds(cls, "border"))
    h, w = aref.SCENE
    want = np.zeros(aref.SCENE, np.uint8)
    want[3, 2:w - 2] = want[h - 4, 2:w - 2] = want[3:h - 3, 2] = want[3:h - 3, w - 3] = 1          # the ring just inside the unseen margin
    assert np.array_equal(border, want)
    both = host(mosaic.access_seeds(cls, dict(points=[(5, 60), (100, 7)], classes=(4,))))
    assert both[60, 5] == 1 and both[7, 100] == 1 and np.array_equal(both != 0, (aref.scene_classes() == 4) | (np.indices(aref.SCENE)[0] == 7) & (np.indices(aref.SCENE)[1] == 100))
    result = mosaic.mosaic_access(dict(votes=dev(aref.scene_votes())), seeds="border", regions=False)
    assert result["converged"] and host(result["d"]).view(np.uint32)[60, 30] != aref.NONE
