"""Connected regions on the GPU: mask_regions, region_table and region_filter (csrc/region_ops.hip through the third hook table)
against the numpy definition (tests/regions_ref.py) by integer equality, and one window end to end through
FlowPredictor(regions=True / min_region_area=9) and tools/predict_video.py --regions."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import motion_modes_ref as modes_ref
import regions_ref as ref
from flood_uav_video_segmentation_amd import _lib, ops, synth
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import PALETTE, FlowPredictor, write_regions_csv

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARDS = {torch.uint8: 0xA5, torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                            # a copy: the shared expectations are read-only


class Guarded:
    """A view of `shape` at element `offset` inside a buffer filled with a guard value (offset 1 and 3 on a byte plane: the byte-store
    path even where W % 4 == 0)."""

    def __init__(self, shape, dtype, offset):
        self.count, self.offset, self.guard = int(np.prod(shape)), offset, GUARDS[dtype]
        self.buf = torch.full((self.count + 64,), self.guard, dtype=dtype, device=DEV)
        self.view = self.buf[offset:offset + self.count].view(shape)

    def intact(self):
        return bool((self.buf[:self.offset] == self.guard).all() and (self.buf[self.offset + self.count:] == self.guard).all())


def run_guarded(mask, conf, k, conn, cap, low, min_area, offset):
    """The three ops through the library itself with every output inside a guarded buffer."""
    lib = _lib.load()
    n, h, w = mask.shape
    labels, index = Guarded((n, h, w), torch.int32, offset), Guarded((n, h, w), torch.int32, offset)
    table, counts = Guarded((n, cap, 10), torch.int64, offset), Guarded((n, 2), torch.int64, offset)
    work, votes = Guarded((n, -(-h * w // ops.REGION_RANK_CHUNK)), torch.int32, offset), Guarded((n, cap, k), torch.int32, offset)
    out = Guarded((n, h, w), torch.uint8, offset)
    check(lib.fs_mask_regions(ptr(mask), n, h, w, k, conn, ptr(labels.view), stream_ptr()))
    check(lib.fs_region_table(ptr(mask), ptr(labels.view), ptr(conf), n, h, w, k, low, cap, ptr(table.view), ptr(counts.view), ptr(index.view),
                              ptr(work.view), stream_ptr()))
    check(lib.fs_region_filter(ptr(mask), ptr(index.view), ptr(table.view), n, h, w, k, cap, min_area, ptr(out.view), ptr(votes.view), stream_ptr()))
    torch.cuda.synchronize()
    assert all(g.intact() for g in (labels, index, table, counts, work, votes, out)), offset
    return labels.view, table.view, counts.view, index.view, out.view


@pytest.mark.parametrize("case", range(len(ref.CASES)))
def test_every_pattern_and_connectivity_equals_the_definition(case):
    for pattern in ref.PATTERNS:
        for conn in (4, 8):
            e = ref.expected(case, pattern, conn)
            what = (ref.CASES[case], pattern, conn)
            mask, conf, k, cap = dev(e["mask"]), dev(e["conf"]), e["classes"], e["cap"]
            labels = ops.mask_regions(mask, k, conn)
            assert labels.dtype == torch.int32 and torch.equal(labels, dev(e["labels"])), what
            for key, c, low, mr in (("with_conf", conf, 100, cap), ("without", None, 128, cap), ("overflow", conf, 100, ref.OVERFLOW_CAP)):
                table, counts, index = ops.region_table(mask, labels, k, c, low, mr)
                want = e[key]
                assert torch.equal(counts, dev(want[1])) and torch.equal(index, dev(want[2])) and torch.equal(table, dev(want[0])), what + (key,)
                if key == "with_conf":
                    for a in ref.MIN_AREAS:
                        assert torch.equal(ops.region_filter(mask, index, table, k, a), dev(e["filtered"][a])), what + (a,)
                elif key == "overflow":
                    assert torch.equal(ops.region_filter(mask, index, table, k, 9), dev(e["filtered_overflow"])), what + (key,)
            # every store path writes the same values and nothing else: outputs at element offsets 4, 1 and 3 of guarded buffers
            for offset in (4, 1, 3):
                got = run_guarded(mask, conf, k, conn, cap, 100, 9, offset)
                for g, w in zip(got, (e["labels"],) + e["with_conf"] + (e["filtered"][9],)):
                    assert torch.equal(g, dev(w)), what + (offset,)


def test_refusals_launch_nothing():
    """Every refusal of the header, with real device buffers: the call fails with its message and no output byte changes."""
    lib = _lib.load()
    n, h, w, k, cap = 2, 8, 8, 5, 16
    mask = torch.zeros((n, h, w), dtype=torch.uint8, device=DEV)
    outs = dict(labels=Guarded((n, h, w), torch.int32, 0), index=Guarded((n, h, w), torch.int32, 0), table=Guarded((n, cap, 10), torch.int64, 0),
                counts=Guarded((n, 2), torch.int64, 0), workspace=Guarded((n, 1), torch.int32, 0), votes=Guarded((n, cap, k), torch.int32, 0),
                out=Guarded((n, h, w), torch.uint8, 0))
    real = dict(mask=mask.data_ptr(), conf=mask.data_ptr(), **{name: g.view.data_ptr() for name, g in outs.items()})
    for op, kw, word in ref.refusal_cases():
        args = dict(real)
        args.update(kw)
        assert ref.call_region_op(lib, op, **args) != 0, (op, kw)
        msg = lib.fs_last_error()
        assert word in msg and op.encode() in msg, (op, kw, msg)
    torch.cuda.synchronize()
    assert all(bool((g.buf == g.guard).all()) for g in outs.values())
    m = torch.zeros((2, 4, 4), dtype=torch.uint8, device=DEV)
    for bad in (lambda: ops.mask_regions(m.float(), 5), lambda: ops.mask_regions(m, 0), lambda: ops.mask_regions(m, 5, 6),
                lambda: ops.region_table(m, m.int()[:1], 5), lambda: ops.region_table(m, m.int(), 5, max_regions=0),
                lambda: ops.region_table(m, m.int(), 5, conf=m.float()), lambda: ops.region_table(m, m.int(), 5, low=256),
                lambda: ops.region_filter(m, m.int(), torch.zeros((2, 4, 9), dtype=torch.int64, device=DEV), 5, 2),
                lambda: ops.region_filter(m, m.int(), torch.zeros((2, 4, 10), dtype=torch.int64, device=DEV), 5, -1)):
        with pytest.raises(RuntimeError):
            bad()
    assert ops.mask_regions(m[:0], 5).shape == (0, 4, 4) and ops.region_table(m[:0], m[:0].int(), 5)[0].shape == (0, 1024, 10)


def test_a_captured_graph_replayed_on_a_new_mask_gives_that_masks_result():
    case, conn, k = 4, 8, 5
    a, b = ref.expected(case, "random5", conn), ref.expected(case, "stripes", conn)
    conf, cap = dev(a["conf"]), a["cap"]
    mask = dev(a["mask"])
    n, h, w = mask.shape
    table = torch.full((n, cap, 10), -12345, dtype=torch.int64, device=DEV)          # never cleared by the caller
    counts = torch.full((n, 2), -12345, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    labels, index = (torch.empty((n, h, w), dtype=torch.int32, device=DEV) for _ in range(2))
    work = torch.empty((n, -(-h * w // ops.REGION_RANK_CHUNK)), dtype=torch.int32, device=DEV)
    votes = torch.empty((n, cap, k), dtype=torch.int32, device=DEV)
    out = torch.empty_like(mask)

    def run():
        s = stream_ptr()
        check(lib.fs_mask_regions(ptr(mask), n, h, w, k, conn, ptr(labels), s))
        check(lib.fs_region_table(ptr(mask), ptr(labels), ptr(conf), n, h, w, k, 100, cap, ptr(table), ptr(counts), ptr(index), ptr(work), s))
        check(lib.fs_region_filter(ptr(mask), ptr(index), ptr(table), n, h, w, k, cap, 9, ptr(out), ptr(votes), s))

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for e in (b, a, b):
        mask.copy_(dev(e["mask"]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(labels, dev(e["labels"])) and torch.equal(out, dev(e["filtered"][9]))
        assert all(torch.equal(g, dev(w)) for g, w in zip((table, counts, index), e["with_conf"]))


def test_full_frame_index_range_on_a_scene_known_in_closed_form():
    """(5, 1072 x 1920): 33.5 x 30 tiles per frame, labels up to 2 * 10^6, a serpentine through every tile row of the frame, 5361
    regions per frame.  The expected labels follow from the construction (regions_ref.lattice_scene): no host labelling."""
    m, want, regions = ref.lattice_scene()
    n, h, w = m.shape
    mask = dev(m)
    for conn in (4, 8):
        labels = ops.mask_regions(mask, 4, conn)
        assert torch.equal(labels, dev(want)), conn
    # the invariants, vectorised, on a scene with no closed form: the same frames with random ids sprinkled over them
    g = torch.Generator(device=DEV).manual_seed(5)
    noisy = torch.where(torch.rand(mask.shape, device=DEV, generator=g) < 0.4, torch.randint(0, 6, mask.shape, device=DEV, generator=g, dtype=torch.uint8), mask)
    for conn in (4, 8):
        lab = ops.mask_regions(noisy, 4, conn).long()
        own = torch.arange(h * w, device=DEV).view(1, h, w)
        fg = noisy < 4
        assert bool(((lab == 0) == ~fg).all()) and bool((lab - 1 <= own)[fg].all())
        flat_lab, flat_mask = lab.view(n, -1), noisy.view(n, -1)
        at = (flat_lab - 1).clamp(min=0)
        assert bool((torch.gather(flat_lab, 1, at) == flat_lab)[fg.view(n, -1)].all())                      # the anchor carries its own label
        assert bool((torch.gather(flat_mask, 1, at) == flat_mask)[fg.view(n, -1)].all())                    # ... and its pixels' class
        for dy, dx in ((0, 1), (1, 0)) + (((1, 1), (1, -1)) if conn == 8 else ()):
            pa = (slice(None), slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
            pb = (slice(None), slice(dy, h), slice(max(0, dx), w + min(0, dx)))
            same = fg[pa] & (noisy[pa] == noisy[pb])
            assert bool((lab[pa] == lab[pb])[same].all()), (conn, dy, dx)                                   # neighbours of one class: one label
    # the table of the closed-form scene: 80 x 67 rectangles of 150 pixels and the serpentine, in raster order
    labels = ops.mask_regions(mask, 4, 8)
    conf = torch.full_like(mask, 7)
    table, counts, index = ops.region_table(mask, labels, 4, conf, 8, 8192)
    assert counts.cpu().tolist() == [[regions, regions]] * n
    t = table.cpu().numpy()
    snake = int((want[0] == 1).sum())
    assert t[0, 0].tolist() == [3, snake, 0, 0, w - 1, h - 16, int(np.nonzero(want[0] == 1)[1].sum()), int(np.nonzero(want[0] == 1)[0].sum()), 7 * snake, snake]
    i, j = np.divmod(np.arange(regions - 1), w // 24)
    rect = t[:, 1:regions]
    assert (rect[..., 1] == 150).all() and (rect[..., 2] == j * 24 + 4).all() and (rect[..., 3] == i * 16 + 3).all()
    assert (rect[..., 4] == j * 24 + 18).all() and (rect[..., 5] == i * 16 + 12).all() and (rect[..., 8] == 1050).all() and (rect[..., 9] == 150).all()
    assert (rect[..., 6] == 150 * (j * 24 + 11)).all() and (2 * rect[..., 7] == 150 * (2 * (i * 16 + 3) + 9)).all()
    assert all((rect[f, :, 0] == (i + j + f) % 3).all() for f in range(n)) and not t[:, regions:].any()
    assert bool((index.view(n, -1)[:, 0] == 0).all()) and int(index.max()) == regions - 1 and bool(((index == -1) == (mask == 4)).all())
    # a cap below the count: the first rows, the full count, no row for the rest; the filter takes the rectangles out (9 < 150 <= 151)
    t2, c2, i2 = ops.region_table(mask, labels, 4, conf, 8, 1000)
    assert c2.cpu().tolist() == [[regions, 1000]] * n and torch.equal(t2, table[:, :1000]) and torch.equal(i2, torch.where(index < 1000, index, -1))
    assert torch.equal(ops.region_filter(mask, index, table, 4, 150), mask)
    gone = ops.region_filter(mask, index, table, 4, 151)
    assert torch.equal(gone, mask)                                                                          # bordered by background only: they stay


# ------------------------------------------------------------------------------------------------ one window, end to end
FH, FW, FRAMES, DELTA = 1072, 1920, 11, 5   # the grid estimator is built for 1072 / 1080 x 1920 frames; the network sees 65 x 65


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    frames = modes_ref.textured_frame(FH + 8 * FRAMES, FW, seed=51, channels=3)
    path = str(tmp_path_factory.mktemp("regions") / "clip.rgb")
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


def rows_of(masks, conf, conn=8, cap=1024, low=128):
    table, counts, _ = ref.region_table(masks, ref.mask_regions(masks, 5, conn), 5, conf, low, cap)
    return [table[f, :counts[f, 1]] for f in range(len(masks))], counts[:, 0]


@pytest.mark.parametrize("size,crop", [((65, 65), None), ((65, 97), (65, 65))])
def test_predictor_with_regions(clip, size, crop):
    item = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8)[1]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=crop, compute_metrics=True, cache_keyframes=False)
    args = (item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"])
    plain = FlowPredictor(fm, **kw).predict_window(*args, to_host=False)
    on = FlowPredictor(fm, regions=True, confidence=True, low_confidence=140, connectivity=4, **kw)
    masks, conf = on.predict_window(*args, to_host=False)
    assert torch.equal(masks, plain)                                          # regions alone: the default masks bit for bit
    m2, _ = next(iter(on.predict_clip([dict(item)], to_host=False)))
    assert torch.equal(m2, plain)
    rows, totals = on.region_report()
    want_rows, want_totals = rows_of(plain.cpu().numpy(), conf.cpu().numpy(), 4, 1024, 140)
    assert len(rows) == 2 * DELTA and np.array_equal(totals, np.concatenate([want_totals] * 2))
    assert all(np.array_equal(rows[f], want_rows[f % DELTA]) for f in range(2 * DELTA))
    assert sum(int(r[:, 1].sum()) for r in rows[:DELTA]) == DELTA * size[0] * size[1] or (totals > 1024).any()
    on.clear_report()
    assert on.region_report()[0] == [] and on.extent_report().shape == (0, 5, 3)
    # min_region_area: the emitted masks are the definition's filter of the default masks, and every consumer sees them
    flt = FlowPredictor(fm, regions=True, min_region_area=9, **kw)
    got = flt.predict_window(*args, to_host=False)
    p = plain.cpu().numpy()
    table, counts, index = ref.region_table(p, ref.mask_regions(p, 5, 8), 5, None, 128, 1024)
    want = ref.region_filter(p, index, table, 5, 9)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(flt.despeckle_counts(), counts[:, 0])
    rows, totals = flt.region_report()
    want_rows, want_totals = rows_of(want, None)
    assert np.array_equal(totals, want_totals) and all(np.array_equal(a, b) for a, b in zip(rows, want_rows))
    score = FlowPredictor(fm, **kw)                                            # the temporal-consistency score of the filtered masks
    score._score(got, DELTA)
    assert torch.equal(flt.hist, score.hist)
    assert torch.equal(next(iter(flt.predict_clip([dict(item)], to_host=False))), got)


def test_predict_video_writes_the_regions_csv(clip, tmp_path):
    """The command-line tool is what this test is about: one child process, --regions on the synthetic clip."""
    size, frames = (65, 65), (FRAMES - 1) // DELTA * DELTA
    csv, out = str(tmp_path / "r.csv"), str(tmp_path / "m.rgb")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "predict_video.py"), "--raw", clip, "--raw-size", str(FH), str(FW), "--pix-fmt", "rgb24",
           "--search", "8", "--synthetic-weights", "--no-cropping", "--size", "65", "65", "--no-metrics", "--raw-out", out, "--out-pix-fmt", "rgb24",
           "--regions", csv, "--connectivity", "4", "--max-regions", "6", "--min-region", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rgb = np.fromfile(out, np.uint8).reshape(frames, size[0], size[1], 3)     # opaque class colours: the (filtered) masks, through the palette
    onehot = np.stack([(rgb == PALETTE[k]).all(-1) for k in range(5)], 1)
    assert (onehot.sum(1) == 1).all()
    masks = onehot.argmax(1).astype(np.uint8)
    rows, totals = rows_of(masks, None, 4, 6)
    want = str(tmp_path / "want.csv")
    write_regions_csv(want, list(range(frames)), rows, with_confidence=False)
    assert open(csv).read() == open(want).read()
    for f, total in enumerate(totals.tolist()):
        assert (f"frame {f} has {total} regions" in r.stderr) == (total > 6)
    assert len(open(csv).read().splitlines()) == 1 + sum(len(x) for x in rows)
