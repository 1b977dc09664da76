"""FlowPredictor with every analysis stage on at once, without a GPU: a stub flow model, every op replaced by its numpy definition from
tests/*_ref.py, chunk sizes small enough that every set of report buffers crosses a chunk border inside a window.  Public API only:
the masks handed out and every *_report() against the definitions applied frame by frame, across reset() and clear_report(), and the
sequence of op calls of every window."""
import numpy as np
import torch

import conf_ref
import distance_ref as dref
import mosaic_ref as mref
import outlines_ref as oref
import regions_ref as rref
import simplify_ref as sref
import stabilize_ref as stref
import tracks_mc_ref as mc
import tracks_ref as tref
from flood_uav_video_segmentation_amd import ops
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

K, HW, FSIZE, N = 3, (6, 8), (32, 48), 3                                      # classes, mask size, decoded frame size, frames per window
CONN, CAP, MIN_AREA, LOW = 4, 20, 3, 128
PAIRS, OVERLAP = 64, 2
CONTOURS, VERTICES, TOL, ROUNDS = 6, 200, 0.5, 3
PERSIST, TRUST = 2, 200
THRESHOLDS, SOURCES, TARGETS = (1, 3), (1,), (0, 2)
CANVAS, INLIERS = (12, 16), 3
ORIGIN = ((CANVAS[0] - HW[0]) // 2, (CANVAS[1] - HW[1]) // 2)
WINDOWS = 5


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bits(ids):
    return mref.exclude_bits(ids)


def window_logits(w):
    """Smooth logits plus noise, so that regions persist from frame to frame and speckles and flicker occur."""
    base = torch.randn((1, K) + HW, generator=torch.Generator().manual_seed(7)) * 2
    return base + torch.randn((N, K) + HW, generator=torch.Generator().manual_seed(100 + w)) * 0.9


class StubFlow(torch.nn.Module):
    """A flow model that returns fixed logits [n,K,H,W] (a foreign network: no fused routes)."""
    feature_based = True
    no_warp = True

    def __init__(self):
        super().__init__()
        self.calls = 0

    def predict(self, frame_prev, frame_next, mvs_left, mvs_right, n, profiler=None, **extra):
        self.calls += 1
        return {"pred": window_logits(self.calls - 1)}


def numpy_ops(monkeypatch, called):
    """Every op the stages call, as the numpy definition on CPU tensors; `called` records (name, frames) in call order."""
    def fill(out, got):
        for dst, src in zip(out, got):
            dst.copy_(t(src))
        return out

    def mask_confidence(logits, size=None):
        called.append(("mask_confidence", logits.shape[0]))
        return tuple(t(a) for a in conf_ref.mask_confidence(logits.numpy(), size))

    def frame_report(mask, conf=None, classes=5, low=128, out=None):
        called.append(("frame_report", mask.shape[0]))
        return out.copy_(t(conf_ref.frame_report(mask.numpy(), conf.numpy(), classes, low)))

    def mask_stabilize(mask, state=None, conf=None, classes=5, persist=3, trust=None, mv=None, frame_size=None, pair_stats=None):
        called.append(("mask_stabilize", mask.shape[0]))
        out, st, counts = stref.mask_stabilize(mask.numpy(), None if state is None else state.numpy(), None if conf is None else conf.numpy(), classes, persist,
                                               trust, mv.numpy(), frame_size, None if pair_stats is None else pair_stats.numpy())
        return t(out), t(st.view(np.int32)), t(counts)

    def mask_regions(mask, classes, connectivity=8):
        called.append(("mask_regions", mask.shape[0]))
        return t(rref.mask_regions(mask.numpy(), classes, connectivity))

    def region_table(mask, labels, classes, conf=None, low=128, max_regions=1024, out=None):
        called.append(("region_table", mask.shape[0]))
        got = rref.region_table(mask.numpy(), labels.numpy(), classes, None if conf is None else conf.numpy(), low, max_regions)
        if out is None:
            return t(got[0]), t(got[1]), t(got[2])
        fill(out, got[:2])
        return out[0], out[1], t(got[2])

    def region_filter(mask, index, table, classes, min_area):
        called.append(("region_filter", mask.shape[0]))
        return t(rref.region_filter(mask.numpy(), index.numpy(), table.numpy(), classes, min_area))

    def region_links(index, table, counts, prev=None, max_pairs=None, min_overlap=1, mv=None, frame_size=None, pair_stats=None):
        called.append(("region_links", index.shape[0]))
        p = None if prev is None else tuple(x.numpy() for x in prev)
        return tuple(t(a) for a in mc.region_links_mc(index.numpy(), table.numpy(), counts.numpy(), mv.numpy(), frame_size, p,
                                                      None if pair_stats is None else pair_stats.numpy(), max_pairs, min_overlap))

    def region_tracks(back, fwd, counts, state, prev_tracks=None, out=None):
        called.append(("region_tracks", back.shape[0]))
        got, new = tref.region_tracks(back.numpy(), fwd.numpy(), counts.numpy(), state.numpy(), None if prev_tracks is None else prev_tracks.numpy())
        state.copy_(t(new))
        return out.copy_(t(got))

    def region_outlines(index, max_regions, connectivity=8, max_contours=4096, max_vertices=32768, out=None):
        called.append(("region_outlines", index.shape[0]))
        return fill(out, oref.region_outlines(index.numpy(), max_regions, connectivity, max_contours, max_vertices))

    def outline_simplify(contours, vertices, counts, tolerance, max_rounds=32, out=None):
        called.append(("outline_simplify", contours.shape[0]))
        return fill(out, sref.outline_simplify(contours.numpy(), vertices.numpy(), counts.numpy(), ops.simplify_tol_q(tolerance), max_rounds))

    def mask_distance(mask, sources, max_dist=0, want_nearest=True, out=None):
        called.append(("mask_distance", mask.shape[0]))
        d2, nearest = dref.mask_distance(mask.numpy(), bits(sources), max_dist)
        return t(d2.view(np.int32)), t(nearest)

    def region_proximity(mask, d2, nearest, index, counts, classes, max_regions, targets, thresholds, out=None):
        called.append(("region_proximity", mask.shape[0]))
        return fill(out, dref.region_proximity(mask.numpy(), d2.numpy().view(np.uint32), nearest.numpy(), index.numpy(), counts.numpy(), classes, max_regions,
                                               bits(targets), thresholds))

    def global_motion(tables, frame_size, mask_size, rounds=4, tol=1.0, min_inliers=12, mask=None, exclude=(), pair_stats=None):
        called.append(("global_motion", tables.shape[0]))
        return t(mref.global_motion(tables.numpy(), frame_size, mask_size, rounds, mref.tol_q20(tol), min_inliers, mask.numpy(), bits(exclude),
                                    None if pair_stats is None else pair_stats.numpy()))

    def pose_chain(model, state, mask_size, canvas_size, origin, max_bridge=2):
        called.append(("pose_chain", model.shape[0]))
        poses, after = mref.pose_chain(model.numpy(), state.numpy(), mask_size, canvas_size, origin, max_bridge)
        state.copy_(t(after))
        return t(poses)

    def mosaic_accumulate(mask, poses, votes, origin):
        called.append(("mosaic_accumulate", mask.shape[0]))
        mref.mosaic_accumulate(mask.numpy(), poses.numpy(), votes.view(torch.int16).numpy().view(np.uint16), origin)   # in place
        return votes

    def mosaic_resolve(votes):
        called.append(("mosaic_resolve", 0))
        cls, conf, seen, totals = mref.mosaic_resolve(votes.view(torch.int16).numpy().view(np.uint16))
        return t(cls), t(conf), t(seen.astype(np.int32)), t(totals)

    for fn in (mask_confidence, frame_report, mask_stabilize, mask_regions, region_table, region_filter, region_links, region_tracks, region_outlines,
               outline_simplify, mask_distance, region_proximity, global_motion, pose_chain, mosaic_accumulate, mosaic_resolve):
        monkeypatch.setattr(ops, fn.__name__, fn)


def definitions(mvs, stats, resets):
    """Per frame of the whole run, by the definitions alone and one frame at a time (no chunks, no windows): the mask handed out and
    every per-frame row a report can hold.  `resets`: the frames in front of which reset() was called."""
    frames, state = [], None
    for f in range(WINDOWS * N):
        logits = window_logits(f // N).numpy()[f % N:f % N + 1]
        raw, conf = conf_ref.mask_confidence(logits, HW)
        state = None if f in resets else state
        held, state, debounce = stref.mask_stabilize(raw, state, conf, K, PERSIST, TRUST, mvs[f:f + 1], FSIZE, stats[f:f + 1])
        table, counts, index = rref.region_table(held, rref.mask_regions(held, K, CONN), K, None, LOW, CAP)
        mask = rref.region_filter(held, index, table, K, MIN_AREA)
        speckled = int(counts[0, 0])
        table, counts, index = rref.region_table(mask, rref.mask_regions(mask, K, CONN), K, conf, LOW, CAP)
        rows = int(counts[0, 1])
        contours, vertices, shape, ocounts = oref.region_outlines(index, CAP, CONN, CONTOURS, VERTICES)
        simple, simple_vertices, scounts = sref.outline_simplify(contours, vertices, ocounts, ops.simplify_tol_q(TOL), ROUNDS)
        d2, nearest = dref.mask_distance(mask, bits(SOURCES), 0)
        exposure, near = dref.region_proximity(mask, d2, nearest, index, counts, K, CAP, bits(TARGETS), THRESHOLDS)
        vertices_kept = 0 if ocounts[0, 3] & 1 else int(ocounts[0, 2])
        frames.append(dict(
            mask=mask[0], conf=conf[0], debounce=debounce[0], speckled=speckled, extent=conf_ref.frame_report(mask, conf, K, LOW)[0],
            table=table[0], counts=counts[0], index=index[0], rows=table[0, :rows], total=int(counts[0, 0]),
            outline=(contours[0, :int(ocounts[0, 1])], vertices[0, :vertices_kept], shape[0, :rows]), outline_flags=int(ocounts[0, 3]),
            simple=(simple[0, :int(scounts[0, 0])], simple_vertices[0, :int(scounts[0, 1])]), simple_counts=scounts[0],
            exposure=exposure[0], near=near[0, :rows]))
    masks = np.stack([fr["mask"] for fr in frames])
    tracks, flags = mc.clip_tracks(masks, K, CONN, CAP, mvs, FSIZE, PAIRS, OVERLAP, resets=resets, stats=stats)
    for fr, rows, flag in zip(frames, tracks, flags):
        fr["tracks"], fr["track_flags"] = rows, int(flag)
    return frames


def mosaic_of(frames, mvs, stats, span):
    """mosaic_report() of the frames span = (first, last + 1) by the definitions: the anchor is the first of them."""
    s = slice(*span)
    masks = np.stack([fr["mask"] for fr in frames[s]])
    model = mref.global_motion(mvs[s], FSIZE, HW, 4, mref.tol_q20(1.0), INLIERS, masks, 0, stats[s])
    poses, _ = mref.pose_chain(model, np.zeros(32, np.int64), HW, CANVAS, ORIGIN, 2)
    cls, conf, seen, totals = mref.mosaic_resolve(mref.mosaic_accumulate(masks, poses, np.zeros((K,) + CANVAS, np.uint16), ORIGIN))
    return cls, conf, seen.astype(np.int32), totals, poses


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and np.array_equal(got, want)


def check_reports(p, frames, span, mosaic):
    """Every report of predictor p against the frames span = (first, last + 1) of the definitions."""
    want = frames[slice(*span)]
    count = len(want)
    assert same(p.extent_report(), np.stack([fr["extent"] for fr in want]))
    assert same(p.stabilize_report(), np.stack([fr["debounce"] for fr in want]))
    assert same(p.despeckle_counts(), np.array([fr["speckled"] for fr in want], np.int64))
    rows, totals = p.region_report()
    assert len(rows) == count and all(same(g, fr["rows"]) for g, fr in zip(rows, want)) and same(totals, np.array([fr["total"] for fr in want], np.int64))
    tracks, overflowed, cuts = p.track_report(with_cuts=True)
    assert len(tracks) == count and all(same(g, fr["tracks"]) for g, fr in zip(tracks, want))
    assert same(overflowed, np.array([fr["track_flags"] & 1 for fr in want], np.int64)) and same(cuts, np.array([fr["track_flags"] >> 1 for fr in want], np.int64))
    assert len(p.track_report()) == 2 and same(p.track_report()[1], overflowed)
    outlines, flags = p.outline_report()
    assert len(outlines) == count and all(same(a, b) for g, fr in zip(outlines, want) for a, b in zip(g, fr["outline"]))
    assert same(flags, np.array([fr["outline_flags"] for fr in want], np.int64))
    simple, counts = p.simple_outline_report()
    assert len(simple) == count and all(same(a, b) for g, fr in zip(simple, want) for a, b in zip(g, fr["simple"]))
    assert same(counts, np.stack([fr["simple_counts"] for fr in want]))
    exposure, near = p.proximity_report()
    assert same(exposure, np.stack([fr["exposure"] for fr in want])) and len(near) == count and all(same(g, fr["near"]) for g, fr in zip(near, want))
    got = p.mosaic_report()
    assert len(got) == 5 and all(same(g, w) for g, w in zip(got, mosaic))
    newest = p.window_regions()                                               # the newest window's frames: whole rows, on the "device"
    assert len(newest) == N
    for (index, table, counts, track_rows), fr in zip(newest, want[-N:]):
        assert same(index.numpy(), fr["index"]) and same(table.numpy(), fr["table"]) and same(counts.numpy(), fr["counts"])
        assert track_rows.shape == (CAP, 4) and same(track_rows.numpy()[:len(fr["tracks"])], fr["tracks"])


def pieces(first, n, chunk):
    """The runs that n frames, the first of them frame `first` of its buffers, are cut into by chunks of `chunk` frames."""
    out, done = [], 0
    while done < n:
        out.append(min(n - done, chunk - (first + done) % chunk))
        done += out[-1]
    return out


def window_calls(first, report_chunk, outline_chunk, simple_chunk):
    """The op calls of one window whose first frame is frame `first` since clear_report(), in order, as (name, frames)."""
    calls = [("mask_confidence", N), ("mask_stabilize", N), ("mask_regions", N), ("region_table", N), ("region_filter", N), ("mask_regions", N)]
    outlined = simplified = first
    for take in pieces(first, N, report_chunk):
        calls.append(("region_table", take))
        for o in pieces(outlined, take, outline_chunk):
            calls.append(("region_outlines", o))
            calls += [("outline_simplify", s) for s in pieces(simplified, o, simple_chunk)]
            simplified += o
        outlined += take
        calls += [("region_links", take), ("region_tracks", take), ("mask_distance", take), ("region_proximity", take)]
    calls += [("global_motion", N), ("pose_chain", N), ("mosaic_accumulate", N)]
    return calls + [("frame_report", take) for take in pieces(first, N, report_chunk)]


def test_every_stage_at_once_across_chunk_borders_reset_and_clear(monkeypatch):
    """Three windows, reset(), one window, clear_report(), one window: REPORT_CHUNK = 4, outline_chunk = 3 and simple_chunk = 2 cut the
    three-frame windows at different frames for the extent / region / track / proximity / stabiliser / mosaic rows, the outlines and the
    simplified rings.  At each stop every report is the definitions' of the masks handed out; reset() restarts the stabiliser and the
    tracks' links and keeps every report and the mosaic; clear_report() drops the reports and the mosaic and keeps the stabiliser's
    state, the previous frame and the track ids.  Every window enqueues the same ops in the same order, cut at the chunk borders."""
    called = []
    numpy_ops(monkeypatch, called)
    monkeypatch.setattr(FlowPredictor, "REPORT_CHUNK", 4)
    p = FlowPredictor(StubFlow(), classes=K, out_size=HW, crop=None, compute_metrics=False, confidence=True, low_confidence=LOW, regions=True,
                      min_region_area=MIN_AREA, connectivity=CONN, max_regions=CAP, track=True, min_overlap=OVERLAP, max_pairs=PAIRS, compensate=True,
                      outlines=True, max_contours=CONTOURS, max_vertices=VERTICES, simplify=TOL, simplify_rounds=ROUNDS, keep_window_regions=True,
                      stabilize=PERSIST, stabilize_trust=TRUST, stabilize_compensate=True, proximity=THRESHOLDS, proximity_sources=SOURCES,
                      proximity_targets=TARGETS, mosaic=CANVAS, mosaic_min_inliers=INLIERS, mosaic_exclude=())
    p.outline_chunk, p.simple_chunk = 3, 2
    rng = np.random.default_rng(5)
    mvs = np.stack([mc._rows(FSIZE[0], FSIZE[1], int(vx), int(vy)) for vx, vy in rng.integers(-6, 7, (WINDOWS * N, 2))])
    stats = np.zeros((WINDOWS * N, 4), np.int32)
    stats[:, 0] = 6
    stats[[7, 13], 2] = 1                                                     # scene cuts inside the third and the last window
    frames = definitions(mvs, stats, resets=(9,))
    x, grids = torch.zeros(1, 3, *HW), [None] * (N - 1)

    def window(w, first):
        """Window w, whose first frame is frame `first` of the report buffers."""
        s = slice(N * w, N * w + N)
        del called[:]
        masks, conf = p.predict_window(x, x, grids, grids, link_mvs=t(mvs[s]), link_frame_size=FSIZE, link_stats=t(stats[s]))
        assert called == window_calls(first, 4, 3, 2), w
        assert same(masks, np.stack([fr["mask"] for fr in frames[s]])) and same(conf, np.stack([fr["conf"] for fr in frames[s]])), w

    for w in range(3):
        window(w, N * w)
    check_reports(p, frames, (0, 9), mosaic_of(frames, mvs, stats, (0, 9)))
    assert any(fr["speckled"] != fr["total"] for fr in frames) and any(fr["debounce"][0] for fr in frames)        # the despeckle and the debounce do act
    assert any(len(fr["outline"][1]) != len(fr["simple"][1]) for fr in frames) and sum(int((fr["tracks"][:, 2] >= 0).sum()) for fr in frames) > 5
    p.reset()
    window(3, 9)
    check_reports(p, frames, (0, 12), mosaic_of(frames, mvs, stats, (0, 12)))
    assert frames[9]["debounce"][2] == HW[0] * HW[1] and (frames[9]["tracks"][:, 1:3] == -1).all()                  # frame 9 seeds, and its regions are born
    p.clear_report()
    assert p.extent_report().shape == (0, K, 3) and p.region_report()[0] == [] and p.track_report()[0] == [] and p.outline_report()[0] == []
    assert p.simple_outline_report()[0] == [] and p.stabilize_report().shape == (0, 4) and p.proximity_report()[1] == [] and p.despeckle_counts().shape == (0,)
    assert p.mosaic_report()[4].shape == (0, 16) and not p.mosaic_report()[2].any()
    window(4, 0)
    check_reports(p, frames, (12, 15), mosaic_of(frames, mvs, stats, (12, 15)))
    assert frames[12]["debounce"][2] < HW[0] * HW[1] // 2 and (frames[12]["tracks"][:, 2] >= 0).any()    # the state and the previous frame survived
    ok = [int(row[12]) for row in mosaic_of(frames, mvs, stats, (0, 12))[4]]
    assert ok[:7] == [0] * 7 and ok[7:] == [2] * 5                            # registered up to the cut, lost behind it
