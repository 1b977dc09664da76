"""Timing of the mosaic ops (profiles/r24_mosaic.txt): ops.global_motion, ops.pose_chain, ops.mosaic_accumulate -- the three a window
costs -- and ops.mosaic_resolve, the report's, on one 1072 x 1920 five-frame window and a 4096 x 4096 canvas with K = 5: a slow pan
(the frames' footprint is a fifth of the canvas) and a pose set that covers the whole canvas (every frame magnified four times).
Device events, medians of 20 groups of 5 back-to-back calls, eagerly through the Python wrappers and as a captured graph replayed; the
clock read before and after.  Next to mosaic_accumulate its byte floor: the mask bytes read plus 2 B read and 2 B written per touched
vote, at 8 TB/s.  Then the four per-merge calls of DESIGN §3.23 (ops.merge_view, ops.merge_gate, ops.link_correct, ops.mosaic_merge) on
two such canvases, B over a quarter of A and over all of it, each next to the bytes it must move.  Last ops.mosaic_change (DESIGN §3.24,
profiles/r31_change.txt) on the same two pairs at tolerance 0, 1, 3 and 8; `--change-only` runs that part alone.  Prints to stdout."""
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flood_uav_video_segmentation_amd import ops  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth
H, W, N, K = 1072, 1920, 5, 5
CANVAS = (4096, 4096)
ONE = ops.POSE_ONE
GROUP, SAMPLES = 5, 20    # one sample = GROUP back-to-back calls between two events


def say(s=""):
    print(s, flush=True)


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return " | ".join(l.strip() for l in r.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)) or "rocm-smi printed no GPU[0] clock"
    except Exception as e:  # noqa: BLE001
        return f"clock not read ({type(e).__name__})"


def sample(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(SAMPLES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(GROUP):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / GROUP)
    return statistics.median(ts), min(ts), max(ts)


def sample_graph(fn):
    """The same GROUP calls captured once and replayed: no Python and no enqueue between the launches."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GROUP):
            fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(SAMPLES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / GROUP)
    return statistics.median(ts)


def row(name, fn, moved=None):
    med, lo, hi = sample(fn)
    dev_us = sample_graph(fn)
    tail = "" if moved is None else f"{moved / 1e6:>10.1f}{moved / HBM_BYTES_PER_S * 1e6:>10.1f}{moved / HBM_BYTES_PER_S * 1e6 / dev_us:>12.3f}"
    say(f"{name:<58}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{dev_us:>10.1f}{tail}")


def pose_rows(scale, shifts):
    """Frame f: x_anchor = scale * x + shift (and its inverse), status ok."""
    rows = []
    for tx, ty in shifts:
        to = [int(scale * ONE), 0, int(tx * ONE), 0, int(scale * ONE), int(ty * ONE)]
        back = [int(ONE / scale), 0, int(-tx / scale * ONE), 0, int(ONE / scale), int(-ty / scale * ONE)]
        rows.append(to + back + [0, 0, 0, 0])
    return torch.tensor(rows, dtype=torch.int64, device="cuda")


def change_section():
    """ops.mosaic_change: the three launches of one call, B over a quarter of A and over all of it.  Votes of a blocky class
    map with 5 % noise on both sides, so that almost every pixel of a tile lands in one (ca, cb) cell, as on a real map.  MB moved:
    change_classes reads 2K B of A a pixel and 2K B of B a reached pixel and writes 2 B; change_codes reads 2 B and writes 1 B a pixel
    (the aprons are not counted)."""
    say()
    say(f"the change between two {CANVAS[0]} x {CANVAS[1]} mosaics, K = {K}: the link is registered and exact; origins (0, 0); min_votes 1, min_conf 0, watch (1,)")
    say(f"{'call':<58}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")

    def votes_of(size, seed):
        r = np.random.RandomState(seed)
        cls = np.kron(r.randint(0, K, (size[0] // 32 + 1, size[1] // 32 + 1)), np.ones((32, 32), np.int64))[:size[0], :size[1]]
        cls = np.where(r.rand(*size) < 0.05, r.randint(0, K, size), cls)
        v = r.randint(0, 3, size=(K,) + tuple(size)).astype(np.int16)
        v[cls, np.arange(size[0])[:, None], np.arange(size[1])[None, :]] += 20
        return torch.from_numpy(v).cuda().view(torch.uint16)

    votes_a = votes_of(CANVAS, 2)
    pixels = CANVAS[0] * CANVAS[1]
    for name, (bh, bw), (ty, tx) in (("B over a quarter of A", (CANVAS[0] // 2, CANVAS[1] // 2), (CANVAS[0] // 4, CANVAS[1] // 4)), ("B over all of A", CANVAS, (0, 0))):
        votes_b = votes_of((bh, bw), 3)
        link = ops.mosaic_link([ONE, 0, tx * ONE, 0, ONE, ty * ONE], [ONE, 0, -tx * ONE, 0, ONE, -ty * ONE], ops.LINK_REGISTERED, "cuda")
        moved = 2 * K * pixels + 2 * K * bh * bw + 2 * pixels + 3 * pixels
        for r in (0, 1, 3, 8):
            row(f"mosaic_change, tolerance {r}, {name}", lambda: ops.mosaic_change(votes_a, (0, 0), votes_b, (0, 0), link, 1, 0, r, (1,)), moved)
        counts = ops.mosaic_change(votes_a, (0, 0), votes_b, (0, 0), link, 1, 0, 1, (1,))[4].cpu().numpy()
        say(f"  (counts at tolerance 1: {counts.tolist()}; eager includes the wrapper's five output allocations)")


torch.set_grad_enabled(False)
if "--change-only" in sys.argv[1:]:
    say(f"clock before: {clocks()}")
    change_section()
    say(f"clock after: {clocks()}")
    sys.exit(0)
rng = np.random.RandomState(0)
base = np.kron(rng.randint(0, 5, (H // 16 + 2, W // 16 + 2)), np.ones((16, 16), np.int64))
frames = np.stack([base[f:f + H, 2 * f:2 * f + W] for f in range(N)])
flip = rng.rand(N, H, W) < 0.05                                               # a segmenter's blobs moving (1, 2) pixels a frame, 5 % noise
mask = torch.from_numpy(np.where(flip, rng.randint(0, 5, (N, H, W)), frames).astype(np.uint8)).cuda()

# ---- the tables of a slow pan with a slight rotation and zoom, a quarter of the rows replaced by random vectors
hb, wb = H // 16, W // 16
by, bx = np.meshgrid(np.arange(hb), np.arange(wb), indexing="ij")
cx, cy = (bx * 16 + 8).reshape(-1), (by * 16 + 8).reshape(-1)
c, s = 1.002 * np.cos(np.radians(0.2)), 1.002 * np.sin(np.radians(0.2))
tables = np.empty((N, hb * wb, 7), np.int32)
tables[:, :, 0], tables[:, :, 1], tables[:, :, 2] = -1, 16, 16
tables[:, :, 5], tables[:, :, 6] = cx, cy
for f in range(N):
    dx = np.rint(c * (cx - W / 2) - s * (cy - H / 2) + W / 2 + 2 - cx).astype(np.int64)
    dy = np.rint(s * (cx - W / 2) + c * (cy - H / 2) + H / 2 + 1 - cy).astype(np.int64)
    wild = rng.rand(hb * wb) < 0.25
    tables[f, :, 3] = cx + np.where(wild, rng.randint(-32, 33, hb * wb), dx)
    tables[f, :, 4] = cy + np.where(wild, rng.randint(-32, 33, hb * wb), dy)
tables = torch.from_numpy(tables).cuda()
origin = ((CANVAS[0] - H) // 2, (CANVAS[1] - W) // 2)

say(f"clock before: {clocks()}")
say(f"one {H} x {W} window of {N} frames, canvas {CANVAS[0]} x {CANVAS[1]}, K = {K}; medians of {SAMPLES} groups of {GROUP} calls (min .. max)")
say(f"{'call':<58}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")
for rounds in (0, 4):
    for with_mask in (False, True):
        kw = dict(mask=mask, exclude=(1,)) if with_mask else {}
        row(f"global_motion, rounds = {rounds}, {'exclusion mask' if with_mask else 'no mask'}",
            lambda: ops.global_motion(tables, (H, W), (H, W), rounds, 1.0, 12, **kw), N * hb * wb * 28 * (1 + rounds))
model = ops.global_motion(tables, (H, W), (H, W), 4, 1.0, 12, mask=mask, exclude=(1,))
host_model = model.cpu().numpy()
say(f"  (the fits: status {host_model[:, 12].tolist()}, usable {host_model[:, 13].tolist()}, inliers {host_model[:, 14].tolist()}, rounds "
    f"{host_model[:, 15].tolist()}; MB moved = the table once for the histogram and once per round)")
state = torch.zeros((32,), dtype=torch.int64, device="cuda")
row("pose_chain, 5 frames", lambda: ops.pose_chain(model, state, (H, W), CANVAS, origin))
for name, poses in (("slow pan (3, 2) px a frame", pose_rows(1.0, [(3 * f, 2 * f) for f in range(N)])),
                    ("whole canvas (frames magnified 4 x)", pose_rows(4.0, [(-origin[1] - 8 * f, -origin[0] - 8 * f) for f in range(N)]))):
    votes = torch.zeros((K,) + CANVAS, dtype=torch.int16, device="cuda").view(torch.uint16)
    ops.mosaic_accumulate(mask, poses, votes, origin)
    lit = votes.view(torch.int16) != 0                                     # the same bits: comparisons exist for the signed type
    touched, seen = int(lit.sum()), int(lit.any(0).sum())                  # the votes one call reads and writes; the canvas pixels under them
    moved = N * H * W + 4 * touched
    row(f"mosaic_accumulate, {name}", lambda: ops.mosaic_accumulate(mask, poses, votes, origin), moved)
    say(f"  ({seen} canvas pixels seen, {touched} votes touched per call; floor = {N * H * W / 1e6:.1f} MB of masks + 4 B per touched vote, at 8.0 TB/s)")
    pixels = CANVAS[0] * CANVAS[1]
    row("mosaic_resolve after it", lambda: ops.mosaic_resolve(votes), pixels * (2 * K + 1 + 1 + 4))
say("(mosaic_resolve: per canvas pixel 2 B of votes per class read, cls, conf and seen written.  eager: through the Python wrapper, its output")
say(" allocations and the enqueue included; graph: GROUP such calls captured and replayed, per call.)")

# ---- the four calls a merge costs: A and B cut from one random texture, so the fit is a real one (the identity)
say()
say(f"merging two {CANVAS[0]} x {CANVAS[1]}-class mosaics, K = {K}: the link is registered and exact; origins (0, 0)")
say(f"{'call':<58}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")
ground = torch.from_numpy(rng.randint(0, 1 << 24, size=CANVAS).astype(np.int32)).cuda() | (0xFF << 24) - (1 << 32)   # alpha 255: seen everywhere
votes_a = torch.from_numpy(rng.randint(0, 40, size=(K,) + CANVAS).astype(np.int16)).cuda().view(torch.uint16)
rank_a = torch.from_numpy(rng.randint(0, 1 << 40, size=CANVAS)).cuda()
for name, (bh, bw), (ty, tx) in (("B over a quarter of A", (CANVAS[0] // 2, CANVAS[1] // 2), (CANVAS[0] // 4, CANVAS[1] // 4)), ("B over all of A", CANVAS, (0, 0))):
    rgba_b = ground[ty:ty + bh, tx:tx + bw].clone()   # a copy: the whole-canvas crop would be A's own memory, which the ops refuse
    votes_b = torch.from_numpy(rng.randint(0, 40, size=(K, bh, bw)).astype(np.int16)).cuda().view(torch.uint16)
    rank_b = torch.from_numpy(rng.randint(0, 1 << 40, size=(bh, bw))).cuda()
    link = ops.mosaic_link([ONE, 0, tx * ONE, 0, ONE, ty * ONE], [ONE, 0, -tx * ONE, 0, ONE, -ty * ONE], ops.LINK_REGISTERED, "cuda")
    window, reached, pixels = (0, 0) + CANVAS, bh * bw, CANVAS[0] * CANVAS[1]
    row(f"merge_view, {name}", lambda: ops.merge_view(ground, (0, 0), rgba_b, (0, 0), link, window), 4 * pixels + 4 * reached + 4 * pixels)
    cur, view, valid_a, valid_b = ops.merge_view(ground, (0, 0), rgba_b, (0, 0), link, window)
    table, stats = ops.block_match_modes(cur, view, 16, 0, 0, return_stats=True)
    blocks = table.shape[0]
    row(f"merge_gate, {blocks} rows", lambda: ops.merge_gate(table, valid_a, valid_b), blocks * (28 + 512))
    fit = ops.global_motion(table[None], CANVAS, CANVAS, 4, 1.0, 12, pair_stats=stats[None])
    scratch = link.clone()
    row("link_correct (with a 128-byte copy of the link in front)", lambda: ops.link_correct(fit, scratch.copy_(link), window, (0, 0)))
    host_fit, kept = fit.cpu().numpy()[0], int((table[:, 3] >= 0).sum())
    say(f"  (the fit: status {host_fit[12]}, usable {host_fit[13]}, inliers {host_fit[14]}, shift {host_fit[2] / ONE:.3f}, {host_fit[5] / ONE:.3f} px; {kept} rows survive the gate)")
    va, ra, ca = votes_a.clone(), rank_a.clone(), ground.clone()
    row(f"mosaic_merge, votes only, {name}", lambda: ops.mosaic_merge(va, (0, 0), votes_b, (0, 0), link), reached * 2 * K * 3)
    row(f"mosaic_merge with the orthophoto, {name}", lambda: ops.mosaic_merge(va, (0, 0), votes_b, (0, 0), link, (ra, ca), (rank_b, rgba_b), 7, "centre"),
        reached * (2 * K * 3 + 16))
    counts = ops.mosaic_merge(va, (0, 0), votes_b, (0, 0), link, (ra, ca), (rank_b, rgba_b), 7, "centre").cpu().numpy()
    say(f"  (counts {counts[:5].tolist()}; MB moved: 2 B of B and 2 + 2 B of A per class and reached pixel, + the two rank words; repeated calls saturate")
    say("   the votes but read and write the same cells; the orthophoto takes its pixels in the FIRST call only: the 12 B written per pixel won are not in these times)")
change_section()
say(f"clock after: {clocks()}")
