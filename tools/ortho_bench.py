"""Timing of the orthophoto ops (profiles/r25_ortho.txt): ops.ortho_accumulate beside ops.mosaic_accumulate and ops.ortho_compose beside
ops.mosaic_resolve in the SAME run, on tools/mosaic_bench.py's scenario: one 1072 x 1920 five-frame window and a 4096 x 4096 canvas with
K = 5, a slow pan (the frames' footprint is a fifth of the canvas) and a pose set that covers the whole canvas (every frame magnified four
times).  Device events, medians of 20 groups of 5 back-to-back calls, eagerly through the Python wrappers and as a captured graph
replayed; the clock read before and after.  ortho_accumulate is measured per window (its five calls) in two states: on a FRESH canvas
(the canvas's reset is inside the timed group and is also timed alone), where the winners fetch their taps and store 12 B, and on a canvas
that already holds the window (every pixel loses: 8 B read).  Next to each its byte floor at 8 TB/s: 8 B per footprint pixel, plus 12 B
and the taps' bytes per winner; compose: 4 + 1 B read and 3 B written per canvas pixel.  Prints to stdout."""
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
    say(f"{name:<66}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{dev_us:>10.1f}{tail}")
    return dev_us


def pose_rows(scale, shifts):
    """Frame f: x_anchor = scale * x + shift (and its inverse), status ok."""
    rows = []
    for tx, ty in shifts:
        to = [int(scale * ONE), 0, int(tx * ONE), 0, int(scale * ONE), int(ty * ONE)]
        back = [int(ONE / scale), 0, int(-tx / scale * ONE), 0, int(ONE / scale), int(-ty / scale * ONE)]
        rows.append(to + back + [0, 0, 0, 0])
    return torch.tensor(rows, dtype=torch.int64, device="cuda")


torch.set_grad_enabled(False)
rng = np.random.RandomState(0)
base = np.kron(rng.randint(0, 5, (H // 16 + 2, W // 16 + 2)), np.ones((16, 16), np.int64))
mask = torch.from_numpy(np.stack([base[f:f + H, 2 * f:2 * f + W] for f in range(N)]).astype(np.uint8)).cuda()
# the decoded frames: RGB24 at the mask's size (one tap a winner), and RGB24 at twice the size (four taps)
same = [(torch.from_numpy(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).cuda(), None, "rgb24", "bt709", False) for _ in range(N)]
twice = [(torch.from_numpy(rng.randint(0, 256, (2 * H, 2 * W, 3)).astype(np.uint8)).cuda(), None, "rgb24", "bt709", False) for _ in range(N)]
origin = ((CANVAS[0] - H) // 2, (CANVAS[1] - W) // 2)
pixels = CANVAS[0] * CANVAS[1]
palette = np.array([[0, 0, 0], [30, 95, 170], [65, 117, 5], [212, 98, 1], [255, 244, 116]], np.uint8)

say(f"clock before: {clocks()}")
say(f"one {H} x {W} window of {N} frames, canvas {CANVAS[0]} x {CANVAS[1]}, K = {K}; medians of {SAMPLES} groups of {GROUP} calls (min .. max)")
say(f"{'call':<66}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")
for name, poses in (("slow pan (3, 2) px a frame", pose_rows(1.0, [(3 * f, 2 * f) for f in range(N)])),
                    ("whole canvas (frames magnified 4 x)", pose_rows(4.0, [(-origin[1] - 8 * f, -origin[0] - 8 * f) for f in range(N)]))):
    say(f"---- {name}")
    votes = torch.zeros((K,) + CANVAS, dtype=torch.int16, device="cuda").view(torch.uint16)
    ops.mosaic_accumulate(mask, poses, votes, origin)
    lit = votes.view(torch.int16) != 0
    touched = int(lit.sum())
    row("mosaic_accumulate, the window (one call)", lambda: ops.mosaic_accumulate(mask, poses, votes, origin), N * H * W + 4 * touched)
    for mode in ("centre", "latest"):
        for label, sources, tap_bytes in (("frames at the mask's size", same, 3), ("frames at twice the size", twice, 12)):
            rank, rgba = ops.ortho_canvas(CANVAS, "cuda")
            footprint = winners = 0                                         # counted once, eagerly: the pixels each call reads, and those it wins
            for f in range(N):
                before = rank.clone()
                ops.ortho_accumulate(sources[f], poses[f], f, (H, W), rank, rgba, origin, mode)
                winners += int((rank != before).sum())
                alone = ops.ortho_canvas(CANVAS, "cuda")
                ops.ortho_accumulate(sources[f], poses[f], f, (H, W), *alone, origin, mode)
                footprint += int((alone[0] != -1).sum())

            def window():
                for f in range(N):
                    ops.ortho_accumulate(sources[f], poses[f], f, (H, W), rank, rgba, origin, mode)

            def fresh_window():
                rank.fill_(-1)
                window()

            t_fresh = row(f"ortho_accumulate {mode}, {label}: fresh canvas + 5 calls", fresh_window, 8 * pixels + 8 * footprint + (12 + tap_bytes) * winners)
            t_full = row(f"ortho_accumulate {mode}, {label}: 5 calls, all lose", window, 8 * footprint)
            say(f"  ({footprint} footprint pixels, {winners} winners per window; per frame {t_fresh / N:.1f} us with the reset, {t_full / N:.1f} us where all lose)")
    row("the canvas's reset alone (rank.fill_(-1))", lambda: rank.fill_(-1), 8 * pixels)
    window()
    cls = ops.mosaic_resolve(votes)[0]
    row("mosaic_resolve", lambda: ops.mosaic_resolve(votes), pixels * (2 * K + 1 + 1 + 4))
    row("ortho_compose, extent map over it", lambda: ops.ortho_compose(rgba, cls, palette, alpha=96), pixels * 8)
    row("ortho_compose, with the edge line of class 1", lambda: ops.ortho_compose(rgba, cls, palette, alpha=96, edge=(1,)), pixels * 8)
    row("ortho_compose, plain", lambda: ops.ortho_compose(rgba, None, palette, alpha=96), pixels * 7)
say("(floors at 8.0 TB/s.  ortho_accumulate: 8 B of rank per footprint pixel, + 12 B stored and the taps' bytes -- 3 B at the mask's size, 12 B")
say(" at twice the size -- per winner; the fresh-canvas rows include the 8 B per canvas pixel of the reset.  ortho_compose: 4 B of rgba and 1 B of")
say(" cls read, 3 B written per canvas pixel.  eager: through the Python wrapper, output allocations and the enqueue included; graph: GROUP such")
say(" calls captured and replayed, per call.)")
say(f"clock after: {clocks()}")
