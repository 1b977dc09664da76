"""Timing of frame-to-map registration (profiles/r26_refine.txt): ops.map_view, ops.map_gate and ops.pose_correct alone, the ops between
them (ops.block_match_modes, ops.global_motion with n = 1) and the whole per-frame chain FlowPredictor(mosaic_refine=True) runs -- pose_chain
(n = 1), map_view, block_match_modes, map_gate, global_motion, pose_correct, ortho_accumulate -- beside ops.mosaic_accumulate in the SAME
run, on tools/mosaic_bench.py's scenario: 1072 x 1920 frames, a five-frame window, a 4096 x 4096 canvas, a slow pan of (3, 2) px a frame
over a random ground texture.  The canvas holds the window's first four frames; the frame measured is the fifth, with a predicted pose
that is (2, 1) px off.  Device events, medians of 20 groups of 5 back-to-back calls, eagerly through the Python wrappers and as a captured
graph replayed; the clock read before and after.  Next to each of the three new kernels its byte floor at 8 TB/s.  Prints to stdout."""
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
SEARCH = 8


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
    tail = "" if moved is None else f"{moved / 1e6:>10.2f}{moved / HBM_BYTES_PER_S * 1e6:>10.2f}{moved / HBM_BYTES_PER_S * 1e6 / dev_us:>12.3f}"
    say(f"{name:<66}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{dev_us:>10.1f}{tail}")
    return dev_us


def pose_row(tx, ty):
    return torch.tensor([ONE, 0, tx * ONE, 0, ONE, ty * ONE, ONE, 0, -tx * ONE, 0, ONE, -ty * ONE, 0, 0, 0, 0], dtype=torch.int64, device="cuda")


torch.set_grad_enabled(False)
rng = np.random.RandomState(0)
ground = rng.randint(0, 256, (H + 2 * N, W + 3 * N, 3)).astype(np.uint8)
sources = [(torch.from_numpy(np.ascontiguousarray(ground[2 * f:2 * f + H, 3 * f:3 * f + W])).cuda(), None, "rgb24", "bt709", False) for f in range(N)]
base = np.kron(rng.randint(0, 5, (H // 16 + 2, W // 16 + 2)), np.ones((16, 16), np.int64))
mask = torch.from_numpy(np.stack([base[f:f + H, 2 * f:2 * f + W] for f in range(N)]).astype(np.uint8)).cuda()
origin = ((CANVAS[0] - H) // 2, (CANVAS[1] - W) // 2)
size, last = (H, W), N - 1
blocks = (H // 16) * (W // 16)

say(f"clock before: {clocks()}")
say(f"{H} x {W} frames, canvas {CANVAS[0]} x {CANVAS[1]}, the fifth frame of a (3, 2) px pan against a map of the first four, search {SEARCH}; medians of "
    f"{SAMPLES} groups of {GROUP} calls (min .. max)")
say(f"{'call':<66}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")

rank, rgba = ops.ortho_canvas(CANVAS, "cuda")
for f in range(last):
    ops.ortho_accumulate(sources[f], pose_row(3 * f, 2 * f), f, size, rank, rgba, origin)
predicted = pose_row(3 * last + 2, 2 * last + 1)                           # the chain's guess: (2, 1) px off
state = torch.zeros((32,), dtype=torch.int64, device="cuda")
state[:12], state[24] = predicted[:12], 1
identity_pair = torch.tensor([[ONE, 0, 0, 0, ONE, 0, ONE, 0, 0, 0, ONE, 0, 0, blocks, blocks, 4]], dtype=torch.int64, device="cuda")

poses = torch.stack([pose_row(3 * f, 2 * f) for f in range(N)])
votes = torch.zeros((K,) + CANVAS, dtype=torch.int16, device="cuda").view(torch.uint16)
ops.mosaic_accumulate(mask, poses, votes, origin)
touched = int((votes.view(torch.int16) != 0).sum())
row("mosaic_accumulate, the window (one call)", lambda: ops.mosaic_accumulate(mask, poses, votes, origin), N * H * W + 4 * touched)

cur, view, valid = ops.map_view(sources[last], predicted, last, size, rank, rgba, origin)
seen = int(valid.sum())
for age in (0, 2):
    row(f"map_view, min_age {age}", lambda: ops.map_view(sources[last], predicted, last, size, rank, rgba, origin, age),
        H * W * (3 + 3) + (4 + (8 if age else 0)) * seen)
table, stats = ops.block_match_modes(cur, view, SEARCH, 0, 65535, return_stats=True)
row(f"block_match_modes(cur, view), search {SEARCH}", lambda: ops.block_match_modes(cur, view, SEARCH, 0, 65535, return_stats=True))
gated = ops.map_gate(table.clone(), valid)
kept = int((gated[:, 0] == -1).logical_and(gated[:, 3] >= 0).sum())
row("map_gate", lambda: ops.map_gate(table, valid), blocks * (28 + 256))
fit = ops.global_motion(gated[None], size, size, 4, 1.0, 12, mask=mask[last:last + 1], exclude=(1,), pair_stats=stats[None])
row("global_motion, n = 1", lambda: ops.global_motion(gated[None], size, size, 4, 1.0, 12, mask=mask[last:last + 1], exclude=(1,), pair_stats=stats[None]))
pose = predicted.clone()
out = ops.pose_correct(fit, state.clone(), pose, size, CANVAS, origin)
say(f"  ({seen} of {H * W} view pixels valid, {kept} of {blocks} rows kept by the gate; the fit: status {int(fit[0, 12])}, {int(fit[0, 14])} inliers, shift "
    f"({int(fit[0, 2]) / ONE:.4f}, {int(fit[0, 5]) / ONE:.4f}) px; pose_correct status {int(out[0])}, corrected translation "
    f"({int(pose[2]) / ONE:.4f}, {int(pose[5]) / ONE:.4f}) against the true ({3 * last}, {2 * last}))")
no_fit = fit.clone()
no_fit[0, 12] = 2                                                          # status 2: the state is left alone, so every call of a group does the same work
row("pose_correct (a model without a fit: nothing changes)", lambda: ops.pose_correct(no_fit, state, predicted, size, CANVAS, origin), (16 + 32 + 16 + 16 + 12 + 8) * 8)


def per_frame():
    """The seven launches of one refined frame.  The pair model is the identity and the canvas already holds the frame after the first
    call, so every call of a group finds the same state: a predicted pose that the fit moves (or leaves) the same way."""
    state[:12] = predicted[:12]
    row_ = ops.pose_chain(identity_pair, state, size, CANVAS, origin)[0]
    c, v, ok = ops.map_view(sources[last], row_, last, size, rank, rgba, origin)
    t, s = ops.block_match_modes(c, v, SEARCH, 0, 65535, return_stats=True)
    ops.map_gate(t, ok)
    m = ops.global_motion(t[None], size, size, 4, 1.0, 12, mask=mask[last:last + 1], exclude=(1,), pair_stats=s[None])
    ops.pose_correct(m, state, row_, size, CANVAS, origin)
    ops.ortho_accumulate(sources[last], row_, last, size, rank, rgba, origin)


def unrefined_frame():
    state[:12] = predicted[:12]
    row_ = ops.pose_chain(identity_pair, state, size, CANVAS, origin)[0]
    ops.ortho_accumulate(sources[last], row_, last, size, rank, rgba, origin)


t_plain = row("one frame without registration: pose_chain (n = 1), ortho_accumulate", unrefined_frame)
t_chain = row("one frame with it: the seven launches", per_frame)
say(f"  (registration adds {t_chain - t_plain:.1f} us a frame replayed; five such frames {5 * (t_chain - t_plain) / 1000:.3f} ms a window)")
say("(floors at 8.0 TB/s.  map_view: 3 B of frame read and 3 B of planes written per frame pixel, + 4 B of rgba per valid pixel, + 8 B of rank")
say(" with an age gate.  map_gate: a 28 B row and the 256 valid bytes under its winner per block.  pose_correct: the three rows in, pose, twelve")
say(" state words and the out row back.  eager: through the Python wrapper, output allocations and the enqueue included; graph: GROUP such calls")
say(" captured and replayed, per call.)")
say(f"clock after: {clocks()}")
