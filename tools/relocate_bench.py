"""Timing of relocalisation against the orthophoto (profiles/r28_relocate.txt): ops.map_coarse, ops.map_patch, ops.map_locate,
ops.pose_relocate and ops.relocate_commit alone, and the whole sequence FlowPredictor(mosaic_relocate=True) runs for a lost frame -- those
five with the fine registration (map_view, block_match_modes, map_gate, global_motion, pose_correct) in their middle -- on
tools/mosaic_bench.py's scenario: 1072 x 1920 frames and a 4096 x 4096 canvas.  The map holds eight frames of a pan of (80, 48) px a
frame over a blocky random ground; the chain is lost with the last frame's pose, and the frame measured lies where the first one was,
(560, 336) px away.  S = 8 and S = 16.  Device events, medians of 20 groups of 5 back-to-back calls, eagerly through the Python wrappers
and as a captured graph replayed; the clock read before and after.  map_locate's rate counts one absolute difference per patch cell and
placement, whether or not the cell is valid, beside the block matcher's.  Prints to stdout."""
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
H, W, N = 1072, 1920, 8
STEP = (80, 48)           # (x, y) px a frame: whole cells at S = 8 and S = 16
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
ground = np.kron(rng.randint(0, 256, ((H + N * STEP[1]) // 8 + 1, (W + N * STEP[0]) // 8 + 1, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8)
sources = [(torch.from_numpy(np.ascontiguousarray(ground[STEP[1] * f:STEP[1] * f + H, STEP[0] * f:STEP[0] * f + W])).cuda(), None, "rgb24", "bt709", False)
           for f in range(N)]
mask = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
origin = ((CANVAS[0] - H) // 2 - 200, (CANVAS[1] - W) // 2 - 400)        # whole cells of 8 and 16
size, ordinal = (H, W), N

say(f"clock before: {clocks()}")
say(f"{H} x {W} frames, canvas {CANVAS[0]} x {CANVAS[1]}, a map of {N} frames {STEP} px apart; the lost frame lies {((N - 1) * STEP[0], (N - 1) * STEP[1])} px from "
    f"the last pose; medians of {SAMPLES} groups of {GROUP} calls (min .. max)")
say(f"{'call':<66}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")

rank, rgba = ops.ortho_canvas(CANVAS, "cuda")
for f in range(N):
    ops.ortho_accumulate(sources[f], pose_row(STEP[0] * f, STEP[1] * f), f, size, rank, rgba, origin)
last = pose_row(STEP[0] * (N - 1), STEP[1] * (N - 1))
lost = torch.zeros((32,), dtype=torch.int64, device="cuda")
lost[:12], lost[12], lost[16], lost[18], lost[22], lost[24], lost[25], lost[26] = last[:12], ONE, ONE, ONE, ONE, 2, N + 1, 1
lost_pose = torch.tensor([ONE, 0, 0, 0, ONE, 0, ONE, 0, 0, 0, ONE, 0, 2, 0, 0, 0], dtype=torch.int64, device="cuda")
frame = sources[0]                                                          # the cut: back to where the first frame was

for s in (8, 16):
    say(f"S = {s}")
    ch, cw = CANVAS[0] // s, CANVAS[1] // s
    cl, cv = ops.map_coarse(rgba, s)
    row(f"  map_coarse ({ch} x {cw} cells)", lambda: ops.map_coarse(rgba, s), 4 * ch * s * cw * s + 2 * ch * cw)
    tl, tv, geom = ops.map_patch(frame, lost, size, CANVAS, origin, s)
    g = geom.tolist()
    row(f"  map_patch ({g[4]} x {g[3]} cells, {g[5]} valid)", lambda: ops.map_patch(frame, lost, size, CANVAS, origin, s), 3 * g[3] * g[4] * s * s + 2 * g[3] * g[4])
    found = ops.map_locate(cl, cv, tl, tv, geom, 500, 2)
    fl = found.tolist()
    pairs = fl[10] * g[3] * g[4]
    t_locate = row(f"  map_locate ({fl[10]} placements, {fl[11]} eligible)", lambda: ops.map_locate(cl, cv, tl, tv, geom, 500, 2))
    say(f"    ({pairs / 1e9:.3f} G masked absolute differences: {pairs / t_locate / 1e6:.2f} T/s over both launches, beside the block matcher's 61 T/s; found: status "
        f"{fl[0]}, shift ({fl[1]}, {fl[2]}) cells, sad {fl[3]} on {fl[4]} cells, runner-up sad {fl[8]} on {fl[9]})")
    cand_state, cand_pose = ops.pose_relocate(found, lost, size, CANVAS, origin, s, 16, 800)
    row("  pose_relocate", lambda: ops.pose_relocate(found, lost, size, CANVAS, origin, s, 16, 800), (16 + 32 + 32 + 16) * 8)
    no_fit = torch.tensor([2, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device="cuda")   # status 5: nothing is copied, so every call of a group does the same work
    row("  relocate_commit (a candidate without a fine fit: nothing changes)",
        lambda: ops.relocate_commit(cand_state, cand_pose, no_fit, lost, lost_pose.clone(), found, s), (32 + 16 + 8 + 16 + 8) * 8)

    def sequence():
        """The launches of one lost frame.  The state is restored first, so every call of a group finds the same lost chain."""
        state = lost.clone()
        pose = lost_pose.clone()
        a, b = ops.map_coarse(rgba, s)
        p, q, gm = ops.map_patch(frame, state, size, CANVAS, origin, s)
        f_ = ops.map_locate(a, b, p, q, gm, 500, 2)
        cs, cp = ops.pose_relocate(f_, state, size, CANVAS, origin, s, 16, 800)
        c, v, ok = ops.map_view(frame, cp, ordinal, size, rank, rgba, origin)
        t, st = ops.block_match_modes(c, v, SEARCH, 0, 65535, return_stats=True)
        ops.map_gate(t, ok)
        m = ops.global_motion(t[None], size, size, 4, 1.0, 12, mask=mask, exclude=(), pair_stats=st[None])
        co = ops.pose_correct(m, cs, cp, size, CANVAS, origin)
        return ops.relocate_commit(cs, cp, co, state, pose, f_, s), pose

    out, pose = sequence()
    say(f"    (the sequence: status {int(out[0])}, shift {out[1:3].tolist()} px, the committed translation ({int(pose[2]) / ONE:.2f}, {int(pose[5]) / ONE:.2f}) against "
        f"the true (0, 0))")
    row("  the whole lost-frame sequence: 14 launches and two row copies", sequence)
say("(floors at 8.0 TB/s.  map_coarse: the canvas words its cells cover, read once, and two bytes a cell written.  map_patch: three frame bytes per")
say(" pixel of the patch and two bytes a cell.  The two steps: their rows.  eager: through the Python wrapper, output allocations and the enqueue")
say(" included; graph: GROUP such calls captured and replayed, per call.)")
say(f"clock after: {clocks()}")
