"""Timing of the distance ops (profiles/r23_distance.txt): ops.mask_distance and ops.region_proximity on one 1072 x 1920 five-frame window,
with and without the nearest plane, unbounded (R = 0) and bounded by the largest threshold, on three inputs -- a synthetic flood scene
(tools/stabilize_bench.py's moving blobs, class 1 the water), the single-source-pixel worst case of the row scan, and the empty frame --
against the bytes each call has to move (device events, medians of groups of back-to-back calls, run-to-run spread, the clock noted);
then the same windows of predict_clip without regions, with regions=True alone and with proximity on, unbounded and bounded,
alternating, in this one process.  Prints to stdout.  Every call is timed twice: eagerly through the Python wrapper and as a captured
graph of GROUP calls replayed.  `--op-only` skips the predict_clip part."""
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flood_uav_video_segmentation_amd import ops, synth  # noqa: E402
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows  # noqa: E402
from flood_uav_video_segmentation_amd.flow.model import FlowModel  # noqa: E402
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth
H, W, N = 1072, 1920, 5
THRESHOLDS = (8, 16, 32)
MAX_REGIONS = 1024
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


torch.set_grad_enabled(False)
rng = np.random.RandomState(0)
base = np.kron(rng.randint(0, 5, (H // 16 + 2, W // 16 + 2)), np.ones((16, 16), np.int64))
frames = np.stack([base[f:f + H, 2 * f:2 * f + W] for f in range(N)])
flip = rng.rand(N, H, W) < 0.05                                               # a segmenter's blobs moving (1, 2) pixels a frame, 5 % noise
flood = np.where(flip, rng.randint(0, 5, (N, H, W)), frames).astype(np.uint8)
single = np.zeros((N, H, W), np.uint8)
single[:, H // 2, W // 2] = 1                                                 # one source pixel a frame: every scan runs to the source's distance
empty = np.zeros((N, H, W), np.uint8)
scenes = [("flood scene", flood), ("single source pixel", single), ("empty frame", empty)]
px = H * W
d2 = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
nearest = torch.empty((N, H, W), dtype=torch.int32, device="cuda")
exposure = torch.empty((N, 5, len(THRESHOLDS)), dtype=torch.int64, device="cuda")
near = torch.empty((N, MAX_REGIONS, 8), dtype=torch.int64, device="cuda")

say(f"clock before: {clocks()}")
say(f"one {H} x {W} window of {N} frames, sources (1,), thresholds {THRESHOLDS}; medians of {SAMPLES} groups of {GROUP} calls (min .. max)")
say(f"{'call':<58}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")
for scene, host in scenes:
    mask = torch.from_numpy(host).cuda()
    labels = ops.mask_regions(mask, 5, 8)
    _, counts, index = ops.region_table(mask, labels, 5, None, 128, MAX_REGIONS)
    for want in (True, False):
        for r in (0, THRESHOLDS[-1]):
            out = (d2, nearest if want else None)
            call = lambda: ops.mask_distance(mask, (1,), r, want, out=out)  # noqa: E731
            med, lo, hi = sample(call)
            dev_us = sample_graph(call)
            per_pixel = 2 + 4 + (4 if want else 0) + 4 + 8 / 64                # mask twice, d2, nearest, the column entries out and in
            floor = N * per_pixel * px / HBM_BYTES_PER_S * 1e6
            name = f"mask_distance, {scene}, nearest {'yes' if want else 'no'}, R = {r}"
            say(f"{name:<58}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{dev_us:>10.1f}{N * per_pixel * px / 1e6:>10.1f}{floor:>10.1f}{floor / dev_us:>12.3f}")
    for r in (0, THRESHOLDS[-1]):
        ops.mask_distance(mask, (1,), r, True, out=(d2, nearest))
        call = lambda: ops.region_proximity(mask, d2, nearest, index, counts, 5, MAX_REGIONS, (3, 4), THRESHOLDS, out=(exposure, near))  # noqa: E731
        med, lo, hi = sample(call)
        dev_us = sample_graph(call)
        per_pixel = 1 + 4 + 4                                                  # mask, d2, index
        floor = N * per_pixel * px / HBM_BYTES_PER_S * 1e6
        name = f"region_proximity, {scene}, field of R = {r}"
        say(f"{name:<58}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{dev_us:>10.1f}{N * per_pixel * px / 1e6:>10.1f}{floor:>10.1f}{floor / dev_us:>12.3f}")
say("(mask_distance: per pixel 2 x 1 B of mask (both column passes read it), 4 B of d2, 4 B of nearest, 2 B of column entries written and")
say(" read back, 8 B per 64 pixels of chunk summaries; region_proximity: 1 B of mask, 4 B of d2, 4 B of index; the tables are small.")
say(" floor = bytes / 8.0 TB/s.  eager: through the Python wrapper, its workspace allocation and the enqueue included; graph: GROUP such")
say(" calls captured and replayed, per call.)")
say(f"clock after: {clocks()}")
if "--op-only" in sys.argv:
    sys.exit(0)

# ---- the same windows of predict_clip with and without proximity, alternating
from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet  # noqa: E402


class HP:
    layers, classes, pretrained = 50, 5, False


net = FlowPSPNet(HP()).eval()
net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
fm = FlowModel(net, feature_based=False, no_warp=False).eval()
delta, nframes = 5, 11
tex = np.kron(rng.randint(0, 256, ((H + 8 * nframes) // 8 + 1, W // 8, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "clip.rgb")
    with open(path, "wb") as fh:
        for i in range(nframes):
            fh.write(np.ascontiguousarray(tex[8 * i:8 * i + H, :W]).tobytes())
    ds = RawVideoWindows(path, H, W, "rgb24", size=(H, W), frame_delta=delta, grids="estimate", search=8)
    items = [ds[0], ds[1]]
kw = dict(classes=5, out_size=(H, W), crop=None, compute_metrics=True, cache_keyframes=False)
variants = [("no regions", dict()), ("regions=True", dict(regions=True)), ("regions=True, proximity (unbounded)", dict(regions=True, proximity=THRESHOLDS)),
            (f"regions=True, proximity_max={THRESHOLDS[-1]}", dict(regions=True, proximity=THRESHOLDS, proximity_max=THRESHOLDS[-1]))]
times = {name: [] for name, _ in variants}
for rep in range(8):
    for name, extra in variants:
        p = FlowPredictor(fm, **kw, **extra)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for m in p.predict_clip([dict(i) for i in items], to_host=False):
            pass
        torch.cuda.synchronize()
        if rep >= 2:                                                          # two warm-up rounds of every variant
            times[name].append((time.perf_counter() - t0) * 1e3)
say()
say(f"predict_clip, two {H} x {W} windows of {delta} frames (PSPNet-50, synthetic weights, whole frame, to_host=False), 6 alternating runs after 2 warm-ups")
for name, _ in variants:
    t = times[name]
    say(f"{name:<44} median {statistics.median(t):8.2f} ms per clip   min {min(t):8.2f}   max {max(t):8.2f}")
say(f"clock after: {clocks()}")
