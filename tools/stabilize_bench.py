"""Timing of the temporal mask stabiliser (profiles/r22_stabilize.txt): ops.mask_stabilize on one 1072 x 1920 five-frame window, in
place and compensated, with and without a confidence plane, against the bytes each route has to move (device events, medians of
groups of back-to-back calls, run-to-run spread, the clock noted); then the same windows of predict_clip with and without stabilize=3,
alternating, in this one process.  Prints to stdout.  Every route is timed twice: eagerly through the Python wrapper (what a caller
pays per call, enqueue included) and as a captured graph of GROUP calls replayed (the device's time, launch boundaries included).
`--op-only` skips the predict_clip part; `--kernels N`: only N calls of each route, for a rocprofv3 --kernel-trace --stats run."""
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
H, W, N, PERSIST = 1072, 1920, 5, 3
GROUP, SAMPLES = 10, 30   # one sample = GROUP back-to-back calls between two events


def say(s=""):
    print(s, flush=True)


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return " | ".join(l.strip() for l in r.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)) or "rocm-smi printed no GPU[0] clock"
    except Exception as e:  # noqa: BLE001
        return f"clock not read ({type(e).__name__})"


def sample(fn):
    for _ in range(20):
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
    for _ in range(5):
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
mask = torch.from_numpy(np.where(flip, rng.randint(0, 5, (N, H, W)), frames).astype(np.uint8)).cuda()
conf = torch.from_numpy(rng.randint(0, 256, (N, H, W)).astype(np.uint8)).cuda()
hb, wb = H // 16, W // 16
by, bx = np.mgrid[0:hb, 0:wb]
row = np.stack([np.full((hb, wb), -1), np.full((hb, wb), 16), np.full((hb, wb), 16), bx * 16 + 8 - 2, by * 16 + 8 - 1, bx * 16 + 8, by * 16 + 8], -1)
mv = torch.from_numpy(np.stack([row.reshape(hb * wb, 7)] * N).astype(np.int32)).cuda()
out = torch.empty_like(mask)
state = ops.mask_stabilize(mask, None, persist=PERSIST)[1]                     # a valid plane: every timed call is a chained one
px = H * W

routes = [
    ("in place", dict(), N * 2 + 8),
    ("in place, conf + trust", dict(conf=conf, trust=200), N * 3 + 8),
    ("compensated", dict(mv=mv, frame_size=(H, W)), N * (2 + 8) + 8),         # + the odd-n copy of the caller's plane: 8 B
    ("compensated, conf + trust", dict(conf=conf, trust=200, mv=mv, frame_size=(H, W)), N * (3 + 8) + 8),
]
if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    for _ in range(int(sys.argv[2])):
        for _, kw, _ in routes:
            ops.mask_stabilize(mask, state, persist=PERSIST, out=out, **kw)
    torch.cuda.synchronize()
    sys.exit(0)

say(f"clock before: {clocks()}")
say(f"ops.mask_stabilize, one {H} x {W} window of {N} frames, persist {PERSIST}; medians of {SAMPLES} groups of {GROUP} calls (min .. max)")
say(f"{'route':<28}{'eager us':>10}{'min':>8}{'max':>8}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")
for name, kw, per_pixel in routes:
    med, lo, hi = sample(lambda: ops.mask_stabilize(mask, state, persist=PERSIST, out=out, **kw))
    dev_us = sample_graph(lambda: ops.mask_stabilize(mask, state, persist=PERSIST, out=out, **kw))
    floor = per_pixel * px / HBM_BYTES_PER_S * 1e6
    say(f"{name:<28}{med:>10.1f}{lo:>8.1f}{hi:>8.1f}{dev_us:>10.1f}{per_pixel * px / 1e6:>10.1f}{floor:>10.1f}{floor / dev_us:>12.2f}")
say("(in place: n (1 or 2 B in + 1 B out) + 8 B of state per pixel and CALL; compensated: n (that + 8 B of state) per pixel, plus 8 B for the")
say(" copy of the caller's plane that an odd n needs.  floor = bytes / 8.0 TB/s.  eager: through the Python wrapper, its allocations of")
say(" counts and workspace and the enqueue included; graph: 10 such calls captured and replayed, per call.)")
say(f"clock after: {clocks()}")
if "--op-only" in sys.argv:
    sys.exit(0)

# ---- the same windows of predict_clip with and without stabilize, alternating
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
    ds = RawVideoWindows(path, H, W, "rgb24", size=(H, W), frame_delta=delta, grids="estimate", search=8, link_vectors=True)
    items = [ds[0], ds[1]]
kw = dict(classes=5, out_size=(H, W), crop=None, compute_metrics=True, cache_keyframes=False)
variants = [("stabilize off", dict()), ("stabilize=3", dict(stabilize=3)), ("stabilize=3, compensated", dict(stabilize=3, stabilize_compensate=True))]
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
    say(f"{name:<28} median {statistics.median(t):8.2f} ms per clip   min {min(t):8.2f}   max {max(t):8.2f}")
say(f"clock after: {clocks()}")
