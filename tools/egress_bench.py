"""Timing of frame egress (profiles/r10_egress.txt): ops.compose_frame against fs_colorize on one 1072 x 1920 mask (device events, medians,
run-to-run spread, the clock noted), and device masks -> bytes on the host through colorize().cpu() and through compose_window +
RawVideoWriter.  One process; prints to stdout.  `--kernels N`: only N calls of each variant, for a rocprofv3 --kernel-trace --stats run."""
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
from flood_uav_video_segmentation_amd import ops  # noqa: E402
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWriter, raw_frame_bytes  # noqa: E402
from flood_uav_video_segmentation_amd.flow.predict import PALETTE, colorize, compose_window  # noqa: E402



def say(s=""):
    print(s, flush=True)


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return " | ".join(l.strip() for l in r.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)) or "rocm-smi printed no GPU[0] clock"
    except Exception as e:  # noqa: BLE001
        return f"clock not read ({type(e).__name__})"


torch.set_grad_enabled(False)
h, w = 1072, 1920
rng = np.random.RandomState(0)
mask = torch.from_numpy(rng.randint(0, 5, (h, w)).astype(np.uint8)).cuda()
# a blobby mask as a segmenter gives it (runs of equal classes), besides the noise one
blob = torch.from_numpy(np.kron(rng.randint(0, 5, (h // 16, w // 16)), np.ones((16, 16))).astype(np.uint8)).cuda()
y = torch.from_numpy(rng.randint(0, 256, (1080, 1920)).astype(np.uint8)).cuda()
uv = torch.from_numpy(rng.randint(0, 256, (540, 960, 2)).astype(np.uint8)).cuda()
pal4 = np.concatenate([PALETTE, np.full((5, 1), 128, np.uint8)], axis=1)
rgb_out = torch.empty(raw_frame_bytes(h, w, "rgb24"), dtype=torch.uint8, device="cuda")
nv_out = torch.empty(raw_frame_bytes(h, w, "nv12"), dtype=torch.uint8, device="cuda")

GROUP, SAMPLES = 10, 30   # one sample = GROUP back-to-back launches between two events (a single ~5 us launch is below the events' resolution)


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
    return statistics.median(ts)


def cases(m):
    return [
        ("fs_colorize (parent)", lambda: colorize(m), h * w + h * w * 3),
        ("frame_compose RGB24 opaque", lambda: ops.compose_frame(m, PALETTE, out_fmt="rgb24", out=rgb_out), h * w + h * w * 3),
        ("frame_compose NV12 opaque", lambda: ops.compose_frame(m, PALETTE, out_fmt="nv12", out_matrix="bt709", out=nv_out), h * w + h * w * 3 // 2),
        ("frame_compose NV12 overlay <- 1080x1920 NV12", lambda: ops.compose_frame(m, pal4, y, uv, "nv12", "bt709", False, "nv12", out=nv_out),
         h * w + h * w * 3 // 2 + 1080 * 1920 * 3 // 2),
    ]


if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    for _ in range(int(sys.argv[2])):
        for _, fn, _ in cases(mask):
            fn()
    torch.cuda.synchronize()
    sys.exit(0)

say("frame egress timing, MI355X, one process; %d x %d; python wrapper included (launch through ctypes, stream-ordered)" % (h, w))
say("per sample: %d back-to-back calls between two device events; median of %d samples after 20 warm-up calls; 5 rounds, the variants alternating" % (GROUP, SAMPLES))
say("clock before: " + clocks())
for label, m in (("noise mask", mask), ("blob mask (16 x 16 runs)", blob)):
    rounds = {name: [] for name, _, _ in cases(m)}
    for _ in range(5):
        for name, fn, _ in cases(m):
            rounds[name].append(sample(fn))
    say("")
    say(label + ":   us per call (median of the 5 round medians; min .. max = run-to-run spread);  GB/s = bytes the op must move / that time")
    for name, _, nbytes in cases(m):
        r = rounds[name]
        med = statistics.median(r)
        say(f"  {name:48s} {med:8.2f} us  ({min(r):.2f} .. {max(r):.2f}, spread {max(r) - min(r):.2f})  {nbytes / med / 1e3:8.1f} GB/s")
    c, e = rounds["fs_colorize (parent)"], rounds["frame_compose RGB24 opaque"]
    diff = statistics.median(e) - statistics.median(c)
    allowed = (max(c) - min(c)) + (max(e) - min(e))
    say(f"  condition: RGB24 opaque - fs_colorize = {diff:+.2f} us, allowed <= combined spread {allowed:.2f} us -> {'HOLDS' if diff <= allowed else 'FAILS'}")
say("clock after: " + clocks())

# the calls above include the python wrapper; the bare enqueue cost, for scale
t0 = time.perf_counter()
for _ in range(2000):
    ops.compose_frame(mask, PALETTE, out_fmt="nv12", out_matrix="bt709", out=nv_out)
torch.cuda.synchronize()
say("")
say("2000 NV12 opaque calls enqueued and finished: %.2f us per call wall (host-side wrapper + launch bound)" % ((time.perf_counter() - t0) / 2000 * 1e6))

# ------------------------------------------------------------------ device masks -> bytes on the host, per frame
masks = torch.stack([mask, blob, mask.flip(0), blob.flip(1), mask.flip(1)])   # one window of 5 frames
N = 40


class Sink:
    def write(self, b):
        return len(b)

    def flush(self):
        pass


def parent_route():
    for _ in range(N):
        colorize(masks).cpu().numpy()


def new_route(target):
    with RawVideoWriter(target, h, w, "nv12", frames=None if not isinstance(target, str) else N * 5) as wr:
        for i in range(N):
            for p, buf in enumerate(compose_window(masks, None, PALETTE, out_fmt="nv12")):
                wr.write(i * 5 + p, buf)


def wall(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) / (N * 5) * 1e3)
    return ts


say("")
say("device masks [5,%d,%d] -> bytes on the host, ms per frame (3 repeats of %d windows after one warm-up pass):" % (h, w, N))
say("  parent route  colorize(masks).cpu()  (6.2 MB/frame, pageable copy):      " + "  ".join(f"{t:.3f}" for t in wall(parent_route)))
say("  new route     compose_window NV12 -> RawVideoWriter (3.1 MB/frame, pinned), discarding sink: " + "  ".join(f"{t:.3f}" for t in wall(lambda: new_route(Sink()))))
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "out.nv12")
    say("  new route     the same into a regular file (pwrite, page cache):           " + "  ".join(f"{t:.3f}" for t in wall(lambda: new_route(path))))
say("done")
