"""Timing of the georeferencing ops (profiles/r34_ground.txt) on a 4096 x 4096 five-class canvas and a 4096 x 4096 north-up
raster under a mildly projective ground model: ops.ground_area without and with region_table's index plane, ops.ground_rectify of one
and of four uint8 planes, with and without the orthophoto, onto a raster the canvas' footprint fills and onto one it fills a quarter of
(the other tiles are empty and return after four projections), and ops.ground_points of 2^20 vertices.  Each eagerly through the Python
wrapper (its allocations and the enqueue are in the time) and as a replayed graph of REPS calls, device events, medians of SAMPLES
(min .. max), next to the bytes the op must move: ground_area 1 B per canvas pixel and 4 B more with the index; ground_rectify the
bytes read under the footprint plus the bytes written; ground_points 8 B in and 16 B out per point.  Prints to stdout."""
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flood_uav_video_segmentation_amd import ops  # noqa: E402
from flood_uav_video_segmentation_amd.flow.georef import GroundModel  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth
CH = CW = GH = GW = 4096
K, REGIONS = 5, 1024
SAMPLES, REPS = 20, 10
ORIGIN = (1024, 1536)


def say(s=""):
    print(s, flush=True)


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return " | ".join(l.strip() for l in r.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)) or "rocm-smi printed no GPU[0] clock"
    except Exception as e:  # noqa: BLE001
        return f"clock not read ({type(e).__name__})"


def events(fn, calls):
    ts = []
    for _ in range(SAMPLES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(ts), min(ts), max(ts)


def measure(name, fn, floor_bytes, note=""):
    """Eager and replayed microseconds a call, next to the time the bytes would take at the peak bandwidth."""
    fn()
    torch.cuda.synchronize()
    eager = events(fn, 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    replay = events(graph.replay, REPS)
    floor = floor_bytes / HBM_BYTES_PER_S * 1e6
    say(f"{name}: eager {eager[0]:.1f} us ({eager[1]:.1f} .. {eager[2]:.1f}), graph {replay[0]:.1f} us ({replay[1]:.1f} .. {replay[2]:.1f}); "
        f"{floor_bytes / 1e6:.1f} MB, floor {floor:.1f} us: {floor / replay[0]:.3f} of it{note}")
    return replay[0]


def main():
    torch.set_grad_enabled(False)
    rng = np.random.default_rng(34)
    # large patches of one class (a resolved mosaic looks like that), a quarter of the canvas never seen, 1024 block regions
    cls = np.repeat(np.repeat(rng.integers(0, K, (CH // 64, CW // 128)).astype(np.uint8), 64, axis=0), 128, axis=1)
    cls[:, :CW // 4] = 255
    index = (np.arange(CH)[:, None] // 128 * 32 + np.arange(CW)[None, :] // 128).astype(np.int32)
    index[cls == 255] = -1
    d_cls, d_index = torch.from_numpy(cls).cuda(), torch.from_numpy(index).cuda()
    planes = [d_cls] + [torch.from_numpy(rng.integers(0, 256, (CH, CW)).astype(np.uint8)).cuda() for _ in range(3)]
    rgba = torch.from_numpy((rng.integers(0, 1 << 24, (CH, CW)).astype(np.int64) | (0xFF << 24)).astype(np.uint32).view(np.int32)).cuda()
    model = GroundModel([250.0, 9.0, 0.0, 7.0, -250.0, 0.0, 2e-6, -1e-6, 1.0], (431250.0, 5412800.0), "projective")
    say(f"clock before: {clocks()}")
    say(f"canvas {CH} x {CW}, K = {K}, a quarter unseen, {REGIONS} regions; raster {GH} x {GW}; origin {ORIGIN}; a projective model of about 0.25 m a pixel; "
        f"medians of {SAMPLES} (min .. max); graphs of {REPS} calls")
    px = CH * CW
    measure("ground_area, classes only", lambda: ops.ground_area(d_cls, model, ORIGIN, K), px)
    measure("ground_area, classes and regions", lambda: ops.ground_area(d_cls, model, ORIGIN, K, d_index, REGIONS), px * 5,
            " (the unseen quarter's tiles read 1 B a pixel and return: the floor counts 5 B for them too)")
    _, gsd, top_left = model.raster((CH, CW), ORIGIN)
    full_size, full_gsd, full_top_left = model.raster((CH, CW), ORIGIN, gsd)
    say(f"the canvas' footprint at the model's mean pixel size of {gsd} mm: a raster of {full_size[0]} x {full_size[1]}")
    for label, g, tl in (("the footprint fills the raster", gsd, top_left), ("the footprint fills a quarter of it", 2 * gsd, top_left)):
        inside = torch.from_numpy(np.ones((1, 1), np.uint8)).cuda().expand(CH, CW).contiguous()
        covered = int((ops.ground_rectify(model, ORIGIN, (GH, GW), g, tl, (inside,), None, 0)[0][0] == 1).sum().item())
        # bytes read under the footprint: every canvas pixel under a raster sample once at the most, at the raster's own density at the least
        read_px = min(covered, px)
        for n_planes, with_rgb in ((1, False), (4, False), (1, True), (4, True)):
            floor = read_px * (n_planes + (4 if with_rgb else 0)) + GH * GW * (n_planes + (3 if with_rgb else 0))
            measure(f"ground_rectify, {label}, {n_planes} plane{'s' if n_planes > 1 else ''}{' and the orthophoto' if with_rgb else ''} ({covered} raster pixels on the canvas)",
                    lambda: ops.ground_rectify(model, ORIGIN, (GH, GW), g, tl, planes[:n_planes], rgba if with_rgb else None), floor)
    n = 1 << 20
    pts = torch.from_numpy(np.stack([rng.integers(0, CW + 1, n), rng.integers(0, CH + 1, n)], axis=1).astype(np.int32)).cuda()
    measure(f"ground_points, {n} vertices", lambda: ops.ground_points(pts, model, ORIGIN), n * 24)
    say("(float64 work per call: ground_area two divisions per lattice corner of a tile that is not all unseen, 65 x 17 corners per 64 x 16 pixels;")
    say(" ground_rectify two divisions per raster pixel of a tile that is not empty; ground_points two per point.  Per-kernel times, counters, K = 32,")
    say(" other tile shapes and real mosaics: NOT MEASURED.)")
    say(f"clock after: {clocks()}")


if __name__ == "__main__":
    main()
