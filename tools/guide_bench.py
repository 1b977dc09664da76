"""Timing of ops.guide_vectors (profiles/r27_guide.txt): table-only and with evidence, beside the search (ops.block_match_modes, search 24,
with its costs) and the fit (ops.global_motion, n = 1) it follows, in the SAME run, at 1072 x 1920: a pan of (20, 0) px over a random
ground texture with a flat noisy lake of 20 x 30 blocks, intra_bias 0, so that the lake's rows are void (filled) and a tenth of the
other rows, overwritten with random vectors, are outliers (replaced, dropped, or, with evidence, looked at).  Device events, medians of
20 groups of 5 back-to-back calls, eagerly through the Python wrappers and as a captured graph replayed; the clock read before and
after.  Next to guide_vectors its byte floor at 8 TB/s.  Prints to stdout."""
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
H, W = 1072, 1920
PAN, SEARCH, PENALTY = (20, 0), 24, 1
LAKE = (320, 480, 640, 960)   # y0, x0, y1, x1 of the current frame: 20 x 30 blocks
GROUP, SAMPLES = 5, 20        # one sample = GROUP back-to-back calls between two events


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
    tail = "" if moved is None else f"{moved / 1e6:>10.3f}{moved / HBM_BYTES_PER_S * 1e6:>10.3f}{moved / HBM_BYTES_PER_S * 1e6 / dev_us:>12.4f}"
    say(f"{name:<66}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{dev_us:>10.1f}{tail}")
    return dev_us


torch.set_grad_enabled(False)
rng = np.random.RandomState(0)
y0, x0, y1, x1 = LAKE
ref = rng.randint(0, 256, (H, W)).astype(np.uint8)
ref[y0 + PAN[1]:y1 + PAN[1], x0 + PAN[0]:x1 + PAN[0]] = 100 + rng.randint(-3, 4, (y1 - y0, x1 - x0))
cur = rng.randint(0, 256, (H, W)).astype(np.uint8)
cur[:, :W - PAN[0]] = ref[:, PAN[0]:]
cur[y0:y1, x0:x1] = 100 + rng.randint(-3, 4, (y1 - y0, x1 - x0))
cur, ref = torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda()
size, blocks = (H, W), (H // 16) * (W // 16)

say(f"clock before: {clocks()}")
say(f"{H} x {W} luma frames, a pan of {PAN} px, search {SEARCH}, penalty {PENALTY}, intra_bias 0; medians of {SAMPLES} groups of {GROUP} calls (min .. max)")
say(f"{'call':<66}{'eager us':>10}{'min':>9}{'max':>9}{'graph us':>10}{'MB moved':>10}{'floor us':>10}{'floor/graph':>12}")

search = lambda: ops.block_match_modes(cur, ref, SEARCH, PENALTY, 0, return_cost=True, return_stats=True)  # noqa: E731
table, cost, stats = search()
t_search = row(f"block_match_modes, search {SEARCH}, with costs and stats", search)
fit = lambda: ops.global_motion(table[None], size, size, 4, 1.0, 12, pair_stats=stats[None])  # noqa: E731
model = fit()
t_fit = row("global_motion, n = 1, mask_size = frame_size", fit)

noisy = table.clone()                                                      # a tenth of the rows that carry a vector: random vectors instead
pick = torch.from_numpy(rng.permutation(blocks)[:blocks // 10]).cuda()
pick = pick[noisy[pick, 3] >= 0]
noisy[pick, 3] = noisy[pick, 5] + torch.from_numpy(rng.randint(-32, 33, len(pick))).cuda().int()
noisy[pick, 4] = noisy[pick, 6] + torch.from_numpy(rng.randint(-32, 33, len(pick))).cuda().int()
tables, costs, curs, refs = noisy[None].contiguous(), cost[None].contiguous(), cur[None], ref[None]
out = torch.empty_like(tables)

_, counts = ops.guide_vectors(tables, model, size, outlier=1.0, out=out)
names = ops.GUIDE_COUNTS
say(f"  (the fit: status {int(model[0, 12])}, shift ({int(model[0, 2]) / ops.POSE_ONE:.3f}, {int(model[0, 5]) / ops.POSE_ONE:.3f}) px, {int(model[0, 14])} inliers; table only: "
    + ", ".join(f"{k} {int(v)}" for k, v in zip(names, counts[0].tolist())) + ")")
table_bytes = blocks * (28 + 28) + 16 * 8 + 2 * 8 * 8
t_table = row("guide_vectors, table only, outlier 1.0, fill_void", lambda: ops.guide_vectors(tables, model, size, outlier=1.0, out=out), table_bytes)
t_place = row("guide_vectors, table only, in place (out = tables' copy)", lambda: ops.guide_vectors(out, model, size, outlier=1.0, out=out), table_bytes)
for bias in (0, 65535):
    _, counts = ops.guide_vectors(tables, model, size, outlier=1.0, cur=curs, ref=refs, cost=costs, penalty=PENALTY, guide_bias=bias, out=out)
    asked = int(counts[0, 4] + counts[0, 6])
    say(f"  (evidence, guide_bias {bias}: " + ", ".join(f"{k} {int(v)}" for k, v in zip(names, counts[0].tolist())) + f"; {asked} blocks read the frames)")
    t_ev = row(f"guide_vectors, evidence, guide_bias {bias}",
               lambda: ops.guide_vectors(tables, model, size, outlier=1.0, cur=curs, ref=refs, cost=costs, penalty=PENALTY, guide_bias=bias, out=out),
               table_bytes + blocks * 4 + asked * 2 * 256)


def chain():
    t, c, s = search()
    m = ops.global_motion(t[None], size, size, 4, 1.0, 12, pair_stats=s[None])
    ops.guide_vectors(t[None], m, size, outlier=1.0, cur=curs, ref=refs, cost=c[None], penalty=PENALTY, guide_bias=0)


def unguided():
    search()


t_plain = row("the pair without guidance: the search", unguided)
t_chain = row("the pair with it: search, fit, guide (evidence)", chain)
say(f"  (guidance adds {t_chain - t_plain:.1f} us a pair replayed: the fit {t_fit:.1f}, the guide {t_ev:.1f} with evidence, {t_table:.1f} without; the search alone {t_search:.1f})")
say("(floors at 8.0 TB/s.  guide_vectors: a 28 B row in and out per block, the model row, the counts cleared and added to; with evidence 4 B of cost")
say(" per block and 2 x 256 B of pixels for every block that asks the frames.  eager: through the Python wrapper, output allocations and the enqueue")
say(" included; graph: GROUP such calls captured and replayed, per call.  Not measured: RGB frames, n > 1, frames that do not allow dword loads.)")
say(f"clock after: {clocks()}")
