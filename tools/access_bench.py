"""Timing of ops.mask_access (profiles/r32_access.txt) on a 4096 x 4096 five-class canvas, on two maps: an open field with
one seed in the middle, which needs few rounds, and a serpentine of corridors 31 pixels wide between walls of water with a gap at
alternating ends, which needs many.  The round count depends on the map's shape, not on the kernel alone.  For each map: the rounds the
field needs (found by resuming in chunks until status says converged, and summing the rounds that lowered something), then whole calls
with exactly that many rounds plus one, timed with device events (medians of SAMPLES calls, through the Python wrapper: the enqueue of
every round is in it), the time of a call on the converged planes (every round idle but the first), and the bytes: per call the init and
finish passes, per round the flags of every tile, per dirty tile its staged keys and classes and the keys it writes back.  Also
ops.region_access on the open field's planes.  Prints to stdout."""
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
H = W = 4096
COST, TERMINAL = {4: 1, 0: 2, 2: 6, 3: 2}, (3,)
CHUNK, SAMPLES = 4096, 5
T = ops.ACCESS_TILE


def say(s=""):
    print(s, flush=True)


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return " | ".join(l.strip() for l in r.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)) or "rocm-smi printed no GPU[0] clock"
    except Exception as e:  # noqa: BLE001
        return f"clock not read ({type(e).__name__})"


def timed(fn, samples=SAMPLES):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def rounds_needed(mask, seeds):
    """Resume in chunks until converged -> (the rounds that lowered something, the chunks, the pixels with a value)."""
    planes, lowered, chunks = None, 0, 0
    while True:
        d, origin, status = ops.mask_access(mask, seeds, COST, TERMINAL, 8, rounds=CHUNK, resume=planes)
        planes, chunks = (d, origin), chunks + 1
        st = status[0].tolist()
        lowered += st[1]
        if st[0]:
            return lowered, chunks, st[2], planes
        if chunks * CHUNK > 1 << 22:
            raise SystemExit(f"not converged after {chunks * CHUNK} rounds")


def whole_call(mask, seeds, rounds, out):
    """One field from the seeds in as few calls as the op's 65535 rounds a call allow."""
    planes, left, status = None, rounds, None
    while left > 0:
        step = min(left, 65535)
        _, _, status = ops.mask_access(mask, seeds, COST, TERMINAL, 8, rounds=step, resume=planes, out=out if planes is None else None)
        planes, left = out, left - step
    return status


torch.set_grad_enabled(False)
open_field = np.zeros((1, H, W), np.uint8)
serpentine = np.zeros((1, H, W), np.uint8)
serpentine[0, 31::32] = 1                                                    # a wall of water under every corridor of 31 rows
for i, y in enumerate(range(31, H, 32)):
    serpentine[0, y, W - 31:] = 0 if i % 2 == 0 else 1                       # the gap: 31 pixels at alternating ends
    serpentine[0, y, :31] = 1 if i % 2 == 0 else 0
maps = [("open field, one seed in the middle", open_field, (W // 2, H // 2)), ("serpentine, corridors of 31 rows, seed in a corner", serpentine, (0, 0))]
tiles = (H // T) * (W // T)
px = H * W
say(f"clock before: {clocks()}")
say(f"ops.mask_access, {H} x {W}, K = 5, connectivity 8, with the origin plane; tile {T} x {T}: {tiles} tiles; medians of {SAMPLES} calls (min .. max)")
call_bytes = px * (1 + 1 + 8) + px * (8 + 4 + 4)                             # init: mask, seeds in, keys out; finish: keys in, d and origin out
tile_bytes = (T + 2) * (T + 2) * (8 + 1)
say(f"bytes: {call_bytes / 1e6:.1f} MB per call for the init and finish passes ({call_bytes / HBM_BYTES_PER_S * 1e6:.1f} us at 8.0 TB/s); per round {tiles * 4 / 1e3:.1f} kB of "
    f"flags, and per DIRTY tile {tile_bytes} B staged plus 8 B per lowered pixel written back (at most {T * T * 8} B); every tile dirty: "
    f"{tiles * (tile_bytes + T * T * 8) / 1e6:.1f} MB a round")
for name, host, (sx, sy) in maps:
    mask = torch.from_numpy(host).cuda()
    seeds = torch.zeros_like(mask)
    seeds[0, sy, sx] = 1
    lowered, chunks, valued, planes = rounds_needed(mask, seeds)
    rounds = lowered + 1
    out = (torch.empty_like(planes[0]), torch.empty_like(planes[1]))
    status = whole_call(mask, seeds, rounds, out)
    ok = bool(status[0, 0].item()) and torch.equal(out[0], planes[0]) and torch.equal(out[1], planes[1])
    med, lo, hi = timed(lambda: whole_call(mask, seeds, rounds, out))
    idle_med, idle_lo, idle_hi = timed(lambda: ops.mask_access(mask, seeds, COST, TERMINAL, 8, rounds=min(rounds, 65535), resume=out))
    reach = int((planes[0] != -1).sum().item())
    say(f"{name}: {lowered} rounds lowered a value ({chunks} chunks of {CHUNK} to find that), {valued} pixels with a value, largest cost {int(planes[0].max().item())}")
    say(f"    a whole call of {rounds} rounds: {med:.2f} ms ({lo:.2f} .. {hi:.2f}), {med / rounds * 1e3:.2f} us a round; converged and equal to the chunked planes: {ok}")
    say(f"    the same call resumed on the converged planes (round 0 every tile dirty, then every tile idle): {idle_med:.2f} ms ({idle_lo:.2f} .. {idle_hi:.2f}), "
        f"{idle_med / min(rounds, 65535) * 1e3:.2f} us a round")
    say(f"    pixels reached {reach}; bytes if every reached pixel were staged once per round it changed in: not measured (the dirty tiles per round are not counted)")
    if host is open_field:
        labels = ops.mask_regions(mask, 5, 8)
        _, counts, index = ops.region_table(mask, labels, 5, None, 128, 1024)
        res = (torch.empty((1, 5, 4), dtype=torch.int64, device="cuda"), torch.empty((1, 1024, 8), dtype=torch.int64, device="cuda"))
        t_med, t_lo, t_hi = timed(lambda: ops.region_access(mask, planes[0], planes[1], index, counts, 5, 1024, out=res), 20)
        floor = px * (1 + 4 + 4) / HBM_BYTES_PER_S * 1e3
        say(f"    ops.region_access on these planes: {t_med * 1e3:.1f} us ({t_lo * 1e3:.1f} .. {t_hi * 1e3:.1f}); {px * 9 / 1e6:.1f} MB, floor {floor * 1e3:.1f} us: {floor / t_med:.3f} of it")
say("(eager calls through the Python wrapper: the workspace allocation and the enqueue of every round are in the time; no graph, no counters.")
say(" The round count is the map's: an open field needs about one round per tile between the seed and the farthest corner, a corridor one per")
say(" tile border it crosses.)")
say(f"clock after: {clocks()}")
