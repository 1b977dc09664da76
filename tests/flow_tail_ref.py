"""The key-frame window tail as a definition: plain torch on the CPU in float64, no project kernel anywhere in this file.

  seg_tail_ref       flow/model.py:184-241 (as oracle/flow_oracle.predict_segmentation restates it) after the two decoder calls
  canvas_ref         the accumulation of flow/base.py:182-209: softmax over the classes of every crop, summed at its placement
  resize_argmax_ref  flow/base.py:275-276
  decided            the pixels at which an argmax may be compared at all: top value ahead of the second by more than a margin

All fp32 inputs (logits, grids, weights) convert to float64 exactly, so the reference differs from the kernels by the kernels' own
rounding alone.  `seg_tail_cpu32` is the SAME chain in fp32 on the CPU (ATen): its error against the float64 chain is the yardstick
the GPU tolerances are stated in (tests/test_gpu_flow_tail.py), and tests/test_flow_tail_cpu.py ties both to the oracle and to the
reference-generated golden.

The second half of the file is the committed table of test cases (geometries, seeds, inputs), shared by the CPU and the GPU test so
that what the CPU file asserts about a case (undecided share, fp32 error) holds for the inputs the GPU test runs."""
import functools

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------ the definition
def _up(t, h, w):
    if t.shape[2] != h or t.shape[3] != w:
        t = F.interpolate(t, size=(h, w), mode="bilinear", align_corners=True)
    return t


def _tail(lo_prev, lo_next, grids_left, grids_right, n, out_hw, no_warp, weights, dtype):
    def cast(t):
        return torch.as_tensor(t).detach().cpu().to(dtype)

    h, w = int(out_hw[0]), int(out_hw[1])
    o = _up(cast(lo_prev), h, w)
    if lo_next is None:
        return o
    o_next = _up(cast(lo_next), h, w)
    if no_warp:
        fwd, bwd = [o] * (n - 1), [o_next] * (n - 1)
    else:
        assert len(grids_left) == n - 1 and len(grids_right) == n - 1
        fwd, bwd = [], []
        for first, grids, acc in ((o, grids_left, fwd), (o_next, grids_right, bwd)):
            cur = first
            for g in grids:  # every later step samples the previous step's grid-resolution result
                cur = F.grid_sample(cur, cast(g), mode="bilinear", padding_mode="border", align_corners=False)
                acc.append(_up(cur, h, w))
    maps = [o]
    for f in range(1, n):
        a, b = fwd[f - 1], bwd[n - f - 1]
        if weights is None:
            maps.append((n - f) / n * a + f / n * b)
            continue
        wa, wb = float(weights[f][0]), float(weights[f][1])
        if wb == 0.0:    # a held frame is the other chain's value itself: no 0 * x term
            maps.append(a)
        elif wa == 0.0:
            maps.append(b)
        else:
            maps.append(wa * a + wb * b)
    return torch.cat(maps, 0)


def seg_tail_ref(lo_prev, lo_next, grids_left, grids_right, n, out_hw, no_warp, weights=None):
    """float64 logits [n | 1, K, H, W]."""
    return _tail(lo_prev, lo_next, grids_left, grids_right, n, out_hw, no_warp, weights, torch.float64)


def seg_tail_cpu32(lo_prev, lo_next, grids_left, grids_right, n, out_hw, no_warp, weights=None):
    """The same chain through ATen's fp32 CPU kernels: the yardstick, never the reference."""
    return _tail(lo_prev, lo_next, grids_left, grids_right, n, out_hw, no_warp, weights, torch.float32)


def canvas_ref(logit_sets, placements, canvas_hw):
    """(canvas_sum [n,K,H,W], count [H,W]) in float64; the finished canvas is canvas_sum / count (NaN where count == 0)."""
    n, k = logit_sets[0].shape[:2]
    canvas = torch.zeros((n, k, int(canvas_hw[0]), int(canvas_hw[1])), dtype=torch.float64)
    count = torch.zeros((int(canvas_hw[0]), int(canvas_hw[1])), dtype=torch.float64)
    for lo, (y0, x0) in zip(logit_sets, placements):
        h, w = lo.shape[2:]
        canvas[:, :, y0:y0 + h, x0:x0 + w] += torch.softmax(lo.double(), dim=1)
        count[y0:y0 + h, x0:x0 + w] += 1
    return canvas, count


def resize_argmax_ref(x, size):
    """(float64 F.interpolate(x, size, bilinear, align_corners=True), its first-index argmax)."""
    r = F.interpolate(torch.as_tensor(x).detach().cpu().double(), size=(int(size[0]), int(size[1])), mode="bilinear", align_corners=True)
    return r, r.max(1)[1]


def decided(ref, margin):
    """bool [n,H,W]: the float64 top value exceeds the second by more than `margin` (all true for K = 1)."""
    if ref.shape[1] == 1:
        return torch.ones((ref.shape[0],) + tuple(ref.shape[2:]), dtype=torch.bool)
    top = ref.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > margin


def max_rel(got, ref):
    """max |got - ref| / max |ref|, as conftest.rel_err (which the GPU test uses for the recorded figures)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


# ------------------------------------------------------------------------------------------ the committed cases
#        name      K   h   w  Hg  Wg   H    W   n  seed
TAIL_CASES = {
    "base":   (5,  9, 12,  5,  7, 33,  47,  5, 101),   # the common path
    "wide8":  (8,  7,  5,  3,  4, 19, 300,  3, 102),   # two x-blocks, the second partial; K = KMAX of the small instantiation
    "wide32": (32, 4,  6,  6,  4, 21, 258,  2, 103),   # K = 32, n = 2, 2 pixels in the second block
    "k9":     (9,  5,  5,  4,  4, 17,  23,  4, 104),   # first K of the 32-class instantiation
    "k1":     (1,  4,  4,  3,  3,  9,   9,  3, 105),   # mask all zeros
    "row":    (5,  1,  6,  1,  1, 17,  23,  2, 106),   # 1-row logits, 1 x 1 grid
    "col":    (6,  6,  1,  4,  9, 40,   1,  4, 307),   # W = 1 (scale 0), w = 1 (seed 107 left one of 160 pixels undecided)
    "dot":    (5,  3,  3,  2,  2,  1,   1,  3, 108),   # one output pixel
    "same":   (5, 12, 14, 12, 14, 12,  14,  3, 109),   # no resize anywhere
    "down":   (5, 20, 24, 30, 40, 10,  12,  3, 110),   # logits and grid larger than the frame
    "long":   (5,  6,  7,  4,  5, 18,  22, 25, 111),   # the reference's default frame_delta
    "one":    (5,  6,  7,  4,  5, 18,  22,  1, 112),   # both key frames, no grids
}
TAIL_MODES = ("warp", "no_warp", "single")
CANVAS_CASES = ("base", "wide8", "wide32", "k1", "col")
CUT_CASES = {"base": 2, "k9": 3}   # case -> the frame pair that carries the cut
TIE_CASES = ("base", "k9")         # one per K instantiation (KMAX = 8, KMAX = 32)
MARGIN = 1e-4                      # x max|ref|: the argmax is compared where the float64 top-2 gap exceeds it


def _plant_special(g, hs, ws):
    """Overwrite the first coordinates of one grid with -1, +1 and values that land exactly on integer source coordinates of an
    hs x ws source (align_corners=False: x = (g + 1) * size / 2 - 0.5 is the integer j at g = (2j + 1) / size - 1)."""
    flat = g.view(-1)  # (x, y) interleaved
    on = lambda j, size: (2 * j + 1) / size - 1.0  # noqa: E731
    vals = [-1.0, -1.0, 1.0, 1.0, on(0, ws), on(0, hs), on(ws // 2, ws), on(hs // 2, hs), on(ws - 1, ws), on(hs - 1, hs), -1.0, 1.0,
            1.0, -1.0]
    m = min(len(vals), flat.numel())
    flat[:m] = torch.tensor(vals[:m], dtype=g.dtype)


@functools.lru_cache(maxsize=None)
def tail_inputs(name, tie=False):
    """The fp32 inputs of one case (cached: treat as read-only).  tie: class 2 is a copy of class 0 in both key frames."""
    K, h, w, Hg, Wg, H, W, n, seed = TAIL_CASES[name]
    gen = torch.Generator().manual_seed(seed)
    lo_prev = torch.randn(1, K, h, w, generator=gen) * 3
    lo_next = torch.randn(1, K, h, w, generator=gen) * 3
    gl = [torch.rand(1, Hg, Wg, 2, generator=gen) * 2.6 - 1.3 for _ in range(n - 1)]
    gr = [torch.rand(1, Hg, Wg, 2, generator=gen) * 2.6 - 1.3 for _ in range(n - 1)]
    if gl:
        _plant_special(gl[0], H, W)          # step 0 samples the virtual H x W map
    if n > 2:
        _plant_special(gr[-1], Hg, Wg)       # a later step samples the previous Hg x Wg result
    if tie:
        lo_prev[:, 2] = lo_prev[:, 0]
        lo_next[:, 2] = lo_next[:, 0]
    return dict(name=name, K=K, n=n, out_hw=(H, W), lo_prev=lo_prev, lo_next=lo_next, gl=gl, gr=gr)


def swapped(inp):
    """A second, different crop of the same geometry: the two key frames and the two grid lists change places."""
    return dict(inp, lo_prev=inp["lo_next"], lo_next=inp["lo_prev"], gl=inp["gr"], gr=inp["gl"])


def tail_args(inp, mode):
    """(lo_prev, lo_next, grids_left, grids_right, n, out_hw, no_warp) of one mode, in seg_tail's order."""
    if mode == "single":
        return inp["lo_prev"], None, [], [], inp["n"], inp["out_hw"], False
    return inp["lo_prev"], inp["lo_next"], inp["gl"], inp["gr"], inp["n"], inp["out_hw"], mode == "no_warp"


def linear_rows(n):
    """The rows the unweighted entry point uses: (float)((double)(n - f) / n), (float)((double)f / n)."""
    return torch.tensor([[(n - f) / n, f / n] for f in range(n)], dtype=torch.float64).float()


def cut_rows(n, c):
    """tests/cut_ref.window_weights for one cut at the pair (c-1 -> c)."""
    import cut_ref

    return torch.from_numpy(cut_ref.window_weights([j == c for j in range(1, n + 1)], n)[0])


@functools.lru_cache(maxsize=None)
def tail_pair(name, mode, weights=None, tie=False, swap=False):
    """(float64 reference, fp32 torch-CPU chain) of one case and mode, computed once.  weights: None | "cut"."""
    inp = tail_inputs(name, tie)
    if swap:
        inp = swapped(inp)
    rows = cut_rows(inp["n"], CUT_CASES[name]) if weights == "cut" else None
    args = tail_args(inp, mode)
    return seg_tail_ref(*args, weights=rows), seg_tail_cpu32(*args, weights=rows)


def canvas_layout(name):
    """Canvas mode: a canvas a few pixels larger than the crop and two overlapping placements, the second one touching the
    bottom-right corner exactly."""
    H, W = TAIL_CASES[name][5], TAIL_CASES[name][6]
    return (H + 3, W + 4), [(1, 2 if W > 2 else 4), (3, 4)]


def canvas_pair(logit_pairs, placements, canvas_hw):
    """(canvas_ref of the float64 logits, the fp32 yardstick: fp32 torch.softmax of the fp32 CPU logits summed in float64, count)."""
    ref, count = canvas_ref([p[0] for p in logit_pairs], placements, canvas_hw)
    c32 = torch.zeros_like(ref)
    for (_, lo32), (y0, x0) in zip(logit_pairs, placements):
        h, w = lo32.shape[2:]
        c32[:, :, y0:y0 + h, x0:x0 + w] += torch.softmax(lo32, dim=1).double()
    return ref, c32, count


# crops_fuse: crops of 24 x 28 from 6 x 7 logits, 3 x 4 grids
CROP_HW, CROP_LO, CROP_GRID = (24, 28), (6, 7), (3, 4)
CROP_LAYOUTS = {
    #          canvas      crop offsets
    "four":   ((47, 55),  [(0, 0), (0, 27), (23, 0), (23, 27)]),                  # the four crops overlap in the one pixel (23, 27)
    "wide":   ((40, 300), [(0, 0), (16, 68), (8, 136), (3, 204), (16, 272)]),     # second x-block, five crops along it
    "whole":  ((24, 28),  [(0, 0)]),                                              # a single crop equal to the canvas
    "strip":  ((24, 60),  [(0, 0), (0, 32)]),                                     # columns 28..31 stay uncovered
}
CROP_KS, CROP_NS = (1, 5, 8), (1, 2, 5, 6, 11)   # n: one full chunk of 5 frames, a chunk plus one, two chunks plus one
# every (K, n, warp) on "four"; the other layouts at three (K, n) each, warp and no_warp
CROP_CASES = [("four", k, n, nw) for k in CROP_KS for n in CROP_NS for nw in (False, True)] + \
             [(lay, k, n, nw) for lay in ("wide", "whole", "strip") for k, n in ((5, 6), (8, 11), (1, 2)) for nw in (False, True)]
CROP_MARGIN = 1e-6   # absolute, on the crop-averaged probabilities


@functools.lru_cache(maxsize=None)
def crops_inputs(layout, K, n):
    canvas_hw, yx = CROP_LAYOUTS[layout]
    nc = len(yx)
    gen = torch.Generator().manual_seed(1000 + 100 * list(CROP_LAYOUTS).index(layout) + 11 * K + n)
    lo_prev = torch.randn(nc, K, *CROP_LO, generator=gen) * 3
    lo_next = torch.randn(nc, K, *CROP_LO, generator=gen) * 3
    grids = torch.rand(nc, 2 * (n - 1), *CROP_GRID, 2, generator=gen) * 2.6 - 1.3
    if n > 1:
        _plant_special(grids[0, 0], *CROP_HW)
    return dict(canvas_hw=canvas_hw, yx=yx, lo_prev=lo_prev, lo_next=lo_next, grids=grids)


@functools.lru_cache(maxsize=None)
def crops_pair(layout, K, n, no_warp):
    """(finished float64 canvas = canvas_ref / count, the fp32 yardstick / count, count)."""
    inp = crops_inputs(layout, K, n)
    pairs = []
    for c in range(len(inp["yx"])):
        gl = [inp["grids"][c, j][None] for j in range(n - 1)]
        gr = [inp["grids"][c, n - 1 + j][None] for j in range(n - 1)]
        args = (inp["lo_prev"][c:c + 1], inp["lo_next"][c:c + 1], gl, gr, n, CROP_HW, no_warp)
        pairs.append((seg_tail_ref(*args), seg_tail_cpu32(*args)))
    ref, c32, count = canvas_pair(pairs, inp["yx"], inp["canvas_hw"])
    return ref / count, c32 / count, count


# canvas_finish / canvas_resize_argmax / resize_argmax_u8
RESIZE_SIZES = {
    "up": ((13, 17), (29, 41)), "down": ((29, 41), (13, 17)), "identity": ((13, 17), (13, 17)),
    "Ho1": ((13, 17), (1, 41)), "Wo1": ((13, 17), (29, 1)), "Hi1": ((1, 17), (29, 41)),
}
RESIZE_KN = [(k, n) for k in (1, 5) for n in (1, 3)]
CANVAS_MARGIN = 1e-12   # x max|ref|: the canvas is resized in float64 on both sides


@functools.lru_cache(maxsize=None)
def resize_inputs(size, K, n):
    (hi, wi), _ = RESIZE_SIZES[size]
    gen = torch.Generator().manual_seed(2000 + 100 * list(RESIZE_SIZES).index(size) + 11 * K + n)
    logits = torch.randn(n, K, hi, wi, generator=gen) * 3
    canvas = torch.rand(n, K, hi, wi, generator=gen, dtype=torch.float64) * 3
    count = torch.randint(1, 4, (hi, wi), generator=gen).double()
    return logits, canvas, count


def undecided_share(ref, margin):
    return 1.0 - decided(ref, margin).double().mean().item()
