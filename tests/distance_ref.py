"""The definition of the distance ops (include/floodseg_test.h: mask_distance, region_proximity) in plain numpy, and the
cases the CPU and the GPU tests share.  Nothing of the package's ops is imported here.

  source pixel  a pixel q of frame f with mask[f][q] < 32 and bit mask[f][q] of source_set set
  d2            uint32 [n][H][W]: min over the source pixels q of the SAME frame of (p.y - q.y)^2 + (p.x - q.x)^2; 0 on a source pixel;
                NONE = 0xFFFFFFFF in a frame without a source and, with R > 0, where the minimum exceeds R^2.  R never changes a value.
  nearest       int32 [n][H][W]: q.y * W + q.x of a minimising source pixel, the smallest raster index among several; -1 where d2 is NONE
  exposure      int64 [n][K][B]: pixels with mask == k and d2 <= thresholds[b]^2, for k in target_set (k < 32), else 0
  near          int64 [n][max_regions][8] = (min_d2, at_x, at_y, src_x, src_y, src_row, near_pixels, 0) per row of the region table;
                (-1, -1, -1, -1, -1, -1, 0, 0) for a row without a finite d2; zero at and behind counts[f][1]
"""
import functools

import numpy as np

import regions_ref as rref

NONE = 0xFFFFFFFF
K = 5
SEED = 20263
RADII = [0, 1, 2, 7, 32767]
SOURCE_SETS = [0b00010, 0b01010]                     # class 1 (water) alone; classes 1 and 3
TARGET_SET = 0b11001 | (1 << 7)                      # classes 0, 3, 4 and one that is no class
THRESHOLDS_8 = (0, 1, 2, 3, 5, 8, 13, 40)
THRESHOLDS_1 = (2,)
SMALL_CAP = 7

# the smallest frames that cross every boundary of a tiling: a single pixel, a single row / column, ragged in both axes (37 x 301, the
# siblings'), 67 x 120 and 130 x 257 (more than one and two 64-row chunks, a width above 256 by one), a row wider than a 1024-thread
# workgroup, a column longer than any chunk
GEOMETRIES = [(1, 1), (1, 9), (9, 1), (37, 301), (67, 120), (130, 257), (3, 1500), (1100, 5)]
# the frames of one call, by pattern: n = 1..3; an empty frame between two full ones; frames with different source counts
FRAME_SETS = [("random50", "none", "all"), ("corner0", "corner1", "corner2"), ("corner3",), ("row", "column", "checker"), ("ties", "corners"),
              ("random01", "random5", "random50")]


def is_source(mask, source_set):
    m = mask.astype(np.int64)
    return (m < 32) & (((source_set >> np.minimum(m, 31)) & 1) != 0)


# ------------------------------------------------------------------------------------------------ the definition, separable form
def column_rows(src):
    """bool [H][W] -> int64 [H][W]: per pixel the row of the nearest source of its own column, the upper one on a tie; -1 without one."""
    h, w = src.shape
    yy = np.arange(h, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(src, yy, -1), axis=0)
    big = 1 << 40
    down = np.minimum.accumulate(np.where(src, yy, big)[::-1], axis=0)[::-1]
    take_up = (up >= 0) & ((down >= big) | (yy - up <= down - yy))
    return np.where(take_up, up, np.where(down < big, down, -1))


def _frame_distance(src):
    h, w = src.shape
    rows = column_rows(src)
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                              # [x][x']
    best = np.empty((h, w), np.uint64)
    for y in range(h):
        r = rows[y]
        cost = dx2 + ((y - r) ** 2)[None, :]
        packed = (cost.astype(np.uint64) << np.uint64(32)) | (r * w + xs).astype(np.uint64)[None, :]   # (value, raster index): the tie rule
        packed = np.where((r >= 0)[None, :], packed, np.uint64(0xFFFFFFFFFFFFFFFF))
        best[y] = packed.min(axis=1)
    return best


def mask_distance(mask, source_set, max_dist=0):
    assert mask.dtype == np.uint8 and mask.ndim == 3 and 0 < source_set < 2 ** 32 and 0 <= max_dist <= 32767
    n, h, w = mask.shape
    d2 = np.empty((n, h, w), np.uint32)
    nearest = np.empty((n, h, w), np.int32)
    for f in range(n):
        best = _frame_distance(is_source(mask[f], source_set))
        none = best == np.uint64(0xFFFFFFFFFFFFFFFF)
        v = (best >> np.uint64(32)).astype(np.int64)
        if max_dist > 0:
            none |= v > max_dist * max_dist
        d2[f] = np.where(none, NONE, v).astype(np.uint32)
        nearest[f] = np.where(none, -1, (best & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return d2, nearest


def mask_distance_bruteforce(mask, source_set, max_dist=0):
    """Literally the definition: a minimum over all pairs (frames of at most 24 x 24)."""
    n, h, w = mask.shape
    assert h <= 24 and w <= 24
    d2 = np.full((n, h, w), NONE, np.uint32)
    nearest = np.full((n, h, w), -1, np.int32)
    for f in range(n):
        sources = [(qy, qx) for qy in range(h) for qx in range(w) if mask[f, qy, qx] < 32 and (source_set >> int(mask[f, qy, qx])) & 1]   # raster order
        for py in range(h):
            for px in range(w):
                best = None
                for qy, qx in sources:
                    v = (py - qy) ** 2 + (px - qx) ** 2
                    if best is None or v < best[0]:                        # strictly: the first in raster order stays on a tie
                        best = (v, qy * w + qx)
                if best is not None and (max_dist == 0 or best[0] <= max_dist ** 2):
                    d2[f, py, px], nearest[f, py, px] = best
    return d2, nearest


def capped(d2, nearest, max_dist):
    """What max_dist = R > 0 makes of the unbounded result: values above R^2 become NONE / -1, nothing else changes."""
    if max_dist == 0:
        return d2, nearest
    far = (d2 != NONE) & (d2.astype(np.int64) > max_dist * max_dist)
    return np.where(far, NONE, d2).astype(np.uint32), np.where(far, -1, nearest).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the tabulation, plain loops
def region_proximity(mask, d2, nearest, index, counts, classes, max_regions, target_set, thresholds):
    n, h, w = mask.shape
    b_count = len(thresholds)
    assert 1 <= b_count <= 8 and all(0 <= t <= 32767 for t in thresholds) and all(b > a for a, b in zip(thresholds, thresholds[1:]))
    exposure = np.zeros((n, classes, b_count), np.int64)
    near = np.zeros((n, max_regions, 8), np.int64)
    for f in range(n):
        rows = int(min(max(counts[f, 1], 0), max_regions))
        finite = d2[f] != NONE
        dist = d2[f].astype(np.int64)
        for k in range(min(classes, 32)):
            if (target_set >> k) & 1:
                for b, t in enumerate(thresholds):
                    exposure[f, k, b] = int(((mask[f] == k) & finite & (dist <= t * t)).sum())
        near[f, :rows, :6] = -1
        idx = index[f].reshape(-1).astype(np.int64)
        flat, fin = dist.reshape(-1), finite.reshape(-1)
        pixels = np.flatnonzero((idx >= 0) & (idx < rows) & fin)
        pixels = pixels[np.argsort(idx[pixels], kind="stable")]            # grouped by row, in raster order inside a row
        owners = idx[pixels]
        starts = np.flatnonzero(np.r_[True, owners[1:] != owners[:-1]]) if len(pixels) else []
        for a, b in zip(starts, list(starts[1:]) + [len(pixels)]):         # one table row after the other
            own = pixels[a:b]
            row = near[f, owners[a]]
            p = int(own[np.argmin(flat[own])])                             # the first minimum: the lowest raster index on a tie
            row[0], row[1], row[2] = flat[p], p % w, p // w
            row[6] = int((flat[own] <= thresholds[0] ** 2).sum())
            if nearest is not None:
                q = int(nearest[f].reshape(-1)[p])
                i = int(idx[q])
                row[3], row[4], row[5] = q % w, q // w, i if 0 <= i < rows else -1
    return exposure, near


# ------------------------------------------------------------------------------------------------ the shared cases
def tie_plane(h, w):
    """Two sources mirror-symmetric about the centre pixel (in x, in y where the frame has one column), a second pair about it the other
    way: every pixel of the axis between them has two or four nearest sources."""
    m = np.zeros((h, w), np.uint8)
    cy, cx = h // 2, w // 2
    for dy, dx in ((0, min(3, cx)), (min(2, cy), 0)):
        m[cy - dy, cx - dx] = 1
        m[cy + dy if cy + dy < h else cy - dy, cx + dx if cx + dx < w else cx - dx] = 1
    return m


def make_frame(pattern, h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((yy // 3 + xx // 5) % 2 * 2 + (yy + xx) % 2 * 2).astype(np.uint8)           # classes 0, 2 and 4: none of them a source
    if pattern == "none":
        pass
    elif pattern == "all":
        m[:] = 1
    elif pattern.startswith("corner") and pattern != "corners":
        j = int(pattern[6:])
        m[(h - 1) * (j // 2), (w - 1) * (j % 2)] = 1
    elif pattern == "corners":
        m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 1
    elif pattern == "row":
        m[(2 * h) // 3, :] = 1
    elif pattern == "column":
        m[:, w // 3] = 1
    elif pattern == "checker":
        m[(yy + xx) % 2 == 0] = 1
    elif pattern == "ties":
        t = tie_plane(h, w)
        m[t == 1] = 1
    elif pattern.startswith("random"):
        density = {"random01": 0.001, "random5": 0.05, "random50": 0.5}[pattern]
        m[rng.random((h, w)) < density] = 1
        other = rng.random((h, w))
        m[(other < 0.02) & (m != 1)] = 5                                   # ids that are no class: K, 32 + 1 (bit 1 must not wrap), 200
        m[(other >= 0.02) & (other < 0.04) & (m != 1)] = 33
        m[(other >= 0.04) & (other < 0.05) & (m != 1)] = 200
    else:
        raise ValueError(pattern)
    if pattern not in ("none", "all") and h * w > 1:
        m[h // 2, (w // 2 + 1) % w] = 3                                    # one pixel of class 3: the second source set differs from the first
    return m


@functools.lru_cache(maxsize=None)
def case_list():
    cases = []
    for g, (h, w) in enumerate(GEOMETRIES):
        for s, patterns in enumerate(FRAME_SETS):
            rng = np.random.default_rng(SEED + 31 * g + s)
            mask = np.stack([make_frame(p, h, w, rng) for p in patterns])
            mask.setflags(write=False)
            cases.append(dict(mask=mask, patterns=patterns, geometry=(h, w)))
    return cases


def _readonly(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def expected(i, source_set, max_dist=0):
    """(d2, nearest) of case i; the capped results are cut from the unbounded one (R never changes a value)."""
    if max_dist:
        return _readonly(*capped(*expected(i, source_set, 0), max_dist))
    return _readonly(*mask_distance(case_list()[i]["mask"], source_set, 0))


@functools.lru_cache(maxsize=None)
def region_tables(i):
    """(index, counts) of case i's masks at 8-connectivity with an ample cap and with SMALL_CAP rows: {cap: (index, counts)}."""
    mask = case_list()[i]["mask"]
    labels = rref.mask_regions(mask, K, 8)
    out = {}
    for cap in (ample_cap(i), SMALL_CAP):
        _, counts, index = rref.region_table(mask, labels, K, None, 128, cap)
        out[cap] = _readonly(index, counts)
    return out


def ample_cap(i):
    h, w = case_list()[i]["geometry"]
    return min(h * w + 1, 65536)


@functools.lru_cache(maxsize=None)
def expected_proximity(i, source_set, max_dist, cap, thresholds, with_nearest=True):
    d2, nearest = expected(i, source_set, max_dist)
    index, counts = region_tables(i)[cap]
    return _readonly(*region_proximity(case_list()[i]["mask"], d2, nearest if with_nearest else None, index, counts, K, cap, TARGET_SET, thresholds))


def workspace_bytes(n, h, w):
    return (n * ((h + 63) // 64) * w * 4 + n * h * w * 2 + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ refusals
def refusal_cases():
    """(op, keyword overrides, a word of the message): every refusal the header lists, with fake non-null pointers."""
    sizes = [(dict(n=0), b"at least one frame"), (dict(n=65536), b"65535"), (dict(H=0), b">= 1"), (dict(W=-1), b">= 1"),
             (dict(H=46341, W=46341), b"2^31"), (dict(H=32769), b"<= 32768"), (dict(W=32769), b"<= 32768")]
    distance = sizes + [(dict(mask=None), b"null"), (dict(d2=None), b"null"), (dict(workspace=None), b"null"), (dict(source_set=0), b"source_set"),
                        (dict(max_dist=-1), b"max_dist"), (dict(max_dist=32768), b"max_dist"), (dict(d2=0x1002), b"d2 is not aligned"),
                        (dict(nearest=0x1001), b"nearest is not aligned"), (dict(workspace=0x1002), b"workspace is not aligned")]
    proximity = sizes + [(dict(**{name: None}), b"null") for name in ("mask", "d2", "index", "counts", "thresholds", "exposure", "near")]
    proximity += [(dict(K=0), b"classes"), (dict(K=256), b"classes"), (dict(max_regions=0), b"max_regions"), (dict(max_regions=65537), b"max_regions"),
                  (dict(thresholds=()), b"thresholds, out of range"), (dict(thresholds=tuple(range(9))), b"thresholds, out of range"),
                  (dict(thresholds=(-1, 2)), b"thresholds[0]"), (dict(thresholds=(1, 32768)), b"thresholds[1]"), (dict(thresholds=(1, 1)), b"ascending"),
                  (dict(thresholds=(3, 2, 5)), b"ascending"), (dict(d2=0x1002), b"aligned to 4"), (dict(nearest=0x1002), b"aligned to 4"),
                  (dict(index=0x1001), b"aligned to 4"), (dict(counts=0x1004), b"aligned to 8"), (dict(exposure=0x1004), b"aligned to 8"),
                  (dict(near=0x1004), b"aligned to 8")]
    return [("mask_distance", kw, word) for kw, word in distance] + [("region_proximity", kw, word) for kw, word in proximity]


def call_distance_op(lib, op, **kw):
    """fs_<op> through the hook table with every argument a keyword; pointers default to a fake non-null address."""
    import ctypes

    fake = 0x1000
    a = dict(mask=fake, d2=fake, nearest=fake, workspace=fake, index=fake, counts=fake, exposure=fake, near=fake, n=2, H=8, W=8, K=5, source_set=2,
             max_dist=0, max_regions=16, target_set=24, thresholds=(1, 2, 4))
    a.update(kw)
    if op == "mask_distance":
        return lib.fs_mask_distance(a["mask"], a["n"], a["H"], a["W"], a["source_set"], a["max_dist"], a["d2"], a["nearest"], a["workspace"], None)
    thr = a["thresholds"]
    host = None if thr is None else (ctypes.c_int32 * max(len(thr), 1))(*thr)
    return lib.fs_region_proximity(a["mask"], a["d2"], a["nearest"], a["index"], a["counts"], a["n"], a["H"], a["W"], a["K"], a["max_regions"],
                                   a["target_set"], None if host is None else ctypes.cast(host, ctypes.c_void_p), 0 if thr is None else len(thr),
                                   a["exposure"], a["near"], None)
