"""The definition of the region ops (include/floodseg_test.h: mask_regions, region_table, region_filter) in plain
numpy, and the cases the CPU and the GPU tests share.  Nothing of the package's ops is imported here.

  mask        uint8 [n][H][W]; 1 <= K <= 255; connectivity 4 or 8
  background  id >= K: no region, label 0, index -1, never changed, never votes
  region      a maximal set of pixels of ONE frame with the same id < K, connected under the connectivity
  anchor      the region's first pixel in raster order;  label = 1 + (y_a * W + x_a)
  table       int64 [n][max_regions][10], rows in ascending anchor order:
              (class, area, x0, y0, x1, y1, sum_x, sum_y, conf_sum, low_pixels), box inclusive, the last two 0 without confidence
  counts      int64 [n][2] = (regions, rows written = min(regions, max_regions))
  index       int32 [n][H][W]: the row of the pixel's region, -1 for background and for regions beyond max_regions
  filter      a speckle = a region with a row and area < min_area takes the class with the most votes (lowest id on a tie, none: stays);
              a vote = (pixel p of the speckle, in-frame 4-neighbour q of p whose region has a row and area >= min_area), for q's class;
              votes read the input mask; one pass
"""
import functools

import numpy as np

TILE_H, TILE_W = 32, 64  # the labelling kernel's tile (csrc/region_uf.h): the corner pattern and the last two cases are placed against it
SEED = 20261

# (frames, H, W): the smallest frame; a single row / column; below one tile with odd sizes and three different frames; 3 x 3 and 5 x 2
# tiles of 32 x 64 with a remainder in both directions (70 = 2 * 32 + 6, 150 = 2 * 64 + 22, 130 = 4 * 32 + 2, 67 = 64 + 3); and 3 x 3
# tiles again at a width that is a multiple of 4 (152 = 2 * 64 + 24): the only case whose filter output takes the dword stores
CASES = [(1, 1, 1), (1, 1, 37), (1, 37, 1), (3, 17, 33), (2, 70, 150), (2, 130, 67), (2, 70, 152)]
PATTERNS = ["percolation", "random5", "spiral", "comb", "checker", "uniform", "stripes", "frames", "corners"]
MIN_AREAS = [0, 1, 2, 9, 10 ** 6]
OVERFLOW_CAP = 7


def pattern_classes(pattern):
    return 2 if pattern in ("percolation", "checker") else 5


def _spiral(h, w):
    """A one-pixel path that winds inwards through the whole frame, one pixel of the other class between its turns."""
    g = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    g[0, 0] = 1

    def free(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and g[yy, xx] == 0

    def can(dy, dx):
        ny, nx = y + dy, x + dx
        if not free(ny, nx):
            return False
        ay, ax = ny + dy, nx + dx                                   # the pixel beyond: an earlier turn there would make the path touch
        return not (0 <= ay < h and 0 <= ax < w and g[ay, ax] == 1)

    turns = 0
    while turns < 2:
        if can(dy, dx):
            y, x = y + dy, x + dx
            g[y, x] = 1
            turns = 0
        else:
            dy, dx = dx, -dy                                          # right turn
            turns += 1
    return g


@functools.lru_cache(maxsize=None)
def make_mask(case, pattern):
    n, h, w = CASES[case]
    rng = np.random.default_rng(SEED + 97 * case + PATTERNS.index(pattern))
    yy, xx = np.mgrid[0:h, 0:w]
    if pattern == "percolation":        # 59 % of one class: next to the site-percolation threshold, long tortuous regions
        m = (rng.random((n, h, w)) >= 0.59).astype(np.uint8)
    elif pattern == "random5":
        m = rng.integers(0, 5, (n, h, w), dtype=np.uint8)
    elif pattern == "spiral":
        m = np.stack([_spiral(h, w) * (1 + f) for f in range(n)]).astype(np.uint8)
    elif pattern == "comb":             # teeth in every other column that meet in the bottom row only
        m = np.broadcast_to(((xx % 2 == 0) | (yy == h - 1)).astype(np.uint8) * 3, (n, h, w)).copy()
    elif pattern == "checker":
        m = np.broadcast_to(((yy + xx) % 2).astype(np.uint8), (n, h, w)).copy()
    elif pattern == "uniform":
        m = np.full((n, h, w), 3, np.uint8)
    elif pattern == "stripes":          # ids >= K: rows of 200, columns of 5 (= K)
        m = rng.integers(0, 5, (n, h, w), dtype=np.uint8)
        m[:, yy[:, 0] % 7 == 3, :] = 200
        m[:, :, xx[0] % 11 == 5] = 5
    elif pattern == "frames":           # one class along the last rows of frame f and the first row of frame f + 1
        m = (rng.random((n, h, w)) < 0.3).astype(np.uint8)
        m[:, -2:, :] = 2
        m[:, 0, :] = 2
    elif pattern == "corners":          # contacts through a diagonal only, exactly on the tile corners (the frame's centre without one)
        m = np.zeros((n, h, w), np.uint8)
        corners = [(cy, cx) for cy in range(TILE_H, h, TILE_H) for cx in range(TILE_W, w, TILE_W)] or [(max(1, h // 2), max(1, w // 2))]
        for j, (cy, cx) in enumerate(corners):
            if cy < 1 or cx < 1 or cy >= h or cx >= w:
                continue
            if j % 2 == 0:
                m[:, cy - 1, cx - 1] = 1
                m[:, cy, cx] = 1
            else:
                m[:, cy - 1, cx] = 1
                m[:, cy, cx - 1] = 1
        m[1:, 0, 0] = 4
    else:
        raise ValueError(pattern)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def make_conf(case):
    n, h, w = CASES[case]
    c = np.random.default_rng(SEED + 7 + case).integers(0, 256, (n, h, w), dtype=np.uint8)
    c.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------ labels
def _label_frame(m, classes, connectivity):
    """Union-find over the whole frame: hook the larger root of every edge under the smaller one, compress, repeat until no edge
    joins two roots.  parent[i] <= i throughout, so a set's root is its smallest index: the anchor."""
    h, w = m.shape
    fg = m < classes
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    offsets = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    ea, eb = [], []
    for dy, dx in offsets:
        a = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
        b = (slice(dy, h), slice(max(0, dx), w + min(0, dx)))
        same = fg[a] & fg[b] & (m[a] == m[b])
        ea.append(idx[a][same])
        eb.append(idx[b][same])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = np.arange(h * w, dtype=np.int64)
    while True:
        pa, pb = parent[ea], parent[eb]
        lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
        if (lo == hi).all():
            break
        np.minimum.at(parent, hi, lo)
        while True:
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
    return np.where(fg, parent.reshape(h, w) + 1, 0).astype(np.int32)


def mask_regions(mask, classes, connectivity=8):
    assert mask.dtype == np.uint8 and mask.ndim == 3 and 1 <= classes <= 255 and connectivity in (4, 8)
    return np.stack([_label_frame(m, classes, connectivity) for m in mask])


def mask_regions_bfs(mask, classes, connectivity=8):
    """The same labels by a flood fill in raster order (slow: the cross-check of the small cases)."""
    n, h, w = mask.shape
    out = np.zeros((n, h, w), np.int32)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for f in range(n):
        m = mask[f]
        for y in range(h):
            for x in range(w):
                if m[y, x] >= classes or out[f, y, x]:
                    continue
                lab, stack = 1 + y * w + x, [(y, x)]
                out[f, y, x] = lab
                while stack:
                    cy, cx = stack.pop()
                    for dy, dx in nb:
                        qy, qx = cy + dy, cx + dx
                        if 0 <= qy < h and 0 <= qx < w and not out[f, qy, qx] and m[qy, qx] == m[y, x]:
                            out[f, qy, qx] = lab
                            stack.append((qy, qx))
    return out


# ------------------------------------------------------------------------------------------------ table
def region_table(mask, labels, classes, conf=None, low=128, max_regions=1024):
    n, h, w = mask.shape
    table = np.zeros((n, max_regions, 10), np.int64)
    counts = np.zeros((n, 2), np.int64)
    index = np.full((n, h, w), -1, np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    for f in range(n):
        lab = labels[f].astype(np.int64)
        anchors = np.unique(lab[lab > 0])                              # ascending labels = ascending anchors
        rows = min(len(anchors), max_regions)
        counts[f] = (len(anchors), rows)
        rank = np.searchsorted(anchors, lab)
        rank = np.where((lab > 0) & (rank < max_regions), rank, -1)
        index[f] = rank
        sel = rank >= 0
        r, y, x = rank[sel], yy[sel], xx[sel]
        t = table[f]
        t[:rows, 0] = mask[f].reshape(-1)[anchors[:rows] - 1]
        t[:, 1] = np.bincount(r, minlength=max_regions)
        big = np.iinfo(np.int64).max
        for col, val, fn, start in ((2, x, np.minimum, big), (3, y, np.minimum, big), (4, x, np.maximum, -1), (5, y, np.maximum, -1)):
            acc = np.full(max_regions, start, np.int64)
            fn.at(acc, r, val)
            t[:rows, col] = acc[:rows]
        t[:, 6] = np.bincount(r, weights=x, minlength=max_regions).astype(np.int64)
        t[:, 7] = np.bincount(r, weights=y, minlength=max_regions).astype(np.int64)
        if conf is not None:
            c = conf[f][sel].astype(np.int64)
            t[:, 8] = np.bincount(r, weights=c, minlength=max_regions).astype(np.int64)
            t[:, 9] = np.bincount(r, weights=(c < low), minlength=max_regions).astype(np.int64)
    return table, counts, index


# ------------------------------------------------------------------------------------------------ filter
def region_filter(mask, index, table, classes, min_area):
    n, h, w = mask.shape
    out = mask.copy()
    for f in range(n):
        idx, m = index[f].astype(np.int64), mask[f]
        has = idx >= 0
        area = np.where(has, table[f][np.maximum(idx, 0), 1], 0)
        speckle, voter = has & (area < min_area), has & (area >= min_area)
        votes = np.zeros((table.shape[1], classes), np.int64)
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            p = (slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx)))
            q = (slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx)))
            ok = speckle[p] & voter[q]
            np.add.at(votes, (idx[p][ok], m[q][ok].astype(np.int64)), 1)
        decided = votes.max(1) > 0
        choice = votes.argmax(1)                                       # the first maximum: the lowest class id on a tie
        take = speckle & decided[np.maximum(idx, 0)]
        out[f][take] = choice[idx[take]].astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def expected(case, pattern, connectivity):
    """Everything the tests compare against for one case, computed once: labels, then the table with and without confidence and with
    an overflowing cap, then the filtered masks.  cap = H * W + 1: above any possible number of regions."""
    mask, conf, k = make_mask(case, pattern), make_conf(case), pattern_classes(pattern)
    n, h, w = mask.shape
    cap = h * w + 1
    labels = mask_regions(mask, k, connectivity)
    full = region_table(mask, labels, k, conf, 100, cap)
    out = dict(mask=mask, conf=conf, classes=k, cap=cap, labels=labels, with_conf=full, without=region_table(mask, labels, k, None, 128, cap),
               overflow=region_table(mask, labels, k, conf, 100, OVERFLOW_CAP))
    out["filtered"] = {a: region_filter(mask, full[2], full[0], k, a) for a in MIN_AREAS}
    out["filtered_overflow"] = region_filter(mask, out["overflow"][2], out["overflow"][0], k, 9)
    return out


def partitions_equal(a, b):
    """Two label planes describe the same partition: the pairing of their labels is one to one (0 with 0)."""
    pairs = np.unique(np.stack([a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])) and ((pairs[:, 0] == 0) == (pairs[:, 1] == 0)).all()


# ------------------------------------------------------------------------------------------------ refusals
def refusal_cases():
    """(op, keyword overrides, a word of the message): every refusal the header lists, with fake non-null pointers."""
    sizes = [(dict(n=0), b">= 1"), (dict(H=0), b">= 1"), (dict(W=-1), b">= 1"), (dict(n=65536), b"65535"), (dict(K=0), b"out of range"),
             (dict(K=256), b"out of range"), (dict(H=46341, W=46341), b"2^31"), (dict(H=1, W=2 ** 31 - 1), b"2^31")]
    cap = [(dict(max_regions=0), b"max_regions"), (dict(max_regions=65537), b"max_regions")]
    return ([("mask_regions", kw, word) for kw, word in sizes + [(dict(mask=None), b"null"), (dict(labels=None), b"null"),
                                                                  (dict(connectivity=6), b"connectivity"), (dict(connectivity=0), b"connectivity"),
                                                                  (dict(H=2 ** 30, W=1), b"tiles"), (dict(H=1, W=2 ** 30 + 64), b"tiles")]]
            + [("region_table", kw, word) for kw, word in sizes + cap + [(dict(low=-1), b"low"), (dict(low=256), b"low")]
               + [(dict(**{name: None}), b"null") for name in ("mask", "labels", "table", "counts", "index", "workspace")]]
            + [("region_filter", kw, word) for kw, word in sizes + cap + [(dict(min_area=-1), b"min_area")]
               + [(dict(**{name: None}), b"null") for name in ("mask", "index", "table", "out", "votes")]])


def call_region_op(lib, op, **kw):
    """fs_<op> through the hook table with every argument a keyword; pointers default to a fake non-null address."""
    fake = 0x1000
    a = dict(mask=fake, labels=fake, conf=fake, table=fake, counts=fake, index=fake, workspace=fake, out=fake, votes=fake, n=2, H=8, W=8, K=5,
             connectivity=8, low=128, max_regions=16, min_area=4)
    a.update(kw)
    if op == "mask_regions":
        return lib.fs_mask_regions(a["mask"], a["n"], a["H"], a["W"], a["K"], a["connectivity"], a["labels"], None)
    if op == "region_table":
        return lib.fs_region_table(a["mask"], a["labels"], a["conf"], a["n"], a["H"], a["W"], a["K"], a["low"], a["max_regions"], a["table"],
                                   a["counts"], a["index"], a["workspace"], None)
    return lib.fs_region_filter(a["mask"], a["index"], a["table"], a["n"], a["H"], a["W"], a["K"], a["max_regions"], a["min_area"], a["out"],
                                a["votes"], None)


# ------------------------------------------------------------------------------------------------ the full-frame scene, in closed form
def lattice_scene(n=5, h=1072, w=1920):
    """A scene whose labels follow from its construction: K = 4, everything id 4 (background) except
      - a lattice of disjoint 10 x 15 rectangles, one per 16 x 24 cell at offset (3, 4), of class (i + j + f) % 3: label 1 + its corner;
      - one serpentine of class 3: every 16th row across the frame, joined at alternating ends: label 1 (it starts at pixel 0).
    Returns mask, labels, and per frame the number of regions."""
    assert h % 16 == 0 and w % 24 == 0
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx, i, j = yy % 16, xx % 24, yy // 16, xx // 24
    rect = (cy >= 3) & (cy < 13) & (cx >= 4) & (cx < 19)
    snake = (cy == 0) | ((xx == w - 1) & (i % 2 == 0) & (i < h // 16 - 1)) | ((xx == 0) & (i % 2 == 1) & (i < h // 16 - 1))
    mask = np.full((n, h, w), 4, np.uint8)
    labels = np.zeros((n, h, w), np.int32)
    corner = (i * 16 + 3) * w + j * 24 + 4 + 1
    for f in range(n):
        mask[f][rect] = ((i + j + f) % 3)[rect]
        mask[f][snake] = 3
        labels[f][rect] = corner[rect]
        labels[f][snake] = 1
    return mask, labels, (h // 16) * (w // 24) + 1
