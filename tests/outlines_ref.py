"""The region outlines' definition (include/floodseg_test.h, region_outlines) in plain Python and numpy, written from
the definition and not from the kernels: enumerate the cracks, map every corner to the cracks that start there, apply the successor
rule, walk every cycle, and build the four outputs with both overflow rules.  Also the shared test cases."""
import ctypes

import numpy as np

import regions_ref as rref

BG = 255
# per d: the neighbour across the edge (dx, dy), the start corner and the end corner relative to the pixel
ACROSS = ((0, -1), (1, 0), (0, 1), (-1, 0))
START = ((0, 0), (1, 0), (1, 1), (0, 1))
END = ((1, 0), (1, 1), (0, 1), (0, 0))


def outline_frame(index, max_regions, connectivity):
    """One index plane -> the list of its contours in contour order: dicts with region, anchor, cracks, vertices [(X, Y)], area2."""
    h, w = index.shape
    idx = np.where((index >= 0) & (index < max_regions), index, -1).astype(np.int64)

    def at(x, y):
        return int(idx[y, x]) if 0 <= x < w and 0 <= y < h else -1

    cracks = {}                                               # slot -> (region, x, y, d)
    starting = {}                                             # (corner, region) -> [slot]
    for y in range(h):
        for x in range(w):
            r = at(x, y)
            if r < 0:
                continue
            for d in range(4):
                if at(x + ACROSS[d][0], y + ACROSS[d][1]) != r:
                    slot = 4 * (y * w + x) + d
                    cracks[slot] = (r, x, y, d)
                    starting.setdefault(((x + START[d][0], y + START[d][1]), r), []).append(slot)
    succ = {}
    for slot, (r, x, y, d) in cracks.items():
        cand = starting[((x + END[d][0], y + END[d][1]), r)]
        if len(cand) == 1:
            succ[slot] = cand[0]
        else:                                                 # a saddle: left turn at 8, right turn at 4
            assert len(cand) == 2
            want = (d + 3) % 4 if connectivity == 8 else (d + 1) % 4
            (succ[slot],) = [c for c in cand if c % 4 == want]
    assert sorted(succ.values()) == sorted(cracks)            # a permutation
    seen, contours = set(), []
    for first in sorted(cracks):
        if first in seen:
            continue
        cycle, cur = [], first
        while cur not in seen:
            seen.add(cur)
            cycle.append(cur)
            cur = succ[cur]
        starts = [k for k in range(len(cycle)) if cycle[k - 1] % 4 != cycle[k] % 4]
        anchor = min(cycle[k] for k in starts)
        k0 = cycle.index(anchor)
        order = [k for k in starts if k >= k0] + [k for k in starts if k < k0]
        verts = []
        for k in order:
            r, x, y, d = cracks[cycle[k]]
            verts.append((x + START[d][0], y + START[d][1]))
        area2 = sum(verts[i][0] * verts[(i + 1) % len(verts)][1] - verts[(i + 1) % len(verts)][0] * verts[i][1] for i in range(len(verts)))
        contours.append(dict(region=cracks[anchor][0], anchor=anchor, cracks=len(cycle), vertices=verts, area2=area2))
    contours.sort(key=lambda c: c["anchor"])
    return contours


def region_outlines(index, max_regions, connectivity=8, max_contours=4096, max_vertices=32768):
    """index int32 [n,H,W] -> (contours int64 [n,max_contours,6], vertices int32 [n,max_vertices,2], shape int64 [n,R,3], counts int64 [n,4])."""
    n = index.shape[0]
    contours = np.zeros((n, max_contours, 6), np.int64)
    vertices = np.zeros((n, max_vertices, 2), np.int32)
    shape = np.zeros((n, max_regions, 3), np.int64)
    counts = np.zeros((n, 4), np.int64)
    for f in range(n):
        found = outline_frame(index[f], max_regions, connectivity)
        total = sum(len(c["vertices"]) for c in found)
        for c in found:
            shape[f, c["region"]] += (c["cracks"], 1, len(c["vertices"]))
        if total > max_vertices:                              # flag bit 0: nothing rather than a part
            shape[f, shape[f, :, 0] > 0, 1] = -1
            counts[f] = (0, 0, total, 1)
            continue
        off = 0
        for k, c in enumerate(found):
            if k < max_contours:
                contours[f, k] = (c["region"], off, len(c["vertices"]), c["cracks"], c["area2"], c["anchor"])
            vertices[f, off:off + len(c["vertices"])] = c["vertices"]
            off += len(c["vertices"])
        counts[f] = (len(found), min(len(found), max_contours), total, 2 if len(found) > max_contours else 0)
    return contours, vertices, shape, counts


def workspace_bytes(n, h, w, max_regions, max_contours, max_vertices):
    """FS_REGION_OUTLINES_WORKSPACE_BYTES, restated."""
    v = max_vertices
    return n * 8 * (2 * v + 7 * ((v + 1) // 2) + ((h * w + 1023) // 1024 + 1) // 2 + (v + 1023) // 1024 + 2)


def rings_of(contours, vertices, counts, f):
    """Frame f of a result -> {region row: [ring, ...]}, each ring a list of (X, Y), the outer contour first, then the holes."""
    out = {}
    for row in contours[f, :int(counts[f, 1])]:
        ring = [tuple(int(v) for v in p) for p in vertices[f, int(row[1]):int(row[1] + row[2])]]
        if row[4] > 0:
            out.setdefault(int(row[0]), []).insert(0, ring)
        else:
            out.setdefault(int(row[0]), []).append(ring)
    return out


# ------------------------------------------------------------------------------------------------ cases
def tables_of(mask, classes, connectivity, cap):
    """mask uint8 [n,H,W] -> (table, counts, index) by the regions' numpy definition."""
    labels = rref.mask_regions(mask, classes, connectivity)
    return rref.region_table(mask, labels, classes, None, 128, cap)


def _frame(rows):
    return np.array([[BG if c == "." else int(c) for c in row] for row in rows], np.uint8)[None]


def serpentine(h=64, w=130):
    """One simply connected region with a very long outline: every third row is a full spine, one-pixel teeth hang below it at every
    second column, and column 0 joins the spines -- several thousand vertices on ONE contour, the same at both connectivities."""
    m = np.full((h, w), BG, np.uint8)
    m[0::3] = 0
    m[1::3, 0::2] = 0
    m[2::3, 0] = 0
    return m[None]


def hand_cases():
    """(name, mask [1,H,W], classes): the cases the tests know the answers of."""
    lake = np.zeros((9, 7), np.uint8)
    lake[1:6, 1:6] = 1
    lake[2:5, 2:5] = BG
    lake[3, 3] = 0
    lake[7, 3] = BG
    return [
        ("pixel", _frame(["0"]), 1),
        ("ring", _frame([".....", ".111.", ".1.1.", ".111.", "....."]), 2),
        ("diagonal", _frame(["0.", ".0"]), 1),
        ("diagonal_hole", _frame(["0000", "0.00", "00.0", "0000"]), 1),
        ("lake", lake[None], 2),
    ]


def random_mask(n, h, w, seed, classes=3, background=0.2, smooth=True):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, classes, (n, h, w)).astype(np.uint8)
    if smooth:                                                # larger bodies: repeat a coarse field
        coarse = rng.integers(0, classes, (n, -(-h // 3), -(-w // 3))).astype(np.uint8)
        big = np.repeat(np.repeat(coarse, 3, 1), 3, 2)[:, :h, :w]
        m = np.where(rng.random((n, h, w)) < 0.7, big, m)
    m[rng.random((n, h, w)) < background] = BG
    return m


def gpu_cases():
    """(name, mask [n,H,W], classes, max_regions): the shapes of tests/test_gpu_outlines.py; the cap holds every region unless the name
    says otherwise."""
    full = np.zeros((1, 40, 300), np.uint8)
    full[0, 5:35:6, 10:290] = BG                              # slits: holes longer than a workgroup is wide
    checker = (np.indices((32, 32)).sum(0) % 2).astype(np.uint8)[None]
    checker = np.where(checker == 1, BG, 0).astype(np.uint8)
    out = [
        ("1x1", _frame(["0"]), 1, 4),
        ("1x7", _frame(["01.0011"]), 2, 8),
        ("5x1", _frame(["0", "0", ".", "1", "0"]), 2, 8),
        ("33x67", random_mask(1, 33, 67, 11), 3, 1024),
        ("40x300", full, 1, 16),
        ("serpentine", serpentine(), 1, 4),
        ("checker", checker, 1, 1024),
        ("n3", random_mask(3, 21, 45, 12), 3, 1024),
        ("capped", random_mask(1, 33, 67, 13, smooth=False), 3, 40),
    ]
    return out + [(name, mask, k, 16) for name, mask, k in hand_cases()]


_EXPECTED = {}


def expected(name, mask, classes, cap, connectivity, max_contours=4096, max_vertices=32768):
    """The reference's result for a case, computed once and shared: dict with index, table, counts and the four outputs."""
    key = (name, connectivity, max_contours, max_vertices)
    if key not in _EXPECTED:
        table, tcounts, index = tables_of(mask, classes, connectivity, cap)
        got = region_outlines(index, cap, connectivity, max_contours, max_vertices)
        for a in (table, tcounts, index) + got:
            a.setflags(write=False)
        _EXPECTED[key] = dict(index=index, table=table, tcounts=tcounts, contours=got[0], vertices=got[1], shape=got[2], counts=got[3])
    return _EXPECTED[key]


# ------------------------------------------------------------------------------------------------ refusals
def refusal_cases():
    """(keyword overrides of a valid call, a word of the message)."""
    return [
        (dict(index=0), "null"), (dict(contours=0), "null"), (dict(vertices=0), "null"), (dict(shape=0), "null"), (dict(counts=0), "null"),
        (dict(workspace=0), "null"),
        (dict(n=0), "sizes"), (dict(H=0), "sizes"), (dict(W=0), "sizes"), (dict(n=65536), "65535"),
        (dict(H=1 << 15, W=1 << 14), "2^29"),
        (dict(max_regions=0), "max_regions"), (dict(max_regions=65537), "max_regions"),
        (dict(connectivity=6), "connectivity"), (dict(connectivity=0), "connectivity"),
        (dict(max_contours=0), "max_contours"), (dict(max_contours=(1 << 20) + 1), "max_contours"),
        (dict(max_vertices=3), "max_vertices"), (dict(max_vertices=(1 << 22) + 1), "max_vertices"),
        (dict(workspace=0x1004), "aligned"),
    ]


def call_outlines(lib, **kw):
    """The library's region_outlines with fake non-null pointers: only for calls that are refused before a launch."""
    a = dict(index=0x1000, n=1, H=8, W=8, max_regions=16, connectivity=8, max_contours=16, max_vertices=64, contours=0x1000, vertices=0x1000,
             shape=0x1000, counts=0x1000, workspace=0x1000)
    a.update(kw)
    p = ctypes.c_void_p
    return lib.fs_region_outlines(p(a["index"]), a["n"], a["H"], a["W"], a["max_regions"], a["connectivity"], a["max_contours"], a["max_vertices"],
                                  p(a["contours"]), p(a["vertices"]), p(a["shape"]), p(a["counts"]), p(a["workspace"]), p(0))
