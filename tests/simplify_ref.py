"""The outline simplification's definition (include/floodseg_test.h, outline_simplify) in plain Python and numpy, written
from the definition and not from the kernels: the classic RECURSIVE Douglas-Peucker on every ring, with a depth counter in the place of
the kernels' rounds.  Also the shared test cases."""
import ctypes
import sys

import numpy as np

import outlines_ref as oref

BG = oref.BG
MAX_COORD = 16384
MAX_CONTOURS, MAX_VERTICES = 4096, 32768                      # the caps of the cases: the defaults of region_outlines
TOLS = (0, 4, 16, 64)                                         # tol_q of 0, 0.5, 1 and 2 pixels


def keys(v, l, r):
    """The distance keys q of the interior vertices l + 1 .. r - 1 of the segment v[l] -> v[r] (index m is vertex 0 again), and L."""
    a, b, p = v[l], v[r % len(v)], v[l + 1:r]
    u, w = b - a, p - a
    length2 = int(u @ u)
    d2 = (w * w).sum(1)
    if length2 == 0:
        return d2, 0
    t = w @ u
    z = p - b
    cross = u[0] * w[:, 1] - u[1] * w[:, 0]
    return np.where(t <= 0, d2 * length2, np.where(t >= length2, (z * z).sum(1) * length2, cross * cross)), length2


def simplify_ring(ring, tol_q, max_rounds):
    """One ring [m, 2] -> (ascending indices of the kept vertices, the deepest level that split a segment, unconverged)."""
    v = np.clip(np.asarray(ring, np.int64), 0, MAX_COORD)
    m = len(v)
    kept, state = [0], dict(rounds=0, unconverged=False)

    def examine(l, r, depth):
        if r - l < 2:
            return
        if depth > max_rounds:                                # open after the last round: everything stays
            kept.extend(range(l + 1, r))
            state["unconverged"] = True
            return
        q, length2 = keys(v, l, r)
        at = int(np.argmax(q))                                # the first of the largest: the smallest index on a tie
        far = int(q[at])
        if depth >= 2 and not 16 * far > tol_q * length2:
            return
        if depth == 1 and not far > 0:
            return
        s = l + 1 + at
        kept.append(s)
        state["rounds"] = max(state["rounds"], depth)
        examine(l, s, depth + 1)
        examine(s, r, depth + 1)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, max_rounds + 200))
    try:
        examine(0, m, 0)
    finally:
        sys.setrecursionlimit(limit)
    return sorted(kept), state["rounds"], state["unconverged"]


def area2_of(v):
    v = np.asarray(v, np.int64)
    w = np.roll(v, -1, 0)
    return int((v[:, 0] * w[:, 1] - w[:, 0] * v[:, 1]).sum())


def frame_rows(contours, counts, f, max_vertices):
    """The rows of frame f when the frame is what region_outlines guarantees, else None."""
    _, rows, total, _ = (int(c) for c in counts[f])
    if not 0 <= rows <= contours.shape[1] or total > max_vertices:
        return None
    at, out = 0, []
    for _, off, m, _, _, _ in contours[f, :rows].tolist():
        if m < 3 or off != at:
            return None
        out.append((off, m))
        at += m
    return out if at <= total else None


def outline_simplify(contours, vertices, counts, tol_q, max_rounds):
    """(contours int64 [n,C,6], vertices int32 [n,V,2], counts int64 [n,4]) -> (simple int64 [n,C,4], simple_vertices int32 [n,V,2],
    simple_counts int64 [n,4])."""
    n, c, _ = contours.shape
    v = vertices.shape[1]
    simple = np.zeros((n, c, 4), np.int64)
    simple_vertices = np.zeros((n, v, 2), np.int32)
    simple_counts = np.zeros((n, 4), np.int64)
    for f in range(n):
        if int(counts[f, 3]) & 1:
            simple_counts[f, 3] = 2
            continue
        rows = frame_rows(contours, counts, f, v)
        if rows is None:
            simple_counts[f, 3] = 8
            continue
        at, deepest, flags = 0, 0, 4 if int(counts[f, 0]) > len(rows) else 0
        for k, (off, m) in enumerate(rows):
            ring = np.clip(vertices[f, off:off + m], 0, MAX_COORD)
            kept, rounds, unconverged = simplify_ring(ring, tol_q, max_rounds)
            simple_vertices[f, at:at + len(kept)] = ring[kept]
            simple[f, k] = (at, len(kept), area2_of(ring[kept]), int(unconverged))
            at += len(kept)
            deepest = max(deepest, rounds)
            flags |= int(unconverged)
        simple_counts[f] = (len(rows), at, deepest, flags)
    return simple, simple_vertices, simple_counts


def workspace_bytes(n, max_contours, max_vertices):
    """FS_OUTLINE_SIMPLIFY_WORKSPACE_BYTES, restated."""
    return n * 8 * (6 * max_vertices + ((max_vertices + 1023) // 1024 + 1) // 2 + (max_contours + 1) // 2 + 262)


# ------------------------------------------------------------------------------------------------ cases
def comb():
    """Rows 68-69 filled, and for i in 0..63 a tooth in column 2 i + 1 from row 67 - i down: one contour whose teeth grow along a diagonal."""
    m = np.full((70, 131), BG, np.uint8)
    m[68:70] = 0
    for i in range(64):
        m[67 - i:68, 2 * i + 1] = 0
    return m[None]


def blob():
    """A wavy ellipse with a round hole: what a water body looks like."""
    y, x = np.mgrid[0:96, 0:128].astype(np.float64)
    inside = (x - 64) ** 2 / 55 ** 2 + (y - 48) ** 2 / 40 ** 2 + 0.15 * np.sin(x / 5) * np.cos(y / 4) < 1
    inside &= ~((x - 70) ** 2 + (y - 50) ** 2 < 12 ** 2)
    return np.where(inside, 0, BG).astype(np.uint8)[None]


def cases():
    """{name: (name, mask [n,H,W], classes, max_regions)}: the outlines' shapes and the two of this file."""
    out = {c[0]: c for c in oref.gpu_cases()}
    out["comb"] = ("comb", comb(), 1, 4)
    out["blob"] = ("blob", blob(), 1, 4)
    return out


CASES = cases()
_EXPECTED = {}


def outlines_of(name, connectivity, max_contours=MAX_CONTOURS, max_vertices=MAX_VERTICES):
    """The outlines' reference for a case (shared, read-only): dict with index, contours, vertices, counts, ..."""
    return oref.expected(*CASES[name], connectivity, max_contours, max_vertices)


def expected(name, connectivity, tol_q, max_rounds, max_contours=MAX_CONTOURS, max_vertices=MAX_VERTICES):
    """The reference's three outputs for a case, computed once and shared."""
    key = (name, connectivity, tol_q, max_rounds, max_contours, max_vertices)
    if key not in _EXPECTED:
        e = outlines_of(name, connectivity, max_contours, max_vertices)
        got = outline_simplify(e["contours"], e["vertices"], e["counts"], tol_q, max_rounds)
        for a in got:
            a.setflags(write=False)
        _EXPECTED[key] = got
    return _EXPECTED[key]


def broken_frames():
    """(what, contours, vertices, counts, expected flag): the lake's outlines, each with one rule broken."""
    e = outlines_of("lake", 8, 8, 64)
    assert e["counts"].tolist() == [[6, 6, 24, 0]]

    def frame(change):
        c, v, n = (np.array(e[key]) for key in ("contours", "vertices", "counts"))
        change(c, v, n)
        return c, v, n

    def put(a, where, value):
        a[where] = value

    return [
        ("overflowed", *frame(lambda c, v, n: put(n, (0, 3), 1)), 2),
        ("overflowed and broken", *frame(lambda c, v, n: (put(n, (0, 3), 3), put(n, (0, 1), 99))), 2),
        ("more rows than the table holds", *frame(lambda c, v, n: put(n, (0, 1), 9)), 8),
        ("a negative row count", *frame(lambda c, v, n: put(n, (0, 1), -1)), 8),
        ("a total past the vertex cap", *frame(lambda c, v, n: put(n, (0, 2), 65)), 8),
        ("a count below 3", *frame(lambda c, v, n: (put(c, (0, 2, 2), 2), put(c, (0, 3, 1), 10))), 8),
        ("a negative count", *frame(lambda c, v, n: put(c, (0, 5, 2), -4)), 8),
        ("a huge count", *frame(lambda c, v, n: put(c, (0, 5, 2), 1 << 40)), 8),
        ("a gap between two rows", *frame(lambda c, v, n: put(c, (0, 3, 1), 13)), 8),
        ("two rows that overlap", *frame(lambda c, v, n: put(c, (0, 3, 1), 11)), 8),
        ("a first row that does not start at 0", *frame(lambda c, v, n: put(c, (0, 0, 1), 1)), 8),
        ("a last row past the total", *frame(lambda c, v, n: put(n, (0, 2), 23)), 8),
        ("a negative total", *frame(lambda c, v, n: put(n, (0, 2), -1)), 8),
    ]


# ------------------------------------------------------------------------------------------------ refusals
def refusal_cases():
    """(keyword overrides of a valid call, a word of the message)."""
    return [
        (dict(contours=0), "null"), (dict(vertices=0), "null"), (dict(counts=0), "null"), (dict(simple=0), "null"), (dict(simple_vertices=0), "null"),
        (dict(simple_counts=0), "null"), (dict(workspace=0), "null"),
        (dict(n=0), "frames"), (dict(n=65536), "65535"),
        (dict(max_contours=0), "max_contours"), (dict(max_contours=(1 << 20) + 1), "max_contours"),
        (dict(max_vertices=3), "max_vertices"), (dict(max_vertices=(1 << 22) + 1), "max_vertices"),
        (dict(tol_q=-1), "tol_q"), (dict(tol_q=(1 << 20) + 1), "tol_q"),
        (dict(max_rounds=0), "max_rounds"), (dict(max_rounds=257), "max_rounds"),
        (dict(workspace=0x1004), "aligned"),
    ]


def call_simplify(lib, **kw):
    """The library's outline_simplify with fake non-null pointers: only for calls that are refused before a launch."""
    a = dict(contours=0x1000, vertices=0x1000, counts=0x1000, n=1, max_contours=16, max_vertices=64, tol_q=16, max_rounds=32, simple=0x1000,
             simple_vertices=0x1000, simple_counts=0x1000, workspace=0x1000)
    a.update(kw)
    p = ctypes.c_void_p
    return lib.fs_outline_simplify(p(a["contours"]), p(a["vertices"]), p(a["counts"]), a["n"], a["max_contours"], a["max_vertices"], a["tol_q"],
                                   a["max_rounds"], p(a["simple"]), p(a["simple_vertices"]), p(a["simple_counts"]), p(a["workspace"]), p(0))
