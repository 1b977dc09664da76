"""The rules of georeferencing the mosaic (csrc/ground_defs.h; include/floodseg_test.h: ground_area, ground_rectify, ground_points; DESIGN
§3.26) restated in numpy, twice: vectorised (area, rectify, points) and as literal loops over Python floats and ints (area_loops,
rectify_loops, points_loops).  Python floats and numpy float64 are IEEE doubles and neither contracts a product into a sum, so both
forms round as the header does.  Also here: the models and cases the tests share, the boundary shoelace taken crack by crack in exact
integers, and the header's bounds restated (check_forward, check_inverse)."""
import functools
import math

import numpy as np

TW, TH = 64, 16                # the tile of csrc/ground_ops.hip
UNSEEN = 255
NO_POINT = -2 ** 63            # FS_GROUND_NO_POINT
MAX_MM, MAX_STEP, MAX_RATIO, MAX_AREA2 = 2.0 ** 31, 2.0 ** 30, 4.0, 2.0 ** 62
REFUSALS = ("ok", "not finite", "denominator", "ratio", "range", "step", "area", "orientation")


# ------------------------------------------------------------------------------------------------ the corner rule
def project(m, i, j):
    """The three sums and two divisions, vectorised: float64 arrays in, float64 quotients out."""
    i, j = np.asarray(i, np.float64), np.asarray(j, np.float64)
    with np.errstate(all="ignore"):
        nu = (m[0] * i + m[1] * j) + m[2]
        nv = (m[3] * i + m[4] * j) + m[5]
        d = (m[6] * i + m[7] * j) + m[8]
        return nu / d, nv / d, d


def corner(fwd, i, j):
    """Lattice points (i, j) in anchor coordinates -> int64 (E, N) millimetres."""
    qe, qn, _ = project(fwd, i, j)
    return np.floor(qe + 0.5).astype(np.int64), np.floor(qn + 0.5).astype(np.int64)


def corner_literal(fwd, i, j):
    a0, a1, a2, b0, b1, b2, c0, c1, c2 = (float(v) for v in fwd)
    i, j = float(i), float(j)
    ne = (a0 * i + a1 * j) + a2
    nn = (b0 * i + b1 * j) + b2
    d = (c0 * i + c1 * j) + c2
    return math.floor(ne / d + 0.5), math.floor(nn / d + 0.5)


def orientation(m):
    m = [float(v) for v in m]
    det = (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])
    return 1 if det > 0 else -1 if det < 0 else 0


def invert(fwd):
    """The inverse model as the host hands it to the library: numpy.linalg.inv of the forward 3 x 3, as it is."""
    return np.linalg.inv(np.asarray(fwd, np.float64).reshape(3, 3)).reshape(-1)


# ------------------------------------------------------------------------------------------------ the bounds
def _denominators(m, x0, y0, x1, y1):
    d = [(m[6] * x + m[7] * y) + m[8] for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    if not all(v > 0 for v in d):
        return 2, None
    if not max(d) <= MAX_RATIO * min(d):
        return 3, None
    return 0, min(d)


def check_forward(m, size, origin):
    """csrc/ground_defs.h's check_forward -> the index into REFUSALS."""
    m = [float(v) for v in m]
    (ch, cw), (oy, ox) = size, origin
    if not all(math.isfinite(v) for v in m):
        return 1
    if orientation(m) == 0:
        return 7
    x0, y0, x1, y1 = float(-ox), float(-oy), float(cw - ox), float(ch - oy)
    r, dmin = _denominators(m, x0, y0, x1, y1)
    if r:
        return r
    pts = [tuple(float(v) for v in project(m, x, y)[:2]) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    if not all(abs(e) < MAX_MM - 1 and abs(n) < MAX_MM - 1 for e, n in pts):
        return 4
    emax, nmax = max(abs(e) for e, _ in pts), max(abs(n) for _, n in pts)
    step_e = ((abs(m[0]) + emax * abs(m[6])) + (abs(m[1]) + emax * abs(m[7]))) / dmin
    step_n = ((abs(m[3]) + nmax * abs(m[6])) + (abs(m[4]) + nmax * abs(m[7]))) / dmin
    if not (step_e + 1 < MAX_STEP and step_n + 1 < MAX_STEP):
        return 5
    quad = 0.0
    for k in range(4):
        quad += pts[k][0] * pts[(k + 1) & 3][1] - pts[(k + 1) & 3][0] * pts[k][1]
    return 0 if abs(quad) < MAX_AREA2 else 6


def check_inverse(m, raster_size, gsd_mm, top_left_mm):
    m = [float(v) for v in m]
    (gh, gw), (e0, ntop) = raster_size, top_left_mm
    if not all(math.isfinite(v) for v in m):
        return 1
    return _denominators(m, float(e0), float(ntop - gh * gsd_mm), float(e0 + gw * gsd_mm), float(ntop))[0]


# ------------------------------------------------------------------------------------------------ ground_area
def lattice(fwd, size, origin):
    """Every lattice corner of the canvas -> int64 E, N [CH+1, CW+1]."""
    (ch, cw), (oy, ox) = size, origin
    ys, xs = np.mgrid[0:ch + 1, 0:cw + 1]
    return corner(fwd, xs - ox, ys - oy)


def pixel_area2(fwd, size, origin):
    """Every pixel's oriented area2, int64 [CH, CW]."""
    e, n = lattice(fwd, size, origin)
    e0, n0 = e[:-1, :-1], n[:-1, :-1]
    ux, uy = e[:-1, 1:] - e0, n[:-1, 1:] - n0
    vx, vy = e[1:, 1:] - e0, n[1:, 1:] - n0
    wx, wy = e[1:, :-1] - e0, n[1:, :-1] - n0
    return ((ux * vy - uy * vx) + (vx * wy - vy * wx)) * orientation(fwd)


def area(cls, fwd, origin, classes, index=None, max_regions=0):
    a = pixel_area2(fwd, cls.shape, origin)
    valid = cls < classes
    summed = valid & (a > 0)
    class_area2, region_area2 = np.zeros(classes, np.int64), np.zeros(max_regions, np.int64)
    np.add.at(class_area2, cls[summed].astype(np.int64), a[summed])
    if index is not None:
        rows = summed & (index >= 0) & (index < max_regions)
        np.add.at(region_area2, index[rows].astype(np.int64), a[rows])
    counts = np.array([summed.sum(), (valid & (a <= 0)).sum(), ((cls >= classes) & (cls != UNSEEN)).sum(), 0], np.int64)
    return class_area2, region_area2, counts


def area_loops(cls, fwd, origin, classes, index=None, max_regions=0):
    ch, cw = cls.shape
    oy, ox = origin
    sign = orientation(fwd)
    class_area2, region_area2, counts = [0] * classes, [0] * max_regions, [0, 0, 0, 0]
    for y in range(ch):
        for x in range(cw):
            c = int(cls[y, x])
            if c == UNSEEN:
                continue
            if c >= classes:
                counts[2] += 1
                continue
            p = [corner_literal(fwd, i - ox, j - oy) for i, j in ((x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1))]
            ux, uy, vx, vy, wx, wy = p[1][0] - p[0][0], p[1][1] - p[0][1], p[2][0] - p[0][0], p[2][1] - p[0][1], p[3][0] - p[0][0], p[3][1] - p[0][1]
            a = ((ux * vy - uy * vx) + (vx * wy - vy * wx)) * sign
            if a <= 0:
                counts[1] += 1
                continue
            counts[0] += 1
            class_area2[c] += a
            if index is not None and 0 <= int(index[y, x]) < max_regions:
                region_area2[int(index[y, x])] += a
    return np.array(class_area2, np.int64), np.array(region_area2, np.int64), np.array(counts, np.int64)


def boundary_shoelace(inside, fwd, origin):
    """The shoelace of a pixel set's boundary taken crack by crack, in exact Python integers about the absolute corners: every crack
    between a pixel of the set and one outside it (or the canvas edge), walked in the direction the pixel's own corner order walks it.
    -> twice the signed area in mm^2, NOT oriented."""
    ch, cw = inside.shape
    e, n = lattice(fwd, inside.shape, origin)
    at = lambda x, y: (int(e[y, x]), int(n[y, x]))  # noqa: E731
    has = lambda x, y: 0 <= x < cw and 0 <= y < ch and bool(inside[y, x])  # noqa: E731
    total = 0
    for y in range(ch):
        for x in range(cw):
            if not inside[y, x]:
                continue
            for (nx, ny), a, b in (((x, y - 1), (x, y), (x + 1, y)), ((x + 1, y), (x + 1, y), (x + 1, y + 1)), ((x, y + 1), (x + 1, y + 1), (x, y + 1)),
                                   ((x - 1, y), (x, y + 1), (x, y))):
                if not has(nx, ny):
                    (ax, ay), (bx, by) = at(*a), at(*b)
                    total += ax * by - ay * bx
    return total


def polygon_shoelace(e, n):
    """A closed ring's doubled signed area in exact Python integers."""
    e, n = [int(v) for v in e], [int(v) for v in n]
    return sum(e[k] * n[(k + 1) % len(e)] - e[(k + 1) % len(e)] * n[k] for k in range(len(e)))


# ------------------------------------------------------------------------------------------------ ground_points
def points(pts, fwd, origin):
    pts = np.asarray(pts, np.int64)
    oy, ox = origin
    ok = (np.abs(pts) <= 1 << 20).all(axis=1)
    x, y = np.where(ok, pts[:, 0], 0), np.where(ok, pts[:, 1], 0)
    qe, qn, d = project(fwd, x - ox, y - oy)
    with np.errstate(all="ignore"):
        re, rn = np.floor(qe + 0.5), np.floor(qn + 0.5)
        ok &= (d > 0) & (np.abs(re) < 2.0 ** 53) & (np.abs(rn) < 2.0 ** 53)
    out = np.full((len(pts), 2), NO_POINT, np.int64)
    out[ok, 0], out[ok, 1] = re[ok].astype(np.int64), rn[ok].astype(np.int64)
    return out


def points_loops(pts, fwd, origin):
    oy, ox = origin
    out = []
    for x, y in np.asarray(pts).tolist():
        row = [NO_POINT, NO_POINT]
        if abs(x) <= 1 << 20 and abs(y) <= 1 << 20:
            i, j = float(x - ox), float(y - oy)
            d = (fwd[6] * i + fwd[7] * j) + fwd[8]
            if d > 0:
                e, n = corner_literal(fwd, x - ox, y - oy)
                if abs(e) < 2 ** 53 and abs(n) < 2 ** 53:
                    row = [e, n]
        out.append(row)
    return np.array(out, np.int64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ ground_rectify
def _blend(t, wx, wy, shift):
    c = [(v >> shift) & 0xFF for v in t]
    ax, ay = 256 - wx, 256 - wy
    return (ax * ay * c[0] + wx * ay * c[1] + ax * wy * c[2] + wx * wy * c[3] + 32768) >> 16


def rectify(inv, origin, size, raster_size, gsd_mm, top_left_mm, planes=(), rgba=None, fill=255, rgb_fill=(0, 0, 0)):
    """-> ([uint8 [GH, GW] per plane], uint8 [GH, GW, 3] or None).  size = (CH, CW) of the canvas; rgba: uint32 words."""
    (ch, cw), (oy, ox), (gh, gw), (e0, ntop) = size, origin, raster_size, top_left_mm
    v, u = np.mgrid[0:gh, 0:gw]
    eg = float(e0) + (u + 0.5) * float(gsd_mm)
    ng = float(ntop) - (v + 0.5) * float(gsd_mm)
    x, y, _ = project(inv, eg, ng)
    with np.errstate(all="ignore"):
        placed = (np.abs(x) < 2.0 ** 20) & (np.abs(y) < 2.0 ** 20)
    x, y = np.where(placed, x, 0.0), np.where(placed, y, 0.0)
    nx, ny = np.floor(x).astype(np.int64) + ox, np.floor(y).astype(np.int64) + oy
    on = placed & (nx >= 0) & (nx < cw) & (ny >= 0) & (ny < ch)
    cx, cy = np.clip(nx, 0, cw - 1), np.clip(ny, 0, ch - 1)
    outs = [np.where(on, p[cy, cx], fill).astype(np.uint8) for p in planes]
    if rgba is None:
        return outs, None
    words = rgba.astype(np.int64) & 0xFFFFFFFF

    def tap(tx, ty):
        inside = (tx >= 0) & (tx < cw) & (ty >= 0) & (ty < ch)
        return np.where(inside, words[np.clip(ty, 0, ch - 1), np.clip(tx, 0, cw - 1)], 0)

    sx, sy = x - 0.5, y - 0.5
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = np.floor((sx - fx) * 256.0).astype(np.int64), np.floor((sy - fy) * 256.0).astype(np.int64)
    x0, y0 = fx.astype(np.int64) + ox, fy.astype(np.int64) + oy
    t = [tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)]
    every = np.logical_and.reduce([(w >> 24) != 0 for w in t])
    near = tap(nx, ny)
    word = int(rgb_fill[0]) | int(rgb_fill[1]) << 8 | int(rgb_fill[2]) << 16
    rgb = np.empty((gh, gw, 3), np.uint8)
    for ch_, shift in enumerate((0, 8, 16)):
        mixed = _blend(t, wx, wy, shift)
        single = np.where((near >> 24) != 0, (near >> shift) & 0xFF, (word >> shift) & 0xFF)
        rgb[..., ch_] = np.where(placed, np.where(every, mixed, single), (word >> shift) & 0xFF)
    return outs, rgb


def rectify_loops(inv, origin, size, raster_size, gsd_mm, top_left_mm, planes=(), rgba=None, fill=255, rgb_fill=(0, 0, 0)):
    (ch, cw), (oy, ox), (gh, gw), (e0, ntop) = size, origin, raster_size, top_left_mm
    inv = [float(m) for m in inv]
    outs = [np.full((gh, gw), fill, np.uint8) for _ in planes]
    rgb = None if rgba is None else np.empty((gh, gw, 3), np.uint8)
    tap = lambda tx, ty: int(rgba[ty, tx]) & 0xFFFFFFFF if 0 <= tx < cw and 0 <= ty < ch else 0  # noqa: E731
    for v in range(gh):
        for u in range(gw):
            eg = float(e0) + (u + 0.5) * float(gsd_mm)
            ng = float(ntop) - (v + 0.5) * float(gsd_mm)
            nu = (inv[0] * eg + inv[1] * ng) + inv[2]
            nv = (inv[3] * eg + inv[4] * ng) + inv[5]
            d = (inv[6] * eg + inv[7] * ng) + inv[8]
            try:
                x, y = nu / d, nv / d
            except ZeroDivisionError:
                x = y = math.nan
            placed = abs(x) < 2.0 ** 20 and abs(y) < 2.0 ** 20
            colour = rgb_fill
            if placed:
                nx, ny = math.floor(x) + ox, math.floor(y) + oy
                if 0 <= nx < cw and 0 <= ny < ch:
                    for p, o in zip(planes, outs):
                        o[v, u] = p[ny, nx]
                if rgba is not None:
                    sx, sy = x - 0.5, y - 0.5
                    fx, fy = math.floor(sx), math.floor(sy)
                    wx, wy = math.floor((sx - fx) * 256.0), math.floor((sy - fy) * 256.0)
                    x0, y0 = fx + ox, fy + oy
                    t = [tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)]
                    if all(w >> 24 for w in t):
                        colour = tuple(_blend(t, wx, wy, s) for s in (0, 8, 16))
                    elif tap(nx, ny) >> 24:
                        colour = tuple((tap(nx, ny) >> s) & 0xFF for s in (0, 8, 16))
            if rgba is not None:
                rgb[v, u] = colour
    return outs, rgb


# ------------------------------------------------------------------------------------------------ the models and cases the tests share
def model_flip(gsd_mm=250, east_mm=0, north_mm=0):
    """North up, y down, whole millimetres: E = gsd * i + east, N = -gsd * j + north."""
    return np.array([gsd_mm, 0, east_mm, 0, -gsd_mm, north_mm, 0, 0, 1], np.float64)


def model_turn(gsd_mm=250):
    """A quarter turn with the reflection: E = gsd * j, N = gsd * i."""
    return np.array([0, gsd_mm, 0, gsd_mm, 0, 0, 0, 0, 1], np.float64)


def models(size, origin):
    """(name, forward) for a canvas: the integer flip, the quarter turn, a sheared affine, and a mild, a strong and a steep projective.
    The strong one's denominator runs from 1 to 2.2 across the canvas, the steep one's from 1 to 3.5, inside the factor of 4; a raster
    around the steep one's footprint would take the inverse beyond ITS factor of 4, so the steep cases carry no raster."""
    (ch, cw), (oy, ox) = size, origin
    shear = [812.37, 133.9, -4000.25, 95.11, -790.6, 9000.5]
    tilt = lambda t, w, h: np.array(shear + [t / w, t / h, 1.0 + t / w * ox + t / h * oy], np.float64)  # noqa: E731
    return [("flip", model_flip()), ("turn", model_turn()), ("shear", np.array(shear + [0, 0, 1], np.float64)),
            ("mild", np.array(shear + [1e-4, -5e-5, 1.0], np.float64)), ("strong", tilt(0.6, max(cw, 8), max(ch, 8))), ("steep", tilt(1.25, cw, ch))]


SIZES = [(1, 1), (1, 37), (41, 1), (37, 53)] + [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)]
CLASSES = 5
MAX_REGIONS = 24


def planes_for(size, seed):
    """(cls with 255 and ids >= K, a second id plane, index with -1 and ids beyond the cap in runs, rgba with unseen holes) for a canvas."""
    rng = np.random.default_rng(seed)
    ch, cw = size
    cls = rng.integers(0, CLASSES, size).astype(np.uint8)
    cls[rng.random(size) < 0.15] = UNSEEN
    cls[rng.random(size) < 0.05] = CLASSES + 2
    other = rng.integers(0, 256, size).astype(np.uint8)
    blocks = rng.integers(-2, MAX_REGIONS + 3, (-(-ch // 3), -(-cw // 7))).astype(np.int32)
    index = np.repeat(np.repeat(blocks, 3, axis=0), 7, axis=1)[:ch, :cw].copy()
    rgba = rng.integers(0, 1 << 24, size).astype(np.int64) | (0xFF << 24)
    rgba[rng.random(size) < 0.1] = 0
    return cls, other, np.ascontiguousarray(index), rgba.astype(np.uint32)


def raster_for(fwd, size, origin, margin=2, scale=1.0):
    """A raster around the canvas' ground footprint: (raster_size, gsd_mm, top_left_mm), the gsd the model's mean pixel size times scale."""
    (ch, cw), (oy, ox) = size, origin
    xs, ys = np.array([0, cw, cw, 0]) - ox, np.array([0, 0, ch, ch]) - oy
    e, n = corner(fwd, xs, ys)
    gsd = max(1, int(round(scale * math.sqrt(abs(polygon_shoelace(e, n)) / 2.0 / (ch * cw)))))
    e0, ntop = int(e.min()) - margin * gsd, int(n.max()) + margin * gsd
    gw, gh = -(-(int(e.max()) + margin * gsd - e0) // gsd), -(-(ntop - (int(n.min()) - margin * gsd)) // gsd)
    return (min(gh, 400), min(gw, 400)), gsd, (e0, ntop)


@functools.lru_cache(maxsize=None)
def op_cases():
    """(name, size, origin, forward, cls, other, index, rgba, raster) for every size and model; the origins are off-centre."""
    cases = []
    for n, size in enumerate(SIZES):
        origin = (size[0] // 3 - 2, size[1] // 4 + 1)
        cls, other, index, rgba = planes_for(size, 100 + n)
        for name, fwd in models(size, origin):
            cases.append((f"{size[0]}x{size[1]} {name}", size, origin, fwd, cls, other, index, rgba, None if name == "steep" else raster_for(fwd, size, origin)))
    # one raster far larger than the canvas' footprint: tiles wholly outside, straddling and inside
    size, origin = (37, 53), (5, -4)
    cls, other, index, rgba = planes_for(size, 300)
    for name, fwd in models(size, origin)[2:4]:
        cases.append((f"wide {name}", size, origin, fwd, cls, other, index, rgba, raster_for(fwd, size, origin, margin=90, scale=0.5)))
    return cases


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The vectorised reference of a case, computed once: (area with index, area without, rectify of four planes with rgba or None
    without a raster, points)."""
    _, size, origin, fwd, cls, other, index, rgba, raster = [c for c in op_cases() if c[0] == name][0]
    rasters = None
    if raster is not None:
        rasters = rectify(invert(fwd), origin, size, raster[0], raster[1], raster[2], rectify_planes(cls, other, index), rgba, FILL, RGB_FILL)
    return (area(cls, fwd, origin, CLASSES, index, MAX_REGIONS), area(cls, fwd, origin, CLASSES), rasters, points(case_points(size), fwd, origin))


FILL, RGB_FILL = 254, (9, 8, 7)


def rectify_planes(cls, other, index):
    """The four uint8 planes the rectify cases carry: class, an arbitrary byte plane, the index's low byte, the class again."""
    return cls, other, index.astype(np.uint8), cls


def case_points(size):
    """Lattice points of the canvas, a few beyond it, and two nobody can place."""
    ch, cw = size
    ys, xs = np.mgrid[0:ch + 1:max(1, ch // 5), 0:cw + 1:max(1, cw // 5)]
    pts = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)
    return np.concatenate([pts, [[cw, ch], [-3, -2], [cw + 4, ch + 1], [(1 << 20) + 1, 0], [0, -(1 << 20) - 1]]]).astype(np.int32)


def blob(size, seed):
    """A random connected-looking pixel set with holes: a thresholded smooth field."""
    rng = np.random.default_rng(seed)
    f = rng.random(size)
    for _ in range(3):
        p = np.pad(f, 1, mode="edge")
        f = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] + p[1:-1, 1:-1]) / 5.0
    return f > np.median(f)
