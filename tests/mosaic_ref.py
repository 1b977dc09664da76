"""CPU restatement of the flood-extent mosaic (include/floodseg_test.h: global_motion, pose_chain, mosaic_accumulate, mosaic_resolve;
csrc/mosaic_defs.h) for the tests of the HIP route, in two forms:

  * vectorised numpy (global_motion, mosaic_accumulate, mosaic_resolve): int64 arrays, what the GPU tests compare with, bit for bit;
  * a literal per-row, per-pixel loop with Python integers (global_motion_loop, mosaic_accumulate_loop, mosaic_resolve_loop): the
    definition read aloud, with the mode found by sorting tuples rather than through the packed key.

The float64 part (gm_solve, gm_finish) is scalar and written once: Python floats are IEEE doubles, every operation below is one
rounding, and round() rounds ties to even -- the order of operations is mosaic_defs.h's, statement for statement.  The pose chain is
scalar as well (n <= 64 frames).  A test helper, not an oracle module.
"""
import functools

import numpy as np

FRAC = 20
ONE = 1 << FRAC
HALF = 1 << (FRAC - 1)
MAX_VECTOR = 32
SIDE = 2 * MAX_VECTOR + 1
MAX_TOL_Q20 = 64 * ONE
PARAM_LIMIT = 1048576.0
PLAUSIBLE = ONE // 4
PAIR_LINEAR_MAX = 2 * ONE
PAIR_SHIFT_LIMIT = (1 << 16) * ONE
POSE_LINEAR_LIMIT = 16 * ONE
POSE_SHIFT_LIMIT = (1 << 14) * ONE
POSE_BACK_SHIFT_LIMIT = (1 << 20) * ONE
IDENTITY = [ONE, 0, 0, 0, ONE, 0]
OK, CUT, FEW, DEGENERATE = 0, 1, 2, 3
POSE_OK, POSE_BRIDGED, POSE_LOST = 0, 1, 2
VOID_ROW = (-1, 16, 16, -16, -16, -16, -16)


def rshr(v):
    """(v + 2^19) >> 20, arithmetic: Python integers and int64 arrays alike."""
    return (v + HALF) >> FRAC


def tol_q20(tol):
    """Pixels -> Q20, as ops.global_motion converts its `tol`."""
    return int(round(float(tol) * ONE))


def exclude_bits(exclude):
    bits = 0
    for k in exclude:
        bits |= 1 << int(k)
    return bits


# ------------------------------------------------------------------------------------------------ the float64 part, scalar
def q20_of(v):
    if not (-PARAM_LIMIT < v < PARAM_LIMIT):
        return None
    return int(round(v * 1048576.0))


def gm_solve(s):
    """The twelve sums -> (a0, a1, a2, b0, b1, b2) in Q20, or None (determinant 0, or a parameter out of range)."""
    m00, m01, m02, m11, m12, m22 = (float(int(v)) for v in s[:6])
    c00 = m11 * m22 - m12 * m12
    c01 = m01 * m22 - m12 * m02
    c02 = m01 * m12 - m11 * m02
    c11 = m00 * m22 - m02 * m02
    c12 = m00 * m12 - m01 * m02
    c22 = m00 * m11 - m01 * m01
    det = m00 * c00 - m01 * c01
    det = det + m02 * c02
    if det == 0.0:
        return None
    out = []
    for k in range(2):
        r0, r1, r2 = (float(int(v)) for v in s[6 + 3 * k:9 + 3 * k])
        u = c00 * r0 - c01 * r1
        u = u + c02 * r2
        v0 = u / det
        u = c11 * r1 - c01 * r0
        u = u - c12 * r2
        v1 = u / det
        u = c02 * r0 - c12 * r1
        u = u + c22 * r2
        v2 = u / det
        out += [q20_of(v0), q20_of(v1), q20_of(v2)]
    return None if any(v is None for v in out) else out


def pair_in_bounds(fwd, inv):
    return (all(abs(m[i]) <= PAIR_LINEAR_MAX for m in (fwd, inv) for i in (0, 1, 3, 4))
            and all(abs(m[i]) < PAIR_SHIFT_LIMIT for m in (fwd, inv) for i in (2, 5)))


def gm_finish(model, fh, fw, h, w):
    """The pair model in mask pixels -> (fwd, inv) Q20, or None (implausible)."""
    one = 1048576.0
    a0, a1, a2, b0, b1, b2 = (float(int(v)) / one for v in model)
    wb, hb = float(fw // 16), float(fh // 16)
    dw, dh, dfw, dfh = float(w), float(h), float(fw), float(fh)
    sx, sy = dw / dfw, dh / dfh
    kxy = (dw * dfh) / (dfw * dh)
    kyx = (dh * dfw) / (dfh * dw)
    f = [1.0 + a1 / 8.0, (a2 / 8.0) * kxy, ((a0 - a1 * wb) - a2 * hb) * sx, (b1 / 8.0) * kyx, 1.0 + b2 / 8.0, ((b0 - b1 * wb) - b2 * hb) * sy]
    m = [q20_of(v) for v in f]
    if any(v is None for v in m):
        return None
    if abs(m[0] - ONE) > PLAUSIBLE or abs(m[4] - ONE) > PLAUSIBLE or abs(m[1]) > PLAUSIBLE or abs(m[3]) > PLAUSIBLE:
        return None
    g00, g01, g02, g10, g11, g12 = (float(v) / one for v in m)
    det = g00 * g11 - g01 * g10
    i00, i11 = g11 / det, g00 / det
    i01 = -(g01 / det)
    i10 = -(g10 / det)
    i02 = -(i00 * g02 + i01 * g12)
    i12 = -(i10 * g02 + i11 * g12)
    inv = [q20_of(v) for v in (i00, i01, i02, i10, i11, i12)]
    if any(v is None for v in inv) or not pair_in_bounds(m, inv):
        return None
    return m, inv


def round_tolerance(tol, rounds, r):
    return min(int(tol) << (rounds - 1 - r), MAX_TOL_Q20)


def model_row(fwd, inv, status, usable, inliers, done):
    return list(fwd) + list(inv) + [status, usable, inliers, done]


def _fit(usable, mode, rounds, tol, min_inliers, sums_of, fh, fw, h, w):
    """The part after the histogram, shared by the two forms: sums_of(model, T) -> the twelve sums over the inliers."""
    count, dx, dy = mode
    model = [dx * ONE, 0, 0, dy * ONE, 0, 0]
    inliers, done = count, 0
    status = FEW if usable < min_inliers else OK
    for r in range(rounds):
        if status != OK:
            break
        s = sums_of(model, round_tolerance(tol, rounds, r))
        nxt = None if s[0] < min_inliers else gm_solve(s)
        if nxt is None:
            if r == 0:
                status = FEW if s[0] < min_inliers else DEGENERATE
            break
        model, inliers, done = nxt, int(s[0]), r + 1
    got = gm_finish(model, fh, fw, h, w) if status == OK else None
    if status == OK and got is None:
        status = DEGENERATE
    fwd, inv = got if got is not None else (IDENTITY, IDENTITY)
    return model_row(fwd, inv, status, usable, inliers, done)


# ------------------------------------------------------------------------------------------------ global_motion, the loop
def usable_rows_loop(table, fh, fw, mask, h, w, exclude_set):
    rows = []
    hb, wb = fh // 16, fw // 16
    for row in np.asarray(table).tolist():
        sx, sy, tx, ty = row[3:7]
        if sx < 0 or tx < 0 or ty < 0 or tx >= fw or ty >= fh:
            continue
        dx, dy = sx - tx, sy - ty
        if abs(dx) > MAX_VECTOR or abs(dy) > MAX_VECTOR:
            continue
        if mask is not None:
            cls = int(mask[min(h - 1, ty * h // fh), min(w - 1, tx * w // fw)])
            if cls < 32 and (exclude_set >> cls) & 1:
                continue
        rows.append((2 * (tx >> 4) + 1 - wb, 2 * (ty >> 4) + 1 - hb, dx, dy))
    return rows


def global_motion_loop(tables, frame_size, mask_size, rounds=4, tol=ONE, min_inliers=12, mask=None, exclude_set=0, pair_stats=None):
    """tol in Q20.  -> int64 [n, 16]."""
    (fh, fw), (h, w) = frame_size, mask_size
    out = []
    for f in range(len(tables)):
        if pair_stats is not None and pair_stats[f][2] != 0:
            out.append(model_row(IDENTITY, IDENTITY, CUT, 0, 0, 0))
            continue
        rows = usable_rows_loop(tables[f], fh, fw, None if mask is None else mask[f], h, w, exclude_set)
        hist = {}
        for _, _, dx, dy in rows:
            hist[(dy, dx)] = hist.get((dy, dx), 0) + 1
        if hist:
            (dy, dx), count = min(hist.items(), key=lambda kv: (-kv[1], abs(kv[0][1]) + abs(kv[0][0]), kv[0][0], kv[0][1]))
        else:  # an empty histogram: every bin ties at 0, the order's first is the zero vector
            dy, dx, count = 0, 0, 0

        def sums_of(model, T, rows=rows):
            s = [0] * 12
            for p, q, dx, dy in rows:
                px = model[0] + model[1] * p + model[2] * q
                py = model[3] + model[4] * p + model[5] * q
                if abs(dx * ONE - px) <= T and abs(dy * ONE - py) <= T:
                    for i, v in enumerate((1, p, q, p * p, p * q, q * q, dx, p * dx, q * dx, dy, p * dy, q * dy)):
                        s[i] += v
            return s

        out.append(_fit(len(rows), (count, dx, dy), rounds, tol, min_inliers, sums_of, fh, fw, h, w))
    return np.array(out, dtype=np.int64).reshape(len(tables), 16)


# ------------------------------------------------------------------------------------------------ global_motion, vectorised
def usable_rows(table, fh, fw, mask, h, w, exclude_set):
    """-> int64 arrays (p, q, dx, dy) of the usable rows."""
    t = np.asarray(table).astype(np.int64)
    sx, sy, tx, ty = t[:, 3], t[:, 4], t[:, 5], t[:, 6]
    ok = (sx >= 0) & (tx >= 0) & (ty >= 0) & (tx < fw) & (ty < fh)
    dx, dy = sx - tx, sy - ty
    ok &= (np.abs(dx) <= MAX_VECTOR) & (np.abs(dy) <= MAX_VECTOR)
    if mask is not None:
        excl = np.array([k < 32 and (exclude_set >> k) & 1 == 1 for k in range(256)])
        cy = np.minimum(h - 1, np.clip(ty, 0, fh - 1) * h // fh)
        cx = np.minimum(w - 1, np.clip(tx, 0, fw - 1) * w // fw)
        ok &= ~excl[np.asarray(mask)[cy, cx]]
    tx, ty, dx, dy = tx[ok], ty[ok], dx[ok], dy[ok]
    return 2 * (tx >> 4) + 1 - fw // 16, 2 * (ty >> 4) + 1 - fh // 16, dx, dy


def mode_key(count, bins):
    dy, dx = bins // SIDE - MAX_VECTOR, bins % SIDE - MAX_VECTOR
    return (count.astype(np.int64) << 32) | ((2 * MAX_VECTOR - np.abs(dx) - np.abs(dy)) << 16) | ((MAX_VECTOR - dy) << 8) | (MAX_VECTOR - dx)


def global_motion(tables, frame_size, mask_size, rounds=4, tol=ONE, min_inliers=12, mask=None, exclude_set=0, pair_stats=None):
    """tol in Q20.  -> int64 [n, 16]."""
    (fh, fw), (h, w) = frame_size, mask_size
    out = []
    for f in range(len(tables)):
        if pair_stats is not None and pair_stats[f][2] != 0:
            out.append(model_row(IDENTITY, IDENTITY, CUT, 0, 0, 0))
            continue
        p, q, dx, dy = usable_rows(tables[f], fh, fw, None if mask is None else mask[f], h, w, exclude_set)
        hist = np.bincount((dy + MAX_VECTOR) * SIDE + dx + MAX_VECTOR, minlength=SIDE * SIDE)
        key = int(mode_key(hist, np.arange(SIDE * SIDE)).max())
        mode = (key >> 32, MAX_VECTOR - (key & 0xFF), MAX_VECTOR - ((key >> 8) & 0xFF))

        def sums_of(model, T, p=p, q=q, dx=dx, dy=dy):
            px = model[0] + model[1] * p + model[2] * q
            py = model[3] + model[4] * p + model[5] * q
            inl = (np.abs(dx * ONE - px) <= T) & (np.abs(dy * ONE - py) <= T)
            a, b, u, v = p[inl], q[inl], dx[inl], dy[inl]
            return [int(x) for x in (inl.sum(), a.sum(), b.sum(), (a * a).sum(), (a * b).sum(), (b * b).sum(), u.sum(), (a * u).sum(), (b * u).sum(),
                                     v.sum(), (a * v).sum(), (b * v).sum())]

        out.append(_fit(len(p), mode, rounds, tol, min_inliers, sums_of, fh, fw, h, w))
    return np.array(out, dtype=np.int64).reshape(len(tables), 16)


# ------------------------------------------------------------------------------------------------ pose_chain (Python integers)
def compose(a, b):
    return [rshr(a[0] * b[0] + a[1] * b[3]), rshr(a[0] * b[1] + a[1] * b[4]), rshr(a[0] * b[2] + a[1] * b[5]) + a[2],
            rshr(a[3] * b[0] + a[4] * b[3]), rshr(a[3] * b[1] + a[4] * b[4]), rshr(a[3] * b[2] + a[4] * b[5]) + a[5]]


def pose_in_bounds(to_anchor, from_anchor):
    return (all(abs(m[i]) < POSE_LINEAR_LIMIT for m in (to_anchor, from_anchor) for i in (0, 1, 3, 4))
            and abs(to_anchor[2]) < POSE_SHIFT_LIMIT and abs(to_anchor[5]) < POSE_SHIFT_LIMIT
            and abs(from_anchor[2]) < POSE_BACK_SHIFT_LIMIT and abs(from_anchor[5]) < POSE_BACK_SHIFT_LIMIT)


def frame_clipped(to_anchor, h, w, ch, cw, ox, oy):
    for x, y in ((0, 0), (w, 0), (0, h), (w, h)):
        cx = to_anchor[0] * x + to_anchor[1] * y + to_anchor[2] + ox * ONE
        cy = to_anchor[3] * x + to_anchor[4] * y + to_anchor[5] + oy * ONE
        if cx < 0 or cy < 0 or cx > cw * ONE or cy > ch * ONE:
            return True
    return False


def pose_chain(model, state, mask_size, canvas_size, origin, max_bridge=2):
    """model int64 [n, 16], state int64 [32] (all zero: fresh) -> (poses int64 [n, 16], the state after).  origin = (oy, ox)."""
    (h, w), (ch, cw), (oy, ox) = mask_size, canvas_size, origin
    st = [int(v) for v in state]
    poses = []
    for row in np.asarray(model).tolist():
        status, inliers, usable = POSE_OK, 0, 0
        if st[24] == 0:
            st[0:6], st[6:12], st[12:18], st[18:24] = IDENTITY, IDENTITY, IDENTITY, IDENTITY
            st[24], st[27] = 1, 0
        elif st[24] != 1:
            status = POSE_LOST
        else:
            ms = row[12] if row[12] in (OK, CUT) else DEGENERATE
            if ms == OK and not pair_in_bounds(row[0:6], row[6:12]):
                ms = DEGENERATE
            inliers, usable = row[14], row[13]
            if ms == OK:
                st[12:18], st[18:24], st[27] = row[0:6], row[6:12], 0
            elif ms == CUT or st[27] < 0 or st[27] >= max_bridge or not pair_in_bounds(st[12:18], st[18:24]):
                status = POSE_LOST
            else:
                status = POSE_BRIDGED
                st[27] += 1
            if status != POSE_LOST:
                ok = pose_in_bounds(st[0:6], st[6:12])
                if ok:
                    to_next, from_next = compose(st[0:6], st[12:18]), compose(st[18:24], st[6:12])
                    ok = pose_in_bounds(to_next, from_next)
                if ok:
                    st[0:6], st[6:12] = to_next, from_next
                else:
                    status = POSE_LOST
            if status == POSE_LOST:
                st[24] = 2
        st[25] += 1
        if status == POSE_LOST:
            st[26] += 1
            poses.append(IDENTITY + IDENTITY + [POSE_LOST, 0, inliers, usable])
        else:
            poses.append(st[0:6] + st[6:12] + [status, int(frame_clipped(st[0:6], h, w, ch, cw, ox, oy)), inliers, usable])
    return np.array(poses, dtype=np.int64).reshape(-1, 16), np.array(st, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ mosaic_accumulate
def pose_votes(pose):
    pose = [int(v) for v in pose]
    back = pose[6:12]
    return (pose[12] in (POSE_OK, POSE_BRIDGED) and all(abs(back[i]) < POSE_LINEAR_LIMIT for i in (0, 1, 3, 4))
            and abs(back[2]) < POSE_BACK_SHIFT_LIMIT and abs(back[5]) < POSE_BACK_SHIFT_LIMIT)


def mosaic_accumulate_loop(mask, poses, votes, origin):
    """The definition literally; votes uint16 [K, CH, CW] is updated in place and returned."""
    (n, h, w), (k_max, ch, cw), (oy, ox) = mask.shape, votes.shape, origin
    for Y in range(ch):
        for X in range(cw):
            ax, ay = (2 * (X - ox) + 1) << 19, (2 * (Y - oy) + 1) << 19
            for f in range(n):
                if not pose_votes(poses[f]):
                    continue
                m = [int(v) for v in poses[f][6:12]]
                x = (rshr(m[0] * ax + m[1] * ay) + m[2]) >> FRAC
                y = (rshr(m[3] * ax + m[4] * ay) + m[5]) >> FRAC
                if 0 <= x < w and 0 <= y < h and mask[f, y, x] < k_max:
                    k = int(mask[f, y, x])
                    votes[k, Y, X] = min(int(votes[k, Y, X]) + 1, 65535)
    return votes


def mosaic_accumulate(mask, poses, votes, origin):
    """Vectorised; votes uint16 [K, CH, CW] is updated in place and returned."""
    (n, h, w), (k_max, ch, cw), (oy, ox) = mask.shape, votes.shape, origin
    ax = (((2 * (np.arange(cw, dtype=np.int64) - ox) + 1)) << 19)[None, :]
    ay = (((2 * (np.arange(ch, dtype=np.int64) - oy) + 1)) << 19)[:, None]
    for f in range(n):
        if not pose_votes(poses[f]):
            continue
        m = [int(v) for v in poses[f][6:12]]
        x = (rshr(m[0] * ax + m[1] * ay) + m[2]) >> FRAC
        y = (rshr(m[3] * ax + m[4] * ay) + m[5]) >> FRAC
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        Y, X = np.nonzero(inside)
        k = mask[f][y[Y, X], x[Y, X]].astype(np.int64)
        keep = k < k_max
        k, Y, X = k[keep], Y[keep], X[keep]
        votes[k, Y, X] = np.minimum(votes[k, Y, X].astype(np.int64) + 1, 65535).astype(np.uint16)  # one (Y, X) per frame: no duplicates
    return votes


# ------------------------------------------------------------------------------------------------ mosaic_resolve
def mosaic_resolve_loop(votes):
    k_max, ch, cw = votes.shape
    cls, conf = np.full((ch, cw), 255, np.uint8), np.zeros((ch, cw), np.uint8)
    seen, totals = np.zeros((ch, cw), np.uint32), np.zeros((k_max, 2), np.int64)
    for Y in range(ch):
        for X in range(cw):
            v = [int(votes[k, Y, X]) for k in range(k_max)]
            total, most = sum(v), max(v)
            seen[Y, X] = total
            for k in range(k_max):
                totals[k, 1] += v[k]
            if total:
                cls[Y, X] = v.index(most)
                conf[Y, X] = (255 * most + total // 2) // total
                totals[v.index(most), 0] += 1
    return cls, conf, seen, totals


def mosaic_resolve(votes):
    """-> (cls uint8 [CH, CW], conf uint8, seen uint32, totals int64 [K, 2])."""
    v = votes.astype(np.int64)
    total, most, best = v.sum(0), v.max(0), v.argmax(0)  # argmax: the first, i.e. the lowest id
    lit = total > 0
    cls = np.where(lit, best, 255).astype(np.uint8)
    conf = np.where(lit, (255 * most + total // 2) // np.maximum(total, 1), 0).astype(np.uint8)
    totals = np.stack([np.bincount(best[lit], minlength=v.shape[0]), v.reshape(v.shape[0], -1).sum(1)], 1).astype(np.int64)
    return cls, conf, total.astype(np.uint32), totals


# ------------------------------------------------------------------------------------------------ synthetic tables and poses
def grid_table(hb, wb, vector_of):
    """A matcher-shaped table of a hb x wb block grid: vector_of(cx, cy) -> (dx, dy) integer arrays at the block centres."""
    by, bx = np.meshgrid(np.arange(hb), np.arange(wb), indexing="ij")
    cx, cy = (bx * 16 + 8).reshape(-1), (by * 16 + 8).reshape(-1)
    dx, dy = vector_of(cx, cy)
    t = np.empty((hb * wb, 7), np.int32)
    t[:, 0], t[:, 1], t[:, 2] = -1, 16, 16
    t[:, 3], t[:, 4], t[:, 5], t[:, 6] = cx + dx, cy + dy, cx, cy
    return t


def affine_vectors(hb, wb, degrees=0.5, zoom=1.005, shift=(7, -3)):
    """vector_of for a rotation and zoom about the frame centre plus a shift (dx, dy), rounded to whole pixels as a matcher finds them."""
    c, s = zoom * np.cos(np.radians(degrees)), zoom * np.sin(np.radians(degrees))
    mx, my = 8.0 * wb, 8.0 * hb

    def vector_of(cx, cy):
        u, v = cx - mx, cy - my
        return np.rint(c * u - s * v + mx + shift[0] - cx).astype(np.int64), np.rint(s * u + c * v + my + shift[1] - cy).astype(np.int64)

    return vector_of


def with_outliers(table, fraction, seed):
    """A copy with `fraction` of the rows replaced by random vectors within +-32."""
    rng = np.random.RandomState(seed)
    t = table.copy()
    pick = rng.permutation(len(t))[:int(round(fraction * len(t)))]
    t[pick, 3] = t[pick, 5] + rng.randint(-32, 33, size=len(pick))
    t[pick, 4] = t[pick, 6] + rng.randint(-32, 33, size=len(pick))
    return t


def affine_pose(a, b, c, d, tx, ty):
    """(to_anchor, from_anchor) Q20 of x' = a x + b y + tx, y' = c x + d y + ty, each rounded from float64 (a test input, not a rule)."""
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    q = lambda v: int(round(v * ONE))  # noqa: E731
    return [q(a), q(b), q(tx), q(c), q(d), q(ty)], [q(ia), q(ib), q(-(ia * tx + ib * ty)), q(ic), q(id_), q(-(ic * tx + id_ * ty))]


def pose_rows(pairs, status=None):
    """int64 [n, 16] pose rows from (to_anchor, from_anchor) pairs; status per frame (default ok)."""
    rows = [list(t) + list(f) + [0 if status is None else status[i], 0, 0, 0] for i, (t, f) in enumerate(pairs)]
    return np.array(rows, dtype=np.int64).reshape(-1, 16)


# ------------------------------------------------------------------------------------------------ the end-to-end scene
SCENE_VIEW, SCENE_CANVAS, SCENE_ORIGIN = (128, 192), (200, 300), (54, 36)
SCENE_STEPS = ((5, -7), (3, 6), (-4, 7), (-6, -3), (7, 5))  # (dy, dx) from view to view, from offset (60, 90)
SCENE_SETTINGS = dict(rounds=4, tol=ONE, min_inliers=6)


@functools.lru_cache(maxsize=None)
def scene():
    """A 256 x 384 random uint8 texture with a four-class label map, and six 128 x 192 views of it.  -> (frames uint8 [6, 128, 192],
    masks uint8 [6, 128, 192], offsets [(y, x)] * 6, labels uint8 [256, 384]); read-only."""
    world = np.random.RandomState(7).randint(0, 256, size=(256, 384)).astype(np.uint8)
    yy, xx = np.mgrid[0:256, 0:384]
    labels = ((yy // 37 + 2 * (xx // 53) + (yy + xx) // 101) % 4).astype(np.uint8)
    offsets = [(60, 90)]
    for dy, dx in SCENE_STEPS:
        offsets.append((offsets[-1][0] + dy, offsets[-1][1] + dx))
    vh, vw = SCENE_VIEW
    frames = np.stack([world[y:y + vh, x:x + vw] for y, x in offsets])
    masks = np.stack([labels[y:y + vh, x:x + vw] for y, x in offsets])
    for a in (frames, masks, labels):
        a.setflags(write=False)
    return frames, masks, offsets, labels


def scene_expectation():
    """What the scene's mosaic must be, analytically: (seen [200, 300], cls with 255 where unseen)."""
    _, _, offsets, labels = scene()
    (ch, cw), (oy, ox), (vh, vw) = SCENE_CANVAS, SCENE_ORIGIN, SCENE_VIEW
    seen = np.zeros((ch, cw), np.int64)
    for y, x in offsets:
        top, left = oy + y - offsets[0][0], ox + x - offsets[0][1]
        seen[top:top + vh, left:left + vw] += 1
    world = np.full((ch, cw), 255, np.uint8)  # canvas pixel (Y, X) shows world pixel (Y - oy + y0, X - ox + x0)
    y0, x0 = offsets[0][0] - oy, offsets[0][1] - ox
    world[:, :] = labels[y0:y0 + ch, x0:x0 + cw]
    return seen, np.where(seen > 0, world, 255).astype(np.uint8)


def run_scene(tables, masks, motion=global_motion, accumulate=mosaic_accumulate):
    """The four ops of the reference on the scene's tables [6][blocks, 7] (row 0: anything; the anchor's is ignored)."""
    model = motion(tables, SCENE_VIEW, SCENE_VIEW, **SCENE_SETTINGS)
    poses, state = pose_chain(model, np.zeros(32, np.int64), SCENE_VIEW, SCENE_CANVAS, SCENE_ORIGIN)
    votes = accumulate(masks, poses, np.zeros((4,) + SCENE_CANVAS, np.uint16), SCENE_ORIGIN)
    return model, poses, state, votes, mosaic_resolve(votes)


# ------------------------------------------------------------------------------------------------ the library's refusals
def good_arguments():
    """Per op the arguments of a call that passes validation (dummy non-null pointers), in the ABI's order, by name."""
    return {
        "global_motion": dict(tables=64, pair_stats=64, mask=64, exclude_set=2, n=5, FH=128, FW=192, H=128, W=192, rounds=4, tol_q20=ONE, min_inliers=12,
                              model=64, stream=None),
        "pose_chain": dict(model=64, state=64, poses=64, n=5, H=128, W=192, CH=200, CW=300, ox=36, oy=54, max_bridge=2, stream=None),
        "mosaic_accumulate": dict(mask=64, poses=64, n=5, H=128, W=192, K=5, CH=200, CW=300, ox=36, oy=54, votes=64, stream=None),
        "mosaic_resolve": dict(votes=64, K=5, CH=200, CW=300, cls=64, conf=64, seen=64, totals=64, stream=None),
    }


def refusal_cases():
    """(op, changed arguments, a word of the message)."""
    cases = []
    for op, ptrs in (("global_motion", ("tables", "model")), ("pose_chain", ("model", "state", "poses")), ("mosaic_accumulate", ("mask", "poses", "votes")),
                     ("mosaic_resolve", ("votes", "cls", "conf", "seen", "totals"))):
        cases += [(op, {p: None}, b"null") for p in ptrs]
    for op in ("global_motion", "pose_chain", "mosaic_accumulate"):
        cases += [(op, dict(n=0), b"n="), (op, dict(n=65), b"n="), (op, dict(H=0), b"0x"), (op, dict(W=16385), b"16385")]
    cases += [("global_motion", dict(FH=15), b"15x"), ("global_motion", dict(FW=16385), b"16385"), ("global_motion", dict(rounds=-1), b"rounds=-1"),
              ("global_motion", dict(rounds=9), b"rounds=9"), ("global_motion", dict(tol_q20=-1), b"tol_q20=-1"),
              ("global_motion", dict(tol_q20=MAX_TOL_Q20 + 1), b"tol_q20="), ("global_motion", dict(min_inliers=2), b"min_inliers=2"),
              ("global_motion", dict(tables=66), b"aligned to 4"), ("global_motion", dict(pair_stats=66), b"aligned to 4"),
              ("global_motion", dict(model=68), b"aligned to 8")]
    cases += [("pose_chain", dict(CH=0), b"canvas"), ("pose_chain", dict(CW=16385), b"canvas"), ("pose_chain", dict(ox=16385), b"origin"),
              ("pose_chain", dict(oy=-16385), b"origin"), ("pose_chain", dict(max_bridge=-1), b"max_bridge=-1"), ("pose_chain", dict(max_bridge=65), b"max_bridge=65"),
              ("pose_chain", dict(model=68), b"aligned to 8"), ("pose_chain", dict(state=68), b"aligned to 8"), ("pose_chain", dict(poses=68), b"aligned to 8")]
    cases += [("mosaic_accumulate", dict(K=0), b"classes=0"), ("mosaic_accumulate", dict(K=33), b"classes=33"), ("mosaic_accumulate", dict(CH=16385), b"canvas"),
              ("mosaic_accumulate", dict(ox=-16385), b"origin"), ("mosaic_accumulate", dict(poses=68), b"aligned to 8"),
              ("mosaic_accumulate", dict(votes=65), b"aligned to 2")]
    cases += [("mosaic_resolve", dict(K=0), b"classes=0"), ("mosaic_resolve", dict(K=33), b"classes=33"), ("mosaic_resolve", dict(CH=0), b"canvas"),
              ("mosaic_resolve", dict(CW=16385), b"canvas"), ("mosaic_resolve", dict(votes=65), b"aligned to 2"), ("mosaic_resolve", dict(seen=66), b"aligned to 4"),
              ("mosaic_resolve", dict(totals=68), b"aligned to 8")]
    return cases


def call_mosaic_op(lib, op, **changed):
    args = dict(good_arguments()[op])
    args.update(changed)
    return getattr(lib, "fs_" + op)(*args.values())
