"""CPU restatement of map-to-map registration and of the merge of two mosaics (include/floodseg_test.h: merge_view, merge_gate,
link_correct, mosaic_merge; the same rules as csrc/merge_defs.h) for the tests: plain numpy.  The three ops that walk a
plane or a table appear vectorised (what the GPU tests compare with, bit for bit) and as literal loops over Python integers (the
definition read aloud); correct_step is scalar, it is one row.  Everything is integer.  The matcher and the fit between the ops are
motion_modes_ref's and mosaic_ref's, the canvases ortho_ref's.  A test helper, not an oracle module."""
import functools

import numpy as np

import mosaic_ref as mref
import motion_modes_ref as mmref
import ortho_ref as oref
import refine_ref as rref
import relocate_ref as lref

ONE = mref.ONE
REGISTERED, INITIAL, NO_FIT, OUT_OF_BOUNDS = 0, 1, 2, 3          # word 12 of a link
OK, CORRECT_NO_FIT, CORRECT_OUT_OF_BOUNDS, NOT_LINKED = 0, 2, 3, 4  # link_correct's status
EMPTY = oref.EMPTY
ORDINAL_LAST = 0xFFFFFFFE


# ------------------------------------------------------------------------------------------------ the link and the gather
def link_row(b_to_a=None, a_to_b=None, status=INITIAL, tail=(0, 0, 0)):
    return np.array(list(mref.IDENTITY if b_to_a is None else b_to_a) + list(mref.IDENTITY if a_to_b is None else a_to_b) + [status] + list(tail), np.int64)


def link_in_bounds(link):
    link = [int(v) for v in link]
    return mref.pose_in_bounds(link[0:6], link[6:12])


def link_views(link):
    return int(link[12]) in (REGISTERED, INITIAL) and link_in_bounds(link)


def link_merges(link):
    return int(link[12]) == REGISTERED and link_in_bounds(link)


def b_pixel(a_to_b, X, Y, origin_a, origin_b):
    """The definition literally, Python integers (or int64 arrays): the B canvas pixel under the centre of A canvas pixel (X, Y)."""
    (oy_a, ox_a), (oy_b, ox_b) = origin_a, origin_b
    ax, ay = (2 * (X - ox_a) + 1) << 19, (2 * (Y - oy_a) + 1) << 19
    x = (mref.rshr(a_to_b[0] * ax + a_to_b[1] * ay) + a_to_b[2]) >> mref.FRAC
    y = (mref.rshr(a_to_b[3] * ax + a_to_b[4] * ay) + a_to_b[5]) >> mref.FRAC
    return x + ox_b, y + oy_b


def b_pixels(link, window, origin_a, size_b, origin_b):
    """Vectorised over window = (Y0, X0, WH, WW) of A -> (bx, by, exists), int64 / bool [WH, WW]."""
    y0, x0, wh, ww = window
    m = [int(v) for v in link[6:12]]
    bx, by = b_pixel(m, np.arange(x0, x0 + ww, dtype=np.int64)[None, :], np.arange(y0, y0 + wh, dtype=np.int64)[:, None], origin_a, origin_b)
    return bx, by, (bx >= 0) & (bx < size_b[1]) & (by >= 0) & (by < size_b[0])


def whole_window(size):
    return (0, 0, size[0] // 16 * 16, size[1] // 16 * 16)


# ------------------------------------------------------------------------------------------------ merge_view
def merge_view_loop(rgba_a, origin_a, rgba_b, origin_b, link, window=None):
    y0, x0, wh, ww = whole_window(rgba_a.shape) if window is None else window
    cur, view, valid_a, valid_b = (np.zeros((wh, ww), np.uint8) for _ in range(4))
    usable = link_views(link)
    m = [int(v) for v in link[6:12]]
    for j in range(wh):
        for i in range(ww):
            a = int(rgba_a[y0 + j, x0 + i])
            cur[j, i], valid_a[j, i] = rref.luma_of(a), int(a >> 24 != 0)
            if not usable:
                continue
            bx, by = b_pixel(m, x0 + i, y0 + j, origin_a, origin_b)
            if 0 <= bx < rgba_b.shape[1] and 0 <= by < rgba_b.shape[0] and int(rgba_b[by, bx]) >> 24 != 0:
                view[j, i], valid_b[j, i] = rref.luma_of(int(rgba_b[by, bx])), 1
    return cur, view, valid_a, valid_b


def merge_view(rgba_a, origin_a, rgba_b, origin_b, link, window=None):
    window = whole_window(rgba_a.shape) if window is None else window
    y0, x0, wh, ww = window
    a = rgba_a[y0:y0 + wh, x0:x0 + ww].astype(np.int64)
    cur, valid_a = rref.luma_of(a).astype(np.uint8), ((a >> 24) != 0).astype(np.uint8)
    view, valid_b = np.zeros((wh, ww), np.uint8), np.zeros((wh, ww), np.uint8)
    if link_views(link):
        bx, by, exists = b_pixels(link, window, origin_a, rgba_b.shape, origin_b)
        j, i = np.nonzero(exists)
        b = rgba_b[by[j, i], bx[j, i]].astype(np.int64)
        ok = (b >> 24) != 0
        view[j[ok], i[ok]], valid_b[j[ok], i[ok]] = rref.luma_of(b[ok]), 1
    return cur, view, valid_a, valid_b


# ------------------------------------------------------------------------------------------------ merge_gate
def merge_gate_loop(table, valid_a, valid_b):
    h, w = valid_a.shape
    wb = w // 16
    out = []
    for index, row in enumerate(np.asarray(table).tolist()):
        ax, ay = 16 * (index % wb), 16 * (index // wb)
        x0, y0 = row[3] - 8, row[4] - 8
        keep = all(valid_a[ay + j, ax + i] == 1 for j in range(16) for i in range(16))
        keep = keep and x0 >= 0 and y0 >= 0 and x0 + 16 <= w and y0 + 16 <= h and all(valid_b[y0 + j, x0 + i] == 1 for j in range(16) for i in range(16))
        out.append(row if keep else list(mref.VOID_ROW))
    return np.array(out, np.int32).reshape(-1, 7)


def merge_gate(table, valid_a, valid_b):
    h, w = valid_a.shape
    own = (valid_a[:h // 16 * 16, :w // 16 * 16] == 1).reshape(h // 16, 16, w // 16, 16).all(axis=(1, 3)).reshape(-1)
    out = rref.map_gate(table, valid_b)
    out[~own] = mref.VOID_ROW
    return out


# ------------------------------------------------------------------------------------------------ link_correct
def conjugate(f, sx, sy):
    return [f[0], f[1], f[2] + sx * ONE - (f[0] * sx + f[1] * sy), f[3], f[4], f[5] + sy * ONE - (f[3] * sx + f[4] * sy)]


def correct_step(model, link, window, origin_a):
    """One row each, Python integers -> (link, out) as int64 arrays; the inputs are not changed."""
    m, ln = [int(v) for v in np.asarray(model).reshape(-1)], [int(v) for v in link]
    (y0, x0, _, _), (oy, ox) = window, origin_a
    status = OK
    if ln[12] not in (REGISTERED, INITIAL):
        status = NOT_LINKED
    elif m[12] != mref.OK or not mref.pair_in_bounds(m[0:6], m[6:12]):
        status = CORRECT_NO_FIT
    else:
        c, ci = conjugate(m[0:6], x0 - ox, y0 - oy), conjugate(m[6:12], x0 - ox, y0 - oy)
        if not mref.pair_in_bounds(c, ci):
            status = CORRECT_NO_FIT
        elif not mref.pose_in_bounds(ln[0:6], ln[6:12]):
            status = CORRECT_OUT_OF_BOUNDS
        else:
            a_to_b, b_to_a = mref.compose(ln[6:12], c), mref.compose(ci, ln[0:6])
            if not mref.pose_in_bounds(b_to_a, a_to_b):
                status = CORRECT_OUT_OF_BOUNDS
            else:
                ln = b_to_a + a_to_b + [REGISTERED, m[14], m[13], m[15]]
    return np.array(ln, np.int64), np.array([status, m[13], m[14], m[15], m[2], m[5], 0, 0], np.int64)


# ------------------------------------------------------------------------------------------------ mosaic_merge
def shifted_rank(rank_b, ordinal_offset, mode):
    """Python integers -> the rank word carried into A's ordinals, or None."""
    if rank_b == EMPTY:
        return None
    ordinal = (rank_b & 0xFFFFFFFF) + ordinal_offset
    if ordinal > ORDINAL_LAST:
        return None
    return ((0xFFFFFFFF - ordinal if oref.MODES[mode] == 1 else rank_b >> 32) << 32) | ordinal


def mosaic_merge_loop(votes_a, origin_a, votes_b, origin_b, link, ortho_a=None, ortho_b=None, ordinal_offset=0, mode="centre"):
    """The definition literally; A's planes are updated in place -> counts int64 [8]."""
    counts = [int(link[12]), 0, 0, 0, 0, 0, 0, 0]
    if not link_merges(link):
        return np.array(counts, np.int64)
    m = [int(v) for v in link[6:12]]
    (k_max, ch, cw), (_, ch_b, cw_b) = votes_a.shape, votes_b.shape
    for Y in range(ch):
        for X in range(cw):
            bx, by = b_pixel(m, X, Y, origin_a, origin_b)
            if not (0 <= bx < cw_b and 0 <= by < ch_b):
                continue
            counts[1] += 1
            more = [int(votes_b[k, by, bx]) for k in range(k_max)]
            counts[2] += int(any(more))
            counts[3] += sum(more)
            for k in range(k_max):
                votes_a[k, Y, X] = min(int(votes_a[k, Y, X]) + more[k], 65535)
            if ortho_a is not None:
                mine = shifted_rank(int(ortho_b[0][by, bx]), ordinal_offset, mode)
                if mine is not None and mine < int(ortho_a[0][Y, X]):     # strictly: ties stay with A
                    ortho_a[0][Y, X], ortho_a[1][Y, X] = mine, ortho_b[1][by, bx]
                    counts[4] += 1
    return np.array(counts, np.int64)


def mosaic_merge(votes_a, origin_a, votes_b, origin_b, link, ortho_a=None, ortho_b=None, ordinal_offset=0, mode="centre"):
    """Vectorised; A's planes are updated in place -> counts int64 [8]."""
    counts = [int(link[12]), 0, 0, 0, 0, 0, 0, 0]
    if not link_merges(link):
        return np.array(counts, np.int64)
    _, ch, cw = votes_a.shape
    bx, by, exists = b_pixels(link, (0, 0, ch, cw), origin_a, votes_b.shape[1:], origin_b)
    Y, X = np.nonzero(exists)
    bx, by = bx[Y, X], by[Y, X]
    more = votes_b[:, by, bx].astype(np.int64)
    counts[1], counts[2], counts[3] = len(Y), int((more.sum(0) > 0).sum()), int(more.sum())
    votes_a[:, Y, X] = np.minimum(votes_a[:, Y, X].astype(np.int64) + more, 65535).astype(np.uint16)
    if ortho_a is not None:
        rb = ortho_b[0][by, bx]
        ordinal = (rb & np.uint64(0xFFFFFFFF)).astype(np.int64) + ordinal_offset
        ok = (rb != np.uint64(EMPTY)) & (ordinal <= ORDINAL_LAST)
        ordinal = np.where(ok, ordinal, 0)
        high = 0xFFFFFFFF - ordinal if oref.MODES[mode] == 1 else (rb >> np.uint64(32)).astype(np.int64)
        mine = (high.astype(np.uint64) << np.uint64(32)) | ordinal.astype(np.uint64)
        win = ok & (mine < ortho_a[0][Y, X])
        ortho_a[0][Y[win], X[win]], ortho_a[1][Y[win], X[win]] = mine[win], ortho_b[1][by[win], bx[win]]
        counts[4] = int(win.sum())
    return np.array(counts, np.int64)


# ------------------------------------------------------------------------------------------------ merge_patch, link_place
PATCH_REACH = 1 << 15
PLACED, NOT_ATTEMPTED, NO_PLACEMENT, REJECTED_MEAN, REJECTED_UNIQUENESS, PATCH_REFUSED, PLACE_OUT_OF_BOUNDS = 0, 1, 2, 3, 4, 6, 7


def box_geometry(link, b_box, origin_b, size_a, origin_a, s):
    """Python integers -> geom [8]."""
    ln = [int(v) for v in link]
    (y0, x0, y1, x1), (oy_b, ox_b), (ch, cw), (oy, ox) = b_box, origin_b, size_a, origin_a
    if ln[12] not in (REGISTERED, INITIAL):
        return [lref.PATCH_NOT_LOST] + [0] * 7
    if not mref.pose_in_bounds(ln[0:6], ln[6:12]):
        return [lref.PATCH_OUT_OF_BOUNDS] + [0] * 7
    corners = [(x - ox_b, y - oy_b) for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
    xs = [ln[0] * x + ln[1] * y + ln[2] + ox * ONE for x, y in corners]
    ys = [ln[3] * x + ln[4] * y + ln[5] + oy * ONE for x, y in corners]
    X0, X1, Y0, Y1 = min(xs) >> 20, (max(xs) + ONE - 1) >> 20, min(ys) >> 20, (max(ys) + ONE - 1) >> 20
    if X0 - ox < -PATCH_REACH or X1 - ox > PATCH_REACH or Y0 - oy < -PATCH_REACH or Y1 - oy > PATCH_REACH:
        return [lref.PATCH_OUT_OF_BOUNDS] + [0] * 7
    pu0, pu1, pv0, pv1 = X0 // s, (X1 + s - 1) // s, Y0 // s, (Y1 + s - 1) // s
    tw, th = pu1 - pu0 if X1 > X0 else 0, pv1 - pv0 if Y1 > Y0 else 0
    if tw < 1 or th < 1 or tw * th > lref.MAX_PATCH_CELLS:
        return [lref.PATCH_CELLS] + [0] * 7
    if tw > cw // s or th > ch // s:
        return [lref.PATCH_WIDER] + [0] * 7
    return [lref.PATCH_OK, pu0, pv0, tw, th, 0, 0, 0]


def whole_box(size):
    return (0, 0, size[0], size[1])


def merge_patch_loop(rgba_b, origin_b, link, size_a, origin_a, s, b_box=None):
    """-> (tl, tv uint8 [th, tw], geom int64 [8]); a failing call has planes of no cell."""
    geom = box_geometry(link, whole_box(rgba_b.shape) if b_box is None else b_box, origin_b, size_a, origin_a, s)
    if geom[0] != lref.PATCH_OK:
        return np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8), np.array(geom, np.int64)
    _, pu0, pv0, tw, th = geom[:5]
    m = [int(v) for v in link[6:12]]
    tl, tv = np.zeros((th, tw), np.uint8), np.zeros((th, tw), np.uint8)
    for j in range(th):
        for i in range(tw):
            total, ok = 0, True
            for q in range(s):
                for p in range(s):
                    bx, by = b_pixel(m, (pu0 + i) * s + p, (pv0 + j) * s + q, origin_a, origin_b)
                    if not (0 <= bx < rgba_b.shape[1] and 0 <= by < rgba_b.shape[0]) or int(rgba_b[by, bx]) >> 24 == 0:
                        ok = False
                        continue
                    total += rref.luma_of(int(rgba_b[by, bx]))
            if ok:
                tl[j, i], tv[j, i] = lref.cell_mean(total, s), 1
    geom[5] = int(tv.sum())
    return tl, tv, np.array(geom, np.int64)


def merge_patch(rgba_b, origin_b, link, size_a, origin_a, s, b_box=None):
    """Vectorised."""
    geom = box_geometry(link, whole_box(rgba_b.shape) if b_box is None else b_box, origin_b, size_a, origin_a, s)
    if geom[0] != lref.PATCH_OK:
        return np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8), np.array(geom, np.int64)
    _, pu0, pv0, tw, th = geom[:5]
    bx, by, exists = b_pixels(link, (pv0 * s, pu0 * s, th * s, tw * s), origin_a, rgba_b.shape, origin_b)
    px = rgba_b[np.clip(by, 0, rgba_b.shape[0] - 1), np.clip(bx, 0, rgba_b.shape[1] - 1)].astype(np.int64)
    ok = exists & ((px >> 24) != 0)
    tv = ok.reshape(th, s, tw, s).all(axis=(1, 3))
    tl = lref.cell_mean(np.where(ok, rref.luma_of(px), 0).reshape(th, s, tw, s).sum(axis=(1, 3)), s)
    geom[5] = int(tv.sum())
    return np.where(tv, tl, 0).astype(np.uint8), tv.astype(np.uint8), np.array(geom, np.int64)


def place_step(found, link, s, max_mean=16, ratio=800):
    """Python integers -> (candidate link, out) as int64 arrays."""
    f, ln = [int(v) for v in found], [int(v) for v in link]
    decision, moved = PLACED, None
    if ln[12] not in (REGISTERED, INITIAL):
        decision = NOT_ATTEMPTED
    elif f[0] == lref.FOUND_NONE:
        decision = NO_PLACEMENT
    elif (f[0] != lref.FOUND or not mref.pose_in_bounds(ln[0:6], ln[6:12]) or not lref._pair_ok(f[3], f[4]) or abs(f[1]) > 16384 or abs(f[2]) > 16384
          or (f[5] != 0 and not lref._pair_ok(f[8], f[9]))):
        decision = PATCH_REFUSED
    elif f[3] > max_mean * f[4]:
        decision = REJECTED_MEAN
    elif f[5] != 0 and 1000 * f[3] * f[9] > ratio * f[8] * f[4]:
        decision = REJECTED_UNIQUENESS
    else:
        moved = lref.translate(ln[0:6], ln[6:12], s * f[1], s * f[2])
        if not mref.pose_in_bounds(*moved):
            decision = PLACE_OUT_OF_BOUNDS
    cand = list(moved[0]) + list(moved[1]) + [INITIAL, 0, 0, 0] if decision == PLACED else ln
    out = [decision, 0, 0, 0, 0, 0, 0, 0]
    if f[0] == lref.FOUND and abs(f[1]) <= 16384 and abs(f[2]) <= 16384:
        out[1:5] = [s * f[1], s * f[2], f[3], f[4]]
        if f[5] != 0:
            out[5:7] = [f[8], f[9]]
    if f[0] in (lref.FOUND, lref.FOUND_NONE):
        out[7] = f[11]
    return np.array(cand, np.int64), np.array(out, np.int64)


def place_cases():
    """(name, found, link, max_mean, ratio, code) for link_place: every code."""
    link = link_row(*mref.affine_pose(1.01, -0.03, 0.03, 0.99, 40.5, -17.25), status=REGISTERED, tail=(7, 8, 9))
    edge = link_row(*mref.affine_pose(1, 0, 0, 1, 16380, 0))
    broken = link.copy()
    broken[6] = 16 * ONE
    fr = lambda **kw: np.array(lref.found_row(**kw), np.int64)  # noqa: E731
    bad_n = fr(u=1, v=1, sad=10, n=5)
    bad_n[4] = 70000
    return [("placed", fr(u=3, v=-2, sad=40, n=20, second=(5, 5, 400, 20), eligible=9), link, 16, 800, PLACED),
            ("placed without a runner-up", fr(u=-7, v=0, sad=0, n=5), link_row(), 0, 1, PLACED),
            ("a tie: the runner-up is as good", fr(u=3, v=-2, sad=40, n=20, second=(9, 9, 40, 20)), link, 16, 800, REJECTED_UNIQUENESS),
            ("mean", fr(u=3, v=-2, sad=17 * 20, n=20), link, 16, 800, REJECTED_MEAN), ("none", fr(status=lref.FOUND_NONE, eligible=0), link, 16, 800, NO_PLACEMENT),
            ("bad geom", fr(status=lref.FOUND_BAD_GEOM), link, 16, 800, PATCH_REFUSED), ("bad counts", bad_n, link, 16, 800, PATCH_REFUSED),
            ("link out of bounds", fr(u=1, v=1, sad=0, n=5), broken, 16, 800, PATCH_REFUSED), ("moved out of bounds", fr(u=2, v=0, sad=0, n=5), edge, 16, 800, PLACE_OUT_OF_BOUNDS),
            ("no-fit link", fr(u=1, v=1, sad=0, n=5), link_row(status=NO_FIT), 16, 800, NOT_ATTEMPTED)]


def patch_links():
    """(name, link, b_box, canvas A, origin B, status) for merge_patch at S = 4 and 8: every status.  The canvas B is view_canvases', but
    for "too many cells", which takes patch_big_b() (200 x 272): 64 x 112 pixels cannot make 65536 cells of 8 x 8 under any link in bounds."""
    c, s = 1.03 * np.cos(np.radians(4)), 1.03 * np.sin(np.radians(4))
    ob, far = VIEW_ORIGIN_B, (-16384, -16384)
    return [("identity", link_row(status=REGISTERED), None, VIEW_A, ob, 0), ("shift", link_row(*mref.affine_pose(1, 0, 0, 1, 13, -6)), None, VIEW_A, ob, 0),
            ("rotation and zoom", link_row(*mref.affine_pose(c, -s, s, c, 21.5, 7.25)), None, (128, 192), ob, 0),
            ("a smaller box", link_row(*mref.affine_pose(1, 0, 0, 1, 13, -6)), (8, 16, 40, 81), VIEW_A, ob, 0),
            ("partly off the canvas", link_row(*mref.affine_pose(1, 0, 0, 1, -60, -30)), None, VIEW_A, ob, 0),
            ("no-fit link", link_row(status=NO_FIT), None, VIEW_A, ob, 1), ("out of bounds", link_row([16 * ONE, 0, 0, 0, ONE, 0], mref.IDENTITY), None, VIEW_A, ob, 2),
            ("too far", link_row(*mref.affine_pose(15, 0, 0, 15, 0, 0)), None, (16384, 16384), far, 2),
            ("too many cells", link_row(*mref.affine_pose(15.9, 0, 0, 15.9, 0, 0)), None, (16384, 16384), (0, 0), 3),
            ("wider than the map", link_row(status=REGISTERED), None, (48, 64), ob, 4)]


def patch_big_b():
    return np.zeros((200, 272), np.uint32)    # 15.9 x 272 / 8 = 541 cells by 15.9 x 200 / 8 = 398: past 65536 at S = 8 too


def patch_canvas_b(name):
    return patch_big_b() if name == "too many cells" else view_canvases()[1]


# ------------------------------------------------------------------------------------------------ the register sequence
REGISTER_DEFAULTS = dict(rounds=2, search=16, intra_bias=0, fit_rounds=4, tol=ONE, min_inliers=12)
PLACE_DEFAULTS = dict(min_overlap=500, exclude=2, max_mean=16, ratio=800, b_box=None)


def place_link(a, b, link, scale, min_overlap=500, exclude=2, max_mean=16, ratio=800, b_box=None, patch=merge_patch, coarse=lref.map_coarse, locate=lref.map_locate):
    """The coarse placement ops.register_mosaics(place=) runs first -> (the candidate link, link_place's out row)."""
    (rgba_a, origin_a), (rgba_b, origin_b) = a, b
    cl, cv = coarse(rgba_a, scale)
    tl, tv, geom = patch(rgba_b, origin_b, link, rgba_a.shape, origin_a, scale, b_box)
    found = locate(cl, cv, tl, tv, geom, min_overlap, exclude)
    return place_step(found, link, scale, max_mean, ratio)


def register_mosaics(a, b, link, rounds=2, search=16, intra_bias=0, fit_rounds=4, tol=ONE, min_inliers=12, window=None, place=None, view=merge_view,
                     gate=merge_gate):
    """What ops.register_mosaics enqueues (tol in Q20) -> (link, outs int64 [rounds (+ 1 with place: link_place's row first), 8], the last
    round's (cur, view, valid_a, valid_b, table))."""
    (rgba_a, origin_a), (rgba_b, origin_b) = a, b
    window = whole_window(rgba_a.shape) if window is None else window
    link, outs, last = np.array(link, np.int64), [], None
    if place is not None:
        link, out = place_link(a, b, link, **place)
        outs.append(out)
    for _ in range(rounds):
        cur, seen, valid_a, valid_b = view(rgba_a, origin_a, rgba_b, origin_b, link, window)
        table, _, _, stats = mmref.block_match_modes(cur, seen, search, 0, intra_bias)
        table = gate(table, valid_a, valid_b)
        model = mref.global_motion([table], window[2:], window[2:], fit_rounds, tol, min_inliers, None, 0, [stats])
        link, out = correct_step(model[0], link, window, origin_a)
        outs.append(out)
        last = (cur, seen, valid_a, valid_b, table)
    return link, np.array(outs, np.int64), last


# ------------------------------------------------------------------------------------------------ the split flight
SPLIT_CANVAS, SPLIT_ORIGIN, SPLIT_CLASSES, SPLIT_AT = rref.FLIGHT_CANVAS, rref.FLIGHT_ORIGIN, 4, 3


def run_part(images, masks, tables, mode, canvas_size=SPLIT_CANVAS, origin=SPLIT_ORIGIN, classes=SPLIT_CLASSES):
    """One mosaic of one uninterrupted chain, as FlowPredictor(mosaic=, ortho=) keeps it: the pair tables' models through pose_chain (row 0
    is the anchor's and ignored), the masks into the vote canvas, the images into the orthophoto with ordinals 0, 1, ...
    -> dict(votes, rank, rgba, poses, state, tail = the state's two poses after the last frame, frames)."""
    size = images[0].shape[:2]
    model = mref.global_motion(tables, size, size, **mref.SCENE_SETTINGS)
    poses, state = mref.pose_chain(model, np.zeros(32, np.int64), size, canvas_size, origin)
    votes = mref.mosaic_accumulate(np.stack(masks), poses, np.zeros((classes,) + tuple(canvas_size), np.uint16), origin)
    rank, rgba = oref.canvas(canvas_size)
    for f, img in enumerate(images):
        oref.ortho_accumulate(img, poses[f], f, rank, rgba, origin, mode)
    return dict(votes=votes, rank=rank, rgba=rgba, poses=poses, state=state, tail=state[:12].copy(), frames=len(images), inputs=(images, masks, tables))


@functools.lru_cache(maxsize=None)
def split_flight(mode="centre", at=SPLIT_AT):
    """rref's straight flight (six 64 x 96 frames, 4 px further right each) with exact pair tables and a four-class mask cut from the same
    ground, mosaicked three times: whole, frames 0..at-1 (A) and frames at..5 (B, its own anchor and ordinals from 0).
    -> (whole, a, b, the initial link: A's tail with status 1, frame `at`'s exact b_to_a)."""
    offsets = [rref.FLIGHT_STEP * f for f in range(6)]
    images, tables, true = rref.flight(offsets, bias=(0, 0))
    (h, w), g = rref.FLIGHT_SIZE, rref.ground()
    masks = [np.ascontiguousarray(g[32:32 + h, 64 + x:64 + x + w, 1] >> 6) for x in offsets]
    whole = run_part(images, masks, tables, mode)
    a = run_part(images[:at], masks[:at], tables[:at], mode)
    b = run_part(images[at:], masks[at:], tables[at:], mode)
    link = link_row(a["tail"][0:6], a["tail"][6:12], INITIAL)
    return whole, a, b, link, [ONE, 0, true[at][0] * ONE, 0, ONE, true[at][1] * ONE]


def merge_parts(a, b, link, mode, **register):
    """Register b against a copy of a and merge it -> (the merged dict, link, outs, counts)."""
    link = np.array(link, np.int64)
    merged = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    link, outs, _ = register_mosaics((merged["rgba"], SPLIT_ORIGIN), (b["rgba"], SPLIT_ORIGIN), link, **register)
    counts = mosaic_merge(merged["votes"], SPLIT_ORIGIN, b["votes"], SPLIT_ORIGIN, link, (merged["rank"], merged["rgba"]), (b["rank"], b["rgba"]), a["frames"], mode)
    return merged, link, outs, counts


CUT_OFFSETS_A, CUT_OFFSETS_B, CUT_BOX_B = (0, 4, 8, 12), (36, 32, 28), (32, 40, 96, 144)


@functools.lru_cache(maxsize=None)
def cut_parts(mode="centre"):
    """A flight with a cut onto new ground whose second half later pans back over the first: A maps offsets 0..12, then the camera
    jumps 24 px (beyond the default search of 16) and B, a chain of its own, pans back from 36 to 28.  -> (a, b, the default initial
    link: A's tail with status 1, the exact b_to_a, B's seen bounding box in its canvas)."""
    (h, w), g = rref.FLIGHT_SIZE, rref.ground()
    parts = []
    for offsets in (CUT_OFFSETS_A, CUT_OFFSETS_B):
        images, tables, _ = rref.flight(list(offsets), bias=(0, 0))
        masks = [np.ascontiguousarray(g[32:32 + h, 64 + x:64 + x + w, 1] >> 6) for x in offsets]
        parts.append(run_part(images, masks, tables, mode))
    a, b = parts
    return a, b, link_row(a["tail"][0:6], a["tail"][6:12], INITIAL), [ONE, 0, CUT_OFFSETS_B[0] * ONE, 0, ONE, 0], CUT_BOX_B


# ------------------------------------------------------------------------------------------------ the cases of the op tests
VIEW_A, VIEW_B, VIEW_ORIGIN_A, VIEW_ORIGIN_B = (96, 160), (64, 112), (20, 30), (9, 14)


def view_canvases(seed=31):
    """A 96 x 160 and B 64 x 112 rgba canvases of random seen pixels with unseen holes (one of them with colour bits under alpha 0)."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 1 << 24, size=VIEW_A).astype(np.uint32) | np.uint32(0xFF000000)
    b = rng.randint(0, 1 << 24, size=VIEW_B).astype(np.uint32) | np.uint32(0xFF000000)
    a[10:23, 40:61] = 0
    a[70:, :17] &= np.uint32(0x00FFFFFF)
    b[20:31, 50:77] = 0
    b[:5, 90:] &= np.uint32(0x00FFFFFF)
    return a, b


def view_links():
    """(name, link): the identity, a whole-pixel shift, a rotation with zoom, B wholly outside, a no-fit link, a link out of bounds."""
    c, s = 1.03 * np.cos(np.radians(4)), 1.03 * np.sin(np.radians(4))
    far = mref.affine_pose(1, 0, 0, 1, 3000, -2000)
    return [("identity", link_row(status=REGISTERED)), ("shift", link_row(*mref.affine_pose(1, 0, 0, 1, 13, -6))),
            ("rotation and zoom", link_row(*mref.affine_pose(c, -s, s, c, 21.5, 7.25), status=REGISTERED)), ("outside", link_row(*far)),
            ("no fit", link_row(*mref.affine_pose(1, 0, 0, 1, 13, -6), status=NO_FIT)), ("out of bounds", link_row([16 * ONE, 0, 0, 0, ONE, 0], mref.IDENTITY))]


VIEW_WINDOWS = (None, (16, 48, 64, 96))


def gate_cases():
    """(name, table, valid_a, valid_b, rows that survive).  The small plane is 32 x 48 (six blocks)."""
    va, vb = np.ones((32, 48), np.uint8), np.ones((32, 48), np.uint8)
    va[5, 20] = 0                                               # block 1's own window
    vb[:, 40:] = 0
    t = mref.grid_table(2, 3, lambda cx, cy: (np.zeros_like(cx), np.zeros_like(cy)))
    t[2, 3], t[3, 3], t[4, 3], t[5] = 33, 7, 32, mref.VOID_ROW  # over valid_b's edge; one pixel out of the plane; touching the edge (kept); void in
    va2, vb2 = np.ones((96, 160), np.uint8), np.ones((96, 160), np.uint8)
    va2[40:60, 100:] = 0
    vb2[:30, :50] = 0
    vb2[70, 70] = 2                                             # neither 0 nor 1: not valid
    rng = np.random.RandomState(4)
    big = mref.grid_table(6, 10, lambda cx, cy: (rng.randint(-9, 10, size=cx.shape), rng.randint(-9, 10, size=cy.shape)))
    big[7, 3], big[8, 4] = 2 ** 31 - 1, -2 ** 31                # garbage: the 64-bit test
    return [("small", t, va, vb, [0, 4]), ("large", big, va2, vb2, None)]


CORRECT_WINDOW, CORRECT_ORIGIN = (16, 48, 64, 96), (20, 30)


def correct_cases():
    """(name, model row, link, status) for link_correct: every status, the other ways into 2 and 3, and a result exactly at the bound."""
    fwd, inv = mref.affine_pose(1.001, 0.002, -0.002, 0.999, -1.25, 0.5)
    good = np.array(mref.model_row(fwd, inv, mref.OK, 20, 16, 4), np.int64)
    shift = np.array(mref.model_row(*mref.affine_pose(1, 0, 0, 1, 3, -2), mref.OK, 30, 28, 4), np.int64)
    few = np.array(mref.model_row(mref.IDENTITY, mref.IDENTITY, mref.FEW, 3, 0, 0), np.int64)
    wild = good.copy()
    wild[1] = 3 * ONE
    spin = np.array(mref.model_row([ONE, 0, 0, 0, ONE, 0], [ONE, 0, -((1 << 16) * ONE - 1), 0, ONE, 0], mref.OK, 20, 16, 4), np.int64)
    spin[0], spin[6] = 2 * ONE, 2 * ONE                          # in the pair bounds itself; conjugated at s = (18, -4) it leaves them
    link = link_row(*mref.affine_pose(1.01, -0.03, 0.03, 0.99, 40.5, -17.25), status=INITIAL, tail=(7, 8, 9))
    at_edge = link_row([ONE, 0, (1 << 14) * ONE - 1 - 3 * ONE, 0, ONE, 0], [ONE, 0, -((1 << 14) * ONE - 1 - 3 * ONE), 0, ONE, 0], REGISTERED)
    over_edge = link_row([ONE, 0, (1 << 14) * ONE - 3 * ONE, 0, ONE, 0], [ONE, 0, -((1 << 14) * ONE - 3 * ONE), 0, ONE, 0], REGISTERED)
    back = np.array(mref.model_row(*mref.affine_pose(1, 0, 0, 1, -3, 0), mref.OK, 30, 28, 4), np.int64)   # C^-1 moves b_to_a by +3 px
    broken = link.copy()
    broken[0] = 16 * ONE
    return [("corrected", good, link, OK), ("registered link", shift, link_row(status=REGISTERED), OK), ("too few", few, link, CORRECT_NO_FIT),
            ("out of the pair bounds", wild, link, CORRECT_NO_FIT), ("conjugated out of the pair bounds", spin, link, CORRECT_NO_FIT),
            ("exactly at the pose bound", back, at_edge, OK), ("one past the pose bound", back, over_edge, CORRECT_OUT_OF_BOUNDS),
            ("link out of bounds", good, broken, CORRECT_OUT_OF_BOUNDS), ("no-fit link", good, link_row(status=NO_FIT), NOT_LINKED),
            ("garbage status", good, link_row(status=77), NOT_LINKED)]


MERGE_A, MERGE_B, MERGE_ORIGIN_A, MERGE_ORIGIN_B = (100, 150), (70, 90), (20, 30), (9, 14)


def merge_mosaics(k, seed=17, mode="centre", first_ordinal_b=0):
    """Two mosaics with random votes (some cells near or at 65535 on either side, some pixels of B without a vote) and orthophotos written
    by random ranks of `mode` (some empty, some equal on both sides under the identity link with offset 0)
    -> (votes_a, (rank_a, rgba_a), votes_b, (rank_b, rgba_b))."""
    rng = np.random.RandomState(seed + k)
    out = []
    for size in (MERGE_A, MERGE_B):
        votes = rng.randint(0, 40, size=(k,) + size).astype(np.uint16)
        votes[:, rng.rand(*size) < 0.1] = 0
        hot = rng.rand(k, *size) < 0.05
        votes[hot] = rng.randint(65500, 65536, size=int(hot.sum())).astype(np.uint16)
        ordinal = rng.randint(0, 50, size=size).astype(np.uint64)
        key = (np.uint64(0xFFFFFFFF) - ordinal) if mode == "latest" else rng.randint(0, 9, size=size).astype(np.uint64)
        rank = (key << np.uint64(32)) | ordinal
        rgba = rng.randint(0, 1 << 24, size=size).astype(np.uint32) | np.uint32(0xFF000000)
        empty = rng.rand(*size) < 0.15
        rank[empty], rgba[empty] = np.uint64(EMPTY), 0
        out += [votes, (rank, rgba)]
    return tuple(out)


def merge_links():
    """(name, link, does it merge)."""
    c, s = 0.98 * np.cos(np.radians(-3)), 0.98 * np.sin(np.radians(-3))
    return [("identity", link_row(status=REGISTERED), True), ("shift", link_row(*mref.affine_pose(1, 0, 0, 1, 37, 22), status=REGISTERED), True),
            ("rotation and zoom", link_row(*mref.affine_pose(c, -s, s, c, 11.5, 3.25), status=REGISTERED), True),
            ("out of reach", link_row(*mref.affine_pose(1, 0, 0, 1, 5000, 100), status=REGISTERED), True),
            ("initial", link_row(*mref.affine_pose(1, 0, 0, 1, 37, 22), status=INITIAL), False), ("no fit", link_row(status=NO_FIT), False),
            ("out of bounds", link_row([16 * ONE, 0, 0, 0, ONE, 0], mref.IDENTITY, REGISTERED), False)]


# ------------------------------------------------------------------------------------------------ the library's refusals
def good_arguments():
    """Per op the arguments of a call that passes validation (dummy non-null pointers), in the ABI's order, by name."""
    return {
        "merge_view": dict(rgba_a=64, CH_a=200, CW_a=300, ox_a=36, oy_a=54, rgba_b=128, CH_b=100, CW_b=150, ox_b=3, oy_b=5, link=64, Y0=16, X0=32, WH=64, WW=96,
                           cur=64, view=64, valid_a=64, valid_b=64, stream=None),
        "merge_gate": dict(table=64, blocks=96, valid_a=64, valid_b=64, H=128, W=192, stream=None),
        "link_correct": dict(model=64, link=192, Y0=16, X0=32, WH=64, WW=96, ox_a=36, oy_a=54, out=64, stream=None),
        "mosaic_merge": dict(votes_a=64, CH_a=200, CW_a=300, ox_a=36, oy_a=54, votes_b=128, CH_b=100, CW_b=150, ox_b=3, oy_b=5, K=5, link=64, rank_a=64, rgba_a=64,
                             rank_b=128, rgba_b=128, ordinal_offset=7, mode=0, counts=64, stream=None),
        "merge_patch": dict(rgba_b=64, CH_b=100, CW_b=150, ox_b=3, oy_b=5, link=64, CH_a=200, CW_a=300, ox_a=36, oy_a=54, S=8, y0=10, x0=20, y1=90, x1=140, tl=64, tv=64,
                            geom=64, stream=None),
        "link_place": dict(found=64, link=64, S=8, max_mean=16, ratio_permille=800, cand=128, out=64, stream=None),
    }


def refusal_cases():
    """(op, changed arguments, a word of the message)."""
    view, gate, fix, merge = "merge_view", "merge_gate", "link_correct", "mosaic_merge"
    cases = [(view, {p: None}, b"null") for p in ("rgba_a", "rgba_b", "link", "cur", "view", "valid_a", "valid_b")]
    cases += [(view, dict(CH_a=0), b"canvas A"), (view, dict(CW_a=16385), b"16385"), (view, dict(CH_b=0), b"canvas B"), (view, dict(CW_b=16385), b"16385"),
              (view, dict(ox_a=16385), b"origin A"), (view, dict(oy_b=-16385), b"origin B"), (view, dict(WH=0), b"window"), (view, dict(WW=40), b"40)"),
              (view, dict(WH=8), b"window"), (view, dict(Y0=-16), b"-16"), (view, dict(Y0=144), b"144"), (view, dict(X0=208), b"208"), (view, dict(rgba_b=64), b"same memory"),
              (view, dict(rgba_a=66), b"aligned to 4"), (view, dict(link=68), b"aligned to 8"), (view, dict(cur=66), b"aligned to 4"), (view, dict(valid_b=65), b"aligned to 4")]
    cases += [(gate, {p: None}, b"null") for p in ("table", "valid_a", "valid_b")]
    cases += [(gate, dict(H=15, blocks=0), b"15x"), (gate, dict(W=16385), b"16385"), (gate, dict(blocks=95), b"blocks=95"), (gate, dict(table=66), b"aligned to 4")]
    cases += [(fix, {p: None}, b"null") for p in ("model", "link", "out")]
    cases += [(fix, dict(WH=24), b"24"), (fix, dict(WW=0), b"window"), (fix, dict(X0=-1), b"-1"), (fix, dict(Y0=16384), b"16384"), (fix, dict(ox_a=16385), b"origin"),
              (fix, dict(oy_a=-16385), b"origin"), (fix, dict(model=68), b"aligned to 8"), (fix, dict(link=68), b"aligned to 8"), (fix, dict(out=68), b"aligned to 8"),
              (fix, dict(link=64), b"same memory")]
    cases += [(merge, {p: None}, b"null") for p in ("votes_a", "votes_b", "link", "counts", "rank_a", "rgba_b")]
    cases += [(merge, dict(CH_a=0), b"canvas A"), (merge, dict(CW_b=16385), b"canvas B"), (merge, dict(ox_a=-16385), b"origin A"), (merge, dict(oy_b=16385), b"origin B"),
              (merge, dict(K=0), b"classes=0"), (merge, dict(K=33), b"classes=33"), (merge, dict(mode=2), b"mode=2"), (merge, dict(ordinal_offset=0xFFFFFFFF), b"4294967295"),
              (merge, dict(votes_b=64), b"same memory"), (merge, dict(rank_b=64), b"same memory"), (merge, dict(rgba_b=64), b"same memory"),
              (merge, dict(votes_a=65), b"aligned to 2"), (merge, dict(link=68), b"aligned to 8"), (merge, dict(counts=68), b"aligned to 8"),
              (merge, dict(rank_a=68), b"aligned to 8"), (merge, dict(rgba_b=130), b"aligned to 4")]
    patch, place = "merge_patch", "link_place"
    cases += [(patch, {p: None}, b"null") for p in ("rgba_b", "link", "tl", "tv", "geom")]
    cases += [(patch, dict(CH_a=0), b"canvas A"), (patch, dict(CW_b=16385), b"canvas B"), (patch, dict(ox_a=16385), b"origin A"), (patch, dict(oy_b=-16385), b"origin B"),
              (patch, dict(S=5), b"S=5"), (patch, dict(CH_a=7), b"no cell"), (patch, dict(y1=10), b"b_box"), (patch, dict(x1=151), b"151"), (patch, dict(y0=-1), b"-1"),
              (patch, dict(rgba_b=66), b"aligned to 4"), (patch, dict(link=68), b"aligned to 8"), (patch, dict(geom=68), b"aligned to 8")]
    cases += [(place, {p: None}, b"null") for p in ("found", "link", "cand", "out")]
    cases += [(place, dict(S=32), b"S=32"), (place, dict(max_mean=256), b"256"), (place, dict(max_mean=-1), b"-1"), (place, dict(ratio_permille=0), b"got 0"),
              (place, dict(ratio_permille=1001), b"1001"), (place, dict(found=68), b"aligned to 8"), (place, dict(cand=68), b"aligned to 8"), (place, dict(cand=64), b"the link itself")]
    return cases


def call_op(lib, op, **changed):
    args = dict(good_arguments()[op])
    args.update(changed)
    return getattr(lib, "fs_" + op)(*args.values())
