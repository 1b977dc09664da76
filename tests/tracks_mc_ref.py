"""The definition of the motion-compensated region links (include/floodseg_test.h: region_links_mc) in plain numpy, and
the cases the CPU and the GPU tests share.  tracks_ref is imported, not edited: the compensated op IS tracks_ref.region_links on a
previous index plane that was warped by the block vectors beforehand.  Everything is integer; // is floor division.

  mask H x W, decoded frame FH x FW, hb = FH // 16, wb = FW // 16, mv[f] = int32 [hb * wb][7] of frame f against frame f-1
  pixel (y, x)   fy = ((2y+1) FH) // (2H), fx = ((2x+1) FW) // (2W); block by = fy // 16, bx = fx // 16; by >= hb or bx >= wb: shift (0, 0)
  row r          void (shift (0, 0)) when r[5] < 0 or r[6] < 0; else vx = r[3] - r[5], vy = r[4] - r[6]; |vx| or |vy| > 1024: void
  shift          sx = sign(vx) ((2 |vx| W + FW) // (2 FW)), sy likewise with H, FH; the source of (y, x) is (y + sy, x + sx)
  overlap(a, b)  pixels p of frame f with index[f][p] == b, a source inside the mask and index[f-1][source] == a
  cut            pair_stats[f][2] != 0: no links at all for the pair, link_counts[f] = (0, 2) (frame 0 without a frame before it: (0, 0))
"""
import functools

import numpy as np

import regions_ref as rref
import tracks_ref as ref

VOID_ROW = (-1, 16, 16, -16, -16, -16, -16)
MAX_VECTOR = 1024
# (mask H, W, frame FH, FW): identity scale with one partial wave per row; ragged scale on both axes with a 256-pixel piece border and a
# ragged last wave; shifts doubled; remainder strips on both axes
GEOMETRIES = [(48, 80, 48, 80), (37, 300, 48, 320), (96, 160, 48, 80), (50, 90, 50, 90)]
TABLES = ["uniform", "per_block", "outward", "void_mixed", "pm32", "garbage"]
FRAMES = 3
BLOB_SCENE = dict(n=4, hw=(96, 160), step=(3, 12), size=8, pitch=32)


# ------------------------------------------------------------------------------------------------ the definition
def shifts(mv, h, w, fh, fw):
    """The (sy, sx) int64 [h, w] planes of one frame's table mv int32 [hb * wb, 7]."""
    hb, wb = fh // 16, fw // 16
    mv = np.asarray(mv).astype(np.int64).reshape(hb * wb, 7)               # 64-bit: a garbage row must not wrap around
    y, x = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
    by, bx = ((2 * y + 1) * fh) // (2 * h) // 16, ((2 * x + 1) * fw) // (2 * w) // 16
    inside = (by[:, None] < hb) & (bx[None, :] < wb)
    row = mv[np.minimum(by, hb - 1)[:, None] * wb + np.minimum(bx, wb - 1)[None, :]]
    vx, vy = row[..., 3] - row[..., 5], row[..., 4] - row[..., 6]
    use = inside & (row[..., 5] >= 0) & (row[..., 6] >= 0) & (abs(vx) <= MAX_VECTOR) & (abs(vy) <= MAX_VECTOR)
    sx = np.sign(vx) * ((2 * abs(vx) * w + fw) // (2 * fw))
    sy = np.sign(vy) * ((2 * abs(vy) * h + fh) // (2 * fh))
    return np.where(use, sy, 0), np.where(use, sx, 0)


def warp_prev(prev_index, mv, fh, fw):
    """The previous index plane gathered at every pixel's source; -1 where the source lies outside the mask."""
    h, w = prev_index.shape
    sy, sx = shifts(mv, h, w, fh, fw)
    yy, xx = np.mgrid[0:h, 0:w]
    ys, xs = yy + sy, xx + sx
    ok = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    return np.where(ok, prev_index[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)], -1).astype(np.int32)


def region_links_mc(index, table, counts, mv, frame_size, prev=None, pair_stats=None, max_pairs=None, min_overlap=1):
    """-> back int32 [n,R,2], fwd int32 [n,R,2], link_counts int64 [n,2]: per pair the warp, then tracks_ref.region_links."""
    n, cap = index.shape[0], table.shape[1]
    back, fwd = np.zeros((n, cap, 2), np.int32), np.zeros((n, cap, 2), np.int32)
    back[..., 0] = fwd[..., 0] = -1
    link_counts = np.zeros((n, 2), np.int64)
    for f in range(n):
        if f == 0 and prev is None:
            continue
        if pair_stats is not None and pair_stats[f][2] != 0:
            link_counts[f] = (0, 2)
            continue
        ia, ta, ca = (index[f - 1], table[f - 1], counts[f - 1]) if f else prev
        s = slice(f, f + 1)
        back[s], fwd[s], link_counts[s] = ref.region_links(index[s], table[s], counts[s], (warp_prev(ia, mv[f], *frame_size), ta, ca), max_pairs, min_overlap)
    return back, fwd, link_counts


def region_links_mc_bruteforce(index, table, counts, mv, frame_size, prev=None, pair_stats=None, max_pairs=None, min_overlap=1):
    """The same by a loop over the pixels with plain Python integers, nothing shared with the functions above."""
    n, h, w = index.shape
    fh, fw = frame_size
    hb, wb = fh // 16, fw // 16
    cap = table.shape[1]
    max_pairs = ref.default_max_pairs(cap) if max_pairs is None else max_pairs
    back, fwd = np.zeros((n, cap, 2), np.int32), np.zeros((n, cap, 2), np.int32)
    back[..., 0] = fwd[..., 0] = -1
    link_counts = np.zeros((n, 2), np.int64)

    def scaled(v, p, fp):
        m = (2 * abs(v) * p + fp) // (2 * fp)
        return m if v >= 0 else -m

    for f in range(n):
        if f == 0 and prev is None:
            continue
        if pair_stats is not None and int(pair_stats[f][2]) != 0:
            link_counts[f] = (0, 2)
            continue
        ia, ta, ca = (index[f - 1], table[f - 1], counts[f - 1]) if f else prev
        rows = [[int(v) for v in r] for r in np.asarray(mv[f]).reshape(hb * wb, 7)]
        seen = {}
        for y in range(h):
            by = ((2 * y + 1) * fh) // (2 * h) // 16
            for x in range(w):
                bx = ((2 * x + 1) * fw) // (2 * w) // 16
                sy = sx = 0
                if by < hb and bx < wb:
                    r = rows[by * wb + bx]
                    if r[5] >= 0 and r[6] >= 0 and abs(r[3] - r[5]) <= MAX_VECTOR and abs(r[4] - r[6]) <= MAX_VECTOR:
                        sx, sy = scaled(r[3] - r[5], w, fw), scaled(r[4] - r[6], h, fh)
                if not (0 <= y + sy < h and 0 <= x + sx < w):
                    continue
                a, b = int(ia[y + sy, x + sx]), int(index[f, y, x])
                if 0 <= a < min(cap, ca[1]) and 0 <= b < min(cap, counts[f][1]) and ta[a, 0] == table[f][b, 0]:
                    seen[(a, b)] = seen.get((a, b), 0) + 1
        if len(seen) > max_pairs:
            link_counts[f] = (max_pairs, 1)
            continue
        link_counts[f] = (len(seen), 0)
        for (a, b), c in sorted(seen.items()):
            if c >= min_overlap and c > back[f, b, 1]:
                back[f, b] = (a, c)
            if c >= min_overlap and c > fwd[f, a, 1]:
                fwd[f, a] = (b, c)
    return back, fwd, link_counts


# ------------------------------------------------------------------------------------------------ tables
def _rows(fh, fw, vx, vy):
    """Rows as the matcher writes them, destination = the block's centre, from per-block vectors (source minus destination)."""
    hb, wb = fh // 16, fw // 16
    by, bx = np.mgrid[0:hb, 0:wb]
    dx, dy = bx * 16 + 8, by * 16 + 8
    vx, vy = np.broadcast_to(vx, (hb, wb)), np.broadcast_to(vy, (hb, wb))
    t = np.stack([np.full((hb, wb), -1), np.full((hb, wb), 16), np.full((hb, wb), 16), dx + vx, dy + vy, dx, dy], -1)
    return t.reshape(hb * wb, 7).astype(np.int32)


def table_uniform(fh, fw, vx, vy):
    return _rows(fh, fw, vx, vy)


def table_void(fh, fw):
    return np.tile(np.array(VOID_ROW, np.int32), ((fh // 16) * (fw // 16), 1))


def make_table(kind, fh, fw, seed, motion=(0, 0)):
    """One frame's table of a kind of TABLES.  motion = the scene's (dy, dx) per frame in FRAME pixels, for "uniform"."""
    hb, wb = fh // 16, fw // 16
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return table_uniform(fh, fw, -motion[1], -motion[0])               # where it was = where it is - the motion
    if kind == "per_block":                                                # runs break at block edges inside a wave
        return _rows(fh, fw, rng.integers(-6, 7, (hb, wb)), rng.integers(-6, 7, (hb, wb)))
    if kind == "outward":                                                  # the border blocks point out of the frame on all four sides
        by, bx = np.mgrid[0:hb, 0:wb]
        vy = np.where(by == 0, -40, np.where(by == hb - 1, 40, rng.integers(-3, 4, (hb, wb))))
        vx = np.where(bx == 0, -40, np.where(bx == wb - 1, 40, rng.integers(-3, 4, (hb, wb))))
        return _rows(fh, fw, vx, vy)
    if kind == "void_mixed":
        t = _rows(fh, fw, rng.integers(-9, 10, (hb, wb)), rng.integers(-9, 10, (hb, wb)))
        t[rng.random(hb * wb) < 0.35] = VOID_ROW
        return t
    if kind == "pm32":
        return _rows(fh, fw, rng.choice([-32, 32], (hb, wb)), rng.choice([-32, 32], (hb, wb)))
    assert kind == "garbage"
    t = rng.integers(-2 ** 31, 2 ** 31, (hb * wb, 7), dtype=np.int64)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    made = [(0, 0, 0, hi, hi, 0, 0), (0, 0, 0, lo, 5, hi, 5), (0, 0, 0, hi, lo, 0, hi), (0, 0, 0, 5, 5, -1, 5), (0, 0, 0, 5, 5, 5, lo),
            (7, 7, 7, 1024 + 9, 9, 9, 9), (7, 7, 7, 1025 + 9, 9, 9, 9), (7, 7, 7, 9, 9, 1024 + 9, 9), (7, 7, 7, 9, 9, 1025 + 9, 9),
            (7, 7, 7, 9, 1024 + 9, 9, 9), (7, 7, 7, 9, 9, 9, 1025 + 9), (lo, hi, lo, 3, 12, 6, 8), (9, 9, 9, 2, 0, 0, 3)]
    at = rng.permutation(hb * wb)
    for j, row in enumerate(made[:hb * wb]):
        t[at[j]] = row
    return t.astype(np.int32)


# ------------------------------------------------------------------------------------------------ scenes
def blob_masks(n, hw, step, size, pitch):
    """size x size blobs of classes 0..2 on a pitch-pixel lattice over background, the whole lattice moving `step` = (dy, dx) per frame."""
    h, w = hw
    m = np.full((n, h, w), ref.BG, np.uint8)
    for f in range(n):
        for i, y0 in enumerate(range(-4 * pitch, h + 4 * pitch, pitch)):
            for j, x0 in enumerate(range(-4 * pitch, w + 4 * pitch, pitch)):
                y, x = y0 + 2 + f * step[0], x0 + 3 + f * step[1]
                ya, yb, xa, xb = max(y, 0), min(y + size, h), max(x, 0), min(x + size, w)
                if ya < yb and xa < xb:
                    m[f, ya:yb, xa:xb] = (i + j) % 3
    return m


def _stripes16(rows_per_stripe):
    m = np.zeros((2, 16, 16), np.uint8)
    m[0] = (np.arange(16)[:, None] // rows_per_stripe % 2)                  # horizontal stripes of classes 0, 1, 0, 1, ...
    m[1] = (np.arange(16)[None, :] // 2 % 2)                                # eight vertical ones
    return m


@functools.lru_cache(maxsize=None)
def case_list():
    cases = []
    b = BLOB_SCENE
    n, (h, w) = b["n"], b["hw"]
    cases.append(dict(name="blobs", mask=blob_masks(**b), classes=5, cap=64, frame_size=(h, w),
                      mv=np.stack([table_uniform(h, w, -b["step"][1], -b["step"][0])] * n)))
    for g, (h, w, fh, fw) in enumerate(GEOMETRIES):
        for pattern, shift in (("random5", (1, 2)), ("stripes", (5, -7))) if g == 1 else (("random5", (1, 2)),):
            mask = ref._pattern_frames((FRAMES, h, w), pattern, shift)
            motion = (round(shift[0] * fh / h), round(shift[1] * fw / w))
            for k, kind in enumerate(TABLES):
                cases.append(dict(name=f"{(h, w, fh, fw)} {pattern} {kind}", mask=mask, classes=rref.pattern_classes(pattern), cap=min(h * w + 1, 1024),
                                  frame_size=(fh, fw), mv=np.stack([make_table(kind, fh, fw, 1000 * g + 10 * k + f, motion) for f in range(FRAMES)])))
    for pattern in ("random5", "stripes"):                                  # tracks_ref's pattern scenes, uniform tables matching their SHIFTS
        for shift in ref.SHIFTS:
            geometry = ref.GEOMETRIES[1]
            n, h, w = geometry
            cases.append(dict(name=f"{geometry} {pattern} {shift} matched", mask=ref._pattern_frames(geometry, pattern, shift), classes=rref.pattern_classes(pattern),
                              cap=min(h * w + 1, 1024), frame_size=(h, w), mv=np.stack([table_uniform(h, w, -shift[1], -shift[0])] * n)))
    cases.append(dict(name="pairs_full", mask=_stripes16(4), classes=2, cap=16, max_pairs=16, frame_size=(16, 16), mv=np.stack([table_uniform(16, 16, 0, 0)] * 2)))
    cases.append(dict(name="pairs_overflow", mask=_stripes16(2), classes=2, cap=16, max_pairs=16, frame_size=(16, 16), mv=np.stack([table_uniform(16, 16, 2, 0)] * 2)))
    h, w, fh, fw = GEOMETRIES[1]
    blocks = (fh // 16) * (fw // 16)
    cases.append(dict(name="cut", mask=ref._pattern_frames((FRAMES, h, w), "random5", (1, 2)), classes=rref.pattern_classes("random5"), cap=1024, frame_size=(fh, fw),
                      mv=np.stack([make_table("per_block", fh, fw, 77 + f) for f in range(FRAMES)]),
                      pair_stats=np.array([[blocks, 0, 0, 0], [blocks, blocks, 1, 0], [blocks, 3, 0, 0]], np.int32)))
    for c in cases:
        c.setdefault("max_pairs", ref.default_max_pairs(c["cap"]))
        c.setdefault("min_overlap", 1)
        c.setdefault("pair_stats", None)
        c["mask"].setflags(write=False)
        c["mv"].setflags(write=False)
        assert c["mv"].dtype == np.int32 and c["mv"].shape == (len(c["mask"]), (c["frame_size"][0] // 16) * (c["frame_size"][1] // 16), 7), c["name"]
    return cases


def case_by_name(name):
    return next(i for i, c in enumerate(case_list()) if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _tables(mask_bytes, shape, classes, cap):
    mask = np.frombuffer(mask_bytes, np.uint8).reshape(shape)
    return rref.region_table(mask, rref.mask_regions(mask, classes, ref.CONN), classes, None, 128, cap)


@functools.lru_cache(maxsize=None)
def expected(i):
    """Everything the tests compare against for one case, computed once: the region tables, then compensated links and tracks of the
    whole clip in one call (no frame before frame 0, ids from 0)."""
    c = case_list()[i]
    table, counts, index = _tables(c["mask"].tobytes(), c["mask"].shape, c["classes"], c["cap"])
    back, fwd, link_counts = region_links_mc(index, table, counts, c["mv"], c["frame_size"], None, c["pair_stats"], c["max_pairs"], c["min_overlap"])
    tracks, state = ref.region_tracks(back, fwd, counts, np.zeros(2, np.int64), None)
    out = dict(c, table=table, counts=counts, index=index, back=back, fwd=fwd, link_counts=link_counts, tracks=tracks, state=state)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def chained(e, pieces):
    """The clip of expected() `e` in calls of the given lengths, each handed the last frame of the one before as prev."""
    backs, fwds, lcs, trs = [], [], [], []
    state, prev, prev_tracks, at = np.zeros(2, np.int64), None, None, 0
    for n in pieces:
        s = slice(at, at + n)
        stats = None if e["pair_stats"] is None else e["pair_stats"][s]
        back, fwd, lc = region_links_mc(e["index"][s], e["table"][s], e["counts"][s], e["mv"][s], e["frame_size"], prev, stats, e["max_pairs"], e["min_overlap"])
        tracks, state = ref.region_tracks(back, fwd, e["counts"][s], state, prev_tracks)
        backs.append(back), fwds.append(fwd), lcs.append(lc), trs.append(tracks)
        at += n
        prev, prev_tracks = (e["index"][at - 1], e["table"][at - 1], e["counts"][at - 1]), tracks[-1]
    return np.concatenate(backs), np.concatenate(fwds), np.concatenate(lcs), np.concatenate(trs), state


def clip_tracks(masks, classes, conn, cap, mvs, frame_size, max_pairs=None, min_overlap=1, resets=(), stats=None, compensate=True):
    """What FlowPredictor(track=True, compensate=...) keeps for a sequence of emitted masks with one table (and stats row) per frame: per
    frame the tracks rows [rows, 4], and the flag words.  `resets`: frame numbers in front of which reset() was called."""
    table, counts, index = rref.region_table(masks, rref.mask_regions(masks, classes, conn), classes, None, 128, cap)
    rows, flags = [], []
    state, prev, prev_tracks = np.zeros(2, np.int64), None, None
    for f in range(len(masks)):
        if f in resets:
            prev, prev_tracks = None, None
        s = slice(f, f + 1)
        if compensate:
            back, fwd, lc = region_links_mc(index[s], table[s], counts[s], mvs[s], frame_size, prev, None if stats is None else stats[s], max_pairs, min_overlap)
        else:
            back, fwd, lc = ref.region_links(index[s], table[s], counts[s], prev, max_pairs, min_overlap)
        tracks, state = ref.region_tracks(back, fwd, counts[s], state, prev_tracks)
        rows.append(tracks[0, :counts[f, 1]])
        flags.append(int(lc[0, 1]))
        prev, prev_tracks = (index[f], table[f], counts[f]), tracks[0]
    return rows, np.array(flags, np.int64)


def continued(rows):
    """(regions of frames 1.. whose track id the frame before already had, regions of frames 1.., ids spent)."""
    cont = total = 0
    for f in range(1, len(rows)):
        cont += int(np.isin(rows[f][:, 0], rows[f - 1][:, 0]).sum())
        total += len(rows[f])
    return cont, total, 1 + max(int(r[:, 0].max()) for r in rows if len(r))


# ------------------------------------------------------------------------------------------------ refusals
def refusal_cases():
    """(keyword overrides, a word of the message): everything region_links refuses, then the compensated op's own refusals."""
    own = [(dict(mv=None), b"null"), (dict(frame_h=15), b"frame"), (dict(frame_w=0), b"frame"), (dict(frame_h=46341, frame_w=46341), b"2^31"),
           (dict(H=16 * 31 + 1, frame_h=16), b"31"), (dict(W=16 * 31 + 1, frame_w=16), b"31")]
    return [(kw, word) for op, kw, word in ref.refusal_cases() if op == "region_links"] + own


def call_links_mc(lib, **kw):
    """fs_region_links_mc through the hook table with every argument a keyword; pointers default to a fake non-null address."""
    fake = 0x1000
    a = dict(index=fake, table=fake, counts=fake, prev_index=fake, prev_table=fake, prev_counts=fake, mv=fake, pair_stats=fake, back=fake, fwd=fake,
             link_counts=fake, workspace=fake, n=2, H=8, W=8, frame_h=16, frame_w=16, max_regions=16, max_pairs=64, min_overlap=1, workspace_offset=0)
    a.update(kw)
    work = None if a["workspace"] is None else a["workspace"] + a["workspace_offset"]
    return lib.fs_region_links_mc(a["index"], a["table"], a["counts"], a["prev_index"], a["prev_table"], a["prev_counts"], a["mv"], a["pair_stats"], a["n"],
                                  a["H"], a["W"], a["frame_h"], a["frame_w"], a["max_regions"], a["max_pairs"], a["min_overlap"], a["back"], a["fwd"],
                                  a["link_counts"], work, None)
