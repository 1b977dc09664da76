"""The definition of the region tracking ops (include/floodseg_test.h: region_links, region_tracks) in plain numpy, and
the cases the CPU and the GPU tests share.  Inputs are built with regions_ref (mask_regions, region_table); nothing of the package's
ops is imported here.  R = max_regions.

  overlap(a, b)  pixels p with index[f-1][p] == a and index[f][p] == b, both rows (a < counts[f-1][1], b < counts[f][1]) of the same
                 class (table column 0); compared in place; background and regions past the cap (-1) take no part
  back[f][b]     (a, overlap) for the a with the largest overlap with b, lowest a on a tie; (-1, 0) below min_overlap (>= 1)
  fwd[f][a]      the same from the other side, indexed by the rows of frame f-1
  overflow       more than max_pairs distinct (a, b) with overlap >= 1: back / fwd (-1, 0) throughout, link_counts (max_pairs, 1)
  continue       b continues a exactly when back[f][b].row == a >= 0, fwd[f][a].row == b and a has a track: a's id and a's parent
  born           every other region with a row: ids next_id, next_id + 1, ... in row order; parent = the track of back[f][b].row or -1
  tracks         int64 [n][R][4] = (track id, parent id, back row, back overlap); rows at and behind counts[f][1]: (-1, -1, -1, 0)
"""
import functools

import numpy as np

import regions_ref as rref

CONN = 8
BG = 9  # a background id of the hand-made frames (>= K)
GEOMETRIES = [(1, 1, 1), (3, 17, 33), (4, 9, 300), (3, 70, 150)]  # (4, 9, 300): a 256-pixel piece border, runs across wave borders
SHIFTS = [(0, 0), (1, 2), (5, -7)]                               # pixels per frame (dy, dx)
BASE_CASE = 4                                                     # regions_ref's (2, 70, 150): the plane the patterns are cut from


def default_max_pairs(cap):
    return max(16, 1 << (4 * cap - 1).bit_length())


# ------------------------------------------------------------------------------------------------ the definition
def region_links(index, table, counts, prev=None, max_pairs=None, min_overlap=1, want_pairs=False):
    """-> back int32 [n,R,2], fwd int32 [n,R,2], link_counts int64 [n,2] (and, want_pairs, the distinct pairs of every frame pair).
    Overlaps from a dense R x R matrix filled by np.add.at."""
    n, h, w = index.shape
    cap = table.shape[1]
    max_pairs = default_max_pairs(cap) if max_pairs is None else max_pairs
    assert 16 <= max_pairs <= 2 ** 20 and max_pairs & (max_pairs - 1) == 0 and min_overlap >= 1
    none = np.array([-1, 0], np.int32)
    back, fwd = np.tile(none, (n, cap, 1)), np.tile(none, (n, cap, 1))
    link_counts = np.zeros((n, 2), np.int64)
    pairs = np.zeros(n, np.int64)
    for f in range(n):
        if f == 0 and prev is None:
            continue
        ia, ta, ca = (index[f - 1], table[f - 1], counts[f - 1]) if f else prev
        a, b = ia.reshape(-1).astype(np.int64), index[f].reshape(-1).astype(np.int64)
        ok = (a >= 0) & (a < min(cap, ca[1])) & (b >= 0) & (b < min(cap, counts[f][1]))
        a, b = a[ok], b[ok]
        same = ta[a, 0] == table[f][b, 0]
        m = np.zeros((cap, cap), np.int64)
        np.add.at(m, (a[same], b[same]), 1)
        pairs[f] = np.count_nonzero(m)
        if pairs[f] > max_pairs:
            link_counts[f] = (max_pairs, 1)
            continue
        link_counts[f] = (pairs[f], 0)
        best_a, best_b = m.argmax(0), m.argmax(1)                 # the first maximum: the lowest row on a tie
        for r in range(cap):
            if m[best_a[r], r] >= min_overlap:
                back[f, r] = (best_a[r], m[best_a[r], r])
            if m[r, best_b[r]] >= min_overlap:
                fwd[f, r] = (best_b[r], m[r, best_b[r]])
    return (back, fwd, link_counts, pairs) if want_pairs else (back, fwd, link_counts)


def region_links_bruteforce(index, table, counts, prev=None, max_pairs=None, min_overlap=1):
    """The same by a loop over the pixels and a dictionary of pairs (slow: the cross-check of the small cases)."""
    n, h, w = index.shape
    cap = table.shape[1]
    max_pairs = default_max_pairs(cap) if max_pairs is None else max_pairs
    back, fwd = np.zeros((n, cap, 2), np.int32), np.zeros((n, cap, 2), np.int32)
    back[..., 0] = fwd[..., 0] = -1
    link_counts = np.zeros((n, 2), np.int64)
    for f in range(n):
        if f == 0 and prev is None:
            continue
        ia, ta, ca = (index[f - 1], table[f - 1], counts[f - 1]) if f else prev
        seen = {}
        for y in range(h):
            for x in range(w):
                a, b = int(ia[y, x]), int(index[f, y, x])
                if 0 <= a < min(cap, ca[1]) and 0 <= b < min(cap, counts[f][1]) and ta[a, 0] == table[f][b, 0]:
                    seen[(a, b)] = seen.get((a, b), 0) + 1
        if len(seen) > max_pairs:
            link_counts[f] = (max_pairs, 1)
            continue
        link_counts[f] = (len(seen), 0)
        for (a, b), c in sorted(seen.items()):                     # ascending (a, b): a later pair needs a strictly larger overlap
            if c >= min_overlap and c > back[f, b, 1]:
                back[f, b] = (a, c)
            if c >= min_overlap and c > fwd[f, a, 1]:
                fwd[f, a] = (b, c)
    return back, fwd, link_counts


def region_tracks(back, fwd, counts, state, prev_tracks=None):
    """-> tracks int64 [n,R,4], the new state int64 [2]."""
    n, cap, _ = back.shape
    tracks = np.zeros((n, cap, 4), np.int64)
    tracks[..., :3] = -1
    next_id = int(state[0])
    for f in range(n):
        pt = tracks[f - 1] if f else prev_tracks
        for b in range(int(min(cap, max(0, counts[f][1])))):
            a, ov = int(back[f, b, 0]), int(back[f, b, 1])
            if not 0 <= a < cap:
                a, ov = -1, 0
            pid, ppar = (int(pt[a, 0]), int(pt[a, 1])) if a >= 0 and pt is not None else (-1, -1)
            if a >= 0 and fwd[f, a, 0] == b and pid >= 0:
                tracks[f, b] = (pid, ppar, a, ov)
            else:
                tracks[f, b] = (next_id, pid, a, ov)
                next_id += 1
    return tracks, np.array([next_id, state[1]], np.int64)


# ------------------------------------------------------------------------------------------------ the cases
def _pattern_frames(geometry, pattern, shift):
    """n frames cut from a plane of the pattern that moves by `shift` pixels from frame to frame (the plane wraps around)."""
    n, h, w = geometry
    base = rref.make_mask(BASE_CASE, pattern)[0]
    plane = np.tile(base, (-(-(h + 16) // base.shape[0]), -(-(w + 16) // base.shape[1])))
    return np.stack([np.roll(plane, (f * shift[0], f * shift[1]), (0, 1))[:h, :w] for f in range(n)]).astype(np.uint8)


def _hand_made():
    """One pair of frames per event; K = 5, everything else background."""
    def frames(*planes, hw=(6, 12)):
        out = np.full((len(planes),) + hw, BG, np.uint8)
        for f, boxes in enumerate(planes):
            for cls, y0, y1, x0, x1 in boxes:
                out[f, y0:y1, x0:x1] = cls
        return out

    bar, pieces = [(1, 2, 3, 0, 11)], [(1, 2, 3, 0, 6), (1, 2, 3, 7, 11)]   # 11 pixels; 6 and 4 of them with a gap at x = 6
    stripes = np.zeros((2, 16, 16), np.uint8)
    stripes[0] = (np.arange(16)[:, None] // 2 % 2)                           # eight horizontal stripes of classes 0, 1, 0, 1, ...
    stripes[1] = (np.arange(16)[None, :] // 2 % 2)                           # eight vertical ones likewise: 2 * 4 * 4 same-class pairs
    return [
        dict(name="continue", mask=frames([(1, 1, 4, 1, 5)], [(1, 1, 4, 2, 6)])),
        dict(name="split", mask=frames(bar, pieces)),
        dict(name="merge", mask=frames(pieces, bar)),
        dict(name="born", mask=frames([(1, 0, 2, 0, 2)], [(1, 0, 2, 0, 2), (2, 4, 6, 8, 12)])),
        dict(name="tie", mask=frames([(1, 0, 1, 0, 4), (1, 2, 3, 0, 4)], [(1, 0, 3, 0, 1), (1, 0, 3, 2, 3)])),
        dict(name="class", mask=frames([(1, 1, 4, 1, 5)], [(2, 1, 4, 1, 5)])),
        dict(name="min_overlap", mask=frames([(1, 1, 4, 1, 5)], [(1, 1, 4, 2, 6)]), min_overlap=10),
        dict(name="cap", mask=frames([(1, 0, 1, 0, 2), (2, 0, 1, 4, 6), (3, 2, 3, 0, 2), (4, 2, 3, 4, 6)],
                                     [(1, 0, 1, 0, 2), (2, 0, 1, 4, 6), (3, 2, 3, 0, 2), (4, 2, 3, 4, 6)]), cap=2),
        dict(name="pairs_full", mask=stripes, classes=2, cap=16, max_pairs=32),
        dict(name="pairs_overflow", mask=stripes, classes=2, cap=16, max_pairs=16),
    ]


@functools.lru_cache(maxsize=None)
def case_list():
    cases = []
    for g, geometry in enumerate(GEOMETRIES):
        for pattern in rref.PATTERNS:
            for shift in SHIFTS:
                n, h, w = geometry
                cases.append(dict(name=f"{geometry} {pattern} {shift}", group=g, mask=_pattern_frames(geometry, pattern, shift),
                                  classes=rref.pattern_classes(pattern), cap=min(h * w + 1, 1024)))
    for c in _hand_made():
        c.setdefault("classes", 5)
        c.setdefault("cap", 16)
        c["group"] = len(GEOMETRIES)
        cases.append(c)
    for c in cases:
        c.setdefault("max_pairs", default_max_pairs(c["cap"]))
        c.setdefault("min_overlap", 1)
        c["mask"].setflags(write=False)
    return cases


GROUPS = len(GEOMETRIES) + 1  # the cases of each geometry, then the hand-made ones


def cases_of(group):
    return [i for i, c in enumerate(case_list()) if c["group"] == group]


def case_by_name(name):
    return next(i for i, c in enumerate(case_list()) if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(i):
    """Everything the tests compare against for one case, computed once: the region tables of its frames, then links and tracks of the
    whole clip in one call (no frame before frame 0, ids from 0)."""
    c = case_list()[i]
    mask, k, cap = c["mask"], c["classes"], c["cap"]
    table, counts, index = rref.region_table(mask, rref.mask_regions(mask, k, CONN), k, None, 128, cap)
    back, fwd, link_counts, pairs = region_links(index, table, counts, None, c["max_pairs"], c["min_overlap"], want_pairs=True)
    tracks, state = region_tracks(back, fwd, counts, np.zeros(2, np.int64), None)
    out = dict(c, table=table, counts=counts, index=index, back=back, fwd=fwd, link_counts=link_counts, pairs=pairs, tracks=tracks, state=state)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def chained(e, pieces):
    """The clip of expected() `e` in calls of the given lengths, each handed the last frame of the one before as prev: what one call gives."""
    backs, fwds, lcs, trs = [], [], [], []
    state, prev, prev_tracks, at = np.zeros(2, np.int64), None, None, 0
    for n in pieces:
        s = slice(at, at + n)
        back, fwd, lc = region_links(e["index"][s], e["table"][s], e["counts"][s], prev, e["max_pairs"], e["min_overlap"])
        tracks, state = region_tracks(back, fwd, e["counts"][s], state, prev_tracks)
        backs.append(back), fwds.append(fwd), lcs.append(lc), trs.append(tracks)
        at += n
        prev, prev_tracks = (e["index"][at - 1], e["table"][at - 1], e["counts"][at - 1]), tracks[-1]
    return np.concatenate(backs), np.concatenate(fwds), np.concatenate(lcs), np.concatenate(trs), state


@functools.lru_cache(maxsize=None)
def five_frames():
    """A clip of five frames (17 x 33, random ids moving by (1, 2)) for the chaining tests: n = 5 against 1 + 1 + 1 + 1 + 1 and 2 + 3."""
    mask = _pattern_frames((5, 17, 33), "random5", (1, 2))
    k, cap = 5, 17 * 33 + 1
    table, counts, index = rref.region_table(mask, rref.mask_regions(mask, k, CONN), k, None, 128, cap)
    e = dict(mask=mask, classes=k, cap=cap, max_pairs=default_max_pairs(cap), min_overlap=1, table=table, counts=counts, index=index)
    e["back"], e["fwd"], e["link_counts"] = region_links(index, table, counts, None, e["max_pairs"], 1)
    e["tracks"], e["state"] = region_tracks(e["back"], e["fwd"], counts, np.zeros(2, np.int64), None)
    return e


def clip_tracks(masks, classes, conn, cap, max_pairs=None, min_overlap=1, resets=()):
    """What FlowPredictor(track=True) keeps for a sequence of emitted masks: per frame the tracks rows [rows, 4], and the overflow flags.
    `resets`: frame numbers in front of which reset() was called (those frames' regions are all born)."""
    table, counts, index = rref.region_table(masks, rref.mask_regions(masks, classes, conn), classes, None, 128, cap)
    rows, flags = [], []
    state, prev, prev_tracks = np.zeros(2, np.int64), None, None
    for f in range(len(masks)):
        if f in resets:
            prev, prev_tracks = None, None
        s = slice(f, f + 1)
        back, fwd, lc = region_links(index[s], table[s], counts[s], prev, max_pairs, min_overlap)
        tracks, state = region_tracks(back, fwd, counts[s], state, prev_tracks)
        rows.append(tracks[0, :counts[f, 1]])
        flags.append(int(lc[0, 1]))
        prev, prev_tracks = (index[f], table[f], counts[f]), tracks[0]
    return rows, np.array(flags, np.int64)


# ------------------------------------------------------------------------------------------------ refusals
def refusal_cases():
    """(op, keyword overrides, a word of the message): every refusal the header lists, with fake non-null pointers."""
    sizes = [(dict(n=0), b"frames"), (dict(n=65536), b"65535"), (dict(max_regions=0), b"max_regions"), (dict(max_regions=65537), b"max_regions")]
    links = sizes + [(dict(H=0), b">= 1"), (dict(W=-1), b">= 1"), (dict(H=46341, W=46341), b"2^31"), (dict(H=1, W=2 ** 31 - 1), b"2^31"),
                     (dict(max_pairs=8), b"max_pairs"), (dict(max_pairs=48), b"max_pairs"), (dict(max_pairs=2 ** 21), b"max_pairs"),
                     (dict(max_pairs=0), b"max_pairs"), (dict(min_overlap=0), b"min_overlap"), (dict(prev_index=None), b"in part"),
                     (dict(prev_table=None, prev_counts=None), b"in part"), (dict(workspace_offset=4), b"aligned")]
    links += [(dict(**{name: None}), b"null") for name in ("index", "table", "counts", "back", "fwd", "link_counts", "workspace")]
    tracks = sizes + [(dict(**{name: None}), b"null") for name in ("back", "fwd", "counts", "state", "tracks")]
    return [("region_links", kw, word) for kw, word in links] + [("region_tracks", kw, word) for kw, word in tracks]


def call_track_op(lib, op, **kw):
    """fs_<op> through the hook table with every argument a keyword; pointers default to a fake non-null address."""
    fake = 0x1000
    a = dict(index=fake, table=fake, counts=fake, prev_index=fake, prev_table=fake, prev_counts=fake, back=fake, fwd=fake, link_counts=fake,
             workspace=fake, prev_tracks=fake, state=fake, tracks=fake, n=2, H=8, W=8, max_regions=16, max_pairs=64, min_overlap=1, workspace_offset=0)
    a.update(kw)
    if op == "region_links":
        work = None if a["workspace"] is None else a["workspace"] + a["workspace_offset"]
        return lib.fs_region_links(a["index"], a["table"], a["counts"], a["prev_index"], a["prev_table"], a["prev_counts"], a["n"], a["H"], a["W"],
                                   a["max_regions"], a["max_pairs"], a["min_overlap"], a["back"], a["fwd"], a["link_counts"], work, None)
    return lib.fs_region_tracks(a["back"], a["fwd"], a["counts"], a["prev_tracks"], a["n"], a["max_regions"], a["state"], a["tracks"], None)
