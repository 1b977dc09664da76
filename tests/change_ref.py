"""CPU restatement of the change map between two registered mosaics (include/floodseg_test.h: mosaic_change; the same rules as
csrc/change_defs.h) for the tests: plain numpy, on top of merge_ref's gather and link tests and mosaic_ref's resolve.
The op appears vectorised (what the GPU tests compare with, bit for bit) and as literal loops over Python integers (the definition
read aloud).  Everything is integer.  A test helper, not an oracle module."""
import functools

import numpy as np

import merge_ref as gref
import mosaic_ref as mref
import ortho_ref as oref
import refine_ref as rref

ONE = mref.ONE
NONE = 255
NOT_COMPARABLE, SAME, EXPLAINED, CHANGED, GAINED, LOST = range(6)
# (R, G, B, A) per code, flow.predict.CHANGE_PALETTE's values: the tests compare the two tables
PALETTE = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [255, 255, 0, 96], [255, 0, 255, 176], [0, 64, 255, 208], [255, 128, 0, 208]], np.uint8)


def class_set(classes):
    bits = 0
    for c in classes:
        bits |= 1 << int(c)
    return bits


# ------------------------------------------------------------------------------------------------ the decided class
def decided(votes, min_votes=1, min_conf=0):
    """uint16 [K, CH, CW] -> uint8 [CH, CW]: mosaic_resolve's winner where the total reaches min_votes and its share min_conf, else 255."""
    cls, conf, seen, _ = mref.mosaic_resolve(votes)
    return np.where((seen.astype(np.int64) >= min_votes) & (conf.astype(np.int64) >= min_conf), cls, NONE).astype(np.uint8)


def decided_pixel(v, min_votes, min_conf):
    """The K counts of one pixel, Python integers -> its decided class."""
    total, most = sum(v), max(v)
    if total < min_votes or (255 * most + total // 2) // total < min_conf:      # min_votes >= 1: no division by zero
        return NONE
    return v.index(most)


# ------------------------------------------------------------------------------------------------ the op, vectorised
def class_planes(votes_a, origin_a, votes_b, origin_b, link, min_votes=1, min_conf=0):
    """-> (cls_a, cls_b uint8 [CH_a, CW_a], exists bool: the A pixels whose B pixel exists; all False under a link that does not merge)."""
    _, ch, cw = votes_a.shape
    cls_a, cls_b, exists = decided(votes_a, min_votes, min_conf), np.full((ch, cw), NONE, np.uint8), np.zeros((ch, cw), bool)
    if gref.link_merges(link):
        bx, by, exists = gref.b_pixels(link, (0, 0, ch, cw), origin_a, votes_b.shape[1:], origin_b)
        Y, X = np.nonzero(exists)
        cls_b[Y, X] = decided(votes_b, min_votes, min_conf)[by[Y, X], bx[Y, X]]
    return cls_a, cls_b, exists


def window_sets(cls, r):
    """uint8 [CH, CW] -> int64 [CH, CW]: the OR of 1 << cls over the window of radius r clipped at the canvas edge, 255 counting for nothing."""
    bits = np.where(cls != NONE, np.int64(1) << np.minimum(cls, 31).astype(np.int64), 0)
    pad = np.pad(bits, r)
    ch, cw = cls.shape
    out = np.zeros_like(bits)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + ch, dx:dx + cw]
    return out


def change_codes(cls_a, cls_b, r, watch_set):
    """The two class planes -> the change plane uint8."""
    ca, cb = cls_a.astype(np.int64), cls_b.astype(np.int64)
    comparable = (cls_a != NONE) & (cls_b != NONE)
    ka, kb = np.where(comparable, ca, 0), np.where(comparable, cb, 0)
    explained = (((window_sets(cls_b, r) >> ka) & 1) != 0) & (((window_sets(cls_a, r) >> kb) & 1) != 0)
    wa, wb = ((watch_set >> ka) & 1) != 0, ((watch_set >> kb) & 1) != 0
    code = np.where(wa == wb, CHANGED, np.where(wb, GAINED, LOST))
    code = np.where(explained, EXPLAINED, code)
    code = np.where(ca == cb, SAME, code)
    return np.where(comparable, code, NOT_COMPARABLE).astype(np.uint8)


def tallies(change, cls_a, cls_b, exists, k, status):
    """-> (transitions int64 [2, K, K], counts int64 [8])."""
    transitions = np.zeros((2, k, k), np.int64)
    for level, mask in enumerate((change >= SAME, change >= CHANGED)):
        np.add.at(transitions[level], (cls_a[mask].astype(np.int64), cls_b[mask].astype(np.int64)), 1)
    counts = [int(status), int(exists.sum()), int((change >= SAME).sum())] + [int((change == c).sum()) for c in range(SAME, LOST + 1)]
    return transitions, np.array(counts, np.int64)


def mosaic_change(votes_a, origin_a, votes_b, origin_b, link, min_votes=1, min_conf=0, tolerance=1, watch=(1,)):
    """Vectorised -> (change, cls_a, cls_b, transitions, counts); the inputs are only read."""
    assert 1 <= min_votes <= 65535 and 0 <= min_conf <= 255 and 0 <= tolerance <= 8 and class_set(watch) >> votes_a.shape[0] == 0
    cls_a, cls_b, exists = class_planes(votes_a, origin_a, votes_b, origin_b, link, min_votes, min_conf)
    change = change_codes(cls_a, cls_b, tolerance, class_set(watch))
    return (change, cls_a, cls_b) + tallies(change, cls_a, cls_b, exists, votes_a.shape[0], link[12])


# ------------------------------------------------------------------------------------------------ the op, read aloud
def mosaic_change_loop(votes_a, origin_a, votes_b, origin_b, link, min_votes=1, min_conf=0, tolerance=1, watch=(1,)):
    """The definition literally."""
    (k_max, ch, cw), (_, ch_b, cw_b), r, watch_set = votes_a.shape, votes_b.shape, tolerance, class_set(watch)
    merges = gref.link_merges(link)
    m = [int(v) for v in link[6:12]]
    cls_a, cls_b = np.full((ch, cw), NONE, np.uint8), np.full((ch, cw), NONE, np.uint8)
    change, transitions, counts = np.zeros((ch, cw), np.uint8), np.zeros((2, k_max, k_max), np.int64), [int(link[12]), 0, 0, 0, 0, 0, 0, 0]
    for Y in range(ch):
        for X in range(cw):
            cls_a[Y, X] = decided_pixel([int(votes_a[k, Y, X]) for k in range(k_max)], min_votes, min_conf)
            if not merges:
                continue
            bx, by = gref.b_pixel(m, X, Y, origin_a, origin_b)
            if 0 <= bx < cw_b and 0 <= by < ch_b:
                counts[1] += 1
                cls_b[Y, X] = decided_pixel([int(votes_b[k, by, bx]) for k in range(k_max)], min_votes, min_conf)
    for Y in range(ch):
        for X in range(cw):
            ca, cb = int(cls_a[Y, X]), int(cls_b[Y, X])
            if ca == NONE or cb == NONE:
                continue
            win_a = win_b = 0
            for y in range(max(0, Y - r), min(ch, Y + r + 1)):
                for x in range(max(0, X - r), min(cw, X + r + 1)):
                    win_a |= 0 if cls_a[y, x] == NONE else 1 << int(cls_a[y, x])
                    win_b |= 0 if cls_b[y, x] == NONE else 1 << int(cls_b[y, x])
            if ca == cb:
                code = SAME
            elif (win_b >> ca) & 1 and (win_a >> cb) & 1:
                code = EXPLAINED
            elif ((watch_set >> ca) & 1) == ((watch_set >> cb) & 1):
                code = CHANGED
            else:
                code = GAINED if (watch_set >> cb) & 1 else LOST
            change[Y, X] = code
            counts[2] += 1
            counts[2 + code] += 1
            transitions[0, ca, cb] += 1
            transitions[1, ca, cb] += int(code >= CHANGED)
    return change, cls_a, cls_b, transitions, np.array(counts, np.int64)


# ------------------------------------------------------------------------------------------------ the cases of the op tests
VIEW_A, VIEW_B, SMALL, VIEW_ORIGIN_A, VIEW_ORIGIN_B = gref.VIEW_A, (70, 130), (17, 65), gref.VIEW_ORIGIN_A, gref.VIEW_ORIGIN_B
THRESHOLDS = ((1, 0), (3, 170))        # (min_votes, min_conf): everything decided; the special pixels of change_votes at and below the bar


def block_classes(size, k=5, shift=(0, 0)):
    """A class plane of blocks, 12 rows by 20 columns each, in at most five ids spread over 0..k - 1 (k = 32: 0, 8, 16, 23, 31); shift =
    (dx, dy) moves the pattern (content at (x, y) comes from (x - dx, y - dy) of the unshifted one, which is defined everywhere)."""
    Y, X = np.meshgrid(np.arange(size[0]) - shift[1], np.arange(size[1]) - shift[0], indexing="ij")
    ids = np.round(np.linspace(0, k - 1, min(k, 5))).astype(np.uint8)
    return ids[(3 * (Y // 12) + 2 * (X // 20)) % len(ids)]


@functools.lru_cache(maxsize=None)
def change_votes(k, size, seed):
    """uint16 [k, CH, CW]: a block pattern's class wins most pixels by a random margin; sprinkled over it pixels without a vote (and
    one rectangular hole), cells at 65535 (with k > 1 two of them: a tie at the top), exact ties (the lowest id wins), totals of exactly
    3 and of 2 (at and below min_votes = 3), and winners' shares of exactly 170/255 (2 of 3 votes) and 169/255 (53 of 80)."""
    rng = np.random.RandomState(seed + 7 * k)
    ch, cw = size
    first = block_classes(size, k, (seed % 5, seed % 3)).astype(np.int64)
    second = (first + 1 + rng.randint(0, max(k - 1, 1), size=size)) % k      # another class when k > 1
    votes = (rng.randint(0, 4, size=(k, ch, cw)) * (rng.rand(k, ch, cw) < 3.0 / max(k, 3))).astype(np.int64)    # a few stray votes, whatever k is
    Y, X = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
    votes[first, Y, X] = rng.randint(8, 40, size=size)
    kind = rng.randint(0, 100, size=size)

    def put(mask, a, b):
        y, x = np.nonzero(mask)
        votes[:, y, x] = 0
        votes[first[y, x], y, x] = a
        if k > 1:
            votes[second[y, x], y, x] = b

    put(kind < 8, 0, 0)
    put((kind >= 8) & (kind < 11), 65535, 65535)
    put((kind >= 11) & (kind < 16), 9, 9)
    put((kind >= 16) & (kind < 20), 3, 0)
    put((kind >= 20) & (kind < 24), 2, 0)
    put((kind >= 24) & (kind < 28), 2, 1)
    put((kind >= 28) & (kind < 32), 53, 27)
    votes[:, ch // 3:ch // 3 + 9, cw // 4:cw // 4 + 21] = 0
    out = votes.astype(np.uint16)
    out.setflags(write=False)
    return out


def op_cases():
    """(name, K, size A, size B, tolerance, thresholds, watch) of the op tests: every K with every tolerance at the family's view
    canvases, the small canvas on either side, the watch sets."""
    cases = []
    for k in (1, 5, 32):
        for r in (0, 1, 3, 8):
            cases.append((f"K{k} r{r}", k, VIEW_A, VIEW_B, r, THRESHOLDS[(k + r) % 2], (k - 1,)))
    cases.append(("small A", 5, SMALL, VIEW_B, 8, THRESHOLDS[1], (1,)))
    cases.append(("small B", 5, VIEW_B, SMALL, 3, THRESHOLDS[0], (1, 2)))
    cases.append(("no watch", 5, VIEW_A, VIEW_B, 1, THRESHOLDS[1], ()))
    cases.append(("all watched", 5, VIEW_A, VIEW_B, 1, THRESHOLDS[1], (0, 1, 2, 3, 4)))
    return cases


def case_inputs(k, size_a, size_b):
    return change_votes(k, tuple(size_a), 3), change_votes(k, tuple(size_b), 11)


def change_links():
    """merge_ref.view_links() with the status a comparison needs: (name, link, does it merge)."""
    out = []
    for name, link in gref.view_links():
        link = link.copy()
        merges = name in ("identity", "shift", "rotation and zoom", "outside")
        if merges:
            link[12] = gref.REGISTERED
        out.append((name, link, merges))
    initial = gref.view_links()[1][1].copy()
    initial[12] = gref.INITIAL
    return out + [("initial", initial, False)]


# ------------------------------------------------------------------------------------------------ two flights over the same ground
FLIGHT_CLASSES, PAINT_CLASS = 4, 1
OFFSETS_A, OFFSETS_B = (0, 4, 8, 12, 16, 20), (12, 16, 20, 24, 28)
PAINT = (54, 126, 61, 141)                   # (y0, x0, y1, x1) in ground coordinates: 7 x 15 pixels of new water, 6 pixels inside a block of class 0


@functools.lru_cache(maxsize=None)
def ground_classes():
    """The class of every pixel of refine_ref.ground(): blocks of 24 rows by 40 columns, four classes."""
    Y, X = np.meshgrid(np.arange(128), np.arange(256), indexing="ij")
    g = ((Y // 24 + 2 * (X // 40)) % FLIGHT_CLASSES).astype(np.uint8)
    g.setflags(write=False)
    return g


def painted_ground():
    g = ground_classes().copy()
    y0, x0, y1, x1 = PAINT
    g[y0:y1, x0:x1] = PAINT_CLASS
    return g


@functools.lru_cache(maxsize=None)
def two_flights(mode="centre"):
    """merge_ref's synthetic whole-pixel pan flown twice over refine_ref.ground(): flight A from offset 0, flight B from offset 12 (a chain
    of its own: its anchor lies 12 px to the right) with PAINT painted into its masks.  Both mosaicked with orthophotos.
    -> (a, b, the exact link: status 0, the painted block in A's canvas as (y0, x0, y1, x1))."""
    (h, w), parts = rref.FLIGHT_SIZE, []
    for offsets, g in ((OFFSETS_A, ground_classes()), (OFFSETS_B, painted_ground())):
        images, tables, _ = rref.flight(list(offsets), bias=(0, 0))
        masks = [np.ascontiguousarray(g[32:32 + h, 64 + x:64 + x + w]) for x in offsets]
        parts.append(gref.run_part(images, masks, tables, mode, classes=FLIGHT_CLASSES))
    shift = OFFSETS_B[0] - OFFSETS_A[0]
    exact = gref.link_row([ONE, 0, shift * ONE, 0, ONE, 0], [ONE, 0, -shift * ONE, 0, ONE, 0], status=gref.REGISTERED)
    oy, ox = gref.SPLIT_ORIGIN                 # A's anchor frame starts at ground (32, 64 + OFFSETS_A[0])
    y0, x0, y1, x1 = PAINT
    block = (y0 - 32 + oy, x0 - 64 - OFFSETS_A[0] + ox, y1 - 32 + oy, x1 - 64 - OFFSETS_A[0] + ox)
    return parts[0], parts[1], exact, block


def off_link(dx, dy=0, status=gref.INITIAL):
    """The exact link of two_flights() moved by (dx, dy) pixels."""
    tx = (OFFSETS_B[0] - OFFSETS_A[0] + dx) * ONE
    return gref.link_row([ONE, 0, tx, 0, ONE, dy * ONE], [ONE, 0, -tx, 0, ONE, -dy * ONE], status=status)


def flights_change(a, b, link, register=True, **options):
    """What flow.predict.mosaic_change enqueues, on the reference: -> (the result tuple of mosaic_change, link, outs or None)."""
    link, outs = np.array(link, np.int64), None
    if register:
        reg = {k: options.pop(k) for k in list(options) if k in gref.REGISTER_DEFAULTS or k in ("window", "place")}
        link, outs, _ = gref.register_mosaics((a["rgba"], gref.SPLIT_ORIGIN), (b["rgba"], gref.SPLIT_ORIGIN), link, **reg)
    return mosaic_change(a["votes"], gref.SPLIT_ORIGIN, b["votes"], gref.SPLIT_ORIGIN, link, **options), link, outs


def change_csv_lines(transitions, counts):
    """flow.predict.write_change_csv's file, line by line."""
    lines = ["from,to,comparable,changed"]
    k = transitions.shape[1]
    lines += [f"{ca},{cb},{int(transitions[0, ca, cb])},{int(transitions[1, ca, cb])}" for ca in range(k) for cb in range(k) if transitions[0, ca, cb]]
    status = ("registered", "initial", "no_fit", "out_of_bounds")[int(counts[0])]
    return lines + ["", "link,reached,comparable,same,explained,changed,gained,lost", ",".join([status] + [str(int(v)) for v in counts[1:]]), ""]


def change_picture(change, rgba):
    return oref.ortho_compose(rgba, change, PALETTE)


# ------------------------------------------------------------------------------------------------ the library's refusals
def good_arguments():
    """The arguments of a call that passes validation (dummy non-null pointers, far enough apart not to overlap), in the ABI's order."""
    mb = 1 << 24
    return dict(votes_a=1 * mb, CH_a=200, CW_a=300, ox_a=36, oy_a=54, votes_b=2 * mb, CH_b=100, CW_b=150, ox_b=3, oy_b=5, K=5, link=3 * mb, min_votes=2, min_conf=128,
                tolerance=3, watch_set=0b10010, change=4 * mb, cls_a=5 * mb, cls_b=6 * mb, transitions=7 * mb, counts=8 * mb, stream=None)


def refusal_cases():
    """(changed arguments, a word of the message)."""
    mb = 1 << 24
    cases = [({p: None}, b"null") for p in ("votes_a", "votes_b", "link", "change", "cls_a", "cls_b", "transitions", "counts")]
    cases += [(dict(K=0), b"classes=0"), (dict(K=33), b"classes=33"), (dict(CH_a=0), b"canvas A"), (dict(CW_a=16385), b"16385"), (dict(CH_b=0), b"canvas B"),
              (dict(CW_b=16385), b"canvas B"), (dict(ox_a=16385), b"origin A"), (dict(oy_a=-16385), b"origin A"), (dict(ox_b=-16385), b"origin B"),
              (dict(oy_b=16385), b"origin B"), (dict(min_votes=0), b"min_votes"), (dict(min_votes=65536), b"65536"), (dict(min_conf=-1), b"min_conf"),
              (dict(min_conf=256), b"256"), (dict(tolerance=-1), b"tolerance"), (dict(tolerance=9), b"got 9"), (dict(watch_set=1 << 5), b"watch_set=0x20"),
              (dict(watch_set=1 << 31), b"watch_set"), (dict(K=1, watch_set=2), b"watch_set=0x2"), (dict(votes_b=1 * mb), b"same memory"),
              (dict(change=1 * mb), b"overlaps"), (dict(cls_a=1 * mb + 2 * 5 * 200 * 300 - 1), b"overlaps"), (dict(cls_b=2 * mb + 64), b"overlaps"),
              (dict(transitions=3 * mb + 64), b"overlaps"), (dict(counts=3 * mb - 56), b"overlaps"), (dict(votes_a=1 * mb + 1), b"aligned to 2"),
              (dict(votes_b=2 * mb + 1), b"aligned to 2"), (dict(link=3 * mb + 4), b"aligned to 8"), (dict(counts=8 * mb + 4), b"aligned to 8"),
              (dict(transitions=7 * mb + 4), b"aligned to 8")]
    return cases


def call_op(lib, **changed):
    args = dict(good_arguments())
    args.update(changed)
    return lib.fs_mosaic_change(*args.values())
