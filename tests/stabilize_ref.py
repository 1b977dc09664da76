"""The definition of the temporal mask stabiliser (include/floodseg_test.h: mask_stabilize) in plain numpy, an independent
per-pixel brute force in Python ints, and the cases the CPU and the GPU tests share.  tracks_mc_ref is imported, not edited: the source
of a pixel is tracks_mc_ref.shifts', the geometries, table kinds, the blob scene and the cut stats are its own.  Everything is integer.

  state word   bit 31 valid | run r << 16 | candidate c << 8 | emitted e; 0 = no state
  prior s      0 (frame 0 without a state; a cut: pair_stats[f][2] != 0), else the state after the frame before at the pixel's source
               (mv given; 0 when the source lies outside the mask) or at the pixel itself
  update       o >= K: out = o, state 0 | s invalid: seed | o == e: c = e, r = 0 | conf >= T: switch, trusted |
               r' = r + 1 capped at 255 if o == c else 1, c = o; r' >= P: switch, else hold (out = e)
  counts[f]    (held, switched, seeded, trusted)
"""
import functools

import numpy as np

import tracks_mc_ref as mc

VALID = 1 << 31
GEOMETRIES = mc.GEOMETRIES
# H * W of all four is a multiple of 4.  The kernels give a thread four consecutive pixels of the flat plane, so these three add planes of
# 4k + 1, 4k + 2 and 4k + 3 pixels: a ragged last thread, and frames whose byte planes start at every alignment
RAGGED_GEOMETRIES = [(37, 301, 48, 320), (7, 18, 16, 32), (9, 11, 16, 16)]
RAGGED_TABLES = ["per_block", "garbage"]
TABLES = mc.TABLES
PERSISTS = (1, 2, 3, 255)
TRUST = 200
K = 5
CUT_STATS = mc.case_list()[mc.case_by_name("cut")]["pair_stats"]          # three rows, the middle one flagged as a cut


def pack(e, c, r):
    return VALID | (r << 16) | (c << 8) | e


def workspace_bytes(n, h, w, hb=0, wb=0):
    return 0 if hb * wb == 0 else (h * w + 3) // 4 * 16 + (n * (hb * wb + 1) + 3) // 4 * 16


# ------------------------------------------------------------------------------------------------ the definition, vectorised
def sources(mv_f, h, w, frame_size):
    """(flat source index int64 [h, w], inside bool [h, w]) of one frame's table."""
    sy, sx = mc.shifts(mv_f, h, w, *frame_size)
    yy, xx = np.mgrid[0:h, 0:w]
    ys, xs = yy + sy, xx + sx
    ok = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    return np.where(ok, ys * w + xs, 0), ok


def mask_stabilize(mask, state=None, conf=None, classes=K, persist=3, trust=None, mv=None, frame_size=None, pair_stats=None, _src=None):
    """-> (out uint8 [n,h,w], state uint32 [h,w], counts int64 [n,4]).  _src: the per-frame sources() of mv, when the caller has them."""
    n, h, w = mask.shape
    T = 256 if trust is None or conf is None else int(trust)
    out, counts = np.empty_like(mask), np.zeros((n, 4), np.int64)
    st = None if state is None else np.asarray(state).view(np.uint32).astype(np.int64).reshape(h, w)
    for f in range(n):
        if st is None or (pair_stats is not None and pair_stats[f][2] != 0):
            s = np.zeros((h, w), np.int64)
        elif mv is not None:
            at, ok = _src[f] if _src is not None else sources(mv[f], h, w, frame_size)
            s = np.where(ok, st.reshape(-1)[at], 0)
        else:
            s = st
        o = mask[f].astype(np.int64)
        valid, e, c, r = (s >> 31) & 1 == 1, s & 255, (s >> 8) & 255, (s >> 16) & 255
        through = o >= classes
        seeded = ~through & ~valid
        same = ~through & valid & (o == e)
        differs = ~through & valid & (o != e)
        trusted = differs & (conf[f] >= T) if conf is not None else np.zeros((h, w), bool)
        rest = differs & ~trusted
        r2 = np.where(o == c, np.minimum(r + 1, 255), 1)
        switched, held = rest & (r2 >= persist), rest & (r2 < persist)
        st = np.where(held, pack(e, o, r2), np.where(through, 0, pack(o, o, 0)))
        out[f] = np.where(held, e, o)
        counts[f] = held.sum(), (switched | trusted).sum(), seeded.sum(), trusted.sum()
        assert not (same & (seeded | differs)).any()
    return out, st.astype(np.uint32), counts


# ------------------------------------------------------------------------------------------------ the same, pixel by pixel
def mask_stabilize_bruteforce(mask, state=None, conf=None, classes=K, persist=3, trust=None, mv=None, frame_size=None, pair_stats=None):
    """A loop over frames and pixels with plain Python integers, nothing shared with the functions above."""
    n, h, w = mask.shape
    words = [0] * (h * w) if state is None else [int(v) for v in np.asarray(state).view(np.uint32).reshape(-1)]
    have = state is not None
    out, counts = np.empty_like(mask), np.zeros((n, 4), np.int64)

    def scaled(v, p, fp):
        m = (2 * abs(v) * p + fp) // (2 * fp)
        return m if v >= 0 else -m

    for f in range(n):
        cut = pair_stats is not None and int(pair_stats[f][2]) != 0
        if mv is not None:
            fh, fw = frame_size
            hb, wb = fh // 16, fw // 16
            rows = [[int(v) for v in row] for row in np.asarray(mv[f]).reshape(hb * wb, 7)]
        new = [0] * (h * w)
        held = switched = seeded = trusted = 0
        for y in range(h):
            for x in range(w):
                o = int(mask[f, y, x])
                s = 0
                if have and not cut:
                    ys, xs = y, x
                    if mv is not None:
                        by, bx = ((2 * y + 1) * fh) // (2 * h) // 16, ((2 * x + 1) * fw) // (2 * w) // 16
                        if by < hb and bx < wb:
                            q = rows[by * wb + bx]
                            if q[5] >= 0 and q[6] >= 0 and abs(q[3] - q[5]) <= 1024 and abs(q[4] - q[6]) <= 1024:
                                ys, xs = y + scaled(q[4] - q[6], h, fh), x + scaled(q[3] - q[5], w, fw)
                    if 0 <= ys < h and 0 <= xs < w:
                        s = words[ys * w + xs]
                emit = o
                if o >= classes:
                    word = 0
                elif not s >> 31:
                    word, seeded = (1 << 31) | (o << 8) | o, seeded + 1
                elif o == s & 255:
                    word = (1 << 31) | (o << 8) | o
                elif conf is not None and trust is not None and int(conf[f, y, x]) >= trust:
                    word, switched, trusted = (1 << 31) | (o << 8) | o, switched + 1, trusted + 1
                else:
                    run = min(((s >> 16) & 255) + 1, 255) if o == (s >> 8) & 255 else 1
                    if run >= persist:
                        word, switched = (1 << 31) | (o << 8) | o, switched + 1
                    else:
                        word, held, emit = (1 << 31) | (run << 16) | (o << 8) | (s & 255), held + 1, s & 255
                new[y * w + x] = word
                out[f, y, x] = emit
        counts[f] = held, switched, seeded, trusted
        words, have = new, True
    return out, np.array(words, np.uint64).astype(np.uint32).reshape(h, w), counts


# ------------------------------------------------------------------------------------------------ cases
def flicker_frames(n, h, w, seed):
    """A scene whose classes persist: 6 x 6 patches of classes 0..4 drifting one pixel a frame, 12 % of the pixels re-drawn per frame (a
    third of those keep their new class for the frame after as well), and a sprinkle of ids that are no class (7 and 255)."""
    rng = np.random.default_rng(seed)
    base = np.kron(rng.integers(0, K, (h // 6 + 3, w // 6 + 3)), np.ones((6, 6), np.int64))
    m = np.empty((n, h, w), np.uint8)
    keep = np.zeros((h, w), bool)
    noise = np.zeros((h, w), np.int64)
    for f in range(n):
        frame = base[f:f + h, (f // 2):(f // 2) + w].copy()
        frame[keep] = noise[keep]
        flip = rng.random((h, w)) < 0.12
        noise = np.where(flip, rng.integers(0, K, (h, w)), noise)
        frame[flip] = noise[flip]
        keep = flip & (rng.random((h, w)) < 0.34)
        other = rng.random((h, w)) < 0.01
        frame[other] = rng.choice([7, 255], (h, w))[other]
        m[f] = frame
    return m


@functools.lru_cache(maxsize=None)
def case_list():
    """Every geometry x every table kind (the ragged geometries x two kinds), n cycling through 3..6: mask, conf, mv, frame_size,
    pair_stats (cuts at frames 1 and 4)."""
    cases = []
    for g, (h, w, fh, fw) in enumerate(GEOMETRIES + RAGGED_GEOMETRIES):
        for k, kind in enumerate(TABLES if g < len(GEOMETRIES) else RAGGED_TABLES):
            n = 3 + (g + k) % 4
            rng = np.random.default_rng(500 + 10 * g + k)
            c = dict(name=f"{(h, w, fh, fw)} {kind} n={n}", mask=flicker_frames(n, h, w, 40 + 10 * g + k), conf=rng.integers(0, 256, (n, h, w), dtype=np.uint8),
                     frame_size=(fh, fw), mv=np.stack([mc.make_table(kind, fh, fw, 3000 + 100 * g + 10 * k + f, (1, 1)) for f in range(n)]),
                     pair_stats=np.ascontiguousarray(CUT_STATS[np.arange(n) % 3]))
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cases.append(c)
    return cases


@functools.lru_cache(maxsize=None)
def case_sources(i):
    c = case_list()[i]
    n, h, w = c["mask"].shape
    return [sources(c["mv"][f], h, w, c["frame_size"]) for f in range(n)]


def case_kwargs(i, persist, use_conf, use_mv, use_stats):
    c = case_list()[i]
    kw = dict(classes=K, persist=persist)
    if use_conf:
        kw.update(conf=c["conf"], trust=TRUST)
    if use_mv:
        kw.update(mv=c["mv"], frame_size=c["frame_size"])
    if use_stats:
        kw.update(pair_stats=c["pair_stats"])
    return kw


@functools.lru_cache(maxsize=None)
def expected(i, persist, use_conf, use_mv, use_stats):
    """(out, state, counts) of the whole clip of case i in one call without a state, computed once and read-only."""
    got = mask_stabilize(case_list()[i]["mask"], None, _src=case_sources(i) if use_mv else None, **case_kwargs(i, persist, use_conf, use_mv, use_stats))
    for v in got:
        v.setflags(write=False)
    return got


def slice_kwargs(kw, s):
    """The keywords of a call for the frames s of the clip."""
    return {k: (v[s] if k in ("conf", "mv", "pair_stats") else v) for k, v in kw.items()}


def chained(mask, pieces, fn=mask_stabilize, **kw):
    """The clip in calls of the given lengths, each handed the state of the one before."""
    outs, counts, state, at = [], [], None, 0
    for n in pieces:
        s = slice(at, at + n)
        out, state, cnt = fn(mask[s], state, **slice_kwargs(kw, s))
        outs.append(out), counts.append(cnt)
        at += n
    return np.concatenate(outs), state, np.concatenate(counts)


# ------------------------------------------------------------------------------------------------ the quality scenes
def noisy_blobs(n, step, seed=7, noise=0.05):
    """(clean, noisy) blob scenes of tracks_mc_ref with the background mapped to class 4 and `noise` of the pixels re-drawn per frame."""
    b = dict(mc.BLOB_SCENE, n=n, step=step)
    clean = mc.blob_masks(**b)
    clean = np.where(clean >= K, 4, clean).astype(np.uint8)
    rng = np.random.default_rng(seed)
    flip = rng.random(clean.shape) < noise
    return clean, np.where(flip, rng.integers(0, K, clean.shape), clean).astype(np.uint8)


def errors(masks, clean):
    """Pixels that differ from the clean scene over frames 1 and later."""
    return int((masks[1:] != clean[1:]).sum())


# ------------------------------------------------------------------------------------------------ refusals
def call_stabilize(lib, **kw):
    """fs_mask_stabilize through the hook table with every argument a keyword; pointers default to a fake non-null, 16-byte aligned address."""
    fake = 0x1000
    a = dict(mask=fake, conf=fake, mv=None, pair_stats=None, n=2, H=8, W=8, frame_h=0, frame_w=0, K=5, persist=3, trust=256, has_state=1, state=fake, out=fake,
             counts=fake, workspace=None)
    a.update(kw)
    return lib.fs_mask_stabilize(a["mask"], a["conf"], a["mv"], a["pair_stats"], a["n"], a["H"], a["W"], a["frame_h"], a["frame_w"], a["K"], a["persist"],
                                 a["trust"], a["has_state"], a["state"], a["out"], a["counts"], a["workspace"], None)


def refusal_cases():
    """(keyword overrides, a word of the message)."""
    mvs = dict(mv=0x1000, frame_h=16, frame_w=16, workspace=0x1000)
    return [(dict(mask=None), b"null"), (dict(out=None), b"null"), (dict(state=None), b"null"), (dict(counts=None), b"null"),
            (dict(K=0), b"classes"), (dict(K=256), b"classes"), (dict(persist=0), b"persist"), (dict(persist=256), b"persist"),
            (dict(trust=-1), b"trust"), (dict(trust=257), b"trust"), (dict(n=0), b"at least one frame"), (dict(H=0), b"sizes"), (dict(W=-1), b"sizes"),
            (dict(H=46341, W=46341), b"2^31"), (dict(H=1, W=2 ** 31 - 1), b"2^31"), (dict(has_state=2), b"has_state"),
            (dict(state=0x1004), b"state plane is not aligned"), (dict(counts=0x1004), b"counts is not aligned"),
            (dict(mvs, workspace=None), b"workspace"), (dict(mvs, workspace=0x1008), b"workspace is not aligned"),
            (dict(mvs, frame_h=0), b"frame"), (dict(mvs, frame_h=15), b"frame"), (dict(mvs, frame_w=0), b"frame"),
            (dict(mvs, frame_h=46341, frame_w=46341, H=46341), b"2^31"), (dict(mvs, H=16 * 31 + 1), b"31"), (dict(mvs, W=16 * 31 + 1), b"31"),
            (dict(mvs, n=65536), b"65535")]
