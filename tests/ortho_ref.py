"""CPU restatement of the orthophoto under the flood-extent mosaic (include/floodseg_test.h: ortho_accumulate, ortho_compose; the same
rules as csrc/ortho_defs.h) for the tests: plain numpy, every op as literal loops and vectorised.  Everything is integer and hence defined
bit for bit, except the image sampled, which is egress_ref.background: the uint8 image the network saw, that the ingest and egress
tests already hold equal to the GPU's.  Which frame pixel lies under a canvas pixel is mosaic_ref's (the mosaic's own gather)."""
import numpy as np

import egress_ref
import mosaic_ref as mref

EMPTY = 0xFFFFFFFFFFFFFFFF
MODES = {"centre": 0, "latest": 1}
UNSEEN = 255


def canvas(size):
    """A fresh (rank uint64 [CH, CW] all ones, rgba uint32 [CH, CW] zero)."""
    return np.full(size, EMPTY, np.uint64), np.zeros(size, np.uint32)


def image(source, mask_size):
    """The image a frame is sampled from: source = (frame, chroma, fmt, matrix, full_range) as numpy -> uint8 [H, W, 3]."""
    frame, chroma, fmt, matrix, full_range = source
    return egress_ref.background(frame, chroma, fmt, matrix, full_range, size=mask_size)


def centre_key(x, y, h, w):
    return (2 * x + 1 - w) ** 2 + (2 * y + 1 - h) ** 2


def frame_rank(mode, x, y, h, w, ordinal):
    """Python ints: exact."""
    key = 0xFFFFFFFF - ordinal if MODES[mode] == 1 else centre_key(int(x), int(y), h, w)
    return (key << 32) | ordinal


def pack_rgba(px):
    return int(px[0]) | int(px[1]) << 8 | int(px[2]) << 16 | 0xFF << 24


# ------------------------------------------------------------------------------------------------ ortho_accumulate
def ortho_accumulate_loop(img, pose, ordinal, rank, rgba, origin, mode="centre"):
    """The definition literally: one frame (its sampled image uint8 [H, W, 3], one pose row, its ordinal) into (rank, rgba), in place."""
    assert 0 <= ordinal < 0xFFFFFFFF
    (h, w, _), (ch, cw), (oy, ox) = img.shape, rank.shape, origin
    if not mref.pose_votes(pose):
        return rank, rgba
    m = [int(v) for v in pose[6:12]]
    for Y in range(ch):
        for X in range(cw):
            ax, ay = (2 * (X - ox) + 1) << 19, (2 * (Y - oy) + 1) << 19
            x = (mref.rshr(m[0] * ax + m[1] * ay) + m[2]) >> mref.FRAC
            y = (mref.rshr(m[3] * ax + m[4] * ay) + m[5]) >> mref.FRAC
            if 0 <= x < w and 0 <= y < h:
                r = frame_rank(mode, x, y, h, w, ordinal)
                if r < int(rank[Y, X]):                                     # strictly
                    rank[Y, X] = r
                    rgba[Y, X] = pack_rgba(img[y, x])
    return rank, rgba


def ortho_accumulate(img, pose, ordinal, rank, rgba, origin, mode="centre"):
    """Vectorised; (rank, rgba) updated in place and returned."""
    assert 0 <= ordinal < 0xFFFFFFFF
    (h, w, _), (ch, cw), (oy, ox) = img.shape, rank.shape, origin
    if not mref.pose_votes(pose):
        return rank, rgba
    m = [int(v) for v in pose[6:12]]
    ax = (((2 * (np.arange(cw, dtype=np.int64) - ox) + 1)) << 19)[None, :]
    ay = (((2 * (np.arange(ch, dtype=np.int64) - oy) + 1)) << 19)[:, None]
    x = (mref.rshr(m[0] * ax + m[1] * ay) + m[2]) >> mref.FRAC
    y = (mref.rshr(m[3] * ax + m[4] * ay) + m[5]) >> mref.FRAC
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    Y, X = np.nonzero(inside)
    x, y = x[Y, X], y[Y, X]
    key = np.full(len(x), 0xFFFFFFFF - ordinal, np.int64) if MODES[mode] == 1 else centre_key(x, y, h, w)
    new = (key.astype(np.uint64) << np.uint64(32)) | np.uint64(ordinal)
    win = new < rank[Y, X]
    Y, X, x, y = Y[win], X[win], x[win], y[win]
    px = img[y, x].astype(np.uint32)
    rank[Y, X] = new[win]
    rgba[Y, X] = px[:, 0] | (px[:, 1] << np.uint32(8)) | (px[:, 2] << np.uint32(16)) | np.uint32(0xFF000000)
    return rank, rgba


def winners(rank):
    """-> (src int32 [CH, CW]: the winning frame's ordinal, -1 where empty; the covered pixel count)."""
    lit = rank != np.uint64(EMPTY)
    src = np.where(lit, (rank & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return src, int(lit.sum())


# ------------------------------------------------------------------------------------------------ ortho_compose
def edge_bits(edge):
    return sum(1 << int(k) for k in set(edge))


def blend255(a, colour, under):
    return (a * colour + (255 - a) * under + 127) // 255


def ortho_compose_loop(rgba, cls=None, palette=None, fill=(0, 0, 0), edge=()):
    """The definition literally -> uint8 [CH, CW, 3].  palette uint8 [K, 4] (R, G, B, A)."""
    ch, cw = rgba.shape
    k_max = 0 if palette is None else len(palette)
    out = np.zeros((ch, cw, 3), np.uint8)
    for Y in range(ch):
        for X in range(cw):
            v = int(rgba[Y, X])
            under = [(v >> (8 * c)) & 255 for c in range(3)] if v >> 24 else [int(c) for c in fill]
            k = UNSEEN if cls is None else int(cls[Y, X])
            px = under
            if cls is not None and k < k_max:                               # without a class plane nothing is looked up, whatever K is
                a = int(palette[k][3])
                if k in edge:
                    near = [int(cls[y, x]) for y, x in ((Y - 1, X), (Y + 1, X), (Y, X - 1), (Y, X + 1)) if 0 <= y < ch and 0 <= x < cw]
                    if any(n != k and n != UNSEEN for n in near):
                        a = 255
                px = [blend255(a, int(palette[k][c]), under[c]) for c in range(3)]
            out[Y, X] = px
    return out


def ortho_compose(rgba, cls=None, palette=None, fill=(0, 0, 0), edge=()):
    """Vectorised."""
    ch, cw = rgba.shape
    seen = (rgba >> np.uint32(24)) != 0
    rgb = np.stack([(rgba >> np.uint32(8 * c)) & np.uint32(255) for c in range(3)], -1).astype(np.int64)
    under = np.where(seen[..., None], rgb, np.array(fill, np.int64)[None, None, :])
    if cls is None:
        return under.astype(np.uint8)
    pal = np.asarray(palette).astype(np.int64)
    k = cls.astype(np.int64)
    drawn = k < len(pal)
    entry = pal[np.where(drawn, k, 0)]
    a = entry[..., 3]
    if edge:
        pad = np.pad(k, 1, constant_values=UNSEEN)
        near = [pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]]
        differs = np.zeros((ch, cw), bool)
        for n in near:
            differs |= (n != k) & (n != UNSEEN)
        a = np.where(np.isin(k, list(edge)) & differs, 255, a)
    o = blend255(a[..., None], entry[..., :3], under)
    return np.where(drawn[..., None], o, under).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ synthetic sources
def make_source(h, w, fmt, matrix="bt601", full_range=False, seed=0):
    """A random decoded frame as numpy: (frame, chroma, fmt, matrix, full_range), smooth enough that the resize has something to blend."""
    rng = np.random.RandomState(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if fmt == "rgb24":
        return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8), None, fmt, matrix, full_range
    y = rng.randint(0, 256, size=(h, w)).astype(np.uint8)
    if fmt == "nv12":
        return y, rng.randint(0, 256, size=(ch, cw, 2)).astype(np.uint8), fmt, matrix, full_range
    return y, (rng.randint(0, 256, size=(ch, cw)).astype(np.uint8), rng.randint(0, 256, size=(ch, cw)).astype(np.uint8)), fmt, matrix, full_range


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# (frame size, mask size): a 2:1 resize, odd sizes (chroma edge, no whole dwords), and the identity resize
FRAME_SIZES = (((48, 80), (24, 40)), ((45, 70), (37, 53)), ((32, 48), (32, 48)))
CANVASES = {(70, 150): (30, 50), (64, 128): (20, 40)}  # canvas -> origin (oy, ox): partial tiles and bytes; whole tiles and the wide stores
COLOURS = [("rgb24", "bt601", False)] + [(f, m, r) for f in ("nv12", "i420") for m in ("bt601", "bt709") for r in (False, True)]
ONE = mref.ONE


def case_poses(canvas):
    """The five pose rows every accumulate case gathers as frames 0..4, placed for this canvas: the identity; a translation that leaves the
    canvas at its top and its left; a 7 degree rotation with zoom 1.2 to the right of the anchor; a lost row; an ok row whose from_anchor
    breaks pose_votes' bounds (a linear entry of 16)."""
    oy, ox = CANVASES[canvas]
    c, s = 1.2 * np.cos(np.radians(7)), 1.2 * np.sin(np.radians(7))
    pairs = [mref.affine_pose(1, 0, 0, 1, 0, 0), mref.affine_pose(1, 0, 0, 1, -ox - 10, -oy - 4), mref.affine_pose(c, -s, s, c, 45, -oy + 5),
             mref.affine_pose(1, 0, 0, 1, 3, 3), (mref.IDENTITY, [16 * ONE, 0, 0, 0, ONE, 0])]
    return mref.pose_rows(pairs, status=[0, 0, 1, 2, 0])


def overlap_poses():
    """Three overlapping views for the order tests: each wins some pixels, in centre mode (nearest its own axis) and in latest mode."""
    c, s = 1.2 * np.cos(np.radians(7)), 1.2 * np.sin(np.radians(7))
    return mref.pose_rows([mref.affine_pose(1, 0, 0, 1, 0, 0), mref.affine_pose(1, 0, 0, 1, 21.5, 9.25), mref.affine_pose(c, -s, s, c, -12, -8)], status=[0, 1, 0])


def compose_planes(canvas, seed=5):
    """(rgba, cls) of a canvas for the compose tests: three quarters seen, classes in blocks with 255 (never seen), an id >= K = 5, and
    class boundaries that run into row 0 and column 0."""
    ch, cw = canvas
    rng = np.random.RandomState(seed)
    rgba = rng.randint(0, 1 << 24, size=canvas).astype(np.uint32) | np.uint32(0xFF000000)
    rgba[rng.rand(ch, cw) < 0.25] = 0
    yy, xx = np.mgrid[0:ch, 0:cw]
    cls = ((yy // 9 + xx // 13) % 5).astype(np.uint8)
    cls[(yy // 7 + xx // 11) % 6 == 0] = 255
    cls[5:9, 20:31] = 7
    cls[0, :6], cls[0, 6:12], cls[:5, 0], cls[5:11, 0] = 1, 3, 1, 2
    return rgba, cls


# ------------------------------------------------------------------------------------------------ the library's refusals
def good_arguments():
    """Per op the arguments of a call that passes validation (dummy non-null pointers), in the ABI's order, by name."""
    return {
        "ortho_accumulate": dict(frame=64, u=64, v=64, format=1, matrix=1, full_range=0, FH=256, FW=384, pose=64, ordinal=3, H=128, W=192, mode=0, CH=200,
                                 CW=300, ox=36, oy=54, rank=64, rgba=64, stream=None),
        "ortho_compose": dict(rgba=64, cls=64, palette=64, K=5, edge_set=0b10, fill=0x102030, CH=200, CW=300, out=64, stream=None),
    }


def refusal_cases():
    """(op, changed arguments, a word of the message)."""
    acc, com = "ortho_accumulate", "ortho_compose"
    cases = [(acc, {p: None}, b"null") for p in ("frame", "pose", "rank", "rgba", "u")]
    cases += [(acc, dict(format=2, v=None), b"null chroma"), (acc, dict(format=3), b"format"), (acc, dict(format=-1), b"format"), (acc, dict(matrix=2), b"matrix"),
              (acc, dict(full_range=2), b"range"), (acc, dict(FH=0), b"0x"), (acc, dict(FW=16385), b"16385"), (acc, dict(H=0), b"0x"), (acc, dict(W=16385), b"16385"),
              (acc, dict(CH=0), b"canvas"), (acc, dict(CW=16385), b"canvas"), (acc, dict(ox=16385), b"origin"), (acc, dict(oy=-16385), b"origin"),
              (acc, dict(mode=2), b"mode=2"), (acc, dict(mode=-1), b"mode=-1"), (acc, dict(ordinal=0xFFFFFFFF), b"ordinal=4294967295"),
              (acc, dict(pose=68), b"aligned to 8"), (acc, dict(rank=68), b"aligned to 8"), (acc, dict(rgba=66), b"aligned to 4")]
    cases += [(com, dict(rgba=None), b"null"), (com, dict(out=None), b"null"), (com, dict(palette=None), b"null"), (com, dict(CH=0), b"canvas"),
              (com, dict(CW=16385), b"canvas"), (com, dict(K=0), b"got 0"), (com, dict(K=257), b"got 257"), (com, dict(edge_set=0b100000), b"edge_set=0x20"),
              (com, dict(K=3, edge_set=0b1000), b"edge_set=0x8"), (com, dict(fill=1 << 24), b"fill=0x1000000"), (com, dict(rgba=66), b"aligned to 4")]
    return cases


def call_op(lib, op, **changed):
    args = dict(good_arguments()[op])
    args.update(changed)
    return getattr(lib, "fs_" + op)(*args.values())
