"""CPU restatement of frame-to-map registration (include/floodseg_test.h: map_view, map_gate, pose_correct; the same rules as
csrc/refine_defs.h) for the tests: plain numpy, map_view and map_gate vectorised and as literal loops over Python integers,
refine_step scalar (it is one row).  Everything is integer and hence defined bit for bit; the image a frame is sampled from is
ortho_ref.image (the uint8 image the network saw), the matcher and the fit between the ops are motion_modes_ref's and mosaic_ref's.
A test helper, not an oracle module."""
import functools

import numpy as np

import mosaic_ref as mref
import motion_modes_ref as mmref
import motion_ref
import ortho_ref as oref

ONE = mref.ONE
VOID_ROW = mref.VOID_ROW
OK, NO_FIT, OUT_OF_BOUNDS, NOT_TRACKING = 0, 2, 3, 4
SKIPPED_ROW = (1, 0, 0, 0, 0, 0, 0, 0)   # FlowPredictor's row for a frame that was not registered (refine_every, or no source)
TRACKING = 1


# ------------------------------------------------------------------------------------------------ map_view
def view_usable(pose):
    pose = [int(v) for v in pose]
    return (pose[12] in (mref.POSE_OK, mref.POSE_BRIDGED) and all(abs(pose[i]) < mref.POSE_LINEAR_LIMIT for i in (0, 1, 3, 4))
            and abs(pose[2]) < mref.POSE_SHIFT_LIMIT and abs(pose[5]) < mref.POSE_SHIFT_LIMIT)


def canvas_pixel(t, x, y, ox, oy):
    """Python integers (or int64 arrays): the canvas pixel under the centre of frame pixel (x, y)."""
    ax, ay = (2 * x + 1) << 19, (2 * y + 1) << 19
    return ((mref.rshr(t[0] * ax + t[1] * ay) + t[2]) >> mref.FRAC) + ox, ((mref.rshr(t[3] * ax + t[4] * ay) + t[5]) >> mref.FRAC) + oy


def luma_of(rgba):
    return (77 * (rgba & 255) + 150 * ((rgba >> 8) & 255) + 29 * ((rgba >> 16) & 255) + 128) >> 8


def map_view_loop(img, pose, ordinal, rank, rgba, origin, min_age=0):
    """The definition literally: img uint8 [H, W, 3] (ortho_ref.image), one pose row, the canvas planes -> (cur, view, valid) uint8 [H, W]."""
    assert 0 <= ordinal < 0xFFFFFFFF and min_age >= 0
    (h, w, _), (ch, cw), (oy, ox) = img.shape, rgba.shape, origin
    cur, view, valid = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    usable = view_usable(pose)
    t = [int(v) for v in pose[0:6]]
    for y in range(h):
        for x in range(w):
            r, g, b = (int(v) for v in img[y, x])
            cur[y, x] = (77 * r + 150 * g + 29 * b + 128) >> 8
            if not usable:
                continue
            X, Y = canvas_pixel(t, x, y, ox, oy)
            if not (0 <= X < cw and 0 <= Y < ch):
                continue
            px = int(rgba[Y, X])
            if px >> 24 == 0:
                continue
            if min_age > 0 and ordinal - (int(rank[Y, X]) & 0xFFFFFFFF) < min_age:
                continue
            view[y, x], valid[y, x] = luma_of(px), 1
    return cur, view, valid


def map_view(img, pose, ordinal, rank, rgba, origin, min_age=0):
    """Vectorised."""
    assert 0 <= ordinal < 0xFFFFFFFF and min_age >= 0
    (h, w, _), (ch, cw), (oy, ox) = img.shape, rgba.shape, origin
    cur = motion_ref.luma(img)
    view, valid = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    if not view_usable(pose):
        return cur, view, valid
    t = [int(v) for v in pose[0:6]]
    X, Y = canvas_pixel(t, np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None], ox, oy)
    inside = (X >= 0) & (X < cw) & (Y >= 0) & (Y < ch)
    y, x = np.nonzero(inside)
    X, Y = X[y, x], Y[y, x]
    px = rgba[Y, X].astype(np.int64)
    ok = (px >> 24) != 0
    if min_age > 0:
        ok &= ordinal - (rank[Y, X] & np.uint64(0xFFFFFFFF)).astype(np.int64) >= min_age
    y, x, px = y[ok], x[ok], px[ok]
    view[y, x], valid[y, x] = luma_of(px), 1
    return cur, view, valid


# ------------------------------------------------------------------------------------------------ map_gate
def map_gate_loop(table, valid):
    """The definition literally -> a gated copy of the table."""
    h, w = valid.shape
    out = []
    for row in np.asarray(table).tolist():
        x0, y0 = row[3] - 8, row[4] - 8
        keep = x0 >= 0 and y0 >= 0 and x0 + 16 <= w and y0 + 16 <= h and all(valid[y0 + j, x0 + i] == 1 for j in range(16) for i in range(16))
        out.append(row if keep else list(VOID_ROW))
    return np.array(out, np.int32).reshape(-1, 7)


def map_gate(table, valid):
    """Vectorised: the count of valid pixels under every 16 x 16 window from a summed-area table."""
    h, w = valid.shape
    t = np.asarray(table).astype(np.int64)
    x0, y0 = t[:, 3] - 8, t[:, 4] - 8
    inside = (x0 >= 0) & (y0 >= 0) & (x0 + 16 <= w) & (y0 + 16 <= h)
    sat = np.zeros((h + 1, w + 1), np.int64)
    sat[1:, 1:] = (valid == 1).cumsum(0).cumsum(1)
    xs, ys = np.where(inside, x0, 0), np.where(inside, y0, 0)
    count = sat[ys + 16, xs + 16] - sat[ys, xs + 16] - sat[ys + 16, xs] + sat[ys, xs]
    out = np.asarray(table).astype(np.int32).copy()
    out[~(inside & (count == 256))] = VOID_ROW
    return out


# ------------------------------------------------------------------------------------------------ pose_correct
def refine_step(model, state, pose, mask_size, canvas_size, origin):
    """One row each, Python integers -> (state, pose, out) as int64 arrays; the inputs are not changed."""
    (h, w), (ch, cw), (oy, ox) = mask_size, canvas_size, origin
    m, st, p = [int(v) for v in np.asarray(model).reshape(-1)], [int(v) for v in state], [int(v) for v in pose]
    status = OK
    if p[12] not in (mref.POSE_OK, mref.POSE_BRIDGED) or st[24] != TRACKING or st[0:6] != p[0:6]:
        status = NOT_TRACKING
    elif m[12] != mref.OK or not mref.pair_in_bounds(m[0:6], m[6:12]):
        status = NO_FIT
    elif not mref.pose_in_bounds(st[0:6], st[6:12]):
        status = OUT_OF_BOUNDS
    else:
        to_next, from_next = mref.compose(st[0:6], m[0:6]), mref.compose(m[6:12], st[6:12])
        if not mref.pose_in_bounds(to_next, from_next):
            status = OUT_OF_BOUNDS
        else:
            st[0:6], st[6:12], p[0:6], p[6:12] = to_next, from_next, to_next, from_next
            p[13] = int(mref.frame_clipped(to_next, h, w, ch, cw, ox, oy))
    out = [status, m[13], m[14], m[15], m[2], m[5], 0, 0]
    return np.array(st, np.int64), np.array(p, np.int64), np.array(out, np.int64)


def step_cases():
    """(name, model row, state, pose row, status) for pose_correct: once for each status, and the other ways into 2 and 4.  The state's
    last 20 words hold values of their own, so a write to any of them shows."""
    to, back = mref.affine_pose(1, 0, 0, 1, 12, -5)
    state = np.arange(100, 132, dtype=np.int64)
    state[0:6], state[6:12], state[24] = to, back, TRACKING
    pose = np.array(to + back + [0, 0, 9, 20], np.int64)
    fwd, inv = mref.affine_pose(1.001, 0.002, -0.002, 0.999, -1.25, 0.5)
    good = np.array(mref.model_row(fwd, inv, mref.OK, 20, 16, 4), np.int64)
    few = np.array(mref.model_row(mref.IDENTITY, mref.IDENTITY, mref.FEW, 3, 0, 0), np.int64)
    wild = good.copy()
    wild[1] = 3 * ONE                                     # an "ok" row outside the pair bounds
    far_to, far_back = mref.affine_pose(1, 0, 0, 1, 16383.5, 0)
    far_state, far_pose = state.copy(), pose.copy()
    far_state[0:6], far_state[6:12], far_pose[0:12] = far_to, far_back, far_to + far_back
    push = np.array(mref.model_row(*mref.affine_pose(1, 0, 0, 1, 1.0, 0), mref.OK, 20, 16, 4), np.int64)
    lost_pose, bridged, lost_state, other = pose.copy(), pose.copy(), state.copy(), state.copy()
    lost_pose[12], bridged[12], lost_state[24], other[2] = mref.POSE_LOST, mref.POSE_BRIDGED, 2, state[2] + 1
    return [("corrected", good, state, pose, OK), ("bridged row", good, state, bridged, OK), ("too few", few, state, pose, NO_FIT),
            ("out of the pair bounds", wild, state, pose, NO_FIT), ("past the canvas bound", push, far_state, far_pose, OUT_OF_BOUNDS),
            ("lost row", good, state, lost_pose, NOT_TRACKING), ("lost chain", good, lost_state, pose, NOT_TRACKING),
            ("another frame's state", good, other, pose, NOT_TRACKING)]


# ------------------------------------------------------------------------------------------------ the per-frame chain
def refine_frame(img, pose, state, ordinal, rank, rgba, canvas_size, origin, mask=None, exclude_set=0, search=8, penalty=0, intra_bias=65535, min_age=0,
                 rounds=4, tol=ONE, min_inliers=12, view=map_view, gate=map_gate):
    """map_view -> block_match_modes -> map_gate -> global_motion -> pose_correct for one frame whose pose row pose_chain has just
    written -> (state, pose, out, (cur, view, valid, table, model)).  mask: the frame's own uint8 [H, W] for global_motion's exclude_set."""
    size = img.shape[:2]
    cur, seen, valid = view(img, pose, ordinal, rank, rgba, origin, min_age)
    table, _, _, stats = mmref.block_match_modes(cur, seen, search, penalty, intra_bias)
    table = gate(table, valid)
    model = mref.global_motion([table], size, size, rounds, tol, min_inliers, None if mask is None else mask[None], exclude_set, [stats])
    state, pose, out = refine_step(model[0], state, pose, size, canvas_size, origin)
    return state, pose, out, (cur, seen, valid, table, model)


def run_flight(images, tables, canvas_size, origin, refine=True, mode="centre", masks=None, chain=None, every=1, pairs=None, **settings):
    """The loop FlowPredictor(mosaic_refine=True) runs, frame by frame: pose_chain with n = 1 on the frame's PAIR model (tables[f], from
    frame f - 1; row 0 is the anchor's and ignored), the registration against the canvas so far, then ortho_accumulate with the corrected
    row.  -> (poses int64 [n, 16], outs int64 [n, 8], state, (rank, rgba)).  chain: global_motion's settings for the pair tables; pairs: the
    pair models int64 [n, 16] themselves, instead of tables.  An image that is None (a frame without a source) is neither registered nor
    gathered."""
    size = next(img for img in images if img is not None).shape[:2]
    chain = dict(mref.SCENE_SETTINGS) if chain is None else chain
    state = np.zeros(32, np.int64)
    rank, rgba = oref.canvas(canvas_size)
    poses, outs = [], []
    for f, img in enumerate(images):
        pair = mref.global_motion([tables[f]], size, size, **chain) if pairs is None else np.asarray(pairs)[f:f + 1]
        row, state = mref.pose_chain(pair, state, size, canvas_size, origin)
        pose, out = row[0], np.array(SKIPPED_ROW, np.int64)
        if refine and f % every == 0 and img is not None:
            state, pose, out, _ = refine_frame(img, pose, state, f, rank, rgba, canvas_size, origin, None if masks is None else masks[f], **settings)
        if img is not None:
            oref.ortho_accumulate(img, pose, f, rank, rgba, origin, mode)
        poses.append(pose)
        outs.append(out)
    return np.array(poses, np.int64), np.array(outs, np.int64), state, (rank, rgba)


# ------------------------------------------------------------------------------------------------ the scenes
FLIGHT_SIZE, FLIGHT_CANVAS, FLIGHT_ORIGIN, FLIGHT_STEP, FLIGHT_BIAS = (64, 96), (128, 192), (32, 48), 4, (1, 0)
FLIGHT_SETTINGS = dict(search=8, min_age=0, rounds=4, tol=ONE, min_inliers=6)


@functools.lru_cache(maxsize=None)
def ground():
    """A seeded random RGB texture, 128 x 256: SAD is 0 at the true offset only."""
    g = np.random.RandomState(26).randint(0, 256, size=(128, 256, 3)).astype(np.uint8)
    g.setflags(write=False)
    return g


def flight(offsets_x, bias=FLIGHT_BIAS, row=32):
    """Frames cut from ground() at integer offsets (row `row`, column 64 + offsets_x[f]) and SYNTHESISED pair tables: every row says the
    true vector plus `bias`.  -> (images [uint8 64 x 96 x 3], tables, true to_anchor translations in pixels [(tx, ty)])."""
    (h, w), g = FLIGHT_SIZE, ground()
    images = [np.ascontiguousarray(g[row:row + h, 64 + x:64 + x + w]) for x in offsets_x]
    steps = [0] + [offsets_x[f] - offsets_x[f - 1] for f in range(1, len(offsets_x))]   # frame f's pixel x is frame f - 1's pixel x + step
    tables = [mref.grid_table(h // 16, w // 16, lambda cx, cy, s=s: (np.full_like(cx, s + bias[0]), np.full_like(cy, bias[1]))) for s in steps]
    return images, tables, [(x - offsets_x[0], 0) for x in offsets_x]


def straight_flight(row=32):
    return flight([FLIGHT_STEP * f for f in range(6)], row=row)


def revisit_flight():
    """Out six frames and back six: frame 11 is where frame 0 was."""
    return flight([FLIGHT_STEP * f for f in range(6)] + [FLIGHT_STEP * (5 - f) for f in range(6)])


def translation_px(pose):
    """A pose row's to_anchor translation in pixels, exact only when it is a whole number of them."""
    return int(pose[2]) / ONE, int(pose[5]) / ONE


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
VIEW_CANVAS, VIEW_ORIGIN = (96, 160), (20, 30)


def view_poses(mask_size):
    """The pose rows every map_view case draws with: the identity; a translation that pushes half the frame off the canvas; a rotation of
    3 degrees with zoom 1.02; a lost row; an ok row whose to_anchor breaks the bounds (a linear entry of 16)."""
    h, w = mask_size
    c, s = 1.02 * np.cos(np.radians(3)), 1.02 * np.sin(np.radians(3))
    pairs = [mref.affine_pose(1, 0, 0, 1, 0, 0), mref.affine_pose(1, 0, 0, 1, VIEW_CANVAS[1] - VIEW_ORIGIN[1] - w // 2, 5), mref.affine_pose(c, -s, s, c, 6, -4),
             mref.affine_pose(1, 0, 0, 1, 3, 3), ([16 * ONE, 0, 0, 0, ONE, 0], mref.IDENTITY)]
    return mref.pose_rows(pairs, status=[0, 1, 0, 2, 0])


def view_canvas(mask_size, seed=12):
    """A canvas written by four earlier frames (ordinals 0..3, random images, shifted poses) in centre mode -> (rank, rgba), read-only."""
    rng = np.random.RandomState(seed)
    rank, rgba = oref.canvas(VIEW_CANVAS)
    for f, shift in enumerate(((0, 0), (VIEW_CANVAS[1] - VIEW_ORIGIN[1] - mask_size[1] // 2 - 7, -6), (17, 9), (-11, 14))):   # the second: under view_poses' second
        img = rng.randint(0, 256, size=mask_size + (3,)).astype(np.uint8)
        oref.ortho_accumulate(img, mref.pose_rows([mref.affine_pose(1, 0, 0, 1, *shift)])[0], f, rank, rgba, VIEW_ORIGIN)
    return rank, rgba


def gate_case():
    """A 48 x 64 valid plane (3 x 4 blocks) that is 1 on columns 0..39 and rows 0..47, and a table whose winners lie fully inside valid
    ground, straddle its edge by one pixel, lie on the plane's border (inside and one pixel out), are void already, or hold garbage.
    -> (table int32 [12, 7], valid uint8 [48, 64], the rows that survive)."""
    valid = np.zeros((48, 64), np.uint8)
    valid[:, :40] = 1
    t = mref.grid_table(3, 4, lambda cx, cy: (np.zeros_like(cx), np.zeros_like(cy)))
    src = [(8, 8), (24, 8), (32, 8), (33, 8),            # kept: on the plane's border; inside; touching the ground's edge.  One pixel over that edge
           (7, 8), (56, 24), (24, 40), (24, 41),         # one pixel out of the plane; in the plane on invalid ground; the bottom border (kept); one pixel below
           (-16, -16), (2 ** 31 - 1, 8), (8, -2 ** 31), (8, 24)]   # void already; garbage twice (the 64-bit test); a window that holds the byte below
    for i, (sx, sy) in enumerate(src):
        t[i, 3], t[i, 4] = sx, sy
    t[8] = VOID_ROW
    valid[20, 3] = 2                                      # a byte that is neither 0 nor 1 is not valid
    return t, valid, [0, 1, 2, 6]


# ------------------------------------------------------------------------------------------------ the library's refusals
def good_arguments():
    """Per op the arguments of a call that passes validation (dummy non-null pointers), in the ABI's order, by name."""
    return {
        "map_view": dict(frame=64, u=64, v=64, format=1, matrix=1, full_range=0, FH=256, FW=384, pose=64, ordinal=3, H=128, W=192, CH=200, CW=300, ox=36, oy=54,
                         rank=64, rgba=64, min_age=0, cur=64, view=64, valid=64, stream=None),
        "map_gate": dict(table=64, blocks=96, valid=64, H=128, W=192, stream=None),
        "pose_correct": dict(model=64, state=64, pose=64, H=128, W=192, CH=200, CW=300, ox=36, oy=54, out=64, stream=None),
    }


def refusal_cases():
    """(op, changed arguments, a word of the message)."""
    view, gate, fix = "map_view", "map_gate", "pose_correct"
    cases = [(view, {p: None}, b"null") for p in ("frame", "pose", "rank", "rgba", "u", "cur", "view", "valid")]
    cases += [(view, dict(format=2, v=None), b"null chroma"), (view, dict(format=3), b"format"), (view, dict(format=-1), b"format"), (view, dict(matrix=2), b"matrix"),
              (view, dict(full_range=2), b"range"), (view, dict(FH=0), b"0x"), (view, dict(FW=16385), b"16385"), (view, dict(H=15), b"15x"), (view, dict(W=15), b"x15"),
              (view, dict(W=16385), b"16385"), (view, dict(CH=0), b"canvas"), (view, dict(CW=16385), b"canvas"), (view, dict(ox=16385), b"origin"),
              (view, dict(oy=-16385), b"origin"), (view, dict(ordinal=0xFFFFFFFF), b"ordinal=4294967295"), (view, dict(min_age=-1), b"min_age=-1"),
              (view, dict(pose=68), b"aligned to 8"), (view, dict(rank=68), b"aligned to 8"), (view, dict(rgba=66), b"aligned to 4")]
    cases += [(gate, dict(table=None), b"null"), (gate, dict(valid=None), b"null"), (gate, dict(H=15, blocks=0), b"15x"), (gate, dict(W=16385), b"16385"),
              (gate, dict(blocks=95), b"blocks=95"), (gate, dict(table=66), b"aligned to 4")]
    cases += [(fix, {p: None}, b"null") for p in ("model", "state", "pose", "out")]
    cases += [(fix, dict(H=0), b"0x"), (fix, dict(W=16385), b"16385"), (fix, dict(CH=0), b"canvas"), (fix, dict(CW=16385), b"canvas"), (fix, dict(ox=16385), b"origin"),
              (fix, dict(oy=-16385), b"origin"), (fix, dict(model=68), b"aligned to 8"), (fix, dict(state=68), b"aligned to 8"), (fix, dict(pose=68), b"aligned to 8"),
              (fix, dict(out=68), b"aligned to 8")]
    return cases


def call_op(lib, op, **changed):
    args = dict(good_arguments()[op])
    args.update(changed)
    return getattr(lib, "fs_" + op)(*args.values())
