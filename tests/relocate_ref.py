"""CPU restatement of relocalisation against the orthophoto (include/floodseg_test.h: map_coarse, map_patch, map_locate, pose_relocate,
relocate_commit; the same rules as csrc/relocate_defs.h) for the tests: plain numpy, the three plane ops vectorised and as
literal loops over Python integers, the two steps scalar (they are one row each).  Everything is integer and hence defined bit for bit;
the image is ortho_ref.image, the fine registration between pose_relocate and relocate_commit is refine_ref's.  A test helper, not an
oracle module."""
import numpy as np

import mosaic_ref as mref
import ortho_ref as oref
import refine_ref as rref

ONE = mref.ONE
PATCH_OK, PATCH_NOT_LOST, PATCH_OUT_OF_BOUNDS, PATCH_CELLS, PATCH_WIDER = 0, 1, 2, 3, 4
FOUND, FOUND_NONE, FOUND_BAD_GEOM = 0, 1, 2
RELOCATED, NOT_ATTEMPTED, NO_PLACEMENT, REJECTED_MEAN, REJECTED_UNIQUENESS, FINE_FAILED, PATCH_REFUSED, OUT_OF_BOUNDS = range(8)
NOT_ATTEMPTED_ROW = (1, 0, 0, 0, 0, 0, 0, 0)   # FlowPredictor's row for a frame it did not try (relocate_every, or no source)
MAX_PATCH_CELLS, MAX_SIDE = 65536, 16384
LOST, TRACKING = 2, 1
DEFAULTS = dict(min_overlap=500, exclude=2, max_mean=16, ratio=800)


def cell_mean(total, s):
    return (total + s * s // 2) // (s * s)


# ------------------------------------------------------------------------------------------------ map_coarse
def map_coarse_loop(rgba, s):
    ch, cw = rgba.shape[0] // s, rgba.shape[1] // s
    cl, cv = np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)
    for cy in range(ch):
        for cx in range(cw):
            px = [int(rgba[cy * s + b, cx * s + a]) for b in range(s) for a in range(s)]
            if all(p >> 24 != 0 for p in px):
                cl[cy, cx], cv[cy, cx] = cell_mean(sum(rref.luma_of(p) for p in px), s), 1
    return cl, cv


def map_coarse(rgba, s):
    ch, cw = rgba.shape[0] // s, rgba.shape[1] // s
    px = rgba[:ch * s, :cw * s].astype(np.int64).reshape(ch, s, cw, s)
    cv = ((px >> 24) != 0).all(axis=(1, 3))
    cl = cell_mean(rref.luma_of(px).sum(axis=(1, 3)), s)
    return np.where(cv, cl, 0).astype(np.uint8), cv.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ map_patch
def patch_geometry(state, mask_size, canvas_size, origin, s):
    """Python integers -> geom [8]."""
    (h, w), (ch, cw), (oy, ox) = mask_size, canvas_size, origin
    st = [int(v) for v in state]
    if st[24] != LOST:
        return [PATCH_NOT_LOST] + [0] * 7
    if not mref.pose_in_bounds(st[0:6], st[6:12]):
        return [PATCH_OUT_OF_BOUNDS] + [0] * 7
    xs = [st[0] * x + st[1] * y + st[2] + ox * ONE for x, y in ((0, 0), (w, 0), (0, h), (w, h))]
    ys = [st[3] * x + st[4] * y + st[5] + oy * ONE for x, y in ((0, 0), (w, 0), (0, h), (w, h))]
    x0, x1, y0, y1 = min(xs) >> 20, (max(xs) + ONE - 1) >> 20, min(ys) >> 20, (max(ys) + ONE - 1) >> 20
    pu0, pu1, pv0, pv1 = x0 // s, (x1 + s - 1) // s, y0 // s, (y1 + s - 1) // s
    tw, th = pu1 - pu0 if x1 > x0 else 0, pv1 - pv0 if y1 > y0 else 0
    if tw < 1 or th < 1 or tw * th > MAX_PATCH_CELLS:
        return [PATCH_CELLS] + [0] * 7
    if tw > cw // s or th > ch // s:
        return [PATCH_WIDER] + [0] * 7
    return [PATCH_OK, pu0, pv0, tw, th, 0, 0, 0]


def _source(m, X, Y, ox, oy):
    ax, ay = (2 * (X - ox) + 1) << 19, (2 * (Y - oy) + 1) << 19
    return (mref.rshr(m[0] * ax + m[1] * ay) + m[2]) >> mref.FRAC, (mref.rshr(m[3] * ax + m[4] * ay) + m[5]) >> mref.FRAC


def map_patch_loop(img, state, canvas_size, origin, s):
    """img uint8 [H, W, 3] (ortho_ref.image) -> (tl, tv uint8 [th, tw], geom int64 [8]); a failing call has planes of no cell."""
    (h, w, _), (oy, ox) = img.shape, origin
    geom = patch_geometry(state, (h, w), canvas_size, origin, s)
    if geom[0] != PATCH_OK:
        return np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8), np.array(geom, np.int64)
    _, pu0, pv0, tw, th = geom[:5]
    m = [int(v) for v in state[6:12]]
    tl, tv = np.zeros((th, tw), np.uint8), np.zeros((th, tw), np.uint8)
    for j in range(th):
        for i in range(tw):
            total, ok = 0, True
            for b in range(s):
                for a in range(s):
                    x, y = _source(m, (pu0 + i) * s + a, (pv0 + j) * s + b, ox, oy)
                    if not (0 <= x < w and 0 <= y < h):
                        ok = False
                        continue
                    r, g, bl = (int(v) for v in img[y, x])
                    total += (77 * r + 150 * g + 29 * bl + 128) >> 8
            if ok:
                tl[j, i], tv[j, i] = cell_mean(total, s), 1
    geom[5] = int(tv.sum())
    return tl, tv, np.array(geom, np.int64)


def map_patch(img, state, canvas_size, origin, s):
    """Vectorised."""
    (h, w, _), (oy, ox) = img.shape, origin
    geom = patch_geometry(state, (h, w), canvas_size, origin, s)
    if geom[0] != PATCH_OK:
        return np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8), np.array(geom, np.int64)
    _, pu0, pv0, tw, th = geom[:5]
    m = [int(v) for v in state[6:12]]
    X = (pu0 * s + np.arange(tw * s, dtype=np.int64))[None, :]
    Y = (pv0 * s + np.arange(th * s, dtype=np.int64))[:, None]
    x, y = _source(m, X, Y, ox, oy)
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    luma = ((77 * img[..., 0].astype(np.int64) + 150 * img[..., 1].astype(np.int64) + 29 * img[..., 2].astype(np.int64) + 128) >> 8)
    seen = np.where(inside, luma[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)
    tv = inside.reshape(th, s, tw, s).all(axis=(1, 3))
    tl = cell_mean(seen.reshape(th, s, tw, s).sum(axis=(1, 3)), s)
    geom[5] = int(tv.sum())
    return np.where(tv, tl, 0).astype(np.uint8), tv.astype(np.uint8), np.array(geom, np.int64)


# ------------------------------------------------------------------------------------------------ map_locate
def geom_ok(geom, ch, cw):
    g = [int(v) for v in geom]
    return (g[0] == PATCH_OK and 1 <= g[3] <= cw and 1 <= g[4] <= ch and g[3] * g[4] <= MAX_PATCH_CELLS and 0 <= g[5] <= g[3] * g[4]
            and abs(g[1]) < 1 << 20 and abs(g[2]) < 1 << 20)


def better(a, b):
    """(sad, n, u, v) tuples; n == 0 is no placement."""
    if a[1] == 0 or b[1] == 0:
        return a[1] != 0
    left, right = a[0] * b[1], b[0] * a[1]
    if left != right:
        return left < right
    if a[1] != b[1]:
        return a[1] > b[1]
    if a[3] != b[3]:
        return a[3] < b[3]
    return a[2] < b[2]


def _pick(scores, nt, permille, exclude):
    """scores: [(sad, n, u, v)] of every placement -> found [16]."""
    none = (0, 0, 0, 0)
    fit = [s for s in scores if s[1] >= 1 and 1000 * s[1] >= permille * nt]
    best = none
    for s in fit:
        if better(s, best):
            best = s
    found = [0] * 16
    found[10], found[11], found[12] = len(scores), len(fit), nt
    if best[1] == 0:
        found[0] = FOUND_NONE
        return np.array(found, np.int64)
    second = none
    for s in fit:
        if max(abs(s[2] - best[2]), abs(s[3] - best[3])) > exclude and better(s, second):
            second = s
    found[1:5] = [best[2], best[3], best[0], best[1]]
    if second[1] != 0:
        found[5:10] = [1, second[2], second[3], second[0], second[1]]
    return np.array(found, np.int64)


def map_locate_loop(cl, cv, tl, tv, geom, min_overlap=500, exclude=2):
    ch, cw = cl.shape
    if not geom_ok(geom, ch, cw):
        return np.array([FOUND_BAD_GEOM] + [0] * 15, np.int64)
    _, pu0, pv0, tw, th, nt = (int(v) for v in geom[:6])
    tl, tv = np.asarray(tl).reshape(-1)[:tw * th].reshape(th, tw), np.asarray(tv).reshape(-1)[:tw * th].reshape(th, tw)
    scores = []
    for av in range(ch - th + 1):
        for au in range(cw - tw + 1):
            sad = n = 0
            for j in range(th):
                for i in range(tw):
                    if cv[av + j, au + i] == 1 and tv[j, i] == 1:
                        n += 1
                        sad += abs(int(cl[av + j, au + i]) - int(tl[j, i]))
            scores.append((sad, n, au - pu0, av - pv0))
    return _pick(scores, nt, min_overlap, exclude)


def map_locate(cl, cv, tl, tv, geom, min_overlap=500, exclude=2):
    """Vectorised over placements."""
    ch, cw = cl.shape
    if not geom_ok(geom, ch, cw):
        return np.array([FOUND_BAD_GEOM] + [0] * 15, np.int64)
    _, pu0, pv0, tw, th, nt = (int(v) for v in geom[:6])
    tl = np.asarray(tl).reshape(-1)[:tw * th].reshape(th, tw).astype(np.int64)
    tv = np.asarray(tv).reshape(-1)[:tw * th].reshape(th, tw) == 1
    wl = np.lib.stride_tricks.sliding_window_view(cl.astype(np.int64), (th, tw))
    wv = np.lib.stride_tricks.sliding_window_view(cv == 1, (th, tw))
    both = wv & tv[None, None]
    n = both.sum(axis=(2, 3))
    sad = (np.abs(wl - tl[None, None]) * both).sum(axis=(2, 3))
    scores = [(int(sad[av, au]), int(n[av, au]), au - pu0, av - pv0) for av in range(ch - th + 1) for au in range(cw - tw + 1)]
    return _pick(scores, nt, min_overlap, exclude)


# ------------------------------------------------------------------------------------------------ pose_relocate, relocate_commit
def translate(to, back, dx, dy):
    """Both poses moved by (dx, dy) whole canvas pixels: exact."""
    to, back = list(to), list(back)
    to[2], to[5] = to[2] + dx * ONE, to[5] + dy * ONE
    back[2], back[5] = back[2] - (back[0] * dx + back[1] * dy), back[5] - (back[3] * dx + back[4] * dy)
    return to, back


def _pair_ok(sad, n):
    return 1 <= n <= MAX_PATCH_CELLS and 0 <= sad <= 255 * n


def relocate_step(found, state, mask_size, canvas_size, origin, s, max_mean=16, ratio=800):
    """-> (cand_state int64 [32], cand_pose int64 [16]); the decision is cand_state[28]."""
    (h, w), (ch, cw), (oy, ox) = mask_size, canvas_size, origin
    f, st = [int(v) for v in found], [int(v) for v in state]
    decision, to, back = RELOCATED, None, None
    if st[24] != LOST:
        decision = NOT_ATTEMPTED
    elif f[0] == FOUND_NONE:
        decision = NO_PLACEMENT
    elif (f[0] != FOUND or not mref.pose_in_bounds(st[0:6], st[6:12]) or not _pair_ok(f[3], f[4]) or abs(f[1]) > MAX_SIDE or abs(f[2]) > MAX_SIDE
          or (f[5] != 0 and not _pair_ok(f[8], f[9]))):
        decision = PATCH_REFUSED
    elif f[3] > max_mean * f[4]:
        decision = REJECTED_MEAN
    elif f[5] != 0 and 1000 * f[3] * f[9] > ratio * f[8] * f[4]:
        decision = REJECTED_UNIQUENESS
    else:
        to, back = translate(st[0:6], st[6:12], s * f[1], s * f[2])
        if not mref.pose_in_bounds(to, back):
            decision = OUT_OF_BOUNDS
    cand = list(st)
    if decision == RELOCATED:
        cand[0:6], cand[6:12], cand[12:18], cand[18:24], cand[24], cand[27] = to, back, mref.IDENTITY, mref.IDENTITY, TRACKING, 0
        pose = to + back + [mref.POSE_OK, int(mref.frame_clipped(to, h, w, ch, cw, ox, oy)), 0, 0]
    else:
        pose = mref.IDENTITY + mref.IDENTITY + [mref.POSE_LOST, 0, 0, 0]
    cand[28] = decision
    return np.array(cand, np.int64), np.array(pose, np.int64)


def commit_step(cand_state, cand_pose, correct_out, state, pose, found, s):
    """-> (state, pose, out [8]); the inputs are not changed."""
    cs, cp, st, p, f = ([int(v) for v in a] for a in (cand_state, cand_pose, state, pose, found))
    d = cs[28]
    status = d if d in (RELOCATED, NOT_ATTEMPTED, NO_PLACEMENT, REJECTED_MEAN, REJECTED_UNIQUENESS, PATCH_REFUSED, OUT_OF_BOUNDS) else PATCH_REFUSED
    if status == RELOCATED and (int(correct_out[0]) != rref.OK or cs[24] != TRACKING or cp[12] != mref.POSE_OK or not mref.pose_in_bounds(cs[0:6], cs[6:12])):
        status = FINE_FAILED
    if status == RELOCATED:
        st[0:28], p[0:14] = cs[0:28], cp[0:14]
    out = [status] + [0] * 7
    if f[0] == FOUND and abs(f[1]) <= MAX_SIDE and abs(f[2]) <= MAX_SIDE:
        out[1:5] = [s * f[1], s * f[2], f[3], f[4]]
        if f[5] != 0:
            out[5:7] = [f[8], f[9]]
    if f[0] in (FOUND, FOUND_NONE):
        out[7] = f[11]
    return np.array(st, np.int64), np.array(p, np.int64), np.array(out, np.int64)


def found_row(status=FOUND, u=0, v=0, sad=0, n=1, second=None, placements=1, eligible=1, nt=1):
    row = [status, u, v, sad, n] + ([1] + list(second) if second else [0, 0, 0, 0, 0]) + [placements, eligible, nt, 0, 0, 0]
    return np.array(row, np.int64)


STEP_GEOMETRY = dict(mask_size=(64, 96), canvas_size=(128, 192), origin=(32, 48))


def step_cases():
    """(name, found, state, max_mean, ratio, decision) for pose_relocate: every decision, and the other ways into 6.  The state's last
    words hold values of their own, so a write to any of them shows."""
    to, back = mref.affine_pose(1.01, 0.02, -0.02, 0.99, 12, -5)
    state = np.arange(100, 132, dtype=np.int64)
    state[0:6], state[6:12], state[24] = to, back, LOST
    tracking = state.copy()
    tracking[24] = TRACKING
    wild = state.copy()
    wild[1] = 16 * ONE
    far = state.copy()
    far[0:6], far[6:12] = mref.affine_pose(1, 0, 0, 1, 16380, 0)
    good = found_row(u=-3, v=2, sad=40, n=20, second=(5, 5, 400, 20))
    return [("accepted", good, state, 16, 800, RELOCATED), ("no runner-up", found_row(u=1, v=0, sad=0, n=7), state, 0, 1, RELOCATED),
            ("mean at the limit", found_row(u=0, v=0, sad=320, n=20), state, 16, 800, RELOCATED),
            ("mean over the limit", found_row(u=0, v=0, sad=321, n=20), state, 16, 800, REJECTED_MEAN),
            ("ratio at the limit", found_row(sad=40, n=20, second=(9, 0, 50, 20)), state, 16, 800, RELOCATED),
            ("ratio over the limit", found_row(sad=41, n=20, second=(9, 0, 50, 20)), state, 16, 800, REJECTED_UNIQUENESS),
            ("both zero", found_row(sad=0, n=20, second=(9, 0, 0, 20)), state, 16, 800, RELOCATED),
            ("no placement", found_row(FOUND_NONE, n=0), state, 16, 800, NO_PLACEMENT), ("bad geom", found_row(FOUND_BAD_GEOM, n=0), state, 16, 800, PATCH_REFUSED),
            ("a status that is none", found_row(9), state, 16, 800, PATCH_REFUSED), ("not lost", good, tracking, 16, 800, NOT_ATTEMPTED),
            ("state out of bounds", good, wild, 16, 800, PATCH_REFUSED), ("n of 0", found_row(n=0), state, 16, 800, PATCH_REFUSED),
            ("a sum over 255 n", found_row(sad=256, n=1), state, 255, 800, PATCH_REFUSED), ("a shift beyond the sides", found_row(u=16385), state, 16, 800, PATCH_REFUSED),
            ("a runner-up of no cells", found_row(second=(1, 1, 0, 0)), state, 16, 800, PATCH_REFUSED),
            ("past the pose bounds", found_row(u=2), far, 16, 800, OUT_OF_BOUNDS)]


def commit_cases():
    """(name, cand_state, cand_pose, correct_out, state, pose, found, status) for relocate_commit."""
    cases = []
    ok, no_fit = np.array([rref.OK, 20, 16, 4, 0, 0, 0, 0], np.int64), np.array([rref.NO_FIT, 3, 0, 0, 0, 0, 0, 0], np.int64)
    pose = np.array(mref.IDENTITY + mref.IDENTITY + [mref.POSE_LOST, 0, 9, 20], np.int64)
    for name, found, state, max_mean, ratio, decision in step_cases():
        cs, cp = relocate_step(found, state, s=4, max_mean=max_mean, ratio=ratio, **STEP_GEOMETRY)
        cases.append((name, cs, cp, ok, state, pose, found, decision))
        if decision == RELOCATED and name == "accepted":
            cases.append((name + ", no fine fit", cs, cp, no_fit, state, pose, found, FINE_FAILED))
            odd = cs.copy()
            odd[28] = 5
            cases.append((name + ", a decision that is none", odd, cp, ok, state, pose, found, PATCH_REFUSED))
            lost = cp.copy()
            lost[12] = mref.POSE_LOST
            cases.append((name + ", a lost candidate row", cs, lost, ok, state, pose, found, FINE_FAILED))
    return cases


# ------------------------------------------------------------------------------------------------ one lost frame, and the flight
def relocate_frame(img, state, pose, ordinal, rank, rgba, canvas_size, origin, s, settings=None, mask=None, coarse=map_coarse, patch=map_patch,
                   locate=map_locate, **refine):
    """The whole sequence for one frame -> (state, pose, out [8], (cl, cv, tl, tv, geom, found, cand_state, cand_pose, correct_out))."""
    k = dict(DEFAULTS, **(settings or {}))
    size = img.shape[:2]
    cl, cv = coarse(rgba, s)
    tl, tv, geom = patch(img, state, canvas_size, origin, s)
    found = locate(cl, cv, tl, tv, geom, k["min_overlap"], k["exclude"])
    cand_state, cand_pose = relocate_step(found, state, size, canvas_size, origin, s, k["max_mean"], k["ratio"])
    cand_state, cand_pose, correct_out, _ = rref.refine_frame(img, cand_pose, cand_state, ordinal, rank, rgba, canvas_size, origin, mask, **refine)
    state, pose, out = commit_step(cand_state, cand_pose, correct_out, state, pose, found, s)
    return state, pose, out, (cl, cv, tl, tv, geom, found, cand_state, cand_pose, correct_out)


def run_flight(images, pairs, canvas_size, origin, relocate=True, s=4, every=1, settings=None, mode="centre", **refine):
    """The loop FlowPredictor(mosaic_refine=True, mosaic_relocate=...) runs: refine_ref.run_flight's, and behind a frame's own registration
    the relocation sequence where the frame's ordinal is a multiple of `every` -> (poses [n, 16], refine outs [n, 8], relocate outs [n, 8],
    state, (rank, rgba))."""
    size = images[0].shape[:2]
    state = np.zeros(32, np.int64)
    rank, rgba = oref.canvas(canvas_size)
    poses, outs, relocs = [], [], []
    for f, img in enumerate(images):
        row, state = mref.pose_chain(np.asarray(pairs)[f:f + 1], state, size, canvas_size, origin)
        state, pose, out, _ = rref.refine_frame(img, row[0], state, f, rank, rgba, canvas_size, origin, **refine)
        reloc = np.array(NOT_ATTEMPTED_ROW, np.int64)
        if relocate and f % every == 0:
            state, pose, reloc, _ = relocate_frame(img, state, pose, f, rank, rgba, canvas_size, origin, s, settings, **refine)
        oref.ortho_accumulate(img, pose, f, rank, rgba, origin, mode)
        poses.append(pose)
        outs.append(out)
        relocs.append(reloc)
    return np.array(poses, np.int64), np.array(outs, np.int64), np.array(relocs, np.int64), state, (rank, rgba)


# ------------------------------------------------------------------------------------------------ the scenes
CUT_AT = 10


def cut_flight(after, bias=(0, 0)):
    """refine_ref.flight's frames: a pan of CUT_AT frames 4 px apart, then the offsets `after`; the pair of frame CUT_AT is flagged as a
    scene cut.  -> (images, pair models int64 [n, 16], true to_anchor translations in pixels)."""
    offsets = [rref.FLIGHT_STEP * f for f in range(CUT_AT)] + list(after)
    images, tables, true = rref.flight(offsets, bias=bias)
    pairs = np.concatenate([mref.global_motion([t], rref.FLIGHT_SIZE, rref.FLIGHT_SIZE, **mref.SCENE_SETTINGS) for t in tables])
    pairs[CUT_AT] = mref.model_row(mref.IDENTITY, mref.IDENTITY, mref.CUT, 0, 0, 0)
    return images, pairs, true


def revisit_after_cut():
    """The cut jumps 40 px back (beyond the matcher's 32) onto ground the first frames mapped, then pans on."""
    return cut_flight([rref.FLIGHT_STEP * f for f in range(4)])


def unmapped_after_cut():
    """The cut jumps to ground no frame has seen: another row band of the texture."""
    images, pairs, true = cut_flight([0, 4, 8])
    g = rref.ground()
    for f in range(CUT_AT, len(images)):
        images[f] = np.ascontiguousarray(g[64:128, 160 - 4 * (f - CUT_AT):256 - 4 * (f - CUT_AT)][::-1])
    return images, pairs, true


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def lost_state(to, back):
    state = np.zeros(32, np.int64)
    state[0:6], state[6:12], state[12:18], state[18:24] = to, back, mref.IDENTITY, mref.IDENTITY
    state[24], state[25], state[26] = LOST, 7, 1
    return state


def patch_states(mask_size):
    """(name, state): the identity; a whole-pixel shift that leaves the cell grid; a rotation of 3 degrees with zoom 1.04 (the bounding box is
    larger than the frame, its corner cells are invalid); a shift that pushes the patch partly off the canvas; and the refusals."""
    c, s = 1.04 * np.cos(np.radians(3)), 1.04 * np.sin(np.radians(3))
    tracking = lost_state(*mref.affine_pose(1, 0, 0, 1, 0, 0))
    tracking[24] = TRACKING
    wild = lost_state(*mref.affine_pose(1, 0, 0, 1, 0, 0))
    wild[4] = 16 * ONE
    return [("identity", lost_state(*mref.affine_pose(1, 0, 0, 1, 0, 0))), ("shifted", lost_state(*mref.affine_pose(1, 0, 0, 1, 7, -3))),
            ("rotated", lost_state(*mref.affine_pose(c, -s, s, c, 6, -4))), ("off the canvas", lost_state(*mref.affine_pose(1, 0, 0, 1, -45, 30))),
            ("not lost", tracking), ("out of bounds", wild), ("too wide", lost_state(*mref.affine_pose(6, 0, 0, 1, 0, 0))),
            ("no cell", lost_state([0, 0, 0, 0, 0, 0], mref.IDENTITY))]


def constant_canvas(size, value=90, hole=None):
    """A canvas seen everywhere with one grey: every placement ties.  hole = (y0, y1, x0, x1) unseen."""
    rank, rgba = oref.canvas(size)
    rgba[:] = np.uint32(value | value << 8 | value << 16 | 0xFF << 24)
    rank[:] = 0
    if hole:
        rgba[hole[0]:hole[1], hole[2]:hole[3]] = 0
    return rank, rgba


# ------------------------------------------------------------------------------------------------ the library's refusals
def good_arguments():
    """Per op the arguments of a call that passes validation (dummy non-null pointers), in the ABI's order, by name."""
    size = dict(H=128, W=192, CH=200, CW=300, ox=36, oy=54, S=8)
    return {
        "map_coarse": dict(rgba=64, CH=200, CW=300, S=8, cl=64, cv=64, stream=None),
        "map_patch": dict(frame=64, u=64, v=64, format=1, matrix=1, full_range=0, FH=256, FW=384, state=64, **size, tl=64, tv=64, geom=64, stream=None),
        "map_locate": dict(cl=64, cv=64, ch=25, cw=37, tl=64, tv=64, geom=64, min_overlap_permille=500, exclude=2, scores=64, found=64, stream=None),
        "pose_relocate": dict(found=64, state=64, cand_state=128, cand_pose=64, max_mean=16, ratio_permille=800, **size, stream=None),
        "relocate_commit": dict(cand_state=64, cand_pose=64, correct_out=64, state=128, pose=64, found=64, S=8, out=64, stream=None),
    }


def refusal_cases():
    """(op, changed arguments, a word of the message)."""
    coarse, patch, locate, step, commit = "map_coarse", "map_patch", "map_locate", "pose_relocate", "relocate_commit"
    cases = [(coarse, {p: None}, b"null") for p in ("rgba", "cl", "cv")]
    cases += [(coarse, dict(CH=0), b"0x"), (coarse, dict(CW=16385), b"16385"), (coarse, dict(S=5), b"S=5"), (coarse, dict(S=0), b"S=0"),
              (coarse, dict(CH=7), b"no cell"), (coarse, dict(CW=3, S=4), b"no cell"), (coarse, dict(rgba=66), b"aligned to 4")]
    cases += [(patch, {p: None}, b"null") for p in ("frame", "state", "tl", "tv", "geom", "u")]
    cases += [(patch, dict(format=2, v=None), b"null chroma"), (patch, dict(format=3), b"format"), (patch, dict(matrix=2), b"matrix"), (patch, dict(full_range=2), b"range"),
              (patch, dict(FH=0), b"0x"), (patch, dict(FW=16385), b"16385"), (patch, dict(H=0), b"0x"), (patch, dict(W=16385), b"16385"), (patch, dict(CH=0), b"canvas"),
              (patch, dict(CW=16385), b"canvas"), (patch, dict(ox=16385), b"origin"), (patch, dict(oy=-16385), b"origin"), (patch, dict(S=32), b"S=32"),
              (patch, dict(CH=15, S=16), b"no cell"), (patch, dict(state=68), b"aligned to 8"), (patch, dict(geom=68), b"aligned to 8")]
    cases += [(locate, {p: None}, b"null") for p in ("cl", "cv", "tl", "tv", "geom", "scores", "found")]
    cases += [(locate, dict(ch=0), b"0x"), (locate, dict(cw=4097), b"4097"), (locate, dict(min_overlap_permille=0), b"got 0"),
              (locate, dict(min_overlap_permille=1001), b"got 1001"), (locate, dict(exclude=-1), b"got -1"), (locate, dict(exclude=65), b"got 65"),
              (locate, dict(geom=68), b"aligned to 8"), (locate, dict(found=68), b"aligned to 8"), (locate, dict(scores=68), b"aligned to 8")]
    cases += [(step, {p: None}, b"null") for p in ("found", "state", "cand_state", "cand_pose")]
    cases += [(step, dict(max_mean=-1), b"got -1"), (step, dict(max_mean=256), b"got 256"), (step, dict(ratio_permille=0), b"got 0"),
              (step, dict(ratio_permille=1001), b"got 1001"), (step, dict(H=0), b"0x"), (step, dict(W=16385), b"16385"), (step, dict(CH=0), b"canvas"),
              (step, dict(ox=16385), b"origin"), (step, dict(S=2), b"S=2"), (step, dict(found=68), b"aligned to 8"), (step, dict(cand_pose=68), b"aligned to 8"),
              (step, dict(cand_state=64), b"the state itself")]
    cases += [(commit, {p: None}, b"null") for p in ("cand_state", "cand_pose", "correct_out", "state", "pose", "found", "out")]
    cases += [(commit, dict(S=12), b"S=12"), (commit, dict(out=68), b"aligned to 8"), (commit, dict(state=132), b"aligned to 8")]
    return cases


def call_op(lib, op, **changed):
    args = dict(good_arguments()[op])
    args.update(changed)
    return getattr(lib, "fs_" + op)(*args.values())
