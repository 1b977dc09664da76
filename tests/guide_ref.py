"""CPU restatement of ops.guide_vectors (include/floodseg_test.h, guide_vectors; csrc/guide_defs.h) for the tests of the HIP route: the
definition twice, vectorised on int64 numpy arrays (guide_vectors) and as literal loops over Python integers (guide_vectors_loop), plus
the tables, models and frames the tests share.  Integers throughout: every comparison with it is exact equality.

A test helper, not an oracle module.
"""
import numpy as np

import mosaic_ref as mref
import motion_ref

ONE, HALF = mref.ONE, mref.HALF
VOID_ROW = mref.VOID_ROW
MAX_VECTOR = 32
ROW_VOID, ROW_FOREIGN, ROW_VECTOR = 0, 1, 2
COPY, FILL, REPLACE, DROP, KEEP = 0, 1, 2, 3, 4
COUNTS = ("blocks", "void_in", "filled", "outliers", "replaced", "dropped", "kept", "foreign")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def outlier_q20(outlier):
    """Pixels -> Q20 as ops.guide_vectors converts `outlier` (None: off = -1)."""
    return -1 if outlier is None else int(round(float(outlier) * ONE))


# ------------------------------------------------------------------------------------------------ the rules on Python integers
def pair_guides(M):
    M = [int(v) for v in M]
    return M[12] == 0 and mref.pair_in_bounds(M[:6], M[6:12])


def predict(M, cx, cy):
    """(gx, gy, pdx, pdy) at the block centre; only for a pair that guides."""
    M = [int(v) for v in M]
    CX, CY = cx * ONE, cy * ONE
    gx = mref.rshr(M[0] * CX + M[1] * CY) + M[2] - CX
    gy = mref.rshr(M[3] * CX + M[4] * CY) + M[5] - CY
    return gx, gy, mref.rshr(gx), mref.rshr(gy)


def available(pdx, pdy, cx, cy, fh, fw):
    if abs(pdx) > MAX_VECTOR or abs(pdy) > MAX_VECTOR:
        return False
    x0, y0 = cx - 8 + pdx, cy - 8 + pdy
    return x0 >= 0 and y0 >= 0 and x0 + 16 <= fw and y0 + 16 <= fh


def classify(r, cx, cy):
    """(class, dx, dy) of a row of the block centred at (cx, cy)."""
    r = [int(v) for v in r]
    if r[3] < 0 or r[5] < 0 or r[6] < 0:
        return ROW_VOID, 0, 0
    ex, ey = r[3] - r[5], r[4] - r[6]
    if (r[5], r[6]) != (cx, cy) or abs(ex) > MAX_VECTOR or abs(ey) > MAX_VECTOR:
        return ROW_FOREIGN, 0, 0
    return ROW_VECTOR, ex, ey


def is_outlier(dx, dy, gx, gy, oq):
    return oq >= 0 and (abs(dx * ONE - gx) > oq or abs(dy * ONE - gy) > oq)


def block_sad(cur, ref, cx, cy, pdx, pdy):
    """SAD of the block of `cur` (luma) centred at (cx, cy) against the window of `ref` displaced by (pdx, pdy)."""
    a = cur[cy - 8:cy + 8, cx - 8:cx + 8].astype(np.int64)
    b = ref[cy - 8 + pdy:cy + 8 + pdy, cx - 8 + pdx:cx + 8 + pdx].astype(np.int64)
    return int(np.abs(a - b).sum())


def decide_row(r, M, guided, cx, cy, fh, fw, fill_void, oq, evidence):
    """One row -> (decision, output row, outlier?, class).  evidence: None or a function (pdx, pdy) -> replaces?"""
    cls, dx, dy = classify(r, cx, cy)
    void = list(VOID_ROW)
    if not guided or cls == ROW_FOREIGN:
        return COPY, [int(v) for v in r], False, cls
    gx, gy, pdx, pdy = predict(M, cx, cy)
    avail = available(pdx, pdy, cx, cy, fh, fw)
    guide = [-1, 16, 16, cx + pdx, cy + pdy, cx, cy]
    if cls == ROW_VOID:
        return (FILL, guide, False, cls) if fill_void and avail else (COPY, [int(v) for v in r], False, cls)
    if not is_outlier(dx, dy, gx, gy, oq):
        return COPY, [int(v) for v in r], False, cls
    if not avail:
        return DROP, void, True, cls
    if evidence is None or evidence(pdx, pdy):
        return REPLACE, guide, True, cls
    return KEEP, [int(v) for v in r], True, cls


def guide_vectors_loop(mv, model, fh, fw, fill_void=1, oq=-1, cur=None, ref=None, cost=None, penalty=0, guide_bias=0):
    """The definition as literal loops over Python integers -> (out int32 [n, blocks, 7], counts int64 [n, 8])."""
    mv, model = np.asarray(mv), np.asarray(model)
    n, blocks = mv.shape[:2]
    hb, wb = fh // 16, fw // 16
    assert blocks == hb * wb and model.shape == (n, 16)
    assert (cur is None) == (ref is None) == (cost is None)
    out = np.empty_like(mv)
    counts = np.zeros((n, 8), np.int64)
    for f in range(n):
        M = [int(v) for v in model[f]]
        guided = pair_guides(M)
        lc, lr = (motion_ref.luma(cur[f]), motion_ref.luma(ref[f])) if cur is not None else (None, None)
        for i in range(blocks):
            cx, cy = 16 * (i % wb) + 8, 16 * (i // wb) + 8
            evidence = None
            if cur is not None:
                def evidence(pdx, pdy, cx=cx, cy=cy, i=i):
                    cost_g = block_sad(lc, lr, cx, cy, pdx, pdy) + penalty * (abs(pdx) + abs(pdy))
                    return cost_g <= int(cost[f][i]) + guide_bias
            decision, row, outlier, cls = decide_row(mv[f, i], M, guided, cx, cy, fh, fw, fill_void, oq, evidence)
            out[f, i] = row
            counts[f, 0] += 1
            counts[f, 1] += cls == ROW_VOID
            counts[f, 7] += cls == ROW_FOREIGN
            counts[f, 3] += outlier
            for col, d in ((2, FILL), (4, REPLACE), (5, DROP), (6, KEEP)):
                counts[f, col] += decision == d
    return out, counts


# ------------------------------------------------------------------------------------------------ the same, vectorised
def centres(fh, fw):
    hb, wb = fh // 16, fw // 16
    i = np.arange(hb * wb, dtype=np.int64)
    return 16 * (i % wb) + 8, 16 * (i // wb) + 8


def guide_cost(cur, ref, fh, fw, pdx, pdy, avail, penalty):
    """cost_g int64 [blocks] where avail (0 elsewhere) of one pair: luma frames, per-block displacements."""
    cx, cy = centres(fh, fw)
    yy, xx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    out = np.zeros(len(cx), np.int64)
    idx = np.flatnonzero(avail)
    ys, xs = (cy[idx] - 8)[:, None, None] + yy, (cx[idx] - 8)[:, None, None] + xx
    a = cur[ys, xs].astype(np.int64)
    b = ref[ys + pdy[idx][:, None, None], xs + pdx[idx][:, None, None]].astype(np.int64)
    out[idx] = np.abs(a - b).sum(axis=(1, 2)) + penalty * (np.abs(pdx[idx]) + np.abs(pdy[idx]))
    return out


def guide_vectors(mv, model, fh, fw, fill_void=1, oq=-1, cur=None, ref=None, cost=None, penalty=0, guide_bias=0):
    """The definition on int64 arrays -> (out int32 [n, blocks, 7], counts int64 [n, 8])."""
    mv, model = np.asarray(mv), np.asarray(model).astype(np.int64)
    n, blocks = mv.shape[:2]
    cx, cy = centres(fh, fw)
    assert blocks == len(cx) and model.shape == (n, 16)
    out = mv.copy()
    counts = np.zeros((n, 8), np.int64)
    for f in range(n):
        r = mv[f].astype(np.int64)
        void = (r[:, 3] < 0) | (r[:, 5] < 0) | (r[:, 6] < 0)
        ex, ey = r[:, 3] - r[:, 5], r[:, 4] - r[:, 6]
        foreign = ~void & ((r[:, 5] != cx) | (r[:, 6] != cy) | (np.abs(ex) > MAX_VECTOR) | (np.abs(ey) > MAX_VECTOR))
        vector = ~void & ~foreign
        counts[f, 0], counts[f, 1], counts[f, 7] = blocks, void.sum(), foreign.sum()
        if not pair_guides(model[f]):
            continue
        M = model[f]
        CX, CY = cx * ONE, cy * ONE
        gx = ((M[0] * CX + M[1] * CY + HALF) >> 20) + M[2] - CX
        gy = ((M[3] * CX + M[4] * CY + HALF) >> 20) + M[5] - CY
        pdx, pdy = (gx + HALF) >> 20, (gy + HALF) >> 20
        x0, y0 = cx - 8 + pdx, cy - 8 + pdy
        avail = (np.abs(pdx) <= MAX_VECTOR) & (np.abs(pdy) <= MAX_VECTOR) & (x0 >= 0) & (y0 >= 0) & (x0 + 16 <= fw) & (y0 + 16 <= fh)
        outlier = vector & (oq >= 0) & ((np.abs(ex * ONE - gx) > oq) | (np.abs(ey * ONE - gy) > oq))
        fill = void & bool(fill_void) & avail
        drop = outlier & ~avail
        replace = outlier & avail
        if cur is not None:
            cost_g = guide_cost(motion_ref.luma(cur[f]), motion_ref.luma(ref[f]), fh, fw, pdx, pdy, replace, penalty)
            replace = replace & (cost_g <= np.asarray(cost[f]).astype(np.int64) + guide_bias)
        keep = outlier & avail & ~replace
        guide = np.stack([np.full_like(cx, -1), np.full_like(cx, 16), np.full_like(cx, 16), cx + np.where(avail, pdx, 0), cy + np.where(avail, pdy, 0), cx, cy], axis=1)
        take = fill | replace
        out[f][take] = guide[take].astype(np.int32)
        out[f][drop] = VOID_ROW
        counts[f, 2:7] = fill.sum(), outlier.sum(), replace.sum(), drop.sum(), keep.sum()
    return out, counts


# ------------------------------------------------------------------------------------------------ models and tables the tests share
def model_of(fwd, status=0, inv=None):
    """One model row from a forward affine of six Q20 integers; the inverse is the exact one of a pure shift, else the identity's
    (guide_vectors reads the inverse for the bounds test alone)."""
    fwd = [int(v) for v in fwd]
    if inv is None:
        inv = [ONE, 0, -fwd[2], 0, ONE, -fwd[5]] if fwd[0] == ONE and fwd[4] == ONE and fwd[1] == 0 and fwd[3] == 0 else list(mref.IDENTITY)
    return mref.model_row(fwd, inv, status, 0, 0, 0)


def shift_model(dx, dy, status=0):
    return model_of([ONE, 0, dx * ONE, 0, ONE, dy * ONE], status)


def rotation_model(fh, fw, degrees=1.5, zoom=1.02):
    """A rotation with zoom about the frame centre: pdx and pdy change sign across the grid."""
    c, s = zoom * np.cos(np.radians(degrees)), zoom * np.sin(np.radians(degrees))
    mx, my = fw / 2.0, fh / 2.0
    q = lambda v: int(round(v * ONE))  # noqa: E731
    return model_of([q(c), q(-s), q(mx - c * mx + s * my), q(s), q(c), q(my - s * mx - c * my)])


def garbage_model():
    """A status-0 row far outside the pair bounds: it must be refused before any product is formed."""
    return [(1 << 62), -(1 << 62), (1 << 62), (1 << 61), I32_MAX << 30, -(1 << 63)] * 2 + [0, 0, 0, 0]


def models(fh, fw):
    """name -> one model row: the cases of the issue."""
    return {
        "identity": shift_model(0, 0),
        "shift": shift_model(3, -2),
        "shift40": shift_model(40, 0),
        "rotation": rotation_model(fh, fw),
        "cut": shift_model(3, -2, status=1),
        "few": shift_model(3, -2, status=2),
        "degenerate": shift_model(3, -2, status=3),
        "garbage": garbage_model(),
    }


def model_table(M, fh, fw):
    """The table that consists of the rounded model vectors (a matcher-shaped row for every block, available or not)."""
    cx, cy = centres(fh, fw)
    t = np.empty((len(cx), 7), np.int64)
    t[:, 0], t[:, 1], t[:, 2], t[:, 5], t[:, 6] = -1, 16, 16, cx, cy
    for i in range(len(cx)):
        _, _, pdx, pdy = predict(M, int(cx[i]), int(cy[i]))
        t[i, 3], t[i, 4] = cx[i] + pdx, cy[i] + pdy
    return t.astype(np.int32)


def adversarial_table(M, fh, fw, seed):
    """A table for model row M that holds every kind of row: the model's vectors, void rows (the matcher's and half-void ones), foreign
    rows (another block's centre, vectors of +-33), INT32_MIN / INT32_MAX garbage, vectors of exactly +-32 and random vectors."""
    rng = np.random.RandomState(seed)
    cx, cy = centres(fh, fw)
    t = model_table(M, fh, fw).astype(np.int64) if pair_guides(M) else mref.grid_table(fh // 16, fw // 16, lambda x, y: (0 * x, 0 * y)).astype(np.int64)
    kinds = rng.randint(0, 12, size=len(cx))   # 8..11: the model's own vector stays
    for i, k in enumerate(kinds):
        x, y = int(cx[i]), int(cy[i])
        if k == 0:                                           # the matcher's void row
            t[i] = VOID_ROW
        elif k == 1:                                         # void by ONE negative word, the others plausible
            t[i, (3, 5, 6)[rng.randint(3)]] = -1 - rng.randint(20)
        elif k == 2:                                         # foreign: another block's centre
            t[i, 5 + rng.randint(2)] += 16
        elif k == 3:                                         # foreign: a component of exactly +-33
            t[i, 3], t[i, 4] = x, y
            t[i, 3 + rng.randint(2)] += (33, -33)[rng.randint(2)]
        elif k == 4:                                         # extreme words
            t[i] = rng.choice([I32_MIN, I32_MAX, 0, -1, 8], size=7)
        elif k == 5:                                         # exactly +-32: still a vector
            t[i, 3], t[i, 4] = x + (32, -32)[rng.randint(2)], y + (32, -32)[rng.randint(2)]
        elif k == 6:                                         # any vector the matcher could have found
            t[i, 3], t[i, 4] = x + rng.randint(-32, 33), y + rng.randint(-32, 33)
        elif k == 7:                                         # seven random ints
            t[i] = rng.randint(I32_MIN, I32_MAX, size=7, dtype=np.int64)
    return t.astype(np.int32)


def deviation_case(fh, fw, oq):
    """(model, table): a translation model whose Q20 shift makes block vectors deviate by EXACTLY oq and by oq + 1 from the camera's.
    The model is a shift of (2 ONE + oq, -ONE - oq - 1) in Q20: the vector (2, -1) deviates by oq in x (no outlier there) and by oq + 1
    in y (an outlier); the vector (2, -1) with the model's y shift lowered by one deviates by oq in both."""
    outl = model_of([ONE, 0, 2 * ONE + oq, 0, ONE, -ONE - oq - 1], inv=list(mref.IDENTITY))
    edge = model_of([ONE, 0, 2 * ONE + oq, 0, ONE, -ONE - oq], inv=list(mref.IDENTITY))
    table = mref.grid_table(fh // 16, fw // 16, lambda x, y: (0 * x + 2, 0 * y - 1))
    return outl, edge, table


# ------------------------------------------------------------------------------------------------ frames for the evidence mode
def evidence_scene(fh, fw, channels, pan=(3, -2), patch_block=(1, 4), patch_vector=(-5, 4), seed=3):
    """(cur, ref): textured ground that pans by `pan` (cur(y, x) = ref(y + pan_y, x + pan_x), motion_ref.shifted_copy), one block of
    which (patch_block = (by, bx)) shows a textured patch that moves by patch_vector instead, against the pan; and one CONSTANT block,
    (by, bx) = (2, 1), grey in both frames wherever it could have come from."""
    ref = motion_ref.noise_frame(fh, fw, seed, channels)
    ref[24:24 + 36, 8:8 + 36] = 100                       # the flat patch and every window the search or the guide can reach from it
    cur = motion_ref.shifted_copy(ref, pan[0], pan[1], seed)
    by, bx = patch_block
    y, x = 16 * by, 16 * bx
    cur[y:y + 16, x:x + 16] = ref[y + patch_vector[1]:y + 16 + patch_vector[1], x + patch_vector[0]:x + 16 + patch_vector[0]]
    cur[32:48, 16:32] = 100
    return cur, ref


def flat_scene(fh, fw, pan=(20, 0), rect=(16, 16, 48, 48), seed=5, level=100, noise=3):
    """(cur, ref) luma: textured ground panning by pan = (dx, dy) (cur(y, x) = ref(y + dy, x + dx)) with a flat, noisy rectangle rect =
    (y0, x0, y1, x1) of cur (block-aligned) that is water in both frames: the level with independent +-noise in each frame, so the winner's
    SAD exceeds the blocks' activity and intra_bias = 0 makes its rows void.  Every other block of cur matches ref at the pan with SAD 0."""
    rng = np.random.RandomState(seed)
    y0, x0, y1, x1 = rect
    ref = motion_ref.noise_frame(fh, fw, seed, 1)
    ref[y0 + pan[1]:y1 + pan[1], x0 + pan[0]:x1 + pan[0]] = level + rng.randint(-noise, noise + 1, size=(y1 - y0, x1 - x0))
    cur = motion_ref.shifted_copy(ref, pan[0], pan[1], seed)
    cur[y0:y1, x0:x1] = level + rng.randint(-noise, noise + 1, size=(y1 - y0, x1 - x0))
    return cur, ref
