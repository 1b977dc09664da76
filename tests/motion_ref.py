"""CPU restatement of ops.block_match (include/floodseg_test.h, block_match) for the tests of the HIP route: plain numpy, one
full-frame absolute difference per candidate displacement, block sums by reshape, the selection rule of the definition literally.

  blocks 16 x 16, hb = H // 16, wb = W // 16; candidates |dx|, |dy| <= R whose window lies inside the reference frame;
  cost = SAD + penalty * (|dx| + |dy|); winner = lexicographic minimum of (cost, |dx| + |dy|, dy, dx);
  row = (-1, 16, 16, src_x, src_y, dst_x, dst_y), dst = block centre, src = dst + (dx, dy).

A test helper, not an oracle module.
"""
import numpy as np

BLOCK = 16


def luma(frame):
    """uint8 [H,W] as is; uint8 [H,W,3] RGB -> (77 R + 150 G + 29 B + 128) >> 8."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    if frame.ndim == 2:
        return frame
    assert frame.ndim == 3 and frame.shape[2] == 3
    f = frame.astype(np.int64)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).astype(np.uint8)


def block_match(cur, ref, search=16, penalty=0):
    """-> (table int32 [hb * wb, 7], cost int32 [hb * wb]), rows in block raster order."""
    cur, ref = luma(cur).astype(np.int32), luma(ref).astype(np.int32)
    assert cur.shape == ref.shape
    H, W = cur.shape
    assert H >= BLOCK and W >= BLOCK and 1 <= search <= 32 and 0 <= penalty <= 255
    hb, wb = H // BLOCK, W // BLOCK
    by, bx = np.meshgrid(np.arange(hb), np.arange(wb), indexing="ij")
    curb = cur[:hb * BLOCK, :wb * BLOCK]
    big = np.iinfo(np.int64).max
    best = np.full((4, hb, wb), big, dtype=np.int64)  # (cost, |dx| + |dy|, dy, dx)
    for dy in range(-search, search + 1):
        for dx in range(-search, search + 1):
            # the reference pixel under current pixel (y, x) is (y + dy, x + dx): shift the frame, out-of-frame pixels never count
            # because a block with any of them is not a candidate
            ys, xs = np.arange(hb * BLOCK) + dy, np.arange(wb * BLOCK) + dx
            shifted = ref[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)]
            sad = np.abs(curb - shifted).reshape(hb, BLOCK, wb, BLOCK).sum(axis=(1, 3)).astype(np.int64)
            valid = (by * BLOCK + dy >= 0) & (by * BLOCK + dy + BLOCK <= H) & (bx * BLOCK + dx >= 0) & (bx * BLOCK + dx + BLOCK <= W)
            mag = abs(dx) + abs(dy)
            cand = (sad + penalty * mag, np.full_like(sad, mag), np.full_like(sad, dy), np.full_like(sad, dx))
            less = np.zeros((hb, wb), dtype=bool)
            equal = np.ones((hb, wb), dtype=bool)
            for c, b in zip(cand, best):  # lexicographic <
                less |= equal & (c < b)
                equal &= c == b
            take = valid & less
            for c, b in zip(cand, best):
                b[take] = c[take]
    dst_x, dst_y = bx * BLOCK + BLOCK // 2, by * BLOCK + BLOCK // 2
    table = np.stack([np.full_like(bx, -1), np.full_like(bx, BLOCK), np.full_like(bx, BLOCK), dst_x + best[3], dst_y + best[2], dst_x, dst_y],
                     axis=-1).reshape(hb * wb, 7).astype(np.int32)
    return table, best[0].reshape(hb * wb).astype(np.int32)


def vectors(table):
    """(dx, dy) per block from a table."""
    table = np.asarray(table)
    return table[:, 3] - table[:, 5], table[:, 4] - table[:, 6]


def noise_frame(h, w, seed, channels=1):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(h, w) if channels == 1 else (h, w, channels)).astype(np.uint8)


def shifted_copy(frame, dx, dy, seed=0):
    """`cur` such that cur(y, x) = frame(y + dy, x + dx) wherever that lies inside the frame (fresh noise elsewhere): a block of cur
    whose source window is inside `frame` matches it at displacement (dx, dy) with SAD 0."""
    H, W = frame.shape[:2]
    out = noise_frame(H, W, seed + 7919, 1 if frame.ndim == 2 else frame.shape[2])
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    out[y0:y1, x0:x1] = frame[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out
