"""CPU restatement of ops.block_match_modes (include/floodseg_test.h, block_match_modes) on top of tests/motion_ref.py's brute-force
search: the winner is motion_ref.block_match's, and this file adds the two decisions of the definition literally.

  activity = sum |Y - m| over the block, m = (S + 128) >> 8, S = the block's luma sum        (0..32640)
  sad      = winning cost - penalty * (|dx| + |dy|)
  intra    = sad > activity + intra_bias
  cut      = intra_blocks * 1000 > cut_permille * blocks
  an intra block's row -- on a cut every row -- is the void row (-1, 16, 16, -16, -16, -16, -16)

A test helper, not an oracle module.
"""
import numpy as np

import motion_ref

BLOCK = motion_ref.BLOCK
VOID_ROW = (-1, 16, 16, -16, -16, -16, -16)


def permille(scene_cut):
    """The Python surface's mapping: a fraction in [0, 1] -> per-mille with round(); None -> 1000 (never a cut)."""
    return 1000 if scene_cut is None else int(round(float(scene_cut) * 1000))


def block_activity(cur):
    """int32 [hb * wb]: the DC-intra cost of every 16 x 16 block of the frame's luma."""
    y = motion_ref.luma(cur).astype(np.int64)
    hb, wb = y.shape[0] // BLOCK, y.shape[1] // BLOCK
    blocks = y[:hb * BLOCK, :wb * BLOCK].reshape(hb, BLOCK, wb, BLOCK).transpose(0, 2, 1, 3).reshape(hb * wb, BLOCK * BLOCK)
    m = (blocks.sum(axis=1) + 128) >> 8
    return np.abs(blocks - m[:, None]).sum(axis=1).astype(np.int32)


def decide(table, cost, activity, penalty, intra_bias=65535, cut_permille=1000):
    """The two rules on a winners' table (motion_ref.block_match's) -> (table with void rows, stats int32 [4])."""
    assert 0 <= intra_bias <= 65535 and 0 <= cut_permille <= 1000
    dx, dy = motion_ref.vectors(table)
    sad = cost.astype(np.int64) - penalty * (np.abs(dx) + np.abs(dy))
    intra = sad > activity.astype(np.int64) + intra_bias
    blocks, n_intra = len(cost), int(intra.sum())
    cut = n_intra * 1000 > cut_permille * blocks
    table = table.copy()
    table[np.ones_like(intra) if cut else intra] = VOID_ROW
    return table, np.array([blocks, n_intra, int(cut), 0], dtype=np.int32)


def block_match_modes(cur, ref, search=16, penalty=0, intra_bias=65535, cut_permille=1000):
    """-> (table int32 [hb * wb, 7], cost int32 [hb * wb], activity int32 [hb * wb], stats int32 [4])."""
    winners, cost = motion_ref.block_match(cur, ref, search, penalty)
    activity = block_activity(cur)
    table, stats = decide(winners, cost, activity, penalty, intra_bias, cut_permille)
    return table, cost, activity, stats


def is_void(table):
    return (np.asarray(table) == np.array(VOID_ROW)).all(axis=1)


# ---- the synthetic scenes of the tests, deterministic, luma or RGB.  The scene is a DARK texture (0..127) and whatever is unrelated to it
# a BRIGHT one (128..255): activity does not see a block's mean level and a SAD does, so a block's true match (SAD 0) lies far below
# its activity (thousands) and the best of any number of wrong matches (>= 256 x the difference of the block means) far above it.
# (Two textures of ONE range do not do: the best of 289 wrong candidates often beats the block's own activity.)
DARK, BRIGHT = (0, 128), (128, 256)


def textured_frame(h, w, seed, channels=1, levels=DARK):
    """Band-limited texture: noise in `levels` on an 8-pixel lattice, bilinearly enlarged, plus a little per-pixel noise."""
    rng = np.random.RandomState(seed)
    shape = (h // 8 + 2, w // 8 + 2) + (() if channels == 1 else (channels,))
    coarse = rng.randint(levels[0], levels[1], size=shape).astype(np.float64)
    yy, xx = np.arange(h) / 8.0, np.arange(w) / 8.0
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = (yy - y0), (xx - x0)
    if channels != 1:
        fy, fx = fy[:, None, None], fx[None, :, None]
    else:
        fy, fx = fy[:, None], fx[None, :]
    top = coarse[y0][:, x0] * (1 - fx) + coarse[y0][:, x0 + 1] * fx
    bot = coarse[y0 + 1][:, x0] * (1 - fx) + coarse[y0 + 1][:, x0 + 1] * fx
    img = top * (1 - fy) + bot * fy + rng.randint(-3, 4, size=top.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def translated_pair(h, w, dx, dy, seed, channels=1):
    """(cur, ref): cur(y, x) = ref(y + dy, x + dx) everywhere -- both are windows of one larger textured canvas.  A block has its
    true match among the candidates when its window at (dx, dy) lies inside the frame; with dx, dy >= 0 and no larger than the
    frame's remainder strips (H % 16, W % 16) that holds for EVERY block."""
    m = 40
    canvas = textured_frame(h + 2 * m, w + 2 * m, seed, channels)
    ref = np.ascontiguousarray(canvas[m:m + h, m:m + w])
    cur = np.ascontiguousarray(canvas[m + dy:m + dy + h, m + dx:m + dx + w])
    return cur, ref


def occluded_pair(h, w, dx, dy, seed, channels=1, rect=None):
    """The translated pair with a rectangle of cur (default: the middle third, block aligned where the frame allows) replaced by
    unrelated texture: blocks inside it have no match in ref."""
    cur, ref = translated_pair(h, w, dx, dy, seed, channels)
    if rect is None:
        y0, x0 = (h // 3) // BLOCK * BLOCK, (w // 3) // BLOCK * BLOCK
        rect = (y0, x0, max(y0 + BLOCK, (2 * h // 3) // BLOCK * BLOCK), max(x0 + BLOCK, (2 * w // 3) // BLOCK * BLOCK))
    y0, x0, y1, x1 = rect
    other = textured_frame(h, w, seed + 1000, channels, BRIGHT)
    cur = cur.copy()
    cur[y0:y1, x0:x1] = other[y0:y1, x0:x1]
    return cur, ref


def unrelated_pair(h, w, seed, channels=1):
    return textured_frame(h, w, seed, channels), textured_frame(h, w, seed + 2000, channels, BRIGHT)
