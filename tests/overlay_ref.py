"""CPU restatement of ops.compose_regions (include/floodseg_test.h, frame_compose_regions) for the tests of the HIP route: plain numpy.

Written to share no structure with the kernels: the outline test compares the row plane with its (2T + 1)^2 - 1 shifted copies under an
in-frame mask (no tile, no separable fold); the labels are painted by a Python loop over the live rows from glyphs held as strings
(no packed words, no per-pixel ink formula); ids are Python integers.  The base picture and the RGB -> YUV conversion are
egress_ref's, which the egress tests hold equal to ops.compose_frame.
"""
import numpy as np

import egress_ref

GLYPHS = {
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
}
HALO, INK = 1, 2


def workspace_bytes(h, w):
    return -(-h * w // 4) * 4


def rows_plane(index, R):
    """The index plane as the overlay sees it: values outside 0 .. R - 1 are -1."""
    index = np.asarray(index).astype(np.int64)
    return np.where((index >= 0) & (index < R), index, -1)


def row_ids(R, tracks=None):
    """Python ints: the id of every row."""
    return [int(tracks[r][0]) for r in range(R)] if tracks is not None else list(range(R))


def labels(h, w, R, table, counts, tracks, scale, min_area):
    """[(row, x0, y0, tw, th, text)] of the rows that get a label, in row order."""
    out = []
    if scale < 1:
        return out
    ids = row_ids(R, tracks)
    for r in range(min(int(counts[1]), R)):
        ident, area = ids[r], int(table[r][1])
        if ident < 0 or area < min_area:
            continue
        text = str(ident % 10 ** 7)
        tw, th = (6 * len(text) - 1) * scale, 7 * scale
        if w < tw + 2 * scale or h < th + 2 * scale:
            continue
        cx, cy = int(table[r][6]) // area, int(table[r][7]) // area
        x0 = min(max(cx - tw // 2, scale), w - tw - scale)
        y0 = min(max(cy - th // 2, scale), h - th - scale)
        out.append((r, x0, y0, tw, th, text))
    return out


def marks(h, w, boxes, scale):
    """The marks plane uint8 [h,w] of labels(): bit 0 inside a halo rectangle, bit 1 ink."""
    m = np.zeros((h, w), dtype=np.uint8)
    for _, x0, y0, tw, th, text in boxes:
        m[y0 - scale:y0 + th + scale, x0 - scale:x0 + tw + scale] |= HALO
        for k, ch in enumerate(text):
            for v, line in enumerate(GLYPHS[ch]):
                for col, cell in enumerate(line):
                    if cell == "#":
                        y, x = y0 + v * scale, x0 + (6 * k + col) * scale
                        m[y:y + scale, x:x + scale] |= INK
    return m


def boundary(rows, T):
    """bool [h,w]: some in-frame pixel within Chebyshev distance T holds another row."""
    h, w = rows.shape
    differ = np.zeros((h, w), dtype=bool)
    for dy in range(-T, T + 1):
        for dx in range(-T, T + 1):
            if (dy, dx) == (0, 0) or abs(dy) >= h or abs(dx) >= w:
                continue
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            differ[yd, xd] |= rows[ys, xs] != rows[yd, xd]     # the pixel at (yd, xd) against its neighbour at (+dy, +dx), both in the frame
    return differ


def over(a, colour, under):
    """(a * colour + (255 - a) * under + 127) // 255 on int64 arrays, every term >= 0."""
    return (a * colour + (255 - a) * under + 127) // 255


def picture(mask, palette, index, table=None, counts=None, tracks=None, fill_palette=None, outline=None, outline_width=1, label_scale=0,
            label_min_area=256, halo=(0, 0, 0, 160), ink=(255, 255, 255), bg=None, R=None):
    """The composed uint8 [h,w,3] picture.  bg: egress_ref.background()'s image or None.  R: max_regions (default: the table's / tracks' rows, else 65536)."""
    mask = np.asarray(mask)
    palette = np.asarray(palette)
    h, w = mask.shape
    if R is None:
        R = len(table) if table is not None else len(tracks) if tracks is not None else 65536
    rows = rows_plane(index, R)
    cls = np.where(mask < palette.shape[0], mask, 0).astype(np.int64)
    pal = palette.astype(np.int64)[cls]                                        # [h,w,4]
    colour, a = pal[..., :3].copy(), pal[..., 3:]
    if fill_palette is not None and len(fill_palette):
        fill = np.asarray(fill_palette).astype(np.int64)
        ids = row_ids(R, tracks)
        lut = np.array([fill[i % len(fill)] if i >= 0 else (-1, -1, -1) for i in ids], dtype=np.int64)   # per row; Python ints: any id size
        hit = (rows >= 0) & (lut[np.maximum(rows, 0)][..., 0] >= 0)
        colour[hit] = lut[rows[hit]]
    o = over(a, colour, bg.astype(np.int64)) if bg is not None else colour
    if outline is not None and outline_width >= 1:
        line = np.asarray(outline).astype(np.int64)[cls]
        drawn = boundary(rows, outline_width) & (rows >= 0) & (line[..., 3] > 0)
        o = np.where(drawn[..., None], over(line[..., 3:], line[..., :3], o), o)
    if label_scale >= 1:
        m = marks(h, w, labels(h, w, R, np.asarray(table), np.asarray(counts), None if tracks is None else np.asarray(tracks), label_scale,
                               label_min_area), label_scale)
        hc, ha = np.array(halo[:3], dtype=np.int64), int(halo[3])
        o = np.where(((m & HALO) != 0)[..., None], over(ha, hc, o), o)
        o = np.where(((m & INK) != 0)[..., None], np.array(ink, dtype=np.int64), o)
    assert o.min() >= 0 and o.max() <= 255
    return o.astype(np.uint8)


def compose(mask, palette, index, out_fmt="nv12", out_matrix="bt601", out_full_range=False, **layers):
    """The bytes of one raw frame (flat uint8 array), as ops.compose_regions writes them."""
    return egress_ref.pack(picture(mask, palette, index, **layers), out_fmt, out_matrix, out_full_range)
