"""CPU restatement of ops.compose_frame (include/floodseg_test.h, frame_compose) for the tests of the HIP route: plain numpy.

Everything here is integer (int32, arithmetic shift, integer division, clip) and hence defined bit for bit, except the resize of
the background, which is ingest_ref's restatement of interp.h (one float32 rounding per operation) -- the image the ingest tests
already hold equal to ops.prepare_frame on the GPU.
"""
import numpy as np

import ingest_ref

# (matrix, full_range) -> (yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb):
#   Y = ((yr R + yg G + yb B + 128) >> 8) + yoff, U = ((ur R + ug G + ub B + 128) >> 8) + 128, V likewise, each clipped to [0, 255]
COEF = {
    ("bt601", False): (66, 129, 25, 16, -38, -74, 112, 112, -94, -18),
    ("bt601", True): (77, 150, 29, 0, -43, -85, 128, 128, -107, -21),
    ("bt709", False): (47, 157, 16, 16, -26, -86, 112, 112, -102, -10),
    ("bt709", True): (54, 183, 19, 0, -29, -99, 128, 128, -116, -12),
}


def raw_frame_bytes(h, w, fmt):
    return h * w * 3 if fmt == "rgb24" else h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def background(frame, chroma=None, fmt="rgb24", matrix="bt601", full_range=False, size=None):
    """The uint8 image the network saw, [h,w,3]: frame_prepare's path up to but not including the normalisation."""
    if fmt == "rgb24":
        rgb = frame
    else:
        u, v = (chroma[..., 0], chroma[..., 1]) if fmt == "nv12" else chroma
        rgb = ingest_ref.planes_to_rgb(frame, u, v, matrix, full_range)
    if size is not None and tuple(size) != rgb.shape[:2]:
        x = np.clip(np.rint(ingest_ref.resize_bilinear(rgb.astype(np.float32), size)), np.float32(0), np.float32(255))
        assert x.dtype == np.float32
        rgb = x.astype(np.uint8)
    return rgb


def blend(mask, palette, bg=None):
    """uint8 mask [h,w], palette [K,4] (R, G, B, A), bg uint8 [h,w,3] or None -> uint8 [h,w,3]."""
    palette = np.asarray(palette)
    assert palette.dtype == np.uint8 and palette.ndim == 2 and palette.shape[1] == 4 and 1 <= palette.shape[0] <= 256
    c = np.where(mask < palette.shape[0], mask, 0).astype(np.int64)
    entry = palette[c].astype(np.int32)
    colour, a = entry[..., :3], entry[..., 3:]
    if bg is None:
        return colour.astype(np.uint8)
    o = (a * colour + (255 - a) * bg.astype(np.int32) + 127) // 255     # every term >= 0: floor == C's integer division
    assert o.min() >= 0 and o.max() <= 255
    return o.astype(np.uint8)


def rgb_to_y(rgb, matrix, full_range):
    yr, yg, yb, yoff = COEF[(matrix, bool(full_range))][:4]
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    return np.clip(((yr * r + yg * g + yb * b + 128) >> 8) + yoff, 0, 255).astype(np.uint8)


def rgb_to_uv(rgb, matrix, full_range):
    """(U, V) of int32 RGB values [..., 3], one sample per entry."""
    ur, ug, ub, vr, vg, vb = COEF[(matrix, bool(full_range))][4:]
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    u = np.clip(((ur * r + ug * g + ub * b + 128) >> 8) + 128, 0, 255).astype(np.uint8)
    v = np.clip(((vr * r + vg * g + vb * b + 128) >> 8) + 128, 0, 255).astype(np.uint8)
    return u, v


def quad_mean(rgb):
    """[h,w,3] uint8 -> int32 [ceil(h/2),ceil(w/2),3]: (sum of the 2 x 2 quad + 2) >> 2, rows / columns past the frame repeat the last one."""
    h, w = rgb.shape[:2]
    ys = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1)
    xs = np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    p = rgb[ys][:, xs].astype(np.int32)
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2


def pack(rgb, out_fmt="nv12", out_matrix="bt601", out_full_range=False):
    """The composed uint8 [h,w,3] picture as the bytes of one raw frame (flat uint8 array)."""
    if out_fmt == "rgb24":
        return np.ascontiguousarray(rgb).reshape(-1)
    y = rgb_to_y(rgb, out_matrix, out_full_range)
    u, v = rgb_to_uv(quad_mean(rgb), out_matrix, out_full_range)
    chroma = np.stack([u, v], axis=-1) if out_fmt == "nv12" else np.stack([u, v], axis=0)
    return np.concatenate([y.reshape(-1), chroma.reshape(-1)])


def compose(mask, palette, bg=None, out_fmt="nv12", out_matrix="bt601", out_full_range=False):
    """bg: the uint8 [h,w,3] image of background(), or None."""
    return pack(blend(mask, palette, bg), out_fmt, out_matrix, out_full_range)
