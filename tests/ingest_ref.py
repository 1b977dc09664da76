"""CPU restatement of ops.prepare_frame (include/floodseg_test.h, frame_prepare) for the tests of the HIP route: plain numpy.

The YUV -> RGB conversion is integer (int32, arithmetic shift, clip), so it is defined bit for bit.  The resize repeats the float32
operation order of csrc/interp.h (lin_coord / bilerp, align_corners = 0): every product, sum and difference below is ONE numpy
operation on float32 operands, hence one float32 rounding each, with no contraction -- no library resize is called, whose rounding
would not be ours.  Then round half to even, clamp, (x - mean) / std in float32 (IEEE division).
"""
import numpy as np

MEAN = [0.485 * 255, 0.456 * 255, 0.406 * 255]
STD = [0.229 * 255, 0.224 * 255, 0.225 * 255]

# (matrix, full_range) -> (ymul, yoff, rv, gu, gv, bu):  c = ymul (Y - yoff), d = U - 128, e = V - 128,
# R = (c + rv e + 128) >> 8, G = (c - gu d - gv e + 128) >> 8, B = (c + bu d + 128) >> 8, each clipped to [0, 255]
COEF = {
    ("bt601", False): (298, 16, 409, 100, 208, 516),
    ("bt601", True): (256, 0, 359, 88, 183, 454),
    ("bt709", False): (298, 16, 459, 55, 136, 541),
    ("bt709", True): (256, 0, 403, 48, 120, 475),
}


def yuv_to_rgb(y, u, v, matrix="bt601", full_range=False):
    """uint8 arrays of one shape -> uint8 [..., 3]."""
    ymul, yoff, rv, gu, gv, bu = COEF[(matrix, bool(full_range))]
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    c, d, e = ymul * (y - yoff), u - 128, v - 128
    rgb = np.stack([(c + rv * e + 128) >> 8, (c - gu * d - gv * e + 128) >> 8, (c + bu * d + 128) >> 8], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def planes_to_rgb(y, u, v, matrix="bt601", full_range=False):
    """Y [H,W], U and V [ceil(H/2), ceil(W/2)] -> RGB [H,W,3]; luma pixel (y, x) takes chroma sample (y >> 1, x >> 1)."""
    h, w = y.shape
    assert u.shape == v.shape == ((h + 1) // 2, (w + 1) // 2)
    yy, xx = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    return yuv_to_rgb(y, u[yy, xx], v[yy, xx], matrix, full_range)


def lin_coord(out_size, in_size):
    """interp.h::lin_coord for every destination index, align_corners = 0: (i0, i1, w0, w1)."""
    f32 = np.float32
    scale = f32(in_size) / f32(out_size)
    dst = np.arange(out_size).astype(f32)
    src = scale * (dst + f32(0.5))
    src = src + f32(-0.5)
    src = np.where(src < 0, f32(0), src).astype(f32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    w1 = np.clip(src - i0.astype(f32), f32(0), f32(1)).astype(f32)
    w0 = f32(1) - w1
    assert src.dtype == w0.dtype == w1.dtype == f32
    return i0, i1, w0, w1


def resize_bilinear(img, size):
    """float32 [H,W,C] -> [h,w,C]: value = wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11), one rounding per operation."""
    img = img.astype(np.float32)
    y0, y1, wy0, wy1 = lin_coord(size[0], img.shape[0])
    x0, x1, wx0, wx1 = lin_coord(size[1], img.shape[1])
    wx0, wx1 = wx0[None, :, None], wx1[None, :, None]
    wy0, wy1 = wy0[:, None, None], wy1[:, None, None]
    top = wx0 * img[y0][:, x0] + wx1 * img[y0][:, x1]
    bot = wx0 * img[y1][:, x0] + wx1 * img[y1][:, x1]
    out = wy0 * top + wy1 * bot
    assert out.dtype == np.float32
    return out


def prepare_rgb(rgb, size=None, mean=MEAN, std=STD):
    """uint8 [H,W,3] -> float32 [1,3,h,w]."""
    x = rgb.astype(np.float32)
    if size is not None and tuple(size) != rgb.shape[:2]:
        x = np.clip(np.rint(resize_bilinear(x, size)), np.float32(0), np.float32(255)).astype(np.float32)
    x = (x - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(2, 0, 1))[None]


def prepare_yuv(y, u, v, size=None, matrix="bt601", full_range=False, mean=MEAN, std=STD):
    return prepare_rgb(planes_to_rgb(y, u, v, matrix, full_range), size, mean, std)
