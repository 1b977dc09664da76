"""numpy restatement of the confidence and extent-report definitions (include/floodseg_test.h: mask_confidence, canvas_confidence,
frame_report), and the inputs the CPU and GPU tests share.

Logits: the align_corners=True bilinear values are formed in float32 with the index and weight arithmetic of csrc/interp.h (the way
tests/multiscale_ref.py forms its resizes: clamped taps, the weight of the second tap, top / bottom rows, then the column blend; the
arithmetic runs in the given dtype), the softmax over them in float64.  Canvas and report: exact arithmetic (float64 products and
rint as the definition states them; integers)."""
import numpy as np

f32 = np.float32


def ac_taps(dst, src, dtype):
    """align_corners=True, per destination index: (i0, i1, w1) -- clamped taps and the weight of the second, in `dtype`."""
    scale = (dtype(src - 1) / dtype(dst - 1)) if dst > 1 else dtype(0)
    pos = (scale * np.arange(dst).astype(dtype)).astype(dtype)
    i0 = np.minimum(pos.astype(np.int64), src - 1)
    i1 = np.minimum(i0 + 1, src - 1)
    w1 = np.clip((pos - i0.astype(dtype)).astype(dtype), dtype(0), dtype(1))
    return i0, i1, w1


def resize_ac(x, new_h, new_w, dtype):
    """[n,K,h,w] -> [n,K,new_h,new_w], align_corners=True, every product and sum rounded to `dtype`."""
    x = np.asarray(x).astype(dtype)
    y0, y1, wy = ac_taps(new_h, x.shape[2], dtype)
    x0, x1, wx = ac_taps(new_w, x.shape[3], dtype)
    wx1, wy1 = wx[None, None, None, :], wy[None, None, :, None]
    wx0, wy0 = dtype(1) - wx1, dtype(1) - wy1
    with np.errstate(invalid="ignore", over="ignore"):
        top = wx0 * x[:, :, y0][:, :, :, x0] + wx1 * x[:, :, y0][:, :, :, x1]
        bot = wx0 * x[:, :, y1][:, :, :, x0] + wx1 * x[:, :, y1][:, :, :, x1]
        return wy0 * top + wy1 * bot


def first_max(v, from_class0):
    """The first maximum over axis 1.  from_class0 (fs_argmax_u8's rule): class 0 until a later value exceeds it; else
    fs_resize_argmax_u8's / fs_canvas_resize_argmax's: the first value above -inf that nothing later exceeds, 0 when there is none."""
    n, k, h, w = v.shape
    best = v[:, 0].copy() if from_class0 else np.full((n, h, w), -np.inf, dtype=v.dtype)
    arg = np.zeros((n, h, w), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for c in range(0 if not from_class0 else 1, k):
            take = v[:, c] > best
            best = np.where(take, v[:, c], best)
            arg[take] = c
    return arg


def logits_values(logits, size=None):
    """The values v[k] of mask_confidence (float32) and whether the equal-size rule applies."""
    logits = np.asarray(logits, dtype=f32)
    same = size is None or tuple(size) == logits.shape[2:]
    return (logits if same else resize_ac(logits, size[0], size[1], f32)), same


def mask_confidence(logits, size=None):
    """(mask uint8, confidence as float64 BEFORE rounding is applied: codes float64 in 0..255) -> (mask, conf uint8)."""
    v, same = logits_values(logits, size)
    mask = first_max(v, same)
    v64 = v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(v64 - np.fmax.reduce(v64, axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    c = np.take_along_axis(p, mask[:, None].astype(np.int64), axis=1)[:, 0]
    return mask, code(c)


def code(c):
    """c == c ? clamp(rint(255 c), 0, 255) : 0, in float64."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(c), 0.0, np.clip(np.rint(255.0 * c), 0.0, 255.0)).astype(np.uint8)


def canvas_confidence(canvas, size=None):
    canvas = np.asarray(canvas, dtype=np.float64)
    size = canvas.shape[2:] if size is None else size
    v = resize_ac(canvas, size[0], size[1], np.float64)   # at equal sizes too: weights 1 and 0, as fs_canvas_resize_argmax evaluates it
    mask = first_max(v, False)
    return mask, code(np.take_along_axis(v, mask[:, None].astype(np.int64), axis=1)[:, 0])


def frame_report(mask, conf=None, classes=5, low=128):
    mask = np.asarray(mask)
    out = np.zeros((mask.shape[0], classes, 3), dtype=np.int64)
    for f in range(mask.shape[0]):
        for k in range(classes):
            sel = mask[f] == k
            out[f, k, 0] = sel.sum()
            if conf is not None:
                out[f, k, 1] = conf[f][sel].astype(np.int64).sum()
                out[f, k, 2] = (conf[f][sel] < low).sum()
    return out


# ---------------------------------------------------------------------------------------------------- shared inputs
# (n, K, (h, w), (H, W)): a single pixel; two classes; resizes to odd sizes (more than one 256-pixel workgroup column at 65 x 65 is
# not reached, more than one row always is); the boundaries of the two register forms (K = 8 | 9, 32); widths not divisible by 4
GEOMETRIES = [(1, 1, (1, 1), (1, 1)), (2, 2, (3, 5), (3, 5)), (3, 5, (17, 19), (33, 47)), (5, 5, (23, 29), (65, 65)),
              (2, 8, (17, 19), (17, 19)), (2, 9, (17, 19), (17, 19)), (2, 19, (17, 19), (17, 19)), (2, 32, (17, 19), (17, 19)),
              (2, 5, (9, 12), (9, 12)), (2, 5, (7, 6), (13, 300))]   # + the dword-store path (W % 4 == 0), equal sizes and resized, W > 256
AMPLITUDES = (1.0, 30.0, 88.0)
SEED = 1234


def make_logits(n, k, hw, amp, seed=SEED):
    """Noise x amp with ties (a block of equal logits; a pair of equal maxima) and, on maps large enough, one NaN in a class > 0 and
    one in class 0."""
    rng = np.random.default_rng(seed + 17 * k + hw[0])
    x = (rng.standard_normal((n, k) + tuple(hw)) * amp).astype(f32)
    if hw[0] >= 3 and hw[1] >= 3:
        x[0, :, 0, :2] = f32(0.25)                       # all classes equal: mask 0, rint(255 / K)
        if k > 1:
            x[-1, :, 1, 1] = f32(-1.0)
            x[-1, [0, k - 1], 1, 1] = f32(2.0)           # two equal maxima: the first wins
            x[0, k - 1, 2, 2] = np.nan
            x[-1, 0, 2, 0] = np.nan
    return x


def make_canvas(n, k, hw, seed=SEED):
    """Mean probabilities as the crop canvas holds them (float64 softmax of noise), with an exact tie and a NaN."""
    rng = np.random.default_rng(seed + 5 * k + hw[1])
    z = rng.standard_normal((n, k) + tuple(hw)) * 3.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    if hw[0] >= 3 and hw[1] >= 3:
        p[0, :, 0, 0] = 1.0 / k
        if k > 1:
            p[-1, 1, 2, 1] = np.nan
    return p
