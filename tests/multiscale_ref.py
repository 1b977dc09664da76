"""CPU restatement of the reference's single-frame multi-scale test (base/foundation.py:177-221, 264-330) for the tests of
the HIP route: numpy / torch-CPU, float64 wherever the reference is float64, with the half-pixel bilinear formula
(source coordinate (i + 0.5) * src / dst - 0.5, taps clamped to the image, horizontal pass first) standing for the two
interpolating cv2.resize calls -- the one part the reference-made fixture cannot pin (cv2 is absent where it is generated).

`forward` is any callable [B,3,h,w] fp32 CPU tensor -> logits [B,K,h',w'].  A test helper, not an oracle module.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

VALUE_SCALE = 255
MEAN = [item * VALUE_SCALE for item in [0.485, 0.456, 0.406]]
STD = [item * VALUE_SCALE for item in [0.229, 0.224, 0.225]]


def half_pixel_taps(dst, src):
    """Per destination index: (i0, i1, w1) -- clamped taps and the weight of the second, in float64."""
    pos = (np.arange(dst, dtype=np.float64) + 0.5) * (float(src) / float(dst)) - 0.5
    i0 = np.floor(pos).astype(np.int64)
    w1 = pos - i0
    low, high = i0 < 0, i0 >= src - 1
    i0 = np.clip(i0, 0, src - 1)
    w1[low | high] = 0.0
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, w1


def resize_half_pixel(img, new_h, new_w, dtype=np.float64):
    """[h,w,C] -> [new_h,new_w,C]; the arithmetic runs in `dtype` (weights rounded to it first)."""
    img = np.asarray(img).astype(dtype)
    y0, y1, wy = half_pixel_taps(new_h, img.shape[0])
    x0, x1, wx = half_pixel_taps(new_w, img.shape[1])
    wx1 = wx.astype(dtype)[None, :, None]
    wy1 = wy.astype(dtype)[:, None, None]
    wx0, wy0 = dtype(1) - wx1, dtype(1) - wy1
    top = wx0 * img[y0][:, x0] + wx1 * img[y0][:, x1]
    bot = wx0 * img[y1][:, x0] + wx1 * img[y1][:, x1]
    return wy0 * top + wy1 * bot


def scaled_size(h, w, scale, base_size=2048):
    long_size = round(scale * base_size)
    new_h = new_w = long_size
    if h > w:
        new_w = round(long_size / float(h) * w)
    else:
        new_h = round(long_size / float(w) * h)
    return new_h, new_w


def pad_split(size, crop):
    pad = max(crop - size, 0)
    return int(pad / 2), pad - int(pad / 2)


def windows(new_h, new_w, crop_h, crop_w, stride_rate=2 / 3):
    stride_h, stride_w = int(np.ceil(crop_h * stride_rate)), int(np.ceil(crop_w * stride_rate))
    grid_h = int(np.ceil(float(new_h - crop_h) / stride_h) + 1)
    grid_w = int(np.ceil(float(new_w - crop_w) / stride_w) + 1)
    out = []
    for ih in range(grid_h):
        for iw in range(grid_w):
            e_h, e_w = min(ih * stride_h + crop_h, new_h), min(iw * stride_w + crop_w, new_w)
            out.append((e_h - crop_h, e_w - crop_w))
    return out


def prepare(raw_chw, new_hw, padded_hw, dtype=np.float64):
    """What fs_ms_prepare computes, in `dtype`: [3,H,W] raw -> [3,PH,PW] resized, mean-padded, normalised (padding = 0)."""
    img = np.asarray(raw_chw).transpose(1, 2, 0)
    new_h, new_w = new_hw
    if (new_h, new_w) != img.shape[:2]:
        img = resize_half_pixel(img, new_h, new_w, dtype)
    img = img.astype(dtype)
    out = np.zeros((padded_hw[0], padded_hw[1], 3), dtype=dtype)
    top, left = (padded_hw[0] - new_h) // 2, (padded_hw[1] - new_w) // 2
    out[top:top + new_h, left:left + new_w] = (img - np.asarray(MEAN).astype(dtype)) / np.asarray(STD).astype(dtype)
    return out.transpose(2, 0, 1)


def net_process(forward, image, classes, flip=True):
    """One crop [h,w,3] (raw values, fp32) -> probabilities [h,w,K] fp32, in the reference's fp32 operation order."""
    x = torch.from_numpy(np.ascontiguousarray(image.transpose((2, 0, 1)))).float()
    for t, m, s in zip(x, MEAN, STD):
        t.sub_(m).div_(s)
    x = x.unsqueeze(0)
    if flip:
        x = torch.cat([x, x.flip(3)], 0)
    with torch.no_grad():
        out = forward(x)
    if not isinstance(out, torch.Tensor):
        out = out["pred"]
    out = out[:, 0:classes]
    if out.shape[2:] != x.shape[2:]:
        out = F.interpolate(out, tuple(x.shape[2:]), mode="bilinear", align_corners=True)
    out = F.softmax(out, dim=1)
    out = (out[0] + out[1].flip(2)) / 2 if flip else out[0]
    return out.numpy().transpose(1, 2, 0)


def probs_from_logits(lo_plain, lo_flip, crop_hw, dtype=torch.float64):
    """net_process behind the network on GIVEN logits [K,h,w] (lo_flip: those of the flipped crop, or None), in `dtype`."""
    def half(lo):
        lo = torch.as_tensor(lo).to(dtype)[None]
        if tuple(lo.shape[2:]) != tuple(crop_hw):
            lo = F.interpolate(lo, tuple(crop_hw), mode="bilinear", align_corners=True)
        return F.softmax(lo, dim=1)[0]
    p = half(lo_plain)
    if lo_flip is not None:
        p = (p + half(lo_flip).flip(2)) / 2
    return p.numpy().transpose(1, 2, 0)


def stitch(crop_probs, wins, crop_hw, padded_hw, new_hw):
    """Float64 sum of the crops' probabilities in crop order / count, padding cut: [new_h,new_w,K]."""
    ch, cw = crop_hw
    k = crop_probs[0].shape[2]
    acc = np.zeros((padded_hw[0], padded_hw[1], k), dtype=float)
    cnt = np.zeros(padded_hw, dtype=float)
    for (y, x), p in zip(wins, crop_probs):
        cnt[y:y + ch, x:x + cw] += 1
        acc[y:y + ch, x:x + cw, :] += p
    with np.errstate(invalid="ignore", divide="ignore"):
        acc /= np.expand_dims(cnt, 2)
    top, left = (padded_hw[0] - new_hw[0]) // 2, (padded_hw[1] - new_hw[1]) // 2
    return acc[top:top + new_hw[0], left:left + new_hw[1]]


def to_frame(scaled, h, w):
    """cv2.resize(prediction_crop, (w, h)) -- a copy at the same size, else half-pixel bilinear in float64."""
    if scaled.shape[:2] == (h, w):
        return scaled.copy()
    return resize_half_pixel(scaled, h, w, np.float64)


def compute_test_output_for_scales(forward, image, h, w, crop_h, crop_w, classes, flip=True):
    """image: [ori_h,ori_w,3] fp32 raw values, already scaled -> float64 [h,w,K]."""
    ori_h, ori_w, _ = image.shape
    (top, bottom), (left, right) = pad_split(ori_h, crop_h), pad_split(ori_w, crop_w)
    if top + bottom or left + right:
        padded = np.empty((ori_h + top + bottom, ori_w + left + right, 3), dtype=image.dtype)
        padded[:] = np.asarray(MEAN, dtype=image.dtype)
        padded[top:top + ori_h, left:left + ori_w] = image
        image = padded
    new_h, new_w, _ = image.shape
    wins = windows(new_h, new_w, crop_h, crop_w)
    probs = [net_process(forward, image[y:y + crop_h, x:x + crop_w].copy(), classes, flip) for y, x in wins]
    return to_frame(stitch(probs, wins, (crop_h, crop_w), (new_h, new_w), (ori_h, ori_w)), h, w)


def predict(forward, raw_chw, scales, crop_h, crop_w, classes, base_size=2048):
    """test_step up to the argmax: raw [3,H,W] fp32 -> (float64 [H,W,K] prediction, int64 mask)."""
    image = np.asarray(raw_chw, dtype=np.float32).transpose(1, 2, 0)
    h, w, _ = image.shape
    prediction = np.zeros((h, w, classes), dtype=float)
    for scale in scales:
        new_h, new_w = scaled_size(h, w, scale, base_size)
        scaled = image if (new_h, new_w) == (h, w) else resize_half_pixel(image, new_h, new_w, np.float64).astype(np.float32)
        prediction += compute_test_output_for_scales(forward, scaled, h, w, crop_h, crop_w, classes)
    prediction /= len(scales)
    return prediction, np.argmax(prediction, axis=2)


def intersection_and_union(output, target, k, ignore_index=255):
    """util/util.py:36-49 restated: per-class intersection / union / target pixel counts."""
    output = np.asarray(output).reshape(-1).astype(np.int64).copy()
    target = np.asarray(target).reshape(-1).astype(np.int64)
    output[target == ignore_index] = ignore_index
    inter = output[output == target]
    area_i = np.bincount(inter[inter < k], minlength=k)[:k]
    area_o = np.bincount(output[output < k], minlength=k)[:k]
    area_t = np.bincount(target[target < k], minlength=k)[:k]
    return area_i, area_o + area_t - area_i, area_t
