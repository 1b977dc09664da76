"""The reference's single-frame test protocol on the HIP path -- mirrors base/foundation.py:27-42 (mean, std, round_train) and
:177-221, 264-330 (BaseModel.test_step -> compute_test_output_for_scales -> net_process), which supervised.py, gan.py and
contrastive.py inherit: multi-scale, flip-averaged sliding crops, the mIoU of the key-frame segmenter itself.

    ev = SingleFrameEvaluator(net, classes=5, test_h=713, test_w=713, test_scales=[0.5, 0.75, 1.0, 1.25, 1.5, 1.75])
    for image, target in test_set:                       # image: the raw 0-255 frame [3,H,W] on the GPU, target uint8 [H,W]
        ev.test_step(image, target, test_idx=0)
    miou, macc, acc, iou_class, acc_class = ev.summary(0)

Per scale one fs_ms_prepare launch writes the resized, mean-padded, normalised frame and its horizontal mirror; the crops of
both are read in place by the network (fs_segment_crops), `crop_batch` windows per call; fs_ms_fuse turns all logits of the
scale into the float64 probabilities of the frame.  Nothing per crop reaches the host.  Images are CHW device tensors (the
reference transposes to HWC numpy, :188-189); probabilities come back [h,w,K] like the reference's.
"""
import math

import numpy as np
import torch

from .. import ops

# base/foundation.py:27-31
value_scale = 255
mean = [0.485, 0.456, 0.406]
mean = [item * value_scale for item in mean]
std = [0.229, 0.224, 0.225]
std = [item * value_scale for item in std]


def round_train(train, arch):
    """Round a crop size to the nearest size the architecture permits (base/foundation.py:34-42)."""
    if arch == "pspnet":
        return (train - 1) // 8 * 8 + 1
    elif arch == "vit":
        return train // 32 * 32
    elif arch == "deeplabv3":
        return (train - 1) // 8 * 8 + 1
    raise ValueError(f"floodseg: unknown arch '{arch}' (pspnet, vit, deeplabv3)")


def scaled_size(h, w, scale, base_size=2048):
    """(new_h, new_w) of test_step for one scale: the long side becomes round(scale * base_size) (base/foundation.py:193-199)."""
    long_size = round(scale * base_size)
    new_h = new_w = long_size
    if h > w:
        new_w = round(long_size / float(h) * w)
    else:
        new_h = round(long_size / float(w) * h)
    return new_h, new_w


def crop_windows(new_h, new_w, crop_h, crop_w, stride_rate=2 / 3):
    """Top-left corners of compute_test_output_for_scales' crops of a (padded) new_h x new_w frame, in its order; the last row /
    column is pulled back to the border (base/foundation.py:275-288)."""
    stride_h = int(math.ceil(crop_h * stride_rate))
    stride_w = int(math.ceil(crop_w * stride_rate))
    grid_h = int(math.ceil(float(new_h - crop_h) / stride_h) + 1)
    grid_w = int(math.ceil(float(new_w - crop_w) / stride_w) + 1)
    out = []
    for index_h in range(grid_h):
        for index_w in range(grid_w):
            e_h = min(index_h * stride_h + crop_h, new_h)
            e_w = min(index_w * stride_w + crop_w, new_w)
            out.append((e_h - crop_h, e_w - crop_w))
    return out


class SingleFrameEvaluator:
    """BaseModel.test_step and what it calls, over a HIP network mirror: PSPNet / DeepLabv3 (crops read in place through
    `segment_crops`) or the Segmenter (its crops are cut and go through `forward`, which already returns crop-size logits)."""

    MAX_CLASSES = 8   # fs_ms_fuse
    MAX_CROPS = 64

    def __init__(self, model, classes, test_h, test_w, test_scales=(1.0,), arch="pspnet", ignore_index=255, base_size=2048, crop_batch=8):
        if round_train(test_h, arch) != test_h or round_train(test_w, arch) != test_w:
            raise ValueError(f"floodseg: crop {test_h}x{test_w} is not a size arch '{arch}' permits "
                             f"(nearest: {round_train(test_h, arch)}x{round_train(test_w, arch)})")
        if not 1 <= classes <= self.MAX_CLASSES:
            raise ValueError(f"floodseg: the multi-scale test takes 1..{self.MAX_CLASSES} classes, not {classes}")
        if not 1 <= crop_batch <= 32:
            raise ValueError("floodseg: crop_batch must lie in 1..32 (fs_segment_crops)")
        if len(test_scales) < 1:
            raise ValueError("floodseg: test_scales is empty")
        self.model = model
        self.classes, self.test_h, self.test_w = int(classes), int(test_h), int(test_w)
        self.test_scales, self.arch, self.ignore_index = list(test_scales), arch, ignore_index
        self.base_size, self.crop_batch = int(base_size), int(crop_batch)
        self.in_place = hasattr(model, "segment_crops")
        self.hist = {}  # meter id -> int64[3,K] (intersection, |pred|, |target|)
        model.reserve(self.crop_batch, self.test_h, self.test_w)

    # -- the network ------------------------------------------------------------------------------
    def _raw(self, image, what):
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise RuntimeError(f"floodseg {what}: the image must be a tensor on the GPU (no CPU fallback exists)")
        if image.dim() == 4 and image.shape[0] == 1:   # assert input.shape[0] == 1, base/foundation.py:181
            image = image[0]
        if image.dim() != 3 or image.shape[0] != 3:
            raise RuntimeError(f"floodseg {what}: expected a raw 0-255 frame [3,H,W], got {tuple(image.shape)}")
        return image

    def _forward(self, x):
        """Logits of a dense batch [B,3,h,w]: low-resolution where the mirror offers `segment`, else forward()'s."""
        if hasattr(self.model, "segment"):
            return self.model.segment(x)
        out = self.model(x)
        return out if isinstance(out, torch.Tensor) else out["pred"]    # base/foundation.py:314-315

    def _crop_logits(self, frames, windows, flip):
        """Logits of every window of frames[0] and, with flip, of the mirrored windows of frames[1] -> (lo_plain, lo_flip)."""
        ch, cw, pw = self.test_h, self.test_w, frames.shape[3]
        halves = [(0, windows)] + ([(1, [(y, pw - x - cw) for y, x in windows])] if flip else [])
        los = []
        for idx, wins in halves:
            lo = None
            for c0 in range(0, len(wins), self.crop_batch):
                sub = wins[c0:c0 + self.crop_batch]
                if self.in_place:   # from the second batch on the library writes straight into the scale's logits
                    part = self.model.segment_crops(frames[idx:idx + 1], None, sub, (ch, cw), out=None if lo is None else lo[c0:c0 + len(sub)])
                else:
                    part = self._forward(torch.stack([frames[idx, :, y:y + ch, x:x + cw] for y, x in sub]))
                if lo is None:
                    lo = part if len(sub) == len(wins) else torch.empty((len(wins),) + tuple(part.shape[1:]), dtype=torch.float32, device=part.device)
                    if lo is not part:
                        lo[:len(sub)] = part
                elif not self.in_place:
                    lo[c0:c0 + len(sub)] = part
            los.append(lo)
        return los[0], (los[1] if flip else None)

    def _scale(self, raw, new_h, new_w, frame_hw, pred, scale_index, nscales, want_mask, flip=True):
        """One scale from the raw frame: prepare, crops through the network, fuse (+ accumulate into `pred` when frame_hw is given)."""
        ch, cw = self.test_h, self.test_w
        ph, pw = max(new_h, ch), max(new_w, cw)     # base/foundation.py:267-274
        windows = crop_windows(ph, pw, ch, cw)
        if len(windows) > self.MAX_CROPS:
            raise RuntimeError(f"floodseg: a {ph}x{pw} scale has {len(windows)} crops of {ch}x{cw}; one scale takes at most {self.MAX_CROPS}")
        frames = ops.ms_prepare(raw, (new_h, new_w), (ph, pw), mean, std, flip=flip)
        lo_plain, lo_flip = self._crop_logits(frames, windows, flip)
        return ops.ms_fuse(lo_plain, lo_flip, windows, (ch, cw), (ph, pw), (new_h, new_w), pred=pred, frame_hw=frame_hw,
                           scale_index=scale_index, nscales=nscales, want_mask=want_mask)

    # -- the reference's methods ------------------------------------------------------------------
    def net_process(self, image_crop, flip=True):
        """One crop [3,h,w] of the (padded) raw frame -> its probabilities [h,w,K] float64: normalise, the crop and its mirror as
        one batch, upsample, softmax, un-flip, average (base/foundation.py:299-330).  The generic per-crop route."""
        raw = self._raw(image_crop, "net_process")
        h, w = raw.shape[1], raw.shape[2]
        frames = ops.ms_prepare(raw, (h, w), (h, w), mean, std, flip=flip)
        lo = self._forward(frames)
        scaled, _, _ = ops.ms_fuse(lo[0:1], lo[1:2] if flip else None, [(0, 0)], (h, w), (h, w), (h, w))
        return scaled

    def compute_test_output_for_scales(self, image, h, w):
        """The already scaled raw frame [3,new_h,new_w] -> crop- and flip-averaged probabilities resized to (h, w): float64 [h,w,K]
        on the device (base/foundation.py:264-295)."""
        raw = self._raw(image, "compute_test_output_for_scales")
        return self._scale(raw, raw.shape[1], raw.shape[2], (int(h), int(w)), None, 0, 1, False)[1]

    def predict(self, image):
        """All scales of one raw frame [3,H,W] -> (prediction float64 [H,W,K], uint8 mask [H,W]) (base/foundation.py:190-203)."""
        raw = self._raw(image, "predict")
        h, w = raw.shape[1], raw.shape[2]
        pred = mask = None
        for i, scale in enumerate(self.test_scales):
            new_h, new_w = scaled_size(h, w, scale, self.base_size)
            _, pred, mask = self._scale(raw, new_h, new_w, (h, w), pred, i, len(self.test_scales), True)
        return pred, mask

    def test_step(self, image, target, test_idx=0):
        """predict + the intersection / union / target histograms of the test list (0 = Florida, > 0 = Texas; :207-214)."""
        _, mask = self.predict(image)
        if not isinstance(target, torch.Tensor) or not target.is_cuda:
            raise RuntimeError("floodseg test_step: the target must be a tensor on the GPU")
        target = target.reshape(mask.shape).to(torch.uint8).contiguous()   # ids 0..K-1 and 255 fit
        meter = 1 if test_idx > 0 else 0
        self.hist[meter] = ops.iou_hist(mask, target, self.classes, self.ignore_index, self.hist.get(meter))
        return mask

    def summary(self, meter=0):
        """(mIoU, mAcc, accuracy, iou_class, accuracy_class) with the reference's 1e-10 epsilon (base/foundation.py:226-230)."""
        if meter not in self.hist:
            return None
        h = self.hist[meter].cpu().numpy().astype(np.float64)
        inter, union, target = h[0], h[1] + h[2] - h[0], h[2]
        iou_class, acc_class = inter / (union + 1e-10), inter / (target + 1e-10)
        return float(np.mean(iou_class)), float(np.mean(acc_class)), float(inter.sum() / (target.sum() + 1e-10)), iou_class, acc_class
