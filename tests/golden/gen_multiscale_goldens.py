#!/usr/bin/env python3
"""Generates tests/golden/multiscale.npz by running THE REFERENCE'S OWN single-frame test code on the CPU:
BaseModel.compute_test_output_for_scales and BaseModel.net_process (base/foundation.py:264-330), unbound, on a stand-in
`self` that carries `hparams` and a `forward` = the reference's own FlowPSPNet (eval, the synthetic weights of
synth.make_pspnet_state(50, 5, seed=0), built by gen_goldens.build_ref_pspnet).

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference>:<repo>:<repo>/tests/golden python3 <repo>/tests/golden/gen_multiscale_goldens.py

base/foundation.py imports the training stack (cv2, wandb, pytorch_lightning, skimage), absent offline and no part of this
arithmetic: import-only stand-ins are registered.  cv2 is the same-size stand-in of gen_goldens (cv2.resize accepted only
where it is a copy) plus copyMakeBorder as the constant pad it is (a copy into a filled array).  That pins the crop order, the
pull-back of the last row / column, the flip batch, upsample, softmax, un-flip and average, the float64 sums, the count
division and the cut-off of the padding; the two INTERPOLATING resizes are not reached (each case's frame already has the
size it is resized to).  Only arrays are stored: raw frames (uint8), the reference's results, figures about them.
"""
import os
import sys
import types

import numpy as np
import torch

import gen_goldens as gg
from flood_uav_video_segmentation_amd import synth

OUT = os.path.dirname(os.path.abspath(__file__))
CROP = 65
CLASSES = 5
CASES = {"i": (97, 150), "ii": (50, 150)}   # (i) 2 x 3 overlapping windows, last row / column pulled back; (ii) pad_h = 15, split 7 / 8
SEED = 2100
MASK_GAP = 2 * 2e-4   # twice the loosest tolerance the GPU test may assert: pixels whose two best classes are closer are not compared
MASK_CAP = 0.01


def make_frame(h, w, seed):
    """Raw 0-255 frame [3,h,w], integer valued: smooth colour fields + noise (seeded numpy PCG64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    img = np.empty((3, h, w))
    for c in range(3):
        fy, fx, ph = rng.uniform(1, 5), rng.uniform(1, 5), rng.uniform(0, 6.28)
        img[c] = 128 + 70 * np.sin(6.28 * (fy * yy + fx * xx) + ph) + rng.normal(0, 25, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def import_reference_foundation():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    names = ("cv2", "wandb", "pytorch_lightning", "skimage", "skimage.io")
    saved = {k: sys.modules.get(k) for k in names}
    cv2 = gg._cv2_same_size_stand_in()

    def copy_make_border(src, top, bottom, left, right, border_type, value=None):
        assert border_type == cv2.BORDER_CONSTANT
        out = np.empty((src.shape[0] + top + bottom, src.shape[1] + left + right) + src.shape[2:], dtype=src.dtype)
        out[:] = np.asarray(value, dtype=src.dtype)
        out[top:top + src.shape[0], left:left + src.shape[1]] = src
        return out

    cv2.BORDER_CONSTANT, cv2.copyMakeBorder = 0, copy_make_border
    sys.modules["cv2"] = cv2
    mod("wandb", run=None, summary={})
    mod("pytorch_lightning", LightningModule=type("LightningModule", (), {}), LightningDataModule=type("LightningDataModule", (), {}))
    mod("skimage", io=mod("skimage.io", imread=None))
    try:
        import base.foundation as ref_foundation  # reference
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref_foundation


def main():
    torch.set_grad_enabled(False)
    ref = import_reference_foundation()
    net = gg.build_ref_pspnet(synth.make_pspnet_state(50, CLASSES, seed=0))
    absmax = [0.0]

    def forward(x):
        out = net.decoder(net.encoder(x))
        absmax[0] = max(absmax[0], out.abs().max().item())
        return out

    obj = object.__new__(ref.BaseModel)
    obj.hparams = types.SimpleNamespace(test_h=CROP, test_w=CROP, classes=CLASSES)
    obj.forward = forward
    arrays = {"crop": np.array([CROP, CROP]), "classes": np.array(CLASSES), "mean": np.array(ref.mean), "std": np.array(ref.std),
              "round_train_in": np.array([873, 713, 65, 704, 720, 100]),
              "round_train_pspnet": np.array([ref.round_train(v, "pspnet") for v in (873, 713, 65, 704, 720, 100)]),
              "round_train_vit": np.array([ref.round_train(v, "vit") for v in (873, 713, 65, 704, 720, 100)]),
              "round_train_deeplabv3": np.array([ref.round_train(v, "deeplabv3") for v in (873, 713, 65, 704, 720, 100)]),
              "mask_gap": np.array(MASK_GAP)}
    for i, (name, (h, w)) in enumerate(CASES.items()):
        raw = make_frame(h, w, SEED + i)
        image = np.transpose(raw.astype(np.float32), (1, 2, 0))          # test_step: image = np.transpose(input, (1, 2, 0))
        pred = ref.BaseModel.compute_test_output_for_scales(obj, image, h, w)
        assert pred.dtype == np.float64 and pred.shape == (h, w, CLASSES)
        top2 = np.sort(pred, axis=2)[:, :, -2:]
        share = float(np.mean(top2[:, :, 1] - top2[:, :, 0] < MASK_GAP))
        assert share <= MASK_CAP, f"case {name}: {share:.4f} of the pixels are closer than {MASK_GAP}; choose another seed"
        arrays[f"raw_{name}"], arrays[f"pred_{name}"], arrays[f"excluded_share_{name}"] = raw, pred, np.array(share)
        print(f"case {name}: {h}x{w} excluded share {share:.5f} classes present {np.unique(pred.argmax(2)).tolist()}")
    # (iii) one crop through net_process, with and without the flip: the top-left window of case (i)
    crop = np.transpose(arrays["raw_i"].astype(np.float32), (1, 2, 0))[:CROP, :CROP].copy()
    arrays["crop_flip"] = ref.BaseModel.net_process(obj, crop.copy())
    arrays["crop_noflip"] = ref.BaseModel.net_process(obj, crop.copy(), flip=False)
    arrays["logit_absmax"] = np.array(absmax[0])
    print(f"largest |logit| {absmax[0]:.3f}")
    gg.save("multiscale.npz", **arrays)
    assert os.path.getsize(os.path.join(OUT, "multiscale.npz")) < 1_000_000


if __name__ == "__main__":
    main()
