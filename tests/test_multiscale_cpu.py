"""Single-frame multi-scale test, CPU side: the numpy / torch-CPU restatement (tests/multiscale_ref.py) against arrays the
REFERENCE'S OWN BaseModel.compute_test_output_for_scales / net_process produced (tests/golden/multiscale.npz, made by
tests/golden/gen_multiscale_goldens.py), the new C ABI symbols, and the constants the package mirrors.

Tolerance of the fixture comparison: rtol = 1e-12 (plus an absolute floor of 1e-12 for probabilities that underflow towards
0).  The restatement performs the reference's operations in the reference's order, and oracle.pspnet_oracle -- the CPU
network the tests have -- issues the same torch calls as the reference's nn.Module on these 65 x 65 flip batches, so the
float64 results agree to rounding (measured: bit for bit).
"""
import os
import re

import numpy as np
import pytest
import torch

import multiscale_ref as ms
from conftest import ROOT, load_golden
from flood_uav_video_segmentation_amd import _lib, synth
from flood_uav_video_segmentation_amd.base import foundation
from oracle import pspnet_oracle

torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def fixture():
    return load_golden("multiscale.npz")


@pytest.fixture(scope="module")
def forward():
    state = synth.make_pspnet_state(50, 5, seed=0)
    return lambda x: pspnet_oracle.decoder(pspnet_oracle.encoder(x, state, 50), state)


RTOL = ATOL = 1e-12


@pytest.mark.parametrize("case", ["i", "ii"])
def test_restatement_reproduces_the_references_scale_output(fixture, forward, case):
    z = fixture
    raw = z[f"raw_{case}"].astype(np.float32)
    h, w = raw.shape[1:]
    ch, cw = (int(v) for v in z["crop"])
    got = ms.compute_test_output_for_scales(forward, raw.transpose(1, 2, 0), h, w, ch, cw, int(z["classes"]))
    ref = z[f"pred_{case}"]
    assert got.dtype == np.float64 and got.shape == ref.shape
    err = np.abs(got - ref).max()
    print(f"case {case}: max abs {err:.3e}")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(ref.sum(2), 1.0, atol=1e-6)   # the padding was cut off: every kept pixel is a distribution
    assert float(z[f"excluded_share_{case}"]) <= 0.01
    # ... and the whole test_step arithmetic at scale 1 of a base_size equal to the long side is this one scale
    pred, mask = ms.predict(forward, raw, [1.0], ch, cw, int(z["classes"]), base_size=max(h, w))
    assert np.array_equal(pred, got) and np.array_equal(mask, got.argmax(2))


def test_windows_of_the_two_cases():
    # (i): 97 x 150 -> 2 x 3 windows of 65 at stride 44, the last row / column pulled back to the border
    assert ms.windows(97, 150, 65, 65) == [(0, 0), (0, 44), (0, 85), (32, 0), (32, 44), (32, 85)]
    # (ii): 50 rows are padded by 15, split 7 above / 8 below
    assert ms.pad_split(50, 65) == (7, 8) and ms.windows(65, 150, 65, 65) == [(0, 0), (0, 44), (0, 85)]
    assert foundation.crop_windows(97, 150, 65, 65) == ms.windows(97, 150, 65, 65)
    assert foundation.crop_windows(2016, 3584, 713, 713) == ms.windows(2016, 3584, 713, 713) and len(ms.windows(2016, 3584, 713, 713)) == 32
    assert foundation.scaled_size(1080, 1920, 1.75) == ms.scaled_size(1080, 1920, 1.75) == (2016, 3584)
    assert foundation.scaled_size(1920, 1080, 0.5) == (1024, 576)


@pytest.mark.parametrize("flip", [True, False])
def test_restatement_reproduces_the_references_net_process(fixture, forward, flip):
    z = fixture
    ch, cw = (int(v) for v in z["crop"])
    crop = z["raw_i"].astype(np.float32).transpose(1, 2, 0)[:ch, :cw].copy()
    got = ms.net_process(forward, crop, int(z["classes"]), flip=flip)
    ref = z["crop_flip" if flip else "crop_noflip"]
    assert got.dtype == np.float32 and got.shape == ref.shape == (ch, cw, int(z["classes"]))
    np.testing.assert_allclose(got.astype(np.float64), ref.astype(np.float64), rtol=RTOL, atol=ATOL)
    assert np.abs(z["crop_flip"].astype(np.float64) - z["crop_noflip"]).max() > 1e-3   # the flip half is not a no-op


def test_half_pixel_resize_is_the_identity_at_the_same_size_and_exact_on_ramps():
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 255, (7, 9, 3))
    assert np.array_equal(ms.resize_half_pixel(img, 7, 9), img)
    ramp = np.arange(8, dtype=np.float64)[None, :, None].repeat(3, 0)
    up = ms.resize_half_pixel(ramp, 3, 16)[0, :, 0]
    np.testing.assert_allclose(up[1:-1], ((np.arange(16) + 0.5) * 0.5 - 0.5)[1:-1], rtol=0, atol=1e-12)
    assert up[0] == 0.0 and up[-1] == 7.0   # clamped at the border


def test_constants_match_the_reference(fixture):
    z = fixture
    assert np.array_equal(np.array(foundation.mean), z["mean"]) and np.array_equal(np.array(foundation.std), z["std"])
    assert np.array_equal(np.array(ms.MEAN), z["mean"]) and np.array_equal(np.array(ms.STD), z["std"])
    for arch in ("pspnet", "vit", "deeplabv3"):
        assert [foundation.round_train(int(v), arch) for v in z["round_train_in"]] == z[f"round_train_{arch}"].tolist()
    with pytest.raises(ValueError):
        foundation.round_train(713, "unet")


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    for name in ("fs_ms_prepare", "fs_ms_fuse"):
        assert name in _lib.exported_symbols()
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert hasattr(_lib.load(), name)


def test_intersection_and_union_restatement():
    z, p = load_golden("metrics.npz"), load_golden("predict_713.npz")   # the pair test_oracle_golden.py feeds the reference's figures
    tgt = p["cfg3_mask"][1].copy()
    tgt[:40] = 255
    i, u, t = ms.intersection_and_union(p["cfg2_mask"][1], tgt, 5, 255)
    assert np.array_equal(i, z["inter"]) and np.array_equal(u, z["union"]) and np.array_equal(t, z["target"])
