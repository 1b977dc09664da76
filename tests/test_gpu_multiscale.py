"""Single-frame multi-scale, flip-averaged sliding-crop test on the GPU (fs_ms_prepare, fs_ms_fuse, SingleFrameEvaluator).

Op level: each kernel through the C ABI against the float64 restatement of tests/multiscale_ref.py, and against the
existing, already pinned ops where the new pass must agree with them bit for bit.  End to end: the evaluator against the
arrays the reference's own compute_test_output_for_scales / net_process produced (tests/golden/multiscale.npz) and against
the per-crop generic route.

Tolerances are 3-5 x the max-abs errors measured on the MI355X (profiles/r07_ms_parity_measured.txt):
  PREP_TOL  fs_ms_prepare vs float64 (normalised units): fp32 weights and three fp32 roundings per pixel of values <= 2.7;
  PROB_TOL  probabilities on given logits vs float64: fp32 upsample + expf + divide, summed in float64;
  E2E_TOL   probabilities behind the network (the HIP network's own error dominates); no looser than the 2e-4 the
            sliding-crop canvas test asserts for the same kind of quantity.
"""
import ctypes

import numpy as np
import pytest
import torch

import multiscale_ref as ms
from conftest import load_golden, note
from flood_uav_video_segmentation_amd import _lib, ops, synth
from flood_uav_video_segmentation_amd._lib import ptr, stream_ptr
from flood_uav_video_segmentation_amd.base.foundation import SingleFrameEvaluator, crop_windows, mean, scaled_size, std

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PREP_TOL = 3e-6
PROB_TOL = 3e-6
E2E_TOL = 5e-5
DEEPLAB_TOL = 2e-4   # see test_deeplabv3_r101_small_frame_against_the_generic_route
assert max(E2E_TOL, DEEPLAB_TOL) <= 2e-4


class HP:
    def __init__(self, layers=50, classes=5):
        self.layers, self.classes, self.pretrained = layers, classes, False


@pytest.fixture(scope="module")
def pspnet():
    from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

    net = FlowPSPNet(HP(50, 5)).eval()
    net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
    return net


def smooth_frame(h, w, seed):
    """A raw 0-255 frame [3,h,w] from the smooth random field every network test of this suite feeds (synth.make_clip)."""
    x = synth.make_clip(1, (h, w), seed=seed)[0]
    return (x * torch.tensor(std)[:, None, None] + torch.tensor(mean)[:, None, None]).clamp(0, 255).float()


def raw_frame(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(0, 255, (3, h, w)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ (a) fs_ms_prepare
def test_prepare_identity_scale_is_bit_exact_and_the_mirror_is_the_flip():
    raw = raw_frame(37, 53, 1)
    out = ops.ms_prepare(raw.cuda(), (37, 53), (37, 53), mean, std).cpu()
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    assert torch.equal(out[0], (raw - m) / s)          # sub, then a true division, in fp32
    assert torch.equal(out[1], out[0].flip(2))
    assert ops.ms_prepare(raw.cuda(), (37, 53), (37, 53), mean, std, flip=False).shape == (1, 3, 37, 53)


def test_prepare_padding_is_exactly_zero_and_split_like_the_reference():
    raw = raw_frame(50, 150, 2)
    out = ops.ms_prepare(raw.cuda(), (50, 150), (65, 150), mean, std).cpu()
    assert torch.count_nonzero(out[:, :, :7]) == 0 and torch.count_nonzero(out[:, :, 57:]) == 0     # pad_h = 15: 7 above, 8 below
    ref = ms.prepare(raw.numpy(), (50, 150), (65, 150), np.float32)
    assert np.array_equal(out[0].numpy(), ref)
    assert torch.equal(out[1], out[0].flip(2))
    out = ops.ms_prepare(raw.cuda(), (50, 150), (65, 161), mean, std).cpu()                         # pad_w = 11: 5 left, 6 right
    assert torch.count_nonzero(out[0, :, :, :5]) == 0 and torch.count_nonzero(out[0, :, :, 155:]) == 0
    assert torch.equal(out[1], out[0].flip(2))                 # the mirror carries the padding mirrored: 6 left, 5 right
    assert np.array_equal(out[0].numpy(), ms.prepare(raw.numpy(), (50, 150), (65, 161), np.float32))


@pytest.mark.parametrize("hw", [(54, 96), (97, 41), (33, 33)])
@pytest.mark.parametrize("scale", [0.5, 0.75, 1.25, 1.75])
def test_prepare_scales_against_float64(hw, scale):
    h, w = hw
    raw = raw_frame(h, w, h * w)
    new_h, new_w = scaled_size(h, w, scale, base_size=96)       # long side 48, 72, 120, 168: down- and up-scales, odd sizes
    ph, pw = max(new_h, 65), max(new_w, 65)
    out = ops.ms_prepare(raw.cuda(), (new_h, new_w), (ph, pw), mean, std).cpu()
    ref = ms.prepare(raw.numpy(), (new_h, new_w), (ph, pw), np.float64)
    err = note(f"ms_prepare_{h}x{w}_s{scale}", np.abs(out[0].numpy().astype(np.float64) - ref).max())
    print(f"ms_prepare {h}x{w} scale {scale}: max abs {err:.3e}")
    assert err < PREP_TOL
    assert torch.equal(out[1], out[0].flip(2))
    assert (out[0].numpy()[ref == 0] == 0).all()                # the padding is exactly zero


# ------------------------------------------------------------------------------------------------ (b) + (c) fs_ms_fuse
def given_logits(nc, k, fh, fw, seed):
    """Random logits with ties between classes and +-30 magnitudes."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn((nc, k, fh, fw), generator=g) * 3
    lo[:, :, ::3, ::2] *= 10                                   # up to about +-30
    lo[:, 1, 1::4] = lo[:, 0, 1::4]                            # exact ties of the first two classes
    return lo.clamp(-30, 30)


def fuse_ref(lo_plain, lo_flip, wins, crop_hw, padded_hw, new_hw, frame_hw=None):
    probs = [ms.probs_from_logits(lo_plain[c], None if lo_flip is None else lo_flip[c], crop_hw) for c in range(len(wins))]
    scaled = ms.stitch(probs, wins, crop_hw, padded_hw, new_hw)
    return scaled, (None if frame_hw is None else ms.to_frame(scaled, *frame_hw))


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("geom", [dict(new=(97, 150), frame=(97, 150)), dict(new=(50, 150), frame=(50, 150)), dict(new=(97, 150), frame=(61, 94)),
                                  dict(new=(70, 110), frame=(131, 200))])
def test_fuse_given_logits_against_float64(geom, flip):
    ch = cw = 65
    new_h, new_w = geom["new"]
    ph, pw = max(new_h, ch), max(new_w, cw)
    wins = crop_windows(ph, pw, ch, cw)
    count = np.zeros((ph, pw))
    for y, x in wins:
        count[y:y + ch, x:x + cw] += 1
    if geom["new"] == (97, 150):
        assert set(np.unique(count)) == {1, 2, 4} and wins[-1] == (32, 85)    # pixels under 1, 2 and 4 crops; pulled back to the border
    lo_a, lo_b = given_logits(len(wins), 5, 9, 9, 3), given_logits(len(wins), 5, 9, 9, 4)
    scaled, pred, _ = ops.ms_fuse(lo_a.cuda(), lo_b.cuda() if flip else None, wins, (ch, cw), (ph, pw), (new_h, new_w), frame_hw=geom["frame"])
    ref_scaled, ref_pred = fuse_ref(lo_a, lo_b if flip else None, wins, (ch, cw), (ph, pw), (new_h, new_w), geom["frame"])
    e1 = np.abs(scaled.cpu().numpy() - ref_scaled).max()
    e2 = np.abs(pred.cpu().numpy() - ref_pred).max()
    note(f"ms_fuse_given_logits_{new_h}x{new_w}_to_{geom['frame'][0]}x{geom['frame'][1]}_flip{int(flip)}", max(e1, e2))
    print(f"ms_fuse {geom} flip={flip}: scaled {e1:.3e} pred {e2:.3e}")
    assert e1 < PROB_TOL and e2 < PROB_TOL
    if geom["frame"] == geom["new"]:
        assert torch.equal(pred, scaled)                       # the resize back to the frame is the exact identity


def test_fuse_one_crop_without_flip_equals_the_existing_ops():
    lo = given_logits(1, 5, 9, 9, 7).cuda()
    ch, cw = 65, 73
    scaled, _, _ = ops.ms_fuse(lo, None, [(0, 0)], (ch, cw), (ch, cw), (ch, cw))
    lib = _lib.load()
    up = ops.resize_bilinear(lo, (ch, cw), align_corners=True)
    canvas = torch.zeros((1, 5, ch, cw), dtype=torch.float64, device="cuda")
    count = torch.zeros((ch, cw), dtype=torch.float64, device="cuda")
    _lib.check(lib.fs_softmax_accumulate(ptr(up), 1, 5, ch, cw, ptr(canvas), ptr(count), ch, cw, 0, 0, stream_ptr()))
    _lib.check(lib.fs_canvas_finish(ptr(canvas), ptr(count), 1, 5, ch * cw, None, stream_ptr()))
    assert torch.equal(scaled, canvas[0].permute(1, 2, 0).contiguous())


def test_fuse_scales_accumulate_and_argmax_ties_take_the_first_class():
    ch = cw = 33
    wins = [(0, 0)]
    lo = torch.zeros((1, 4, 5, 5))
    lo[0, 2:, :, :] = -3.0                                     # classes 0 and 1 tie everywhere
    lo[0, 1, 2:, :] = 1.0                                      # ... except below, where class 1 wins
    pred = None
    for i in range(3):
        scaled, pred, mask = ops.ms_fuse(lo.cuda(), lo.flip(3).cuda(), wins, (ch, cw), (ch, cw), (ch, cw), pred=pred, frame_hw=(ch, cw),
                                         scale_index=i, nscales=3, want_mask=True)
        assert (mask is None) == (i < 2)
    s = scaled.cpu().numpy()
    assert np.array_equal(pred.cpu().numpy(), (s + s + s) / 3)                 # float64 sum over the scales, divided once at the end
    m = mask.cpu().numpy()
    assert np.array_equal(m, np.argmax(pred.cpu().numpy(), axis=2)) and set(np.unique(m)) == {0, 1} and (m[:8] == 0).all()


def test_refusals_return_an_error_without_a_launch():
    lib = _lib.load()
    raw = raw_frame(20, 20, 3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.ms_prepare(raw, (20, 20), (20, 20), mean, std)
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    out = torch.empty((2, 3, 20, 20), device="cuda")
    assert lib.fs_ms_prepare(ptr(raw), 20, 20, 20, 20, 20, 20, m, s, ptr(out), 1, stream_ptr()) != 0      # a host pointer
    assert b"device pointer" in lib.fs_last_error()
    assert lib.fs_ms_prepare(None, 20, 20, 20, 20, 20, 20, m, s, ptr(out), 1, stream_ptr()) != 0
    assert lib.fs_ms_prepare(ptr(raw.cuda()), 20, 20, 20, 20, 19, 20, m, s, ptr(out), 1, stream_ptr()) != 0  # padded < scaled
    lo = torch.zeros((1, 9, 3, 3), device="cuda")
    with pytest.raises(RuntimeError, match="K=9"):
        ops.ms_fuse(lo, None, [(0, 0)], (17, 17), (17, 17), (17, 17))
    lo = torch.zeros((1, 5, 3, 3), device="cuda")
    with pytest.raises(RuntimeError, match="crop 0 outside"):
        ops.ms_fuse(lo, None, [(1, 0)], (17, 17), (17, 17), (17, 17))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.ms_fuse(lo.cpu(), None, [(0, 0)], (17, 17), (17, 17), (17, 17))
    scaled = torch.empty((17, 17, 5), dtype=torch.float64, device="cuda")
    ys = (ctypes.c_int * 1)(0)
    assert lib.fs_ms_fuse(ptr(lo.cpu()), None, 1, ys, ys, 5, 3, 3, 17, 17, 17, 17, 17, 17, ptr(scaled), None, 0, 0, 0, 1, None, stream_ptr()) != 0
    assert b"device pointer" in lib.fs_last_error()
    lo65 = torch.zeros((65, 5, 3, 3), device="cuda")
    with pytest.raises(RuntimeError, match="65 crops"):
        ops.ms_fuse(lo65, None, [(0, 0)] * 65, (17, 17), (17, 17), (17, 17))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
def masks_agree_outside_near_ties(mask, ref_pred, gap, cap=0.01):
    top2 = np.sort(ref_pred, axis=2)[:, :, -2:]
    near = (top2[:, :, 1] - top2[:, :, 0]) < gap
    print(f"near ties (two best classes closer than {gap:.1e}): {near.mean():.5f} of the pixels")
    assert cap is None or near.mean() <= cap, f"{near.mean():.4f} of the pixels are near ties: the exclusion is capped at {cap}"
    return np.array_equal(np.asarray(mask)[~near], np.argmax(ref_pred, axis=2)[~near])


@pytest.mark.parametrize("case", ["i", "ii"])
def test_evaluator_reproduces_the_references_scale_output(pspnet, case):
    z = load_golden("multiscale.npz")
    raw = torch.from_numpy(z[f"raw_{case}"].astype(np.float32)).cuda()
    h, w = raw.shape[1:]
    ev = SingleFrameEvaluator(pspnet, 5, 65, 65, test_scales=[1.0], base_size=max(h, w), crop_batch=4)
    got = ev.compute_test_output_for_scales(raw, h, w)
    assert got.dtype == torch.float64 and got.shape == (h, w, 5) and got.is_cuda
    err = note(f"ms_evaluator_vs_reference_case_{case}", np.abs(got.cpu().numpy() - z[f"pred_{case}"]).max())
    print(f"evaluator vs the reference, case {case}: max abs {err:.3e}")
    assert err < E2E_TOL
    pred, mask = ev.predict(raw)                               # scale 1 of a base_size equal to the long side: the same single scale
    assert torch.equal(pred, got) and mask.dtype == torch.uint8
    assert masks_agree_outside_near_ties(mask.cpu().numpy(), z[f"pred_{case}"], 2 * E2E_TOL)


@pytest.mark.parametrize("flip", [True, False])
def test_net_process_reproduces_the_references(pspnet, flip):
    z = load_golden("multiscale.npz")
    crop = torch.from_numpy(z["raw_i"].astype(np.float32))[:, :65, :65].contiguous().cuda()
    ev = SingleFrameEvaluator(pspnet, 5, 65, 65)
    got = ev.net_process(crop, flip=flip)
    ref = z["crop_flip" if flip else "crop_noflip"]
    assert got.shape == ref.shape
    err = note(f"ms_net_process_vs_reference_flip{int(flip)}", np.abs(got.cpu().numpy() - ref).max())
    print(f"net_process vs the reference, flip={flip}: max abs {err:.3e}")
    assert err < E2E_TOL


def generic_route(ev, raw, scales, base_size):
    """predict through net_process per crop on the device and the helper's resizes and stitching on the host."""
    image = raw.cpu().numpy().transpose(1, 2, 0)
    h, w, _ = image.shape
    ch, cw = ev.test_h, ev.test_w
    prediction = np.zeros((h, w, ev.classes))
    for scale in scales:
        new_h, new_w = ms.scaled_size(h, w, scale, base_size)
        scaled = image if (new_h, new_w) == (h, w) else ms.resize_half_pixel(image, new_h, new_w).astype(np.float32)
        (top, bottom), (left, right) = ms.pad_split(new_h, ch), ms.pad_split(new_w, cw)
        padded = np.empty((new_h + top + bottom, new_w + left + right, 3), dtype=np.float32)
        padded[:] = np.asarray(ms.MEAN, dtype=np.float32)
        padded[top:top + new_h, left:left + new_w] = scaled
        wins = ms.windows(padded.shape[0], padded.shape[1], ch, cw)
        dev = torch.from_numpy(padded.transpose(2, 0, 1).copy()).cuda()
        probs = [ev.net_process(dev[:, y:y + ch, x:x + cw].contiguous()).cpu().numpy() for y, x in wins]
        prediction += ms.to_frame(ms.stitch(probs, wins, (ch, cw), padded.shape[:2], (new_h, new_w)), h, w)
    prediction /= len(scales)
    return prediction, np.argmax(prediction, axis=2)


def check_against_generic(ev, raw, name, tol=E2E_TOL, cap=0.01):
    pred, mask = ev.predict(raw)
    ref_pred, ref_mask = generic_route(ev, raw, ev.test_scales, ev.base_size)
    err = note(name, np.abs(pred.cpu().numpy() - ref_pred).max())
    print(f"{name}: max abs {err:.3e}")
    assert err < tol
    assert masks_agree_outside_near_ties(mask.cpu().numpy(), ref_pred, 2 * tol, cap)
    return pred, mask, ref_mask


def test_predict_1080x1920_three_scales_parity_unpinned(pspnet):
    """One 1080 x 1920 frame, 713 x 713 crops, scales 0.75 / 1.0 / 1.25 (6 + 8 + 15 crops, each with its flip): the one-pass route
    against the per-crop generic route; the meters of test_step against the helper's intersection_and_union.  parity_unpinned:
    the two interpolating resizes are the half-pixel formula on both sides, no cv2 result backs them."""
    raw = smooth_frame(1080, 1920, 41).cuda()
    ev = SingleFrameEvaluator(pspnet, 5, 713, 713, test_scales=[0.75, 1.0, 1.25], base_size=2048, crop_batch=8)
    pred, mask, ref_mask = check_against_generic(ev, raw, "ms_predict_1080x1920_3scales_vs_generic")
    r1 = pspnet._hip_net.reserved_bytes()
    pred2, mask2 = ev.predict(raw)
    assert pspnet._hip_net.reserved_bytes() == r1              # nothing allocates inside the library from the second frame on
    assert torch.equal(pred, pred2) and torch.equal(mask, mask2)
    target = torch.from_numpy(np.random.default_rng(9).integers(0, 6, (1080, 1920))).to(torch.uint8)
    target[target == 5] = 255
    ev.test_step(raw, target.cuda(), test_idx=0)
    ev.test_step(raw, target.cuda(), test_idx=1)
    h = ev.hist[0].cpu().numpy()
    assert np.array_equal(h, ev.hist[1].cpu().numpy())
    i, u, t = ms.intersection_and_union(mask.cpu().numpy(), target.numpy(), 5, 255)
    assert np.array_equal(h[0], i) and np.array_equal(h[1] + h[2] - h[0], u) and np.array_equal(h[2], t)   # exact on the route's own mask
    ri, ru, _ = ms.intersection_and_union(ref_mask, target.numpy(), 5, 255)
    miou, miou_ref = ev.summary(0)[0], float(np.mean(ri / (ru + 1e-10)))
    print(f"mIoU {miou:.6f} vs generic {miou_ref:.6f}")
    assert abs(miou - miou_ref) < 1e-3                         # 0.1 pp


def test_deeplabv3_r101_small_frame_against_the_generic_route():
    """Measured 9.1e-5.  Both routes run the same HIP network on the same crops; what differs is the scale-0.75 input, resized in
    fp32 on the device on one side and in float64 on the host (then rounded to fp32) on the other: last-bit differences of the
    pixels, which 101 layers with synthetic weights amplify (PSPNet-R50: 1.0e-5).  3 x the measured value would pass the 2e-4
    ceiling the sliding-crop canvas tests set for this kind of quantity, so the ceiling itself is asserted (2.2 x).  The synthetic DeepLabv3 ties its two best classes on 5.9 % of this frame (the bottom rows),
    so the 1 % cap on pixels left out of the mask comparison, which is stated for the fixture cases, is not applied here: the share
    is printed, the masks are compared everywhere else."""
    from flood_uav_video_segmentation_amd.model.deeplabv3 import FlowDeepLabv3

    net = FlowDeepLabv3(HP(101, 5)).eval()
    net.load_state_dict(synth.make_deeplab_state(101, 5, seed=0))
    ev = SingleFrameEvaluator(net, 5, 129, 129, test_scales=[0.75, 1.0], arch="deeplabv3", base_size=256, crop_batch=4)
    raw = smooth_frame(150, 256, 11).cuda()
    check_against_generic(ev, raw, "ms_predict_deeplabv3_r101_150x256_vs_generic", tol=DEEPLAB_TOL, cap=None)
    ev1 = SingleFrameEvaluator(net, 5, 129, 129, test_scales=[1.0], arch="deeplabv3", base_size=256, crop_batch=4)
    check_against_generic(ev1, raw, "ms_predict_deeplabv3_r101_150x256_scale1_vs_generic", cap=None)     # identical inputs: the PSPNet tolerance


def test_segmenter_s16_small_frame_against_the_generic_route():
    from flood_uav_video_segmentation_amd.model.vit import VITSegmentModel

    net = VITSegmentModel(5, 704, patch_size=16, d_model=384, n_layers=12, dec_layers=2).eval()
    net.load_state_dict(synth.make_vit_state(5, 704, 16, 384, 12, 2, seed=4))
    ev = SingleFrameEvaluator(net, 5, 704, 704, test_scales=[1.0], arch="vit", base_size=1024, crop_batch=2)
    check_against_generic(ev, smooth_frame(720, 1024, 12).cuda(), "ms_predict_segmenter_s16_720x1024_vs_generic")


def test_evaluator_refuses_what_it_cannot_run(pspnet):
    with pytest.raises(ValueError, match="not a size arch"):
        SingleFrameEvaluator(pspnet, 5, 713, 700)
    with pytest.raises(ValueError, match="unknown arch"):
        SingleFrameEvaluator(pspnet, 5, 713, 713, arch="unet")
    ev = SingleFrameEvaluator(pspnet, 5, 65, 65, base_size=90)
    with pytest.raises(RuntimeError, match="on the GPU"):
        ev.predict(raw_frame(70, 90, 1))
    with pytest.raises(RuntimeError, match="on the GPU"):
        ev.test_step(raw_frame(70, 90, 1).cuda(), torch.zeros((70, 90), dtype=torch.uint8))
