"""Frame egress on the GPU (csrc/egress_ops.hip through the fs_ext_api table, ops.compose_frame, flow.predict.compose_window and
flow.dataset.RawVideoWriter).

Every comparison in this file is an EQUALITY (np.array_equal / torch.equal) against the numpy restatement tests/egress_ref.py: the op
is integer except the resize of the background, which tests/ingest_ref.py restates and tests/test_gpu_ingest.py holds equal to
ops.prepare_frame.  Every GPU step runs once.

Cases of the big comparison: per size and per frame content, EVERY input variant (no background; RGB24; NV12 and I420 under each of
the four matrix / range rows) against EVERY output variant (RGB24; NV12 and I420 under each of the four rows) -- 10 x 9 launches, the
input's and the output's conversion chosen independently.  The restatement's images are computed once per input variant and once
per (input variant, output row) and shared by the launches that must agree on them.
"""
import os

import numpy as np
import pytest
import torch

import egress_ref
import ingest_ref
from flood_uav_video_segmentation_amd import ops, synth
from flood_uav_video_segmentation_amd.flow.dataset import MEAN, STD, RawVideoWindows, RawVideoWriter, raw_frame_bytes
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import PALETTE, FlowPredictor, colorize, compose_window

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROWS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
SIZES = [((1080, 1920), (1072, 1920)), ((1072, 1920), (1072, 1920)), ((720, 1280), (1072, 1920)), ((50, 70), (33, 47)), ((17, 19), (17, 19)),
         ((1, 1), (1, 1)), ((1, 1), (3, 5))]
K = 6
# one opacity of {0, 1, 127, 128, 254, 255} per class
PAL = np.array([[0, 0, 0, 128], [30, 95, 170, 0], [65, 117, 5, 1], [212, 98, 1, 127], [255, 244, 116, 254], [255, 255, 255, 255]], dtype=np.uint8)


def frames_of(h, w, seed):
    """noise, all 0, all 255, and the tie-rich ramp of the ingest tests"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    ramp = np.stack([(yy + xx) % 256, (2 * yy + 3 * xx + 1) % 256, (255 - yy) % 256], axis=-1).astype(np.uint8)
    return {"noise": rng.randint(0, 256, (h, w, 3)).astype(np.uint8), "zeros": np.zeros((h, w, 3), np.uint8),
            "full": np.full((h, w, 3), 255, np.uint8), "ramp": ramp}


def mask_of(h, w, seed):
    """random classes 0..K-1, with ids >= K (K, K + 1, 200, 255) sprinkled in"""
    rng = np.random.RandomState(seed)
    pick = np.array(list(range(K)) * 3 + [K, K + 1, 200, 255], dtype=np.uint8)
    mask = pick[rng.randint(0, len(pick), (h, w))]
    if mask.size >= 8:
        mask.reshape(-1)[1:5] = [K, K + 1, 200, 255]                        # present whatever the draw
    return mask


def planes_of(img):
    """Y, U, V planes cut out of an RGB test picture (any bytes do: the tests compare routes, not colours)."""
    return np.ascontiguousarray(img[..., 0]), np.ascontiguousarray(img[::2, ::2, 1]), np.ascontiguousarray(img[::2, ::2, 2])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


OUT_VARIANTS = [("rgb24", "bt601", False)] + [(f, m, r) for f in ("nv12", "i420") for m, r in ROWS]


def first_difference(got, want):
    bad = got != want
    i = int(np.argmax(bad))
    return f"{int(bad.sum())} of {got.size} bytes differ, first at byte {i}: got {int(got[i])}, want {int(want[i])}"


@pytest.mark.parametrize("src, dst", SIZES)
def test_every_input_against_every_output_equals_the_restatement(src, dst):
    h, w = dst
    mask = mask_of(h, w, seed=h * 3 + w)
    assert (mask >= K).any() or mask.size < 8
    m = dev(mask)
    for name, img in frames_of(src[0], src[1], seed=src[0] + src[1]).items():
        y, u, v = planes_of(img)
        f, ty, tu, tv = dev(img), dev(y), dev(u), dev(v)
        tuv = torch.stack([tu, tv], dim=-1).contiguous()
        inputs = [("none", None, None)] + [("rgb24", None, None)] + [(fmt, mx, fr) for fmt in ("nv12", "i420") for mx, fr in ROWS]
        blended, packed = {}, {}
        for fmt, mx, fr in inputs:
            key = fmt if fmt in ("none", "rgb24") else ("yuv", mx, fr)         # NV12 and I420 of the same planes are the same picture
            if key not in blended:
                bg = None if fmt == "none" else egress_ref.background(img, size=dst) if fmt == "rgb24" else \
                    egress_ref.background(y, (u, v), "i420", mx, fr, size=dst)
                blended[key] = egress_ref.blend(mask, PAL, bg)
            for ofmt, omx, ofr in OUT_VARIANTS:
                pkey = (key, "rgb24") if ofmt == "rgb24" else (key, omx, ofr)
                if pkey not in packed:
                    packed[pkey] = egress_ref.pack(blended[key], "i420" if ofmt != "rgb24" else "rgb24", omx, ofr)
                want = packed[pkey]
                if ofmt == "nv12":
                    n = h * w
                    c = (len(want) - n) // 2
                    want = np.concatenate([want[:n], np.stack([want[n:n + c], want[n + c:]], axis=-1).reshape(-1)])
                out = torch.empty(raw_frame_bytes(h, w, ofmt), dtype=torch.uint8, device="cuda")
                if fmt == "none":
                    res = ops.compose_frame(m, PAL, out_fmt=ofmt, out_matrix=omx, out_full_range=ofr, out=out)
                else:
                    frame, chroma = (f, None) if fmt == "rgb24" else (ty, tuv) if fmt == "nv12" else (ty, (tu, tv))
                    res = ops.compose_frame(m, PAL, frame, chroma, fmt, mx or "bt601", bool(fr), ofmt, omx, ofr, out=out)
                got = out.cpu().numpy()
                assert got.shape == want.shape, (got.shape, want.shape)
                assert np.array_equal(got, want), f"{name} {src} -> {dst}, in {fmt} {mx} {fr}, out {ofmt} {omx} {ofr}: {first_difference(got, want)}"
                first = res if ofmt == "rgb24" else res[0]
                assert first.data_ptr() == out.data_ptr()                       # the planes are views of the caller's buffer


@pytest.mark.parametrize("shape", [(1072, 1920), (33, 47), (2, 1072, 1920), (1, 1)])
def test_rgb24_without_a_background_equals_colorize(shape):
    masks = dev(np.random.RandomState(5).randint(0, 9, shape).astype(np.uint8))   # ids 5..8 are class 0 in both
    want = colorize(masks)
    for mk, wt in zip(masks.reshape(-1, *shape[-2:]), want.reshape(-1, *shape[-2:], 3)):
        got = ops.compose_frame(mk, PALETTE, out_fmt="rgb24")
        assert got.shape == wt.shape and got.dtype == torch.uint8 and torch.equal(got, wt)
        assert torch.equal(ops.compose_frame(mk, PALETTE, out_fmt="rgb24", alpha=7), wt)   # no background: the colour whatever A


@pytest.mark.parametrize("src, dst", [((1080, 1920), (1072, 1920)), ((50, 70), (33, 47)), ((40, 64), (40, 64)), ((33, 47), (50, 70))])
def test_all_transparent_is_the_picture_the_network_saw(src, dst):
    """A = 0 everywhere, RGB24 out: ingest_ref's resized uint8 image -- which is ops.prepare_frame's output de-normalised."""
    img = frames_of(src[0], src[1], seed=9)["noise"]
    y, u, v = planes_of(img)
    m = dev(mask_of(dst[0], dst[1], seed=10))
    mean, std = torch.tensor(MEAN, device="cuda").view(3, 1, 1), torch.tensor(STD, device="cuda").view(3, 1, 1)
    for fmt, frame, chroma, mx, fr in (("rgb24", dev(img), None, "bt601", False), ("i420", dev(y), (dev(u), dev(v)), "bt709", False),
                                       ("nv12", dev(y), torch.stack([dev(u), dev(v)], dim=-1).contiguous(), "bt601", True)):
        got = ops.compose_frame(m, PALETTE, frame, chroma, fmt, mx, fr, out_fmt="rgb24", alpha=0)
        want = egress_ref.background(img if fmt == "rgb24" else y, None if fmt == "rgb24" else (u, v), "rgb24" if fmt == "rgb24" else "i420", mx, fr, dst)
        assert np.array_equal(got.cpu().numpy(), want), (fmt, src, dst)
        prepared = ops.prepare_frame(frame, dst, fmt=fmt, chroma=chroma, matrix=mx, full_range=fr)[0]
        assert torch.equal((prepared * std + mean).round().to(torch.uint8).permute(1, 2, 0), got)
        assert np.array_equal(ingest_ref.prepare_rgb(want), prepared[None].cpu().numpy())


@pytest.mark.parametrize("hw", [(40, 64), (33, 47), (1072, 1920)])
def test_out_slices_at_aligned_and_unaligned_offsets_leave_their_surroundings_alone(hw):
    h, w = hw
    img = frames_of(h + 8, w, seed=12)["noise"]
    mask = mask_of(h, w, seed=13)
    m, f = dev(mask), dev(img)
    blended = egress_ref.blend(mask, PAL, egress_ref.background(img, size=hw))
    plain = egress_ref.blend(mask, PAL, None)
    for ofmt in ("rgb24", "nv12", "i420"):
        n = raw_frame_bytes(h, w, ofmt)
        big = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        for off in (0, 8, 16, 1, 3, 4, 5):
            for bg, pic in ((f, blended), (None, plain)):
                big.fill_(0xA5)
                out = big[off:off + n]
                ops.compose_frame(m, PAL, bg, out_fmt=ofmt, out_matrix="bt709", out_full_range=False, out=out)
                got = big.cpu().numpy()
                want = egress_ref.pack(pic, ofmt, "bt709", False)
                assert np.array_equal(got[off:off + n], want), (ofmt, off, bg is not None, first_difference(got[off:off + n], want))
                assert (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all(), (ofmt, off)
    with pytest.raises(RuntimeError, match="floodseg.*out"):
        ops.compose_frame(m, PAL, out_fmt="nv12", out=torch.empty(raw_frame_bytes(h, w, "nv12") + 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="floodseg.*out"):
        ops.compose_frame(m, PAL, out_fmt="rgb24", out=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"))


def test_repeat_runs_are_identical_and_the_result_feeds_prepare_frame():
    img = frames_of(1080, 1920, seed=14)["noise"]
    y, u, v = planes_of(img)
    ty, tuv = dev(y), torch.stack([dev(u), dev(v)], dim=-1).contiguous()
    m = dev(mask_of(1072, 1920, seed=15))
    runs = [ops.compose_frame(m, PAL, ty, tuv, "nv12", "bt709", False, "nv12") for _ in range(3)]
    for oy, ouv in runs[1:]:
        assert torch.equal(oy, runs[0][0]) and torch.equal(ouv, runs[0][1])
    oy, ouv = runs[0]
    assert oy.shape == (1072, 1920) and ouv.shape == (536, 960, 2)
    again = ops.prepare_frame(oy, (65, 65), fmt="nv12", chroma=ouv, matrix="bt709")          # without reshaping
    want = ingest_ref.prepare_yuv(oy.cpu().numpy(), ouv[..., 0].cpu().numpy(), ouv[..., 1].cpu().numpy(), (65, 65), "bt709", False)
    assert np.array_equal(again.cpu().numpy(), want)
    iy, (iu, iv) = ops.compose_frame(m, PAL, ty, tuv, "nv12", "bt709", False, "i420")
    assert torch.equal(iy, oy) and torch.equal(iu, ouv[..., 0]) and torch.equal(iv, ouv[..., 1])
    ops.prepare_frame(iy, (65, 65), fmt="i420", chroma=(iu, iv), matrix="bt709")


def test_refusals_carry_the_package_s_message():
    m = torch.zeros((16, 20), dtype=torch.uint8, device="cuda")
    f = torch.zeros((16, 20, 3), dtype=torch.uint8, device="cuda")
    y = torch.zeros((16, 20), dtype=torch.uint8, device="cuda")
    uv = torch.zeros((8, 10, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="floodseg.*GPU"):
        ops.compose_frame(m.cpu(), PAL)
    with pytest.raises(RuntimeError, match="floodseg.*GPU"):
        ops.compose_frame(m, PAL, f.cpu())
    with pytest.raises(RuntimeError, match="floodseg.*mask"):
        ops.compose_frame(m.float(), PAL)
    with pytest.raises(RuntimeError, match="floodseg.*mask"):
        ops.compose_frame(f, PAL)
    with pytest.raises(RuntimeError, match="floodseg.*uint8"):
        ops.compose_frame(m, PAL, f.float())
    with pytest.raises(RuntimeError, match="floodseg.*chroma"):
        ops.compose_frame(m, PAL, y, fmt="nv12")
    with pytest.raises(RuntimeError, match="floodseg.*chroma"):
        ops.compose_frame(m, PAL, y, uv[:7], fmt="nv12")
    with pytest.raises(RuntimeError, match="floodseg.*chroma"):
        ops.compose_frame(m, PAL, chroma=uv)
    with pytest.raises(RuntimeError, match=r"floodseg.*\[H,W,3\]"):
        ops.compose_frame(m, PAL, y)
    with pytest.raises(RuntimeError, match="floodseg.*palette"):
        ops.compose_frame(m, np.zeros((5, 2), np.uint8))
    with pytest.raises(RuntimeError, match="floodseg.*palette"):
        ops.compose_frame(m, np.zeros((257, 3), np.uint8))
    with pytest.raises(RuntimeError, match="floodseg.*alpha"):
        ops.compose_frame(m, PALETTE, f)                                     # a [K,3] palette over a background needs its opacity
    with pytest.raises(RuntimeError, match="floodseg.*alpha"):
        ops.compose_frame(m, PALETTE, f, alpha=256)
    with pytest.raises(RuntimeError, match="floodseg.*alpha"):
        ops.compose_frame(m, PAL, f, alpha=3)
    dev_pal = torch.from_numpy(PAL).cuda()                                   # a device palette is taken too
    assert torch.equal(ops.compose_frame(m, dev_pal, f, out_fmt="rgb24"), ops.compose_frame(m, PAL, f, out_fmt="rgb24"))


# ------------------------------------------------------------------------------------------------ end to end
def to_yuv_planes(rgb):
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    return y.astype(np.uint8), u[::2, ::2].astype(np.uint8), v[::2, ::2].astype(np.uint8)


def test_raw_clip_to_result_video_end_to_end(tmp_path):
    """RawVideoWindows -> FlowPredictor -> compose_window -> RawVideoWriter on a small synthetic NV12 clip: the file written equals the
    restatement applied to the masks the predictor returned, over the frames the network saw; and reads back as a raw clip."""
    from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

    class HP:
        layers, classes, pretrained = 50, 5, False

    H, W, size, delta, n = 80, 96, (65, 65), 5, 11
    clip = (synth.make_clip(n, (H, W), seed=43) * 50 + 120).clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()
    planes = [to_yuv_planes(f) for f in clip]
    path = str(tmp_path / "clip.nv12")
    with open(path, "wb") as fh:
        for y, u, v in planes:
            fh.write(y.tobytes() + np.stack([u, v], axis=-1).tobytes())
    ds = RawVideoWindows(path, H, W, "nv12", frame_delta=delta, no_warp=True, size=size, matrix="bt709", full_range=False)
    assert len(ds) == 2
    net = FlowPSPNet(HP()).eval()
    net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
    pred = FlowPredictor(FlowModel(net, feature_based=False, no_warp=True).eval(), classes=5, out_size=size, crop=None, compute_metrics=False)
    pal = np.concatenate([PALETTE, np.array([[64], [160], [160], [96], [128]], dtype=np.uint8)], axis=1)
    overlay, opaque = str(tmp_path / "overlay.nv12"), str(tmp_path / "opaque.yuv")
    all_masks = []
    with RawVideoWriter(overlay, size[0], size[1], "nv12", frames=len(ds) * delta) as wo, RawVideoWriter(opaque, size[0], size[1], "i420") as wp:
        for i in (1, 0):                                                     # window blocks in any order, as two ranks would write them
            item = ds[i]
            masks = pred.predict_window(item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"], to_host=False)
            assert masks.shape == (delta, 65, 65)
            all_masks.append((item["frame_id"], masks.cpu().numpy()))
            for p, buf in enumerate(compose_window(masks, item, pal, out_fmt="nv12", out_matrix="bt709", dataset=ds)):
                wo.write(item["frame_id"] + p, buf)
        for first, masks in sorted(all_masks, key=lambda t: t[0]):          # the reference's video: opaque colours, in order
            for p, buf in enumerate(compose_window(torch.from_numpy(masks).cuda(), None, PALETTE, out_fmt="i420", out_matrix="bt601", out_full_range=True)):
                wp.write(first + p, buf)
    nb = raw_frame_bytes(65, 65, "nv12")
    got = np.fromfile(overlay, dtype=np.uint8).reshape(len(ds) * delta, nb)
    plain = np.fromfile(opaque, dtype=np.uint8).reshape(len(ds) * delta, nb)
    for first, masks in all_masks:
        for p in range(delta):
            y, u, v = planes[first + p]
            bg = egress_ref.background(y, (u, v), "i420", "bt709", False, size)
            want = egress_ref.compose(masks[p], pal, bg, "nv12", "bt709", False)
            assert np.array_equal(got[first + p], want), (first + p, first_difference(got[first + p], want))
            assert np.array_equal(plain[first + p], egress_ref.compose(masks[p], np.concatenate([PALETTE, np.full((5, 1), 255, np.uint8)], axis=1),
                                                                       None, "i420", "bt601", True))
    assert not np.array_equal(got[0], got[5]) and not np.array_equal(got[0, :65 * 65], plain[0, :65 * 65])   # the footage shows through every class
    back = RawVideoWindows(overlay, 65, 65, "nv12", frame_delta=delta, no_warp=True)
    assert back.frames == len(ds) * delta and len(back) == 2
    item = back[0]
    y0, uv0 = back.planes(0)
    assert np.array_equal(np.concatenate([y0.cpu().numpy().ravel(), uv0.cpu().numpy().ravel()]), got[0])
    assert item["frame_prev"].shape == (1, 3, 65, 65)
