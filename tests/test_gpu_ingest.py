"""Frame ingest on the GPU (csrc/ingest_ops.hip through the fs_ext_api table of fs_test_hooks(), ops.prepare_frame, the window datasets and
RawVideoWindows).

Every comparison in this file is an EQUALITY (torch.equal / np.array_equal):
  * RGB input against the chain PredictWindows._frame ran before this op existed, restated in `old_chain` from torch operations and
    ops.resize_bilinear exactly as it stood (the products of that chain are what the golden tests of the transform chains pin);
  * NV12 / I420 input against the numpy restatement tests/ingest_ref.py (integer conversion, float32 resize in interp.h's order).
"""
import os

import numpy as np
import pytest
import torch

import ingest_ref
from flood_uav_video_segmentation_amd import ops, synth
from flood_uav_video_segmentation_amd.flow import motion
from flood_uav_video_segmentation_amd.flow.dataset import MEAN, STD, EvalWindows, PredictWindows, RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel, get_default_grid
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROWS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


def old_chain(img, size):
    """PredictWindows._frame as it was: uint8 [H,W,3] on the device -> float32 [1,3,h,w]."""
    x = img.permute(2, 0, 1)[None].float()                                             # ToTensor (flow/transform.py:26-51)
    if size is not None and tuple(x.shape[2:]) != tuple(size):
        x = ops.resize_bilinear(x, size, align_corners=False).round_().clamp_(0, 255)   # Resize: cv2.INTER_LINEAR, stored as uint8
    mean = torch.tensor(MEAN, device=img.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=img.device).view(1, 3, 1, 1)
    return (x - mean) / std                                                            # Normalize (:56-86)


def frames_of(h, w, seed):
    """noise, all 0, all 255, and a smooth ramp whose interpolated values land on many .5 ties"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    ramp = np.stack([(yy + xx) % 256, (2 * yy + 3 * xx + 1) % 256, (255 - yy) % 256], axis=-1).astype(np.uint8)
    return {"noise": rng.randint(0, 256, (h, w, 3)).astype(np.uint8), "zeros": np.zeros((h, w, 3), np.uint8),
            "full": np.full((h, w, 3), 255, np.uint8), "ramp": ramp}


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} values differ, first at {i}: got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r}")


# ------------------------------------------------------------------------------------------------ RGB against the present chain
@pytest.mark.parametrize("src, dst", [((1080, 1920), (1072, 1920)), ((1072, 1920), (1072, 1920)), ((1072, 1920), None), ((720, 1280), (1072, 1920)),
                                      ((50, 70), (33, 47)), ((17, 19), (17, 19)), ((1, 1), (1, 1)), ((1, 1), (3, 5)), ((40, 66), (36, 66)),
                                      ((64, 66), None), ((33, 47), (50, 70)), ((48, 64), (1, 1))])
def test_rgb_equals_the_present_chain(src, dst):
    for name, img in frames_of(src[0], src[1], seed=src[0] + src[1]).items():
        if src[0] * src[1] > 100000 and name in ("zeros", "ramp"):
            continue   # the large sizes run noise and the saturated frame
        f = torch.from_numpy(img).cuda()
        want = old_chain(f, dst)
        got = ops.prepare_frame(f, dst)
        assert_same(got, want, f"{name} {src} -> {dst}")
        if name == "noise":   # the restatement agrees with both (it is the reference of the YUV tests below)
            assert np.array_equal(got.cpu().numpy(), ingest_ref.prepare_rgb(img, dst)), f"restatement {src} -> {dst}"


@pytest.mark.parametrize("src, dst", [((1080, 1920), (1072, 1920)), ((50, 70), (33, 47)), ((40, 64), (40, 64)), ((40, 64), (36, 64))])
def test_out_slices_aligned_and_unaligned(src, dst):
    f = torch.from_numpy(frames_of(src[0], src[1], seed=5)["noise"]).cuda()
    g = torch.from_numpy(frames_of(src[0], src[1], seed=6)["noise"]).cuda()
    want_f, want_g = old_chain(f, dst), old_chain(g, dst)
    h, w = dst
    # two key frames in one allocation
    batch = torch.full((2, 3, h, w), float("nan"), device="cuda")
    r0 = ops.prepare_frame(f, dst, out=batch[0])
    r1 = ops.prepare_frame(g, dst, out=batch[1:2])
    assert r0.data_ptr() == batch.data_ptr() and r1.shape == (1, 3, h, w)
    assert_same(batch[0:1], want_f, "batch slot 0")
    assert_same(batch[1:2], want_g, "batch slot 1")
    # a destination that is only 4-byte aligned, with guard values around it
    flat = torch.full((3 * h * w + 9,), -7.0, device="cuda")
    for off in (1, 2, 3):
        flat.fill_(-7.0)
        out = flat[off:off + 3 * h * w].view(3, h, w)
        assert out.data_ptr() % 16 != 0
        ops.prepare_frame(f, dst, out=out)
        assert_same(out[None], want_f, f"offset {off}")
        assert (flat[:off] == -7.0).all() and (flat[off + 3 * h * w:] == -7.0).all()
    with pytest.raises(RuntimeError, match="out"):
        ops.prepare_frame(f, dst, out=torch.empty((1, 3, h, w + 1), device="cuda"))
    with pytest.raises(RuntimeError, match="out"):
        ops.prepare_frame(f, dst, out=torch.empty((1, 3, h, w), device="cuda", dtype=torch.float64))


def test_other_statistics_and_a_non_contiguous_frame():
    img = frames_of(50, 70, seed=8)["noise"]
    f = torch.from_numpy(img).cuda()
    mean, std = [10.0, 20.5, 127.25], [1.0, 3.0, 77.7]
    got = ops.prepare_frame(f, (33, 47), mean=mean, std=std)
    assert np.array_equal(got.cpu().numpy(), ingest_ref.prepare_rgb(img, (33, 47), mean, std))
    wide = torch.zeros((50, 70, 4), dtype=torch.uint8, device="cuda")
    wide[..., :3] = f
    assert torch.equal(ops.prepare_frame(wide[..., :3], (33, 47)), ops.prepare_frame(f, (33, 47)))   # made dense, not misread
    assert torch.equal(ops.prepare_frame(f, (33, 47)), old_chain(f, (33, 47)))                        # the default statistics are still cached apart


# ------------------------------------------------------------------------------------------------ NV12 / I420 against the restatement
def yuv_planes(h, w, seed, extreme=False):
    rng = np.random.RandomState(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if extreme:
        pick = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 254, 255], dtype=np.uint8)
        return pick[rng.randint(0, len(pick), (h, w))], pick[rng.randint(0, len(pick), (ch, cw))], pick[rng.randint(0, len(pick), (ch, cw))]
    return tuple(rng.randint(0, 256, s).astype(np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))


def run_yuv(y, u, v, dst, matrix, full_range):
    """(nv12 result, i420 result) of the same planes."""
    ty, tu, tv = (torch.from_numpy(a).cuda() for a in (y, u, v))
    uv = torch.stack([tu, tv], dim=-1).contiguous()
    a = ops.prepare_frame(ty, dst, fmt="nv12", chroma=uv, matrix=matrix, full_range=full_range)
    b = ops.prepare_frame(ty, dst, fmt="i420", chroma=(tu, tv), matrix=matrix, full_range=full_range)
    return a, b


@pytest.mark.parametrize("matrix, full_range", ROWS)
@pytest.mark.parametrize("src, dst", [((37, 53), None), ((37, 53), (20, 31)), ((37, 53), (41, 53)), ((48, 64), None), ((48, 64), (40, 64)),
                                      ((48, 64), (65, 65)), ((1, 1), (2, 3)), ((2, 1), None), ((1, 6), (1, 6))])
def test_yuv_equals_the_restatement(src, dst, matrix, full_range):
    for extreme in (False, True):
        y, u, v = yuv_planes(src[0], src[1], seed=src[0] * 7 + src[1], extreme=extreme)
        want = ingest_ref.prepare_yuv(y, u, v, dst, matrix, full_range)
        nv12, i420 = run_yuv(y, u, v, dst, matrix, full_range)
        assert torch.equal(nv12, i420), "NV12 and I420 of the same planes"
        got = nv12.cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype
        bad = got != want
        assert not bad.any(), (f"{src} -> {dst} {matrix} full={full_range} extreme={extreme}: {int(bad.sum())} values differ, first "
                               f"{np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, want {want[bad][0]!r}")


@pytest.mark.parametrize("matrix, full_range", ROWS)
@pytest.mark.parametrize("src, dst", [((1080, 1920), (1072, 1920)), ((1072, 1920), None), ((1079, 1917), (1072, 1920))])
def test_yuv_full_frames(src, dst, matrix, full_range):
    y, u, v = yuv_planes(src[0], src[1], seed=src[0], extreme=(matrix == "bt709"))
    want = ingest_ref.prepare_yuv(y, u, v, dst, matrix, full_range)
    nv12, i420 = run_yuv(y, u, v, dst, matrix, full_range)
    assert torch.equal(nv12, i420)
    assert np.array_equal(nv12.cpu().numpy(), want)


def test_yuv_planes_at_odd_addresses():
    """The planes of a raw frame are views at any byte offset of one buffer: Y at an odd address takes the byte route."""
    h, w = 48, 64
    y, u, v = yuv_planes(h, w, seed=11)
    want = ingest_ref.prepare_yuv(y, u, v, (40, 64), "bt709", False)
    buf = torch.zeros(1 + h * w + 2 * (h // 2) * (w // 2), dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(np.concatenate([y.ravel(), u.ravel(), v.ravel()])).cuda()
    ty = buf[1:1 + h * w].view(h, w)
    tu = buf[1 + h * w:1 + h * w + 768].view(24, 32)
    tv = buf[1 + h * w + 768:].view(24, 32)
    assert ty.data_ptr() % 4 == 1
    got = ops.prepare_frame(ty, (40, 64), fmt="i420", chroma=(tu, tv), matrix="bt709")
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_carry_the_library_s_message():
    f = torch.zeros((16, 20, 3), dtype=torch.uint8, device="cuda")
    y = torch.zeros((16, 20), dtype=torch.uint8, device="cuda")
    uv = torch.zeros((8, 10, 2), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="floodseg.*GPU"):
        ops.prepare_frame(f.cpu())
    with pytest.raises(RuntimeError, match="floodseg.*GPU"):
        ops.prepare_frame(y, fmt="nv12", chroma=uv.cpu())
    with pytest.raises(RuntimeError, match="floodseg.*uint8"):
        ops.prepare_frame(f.float())
    with pytest.raises(RuntimeError, match="floodseg.*chroma"):
        ops.prepare_frame(y, fmt="nv12", chroma=uv[:7])
    with pytest.raises(RuntimeError, match="floodseg.*chroma"):
        ops.prepare_frame(y, fmt="nv12")
    with pytest.raises(RuntimeError, match="floodseg.*chroma"):
        ops.prepare_frame(y, fmt="i420", chroma=uv)
    with pytest.raises(RuntimeError, match="floodseg.*chroma"):
        ops.prepare_frame(f, chroma=uv)
    with pytest.raises(RuntimeError, match="floodseg.*fmt"):
        ops.prepare_frame(f, fmt="yuv444p")
    with pytest.raises(RuntimeError, match="floodseg.*matrix"):
        ops.prepare_frame(y, fmt="nv12", chroma=uv, matrix="bt2020")
    with pytest.raises(RuntimeError, match=r"floodseg.*\[H,W,3\]"):
        ops.prepare_frame(y)
    with pytest.raises(RuntimeError, match="floodseg.*size"):
        ops.prepare_frame(f, (0, 5))


# ------------------------------------------------------------------------------------------------ enqueue only
def test_prepare_frame_enqueues_without_a_host_synchronisation():
    """Captured into a HIP graph on a side stream after one warm-up call (which fills the per-device cache of the statistics): a
    capture fails on any synchronisation or host copy.  The replay on new frame contents equals the eager result."""
    a, b = (torch.from_numpy(frames_of(1080, 1920, seed=s)["noise"]).cuda() for s in (21, 22))
    want_a, want_b = ops.prepare_frame(a, (1072, 1920)), ops.prepare_frame(b, (1072, 1920))
    frame = a.clone()
    out = torch.zeros((2, 3, 1072, 1920), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ops.prepare_frame(frame, (1072, 1920), out=out[1])
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[1:2], want_a) and not out[0].any()
    frame.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[1:2], want_b)


# ------------------------------------------------------------------------------------------------ the window datasets
def scene_frames(n, h=1080, w=1920):
    """n uint8 RGB frames of a textured scene whose halves pan differently, a few pixels per frame."""
    rng = np.random.RandomState(3)
    canvas = rng.randint(0, 256, size=(h + 128, w + 128, 3)).astype(np.uint8)
    out = []
    for i in range(n):
        frame = np.empty((h, w, 3), dtype=np.uint8)
        frame[:, :w // 2] = canvas[2 * i:2 * i + h, 9 * i:9 * i + w // 2]
        frame[:, w // 2:] = canvas[120 - 12 * i:120 - 12 * i + h, w // 2 + i:w // 2 + i + w // 2]
        out.append(frame)
    return out


@pytest.fixture(scope="module")
def jpeg_folder(tmp_path_factory):
    """(root, video, frames): lossless PNG data under the .jpg names of the dataset layout (the decoder goes by content), one label."""
    from PIL import Image

    root = str(tmp_path_factory.mktemp("ingest"))
    frames = scene_frames(7)
    folder = os.path.join(root, "frames", "clip", "images")
    os.makedirs(folder)
    for i, fr in enumerate(frames):
        Image.fromarray(fr).save(os.path.join(folder, f"{i}.jpg"), format="PNG", compress_level=1)
    os.makedirs(os.path.join(root, "labels"))
    Image.fromarray((np.arange(1080 * 1920).reshape(1080, 1920) % 5).astype(np.uint8)).save(os.path.join(root, "labels", "3.png"))
    with open(os.path.join(root, "list.txt"), "w") as fh:
        fh.write("labels/3.png clip 3\n")
    return root, "clip", frames


@pytest.mark.parametrize("size", [(1072, 1920), (65, 65), None])
def test_predict_windows_items_equal_the_old_chain_and_the_estimated_grids(jpeg_folder, size):
    root, video, frames = jpeg_folder
    dev_frames = [torch.from_numpy(f).cuda() for f in frames]
    ds = PredictWindows(root, video, frame_delta=5, size=size, grids="estimate", search=16, penalty=1)
    assert len(ds) == 1
    item = ds[0]
    assert item["key_ids"] == (0, 5) and item["frame_id"] == 0
    assert_same(item["frame_prev"], old_chain(dev_frames[0], size), "frame_prev")
    assert_same(item["frame_next"], old_chain(dev_frames[5], size), "frame_next")
    default = torch.from_numpy(get_default_grid()).float()
    for ids, key, which in (([1, 2, 3, 4], "mvs_left", 0), ([4, 3, 2, 1], "mvs_right", 1)):
        assert len(item[key]) == 4
        for g, got in zip(ids, item[key]):
            want = motion.estimate_grids(dev_frames[g], dev_frames[g - 1], search=16, penalty=1)[which].float()[None]
            assert got.dtype == torch.float32 and got.shape == (1, 67, 120, 2) and torch.equal(got, want)
            assert not torch.equal(got[0].cpu(), default)
    # the shared decode: one upload serves the estimator and the transform
    assert ds.raw_frame(5) is ds._decoded(5) and ds.raw_frame(99) is None and ds.raw_frame(-1) is None
    again = ds[0]
    assert torch.equal(again["frame_next"], item["frame_next"]) and all(torch.equal(a, b) for a, b in zip(again["mvs_left"], item["mvs_left"]))
    no_warp = PredictWindows(root, video, frame_delta=5, size=size, no_warp=True, grids="estimate")
    assert torch.equal(no_warp[0]["frame_prev"], item["frame_prev"])


def test_eval_windows_items_equal_the_old_chain_and_the_estimated_grids(jpeg_folder):
    root, video, frames = jpeg_folder
    dev_frames = [torch.from_numpy(f).cuda() for f in frames]
    ds = EvalWindows(root, os.path.join(root, "list.txt"), split="test", frame_delta=3, size=(65, 65), grids="estimate", search=8)
    assert len(ds) == 1
    p = ds.plan(0)
    item = ds[0]
    assert_same(item["frame_prev"], old_chain(dev_frames[p["prev_real"]], (65, 65)), "frame_prev")
    assert_same(item["frame_next"], old_chain(dev_frames[p["next_real"]], (65, 65)), "frame_next")
    default = torch.from_numpy(get_default_grid()).float()[None]
    for ids, key, which in ((p["left_ids"], "mvs_left", 0), (p["right_ids"], "mvs_right", 1)):
        for g, got in zip(ids, item[key]):
            want = default if g is None else motion.estimate_grids(dev_frames[g], dev_frames[g - 1], search=8)[which].float()[None]
            assert torch.equal(got.cpu(), want.cpu())
    assert any(g is not None for g in p["left_ids"] + p["right_ids"])


# ------------------------------------------------------------------------------------------------ raw video files
def test_raw_rgb24_file_gives_the_directly_prepared_frames(tmp_path):
    frames = np.random.RandomState(31).randint(0, 256, (7, 40, 52, 3)).astype(np.uint8)
    path = str(tmp_path / "clip.rgb")
    frames.tofile(path)
    ds = RawVideoWindows(path, 40, 52, "rgb24", frame_delta=3, no_warp=True, size=(33, 47))
    assert len(ds) == 2
    for i in range(2):
        item = ds[i]
        assert item["key_ids"] == (3 * i, 3 * i + 3) and item["frame_id"] == 3 * i and len(item["mvs_left"]) == len(item["mvs_right"]) == 2
        for key, f in (("frame_prev", 3 * i), ("frame_next", 3 * i + 3)):
            direct = ops.prepare_frame(torch.from_numpy(frames[f]).cuda(), (33, 47))
            assert_same(item[key], direct, key)
            assert_same(item[key], old_chain(torch.from_numpy(frames[f]).cuda(), (33, 47)), key + " (old chain)")


def to_yuv_planes(rgb):
    """Some Y, U, V planes for an RGB frame (any plausible forward transform does: the tests compare routes, not colours)."""
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    return y.astype(np.uint8), u[::2, ::2].astype(np.uint8), v[::2, ::2].astype(np.uint8)


def test_raw_nv12_file_grids_come_from_the_y_planes(tmp_path):
    planes = [to_yuv_planes(f) for f in scene_frames(6)]
    path = str(tmp_path / "clip.nv12")
    with open(path, "wb") as fh:
        for y, u, v in planes:
            fh.write(y.tobytes())
            fh.write(np.stack([u, v], axis=-1).tobytes())
    ds = RawVideoWindows(path, 1080, 1920, "nv12", frame_delta=5, size=(65, 65), grids="estimate", search=16, penalty=0, matrix="bt601")
    assert len(ds) == 1
    item = ds[0]
    ys = [torch.from_numpy(p[0]).cuda() for p in planes]
    for ids, key, which in (([1, 2, 3, 4], "mvs_left", 0), ([4, 3, 2, 1], "mvs_right", 1)):
        for g, got in zip(ids, item[key]):
            want = motion.estimate_grids(ys[g], ys[g - 1], search=16, penalty=0)[which].float()[None]
            assert got.shape == (1, 67, 120, 2) and torch.equal(got, want)
    assert not torch.equal(item["mvs_left"][0][0].cpu(), torch.from_numpy(get_default_grid()).float())
    for key, f in (("frame_prev", 0), ("frame_next", 5)):
        y, u, v = planes[f]
        assert np.array_equal(item[key].cpu().numpy(), ingest_ref.prepare_yuv(y, u, v, (65, 65), "bt601", False))


def test_one_no_warp_window_from_a_raw_i420_file_through_the_predictor(tmp_path):
    from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

    class HP:
        layers, classes, pretrained = 50, 5, False

    clip = (synth.make_clip(6, (80, 96), seed=41) * 50 + 120).clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()
    planes = [to_yuv_planes(f) for f in clip]
    path = str(tmp_path / "clip.yuv")
    with open(path, "wb") as fh:
        for y, u, v in planes:
            fh.write(y.tobytes() + u.tobytes() + v.tobytes())
    ds = RawVideoWindows(path, 80, 96, "i420", frame_delta=5, no_warp=True, size=(65, 65), matrix="bt709", full_range=True)
    assert len(ds) == 1
    item = ds[0]
    net = FlowPSPNet(HP()).eval()
    net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
    pred = FlowPredictor(FlowModel(net, feature_based=False, no_warp=True).eval(), classes=5, out_size=(65, 65), crop=None, compute_metrics=False)
    masks = pred.predict_window(item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"], to_host=False)
    direct = []
    for f in (0, 5):
        y, u, v = (torch.from_numpy(a).cuda() for a in planes[f])
        direct.append(ops.prepare_frame(y, (65, 65), fmt="i420", chroma=(u, v), matrix="bt709", full_range=True))
        assert np.array_equal(direct[-1].cpu().numpy(), ingest_ref.prepare_yuv(*planes[f], (65, 65), "bt709", True))
    want = pred.predict_window(direct[0], direct[1], item["mvs_left"], item["mvs_right"], to_host=False)
    assert masks.shape == (5, 65, 65) and masks.dtype == torch.uint8 and torch.equal(masks, want)
    assert not torch.equal(item["frame_prev"], item["frame_next"])
