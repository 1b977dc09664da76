"""Per-pixel confidence and the per-frame extent report on the GPU: mask_confidence_kernel, canvas_confidence_kernel and
frame_report_kernel (csrc/conf_ops.hip through the third hook table) against the project's own ops, against the numpy restatement
(tests/conf_ref.py), and one window end to end through FlowPredictor(confidence=True) and tools/predict_video.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conf_ref
import motion_modes_ref as modes_ref
from flood_uav_video_segmentation_amd import _lib, ops, synth
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5


def into_guarded(fn, src, n, k, hw, size, offset):
    """Run fs_<fn> with both outputs inside guarded byte buffers at `offset` (odd: the byte-store path even where W % 4 == 0);
    returns (mask, conf) and checks that no guard byte changed."""
    lib = _lib.load()
    count = n * size[0] * size[1]
    bufs = [torch.full((count + 64,), GUARD, dtype=torch.uint8, device=DEV) for _ in range(2)]
    m, c = (b[offset:offset + count] for b in bufs)
    check(getattr(lib, "fs_" + fn)(ptr(src), n, k, hw[0], hw[1], ptr(m), ptr(c), size[0], size[1], stream_ptr()))
    torch.cuda.synchronize()
    for b in bufs:
        assert (b[:offset] == GUARD).all() and (b[offset + count:] == GUARD).all()
    return m.view(n, *size).clone(), c.view(n, *size).clone()


@functools.lru_cache(maxsize=None)
def logits_case(index, amp):
    n, k, hw, size = conf_ref.GEOMETRIES[index]
    x = conf_ref.make_logits(n, k, hw, amp)
    return x, torch.from_numpy(x).to(DEV), conf_ref.mask_confidence(x, size)


@pytest.mark.parametrize("amp", conf_ref.AMPLITUDES)
@pytest.mark.parametrize("index", range(len(conf_ref.GEOMETRIES)))
def test_mask_confidence(index, amp):
    n, k, hw, size = conf_ref.GEOMETRIES[index]
    x, xd, (_, want) = logits_case(index, amp)
    mask, conf = ops.mask_confidence(xd, size)
    assert mask.shape == conf.shape == (n, *size) and mask.dtype == conf.dtype == torch.uint8
    # masks: the project's own ops on the same input
    same = tuple(size) == tuple(hw)
    assert torch.equal(mask, ops.argmax_u8(xd) if same else ops.resize_argmax_u8(xd, size))
    assert torch.equal(ops.mask_confidence(xd)[0], ops.argmax_u8(xd))
    # every store path writes the same bytes and nothing else: 4-byte aligned (dword stores where W % 4 == 0) and odd offsets
    for offset in (4, 1, 3):
        m2, c2 = into_guarded("mask_confidence", xd, n, k, hw, size, offset)
        assert torch.equal(m2, mask) and torch.equal(c2, conf), offset
    # confidence against float64.  |conf - ref| <= 1: the fp32 softmax is within ~1e-6 relative, 255 x that is far below one code, so
    # only a value next to a rounding boundary of 255 p can move, and by one.  At most 1 % of the pixels may differ at all: a
    # condition on the kernel, not a measurement -- tests/test_conf_cpu.py shows that torch's fp32 softmax on the CPU meets it on
    # these inputs (conf_ref.SEED), so the inputs do not put more pixels than that next to a boundary.
    diff = (conf.cpu().numpy().astype(np.int64) - want.astype(np.int64))
    print(f"mask_confidence {conf_ref.GEOMETRIES[index]} x{amp}: max |diff| {np.abs(diff).max()}, differing {np.mean(diff != 0):.5f}")
    assert np.abs(diff).max() <= 1 and np.mean(diff != 0) <= 0.01
    # confidence, bit for bit against the project's own softmax: fs_softmax_accumulate of the same logits on a zeroed canvas
    if same:
        canvas = torch.zeros((n, k, *hw), dtype=torch.float64, device=DEV)
        count = torch.zeros(hw, dtype=torch.float64, device=DEV)
        check(_lib.load().fs_softmax_accumulate(ptr(xd), n, k, hw[0], hw[1], ptr(canvas), ptr(count), hw[0], hw[1], 0, 0, stream_ptr()))
        top = canvas.cpu().numpy().astype(np.float32)                     # exact: each entry is 0 + (double)(an fp32 probability)
        with np.errstate(invalid="ignore"):
            top = np.fmax.reduce(np.where(np.isnan(top).any(1, keepdims=True), np.float32(np.nan), top), axis=1)
            want_bits = np.where(np.isnan(top), 0, np.rint(np.float32(255) * top)).astype(np.uint8)
        assert np.array_equal(conf.cpu().numpy(), want_bits)


def test_mask_confidence_full_frame_index_range():
    """(5, 5, 1072 x 1920), identity: the index range of the headline frame (dword stores, 8 workgroups per row, 5 frames)."""
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((5, 5, 1072, 1920), device=DEV, generator=g) * 3
    mask, conf = ops.mask_confidence(x)
    assert torch.equal(mask, ops.argmax_u8(x))
    want = torch.softmax(x, 1).amax(1)                                      # torch's fp32 softmax: within one code of any other fp32 one
    diff = (conf.to(torch.int32) - (want * 255).round().to(torch.int32)).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) <= 0.01
    rep = ops.frame_report(mask, conf, 5, 128).cpu().numpy()
    assert (rep[:, :, 0].sum(1) == 1072 * 1920).all()
    assert np.array_equal(rep[:, :, 0], np.stack([np.bincount(m.reshape(-1), minlength=5) for m in mask.cpu().numpy()]))
    assert rep[:, :, 1].sum() == int(conf.sum(dtype=torch.int64)) and rep[:, :, 2].sum() == int((conf < 128).sum())


@pytest.mark.parametrize("index", range(len(conf_ref.GEOMETRIES)))
def test_canvas_confidence(index):
    n, k, hw, size = conf_ref.GEOMETRIES[index]
    p = conf_ref.make_canvas(n, k, hw)
    pd = torch.from_numpy(p).to(DEV)
    mask, conf = ops.canvas_confidence(pd, size)
    assert torch.equal(mask, ops.canvas_resize_argmax(pd, size))
    want_mask, want = conf_ref.canvas_confidence(p, size)
    if tuple(size) == tuple(hw):
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(conf.cpu().numpy(), want)
        assert all(torch.equal(a, b) for a, b in zip(ops.canvas_confidence(pd), (mask, conf)))
    else:
        assert np.abs(conf.cpu().numpy().astype(np.int64) - want.astype(np.int64)).max() <= 1
    for offset in (4, 3):
        m2, c2 = into_guarded("canvas_confidence", pd, n, k, hw, size, offset)
        assert torch.equal(m2, mask) and torch.equal(c2, conf), offset


def report_inputs(n, hw, top, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, top, (n,) + hw, dtype=np.uint8), rng.integers(0, 256, (n,) + hw, dtype=np.uint8)


@pytest.mark.parametrize("k", [1, 5, 255])
def test_frame_report_equals_numpy(k):
    # 131 x 253 = 33143 pixels: three 16384-pixel workgroups per frame, the last one short; ids up to 255 (>= K for K = 1 and 5)
    m, c = report_inputs(3, (131, 253), 256 if k < 255 else 255, 11 + k)
    m[0, :5] = 0
    md, cd = torch.from_numpy(m).to(DEV), torch.from_numpy(c).to(DEV)
    for low in (0, 128, 255):
        got = ops.frame_report(md, cd, k, low).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, conf_ref.frame_report(m, c, k, low)), (k, low)
    got = ops.frame_report(md, None, k).cpu().numpy()
    assert np.array_equal(got, conf_ref.frame_report(m, None, k)) and not got[:, :, 1:].any()
    if k < 255:
        assert (got[:, :, 0].sum(1) < 131 * 253).all()                      # ids >= K are counted nowhere
    # odd byte addresses, a single pixel
    buf = torch.zeros(m.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = md.reshape(-1)
    assert np.array_equal(ops.frame_report(buf[1:].view(md.shape), None, k).cpu().numpy(), conf_ref.frame_report(m, None, k))
    one = torch.full((1, 1, 1), 0, dtype=torch.uint8, device=DEV)
    assert ops.frame_report(one, one + 7, k, 8).cpu().numpy()[0, 0].tolist() == [1, 7, 1]


def test_frame_report_writes_its_output_whole_also_in_a_graph():
    k = 5
    m1, c1 = report_inputs(2, (37, 41), 7, 1)
    m2, c2 = report_inputs(2, (37, 41), 4, 2)
    md, cd = torch.from_numpy(m1).to(DEV), torch.from_numpy(c1).to(DEV)
    out = torch.full((2, k, 3), -12345, dtype=torch.int64, device=DEV)          # never cleared by the caller
    assert ops.frame_report(md, cd, k, 128, out=out) is out
    assert np.array_equal(out.cpu().numpy(), conf_ref.frame_report(m1, c1, k, 128))
    ops.frame_report(torch.from_numpy(m2).to(DEV), torch.from_numpy(c2).to(DEV), k, 128, out=out)  # a second call into the same buffer
    assert np.array_equal(out.cpu().numpy(), conf_ref.frame_report(m2, c2, k, 128))
    # a captured graph replayed on new masks gives that replay's figures
    ops.frame_report(md, cd, k, 128, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.frame_report(md, cd, k, 128, out=out)
    for m, c in ((m2, c2), (m1, c1), (m2, c2)):
        md.copy_(torch.from_numpy(m))
        cd.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), conf_ref.frame_report(m, c, k, 128))


def test_ops_refusals_on_the_device():
    x = torch.zeros((1, 5, 4, 4), device=DEV)
    for bad in (x.double(), x[0], torch.zeros((1, 33, 4, 4), device=DEV)):
        with pytest.raises(RuntimeError):
            ops.mask_confidence(bad)
    with pytest.raises(RuntimeError):
        ops.canvas_confidence(x)
    with pytest.raises(RuntimeError):
        ops.mask_confidence(x, (0, 4))
    m = torch.zeros((2, 4, 4), dtype=torch.uint8, device=DEV)
    for kw in (dict(conf=m[:1]), dict(conf=m.float()), dict(classes=0), dict(classes=256), dict(low=256), dict(out=torch.zeros((2, 5, 3), device=DEV))):
        with pytest.raises(RuntimeError):
            ops.frame_report(m, **kw)
    with pytest.raises(RuntimeError):
        ops.frame_report(m.float())
    # n == 0: empty outputs, no launch
    mask, conf = ops.mask_confidence(x[:0], (8, 8))
    assert mask.shape == conf.shape == (0, 8, 8) and ops.canvas_confidence(x[:0].double())[1].shape == (0, 4, 4)
    assert ops.frame_report(m[:0]).shape == (0, 5, 3)


# ------------------------------------------------------------------------------------------------ one window, end to end
FH, FW, FRAMES, DELTA = 1072, 1920, 11, 5   # the grid estimator is built for 1072 / 1080 x 1920 frames; the network sees 65 x 65


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    frames = modes_ref.textured_frame(FH + 8 * FRAMES, FW, seed=51, channels=3)
    path = str(tmp_path_factory.mktemp("conf") / "clip.rgb")
    with open(path, "wb") as fh:
        for i in range(FRAMES):
            fh.write(np.ascontiguousarray(frames[8 * i:8 * i + FH]).tobytes())
    return path


@functools.lru_cache(maxsize=None)
def network(arch):
    if arch == "pspnet":
        from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

        class HP:
            layers, classes, pretrained = 50, 5, False

        net = FlowPSPNet(HP()).eval()
        net.load_state_dict(synth.make_pspnet_state(50, 5, seed=0))
    else:  # the smallest Segmenter of tests/test_gpu_vit.py
        from flood_uav_video_segmentation_amd.model.vit import VITSegmentModel

        net = VITSegmentModel(5, 96, patch_size=16, d_model=384, n_layers=2, dec_layers=1).eval()
        net.load_state_dict(synth.make_vit_state(5, 96, 16, 384, 2, 1, seed=5))
    return net


def check_window(fm, item, size, crop, weights=None):
    kw = dict(classes=5, out_size=size, crop=crop, compute_metrics=True, cache_keyframes=False)
    off, on = FlowPredictor(fm, **kw), FlowPredictor(fm, confidence=True, low_confidence=140, **kw)
    args = (item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"])
    plain = off.predict_window(*args, to_host=False, weights=weights)
    masks, conf = on.predict_window(*args, to_host=False, weights=weights)
    assert torch.equal(masks, plain) and conf.shape == masks.shape == (DELTA, *size) and conf.dtype == torch.uint8
    assert int(conf.min()) >= 255 // 5 - 1                                   # the winner of five classes holds at least a fifth
    assert torch.equal(on.hist, off.hist)                                    # the temporal-consistency scoring keeps using the masks
    w = dict(item)
    if weights is not None:
        w["weights"] = weights
    else:
        w.pop("weights", None)
    m2, c2 = next(iter(on.predict_clip([w], to_host=False)))
    assert torch.equal(m2, masks) and torch.equal(c2, conf)
    assert torch.equal(next(iter(off.predict_clip([dict(w)], to_host=False))), plain)
    rep = on.extent_report()
    want = conf_ref.frame_report(masks.cpu().numpy(), conf.cpu().numpy(), 5, 140)
    assert rep.shape == (2 * DELTA, 5, 3) and np.array_equal(rep[:DELTA], want) and np.array_equal(rep[DELTA:], want)
    assert off.extent_report().shape == (0, 5, 3)


@pytest.mark.parametrize("arch,feature", [("pspnet", False), ("pspnet", True), ("vit", True)])
@pytest.mark.parametrize("no_warp", [False, True])
def test_predictor_with_confidence_whole_frame(clip, arch, feature, no_warp):
    size = (65, 65)
    item = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8, no_warp=no_warp)[1]
    fm = FlowModel(network(arch), feature_based=feature, no_warp=no_warp).eval()
    check_window(fm, item, size, None)
    if not no_warp:  # the frame resized on the way out: resize_argmax_u8's route
        on = FlowPredictor(fm, classes=5, out_size=(70, 90), compute_metrics=False, confidence=True)
        off = FlowPredictor(fm, classes=5, out_size=(70, 90), compute_metrics=False)
        args = (item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"])
        assert torch.equal(on.predict_window(*args, to_host=False)[0], off.predict_window(*args, to_host=False))


@pytest.mark.parametrize("no_warp", [False, True])
def test_predictor_with_confidence_sliding_crops_and_hold_weights(clip, no_warp):
    size = (65, 97)                                                          # two overlapping 65 x 65 crops
    item = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8, no_warp=no_warp)[1]
    fm = FlowModel(network("pspnet"), feature_based=False, no_warp=no_warp).eval()
    check_window(fm, item, size, (65, 65))
    if not no_warp:  # hold weights once: a cut at pair 2 of the window, on both routes
        weights = ops.window_weights([None, torch.tensor([40, 30, 1, 0], dtype=torch.int32, device=DEV), None, None, None], DELTA)[0]
        check_window(fm, item, size, (65, 65), weights)
        whole = RawVideoWindows(clip, FH, FW, "rgb24", size=(65, 65), frame_delta=DELTA, grids="estimate", search=8)[1]
        check_window(fm, whole, (65, 65), None, weights)
        # the canvas resized on the way out: canvas_resize_argmax's route
        on = FlowPredictor(fm, classes=5, out_size=(70, 90), crop=(65, 65), compute_metrics=False, confidence=True)
        off = FlowPredictor(fm, classes=5, out_size=(70, 90), crop=(65, 65), compute_metrics=False)
        args = (item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"])
        assert torch.equal(on.predict_window(*args, to_host=False)[0], off.predict_window(*args, to_host=False))


def test_predict_video_writes_the_report_and_the_grey_planes(clip, tmp_path):
    """The command-line tool is what this test is about: one child process, --confidence --report --conf-out on the synthetic clip."""
    size, frames = (65, 65), (FRAMES - 1) // DELTA * DELTA
    csv, grey, out = str(tmp_path / "r.csv"), str(tmp_path / "c.gray"), str(tmp_path / "m.rgb")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "predict_video.py"), "--raw", clip, "--raw-size", str(FH), str(FW), "--pix-fmt", "rgb24",
           "--search", "8", "--synthetic-weights", "--no-cropping", "--size", "65", "65", "--no-metrics", "--raw-out", out, "--out-pix-fmt", "rgb24",
           "--confidence", "--low-confidence", "140", "--report", csv, "--conf-out", grey]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    conf = np.fromfile(grey, np.uint8)
    assert conf.size == frames * size[0] * size[1]
    conf = conf.reshape(frames, -1)
    rgb = np.fromfile(out, np.uint8).reshape(frames, -1, 3)                 # opaque class colours: the masks, through the palette
    from flood_uav_video_segmentation_amd.flow.predict import PALETTE
    masks = np.stack([(rgb == PALETTE[k]).all(-1) for k in range(5)], 1)   # [frames, 5, pixels]
    assert (masks.sum(1) == 1).all()
    lines = open(csv).read().splitlines()
    assert lines[0].split(",")[:4] == ["frame", "area_0", "conf_0", "low_0"] and len(lines) == 1 + frames
    for f, line in enumerate(lines[1:]):
        cells = line.split(",")
        assert int(cells[0]) == f and len(cells) == 16
        for k in range(5):
            sel = masks[f, k]
            px = int(sel.sum())
            assert cells[1 + 3 * k] == f"{px / sel.size:.6f}"
            assert cells[2 + 3 * k] == (f"{int(conf[f][sel].astype(np.int64).sum()) / (255.0 * px):.6f}" if px else "")
            assert cells[3 + 3 * k] == (f"{int((conf[f][sel] < 140).sum()) / px:.6f}" if px else "0.000000")
