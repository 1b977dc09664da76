"""Frame ingest without a GPU: the restatement's integer YUV -> RGB conversion on hand-checked triples, the raw-video dataset's index
arithmetic and file checks, the boundary the op enters the package by (the extension table behind the frozen test-hook table) and the tool's new switches."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import ingest_ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow.dataset import PredictWindows, RawVideoWindows, raw_frame_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


# ------------------------------------------------------------------------------------------------ the conversion
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_limited_range_white_and_black(matrix):
    assert ingest_ref.yuv_to_rgb(235, 128, 128, matrix, False).tolist() == [255, 255, 255]   # 298 * 219 + 128 = 65390 >> 8 = 255
    assert ingest_ref.yuv_to_rgb(16, 128, 128, matrix, False).tolist() == [0, 0, 0]
    assert ingest_ref.yuv_to_rgb(126, 128, 128, matrix, False).tolist() == [128] * 3         # (298 * 110 + 128) >> 8 = 32908 >> 8
    # below black and above white clip instead of wrapping
    assert ingest_ref.yuv_to_rgb(0, 128, 128, matrix, False).tolist() == [0, 0, 0]           # (298 * -16 + 128) >> 8 = -19 -> 0
    assert ingest_ref.yuv_to_rgb(255, 128, 128, matrix, False).tolist() == [255, 255, 255]   # 278 -> 255


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_full_range_is_the_identity_on_greys(matrix):
    y = np.arange(256, dtype=np.uint8)
    grey = ingest_ref.yuv_to_rgb(y, np.full(256, 128, np.uint8), np.full(256, 128, np.uint8), matrix, True)
    assert np.array_equal(grey, np.stack([y, y, y], axis=-1))


def test_hand_checked_colours():
    # BT.601 limited, Y = 81, U = 90, V = 240 (the studio-range red): c = 298 * 65 = 19370, d = -38, e = 112
    #   R = (19370 + 45808 + 128) >> 8 = 65306 >> 8 = 255;  G = (19370 + 3800 - 23296 + 128) >> 8 = 2 >> 8 = 0;  B = (19370 - 19608 + 128) >> 8 = -110 >> 8 = -1 -> 0
    assert ingest_ref.yuv_to_rgb(81, 90, 240, "bt601", False).tolist() == [255, 0, 0]
    # BT.601 full, Y = 100, U = 200, V = 50: c = 25600, d = 72, e = -78
    #   R = (25600 - 28002 + 128) >> 8 = -2274 >> 8 = -9 -> 0;  G = (25600 - 6336 + 14274 + 128) >> 8 = 33666 >> 8 = 131;  B = (25600 + 32688 + 128) >> 8 = 58416 >> 8 = 228
    assert ingest_ref.yuv_to_rgb(100, 200, 50, "bt601", True).tolist() == [0, 131, 228]
    # BT.709 limited, Y = 180, U = 100, V = 160: c = 298 * 164 = 48872, d = -28, e = 32
    #   R = (48872 + 14688 + 128) >> 8 = 63688 >> 8 = 248;  G = (48872 + 1540 - 4352 + 128) >> 8 = 46188 >> 8 = 180;  B = (48872 - 15148 + 128) >> 8 = 33852 >> 8 = 132
    assert ingest_ref.yuv_to_rgb(180, 100, 160, "bt709", False).tolist() == [248, 180, 132]
    # BT.709 full, Y = 50, U = 128, V = 255: c = 12800, d = 0, e = 127
    #   R = (12800 + 51181 + 128) >> 8 = 64109 >> 8 = 250;  G = (12800 - 15240 + 128) >> 8 = -2312 >> 8 = -10 -> 0;  B = (12800 + 128) >> 8 = 50
    assert ingest_ref.yuv_to_rgb(50, 128, 255, "bt709", True).tolist() == [250, 0, 50]


@pytest.mark.parametrize("matrix, full_range", ROWS)
def test_saturating_chroma_clips_and_never_wraps(matrix, full_range):
    y, u, v = np.meshgrid(np.arange(0, 256, 5), [0, 1, 127, 128, 129, 254, 255], [0, 1, 127, 128, 129, 254, 255], indexing="ij")
    rgb = ingest_ref.yuv_to_rgb(y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8), matrix, full_range).astype(np.int64)
    ymul, yoff, rv, gu, gv, bu = ingest_ref.COEF[(matrix, full_range)]
    exact = np.stack([ymul * (y - yoff) + rv * (v - 128), ymul * (y - yoff) - gu * (u - 128) - gv * (v - 128), ymul * (y - yoff) + bu * (u - 128)], axis=-1) / 256.0
    assert (rgb[exact <= -0.5] == 0).all() and (rgb[exact >= 255] == 255).all() and (exact <= -0.5).any() and (exact >= 255).any()
    assert np.abs(rgb - np.clip(exact, 0, 255)).max() <= 0.5   # the rounded value of the real-valued formula, nothing else
    # monotone in Y at fixed chroma: a wrapped value would break it
    assert (np.diff(rgb, axis=0) >= 0).all()


def test_chroma_is_replicated_over_odd_sizes():
    rng = np.random.RandomState(0)
    y = rng.randint(0, 256, (5, 7)).astype(np.uint8)
    u, v = rng.randint(0, 256, (2, 3, 4)).astype(np.uint8)
    rgb = ingest_ref.planes_to_rgb(y, u, v, "bt709", True)
    for (py, px) in ((0, 0), (4, 6), (3, 2), (1, 5)):
        assert rgb[py, px].tolist() == ingest_ref.yuv_to_rgb(y[py, px], u[py // 2, px // 2], v[py // 2, px // 2], "bt709", True).tolist()


def test_restated_resize_is_the_identity_at_equal_size_and_exact_on_a_constant():
    img = np.random.RandomState(1).randint(0, 256, (9, 11, 3)).astype(np.uint8)
    assert np.array_equal(ingest_ref.resize_bilinear(img, (9, 11)), img.astype(np.float32))
    flat = np.full((7, 5, 3), 255, dtype=np.uint8)
    out = ingest_ref.prepare_rgb(flat, (13, 4))
    want = ((np.float32(255) - np.asarray(ingest_ref.MEAN, np.float32)) / np.asarray(ingest_ref.STD, np.float32))
    assert out.shape == (1, 3, 13, 4) and out.dtype == np.float32 and np.array_equal(out, np.broadcast_to(want[None, :, None, None], out.shape))


# ------------------------------------------------------------------------------------------------ the raw-video dataset
def test_raw_video_windows_index_arithmetic_and_file_size(tmp_path):
    h, w, n = 6, 10, 13
    assert raw_frame_bytes(h, w, "rgb24") == 180 and raw_frame_bytes(h, w, "nv12") == raw_frame_bytes(h, w, "i420") == 60 + 2 * 15
    assert raw_frame_bytes(5, 7, "nv12") == 35 + 2 * 3 * 4
    data = np.random.RandomState(2).randint(0, 256, (n, raw_frame_bytes(h, w, "i420"))).astype(np.uint8)
    path = str(tmp_path / "clip.yuv")
    data.tofile(path)
    ds = RawVideoWindows(path, h, w, "i420", frame_delta=5, no_warp=True, device="cpu")
    assert len(ds) == 13 // 5 == 2 and ds.frames == 13
    assert ds.indices(0) == (0, 0, 5) and ds.indices(1) == (5, 5, 10)
    assert ds.grid_ids(1) == ([6, 7, 8, 9], [9, 8, 7, 6])
    # the same arithmetic as the folder dataset's (flow/dataset.py:112-146)
    os.makedirs(tmp_path / "frames" / "v" / "images")
    folder = PredictWindows(str(tmp_path), "v", frame_delta=5)
    assert folder.grid_ids(1) == ds.grid_ids(1)
    # ten frames: the last window's next key frame (10) does not exist and is replaced going backward
    data[:10].tofile(path)
    ds10 = RawVideoWindows(path, h, w, "i420", frame_delta=5, no_warp=True, device="cpu")
    assert len(ds10) == 2 and ds10.indices(1) == (5, 5, 9)
    assert ds10.raw_frame(10) is None and ds10.raw_frame(-1) is None
    # the planes are views of the frame's bytes, in the order ffmpeg writes them
    y, (u, v) = ds10.planes(3)
    assert y.shape == (6, 10) and u.shape == v.shape == (3, 5)
    assert np.array_equal(np.concatenate([t.numpy().ravel() for t in (y, u, v)]), data[3])
    assert torch.equal(ds10.raw_frame(3), y)                   # the matcher's input is the Y plane as it is
    nv = RawVideoWindows(path, h, w, "nv12", frame_delta=5, no_warp=True, device="cpu")
    y2, uv = nv.planes(3)
    assert uv.shape == (3, 5, 2) and np.array_equal(uv.numpy().ravel(), data[3, 60:])
    # a file that is not a whole number of frames
    with open(path, "ab") as fh:
        fh.write(b"\0" * 7)
    with pytest.raises(ValueError, match="whole number"):
        RawVideoWindows(path, h, w, "i420", no_warp=True, device="cpu")
    data[:10].tofile(path)
    with pytest.raises(ValueError, match="whole number"):
        RawVideoWindows(path, 7, w, "rgb24", no_warp=True, device="cpu")   # 900 bytes are no whole number of 210-byte frames
    with pytest.raises(ValueError, match="grids"):
        RawVideoWindows(path, h, w, "i420", grids="files", device="cpu")
    with pytest.raises(ValueError, match="pix_fmt"):
        RawVideoWindows(path, h, w, "yuv444p", no_warp=True, device="cpu")
    with pytest.raises(RuntimeError, match="67 x 120"):                    # warp mode keeps the grid producer's geometry
        RawVideoWindows(path, h, w, "i420", device="cpu")


def test_raw_rgb_frames_are_900_bytes_each(tmp_path):
    path = str(tmp_path / "clip.rgb")
    frames = np.random.RandomState(3).randint(0, 256, (5, 6, 10, 3)).astype(np.uint8)
    frames.tofile(path)
    ds = RawVideoWindows(path, 6, 10, "rgb24", frame_delta=2, no_warp=True, device="cpu")
    assert len(ds) == 2 and ds.indices(1) == (2, 2, 4)
    frame, chroma = ds.planes(4)
    assert chroma is None and np.array_equal(frame.numpy(), frames[4])


# ------------------------------------------------------------------------------------------------ library surface
def test_frame_prepare_is_the_first_member_of_the_extension_table():
    """fs_test_api is frozen at block_match (tests/test_motion_cpu.py and tests/test_abi.py pin its last member and its exact size), so
    frame_prepare enters through fs_ext_api, the append-only table the library places right behind it: the same name in the same
    position in the header, in the library's initialiser and in the binding, and the op table itself unchanged."""
    names, ext = _lib.hook_names(), _lib.ext_hook_names()
    assert names[-1] == "block_match" and len(names) == 38 and "frame_prepare" not in names
    assert ext[0] == "frame_prepare" and ext.index("frame_prepare") == 0
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext_api {"):text.index("} fs_ext_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == ext
    assert text.index("} fs_test_api;") < text.index("typedef struct fs_ext_api {") < text.index("typedef struct fs_hook_tables {")
    tables = text[text.index("typedef struct fs_hook_tables {"):text.index("} fs_hook_tables;")]
    assert re.findall(r"\b(fs_[a-z_]+) ([a-z]+);", tables) == [("fs_test_api", "test"), ("fs_ext_api", "ext")]
    src = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read()
    init = src[src.index("static const fs_hook_tables tables = {{"):]
    init = init[:init.index("}};")]
    first, second = init.split("}, {")
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", first, flags=re.M) == ["fs_" + n for n in names]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", second, flags=re.M) == ["fs_" + n for n in ext]
    assert len(_lib.exported_symbols()) == 40 and "fs_frame_prepare" not in _lib.exported_symbols()
    assert "frame_prepare" not in open(os.path.join(ROOT, "include", "floodseg.h")).read()
    lib = _lib.load()
    both = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables)).contents
    assert both.test.size == ctypes.sizeof(_lib.FsTestApi) == ctypes.sizeof(ctypes.c_size_t) + 38 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.FsHookTables.ext.offset == ctypes.sizeof(_lib.FsTestApi)          # directly behind, no padding
    assert both.ext.magic == _lib.EXT_MAGIC == 0x4653455854414231 and both.ext.size == ctypes.sizeof(_lib.FsExtApi) == 16 + 8 * len(ext)
    assert ctypes.cast(both.ext.frame_prepare, ctypes.c_void_p).value
    assert lib.fs_version() == 600 and lib.fs_frame_prepare is not None and lib.fs_block_match is not None


def test_argument_errors_are_refused_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    good = dict(frame=fake, u=fake, v=fake, format=2, matrix=0, full_range=0, H=64, W=64, mean=fake, std=fake, out=fake, h=32, w=32)
    cases = [(dict(frame=None), b"null"), (dict(mean=None), b"null"), (dict(std=None), b"null"), (dict(out=None), b"null"),
             (dict(format=3), b"format"), (dict(format=-1), b"format"), (dict(matrix=2), b"matrix"), (dict(full_range=2), b"range"),
             (dict(H=0), b"empty"), (dict(W=0), b"empty"), (dict(h=0), b"empty"), (dict(w=-3), b"empty"),
             (dict(H=1 << 15, W=1 << 15), b"frame too large"), (dict(h=1 << 15, w=1 << 15), b"output too large"),
             (dict(u=None), b"chroma"), (dict(v=None), b"chroma"), (dict(format=1, u=None), b"chroma")]
    for change, word in cases:
        a = dict(good, **change)
        rc = lib.fs_frame_prepare(a["frame"], a["u"], a["v"], a["format"], a["matrix"], a["full_range"], a["H"], a["W"], a["mean"], a["std"],
                                  a["out"], a["h"], a["w"], None)
        assert rc != 0 and word in lib.fs_last_error(), (change, lib.fs_last_error())


def test_python_surface_refuses_a_cpu_tensor():
    with pytest.raises(RuntimeError, match="GPU"):
        ops.prepare_frame(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="fmt"):
        ops.prepare_frame(torch.zeros(8, 8, 3, dtype=torch.uint8), fmt="yuv444p")


# ------------------------------------------------------------------------------------------------ the tool
def load_tool():
    spec = importlib.util.spec_from_file_location("predict_video_tool", os.path.join(ROOT, "tools", "predict_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parser_takes_the_new_switches(capsys):
    tool = load_tool()
    a = tool.parse_args(["--data-root", "d", "--synthetic-weights"])
    assert a.grids == "files" and a.search == 16 and a.penalty == 0 and a.raw is None              # the defaults are the old behaviour
    a = tool.parse_args(["--data-root", "d", "--synthetic-weights", "--grids", "estimate", "--search", "8", "--penalty", "2"])
    assert (a.grids, a.search, a.penalty) == ("estimate", 8, 2)
    a = tool.parse_args(["--raw", "clip.nv12", "--raw-size", "1080", "1920", "--pix-fmt", "i420", "--matrix", "bt601", "--full-range",
                         "--synthetic-weights"])
    assert (a.raw, a.raw_size, a.pix_fmt, a.matrix, a.full_range, a.grids) == ("clip.nv12", [1080, 1920], "i420", "bt601", True, "estimate")
    a = tool.parse_args(["--raw", "clip.nv12", "--raw-size", "1080", "1920", "--synthetic-weights"])
    assert (a.pix_fmt, a.matrix, a.full_range) == ("nv12", "bt709", False)
    for bad in (["--raw", "c", "--raw-size", "8", "8", "--grids", "files", "--synthetic-weights"], ["--raw", "c", "--synthetic-weights"],
                ["--synthetic-weights"], ["--raw", "c", "--raw-size", "8", "8", "--data-root", "d", "--synthetic-weights"],
                ["--raw", "c", "--raw-size", "8", "8", "--pix-fmt", "yuv444p", "--synthetic-weights"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
    capsys.readouterr()
