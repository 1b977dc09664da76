"""Block motion estimation on the GPU (csrc/motion_ops.hip through the fs_test_api table, ops.block_match, flow/motion.py, the
window datasets' grids="estimate" and tools/estimate_grids.py).

The arithmetic is integer, so every comparison against the CPU restatement (tests/motion_ref.py) is an EQUALITY: no tolerance in
this file but LOGIT_TOL, which is the one tests/test_gpu_net.py asserts for the 65 x 65 PSPNet against the oracle and applies to
the network behind the estimated grids, not to the estimator.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import motion_ref
from conftest import note, rel_err
from flood_uav_video_segmentation_amd import _lib, ops, synth
from flood_uav_video_segmentation_amd._lib import ptr, stream_ptr
from flood_uav_video_segmentation_amd.flow import motion
from flood_uav_video_segmentation_amd.flow.dataset import PredictWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel, get_default_grid
from oracle import flow_oracle, pspnet_oracle
from oracle.crops_oracle import motion_vectors_to_grids
from test_gpu_net import LOGIT_TOL

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_match(cur, ref, search, penalty=0):
    """The table entry itself: numpy uint8 frames -> (table, cost) numpy."""
    lib = _lib.load()
    c, r = torch.from_numpy(np.ascontiguousarray(cur)).cuda(), torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    h, w = cur.shape[:2]
    n = (h // 16) * (w // 16)
    mv = torch.full((n, 7), -12345, dtype=torch.int32, device="cuda")
    cost = torch.full((n,), -12345, dtype=torch.int32, device="cuda")
    rc = lib.fs_block_match(ptr(c), ptr(r), h, w, 3 if cur.ndim == 3 else 1, search, penalty, ptr(mv), ptr(cost), stream_ptr())
    assert rc == 0, lib.fs_last_error()
    torch.cuda.synchronize()
    return mv.cpu().numpy(), cost.cpu().numpy()


def check_pair(cur, ref, search, penalty=0, what=""):
    """GPU == restatement, table and cost; an RGB pair also as the luma planes the definition reduces it to."""
    want_t, want_c = motion_ref.block_match(cur, ref, search, penalty)
    inputs = [(cur, ref)] + ([(motion_ref.luma(cur), motion_ref.luma(ref))] if cur.ndim == 3 else [])
    for c, r in inputs:
        got_t, got_c = gpu_match(c, r, search, penalty)
        bad = np.flatnonzero((got_t != want_t).any(axis=1) | (got_c != want_c))
        assert bad.size == 0, (f"{what} {c.shape} R={search} lambda={penalty}: {bad.size} of {len(want_c)} blocks differ, first {bad[0]}: "
                               f"got {got_t[bad[0]].tolist()} cost {got_c[bad[0]]}, want {want_t[bad[0]].tolist()} cost {want_c[bad[0]]}")
    return want_t, want_c


def planted_per_block(h, w, search, seed, channels=1):
    """(cur, ref): noise reference, and a current frame whose every block is a copy of the reference window at a vector of its own."""
    rng = np.random.RandomState(seed)
    ref = motion_ref.noise_frame(h, w, seed, channels)
    cur = motion_ref.noise_frame(h, w, seed + 1, channels)
    for by in range(h // 16):
        for bx in range(w // 16):
            dx = rng.randint(max(-search, -bx * 16), min(search, w - 16 - bx * 16) + 1)
            dy = rng.randint(max(-search, -by * 16), min(search, h - 16 - by * 16) + 1)
            cur[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = ref[by * 16 + dy:by * 16 + dy + 16, bx * 16 + dx:bx * 16 + dx + 16]
    return cur, ref


# ------------------------------------------------------------------------------------------------ the kernel against the restatement
@pytest.mark.parametrize("h", [1072, 1080])
def test_full_frames_at_search_16(h):
    """The product geometry (1080 = 67 * 16 + 8: the remainder strip is searched but owns no block), RGB and luma input."""
    cur, ref = planted_per_block(h, 1920, 16, seed=h, channels=3)
    cur[:, 960:] = motion_ref.noise_frame(h, 960, seed=h + 5, channels=3)   # right half: unrelated noise, minima far from zero
    table, cost = check_pair(cur, ref, 16, 0, "full frame")
    assert (cost[np.arange(len(cost)) % 120 < 60] == 0).all() and cost.max() > 10000


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("hw", [(50, 70), (16, 16), (16, 200), (130, 16)])
def test_small_and_odd_frames(hw, channels):
    """Widths that are no multiple of 4 (byte-wise staging), one-block frames (only (0, 0) is in frame), a partial last workgroup."""
    h, w = hw
    for search in (3, 16):
        check_pair(motion_ref.noise_frame(h, w, 3, channels), motion_ref.noise_frame(h, w, 4, channels), search, 0, "noise")
    if hw == (16, 16):
        t, _ = gpu_match(motion_ref.noise_frame(16, 16, 3), motion_ref.noise_frame(16, 16, 4), 32)
        assert t.tolist() == [[-1, 16, 16, 8, 8, 8, 8]]


@pytest.mark.parametrize("search", [1, 7, 16, 32])
@pytest.mark.parametrize("penalty", [0, 4, 255])
def test_search_ranges_and_penalties(search, penalty):
    h, w = 160, 240
    check_pair(motion_ref.noise_frame(h, w, 10 + search), motion_ref.noise_frame(h, w, 20 + search), search, penalty, "noise")
    cur, ref = planted_per_block(h, w, search, seed=30 + search, channels=3)
    table, cost = check_pair(cur, ref, search, penalty, "planted")
    if penalty == 0:
        assert not cost.any()
    # a smooth scene with a small pan: near-minima everywhere, the penalty decides many blocks
    base = (synth.make_clip(1, (h + 8, w + 8), seed=7)[0, 0] * 40 + 128).clamp(0, 255).byte().numpy()
    check_pair(np.ascontiguousarray(base[3:3 + h, 5:5 + w]), np.ascontiguousarray(base[:h, :w]), search, penalty, "smooth")


@pytest.mark.parametrize("search", [7, 16, 32])
@pytest.mark.parametrize("penalty", [0, 4, 255])
def test_exact_ties_follow_the_order_of_the_definition(search, penalty):
    """Constant frames and 2-pixel stripes: hundreds of candidates share the minimum; (cost, |dx| + |dy|, dy, dx) decides."""
    h, w = 160, 240
    flat = np.full((h, w), 200, dtype=np.uint8)
    table, cost = check_pair(flat, flat.copy(), search, penalty, "flat")
    vx, vy = motion_ref.vectors(table)
    assert not vx.any() and not vy.any() and not cost.any()
    stripes = np.tile(((np.arange(w) // 2) % 2 * 255).astype(np.uint8), (h, 1))
    for cur, ref in ((stripes, stripes.copy()), (stripes, np.roll(stripes, 2, axis=1)), (stripes, np.roll(stripes, 1, axis=1)),
                     (stripes.T.copy(), np.roll(stripes, 2, axis=1).T.copy()), (stripes, flat)):
        check_pair(np.ascontiguousarray(cur), np.ascontiguousarray(ref), search, penalty, "stripes")


@pytest.mark.parametrize("penalty", [0, 255])
def test_saturated_frames_reach_the_largest_cost(penalty):
    """0 against 255 in every pixel: SAD = 256 * 255 = 65280 needs all 16 bits of a packed accumulator (and a current pixel of 0
    must count like any other: the masked SAD instructions leave it out)."""
    h, w = 96, 128
    yy, xx = np.mgrid[:h, :w]
    zero, full = np.zeros((h, w), dtype=np.uint8), np.full((h, w), 255, dtype=np.uint8)
    table, cost = check_pair(zero, full, 16, penalty, "0 vs 255")
    assert (cost == 65280).all() and not np.any(motion_ref.vectors(table))
    table, cost = check_pair(full, zero, 16, penalty, "255 vs 0")
    assert (cost == 65280).all()
    for cell in (1, 8, 16):
        board = (((yy // cell) + (xx // cell)) % 2 * 255).astype(np.uint8)
        check_pair(board, 255 - board, 16, penalty, f"checkerboard {cell}")
        check_pair(np.stack([board, 255 - board, board], axis=-1), np.stack([255 - board, board, 255 - board], axis=-1), 32, penalty, f"rgb checkerboard {cell}")


def test_python_wrapper_returns_the_same_table():
    cur, ref = planted_per_block(80, 112, 16, seed=77, channels=3)
    want_t, want_c = motion_ref.block_match(cur, ref, 16, 2)
    c, r = torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda()
    mv, cost = ops.block_match(c, r, search=16, penalty=2, return_cost=True)
    assert mv.dtype == torch.int32 and mv.shape == (35, 7) and np.array_equal(mv.cpu().numpy(), want_t) and np.array_equal(cost.cpu().numpy(), want_c)
    assert torch.equal(ops.block_match(c, r, 16, 2), mv) and torch.equal(motion.estimate_motion_vectors(c, r, 16, 2), mv)
    # a non-contiguous view is made dense, not misread
    wide = torch.zeros((80, 112, 4), dtype=torch.uint8, device="cuda")
    wide[..., :3] = c
    assert torch.equal(ops.block_match(wide[..., :3], r, 16, 2), mv)
    with pytest.raises(RuntimeError):
        ops.block_match(c, r[:64])
    with pytest.raises(RuntimeError):
        ops.block_match(c.float(), r.float())
    with pytest.raises(RuntimeError):
        ops.block_match(c, r.cpu())
    with pytest.raises(RuntimeError, match="search"):
        ops.block_match(c, r, search=33)


def test_argument_errors_return_non_zero_with_a_message():
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    for args, word in (((None, fake, 64, 64, 1, 16, 0, fake, None), b"null"), ((fake, fake, 64, 64, 1, 0, 0, fake, None), b"search"),
                       ((fake, fake, 64, 64, 1, 33, 0, fake, None), b"search"), ((fake, fake, 64, 64, 1, 16, 256, fake, None), b"penalty"),
                       ((fake, fake, 15, 64, 1, 16, 0, fake, None), b"smaller"), ((fake, fake, 64, 64, 4, 16, 0, fake, None), b"channels"),
                       ((fake, fake, 1 << 15, 1 << 15, 3, 16, 0, fake, None), b"too large")):
        assert lib.fs_block_match(*args, None) != 0 and word in lib.fs_last_error(), args


# ------------------------------------------------------------------------------------------------ table -> grids
def pan_pair(h, w, dx, dy, seed):
    ref = motion_ref.noise_frame(h, w, seed, 3)
    return motion_ref.shifted_copy(ref, dx, dy, seed=seed), ref


def test_estimate_grids_equals_the_oracle_on_the_restatement_table():
    h, w = 1080, 1920
    cur, ref = planted_per_block(h, w, 16, seed=9, channels=3)
    table, _ = motion_ref.block_match(cur, ref, 16, 0)
    want_g, want_i = motion_vectors_to_grids(table, h, w, get_default_grid())
    grid, inv = motion.estimate_grids(torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda(), search=16)
    assert grid.dtype == torch.float64 and grid.shape == (67, 120, 2) and inv.shape == (67, 120, 2)
    assert np.array_equal(grid.cpu().numpy(), want_g) and np.array_equal(inv.cpu().numpy(), want_i)
    assert not np.array_equal(want_g, get_default_grid())
    with pytest.raises(RuntimeError, match="67 x 120"):
        motion.estimate_grids(torch.zeros(160, 240, dtype=torch.uint8, device="cuda"), torch.zeros(160, 240, dtype=torch.uint8, device="cuda"))


def test_a_pan_by_one_block_moves_the_default_grid_by_one_block():
    h, w = 1072, 1920
    cur, ref = pan_pair(h, w, 16, 0, seed=4)
    grid, inv = motion.estimate_grids(torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda(), search=16)
    default = get_default_grid()
    assert np.array_equal(grid.cpu().numpy()[:, :-1], default[:, 1:])
    got = inv.cpu().numpy()
    assert np.array_equal(got[:, 1:118, 1], default[:, 1:118, 1]) and np.array_equal(got[:, 1:118, 0], default[:, :117, 0])
    cur, ref = pan_pair(h, w, -5, 7, seed=5)           # |dx|, |dy| < 8: src stays in its block
    grid, inv = motion.estimate_grids(torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda(), search=7)
    assert np.array_equal(grid.cpu().numpy(), default) and np.array_equal(inv.cpu().numpy(), default)


def test_estimate_grids_enqueues_without_a_host_synchronisation():
    """Captured into a HIP graph on a side stream after one warm-up call: a capture fails on any synchronisation or host read."""
    cur, ref = planted_per_block(1080, 1920, 16, seed=13, channels=3)
    c, r = torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda()
    want_g, want_i = motion.estimate_grids(c, r, search=16, penalty=1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            grid, inv = motion.estimate_grids(c, r, search=16, penalty=1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(grid, want_g) and torch.equal(inv, want_i)


# ------------------------------------------------------------------------------------------------ datasets, tool, one window
def write_frames(root, video, n, h=1080, w=1920):
    """n frames of a textured scene whose left and right halves pan differently, a few pixels per frame; lossless PNG data under
    the .jpg names the dataset layout uses (the decoder goes by content)."""
    from PIL import Image

    folder = os.path.join(root, "frames", video, "images")
    os.makedirs(folder)
    rng = np.random.RandomState(3)
    canvas = rng.randint(0, 256, size=(h + 128, w + 128, 3)).astype(np.uint8)
    for i in range(n):
        frame = np.empty((h, w, 3), dtype=np.uint8)
        frame[:, :w // 2] = canvas[2 * i:2 * i + h, 9 * i:9 * i + w // 2]                      # (9, 2) pixels per frame
        frame[:, w // 2:] = canvas[120 - 12 * i:120 - 12 * i + h, w // 2 + i:w // 2 + i + w // 2]  # (1, -12) pixels per frame
        Image.fromarray(frame).save(os.path.join(folder, f"{i}.jpg"), format="PNG", compress_level=1)


def test_estimated_windows_equal_the_files_the_tool_writes_and_a_window_runs_on_them(tmp_path):
    root, video = str(tmp_path), "clip"
    write_frames(root, video, 11)
    est = PredictWindows(root, video, frame_delta=5, size=(65, 65), grids="estimate", search=16, penalty=0)
    assert len(est) == 2
    items = [est[i] for i in range(len(est))]
    default = torch.from_numpy(get_default_grid()).float()
    assert any(not torch.equal(g[0].cpu(), default) for it in items for g in it["mvs_left"] + it["mvs_right"])

    tool = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "estimate_grids.py"), root, video, "--search", "16", "--penalty", "0"],
                          capture_output=True, text=True, timeout=600)
    assert tool.returncode == 0, tool.stderr
    for name in ("grids", "inv_grids"):
        assert sorted(os.listdir(os.path.join(root, "frames", video, name))) == sorted(f"{i}.npy" for i in range(11))
    g0 = np.load(os.path.join(root, "frames", video, "grids", "0.npy"))
    assert g0.dtype == np.float64 and np.array_equal(g0, get_default_grid())      # frame 0: no predecessor
    stamp = os.path.getmtime(os.path.join(root, "frames", video, "grids", "3.npy"))
    again = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "estimate_grids.py"), root, video], capture_output=True, text=True, timeout=600)
    assert again.returncode == 0 and "0 files written" in again.stdout and os.path.getmtime(os.path.join(root, "frames", video, "grids", "3.npy")) == stamp

    files = PredictWindows(root, video, frame_delta=5, size=(65, 65))
    assert len(files) == len(est)
    for i, a in enumerate(items):
        b = files[i]
        assert a.keys() == b.keys() and a["frame_id"] == b["frame_id"] and a["key_ids"] == b["key_ids"]
        assert torch.equal(a["frame_prev"], b["frame_prev"]) and torch.equal(a["frame_next"], b["frame_next"])
        for key in ("mvs_left", "mvs_right"):
            assert len(a[key]) == len(b[key]) == 4
            for x, y in zip(a[key], b[key]):
                assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape == (1, 67, 120, 2) and x.device == y.device
                assert torch.equal(x, y)

    # one warp-mode window of the real network on the estimated grids against the oracle fed with the same grids
    from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet

    class HP:
        layers, classes, pretrained = 50, 5, False

    state = synth.make_pspnet_state(50, 5, seed=0)
    net = FlowPSPNet(HP()).eval()
    net.load_state_dict(state)
    it = items[1]
    fm = FlowModel(net, feature_based=False, no_warp=False).eval()
    out = fm.predict(it["frame_prev"], it["frame_next"], it["mvs_left"], it["mvs_right"], 5, None)["pred"]
    torch.cuda.synchronize()
    enc = lambda x: pspnet_oracle.encoder(x, state, 50)  # noqa: E731
    dec = lambda f: pspnet_oracle.decoder(f, state)  # noqa: E731
    want = flow_oracle.predict_segmentation(enc, dec, it["frame_prev"].cpu(), it["frame_next"].cpu(), [g.cpu() for g in it["mvs_left"]],
                                            [g.cpu() for g in it["mvs_right"]], 5, False)["pred"]
    assert out.shape == want.shape == (5, 5, 65, 65)
    err = note("pspnet_65_window_on_estimated_grids_vs_oracle", rel_err(out.cpu(), want))
    print(f"window on estimated grids vs oracle: max rel {err:.3e}")
    assert err < LOGIT_TOL
