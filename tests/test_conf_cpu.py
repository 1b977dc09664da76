"""Per-pixel confidence and the extent report, the parts that need no GPU: the three new members of the third hook table, the
refusals of the library and of the Python surface, the numpy restatement (tests/conf_ref.py) on hand-made cases, the seeds the GPU
test relies on, the CSV writer, the `gray` raw format and the FlowPredictor plumbing on a stub model."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import conf_ref
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow import predict as predict_mod
from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows, RawVideoWriter
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor, write_extent_csv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mask_confidence", "canvas_confidence", "frame_report"]


# ------------------------------------------------------------------------------------------------ library surface
def test_new_members_follow_feat_tail_weighted_in_header_initialiser_and_binding():
    ext2 = _lib.ext2_hook_names()
    assert ext2[4] == "feat_tail_weighted" and ext2[5:8] == NEW
    assert [getattr(_lib.FsExt2Api, n).offset for n in NEW] == [56, 64, 72]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext2_api {"):text.index("} fs_ext2_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body)[:8] == ext2[:8]
    src = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read()
    init = src[src.index("static const fs_hook_tables2 all"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M)[:8] == ["fs_" + n for n in ext2[:8]]
    lib = _lib.load()
    all3 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables2)).contents
    assert all3.ext2.magic == _lib.EXT2_MAGIC and all3.ext2.size >= 80          # from below only: the table grows at its end
    for name in NEW:
        assert ctypes.cast(getattr(all3.ext2, name), ctypes.c_void_p).value and getattr(lib, "fs_" + name) is not None
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + name)                    # table members, not exported symbols
    assert len(_lib.exported_symbols()) == 40 and not any("fs_" + n in _lib.exported_symbols() for n in NEW)
    assert lib.fs_version() == 600
    header = open(os.path.join(ROOT, "include", "floodseg.h")).read()
    assert not any(n in header for n in NEW)


def test_library_refuses_bad_arguments_before_a_launch():
    """Fake non-null pointers: a call that got as far as a launch would fail with another message (or fault on a GPU)."""
    lib = _lib.load()
    fake = 0x1000
    for name in ("mask_confidence", "canvas_confidence"):
        fn = getattr(lib, "fs_" + name)
        kmax = 32 if name == "mask_confidence" else 255

        def call(src=fake, n=2, K=5, h=8, w=8, mask=fake, conf=fake, H=8, W=8):
            return fn(src, n, K, h, w, mask, conf, H, W, None)

        cases = [(dict(src=None), b"null"), (dict(mask=None), b"null"), (dict(conf=None), b"null"), (dict(n=0), b">= 1"), (dict(h=0), b">= 1"),
                 (dict(w=-1), b">= 1"), (dict(H=0), b">= 1"), (dict(W=0), b">= 1"), (dict(n=65536), b"65535"), (dict(K=0), b"out of range"),
                 (dict(K=kmax + 1), b"out of range"), (dict(h=65536, w=32768), b"2^31"), (dict(H=46341, W=46341), b"2^31")]
        for kw, word in cases:
            assert call(**kw) != 0, (name, kw)
            msg = lib.fs_last_error()
            assert word in msg and name.encode() in msg, (name, kw, msg)

    def report(mask=fake, conf=fake, n=2, H=8, W=8, K=5, low=128, out=fake):
        return lib.fs_frame_report(mask, conf, n, H, W, K, low, out, None)

    for kw, word in [(dict(mask=None), b"null"), (dict(out=None), b"null"), (dict(n=0), b">= 1"), (dict(H=0), b">= 1"), (dict(W=0), b">= 1"),
                     (dict(K=0), b"out of range"), (dict(K=256), b"out of range"), (dict(low=-1), b"out of range"), (dict(low=256), b"out of range"),
                     (dict(H=46341, W=46341), b"2^31")]:
        assert report(**kw) != 0, kw
        msg = lib.fs_last_error()
        assert word in msg and b"frame_report" in msg, (kw, msg)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mask_confidence(torch.zeros(1, 5, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.canvas_confidence(torch.zeros(1, 5, 4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_report(torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_report(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_restatement_on_hand_made_cases():
    mask, conf = conf_ref.mask_confidence(np.full((1, 1, 2, 3), -7.5, np.float32))
    assert mask.tolist() == [[[0] * 3] * 2] and conf.tolist() == [[[255] * 3] * 2]                     # K = 1: probability 1
    for k in (2, 3, 5, 7, 32):
        mask, conf = conf_ref.mask_confidence(np.full((1, k, 1, 1), 3.0, np.float32))
        assert mask.item() == 0 and conf.item() == int(np.rint(255 / k))                                # all equal: mask 0, rint(255 / K)
    x = np.zeros((1, 3, 1, 2), np.float32)
    x[0, :, 0, 0] = [0.0, np.log(3.0), 0.0]                                                           # p = (0.2, 0.6, 0.2)
    x[0, 1, 0, 1] = np.nan
    mask, conf = conf_ref.mask_confidence(x)
    assert mask[0, 0].tolist() == [1, 0] and conf[0, 0].tolist() == [153, 0]                           # a NaN gives 0
    x[0, 0, 0, 1] = np.nan                                                                            # NaN in class 0: class 0 stays (argmax_u8's rule)
    assert conf_ref.mask_confidence(x)[0][0, 0, 1] == 0 and conf_ref.mask_confidence(x)[1][0, 0, 1] == 0
    # two equal maxima: the first wins; a resize of a constant map is the constant
    x = np.array([1.0, 4.0, 4.0, -2.0], np.float32).reshape(1, 4, 1, 1)
    assert conf_ref.mask_confidence(x)[0].item() == 1
    up_mask, up_conf = conf_ref.mask_confidence(np.tile(x, (1, 1, 2, 2)), (5, 7))
    assert (up_mask == 1).all() and (up_conf == conf_ref.mask_confidence(x)[1].item()).all()
    # canvas: the winning value itself, in double; half rounds to even; out-of-range values clamp; NaN gives 0
    c = np.array([[np.nan, 0.25, 0.5 / 255, 1.5 / 255, 2.0], [np.nan, 0.75, 0.0, 0.0, -1.0]]).reshape(1, 2, 1, 5)
    mask, conf = conf_ref.canvas_confidence(c)
    assert mask[0, 0].tolist() == [0, 1, 0, 0, 0] and conf[0, 0].tolist() == [0, 191, 0, 2, 255]
    # the values go through the resize arithmetic at equal sizes too: a NaN also reaches the pixel whose zero-weight tap reads it
    c = np.array([[0.25, np.nan], [0.75, 0.5]]).reshape(1, 2, 1, 2)
    mask, conf = conf_ref.canvas_confidence(c)
    assert mask[0, 0].tolist() == [1, 1] and conf[0, 0].tolist() == [191, 128]
    c[0, 1, 0, 1] = np.nan
    assert conf_ref.canvas_confidence(c)[1][0, 0].tolist() == [0, 0]
    mask, conf = conf_ref.canvas_confidence(np.array([0.2, 0.6, 0.2]).reshape(1, 3, 1, 1), (3, 3))
    assert (mask == 1).all() and (conf == 153).all()
    # report: ids >= K are counted nowhere; conf None gives counts only
    m = np.array([[[0, 1, 1], [4, 9, 1]]], np.uint8)
    q = np.array([[[10, 200, 100], [0, 255, 128]]], np.uint8)
    r = conf_ref.frame_report(m, q, classes=5, low=128)
    assert r.shape == (1, 5, 3) and r[0].tolist() == [[1, 10, 1], [3, 428, 1], [0, 0, 0], [0, 0, 0], [1, 0, 1]] and r[0, :, 0].sum() == 5
    assert conf_ref.frame_report(m, None, classes=2)[0].tolist() == [[1, 0, 0], [3, 0, 0]]
    assert conf_ref.frame_report(m, q, classes=5, low=0)[0, :, 2].sum() == 0


def test_seeds_of_the_gpu_test_keep_an_fp32_softmax_inside_the_bound():
    """The GPU test asks |conf - float64 reference| <= 1 everywhere and at most 1 % of the pixels differing at all.  Whether that can be
    met is a property of the INPUTS (how many pixels sit next to a rounding boundary of 255 p), so it is established here with an
    independent fp32 softmax -- torch's on the CPU -- on the very inputs (conf_ref.SEED) the GPU test uses."""
    for n, k, hw, size in conf_ref.GEOMETRIES:
        for amp in conf_ref.AMPLITUDES:
            x = conf_ref.make_logits(n, k, hw, amp)
            v, same = conf_ref.logits_values(x, size)
            mask, want = conf_ref.mask_confidence(x, size)
            p = torch.softmax(torch.from_numpy(v), 1).numpy()
            c = np.take_along_axis(p, mask[:, None].astype(np.int64), axis=1)[:, 0]
            with np.errstate(invalid="ignore"):
                got = np.where(np.isnan(c), 0, np.clip(np.rint(np.float32(255) * c), 0, 255)).astype(np.int64)
            diff = np.abs(got - want.astype(np.int64))
            assert diff.max() <= 1 and (diff != 0).mean() <= 0.01, (n, k, hw, size, amp, diff.max(), (diff != 0).mean())


# ------------------------------------------------------------------------------------------------ CSV and the gray format
def test_extent_csv_and_gray_format(tmp_path):
    report = np.array([[[6, 6 * 255, 0], [2, 255, 1], [0, 0, 0]], [[0, 0, 0], [8, 1020, 8], [0, 0, 0]]], np.int64)
    path = str(tmp_path / "r.csv")
    write_extent_csv(path, [5, 6], report, 8)
    lines = open(path).read().splitlines()
    assert lines[0] == "frame,area_0,conf_0,low_0,area_1,conf_1,low_1,area_2,conf_2,low_2"
    assert lines[1] == "5,0.750000,1.000000,0.000000,0.250000,0.500000,0.500000,0.000000,,0.000000"
    assert lines[2] == "6,0.000000,,0.000000,1.000000,0.500000,1.000000,0.000000,,0.000000" and len(lines) == 3
    write_extent_csv(path, [5, 6], report, 8, with_confidence=False)
    assert open(path).read().splitlines() == ["frame,area_0,area_1,area_2", "5,0.750000,0.250000,0.000000", "6,0.000000,1.000000,0.000000"]
    with pytest.raises(ValueError):
        write_extent_csv(path, [5], report, 8)
    assert ops.raw_frame_bytes(7, 9, "gray") == 63 and ops.raw_frame_bytes(7, 9, "nv12") == 63 + 2 * 4 * 5
    buf = torch.arange(63, dtype=torch.uint8)
    plane, chroma = ops.frame_planes(buf, 7, 9, "gray")
    assert chroma is None and plane.shape == (7, 9) and plane.data_ptr() == buf.data_ptr()
    out = str(tmp_path / "c.gray")
    with RawVideoWriter(out, 7, 9, "gray", frames=3) as wr:
        wr.write(2, buf)
        wr.write(0, buf.flip(0).contiguous())
        with pytest.raises(ValueError):
            wr.write(1, torch.zeros(64, dtype=torch.uint8))
    data = np.fromfile(out, np.uint8)
    assert data.size == 3 * 63 and data[126:].tolist() == list(range(63)) and data[:63].tolist() == list(range(62, -1, -1)) and not data[63:126].any()
    with pytest.raises(ValueError, match="pix_fmt"):
        RawVideoWindows(out, 7, 9, "gray")                                      # an output format only


# ------------------------------------------------------------------------------------------------ FlowPredictor plumbing
class StubFlow(torch.nn.Module):
    """A flow model that returns fixed logits [n,K,H,W] (a foreign network: no fused routes)."""
    feature_based = True
    no_warp = True

    def __init__(self, k=3, hw=(4, 6)):
        super().__init__()
        self.k, self.hw, self.calls = k, hw, 0

    def predict(self, frame_prev, frame_next, mvs_left, mvs_right, n, profiler=None, **extra):
        self.calls += 1
        g = torch.Generator().manual_seed(self.calls)
        return {"pred": torch.randn((n, self.k) + self.hw, generator=g) * 2}


def test_predictor_plumbing_with_a_stub_model(monkeypatch):
    """The ops are replaced by the numpy restatement (they refuse CPU tensors): what is checked is which op is called with what, what
    is returned, and how the report grows across chunk borders."""
    def as_t(pair):
        return tuple(torch.from_numpy(a) for a in pair)

    called = []
    monkeypatch.setattr(ops, "mask_confidence", lambda logits, size=None: (called.append("mc"), as_t(conf_ref.mask_confidence(logits.numpy(), size)))[1])
    monkeypatch.setattr(ops, "resize_argmax_u8", lambda logits, size: (called.append("ra"), as_t(conf_ref.mask_confidence(logits.numpy(), size))[0])[1])

    def report(mask, conf=None, classes=5, low=128, out=None):
        called.append("fr")
        r = torch.from_numpy(conf_ref.frame_report(mask.numpy(), None if conf is None else conf.numpy(), classes, low))
        assert out is not None and out.shape == r.shape and out.is_contiguous()
        out.copy_(r)
        return out

    monkeypatch.setattr(ops, "frame_report", report)
    x = torch.zeros(1, 3, 4, 6)
    grids = [None] * 2                                                           # n = 3
    off = FlowPredictor(StubFlow(), classes=3, out_size=(4, 6), crop=None, compute_metrics=False)
    got = off.predict_window(x, x, grids, grids, to_host=False)
    assert isinstance(got, torch.Tensor) and got.shape == (3, 4, 6) and called == ["ra"]          # off: what it returned, and the op it used
    assert isinstance(off.predict_window(x, x, grids, grids), np.ndarray) and off.extent_report().shape == (0, 3, 3)
    with pytest.raises(ValueError, match="low_confidence"):
        FlowPredictor(StubFlow(), low_confidence=256)

    called.clear()
    monkeypatch.setattr(FlowPredictor, "REPORT_CHUNK", 4)                      # chunk borders inside a window
    on = FlowPredictor(StubFlow(), classes=3, out_size=(4, 6), crop=None, compute_metrics=False, confidence=True, low_confidence=100)
    masks, conf = on.predict_window(x, x, grids, grids, to_host=False)
    assert torch.equal(masks, got) and conf.shape == masks.shape and conf.dtype == torch.uint8  # the same stub call: the same masks
    assert called == ["mc", "fr"]
    kept = [(masks, conf)]
    for _ in range(2):
        m, c = on.predict_window(x, x, grids, grids)
        assert isinstance(m, np.ndarray) and isinstance(c, np.ndarray)
        kept.append((torch.from_numpy(m), torch.from_numpy(c)))
    rep = on.extent_report()
    assert rep.shape == (9, 3, 3) and rep.dtype == np.int64 and len(on._report_chunks) == 3
    want = np.concatenate([conf_ref.frame_report(m.numpy(), c.numpy(), 3, 100) for m, c in kept])
    assert np.array_equal(rep, want) and (rep[:, :, 0].sum(1) == 24).all()
    on.reset()
    assert on.extent_report().shape == (9, 3, 3)                               # reset() keeps the report, as it keeps the histogram
    on.clear_report()
    assert on.extent_report().shape == (0, 3, 3) and on._report_chunks == []
    # predict_clip: a window without key_ids takes predict_window, and yields pairs too
    item = dict(frame_prev=x, frame_next=x, mvs_left=grids, mvs_right=grids)
    (m, c), = list(on.predict_clip([item], to_host=False))
    assert m.shape == c.shape == (3, 4, 6) and on.extent_report().shape == (3, 3, 3)
    assert predict_mod.FlowPredictor.REPORT_CHUNK == 4
