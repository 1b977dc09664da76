"""Predict-split input side of the hot path: which frames / grids make up window i and how they become the
batch dict FlowBaseModel.predict_step consumes (reference flow/dataset.py:61-64, 80-146, 198-216, 218-240;
transforms flow/base.py:426-431 -> Resize, ToTensor, Normalize of flow/transform.py:26-106).

`PredictWindows` mirrors `split == "predict"`, `EvalWindows` the labelled `val` / `test` splits that feed
validation_step / test_step (flow/base.py:143-176); the random training sampling is out of scope.  Decoding is done with
PIL (the reference uses skimage.io.imread), resize + normalisation run on the GPU in one launch (ops.prepare_frame).
`RawVideoWindows` (extension) yields the same windows from one headerless raw video file (NV12, I420 or RGB24).
"""
import os
import random
from collections import OrderedDict

import numpy as np
import torch

from .. import ops
from .grids import load_grid
from .model import get_default_grid

# base/foundation.py:27-31
MEAN = [0.485 * 255, 0.456 * 255, 0.406 * 255]
STD = [0.229 * 255, 0.224 * 255, 0.225 * 255]


def _grid_source(grids, search, penalty, intra_bias=None, scene_cut=None, **guide):
    """grids="files": the grids/ and inv_grids/ folders (the reference's layout); "estimate": a flow.motion.GridEstimator
    (intra_bias / scene_cut: its inter / intra and scene-cut decisions, both off when None; guide, guide_outlier, guide_bias,
    guide_rounds, guide_tol, guide_min_inliers: its tables guided by the fitted camera motion, off by default)."""
    if grids == "files":
        if guide.get("guide") or guide.get("guide_outlier") is not None or guide.get("guide_bias") is not None:
            raise ValueError('guide needs the estimated grids\' motion-vector tables (grids="estimate"); the grids/ folders hold grids, not vectors')
        return None
    if grids != "estimate":
        raise ValueError(f'grids must be "files" or "estimate", got {grids!r}')
    from .motion import GridEstimator

    return GridEstimator(search, penalty, intra_bias=intra_bias, scene_cut=scene_cut, **guide)


def _check_link_vectors(who, link_vectors, grids):
    """link_vectors hands out the block matcher's tables: the grids/ folders hold grids, from which no vector can be recovered."""
    if link_vectors and grids != "estimate":
        raise ValueError(f'{who}: link_vectors needs the estimated grids\' motion-vector tables (grids="estimate"); the grids/ folders hold grids, not vectors')
    return bool(link_vectors)


def _check_link_sources(who, link_sources, link_vectors):
    """link_sources hands out the decoded frames of the very windows whose vectors link_vectors hands out: the one is of no use without the other."""
    if link_sources and not link_vectors:
        raise ValueError(f"{who}: link_sources=True needs link_vectors=True (the frames go with the poses fitted to those vectors), got link_vectors={link_vectors}")
    return bool(link_sources)


def _check_hold_cuts(who, hold_cuts, grids, scene_cut):
    """hold_cuts reacts to the cut flags the grid estimator's matcher writes: without them it could never do anything."""
    if hold_cuts and (grids != "estimate" or scene_cut is None):
        raise ValueError(f'{who}: hold_cuts needs the scene-cut decision of the estimated grids (grids="estimate" and scene_cut=)')
    return bool(hold_cuts)


class PredictWindows:
    """Window i of a video = key frames (i*delta, (i+1)*delta) + the delta-1 grids in between (flow/dataset.py:112-146).

    grids="estimate" (extension): the grids come from block matching of the decoded frames (flow/motion.py, `search`, `penalty`,
    `intra_bias`, `scene_cut`) instead of the grids/ and inv_grids/ folders -- the same grid ids, and a frame is complete when its
    image exists.

    hold_cuts=True (extension; needs grids="estimate" and scene_cut): an item also carries "weights" (float32 [frame_delta, 2]) and
    "source" (int32 [frame_delta]), device tensors from ops.window_weights on the cut flags of the window's frame_delta frame pairs:
    FlowPredictor hands the weights to the tails, which then hold one key frame across a cut instead of blending two scenes.  One
    more search per window (the closing pair); with no_warp every pair is searched -- and every in-between frame decoded -- for its
    flag alone.

    link_vectors=True (extension; needs grids="estimate"): an item also carries "link_mvs" (int32 [frame_delta, blocks, 7]: per emitted
    frame the matcher's table of that frame against the frame before it, all void for frame 0), "link_frame_size" (the decoded frame's
    height and width) and, with intra_bias / scene_cut set, "link_stats" (int32 [frame_delta, 4], the same pairs' stats rows): what
    FlowPredictor(compensate=True) links the regions with.  One more search per window (the pair that ends in the window's key frame),
    unless hold_cuts has searched it; with no_warp every pair is searched for its vectors alone.

    guide=True (extension; needs grids="estimate"; guide_outlier, guide_bias, guide_rounds, guide_tol, guide_min_inliers as
    flow.motion.GridEstimator takes them): the grids and link_mvs come from the tables guided by the fitted camera motion
    (ops.guide_vectors), and with link_vectors an item also carries "link_raw_mvs", the tables as searched, and
    "link_guide_counts" (int64 [frame_delta, 8], the same pairs' rows of ops.guide_vectors' counts): what FlowPredictor.guide_report() keeps.

    link_sources=True (extension; needs link_vectors=True): an item also carries "link_sources", a list of source(frame_id + p) for the
    window's frame_delta emitted frames (None where a frame does not exist): what FlowPredictor(ortho=...) samples the orthophoto from.
    The frames go through the decode cache; with no_warp the in-between frames are decoded for this alone."""

    hold_cuts = False
    link_vectors = False
    link_sources = False

    def __init__(self, data_root, predict_v_id, frame_delta=5, no_warp=False, size=None, device="cuda", grids="files", search=16,
                 penalty=0, intra_bias=None, scene_cut=None, hold_cuts=False, link_vectors=False, link_sources=False, guide=False, guide_outlier=None,
                 guide_bias=None, guide_rounds=4, guide_tol=1.0, guide_min_inliers=12):
        self.hold_cuts = _check_hold_cuts("PredictWindows", hold_cuts, grids, scene_cut)
        self.link_vectors = _check_link_vectors("PredictWindows", link_vectors, grids)
        self.link_sources = _check_link_sources("PredictWindows", link_sources, self.link_vectors)
        self.estimator = _grid_source(grids, search, penalty, intra_bias, scene_cut, guide=guide, guide_outlier=guide_outlier, guide_bias=guide_bias,
                                      guide_rounds=guide_rounds, guide_tol=guide_tol, guide_min_inliers=guide_min_inliers)
        self.data_root, self.video_id = data_root, predict_v_id
        self.frame_delta, self.no_warp = frame_delta, no_warp
        self.size = size  # (h, w) of transform_predict's Resize, None = native
        self.device = device
        # flow/dataset.py:64 -- windows = frames // delta
        self.length = len(os.listdir(os.path.join(data_root, "frames", predict_v_id, "images"))) // frame_delta

    def __len__(self):
        return self.length

    # -- paths (flow/dataset.py:222-236)
    def frame_path(self, f_id):
        return os.path.join(self.data_root, "frames", self.video_id, "images", f"{f_id}.jpg")

    def grid_path(self, i, name):
        return os.path.join(self.data_root, "frames", self.video_id, name, f"{i}.npy")

    def _complete(self, f_id):
        if self.estimator is not None:
            return os.path.exists(self.frame_path(f_id))
        return all(os.path.exists(p) for p in (self.frame_path(f_id), self.grid_path(f_id, "grids"), self.grid_path(f_id, "inv_grids")))

    def indices(self, index, max_search=100000):
        """(f_index, prev_real, next_real): the key frames actually used.  A key frame whose image or grids are missing is
        replaced by the next complete one going FORWARD (previous key) / BACKWARD (next key) -- flow/dataset.py:119-131."""
        f_index = index * self.frame_delta
        prev_real, next_real = f_index, f_index + self.frame_delta
        steps = 0
        while not self._complete(prev_real):
            prev_real += 1
            steps += 1
            if steps > max_search:
                raise FileNotFoundError(f"no complete frame at or after {f_index}")
        steps = 0
        while not self._complete(next_real):
            next_real -= 1
            steps += 1
            if steps > max_search or next_real < 0:
                raise FileNotFoundError(f"no complete frame at or before {f_index + self.frame_delta}")
        return f_index, prev_real, next_real

    def grid_ids(self, index):
        """Forward grids for frames f+1..f+delta-1, inverse grids for the same frames REVERSED (flow/dataset.py:138-146)."""
        f_index = index * self.frame_delta
        ids = [f_index + i + 1 for i in range(self.frame_delta - 1)]
        return ids, ids[::-1]

    def _decode(self, f_id):
        """Decode frame `f_id` on the host and upload it: uint8 [H,W,3] on the device."""
        from PIL import Image

        return torch.from_numpy(np.array(Image.open(self.frame_path(f_id)).convert("RGB"))).to(self.device)

    def _decoded(self, f_id):
        """The decoded frame on the device, decoded and uploaded ONCE: the last frame_delta + 2 frames (a window touches
        frame_delta + 1) are kept by (video, frame id), so the key frame the grid estimator asks for (raw_frame) and the one the
        network gets (_frame), in this window and as the next window's previous key, are one decode and one copy."""
        cache = self.__dict__.setdefault("_decoded_frames", OrderedDict())
        key = (self.video_id, f_id)
        if key in cache:
            cache.move_to_end(key)
            return cache[key]
        frame = cache[key] = self._decode(f_id)
        while len(cache) > self.frame_delta + 2:
            cache.popitem(last=False)
        return frame

    def raw_frame(self, f_id):
        """The decoded uint8 frame [H,W,3] on the device, before Resize and normalisation (what the grid estimator sees, as
        mvextractor sees the decoded picture); None when the image does not exist."""
        if f_id < 0 or not os.path.exists(self.frame_path(f_id)):
            return None
        return self._decoded(f_id)

    def source(self, f_id):
        """(frame, chroma, fmt, matrix, full_range) of decoded frame `f_id` as ops.prepare_frame and ops.compose_frame take a frame: the
        very pixels the network's input was made from (an overlay's background); None when the image does not exist.  Goes through
        the decode cache, so a key frame is still decoded and uploaded once.  With no_warp the frames BETWEEN the key frames are not
        decoded by the prediction itself: an overlay decodes and uploads every one of them (frame_delta - 1 more per window)."""
        frame = self.raw_frame(f_id)
        return None if frame is None else (frame, None, "rgb24", "bt601", False)

    def _grid(self, g, name):
        """Grid `g` of grids/ (name "grids") or inv_grids/ as the float32 [1,67,120,2] device tensor of an item."""
        if self.estimator is None:
            return load_grid(self.grid_path(g, name))[None].to(self.device)
        pair = self._video_estimator().grids_for(g, self.raw_frame)
        return pair[0 if name == "grids" else 1].float()[None]

    def _video_estimator(self):
        if getattr(self, "_estimator_video", None) != self.video_id:  # EvalWindows walks several videos: frame ids are per video
            self.estimator.reset()
            self._estimator_video = self.video_id
        return self.estimator

    def _cut_weights(self, index):
        """(weights, source) of window `index` from the cut flags of its frame pairs; asked for AFTER the item's grids, so that only
        the closing pair (and, with no_warp, every pair) is still to be searched."""
        stats = self._video_estimator().window_stats(index * self.frame_delta, self.frame_delta, self.raw_frame)
        return ops.window_weights(stats, self.frame_delta)

    def _frame(self, f_id):
        """ToTensor, Resize (cv2.INTER_LINEAR on the uint8 image = half-pixel bilinear, stored back as uint8) and Normalize
        (flow/transform.py:26-106) of the decoded frame: one launch (ops.prepare_frame)."""
        return ops.prepare_frame(self._decoded(f_id), self.size, MEAN, STD)

    def __getitem__(self, index):
        if not 0 <= index < self.length:
            raise IndexError(index)
        f_index, prev_real, next_real = self.indices(index)
        # key_ids: the frames actually used as keys.  Window i's next key is window i+1's previous key (same index, same
        # deterministic transform: :113-114), which is what FlowPredictor's key-frame cache is keyed on.
        item = {"frame_prev": self._frame(prev_real), "frame_next": self._frame(next_real), "frame_id": f_index,
                "key_ids": (prev_real, next_real)}
        if self.no_warp:
            # placeholders whose COUNT still encodes n (flow/dataset.py:198-205, flow/base.py:266)
            item["mvs_left"] = [torch.zeros(1, 1, device=self.device) for _ in range(self.frame_delta - 1)]
            item["mvs_right"] = [torch.zeros(1, 1, device=self.device) for _ in range(self.frame_delta - 1)]
        else:
            fwd, inv = self.grid_ids(index)
            item["mvs_left"] = [self._grid(i, "grids") for i in fwd]
            item["mvs_right"] = [self._grid(i, "inv_grids") for i in inv]
        if self.hold_cuts:
            item["weights"], item["source"] = self._cut_weights(index)
        if self.link_vectors:
            self._link_keys(item, f_index)
        return item

    def _link_keys(self, item, f_index):
        """link_mvs, link_frame_size and link_stats of the window that emits frames f_index .. f_index + frame_delta - 1; asked for after
        the item's grids (and weights), so that only the pairs nobody has searched yet are searched."""
        est = self._video_estimator()
        item["link_mvs"] = est.window_tables(f_index, self.frame_delta, self.raw_frame)
        if est.guide:  # link_mvs are the GUIDED tables; the tables as searched go with them, for consumers that fit the camera themselves
            item["link_raw_mvs"] = est.window_raw_tables(f_index, self.frame_delta, self.raw_frame)
            counts = est.window_guide_counts(f_index, self.frame_delta)
            if counts is not None:
                item["link_guide_counts"] = counts
        frame = self.raw_frame(f_index)
        item["link_frame_size"] = (int(frame.shape[0]), int(frame.shape[1]))
        stats = est.window_link_stats(f_index, self.frame_delta)
        if stats is not None:
            item["link_stats"] = stats
        if self.link_sources:
            item["link_sources"] = [self.source(f_index + p) for p in range(self.frame_delta)]


def read_label_list(data_list, frame_delta):
    """make_dataset (flow/dataset.py:16-43): [(label path relative to data_root, video id, frame id)], dropping labelled
    frames closer than frame_delta // 2 to the start of the video.  The list files the reference ships and writes
    (dataset/flow/make_flow.py:107,137) hold THREE fields per line although make_dataset's check asks for four (it would
    reject its own lists); three or four fields are accepted here, anything else raises like the reference."""
    out = []
    with open(data_list) as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            f = line.split(" ")
            if len(f) not in (3, 4):
                raise RuntimeError("Image list file read line error : " + line + "\n")
            if int(f[2]) < frame_delta // 2:
                continue
            out.append((f[0], f[1], int(f[2])))
    return out


def resize_label_nearest(label, size):
    """Resize's label branch, cv2.INTER_NEAREST (flow/transform.py:104-105): src = min(floor(dst * src/dst), src - 1)."""
    h, w = size
    H, W = label.shape
    if (H, W) == (h, w):
        return label
    ys = np.minimum(np.floor(np.arange(h) * (H / h)).astype(np.int64), H - 1)
    xs = np.minimum(np.floor(np.arange(w) * (W / w)).astype(np.int64), W - 1)
    return label[ys][:, xs]


class EvalWindows(PredictWindows):
    """Item i of the `val` / `test` split = labelled frame f with key frames f-l and f+r, l drawn from Random(i) and
    l + r = frame_delta (flow/dataset.py:89-92, 115-117); items carry the batch dimension the DataLoader would add
    (batch_size_test = 1, flow/base.py:164)."""

    def __init__(self, data_root, data_list, split="test", frame_delta=5, no_warp=False, size=None, center_crop=None,
                 classes_ignore=(), device="cuda", grids="files", search=16, penalty=0, intra_bias=None, scene_cut=None, link_sources=False, guide=False, guide_outlier=None,
                 guide_bias=None, guide_rounds=4, guide_tol=1.0, guide_min_inliers=12):
        if split not in ("val", "test"):
            raise ValueError("EvalWindows mirrors the val / test splits; use PredictWindows for predict")
        if link_sources:  # taken so that the three datasets share a signature; an item here is one labelled frame and carries no link keys
            raise ValueError(f"EvalWindows does not support link_sources (its items carry no link_mvs to go with the frames), got link_sources={link_sources}; "
                             "use PredictWindows or RawVideoWindows with link_vectors=True")
        self.estimator = _grid_source(grids, search, penalty, intra_bias, scene_cut, guide=guide, guide_outlier=guide_outlier, guide_bias=guide_bias,
                                      guide_rounds=guide_rounds, guide_tol=guide_tol, guide_min_inliers=guide_min_inliers)
        self.data_root, self.split = data_root, split
        self.frame_delta, self.no_warp = frame_delta, no_warp
        self.size, self.center_crop = size, center_crop      # Resize target (h, w); Crop('center') size of transform_val
        self.classes_ignore = tuple(classes_ignore or ())    # data_classes_ignore (dataset/flow/config.yaml:6)
        self.device = device
        self.label_list = read_label_list(data_list, frame_delta)
        self.length = len(self.label_list)
        self.video_id = None
        self.default_grid = torch.from_numpy(get_default_grid()).float()   # flow/dataset.py:68 + ToTensor

    def plan(self, index):
        """Pure index arithmetic of item `index`: dict(l, r, prev_real, next_real, left_ids, right_ids); a None grid id
        stands for the identity default grid (flow/dataset.py:147-171)."""
        _, v_id, f_index = self.label_list[index]
        self.video_id = v_id
        delta = self.frame_delta
        l = random.Random(index).randrange(1, delta)
        r = delta - l
        prev_real, next_real = f_index - l, f_index + r
        steps = 0
        while not self._complete(prev_real):
            prev_real, steps = prev_real + 1, steps + 1
            if steps > 100000:
                raise FileNotFoundError(f"no complete frame at or after {f_index - l}")
        while not self._complete(next_real):
            next_real -= 1
            if next_real < 0:
                raise FileNotFoundError(f"no complete frame at or before {f_index + r}")
        left = [(g if g > prev_real else None) for g in range(f_index - l + 1, f_index + 1)]
        left += [None] * (delta - 1 - len(left))
        right = [(g if g <= next_real else None) for g in range(f_index + 1, f_index + r + 1)]
        right.reverse()
        right += [None] * (delta - 1 - len(right))
        return {"video": v_id, "frame": f_index, "l": l, "r": r, "prev_real": prev_real, "next_real": next_real,
                "left_ids": left, "right_ids": right}

    def _label(self, rel_path):
        from PIL import Image

        lab = np.array(Image.open(os.path.join(self.data_root, rel_path)))
        if lab.ndim != 2:
            raise RuntimeError(f"label {rel_path} is not single-channel")
        if self.size is not None:
            lab = resize_label_nearest(lab, self.size)
        lab = lab.copy()
        for c in self.classes_ignore:                         # IgnoreClasses (flow/transform.py:361-371)
            lab[lab == c] = 0
        return torch.from_numpy(lab).long()

    def __getitem__(self, index):
        if not 0 <= index < self.length:
            raise IndexError(index)
        p = self.plan(index)
        frame_prev, frame_next = self._frame(p["prev_real"]), self._frame(p["next_real"])
        label = self._label(self.label_list[index][0])[None].to(self.device)
        n1 = self.frame_delta - 1
        if self.no_warp:
            left = [torch.zeros(1, 1, device=self.device) for _ in range(n1)]
            right = [torch.zeros(1, 1, device=self.device) for _ in range(n1)]
        else:
            def grid(g, name):
                return self.default_grid[None].to(self.device) if g is None else self._grid(g, name)
            left = [grid(g, "grids") for g in p["left_ids"]]
            right = [grid(g, "inv_grids") for g in p["right_ids"]]
        if self.center_crop is not None:                      # Crop(..., 'center') of transform_val (flow/transform.py:183-211)
            from .crops import crop_motion_vector

            ch, cw = self.center_crop
            h, w = label.shape[-2:]
            assert h > ch and w > cw
            ho, wo = int((h - ch) / 2), int((w - cw) / 2)
            frame_prev = frame_prev[:, :, ho:ho + ch, wo:wo + cw].contiguous()
            frame_next = frame_next[:, :, ho:ho + ch, wo:wo + cw].contiguous()
            label = label[:, ho:ho + ch, wo:wo + cw].contiguous()
            if not self.no_warp:
                left, right = crop_motion_vector(left, right, h, w, ch, cw, ho, wo)
        return {"frame_prev": frame_prev, "frame_next": frame_next, "mvs_left": left, "mvs_right": right, "label": label,
                "left_index": torch.tensor([p["l"]]), "right_index": torch.tensor([p["r"]])}


RAW_PIX_FMTS = ("nv12", "i420", "rgb24")
RAW_OUT_PIX_FMTS = RAW_PIX_FMTS + ("gray",)  # the writer also takes one 8-bit plane per frame (ffmpeg -pix_fmt gray): confidence planes


raw_frame_bytes = ops.raw_frame_bytes  # bytes of one frame of a headerless raw video; chroma planes of the 4:2:0 formats round up


class RawVideoWindows(PredictWindows):
    """The windows of PredictWindows (frame_prev, frame_next, mvs_left, mvs_right, frame_id, key_ids) over ONE headerless raw video
    file, as `ffmpeg -f rawvideo -pix_fmt nv12|yuv420p|rgb24` writes it (extension: the reference reads JPEG folders only).

    pix_fmt "nv12" (Y plane + interleaved UV), "i420" (= yuv420p: Y, U, V planes) or "rgb24"; frames are read through numpy.memmap and
    uploaded once each; the network's input comes from ops.prepare_frame (`matrix`, `full_range`: the integer YUV -> RGB conversion of
    include/floodseg_test.h).  len = frames // frame_delta; a file that is not a whole number of frames raises.  A raw file has no grid
    folders: the grids are estimated (grids="estimate", flow/motion.py) unless no_warp; "files" raises.  hold_cuts, link_vectors: as
    PredictWindows'.

    For the YUV formats the block matcher gets the stream's Y plane AS IT IS (its one-channel route).  These grids DIFFER from grids
    estimated on the RGB conversion of the same video: there the matcher reduces RGB to its own luma (77 R + 150 G + 29 B + 128) >> 8,
    which is not the stream's Y (range, matrix and the clipping of the conversion all enter)."""

    def __init__(self, path, height, width, pix_fmt, frame_delta=5, no_warp=False, size=None, grids="estimate", search=16, penalty=0,
                 matrix="bt709", full_range=False, device="cuda", intra_bias=None, scene_cut=None, hold_cuts=False, link_vectors=False,
                 link_sources=False, guide=False, guide_outlier=None,
                 guide_bias=None, guide_rounds=4, guide_tol=1.0, guide_min_inliers=12):
        self.hold_cuts = _check_hold_cuts("RawVideoWindows", hold_cuts, grids, scene_cut)
        self.link_vectors = bool(link_vectors)
        self.link_sources = _check_link_sources("RawVideoWindows", link_sources, self.link_vectors)
        if pix_fmt not in RAW_PIX_FMTS:
            raise ValueError(f"RawVideoWindows: pix_fmt must be one of {RAW_PIX_FMTS}, got {pix_fmt!r}")
        if grids == "files":
            raise ValueError('RawVideoWindows: a raw video file has no grids/ folders; use grids="estimate" (or no_warp=True)')
        if matrix not in ("bt601", "bt709"):
            raise ValueError(f'RawVideoWindows: matrix must be "bt601" or "bt709", got {matrix!r}')
        if height < 1 or width < 1 or frame_delta < 1:
            raise ValueError(f"RawVideoWindows: bad geometry {height} x {width}, frame_delta {frame_delta}")
        self.estimator = _grid_source(grids, search, penalty, intra_bias, scene_cut, guide=guide, guide_outlier=guide_outlier, guide_bias=guide_bias,
                                      guide_rounds=guide_rounds, guide_tol=guide_tol, guide_min_inliers=guide_min_inliers)
        if not no_warp:
            from .motion import check_geometry

            check_geometry(height, width)
        self.path, self.video_id = path, path
        self.height, self.width, self.pix_fmt = int(height), int(width), pix_fmt
        self.matrix, self.full_range = matrix, bool(full_range)
        self.frame_delta, self.no_warp, self.size, self.device = frame_delta, no_warp, size, device
        self.frame_bytes = raw_frame_bytes(self.height, self.width, pix_fmt)
        total = os.path.getsize(path)
        if total == 0 or total % self.frame_bytes:
            raise ValueError(f"RawVideoWindows: {path} holds {total} bytes, not a whole number of {self.height} x {self.width} {pix_fmt} "
                             f"frames of {self.frame_bytes} bytes")
        self.frames = total // self.frame_bytes
        self.length = self.frames // frame_delta
        self._file = np.memmap(path, dtype=np.uint8, mode="r", shape=(self.frames, self.frame_bytes))

    def frame_path(self, f_id):
        return f"{self.path}[{f_id}]"

    def _complete(self, f_id):
        return 0 <= f_id < self.frames

    def _decode(self, f_id):
        """Frame f_id's bytes on the device (one copy): uint8 [frame_bytes]."""
        return torch.from_numpy(np.array(self._file[f_id])).to(self.device)

    def planes(self, f_id):
        """(frame, chroma) of frame f_id as ops.prepare_frame takes them: views of the one uploaded buffer."""
        return ops.frame_planes(self._decoded(f_id), self.height, self.width, self.pix_fmt)

    def source(self, f_id):
        """(frame, chroma, fmt, matrix, full_range) of frame f_id for ops.compose_frame's background (see PredictWindows.source: the
        same cache, the same extra uploads under no_warp); None past either end of the file."""
        if not self._complete(f_id):
            return None
        frame, chroma = self.planes(f_id)
        return frame, chroma, self.pix_fmt, self.matrix, self.full_range

    def raw_frame(self, f_id):
        """What the grid estimator sees: the RGB frame [H,W,3], or the Y plane [H,W] of a YUV stream; None past either end."""
        return self.planes(f_id)[0] if self._complete(f_id) else None

    def _frame(self, f_id):
        frame, chroma = self.planes(f_id)
        return ops.prepare_frame(frame, self.size, MEAN, STD, fmt=self.pix_fmt, chroma=chroma, matrix=self.matrix, full_range=self.full_range)


class RawVideoWriter:
    """Writes headerless raw video frames (what `ffmpeg -f rawvideo -pix_fmt nv12|yuv420p|rgb24|gray -s WxH` reads): the output side of
    RawVideoWindows ("gray": one 8-bit plane per frame, the confidence planes of FlowPredictor(confidence=True)).  write(frame_id, buffer) takes one frame of raw_frame_bytes(height, width, pix_fmt) bytes -- a uint8 device
    tensor (ops.compose_frame's `out` buffer) or a host numpy array / tensor.

    A REGULAR FILE is written by position: frame i goes to byte i * frame_bytes (os.pwrite), in any order, and `frames` pre-sizes the
    file.  The ranks of a torchrun launch can therefore write their disjoint window blocks into ONE file (give every rank the same
    `frames`; the file is then not truncated on open, only sized).  Without `frames` the file is truncated on open: one writer.
    A PIPE, a FIFO, any other file object, or "-" (standard output) takes frames strictly in order 0, 1, 2, ...; anything else raises,
    and such a target is refused when world > 1.

    Device frames go through two pinned host buffers, a non-blocking copy and an event each: write(i) enqueues frame i's copy, then
    waits for frame i - 1's and hands it to the file, and returns while copy i is still in flight -- it overlaps the launches of frame
    i + 1.  close() (or leaving the `with` block) drains both."""

    def __init__(self, path_or_fileobj, height, width, pix_fmt, frames=None, world=1):
        import stat
        import sys

        if pix_fmt not in RAW_OUT_PIX_FMTS:
            raise ValueError(f"RawVideoWriter: pix_fmt must be one of {RAW_OUT_PIX_FMTS}, got {pix_fmt!r}")
        if height < 1 or width < 1 or (frames is not None and frames < 0):
            raise ValueError(f"RawVideoWriter: bad geometry {height} x {width}, frames {frames}")
        self.height, self.width, self.pix_fmt = int(height), int(width), pix_fmt
        self.frame_bytes = raw_frame_bytes(self.height, self.width, pix_fmt)
        self._own_fd = self._fd = self._stream = None
        self.frames = frames
        self._next = 0         # sequential targets: the frame id due next
        self._slots = None     # device frames: [pinned buffer, event, pending frame id or None] x 2
        self._turn = 0
        self.written = 0
        if isinstance(path_or_fileobj, str) and path_or_fileobj == "-":
            self._stream = sys.stdout.buffer
        elif isinstance(path_or_fileobj, (str, os.PathLike)):
            self._own_fd = os.open(path_or_fileobj, os.O_WRONLY | os.O_CREAT | (os.O_TRUNC if frames is None else 0), 0o644)
            if stat.S_ISREG(os.fstat(self._own_fd).st_mode):
                self._fd = self._own_fd
            else:
                self._stream = os.fdopen(self._own_fd, "wb", closefd=False)
        else:
            try:   # io.BytesIO has a fileno() that raises
                fd = path_or_fileobj.fileno()
                fd = fd if stat.S_ISREG(os.fstat(fd).st_mode) else None
            except (AttributeError, OSError, ValueError):
                fd = None
            if fd is not None:
                path_or_fileobj.flush()
                self._fd = fd
            else:
                self._stream = path_or_fileobj
        if self._stream is not None and world > 1:
            self.close()
            raise ValueError("RawVideoWriter: a pipe takes frames strictly in order and cannot be shared by the ranks of a multi-GPU run; "
                             "write to a regular file (every rank the same `frames`)")
        if self._fd is not None and frames is not None:
            os.ftruncate(self._fd, frames * self.frame_bytes)

    def _put(self, frame_id, data):
        if self._fd is not None:
            done = 0
            while done < len(data):
                done += os.pwrite(self._fd, data[done:], frame_id * self.frame_bytes + done)
        else:
            self._stream.write(data)
        self.written += 1

    def _drain(self, slot):
        if slot[2] is not None:
            slot[1].synchronize()
            self._put(slot[2], memoryview(slot[0].numpy()))
            slot[2] = None

    def write(self, frame_id, frame):
        frame_id = int(frame_id)
        nbytes = frame.numel() * frame.element_size() if isinstance(frame, torch.Tensor) else np.asarray(frame).nbytes
        dtype_ok = frame.dtype == torch.uint8 if isinstance(frame, torch.Tensor) else np.asarray(frame).dtype == np.uint8
        if nbytes != self.frame_bytes or not dtype_ok:
            raise ValueError(f"RawVideoWriter: a {self.height} x {self.width} {self.pix_fmt} frame is {self.frame_bytes} uint8 bytes, got {nbytes} "
                             f"bytes of {frame.dtype}")
        if frame_id < 0 or (self.frames is not None and frame_id >= self.frames):
            raise ValueError(f"RawVideoWriter: frame id {frame_id} outside 0..{'' if self.frames is None else self.frames - 1}")
        if self._stream is not None:
            if frame_id != self._next:
                raise ValueError(f"RawVideoWriter: a pipe takes frames strictly in order: frame {self._next} is due, got {frame_id}")
            self._next += 1
        if isinstance(frame, torch.Tensor) and frame.is_cuda:
            if self._slots is None:
                self._slots = [[torch.empty(self.frame_bytes, dtype=torch.uint8).pin_memory(), torch.cuda.Event(), None] for _ in range(2)]
            slot, other = self._slots[self._turn], self._slots[self._turn ^ 1]
            self._turn ^= 1
            self._drain(slot)                                     # two writes ago: long finished
            slot[0].copy_(frame.reshape(-1), non_blocking=True)
            slot[1].record(torch.cuda.current_stream(frame.device))
            slot[2] = frame_id
            self._drain(other)                                    # the previous frame, while this one's copy is in flight
            return
        self.flush()                                              # keeps a sequential target in order
        host = frame.contiguous().numpy() if isinstance(frame, torch.Tensor) else np.ascontiguousarray(frame)
        self._put(frame_id, memoryview(host.reshape(-1)))

    def flush(self):
        """Wait for the device frames still in flight and hand them to the file, oldest first."""
        if self._slots is not None:
            self._drain(self._slots[self._turn])
            self._drain(self._slots[self._turn ^ 1])
        if self._stream is not None:
            self._stream.flush()

    def close(self):
        self.flush()
        if self._own_fd is not None:
            os.close(self._own_fd)
            self._own_fd = self._fd = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
