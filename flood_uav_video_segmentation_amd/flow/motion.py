"""Grid source for frame folders: block motion vectors estimated from the decoded frames on the GPU, in place of the
encoder's vectors the reference reads with mvextractor (dataset/flow/extract_motion_vectors.py:47-108).

  frames i-1, i (uint8, as decoded)  --ops.block_match-->  table [8040, 7]  --fs_mv_to_grids-->  grids/<i>, inv_grids/<i>

The table -> grid step is the code that serves mvextractor tables (flow/grids.py); only the table's origin differs.  An encoder
chooses its vectors by rate-distortion, at sub-pel precision, and sends none for an I-frame; this is an integer full search
on luma.  Grids estimated here are therefore not the grids mvextractor would give for the same video.
"""
from collections import OrderedDict

import torch

from .. import ops
from .grids import BLOCK, HEIGHT, WIDTH, motion_vectors_to_grids
from .model import get_default_grid


def estimate_motion_vectors(cur, ref, search=16, penalty=0, return_cost=False):
    """Motion-vector table of frame `cur` against the past frame `ref` (uint8 CUDA tensors [H,W] or [H,W,3]): int32 [H//16 * W//16, 7]
    rows (-1, 16, 16, src_x, src_y, dst_x, dst_y) in block raster order."""
    return ops.block_match(cur, ref, search=search, penalty=penalty, return_cost=return_cost)


def check_geometry(h, w):
    if h // BLOCK != HEIGHT // BLOCK or w // BLOCK != WIDTH // BLOCK:
        raise RuntimeError(f"estimate_grids: the grid producer is built for {HEIGHT // BLOCK} x {WIDTH // BLOCK} blocks of {BLOCK} "
                           f"(1072 x 1920 or 1080 x 1920 frames), got a {h} x {w} frame")


def estimate_grids(cur, ref, search=16, penalty=0):
    """(grid, inv_grid) of frame `cur` against the past frame `ref`: float64 CUDA [67,120,2], normalised with the frame's own height
    and width (extract_motion_vectors.py:94-98).  Enqueues only: nothing is read back to the host."""
    check_geometry(int(cur.shape[0]), int(cur.shape[1]))
    table = ops.block_match(cur, ref, search=search, penalty=penalty)
    with torch.cuda.device(table.device):
        return motion_vectors_to_grids(table, int(cur.shape[0]), int(cur.shape[1]), validate=False)


class GridEstimator:
    """Grids of frame i against frame i-1 on demand, for the window datasets and tools/estimate_grids.py.

    grids_for(frame_id, load_frame) -> (grid, inv_grid) float64 CUDA [67,120,2]; load_frame(i) returns the decoded uint8 frame
    [H,W,3] (or [H,W]) on the GPU, or None when frame i does not exist.  Frame 0, and a frame whose predecessor is missing, get the
    default grid twice: an I-frame carries no vectors in the reference's pipeline either.  The last `cache` results and the last
    two decoded frames are kept (neighbouring windows ask for neighbouring frames)."""

    def __init__(self, search=16, penalty=0, cache=64):
        if not 1 <= int(search) <= 32 or not 0 <= int(penalty) <= 255:
            raise ValueError(f"GridEstimator: search must be 1..32 and penalty 0..255, got {search}, {penalty}")
        self.search, self.penalty = int(search), int(penalty)
        self._cache_size = int(cache)
        self._grids = OrderedDict()
        self._frames = OrderedDict()

    def reset(self):
        """Forget every cached frame and grid (the caller moves to another video)."""
        self._grids.clear()
        self._frames.clear()

    def _frame(self, frame_id, load_frame):
        if frame_id in self._frames:
            return self._frames[frame_id]
        frame = load_frame(frame_id)
        if frame is not None:
            self._frames[frame_id] = frame
            while len(self._frames) > 2:
                self._frames.popitem(last=False)
        return frame

    def grids_for(self, frame_id, load_frame):
        if frame_id in self._grids:
            self._grids.move_to_end(frame_id)
            return self._grids[frame_id]
        cur = self._frame(frame_id, load_frame)
        if cur is None:
            raise FileNotFoundError(f"GridEstimator: frame {frame_id} does not exist")
        ref = self._frame(frame_id - 1, load_frame) if frame_id > 0 else None
        if ref is None:
            check_geometry(int(cur.shape[0]), int(cur.shape[1]))
            default = torch.from_numpy(get_default_grid()).to(cur.device)
            out = (default, default.clone())
        else:
            out = estimate_grids(cur, ref, self.search, self.penalty)
        self._grids[frame_id] = out
        while len(self._grids) > self._cache_size:
            self._grids.popitem(last=False)
        return out
