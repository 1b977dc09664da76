"""Grid source for frame folders: block motion vectors estimated from the decoded frames on the GPU, in place of the
encoder's vectors the reference reads with mvextractor (dataset/flow/extract_motion_vectors.py:47-108).

  frames i-1, i (uint8, as decoded)  --ops.block_match-->  table [8040, 7]  --fs_mv_to_grids-->  grids/<i>, inv_grids/<i>

The table -> grid step is the code that serves mvextractor tables (flow/grids.py); only the table's origin differs.  An encoder
chooses its vectors by rate-distortion, at sub-pel precision, and sends none for an I-frame; this is an integer full search
on luma.  Grids estimated here are therefore not the grids mvextractor would give for the same video.

A table row may be a VOID ROW, (-1, 16, 16, -16, -16, -16, -16): no vector for that block.  Its block indices floor-divide to -1, the
grid producer skips it in both directions, and the block's cells keep the identity grid -- what the reference's script leaves for an
intra macroblock and for a whole I-frame.  ops.block_match never writes one.  With intra_bias= and / or scene_cut= the table comes from
ops.block_match_modes instead, which writes one for every block the matcher cannot explain (SAD of the winner > the block's deviation
from its own mean + intra_bias) and, when more than the fraction scene_cut of the blocks are such, for every block: a scene cut
degrades to "no motion".  Both are off by default; no default has been validated on real video (on flat, noisy water the winner's
SAD is about 1.4 x the activity, so intra_bias = 0 marks such blocks).

What a cut does to the BLEND of the two key frames is the window datasets' hold_cuts= (flow/dataset.py): GridEstimator.window_stats
hands the cut flags of a window's frame pairs -- the closing pair (last in-between frame -> next key frame) included, which feeds no
grid and is searched for this alone -- to ops.window_weights, and the tails hold one key frame's chain on each side of the cut
(include/floodseg_test.h, window_weights).  Without hold_cuts a cut between two key frames still blends the two scenes linearly.

The TABLES themselves have a second consumer: the motion-compensated region links (ops.region_links with mv=) read the
integer vectors, which the grids cannot replace -- a grid cell keeps only the source BLOCK of a vector, so any vector of -8..+7 pixels
is the identity there.  GridEstimator.table_for / window_tables hand them out (the window datasets' link_vectors=True); the block
search of a frame pair is shared with grids_for, whichever is asked first.

GUIDED TABLES (guide=True).  The tables are weakest on flat, noisy water: with intra_bias = 0 such blocks are void rows
that keep the identity grid while the ground around them moves with the camera, and without it they carry the least bad of 1089 wrong
vectors.  After the pair's single search ops.global_motion fits the camera model to the table (in frame pixels) and ops.guide_vectors
fills the void rows with the camera's vector and, with guide_outlier=, replaces vectors that disagree with it -- with guide_bias=
only where the camera's window explains the block no worse than the winner did, up to that bias.  The GUIDED table takes the table's
place everywhere (the cache, grids_for, table_for, window_tables); the RAW one is kept beside it (raw_table_for, window_raw_tables) for
consumers that fit the camera themselves and must not feed on rows the fit produced.  A cut pair and a failed fit pass through
untouched.  Off by default; the defaults are guesses, not validated on real video.
"""
import warnings
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


def _warn_cut_without_bias(intra_bias, scene_cut):
    """scene_cut counts INTRA blocks, and with intra_bias left None (= 65535) no block is ever intra: the cut rule can never fire."""
    if scene_cut is not None and intra_bias is None:
        warnings.warn("scene_cut without intra_bias never detects a cut: the cut rule counts intra blocks, and intra_bias=None marks none "
                      "(give intra_bias as well, e.g. 0)", stacklevel=3)


VOID_ROW = (-1, 16, 16, -16, -16, -16, -16)


def _search(cur, ref, search, penalty, intra_bias, scene_cut, return_cost=False):
    """(table, stats) of the block search of `cur` against the past frame `ref`; stats None with both decisions off.  return_cost:
    (table, stats, cost), cost the winning costs int32 [blocks]."""
    if intra_bias is None and scene_cut is None:
        if return_cost:
            table, cost = ops.block_match(cur, ref, search=search, penalty=penalty, return_cost=True)
            return table, None, cost
        return ops.block_match(cur, ref, search=search, penalty=penalty), None
    if return_cost:
        table, cost, stats = ops.block_match_modes(cur, ref, search=search, penalty=penalty, intra_bias=65535 if intra_bias is None else intra_bias,
                                                   scene_cut=scene_cut, return_cost=True, return_stats=True)
        return table, stats, cost
    return ops.block_match_modes(cur, ref, search=search, penalty=penalty, intra_bias=65535 if intra_bias is None else intra_bias,
                                 scene_cut=scene_cut, return_stats=True)


def _check_guide(what, guide, guide_outlier, guide_bias, guide_rounds, guide_tol, guide_min_inliers):
    """The guide arguments GridEstimator and estimate_grids share -> them, normalised."""
    if guide_outlier is not None and not 0 <= float(guide_outlier) <= 64:
        raise ValueError(f"{what}: guide_outlier must be 0..64 frame pixels or None, got {guide_outlier}")
    if guide_bias is not None and not 0 <= int(guide_bias) <= 65535:
        raise ValueError(f"{what}: guide_bias must be 0..65535 or None, got {guide_bias}")
    if not 0 <= int(guide_rounds) <= 8 or not 0 <= float(guide_tol) <= 64 or not 3 <= int(guide_min_inliers) <= 1 << 20:
        raise ValueError(f"{what}: guide_rounds must be 0..8, guide_tol 0..64 and guide_min_inliers 3..2^20, got {guide_rounds}, {guide_tol}, "
                         f"{guide_min_inliers}")
    if not guide and (guide_outlier is not None or guide_bias is not None):
        raise ValueError(f"{what}: guide_outlier / guide_bias need guide=True, got guide={guide!r}")
    return (bool(guide), None if guide_outlier is None else float(guide_outlier), None if guide_bias is None else int(guide_bias), int(guide_rounds),
            float(guide_tol), int(guide_min_inliers))


def _guided_search(cur, ref, search, penalty, intra_bias, scene_cut, guide_outlier, guide_bias, guide_rounds, guide_tol, guide_min_inliers):
    """(guided table, stats, raw table, counts int64 [8]) of one pair: the search, the camera fit in frame pixels, the guided table."""
    size = (int(cur.shape[0]), int(cur.shape[1]))
    if guide_bias is None:
        (raw, stats), cost = _search(cur, ref, search, penalty, intra_bias, scene_cut), None
    else:
        raw, stats, cost = _search(cur, ref, search, penalty, intra_bias, scene_cut, return_cost=True)
    model = ops.global_motion(raw[None], size, size, rounds=guide_rounds, tol=guide_tol, min_inliers=guide_min_inliers,
                              pair_stats=None if stats is None else stats[None])
    evidence = {} if cost is None else dict(cur=cur[None], ref=ref[None], cost=cost[None], penalty=penalty, guide_bias=guide_bias)
    table, counts = ops.guide_vectors(raw[None], model, size, fill_void=True, outlier=guide_outlier, **evidence)
    return table[0], stats, raw, counts[0]


def estimate_grids(cur, ref, search=16, penalty=0, intra_bias=None, scene_cut=None, return_stats=False, guide=False, guide_outlier=None,
                   guide_bias=None, guide_rounds=4, guide_tol=1.0, guide_min_inliers=12):
    """(grid, inv_grid) of frame `cur` against the past frame `ref`: float64 CUDA [67,120,2], normalised with the frame's own height
    and width (extract_motion_vectors.py:94-98).  Enqueues only: nothing is read back to the host.
    intra_bias (0..65535) and / or scene_cut (fraction 0..1): the table comes from ops.block_match_modes (the one left None is off).
    The cut rule counts intra blocks, so scene_cut needs intra_bias to have any effect: alone it never fires, and warns.
    return_stats appends the call's device stats tensor int32 [4] (None when both are off): how GridEstimator gets at it.
    guide=True (with guide_outlier, guide_bias, guide_rounds, guide_tol, guide_min_inliers as GridEstimator takes them): the grids come
    from the table guided by the fitted camera motion (ops.guide_vectors)."""
    check_geometry(int(cur.shape[0]), int(cur.shape[1]))
    _warn_cut_without_bias(intra_bias, scene_cut)
    guide = _check_guide("estimate_grids", guide, guide_outlier, guide_bias, guide_rounds, guide_tol, guide_min_inliers)
    if guide[0]:
        table, stats = _guided_search(cur, ref, search, penalty, intra_bias, scene_cut, *guide[1:])[:2]
    else:
        table, stats = _search(cur, ref, search, penalty, intra_bias, scene_cut)
    with torch.cuda.device(table.device):
        grids = motion_vectors_to_grids(table, int(cur.shape[0]), int(cur.shape[1]), validate=False)
    return (*grids, stats) if return_stats else grids


class GridEstimator:
    """Grids of frame i against frame i-1 on demand, for the window datasets and tools/estimate_grids.py.

    grids_for(frame_id, load_frame) -> (grid, inv_grid) float64 CUDA [67,120,2]; load_frame(i) returns the decoded uint8 frame
    [H,W,3] (or [H,W]) on the GPU, or None when frame i does not exist.  Frame 0, and a frame whose predecessor is missing, get the
    default grid twice: an I-frame carries no vectors in the reference's pipeline either.  The last `cache` results and the last
    two decoded frames are kept (neighbouring windows ask for neighbouring frames).

    table_for(frame_id, load_frame) -> the int32 [blocks, 7] device table of frame_id against frame_id - 1 (an all-void table for frame
    0 and for a frame whose predecessor is missing); window_tables stacks a window's.  Cached like the grids, and ONE block search per
    frame pair serves both: grids_for takes the table table_for has searched, and the other way round.

    guide=True: every table is the search's table guided by the camera model fitted to it (module docstring); guide_outlier (frame
    pixels, None = fill void rows only), guide_bias (0..65535: ask the frames, None = replace outliers as they stand), guide_rounds /
    guide_tol / guide_min_inliers = ops.global_motion's rounds / tol / min_inliers.  raw_table_for / window_raw_tables hand out the
    tables as searched, guide_counts_for the pair's row of ops.guide_vectors' counts, guide_report all of them in one read-back."""

    STATS_CHUNK = 256

    def __init__(self, search=16, penalty=0, cache=64, intra_bias=None, scene_cut=None, guide=False, guide_outlier=None, guide_bias=None,
                 guide_rounds=4, guide_tol=1.0, guide_min_inliers=12):
        if not 1 <= int(search) <= 32 or not 0 <= int(penalty) <= 255:
            raise ValueError(f"GridEstimator: search must be 1..32 and penalty 0..255, got {search}, {penalty}")
        if intra_bias is not None and not 0 <= int(intra_bias) <= 65535:
            raise ValueError(f"GridEstimator: intra_bias must be 0..65535 or None, got {intra_bias}")
        if scene_cut is not None and not 0 <= float(scene_cut) <= 1:
            raise ValueError(f"GridEstimator: scene_cut must be a fraction in [0, 1] or None, got {scene_cut}")
        self.search, self.penalty = int(search), int(penalty)
        self.intra_bias = None if intra_bias is None else int(intra_bias)
        self.scene_cut = None if scene_cut is None else float(scene_cut)
        _warn_cut_without_bias(intra_bias, scene_cut)
        (self.guide, self.guide_outlier, self.guide_bias, self.guide_rounds, self.guide_tol,
         self.guide_min_inliers) = _check_guide("GridEstimator", guide, guide_outlier, guide_bias, guide_rounds, guide_tol, guide_min_inliers)
        self._cache_size = int(cache)
        self._grids = OrderedDict()
        self._tables = OrderedDict()  # frame id -> int32 [blocks, 7]: the searches, shared by grids_for and table_for
        self._frames = OrderedDict()
        self._stats = {}        # frame id -> one row of a chunk below
        self._stat_chunks = []  # int32 [STATS_CHUNK, 4] device buffers: one allocation per STATS_CHUNK estimated pairs, not one per pair
        self._raw = OrderedDict()  # guide=True: frame id -> the table as searched, cached beside the guided one in _tables
        self._guide_counts = {}    # frame id -> one row of a chunk below
        self._guide_chunks = []    # int64 [STATS_CHUNK, 8] device buffers, as the stats'

    def reset(self):
        """Forget every cached frame, grid and stats tensor (the caller moves to another video)."""
        self._grids.clear()
        self._tables.clear()
        self._frames.clear()
        self._stats.clear()
        self._stat_chunks.clear()
        self._raw.clear()
        self._guide_counts.clear()
        self._guide_chunks.clear()

    def stats_for(self, frame_id):
        """The device stats tensor int32 [4] = (blocks, intra blocks, cut, 0) of a pair this estimator has estimated with intra_bias /
        scene_cut; None for a frame that took the default grid (no predecessor), that was not estimated, or with both decisions off.
        Kept for every estimated frame until reset() -- 16 bytes each, rows of shared [256, 4] buffers, so a long video costs one 4 KB
        allocation per 256 pairs -- unlike the grids, which the cache evicts.  Reading it back is the caller's choice, and cost."""
        return self._stats.get(frame_id)

    def estimated_stats(self):
        """{frame_id: device stats tensor} of every pair estimated since the last reset()."""
        return dict(self._stats)

    def _keep_stats(self, frame_id, stats):
        """Copy a call's stats into frame_id's row of the shared buffers (16 bytes device to device, enqueued like the rest)."""
        if frame_id not in self._stats:  # (a frame estimated again after its grids were evicted keeps its row)
            row = len(self._stats) % self.STATS_CHUNK
            if row == 0:
                self._stat_chunks.append(torch.empty((self.STATS_CHUNK, 4), dtype=torch.int32, device=stats.device))
            self._stats[frame_id] = self._stat_chunks[-1][row]
        self._stats[frame_id].copy_(stats)

    def guide_counts_for(self, frame_id):
        """The device row int64 [8] = ops.GUIDE_COUNTS of a pair this estimator has guided; None for a frame that was not estimated, that
        took the void table, or with guide=False.  Kept until reset() in shared [256, 8] buffers, like the stats."""
        return self._guide_counts.get(frame_id)

    def guide_report(self):
        """(frame ids, int64 [m, 8] host array) of every pair guided since the last reset(), in frame order: ops.GUIDE_COUNTS per pair, read
        back ONCE here (one stack, one copy)."""
        ids = sorted(self._guide_counts)
        if not ids:
            return [], torch.zeros((0, 8), dtype=torch.int64).numpy()
        return ids, torch.stack([self._guide_counts[j] for j in ids]).cpu().numpy()

    def _keep_guide_counts(self, frame_id, counts):
        if frame_id not in self._guide_counts:
            row = len(self._guide_counts) % self.STATS_CHUNK
            if row == 0:
                self._guide_chunks.append(torch.empty((self.STATS_CHUNK, 8), dtype=torch.int64, device=counts.device))
            self._guide_counts[frame_id] = self._guide_chunks[-1][row]
        self._guide_counts[frame_id].copy_(counts)

    def window_stats(self, first_id, n, load_frame):
        """The n stats tensors (stats_for) of the pairs first_id+1 .. first_id+n of a window whose previous key frame is first_id, as
        ops.window_weights takes them.  A pair that has not been estimated yet -- the closing pair (first_id+n-1 -> first_id+n) feeds no
        grid of any window, and with no_warp no pair does -- gets the SEARCH alone here (no table -> grid step); a pair with a missing
        frame yields None, "no cut".  All None with both decisions off."""
        out = []
        for j in range(first_id + 1, first_id + n + 1):
            if j not in self._stats and (self.intra_bias is not None or self.scene_cut is not None):
                ref = self._frame(j - 1, load_frame) if j > 0 else None
                cur = self._frame(j, load_frame) if ref is not None else None
                if cur is not None:
                    self._table(j, cur, ref)
            out.append(self._stats.get(j))
        return out

    def _table(self, frame_id, cur, ref):
        """The table of the pair (frame_id - 1, frame_id), searched once: kept among the last `cache` tables, its stats kept for good."""
        if frame_id in self._tables:
            self._tables.move_to_end(frame_id)
            return self._tables[frame_id]
        if self.guide:
            table, stats, raw, counts = _guided_search(cur, ref, self.search, self.penalty, self.intra_bias, self.scene_cut, self.guide_outlier,
                                                       self.guide_bias, self.guide_rounds, self.guide_tol, self.guide_min_inliers)
            self._keep_guide_counts(frame_id, counts)
            self._raw[frame_id] = raw  # evicted with its guided table below: the two caches hold the same frames
        else:
            table, stats = _search(cur, ref, self.search, self.penalty, self.intra_bias, self.scene_cut)
        if stats is not None:
            self._keep_stats(frame_id, stats)
        self._tables[frame_id] = table
        while len(self._tables) > self._cache_size:
            self._raw.pop(self._tables.popitem(last=False)[0], None)
        return table

    def table_for(self, frame_id, load_frame):
        """The int32 [blocks, 7] device table of frame_id against frame_id - 1, as ops.region_links takes it (mv=).  Frame 0, or a frame
        whose predecessor is missing, gets an all-void table: no vectors, as for an I-frame."""
        if frame_id in self._tables:
            self._tables.move_to_end(frame_id)
            return self._tables[frame_id]
        cur = self._frame(frame_id, load_frame)
        if cur is None:
            raise FileNotFoundError(f"GridEstimator: frame {frame_id} does not exist")
        ref = self._frame(frame_id - 1, load_frame) if frame_id > 0 else None
        if ref is None:
            blocks = (int(cur.shape[0]) // BLOCK) * (int(cur.shape[1]) // BLOCK)
            return torch.tensor(VOID_ROW, dtype=torch.int32, device=cur.device).repeat(blocks, 1)
        return self._table(frame_id, cur, ref)

    def window_tables(self, first_id, n, load_frame):
        """int32 [n, blocks, 7]: the tables of the pairs ending in frames first_id .. first_id + n - 1, the frames a window whose previous
        key frame is first_id emits.  The first pair (the last frame of the window before -> this window's key frame) feeds no grid of
        any window: one more search per window, unless window_stats (hold_cuts) has searched it as the window before's closing pair."""
        return torch.stack([self.table_for(j, load_frame) for j in range(first_id, first_id + n)])

    def raw_table_for(self, frame_id, load_frame):
        """table_for's table as the search wrote it, before guidance (the same tensor as table_for's with guide=False).  The pair is
        searched once, whichever of the two is asked first."""
        table = self.table_for(frame_id, load_frame)
        return self._raw.get(frame_id, table) if self.guide else table

    def window_raw_tables(self, first_id, n, load_frame):
        """window_tables of the raw tables: int32 [n, blocks, 7]."""
        return torch.stack([self.raw_table_for(j, load_frame) for j in range(first_id, first_id + n)])

    def window_guide_counts(self, first_id, n):
        """int64 [n, 8]: the counts rows of the same pairs (zeros for a pair that was not guided: frame 0, a missing predecessor), after
        window_tables; None with guide=False."""
        if not self.guide:
            return None
        rows = [self._guide_counts.get(j) for j in range(first_id, first_id + n)]
        some = next((r for r in rows if r is not None), None)
        if some is None:
            return None
        return torch.stack([torch.zeros_like(some) if r is None else r for r in rows])

    def window_link_stats(self, first_id, n):
        """int32 [n, 4]: the stats rows of the same pairs (zeros for a pair without stats: no cut), after window_tables; None with both
        decisions off."""
        if self.intra_bias is None and self.scene_cut is None:
            return None
        rows = [self._stats.get(j) for j in range(first_id, first_id + n)]
        some = next((r for r in rows if r is not None), None)
        if some is None:
            return None
        return torch.stack([torch.zeros_like(some) if r is None else r for r in rows])

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
            check_geometry(int(cur.shape[0]), int(cur.shape[1]))
            table = self._table(frame_id, cur, ref)  # the search estimate_grids would make, shared with table_for
            with torch.cuda.device(table.device):
                out = tuple(motion_vectors_to_grids(table, int(cur.shape[0]), int(cur.shape[1]), validate=False))
        self._grids[frame_id] = out
        while len(self._grids) > self._cache_size:
            self._grids.popitem(last=False)
        return out
