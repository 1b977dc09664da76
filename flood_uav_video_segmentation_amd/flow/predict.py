"""predict_step on the HIP path -- mirrors the timed unit and the post-processing of the reference's
FlowBaseModel.predict_step / on_predict_end (flow/base.py:236-343) without Lightning:

    p = FlowPredictor(flow_model, classes=5, out_size=(1072, 1920), crop=None)
    masks = p.predict_window(frame_prev, frame_next, mvs_left, mvs_right)   # uint8 numpy [n, 1072, 1920]
    p.temporal_consistency()                                               # mIoU / mAcc / accuracy between consecutive frames

Extension (no reference counterpart): FlowPredictor(..., confidence=True) also returns a uint8 confidence plane per mask and keeps a
per-frame, per-class extent report on the device (ops.mask_confidence / canvas_confidence / frame_report):
    masks, conf = p.predict_window(...)
    p.extent_report()                                                      # int64 [frames, K, 3], read back once
FlowPredictor(..., regions=True) keeps a per-frame table of the masks' connected regions on the device, and min_region_area=N emits
masks without regions smaller than N pixels (ops.mask_regions / region_table / region_filter):
    rows, totals = p.region_report()                                       # per frame int64 [regions, 10]; read back once
FlowPredictor(..., regions=True, track=True) also links every frame's regions to those of the frame before it and gives each region a
track id that lasts as long as the region does (ops.region_links / region_tracks):
    tracks, overflowed = p.track_report()                                  # per frame int64 [regions, 4], parallel to rows
FlowPredictor(..., regions=True, track=True, compensate=True) compares each frame with the frame before it READ AT THE SOURCE of every
pixel under the block matcher's vectors, which the estimate-mode window datasets hand out with link_vectors=True (ops.region_links with
mv=): a region that moves further than its own width per frame keeps its track.
FlowPredictor(..., regions=True, outlines=True) also outlines every region on the device -- ordered polygons on the pixel lattice, the
outer contour and the holes, with the perimeter and the hole count per region (ops.region_outlines):
    frames, flags = p.outline_report()                                     # per frame (contour rows, vertices, shape rows); read back once
    write_outlines_geojson("o.geojson", ids, rows, (frames, flags))        # one Polygon feature per frame and region
FlowPredictor(..., regions=True, outlines=True, simplify=1.0) also simplifies every ring on the device to a tolerance in pixels
(ops.outline_simplify):
    simple, counts = p.simple_outline_report()                             # per frame (rows, kept vertices); counts [frames, 4]
    write_outlines_geojson("o.geojson", ids, rows, (frames, flags), simplified=(simple, counts), tolerance=1.0)
FlowPredictor(..., regions=True, track=True, keep_window_regions=True) keeps the newest window's index planes, tables and tracks on the
device so that the result video can show them (ops.compose_regions):
    frames = compose_window(masks, item, palette, dataset=ds, regions=p.window_regions(), style={"outline": rgba, "label_scale": 2})
FlowPredictor(..., stabilize=3) debounces every pixel's class along the time axis before anything else sees the masks: a class is emitted
once it has been observed 3 frames running (ops.mask_stabilize), optionally read along the block matcher's vectors
(stabilize_compensate=True) and with confident observations taken at once (stabilize_trust=T with confidence=True):
    p.stabilize_report()                                                   # int64 [frames, 4] = (held, switched, seeded, trusted)
FlowPredictor(..., regions=True, proximity=(8, 16, 32)) relates the classes to each other: the exact distance of every pixel to the nearest
water pixel of its frame, tabulated per class and per region (ops.mask_distance, ops.region_proximity), in mask pixels:
    exposure, near = p.proximity_report()                                  # [frames, K, B] pixels within each threshold; per frame [rows, 8]
    write_regions_csv("regions.csv", ids, rows, proximity=near)            # adds dist, near_px, nearest_region
    write_exposure_csv("exposure.csv", ids, exposure, (8, 16, 32), h * w)
FlowPredictor(..., mosaic=(4096, 4096)) registers every frame's mask to the first frame through the camera's motion -- one robust affine
per frame pair, fitted to the block matcher's vectors -- and accumulates the masks into one extent map in which each piece of ground is
counted once (ops.global_motion, ops.pose_chain, ops.mosaic_accumulate, ops.mosaic_resolve):
    cls, conf, seen, totals, poses = p.mosaic_report()                     # the mosaic mask, its confidence, votes, class areas, poses
    write_mosaic_csv("mosaic.csv", ids, poses, totals)
"""
import numpy as np
import torch

from .. import _lib, ops
from .._lib import check, ptr, stream_ptr
from . import crops
from .frame_rows import FrameRows
from .mosaic import (CHANGE_PALETTE, LINK_STATUS, MOSAIC_STATUS, PART_ARRAYS, REFINE_STATUS, RELOCATE_STATUS, _CHANGE_KEYS, _CHANGE_REGION_KEYS,  # noqa: F401
                     _CHANGE_REGISTER_KEYS, MosaicBuilder, _compose_q20, change_image, change_report, merge_part, mosaic_change, mosaic_part_arrays, part_seen_box,
                     read_mosaic_part, write_change_csv, write_change_png, write_merge_csv, write_mosaic_csv, write_mosaic_part, write_relocate_csv)

PALETTE = np.array(ops.FLOOD_PALETTE, dtype=np.uint8)  # dataset/flow/list/colors.txt (one table: ops.ortho_compose's default is the same object)


class FlowPredictor:
    """cache_keyframes=True + `key_ids=(prev_frame_id, next_frame_id)` in predict_window: the network output of the previous
    window's `frame_next` is reused when it is this window's `frame_prev` (flow/dataset.py:112-114 builds consecutive windows
    that way), so a video costs one new key-frame inference per window; masks are bit-identical to the uncached run.

    confidence=True (extension): predict_window returns, and predict_clip yields, (masks, conf) -- conf uint8 [n,H,W], 255 x the
    probability of the emitted class (the softmax of the frame's logits on the whole-frame route, the crop-averaged probability on
    the sliding-crop route).  The masks are the confidence=False masks bit for bit; they come from the same launch as the confidence,
    which needs the window's logits / canvas written out once (the masks-only tails skip that).  Every window's per-class report
    (pixels, sum of confidence codes, pixels with confidence < low_confidence) goes into rows of chunked device buffers; nothing is
    read back until extent_report().  Every stage below keeps its per-frame rows the same way, in a FrameRows of its own (REPORT_CHUNK
    frames a chunk; outline_chunk and simple_chunk for the two big ones), and clear_report() clears them all.

    regions=True (extension): every emitted mask is labelled (connectivity 4 or 8) and its region table -- per region class, area,
    bounding box, coordinate sums, and with confidence=True the confidence sum and the low-confidence pixels -- goes into chunked
    device buffers like the extent report: max_regions x 80 B per frame (1024 regions: 80 KiB a frame, 20 MiB per 256-frame chunk),
    nothing read back until region_report().  A frame with more regions keeps its first max_regions (in raster order of their first
    pixels) and reports the full count.  With min_region_area <= 1 the masks are the default masks bit for bit.
    min_region_area=N > 1 (extension): regions smaller than N pixels are re-classed by the vote of their 4-neighbours (one pass; a
    speckle nobody borders stays) before anything else sees the masks: what is returned, scored, reported and -- with regions=True,
    after labelling the filtered masks again -- tabulated are the filtered masks.  The confidence plane stays as computed: a
    re-classed pixel keeps the confidence of its old class.  The filter sees the first max_regions regions of a frame only (in
    raster order of their first pixels): by the definition a region past the cap is neither a speckle nor a voter, so on a frame with
    more regions than max_regions the lower part of the frame is left unfiltered.  The pass's region counts are kept on the device
    (16 B per frame); despeckle_counts() reads them back so that a caller can see such frames and raise max_regions.

    track=True (extension, needs regions=True): every tabulated frame is linked to the frame emitted before it -- the previous frame of
    the window, or the last frame of the window before, whose index plane (a copy), table, counts and tracks row the predictor keeps
    on the device -- by the pixel overlap of regions of one class, compared in place (no motion compensation), and every region gets
    (track id, parent id, previous row, overlap): a region that is its best predecessor's best successor continues that track, every
    other one is born with the next id and its best predecessor's track as parent.  A pair needs min_overlap pixels; max_pairs (a
    power of two, default the next one >= 4 max_regions) is the size of the pair table -- a frame pair with more distinct overlapping
    pairs gets no links (all its regions are born) and its flag in track_report().  max_regions x 32 B per frame in chunked device
    buffers beside the region tables.  Ids count from 0 and never restart: reset() (a new video) drops the previous frame, so the next
    frame's regions are all born, and keeps the next id; clear_report() drops the buffers and keeps both.

    compensate=True (extension, needs track=True): the links are motion-compensated -- every window must then come with link_mvs (int32
    [n, blocks, 7]: per emitted frame the block matcher's table of that frame against the frame before it), link_frame_size (the decoded
    frame's height and width) and optionally link_stats (int32 [n, 4], block_match_modes' stats rows: a pair flagged as a scene cut
    gets no links and its flag in track_report(with_cuts=True)).  A window without link_mvs raises: there is no silent fall-back to the
    in-place comparison.  The first frame after reset() has no frame before it, so its vectors are ignored.

    outlines=True (extension, needs regions=True): every tabulated frame's regions are outlined -- ordered polygons on the mask's pixel
    lattice, an outer contour and the holes per region, plus per region its perimeter, contour and vertex counts (ops.region_outlines;
    DESIGN §3.13) -- right behind the table of the (filtered) masks, into chunked device buffers beside the region tables; nothing is
    read back until outline_report().  Device memory per frame: 8 max_vertices + 48 max_contours + 24 max_regions + 32 bytes (at the
    defaults 472 KiB; a chunk holds as many frames as fit 64 MiB, 138 at the defaults), plus the op's workspace while a window is
    outlined.  A frame with more than max_vertices vertices gets NO contours and flag bit 0, one with more than max_contours contours
    keeps the first max_contours and flag bit 1; outline_report() hands the flags out.  The defaults (4096 contours, 32768 vertices) are
    guesses for ragged 1080p water masks: no default has been validated on real video.  The masks are not touched.

    simplify=TOL (extension, needs outlines=True; None: off): every outlined frame's rings are simplified on the device right behind
    the outlines -- Ramer-Douglas-Peucker per ring, every dropped vertex within TOL pixels of the kept segment that spans it
    (ops.outline_simplify) -- into chunked device buffers of their own (32 max_contours + 8 max_vertices + 32 bytes per
    frame); the outline buffers stay as they are, and nothing is read back until simple_outline_report().  simplify_rounds (1..256)
    caps the rounds: a ring with segments still open after the last round keeps all their vertices and is flagged, and the report's
    `rounds` column tells how many a frame needed.  The default of 32 is a guess for natural shorelines, NOT validated on real video.

    keep_window_regions=True (extension, needs regions=True): the index planes, table rows, counts and -- with track=True -- track rows of
    the MOST RECENT window stay reachable on the device through window_regions(), one tuple per frame, for ops.compose_regions /
    compose_window(regions=) to draw outlines, track colours and ids into the result video.  Views of the report
    buffers and the window's index tensor: no copy, nothing read back, valid until the next window.

    stabilize=N (extension; None, 0 or 1: off, and the op is never called): every window's masks go through ops.mask_stabilize with
    persist=N FIRST -- a pixel keeps its emitted class until another class has been observed N frames running, so a change that lasts is
    emitted N - 1 frames late and a flicker shorter than N frames never shows -- and what is despeckled, scored (temporal_consistency()
    included), tabulated, reported and returned are the stabilised masks.  The state plane (4 B per pixel) lives on the device across
    windows: reset() drops it, so the next frame seeds; clear_report() keeps it and drops the counts.  The per-frame counts (held,
    switched, seeded, trusted) go into chunked device buffers and are read back once by stabilize_report().  The confidence plane stays
    as computed: a held pixel keeps the confidence of the class it was OBSERVED as (the despeckle's rule).  Mask ids >= classes pass
    through.  stabilize_trust=T (0..256, needs confidence=True): an observation with confidence >= T is emitted at once.
    stabilize_compensate=True: the state is read at every pixel's source under the block matcher's vectors -- every window must then
    come with link_mvs and link_frame_size (and optionally link_stats: a frame flagged as a scene cut seeds), exactly what compensate=True
    takes; a window without them raises, there is no silent in-place fall-back.  Without it a moving scene is compared in place, where
    the filter lags behind the motion and can make the masks worse.  Under a sharded run every rank's block starts unseeded.  No default
    here has been validated on real video.

    proximity=(PX, ...) (extension, needs regions=True; None: off, and neither op is ever called): 1..8 strictly ascending distances in
    MASK PIXELS (of a moving, un-georeferenced camera: no metres follow from them).  Every window's masks -- the ones handed out, after
    the stabiliser and the despeckle -- go through ops.mask_distance with the classes proximity_sources (default (1,), water) as
    sources, and ops.region_proximity tabulates the field against the region tables' index planes: per frame and class of
    proximity_targets (default (3, 4), buildings and streets) the pixels within each threshold, and per region its smallest distance,
    where it is attained, the nearest source pixel and that pixel's region, and its pixels within the first threshold.  Both tables go
    into chunked device buffers in step with the region report's and are read back once by proximity_report(); clear_report() drops
    them, reset() keeps them.  proximity_max=R (1..32767, at least the largest threshold) bounds the search: a region further than R
    pixels from every source then reports min_d2 = -1, "not within R", and no scan is longer than R steps.  None or 0: unbounded, every
    region of a frame with a source gets its distance; a frame whose only source is a speck then costs a scan of up to the frame's
    width per pixel (measured at 7.4 ms for a 1072 x 1920 five-frame window against 0.18 ms on a flood scene and 0.45 ms at R = 32;
    DESIGN §3.17).  The thresholds and the class choices are guesses, NOT validated on real video.

    mosaic=(CH, CW) (extension; None: off, and none of its ops is ever called; it does not need regions=True): the flood-extent mosaic
    of DESIGN §3.18.  Every window must come with link_mvs and link_frame_size (and optionally link_stats), as for compensate=True.  The
    masks handed out -- after the stabiliser and the despeckle -- vote, per frame, into a uint16 canvas [mosaic_classes, CH, CW] that
    lives on the device with the pose chain's state; the first frame predicted is the anchor, placed with its top-left corner at
    mosaic_origin = (oy, ox) (None: centred).  ops.global_motion fits each pair's model with mosaic_rounds, mosaic_tol and
    mosaic_min_inliers, leaving out the blocks whose centre lies on a class of mosaic_exclude (default (1,), water: it moves on its
    own); up to mosaic_bridge failed pairs running are bridged with the last good model, after which -- or at a scene cut -- the chain is
    lost and the frames vote nowhere.  mosaic_report() resolves the canvas and reads back once; clear_report() drops canvas and state
    (the next frame anchors a new mosaic), reset() keeps them.  All these defaults are guesses, NOT validated on real video; an affine
    per pair is not a homography, the chain drifts over a long flight and nothing closes loops.  This and the stages below are
    flow/mosaic.py's: the predictor always makes ONE MosaicBuilder of its arguments (mosaic_builder; mosaic=None: one that is off) and hands it
    every window's masks; but for the switches mosaic, ortho, mosaic_refine and mosaic_relocate, settings and state are the builder's alone.

    ortho="centre" | "latest" (extension, needs mosaic=; None: off, and none of its ops is ever called): the orthophoto under that mosaic
    (DESIGN §3.19).  Every window must then also come with link_sources (the datasets' link_sources=True): after the pose chain each
    frame's pixels -- the uint8 image the network saw -- are gathered into a canvas of the mosaic's size by ops.ortho_accumulate with that
    frame's pose row and its ordinal, the number of frames since the anchor; a None entry (a frame that does not exist) is skipped.
    "centre": per canvas pixel the view in which the ground point is nearest the optical axis wins; "latest": the newest frame.
    ortho_report() draws it, by default with the extent map over it, and reads back once; clear_report() drops the canvas and the
    counter, reset() keeps them.  No feathering or exposure matching across seams, no lens model, the mask's resolution, and the chain's
    drift shows as broken seams; NOT validated on real video.

    mosaic_refine=True (extension, needs ortho=; False: off, none of its ops is ever called and MosaicBuilder.add's calls are what they were):
    frame-to-map registration.  The window is then walked frame by frame: pose_chain with n = 1; for a frame whose ordinal
    is a multiple of refine_every and whose source exists, ops.map_view draws the orthophoto canvas as the frame should see it under that
    pose, ops.block_match_modes (refine_search 1..32, refine_penalty, refine_intra_bias) matches the frame against it, ops.map_gate voids
    the rows that touch unmapped ground (or, with refine_min_age > 0, ground no frame at least that many ordinals older owns: loop
    closure on a revisit only), ops.global_motion fits the residual motion with the mosaic's own settings and ops.pose_correct folds it
    into the chain BEFORE the frame votes; then ops.ortho_accumulate with the corrected row, so a frame's view holds exactly the frames
    before it.  refine_report() -> int64 [frames, 8]: status (0 corrected, 1 not attempted, 2 no fit, 3 out of the pose bounds, 4 the
    chain is lost), usable rows, inliers, rounds, the fit's shift (x, y) in Q20, 0, 0.  Earlier frames are never re-posed, drift beyond
    refine_search is not recovered, and all these defaults are guesses, NOT validated on real video.

    mosaic_relocate=True (extension, needs mosaic_refine=True; False: off, none of its ops is ever called): a lost chain is relocalised
    against the orthophoto.  Behind its own registration, every frame whose source exists and whose ordinal is a multiple
    of relocate_every gets ops.map_coarse (relocate_scale 4, 8 or 16), ops.map_patch with the last pose the chain's state holds,
    ops.map_locate (relocate_min_overlap 0..1 of the patch's cells on mapped ground, relocate_exclude cells around the best placement
    that the runner-up must keep away from), ops.pose_relocate (relocate_max_mean, relocate_ratio), the fine registration above on the
    CANDIDATE pose, and ops.relocate_commit, which replaces the chain's state and the frame's row on the device only if the candidate
    passed all of it.  Nothing is read back, so the host does not know whether the chain is lost: the sequence runs for every such frame
    and its kernels return at once for a chain that is tracking (status 1).  A relocated frame votes and enters the orthophoto like a
    tracked one.  relocate_report() -> int64 [frames, 8]: status (0 relocated, 1 not attempted, 2 no placement, 3 rejected by the mean,
    4 rejected by uniqueness, 5 the fine registration failed, 6 the patch was refused, 7 out of the pose bounds), the shift in canvas
    pixels (x, y), sad*, n*, sad2, n2, eligible placements.  Translation only; flat water and repetitive ground are rejected, not placed;
    ground voted before the break is never re-posed; all these defaults are guesses, NOT validated on real video."""

    REPORT_CHUNK = 256  # frames per device buffer of the report: one allocation per 256 frames, not one per window

    def __init__(self, flow_model, classes=5, out_size=(1072, 1920), crop=None, compute_metrics=True, ignore_index=255,
                 cache_keyframes=False, confidence=False, low_confidence=128, regions=False, min_region_area=0, connectivity=8,
                 max_regions=1024, track=False, min_overlap=1, max_pairs=None, compensate=False, outlines=False, max_contours=4096,
                 max_vertices=32768, simplify=None, simplify_rounds=32, keep_window_regions=False, stabilize=None, stabilize_trust=None,
                 stabilize_compensate=False, proximity=None, proximity_sources=(1,), proximity_targets=(3, 4), proximity_max=None, mosaic=None,
                 mosaic_classes=None, mosaic_rounds=4, mosaic_tol=1.0, mosaic_min_inliers=12, mosaic_exclude=(1,), mosaic_bridge=2, mosaic_origin=None,
                 ortho=None, mosaic_refine=False, refine_search=8, refine_penalty=0, refine_intra_bias=65535, refine_min_age=0, refine_every=1,
                 mosaic_relocate=False, relocate_scale=8, relocate_every=1, relocate_min_overlap=0.5, relocate_exclude=2, relocate_max_mean=16, relocate_ratio=0.8):
        from .model import KeyframeCache

        self.model = flow_model
        self.key_cache = KeyframeCache() if cache_keyframes else None
        self.classes = classes
        self.out_size = tuple(out_size)
        self.crop = crop  # (crop_h, crop_w) -> sliding crops (no_cropping=False); None -> whole frame (no_cropping=True)
        self.compute_metrics = compute_metrics
        self.ignore_index = ignore_index
        self.last_output = None  # flow/base.py:247, :295
        self.hist = None         # int64[3,K]: intersection, |pred|, |target| accumulated over the run
        if not 0 <= int(low_confidence) <= 255:
            raise ValueError(f"FlowPredictor: low_confidence must be 0..255, got {low_confidence}")
        self.confidence = bool(confidence)
        self.low_confidence = int(low_confidence)
        self._extent = FrameRows(((classes, 3), torch.int64))  # the extent report's rows, REPORT_CHUNK frames a chunk
        if connectivity not in (4, 8):
            raise ValueError(f"FlowPredictor: connectivity must be 4 or 8, got {connectivity}")
        if not 1 <= int(max_regions) <= 65536:
            raise ValueError(f"FlowPredictor: max_regions must be 1..65536, got {max_regions}")
        if not 0 <= int(min_region_area) < 2 ** 31:
            raise ValueError(f"FlowPredictor: min_region_area must be 0..2^31 - 1, got {min_region_area}")
        self.regions = bool(regions)
        self.min_region_area = int(min_region_area)
        self.connectivity = int(connectivity)
        self.max_regions = int(max_regions)
        self._regions = FrameRows(((self.max_regions, 10), torch.int64), ((2,), torch.int64))  # (table, counts), REPORT_CHUNK frames a chunk
        self._despeckle_counts = []  # min_region_area > 1: the filter pass's int64 [n, 2] counts, one device tensor per window
        if track and not regions:
            raise ValueError("FlowPredictor: track=True needs regions=True (the tracks follow the region tables' rows)")
        if int(min_overlap) < 1 or int(min_overlap) >= 2 ** 31:
            raise ValueError(f"FlowPredictor: min_overlap must be 1..2^31 - 1, got {min_overlap}")
        pairs = ops.default_max_pairs(self.max_regions) if max_pairs is None else int(max_pairs)
        if not 16 <= pairs <= 2 ** 20 or pairs & (pairs - 1):
            raise ValueError(f"FlowPredictor: max_pairs must be a power of two in 16..2^20, got {max_pairs}")
        if compensate and not track:
            raise ValueError("FlowPredictor: compensate=True needs track=True (it changes how the tracks' links are counted)")
        self.track = bool(track)
        self.compensate = bool(compensate)
        self.min_overlap = int(min_overlap)
        self.max_pairs = pairs
        self._tracks = FrameRows(((self.max_regions, 4), torch.int64), ((2,), torch.int64))  # (tracks, link counts), in step with _regions
        self._track_prev = None   # the last tabulated frame: (index [H,W], table [max_regions,10], counts [2], tracks [max_regions,4]), copies
        self._track_state = None  # device int64 [2] = (next track id, 0)
        if outlines and not regions:
            raise ValueError("FlowPredictor: outlines=True needs regions=True (the outlines follow the region tables' index planes)")
        if not 1 <= int(max_contours) <= 2 ** 20 or not 4 <= int(max_vertices) <= 2 ** 22:
            raise ValueError(f"FlowPredictor: max_contours must be 1..2^20 and max_vertices 4..2^22, got {max_contours} and {max_vertices}")
        self.outlines = bool(outlines)
        self.max_contours = int(max_contours)
        self.max_vertices = int(max_vertices)
        per_frame = 8 * self.max_vertices + 48 * self.max_contours + 24 * self.max_regions + 32
        self.outline_chunk = max(1, min(self.REPORT_CHUNK, ((64 << 20) - 1) // per_frame))  # frames per device buffer: below 64 MiB
        self._outlines = FrameRows(((self.max_contours, 6), torch.int64), ((self.max_vertices, 2), torch.int32), ((self.max_regions, 3), torch.int64),
                                   ((4,), torch.int64))  # (contours, vertices, shape, counts), outline_chunk frames a chunk
        if simplify is not None and not outlines:
            raise ValueError("FlowPredictor: simplify needs outlines=True (it simplifies the rings the outlines just wrote)")
        if not 1 <= int(simplify_rounds) <= 256:
            raise ValueError(f"FlowPredictor: simplify_rounds must be 1..256, got {simplify_rounds}")
        if simplify is not None:
            ops.simplify_tol_q(simplify)  # ValueError outside 0..256 pixels
        self.simplify = None if simplify is None else float(simplify)
        self.simplify_rounds = int(simplify_rounds)
        per_frame = 8 * self.max_vertices + 32 * self.max_contours + 32
        self.simple_chunk = max(1, min(self.REPORT_CHUNK, ((64 << 20) - 1) // per_frame))  # frames per device buffer: below 64 MiB
        self._simple = FrameRows(((self.max_contours, 4), torch.int64), ((self.max_vertices, 2), torch.int32),
                                 ((4,), torch.int64))  # (simple, simple_vertices, simple_counts), simple_chunk frames a chunk
        if keep_window_regions and not regions:
            raise ValueError("FlowPredictor: keep_window_regions=True needs regions=True (it keeps the region tables' index planes and rows)")
        self.keep_window_regions = bool(keep_window_regions)
        self._window_regions = None  # the most recent window's pieces: [(index [take,H,W], table, counts, tracks or None)], device views
        persist = 0 if stabilize is None else int(stabilize)
        if not 0 <= persist <= 255:
            raise ValueError(f"FlowPredictor: stabilize must be 0..255 frames (None, 0 or 1: off), got {stabilize}")
        if persist <= 1 and (stabilize_trust is not None or stabilize_compensate):
            raise ValueError("FlowPredictor: stabilize_trust and stabilize_compensate need stabilize=N with N >= 2")
        if stabilize_trust is not None and not self.confidence:
            raise ValueError("FlowPredictor: stabilize_trust needs confidence=True (it compares the confidence plane with the threshold)")
        if stabilize_trust is not None and not 0 <= int(stabilize_trust) <= 256:
            raise ValueError(f"FlowPredictor: stabilize_trust must be 0..256, got {stabilize_trust}")
        self.stabilize = persist if persist > 1 else 0
        self.stabilize_trust = None if stabilize_trust is None else int(stabilize_trust)
        self.stabilize_compensate = bool(stabilize_compensate)
        self._stabilize_state = None   # the state plane int32 [H, W] on the device, carried from window to window
        self._stabilize_counts = FrameRows(((4,), torch.int64))  # the per-frame counts, REPORT_CHUNK frames a chunk
        self.proximity = None
        if proximity is not None:
            if not self.regions:
                raise ValueError("FlowPredictor: proximity needs regions=True (the distances are tabulated against the region tables' index planes)")
            thr = tuple(int(t) for t in proximity)
            if not 1 <= len(thr) <= 8 or any(not 0 <= t <= 32767 for t in thr) or any(b <= a for a, b in zip(thr, thr[1:])):
                raise ValueError(f"FlowPredictor: proximity must be 1..8 strictly ascending distances of 0..32767 pixels, got {proximity}")
            ops.class_set(proximity_sources, "proximity_sources", "FlowPredictor")
            ops.class_set(proximity_targets, "proximity_targets", "FlowPredictor", allow_empty=True)
            if proximity_max is not None and not 0 <= int(proximity_max) <= 32767:
                raise ValueError(f"FlowPredictor: proximity_max must be 0..32767 pixels (None or 0: unbounded), got {proximity_max}")
            if proximity_max is not None and 0 < int(proximity_max) < thr[-1]:
                raise ValueError(f"FlowPredictor: proximity_max={proximity_max} lies below the largest threshold {thr[-1]}: that threshold could never be told "
                                 "from the bound")
            self.proximity = thr
        self.proximity_sources = tuple(int(c) for c in proximity_sources)
        self.proximity_targets = tuple(int(c) for c in proximity_targets)
        self.proximity_max = int(proximity_max or 0) if self.proximity else 0
        self._proximity = FrameRows(((classes, len(self.proximity or ())), torch.int64), ((self.max_regions, 8), torch.int64))  # (exposure, near), in step with _regions
        # the mosaic family's settings and state (flow/mosaic.py): checked and kept there, also when mosaic is None
        self.mosaic_builder = MosaicBuilder(mosaic, self.classes if mosaic_classes is None else mosaic_classes, mosaic_rounds, mosaic_tol, mosaic_min_inliers,
                                            mosaic_exclude, mosaic_bridge, mosaic_origin, ortho, mosaic_refine, refine_search, refine_penalty, refine_intra_bias,
                                            refine_min_age, refine_every, mosaic_relocate, relocate_scale, relocate_every, relocate_min_overlap, relocate_exclude,
                                            relocate_max_mean, relocate_ratio, chunk=self.REPORT_CHUNK)
        self.mosaic, self.ortho = self.mosaic_builder.size, ortho  # the switches this class's own control flow reads
        self.mosaic_refine, self.mosaic_relocate = bool(mosaic_refine), bool(mosaic_relocate)
        self._guide_counts = FrameRows(((8,), torch.int64))   # the windows' link_guide_counts rows (the datasets' guide=True), as they come

    # the chunk lists that tests count, under the names they had before the tables moved into FrameRows
    _report_chunks = property(lambda self: self._extent.chunks)
    _region_chunks = property(lambda self: self._regions.chunks)
    _track_chunks = property(lambda self: self._tracks.chunks)
    _proximity_chunks = property(lambda self: self._proximity.chunks)

    def reset(self):
        """Start a new video: forget the cached key frame and the last mask (the temporal-consistency metric pairs each frame with
        its predecessor, flow/base.py:247,295 -- which must not be another video's last frame).  The histogram keeps running, and
        so do the extent report, the region report and the track ids (clear_report() drops the reports)."""
        if self.key_cache is not None:
            self.key_cache.clear()
        self.last_output = None
        self._track_prev = None  # the next frame's regions are all born; the next track id is kept
        self._stabilize_state = None  # the next frame seeds

    def clear_report(self):
        """Forget the extent report and the region report of the frames predicted so far."""
        for table in (self._extent, self._regions, self._tracks, self._outlines, self._simple, self._stabilize_counts, self._proximity, self._guide_counts):
            table.clear()  # the tracks' previous frame and next id stay, and so does the stabiliser's state plane
        self._despeckle_counts = []
        self.mosaic_builder.clear()  # the next frame anchors a new mosaic

    def extent_report(self):
        """confidence=True: int64 numpy [frames, K, 3] for every frame predicted since the start (or clear_report()), in the order
        the windows were predicted: per class the pixels, the sum of their confidence codes (mean confidence = sum / (255 pixels))
        and the pixels with confidence < low_confidence.  ONE read-back, here."""
        if not self._extent.chunks:
            return np.zeros((0, self.classes, 3), dtype=np.int64)
        return self._extent.flat().cpu().numpy()

    def _keep_report(self, masks, conf):
        """The window's report into the next rows of the chunked buffers (frame_report writes its rows whole; nothing is read)."""
        for done, take, _, (rows,) in self._extent.pieces(masks.shape[0], self.REPORT_CHUNK, masks.device):
            ops.frame_report(masks[done:done + take], conf[done:done + take], self.classes, self.low_confidence, out=rows)

    def region_report(self):
        """regions=True: (rows, totals) for every frame predicted since the start (or clear_report()), in the order the windows were
        predicted: rows[f] = int64 numpy [min(regions, max_regions), 10] (class, area, x0, y0, x1, y1, sum_x, sum_y, conf_sum,
        low_pixels), totals = int64 numpy [frames], the frames' full region counts (totals[f] > max_regions: the table is cut).  The
        read-back happens here and nowhere else, chunk by chunk into host arrays (no second copy of the report on the device)."""
        if not self._regions.chunks:
            return [], np.zeros((0,), dtype=np.int64)
        rows, totals = [], []
        for take, (table, counts) in self._regions.filled(self.REPORT_CHUNK):
            c, t = counts.cpu().numpy(), table.cpu().numpy()
            rows.extend(t[f, :int(c[f, 1])] for f in range(take))
            totals.append(c[:, 0])
        return rows, np.concatenate(totals)

    def despeckle_counts(self):
        """min_region_area > 1: int64 numpy [frames], the number of regions the filter pass found in each frame's unfiltered mask since
        the start (or clear_report()).  A value above max_regions marks a frame of which only the first max_regions regions were
        filtered.  One read-back, here."""
        if not self._despeckle_counts:
            return np.zeros((0,), dtype=np.int64)
        return torch.cat(self._despeckle_counts)[:, 0].cpu().numpy()

    def _despeckle(self, masks):
        """The masks without regions below min_region_area: label, tabulate, filter (nothing is read back)."""
        masks = masks.contiguous()
        labels = ops.mask_regions(masks, self.classes, self.connectivity)
        table, counts, index = ops.region_table(masks, labels, self.classes, None, self.low_confidence, self.max_regions)
        self._despeckle_counts.append(counts)
        return ops.region_filter(masks, index, table, self.classes, self.min_region_area)

    def _stabilize(self, masks, conf, link):
        """The window's masks through the debounce, the state plane carried on, the counts into the next rows of the chunked buffers
        (nothing is read back)."""
        kw = {} if not self.stabilize_compensate else dict(mv=link[0], frame_size=link[1], pair_stats=link[2])
        out, self._stabilize_state, counts = ops.mask_stabilize(masks.contiguous(), self._stabilize_state, conf if self.stabilize_trust is not None else None,
                                                                self.classes, self.stabilize, self.stabilize_trust, **kw)
        for done, take, _, (rows,) in self._stabilize_counts.pieces(out.shape[0], self.REPORT_CHUNK, out.device):
            rows.copy_(counts[done:done + take])
        return out

    def stabilize_report(self):
        """stabilize=N: int64 numpy [frames, 4] = (held, switched, seeded, trusted) pixels of every frame predicted since the start (or
        clear_report()), in the order the windows were predicted.  ONE read-back, here."""
        if not self._stabilize_counts.chunks:
            return np.zeros((0, 4), dtype=np.int64)
        return self._stabilize_counts.flat().cpu().numpy()

    def _keep_guide_counts(self, n, link_guide_counts):
        """A window's link_guide_counts (int64 [n, 8], ops.guide_vectors' counts of its n frame pairs; None: the window was not guided)
        into the next rows of the chunked buffers, device to device; nothing is read back."""
        if link_guide_counts is None:
            return
        if link_guide_counts.dtype != torch.int64 or tuple(link_guide_counts.shape) != (n, 8):
            raise ValueError(f"FlowPredictor: link_guide_counts must be int64 [{n}, 8] for the window's n = {n} frames, got {link_guide_counts.dtype} "
                             f"{tuple(link_guide_counts.shape)}")
        for done, take, _, (rows,) in self._guide_counts.pieces(n, self.REPORT_CHUNK, link_guide_counts.device):
            rows.copy_(link_guide_counts[done:done + take])

    def guide_report(self):
        """int64 numpy [frames, 8] = ops.GUIDE_COUNTS (blocks, void rows in, filled, outliers, replaced, dropped, kept by evidence, foreign)
        of the frame pair that ends in every frame predicted since the start (or clear_report()) whose window came with
        link_guide_counts, in the order the windows were predicted; a frame without a guided pair has a row of zeros.  ONE read-back, here."""
        if not self._guide_counts.chunks:
            return np.zeros((0, 8), dtype=np.int64)
        return self._guide_counts.flat().cpu().numpy()

    def _track_link(self, link):
        """What _link_inputs returned, for the tracks: theirs only under compensate=True (stabilize_compensate=True alone leaves them in place)."""
        return link if self.compensate else None

    # ---- the mosaic family: what mosaic_builder hands out, under the names and with the contracts it has here
    def mosaic_part(self):
        """mosaic=: this predictor's mosaic as a dict of DEVICE tensors and plain numbers, nothing read back: votes uint16 [K, CH, CW]; rank,
        rgba (ortho=; None without); state int64 [32]; poses int64 [frames, 16]; tail int64 [12], the two poses (to_anchor, from_anchor)
        after the last frame -- or after the last merged part's; origin (oy, ox); mask_size (H, W); frames, the next ordinal; mode.  The
        tensors are the predictor's own, not copies.  write_mosaic_part() saves it, another predictor's merge_mosaic() takes it."""
        return self.mosaic_builder.part()

    def merge_mosaic(self, part, link=None, **register):
        """Register another mosaic (mosaic_part()'s dict, or read_mosaic_part()'s) against this predictor's and fold it in: ops.register_mosaics
        on the two orthophotos (so both need ortho=), then ops.mosaic_merge with this predictor's frame count as the ordinal offset.
        link: int64 [16] on the device; default: this mosaic's tail with status 1 -- the multi-rank case, in which the part's anchor
        frame is the frame after this one's last.  **register goes to ops.register_mosaics; a place= without b_box takes the part's
        seen box where it has one.  Afterwards the ordinal counter has grown by the part's frames and, if the link was registered
        (decided on the device), the tail is compose(b_to_a, the part's tail).  Nothing is read back; merge_report() does that.
        Votes are not idempotent: merging the same part twice counts its frames twice."""
        return self.mosaic_builder.merge(part, link, **register)

    def change_against(self, part, **kw):
        """Where another mosaic of the same ground (mosaic_part()'s dict, or read_mosaic_part()'s) differs from this predictor's, in this
        one's canvas: mosaic_change(self.mosaic_part(), part, **kw).  Neither mosaic is changed; nothing is read back."""
        return self.mosaic_builder.change_against(part, **kw)

    def merge_report(self):
        """(links int64 numpy [parts, 16], outs: per part int64 [rows, 8] -- link_place's row first where a placement ran, then one
        link_correct row per round --, counts int64 [parts, 8]) of the parts merged since the start (or clear_report()).  The ONE read-back."""
        return self.mosaic_builder.merge_report()

    def relocate_report(self):
        """mosaic_relocate=True: int64 numpy [frames, 8], relocate_commit's out row of every frame predicted since the start (or
        clear_report()), in the order of mosaic_report()'s poses: status (0 relocated, 1 not attempted, 2 no placement, 3 rejected by the
        mean, 4 rejected by uniqueness, 5 the fine registration failed, 6 the patch was refused, 7 out of the pose bounds), the shift in
        canvas pixels x and y, sad*, n*, sad2, n2, eligible placements.  The ONE read-back."""
        return self.mosaic_builder.relocate_report()

    def refine_report(self):
        """mosaic_refine=True: int64 numpy [frames, 8], pose_correct's out row of every frame predicted since the start (or
        clear_report()), in the order of mosaic_report()'s poses: status (0 corrected, 1 not attempted, 2 no fit, 3 out of the pose
        bounds, 4 the chain is lost), usable rows, inliers, rounds done, the fit's shift x and y in Q20, 0, 0.  The ONE read-back."""
        return self.mosaic_builder.refine_report()

    def ortho_report(self, palette=PALETTE, alpha=None, edge=(), fill=(0, 0, 0), overlay=True):
        """ortho=: (image, src, covered) of the frames predicted since the start (or clear_report()): image uint8 numpy [CH, CW, 3], the
        orthophoto -- with overlay=True the mosaic's classes blended over it (palette, alpha and edge as ops.ortho_compose takes them) --
        showing `fill` where no frame has been; src int32 [CH, CW], the ordinal (frames since the anchor: the row of mosaic_report()'s
        poses) of the frame each pixel came from, -1 where none; covered, the number of canvas pixels some frame won.  mosaic_resolve
        (overlay=True) and ortho_compose run here, and so does the ONE read-back."""
        return self.mosaic_builder.ortho_report(palette, alpha, edge, fill, overlay)

    def mosaic_report(self):
        """mosaic=(CH, CW): (cls, conf, seen, totals, poses) of the frames predicted since the start (or clear_report()): cls uint8 numpy
        [CH, CW], the class most frames saw at each piece of ground (255: never seen); conf uint8, that class's share of the votes as a
        code 0..255; seen int32, the number of votes; totals int64 [K, 2], per class the canvas pixels and the votes; poses int64
        [frames, 16], per frame to_anchor (6) and from_anchor (6) in Q20, status (0 ok, 1 bridged, 2 lost), clipped, inliers, usable rows.
        The resolve pass runs here, and so does the ONE read-back."""
        return self.mosaic_builder.report()

    def _link_inputs(self, n, link_mvs, link_frame_size, link_stats, link_raw_mvs=None):
        """compensate=True, stabilize_compensate=True or mosaic=: the window's (mvs [n, blocks, 7], frame size, stats [n, 4] or None, raw
        mvs or None), checked; None otherwise.  The raw mvs are the tables as searched, which a dataset with guide=True hands out beside
        the guided link_mvs: the mosaic's camera fit takes them, so that it never feeds on rows a camera fit produced."""
        if not self.compensate and not self.stabilize_compensate and not self.mosaic:
            return None
        if (link_mvs is None or link_frame_size is None) and not self.compensate and not self.stabilize_compensate:
            raise ValueError("FlowPredictor: mosaic=(CH, CW) needs link_mvs and link_frame_size with every window (an estimate-mode dataset with "
                             "link_vectors=True provides them); the camera's motion is never taken as zero instead")
        if (link_mvs is None or link_frame_size is None) and not self.compensate:
            raise ValueError("FlowPredictor: stabilize_compensate=True needs link_mvs and link_frame_size with every window (an estimate-mode dataset "
                             "with link_vectors=True provides them); the state is never read in place instead")
        if link_mvs is None or link_frame_size is None:
            raise ValueError("FlowPredictor: compensate=True needs link_mvs and link_frame_size with every window (an estimate-mode dataset with "
                             "link_vectors=True provides them); the links are never compared in place instead")
        if link_mvs.dim() != 3 or link_mvs.shape[0] != n or (link_stats is not None and tuple(link_stats.shape) != (n, 4)):
            raise ValueError(f"FlowPredictor: link_mvs must be [n, blocks, 7] and link_stats [n, 4] for the window's n = {n} frames, got "
                             f"{tuple(link_mvs.shape)} and {None if link_stats is None else tuple(link_stats.shape)}")
        if link_raw_mvs is not None and (link_raw_mvs.shape != link_mvs.shape or link_raw_mvs.dtype != link_mvs.dtype):
            raise ValueError(f"FlowPredictor: link_raw_mvs must have link_mvs' shape and dtype, got {link_raw_mvs.dtype} {tuple(link_raw_mvs.shape)} and "
                             f"{link_mvs.dtype} {tuple(link_mvs.shape)}")
        return link_mvs, (int(link_frame_size[0]), int(link_frame_size[1])), link_stats, link_raw_mvs

    def _keep_regions(self, masks, conf, link=None):
        """The window's region tables into the next rows of the chunked buffers (region_table writes its rows whole; nothing is read)."""
        masks = masks.contiguous()
        labels = ops.mask_regions(masks, self.classes, self.connectivity)
        kept = []
        for done, take, row, (table, counts) in self._regions.pieces(masks.shape[0], self.REPORT_CHUNK, masks.device):
            _, _, index = ops.region_table(masks[done:done + take], labels[done:done + take], self.classes, None if conf is None else conf[done:done + take],
                                           self.low_confidence, self.max_regions, out=(table, counts))
            tracks = None
            if self.outlines:
                self._keep_outlines(index)
            if self.track:
                piece = None if link is None else (link[0][done:done + take], link[1], None if link[2] is None else link[2][done:done + take])
                tracks = self._keep_tracks(index, table, counts, row, piece)
            if self.proximity:
                self._keep_proximity(masks[done:done + take], index, counts, row)
            if self.keep_window_regions:
                kept.append((index, table, counts, tracks))
        if self.keep_window_regions:
            self._window_regions = kept

    def _keep_proximity(self, masks, index, counts, row):
        """The distance field of the piece region_table just tabulated (rows row.. of the newest chunk) and its two tables into the same
        rows of their own chunked buffers (region_proximity writes its rows whole; nothing is read back)."""
        rows = self._proximity.rows(row, masks.shape[0], self.REPORT_CHUNK, masks.device)
        d2, nearest = ops.mask_distance(masks, self.proximity_sources, self.proximity_max)
        ops.region_proximity(masks, d2, nearest, index, counts, self.classes, self.max_regions, self.proximity_targets, self.proximity, out=rows)

    def proximity_report(self):
        """proximity=(PX, ...): (exposure, near) for every frame of region_report(), in its order: exposure = int64 numpy [frames, K, B], the
        pixels of each target class within each threshold of a source pixel (cumulative over the thresholds; zero rows for the other
        classes); near[f] = int64 numpy [rows, 8] = (min_d2, at_x, at_y, src_x, src_y, src_row, near_pixels, 0), row for row
        region_report()'s rows[f]: the region's smallest squared distance to a source pixel (-1 in all six leading columns: the frame has
        no source pixel, or none within proximity_max), the pixel that attains it, the source pixel nearest to that one and its region's row (-1: none), and the region's
        pixels within the first threshold.  Distances are in mask pixels.  The read-back happens here, chunk by chunk."""
        if not self._proximity.chunks:
            return np.zeros((0, self.classes, len(self.proximity or ())), dtype=np.int64), []
        exposures, rows = [], []
        for take, (_, counts), (exposure, near) in self._regions.filled(self.REPORT_CHUNK, self._proximity):
            c, t = counts.cpu().numpy(), near.cpu().numpy()
            rows.extend(t[f, :int(c[f, 1])] for f in range(take))
            exposures.append(exposure.cpu().numpy())
        return np.concatenate(exposures), rows

    def window_regions(self):
        """keep_window_regions=True: the most recent window's regions as a list of n per-frame tuples (index int32 [H,W], table int64
        [max_regions,10], counts int64 [2], tracks int64 [max_regions,4] or None without track=True) -- what ops.compose_regions and
        compose_window(regions=) draw from.  Device tensors and views of the report buffers, nothing read back; valid until the next
        window is predicted.  The index planes are those of the masks the window handed out (the filtered ones under min_region_area)."""
        if not self.keep_window_regions:
            raise RuntimeError("FlowPredictor.window_regions: the predictor was not made with keep_window_regions=True")
        if self._window_regions is None:
            raise RuntimeError("FlowPredictor.window_regions: no window has been predicted yet")
        return [(index[f], table[f], counts[f], None if tracks is None else tracks[f])
                for index, table, counts, tracks in self._window_regions for f in range(index.shape[0])]

    def _keep_outlines(self, index):
        """The outlines of the index planes region_table just wrote into the next rows of their own chunked buffers (region_outlines
        writes its rows whole; nothing is read back)."""
        for done, take, _, rows in self._outlines.pieces(index.shape[0], self.outline_chunk, index.device):
            ops.region_outlines(index[done:done + take], self.max_regions, self.connectivity, self.max_contours, self.max_vertices, out=rows)
            if self.simplify is not None:
                self._keep_simple(rows[0], rows[1], rows[3])

    def _keep_simple(self, contours, vertices, counts):
        """The simplified rings of the outlines region_outlines just wrote into the next rows of their own chunked buffers
        (outline_simplify writes its rows whole; nothing is read back)."""
        for done, take, _, rows in self._simple.pieces(contours.shape[0], self.simple_chunk, contours.device):
            ops.outline_simplify(contours[done:done + take], vertices[done:done + take], counts[done:done + take], self.simplify, self.simplify_rounds,
                                 out=rows)

    def simple_outline_report(self):
        """simplify=TOL: (frames, counts) for every frame of outline_report(), in its order: frames[f] = (rows int64 numpy [rows, 4],
        vertices int32 numpy [kept, 2]) -- row for row outline_report()'s contour rows (first offset, kept count, area2 of the kept
        ring, flags: bit 0 unconverged) and the kept vertices back to back; counts = int64 numpy [frames, 4] = (rows, kept vertices,
        rounds, flags), flags bit 0: some ring still had open segments after simplify_rounds rounds (all their vertices are kept: raise
        simplify_rounds above the `rounds` column), bit 1: the frame's outlines had overflowed (nothing), bit 2: the outlines had more
        contours than rows, bit 3: inconsistent rows (nothing).  The read-back happens here, chunk by chunk."""
        if not self._simple.chunks:
            return [], np.zeros((0, 4), dtype=np.int64)
        frames, counts = [], []
        for take, (simple, vertices, cnt) in self._simple.filled(self.simple_chunk):
            c = cnt.cpu().numpy()
            rows, verts = simple.cpu().numpy(), vertices.cpu().numpy()
            frames.extend((rows[f, :int(c[f, 0])], verts[f, :int(c[f, 1])]) for f in range(take))
            counts.append(c)
        return frames, np.concatenate(counts)

    def outline_report(self):
        """outlines=True: (frames, flags) for every frame of region_report(), in its order: frames[f] = (contours int64 numpy [rows, 6],
        vertices int32 numpy [vertices, 2], shape int64 numpy [regions, 3]) -- the contour rows written (region row, first vertex
        offset, vertex count, cracks, area2, anchor), all vertex lists back to back, and row for row region_report()'s rows[f] the
        (perimeter, contours, vertices) of each region; flags = int64 numpy [frames], bit 0: more than max_vertices vertices (no
        contours at all for that frame, shape's contours column -1), bit 1: more than max_contours contours (the first max_contours
        are there).  The read-back happens here, chunk by chunk."""
        if not self._outlines.chunks:
            return [], np.zeros((0,), dtype=np.int64)
        regions = np.concatenate([counts[:, 1].cpu().numpy() for _, counts in self._regions.chunks])
        frames, flags = [], []
        for take, (contours, vertices, shape, counts) in self._outlines.filled(self.outline_chunk):
            c = counts.cpu().numpy()
            rows, verts, shp = contours.cpu().numpy(), vertices.cpu().numpy(), shape.cpu().numpy()
            for f in range(take):
                total = 0 if c[f, 3] & 1 else int(c[f, 2])
                frames.append((rows[f, :int(c[f, 1])], verts[f, :total], shp[f, :int(regions[len(frames)])]))
            flags.append(c[:, 3])
        return frames, np.concatenate(flags)

    def _keep_tracks(self, index, table, counts, row, link=None):
        """Links and track ids of the piece region_table just wrote (rows row.. of the newest chunk), against the frame tabulated before
        it; then that piece's last frame becomes the previous frame.  Nothing is read back.  link: the piece's (mvs, frame size, stats)
        under compensate=True.  Returns the piece's track rows (views of the buffer)."""
        tracks, flags = self._tracks.rows(row, index.shape[0], self.REPORT_CHUNK, index.device)
        if self._track_state is None:
            self._track_state = torch.zeros(2, dtype=torch.int64, device=index.device)
        prev = self._track_prev
        kw = {} if link is None else dict(mv=link[0], frame_size=link[1], pair_stats=link[2])
        back, fwd, link_counts = ops.region_links(index, table, counts, None if prev is None else prev[:3], self.max_pairs, self.min_overlap, **kw)
        ops.region_tracks(back, fwd, counts, self._track_state, None if prev is None else prev[3], out=tracks)
        flags.copy_(link_counts)
        self._track_prev = (index[-1].clone(), table[-1].clone(), counts[-1].clone(), tracks[-1].clone())
        return tracks

    def track_report(self, with_cuts=False):
        """track=True: (tracks, overflowed) for every frame of region_report(), in its order: tracks[f] = int64 numpy [rows, 4] = (track
        id, parent id, the row of the best predecessor in the frame before or -1, the overlap with it), row for row region_report()'s
        rows[f]; overflowed = int64 numpy [frames], 1 where the frame's pair table overflowed (all its regions were born: raise
        max_pairs).  with_cuts=True appends cuts = int64 numpy [frames], 1 where compensate=True found the pair flagged as a scene cut
        (all its regions were born as well).  The read-back happens here, chunk by chunk."""
        if not self._tracks.chunks:
            return ([], np.zeros((0,), dtype=np.int64)) + ((np.zeros((0,), dtype=np.int64),) if with_cuts else ())
        rows, flags = [], []
        for take, (_, counts), (tracks, link_counts) in self._regions.filled(self.REPORT_CHUNK, self._tracks):
            c, t = counts.cpu().numpy(), tracks.cpu().numpy()
            rows.extend(t[f, :int(c[f, 1])] for f in range(take))
            flags.append(link_counts[:, 1].cpu().numpy())
        flags = np.concatenate(flags)                                        # the flag word: bit 0 overflow, bit 1 cut
        return (rows, flags & 1, (flags >> 1) & 1) if with_cuts else (rows, flags & 1)

    def _finish(self, masks, conf, n, to_host, link=None, sources=None):
        """Stabilise, despeckle, score, keep the reports, and hand out what the caller asked for: masks, or (masks, conf) with
        confidence=True."""
        if self.stabilize:
            masks = self._stabilize(masks, conf, link)
        if self.min_region_area > 1:
            masks = self._despeckle(masks)
        self._score(masks, n)
        if self.regions:
            self._keep_regions(masks, conf, self._track_link(link))
        if self.mosaic:
            self.mosaic_builder.add(masks, link, sources, self.REPORT_CHUNK)
        if not self.confidence:
            return masks.cpu().numpy() if to_host else masks            # :277
        self._keep_report(masks, conf)
        return (masks.cpu().numpy(), conf.cpu().numpy()) if to_host else (masks, conf)

    def predict_window(self, frame_prev, frame_next, mvs_left, mvs_right, profiler=None, to_host=True, key_ids=None, key_cache=None,
                       weights=None, link_mvs=None, link_frame_size=None, link_stats=None, link_sources=None, link_raw_mvs=None,
                       link_guide_counts=None):
        """key_cache: a KeyframeCache to use for this call instead of the predictor's own (predict_clip's fallback passes a
        cache that lives for the clip only).  weights: an item's "weights" (the window datasets' hold_cuts; ops.window_weights) for
        the whole-frame and the sliding-crop tails alike, None = the reference's blend.  The key-frame cache is unaffected: the
        network's outputs do not depend on them.  link_mvs, link_frame_size, link_stats: an item's keys of those names (the estimate-mode
        datasets' link_vectors=True), needed and used with compensate=True only.  link_sources: an item's key of that name (the datasets'
        link_sources=True), needed and used with ortho= only.  link_raw_mvs: an item's key of that name (the datasets' guide=True): the
        tables as searched, which the mosaic's camera fit takes in place of the guided link_mvs; tracks and stabiliser take link_mvs.
        link_guide_counts: an item's key of that name, kept for guide_report()."""
        assert frame_prev.shape[0] == 1                      # flow/base.py:263
        assert len(mvs_left) == len(mvs_right)               # :264
        n = len(mvs_left) + 1                                # :266 -- the list length encodes n, also for no_warp dummies
        link = self._link_inputs(n, link_mvs, link_frame_size, link_stats, link_raw_mvs)
        self._keep_guide_counts(n, link_guide_counts)
        sources = self.mosaic_builder.check_sources(n, link_sources)
        cache = key_cache if key_cache is not None else self.key_cache
        kc = cache.window(*key_ids) if (cache is not None and key_ids is not None) else None
        conf = None
        if self.confidence and self.crop is None:
            extra = {} if kc is None else {"key_cache": kc}
            if weights is not None:
                extra["weights"] = weights
            logits = self.model.predict(frame_prev, frame_next, mvs_left, mvs_right, n, profiler, **extra)["pred"]
            masks, conf = ops.mask_confidence(logits, self.out_size)   # :275-276 and the winning class's softmax, one launch
        elif self.confidence:
            canvas = crops.compute_output(self.model, n, frame_prev, frame_next, mvs_left, mvs_right, self.crop[0], self.crop[1],
                                          self.classes, profiler, want_mask=False, key_cache=kc, out_size=self.out_size, want_canvas=True,
                                          weights=weights)
            masks, conf = ops.canvas_confidence(canvas, self.out_size)
        elif self.crop is None:
            extra = {} if kc is None else {"key_cache": kc}
            if weights is not None:
                extra["weights"] = weights
            if self._native(frame_prev) and not getattr(self.model, "feature_based", True) and hasattr(self.model, "predict_masks"):
                # out_size IS the frame size: the align_corners=True resize of :275 is the identity (source index = destination
                # index, weight 0), so :275-276 is the argmax of the logits themselves -- which the fused tail emits without
                # writing the fp32 logits out and reading them back
                masks = self.model.predict_masks(frame_prev, frame_next, mvs_left, mvs_right, n, profiler, **extra)
            else:
                logits = self.model.predict(frame_prev, frame_next, mvs_left, mvs_right, n, profiler, **extra)["pred"]
                masks = ops.resize_argmax_u8(logits, self.out_size)       # :275-276 without the fp32 intermediate
        else:
            # :273 compute_output, then :275-276 (float64 resize + argmax) fused into the canvas's last pass
            _, masks = crops.compute_output(self.model, n, frame_prev, frame_next, mvs_left, mvs_right, self.crop[0], self.crop[1],
                                            self.classes, profiler, want_mask=True, key_cache=kc, out_size=self.out_size, want_canvas=False,
                                            weights=weights)
        return self._finish(masks, conf, n, to_host, link, sources)

    def _native(self, frame):
        return self.out_size == (frame.shape[2], frame.shape[3])

    def _score(self, masks, n):
        if self.compute_metrics:                                      # :280-295 temporal consistency between consecutive frames
            for p in range(n):
                prev = masks[p - 1] if p > 0 else self.last_output
                if prev is not None:
                    self.hist = ops.iou_hist(masks[p], prev, self.classes, self.ignore_index, self.hist)
            self.last_output = masks[n - 1].clone()

    def predict_clip(self, items, profiler=None, to_host=True, keys_per_pass=2):
        """A clip's consecutive windows (dicts as PredictWindows yields them: frame_prev, frame_next, mvs_left, mvs_right,
        key_ids) with the key-frame cache AND look-ahead: key frames go through the network two at a time (each exactly once),
        and a window is emitted as soon as both of its key frames are there -- every key frame at the efficiency of a full batch
        (a lone frame runs ~10 % slower per frame: half-empty tile rounds).  Yields the masks of every window, in order,
        bit-identical to predict_window on the same windows (a frame's network output does not depend on its batch).

        `items` is consumed LAZILY: windows are pulled only until two not-yet-segmented key frames are at hand, so at most two
        windows' frames (and three key frames' low-resolution logits) are alive at once, however long the clip -- a lazily
        loading iterable such as PredictWindows streams.  Segmentation mode (whole frame or sliding crops); feature mode, a
        network without a fused `segment`, or a window without key_ids take predict_window with a cache that lives for this
        clip only (the predictor's own cache, when it has one).

        keys_per_pass (round 5; whole-frame route): how many NEW key frames go through the network per pass.  2 = one window of
        look-ahead.  4 or 6 trade latency (that many windows are pulled ahead) for throughput: a pass over four frames costs 8 % less per
        frame than two passes over two (11 % at six; profiles/r05_experiments.txt section 9) -- every launch of layers 1-3 is short enough
        to be bound by its fixed cost.  Masks stay bit-identical (a frame's network output does not depend on its batch)."""
        from collections import deque

        from .model import KeyframeCache, _region

        fm = self.model
        lookahead = not getattr(fm, "feature_based", True) and hasattr(fm.model, "segment") and hasattr(fm.model, "encode_frames")
        group = max(2, int(keys_per_pass)) if self.crop is None else 2  # the sliding-crop route batches the crops of TWO frames
        local_cache = self.key_cache if self.key_cache is not None else KeyframeCache()
        store = {}         # frame id -> decoder logits of that key frame ([1,K,fh,fw]; [ncrops,K,fh,fw] on the sliding-crop route)
        queue = []         # key frames not segmented yet, in order of first use: (frame id, tensor)
        pending = deque()  # windows pulled from `items` and not emitted yet
        last_next = None   # the newest emitted window's next key: the window still to come names it as its previous key
        it = iter(items)
        exhausted = False

        def run(frames):  # the queued key frames (up to `group`) through the network as ONE batch
            with _region(profiler, "predict_encoder"), _region(profiler, "predict_decoder"):
                if self.crop is None:
                    lows = fm._segment(*frames)
                    return [lows[j:j + 1] for j in range(len(frames))]
                a, b = crops.segment_crop_windows(fm, frames[0], frames[1] if len(frames) > 1 else None, self.crop[0], self.crop[1])
                return [a] if b is None else [a, b]

        def emit(w):
            assert w["frame_prev"].shape[0] == 1 and len(w["mvs_left"]) == len(w["mvs_right"])   # flow/base.py:263-264
            n = len(w["mvs_left"]) + 1
            link = self._link_inputs(n, w.get("link_mvs"), w.get("link_frame_size"), w.get("link_stats"), w.get("link_raw_mvs"))
            self._keep_guide_counts(n, w.get("link_guide_counts"))
            sources = self.mosaic_builder.check_sources(n, w.get("link_sources"))
            lo_prev, lo_next = store[w["key_ids"][0]], store[w["key_ids"][1]]
            h, wd = w["frame_prev"].shape[2], w["frame_prev"].shape[3]
            conf = None
            if self.confidence and self.crop is None:
                with _region(profiler, "predict_warp"), _region(profiler, "predict_fusion"):
                    logits, _ = ops.seg_tail(lo_prev, lo_next, w["mvs_left"], w["mvs_right"], n, (h, wd), fm.no_warp, want_logits=True, weights=w.get("weights"))
                masks, conf = ops.mask_confidence(logits, self.out_size)
            elif self.confidence:
                canvas = crops.compute_output(fm, n, w["frame_prev"], w["frame_next"], w["mvs_left"], w["mvs_right"], self.crop[0],
                                              self.crop[1], self.classes, profiler, want_mask=False, out_size=self.out_size,
                                              lows=(lo_prev, lo_next), want_canvas=True, weights=w.get("weights"))
                masks, conf = ops.canvas_confidence(canvas, self.out_size)
            elif self.crop is None and self._native(w["frame_prev"]):
                with _region(profiler, "predict_warp"), _region(profiler, "predict_fusion"):  # identity resize: see predict_window
                    _, masks = ops.seg_tail(lo_prev, lo_next, w["mvs_left"], w["mvs_right"], n, (h, wd), fm.no_warp, want_logits=False, want_mask=True,
                                                weights=w.get("weights"))
            elif self.crop is None:
                with _region(profiler, "predict_warp"), _region(profiler, "predict_fusion"):
                    logits, _ = ops.seg_tail(lo_prev, lo_next, w["mvs_left"], w["mvs_right"], n, (h, wd), fm.no_warp, want_logits=True, weights=w.get("weights"))
                masks = ops.resize_argmax_u8(logits, self.out_size)
            else:
                _, masks = crops.compute_output(fm, n, w["frame_prev"], w["frame_next"], w["mvs_left"], w["mvs_right"], self.crop[0],
                                                self.crop[1], self.classes, profiler, want_mask=True, out_size=self.out_size,
                                                lows=(lo_prev, lo_next), want_canvas=False, weights=w.get("weights"))
            return self._finish(masks, conf, n, to_host, link, sources)

        while True:
            plain = None  # a window that cannot take the look-ahead route (no key_ids / feature mode / foreign network)
            while len(queue) < group and not exhausted and plain is None:
                if pending and not queue and all(k in store for k in pending[0]["key_ids"]):
                    break  # nothing to wait for: emit before pulling more
                try:
                    w = next(it)
                except StopIteration:
                    exhausted = True
                    break
                if not lookahead or w.get("key_ids") is None:
                    plain = w
                    break
                pending.append(w)
                for fid, t in zip(w["key_ids"], (w["frame_prev"], w["frame_next"])):
                    if fid not in store and all(fid != q for q, _ in queue):
                        queue.append((fid, t))
            # segment what is queued: full groups while there are full groups; a smaller one only when nothing can join it any more
            while len(queue) >= group or (queue and (exhausted or plain is not None)):
                pair, queue = queue[:group], queue[group:]
                for (fid, _), lo in zip(pair, run([t for _, t in pair])):
                    store[fid] = lo
            while pending and all(k in store for k in pending[0]["key_ids"]):
                w = pending.popleft()
                last_next = w["key_ids"][1]
                yield emit(w)
            live = {k for w in pending for k in w["key_ids"]} | {last_next}
            store = {k: v for k, v in store.items() if k in live}  # only what a window still to come can need
            if plain is not None:
                yield self.predict_window(plain["frame_prev"], plain["frame_next"], plain["mvs_left"], plain["mvs_right"], profiler, to_host,
                                          plain.get("key_ids"), key_cache=local_cache, weights=plain.get("weights"), link_mvs=plain.get("link_mvs"),
                                          link_frame_size=plain.get("link_frame_size"), link_stats=plain.get("link_stats"),
                                          link_sources=plain.get("link_sources"), link_raw_mvs=plain.get("link_raw_mvs"),
                                          link_guide_counts=plain.get("link_guide_counts"))
            elif exhausted and not pending and not queue:
                return

    def temporal_consistency(self):
        """on_predict_end's summary (flow/base.py:330-343): (mIoU, mAcc, accuracy) with the reference's 1e-10 epsilon."""
        if self.hist is None:
            return None
        h = self.hist.cpu().numpy().astype(np.float64)
        inter, union, target = h[0], h[1] + h[2] - h[0], h[2]
        return float(np.mean(inter / (union + 1e-10))), float(np.mean(inter / (target + 1e-10))), float(inter.sum() / (target.sum() + 1e-10))


class FlowEvaluator:
    """validation_step / test_step on the HIP path (flow/base.py:143-176, summary of on_test_epoch_end in
    base/foundation.py): one interpolated frame per item from FlowModel.forward, argmax, intersection / union / target
    histograms against the label, one meter set per test list (Florida = 0, Texas = 1, flow/base.py:170-175).

        ev = FlowEvaluator(flow_model, classes=5, crop=(713, 713))       # crop=None <=> no_cropping=True
        for item in EvalWindows(...): ev.test_step(item, test_idx=0)
        miou, macc, acc, iou_class, acc_class = ev.summary(0)
    """

    def __init__(self, flow_model, classes=5, crop=None, ignore_index=255):
        self.model = flow_model
        self.classes, self.crop, self.ignore_index = classes, crop, ignore_index
        self.hist = {}  # meter id -> int64[3,K] (intersection, |pred|, |target|)

    def forward(self, frame_prev, frame_next, mvs_left, mvs_right, left_index, right_index):
        return self.model(None, frame_prev, frame_next, mvs_left, mvs_right, left_index, right_index)   # flow/base.py:134-135

    def _update(self, meter, pred, label):
        pred, label = pred.to(torch.uint8).contiguous(), label.to(torch.uint8).contiguous()   # ids 0..K-1 and 255 fit
        self.hist[meter] = ops.iou_hist(pred, label, self.classes, self.ignore_index, self.hist.get(meter))

    def validation_step(self, batch):
        out = self.forward(batch["frame_prev"], batch["frame_next"], batch["mvs_left"], batch["mvs_right"], batch["left_index"],
                           batch["right_index"])["pred"]
        pred = ops.argmax_u8(out)
        self._update("val", pred, batch["label"])
        return pred

    def test_step(self, batch, test_idx=0):
        frame_prev, frame_next, label = batch["frame_prev"], batch["frame_next"], batch["label"]
        assert frame_prev.shape[0] == 1 and label.shape[0] == 1                                    # flow/base.py:160
        li, ri = batch["left_index"], batch["right_index"]
        if self.crop is None:
            out = self.forward(frame_prev, frame_next, batch["mvs_left"], batch["mvs_right"], li, ri)["pred"]
            pred = ops.argmax_u8(out)
        else:
            fn = lambda p, q, ml, mr: self.forward(p, q, ml, mr, li, ri)["pred"]                # compute_test_crop (:212-222)
            _, pred = crops.compute_output(self.model, frame_prev.shape[0], frame_prev, frame_next, batch["mvs_left"],
                                           batch["mvs_right"], self.crop[0], self.crop[1], self.classes, want_mask=True,
                                           function=fn)
        self._update(1 if test_idx > 0 else 0, pred, label)
        return pred

    def summary(self, meter=0):
        """(mIoU, mAcc, accuracy, iou_class, accuracy_class) with the reference's 1e-10 epsilon (flow/base.py:332-336)."""
        if meter not in self.hist:
            return None
        h = self.hist[meter].cpu().numpy().astype(np.float64)
        inter, union, target = h[0], h[1] + h[2] - h[0], h[2]
        iou_class, acc_class = inter / (union + 1e-10), inter / (target + 1e-10)
        return float(np.mean(iou_class)), float(np.mean(acc_class)), float(inter.sum() / (target.sum() + 1e-10)), iou_class, acc_class


def write_extent_csv(path, frame_ids, report, frame_pixels, with_confidence=True):
    """One CSV row per frame from an extent report int64 [frames, K, 3] (FlowPredictor.extent_report / ops.frame_report read back):
    frame id, then per class k  area_k = pixels / frame_pixels,  conf_k = sum / (255 pixels)  (mean confidence, empty for a class
    without pixels)  and  low_k = low-confidence pixels / pixels  (0 without pixels).  with_confidence=False: the areas only."""
    report = np.asarray(report)
    if report.ndim != 3 or report.shape[2] != 3 or len(frame_ids) != report.shape[0]:
        raise ValueError(f"write_extent_csv: report must be [frames, K, 3] with one frame id per row, got {report.shape} and {len(frame_ids)} ids")
    classes = report.shape[1]
    cols = ["frame"] + [f"{name}_{k}" for k in range(classes) for name in (("area", "conf", "low") if with_confidence else ("area",))]
    with open(path, "w", newline="") as f:
        f.write(",".join(cols) + "\n")
        for fid, rows in zip(frame_ids, report):
            cells = [str(int(fid))]
            for pixels, total, low in rows.tolist():
                cells.append(f"{pixels / frame_pixels:.6f}")
                if with_confidence:
                    cells.append(f"{total / (255.0 * pixels):.6f}" if pixels else "")
                    cells.append(f"{low / pixels:.6f}" if pixels else "0.000000")
            f.write(",".join(cells) + "\n")


def write_exposure_csv(path, frame_ids, exposure, thresholds, frame_pixels):
    """One CSV row per frame from FlowPredictor.proximity_report()'s exposure int64 [frames, K, B] (ops.region_proximity read back) and
    the thresholds it was made with: frame id, then per class k and threshold t  within_k_t = the pixels of class k within t mask pixels
    of a source pixel  and  share_k_t = within / frame_pixels.  Classes that were no targets have zeros.  Distances are mask pixels of
    a moving camera, not metres."""
    exposure = np.asarray(exposure)
    if exposure.ndim != 3 or len(frame_ids) != exposure.shape[0] or exposure.shape[2] != len(thresholds):
        raise ValueError(f"write_exposure_csv: exposure must be [frames, K, {len(thresholds)}] with one frame id per row, got {exposure.shape} and "
                         f"{len(frame_ids)} ids")
    cols = ["frame"] + [f"{name}_{k}_{int(t)}" for k in range(exposure.shape[1]) for t in thresholds for name in ("within", "share")]
    with open(path, "w", newline="") as f:
        f.write(",".join(cols) + "\n")
        for fid, rows in zip(frame_ids, exposure):
            cells = [str(int(fid))]
            for pixels in rows.reshape(-1).tolist():
                cells += [str(pixels), f"{pixels / frame_pixels:.6f}"]
            f.write(",".join(cells) + "\n")


def write_guide_csv(path, frame_ids, counts):
    """FlowPredictor.guide_report()'s (or GridEstimator.guide_report()'s) int64 [m, 8] counts with their frame ids as a CSV, one row per
    frame (the pair that ends in that frame): frame, then ops.GUIDE_COUNTS (blocks, void rows in, filled, outliers, replaced, dropped, kept by evidence, foreign)."""
    from ..ops import GUIDE_COUNTS

    with open(path, "w") as fh:
        fh.write("frame," + ",".join(GUIDE_COUNTS) + "\n")
        for frame, row in zip(frame_ids, counts):
            fh.write(f"{int(frame)}," + ",".join(str(int(v)) for v in row) + "\n")


def _distance_cell(min_d2):
    """sqrt(min_d2) in mask pixels, empty for -1 (no source within reach)."""
    return f"{float(min_d2) ** 0.5:.3f}" if min_d2 >= 0 else ""


def write_regions_csv(path, frame_ids, rows, with_confidence=True, tracks=None, shapes=None, proximity=None):
    """One CSV row per frame and region from FlowPredictor.region_report()'s rows (per frame int64 [regions, 10]): frame id, the
    region's number in the frame, class, area, the inclusive box x0, y0, x1, y1, the centroid cx = sum_x / area, cy = sum_y / area,
    and with_confidence: conf = conf_sum / (255 area) (mean confidence) and low = low-confidence pixels / area.  tracks =
    FlowPredictor.track_report()'s rows (per frame int64 [regions, 4]): the columns track, parent (-1: none) and overlap (the pixels
    shared with the best predecessor in the frame before) are appended; None: the file without them, byte for byte.  shapes = per
    frame the int64 [regions, 3] shape rows of FlowPredictor.outline_report(): the columns perimeter and holes (contours - 1; -1 for a
    frame whose outlines overflowed) are appended; None: the file without them, byte for byte.  proximity = per frame the int64
    [regions, 8] near rows of FlowPredictor.proximity_report(): the columns dist (the region's smallest distance to a source pixel in
    mask pixels, empty: none within reach), near_px (its pixels within the first threshold) and nearest_region (the number, in the same
    frame, of the region the nearest source pixel lies in; -1: none) are appended, and with tracks also nearest_track, that region's
    track id (-1: none); None: the file without them, byte for byte."""
    if proximity is not None and (len(proximity) != len(rows) or any(len(t) != len(r) for t, r in zip(proximity, rows))):
        raise ValueError("write_regions_csv: proximity must hold one row per region of every frame")
    if len(frame_ids) != len(rows):
        raise ValueError(f"write_regions_csv: one frame id per frame, got {len(frame_ids)} ids for {len(rows)} frames")
    if tracks is not None and (len(tracks) != len(rows) or any(len(t) != len(r) for t, r in zip(tracks, rows))):
        raise ValueError("write_regions_csv: tracks must hold one row per region of every frame")
    if shapes is not None and (len(shapes) != len(rows) or any(len(t) != len(r) for t, r in zip(shapes, rows))):
        raise ValueError("write_regions_csv: shapes must hold one row per region of every frame")
    with open(path, "w") as fh:
        fh.write("frame,region,class,area,x0,y0,x1,y1,cx,cy" + (",conf,low" if with_confidence else "") + (",track,parent,overlap" if tracks is not None else "")
                 + (",perimeter,holes" if shapes is not None else "")
                 + ((",dist,near_px,nearest_region" + (",nearest_track" if tracks is not None else "")) if proximity is not None else "") + "\n")
        for f, (fid, frame) in enumerate(zip(frame_ids, rows)):
            for r, (cls, area, x0, y0, x1, y1, sx, sy, cs, lo) in enumerate(np.asarray(frame).tolist()):
                cells = [str(fid), str(r), str(cls), str(area), str(x0), str(y0), str(x1), str(y1), f"{sx / area:.3f}", f"{sy / area:.3f}"]
                if with_confidence:
                    cells += [f"{cs / (255.0 * area):.6f}", f"{lo / area:.6f}"]
                if tracks is not None:
                    tid, parent, _, overlap = np.asarray(tracks[f][r]).tolist()
                    cells += [str(tid), str(parent), str(overlap)]
                if shapes is not None:
                    perimeter, contours, _ = np.asarray(shapes[f][r]).tolist()
                    cells += [str(perimeter), str(contours - 1 if contours >= 0 else -1)]
                if proximity is not None:
                    min_d2, _, _, _, _, src_row, near_px, _ = np.asarray(proximity[f][r]).tolist()
                    cells += [_distance_cell(min_d2), str(near_px), str(src_row)]
                    if tracks is not None:
                        cells.append(str(int(np.asarray(tracks[f][src_row])[0])) if 0 <= src_row < len(tracks[f]) else "-1")
                fh.write(",".join(cells) + "\n")


def write_outlines_geojson(path, frame_ids, rows, outlines, tracks=None, simplified=None, tolerance=None):
    """The regions' shapes as one GeoJSON FeatureCollection, one Feature per frame and region, from region_report()'s rows and
    outlines = FlowPredictor.outline_report()'s (frames, flags).  The geometry is a Polygon whose rings are the region's outer contour
    first, then its holes, each closed by repeating its first vertex; the coordinates are mask pixel lattice coordinates (x to the
    right, y down; no georeferencing).  Properties: frame, region, class, area, perimeter, holes, and with tracks =
    track_report()'s rows also track and parent.  A frame whose flag bit 0 is set (more vertices than max_vertices: it has no contours)
    contributes no features and is named in the top-level list "overflowed_frames"; a frame with bit 1 (more contours than
    max_contours) is named in "truncated_frames", and its regions come with the rings that have rows -- a region whose outer contour
    has none is left out.
    simplified = FlowPredictor.simple_outline_report()'s (frames, counts), with tolerance = the tolerance in pixels they were made with:
    the rings are the SIMPLIFIED ones (each ring on its own: neighbouring regions' rings may cross or leave slivers), every feature
    gains the properties tolerance, vertices_full (the vertices its rings had before) and area2_simplified (twice the simplified
    polygon's area, holes taken off; `area` stays the pixel count), and the frames in which some ring hit the round cap -- it kept all
    vertices of the segments still open -- are named in the top-level list "unconverged_frames".  None: the file without any of it,
    byte for byte."""
    import json

    frames, flags = outlines
    if len(frame_ids) != len(rows) or len(frames) != len(rows) or len(flags) != len(rows):
        raise ValueError(f"write_outlines_geojson: one frame id and one outline per frame, got {len(frame_ids)} ids, {len(frames)} outlines "
                         f"for {len(rows)} frames")
    if tracks is not None and (len(tracks) != len(rows) or any(len(t) != len(r) for t, r in zip(tracks, rows))):
        raise ValueError("write_outlines_geojson: tracks must hold one row per region of every frame")
    if simplified is not None:
        if tolerance is None:
            raise ValueError("write_outlines_geojson: simplified rings need the tolerance they were made with")
        if len(simplified[0]) != len(rows) or len(simplified[1]) != len(rows):
            raise ValueError(f"write_outlines_geojson: one simplified outline per frame, got {len(simplified[0])} for {len(rows)} frames")
    features, overflowed, truncated, unconverged = [], [], [], []
    for f, (fid, table, (contours, vertices, shape)) in enumerate(zip(frame_ids, rows, frames)):
        if int(flags[f]) & 1:
            overflowed.append(fid)
            continue
        if int(flags[f]) & 2:
            truncated.append(fid)
        outer, holes, full, simple_area2 = {}, {}, {}, {}
        if simplified is not None:
            simple_rows, simple_vertices = simplified[0][f]
            if len(simple_rows) != len(contours) or int(simplified[1][f][3]) & 10:
                raise ValueError(f"write_outlines_geojson: frame {fid} has {len(contours)} contour rows but {len(simple_rows)} simplified ones "
                                 f"(flags {int(simplified[1][f][3])})")
            if int(simplified[1][f][3]) & 1:
                unconverged.append(fid)
            simple_rows = np.asarray(simple_rows).tolist()
        for k, (region, first, count, _, area2, _) in enumerate(np.asarray(contours).tolist()):
            if simplified is None:
                ring = np.asarray(vertices[first:first + count]).tolist()
            else:
                ring = np.asarray(simple_vertices[simple_rows[k][0]:simple_rows[k][0] + simple_rows[k][1]]).tolist()
                full[region] = full.get(region, 0) + count
                simple_area2[region] = simple_area2.get(region, 0) + simple_rows[k][2]
            ring.append(ring[0])
            if area2 > 0:
                outer[region] = ring
            else:
                holes.setdefault(region, []).append(ring)
        for r, row in enumerate(np.asarray(table).tolist()):
            if r not in outer:
                continue
            perimeter, count, _ = np.asarray(shape[r]).tolist()
            props = {"frame": fid, "region": r, "class": row[0], "area": row[1], "perimeter": perimeter, "holes": count - 1}
            if tracks is not None:
                props["track"], props["parent"] = np.asarray(tracks[f][r]).tolist()[:2]
            if simplified is not None:
                props["tolerance"], props["vertices_full"], props["area2_simplified"] = float(tolerance), full[r], simple_area2[r]
            features.append({"type": "Feature", "properties": props,
                             "geometry": {"type": "Polygon", "coordinates": [outer[r]] + holes.get(r, [])}})
    with open(path, "w") as fh:
        doc = {"type": "FeatureCollection", "overflowed_frames": overflowed, "truncated_frames": truncated}
        if simplified is not None:
            doc["unconverged_frames"] = unconverged
        doc["features"] = features
        json.dump(doc, fh)
        fh.write("\n")


def write_tracks_csv(path, frame_ids, rows, tracks, proximity=None):
    """The growth summary: one CSV row per track, in id order, from region_report()'s rows and track_report()'s tracks: track id, class,
    parent track (-1: none), the first and the last frame it was seen in, the number of frames, its area in the first and in the last of
    them, its largest area and the (first) frame of that.  proximity = per frame the near rows of FlowPredictor.proximity_report(): the
    columns first_dist, last_dist and min_dist are appended -- the track's distance to the nearest source pixel (mask pixels) in the
    first and the last frame it was seen in and the smallest over its frames, each empty where no source was within reach; None: the
    file without them, byte for byte."""
    if proximity is not None and (len(proximity) != len(rows) or any(len(t) != len(r) for t, r in zip(proximity, rows))):
        raise ValueError("write_tracks_csv: proximity must hold one row per region of every frame")
    if len(frame_ids) != len(rows) or len(tracks) != len(rows) or any(len(t) != len(r) for t, r in zip(tracks, rows)):
        raise ValueError(f"write_tracks_csv: one frame id and one tracks row per region of every frame, got {len(frame_ids)} ids, {len(rows)} and "
                         f"{len(tracks)} frames")
    seen = {}  # id -> [class, parent, first frame, last frame, frames, first area, last area, max area, frame of the max]
    for fid, frame, links in zip(frame_ids, rows, tracks):
        for region, link in zip(np.asarray(frame).tolist(), np.asarray(links).tolist()):
            tid, area = link[0], region[1]
            t = seen.setdefault(tid, [region[0], link[1], fid, fid, 0, area, area, area, fid])
            t[3], t[4], t[6] = fid, t[4] + 1, area
            if area > t[7]:
                t[7], t[8] = area, fid
    dist = {}  # id -> [first, last, min] of min_d2 over the track's frames (-1: none within reach)
    if proximity is not None:
        for links, near in zip(tracks, proximity):
            for link, row in zip(np.asarray(links).tolist(), np.asarray(near).tolist()):
                d = dist.setdefault(link[0], [row[0], row[0], row[0]])
                d[1] = row[0]
                if row[0] >= 0 and (d[2] < 0 or row[0] < d[2]):
                    d[2] = row[0]
    with open(path, "w") as fh:
        fh.write("track,class,parent,first_frame,last_frame,frames,first_area,last_area,max_area,max_frame"
                 + (",first_dist,last_dist,min_dist" if proximity is not None else "") + "\n")
        for tid in sorted(seen):
            fh.write(",".join([str(v) for v in [tid] + seen[tid]] + ([_distance_cell(v) for v in dist[tid]] if proximity is not None else [])) + "\n")


def colorize(masks_u8, palette=PALETTE):
    """colors[output] (flow/base.py:308-312): uint8 [..., 3] RGB frames for the video writer / PNG dump."""
    lib = _lib.load()
    m = masks_u8.contiguous()
    pal = torch.as_tensor(palette, dtype=torch.uint8, device=m.device).contiguous()
    out = torch.empty(tuple(m.shape) + (3,), dtype=torch.uint8, device=m.device)
    if m.numel() == 0:
        return out
    check(lib.fs_colorize(ptr(m), ptr(pal), pal.shape[0], ptr(out), m.numel(), stream_ptr()))
    return out


REGION_STYLE_KEYS = ("fill_palette", "outline", "outline_width", "label_scale", "label_min_area", "halo", "ink")  # ops.compose_regions' drawing options


def compose_window(masks_u8, item_or_sources=None, palette=PALETTE, alpha=None, out_fmt="nv12", out_matrix="bt709", out_full_range=False,
                   dataset=None, regions=None, style=None):
    """The result video frames of one window, composed on the device (ops.compose_frame, one launch per frame): yields, for
    masks_u8 [n,h,w], n flat uint8 buffers of ops.raw_frame_bytes(h, w, out_fmt) bytes each -- what RawVideoWriter.write takes, and
    what ops.frame_planes splits into the planes ops.prepare_frame reads.
    item_or_sources: None -- the class colours alone (the reference's video, flow/base.py:308-312); a sequence of n entries, or a
    callable p -> entry, each a (frame, chroma, fmt, matrix, full_range) tuple as PredictWindows.source / RawVideoWindows.source
    return it (None: no overlay for that frame) -- the colours blended over the footage; or a window item together with
    `dataset=`, which stands for dataset.source(item["frame_id"] + p).  Sources are asked for one frame at a time, so the decoded
    frames of a window need not be alive together.  palette / alpha: as ops.compose_frame ([K,3] + alpha, or [K,4]).
    regions: FlowPredictor.window_regions()'s list, one (index, table, counts, tracks) entry per mask (None: that frame without
    layers) -- the frames are then composed by ops.compose_regions with the drawing options of `style`, a dict with keys among
    REGION_STYLE_KEYS (fill_palette, outline, outline_width, label_scale, label_min_area, halo, ink).  regions=None: ops.compose_frame."""
    if style is not None and regions is None:
        raise RuntimeError("floodseg.compose_window: style= goes with regions= (the layers are drawn from the regions)")
    if regions is not None:
        style = dict(style or {})
        unknown = sorted(set(style) - set(REGION_STYLE_KEYS))
        if unknown:
            raise RuntimeError(f"floodseg.compose_window: unknown style keys {unknown}; the drawing options are {list(REGION_STYLE_KEYS)}")
        if len(regions) != masks_u8.shape[0]:
            raise RuntimeError(f"floodseg.compose_window: {len(regions)} region entries for {masks_u8.shape[0]} masks")
    if isinstance(item_or_sources, dict):
        if dataset is None:
            raise RuntimeError("floodseg.compose_window: a window item needs dataset= to find its decoded frames")
        first = item_or_sources["frame_id"]
        source = lambda p: dataset.source(first + p)  # noqa: E731
    elif item_or_sources is None:
        source = lambda p: None  # noqa: E731
    elif callable(item_or_sources):
        source = item_or_sources
    else:
        if len(item_or_sources) != masks_u8.shape[0]:
            raise RuntimeError(f"floodseg.compose_window: {len(item_or_sources)} sources for {masks_u8.shape[0]} masks")
        source = item_or_sources.__getitem__
    if masks_u8.dim() != 3:
        raise RuntimeError(f"floodseg.compose_window: masks must be [n,h,w], got {tuple(masks_u8.shape)}")
    for p in range(masks_u8.shape[0]):
        src = source(p)
        out = torch.empty(ops.raw_frame_bytes(masks_u8.shape[1], masks_u8.shape[2], out_fmt), dtype=torch.uint8, device=masks_u8.device)
        if regions is not None and regions[p] is not None:
            index, table, counts, tracks = regions[p]
            if src is None:
                ops.compose_regions(masks_u8[p], palette, index, table, counts, tracks, out_fmt=out_fmt, out_matrix=out_matrix,
                                    out_full_range=out_full_range, out=out, **style)
            else:
                frame, chroma, fmt, matrix, full_range = src
                ops.compose_regions(masks_u8[p], palette, index, table, counts, tracks, background=frame, chroma=chroma, fmt=fmt, matrix=matrix,
                                    full_range=full_range, out_fmt=out_fmt, out_matrix=out_matrix, out_full_range=out_full_range, out=out, alpha=alpha,
                                    **style)
        elif src is None:
            ops.compose_frame(masks_u8[p], palette, out_fmt=out_fmt, out_matrix=out_matrix, out_full_range=out_full_range, out=out)
        else:
            frame, chroma, fmt, matrix, full_range = src
            ops.compose_frame(masks_u8[p], palette, frame, chroma, fmt, matrix, full_range, out_fmt, out_matrix, out_full_range, out=out, alpha=alpha)
        yield out
