#!/usr/bin/env python3
"""Stand-alone counterpart of the reference's `predict_flow.sh` run (Lightning `predict` of FlowBaseModel,
flow/base.py:236-343) on the HIP path: walks the key-frame windows of one video, segments the key frames, interpolates the
frames in between and writes the colourised masks.

    python tools/predict_video.py --data-root dataset/flow --video-id florida-01 --frame-delta 5 \\
        --arch pspnet --layers 50 --ckpt logs/<run>/last.ckpt --out out/florida-01

    python tools/predict_video.py --raw clip.nv12 --raw-size 1080 1920 --pix-fmt nv12 --matrix bt709 --arch pspnet --ckpt ... --out out/clip

    python tools/predict_video.py --raw clip.nv12 --raw-size 1080 1920 --arch pspnet --ckpt ... --raw-out result.nv12 --overlay 128

`--raw-out FILE|-` writes the result VIDEO as raw frames (`--out-pix-fmt nv12|i420|rgb24`), composed on the device in one launch per
frame (ops.compose_frame) and copied out through pinned buffers; the ffmpeg line that encodes it is printed on stderr.  `--overlay A`
blends the class colours with opacity A (0..255) over the footage the network saw; omitted = opaque colours, the reference's video.
Under torchrun every rank writes its own window block into the one file (not into a pipe).
`--grids estimate` (with `--search`, `--penalty`) takes the grids from block matching of the decoded frames instead of the grids/
folders; a raw video file (`--raw`, as `ffmpeg -f rawvideo -pix_fmt nv12|yuv420p|rgb24` writes it) always does.  `--intra-bias N`
and `--scene-cut F` (both off by default, no value validated on real video) leave blocks the matcher cannot explain, and whole frames
across a scene cut, on the identity grid; the frames judged cuts and the mean intra share are printed after the run.  `--hold-cuts`
(needs `--scene-cut`; segmentation mode and `--feature-based` alike) also makes the blend react: in a window with a cut, a frame before
the cut is the previous key frame's prediction alone and a frame after it the next key frame's, instead of a mix of two scenes (in
feature mode: the decoder sees one key frame's warped features, not a mixture); how many frames were blended and held is printed with
the rest.
`--confidence` (an extension) also computes a per-pixel confidence, 255 x the probability of the emitted class, and a
per-frame, per-class extent report on the device; the masks are unchanged.  `--report FILE.csv` writes, once at the end, one row per
frame: the frame id and per class the area fraction, the mean confidence (sum / (255 pixels)) and the share of the class's pixels
with confidence below `--low-confidence` (default 128); without `--confidence` the areas only.  `--conf-out FILE` (needs
`--confidence`) writes the confidence planes as a headerless 8-bit grey raw video (`ffmpeg -f rawvideo -pix_fmt gray` reads it).

`--regions FILE.csv` (an extension) labels the connected regions of every emitted mask on the device (`--connectivity` 4
or 8, at most `--max-regions` rows per frame) and writes, once at the end, one row per frame and region: frame, class, area, bounding
box, centroid and, with `--confidence`, the mean confidence and the low-confidence share.  A frame with more regions than
`--max-regions` gets a warning and its first rows.  `--min-region N` removes regions smaller than N pixels from the emitted masks (each
takes the class most of its 4-neighbours have); every output -- masks, overlays, reports, metrics -- then shows the filtered masks.
The filter works on the first `--max-regions` regions of a frame (in raster order); a frame with more gets a warning after the run.
`--tracks FILE.csv` (an extension; needs `--regions`) follows the regions from frame to frame on the device: a region that
shares at least `--min-overlap` pixels with its best predecessor of the same class (compared in place), and is that one's best
successor, keeps its track id; every other region starts a new track with its best predecessor's track as parent.  The regions CSV gets
the columns track, parent and overlap, and FILE.csv one row per track: class, parent, first and last frame, frames seen, first / last /
largest area and the frame of the largest -- the growth summary.  `--max-pairs` sizes the table of overlapping pairs of a frame pair (a
power of two); a frame whose table overflowed gets a warning and all its regions start new tracks.  `--compensate` (needs `--tracks`
and estimated grids: `--raw`, or `--grids estimate`) compares each frame with the frame before it read at the source of every pixel
under the block matcher's vectors, so that a region which moves further than its own width per frame keeps its track; with
`--scene-cut` the frames that follow a cut are listed and their regions all start new tracks.  Single process only: ids are per
predictor.
`--outlines FILE.geojson` (an extension; needs `--regions`) outlines every region on the device and writes, once at the
end, one GeoJSON Polygon feature per frame and region -- the outer contour first, then the holes, closed rings in mask pixel lattice
coordinates -- with frame, region, class, area, perimeter and holes (and track, parent with `--tracks`); the regions CSV gets the columns
perimeter and holes.  A frame with more than `--max-vertices` outline vertices gets no outlines at all, one with more than
`--max-contours` contours keeps the first ones; both get a warning.  The defaults are guesses, not validated on real video.
`--simplify PX` (an extension; needs `--outlines`) simplifies every ring on the device before it is written: every dropped
vertex lies within PX pixels of the ring that is written, and every feature gains tolerance, vertices_full and area2_simplified.
`--simplify-rounds N` (1..256, default 32) caps the rounds: a frame in which some ring still had open segments after N rounds gets a
warning (those segments keep all their vertices), and the largest number of rounds a frame needed is printed at the end -- the figure
to set N by.  The default is a guess for natural shorelines, not validated on real video.
`--draw-outlines [W]`, `--draw-tracks`, `--draw-ids [SCALE]` (an extension; all need `--raw-out` and `--regions`) draw the
regions into the result video on the device (ops.compose_regions instead of ops.compose_frame): a white line W pixels wide (0..4,
default 1) along the inside of every region's boundary (none for class 0 under `--overlay-keep-class0`); with `--tracks`, every region
filled in a colour picked by its track id (ops.TRACK_PALETTE, with the class's opacity under `--overlay`) and / or labelled with its
track id (mod 10^7) in a 5 x 7 font scaled by SCALE (1..4, default 2) at its centroid -- the number in the track column of the regions
CSV and in the GeoJSON features.  `--label-min-area N` (default 256) leaves regions below N pixels without a label.  Colours, widths and
the area bound are guesses, not validated on real video.  The PNG route (`--out`) is unchanged.
`--stabilize N` (an extension; 2..255, 0 or 1: off) debounces every pixel's class along the time axis on the device before
anything else sees the masks: a pixel keeps its emitted class until another class has been observed N frames running, so a change that
lasts shows N - 1 frames late and a shorter flicker never does; every output -- masks, overlays, reports, regions, tracks, metrics --
then shows the stabilised masks, and the totals of held, switched and seeded pixels are printed after the temporal-consistency line.
`--stabilize-trust T` (0..256, needs `--confidence`) emits an observation whose confidence code is at least T at once.
`--stabilize-compensate` (needs estimated grids: `--raw`, or `--grids estimate`) reads the state at the source of every pixel under the
block matcher's vectors, and a frame that follows a `--scene-cut` starts afresh; without it a moving scene is compared in place, where
the filter lags and can make the masks worse.  Under torchrun every rank's block of windows starts unseeded.  No default is validated
on real video.
`--proximity PX [PX ...]` (an extension; needs `--regions`; 1..8 ascending distances in mask pixels) measures, on the device,
the exact distance of every pixel to the nearest pixel of the classes `--proximity-sources` (default 1, water) and tabulates it: the
regions CSV gains `dist` (the region's smallest distance, empty: none within reach), `near_px` (its pixels within the first PX) and
`nearest_region` (and `nearest_track` with `--tracks`), the tracks CSV `first_dist`, `last_dist` and `min_dist`, and `--exposure FILE.csv`
gets one row per frame: per class of `--proximity-targets` (default 3 4) the pixels within each PX.  `--proximity-max R` bounds the search
to R >= the largest PX pixels (regions further away then have an empty `dist`); unbounded, the default, costs a scan of up to the
frame's width per pixel where water is a single speck.  Distances
are mask pixels of a moving, un-georeferenced camera -- no metres follow from them -- and the thresholds are guesses, not validated on
real video.
`--mosaic FILE.png` (an extension; needs estimated grids: `--raw`, or `--grids estimate`.  Under torchrun, with `--ortho`,
every rank mosaics its own block of windows and writes `FILE.partNNN.npz`; rank 0 then registers the parts against each other in rank
order, merges them and writes the outputs, DESIGN §3.23 -- `--mosaic-report` lists rank 0's frames and `FILE.merge.csv` beside it one row
per merged part.  `--mosaic-part FILE.npz`, with `--ortho`, saves the (merged) mosaic for `tools/merge_mosaics.py`) registers every
frame's mask to the first frame through the camera's motion -- one robust affine per frame pair, fitted on the device to the block
matcher's vectors, without the blocks that lie on the classes of `--mosaic-exclude` (default 1, water) -- and accumulates the masks
into one extent map of `--mosaic-size H W` pixels (default: twice the output size), in which each piece of ground is counted once.  The
PNG shows, in the palette's colours, the class most frames saw at each pixel, black where no frame looked.  `--mosaic-rounds N` (0..8,
default 4) and `--mosaic-tol PX` (default 1.0 frame pixels) steer the fit.  `--mosaic-report FILE.csv` lists per frame the pose, its
status (ok, bridged, lost), whether the frame left the canvas, and the fit's inliers and usable blocks, then per class the canvas
pixels and their share of the ground seen.  A scene cut ends the chain: the frames after it are reported as lost.  The defaults are
guesses, not validated on real video; an affine per pair is not a homography, the chain drifts over a long flight and nothing closes
loops; areas are pixels of the first frame, not metres.
`--ortho FILE.png` (an extension; needs `--mosaic`, and so estimated grids) gathers, with the same poses, the
frames' pixels -- the image the network saw, at the mask's resolution -- into an orthophoto of the mosaic's size and writes it with the extent
map blended over it at `--ortho-alpha A` (default 96 of 255); `--ortho-edge K [K ...]` draws a one-pixel line along the inside of those
classes' boundaries, `--ortho-plain` leaves the extent map off.  `--ortho-mode centre` (default) gives each piece of ground to the view that
saw it nearest its optical axis, `latest` to the newest view.  No feathering or exposure matching across seams and no lens model: the
chain's drift shows as broken roads at the seams, which is what the picture is for.  Not validated on real video.
`--mosaic-refine` (an extension; needs `--ortho`) registers every frame against the orthophoto gathered so far before it
votes: the map is drawn as the frame should see it under its predicted pose, the block matcher finds the residual shift within
`--refine-search R` mask pixels (default 8), the camera-motion fit of `--mosaic` turns it into an affine, and the pose chain is corrected.
`--refine-min-age N` matches only against ground owned by a frame at least N frames older (loop closure on a revisit only),
`--refine-every N` registers every N-th frame, `--refine-intra-bias B` lets the matcher drop blocks the map does not explain.
`--mosaic-report` then also lists the correction per frame.  Earlier frames are never re-posed and drift beyond the search radius is not
recovered; the defaults are guesses, not validated on real video.
`--mosaic-relocate` (an extension; needs `--mosaic-refine`) relocalises a lost chain -- a scene cut, a run of failed fits
over open water -- against the orthophoto: the frame is drawn with the last pose the chain held, reduced to `--relocate-scale S` (4, 8
or 16, default 8) pixel cells and slid over the whole reduced canvas; a placement with a mean difference of at most `--relocate-max-mean`
that beats the best placement elsewhere by `--relocate-ratio`, on at least `--relocate-min-overlap` of its cells, goes through the fine
registration above and, only if that succeeds, the chain resumes on the same mosaic.  `--relocate-every N` tries every N-th frame,
`--relocate-report FILE.csv` lists the outcome per frame.  Translation only; flat water and repetitive ground are rejected, not placed;
ground voted before the break is never re-posed; the defaults are guesses, not validated on real video.
Directory layout read (flow/dataset.py:222-240): <data-root>/frames/<video-id>/{images/<i>.jpg, grids/<i>.npy, inv_grids/<i>.npy}.
Checkpoints are loaded with `torch.load(..., weights_only=True)` (a Lightning `state_dict` with the `model_G.model.` prefix, or
a bare state_dict); `--synthetic-weights` uses the seeded random weights of the test-suite instead (no checkpoint ships with
the reference).  Multi-GPU: launch with torchrun; each rank takes a contiguous block of windows, the one temporal-consistency
pair across each block boundary is scored from the neighbour's last mask (one all_gather at the end), metrics are reduced.
Consecutive windows share a key frame: it is segmented once (`--no-keyframe-cache` recomputes it, as the reference does).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flood_uav_video_segmentation_amd import ops, shard, synth  # noqa: E402
from flood_uav_video_segmentation_amd.flow.dataset import PredictWindows, RawVideoWindows, RawVideoWriter  # noqa: E402
from flood_uav_video_segmentation_amd.flow.model import FlowModel  # noqa: E402
from flood_uav_video_segmentation_amd.flow.predict import PALETTE, FlowPredictor, colorize, compose_window, write_exposure_csv, write_extent_csv, write_guide_csv, read_mosaic_part, write_merge_csv, write_mosaic_csv, write_mosaic_part, write_relocate_csv, write_outlines_geojson, write_regions_csv, write_tracks_csv  # noqa: E402
from flood_uav_video_segmentation_amd.model.deeplabv3 import FlowDeepLabv3  # noqa: E402
from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet  # noqa: E402


def load_weights(net, args):
    if args.synthetic_weights:
        make = synth.make_pspnet_state if args.arch == "pspnet" else synth.make_deeplab_state
        net.load_state_dict(make(args.layers, args.classes, seed=0))
        return
    ckpt = torch.load(args.ckpt, map_location="cpu", weights_only=True)
    state = ckpt.get("state_dict", ckpt)
    for prefix in ("model_G.model.", "model.model.", "model."):
        sub = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
        if sub:
            state = sub
            break
    net.load_state_dict(state)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data-root", help="folder input: <data-root>/frames/<video-id>/...")
    ap.add_argument("--video-id", default="florida-01")                      # data.predict_v_id
    ap.add_argument("--frame-delta", type=int, default=5)                    # data.frame_delta
    ap.add_argument("--arch", choices=("pspnet", "deeplabv3"), default="pspnet")
    ap.add_argument("--layers", type=int, default=50)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--ckpt")
    ap.add_argument("--synthetic-weights", action="store_true")
    ap.add_argument("--feature-based", action="store_true")                  # model.feature_based
    ap.add_argument("--no-warp", action="store_true")                        # model.no_warp
    ap.add_argument("--no-cropping", action="store_true")                    # model.no_cropping: whole frame instead of sliding crops
    ap.add_argument("--crop", type=int, nargs=2, default=(713, 713), metavar=("H", "W"))   # model.test_h / test_w
    ap.add_argument("--size", type=int, nargs=2, default=(1072, 1920), metavar=("H", "W"))  # transform_predict Resize, and the output size
    ap.add_argument("--palette", help="colors.txt (dataset/flow/list/colors.txt); default: the 5-class flood palette")
    ap.add_argument("--out", help="directory for <frame>.png (model.save_images); omit to only time and score")
    ap.add_argument("--no-metrics", action="store_true")                     # model.compute_metrics False
    ap.add_argument("--no-keyframe-cache", action="store_true", help="segment both key frames of every window (reference behaviour)")
    ap.add_argument("--grids", choices=("files", "estimate"), help="grids/ and inv_grids/ folders (default for a frame folder), or block "
                    "matching of the decoded frames (flow/motion.py; the only source for --raw)")
    ap.add_argument("--search", type=int, default=16, help="--grids estimate: search range in pixels, 1..32")
    ap.add_argument("--penalty", type=int, default=0, help="--grids estimate: cost per pixel of displacement, 0..255")
    ap.add_argument("--intra-bias", type=int, metavar="N", help="--grids estimate: 0..65535; a block whose best match is worse than its own "
                    "deviation from its mean + N gets no vector (identity grid cells).  Default: off; the right N depends on the sensor's noise")
    ap.add_argument("--scene-cut", type=float, metavar="F", help="--grids estimate: 0..1; a frame with more than this fraction of such blocks "
                    "gets the default grid (a scene cut).  Default: off.  Counts the blocks --intra-bias marks: without --intra-bias it never fires")
    ap.add_argument("--guide", action="store_true", help="--grids estimate: guide the matcher's tables with the camera motion fitted to them "
                    "(ops.guide_vectors; DESIGN 3.21): blocks without a vector take the camera's.  Default: off")
    ap.add_argument("--guide-outlier", type=float, metavar="PX", help="--guide: also replace vectors further than PX pixels (0..64) from the camera's")
    ap.add_argument("--guide-bias", type=int, metavar="N", help="--guide-outlier: replace only where the camera's window explains the block no worse "
                    "than the winner did, up to N (0..65535); default: replace as it stands")
    ap.add_argument("--guide-report", metavar="FILE.csv", help="--guide: per frame pair the counts of void, filled, outlier, replaced, dropped and kept rows")
    ap.add_argument("--hold-cuts", action="store_true", help="--scene-cut: across a detected cut hold one key frame's prediction on each side "
                    "instead of blending the two scenes, logits or (--feature-based) encoder features (one more block search per window)")
    ap.add_argument("--raw", metavar="FILE", help="raw video input (ffmpeg -f rawvideo) instead of --data-root / --video-id")
    ap.add_argument("--raw-size", type=int, nargs=2, metavar=("H", "W"), help="--raw: frame height and width")
    ap.add_argument("--pix-fmt", choices=("nv12", "i420", "rgb24"), default="nv12", help="--raw: pixel format (i420 = ffmpeg's yuv420p)")
    ap.add_argument("--matrix", choices=("bt601", "bt709"), default="bt709", help="--raw, YUV formats: conversion matrix")
    ap.add_argument("--full-range", action="store_true", help="--raw, YUV formats: full-range (JPEG) levels instead of limited")
    ap.add_argument("--raw-out", metavar="FILE", help="write the result video as raw frames to FILE ('-' = standard output)")
    ap.add_argument("--out-pix-fmt", choices=("nv12", "i420", "rgb24"), default="nv12", help="--raw-out: pixel format (i420 = ffmpeg's yuv420p)")
    ap.add_argument("--overlay", type=int, metavar="A", help="--raw-out: blend the colours with opacity A (0..255) over the footage; "
                    "omitted = opaque colours (the reference's video)")
    ap.add_argument("--overlay-keep-class0", action="store_true", help="--overlay: class 0 gets opacity 0 (background stays plain footage)")
    ap.add_argument("--out-matrix", choices=("bt601", "bt709"), help="--raw-out, YUV formats: conversion matrix (default: the input's for "
                    "--raw, bt709 for a frame folder)")
    ap.add_argument("--out-full-range", action="store_true", default=None, help="--raw-out, YUV formats: full-range levels (default: the "
                    "input's for --raw, limited for a frame folder)")
    ap.add_argument("--confidence", action="store_true", help="also compute a per-pixel confidence (255 x the probability of the emitted "
                    "class) and a per-frame, per-class extent report on the device; the masks are unchanged")
    ap.add_argument("--low-confidence", type=int, default=128, metavar="C", help="--confidence: a pixel with a confidence code below C "
                    "(0..255) counts as low-confidence in the report")
    ap.add_argument("--report", metavar="FILE.csv", help="write one row per frame: per class the area fraction and, with --confidence, the "
                    "mean confidence and the low-confidence share (single GPU)")
    ap.add_argument("--conf-out", metavar="FILE", help="--confidence: write the confidence planes as 8-bit grey raw video (-pix_fmt gray)")
    ap.add_argument("--regions", metavar="FILE.csv", help="label the connected regions of every mask on the device and write one row per frame "
                    "and region: class, area, box, centroid and, with --confidence, mean confidence and low-confidence share (single GPU)")
    ap.add_argument("--min-region", type=int, default=0, metavar="N", help="remove regions smaller than N pixels from the emitted masks (each takes "
                    "the class most of its 4-neighbours have); 0 or 1: off.  Only the first --max-regions regions of a frame are filtered: a "
                    "frame with more gets a warning after the run")
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8], help="--regions / --min-region: 4 = edge neighbours, 8 = corners too")
    ap.add_argument("--max-regions", type=int, default=1024, metavar="N", help="--regions / --min-region: rows per frame (1..65536)")
    ap.add_argument("--tracks", metavar="FILE.csv", help="--regions: follow the regions from frame to frame on the device; the regions CSV gets "
                    "the columns track, parent and overlap, and FILE.csv one row per track (class, parent, first / last frame, frames, first / "
                    "last / largest area): the growth summary (single process)")
    ap.add_argument("--min-overlap", type=int, default=1, metavar="N", help="--tracks: a region continues its predecessor only if they share at "
                    "least N pixels")
    ap.add_argument("--max-pairs", type=int, default=None, metavar="N", help="--tracks: slots of the table of overlapping region pairs of two "
                    "consecutive frames, a power of two in 16..1048576 (default: the next one >= 4 x --max-regions)")
    ap.add_argument("--outlines", metavar="FILE.geojson", help="--regions: outline every region on the device and write one GeoJSON polygon "
                    "(outer contour and holes, mask pixel coordinates) per frame and region; the regions CSV gets the columns perimeter and "
                    "holes")
    ap.add_argument("--max-contours", type=int, default=4096, metavar="N", help="--outlines: contour rows per frame (1..1048576)")
    ap.add_argument("--max-vertices", type=int, default=32768, metavar="N", help="--outlines: polygon vertices per frame (4..4194304); a frame "
                    "with more gets no outlines at all")
    ap.add_argument("--simplify", type=float, default=None, metavar="PX", help="--outlines: simplify every ring on the device (Douglas-Peucker), "
                    "every dropped vertex within PX pixels (0..256) of the ring that is written")
    ap.add_argument("--simplify-rounds", type=int, default=32, metavar="N", help="--simplify: the round cap (1..256); rings that need more keep "
                    "all vertices of the segments still open and get a warning.  The default is a guess, not validated on real video")
    ap.add_argument("--compensate", action="store_true", help="--tracks with estimated grids: compare each frame with the frame before it read at "
                    "the source of every pixel under the block matcher's vectors, so that a small region that moves fast keeps its track")
    ap.add_argument("--stabilize", type=int, default=0, metavar="N", help="debounce every pixel's class along the time axis: a class is emitted once "
                    "it has been observed N frames running (2..255; 0 or 1: off).  Not validated on real video")
    ap.add_argument("--stabilize-trust", type=int, default=None, metavar="T", help="--stabilize with --confidence: an observation with a confidence "
                    "code >= T (0..256) is emitted at once")
    ap.add_argument("--stabilize-compensate", action="store_true", help="--stabilize with estimated grids: read the state at the source of every pixel "
                    "under the block matcher's vectors")
    ap.add_argument("--proximity", type=int, nargs="+", default=None, metavar="PX", help="--regions: measure every pixel's exact distance to the nearest "
                    "source pixel on the device and tabulate it per region and class at these 1..8 ascending distances (mask pixels; guesses, not "
                    "validated on real video)")
    ap.add_argument("--proximity-sources", type=int, nargs="+", default=[1], metavar="CLASS", help="--proximity: the classes distances are measured to "
                    "(default 1, water)")
    ap.add_argument("--proximity-targets", type=int, nargs="+", default=[3, 4], metavar="CLASS", help="--proximity: the classes --exposure counts "
                    "(default 3 4, buildings and streets)")
    ap.add_argument("--proximity-max", type=int, default=None, metavar="R", help="--proximity: search no further than R pixels, R at least the largest "
                    "PX (default: unbounded)")
    ap.add_argument("--exposure", default=None, metavar="FILE.csv", help="--proximity: one row per frame, per target class the pixels within each PX")
    ap.add_argument("--mosaic", default=None, metavar="FILE.png", help="register every frame's mask to the first frame through the camera's motion "
                    "(estimated grids only) and write the accumulated extent map, each piece of ground counted once.  Not validated on real video")
    ap.add_argument("--mosaic-size", type=int, nargs=2, default=None, metavar=("H", "W"), help="--mosaic: the canvas (default: twice --size)")
    ap.add_argument("--mosaic-exclude", type=int, nargs="*", default=[1], metavar="K", help="--mosaic: blocks on these classes do not vote on the "
                    "camera's motion (default 1, water)")
    ap.add_argument("--mosaic-rounds", type=int, default=4, metavar="N", help="--mosaic: least-squares rounds of the motion fit (0..8; 0: the vectors' mode)")
    ap.add_argument("--mosaic-tol", type=float, default=1.0, metavar="PX", help="--mosaic: inlier tolerance of the last round in frame pixels (0..64)")
    ap.add_argument("--ortho", default=None, metavar="FILE.png", help="--mosaic: also gather the frames' pixels into an orthophoto of the mosaic's size and "
                    "write it with the extent map drawn over it (DESIGN §3.19)")
    ap.add_argument("--ortho-mode", choices=("centre", "latest"), default=None, help="--ortho: which view owns a piece of ground: the one that saw it nearest "
                    "its optical axis (default), or the newest")
    ap.add_argument("--ortho-alpha", type=int, default=None, metavar="A", help="--ortho: opacity of the class colours over the imagery (0..255, default 96)")
    ap.add_argument("--ortho-edge", type=int, nargs="+", default=None, metavar="K", help="--ortho: classes that get a one-pixel opaque line along the inside "
                    "of their boundary (default: none)")
    ap.add_argument("--ortho-plain", action="store_true", help="--ortho: the imagery alone, without the extent map")
    ap.add_argument("--mosaic-refine", action="store_true", help="--ortho: register every frame against the orthophoto so far and correct its pose before it "
                    "votes (DESIGN 3.20; the defaults are guesses, not validated on real video)")
    ap.add_argument("--refine-search", type=int, default=None, metavar="R", help="--mosaic-refine: the matcher's search radius against the map in mask pixels "
                    "(1..32, default 8); drift beyond it is not recovered")
    ap.add_argument("--refine-min-age", type=int, default=None, metavar="N", help="--mosaic-refine: match only against ground owned by a frame at least N "
                    "frames older (default 0: any mapped ground; N > 0: loop closure on a revisit only)")
    ap.add_argument("--refine-every", type=int, default=None, metavar="N", help="--mosaic-refine: register every N-th frame (default 1)")
    ap.add_argument("--refine-intra-bias", type=int, default=None, metavar="B", help="--mosaic-refine: the matcher's intra bias against the map (0..65535, "
                    "default 65535: no block is intra)")
    ap.add_argument("--mosaic-relocate", action="store_true", help="--mosaic-refine: relocalise a lost pose chain against the orthophoto and resume the mosaic "
                    "(DESIGN 3.22)")
    ap.add_argument("--relocate-scale", type=int, default=None, metavar="S", help="--mosaic-relocate: the coarse cell edge in canvas pixels, 4, 8 or 16 (default 8)")
    ap.add_argument("--relocate-every", type=int, default=None, metavar="N", help="--mosaic-relocate: try every N-th frame (default 1)")
    ap.add_argument("--relocate-min-overlap", type=float, default=None, metavar="F", help="--mosaic-relocate: the share of the frame's cells that must lie on "
                    "mapped ground, 0.001..1 (default 0.5)")
    ap.add_argument("--relocate-max-mean", type=int, default=None, metavar="M", help="--mosaic-relocate: the largest mean luma difference of an accepted "
                    "placement, 0..255 (default 16)")
    ap.add_argument("--relocate-ratio", type=float, default=None, metavar="F", help="--mosaic-relocate: the best placement's mean must be at most F times the "
                    "runner-up's, 0.001..1 (default 0.8)")
    ap.add_argument("--relocate-report", default=None, metavar="FILE.csv", help="--mosaic-relocate: the outcome of the relocation per frame as CSV")
    ap.add_argument("--mosaic-part", default=None, metavar="FILE.npz", help="--mosaic --ortho: also save the mosaic (votes, orthophoto, pose rows, seen box) as one "
                    "file that tools/merge_mosaics.py merges with other runs' (DESIGN 3.23)")
    ap.add_argument("--mosaic-report", default=None, metavar="FILE.csv", help="--mosaic: per frame the pose, status, clipped flag, inliers and usable "
                    "blocks; per class the canvas pixels and their share of the ground seen")
    ap.add_argument("--draw-outlines", type=int, nargs="?", const=1, default=None, metavar="W", help="--raw-out with --regions: draw a white line W "
                    "pixels wide (0..4, default 1) along the inside of every region's boundary")
    ap.add_argument("--draw-tracks", action="store_true", help="--raw-out with --regions and --tracks: fill every region in a colour picked by its track id")
    ap.add_argument("--draw-ids", type=int, nargs="?", const=2, default=None, metavar="SCALE", help="--raw-out with --regions and --tracks: print every "
                    "region's track id at its centroid, in a 5 x 7 font scaled by SCALE (1..4, default 2)")
    ap.add_argument("--label-min-area", type=int, default=None, metavar="N", help="--draw-ids: regions below N pixels get no label (default 256)")
    args = ap.parse_args(argv)
    for given, name in ((args.draw_outlines is not None, "--draw-outlines"), (args.draw_tracks, "--draw-tracks"), (args.draw_ids is not None, "--draw-ids")):
        if given and not (args.raw_out and args.regions):
            ap.error(f"{name} needs --raw-out and --regions")
        if given and name != "--draw-outlines" and not args.tracks:
            ap.error(f"{name} needs --tracks")
    if args.draw_outlines is not None and not 0 <= args.draw_outlines <= 4:
        ap.error("--draw-outlines takes a width of 0..4 pixels")
    if args.draw_ids is not None and not 1 <= args.draw_ids <= 4:
        ap.error("--draw-ids takes a scale of 1..4")
    if args.label_min_area is not None and args.draw_ids is None:
        ap.error("--label-min-area needs --draw-ids")
    if args.label_min_area is not None and args.label_min_area < 1:
        ap.error("--label-min-area takes N >= 1")
    if args.tracks and not args.regions:
        ap.error("--tracks needs --regions")
    if args.outlines and not args.regions:
        ap.error("--outlines needs --regions")
    if not 1 <= args.max_contours <= 2 ** 20 or not 4 <= args.max_vertices <= 2 ** 22:
        ap.error("--max-contours takes 1..1048576 and --max-vertices 4..4194304")
    if args.simplify is not None and not args.outlines:
        ap.error("--simplify needs --outlines")
    if args.simplify is not None and not 0.0 <= args.simplify <= 256.0:
        ap.error("--simplify takes a tolerance of 0..256 pixels")
    if not 1 <= args.simplify_rounds <= 256:
        ap.error("--simplify-rounds takes 1..256")
    if args.compensate and not args.tracks:
        ap.error("--compensate needs --tracks: it changes how the tracks' links are counted")
    if args.compensate and (args.grids == "files" or (not args.raw and args.grids is None)):
        ap.error("--compensate needs the block matcher's vectors: --grids estimate (the grids/ folders hold grids, from which no vector can be recovered)")
    if not args.guide and (args.guide_outlier is not None or args.guide_bias is not None or args.guide_report):
        ap.error("--guide-outlier, --guide-bias and --guide-report need --guide")
    if args.guide and (args.grids == "files" or (not args.raw and args.grids is None)):
        ap.error("--guide needs the block matcher's vectors: --grids estimate (the grids/ folders hold grids, from which no vector can be recovered)")
    if (args.guide_outlier is not None and not 0 <= args.guide_outlier <= 64) or (args.guide_bias is not None and not 0 <= args.guide_bias <= 65535):
        ap.error("--guide-outlier takes 0..64 pixels and --guide-bias 0..65535")
    if args.guide_bias is not None and args.guide_outlier is None:
        ap.error("--guide-bias needs --guide-outlier: only a vector that disagrees with the camera's is put to the frames")
    if not args.mosaic and (args.mosaic_size is not None or args.mosaic_report):
        ap.error("--mosaic-size and --mosaic-report need --mosaic FILE.png")
    if args.mosaic_part and not (args.mosaic and args.ortho):
        ap.error("--mosaic-part needs --mosaic FILE.png and --ortho FILE.png: mosaics are registered against each other on their orthophotos")
    if args.mosaic and (args.grids == "files" or (not args.raw and args.grids is None)):
        ap.error("--mosaic needs the block matcher's vectors: --grids estimate (the grids/ folders hold grids, from which no vector can be recovered)")
    if args.mosaic and args.no_warp:
        ap.error("--mosaic needs the block matcher's vectors: --no-warp estimates none")
    if args.mosaic_size is not None and any(not 1 <= v <= 16384 for v in args.mosaic_size):
        ap.error("--mosaic-size takes H W of 1..16384 pixels")
    if not args.mosaic and (args.ortho or args.ortho_mode is not None or args.ortho_alpha is not None or args.ortho_edge is not None or args.ortho_plain):
        ap.error("--ortho and its options need --mosaic FILE.png: the orthophoto is gathered with the mosaic's poses, onto its canvas")
    if not args.ortho and (args.ortho_mode is not None or args.ortho_alpha is not None or args.ortho_edge is not None or args.ortho_plain):
        ap.error("--ortho-mode, --ortho-alpha, --ortho-edge and --ortho-plain need --ortho FILE.png")
    refine_options = (args.refine_search, args.refine_min_age, args.refine_every, args.refine_intra_bias)
    if not args.ortho and (args.mosaic_refine or any(v is not None for v in refine_options)):
        ap.error("--mosaic-refine and its options need --ortho FILE.png: a frame is registered against the orthophoto canvas")
    if not args.mosaic_refine and any(v is not None for v in refine_options):
        ap.error("--refine-search, --refine-min-age, --refine-every and --refine-intra-bias need --mosaic-refine")
    relocate_options = (args.relocate_scale, args.relocate_every, args.relocate_min_overlap, args.relocate_max_mean, args.relocate_ratio, args.relocate_report)
    if not args.ortho and (args.mosaic_relocate or any(v is not None for v in relocate_options)):
        ap.error("--mosaic-relocate and its options need --ortho FILE.png and --mosaic-refine: a lost frame is searched for on the orthophoto canvas")
    if not args.mosaic_refine and (args.mosaic_relocate or any(v is not None for v in relocate_options)):
        ap.error("--mosaic-relocate and its options need --mosaic-refine: a coarse placement is committed only through the fine registration")
    if not args.mosaic_relocate and any(v is not None for v in relocate_options):
        ap.error("--relocate-scale, --relocate-every, --relocate-min-overlap, --relocate-max-mean, --relocate-ratio and --relocate-report need --mosaic-relocate")
    args.relocate_scale = 8 if args.relocate_scale is None else args.relocate_scale
    args.relocate_every = 1 if args.relocate_every is None else args.relocate_every
    args.relocate_min_overlap = 0.5 if args.relocate_min_overlap is None else args.relocate_min_overlap
    args.relocate_max_mean = 16 if args.relocate_max_mean is None else args.relocate_max_mean
    args.relocate_ratio = 0.8 if args.relocate_ratio is None else args.relocate_ratio
    if (args.relocate_scale not in (4, 8, 16) or args.relocate_every < 1 or not 0.001 <= args.relocate_min_overlap <= 1 or not 0 <= args.relocate_max_mean <= 255
            or not 0.001 <= args.relocate_ratio <= 1):
        ap.error("--relocate-scale takes 4, 8 or 16, --relocate-every 1 or more, --relocate-min-overlap and --relocate-ratio 0.001..1 and --relocate-max-mean 0..255")
    args.refine_search = 8 if args.refine_search is None else args.refine_search
    args.refine_min_age = 0 if args.refine_min_age is None else args.refine_min_age
    args.refine_every = 1 if args.refine_every is None else args.refine_every
    args.refine_intra_bias = 65535 if args.refine_intra_bias is None else args.refine_intra_bias
    if not 1 <= args.refine_search <= 32 or args.refine_min_age < 0 or args.refine_every < 1 or not 0 <= args.refine_intra_bias <= 65535:
        ap.error("--refine-search takes 1..32, --refine-min-age 0 or more, --refine-every 1 or more and --refine-intra-bias 0..65535")
    args.ortho_mode = args.ortho_mode or "centre"
    args.ortho_alpha = 96 if args.ortho_alpha is None else args.ortho_alpha
    args.ortho_edge = args.ortho_edge or []
    if not 0 <= args.ortho_alpha <= 255 or any(not 0 <= k < min(args.classes, 32) for k in args.ortho_edge):
        ap.error(f"--ortho-alpha takes 0..255 and --ortho-edge class ids 0..{min(args.classes, 32) - 1}")
    if not 0 <= args.mosaic_rounds <= 8 or not 0 <= args.mosaic_tol <= 64 or any(not 0 <= k <= 31 for k in args.mosaic_exclude):
        ap.error("--mosaic-rounds takes 0..8, --mosaic-tol 0..64 pixels and --mosaic-exclude class ids 0..31")
    if args.proximity is not None and not args.regions:
        ap.error("--proximity needs --regions: the distances are tabulated per region")
    if args.proximity is None and (args.exposure or args.proximity_max is not None):
        ap.error("--exposure and --proximity-max need --proximity PX [PX ...]")
    if args.proximity is not None and (not 1 <= len(args.proximity) <= 8 or any(not 0 <= t <= 32767 for t in args.proximity)
                                       or any(b <= a for a, b in zip(args.proximity, args.proximity[1:]))):
        ap.error("--proximity takes 1..8 strictly ascending distances of 0..32767 pixels")
    if args.proximity_max is not None and (not 0 <= args.proximity_max <= 32767 or 0 < args.proximity_max < args.proximity[-1]):
        ap.error("--proximity-max takes R of 0..32767 pixels (0: unbounded), at least the largest PX")
    if not 0 <= args.stabilize <= 255:
        ap.error("--stabilize takes N of 0..255 frames")
    if (args.stabilize_trust is not None or args.stabilize_compensate) and args.stabilize <= 1:
        ap.error("--stabilize-trust and --stabilize-compensate need --stabilize N with N >= 2")
    if args.stabilize_trust is not None and (not args.confidence or not 0 <= args.stabilize_trust <= 256):
        ap.error("--stabilize-trust takes a code 0..256 and needs --confidence")
    if args.stabilize_compensate and (args.grids == "files" or (not args.raw and args.grids is None)):
        ap.error("--stabilize-compensate needs the block matcher's vectors: --grids estimate (the grids/ folders hold grids, from which no vector can be "
                 "recovered)")
    if args.min_overlap < 1 or (args.max_pairs is not None and (not 16 <= args.max_pairs <= 2 ** 20 or args.max_pairs & (args.max_pairs - 1))):
        ap.error("--min-overlap takes N >= 1 and --max-pairs a power of two in 16..1048576")
    if args.min_region < 0 or not 1 <= args.max_regions <= 65536:
        ap.error("--min-region takes N >= 0 and --max-regions 1..65536")
    if args.conf_out and not args.confidence:
        ap.error("--conf-out needs --confidence")
    if not 0 <= args.low_confidence <= 255:
        ap.error("--low-confidence takes a code 0..255")
    if not args.raw_out:
        for given, name in ((args.overlay is not None, "--overlay"), (args.overlay_keep_class0, "--overlay-keep-class0"),
                            (args.out_matrix is not None, "--out-matrix"), (args.out_full_range is not None, "--out-full-range"),
                            (args.out_pix_fmt != "nv12", "--out-pix-fmt")):
            if given:
                ap.error(f"{name} needs --raw-out")
    if args.overlay is not None and not 0 <= args.overlay <= 255:
        ap.error("--overlay takes an opacity 0..255")
    if args.overlay_keep_class0 and args.overlay is None:
        ap.error("--overlay-keep-class0 needs --overlay")
    if args.raw_out and args.out_pix_fmt == "rgb24" and (args.out_matrix is not None or args.out_full_range is not None):
        ap.error("--out-matrix / --out-full-range apply to the YUV output formats")
    if args.raw_out and args.raw and args.raw_out != "-" and os.path.abspath(args.raw_out) == os.path.abspath(args.raw):
        ap.error("--raw-out would overwrite the --raw input")
    if args.out_matrix is None:
        args.out_matrix = args.matrix if args.raw else "bt709"
    if args.out_full_range is None:
        args.out_full_range = bool(args.full_range) if args.raw else False
    if args.hold_cuts and (args.scene_cut is None or args.grids == "files" or (not args.raw and args.grids is None)):
        ap.error("--hold-cuts needs --scene-cut (and --grids estimate for a frame folder)")
    if not args.synthetic_weights and not args.ckpt:
        ap.error("give --ckpt or --synthetic-weights")
    if args.raw:
        if args.data_root:
            ap.error("--raw replaces --data-root / --video-id")
        if not args.raw_size:
            ap.error("--raw needs --raw-size H W")
        if args.grids == "files":
            ap.error("--raw has no grids/ folders: --grids estimate (the default there) or --no-warp")
        args.grids = "estimate"
    elif not args.data_root:
        ap.error("give --data-root (a frame folder) or --raw (a raw video file)")
    else:
        args.grids = args.grids or "files"
    return args


def mosaic_part_path(mosaic, rank):
    """The part file rank `rank` of a multi-rank launch writes beside --mosaic FILE.png: FILE.partNNN.npz."""
    return f"{os.path.splitext(mosaic)[0]}.part{int(rank):03d}.npz"


def merge_command(args, paths):
    """The tools/merge_mosaics.py command line that merges `paths` into what --mosaic, --ortho and --mosaic-report name."""
    merged = os.path.splitext(args.mosaic_report)[0] + ".merge.csv" if args.mosaic_report else None
    return " ".join(["python", "tools/merge_mosaics.py"] + list(paths) + ["--out", args.mosaic] + (["--ortho", args.ortho] if args.ortho else [])
                    + (["--report", merged] if merged else []))


def check_multi_rank_mosaic(args, world):
    """--mosaic under a multi-rank launch: every rank's pose chain is its own, and the ranks' mosaics are registered against each other on
    their orthophotos, so the launch needs --ortho."""
    if args.mosaic and world > 1 and not args.ortho:
        raise SystemExit("--mosaic under a multi-rank launch needs --ortho FILE.png: every rank's pose chain is its own, and the ranks' mosaics are "
                         "registered against each other on their orthophotos before they are merged")


def merge_rank_parts(pred, args, blocks):
    """Rank 0 of a multi-rank launch, after every rank has written its part: fold the parts of the ranks behind it, in rank order, into
    its own predictor's mosaic (FlowPredictor.merge_mosaic with the default link: a rank's anchor frame is the frame after the last one
    of the rank before it).  blocks[r]: the number of windows rank r had; a rank without windows wrote no part.  -> the merged parts'
    paths.  Enqueues only; pred.merge_report() reads back."""
    paths = [mosaic_part_path(args.mosaic, r) for r in range(1, len(blocks)) if blocks[r] > 0]
    for path in paths:
        pred.merge_mosaic(read_mosaic_part(path, "cuda"))
    return paths


def main():
    args = parse_args()

    rank, local_rank, world = shard.init()
    torch.cuda.set_device(local_rank)
    torch.set_grad_enabled(False)

    class HP:
        layers, classes, pretrained = args.layers, args.classes, False

    net = (FlowPSPNet if args.arch == "pspnet" else FlowDeepLabv3)(HP()).eval()
    load_weights(net, args)
    fm = FlowModel(net, feature_based=args.feature_based, no_warp=args.no_warp).eval()
    if args.tracks and world > 1:
        raise SystemExit("--tracks: track ids are per predictor and joining the ranks' blocks is out of scope: run it in a single process")
    check_multi_rank_mosaic(args, world)
    mosaic_size = None if not args.mosaic else tuple(args.mosaic_size) if args.mosaic_size else (min(2 * args.size[0], 16384), min(2 * args.size[1], 16384))
    draw = args.draw_outlines is not None or args.draw_tracks or args.draw_ids is not None
    pred = FlowPredictor(fm, classes=args.classes, out_size=tuple(args.size), crop=None if args.no_cropping else tuple(args.crop),
                         compute_metrics=not args.no_metrics, cache_keyframes=not args.no_keyframe_cache, confidence=args.confidence,
                         low_confidence=args.low_confidence, regions=bool(args.regions), min_region_area=args.min_region,
                         connectivity=args.connectivity, max_regions=args.max_regions, track=bool(args.tracks), min_overlap=args.min_overlap,
                         max_pairs=args.max_pairs, compensate=args.compensate, outlines=bool(args.outlines), max_contours=args.max_contours,
                         max_vertices=args.max_vertices, simplify=args.simplify, simplify_rounds=args.simplify_rounds, keep_window_regions=draw,
                         stabilize=args.stabilize, stabilize_trust=args.stabilize_trust, stabilize_compensate=args.stabilize_compensate,
                         proximity=args.proximity, proximity_sources=args.proximity_sources, proximity_targets=args.proximity_targets,
                         proximity_max=args.proximity_max, mosaic=mosaic_size, mosaic_classes=min(args.classes, 32), mosaic_rounds=args.mosaic_rounds,
                         mosaic_tol=args.mosaic_tol, mosaic_exclude=args.mosaic_exclude, ortho=args.ortho_mode if args.ortho else None,
                         mosaic_refine=args.mosaic_refine, refine_search=args.refine_search, refine_intra_bias=args.refine_intra_bias,
                         refine_min_age=args.refine_min_age, refine_every=args.refine_every,
                         mosaic_relocate=args.mosaic_relocate, relocate_scale=args.relocate_scale, relocate_every=args.relocate_every,
                         relocate_min_overlap=args.relocate_min_overlap, relocate_max_mean=args.relocate_max_mean, relocate_ratio=args.relocate_ratio)
    if (args.report or args.regions) and world > 1:
        raise SystemExit("--report / --regions cover one process's frames: run them on a single GPU")
    if args.raw:
        ds = RawVideoWindows(args.raw, args.raw_size[0], args.raw_size[1], args.pix_fmt, frame_delta=args.frame_delta, no_warp=args.no_warp,
                             size=tuple(args.size), grids=args.grids, search=args.search, penalty=args.penalty, matrix=args.matrix,
                             full_range=args.full_range, intra_bias=args.intra_bias, scene_cut=args.scene_cut, hold_cuts=args.hold_cuts,
                             link_vectors=args.compensate or args.stabilize_compensate or bool(args.mosaic), link_sources=bool(args.ortho),
                             guide=args.guide, guide_outlier=args.guide_outlier, guide_bias=args.guide_bias)
    else:
        ds = PredictWindows(args.data_root, args.video_id, frame_delta=args.frame_delta, no_warp=args.no_warp, size=tuple(args.size),
                            grids=args.grids, search=args.search, penalty=args.penalty, intra_bias=args.intra_bias, scene_cut=args.scene_cut,
                            hold_cuts=args.hold_cuts, link_vectors=args.compensate or args.stabilize_compensate or bool(args.mosaic),
                            link_sources=bool(args.ortho), guide=args.guide, guide_outlier=args.guide_outlier, guide_bias=args.guide_bias)
    palette = np.loadtxt(args.palette).astype("uint8") if args.palette else PALETTE
    if args.out and rank == 0:
        os.makedirs(args.out, exist_ok=True)
    writer = None
    if args.raw_out:
        h, w = args.size
        pal = np.asarray(palette, dtype=np.uint8)
        if args.overlay is not None:   # per-class opacity: [K,4]
            pal = np.concatenate([pal[:, :3], np.full((pal.shape[0], 1), args.overlay, dtype=np.uint8)], axis=1)
            if args.overlay_keep_class0:
                pal[0, 3] = 0
        # every rank sizes the one file for all frames and writes its own window block into it
        writer = RawVideoWriter(args.raw_out, h, w, args.out_pix_fmt, frames=None if args.raw_out == "-" else len(ds) * args.frame_delta,
                                world=world)
        if rank == 0:
            ff = {"nv12": "nv12", "i420": "yuv420p", "rgb24": "rgb24"}[args.out_pix_fmt]
            print(f"encode with: ffmpeg -f rawvideo -pix_fmt {ff} -s {w}x{h} -r 25 -i {args.raw_out} result.mp4"
                  + ("" if args.out_pix_fmt == "rgb24" else f"   ({args.out_matrix}, {'full' if args.out_full_range else 'limited'} range)"), file=sys.stderr)
    style = None
    if draw:  # the drawing options of ops.compose_regions
        style = {"outline_width": 0}
        if args.draw_outlines:
            line = np.full((len(palette), 4), 255, dtype=np.uint8)   # white, opaque; a guess
            if args.overlay_keep_class0:
                line[0, 3] = 0
            style.update(outline=line, outline_width=args.draw_outlines)
        if args.draw_tracks:
            style["fill_palette"] = np.asarray(ops.TRACK_PALETTE, dtype=np.uint8)
        if args.draw_ids is not None:
            style.update(label_scale=args.draw_ids, label_min_area=256 if args.label_min_area is None else args.label_min_area)
    conf_writer = None
    if args.conf_out:
        conf_writer = RawVideoWriter(args.conf_out, args.size[0], args.size[1], "gray", frames=len(ds) * args.frame_delta, world=world)
    shard.barrier()

    # windows are independent units given their two key frames: each rank takes a contiguous block (SURVEY 8e "frame-window
    # sharding"), so that the temporal-consistency pairs inside a block are the reference's; the pair across each block
    # boundary (this rank's first frame vs the previous block's last) is scored after the loop from the neighbour's mask
    mine = shard.window_block(len(ds), rank, world)
    frames = 0
    first_mask = last_mask = None
    sources = []  # --hold-cuts: every window's device `source` tensor, read back once after the timed run
    report_ids, areas = [], []  # --report / --regions: the frame ids, and without --confidence every window's device counts
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for w in mine:
        item = ds[w]
        masks = pred.predict_window(item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"], to_host=False,
                                    key_ids=item["key_ids"], weights=item.get("weights"), link_mvs=item.get("link_mvs"),
                                    link_frame_size=item.get("link_frame_size"), link_stats=item.get("link_stats"), link_sources=item.get("link_sources"),
                                    link_raw_mvs=item.get("link_raw_mvs"), link_guide_counts=item.get("link_guide_counts"))
        if args.confidence:
            masks, conf = masks
            if conf_writer is not None:
                for p in range(conf.shape[0]):
                    conf_writer.write(item["frame_id"] + p, conf[p].reshape(-1))
        elif args.report:
            areas.append(ops.frame_report(masks, None, args.classes))
        report_ids.extend(item["frame_id"] + p for p in range(masks.shape[0]))
        if "source" in item:
            sources.append(item["source"])
        if first_mask is None:
            first_mask = masks[0].clone()
        last_mask = masks[-1]
        frames += masks.shape[0]
        if writer is not None:
            frames_of = (lambda p: ds.source(item["frame_id"] + p)) if args.overlay is not None else None
            for p, buf in enumerate(compose_window(masks, frames_of, pal, out_fmt=args.out_pix_fmt, out_matrix=args.out_matrix,
                                                   out_full_range=args.out_full_range, regions=pred.window_regions() if draw else None,
                                                   style=style)):
                writer.write(item["frame_id"] + p, buf)
        if args.out:
            from PIL import Image

            rgb = colorize(masks, palette).cpu().numpy()
            for p in range(rgb.shape[0]):
                Image.fromarray(rgb[p]).save(os.path.join(args.out, f"{item['frame_id'] + p}.png"))
    if writer is not None:
        writer.close()   # the last two frames' copies and writes belong to the timed work
    if conf_writer is not None:
        conf_writer.close()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0  # this rank's own work: the end-of-run exchange below waits for the slowest rank and is not part of it
    if world > 1 and not args.no_metrics:
        dev = torch.device("cuda", local_rank)
        blank = torch.zeros(tuple(args.size), dtype=torch.uint8, device=dev)
        neighbour = shard.exchange_boundary(last_mask if last_mask is not None else blank, len(mine) > 0, dev)
        if neighbour is not None:  # flow/base.py:284-291 for p == 0 with last_output = the previous block's final frame
            pred.hist = ops.iou_hist(first_mask, neighbour, args.classes, 255, pred.hist)
    torch.cuda.synchronize()
    hist = pred.hist if pred.hist is not None else torch.zeros(3, args.classes, dtype=torch.int64)
    hist, frames, seconds = shard.reduce_run(hist.cpu() if world == 1 else hist, frames, seconds, "cpu" if world == 1 else torch.device("cuda", local_rank))
    if rank == 0:
        h = hist.double()
        line = f"{frames} frames of {args.raw or args.video_id} in {seconds:.2f} s = {frames / seconds:.1f} FPS on {world} GPU(s)"
        if not args.no_metrics and float(h[2].sum()) > 0:
            inter, union, target = h[0], h[1] + h[2] - h[0], h[2]
            line += (f"; temporal consistency mIoU {float((inter / (union + 1e-10)).mean()):.4f}"
                     f" mAcc {float((inter / (target + 1e-10)).mean()):.4f} acc {float(inter.sum() / (target.sum() + 1e-10)):.4f}")
        print(line, file=sys.stderr if args.raw_out == "-" else sys.stdout)   # standard output may be the video
    if args.stabilize > 1:  # the device counts are read back ONCE, here, after the timed run
        held, switched, seeded, trusted = pred.stabilize_report().sum(0).tolist()
        print(f"rank {rank}: --stabilize {args.stabilize}: {held} pixels held, {switched} switched ({trusted} of them trusted), {seeded} seeded",
              file=sys.stderr if args.raw_out == "-" else sys.stdout)
    kept = ds.estimator.estimated_stats() if ds.estimator is not None else {}
    if kept:  # --intra-bias / --scene-cut: the kept device stats are read back ONCE, here, after the timed run
        ids = sorted(kept)
        host = torch.stack([kept[i] for i in ids]).cpu().numpy()
        cuts = [i for i, s in zip(ids, host) if s[2]]
        print(f"rank {rank}: {len(ids)} frame pairs estimated, mean intra share {float((host[:, 1] / host[:, 0]).mean()):.4f}, "
              f"scene cuts at frames {cuts if cuts else 'none'}", file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if args.guide and ds.estimator is not None:  # the kept device counts are read back ONCE, here, after the timed run
        guided_ids, guided = ds.estimator.guide_report()
        if args.guide_report:
            write_guide_csv(args.guide_report, guided_ids, guided)
        print(f"rank {rank}: --guide: {len(guided_ids)} frame pairs, {int(guided[:, 2].sum())} rows filled, {int(guided[:, 4].sum())} replaced, "
              f"{int(guided[:, 5].sum())} dropped, {int(guided[:, 6].sum())} kept by evidence", file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if sources:
        counts = torch.bincount(torch.cat(sources).cpu().long(), minlength=4).tolist()
        print(f"rank {rank}: --hold-cuts: {counts[0]} frames blended, {counts[1]} held from the previous key frame, {counts[2]} from the next, "
              f"{counts[3]} between two cuts", file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if args.mosaic and world > 1:  # every rank's mosaic is its own: each writes FILE.partNNN.npz, rank 0 merges them behind the wait below
        blocks = [len(shard.window_block(len(ds), r, world)) for r in range(world)]
        if blocks[rank] > 0:
            write_mosaic_part(mosaic_part_path(args.mosaic, rank), pred.mosaic_part())
        shard.barrier(torch.device("cuda", local_rank))
        if rank == 0 and blocks[0] > 0:
            paths = merge_rank_parts(pred, args, blocks)
            links, outs, counts = pred.merge_report()
            if args.mosaic_report:
                write_merge_csv(os.path.splitext(args.mosaic_report)[0] + ".merge.csv", [os.path.basename(p) for p in paths], (links, outs, counts))
            for path, link, count in zip(paths, links.tolist(), counts.tolist()):
                print(f"--mosaic: {os.path.basename(path)} " + (f"merged: {count[2]} pixels received {count[3]} votes, {count[4]} orthophoto pixels taken"
                                                               if link[12] == 0 else "could NOT be registered against the ranks before it and is left out"),
                      file=sys.stderr if args.raw_out == "-" else sys.stdout)
        elif rank == 0:  # fewer windows than ranks: rank 0 has no mosaic to merge into
            print("--mosaic: rank 0 had no window; merge the parts by hand: "
                  + merge_command(args, [mosaic_part_path(args.mosaic, r) for r in range(world) if blocks[r] > 0]), file=sys.stderr if args.raw_out == "-" else sys.stdout)
    mosaic_out = bool(args.mosaic) and (world == 1 or (rank == 0 and len(mine) > 0))  # under a multi-rank launch rank 0 writes the merged outputs
    if mosaic_out:  # the canvas is resolved and read back ONCE, here, after the timed run
        from PIL import Image

        cls, _, seen, totals, poses = pred.mosaic_report()
        rgb = colorize(torch.from_numpy(cls).cuda(), palette).cpu().numpy()
        rgb[cls == 255] = 0  # no frame looked here
        Image.fromarray(rgb).save(args.mosaic)
        if args.mosaic_report:
            write_mosaic_csv(args.mosaic_report, report_ids, poses, totals, pred.refine_report() if args.mosaic_refine else None)
        lost = int((poses[:, 12] == 2).sum())
        print(f"--mosaic: {int((seen > 0).sum())} canvas pixels seen by {len(poses) - lost} frames"
              + (f"; {lost} frames lost (a scene cut, or more failed fits running than are bridged)" if lost else "")
              + (f"; {int(poses[:, 13].sum())} frames reach beyond the canvas (--mosaic-size)" if poses[:, 13].any() else ""),
              file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if args.mosaic_part and mosaic_out:  # the part's read-back, after the timed run (a multi-rank launch: the merged mosaic)
        write_mosaic_part(args.mosaic_part, pred.mosaic_part())
        print(f"--mosaic-part: {args.mosaic_part} (merge parts with tools/merge_mosaics.py)", file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if args.ortho and mosaic_out:  # drawn and read back ONCE, here, after the timed run
        from PIL import Image

        image, src, covered = pred.ortho_report(palette=palette, alpha=args.ortho_alpha, edge=args.ortho_edge, overlay=not args.ortho_plain)
        Image.fromarray(image).save(args.ortho)
        print(f"--ortho: {covered} canvas pixels covered, taken from {len(set(np.unique(src).tolist()) - {-1})} frames ({args.ortho_mode} view wins)",
              file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if args.mosaic_refine:
        status = pred.refine_report()[:, 0]
        print(f"--mosaic-refine: {int((status == 0).sum())} of {len(status)} frames corrected against the map, {int((status == 2).sum())} without a fit",
              file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if args.mosaic_relocate:
        relocated = pred.relocate_report()
        if args.relocate_report and rank == 0:
            write_relocate_csv(args.relocate_report, report_ids, relocated)
        print(f"--mosaic-relocate: the chain was relocalised {int((relocated[:, 0] == 0).sum())} times; {int((relocated[:, 0] > 1).sum())} attempts on a lost chain failed",
              file=sys.stderr if args.raw_out == "-" else sys.stdout)
    if args.report:  # the device report is read back ONCE, here, after the timed run
        report = pred.extent_report() if args.confidence else (torch.cat(areas).cpu().numpy() if areas else np.zeros((0, args.classes, 3), np.int64))
        write_extent_csv(args.report, report_ids, report, args.size[0] * args.size[1], with_confidence=args.confidence)
    if args.min_region > 1:  # the filter pass's counts, read back once after the timed run
        for fid, total in zip(report_ids, pred.despeckle_counts().tolist()):
            if total > args.max_regions:
                print(f"warning: frame {fid} had {total} regions before --min-region, --max-regions {args.max_regions}: only the first "
                      f"{args.max_regions} (in raster order) were filtered", file=sys.stderr)
    if args.regions:  # likewise: one read-back after the timed run
        region_rows, totals = pred.region_report()
        track_rows, overflowed, cut = pred.track_report(with_cuts=True) if args.tracks else (None, [], [])
        outlines = pred.outline_report() if args.outlines else None
        exposure, near_rows = pred.proximity_report() if args.proximity else (None, None)
        write_regions_csv(args.regions, report_ids, region_rows, with_confidence=args.confidence, tracks=track_rows,
                          shapes=[o[2] for o in outlines[0]] if outlines else None, proximity=near_rows)
        if args.exposure:
            write_exposure_csv(args.exposure, report_ids, exposure, args.proximity, args.size[0] * args.size[1])
        if outlines:
            simple = pred.simple_outline_report() if args.simplify is not None else None
            write_outlines_geojson(args.outlines, report_ids, region_rows, outlines, tracks=track_rows, simplified=simple, tolerance=args.simplify)
            if simple:
                for fid, (_, _, _, flag) in zip(report_ids, simple[1].tolist()):
                    if flag & 1:
                        print(f"warning: frame {fid} has rings that were still being split after --simplify-rounds {args.simplify_rounds}: their open "
                              "segments keep all vertices", file=sys.stderr)
                    if flag & ~1:
                        print(f"warning: frame {fid} is not simplified in full (flags {flag}: 2 = its outlines overflowed, 4 = contours without a "
                              "row, 8 = inconsistent rows)", file=sys.stderr)
                kept, full = int(simple[1][:, 1].sum()), sum(len(o[1]) for o in outlines[0])
                print(f"simplify {args.simplify} px: {kept} of {full} vertices written; the largest number of rounds a frame needed: "
                      f"{int(simple[1][:, 2].max()) if len(simple[1]) else 0} (--simplify-rounds {args.simplify_rounds})", file=sys.stderr)
            for fid, flag in zip(report_ids, outlines[1].tolist()):
                if flag & 1:
                    print(f"warning: frame {fid} has more than --max-vertices {args.max_vertices} outline vertices: it has no outlines",
                          file=sys.stderr)
                elif flag & 2:
                    print(f"warning: frame {fid} has more than --max-contours {args.max_contours} contours: the first {args.max_contours} are "
                          "written", file=sys.stderr)
        if args.tracks:
            write_tracks_csv(args.tracks, report_ids, region_rows, track_rows, proximity=near_rows)
            for fid, flag in zip(report_ids, overflowed.tolist()):
                if flag:
                    print(f"warning: frame {fid}: the pair table overflowed (--max-pairs {pred.max_pairs}): its regions all start new tracks",
                          file=sys.stderr)
            cut_ids = [fid for fid, flag in zip(report_ids, cut.tolist()) if flag]
            if cut_ids:
                print(f"--compensate: frames {cut_ids} follow a scene cut: their regions all start new tracks", file=sys.stderr)
        for fid, total in zip(report_ids, totals.tolist()):
            if total > args.max_regions:
                print(f"warning: frame {fid} has {total} regions, --max-regions {args.max_regions}: the first {args.max_regions} are listed",
                      file=sys.stderr)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
