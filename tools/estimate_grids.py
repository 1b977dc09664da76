#!/usr/bin/env python3
"""Offline replacement for the reference's dataset/flow/extract_motion_vectors.py on a FRAME FOLDER: writes

    <DATA_ROOT>/frames/<VIDEO_ID>/grids/<i>.npy  and  inv_grids/<i>.npy      (float64 [67,120,2], the reference's format)

for every <DATA_ROOT>/frames/<VIDEO_ID>/images/<i>.jpg, from block matching of frame i against frame i-1 on the GPU
(flow/motion.py) instead of an H.264 stream's vectors.  Files that exist are skipped, as the reference's script does.  Frame 0
and a frame whose predecessor is missing get the default grid.  Encoder vectors and these differ (rate-distortion choices,
sub-pel vectors, I-frames); the table -> grid step is the same code.

    python tools/estimate_grids.py dataset/flow florida-01 --search 16 --penalty 0
    python tools/estimate_grids.py dataset/flow florida-01 --intra-bias 256 --scene-cut 0.5     (unexplained blocks and cuts: identity)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flood_uav_video_segmentation_amd.flow.dataset import PredictWindows  # noqa: E402
from flood_uav_video_segmentation_amd.flow.grids import save_grid  # noqa: E402
from flood_uav_video_segmentation_amd.flow.motion import GridEstimator  # noqa: E402
from flood_uav_video_segmentation_amd.flow.predict import write_guide_csv  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("data_root")
    ap.add_argument("video_id")
    ap.add_argument("--search", type=int, default=16)
    ap.add_argument("--penalty", type=int, default=0)
    ap.add_argument("--intra-bias", type=int, metavar="N", help="0..65535: a block whose best match is worse than its own deviation from its "
                    "mean + N gets no vector (its cells keep the identity grid); default: off.  The right N depends on the sensor's noise")
    ap.add_argument("--scene-cut", type=float, metavar="F", help="0..1: a frame with more than this fraction of such blocks gets the default "
                    "grid (a scene cut); default: off.  Counts the blocks --intra-bias marks: without --intra-bias it never fires")
    ap.add_argument("--guide", action="store_true", help="guide the matcher's tables with the camera motion fitted to them (ops.guide_vectors; "
                    "DESIGN 3.21): blocks without a vector take the camera's.  Default: off")
    ap.add_argument("--guide-outlier", type=float, metavar="PX", help="--guide: also replace vectors further than PX pixels (0..64) from the camera's")
    ap.add_argument("--guide-bias", type=int, metavar="N", help="--guide-outlier: replace only where the camera's window explains the block no worse "
                    "than the winner did, up to N (0..65535); default: replace as it stands")
    ap.add_argument("--guide-report", metavar="FILE.csv", help="--guide: per frame pair the counts of void, filled, outlier, replaced, dropped and kept rows")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if not args.guide and (args.guide_outlier is not None or args.guide_bias is not None or args.guide_report):
        ap.error("--guide-outlier, --guide-bias and --guide-report need --guide")
    if (args.guide_outlier is not None and not 0 <= args.guide_outlier <= 64) or (args.guide_bias is not None and not 0 <= args.guide_bias <= 65535):
        ap.error("--guide-outlier takes 0..64 pixels and --guide-bias 0..65535")
    if args.guide_bias is not None and args.guide_outlier is None:
        ap.error("--guide-bias needs --guide-outlier: only a vector that disagrees with the camera's is put to the frames")

    folder = os.path.join(args.data_root, "frames", args.video_id)
    ids = sorted(int(n[:-4]) for n in os.listdir(os.path.join(folder, "images")) if n.endswith(".jpg") and n[:-4].isdigit())
    for name in ("grids", "inv_grids"):
        os.makedirs(os.path.join(folder, name), exist_ok=True)
    frames = PredictWindows(args.data_root, args.video_id, no_warp=True, device=args.device)  # paths + decoding only
    estimator = GridEstimator(args.search, args.penalty, intra_bias=args.intra_bias, scene_cut=args.scene_cut, guide=args.guide,
                              guide_outlier=args.guide_outlier, guide_bias=args.guide_bias)
    written = 0
    for i in ids:
        paths = [frames.grid_path(i, "grids"), frames.grid_path(i, "inv_grids")]
        if all(os.path.exists(p) for p in paths):
            continue
        for path, grid in zip(paths, estimator.grids_for(i, frames.raw_frame)):
            if not os.path.exists(path):
                save_grid(path, grid)
                written += 1
    print(f"estimate_grids: {len(ids)} frames, {written} files written under {folder}")
    if args.guide_report:  # the counts are read back ONCE, here
        write_guide_csv(args.guide_report, *estimator.guide_report())
    return 0


if __name__ == "__main__":
    sys.exit(main())
