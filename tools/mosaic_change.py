"""Where the water advanced and where it receded between two flights over the same ground:

    python tools/mosaic_change.py BEFORE.npz AFTER.npz --out CHANGE.png [--report CHANGE.csv] [--regions REGIONS.csv]
                                  [--outlines OUTLINES.geojson] [--min-region N] [--tolerance R] [--min-votes N] [--min-conf C]
                                  [--watch K ...] [--search-scale S] [--no-register]

BEFORE and AFTER are mosaic parts, what `tools/predict_video.py --mosaic-part FILE.npz` (or flow.mosaic.write_mosaic_part) wrote.  AFTER
is registered against BEFORE on their orthophotos, starting from "both have the same anchor" (`--search-scale S`, 4, 8 or 16, first
slides AFTER's seen box over the whole map in S x S cells, as merge_mosaics.py does), and compared class by class in BEFORE's canvas;
nothing is merged.  --out is BEFORE's orthophoto with the pixels that differ drawn over it: explained by the tolerance, changed between
two other classes, gained (the --watch classes, by default class 1, appeared) and lost.  --report has, per class pair, the comparable
and the changed pixels, then the eight counts; --regions and --outlines list every connected area of one code as predict_video.py's
--regions and --outlines do (class = the change code, frame 0).  --no-register compares under the identity link: two parts of one
anchor.  The defaults are guesses, not validated on real video."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flood_uav_video_segmentation_amd import ops  # noqa: E402
from flood_uav_video_segmentation_amd.flow.mosaic import LINK_STATUS, change_report, mosaic_change, read_mosaic_part, write_change_csv, write_change_png  # noqa: E402
from flood_uav_video_segmentation_amd.flow.predict import write_outlines_geojson, write_regions_csv  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before", metavar="BEFORE.npz", help="the mosaic part whose canvas the change is drawn in")
    ap.add_argument("after", metavar="AFTER.npz", help="the mosaic part of the later flight")
    ap.add_argument("--out", required=True, metavar="FILE.png", help="the change drawn over BEFORE's orthophoto")
    ap.add_argument("--report", default=None, metavar="FILE.csv", help="per class pair the comparable and the changed pixels, then the counts")
    ap.add_argument("--regions", default=None, metavar="FILE.csv", help="every connected area of one change code: area, box, centroid")
    ap.add_argument("--outlines", default=None, metavar="FILE.geojson", help="the same areas as polygons")
    ap.add_argument("--min-region", type=int, default=0, metavar="N", help="areas below N pixels take their neighbours' code first")
    ap.add_argument("--tolerance", type=int, default=1, metavar="R", help="a difference that a shift of at most R pixels explains is no change (0..8)")
    ap.add_argument("--min-votes", type=int, default=1, metavar="N", help="a pixel with fewer votes is not compared (1..65535)")
    ap.add_argument("--min-conf", type=int, default=0, metavar="C", help="nor one whose winning class has a smaller share, in 255ths (0..255)")
    ap.add_argument("--watch", type=int, nargs="+", default=[1], metavar="K", help="the class ids that count as water")
    ap.add_argument("--search-scale", type=int, default=None, metavar="S", help="place AFTER coarsely first, in cells of S x S canvas pixels (4, 8 or 16)")
    ap.add_argument("--no-register", action="store_true", help="compare under the identity link")
    args = ap.parse_args(argv)
    if args.search_scale is not None and args.search_scale not in ops.RELOCATE_SCALES:
        ap.error("--search-scale takes 4, 8 or 16")
    if args.search_scale is not None and args.no_register:
        ap.error("--search-scale places AFTER for the registration: it does not go with --no-register")
    if not 0 <= args.tolerance <= ops.CHANGE_MAX_TOLERANCE:
        ap.error(f"--tolerance takes 0..{ops.CHANGE_MAX_TOLERANCE} pixels")
    if not 1 <= args.min_votes <= 65535 or not 0 <= args.min_conf <= 255:
        ap.error("--min-votes takes 1..65535 and --min-conf 0..255")
    if args.min_region < 0:
        ap.error("--min-region takes a pixel count")
    return args


def main(argv=None):
    args = parse_args(argv)
    torch.set_grad_enabled(False)
    before, after = read_mosaic_part(args.before, "cuda"), read_mosaic_part(args.after, "cuda")
    if not args.no_register and (before["rgba"] is None or after["rgba"] is None):
        raise SystemExit("a part has no orthophoto: the registration reads both (predict_video.py --ortho), or compare with --no-register")
    kw = dict(min_votes=args.min_votes, min_conf=args.min_conf, tolerance=args.tolerance, watch=args.watch)
    if args.no_register:
        kw.update(register=False, link=ops.mosaic_link(status=ops.LINK_REGISTERED, device="cuda"))
    elif args.search_scale is not None:
        kw.update(place=dict(scale=args.search_scale))
    want_regions = bool(args.regions or args.outlines)
    result = mosaic_change(before, after, regions=want_regions, min_region_area=args.min_region if want_regions else 0, outlines=bool(args.outlines), **kw)
    report = change_report(result)              # the read-back happens here, after everything is enqueued
    write_change_png(args.out, result, before["rgba"])
    if args.report:
        write_change_csv(args.report, report)
    if args.regions:
        write_regions_csv(args.regions, [0], report["rows"], with_confidence=False, shapes=report["shapes"])
    if args.outlines:
        write_outlines_geojson(args.outlines, [0], report["rows"], report["outlines"])
    counts, link = report["counts"].tolist(), report["link"].tolist()
    status = LINK_STATUS[link[12]] if 0 <= link[12] < len(LINK_STATUS) else "out_of_bounds"
    print(f"{os.path.basename(args.after)} against {os.path.basename(args.before)}: {status}; shift ({link[2] / (1 << 20):.2f}, {link[5] / (1 << 20):.2f}) px; "
          f"{counts[2]} comparable pixels: {counts[3]} same, {counts[4]} explained, {counts[5]} changed, {counts[6]} gained, {counts[7]} lost"
          + ("" if link[12] == 0 else " -- NOT COMPARED"))


if __name__ == "__main__":
    main()
