"""A flood mosaic in map coordinates: hectares per class, region polygons in eastings and northings, north-up rasters:

    python tools/mosaic_ground.py PART.npz --gcp FILE.csv [--gcp-indices] [--kind similarity|affine|projective] [--gsd M] [--crs NAME]
                                  [--class-png F.png] [--ortho-png F.png] [--areas F.csv] [--outlines F.geojson] [--simplify PX]
                                  [--min-votes N] [--max-regions N]

PART is a mosaic part, what `tools/predict_video.py --mosaic-part FILE.npz` (or flow.mosaic.write_mosaic_part) wrote.  --gcp names the
control points: a CSV with the columns x,y,easting,northing, x and y continuous coordinates in the written mosaic or orthophoto PNG
(pixel i covers [i, i+1)); with --gcp-indices they are pixel indices as an image viewer shows them, and half a pixel is added.
Eastings and northings are metres of any projected CRS; --crs is only written through to the files.  The ground model (--kind, by
default affine) is fitted on the host; the areas, the rasters and the polygons' coordinates are computed on the GPU.  --gsd is the
rasters' pixel in metres, by default the model's mean pixel size rounded to millimetres.  Each PNG gets a six-line .pgw world file
beside it.  --areas has one row per class (m^2, hectares, share), the fit's residuals and one row per region; --outlines one polygon
per region, with holes; --simplify PX simplifies them first (Ramer-Douglas-Peucker, PX canvas pixels).

A planar ground model over the mosaic's affine pose chain: the chain's drift and the parallax of anything above the ground are in the
result.  No DEM, no lens model; not validated on real video or against surveyed points."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flood_uav_video_segmentation_amd.flow.georef import KINDS, GroundModel, read_gcp_csv  # noqa: E402
from flood_uav_video_segmentation_amd.flow.mosaic import (ground_report, mosaic_ground, read_mosaic_part, write_ground_csv, write_ground_geojson,  # noqa: E402
                                                          write_ground_png)

CLASS_NAMES = ("background", "water", "tree", "building", "street")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", metavar="PART.npz", help="the mosaic part")
    ap.add_argument("--gcp", required=True, metavar="FILE.csv", help="control points: x,y,easting,northing")
    ap.add_argument("--gcp-indices", action="store_true", help="x and y are pixel indices: half a pixel is added")
    ap.add_argument("--kind", default="affine", choices=sorted(KINDS), help="the ground model")
    ap.add_argument("--gsd", type=float, default=None, metavar="M", help="the rasters' pixel in metres (default: the model's mean pixel size)")
    ap.add_argument("--crs", default=None, metavar="NAME", help="the CRS' name, written through to the files")
    ap.add_argument("--class-png", default=None, metavar="FILE.png", help="the class plane as a north-up raster, with a .pgw beside it")
    ap.add_argument("--ortho-png", default=None, metavar="FILE.png", help="the orthophoto as a north-up raster, with a .pgw beside it")
    ap.add_argument("--areas", default=None, metavar="FILE.csv", help="m^2 per class and per region, the fit's residuals")
    ap.add_argument("--outlines", default=None, metavar="FILE.geojson", help="one polygon per region in eastings and northings")
    ap.add_argument("--simplify", type=float, default=None, metavar="PX", help="simplify the outlines within PX canvas pixels")
    ap.add_argument("--min-votes", type=int, default=1, metavar="N", help="a pixel with fewer votes counts as never seen (1..65535)")
    ap.add_argument("--max-regions", type=int, default=1024, metavar="N", help="rows of the region table (1..65536)")
    args = ap.parse_args(argv)
    if not (args.class_png or args.ortho_png or args.areas or args.outlines):
        ap.error("nothing to write: give --class-png, --ortho-png, --areas or --outlines")
    if args.gsd is not None and not 0.001 <= args.gsd <= 1048.576:
        ap.error("--gsd takes 0.001 .. 1048.576 metres")
    if args.simplify is not None and not args.outlines:
        ap.error("--simplify goes with --outlines")
    if args.simplify is not None and not 0.0 <= args.simplify <= 256.0:
        ap.error("--simplify takes 0..256 pixels")
    if not 1 <= args.min_votes <= 65535:
        ap.error("--min-votes takes 1..65535")
    if not 1 <= args.max_regions <= 65536:
        ap.error("--max-regions takes 1..65536")
    return args


def main(argv=None):
    args = parse_args(argv)
    torch.set_grad_enabled(False)
    xy, en = read_gcp_csv(args.gcp, indices=args.gcp_indices)
    part = read_mosaic_part(args.part, "cuda")
    model = GroundModel.fit(xy, en, args.kind, origin=part["origin"], crs=args.crs)
    if args.ortho_png and part.get("rgba") is None:
        raise SystemExit(f"{args.part} has no orthophoto (a mosaic made with ortho=): --ortho-png has nothing to draw")
    regions = bool(args.areas or args.outlines)
    result = mosaic_ground(part, model, gsd=args.gsd, regions=regions, outlines=bool(args.outlines), simplify=args.simplify, min_votes=args.min_votes,
                           max_regions=args.max_regions, raster=bool(args.class_png or args.ortho_png))
    report = ground_report(result)
    if args.areas:
        write_ground_csv(args.areas, report, CLASS_NAMES)
    if args.class_png:
        write_ground_png(args.class_png, report, "class")
    if args.ortho_png:
        write_ground_png(args.ortho_png, report, "ortho")
    if args.outlines:
        write_ground_geojson(args.outlines, report, CLASS_NAMES)
    water = report["classes"][1][1] if len(report["classes"]) > 1 else 0.0
    print(f"{os.path.basename(args.part)}: {report['summed_m2'] / 1e4:.4f} ha seen, {water / 1e4:.4f} ha water; {model.kind} fit of {len(model.residuals)} points, "
          f"RMS {model.rms:.3f} m" + (f"; {int(report['counts'][1])} folded pixels" if int(report["counts"][1]) else ""))


if __name__ == "__main__":
    main()
