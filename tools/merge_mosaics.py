"""Merge the flood-extent mosaics of several pose chains into one:

    python tools/merge_mosaics.py FLIGHT.part000.npz FLIGHT.part001.npz ... --out MOSAIC.png [--ortho ORTHO.png] [--report MERGE.csv]
                                  [--search-scale S]

The parts are what `tools/predict_video.py --mosaic-part FILE.npz` (or flow.mosaic.write_mosaic_part) wrote, each with an orthophoto.  They
are merged IN ORDER into the first: part k is registered against the mosaic so far, starting from the link "its anchor frame is the frame
after the last one merged" (the case of consecutive blocks of one video), and its votes and orthophoto are folded in on the GPU.
`--search-scale S` (4, 8 or 16) first slides the part's seen box over the whole map in S x S cells, for parts that do not follow on from
each other within the matcher's 16 pixels.  A part that cannot be registered changes nothing and is reported.  --out, --ortho and
--report are what predict_video.py's --mosaic, --ortho and (per part, not per frame) --mosaic-report write.  Votes are not idempotent:
naming a part twice counts its frames twice.  The defaults of the registration are guesses, not validated on real video."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flood_uav_video_segmentation_amd import ops  # noqa: E402
from flood_uav_video_segmentation_amd.flow.mosaic import LINK_STATUS, merge_part, read_mosaic_part, write_merge_csv  # noqa: E402
from flood_uav_video_segmentation_amd.flow.predict import PALETTE, colorize  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parts", nargs="+", metavar="PART.npz", help="mosaic parts, merged in this order into the first")
    ap.add_argument("--out", required=True, metavar="FILE.png", help="the merged extent map, as --mosaic writes it")
    ap.add_argument("--ortho", default=None, metavar="FILE.png", help="the merged orthophoto with the extent map over it, as --ortho writes it")
    ap.add_argument("--report", default=None, metavar="FILE.csv", help="per merged part the link, the registration and the counts")
    ap.add_argument("--search-scale", type=int, default=None, metavar="S", help="place every part coarsely first, in cells of S x S canvas pixels (4, 8 or 16)")
    args = ap.parse_args(argv)
    if len(args.parts) < 2:
        ap.error("name at least two parts: the first is merged into")
    if args.search_scale is not None and args.search_scale not in ops.RELOCATE_SCALES:
        ap.error("--search-scale takes 4, 8 or 16")
    return args


def main(argv=None):
    from PIL import Image

    args = parse_args(argv)
    torch.set_grad_enabled(False)
    mine = read_mosaic_part(args.parts[0], "cuda")
    if mine["rgba"] is None:
        raise SystemExit(f"{args.parts[0]} has no orthophoto: the registration reads both orthophotos (predict_video.py --ortho)")
    merged = []
    for path in args.parts[1:]:
        part = read_mosaic_part(path, "cuda")
        if part["rgba"] is None or tuple(part["votes"].shape[:1]) != tuple(mine["votes"].shape[:1]):
            raise SystemExit(f"{path} has no orthophoto or another number of classes than {args.parts[0]}")
        merged.append(merge_part(mine, part, place=None if args.search_scale is None else dict(scale=args.search_scale)))
    links = torch.stack([m[0] for m in merged]).cpu().numpy()     # the read-backs happen here, after everything is enqueued
    outs, counts = [m[1].cpu().numpy() for m in merged], torch.stack([m[2] for m in merged]).cpu().numpy()
    cls = ops.mosaic_resolve(mine["votes"])[0]
    rgb = colorize(cls, PALETTE).cpu().numpy()
    rgb[cls.cpu().numpy() == 255] = 0
    Image.fromarray(rgb).save(args.out)
    if args.ortho:
        Image.fromarray(ops.ortho_compose(mine["rgba"], cls, PALETTE).cpu().numpy()).save(args.ortho)
    if args.report:
        write_merge_csv(args.report, [os.path.basename(p) for p in args.parts[1:]], (links, outs, counts))
    for path, link, count in zip(args.parts[1:], links.tolist(), counts.tolist()):
        status = LINK_STATUS[link[12]] if 0 <= link[12] < len(LINK_STATUS) else "out_of_bounds"
        print(f"{os.path.basename(path)}: {status}; shift ({link[2] / (1 << 20):.2f}, {link[5] / (1 << 20):.2f}) px; {count[2]} pixels received {count[3]} votes, "
              f"{count[4]} orthophoto pixels taken" + ("" if link[12] == 0 else " -- NOT MERGED"))


if __name__ == "__main__":
    main()
