"""Which buildings of a flood mosaic can still be reached over ground that is not under water:

    python tools/mosaic_access.py PART.npz [--csv REGIONS.csv] [--png FIELD.png] [--routes ROUTES.geojson]
                                  [--seed-point X Y ...] [--seed-class K ...] [--seed-border] [--cost K=COST ...] [--terminal K ...]
                                  [--min-votes N] [--connectivity 4|8] [--max-cost R] [--max-rounds N] [--max-regions N]

PART is a mosaic part, what `tools/predict_video.py --mosaic-part FILE.npz` (or flow.mosaic.write_mosaic_part) wrote.  Its class plane
is resolved (a pixel with fewer than --min-votes votes counts as never seen, and unseen ground is a barrier), the seeds are the canvas
pixels --seed-point names, every pixel of the --seed-class classes and/or (the default without either) the border of the seen area,
and the cheapest route from any seed to every pixel is computed on the GPU: a move to a neighbour costs 5 (straight) or 7 (diagonal)
times the sum of the two pixels' class costs, by default Street 1, Background 2, Tree 6, Building 2, Water 0 = barrier; the --terminal
classes (by default 3, Building) are arrived at but never crossed.  --csv has one row per connected region: class, area, centroid,
reached or cut_off, and for a reached one the route's cost, where it arrives, and the seed it starts from; --png the cost field as a
ramp over the class colours with the cut-off buildings highlighted; --routes one LineString per reached building.  Costs are tenths of
a mask pixel of the anchor frame, not metres.  The default costs and the round limit are guesses, not validated on real video."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flood_uav_video_segmentation_amd import ops  # noqa: E402
from flood_uav_video_segmentation_amd.flow.mosaic import (ACCESS_MAX_ROUNDS, access_report, mosaic_access, read_mosaic_part, write_access_csv,  # noqa: E402
                                                          write_access_geojson, write_access_png)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", metavar="PART.npz", help="the mosaic part")
    ap.add_argument("--csv", default=None, metavar="FILE.csv", help="one row per region: class, area, centroid, reached or cut off, route cost, origin")
    ap.add_argument("--png", default=None, metavar="FILE.png", help="the cost field over the class colours, cut-off buildings highlighted")
    ap.add_argument("--routes", default=None, metavar="FILE.geojson", help="one LineString per reached region of a terminal class")
    ap.add_argument("--seed-point", type=int, nargs=2, action="append", default=None, metavar=("X", "Y"), help="a canvas pixel routes start from (repeatable)")
    ap.add_argument("--seed-class", type=int, nargs="+", default=None, metavar="K", help="every pixel of these classes is a seed")
    ap.add_argument("--seed-border", action="store_true", help="the border of the seen area is a seed (the default without another seed)")
    ap.add_argument("--cost", nargs="+", default=None, metavar="K=COST", help="the walking cost of class K, 0..255, 0 = barrier; classes not named are barriers")
    ap.add_argument("--terminal", type=int, nargs="*", default=[3], metavar="K", help="classes that are arrived at but never crossed")
    ap.add_argument("--min-votes", type=int, default=1, metavar="N", help="a pixel with fewer votes counts as never seen (1..65535)")
    ap.add_argument("--connectivity", type=int, default=8, help="4 or 8")
    ap.add_argument("--max-cost", type=int, default=0, metavar="R", help="routes that cost more are not reported (0: no bound)")
    ap.add_argument("--max-rounds", type=int, default=ACCESS_MAX_ROUNDS, metavar="N", help="give up after N rounds: the result is then flagged as not converged")
    ap.add_argument("--max-regions", type=int, default=1024, metavar="N", help="rows of the region table (1..65536)")
    args = ap.parse_args(argv)
    if not (args.csv or args.png or args.routes):
        ap.error("nothing to write: give --csv, --png or --routes")
    if args.connectivity not in (4, 8):
        ap.error("--connectivity takes 4 or 8")
    if args.cost is not None:
        table = {}
        for item in args.cost:
            k, sep, c = item.partition("=")
            if not sep or not k.isdigit() or not c.isdigit():
                ap.error(f"--cost takes K=COST pairs, got {item!r}")
            if not 0 <= int(k) <= 31 or not 0 <= int(c) <= 255:
                ap.error(f"--cost takes class ids 0..31 and costs 0..255, got {item!r}")
            table[int(k)] = int(c)
        args.cost = table
    if not 1 <= args.min_votes <= 65535:
        ap.error("--min-votes takes 1..65535")
    if not 0 <= args.max_cost <= ops.ACCESS_MAX_COST:
        ap.error(f"--max-cost takes 0..{ops.ACCESS_MAX_COST}")
    if args.max_rounds < 1:
        ap.error("--max-rounds takes at least 1")
    if not 1 <= args.max_regions <= 65536:
        ap.error("--max-regions takes 1..65536")
    args.seed_border = args.seed_border or (args.seed_point is None and args.seed_class is None)
    return args


def seed_spec(args):
    spec = {}
    if args.seed_point:
        spec["points"] = [tuple(p) for p in args.seed_point]
    if args.seed_class:
        spec["classes"] = list(args.seed_class)
    if args.seed_border:
        spec["border"] = True
    return spec


def main(argv=None):
    args = parse_args(argv)
    torch.set_grad_enabled(False)
    part = read_mosaic_part(args.part, "cuda")
    result = mosaic_access(part, seeds=seed_spec(args), cost=args.cost, terminal=args.terminal, min_votes=args.min_votes, connectivity=args.connectivity,
                           max_cost=args.max_cost, max_rounds=args.max_rounds, max_regions=args.max_regions)
    report = access_report(result)
    if args.csv:
        write_access_csv(args.csv, report)
    if args.png:
        write_access_png(args.png, report)
    if args.routes and report["converged"]:
        write_access_geojson(args.routes, report)
    kinds = [(int(t[0]) in report["terminal"], int(a[0]) >= 0) for t, a in zip(report["table"], report["rows"])]
    print(f"{os.path.basename(args.part)}: {int(report['status'][2])} pixels reached in {report['rounds']} rounds; "
          f"{sum(t and r for t, r in kinds)} terminal regions reached, {sum(t and not r for t, r in kinds)} cut off"
          + ("" if report["converged"] else f" -- NOT CONVERGED within {report['rounds']} rounds: costs are upper bounds, no routes written"))


if __name__ == "__main__":
    main()
