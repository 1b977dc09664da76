"""FlowPredictor with every analysis stage on, on the GPU: nothing it hands out depends on how many frames a chunk of its report buffers
holds.  Two windows of the synthetic network over the shared raw clip, once with the default chunk sizes (no chunk border is reached) and
once with chunks of three and two frames (every table crosses borders inside both windows): masks, confidence and every report bit for
bit.  What the reports must contain is the business of each stage's own test; this one states that the chunking cannot be seen."""
import numpy as np
import pytest
import torch

from flood_uav_video_segmentation_amd.flow.dataset import RawVideoWindows
from flood_uav_video_segmentation_amd.flow.model import FlowModel
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor
from test_gpu_regions import DELTA, FH, FW, clip, network  # noqa: F401  (clip: the module's synthetic raw video)

pytestmark = pytest.mark.gpu


def same(a, b):
    """Equal bit for bit, through the lists and tuples the reports are made of."""
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)


def test_reports_do_not_depend_on_the_chunk_size(clip):  # noqa: F811
    size = (65, 65)
    ds = RawVideoWindows(clip, FH, FW, "rgb24", size=size, frame_delta=DELTA, grids="estimate", search=8, link_vectors=True)
    items = [ds[0], ds[1]]
    fm = FlowModel(network(), feature_based=False, no_warp=False).eval()
    kw = dict(classes=5, out_size=size, crop=None, compute_metrics=True, cache_keyframes=False, confidence=True, regions=True, min_region_area=9, track=True,
              compensate=True, outlines=True, simplify=1.0, keep_window_regions=True, stabilize=3, stabilize_trust=200, stabilize_compensate=True,
              proximity=(2, 4, 8), mosaic=(96, 120), mosaic_min_inliers=6, mosaic_exclude=())
    whole, cut = FlowPredictor(fm, **kw), FlowPredictor(fm, **kw)
    assert (whole.REPORT_CHUNK, whole.outline_chunk, whole.simple_chunk) == (256, 138, 170)
    cut.REPORT_CHUNK, cut.outline_chunk, cut.simple_chunk = 3, 2, 2                # DELTA = 5 frames a window: borders at 3, 6, 9 and at 2, 4, 6, 8
    for item in items:
        got = [p.predict_window(item["frame_prev"], item["frame_next"], item["mvs_left"], item["mvs_right"], to_host=False, link_mvs=item["link_mvs"],
                                link_frame_size=item["link_frame_size"], link_stats=item.get("link_stats")) for p in (whole, cut)]
        assert same(got[0], got[1]) and got[0][0].shape == (DELTA,) + size and same(whole.window_regions(), cut.window_regions())
    reports = [(p.extent_report(), p.stabilize_report(), p.despeckle_counts(), p.region_report(), p.track_report(with_cuts=True), p.outline_report(),
                p.simple_outline_report(), p.proximity_report(), p.mosaic_report(), p.temporal_consistency()) for p in (whole, cut)]
    for name, a, b in zip(("extent", "stabilize", "despeckle", "region", "track", "outline", "simple", "proximity", "mosaic"), *reports):
        assert same(a, b), name
    assert reports[0][-1] == reports[1][-1]
    # not vacuous: ten frames in every report, regions with tracks, outlines and simplified rings, votes on the canvas
    extent, stabilize, despeckle, (rows, totals), (tracks, _, _), (outlines, _), (simple, counts), (exposure, near), mosaic = reports[1][:9]
    assert extent.shape == (2 * DELTA, 5, 3) and stabilize.shape == (2 * DELTA, 4) and despeckle.shape == (2 * DELTA,) and exposure.shape == (2 * DELTA, 5, 3)
    assert len(rows) == len(tracks) == len(outlines) == len(simple) == len(near) == 2 * DELTA and mosaic[4].shape == (2 * DELTA, 16)
    assert min(totals) >= 2 and all(len(t) == len(r) == len(n) for t, r, n in zip(tracks, rows, near)) and all(len(o[1]) > 0 for o in outlines)
    assert counts[:, 1].min() > 0 and mosaic[2].max() >= 2
