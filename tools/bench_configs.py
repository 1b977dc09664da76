#!/usr/bin/env python3
"""FPS of every BASELINE.json config on ONE MI355X (secondary numbers for DESIGN.md; bench.py is the headline).
All fp32, synthetic weights/frames, inputs resident in HBM, uint8 masks copied to the host each step.

    python tools/bench_configs.py                 # all rows
    python tools/bench_configs.py --only cfg2     # one config (cfg0 cfg1 cfg4 feat motion ingest cuts conf regions tracks outlines simplify overlay cfg2 cfg3 vitb) -- the command that
                                                  # `rocprofv3 --kernel-trace --stats` wraps for profiles/r02_cfg*_kernel_stats.csv
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flood_uav_video_segmentation_amd import ops, synth  # noqa: E402
from flood_uav_video_segmentation_amd.flow.model import FlowModel  # noqa: E402
from flood_uav_video_segmentation_amd.model.deeplabv3 import FlowDeepLabv3  # noqa: E402
from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet  # noqa: E402
from flood_uav_video_segmentation_amd.model.vit import VITSegmentModel  # noqa: E402

torch.set_grad_enabled(False)
N = 5


class HP:
    OPTIONS = ()   # --opt words: hip_* attributes of the reference-style hparams (model/hipnet.py::hip_options)

    def __init__(self, layers):
        self.layers, self.classes, self.pretrained = layers, 5, False
        for word in HP.OPTIONS:  # NAME or NAME=INT
            name, _, val = word.partition("=")
            setattr(self, name, int(val) if val else True)


def timeit(fn, steps=10, warmup=2):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _bench_lib():
    from flood_uav_video_segmentation_amd import _lib
    return _lib.load()


def _check(rc):
    from flood_uav_video_segmentation_amd import _lib
    _lib.check(rc)


def _ptr(t):
    from flood_uav_video_segmentation_amd import _lib
    return _lib.ptr(t)


def _stream():
    from flood_uav_video_segmentation_amd import _lib
    return _lib.stream_ptr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="cfg0 | cfg1 | cfg4 | feat | crops | crops_cached | ms1 | ms6 | motion | ingest | cuts | conf | regions | tracks | outlines | simplify | overlay | cfg2 | cfg3 | vitb")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--opt", action="append", default=[], help="hip_no_split_bf16 | hip_no_winograd | hip_winograd_tile=4 | ... (repeatable; model/hipnet.py::HIP_OPTIONS)")
    ap.add_argument("--lib", default=None, help="development A/B: load this build of the library instead of the in-tree one")
    ap.add_argument("--vit-two-step", action="store_true", help="A/B: the Segmenter's upsample, unpadding and argmax as separate steps (cfg3)")
    ap.add_argument("--feat-op-by-op", action="store_true", help="A/B: predict_feature's tail op by op instead of fs_feat_tail (feat, cfg3)")
    ap.add_argument("--json", action="store_true", help="also print one JSON line {value, unit, ms_per_step, steps} of the last config run")
    args = ap.parse_args()
    HP.OPTIONS = tuple(args.opt)
    if args.lib:
        from flood_uav_video_segmentation_amd import _lib
        _lib.LIB_PATH, _lib.ALLOW_MISSING = os.path.abspath(args.lib), True
    want = lambda k: not args.only or args.only == k  # noqa: E731
    dev = "cuda"
    host = torch.empty((N, 713, 713), dtype=torch.uint8).pin_memory()
    rows = []
    keys = synth.make_clip(21, 713, seed=1000, only=[0, 5, 10, 15, 20]).to(dev)
    dl, dr = [[g.to(dev) for g in gs] for gs in synth.dummy_grids(N)]
    wl, wr = [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 44, 44, seed=2000)]

    def window(fm, grids):
        fm.fused_feature_tail = not args.feat_op_by_op

        def step(i):
            r = fm.predict(keys[i % 4:i % 4 + 1], keys[i % 4 + 1:i % 4 + 2], grids[0], grids[1], N, None, with_mask=True)
            host.copy_(r["mask"], non_blocking=True)  # logits AND masks are produced; the masks go to the host
            torch.cuda.current_stream().synchronize()
        return step

    psp = None
    if any(want(k) for k in ("cfg0", "cfg1", "cfg4", "feat", "crops", "crops_cached", "ms1", "ms6", "motion")):
        psp = FlowPSPNet(HP(50)).eval()
        psp.load_state_dict(synth.make_pspnet_state(50, 5, 0))

    def single(i):  # configs[0] semantics on the GPU: one frame per step, PSPNet.forward + argmax
        lo = psp.segment(keys[i % 5:i % 5 + 1])
        _, mask = ops.seg_tail(lo, None, [], [], 1, (713, 713), True, want_logits=False, want_mask=True)
        host[:1].copy_(mask, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    st = args.steps
    if want("cfg0"):
        t = timeit(single, st)
        rows.append(("configs[0] PSPNet-R50 single-frame (GPU)", 1 / t, t * 1e3))
    if want("cfg1"):
        t = timeit(window(FlowModel(psp, feature_based=False, no_warp=True).eval(), (dl, dr)), st)
        rows.append(("configs[1] PSPNet-R50 keyframe + linear interp", N / t, t * 1e3))
    if want("cfg4"):
        t = timeit(window(FlowModel(psp, feature_based=False, no_warp=False).eval(), (wl, wr)), st)
        rows.append(("configs[4]/1GPU PSPNet-R50 keyframe + logit warp", N / t, t * 1e3))
    if want("feat"):
        t = timeit(window(FlowModel(psp, feature_based=True, no_warp=False).eval(), (wl, wr)), steps=max(1, st // 2))
        rows.append(("(extra) PSPNet-R50 keyframe + FEATURE warp", N / t, t * 1e3))
    for cached in (False, True):
        if not want("crops_cached" if cached else "crops"):
            continue
        # the reference's default real-video route (flow/base.py:182-209): 1072x1920 frames, 8 overlapping 713x713 crops of both key
        # frames, warp, float64 canvas, masks at 1072x1920 (bench.py's fps_real_video_route_* variants, on their own for rocprofv3)
        from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor
        hd = synth.make_clip(16, (1072, 1920), seed=1200, only=[0, 5, 10, 15]).to(dev)
        gl, gr = [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2100, frame=(1072, 1920), jitter=0.01)]
        pred = FlowPredictor(FlowModel(psp, feature_based=False, no_warp=False).eval(), 5, (1072, 1920), crop=(713, 713), compute_metrics=False,
                             cache_keyframes=cached)
        psp.reserve(16, 713, 713)
        host_hd = torch.empty((N, 1072, 1920), dtype=torch.uint8).pin_memory()

        def crops_step(i, pred=pred, cached=cached):
            w = i % 3
            if cached and w == 0:
                pred.reset()
            host_hd.copy_(pred.predict_window(hd[w:w + 1], hd[w + 1:w + 2], gl, gr, to_host=False, key_ids=(5 * w, 5 * w + 5) if cached else None),
                          non_blocking=True)
            torch.cuda.current_stream().synchronize()
        t = timeit(crops_step, steps=max(3, st))
        rows.append(("(reference default route) 1072x1920, 8 crops x 2 key frames, warp" + (", key-frame cache" if cached else ""), N / t, t * 1e3))
        del pred, hd
    for key, scales in (("ms1", [1.0]), ("ms6", [0.5, 0.75, 1.0, 1.25, 1.5, 1.75])):
        if not want(key):
            continue
        # the single-frame multi-scale test (base/foundation.py:177-221): 1080 x 1920, 713 x 713 crops, every crop with its flip
        from flood_uav_video_segmentation_amd.base.foundation import SingleFrameEvaluator, crop_windows, mean, scaled_size, std
        ev = SingleFrameEvaluator(psp, 5, 713, 713, test_scales=scales, crop_batch=8)
        raw = (synth.make_clip(1, (1080, 1920), seed=1300)[0] * torch.tensor(std)[:, None, None] + torch.tensor(mean)[:, None, None]).clamp(0, 255).to(dev)
        host_ms = torch.empty((1080, 1920), dtype=torch.uint8).pin_memory()

        def ms_step(i, ev=ev, raw=raw):
            host_ms.copy_(ev.predict(raw)[1], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        t = timeit(ms_step, steps=max(3, st // 2))
        # the same frame without the network: the new kernels on held logits, and the per-crop composition of existing ops they replace
        geo = []
        for sc in scales:
            nh, nw = scaled_size(1080, 1920, sc)
            ph, pw = max(nh, 713), max(nw, 713)
            wins = crop_windows(ph, pw, 713, 713)
            geo.append((nh, nw, ph, pw, wins, torch.randn((2, len(wins), 5, 90, 90), device=dev)))
        canvas = torch.zeros((1, 5, 2016, 3584), dtype=torch.float64, device=dev)
        count = torch.zeros((2016, 3584), dtype=torch.float64, device=dev)
        lib = _bench_lib()

        def new_kernels(i):
            pred = None
            for j, (nh, nw, ph, pw, wins, lo) in enumerate(geo):
                ops.ms_prepare(raw, (nh, nw), (ph, pw), mean, std)
                pred = ops.ms_fuse(lo[0], lo[1], wins, (713, 713), (ph, pw), (nh, nw), pred=pred, frame_hw=(1080, 1920), scale_index=j,
                                   nscales=len(geo), want_mask=True)[1]

        def old_composition(i):  # upsample + softmax-accumulate per crop and flip (no un-flip, no averaging, no resize back: a lower bound)
            for nh, nw, ph, pw, wins, lo in geo:
                for half in range(2):
                    for c, (y, x) in enumerate(wins):
                        up = ops.resize_bilinear(lo[half, c:c + 1], (713, 713), align_corners=True)
                        _check(lib.fs_softmax_accumulate(_ptr(up), 1, 5, 713, 713, _ptr(canvas), _ptr(count), ph, pw, y, x, _stream()))
        t_new, t_old = timeit(new_kernels, steps=max(3, st // 2)), timeit(old_composition, steps=max(3, st // 2))
        rows.append((f"single-frame multi-scale test 1080x1920, 713 crops + flips, {len(scales)} scale(s)", 1 / t, t * 1e3))
        rows.append((f"  new kernels alone (prepare + fuse + accumulate): {100 * t_new / t:.1f} % of the frame", 1 / t_new, t_new * 1e3))
        rows.append(("  existing ops per crop and flip (resize + softmax_accumulate only)", 1 / t_old, t_old * 1e3))
        del ev, geo, canvas, count
    if want("motion"):
        # block motion estimation (csrc/motion_ops.hip, flow/motion.py): one 1080 x 1920 frame pair per call, every loop >= 0.5 s; a
        # full search does the same work whatever the frames hold.  Beside it the window that consumes four pairs' grids.
        from flood_uav_video_segmentation_amd.flow import motion
        gen = torch.Generator().manual_seed(1400)
        rgb = [torch.randint(0, 256, (1080, 1920, 3), generator=gen, dtype=torch.uint8).to(dev) for _ in range(2)]
        luma = [f[..., 1].contiguous() for f in rgb]

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)
        pairs_ms = {}
        for search in (8, 16, 32):
            for name, (a, b) in (("luma", luma), ("RGB", rgb)):
                t = timed(lambda i, a=a, b=b, search=search: ops.block_match(a, b, search=search))
                rows.append((f"block_match 1080x1920 R={search:2d} {name} input (pairs/s)", 1 / t, t * 1e3))
                # the same search with the intra / scene-cut decisions and the finishing pass, alternating with block_match on the same
                # frames (three rounds each, the fastest of each side: the difference is a few microseconds)
                alt = [(timed(lambda i, a=a, b=b, search=search: ops.block_match(a, b, search=search)),
                        timed(lambda i, a=a, b=b, search=search: ops.block_match_modes(a, b, search=search, intra_bias=0, scene_cut=0.5,
                                                                                       return_activity=True, return_stats=True)))
                       for _ in range(3)]
                t_old, t_new = min(x[0] for x in alt), min(x[1] for x in alt)
                rows.append((f"  block_match_modes (bias 0, cut 0.5, activity + stats) R={search:2d} {name}: +{(t_new - t_old) * 1e6:.1f} us on "
                             f"block_match's {t_old * 1e6:.1f} us beside it", 1 / t_new, t_new * 1e3))
                t = timed(lambda i, a=a, b=b, search=search: motion.estimate_grids(a, b, search=search))
                rows.append((f"  estimate_grids (matcher + grid producer) R={search:2d} {name}", 1 / t, t * 1e3))
                pairs_ms[(search, name)] = t * 1e3
        # the yardstick for "one short launch": block_match on a one-block frame (one workgroup, one candidate) through the same wrapper
        tiny = [f[:16, :16].contiguous() for f in luma]
        t = timed(lambda i: ops.block_match(tiny[0], tiny[1], search=1))
        rows.append(("  near-empty launch beside them (block_match on a 16x16 frame, same wrapper)", 1 / t, t * 1e3))
        fm = FlowModel(psp, feature_based=False, no_warp=False).eval()
        t_win = timeit(window(fm, (wl, wr)), st)
        lows = psp.segment(keys[0:1], keys[1:2])
        t_tail = timed(lambda i: ops.seg_tail(lows[0:1], lows[1:2], wl, wr, N, (713, 713), False, want_logits=True, want_mask=True))
        rows.append(("warp window 713x713 (configs[1] geometry, logit warp), frames/s", N / t_win, t_win * 1e3))
        rows.append(("  its seg tail alone (warp + blend + upsample + argmax on held logits)", 1 / t_tail, t_tail * 1e3))
        for search in (8, 16, 32):
            four = 4 * pairs_ms[(search, "RGB")]
            rows.append((f"  four RGB pairs' grids at R={search}: {100 * four / (t_win * 1e3):.2f} % of the window, {four / (t_tail * 1e3):.2f} x its seg tail",
                         1e3 / four, four))
    if want("ingest"):
        # frame ingest (csrc/ingest_ops.hip, ops.prepare_frame): one decoded 1080 x 1920 uint8 frame -> the network's input, against the
        # chain flow/dataset.py ran before the op existed (restated here as the A/B baseline), on the same frames, alternating, every
        # loop >= 0.5 s.  Bytes per frame: what the op must read and write once.
        import tempfile

        import numpy as np
        from flood_uav_video_segmentation_amd.flow.dataset import MEAN, STD, PredictWindows
        gen = torch.Generator().manual_seed(1500)
        rgb1080 = [torch.randint(0, 256, (1080, 1920, 3), generator=gen, dtype=torch.uint8).to(dev) for _ in range(2)]
        rgb1072 = [f[:1072].contiguous() for f in rgb1080]
        ys = [f[..., 1].contiguous() for f in rgb1080]
        uvs = [f[::2, ::2, :2].contiguous() for f in rgb1080]
        out = torch.empty((2, 3, 1072, 1920), dtype=torch.float32, device=dev)

        def old_chain(img, size):  # PredictWindows._frame before ops.prepare_frame: six passes and two synchronous host-to-device copies
            x = img.permute(2, 0, 1)[None].float()
            if size is not None and tuple(x.shape[2:]) != tuple(size):
                x = ops.resize_bilinear(x, size, align_corners=False).round_().clamp_(0, 255)
            mean = torch.tensor(MEAN, device=img.device).view(1, 3, 1, 1)
            std = torch.tensor(STD, device=img.device).view(1, 3, 1, 1)
            return (x - mean) / std

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)
        size = (1072, 1920)
        cases = [("RGB24 1080 -> 1072 rows", lambda i: ops.prepare_frame(rgb1080[i % 2], size, out=out[i % 2]), lambda i: old_chain(rgb1080[i % 2], size), 1080 * 1920 * 3),
                 ("RGB24 native 1072 rows", lambda i: ops.prepare_frame(rgb1072[i % 2], size, out=out[i % 2]), lambda i: old_chain(rgb1072[i % 2], size), 1072 * 1920 * 3),
                 ("NV12 1080 -> 1072 rows", lambda i: ops.prepare_frame(ys[i % 2], size, fmt="nv12", chroma=uvs[i % 2], matrix="bt709", out=out[i % 2]), None,
                  1080 * 1920 * 3 // 2)]
        for name, new_fn, old_fn, read_bytes in cases:
            assert old_fn is None or torch.equal(new_fn(0).view(1, 3, 1072, 1920), old_fn(0))
            t_new = [timed(new_fn)]
            t_old = [timed(old_fn)] if old_fn else []
            t_new.append(timed(new_fn))      # alternating: new, old, new, old
            if old_fn:
                t_old.append(timed(old_fn))
            tn = min(t_new)
            moved = read_bytes + 3 * 1072 * 1920 * 4
            rows.append((f"prepare_frame {name}: {moved / 1e6:.1f} MB, {moved / tn / 1e12:.2f} TB/s (host clock)", 1 / tn, tn * 1e3))
            if old_fn:
                to = min(t_old)
                rows.append((f"  the torch chain it replaces (same frames, same call): {to / tn:.1f} x the time", 1 / to, to * 1e3))
        # one PredictWindows item with grids="estimate" from a synthetic image folder, with and without the shared decode (HOST-bound:
        # PIL decodes on the CPU; the figure shows decodes saved, not GPU time)
        with tempfile.TemporaryDirectory() as root:
            from PIL import Image
            folder = os.path.join(root, "frames", "clip", "images")
            os.makedirs(folder)
            rng = np.random.RandomState(3)
            base = (synth.make_clip(1, (1080 + 64, 1920 + 64), seed=1501)[0] * 50 + 120).clamp(0, 255).byte().permute(1, 2, 0).numpy()
            for i in range(11):
                Image.fromarray(np.ascontiguousarray(base[2 * i:2 * i + 1080, 3 * i:3 * i + 1920])).save(os.path.join(folder, f"{i}.jpg"), quality=90)
            del rng

            class TwiceDecoded(PredictWindows):  # the parent's behaviour: _frame and raw_frame each decode and upload
                def _decoded(self, f_id):
                    return self._decode(f_id)

            for label, cls in (("shared decode", PredictWindows), ("every use decodes (parent)", TwiceDecoded)):
                def item_step(i, cls=cls):
                    ds = cls(root, "clip", frame_delta=5, size=size, grids="estimate")   # a fresh dataset: nothing cached across steps
                    ds[i % 2]
                    torch.cuda.current_stream().synchronize()
                t = timeit(item_step, steps=6, warmup=2)
                rows.append((f"PredictWindows item, grids=estimate, JPEG folder (host-bound), {label}", 1 / t, t * 1e3))
    if want("conf"):
        # per-pixel confidence and the extent report (ops.mask_confidence / canvas_confidence / frame_report, csrc/conf_ops.hip): what the
        # opt-in costs behind each tail, on the same held logits, alternating (three rounds each, the fastest of each side), every loop
        # >= 0.5 s.  Whole frame: the masks-only tail against logits + mask_confidence + frame_report; sliding crops: crops_fuse
        # masks-only against canvas + canvas_confidence + frame_report.  Then the three kernels alone with their achieved bytes / s.
        from flood_uav_video_segmentation_amd.flow.crops import crop_windows
        gen = torch.Generator().manual_seed(1700)

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)

        def ab(label, old, new):
            alt = [(timed(old), timed(new)) for _ in range(3)]
            t_old, t_new = (min(x[j] for x in alt) for j in range(2))
            rows.append((f"{label}, masks only", 1 / t_old, t_old * 1e3))
            rows.append((f"  + confidence + report: {(t_new / t_old - 1) * 100:+.2f} % ({(t_new - t_old) * 1e3:+.3f} ms)", 1 / t_new, t_new * 1e3))

        def alone(label, fn, nbytes):
            t = min(timed(fn) for _ in range(3))
            rows.append((f"  {label}: {nbytes / 1e6:.1f} MB, {nbytes / t / 1e12:.2f} TB/s", 1 / t, t * 1e3))

        for (hh, ww), hg in (((713, 713), 44), ((1072, 1920), None)):
            lo = torch.randn((2, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            gl, gr = (wl, wr) if hg else [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2001, frame=(hh, ww))]
            report = torch.empty((N, 5, 3), dtype=torch.int64, device=dev)

            def with_conf(i, lo=lo, gl=gl, gr=gr, no_warp=False, hh=hh, ww=ww, report=report):
                logits, _ = ops.seg_tail(lo[0:1], lo[1:2], gl, gr, N, (hh, ww), no_warp, want_logits=True)
                mask, conf = ops.mask_confidence(logits)
                ops.frame_report(mask, conf, 5, 128, out=report)
            for no_warp in (False, True):
                ab(f"seg_tail {hh}x{ww} {'no_warp' if no_warp else 'warp'}",
                   lambda i, lo=lo, gl=gl, gr=gr, no_warp=no_warp, hh=hh, ww=ww: ops.seg_tail(lo[0:1], lo[1:2], gl, gr, N, (hh, ww), no_warp, want_logits=False,
                                                                                         want_mask=True),
                   lambda i, f=with_conf, no_warp=no_warp: f(i, no_warp=no_warp))
            logits = torch.randn((N, 5, hh, ww), generator=gen).to(dev) * 3
            mask, conf = ops.mask_confidence(logits)
            alone(f"mask_confidence {hh}x{ww} n {N} K 5", lambda i, x=logits: ops.mask_confidence(x), logits.numel() * 4 + 2 * mask.numel())
            alone(f"frame_report {hh}x{ww} n {N} K 5", lambda i, m=mask, c=conf, r=report: ops.frame_report(m, c, 5, 128, out=r), 2 * mask.numel())
            canvas = torch.softmax(logits.double(), 1)
            alone(f"canvas_confidence {hh}x{ww} n {N} K 5", lambda i, x=canvas: ops.canvas_confidence(x), canvas.numel() * 8 + 2 * mask.numel())
            del logits, canvas
        wins = crop_windows(1072, 1920, 713, 713)
        yx = [(y, x) for (y, _, x, _) in wins]
        lo_c = torch.randn((2, len(yx), 5, 90, 90), generator=gen).to(dev)
        g1080 = [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2002, frame=(1072, 1920))]
        cg = ops.crop_grids(g1080[0] + g1080[1], (1072, 1920), yx, (713, 713))
        report = torch.empty((N, 5, 3), dtype=torch.int64, device=dev)

        def crops_conf(i, no_warp):
            canvas, _ = ops.crops_fuse(lo_c[0], lo_c[1], None if no_warp else cg, yx, (713, 713), N, no_warp, (1072, 1920), want_canvas=True)
            mask, conf = ops.canvas_confidence(canvas)
            ops.frame_report(mask, conf, 5, 128, out=report)
        for no_warp in (False, True):
            ab(f"crops_fuse 1072x1920, {len(yx)} crops of 713x713, {'no_warp' if no_warp else 'warp'}",
               lambda i, no_warp=no_warp: ops.crops_fuse(lo_c[0], lo_c[1], None if no_warp else cg, yx, (713, 713), N, no_warp, (1072, 1920),
                                                         want_canvas=False, want_mask=True),
               lambda i, no_warp=no_warp: crops_conf(i, no_warp))
    if want("regions"):
        # connected regions (ops.mask_regions / region_table / region_filter, csrc/region_ops.hip): each op alone at the two geometries
        # on masks of a blob-like scene (the argmax of smooth random logits: a few large regions and many small ones) with the bytes
        # each must move at least -- at the default cap of 1024 rows, which these scenes overflow (most regions get no row, no table
        # atomics and no votes), and at a cap of 32768 that holds every region -- then what the opt-in adds to a window: the masks-only tail against the tail + label + table
        # (regions=True) and against label + table + filter + label + table (min_region_area=9), alternating, every loop >= 0.5 s.
        gen = torch.Generator().manual_seed(1800)

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)

        def alone(label, fn, nbytes):
            t = min(timed(fn) for _ in range(3))
            rows.append((f"  {label}: {nbytes / 1e6:.1f} MB, {nbytes / t / 1e12:.3f} TB/s", 1 / t, t * 1e3))

        def regions_of(mask, conf, cap=1024):
            labels = ops.mask_regions(mask, 5, 8)
            return ops.region_table(mask, labels, 5, conf, 128, cap)

        def despeckled(mask, conf):
            table, _, index = regions_of(mask, None)
            out = ops.region_filter(mask, index, table, 5, 9)
            return regions_of(out, conf)

        for (hh, ww), hg in (((713, 713), 44), ((1072, 1920), None)):
            low = torch.randn((N, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            mask, conf = ops.mask_confidence(low, (hh, ww))
            px = mask.numel()
            labels = ops.mask_regions(mask, 5, 8)
            table, counts, index = ops.region_table(mask, labels, 5, conf, 128, 1024)
            rows.append((f"regions {hh}x{ww} n {N} K 5: {counts[:, 0].tolist()} regions per frame", 0.0, 0.0))
            alone(f"mask_regions {hh}x{ww} n {N} K 5 (8)", lambda i, m=mask: ops.mask_regions(m, 5, 8), px * (1 + 4 + 4 + 4))
            for cap in (1024, 32768):
                table, counts, index = ops.region_table(mask, labels, 5, conf, 128, cap)
                alone(f"region_table {hh}x{ww} n {N} K 5 + conf, cap {cap}", lambda i, m=mask, l=labels, c=conf, cap=cap: ops.region_table(m, l, 5, c, 128, cap),
                      px * (4 + 4 + 4 + 4 + 1 + 4) + N * cap * 80)
                alone(f"region_filter {hh}x{ww} n {N} K 5 min 9, cap {cap}", lambda i, m=mask, x=index, t=table: ops.region_filter(m, x, t, 5, 9),
                      px * (4 + 4 + 1 + 1) + N * cap * 5 * 4)
            lo = torch.randn((2, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            gl, gr = (wl, wr) if hg else [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2001, frame=(hh, ww))]

            def tail(i, lo=lo, gl=gl, gr=gr, hh=hh, ww=ww):
                return ops.seg_tail(lo[0:1], lo[1:2], gl, gr, N, (hh, ww), False, want_logits=False, want_mask=True)[1]
            alt = [(timed(tail), timed(lambda i: regions_of(tail(i), None)), timed(lambda i: despeckled(tail(i), None)),
                    timed(lambda i: regions_of(tail(i), None, 32768))) for _ in range(3)]
            t_old, t_reg, t_flt, t_big = (min(x[j] for x in alt) for j in range(4))
            rows.append((f"seg_tail {hh}x{ww} warp, masks only", 1 / t_old, t_old * 1e3))
            rows.append((f"  + regions: {(t_reg / t_old - 1) * 100:+.2f} % ({(t_reg - t_old) * 1e3:+.3f} ms)", 1 / t_reg, t_reg * 1e3))
            rows.append((f"  + regions, max_regions 32768: {(t_big / t_old - 1) * 100:+.2f} % ({(t_big - t_old) * 1e3:+.3f} ms)", 1 / t_big, t_big * 1e3))
            rows.append((f"  + min_region_area 9 + regions: {(t_flt / t_old - 1) * 100:+.2f} % ({(t_flt - t_old) * 1e3:+.3f} ms)", 1 / t_flt, t_flt * 1e3))
    if want("outlines"):
        # region outlines (ops.region_outlines, csrc/outline_ops.hip): the op alone per call of N frames, connectivity 8, at the two
        # geometries, on the blob-like masks of the regions section (same seed, same draws: the argmax of smooth random logits) and on a
        # second scene with a few large regions (logits 64 times coarser than the mask), with caps that hold every region, contour and
        # vertex -- the totals are printed -- and with the bytes the passes must move at least: the index plane read by the marking and
        # by the compaction pass (4 B a pixel each), per node 36 B a ranking round and 92 B for the other passes, and the outputs
        # written once (zeroed).  Then what outlines=True adds to a window over regions=True alone (tail + label + table against tail +
        # label + table + outlines), alternating, every loop >= 0.5 s: at the defaults (1024 rows, 4096 contours, 32768 vertices, which
        # the blob scene overflows: the frame gets nothing) and at the caps that hold everything.
        gen = torch.Generator().manual_seed(1800)

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)

        def pow2(v):
            return 1 << max(2, int(v - 1).bit_length())

        for (hh, ww), hg in (((713, 713), 44), ((1072, 1920), None)):
            low = torch.randn((N, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            lo = torch.randn((2, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            coarse = torch.randn((N, 5, (hh - 1) // 64 + 1, (ww - 1) // 64 + 1), generator=torch.Generator().manual_seed(1801)).to(dev)
            gl, gr = (wl, wr) if hg else [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2001, frame=(hh, ww))]
            fits = {}
            for scene, logits in (("blobs", low), ("a few large regions", coarse)):
                mask = ops.mask_confidence(logits, (hh, ww))[0]
                cap = 32768
                table, counts, index = ops.region_table(mask, ops.mask_regions(mask, 5, 8), 5, None, 128, cap)
                probe = ops.region_outlines(index, cap, 8, 4, 4)[3]        # nothing fits: the counts carry the vertex totals
                mv = pow2(int(probe[:, 2].max()))
                mc = pow2(mv // 4)
                got = ops.region_outlines(index, cap, 8, mc, mv)[3]
                nodes, px = int(got[:, 2].sum()), mask.numel()
                rounds = (mv - 1).bit_length()
                floor = 8 * px + nodes * (36 * rounds + 92) + N * (48 * mc + 8 * mv + 24 * cap + 32)
                rows.append((f"outlines {hh}x{ww} n {N} (8), {scene}: regions {counts[:, 0].tolist()} of {cap}, contours {got[:, 0].tolist()} of {mc}, "
                             f"vertices {got[:, 2].tolist()} of {mv}, flags {got[:, 3].tolist()}", 0.0, 0.0))
                t = min(timed(lambda i, x=index, mc=mc, mv=mv: ops.region_outlines(x, 32768, 8, mc, mv)) for _ in range(3))
                rows.append((f"  region_outlines, {rounds} ranking rounds: floor {floor / 1e6:.1f} MB, {floor / t / 1e12:.3f} TB/s", 1 / t, t * 1e3))
                fits[scene] = (mc, mv)

            def tail(i, lo=lo, gl=gl, gr=gr, hh=hh, ww=ww):
                return ops.seg_tail(lo[0:1], lo[1:2], gl, gr, N, (hh, ww), False, want_logits=False, want_mask=True)[1]

            def regions_of(m, cap):
                return ops.region_table(m, ops.mask_regions(m, 5, 8), 5, None, 128, cap)

            def outlined(m, cap, mc, mv):
                return ops.region_outlines(regions_of(m, cap)[2], cap, 8, mc, mv)

            for cap, (mc, mv), note in ((1024, (4096, 32768), "the defaults"), (32768, fits["blobs"], "the blob scene's caps")):
                note += f", flags {outlined(tail(0), cap, mc, mv)[3][:, 3].tolist()}"
                alt = [(timed(lambda i: regions_of(tail(i), cap)), timed(lambda i: outlined(tail(i), cap, mc, mv))) for _ in range(3)]
                t_reg, t_out = (min(x[j] for x in alt) for j in range(2))
                rows.append((f"seg_tail {hh}x{ww} warp + regions, max_regions {cap}", 1 / t_reg, t_reg * 1e3))
                rows.append((f"  + outlines, max_contours {mc}, max_vertices {mv} ({note}): {(t_out / t_reg - 1) * 100:+.2f} % ({(t_out - t_reg) * 1e3:+.3f} ms)",
                             1 / t_out, t_out * 1e3))
    if want("overlay"):
        # region overlay (ops.compose_regions, csrc/overlay_ops.hip) against ops.compose_frame on the same mask, NV12 background (at the
        # frame's size) and NV12 output, at the two geometries, on the blob-like masks of the regions section (the argmax of smooth random
        # logits; at the default cap of 1024 rows, which holds the regions of the frame's top only, and at 32768, which holds all; ids = a
        # permutation of the rows): outlines alone at T = 1 and T = 4, fill alone, all three layers.  Two
        # figures per variant, alternating with compose_frame in one process, every loop >= 0.5 s, the fastest of three: the call as a
        # caller makes it (host work included: these kernels take microseconds) and the device time per call, from a captured graph of 50
        # calls replayed.  Beside each: the bytes the variant must move at least -- mask 1 B, index 4 B, background 1.5 B in, frame 1.5 B
        # out per pixel, and with labels the marks plane zeroed and read (2 B) -- and that floor over the device time.
        import numpy as np

        from flood_uav_video_segmentation_amd.flow.predict import PALETTE

        gen = torch.Generator().manual_seed(2100)

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)

        def graphed(fn, calls=50):
            fn(0)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for i in range(calls):
                    fn(i)
            return (lambda i: g.replay()), calls

        for (hh, ww), cap in (((713, 713), 1024), ((713, 713), 32768), ((1072, 1920), 1024), ((1072, 1920), 32768)):
            low = torch.randn((1, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=torch.Generator().manual_seed(2100 + hh)).to(dev)
            mask = ops.mask_confidence(low, (hh, ww))[0]
            table, counts, index = ops.region_table(mask, ops.mask_regions(mask, 5, 8), 5, None, 128, cap)
            tracks = torch.full((cap, 4), -1, dtype=torch.int64)
            tracks[:, 0] = torch.randperm(cap, generator=gen)
            tracks = tracks.to(dev)
            y = torch.randint(0, 256, (hh, ww), generator=gen, dtype=torch.uint8).to(dev)
            uv = torch.randint(0, 256, ((hh + 1) // 2, (ww + 1) // 2, 2), generator=gen, dtype=torch.uint8).to(dev)
            pal = np.concatenate([np.asarray(PALETTE, np.uint8), np.full((5, 1), 128, np.uint8)], axis=1)
            line = np.full((5, 4), 255, np.uint8)
            fill = np.asarray(ops.TRACK_PALETTE, np.uint8)
            out = torch.empty(ops.raw_frame_bytes(hh, ww, "nv12"), dtype=torch.uint8, device=dev)
            m0, i0, t0, c0 = mask[0], index[0], table[0], counts[0]
            px = hh * ww
            base_floor = px * (1 + 1.5 + 1.5)

            def plain(i):
                ops.compose_frame(m0, pal, y, uv, "nv12", "bt709", False, "nv12", out=out)

            variants = (("outline T 1", dict(outline=line, outline_width=1), 4), ("outline T 4", dict(outline=line, outline_width=4), 4),
                        ("fill", dict(fill_palette=fill, outline_width=0), 4),
                        ("outline T 2 + fill + ids x2", dict(outline=line, outline_width=2, fill_palette=fill, label_scale=2, label_min_area=256), 6))
            rows.append((f"overlay {hh}x{ww}, NV12 in and out: regions {counts[0].tolist()} of {cap}", 0.0, 0.0))
            gp, calls = graphed(plain)
            for name, style, extra in variants:
                def layered(i, style=style):
                    ops.compose_regions(m0, pal, i0, t0, c0, tracks, background=y, chroma=uv, fmt="nv12", matrix="bt709", full_range=False,
                                        out_fmt="nv12", out=out, **style)
                gl, _ = graphed(layered)
                alt = [(timed(plain), timed(layered), timed(gp) / calls, timed(gl) / calls) for _ in range(3)]
                t_old, t_new, d_old, d_new = (min(x[j] for x in alt) for j in range(4))
                floor = base_floor + extra * px
                rows.append((f"  compose_frame, call {t_old * 1e6:.1f} us; device {d_old * 1e6:.2f} us, floor {base_floor / 1e6:.1f} MB, "
                             f"{base_floor / d_old / 1e12:.2f} TB/s", 1 / d_old, d_old * 1e3))
                rows.append((f"  compose_regions {name}, call {t_new * 1e6:.1f} us; device {d_new * 1e6:.2f} us ({d_new / d_old:.2f} x, floors "
                             f"{floor / base_floor:.2f} x), floor {floor / 1e6:.1f} MB, {floor / d_new / 1e12:.2f} TB/s", 1 / d_new, d_new * 1e3))
    if want("simplify"):
        # outline simplification (ops.outline_simplify, csrc/simplify_ops.hip): the four scenes of the outlines section (same seeds, same
        # caps), outlined once; then per call of N frames the outlines alone and the simplification alone at 1 px and the default 32
        # rounds, alternating, every loop >= 0.5 s, beside the bytes the simplification must move at least: the outputs written once
        # (zeroed: 32 B a contour row, 8 B a vertex of the caps), per vertex 8 B read, 16 B of cell written and read per round it is
        # open in (taken as the frame's `rounds`, an upper bound on no vertex), and 8 B per kept vertex.  Then the kept vertices and the
        # rounds at 0.5, 1 and 2 px with 256 rounds allowed, which is what tells whether 32 are enough.
        gen = torch.Generator().manual_seed(1800)

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)

        def pow2(v):
            return 1 << max(2, int(v - 1).bit_length())

        for hh, ww in ((713, 713), (1072, 1920)):
            low = torch.randn((N, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            torch.randn((2, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen)     # the outlines section's second draw: keeps the scenes in step
            coarse = torch.randn((N, 5, (hh - 1) // 64 + 1, (ww - 1) // 64 + 1), generator=torch.Generator().manual_seed(1801)).to(dev)
            for scene, logits in (("blobs", low), ("a few large regions", coarse)):
                mask = ops.mask_confidence(logits, (hh, ww))[0]
                cap = 32768
                index = ops.region_table(mask, ops.mask_regions(mask, 5, 8), 5, None, 128, cap)[2]
                mv = pow2(int(ops.region_outlines(index, cap, 8, 4, 4)[3][:, 2].max()))
                mc = pow2(mv // 4)
                contours, vertices, _, counts = ops.region_outlines(index, cap, 8, mc, mv)
                full = int(counts[:, 2].sum())
                got = ops.outline_simplify(contours, vertices, counts, 1.0, 32)[2]
                floor = N * (32 * mc + 8 * mv + 32) + full * (8 + 16 * int(got[:, 2].max())) + 8 * int(got[:, 1].sum())
                alt = [(timed(lambda i: ops.region_outlines(index, cap, 8, mc, mv)), timed(lambda i: ops.outline_simplify(contours, vertices, counts, 1.0, 32)))
                       for _ in range(3)]
                t_out, t_smp = (min(x[j] for x in alt) for j in range(2))
                rows.append((f"simplify {hh}x{ww} n {N} (8), {scene}: {full} vertices on {counts[:, 0].tolist()} contours, caps {mc} / {mv}", 0.0, 0.0))
                rows.append(("  region_outlines alone", 1 / t_out, t_out * 1e3))
                rows.append((f"  outline_simplify 1 px, 32 rounds ({10 + 2 * 32} launches): kept {got[:, 1].tolist()}, rounds {got[:, 2].tolist()}, flags "
                             f"{got[:, 3].tolist()}; floor {floor / 1e6:.1f} MB, {floor / t_smp / 1e12:.3f} TB/s", 1 / t_smp, t_smp * 1e3))
                for tol in (0.5, 1.0, 2.0):
                    g = ops.outline_simplify(contours, vertices, counts, tol, 256)[2]
                    rows.append((f"  {tol} px, 256 rounds allowed: kept {int(g[:, 1].sum())} of {full} ({g[:, 1].tolist()}), rounds {g[:, 2].tolist()}, flags "
                                 f"{g[:, 3].tolist()}", 0.0, 0.0))
    if want("tracks"):
        # region identity across frames (ops.region_links / region_tracks, csrc/track_ops.hip): each op alone per call of N frames at the two
        # geometries on the closed-form lattice scene of the region tests (tests/regions_ref.py: disjoint 10 x 15 rectangles and one
        # serpentine; 1981 regions a frame at 713 x 713, 5361 at 1072 x 1920) moving by 3 pixels per frame, frame 0 linked to a frame
        # before it -- at a cap of 1024 rows (the scene overflows it: the lower part of the frame takes no part) and at 32768 -- with the
        # bytes each must move at least; then what track=True adds to a window over regions=True alone (tail + label + table against tail +
        # label + table + links + tracks + the copies of the last frame), alternating, every loop >= 0.5 s.
        # The motion-compensated links (ops.region_links with mv=) run beside the in-place ones, the two alternating: the same scene with
        # the uniform vector table of a 1080 x 1920 decoded frame that matches its 3 pixels per frame (-8 frame pixels at 713 wide, -3
        # at 1920), so the compensated op finds every region where it was.  Its floor is the in-place one's plus the packed shifts.  Then
        # what compensate=True adds to a window on top of track=True, and the one block search per window it costs the dataset.
        import numpy as np

        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import regions_ref
        gen = torch.Generator().manual_seed(1900)

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)

        def alone(label, fn, nbytes):
            t = min(timed(fn) for _ in range(3))
            rows.append((f"  {label}: {nbytes / 1e6:.1f} MB, {nbytes / t / 1e12:.3f} TB/s", 1 / t, t * 1e3))

        for (hh, ww), hg in (((713, 713), 44), ((1072, 1920), None)):
            plane = regions_ref.lattice_scene(1, -(-hh // 16) * 16, -(-ww // 24) * 24)[0][0]
            mask = torch.from_numpy(np.stack([np.roll(plane, 3 * f, 1)[:hh, :ww] for f in range(N + 1)])).to(dev)
            labels = ops.mask_regions(mask, 4, 8)
            px = N * hh * ww
            fh, fw, hb, wb = 1080, 1920, 67, 120
            vx = -((2 * 3 * fw + ww) // (2 * ww))                     # 3 mask pixels to the right per frame, in frame pixels, source minus destination
            by, bx = np.mgrid[0:hb, 0:wb]
            one = np.stack([np.full_like(bx, -1), np.full_like(bx, 16), np.full_like(bx, 16), bx * 16 + 8 + vx, by * 16 + 8, bx * 16 + 8, by * 16 + 8], -1)
            mv = torch.from_numpy(np.stack([one.reshape(-1, 7)] * N).astype(np.int32)).to(dev)
            for cap in (1024, 32768):
                table, counts, index = ops.region_table(mask, labels, 4, None, 128, cap)
                prev = (index[0].clone(), table[0].clone(), counts[0].clone())
                index, table, counts = index[1:].contiguous(), table[1:].contiguous(), counts[1:].contiguous()
                pairs = ops.default_max_pairs(cap)
                state = torch.zeros(2, dtype=torch.int64, device=dev)
                back, fwd, lc = ops.region_links(index, table, counts, prev)
                seed = ops.region_tracks(back, fwd, counts, state)[0].clone()  # stands for the tracks row of the frame before
                out = torch.empty((N, cap, 4), dtype=torch.int64, device=dev)
                rows.append((f"tracks {hh}x{ww} n {N} cap {cap}: rows {counts[:, 1].tolist()}, pairs / overflow {lc.tolist()} of {pairs} slots", 0.0, 0.0))
                in_place = lambda i, x=index, t=table, c=counts, p=prev: ops.region_links(x, t, c, p)  # noqa: E731
                moved = lambda i, x=index, t=table, c=counts, p=prev: ops.region_links(x, t, c, p, mv=mv, frame_size=(fh, fw))  # noqa: E731
                lc_mc = moved(0)[2]
                alt = [(timed(in_place), timed(moved)) for _ in range(3)]
                t_in, t_mc = (min(x[j] for x in alt) for j in range(2))
                floor = px * 8 + ops.region_links_workspace_bytes(N, cap, pairs) + N * cap * 16
                rows.append((f"  region_links {hh}x{ww} n {N} cap {cap}, max_pairs {pairs}: {floor / 1e6:.1f} MB, {floor / t_in / 1e12:.3f} TB/s", 1 / t_in, t_in * 1e3))
                floor += N * hb * wb * (28 + 2 * 4)                   # the table rows read once, the packed shifts written and read
                rows.append((f"  region_links compensated ({fh}x{fw} frame, vx {vx}), pairs / flags {lc_mc.tolist()}: {floor / 1e6:.1f} MB, "
                             f"{floor / t_mc / 1e12:.3f} TB/s, {t_mc / t_in:.2f} x in place", 1 / t_mc, t_mc * 1e3))
                alone(f"region_tracks n {N} cap {cap}", lambda i, b=back, f=fwd, c=counts, s=state, p=seed, o=out: ops.region_tracks(b, f, c, s, p, out=o),
                      N * cap * (16 + 32 + 32))
            lo = torch.randn((2, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            gl, gr = (wl, wr) if hg else [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2001, frame=(hh, ww))]

            def tail(i, lo=lo, gl=gl, gr=gr, hh=hh, ww=ww):
                return ops.seg_tail(lo[0:1], lo[1:2], gl, gr, N, (hh, ww), False, want_logits=False, want_mask=True)[1]

            def regions_of(m, cap):
                return ops.region_table(m, ops.mask_regions(m, 5, 8), 5, None, 128, cap)

            kept = {}

            def tracked(m, cap, mv=None):  # what FlowPredictor._keep_tracks does behind the table
                table, counts, index = regions_of(m, cap)
                key = (cap, mv is not None)
                prev, st = kept.get(key), kept.setdefault(("state",) + key, torch.zeros(2, dtype=torch.int64, device=dev))
                back, fwd, _ = ops.region_links(index, table, counts, None if prev is None else prev[:3], mv=mv, frame_size=None if mv is None else (fh, fw))
                tracks = ops.region_tracks(back, fwd, counts, st, None if prev is None else prev[3])
                kept[key] = (index[-1].clone(), table[-1].clone(), counts[-1].clone(), tracks[-1].clone())

            for cap in (1024, 32768):
                alt = [(timed(lambda i: regions_of(tail(i), cap)), timed(lambda i: tracked(tail(i), cap)), timed(lambda i: tracked(tail(i), cap, mv)))
                       for _ in range(3)]
                t_reg, t_trk, t_cmp = (min(x[j] for x in alt) for j in range(3))
                rows.append((f"seg_tail {hh}x{ww} warp + regions, max_regions {cap}", 1 / t_reg, t_reg * 1e3))
                rows.append((f"  + track: {(t_trk / t_reg - 1) * 100:+.2f} % ({(t_trk - t_reg) * 1e3:+.3f} ms)", 1 / t_trk, t_trk * 1e3))
                rows.append((f"  + track, compensate: {(t_cmp / t_reg - 1) * 100:+.2f} % ({(t_cmp - t_reg) * 1e3:+.3f} ms; {(t_cmp - t_trk) * 1e3:+.3f} ms over track)",
                             1 / t_cmp, t_cmp * 1e3))
        frames = torch.randint(0, 256, (2, 1080, 1920), generator=gen, dtype=torch.uint8).to(dev)
        for search in (16, 32):  # link_vectors=True: one more search per window, the pair that ends in the window's key frame
            t = min(timed(lambda i: ops.block_match(frames[1], frames[0], search=search)) for _ in range(3))
            rows.append((f"block_match 1080x1920 luma, search {search}: the extra search per window of link_vectors=True", 1 / t, t * 1e3))
    if want("cuts"):
        # holding one key frame across a scene cut (ops.window_weights, the weighted instantiations of the fused tails): the weighted
        # call against the unweighted one on the same held logits, alternating (three rounds each, the fastest of each side), every loop
        # >= 0.5 s; weights of a window without a cut (the same blend) and of one cut in its middle (held frames read ONE chain).  Then
        # what a window pays for its weights: one window_weights launch and the closing pair's search.
        from flood_uav_video_segmentation_amd.flow.crops import crop_windows
        gen = torch.Generator().manual_seed(1600)

        def timed(fn):
            t = timeit(fn, steps=20, warmup=5)
            return timeit(fn, steps=max(20, int(0.6 / t) + 1), warmup=0)

        def flags(cuts):
            return [torch.tensor([8040, 0, c, 0], dtype=torch.int32, device=dev) for c in cuts]
        w_none, w_cut = ops.window_weights(flags([0] * N), N)[0], ops.window_weights(flags([0, 0, 1, 0, 0]), N)[0]

        def ab(label, call):
            alt = [(timed(lambda i: call(None)), timed(lambda i: call(w_none)), timed(lambda i: call(w_cut))) for _ in range(3)]
            t_old, t_same, t_cut = (min(x[j] for x in alt) for j in range(3))
            rows.append((f"{label}, unweighted", 1 / t_old, t_old * 1e3))
            rows.append((f"  weights of a window without a cut: {(t_same / t_old - 1) * 100:+.2f} %", 1 / t_same, t_same * 1e3))
            rows.append((f"  weights of a cut at pair 3 (two frames held from each side): {(t_cut / t_old - 1) * 100:+.2f} %", 1 / t_cut, t_cut * 1e3))
        for (hh, ww), hg in (((713, 713), 44), ((1072, 1920), None)):
            lo = torch.randn((2, 5, (hh - 1) // 8 + 1, (ww - 1) // 8 + 1), generator=gen).to(dev)
            gl, gr = (wl, wr) if hg else [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2001, frame=(hh, ww))]
            for no_warp in (False, True):
                ab(f"seg_tail {hh}x{ww} {'no_warp' if no_warp else 'warp'}, logits + masks",
                   lambda w, lo=lo, gl=gl, gr=gr, no_warp=no_warp, hh=hh, ww=ww: ops.seg_tail(lo[0:1], lo[1:2], gl, gr, N, (hh, ww), no_warp, want_logits=True,
                                                                                         want_mask=True, weights=w))
        wins = crop_windows(1072, 1920, 713, 713)
        yx = [(y, x) for (y, _, x, _) in wins]
        lo_c = torch.randn((2, len(yx), 5, 90, 90), generator=gen).to(dev)
        g1080 = [[g.to(dev) for g in gs] for gs in synth.make_grids(N, 67, 120, seed=2002, frame=(1072, 1920))]
        cg = ops.crop_grids(g1080[0] + g1080[1], (1072, 1920), yx, (713, 713))
        for no_warp in (False, True):
            ab(f"crops_fuse 1072x1920, {len(yx)} crops of 713x713, {'no_warp' if no_warp else 'warp'}, masks only",
               lambda w, no_warp=no_warp: ops.crops_fuse(lo_c[0], lo_c[1], None if no_warp else cg, yx, (713, 713), N, no_warp, (1072, 1920),
                                                         want_canvas=False, want_mask=True, weights=w))
        # the feature tail (fs_feat_tail against feat_tail_weighted): PSPNet's maps at 713^2 and the Segmenter's token map, warp mode,
        # 44 x 44 grids, the 67 x 120 default grid
        from flood_uav_video_segmentation_amd.flow.model import get_default_grid
        g0 = torch.from_numpy(get_default_grid()).float().unsqueeze(0).to(dev)
        for label, C, fs in (("PSPNet", 4096, 90), ("Segmenter", 384, 45)):
            ft = [(torch.randn((1, C, fs, fs), generator=gen) * 3).to(dev).contiguous(memory_format=torch.channels_last) for _ in range(2)]
            ab(f"feat_tail {label} geometry (C {C}, {fs}x{fs} maps, 44x44 grids, n {N}), warp",
               lambda w, ft=ft: ops.feat_tail(ft[0], ft[1], wl, wr, N, False, g0, weights=w))
            del ft
        st5 = flags([0, 0, 1, 0, 0])
        t = timed(lambda i: ops.window_weights(st5, N))
        rows.append(("window_weights, n = 5 (one launch + two allocations, host clock)", 1 / t, t * 1e3))
        rgb = [torch.randint(0, 256, (1080, 1920, 3), generator=gen, dtype=torch.uint8).to(dev) for _ in range(2)]
        for search in (8, 16):
            t = timed(lambda i, search=search: ops.block_match_modes(rgb[0], rgb[1], search=search, intra_bias=0, scene_cut=0.5, return_stats=True))
            rows.append((f"the closing pair's search per window, 1080x1920 RGB R={search} (block_match_modes, stats only)", 1 / t, t * 1e3))
    del psp
    if want("cfg2"):
        dl3 = FlowDeepLabv3(HP(101)).eval()
        dl3.load_state_dict(synth.make_deeplab_state(101, 5, 0))
        t = timeit(window(FlowModel(dl3, feature_based=False, no_warp=False).eval(), (wl, wr)), st)
        rows.append(("configs[2] DeepLabv3-R101 keyframe + logit warp", N / t, t * 1e3))
        del dl3
    if want("cfg3"):
        vit = VITSegmentModel(5, 704, patch_size=16, d_model=384, n_layers=12, dec_layers=2, **{w.partition("=")[0]: (int(w.partition("=")[2]) if "=" in w else True) for w in HP.OPTIONS}).eval()
        vit.load_state_dict(synth.make_vit_state(5, 704, 16, 384, 12, 2, seed=0))
        if args.vit_two_step:
            vit.decode_fit = None  # FlowModel._decode_fit then takes decoder -> fit_output -> argmax_u8 one by one
        t = timeit(window(FlowModel(vit, feature_based=True, no_warp=False).eval(), (wl, wr)), st)
        rows.append(("configs[3] Segmenter ViT-S/16 keyframe + feature flow (extension)", N / t, t * 1e3))
        del vit
    if want("vitb"):
        vitb = VITSegmentModel(5, 704, **{w.partition("=")[0]: (int(w.partition("=")[2]) if "=" in w else True) for w in HP.OPTIONS}).eval()
        vitb.load_state_dict(synth.make_vit_state(5, 704, seed=0))

        def vit_single(i):
            out = vitb(keys[i % 5:i % 5 + 1])["pred"]
            host[:1].copy_(ops.argmax_u8(out), non_blocking=True)
            torch.cuda.current_stream().synchronize()
        t = timeit(vit_single, st)
        rows.append(("(extra) Segmenter ViT-B/32 per-frame (as model/vit.py builds it)", 1 / t, t * 1e3))
    print(f"{'config':68s} {'FPS':>9s} {'ms/step':>9s}")
    for name, fps, ms in rows:
        print(f"{name:68s} {fps:9.1f} {ms:9.4f}" if ms < 1 else f"{name:68s} {fps:9.1f} {ms:9.3f}")
    if args.json and rows:
        import json
        print(json.dumps({"config": rows[-1][0], "options": list(HP.OPTIONS), "value": round(rows[-1][1], 2), "unit": "frames/s",
                          "ms_per_step": round(rows[-1][2], 4), "steps": st}))


if __name__ == "__main__":
    main()
