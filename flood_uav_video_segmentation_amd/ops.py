"""Tensor-level wrappers over the C ABI (torch is only the allocator / stream provider here).

Every function enqueues on torch's current HIP stream and returns freshly allocated tensors;
inputs are never modified.  Reference ops restated: see include/floodseg.h.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, one_device, ptr, stream_ptr


def _f32c(t, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"floodseg: {name} must live on the GPU (no CPU fallback exists)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def is_channels_last_dense(t):
    """True when a logical NCHW tensor is stored pixel-major with pixel stride == C."""
    if t.dim() != 4:
        return False
    b, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    # (the stride of a size-1 dimension is arbitrary: torch keeps whatever the tensor was made with)
    return all(n == 1 or s == ws for n, s, ws in zip(t.shape, t.stride(), want)) or (c == 1 and t.is_contiguous())


def as_nhwc(t):
    """Logical NCHW tensor -> dense channels_last storage (copy only if needed)."""
    t = t if t.dtype == torch.float32 else t.float()
    if is_channels_last_dense(t):
        return t
    return t.contiguous(memory_format=torch.channels_last)


def empty_nhwc(b, c, h, w, device):
    return torch.empty((b, c, h, w), dtype=torch.float32, device=device, memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------ flow ops
def grid_sample(inp, grid, align_corners=False):
    """F.grid_sample(inp, grid, mode='bilinear', padding_mode='border') (flow/model.py:157,248)."""
    lib = _lib.load()
    b, c, hi, wi = inp.shape
    gb, hg, wg, two = grid.shape
    if two != 2 or gb != b:
        raise RuntimeError(f"floodseg.grid_sample: grid shape {tuple(grid.shape)} does not match input batch {b}")
    dev = one_device(inp, grid, what="floodseg.grid_sample")
    with torch.cuda.device(dev):
        grid = _f32c(grid, "grid")
        if b == 0:  # empty batch: nothing to launch (torch returns an empty tensor too)
            return torch.empty((0, c, hg, wg), dtype=torch.float32, device=dev)
        if inp.dim() == 4 and c % 4 == 0 and c >= 64 and is_channels_last_dense(inp):
            src = inp if inp.dtype == torch.float32 else inp.float()
            out = empty_nhwc(b, c, hg, wg, dev)
            check(lib.fs_grid_sample_nhwc(ptr(src), c, b, c, hi, wi, ptr(grid), hg, wg, ptr(out), c, int(align_corners), stream_ptr()))
            return out
        src = _f32c(inp, "input")
        out = torch.empty((b, c, hg, wg), dtype=torch.float32, device=dev)
        check(lib.fs_grid_sample_nchw(ptr(src), b, c, hi, wi, ptr(grid), hg, wg, ptr(out), int(align_corners), stream_ptr()))
        return out


def _check_out(out, shape, nhwc, what):
    """`out=`: a caller-owned destination (e.g. one image slot of a batch tensor) -- must already have the layout the op writes."""
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32:
        raise RuntimeError(f"{what}: out must be float32 {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")
    if not (is_channels_last_dense(out) if nhwc else out.is_contiguous()):
        raise RuntimeError(f"{what}: out must be dense {'channels_last' if nhwc else 'contiguous'}")
    return out


def resize_bilinear(inp, size, align_corners=True, out=None):
    """F.interpolate(inp, size, mode='bilinear', align_corners=...) (flow/model.py:42..228)."""
    lib = _lib.load()
    b, c, hi, wi = inp.shape
    ho, wo = int(size[0]), int(size[1])
    dev = one_device(inp, out, what="floodseg.resize_bilinear")
    with torch.cuda.device(dev):
        if b == 0:
            return torch.empty((0, c, ho, wo), dtype=torch.float32, device=dev)
        if c % 4 == 0 and c >= 64 and is_channels_last_dense(inp):
            src = inp if inp.dtype == torch.float32 else inp.float()
            out = empty_nhwc(b, c, ho, wo, dev) if out is None else _check_out(out, (b, c, ho, wo), True, "floodseg.resize_bilinear")
            check(lib.fs_resize_bilinear_nhwc(ptr(src), c, b, c, hi, wi, ptr(out), c, ho, wo, int(align_corners), stream_ptr()))
            return out
        src = _f32c(inp, "input")
        out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=dev) if out is None else _check_out(out, (b, c, ho, wo), False, "floodseg.resize_bilinear")
        check(lib.fs_resize_bilinear_nchw(ptr(src), b * c, hi, wi, ptr(out), ho, wo, int(align_corners), stream_ptr()))
        return out


def blend(a, wa, b=None, wb=0.0, out=None):
    """wa*a + wb*b with the reference's rounding order (flow/model.py:104,168,234-236).  out: optional destination of the
    layout the result has (channels_last when `a` is, else contiguous), e.g. one image slot of a preallocated batch."""
    lib = _lib.load()
    if b is not None and a.shape != b.shape:
        raise RuntimeError(f"floodseg.blend: shapes differ ({tuple(a.shape)} vs {tuple(b.shape)})")
    dev = one_device(a, b, out, what="floodseg.blend")
    with torch.cuda.device(dev):
        # the kernel walks both operands as flat arrays: bring BOTH to one dense layout (channels_last kept when `a` has it,
        # so the feature-mode maps are not transposed; any other view -- equal strides or not -- becomes plain contiguous)
        if is_channels_last_dense(a):
            if b is not None:
                b = as_nhwc(b)
        else:
            a = a.contiguous()
            if b is not None:
                b = b.contiguous()
        a = a if a.dtype == torch.float32 else a.float()
        if b is not None and b.dtype != torch.float32:
            b = b.float()
        out = torch.empty_like(a) if out is None else _check_out(out, a.shape, a.dim() == 4 and is_channels_last_dense(a) and not a.is_contiguous(),
                                                                 "floodseg.blend")
        if a.numel() == 0:
            return out
        check(lib.fs_blend(ptr(a), float(wa), ptr(b), float(wb), ptr(out), a.numel(), stream_ptr()))
        return out


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _window_weights_arg(weights, n, dev, what):
    """The device [n,2] float32 blend weights of window_weights, checked; None stays None (the unweighted entry point)."""
    if weights is None:
        return None
    if not weights.is_cuda or weights.device != dev:
        raise RuntimeError(f"{what}: weights must live on the tensors' device ({dev})")
    if weights.dtype != torch.float32 or tuple(weights.shape) != (int(n), 2) or not weights.is_contiguous():
        raise RuntimeError(f"{what}: weights must be a contiguous float32 [{int(n)}, 2] tensor, got {weights.dtype} {tuple(weights.shape)}")
    return weights


def window_weights(stats, n):
    """Per-frame blend weights of one key-frame window from the cut flags of its n frame pairs (definition: include/floodseg_test.h,
    window_weights).  stats: n entries, stats[j-1] = the int32 [4] stats tensor block_match_modes wrote for the pair (j-1 -> j), or
    None (not estimated: no cut).  Returns (weights float32 [n,2], source int32 [n]: 0 blended, 1 held from the previous key frame,
    2 held from the next one, 3 a scene neither key frame shows) -- device tensors from one launch; nothing is read back."""
    lib = _lib.load()
    n = int(n)
    stats = list(stats)
    if len(stats) != n:
        raise RuntimeError(f"floodseg.window_weights: need one stats entry (or None) per frame pair, got {len(stats)} for n={n}")
    if not 1 <= n <= 64:
        raise RuntimeError(f"floodseg.window_weights: n must be 1..64, got {n}")
    if any(t is not None for t in stats):
        dev = one_device(*stats, what="floodseg.window_weights")
    else:  # no pair was estimated: the linear weights, on the current device
        dev = torch.device("cuda", torch.cuda.current_device())
    for t in stats:
        if t is not None and (t.dtype != torch.int32 or t.numel() < 4 or not t.is_contiguous()):
            raise RuntimeError("floodseg.window_weights: a stats entry must be a contiguous int32 tensor of 4 values")
    with torch.cuda.device(dev):
        arr = (ctypes.c_void_p * n)()
        for i, t in enumerate(stats):
            arr[i] = None if t is None else t.data_ptr()
        weights = torch.empty((n, 2), dtype=torch.float32, device=dev)
        source = torch.empty((n,), dtype=torch.int32, device=dev)
        check(lib.fs_window_weights(n, arr, ptr(weights), ptr(source), stream_ptr()))
    return weights, source


def seg_tail(lo_prev, lo_next, grids_left, grids_right, n, out_hw, no_warp, want_logits=True, want_mask=False, weights=None):
    """Fused predict_segmentation tail (flow/model.py:184-241 after the two decoder calls).

    lo_prev/lo_next: [1,K,h,w] decoder logits; grids: lists of n-1 [1,Hg,Wg,2] tensors.
    weights: None (frame f blends the two chains with (n-f)/n and f/n), or window_weights' device [n,2] tensor: frame f >= 1 blends
    with its row, and a row with a zero HOLDS the frame -- it is the other chain's value, bit for bit.
    Returns (logits [n,K,H,W] or None, mask uint8 [n,H,W] or None).
    """
    lib = _lib.load()
    grids = [] if (lo_next is None or no_warp) else list(grids_left) + list(grids_right)
    dev = one_device(lo_prev, lo_next, *grids, what="floodseg.seg_tail")
    with torch.cuda.device(dev):
        lo_prev = _f32c(lo_prev, "lo_prev")
        _, k, h, w = lo_prev.shape
        hh, ww = out_hw
        frames = n if lo_next is not None else 1
        logits = torch.empty((frames, k, hh, ww), dtype=torch.float32, device=dev) if want_logits else None
        mask = torch.empty((frames, hh, ww), dtype=torch.uint8, device=dev) if want_mask else None
        gl = gr = None
        hg = wg = 1
        scratch = None
        keep = []
        if lo_next is not None:
            lo_next = _f32c(lo_next, "lo_next")
            if not no_warp and n > 1:  # n == 1: no grids, every frame a key frame -- the one map of lo_prev (the frame loop is empty)
                if len(grids_left) != n - 1 or len(grids_right) != n - 1:
                    raise RuntimeError("floodseg.seg_tail: need n-1 grids per direction")
                keep = [_f32c(g, "grid") for g in grids]
                hg, wg = keep[0].shape[1], keep[0].shape[2]
                for g in keep:
                    if tuple(g.shape) != (1, hg, wg, 2):
                        raise RuntimeError("floodseg.seg_tail: all grids must be [1,Hg,Wg,2] of one size")
                gl = _ptr_array(keep[: n - 1])
                gr = _ptr_array(keep[n - 1:])
                scratch = torch.empty(2 * (n - 1) * k * hg * wg, dtype=torch.float32, device=dev)
        weights = _window_weights_arg(weights, n, dev, "floodseg.seg_tail")
        if weights is None:
            check(lib.fs_seg_tail(ptr(lo_prev), ptr(lo_next), gl, gr, k, h, w, hg, wg, hh, ww, int(n), int(bool(no_warp)),
                                  ptr(logits), ptr(mask), ptr(scratch), stream_ptr()))
        else:
            check(lib.fs_seg_tail_weighted(ptr(lo_prev), ptr(lo_next), gl, gr, k, h, w, hg, wg, hh, ww, int(n), int(bool(no_warp)),
                                           ptr(logits), ptr(mask), None, None, 0, 0, 0, 0, ptr(scratch), ptr(weights), stream_ptr()))
    return logits, mask


def feat_tail(f_prev, f_next, grids_left, grids_right, n, no_warp, default_grid=None, weights=None):
    """Fused predict_feature tail (flow/model.py:131-171 between the encoder and the batched decoder call): f_prev / f_next
    [1,C,fh,fw] stored channels_last; grids: lists of n-1 [1,Hg,Wg,2]; default_grid [1,H0,W0,2] (warp mode).  Returns the decoder's
    batch [n,C,fh,fw] ([1,C,fh,fw] when f_next is None), channels_last -- bit-identical to the op-by-op route.
    weights: None (map p blends the two chains with (n-p)/n and p/n), or window_weights' device [n,2] tensor: map p >= 1 blends with
    its row, and a row with a zero HOLDS the map -- it is the other key frame's chain, bit for bit, and the unused one is not read."""
    lib = _lib.load()
    warp = not no_warp
    grids = list(grids_left) + list(grids_right) if (warp and f_next is not None) else []
    dev = one_device(f_prev, f_next, default_grid if warp else None, *grids, what="floodseg.feat_tail")
    for t in (f_prev, f_next):
        if t is not None and not (t.dim() == 4 and t.shape[0] == 1 and t.dtype == torch.float32 and is_channels_last_dense(t)):
            raise RuntimeError("floodseg.feat_tail: feature maps must be float32 [1,C,fh,fw] stored channels_last")
    _, c, fh, fw = f_prev.shape
    if c % 4 != 0:
        raise RuntimeError("floodseg.feat_tail: C must be a multiple of 4")
    if f_next is not None and f_next.shape != f_prev.shape:
        raise RuntimeError("floodseg.feat_tail: f_prev / f_next shapes differ")
    weights = _window_weights_arg(weights, n, dev, "floodseg.feat_tail")
    with torch.cuda.device(dev):
        nmaps = n if f_next is not None else 1
        stack = empty_nhwc(nmaps, c, fh, fw, dev)
        gl = gr = None
        hg = wg = h0 = w0 = 1
        scratch = g0 = None
        keep = []
        if warp:
            if default_grid is None:
                raise RuntimeError("floodseg.feat_tail: warp mode needs the default grid")
            g0 = _f32c(default_grid, "default_grid")
            if g0.dim() != 4 or g0.shape[0] != 1 or g0.shape[3] != 2:
                raise RuntimeError("floodseg.feat_tail: default grid must be [1,H0,W0,2]")
            h0, w0 = g0.shape[1], g0.shape[2]
            if f_next is not None and n > 1:
                if len(grids_left) != n - 1 or len(grids_right) != n - 1:
                    raise RuntimeError("floodseg.feat_tail: need n-1 grids per direction")
                keep = [_f32c(g, "grid") for g in grids]
                hg, wg = keep[0].shape[1], keep[0].shape[2]
                for g in keep:
                    if tuple(g.shape) != (1, hg, wg, 2):
                        raise RuntimeError("floodseg.feat_tail: all grids must be [1,Hg,Wg,2] of one size")
                gl = _ptr_array(keep[: n - 1])
                gr = _ptr_array(keep[n - 1:])
                scratch = torch.empty(2 * (n - 1) * hg * wg * c, dtype=torch.float32, device=dev)
        if weights is None:
            check(lib.fs_feat_tail(ptr(f_prev), ptr(f_next), c, fh, fw, gl, gr, hg, wg, ptr(g0), h0, w0, int(n), int(bool(no_warp)), ptr(stack),
                                   ptr(scratch), stream_ptr()))
        else:
            check(lib.fs_feat_tail_weighted(ptr(f_prev), ptr(f_next), c, fh, fw, gl, gr, hg, wg, ptr(g0), h0, w0, int(n), int(bool(no_warp)),
                                            ptr(stack), ptr(scratch), ptr(weights), stream_ptr()))
    return stack


def seg_tail_accumulate(lo_prev, lo_next, grids_left, grids_right, n, crop_hw, no_warp, canvas, count, y0, x0, weights=None):
    """The same tail feeding the sliding-crop canvas (flow/base.py:204-205, 226-234): softmax over K of every output frame
    of this crop is ADDED to canvas [n,K,H,W] (float64) at (y0, x0), count[H,W] += 1 over the crop -- in place.  weights: as seg_tail's."""
    lib = _lib.load()
    grids = [] if (lo_next is None or no_warp) else list(grids_left) + list(grids_right)
    dev = one_device(lo_prev, lo_next, canvas, count, *grids, what="floodseg.seg_tail_accumulate")
    if canvas.dtype != torch.float64 or count.dtype != torch.float64 or not canvas.is_contiguous() or not count.is_contiguous():
        raise RuntimeError("floodseg.seg_tail_accumulate: canvas / count must be contiguous float64 tensors")
    with torch.cuda.device(dev):
        lo_prev = _f32c(lo_prev, "lo_prev")
        _, k, h, w = lo_prev.shape
        frames = n if lo_next is not None else 1
        if tuple(canvas.shape[:2]) != (frames, k) or tuple(canvas.shape[2:]) != tuple(count.shape):
            raise RuntimeError(f"floodseg.seg_tail_accumulate: canvas {tuple(canvas.shape)} / count {tuple(count.shape)} do not match [{frames},{k},H,W]")
        gl = gr = None
        hg = wg = 1
        scratch = None
        keep = []
        if lo_next is not None:
            lo_next = _f32c(lo_next, "lo_next")
            if not no_warp and n > 1:  # as seg_tail: a window of one frame has no grids
                if len(grids_left) != n - 1 or len(grids_right) != n - 1:
                    raise RuntimeError("floodseg.seg_tail_accumulate: need n-1 grids per direction")
                keep = [_f32c(g, "grid") for g in grids]
                hg, wg = keep[0].shape[-3], keep[0].shape[-2]
                for g in keep:
                    if tuple(g.shape[-3:]) != (hg, wg, 2) or g.numel() != hg * wg * 2:
                        raise RuntimeError("floodseg.seg_tail_accumulate: all grids must be [1,Hg,Wg,2] of one size")
                gl = _ptr_array(keep[: n - 1])
                gr = _ptr_array(keep[n - 1:])
                scratch = torch.empty(2 * (n - 1) * k * hg * wg, dtype=torch.float32, device=dev)
        weights = _window_weights_arg(weights, n, dev, "floodseg.seg_tail_accumulate")
        if weights is None:
            check(lib.fs_seg_tail_accumulate(ptr(lo_prev), ptr(lo_next), gl, gr, k, h, w, hg, wg, int(crop_hw[0]), int(crop_hw[1]), int(n),
                                             int(bool(no_warp)), ptr(canvas), ptr(count), canvas.shape[2], canvas.shape[3], int(y0), int(x0),
                                             ptr(scratch), stream_ptr()))
        else:
            check(lib.fs_seg_tail_weighted(ptr(lo_prev), ptr(lo_next), gl, gr, k, h, w, hg, wg, int(crop_hw[0]), int(crop_hw[1]), int(n),
                                           int(bool(no_warp)), None, None, ptr(canvas), ptr(count), canvas.shape[2], canvas.shape[3], int(y0),
                                           int(x0), ptr(scratch), ptr(weights), stream_ptr()))


def crop_grids(grids, frame_hw, crop_yx, crop_hw):
    """crop_motion_vector (flow/transform.py:215-261) for all crops x all grids of a window in ONE launch.
    grids: list of [1,Hg,Wg,2] tensors normalised to the frame (H, W); crop_yx: [(y0, x0), ...]; returns fp32
    [ncrops, len(grids), ch//16, cw//16, 2] -- out[c, j][None] is the grid the reference hands to the network for crop c."""
    lib = _lib.load()
    dev = one_device(*grids, what="floodseg.crop_grids")
    with torch.cuda.device(dev):
        keep = [_f32c(g, "grid") for g in grids]
        hg, wg = keep[0].shape[-3], keep[0].shape[-2]
        for g in keep:
            if tuple(g.shape[-3:]) != (hg, wg, 2) or g.numel() != hg * wg * 2:
                raise RuntimeError("floodseg.crop_grids: all grids must be [1,Hg,Wg,2] of one size")
        nc = len(crop_yx)
        ys = (ctypes.c_int * nc)(*[int(y) for y, _ in crop_yx])
        xs = (ctypes.c_int * nc)(*[int(x) for _, x in crop_yx])
        out = torch.empty((nc, len(keep), int(crop_hw[0]) // 16, int(crop_hw[1]) // 16, 2), dtype=torch.float32, device=dev)
        check(lib.fs_crop_grids(_ptr_array(keep), len(keep), hg, wg, int(frame_hw[0]), int(frame_hw[1]), nc, ys, xs, int(crop_hw[0]),
                                int(crop_hw[1]), ptr(out), stream_ptr()))
    return out


def crops_fuse(lo_prev, lo_next, grids, crop_yx, crop_hw, n, no_warp, frame_hw, want_canvas=True, want_mask=False, weights=None):
    """compute_output after the network for ALL crops of a window in one pass (fs_crops_fuse): lo_prev / lo_next = per-crop
    decoder logits [nc,K,h,w]; grids = crop_grids' output [nc, 2(n-1), fh, fw, 2] or None (no_warp); weights: as seg_tail's.  Returns
    (float64 canvas [n,K,H,W] already divided by the crop count, or None; uint8 argmax [n,H,W] or None) -- each pixel written once."""
    lib = _lib.load()
    dev = one_device(lo_prev, lo_next, grids, what="floodseg.crops_fuse")
    with torch.cuda.device(dev):
        lo_prev = _f32c(lo_prev, "lo_prev")
        nc, k, h, w = lo_prev.shape
        if nc != len(crop_yx):
            raise RuntimeError(f"floodseg.crops_fuse: {nc} crops of logits but {len(crop_yx)} crop windows")
        frames = n if lo_next is not None else 1
        hh, ww = int(frame_hw[0]), int(frame_hw[1])
        warp = lo_next is not None and not no_warp and n > 1
        hg = wg = 1
        scratch = None
        if lo_next is not None:
            lo_next = _f32c(lo_next, "lo_next")
            if lo_next.shape != lo_prev.shape:
                raise RuntimeError("floodseg.crops_fuse: lo_prev / lo_next shapes differ")
        if warp:
            grids = _f32c(grids, "grids")
            if grids.dim() != 5 or grids.shape[0] != nc or grids.shape[1] != 2 * (n - 1) or grids.shape[4] != 2:
                raise RuntimeError(f"floodseg.crops_fuse: grids must be [nc, 2(n-1), Hg, Wg, 2], got {tuple(grids.shape)}")
            hg, wg = grids.shape[2], grids.shape[3]
            scratch = torch.empty(nc * 2 * (n - 1) * k * hg * wg, dtype=torch.float32, device=dev)
        canvas = torch.empty((frames, k, hh, ww), dtype=torch.float64, device=dev) if want_canvas else None
        mask = torch.empty((frames, hh, ww), dtype=torch.uint8, device=dev) if want_mask else None
        ys = (ctypes.c_int * nc)(*[int(y) for y, _ in crop_yx])
        xs = (ctypes.c_int * nc)(*[int(x) for _, x in crop_yx])
        weights = _window_weights_arg(weights, n, dev, "floodseg.crops_fuse")
        if weights is None:
            check(lib.fs_crops_fuse(ptr(lo_prev), ptr(lo_next), ptr(grids) if warp else None, nc, ys, xs, k, h, w, hg, wg, int(crop_hw[0]),
                                    int(crop_hw[1]), int(n), int(not warp), ptr(canvas), ptr(mask), hh, ww, ptr(scratch), stream_ptr()))
        else:
            check(lib.fs_crops_fuse_weighted(ptr(lo_prev), ptr(lo_next), ptr(grids) if warp else None, nc, ys, xs, k, h, w, hg, wg,
                                             int(crop_hw[0]), int(crop_hw[1]), int(n), int(not warp), ptr(canvas), ptr(mask), hh, ww,
                                             ptr(scratch), ptr(weights), stream_ptr()))
    return canvas, mask


def canvas_finish(canvas, count, out_size=None, want_mask=False):
    """canvas /= count in place (flow/base.py:208); optionally the uint8 argmax of its align_corners=True bilinear resize to
    `out_size` evaluated in float64 (flow/base.py:275-276) -- the identity resize when out_size is the canvas size."""
    lib = _lib.load()
    dev = one_device(canvas, count, what="floodseg.canvas_finish")
    n, k, h, w = canvas.shape
    with torch.cuda.device(dev):
        same = out_size is None or (int(out_size[0]), int(out_size[1])) == (h, w)
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if (want_mask and same) else None
        check(lib.fs_canvas_finish(ptr(canvas), ptr(count), n, k, h * w, ptr(mask), stream_ptr()))
        if want_mask and not same:
            mask = torch.empty((n, int(out_size[0]), int(out_size[1])), dtype=torch.uint8, device=dev)
            check(lib.fs_canvas_resize_argmax(ptr(canvas), n, k, h, w, ptr(mask), int(out_size[0]), int(out_size[1]), stream_ptr()))
    return mask


def canvas_resize_argmax(canvas, out_size):
    """uint8 argmax of the align_corners=True bilinear resize (in float64) of a crop-averaged canvas (flow/base.py:275-276)."""
    lib = _lib.load()
    dev = one_device(canvas, what="floodseg.canvas_resize_argmax")
    n, k, h, w = canvas.shape
    with torch.cuda.device(dev):
        mask = torch.empty((n, int(out_size[0]), int(out_size[1])), dtype=torch.uint8, device=dev)
        check(lib.fs_canvas_resize_argmax(ptr(canvas), n, k, h, w, ptr(mask), int(out_size[0]), int(out_size[1]), stream_ptr()))
    return mask


def argmax_u8(logits):
    """logits.max(1)[1] as uint8 (flow/base.py:276-277)."""
    lib = _lib.load()
    with torch.cuda.device(one_device(logits, what="floodseg.argmax_u8")):
        x = _f32c(logits)
        b, k, h, w = x.shape
        out = torch.empty((b, h, w), dtype=torch.uint8, device=x.device)
        if b == 0:
            return out
        check(lib.fs_argmax_u8(ptr(x), b, k, h * w, ptr(out), stream_ptr()))
    return out


def resize_argmax_u8(logits, size):
    """F.interpolate(logits, size, bilinear, align_corners=True).max(1)[1] without the big intermediate."""
    lib = _lib.load()
    with torch.cuda.device(one_device(logits, what="floodseg.resize_argmax_u8")):
        x = _f32c(logits)
        b, k, h, w = x.shape
        out = torch.empty((b, int(size[0]), int(size[1])), dtype=torch.uint8, device=x.device)
        if b == 0:
            return out
        check(lib.fs_resize_argmax_u8(ptr(x), b, k, h, w, ptr(out), int(size[0]), int(size[1]), stream_ptr()))
    return out


def resize_crop(logits, full_size, size, align_corners=False, want_logits=True, want_mask=False):
    """F.interpolate(logits, full_size, bilinear, align_corners)[:, :, :size[0], :size[1]] as a DENSE tensor, and / or its
    .max(1)[1] as uint8 -- the Segmenter's upsample + unpadding (segm/model/segmenter.py:45-46, segm/model/utils.py:79-89) in
    one launch.  Returns (logits or None, mask or None)."""
    lib = _lib.load()
    if not (want_logits or want_mask):
        raise RuntimeError("floodseg.resize_crop: no output requested")
    with torch.cuda.device(one_device(logits, what="floodseg.resize_crop")):
        x = _f32c(logits)
        b, k, hi, wi = x.shape
        hf, wf, ho, wo = int(full_size[0]), int(full_size[1]), int(size[0]), int(size[1])
        if ho > hf or wo > wf or min(ho, wo) < 1:
            raise RuntimeError(f"floodseg.resize_crop: kept region {ho}x{wo} is not inside the resized frame {hf}x{wf}")
        out = torch.empty((b, k, ho, wo), dtype=torch.float32, device=x.device) if want_logits else None
        mask = torch.empty((b, ho, wo), dtype=torch.uint8, device=x.device) if want_mask else None
        if b:
            check(lib.fs_resize_crop(ptr(x), b, k, hi, wi, hf, wf, int(align_corners), ptr(out) if want_logits else None,
                                     ptr(mask) if want_mask else None, ho, wo, stream_ptr()))
    return out, mask


def iou_hist(pred_u8, target_u8, classes, ignore_index=255, hist=None):
    """Accumulate int64[3,K] = (intersection, |pred|, |target|) (util/util.py:52-63)."""
    lib = _lib.load()
    p = pred_u8.contiguous()
    t = target_u8.contiguous()
    if p.dtype != torch.uint8 or t.dtype != torch.uint8 or p.shape != t.shape:
        raise RuntimeError("floodseg.iou_hist: uint8 tensors of equal shape required")
    dev = one_device(p, t, hist, what="floodseg.iou_hist")
    with torch.cuda.device(dev):
        if hist is None:
            hist = torch.zeros((3, classes), dtype=torch.int64, device=dev)
        if p.numel() == 0:
            return hist
        check(lib.fs_iou_hist(ptr(p), ptr(t), p.numel(), classes, ignore_index, ptr(hist), stream_ptr()))
    return hist


# ------------------------------------------------------------------------------------------ confidence and the extent report
def _confidence_out(n, size, h, w, dev):
    hh, ww = (h, w) if size is None else (int(size[0]), int(size[1]))
    if hh < 1 or ww < 1:
        raise RuntimeError(f"floodseg: size must be at least 1 x 1, got {hh} x {ww}")
    return hh, ww, torch.empty((n, hh, ww), dtype=torch.uint8, device=dev), torch.empty((n, hh, ww), dtype=torch.uint8, device=dev)


def mask_confidence(logits, size=None):
    """fp32 logits [n,K,h,w] -> (mask, confidence), uint8 [n,H,W] each, in one launch (definition: include/floodseg_test.h,
    mask_confidence): the argmax of the align_corners=True resize to `size` (None = the logits' size: the logits themselves) as
    resize_argmax_u8 / argmax_u8 give it, and round(255 * softmax probability of that class).  K <= 32."""
    lib = _lib.load()
    dev = one_device(logits, what="floodseg.mask_confidence")
    if logits.dtype != torch.float32 or logits.dim() != 4:
        raise RuntimeError(f"floodseg.mask_confidence: logits must be float32 [n,K,h,w], got {logits.dtype} {tuple(logits.shape)}")
    n, k, h, w = logits.shape
    if not 1 <= k <= 32 or h < 1 or w < 1:
        raise RuntimeError(f"floodseg.mask_confidence: 1..32 classes on a non-empty map, got {tuple(logits.shape)}")
    with torch.cuda.device(dev):
        hh, ww, mask, conf = _confidence_out(n, size, h, w, dev)
        if n:
            check(lib.fs_mask_confidence(ptr(logits.contiguous()), n, k, h, w, ptr(mask), ptr(conf), hh, ww, stream_ptr()))
    return mask, conf


def canvas_confidence(canvas, size=None):
    """The float64 crop-averaged canvas [n,K,h,w] of crops_fuse(want_canvas=True) -> (mask, confidence), uint8 [n,H,W] each, in one
    launch (definition: include/floodseg_test.h, canvas_confidence): canvas_resize_argmax's mask and round(255 * the winning mean
    probability), the resize evaluated in float64."""
    lib = _lib.load()
    dev = one_device(canvas, what="floodseg.canvas_confidence")
    if canvas.dtype != torch.float64 or canvas.dim() != 4:
        raise RuntimeError(f"floodseg.canvas_confidence: canvas must be float64 [n,K,h,w], got {canvas.dtype} {tuple(canvas.shape)}")
    n, k, h, w = canvas.shape
    if not 1 <= k <= 255 or h < 1 or w < 1:
        raise RuntimeError(f"floodseg.canvas_confidence: 1..255 classes on a non-empty map, got {tuple(canvas.shape)}")
    with torch.cuda.device(dev):
        hh, ww, mask, conf = _confidence_out(n, size, h, w, dev)
        if n:
            check(lib.fs_canvas_confidence(ptr(canvas.contiguous()), n, k, h, w, ptr(mask), ptr(conf), hh, ww, stream_ptr()))
    return mask, conf


def frame_report(mask, conf=None, classes=5, low=128, out=None):
    """uint8 masks [n,H,W] (and their confidence planes) -> int64 [n,K,3]: per frame and class the pixels, the sum of their confidence
    codes and the pixels with confidence < low (definition: include/floodseg_test.h, frame_report).  conf None: counts only.  Mask ids
    >= classes are counted nowhere.  out: a caller-owned contiguous int64 [n,K,3] destination (rows of a larger buffer); it is
    written whole, never accumulated into."""
    lib = _lib.load()
    dev = one_device(mask, conf, out, what="floodseg.frame_report")
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise RuntimeError(f"floodseg.frame_report: mask must be uint8 [n,H,W], got {mask.dtype} {tuple(mask.shape)}")
    if conf is not None and (conf.dtype != torch.uint8 or conf.shape != mask.shape):
        raise RuntimeError(f"floodseg.frame_report: conf must be uint8 of the mask's shape {tuple(mask.shape)}, got {conf.dtype} {tuple(conf.shape)}")
    k, low = int(classes), int(low)
    if not 1 <= k <= 255 or not 0 <= low <= 255:
        raise RuntimeError(f"floodseg.frame_report: classes must be 1..255 and low 0..255, got {classes} and {low}")
    n, h, w = mask.shape
    if h < 1 or w < 1:
        raise RuntimeError(f"floodseg.frame_report: empty frames {tuple(mask.shape)}")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((n, k, 3), dtype=torch.int64, device=dev)
        elif out.dtype != torch.int64 or tuple(out.shape) != (n, k, 3) or not out.is_contiguous():
            raise RuntimeError(f"floodseg.frame_report: out must be a contiguous int64 [{n},{k},3] tensor, got {out.dtype} {tuple(out.shape)}")
        if n:
            check(lib.fs_frame_report(ptr(mask.contiguous()), ptr(conf.contiguous()) if conf is not None else None, n, h, w, k, low, ptr(out),
                                      stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ connected regions
REGION_RANK_CHUNK = 1024  # pixels per int of region_table's workspace (include/floodseg_test.h)


def _region_mask(mask, classes, what):
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise RuntimeError(f"floodseg.{what}: mask must be uint8 [n,H,W], got {mask.dtype} {tuple(mask.shape)}")
    n, h, w = mask.shape
    if not 1 <= int(classes) <= 255 or h < 1 or w < 1 or h * w >= 2 ** 31 - 1:
        raise RuntimeError(f"floodseg.{what}: 1..255 classes on non-empty frames below 2^31 - 1 pixels, got {classes} and {tuple(mask.shape)}")
    return n, h, w, int(classes)


def mask_regions(mask, classes, connectivity=8):
    """uint8 masks [n,H,W] -> int32 labels [n,H,W] of their connected regions (definition: include/floodseg_test.h, mask_regions): a
    region is a maximal connected set of pixels of one frame with the same id < classes, its label 1 + the raster index of its first
    pixel; ids >= classes are background, label 0.  connectivity 4 or 8.  Three launches, no workspace, nothing read back."""
    lib = _lib.load()
    dev = one_device(mask, what="floodseg.mask_regions")
    n, h, w, k = _region_mask(mask, classes, "mask_regions")
    if connectivity not in (4, 8):
        raise RuntimeError(f"floodseg.mask_regions: connectivity must be 4 or 8, got {connectivity}")
    with torch.cuda.device(dev):
        labels = torch.empty((n, h, w), dtype=torch.int32, device=dev)
        if n:
            check(lib.fs_mask_regions(ptr(mask.contiguous()), n, h, w, k, int(connectivity), ptr(labels), stream_ptr()))
    return labels


def region_table(mask, labels, classes, conf=None, low=128, max_regions=1024, out=None):
    """Masks and their labels (mask_regions) -> (table int64 [n,max_regions,10], counts int64 [n,2], index int32 [n,H,W]) (definition:
    include/floodseg_test.h, region_table).  Table rows, in the order of the regions' first pixels: class, area, x0, y0, x1, y1
    (inclusive), sum_x, sum_y, the sum of the confidence codes, the pixels with confidence < low (the last two 0 without conf).
    counts = (regions, rows written); index = the row of each pixel's region, -1 for background and past max_regions.
    out: caller-owned contiguous (table, counts) destinations (rows of larger buffers); they are written whole.  The workspace
    (one int per 1024 pixels) is allocated here."""
    lib = _lib.load()
    dev = one_device(mask, labels, conf, *(out or ()), what="floodseg.region_table")
    n, h, w, k = _region_mask(mask, classes, "region_table")
    if labels.dtype != torch.int32 or labels.shape != mask.shape:
        raise RuntimeError(f"floodseg.region_table: labels must be int32 of the mask's shape {tuple(mask.shape)}, got {labels.dtype} {tuple(labels.shape)}")
    if conf is not None and (conf.dtype != torch.uint8 or conf.shape != mask.shape):
        raise RuntimeError(f"floodseg.region_table: conf must be uint8 of the mask's shape {tuple(mask.shape)}, got {conf.dtype} {tuple(conf.shape)}")
    low, cap = int(low), int(max_regions)
    if not 0 <= low <= 255 or not 1 <= cap <= 65536:
        raise RuntimeError(f"floodseg.region_table: low must be 0..255 and max_regions 1..65536, got {low} and {max_regions}")
    with torch.cuda.device(dev):
        if out is None:
            table = torch.empty((n, cap, 10), dtype=torch.int64, device=dev)
            counts = torch.empty((n, 2), dtype=torch.int64, device=dev)
        else:
            table, counts = out
            if (table.dtype != torch.int64 or tuple(table.shape) != (n, cap, 10) or not table.is_contiguous() or counts.dtype != torch.int64
                    or tuple(counts.shape) != (n, 2) or not counts.is_contiguous()):
                raise RuntimeError(f"floodseg.region_table: out must be contiguous int64 [{n},{cap},10] and [{n},2] tensors")
        index = torch.empty((n, h, w), dtype=torch.int32, device=dev)
        if n:
            work = torch.empty((n, -(-h * w // REGION_RANK_CHUNK)), dtype=torch.int32, device=dev)
            check(lib.fs_region_table(ptr(mask.contiguous()), ptr(labels.contiguous()), ptr(conf.contiguous()) if conf is not None else None, n, h, w,
                                      k, low, cap, ptr(table), ptr(counts), ptr(index), ptr(work), stream_ptr()))
    return table, counts, index


def region_filter(mask, index, table, classes, min_area):
    """Despeckle (definition: include/floodseg_test.h, region_filter): every region of region_table's result with area < min_area takes
    the class most of its pixels' 4-neighbours in large-enough regions have (lowest id on a tie; nobody to ask: it stays).  One pass
    over the input mask; returns a new mask, equal to the input outside such regions and bit for bit for min_area <= 1.  The vote
    workspace (int32 [n,max_regions,classes]) is allocated here."""
    lib = _lib.load()
    dev = one_device(mask, index, table, what="floodseg.region_filter")
    n, h, w, k = _region_mask(mask, classes, "region_filter")
    if index.dtype != torch.int32 or index.shape != mask.shape:
        raise RuntimeError(f"floodseg.region_filter: index must be int32 of the mask's shape {tuple(mask.shape)}, got {index.dtype} {tuple(index.shape)}")
    if table.dtype != torch.int64 or table.dim() != 3 or table.shape[0] != n or table.shape[2] != 10 or not 1 <= table.shape[1] <= 65536:
        raise RuntimeError(f"floodseg.region_filter: table must be int64 [{n},max_regions,10], got {table.dtype} {tuple(table.shape)}")
    if int(min_area) < 0 or int(min_area) >= 2 ** 31:
        raise RuntimeError(f"floodseg.region_filter: min_area must be 0..2^31 - 1, got {min_area}")
    with torch.cuda.device(dev):
        out = torch.empty_like(mask, memory_format=torch.contiguous_format)
        if n:
            votes = torch.empty((n, table.shape[1], k), dtype=torch.int32, device=dev)
            check(lib.fs_region_filter(ptr(mask.contiguous()), ptr(index.contiguous()), ptr(table.contiguous()), n, h, w, k, table.shape[1], int(min_area),
                                       ptr(out), ptr(votes), stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ region identity across frames
def default_max_pairs(max_regions):
    """The pair table of region_links by default: the next power of two >= 4 x max_regions (at least 16)."""
    return max(16, 1 << (4 * int(max_regions) - 1).bit_length())


def region_links_workspace_bytes(n, max_regions, max_pairs):
    """FS_REGION_LINKS_WORKSPACE_BYTES of include/floodseg_test.h."""
    return n * (12 * max_pairs + 16 * max_regions + 8)


def region_links_mc_workspace_bytes(n, max_regions, max_pairs, hb, wb):
    """FS_REGION_LINKS_MC_WORKSPACE_BYTES of include/floodseg_test.h: region_links' and one dword per block and frame behind it."""
    return region_links_workspace_bytes(n, max_regions, max_pairs) + (n * hb * wb * 4 + 7) // 8 * 8


def _int64_2d(t, shape, name, what):
    if t.dtype != torch.int64 or tuple(t.shape) != shape:
        raise RuntimeError(f"floodseg.{what}: {name} must be int64 {list(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def region_links(index, table, counts, prev=None, max_pairs=None, min_overlap=1, mv=None, frame_size=None, pair_stats=None):
    """region_table's (index int32 [n,H,W], table int64 [n,R,10], counts int64 [n,2]) of consecutive frames -> (back int32 [n,R,2],
    fwd int32 [n,R,2], link_counts int64 [n,2]) (definition: include/floodseg_test.h, region_links): back[f][b] = (row, overlap) of the
    row of frame f-1 that shares the most pixels with row b of frame f among the rows of b's class, fwd[f][a] the same for row a of frame
    f-1 among the rows of frame f; (-1, 0) without a partner of at least min_overlap pixels.  prev = (index [H,W], table [R,10], counts
    [2]) of the frame before frame 0, None: frame 0 has no links.  max_pairs: the slots of the pair table, a power of two in 16..2^20
    (default: the next one >= 4 R); a frame pair with more distinct overlapping pairs has no links at all and link_counts[f] = (max_pairs,
    1).  The workspace is allocated here.
    mv = int32 [n, (FH // 16) * (FW // 16), 7] with frame_size = (FH, FW): the MOTION-COMPENSATED links (definition: region_links_mc) --
    mv[f] is block_match's / block_match_modes' table of frame f against frame f-1 on decoded frames of FH x FW pixels, and the frame
    before is read at every pixel's source under its block's vector, scaled to the mask.  pair_stats = int32 [n, 4], block_match_modes'
    stats rows (optional): a pair flagged as a cut gets no links and link_counts[f] = (0, 2).  With mv=None exactly the in-place call."""
    lib = _lib.load()
    dev = one_device(index, table, counts, *(prev or ()), mv, pair_stats, what="floodseg.region_links")
    if index.dtype != torch.int32 or index.dim() != 3:
        raise RuntimeError(f"floodseg.region_links: index must be int32 [n,H,W], got {index.dtype} {tuple(index.shape)}")
    n, h, w = index.shape
    if table.dtype != torch.int64 or table.dim() != 3 or table.shape[0] != n or table.shape[2] != 10 or not 1 <= table.shape[1] <= 65536:
        raise RuntimeError(f"floodseg.region_links: table must be int64 [{n},max_regions,10], got {table.dtype} {tuple(table.shape)}")
    cap = table.shape[1]
    counts = _int64_2d(counts, (n, 2), "counts", "region_links")
    if h < 1 or w < 1 or h * w >= 2 ** 31 - 1 or n > 65535:
        raise RuntimeError(f"floodseg.region_links: at most 65535 non-empty frames below 2^31 - 1 pixels, got {tuple(index.shape)}")
    pairs = default_max_pairs(cap) if max_pairs is None else int(max_pairs)
    if not 16 <= pairs <= 2 ** 20 or pairs & (pairs - 1) or int(min_overlap) < 1 or int(min_overlap) >= 2 ** 31:
        raise RuntimeError(f"floodseg.region_links: max_pairs must be a power of two in 16..2^20 and min_overlap >= 1, got {max_pairs} and {min_overlap}")
    if prev is not None:
        if len(prev) != 3 or prev[0].dtype != torch.int32 or tuple(prev[0].shape) != (h, w):
            raise RuntimeError(f"floodseg.region_links: prev must be (index int32 [{h},{w}], table int64 [{cap},10], counts int64 [2])")
        prev = (prev[0].contiguous(), _int64_2d(prev[1], (cap, 10), "prev table", "region_links"), _int64_2d(prev[2], (2,), "prev counts", "region_links"))
    if mv is None:
        if frame_size is not None or pair_stats is not None:
            raise RuntimeError("floodseg.region_links: frame_size and pair_stats go with mv (the motion-compensated links)")
    else:
        if frame_size is None or len(frame_size) != 2 or min(int(v) for v in frame_size) < 16 or int(frame_size[0]) * int(frame_size[1]) >= 2 ** 31:
            raise RuntimeError(f"floodseg.region_links: mv needs frame_size = (height, width) of the decoded frame, both >= 16, got {frame_size}")
        fh, fw = int(frame_size[0]), int(frame_size[1])
        hb, wb = fh // 16, fw // 16
        if mv.dtype != torch.int32 or tuple(mv.shape) != (n, hb * wb, 7):
            raise RuntimeError(f"floodseg.region_links: mv must be int32 [{n},{hb * wb},7] for a {fh} x {fw} frame, got {mv.dtype} {tuple(mv.shape)}")
        if h > 31 * fh or w > 31 * fw:
            raise RuntimeError(f"floodseg.region_links: the mask ({h} x {w}) may be at most 31 times the decoded frame ({fh} x {fw}) along an axis")
        if pair_stats is not None and (pair_stats.dtype != torch.int32 or tuple(pair_stats.shape) != (n, 4)):
            raise RuntimeError(f"floodseg.region_links: pair_stats must be int32 [{n},4], got {pair_stats.dtype} {tuple(pair_stats.shape)}")
    with torch.cuda.device(dev):
        back = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)
        fwd = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)
        link_counts = torch.empty((n, 2), dtype=torch.int64, device=dev)
        p = prev or (None, None, None)
        if n and mv is not None:
            work = torch.empty((region_links_mc_workspace_bytes(n, cap, pairs, hb, wb) // 8,), dtype=torch.int64, device=dev)
            check(lib.fs_region_links_mc(ptr(index.contiguous()), ptr(table.contiguous()), ptr(counts), ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(mv.contiguous()),
                                         ptr(None if pair_stats is None else pair_stats.contiguous()), n, h, w, fh, fw, cap, pairs, int(min_overlap),
                                         ptr(back), ptr(fwd), ptr(link_counts), ptr(work), stream_ptr()))
        elif n:
            work = torch.empty((region_links_workspace_bytes(n, cap, pairs) // 8,), dtype=torch.int64, device=dev)
            check(lib.fs_region_links(ptr(index.contiguous()), ptr(table.contiguous()), ptr(counts), ptr(p[0]), ptr(p[1]), ptr(p[2]), n, h, w, cap, pairs,
                                      int(min_overlap), ptr(back), ptr(fwd), ptr(link_counts), ptr(work), stream_ptr()))
    return back, fwd, link_counts


def region_tracks(back, fwd, counts, state, prev_tracks=None, out=None):
    """region_links' back / fwd and the frames' counts -> tracks int64 [n,R,4] = (track id, parent id, previous row, overlap with it)
    (definition: include/floodseg_test.h, region_tracks): a region whose best predecessor's best successor it is continues that track;
    every other region is born, with the next ids in row order and its best predecessor's track as parent (-1: none).  state = a
    device int64 [2] = (next id, 0), read and updated in place.  prev_tracks = the int64 [R,4] tracks row of the frame before frame 0
    (None: every region of frame 0 is born without a parent).  out: a caller-owned contiguous int64 [n,R,4] destination (rows of a larger
    buffer); it is written whole."""
    lib = _lib.load()
    dev = one_device(back, fwd, counts, state, prev_tracks, out, what="floodseg.region_tracks")
    if back.dtype != torch.int32 or back.dim() != 3 or back.shape[2] != 2 or not 1 <= back.shape[1] <= 65536 or back.shape[0] > 65535:
        raise RuntimeError(f"floodseg.region_tracks: back must be int32 [n,max_regions,2], got {back.dtype} {tuple(back.shape)}")
    n, cap = back.shape[0], back.shape[1]
    if fwd.dtype != torch.int32 or fwd.shape != back.shape:
        raise RuntimeError(f"floodseg.region_tracks: fwd must be int32 {list(back.shape)}, got {fwd.dtype} {tuple(fwd.shape)}")
    counts = _int64_2d(counts, (n, 2), "counts", "region_tracks")
    if state.dtype != torch.int64 or tuple(state.shape) != (2,) or not state.is_contiguous():
        raise RuntimeError(f"floodseg.region_tracks: state must be a contiguous int64 [2] tensor, got {state.dtype} {tuple(state.shape)}")
    if prev_tracks is not None:
        prev_tracks = _int64_2d(prev_tracks, (cap, 4), "prev_tracks", "region_tracks")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((n, cap, 4), dtype=torch.int64, device=dev)
        elif out.dtype != torch.int64 or tuple(out.shape) != (n, cap, 4) or not out.is_contiguous():
            raise RuntimeError(f"floodseg.region_tracks: out must be a contiguous int64 [{n},{cap},4] tensor, got {out.dtype} {tuple(out.shape)}")
        if n:
            check(lib.fs_region_tracks(ptr(back.contiguous()), ptr(fwd.contiguous()), ptr(counts), ptr(prev_tracks), n, cap, ptr(state), ptr(out),
                                       stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ temporal mask stabiliser
def mask_stabilize_workspace_bytes(n, h, w, hb=0, wb=0):
    """FS_MASK_STABILIZE_WORKSPACE_BYTES of include/floodseg_test.h: 0 in place (hb = wb = 0); with mv the second state plane (4 B per
    pixel, rounded up to 16) and hb * wb + 1 dwords per frame."""
    if hb * wb == 0:
        return 0
    return (h * w + 3) // 4 * 16 + (n * (hb * wb + 1) + 3) // 4 * 16


def mask_stabilize(mask, state=None, conf=None, classes=5, persist=3, trust=None, mv=None, frame_size=None, pair_stats=None, out=None):
    """Causal per-pixel class debounce along the time axis (definition: include/floodseg_test.h, mask_stabilize):
    uint8 masks [n,H,W] -> (out uint8 [n,H,W], state uint32-as-int32 [H,W], counts int64 [n,4] = (held, switched, seeded, trusted)).
    A pixel keeps its emitted class until another class has been observed `persist` frames running (persist=1: out == mask), or at
    once where conf (uint8 [n,H,W]) >= trust (0..256; None: nothing is trusted outright).  Ids >= classes pass through and end the
    pixel's history.  state: the int32 [H,W] plane an earlier call returned (the words: bit 31 valid, emitted | candidate << 8 | run <<
    16), UPDATED IN PLACE and returned; None: frame 0 seeds and a new plane is returned.  One call over n frames equals any chain of calls.
    mv = int32 [n, (FH // 16) * (FW // 16), 7] with frame_size = (FH, FW): the prior state is read at every pixel's SOURCE under the
    block matcher's vectors (ops.region_links' rule), 0 where the source lies outside the mask.  pair_stats = int32 [n,4],
    block_match_modes' stats rows: a frame flagged as a cut starts from no state, with or without mv.  out: a caller-owned contiguous
    uint8 [n,H,W] destination.  The compensated workspace is allocated here; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.mask_stabilize"
    dev = one_device(mask, state, conf, mv, pair_stats, out, what=what)
    n, h, w, k = _region_mask(mask, classes, "mask_stabilize")
    if conf is not None and (conf.dtype != torch.uint8 or conf.shape != mask.shape):
        raise RuntimeError(f"{what}: conf must be uint8 of the mask's shape {tuple(mask.shape)}, got {conf.dtype} {tuple(conf.shape)}")
    if not 1 <= int(persist) <= 255:
        raise RuntimeError(f"{what}: persist must be 1..255, got {persist}")
    if trust is not None and (conf is None or not 0 <= int(trust) <= 256):
        raise RuntimeError(f"{what}: trust must be 0..256 and needs conf, got {trust} with conf {'given' if conf is not None else 'missing'}")
    if state is not None and (state.dtype != torch.int32 or tuple(state.shape) != (h, w) or not state.is_contiguous() or state.data_ptr() % 16):
        raise RuntimeError(f"{what}: state must be a contiguous 16-byte aligned int32 [{h},{w}] tensor (an earlier call's), got {state.dtype} {tuple(state.shape)}")
    fh = fw = hb = wb = 0
    if mv is None:
        if frame_size is not None:
            raise RuntimeError(f"{what}: frame_size goes with mv (the motion-compensated route)")
    else:
        if frame_size is None or len(frame_size) != 2 or min(int(v) for v in frame_size) < 16 or int(frame_size[0]) * int(frame_size[1]) >= 2 ** 31:
            raise RuntimeError(f"{what}: mv needs frame_size = (height, width) of the decoded frame, both >= 16, got {frame_size}")
        fh, fw = int(frame_size[0]), int(frame_size[1])
        hb, wb = fh // 16, fw // 16
        if mv.dtype != torch.int32 or tuple(mv.shape) != (n, hb * wb, 7):
            raise RuntimeError(f"{what}: mv must be int32 [{n},{hb * wb},7] for a {fh} x {fw} frame, got {mv.dtype} {tuple(mv.shape)}")
        if h > 31 * fh or w > 31 * fw or n > 65535:
            raise RuntimeError(f"{what}: the mask ({h} x {w}) may be at most 31 times the decoded frame ({fh} x {fw}) along an axis, and n at most 65535")
    if pair_stats is not None and (pair_stats.dtype != torch.int32 or tuple(pair_stats.shape) != (n, 4)):
        raise RuntimeError(f"{what}: pair_stats must be int32 [{n},4], got {pair_stats.dtype} {tuple(pair_stats.shape)}")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w) or not out.is_contiguous():
            raise RuntimeError(f"{what}: out must be a contiguous uint8 [{n},{h},{w}] tensor, got {out.dtype} {tuple(out.shape)}")
        has_state = state is not None
        if state is None:
            state = torch.empty((h, w), dtype=torch.int32, device=dev)
        counts = torch.empty((n, 4), dtype=torch.int64, device=dev)
        if n:
            work = None
            if mv is not None:
                work = torch.empty((mask_stabilize_workspace_bytes(n, h, w, hb, wb) // 16, 2), dtype=torch.int64, device=dev)
            check(lib.fs_mask_stabilize(ptr(mask.contiguous()), ptr(None if conf is None else conf.contiguous()), ptr(None if mv is None else mv.contiguous()),
                                        ptr(None if pair_stats is None else pair_stats.contiguous()), n, h, w, fh, fw, k, int(persist),
                                        256 if trust is None else int(trust), int(has_state), ptr(state), ptr(out), ptr(counts), ptr(work), stream_ptr()))
        elif not has_state:
            state.zero_()
    return out, state, counts


# ------------------------------------------------------------------------------------------ distance to a class
DIST_NONE = 0xFFFFFFFF  # FS_DIST_NONE; the int32 tensors that carry d2 show it as -1


def mask_distance_workspace_bytes(n, h, w):
    """FS_MASK_DISTANCE_WORKSPACE_BYTES of include/floodseg_test.h: one dword per column and chunk of 64 rows, 2 bytes per pixel."""
    return (n * ((h + 63) // 64) * w * 4 + n * h * w * 2 + 15) // 16 * 16


def class_set(classes, name, what, allow_empty=False):
    """An iterable of class ids 0..31 -> the uint32 with those bits set (source_set / target_set of the distance ops)."""
    ids = [int(c) for c in classes]
    if any(not 0 <= c <= 31 for c in ids) or (not ids and not allow_empty):
        raise ValueError(f"{what}: {name} must be class ids 0..31{'' if allow_empty else ', at least one'}, got {list(classes)}")
    bits = 0
    for c in ids:
        bits |= 1 << c
    return bits


def mask_distance(mask, sources, max_dist=0, want_nearest=True, out=None):
    """The exact squared Euclidean distance of every pixel to the nearest pixel of the classes `sources` in its own frame (definition:
    include/floodseg_test.h, mask_distance): uint8 masks [n,H,W] -> (d2, nearest).  d2: int32 [n,H,W] holding the uint32
    values (0 on a source pixel; FS_DIST_NONE = 0xFFFFFFFF, read as -1, in a frame without a source and, with max_dist = R > 0, beyond
    R pixels; every other value is the exact minimum).  nearest: int32 [n,H,W], the raster index y * W + x of the nearest source pixel,
    the smallest index among several, -1 where d2 is FS_DIST_NONE; None with want_nearest=False.  sources: class ids 0..31.  Distances are
    in mask pixels.  out: caller-owned contiguous (d2, nearest) destinations.  The workspace is allocated here; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.mask_distance"
    dev = one_device(mask, *(out or ()), what=what)
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise ValueError(f"{what}: mask must be uint8 [n,H,W], got {mask.dtype} {tuple(mask.shape)}")
    n, h, w = mask.shape
    if not 1 <= h <= 32768 or not 1 <= w <= 32768 or n > 65535:
        raise ValueError(f"{what}: at most 65535 frames of 1..32768 pixels a side, got {tuple(mask.shape)}")
    bits = class_set(sources, "sources", what)
    if not 0 <= int(max_dist) <= 32767:
        raise ValueError(f"{what}: max_dist must be 0..32767 pixels (0: unbounded), got {max_dist}")
    with torch.cuda.device(dev):
        if out is None:
            d2 = torch.empty((n, h, w), dtype=torch.int32, device=dev)
            nearest = torch.empty((n, h, w), dtype=torch.int32, device=dev) if want_nearest else None
        else:
            d2, nearest = out
            for t, name in ((d2, "d2"), (nearest, "nearest")):
                if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (n, h, w) or not t.is_contiguous()):
                    raise ValueError(f"{what}: out's {name} must be a contiguous int32 [{n},{h},{w}] tensor, got {t.dtype} {tuple(t.shape)}")
            if (nearest is not None) != bool(want_nearest):
                raise ValueError(f"{what}: out = (d2, nearest) must hold a nearest plane exactly when want_nearest is set")
        if n:
            work = torch.empty((mask_distance_workspace_bytes(n, h, w) // 4,), dtype=torch.int32, device=dev)
            check(lib.fs_mask_distance(ptr(mask.contiguous()), n, h, w, bits, int(max_dist), ptr(d2), ptr(nearest), ptr(work), stream_ptr()))
    return d2, nearest


def region_proximity(mask, d2, nearest, index, counts, classes, max_regions, targets, thresholds, out=None):
    """mask_distance's field tabulated per class and per region (definition: include/floodseg_test.h, region_proximity):
    -> (exposure int64 [n,classes,B], near int64 [n,max_regions,8]).  exposure[f][k][b] = the pixels of class k (k in targets, ids 0..31)
    within thresholds[b] pixels of a source, cumulative in b.  near rows, one per row of region_table's table (index, counts):
    (min_d2, at_x, at_y, src_x, src_y, src_row, near_pixels, 0) -- the region's smallest squared distance, the pixel that attains it
    (lowest raster index), the source pixel nearest to it and that pixel's region row (-1: none; all three -1 with nearest=None), and
    the region's pixels within thresholds[0]; a region out of reach of every source: (-1, -1, -1, -1, -1, -1, 0, 0).  thresholds: 1..8
    strictly ascending ints 0..32767.  out: caller-owned contiguous (exposure, near) destinations; they are written whole."""
    lib = _lib.load()
    what = "floodseg.region_proximity"
    dev = one_device(mask, d2, nearest, index, counts, *(out or ()), what=what)
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise ValueError(f"{what}: mask must be uint8 [n,H,W], got {mask.dtype} {tuple(mask.shape)}")
    n, h, w = mask.shape
    if not 1 <= h <= 32768 or not 1 <= w <= 32768 or n > 65535:
        raise ValueError(f"{what}: at most 65535 frames of 1..32768 pixels a side, got {tuple(mask.shape)}")
    for t, name in ((d2, "d2"), (nearest, "nearest"), (index, "index")):
        if (t is None and name != "nearest") or (t is not None and (t.dtype != torch.int32 or t.shape != mask.shape)):
            raise ValueError(f"{what}: {name} must be int32 of the mask's shape {tuple(mask.shape)}, got "
                             f"{None if t is None else (t.dtype, tuple(t.shape))}")
    if counts.dtype != torch.int64 or tuple(counts.shape) != (n, 2):
        raise ValueError(f"{what}: counts must be int64 [{n},2] (region_table's), got {counts.dtype} {tuple(counts.shape)}")
    k, cap = int(classes), int(max_regions)
    if not 1 <= k <= 255 or not 1 <= cap <= 65536:
        raise ValueError(f"{what}: classes must be 1..255 and max_regions 1..65536, got {classes} and {max_regions}")
    bits = class_set(targets, "targets", what, allow_empty=True)
    thr = [int(t) for t in thresholds]
    if not 1 <= len(thr) <= 8 or any(not 0 <= t <= 32767 for t in thr) or any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError(f"{what}: thresholds must be 1..8 strictly ascending distances of 0..32767 pixels, got {list(thresholds)}")
    host = (ctypes.c_int32 * len(thr))(*thr)  # read by the library during the call
    with torch.cuda.device(dev):
        if out is None:
            exposure = torch.empty((n, k, len(thr)), dtype=torch.int64, device=dev)
            near = torch.empty((n, cap, 8), dtype=torch.int64, device=dev)
        else:
            exposure, near = out
            if (exposure.dtype != torch.int64 or tuple(exposure.shape) != (n, k, len(thr)) or not exposure.is_contiguous() or near.dtype != torch.int64
                    or tuple(near.shape) != (n, cap, 8) or not near.is_contiguous()):
                raise ValueError(f"{what}: out must be contiguous int64 [{n},{k},{len(thr)}] and [{n},{cap},8] tensors")
        if n:
            check(lib.fs_region_proximity(ptr(mask.contiguous()), ptr(d2.contiguous()), ptr(None if nearest is None else nearest.contiguous()),
                                          ptr(index.contiguous()), ptr(counts.contiguous()), n, h, w, k, cap, bits,
                                          ctypes.cast(host, ctypes.c_void_p), len(thr), ptr(exposure), ptr(near), stream_ptr()))
    return exposure, near


# ------------------------------------------------------------------------------------------ dry-route reachability
ACCESS_NONE = 0xFFFFFFFF  # FS_ACCESS_NONE; the int32 tensors that carry d show it as -1
ACCESS_TILE = 32  # FS_ACCESS_TILE
ACCESS_MAX_COST = 2 ** 31 - 4096  # FS_ACCESS_MAX_COST
ACCESS_ROUNDS = 64  # rounds per call by default: a guess (an open field needs about one per tile the route crosses)


def mask_access_workspace_bytes(n, h, w):
    """FS_MASK_ACCESS_WORKSPACE_BYTES of include/floodseg_test.h: one 64-bit key per pixel, two dwords per tile, four per frame."""
    return n * h * w * 8 + n * (-(-h // ACCESS_TILE)) * (-(-w // ACCESS_TILE)) * 8 + n * 16


def access_cost_table(cost, what="floodseg.mask_access"):
    """A cost argument -> the 32 bytes the library reads: a mapping {class id: cost} or a sequence of up to 32 costs, each 0..255."""
    items = list(cost.items()) if hasattr(cost, "items") else list(enumerate(cost))
    table = [0] * 32
    for k, c in items:
        if not 0 <= int(k) <= 31 or not 0 <= int(c) <= 255:
            raise ValueError(f"{what}: cost must map class ids 0..31 to 0..255, got {cost}")
        table[int(k)] = int(c)
    if not any(table):
        raise ValueError(f"{what}: the cost table is all zero (cost[k] > 0: class k can be walked on)")
    return table


def mask_access(mask, seeds, cost, terminal=(), connectivity=8, max_cost=0, rounds=ACCESS_ROUNDS, resume=None, want_origin=True, out=None):
    """The cheapest route from any seed pixel to every pixel of its frame over ground that can be walked on (definition:
    include/floodseg_test.h, mask_access): uint8 masks and seed planes [n,H,W] -> (d, origin, status).  cost: {class id:
    0..255} or a sequence, 0 = barrier (ids >= 32 always are); terminal: classes that can be arrived at but not crossed.  A move
    costs 5 (orthogonal) or 7 (diagonal, connectivity 8, no corner cutting) times the sum of the two pixels' costs.  d: int32 [n,H,W]
    holding the uint32 values (0 on a seed that counts; FS_ACCESS_NONE, read as -1, where no route exists or it costs more than
    max_cost).  origin: int32 [n,H,W], the raster index of the seed the route starts from, the smallest among several, -1 where d is
    FS_ACCESS_NONE; None with want_origin=False.  status: int32 [n,4] = (converged, rounds that lowered a value, pixels with a value,
    0), on the device.  The call enqueues `rounds` rounds and reads nothing back: where status says 0 the values are upper bounds --
    costs of real routes -- and resume=(d, origin) of that call continues in place towards the same result.  out: caller-owned contiguous
    (d, origin) destinations.  The workspace is allocated here.  The default of `rounds` is a guess."""
    lib = _lib.load()
    what = "floodseg.mask_access"
    if resume is not None and out is not None:
        raise ValueError(f"{what}: give resume or out, not both (a resumed call writes the planes it resumes from)")
    planes = resume if resume is not None else out
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise ValueError(f"{what}: mask must be uint8 [n,H,W], got {mask.dtype} {tuple(mask.shape)}")
    if seeds.dtype != torch.uint8 or seeds.shape != mask.shape:
        raise ValueError(f"{what}: seeds must be uint8 of the mask's shape {tuple(mask.shape)}, got {seeds.dtype} {tuple(seeds.shape)}")
    n, h, w = mask.shape
    if not 1 <= h <= 32768 or not 1 <= w <= 32768 or n > 65535 or h * w >= 2 ** 31 - 1:
        raise ValueError(f"{what}: at most 65535 frames of 1..32768 pixels a side, got {tuple(mask.shape)}")
    table = access_cost_table(cost, what)
    bits = class_set(terminal, "terminal", what, allow_empty=True)
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity}")
    if not 0 <= int(max_cost) <= ACCESS_MAX_COST:
        raise ValueError(f"{what}: max_cost must be 0..{ACCESS_MAX_COST} (0: the largest), got {max_cost}")
    if not 1 <= int(rounds) <= 65535:
        raise ValueError(f"{what}: rounds must be 1..65535, got {rounds}")
    host = (ctypes.c_uint8 * 32)(*table)  # read by the library during the call
    if planes is not None:
        for t, name in zip(planes, ("d", "origin")):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (n, h, w) or not t.is_contiguous()):
                raise ValueError(f"{what}: the {name} plane must be a contiguous int32 [{n},{h},{w}] tensor, got {t.dtype} {tuple(t.shape)}")
        if planes[0] is None or (planes[1] is not None) != bool(want_origin):
            raise ValueError(f"{what}: (d, origin) must hold d, and an origin plane exactly when want_origin is set")
    dev = one_device(mask, seeds, *(planes or ()), what=what)
    with torch.cuda.device(dev):
        if planes is None:
            d = torch.empty((n, h, w), dtype=torch.int32, device=dev)
            origin = torch.empty((n, h, w), dtype=torch.int32, device=dev) if want_origin else None
        else:
            d, origin = planes
        status = torch.empty((n, 4), dtype=torch.int32, device=dev)
        if n:
            work = torch.empty((mask_access_workspace_bytes(n, h, w) // 8,), dtype=torch.int64, device=dev)
            check(lib.fs_mask_access(ptr(mask.contiguous()), ptr(seeds.contiguous()), n, h, w, ctypes.cast(host, ctypes.c_void_p), bits, int(connectivity),
                                     int(max_cost), int(rounds), int(resume is not None), ptr(d), ptr(origin), ptr(status), ptr(work), stream_ptr()))
    return d, origin, status


def region_access(mask, d, origin, index, counts, classes, max_regions, out=None):
    """mask_access' field tabulated per class and per region (definition: include/floodseg_test.h, region_access):
    -> (reach int64 [n,classes,4], rows int64 [n,max_regions,8]).  reach[f][k] = (pixels of class k, those with a value, the sum of
    their values, the largest).  rows, one per row of region_table's table (index, counts): (min_d, at_x, at_y, origin_x, origin_y,
    origin_row, valued pixels, max_d) -- the region's cheapest pixel (lowest raster index), the seed its route starts from and that
    seed's region row (-1: none; all three -1 with origin=None); a region no pixel of which has a value: (-1, -1, -1, -1, -1, -1, 0, -1).
    out: caller-owned contiguous (reach, rows) destinations; they are written whole."""
    lib = _lib.load()
    what = "floodseg.region_access"
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise ValueError(f"{what}: mask must be uint8 [n,H,W], got {mask.dtype} {tuple(mask.shape)}")
    n, h, w = mask.shape
    if not 1 <= h <= 32768 or not 1 <= w <= 32768 or n > 65535 or h * w >= 2 ** 31 - 1:
        raise ValueError(f"{what}: at most 65535 frames of 1..32768 pixels a side, got {tuple(mask.shape)}")
    for t, name in ((d, "d"), (origin, "origin"), (index, "index")):
        if (t is None and name != "origin") or (t is not None and (t.dtype != torch.int32 or t.shape != mask.shape)):
            raise ValueError(f"{what}: {name} must be int32 of the mask's shape {tuple(mask.shape)}, got "
                             f"{None if t is None else (t.dtype, tuple(t.shape))}")
    if counts.dtype != torch.int64 or tuple(counts.shape) != (n, 2):
        raise ValueError(f"{what}: counts must be int64 [{n},2] (region_table's), got {counts.dtype} {tuple(counts.shape)}")
    k, cap = int(classes), int(max_regions)
    if not 1 <= k <= 255 or not 1 <= cap <= 65536:
        raise ValueError(f"{what}: classes must be 1..255 and max_regions 1..65536, got {classes} and {max_regions}")
    if out is not None and (out[0].dtype != torch.int64 or tuple(out[0].shape) != (n, k, 4) or not out[0].is_contiguous() or out[1].dtype != torch.int64
                            or tuple(out[1].shape) != (n, cap, 8) or not out[1].is_contiguous()):
        raise ValueError(f"{what}: out must be contiguous int64 [{n},{k},4] and [{n},{cap},8] tensors")
    dev = one_device(mask, d, origin, index, counts, *(out or ()), what=what)
    with torch.cuda.device(dev):
        if out is None:
            reach = torch.empty((n, k, 4), dtype=torch.int64, device=dev)
            rows = torch.empty((n, cap, 8), dtype=torch.int64, device=dev)
        else:
            reach, rows = out
        if n:
            check(lib.fs_region_access(ptr(mask.contiguous()), ptr(d.contiguous()), ptr(None if origin is None else origin.contiguous()),
                                       ptr(index.contiguous()), ptr(counts.contiguous()), n, h, w, k, cap, ptr(reach), ptr(rows), stream_ptr()))
    return reach, rows


# ------------------------------------------------------------------------------------------ the flood-extent mosaic
POSE_ONE = 1 << 20  # 1 << FS_POSE_FRAC: poses and pair models are Q20
MOSAIC_MAX_SIDE = 16384


def _mosaic_size(size, name, what, lo=1):
    h, w = (int(v) for v in size)
    if not lo <= h <= MOSAIC_MAX_SIDE or not lo <= w <= MOSAIC_MAX_SIDE:
        raise ValueError(f"{what}: {name} must be (H, W) with {lo}..{MOSAIC_MAX_SIDE} pixels a side, got {tuple(size)}")
    return h, w


def _mosaic_origin(origin, what):
    oy, ox = (int(v) for v in origin)
    if abs(oy) > MOSAIC_MAX_SIDE or abs(ox) > MOSAIC_MAX_SIDE:
        raise ValueError(f"{what}: origin must be (oy, ox) within {MOSAIC_MAX_SIDE} pixels of the canvas corner, got {tuple(origin)}")
    return oy, ox


def _mosaic_rows(t, name, what, n=None):
    if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 16 or not 1 <= t.shape[0] <= 64 or (n is not None and t.shape[0] != n):
        raise ValueError(f"{what}: {name} must be int64 [{'n' if n is None else n},16] with n in 1..64, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def global_motion(tables, frame_size, mask_size, rounds=4, tol=1.0, min_inliers=12, mask=None, exclude=(), pair_stats=None):
    """One robust affine camera-motion model per frame pair from the block matcher's tables (definition: include/floodseg_test.h,
    global_motion): int32 tables [n,blocks,7] of frames of frame_size = (FH, FW) -> model int64 [n,16] = the forward affine
    (mask pixel of frame f -> mask pixel of frame f-1; six Q20 values), its inverse, status (0 ok, 1 cut, 2 too few, 3 degenerate or
    implausible), usable rows, inliers, rounds completed.  mask_size = (H, W) of the masks the model is for.  rounds 0..8 least-squares
    rounds from the vectors' mode (0: the mode translation); tol: the last round's inlier tolerance in frame pixels (0..64), doubled per
    round before it; min_inliers 3..2^20.  mask uint8 [n,H,W] with exclude = class ids 0..31: rows whose block centre lies on an excluded
    class do not count (water moves on its own).  pair_stats int32 [n,4]: a pair flagged as a cut is not fitted.  One launch; nothing is
    read back."""
    lib = _lib.load()
    what = "floodseg.global_motion"
    fh, fw = _mosaic_size(frame_size, "frame_size", what, 16)
    h, w = _mosaic_size(mask_size, "mask_size", what)
    if not 0 <= int(rounds) <= 8:
        raise ValueError(f"{what}: rounds must be 0..8, got {rounds}")
    if not 0 <= float(tol) <= 64:
        raise ValueError(f"{what}: tol must be 0..64 frame pixels, got {tol}")
    if not 3 <= int(min_inliers) <= 1 << 20:
        raise ValueError(f"{what}: min_inliers must be 3..2^20, got {min_inliers}")
    bits = class_set(exclude, "exclude", what, allow_empty=True)
    blocks = (fh // 16) * (fw // 16)
    if tables.dtype != torch.int32 or tables.dim() != 3 or not 1 <= tables.shape[0] <= 64 or tuple(tables.shape[1:]) != (blocks, 7):
        raise ValueError(f"{what}: tables must be int32 [n,{blocks},7] with n in 1..64 for frames of {fh}x{fw}, got {tables.dtype} {tuple(tables.shape)}")
    n = tables.shape[0]
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (n, h, w)):
        raise ValueError(f"{what}: mask must be uint8 [{n},{h},{w}], got {mask.dtype} {tuple(mask.shape)}")
    if pair_stats is not None and (pair_stats.dtype != torch.int32 or tuple(pair_stats.shape) != (n, 4)):
        raise ValueError(f"{what}: pair_stats must be int32 [{n},4], got {pair_stats.dtype} {tuple(pair_stats.shape)}")
    dev = one_device(tables, mask, pair_stats, what=what)
    with torch.cuda.device(dev):
        model = torch.empty((n, 16), dtype=torch.int64, device=dev)
        check(lib.fs_global_motion(ptr(tables.contiguous()), ptr(None if pair_stats is None else pair_stats.contiguous()),
                                   ptr(None if mask is None else mask.contiguous()), bits, n, fh, fw, h, w, int(rounds), int(round(float(tol) * POSE_ONE)),
                                   int(min_inliers), ptr(model), stream_ptr()))
    return model


def pose_chain(model, state, mask_size, canvas_size, origin, max_bridge=2):
    """global_motion's pair models composed into poses relative to the mosaic's anchor frame (definition: include/floodseg_test.h,
    pose_chain): model int64 [n,16], state int64 [32] (all zero: fresh; UPDATED IN PLACE, carry it from window to window) -> poses int64
    [n,16] = to_anchor (6), from_anchor (6), status (0 ok, 1 bridged, 2 lost), clipped, inliers, usable rows.  canvas_size = (CH, CW),
    origin = (oy, ox), the canvas pixel of the anchor's top-left corner; max_bridge 0..64 failed pairs running are bridged with the last
    good pair's model.  One launch of one wave; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.pose_chain"
    h, w = _mosaic_size(mask_size, "mask_size", what)
    ch, cw = _mosaic_size(canvas_size, "canvas_size", what)
    oy, ox = _mosaic_origin(origin, what)
    if not 0 <= int(max_bridge) <= 64:
        raise ValueError(f"{what}: max_bridge must be 0..64, got {max_bridge}")
    model = _mosaic_rows(model, "model", what)
    if state.dtype != torch.int64 or tuple(state.shape) != (32,) or not state.is_contiguous():
        raise ValueError(f"{what}: state must be a contiguous int64 [32] tensor, got {state.dtype} {tuple(state.shape)}")
    dev = one_device(model, state, what=what)
    with torch.cuda.device(dev):
        poses = torch.empty((model.shape[0], 16), dtype=torch.int64, device=dev)
        check(lib.fs_pose_chain(ptr(model), ptr(state), ptr(poses), model.shape[0], h, w, ch, cw, ox, oy, int(max_bridge), stream_ptr()))
    return poses


def _mosaic_votes(votes, what):
    if votes.dtype != torch.uint16 or votes.dim() != 3 or not 1 <= votes.shape[0] <= 32 or not votes.is_contiguous():
        raise ValueError(f"{what}: votes must be a contiguous uint16 [K,CH,CW] tensor with K in 1..32, got {votes.dtype} {tuple(votes.shape)}")
    _mosaic_size(votes.shape[1:], "the canvas", what)
    return votes


def mosaic_accumulate(mask, poses, votes, origin):
    """The masks of n frames gathered into the vote canvas (definition: include/floodseg_test.h, mosaic_accumulate): uint8 mask [n,H,W],
    pose_chain's poses int64 [n,16], votes uint16 [K,CH,CW] UPDATED IN PLACE (and returned): every canvas pixel looks up, per frame that
    is not lost, the frame pixel under its centre and gives that pixel's class one vote, saturating at 65535.  origin = (oy, ox).  One
    launch that costs the frames' footprint, not the canvas; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.mosaic_accumulate"
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise ValueError(f"{what}: mask must be uint8 [n,H,W], got {mask.dtype} {tuple(mask.shape)}")
    n = mask.shape[0]
    h, w = _mosaic_size(mask.shape[1:], "the mask", what)
    poses = _mosaic_rows(poses, "poses", what, n)
    votes = _mosaic_votes(votes, what)
    oy, ox = _mosaic_origin(origin, what)
    dev = one_device(mask, poses, votes, what=what)
    with torch.cuda.device(dev):
        check(lib.fs_mosaic_accumulate(ptr(mask.contiguous()), ptr(poses), n, h, w, votes.shape[0], votes.shape[1], votes.shape[2], ox, oy, ptr(votes),
                                       stream_ptr()))
    return votes


def mosaic_resolve(votes):
    """The vote canvas read out (definition: include/floodseg_test.h, mosaic_resolve): votes uint16 [K,CH,CW] -> (cls uint8 [CH,CW]: the
    class with the most votes, the lowest id on a tie, 255 where unseen; conf uint8: the winner's share of the votes as a code 0..255;
    seen int32 [CH,CW]: the votes; totals int64 [K,2]: per class the canvas pixels won and the votes received).  Nothing is read back."""
    lib = _lib.load()
    what = "floodseg.mosaic_resolve"
    votes = _mosaic_votes(votes, what)
    dev = one_device(votes, what=what)
    k, ch, cw = votes.shape
    with torch.cuda.device(dev):
        cls = torch.empty((ch, cw), dtype=torch.uint8, device=dev)
        conf = torch.empty((ch, cw), dtype=torch.uint8, device=dev)
        seen = torch.empty((ch, cw), dtype=torch.int32, device=dev)
        totals = torch.empty((k, 2), dtype=torch.int64, device=dev)
        check(lib.fs_mosaic_resolve(ptr(votes), k, ch, cw, ptr(cls), ptr(conf), ptr(seen), ptr(totals), stream_ptr()))
    return cls, conf, seen, totals


# ------------------------------------------------------------------------------------------ the orthophoto under the mosaic
ORTHO_MODES = {"centre": 0, "latest": 1}
FLOOD_PALETTE = ((0, 0, 0), (30, 95, 170), (65, 117, 5), (212, 98, 1), (255, 244, 116))  # dataset/flow/list/colors.txt; flow/predict.py's PALETTE is this table


def ortho_canvas(size, device):
    """A fresh orthophoto canvas of size = (CH, CW) on `device`: (rank int64 [CH,CW] holding the uint64 rank words, every bit set =
    empty; rgba int32 [CH,CW], zero = unseen) for ops.ortho_accumulate."""
    ch, cw = _mosaic_size(size, "size", "floodseg.ortho_canvas")
    return torch.full((ch, cw), -1, dtype=torch.int64, device=device), torch.zeros((ch, cw), dtype=torch.int32, device=device)


def _ortho_planes(rank, rgba, what):
    if rgba.dtype != torch.int32 or rgba.dim() != 2 or not rgba.is_contiguous():
        raise ValueError(f"{what}: rgba must be a contiguous int32 [CH,CW] tensor, got {rgba.dtype} {tuple(rgba.shape)}")
    if rank is not None and (rank.dtype != torch.int64 or tuple(rank.shape) != tuple(rgba.shape) or not rank.is_contiguous()):
        raise ValueError(f"{what}: rank must be a contiguous int64 {list(rgba.shape)} tensor like rgba, got {rank.dtype} {tuple(rank.shape)}")
    return _mosaic_size(rgba.shape, "the canvas", what)


def _ortho_source(source, what):
    """The checks ortho_accumulate makes of its 5-tuple, for the ops that take the same one -> (frame, chroma planes, fmt, matrix, full_range, fh, fw)."""
    if not isinstance(source, (tuple, list)) or len(source) != 5:
        raise ValueError(f"{what}: source must be the 5-tuple (frame, chroma, fmt, matrix, full_range), got a {type(source).__name__}"
                         + (f" of {len(source)}" if isinstance(source, (tuple, list)) else ""))
    frame, chroma, fmt, matrix, full_range = source
    if fmt not in _FORMATS:
        raise ValueError(f"{what}: fmt must be one of {sorted(_FORMATS)}, got {fmt!r}")
    if matrix not in _MATRICES:
        raise ValueError(f"{what}: matrix must be one of {sorted(_MATRICES)}, got {matrix!r}")
    planes = [] if chroma is None else list(chroma) if isinstance(chroma, (tuple, list)) else [chroma]
    if frame.dtype != torch.uint8 or any(p.dtype != torch.uint8 for p in planes):
        raise ValueError(f"{what}: frames must be uint8, got {[str(t.dtype) for t in [frame] + planes]}")
    rgb = fmt == "rgb24"
    if frame.dim() != (3 if rgb else 2) or (rgb and frame.shape[2] != 3):
        raise ValueError(f"{what}: a {fmt} frame must be {'[H,W,3]' if rgb else 'the Y plane [H,W]'}, got {tuple(frame.shape)}")
    fh, fw = _mosaic_size(frame.shape[:2], "the frame", what)
    want = [] if rgb else [((fh + 1) // 2, (fw + 1) // 2, 2)] if fmt == "nv12" else [((fh + 1) // 2, (fw + 1) // 2)] * 2
    if [tuple(p.shape) for p in planes] != want:
        raise ValueError(f"{what}: a {fh} x {fw} {fmt} frame takes chroma {want if want else None}, got {[tuple(p.shape) for p in planes]}")
    return frame, planes, fmt, matrix, full_range, fh, fw


def ortho_accumulate(source, pose, ordinal, mask_size, rank, rgba, origin, mode="centre"):
    """One frame's pixels gathered into the orthophoto canvas (definition: include/floodseg_test.h, ortho_accumulate).
    source = (frame, chroma, fmt, matrix, full_range) as the window datasets' source(f_id) returns it and prepare_frame takes it; the
    image sampled is that frame through prepare_frame's resize to mask_size = (H, W), as stored uint8.  pose: ONE row of pose_chain's
    output, int64 [16] on the device; ordinal: the frame's number since the anchor (0 .. 2^32 - 2).  rank, rgba: ortho_canvas's planes,
    UPDATED IN PLACE (and returned): a canvas pixel takes the frame's pixel where the frame's rank is strictly smaller -- mode "centre":
    the view in which the ground point is nearest the optical axis, ties to the earlier frame; "latest": the newest frame.  origin =
    (oy, ox) as mosaic_accumulate's.  One launch that costs the frame's footprint; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.ortho_accumulate"
    frame, planes, fmt, matrix, full_range, fh, fw = _ortho_source(source, what)
    if mode not in ORTHO_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(ORTHO_MODES)}, got {mode!r}")
    if not 0 <= int(ordinal) < 0xFFFFFFFF:
        raise ValueError(f"{what}: ordinal must be 0..{0xFFFFFFFF - 1}, got {ordinal}")
    h, w = _mosaic_size(mask_size, "mask_size", what)
    if pose.dtype != torch.int64 or tuple(pose.shape) != (16,) or not pose.is_contiguous():
        raise ValueError(f"{what}: pose must be one contiguous int64 [16] row of pose_chain's output, got {pose.dtype} {tuple(pose.shape)}")
    ch, cw = _ortho_planes(rank, rgba, what)
    oy, ox = _mosaic_origin(origin, what)
    dev = one_device(frame, pose, rank, rgba, *planes, what=what)
    with torch.cuda.device(dev):
        planes = [p.contiguous() for p in planes]
        check(lib.fs_ortho_accumulate(ptr(frame.contiguous()), ptr(planes[0]) if planes else None, ptr(planes[1]) if len(planes) > 1 else None, _FORMATS[fmt],
                                      _MATRICES[matrix], int(bool(full_range)), fh, fw, ptr(pose), int(ordinal), h, w, ORTHO_MODES[mode], ch, cw, ox, oy,
                                      ptr(rank), ptr(rgba), stream_ptr()))
    return rank, rgba


def ortho_compose(rgba, cls=None, palette=FLOOD_PALETTE, alpha=None, fill=(0, 0, 0), edge=()):
    """The orthophoto canvas drawn, optionally with the extent map over it (definition: include/floodseg_test.h, ortho_compose): rgba
    int32 [CH,CW] of ortho_accumulate, cls = mosaic_resolve's uint8 class plane or None (the plain orthophoto) -> uint8 [CH,CW,3].
    Unseen ground shows fill = (r, g, b).  palette: uint8 [K,3] with alpha (0..255, default 96) or [K,4] as compose_frame takes it;
    a class below K is blended over the imagery, 255 (never seen) and any id >= K leave it as it is.  edge: class ids (below min(K, 32))
    that get a one-pixel opaque line along the inside of their boundary with other seen classes.  One launch; nothing is read back."""
    import numpy as np

    lib = _lib.load()
    what = "floodseg.ortho_compose"
    ch, cw = _ortho_planes(None, rgba, what)
    if cls is not None and (cls.dtype != torch.uint8 or tuple(cls.shape) != (ch, cw)):
        raise ValueError(f"{what}: cls must be uint8 [{ch},{cw}] like rgba, got {cls.dtype} {tuple(cls.shape)}")
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError(f"{what}: fill must be (r, g, b) with 0..255 each, got {fill}")
    if isinstance(palette, torch.Tensor):
        pal = palette.detach().cpu().numpy()
    else:
        pal = np.asarray(palette) if hasattr(palette, "dtype") else np.asarray(palette, dtype=np.int64)
        if not hasattr(palette, "dtype") and pal.size and 0 <= pal.min() and pal.max() <= 255:
            pal = pal.astype(np.uint8)  # a plain sequence of 0..255 values
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] not in (3, 4) or not 1 <= pal.shape[0] <= 256:
        raise ValueError(f"{what}: palette must be uint8 [K,3] or [K,4] with 1 <= K <= 256, got {pal.dtype} {pal.shape}")
    if pal.shape[1] == 4 and alpha is not None:
        raise ValueError(f"{what}: alpha={alpha} goes with a [K,3] palette; a [K,4] palette carries its own opacities")
    if pal.shape[1] == 3:
        alpha = 96 if alpha is None else int(alpha)
        if not 0 <= alpha <= 255:
            raise ValueError(f"{what}: alpha must be 0..255, got {alpha}")
    k = pal.shape[0]
    edge = tuple(int(c) for c in edge)
    if any(not 0 <= c < min(k, 32) for c in edge):
        raise ValueError(f"{what}: edge must hold class ids 0..{min(k, 32) - 1}, got {edge}")
    bits = sum(1 << c for c in set(edge))
    dev = one_device(rgba, cls, what=what)
    with torch.cuda.device(dev):
        pal = _palette_rgba(dev, pal, alpha if pal.shape[1] == 3 else None, False)
        out = torch.empty((ch, cw, 3), dtype=torch.uint8, device=dev)
        check(lib.fs_ortho_compose(ptr(rgba), ptr(None if cls is None else cls.contiguous()), ptr(pal), k, bits, fill[0] | fill[1] << 8 | fill[2] << 16, ch, cw,
                                   ptr(out), stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ frame-to-map registration
def map_view(source, pose, ordinal, mask_size, rank, rgba, origin, min_age=0):
    """The orthophoto canvas as this frame should see it under its predicted pose (definition: include/floodseg_test.h, map_view;
    DESIGN §3.20).  source, pose (ONE row of pose_chain's output), ordinal, mask_size = (H, W), rank, rgba and origin = (oy, ox) as
    ops.ortho_accumulate takes them; the canvas is only read.  -> (cur, view, valid), uint8 [H,W] each: the frame's own luma (of the
    image ortho_accumulate samples), the luma of the canvas pixel under each frame pixel, and 1 where that canvas pixel exists, has been
    seen and -- with min_age > 0 -- belongs to a frame at least min_age ordinals older (0 elsewhere, and everywhere for a lost pose).
    block_match_modes(cur, view) then finds how far the frame lies from where the chain put it.  One launch; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.map_view"
    frame, planes, fmt, matrix, full_range, fh, fw = _ortho_source(source, what)
    if not 0 <= int(ordinal) < 0xFFFFFFFF:
        raise ValueError(f"{what}: ordinal must be 0..{0xFFFFFFFF - 1}, got {ordinal}")
    if not 0 <= int(min_age) < 1 << 31:
        raise ValueError(f"{what}: min_age must be 0..2^31 - 1 frames, got {min_age}")
    h, w = _mosaic_size(mask_size, "mask_size", what, 16)
    if pose.dtype != torch.int64 or tuple(pose.shape) != (16,) or not pose.is_contiguous():
        raise ValueError(f"{what}: pose must be one contiguous int64 [16] row of pose_chain's output, got {pose.dtype} {tuple(pose.shape)}")
    ch, cw = _ortho_planes(rank, rgba, what)
    oy, ox = _mosaic_origin(origin, what)
    dev = one_device(frame, pose, rank, rgba, *planes, what=what)
    with torch.cuda.device(dev):
        planes = [p.contiguous() for p in planes]
        cur, view, valid = (torch.empty((h, w), dtype=torch.uint8, device=dev) for _ in range(3))
        check(lib.fs_map_view(ptr(frame.contiguous()), ptr(planes[0]) if planes else None, ptr(planes[1]) if len(planes) > 1 else None, _FORMATS[fmt],
                              _MATRICES[matrix], int(bool(full_range)), fh, fw, ptr(pose), int(ordinal), h, w, ch, cw, ox, oy, ptr(rank), ptr(rgba),
                              int(min_age), ptr(cur), ptr(view), ptr(valid), stream_ptr()))
    return cur, view, valid


def map_gate(table, valid):
    """The matcher's table of (cur, view) gated IN PLACE (and returned) by map_view's valid plane (definition: include/floodseg_test.h,
    map_gate): int32 table [(H//16) * (W//16), 7], uint8 valid [H,W].  A row stays iff its winner's 16 x 16 window lies wholly on valid
    pixels; every other row becomes the void row.  One launch; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.map_gate"
    if valid.dtype != torch.uint8 or valid.dim() != 2 or not valid.is_contiguous():
        raise ValueError(f"{what}: valid must be a contiguous uint8 [H,W] tensor, got {valid.dtype} {tuple(valid.shape)}")
    h, w = _mosaic_size(valid.shape, "valid", what, 16)
    blocks = (h // 16) * (w // 16)
    if table.dtype != torch.int32 or tuple(table.shape) != (blocks, 7) or not table.is_contiguous():
        raise ValueError(f"{what}: table must be a contiguous int32 [{blocks},7] tensor for a {h} x {w} plane, got {table.dtype} {tuple(table.shape)}")
    dev = one_device(table, valid, what=what)
    with torch.cuda.device(dev):
        check(lib.fs_map_gate(ptr(table), blocks, ptr(valid), h, w, stream_ptr()))
    return table


def pose_correct(model, state, pose, mask_size, canvas_size, origin):
    """global_motion's fit of a frame against its map_view folded into the pose chain (definition: include/floodseg_test.h,
    pose_correct): model int64 [16] or [1,16], state int64 [32] (pose_chain's) and pose int64 [16] (the frame's row) are UPDATED IN
    PLACE where the fit is good -> out int64 [8] = (status, usable rows, inliers, rounds done, the fit's shift x and y in Q20, 0, 0);
    status 0 corrected, 2 no fit, 3 the corrected pose would leave the pose bounds, 4 the chain is not tracking this row.  One launch
    of one wave; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.pose_correct"
    h, w = _mosaic_size(mask_size, "mask_size", what)
    ch, cw = _mosaic_size(canvas_size, "canvas_size", what)
    oy, ox = _mosaic_origin(origin, what)
    if model.dtype != torch.int64 or tuple(model.shape) not in ((16,), (1, 16)) or not model.is_contiguous():
        raise ValueError(f"{what}: model must be one contiguous int64 [16] row of global_motion's output, got {model.dtype} {tuple(model.shape)}")
    if state.dtype != torch.int64 or tuple(state.shape) != (32,) or not state.is_contiguous():
        raise ValueError(f"{what}: state must be a contiguous int64 [32] tensor, got {state.dtype} {tuple(state.shape)}")
    if pose.dtype != torch.int64 or tuple(pose.shape) != (16,) or not pose.is_contiguous():
        raise ValueError(f"{what}: pose must be one contiguous int64 [16] row of pose_chain's output, got {pose.dtype} {tuple(pose.shape)}")
    dev = one_device(model, state, pose, what=what)
    with torch.cuda.device(dev):
        out = torch.empty((8,), dtype=torch.int64, device=dev)
        check(lib.fs_pose_correct(ptr(model), ptr(state), ptr(pose), h, w, ch, cw, ox, oy, ptr(out), stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ relocalisation against the orthophoto
RELOCATE_SCALES = (4, 8, 16)
RELOCATE_PATCH_BYTES = 65536  # FS map_patch: tl and tv, of which the first tw * th bytes are written


def _relocate_scale(scale, what):
    if scale not in RELOCATE_SCALES:
        raise ValueError(f"{what}: scale must be one of {list(RELOCATE_SCALES)}, got {scale!r}")
    return int(scale)


def _relocate_row(t, words, name, what):
    if t.dtype != torch.int64 or tuple(t.shape) != (words,) or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous int64 [{words}] tensor, got {t.dtype} {tuple(t.shape)}")


def map_coarse(rgba, scale):
    """The orthophoto canvas reduced to scale x scale cells (definition: include/floodseg_test.h, map_coarse): rgba uint32
    (held as int32) [CH,CW] -> (cl, cv) uint8 [CH // scale, CW // scale]: a cell is valid (cv 1) iff every one of its pixels has been
    seen, and cl is then the rounded mean of their lumas; 0, 0 otherwise.  One launch; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.map_coarse"
    if rgba.dtype != torch.int32 or rgba.dim() != 2 or not rgba.is_contiguous():
        raise ValueError(f"{what}: rgba must be a contiguous int32 [CH,CW] tensor (ortho_canvas's), got {rgba.dtype} {tuple(rgba.shape)}")
    ch, cw = _mosaic_size(rgba.shape, "the canvas", what)
    s = _relocate_scale(scale, what)
    if ch // s < 1 or cw // s < 1:
        raise ValueError(f"{what}: a {ch} x {cw} canvas has no cell of scale {s}")
    dev = one_device(rgba, what=what)
    with torch.cuda.device(dev):
        cl, cv = (torch.empty((ch // s, cw // s), dtype=torch.uint8, device=dev) for _ in range(2))
        check(lib.fs_map_coarse(ptr(rgba), ch, cw, s, ptr(cl), ptr(cv), stream_ptr()))
    return cl, cv


def map_patch(source, state, mask_size, canvas_size, origin, scale):
    """A lost frame drawn into canvas cells with the last pose the chain's state holds (definition: include/floodseg_test.h, map_patch).
    source, mask_size = (H, W), origin = (oy, ox) as ops.map_view takes them; state: pose_chain's int64 [32], only read.  -> (tl, tv,
    geom): uint8 [65536] each, of which the first tw * th bytes are the patch's lumas and validity as [th, tw], and int64 [8] =
    (status, pu0, pv0, tw, th, valid cells, 0, 0); status 0 drawn, 1 the chain is not lost, 2 its poses are out of bounds, 3 / 4 the
    patch has no or too many cells / more cells than the coarse canvas.  Two launches; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.map_patch"
    frame, planes, fmt, matrix, full_range, fh, fw = _ortho_source(source, what)
    h, w = _mosaic_size(mask_size, "mask_size", what)
    ch, cw = _mosaic_size(canvas_size, "canvas_size", what)
    oy, ox = _mosaic_origin(origin, what)
    s = _relocate_scale(scale, what)
    if ch // s < 1 or cw // s < 1:
        raise ValueError(f"{what}: a {ch} x {cw} canvas has no cell of scale {s}")
    _relocate_row(state, 32, "state", what)
    dev = one_device(frame, state, *planes, what=what)
    with torch.cuda.device(dev):
        planes = [p.contiguous() for p in planes]
        tl, tv = (torch.empty((RELOCATE_PATCH_BYTES,), dtype=torch.uint8, device=dev) for _ in range(2))
        geom = torch.empty((8,), dtype=torch.int64, device=dev)
        check(lib.fs_map_patch(ptr(frame.contiguous()), ptr(planes[0]) if planes else None, ptr(planes[1]) if len(planes) > 1 else None, _FORMATS[fmt],
                               _MATRICES[matrix], int(bool(full_range)), fh, fw, ptr(state), h, w, ch, cw, ox, oy, s, ptr(tl), ptr(tv), ptr(geom), stream_ptr()))
    return tl, tv, geom


def map_locate(cl, cv, tl, tv, geom, min_overlap_permille=500, exclude=2):
    """The patch slid over the whole coarse canvas in whole cells (definition: include/floodseg_test.h, map_locate): cl, cv map_coarse's,
    tl, tv, geom map_patch's -> found int64 [16] = (status, u*, v*, sad*, n*, runner-up exists, u2, v2, sad2, n2, placements, eligible
    placements, valid patch cells, 0, 0, 0); status 0 found, 1 no eligible placement, 2 bad geom.  A placement is eligible with at
    least min_overlap_permille / 1000 of the patch's valid cells on valid canvas cells; the best has the smallest mean absolute
    difference; the runner-up is the best more than `exclude` cells from it.  Two launches; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.map_locate"
    if cl.dtype != torch.uint8 or cl.dim() != 2 or not cl.is_contiguous() or cv.dtype != torch.uint8 or tuple(cv.shape) != tuple(cl.shape) or not cv.is_contiguous():
        raise ValueError(f"{what}: cl and cv must be contiguous uint8 planes of one shape, got {cl.dtype} {tuple(cl.shape)} and {cv.dtype} {tuple(cv.shape)}")
    ch, cw = (int(v) for v in cl.shape)
    if not (1 <= ch <= 4096 and 1 <= cw <= 4096):
        raise ValueError(f"{what}: the coarse canvas must be 1..4096 cells a side, got {(ch, cw)}")
    for name, t in (("tl", tl), ("tv", tv)):
        if t.dtype != torch.uint8 or tuple(t.shape) != (RELOCATE_PATCH_BYTES,) or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be map_patch's contiguous uint8 [{RELOCATE_PATCH_BYTES}] tensor, got {t.dtype} {tuple(t.shape)}")
    _relocate_row(geom, 8, "geom", what)
    if not 1 <= int(min_overlap_permille) <= 1000:
        raise ValueError(f"{what}: min_overlap_permille must be 1..1000, got {min_overlap_permille}")
    if not 0 <= int(exclude) <= 64:
        raise ValueError(f"{what}: exclude must be 0..64 cells, got {exclude}")
    dev = one_device(cl, cv, tl, tv, geom, what=what)
    with torch.cuda.device(dev):
        scores = torch.empty((ch, cw, 2), dtype=torch.int32, device=dev)
        found = torch.empty((16,), dtype=torch.int64, device=dev)
        check(lib.fs_map_locate(ptr(cl), ptr(cv), ch, cw, ptr(tl), ptr(tv), ptr(geom), int(min_overlap_permille), int(exclude), ptr(scores), ptr(found), stream_ptr()))
    return found


def pose_relocate(found, state, mask_size, canvas_size, origin, scale, max_mean=16, ratio_permille=800):
    """map_locate's placement as a CANDIDATE state and pose row (definition: include/floodseg_test.h, pose_relocate); `state` is only
    read.  -> (cand_state int64 [32], cand_pose int64 [16]).  Accepted iff found, sad* <= max_mean n*, and no runner-up or
    1000 sad* n2 <= ratio_permille sad2 n*: the candidate is then the state with both poses translated by (scale u*, scale v*) canvas
    pixels, tracking, its last pair motion the identity; otherwise the state and a lost row.  cand_state[28] holds the decision
    (relocate_commit's status codes).  One launch; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.pose_relocate"
    h, w = _mosaic_size(mask_size, "mask_size", what)
    ch, cw = _mosaic_size(canvas_size, "canvas_size", what)
    oy, ox = _mosaic_origin(origin, what)
    s = _relocate_scale(scale, what)
    if not 0 <= int(max_mean) <= 255:
        raise ValueError(f"{what}: max_mean must be 0..255, got {max_mean}")
    if not 1 <= int(ratio_permille) <= 1000:
        raise ValueError(f"{what}: ratio_permille must be 1..1000, got {ratio_permille}")
    _relocate_row(found, 16, "found", what)
    _relocate_row(state, 32, "state", what)
    dev = one_device(found, state, what=what)
    with torch.cuda.device(dev):
        cand_state = torch.empty((32,), dtype=torch.int64, device=dev)
        cand_pose = torch.empty((16,), dtype=torch.int64, device=dev)
        check(lib.fs_pose_relocate(ptr(found), ptr(state), ptr(cand_state), ptr(cand_pose), int(max_mean), int(ratio_permille), h, w, ch, cw, ox, oy, s, stream_ptr()))
    return cand_state, cand_pose


def relocate_commit(cand_state, cand_pose, correct_out, state, pose, found, scale):
    """The candidate replaces the chain's state and the frame's pose row, IN PLACE, iff pose_relocate accepted the placement and
    pose_correct then reported 0 on the candidate (definition: include/floodseg_test.h, relocate_commit); otherwise nothing changes.
    -> out int64 [8] = (status, scale u*, scale v*, sad*, n*, sad2, n2, eligible placements); status 0 relocated, 1 not attempted (the
    chain is not lost), 2 no placement, 3 rejected by the mean, 4 rejected by uniqueness, 5 the fine registration failed, 6 the patch
    was refused, 7 out of the pose bounds.  One launch; the decision is taken on the device, nothing is read back."""
    lib = _lib.load()
    what = "floodseg.relocate_commit"
    s = _relocate_scale(scale, what)
    for name, t, words in (("cand_state", cand_state, 32), ("cand_pose", cand_pose, 16), ("correct_out", correct_out, 8), ("state", state, 32), ("pose", pose, 16),
                           ("found", found, 16)):
        _relocate_row(t, words, name, what)
    dev = one_device(cand_state, cand_pose, correct_out, state, pose, found, what=what)
    with torch.cuda.device(dev):
        out = torch.empty((8,), dtype=torch.int64, device=dev)
        check(lib.fs_relocate_commit(ptr(cand_state), ptr(cand_pose), ptr(correct_out), ptr(state), ptr(pose), ptr(found), s, ptr(out), stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ map-to-map registration, the merge of two mosaics
LINK_REGISTERED, LINK_INITIAL, LINK_NO_FIT, LINK_OUT_OF_BOUNDS = 0, 1, 2, 3  # word 12 of a link


def mosaic_link(b_to_a=None, a_to_b=None, status=LINK_INITIAL, device=None):
    """A link row, int64 [16], on `device`: b_to_a and a_to_b as six Q20 integers each (default: the identity), the status (default 1:
    a guess that ops.register_mosaics has yet to confirm), zeros."""
    ident = [POSE_ONE, 0, 0, 0, POSE_ONE, 0]
    fwd, back = (ident if m is None else [int(v) for v in m] for m in (b_to_a, a_to_b))
    if len(fwd) != 6 or len(back) != 6:
        raise ValueError(f"floodseg.mosaic_link: b_to_a and a_to_b must hold six Q20 integers each, got {len(fwd)} and {len(back)}")
    if int(status) not in (LINK_REGISTERED, LINK_INITIAL, LINK_NO_FIT, LINK_OUT_OF_BOUNDS):
        raise ValueError(f"floodseg.mosaic_link: status must be 0..3, got {status!r}")
    return torch.tensor(fwd + back + [int(status), 0, 0, 0], dtype=torch.int64, device=device)


def _merge_window(window, canvas, what):
    ch, cw = canvas
    if window is None:
        window = (0, 0, ch // 16 * 16, cw // 16 * 16)
    if len(window) != 4:
        raise ValueError(f"{what}: window must be (Y0, X0, WH, WW), got {tuple(window)}")
    y0, x0, wh, ww = (int(v) for v in window)
    if wh < 16 or ww < 16 or wh % 16 or ww % 16 or y0 < 0 or x0 < 0 or y0 + wh > ch or x0 + ww > cw:
        raise ValueError(f"{what}: window must be (Y0, X0, WH, WW) of whole blocks of 16 (at least one) inside the {ch} x {cw} canvas, got {(y0, x0, wh, ww)}")
    return y0, x0, wh, ww


def _same_memory(a, b):
    return a.data_ptr() == b.data_ptr()


def merge_view(rgba_a, origin_a, rgba_b, origin_b, link, window=None):
    """Two orthophoto canvases as the block matcher should see them (definition: include/floodseg_test.h, merge_view).
    rgba_a, rgba_b: int32 [CH,CW] of ortho_canvas, only read; origin_* = (oy, ox); link int64 [16] (ops.mosaic_link); window = (Y0, X0,
    WH, WW) of A's canvas in whole blocks of 16, default the whole canvas cut down to multiples of 16.  -> (cur, view, valid_a, valid_b)
    uint8 [WH,WW]: A's luma and where A has been seen; the luma of the B pixel under each A pixel and 1 where that pixel exists and
    has been seen (0 elsewhere, and everywhere for a link that is neither registered nor initial or is out of bounds).  One launch;
    nothing is read back."""
    lib = _lib.load()
    what = "floodseg.merge_view"
    ch_a, cw_a = _ortho_planes(None, rgba_a, what)
    ch_b, cw_b = _ortho_planes(None, rgba_b, what)
    oy_a, ox_a = _mosaic_origin(origin_a, what)
    oy_b, ox_b = _mosaic_origin(origin_b, what)
    _relocate_row(link, 16, "link", what)
    y0, x0, wh, ww = _merge_window(window, (ch_a, cw_a), what)
    if _same_memory(rgba_a, rgba_b):
        raise ValueError(f"{what}: A and B are the same memory (rgba at {rgba_a.data_ptr():#x})")
    dev = one_device(rgba_a, rgba_b, link, what=what)
    with torch.cuda.device(dev):
        cur, view, valid_a, valid_b = (torch.empty((wh, ww), dtype=torch.uint8, device=dev) for _ in range(4))
        check(lib.fs_merge_view(ptr(rgba_a), ch_a, cw_a, ox_a, oy_a, ptr(rgba_b), ch_b, cw_b, ox_b, oy_b, ptr(link), y0, x0, wh, ww, ptr(cur), ptr(view),
                                ptr(valid_a), ptr(valid_b), stream_ptr()))
    return cur, view, valid_a, valid_b


def merge_gate(table, valid_a, valid_b):
    """The matcher's table of merge_view's (cur, view) gated IN PLACE (and returned) (definition: include/floodseg_test.h, merge_gate):
    int32 table [(H//16) * (W//16), 7], uint8 valid_a, valid_b [H,W].  A row stays iff the block's own 16 x 16 window lies wholly on
    valid_a and its winner's window wholly on valid_b; every other row becomes the void row.  One launch; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.merge_gate"
    if valid_a.dtype != torch.uint8 or valid_a.dim() != 2 or not valid_a.is_contiguous():
        raise ValueError(f"{what}: valid_a must be a contiguous uint8 [H,W] tensor, got {valid_a.dtype} {tuple(valid_a.shape)}")
    if valid_b.dtype != torch.uint8 or tuple(valid_b.shape) != tuple(valid_a.shape) or not valid_b.is_contiguous():
        raise ValueError(f"{what}: valid_b must be a contiguous uint8 {list(valid_a.shape)} tensor like valid_a, got {valid_b.dtype} {tuple(valid_b.shape)}")
    h, w = _mosaic_size(valid_a.shape, "valid_a", what, 16)
    blocks = (h // 16) * (w // 16)
    if table.dtype != torch.int32 or tuple(table.shape) != (blocks, 7) or not table.is_contiguous():
        raise ValueError(f"{what}: table must be a contiguous int32 [{blocks},7] tensor for a {h} x {w} plane, got {table.dtype} {tuple(table.shape)}")
    dev = one_device(table, valid_a, valid_b, what=what)
    with torch.cuda.device(dev):
        check(lib.fs_merge_gate(ptr(table), blocks, ptr(valid_a), ptr(valid_b), h, w, stream_ptr()))
    return table


def link_correct(model, link, window, origin_a):
    """global_motion's fit of merge_view's (cur, view), with frame_size = mask_size = the window, folded into the link IN PLACE
    (definition: include/floodseg_test.h, link_correct): model int64 [16] or [1,16]; window = (Y0, X0, WH, WW) the view was drawn for;
    origin_a = (oy, ox) of A.  -> out int64 [8] = (status, usable rows, inliers, rounds done, the fit's shift x and y in Q20, 0, 0);
    status 0 corrected (the link's status becomes 0), 2 no fit, 3 out of the pose bounds, 4 the link was neither registered nor
    initial; on 2, 3 and 4 the link is unchanged.  One launch of one wave; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.link_correct"
    if model.dtype != torch.int64 or tuple(model.shape) not in ((16,), (1, 16)) or not model.is_contiguous():
        raise ValueError(f"{what}: model must be one contiguous int64 [16] row of global_motion's output, got {model.dtype} {tuple(model.shape)}")
    _relocate_row(link, 16, "link", what)
    y0, x0, wh, ww = _merge_window(window, (MOSAIC_MAX_SIDE, MOSAIC_MAX_SIDE), what)
    oy, ox = _mosaic_origin(origin_a, what)
    dev = one_device(model, link, what=what)
    with torch.cuda.device(dev):
        out = torch.empty((8,), dtype=torch.int64, device=dev)
        check(lib.fs_link_correct(ptr(model), ptr(link), y0, x0, wh, ww, ox, oy, ptr(out), stream_ptr()))
    return out


def mosaic_merge(votes_a, origin_a, votes_b, origin_b, link, ortho_a=None, ortho_b=None, ordinal_offset=0, mode="centre"):
    """Mosaic B folded into mosaic A, IN PLACE, under a registered link (definition: include/floodseg_test.h, mosaic_merge).  votes_a,
    votes_b: uint16 [K,CH,CW] with one K; origin_* = (oy, ox); ortho_a, ortho_b: (rank, rgba) of ortho_canvas, both or neither.  Every A
    canvas pixel adds the votes of the B pixel under it (saturating at 65535) and takes B's orthophoto pixel where B's rank, with
    ordinal_offset added to its ordinal (mode "latest": and its key rebuilt from it), is strictly smaller than A's.  A link whose
    status is not 0 changes nothing; that is decided on the device.  -> counts int64 [8] = (link status, A pixels B reached, pixels
    that received a vote, votes added before saturation, orthophoto pixels taken, 0, 0, 0).  VOTES ARE NOT IDEMPOTENT: a second call
    adds B's votes again (the orthophoto is unchanged by it).  Two launches; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.mosaic_merge"
    votes_a, votes_b = _mosaic_votes(votes_a, what), _mosaic_votes(votes_b, what)
    if votes_a.shape[0] != votes_b.shape[0]:
        raise ValueError(f"{what}: both vote canvases must have one K, got {votes_a.shape[0]} and {votes_b.shape[0]}")
    oy_a, ox_a = _mosaic_origin(origin_a, what)
    oy_b, ox_b = _mosaic_origin(origin_b, what)
    _relocate_row(link, 16, "link", what)
    if mode not in ORTHO_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(ORTHO_MODES)}, got {mode!r}")
    if not 0 <= int(ordinal_offset) < 0xFFFFFFFF:
        raise ValueError(f"{what}: ordinal_offset must be 0..{0xFFFFFFFF - 1}, got {ordinal_offset}")
    if (ortho_a is None) != (ortho_b is None):
        raise ValueError(f"{what}: ortho_a and ortho_b go together, got {'None' if ortho_a is None else 'planes'} and {'None' if ortho_b is None else 'planes'}")
    planes = []
    for name, ortho, votes in (("ortho_a", ortho_a, votes_a), ("ortho_b", ortho_b, votes_b)):
        if ortho is None:
            continue
        if not isinstance(ortho, (tuple, list)) or len(ortho) != 2:
            raise ValueError(f"{what}: {name} must be (rank, rgba), got a {type(ortho).__name__}")
        if _ortho_planes(ortho[0], ortho[1], what) != tuple(votes.shape[1:]):
            raise ValueError(f"{what}: {name} must be as large as its vote canvas {tuple(votes.shape[1:])}, got {tuple(ortho[1].shape)}")
        planes += list(ortho)
    pairs = [(votes_a, votes_b)] + ([(planes[0], planes[2]), (planes[1], planes[3])] if planes else [])
    if any(_same_memory(x, y) for x, y in pairs):
        raise ValueError(f"{what}: A and B are the same memory (votes at {votes_a.data_ptr():#x} and {votes_b.data_ptr():#x})")
    dev = one_device(votes_a, votes_b, link, *planes, what=what)
    with torch.cuda.device(dev):
        counts = torch.empty((8,), dtype=torch.int64, device=dev)
        rank_a, rgba_a, rank_b, rgba_b = (ptr(p) for p in planes) if planes else (None,) * 4
        check(lib.fs_mosaic_merge(ptr(votes_a), votes_a.shape[1], votes_a.shape[2], ox_a, oy_a, ptr(votes_b), votes_b.shape[1], votes_b.shape[2], ox_b, oy_b,
                                  votes_a.shape[0], ptr(link), rank_a, rgba_a, rank_b, rgba_b, int(ordinal_offset), ORTHO_MODES[mode], ptr(counts), stream_ptr()))
    return counts


def merge_patch(rgba_b, origin_b, link, canvas_a, origin_a, scale, b_box=None):
    """Mosaic B's orthophoto drawn into A's canvas cells under the link, for ops.map_locate against ops.map_coarse(rgba_a) (definition:
    include/floodseg_test.h, merge_patch).  canvas_a = (CH, CW) of A; b_box = (y0, x0, y1, x1) in B canvas pixels, the part of B that is
    drawn (default the whole canvas; FlowPredictor's parts pass the bounding box of what their frames saw).  -> (tl, tv, geom) exactly
    as ops.map_patch returns them; geom[0]: 0 drawn, 1 the link is neither registered nor initial, 2 the link is out of bounds or the
    box lands too far from A's anchor, 3 / 4 the patch has no or too many cells / more cells than A's coarse canvas.  Two launches;
    nothing is read back."""
    lib = _lib.load()
    what = "floodseg.merge_patch"
    ch_b, cw_b = _ortho_planes(None, rgba_b, what)
    ch_a, cw_a = _mosaic_size(canvas_a, "canvas_a", what)
    oy_a, ox_a = _mosaic_origin(origin_a, what)
    oy_b, ox_b = _mosaic_origin(origin_b, what)
    s = _relocate_scale(scale, what)
    if ch_a // s < 1 or cw_a // s < 1:
        raise ValueError(f"{what}: a {ch_a} x {cw_a} canvas has no cell of scale {s}")
    _relocate_row(link, 16, "link", what)
    box = (0, 0, ch_b, cw_b) if b_box is None else tuple(int(v) for v in b_box)
    if len(box) != 4 or not (0 <= box[0] < box[2] <= ch_b and 0 <= box[1] < box[3] <= cw_b):
        raise ValueError(f"{what}: b_box must be a non-empty (y0, x0, y1, x1) inside the {ch_b} x {cw_b} canvas B, got {box}")
    dev = one_device(rgba_b, link, what=what)
    with torch.cuda.device(dev):
        tl, tv = (torch.empty((RELOCATE_PATCH_BYTES,), dtype=torch.uint8, device=dev) for _ in range(2))
        geom = torch.empty((8,), dtype=torch.int64, device=dev)
        check(lib.fs_merge_patch(ptr(rgba_b), ch_b, cw_b, ox_b, oy_b, ptr(link), ch_a, cw_a, ox_a, oy_a, s, *box, ptr(tl), ptr(tv), ptr(geom), stream_ptr()))
    return tl, tv, geom


def link_place(found, link, scale, max_mean=16, ratio_permille=800):
    """map_locate's placement of merge_patch's patch as a CANDIDATE link (definition: include/floodseg_test.h, link_place); `link` is only
    read.  -> (cand int64 [16], out int64 [8]).  Accepted as ops.pose_relocate accepts (the mean, the uniqueness, the bounds): the
    candidate is then the link with both affines moved by (scale u*, scale v*) A canvas pixels and status 1; otherwise the link as
    it was.  out = (code, scale u*, scale v*, sad*, n*, sad2, n2, eligible placements); code 0 placed, 1 the link is neither registered
    nor initial, 2 no placement, 3 / 4 rejected by the mean / by uniqueness, 6 an unusable row, 7 out of the pose bounds.  One launch
    of one wave; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.link_place"
    s = _relocate_scale(scale, what)
    if not 0 <= int(max_mean) <= 255:
        raise ValueError(f"{what}: max_mean must be 0..255, got {max_mean}")
    if not 1 <= int(ratio_permille) <= 1000:
        raise ValueError(f"{what}: ratio_permille must be 1..1000, got {ratio_permille}")
    _relocate_row(found, 16, "found", what)
    _relocate_row(link, 16, "link", what)
    dev = one_device(found, link, what=what)
    with torch.cuda.device(dev):
        cand = torch.empty((16,), dtype=torch.int64, device=dev)
        out = torch.empty((8,), dtype=torch.int64, device=dev)
        check(lib.fs_link_place(ptr(found), ptr(link), s, int(max_mean), int(ratio_permille), ptr(cand), ptr(out), stream_ptr()))
    return cand, out


_PLACE_KEYS = {"scale", "min_overlap_permille", "exclude", "max_mean", "ratio_permille", "b_box"}


def register_mosaics(a, b, link, rounds=2, search=16, intra_bias=0, fit_rounds=4, tol=1.0, min_inliers=12, window=None, place=None):
    """Mosaic B registered against mosaic A: a = (rgba_a, origin_a), b = (rgba_b, origin_b), link int64 [16] with status 0
    or 1, UPDATED IN PLACE.  With place = dict(scale=4 | 8 | 16[, min_overlap_permille, exclude, max_mean, ratio_permille, b_box]) the
    coarse placement runs first: merge_patch, map_coarse(rgba_a), map_locate, link_place, and the candidate replaces the link (a device
    copy).  Then `rounds` times: merge_view, block_match_modes(cur, view, search, 0, intra_bias), merge_gate, global_motion(fit_rounds,
    tol, min_inliers) on the window, link_correct.  Without place the residual between the link and the truth must lie within `search`
    pixels; a link that no round confirms keeps its status 1, and ops.mosaic_merge then changes nothing.  Enqueues only (6 launches a
    round, 7 and a copy for the placement, one stream, nothing read back): capturable as one linear graph.  -> (link, outs int64
    [rounds (+ 1: link_place's row first), 8]).  The defaults are guesses, not validated on real video."""
    what = "floodseg.register_mosaics"
    if place is not None and (not isinstance(place, dict) or "scale" not in place or set(place) - _PLACE_KEYS):
        raise ValueError(f"{what}: place must be a dict with scale and at most {sorted(_PLACE_KEYS)}, got {place!r}")
    if not 1 <= int(rounds) <= 8:
        raise ValueError(f"{what}: rounds must be 1..8, got {rounds}")
    if not 1 <= int(search) <= 32:
        raise ValueError(f"{what}: search must be 1..32 pixels, got {search}")
    for name, m in (("a", a), ("b", b)):
        if not isinstance(m, (tuple, list)) or len(m) != 2:
            raise ValueError(f"{what}: {name} must be (rgba, origin), got a {type(m).__name__}")
    (rgba_a, origin_a), (rgba_b, origin_b) = a, b
    win = _merge_window(window, _ortho_planes(None, rgba_a, what), what)
    outs = []
    if place is not None:
        tl, tv, geom = merge_patch(rgba_b, origin_b, link, rgba_a.shape, origin_a, place["scale"], place.get("b_box"))
        cl, cv = map_coarse(rgba_a, place["scale"])
        found = map_locate(cl, cv, tl, tv, geom, place.get("min_overlap_permille", 500), place.get("exclude", 2))
        cand, out = link_place(found, link, place["scale"], place.get("max_mean", 16), place.get("ratio_permille", 800))
        link.copy_(cand)
        outs.append(out)
    for _ in range(int(rounds)):
        cur, view, valid_a, valid_b = merge_view(rgba_a, origin_a, rgba_b, origin_b, link, win)
        table, stats = block_match_modes(cur, view, search, 0, intra_bias, return_stats=True)
        merge_gate(table, valid_a, valid_b)
        fit = global_motion(table[None], win[2:], win[2:], fit_rounds, tol, min_inliers, pair_stats=stats[None])
        outs.append(link_correct(fit, link, win, origin_a))
    return link, torch.stack(outs)


# ------------------------------------------------------------------------------------------ the change between two registered mosaics
CHANGE_CODES = ("not_comparable", "same", "explained", "changed", "gained", "lost")  # the values of mosaic_change's change plane
CHANGE_CLASSES = len(CHANGE_CODES)  # the change plane as a mask for ops.mask_regions and ops.region_table
CHANGE_MAX_TOLERANCE = 8


def mosaic_change(votes_a, origin_a, votes_b, origin_b, link, min_votes=1, min_conf=0, tolerance=1, watch=(1,)):
    """Where two mosaics of the same ground differ, in A's canvas, under a registered link (definition: include/floodseg_test.h,
    mosaic_change).  votes_a, votes_b: uint16 [K,CH,CW] with one K, only read; origin_* = (oy, ox); link int64 [16] of
    ops.register_mosaics.  A pixel's class is mosaic_resolve's winner where its votes reach min_votes (1..65535) and the winner's share
    min_conf (0..255), else 255; B's pixel under each A pixel comes through mosaic_merge's gather.  tolerance = r (0..8 pixels): a pixel
    whose two classes differ is "explained" where B holds A's class and A holds B's class within r pixels.  watch: the class ids that
    count as water.  -> (change, cls_a, cls_b, transitions, counts): change uint8 [CH_a,CW_a] with 0 not comparable, 1 same, 2
    explained, 3 changed between two watched or two other classes, 4 gained (A not watched, B watched), 5 lost; cls_a, cls_b uint8
    [CH_a,CW_a]; transitions int64 [2,K,K], [0][ca][cb] the comparable pixels and [1][ca][cb] those with code >= 3; counts int64 [8] =
    (link status, A pixels whose B pixel exists, comparable, same, explained, changed, gained, lost).  A link whose status is not 0
    compares nothing (all 0); that is decided on the device.  Three launches; nothing is read back.
    The defaults are guesses, not validated on real video."""
    lib = _lib.load()
    what = "floodseg.mosaic_change"
    votes_a, votes_b = _mosaic_votes(votes_a, what), _mosaic_votes(votes_b, what)
    if votes_a.shape[0] != votes_b.shape[0]:
        raise ValueError(f"{what}: both vote canvases must have one K, got {votes_a.shape[0]} and {votes_b.shape[0]}")
    oy_a, ox_a = _mosaic_origin(origin_a, what)
    oy_b, ox_b = _mosaic_origin(origin_b, what)
    _relocate_row(link, 16, "link", what)
    if not 1 <= int(min_votes) <= 65535:
        raise ValueError(f"{what}: min_votes must be 1..65535, got {min_votes}")
    if not 0 <= int(min_conf) <= 255:
        raise ValueError(f"{what}: min_conf must be 0..255, got {min_conf}")
    if not 0 <= int(tolerance) <= CHANGE_MAX_TOLERANCE:
        raise ValueError(f"{what}: tolerance must be 0..{CHANGE_MAX_TOLERANCE} pixels, got {tolerance}")
    k = votes_a.shape[0]
    watch_set = class_set(watch, "watch", what, allow_empty=True)
    if watch_set >> k:
        raise ValueError(f"{what}: watch must be class ids below K = {k}, got {list(watch)}")
    if _same_memory(votes_a, votes_b):
        raise ValueError(f"{what}: A and B are the same memory (votes at {votes_a.data_ptr():#x})")
    dev = one_device(votes_a, votes_b, link, what=what)
    with torch.cuda.device(dev):
        change, cls_a, cls_b = (torch.empty(tuple(votes_a.shape[1:]), dtype=torch.uint8, device=dev) for _ in range(3))
        transitions = torch.empty((2, k, k), dtype=torch.int64, device=dev)
        counts = torch.empty((8,), dtype=torch.int64, device=dev)
        check(lib.fs_mosaic_change(ptr(votes_a), votes_a.shape[1], votes_a.shape[2], ox_a, oy_a, ptr(votes_b), votes_b.shape[1], votes_b.shape[2], ox_b, oy_b, k,
                                   ptr(link), int(min_votes), int(min_conf), int(tolerance), watch_set, ptr(change), ptr(cls_a), ptr(cls_b), ptr(transitions),
                                   ptr(counts), stream_ptr()))
    return change, cls_a, cls_b, transitions, counts


# ------------------------------------------------------------------------------------------ georeferencing the mosaic
GROUND_MAX_PLANES = 8  # FS_GROUND_MAX_PLANES
GROUND_NO_POINT = -2 ** 63  # FS_GROUND_NO_POINT
GROUND_MAX_GSD_MM = 1 << 20


def ground_model_rows(model, what="floodseg.ground_area"):
    """A ground model -> (forward, inverse), two lists of nine finite floats: an object with .forward and .inverse (flow.georef.GroundModel)
    or a pair of sequences.  forward: anchor pixel coordinates to millimetres about the model's ground origin; inverse: back."""
    pair = (model.forward, model.inverse) if hasattr(model, "forward") and hasattr(model, "inverse") else model
    try:
        rows = [[float(v) for v in (m.reshape(-1).tolist() if hasattr(m, "reshape") else list(m))] for m in pair]
    except (TypeError, ValueError):
        rows = None
    if rows is None or len(rows) != 2 or any(len(r) != 9 for r in rows):
        raise ValueError(f"{what}: model must hold a forward and an inverse model of nine float64 each, got {model!r}")
    for name, r in zip(("forward", "inverse"), rows):
        if any(v != v or v in (float("inf"), float("-inf")) for v in r):
            raise ValueError(f"{what}: the {name} model holds a value that is not finite: {r}")
    return rows


def _ground_plane(t, name, what, shape=None):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{what}: {name} must be a uint8 [CH,CW] tensor{'' if shape is None else ' of the canvas ' + str(list(shape))}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    _mosaic_size(t.shape, name, what)
    return t.contiguous()


def ground_area(cls, model, origin, classes, index=None, max_regions=0):
    """Hectares instead of pixels (definition: include/floodseg_test.h, ground_area): cls uint8 [CH,CW] (mosaic_resolve's
    class plane, or mosaic_change's change plane with classes=6; 255 = unseen) -> (class_area2 int64 [classes], region_area2 int64
    [max_regions], counts int64 [4]).  Every canvas pixel's four lattice corners go through the model's corner rule to int64 millimetres
    and the pixel's area2 is their shoelace sum, twice its area in mm^2, oriented positive; adjacent pixels share corners, so the sums
    are exact.  index: region_table's int32 index plane of this canvas ([CH,CW] or [1,CH,CW]) with max_regions >= 1.  counts = (pixels
    summed, folded pixels, pixels with classes <= id < 255, 0).  origin = (oy, ox).  The model's bounds are the library's to refuse
    (RuntimeError naming the model).  Two launches; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.ground_area"
    cls = _ground_plane(cls, "cls", what)
    ch, cw = cls.shape
    forward, _ = ground_model_rows(model, what)
    oy, ox = _mosaic_origin(origin, what)
    k, cap = int(classes), int(max_regions)
    if not 1 <= k <= 255:
        raise ValueError(f"{what}: classes must be 1..255, got {classes}")
    if not 0 <= cap <= 65536:
        raise ValueError(f"{what}: max_regions must be 0..65536, got {max_regions}")
    if (index is None) != (cap == 0):
        raise ValueError(f"{what}: index goes with max_regions >= 1 and only with it, got max_regions={max_regions} and index "
                         f"{'None' if index is None else 'given'}")
    if index is not None:
        if index.dtype != torch.int32 or index.numel() != ch * cw or tuple(index.shape[-2:]) != (ch, cw):
            raise ValueError(f"{what}: index must be int32 [{ch},{cw}] (region_table's of this canvas), got {index.dtype} {tuple(index.shape)}")
        index = index.contiguous()
    dev = one_device(cls, index, what=what)
    host = (ctypes.c_double * 9)(*forward)  # read by the library during the call
    with torch.cuda.device(dev):
        class_area2 = torch.empty((k,), dtype=torch.int64, device=dev)
        region_area2 = torch.empty((cap,), dtype=torch.int64, device=dev)
        counts = torch.empty((4,), dtype=torch.int64, device=dev)
        check(lib.fs_ground_area(ptr(cls), ch, cw, ox, oy, ctypes.cast(host, ctypes.c_void_p), k, ptr(index), cap, ptr(class_area2),
                                 ptr(region_area2 if cap else None), ptr(counts), stream_ptr()))
    return class_area2, region_area2, counts


def ground_rectify(model, origin, raster_size, gsd_mm, top_left_mm, planes=(), rgba=None, fill=255, rgb_fill=(0, 0, 0)):
    """North-up rasters of canvas planes (definition: include/floodseg_test.h, ground_rectify) -> (rasters, rgb): a list of
    uint8 [GH,GW] tensors, one per uint8 [CH,CW] plane of `planes` (class, confidence, change, any id plane; nearest sampling, `fill`
    outside the canvas), and uint8 [GH,GW,3] from the orthophoto's int32 rgba plane (Q8 bilinear over seen taps, the nearest tap beside
    unseen ground, rgb_fill where that is unseen too), None without rgba.  raster_size = (GH, GW); gsd_mm: the raster pixel's side in whole
    millimetres, 1..2^20; top_left_mm = (E, N) of the raster's top-left CORNER in whole millimetres about the model's ground origin.
    Raster pixel (u, v) samples the ground point (E + (u + 0.5) gsd, N - (v + 0.5) gsd) through the model's inverse.  origin = (oy, ox).
    One launch for all planes; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.ground_rectify"
    _, inverse = ground_model_rows(model, what)
    oy, ox = _mosaic_origin(origin, what)
    gh, gw = _mosaic_size(raster_size, "raster_size", what)
    if int(gsd_mm) != gsd_mm or not 1 <= int(gsd_mm) <= GROUND_MAX_GSD_MM:
        raise ValueError(f"{what}: gsd_mm must be a whole number 1..{GROUND_MAX_GSD_MM}, got {gsd_mm}")
    e0, ntop = top_left_mm
    if int(e0) != e0 or int(ntop) != ntop or abs(int(e0)) >= 2 ** 40 or abs(int(ntop)) >= 2 ** 40:
        raise ValueError(f"{what}: top_left_mm must be (E, N) in whole millimetres within 2^40 of the ground origin, got {tuple(top_left_mm)}")
    planes = list(planes)
    if len(planes) > GROUND_MAX_PLANES or (not planes and rgba is None):
        raise ValueError(f"{what}: 0..{GROUND_MAX_PLANES} planes and at least one plane or rgba, got {len(planes)} planes and rgba "
                         f"{'None' if rgba is None else 'given'}")
    shape = tuple(rgba.shape) if rgba is not None else tuple(planes[0].shape) if torch.is_tensor(planes[0]) else None
    if rgba is not None:
        _ortho_planes(None, rgba, what)
    planes = [_ground_plane(p, f"plane {i}", what, shape) for i, p in enumerate(planes)]
    ch, cw = shape
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"{what}: fill must be 0..255, got {fill}")
    if len(tuple(rgb_fill)) != 3 or any(not 0 <= int(c) <= 255 for c in rgb_fill):
        raise ValueError(f"{what}: rgb_fill must be (r, g, b) with 0..255 each, got {tuple(rgb_fill)}")
    word = int(rgb_fill[0]) | int(rgb_fill[1]) << 8 | int(rgb_fill[2]) << 16
    dev = one_device(*planes, rgba, what=what)
    host = (ctypes.c_double * 9)(*inverse)  # read by the library during the call, as the two pointer arrays
    with torch.cuda.device(dev):
        outs = [torch.empty((gh, gw), dtype=torch.uint8, device=dev) for _ in planes]
        rgb = torch.empty((gh, gw, 3), dtype=torch.uint8, device=dev) if rgba is not None else None
        ins = (ctypes.c_void_p * max(len(planes), 1))(*[p.data_ptr() for p in planes])
        dst = (ctypes.c_void_p * max(len(planes), 1))(*[o.data_ptr() for o in outs])
        check(lib.fs_ground_rectify(ctypes.cast(host, ctypes.c_void_p), ch, cw, ox, oy, gh, gw, int(gsd_mm), int(e0), int(ntop), len(planes),
                                    ctypes.cast(ins, ctypes.c_void_p), ctypes.cast(dst, ctypes.c_void_p), ptr(rgba), ptr(rgb), int(fill), word, stream_ptr()))
    return outs, rgb


def ground_points(points, model, origin):
    """Canvas lattice points in map coordinates (definition: include/floodseg_test.h, ground_points): points int32 [n,2] =
    (x, y), pixel corners as region_outlines and outline_simplify write their vertices -> int64 [n,2] = (E, N) millimetres about the
    model's ground origin, by ground_area's corner rule: a polygon's shoelace over them equals ground_area's sum over its pixels.  A
    point the model cannot place gets GROUND_NO_POINT twice.  origin = (oy, ox).  One launch; nothing is read back."""
    lib = _lib.load()
    what = "floodseg.ground_points"
    if not torch.is_tensor(points) or points.dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 2 or points.shape[0] > 2 ** 28:
        raise ValueError(f"{what}: points must be int32 [n,2] with n <= 2^28, got {getattr(points, 'dtype', type(points))} {tuple(getattr(points, 'shape', ()))}")
    forward, _ = ground_model_rows(model, what)
    oy, ox = _mosaic_origin(origin, what)
    dev = one_device(points, what=what)
    n = int(points.shape[0])
    host = (ctypes.c_double * 9)(*forward)  # read by the library during the call
    with torch.cuda.device(dev):
        out = torch.empty((n, 2), dtype=torch.int64, device=dev)
        if n:
            check(lib.fs_ground_points(ptr(points.contiguous()), n, ctypes.cast(host, ctypes.c_void_p), ox, oy, ptr(out), stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ region outlines
def region_outlines_workspace_bytes(n, h, w, max_regions, max_contours, max_vertices):
    """FS_REGION_OUTLINES_WORKSPACE_BYTES of include/floodseg_test.h."""
    v = max_vertices
    return n * 8 * (2 * v + 7 * ((v + 1) // 2) + ((h * w + 1023) // 1024 + 1) // 2 + (v + 1023) // 1024 + 2)


def region_outlines(index, max_regions, connectivity=8, max_contours=4096, max_vertices=32768, out=None):
    """region_table's index planes int32 [n,H,W] -> (contours int64 [n,max_contours,6], vertices int32 [n,max_vertices,2], shape int64
    [n,max_regions,3], counts int64 [n,4]) (definition: include/floodseg_test.h, region_outlines): every region's outline as ordered
    polygons on the pixel lattice.  A contours row is (region row, first vertex offset, vertex count, cracks, area2, anchor), in ascending
    anchor order; area2 > 0 is a region's outer contour (clockwise on the screen), area2 < 0 a hole.  vertices holds all lists back to
    back, not closed.  shape rows are (perimeter, contours, vertices) per region; counts rows (contours, rows written, vertices, flags):
    bit 0 = more than max_vertices vertices (the frame gets no contours at all), bit 1 = more than max_contours contours.  connectivity
    must be the one the labels were made with.  out: caller-owned contiguous destinations (rows of larger buffers) in the order of the
    result; they are written whole.  The workspace (44 bytes per possible vertex and frame) is allocated here."""
    lib = _lib.load()
    dev = one_device(index, *(out or ()), what="floodseg.region_outlines")
    if index.dtype != torch.int32 or index.dim() != 3:
        raise RuntimeError(f"floodseg.region_outlines: index must be int32 [n,H,W], got {index.dtype} {tuple(index.shape)}")
    n, h, w = index.shape
    cap, mc, mv = int(max_regions), int(max_contours), int(max_vertices)
    if h < 1 or w < 1 or h * w >= 2 ** 29 or n > 65535:
        raise RuntimeError(f"floodseg.region_outlines: at most 65535 non-empty frames below 2^29 pixels, got {tuple(index.shape)}")
    if connectivity not in (4, 8) or not 1 <= cap <= 65536 or not 1 <= mc <= 2 ** 20 or not 4 <= mv <= 2 ** 22:
        raise RuntimeError("floodseg.region_outlines: connectivity 4 or 8, max_regions 1..65536, max_contours 1..2^20 and max_vertices 4..2^22, "
                           f"got {connectivity}, {max_regions}, {max_contours} and {max_vertices}")
    shapes = ((n, mc, 6), (n, mv, 2), (n, cap, 3), (n, 4))
    dtypes = (torch.int64, torch.int32, torch.int64, torch.int64)
    with torch.cuda.device(dev):
        if out is None:
            out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
        elif len(out) != 4 or any(t.dtype != d or tuple(t.shape) != s or not t.is_contiguous() for t, s, d in zip(out, shapes, dtypes)):
            raise RuntimeError(f"floodseg.region_outlines: out must be contiguous int64 {list(shapes[0])}, int32 {list(shapes[1])}, int64 {list(shapes[2])} "
                               f"and int64 {list(shapes[3])} tensors")
        if n:
            work = torch.empty((region_outlines_workspace_bytes(n, h, w, cap, mc, mv) // 8,), dtype=torch.int64, device=dev)
            check(lib.fs_region_outlines(ptr(index.contiguous()), n, h, w, cap, int(connectivity), mc, mv, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                         ptr(out[3]), ptr(work), stream_ptr()))
    return tuple(out)


# ------------------------------------------------------------------------------------------ outline simplification
def outline_simplify_workspace_bytes(n, max_contours, max_vertices):
    """FS_OUTLINE_SIMPLIFY_WORKSPACE_BYTES of include/floodseg_test.h."""
    return n * 8 * (6 * max_vertices + ((max_vertices + 1023) // 1024 + 1) // 2 + (max_contours + 1) // 2 + 262)


def simplify_tol_q(tolerance):
    """A tolerance in pixels -> tol_q = round(16 tolerance^2), the integer the op compares with (0..2^20, that is 0..256 px)."""
    tol = float(tolerance)
    if not 0.0 <= tol <= 256.0:                                # NaN fails both comparisons
        raise ValueError(f"floodseg.outline_simplify: tolerance must be 0..256 pixels, got {tolerance}")
    return int(round(16.0 * tol * tol))


def outline_simplify(contours, vertices, counts, tolerance, max_rounds=32, out=None):
    """region_outlines' (contours int64 [n,C,6], vertices int32 [n,V,2], counts int64 [n,4]) -> (simple int64 [n,C,4], simple_vertices
    int32 [n,V,2], simple_counts int64 [n,4]) (definition: include/floodseg_test.h, outline_simplify): Ramer-Douglas-Peucker on every
    contour ring, every dropped vertex within `tolerance` pixels of the kept segment that spans it (tol_q = round(16 tolerance^2)).  A
    simple row is (first offset, kept count, area2 of the kept ring, flags: bit 0 unconverged), parallel to the contour rows;
    simple_vertices holds the kept vertices back to back; simple_counts rows are (rows, kept vertices, rounds, flags): bit 0 = some
    contour still had open segments after max_rounds rounds (their vertices are all kept), bit 1 = the frame's outlines had overflowed
    (nothing), bit 2 = the outlines had more contours than rows, bit 3 = inconsistent rows (nothing).  rounds is the largest round that
    split a segment: a frame flagged bit 0 needs a larger max_rounds (1..256; the default 32 is a guess for natural shorelines, not
    validated on real video).  out: caller-owned contiguous destinations in the order of the result; they are written whole.  The
    workspace (48 bytes per possible vertex and frame) is allocated here."""
    tol_q = simplify_tol_q(tolerance)
    if not 1 <= int(max_rounds) <= 256:
        raise ValueError(f"floodseg.outline_simplify: max_rounds must be 1..256, got {max_rounds}")
    lib = _lib.load()
    dev = one_device(contours, vertices, counts, *(out or ()), what="floodseg.outline_simplify")
    if (contours.dtype != torch.int64 or contours.dim() != 3 or contours.shape[2] != 6 or vertices.dtype != torch.int32 or vertices.dim() != 3
            or vertices.shape[2] != 2 or counts.dtype != torch.int64 or tuple(counts.shape) != (contours.shape[0], 4)
            or vertices.shape[0] != contours.shape[0]):
        raise RuntimeError("floodseg.outline_simplify: contours must be int64 [n,C,6], vertices int32 [n,V,2] and counts int64 [n,4], got "
                           f"{contours.dtype} {tuple(contours.shape)}, {vertices.dtype} {tuple(vertices.shape)} and {counts.dtype} {tuple(counts.shape)}")
    n, mc, mv = contours.shape[0], contours.shape[1], vertices.shape[1]
    if n > 65535 or not 1 <= mc <= 2 ** 20 or not 4 <= mv <= 2 ** 22:
        raise RuntimeError(f"floodseg.outline_simplify: at most 65535 frames, 1..2^20 contour rows and 4..2^22 vertices, got {n}, {mc} and {mv}")
    shapes = ((n, mc, 4), (n, mv, 2), (n, 4))
    dtypes = (torch.int64, torch.int32, torch.int64)
    with torch.cuda.device(dev):
        if out is None:
            out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
        elif len(out) != 3 or any(t.dtype != d or tuple(t.shape) != s or not t.is_contiguous() for t, s, d in zip(out, shapes, dtypes)):
            raise RuntimeError(f"floodseg.outline_simplify: out must be contiguous int64 {list(shapes[0])}, int32 {list(shapes[1])} and int64 "
                               f"{list(shapes[2])} tensors")
        if n:
            work = torch.empty((outline_simplify_workspace_bytes(n, mc, mv) // 8,), dtype=torch.int64, device=dev)
            check(lib.fs_outline_simplify(ptr(contours.contiguous()), ptr(vertices.contiguous()), ptr(counts.contiguous()), n, mc, mv, tol_q,
                                          int(max_rounds), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(work), stream_ptr()))
    return tuple(out)


# ------------------------------------------------------------------------------------------ block motion estimation
def block_match(cur, ref, search=16, penalty=0, return_cost=False):
    """Full-search block matching of two uint8 frames [H,W] (luma) or [H,W,3] (RGB as decoded), `ref` the past frame: the motion-vector
    table int32 [H//16 * W//16, 7] that flow.grids.motion_vectors_to_grids takes (definition: include/floodseg_test.h, block_match).
    return_cost: also the winning costs, int32 [H//16 * W//16].
    Every row this op writes is a winner's.  A table may also hold VOID ROWS, (-1, 16, 16, -16, -16, -16, -16): "no vector for this
    block", as an encoder sends none for an intra block.  The grid producer skips them, so their cells keep the identity grid;
    block_match_modes below writes them."""
    lib = _lib.load()
    dev = one_device(cur, ref, what="floodseg.block_match")
    if cur.dtype != torch.uint8 or ref.dtype != torch.uint8:
        raise RuntimeError(f"floodseg.block_match: frames must be uint8, got {cur.dtype} and {ref.dtype}")
    if cur.shape != ref.shape or cur.dim() not in (2, 3) or (cur.dim() == 3 and cur.shape[2] != 3):
        raise RuntimeError(f"floodseg.block_match: frames must be two [H,W] or [H,W,3] tensors of one size, got {tuple(cur.shape)} and {tuple(ref.shape)}")
    h, w = int(cur.shape[0]), int(cur.shape[1])
    with torch.cuda.device(dev):
        cur, ref = cur.contiguous(), ref.contiguous()
        n = (h // 16) * (w // 16)
        mv = torch.empty((n, 7), dtype=torch.int32, device=dev)
        cost = torch.empty((n,), dtype=torch.int32, device=dev) if return_cost else None
        check(lib.fs_block_match(ptr(cur), ptr(ref), h, w, 3 if cur.dim() == 3 else 1, int(search), int(penalty), ptr(mv), ptr(cost), stream_ptr()))
    return (mv, cost) if return_cost else mv


VOID_ROW = (-1, 16, 16, -16, -16, -16, -16)  # a table row that carries no vector (include/floodseg_test.h, block_match_modes)


def block_match_modes(cur, ref, search=16, penalty=0, intra_bias=65535, scene_cut=None, return_cost=False, return_activity=False,
                      return_stats=False):
    """block_match with two decisions made on the device (definition: include/floodseg_test.h, block_match_modes).  A block whose
    winner explains it worse than its own mean does (SAD > activity + intra_bias, 0..65535) is INTRA and gets a void row; a pair with
    more than the fraction `scene_cut` (0..1, mapped to per-mille with round(); None = never) of intra blocks is a CUT and gets void
    rows only.  Returns the table, then, as asked for, cost int32 [n], activity int32 [n] and stats int32 [4] = (blocks, intra
    blocks before the cut rule, cut, 0) -- device tensors all: nothing is read back."""
    lib = _lib.load()
    dev = one_device(cur, ref, what="floodseg.block_match_modes")
    if cur.dtype != torch.uint8 or ref.dtype != torch.uint8:
        raise RuntimeError(f"floodseg.block_match_modes: frames must be uint8, got {cur.dtype} and {ref.dtype}")
    if cur.shape != ref.shape or cur.dim() not in (2, 3) or (cur.dim() == 3 and cur.shape[2] != 3):
        raise RuntimeError(f"floodseg.block_match_modes: frames must be two [H,W] or [H,W,3] tensors of one size, got {tuple(cur.shape)} and {tuple(ref.shape)}")
    if scene_cut is not None and not 0 <= float(scene_cut) <= 1:
        raise RuntimeError(f"floodseg.block_match_modes: scene_cut must be a fraction in [0, 1] or None, got {scene_cut}")
    permille = 1000 if scene_cut is None else int(round(float(scene_cut) * 1000))
    h, w = int(cur.shape[0]), int(cur.shape[1])
    with torch.cuda.device(dev):
        cur, ref = cur.contiguous(), ref.contiguous()
        n = (h // 16) * (w // 16)
        mv = torch.empty((n, 7), dtype=torch.int32, device=dev)
        cost = torch.empty((n,), dtype=torch.int32, device=dev) if return_cost else None
        activity = torch.empty((n,), dtype=torch.int32, device=dev) if return_activity else None
        stats = torch.empty((4,), dtype=torch.int32, device=dev) if return_stats else None
        check(lib.fs_block_match_modes(ptr(cur), ptr(ref), h, w, 3 if cur.dim() == 3 else 1, int(search), int(penalty), int(intra_bias), permille,
                                       ptr(mv), ptr(cost), ptr(activity), ptr(stats), stream_ptr()))
    extra = [t for t in (cost, activity, stats) if t is not None]
    return (mv, *extra) if extra else mv


GUIDE_COUNTS = ("blocks", "void_in", "filled", "outliers", "replaced", "dropped", "kept", "foreign")  # the columns of guide_vectors' counts


def guide_vectors(tables, model, frame_size, fill_void=True, outlier=None, cur=None, ref=None, cost=None, penalty=0, guide_bias=None, out=None):
    """The matcher's tables guided by the fitted camera motion (definition: include/floodseg_test.h, guide_vectors): int32
    tables [n,blocks,7] of frames of frame_size = (FH, FW) and model int64 [n,16], global_motion's rows fitted with mask_size ==
    frame_size -> (tables, counts).  fill_void: a void row whose block the camera's vector can serve takes that vector.  outlier (frame
    pixels, 0..64, None = off; converted to Q20 as global_motion converts tol): a vector further from the camera's than that in x or y is
    replaced by the camera's, or dropped (made void) where the camera's window leaves the frame.  With cur, ref (uint8 [n,FH,FW] or
    [n,FH,FW,3]) and cost (int32 [n,blocks], the matcher's winning costs; penalty = the matcher's) an outlier is replaced only if the
    camera's window explains the block no worse than the winner did, up to guide_bias (0..65535, None = 0): SAD_g + penalty (|dx| + |dy|)
    <= cost + guide_bias; without them it is replaced as it stands.  A pair whose model has status != 0 is copied.  out: an int32
    tensor of tables' shape, which may be tables itself.  counts int64 [n,8] = GUIDE_COUNTS per pair.  Two launches; nothing is read
    back."""
    lib = _lib.load()
    what = "floodseg.guide_vectors"
    fh, fw = _mosaic_size(frame_size, "frame_size", what, 16)
    blocks = (fh // 16) * (fw // 16)
    if tables.dtype != torch.int32 or tables.dim() != 3 or not 1 <= tables.shape[0] <= 64 or tuple(tables.shape[1:]) != (blocks, 7) or not tables.is_contiguous():
        raise ValueError(f"{what}: tables must be contiguous int32 [n,{blocks},7] with n in 1..64 for frames of {fh}x{fw}, got {tables.dtype} {tuple(tables.shape)}")
    n = tables.shape[0]
    model = _mosaic_rows(model, "model", what, n)
    if outlier is not None and not 0 <= float(outlier) <= 64:
        raise ValueError(f"{what}: outlier must be 0..64 frame pixels or None, got {outlier}")
    if not 0 <= int(penalty) <= 255:
        raise ValueError(f"{what}: penalty must be 0..255, got {penalty}")
    if guide_bias is not None and not 0 <= int(guide_bias) <= 65535:
        raise ValueError(f"{what}: guide_bias must be 0..65535 or None, got {guide_bias}")
    given = [name for name, t in (("cur", cur), ("ref", ref), ("cost", cost)) if t is not None]
    if given and len(given) != 3:
        raise ValueError(f"{what}: cur, ref and cost come together or not at all, got only {given}")
    channels = 1
    if given:
        if cur.dtype != torch.uint8 or ref.dtype != torch.uint8 or cur.shape != ref.shape or tuple(cur.shape[:3]) != (n, fh, fw) \
                or cur.dim() not in (3, 4) or (cur.dim() == 4 and cur.shape[3] not in (1, 3)):
            raise ValueError(f"{what}: cur and ref must be uint8 [{n},{fh},{fw}] or [{n},{fh},{fw},3], got {cur.dtype} {tuple(cur.shape)} and "
                             f"{ref.dtype} {tuple(ref.shape)} (channels must be 1 or 3)")
        channels = int(cur.shape[3]) if cur.dim() == 4 else 1
        if cost.dtype != torch.int32 or tuple(cost.shape) != (n, blocks):
            raise ValueError(f"{what}: cost must be int32 [{n},{blocks}], got {cost.dtype} {tuple(cost.shape)}")
    if out is not None and (out.dtype != torch.int32 or out.shape != tables.shape or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous int32 {list(tables.shape)} tensor, got {out.dtype} {tuple(out.shape)}")
    dev = one_device(tables, model, cur, ref, cost, out, what=what)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(tables)
        counts = torch.empty((n, 8), dtype=torch.int64, device=dev)
        if given:
            cur, ref, cost = cur.contiguous(), ref.contiguous(), cost.contiguous()
        check(lib.fs_guide_vectors(ptr(tables), ptr(model), n, fh, fw, int(bool(fill_void)), -1 if outlier is None else int(round(float(outlier) * POSE_ONE)),
                                   ptr(cur), ptr(ref), channels, ptr(cost), int(penalty), 0 if guide_bias is None else int(guide_bias), ptr(out),
                                   ptr(counts), stream_ptr()))
    return out, counts


# ------------------------------------------------------------------------------------------ frame ingest
# base/foundation.py:27-31 (the value_scale = 255 statistics every transform chain of the reference normalises with)
MEAN = [0.485 * 255, 0.456 * 255, 0.406 * 255]
STD = [0.229 * 255, 0.224 * 255, 0.225 * 255]
_FORMATS = {"rgb24": 0, "nv12": 1, "i420": 2}
_MATRICES = {"bt601": 0, "bt709": 1}
_norm_cache = {}  # (device, mean, std) -> device tensor [2,3]: one host-to-device copy per device and statistics, not one per frame


def _norm_constants(dev, mean, std):
    key = (dev, tuple(float(v) for v in mean), tuple(float(v) for v in std))
    t = _norm_cache.get(key)
    if t is None:
        if len(key[1]) != 3 or len(key[2]) != 3 or min(key[2]) <= 0:
            raise RuntimeError(f"floodseg.prepare_frame: mean and std must be three values each, std positive, got {mean} and {std}")
        t = _norm_cache[key] = torch.tensor([key[1], key[2]], dtype=torch.float32).to(dev)
    return t


def prepare_frame(frame, size=None, mean=MEAN, std=STD, fmt="rgb24", chroma=None, matrix="bt601", full_range=False, out=None):
    """One decoded uint8 frame -> the network's input, float32 [1,3,h,w], in one launch (definition: include/floodseg_test.h,
    frame_prepare): half-pixel bilinear resize to `size` (None = native), stored as the uint8 image cv2.resize would give (round half
    to even, clamp), then (x - mean) / std -- transform_predict of the reference (flow/transform.py:26-106).
    fmt "rgb24": frame = [H,W,3].  "nv12": frame = Y [H,W], chroma = the interleaved UV plane [ceil(H/2), ceil(W/2), 2].  "i420":
    chroma = (U, V), [ceil(H/2), ceil(W/2)] each.  matrix "bt601" | "bt709" and full_range pick the integer YUV -> RGB conversion.
    out: a caller-owned contiguous float32 [1,3,h,w] or [3,h,w] destination (one image of a batch tensor)."""
    lib = _lib.load()
    if fmt not in _FORMATS:
        raise RuntimeError(f"floodseg.prepare_frame: fmt must be one of {sorted(_FORMATS)}, got {fmt!r}")
    if matrix not in _MATRICES:
        raise RuntimeError(f"floodseg.prepare_frame: matrix must be one of {sorted(_MATRICES)}, got {matrix!r}")
    planes = [] if chroma is None else list(chroma) if isinstance(chroma, (tuple, list)) else [chroma]
    dev = one_device(frame, out, *planes, what="floodseg.prepare_frame")
    if frame.dtype != torch.uint8 or any(p.dtype != torch.uint8 for p in planes):
        raise RuntimeError(f"floodseg.prepare_frame: frames must be uint8, got {[str(t.dtype) for t in [frame] + planes]}")
    rgb = fmt == "rgb24"
    if frame.dim() != (3 if rgb else 2) or (rgb and frame.shape[2] != 3) or frame.numel() == 0:
        raise RuntimeError(f"floodseg.prepare_frame: a {fmt} frame must be {'[H,W,3]' if rgb else 'the Y plane [H,W]'}, got {tuple(frame.shape)}")
    H, W = int(frame.shape[0]), int(frame.shape[1])
    ch, cw = (H + 1) // 2, (W + 1) // 2
    want = [] if rgb else [(ch, cw, 2)] if fmt == "nv12" else [(ch, cw), (ch, cw)]
    if [tuple(p.shape) for p in planes] != want:
        raise RuntimeError(f"floodseg.prepare_frame: a {H} x {W} {fmt} frame takes chroma {want if want else None}, got {[tuple(p.shape) for p in planes]}")
    h, w = (H, W) if size is None else (int(size[0]), int(size[1]))
    if h < 1 or w < 1:
        raise RuntimeError(f"floodseg.prepare_frame: size must be at least 1 x 1, got {h} x {w}")
    with torch.cuda.device(dev):
        frame = frame.contiguous()
        planes = [p.contiguous() for p in planes]
        if out is None:
            out = torch.empty((1, 3, h, w), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) not in ((1, 3, h, w), (3, h, w)) or not out.is_contiguous():
            raise RuntimeError(f"floodseg.prepare_frame: out must be contiguous float32 [1,3,{h},{w}] or [3,{h},{w}], got {out.dtype} {tuple(out.shape)}")
        norm = _norm_constants(dev, mean, std)
        check(lib.fs_frame_prepare(ptr(frame), ptr(planes[0]) if planes else None, ptr(planes[1]) if len(planes) > 1 else None, _FORMATS[fmt],
                                   _MATRICES[matrix], int(bool(full_range)), H, W, ptr(norm[0]), ptr(norm[1]), ptr(out), h, w, stream_ptr()))
    return out.view(1, 3, h, w)


# ------------------------------------------------------------------------------------------ frame egress
_palette_cache = {}  # (device, palette bytes, K) -> device tensor [K,4]: one host-to-device copy per device and palette, not one per frame


def raw_frame_bytes(height, width, pix_fmt):
    """Bytes of one frame of a headerless raw video (ffmpeg -f rawvideo): chroma planes of the 4:2:0 formats round up."""
    if pix_fmt == "rgb24":
        return height * width * 3
    if pix_fmt == "gray":  # one 8-bit plane (ffmpeg -pix_fmt gray): the confidence planes
        return height * width
    return height * width + 2 * ((height + 1) // 2) * ((width + 1) // 2)


def frame_planes(buf, height, width, pix_fmt):
    """(frame, chroma) views of one raw frame's bytes `buf` (uint8 [raw_frame_bytes]) as prepare_frame takes and compose_frame returns
    them: rgb24 -> ([H,W,3], None); gray -> ([H,W], None); nv12 -> (Y [H,W], UV [ceil(H/2),ceil(W/2),2]); i420 -> (Y, (U, V))."""
    h, w = height, width
    if pix_fmt == "rgb24":
        return buf.view(h, w, 3), None
    if pix_fmt == "gray":
        return buf.view(h, w), None
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = buf[:h * w].view(h, w)
    if pix_fmt == "nv12":
        return y, buf[h * w:].view(ch, cw, 2)
    return y, (buf[h * w:h * w + ch * cw].view(ch, cw), buf[h * w + ch * cw:].view(ch, cw))


def _palette_rgba(dev, palette, alpha, opaque_default):
    """uint8 [K,4] (R, G, B, A) on `dev` from a [K,3] or [K,4] palette (numpy array, sequence or tensor), cached per device and contents."""
    import numpy as np

    pal = palette.detach().cpu().numpy() if isinstance(palette, torch.Tensor) else np.asarray(palette)
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] not in (3, 4) or not 1 <= pal.shape[0] <= 256:
        raise RuntimeError(f"floodseg.compose_frame: palette must be uint8 [K,3] or [K,4] with 1 <= K <= 256, got {pal.dtype} {pal.shape}")
    if pal.shape[1] == 4:
        if alpha is not None:
            raise RuntimeError("floodseg.compose_frame: alpha= goes with a [K,3] palette; a [K,4] palette carries its own opacities")
    else:
        if alpha is None and not opaque_default:
            raise RuntimeError("floodseg.compose_frame: a [K,3] palette over a background needs alpha= (0..255)")
        a = 255 if alpha is None else int(alpha)
        if not 0 <= a <= 255:
            raise RuntimeError(f"floodseg.compose_frame: alpha must be 0..255, got {alpha}")
        pal = np.concatenate([pal, np.full((pal.shape[0], 1), a, dtype=np.uint8)], axis=1)
    key = (dev, pal.tobytes(), pal.shape[0])
    t = _palette_cache.get(key)
    if t is None:
        t = _palette_cache[key] = torch.from_numpy(np.ascontiguousarray(pal)).to(dev)
    return t


def compose_frame(mask, palette, background=None, chroma=None, fmt="rgb24", matrix="bt601", full_range=False, out_fmt="nv12", out_matrix=None,
                  out_full_range=None, out=None, alpha=None):
    """One uint8 mask [h,w] -> one result video frame in one launch (definition: include/floodseg_test.h, frame_compose): the class
    colours of `palette`, optionally blended over the decoded frame the network saw, as RGB24, NV12 or I420 bytes for a video encoder.
    palette: uint8 [K,3] or [K,4] (R, G, B, A), numpy or tensor, cached on the device by contents; a [K,3] palette takes `alpha`
    (0..255) for every class, or is opaque when there is no background.  Mask values >= K are class 0 (colorize's rule).
    background, chroma, fmt, matrix, full_range: one decoded frame exactly as prepare_frame takes it (any size: it is resized to
    [h,w] as prepare_frame would, and blended o = (A * colour + (255 - A) * b + 127) // 255); None: the colours alone.
    out_fmt "rgb24" | "nv12" | "i420"; out_matrix / out_full_range pick the integer RGB -> YUV conversion (default: the input's).
    Returns rgb [h,w,3], or (y, chroma) in the shapes prepare_frame takes.  out: ONE caller-owned contiguous uint8 buffer of
    raw_frame_bytes(h, w, out_fmt) bytes that the returned planes are views of (a slice at any byte offset is fine), so that one
    device-to-host copy moves a frame."""
    lib = _lib.load()
    if fmt not in _FORMATS or out_fmt not in _FORMATS:
        raise RuntimeError(f"floodseg.compose_frame: fmt and out_fmt must be one of {sorted(_FORMATS)}, got {fmt!r} and {out_fmt!r}")
    out_matrix = matrix if out_matrix is None else out_matrix
    out_full_range = full_range if out_full_range is None else out_full_range
    if matrix not in _MATRICES or out_matrix not in _MATRICES:
        raise RuntimeError(f"floodseg.compose_frame: matrix and out_matrix must be one of {sorted(_MATRICES)}, got {matrix!r} and {out_matrix!r}")
    planes = [] if chroma is None else list(chroma) if isinstance(chroma, (tuple, list)) else [chroma]
    dev = one_device(mask, background, out, *planes, what="floodseg.compose_frame")
    if mask.dtype != torch.uint8 or mask.dim() != 2 or mask.numel() == 0:
        raise RuntimeError(f"floodseg.compose_frame: mask must be a non-empty uint8 [h,w] tensor, got {mask.dtype} {tuple(mask.shape)}")
    h, w = int(mask.shape[0]), int(mask.shape[1])
    H = W = 0
    if background is None:
        if planes:
            raise RuntimeError("floodseg.compose_frame: chroma planes without a background frame")
    else:
        if background.dtype != torch.uint8 or any(p.dtype != torch.uint8 for p in planes):
            raise RuntimeError(f"floodseg.compose_frame: frames must be uint8, got {[str(t.dtype) for t in [background] + planes]}")
        rgb = fmt == "rgb24"
        if background.dim() != (3 if rgb else 2) or (rgb and background.shape[2] != 3) or background.numel() == 0:
            raise RuntimeError(f"floodseg.compose_frame: a {fmt} background must be {'[H,W,3]' if rgb else 'the Y plane [H,W]'}, got {tuple(background.shape)}")
        H, W = int(background.shape[0]), int(background.shape[1])
        ch, cw = (H + 1) // 2, (W + 1) // 2
        want = [] if rgb else [(ch, cw, 2)] if fmt == "nv12" else [(ch, cw), (ch, cw)]
        if [tuple(p.shape) for p in planes] != want:
            raise RuntimeError(f"floodseg.compose_frame: a {H} x {W} {fmt} background takes chroma {want if want else None}, got {[tuple(p.shape) for p in planes]}")
    nbytes = raw_frame_bytes(h, w, out_fmt)
    with torch.cuda.device(dev):
        pal = _palette_rgba(dev, palette, alpha, background is None)
        mask = mask.contiguous()
        planes = [p.contiguous() for p in planes]
        background = background.contiguous() if background is not None else None
        if out is None:
            out = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() != nbytes or not out.is_contiguous():
            raise RuntimeError(f"floodseg.compose_frame: out must be a contiguous uint8 [{nbytes}] buffer (one {h} x {w} {out_fmt} frame), got {out.dtype} {tuple(out.shape)}")
        frame, ochroma = frame_planes(out, h, w, out_fmt)
        oplanes = [] if ochroma is None else list(ochroma) if isinstance(ochroma, tuple) else [ochroma]
        check(lib.fs_frame_compose(ptr(mask), h, w, ptr(pal), pal.shape[0], ptr(background), ptr(planes[0]) if planes else None,
                                   ptr(planes[1]) if len(planes) > 1 else None, _FORMATS[fmt], _MATRICES[matrix], int(bool(full_range)), H, W,
                                   ptr(frame), ptr(oplanes[0]) if oplanes else None, ptr(oplanes[1]) if len(oplanes) > 1 else None,
                                   _FORMATS[out_fmt], _MATRICES[out_matrix], int(bool(out_full_range)), stream_ptr()))
    return frame if out_fmt == "rgb24" else (frame, ochroma)



# ------------------------------------------------------------------------------------------ region overlay
# A default fill palette for track ids: 16 hues spaced round the colour wheel, alternating two lightness levels so that neighbouring
# entries differ in both.  The choice is a guess -- nobody has tested it on viewers or on colour-blind ones; pass fill_palette= for another.
TRACK_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
                 (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195))
_plain_palette_cache = {}  # (device, bytes, rows, columns) -> device tensor: the fill and outline palettes, cached as the class palette is


def compose_regions_workspace_bytes(h, w):
    """Bytes of compose_regions' marks plane (FS_FRAME_COMPOSE_REGIONS_WORKSPACE_BYTES in include/floodseg_test.h): h * w rounded up to 4."""
    return (int(h) * int(w) + 3) // 4 * 4


def _plain_palette(dev, palette, columns, name, max_rows):
    import numpy as np

    pal = palette.detach().cpu().numpy() if isinstance(palette, torch.Tensor) else np.asarray(palette)
    if pal.ndim == 2 and pal.dtype != np.uint8 and pal.size and pal.min() >= 0 and pal.max() <= 255 and np.issubdtype(pal.dtype, np.integer):
        pal = pal.astype(np.uint8)  # a tuple of tuples, as TRACK_PALETTE
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != columns or not 1 <= pal.shape[0] <= max_rows:
        raise RuntimeError(f"floodseg.compose_regions: {name} must be uint8 [1..{max_rows},{columns}], got {pal.dtype} {pal.shape}")
    key = (dev, pal.tobytes(), pal.shape[0], columns)
    t = _plain_palette_cache.get(key)
    if t is None:
        t = _plain_palette_cache[key] = torch.from_numpy(np.ascontiguousarray(pal)).to(dev)
    return t


def _packed_colour(value, n, name):
    v = tuple(int(c) for c in value)
    if len(v) != n or any(not 0 <= c <= 255 for c in v):
        raise RuntimeError(f"floodseg.compose_regions: {name} must be {n} values 0..255, got {value!r}")
    return sum(c << (8 * i) for i, c in enumerate(v))


def compose_regions(mask, palette, index, table=None, counts=None, tracks=None, fill_palette=None, outline=None, outline_width=1, label_scale=0,
                    label_min_area=256, halo=(0, 0, 0, 160), ink=(255, 255, 255), background=None, chroma=None, fmt="rgb24", matrix="bt601",
                    full_range=False, out_fmt="nv12", out_matrix=None, out_full_range=None, out=None, alpha=None):
    """compose_frame's picture with the regions drawn into it (definition: include/floodseg_test.h, frame_compose_regions), on the device,
    nothing read back.  mask, palette, background .. alpha, the returns and the out= contract are compose_frame's.
    index int32 [h,w], table int64 [R,10], counts int64 [2]: one frame of region_table's result; tracks int64 [R,4]: that frame of
    region_tracks' result, or None -- a region's id is then its row.
    fill_palette uint8 [P,3] (e.g. TRACK_PALETTE), P <= 256: every region with an id >= 0 takes colour id % P, with its class's opacity.
    outline uint8 [K,4] (R, G, B, A per class; A = 0: none for that class) with outline_width 0..4: a line that wide along the inside
    of every region's boundary.  label_scale 1..4: the id (mod 10^7) in a 5 x 7 font of that scale, on a `halo` (R, G, B, A) backdrop
    in `ink` (R, G, B), centred on the region's centroid and clamped to the frame, for regions of at least label_min_area pixels;
    needs table and counts.  The marks workspace is allocated here.  With no layer on this is compose_frame, byte for byte."""
    what = "floodseg.compose_regions"
    lib = _lib.load()
    if fmt not in _FORMATS or out_fmt not in _FORMATS:
        raise RuntimeError(f"{what}: fmt and out_fmt must be one of {sorted(_FORMATS)}, got {fmt!r} and {out_fmt!r}")
    out_matrix = matrix if out_matrix is None else out_matrix
    out_full_range = full_range if out_full_range is None else out_full_range
    if matrix not in _MATRICES or out_matrix not in _MATRICES:
        raise RuntimeError(f"{what}: matrix and out_matrix must be one of {sorted(_MATRICES)}, got {matrix!r} and {out_matrix!r}")
    planes = [] if chroma is None else list(chroma) if isinstance(chroma, (tuple, list)) else [chroma]
    dev = one_device(mask, index, table, counts, tracks, background, out, *planes, what=what)
    if mask.dtype != torch.uint8 or mask.dim() != 2 or mask.numel() == 0:
        raise RuntimeError(f"{what}: mask must be a non-empty uint8 [h,w] tensor, got {mask.dtype} {tuple(mask.shape)}")
    h, w = int(mask.shape[0]), int(mask.shape[1])
    if index.dtype != torch.int32 or tuple(index.shape) != (h, w):
        raise RuntimeError(f"{what}: index must be int32 of the mask's shape {(h, w)}, got {index.dtype} {tuple(index.shape)}")
    T, scale, min_area = int(outline_width), int(label_scale), int(label_min_area)
    if not 0 <= T <= 4 or not 0 <= scale <= 4 or not 1 <= min_area < 2 ** 63:
        raise RuntimeError(f"{what}: outline_width and label_scale must be 0..4 and label_min_area at least 1, got {outline_width}, {label_scale} and "
                           f"{label_min_area}")
    cap = None
    for t, cols, name in ((table, 10, "table"), (tracks, 4, "tracks")):
        if t is None:
            continue
        if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != cols or not 1 <= t.shape[0] <= 65536 or (cap is not None and t.shape[0] != cap):
            raise RuntimeError(f"{what}: {name} must be int64 [max_regions,{cols}] with 1 <= max_regions <= 65536"
                               f"{'' if cap is None else f' = {cap}'}, got {t.dtype} {tuple(t.shape)}")
        cap = int(t.shape[0])
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (2,)):
        raise RuntimeError(f"{what}: counts must be int64 [2] (one frame of region_table's counts), got {counts.dtype} {tuple(counts.shape)}")
    if scale and (table is None or counts is None):
        raise RuntimeError(f"{what}: labels (label_scale={scale}) need table= and counts=")
    if cap is None:
        cap = 65536  # neither table nor tracks: every non-negative index below the largest cap is a row
    halo_word, ink_word = _packed_colour(halo, 4, "halo"), _packed_colour(ink, 3, "ink")
    H = W = 0
    if background is None:
        if planes:
            raise RuntimeError(f"{what}: chroma planes without a background frame")
    else:
        if background.dtype != torch.uint8 or any(p.dtype != torch.uint8 for p in planes):
            raise RuntimeError(f"{what}: frames must be uint8, got {[str(t.dtype) for t in [background] + planes]}")
        rgb = fmt == "rgb24"
        if background.dim() != (3 if rgb else 2) or (rgb and background.shape[2] != 3) or background.numel() == 0:
            raise RuntimeError(f"{what}: a {fmt} background must be {'[H,W,3]' if rgb else 'the Y plane [H,W]'}, got {tuple(background.shape)}")
        H, W = int(background.shape[0]), int(background.shape[1])
        ch, cw = (H + 1) // 2, (W + 1) // 2
        want = [] if rgb else [(ch, cw, 2)] if fmt == "nv12" else [(ch, cw), (ch, cw)]
        if [tuple(p.shape) for p in planes] != want:
            raise RuntimeError(f"{what}: a {H} x {W} {fmt} background takes chroma {want if want else None}, got {[tuple(p.shape) for p in planes]}")
    nbytes = raw_frame_bytes(h, w, out_fmt)
    with torch.cuda.device(dev):
        pal = _palette_rgba(dev, palette, alpha, background is None)
        fill = _plain_palette(dev, fill_palette, 3, "fill_palette", 256) if fill_palette is not None else None
        line = _plain_palette(dev, outline, 4, "outline", 256) if outline is not None else None
        if line is not None and line.shape[0] != pal.shape[0]:
            raise RuntimeError(f"{what}: outline must have one (R, G, B, A) row per class of the palette ({pal.shape[0]}), got {tuple(line.shape)}")
        mask = mask.contiguous()
        planes = [p.contiguous() for p in planes]
        background = background.contiguous() if background is not None else None
        if out is None:
            out = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() != nbytes or not out.is_contiguous():
            raise RuntimeError(f"{what}: out must be a contiguous uint8 [{nbytes}] buffer (one {h} x {w} {out_fmt} frame), got {out.dtype} {tuple(out.shape)}")
        frame, ochroma = frame_planes(out, h, w, out_fmt)
        oplanes = [] if ochroma is None else list(ochroma) if isinstance(ochroma, tuple) else [ochroma]
        work = torch.empty((compose_regions_workspace_bytes(h, w),), dtype=torch.uint8, device=dev) if scale else None
        check(lib.fs_frame_compose_regions(
            ptr(mask), h, w, ptr(pal), pal.shape[0], ptr(background), ptr(planes[0]) if planes else None, ptr(planes[1]) if len(planes) > 1 else None,
            _FORMATS[fmt], _MATRICES[matrix], int(bool(full_range)), H, W, ptr(frame), ptr(oplanes[0]) if oplanes else None,
            ptr(oplanes[1]) if len(oplanes) > 1 else None, _FORMATS[out_fmt], _MATRICES[out_matrix], int(bool(out_full_range)),
            ptr(index.contiguous()), ptr(table.contiguous()) if table is not None else None, ptr(counts.contiguous()) if counts is not None else None,
            ptr(tracks.contiguous()) if tracks is not None else None, cap, ptr(fill), fill.shape[0] if fill is not None else 0, ptr(line), T, scale, min_area,
            halo_word, ink_word, ptr(work), stream_ptr()))
    return frame if out_fmt == "rgb24" else (frame, ochroma)

# ------------------------------------------------------------------------------------------ single-frame multi-scale test
def ms_prepare(raw, new_hw, padded_hw, mean, std, flip=True):
    """One scale's network input from the raw 0-255 frame [3,H,W] (base/foundation.py:193-200, 267-273, 300-306): resized to
    `new_hw` (half-pixel bilinear), mean-padded to `padded_hw`, normalised -> fp32 [2 if flip else 1, 3, PH, PW]; [1] is the
    horizontal mirror of [0] (fs_ms_prepare)."""
    lib = _lib.load()
    if raw.dim() != 3 or raw.shape[0] != 3:
        raise RuntimeError(f"floodseg.ms_prepare: expected a [3,H,W] frame, got {tuple(raw.shape)}")
    with torch.cuda.device(one_device(raw, what="floodseg.ms_prepare")):
        x = _f32c(raw)
        ph, pw = int(padded_hw[0]), int(padded_hw[1])
        out = torch.empty((2 if flip else 1, 3, ph, pw), dtype=torch.float32, device=x.device)
        m = (ctypes.c_float * 3)(*[float(v) for v in mean])
        s = (ctypes.c_float * 3)(*[float(v) for v in std])
        check(lib.fs_ms_prepare(ptr(x), x.shape[1], x.shape[2], int(new_hw[0]), int(new_hw[1]), ph, pw, m, s, ptr(out), int(bool(flip)),
                                stream_ptr()))
    return out


def ms_fuse(lo_plain, lo_flip, crop_yx, crop_hw, padded_hw, new_hw, pred=None, frame_hw=None, scale_index=0, nscales=1, want_mask=False):
    """Crop / flip fusion of one scale and its accumulation over the scales (base/foundation.py:279-295, 322-325, 201-203;
    fs_ms_fuse).  lo_plain / lo_flip: [ncrops,K,h,w] logits of the crops `crop_yx` (offsets in the padded frame) of the prepared
    frame / of its mirror (None: flip=False).  Returns (scaled [new_h,new_w,K] float64, pred, mask): with `frame_hw` the scale is
    resized to the frame and added to `pred` [H,W,K] float64 (allocated when None; written, not added, at scale_index 0); the
    last scale divides by `nscales` and, if want_mask, gives the uint8 argmax."""
    lib = _lib.load()
    dev = one_device(lo_plain, lo_flip, pred, what="floodseg.ms_fuse")
    if lo_plain.dim() != 4 or (lo_flip is not None and lo_flip.shape != lo_plain.shape):
        raise RuntimeError("floodseg.ms_fuse: logits must be [ncrops,K,h,w], the flipped ones of the same shape")
    nc, k, h, w = lo_plain.shape
    if nc != len(crop_yx):
        raise RuntimeError(f"floodseg.ms_fuse: {nc} logit maps for {len(crop_yx)} crops")
    with torch.cuda.device(dev):
        a = _f32c(lo_plain)
        b = _f32c(lo_flip) if lo_flip is not None else None
        nh, nw = int(new_hw[0]), int(new_hw[1])
        scaled = torch.empty((max(nh, 0), max(nw, 0), k), dtype=torch.float64, device=dev)
        mask = None
        fh = fw = 0
        if frame_hw is not None:
            fh, fw = int(frame_hw[0]), int(frame_hw[1])
            if pred is None:
                pred = torch.empty((fh, fw, k), dtype=torch.float64, device=dev)
            if pred.dtype != torch.float64 or tuple(pred.shape) != (fh, fw, k) or not pred.is_contiguous():
                raise RuntimeError(f"floodseg.ms_fuse: pred must be a contiguous float64 [{fh},{fw},{k}] tensor")
            if want_mask and scale_index == nscales - 1:
                mask = torch.empty((fh, fw), dtype=torch.uint8, device=dev)
        elif pred is not None or want_mask:
            raise RuntimeError("floodseg.ms_fuse: pred / mask need frame_hw")
        ys = (ctypes.c_int * nc)(*[int(y) for y, _ in crop_yx])
        xs = (ctypes.c_int * nc)(*[int(x) for _, x in crop_yx])
        check(lib.fs_ms_fuse(ptr(a), ptr(b), nc, ys, xs, k, h, w, int(crop_hw[0]), int(crop_hw[1]), int(padded_hw[0]), int(padded_hw[1]), nh, nw,
                             ptr(scaled), ptr(pred) if frame_hw is not None else None, fh, fw, int(scale_index), int(nscales), ptr(mask),
                             stream_ptr()))
    return scaled, pred, mask


# ------------------------------------------------------------------------------------------ building blocks
# (test / bring-up helpers over the op-level hooks of include/floodseg_test.h; nothing on the product path calls them)
def conv2d_nhwc(x, weight, scale=None, shift=None, residual=None, stride=1, pad=0, dil=1, relu=False, tile=0, out=None, split=False):
    """Conv2d on the matrix cores; x logical NCHW (stored NHWC), weight OIHW. Test/bring-up helper.  split=True: the split-operand
    kernel (three bf16 terms per fp32 value, bf16 MFMA, fp32 accumulate: fs_conv2d_nhwc_split) instead of the fp32-MFMA one."""
    lib = _lib.load()
    with torch.cuda.device(one_device(x, weight, scale, shift, residual, out, what="floodseg.conv2d_nhwc")):
        x = as_nhwc(x)
        b, cin, h, w = x.shape
        o, i, kh, kw = weight.shape
        wp = torch.empty((o, kh, kw, i), dtype=torch.float32, device=x.device)
        check(lib.fs_pack_conv_weight(ptr(_f32c(weight)), ptr(wp), o, i, kh, kw, stream_ptr()))
        ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
        wo = (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1
        if out is None:
            out = empty_nhwc(b, o, ho, wo, x.device)
        res = as_nhwc(residual) if residual is not None else None
        if split:
            planes = torch.empty(3 * wp.numel(), dtype=torch.bfloat16, device=x.device)
            check(lib.fs_split_bf16x3(ptr(wp), wp.numel(), ptr(planes), stream_ptr()))
            check(lib.fs_conv2d_nhwc_split(ptr(x), cin, ptr(planes), ptr(scale), ptr(shift), ptr(res), o, ptr(out), o, b, h, w, cin, o, kh, kw,
                                           stride, pad, dil, int(relu), tile, stream_ptr()))
        else:
            check(lib.fs_conv2d_nhwc(ptr(x), cin, ptr(wp), ptr(scale), ptr(shift), ptr(res), o, ptr(out), o, b, h, w, cin, o, kh, kw,
                                     stride, pad, dil, int(relu), tile, stream_ptr()))
    return out


def attention(qkv, heads, split_operands=True):
    """softmax(q k^T / 8) v per head (segm/model/blocks.py:39-66) for qkv [B, N, 3 * heads * 64] -> [B, N, heads * 64].
    split_operands: True the bf16-matrix-core route with three bf16 terms per fp32 value (the networks' default), False the fp32-MFMA one."""
    lib = _lib.load()
    with torch.cuda.device(one_device(qkv, what="floodseg.attention")):
        qkv = _f32c(qkv)
        b, n, c = qkv.shape
        if c != 3 * heads * 64:
            raise ValueError(f"floodseg.attention: last dim {c} != 3 * {heads} * 64")
        out = torch.empty((b, n, heads * 64), dtype=torch.float32, device=qkv.device)
        ws = torch.empty(max(1, lib.fs_attention_workspace_floats(b, n, heads, int(split_operands))), dtype=torch.float32, device=qkv.device)
        check(lib.fs_attention(ptr(qkv), ptr(out), b, n, heads, 0.125, int(split_operands), ptr(ws), stream_ptr()))
    return out
