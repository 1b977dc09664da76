"""GPU parity of the CNN heads' kernels and of the projection shortcut op by op (include/floodseg_test.h, the hooks after dec_assemble):
the concatenated-K conv3 + downsample launch on both arithmetic routes, the two filter repacks behind it and behind the fused head, the
pyramid pooling (one-pass and ragged), the batched small-M 1x1 conv, the upsample into a channel slice, the classifier, and the PSPNet
head finish (pyramid term + BatchNorm + ReLU + classifier) alone and behind the network's grouped Z GEMM.  Every check is against a
float64 torch-CPU restatement written here, or bit for bit against the route it claims to equal.  Outputs are allocated NaN-filled and
wider / longer than needed, inputs with NaN in their padding channels, so an unwritten, over-written or over-read element shows.
Tolerances are the constants of tests/test_gpu_ops.py (max |got - ref| / max |ref|): CONV_TOL for the fp32 accumulation chains (dual
conv, rowdot, classifier, pyramid term: at most 4096 + 512 terms), 5e-6 for pooling, INTERP_TOL for the upsample; an fp32 torch-CPU
evaluation of the same formulas is 1e-7 .. 7e-7 away from float64, so a correct kernel has no reason to come near them."""
import ctypes
import random

import pytest
from conftest import note
import torch
import torch.nn.functional as F

from flood_uav_video_segmentation_amd import _lib
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONV_TOL = 2e-5    # as tests/test_gpu_ops.py: fp32 matrix-core / fma sums against float64, K up to 4608
POOL_TOL = 5e-6    # as tests/test_gpu_ops.py::test_adaptive_avgpool (covers the hierarchical window sums of the one-pass pyramid)
INTERP_TOL = 2e-6  # as tests/test_gpu_ops.py
NAN = float("nan")
BINS = (1, 2, 3, 6)


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "unwritten (NaN) or non-finite output elements"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def padded(x, extra=4):
    """x [..., C] on the device inside a [..., C + extra] tensor whose padding channels are NaN; returns (view of the C channels, ld)."""
    buf = nans(*x.shape[:-1], x.shape[-1] + extra)
    buf[..., :x.shape[-1]] = x.to(DEV)
    return buf, x.shape[-1] + extra


def planes_of(w):
    planes = torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=DEV)
    check(_lib.load().fs_split_bf16x3(ptr(w), w.numel(), ptr(planes), stream_ptr()))
    return planes


def refused(rc, word):
    assert rc != 0
    msg = _lib.load().fs_last_error().decode()
    assert word in msg, msg


# --------------------------------------------------------------------------------------------------- filter repacks (exact)
def concat_scaled(wa, sa, ha, wb, sb, hb):
    O, Ka, Kb = wa.shape[0], wa.shape[1], wb.shape[1]
    out, shift = nans(O * (Ka + Kb) + 8), nans(O + 8)
    check(_lib.load().fs_concat_scaled_filters(ptr(wa), ptr(sa), ptr(ha), Ka, ptr(wb), ptr(sb), ptr(hb), Kb, ptr(out), ptr(shift), O, stream_ptr()))
    assert torch.isnan(out[O * (Ka + Kb):]).all() and torch.isnan(shift[O:]).all()
    return out[:O * (Ka + Kb)].view(O, Ka + Kb), shift[:O]


@pytest.mark.parametrize("O,Ka,Kb", [(64, 32, 32), (256, 64, 128), (2048, 512, 1024), (5, 3, 7)])
def test_concat_scaled_filters_is_exact(O, Ka, Kb):
    """One fp32 multiply per filter value and one add per bias: equal to the same expressions in fp32 on the CPU."""
    g = torch.Generator().manual_seed(O + Ka)
    wa, wb = torch.randn(O, Ka, generator=g), torch.randn(O, Kb, generator=g)
    sa, sb, ha, hb = (torch.randn(O, generator=g) for _ in range(4))
    bank, shift = concat_scaled(*(t.to(DEV) for t in (wa, sa, ha, wb, sb, hb)))
    assert torch.equal(bank[:, :Ka].cpu(), sa[:, None] * wa)
    assert torch.equal(bank[:, Ka:].cpu(), sb[:, None] * wb)
    assert torch.equal(shift.cpu(), ha + hb)


def pack_slice(w, c0, nc):
    O, I, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
    out = nans(taps * O * nc + 8)
    check(_lib.load().fs_pack_slice_tap_major(ptr(w), ptr(out), O, I, c0, nc, taps, stream_ptr()))
    assert torch.isnan(out[taps * O * nc:]).all()
    return out[:taps * O * nc].view(taps * O, nc)


@pytest.mark.parametrize("k", [1, 3])
def test_pack_slice_tap_major_is_the_permuted_slice(k):
    """Slices at the start, in the middle and at the end of the bank, 1 and 9 taps; a slice that leaves the bank is refused."""
    g = torch.Generator().manual_seed(k)
    O, I = 24, 160
    w = torch.randn(O, I, k, k, generator=g).to(DEV)
    for c0, nc in ((0, 32), (0, 1), (37, 64), (96, 64), (159, 1), (0, 160)):
        ref = w[:, c0:c0 + nc].reshape(O, nc, k * k).permute(2, 0, 1).reshape(k * k * O, nc)
        assert torch.equal(pack_slice(w, c0, nc), ref), (c0, nc)
    lib = _lib.load()
    out = nans(16)
    for c0, nc in ((128, 64), (-1, 8), (0, 0), (160, 1)):
        refused(lib.fs_pack_slice_tap_major(ptr(w), ptr(out), O, I, c0, nc, k * k, stream_ptr()), "channel range")


# --------------------------------------------------------------------------------------------------- conv3 + projection shortcut
def dual_conv(a, ld_a, b, ld_b, bank, planes, shift, B, Ho, Wo, Cin, Cin2, H2, W2, stride2, Cout, relu, tile):
    ld_out = Cout + 8
    out = nans(B, Ho, Wo, ld_out)
    check(_lib.load().fs_dual_conv(ptr(a), ld_a, ptr(b), ld_b, ptr(bank), ptr(planes), ptr(shift), ptr(out), ld_out, B, Ho, Wo, Cin, Cin2, H2, W2,
                                   stride2, Cout, relu, tile, stream_ptr()))
    assert torch.isnan(out[..., Cout:]).all(), "wrote past Cout"
    return out[..., :Cout]


DUAL_CASES = [  # B, H2, W2, stride2, Cin, Cin2, Cout
    (1, 45, 45, 2, 32, 32, 64),        # odd H2 / W2 under stride 2 (45 -> 23)
    (3, 46, 45, 2, 64, 128, 256),      # even / odd (46 -> 23, 45 -> 23): layer1's channel counts
    (1, 23, 17, 1, 512, 1024, 2048),   # layer4.0 of the network (stride 1: dilated)
    (3, 23, 17, 2, 128, 256, 512),     # layer2.0 (23 x 17 -> 12 x 9)
    (1, 2, 2, 2, 32, 64, 64),          # a single output pixel
    (1, 1, 1, 1, 64, 32, 128),         # ... and a single input pixel
]


@pytest.mark.parametrize("case", DUAL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dual_conv_against_float64_and_across_tiles(case):
    """relu(sa * conv(a, wa) + ha + sb * conv(b, wb, stride) + hb) with the bank from concat_scaled_filters, fp32-MFMA and split-operand
    routes, tiles 0 / 1 / 2; within a route every tile gives the same bits."""
    B, H2, W2, st, Cin, Cin2, Cout = case
    Ho, Wo = (H2 - 1) // st + 1, (W2 - 1) // st + 1
    g = torch.Generator().manual_seed(sum(case))
    a, b = torch.randn(B, Ho, Wo, Cin, generator=g), torch.randn(B, H2, W2, Cin2, generator=g)
    wa, wb = torch.randn(Cout, Cin, generator=g) * Cin ** -0.5, torch.randn(Cout, Cin2, generator=g) * Cin2 ** -0.5
    sa, sb = torch.rand(Cout, generator=g) + 0.5, torch.rand(Cout, generator=g) + 0.5
    ha, hb = torch.randn(Cout, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.1
    bank, shift = concat_scaled(*(t.to(DEV) for t in (wa, sa, ha, wb, sb, hb)))
    bank, shift = bank.contiguous(), shift.contiguous()
    ad, ld_a = padded(a)
    bd, ld_b = padded(b, 12)
    raw = sa.double() * (a.double() @ wa.double().t()) + ha.double() + sb.double() * (b[:, ::st, ::st].double() @ wb.double().t()) + hb.double()
    for relu in (1, 0):
        ref = raw.clamp_min(0) if relu else raw
        for route, planes in (("f32", None), ("split", planes_of(bank))):
            outs = [dual_conv(ad, ld_a, bd, ld_b, bank, planes, shift, B, Ho, Wo, Cin, Cin2, H2, W2, st, Cout, relu, t) for t in (0, 1, 2)]
            e = max(rel(o, ref) for o in outs)
            note(f"head_dual_conv_{route}_{'x'.join(map(str, case))}_relu{relu}", e)
            assert e < CONV_TOL, (case, route, relu, e)
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2]), (case, route, "tiles differ")


def test_dual_conv_refuses_bad_geometry():
    lib = _lib.load()
    x = torch.zeros(4096, device=DEV)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(a=ptr(x), ld_a=32, b=ptr(x), ld_b=32, w=ptr(x), pl=None, sh=None, out=ptr(x), ld_out=32, B=1, Ho=2,  # noqa: E731
                                                      Wo=2, Cin=32, Cin2=32, H2=3, W2=3, st=2, Cout=32, relu=1, tile=0).items()] + [stream_ptr()]
    refused(lib.fs_dual_conv(*args(tile=3)), "tile")
    refused(lib.fs_dual_conv(*args(tile=6)), "tile")
    refused(lib.fs_dual_conv(*args(H2=5)), "second operand")       # (5 - 1) / 2 + 1 != 2
    refused(lib.fs_dual_conv(*args(ld_b=16)), "second operand")    # ld_in2 < Cin2
    refused(lib.fs_dual_conv(*args(Cin2=48)), "second operand")
    refused(lib.fs_dual_conv(*args(st=0)), "bad arguments")


# --------------------------------------------------------------------------------------------------- pyramid pooling
def pyramid_pool(x, ld, B, H, W, C):
    out = nans(50 * B * C + 64)
    check(_lib.load().fs_pyramid_pool(ptr(x), ld, ptr(out), B, H, W, C, stream_ptr()))
    assert torch.isnan(out[50 * B * C:]).all()
    levels, off = [], 0
    for bin_ in BINS:
        levels.append(out[off:off + B * bin_ * bin_ * C].view(B, bin_ * bin_, C))
        off += B * bin_ * bin_ * C
    return levels


POOL_MAPS = [(6, 6), (6, 12), (12, 18), (90, 90), (5, 6), (13, 17), (21, 29), (7, 6)]


@pytest.mark.parametrize("H,W", POOL_MAPS)
def test_pyramid_pooling_against_float64(H, W):
    """Maps that are multiples of 6 (one pass + combine) and ragged ones (four launches, 5 x 6 and 7 x 6: windows of the 6 x 6 level that
    overlap or are single rows), C = 32 and 2048, B = 1 and 3, against F.adaptive_avg_pool2d in float64; on the divisible maps also against
    four plain adaptive_avgpool calls (the 6 x 6 level is the same launch: equal bits)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(H * 100 + W)
    combos = [(32, 3), (2048, 1)] if H * W > 1000 else [(32, 1), (32, 3), (2048, 1), (2048, 3)]
    for C, B in combos:
        x = torch.randn(B, H, W, C, generator=g) + 0.5
        xd, ld = padded(x)
        got = pyramid_pool(xd, ld, B, H, W, C)
        x64 = x.double().permute(0, 3, 1, 2)
        for bin_, lv in zip(BINS, got):
            ref = F.adaptive_avg_pool2d(x64, bin_).permute(0, 2, 3, 1).reshape(B, bin_ * bin_, C)
            e = rel(lv, ref)
            note(f"head_pyramid_pool_{H}x{W}_C{C}_B{B}_bin{bin_}", e)
            assert e < POOL_TOL, (H, W, C, B, bin_, e)
            if H % 6 == 0 and W % 6 == 0:
                plain = nans(B, bin_ * bin_, C)
                check(lib.fs_adaptive_avgpool_nhwc(ptr(xd), ld, ptr(plain), B, H, W, C, bin_, stream_ptr()))
                assert rel(lv, plain) < POOL_TOL, (H, W, C, B, bin_)
                if bin_ == 6:
                    assert torch.equal(lv, plain)


def test_pyramid_pool_refuses_bad_arguments():
    lib = _lib.load()
    x, out = torch.zeros(36 * 48, device=DEV), nans(50 * 64)
    refused(lib.fs_pyramid_pool(ptr(x), 48, ptr(out), 1, 6, 6, 48, stream_ptr()), "pyramid_pool")   # C % 32
    refused(lib.fs_pyramid_pool(ptr(x), 16, ptr(out), 1, 6, 6, 32, stream_ptr()), "pyramid_pool")   # ld_in < C
    refused(lib.fs_pyramid_pool(ptr(x), 32, ptr(out), 0, 6, 6, 32, stream_ptr()), "pyramid_pool")


# --------------------------------------------------------------------------------------------------- batched small-M 1x1 conv
def rowdot(xs, ws, scales, shifts, K, N, relu):
    """xs[i]: [M_i][K] CPU; returns the list of [M_i][N] outputs (checked: nothing written beyond row M_i or column N)."""
    n = len(xs)
    ld_in, ld_out = K + 4, N + 4
    xd = [padded(x)[0] for x in xs]
    outs = [nans(x.shape[0] + 2, ld_out) for x in xs]
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    Ms = (ctypes.c_int * n)(*[x.shape[0] for x in xs])
    check(_lib.load().fs_rowdot_batch(n, arr(xd), arr(ws), arr(scales), arr(shifts), arr(outs), Ms, ld_in, ld_out, K, N, relu, stream_ptr()))
    for x, o in zip(xs, outs):
        assert torch.isnan(o[x.shape[0]:]).all() and torch.isnan(o[:, N:]).all(), "wrote outside [M][N]"
    return [o[:x.shape[0], :N] for x, o in zip(xs, outs)]


ROWDOT_MS = [(1, 4, 9, 36), (3, 12, 27, 108), (1, 1, 1, 73)] + [(m,) for m in (1, 5, 6, 7, 71, 72, 73)]


@pytest.mark.parametrize("N", [4, 6, 256, 512])
@pytest.mark.parametrize("K", [256, 512, 2048, 4096])
def test_rowdot_batch_against_float64(K, N):
    """The row chunking is decided by the largest problem (gridDim.y = min(12, max M / 6)) and applied to all: M sets that put the
    problems on different sides of it, single problems around the 6- and 72-row steps; N that is not a whole block of 4 waves.
    Measured 1.4e-7 .. 7.2e-7, except K = 2048, N = 4 at 5.9e-6: with four output columns and a single row the ReLU leaves a reference
    whose largest value is far below the typical |dot product|, and the figure is relative to that largest value."""
    g = torch.Generator().manual_seed(K + N)
    w_all = torch.randn(4, N, K, generator=g) * K ** -0.5
    wd = [w_all[i].contiguous().to(DEV) for i in range(4)]
    sc_all, sh_all = torch.rand(4, N, generator=g) + 0.5, torch.randn(4, N, generator=g) * 0.3
    worst = 0.0
    for idx, Ms in enumerate(ROWDOT_MS):
        xs = [torch.randn(m, K, generator=g) for m in Ms]
        for affine, relu in (((1, 1), (0, 0)) if len(Ms) > 1 else ((idx % 2, (idx // 2) % 2),)):
            n = len(Ms)
            sc = [sc_all[i].to(DEV) if affine else None for i in range(n)]
            sh = [sh_all[i].to(DEV) if affine else None for i in range(n)]
            if affine and n > 1:
                sc[1] = None  # single entries may be NULL too
            got = rowdot(xs, wd[:n], sc, sh, K, N, relu)
            for i in range(n):
                ref = xs[i].double() @ w_all[i].double().t()
                if sc[i] is not None:
                    ref = ref * sc_all[i].double()
                if sh[i] is not None:
                    ref = ref + sh_all[i].double()
                if relu:
                    ref = ref.clamp_min(0)
                e = rel(got[i], ref)
                assert e < CONV_TOL, (K, N, Ms, i, affine, relu, e)
                worst = max(worst, e)
    note(f"head_rowdot_vs_f64_K{K}_N{N}", worst)


def test_rowdot_refuses_unsupported_k_and_bad_problems():
    lib = _lib.load()
    x, w, o = torch.zeros(8, 4400, device=DEV), torch.zeros(4, 4400, device=DEV), nans(8, 8)
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
    M = (ctypes.c_int * 1)(8)
    for K in (128, 4352):
        refused(lib.fs_rowdot_batch(1, one(x), one(w), None, None, one(o), M, 4400, 8, K, 4, 0, stream_ptr()), "rowdot")
    refused(lib.fs_rowdot_batch(5, one(x), one(w), None, None, one(o), M, 4400, 8, 256, 4, 0, stream_ptr()), "rowdot")
    refused(lib.fs_rowdot_batch(1, one(x), one(w), None, None, one(o), M, 128, 8, 256, 4, 0, stream_ptr()), "rowdot")   # ld_in < K
    refused(lib.fs_rowdot_batch(1, one(x), one(w), None, None, one(o), (ctypes.c_int * 1)(0), 4400, 8, 256, 4, 0, stream_ptr()), "rowdot")


# --------------------------------------------------------------------------------------------------- upsample into a channel slice
@pytest.mark.parametrize("ac", [1, 0])
@pytest.mark.parametrize("hw", [1, 2, 3, 6])
def test_upsample_into_a_slice_of_a_wider_buffer(hw, ac):
    """The pyramid's align_corners = True upsampling (PPM) and align_corners = False (ASPP's pooled 1 x 1 map), written at a channel
    offset of a wider NHWC buffer whose other channels must keep their NaNs."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(10 * hw + ac)
    B, C, off, ld = 2, 32, 36, 100
    src = torch.randn(B, hw * hw, C, generator=g)
    sd = src.to(DEV)
    worst = 0.0
    for Ho, Wo in ((5, 6), (13, 17), (90, 90)):
        buf = nans(B, Ho, Wo, ld)
        check(lib.fs_upsample_into(ptr(sd), hw, hw, ctypes.c_void_p(buf.data_ptr() + 4 * off), ld, B, Ho, Wo, C, ac, stream_ptr()))
        assert torch.isnan(buf[..., :off]).all() and torch.isnan(buf[..., off + C:]).all(), "wrote outside the slice"
        ref = F.interpolate(src.double().view(B, hw, hw, C).permute(0, 3, 1, 2), (Ho, Wo), mode="bilinear", align_corners=bool(ac))
        e = rel(buf[..., off:off + C], ref.permute(0, 2, 3, 1))
        assert e < INTERP_TOL, (hw, ac, Ho, Wo, e)
        worst = max(worst, e)
    note(f"head_upsample_into_{hw}x{hw}_ac{ac}", worst)
    buf = nans(2, 5, 6, ld)
    refused(lib.fs_upsample_into(ptr(sd), hw, hw, ptr(buf), 16, B, 5, 6, C, ac, stream_ptr()), "upsample_into")            # ld_out < C
    refused(lib.fs_upsample_into(ptr(sd), hw, hw, ctypes.c_void_p(buf.data_ptr() + 4), ld, B, 5, 6, C, ac, stream_ptr()), "upsample_into")  # unaligned


# --------------------------------------------------------------------------------------------------- classifier
@pytest.mark.parametrize("K,C", [(1, 512), (5, 512), (8, 512), (9, 512), (16, 512), (19, 512), (32, 512), (64, 256), (33, 256)])
def test_classifier_nchw_against_float64(K, C):
    """Classes in passes of 8 with a remainder, pixel counts that leave the last 16-pixel block partly empty, ld_in > C, with and
    without bias; K * C up to exactly the 64 KiB of LDS."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(K * 1000 + C)
    w, bias = torch.randn(K, C, generator=g) * C ** -0.5, torch.randn(K, generator=g)
    wd, bd = w.to(DEV), bias.to(DEV)
    worst = 0.0
    for B, HW in ((1, 1), (1, 17), (3, 221), (2, 16)):
        x = torch.randn(B, HW, C, generator=g)
        xd, ld = padded(x)
        for b in (bd, None):
            out = nans(B * K * HW + 32)
            check(lib.fs_classifier_nchw(ptr(xd), ld, ptr(wd), ptr(b), ptr(out), B, HW, C, K, stream_ptr()))
            assert torch.isnan(out[B * K * HW:]).all()
            ref = x.double() @ w.double().t() + (bias.double() if b is not None else 0)
            e = rel(out[:B * K * HW].view(B, K, HW), ref.permute(0, 2, 1))
            assert e < CONV_TOL, (K, C, B, HW, b is not None, e)
            worst = max(worst, e)
    note(f"head_classifier_vs_f64_K{K}_C{C}", worst)


def test_classifier_refuses_filters_larger_than_lds():
    lib = _lib.load()
    x, w, out = torch.zeros(16, 512, device=DEV), torch.zeros(65 * 512, device=DEV), nans(65 * 16)
    refused(lib.fs_classifier_nchw(ptr(x), 512, ptr(w), None, ptr(out), 1, 16, 512, 33, stream_ptr()), "LDS")   # one row over 32 x 512
    refused(lib.fs_classifier_nchw(ptr(x), 256, ptr(w), None, ptr(out), 1, 16, 256, 65, stream_ptr()), "LDS")   # one row over 64 x 256
    refused(lib.fs_classifier_nchw(ptr(x), 128, ptr(w), None, ptr(out), 1, 16, 256, 5, stream_ptr()), "classifier")  # ld_in < C


# --------------------------------------------------------------------------------------------------- PSPNet head finish
def head_inputs(g, B, H, W, C, K, Cr):
    """Random head: raw conv sums T, pooled maps p_i [B][Cr][bin][bin], the levels' 3x3 filters Wp [C][4 * Cr][3][3], BatchNorm, classifier."""
    T = torch.randn(B, H, W, C, generator=g)
    pools = [torch.randn(B, Cr, b, b, generator=g) for b in BINS]
    Wp = torch.randn(C, 4 * Cr, 3, 3, generator=g) * (36 * Cr) ** -0.5
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    cls_w, cls_b = torch.randn(K, C, generator=g) * C ** -0.5, torch.randn(K, generator=g)
    return T, pools, Wp, scale, shift, cls_w, cls_b


def head64(T, pools, Wp, scale, shift, cls_w, cls_b, relu):
    """cls(act(scale * (T + sum_b conv3x3(interp_ac1(p_b), W_b, pad 1)) + shift)) + bias in float64 -> [B][K][H][W]"""
    B, H, W, _ = T.shape
    ups = torch.cat([F.interpolate(p.double(), (H, W), mode="bilinear", align_corners=True) for p in pools], 1)
    v = T.double().permute(0, 3, 1, 2) + F.conv2d(ups, Wp.double(), padding=1)
    if scale is not None:
        v = v * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        v = v + shift.double().view(1, -1, 1, 1)
    if relu:
        v = v.clamp_min(0)
    out = torch.einsum("bchw,kc->bkhw", v, cls_w.double())
    return out + cls_b.double().view(1, -1, 1, 1) if cls_b is not None else out


def z_maps(pools, Wp):
    """Z_i[b * bin^2 + cell][tap][o] = sum_c Wp[o][i * Cr + c][tap] * p_i[b][c][cell], computed in float64 and rounded to fp32 once."""
    Cr = pools[0].shape[1]
    zs = []
    for i, p in enumerate(pools):
        B, _, b, _ = p.shape
        z = torch.einsum("bcij,octs->bijtso", p.double(), Wp[:, i * Cr:(i + 1) * Cr].double())
        zs.append(z.reshape(B * b * b, 9, Wp.shape[0]).float().contiguous().to(DEV))
    return zs


def ppm_term_classify(T, zs, scale, shift, cls_w, cls_b, relu):
    lib = _lib.load()
    B, H, W, C = T.shape
    K = cls_w.shape[0]
    Td, ld = padded(T)
    sc, sh, cw, cb = (t.to(DEV) if t is not None else None for t in (scale, shift, cls_w, cls_b))  # kept alive across the call
    scratch = nans(lib.fs_ppm_term_scratch_floats(B, H, C))
    out = nans(B * K * H * W + 32)
    bins = (ctypes.c_int * 4)(*BINS)
    check(lib.fs_ppm_term_classify(ptr(Td), ld, ptr(zs[0]), ptr(zs[1]), ptr(zs[2]), ptr(zs[3]), bins, ptr(sc), ptr(sh), B, H, W, C, relu, ptr(cw),
                                   ptr(cb), ptr(out), K, ptr(scratch), stream_ptr()))
    assert torch.isnan(out[B * K * H * W:]).all()
    assert torch.equal(Td[..., :C].cpu(), T), "T is read once and never written back"
    return out[:B * K * H * W].view(B, K, H, W)


HEAD_KS = (1, 5, 8, 9, 19, 33)
HEAD_WIDTHS = (5, 6, 7, 11, 12, 13, 17, 29)


@pytest.mark.parametrize("H", [5, 6, 13])
@pytest.mark.parametrize("W", HEAD_WIDTHS)
def test_ppm_term_classify_map_geometries(W, H):
    """C = 512 (the network's).  Widths that put the map's right edge at every position of a 6-pixel run, maps narrower and lower than
    the 6 x 6 level; the class count walks through 1, 5, 8, 9, 19, 33 (whole passes of 8, remainders, more than four passes)."""
    K = HEAD_KS[(HEAD_WIDTHS.index(W) + H) % len(HEAD_KS)]
    g = torch.Generator().manual_seed(W * 100 + H)
    T, pools, Wp, scale, shift, cls_w, cls_b = head_inputs(g, 1, H, W, 512, K, 4)
    got = ppm_term_classify(T, z_maps(pools, Wp), scale, shift, cls_w, cls_b, 1)
    e = rel(got, head64(T, pools, Wp, scale, shift, cls_w, cls_b, 1))
    note(f"head_ppm_term_classify_{H}x{W}_K{K}", e)
    assert e < CONV_TOL, (H, W, K, e)


@pytest.mark.parametrize("K", HEAD_KS)
@pytest.mark.parametrize("C", [4, 252, 260, 512, 1024])
def test_ppm_term_classify_channel_and_class_counts(C, K):
    """C / 4 lanes that are not whole waves (`dup` lanes: 4, 252, 260) and that are (512, 1024), one to four waves; every class-pass
    remainder; ReLU on / off and BatchNorm present / absent in all four combinations over the cases; B = 3; two map shapes."""
    combo = (HEAD_KS.index(K) + C // 4) % 4
    relu, affine = combo & 1, combo >> 1
    g = torch.Generator().manual_seed(C * 100 + K)
    worst = 0.0
    for H, W in ((6, 13), (5, 7)):
        T, pools, Wp, scale, shift, cls_w, cls_b = head_inputs(g, 3, H, W, C, K, 4)
        if not affine:
            scale = shift = None
        got = ppm_term_classify(T, z_maps(pools, Wp), scale, shift, cls_w, cls_b, relu)
        e = rel(got, head64(T, pools, Wp, scale, shift, cls_w, cls_b, relu))
        assert e < CONV_TOL, (C, K, H, W, relu, affine, e)
        worst = max(worst, e)
    note(f"head_ppm_term_classify_C{C}_K{K}", worst)


@pytest.mark.parametrize("relu,has_scale,has_shift,has_bias", [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 0, 1), (0, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 1)])
def test_ppm_term_classify_optional_epilogue_parts(relu, has_scale, has_shift, has_bias):
    g = torch.Generator().manual_seed(relu * 8 + has_scale * 4 + has_shift * 2 + has_bias)
    T, pools, Wp, scale, shift, cls_w, cls_b = head_inputs(g, 3, 6, 11, 512, 5, 4)
    scale, shift, cls_b = scale if has_scale else None, shift if has_shift else None, cls_b if has_bias else None
    got = ppm_term_classify(T, z_maps(pools, Wp), scale, shift, cls_w, cls_b, relu)
    e = rel(got, head64(T, pools, Wp, scale, shift, cls_w, cls_b, relu))
    assert e < CONV_TOL, e


@pytest.mark.parametrize("H,W,C,K", [(13, 17, 512, 5), (5, 7, 252, 9), (6, 12, 1024, 33)])
def test_ppm_term_classify_batch_equals_single_images(H, W, C, K):
    """DESIGN: a frame's result never depends on the batch it is processed in -- bit for bit."""
    g = torch.Generator().manual_seed(H + W + C + K)
    T, pools, Wp, scale, shift, cls_w, cls_b = head_inputs(g, 3, H, W, C, K, 4)
    both = ppm_term_classify(T, z_maps(pools, Wp), scale, shift, cls_w, cls_b, 1)
    for b in range(3):
        one = ppm_term_classify(T[b:b + 1], z_maps([p[b:b + 1] for p in pools], Wp), scale, shift, cls_w, cls_b, 1)
        assert torch.equal(one[0], both[b]), b


def test_ppm_term_classify_refuses_bad_arguments():
    lib = _lib.load()
    x, out = torch.zeros(1 << 16, device=DEV), nans(1 << 12)
    good = (ctypes.c_int * 4)(*BINS)

    def call(bins=good, C=8, ld=8, K=2, z6=x):
        return lib.fs_ppm_term_classify(ptr(x), ld, ptr(x), ptr(x), ptr(x), ptr(z6), bins, None, None, 1, 5, 5, C, 1, ptr(x), None, ptr(out), K, ptr(x),
                                        stream_ptr())
    refused(call(bins=(ctypes.c_int * 4)(1, 2, 3, 5)), "pyramid levels")
    refused(call(bins=(ctypes.c_int * 4)(1, 1, 3, 7)), "pyramid level")    # adds up to 12, but a level wider than the six-column table
    refused(call(C=6), "ppm_term_classify")
    refused(call(C=1028, ld=1028), "ppm_term_classify")
    refused(call(ld=4), "bad arguments")
    refused(call(K=0), "bad arguments")
    refused(call(z6=None), "pyramid level")


# --------------------------------------------------------------------------------------------------- the whole fused head after the main conv
def ppm_head(T, pools, Wp, scale, shift, cls_w, cls_b, relu, split, c_main=32):
    """fs_ppm_head: the levels' filters are cut tap-major out of an OIHW bank [C][c_main + 4 * Cr][3][3] by pack_slice_tap_major (as
    fs_finalize does), the reduced maps sit in their 36-row slots (unused rows NaN), then the network's grouped Z GEMM and the finish."""
    lib = _lib.load()
    B, H, W, C = T.shape
    K, Cr = cls_w.shape[0], pools[0].shape[1]
    bank = torch.cat([torch.full((C, c_main, 3, 3), NAN), Wp], 1).contiguous().to(DEV)
    zw = torch.cat([pack_slice(bank, c_main + i * Cr, Cr).reshape(-1) for i in range(4)]).contiguous()
    reduced = nans(4, B * 36, Cr)
    for i, p in enumerate(pools):
        b = p.shape[2]
        reduced[i, :B * b * b] = p.permute(0, 2, 3, 1).reshape(B * b * b, Cr).to(DEV)
    Td, ld = padded(T)
    sc, sh, cw, cb = (t.to(DEV) if t is not None else None for t in (scale, shift, cls_w, cls_b))  # kept alive across the call
    planes = planes_of(zw) if split else None
    ws = nans(lib.fs_ppm_head_workspace_floats(B, H, C) + 16)
    out = nans(B * K * H * W + 32)
    bins = (ctypes.c_int * 4)(*BINS)
    check(lib.fs_ppm_head(ptr(Td), ld, ptr(reduced), Cr, ptr(zw), ptr(planes), bins, ptr(sc), ptr(sh), B, H, W, C, relu, ptr(cw), ptr(cb), ptr(out), K,
                          ptr(ws), stream_ptr()))
    assert torch.isnan(out[B * K * H * W:]).all() and torch.isnan(ws[-16:]).all()
    return out[:B * K * H * W].view(B, K, H, W)


@pytest.mark.parametrize("split", [0, 1], ids=["f32", "split"])
@pytest.mark.parametrize("B,H,W,C,K,Cr", [(1, 6, 6, 128, 5, 32), (3, 13, 17, 512, 19, 32), (2, 5, 7, 64, 33, 64), (1, 13, 17, 512, 5, 512), (3, 12, 6, 256, 8, 32)])
def test_fused_head_behind_the_grouped_z_gemm(B, H, W, C, K, Cr, split):
    """Z from the network's grouped GEMM (four levels, one launch) on both arithmetic routes, then the finish: one float64 expression
    for everything the fused PSPNet route runs after the main head conv.  (1, 13, 17, 512, 5, 512) is the network's own size."""
    g = torch.Generator().manual_seed(B + H * W + C + K + Cr)
    T, pools, Wp, scale, shift, cls_w, cls_b = head_inputs(g, B, H, W, C, K, Cr)
    got = ppm_head(T, pools, Wp, scale, shift, cls_w, cls_b, 1, split)
    e = rel(got, head64(T, pools, Wp, scale, shift, cls_w, cls_b, 1))
    note(f"head_fused_head_{'split' if split else 'f32'}_B{B}_{H}x{W}_C{C}_K{K}_Cr{Cr}", e)
    assert e < CONV_TOL, e
    if B > 1:
        one = ppm_head(T[1:2], [p[1:2] for p in pools], Wp, scale, shift, cls_w, cls_b, 1, split)
        assert torch.equal(one[0], got[1])


def test_fused_head_on_seeded_random_shapes():
    """About 20 draws over H, W in 5..40, K in 1..40, B in 1..3 (C, the route and the epilogue drawn too); the shapes are printed on failure."""
    rng = random.Random(20261016)
    worst = 0.0
    for draw in range(20):
        B, H, W, K = rng.randint(1, 3), rng.randint(5, 40), rng.randint(5, 40), rng.randint(1, 40)
        C, split, relu, affine = rng.choice((64, 128, 256, 512)), rng.randint(0, 1), rng.randint(0, 1), rng.randint(0, 1)
        shape = dict(draw=draw, B=B, H=H, W=W, K=K, C=C, split=split, relu=relu, affine=affine)
        g = torch.Generator().manual_seed(1000 + draw)
        T, pools, Wp, scale, shift, cls_w, cls_b = head_inputs(g, B, H, W, C, K, 32)
        if not affine:
            scale = shift = None
        got = ppm_head(T, pools, Wp, scale, shift, cls_w, cls_b, relu, split)
        e = rel(got, head64(T, pools, Wp, scale, shift, cls_w, cls_b, relu))
        assert e < CONV_TOL, (shape, e)
        worst = max(worst, e)
    note("head_fused_head_random_sweep_worst", worst)
