"""GPU parity of the Segmenter's kernels op by op (include/floodseg_test.h, the hooks after nhwc_to_nchw): LayerNorm, the Linear on both
arithmetic routes with and without split-K (and the merge + LayerNorm pass), the qkv Linear whose epilogue writes the attention's K / V^T
planes, the mask head, patchify and the two token assemblies.  Every check is against a float64 restatement of the op, or bit for bit
against the route it claims to equal.  The network tests (test_gpu_vit.py) only see these through a 1e-3 logit tolerance.
Tolerances are relative to the reference's max |value|: LN_TOL and MASK_TOL are about 3 x the error measured on the MI355X, the Linear
and attention checks keep the bounds of test_gpu_ops.py (measured here 10-20 x below them); note() records every measurement."""
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
CONV_TOL = 2e-5  # as tests/test_gpu_ops.py: fp32 matrix-core sums against float64, K up to 4608
LN_TOL = 1e-6    # LayerNorm of O(1) rows against float64: measured <= 3.6e-7 (D = 4), 1.2-1.8e-7 elsewhere (an ulp or two of the output)
ATT_TOL = 2e-5   # as tests/test_gpu_ops.py::test_attention_both_routes_against_float64 (measured here <= 1.1e-6)
MASK_TOL = 1e-5  # mask head: cosine scores x LayerNorm over K, which divides by the scores' spread (~1/sqrt(D)): measured <= 3.6e-6


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def ln64(x, g, b):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5) * g.double() + b.double()


def planes_of(w):
    """split_bf16x3 planes of a [N][K] weight (the split-operand route's filter bank)."""
    planes = torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=DEV)
    check(_lib.load().fs_split_bf16x3(ptr(w), w.numel(), ptr(planes), stream_ptr()))
    return planes


def layernorm(x, g, b, rows_per_batch=0, drop_first=0):
    rows, D = x.shape
    out = torch.full((rows - (rows // rows_per_batch if drop_first else 0), D), float("nan"), device=DEV)
    check(_lib.load().fs_layernorm(ptr(x), ptr(g), ptr(b), ptr(out), rows, D, rows_per_batch, drop_first, stream_ptr()))
    return out


def linear(x, w, planes, bias=None, res=None, act=0, nsplit=1, rows_per_image=0, ln=None):
    """fs_linear; returns out (and ln_out when ln = (gamma, beta)).  `part` is sized for the largest split the call can take."""
    lib = _lib.load()
    rows, K = x.shape
    N = w.shape[0]
    out = torch.full((rows, N), float("nan"), device=DEV)
    part = torch.full((max(nsplit, 4) * rows * N,), float("nan"), device=DEV) if nsplit != 1 else None
    g, b = ln if ln else (None, None)
    ln_out = torch.full((rows, N), float("nan"), device=DEV) if ln else None
    check(lib.fs_linear(ptr(x), ptr(w), ptr(planes), ptr(bias), ptr(res), ptr(out), rows, K, N, act, nsplit, rows_per_image, ptr(part),
                        ptr(g), ptr(b), ptr(ln_out), stream_ptr()))
    return (out, ln_out) if ln else out


def linear64(x, w, bias=None, res=None, act=0):
    y = x.double().cpu() @ w.double().cpu().t()
    if bias is not None:
        y = y + bias.double().cpu()
    if res is not None:
        y = y + res.double().cpu()
    return 0.5 * y * (1 + torch.erf(y / 2 ** 0.5)) if act == 2 else y


def weights(g, K, N, bias=True):
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV)
    return w, (torch.randn(N, generator=g) * 0.1).to(DEV) if bias else None


# ----------------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("D", [4, 64, 252, 256, 260, 384, 512, 768, 1020, 1024])
def test_layernorm_against_float64(D):
    """Every instantiation NI = 1..4 (chunks of 64 float4), partial last chunks (252, 260, 1020), rows that leave the last workgroup's
    waves idle (1, 3, 5, 4097); drop_first (the encoder's final norm without the cls token) against the kept rows in compacted order."""
    g = torch.Generator().manual_seed(D)
    gam, bet = (torch.rand(D, generator=g) + 0.5).to(DEV), (torch.randn(D, generator=g) * 0.3).to(DEV)
    worst = 0.0
    for rows in (1, 3, 4, 5, 4097):
        x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(DEV)
        e = rel(layernorm(x, gam, bet), ln64(x.cpu(), gam.cpu(), bet.cpu()))
        assert e < LN_TOL, (D, rows, e)
        worst = max(worst, e)
    for B, T in ((1, 5), (3, 7), (3, 197)):
        x = torch.randn(B * T, D, generator=g).to(DEV)
        ref = ln64(x.cpu().view(B, T, D)[:, 1:].reshape(-1, D), gam.cpu(), bet.cpu())
        e = rel(layernorm(x, gam, bet, T, 1), ref)
        assert e < LN_TOL, (D, B, T, e)
        worst = max(worst, e)
    note(f"vit_layernorm_vs_f64_D{D}", worst)


def test_layernorm_awkward_rows():
    """Constant rows (variance 0: the output is beta exactly -- (x - mean) is 0 -- where the constant is exactly representable and sums
    exactly), rows with mean 1e3 and std 1 (the two-pass variance keeps them accurate), rows of +-1e-20 (variance far below eps)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for D in (64, 384, 768, 1024):
        gam, bet = (torch.rand(D, generator=g) + 0.5).to(DEV), torch.randn(D, generator=g).to(DEV)
        const = torch.tensor([0.0, 3.0, -0.75, 1024.0]).view(-1, 1).expand(4, D).contiguous().to(DEV)
        got = layernorm(const, gam, bet)
        assert torch.equal(got, bet.expand(4, D)), D
        big = (1e3 + torch.randn(33, D, generator=g, dtype=torch.float64)).float().to(DEV)
        e_big = rel(layernorm(big, gam, bet), ln64(big.cpu(), gam.cpu(), bet.cpu()))
        note(f"vit_layernorm_mean1e3_vs_f64_D{D}", e_big)
        assert e_big < 6e-5, (D, e_big)  # the fp32 mean of values near 1e3 is off by ~1e-5 of the unit spread: measured <= 2.6e-5
        tiny = (torch.randint(0, 2, (9, D), generator=g).float() * 2 - 1) * 1e-20
        e_tiny = rel(layernorm(tiny.to(DEV), gam, bet), ln64(tiny, gam.cpu(), bet.cpu()))
        assert e_tiny < LN_TOL, (D, e_tiny)
    x = torch.zeros(8, 1028, device=DEV)
    for D in (1028, 6, 2):
        assert lib.fs_layernorm(ptr(x), ptr(x), ptr(x), ptr(x), 2, D, 0, 0, stream_ptr()) != 0, D


# ----------------------------------------------------------------------------------------------------------------------- Linear
LINEAR_CASES = [
    # rows, K, N, bias, res, act (the Segmenter's Linears at S / B / L widths, and ragged row counts)
    (1, 384, 1152, True, False, 0),      # qkv, one token
    (63, 384, 384, True, True, 0),       # proj + shortcut
    (129, 384, 1536, True, False, 2),    # fc1 + GELU
    (2026, 1536, 384, True, True, 0),    # fc2 S/16 at 713
    (1937, 768, 2304, True, False, 0),   # qkv B at 704
    (129, 3072, 768, True, True, 0),     # fc2 B
    (63, 4096, 1024, False, True, 0),    # fc2 L
    (2026, 768, 96, False, False, 0),
    (1, 4096, 3072, True, True, 0),
    (63, 1536, 1152, False, True, 0),
    (129, 768, 3072, True, False, 2),
]


@pytest.mark.parametrize("case", LINEAR_CASES)
def test_linear_both_routes_against_float64(case):
    """fs_linear without split-K on the fp32 matrix cores and on the split-operand route (the network's default) against a float64
    Linear; the split route is as accurate as the fp32 one (the convention of test_gpu_ops.py)."""
    rows, K, N, has_bias, has_res, act = case
    g = torch.Generator().manual_seed(rows * 7 + K + N)
    x = torch.randn(rows, K, generator=g).to(DEV)
    w, bias = weights(g, K, N, has_bias)
    res = torch.randn(rows, N, generator=g).to(DEV) if has_res else None
    ref = linear64(x, w, bias, res, act)
    e32 = note(f"vit_linear_fp32_vs_f64_{rows}x{K}x{N}", rel(linear(x, w, None, bias, res, act), ref))
    es = note(f"vit_linear_split_vs_f64_{rows}x{K}x{N}", rel(linear(x, w, planes_of(w), bias, res, act), ref))
    assert e32 < CONV_TOL and es < CONV_TOL, (e32, es)
    assert es < 1.5 * e32 + 1e-7, (es, e32)


SPLITK_CASES = [(129, 1536, 384), (63, 3072, 768), (33, 768, 1024), (5, 1536, 96), (17, 768, 256)]  # N <= 512: NI = 2; N > 512: NI = 4


@pytest.mark.parametrize("case", SPLITK_CASES)
@pytest.mark.parametrize("route", ["fp32", "split"])
def test_splitk_merges_against_float64_and_each_other(case, route):
    """Forced split-K (nsplit 2, 3, 4: the compile-time merge; 6 and 8: the generic NS = 0 merge).  The merge + LayerNorm pass
    (splitk_combine_ln) must give the plain merge's `out` bit for bit, and its ln_out must be the LayerNorm hook applied to that `out`,
    bit for bit.  The LayerNorm runs another instantiation NI than the merge at D = 96, 256 (1 against 2) and 768 (3 against 4); both
    kernels take the variance from vit_ops.hip::ln_sq_sum, whose fma chain is written out -- left to the compiler's contraction, NI = 1
    compiled to multiplies and separate adds and D <= 256 came out 1 ulp off.  With and without bias / residual."""
    rows, K, N = case
    g = torch.Generator().manual_seed(rows + K + N)
    x = torch.randn(rows, K, generator=g).to(DEV)
    w, bias = weights(g, K, N)
    planes = planes_of(w) if route == "split" else None
    res = torch.randn(rows, N, generator=g).to(DEV)
    gam, bet = (torch.rand(N, generator=g) + 0.5).to(DEV), (torch.randn(N, generator=g) * 0.3).to(DEV)
    worst = 0.0
    for with_extras in (True, False):
        b, r = (bias, res) if with_extras else (None, None)
        ref = linear64(x, w, b, r)
        for ns in (2, 3, 4, 6, 8):
            if K % (32 * ns):
                continue
            out = linear(x, w, planes, b, r, nsplit=ns)
            out_ln, ln_out = linear(x, w, planes, b, r, nsplit=ns, ln=(gam, bet))
            assert torch.equal(out, out_ln), (ns, with_extras)
            assert torch.equal(ln_out, layernorm(out, gam, bet)), (ns, with_extras)
            e = rel(out, ref)
            assert e < CONV_TOL, (ns, with_extras, e)
            worst = max(worst, e)
    note(f"vit_splitk_{route}_vs_f64_{rows}x{K}x{N}", worst)


def test_splitk_refusals():
    lib = _lib.load()
    x, w = torch.zeros(4, 768, device=DEV), torch.zeros(96, 768, device=DEV)
    out, part = torch.zeros(4, 96, device=DEV), torch.zeros(16 * 4 * 96, device=DEV)
    s = stream_ptr()
    assert lib.fs_linear(ptr(x), ptr(w), None, None, None, ptr(out), 4, 768, 96, 0, 5, 0, ptr(part), None, None, None, s) != 0  # 768 % 160
    assert lib.fs_linear(ptr(x), ptr(w), None, None, None, ptr(out), 4, 768, 96, 2, 2, 0, ptr(part), None, None, None, s) != 0  # GELU
    assert lib.fs_linear(ptr(x), ptr(w), None, None, None, ptr(out), 4, 768, 96, 0, 2, 0, None, None, None, None, s) != 0  # no part
    assert lib.fs_linear(ptr(x), ptr(w), None, None, None, ptr(out), 4, 768, 96, 0, 1, 0, None, ptr(w), ptr(w), ptr(out), s) != 0  # LN, no split
    check(lib.fs_linear(ptr(x), ptr(w), None, None, None, ptr(out), 4, 768, 96, 0, 2, 0, ptr(part), None, None, None, s))


@pytest.mark.parametrize("shape", [(197, 1536, 384), (1937, 1536, 384), (577, 3072, 768), (145, 4096, 1024)])
@pytest.mark.parametrize("route", ["fp32", "split"])
def test_library_split_choice_does_not_depend_on_the_batch(shape, route):
    """nsplit = 0 with rows_per_image = tokens: the split count (and the cost model's tile) is decided per image, so the rows of image 0
    are bit-identical whether it is computed alone or as the first of two -- what the key-frame cache relies on."""
    T, K, N = shape
    lib = _lib.load()
    assert lib.fs_linear_splits(K, N, T, 0, int(route == "split")) >= 2, shape  # the shapes do take split-K
    g = torch.Generator().manual_seed(T + K)
    x = torch.randn(2 * T, K, generator=g).to(DEV)
    w, bias = weights(g, K, N)
    res = torch.randn(2 * T, N, generator=g).to(DEV)
    planes = planes_of(w) if route == "split" else None
    both = linear(x, w, planes, bias, res, nsplit=0, rows_per_image=T)
    one = linear(x[:T].contiguous(), w, planes, bias, res[:T].contiguous(), nsplit=0, rows_per_image=T)
    assert torch.equal(both[:T], one)
    assert rel(one, linear64(x[:T], w, bias, res[:T])) < CONV_TOL


# ----------------------------------------------------------------------------------------------------------------------- qkv + attention
def vt_positions(Npad):
    """V^T column of key k: inside each 16 keys (k & 3) + 4 (k >> 3) + 8 ((k >> 2) & 1) (the S^T accumulator's key order)."""
    k = torch.arange(Npad)
    kk = k & 15
    return (k & ~15) + (kk & 3) + 4 * (kk >> 3) + 8 * ((kk >> 2) & 1)


def qkv_attention(x, w, planes, bias, B, T, D, fused):
    lib = _lib.load()
    qkv = torch.full((B * T, 3 * D), float("nan"), device=DEV)
    att = torch.full((B * T, D), float("nan"), device=DEV)
    ws = torch.empty(lib.fs_qkv_attention_workspace_floats(B, T, D), device=DEV)
    ws.view(torch.uint8).fill_(0xFF)  # NaN bytes: whatever the call does not write shows up
    check(lib.fs_qkv_attention(ptr(x), ptr(w), ptr(planes), ptr(bias), B, T, D, ptr(qkv), ptr(att), fused, ptr(ws), stream_ptr()))
    torch.cuda.synchronize()
    return qkv, att, ws


def attention64(qkv, B, T, heads):
    q, k, v = [t.reshape(B, T, heads, 64).permute(0, 2, 1, 3) for t in qkv.double().cpu().split(heads * 64, dim=1)]
    return (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * T, heads * 64)


QKV_TOKENS = [1, 31, 32, 33, 127, 128, 129, 197]


@pytest.mark.parametrize("D", [192, 384, 576, 768, 960])
def test_qkv_epilogue_planes_and_attention(D):
    """The qkv Linear that writes the attention's K / V^T bf16 x 3 planes from its epilogue (fused = 1) against the plain Linear + the
    attention's pre-pass (fused = 0), on a workspace filled with NaN bytes: the planes are byte-equal over their whole extent, the pad keys
    [tokens, Npad) are zeros, the planes add up to the K / V columns of qkv exactly, Q and the attention output are bit-equal across the two
    routes, and the attention is within ATT_TOL of a float64 attention of the returned qkv.  Odd head counts (D = 192, 576, 960: 3, 9, 15
    heads), token counts at and around the 32-key groups, B = 1, 2, 3."""
    heads = D // 64
    g = torch.Generator().manual_seed(D)
    w, bias = weights(g, D, 3 * D)
    w = w * 1.5  # q / k / v of spread 1.5 (as test_gpu_ops.py): attention far from uniform
    planes = planes_of(w)
    cases = [(T, 1 + i % 3) for i, T in enumerate(QKV_TOKENS)]
    if D == 384:
        cases += [(1937, 1), (2026, 2)]  # the S/16 token counts at 704 / 713 (key split + merge)
    worst = 0.0
    for T, B in cases:
        Npad = (T + 31) // 32 * 32
        pe = B * heads * Npad * 64
        x = torch.randn(B * T, D, generator=g).to(DEV)
        qkv_f, att_f, ws_f = qkv_attention(x, w, planes, bias, B, T, D, 1)
        qkv_u, att_u, ws_u = qkv_attention(x, w, planes, bias, B, T, D, 0)
        pf, pu = ws_f.view(torch.int16)[:6 * pe], ws_u.view(torch.int16)[:6 * pe]
        assert torch.equal(pf, pu), (D, T, B, (pf != pu).nonzero()[:4].flatten().tolist())
        kp = ws_u.view(torch.bfloat16)[:3 * pe].view(3, B * heads, Npad, 64).double().cpu()
        vp = ws_u.view(torch.bfloat16)[3 * pe:6 * pe].view(3, B * heads, 64, Npad).double().cpu()
        assert not kp[:, :, T:].any() and not vp[:, :, :, vt_positions(Npad)[T:]].any(), (D, T, B)
        kv = qkv_u.cpu().view(B, T, 3, heads, 64)
        k_ref = kv[:, :, 1].permute(0, 2, 1, 3).reshape(B * heads, T, 64).double()
        v_ref = kv[:, :, 2].permute(0, 2, 3, 1).reshape(B * heads, 64, T).double()
        assert torch.equal(kp.sum(0)[:, :T], k_ref), (D, T, B)
        assert torch.equal(vp.sum(0)[:, :, vt_positions(Npad)[:T]], v_ref), (D, T, B)
        assert torch.equal(qkv_f[:, :D], qkv_u[:, :D]), (D, T, B)
        assert torch.isfinite(att_f).all() and torch.equal(att_f, att_u), (D, T, B)
        assert rel(qkv_u, linear64(x, w, bias)) < CONV_TOL, (D, T, B)
        e = rel(att_u, attention64(qkv_u, B, T, heads))
        assert e < ATT_TOL, (D, T, B, e)
        worst = max(worst, e)
    note(f"vit_qkv_attention_vs_f64_D{D}", worst)


def test_qkv_attention_refusals():
    lib = _lib.load()
    x, w = torch.zeros(4, 128, device=DEV), torch.zeros(384, 128, device=DEV)
    planes = planes_of(w)
    qkv, att = torch.zeros(4, 384, device=DEV), torch.zeros(4, 128, device=DEV)
    ws = torch.zeros(lib.fs_qkv_attention_workspace_floats(1, 4, 128) + 4, device=DEV)
    s = stream_ptr()
    assert lib.fs_qkv_attention(ptr(x), ptr(w), ptr(planes), None, 1, 4, 128, ptr(qkv), ptr(att), 1, ptr(ws), s) != 0  # 128 % 96
    assert lib.fs_qkv_attention(ptr(x), ptr(w), None, None, 1, 4, 128, ptr(qkv), ptr(att), 0, ptr(ws), s) != 0  # no split planes
    assert lib.fs_qkv_attention(ptr(x), ptr(w), ptr(planes), None, 1, 4, 128, ptr(qkv), ptr(att), 0, ptr(ws[1:]), s) != 0  # unaligned
    check(lib.fs_qkv_attention(ptr(x), ptr(w), ptr(planes), None, 1, 4, 128, ptr(qkv), ptr(att), 0, ptr(ws), s))


# ----------------------------------------------------------------------------------------------------------------------- mask head
def mask_head(pp, cc, gam, bet, B, N, K, D):
    out = torch.full((B, K, N), float("nan"), device=DEV)
    check(_lib.load().fs_mask_head(ptr(pp), ptr(cc), ptr(gam), ptr(bet), ptr(out), B, N, K, D, stream_ptr()))
    return out


@pytest.mark.parametrize("D", [64, 384, 768, 1024])
def test_mask_head_against_float64(D):
    """LayerNorm_K((p / |p|) (c / |c|)^T) for K = 1 (variance 0: exactly beta), 2, 5, 19, 63, 64 (every lane of the wave a class);
    B = 3 with B * N not a multiple of 4 (a partly idle last workgroup).  K = 65 is refused."""
    g = torch.Generator().manual_seed(D)
    B, N = 3, 37
    worst = 0.0
    for K in (1, 2, 5, 19, 63, 64):
        u = torch.randn(D, generator=g)  # a direction every token shares: scores with a non-zero mean
        pp = torch.randn(B, N + K, D, generator=g) + 0.5 * u
        cc = torch.randn(B, N + K, D, generator=g) + 0.5 * u
        gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
        got = mask_head(pp.to(DEV), cc.to(DEV), gam.to(DEV), bet.to(DEV), B, N, K, D)
        if K == 1:
            assert torch.equal(got.cpu(), bet.view(1, 1, 1).expand(B, 1, N)), D
            continue
        p = pp[:, :N].double()
        c = cc[:, N:].double()
        s = (p / p.norm(dim=-1, keepdim=True)) @ (c / c.norm(dim=-1, keepdim=True)).transpose(1, 2)
        e = rel(got, ln64(s, gam, bet).permute(0, 2, 1))
        assert e < MASK_TOL, (D, K, e)
        worst = max(worst, e)
    note(f"vit_mask_head_vs_f64_D{D}", worst)
    z = torch.ones(B * (N + 65) * D, device=DEV)
    assert _lib.load().fs_mask_head(ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), B, N, 65, D, stream_ptr()) != 0


# ----------------------------------------------------------------------------------------------------------------------- patchify / assembly
def ctypes_offset(t, elems):
    return ctypes.c_void_p(t.data_ptr() + 4 * elems)


def patchify_ref(x, P):
    B, C, H, W = x.shape
    gh, gw = -(-H // P), -(-W // P)
    xp = F.pad(x, (0, gw * P - W, 0, gh * P - H))
    return xp.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B * gh * gw, C * P * P)


@pytest.mark.parametrize("P", [4, 8, 16, 32, 6])
def test_patchify_against_unfold(P):
    """F.pad + unfold (columns c, py, px), bit for bit: ragged H x W, B = 3 split over two frame pointers (B1 = 2), all frames behind
    either pointer (B1 = 0 / 3), and an output 4 bytes off 16-B alignment -- which runs the element-wise kernel (as P % 4 != 0 does), and it
    must give what the four-pixel kernel gives."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(P)
    for H, W in ((37, 50), (P, P), (1, 2 * P + 1), (64, 63)):
        x = torch.randn(3, 3, H, W, generator=g)
        ref = patchify_ref(x, P)
        xa, xb = x[:2].contiguous().to(DEV), x[2:].contiguous().to(DEV)
        xall = x.to(DEV)
        for B1, a, b in ((2, xa, xb), (0, None, xall), (3, xall, None)):
            buf = torch.full((ref.numel() + 4,), float("nan"), device=DEV)
            check(lib.fs_patchify(ptr(a), ptr(b), B1, ptr(buf), 3, H, W, P, stream_ptr()))
            assert torch.equal(buf[:ref.numel()].view(ref.shape).cpu(), ref), (P, H, W, B1)
            off = torch.full((ref.numel() + 4,), float("nan"), device=DEV)
            check(lib.fs_patchify(ptr(a), ptr(b), B1, ctypes_offset(off, 1), 3, H, W, P, stream_ptr()))
            assert torch.equal(off[1:ref.numel() + 1].view(ref.shape).cpu(), ref), (P, H, W, B1, "unaligned")
    assert lib.fs_patchify(ptr(xa), None, 2, ptr(buf), 3, 8, 8, P, stream_ptr()) != 0  # images 2.. need in2


@pytest.mark.parametrize("D", [384, 68])
def test_token_assembly_is_cat_plus_add(D):
    """vit_assemble (cls token + patch embeddings + position table) and dec_assemble (patch tokens + class embeddings) equal
    torch.cat and one fp32 add exactly; D % 4 != 0 is refused."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(D)
    B, N, K = 3, 37, 19
    emb, cls, pos = torch.randn(B * N, D, generator=g), torch.randn(D, generator=g), torch.randn(N + 1, D, generator=g)
    X = torch.full((B, N + 1, D), float("nan"), device=DEV)
    ed, cd, pd = emb.to(DEV), cls.to(DEV), pos.to(DEV)  # held: a temporary's memory may be reused before the kernel reads it
    check(lib.fs_vit_assemble(ptr(ed), ptr(cd), ptr(pd), ptr(X), B, N, D, stream_ptr()))
    ref = torch.cat([cls.view(1, 1, D).expand(B, 1, D), emb.view(B, N, D)], 1) + pos
    assert torch.equal(X.cpu(), ref)
    Y, ce = torch.randn(B * N, D, generator=g), torch.randn(K, D, generator=g)
    Z = torch.full((B, N + K, D), float("nan"), device=DEV)
    yd, ced = Y.to(DEV), ce.to(DEV)
    check(lib.fs_dec_assemble(ptr(yd), ptr(ced), ptr(Z), B, N, K, D, stream_ptr()))
    assert torch.equal(Z.cpu(), torch.cat([Y.view(B, N, D), ce.expand(B, K, D)], 1))
    assert lib.fs_vit_assemble(ptr(X), ptr(X), ptr(X), ptr(X), B, N, D - 2, stream_ptr()) != 0
    assert lib.fs_dec_assemble(ptr(Z), ptr(Z), ptr(Z), B, N, K, D - 2, stream_ptr()) != 0


# ----------------------------------------------------------------------------------------------------------------------- seeded sweep
def test_linear_and_layernorm_on_seeded_random_geometries():
    """30 seeded random Linear geometries (rows, K, N, forced split count, route, bias / residual / GELU) and 40 LayerNorm geometries
    (rows, D, drop_first) against float64, as test_gpu_ops.py::test_conv_and_winograd_on_seeded_random_shapes does for the convs."""
    rnd = random.Random(20261016)
    for it in range(30):
        rows = rnd.choice([1, 2, 17, 63, 64, 65, 200, 513])
        K = 32 * rnd.choice([1, 3, 12, 24, 36, 48, 96])
        N = rnd.choice([4, 36, 96, 100, 384, 580, 768, 1024, 1156])
        ns = rnd.choice([1, 1, 2, 3, 4, 5, 6, 8])
        if ns > 1 and K % (32 * ns):
            ns = 1
        act = rnd.choice([0, 0, 2]) if ns == 1 else 0
        split = rnd.random() < 0.6
        g = torch.Generator().manual_seed(1000 + it)
        x = torch.randn(rows, K, generator=g).to(DEV)
        w, bias = weights(g, K, N, rnd.random() < 0.7)
        res = torch.randn(rows, N, generator=g).to(DEV) if rnd.random() < 0.5 else None
        got = linear(x, w, planes_of(w) if split else None, bias, res, act, ns)
        e = rel(got, linear64(x, w, bias, res, act))
        assert e < CONV_TOL, (it, rows, K, N, ns, act, split, e)
    for it in range(40):
        D = 4 * rnd.randint(1, 256)
        B, T = rnd.choice([1, 2, 3]), rnd.randint(1, 90)
        drop = rnd.random() < 0.3
        g = torch.Generator().manual_seed(2000 + it)
        scale = rnd.choice([0.01, 1.0, 30.0])
        x = ((torch.randn(B * T, D, generator=g) + rnd.choice([0.0, 1.0, -3.0])) * scale).to(DEV)
        gam, bet = (torch.rand(D, generator=g) + 0.5).to(DEV), torch.randn(D, generator=g).to(DEV)
        if drop and T > 1:
            got, ref = layernorm(x, gam, bet, T, 1), ln64(x.cpu().view(B, T, D)[:, 1:].reshape(-1, D), gam.cpu(), bet.cpu())
        else:
            got, ref = layernorm(x, gam, bet), ln64(x.cpu(), gam.cpu(), bet.cpu())
        e = rel(got, ref)
        assert e < LN_TOL, (it, B, T, D, drop, e)
