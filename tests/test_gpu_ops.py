"""GPU parity of every kernel behind the C ABI against the torch-CPU op it replaces (fp32).
Tolerances are relative to the reference tensor's max |value| and written per test."""
import pytest
from conftest import note
import flow_tail_ref
import torch
import torch.nn.functional as F

from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONV_TOL = 2e-5   # fp32 MFMA fmaf chain vs CPU blocked summation, K up to 4608
INTERP_TOL = 2e-6  # same formulas, un-contracted: a few ulp of the largest value


def rel(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


CONV_CASES = [
    # b, h, w, cin, cout, k, stride, pad, dil, relu, res
    (1, 19, 19, 64, 64, 1, 1, 0, 1, False, False),
    (2, 37, 35, 64, 128, 3, 1, 1, 1, True, False),
    (1, 45, 45, 128, 128, 3, 2, 1, 1, True, False),
    (1, 23, 23, 256, 256, 3, 1, 2, 2, True, True),
    (1, 23, 23, 512, 192, 3, 1, 4, 4, False, True),
    (2, 45, 45, 256, 512, 1, 2, 0, 1, False, False),
    (1, 9, 9, 2048, 96, 3, 1, 12, 12, True, False),   # ASPP-style: dilation larger than the map
    (1, 1, 1, 32, 32, 1, 1, 0, 1, False, False),      # single pixel
    (2, 40, 33, 64, 96, 3, 1, 18, 18, True, False),   # taps outside the map for whole tiles (top / bottom rows)
]


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_igemm(case, tile):
    b, h, w, cin, cout, k, stride, pad, dil, relu, res = case
    g = torch.Generator().manual_seed(h * 1000 + cin + cout + k)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x, wt, None, stride, pad, dil) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    r = torch.randn(ref.shape, generator=g) if res else None
    if res:
        ref = ref + r
    if relu:
        ref = ref.relu()
    got = ops.conv2d_nhwc(x.to(DEV), wt.to(DEV), sc.to(DEV), sh.to(DEV), r.to(DEV) if res else None, stride, pad, dil, relu, tile)
    assert rel(got, ref) < CONV_TOL


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 6])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_igemm_split_operands(case, tile):
    """The split-operand kernel (round 3, the networks' default): every fp32 pixel / filter value as the exact sum of three bf16
    terms, six of the nine cross products on the bf16 matrix cores, fp32 accumulation.  Same cases, same tolerance as the fp32-MFMA
    kernel -- and measured against a float64 convolution of the same fp32 inputs its error is within 1.5x of that kernel's.  Tile 6
    (128 x 96) exists on this route only; every tile shape gives the SAME bits (an output element's products are summed in
    the same order whatever tile it falls in), which is what lets the cost model choose by the batch."""
    b, h, w, cin, cout, k, stride, pad, dil, relu, res = case
    g = torch.Generator().manual_seed(h * 1000 + cin + cout + k)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) * 0.1
    ref64 = F.conv2d(x.double(), wt.double(), None, stride, pad, dil) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    r = torch.randn(ref64.shape, generator=g) if res else None
    if res:
        ref64 = ref64 + r.double()
    if relu:
        ref64 = ref64.relu()
    args = (x.to(DEV), wt.to(DEV), sc.to(DEV), sh.to(DEV), r.to(DEV) if res else None, stride, pad, dil, relu)
    got = ops.conv2d_nhwc(*args, tile, split=True)
    f32 = ops.conv2d_nhwc(*args, tile if tile < 6 else 0)
    if tile:
        assert torch.equal(got, ops.conv2d_nhwc(*args, 3, split=True))
    e_split, e_f32 = rel(got.double(), ref64), rel(f32.double(), ref64)
    note(f"conv_split_vs_f64_tile{tile}_cin{cin}_k{k}", e_split)
    note(f"conv_fp32mfma_vs_f64_tile{tile}_cin{cin}_k{k}", e_f32)
    assert rel(got, ref64.float()) < CONV_TOL
    assert e_split < 1.5 * e_f32 + 1e-7, (e_split, e_f32)


def test_gelu_epilogue_against_float64():
    """relu = 2: nn.GELU (erf form, segm/model/blocks.py:16-28) in the conv epilogue, with the library's own branch-free erf
    (csrc/igemm_epilogue.h::gelu_erf).  An identity 1x1 conv hands the epilogue 400 k values from -12 to 12 (dense around 0 and around
    the |v| / sqrt 2 = 4 clamp); against float64 the error stays within what rounding 0.5 v (1 + erf) to fp32 costs anyway."""
    n, c = 12500, 32
    v = torch.cat([torch.linspace(-12, 12, n * c // 2), torch.linspace(-1e-3, 1e-3, n * c // 4), torch.linspace(5.5, 5.8, n * c // 8),
                   -torch.linspace(5.5, 5.8, n * c // 8)]).view(1, n, 1, c).permute(0, 3, 1, 2).contiguous()
    eye = torch.eye(c).view(c, c, 1, 1)
    ref = 0.5 * v.double() * (1 + torch.erf(v.double() / 2 ** 0.5))
    for split in (False, True):
        got = ops.conv2d_nhwc(v.to(DEV), eye.to(DEV), None, None, None, 1, 0, 1, 2, 0, split=split).cpu().double()
        err = (got - ref).abs()
        bound = 2.5e-7 * v.abs().double().clamp_min(1.0)  # half an ulp of the result + 0.5 |v| x the erf's 1e-7
        assert (err <= bound).all(), (split, float(err.max()), float(v.flatten()[err.argmax()]))
        note(f"gelu_epilogue_max_abs_err_{'split' if split else 'fp32'}", float(err.max()))
    assert torch.equal(ops.conv2d_nhwc(torch.full((1, c, 1, 1), float("nan")).to(DEV), eye.to(DEV), None, None, None, 1, 0, 1, 2).isnan().cpu(),
                       torch.ones(1, c, 1, 1, dtype=torch.bool))


@pytest.mark.parametrize("relu", [False, True])
def test_conv_non_finite_operands(relu):
    """What include/floodseg.h promises about +-inf, NaN and finite values beyond the largest bf16 (3.3895e38) on both arithmetic
    routes.  1x1 conv, so output pixel p depends on input pixel p only: five poisoned pixels, every other pixel must be BIT-equal to
    the clean run.  fp32-MFMA route: IEEE, the torch-CPU convolution's NaN / inf pattern.  Split route: every output a poisoned
    operand contributes to is NaN.  With the fused ReLU (max(v, 0)) a NaN becomes 0 on both routes -- documented, unlike F.relu."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 64, 8, 8, generator=g)
    wt = torch.randn(96, 64, 1, 1, generator=g) * 0.2
    clean = {s: ops.conv2d_nhwc(x.to(DEV), wt.to(DEV), None, None, None, 1, 0, 1, relu, 0, split=s).cpu() for s in (False, True)}
    xp = x.clone()
    poison = {(0, 1): float("inf"), (2, 3): float("-inf"), (4, 4): float("nan"), (6, 0): 3.4e38, (7, 7): -3.4e38}
    for (py, px), v in poison.items():
        xp[0, 5, py, px] = v
    xp[0, 9, 0, 1] = float("-inf")  # +inf and -inf meet in one dot product: NaN under IEEE as well
    ref = F.conv2d(xp, wt)
    if relu:
        ref = ref.relu()
    touched = torch.zeros(8, 8, dtype=torch.bool)
    for (py, px) in poison:
        touched[py, px] = True
    for split in (False, True):
        got = ops.conv2d_nhwc(xp.to(DEV), wt.to(DEV), None, None, None, 1, 0, 1, relu, 0, split=split).cpu()
        assert torch.equal(got[0][:, ~touched], clean[split][0][:, ~touched])  # nothing leaks into the other pixels
        bad = got[0][:, touched]
        rbad = ref[0][:, touched]
        if relu:
            assert ((bad == 0) | ~torch.isfinite(bad) | torch.isfinite(rbad)).all()  # NaN -> 0 through max(v, 0); -inf -> 0; +inf stays
            if not split:
                keep = ~torch.isnan(rbad)
                assert torch.equal(torch.isinf(bad[keep]), torch.isinf(rbad[keep]))
        elif split:
            assert torch.isnan(bad).all()
        else:
            assert torch.equal(torch.isnan(bad), torch.isnan(rbad)) and torch.equal(torch.isinf(bad), torch.isinf(rbad))
            assert torch.equal(bad[torch.isinf(bad)], rbad[torch.isinf(rbad)])  # the same signs
            fin = torch.isfinite(rbad)
            assert ((bad[fin] - rbad[fin]).abs() <= 2e-5 * rbad[fin].abs().max()).all()  # 3.4e38 * w stays finite in fp32


def test_split_bf16x3_is_exact():
    """fs_split_bf16x3: the three bf16 planes add up to the fp32 value bit for bit (any exponent, both signs, zeros)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    w = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-60, 60, (1 << 16,), generator=g).float())
    w[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.38e38, -3.38e38, 2.0 ** -100, -(2.0 ** -100) * 1.9999999])  # |x| <= bf16 max (3.389e38)
    wd = w.to(DEV)
    planes = torch.empty(3 * wd.numel(), dtype=torch.bfloat16, device=DEV)
    check(lib.fs_split_bf16x3(ptr(wd), wd.numel(), ptr(planes), stream_ptr()))
    p = planes.view(3, -1).double()
    back = (p[0] + p[1] + p[2]).float().cpu()
    bad = (back != w).nonzero().flatten()
    assert bad.numel() == 0, (bad[:5], w[bad[:5]], back[bad[:5]])
    assert lib.fs_split_bf16x3(ptr(wd), 12, ptr(planes), stream_ptr()) != 0  # n % 8 != 0 is refused


def _bf16_rne(x):
    """float32 array -> (bf16 bit patterns, the bf16 values as float32): round to nearest even on the uint32 pattern."""
    import numpy as np

    bits = x.view(np.uint32).astype(np.uint64)
    hi = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint32)
    return hi.astype(np.uint16), (hi << 16).view(np.float32)


def _split_planes_host(x):
    """The three planes of csrc/split.h restated in numpy: round, subtract (exact in fp32), round, subtract, round."""
    h, hf = _bf16_rne(x)
    r = x - hf
    m, mf = _bf16_rne(r)
    l, _ = _bf16_rne(r - mf)
    return h, m, l, r


def _split_plane_inputs():
    """+-0, subnormals, ties at the first and at the second level (to even both ways), every exponent that stays finite, and the
    largest magnitudes the split takes (up to the last pattern that still rounds to the largest bf16, 3.3961e38 > 3.39e38)."""
    import numpy as np

    rng = np.random.default_rng(12)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00000100, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,
                        0x00800000, 0x3F800000, 0x3F808000, 0x3F818000, 0x3F804080, 0x3F8040C0, 0x3F80C040,
                        0x7F7F0000, 0xFF7F0000, 0x7F7EFFFF, 0x7F7F7FFF, 0xFF7F7FFF], dtype=np.uint32)
    big = np.array([3.39e38, -3.39e38, 3.38e38, -3.3895e38], dtype=np.float32).view(np.uint32)
    # mantissa = a7 | b8 | c8: b8 c8 = 0x80 0x00 is a tie of the first rounding, a residue whose ninth bit is its last a tie of the second
    a7 = np.array([0x00, 0x01, 0x2A, 0x7E, 0x7F], dtype=np.uint32)
    b8 = np.arange(256, dtype=np.uint32)
    c8 = np.array([0x00, 0x01, 0x20, 0x40, 0x60, 0x80, 0xC0, 0xFF], dtype=np.uint32)
    ex = np.array([0, 1, 2, 17, 100, 126, 127, 128, 200, 253], dtype=np.uint32)  # 0: subnormals; 254 is left to `special` / `big`
    grid = (ex[:, None, None, None] << 23) | (a7[None, :, None, None] << 16) | (b8[None, None, :, None] << 8) | c8[None, None, None, :]
    grid = grid.reshape(-1)
    grid = np.concatenate([grid, grid | np.uint32(0x80000000)])
    rand = rng.integers(0, 0x7F7F0000, 1 << 15, dtype=np.uint32) | (rng.integers(0, 2, 1 << 15, dtype=np.uint32) << 31)
    bits = np.concatenate([special, big, grid, rand])
    bits = np.concatenate([bits, np.zeros(-len(bits) % 8, dtype=np.uint32)])
    return bits.view(np.float32)


def test_split_bf16x3_planes_bit_for_bit():
    """fs_split_bf16x3 pins the PLANES, not only their sum: each of h, m, l is bit-equal to a host restatement of csrc/split.h
    (numpy round-to-nearest-even on the uint32 pattern, three levels).  A changed rounding or residue step in the one definition
    shows here even where h + m + l still adds up.  The generator is checked against itself first: it holds ties of both levels,
    and its planes sum to x exactly wherever the split is exact (2^-110 <= |x|, and zero)."""
    import numpy as np

    x = _split_plane_inputs()
    h, m, l, r = _split_planes_host(x)
    xb, rb = x.view(np.uint32), r.view(np.uint32)
    assert ((xb & 0xFFFF) == 0x8000).sum() >= 100 and (((rb & 0xFFFF) == 0x8000) & ((xb & 0xFFFF) != 0x8000)).sum() >= 100  # ties, levels 0 and 1
    assert ((xb & 0x7F800000) == 0).sum() >= 1000 and np.abs(x).max() > 3.39e38 and np.isfinite(x).all()
    f64 = lambda p: (p.astype(np.uint32) << 16).view(np.float32).astype(np.float64)  # noqa: E731
    exact = (np.abs(x) >= 2.0 ** -110) | (x == 0)
    assert np.array_equal((f64(h) + f64(m) + f64(l))[exact], x.astype(np.float64)[exact])
    lib = _lib.load()
    wd = torch.from_numpy(x.copy()).to(DEV)
    planes = torch.empty(3 * wd.numel(), dtype=torch.bfloat16, device=DEV)
    check(lib.fs_split_bf16x3(ptr(wd), wd.numel(), ptr(planes), stream_ptr()))
    got = planes.view(torch.int16).cpu().numpy().view(np.uint16).reshape(3, -1)
    for name, g, e in (("h", got[0], h), ("m", got[1], m), ("l", got[2], l)):
        bad = np.nonzero(g != e)[0]
        print(f"split plane {name}: {bad.size} of {e.size} differ")
        assert bad.size == 0, (name, [(hex(int(xb[i])), hex(int(g[i])), hex(int(e[i]))) for i in bad[:8]])


def test_conv_and_winograd_on_seeded_random_shapes():
    """30 seeded random geometries (batch, ragged H x W, channel counts that leave partial n-tiles, kernel 1 / 3, stride, dilation,
    residual, activation) through fs_conv2d_nhwc with the cost model's tile, and -- where eligible -- through the Winograd route,
    against F.conv2d: a net for indexing slips that the hand-picked cases above may miss."""
    import random

    rnd = random.Random(20261004)
    lib = _lib.load()
    for it in range(30):
        b = rnd.choice([1, 1, 2, 3])
        h, w = rnd.randint(1, 61), rnd.randint(1, 61)
        cin = 32 * rnd.randint(1, 8)
        cout = rnd.choice([8, 32, 40, 64, 96, 130, 192, 256])
        k = rnd.choice([1, 3])
        dil = rnd.choice([1, 1, 2, 4, 7]) if k == 3 else 1
        stride = rnd.choice([1, 1, 2])
        pad = dil if k == 3 else 0
        relu, res = rnd.random() < 0.5, rnd.random() < 0.4
        g = torch.Generator().manual_seed(it)
        x = torch.randn(b, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        ref = F.conv2d(x, wt, None, stride, pad, dil) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        r = torch.randn(ref.shape, generator=g) if res else None
        if res:
            ref = ref + r
        if relu:
            ref = ref.relu()
        got = ops.conv2d_nhwc(x.to(DEV), wt.to(DEV), sc.to(DEV), sh.to(DEV), r.to(DEV) if res else None, stride, pad, dil, relu, 0)
        assert rel(got, ref) < CONV_TOL, (it, b, h, w, cin, cout, k, stride, dil, relu, res)
        if k == 3 and stride == 1 and not res and cout % 4 == 0:
            for tile_m in (3, 4, 6):
                out = torch.empty((b, h, w, cout), device=DEV)
                ws = torch.empty(lib.fs_winograd_workspace_floats(b, h, w, cin, cout, dil, tile_m), device=DEV)
                xd = ops.as_nhwc(x.to(DEV))
                wd, scd, shd = wt.to(DEV), sc.to(DEV), sh.to(DEV)
                check(lib.fs_conv3x3_winograd_nhwc(ptr(xd), cin, ptr(wd), ptr(scd), ptr(shd), ptr(out), cout, b, h, w, cin, cout, dil, int(relu),
                                                   tile_m, ptr(ws), stream_ptr()))
                assert rel(out.permute(0, 3, 1, 2), ref) < WINO_TOL, (it, tile_m, b, h, w, cin, cout, dil)


@pytest.mark.parametrize("dil", [1, 7, 18, 36])
def test_conv_chunk_major_filters_over_dilations(dil):
    """The layout the network uses for 3x3 convs ([O][I/32][KH][KW][32], tile bit 10) with dilations from 'all taps live' to
    'only the centre tap ever lands inside the map' (ASPP at 90x90 sits in between: whole tap rows are dead per tile)."""
    lib = _lib.load()
    b, h, w, cin, cout = 2, 40, 33, 96, 64
    g = torch.Generator().manual_seed(dil)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    ref = F.conv2d(x, wt, None, 1, dil, dil).relu()
    xd = ops.as_nhwc(x.to(DEV))
    wd = wt.view(cout, cin // 32, 32, 3, 3).permute(0, 1, 3, 4, 2).contiguous().to(DEV)
    out = torch.empty((b, h, w, cout), device=DEV)
    for tile in (0, 1, 3):
        out.fill_(-3.0)
        check(lib.fs_conv2d_nhwc(ptr(xd), cin, ptr(wd), None, None, None, 0, ptr(out), cout, b, h, w, cin, cout, 3, 3, 1, dil, dil, 1,
                                 tile | (1 << 10), stream_ptr()))
        assert rel(out.permute(0, 3, 1, 2), ref) < CONV_TOL


def test_conv_writes_only_its_channel_slice_and_supports_inplace_residual():
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    b, h, w, cin, cout = 1, 30, 30, 96, 160
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    ref = F.conv2d(x, wt, None, 1, 1)
    xd = ops.as_nhwc(x.to(DEV))
    wp = torch.empty((cout, 3, 3, cin), device=DEV)
    check(lib.fs_pack_conv_weight(ptr(wt.to(DEV)), ptr(wp), cout, cin, 3, 3, stream_ptr()))
    big = torch.full((b, h, w, cout + 64), -7.0, device=DEV)
    view = big[..., 32:]
    check(lib.fs_conv2d_nhwc(ptr(xd), cin, ptr(wp), None, None, None, 0, ptr(view), cout + 64, b, h, w, cin, cout, 3, 3, 1, 1, 1, 0, 0, stream_ptr()))
    assert rel(big[..., 32:32 + cout].permute(0, 3, 1, 2), ref) < CONV_TOL
    assert (big[..., :32] == -7.0).all() and (big[..., 32 + cout:] == -7.0).all()
    # residual aliased with the output (how the bottleneck shortcut is accumulated in place)
    acc = torch.randn(b, h, w, cout, generator=g).to(DEV)
    expect = (ref + acc.permute(0, 3, 1, 2).cpu()).relu()
    check(lib.fs_conv2d_nhwc(ptr(xd), cin, ptr(wp), None, None, ptr(acc), cout, ptr(acc), cout, b, h, w, cin, cout, 3, 3, 1, 1, 1, 1, 0, stream_ptr()))
    assert rel(acc.permute(0, 3, 1, 2), expect) < CONV_TOL


def test_conv_rejects_bad_shapes():
    lib = _lib.load()
    x = torch.zeros(1, 8, 8, 48, device=DEV)
    w = torch.zeros(32, 1, 1, 48, device=DEV)
    o = torch.zeros(1, 8, 8, 32, device=DEV)
    rc = lib.fs_conv2d_nhwc(ptr(x), 48, ptr(w), None, None, None, 0, ptr(o), 32, 1, 8, 8, 48, 32, 1, 1, 1, 0, 1, 0, 0, stream_ptr())
    assert rc != 0 and b"multiple of 32" in lib.fs_last_error()


@pytest.mark.parametrize("cout", [64, 128, 96, 16])
@pytest.mark.parametrize("k,stride,pad", [(3, 2, 1), (7, 2, 3), (3, 1, 1)])
def test_stem_conv(k, stride, pad, cout):
    """Cin = 3 stem conv from NCHW: Cout % 32 == 0 (<= 128) runs on the matrix cores (one, two, three or four 32-channel
    sub-tiles; 27 / 147 taps padded to whole batches of 8 MFMA k-steps with zero weights), Cout = 16 keeps the VALU kernel."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(k * 100 + cout)
    x = torch.randn(2, 3, 65, 71, generator=g)
    wt = torch.randn(cout, 3, k, k, generator=g) * 0.2
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    ref = (F.conv2d(x, wt, None, stride, pad) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).relu()
    out = torch.empty((2, ref.shape[2], ref.shape[3], cout), device=DEV)
    xd, wd, scd, shd = x.to(DEV), wt.permute(2, 3, 1, 0).contiguous().to(DEV), sc.to(DEV), sh.to(DEV)
    check(lib.fs_stem_conv_nchw(ptr(xd), ptr(wd), ptr(scd), ptr(shd), ptr(out), 2, 65, 71, cout, k, k, stride, pad, stream_ptr()))
    assert rel(out.permute(0, 3, 1, 2), ref) < CONV_TOL
    if cout % 32 == 0:
        # round 5: the split-operand form (bf16 matrix cores, three bf16 terms per fp32 value): what the networks run.  Same tolerance,
        # and against a float64 convolution of the same fp32 inputs its error is within 1.5x of the fp32-MFMA kernel's
        out3 = torch.empty_like(out)
        check(lib.fs_stem_conv_nchw_split(ptr(xd), ptr(wd), ptr(scd), ptr(shd), ptr(out3), 2, 65, 71, cout, k, k, stride, pad, stream_ptr()))
        assert rel(out3.permute(0, 3, 1, 2), ref) < CONV_TOL
        ref64 = (F.conv2d(x.double(), wt.double(), None, stride, pad) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).relu()
        e3, e1 = rel(out3.permute(0, 3, 1, 2).double(), ref64), rel(out.permute(0, 3, 1, 2).double(), ref64)
        note(f"stem_split_vs_f64_k{k}_s{stride}_c{cout}", e3)
        assert e3 < 1.5 * e1 + 1e-7, (e3, e1)
        again = torch.empty_like(out)
        check(lib.fs_stem_conv_nchw_split(ptr(xd), ptr(wd), ptr(scd), ptr(shd), ptr(again), 2, 65, 71, cout, k, k, stride, pad, stream_ptr()))
        assert torch.equal(again, out3)


def test_maxpool_and_adaptive_avgpool():
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 128, 37, 41, generator=g)
    xd = ops.as_nhwc(x.to(DEV))
    ref = F.max_pool2d(x, 3, 2, 1)
    out = torch.empty((2, ref.shape[2], ref.shape[3], 128), device=DEV)
    check(lib.fs_maxpool3x3s2_nhwc(ptr(xd), ptr(out), 2, 37, 41, 128, stream_ptr()))
    assert torch.equal(out.permute(0, 3, 1, 2).cpu(), ref)  # max is exact
    for (h, w) in ((23, 29), (90, 90)):  # ragged windows and the 713-input geometry
        x = torch.randn(2, 128, h, w, generator=g)
        xd = ops.as_nhwc(x.to(DEV))
        for bin_ in (1, 2, 3, 6):
            out = torch.empty((2, bin_ * bin_, 128), device=DEV)
            check(lib.fs_adaptive_avgpool_nhwc(ptr(xd), 128, ptr(out), 2, h, w, 128, bin_, stream_ptr()))
            assert rel(out.view(2, bin_, bin_, 128).permute(0, 3, 1, 2), F.adaptive_avg_pool2d(x, bin_)) < 5e-6


def test_layout_round_trip():
    lib = _lib.load()
    x = torch.randn(2, 37, 151)
    xd = x.to(DEV)
    out = torch.empty((2, 151, 37), device=DEV)
    check(lib.fs_nchw_to_nhwc(ptr(xd), ptr(out), 2, 37, 151, stream_ptr()))
    assert torch.equal(out.cpu(), x.permute(0, 2, 1))
    back = torch.empty_like(xd)
    check(lib.fs_nhwc_to_nchw(ptr(out), ptr(back), 2, 37, 151, stream_ptr()))
    assert torch.equal(back.cpu(), x)


@pytest.mark.parametrize("ac", [False, True])
def test_grid_sample_and_resize(ac):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 5, 17, 23, generator=g)
    grid = torch.rand(2, 9, 11, 2, generator=g) * 2.6 - 1.3  # out-of-range -> border clamp
    ref = F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=ac)
    assert rel(ops.grid_sample(x.to(DEV), grid.to(DEV), ac), ref) < INTERP_TOL
    assert rel(ops.grid_sample(x.to(DEV), grid.double().to(DEV), ac), ref) < INTERP_TOL  # f64 grids are cast (flow/model.py:246)
    x = torch.randn(1, 128, 19, 21, generator=g)
    grid = torch.rand(1, 7, 9, 2, generator=g) * 2.4 - 1.2
    ref = F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=ac)
    assert rel(ops.grid_sample(ops.as_nhwc(x.to(DEV)), grid.to(DEV), ac), ref) < INTERP_TOL
    x = torch.randn(2, 5, 13, 17, generator=g)
    for size in ((41, 37), (7, 9), (13, 17), (1, 1)):
        ref = F.interpolate(x, size=size, mode="bilinear", align_corners=ac)
        assert rel(ops.resize_bilinear(x.to(DEV), size, ac), ref) < INTERP_TOL
    x = torch.randn(1, 64, 11, 12, generator=g)
    ref = F.interpolate(x, size=(23, 25), mode="bilinear", align_corners=ac)
    assert rel(ops.resize_bilinear(ops.as_nhwc(x.to(DEV)), (23, 25), ac), ref) < INTERP_TOL


def test_blend_is_bit_exact():
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(3, 5, 31, 33, generator=g), torch.randn(3, 5, 31, 33, generator=g)
    for p in range(1, 5):
        wa, wb = (5 - p) / 5, p / 5
        assert torch.equal(ops.blend(a.to(DEV), wa, b.to(DEV), wb).cpu(), wa * a + wb * b)
    assert torch.equal(ops.blend(a.to(DEV), 0.6).cpu(), 0.6 * a)
    odd = torch.randn(1, 1, 3, 7, generator=g)  # numel % 4 != 0 exercises the scalar tail
    assert torch.equal(ops.blend(odd.to(DEV), 0.25, odd.to(DEV), 0.75).cpu(), 0.25 * odd + 0.75 * odd)
    # operands with EQUAL but non-dense strides (two `x[:, :, ::2]` views): both must be densified, not only the first
    big_a, big_b = torch.randn(2, 5, 16, 9, generator=g).to(DEV), torch.randn(2, 5, 16, 9, generator=g).to(DEV)
    va, vb = big_a[:, :, ::2], big_b[:, :, ::2]
    assert va.stride() == vb.stride() and not va.is_contiguous()
    assert torch.equal(ops.blend(va, 0.4, vb, 0.6).cpu(), (0.4 * va + 0.6 * vb).cpu())
    # channels_last `a` with a contiguous `b`: one common layout, values unchanged
    ca = torch.randn(1, 64, 6, 7, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    cb = torch.randn(1, 64, 6, 7, generator=g).to(DEV)
    assert torch.equal(ops.blend(ca, 0.4, cb, 0.6).cpu(), (0.4 * ca + 0.6 * cb).cpu())
    with pytest.raises(RuntimeError, match="shapes differ"):
        ops.blend(ca, 0.5, cb[:, :32], 0.5)
    # out=: results written straight into one image slot of a preallocated batch (what predict_feature / warp_batch do)
    batch = ops.empty_nhwc(3, 64, 6, 7, DEV)
    got = ops.blend(ca, 0.4, cb, 0.6, out=batch[1:2])
    assert got.data_ptr() == batch[1:2].data_ptr() and torch.equal(batch[1:2], ops.blend(ca, 0.4, cb, 0.6))
    up = ops.resize_bilinear(ca, (6, 7), out=batch[2:3])
    assert up.data_ptr() == batch[2:3].data_ptr() and torch.equal(batch[2:3], ca)  # identity resize
    with pytest.raises(RuntimeError, match="out must be"):
        ops.blend(ca, 0.4, cb, 0.6, out=torch.empty(1, 64, 6, 7, device=DEV))      # contiguous slot for a channels_last result
    with pytest.raises(RuntimeError, match="out must be"):
        ops.blend(big_a, 1.0, out=torch.empty(2, 5, 16, 8, device=DEV))            # wrong shape


def _feature_tail_op_by_op(f, f_next, mvl, mvr, n, no_warp, g0):
    """predict_feature's tail as the reference issues it (flow/model.py:131-171), one HIP op per torch op."""
    fh, fw = f.shape[2:]
    fit = lambda t: t if t.shape[2:] == (fh, fw) else ops.resize_bilinear(t, (fh, fw), align_corners=True)  # noqa: E731
    fwd, bwd = [], []
    if f_next is not None and not no_warp:
        cur = f
        for m in mvl:
            cur = ops.grid_sample(cur, m, align_corners=False)
            fwd.append(fit(cur))
        cur = f_next
        for m in mvr:
            cur = ops.grid_sample(cur, m, align_corners=False)
            bwd.append(fit(cur))
    maps = [fit(ops.grid_sample(f, g0, align_corners=True)) if not no_warp else ops.blend(f, 1.0)]
    if f_next is not None:
        for p in range(1, n):
            maps.append(ops.blend(f, (n - p) / n, f_next, p / n) if no_warp else ops.blend(fwd[p - 1], (n - p) / n, bwd[n - p - 1], p / n))
    return torch.cat(maps, 0)


@pytest.mark.parametrize("case", [
    # C, fh, fw, Hg, Wg, H0, W0, n
    (64, 17, 13, 8, 6, 9, 15, 5),     # everything resized, odd sizes
    (96, 12, 12, 12, 12, 7, 9, 3),    # grids already at the feature size: the chain maps are used as they are (flow/model.py:138)
    (128, 9, 11, 5, 4, 9, 11, 4),     # default grid at the feature size: no resize of the key-frame map (:158)
    (68, 6, 5, 3, 3, 4, 4, 2),        # n = 2: one map between the keys, C not a multiple of 64
    (384, 45, 45, 44, 44, 67, 120, 5),   # the Segmenter's token map at 713^2 (configs[3])
])
@pytest.mark.parametrize("no_warp", [False, True])
@pytest.mark.parametrize("single", [False, True])
def test_feat_tail_is_bit_identical_to_the_op_by_op_route(case, no_warp, single):
    """fs_feat_tail (the fused predict_feature tail) against grid_sample -> resize -> blend per map: same bits, including grid
    coordinates outside [-1, 1] (border clamp)."""
    C, fh, fw, Hg, Wg, H0, W0, n = case
    g = torch.Generator().manual_seed(C + fh + n)
    f = (torch.randn(1, C, fh, fw, generator=g) * 3).to(DEV).contiguous(memory_format=torch.channels_last)
    f_next = None if single else (torch.randn(1, C, fh, fw, generator=g) * 3).to(DEV).contiguous(memory_format=torch.channels_last)
    mk = lambda: (torch.rand(1, Hg, Wg, 2, generator=g) * 2.6 - 1.3).to(DEV)  # noqa: E731
    mvl, mvr = [mk() for _ in range(n - 1)], [mk() for _ in range(n - 1)]
    g0 = (torch.rand(1, H0, W0, 2, generator=g) * 2.2 - 1.1).to(DEV)
    got = ops.feat_tail(f, f_next, mvl, mvr, n, no_warp, None if no_warp else g0)
    want = _feature_tail_op_by_op(f, f_next, mvl, mvr, n, no_warp, g0)
    assert got.shape == want.shape == (1 if single else n, C, fh, fw) and ops.is_channels_last_dense(got)
    assert torch.equal(got, want)
    if not no_warp and not single:  # and against torch's own ops on the CPU (same formulas, un-contracted)
        fc, nc = f.cpu(), f_next.cpu()
        up = lambda t: t if t.shape[2:] == (fh, fw) else F.interpolate(t, (fh, fw), mode="bilinear", align_corners=True)  # noqa: E731
        cur, ref_f = fc, []
        for m in mvl:
            cur = F.grid_sample(cur, m.cpu(), mode="bilinear", padding_mode="border", align_corners=False)
            ref_f.append(up(cur))
        cur, ref_b = nc, []
        for m in mvr:
            cur = F.grid_sample(cur, m.cpu(), mode="bilinear", padding_mode="border", align_corners=False)
            ref_b.append(up(cur))
        ref = [up(F.grid_sample(fc, g0.cpu(), mode="bilinear", padding_mode="border", align_corners=True))]
        ref += [(n - p) / n * ref_f[p - 1] + p / n * ref_b[n - p - 1] for p in range(1, n)]
        assert rel(got, torch.cat(ref, 0)) < INTERP_TOL


def test_feat_tail_on_seeded_random_geometries():
    """40 seeded random geometries through fs_feat_tail against the op-by-op route, bit for bit: grids larger AND smaller than the map
    (the run loop's down-sampling branch reloads both register sets), 1-pixel maps and grids, channel counts that leave the last XCD's
    slab short or empty, n = 1 (no chain at all) .. 7."""
    import random
    rnd = random.Random(606)
    for it in range(40):
        C = 4 * rnd.choice([16, 17, 24, 31, 32, 33, 64, 96, 130])
        fh, fw = rnd.choice([(1, 1), (1, 9), (7, 1), (5, 6), (13, 11), (23, 31)])
        Hg, Wg = rnd.choice([(1, 1), (2, 3), (fh, fw), (2 * fh + 1, 3 * fw), (9, 4)])
        H0, W0 = rnd.choice([(1, 1), (fh, fw), (3, 5), (11, 17)])
        n = rnd.choice([1, 2, 3, 5, 7])
        no_warp, single = rnd.random() < 0.25, rnd.random() < 0.2
        g = torch.Generator().manual_seed(1000 + it)
        f = (torch.randn(1, C, fh, fw, generator=g) * 2).to(DEV).contiguous(memory_format=torch.channels_last)
        f_next = None if single else (torch.randn(1, C, fh, fw, generator=g) * 2).to(DEV).contiguous(memory_format=torch.channels_last)
        mk = lambda: (torch.rand(1, Hg, Wg, 2, generator=g) * 2.4 - 1.2).to(DEV)  # noqa: E731
        mvl, mvr = [mk() for _ in range(n - 1)], [mk() for _ in range(n - 1)]
        g0 = (torch.rand(1, H0, W0, 2, generator=g) * 2.4 - 1.2).to(DEV)
        got = ops.feat_tail(f, f_next, mvl, mvr, n, no_warp, None if no_warp else g0)
        want = _feature_tail_op_by_op(f, f_next, mvl, mvr, n, no_warp, g0)
        assert torch.equal(got, want), (it, C, fh, fw, Hg, Wg, H0, W0, n, no_warp, single)


def test_feat_tail_refuses_what_it_cannot_address():
    f = torch.randn(1, 64, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last)
    g = [torch.zeros(1, 4, 4, 2, device=DEV)]
    with pytest.raises(RuntimeError, match="channels_last"):
        ops.feat_tail(torch.randn(1, 64, 8, 8, device=DEV), None, [], [], 1, True)          # NCHW storage
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.feat_tail(torch.randn(1, 6, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last), None, [], [], 1, True)
    with pytest.raises(RuntimeError, match="default grid"):
        ops.feat_tail(f, f, g, g, 2, False, None)
    with pytest.raises(RuntimeError, match="n-1 grids"):
        ops.feat_tail(f, f, g, g, 3, False, torch.zeros(1, 3, 3, 2, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.feat_tail(f.cpu(), None, [], [], 1, True)


def test_argmax_resize_argmax_and_iou_hist():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 5, 40, 44, generator=g)
    x[0, :, 0, 0] = 1.0  # tie -> first index wins (tensor.max(1)[1])
    assert torch.equal(ops.argmax_u8(x.to(DEV)).cpu(), x.max(1)[1].to(torch.uint8))
    ref = F.interpolate(x, size=(67, 120), mode="bilinear", align_corners=True).max(1)[1].to(torch.uint8)
    got = ops.resize_argmax_u8(x.to(DEV), (67, 120)).cpu()
    assert (got == ref).float().mean() > 0.9995
    # and no pixel differs from the float64 argmax where that one is decided (top-2 gap > 1e-4 max|ref|): an agreement share alone
    # cannot tell a tie broken the other way from a wrong pixel in an edge column
    r64, arg64 = flow_tail_ref.resize_argmax_ref(x, (67, 120))
    ok = flow_tail_ref.decided(r64, 1e-4 * r64.abs().max().item())
    assert ok.float().mean() >= 0.99 and torch.equal(got.long()[ok], arg64[ok])
    p = torch.randint(0, 5, (3, 50, 60), generator=g, dtype=torch.uint8)
    t = torch.randint(0, 5, (3, 50, 60), generator=g, dtype=torch.uint8)
    t[0, :5] = 255
    hist = ops.iou_hist(p.to(DEV), t.to(DEV), 5).cpu()
    pm = p.clone()
    pm[t == 255] = 255
    for k in range(5):
        assert hist[0, k] == ((pm == k) & (t == k)).sum()
        assert hist[1, k] == (pm == k).sum()
        assert hist[2, k] == (t == k).sum()


@pytest.mark.parametrize("geom", [
    # b, k, hi, wi, full, keep, align_corners
    (5, 5, 45, 45, (720, 720), (713, 713), False),   # configs[3]: the Segmenter's 16x upsample of a 713 frame padded to 720
    (2, 5, 44, 44, (704, 704), (704, 704), False),   # nothing to crop
    (1, 7, 9, 13, (36, 52), (33, 41), True),
    (3, 1, 5, 4, (17, 9), (1, 1), False),            # K = 1: the mask is all zeros
])
def test_resize_crop_is_the_resize_then_the_crop_then_the_argmax(geom):
    """fs_resize_crop: upsample at the padded size's scale, only the kept pixels, dense -- bit-identical to resize_bilinear at the
    full size, cropped, and to argmax_u8 of that; each output alone equals the pair."""
    b, k, hi, wi, full, keep, ac = geom
    x = torch.randn(b, k, hi, wi, generator=torch.Generator().manual_seed(5)).to(DEV)
    x[0, :, 0, 0] = 0.25  # a tie: the first class wins
    two_steps = ops.resize_bilinear(x, full, align_corners=ac)[:, :, :keep[0], :keep[1]].contiguous()
    logits, mask = ops.resize_crop(x, full, keep, align_corners=ac, want_logits=True, want_mask=True)
    assert logits.is_contiguous() and torch.equal(logits, two_steps)
    assert torch.equal(mask, ops.argmax_u8(two_steps)) and mask[0, 0, 0] == 0
    assert torch.equal(ops.resize_crop(x, full, keep, align_corners=ac)[0], two_steps)
    only_mask = ops.resize_crop(x, full, keep, align_corners=ac, want_logits=False, want_mask=True)
    assert only_mask[0] is None and torch.equal(only_mask[1], mask)
    ref = F.interpolate(x.cpu(), size=full, mode="bilinear", align_corners=ac)[:, :, :keep[0], :keep[1]]
    assert (logits.cpu() - ref).abs().max() < 1e-5


def test_resize_crop_refuses_a_region_outside_the_frame_and_an_empty_request():
    x = torch.randn(1, 5, 8, 8).to(DEV)
    with pytest.raises(RuntimeError, match="not inside"):
        ops.resize_crop(x, (32, 32), (33, 32))
    with pytest.raises(RuntimeError, match="no output"):
        ops.resize_crop(x, (32, 32), (32, 32), want_logits=False, want_mask=False)
    assert ops.resize_crop(x[:0], (32, 32), (30, 30), want_mask=True)[1].shape == (0, 30, 30)


WINO_TOL = 5e-5  # F(4x4,3x3) in fp32: ~7e-6 relative on unit-scale data, F(6x6,3x3) ~1.5x that; the tolerance leaves room for K = 1024
# The error grows ~sqrt(Cin).  Cin = 2048 with F(6,3) measures 6.7e-5 on a single conv (round 2, gpurun_out/r02_pytest_gpu_1.txt) --
# and F(6,3) IS what the network runs for the 2048-channel PSPNet head at 713x713 (90x90 = exactly 15x15 tiles of 6x6), so
# this is the shipped per-conv error of that layer (the "head geometry" case below pins it); end to end the 713^2 logits are within
# 8e-6 of the reference.  Asserted: ~2x the measured value, far inside SURVEY 8(d)'s 1e-3.
WINO_TOL_2048 = 1.5e-4


@pytest.mark.parametrize("case", [
    # b, h, w, cin, cout, dil, relu
    (1, 16, 16, 256, 64, 1, True),
    (2, 23, 29, 256, 96, 1, False),     # ragged: not a multiple of the 4x4 output tile
    (1, 45, 45, 256, 128, 2, True),     # dilation 2 -> 4 lattice phases of 23/22 rows
    (1, 31, 27, 512, 64, 4, True),      # dilation 4 -> 16 phases, some with a single tile row
    (1, 9, 9, 1024, 32, 1, False),
    (1, 3, 5, 256, 32, 4, False),       # image smaller than the dilation lattice step
    (1, 45, 40, 256, 64, 12, True),     # ASPP-style dilations: 144 lattice phases of 4x4 / 3x4 pixels
    (2, 30, 30, 256, 32, 24, False),    # 576 phases, most of them 1x1 or 2x2 pixels
    (1, 90, 90, 2048, 256, 12, True),   # DeepLabv3 ASPP at 713x713 (BASELINE configs[2]): 144 phases of 8x8 / 7x7 pixels,
    (1, 90, 90, 2048, 256, 24, True),   #   576 phases of 4x4 / 3x3,
    (1, 90, 90, 2048, 256, 36, True),   #   1296 phases of 3x3 / 2x2 -- all three take the lattice path in the network
    (2, 90, 90, 2048, 512, 1, True),    # THE PSPNet head conv of a 713x713 window (decoder.0 over the backbone channels, B = 2): with
                                        #   tile_m = 0 the library picks F(6,3) here, as the network does
])
@pytest.mark.parametrize("tile_m", [3, 4, 6, 0])
def test_winograd_conv3x3(case, tile_m):
    """F(3x3,3x3) / F(4x4,3x3) / F(6x6,3x3): input/filter/output transforms + 25 / 36 / 64 grouped MFMA GEMMs vs torch conv2d (direct)
    on ragged maps, batch > 1, dilation lattices; tile_m = 0 lets the library take the cheapest tiling for the map (F(3,3) for the
    dilation-36 ASPP case: its lattices are 3 x 3 pixels, one tile each)."""
    lib = _lib.load()
    b, h, w, cin, cout, dil, relu = case
    g = torch.Generator().manual_seed(h * 100 + cin + dil)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x, wt, None, 1, dil, dil) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    if relu:
        ref = ref.relu()
    xd = ops.as_nhwc(x.to(DEV))
    out = torch.full((b, h, w, cout + 32), -7.0, device=DEV)  # written as a channel slice of a wider buffer
    ws = torch.empty(lib.fs_winograd_workspace_floats(b, h, w, cin, cout, dil, tile_m), device=DEV)
    wd, scd, shd = wt.to(DEV), sc.to(DEV), sh.to(DEV)
    view = out[..., 16:]
    check(lib.fs_conv3x3_winograd_nhwc(ptr(xd), cin, ptr(wd), ptr(scd), ptr(shd), ptr(view), cout + 32, b, h, w, cin, cout, dil, int(relu),
                                       tile_m, ptr(ws), stream_ptr()))
    assert note(f"winograd_op_{h}x{w}x{cin}_d{dil}_m{tile_m}", rel(out[..., 16:16 + cout].permute(0, 3, 1, 2), ref)) < (WINO_TOL if cin <= 1024 else WINO_TOL_2048)
    assert (out[..., :16] == -7.0).all() and (out[..., 16 + cout:] == -7.0).all()


WINO_FUSED_TOL = 3e-5  # F(4x4,3x3) in fp32 at Cin <= 256: measured <= 1e-5 (gpurun_out/parity_measured.txt)


@pytest.mark.parametrize("case", [
    # b, h, w, cin, cout, relu
    (1, 16, 16, 64, 64, True),
    (2, 23, 29, 64, 128, False),     # ragged: last tile row / column partly outside the map
    (1, 5, 3, 32, 64, True),         # smaller than two tiles
    (2, 45, 45, 128, 128, True),     # layer2 conv2 geometry at 353^2
    (1, 9, 9, 256, 64, False),
    (1, 179, 179, 64, 64, True),     # layer1 conv2 of a 713x713 frame
    (1, 357, 357, 64, 128, True),    # the deep stem's layer0.6 of a 713x713 frame
    (1, 20, 20, 96, 64, False),      # six K stages (not a power of two)
    (2, 70, 66, 32, 192, True),      # three channel blocks: the persistent form's grid must stay a multiple of 3 (630 blocks on 255 workgroups)
])
@pytest.mark.parametrize("variant", [0, 2, 3])
def test_winograd_fused_conv3x3(case, variant):
    """The one-kernel Winograd F(4x4,3x3) (wino_fused.hip: transforms and the 36 position GEMMs fused, nothing but the input and
    output maps in HBM) vs torch conv2d + scale/shift (+ReLU): both workgroup shapes, ragged maps, a channel slice of a wider
    output buffer, batch > 1; and bit-repeatable from run to run."""
    lib = _lib.load()
    b, h, w, cin, cout, relu = case
    g = torch.Generator().manual_seed(h * 100 + cin + cout)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x, wt, None, 1, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    if relu:
        ref = ref.relu()
    xd = ops.as_nhwc(x.to(DEV))
    ws = torch.empty(lib.fs_winograd_fused_workspace_floats(cin, cout), device=DEV)
    wd, scd, shd = wt.to(DEV), sc.to(DEV), sh.to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((b, h, w, cout + 32), -7.0, device=DEV)
        view = out[..., 16:]
        check(lib.fs_conv3x3_winograd_fused_nhwc(ptr(xd), cin, ptr(wd), ptr(scd), ptr(shd), ptr(view), cout + 32, b, h, w, cin, cout, int(relu),
                                                 variant, ptr(ws), stream_ptr()))
        outs.append(out)
    out = outs[0]
    assert note(f"winograd_fused_{h}x{w}x{cin}x{cout}_v{variant}", rel(out[..., 16:16 + cout].permute(0, 3, 1, 2), ref)) < WINO_FUSED_TOL
    assert (out[..., :16] == -7.0).all() and (out[..., 16 + cout:] == -7.0).all()
    assert torch.equal(outs[0], outs[1])
    if variant:  # every workgroup shape forms the same products in the same order: bit-identical (the network picks by batch size)
        base = torch.full((b, h, w, cout + 32), -7.0, device=DEV)
        check(lib.fs_conv3x3_winograd_fused_nhwc(ptr(xd), cin, ptr(wd), ptr(scd), ptr(shd), ptr(base[..., 16:]), cout + 32, b, h, w, cin, cout,
                                                 int(relu), 2 if variant != 2 else 3, ptr(ws), stream_ptr()))
        assert torch.equal(base, out)


@pytest.mark.parametrize("case", [
    # b, h, w, cin, cout
    (2, 357, 357, 64, 128),   # the deep stem's layer0.6 + max-pool of a 713x713 key-frame pair
    (1, 16, 16, 64, 64),      # exactly one 4 x 4 block of tiles
    (2, 23, 29, 64, 128),     # ragged: blocks, tiles and pooling windows cut by the map's edge; odd sizes
    (1, 5, 3, 32, 64),
    (3, 70, 66, 32, 192),     # even sizes (the last pooling window has no right / bottom neighbour), three channel blocks
    (1, 33, 17, 128, 64),
])
def test_winograd_fused_conv3x3_with_maxpool_is_bit_identical_to_conv_then_pool(case):
    """Round 5: conv3x3 + BatchNorm + ReLU + MaxPool2d(3, 2, 1) in ONE kernel (the one-kernel Winograd with the pooling in its epilogue:
    inner cells of every 16 x 16 block as plain stores, rim cells as integer atomic maxima against a zeroed map).  A maximum is exact
    and order-independent: the pooled map must equal fs_conv3x3_winograd_fused_nhwc -> fs_maxpool3x3s2_nhwc BIT for bit, run after run;
    and torch's max_pool2d of the torch convolution within the Winograd tolerance."""
    lib = _lib.load()
    b, h, w, cin, cout = case
    g = torch.Generator().manual_seed(h * 100 + cin + cout + 1)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1 - 0.2
    ref = F.max_pool2d((F.conv2d(x, wt, None, 1, 1, 1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).relu(), 3, 2, 1)
    hp, wp = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert ref.shape == (b, cout, hp, wp)
    xd = ops.as_nhwc(x.to(DEV))
    ws = torch.empty(lib.fs_winograd_fused_workspace_floats(cin, cout), device=DEV)
    wd, scd, shd = wt.to(DEV), sc.to(DEV), sh.to(DEV)
    full = torch.empty((b, h, w, cout), device=DEV)
    check(lib.fs_conv3x3_winograd_fused_nhwc(ptr(xd), cin, ptr(wd), ptr(scd), ptr(shd), ptr(full), cout, b, h, w, cin, cout, 1, 2, ptr(ws), stream_ptr()))
    two = torch.empty((b, hp, wp, cout), device=DEV)
    check(lib.fs_maxpool3x3s2_nhwc(ptr(full), ptr(two), b, h, w, cout, stream_ptr()))
    for _ in range(3):
        one = torch.full((b, hp, wp, cout), float("nan"), device=DEV)  # the launcher zeroes the map itself
        check(lib.fs_conv3x3_winograd_fused_pool_nhwc(ptr(xd), cin, ptr(wd), ptr(scd), ptr(shd), ptr(one), b, h, w, cin, cout, ptr(ws), stream_ptr()))
        assert torch.equal(one, two)
    assert note(f"winograd_fused_pool_{h}x{w}x{cin}x{cout}", rel(one.permute(0, 3, 1, 2), ref)) < WINO_FUSED_TOL


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("shape", [
    # b, h, w, cin, cout, k, pad, res  -- the layer shapes of a 713x713 window, where every CU holds 2-5 workgroups at once
    (2, 90, 90, 2048, 512, 1, 0, False),
    (2, 90, 90, 512, 2048, 1, 0, True),
    (2, 90, 90, 256, 1024, 1, 0, True),
    (2, 179, 179, 64, 64, 3, 1, False),
])
def test_conv_at_network_size_is_exact_and_repeatable(shape, tile):
    """Full-occupancy launches: results must match torch AND be bit-identical from run to run (a wave's direct-to-LDS
    loads racing its neighbours' fragment reads showed up exactly here, as run-to-run differences)."""
    b, h, w, cin, cout, k, pad, res = shape
    g = torch.Generator().manual_seed(cin + cout + tile)
    x = torch.randn(b, cin, h, w, generator=g).to(DEV)
    wt = (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5).to(DEV)
    sc, sh = (torch.rand(cout, generator=g) + 0.5).to(DEV), (torch.randn(cout, generator=g) * 0.1).to(DEV)
    r = torch.randn(b, cout, h, w, generator=g).to(DEV) if res else None
    ref = F.conv2d(x.double(), wt.double(), None, 1, pad, 1) * sc.view(1, -1, 1, 1).double() + sh.view(1, -1, 1, 1).double()
    if res:
        ref = ref + r.double()
    ref = ref.relu()
    outs = [ops.conv2d_nhwc(x, wt, sc, sh, r, 1, pad, 1, True, tile) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    assert ((outs[0].double() - ref).abs().max() / ref.abs().max()).item() < CONV_TOL


@pytest.mark.parametrize("shape", [(2, 2026, 6), (1, 1937, 6), (3, 77, 2), (1, 1, 1), (2, 130, 12), (1, 530, 12), (1, 33, 3)])
def test_attention_both_routes_against_float64(shape):
    """fs_attention: softmax(q k^T / 8) v per head, head_dim 64, on the fp32 matrix cores and on the split-operand route (three bf16
    terms per value of q, k, v and of the probabilities).  Token counts that are not multiples of 32 / 64 / 128 exercise the key
    masking and the zero-padded K / V^T planes; 2026 and 1937 are the S/16 counts at 713 / 704 (key split + merge)."""
    b, n, heads = shape
    g = torch.Generator().manual_seed(n * 7 + heads)
    qkv = torch.randn(b, n, 3 * heads * 64, generator=g) * 1.5
    q, k, v = [t.view(b, n, heads, 64).permute(0, 2, 1, 3).double() for t in qkv.split(heads * 64, dim=2)]
    ref = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).permute(0, 2, 1, 3).reshape(b, n, heads * 64)
    e = {}
    for split in (False, True):
        got = ops.attention(qkv.to(DEV), heads, split_operands=split)
        e[split] = note(f"attention_{'split' if split else 'fp32'}_{b}x{n}x{heads}", rel(got.double(), ref))
        assert e[split] < 2e-5, (split, e[split])
        assert torch.equal(got, ops.attention(qkv.to(DEV), heads, split_operands=split))  # and repeatable bit for bit
    assert e[True] < 2.0 * e[False] + 2e-7, e  # the split route is as accurate as the fp32-MFMA one
