"""The split-operand implicit GEMM's lane maps, on the smallest shapes at which they can go wrong (csrc/conv_igemm.hip, SPLIT = true):
which tile row and which k a lane's operand registers hold, which output element an accumulator register is, in every tile shape.
All data here is exact: small integers (times 2^-4), so every product and every partial sum is an fp32 number whatever the order of
summation, the three-bf16-term split of an operand is lossless, and the result must be BIT-equal to a float64 matmul cast to fp32 --
there is no tolerance to choose.  Outputs are NaN-filled, wider than Cout and longer than M, so a write outside the result shows.
The last test is the only one on random data: all tiles give the same bits, and so do repeated runs."""
import pytest
import torch

from flood_uav_video_segmentation_amd import _lib
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILES = (1, 2, 3, 4, 6)


def tiles_for(cout):
    """Tile 6 is 128 x 96: for column counts that 96 divides (pick_tile's rule)."""
    return [t for t in TILES if t != 6 or cout % 96 == 0]


def planes_of(w):
    planes = torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=DEV)
    check(_lib.load().fs_split_bf16x3(ptr(w), w.numel(), ptr(planes), stream_ptr()))
    return planes


def conv_split(x, w, tile, kh=1, pad=0, res=None, relu=0):
    """x [B, H, W, Cin] and packed filters w [Cout, kh * kh * Cin] (tap-major, as fs_pack_conv_weight lays them out), both on the device ->
    [B * Ho * Wo, Cout] through fs_conv2d_nhwc_split, scale = 1, shift = 0.  The output buffer is NaN-filled, 8 columns wider and 3 rows
    longer than the result."""
    B, H, W, cin = x.shape
    cout = w.shape[0]
    ho, wo = H + 2 * pad - kh + 1, W + 2 * pad - kh + 1
    M, ld = B * ho * wo, cout + 8
    out = torch.full((M + 3, ld), float("nan"), device=DEV)
    one, zero, planes = torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV), planes_of(w)
    check(_lib.load().fs_conv2d_nhwc_split(ptr(x), cin, ptr(planes), ptr(one), ptr(zero), ptr(res), cout, ptr(out), ld, B, H, W, cin, cout, kh, kh,
                                           1, pad, 1, relu, tile, stream_ptr()))
    assert torch.isnan(out[:M, cout:]).all() and torch.isnan(out[M:]).all(), "wrote outside the result"
    return out[:M, :cout]


def small_ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------ 1. row halves
@pytest.mark.parametrize("cout", [32, 96, 160])
@pytest.mark.parametrize("w_px", [1, 15, 16, 17, 31, 33, 129])
def test_rows_straddling_16_32_and_128_are_exact(w_px, cout):
    """1 x 1 conv, one chunk of K, M = w_px rows: every row block of 16 / 32 / 128 half-filled, filled, and one row over."""
    g = torch.Generator().manual_seed(1000 * w_px + cout)
    x, w = small_ints(g, 1, 1, w_px, 32) / 16, small_ints(g, cout, 32) / 16
    ref = (x.view(w_px, 32).double() @ w.double().t()).float()
    for tile in tiles_for(cout):
        got = conv_split(x.to(DEV), w.to(DEV), tile)
        assert torch.equal(got.cpu(), ref), (tile, (got.cpu() != ref).nonzero()[:4].tolist())


# ------------------------------------------------------------------------------------------------ 2. k map
def k_weights(cout, K):
    n, k = torch.arange(cout).view(-1, 1), torch.arange(K).view(1, -1)
    return (1 + n + 37 * k).float()  # < 2^24: exact in fp32 and in three bf16 terms


@pytest.mark.parametrize("K", [32, 64, 96])
def test_every_k_of_a_chunk_meets_its_own_filter_value(K):
    """x[m, k] = (k == k0): output column n is w[n, k0].  Row m looks at chunk m % (K / 32), so every chunk is some row's; one launch per k0
    of a chunk and tile.  A disagreement between the two operands' lane-to-k maps, or a wrong swizzle, is a wrong integer."""
    cout, M, nch = 64, 33, K // 32
    w = k_weights(cout, K)
    wd = w.to(DEV)
    for k0 in range(32):
        hot = 32 * (torch.arange(M) % nch) + k0
        x = torch.zeros(M, K)
        x[torch.arange(M), hot] = 1.0
        ref = w[:, hot].t().contiguous()
        for tile in tiles_for(cout):
            got = conv_split(x.view(1, 1, M, K).to(DEV), wd, tile)
            assert torch.equal(got.cpu(), ref), (K, k0, tile)


def test_every_k_of_a_3x3_chunk_meets_its_own_filter_value():
    """K = 288: a 3 x 3 conv with Cin = 32 and padding 1 on a 5 x 5 map that is zero but for channel c0 of the centre pixel: the output
    pixel at offset (-dy, -dx) from the centre is filter tap (dy, dx), channel c0."""
    cout, cin = 64, 32
    w = k_weights(cout, 9 * cin)
    wd = w.to(DEV)
    for c0 in range(cin):
        x = torch.zeros(1, 5, 5, cin)
        x[0, 2, 2, c0] = 1.0
        ref = torch.zeros(5, 5, cout)
        for r in range(3):
            for s in range(3):
                ref[2 - (r - 1), 2 - (s - 1)] = w[:, (r * 3 + s) * cin + c0]
        for tile in tiles_for(cout):
            got = conv_split(x.to(DEV), wd, tile, kh=3, pad=1)
            assert torch.equal(got.cpu(), ref.view(25, cout)), (c0, tile)


# ------------------------------------------------------------------------------------------------ 3. epilogue
@pytest.mark.parametrize("cout", [96, 160])
def test_residual_and_relu_land_on_their_own_elements(cout):
    """scale = 1, shift = 0, a residual of small integers and ReLU on exact data: relu(x w^T + r) bit for bit."""
    M, K = 131, 64
    g = torch.Generator().manual_seed(cout)
    x, w, r = small_ints(g, 1, 1, M, K) / 16, small_ints(g, cout, K) / 16, small_ints(g, M, cout)
    ref = (x.view(M, K).double() @ w.double().t() + r.double()).clamp_min(0).float()
    for tile in tiles_for(cout):
        got = conv_split(x.to(DEV), w.to(DEV), tile, res=r.to(DEV), relu=1)
        assert torch.equal(got.cpu(), ref), tile


@pytest.mark.parametrize("cout", [64, 160])
def test_concatenated_k_is_exact(cout):
    """The concatenated-K (DUAL) instantiations through fs_dual_conv: relu(a wa^T + b[::2, ::2] wb^T), the second operand a strided 1 x 1
    conv of a 9 x 7 map, on exact data."""
    B, H2, W2, st, cin, cin2 = 3, 9, 7, 2, 32, 64
    ho, wo = (H2 - 1) // st + 1, (W2 - 1) // st + 1
    M = B * ho * wo
    g = torch.Generator().manual_seed(7 + cout)
    a, b = small_ints(g, B, ho, wo, cin) / 16, small_ints(g, B, H2, W2, cin2) / 16
    wa, wb = small_ints(g, cout, cin) / 16, small_ints(g, cout, cin2) / 16
    bank = torch.cat([wa, wb], 1).contiguous().to(DEV)
    ref = (a.double() @ wa.double().t() + b[:, ::st, ::st].double() @ wb.double().t()).clamp_min(0).float().view(M, cout)
    ld = cout + 8
    ad, bd, planes, zero = a.to(DEV), b.to(DEV), planes_of(bank), torch.zeros(cout, device=DEV)
    for tile in (0, 1, 2):
        out = torch.full((M + 3, ld), float("nan"), device=DEV)
        check(_lib.load().fs_dual_conv(ptr(ad), cin, ptr(bd), cin2, ptr(bank), ptr(planes), ptr(zero), ptr(out), ld, B, ho, wo, cin,
                                       cin2, H2, W2, st, cout, 1, tile, stream_ptr()))
        assert torch.isnan(out[:M, cout:]).all() and torch.isnan(out[M:]).all(), "wrote outside the result"
        assert torch.equal(out[:M, :cout].cpu(), ref), tile


# ------------------------------------------------------------------------------------------------ 4. tile identity, repeatability
def test_tiles_and_repeated_runs_give_the_same_bits():
    """Random data, K = 2048 on a 23 x 23 map, 192 columns: an output element's products are summed in the same order whatever tile it falls
    in, and in the same order every time."""
    g = torch.Generator().manual_seed(2048)
    x = torch.randn(1, 23, 23, 2048, generator=g).to(DEV)
    w = (torch.randn(192, 2048, generator=g) * 2048 ** -0.5).to(DEV)
    first = conv_split(x, w, 3).clone()
    ref = (x.view(529, 2048).double() @ w.double().t()).cpu()
    assert ((first.cpu().double() - ref).abs().max() / ref.abs().max()).item() < 2e-5  # CONV_TOL of tests/test_gpu_ops.py: the case is not vacuous
    for tile in TILES:
        for _ in range(3):
            assert torch.equal(conv_split(x, w, tile), first), tile
