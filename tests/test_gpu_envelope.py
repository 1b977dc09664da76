"""The matrix-core kernels judged element by element (operands and references: tests/envelope_ref.py; what these tests rely on is
proved from the inputs alone in tests/test_envelope_cpu.py).

  family 1  exact sums: operands on a grid on which every partial sum of either arithmetic route is exact in fp32, so the float64 result
            is the only right answer: torch.equal, no tolerance.  A lost or misformed product class of the split route fails here.
  family 2  power-of-two scaling: rows, filters, images and lattice phases scaled by 2^e over about 2^+-60 in ONE launch must give
            ldexp(base launch) bit for bit -- the small rows and channels that a global maximum hides.
  family 3  |got - ref64| <= c 2^-24 D for every element, D = |scale| conv(|x|, |w|) + |shift| + |res| in float64, on operands with a
            2^40 spread between rows and between channels.  c counts the roundings: K + 4 on the fp32-MFMA route (a k-ordered fmaf chain
            of K terms, then the epilogue's multiply, add and residual add, and one to spare for the second-order terms), 6 K + 8 on the
            split route (six exact bf16 products per k, each added in fp32: 6 K; the three dropped products are below 2^-23 |x w| each
            k, 2 x 2^-24 D in all: 2; the epilogue: 3; to first order in 2^-8, the size of m against h).  Loose in K, but asked of
            every element.
The Winograd kernels are in family 2 only: no amplification constant is derived for their transforms."""
import numpy as np
import pytest
from conftest import note
import torch

import envelope_ref as er
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROUTES = ("fp32", "split")
U = 2.0 ** -24


def tiles_of(route):
    return (0, 1, 2, 3, 4, 6) if route == "split" else (0, 1, 2, 3, 4)


def dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def pow2(e):
    """2^e as float32 (|e| <= 126)."""
    return torch.ldexp(torch.ones(np.shape(e)), torch.as_tensor(np.asarray(e)))


def ldexp(t, e):
    """t * 2^e element for element in float32: exact while the result is a normal number."""
    return torch.ldexp(t, torch.as_tensor(np.asarray(e)).expand(t.shape))


def conv(x, w, scale=None, shift=None, res=None, stride=1, pad=0, dil=1, relu=False, tile=0, route="fp32"):
    return ops.conv2d_nhwc(dev(x), dev(w), dev(scale), dev(shift), dev(res), stride, pad, dil, relu, tile, split=route == "split").cpu().contiguous()


def planes_of(w):
    planes = torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=DEV)
    check(_lib.load().fs_split_bf16x3(ptr(w), w.numel(), ptr(planes), stream_ptr()))
    return planes


def linear(x, w, route, bias=None, res=None, act=0, nsplit=1):
    """fs_linear: x [rows][K], w [N][K] -> [rows][N] on the CPU."""
    x, w, bias, res = dev(x), dev(w), dev(bias), dev(res)
    rows, K = x.shape
    N = w.shape[0]
    out = torch.full((rows, N), float("nan"), device=DEV)
    part = torch.full((max(nsplit, 1) * rows * N,), float("nan"), device=DEV) if nsplit != 1 else None
    check(_lib.load().fs_linear(ptr(x), ptr(w), ptr(planes_of(w)) if route == "split" else None, ptr(bias), ptr(res), ptr(out), rows, K, N, act,
                                nsplit, 0, ptr(part), None, None, None, stream_ptr()))
    return out.cpu()


def linear_split_counts(K, N, route):
    """1 (no split-K) and every slice count the network's rule gives this (K, N) over the row counts it meets."""
    lib = _lib.load()
    counts = {1}
    for rows in (1, 33, 135, 197, 577, 1937, 2026, 4052):
        n = lib.fs_linear_splits(K, N, rows, 0, int(route == "split"))
        if n >= 2:
            counts.add(n)
    return sorted(counts)


def dual_conv(a, b, bank, shift, c, relu, tile, route):
    """fs_dual_conv: a [B][Ho][Wo][Cin], b [B][H2][W2][Cin2], bank [Cout][Cin + Cin2] -> [B][Ho][Wo][Cout] on the CPU."""
    a, b, bank, shift = dev(a), dev(b), dev(bank), dev(shift)
    B, Ho, Wo, Cin = a.shape
    out = torch.full((B, Ho, Wo, c["Cout"]), float("nan"), device=DEV)
    check(_lib.load().fs_dual_conv(ptr(a), Cin, ptr(b), c["Cin2"], ptr(bank), ptr(planes_of(bank)) if route == "split" else None, ptr(shift), ptr(out),
                                   c["Cout"], B, Ho, Wo, Cin, c["Cin2"], c["H2"], c["W2"], c["stride2"], c["Cout"], int(relu), tile, stream_ptr()))
    return out.cpu()


def dual_operands(A, c, filler):
    """Rows of A [B * Ho * Wo][Cin + Cin2] as the two maps of fs_dual_conv: a = the first Cin columns; b = the others at the pixels the
    stride keeps, `filler` (values that would wreck the result) at the pixels it skips."""
    st = c["stride2"]
    Ho, Wo = (c["H2"] - 1) // st + 1, (c["W2"] - 1) // st + 1
    A = torch.as_tensor(A).view(c["B"], Ho, Wo, c["Cin"] + c["Cin2"])
    b = torch.full((c["B"], c["H2"], c["W2"], c["Cin2"]), float(filler))
    b[:, ::st, ::st] = A[..., c["Cin"]:]
    return A[..., :c["Cin"]].contiguous(), b


def stem(x, w, scale, shift, route):
    """fs_stem_conv_nchw(_split), 3x3 stride 2 pad 1 (+ ReLU, always): x [B][3][H][W], w OIHW -> NCHW on the CPU."""
    lib = _lib.load()
    x, scale, shift = dev(x), dev(scale), dev(shift)
    wd = dev(w).permute(2, 3, 1, 0).contiguous()
    B, _, H, W = x.shape
    cout = wd.shape[3]
    out = torch.full((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout), float("nan"), device=DEV)
    fn = lib.fs_stem_conv_nchw_split if route == "split" else lib.fs_stem_conv_nchw
    check(fn(ptr(x), ptr(wd), ptr(scale), ptr(shift), ptr(out), B, H, W, cout, 3, 3, 2, 1, stream_ptr()))
    return out.permute(0, 3, 1, 2).cpu().contiguous()


def winograd(x, w, scale, shift, dil, relu, tile_m):
    lib = _lib.load()
    xd, wd, scale, shift = ops.as_nhwc(dev(x)), dev(w), dev(scale), dev(shift)
    b, cin, h, wdt = xd.shape
    cout = wd.shape[0]
    out = torch.full((b, h, wdt, cout), float("nan"), device=DEV)
    ws = torch.empty(lib.fs_winograd_workspace_floats(b, h, wdt, cin, cout, dil, tile_m), device=DEV)
    check(lib.fs_conv3x3_winograd_nhwc(ptr(xd), cin, ptr(wd), ptr(scale), ptr(shift), ptr(out), cout, b, h, wdt, cin, cout, dil, int(relu), tile_m,
                                       ptr(ws), stream_ptr()))
    return out.permute(0, 3, 1, 2).cpu().contiguous()


def winograd_fused(x, w, scale, shift, relu, variant):
    lib = _lib.load()
    xd, wd, scale, shift = ops.as_nhwc(dev(x)), dev(w), dev(scale), dev(shift)
    b, cin, h, wdt = xd.shape
    cout = wd.shape[0]
    out = torch.full((b, h, wdt, cout), float("nan"), device=DEV)
    ws = torch.empty(lib.fs_winograd_fused_workspace_floats(cin, cout), device=DEV)
    check(lib.fs_conv3x3_winograd_fused_nhwc(ptr(xd), cin, ptr(wd), ptr(scale), ptr(shift), ptr(out), cout, b, h, wdt, cin, cout, int(relu), variant,
                                             ptr(ws), stream_ptr()))
    return out.permute(0, 3, 1, 2).cpu().contiguous()


def same_bits(got, want, what):
    """torch.equal with the first differing elements in the message."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:4]]
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first {first}")


# ======================================================================================================== family 1: exact sums
def exact_ref(x, w, stride=1, pad=0, relu=False):
    ref = er.conv64(x, w, stride, pad)
    ref = ref.relu() if relu else ref
    assert torch.equal(ref.float().double(), ref)
    return ref.float()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", er.EXACT_GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", er.KINDS)
def test_exact_conv1x1(kind, shape, route):
    x, w = er.gemm_as_conv(*er.exact_case(kind, *shape, er.SEED))
    for relu in (False, True):
        ref = exact_ref(x, w, relu=relu)
        for tile in tiles_of(route):
            same_bits(conv(x, w, relu=relu, tile=tile, route=route), ref, (kind, shape, route, relu, tile))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", er.KINDS)
def test_exact_conv3x3(kind, route):
    """The exact operands as a 3x3 pad-1 convolution on a 9 x 15 map: taps outside the map drop out of the sums, which stay exact."""
    x, w = er.exact_conv3(kind)
    for relu in (False, True):
        ref = exact_ref(x, w, 1, 1, relu)
        for tile in tiles_of(route):
            same_bits(conv(x, w, pad=1, relu=relu, tile=tile, route=route), ref, (kind, route, relu, tile))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", er.KINDS)
def test_exact_linear_with_every_split_k_count(kind, route):
    """fs_linear at (K, N) = (2304, 96): the partial sums of every slice and their merge are exact under the same condition."""
    rows, K, N = er.EXACT_LINEAR_SHAPE
    A, W = er.exact_case(kind, rows, K, N, er.SEED)
    ref = exact_ref(*er.gemm_as_conv(A, W))[0, :, :, 0].t().contiguous()
    counts = linear_split_counts(K, N, route)
    assert len(counts) >= 2, counts  # the network does split this shape
    for ns in counts:
        same_bits(linear(A, W, route, nsplit=ns), ref, (kind, route, "nsplit", ns))
    same_bits(linear(A, W, route, act=1), ref.relu(), (kind, route, "relu"))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", er.KINDS)
def test_exact_dual_conv(kind, route):
    """conv3 + projection shortcut over the concatenated K, scales of 1: the bank concat_scaled_filters writes is the operands themselves.
    The pixels of the second map that stride 2 skips hold 1e30: read, they would show."""
    c = er.EXACT_DUAL
    A, W = er.exact_dual(kind)
    a, b = dual_operands(A, c, 1e30)
    lib = _lib.load()
    ones, zeros = torch.ones(c["Cout"], device=DEV), torch.zeros(c["Cout"], device=DEV)
    wa, wb = dev(W[:, :c["Cin"]].copy()), dev(W[:, c["Cin"]:].copy())
    bank, shift = torch.empty(c["Cout"], c["Cin"] + c["Cin2"], device=DEV), torch.empty(c["Cout"], device=DEV)
    check(lib.fs_concat_scaled_filters(ptr(wa), ptr(ones), ptr(zeros), c["Cin"], ptr(wb), ptr(ones), ptr(zeros), c["Cin2"], ptr(bank), ptr(shift),
                                       c["Cout"], stream_ptr()))
    assert torch.equal(bank.cpu(), torch.from_numpy(W)) and not shift.any()
    ref = exact_ref(*er.gemm_as_conv(A, W))[0, :, :, 0].t().reshape(c["B"], -1, c["Cout"])
    for relu in (False, True):
        for tile in (0, 1, 2):
            got = dual_conv(a, b, bank, shift, c, relu, tile, route)
            same_bits(got.view(c["B"], -1, c["Cout"]), ref.relu() if relu else ref, (kind, route, relu, tile))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", er.KINDS)
def test_exact_stem(kind, route):
    """The Cin = 3 stem (3x3, stride 2, pad 1, Cout 64, ReLU always) on a 17 x 19 frame: K = 27, every operand dense."""
    x, w = er.exact_stem_case(kind, er.SEED)
    cout = w.shape[0]
    same_bits(stem(x, w, torch.ones(cout), torch.zeros(cout), route), exact_ref(x, w, 2, 1, True), (kind, route))


# ======================================================================================================== family 2: power-of-two scaling
def spans(e):
    """the scaled launch really spans the range: exponents at both ends."""
    return int(np.min(e)) < -20 and int(np.max(e)) > 20


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", er.EXACT_GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scaling_conv1x1(shape, route):
    c = er.scaling_case(*shape, er.SEED)
    rows, K, N = shape
    x, w = er.gemm_as_conv(c["A"], c["W"])
    xs, ws = er.gemm_as_conv(er.scaled(c["A"], c["e"][:, None]), er.scaled(c["W"], c["f"][:, None]))
    E = (c["f"] + c["g"])[None, :, None, None] + c["e"][None, None, :, None]        # [1][N][rows][1]
    assert spans(E)
    r = np.ascontiguousarray(c["R"].T.reshape(1, N, rows, 1))
    rs = er.scaled(r, E)
    one, zero, sg = torch.ones(N), torch.zeros(N), pow2(c["g"])
    for relu, res, res_s in ((False, None, None), (True, r, rs), (False, r, rs)):
        for tile in tiles_of(route):
            base = conv(x, w, one, zero, res, relu=relu, tile=tile, route=route)
            assert (base != 0).float().mean() > (0.3 if relu else 0.9)
            got = conv(xs, ws, sg, zero, res_s, relu=relu, tile=tile, route=route)
            same_bits(got, ldexp(base, E), (shape, route, relu, res is not None, tile))


@pytest.mark.parametrize("route", ROUTES)
def test_scaling_linear_with_every_split_k_count(route):
    rows, K, N = er.EXACT_LINEAR_SHAPE
    c = er.scaling_case(rows, K, N, er.SEED)
    As, Ws = er.scaled(c["A"], c["e"][:, None]), er.scaled(c["W"], c["f"][:, None])
    E = c["e"][:, None] + c["f"][None, :]          # fs_linear has no epilogue scale: the output carries e_i + f_j
    assert spans(E)
    Rs = er.scaled(c["R"], E)
    for ns in linear_split_counts(K, N, route):
        for res, res_s in ((None, None), (c["R"], Rs)):
            base = linear(c["A"], c["W"], route, res=res, nsplit=ns)
            assert (base != 0).float().mean() > 0.9
            same_bits(linear(As, Ws, route, res=res_s, nsplit=ns), ldexp(base, E), (route, ns, res is not None))
    base = linear(c["A"], c["W"], route, res=c["R"], act=1)
    same_bits(linear(As, Ws, route, res=Rs, act=1), ldexp(base, E), (route, "relu"))


def conv_scaling_operands(c):
    """(xs, ws, E_out) of a scaling_conv_case: pixels scaled per image and lattice phase, filters per output channel."""
    xs = er.scaled(c["x"], c["E"][:, None])
    ws = er.scaled(c["w"], c["f"][:, None, None, None])
    E = c["E"][:, None] + (c["f"] + c["g"])[None, :, None, None]
    return xs, ws, E


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dil", er.SCALE_CONV3_DILS)
def test_scaling_conv3x3(dil, route):
    c = er.scaling_conv_case(**er.SCALE_CONV3, dil=dil, seed=er.SEED)
    xs, ws, E = conv_scaling_operands(c)
    assert spans(E)
    rs = er.scaled(c["r"], E)
    cout = c["w"].shape[0]
    one, zero, sg = torch.ones(cout), torch.zeros(cout), pow2(c["g"])
    for relu, res, res_s in ((False, None, None), (True, c["r"], rs)):
        for tile in tiles_of(route):
            base = conv(c["x"], c["w"], one, zero, res, 1, dil, dil, relu, tile, route)
            assert (base != 0).float().mean() > (0.3 if relu else 0.9)
            got = conv(xs, ws, sg, zero, res_s, 1, dil, dil, relu, tile, route)
            same_bits(got, ldexp(base, E), (dil, route, relu, tile))


@pytest.mark.parametrize("route", ROUTES)
def test_scaling_stem(route):
    c = er.scaling_stem_case(er.SEED)
    cout = c["w"].shape[0]
    xs = er.scaled(c["x"], c["ei"][:, None, None, None])
    ws = er.scaled(c["w"], c["f"][:, None, None, None])
    E = c["ei"][:, None, None, None] + (c["f"] + c["g"])[None, :, None, None]
    assert spans(E)
    base = stem(c["x"], c["w"], torch.ones(cout), torch.zeros(cout), route)
    assert (base != 0).float().mean() > 0.3
    same_bits(stem(xs, ws, pow2(c["g"]), torch.zeros(cout), route), ldexp(base, E), route)


@pytest.mark.parametrize("dil", er.SCALE_WINO_DILS)
@pytest.mark.parametrize("tile_m", [3, 4, 6])
def test_scaling_winograd(tile_m, dil):
    """F(m x m, 3x3) with the lattice path at dilation 2 and 12: every transform is linear, so a power of two per image, per lattice
    phase and per output channel passes through it exactly."""
    c = er.scaling_conv_case(**er.SCALE_WINO, dil=dil, seed=er.SEED, lim=er.WINO_LIM)
    xs, ws, E = conv_scaling_operands(c)
    assert int(E.min()) < -12 and int(E.max()) > 12
    cout = c["w"].shape[0]
    for relu in (False, True):
        base = winograd(c["x"], c["w"], torch.ones(cout), torch.zeros(cout), dil, relu, tile_m)
        assert (base != 0).float().mean() > (0.3 if relu else 0.9)
        same_bits(winograd(xs, ws, pow2(c["g"]), torch.zeros(cout), dil, relu, tile_m), ldexp(base, E), (tile_m, dil, relu))


@pytest.mark.parametrize("variant", [0, 2, 3])
def test_scaling_winograd_fused(variant):
    c = er.scaling_conv_case(**er.SCALE_WINO_FUSED, dil=1, seed=er.SEED, lim=er.WINO_LIM)
    xs, ws, E = conv_scaling_operands(c)
    assert int(E.min()) < -12 and int(E.max()) > 12
    cout = c["w"].shape[0]
    for relu in (False, True):
        base = winograd_fused(c["x"], c["w"], torch.ones(cout), torch.zeros(cout), relu, variant)
        assert (base != 0).float().mean() > (0.3 if relu else 0.9)
        same_bits(winograd_fused(xs, ws, pow2(c["g"]), torch.zeros(cout), relu, variant), ldexp(base, E), (variant, relu))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", er.ATTENTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scaling_attention(shape, route):
    """Column d of head h of V scaled by 2^f(h, d): the softmax weights do not change and the output column scales with it (the weighted
    sums and the running rescale are linear in V)."""
    B, N, heads = shape
    c = er.attention_case(*shape)
    D = heads * 64
    scaled = c["qkv"].copy()
    scaled[..., 2 * D:] = er.scaled(scaled[..., 2 * D:], c["f"])
    base = ops.attention(dev(c["qkv"]), heads, split_operands=route == "split").cpu()
    assert (base != 0).float().mean() > 0.9
    got = ops.attention(dev(scaled), heads, split_operands=route == "split").cpu()
    same_bits(got, ldexp(base, c["f"]), (shape, route))


# ======================================================================================================== family 3: per-element bound
def bound_c(route, K):
    return K + 4 if route == "fp32" else 6 * K + 8


def within_bound(got, ref, D, route, K, name):
    """|got - ref| <= c 2^-24 D for every element; the measured maximum of |err| / D goes to parity_measured.txt."""
    assert torch.isfinite(got).all(), name
    ratio = (got.double() - ref).abs() / D
    worst = ratio.max().item()
    print(f"{name}: max |err| / D = {worst:.3e} = {worst / U:.2f} x 2^-24; bound {bound_c(route, K)} x 2^-24")
    bad = (ratio > bound_c(route, K) * U).nonzero()
    assert bad.shape[0] == 0, (name, bad.shape[0], worst / U, bound_c(route, K), bad[:4].tolist())
    return worst


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", er.SCALE_GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bound_conv1x1_and_linear(shape, route):
    rows, K, N = shape
    c = er.bound_gemm_case(rows, K, N, er.SEED)
    x, w = er.gemm_as_conv(c["A"].numpy(), c["W"].numpy())
    res = c["res"].t().reshape(1, N, rows, 1).contiguous()
    D = er.abs_bound(x, w, c["scale"], c["shift"], res)
    assert (D.max() / D.min()).item() > 2.0 ** 40
    worst = 0.0
    for relu in (False, True):
        ref = er.ref64(x, w, c["scale"], c["shift"], res, relu=relu)
        for tile in tiles_of(route):
            got = conv(x, w, c["scale"], c["shift"], res, relu=relu, tile=tile, route=route)
            worst = max(worst, within_bound(got, ref, D, route, K, f"conv1x1 {shape} {route} relu{int(relu)} tile{tile}"))
    note(f"envelope_conv1x1_{route}_{rows}x{K}x{N}_max_err_over_D", worst)
    # fs_linear: bias in place of the shift, no scale; unsplit and with every split-K count of the shape (K / ns-term chains + ns - 1 adds)
    Dl = er.abs_bound(x, w, None, c["shift"], res)[0, :, :, 0].t()
    refl = er.ref64(x, w, None, c["shift"], res)[0, :, :, 0].t()
    worst = 0.0
    for ns in linear_split_counts(K, N, route):
        got = linear(c["A"], c["W"], route, c["shift"], c["res"], nsplit=ns)
        worst = max(worst, within_bound(got, refl, Dl, route, K, f"linear {shape} {route} nsplit{ns}"))
    note(f"envelope_linear_{route}_{rows}x{K}x{N}_max_err_over_D", worst)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dil", er.SCALE_CONV3_DILS)
def test_bound_conv3x3(dil, route):
    g = er.SCALE_CONV3
    c = er.bound_conv_case(g["B"], g["H"], g["Wd"], g["Cin"], g["Cout"], er.SEED + dil)
    K = 9 * g["Cin"]
    D = er.abs_bound(c["x"], c["w"], c["scale"], c["shift"], c["res"], 1, dil, dil)
    assert (D.max() / D.min()).item() > 2.0 ** 40
    worst = 0.0
    for relu in (False, True):
        ref = er.ref64(c["x"], c["w"], c["scale"], c["shift"], c["res"], 1, dil, dil, relu)
        for tile in tiles_of(route):
            got = conv(c["x"], c["w"], c["scale"], c["shift"], c["res"], 1, dil, dil, relu, tile, route)
            worst = max(worst, within_bound(got, ref, D, route, K, f"conv3x3 d{dil} {route} relu{int(relu)} tile{tile}"))
    note(f"envelope_conv3x3_d{dil}_{route}_max_err_over_D", worst)


@pytest.mark.parametrize("route", ROUTES)
def test_bound_dual_conv(route):
    """The bank is concat_scaled_filters' (sa wa | sb wb, one fp32 rounding each) and the reference takes it as given: the bound is about
    the GEMM over the concatenated K and its epilogue (shift = ha + hb, no scale, no residual)."""
    c = er.EXACT_DUAL
    K = c["Cin"] + c["Cin2"]
    b = er.bound_gemm_case(c["B"] * 90, K, c["Cout"], er.SEED + 2)
    A, W = b["A"], b["W"]
    lib = _lib.load()
    wa, wb = dev(W[:, :c["Cin"]].contiguous()), dev(W[:, c["Cin"]:].contiguous())
    sa, sb, ha, hb = dev(b["scale"]), dev(b["scale"].flip(0)), dev(b["shift"]), dev(b["shift"].flip(0) * 0.5)
    bank, shift = torch.empty(c["Cout"], K, device=DEV), torch.empty(c["Cout"], device=DEV)
    check(lib.fs_concat_scaled_filters(ptr(wa), ptr(sa), ptr(ha), c["Cin"], ptr(wb), ptr(sb), ptr(hb), c["Cin2"], ptr(bank), ptr(shift), c["Cout"],
                                       stream_ptr()))
    a_map, b_map = dual_operands(A, c, 1e30)
    x, w = er.gemm_as_conv(A.numpy(), bank.cpu().numpy())
    D = er.abs_bound(x, w, None, shift.cpu())[0, :, :, 0].t()
    assert (D.max() / D.min()).item() > 2.0 ** 40
    worst = 0.0
    for relu in (False, True):
        ref = er.ref64(x, w, None, shift.cpu(), relu=relu)[0, :, :, 0].t()
        for tile in (0, 1, 2):
            got = dual_conv(a_map, b_map, bank, shift, c, relu, tile, route).view(-1, c["Cout"])
            worst = max(worst, within_bound(got, ref, D, route, K, f"dual_conv {route} relu{int(relu)} tile{tile}"))
    note(f"envelope_dual_conv_{route}_max_err_over_D", worst)
