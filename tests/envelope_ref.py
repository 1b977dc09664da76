"""Operands and float64 references for the per-element tests of the matrix-core kernels (tests/test_envelope_cpu.py proves what is
claimed here from the inputs alone, tests/test_gpu_envelope.py runs the kernels on them).  numpy / torch on the CPU, nothing of the
library.

Three families of inputs:

  exact cases    operands whose every product -- of the fp32 values and of their bf16 terms -- is a multiple of one grid q, with
                 sum_k |a_k| |w_k| < 2^24 q for every output.  Then every partial sum, in any order, on the fp32-MFMA route (a k-ordered
                 fmaf chain) and on the split-operand route (six bf16 term products per k, fp32 accumulation), is a multiple of q below
                 2^24 q, i.e. exact in fp32: the float64 result is the ONLY correct answer, bit for bit.  The terms dropped by the split
                 route (m l', l m', l l': csrc/split.h) are zero by construction: an operand has an l term only where the other
                 operand has nothing below h.
  scaling cases  base operands with |v| in {0} U [2^-10, 8) and integer exponent vectors.  Multiplying a row / a filter / an image by a
                 power of two multiplies every term, product and partial sum by it exactly as long as nothing overflows or goes
                 subnormal, so the scaled launch must equal ldexp(base launch) element for element.
  bound cases    randn operands with per-row / per-channel factors 2^u, for the per-element bound |err| <= c 2^-24 D (abs_bound).
"""
import numpy as np
import torch
import torch.nn.functional as F

Q = 2.0 ** -18          # the grid of every exact case
HEADROOM = 2.0 ** 24    # sum |a| |w| < HEADROOM * Q
KINDS = ("A3", "W3", "A2W2")
# the six retained products as (term of the first operand, term of the second): csrc/split.h SPLIT_PA / SPLIT_PB; 0 = h, 1 = m, 2 = l
CLASSES = {"lh": (2, 0), "hl": (0, 2), "mm": (1, 1), "mh": (1, 0), "hm": (0, 1), "hh": (0, 0)}
# the classes each kind is there to exercise (first operand = pixels / activations, second = filters)
KIND_CLASSES = {"A3": ("hh", "mh", "lh"), "W3": ("hh", "hm", "hl"), "A2W2": ("hh", "mh", "hm", "mm")}


# ------------------------------------------------------------------------------------------------------------ the split, restated
def bf16_rne(x):
    """float32 array -> the nearest bf16 (ties to even) as float32, in integer arithmetic on the bit pattern."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32).astype(np.uint64)
    hi = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint32)
    return (hi << 16).view(np.float32).reshape(x.shape)


def bf16_trunc(x):
    """float32 array -> bf16 by dropping the low 16 bits (the WRONG rounding; the sensitivity check uses it)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(x.shape)


def split_terms(x, trunc_plane=None):
    """The three bf16 terms (h, m, l) of an fp32 array as float32 arrays: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), each rounded
    to nearest even, the residues exact fp32 subtractions (csrc/split.h).  trunc_plane = 0 / 1 / 2 (sensitivity checks only): that one
    plane is what truncation makes of the value it rounds, the other two stay as they are -- a plane formed with the wrong rounding."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = bf16_rne(x)
    r = x - h
    m = bf16_rne(r)
    r2 = r - m
    terms = [h, m, bf16_rne(r2)]
    if trunc_plane is not None:
        terms[trunc_plane] = bf16_trunc((x, r, r2)[trunc_plane])
    return tuple(terms)


# ------------------------------------------------------------------------------------------------------------ exact cases
def _multi(rng, shape, nterms, amax):
    """s (a +- b 2^-9 +- c 2^-18), a in 1..amax, b, c in 1..3, random signs; nterms = 1 / 2 / 3 keeps a / a, b / a, b, c.  The inner signs
    make the first and second roundings go both ways (and hit ties), so a plane rounded by truncation differs from the right one."""
    v = rng.integers(1, amax + 1, shape).astype(np.float64)
    if nterms >= 2:
        v += rng.integers(1, 4, shape) * rng.choice([-1.0, 1.0], shape) * 2.0 ** -9
    if nterms >= 3:
        v += rng.integers(1, 4, shape) * rng.choice([-1.0, 1.0], shape) * 2.0 ** -18
    return (v * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _ints(rng, shape, wmax, zeros=True):
    v = rng.integers(-wmax, wmax + 1, shape) if zeros else rng.integers(1, wmax + 1, shape) * rng.choice([-1, 1], shape)
    return v.astype(np.float32)


def _spread(rng, rows, K, nnz):
    """nnz positions per row, one in each of nnz equal strata of 0..K-1: spread over the whole of K."""
    nnz = min(nnz, K)
    lo = (np.arange(nnz) * K) // nnz
    hi = (np.arange(1, nnz + 1) * K) // nnz
    return lo[None, :] + (rng.random((rows, nnz)) * (hi - lo)[None, :]).astype(np.int64)


def _operands(kind, rng, a_shape, w_shape, a_amax, w_amax):
    """dense values of both operands for a kind: (first, second)."""
    if kind == "A3":
        return _multi(rng, a_shape, 3, a_amax), _ints(rng, w_shape, w_amax)
    if kind == "W3":
        return _ints(rng, a_shape, w_amax, zeros=False), _multi(rng, w_shape, 3, a_amax)
    if kind == "A2W2":
        return _multi(rng, a_shape, 2, a_amax), _multi(rng, w_shape, 2, w_amax)
    raise ValueError(kind)


def exact_case(kind, rows, K, N, seed, nnz=8, taps=1):
    """A [rows][K] with at most nnz non-zeros per row (spread over K) and W [N][taps * K] dense, float32, on the grid Q.
    |A| <= 3 + 3 2^-9 + 3 2^-18 and |W| <= 2 + 3 2^-9 (A3 / A2W2), |A| <= 2 and |W| <= 3 + ... (W3): with nnz * taps <= 9 non-zero products per
    output the sum of |a| |w| stays below 9 * 3.006 * 2.006 = 54.3 < 64 = 2^24 Q.  taps > 1: the filter bank of a taps-tap convolution
    over a map whose pixels are the rows of A, K index (tap, channel)."""
    rng = np.random.default_rng([seed, rows, K, N, KINDS.index(kind)])
    dense, W = _operands(kind, rng, (rows, K), (N, taps * K), 3, 2)
    A = np.zeros((rows, K), np.float32)
    pos = _spread(rng, rows, K, nnz)
    np.put_along_axis(A, pos, np.take_along_axis(dense, pos, 1), 1)
    return A, W


def exact_stem_case(kind, seed, B=2, H=17, Wd=19, Cout=64):
    """Dense operands of the Cin = 3, 3x3 stem (K = 27): x [B][3][H][Wd], w [Cout][3][3][3] (OIHW).  Leading digit 1 on the multi-term
    side, |v| <= 2 on the other: 27 * 1.006 * 2.006 = 54.5 < 64."""
    rng = np.random.default_rng([seed, 27, KINDS.index(kind)])
    x, w = _operands(kind, rng, (B, 3, H, Wd), (Cout, 3, 3, 3), 1, 1 if kind == "A2W2" else 2)
    return x, w


def map_of_rows(A, H, Wd):
    """A [H * Wd][C] (pixel rows) -> x [1][C][H][Wd]."""
    return np.ascontiguousarray(A.reshape(1, H, Wd, A.shape[1]).transpose(0, 3, 1, 2))


def bank_oihw(W, C, kh=3, kw=3):
    """W [N][kh * kw * C], K index (tap, channel) -> OIHW [N][C][kh][kw]."""
    return np.ascontiguousarray(W.reshape(W.shape[0], kh, kw, C).transpose(0, 3, 1, 2))


def conv64(x, w, stride=1, pad=0, dil=1):
    """float64 F.conv2d of float32 / float64 numpy or torch operands (NCHW, OIHW) -> torch float64."""
    return F.conv2d(torch.as_tensor(x).double(), torch.as_tensor(w).double(), None, stride, pad, dil)


def class_conv64(x, w, stride=1, pad=0, dil=1, leave_out=None, trunc_plane=None):
    """The convolution as the split route forms it, in float64 from the split terms: the sum of the six retained classes (CLASSES), or of
    five of them (leave_out = a class name).  trunc_plane: that plane of BOTH operands formed by truncation (split_terms).  Returns
    (sum, {class: its contribution})."""
    tx = split_terms(x, trunc_plane)
    tw = split_terms(w, trunc_plane)
    parts = {name: conv64(tx[i], tw[j], stride, pad, dil) for name, (i, j) in CLASSES.items()}
    return sum(v for name, v in parts.items() if name != leave_out), parts


def gemm_as_conv(A, W):
    """A [rows][K], W [N][K] -> (x [1][K][rows][1], w [N][K][1][1]): a GEMM as a 1x1 convolution, for conv64 / abs_bound."""
    A, W = np.asarray(A), np.asarray(W)
    return np.ascontiguousarray(A.T.reshape(1, A.shape[1], A.shape[0], 1)), W.reshape(W.shape[0], W.shape[1], 1, 1)


# ------------------------------------------------------------------------------------------------------------ scaling cases
def base_values(rng, shape, zero_frac=0.1):
    """float32 values with |v| in {0} U [2^-10, 8): a random 24-bit significand, an exponent uniform in -10..2, a random sign."""
    mant = 1.0 + rng.integers(0, 1 << 23, shape) * 2.0 ** -23
    v = np.ldexp(mant, rng.integers(-10, 3, shape)) * rng.choice([-1.0, 1.0], shape)
    v[rng.random(shape) < zero_frac] = 0.0
    return v.astype(np.float32)


def exponents(rng, shape, lo, hi):
    """integers uniform in lo..hi; the first two (in flat order) are lo and hi themselves, so both ends of the range are run."""
    e = rng.integers(lo, hi + 1, shape).astype(np.int32)
    flat = e.reshape(-1)
    if flat.size >= 2:
        flat[0], flat[1] = lo, hi
    return e


def scaled(v, e):
    """v * 2^e in float32 (exact inside the ranges test_envelope_cpu.py checks); e broadcasts against v."""
    out = np.ldexp(np.asarray(v, np.float64), np.asarray(e))
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def scaling_case(rows, K, N, seed, lim=26, glim=8):
    """A GEMM / 1x1 problem: base A [rows][K], W [N][K], residual R [rows][N] and exponents e [rows], f [N] in -lim..lim, g [N] in
    -glim..glim (the epilogue's scale 2^g).  The scaled problem is (A 2^e_i, W 2^f_j, scale 2^g_j, R 2^(e_i + f_j + g_j)) against the
    base problem (A, W, scale 1, R); output (i, j) carries the exponent e_i + f_j + g_j."""
    rng = np.random.default_rng([seed, rows, K, N, 2])
    return dict(A=base_values(rng, (rows, K)), W=base_values(rng, (N, K)), R=base_values(rng, (rows, N)),
                e=exponents(rng, rows, -lim, lim), f=exponents(rng, N, -lim, lim), g=exponents(rng, N, -glim, glim))


def scaling_conv_case(B, H, Wd, Cin, Cout, dil, seed, lim=26, glim=8, k=3):
    """A k x k stride-1 pad = dil problem: base x [B][Cin][H][Wd], w [Cout][Cin][k][k], residual r [B][Cout][H][Wd]; exponents per image
    (ei [B]) and per lattice phase (ep [dil][dil], zeros at dil 1) that add up to at most lim in magnitude, per filter f [Cout] in
    -lim..lim, g [Cout] in -glim..glim.  An output pixel of phase (y mod dil, x mod dil) reads input pixels of that phase only, so with
    E[b][y][x] = ei[b] + ep[y mod dil][x mod dil] the output (b, c, y, x) carries E[b][y][x] + f[c] + g[c]."""
    rng = np.random.default_rng([seed, B, H, Wd, Cin, Cout, dil, 3])
    half = lim // 2
    ei = exponents(rng, B, -half, half) if dil > 1 else exponents(rng, B, -lim, lim)
    ep = exponents(rng, (dil, dil), -half, half) if dil > 1 else np.zeros((1, 1), np.int32)
    yy, xx = np.arange(H) % dil, np.arange(Wd) % dil
    E = ei[:, None, None] + ep[yy][:, xx][None]
    return dict(x=base_values(rng, (B, Cin, H, Wd)), w=base_values(rng, (Cout, Cin, k, k)), r=base_values(rng, (B, Cout, H, Wd)),
                ei=ei, ep=ep, E=E.astype(np.int32), f=exponents(rng, Cout, -lim, lim), g=exponents(rng, Cout, -glim, glim))


def scaling_stem_case(seed, B=2, H=17, Wd=19, Cout=64, lim=26, glim=8):
    """The Cin = 3 stem: base x [B][3][H][Wd], w [Cout][3][3][3], exponents per image and per output channel."""
    rng = np.random.default_rng([seed, 27, 4])
    return dict(x=base_values(rng, (B, 3, H, Wd)), w=base_values(rng, (Cout, 3, 3, 3)),
                ei=exponents(rng, B, -lim, lim), f=exponents(rng, Cout, -lim, lim), g=exponents(rng, Cout, -glim, glim))


def lowest_bit(v):
    """The value of the lowest set bit of each non-zero float32 (as float64); inf for zeros.  Every partial sum of products of two
    arrays is a multiple of lowest_bit(a).min() * lowest_bit(b).min(), before and after any rounding to fp32."""
    v = np.abs(np.asarray(v, np.float32)).astype(np.float64)
    m, e = np.frexp(v)
    n = (m * 2.0 ** 24).astype(np.int64)            # a 24-bit integer significand (exact: v is a float32)
    low = (n & -n).astype(np.float64)
    with np.errstate(over="ignore"):
        out = np.ldexp(low, e - 24)
    return np.where(v == 0, np.inf, out)


# ------------------------------------------------------------------------------------------------------------ bound cases
def bound_gemm_case(rows, K, N, seed, spread=20):
    """randn operands with factors 2^u, u uniform in [-spread, spread]: one per row of A, one per input channel (a column of A: the
    outlier channels of an activation map), one per filter (a row of W: the folded BatchNorm scales); a generic per-channel scale and
    shift and a residual of the outputs' own magnitude."""
    g = torch.Generator().manual_seed(seed * 7919 + rows + K + N)
    pw = lambda n: torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * 2 * spread - spread)  # noqa: E731
    ur, uk, uf = pw(rows), pw(K), pw(N)
    A = (torch.randn(rows, K, generator=g, dtype=torch.float64) * ur[:, None] * uk[None, :]).float()
    W = (torch.randn(N, K, generator=g, dtype=torch.float64) * uf[:, None]).float()
    scale = ((torch.rand(N, generator=g, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)).float()
    mag = ur[:, None] * uf[None, :] * uk.max() * K ** 0.5
    shift = (torch.randn(N, generator=g, dtype=torch.float64) * uf * uk.max()).float()
    res = (torch.randn(rows, N, generator=g, dtype=torch.float64) * mag).float()
    return dict(A=A, W=W, scale=scale, shift=shift, res=res)


def bound_conv_case(B, H, Wd, Cin, Cout, seed, spread=20, k=3):
    """The same for a k x k convolution: factors per pixel, per input channel and per filter."""
    g = torch.Generator().manual_seed(seed * 7919 + B + H + Wd + Cin + Cout)
    pw = lambda *n: torch.exp2(torch.rand(*n, generator=g, dtype=torch.float64) * 2 * spread - spread)  # noqa: E731
    up, uk, uf = pw(B, 1, H, Wd), pw(1, Cin, 1, 1), pw(Cout)
    x = (torch.randn(B, Cin, H, Wd, generator=g, dtype=torch.float64) * up * uk).float()
    w = (torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64) * uf.view(-1, 1, 1, 1)).float()
    scale = ((torch.rand(Cout, generator=g, dtype=torch.float64) + 0.5) * (torch.randint(0, 2, (Cout,), generator=g) * 2 - 1)).float()
    shift = (torch.randn(Cout, generator=g, dtype=torch.float64) * uf * uk.max()).float()
    res = (torch.randn(B, Cout, H, Wd, generator=g, dtype=torch.float64) * up * uf.view(1, -1, 1, 1) * uk.max() * (Cin * k * k) ** 0.5).float()
    return dict(x=x, w=w, scale=scale, shift=shift, res=res)


def abs_bound(x, w, scale=None, shift=None, res=None, stride=1, pad=0, dil=1):
    """The float64 per-element denominator D = |scale_j| conv(|x|, |w|) + |shift_j| + |res| (NCHW / OIHW operands; scale, shift [Cout];
    res the output's shape; None = 1 / 0 / 0).  Every rounding a kernel commits on the way to output (i, j) is relative to a partial
    sum or an epilogue value bounded by D_ij, so |err_ij| <= c 2^-24 D_ij with c counting the roundings."""
    D = conv64(torch.as_tensor(x).double().abs(), torch.as_tensor(w).double().abs(), stride, pad, dil)
    if scale is not None:
        D = D * torch.as_tensor(scale).double().abs().view(1, -1, 1, 1)
    if shift is not None:
        D = D + torch.as_tensor(shift).double().abs().view(1, -1, 1, 1)
    if res is not None:
        D = D + torch.as_tensor(res).double().abs()
    return D


def ref64(x, w, scale=None, shift=None, res=None, stride=1, pad=0, dil=1, relu=False):
    """float64 act(scale * conv(x, w) + shift + res)."""
    y = conv64(x, w, stride, pad, dil)
    if scale is not None:
        y = y * torch.as_tensor(scale).double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + torch.as_tensor(shift).double().view(1, -1, 1, 1)
    if res is not None:
        y = y + torch.as_tensor(res).double()
    return y.relu() if relu else y


# ------------------------------------------------------------------------------------------------------------ the cases both test files use
SEED = 21
EXACT_GEMM_SHAPES = [(135, 64, 96), (135, 2304, 40)]     # rows, K, N: one full 128-row tile + a ragged one; partial column tiles
EXACT_LINEAR_SHAPE = (135, 2304, 96)
EXACT_CONV3 = dict(H=9, Wd=15, Cin=64, N=40)              # 135 pixels, K = 9 * 64, one non-zero channel per pixel
EXACT_DUAL = dict(B=2, H2=17, W2=19, stride2=2, Cin=32, Cin2=32, Cout=96)   # 2 x 9 x 10 = 180 output rows
SCALE_GEMM_SHAPES = EXACT_GEMM_SHAPES + [EXACT_LINEAR_SHAPE]
SCALE_CONV3 = dict(B=2, H=13, Wd=11, Cin=64, Cout=40)
SCALE_CONV3_DILS = (1, 2, 4)
SCALE_WINO = dict(B=2, H=23, Wd=29, Cin=256, Cout=32)
SCALE_WINO_DILS = (1, 2, 12)
SCALE_WINO_FUSED = dict(B=2, H=23, Wd=29, Cin=64, Cout=64)
WINO_LIM = 12                                              # the transforms round: their intermediates sit on no grid
ATTENTION_SHAPES = [(2, 130, 2), (1, 33, 3)]               # B, tokens, heads
ATTENTION_LIM = 20


def exact_conv3(kind):
    """(x [1][Cin][H][Wd], w [N][Cin][3][3]) of the exact 3x3 pad-1 case."""
    c = EXACT_CONV3
    A, W = exact_case(kind, c["H"] * c["Wd"], c["Cin"], c["N"], SEED, nnz=1, taps=9)
    return map_of_rows(A, c["H"], c["Wd"]), bank_oihw(W, c["Cin"])


def exact_dual(kind):
    """(A [rows][Cin + Cin2], W [Cout][Cin + Cin2]) of the exact concatenated-K case; columns < Cin are the first operand's channels."""
    c = EXACT_DUAL
    ho, wo = (c["H2"] - 1) // c["stride2"] + 1, (c["W2"] - 1) // c["stride2"] + 1
    return exact_case(kind, c["B"] * ho * wo, c["Cin"] + c["Cin2"], c["Cout"], SEED + 1)


def exact_problems():
    """Every exact case the GPU tests run, in convolution form: dicts id, kind, x (NCHW), w (OIHW), stride, pad."""
    out = []
    for kind in KINDS:
        for shape in EXACT_GEMM_SHAPES + [EXACT_LINEAR_SHAPE]:
            x, w = gemm_as_conv(*exact_case(kind, *shape, SEED))
            out.append(dict(id=f"gemm{'x'.join(map(str, shape))}-{kind}", kind=kind, x=x, w=w, stride=1, pad=0))
        x, w = exact_conv3(kind)
        out.append(dict(id=f"conv3-{kind}", kind=kind, x=x, w=w, stride=1, pad=1))
        x, w = gemm_as_conv(*exact_dual(kind))
        out.append(dict(id=f"dual-{kind}", kind=kind, x=x, w=w, stride=1, pad=0))
        x, w = exact_stem_case(kind, SEED)
        out.append(dict(id=f"stem-{kind}", kind=kind, x=x, w=w, stride=2, pad=1))
    return out


def attention_case(B, N, heads, seed=SEED):
    """qkv [B][N][3 * heads * 64]: q, k ~ randn (the softmax weights stay above e^-30), v from base_values; f [heads * 64] in
    -ATTENTION_LIM..ATTENTION_LIM scales column d of head h of V, and the output column with it."""
    rng = np.random.default_rng([seed, B, N, heads, 5])
    D = heads * 64
    qkv = np.concatenate([rng.standard_normal((B, N, 2 * D)).astype(np.float32), base_values(rng, (B, N, D))], axis=2)
    return dict(qkv=qkv, f=exponents(rng, D, -ATTENTION_LIM, ATTENTION_LIM))


def scaling_problems():
    """Every scaling case the GPU tests run, in convolution form: dicts id, x, w, r (residual or None), stride, pad, dil, and the
    extreme exponent sums: acc_min (pixel + filter, where the accumulation runs), out_min / out_max (with the epilogue's g)."""
    out = []

    def add(name, x, w, r, e_in, f, g, stride=1, pad=0, dil=1):
        e_in, f, g = np.asarray(e_in), np.asarray(f), np.asarray(g)
        out.append(dict(id=name, x=x, w=w, r=r, stride=stride, pad=pad, dil=dil, acc_min=int(e_in.min() + f.min()),
                        out_min=int(e_in.min() + (f + g).min()), out_max=int(e_in.max() + (f + g).max()),
                        acc_max=int(e_in.max() + f.max())))

    for shape in SCALE_GEMM_SHAPES:
        c = scaling_case(*shape, SEED)
        x, w = gemm_as_conv(c["A"], c["W"])
        add(f"gemm{'x'.join(map(str, shape))}", x, w, c["R"].T.reshape(1, shape[2], shape[0], 1), c["e"], c["f"], c["g"])
    for dil in SCALE_CONV3_DILS:
        c = scaling_conv_case(**SCALE_CONV3, dil=dil, seed=SEED)
        add(f"conv3-d{dil}", c["x"], c["w"], c["r"], c["E"], c["f"], c["g"], 1, dil, dil)
    c = scaling_stem_case(SEED)
    add("stem", c["x"], c["w"], None, c["ei"], c["f"], c["g"], 2, 1, 1)
    for dil in SCALE_WINO_DILS:
        c = scaling_conv_case(**SCALE_WINO, dil=dil, seed=SEED, lim=WINO_LIM)
        add(f"wino-d{dil}", c["x"], c["w"], None, c["E"], c["f"], c["g"], 1, dil, dil)
    c = scaling_conv_case(**SCALE_WINO_FUSED, dil=1, seed=SEED, lim=WINO_LIM)
    add("wino-fused", c["x"], c["w"], None, c["E"], c["f"], c["g"], 1, 1, 1)
    return out
