"""What tests/test_gpu_envelope.py relies on, proved from the inputs alone (no GPU, no library): the exact cases sit on their grid with
room to spare and reach every retained product class; a split kernel that loses one class, or forms one plane with the wrong rounding,
cannot reproduce their float64 results; and the scaling cases neither overflow nor go subnormal at either end of their exponent ranges."""
import functools

import numpy as np
import pytest
import torch

import envelope_ref as er


@functools.lru_cache(maxsize=None)
def exact_problems():
    return er.exact_problems()


@functools.lru_cache(maxsize=None)
def scaling_problems():
    return er.scaling_problems()


def _ids(problems):
    return [p["id"] for p in problems]


def test_split_terms_restate_the_definition():
    """h + m + l == x exactly for fp32 values inside the split's range, each term is a bf16, ties go to even at both levels."""
    rng = np.random.default_rng(7)
    x = np.concatenate([er.base_values(rng, 4096) * np.float32(2.0) ** rng.integers(-60, 60, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -16, 3.3895e38, -2.0 ** -100])]).astype(np.float32)
    h, m, l = er.split_terms(x)
    for t in (h, m, l):
        assert not (t.view(np.uint32) & 0xFFFF).any()
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    assert er.bf16_rne(np.float32([1.0 + 2.0 ** -8]))[0] == 1.0 and er.bf16_rne(np.float32([1.0 + 3 * 2.0 ** -8]))[0] == np.float32(1.0 + 2.0 ** -6)
    assert er.bf16_trunc(np.float32([1.0 + 3 * 2.0 ** -8]))[0] == np.float32(1.0 + 2.0 ** -7)


@pytest.mark.parametrize("p", exact_problems(), ids=_ids(exact_problems()))
def test_exact_case_sits_on_its_grid_and_reaches_its_classes(p):
    x, w, kind = p["x"], p["w"], p["kind"]
    geo = (p["stride"], p["pad"])
    tx, tw = er.split_terms(x), er.split_terms(w)
    # every value and every term is a multiple of the grid of ITS side, and the product of the two side grids is Q: so is every product
    gx = min(er.lowest_bit(t).min() for t in tx + (x,))
    gw = min(er.lowest_bit(t).min() for t in tw + (w,))
    assert gx * gw >= er.Q, (gx, gw)
    # the terms add up to the values, and a side has an l term only where the other side is h alone: the dropped products are zero
    for v, t in ((x, tx), (w, tw)):
        assert np.array_equal(sum(a.astype(np.float64) for a in t), v.astype(np.float64))
    for i, j in ((1, 2), (2, 1), (2, 2)):
        assert not tx[i].any() or not tw[j].any(), (kind, i, j)
    # sum_k (|h| + |m| + |l|)(|h'| + |m'| + |l'|) < 2^24 Q for every output: every partial sum of either route, in any order, is exact
    ax = sum(np.abs(t).astype(np.float64) for t in tx)
    aw = sum(np.abs(t).astype(np.float64) for t in tw)
    room = er.conv64(ax, aw, *geo)
    assert room.max().item() < er.HEADROOM * er.Q, room.max().item()
    assert er.conv64(np.abs(x), np.abs(w), *geo).max().item() < er.HEADROOM * er.Q
    # the float64 result is an fp32 number, and the six classes add up to it
    ref = er.conv64(x, w, *geo)
    assert torch.equal(ref.float().double(), ref)
    total, parts = er.class_conv64(x, w, *geo)
    assert torch.equal(total, ref)
    for name in er.KIND_CLASSES[kind]:
        share = (parts[name] != 0).double().mean().item()
        assert share >= 0.25, (kind, name, share)
    assert (ref != 0).double().mean().item() >= 0.25


def _by_shape(problems):
    groups = {}
    for p in problems:
        groups.setdefault(p["id"].rsplit("-", 1)[0], []).append(p)
    return groups


@pytest.mark.parametrize("shape", sorted(_by_shape(exact_problems())))
def test_a_wrong_split_kernel_cannot_pass_the_exact_cases(shape):
    """Leave one retained class out, or form the h or the m plane by truncation: for each such fault at least one of the three kinds
    then differs from the float64 result in at least 10 % of its outputs.  (The l plane rounds a residue of at most 8 significant bits:
    truncation and round-to-nearest-even agree on it, which is checked; it is not a fault.)"""
    group = _by_shape(exact_problems())[shape]
    assert sorted(p["kind"] for p in group) == sorted(er.KINDS)
    worst = {}
    for p in group:
        geo = (p["stride"], p["pad"])
        ref = er.conv64(p["x"], p["w"], *geo)
        for name in er.CLASSES:
            got, _ = er.class_conv64(p["x"], p["w"], *geo, leave_out=name)
            worst[name] = max(worst.get(name, 0.0), (got != ref).double().mean().item())
        for plane in (0, 1):
            got, _ = er.class_conv64(p["x"], p["w"], *geo, trunc_plane=plane)
            worst[f"trunc{plane}"] = max(worst.get(f"trunc{plane}", 0.0), (got != ref).double().mean().item())
        assert torch.equal(er.class_conv64(p["x"], p["w"], *geo, trunc_plane=2)[0], ref)
    assert set(worst) == set(er.CLASSES) | {"trunc0", "trunc1"}
    assert min(worst.values()) >= 0.10, worst


@pytest.mark.parametrize("p", scaling_problems(), ids=_ids(scaling_problems()))
def test_scaling_case_stays_inside_the_normal_range(p):
    """Every partial sum of products of x and w is a multiple of lowest_bit(x) * lowest_bit(w) (rounding to fp32 keeps multiples of a finer
    grid), and so is every bf16 term product: a term is a multiple of its value's lowest bit.  With that grain times 2^(smallest exponent
    sum) >= 2^-126 no non-zero intermediate of the scaled launch is subnormal -- which covers the smallest non-zero term product; with the
    largest sum |x| |w| (+ |r|) times 2^(largest exponent sum) < 2^127 none overflows."""
    x, w, r = p["x"], p["w"], p["r"]
    assert np.abs(x).max() < 8 and np.abs(w).max() < 8 and np.abs(x[x != 0]).min() >= 2.0 ** -10 and np.abs(w[w != 0]).min() >= 2.0 ** -10
    grain = er.lowest_bit(x).min() * er.lowest_bit(w).min()
    tx, tw = er.split_terms(x), er.split_terms(w)
    smallest_term_product = min(np.abs(t[t != 0]).min() for t in tx) * min(np.abs(t[t != 0]).min() for t in tw)
    assert smallest_term_product >= grain
    assert grain * 2.0 ** p["acc_min"] >= 2.0 ** -126 and grain * 2.0 ** p["out_min"] >= 2.0 ** -126, (grain, p["acc_min"], p["out_min"])
    D = er.abs_bound(x, w, None, None, None, p["stride"], p["pad"], p["dil"])
    assert D.max().item() * 2.0 ** p["acc_max"] < 2.0 ** 127
    if r is not None:
        assert er.lowest_bit(r).min() * 2.0 ** p["out_min"] >= 2.0 ** -126
        D = D + torch.as_tensor(r).double().abs()
    assert D.max().item() * 2.0 ** p["out_max"] < 2.0 ** 127
    # both ends of every exponent range are present
    assert p["out_min"] < -20 and p["out_max"] > 20


@pytest.mark.parametrize("shape", er.ATTENTION_SHAPES)
def test_attention_scaling_case_stays_inside_the_normal_range(shape):
    """The smallest softmax weight (float64) at its lowest of 24 bits, times the lowest bit of V, times 2^-20, is a normal fp32 number;
    the largest output times 2^20 is far from overflow."""
    B, N, heads = shape
    c = er.attention_case(*shape)
    qkv = torch.from_numpy(c["qkv"]).double()
    q, k, v = [t.view(B, N, heads, 64).permute(0, 2, 1, 3) for t in qkv.split(heads * 64, dim=2)]
    s = q @ k.transpose(-1, -2) * 0.125
    p_min = torch.exp(s - s.max(-1, keepdim=True).values).min().item()
    assert p_min * 2.0 ** -24 * er.lowest_bit(c["qkv"][..., 2 * heads * 64:]).min() * 2.0 ** -er.ATTENTION_LIM >= 2.0 ** -126
    assert np.abs(c["qkv"]).max() * N * 2.0 ** er.ATTENTION_LIM < 2.0 ** 127
    assert c["f"].min() == -er.ATTENTION_LIM and c["f"].max() == er.ATTENTION_LIM


def test_abs_bound_dominates_the_error_of_an_fp32_chain():
    """abs_bound against an independent statement: an fp32 k-ordered fmaf-free chain (numpy float32 multiply-adds) of a bound case stays
    inside (2 K + 4) 2^-24 D -- twice the fmaf chain's K, one rounding for each product and one for each add -- element for element."""
    c = er.bound_gemm_case(37, 64, 24, 3)
    A, W = c["A"].numpy(), c["W"].numpy()
    acc = np.zeros((37, 24), np.float32)
    for k in range(64):
        acc = acc + A[:, k:k + 1] * W[None, :, k]
    got = (acc * c["scale"].numpy()[None] + c["shift"].numpy()[None]) + c["res"].numpy()
    x, w = er.gemm_as_conv(A, W)
    res = c["res"].t().reshape(1, 24, 37, 1)
    ref = er.ref64(x, w, c["scale"], c["shift"], res)
    D = er.abs_bound(x, w, c["scale"], c["shift"], res)
    err = (torch.from_numpy(got.T.reshape(1, 24, 37, 1)).double() - ref).abs()
    assert (err <= (2 * 64 + 4) * 2.0 ** -24 * D).all()
    assert (D.max() / D.min()).item() > 2.0 ** 40  # the spread a global maximum would hide
