"""Ties tests/flow_tail_ref.py (the float64 definition of the key-frame window tail) to what the repository already trusts, without
a GPU, so that tests/test_gpu_flow_tail.py does not rest on a new unchecked reference:

  * seg_tail_ref against oracle/flow_oracle.predict_segmentation on every committed geometry,
  * through the toy encoder / decoder against the reference-generated tests/golden/toy_predict.npz,
  * canvas_ref against oracle/crops_oracle.compute_output,
  * the weights rule against tests/cut_ref.window_weights,

and asserts, for every committed case and seed, the two quantities the GPU tolerances are built from: e_cpu32 (the fp32 torch-CPU
chain against the float64 one, max|err| / max|ref|) and the share of pixels the decided() rule leaves out of the mask comparison
(at most 0.5 %: half of what the GPU test allows).  Run with -s to see the figures."""
import pytest
import torch
import torch.nn.functional as F

import flow_tail_ref as R
from conftest import load_golden, rel_err, toy_weights
from flood_uav_video_segmentation_amd import synth
from oracle import crops_oracle, flow_oracle

torch.set_grad_enabled(False)

SHARE_CAP = 0.005
# fp32 against float64 over one chain: the key frame's resize, then per warp step a grid_sample, the resize of its result and the
# blend.  A stage rounds its weights, products and sums (<= 16 roundings of 2^-24 relative to the map's maximum), and its fp32
# source coordinate is off by up to an ulp of the source extent s (s * 2^-23), which a map of slope <= 2 max|v| per source cell
# turns into 4 s * 2^-24 max|v| -- the dominant term when a 20 x 24 map is sampled DOWN (measured 2.0e-6 there, 1e-7 .. 7e-7
# elsewhere).  A bound with room, from the formats, not a measurement.
def f32_bound(steps, extent):
    return (1 + steps) * (16 + 4 * extent) * 2.0 ** -24


def case_bound(name, mode):
    K, h, w, Hg, Wg, H, W, n, _ = R.TAIL_CASES[name]
    return f32_bound(n - 1, max(h, w, Hg, Wg)) if mode == "warp" else f32_bound(0, max(h, w))


def _oracle_f32(inp, mode):
    """flow_oracle.predict_segmentation on the case's fp32 inputs: enc is the identity on a frame that only carries the output size
    and says which key frame it is, dec hands out that key frame's logits."""
    lo_prev, lo_next, gl, gr, n, (H, W), no_warp = R.tail_args(inp, mode)
    prev = torch.zeros(1, 1, H, W)
    nxt = None if lo_next is None else torch.ones(1, 1, H, W)
    dec = lambda f: lo_next if f.flatten()[0].item() == 1.0 else lo_prev  # noqa: E731
    if no_warp:
        gl, gr = synth.dummy_grids(n)
    return flow_oracle.predict_segmentation(lambda x: x, dec, prev, nxt, gl, gr, n, no_warp)["pred"]


@pytest.mark.parametrize("mode", R.TAIL_MODES)
@pytest.mark.parametrize("name", list(R.TAIL_CASES))
def test_reference_agrees_with_the_oracle_and_the_case_is_decidable(name, mode):
    inp = R.tail_inputs(name)
    ref, c32 = R.tail_pair(name, mode)
    K, n, (H, W) = inp["K"], inp["n"], inp["out_hw"]
    frames = 1 if mode == "single" else n
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (frames, K, H, W)
    ora = _oracle_f32(inp, mode)
    assert ora.dtype == torch.float32 and ora.shape == ref.shape
    e_oracle = rel_err(ora, ref)
    e_cpu32 = rel_err(c32, ref)
    share = R.undecided_share(ref, R.MARGIN * ref.abs().max().item())
    print(f"tail_{name}_{mode}: oracle_vs_f64={e_oracle:.2e} cpu32_vs_f64={e_cpu32:.2e} undecided={100 * share:.3f}%")
    assert torch.equal(ora, c32)  # the yardstick IS the oracle's chain
    assert e_oracle <= case_bound(name, mode)
    assert share <= SHARE_CAP


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("mode", ["warp", "no_warp"])
@pytest.mark.parametrize("name", list(R.CUT_CASES))
def test_cut_and_tie_inputs_are_fp32_close(name, mode, tie):
    """The cut row sets (decidable like the plain cases) and the planted-tie inputs (undecided by construction: only their logits
    and the first-index rule are checked on the GPU)."""
    ref, c32 = R.tail_pair(name, mode, None, True) if tie else R.tail_pair(name, mode, "cut")
    e = rel_err(c32, ref)
    share = R.undecided_share(ref, R.MARGIN * ref.abs().max().item())
    print(f"tail_{name}_{mode}_{'tie' if tie else 'cut'}: cpu32_vs_f64={e:.2e} undecided={100 * share:.3f}%")
    assert e <= case_bound(name, mode)
    if tie:
        assert torch.equal(ref[:, 0], ref[:, 2]) and share > 0.05
    else:
        assert share <= SHARE_CAP


@pytest.mark.parametrize("name", R.CANVAS_CASES)
@pytest.mark.parametrize("mode", R.TAIL_MODES)
def test_canvas_cases_fp32_yardstick(name, mode):
    canvas_hw, yx = R.canvas_layout(name)
    ref, c32, count = R.canvas_pair([R.tail_pair(name, mode), R.tail_pair(name, mode, swap=True)], yx, canvas_hw)
    H, W = R.TAIL_CASES[name][5:7]
    assert yx[1][0] + H == canvas_hw[0] and yx[1][1] + W == canvas_hw[1]  # touches the bottom-right corner exactly
    assert count.max().item() == 2.0 and count.min().item() == 0.0       # the placements overlap, and leave cells untouched
    e = (c32 - ref).abs().max().item()
    print(f"canvas_{name}_{mode}: cpu32_vs_f64(abs)={e:.2e}")
    assert e <= 2 * 32 * 2.0 ** -24  # two probabilities <= 1, each a few fp32 roundings + the logits' error through the softmax


def _toy_logits(x):
    w = toy_weights()
    return F.conv2d(F.relu(F.conv2d(x, w["enc_w"], w["enc_b"], 4, 1)), w["dec_w"], w["dec_b"])


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("nw", [False, True])
def test_reference_reproduces_the_toy_golden(n, nw):
    z = load_golden("toy_predict.npz")
    prev, nxt = torch.from_numpy(z["prev"]), torch.from_numpy(z["next"])
    h, w = prev.shape[2:]
    mvl, mvr = synth.dummy_grids(n) if nw else synth.make_grids(n, 4, 5, seed=40 + n, frame=(h, w), jitter=0.05)
    out = R.seg_tail_ref(_toy_logits(prev), _toy_logits(nxt), mvl, mvr, n, (h, w), nw)
    assert rel_err(out, z[f"predict_n{n}_fb0_nw{int(nw)}"]) < 1e-6  # as tests/test_oracle_golden.py asserts for the oracle


def test_reference_reproduces_the_toy_golden_single_frame():
    z = load_golden("toy_predict.npz")
    prev = torch.from_numpy(z["prev"])
    out = R.seg_tail_ref(_toy_logits(prev), None, [], [], 5, prev.shape[2:], False)
    assert out.shape[0] == 1 and rel_err(out, z["single_n5"]) < 1e-6


def test_canvas_ref_is_compute_output():
    """Four crops of 7 x 9 on a 10 x 13 frame, in compute_output's own crop order."""
    g = torch.Generator().manual_seed(5)
    n, K, ch, cw, H, W = 3, 5, 7, 9, 10, 13
    sets = [torch.randn(n, K, ch, cw, generator=g, dtype=torch.float64) * 3 for _ in range(4)]
    it = iter(sets)
    seen = []

    def predict(prev_crop, next_crop, ml, mr):
        seen.append(int(prev_crop[0, 0, 0, 0]))  # the frame holds y * W + x: the crop's top-left value names its offset
        return next(it)

    frame = torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W)
    out = crops_oracle.compute_output(predict, n, frame, frame, None, None, ch, cw, K)
    yx = [(v // W, v % W) for v in seen]
    assert yx == [(0, 0), (0, 4), (3, 0), (3, 4)]
    canvas, count = R.canvas_ref(sets, yx, (H, W))
    assert count.min() == 1 and count.max() == 4
    assert torch.allclose(canvas / count, out, rtol=1e-14, atol=0)
    # an uncovered cell is 0 / 0
    canvas, count = R.canvas_ref(sets[:1], yx[:1], (H, W))
    assert torch.isnan((canvas / count)[:, :, -1, -1]).all()


@pytest.mark.parametrize("name", ["base", "k9", "long"])
def test_weights_rule_against_window_weights(name):
    import cut_ref

    inp = R.tail_inputs(name)
    n = inp["n"]
    args = R.tail_args(inp, "warp")
    plain = R.seg_tail_ref(*args)
    # no cut: window_weights gives the linear rows (fp32-rounded), hence the unweighted result up to that rounding
    rows, source = cut_ref.window_weights([None] * n, n)
    assert (source == cut_ref.BLENDED).all() and torch.equal(torch.from_numpy(rows), R.linear_rows(n))
    assert rel_err(R.seg_tail_ref(*args, weights=torch.from_numpy(rows)), plain) <= 2.0 ** -23
    # a cut at pair c: frames < c are the forward chain alone, the rest the backward chain alone
    fwd = R.seg_tail_ref(*args, weights=torch.tensor([[1.0, 0.0]] * n))
    bwd = R.seg_tail_ref(*args, weights=torch.tensor([[0.0, 1.0]] * n))
    for c in sorted({1, 2, n - 1, n}):
        cut = R.seg_tail_ref(*args, weights=R.cut_rows(n, c))
        assert torch.equal(cut[0], plain[0])
        for f in range(1, n):
            assert torch.equal(cut[f], (fwd if f < c else bwd)[f]), (c, f)
    # a held frame carries no 0 * x term: a non-finite value in the unused chain does not reach it
    lo_next = inp["lo_next"].clone()
    lo_next[0, 0, 0, 0] = float("inf")
    held = R.seg_tail_ref(inp["lo_prev"], lo_next, *args[2:], weights=torch.tensor([[1.0, 0.0]] * n))
    assert torch.equal(held, fwd)


@pytest.mark.parametrize("case", R.CROP_CASES, ids=lambda c: f"{c[0]}-K{c[1]}-n{c[2]}-{'nowarp' if c[3] else 'warp'}")
def test_crops_cases_are_decidable(case):
    layout, K, n, nw = case
    ref, c32, count = R.crops_pair(layout, K, n, nw)
    covered = count > 0
    assert torch.isnan(ref[:, :, ~covered]).all() and torch.isfinite(ref[:, :, covered]).all()
    assert covered.all() == (layout in ("four", "whole"))
    if layout == "four":
        assert (count == 4).sum() == 1 and count[23, 27] == 4
    share = 1.0 - R.decided(ref[:, :, covered][..., None], R.CROP_MARGIN).double().mean().item()
    e = (c32 - ref)[:, :, covered].abs().max().item()
    print(f"crops_{layout}_K{K}_n{n}_nw{int(nw)}: cpu32_vs_f64(abs)={e:.2e} undecided={100 * share:.3f}%")
    assert share <= SHARE_CAP
    assert e <= 32 * 2.0 ** -24  # an average of probabilities <= 1


@pytest.mark.parametrize("kn", R.RESIZE_KN, ids=lambda kn: f"K{kn[0]}-n{kn[1]}")
@pytest.mark.parametrize("size", list(R.RESIZE_SIZES))
def test_resize_cases_are_decidable(size, kn):
    K, n = kn
    logits, canvas, count = R.resize_inputs(size, K, n)
    out = R.RESIZE_SIZES[size][1]
    r, arg = R.resize_argmax_ref(logits, out)
    assert r.dtype == torch.float64 and tuple(r.shape) == (n, K) + out and tuple(arg.shape) == (n,) + out
    rc, _ = R.resize_argmax_ref(canvas / count, out)
    s_logits = R.undecided_share(r, R.MARGIN * r.abs().max().item())
    s_canvas = R.undecided_share(rc, R.CANVAS_MARGIN * rc.abs().max().item())
    print(f"resize_{size}_K{K}_n{n}: undecided logits={100 * s_logits:.3f}% canvas={100 * s_canvas:.3f}%")
    assert s_logits <= SHARE_CAP and s_canvas <= SHARE_CAP
    # fp32 ATen resize against the float64 one: the figure INTERP_TOL of tests/test_gpu_ops.py bounds
    e = rel_err(F.interpolate(logits, size=out, mode="bilinear", align_corners=True), r)
    assert e < 2e-6


def test_decided_and_first_index_argmax():
    x = torch.tensor([[[[1.0, 2.0, 5.0]], [[1.0, 2.0 + 1e-3, 4.0]], [[0.0, 2.0 + 2e-3, 5.0]]]], dtype=torch.float64)  # [1,3,1,3]
    assert R.decided(x, 5e-4).tolist() == [[[False, True, False]]]
    assert R.decided(x, 2e-3).tolist() == [[[False, False, False]]]
    assert R.resize_argmax_ref(x, (1, 3))[1].tolist() == [[[0, 2, 0]]]  # exact ties go to the first index
    assert R.decided(x[:, :1], 1.0).all()
