"""The CNN networks against the CPU oracle in EVERY conv-route regime of the executor (csrc/net.hip), not only at the sizes the rest
of the suite happens to run.

csrc/net.hip picks each 3 x 3 conv's kernel from the geometry of one image: direct implicit GEMM, three-launch Winograd F(3,3) /
F(4,4) / F(6,6), the one-kernel Winograd, the one-kernel Winograd with the stem's max-pool fused in.  tests/net_routes_ref.py
restates those decisions; tests/test_net_routes_cpu.py enumerates the regimes they produce and demands a frame here for each.  For
every such frame, in one test:

  * the profiler's (name, kernel family) rows -- and the Winograd GEMM's booked flops, which pin the tile size -- equal the restated
    table, at B and at B + 1, and an image's rows do not change with the batch;
  * encoder, decoder and fused segment agree with the oracle evaluated in FLOAT64 to LOGIT_TOL = 3e-5, tests/test_gpu_net.py's figure;
  * a batch of two equals two single-frame calls bit for bit;
  * on a fresh handle, fs_reserve at this geometry and then the forwards grow no workspace (reserve_conv makes the same route
    decision on its own: a disagreement would be an undersized Winograd workspace).

Measured errors go to conftest.note's parity record as routes_<H>x<W>_{feat,logits,segment}_vs_f64; DESIGN.md section 5 quotes them."""
import time

import pytest
import torch

import net_routes_ref as R
from conftest import memo_by_content, note, rel_err
from flood_uav_video_segmentation_amd import synth
from flood_uav_video_segmentation_amd.model.deeplabv3 import FlowDeepLabv3
from flood_uav_video_segmentation_amd.model.pspnet import FlowPSPNet
from oracle import deeplab_oracle, pspnet_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOGIT_TOL = 3e-5  # tests/test_gpu_net.py: 3-5x the 3-8e-6 measured at 713 x 713


class HP:
    def __init__(self, layers=50, classes=5):
        self.layers, self.classes, self.pretrained = layers, classes, False


def _double(state):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}


class Case:
    """One network under test: the HIP mirror, its weights, and the oracle in float64 (and, for the one large frame, in fp32)."""

    def __init__(self, arch, cls, state, oracle):
        self.arch, self.cls, self.state, self.oracle = arch, cls, state, oracle
        self.state64 = _double(state)
        self.net = self.fresh()
        self.fp32 = memo_by_content(lambda x: self._oracle(x, self.state))

    def fresh(self):
        net = self.cls(HP(50, 5)).eval()
        net.load_state_dict(self.state)
        return net

    def _oracle(self, x, state):
        feat = self.oracle.encoder(x, state, 50)
        return feat, self.oracle.decoder(feat, state)

    def f64(self, x):
        return self._oracle(x.double(), self.state64)


@pytest.fixture(scope="module")
def psp():
    return Case("pspnet", FlowPSPNet, synth.make_pspnet_state(50, 5, seed=0), pspnet_oracle)


@pytest.fixture(scope="module")
def deeplab():
    return Case("deeplabv3", FlowDeepLabv3, synth.make_deeplab_state(50, 5, seed=0), deeplab_oracle)


def _profiled_segment(net, x):
    hn = net._hip_net
    hn.profile(True)
    try:
        out = net.segment(x)
        rows = hn.profile_dump()
    finally:
        hn.profile(False)
    return out, rows


def _assert_rows(got, want, what):
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not diff, f"{what}: profiler rows differ from the restated table (index, profiler, restated), " \
                                               f"{len(got)} vs {len(want)} rows: {diff[:6]}"


def _check(case, H, W, B, tag, big=False):
    net, arch = case.net, case.arch
    clip = synth.make_clip(B + 1, (H, W), seed=1000 + H + W)
    x, x1 = clip[:B].cuda(), clip.cuda()

    # ---- route table: at B, at B + 1, and per image the same
    seg, rows = _profiled_segment(net, x)
    want = R.route_table(arch, 50, B, H, W)
    _assert_rows(R.observed(rows), R.keyed(want), f"{tag} B={B}")
    seg1, rows1 = _profiled_segment(net, x1)
    want1 = R.route_table(arch, 50, B + 1, H, W)
    _assert_rows(R.observed(rows1), R.keyed(want1), f"{tag} B={B + 1}")
    assert R.per_image(want, B) == R.per_image(want1, B + 1)
    assert [(n, k, None if f is None else f / B) for n, k, f in R.observed(rows)] == \
           [(n, k, None if f is None else f / (B + 1)) for n, k, f in R.observed(rows1)]
    assert torch.equal(seg1[:B], seg)  # and neither does its result

    # ---- parity with the oracle
    feat = net.encoder(x)
    logits = net.decoder(feat)
    if big:
        t0 = time.perf_counter()
        ofeat, ologits = case.fp32(clip[:B])
        note(f"routes_{tag}_fp32_oracle_seconds", time.perf_counter() - t0)
        ref = "fp32_oracle"
    else:
        ofeat, ologits = case.f64(clip[:B])
        ref = "f64"
    assert feat.shape == ofeat.shape and logits.shape == ologits.shape == seg.shape
    e_feat = note(f"routes_{tag}_feat_vs_{ref}", rel_err(feat.cpu(), ofeat))
    e_logits = note(f"routes_{tag}_logits_vs_{ref}", rel_err(logits.cpu(), ologits))
    e_seg = note(f"routes_{tag}_segment_vs_{ref}", rel_err(seg.cpu(), ologits))
    assert e_feat < LOGIT_TOL and e_logits < LOGIT_TOL and e_seg < LOGIT_TOL, (e_feat, e_logits, e_seg)

    # ---- a batch of two is two single frames
    if B == 2:
        assert torch.equal(seg, torch.cat([net.segment(x[i:i + 1]) for i in range(2)], 0))

    # ---- fs_reserve sized every workspace this geometry's routes need
    fresh = case.fresh()
    hn = fresh._hip_net
    fresh.reserve(B, H, W)
    r0 = hn.reserved_bytes()
    assert r0 > 0
    again = fresh.segment(x)
    torch.cuda.synchronize()
    assert hn.reserved_bytes() == r0, "fs_segment_forward grew a workspace after fs_reserve"
    assert torch.equal(again, seg)
    f2 = fresh.encoder(x)
    fresh.decoder(f2)
    torch.cuda.synchronize()
    assert hn.reserved_bytes() == r0, "fs_encoder_forward / fs_decoder_forward grew a workspace after fs_reserve"
    assert torch.equal(f2, feat)


@pytest.mark.parametrize("H,W,B", [f for f in R.PSPNET_FRAMES if f[:2] != R.BIG_FRAME], ids=lambda v: str(v))
def test_pspnet_regime_against_the_float64_oracle(psp, H, W, B):
    _check(psp, H, W, B, f"{H}x{W}")


def test_pspnet_one_kernel_winograd_on_layer2_against_the_fp32_oracle(psp):
    """1217 x 1217, B = 1: the smallest (8k + 1)-square frame whose stride-8 map (153 x 153: 39 * 39 = 1521 tiles of 4 x 4) sends
    layer2's 128-channel convs to the one-kernel Winograd.  The one expensive case of this file: the oracle needs several seconds
    here in fp32 and twice that in float64, so it runs ONCE, in fp32, memoised on the clip's content, under the same LOGIT_TOL --
    the fp32 oracle is itself 2.5e-6 (features: 8.6e-7) from the float64 one on this clip's logits, measured on the CPU: an order
    below the tolerance.  Its wall time is recorded as routes_1217x1217_fp32_oracle_seconds (about 4 s on 16 CPUs; the whole
    case 5 - 6 s)."""
    H, W = R.BIG_FRAME
    _check(psp, H, W, 1, f"{H}x{W}", big=True)


@pytest.mark.parametrize("H,W,B", R.DEEPLAB_FRAMES, ids=lambda v: str(v))
def test_deeplabv3_regime_against_the_float64_oracle_parity_unpinned(deeplab, H, W, B):
    """DeepLabv3-50 at the smallest frame that keeps every ASPP conv on the direct kernel, and at the smallest where an ASPP dilation
    takes the lattice Winograd path while the 7 x 7-stem network's layer1.*.conv2 takes the one-kernel form (both picked from
    route_table: tests/test_net_routes_cpu.py).  PARITY UNPINNED, as for every DeepLabv3 test: the oracle restates torchvision."""
    _check(deeplab, H, W, B, f"deeplab_{H}x{W}")
