"""The CNN executor's host-side route decisions, restated in plain Python from csrc/kernels.h and csrc/net.hip.

`route_table(arch, layers, B, H, W, options)` gives, launch by launch, what fs_segment_forward's profiler would record for a
PSPNet / DeepLabv3 over ResNet-50 / 101 / 152: the row's name and its kernel FAMILY (the implicit GEMM's tile labels all fold into
`conv_igemm`, `stem_conv_split` into `stem_conv`), plus the Winograd tile size m and -- for the GEMM between the two transforms -- the
flops the profiler books, which are 2 * (m+2)^2 * tiles * Cin * Cout and so pin m from the outside.

No GPU code and no torch: tests/test_net_routes_cpu.py runs it anywhere, tests/test_gpu_net_routes.py holds the profiler against it.
A threshold moved in net.hip without this file following fails both.
"""
from collections import namedtuple
from functools import lru_cache

# name, family: as the profiler prints them (family(): labels folded); m: Winograd tile size of the three-launch rows, else 0;
# flops: booked flops of a `.wino_gemm` row, else None; stage: "stem" | "layer1".."layer4" | "aspp" | "head" for the 3x3 convs, else ""
Row = namedtuple("Row", "name family m flops stage")

BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
BINS = (1, 2, 3, 6)
OPTIONS = ("no_winograd", "no_fused_head", "no_fused_shortcut", "no_fused_winograd", "no_split_bf16", "no_res_touch", "no_fused_pool",
           "winograd_tile")

# ---------------------------------------------------------------------------------------------------------------------------
# The frames tests/test_gpu_net_routes.py runs: (H, W, B).  test_net_routes_cpu.py asserts that they cover every regime the
# dispatch has on square frames of 33..1300 px, so a moved threshold fails there until this list follows.
PSPNET_FRAMES = (
    (49, 49, 2),      # igemm stem, igemm layer1, F3 layer2, igemm layer3 / layer4, F3 head
    (169, 169, 2),    # the last size below the stem threshold
    (177, 177, 2),    # fused stem + pool, layer1 still on the implicit GEMM
    (185, 233, 2),    # F4 by the map itself; 24 x 30 map: one-pass pyramid, not square
    (257, 257, 1),    # F3 / F6 / F6 / F3 in one forward
    (345, 345, 1),    # just below the layer1 threshold
    (353, 353, 1),    # just above it
    (385, 385, 1),    # F4 / F6 / F4 / F4
    (625, 625, 1),    # F4 everywhere above the layer1 threshold (625 and 633 px are the only square frames that do it)
    (1217, 1217, 1),  # one-kernel Winograd on layer2's 128-channel convs
)
BIG_FRAME = (1217, 1217)  # the one expensive case: fp32 oracle, see the GPU test
DEEPLAB_FRAMES = (
    (33, 33, 2),      # the smallest frame: every ASPP conv on the direct kernel
    (353, 353, 1),    # the smallest with an ASPP dilation on the lattice Winograd path AND layer1.*.conv2 on the one-kernel form
)


def cdiv(a, b):
    return -(-a // b)


def conv_out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def winograd_tiles(B, H, W, dil, mt):
    return B * dil * dil * ((cdiv(H, dil) + mt - 1) // mt) * ((cdiv(W, dil) + mt - 1) // mt)


def winograd_gemm_rows(B, H, W, dil, mt):
    return float((mt + 2) * (mt + 2)) * float(cdiv(winograd_tiles(B, H, W, dil, mt), 64) * 64)


@lru_cache(maxsize=None)
def winograd_pick_m(H, W, dil):
    """kernels.h: the cheaper tile size for this map, on ONE image's geometry."""
    m = 6 if winograd_gemm_rows(1, H, W, dil, 6) < winograd_gemm_rows(1, H, W, dil, 4) else 4
    return 3 if winograd_gemm_rows(1, H, W, dil, 3) < winograd_gemm_rows(1, H, W, dil, m) else m


class Conv:
    """One conv of the plan (net.hip make_conv): geometry, and which Winograd forms it was given banks for."""

    def __init__(self, name, cin, cout, k, stride=1, pad=0, dil=1, hwio=False, stage=""):
        self.name, self.cin, self.cout, self.k, self.stride, self.pad, self.dil, self.stage = name, cin, cout, k, stride, pad, dil, stage
        chunk_major = not hwio and k * k > 1 and cin % 32 == 0
        self.wino = wino_eligible(self, hwio)
        self.wf = chunk_major and cin <= 128 and wino_fused_supported(cin, cout, k, stride, pad, dil)

    def out_size(self, n):
        return conv_out_size(n, self.k, self.stride, self.pad, self.dil)


def wino_eligible(c, hwio=False):
    return not hwio and c.k == 3 and c.stride == 1 and c.pad == c.dil and c.cin >= 128 and c.cin % 32 == 0 and c.cout % 4 == 0


def wino_fused_supported(cin, cout, k, stride, pad, dil):
    return k == 3 and stride == 1 and pad == 1 and dil == 1 and cin % 32 == 0 and 32 <= cin <= 256 and cout % 64 == 0


class Opts:
    def __init__(self, options=None):
        o = {(k[4:] if k.startswith("hip_") else k): v for k, v in dict(options or {}).items()}
        unknown = sorted(set(o) - set(OPTIONS))
        if unknown:
            raise ValueError(f"unknown option(s) {unknown}")
        self.use_winograd = not o.get("no_winograd", False)
        self.use_fused_winograd = not (o.get("no_fused_winograd", False) or o.get("no_winograd", False))
        self.use_fused_head = not o.get("no_fused_head", False)
        self.use_fused_shortcut = not o.get("no_fused_shortcut", False)
        self.use_fused_pool = not o.get("no_fused_pool", False)
        self.force_m = int(o.get("winograd_tile", 0))


def wino_m(opts, H, W, dil):
    return opts.force_m if opts.force_m else winograd_pick_m(H, W, dil)


def takes_winograd(opts, c, B, H, W, has_res=False):
    if not (c.wino and opts.use_winograd and not has_res):
        return False
    if c.cin < 256 and c.wf and opts.use_fused_winograd and cdiv(H, 4) * cdiv(W, 4) >= 1500:
        return False
    mt = wino_m(opts, H, W, c.dil)
    wino_rows = float((mt + 2) * (mt + 2)) * float(winograd_tiles(B, H, W, c.dil, mt))
    direct_rows = 9.0 * float(B) * c.out_size(H) * c.out_size(W)
    return wino_rows < (0.8 if c.dil <= 4 else 0.7) * direct_rows


def takes_fused_winograd(opts, c, B, H, W, ld_in, ld_out, has_res=False):
    fits = B * H * W * ld_in * 4 < (1 << 30) and B * H * W * ld_out * 4 < (1 << 31)
    return bool(c.wf and opts.use_fused_winograd and not has_res and fits and cdiv(H, 4) * cdiv(W, 4) >= 500)


def geometry(stem0, H, W):
    """(H1, W1) after the stem conv, (H2, W2) after the max-pool, (H3, W3) the stride-8 map."""
    H1, W1 = stem0.out_size(H), stem0.out_size(W)
    H2, W2 = conv_out_size(H1, 3, 2, 1, 1), conv_out_size(W1, 3, 2, 1, 1)
    return (H1, W1), (H2, W2), (conv_out_size(H2, 3, 2, 1, 1), conv_out_size(W2, 3, 2, 1, 1))


def one_pass_pyramid(fh, fw):
    return fh % 6 == 0 and fw % 6 == 0


def family(label):
    """A profiler kernel label -> its family: every implicit-GEMM tile ("igemm128x64", "split64x128", "split128x128cat", ...) is
    conv_igemm (the tile is a cost-model choice this file does not restate), the stem's two arithmetic routes are stem_conv."""
    if label.startswith(("igemm", "split")):
        return "conv_igemm"
    if label.startswith("stem_conv"):
        return "stem_conv"
    return label


class Plan:
    """net_finalize's layer plan for the torch-free part: names and shapes only."""

    def __init__(self, arch, layers):
        if arch not in ("pspnet", "deeplabv3") or layers not in BLOCKS:
            raise ValueError(f"route_table: arch {arch!r} / layers {layers!r}")
        self.psp = arch == "pspnet"
        bb = "" if self.psp else "backbone."
        if self.psp:
            self.stem = [Conv("layer0.0.weight", 3, 64, 3, 2, 1, 1, hwio=True), Conv("layer0.3.weight", 64, 64, 3, 1, 1, 1, stage="stem"),
                         Conv("layer0.6.weight", 64, 128, 3, 1, 1, 1, stage="stem")]
        else:
            self.stem = [Conv("backbone.conv1.weight", 3, 64, 7, 2, 3, 1, hwio=True)]
        self.blocks = []
        cin = self.stem[-1].cout
        for L, n in enumerate(BLOCKS[layers], 1):
            planes = 32 << L
            for b in range(n):
                pre = f"{bb}layer{L}.{b}."
                stride = 2 if (L == 2 and b == 0) else 1
                if self.psp:
                    dil = {3: 2, 4: 4}.get(L, 1)
                else:
                    dil = {3: 1 if b == 0 else 2, 4: 2 if b == 0 else 4}.get(L, 1)
                c1 = Conv(pre + "conv1.weight", cin, planes, 1)
                c2 = Conv(pre + "conv2.weight", planes, planes, 3, stride, dil, dil, stage=f"layer{L}")
                c3 = Conv(pre + "conv3.weight", planes, 4 * planes, 1)
                ds = Conv(pre + "downsample.0.weight", cin, 4 * planes, 1, stride) if b == 0 else None
                self.blocks.append((pre, c1, c2, c3, ds))
                cin = 4 * planes
        if self.psp:
            self.cls_conv = Conv("decoder.0.weight", 4096, 512, 3, 1, 1, 1, stage="head")
            self.cls_main = Conv("decoder.0.weight[:, :2048]", 2048, 512, 3, 1, 1, 1, stage="head")
        else:
            self.aspp = [Conv("classifier.0.convs.0.0.weight", 2048, 256, 1)]
            self.aspp += [Conv(f"classifier.0.convs.{i}.0.weight", 2048, 256, 3, 1, r, r, stage="aspp") for i, r in ((1, 12), (2, 24), (3, 36))]
            self.project = Conv("classifier.0.project.0.weight", 1280, 256, 1)
            self.head_conv = Conv("classifier.1.weight", 256, 256, 3, 1, 1, 1, stage="head")


_PLANS = {}


def _plan(arch, layers):
    if (arch, layers) not in _PLANS:
        _PLANS[(arch, layers)] = Plan(arch, layers)
    return _PLANS[(arch, layers)]


def _igemm(name, stage=""):
    return Row(name, "conv_igemm", 0, None, stage)


def _plain(name, fam):
    return Row(name, fam, 0, None, "")


def run_conv(opts, c, B, H, W, ld_in, ld_out, has_res=False):
    """net.hip run_conv: the rows one conv + BN + activation leaves in the profile."""
    if takes_winograd(opts, c, B, H, W, has_res):
        mt = wino_m(opts, H, W, c.dil)
        groups_tiles = (mt + 2) * (mt + 2) * winograd_tiles(B, H, W, c.dil, mt)
        return [Row(c.name + ".wino_in", "winograd_input", mt, None, c.stage),
                Row(c.name + ".wino_gemm", "conv_igemm", mt, 2.0 * groups_tiles * c.cin * c.cout, c.stage),
                Row(c.name + ".wino_out", "winograd_output", mt, None, c.stage)]
    if takes_fused_winograd(opts, c, B, H, W, ld_in, ld_out, has_res):
        return [Row(c.name, "wino_fused", 0, None, c.stage)]
    return [_igemm(c.name, c.stage)]


def pyramid_reduce_rows(fh, fw):
    if one_pass_pyramid(fh, fw):
        rows = [_plain("ppm.pool6+combine", "adaptive_avgpool")]
    else:
        rows = [_plain(f"ppm.pool{b}", "adaptive_avgpool") for b in BINS]
    return rows + [_plain("ppm.features.*.1.weight", "rowdot_1x1")]


def encoder_rows(plan, opts, B, H, W, fused):
    """net.hip encoder_core.  fused: the PSPNet fused-head route (the pyramid is run by the caller and never upsampled)."""
    (H1, W1), (H2, W2), (H3, W3) = geometry(plan.stem[0], H, W)
    rows = [_plain(plan.stem[0].name, "stem_conv")]
    C = plan.stem[0].cout
    pooled = False
    if plan.psp:
        s1, s2 = plan.stem[1], plan.stem[2]
        rows += run_conv(opts, s1, B, H1, W1, C, s1.cout)
        pooled = opts.use_fused_pool and takes_fused_winograd(opts, s2, B, H1, W1, s1.cout, s2.cout) and \
            H2 == (H1 - 1) // 2 + 1 and W2 == (W1 - 1) // 2 + 1
        if pooled:
            rows.append(Row(s2.name + "+maxpool", "wino_fused_pool", 0, None, "stem"))
        else:
            rows += run_conv(opts, s2, B, H1, W1, s1.cout, s2.cout)
        C = s2.cout
    if not pooled:
        rows.append(_plain("maxpool", "maxpool3x3s2"))
    curH, curW = H2, W2
    for bi, (pre, c1, c2, c3, ds) in enumerate(plan.blocks):
        last = bi == len(plan.blocks) - 1
        oH, oW = c2.out_size(curH), c2.out_size(curW)
        rows += run_conv(opts, c1, B, curH, curW, C, c1.cout)
        rows += run_conv(opts, c2, B, curH, curW, c1.cout, c2.cout)
        ld_dst = (4096 if plan.psp else 2048) if (last and not fused) else c3.cout
        if ds is not None and opts.use_fused_shortcut:
            rows.append(_igemm(pre + "conv3+downsample"))
        elif ds is not None:
            rows += run_conv(opts, ds, B, curH, curW, C, c3.cout)
            rows += run_conv(opts, c3, B, oH, oW, c2.cout, ld_dst, has_res=True)
        else:
            rows += run_conv(opts, c3, B, oH, oW, c2.cout, ld_dst, has_res=True)
        C, curH, curW = c3.cout, oH, oW
    assert (curH, curW) == (H3, W3) and C == 2048
    if plan.psp and not fused:
        rows += pyramid_reduce_rows(H3, W3)
        rows += [_plain(f"ppm.up{b}", "upsample_into") for b in BINS]
    return rows


def decoder_rows(plan, opts, B, fh, fw):
    """net.hip net_decoder."""
    if plan.psp:
        return run_conv(opts, plan.cls_conv, B, fh, fw, 4096, 512) + [_plain("decoder.4", "classifier_nchw")]
    rows = []
    for i, c in enumerate(plan.aspp):
        rows += run_conv(opts, c, B, fh, fw, 2048, 1280)
    rows += [_plain("aspp.pool", "adaptive_avgpool"), _plain("classifier.0.convs.4.1.weight", "rowdot_1x1"), _plain("aspp.up", "upsample_into")]
    rows += run_conv(opts, plan.project, B, fh, fw, 1280, 256)
    rows += run_conv(opts, plan.head_conv, B, fh, fw, 256, 256)
    return rows + [_plain("classifier.4", "classifier_nchw")]


def route_table(arch, layers, B, H, W, options=None, call="segment"):
    """The profile of one fs_segment_forward (call="encoder" / "decoder": of fs_encoder_forward / fs_decoder_forward; the decoder's
    H x W is still the FRAME's) over B frames of H x W: a list of Row."""
    plan, opts = _plan(arch, layers), Opts(options)
    if H < 33 or W < 33 or B < 1:
        raise ValueError("route_table: frames of at least 33 x 33")
    fh, fw = geometry(plan.stem[0], H, W)[2]
    if call == "encoder":
        return encoder_rows(plan, opts, B, H, W, False)
    if call == "decoder":
        return decoder_rows(plan, opts, B, fh, fw)
    if call != "segment":
        raise ValueError(f"route_table: call {call!r}")
    if not plan.psp or not opts.use_fused_head:
        return encoder_rows(plan, opts, B, H, W, False) + decoder_rows(plan, opts, B, fh, fw)
    rows = encoder_rows(plan, opts, B, H, W, True) + pyramid_reduce_rows(fh, fw)
    rows.append(_igemm("decoder.0.weight[:, ppm]"))
    rows += run_conv(opts, plan.cls_main, B, fh, fw, 2048, 512)
    return rows + [_plain("decoder.0.pyramid_term+decoder.4", "ppm_term_classify")]


# ---------------------------------------------------------------------------------------------------------------------------
# Views of a table
def keyed(rows):
    """What the GPU test compares with the profiler, launch by launch: (name, family, booked flops of a .wino_gemm row or None)."""
    return [(r.name, r.family, r.flops) for r in rows]


def observed(profile_rows):
    """HipNet.profile_dump() rows in the form of keyed()."""
    return [(name, family(label), flops if name.endswith(".wino_gemm") else None) for name, label, flops, _bytes, _ms in profile_rows]


def per_image(rows, B):
    """keyed() with the Winograd GEMM's flops divided by the batch: equal for every B when no route depends on the batch."""
    return [(r.name, r.family, r.m, None if r.flops is None else r.flops / B) for r in rows]


def _route(r):
    if r.family in ("winograd_input", "winograd_output"):
        return f"F{r.m}"
    return {"conv_igemm": "igemm", "wino_fused": "fused", "wino_fused_pool": "fused+pool"}[r.family]


def stage_routes(rows):
    """{stage: the distinct routes of its 3x3 stride-1 convs, in launch order} -- e.g. {"stem": ("fused", "fused+pool"), "layer1":
    ("igemm",), "layer2": ("F3",), ...}; plus "maxpool": present?, "pools": number of adaptive_avgpool launches.  The stride-2 conv2
    of layer2.0 has no choice (always the implicit GEMM) and is left out."""
    out = {}
    for r in rows:
        if not r.stage or r.name.endswith(".wino_gemm") or r.name.startswith(("layer2.0.", "backbone.layer2.0.")):
            continue
        got = out.setdefault(r.stage, [])
        if _route(r) not in got:
            got.append(_route(r))
    out = {k: tuple(v) for k, v in out.items()}
    out["maxpool"] = any(r.family == "maxpool3x3s2" for r in rows)
    out["pools"] = sum(r.family == "adaptive_avgpool" for r in rows)
    return out


def tile_sizes(rows):
    return frozenset(r.m for r in rows if r.m)


def regime(rows):
    """What the regime list is keyed on: stem route, layer1 route, layer2 route (igemm / winograd / fused) and the SET of Winograd tile
    sizes the forward mixes."""
    s = stage_routes(rows)
    l2 = tuple("winograd" if x.startswith("F") else x for x in s["layer2"])
    return (s.get("stem", ("igemm",)), s["layer1"], l2, tuple(sorted(tile_sizes(rows))))


def unpinned_stages(arch, layers, B, H, W, options=None):
    """The stages with a three-launch conv whose booked GEMM flops another tile size would book as well (there the profiler cannot tell
    the two apart: a 49 x 49 map at dilation 4 is 256 tiles of 4 x 4 or 144 of 6 x 6, 9216 GEMM rows either way).  Everywhere else
    the profiler's flops identify m."""
    plan = _plan(arch, layers)
    convs = {b[2].name: b[2] for b in plan.blocks}
    convs.update({c.name: c for c in ([plan.cls_conv, plan.cls_main] if plan.psp else plan.aspp[1:] + [plan.head_conv])})
    H3, W3 = geometry(plan.stem[0], H, W)[2]  # every Winograd-eligible conv runs on the stride-8 map
    out = set()
    for r in route_table(arch, layers, B, H, W, options):
        if not r.name.endswith(".wino_gemm"):
            continue
        c = convs[r.name[:-len(".wino_gemm")]]
        for m in (3, 4, 6):
            if m != r.m and 2.0 * (m + 2) * (m + 2) * winograd_tiles(B, H3, W3, c.dil, m) * c.cin * c.cout == r.flops:
                out.add(c.stage)
    return out


def decisions(arch, layers, B, H, W, options=None):
    """The route decisions alone, one per distinct (conv shape, map) of the plan: what a sweep over tens of thousands of frames can
    afford.  Each entry is the tuple of (family, m) that conv's launches get."""
    plan, opts = _plan(arch, layers), Opts(options)
    (H1, W1), (H2, W2), (H3, W3) = geometry(plan.stem[0], H, W)
    out = []
    if plan.psp:
        s1, s2 = plan.stem[1], plan.stem[2]
        out.append(run_conv(opts, s1, B, H1, W1, 64, s1.cout))
        out.append(run_conv(opts, s2, B, H1, W1, s1.cout, s2.cout))
        out.append(opts.use_fused_pool and takes_fused_winograd(opts, s2, B, H1, W1, s1.cout, s2.cout))
    seen = set()
    for _pre, _c1, c2, _c3, _ds in plan.blocks:
        if c2.stride == 1 and (c2.cin, c2.dil) not in seen:
            seen.add((c2.cin, c2.dil))
            h, w = (H2, W2) if c2.stage == "layer1" else (H3, W3)
            out.append(run_conv(opts, c2, B, h, w, c2.cin, c2.cout))
    if plan.psp:
        out += [run_conv(opts, plan.cls_main, B, H3, W3, 2048, 512), run_conv(opts, plan.cls_conv, B, H3, W3, 4096, 512)]
    else:
        out += [run_conv(opts, c, B, H3, W3, 2048, 1280) for c in plan.aspp[1:]] + [run_conv(opts, plan.head_conv, B, H3, W3, 256, 256)]
    out.append(one_pass_pyramid(H3, W3))
    return tuple(x if isinstance(x, bool) else tuple((r.family, r.m) for r in x) for x in out)
