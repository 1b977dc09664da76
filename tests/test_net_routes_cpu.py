"""The restated conv-route dispatch (tests/net_routes_ref.py) on its own, no GPU: anchors the code's comments give, the promise that a
frame's routes do not depend on the batch, and the list of regimes the dispatch has -- each of which tests/test_gpu_net_routes.py
must run against the oracle.  A threshold moved in csrc/net.hip or csrc/kernels.h is followed in net_routes_ref.py (the GPU test
fails until it is), and then THIS file fails until the GPU test's frame list covers the regimes the move created."""
import net_routes_ref as R
from net_routes_ref import route_table, stage_routes

SIZES = range(33, 1301, 8)  # the frames the networks take: (H - 1) % 8 == 0, at least 33 px
BATCHES = (2, 3, 5, 8)


def routes(arch, H, W, B=1, **options):
    return stage_routes(route_table(arch, 50, B, H, W, options))


def test_geometry_and_tile_counts_the_sources_state():
    """Figures csrc/ states in its own comments, so that the restatement is held to something other than itself."""
    plan = R.Plan("pspnet", 50)
    assert R.geometry(plan.stem[0], 713, 713) == ((357, 357), (179, 179), (90, 90))          # net.hip: "the 357 x 357 x 128 map"
    assert R.geometry(plan.stem[0], 1072, 1920) == ((536, 960), (268, 480), (134, 240))      # test_gpu_net: stem 536x960, map 134x240
    assert R.geometry(R.Plan("deeplabv3", 50).stem[0], 257, 257)[2] == (33, 33)
    assert R.winograd_tiles(1, 90, 90, 1, 6) == 15 * 15 and R.winograd_tiles(1, 90, 90, 1, 4) == 23 * 23  # kernels.h winograd_pick_m
    assert R.cdiv(90, 4) ** 2 == 529                                                          # net.hip: "529 tiles per image"
    assert R.winograd_tiles(2, 33, 33, 12, 3) == 2 * 144                                      # 144 phases of 3 x 3 pixels
    assert R.winograd_pick_m(90, 90, 1) == 6 and R.winograd_pick_m(90, 90, 36) == 3           # kernels.h, round 6
    assert R.winograd_gemm_rows(1, 90, 90, 1, 6) == 64.0 * 256                                # 225 tiles round up to 256 rows


def test_anchor_713_is_fused_stem_fused_layer1_f6_everywhere_one_pass_pyramid():
    for b in (1, 2):
        t = route_table("pspnet", 50, b, 713, 713)
        assert stage_routes(t) == dict(stem=("fused", "fused+pool"), layer1=("fused",), layer2=("F6",), layer3=("F6",), layer4=("F6",),
                                       head=("F6",), maxpool=False, pools=1)
        names = [r.name for r in t]
        assert names[:3] == ["layer0.0.weight", "layer0.3.weight", "layer0.6.weight+maxpool"] and "maxpool" not in names
        assert [r.name for r in t if r.family == "adaptive_avgpool"] == ["ppm.pool6+combine"]
        assert names[-5:] == ["decoder.0.weight[:, ppm]", "decoder.0.weight[:, :2048].wino_in", "decoder.0.weight[:, :2048].wino_gemm",
                              "decoder.0.weight[:, :2048].wino_out", "decoder.0.pyramid_term+decoder.4"]
        # 3 stem rows, 16 blocks of 3 launches, 2 more per three-launch Winograd conv (12 of them), pool + reduce, Z GEMM, head (3), tail
        assert len(t) == 3 + 16 * 3 + 12 * 2 + 2 + 1 + 3 + 1
        gemm = {r.name: r.flops for r in t if r.flops is not None}
        assert gemm["layer3.0.conv2.weight.wino_gemm"] == 2.0 * 64 * (b * 4 * 8 * 8) * 256 * 256  # 45 x 45 lattices: 8 x 8 tiles of 6 x 6
        assert gemm["decoder.0.weight[:, :2048].wino_gemm"] == 2.0 * 64 * (b * 225) * 2048 * 512


def test_anchor_65_is_all_direct_with_f3():
    t = route_table("pspnet", 50, 2, 65, 65)
    s = stage_routes(t)
    assert s["stem"] == ("igemm",) and s["layer1"] == ("igemm",) and s["maxpool"] and s["pools"] == 4
    assert R.tile_sizes(t) == {3}
    assert all(set(s[k]) <= {"igemm", "F3"} for k in ("layer2", "layer3", "layer4", "head"))
    assert [r.name for r in t if r.family == "adaptive_avgpool"] == ["ppm.pool1", "ppm.pool2", "ppm.pool3", "ppm.pool6"]


def test_what_the_suite_and_the_sources_say_about_other_frames():
    # 97 x 97 and 97 x 130 drop layer4 to the direct kernel; the small maps that are multiples of six pool in one pass
    assert routes("pspnet", 97, 97)["layer4"] == ("igemm",) and routes("pspnet", 97, 130, B=3)["layer4"] == ("igemm",)
    assert routes("pspnet", 41, 89)["pools"] == 1 and routes("pspnet", 89, 137)["pools"] == 1
    # tests/test_gpu_fullsize.py: 129 x 161 and 65 x 65 keep the max-pool launch, 257 x 323 and 713 x 713 fuse it
    assert routes("pspnet", 129, 161)["maxpool"] and routes("pspnet", 65, 65)["maxpool"]
    assert not routes("pspnet", 257, 323, B=3)["maxpool"] and not routes("pspnet", 713, 713)["maxpool"]
    # the full-HD frame takes the one-kernel Winograd on layer2's 128-channel convs (134 x 240 map: 34 * 60 = 2040 tiles)
    assert routes("pspnet", 1072, 1920)["layer2"] == ("fused",)
    # tests/test_gpu_net.py: DeepLabv3 at 257 px has dilation 12 on the lattice path, 24 and 36 direct; at 713 px all three take it
    t = {r.name: r for r in route_table("deeplabv3", 50, 1, 257, 257)}
    assert "classifier.0.convs.1.0.weight.wino_in" in t and "classifier.0.convs.2.0.weight" in t and "classifier.0.convs.3.0.weight" in t
    assert "igemm" not in routes("deeplabv3", 713, 713)["aspp"]
    assert "stem" not in routes("deeplabv3", 713, 713) and routes("deeplabv3", 713, 713)["maxpool"]  # the 7 x 7 stem has one route


def test_options_switch_the_routes_off():
    assert R.tile_sizes(route_table("pspnet", 50, 1, 713, 713, dict(hip_no_winograd=True))) == set()
    assert {r.family for r in route_table("pspnet", 50, 1, 713, 713, dict(hip_no_winograd=True))} == \
        {"stem_conv", "conv_igemm", "maxpool3x3s2", "adaptive_avgpool", "rowdot_1x1", "ppm_term_classify"}
    for m in (3, 4, 6):
        assert R.tile_sizes(route_table("pspnet", 50, 1, 713, 713, dict(hip_winograd_tile=m))) == {m}
    s = routes("pspnet", 713, 713, hip_no_fused_pool=True)
    assert s["stem"] == ("fused",) and s["maxpool"]
    s = routes("pspnet", 1217, 1217, hip_no_fused_winograd=True)
    assert s["stem"] == ("igemm",) and s["layer1"] == ("igemm",) and s["layer2"] == ("F6",) and s["maxpool"]
    names = [r.name for r in route_table("pspnet", 50, 1, 65, 65, dict(hip_no_fused_head=True, hip_no_fused_shortcut=True))]
    assert names[-2:] == ["decoder.0.weight.wino_out", "decoder.4"] and "decoder.0.weight[:, ppm]" not in names
    assert "layer1.0.downsample.0.weight" in names and "layer1.0.conv3+downsample" not in names and "ppm.up6" in names


def test_a_frames_routes_do_not_depend_on_the_batch():
    """net.hip: "a frame's result must not depend on the batch it is computed in".  The ratio rule of takes_winograd multiplies both
    sides by B in doubles, so an exact tie (36 * tiles == 0.8 * 9 * pixels) is where a batch could flip a route.  Frames
    (8i + 1) x (8j + 1) of 33..1297 px, B = 2, 3, 5, 8 against B = 1, both networks: every height, with every third width from it
    upwards (H <= W: every rule is symmetric in the two sides; the first width shifts with the row, so all widths occur) on the
    decisions alone, one per distinct conv shape -- 4300 frames in about 3 s -- and the whole table along the diagonal."""
    flipped = []
    for arch in ("pspnet", "deeplabv3"):
        for i, h in enumerate(SIZES):
            for w in range(h + 8 * (i % 3), 1301, 24):
                one = R.decisions(arch, 50, 1, h, w)
                flipped += [(arch, h, w, b) for b in BATCHES if R.decisions(arch, 50, b, h, w) != one]
    assert not flipped, flipped[:10]
    for arch in ("pspnet", "deeplabv3"):
        for h in SIZES:
            one = R.per_image(route_table(arch, 50, 1, h, h), 1)
            assert all(R.per_image(route_table(arch, 50, b, h, h), b) == one for b in BATCHES), (arch, h)
    assert R.decisions("pspnet", 50, 2, 89, 137) == R.decisions("pspnet", 50, 2, 137, 89)


def test_decisions_agree_with_the_table():
    for arch, frames in (("pspnet", R.PSPNET_FRAMES), ("deeplabv3", R.DEEPLAB_FRAMES)):
        for h, w, b in frames:
            t = route_table(arch, 50, b, h, w)
            d = {x for dec in R.decisions(arch, 50, b, h, w) if not isinstance(dec, bool) for x in dec if x[0] != "conv_igemm" or x[1]}
            in_table = {(r.family.replace("_pool", ""), r.m) for r in t if r.stage and (r.family != "conv_igemm" or r.m)}
            # the decoder's own head conv (fs_decoder_forward) is decided too, and is not a launch of fs_segment_forward
            assert in_table <= d and d - in_table <= {(r.family, r.m) for r in route_table(arch, 50, b, h, w, call="decoder")}


def test_the_gpu_frames_cover_every_regime_of_the_dispatch():
    """Every distinct (stem route, layer1 route, layer2 route, set of Winograd tile sizes) that a square frame of 33..1297 px takes
    has a frame in the GPU test's list."""
    seen = {}
    for h in SIZES:
        seen.setdefault(R.regime(route_table("pspnet", 50, 1, h, h)), []).append(h)
    covered = {R.regime(route_table("pspnet", 50, b, h, w)) for h, w, b in R.PSPNET_FRAMES}
    missing = {k: v[:4] for k, v in seen.items() if k not in covered}
    assert not missing, f"regimes without a frame in net_routes_ref.PSPNET_FRAMES (first sizes that take them): {missing}"
    assert len(seen) == 9  # the count this list was written for: a new regime is a new row in DESIGN.md's table as well
    for h, w, _ in R.PSPNET_FRAMES + R.DEEPLAB_FRAMES:
        assert (h - 1) % 8 == 0 and (w - 1) % 8 == 0
    assert R.BIG_FRAME == R.PSPNET_FRAMES[-1][:2]


def test_the_listed_frames_take_the_regimes_they_are_listed_for():
    want = {
        (49, 49): ("igemm", "igemm", "F3", "igemm", "igemm", "F3"),
        (169, 169): ("igemm", "igemm", "F3", "F3", "F3", "F3"),
        (177, 177): ("fused+pool", "igemm", "F3", "F3", "F3", "F3"),
        (185, 233): ("fused+pool", "igemm", "F4", "F4", "F4", "F4"),
        (257, 257): ("fused+pool", "igemm", "F3", "F6", "F6", "F3"),
        (345, 345): ("fused+pool", "igemm", "F6", "F6", "F6", "F6"),
        (353, 353): ("fused+pool", "fused", "F6", "F6", "F6", "F6"),
        (385, 385): ("fused+pool", "fused", "F4", "F6", "F4", "F4"),
        (625, 625): ("fused+pool", "fused", "F4", "F4", "F4", "F4"),
        (1217, 1217): ("fused+pool", "fused", "fused", "F6", "F6", "F6"),
    }
    assert {f[:2] for f in R.PSPNET_FRAMES} == set(want)
    for h, w, b in R.PSPNET_FRAMES:
        for bb in (b, b + 1):
            s = routes("pspnet", h, w, B=bb)
            got = (s["stem"][-1],) + tuple(s[k][0] for k in ("layer1", "layer2", "layer3", "layer4", "head"))
            assert got == want[(h, w)] and all(len(s[k]) == 1 for k in ("layer1", "layer2", "layer3", "layer4", "head")), (h, w, s)
            assert s["maxpool"] == (want[(h, w)][0] == "igemm") and s["pools"] == (1 if (h, w) == (185, 233) else 4)
    # the thresholds they straddle, one 8 px step apart
    assert routes("pspnet", 169, 169)["stem"] == ("igemm",) and routes("pspnet", 177, 177)["stem"] == ("fused", "fused+pool")
    assert routes("pspnet", 345, 345)["layer1"] == ("igemm",) and routes("pspnet", 353, 353)["layer1"] == ("fused",)
    assert routes("pspnet", 1209, 1209)["layer2"] == ("F6",) and routes("pspnet", 1217, 1217)["layer2"] == ("fused",)


def test_the_deeplab_frames_are_the_smallest_of_their_kind():
    def all_direct(h):
        return routes("deeplabv3", h, h)["aspp"] == ("igemm",)

    def lattice_and_fused_layer1(h):
        s = routes("deeplabv3", h, h)
        return any(x.startswith("F") for x in s["aspp"]) and s["layer1"] == ("fused",)

    assert next(h for h in SIZES if all_direct(h)) == R.DEEPLAB_FRAMES[0][0] == R.DEEPLAB_FRAMES[0][1]
    assert next(h for h in SIZES if lattice_and_fused_layer1(h)) == R.DEEPLAB_FRAMES[1][0] == R.DEEPLAB_FRAMES[1][1]
    s = routes("deeplabv3", 353, 353)
    assert s["aspp"] == ("F4", "igemm") and s["layer2"] == s["layer3"] == s["layer4"] == s["head"] == ("F6",)


def test_the_profilers_flops_identify_the_tile_size_at_the_listed_frames():
    """The profiler prints no tile size; the GPU test reads it off the booked flops of the Winograd GEMM.  That works wherever no
    other tile size books the same number -- everywhere on the list but layer4 at 385 px (49 x 49 map, dilation 4: 256 tiles of
    4 x 4 and 144 of 6 x 6 are 9216 GEMM rows each; F4 is pinned by layer2 and the head there, F6 by layer3)."""
    for arch, frames in (("pspnet", R.PSPNET_FRAMES), ("deeplabv3", R.DEEPLAB_FRAMES)):
        for h, w, b in frames:
            for bb in (b, b + 1):
                assert R.unpinned_stages(arch, 50, bb, h, w) == ({"layer4"} if (arch, h) == ("pspnet", 385) else set()), (arch, h, w, bb)


def test_family_folds_the_profilers_labels():
    for label in ("igemm128x128", "igemm64x64", "split128x64", "split64x128", "split128x128cat", "igemm128x64cat", "split128x96"):
        assert R.family(label) == "conv_igemm"
    assert R.family("stem_conv_split") == R.family("stem_conv") == "stem_conv"
    for label in ("winograd_input", "winograd_output", "wino_fused", "wino_fused_pool", "maxpool3x3s2", "adaptive_avgpool"):
        assert R.family(label) == label
    rows = [("layer3.0.conv2.weight.wino_gemm", "split128x128", 1e9, 2e6, 0.1), ("maxpool", "maxpool3x3s2", 0.0, 1e6, 0.01)]
    assert R.observed(rows) == [("layer3.0.conv2.weight.wino_gemm", "conv_igemm", 1e9), ("maxpool", "maxpool3x3s2", None)]
