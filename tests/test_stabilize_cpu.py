"""The temporal mask stabiliser, the parts that need no GPU: the definition in numpy (tests/stabilize_ref.py) against an independent brute
force and hand-computed sequences, what the filter is for (quality conditions on the reference alone), csrc/stabilize_defs.h run on the
CPU by a stand-alone sanitized host program, the seventh hook table, the refusals, and FlowPredictor's argument checks."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stabilize_ref as sref
import tracks_mc_ref as mc
from flood_uav_video_segmentation_amd import _lib, ops
from flood_uav_video_segmentation_amd.flow.predict import FlowPredictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "mask_stabilize"
CASES = range(len(sref.case_list()))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_the_case_list_covers_what_it_says():
    cases = sref.case_list()
    assert len(cases) == len(sref.GEOMETRIES) * len(sref.TABLES) + len(sref.RAGGED_GEOMETRIES) * len(sref.RAGGED_TABLES) == 30
    assert {c["mask"].shape[0] for c in cases} == {3, 4, 5, 6}
    assert {"garbage", "outward"} <= set(sref.TABLES) and sref.GEOMETRIES == [(48, 80, 48, 80), (37, 300, 48, 320), (96, 160, 48, 80), (50, 90, 50, 90)]
    assert {(c["mask"].shape[1] * c["mask"].shape[2]) % 4 for c in cases} == {0, 1, 2, 3} and any(c["mask"].shape[2] % 4 for c in cases[:24])
    for c in cases:
        assert (c["mask"] >= sref.K).any() and c["pair_stats"][1][2] != 0 and c["pair_stats"][0][2] == 0
    held = [sref.expected(i, 3, False, False, False)[2][:, 0].sum() for i in CASES]
    assert min(held) > 10                                                  # the scenes flicker: the filter has something to hold


@pytest.mark.parametrize("i", CASES)
def test_reference_equals_the_brute_force(i):
    """One configuration per case, cycling through the persistences and the eight on / off combinations of conf, mv and pair_stats."""
    persist, combo = sref.PERSISTS[i % 4], (i // 4 + i) % 8
    flags = (bool(combo & 1), bool(combo & 2), bool(combo & 4))
    kw = sref.case_kwargs(i, persist, *flags)
    assert same(sref.mask_stabilize_bruteforce(sref.case_list()[i]["mask"], None, **kw), sref.expected(i, persist, *flags))


def test_the_brute_force_takes_a_state_too():
    i = 1
    c = sref.case_list()[i]
    kw = sref.case_kwargs(i, 2, True, True, True)
    assert same(sref.chained(c["mask"], (1, 2, c["mask"].shape[0] - 3), sref.mask_stabilize_bruteforce, **kw), sref.expected(i, 2, True, True, True))


def seq(obs, persist, state=None, conf=None, trust=None, cuts=()):
    """One pixel through len(obs) frames -> (emitted classes, final word, counts)."""
    mask = np.array(obs, np.uint8).reshape(-1, 1, 1)
    stats = np.array([[1, 0, int(f in cuts), 0] for f in range(len(obs))], np.int32) if cuts else None
    out, st, counts = sref.mask_stabilize(mask, None if state is None else np.array([[state]], np.uint32), None if conf is None else
                                          np.array(conf, np.uint8).reshape(-1, 1, 1), 5, persist, trust, pair_stats=stats)
    return out.reshape(-1).tolist(), int(st[0, 0]), counts.tolist()


HELD, SWITCHED, SEEDED, TRUSTED, NONE = [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 0, 1], [0, 0, 0, 0]


def test_hand_computed_sequences():
    # P = 1: every observation is emitted; 7 is no class: passed through, the history ends and the next frame seeds
    assert seq([0, 1, 1, 2, 7, 2, 0, 0], 1) == ([0, 1, 1, 2, 7, 2, 0, 0], sref.pack(0, 0, 0), [SEEDED, SWITCHED, NONE, SWITCHED, NONE, SEEDED, SWITCHED, NONE])
    # P = 2: a one-frame flicker is held, the second frame running switches; coming back to e resets the run
    assert seq([0, 1, 0, 1, 1, 2, 1, 1], 2) == ([0, 0, 0, 0, 1, 1, 1, 1], sref.pack(1, 1, 0), [SEEDED, HELD, NONE, HELD, SWITCHED, HELD, NONE, NONE])
    # P = 3: a third class (2) interrupts the run of 1, which starts again at 1; the last 0 starts a run of its own
    assert seq([0, 1, 1, 2, 1, 1, 1, 0], 3) == ([0, 0, 0, 0, 0, 0, 1, 1], sref.pack(1, 0, 1), [SEEDED, HELD, HELD, HELD, HELD, HELD, SWITCHED, HELD])
    # P = 255: eight frames never switch; the run is counted
    assert seq([0, 1, 1, 1, 1, 1, 1, 1], 255) == ([0] * 8, sref.pack(0, 1, 7), [SEEDED] + [HELD] * 7)
    # the run saturates at 255, which still reaches P = 255: from r = 253 one frame is held, the next switches; r = 255 switches at once
    assert seq([1, 1], 255, state=sref.pack(0, 1, 253)) == ([0, 1], sref.pack(1, 1, 0), [HELD, SWITCHED])
    assert seq([1], 255, state=sref.pack(0, 1, 255)) == ([1], sref.pack(1, 1, 0), [SWITCHED])
    assert seq([2], 255, state=sref.pack(0, 1, 255)) == ([0], sref.pack(0, 2, 1), [HELD])
    # trust: confidence >= 200 switches at once (frames 1, 4, 7), below it the run is counted as usual
    assert seq([0, 1, 2, 2, 2, 2, 0, 0], 3, conf=[9, 255, 199, 10, 200, 0, 0, 200], trust=200) == \
        ([0, 1, 1, 1, 2, 2, 2, 0], sref.pack(0, 0, 0), [SEEDED, TRUSTED, HELD, HELD, TRUSTED, NONE, HELD, TRUSTED])
    # the same planes with trust off (256) and without a plane
    assert seq([0, 1, 2, 2, 2, 2, 0, 0], 3, conf=[9, 255, 199, 10, 200, 0, 0, 200], trust=256)[0] == [0, 0, 0, 0, 2, 2, 2, 2]
    assert seq([0, 1, 2, 2, 2, 2, 0, 0], 3)[0] == [0, 0, 0, 0, 2, 2, 2, 2]
    # cuts at frames 1 and 5: the frame seeds whatever came before
    assert seq([0, 1, 0, 0, 3, 3, 3, 3], 2, cuts=(1, 5)) == ([0, 1, 1, 0, 0, 3, 3, 3], sref.pack(3, 3, 0), [SEEDED, SEEDED, HELD, SWITCHED, HELD, SEEDED, NONE, NONE])
    # a word that is not valid is no state, whatever its low bits
    assert seq([2], 3, state=0x00010203) == ([2], sref.pack(2, 2, 0), [SEEDED])


@pytest.mark.parametrize("i", CASES)
def test_consequences_on_the_reference(i):
    c = sref.case_list()[i]
    mask, n = c["mask"], c["mask"].shape[0]
    assert np.array_equal(sref.expected(i, 1, False, True, True)[0], mask)                                  # P = 1
    assert np.array_equal(sref.mask_stabilize(mask, None, c["conf"], sref.K, 3, 0)[0], mask)                # T = 0 with a plane
    flags = (bool(i & 1), True, bool(i & 2))
    for pieces in ((1,) * n, (2, n - 2), (n - 1, 1)):
        assert same(sref.chained(mask, pieces, **sref.case_kwargs(i, 2, *flags)), sref.expected(i, 2, *flags))
    fh, fw = c["frame_size"]
    plain = sref.expected(i, 3, True, False, False)
    for table in (mc.table_void(fh, fw), mc.table_uniform(fh, fw, 0, 0)):
        assert same(sref.mask_stabilize(mask, None, c["conf"], sref.K, 3, sref.TRUST, np.stack([table] * n), (fh, fw)), plain)


# ------------------------------------------------------------------------------------------------ what the filter is for
def test_quality_conditions_on_the_reference():
    """The factors are about half of what a prototype measured (static 6648 -> 830, moving compensated 4261 -> 1493, moving in place 4261
    -> 8604), so that the seed cannot fail them."""
    clean, noisy = sref.noisy_blobs(12, (0, 0))
    out = sref.mask_stabilize(noisy, None, None, sref.K, 2)[0]
    assert sref.errors(noisy, clean) >= 4 * sref.errors(out, clean) and sref.errors(noisy, clean) > 1000
    step = mc.BLOB_SCENE["step"]
    clean, noisy = sref.noisy_blobs(8, step)
    h, w = clean.shape[1:]
    mv = np.stack([mc.table_uniform(h, w, -step[1], -step[0])] * 8)
    comp = sref.mask_stabilize(noisy, None, None, sref.K, 2, None, mv, (h, w))[0]
    assert 2 * sref.errors(comp, clean) < sref.errors(noisy, clean)
    assert sref.errors(sref.mask_stabilize(noisy, None, None, sref.K, 2)[0], clean) > sref.errors(noisy, clean)   # in place the filter lags and hurts
    assert sref.errors(sref.mask_stabilize(clean, None, None, sref.K, 2, None, mv, (h, w))[0], clean) == 0


# ------------------------------------------------------------------------------------------------ the header's functions on the CPU
def test_the_headers_transition_is_the_references_under_sanitizers(tmp_path):
    """csrc/stabilize_defs.h is plain __host__ __device__ C++: tests/stabilize_host_check.cpp prints every pixel's emitted class and state
    word through stb::step, as a stand-alone program built with -fsanitize=address,undefined; they are the reference's, line by line."""
    makefile = open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)          # the compiler the project cannot be built without
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang++")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (os.path.exists(rocm_clang) and rocm_clang)
    assert cxx, f"no host C++ compiler: none of $CXX, g++, clang++, c++ on PATH, and no {rocm_clang}"
    exe, data = str(tmp_path / "stabilize_host_check"), str(tmp_path / "cases.bin")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
            os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc"), os.path.join(ROOT, "tests", "stabilize_host_check.cpp"), "-o", exe]
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):   # the runtimes linked in where the compiler can
        build = subprocess.run(base + static, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    # every (valid, e, c, r) of interest against every observation, with and without trust, then a flickering scene at each persistence
    words = [0, 0x00010203] + [sref.pack(e, c, r) for e in (0, 3, 4) for c in (0, 3, 4, 200) for r in (0, 1, 2, 253, 254, 255)]
    obs = [0, 3, 4, 5, 200, 255]
    state = np.repeat(np.array(words, np.uint32), len(obs))
    first = np.tile(np.array(obs, np.uint8), len(words))
    grid_mask = np.stack([first, np.roll(first, 1)])
    grid_conf = np.stack([np.arange(len(first)) % 2 * 255, np.arange(len(first)) % 3 * 100]).astype(np.uint8)
    entries = [(grid_mask, grid_conf if t is not None else None, state, p, t) for p in sref.PERSISTS for t in (None, 200)]
    c = sref.case_list()[0]
    flat = c["mask"].reshape(c["mask"].shape[0], -1)
    entries += [(flat, c["conf"].reshape(flat.shape), None, p, sref.TRUST) for p in sref.PERSISTS] + [(flat, None, None, 3, None)]
    want = []
    with open(data, "wb") as fh:
        fh.write(np.int32(len(entries)).tobytes())
        for j, (mask, conf, st, p, t) in enumerate(entries):
            n, hw = mask.shape
            fh.write(np.array([n, hw, sref.K, p, 256 if t is None else t, conf is not None, st is not None], np.int32).tobytes())
            fh.write(np.ascontiguousarray(mask).tobytes())
            if conf is not None:
                fh.write(np.ascontiguousarray(conf).tobytes())
            if st is not None:
                fh.write(st.tobytes())
            want.append(f"case {j}")
            words_now = None if st is None else st.reshape(1, hw)
            for f in range(n):
                out, words_now, counts = sref.mask_stabilize(mask[f].reshape(1, 1, hw), words_now, None if conf is None else conf[f].reshape(1, 1, hw),
                                                             sref.K, p, t)
                want.append(f"frame {f}")
                want.extend(f"{o} {s:x}" for o, s in zip(out.reshape(-1).tolist(), words_now.reshape(-1).tolist()))
                want.append("counts " + " ".join(str(v) for v in counts[0].tolist()))
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert run.stdout.split("\n")[:-1] == want
    assert len(want) > 40000                                                # not vacuous


# ------------------------------------------------------------------------------------------------ library surface
def test_the_seventh_table_in_header_initialiser_and_binding():
    assert _lib.ext6_hook_names() == [NEW]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "floodseg_test.h")).read(), flags=re.S)
    body = text[text.index("typedef struct fs_ext6_api {"):text.index("} fs_ext6_api;")]
    assert re.findall(r"\(\*([a-z0-9_]+)\)\s*\(", body) == _lib.ext6_hook_names()
    assert re.findall(r"\b(uint64_t|size_t) ([a-z]+);", body) == [("uint64_t", "magic"), ("size_t", "size")]
    assert text.index("} fs_hook_tables5;") < text.index("typedef struct fs_ext6_api {") < text.index("typedef struct fs_hook_tables6 {")
    tables6 = text[text.index("typedef struct fs_hook_tables6 {"):text.index("} fs_hook_tables6;")]
    assert re.findall(r"\b(fs_[a-z0-9_]+) ([a-z0-9]+);", tables6) == [("fs_hook_tables5", "base5"), ("fs_ext6_api", "ext6")]
    assert int(re.search(r"#define FS_EXT6_MAGIC (0x[0-9a-f]+)ull", text).group(1), 16) == _lib.EXT6_MAGIC == int.from_bytes(b"FSEXTAB6", "big")
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "api_test.hip")).read())   # code, not comments
    init = src[src.index("static const fs_hook_tables6 all6 = {all5, {"):]
    init = init[:init.index("}};")]
    assert re.findall(r"^\s+(fs_[a-z0-9_]+),$", init, flags=re.M) == ["fs_" + NEW]
    assert "FS_EXT6_MAGIC," in init and "sizeof(fs_ext6_api)," in init
    assert re.search(r"static const fs_hook_tables5& hook_tables\(void\) \{.*return all6\.base5;\s+}", src, flags=re.S)   # the head of the new object
    assert "launch_mask_stabilize" in open(os.path.join(ROOT, "flood_uav_video_segmentation_amd", "csrc", "kernels.h")).read()
    # the six older tables and the export list are what they were
    assert [len(_lib.hook_names()), len(_lib.ext_hook_names()), len(_lib.ext2_hook_names()), len(_lib.ext3_hook_names()), len(_lib.ext4_hook_names()),
            len(_lib.ext5_hook_names())] == [38, 2, 14, 1, 1, 1]
    assert [ctypes.sizeof(t) for t in (_lib.FsExtApi, _lib.FsExt2Api, _lib.FsExt3Api, _lib.FsExt4Api, _lib.FsExt5Api)] == [32, 128, 24, 24, 24]
    assert "fs_" + NEW not in _lib.exported_symbols() and len(_lib.exported_symbols()) == 40
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r" T (fs_[a-z0-9_]+)", out)) == _lib.exported_symbols()
    assert NEW not in open(os.path.join(ROOT, "include", "floodseg.h")).read()
    lib = _lib.load()
    assert lib.fs_version() == 600
    assert _lib.FsHookTables6.ext6.offset == ctypes.sizeof(_lib.FsHookTables5)                           # directly behind, no padding
    assert _lib.FsExt6Api.mask_stabilize.offset == 16 and ctypes.sizeof(_lib.FsExt6Api) == 24
    all6 = ctypes.cast(lib.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables6)).contents
    assert all6.base5.ext5.magic == _lib.EXT5_MAGIC and all6.base5.ext5.size == 24
    assert all6.base5.base4.ext4.magic == _lib.EXT4_MAGIC and all6.base5.base4.base3.ext3.magic == _lib.EXT3_MAGIC
    assert all6.ext6.magic == _lib.EXT6_MAGIC and all6.ext6.size >= 24                                   # from below only: the table grows at its end
    assert ctypes.cast(all6.ext6.mask_stabilize, ctypes.c_void_p).value == ctypes.cast(lib.fs_mask_stabilize, ctypes.c_void_p).value
    assert ctypes.cast(all6.base5.ext5.frame_compose_regions, ctypes.c_void_p).value == ctypes.cast(lib.fs_frame_compose_regions, ctypes.c_void_p).value
    with pytest.raises(AttributeError):
        getattr(ctypes.CDLL(_lib.LIB_PATH), "fs_" + NEW)                                                 # a table member, not an exported symbol
    macro = re.search(r"#define FS_MASK_STABILIZE_WORKSPACE_BYTES\(n, H, W, hb, wb\) \\\n(.*)", text).group(1)
    for n, h, w, hb, wb in ((1, 1, 1, 1, 1), (5, 1072, 1920, 67, 120), (3, 37, 300, 3, 20), (6, 50, 90, 3, 5), (4, 33, 47, 0, 0), (2, 7, 9, 2, 0), (65535, 3, 5, 1, 2)):
        got = eval(macro.replace("(size_t)", "").replace("/", "//"), dict(n=n, H=h, W=w, hb=hb, wb=wb))
        assert got == ops.mask_stabilize_workspace_bytes(n, h, w, hb, wb) == sref.workspace_bytes(n, h, w, hb, wb) and got % 16 == 0
        assert (got == 0) == (hb * wb == 0) and (got == 0 or got >= 4 * h * w + 4 * n * (hb * wb + 1))


def test_the_magic_is_checked_before_use(monkeypatch):
    """A binding that expects another magic finds no seventh table in this library and says so, instead of calling through it."""
    fresh = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    fresh._cdll.fs_test_hooks.restype = ctypes.c_void_p
    monkeypatch.setattr(_lib, "EXT6_MAGIC", _lib.EXT6_MAGIC + 1)
    with pytest.raises(RuntimeError, match="sixth extension table"):
        fresh.fs_mask_stabilize
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "EXT5_MAGIC", _lib.EXT5_MAGIC + 1)
    with pytest.raises(RuntimeError, match="first six hook tables"):
        fresh.fs_mask_stabilize
    monkeypatch.undo()
    assert fresh.fs_mask_stabilize is not None and fresh.fs_frame_compose_regions is not None


def test_library_refuses_bad_arguments_before_a_launch():
    """Dummy non-null pointers: every one of these must fail in argument validation (there is no GPU here to launch on)."""
    lib = _lib.load()
    assert len(sref.refusal_cases()) >= 27
    for kw, word in sref.refusal_cases():
        assert sref.call_stabilize(lib, **kw) != 0, kw
        msg = lib.fs_last_error()
        assert msg.startswith(b"mask_stabilize:") and word in msg, (kw, msg)


# ------------------------------------------------------------------------------------------------ Python argument checks
def test_op_refuses_with_the_packages_message_before_the_library_is_asked():
    mask = torch.zeros((2, 4, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="floodseg.mask_stabilize: tensors must live on the GPU"):
        ops.mask_stabilize(mask)
    assert ops.mask_stabilize_workspace_bytes(5, 1072, 1920) == 0
    assert ops.mask_stabilize_workspace_bytes(5, 1072, 1920, 67, 120) == 1072 * 1920 * 4 + (5 * 8041 + 3) // 4 * 16


def test_predictor_argument_checks():
    ident = torch.nn.Identity()
    for off in (None, 0, 1):
        p = FlowPredictor(ident, stabilize=off)
        assert p.stabilize == 0 and p.stabilize_report().shape == (0, 4) and p.stabilize_report().dtype == np.int64
    assert FlowPredictor(ident).stabilize == 0
    assert FlowPredictor(ident, stabilize=3).stabilize == 3
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="stabilize must be"):
            FlowPredictor(ident, stabilize=bad)
    with pytest.raises(ValueError, match="stabilize_trust needs confidence=True"):
        FlowPredictor(ident, stabilize=3, stabilize_trust=200)
    with pytest.raises(ValueError, match="stabilize_trust must be 0..256"):
        FlowPredictor(ident, stabilize=3, stabilize_trust=257, confidence=True)
    with pytest.raises(ValueError, match="need stabilize"):
        FlowPredictor(ident, stabilize_trust=200, confidence=True)
    with pytest.raises(ValueError, match="need stabilize"):
        FlowPredictor(ident, stabilize_compensate=True)
    p = FlowPredictor(ident, stabilize=2, stabilize_compensate=True)
    with pytest.raises(ValueError, match="stabilize_compensate=True needs link_mvs"):
        p._link_inputs(3, None, None, None)
    mvs = torch.zeros((3, 15, 7), dtype=torch.int32)
    assert p._link_inputs(3, mvs, (48, 80), None)[1] == (48, 80)
    assert p._track_link(p._link_inputs(3, mvs, (48, 80), None)) is None     # the tracks of this predictor are not compensated
    both = FlowPredictor(ident, regions=True, track=True, compensate=True, stabilize=2)
    with pytest.raises(ValueError, match="compensate=True needs link_mvs"):
        both._link_inputs(3, None, None, None)
    assert both._track_link("x") == "x"
    with pytest.raises(ValueError, match="link_mvs must be"):
        p._link_inputs(2, mvs, (48, 80), None)
