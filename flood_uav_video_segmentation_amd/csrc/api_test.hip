// Op-level test hooks (include/floodseg_test.h): the building blocks behind the networks, reachable for the parity tests and the
// measurement tools through ONE exported symbol, fs_test_hooks(), that returns a table of function pointers -- they are not part of the
// product's symbol surface (include/floodseg.h).
#include "../../include/floodseg_test.h"
#include "kernels.h"
#include "net.h"

#include <algorithm>
#include <cmath>

#define FS_API extern "C" __attribute__((visibility("default")))

static inline hipStream_t S(fs_stream s) { return reinterpret_cast<hipStream_t>(s); }

static int fs_pack_conv_weight(const float* oihw, float* ohwi, int O, int I, int KH, int KW, fs_stream stream) {
    if (!oihw || !ohwi || O < 1 || I < 1 || KH < 1 || KW < 1) return fs::fail("fs_pack_conv_weight: bad arguments");
    return fs::launch_pack_oihw_to_ohwi(oihw, ohwi, O, I, KH, KW, S(stream));
}
static int conv2d_entry(const float* in, int ld_in, const float* wgt_ohwi, const void* wgt3, const float* scale, const float* shift,
                        const float* res, int ld_res, float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int KH,
                        int KW, int stride, int pad, int dil, int relu, int tile, fs_stream stream) {
    if (!in || (!wgt_ohwi && !wgt3) || !out || B < 1 || H < 1 || W < 1 || stride < 1 || dil < 1 || pad < 0)
        return fs::fail("fs_conv2d_nhwc: bad arguments");
    const int tid = tile & ~FS_CONV_CHUNK_MAJOR;
    fs::ConvParams p = fs::conv2d_params(in, ld_in, wgt_ohwi, scale, shift, res, ld_res, out, ld_out, B, H, W, Cin, Cout, KH, KW, stride, pad, dil, relu,
                                         (tile & FS_CONV_CHUNK_MAJOR) ? 1 : 0);
    fs::attach_planes(p, wgt3, (size_t)Cout * KH * KW * Cin);
    if (p.Ho < 1 || p.Wo < 1) return fs::fail("fs_conv2d_nhwc: empty output");
    // tile = workgroup tile id 0..4 or 6 (6: split route only), optionally | FS_CONV_CHUNK_MAJOR; anything else is refused (no hidden experiment bits)
    if (tid < 0 || tid > 6 || tid == 5) return fs::fail("fs_conv2d_nhwc: tile must be 0..4 or 6, optionally | FS_CONV_CHUNK_MAJOR (got 0x%x)", tile);
    return fs::launch_conv_igemm(p, S(stream), tid);
}
static int fs_conv2d_nhwc(const float* in, int ld_in, const float* wgt_ohwi, const float* scale, const float* shift,
                          const float* res, int ld_res, float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int KH,
                          int KW, int stride, int pad, int dil, int relu, int tile, fs_stream stream) {
    return conv2d_entry(in, ld_in, wgt_ohwi, nullptr, scale, shift, res, ld_res, out, ld_out, B, H, W, Cin, Cout, KH, KW, stride, pad, dil, relu,
                        tile, stream);
}
static int fs_split_bf16x3(const float* w, int64_t n, void* planes, fs_stream stream) { return fs::launch_split_bf16x3(w, n, planes, S(stream)); }
static int fs_conv2d_nhwc_split(const float* in, int ld_in, const void* wgt_planes, const float* scale, const float* shift,
                                const float* res, int ld_res, float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int KH,
                                int KW, int stride, int pad, int dil, int relu, int tile, fs_stream stream) {
    if (!wgt_planes) return fs::fail("fs_conv2d_nhwc_split: bad arguments");
    return conv2d_entry(in, ld_in, nullptr, wgt_planes, scale, shift, res, ld_res, out, ld_out, B, H, W, Cin, Cout, KH, KW, stride, pad, dil,
                        relu, tile, stream);
}
static size_t fs_attention_workspace_floats(int B, int N, int heads, int split_operands) {
    if (B < 1 || N < 1 || heads < 1) return 0;
    return fs::attention_scratch_floats(B, N, heads) + (split_operands ? fs::attention_split_floats(B, N, heads) + 64 : 0) + 64;
}
static int fs_attention(const float* qkv, float* out, int B, int N, int heads, float scale, int split_operands, float* workspace, fs_stream stream) {
    if (!qkv || !out || !workspace || B < 1 || N < 1 || heads < 1 || split_operands < 0 || split_operands > 1) return fs::fail("fs_attention: bad arguments");
    const size_t sc = fs::attention_scratch_floats(B, N, heads);
    float* scratch = sc ? workspace : nullptr;
    if (!split_operands) return fs::launch_attention_f32(qkv, out, B, N, heads, scale, scratch, S(stream));
    float* planes = workspace + sc;
    planes += (64 - ((uintptr_t)planes / 4) % 64) % 64;  // 256-B aligned
    return fs::launch_attention_split(qkv, out, B, N, heads, scale, scratch, planes, S(stream));
}
static size_t bank_floats(int mt, int Cin, int Cout) { return (size_t)(mt + 2) * (mt + 2) * Cout * Cin; }  // U [(mt+2)^2][Cout][Cin]
static size_t fs_winograd_workspace_floats(int B, int H, int W, int Cin, int Cout, int dil, int tile_m) {
    if (B < 1 || H < 1 || W < 1 || dil < 1 || !(tile_m == 0 || tile_m == 3 || tile_m == 4 || tile_m == 6)) return 0;
    const int mt = fs::wino_m(tile_m, H, W, dil);
    return fs::wino_vm_floats(mt, (size_t)fs::winograd_tiles(B, H, W, dil, mt), Cin, Cout, 1) + bank_floats(mt, Cin, Cout);
}
static int fs_conv3x3_winograd_nhwc(const float* in, int ld_in, const float* wgt_oihw, const float* scale, const float* shift,
                                    float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int dil, int relu, int tile_m,
                                    float* workspace, fs_stream stream) {
    if (!in || !wgt_oihw || !out || !workspace || B < 1 || H < 1 || W < 1 || dil < 1 || Cin % 32 != 0 || Cout % 4 != 0 ||
        !(tile_m == 0 || tile_m == 3 || tile_m == 4 || tile_m == 6))
        return fs::fail("fs_conv3x3_winograd_nhwc: bad arguments (Cin %% 32, Cout %% 4, tile_m in {0, 3, 4, 6} required)");
    // workspace: the transformed bank U, then V and M back to back; fp32-MFMA GEMM (no planes)
    const int mt = fs::wino_m(tile_m, H, W, dil);
    float* U = workspace;
    float* V = U + bank_floats(mt, Cin, Cout);
    float* M = V + fs::wino_v_floats(mt, (size_t)fs::winograd_tiles(B, H, W, dil, mt), Cin, 1);
    if (int rc = fs::launch_winograd_filter(wgt_oihw, U, Cout, Cin, mt, S(stream))) return rc;
    return fs::conv_winograd(nullptr, "", in, ld_in, U, nullptr, 0, V, M, scale, shift, out, ld_out, B, H, W, Cin, Cout, dil, relu, mt, S(stream));
}
static size_t fs_winograd_fused_workspace_floats(int Cin, int Cout) { return fs::wino_fused_bank_floats(Cin, Cout); }
static int fs_conv3x3_winograd_fused_nhwc(const float* in, int ld_in, const float* wgt_oihw, const float* scale, const float* shift,
                                          float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int relu, int variant,
                                          float* workspace, fs_stream stream) {
    if (!in || !wgt_oihw || !out || !workspace || B < 1 || H < 1 || W < 1 || !(variant == 0 || variant == 2 || variant == 3) ||
        !fs::wino_fused_supported(Cin, Cout, 3, 3, 1, 1, 1))
        return fs::fail("fs_conv3x3_winograd_fused_nhwc: bad arguments (Cin %% 32 == 0, 32 <= Cin <= 256, Cout %% 64 == 0, variant 0, 2 or 3)");
    if (int rc = fs::launch_wino4_filter_packed(wgt_oihw, workspace, Cout, Cin, S(stream))) return rc;
    return fs::launch_wino4_fused(in, ld_in, workspace, scale, shift, out, ld_out, B, H, W, Cin, Cout, relu, S(stream), variant);
}
static int fs_conv3x3_winograd_fused_pool_nhwc(const float* in, int ld_in, const float* wgt_oihw, const float* scale, const float* shift, float* pool,
                                               int B, int H, int W, int Cin, int Cout, float* workspace, fs_stream stream) {
    if (!in || !wgt_oihw || !pool || !workspace || B < 1 || H < 1 || W < 1 || !fs::wino_fused_supported(Cin, Cout, 3, 3, 1, 1, 1))
        return fs::fail("fs_conv3x3_winograd_fused_pool_nhwc: bad arguments (Cin %% 32 == 0, 32 <= Cin <= 256, Cout %% 64 == 0)");
    if (int rc = fs::launch_wino4_filter_packed(wgt_oihw, workspace, Cout, Cin, S(stream))) return rc;
    return fs::launch_wino4_fused_pool(in, ld_in, workspace, scale, shift, pool, Cout, B, H, W, Cin, Cout, S(stream));
}
static int stem_entry(const float* in_nchw, const float* wgt_hwio, const float* scale, const float* shift, float* out_nhwc, int B, int H, int W, int Cout,
                      int KH, int KW, int stride, int pad, int split, fs_stream stream);
static int fs_stem_conv_nchw(const float* in_nchw, const float* wgt_hwio, const float* scale, const float* shift,
                             float* out_nhwc, int B, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                             fs_stream stream) {
    return stem_entry(in_nchw, wgt_hwio, scale, shift, out_nhwc, B, H, W, Cout, KH, KW, stride, pad, 0, stream);
}
static int fs_stem_conv_nchw_split(const float* in_nchw, const float* wgt_hwio, const float* scale, const float* shift,
                                   float* out_nhwc, int B, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                                   fs_stream stream) {
    return stem_entry(in_nchw, wgt_hwio, scale, shift, out_nhwc, B, H, W, Cout, KH, KW, stride, pad, 1, stream);
}
static int stem_entry(const float* in_nchw, const float* wgt_hwio, const float* scale, const float* shift, float* out_nhwc, int B, int H, int W, int Cout,
                      int KH, int KW, int stride, int pad, int split, fs_stream stream) {
    if (!in_nchw || !wgt_hwio || !scale || !shift || !out_nhwc || B < 1) return fs::fail("fs_stem_conv_nchw: bad arguments");
    const fs::StemParams p = fs::stem_params(fs::frames_plain(in_nchw, nullptr, B), wgt_hwio, scale, shift, out_nhwc, B, H, W, Cout, KH, KW, stride, pad, split);
    return fs::launch_stem_conv(p, S(stream));
}
static int fs_maxpool3x3s2_nhwc(const float* in, float* out, int B, int H, int W, int C, fs_stream stream) {
    if (!in || !out || B < 1 || H < 1 || W < 1) return fs::fail("fs_maxpool3x3s2_nhwc: bad arguments");
    return fs::launch_maxpool3x3s2(in, C, out, C, B, H, W, C, fs::conv_out_size(H, 3, 2, 1, 1), fs::conv_out_size(W, 3, 2, 1, 1), S(stream));
}
static int fs_adaptive_avgpool_nhwc(const float* in, int ld_in, float* out, int B, int H, int W, int C, int bin, fs_stream stream) {
    if (!in || !out || B < 1 || H < 1 || W < 1 || bin < 1) return fs::fail("fs_adaptive_avgpool_nhwc: bad arguments");
    return fs::launch_adaptive_avgpool(in, ld_in, out, B, H, W, C, bin, S(stream));
}
static int fs_nchw_to_nhwc(const float* in, float* out, int B, int C, int HW, fs_stream stream) {
    if (!in || !out || B < 1 || C < 1 || HW < 1) return fs::fail("fs_nchw_to_nhwc: bad arguments");
    return fs::launch_nchw_to_nhwc(in, out, C, B, C, HW, S(stream));
}
static int fs_nhwc_to_nchw(const float* in, float* out, int B, int C, int HW, fs_stream stream) {
    if (!in || !out || B < 1 || C < 1 || HW < 1) return fs::fail("fs_nhwc_to_nchw: bad arguments");
    return fs::launch_nhwc_to_nchw(in, C, out, B, C, HW, S(stream));
}

// ---- Segmenter pieces: the launchers and the Linear geometry builders the network runs (vit_net.hip), nothing restated here
static int fs_layernorm(const float* in, const float* gamma, const float* beta, float* out, int rows, int D, int rows_per_batch, int drop_first,
                        fs_stream stream) {
    if (!in || !gamma || !beta || !out || rows < 1 || (drop_first && (rows_per_batch < 1 || rows % rows_per_batch != 0)))
        return fs::fail("fs_layernorm: bad arguments");
    return fs::launch_layernorm(in, gamma, beta, out, rows, D, rows_per_batch, drop_first, S(stream));
}
static int fs_linear_splits(int K, int N, int rows_per_image, int act, int split_route) {
    if (K < 1 || N < 1 || rows_per_image < 1) return 0;
    return fs::linear_splits(K, N, rows_per_image, act, split_route != 0);
}
static int fs_linear(const float* in, const float* w, const void* w_planes, const float* bias, const float* res, float* out, int rows, int K,
                     int N, int act, int nsplit, int rows_per_image, float* part, const float* gamma, const float* beta, float* ln_out,
                     fs_stream stream) {
    if (!in || !w || !out || rows < 1 || K < 1 || N < 1 || act < 0 || act > 2 || nsplit < 0 || nsplit > 16 || rows_per_image < 0)
        return fs::fail("fs_linear: bad arguments");
    const bool ln = gamma || beta || ln_out;
    if (ln && !(gamma && beta && ln_out)) return fs::fail("fs_linear: the LayerNorm merge needs gamma, beta and ln_out");
    int split = 0;
    if (nsplit == 0) split = part ? fs::linear_splits(K, N, rows_per_image ? rows_per_image : rows, act, w_planes != nullptr) : 0;
    else if (nsplit >= 2) {
        if (!part || act != 0 || K % (32 * nsplit) != 0)
            return fs::fail("fs_linear: a forced split-K needs `part`, act 0 and K %% (32 * nsplit) == 0 (K %d, nsplit %d, act %d)", K, nsplit, act);
        split = nsplit;
    }
    if (ln && !split) return fs::fail("fs_linear: the LayerNorm merge runs on split-K launches only");
    if (split) {
        fs::ConvParams p = fs::linear_splitk_params(in, w, part, rows, K, N, split);
        fs::attach_planes(p, w_planes, (size_t)N * K);
        if (int rc = fs::launch_conv_igemm(p, S(stream))) return rc;
        if (ln) return fs::launch_splitk_combine_ln(part, split, bias, res, out, gamma, beta, ln_out, rows, N, S(stream));
        return fs::launch_splitk_combine(part, split, bias, res, out, rows, N, S(stream));
    }
    fs::ConvParams p = fs::linear_params(in, w, bias, res, out, rows, K, N, act, res != nullptr);
    fs::attach_planes(p, w_planes, (size_t)N * K);
    return fs::launch_conv_igemm(p, S(stream));
}
static size_t fs_qkv_attention_workspace_floats(int B, int tokens, int D) {
    if (B < 1 || tokens < 1 || D < 64 || D % 64 != 0) return 0;
    return fs::attention_split_floats(B, tokens, D / 64) + fs::attention_scratch_floats(B, tokens, D / 64);
}
static int fs_qkv_attention(const float* in, const float* w, const void* w_planes, const float* bias, int B, int tokens, int D, float* qkv_out,
                            float* att_out, int fused, float* workspace, fs_stream stream) {
    if (!in || !w || !w_planes || !qkv_out || !att_out || !workspace || B < 1 || tokens < 1 || D < 64 || D % 64 != 0 || fused < 0 || fused > 1 ||
        ((uintptr_t)workspace & 15) != 0)
        return fs::fail("fs_qkv_attention: bad arguments");
    if (fused && D % 96 != 0) return fs::fail("fs_qkv_attention: the fused K / V^T epilogue needs D %% 96 == 0 (D %d)", D);
    const int heads = D / 64;
    float* planes = workspace;
    float* scratch = fs::attention_scratch_floats(B, tokens, heads) ? workspace + fs::attention_split_floats(B, tokens, heads) : nullptr;
    if (fused) {
        fs::ConvParams p = fs::linear_qkv_params(in, w, bias, qkv_out, B, tokens, D, planes);
        fs::attach_planes(p, w_planes, (size_t)3 * D * D);
        if (int rc = fs::launch_conv_igemm(p, S(stream), 6)) return rc;
    } else {
        fs::ConvParams p = fs::linear_params(in, w, bias, nullptr, qkv_out, B * tokens, D, 3 * D, 0, false);
        fs::attach_planes(p, w_planes, (size_t)3 * D * D);
        if (int rc = fs::launch_conv_igemm(p, S(stream))) return rc;
    }
    return fs::launch_attention_split(qkv_out, att_out, B, tokens, heads, 0.125f, scratch, planes, S(stream), fused != 0);
}
static int fs_mask_head(const float* pp, const float* cc, const float* gamma, const float* beta, float* out, int B, int N, int K, int D,
                        fs_stream stream) {
    if (!pp || !cc || !gamma || !beta || !out || B < 1 || N < 1 || D < 4) return fs::fail("fs_mask_head: bad arguments");
    return fs::launch_mask_head(pp, cc, gamma, beta, out, B, N, K, D, S(stream));
}
static int fs_patchify(const float* in, const float* in2, int B1, float* out, int B, int H, int W, int P, fs_stream stream) {
    if (!out || B < 1 || H < 1 || W < 1 || P < 1) return fs::fail("fs_patchify: bad arguments");
    return fs::launch_patchify(in, in2, B1, out, B, H, W, P, (H + P - 1) / P, (W + P - 1) / P, S(stream));
}
static int fs_vit_assemble(const float* emb, const float* cls, const float* pos, float* X, int B, int N, int D, fs_stream stream) {
    if (!emb || !cls || !pos || !X || B < 1 || N < 1 || D < 4) return fs::fail("fs_vit_assemble: bad arguments");
    return fs::launch_vit_assemble(emb, cls, pos, X, B, N, D, S(stream));
}
static int fs_dec_assemble(const float* Y, const float* cls_emb, float* Z, int B, int N, int K, int D, fs_stream stream) {
    if (!Y || !cls_emb || !Z || B < 1 || N < 1 || K < 1 || D < 4) return fs::fail("fs_dec_assemble: bad arguments");
    return fs::launch_dec_assemble(Y, cls_emb, Z, B, N, K, D, S(stream));
}

// ---- CNN heads and projection shortcut: the launchers and the geometry builders of net.h that net.hip itself calls
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int fs_concat_scaled_filters(const float* wa, const float* sa, const float* ha, int Ka, const float* wb, const float* sb, const float* hb, int Kb,
                                    float* out, float* shift_out, int O, fs_stream stream) {
    return fs::launch_concat_scaled_filters(wa, sa, ha, Ka, wb, sb, hb, Kb, out, shift_out, O, S(stream));  // validates its arguments itself
}
static int fs_pack_slice_tap_major(const float* oihw, float* out, int O, int I, int c0, int nc, int taps, fs_stream stream) {
    if (!oihw || !out || O < 1 || I < 1 || taps < 1) return fs::fail("fs_pack_slice_tap_major: bad arguments");
    return fs::launch_pack_slice_tap_major(oihw, out, O, I, c0, nc, taps, S(stream));
}
static int fs_dual_conv(const float* a, int ld_a, const float* b, int ld_b, const float* wgt, const void* wgt_planes, const float* shift, float* out,
                        int ld_out, int B, int Ho, int Wo, int Cin, int Cin2, int H2, int W2, int stride2, int Cout, int relu, int tile,
                        fs_stream stream) {
    if (!a || !b || (!wgt && !wgt_planes) || !out || B < 1 || Ho < 1 || Wo < 1 || H2 < 1 || W2 < 1 || Cin < 32 || Cin2 < 32 || Cout < 1 || stride2 < 1 ||
        relu < 0 || relu > 2)
        return fs::fail("fs_dual_conv: bad arguments");
    if (tile < 0 || tile > 2) return fs::fail("fs_dual_conv: tile must be 0, 1 or 2 (got %d): the concatenated-K kernels have the two 128-row tiles", tile);
    fs::ConvParams p = fs::dual_conv_params(a, ld_a, b, ld_b, wgt, shift, out, ld_out, B, Ho, Wo, Cin, Cin2, H2, W2, stride2, Cout, relu);
    fs::attach_planes(p, wgt_planes, (size_t)Cout * ((size_t)Cin + Cin2));
    return fs::launch_conv_igemm(p, S(stream), tile);
}
static int fs_pyramid_pool(const float* in, int ld_in, float* out, int B, int H, int W, int C, fs_stream stream) {
    if (!in || !out || B < 1 || B > 65535 || H < 1 || W < 1 || C < 32 || C % 32 != 0 || ld_in < C || ld_in % 4 != 0 || !al16(in) || !al16(out))
        return fs::fail("fs_pyramid_pool: bad arguments (C %% 32 == 0, ld_in >= C, ld_in %% 4 == 0, 16-B aligned maps)");
    const int bins[4] = {1, 2, 3, 6};
    return fs::pyramid_pool(nullptr, in, ld_in, out, B, H, W, C, bins, S(stream));
}
static int fs_rowdot_batch(int nprob, const float* const* in, const float* const* wgt, const float* const* scale, const float* const* shift,
                           float* const* out, const int* M, int ld_in, int ld_out, int K, int N, int relu, fs_stream stream) {
    if (nprob < 1 || nprob > 4 || !in || !wgt || !out || !M || K < 1 || N < 1 || ld_in < K || ld_in % 4 != 0 || ld_out < N)
        return fs::fail("fs_rowdot_batch: bad arguments (1..4 problems, ld_in >= K, ld_in %% 4 == 0, ld_out >= N)");
    fs::RowdotBatch pb{};
    for (int i = 0; i < nprob; ++i) {
        if (!in[i] || !wgt[i] || !out[i] || M[i] < 1 || !al16(in[i]) || !al16(wgt[i])) return fs::fail("fs_rowdot_batch: bad problem %d", i);
        pb.p[i] = fs::RowdotProblem{in[i], wgt[i], scale ? scale[i] : nullptr, shift ? shift[i] : nullptr, out[i], M[i]};
    }
    return fs::launch_rowdot_1x1_batch(pb, nprob, ld_in, ld_out, K, N, relu, S(stream));
}
static int fs_upsample_into(const float* in, int hi, int wi, float* out, int ld_out, int B, int Ho, int Wo, int C, int align_corners, fs_stream stream) {
    if (!in || !out || hi < 1 || wi < 1 || B < 1 || Ho < 1 || Wo < 1 || C < 4 || ld_out < C || align_corners < 0 || align_corners > 1 || !al16(in))
        return fs::fail("fs_upsample_into: bad arguments");
    return fs::launch_upsample_into(in, hi, wi, out, ld_out, B, Ho, Wo, C, align_corners, S(stream));
}
static int fs_classifier_nchw(const float* in, int ld_in, const float* wgt, const float* bias, float* out, int B, int HW, int C, int K, fs_stream stream) {
    if (!in || !wgt || !out || B < 1 || HW < 1 || C < 4 || K < 1 || ld_in < C || !al16(in)) return fs::fail("fs_classifier_nchw: bad arguments");
    return fs::launch_classifier_nchw(in, ld_in, wgt, bias, out, B, HW, C, K, S(stream));
}
static int ppm_head_args(const char* what, const float* T, int ld, const int* bins, const float* scale, const float* shift, int B, int H, int W, int C,
                         const float* cls_w, float* logits, int K, const float* scratch) {
    if (!T || !bins || !cls_w || !logits || !scratch || B < 1 || H < 1 || W < 1 || C < 4 || K < 1 || ld < C || !al16(scale) || !al16(shift) || !al16(scratch))
        return fs::fail("%s: bad arguments", what);
    return 0;
}
static size_t fs_ppm_term_scratch_floats(int B, int H, int C) { return B < 1 || H < 1 || C < 1 ? 0 : fs::ppm_term_scratch_floats(B, H, C); }
static int fs_ppm_term_classify(const float* T, int ld, const float* z1, const float* z2, const float* z3, const float* z6, const int* bins,
                                const float* scale, const float* shift, int B, int H, int W, int C, int relu, const float* cls_w, const float* cls_b,
                                float* logits, int K, float* scratch, fs_stream stream) {
    if (int rc = ppm_head_args("fs_ppm_term_classify", T, ld, bins, scale, shift, B, H, W, C, cls_w, logits, K, scratch)) return rc;
    const float* Z[4] = {z1, z2, z3, z6};
    return fs::launch_ppm_term_classify(T, ld, Z, bins, scratch, scale, shift, B, H, W, C, relu, cls_w, cls_b, logits, K, S(stream));
}
static size_t fs_ppm_head_workspace_floats(int B, int H, int C) {
    return B < 1 || H < 1 || C < 1 ? 0 : (size_t)4 * B * 36 * 9 * C + fs::ppm_term_scratch_floats(B, H, C);
}
static int fs_ppm_head(const float* T, int ld, const float* reduced, int Cr, const float* zw, const void* zw_planes, const int* bins, const float* scale,
                       const float* shift, int B, int H, int W, int C, int relu, const float* cls_w, const float* cls_b, float* logits, int K,
                       float* workspace, fs_stream stream) {
    if (int rc = ppm_head_args("fs_ppm_head", T, ld, bins, scale, shift, B, H, W, C, cls_w, logits, K, workspace)) return rc;
    if (!reduced || !zw || Cr < 32 || Cr % 32 != 0) return fs::fail("fs_ppm_head: bad reduced maps / filter bank (Cr %% 32 == 0 required, got %d)", Cr);
    for (int i = 0; i < 4; ++i)
        if (bins[i] < 1 || bins[i] > 6) return fs::fail("fs_ppm_head: a level's slot holds 36 cells (bin %d)", bins[i]);
    float* zbuf = workspace;
    fs::ConvParams p = fs::ppm_z_params(reduced, zw, zbuf, B, Cr, 9 * C);
    fs::attach_planes(p, zw_planes, (size_t)4 * 9 * C * Cr);
    if (int rc = fs::launch_conv_igemm(p, S(stream))) return rc;
    const float* Z[4];
    for (int i = 0; i < 4; ++i) Z[i] = zbuf + (size_t)i * p.g_out;
    return fs::launch_ppm_term_classify(T, ld, Z, bins, zbuf + (size_t)4 * p.g_out, scale, shift, B, H, W, C, relu, cls_w, cls_b, logits, K, S(stream));
}
// the argument refusals block_match and block_match_modes share, under the caller's name
static int block_match_args(const char* what, const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int search, int penalty,
                            const int32_t* mv) {
    if (!cur || !ref || !mv) return fs::fail("%s: null pointer", what);
    if (channels != 1 && channels != 3) return fs::fail("%s: channels must be 1 (luma) or 3 (RGB), got %d", what, channels);
    if (H < 16 || W < 16) return fs::fail("%s: frame %d x %d is smaller than one 16 x 16 block", what, H, W);
    if (search < 1 || search > 32) return fs::fail("%s: search range must be 1..32, got %d", what, search);
    if (penalty < 0 || penalty > 255) return fs::fail("%s: penalty must be 0..255, got %d", what, penalty);
    if ((int64_t)H * W * channels >= ((int64_t)1 << 31)) return fs::fail("%s: frame too large (%d x %d x %d bytes pass 2^31)", what, H, W, channels);
    return 0;
}
static int fs_block_match(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int search, int penalty, int32_t* mv, int32_t* cost,
                          fs_stream stream) {
    if (int rc = block_match_args("fs_block_match", cur, ref, H, W, channels, search, penalty, mv)) return rc;
    return fs::launch_block_match(cur, ref, H, W, channels, search, penalty, mv, cost, S(stream));
}
static int fs_block_match_modes(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int search, int penalty, int intra_bias,
                                int cut_permille, int32_t* mv, int32_t* cost, int32_t* activity, int32_t* stats, fs_stream stream) {
    if (int rc = block_match_args("fs_block_match_modes", cur, ref, H, W, channels, search, penalty, mv)) return rc;
    if (intra_bias < 0 || intra_bias > 65535) return fs::fail("fs_block_match_modes: intra_bias must be 0..65535, got %d", intra_bias);
    if (cut_permille < 0 || cut_permille > 1000) return fs::fail("fs_block_match_modes: cut_permille must be 0..1000, got %d", cut_permille);
    return fs::launch_block_match_modes(cur, ref, H, W, channels, search, penalty, intra_bias, cut_permille, mv, cost, activity, stats, S(stream));
}
static int fs_window_weights(int n, const int32_t* const* stats, float* weights, int32_t* source, fs_stream stream) {
    if (n < 1 || n > fs::WINDOW_MAX_FRAMES) return fs::fail("fs_window_weights: n must be 1..%d, got %d", fs::WINDOW_MAX_FRAMES, n);
    if (!weights || !source) return fs::fail("fs_window_weights: null output pointer");
    return fs::launch_window_weights(stats, n, weights, source, S(stream));
}
// fs_seg_tail / fs_seg_tail_accumulate / fs_crops_fuse with per-frame blend weights: the same launch functions, one more pointer
static int fs_seg_tail_weighted(const float* lo_prev, const float* lo_next, const float* const* grids_left, const float* const* grids_right, int K,
                                int h, int w, int Hg, int Wg, int H, int W, int n, int no_warp, float* out_logits, uint8_t* out_mask, double* canvas,
                                double* count, int cH, int cW, int y0, int x0, float* scratch, const float* weights, fs_stream stream) {
    if (!lo_prev || h < 1 || w < 1 || H < 1 || W < 1) return fs::fail("fs_seg_tail_weighted: bad arguments");
    if (canvas && (!count || cH < 1 || cW < 1)) return fs::fail("fs_seg_tail_weighted: a canvas without its count or size");
    fs::SegTailParams p{};
    p.lo_prev = lo_prev;
    p.lo_next = lo_next;
    p.grids_left = grids_left;
    p.grids_right = grids_right;
    p.K = K;
    p.h = h;
    p.w = w;
    p.Hg = Hg;
    p.Wg = Wg;
    p.H = H;
    p.W = W;
    p.n = n;
    p.no_warp = no_warp;
    p.out_logits = out_logits;
    p.out_mask = out_mask;
    p.scratch = scratch;
    p.canvas = canvas;
    p.count = count;
    p.cH = cH;
    p.cW = cW;
    p.y0 = y0;
    p.x0 = x0;
    p.weights = weights;
    return fs::launch_seg_tail(p, S(stream));
}
static int fs_crops_fuse_weighted(const float* lo_prev, const float* lo_next, const float* crop_grids, int ncrops, const int* crop_y,
                                  const int* crop_x, int K, int h, int w, int Hg, int Wg, int ch, int cw, int n, int no_warp, double* canvas,
                                  uint8_t* mask, int H, int W, float* scratch, const float* weights, fs_stream stream) {
    if (!lo_prev || !crop_y || !crop_x || ncrops < 1 || ncrops > 64 || h < 1 || w < 1 || ch < 1 || cw < 1 || H < 1 || W < 1 || H > 32767 || W > 32767)
        return fs::fail("fs_crops_fuse_weighted: bad arguments (1..64 crops, frame at most 32767 px)");
    fs::CropsFuseParams p{};
    p.lo_prev = lo_prev;
    p.lo_next = lo_next;
    p.nc = ncrops;
    for (int c = 0; c < ncrops; ++c) {
        p.cy[c] = (short)crop_y[c];
        p.cx[c] = (short)crop_x[c];
    }
    p.K = K; p.h = h; p.w = w; p.Hg = Hg; p.Wg = Wg; p.ch = ch; p.cw = cw; p.n = n; p.no_warp = no_warp;
    p.canvas = canvas;
    p.mask = mask;
    p.H = H;
    p.W = W;
    p.weights = weights;
    return fs::launch_crops_fuse(p, crop_grids, scratch, S(stream));
}
// fs_feat_tail with per-map blend weights: the same launch function, one more pointer
static int fs_feat_tail_weighted(const float* f_prev, const float* f_next, int C, int fh, int fw, const float* const* grids_left,
                                 const float* const* grids_right, int Hg, int Wg, const float* grid0, int H0, int W0, int n, int no_warp, float* stack,
                                 float* scratch, const float* weights, fs_stream stream) {
    if (!f_prev || !stack || C < 1 || fh < 1 || fw < 1) return fs::fail("fs_feat_tail_weighted: bad arguments");
    fs::FeatTailParams p{};
    p.f_prev = f_prev;
    p.f_next = f_next;
    p.grids_left = grids_left;
    p.grids_right = grids_right;
    p.grid0 = grid0;
    p.C = C;
    p.fh = fh;
    p.fw = fw;
    p.Hg = Hg;
    p.Wg = Wg;
    p.H0 = H0;
    p.W0 = W0;
    p.n = n;
    p.no_warp = no_warp;
    p.stack = stack;
    p.scratch = scratch;
    p.weights = weights;
    return fs::launch_feat_tail(p, S(stream));
}
// per-pixel confidence and the per-frame extent report (conf_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_mask_confidence(const float* logits, int n, int K, int h, int w, uint8_t* mask, uint8_t* confidence, int H, int W, fs_stream stream) {
    return fs::launch_mask_confidence(logits, n, K, h, w, mask, confidence, H, W, S(stream));
}
static int fs_canvas_confidence(const double* canvas, int n, int K, int h, int w, uint8_t* mask, uint8_t* confidence, int H, int W, fs_stream stream) {
    return fs::launch_canvas_confidence(canvas, n, K, h, w, mask, confidence, H, W, S(stream));
}
static int fs_frame_report(const uint8_t* mask, const uint8_t* confidence, int n, int H, int W, int K, int low, int64_t* report, fs_stream stream) {
    return fs::launch_frame_report(mask, confidence, n, H, W, K, low, reinterpret_cast<long long*>(report), S(stream));
}
// connected regions of a mask (region_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_mask_regions(const uint8_t* mask, int n, int H, int W, int K, int connectivity, int32_t* labels, fs_stream stream) {
    return fs::launch_mask_regions(mask, n, H, W, K, connectivity, labels, S(stream));
}
static int fs_region_table(const uint8_t* mask, const int32_t* labels, const uint8_t* confidence, int n, int H, int W, int K, int low, int max_regions,
                           int64_t* table, int64_t* counts, int32_t* index, int32_t* workspace, fs_stream stream) {
    return fs::launch_region_table(mask, labels, confidence, n, H, W, K, low, max_regions, reinterpret_cast<long long*>(table),
                                   reinterpret_cast<long long*>(counts), index, workspace, S(stream));
}
static int fs_region_filter(const uint8_t* mask, const int32_t* index, const int64_t* table, int n, int H, int W, int K, int max_regions, int min_area,
                            uint8_t* out, int32_t* votes, fs_stream stream) {
    return fs::launch_region_filter(mask, index, reinterpret_cast<const long long*>(table), n, H, W, K, max_regions, min_area, out, votes, S(stream));
}
// region identity across frames (track_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_region_links(const int32_t* index, const int64_t* table, const int64_t* counts, const int32_t* prev_index, const int64_t* prev_table,
                           const int64_t* prev_counts, int n, int H, int W, int max_regions, int max_pairs, int min_overlap, int32_t* back, int32_t* fwd,
                           int64_t* link_counts, void* workspace, fs_stream stream) {
    return fs::launch_region_links(index, reinterpret_cast<const long long*>(table), reinterpret_cast<const long long*>(counts), prev_index,
                                   reinterpret_cast<const long long*>(prev_table), reinterpret_cast<const long long*>(prev_counts), n, H, W, max_regions,
                                   max_pairs, min_overlap, back, fwd, reinterpret_cast<long long*>(link_counts), workspace, S(stream));
}
static int fs_region_tracks(const int32_t* back, const int32_t* fwd, const int64_t* counts, const int64_t* prev_tracks, int n, int max_regions,
                            int64_t* state, int64_t* tracks, fs_stream stream) {
    return fs::launch_region_tracks(back, fwd, reinterpret_cast<const long long*>(counts), reinterpret_cast<const long long*>(prev_tracks), n, max_regions,
                                    reinterpret_cast<long long*>(state), reinterpret_cast<long long*>(tracks), S(stream));
}
static int fs_region_links_mc(const int32_t* index, const int64_t* table, const int64_t* counts, const int32_t* prev_index, const int64_t* prev_table,
                              const int64_t* prev_counts, const int32_t* mv, const int32_t* pair_stats, int n, int H, int W, int frame_h, int frame_w,
                              int max_regions, int max_pairs, int min_overlap, int32_t* back, int32_t* fwd, int64_t* link_counts, void* workspace,
                              fs_stream stream) {
    return fs::launch_region_links_mc(index, reinterpret_cast<const long long*>(table), reinterpret_cast<const long long*>(counts), prev_index,
                                      reinterpret_cast<const long long*>(prev_table), reinterpret_cast<const long long*>(prev_counts), mv, pair_stats, n, H, W,
                                      frame_h, frame_w, max_regions, max_pairs, min_overlap, back, fwd, reinterpret_cast<long long*>(link_counts), workspace,
                                      S(stream));
}
// region outlines (outline_ops.hip): the launcher validates, nothing is launched on a refusal
static int fs_region_outlines(const int32_t* index, int n, int H, int W, int max_regions, int connectivity, int max_contours, int max_vertices,
                              int64_t* contours, int32_t* vertices, int64_t* shape, int64_t* counts, void* workspace, fs_stream stream) {
    return fs::launch_region_outlines(index, n, H, W, max_regions, connectivity, max_contours, max_vertices, reinterpret_cast<long long*>(contours),
                                      vertices, reinterpret_cast<long long*>(shape), reinterpret_cast<long long*>(counts), workspace, S(stream));
}
// outline simplification (simplify_ops.hip): the launcher validates, nothing is launched on a refusal
static int fs_outline_simplify(const int64_t* contours, const int32_t* vertices, const int64_t* counts, int n, int max_contours, int max_vertices, int tol_q,
                               int max_rounds, int64_t* simple, int32_t* simple_vertices, int64_t* simple_counts, void* workspace, fs_stream stream) {
    return fs::launch_outline_simplify(reinterpret_cast<const long long*>(contours), vertices, reinterpret_cast<const long long*>(counts), n, max_contours,
                                       max_vertices, tol_q, max_rounds, reinterpret_cast<long long*>(simple), simple_vertices,
                                       reinterpret_cast<long long*>(simple_counts), workspace, S(stream));
}
static int fs_frame_prepare(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int H, int W,
                            const float* mean, const float* std, float* out, int h, int w, fs_stream stream) {
    if (!frame || !mean || !std || !out) return fs::fail("fs_frame_prepare: null pointer");
    if (format < 0 || format > 2) return fs::fail("fs_frame_prepare: format must be 0 (RGB24), 1 (NV12) or 2 (I420), got %d", format);
    if (matrix != 0 && matrix != 1) return fs::fail("fs_frame_prepare: matrix must be 0 (BT.601) or 1 (BT.709), got %d", matrix);
    if (full_range != 0 && full_range != 1) return fs::fail("fs_frame_prepare: range must be 0 (limited) or 1 (full), got %d", full_range);
    if (H < 1 || W < 1 || h < 1 || w < 1) return fs::fail("fs_frame_prepare: empty frame (%d x %d -> %d x %d)", H, W, h, w);
    if ((int64_t)H * W * 3 >= ((int64_t)1 << 31)) return fs::fail("fs_frame_prepare: frame too large (%d x %d x 3 bytes pass 2^31)", H, W);
    if ((int64_t)h * w * 3 >= ((int64_t)1 << 31)) return fs::fail("fs_frame_prepare: output too large (3 x %d x %d values pass 2^31)", h, w);
    if (format != 0 && (!u || (format == 2 && !v))) return fs::fail("fs_frame_prepare: null chroma pointer for a YUV format");
    if (reinterpret_cast<uintptr_t>(out) % 4 != 0) return fs::fail("fs_frame_prepare: out is not aligned to a float");
    return fs::launch_frame_prepare(frame, u, v, format, matrix, full_range, H, W, mean, std, out, h, w, S(stream));
}
// the refusals frame_compose and frame_compose_regions share, under the caller's name
static int frame_compose_args(const char* what, const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u,
                              const uint8_t* v, int format, int matrix, int full_range, int H, int W, const uint8_t* out, const uint8_t* out_u,
                              const uint8_t* out_v, int out_format, int out_matrix, int out_full_range) {
    if (!mask || !palette || !out) return fs::fail("%s: null pointer", what);
    if (format < 0 || format > 2 || out_format < 0 || out_format > 2)
        return fs::fail("%s: format must be 0 (RGB24), 1 (NV12) or 2 (I420), got %d in, %d out", what, format, out_format);
    if ((matrix != 0 && matrix != 1) || (out_matrix != 0 && out_matrix != 1))
        return fs::fail("%s: matrix must be 0 (BT.601) or 1 (BT.709), got %d in, %d out", what, matrix, out_matrix);
    if ((full_range != 0 && full_range != 1) || (out_full_range != 0 && out_full_range != 1))
        return fs::fail("%s: range must be 0 (limited) or 1 (full), got %d in, %d out", what, full_range, out_full_range);
    if (K < 1 || K > 256) return fs::fail("%s: palette must hold 1..256 classes, got %d", what, K);
    if (h < 1 || w < 1) return fs::fail("%s: empty frame (%d x %d)", what, h, w);
    if ((int64_t)h * w * 3 >= ((int64_t)1 << 31)) return fs::fail("%s: output too large (%d x %d x 3 bytes pass 2^31)", what, h, w);
    if (out_format != 0 && (!out_u || (out_format == 2 && !out_v))) return fs::fail("%s: null output chroma pointer for a YUV format", what);
    if (!frame) {
        if (H != 0 || W != 0 || u || v) return fs::fail("%s: background geometry or chroma (%d x %d) without a background frame", what, H, W);
    } else {
        if (H < 1 || W < 1) return fs::fail("%s: a background frame without its geometry (%d x %d)", what, H, W);
        if ((int64_t)H * W * 3 >= ((int64_t)1 << 31)) return fs::fail("%s: background too large (%d x %d x 3 bytes pass 2^31)", what, H, W);
        if (format != 0 && (!u || (format == 2 && !v))) return fs::fail("%s: null background chroma pointer for a YUV format", what);
    }
    return 0;
}
static int fs_frame_compose(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                            int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                            int out_matrix, int out_full_range, fs_stream stream) {
    if (int rc = frame_compose_args("fs_frame_compose", mask, h, w, palette, K, frame, u, v, format, matrix, full_range, H, W, out, out_u, out_v, out_format,
                                    out_matrix, out_full_range))
        return rc;
    return fs::launch_frame_compose(mask, h, w, palette, K, frame, u, v, format, matrix, full_range, H, W, out, out_u, out_v, out_format, out_matrix,
                                    out_full_range, S(stream));
}
// region overlay (overlay_ops.hip): frame_compose's refusals, then the layers'; nothing is launched on a refusal
static int fs_frame_compose_regions(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                                    int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                                    int out_matrix, int out_full_range, const int32_t* index, const int64_t* table, const int64_t* counts,
                                    const int64_t* tracks, int max_regions, const uint8_t* fill_palette, int fill_colours, const uint8_t* outline,
                                    int outline_width, int label_scale, int64_t label_min_area, uint32_t halo_rgba, uint32_t ink_rgb, void* workspace,
                                    fs_stream stream) {
    const char* what = "fs_frame_compose_regions";
    if (int rc = frame_compose_args(what, mask, h, w, palette, K, frame, u, v, format, matrix, full_range, H, W, out, out_u, out_v, out_format, out_matrix,
                                    out_full_range))
        return rc;
    if (!index) return fs::fail("%s: null index plane", what);
    if (max_regions < 1 || max_regions > 65536) return fs::fail("%s: max_regions must be 1..65536, got %d", what, max_regions);
    if (fill_colours < 0 || fill_colours > 256) return fs::fail("%s: the fill palette must hold 0..256 colours, got %d", what, fill_colours);
    if (outline_width < 0 || outline_width > 4) return fs::fail("%s: outline_width must be 0..4, got %d", what, outline_width);
    if (label_scale < 0 || label_scale > 4) return fs::fail("%s: label_scale must be 0..4, got %d", what, label_scale);
    if (label_min_area < 1) return fs::fail("%s: label_min_area must be at least 1, got %lld", what, (long long)label_min_area);
    if (fill_colours > 0 && !fill_palette) return fs::fail("%s: %d fill colours without a fill palette", what, fill_colours);
    if (label_scale > 0 && (!table || !counts)) return fs::fail("%s: labels need the region table and its counts", what);
    if (label_scale > 0 && !workspace) return fs::fail("%s: labels need the marks workspace", what);
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return fs::fail("%s: the workspace is not aligned to 4 bytes", what);
    return fs::launch_frame_compose_regions(mask, h, w, palette, K, frame, u, v, format, matrix, full_range, H, W, out, out_u, out_v, out_format, out_matrix,
                                            out_full_range, index, reinterpret_cast<const long long*>(table), reinterpret_cast<const long long*>(counts),
                                            reinterpret_cast<const long long*>(tracks), max_regions, fill_palette, fill_colours, outline, outline_width,
                                            label_scale, label_min_area, halo_rgba, ink_rgb, workspace, S(stream));
}
// temporal mask stabiliser (stabilize_ops.hip): the launcher validates, nothing is launched on a refusal
static int fs_mask_stabilize(const uint8_t* mask, const uint8_t* confidence, const int32_t* mv, const int32_t* pair_stats, int n, int H, int W, int frame_h,
                             int frame_w, int K, int persist, int trust, int has_state, uint32_t* state, uint8_t* out, int64_t* counts, void* workspace,
                             fs_stream stream) {
    return fs::launch_mask_stabilize(mask, confidence, mv, pair_stats, n, H, W, frame_h, frame_w, K, persist, trust, has_state, state, out,
                                     reinterpret_cast<long long*>(counts), workspace, S(stream));
}

// distance to a class (distance_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_mask_distance(const uint8_t* mask, int n, int H, int W, uint32_t source_set, int max_dist, uint32_t* d2, int32_t* nearest, void* workspace,
                            fs_stream stream) {
    return fs::launch_mask_distance(mask, n, H, W, source_set, max_dist, d2, nearest, workspace, S(stream));
}
static int fs_region_proximity(const uint8_t* mask, const uint32_t* d2, const int32_t* nearest, const int32_t* index, const int64_t* counts, int n, int H,
                               int W, int K, int max_regions, uint32_t target_set, const int32_t* thresholds, int B, int64_t* exposure, int64_t* near,
                               fs_stream stream) {
    return fs::launch_region_proximity(mask, d2, nearest, index, reinterpret_cast<const long long*>(counts), n, H, W, K, max_regions, target_set, thresholds,
                                       B, reinterpret_cast<long long*>(exposure), reinterpret_cast<long long*>(near), S(stream));
}

// the flood-extent mosaic (mosaic_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_global_motion(const int32_t* tables, const int32_t* pair_stats, const uint8_t* mask, uint32_t exclude_set, int n, int FH, int FW, int H, int W,
                            int rounds, int64_t tol_q20, int min_inliers, int64_t* model, fs_stream stream) {
    return fs::launch_global_motion(tables, pair_stats, mask, exclude_set, n, FH, FW, H, W, rounds, (long long)tol_q20, min_inliers,
                                    reinterpret_cast<long long*>(model), S(stream));
}
static int fs_pose_chain(const int64_t* model, int64_t* state, int64_t* poses, int n, int H, int W, int CH, int CW, int ox, int oy, int max_bridge,
                         fs_stream stream) {
    return fs::launch_pose_chain(reinterpret_cast<const long long*>(model), reinterpret_cast<long long*>(state), reinterpret_cast<long long*>(poses), n, H, W,
                                 CH, CW, ox, oy, max_bridge, S(stream));
}
static int fs_mosaic_accumulate(const uint8_t* mask, const int64_t* poses, int n, int H, int W, int K, int CH, int CW, int ox, int oy, uint16_t* votes,
                                fs_stream stream) {
    return fs::launch_mosaic_accumulate(mask, reinterpret_cast<const long long*>(poses), n, H, W, K, CH, CW, ox, oy, votes, S(stream));
}
static int fs_mosaic_resolve(const uint16_t* votes, int K, int CH, int CW, uint8_t* cls, uint8_t* conf, uint32_t* seen, int64_t* totals, fs_stream stream) {
    return fs::launch_mosaic_resolve(votes, K, CH, CW, cls, conf, seen, reinterpret_cast<long long*>(totals), S(stream));
}

// the orthophoto under the mosaic (ortho_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_ortho_accumulate(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW,
                               const int64_t* pose, uint32_t ordinal, int H, int W, int mode, int CH, int CW, int ox, int oy, uint64_t* rank, uint32_t* rgba,
                               fs_stream stream) {
    return fs::launch_ortho_accumulate(frame, u, v, format, matrix, full_range, FH, FW, reinterpret_cast<const long long*>(pose), ordinal, H, W, mode, CH, CW,
                                       ox, oy, reinterpret_cast<unsigned long long*>(rank), rgba, S(stream));
}
static int fs_ortho_compose(const uint32_t* rgba, const uint8_t* cls, const uint8_t* palette, int K, uint32_t edge_set, uint32_t fill, int CH, int CW,
                            uint8_t* out, fs_stream stream) {
    return fs::launch_ortho_compose(rgba, cls, palette, K, edge_set, fill, CH, CW, out, S(stream));
}

// frame-to-map registration (refine_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_map_view(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const int64_t* pose,
                       uint32_t ordinal, int H, int W, int CH, int CW, int ox, int oy, const uint64_t* rank, const uint32_t* rgba, int min_age, uint8_t* cur,
                       uint8_t* view, uint8_t* valid, fs_stream stream) {
    return fs::launch_map_view(frame, u, v, format, matrix, full_range, FH, FW, reinterpret_cast<const long long*>(pose), ordinal, H, W, CH, CW, ox, oy,
                               reinterpret_cast<const unsigned long long*>(rank), rgba, min_age, cur, view, valid, S(stream));
}
static int fs_map_gate(int32_t* table, int blocks, const uint8_t* valid, int H, int W, fs_stream stream) {
    return fs::launch_map_gate(table, blocks, valid, H, W, S(stream));
}
static int fs_pose_correct(const int64_t* model, int64_t* state, int64_t* pose, int H, int W, int CH, int CW, int ox, int oy, int64_t* out, fs_stream stream) {
    return fs::launch_pose_correct(reinterpret_cast<const long long*>(model), reinterpret_cast<long long*>(state), reinterpret_cast<long long*>(pose), H, W, CH,
                                   CW, ox, oy, reinterpret_cast<long long*>(out), S(stream));
}

// the matcher's tables guided by the camera model (motion_ops.hip): the launcher validates, nothing is launched on a refusal
static int fs_guide_vectors(const int32_t* mv, const int64_t* model, int n, int FH, int FW, int fill_void, int64_t outlier_q20, const uint8_t* cur,
                            const uint8_t* ref, int channels, const int32_t* cost, int penalty, int guide_bias, int32_t* out, int64_t* counts,
                            fs_stream stream) {
    return fs::launch_guide_vectors(mv, reinterpret_cast<const long long*>(model), n, FH, FW, fill_void, (long long)outlier_q20, cur, ref, channels, cost,
                                    penalty, guide_bias, out, reinterpret_cast<long long*>(counts), S(stream));
}

// relocalisation against the orthophoto (relocate_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_map_coarse(const uint32_t* rgba, int CH, int CW, int scale, uint8_t* cl, uint8_t* cv, fs_stream stream) {
    return fs::launch_map_coarse(rgba, CH, CW, scale, cl, cv, S(stream));
}
static int fs_map_patch(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const int64_t* state, int H,
                        int W, int CH, int CW, int ox, int oy, int scale, uint8_t* tl, uint8_t* tv, int64_t* geom, fs_stream stream) {
    return fs::launch_map_patch(frame, u, v, format, matrix, full_range, FH, FW, reinterpret_cast<const long long*>(state), H, W, CH, CW, ox, oy, scale, tl, tv,
                                reinterpret_cast<long long*>(geom), S(stream));
}
static int fs_map_locate(const uint8_t* cl, const uint8_t* cv, int ch, int cw, const uint8_t* tl, const uint8_t* tv, const int64_t* geom, int min_overlap_permille,
                         int exclude, uint32_t* scores, int64_t* found, fs_stream stream) {
    return fs::launch_map_locate(cl, cv, ch, cw, tl, tv, reinterpret_cast<const long long*>(geom), min_overlap_permille, exclude, scores,
                                 reinterpret_cast<long long*>(found), S(stream));
}
static int fs_pose_relocate(const int64_t* found, const int64_t* state, int64_t* cand_state, int64_t* cand_pose, int max_mean, int ratio_permille, int H, int W,
                            int CH, int CW, int ox, int oy, int scale, fs_stream stream) {
    return fs::launch_pose_relocate(reinterpret_cast<const long long*>(found), reinterpret_cast<const long long*>(state), reinterpret_cast<long long*>(cand_state),
                                    reinterpret_cast<long long*>(cand_pose), max_mean, ratio_permille, H, W, CH, CW, ox, oy, scale, S(stream));
}
static int fs_relocate_commit(const int64_t* cand_state, const int64_t* cand_pose, const int64_t* correct_out, int64_t* state, int64_t* pose, const int64_t* found,
                              int scale, int64_t* out, fs_stream stream) {
    return fs::launch_relocate_commit(reinterpret_cast<const long long*>(cand_state), reinterpret_cast<const long long*>(cand_pose),
                                      reinterpret_cast<const long long*>(correct_out), reinterpret_cast<long long*>(state), reinterpret_cast<long long*>(pose),
                                      reinterpret_cast<const long long*>(found), scale, reinterpret_cast<long long*>(out), S(stream));
}

// map-to-map registration and the merge of two mosaics (merge_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_merge_view(const uint32_t* rgba_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b,
                         const int64_t* link, int Y0, int X0, int WH, int WW, uint8_t* cur, uint8_t* view, uint8_t* valid_a, uint8_t* valid_b, fs_stream stream) {
    return fs::launch_merge_view(rgba_a, CH_a, CW_a, ox_a, oy_a, rgba_b, CH_b, CW_b, ox_b, oy_b, reinterpret_cast<const long long*>(link), Y0, X0, WH, WW, cur, view,
                                 valid_a, valid_b, S(stream));
}
static int fs_merge_gate(int32_t* table, int blocks, const uint8_t* valid_a, const uint8_t* valid_b, int H, int W, fs_stream stream) {
    return fs::launch_merge_gate(table, blocks, valid_a, valid_b, H, W, S(stream));
}
static int fs_link_correct(const int64_t* model, int64_t* link, int Y0, int X0, int WH, int WW, int ox_a, int oy_a, int64_t* out, fs_stream stream) {
    return fs::launch_link_correct(reinterpret_cast<const long long*>(model), reinterpret_cast<long long*>(link), Y0, X0, WH, WW, ox_a, oy_a,
                                   reinterpret_cast<long long*>(out), S(stream));
}
static int fs_mosaic_merge(uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                           const int64_t* link, uint64_t* rank_a, uint32_t* rgba_a, const uint64_t* rank_b, const uint32_t* rgba_b, uint32_t ordinal_offset, int mode,
                           int64_t* counts, fs_stream stream) {
    return fs::launch_mosaic_merge(votes_a, CH_a, CW_a, ox_a, oy_a, votes_b, CH_b, CW_b, ox_b, oy_b, K, reinterpret_cast<const long long*>(link),
                                   reinterpret_cast<unsigned long long*>(rank_a), rgba_a, reinterpret_cast<const unsigned long long*>(rank_b), rgba_b,
                                   ordinal_offset, mode, reinterpret_cast<long long*>(counts), S(stream));
}
static int fs_merge_patch(const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b, const int64_t* link, int CH_a, int CW_a, int ox_a, int oy_a, int scale,
                          int y0, int x0, int y1, int x1, uint8_t* tl, uint8_t* tv, int64_t* geom, fs_stream stream) {
    return fs::launch_merge_patch(rgba_b, CH_b, CW_b, ox_b, oy_b, reinterpret_cast<const long long*>(link), CH_a, CW_a, ox_a, oy_a, scale, y0, x0, y1, x1, tl, tv,
                                  reinterpret_cast<long long*>(geom), S(stream));
}
static int fs_link_place(const int64_t* found, const int64_t* link, int scale, int max_mean, int ratio_permille, int64_t* cand, int64_t* out, fs_stream stream) {
    return fs::launch_link_place(reinterpret_cast<const long long*>(found), reinterpret_cast<const long long*>(link), scale, max_mean, ratio_permille,
                                 reinterpret_cast<long long*>(cand), reinterpret_cast<long long*>(out), S(stream));
}

// the flood-extent change between two registered mosaics (change_ops.hip): the launcher validates, nothing is launched on a refusal
static int fs_mosaic_change(const uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                            const int64_t* link, int min_votes, int min_conf, int tolerance, uint32_t watch_set, uint8_t* change, uint8_t* cls_a, uint8_t* cls_b,
                            int64_t* transitions, int64_t* counts, fs_stream stream) {
    return fs::launch_mosaic_change(votes_a, CH_a, CW_a, ox_a, oy_a, votes_b, CH_b, CW_b, ox_b, oy_b, K, reinterpret_cast<const long long*>(link), min_votes, min_conf,
                                    tolerance, watch_set, change, cls_a, cls_b, reinterpret_cast<long long*>(transitions), reinterpret_cast<long long*>(counts), S(stream));
}

// dry-route reachability (access_ops.hip): the launchers validate, nothing is launched on a refusal
static int fs_mask_access(const uint8_t* mask, const uint8_t* seeds, int n, int H, int W, const uint8_t* cost, uint32_t terminal_set, int connectivity,
                          uint32_t max_cost, int rounds, int resume, uint32_t* d, int32_t* origin, int32_t* status, void* workspace, fs_stream stream) {
    return fs::launch_mask_access(mask, seeds, n, H, W, cost, terminal_set, connectivity, max_cost, rounds, resume, d, origin, status, workspace, S(stream));
}
static int fs_region_access(const uint8_t* mask, const uint32_t* d, const int32_t* origin, const int32_t* index, const int64_t* counts, int n, int H, int W,
                            int K, int max_regions, int64_t* reach, int64_t* rows, fs_stream stream) {
    return fs::launch_region_access(mask, d, origin, index, reinterpret_cast<const long long*>(counts), n, H, W, K, max_regions,
                                    reinterpret_cast<long long*>(reach), reinterpret_cast<long long*>(rows), S(stream));
}

// georeferencing (ground_ops.hip): the launchers validate, nothing is launched on a refusal; the models are host arrays of nine doubles
static int fs_ground_area(const uint8_t* cls, int CH, int CW, int ox, int oy, const double* forward, int K, const int32_t* index, int max_regions,
                          int64_t* class_area2, int64_t* region_area2, int64_t* counts, fs_stream stream) {
    return fs::launch_ground_area(cls, CH, CW, ox, oy, forward, K, index, max_regions, reinterpret_cast<long long*>(class_area2),
                                  reinterpret_cast<long long*>(region_area2), reinterpret_cast<long long*>(counts), S(stream));
}
static int fs_ground_rectify(const double* inverse, int CH, int CW, int ox, int oy, int GH, int GW, int gsd_mm, int64_t e0_mm, int64_t ntop_mm, int nplanes,
                             const uint8_t* const* planes, uint8_t* const* outs, const uint32_t* rgba, uint8_t* rgb_out, int fill, uint32_t rgb_fill,
                             fs_stream stream) {
    return fs::launch_ground_rectify(inverse, CH, CW, ox, oy, GH, GW, gsd_mm, (long long)e0_mm, (long long)ntop_mm, nplanes, planes, outs, rgba, rgb_out, fill,
                                     rgb_fill, S(stream));
}
static int fs_ground_points(const int32_t* points, int n, const double* forward, int ox, int oy, int64_t* out, fs_stream stream) {
    return fs::launch_ground_points(points, n, forward, ox, oy, reinterpret_cast<long long*>(out), S(stream));
}

// the seventeen tables as one object: each table is built from the one before it, so there is one definition of every member list.  The
// first six are handed out as the fs_hook_tables5 at the head of that object.
static const fs_hook_tables5& hook_tables(void) {
    // fs_test_api (frozen) with the extension table right behind it: one object, so &tables.test is also &tables
    static const fs_hook_tables tables = {{
        sizeof(fs_test_api),
        fs_pack_conv_weight,
        fs_conv2d_nhwc,
        fs_split_bf16x3,
        fs_conv2d_nhwc_split,
        fs_attention_workspace_floats,
        fs_attention,
        fs_winograd_workspace_floats,
        fs_conv3x3_winograd_nhwc,
        fs_winograd_fused_workspace_floats,
        fs_conv3x3_winograd_fused_nhwc,
        fs_conv3x3_winograd_fused_pool_nhwc,
        fs_stem_conv_nchw,
        fs_stem_conv_nchw_split,
        fs_maxpool3x3s2_nhwc,
        fs_adaptive_avgpool_nhwc,
        fs_nchw_to_nhwc,
        fs_nhwc_to_nchw,
        fs_layernorm,
        fs_linear_splits,
        fs_linear,
        fs_qkv_attention_workspace_floats,
        fs_qkv_attention,
        fs_mask_head,
        fs_patchify,
        fs_vit_assemble,
        fs_dec_assemble,
        fs_concat_scaled_filters,
        fs_pack_slice_tap_major,
        fs_dual_conv,
        fs_pyramid_pool,
        fs_rowdot_batch,
        fs_upsample_into,
        fs_classifier_nchw,
        fs_ppm_term_scratch_floats,
        fs_ppm_term_classify,
        fs_ppm_head_workspace_floats,
        fs_ppm_head,
        fs_block_match,
    }, {
        FS_EXT_MAGIC,
        sizeof(fs_ext_api),
        fs_frame_prepare,
        fs_frame_compose,
    }};
    // the two tables above are frozen in text and size; later extension ops live in a third, append-only table behind them.  `all`
    // takes its first two tables from `tables` (one definition of the member lists), and &all.base.test is also &all.
    static const fs_hook_tables2 all = {tables, {
        FS_EXT2_MAGIC,
        sizeof(fs_ext2_api),
        fs_block_match_modes,
        fs_window_weights,
        fs_seg_tail_weighted,
        fs_crops_fuse_weighted,
        fs_feat_tail_weighted,
        fs_mask_confidence,
        fs_canvas_confidence,
        fs_frame_report,
        fs_mask_regions,
        fs_region_table,
        fs_region_filter,
        fs_region_links,
        fs_region_tracks,
        fs_region_links_mc,
    }};
    // fs_ext2_api is frozen too (size and text); the fourth table lies behind it by the same pattern, and &all3.base2.base.test is &all3.
    static const fs_hook_tables3 all3 = {all, {
        FS_EXT3_MAGIC,
        sizeof(fs_ext3_api),
        fs_region_outlines,
    }};
    // fs_ext3_api is frozen too (one member, 24 bytes); the fifth table lies behind it by the same pattern, and &all4.base3.base2.base.test is &all4.
    static const fs_hook_tables4 all4 = {all3, {
        FS_EXT4_MAGIC,
        sizeof(fs_ext4_api),
        fs_outline_simplify,
    }};
    // fs_ext4_api is frozen too (one member, 24 bytes); the sixth table lies behind it by the same pattern, and &all5.base4 is &all5.
    static const fs_hook_tables5 all5 = {all4, {
        FS_EXT5_MAGIC,
        sizeof(fs_ext5_api),
        fs_frame_compose_regions,
    }};
    // fs_ext5_api is frozen too (one member, 24 bytes); the seventh table lies behind it by the same pattern, and &all6.base5 is &all6.
    static const fs_hook_tables6 all6 = {all5, {
        FS_EXT6_MAGIC,
        sizeof(fs_ext6_api),
        fs_mask_stabilize,
    }};
    // fs_ext6_api is frozen too (one member, 24 bytes); the eighth table lies behind it by the same pattern, and &all7.base6 is &all7.
    static const fs_hook_tables7 all7 = {all6, {
        FS_EXT7_MAGIC,
        sizeof(fs_ext7_api),
        fs_mask_distance,
        fs_region_proximity,
    }};
    // fs_ext7_api is frozen too (two members, 32 bytes; tests/test_distance_cpu.py); the ninth table lies behind it, and &all8.base7 is &all8.
    static const fs_hook_tables8 all8 = {all7, {
        FS_EXT8_MAGIC,
        sizeof(fs_ext8_api),
        fs_global_motion,
        fs_pose_chain,
        fs_mosaic_accumulate,
        fs_mosaic_resolve,
    }};
    // fs_ext8_api is frozen too (four members, 48 bytes; tests/test_mosaic_cpu.py); the tenth table lies behind it, and &all9.base8 is &all9.
    static const fs_hook_tables9 all9 = {all8, {
        FS_EXT9_MAGIC,
        sizeof(fs_ext9_api),
        fs_ortho_accumulate,
        fs_ortho_compose,
    }};
    // fs_ext9_api is frozen too (two members, 32 bytes; tests/test_ortho_cpu.py); the eleventh table lies behind it, and &all10.base9 is &all10.
    static const fs_hook_tables10 all10 = {all9, {
        FS_EXT10_MAGIC,
        sizeof(fs_ext10_api),
        fs_map_view,
        fs_map_gate,
        fs_pose_correct,
    }};
    // fs_ext10_api is frozen too (three members, 40 bytes; tests/test_guide_cpu.py); the twelfth table lies behind it, and &all11.base10 is &all11.
    static const fs_hook_tables11 all11 = {all10, {
        FS_EXT11_MAGIC,
        sizeof(fs_ext11_api),
        fs_guide_vectors,
    }};
    // fs_ext11_api is frozen too (one member, 24 bytes; tests/test_relocate_cpu.py); the thirteenth table lies behind it, and &all12.base11 is &all12.
    static const fs_hook_tables12 all12 = {all11, {
        FS_EXT12_MAGIC,
        sizeof(fs_ext12_api),
        fs_map_coarse,
        fs_map_patch,
        fs_map_locate,
        fs_pose_relocate,
        fs_relocate_commit,
    }};
    // fs_ext12_api is frozen too (five members, 56 bytes; tests/test_merge_cpu.py); the fourteenth table lies behind it, and &all13.base12 is &all13.
    static const fs_hook_tables13 all13 = {all12, {
        FS_EXT13_MAGIC,
        sizeof(fs_ext13_api),
        fs_merge_view,
        fs_merge_gate,
        fs_link_correct,
        fs_mosaic_merge,
        fs_merge_patch,
        fs_link_place,
    }};
    // fs_ext13_api is frozen too (six members, 64 bytes; tests/test_change_cpu.py); the fifteenth table lies behind it, and &all14.base13 is &all14.
    static const fs_hook_tables14 all14 = {all13, {
        FS_EXT14_MAGIC,
        sizeof(fs_ext14_api),
        fs_mosaic_change,
    }};
    // fs_ext14_api is frozen too (one member, 24 bytes; tests/test_access_cpu.py); the sixteenth table lies behind it, and &all15.base14 is &all15.
    static const fs_hook_tables15 all15 = {all14, {
        FS_EXT15_MAGIC,
        sizeof(fs_ext15_api),
        fs_mask_access,
        fs_region_access,
    }};
    // fs_ext15_api is frozen too (two members, 32 bytes; tests/test_ground_cpu.py); the seventeenth table lies behind it, and &all16.base15 is &all16.
    static const fs_hook_tables16 all16 = {all15, {
        FS_EXT16_MAGIC,
        sizeof(fs_ext16_api),
        fs_ground_area,
        fs_ground_rectify,
        fs_ground_points,
    }};
    {
        const fs_hook_tables15& all15 = all16.base15;
        const fs_hook_tables14& all14 = all15.base14;
        const fs_hook_tables13& all13 = all14.base13;
        const fs_hook_tables12& all12 = all13.base12;
        const fs_hook_tables11& all11 = all12.base11;
        const fs_hook_tables10& all10 = all11.base10;
        const fs_hook_tables9& all9 = all10.base9;
        const fs_hook_tables8& all8 = all9.base8;
        const fs_hook_tables7& all7 = all8.base7;  // from here on both names mean the head of the whole object, not the copies it was built from
        const fs_hook_tables6& all6 = all7.base6;
        return all6.base5;
    }
}

FS_API const fs_test_api* fs_test_hooks(void) {
    const fs_hook_tables4& all4 = hook_tables().base4;  // the first five tables of the object; its address is the whole object's
    return &all4.base3.base2.base.test;
}
