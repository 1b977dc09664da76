/*
 * floodseg_test.h -- op-level hooks of libfloodseg.so: the building blocks behind the networks (implicit-GEMM conv, Winograd forms,
 * stem, pooling, attention, layout copies, the Segmenter's LayerNorm, Linear / split-K merges, qkv + attention, mask head, patchify
 * and token assembly, and the CNN heads' pyramid, classifier and concatenated-K shortcut kernels), for the parity tests
 * (tests/test_gpu_ops.py, tests/test_gpu_vit_ops.py, tests/test_gpu_head_ops.py) and the measurement tools (tools/).  The table
 * also carries EXTENSION OPS: product features that have no reference call site (block matching, flow/motion.py) and therefore no
 * place in the capped export list of floodseg.h; the Python package reaches them like any other function.  fs_test_api is frozen at
 * block_match; later extension ops (frame ingest, frame egress) are members of fs_ext_api, the table right behind it, and the ones
 * after those (block_match_modes, window_weights, seg_tail_weighted, crops_fuse_weighted, feat_tail_weighted, mask_confidence,
 * canvas_confidence, frame_report) of fs_ext2_api, the table behind both (end of this file).
 *
 * They are NOT part of the product's symbol surface (include/floodseg.h): the library exports ONE extra symbol, fs_test_hooks(), that
 * returns a table of function pointers.  The table was append-only up to block_match and is frozen now; `size` is sizeof(fs_test_api)
 * of the library that was built.  Conventions (device pointers, fs_stream, return codes,
 * fs_last_error) are those of floodseg.h.  No reference call site binds to anything in this file.
 */
#ifndef FLOODSEG_TEST_H_
#define FLOODSEG_TEST_H_

#include "floodseg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* conv2d `tile` argument: | FS_CONV_CHUNK_MAJOR = the filters are packed chunk-major ([O][I/32][KH][KW][32]) */
#define FS_CONV_CHUNK_MAJOR 0x400

typedef struct fs_test_api {
    size_t size;

    /* OIHW -> OHWI filter repack (what fs_finalize does once per conv) */
    int (*pack_conv_weight)(const float* oihw, float* ohwi, int O, int I, int KH, int KW, fs_stream stream);

    /* Conv2d (+ per-channel scale/shift, + residual, + ReLU (relu = 1) / GELU (2)) on the fp32 matrix cores; Cin % 32 == 0.
     * in/out/res are NHWC with pixel strides ld_*; wgt_ohwi from pack_conv_weight.  tile: 0 = cost-model choice, 1..4 force the
     * workgroup tile 128x128, 128x64, 64x64, 64x128 (tests / sweeps), optionally | FS_CONV_CHUNK_MAJOR.  Anything else is refused. */
    int (*conv2d_nhwc)(const float* in, int ld_in, const float* wgt_ohwi, const float* scale, const float* shift, const float* res,
                       int ld_res, float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       int dil, int relu, int tile, fs_stream stream);

    /* The same convolution with SPLIT operands: every fp32 filter value and every fp32 pixel is the exact sum of three bf16 terms
     * (round-to-nearest residues) and the six cross products of order <= 2^-16 run on the bf16 matrix cores with fp32 accumulation (the
     * three dropped ones are <= 2^-23 of the product: below the rounding of one fp32 add).  split_bf16x3 writes the three planes
     * (3 * n bf16, n % 8 == 0) of a packed filter bank; conv2d_nhwc_split takes them in place of wgt_ohwi (tiles 0..4 and 6 = 128x96,
     * which the cost model considers where 96 divides Cout: the Segmenter's Linears).
     * Non-finite and out-of-range operands (tests/test_gpu_ops.py::test_conv_non_finite_operands): the split is exact for every finite
     * fp32 value up to the largest bf16, |x| <= 3.3895e38 (and flushes nothing above 2^-110).  An operand that is +-inf, NaN, or finite
     * with 3.3895e38 < |x| <= FLT_MAX makes EVERY output it contributes to NaN on this route; the fp32-MFMA route (conv2d_nhwc,
     * FS_OPT_NO_SPLIT_BF16) follows IEEE like the reference's convolution.  On BOTH routes the fused ReLU epilogue is max(v, 0) and maps
     * a NaN to 0 (torch's F.relu keeps it): a caller that must detect corrupt frames checks its inputs. */
    int (*split_bf16x3)(const float* w, int64_t n, void* planes, fs_stream stream);
    int (*conv2d_nhwc_split)(const float* in, int ld_in, const void* wgt_planes, const float* scale, const float* shift, const float* res,
                             int ld_res, float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                             int pad, int dil, int relu, int tile, fs_stream stream);

    /* Multi-head attention of the Segmenter (segm/model/blocks.py:39-66): out[b][n][h*64 + d] = softmax_keys(q k^T * scale) v for
     * qkv = [B][N][3 * heads * 64] (q | k | v, head-major inside each third), head_dim 64.  split_operands = 0: fp32 matrix cores;
     * 1: the split-operand route (three bf16 terms per fp32 value of q, k, v and of the probabilities, bf16 matrix cores, fp32
     * accumulation and softmax).  workspace: attention_workspace_floats(B, N, heads, split_operands) floats. */
    size_t (*attention_workspace_floats)(int B, int N, int heads, int split_operands);
    int (*attention)(const float* qkv, float* out, int B, int N, int heads, float scale, int split_operands, float* workspace,
                     fs_stream stream);

    /* 3x3 stride-1 conv with padding == dilation as Winograd F(m x m,3x3) (transforms + (m+2)^2 grouped MFMA GEMMs); the networks use
     * it for every such conv with Cin >= 256.  tile_m: 3, 4, 6, or 0 = whichever needs the fewest GEMM rows for this map (a 90x90 map is
     * exactly 15x15 tiles of 6x6).  workspace: winograd_workspace_floats(..., same tile_m) floats of device memory. */
    size_t (*winograd_workspace_floats)(int B, int H, int W, int Cin, int Cout, int dil, int tile_m);
    int (*conv3x3_winograd_nhwc)(const float* in, int ld_in, const float* wgt_oihw, const float* scale, const float* shift, float* out,
                                 int ld_out, int B, int H, int W, int Cin, int Cout, int dil, int relu, int tile_m, float* workspace,
                                 fs_stream stream);

    /* 3x3 stride-1 pad-1 conv with FEW input channels (32 <= Cin <= 256, Cin % 32 == 0, Cout % 64 == 0) as ONE fused Winograd
     * F(4x4,3x3) kernel: input transform, the 36 position GEMMs on the fp32 matrix cores and the output transform (+ scale/shift,
     * ReLU) without the Winograd-domain tensors ever reaching HBM (the deep stem's 64-channel convs, conv2 of layer1:
     * model/resnet.py:110-116, 67-69).  workspace: winograd_fused_workspace_floats(Cin, Cout) floats (the packed filter bank, rebuilt by
     * every call of this test entry; the network builds it once at fs_finalize).  variant: 0 = by workgroup count, 2 = 16 tiles x 64
     * channels per workgroup (two workgroups per CU), 3 = 16 x 64 warp-specialised; all give bit-identical results.  1 (a retired
     * 32 x 64 form) and anything else are refused. */
    size_t (*winograd_fused_workspace_floats)(int Cin, int Cout);
    int (*conv3x3_winograd_fused_nhwc)(const float* in, int ld_in, const float* wgt_oihw, const float* scale, const float* shift, float* out,
                                       int ld_out, int B, int H, int W, int Cin, int Cout, int relu, int variant, float* workspace,
                                       fs_stream stream);
    /* the same conv (+ BatchNorm + ReLU) followed by MaxPool2d(3, stride 2, padding 1) as ONE launch (the deep stem's layer0.6 +
     * max-pool): pool = [B][(H-1)/2+1][(W-1)/2+1][Cout]; bit-identical to the two calls it replaces. */
    int (*conv3x3_winograd_fused_pool_nhwc)(const float* in, int ld_in, const float* wgt_oihw, const float* scale, const float* shift,
                                            float* pool, int B, int H, int W, int Cin, int Cout, float* workspace, fs_stream stream);

    /* stem convolution read from NCHW frames; wgt_hwio: [KH][KW][3][Cout] (weight.permute(2,3,1,0)).  _split: three bf16 terms per fp32
     * value on the bf16 matrix cores (what the network handles run unless FS_OPT_NO_SPLIT_BF16); Cout % 32 == 0, <= 128. */
    int (*stem_conv_nchw)(const float* in_nchw, const float* wgt_hwio, const float* scale, const float* shift, float* out_nhwc, int B,
                          int H, int W, int Cout, int KH, int KW, int stride, int pad, fs_stream stream);
    int (*stem_conv_nchw_split)(const float* in_nchw, const float* wgt_hwio, const float* scale, const float* shift, float* out_nhwc,
                                int B, int H, int W, int Cout, int KH, int KW, int stride, int pad, fs_stream stream);

    int (*maxpool3x3s2_nhwc)(const float* in, float* out, int B, int H, int W, int C, fs_stream stream);
    int (*adaptive_avgpool_nhwc)(const float* in, int ld_in, float* out, int B, int H, int W, int C, int bin, fs_stream stream);
    int (*nchw_to_nhwc)(const float* in, float* out, int B, int C, int HW, fs_stream stream);
    int (*nhwc_to_nchw)(const float* in, float* out, int B, int C, int HW, fs_stream stream);

    /* ---- Segmenter pieces (csrc/vit_ops.hip, vit_net.hip): the launchers and the Linear geometry the network itself runs.  Token
     * matrices are row-major [rows][D] fp32; weights of a Linear are [N][K] as torch stores them. */
    /* nn.LayerNorm(D) per row, eps 1e-5; 4 <= D <= 1024, D % 4 == 0.  drop_first != 0: rows = B * rows_per_batch and row 0 of every batch
     * (the cls token) is left out of `out`, which then holds B * (rows_per_batch - 1) rows in order (the encoder's final norm). */
    int (*layernorm)(const float* in, const float* gamma, const float* beta, float* out, int rows, int D, int rows_per_batch, int drop_first,
                     fs_stream stream);
    /* the split-K slice count the network chooses for a Linear (0 = none) from ONE image's rows; split_route: the split-operand filters */
    int (*linear_splits)(int K, int N, int rows_per_image, int act, int split_route);
    /* out[rows][N] = act(in[rows][K] @ w^T + bias (+ res)), act 0 / 1 (ReLU) / 2 (GELU); K % 32 == 0.  w_planes: split_bf16x3 of w (the
     * split-operand route), or NULL (fp32 matrix cores).  nsplit: 0 = the network's choice (linear_splits(K, N, rows_per_image or rows,
     * act, w_planes != NULL), only when `part` is given), 1 = no split, >= 2 (<= 16) = split-K forced (act 0, K % (32 nsplit) == 0).
     * part: nsplit * rows * N floats of partial products.  gamma / beta / ln_out (all or none, split-K only): the merge also writes
     * LayerNorm(gamma, beta) of `out` into ln_out (splitk_combine_ln, N <= 1024). */
    int (*linear)(const float* in, const float* w, const void* w_planes, const float* bias, const float* res, float* out, int rows, int K,
                  int N, int act, int nsplit, int rows_per_image, float* part, const float* gamma, const float* beta, float* ln_out,
                  fs_stream stream);
    /* The first half of a transformer block on the split-operand route: qkv_out[B * tokens][3D] = in @ w^T + bias, then multi-head
     * attention (head_dim 64, scale 1/8) into att_out[B * tokens][D].  fused = 1: the qkv Linear's epilogue writes the attention's K / V^T
     * operand planes (D % 96 == 0); 0: the plain Linear and the attention's own pre-pass.  workspace (16-B aligned):
     * qkv_attention_workspace_floats(B, tokens, D) floats; at byte 0 the K planes, bf16 [3][B * heads][Npad][64], then the V^T planes,
     * bf16 [3][B * heads][64][Npad] (Npad = tokens rounded up to 32; keys tokens .. Npad-1 are zeros), then the key-split scratch. */
    size_t (*qkv_attention_workspace_floats)(int B, int tokens, int D);
    int (*qkv_attention)(const float* in, const float* w, const void* w_planes, const float* bias, int B, int tokens, int D, float* qkv_out,
                         float* att_out, int fused, float* workspace, fs_stream stream);
    /* decoder mask head: pp, cc = [B][N + K][D]; out[b][k][i] = LayerNorm_K(<pp[b][i] / |pp[b][i]|, cc[b][N + k] / |cc[b][N + k]|>) (eps 1e-5),
     * NCHW; 1 <= K <= 64, D % 4 == 0, D <= 1024 */
    int (*mask_head)(const float* pp, const float* cc, const float* gamma, const float* beta, float* out, int B, int N, int K, int D,
                     fs_stream stream);
    /* zero-padded (right / bottom) P x P patches of NCHW frames -> [B * ceil(H/P) * ceil(W/P)][3 P P], columns (c, py, px); images
     * 0 .. B1-1 from in, B1 .. B-1 from in2 */
    int (*patchify)(const float* in, const float* in2, int B1, float* out, int B, int H, int W, int P, fs_stream stream);
    /* X[b][0] = cls + pos[0], X[b][1 + i] = emb[b * N + i] + pos[1 + i]; D % 4 == 0 */
    int (*vit_assemble)(const float* emb, const float* cls, const float* pos, float* X, int B, int N, int D, fs_stream stream);
    /* Z[b][i < N] = Y[b * N + i], Z[b][N + k] = cls_emb[k]; D % 4 == 0 */
    int (*dec_assemble)(const float* Y, const float* cls_emb, float* Z, int B, int N, int K, int D, fs_stream stream);
    /* ---- CNN heads and projection shortcut (csrc/net_ops.hip, net.hip): the launchers and the launch geometry the networks run. */
    /* out[o][0..Ka) = sa[o] * wa[o][:], out[o][Ka..Ka+Kb) = sb[o] * wb[o][:], shift_out[o] = ha[o] + hb[o] (one fp32 rounding each): the
     * filter bank and bias of BN_a(conv_a(x)) + BN_b(conv_b(y)) as one GEMM over the concatenated K (both convs 1x1, filters [O][K*]) */
    int (*concat_scaled_filters)(const float* wa, const float* sa, const float* ha, int Ka, const float* wb, const float* sb, const float* hb,
                                 int Kb, float* out, float* shift_out, int O, fs_stream stream);
    /* out[(tap * O + o) * nc + c] = oihw[o][c0 + c][tap]: the input-channel slice c0 .. c0 + nc - 1 of an [O][I][taps] bank as a
     * [taps * O][nc] 1x1 filter matrix (the pyramid levels' share of the PSPNet head conv); 0 <= c0, c0 + nc <= I */
    int (*pack_slice_tap_major)(const float* oihw, float* out, int O, int I, int c0, int nc, int taps, fs_stream stream);
    /* conv3 + projection shortcut of a bottleneck as ONE launch: out[b][y][x][:] = act(a[b][y][x][:] @ W[:, :Cin]^T +
     * b[b][y * stride2][x * stride2][:] @ W[:, Cin:]^T + shift), a = [B][Ho][Wo] x ld_a, b = [B][H2][W2] x ld_b with
     * (H2 - 1) / stride2 + 1 == Ho (same for W), W = [Cout][Cin + Cin2] from concat_scaled_filters; Cin, Cin2 multiples of 32.
     * wgt_planes: split_bf16x3 of W (the split-operand route) or NULL (fp32 matrix cores).  tile: 0 = cost-model choice, 1 = 128x128,
     * 2 = 128x64 (the only concatenated-K tiles); all give the same bits.  relu as conv2d_nhwc (the network passes 1). */
    int (*dual_conv)(const float* a, int ld_a, const float* b, int ld_b, const float* wgt, const void* wgt_planes, const float* shift, float* out,
                     int ld_out, int B, int Ho, int Wo, int Cin, int Cin2, int H2, int W2, int stride2, int Cout, int relu, int tile,
                     fs_stream stream);
    /* The pooling half of the PSPNet pyramid: AdaptiveAvgPool2d(1, 2, 3, 6) of an NHWC map into out = [B][1][C] | [B][4][C] | [B][9][C] |
     * [B][36][C] back to back (50 * B * C floats).  H and W multiples of 6: one pass over the map (6 x 6 cell means) + a combine of the
     * cells into bins 3, 2, 1; otherwise four adaptive_avgpool launches.  C % 32 == 0. */
    int (*pyramid_pool)(const float* in, int ld_in, float* out, int B, int H, int W, int C, fs_stream stream);
    /* 1..4 small-M 1x1 convs of one (K, N) in one launch (the pyramid levels' conv + BN + ReLU; ASPP's pooling branch): problem i computes
     * out[i][m][n] = act(scale[i][n] * <in[i][m], wgt[i][n]> + shift[i][n]) for m < M[i].  in / wgt / scale / shift / out / M are HOST
     * arrays of nprob entries (device pointers inside; scale / shift, or single entries of them, may be NULL = 1 / 0).  K % 256 == 0,
     * K <= 4096; rows are cut into min(12, max M / 6) chunks, the same cut for every problem. */
    int (*rowdot_batch)(int nprob, const float* const* in, const float* const* wgt, const float* const* scale, const float* const* shift,
                        float* const* out, const int* M, int ld_in, int ld_out, int K, int N, int relu, fs_stream stream);
    /* bilinear resize of a small map in = [B][hi * wi][C] into the C-channel slice that starts at `out` of an NHWC buffer
     * [B][Ho][Wo] x ld_out (out already points at the slice's first channel); C % 4 == 0, ld_out % 4 == 0, out 16-B aligned */
    int (*upsample_into)(const float* in, int hi, int wi, float* out, int ld_out, int B, int Ho, int Wo, int C, int align_corners,
                         fs_stream stream);
    /* classifier 1x1 conv + bias (NULL = none), NHWC in -> NCHW out [B][K][HW]; wgt = [K][C]; C % 4 == 0; the filters live in LDS:
     * K * C <= 16384, more is refused */
    int (*classifier_nchw)(const float* in, int ld_in, const float* wgt, const float* bias, float* out, int B, int HW, int C, int K,
                           fs_stream stream);
    /* The PSPNet head finish: logits[b][k][y][x] = cls_b[k] + <cls_w[k], act(scale * (T[b][y][x] + term[b][y][x]) + shift)> with
     * term = sum over the four levels of conv3x3(pad 1) of the align_corners = True upsampling of the level's pooled map, taken from
     * z_i = [B * bin_i^2][9][C] (cell-major, then tap (r, s), then channel): what the level's cells contribute per tap.  T = [B][H][W] x ld
     * raw head-conv sums, bins = 4 host ints (1..6 each, adding up to 12), scale / shift / cls_b may be NULL, C % 4 == 0, C <= 1024, any
     * K >= 1.  scratch: ppm_term_scratch_floats(B, H, C) floats. */
    size_t (*ppm_term_scratch_floats)(int B, int H, int C);
    int (*ppm_term_classify)(const float* T, int ld, const float* z1, const float* z2, const float* z3, const float* z6, const int* bins,
                             const float* scale, const float* shift, int B, int H, int W, int C, int relu, const float* cls_w, const float* cls_b,
                             float* logits, int K, float* scratch, fs_stream stream);
    /* The same preceded by the network's grouped Z GEMM: reduced = [4][B * 36][Cr] (level i's B * bin_i^2 rows first in its slot, the
     * rest of the slot is multiplied but never used), zw = [4][9 * C][Cr] from pack_slice_tap_major (zw_planes: split_bf16x3 of all of
     * it, or NULL for the fp32 matrix cores); Cr % 32 == 0.  workspace: ppm_head_workspace_floats(B, H, C) floats. */
    size_t (*ppm_head_workspace_floats)(int B, int H, int C);
    int (*ppm_head)(const float* T, int ld, const float* reduced, int Cr, const float* zw, const void* zw_planes, const int* bins,
                    const float* scale, const float* shift, int B, int H, int W, int C, int relu, const float* cls_w, const float* cls_b,
                    float* logits, int K, float* workspace, fs_stream stream);
    /* ---- Extension ops: product features that no reference call site binds to (the exported surface of floodseg.h is capped). */
    /* Full-search block matching (csrc/motion_ops.hip): cur, ref = two uint8 device frames of one size, luma [H][W] (channels = 1) or
     * RGB [H][W][3] (channels = 3, reduced to Y = (77 R + 150 G + 29 B + 128) >> 8); ref is the PAST frame.  Blocks are 16 x 16,
     * hb = H / 16, wb = W / 16 (a remainder strip belongs to no block but is searched).  For every block the winner among the
     * displacements |dx|, |dy| <= search (1..32) whose 16 x 16 window lies inside ref minimises, lexicographically,
     * (SAD + penalty (|dx| + |dy|), |dx| + |dy|, dy, dx), penalty 0..255.  mv = int32 [hb * wb][7], block raster order, rows
     * (-1, 16, 16, src_x, src_y, dst_x, dst_y) with dst = the block centre and src = dst + (dx, dy): the table fs_mv_to_grids takes.
     * cost = int32 [hb * wb] winning costs, or NULL.  Integer arithmetic throughout: results are exact.  This entry writes a winner's
     * row for every block; a table may also hold VOID ROWS (-1, 16, 16, -16, -16, -16, -16), "no vector for this block", which
     * fs_mv_to_grids skips: block_match_modes (fs_ext2_api, end of this file) writes them.  H, W >= 16 and
     * H * W * channels < 2^31; anything else is refused before a launch. */
    int (*block_match)(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int search, int penalty, int32_t* mv, int32_t* cost,
                       fs_stream stream);
} fs_test_api;

/* ---- The extension table.  fs_test_api above is FROZEN at block_match: its members, their order and its size never change again
 * (callers and tests pin them).  Extension ops added since live in a second, append-only table that the library places directly behind
 * it: fs_test_hooks() returns the address of fs_hook_tables.test, which is also the address of the fs_hook_tables object, so
 *     const fs_hook_tables* t = (const fs_hook_tables*)fs_test_hooks();   t->ext.frame_prepare(...)
 * A library built before this table existed returns a bare fs_test_api: a caller that may meet one checks t->ext.magic == FS_EXT_MAGIC
 * (and ext.size for the members it needs) before it uses the table; the Python package and the library are built together. */
#define FS_EXT_MAGIC 0x4653455854414231ull /* "FSEXTAB1" */

typedef struct fs_ext_api {
    uint64_t magic; /* FS_EXT_MAGIC */
    size_t size;    /* sizeof(fs_ext_api) of the library that was built */

    /* Frame ingest (csrc/ingest_ops.hip): one decoded uint8 device frame -> the network's input out = fp32 [3][h][w] (NCHW, one image; any
     * 4-byte aligned address, e.g. one image of a [B][3][h][w] tensor), in one launch.  Per output pixel and channel c:
     *   x = clamp(round_half_even(bilinear(rgb_c)), 0, 255);  out = (x - mean[c]) / std[c]   (fp32, true division)
     * where bilinear is the half-pixel (align_corners = 0) resize of fs_resize_bilinear_nchw, operation for operation, on the uint8 taps
     * as floats; when (h, w) == (H, W) the pixel is its own value (no rounding step is needed).  mean, std: 3 DEVICE floats each.
     * format 0 = RGB24: frame = interleaved [H][W][3], u = v = NULL.
     * format 1 = NV12: frame = Y [H][W], u = interleaved UV plane [ceil(H/2)][ceil(W/2)][2], v ignored.
     * format 2 = I420: frame = Y [H][W], u, v = [ceil(H/2)][ceil(W/2)] each.
     * Chroma is replicated: luma pixel (y, x) takes chroma sample (y >> 1, x >> 1); odd H and W are allowed.  YUV -> RGB is OUR DEFINITION,
     * in int32 with an arithmetic shift, each result clipped to [0, 255]; d = U - 128, e = V - 128:
     *   matrix 0 (BT.601), full_range 0: c = 298 (Y - 16); R = (c + 409 e + 128) >> 8; G = (c - 100 d - 208 e + 128) >> 8; B = (c + 516 d + 128) >> 8
     *   matrix 0 (BT.601), full_range 1: c = 256 Y;        R = (c + 359 e + 128) >> 8; G = (c -  88 d - 183 e + 128) >> 8; B = (c + 454 d + 128) >> 8
     *   matrix 1 (BT.709), full_range 0: c = 298 (Y - 16); R = (c + 459 e + 128) >> 8; G = (c -  55 d - 136 e + 128) >> 8; B = (c + 541 d + 128) >> 8
     *   matrix 1 (BT.709), full_range 1: c = 256 Y;        R = (c + 403 e + 128) >> 8; G = (c -  48 d - 120 e + 128) >> 8; B = (c + 475 d + 128) >> 8
     * H, W, h, w >= 1, H * W * 3 < 2^31 and h * w * 3 < 2^31; a null pointer (a chroma pointer the format needs included) and an unknown
     * format, matrix or range are refused before a launch. */
    int (*frame_prepare)(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int H, int W,
                         const float* mean, const float* std, float* out, int h, int w, fs_stream stream);

    /* Frame egress (csrc/egress_ops.hip): one mask -> one result video frame, in one launch.  mask = uint8 [h][w]; palette = uint8 [K][4],
     * (R, G, B, A) per class, 1 <= K <= 256.  Background (optional; frame = NULL, u = v = NULL, H = W = 0: none): one decoded uint8 frame
     * H x W described exactly as frame_prepare's input (format, u, v, matrix, full_range).  Per output pixel:
     *   c = mask < K ? mask : 0 (the rule of fs_colorize);  (R, G, B, A) = palette[c];
     *   b = the uint8 image the network saw: the source pixel through frame_prepare's path, operation for operation, up to but not
     *       including the normalisation (integer YUV -> RGB, half-pixel bilinear to h x w, round half to even, clamp to 0..255);
     *   per channel, int32: o = (A * colour + (255 - A) * b + 127) / 255 (integer division); without a background o = colour whatever A.
     * out_format 0 = RGB24: out = interleaved [h][w][3], out_u = out_v ignored.
     * out_format 1 = NV12: out = Y [h][w], out_u = interleaved UV plane [ceil(h/2)][ceil(w/2)][2], out_v ignored.
     * out_format 2 = I420: out = Y [h][w], out_u, out_v = [ceil(h/2)][ceil(w/2)] each.
     * Y comes from each pixel's own o; a chroma sample from the per-channel mean of its 2 x 2 quad, (sum of four + 2) >> 2, rows and
     * columns past the frame repeating the last one (odd h and w are allowed).  RGB -> YUV is OUR DEFINITION, in int32 with an arithmetic
     * shift, each result clipped to [0, 255]; every chroma row sums to 0, so a grey pixel gives U = V = 128 exactly (which is why the
     * BT.709 limited U row has -86 and not the nearest integer -87).  out_matrix / out_full_range need not equal the input's:
     *   out_matrix 0 (BT.601), out_full_range 0: Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16; U = ((-38 R - 74 G + 112 B + 128) >> 8) + 128; V = ((112 R - 94 G - 18 B + 128) >> 8) + 128
     *   out_matrix 0 (BT.601), out_full_range 1: Y = ((77 R + 150 G + 29 B + 128) >> 8) + 0; U = ((-43 R - 85 G + 128 B + 128) >> 8) + 128; V = ((128 R - 107 G - 21 B + 128) >> 8) + 128
     *   out_matrix 1 (BT.709), out_full_range 0: Y = ((47 R + 157 G + 16 B + 128) >> 8) + 16; U = ((-26 R - 86 G + 112 B + 128) >> 8) + 128; V = ((112 R - 102 G - 10 B + 128) >> 8) + 128
     *   out_matrix 1 (BT.709), out_full_range 1: Y = ((54 R + 183 G + 19 B + 128) >> 8) + 0; U = ((-29 R - 99 G + 128 B + 128) >> 8) + 128; V = ((128 R - 116 G - 12 B + 128) >> 8) + 128
     * The output buffers are the caller's, at any byte address (8-byte aligned planes and w % 8 == 0 take the wide stores).  Refused
     * before a launch: a null mask / palette / out, a null chroma pointer that a format needs (in or out), an unknown format, matrix or
     * range (in or out; checked with or without a background), K outside 1..256, h or w < 1, h * w * 3 >= 2^31 or H * W * 3 >= 2^31,
     * H / W / u / v given without a background frame, and a background frame with H or W < 1. */
    int (*frame_compose)(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                         int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                         int out_matrix, int out_full_range, fs_stream stream);
} fs_ext_api;

typedef struct fs_hook_tables {
    fs_test_api test;
    fs_ext_api ext;
} fs_hook_tables;

/* ---- The second extension table.  fs_ext_api is pinned as well (frame_prepare, frame_compose, 32 bytes: tests/test_ingest_cpu.py,
 * tests/test_egress_cpu.py), and so is the two-member fs_hook_tables.  Extension ops added since live in a THIRD table, append-only, that
 * the library places directly behind the two frozen ones: the object fs_test_hooks() points into is an fs_hook_tables2, and its address
 * is that of its fs_hook_tables and of its fs_test_api,
 *     const fs_hook_tables2* t = (const fs_hook_tables2*)fs_test_hooks();   t->ext2.block_match_modes(...)
 * A library built before this table existed returns an fs_hook_tables with nothing behind it: a caller that may meet one checks
 * t->base.ext.magic first, then t->ext2.magic == FS_EXT2_MAGIC and ext2.size >= the end of the member it needs.  Only the POSITION of a
 * member is fixed (block_match_modes is the first, at offset 16); the table grows at its end. */
#define FS_EXT2_MAGIC 0x4653455854414232ull /* "FSEXTAB2" */

typedef struct fs_ext2_api {
    uint64_t magic; /* FS_EXT2_MAGIC */
    size_t size;    /* sizeof(fs_ext2_api) of the library that was built */

    /* Block matching with an inter / intra decision per block and a scene-cut decision per frame pair (csrc/motion_ops.hip).  An
     * encoder sends no vector for an intra-coded macroblock and none at all for an I-frame, and the cells of such blocks keep the
     * identity grid (dataset/flow/extract_motion_vectors.py:21-43); block_match emits a winner for every block, however bad.  This
     * entry makes the two decisions on the device and expresses them as the reference's data does: as vectors that are not there.
     * Integer arithmetic throughout: results are exact.
     *
     * cur, ref, H, W, channels, search, penalty, the luma, the 16 x 16 blocks of cur, the candidate window and the WINNER are
     * block_match's, unchanged: the lexicographic minimum of (SAD + penalty (|dx| + |dy|), |dx| + |dy|, dy, dx).  Per block:
     *   S        = the sum of the block's 256 luma values;  m = (S + 128) >> 8
     *   activity = sum over the block of |Y - m|            (0..32640: the DC-intra cost)
     *   sad      = winning cost - penalty (|dx| + |dy|)     (the winner's plain SAD, 0..65280)
     *   intra    <=>  sad > activity + intra_bias           intra_bias 0..65535; from 65280 on no block is ever intra
     * Per frame pair, with blocks = hb * wb and intra_blocks the number of intra blocks:
     *   cut      <=>  intra_blocks * 1000 > cut_permille * blocks      cut_permille 0..1000; 1000 can never cut
     * mv = int32 [hb * wb][7], block raster order, as block_match's.  The row of an inter block is block_match's row.  The row of an
     * intra block -- on a cut, EVERY row -- is the VOID ROW (-1, 16, 16, -16, -16, -16, -16): its source and destination block indices
     * floor-divide to -1, so fs_mv_to_grids skips it in both directions (the reference's two range checks) and the cells it would have
     * owned keep the identity grid.  No compaction, no data-dependent sizes, no synchronisation.
     * Side outputs, each optional (NULL skips it):
     *   cost     = int32 [hb * wb] winning costs as block_match's, for intra blocks too;
     *   activity = int32 [hb * wb];
     *   stats    = int32 [4] = {blocks, intra_blocks (counted before the cut rule), cut as 0 | 1, 0}, written whole by every call (on the
     *              stream; nothing accumulates), so a HIP-graph replay on new frames gives that replay's figures.
     * The right intra_bias depends on the sensor's noise: on flat, noisy water sad is about 1.4 x activity, so bias 0 marks such
     * blocks intra.  Refused before a launch: what block_match refuses (a null cur / ref / mv included), intra_bias outside 0..65535,
     * cut_permille outside 0..1000. */
    int (*block_match_modes)(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int search, int penalty, int intra_bias,
                             int cut_permille, int32_t* mv, int32_t* cost, int32_t* activity, int32_t* stats, fs_stream stream);

    /* Per-frame blend weights of one key-frame window from the cut flags of its frame pairs (csrc/motion_ops.hip): what lets the tails
     * HOLD one key frame across a detected scene cut instead of blending two scenes.  OUR DEFINITION.  The window has frames 0..n:
     * frame 0 is the previous key frame, frame n the next one (not emitted), 1 <= n <= 64.  stats = a HOST array of n DEVICE pointers,
     * stats[j - 1] for the pair (j-1 -> j), j = 1..n, each an int32 [4] as block_match_modes writes it (cut at index 2); a NULL entry
     * -- or stats == NULL -- means "not estimated: no cut".  Outputs, both on the device, written whole by one launch of one small
     * workgroup (no atomics, nothing read on the host, so a HIP-graph replay on new stats gives that replay's weights):
     *   weights = float [n][2] = (wa, wb) per emitted frame f = 0..n-1;  source = int32 [n].
     * With first / last the smallest / largest j whose pair is a cut:
     *   no cut:              wa = (float)((double)(n - f) / n), wb = (float)((double)f / n), source 0 (the linear blend, bit for bit
     *                        the expression the tails evaluate without weights)
     *   f < first:           (1, 0), source 1: held from the previous key frame
     *   f >= last:           (0, 1), source 2: held from the next key frame
     *   first <= f < last:   a scene neither key frame shows: (1, 0) if 2 f <= n, else (0, 1); source 3
     * Frame 0 is (1, 0) in every case.  Refused before a launch: n < 1, n > 64, a null output. */
    int (*window_weights)(int n, const int32_t* const* stats, float* weights, int32_t* source, fs_stream stream);

    /* fs_seg_tail and fs_seg_tail_accumulate (floodseg.h) in one entry, with per-frame blend weights: every argument means what it
     * means there (out_logits / out_mask: fs_seg_tail's outputs, each optional; canvas / count / cH / cW / y0 / x0: the sliding-crop
     * canvas of fs_seg_tail_accumulate, canvas == NULL: none), through the same launch function.  weights = device float [n][2] as
     * window_weights writes it, or NULL: the existing entries' result, bit for bit.  For frame f >= 1 with (wa, wb) = weights[f]:
     *   wb == 0: v = va;   else wa == 0: v = vb;   else v = fadd_rn(fmul_rn(wa, va), fmul_rn(wb, vb))
     * va / vb being the previous / next key frame's chain at that pixel (the warp chain, or the upsampled logits when no_warp).  A held
     * frame is exactly one chain's value: no 0 * x term, so no sign of a zero and no non-finite value leaks from the unused chain.
     * Frame 0 never reads its weights.  Warp chains, upsample, argmax, softmax and the float64 canvas are the unweighted tail's. */
    int (*seg_tail_weighted)(const float* lo_prev, const float* lo_next, const float* const* grids_left, const float* const* grids_right, int K,
                             int h, int w, int Hg, int Wg, int H, int W, int n, int no_warp, float* out_logits, uint8_t* out_mask, double* canvas,
                             double* count, int cH, int cW, int y0, int x0, float* scratch, const float* weights, fs_stream stream);

    /* fs_crops_fuse (floodseg.h) with the same per-frame weights: its arguments, then weights (device float [n][2], or NULL: the result
     * of fs_crops_fuse).  Bit-identical to seg_tail_weighted in canvas mode per crop, in crop order, followed by fs_canvas_finish. */
    int (*crops_fuse_weighted)(const float* lo_prev, const float* lo_next, const float* crop_grids, int ncrops, const int* crop_y,
                               const int* crop_x, int K, int h, int w, int Hg, int Wg, int ch, int cw, int n, int no_warp, double* canvas,
                               uint8_t* mask, int H, int W, float* scratch, const float* weights, fs_stream stream);

    /* fs_feat_tail (floodseg.h) with the same per-frame weights: its arguments, then weights (device float [n][2] as window_weights
     * writes it, or NULL: the result of fs_feat_tail, bit for bit, through the same launch function).  For map p >= 1 of the decoder's
     * batch with (wa, wb) = weights[2p], weights[2p+1]:
     *   wb == 0: r = va;   else wa == 0: r = vb;   else r = fadd_rn(fmul_rn(wa, va), fmul_rn(wb, vb))
     * va / vb being the previous / next key frame's value at that element: in warp mode the upsampled forward map p-1 / backward map
     * n-p-1 of the warp chains (the map itself when the grid has the feature size), with no_warp f_prev / f_next.  A held map is exactly
     * one chain's value: no 0 * x term, so neither the sign of a zero nor a NaN / Inf of the unused chain reaches it, and in warp mode
     * the unused chain's rows are not read (half the tap loads of a blended map).  Map 0 never reads its weights (the key map through
     * the default grid, or 1 * f_prev with no_warp); both warp chains are still computed; weights is ignored when f_next == NULL or
     * n == 1.  Refused before a launch, here and by fs_feat_tail: a NULL entry among the n-1 grids of a direction (warp mode, two key
     * frames), and fh * fw * C >= 2^32 in warp mode (the key map's tap offsets are 32-bit element offsets). */
    int (*feat_tail_weighted)(const float* f_prev, const float* f_next, int C, int fh, int fw, const float* const* grids_left,
                              const float* const* grids_right, int Hg, int Wg, const float* grid0, int H0, int W0, int n, int no_warp,
                              float* stack, float* scratch, const float* weights, fs_stream stream);

    /* Per-pixel confidence from fp32 logits (csrc/conf_ops.hip).  OUR DEFINITION: the reference emits hard masks only.  logits =
     * float [n][K][h][w] (NCHW, what the tails write as logits), 1 <= K <= 32; mask, confidence = uint8 [n][H][W], both written by one
     * launch, at any byte address (dword stores when W % 4 == 0 and both are 4-byte aligned, byte stores otherwise).  Per output pixel:
     *   v[k]  = the align_corners=True bilinear value fs_resize_argmax_u8 takes the argmax of (the same index, weight and
     *           interpolation arithmetic in the same order); with (H, W) == (h, w) the logit itself, read directly
     *   mask  = the first maximum of v: with a resize fs_resize_argmax_u8's rule (the first k whose v[k] exceeds -inf and that no later
     *           k exceeds), at equal sizes fs_argmax_u8's (class 0 until a later value exceeds it).  The two differ on NaNs only.
     *   p     = the fp32 softmax over the K values as the tails and fs_softmax_accumulate compute it: m = max v, e[k] = expf(v[k] - m),
     *           s = e[0] + e[1] + ... in class order, p[k] = e[k] / s
     *   c     = p[mask];   confidence = c == c ? min(255, max(0, round-half-even(255.f * c))) : 0     (product and rounding in fp32)
     * So K == 1 gives 255, K equal logits give round(255 / K) with mask 0, and a NaN among a pixel's values gives 0.
     * Refused before a launch: a null pointer, n, h, w, H or W < 1, n > 65535, K outside 1..32, h * w or H * W >= 2^31. */
    int (*mask_confidence)(const float* logits, int n, int K, int h, int w, uint8_t* mask, uint8_t* confidence, int H, int W, fs_stream stream);

    /* The same two planes from the float64 crop-averaged canvas [n][K][h][w] (mean class probabilities, already divided by the crop
     * count: what fs_crops_fuse / fs_canvas_finish leave).  OUR DEFINITION.  1 <= K <= 255.  Per output pixel:
     *   v[k]  = the float64 align_corners=True bilinear value fs_canvas_resize_argmax takes the argmax of (same arithmetic, at equal
     *           sizes too: the canvas value itself for finite data; a NaN reaches the neighbours whose zero-weight taps read it)
     *   mask  = fs_canvas_resize_argmax's: the first k whose v[k] exceeds -inf and that no later k exceeds (0 when there is none)
     *   c     = v[mask];   confidence = c == c ? clamp(rint(255.0 * c), 0, 255) : 0                  (in double)
     * Stores and refusals as mask_confidence's (K outside 1..255). */
    int (*canvas_confidence)(const double* canvas, int n, int K, int h, int w, uint8_t* mask, uint8_t* confidence, int H, int W, fs_stream stream);

    /* Per frame and class, the extent and how far it can be trusted (csrc/conf_ops.hip).  OUR DEFINITION.  mask, confidence = uint8
     * [n][H][W]; 1 <= K <= 255; 0 <= low <= 255.  report = int64 [n][K][3]:
     *   report[f][k] = (pixels of frame f with mask == k,  the sum of their confidence codes,  those of them with confidence < low)
     * Mask ids >= K are counted nowhere: a frame's pixel counts then sum to less than H * W, which is how a caller sees them.
     * confidence == NULL: the pixel counts only, the other two columns zero.  Every call writes the whole report (it is zeroed on the
     * stream first), so the caller never clears it and a HIP-graph replay on new masks gives that replay's figures.  Integers
     * throughout: exact, whatever the order.  Refused before a launch: a null mask or report, n, H or W < 1, n > 65535, K or low out of
     * range, H * W >= 2^31 - 16384. */
    int (*frame_report)(const uint8_t* mask, const uint8_t* confidence, int n, int H, int W, int K, int low, int64_t* report, fs_stream stream);

    /* ---- Connected regions of a mask (csrc/region_ops.hip, csrc/region_uf.h).  OUR DEFINITION: the reference emits hard
     * masks only.  Integers throughout; every result is a function of the inputs alone, whatever order threads arrive in.
     *   mask         uint8 [n][H][W];  1 <= K <= 255;  connectivity 4 or 8.
     *   background   a pixel with id >= K (what frame_report counts nowhere): no region, label 0, index -1, never changed, never votes.
     *   region       a maximal set of pixels of ONE frame with the same id < K, connected under the connectivity (4: the edge
     *                neighbours; 8: the corner neighbours as well).  Frames never connect.
     *   anchor       the region's first pixel in raster order, (y_a, x_a).
     *   label        1 + (y_a * W + x_a): canonical -- a function of the mask alone, whatever algorithm found the regions.
     *
     * mask_regions writes labels = int32 [n][H][W] (whole), in three launches on the stream: a union-find per 32 x 64 tile in LDS, a
     * pass over the tile edges (find + atomic minimum on the plane itself; at 8 the diagonal pairs at tile corners too), and a pass
     * that replaces every cell by its root's label.  parent <= own index always holds, so a find strictly descends and a failed
     * union retries from a strictly smaller index: no loop waits for another thread, and nothing is iterated until stable.
     * No workspace.  Refused before a launch: a null pointer, n, H or W < 1, n > 65535, K outside 1..255, connectivity not 4 or 8,
     * H * W >= 2^31 - 1, ceil(H / 32) * ceil(W / 64) >= 2^24 (a frame of 2^24 tiles: thinner than a tile and over 2^29 pixels long). */
    int (*mask_regions)(const uint8_t* mask, int n, int H, int W, int K, int connectivity, int32_t* labels, fs_stream stream);

    /* The regions of each frame as a table, from the mask and mask_regions' labels (any plane of canonical labels of that mask).
     *   table  = int64 [n][max_regions][10], rows in ascending anchor (= label) order:
     *            (class, area, x0, y0, x1, y1, sum_x, sum_y, conf_sum, low_pixels) -- the bounding box inclusive; sum_x / sum_y the sums
     *            of the pixels' coordinates (centroid = sum / area: the caller divides, the kernel does not); conf_sum the sum of the
     *            region's confidence codes, low_pixels its pixels with confidence < low (0 <= low <= 255); both 0 when confidence ==
     *            NULL.  confidence = uint8 [n][H][W] as mask_confidence writes it.
     *   counts = int64 [n][2] = (regions in the frame, rows written = min(regions, max_regions)).
     *   index  = int32 [n][H][W]: per pixel the row of its region; -1 for background and for regions beyond max_regions, which get no
     *            row (the caller sees counts[f][0] > max_regions).
     * Every call writes its three outputs whole: the table is zeroed on the stream first, so rows at and behind counts[f][1] are zero
     * and a HIP-graph replay on new masks gives that replay's figures.  1 <= max_regions <= 65536.
     * workspace = int32 [n][ceil(H * W / 1024)] (per-chunk anchor counts, scanned in place), the caller's; nothing is allocated and
     * nothing is read on the host.  Refused before a launch: a null pointer (confidence may be NULL), what mask_regions refuses about
     * n, H, W and K, low outside 0..255, max_regions outside 1..65536. */
    int (*region_table)(const uint8_t* mask, const int32_t* labels, const uint8_t* confidence, int n, int H, int W, int K, int low, int max_regions,
                        int64_t* table, int64_t* counts, int32_t* index, int32_t* workspace, fs_stream stream);

    /* Despeckle: one pass of an area filter over region_table's result.  A SPECKLE is a region with a row and area < min_area.  Its
     * replacement class is the class with the most VOTES, a vote being a pair (pixel p of the speckle, in-frame 4-neighbour q of p)
     * where q's region has a row and area >= min_area; the vote goes to q's class.  Ties go to the lowest class id; with no vote the
     * speckle stays as it is.  All votes read the INPUT mask: one pass, not iterated; out differs from mask on speckle pixels only.  (A
     * 4-neighbour of the same class is in the same region under either connectivity, so a speckle never votes for itself; regions
     * beyond max_regions are neither speckles nor voters.)  min_area <= 1 gives the input bit for bit.
     * out = uint8 [n][H][W] at any byte address (dword stores when W % 4 == 0 and out is 4-byte aligned, byte stores otherwise), not
     * the input plane.  votes = int32 [n][max_regions][K], the caller's workspace, zeroed on the stream by the call; afterwards a
     * row's first cell holds its replacement class (-1: none).  Refused before a launch: a null pointer, what mask_regions refuses
     * about n, H, W and K, max_regions outside 1..65536, min_area < 0. */
    int (*region_filter)(const uint8_t* mask, const int32_t* index, const int64_t* table, int n, int H, int W, int K, int max_regions, int min_area,
                         uint8_t* out, int32_t* votes, fs_stream stream);

    /* ---- Region identity across frames (csrc/track_ops.hip, csrc/track_defs.h).  OUR DEFINITION.  Integers throughout;
     * every result is a function of the inputs alone, whatever the hash function and whatever order threads arrive in.  R = max_regions.
     * Two consecutive frames f-1 and f, both with region_table's index plane, table and counts at the same R:
     *   overlap(a, b)  the number of pixels p with index[f-1][p] == a and index[f][p] == b, a a row of frame f-1 (0 <= a < its
     *                  counts[1]) and b a row of frame f, BOTH ROWS OF THE SAME CLASS (table column 0).  Pixels are compared in place:
     *                  no motion compensation.  Background and regions past the cap (index -1) take no part.
     *   back[f][b]     (a, overlap(a, b)) for the row a with the largest overlap with b, the lowest a on a tie; (-1, 0) when that
     *                  overlap is below min_overlap (>= 1).
     *   fwd[f][a]      the same from the other side, indexed by the rows of frame f-1: (b, overlap(a, b)) for the row b of frame f with
     *                  the largest overlap with a, the lowest b on a tie; (-1, 0) likewise.
     *   pairs          the distinct (a, b) with overlap >= 1 are counted in a table of max_pairs slots, a power of two in 16 .. 2^20.
     *                  A frame pair OVERFLOWS exactly when it has more than max_pairs such pairs (an insertion probes every slot
     *                  before it gives up); then back[f] and fwd[f] are (-1, 0) throughout.
     * region_links: index = int32 [n][H][W], table = int64 [n][R][10], counts = int64 [n][2].  Frame f >= 1 is linked to frame f-1 of
     * the call, frame 0 to the frame prev_index [H][W] / prev_table [R][10] / prev_counts [2]; these three are all NULL when there is
     * none, and frame 0 then gets (-1, 0) throughout and link_counts (0, 0).  Outputs, each written whole by every call (so a HIP-graph
     * replay on new planes gives that replay's links):
     *   back, fwd    = int32 [n][R][2]
     *   link_counts  = int64 [n][2] = (pairs stored, overflow 0 | 1); an overflowing pair stores max_pairs.
     * workspace = FS_REGION_LINKS_WORKSPACE_BYTES(n, R, max_pairs) bytes at an 8-byte aligned address, the caller's: per frame the
     * keys (8 B x max_pairs), the packed best values (8 B x 2 R), two 32-bit figures and the pair counts (4 B x max_pairs).  It is
     * cleared on the stream; nothing is allocated, synchronised or read on the host.
     * Refused before a launch: a null pointer (prev_* may be NULL together), prev_* given in part, n, H or W < 1, n > 65535, R outside
     * 1..65536, max_pairs not a power of two in 16 .. 2^20, min_overlap < 1, H * W >= 2^31 - 1, a workspace not aligned to 8 bytes. */
#define FS_REGION_LINKS_WORKSPACE_BYTES(n, R, max_pairs) ((size_t)(n) * (12 * (size_t)(max_pairs) + 16 * (size_t)(R) + 8))
    int (*region_links)(const int32_t* index, const int64_t* table, const int64_t* counts, const int32_t* prev_index, const int64_t* prev_table,
                        const int64_t* prev_counts, int n, int H, int W, int max_regions, int max_pairs, int min_overlap, int32_t* back, int32_t* fwd,
                        int64_t* link_counts, void* workspace, fs_stream stream);

    /* Track ids from region_links' result.  Row b of frame f CONTINUES row a of frame f-1 exactly when back[f][b].row == a >= 0,
     * fwd[f][a].row == b and a has a track; it then has a's track id and a's parent id.  Every other region with a row (b <
     * counts[f][1]) is BORN: the born regions of a frame take the ids next_id, next_id + 1, ... in ascending row order, next_id
     * advances by their number, and a born region's parent is the track id of back[f][b].row, -1 when it has none.  So a split leaves
     * the larger piece on the old track and the others born with that parent; a merge continues the larger contributor and the other
     * track ends, its fwd pointing into the merged region; no id occurs twice in a frame.
     *   tracks = int64 [n][R][4] = (track id, parent id, previous row, overlap with it), the last two back[f][b] as given; rows at and
     *            behind counts[f][1] are (-1, -1, -1, 0).  Written whole.
     *   prev_tracks = int64 [R][4], the tracks row of the frame before frame 0, or NULL: every region of frame 0 is then born with
     *            parent -1.   state = int64 [2] = (next id, 0) on the device, read and updated (ids count from 0 and never restart).
     * Two launches: the rows without a region are filled in parallel, then one workgroup walks the frames in order.  Refused before a launch: a null pointer (prev_tracks may be NULL),
     * n < 1, n > 65535, R outside 1..65536. */
    int (*region_tracks)(const int32_t* back, const int32_t* fwd, const int64_t* counts, const int64_t* prev_tracks, int n, int max_regions,
                         int64_t* state, int64_t* tracks, fs_stream stream);

    /* region_links with MOTION COMPENSATION: the frame before is read at every pixel's SOURCE under the block matcher's vectors, so a
     * region that moves further than its own width between two frames still overlaps itself.  Integers throughout; // is floor division.
     * Inputs as region_links', and on top:
     *   mv         = int32 [n][hb * wb][7], mv[f] the table of frame f against frame f-1 as block_match / block_match_modes write it,
     *                measured on a decoded frame of frame_h x frame_w pixels (FH x FW below), hb = FH // 16, wb = FW // 16.  The mask
     *                (H x W) and the decoded frame need not have the same size.  mv[0] is used only when prev_* is given.
     *   pair_stats = int32 [n][4], rows as block_match_modes writes its stats, or NULL.
     * For pixel (y, x) of frame f:
     *   its centre in the frame   fy = ((2y + 1) FH) // (2H), fx = ((2x + 1) FW) // (2W)
     *   its block                 by = fy // 16, bx = fx // 16; a pixel of the remainder strip (by >= hb or bx >= wb) has shift (0, 0)
     *   its row                   r = mv[f][by * wb + bx]; a VOID row (r[5] < 0 or r[6] < 0; the matcher's void row is
     *                             (-1, 16, 16, -16, -16, -16, -16)) has shift (0, 0); otherwise vx = r[3] - r[5], vy = r[4] - r[6]
     *                             (source minus destination: where the block was in the frame before), and a row with |vx| or |vy| >
     *                             1024 counts as void.  The differences are taken in 64 bits: ANY seven ints are a valid row.
     *   its shift in mask pixels  sx = sign(vx) ((2 |vx| W + FW) // (2 FW)), sy = sign(vy) ((2 |vy| H + FH) // (2 FH)): nearest, ties
     *                             away from zero
     *   its source                (y + sy, x + sx); a pixel whose source lies outside the mask takes no part
     *   overlap(a, b)  the number of pixels p of frame f with index[f][p] == b, a source s(p) inside the mask and index[f-1][s(p)] == a;
     *                  both rows exist and are of the same class.  Several pixels may share a source, so the overlaps of a row a can add
     *                  up to more than a's area; overlap(a, b) <= area(b) always holds.
     * back, fwd, min_overlap, the pair table, its overflow rule, the tie rules and link_counts[f][0] are region_links', word for word.
     * SCENE CUTS: where pair_stats is given and pair_stats[f][2] != 0 the pair gets no links at all -- back[f] and fwd[f] are (-1, 0)
     * throughout and link_counts[f] = (0, 2): on a cut block_match_modes voids every row, and regions of two unrelated scenes would be
     * compared in place.  Column 1 of link_counts is a flag word for this op: bit 0 overflow, bit 1 cut.  (Frame 0 without prev_* has no
     * pair: (0, 0) as in region_links.)
     * Consequences: with every row void, or every vector 0, all three outputs equal region_links' bit for bit; with H, W == FH, FW the
     * shift is the vector itself; for n == 1 the outputs equal region_links on a previous index plane warped beforehand (a gathered at
     * the source, -1 where the source is outside).
     * workspace = FS_REGION_LINKS_MC_WORKSPACE_BYTES(n, R, max_pairs, hb, wb) bytes at an 8-byte aligned address: region_links' and, behind
     * it, one packed dword per block and frame (sy << 16 | sx in 16-bit halves), written by a pass of its own so that the overlap pass
     * reads one dword per pixel.  Five launches (zero, shifts, overlap, best, unpack); nothing is allocated, synchronised or read on the
     * host; every output is written whole.
     * Refused before a launch: everything region_links refuses; a null mv; frame_h or frame_w < 16; frame_h * frame_w >= 2^31; H > 31
     * frame_h or W > 31 frame_w (a shift is at most 1024 * 31 + 1/2 mask pixels then and fits its 16 bits). */
#define FS_REGION_LINKS_MC_WORKSPACE_BYTES(n, R, max_pairs, hb, wb) \
    (FS_REGION_LINKS_WORKSPACE_BYTES(n, R, max_pairs) + (((size_t)(n) * (size_t)(hb) * (size_t)(wb) * 4 + 7) / 8) * 8)
    int (*region_links_mc)(const int32_t* index, const int64_t* table, const int64_t* counts, const int32_t* prev_index, const int64_t* prev_table,
                           const int64_t* prev_counts, const int32_t* mv, const int32_t* pair_stats, int n, int H, int W, int frame_h, int frame_w,
                           int max_regions, int max_pairs, int min_overlap, int32_t* back, int32_t* fwd, int64_t* link_counts, void* workspace,
                           fs_stream stream);
} fs_ext2_api;

typedef struct fs_hook_tables2 {
    fs_hook_tables base;
    fs_ext2_api ext2;
} fs_hook_tables2;

/* ---- The FOURTH table.  fs_ext2_api is frozen as well (14 members, 128 bytes; tests/test_tracks_mc_cpu.py), so ops added since live in
 * a table of their own, append-only, that the library places directly behind fs_hook_tables2 by the same pattern: the object
 * fs_test_hooks() points into is an fs_hook_tables3, and its address is that of its fs_hook_tables2,
 *     const fs_hook_tables3* t = (const fs_hook_tables3*)fs_test_hooks();   t->ext3.region_outlines(...)
 * A library built before this table existed has nothing behind its fs_hook_tables2: a caller that may meet one checks
 * t->base2.ext2.magic == FS_EXT2_MAGIC and ext2.size == sizeof(fs_ext2_api) first, then t->ext3.magic == FS_EXT3_MAGIC and ext3.size >=
 * the end of the member it needs. */
#define FS_EXT3_MAGIC 0x4653455854414233ull /* "FSEXTAB3" */

typedef struct fs_ext3_api {
    uint64_t magic; /* FS_EXT3_MAGIC */
    size_t size;    /* sizeof(fs_ext3_api) of the library that was built */

    /* ---- Region outlines (csrc/outline_ops.hip, csrc/outline_defs.h).  OUR DEFINITION.  Integers throughout; every result
     * is a function of the inputs alone, whatever order threads arrive in.  R = max_regions.
     * Inputs:
     *   index         int32 [n][H][W] as region_table writes it: a pixel holds the row r of its region, 0 <= r < R, or -1 (background,
     *                 regions past the cap).  Any value outside 0 .. R - 1 counts as -1.  Pixels with index -1 own no cracks.
     *   connectivity  4 or 8, the one the labels were made with.
     * CRACKS.  A lattice corner is (X, Y), 0 <= X <= W, 0 <= Y <= H.  A crack is a unit edge of a pixel p = (x, y) with index[p] = r >= 0
     * whose 4-neighbour across that edge lies outside the frame or has an index different from r.  It is directed so that p is on its
     * right, and has the slot id 4 * (y * W + x) + d:
     *   d = 0  top     heading east    (x, y)         -> (x + 1, y)
     *   d = 1  right   heading south   (x + 1, y)     -> (x + 1, y + 1)
     *   d = 2  bottom  heading west    (x + 1, y + 1) -> (x, y + 1)
     *   d = 3  left    heading north   (x, y + 1)     -> (x, y)
     * so an outer boundary runs clockwise on the screen.
     * SUCCESSOR.  The successor of a crack of r that ends at corner V is the crack of r that starts at V.  There are two such cracks only
     * at a SADDLE, where r holds two diagonal pixels at V and neither of the other two: at connectivity 8 the successor is the left turn
     * (onto the diagonal pixel), at 4 the right turn (the same pixel's next edge).  The successor is a permutation of the cracks; its
     * cycles are the CONTOURS.
     * VERTICES.  A run start is a crack whose predecessor has another direction; its vertex is its start corner.  A contour's ANCHOR is
     * the smallest slot id among its run starts.  Its vertex list starts at the anchor's vertex, follows the successor order, holds one
     * entry per run start and is not closed.  The contours of a frame are ordered by ascending anchor.  A region's outer contour has the
     * anchor 4 * (label - 1): the top edge of its first pixel is a run start and the region's smallest slot.
     * Outputs, each written whole by every call (so a HIP-graph replay on new planes gives that replay's figures):
     *   contours = int64 [n][max_contours][6], rows in contour order, zero behind the last written row:
     *              (region row, first vertex offset, vertex count, cracks = the contour's length, area2, anchor).
     *              area2 = sum of x0 y1 - x1 y0 over the vertices as a closed polygon: positive for an outer contour, negative for a
     *              hole.  Offsets are the exclusive prefix sums of the vertex counts over ALL contours of the frame, in contour order.
     *   vertices = int32 [n][max_vertices][2] = (X, Y), the lists of all contours concatenated in contour order, those without a row
     *              included; zero behind the total.
     *   shape    = int64 [n][R][3] = per region row (perimeter = its cracks, contours, vertices); contours - 1 is its number of holes.
     *              Rows without a region are zero.
     *   counts   = int64 [n][4] = (contours, contour rows written, vertices, flags).
     * OVERFLOW.  Flag bit 0: the frame has more than max_vertices vertices.  It gets nothing rather than an arbitrary part (the pair
     * table's rule, region_links): contours and vertices are zero, counts = (0, 0, vertices, 1), and the contours column of shape is -1
     * in every row that has a region (perimeter > 0); perimeter and vertices of shape are local sums and stay valid.  Flag bit 1: more
     * than max_contours contours; the first max_contours get rows, and all vertex lists are still written.
     * workspace = FS_REGION_OUTLINES_WORKSPACE_BYTES(n, H, W, R, max_contours, max_vertices) bytes at an 8-byte aligned address, the
     * caller's: per frame 44 bytes per possible vertex, 4 per 1024 pixels, 8 per 1024 possible vertices and 16.  Nothing is allocated,
     * synchronised or read on the host; the 11 + ceil(log2 max_vertices) launches capture into a HIP graph.
     * Refused before a launch: a null pointer; n, H or W < 1; n > 65535; H * W >= 2^29 (slot ids are 32-bit); R outside 1..65536;
     * connectivity other than 4 or 8; max_contours outside 1..2^20; max_vertices outside 4..2^22; a workspace not aligned to 8 bytes. */
#define FS_REGION_OUTLINES_WORKSPACE_BYTES(n, H, W, R, max_contours, max_vertices)                                                     \
    ((size_t)(n) * 8 * (2 * (size_t)(max_vertices) + 7 * (((size_t)(max_vertices) + 1) / 2) +                                        \
                        (((size_t)(H) * (size_t)(W) + 1023) / 1024 + 1) / 2 + ((size_t)(max_vertices) + 1023) / 1024 + 2))
    int (*region_outlines)(const int32_t* index, int n, int H, int W, int max_regions, int connectivity, int max_contours, int max_vertices,
                           int64_t* contours, int32_t* vertices, int64_t* shape, int64_t* counts, void* workspace, fs_stream stream);
} fs_ext3_api;

typedef struct fs_hook_tables3 {
    fs_hook_tables2 base2;
    fs_ext3_api ext3;
} fs_hook_tables3;

/* ---- The FIFTH table.  fs_ext3_api is frozen as well (1 member, 24 bytes; tests/test_outlines_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables3 by the same pattern:
 *     const fs_hook_tables4* t = (const fs_hook_tables4*)fs_test_hooks();   t->ext4.outline_simplify(...)
 * A library built before this table existed has nothing behind its fs_hook_tables3: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext4.magic == FS_EXT4_MAGIC and ext4.size >= the end of the member it needs. */
#define FS_EXT4_MAGIC 0x4653455854414234ull /* "FSEXTAB4" */

typedef struct fs_ext4_api {
    uint64_t magic; /* FS_EXT4_MAGIC */
    size_t size;    /* sizeof(fs_ext4_api) of the library that was built */

    /* ---- Outline simplification (csrc/simplify_ops.hip, csrc/simplify_defs.h).  OUR DEFINITION: Ramer-Douglas-Peucker
     * on every contour ring of region_outlines, with a tolerance in pixels.  Integers throughout; every result is a function of the
     * inputs alone, whatever order threads arrive in.  C = max_contours, V = max_vertices.
     * Inputs: the outputs of region_outlines for n frames,
     *   contours  int64 [n][C][6], of which the columns 1 (first vertex offset) and 2 (vertex count) are read,
     *   vertices  int32 [n][V][2]; every coordinate is read clamped to 0..16384,
     *   counts    int64 [n][4] = (contours, rows, vertices, flags): a frame's rows are the first counts[f][1], its total counts[f][2],
     *   tol_q     = 16 * tolerance^2 in pixel^2 (0.5 px = 4, 1 px = 16, 2 px = 64), 0..2^20,
     *   max_rounds  1..256.
     * VALID FRAMES.  A frame is simplified only if its flag bit 0 is clear, 0 <= rows <= C, total <= V, every row has count >= 3, every
     * row's offset is the exclusive prefix sum of the counts of the rows before it, and the counts sum to at most total -- what
     * region_outlines guarantees.  Any other frame gets nothing and a flag, so no garbage plane steers a store outside the buffers.
     * DISTANCE KEY.  For a segment a = v[l] -> b = v[r] and a vertex p: L = |b - a|^2, t = (b - a).(p - a);
     *   L = 0: q = |p - a|^2;   t <= 0: q = |p - a|^2 L;   t >= L: q = |p - b|^2 L;   else q = cross(b - a, p - a)^2,
     * so q / L is the squared distance from p to the SEGMENT, exactly (coordinates <= 2^14: q <= 2^58, 16 q <= 2^62).
     * PER CONTOUR, vertices v[0..m-1], v[0] the anchor's vertex, index m = v[0] again.
     *   Round 0: v[0] is kept; the whole ring (0, m) is one open segment with a = b = v[0], and it always splits at its vertex of
     *     largest q -- the vertex farthest from v[0] -- smallest index on a tie.
     *   Round k = 1..max_rounds: every open segment with interior vertices finds its interior vertex of largest q, smallest index on a
     *     tie.  If the test passes the vertex is kept and the segment splits into two open segments examined in round k + 1; if not,
     *     the segment is closed and its interior vertices are dropped.  The test is q > 0 in round 1, whatever the tolerance (a closed
     *     lattice contour does not lie on one segment, so every ring keeps at least 3 vertices), and 16 q > tol_q L from round 2 on.
     *   After the last round every segment still open keeps ALL its interior vertices and the contour is flagged unconverged: every
     *     dropped vertex is within the tolerance of the kept segment that spans it, cap or no cap.
     * Outputs, each written whole by every call:
     *   simple          = int64 [n][C][4] = (first offset, kept count, area2 of the kept ring, flags) per row, parallel to the rows of
     *                     contours; flag bit 0 = unconverged; rows behind the last are zero.
     *   simple_vertices = int32 [n][V][2], the kept vertices in input order, rings back to back in row order (offsets are the
     *                     exclusive prefix sums of the kept counts); zero behind the total.
     *   simple_counts   = int64 [n][4] = (rows, kept vertices, rounds, flags); rounds = the largest round in which a segment of the
     *                     frame split.  Flag bit 0: some contour is unconverged; bit 1: the input frame had overflowed its vertices
     *                     (input flag bit 0) and gets nothing; bit 2: the input had more contours than rows (counts[f][0] >
     *                     counts[f][1]), those without a row are not simplified; bit 3: the rows are inconsistent, the frame gets nothing.
     * workspace = FS_OUTLINE_SIMPLIFY_WORKSPACE_BYTES(n, max_contours, max_vertices) bytes at an 8-byte aligned address, the caller's:
     * per frame 48 bytes per possible vertex, 4 per possible contour, 4 per 1024 possible vertices and 2096.  Nothing is allocated,
     * synchronised or read on the host; the 10 + 2 max_rounds launches capture into a HIP graph.
     * Refused before a launch: a null pointer; n outside 1..65535; max_contours outside 1..2^20; max_vertices outside 4..2^22; tol_q
     * outside 0..2^20; max_rounds outside 1..256; a workspace not aligned to 8 bytes. */
#define FS_OUTLINE_SIMPLIFY_WORKSPACE_BYTES(n, max_contours, max_vertices)                                                             \
    ((size_t)(n) * 8 * (6 * (size_t)(max_vertices) + (((size_t)(max_vertices) + 1023) / 1024 + 1) / 2 + ((size_t)(max_contours) + 1) / 2 + 262))
    int (*outline_simplify)(const int64_t* contours, const int32_t* vertices, const int64_t* counts, int n, int max_contours, int max_vertices,
                            int tol_q, int max_rounds, int64_t* simple, int32_t* simple_vertices, int64_t* simple_counts, void* workspace,
                            fs_stream stream);
} fs_ext4_api;

typedef struct fs_hook_tables4 {
    fs_hook_tables3 base3;
    fs_ext4_api ext4;
} fs_hook_tables4;

/* ---- The SIXTH table.  fs_ext4_api is frozen as well (1 member, 24 bytes; tests/test_simplify_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables4 by the same pattern:
 *     const fs_hook_tables5* t = (const fs_hook_tables5*)fs_test_hooks();   t->ext5.frame_compose_regions(...)
 * A library built before this table existed has nothing behind its fs_hook_tables4: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext5.magic == FS_EXT5_MAGIC and ext5.size >= the end of the member it needs. */
#define FS_EXT5_MAGIC 0x4653455854414235ull /* "FSEXTAB5" */

typedef struct fs_ext5_api {
    uint64_t magic; /* FS_EXT5_MAGIC */
    size_t size;    /* sizeof(fs_ext5_api) of the library that was built */

    /* ---- Region overlay of frame egress (csrc/overlay_ops.hip, csrc/overlay_defs.h).  OUR DEFINITION: the reference
     * writes class colours only.  frame_compose's picture plus three optional layers drawn from region_table's index plane and
     * region_tracks' rows: a fill colour per id, an outline inside every region, the id as a label.  Integers throughout; every output
     * byte is a function of the inputs alone, whatever order threads arrive in.  R = max_regions; // is floor division.
     * Inputs: frame_compose's (mask .. out_full_range), which keep their meaning, refusals included, and on top:
     *   index          int32 [h][w] as region_table writes it; a value outside 0 .. R - 1 counts as -1.  1 <= R <= 65536.
     *   table          int64 [R][10], counts int64 [2]: region_table's, read only for labels; both may be NULL when label_scale == 0.
     *   tracks         int64 [R][4] as region_tracks writes one frame, or NULL.  The ID of row r is tracks[r][0], without tracks r itself.
     *   fill_palette   uint8 [fill_colours][3], 0 <= fill_colours = P <= 256; not read (NULL) when P == 0.
     *   outline        uint8 [K][4] = (R, G, B, A) per class, or NULL: no outline.
     *   outline_width  T, 0..4.      label_scale  s, 0..4.      label_min_area >= 1.
     *   halo_rgba, ink_rgb   packed R | G << 8 | B << 16 (| A << 24): the label's backdrop with its opacity, and the digits' colour.
     * Per output pixel p, per channel in int32, in this order:
     *   1. class colour   c = mask < K ? mask : 0;  (R, G, B, A) = palette[c];  r = the pixel's row, or -1.
     *   2. fill by id     if P >= 1, r >= 0 and id(r) >= 0: (R, G, B) = fill_palette[id(r) % P]; A stays the class's.
     *   3. base           o = frame_compose's: (A * colour + (255 - A) * b + 127) / 255 over the resized source b, or the colour alone.
     *   4. outline        drawn when T >= 1, r >= 0, outline is given, OA = outline[c].A > 0, and some pixel q INSIDE THE FRAME with
     *                     max(|qx - px|, |qy - py|) <= T has a row different from r:  o = (OA * outline[c] + (255 - OA) * o + 127) / 255.
     *                     Pixels outside the frame are not neighbours (the frame edge draws no line); pixels of row -1 are never drawn
     *                     but bound their neighbours.  The line is T pixels wide and lies inside the region.
     *   5. label          where the marks plane has the ink bit o = ink; where it has the halo bit alone, with HA = the halo's A,
     *                     o = (HA * halo + (255 - HA) * o + 127) / 255.
     * Then RGB24, NV12 or I420 exactly as frame_compose does it: chroma from the (sum + 2) >> 2 mean of the FINAL o of each 2 x 2 quad,
     * with the same edge rule.
     * LABELS.  Row r is LIVE when r < min(counts[1], R).  A live row gets a label when s >= 1, id(r) >= 0, area = table[r][1] >=
     * label_min_area, and the box fits: w >= tw + 2 s and h >= th + 2 s.  The text is the decimal digits of id mod 10^7, most significant
     * first, no leading zeros, nd of them;  tw = (6 nd - 1) s, th = 7 s;  cx = sum_x // area, cy = sum_y // area (columns 6, 7);
     *   x0 = min(max(cx - tw // 2, s), w - tw - s),  y0 = min(max(cy - th // 2, s), h - th - s);
     *   halo rectangle [x0 - s, x0 + tw + s) x [y0 - s, y0 + th + s)  (at most 172 x 36 pixels, always inside the frame);
     *   ink at (x, y) of the text box [x0, x0 + tw) x [y0, y0 + th):  u = (x - x0) // s, v = (y - y0) // s, digit k = u // 6, column
     *   col = u % 6:  ink exactly when col < 5 and bit 4 - col of FONT[digit k][v] is set.  FONT, rows top to bottom, bit 4 leftmost:
     *     0: 0E 11 13 15 19 11 0E    1: 04 0C 04 04 04 04 0E    2: 0E 11 01 02 04 08 1F    3: 1F 02 04 02 01 11 0E    4: 02 06 0A 12 1F 02 02
     *     5: 1F 10 1E 01 01 11 0E    6: 06 08 10 1E 11 11 0E    7: 1F 01 02 04 08 08 08    8: 0E 11 11 0E 11 11 0E    9: 0E 11 11 0F 01 02 0C
     * MARKS.  workspace = one uint8 per pixel, FS_FRAME_COMPOSE_REGIONS_WORKSPACE_BYTES(h, w) bytes at a 4-byte aligned address, the
     * caller's; NULL is allowed when s == 0, and the plane is then neither zeroed nor read.  With s >= 1 the call zeroes it on the
     * stream, then one workgroup per row ORs bit 0 (inside some label's halo rectangle) and bit 1 (ink of some label) into it with
     * 32-bit integer atomics; overlapping labels OR together, so ink beats halo whatever the order of arrival.  Nothing is allocated,
     * synchronised or read on the host: a HIP-graph replay on new planes gives that replay's picture.
     * Consequences: with P == 0, T == 0 (or outline == NULL) and s == 0 the output is frame_compose's, byte for byte (the call is handed
     * to frame_compose's kernel); with index all -1 and no live row likewise, whatever the options.
     * Refused before a launch: everything frame_compose refuses; a null index; R, P, T, s or label_min_area out of range; fill colours
     * without a fill palette; s >= 1 without table, counts or workspace; a workspace not aligned to 4 bytes. */
#define FS_FRAME_COMPOSE_REGIONS_WORKSPACE_BYTES(h, w) ((((size_t)(h) * (size_t)(w) + 3) / 4) * 4)
    int (*frame_compose_regions)(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u,
                                 const uint8_t* v, int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v,
                                 int out_format, int out_matrix, int out_full_range, const int32_t* index, const int64_t* table, const int64_t* counts,
                                 const int64_t* tracks, int max_regions, const uint8_t* fill_palette, int fill_colours, const uint8_t* outline,
                                 int outline_width, int label_scale, int64_t label_min_area, uint32_t halo_rgba, uint32_t ink_rgb, void* workspace,
                                 fs_stream stream);
} fs_ext5_api;

typedef struct fs_hook_tables5 {
    fs_hook_tables4 base4;
    fs_ext5_api ext5;
} fs_hook_tables5;

/* ---- The SEVENTH table.  fs_ext5_api is frozen as well (1 member, 24 bytes; tests/test_overlay_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables5 by the same pattern:
 *     const fs_hook_tables6* t = (const fs_hook_tables6*)fs_test_hooks();   t->ext6.mask_stabilize(...)
 * A library built before this table existed has nothing behind its fs_hook_tables5: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext6.magic == FS_EXT6_MAGIC and ext6.size >= the end of the member it needs. */
#define FS_EXT6_MAGIC 0x4653455854414236ull /* "FSEXTAB6" */

typedef struct fs_ext6_api {
    uint64_t magic; /* FS_EXT6_MAGIC */
    size_t size;    /* sizeof(fs_ext6_api) of the library that was built */

    /* ---- Temporal mask stabiliser (csrc/stabilize_ops.hip, csrc/stabilize_defs.h).  OUR DEFINITION: the reference
     * measures the flicker of its masks (the temporal-consistency mIoU) and has nothing that acts on it.  A causal, per-pixel class
     * debounce along the time axis, optionally read along the block matcher's vectors.  Integers throughout; every result is a function
     * of the inputs alone, whatever order threads arrive in.
     * Inputs:
     *   mask        uint8 [n][H][W], the observed classes o.
     *   confidence  uint8 [n][H][W] as mask_confidence writes it, or NULL.
     *   mv          int32 [n][hb * wb][7] with frame_h x frame_w = FH x FW, hb = FH // 16, wb = FW // 16: region_links_mc's tables, mv[f]
     *               the table of frame f against frame f-1; or NULL: the in-place op (frame_h, frame_w are then not looked at).
     *   pair_stats  int32 [n][4], rows as block_match_modes writes its stats, or NULL; it is honoured with and without mv.
     *   K classes 1..255;  persist P 1..255;  trust T 0..256 (256, or no confidence plane: nothing is trusted outright).
     *   state       uint32 [H][W], the caller's, kept across calls: read when has_state == 1, written by every call.
     * STATE WORD of a pixel: bit 31 = valid, bits 0-7 = the emitted class e, bits 8-15 = the candidate class c, bits 16-23 = the run
     * length r; the word 0 = no state.
     * PRIOR WORD s of frame f and pixel p, with o = mask[f][p]:
     *   0                                        if f == 0 and has_state == 0;
     *   0 for every pixel of the frame           if pair_stats is given and pair_stats[f][2] != 0 (a scene cut);
     *   with mv: the state after frame f-1 (the caller's for f == 0) at the SOURCE of p -- region_links_mc's rule, word for word: centre,
     *            block, row, void rows, the 64-bit differences, the shift scaled to mask pixels, (y + sy, x + sx) -- and 0 when the
     *            source lies outside the mask;
     *   otherwise the state after frame f-1 at p.
     * UPDATE, in this order:
     *   1. o >= K:        out = o, new state 0, nothing counted (not a class: passed through, and the pixel's history ends).
     *   2. s not valid:   e = c = o, r = 0, out = o.                                                      Counted as SEEDED.
     *   3. o == e:        c = e, r = 0, out = e.
     *   4. o != e:        if a confidence plane is given and confidence[f][p] >= T:
     *                         e = c = o, r = 0, out = o.                                                  Counted as SWITCHED and as TRUSTED.
     *                     else r' = (o == c) ? min(r + 1, 255) : 1, and c = o;
     *                         if r' >= P:  e = o, r = 0, out = o.                                         Counted as SWITCHED.
     *                         else         r = r', out = e.                                               Counted as HELD.
     * Outputs, each written whole by every call (so a HIP-graph replay on new planes gives that replay's result):
     *   out     uint8 [n][H][W];   state = the words after frame n-1;
     *   counts  int64 [n][4] = (held, switched, seeded, trusted) per frame: order-independent integer sums.
     * Consequences: P == 1 gives out == mask bit for bit, and so does T == 0 with a confidence plane; one call over n frames equals any
     * split into chained calls (has_state = 1 from the second on, mv / pair_stats / confidence sliced alike); with every row void, or
     * every vector 0, the compensated call equals the in-place one, all three outputs; a change that lasts is emitted P - 1 frames late.
     * LAUNCHES.  Without mv one launch for the whole call (one per 2048 frames), behind a 32 n-byte clearing launch for the counts: a
     * thread keeps the words of four consecutive pixels in registers through all n frames, so the state costs 8 bytes per pixel and
     * CALL.  With mv one launch packs a shift dword per block and frame (with a no-prior flag per frame, and clears the counts), then
     * one launch per frame gathers the prior words at their sources, ping-pong between the caller's plane and a second one in the
     * workspace such that the last frame writes the caller's; for odd n with has_state the caller's plane is copied to the second one
     * first (a frame must not gather from the plane it writes).  Events are summed per thread, wave and workgroup, then one 64-bit
     * atomic per counter, frame and workgroup, on at most 2 workgroups of 1024 threads per compute unit.  Nothing is allocated,
     * synchronised or read on the host.
     * workspace = FS_MASK_STABILIZE_WORKSPACE_BYTES(n, H, W, hb, wb) bytes at a 16-byte aligned address with mv: the second plane (4 B per
     * pixel, rounded up to 16) and hb * wb + 1 dwords per frame.  Without mv it is 0 bytes (pass hb = wb = 0) and NULL is allowed.
     * Refused before a launch: a null mask, out, state or counts; n < 1; H or W < 1; H * W >= 2^31 - 1; K, P or T out of range; has_state
     * other than 0 or 1; a state plane not aligned to 16 bytes, counts not aligned to 8; and with mv: a null workspace or one not aligned to
     * 16 bytes; n > 65535; frame_h or frame_w < 16; frame_h * frame_w >= 2^31; H > 31 frame_h or W > 31 frame_w. */
#define FS_MASK_STABILIZE_WORKSPACE_BYTES(n, H, W, hb, wb) \
    (((size_t)(hb) * (size_t)(wb) != 0) * ((((size_t)(H) * (size_t)(W) + 3) / 4) * 16 + (((size_t)(n) * ((size_t)(hb) * (size_t)(wb) + 1) + 3) / 4) * 16))
    int (*mask_stabilize)(const uint8_t* mask, const uint8_t* confidence, const int32_t* mv, const int32_t* pair_stats, int n, int H, int W, int frame_h,
                          int frame_w, int K, int persist, int trust, int has_state, uint32_t* state, uint8_t* out, int64_t* counts, void* workspace,
                          fs_stream stream);
} fs_ext6_api;

typedef struct fs_hook_tables6 {
    fs_hook_tables5 base5;
    fs_ext6_api ext6;
} fs_hook_tables6;

/* ---- The EIGHTH table.  fs_ext6_api is frozen as well (1 member, 24 bytes; tests/test_stabilize_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables6 by the same pattern:
 *     const fs_hook_tables7* t = (const fs_hook_tables7*)fs_test_hooks();   t->ext7.mask_distance(...)
 * A library built before this table existed has nothing behind its fs_hook_tables6: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext7.magic == FS_EXT7_MAGIC and ext7.size >= the end of the member it needs. */
#define FS_EXT7_MAGIC 0x4653455854414237ull /* "FSEXTAB7" */
#define FS_DIST_NONE 0xFFFFFFFFu            /* d2 of a pixel without a source in reach */

typedef struct fs_ext7_api {
    uint64_t magic; /* FS_EXT7_MAGIC */
    size_t size;    /* sizeof(fs_ext7_api) of the library that was built */

    /* ---- Exact distance to a class (csrc/distance_ops.hip, csrc/distance_defs.h).  OUR DEFINITION: the reference has
     * nothing like it.  Integers throughout; every result is a function of the inputs alone, whatever order threads arrive in.
     * Distances are in MASK PIXELS of a moving, un-georeferenced camera.
     * Inputs:
     *   mask        uint8 [n][H][W], at any byte address.
     *   source_set  uint32, non-zero: bit k set = class k is a source.  Mask ids >= 32 are never sources.
     *   max_dist    R, 0..32767; 0 = unbounded.
     * A pixel q of frame f is a SOURCE PIXEL if mask[f][q] < 32 and bit mask[f][q] of source_set is set.
     * Outputs, each written whole by every call (so a HIP-graph replay on new planes gives that replay's result):
     *   d2       uint32 [n][H][W]: for pixel p of frame f the minimum of (p.y - q.y)^2 + (p.x - q.x)^2 over the source pixels q of frame f; 0
     *            on a source pixel; FS_DIST_NONE where frame f has no source pixel, and with R > 0 also where that minimum exceeds R * R.  A
     *            value that is not FS_DIST_NONE is always the exact minimum: R replaces values by FS_DIST_NONE, it never changes one.
     *   nearest  int32 [n][H][W], or NULL: the raster index q.y * W + q.x of a source pixel that attains the minimum, among several the
     *            smallest raster index; -1 wherever d2 is FS_DIST_NONE.
     * Frames never see each other's sources.
     * LAUNCHES.  The separable form, three launches.  (1) Per column and chunk of 64 rows one dword: the first and the last source row
     * of the chunk.  (2) Per pixel the row of the nearest source pixel of its own COLUMN, the upper one on a tie (2 bytes, 0xFFFF: the
     * column has none): the chunk's 64 mask bytes as one 64-bit word, the nearest rows outside the chunk from the dwords of (1), at most
     * ceil(H / 64) - 1 of them.  (3) One workgroup per row stages the row's entries of (2) in LDS (2 W bytes, at most 64 KiB); a thread
     * scans outwards from its own x, d = 0, 1, 2, ..., taking the minimum of (d * d + g * g, raster index) over the columns x - d and
     * x + d, g the vertical distance to that column's entry, and stops at the first d with d * d > best (with nearest == NULL:
     * d * d >= best), when d passes R, or at the row's ends: every candidate at offset d costs at least d * d.  A row without any entry
     * means a frame without a source: nothing is scanned.  The scan is short where a source is near and O(W) per pixel for a frame with
     * one source pixel and R = 0 (measured: profiles/r23_distance.txt).
     * workspace = FS_MASK_DISTANCE_WORKSPACE_BYTES(n, H, W) bytes at a 4-byte aligned address, the caller's: the dwords of (1), then the
     * entries of (2).  Nothing is allocated, synchronised or read on the host.
     * Refused before a launch: a null mask, d2 or workspace; n < 1 or n > 65535; H or W < 1; H * W >= 2^31 - 1; H or W > 32768 (the bound
     * keeps d2 < 2^31); source_set == 0; R outside 0..32767; d2, nearest or the workspace not aligned to 4 bytes. */
#define FS_MASK_DISTANCE_WORKSPACE_BYTES(n, H, W) \
    ((((size_t)(n) * (((size_t)(H) + 63) / 64) * (size_t)(W) * 4 + (size_t)(n) * (size_t)(H) * (size_t)(W) * 2) + 15) / 16 * 16)
    int (*mask_distance)(const uint8_t* mask, int n, int H, int W, uint32_t source_set, int max_dist, uint32_t* d2, int32_t* nearest, void* workspace,
                         fs_stream stream);

    /* ---- The distance field tabulated per class and per region (csrc/distance_ops.hip).  OUR DEFINITION.
     * Inputs:
     *   mask        uint8 [n][H][W];   d2 uint32 [n][H][W] and nearest int32 [n][H][W] (or NULL) as mask_distance wrote them;
     *   index       int32 [n][H][W] and counts int64 [n][2], region_table's;   K classes 1..255;   max_regions 1..65536;
     *   target_set  uint32: bit k set = class k is tabulated in `exposure`;
     *   thresholds  int32 [B] in HOST memory, 1 <= B <= 8, strictly ascending distances in pixels, each 0..32767 (read during the call).
     * rows(f) = min(max(counts[f][1], 0), max_regions); a pixel p of frame f BELONGS to row r if index[f][p] == r and 0 <= r < rows(f).
     * Outputs, each cleared on the stream and written whole by every call:
     *   exposure  int64 [n][K][B]: exposure[f][k][b] = the number of pixels of frame f with mask == k and d2 <= thresholds[b]^2
     *             (cumulative in b; FS_DIST_NONE is above every threshold); all zero for a class outside target_set and for k >= 32.
     *   near      int64 [n][max_regions][8], row r of frame f = (min_d2, at_x, at_y, src_x, src_y, src_row, near_pixels, 0):
     *             min_d2 the smallest d2 other than FS_DIST_NONE over the row's pixels, (at_x, at_y) the pixel that attains it, the
     *             lowest raster index on a tie; (src_x, src_y) = nearest at that pixel, src_row = index at the source pixel, -1 if
     *             that pixel belongs to no row; near_pixels = the row's pixels with d2 <= thresholds[0]^2.  A row none of whose pixels
     *             has a d2 other than FS_DIST_NONE: (-1, -1, -1, -1, -1, -1, 0, 0).  nearest == NULL: src_x = src_y = src_row = -1.  Rows at
     *             and behind rows(f) are zero.  Regions of every class get a row: a source region's own is min_d2 = 0 at its anchor.
     * LAUNCHES.  Three: set up (the minimum's word starts at all ones, everything else at 0); one pass over the pixels (an LDS
     * histogram [32][8] per workgroup, flushed cumulatively with one 64-bit atomic per non-zero cell; per row a 64-bit atomic minimum of
     * d2 << 32 | raster index and an atomic sum, once per run of a row along the 1024 consecutive pixels a wave owns, and the minimum
     * only where it would lower the word); finish (the word becomes the row).  Integer sums and minima: the order does not matter.  No
     * workspace; nothing is allocated, synchronised or read on the host except `thresholds`.
     * Refused before a launch: a null mask, d2, index, counts, thresholds, exposure or near; n < 1 or n > 65535; H or W < 1; H * W >= 2^31 -
     * 1; H or W > 32768; K or max_regions out of range; B outside 1..8; a threshold outside 0..32767 or not above the one before it; d2,
     * nearest or index not aligned to 4 bytes; counts, exposure or near not aligned to 8. */
    int (*region_proximity)(const uint8_t* mask, const uint32_t* d2, const int32_t* nearest, const int32_t* index, const int64_t* counts, int n, int H,
                            int W, int K, int max_regions, uint32_t target_set, const int32_t* thresholds, int B, int64_t* exposure, int64_t* near,
                            fs_stream stream);
} fs_ext7_api;

typedef struct fs_hook_tables7 {
    fs_hook_tables6 base6;
    fs_ext7_api ext7;
} fs_hook_tables7;

/* ---- The NINTH table.  fs_ext7_api is frozen as well (2 members, 32 bytes; tests/test_distance_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables7 by the same pattern:
 *     const fs_hook_tables8* t = (const fs_hook_tables8*)fs_test_hooks();   t->ext8.global_motion(...)
 * A library built before this table existed has nothing behind its fs_hook_tables7: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext8.magic == FS_EXT8_MAGIC and ext8.size >= the end of the member it needs. */
#define FS_EXT8_MAGIC 0x4653455854414238ull /* "FSEXTAB8" */
#define FS_POSE_FRAC 20                     /* poses and pair models are Q20: ONE = 1 << 20 */

typedef struct fs_ext8_api {
    uint64_t magic; /* FS_EXT8_MAGIC */
    size_t size;    /* sizeof(fs_ext8_api) of the library that was built */

    /* ---- THE FLOOD-EXTENT MOSAIC (csrc/mosaic_ops.hip, csrc/mosaic_defs.h).  OUR DEFINITION: the reference has nothing
     * like it.  Four ops: a robust affine camera-motion fit per frame pair from the block matcher's table, a pose chain kept across
     * windows, a per-class vote canvas that masks are gathered into, and a resolve pass.  Integers wherever possible; every result is a
     * function of the inputs alone, whatever order threads arrive in.  Fixed point: ONE = 1 << FS_POSE_FRAC;
     * rshr(v) = (v + (1 << 19)) >> 20 on int64 with an arithmetic shift.  An affine is six int64 (m00, m01, m02, m10, m11, m12) in Q20,
     * x' = m00 x + m01 y + m02, acting on continuous pixel coordinates in which pixel i covers [i, i + 1).  The same rules as code:
     * csrc/mosaic_defs.h (host and device) and tests/mosaic_ref.py (numpy).
     *
     * global_motion fits one model per frame pair.  Inputs:
     *   tables      int32 [n][blocks][7], the matcher's rows (-1, 16, 16, src_x, src_y, dst_x, dst_y), blocks = (FH / 16) * (FW / 16);
     *   pair_stats  int32 [n][4] or NULL: word 2 non-zero = the pair is a scene cut;
     *   mask        uint8 [n][H][W] or NULL, with exclude_set (bit k set = class k is excluded; ids >= 32 never are);
     *   rounds 0..8, tol_q20 0..64 ONE, min_inliers 3..2^20.
     * A row is USABLE if src_x >= 0 (not void), its block centre lies in the frame (0 <= dst_x < FW, 0 <= dst_y < FH: the matcher writes no
     * other), |dx|, |dy| <= 32 with dx = src_x - dst_x, dy = src_y - dst_y, and, with a mask, the class at
     * mask[f][min(H - 1, dst_y H / FH)][min(W - 1, dst_x W / FW)] (floor divisions) is not excluded.  Block coordinates with hb = FH / 16,
     * wb = FW / 16: p = 2 (dst_x >> 4) + 1 - wb, q = 2 (dst_y >> 4) + 1 - hb: units of 8 pixels about the centre of the block grid.
     * The model is dx ~ a0 + a1 p + a2 q, dy ~ b0 + b1 p + b2 q, six Q20 int64.
     * START: the 65 x 65 histogram of the usable (dy, dx); its mode is the largest count, then the smallest |dx| + |dy|, then the smallest
     * dy, then the smallest dx (the matcher's own order); the start model is that translation with zero slopes.
     * ROUNDS: in round r = 0 .. rounds - 1 the tolerance is T = min(tol_q20 << (rounds - 1 - r), 64 ONE); the inliers are the usable rows
     * with |dx ONE - pred_x| <= T and |dy ONE - pred_y| <= T under the current model (integer comparisons); twelve int64 sums over them
     * (N, Sp, Sq, Spp, Spq, Sqq, Sdx, Spdx, Sqdx, Sdy, Spdy, Sqdy); the next model is gm_solve's (mosaic_defs.h): the 3 x 3 normal equations
     * by Cramer's rule in float64, the order of operations written out there, no fused multiply-add, each parameter rounded to Q20 to
     * nearest, ties to even.  A round with N < min_inliers, or one whose determinant gm_solve computes as 0 or whose solution holds a
     * parameter that is not a finite number below 2^20 pixels, stops the rounds: in round 0 the pair fails (too few / degenerate), later
     * the model of the round before stands.  rounds = 0 is the mode translation.  A pair with fewer than min_inliers usable rows fails as
     * too few whatever the rounds.
     * CONVERSION (gm_finish): in frame pixels x_prev = x + a0 + a1 (x - 8 wb) / 8 + a2 (y - 8 hb) / 8 (y alike); scaled to mask pixels
     * (m01 *= (W FH) / (FW H), m10 *= (H FW) / (FH W), m02 *= W / FW, m12 *= H / FH) in float64 and rounded once to Q20; the inverse affine
     * in float64 from the QUANTISED forward model, rounded once.  A pair is implausible and fails as degenerate if any of |m00 - ONE|,
     * |m11 - ONE|, |m01|, |m10| exceeds ONE / 4 (or a translation reaches 2^16 pixels, which keeps the chain's products in 63 bits).
     * A pair whose pair_stats row has the cut flag set fails as a cut without being fitted.
     * Output model int64 [n][16]: forward affine (6), inverse affine (6), status (0 ok, 1 cut, 2 too few, 3 degenerate or implausible),
     * usable rows, inliers of the last completed round (the mode's count until a round completes), rounds completed.  On failure the
     * twelve parameters are the identity.
     * ONE launch: a workgroup of 1024 threads per pair; rows in a strided loop; the histogram in LDS (65 x 65 dwords, LDS atomics); the
     * mode by a wave-then-workgroup maximum of a packed key; per round a classification and twelve sums reduced by shuffles, then across
     * the waves in LDS; one thread solves and broadcasts through LDS.  No global atomics, no workspace, nothing between workgroups; the
     * table is re-read (from L2) each round, 28 B x blocks.
     * Refused before a launch: a null tables or model; n outside 1..64; FH or FW outside 16..16384; H or W outside 1..16384; rounds, tol_q20
     * or min_inliers out of range; tables or pair_stats not aligned to 4 bytes, model not aligned to 8. */
    int (*global_motion)(const int32_t* tables, const int32_t* pair_stats, const uint8_t* mask, uint32_t exclude_set, int n, int FH, int FW, int H, int W,
                         int rounds, int64_t tol_q20, int min_inliers, int64_t* model, fs_stream stream);

    /* ---- pose_chain composes the pair models into poses relative to the ANCHOR, the first frame of the mosaic.
     * compose(A, B) = A o B: c00 = rshr(a00 b00 + a01 b10), c01 = rshr(a00 b01 + a01 b11), c02 = rshr(a00 b02 + a01 b12) + a02, row 1 alike:
     * exact int64.  state int64 [32] on the device, read and written, lasts across calls; all zero = fresh.  It holds to_anchor (6),
     * from_anchor (6), last_fwd (6), last_inv (6), a phase (0 fresh, 1 tracking, 2 lost), the frames seen, the frames lost, the length of
     * the current bridge run, and four spare words.
     * Frames are walked in order.  From a fresh state the first frame is the anchor: its pose is the identity, its own model row is
     * ignored (its table relates it to a frame outside the mosaic), and the last good pair starts as the identity.  Otherwise a model
     * with status 0 gives to_anchor = compose(to_anchor, fwd), from_anchor = compose(inv, from_anchor) and becomes the last good pair.  A
     * model with status 2 or 3 (or any status that is none of 0..3, or a status-0 row whose entries exceed the pair bounds of
     * mosaic_defs.h) is BRIDGED: the last good pair's model is used in its place, for at most max_bridge pairs running.  A cut, or a bridge
     * run that is exhausted, makes the chain LOST; lost is sticky until the caller hands in a fresh state.  A frame whose composed
     * |to_anchor translation| >= 2^14 ONE is lost as well (so is one whose linear entries reach 16 in either direction, or whose
     * from_anchor translation reaches 2^20 ONE): these bounds keep every later product inside 63 bits; the derivation is in mosaic_defs.h.
     * Output poses int64 [n][16]: to_anchor (6), from_anchor (6), status (0 ok, 1 bridged, 2 lost), clipped (1 if any of the frame's four
     * corners (0, 0), (W, 0), (0, H), (W, H) under to_anchor plus the origin (ox, oy) falls outside [0, CW] x [0, CH]), inliers, usable rows
     * (both copied from the model row; 0 for the anchor).  A lost frame's row holds identities, clipped 0.
     * ONE launch of one wave; lane 0 walks the n <= 64 frames.
     * Refused before a launch: a null pointer; n outside 1..64; H, W, CH or CW outside 1..16384; |ox| or |oy| > 16384; max_bridge outside
     * 0..64; a pointer not aligned to 8 bytes. */
    int (*pose_chain)(const int64_t* model, int64_t* state, int64_t* poses, int n, int H, int W, int CH, int CW, int ox, int oy, int max_bridge,
                      fs_stream stream);

    /* ---- mosaic_accumulate gathers n masks into the vote canvas.  votes uint16 [K][CH][CW], K <= 32, updated in place; (ox, oy) = the
     * canvas pixel of the anchor frame's top-left corner.  For canvas pixel (X, Y) and each frame f that is not lost (status 0 or 1, and a
     * from_anchor inside the pose bounds), in order: AX = (2 (X - ox) + 1) << 19, AY alike; sx = rshr(f00 AX + f01 AY) + f02, sy alike, with
     * from_anchor; x = sx >> 20, y = sy >> 20 (floor); if 0 <= x < W, 0 <= y < H and k = mask[f][y][x] < K then
     * votes[k][Y][X] = min(votes[k][Y][X] + 1, 65535).  A lost frame votes nowhere.  A gather with nearest sampling: every canvas pixel has
     * one owner, so there are no atomics, no holes under zoom and no dependence on order.
     * ONE launch: a workgroup per 64 x 16 canvas tile maps the tile's four corners through every live frame's from_anchor and drops the
     * frames whose bounding box cannot touch the frame (one pixel of slack covers the rounding); a tile that no frame touches reads and
     * writes nothing more, so a window costs its footprint, not the canvas.
     * Refused before a launch: a null pointer; n outside 1..64; H, W, CH or CW outside 1..16384; K outside 1..32; |ox| or |oy| > 16384;
     * poses not aligned to 8 bytes, votes not aligned to 2. */
    int (*mosaic_accumulate)(const uint8_t* mask, const int64_t* poses, int n, int H, int W, int K, int CH, int CW, int ox, int oy, uint16_t* votes,
                             fs_stream stream);

    /* ---- mosaic_resolve reads the canvas.  Outputs, each written whole: cls uint8 [CH][CW] = the class with the most votes, the lowest id
     * on a tie, 255 where there are none; conf uint8 = (255 max + total / 2) / total, 0 where unseen; seen uint32 = the total;
     * totals int64 [K][2] = per class the canvas pixels won and the votes received.
     * TWO launches: totals cleared; one pass, an LDS histogram per workgroup flushed with one 64-bit atomic per non-zero cell.
     * Refused before a launch: a null pointer; K outside 1..32; CH or CW outside 1..16384; votes not aligned to 2 bytes, seen to 4,
     * totals to 8. */
    int (*mosaic_resolve)(const uint16_t* votes, int K, int CH, int CW, uint8_t* cls, uint8_t* conf, uint32_t* seen, int64_t* totals, fs_stream stream);
} fs_ext8_api;

typedef struct fs_hook_tables8 {
    fs_hook_tables7 base7;
    fs_ext8_api ext8;
} fs_hook_tables8;

/* ---- The TENTH table.  fs_ext8_api is frozen as well (4 members, 48 bytes; tests/test_mosaic_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables8 by the same pattern:
 *     const fs_hook_tables9* t = (const fs_hook_tables9*)fs_test_hooks();   t->ext9.ortho_accumulate(...)
 * A library built before this table existed has nothing behind its fs_hook_tables8: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext9.magic == FS_EXT9_MAGIC and ext9.size >= the end of the member it needs. */
#define FS_EXT9_MAGIC 0x4653455854414239ull /* "FSEXTAB9" */
#define FS_ORTHO_EMPTY 0xFFFFFFFFFFFFFFFFull /* a rank word no frame has won */

typedef struct fs_ext9_api {
    uint64_t magic; /* FS_EXT9_MAGIC */
    size_t size;    /* sizeof(fs_ext9_api) of the library that was built */

    /* ---- THE ORTHOPHOTO UNDER THE MOSAIC (csrc/ortho_ops.hip, csrc/ortho_defs.h).  OUR DEFINITION: the reference has
     * nothing like it.  The gather that registers the frames' PIXELS the way mosaic_accumulate registers their classes, and a compose
     * pass that lays the extent map over it.  The same rules as code: csrc/ortho_defs.h (host and device) and tests/ortho_ref.py (numpy).
     *
     * ortho_accumulate takes ONE frame per call.  Canvas state, both [CH][CW], updated in place: rank uint64 (FS_ORTHO_EMPTY = all ones:
     * empty) and rgba uint32 (0: unseen).  The image sampled is I = the decoded frame (frame, u, v, format, matrix, full_range, FH, FW:
     * exactly frame_prepare's arguments) through frame_prepare's own resize to the mask size H x W, as stored uint8: the image
     * frame_compose draws under that frame's mask, bit for bit.  pose is ONE row of pose_chain's output, ordinal the frame's number since
     * the anchor (the caller counts).  For canvas pixel (X, Y): if the pose is not lost and its from_anchor lies inside the pose bounds
     * (pose_votes), (x, y) is the frame pixel mosaic_accumulate would take its vote from (anchor_coord, source_pixel with from_anchor; the
     * origin (ox, oy) as there).  If 0 <= x < W and 0 <= y < H the frame's rank there is
     *   mode 0 (centre):  key << 32 | ordinal with key = (2x + 1 - W)^2 + (2y + 1 - H)^2 < 2^29: the view in which the ground point is
     *                     nearest the optical axis wins, ties go to the earlier frame (the orthomosaic seam rule);
     *   mode 1 (latest):  (0xFFFFFFFF - ordinal) << 32 | ordinal: the newest frame wins.
     * Only if that rank is STRICTLY smaller than the stored one are rank and rgba = R | G << 8 | B << 16 | 0xFF << 24 of I[y][x] stored.
     * The result is therefore the minimum over the frames: it does not depend on the order of the calls or on how frames are split into
     * windows; a repeated call changes nothing (safe under graph replay); every canvas pixel has one owner, so there are no atomics.
     * ONE launch: a workgroup per 64 x 16 canvas tile; a tile whose four corners under from_anchor cannot touch the frame (touches, one
     * pixel of slack) returns having read the pose row only, so a frame costs its footprint, not the canvas.  A thread reads its rank
     * word; only a winner fetches the taps (four, two where only the rows are resampled, one at equal sizes; YUV -> RGB where needed).
     * Refused before a launch: a null frame, pose, rank or rgba, or a null chroma pointer of a YUV format; format, matrix or range code
     * out of range; FH, FW, H, W, CH or CW outside 1..16384; |ox| or |oy| > 16384; mode not 0 or 1; ordinal 0xFFFFFFFF; pose or rank not
     * aligned to 8 bytes, rgba to 4. */
    int (*ortho_accumulate)(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW,
                            const int64_t* pose, uint32_t ordinal, int H, int W, int mode, int CH, int CW, int ox, int oy, uint64_t* rank, uint32_t* rgba,
                            fs_stream stream);

    /* ---- ortho_compose draws the canvas: out uint8 RGB24 [CH][CW][3], written whole.  under = the pixel's (R, G, B) where rgba >> 24 != 0,
     * else fill (r | g << 8 | b << 16).  k = cls[Y][X] (mosaic_resolve's plane).  With cls NULL no class is drawn, whatever K is:
     * out = under, the plain orthophoto (palette may then be NULL too).  Otherwise for k < K the output is (A_k colour_k + (255 - A_k) under + 127) / 255 per channel from palette uint8 [K][4] (R, G, B, A) -- frame_compose's
     * blend -- and `under` otherwise: unlike frame_compose, ids >= K take no colour, because 255 means "never seen" here.  EDGE LINE: a
     * pixel whose class k is in edge_set (bit k, k < min(K, 32)) and that has a 4-neighbour INSIDE the canvas whose class is neither k nor
     * 255 takes colour_k opaque: a one-pixel line along the inside of that class's boundary.  Unseen ground makes no edge.
     * ONE launch: 64 x 16 tiles, a thread per four pixels of a row; the palette in LDS; with an edge set the class tile and a one-pixel
     * apron in LDS.  Four pixels leave as three dwords where CW % 4 == 0, rgba is aligned to 16 bytes and cls and out to 4; as bytes
     * otherwise.
     * Refused before a launch: a null rgba or out, or cls without a palette; CH or CW outside 1..16384; K outside 1..256; an edge_set bit at
     * or above min(K, 32); fill >= 2^24; rgba not aligned to 4 bytes. */
    int (*ortho_compose)(const uint32_t* rgba, const uint8_t* cls, const uint8_t* palette, int K, uint32_t edge_set, uint32_t fill, int CH, int CW,
                         uint8_t* out, fs_stream stream);
} fs_ext9_api;

typedef struct fs_hook_tables9 {
    fs_hook_tables8 base8;
    fs_ext9_api ext9;
} fs_hook_tables9;

/* ---- The ELEVENTH table.  fs_ext9_api is frozen as well (2 members, 32 bytes; tests/test_ortho_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables9 by the same pattern:
 *     const fs_hook_tables10* t = (const fs_hook_tables10*)fs_test_hooks();   t->ext10.map_view(...)
 * A library built before this table existed has nothing behind its fs_hook_tables9: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext10.magic == FS_EXT10_MAGIC and ext10.size >= the end of the member it needs. */
#define FS_EXT10_MAGIC 0x4653455854413130ull /* "FSEXTA10" */

typedef struct fs_ext10_api {
    uint64_t magic; /* FS_EXT10_MAGIC */
    size_t size;    /* sizeof(fs_ext10_api) of the library that was built */

    /* ---- FRAME-TO-MAP REGISTRATION (csrc/refine_ops.hip, csrc/refine_defs.h).  OUR DEFINITION: the reference has nothing
     * like it.  The pose chain is built from frame-to-frame fits alone and drifts; these three ops are the link between the orthophoto
     * canvas, the block matcher and global_motion that lets a frame be registered against the ground mapped so far BEFORE it votes:
     *   map_view -> block_match_modes(cur, view) -> map_gate -> global_motion (n = 1, frame_size = mask_size = (H, W)) -> pose_correct.
     * The same rules as code: csrc/refine_defs.h (host and device) and tests/refine_ref.py (numpy).  All integer, bit for bit.
     *
     * map_view draws the map as this frame should see it under its predicted pose.  The frame arguments (frame, u, v, format, matrix,
     * full_range, FH, FW), pose (ONE row of pose_chain's output), ordinal, H, W, CH, CW, ox, oy, rank and rgba are ortho_accumulate's;
     * the canvas is only read.  Three uint8 planes [H][W], each written whole:
     *   cur[y][x]   = luma(I[y][x]), I = ortho_accumulate's image (the frame through frame_prepare's resize to H x W, as stored uint8),
     *                 luma = (77 R + 150 G + 29 B + 128) >> 8, the block matcher's;
     *   valid[y][x] = 1 iff the pose is usable and the canvas pixel (X, Y) under the centre of frame pixel (x, y) lies in the canvas, has
     *                 rgba >> 24 != 0 and, ONLY when min_age > 0, ordinal - (uint32_t)rank >= min_age taken in 64 bits (an owner with an
     *                 ordinal above the frame's own is NOT valid); with min_age == 0 rank is not read.  0 otherwise;
     *   view[y][x]  = luma of that canvas pixel's (R, G, B) where valid, 0 where not.
     * The pose is usable when its status is 0 or 1 and to_anchor's linear entries are below 16 and its translation below 2^14 pixels in
     * magnitude (pose_in_bounds' bounds for to_anchor), tested before any product.  Then, with t = to_anchor:
     *   ax = (2x + 1) << 19, ay alike;  cx = ((t00 ax + t01 ay + 2^19) >> 20) + t02;  X = (cx >> 20) + ox;  Y alike.
     * |t| < 2^24 and |ax| < 2^35: the two products stay below 2^60.
     * ONE launch: a thread per four pixels of a row; dword stores where W % 4 == 0 and the three planes are aligned to 4 bytes, bytes
     * otherwise.
     * Refused before a launch: a null frame, pose, rank, rgba, cur, view or valid, or a null chroma pointer of a YUV format; format,
     * matrix or range code out of range; FH, FW, CH or CW outside 1..16384; H or W outside 16..16384; |ox| or |oy| > 16384; ordinal
     * 0xFFFFFFFF; min_age negative; pose or rank not aligned to 8 bytes, rgba to 4. */
    int (*map_view)(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const int64_t* pose,
                    uint32_t ordinal, int H, int W, int CH, int CW, int ox, int oy, const uint64_t* rank, const uint32_t* rgba, int min_age, uint8_t* cur,
                    uint8_t* view, uint8_t* valid, fs_stream stream);

    /* ---- map_gate: no vector from ground the map does not hold.  table is block_match_modes' for (cur, view), blocks = (H / 16) (W / 16)
     * rows of 7 ints, gated IN PLACE: a row stays as it is iff the WINNER's window [src_x - 8, src_x + 8) x [src_y - 8, src_y + 8) lies
     * inside the plane (tested in 64 bits before any read: a row is device memory and may hold anything) and all 256 bytes of `valid`
     * under it are 1; every other row becomes the void row (-1, 16, 16, -16, -16, -16, -16).  A void row has no window inside any plane
     * and stays void.  A candidate that lay over invalid pixels saw zeros there: if it won, its row is voided; if it lost, the winner
     * beat it honestly.  ONE launch: a wave per row, four bytes a lane, one ballot.
     * Refused before a launch: a null table or valid; H or W outside 16..16384; blocks != (H / 16) (W / 16); table not aligned to 4. */
    int (*map_gate)(int32_t* table, int blocks, const uint8_t* valid, int H, int W, fs_stream stream);

    /* ---- pose_correct folds global_motion's fit of (cur, view) into the chain.  model: ONE row of global_motion; state: pose_chain's 32
     * words; pose: the frame's row, the one map_view drew with; out: 8 words = (status, usable rows, inliers, rounds done, fwd[2],
     * fwd[5], 0, 0), the middle five copied from the model row.  The forward model maps a frame pixel to the view pixel that shows the
     * same ground, and the view was drawn with to_anchor, so:
     *   status 4: the pose row is lost, the state's phase is not TRACKING, or the state's to_anchor is not the row's.  Nothing changes.
     *   status 2: model[12] != 0, or the model is outside pose_chain's pair bounds.  Nothing changes.
     *   else to_next = compose(to_anchor, fwd), from_next = compose(inv, from_anchor) -- pose_chain's own two lines;
     *   status 3: the state's poses or the new ones are outside pose_chain's pose bounds.  Nothing changes.
     *   status 0: words 0..11 of the state and of the pose row become the new poses, pose[13] (clipped) is recomputed.
     * last_fwd, last_inv, the phase, the counters and the bridge run of the state are never written.  ONE launch of one wave.
     * Refused before a launch: a null pointer; H, W, CH or CW outside 1..16384; |ox| or |oy| > 16384; a pointer not aligned to 8 bytes. */
    int (*pose_correct)(const int64_t* model, int64_t* state, int64_t* pose, int H, int W, int CH, int CW, int ox, int oy, int64_t* out, fs_stream stream);
} fs_ext10_api;

typedef struct fs_hook_tables10 {
    fs_hook_tables9 base9;
    fs_ext10_api ext10;
} fs_hook_tables10;

/* ---- The TWELFTH table.  fs_ext10_api is frozen as well (3 members, 40 bytes; tests/test_guide_cpu.py), so ops added since live in a
 * table of their own, append-only, that the library places directly behind fs_hook_tables10 by the same pattern:
 *     const fs_hook_tables11* t = (const fs_hook_tables11*)fs_test_hooks();   t->ext11.guide_vectors(...)
 * A library built before this table existed has nothing behind its fs_hook_tables10: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext11.magic == FS_EXT11_MAGIC and ext11.size >= the end of the member it needs. */
#define FS_EXT11_MAGIC 0x4653455854413131ull /* "FSEXTA11" */

typedef struct fs_ext11_api {
    uint64_t magic; /* FS_EXT11_MAGIC */
    size_t size;    /* sizeof(fs_ext11_api) of the library that was built */

    /* ---- THE MATCHER'S VECTORS GUIDED BY THE CAMERA MODEL (csrc/motion_ops.hip, csrc/guide_defs.h).  OUR DEFINITION: the
     * global-motion predictor candidate of an encoder, applied to the finished table.  Integers throughout, bit for bit; the same rules
     * as code: csrc/guide_defs.h (host and device) and tests/guide_ref.py (numpy).  ONE, rshr and pair_in_bounds are global_motion's
     * (fs_ext8_api above, csrc/mosaic_defs.h).
     * Inputs:
     *   mv           int32 [n][hb * wb][7], hb = FH / 16, wb = FW / 16: the tables of n frame pairs as block_match / block_match_modes write them;
     *   model        int64 [n][16]: global_motion's rows, fitted with mask_size == frame_size so that the forward affine is in frame pixels;
     *   fill_void    0 | 1;   outlier_q20  -1 = off, else 0 .. 64 ONE;
     *   evidence, all three or none: cur, ref uint8 [n][FH][FW][channels] (channels 1 = luma, 3 = RGB reduced with block_match's luma),
     *   cost int32 [n][hb * wb] (the matcher's winning costs); penalty 0..255 (the matcher's); guide_bias 0..65535.
     * Outputs: out int32 of mv's shape (it may BE mv); counts int64 [n][8], written whole by every call.
     * Per pair f and block i = by wb + bx, with the centre taken from the INDEX, (cx, cy) = (16 bx + 8, 16 by + 8) (a void row has lost
     * its dst), M = model[f], CX = cx ONE, CY = cy ONE:
     *   PREDICTION   gx = rshr(M0 CX + M1 CY) + M2 - CX, gy = rshr(M3 CX + M4 CY) + M5 - CY (Q20); pdx = rshr(gx), pdy = rshr(gy).
     *                The pair has NO GUIDE if M[12] != 0 or the row fails pair_in_bounds(M, M + 6); both are tested before any product
     *                (a row may hold anything).  Inside the bounds |M0|, |M1| <= 2^21 and CX < 2^34: a product is below 2^55, the sum of
     *                two below 2^56, |gx| < 2^38.
     *   AVAILABLE    the block's guide is available iff |pdx|, |pdy| <= 32 and the 16 x 16 window at (cx - 8 + pdx, cy - 8 + pdy) lies
     *                inside the frame: the matcher's own candidate rule.
     *   CLASS        VOID: r[3] < 0 or r[5] < 0 or r[6] < 0.  FOREIGN: not void, and (r[5], r[6]) != (cx, cy) or |r[3] - r[5]| > 32 or
     *                |r[4] - r[6]| > 32 (differences in 64 bits).  VECTOR (dx, dy) = (r[3] - r[5], r[4] - r[6]): otherwise.
     *   OUTLIER      a VECTOR row of a pair with a guide, outlier_q20 >= 0 and |dx ONE - gx| > outlier_q20 or |dy ONE - gy| > outlier_q20
     *                (integer comparisons; equality is not an outlier).
     *   DECISION     a pair without a guide: every row copied.  FOREIGN: copied.  VOID with fill_void and an available guide: FILLED,
     *                (-1, 16, 16, cx + pdx, cy + pdy, cx, cy); otherwise as it was.  OUTLIER without an available guide: DROPPED, the void
     *                row (-1, 16, 16, -16, -16, -16, -16) -- the camera says its source lay outside the previous frame, so whatever it
     *                matched is something else.  OUTLIER with an available guide: without evidence REPLACED by the guide row; with
     *                evidence cost_g = SAD of the block of cur[f] at (cx - 8, cy - 8) against the window of ref[f] at
     *                (cx - 8 + pdx, cy - 8 + pdy), in the matcher's luma, + penalty (|pdx| + |pdy|), REPLACED iff
     *                cost_g <= cost[f][i] + guide_bias (in 64 bits), else KEPT BY EVIDENCE (copied).  Every other VECTOR row: copied.
     *   counts[f]    (blocks, void rows in, filled, outliers, replaced, dropped, kept by evidence, foreign); void and foreign rows are
     *                counted whether or not the pair has a guide, the other five are 0 without one.
     * So fill_void = 0 with outlier_q20 = -1 is a copy, and so is a model with status != 0; without evidence a second pass over the
     * result with the same model changes no row and fills nothing; a table of the rounded model vectors has no outlier at
     * outlier_q20 >= ONE / 2.
     * TWO launches: counts cleared by a kernel (not a memset node: DESIGN §3.16); then one wave per block, four blocks per workgroup of
     * 256, blockIdx.y the pair.  Every lane computes the same prediction, class and decision: the branches are wave-uniform.  Only a wave
     * whose row is an outlier with an available guide, in evidence mode, reads the frames: 4 pixels a lane, v_sad_u8, one wave sum.
     * Lanes 0..6 write the row.  counts: an LDS tally per workgroup, one 64-bit atomic per non-zero cell (integer sums: any order gives
     * the same result).  No thread waits for another workgroup; nothing is allocated, synchronised or read on the host.
     * Refused before a launch, the offending value named: a null mv, model, out or counts; n outside 1..64; FH or FW outside 16..16384;
     * outlier_q20 outside -1 .. 64 ONE; penalty outside 0..255; guide_bias outside 0..65535; some but not all of cur, ref, cost;
     * channels other than 1 or 3; mv, out or cost not aligned to 4 bytes, model or counts not aligned to 8. */
    int (*guide_vectors)(const int32_t* mv, const int64_t* model, int n, int FH, int FW, int fill_void, int64_t outlier_q20, const uint8_t* cur,
                         const uint8_t* ref, int channels, const int32_t* cost, int penalty, int guide_bias, int32_t* out, int64_t* counts,
                         fs_stream stream);
} fs_ext11_api;

typedef struct fs_hook_tables11 {
    fs_hook_tables10 base10;
    fs_ext11_api ext11;
} fs_hook_tables11;

/* ---- The THIRTEENTH table.  fs_ext11_api is frozen as well (1 member, 24 bytes; tests/test_relocate_cpu.py), so ops added since live in
 * a table of their own, append-only, that the library places directly behind fs_hook_tables11 by the same pattern:
 *     const fs_hook_tables12* t = (const fs_hook_tables12*)fs_test_hooks();   t->ext12.map_locate(...)
 * A library built before this table existed has nothing behind its fs_hook_tables11: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext12.magic == FS_EXT12_MAGIC and ext12.size >= the end of the member it needs. */
#define FS_EXT12_MAGIC 0x4653455854413132ull /* "FSEXTA12" */

typedef struct fs_ext12_api {
    uint64_t magic; /* FS_EXT12_MAGIC */
    size_t size;    /* sizeof(fs_ext12_api) of the library that was built */

    /* ---- RELOCALISATION AGAINST THE ORTHOPHOTO (csrc/relocate_ops.hip, csrc/relocate_defs.h).  OUR DEFINITION: the
     * reference has nothing like it.  pose_chain makes a lost chain stay lost; these five ops find where on the map a lost frame lies
     * by an exhaustive coarse search and let the chain resume ON THE SAME MOSAIC.  For one lost frame (pose_chain has just written a
     * lost row and the state's phase is 2; words 0..11 of the state still hold the last pose):
     *   map_coarse -> map_patch -> map_locate -> pose_relocate -> [map_view -> block_match_modes -> map_gate -> global_motion ->
     *   pose_correct, all on the CANDIDATE state and row] -> relocate_commit.
     * The same rules as code: csrc/relocate_defs.h (host and device) and tests/relocate_ref.py (numpy).  All integer, bit for bit.
     * S is the coarse cell edge, 4, 8 or 16; ch = CH / S, cw = CW / S (floor: a remainder strip owns no cell); luma_of is map_view's.
     *
     * map_coarse: cl, cv uint8 [ch][cw].  cv = 1 iff all S^2 words of the cell have rgba >> 24 != 0; then cl = (sum of luma_of + S^2 / 2)
     * / S^2 (the sum is at most 255 * 256); otherwise cl = cv = 0.  ONE launch, a thread per cell.
     * Refused before a launch: a null pointer; CH or CW outside 1..16384; S not 4, 8 or 16; ch or cw == 0; rgba not aligned to 4. */
    int (*map_coarse)(const uint32_t* rgba, int CH, int CW, int S, uint8_t* cl, uint8_t* cv, fs_stream stream);

    /* ---- map_patch draws the lost frame into canvas cells with the last pose the state holds.  The frame arguments, H, W, CH, CW, ox, oy
     * as map_view's; state: pose_chain's 32 words, only read.  tl, tv: 65536 bytes each, of which the first tw th are written, as
     * [th][tw]; geom int64 [8] = (status, pu0, pv0, tw, th, nt, 0, 0), written by EVERY call (a failing one: the status, then zeros).
     * In this order, everything read from the state tested before any product:
     *   status 1: state[24] != 2 (the chain is not lost).        status 2: the state's poses fail pose_chain's pose bounds.
     *   The four corners (x, y) in {0, W} x {0, H} under t = to_anchor, frame_clipped's rule: cx = t00 x + t01 y + t02 + ox ONE (|t| <
     *   2^24, x <= 2^14: below 2^40), cy alike.  The patch covers canvas pixels [min cx >> 20, (max cx + ONE - 1) >> 20), widened
     *   outwards to whole cells: pu0 = that lower pixel >> log2 S (arithmetic), pu1 = (the upper + S - 1) >> log2 S, tw = pu1 - pu0 (0 for a range without a pixel); v alike.
     *   status 3: tw < 1, th < 1 or tw th > 65536.               status 4: tw > cw or th > ch.
     *   status 0: patch cell (i, j) is canvas cell (pu0 + i, pv0 + j) -- it may lie outside the canvas.  It is valid (tv = 1) iff every
     *   one of its S^2 canvas pixels (X, Y) has source_pixel(from_anchor, anchor_coord(X, ox), anchor_coord(Y, oy)) inside [0, W) x
     *   [0, H); tl is then the rounded mean, as map_coarse's, of luma(I[y][x]), I and luma as map_view's cur; otherwise tl = tv = 0.
     *   Once tw S <= CW <= 2^14, |X - ox| < 2^15 + 32, so source_pixel's products stay below 2^61.  nt = the number of valid cells.
     * TWO launches: a wave per cell (the grid covers min(65536, ch cw) cells; a wave past tw th returns), then one workgroup that
     * counts nt and writes geom.
     * Refused before a launch: a null frame, state, tl, tv or geom, or a null chroma pointer of a YUV format; format, matrix or range
     * code out of range; FH, FW, H, W, CH or CW outside 1..16384; |ox| or |oy| > 16384; S not 4, 8 or 16; ch or cw == 0; state or geom
     * not aligned to 8 bytes. */
    int (*map_patch)(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const int64_t* state, int H,
                     int W, int CH, int CW, int ox, int oy, int S, uint8_t* tl, uint8_t* tv, int64_t* geom, fs_stream stream);

    /* ---- map_locate slides the patch over the whole coarse canvas.  cl, cv: map_coarse's, ch x cw CELLS; tl, tv, geom: map_patch's;
     * scores: the caller's workspace, uint32 [ch][cw][2]; found int64 [16] = (status, u*, v*, sad*, n*, runner-up exists, u2, v2, sad2,
     * n2, placements, eligible placements, nt, 0, 0, 0), written by every call.
     *   status 2 (bad geom, everything else 0): geom[0] != 0, tw or th outside 1..cw / 1..ch, tw th > 65536, nt outside 0..tw th, or
     *   |pu0| or |pv0| >= 2^20 -- tested before any product or index.
     *   Placements: every shift (u, v) in cells with 0 <= pu0 + u <= cw - tw and 0 <= pv0 + v <= ch - th.  Over the cells where
     *   cv[pv0 + v + j][pu0 + u + i] == 1 and tv[j][i] == 1: n = their number, sad = the sum of |cl - tl|.
     *   Eligible: n >= 1 and 1000 n >= min_overlap_permille nt.
     *   Order: the smaller mean, compared as sad_a n_b < sad_b n_a in 64 bits (sad < 2^24, n <= 2^16: below 2^40); then the larger n,
     *   the smaller v, the smaller u.  Best: the first eligible placement in that order; status 1 (no eligible placement) if none.
     *   Runner-up: the first eligible placement with max(|u - u*|, |v - v*|) > exclude.
     * A shift by (u, v) cells is the state's pose translated by (S u, S v) canvas pixels.
     * TWO launches: the score plane (a workgroup per 64 x 4 placements; patch and canvas strip through LDS as bytes, four cells per
     * v_sad_u8 on dwords ANDed with the joint validity, n from the same mask; no atomics), then one workgroup that folds the plane.
     * Refused before a launch: a null pointer; ch or cw outside 1..4096; min_overlap_permille outside 1..1000; exclude outside 0..64;
     * geom, found or scores not aligned to 8 bytes. */
    int (*map_locate)(const uint8_t* cl, const uint8_t* cv, int ch, int cw, const uint8_t* tl, const uint8_t* tv, const int64_t* geom, int min_overlap_permille,
                      int exclude, uint32_t* scores, int64_t* found, fs_stream stream);

    /* ---- pose_relocate turns the placement into a CANDIDATE state (32 words) and pose row (16 words); `state` is only read.  The
     * decision, in this order, lands in cand_state[28] (a spare word of the candidate only):
     *   1 state[24] != 2: the chain is not lost, there is nothing to do (a caller need not know beforehand whether it is);
     *   2 found[0] == 1 (no eligible placement);
     *   6 found[0] != 0, the state's poses out of the pose bounds, n* outside 1..65536, sad* outside 0..255 n*, |u*| or
     *     |v*| > 16384, or a flagged runner-up with such counts -- all tested before any product;
     *   3 sad* > max_mean n*;
     *   4 a runner-up exists and 1000 sad* n2 > ratio_permille sad2 n* (below 2^50);
     *   7 the translated poses fail the pose bounds;      0 accepted.
     * The translation by (dx, dy) = (S u*, S v*) whole canvas pixels is exact: to[2] += dx ONE, to[5] += dy ONE, from[2] -= from[0] dx +
     * from[1] dy, from[5] -= from[3] dx + from[4] dy (2^24 x 2^18 = 2^42).
     * Accepted: the candidate state is the state with both poses translated, last_fwd = last_inv = identity (a bridge after relocation
     * never replays the motion from before the break), phase 1, bridge run 0; the row is (to, from, 0, frame_clipped, 0, 0).
     * Otherwise: the candidate state is the state, the row (identity, identity, 2, 0, 0, 0) -- map_view then sees nothing and
     * pose_correct reports 4.  ONE launch of one wave.
     * Refused before a launch: a null pointer; max_mean outside 0..255; ratio_permille outside 1..1000; H, W, CH or CW outside
     * 1..16384; |ox| or |oy| > 16384; S not 4, 8 or 16; a pointer not aligned to 8 bytes; cand_state == state. */
    int (*pose_relocate)(const int64_t* found, const int64_t* state, int64_t* cand_state, int64_t* cand_pose, int max_mean, int ratio_permille, int H, int W,
                         int CH, int CW, int ox, int oy, int S, fs_stream stream);

    /* ---- relocate_commit.  correct_out: pose_correct's row for the candidate.  out int64 [8] = (status, S u*, S v*, sad*, n*, sad2, n2,
     * eligible placements); the numbers are found's (0 where found has none).  status: cand_state[28] if it is 1, 2, 3, 4, 6 or 7 (any
     * other value but 0: 6); else 5 (fine registration failed) unless correct_out[0] == 0, the candidate's phase is 1, its row's status
     * 0 and its poses inside the pose bounds; else 0: words 0..27 of the candidate state replace the state's and words 0..13 of the
     * candidate row the row's (the state's spare words and the row's pair counts stay).  With any other status NOTHING is written but
     * out: the chain stays lost exactly as it was, and a coarse-only pose never votes.  1 (not attempted) is also the caller's row for a
     * frame it did not try.  ONE launch of one wave; the decision is taken on the device.
     * Refused before a launch: a null pointer; S not 4, 8 or 16; a pointer not aligned to 8 bytes. */
    int (*relocate_commit)(const int64_t* cand_state, const int64_t* cand_pose, const int64_t* correct_out, int64_t* state, int64_t* pose, const int64_t* found,
                           int S, int64_t* out, fs_stream stream);
} fs_ext12_api;

typedef struct fs_hook_tables12 {
    fs_hook_tables11 base11;
    fs_ext12_api ext12;
} fs_hook_tables12;

/* ---- The FOURTEENTH table.  fs_ext12_api is frozen as well (5 members, 56 bytes; tests/test_merge_cpu.py), so ops added since live in
 * a table of their own, append-only, that the library places directly behind fs_hook_tables12 by the same pattern:
 *     const fs_hook_tables13* t = (const fs_hook_tables13*)fs_test_hooks();   t->ext13.mosaic_merge(...)
 * A library built before this table existed has nothing behind its fs_hook_tables12: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext13.magic == FS_EXT13_MAGIC and ext13.size >= the end of the member it needs. */
#define FS_EXT13_MAGIC 0x4653455854413133ull /* "FSEXTA13" */

typedef struct fs_ext13_api {
    uint64_t magic; /* FS_EXT13_MAGIC */
    size_t size;    /* sizeof(fs_ext13_api) of the library that was built */

    /* ---- MAP-TO-MAP REGISTRATION AND THE MERGE OF TWO MOSAICS (csrc/merge_ops.hip, csrc/merge_defs.h).  OUR DEFINITION:
     * the reference has nothing like it.  Two mosaics A and B (vote canvas, orthophoto, origin each) of overlapping ground, each with a
     * pose chain and an anchor frame of its own, are registered against each other and B is folded into A:
     *   [merge_view -> block_match_modes(cur, view) -> merge_gate -> global_motion (frame_size = mask_size = the window) -> link_correct]
     *   a few times, then mosaic_merge.
     * The same rules as code: csrc/merge_defs.h (host and device) and tests/merge_ref.py (numpy).  All integer, bit for bit.
     *
     * A LINK is int64 [16], shaped like a pose row: words 0..5 b_to_a (B's anchor coordinates -> A's, Q20; to_anchor's place), 6..11
     * a_to_b (from_anchor's place), 12 the status (0 registered, 1 initial: a caller's guess not yet confirmed, 2 no fit, 3 out of the
     * pose bounds), 13..15 inliers, usable rows, rounds done of the fit that registered it.  It is IN BOUNDS under pose_chain's pose
     * bounds (|linear| < 16 ONE both ways, |b_to_a translation| < 2^14 ONE, |a_to_b translation| < 2^20 ONE), tested before any product.
     *
     * THE GATHER all ops share: a canvas is addressed as in mosaic_accumulate (pixel (X, Y) of a canvas with origin (ox, oy) has the
     * anchor coordinate ((2 (X - ox) + 1) << 19, (2 (Y - oy) + 1) << 19)).  The B canvas pixel under A canvas pixel (X, Y) is
     *   (bx, by) = source_pixel(a_to_b, anchor_coord(X, ox_a), anchor_coord(Y, oy_a)) + (ox_b, oy_b)
     * with mosaic_accumulate's source_pixel (it yields pixel indices of B's anchor frame already); it EXISTS iff 0 <= bx < CW_b and
     * 0 <= by < CH_b.  |X - ox_a| <= 2^15, so the products stay below 2^61 as in mosaic_accumulate.
     *
     * merge_view draws, for the window [Y0, Y0 + WH) x [X0, X0 + WW) of A's canvas, four uint8 planes [WH][WW]: cur = luma_of(A's
     * word) (map_view's luma_of; whatever the word holds), valid_a = 1 iff that word's alpha byte is not 0; view = luma_of(B's word
     * under it) and valid_b = 1 where that pixel exists and ITS alpha byte is not 0, both 0 elsewhere -- and everywhere for a link whose
     * status is neither 0 nor 1 or that is out of bounds.  ONE launch, a thread per four pixels of a row, a dword per plane.
     * Refused before a launch: a null pointer; CH or CW of A or B outside 1..16384; |ox| or |oy| of A or B > 16384; a window that is
     * not whole blocks of 16 (WH, WW >= 16, multiples of 16) inside A's canvas; rgba_a == rgba_b; rgba not aligned to 4, link not
     * aligned to 8, a plane not aligned to 4 bytes. */
    int (*merge_view)(const uint32_t* rgba_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b,
                      const int64_t* link, int Y0, int X0, int WH, int WW, uint8_t* cur, uint8_t* view, uint8_t* valid_a, uint8_t* valid_b, fs_stream stream);

    /* ---- merge_gate gates the matcher's table of (cur, view), H x W = the window, IN PLACE.  Row i belongs to the block at
     * (16 (i % (W / 16)), 16 (i / (W / 16))) -- taken from the row's INDEX, not from its words.  The row stays iff that block's own
     * 16 x 16 window lies wholly on valid_a == 1 AND map_gate's rule holds on valid_b: the winner's window [src_x - 8, src_x + 8) x
     * [src_y - 8, src_y + 8) lies inside the plane (tested in 64 bits before a byte is read) and wholly on valid_b == 1.  Every other
     * row becomes the void row (-1, 16, 16, -16, -16, -16, -16); a void row has no window in any plane and stays void.  ONE launch, a
     * wave per row.
     * Refused before a launch: a null pointer; H or W outside 16..16384; blocks != (H / 16) (W / 16); table not aligned to 4. */
    int (*merge_gate)(int32_t* table, int blocks, const uint8_t* valid_a, const uint8_t* valid_b, int H, int W, fs_stream stream);

    /* ---- link_correct folds global_motion's row for (cur, view) into the link, IN PLACE.  The fit's forward model F takes a window
     * pixel to its place in view; with s = (X0 - ox_a, Y0 - oy_a) the correction in A's anchor coordinates is C(P) = F(P - s) + s:
     * F's linear part and the translation F.t + s ONE - F.lin s (whole pixels: exact); the inverse model is conjugated the same way.
     * out int64 [8] = (status, usable, inliers, rounds done, F.t x, F.t y, 0, 0), pose_correct's layout.  In this order:
     *   4  the link's status is neither 0 nor 1;
     *   2  model[12] != 0, or the model or the CONJUGATED pair is out of global_motion's pair bounds (|linear| <= 2 ONE, |t| < 2^16 ONE);
     *   3  the link is out of the pose bounds, or the result would be;
     *   0  a_to_b <- compose(a_to_b, C), b_to_a <- compose(C^-1, b_to_a), the link's status becomes 0 and its words 13..15 the fit's
     *      inliers, usable rows and rounds.
     * On 2, 3 and 4 the link is unchanged.  ONE launch of one wave.
     * Refused before a launch: a null pointer; a window that is not whole blocks of 16 with 0 <= Y0, X0 and Y0 + WH, X0 + WW <= 16384;
     * |ox_a| or |oy_a| > 16384; a pointer not aligned to 8 bytes; model == link. */
    int (*link_correct)(const int64_t* model, int64_t* link, int Y0, int X0, int WH, int WW, int ox_a, int oy_a, int64_t* out, fs_stream stream);

    /* ---- mosaic_merge folds B into A, IN PLACE, under a link whose status is 0 and that is in bounds; under any other link NOTHING of A
     * changes (decided on the device) and counts = (the link's status, 0, ...).  votes uint16 [K][CH][CW] on both sides, the same K; rank
     * and rgba: ortho_accumulate's planes of A and B, all four or all null (votes only).  For every A canvas pixel whose B pixel exists:
     *   votes: for every k < K, votes_a[k] = min(65535, votes_a[k] + votes_b[k][that pixel]) -- nearest neighbour, one owner per A pixel;
     *   orthophoto: where B's rank word is not all ones, ord' = its low word + ordinal_offset; ord' > 0xFFFFFFFE takes nothing; the new
     *   word is (high << 32) | ord' with high = B's high word (mode 0, centre) or 0xFFFFFFFF - ord' (mode 1, latest); A's pixel takes
     *   the word and B's rgba iff the new word is strictly smaller than A's: ties stay with A, and a second identical call changes
     *   nothing in the orthophoto.  VOTES ARE NOT IDEMPOTENT: a second call adds them again.
     * counts int64 [8] = (link status, A pixels whose B pixel exists, of those the pixels where B had a vote, the votes added before
     * saturation, orthophoto pixels taken, 0, 0, 0).
     * TWO launches: a kernel that clears counts, then one workgroup of 256 per 64 x 16 tile of A; a tile B's canvas rectangle cannot
     * reach (mosaic_accumulate's touches with B's origin folded into the translation) returns before touching a canvas.  No canvas
     * takes an atomic; counts go through an LDS tally and one 64-bit atomic per workgroup and non-zero cell.
     * Refused before a launch: a null votes, link or counts pointer, or some but not all of the four orthophoto pointers; CH or CW of
     * A or B outside 1..16384; |ox| or |oy| > 16384; K outside 1..32; mode not 0 or 1; ordinal_offset == 0xFFFFFFFF; A and B the same
     * memory (votes, rank or rgba); votes not aligned to 2, rgba to 4, rank, link or counts to 8 bytes. */
    int (*mosaic_merge)(uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                        const int64_t* link, uint64_t* rank_a, uint32_t* rgba_a, const uint64_t* rank_b, const uint32_t* rgba_b, uint32_t ordinal_offset, int mode,
                        int64_t* counts, fs_stream stream);

    /* ---- merge_patch and link_place: the COARSE PLACEMENT for two mosaics whose link is not known to within the matcher's search, through
     * §3.22's map_coarse(rgba_a) and map_locate, which run unchanged:
     *   merge_patch -> map_coarse -> map_locate -> link_place -> [the fine rounds above on the candidate].
     * merge_patch draws B into A's canvas cells under the link; tl, tv, geom exactly as map_patch writes them.  The geometry is
     * map_patch's box rule on the corners of b_box = [x0, x1) x [y0, y1) (B canvas pixels) under t = b_to_a: a corner (x, y) lies at
     * cx = t00 (x - ox_b) + t01 (y - oy_b) + t02 + ox_a ONE (below 2^41), cy alike; canvas pixels [min cx >> 20, (max cx + ONE - 1) >> 20),
     * widened outwards to whole cells.  status 1: the link's status is neither 0 nor 1.  status 2: the link is out of the pose bounds,
     * or the box's pixels lie more than 2^15 from A's anchor (the gather's products then stay below 2^62).  status 3, 4: map_patch's.
     * status 0: patch cell (i, j) is A's canvas cell (pu0 + i, pv0 + j); it is valid iff the B pixel under every one of its S^2 canvas
     * pixels exists (THE GATHER above) and has been seen; tl is then the rounded mean of their luma_of, as map_coarse's.
     * TWO launches, as map_patch's.
     * Refused before a launch: a null pointer; CH or CW of A or B outside 1..16384; |ox| or |oy| > 16384; S not 4, 8 or 16; A's canvas
     * without a cell; a b_box that is empty or not inside B's canvas; rgba_b not aligned to 4, link or geom to 8 bytes. */
    int (*merge_patch)(const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b, const int64_t* link, int CH_a, int CW_a, int ox_a, int oy_a, int S, int y0,
                       int x0, int y1, int x1, uint8_t* tl, uint8_t* tv, int64_t* geom, fs_stream stream);

    /* ---- link_place turns map_locate's placement into a CANDIDATE link (16 words); `link` is only read.  pose_relocate's acceptance and
     * codes, in this order: 1 the link's status is neither 0 nor 1; 2 found[0] == 1; 6 found[0] != 0, the link out of the pose bounds,
     * or counts that pose_relocate refuses; 3 sad* > max_mean n*; 4 a runner-up with 1000 sad* n2 > ratio_permille sad2 n*; 7 the moved
     * link fails the pose bounds; 0 placed: both affines moved by (S u*, S v*) A canvas pixels with pose_relocate's exact translation,
     * status 1, words 13..15 zero.  With any other code the candidate is the link as it was.  out int64 [8] = relocate_commit's row
     * (code, S u*, S v*, sad*, n*, sad2, n2, eligible placements).  ONE launch of one wave.
     * Refused before a launch: a null pointer; S not 4, 8 or 16; max_mean outside 0..255; ratio_permille outside 1..1000; a pointer not
     * aligned to 8 bytes; cand == link. */
    int (*link_place)(const int64_t* found, const int64_t* link, int S, int max_mean, int ratio_permille, int64_t* cand, int64_t* out, fs_stream stream);
} fs_ext13_api;

typedef struct fs_hook_tables13 {
    fs_hook_tables12 base12;
    fs_ext13_api ext13;
} fs_hook_tables13;

/* ---- The FIFTEENTH table.  fs_ext13_api is frozen as well (6 members, 64 bytes; tests/test_change_cpu.py), so ops added since live in
 * a table of their own, append-only, that the library places directly behind fs_hook_tables13 by the same pattern:
 *     const fs_hook_tables14* t = (const fs_hook_tables14*)fs_test_hooks();   t->ext14.mosaic_change(...)
 * A library built before this table existed has nothing behind its fs_hook_tables13: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext14.magic == FS_EXT14_MAGIC and ext14.size >= the end of the member it needs. */
#define FS_EXT14_MAGIC 0x4653455854413134ull /* "FSEXTA14" */

typedef struct fs_ext14_api {
    uint64_t magic; /* FS_EXT14_MAGIC */
    size_t size;    /* sizeof(fs_ext14_api) of the library that was built */

    /* ---- THE FLOOD-EXTENT CHANGE BETWEEN TWO REGISTERED MOSAICS (csrc/change_ops.hip, csrc/change_defs.h).  OUR DEFINITION:
     * the reference has nothing like it.  Two vote canvases of the same ground, A and B, under a link that ops of the fourteenth table
     * registered, are compared class by class IN A'S CANVAS; neither canvas is changed.  The same rules as code: csrc/change_defs.h (host
     * and device) and tests/change_ref.py (numpy).  All integer, bit for bit.
     *
     * votes_a uint16 [K][CH_a][CW_a] with origin (ox_a, oy_a), votes_b uint16 [K][CH_b][CW_b] with origin (ox_b, oy_b), the same K in
     * 1..32; link int64 [16] as the fourteenth table defines it; min_votes 1..65535, min_conf 0..255, tolerance r 0..8 pixels;
     * watch_set: bit k for k < K.
     *
     * THE DECIDED CLASS of a canvas pixel: with total = the sum of its K counts and most = the largest, taken by the first class that
     * has it (mosaic_resolve's winner: strictly more votes, so the lowest id on a tie), it is that class iff total >= min_votes and
     * vote_confidence(most, total) = (255 most + total / 2) / total >= min_conf; 255 otherwise.
     *
     * THE CLASS PLANES, uint8 [CH_a][CW_a], always written whole: cls_a[Y][X] is the decided class of A's pixel; cls_b[Y][X] the
     * decided class of the B pixel under it through THE GATHER of the fourteenth table, 255 where that pixel does not exist, and 255
     * everywhere unless the link's status is 0 and it is in bounds (decided on the device, as in mosaic_merge).
     *
     * THE WINDOW SETS: win_a(X, Y) is the OR of 1u << cls_a over the pixels of [X - r, X + r] x [Y - r, Y + r] that lie inside A's
     * canvas and whose cls_a is not 255; win_b(X, Y) the same over cls_b.
     *
     * THE CHANGE CODE, change uint8 [CH_a][CW_a], with ca = cls_a and cb = cls_b at the pixel, the first that applies:
     *   0  not comparable: ca or cb is 255;
     *   1  same: ca == cb;
     *   2  differs, but explained by a shift of at most r pixels: bit ca is in win_b AND bit cb is in win_a (never with r = 0);
     *   3  changed, ca and cb both in watch_set or both outside it;
     *   4  gained: ca not in watch_set, cb in it ("flooded" when B is the later flight and watch_set is water);
     *   5  lost: ca in watch_set, cb not.
     * Both tests of code 2 are needed: a misregistration of at most r pixels passes both, and a class B brings that A holds nowhere
     * within r keeps every one of its pixels.
     *
     * transitions int64 [2][K][K]: [0][ca][cb] counts the comparable pixels (code >= 1), [1][ca][cb] those with code >= 3.
     * counts int64 [8] = (the link's status, A pixels whose B pixel exists, comparable, same, explained, changed-other, gained, lost).
     * Under a link that does not merge counts = (status, 0, ...), transitions and change are all 0.
     *
     * THREE launches on one stream: a kernel that clears counts and transitions; change_classes, one workgroup of 256 per 64 x 16 tile
     * of A, a thread owning a column of four rows and looping over K (a tile that B's canvas rectangle cannot reach resolves A and
     * writes 255 to cls_b without touching B); change_codes on the same tiles, 1u << cls of both planes staged in LDS for the tile plus
     * an apron of r pixels clipped at the canvas edge, the window OR done separably (rows, then columns), r = 0 an instantiation of its
     * own that stages nothing.  Every plane pixel has one owner; counts and transitions go through an LDS tally of 8 + 2 K^2 dwords
     * and one 64-bit atomic per workgroup and non-zero cell.  Nothing else takes an atomic.
     * Refused before a launch: a null pointer; K outside 1..32; CH or CW of A or B outside 1..16384; |ox| or |oy| > 16384; min_votes
     * outside 1..65535, min_conf outside 0..255, tolerance outside 0..8; a watch_set bit at or above K; votes_a == votes_b; an output
     * that overlaps an input; votes not aligned to 2, link, counts or transitions not aligned to 8 bytes. */
    int (*mosaic_change)(const uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                         const int64_t* link, int min_votes, int min_conf, int tolerance, uint32_t watch_set, uint8_t* change, uint8_t* cls_a, uint8_t* cls_b,
                         int64_t* transitions, int64_t* counts, fs_stream stream);
} fs_ext14_api;

typedef struct fs_hook_tables14 {
    fs_hook_tables13 base13;
    fs_ext14_api ext14;
} fs_hook_tables14;

/* ---- The SIXTEENTH table.  fs_ext14_api is frozen as well (1 member, 24 bytes; tests/test_access_cpu.py), so ops added since live in
 * a table of their own, append-only, that the library places directly behind fs_hook_tables14 by the same pattern:
 *     const fs_hook_tables15* t = (const fs_hook_tables15*)fs_test_hooks();   t->ext15.mask_access(...)
 * A library built before this table existed has nothing behind its fs_hook_tables14: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext15.magic == FS_EXT15_MAGIC and ext15.size >= the end of the member it needs. */
#define FS_EXT15_MAGIC 0x4653455854413135ull /* "FSEXTA15" */
#define FS_ACCESS_NONE 0xFFFFFFFFu           /* mask_access' d where no route exists or the cheapest one costs more than R */
#define FS_ACCESS_TILE 32                    /* the edge of the tile one workgroup of mask_access relaxes */
#define FS_ACCESS_MAX_COST 0x7FFFF000u       /* the largest R: 2^31 - 4096 */

typedef struct fs_ext15_api {
    uint64_t magic; /* FS_EXT15_MAGIC */
    size_t size;    /* sizeof(fs_ext15_api) of the library that was built */

    /* ---- DRY-ROUTE REACHABILITY: THE COST FIELD (csrc/access_ops.hip, csrc/access_defs.h).  OUR DEFINITION: the reference
     * has nothing like it.  The cheapest route from any seed pixel to every pixel over ground that can be walked on, around barriers.
     * The same rules as code: csrc/access_defs.h (host and device) and tests/access_ref.py (a heap Dijkstra and a literal relaxation).
     * Integers throughout.  Costs are in MASK PIXELS of whatever produced the mask, tenths of a pixel on the 5-7 chamfer metric.
     * Inputs, per frame:
     *   mask          uint8 [n][H][W], at any byte address.  Ids >= 32 (the mosaic's 255 = never seen among them) are always barriers.
     *   seeds         uint8 [n][H][W], at any byte address; non-zero marks a seed.
     *   cost          uint8 [32] in HOST memory (read during the call): the walking cost of class k; 0 = barrier.  Not all zero.
     *   terminal_set  uint32: a class in it with cost > 0 is TERMINAL: it can be arrived at, never left or crossed.
     *   connectivity  4 or 8.      max_cost  R: 0 = the largest allowed, FS_ACCESS_MAX_COST; else 1 <= R <= FS_ACCESS_MAX_COST.
     * A pixel is PASSABLE if its class has cost > 0 and is not terminal.  A seed pixel counts only if it is passable.
     * A MOVE goes from a pixel p to a neighbour q of the same frame and costs step * (cost[mask[p]] + cost[mask[q]]), step = 5 for an
     * orthogonal move and 7 for a diagonal one (connectivity 8 only).  It is allowed iff p is passable, q is passable or terminal, and,
     * for a diagonal move, both pixels orthogonally between p and q are passable (no corner cutting: a diagonal line of barrier pixels
     * one pixel wide is a wall).  The largest move costs 7 * 510 = 3570, so no sum below passes 2^31.
     * Outputs:
     *   d       uint32 [n][H][W]: the minimum total cost of a sequence of allowed moves from any seed pixel of the same frame that counts;
     *           0 on such a seed; FS_ACCESS_NONE where no sequence exists or the minimum exceeds R.  A value that is not FS_ACCESS_NONE is
     *           the exact minimum: R only removes values.
     *   origin  int32 [n][H][W], or NULL: the raster index y * W + x of a seed pixel that attains d, the smallest index among several (the
     *           minimum of the 64-bit key d << 32 | origin over all routes); -1 where d is FS_ACCESS_NONE.
     *   status  int32 [n][4], written on the device: (converged 0/1, the rounds of this call in which a value was lowered, the pixels
     *           with a value, 0).
     * THE CONTRACT.  The op enqueues `rounds` (1..65535) rounds whatever happens in them.  The fixed point is unique, so once status
     * says converged the planes are a function of the inputs alone.  Where it does not, every value that is not FS_ACCESS_NONE is still
     * the cost of a real route: an upper bound, never too small, and origin is the seed of such a route.  resume = 1: the op starts from
     * the d (and origin) planes as an earlier call with the same other arguments left them, instead of from the seeds, and goes on
     * towards the same fixed point; a converged frame stays exactly as it is.  The second status word depends on how the tiles cut the
     * frame and on which of two neighbouring tiles of a round wrote first; the planes and the other words do not once converged.
     * LAUNCHES.  2 + rounds.  (1) Every pixel's key d << 32 | origin as one 64-bit word of the workspace (from the seeds, or from the
     * planes); every tile dirty.  (2) One round: one workgroup of 256 per FS_ACCESS_TILE x FS_ACCESS_TILE tile; a tile that is not dirty
     * returns at once; a dirty one stages its keys and a ring of one pixel in LDS (34 x 34 x 10 bytes), turns the classes into the eight
     * move costs of each of its four pixels per thread, and sweeps in gather form -- all read, a barrier, the owners write, a barrier --
     * until a sweep lowers nothing, at most 128 times (then it marks itself dirty); lowered keys go back as aligned 64-bit words; the
     * tile marks dirty every neighbour tile whose ring holds a pixel it lowered.  Nothing waits on another workgroup: a tile that reads a
     * neighbour's key while that neighbour lowers it sees the old or the new word and is marked by that neighbour either way.  (3) The
     * keys become the planes; status.  The two sets of dirty flags alternate by the round's parity.
     * workspace = FS_MASK_ACCESS_WORKSPACE_BYTES(n, H, W) bytes at an 8-byte aligned address, the caller's: the keys, two dwords per
     * tile, four per frame.  Its contents need not survive between calls.  Nothing is allocated, synchronised or read back on the host;
     * `cost` is read during the call.
     * Refused before a launch: a null mask, seeds, cost, d, status or workspace; n < 1 or n > 65535; H or W < 1; H * W >= 2^31 - 1; H or
     * W > 32768; connectivity not 4 or 8; R above FS_ACCESS_MAX_COST; rounds outside 1..65535; resume not 0 or 1; d, origin or status not
     * aligned to 4 bytes, the workspace not to 8; a cost table that is all zero. */
#define FS_MASK_ACCESS_WORKSPACE_BYTES(n, H, W)                                                                                                      \
    ((size_t)(n) * (size_t)(H) * (size_t)(W) * 8 +                                                                                                   \
     (size_t)(n) * (((size_t)(H) + FS_ACCESS_TILE - 1) / FS_ACCESS_TILE) * (((size_t)(W) + FS_ACCESS_TILE - 1) / FS_ACCESS_TILE) * 8 + (size_t)(n) * 16)
    int (*mask_access)(const uint8_t* mask, const uint8_t* seeds, int n, int H, int W, const uint8_t* cost, uint32_t terminal_set, int connectivity,
                       uint32_t max_cost, int rounds, int resume, uint32_t* d, int32_t* origin, int32_t* status, void* workspace, fs_stream stream);

    /* ---- The cost field tabulated per class and per region (csrc/access_ops.hip).  OUR DEFINITION; the sibling of
     * region_proximity.
     * Inputs:
     *   mask    uint8 [n][H][W];   d uint32 [n][H][W] and origin int32 [n][H][W] (or NULL) as mask_access wrote them;
     *   index   int32 [n][H][W] and counts int64 [n][2], region_table's;   K classes 1..255;   max_regions 1..65536.
     * rows(f) = min(max(counts[f][1], 0), max_regions); a pixel p of frame f BELONGS to row r if index[f][p] == r and 0 <= r < rows(f).
     * Outputs, each cleared on the stream and written whole by every call:
     *   reach  int64 [n][K][4]: per class k (the pixels with mask == k, those of them with a value, the sum of their values, the
     *          largest value; the last two 0 without one).
     *   rows   int64 [n][max_regions][8], row r of frame f = (min_d, at_x, at_y, origin_x, origin_y, origin_row, valued, max_d): min_d
     *          the smallest d other than FS_ACCESS_NONE over the row's pixels, (at_x, at_y) the pixel that attains it, the lowest raster
     *          index on a tie; (origin_x, origin_y) = origin at that pixel, origin_row = index at the origin pixel, -1 if that pixel
     *          belongs to no row; valued = the row's pixels with a value, max_d the largest of them.  A row none of whose pixels has a
     *          value: (-1, -1, -1, -1, -1, -1, 0, -1).  origin == NULL: origin_x = origin_y = origin_row = -1.  Rows at and behind
     *          rows(f) are zero.
     * LAUNCHES.  Three: set up; one pass over the pixels (an LDS table [K][4] per workgroup, a wave whose 64 pixels are of one class
     * adding to it once, flushed with one 64-bit atomic per non-zero cell; per row a 64-bit atomic minimum of d << 32 | raster index, an atomic sum and an atomic maximum, once per run of a
     * row along the 1024 consecutive pixels a wave owns); finish.  Integer sums, minima and maxima: the order does not matter.  No
     * workspace; nothing is allocated, synchronised or read on the host.
     * Refused before a launch: a null mask, d, index, counts, reach or rows; n, H, W as mask_access; K or max_regions out of range; d,
     * origin or index not aligned to 4 bytes; counts, reach or rows not aligned to 8. */
    int (*region_access)(const uint8_t* mask, const uint32_t* d, const int32_t* origin, const int32_t* index, const int64_t* counts, int n, int H, int W,
                         int K, int max_regions, int64_t* reach, int64_t* rows, fs_stream stream);
} fs_ext15_api;

typedef struct fs_hook_tables15 {
    fs_hook_tables14 base14;
    fs_ext15_api ext15;
} fs_hook_tables15;

/* ---- The SEVENTEENTH table.  fs_ext15_api is frozen as well (2 members, 32 bytes; tests/test_ground_cpu.py), so ops added since live in
 * a table of their own, append-only, that the library places directly behind fs_hook_tables15 by the same pattern:
 *     const fs_hook_tables16* t = (const fs_hook_tables16*)fs_test_hooks();   t->ext16.ground_area(...)
 * A library built before this table existed has nothing behind its fs_hook_tables15: a caller that may meet one checks the older
 * tables' magics and sizes first, then t->ext16.magic == FS_EXT16_MAGIC and ext16.size >= the end of the member it needs. */
#define FS_EXT16_MAGIC 0x4653455854413136ull /* "FSEXTA16" */
#define FS_GROUND_MAX_PLANES 8               /* uint8 planes of one ground_rectify call */
#define FS_GROUND_NO_POINT INT64_MIN         /* ground_points: both words of a point the model cannot place */

typedef struct fs_ext16_api {
    uint64_t magic; /* FS_EXT16_MAGIC */
    size_t size;    /* sizeof(fs_ext16_api) of the library that was built */

    /* ---- GEOREFERENCING: GROUND AREAS (csrc/ground_ops.hip, csrc/ground_defs.h).  OUR DEFINITION: the reference has nothing
     * like it.  The same rules as code: csrc/ground_defs.h (host and device) and tests/ground_ref.py (vectorised numpy and literal loops).
     * A MODEL is nine float64 (a0 a1 a2 b0 b1 b2 c0 c1 c2) in HOST memory, read during the call.  The FORWARD model takes anchor pixel
     * coordinates (i, j) -- canvas lattice point (X, Y) is i = X - ox, j = Y - oy; canvas pixel (X, Y) covers [X, X+1) x [Y, Y+1) -- to
     * millimetres east and north of a ground origin that only the host knows.
     * THE CORNER of lattice point (i, j), all in float64, one operation per statement, no contraction:
     *     ne = (a0*i + a1*j) + a2;  nn = (b0*i + b1*j) + b2;  d = (c0*i + c1*j) + c2;  E = (int64) floor(ne / d + 0.5), N likewise.
     * THE AREA of canvas pixel (X, Y): area2 = the shoelace sum of its corners (X,Y), (X+1,Y), (X+1,Y+1), (X,Y+1) about the first, in
     * int64: twice the signed area in mm^2; times the model's ORIENTATION, the sign of det(model) (-1 with north up), it is positive;
     * a pixel whose oriented area2 is <= 0 is FOLDED: counted, not summed.  Adjacent pixels share corners, so the areas of any set of
     * pixels sum exactly to the shoelace of the set's boundary.
     * Inputs:  cls uint8 [CH][CW] (mosaic_resolve's class plane, mosaic_change's change plane, any id plane; 255 = unseen: skipped);
     *          K classes 1..255;  index int32 [CH][CW] (region_table's, of one frame) with max_regions 1..65536, or NULL with 0.
     * Outputs, cleared on the stream by a kernel and written whole by every call:
     *   class_area2   int64 [K]: the sum of the oriented area2 over the pixels of class k that are not folded;
     *   region_area2  int64 [max_regions] (NULL with max_regions 0): the same over the summed pixels whose index is r;
     *   counts        int64 [4] = (pixels summed, folded pixels of an id < K, pixels with K <= id < 255, 0).
     * LAUNCHES.  Two: clear; one workgroup of 256 per 64 x 16 canvas tile.  It reads its bytes and returns if all are 255; otherwise it
     * projects its 65 x 17 corners once into LDS, sums classes through an int64 LDS histogram flushed with one 64-bit atomic per
     * non-zero cell, and merges the region sums per run of equal rows in the wave.  Integer sums: the order does not matter.
     * THE BOUNDS (ground_defs.h derives why no product and no sum leaves 63 bits).  Refused before a launch, naming the model: a value
     * that is not finite; det(model) = 0; the denominator not positive at each of the four canvas corners; the largest corner
     * denominator more than 4 times the smallest; |E| or |N| >= 2^31 - 1 mm at a canvas corner; one pixel's corner differences that may
     * reach 2^30 (bounded through (|a| + the largest corner |E| times |c|) / the smallest denominator); a corner quadrilateral of 2^61 mm^2 or more.  Also refused:
     * a null cls, forward, class_area2 or counts; CH or CW outside 1..16384; |ox| or |oy| > 16384; K or max_regions out of range; index
     * or region_area2 without max_regions >= 1 or the reverse; index not aligned to 4 bytes, an output not to 8. */
    int (*ground_area)(const uint8_t* cls, int CH, int CW, int ox, int oy, const double* forward, int K, const int32_t* index, int max_regions,
                       int64_t* class_area2, int64_t* region_area2, int64_t* counts, fs_stream stream);

    /* ---- GEOREFERENCING: NORTH-UP RASTERS (csrc/ground_ops.hip).  OUR DEFINITION.  Raster pixel (u, v) of a GH x GW raster
     * with integer gsd_mm whose top-left ground CORNER is (e0_mm, ntop_mm), through the INVERSE model (millimetres to anchor coordinates):
     *     Eg = e0 + (u + 0.5) * gsd;  Ng = ntop - (v + 0.5) * gsd;  x, y = the three sums and two divisions of the corner rule.
     * A pixel with |x| or |y| >= 2^20 (or not a number) takes the fills.  uint8 planes, NEAREST: canvas X = floor(x) + ox, Y = floor(y) + oy;
     * outside the canvas: `fill`.  COLOUR from the orthophoto's rgba plane (r | g << 8 | b << 16 | a << 24, a = 0: unseen): taps at
     * floor(x - 0.5), floor(y - 0.5) and one further; Q8 weights w = floor(frac * 256); per channel (sum of w * c + 32768) >> 16; a tap
     * that is unseen or off the canvas makes the pixel take the nearest tap (floor(x), floor(y)); an unseen nearest tap gives rgb_fill.
     * Inputs:  nplanes 0..FS_GROUND_MAX_PLANES; planes, outs = HOST arrays of nplanes device pointers, uint8 [CH][CW] and [GH][GW];
     *          rgba uint32 [CH][CW] with rgb_out uint8 [GH][GW][3], or both NULL; fill 0..255; rgb_fill = r | g << 8 | b << 16.
     * LAUNCHES.  One: a workgroup of 256 per 64 x 16 raster tile, one owner per raster pixel, no atomics, all planes at once.  A tile whose
     * four lattice corners map beyond the SAME side of the canvas box grown by one pixel writes the fills and returns: with a positive
     * denominator the tile lies in the hull of those four points.
     * Refused before a launch, naming the value: an inverse value that is not finite; the denominator not positive at the four raster
     * corners, or their ratio above 4; CH, CW, GH or GW outside 1..16384; |ox| or |oy| > 16384; gsd_mm outside 1..2^20; e0_mm or ntop_mm
     * 2^40 or more from the origin; nplanes out of range; a null plane; rgba without rgb_out or the reverse; neither a plane nor rgba;
     * fill or rgb_fill out of range; rgba not aligned to 4 bytes. */
    int (*ground_rectify)(const double* inverse, int CH, int CW, int ox, int oy, int GH, int GW, int gsd_mm, int64_t e0_mm, int64_t ntop_mm, int nplanes,
                          const uint8_t* const* planes, uint8_t* const* outs, const uint32_t* rgba, uint8_t* rgb_out, int fill, uint32_t rgb_fill,
                          fs_stream stream);

    /* ---- GEOREFERENCING: POINTS (csrc/ground_ops.hip).  points int32 [n][2] = (x, y) canvas lattice points (the vertices of
     * region_outlines and outline_simplify, pixel corners) -> out int64 [n][2] = (E, N) millimetres: THE CORNER of ground_area, the same
     * function, so a polygon's shoelace over these points equals ground_area's sum of its pixels.  A point with |x| or |y| > 2^20, a
     * denominator that is not positive there or a result of 2^53 or more gets FS_GROUND_NO_POINT in both words.  One launch.
     * Refused: a null pointer; n outside 1..2^28; |ox| or |oy| > 16384; a model value that is not finite or det = 0; points not aligned
     * to 4 bytes, out not to 8. */
    int (*ground_points)(const int32_t* points, int n, const double* forward, int ox, int oy, int64_t* out, fs_stream stream);
} fs_ext16_api;

typedef struct fs_hook_tables16 {
    fs_hook_tables15 base15;
    fs_ext16_api ext16;
} fs_hook_tables16;

const fs_test_api* fs_test_hooks(void);

#ifdef __cplusplus
}
#endif
#endif /* FLOODSEG_TEST_H_ */
