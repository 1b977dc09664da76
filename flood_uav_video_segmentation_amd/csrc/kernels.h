// Launcher declarations for the hand-written gfx950 kernels.
// All tensors are fp32. Activations inside the library are NHWC ("pixel-major"):
// element (b, y, x, c) lives at ((b*H + y)*W + x) * ld + c, ld >= C (ld > C when the
// tensor is a channel slice of a wider concat buffer).
#pragma once
#include "common.h"

namespace fs {

// ---------------------------------------------------------------------------------
// Implicit-GEMM convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
//   out[m][n] = act( scale[n] * sum_k A[m][k] * Wt[n][k] + shift[n] (+ res[m][n]) )
//   m = (b, oy, ox) output pixel, n = output channel, k = (r, s, c) filter tap/channel.
// Restates nn.Conv2d + eval BatchNorm2d + ReLU (+ residual add) of the reference's
// Bottleneck (model/resnet.py:76-96) and PSPNet heads (model/pspnet.py:21-26, 70-76).
// ---------------------------------------------------------------------------------
struct ConvParams {
    const float* in;    int ld_in;   // NHWC input
    const float* wgt;                // [Cout][KH*KW*Cin], k ordered (r, s, c), c fastest
    int ld_wgt;                      // floats between two filter rows; 0 = KH*KW*Cin (+ Cin2).  > K: the launch multiplies a K-slice
                                     // of wider rows (split-K groups of one nn.Linear: group g takes columns g*Cin .. of W[out][in])
    const float* scale;              // [Cout] or nullptr (=1)
    const float* shift;              // [Cout] or nullptr (=0)
    const float* res;   int ld_res;  // residual, NHWC at output resolution, or nullptr
    float* out;         int ld_out;  // NHWC output
    int B, H, W, Cin;
    int Ho, Wo, Cout;
    int KH, KW, stride, pad, dil;
    // second input of a concatenated-K GEMM (nullptr = none): a 1x1 conv with stride `stride2` over an H2 x W2 x Cin2 map whose
    // output geometry is Ho x Wo; its Cin2 weights follow the first conv's K in every filter row.  The bottleneck block with a
    // projection shortcut runs conv3 and downsample as ONE launch this way (model/resnet.py:86-94); first conv must be 1x1 s1.
    const float* in2;   int ld_in2;
    int Cin2, stride2, H2, W2;
    int relu;  // epilogue activation: 0 none, 1 ReLU, 2 GELU (erf)
    int res_touch;  // split route (round 5): != 0 -> after the barrier of the last-but-one chunk every lane touches two 128-B lines of the
                    // residual tile (dead loads), so that the epilogue's 64 residual loads per lane find them in L2: -3 % on layer3 /
                    // layer4 conv3, -7 % on layer1 / layer2 conv3 (profiles/r05_experiments.txt section 3); same results bit for bit
    int korder;  // weight k order: 0 = (r, s, c) ; 1 = (c/32, r, s, c%32)
    // grouped GEMM (Winograd: one GEMM per transform position): group g uses in + g*g_in, wgt + g*g_wgt, out + g*g_out
    int groups;  // 0 or 1 = plain
    long long g_in, g_wgt, g_out;  // strides in floats
    // Split-operand route (conv_igemm_dma_f32<..., SPLIT = true>): the SAME filters as `wgt`, each fp32 value as its three bf16 terms
    // (split.h), stored as three planes [3][rows][ld_wgt or K] of bf16 (split_bf16x3).
    // nullptr = the fp32-MFMA kernel.  plane_bytes = bytes of one plane.
    const void* wgt3;
    unsigned plane_bytes;
    // Segmenter qkv Linear (round 6, 128 x 96 tile of the split route only): kv_k != nullptr -> the launch is grouped by IMAGE (groups = B,
    // M = the tokens of one image, so a tile's rows are keys of one image and 32-row blocks are aligned with the attention's 16-key groups)
    // and the epilogue of the K and V column tiles writes the attention kernel's operand planes -- K as three bf16 planes [bh][Npad][64],
    // V transposed as three planes [bh][64][Npad] in the key order of the S^T accumulator (vit_ops.hip::attention_split_kv_kernel, whose
    // work this is), keys N .. Npad-1 as zeros -- instead of fp32 rows; the Q columns are stored as usual.  Cout = 3 * kv_heads * 64.
    unsigned short* kv_k;
    unsigned short* kv_vt;
    int kv_N, kv_Npad, kv_heads;
    unsigned kv_plane_bytes;   // bytes of one plane of K (= of V^T): B * heads * Npad * 64 * 2
    int kv_b;                  // image of this workgroup's group (set by the kernel)
};
// tile: 0 = heuristic, 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 64x128, 6 = 128x96 (split route only); any other id is refused
int launch_conv_igemm(const ConvParams& p, hipStream_t s, int tile = 0);
const char* conv_igemm_tile_name(const ConvParams& p, int tile = 0);
// planes[t][i] (t = 0, 1, 2; bf16) = term t of w[i] as split.h defines it (split3); ConvParams::wgt3
int launch_split_bf16x3(const float* w, long long n, void* planes, hipStream_t s);

// Host-side builders: every ConvParams of the library comes from conv2d_params, directly or through gemm_params and the layer-level
// builders on top of them (winograd_gemm_params below, conv_params / dual_conv_params / ppm_z_params / linear_*_params in net.h).
// output size of a conv or pooling window along one axis (nn.Conv2d / nn.MaxPool2d, floor)
static inline int conv_out_size(int in, int k, int stride, int pad, int dil) { return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1; }
static inline ConvParams conv2d_params(const float* in, int ld_in, const float* wgt, const float* scale, const float* shift, const float* res, int ld_res,
                                       float* out, int ld_out, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                                       int relu, int korder) {
    ConvParams p{};
    p.in = in; p.ld_in = ld_in; p.wgt = wgt; p.scale = scale; p.shift = shift; p.res = res; p.ld_res = ld_res; p.out = out; p.ld_out = ld_out;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.Ho = conv_out_size(H, KH, stride, pad, dil);
    p.Wo = conv_out_size(W, KW, stride, pad, dil);
    p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad; p.dil = dil; p.relu = relu; p.korder = korder;
    return p;
}
// out[rows][N] (ld_out) = in[rows][K] (ld_in) x w[N][K]^T: a 1x1 conv over a rows x 1 map; no scale / shift / residual / activation
static inline ConvParams gemm_params(const float* in, int ld_in, const float* w, float* out, int ld_out, int rows, int K, int N) {
    return conv2d_params(in, ld_in, w, nullptr, nullptr, nullptr, 0, out, ld_out, 1, rows, 1, K, N, 1, 1, 1, 0, 1, 0, 0);
}
// points a launch at the three bf16 planes of its filter bank of `elems` floats (the op-level hooks; the networks go through split_use)
static inline void attach_planes(ConvParams& p, const void* planes, size_t elems) {
    p.wgt3 = planes;
    p.plane_bytes = (unsigned)(elems * 2);
}

// ---------------------------------------------------------------------------------
// Stem convolution with Cin = 3 read straight from the caller's NCHW frame
// (model/resnet.py:110 3x3 s2 p1; torchvision ResNet 7x7 s2 p3), + BN + ReLU, NHWC out.
// ---------------------------------------------------------------------------------
// Where the B input images of a forward pass live.  Plain mode (ncrops == 0): images 0 .. B1-1 are in[b] and images
// B1 .. B-1 are in2[b - B1], both NCHW [*,3,H,W] (the two key frames of a window are two tensors in the reference's API,
// flow/model.py:189-204: reading both in place replaces a torch.cat).  Crop mode (ncrops > 0, the sliding-crop route of
// flow/base.py:182-209): `in` and `in2` are two FULL frames [1,3,FH,FW]; image b < ncrops is the H x W window of `in` whose
// top-left corner is (cy[b], cx[b]), image ncrops + b the same window of `in2` -- the crops are never copied out.
struct FrameSrc {
    const float* in;
    const float* in2;
    int B1;
    int ncrops, FH, FW;
    short cy[32], cx[32];
};
static inline FrameSrc frames_plain(const float* in, const float* in2, int B1) {
    FrameSrc f{};
    f.in = in;
    f.in2 = in2;
    f.B1 = B1;
    return f;
}

struct StemParams {
    FrameSrc src;
    const float* wgt; // [KH*KW*3][Cout]  (tap-major, Cout fastest)
    const float* scale; const float* shift;
    float* out; int ld_out;  // NHWC [B,Ho,Wo,Cout]
    int B, H, W, Ho, Wo, Cout, KH, KW, stride, pad;
    int split;  // != 0: the split-operand route (three bf16 terms per fp32 value, bf16 matrix cores, fp32 accumulation), round 5
};
int launch_stem_conv(const StemParams& p, hipStream_t s);
static inline StemParams stem_params(const FrameSrc& src, const float* wgt, const float* scale, const float* shift, float* out, int B, int H, int W,
                                     int Cout, int KH, int KW, int stride, int pad, int split) {
    StemParams p{};
    p.src = src; p.wgt = wgt; p.scale = scale; p.shift = shift; p.out = out; p.ld_out = Cout;
    p.B = B; p.H = H; p.W = W; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad; p.split = split;
    p.Ho = conv_out_size(H, KH, stride, pad, 1);
    p.Wo = conv_out_size(W, KW, stride, pad, 1);
    return p;
}

// MaxPool2d(kernel 3, stride 2, padding 1) NHWC (model/resnet.py:117).
int launch_maxpool3x3s2(const float* in, int ld_in, float* out, int ld_out, int B, int H, int W, int C,
                        int Ho, int Wo, hipStream_t s);

// AdaptiveAvgPool2d(bin) NHWC -> [B][bin*bin][C] (model/pspnet.py:22; torchvision ASPPPooling).
int launch_adaptive_avgpool(const float* in, int ld_in, float* out, int B, int H, int W, int C, int bin,
                            hipStream_t s);

// bins 1, 2, 3 from the 6x6 cell means (all windows equal-sized: H, W multiples of 6)
int launch_ppm_pool_combine(const float* cell_mean, float* out1, float* out2, float* out3, int B, int C, hipStream_t s);

// Small-M 1x1 convolution (+scale/shift+ReLU): out[m][n] = act(scale[n]*dot(in[m], w[n]) + shift[n]).
// Used for the pooled PPM / ASPP-pooling branches (M = B*bin*bin <= ~100).
int launch_rowdot_1x1(const float* in, int ld_in, const float* wgt, const float* scale, const float* shift,
                      float* out, int ld_out, int M, int K, int N, int relu, hipStream_t s);
// up to four such problems of one (K, N, ld_in, ld_out) in ONE launch (the four pyramid levels: M = B, 4B, 9B, 36B)
struct RowdotProblem { const float* in; const float* wgt; const float* scale; const float* shift; float* out; int M; };
struct RowdotBatch { RowdotProblem p[4]; };
int launch_rowdot_1x1_batch(const RowdotBatch& pb, int nprob, int ld_in, int ld_out, int K, int N, int relu, hipStream_t s);

// Bilinear (align_corners as given) upsample of a tiny [B][hi*wi][C] map into a channel
// slice of an NHWC buffer (PPM: model/pspnet.py:33, align_corners=True).
int launch_upsample_into(const float* in, int hi, int wi, float* out, int ld_out, int B, int Ho, int Wo,
                         int C, int align_corners, hipStream_t s);

// Final classifier 1x1 conv with bias, NHWC in -> NCHW out (model/pspnet.py:75).
int launch_classifier_nchw(const float* in, int ld_in, const float* wgt /*[K][C]*/, const float* bias,
                           float* out /*[B,K,H,W]*/, int B, int HW, int C, int K, hipStream_t s);

// ---------------------------------------------------------------------------------
// Layout / weight packing
// ---------------------------------------------------------------------------------
int launch_pack_oihw_to_ohwi(const float* w, float* out, int O, int I, int KH, int KW, hipStream_t s);
int launch_pack_oihw_to_hwio(const float* w, float* out, int O, int I, int KH, int KW, hipStream_t s);
// [O][I/32][KH][KW][32]: the taps of one 32-channel slab are consecutive along k (ConvParams::korder == 1), so the
// pixel lines a 3x3 conv re-reads for its 9 taps are touched back to back and hit in L2.
int launch_pack_oihw_chunk_major(const float* w, float* out, int O, int I, int KH, int KW, hipStream_t s);
// out[(tap*O + o)*nc + c] = w[o][c0 + c][tap]: input-channel slice of an OIHW bank as a [taps*O][nc] 1x1 filter matrix
int launch_pack_slice_tap_major(const float* w, float* out, int O, int I, int c0, int nc, int taps, hipStream_t s);
// PSPNet head finish (net_ops.hip): v = act(scale * (T + sum_b conv-of-upsampled-pyramid term from Z_b) + shift), then the classifier
// 1x1 conv + bias (model/pspnet.py:75) on v while it is in registers: T (the raw backbone conv sums) is read once and never written
// back, logits come out NCHW [B][K][H][W].  scratch: ppm_term_scratch_floats(B, H, C) floats (row-collapsed pyramid term)
size_t ppm_term_scratch_floats(int B, int H, int C);
int launch_ppm_term_classify(const float* T, int ld, const float* const Z[4], const int bins[4], float* scratch, const float* scale,
                             const float* shift, int B, int H, int W, int C, int relu, const float* cls_w /*[K][C]*/, const float* cls_b,
                             float* logits_nchw, int K, hipStream_t s);
// out[o][0..Ka) = sa[o] * wa[o][:], out[o][Ka..Ka+Kb) = sb[o] * wb[o][:]; shift_out[o] = ha[o] + hb[o]: the filter bank and bias of
// BN_a(conv_a(x)) + BN_b(conv_b(y)) written as one GEMM over the concatenated K (both 1x1)
int launch_concat_scaled_filters(const float* wa, const float* sa, const float* ha, int Ka, const float* wb, const float* sb, const float* hb,
                                 int Kb, float* out, float* shift_out, int O, hipStream_t s);
int launch_nchw_to_nhwc(const float* in, float* out, int ld_out, int B, int C, int HW, hipStream_t s);
int launch_nhwc_to_nchw(const float* in, int ld_in, float* out, int B, int C, int HW, hipStream_t s);

// ---------------------------------------------------------------------------------
// Flow / interpolation tail (flow/model.py:184-249, flow/base.py:275-276)
// ---------------------------------------------------------------------------------
// F.grid_sample(mode=bilinear, padding_mode=border), NCHW in/out, N = 1..B.
int launch_grid_sample_nchw(const float* in, int B, int C, int Hi, int Wi, const float* grid, int Hg, int Wg,
                            float* out, int align_corners, hipStream_t s);
// Same on NHWC tensors (feature-based mode, C = 4096).
int launch_grid_sample_nhwc(const float* in, int ld_in, int B, int C, int Hi, int Wi, const float* grid, int Hg,
                            int Wg, float* out, int ld_out, int align_corners, hipStream_t s);
// F.interpolate(mode=bilinear), NCHW.
int launch_resize_bilinear_nchw(const float* in, int BC, int Hi, int Wi, float* out, int Ho, int Wo,
                                int align_corners, hipStream_t s);
// NHWC bilinear resize (feature maps).
int launch_resize_bilinear_nhwc(const float* in, int ld_in, int B, int C, int Hi, int Wi, float* out, int ld_out,
                                int Ho, int Wo, int align_corners, hipStream_t s, int max_blocks = 16384);
// out = wa*a + wb*b  (b may be nullptr -> out = wa*a)
int launch_blend(const float* a, float wa, const float* b, float wb, float* out, int64_t numel, hipStream_t s);

// Fused predict_segmentation tail.  SegFuseArgs is what the unweighted fusion kernels take by value; SegTailParams adds what only the
// weighted instantiations read, so the kernel-argument segment of the unweighted ones is the one they always had.
struct SegFuseArgs {
    const float* lo_prev;   // [K, h, w]   decoder logits of the previous key frame
    const float* lo_next;   // [K, h, w]   or nullptr (single-frame)
    const float* const* grids_left;   // n-1 device pointers [Hg,Wg,2] (ignored when no_warp)
    const float* const* grids_right;  // n-1 device pointers
    int K, h, w;            // low-res logits geometry
    int Hg, Wg;             // grid geometry
    int H, W;               // output frame size
    int n;                  // frame_delta
    int no_warp;
    float* out_logits;      // [n, K, H, W] or nullptr
    uint8_t* out_mask;      // [n, H, W] argmax or nullptr
    float* scratch;         // >= 2*(n-1)*K*Hg*Wg floats when warping
    // sliding-crop mode (flow/base.py:204-205, 226-234): canvas[n,K,cH,cW] += softmax_K(frame logits) at (y0, x0), count += 1
    double* canvas;         // float64 [n, K, cH, cW] or nullptr
    double* count;          // float64 [cH, cW]
    int cH, cW, y0, x0;
};
struct SegTailParams : SegFuseArgs {
    const float* weights;   // device [n][2] per-frame blend weights (launch_window_weights), or nullptr: (n-f)/n and f/n
};
int launch_seg_tail(const SegTailParams& p, hipStream_t s);

// Fused predict_feature tail (flow/model.py:131-171): warp chains at grid resolution + every map of the decoder's batch in one launch.
struct FeatTailParams {
    const float* f_prev;    // NHWC [fh][fw][C] encoder features of the previous key frame
    const float* f_next;    // the next key frame's, or nullptr (single frame: stack holds one map)
    const float* const* grids_left;   // n-1 device pointers [Hg,Wg,2] (ignored when no_warp)
    const float* const* grids_right;
    const float* grid0;     // [H0,W0,2] the default (identity) grid the key-frame map is resampled through (warp mode)
    int C, fh, fw, Hg, Wg, H0, W0, n, no_warp;
    float* stack;           // NHWC [n | 1][fh][fw][C]: the decoder's batch
    float* scratch;         // >= 2*(n-1)*Hg*Wg*C floats when warping with two key frames
    const float* weights;   // device [n][2] per-map blend weights (launch_window_weights), or nullptr: (n-p)/n and p/n; read only when
                            // f_next is given and n > 1
};
int launch_feat_tail(const FeatTailParams& p, hipStream_t s);

// Sliding crops in one pass (flow/base.py:182-209 after the network): every pixel of the full frame from the crops covering it.
// CropsFuseArgs / CropsFuseParams: split as SegFuseArgs / SegTailParams are.
struct CropsFuseArgs {
    const float* lo_prev;   // [nc, K, h, w] per-crop decoder logits of the previous key frame
    const float* lo_next;   // the same for the next key frame, or nullptr (single frame)
    const float* scratch;   // warp mode: [nc][2][n-1][K][Hg][Wg] warped maps (filled by the launcher)
    int nc;
    short cy[64], cx[64];   // crop offsets, in the reference's crop order
    int K, h, w, Hg, Wg, ch, cw, n, no_warp;
    double* canvas;         // [n, K, H, W] crop-averaged softmax (already divided by the count) or nullptr
    uint8_t* mask;          // [n, H, W] its argmax or nullptr
    int H, W;
    float sy_lo, sx_lo, sy_g, sx_g;
};
struct CropsFuseParams : CropsFuseArgs {
    const float* weights;   // device [n][2] per-frame blend weights (launch_window_weights), or nullptr: (n-f)/n and f/n
};
// grids: [nc][2(n-1)][Hg][Wg][2] (fs_crop_grids' output) in warp mode; scratch: nc * 2(n-1) * K * Hg * Wg floats
int launch_crops_fuse(CropsFuseParams p, const float* grids, float* scratch, hipStream_t s);

// Single-frame multi-scale test (base/foundation.py:177-221, 264-330), ms_ops.hip.
// (a) raw 0-255 frame [3,H,W] -> out[0] = scaled to new_h x new_w, mean-padded to PH x PW, normalised; out[1] (flip) = its mirror
int launch_ms_prepare(const float* raw, int H, int W, int new_h, int new_w, int PH, int PW, const float* mean, const float* std, float* out,
                      int flip, hipStream_t s);
struct MsFuseParams {
    const float* lo_plain;  // [nc, K, h, w] logits of the crops of the prepared frame
    const float* lo_flip;   // the same crops of the mirrored frame (net_process' input.flip(3) half), or nullptr: flip=False
    int nc;
    short cy[64], cx[64];   // crop offsets in the PADDED scaled frame, in the reference's crop order
    int K, h, w, ch, cw;
    int PH, PW, new_h, new_w;  // padded and un-padded size of the scaled frame
    double* scaled;         // [new_h, new_w, K] crop- and flip-averaged probabilities of the un-padded region
    int pad_top, pad_left;  // filled by the launcher
    float sy_lo, sx_lo;
};
// (b) scaled = fusion of the crops; (c) when pred != nullptr: pred[H,W,K] (+)= resize(scaled), the last scale divides by nscales
// and writes mask[H,W] (may be nullptr).  At most 64 crops: a scale that needs more is refused.
int launch_ms_fuse(MsFuseParams p, double* pred, int H, int W, int scale_index, int nscales, uint8_t* mask, hipStream_t s);

// argmax over channel dim of NCHW logits -> uint8 (first max wins; flow/base.py:276).
int launch_argmax_u8(const float* in, int B, int K, int64_t HW, uint8_t* out, hipStream_t s);
// argmax of the align_corners=True bilinear upsample of NCHW logits, without materialising it
// (flow/base.py:275-276: F.interpolate(output,(1072,1920)) then max(1)[1]).
int launch_resize_argmax_u8(const float* in, int B, int K, int Hi, int Wi, uint8_t* out, int Ho, int Wo,
                            hipStream_t s);
// Sliding-crop accumulation of compute_output / compute_predict_crop (flow/base.py:182-234): softmax over K of one
// crop's logits added into a float64 canvas + per-pixel crop count; finish = divide by the count (+ argmax).
int launch_softmax_accumulate(const float* logits, int n, int K, int h, int w, double* canvas, double* count, int H, int W, int y0,
                              int x0, hipStream_t s);
int launch_canvas_finish(double* canvas, const double* count, int n, int K, int64_t HW, uint8_t* mask, hipStream_t s);
// argmax over K of the align_corners=True bilinear resize (in float64) of the crop-averaged canvas (flow/base.py:275-276)
int launch_resize_crop(const float* in, int B, int K, int Hi, int Wi, int Hfull, int Wfull, int align_corners, float* logits,
                       uint8_t* mask, int Ho, int Wo, hipStream_t s);
int launch_canvas_resize_argmax(const double* canvas, int n, int K, int Hi, int Wi, uint8_t* mask, int Ho, int Wo, hipStream_t s);
// crop_motion_vector (flow/transform.py:215-261) for every crop x every grid of a window in one launch
struct CropGridParams {
    const float* grids[32];  // ngrids device pointers, each [Hg, Wg, 2] fp32
    int ngrids, Hg, Wg;
    int H, W;                // frame size the grids are normalised to
    int ncrops, fh, fw;      // output grids [ncrops][ng_total][fh][fw][2]; this launch fills grids g0 .. g0+ngrids-1 of its crops
    int ng_total, g0;        // (a window with more than 32 grids or crops is cut into several launches by fs_crop_grids)
    short bho[32], bwo[32], bh[32], bw[32];          // block range per crop (Python-rounded on the host)
    float off_h[32], off_w[32], den_h[32], den_w[32];  // pixel offset of the crop; bh * pixels-per-block, bw * pixels-per-block
    float* out;
};
int launch_crop_grids(const CropGridParams& p, hipStream_t s);
// rgb[i] = palette[mask[i]] (flow/base.py:308-312)
int launch_colorize(const uint8_t* mask, const uint8_t* palette, int K, uint8_t* rgb, int64_t numel, hipStream_t s);
// H.264 block motion vectors -> forward / inverse sampling grids (dataset/flow/extract_motion_vectors.py:21-43), float64
int launch_mv_to_grids(const int* mv, int n, int stride, int hb, int wb, int bs, int H, int W, int* owners, double* grid,
                       double* inv_grid, hipStream_t s);
// Full-search block matching of two uint8 frames (luma [H][W], channels = 1, or RGB [H][W][3], channels = 3; ref = the past frame):
// for every 16x16 block of `cur` the displacement |dx|, |dy| <= R whose window lies inside `ref` and minimises
// (SAD + lambda (|dx| + |dy|), |dx| + |dy|, dy, dx); mv = int32 [H/16 * W/16][7] rows (-1, 16, 16, src_x, src_y, dst_x, dst_y) in
// block raster order (the table launch_mv_to_grids takes), cost = int32 [H/16 * W/16] winning costs or nullptr (motion_ops.hip)
int launch_block_match(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int R, int lambda, int* mv, int* cost,
                       hipStream_t s);
// The same search with the inter / intra decision per block and the scene-cut decision per pair (include/floodseg_test.h,
// block_match_modes): intra rows -- on a cut all rows -- are void rows (-1, 16, 16, -16, -16, -16, -16); activity = int32 [H/16 * W/16]
// or nullptr, stats = int32 [4] {blocks, intra blocks, cut, 0} or nullptr, written by the call.  Two launches (search, finishing pass).
int launch_block_match_modes(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int R, int lambda, int intra_bias, int cut_permille,
                             int* mv, int* cost, int* activity, int* stats, hipStream_t s);
// Per-frame blend weights of one window from the cut flags of its n frame pairs (include/floodseg_test.h, window_weights):
// stats[j-1] = the int32 [4] stats of pair (j-1 -> j) as launch_block_match_modes writes them (cut at index 2), or nullptr = no cut;
// weights = float [n][2], source = int32 [n], written whole by ONE launch of one workgroup.  1 <= n <= WINDOW_MAX_FRAMES (caller).
constexpr int WINDOW_MAX_FRAMES = 64;
int launch_window_weights(const int* const* stats, int n, float* weights, int* source, hipStream_t s);
// The matcher's tables guided by global_motion's camera model (motion_ops.hip, guide_defs.h; definition: include/floodseg_test.h,
// guide_vectors): mv, out = int32 [n][FH/16 * FW/16][7] (out may be mv), model = int64 [n][16], counts = int64 [n][8]; cur, ref
// (uint8 [n][FH][FW][channels]) and cost (int32 [n][blocks]) all given = evidence mode, all nullptr = table only.  The launcher refuses
// bad arguments before it launches anything.  Two launches (counts cleared, the pass); nothing is allocated, synchronised or read on
// the host.
int launch_guide_vectors(const int32_t* mv, const long long* model, int n, int FH, int FW, int fill_void, long long outlier_q20, const uint8_t* cur,
                         const uint8_t* ref, int channels, const int32_t* cost, int penalty, int guide_bias, int32_t* out, long long* counts, hipStream_t s);
// Frame ingest (ingest_ops.hip): one decoded uint8 frame -> normalised NCHW fp32 [3][h][w].  format 0: RGB24 [H][W][3] in `frame`;
// 1: NV12, `frame` = Y [H][W], u = interleaved UV [ceil(H/2)][ceil(W/2)][2] (v unused); 2: I420, u and v = [ceil(H/2)][ceil(W/2)] each.
// matrix 0 / 1 (BT.601 / BT.709) and full_range 0 / 1 pick the integer conversion of include/floodseg_test.h.  mean, std: 3 device
// floats each.  Arguments are validated by the caller (api_test.hip).
int launch_frame_prepare(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int H, int W,
                         const float* mean, const float* std, float* out, int h, int w, hipStream_t s);
// Frame egress (egress_ops.hip): mask uint8 [h][w] + palette uint8 [K][4] (R, G, B, A) (+ a decoded background frame, described as
// launch_frame_prepare's input; frame == nullptr: none) -> one RGB24 / NV12 / I420 frame (out_format 0 / 1 / 2; out = the interleaved
// frame or the Y plane, out_u = the UV plane or the U plane, out_v = the V plane); out_matrix / out_full_range pick the integer
// RGB -> YUV conversion of include/floodseg_test.h.  Arguments are validated by the caller (api_test.hip).
int launch_frame_compose(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                         int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                         int out_matrix, int out_full_range, hipStream_t s);
// Region overlay (overlay_ops.hip; include/floodseg_test.h, frame_compose_regions): launch_frame_compose's arguments and picture, plus
// the fill-by-id, outline and id-label layers drawn from region_table's index plane / table / counts and region_tracks' rows.  workspace:
// the marks plane, FS_FRAME_COMPOSE_REGIONS_WORKSPACE_BYTES(h, w) bytes (labels only).  Arguments are validated by the caller.
int launch_frame_compose_regions(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                                 int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                                 int out_matrix, int out_full_range, const int32_t* index, const long long* table, const long long* counts,
                                 const long long* tracks, int max_regions, const uint8_t* fill_palette, int P, const uint8_t* outline, int outline_width,
                                 int label_scale, long long label_min_area, uint32_t halo_rgba, uint32_t ink_rgb, void* workspace, hipStream_t s);
// intersection / union / target histograms (util/util.py:52-63), int64[3][K] accumulated.
int launch_iou_hist(const uint8_t* pred, const uint8_t* target, int64_t numel, int K, int ignore_index,
                    long long* hist3K, hipStream_t s);
// Per-pixel confidence and the per-frame extent report (conf_ops.hip; definitions: include/floodseg_test.h).  Each launcher refuses
// null pointers, sizes < 1, K out of range (1..32 for logits, 1..255 otherwise) and planes of 2^31 elements before any launch.
// mask / conf: uint8 [n][H][W] at any byte address.
int launch_mask_confidence(const float* logits, int n, int K, int h, int w, uint8_t* mask, uint8_t* conf, int H, int W, hipStream_t s);
int launch_canvas_confidence(const double* canvas, int n, int K, int Hi, int Wi, uint8_t* mask, uint8_t* conf, int Ho, int Wo, hipStream_t s);
// out: int64 [n][K][3] = (pixels, sum of confidence codes, pixels with code < low), written whole; conf == nullptr: counts only
int launch_frame_report(const uint8_t* mask, const uint8_t* conf, int n, int H, int W, int K, int low, long long* out, hipStream_t s);

// Connected regions of a mask (region_ops.hip, region_uf.h; definitions: include/floodseg_test.h).  Each launcher refuses bad arguments
// before it launches anything; workspaces are the caller's (sizes in the header), nothing is allocated or synchronised.
int region_rank_chunks(int H, int W);  // ints of region_table's workspace per frame
int launch_mask_regions(const uint8_t* mask, int n, int H, int W, int K, int connectivity, int* labels, hipStream_t s);
int launch_region_table(const uint8_t* mask, const int* labels, const uint8_t* conf, int n, int H, int W, int K, int low, int max_regions,
                        long long* table, long long* counts, int* index, int* workspace, hipStream_t s);
int launch_region_filter(const uint8_t* mask, const int* index, const long long* table, int n, int H, int W, int K, int max_regions,
                         int min_area, uint8_t* out, int* votes, hipStream_t s);

// Region identity across frames (track_ops.hip, track_defs.h; definitions: include/floodseg_test.h).  The launchers refuse bad arguments
// before they launch anything; the workspace is the caller's (FS_REGION_LINKS_WORKSPACE_BYTES), nothing is allocated or synchronised.
int launch_region_links(const int* index, const long long* table, const long long* counts, const int* prev_index, const long long* prev_table,
                        const long long* prev_counts, int n, int H, int W, int max_regions, int max_pairs, int min_overlap, int* back, int* fwd,
                        long long* link_counts, void* workspace, hipStream_t s);
// mv: int32 [n][(frame_h / 16) * (frame_w / 16)][7], pair_stats: int32 [n][4] or nullptr; workspace: FS_REGION_LINKS_MC_WORKSPACE_BYTES
int launch_region_links_mc(const int* index, const long long* table, const long long* counts, const int* prev_index, const long long* prev_table,
                           const long long* prev_counts, const int* mv, const int* pair_stats, int n, int H, int W, int frame_h, int frame_w,
                           int max_regions, int max_pairs, int min_overlap, int* back, int* fwd, long long* link_counts, void* workspace, hipStream_t s);
int launch_region_tracks(const int* back, const int* fwd, const long long* counts, const long long* prev_tracks, int n, int max_regions,
                         long long* state, long long* tracks, hipStream_t s);

// Temporal mask stabiliser (stabilize_ops.hip, stabilize_defs.h; definition: include/floodseg_test.h, mask_stabilize).  The launcher
// refuses bad arguments before it launches anything.  conf, mv, pair_stats and (without mv) workspace may be nullptr; has_state 0: the
// state plane is written only.  workspace: FS_MASK_STABILIZE_WORKSPACE_BYTES with mv.
int launch_mask_stabilize(const uint8_t* mask, const uint8_t* conf, const int* mv, const int* pair_stats, int n, int H, int W, int frame_h, int frame_w,
                          int K, int persist, int trust, int has_state, uint32_t* state, uint8_t* out, long long* counts, void* workspace, hipStream_t s);

// Distance to a class (distance_ops.hip, distance_defs.h; definitions: include/floodseg_test.h, mask_distance and region_proximity).  The
// launchers refuse bad arguments before they launch anything.  nearest may be nullptr in both; workspace: FS_MASK_DISTANCE_WORKSPACE_BYTES,
// the caller's; thresholds: B ints in HOST memory.  Nothing is allocated or synchronised.
int launch_mask_distance(const uint8_t* mask, int n, int H, int W, uint32_t source_set, int max_dist, uint32_t* d2, int32_t* nearest, void* workspace,
                         hipStream_t s);
int launch_region_proximity(const uint8_t* mask, const uint32_t* d2, const int32_t* nearest, const int32_t* index, const long long* counts, int n, int H,
                            int W, int K, int max_regions, uint32_t target_set, const int32_t* thresholds, int B, long long* exposure, long long* near,
                            hipStream_t s);

// The flood-extent mosaic (mosaic_ops.hip, mosaic_defs.h; definitions: include/floodseg_test.h, global_motion, pose_chain,
// mosaic_accumulate and mosaic_resolve).  The launchers refuse bad arguments before they launch anything.  pair_stats and mask may be
// nullptr in launch_global_motion.  No workspace; nothing is allocated, synchronised or read on the host.
int launch_global_motion(const int32_t* tables, const int32_t* pair_stats, const uint8_t* mask, uint32_t exclude_set, int n, int FH, int FW, int H, int W,
                         int rounds, long long tol_q20, int min_inliers, long long* model, hipStream_t s);
int launch_pose_chain(const long long* model, long long* state, long long* poses, int n, int H, int W, int CH, int CW, int ox, int oy, int max_bridge,
                      hipStream_t s);
int launch_mosaic_accumulate(const uint8_t* mask, const long long* poses, int n, int H, int W, int K, int CH, int CW, int ox, int oy, uint16_t* votes,
                             hipStream_t s);
int launch_mosaic_resolve(const uint16_t* votes, int K, int CH, int CW, uint8_t* cls, uint8_t* conf, uint32_t* seen, long long* totals, hipStream_t s);

// The orthophoto under the mosaic (ortho_ops.hip, ortho_defs.h; definitions: include/floodseg_test.h, ortho_accumulate and
// ortho_compose).  The launchers refuse bad arguments before they launch anything.  u and v as frame_prepare takes them; cls may be
// nullptr in launch_ortho_compose (the plain orthophoto).  No workspace; nothing is allocated, synchronised or read on the host.
int launch_ortho_accumulate(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW,
                            const long long* pose, uint32_t ordinal, int H, int W, int mode, int CH, int CW, int ox, int oy, unsigned long long* rank,
                            uint32_t* rgba, hipStream_t s);
int launch_ortho_compose(const uint32_t* rgba, const uint8_t* cls, const uint8_t* palette, int K, uint32_t edge_set, uint32_t fill, int CH, int CW,
                         uint8_t* out, hipStream_t s);

// Frame-to-map registration (refine_ops.hip, refine_defs.h; definitions: include/floodseg_test.h, map_view, map_gate and pose_correct).
// The launchers refuse bad arguments before they launch anything.  The frame arguments as launch_ortho_accumulate takes them; table is
// the matcher's, `blocks` rows of seven ints, gated in place.  No workspace; nothing is allocated, synchronised or read on the host.
int launch_map_view(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const long long* pose,
                    uint32_t ordinal, int H, int W, int CH, int CW, int ox, int oy, const unsigned long long* rank, const uint32_t* rgba, int min_age,
                    uint8_t* cur, uint8_t* view, uint8_t* valid, hipStream_t s);
int launch_map_gate(int32_t* table, int blocks, const uint8_t* valid, int H, int W, hipStream_t s);
// the one gate launch, UNCHECKED: behind launch_map_gate (own == nullptr) and launch_merge_gate (own = valid_a), which check the arguments
int launch_gate_rows(int32_t* table, int blocks, const uint8_t* own, const uint8_t* valid, int H, int W, hipStream_t s);
int launch_pose_correct(const long long* model, long long* state, long long* pose, int H, int W, int CH, int CW, int ox, int oy, long long* out, hipStream_t s);

// Relocalisation of a lost pose chain against the orthophoto (relocate_ops.hip, relocate_defs.h; definitions: include/floodseg_test.h,
// map_coarse, map_patch, map_locate, pose_relocate and relocate_commit).  The launchers refuse bad arguments before they launch
// anything.  cl, cv = uint8 [CH / S][CW / S]; tl, tv = uint8 [65536], the first tw th bytes written as [th][tw]; geom = int64 [8];
// scores = uint32 [ch][cw][2], the caller's workspace; found = int64 [16]; the frame arguments as launch_map_view takes them.  Nothing is
// allocated, synchronised or read on the host.
int launch_map_coarse(const uint32_t* rgba, int CH, int CW, int S, uint8_t* cl, uint8_t* cv, hipStream_t s);
int launch_map_patch(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const long long* state, int H,
                     int W, int CH, int CW, int ox, int oy, int S, uint8_t* tl, uint8_t* tv, long long* geom, hipStream_t s);
int launch_map_locate(const uint8_t* cl, const uint8_t* cv, int ch, int cw, const uint8_t* tl, const uint8_t* tv, const long long* geom, int min_overlap_permille,
                      int exclude, uint32_t* scores, long long* found, hipStream_t s);
int launch_pose_relocate(const long long* found, const long long* state, long long* cand_state, long long* cand_pose, int max_mean, int ratio_permille, int H, int W,
                         int CH, int CW, int ox, int oy, int S, hipStream_t s);
int launch_relocate_commit(const long long* cand_state, const long long* cand_pose, const long long* correct_out, long long* state, long long* pose,
                           const long long* found, int S, long long* out, hipStream_t s);

// Map-to-map registration and the merge of two mosaics (merge_ops.hip, merge_defs.h; definitions: include/floodseg_test.h, merge_view,
// merge_gate, link_correct, mosaic_merge, merge_patch and link_place).  The launchers refuse bad arguments before they launch anything.  link = int64 [16];
// cur, view, valid_a, valid_b = uint8 [WH][WW]; out, counts = int64 [8]; rank and rgba of mosaic_merge all four or all null.  Nothing is
// allocated, synchronised or read on the host.
int launch_merge_view(const uint32_t* rgba_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b,
                      const long long* link, int Y0, int X0, int WH, int WW, uint8_t* cur, uint8_t* view, uint8_t* valid_a, uint8_t* valid_b, hipStream_t s);
int launch_merge_gate(int32_t* table, int blocks, const uint8_t* valid_a, const uint8_t* valid_b, int H, int W, hipStream_t s);
int launch_link_correct(const long long* model, long long* link, int Y0, int X0, int WH, int WW, int ox_a, int oy_a, long long* out, hipStream_t s);
int launch_mosaic_merge(uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                        const long long* link, unsigned long long* rank_a, uint32_t* rgba_a, const unsigned long long* rank_b, const uint32_t* rgba_b,
                        uint32_t ordinal_offset, int mode, long long* counts, hipStream_t s);
// tl, tv, geom as launch_map_patch writes them and launch_map_locate reads them; found = map_locate's; cand = int64 [16]
int launch_merge_patch(const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b, const long long* link, int CH_a, int CW_a, int ox_a, int oy_a, int S, int y0,
                       int x0, int y1, int x1, uint8_t* tl, uint8_t* tv, long long* geom, hipStream_t s);
int launch_link_place(const long long* found, const long long* link, int S, int max_mean, int ratio_permille, long long* cand, long long* out, hipStream_t s);

// The flood-extent change between two registered mosaics (change_ops.hip, change_defs.h; definition: include/floodseg_test.h,
// mosaic_change).  The launcher refuses bad arguments before it launches anything.  votes as launch_mosaic_merge takes
// them, both only read; change, cls_a, cls_b = uint8 [CH_a][CW_a]; transitions = int64 [2][K][K]; counts = int64 [8].  No workspace;
// nothing is allocated, synchronised or read on the host.
int launch_mosaic_change(const uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                         const long long* link, int min_votes, int min_conf, int tolerance, uint32_t watch_set, uint8_t* change, uint8_t* cls_a, uint8_t* cls_b,
                         long long* transitions, long long* counts, hipStream_t s);

// Dry-route reachability (access_ops.hip, access_defs.h; definitions: include/floodseg_test.h, mask_access and region_access; DESIGN
// §3.25).  The launchers refuse bad arguments before they launch anything.  mask, seeds = uint8 [n][H][W]; cost = uint8 [32] in HOST
// memory, read during the call; d = uint32 and origin = int32 (or null) [n][H][W]; status = int32 [n][4]; the workspace is the caller's
// (FS_MASK_ACCESS_WORKSPACE_BYTES, 8-byte aligned).  2 + rounds launches; nothing is allocated, synchronised or read back on the host.
int launch_mask_access(const uint8_t* mask, const uint8_t* seeds, int n, int H, int W, const uint8_t* cost, uint32_t terminal_set, int connectivity,
                       uint32_t max_cost, int rounds, int resume, uint32_t* d, int32_t* origin, int32_t* status, void* workspace, hipStream_t s);
// index, counts = region_table's; reach = int64 [n][K][4]; rows = int64 [n][max_regions][8].  Three launches, no workspace.
int launch_region_access(const uint8_t* mask, const uint32_t* d, const int32_t* origin, const int32_t* index, const long long* counts, int n, int H, int W,
                         int K, int max_regions, long long* reach, long long* rows, hipStream_t s);

// Georeferencing the mosaic (ground_ops.hip, ground_defs.h; definitions: include/floodseg_test.h, ground_area, ground_rectify and
// ground_points).  The launchers refuse bad arguments, the models' bounds among them, before they launch anything.  forward,
// inverse = nine doubles in HOST memory, read during the call; planes, outs = HOST arrays of device pointers.  Nothing is allocated,
// synchronised or read back on the host.  ground_area: two launches; the other two: one.
int launch_ground_area(const uint8_t* cls, int CH, int CW, int ox, int oy, const double* forward, int K, const int32_t* index, int max_regions,
                       long long* class_area2, long long* region_area2, long long* counts, hipStream_t s);
int launch_ground_rectify(const double* inverse, int CH, int CW, int ox, int oy, int GH, int GW, int gsd_mm, long long e0_mm, long long ntop_mm, int nplanes,
                          const uint8_t* const* planes, uint8_t* const* outs, const uint32_t* rgba, uint8_t* rgb_out, int fill, uint32_t rgb_fill, hipStream_t s);
int launch_ground_points(const int32_t* points, int n, const double* forward, int ox, int oy, long long* out, hipStream_t s);

// Region outlines (outline_ops.hip, outline_defs.h; definitions: include/floodseg_test.h).  The launcher refuses bad arguments before it
// launches anything; the workspace is the caller's (FS_REGION_OUTLINES_WORKSPACE_BYTES), nothing is allocated or synchronised.
int launch_region_outlines(const int* index, int n, int H, int W, int max_regions, int connectivity, int max_contours, int max_vertices,
                           long long* contours, int* vertices, long long* shape, long long* counts, void* workspace, hipStream_t s);

// Outline simplification (simplify_ops.hip, simplify_defs.h; definitions: include/floodseg_test.h).  The launcher refuses bad arguments
// before it launches anything; the workspace is the caller's (FS_OUTLINE_SIMPLIFY_WORKSPACE_BYTES), nothing is allocated or synchronised.
int launch_outline_simplify(const long long* contours, const int* vertices, const long long* counts, int n, int max_contours, int max_vertices, int tol_q,
                            int max_rounds, long long* simple, int* simple_vertices, long long* simple_counts, void* workspace, hipStream_t s);

// ---------------------------------------------------------------------------------
// Segmenter / ViT pieces (segm/model/vit.py, blocks.py, decoder.py); token matrices are row-major
// [rows][D] -- i.e. the same "NHWC with ld" layout, so every nn.Linear runs on conv_igemm_f32.
// ---------------------------------------------------------------------------------
// Zero-padded (right/bottom) im2col of non-overlapping PxP patches: NCHW frame -> [B*gh*gw][3*P*P],
// column order (c, py, px) = Conv2d(k=s=P) weight flattening (segm/model/vit.py:28-35, utils.py:65-76).
// in: images 0 .. B1-1, in2: images B1 .. B-1 (nullptr when B1 == B), as in StemParams
int launch_patchify(const float* in, const float* in2, int B1, float* out, int B, int H, int W, int P, int gh, int gw, hipStream_t s);
// X[b][0] = cls + pos[0];  X[b][1+i] = emb[b*N+i] + pos[1+i]   (segm/model/vit.py:112-131)
int launch_vit_assemble(const float* emb, const float* cls, const float* pos, float* X, int B, int N, int D, hipStream_t s);
// Z[b][i<N] = Y[b*N+i];  Z[b][N+k] = cls_emb[k]                (segm/model/decoder.py:84-86)
int launch_dec_assemble(const float* Y, const float* cls_emb, float* Z, int B, int N, int K, int D, hipStream_t s);
// nn.LayerNorm(D) per row; drop_first > 0: input rows are [B][rows_per_batch] and row 0 of every batch
// (the cls token) is skipped in the output (segm/model/segmenter.py:41-42).
int launch_layernorm(const float* in, const float* gamma, const float* beta, float* out, int rows, int D, int rows_per_batch,
                     int drop_first, hipStream_t s);
// softmax(q k^T * scale) v for all heads, fp32 MFMA flash-style; qkv rows are [3][heads][64] (blocks.py:56-77), qkv 16-B aligned and
// one image's qkv smaller than 2 GiB.  scratch: attention_scratch_floats(B, N, heads) floats for the key-split partials (nullptr = single pass)
size_t attention_scratch_floats(int B, int N, int heads);
int launch_attention_f32(const float* qkv, float* out, int B, int N, int heads, float scale, float* scratch, hipStream_t s);
// the same on the bf16 matrix cores with split operands (three bf16 terms per fp32 value, fp32 accumulate: vit_ops.hip);
// planes: attention_split_floats(B, N, heads) floats of workspace for the K / V^T planes
size_t attention_split_floats(int B, int N, int heads);
int launch_attention_split(const float* qkv, float* out, int B, int N, int heads, float scale, float* scratch, float* planes, hipStream_t s, bool planes_ready = false);
// masks[b][k][i] = LayerNorm_K( <pp[b][i]/|pp|, cc[b][N+k]/|cc|> )  (segm/model/decoder.py:90-100), NCHW out
// out[r][c] = sum_s part[s][r][c] + bias[c] (+ res[r][c]): merges the split-K partial products of a Linear
int launch_splitk_combine(const float* part, int nsplit, const float* bias, const float* res, float* out, int rows, int N, hipStream_t s);
// the same merge + nn.LayerNorm(N) of the merged rows into ln_out, one pass (fc2 of block i feeding norm1 of block i + 1)
int launch_splitk_combine_ln(const float* part, int nsplit, const float* bias, const float* res, float* out, const float* gamma, const float* beta,
                             float* ln_out, int rows, int N, hipStream_t s);
int launch_mask_head(const float* pp, const float* cc, const float* gamma, const float* beta, float* out, int B, int N, int K,
                     int D, hipStream_t s);


// ---------------------------------------------------------------------------------
// Winograd F(m x m, 3x3), m = 4 or 6, for stride-1 3x3 convolutions with pad == dil and many input channels (the PSPNet
// head conv and the dilated bottleneck conv2 layers).  (m+2)^2 GEMMs [tiles x Cin] x [Cin x Cout] on the fp32 MFMA
// kernel replace the direct conv: 2.25 (m = 4) or 1.78 (m = 6) multiplies per output instead of 9; fp32 error ~1e-5
// relative (m = 4) / ~1.5e-5 (m = 6), direct 3e-7.
//   V[xi][t][c]  = (B^T d B)[xi]      input transform,  xi in 0..(m+2)^2-1, t = (b, phase, ty, tx) m x m-output tiles
//   M[xi][t][o]  = sum_c V[xi][t][c] * U[xi][o][c]      (grouped conv_igemm_dma_f32)
//   out          = act(scale * (A^T M A) + shift)       output transform
// ---------------------------------------------------------------------------------
// chunk_major != 0: `w` is the direct kernel's packed bank [O][I/32][3][3][32] (ConvParams::korder == 1) instead of OIHW
int launch_winograd_filter(const float* w, float* U /*[(m+2)^2][O][I]*/, int O, int I, int mt, hipStream_t s, int chunk_major = 0);
// dil > 1 (pad == dil): the conv is d*d independent undilated convs on the pixel lattices (py + d*i, px + d*j);
// tiles are enumerated (b, py, px, ty, tx).
int launch_winograd_input(const float* in, int ld_in, float* V /*[(m+2)^2][T][C]*/, int B, int H, int W, int C, int dil, int mt,
                          hipStream_t s);
int launch_winograd_output(const float* M /*[(m+2)^2][T][N]*/, const float* scale, const float* shift, float* out, int ld_out, int B,
                           int H, int W, int N, int relu, int dil, int mt, hipStream_t s);
// element (position xi, tile t, channel c) of V (C = Cin) / M (C = Cout) lives at xi * s_pos + t * s_tile + c
struct WinoLayout { bool tile_major; long long s_pos, s_tile; };
WinoLayout winograd_layout(int mt, long long T, int C);
// the grouped GEMM between the transforms: group g = position g multiplies V's T tile rows with U + g * Cout * Cin into M; V / M are
// tile-major when that fits a buffer descriptor (winograd.hip)
static inline ConvParams winograd_gemm_params(const float* V, const float* U, float* M, int mt, int T, int Cin, int Cout) {
    ConvParams p = gemm_params(V, Cin, U, M, Cout, T, Cin, Cout);
    const WinoLayout a = winograd_layout(mt, T, Cin), o = winograd_layout(mt, T, Cout);
    p.ld_in = (int)a.s_tile;
    p.g_in = a.s_pos;
    p.ld_out = (int)o.s_tile;
    p.g_out = o.s_pos;
    p.groups = (mt + 2) * (mt + 2);
    p.g_wgt = (long long)Cout * Cin;
    return p;
}
// floats of V [(m+2)^2][T][Cin], rounded up to a multiple of `align`, and of V followed by M [(m+2)^2][T][Cout]
static inline size_t wino_v_floats(int mt, size_t T, int Cin, size_t align) { return ((size_t)(mt + 2) * (mt + 2) * T * Cin + align - 1) / align * align; }
static inline size_t wino_vm_floats(int mt, size_t T, int Cin, int Cout, size_t align) {
    return wino_v_floats(mt, T, Cin, align) + (size_t)(mt + 2) * (mt + 2) * T * Cout;
}
static inline int winograd_tiles(int B, int H, int W, int dil, int mt) {
    return B * dil * dil * ((cdiv(H, dil) + mt - 1) / mt) * ((cdiv(W, dil) + mt - 1) / mt);
}
// GEMM rows the grouped launch really multiplies: (m+2)^2 groups x tiles rounded up to the 64-row tile
static inline double winograd_gemm_rows(int B, int H, int W, int dil, int mt) {
    return (double)(mt + 2) * (mt + 2) * (double)(cdiv(winograd_tiles(B, H, W, dil, mt), 64) * 64);
}
// the cheaper tile size for this map (a 90x90 map is 15x15 tiles of 6x6 exactly, but 23x23 of 4x4).  Decided on the
// geometry of ONE image, so that a frame's result does not depend on the batch it is processed in.
// Round 6: F(3,3) joins where BOTH larger forms are mostly empty tiles (lattices of <= 3 pixels: ASPP's dilation 36 on a 90x90 map).
static inline int winograd_pick_m(int /*B*/, int H, int W, int dil) {
    const int m = winograd_gemm_rows(1, H, W, dil, 6) < winograd_gemm_rows(1, H, W, dil, 4) ? 6 : 4;
    return winograd_gemm_rows(1, H, W, dil, 3) < winograd_gemm_rows(1, H, W, dil, m) ? 3 : m;
}
// the tile size a conv runs with: a forced one (3, 4 or 6) or the map's own
static inline int wino_m(int force, int H, int W, int dil) { return force ? force : winograd_pick_m(1, H, W, dil); }

// ---------------------------------------------------------------------------------
// Fused Winograd F(4x4,3x3) for 3x3 stride-1 pad-1 convs with few input channels (wino_fused.hip): input transform, the 36
// position GEMMs and the output transform (+BN, ReLU) in ONE kernel -- only the input and output maps touch HBM.
// U: packed bank [36][Cin/16][Cout][16] from launch_wino4_filter_packed (w: OIHW, or the chunk-major bank when chunk_major).
// ---------------------------------------------------------------------------------
size_t wino_fused_bank_floats(int Cin, int Cout);
bool wino_fused_supported(int Cin, int Cout, int KH, int KW, int stride, int pad, int dil);
int launch_wino4_filter_packed(const float* w, float* U, int O, int I, hipStream_t s, int chunk_major = 0);
// variant: 0 = by workgroup count, 2 = 16 tiles x 64 channels per workgroup (4 waves, two
// workgroups per CU), 3 = 16 x 64 warp-specialised (4 MFMA waves + 4 transform waves); bit-identical results.  1 (retired) is refused.
int launch_wino4_fused(const float* in, int ld_in, const float* U, const float* scale, const float* shift, float* out, int ld_out, int B, int H,
                       int W, int Cin, int Cout, int relu, hipStream_t s, int variant = 0);

// Round 5: the same conv + BatchNorm + ReLU with MaxPool2d(3, stride 2, padding 1) fused into the epilogue (model/resnet.py:114-117:
// layer0.6 -> layer0.8 -> maxpool): pool = [B][(H-1)/2+1][(W-1)/2+1][ld_pool], zeroed by the launcher; the full-resolution map is
// never written.  Bit-identical to launch_wino4_fused followed by launch_maxpool3x3s2.
int launch_wino4_fused_pool(const float* in, int ld_in, const float* U, const float* scale, const float* shift, float* pool, int ld_pool, int B,
                            int H, int W, int Cin, int Cout, hipStream_t s);

}  // namespace fs
