// Single-frame multi-scale, flip-averaged sliding-crop test (base/foundation.py:177-221 test_step, :264-295
// compute_test_output_for_scales, :299-330 net_process) around the network: the frame preparation of one scale in front of
// fs_segment_crops, and behind it the crop / flip fusion of that scale and its accumulation into the frame's prediction.
// Nothing per crop reaches the host (the reference copies every crop's probabilities there: :328).
//
// The two interpolating cv2.resize calls (:200 the raw frame, :294 the float64 probabilities) are restated as half-pixel
// bilinear interpolation: source coordinate (i + 0.5) * src / dst - 0.5 evaluated in double, the two taps floor / floor + 1
// clamped to the image, horizontal pass first, then vertical.  When dst == src the coordinate is the integer i itself and the
// weights are exactly 0 / 1: the resize is the identity bit for bit (cv2 returns a copy there).
#include "common.h"
#include "interp.h"
#include "kernels.h"

#include <algorithm>

namespace fs {

struct HalfPix {
    int i0, i1;
    double w1;  // weight of tap i1; tap i0 takes 1 - w1
};

// destination index -> the two clamped source taps and the weight of the second
__device__ __forceinline__ HalfPix half_pix(int dst, int in_size, double scale) {
    const double src = ((double)dst + 0.5) * scale - 0.5;
    const double fl = floor(src);
    int i0 = (int)fl;
    double w1 = src - fl;
    if (i0 < 0) { i0 = 0; w1 = 0.0; }
    if (i0 >= in_size - 1) { i0 = in_size - 1; w1 = 0.0; }
    HalfPix c;
    c.i0 = i0;
    c.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    c.w1 = w1;
    return c;
}

// the same taps with fp32 weights, as bilerp takes them
__device__ __forceinline__ LinCoord lin_from_half(const HalfPix& h) {
    LinCoord c;
    c.i0 = h.i0;
    c.i1 = h.i1;
    c.w1 = (float)h.w1;
    c.w0 = __fadd_rn(1.f, -c.w1);
    return c;
}

// ------------------------------------------------------------------ (a) frame preparation, one launch per scale
// out[0] = the scaled (:200), mean-padded (:272-273), normalised (:300-306) frame [3][PH][PW]; out[1] (flip) = its horizontal
// mirror.  A padding pixel holds `mean`, so its normalised value (mean - mean) / std is exactly 0.  Each thread owns one column
// of MS_ROWS rows: the column's taps and weights are computed once; the taps are loaded from clamped addresses whether or not
// the pixel is padding and the result is zeroed afterwards.
constexpr int MS_ROWS = 4;

__global__ __launch_bounds__(256) void ms_prepare_kernel(const float* __restrict__ raw, int H, int W, int new_h, int new_w, int PH, int PW,
                                                         int pad_top, int pad_left, double sy, double sx, float m0, float m1, float m2,
                                                         float s0, float s1, float s2, float* __restrict__ out, int flip) {
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= PW) return;
    const int x = min(max(X - pad_left, 0), new_w - 1);
    const bool x_in = X >= pad_left && X < pad_left + new_w;
    const LinCoord cx = lin_from_half(half_pix(x, W, sx));
    const size_t plane_in = (size_t)H * W, plane_out = (size_t)PH * PW;
    const float mean[3] = {m0, m1, m2}, std[3] = {s0, s1, s2};
    for (int r = 0; r < MS_ROWS; ++r) {
        const int Y = blockIdx.y * MS_ROWS + r;
        if (Y >= PH) break;
        const int y = min(max(Y - pad_top, 0), new_h - 1);
        const bool inside = x_in && Y >= pad_top && Y < pad_top + new_h;
        const LinCoord cy = lin_from_half(half_pix(y, H, sy));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = bilerp_at(raw + c * plane_in, (size_t)W, cy, cx);
            float o = __fdiv_rn(__fadd_rn(v, -mean[c]), std[c]);  // t.sub_(m).div_(s), :305-306
            if (!inside) o = 0.f;
            out[c * plane_out + (size_t)Y * PW + X] = o;
            if (flip) out[(3 + c) * plane_out + (size_t)Y * PW + (PW - 1 - X)] = o;
        }
    }
}

int launch_ms_prepare(const float* raw, int H, int W, int new_h, int new_w, int PH, int PW, const float* mean, const float* std, float* out,
                      int flip, hipStream_t s) {
    FS_REQUIRE(H >= 1 && W >= 1 && new_h >= 1 && new_w >= 1 && H <= 32767 && W <= 32767 && PH <= 32767 && PW <= 32767,
               "ms_prepare: frame sizes must lie in 1..32767");
    FS_REQUIRE(PH >= new_h && PW >= new_w, "ms_prepare: the padded frame %dx%d is smaller than the scaled frame %dx%d", PH, PW, new_h, new_w);
    for (int c = 0; c < 3; ++c) FS_REQUIRE(std[c] > 0.f, "ms_prepare: std[%d] must be positive", c);
    const int pad_top = (PH - new_h) / 2, pad_left = (PW - new_w) / 2;  // int(pad / 2), :269-270
    hipLaunchKernelGGL(ms_prepare_kernel, dim3((unsigned)cdiv(PW, 256), (unsigned)cdiv(PH, MS_ROWS)), dim3(256), 0, s, raw, H, W, new_h, new_w,
                       PH, PW, pad_top, pad_left, (double)H / (double)new_h, (double)W / (double)new_w, mean[0], mean[1], mean[2], std[0], std[1],
                       std[2], out, flip);
    FS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ (b) crop and flip fusion of one scale
// Every pixel of the un-padded region of the scaled frame is written once from the crops that cover it, in the reference's crop
// order (:281-291; the float64 sums depend on it).  Per covering crop: net_process' align_corners=True upsample (:322, the
// operation order of crops_fuse_kernel / resize_bilinear_nchw: bilerp_at) and fp32 softmax over K (:323: softmax_k) of the crop's
// logits; with lo_flip the same for the flipped crop's logits at the mirrored column
// cw - 1 - x (output[1].flip(2)) and (a + b) / 2 in fp32 (:325).  Summed in float64 (:279, :291), divided by the float64 crop
// count (:292); the padding is never computed (:293).  scaled: [new_h][new_w][K] float64, pixel-major, which is what (c) reads:
// its four taps are four runs of K contiguous doubles.
template <int KMAX>
__device__ __forceinline__ void ms_crop_softmax(const float* __restrict__ lo, int K, int h, int w, const LinCoord& cy, const LinCoord& cx,
                                                float (&p)[KMAX]) {
    const int plane = h * w;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) p[k] = bilerp_at(lo + (size_t)k * plane, w, cy, cx);
    softmax_k<KMAX>(p, K, [&](int k, float q) { p[k] = q; });
}

template <int KMAX>
__global__ __launch_bounds__(256) void ms_fuse_crops_kernel(MsFuseParams p) {
    const int x_un = blockIdx.x * 256 + threadIdx.x;
    if (x_un >= p.new_w) return;
    const int K = p.K;
    const size_t lo_stride = (size_t)K * p.h * p.w;
    const int X = x_un + p.pad_left;
    for (int y_un = blockIdx.y; y_un < p.new_h; y_un += gridDim.y) {
        const int Y = y_un + p.pad_top;
        double acc[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
        int cnt = 0;
        for (int c = 0; c < p.nc; ++c) {
            const int y = Y - p.cy[c], x = X - p.cx[c];
            if ((unsigned)y >= (unsigned)p.ch || (unsigned)x >= (unsigned)p.cw) continue;
            ++cnt;
            float a[KMAX];
            const LinCoord cy = lin_coord(y, p.h, p.sy_lo, 1), cx = lin_coord(x, p.w, p.sx_lo, 1);
            ms_crop_softmax<KMAX>(p.lo_plain + (size_t)c * lo_stride, K, p.h, p.w, cy, cx, a);
            if (p.lo_flip) {
                float b[KMAX];
                const LinCoord fx = lin_coord(p.cw - 1 - x, p.w, p.sx_lo, 1);
                ms_crop_softmax<KMAX>(p.lo_flip + (size_t)c * lo_stride, K, p.h, p.w, cy, fx, b);
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) a[k] = __fdiv_rn(__fadd_rn(a[k], b[k]), 2.f);
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) acc[k] += (double)a[k];
        }
        const double count = (double)cnt;
        double* o = p.scaled + ((size_t)y_un * p.new_w + x_un) * K;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) o[k] = acc[k] / count;
    }
}

// ------------------------------------------------------------------ (c) accumulation over the scales
// pred[H][W][K] (+)= half-pixel bilinear resize, in float64, of (b)'s map to the frame (:294, :201); the first scale writes
// instead of adding (:191 zeros), the last one divides by the number of scales (:202) and writes the argmax (:203, the first
// maximum wins as np.argmax).
template <int KMAX>
__global__ __launch_bounds__(256) void ms_accumulate_kernel(const double* __restrict__ scaled, int new_h, int new_w, int K, double sy, double sx,
                                                            double* __restrict__ pred, int H, int W, int first, int last, double nscales,
                                                            uint8_t* __restrict__ mask) {
    const int X = blockIdx.x * 256 + threadIdx.x;
    if (X >= W) return;
    const HalfPix cx = half_pix(X, new_w, sx);
    const double wx0 = 1.0 - cx.w1;
    for (int Y = blockIdx.y; Y < H; Y += gridDim.y) {
        const HalfPix cy = half_pix(Y, new_h, sy);
        const double wy0 = 1.0 - cy.w1;
        const double* t00 = scaled + ((size_t)cy.i0 * new_w + cx.i0) * K;
        const double* t01 = scaled + ((size_t)cy.i0 * new_w + cx.i1) * K;
        const double* t10 = scaled + ((size_t)cy.i1 * new_w + cx.i0) * K;
        const double* t11 = scaled + ((size_t)cy.i1 * new_w + cx.i1) * K;
        double* o = pred + ((size_t)Y * W + X) * K;
        double best = 0.0;
        int arg = 0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                const double top = wx0 * t00[k] + cx.w1 * t01[k], bot = wx0 * t10[k] + cx.w1 * t11[k];
                double v = wy0 * top + cy.w1 * bot;
                if (!first) v = o[k] + v;
                if (last) v = v / nscales;
                o[k] = v;
                if (k == 0 || v > best) { best = v; arg = k; }
            }
        if (mask) mask[(size_t)Y * W + X] = (uint8_t)arg;
    }
}

int launch_ms_fuse(MsFuseParams p, double* pred, int H, int W, int scale_index, int nscales, uint8_t* mask, hipStream_t s) {
    FS_REQUIRE(p.K >= 1 && p.K <= 8, "ms_fuse: K=%d out of range (1..8)", p.K);
    FS_REQUIRE(p.nc >= 1 && p.nc <= 64, "ms_fuse: %d crops; one scale takes 1..64 (a larger scale is refused, not split)", p.nc);
    FS_REQUIRE(p.h >= 1 && p.w >= 1 && p.ch >= 1 && p.cw >= 1 && p.new_h >= 1 && p.new_w >= 1, "ms_fuse: empty geometry");
    FS_REQUIRE(p.PH >= p.new_h && p.PW >= p.new_w && p.PH <= 32767 && p.PW <= 32767, "ms_fuse: padded frame %dx%d does not hold the scaled frame %dx%d",
               p.PH, p.PW, p.new_h, p.new_w);
    FS_REQUIRE((int64_t)p.h * p.w * p.K < ((int64_t)1 << 31), "ms_fuse: logits of one crop too large");
    for (int c = 0; c < p.nc; ++c)
        FS_REQUIRE(p.cy[c] >= 0 && p.cx[c] >= 0 && p.cy[c] + p.ch <= p.PH && p.cx[c] + p.cw <= p.PW, "ms_fuse: crop %d outside the %dx%d frame", c,
                   p.PH, p.PW);
    FS_REQUIRE(!pred || (H >= 1 && W >= 1 && H <= 32767 && W <= 32767), "ms_fuse: frame sizes must lie in 1..32767");
    FS_REQUIRE(!pred || (nscales >= 1 && scale_index >= 0 && scale_index < nscales), "ms_fuse: scale %d of %d", scale_index, nscales);
    FS_REQUIRE(pred || !mask, "ms_fuse: the mask is the argmax of the frame prediction, which was not given");
    p.pad_top = (p.PH - p.new_h) / 2;  // int(pad / 2), :269-270
    p.pad_left = (p.PW - p.new_w) / 2;
    p.sy_lo = resize_scale(p.h, p.ch, 1);
    p.sx_lo = resize_scale(p.w, p.cw, 1);
    hipLaunchKernelGGL((ms_fuse_crops_kernel<8>), dim3((unsigned)cdiv(p.new_w, 256), (unsigned)std::min(p.new_h, 65535)), dim3(256), 0, s, p);
    if (pred) {
        const int last = scale_index == nscales - 1;
        hipLaunchKernelGGL((ms_accumulate_kernel<8>), dim3((unsigned)cdiv(W, 256), (unsigned)std::min(H, 65535)), dim3(256), 0, s, p.scaled, p.new_h,
                           p.new_w, p.K, (double)p.new_h / (double)H, (double)p.new_w / (double)W, pred, H, W, scale_index == 0, last,
                           (double)nscales, last ? mask : nullptr);
    }
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
