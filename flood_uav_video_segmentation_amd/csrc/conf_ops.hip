// Per-pixel confidence and the per-frame extent report (include/floodseg_test.h: mask_confidence, canvas_confidence, frame_report;
// DESIGN §3.10).  OUR DEFINITION -- the reference emits hard masks only.  Opt-in passes behind the tails: nothing on the shipped
// routes calls them.
//   mask_confidence     fp32 logits [n,K,h,w]        -> uint8 mask + uint8 confidence [n,H,W]: softmax_k of the (resized) logits
//   canvas_confidence   float64 mean probabilities   -> the same two planes: the winning probability itself
//   frame_report        mask (+ confidence) [n,H,W]  -> int64 [n][K][3]: pixels, sum of confidence codes, pixels below `low`
// The interpolation and the softmax are interp.h's (lin_coord, bilerp, softmax_k); the float64 resize restates
// canvas_resize_argmax_kernel (flow_ops.hip) expression by expression.  One thread per output pixel, a row of 256 pixels per
// workgroup: the loads of a wave are 64 consecutive floats of each tap row, and with W % 4 == 0 and 4-byte aligned planes four
// neighbouring lanes pack their bytes through cross-lane moves into one dword store (wave64: the four lanes sit in one wave).
// Every tap index is clamped before the load and every load is unconditional: lanes past the row's end compute
// the row's last pixel and store nothing.
#include "interp.h"
#include "kernels.h"

#include <algorithm>

namespace fs {

namespace {

// the two result bytes of one pixel: a byte store each, or -- WIDE -- one dword each per four lanes
template <bool WIDE>
__device__ __forceinline__ void store_pair(uint8_t* __restrict__ mask, uint8_t* __restrict__ conf, size_t row, int x, int W, unsigned m,
                                           unsigned c) {
    if (WIDE) {
        const unsigned p0 = m | (c << 8);
        const unsigned p1 = __shfl_down(p0, 1), p2 = __shfl_down(p0, 2), p3 = __shfl_down(p0, 3);
        if ((threadIdx.x & 3) == 0 && x < W) {  // W % 4 == 0: x + 3 < W as well
            const unsigned mw = (p0 & 255u) | ((p1 & 255u) << 8) | ((p2 & 255u) << 16) | ((p3 & 255u) << 24);
            const unsigned cw = ((p0 >> 8) & 255u) | (((p1 >> 8) & 255u) << 8) | (((p2 >> 8) & 255u) << 16) | (((p3 >> 8) & 255u) << 24);
            *reinterpret_cast<unsigned*>(mask + row + x) = mw;
            *reinterpret_cast<unsigned*>(conf + row + x) = cw;
        }
    } else if (x < W) {
        mask[row + x] = (uint8_t)m;
        conf[row + x] = (uint8_t)c;
    }
}

}  // namespace

// ------------------------------------------------------------------ confidence from fp32 logits
// RESIZE: the values of resize_argmax_u8_kernel (lin_coord + bilerp_at, align_corners=True) and its argmax (first value above
// -inf that nothing later exceeds); !RESIZE: the logits themselves and argmax_u8_kernel's argmax (class 0 until a later value
// exceeds it).  grid = (256-pixel row pieces, rows, frames): no division per pixel, and a row's trip count is uniform per workgroup,
// which the cross-lane packing needs.
template <int KMAX, bool RESIZE, bool WIDE>
__global__ __launch_bounds__(256) void mask_confidence_kernel(const float* __restrict__ in, int K, int h, int w, uint8_t* __restrict__ mask,
                                                              uint8_t* __restrict__ conf, int H, int W, float sy, float sx) {
    const int HWi = h * w;  // < 2^31 (launcher)
    const float* base = in + (size_t)blockIdx.z * K * HWi;
    const size_t obase = (size_t)blockIdx.z * H * W;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int xc = min(x, W - 1);
    LinCoord cx{};
    if (RESIZE) cx = lin_coord(xc, w, sx, 1);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        float v[KMAX];
        int arg = 0;
        if (RESIZE) {
            const LinCoord cy = lin_coord(y, h, sy, 1);
            // bilerp_at's four taps, their offsets formed once per pixel for all classes: a class's plane base is uniform, so a tap is a
            // scalar base + one 32-bit lane offset.  The K <= 32 form still spills here (246..251 VGPRs, 1668 B of scratch per lane, as
            // seg_fuse_kernel<32, false, false> does): correct, slow, and on no route of this project (K = 5).
            const int o00 = cy.i0 * w + cx.i0, o01 = cy.i0 * w + cx.i1, o10 = cy.i1 * w + cx.i0, o11 = cy.i1 * w + cx.i1;
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) {
                    const float* pl = base + (size_t)k * HWi;
                    v[k] = bilerp(pl[o00], pl[o01], pl[o10], pl[o11], cy, cx);
                }
            float best = -INFINITY;
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K && v[k] > best) { best = v[k]; arg = k; }
        } else {
            const int px = y * w + xc;
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) v[k] = base[(size_t)k * HWi + px];
            float best = v[0];
#pragma unroll
            for (int k = 1; k < KMAX; ++k)
                if (k < K && v[k] > best) { best = v[k]; arg = k; }
        }
        float c = 0.f;
        softmax_k<KMAX>(v, K, [&](int k, float q) { c = k == arg ? q : c; });
        const int code = min(255, max(0, __float2int_rn(255.f * c)));
        store_pair<WIDE>(mask, conf, obase + (size_t)y * W, x, W, (unsigned)arg, c == c ? (unsigned)code : 0u);
    }
}

int launch_mask_confidence(const float* logits, int n, int K, int h, int w, uint8_t* mask, uint8_t* conf, int H, int W, hipStream_t s) {
    FS_REQUIRE(logits && mask && conf, "mask_confidence: null pointer");
    FS_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "mask_confidence: sizes must be >= 1 (at most 65535 frames), got n=%d %dx%d -> %dx%d", n, h, w, H, W);
    FS_REQUIRE(K >= 1 && K <= 32, "mask_confidence: K=%d out of range (1..32)", K);
    FS_REQUIRE((int64_t)h * w < ((int64_t)1 << 31) && (int64_t)H * W < ((int64_t)1 << 31), "mask_confidence: a plane of 2^31 elements or more (%dx%d -> %dx%d)", h, w, H, W);
    const bool resize = h != H || w != W;
    const bool wide = W % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0 && reinterpret_cast<uintptr_t>(conf) % 4 == 0;
    const float sy = resize_scale(h, H, 1), sx = resize_scale(w, W, 1);
    const dim3 grid((unsigned)cdiv(W, 256), (unsigned)std::min(H, 65535), (unsigned)n), block(256);
#define FS_CONF(KM_, R_, W_) hipLaunchKernelGGL((mask_confidence_kernel<KM_, R_, W_>), grid, block, 0, s, logits, K, h, w, mask, conf, H, W, sy, sx)
#define FS_CONF_K(KM_)                                                    \
    do {                                                                  \
        if (resize) { if (wide) FS_CONF(KM_, true, true); else FS_CONF(KM_, true, false); } \
        else { if (wide) FS_CONF(KM_, false, true); else FS_CONF(KM_, false, false); }      \
    } while (0)
    if (K <= 8) FS_CONF_K(8);
    else FS_CONF_K(32);
#undef FS_CONF_K
#undef FS_CONF
    FS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ confidence from the float64 crop-averaged canvas
// The values and the mask of canvas_resize_argmax_kernel (ATen's upsample_bilinear2d with accscalar_t = double, align_corners=True);
// the confidence is the winning value.  No class array: the maximum is all that is kept, so K runs to 255.  Equal sizes take the same
// four taps (weights 1 and 0): the value is the canvas value for finite data, and a NaN reaches the neighbours it reaches in that op,
// so the mask is that op's mask on any input.
template <bool WIDE>
__global__ __launch_bounds__(256) void canvas_confidence_kernel(const double* __restrict__ canvas, int K, int Hi, int Wi,
                                                                uint8_t* __restrict__ mask, uint8_t* __restrict__ conf, int Ho, int Wo, double sy,
                                                                double sx) {
    const size_t HWi = (size_t)Hi * Wi;
    const double* base = canvas + (size_t)blockIdx.z * K * HWi;
    const size_t obase = (size_t)blockIdx.z * Ho * Wo;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int ox = min(x, Wo - 1);
    const double w1r = sx * ox;
    const int w1 = min((int)w1r, Wi - 1);
    const int w1p = w1 < Wi - 1 ? 1 : 0;
    const double w1l = w1r - w1, w0l = 1.0 - w1l;
    for (int oy = blockIdx.y; oy < Ho; oy += gridDim.y) {
        const double h1r = sy * oy;
        const int h1 = min((int)h1r, Hi - 1);
        const int h1p = h1 < Hi - 1 ? 1 : 0;
        const double h1l = h1r - h1, h0l = 1.0 - h1l;
        double best = -INFINITY;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const double* pl = base + (size_t)k * HWi + (size_t)h1 * Wi + w1;
            const double v = h0l * (w0l * pl[0] + w1l * pl[w1p]) + h1l * (w0l * pl[(size_t)h1p * Wi] + w1l * pl[(size_t)h1p * Wi + w1p]);
            if (v > best) { best = v; arg = k; }
        }
        // the winning value (no value above -inf: class 0, whose value is a NaN or -inf -- code 0 either way)
        const double code = fmin(255.0, fmax(0.0, rint(255.0 * best)));
        store_pair<WIDE>(mask, conf, obase + (size_t)oy * Wo, x, Wo, (unsigned)arg, best == best ? (unsigned)(int)code : 0u);
    }
}

int launch_canvas_confidence(const double* canvas, int n, int K, int Hi, int Wi, uint8_t* mask, uint8_t* conf, int Ho, int Wo, hipStream_t s) {
    FS_REQUIRE(canvas && mask && conf, "canvas_confidence: null pointer");
    FS_REQUIRE(n >= 1 && n <= 65535 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "canvas_confidence: sizes must be >= 1 (at most 65535 frames), got n=%d %dx%d -> %dx%d", n, Hi, Wi, Ho, Wo);
    FS_REQUIRE(K >= 1 && K <= 255, "canvas_confidence: K=%d out of range (1..255)", K);
    FS_REQUIRE((int64_t)Hi * Wi < ((int64_t)1 << 31) && (int64_t)Ho * Wo < ((int64_t)1 << 31), "canvas_confidence: a plane of 2^31 elements or more (%dx%d -> %dx%d)", Hi, Wi, Ho, Wo);
    const bool wide = Wo % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0 && reinterpret_cast<uintptr_t>(conf) % 4 == 0;
    const double sy = Ho > 1 ? (double)(Hi - 1) / (double)(Ho - 1) : 0.0, sx = Wo > 1 ? (double)(Wi - 1) / (double)(Wo - 1) : 0.0;
    const dim3 grid((unsigned)cdiv(Wo, 256), (unsigned)std::min(Ho, 65535), (unsigned)n), block(256);
    if (wide) hipLaunchKernelGGL((canvas_confidence_kernel<true>), grid, block, 0, s, canvas, K, Hi, Wi, mask, conf, Ho, Wo, sy, sx);
    else hipLaunchKernelGGL((canvas_confidence_kernel<false>), grid, block, 0, s, canvas, K, Hi, Wi, mask, conf, Ho, Wo, sy, sx);
    FS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ per-frame, per-class report
// out[f][k] = (pixels of class k, sum of their confidence codes, pixels of class k with code < low), int64, integers throughout: the
// result does not depend on the order of anything.  A workgroup owns REPORT_CHUNK consecutive pixels of one frame and counts them
// into LDS, one table per wave (four waves do not contend for one class's counter), the three figures of a pixel packed into ONE
// 64-bit LDS add: bits 0..23 the code sum (<= 255 * 16384 < 2^24), 24..43 the pixels below `low`, 44..63 the pixels (<= 16384
// each).  The tables are then unpacked and merged into the output with 64-bit integer vector atomics -- at most 3 K per workgroup.
// The output is zeroed by a launch of its own in front (report_zero_kernel), on the same stream: every call writes it whole.
constexpr int REPORT_CHUNK = 16384;

__global__ __launch_bounds__(256) void report_zero_kernel(unsigned long long* __restrict__ out, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) out[i] = 0ull;
}

template <bool CONF>
__global__ __launch_bounds__(256) void frame_report_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ conf, int HW, int K,
                                                           int low, unsigned long long* __restrict__ out) {
    extern __shared__ unsigned long long tab[];  // [4 waves][K]
    for (int i = threadIdx.x; i < 4 * K; i += 256) tab[i] = 0ull;
    __syncthreads();
    const size_t fbase = (size_t)blockIdx.y * HW;
    unsigned long long* mine = tab + (threadIdx.x >> 6) * K;
    const int begin = blockIdx.x * REPORT_CHUNK, end = min(HW, begin + REPORT_CHUNK);  // begin < HW (grid), HW < 2^31 - REPORT_CHUNK (launcher)
    for (int i = begin + threadIdx.x; i < end; i += 256) {
        const int m = mask[fbase + i];
        unsigned long long add = 1ull << 44;
        if (CONF) {
            const unsigned c = conf[fbase + i];
            add |= (unsigned long long)c | ((unsigned long long)(c < (unsigned)low ? 1u : 0u) << 24);
        }
        if (m < K) atomicAdd(&mine[m], add);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const unsigned long long t = tab[k] + tab[K + k] + tab[2 * K + k] + tab[3 * K + k];  // fields cannot carry: sums over one chunk
        unsigned long long* row = out + ((size_t)blockIdx.y * K + k) * 3;
        const unsigned long long pixels = t >> 44, below = (t >> 24) & 0xFFFFFull, sum = t & 0xFFFFFFull;
        if (pixels) atomicAdd(&row[0], pixels);
        if (sum) atomicAdd(&row[1], sum);
        if (below) atomicAdd(&row[2], below);
    }
}

int launch_frame_report(const uint8_t* mask, const uint8_t* conf, int n, int H, int W, int K, int low, long long* out, hipStream_t s) {
    FS_REQUIRE(mask && out, "frame_report: null pointer");
    FS_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1, "frame_report: sizes must be >= 1 (at most 65535 frames), got n=%d %dx%d", n, H, W);
    FS_REQUIRE(K >= 1 && K <= 255, "frame_report: K=%d out of range (1..255)", K);
    FS_REQUIRE(low >= 0 && low <= 255, "frame_report: low=%d out of range (0..255)", low);
    FS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - REPORT_CHUNK, "frame_report: a frame of 2^31 pixels or more (%dx%d)", H, W);
    const int HW = H * W, total = n * K * 3;
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    hipLaunchKernelGGL(report_zero_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, o, total);
    const dim3 grid((unsigned)cdiv(HW, REPORT_CHUNK), (unsigned)n);
    const size_t lds = (size_t)4 * K * sizeof(unsigned long long);
    if (conf) hipLaunchKernelGGL((frame_report_kernel<true>), grid, dim3(256), lds, s, mask, conf, HW, K, low, o);
    else hipLaunchKernelGGL((frame_report_kernel<false>), grid, dim3(256), lds, s, mask, conf, HW, K, low, o);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
