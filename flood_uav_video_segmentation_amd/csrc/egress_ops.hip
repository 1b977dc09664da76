// Frame egress: one uint8 mask (+ a palette with per-class opacity, + optionally the decoded source frame as background) -> one result
// video frame in RGB24, NV12 or I420, one launch (the mirror image of ingest_ops.hip; the reference appends colors[output] to an .avi
// on the host, flow/base.py:250-253, 308-312).  Per output pixel: class c = mask < K ? mask : 0 (colorize_kernel's rule), colour and
// opacity (R, G, B, A) = palette[c]; background b = the uint8 image the network saw (resized4 of ingest_src.h, the very code
// frame_prepare runs up to its normalisation); o = (A * colour + (255 - A) * b + 127) / 255 in int32, or o = colour without a
// background; then, for the 4:2:0 outputs, the integer RGB -> YUV of include/floodseg_test.h: Y from the pixel's own RGB, one U / V
// pair from the per-channel mean (sum + 2) >> 2 of its 2 x 2 quad (rows / columns past the frame repeat the last one).  Nothing in
// between reaches HBM.
//
// Bandwidth-bound (1072 x 1920: 2.1 MB of mask read, 6.2 MB of RGB24 or 3.1 MB of NV12 written, + 3.1 MB of NV12 background).
// Width per thread: TWO ROWS BY EIGHT COLUMNS = four whole chroma quads.  The mask rows are read as two dwords each; a Y row leaves as
// one 8-byte store, the NV12 UV row as one 8-byte store (I420: one dword per plane), an RGB24 row as three 8-byte stores -- the
// 8 - 16 bytes per lane the guides name as the coalescing sweet spot.  Sixteen columns would make every store 16 bytes but leaves
// only ~1000 waves at 1072 x 1920 (4 per CU, too few to hide the latency of the loads in front of the stores), doubles the 48
// background values a thread already holds on the overlay path, and needs w % 16 == 0; four columns makes the Y and UV stores
// single dwords.  The palette (<= 1 KiB) is staged in LDS once per workgroup with the ids >= K already mapped to class 0, so a lookup
// is one ds_read.
// The wide route needs w % 8 == 0 and 8-byte aligned mask / output planes (4-byte: the I420 chroma planes).  Everything else (odd
// sizes, a destination at any byte offset) takes the straight-line byte route: every element past the frame is given the value of
// the last one inside it and is stored at that one's address -- the same thread rewriting the same byte with the same value -- so
// that no store sits behind a branch of its own (tests/test_isa_guards.py).  The odd last row is handled that way on both routes.
// The per-thread pieces (classes, background, blend, RGB -> YUV, both store routes) live in egress_px.h, which the region overlay
// (overlay_ops.hip) shares; this file keeps the kernel, the coefficient table and the launcher.
#include "common.h"
#include "egress_px.h"
#include "ingest_src.h"
#include "interp.h"
#include "kernels.h"

namespace fs {
namespace {

// rows of the RGB -> YUV table of include/floodseg_test.h, index matrix * 2 + full_range: yr yg yb yoff | ur ug ub | vr vg vb
constexpr int RGB_COEF[4][10] = {{66, 129, 25, 16, -38, -74, 112, 112, -94, -18},
                                 {77, 150, 29, 0, -43, -85, 128, 128, -107, -21},
                                 {47, 157, 16, 16, -26, -86, 112, 112, -102, -10},
                                 {54, 183, 19, 0, -29, -99, 128, 128, -116, -12}};

// BG 0: no background; 1: RGB24 source; 2: NV12 / I420 source.  MODE: resized4's (ingest_src.h).  VEC: the wide route.
template <int BG, int MODE, bool YUV_OUT, bool VEC>
__global__ __launch_bounds__(256) void frame_compose_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ palette, int K, IngestSrc s,
                                                            EgressOut o, int h, int w, int ngroups, int npairs, float sy, float sx) {
    __shared__ uint32_t pal[256];  // R | G << 8 | B << 16 | A << 24 per mask value: values >= K hold class 0's entry
    stage_palette(pal, palette, K);
    __syncthreads();
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)npairs * (unsigned)ngroups) return;
    const int py = (int)(idx / (unsigned)ngroups), x0 = (int)(idx - (unsigned)py * (unsigned)ngroups) * 8;
    const int row[2] = {2 * py, min(2 * py + 1, h - 1)};  // an odd last row is its own partner
    int col[8];                                            // the column each of the eight slots stands for
#pragma unroll
    for (int i = 0; i < 8; ++i) col[i] = VEC ? x0 + i : min(x0 + i, w - 1);

    int px[2][8][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t cls[8];
        egress_classes<VEC>(mask + (size_t)row[r] * w, x0, col, cls);
        float bg[8][3];
        if (BG) egress_background<BG, MODE, VEC>(s, row[r], x0, w, sy, sx, bg);
#pragma unroll
        for (int i = 0; i < 8; ++i) egress_blend<BG>(pal[cls[i]], bg[i], px[r][i]);
    }
    egress_store<YUV_OUT, VEC>(o, px, row, col, x0, py, w);
}

template <int BG, int MODE>
void launch_out(const uint8_t* mask, const uint8_t* palette, int K, const IngestSrc& s, const EgressOut& o, int h, int w, bool yuv_out, bool vec,
                hipStream_t st) {
    const int ngroups = cdiv(w, 8), npairs = cdiv(h, 2);
    const dim3 grid((unsigned)cdiv64((int64_t)npairs * ngroups, 256));
    const float sy = BG ? resize_scale(s.H, h, 0) : 1.f, sx = BG ? resize_scale(s.W, w, 0) : 1.f;
    if (yuv_out && vec)
        frame_compose_kernel<BG, MODE, true, true><<<grid, 256, 0, st>>>(mask, palette, K, s, o, h, w, ngroups, npairs, sy, sx);
    else if (yuv_out)
        frame_compose_kernel<BG, MODE, true, false><<<grid, 256, 0, st>>>(mask, palette, K, s, o, h, w, ngroups, npairs, sy, sx);
    else if (vec)
        frame_compose_kernel<BG, MODE, false, true><<<grid, 256, 0, st>>>(mask, palette, K, s, o, h, w, ngroups, npairs, sy, sx);
    else
        frame_compose_kernel<BG, MODE, false, false><<<grid, 256, 0, st>>>(mask, palette, K, s, o, h, w, ngroups, npairs, sy, sx);
}

template <int BG>
void launch_mode(const uint8_t* mask, const uint8_t* palette, int K, const IngestSrc& s, const EgressOut& o, int h, int w, bool yuv_out, bool vec,
                 hipStream_t st) {
    if (s.H == h && s.W == w)
        launch_out<BG, 2>(mask, palette, K, s, o, h, w, yuv_out, vec, st);
    else if (s.W == w)
        launch_out<BG, 1>(mask, palette, K, s, o, h, w, yuv_out, vec, st);
    else
        launch_out<BG, 0>(mask, palette, K, s, o, h, w, yuv_out, vec, st);
}

}  // namespace

EgressOut make_egress_out(const uint8_t* mask, int w, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format, int out_matrix, int out_full_range,
                          bool* vec) {
    EgressOut o{};
    o.p0 = out;
    auto aligned = [](const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
    *vec = w % 8 == 0 && aligned(mask, 8) && aligned(out, 8);
    if (out_format != 0) {
        const int* k = RGB_COEF[out_matrix * 2 + out_full_range];
        o.yr = k[0], o.yg = k[1], o.yb = k[2], o.yoff = k[3], o.ur = k[4], o.ug = k[5], o.ub = k[6], o.vr = k[7], o.vg = k[8], o.vb = k[9];
        o.cstep = out_format == 1 ? 2 : 1;
        o.pu = out_u;
        o.pv = out_format == 1 ? out_u + 1 : out_v;
        *vec = *vec && (out_format == 1 ? aligned(out_u, 8) : aligned(out_u, 4) && aligned(out_v, 4));
    }
    return o;
}

int launch_frame_compose(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                         int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                         int out_matrix, int out_full_range, hipStream_t st) {
    bool vec;
    const EgressOut o = make_egress_out(mask, w, out, out_u, out_v, out_format, out_matrix, out_full_range, &vec);
    if (!frame) {
        launch_out<0, 2>(mask, palette, K, IngestSrc{}, o, h, w, out_format != 0, vec, st);
    } else {
        const IngestSrc s = make_ingest_src(frame, u, v, format, matrix, full_range, H, W);
        if (format == 0)
            launch_mode<1>(mask, palette, K, s, o, h, w, out_format != 0, vec, st);
        else
            launch_mode<2>(mask, palette, K, s, o, h, w, out_format != 0, vec, st);
    }
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
