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
#include "common.h"
#include "ingest_src.h"
#include "interp.h"
#include "kernels.h"

namespace fs {
namespace {

struct EgressOut {
    uint8_t* p0;  // RGB24: the interleaved frame; YUV: the Y plane
    uint8_t* pu;  // YUV: the first U sample
    uint8_t* pv;  // YUV: the first V sample
    int cstep;    // bytes from one sample of a chroma plane to the next (2: NV12, 1: I420)
    int yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb;
};

// rows of the RGB -> YUV table of include/floodseg_test.h, index matrix * 2 + full_range: yr yg yb yoff | ur ug ub | vr vg vb
constexpr int RGB_COEF[4][10] = {{66, 129, 25, 16, -38, -74, 112, 112, -94, -18},
                                 {77, 150, 29, 0, -43, -85, 128, 128, -107, -21},
                                 {47, 157, 16, 16, -26, -86, 112, 112, -102, -10},
                                 {54, 183, 19, 0, -29, -99, 128, 128, -116, -12}};

__device__ __forceinline__ uint32_t clip255(int v) { return (uint32_t)min(max(v, 0), 255); }
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }

// BG 0: no background; 1: RGB24 source; 2: NV12 / I420 source.  MODE: resized4's (ingest_src.h).  VEC: the wide route.
template <int BG, int MODE, bool YUV_OUT, bool VEC>
__global__ __launch_bounds__(256) void frame_compose_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ palette, int K, IngestSrc s,
                                                            EgressOut o, int h, int w, int ngroups, int npairs, float sy, float sx) {
    __shared__ uint32_t pal[256];  // R | G << 8 | B << 16 | A << 24 per mask value: values >= K hold class 0's entry
    {
        const uint8_t* p = palette + 4 * ((int)threadIdx.x < K ? (int)threadIdx.x : 0);
        pal[threadIdx.x] = pack4(p[0], p[1], p[2], p[3]);
    }
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
        const uint8_t* mrow = mask + (size_t)row[r] * w;
        uint32_t cls[8];
        if (VEC) {
            const uint2 m = *reinterpret_cast<const uint2*>(mrow + x0);
#pragma unroll
            for (int i = 0; i < 4; ++i) cls[i] = (m.x >> (8 * i)) & 255, cls[4 + i] = (m.y >> (8 * i)) & 255;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) cls[i] = mrow[col[i]];
        }
        float bg[8][3];
        if (BG) {
            float a[4][3], b[4][3];
            resized4<BG == 2, MODE>(s, row[r], x0, w, sy, sx, a);
            resized4<BG == 2, MODE>(s, row[r], (VEC || x0 + 4 < w) ? x0 + 4 : x0, w, sy, sx, b);  // a group wholly past the frame is replaced below
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) bg[i][c] = a[i][c], bg[4 + i][c] = b[i][c];
            if (!VEC) {
#pragma unroll
                for (int i = 1; i < 8; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) bg[i][c] = x0 + i < w ? bg[i][c] : bg[i - 1][c];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t e = pal[cls[i]];
            const int A = (int)(e >> 24);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int colour = (int)((e >> (8 * c)) & 255);
                px[r][i][c] = BG ? (int)((unsigned)(A * colour + (255 - A) * (int)bg[i][c] + 127) / 255u) : colour;  // all terms >= 0
            }
        }
    }

    if (!YUV_OUT) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint8_t* dst = o.p0 + (size_t)row[r] * w * 3;
            if (VEC) {
                uint32_t d[6];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 | ...
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int i = 4 * g;
                    d[3 * g] = pack4(px[r][i][0], px[r][i][1], px[r][i][2], px[r][i + 1][0]);
                    d[3 * g + 1] = pack4(px[r][i + 1][1], px[r][i + 1][2], px[r][i + 2][0], px[r][i + 2][1]);
                    d[3 * g + 2] = pack4(px[r][i + 2][2], px[r][i + 3][0], px[r][i + 3][1], px[r][i + 3][2]);
                }
                uint2* q = reinterpret_cast<uint2*>(dst + (size_t)x0 * 3);
                q[0] = make_uint2(d[0], d[1]);
                q[1] = make_uint2(d[2], d[3]);
                q[2] = make_uint2(d[4], d[5]);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) dst[(size_t)col[i] * 3 + c] = (uint8_t)px[r][i][c];
            }
        }
        return;
    }

    uint32_t Y[2][8];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            Y[r][i] = clip255(((o.yr * px[r][i][0] + o.yg * px[r][i][1] + o.yb * px[r][i][2] + 128) >> 8) + o.yoff);
    const int cw = (w + 1) >> 1;
    uint32_t U[4], V[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = (px[0][2 * j][c] + px[0][2 * j + 1][c] + px[1][2 * j][c] + px[1][2 * j + 1][c] + 2) >> 2;
        U[j] = clip255(((o.ur * m[0] + o.ug * m[1] + o.ub * m[2] + 128) >> 8) + 128);
        V[j] = clip255(((o.vr * m[0] + o.vg * m[1] + o.vb * m[2] + 128) >> 8) + 128);
    }
    const int c0 = x0 >> 1;
    if (VEC) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
            *reinterpret_cast<uint2*>(o.p0 + (size_t)row[r] * w + x0) = make_uint2(pack4(Y[r][0], Y[r][1], Y[r][2], Y[r][3]), pack4(Y[r][4], Y[r][5], Y[r][6], Y[r][7]));
        const size_t q = ((size_t)py * cw + c0) * o.cstep;
        if (o.cstep == 2) {
            *reinterpret_cast<uint2*>(o.pu + q) = make_uint2(pack4(U[0], V[0], U[1], V[1]), pack4(U[2], V[2], U[3], V[3]));
        } else {
            *reinterpret_cast<uint32_t*>(o.pu + q) = pack4(U[0], U[1], U[2], U[3]);
            *reinterpret_cast<uint32_t*>(o.pv + q) = pack4(V[0], V[1], V[2], V[3]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i) o.p0[(size_t)row[r] * w + col[i]] = (uint8_t)Y[r][i];
#pragma unroll
        for (int j = 1; j < 4; ++j)  // a quad wholly past the frame takes the last one inside it (not the replicated column's own quad)
            U[j] = c0 + j < cw ? U[j] : U[j - 1], V[j] = c0 + j < cw ? V[j] : V[j - 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t q = ((size_t)py * cw + min(c0 + j, cw - 1)) * o.cstep;
            o.pu[q] = (uint8_t)U[j];
            o.pv[q] = (uint8_t)V[j];
        }
    }
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

int launch_frame_compose(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                         int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                         int out_matrix, int out_full_range, hipStream_t st) {
    EgressOut o{};
    o.p0 = out;
    auto aligned = [](const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
    bool vec = w % 8 == 0 && aligned(mask, 8) && aligned(out, 8);
    if (out_format != 0) {
        const int* k = RGB_COEF[out_matrix * 2 + out_full_range];
        o.yr = k[0], o.yg = k[1], o.yb = k[2], o.yoff = k[3], o.ur = k[4], o.ug = k[5], o.ub = k[6], o.vr = k[7], o.vg = k[8], o.vb = k[9];
        o.cstep = out_format == 1 ? 2 : 1;
        o.pu = out_u;
        o.pv = out_format == 1 ? out_u + 1 : out_v;
        vec = vec && (out_format == 1 ? aligned(out_u, 8) : aligned(out_u, 4) && aligned(out_v, 4));
    }
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
