// The per-thread pieces of frame egress that frame_compose_kernel (egress_ops.hip) and frame_compose_regions_kernel (overlay_ops.hip)
// share, so that the two agree bit for bit on everything but the layers the second one adds: the mask classes and the background of
// one row of eight slots, the per-pixel blend, and the stores of a thread's two rows by eight columns as RGB24, NV12 or I420 on the
// wide and on the byte route (the routes and their reasons: the head of egress_ops.hip).  Compile every user with -ffp-contract=off
// (ingest_src.h).
#pragma once
#include "common.h"
#include "ingest_src.h"
#include "interp.h"

namespace fs {

struct EgressOut {
    uint8_t* p0;  // RGB24: the interleaved frame; YUV: the Y plane
    uint8_t* pu;  // YUV: the first U sample
    uint8_t* pv;  // YUV: the first V sample
    int cstep;    // bytes from one sample of a chroma plane to the next (2: NV12, 1: I420)
    int yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb;
};

// the output planes and the RGB -> YUV row of one call (egress_ops.hip holds the table); *vec: the wide route is possible (w % 8 == 0 and
// mask and planes aligned as the head of egress_ops.hip says)
EgressOut make_egress_out(const uint8_t* mask, int w, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format, int out_matrix, int out_full_range,
                          bool* vec);

__device__ __forceinline__ uint32_t clip255(int v) { return (uint32_t)min(max(v, 0), 255); }
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }

// one palette of <= 256 (R, G, B, A) entries into LDS as R | G << 8 | B << 16 | A << 24 per mask value: values >= K hold class 0's entry.
// 256 threads; the caller synchronises.
__device__ __forceinline__ void stage_palette(uint32_t (&pal)[256], const uint8_t* __restrict__ palette, int K) {
    const uint8_t* p = palette + 4 * ((int)threadIdx.x < K ? (int)threadIdx.x : 0);
    pal[threadIdx.x] = pack4(p[0], p[1], p[2], p[3]);
}

// the mask values of row `mrow` at the eight slots (VEC: columns x0 .. x0 + 7 as two dwords; else the columns col[])
template <bool VEC>
__device__ __forceinline__ void egress_classes(const uint8_t* __restrict__ mrow, int x0, const int (&col)[8], uint32_t (&cls)[8]) {
    if (VEC) {
        const uint2 m = *reinterpret_cast<const uint2*>(mrow + x0);
#pragma unroll
        for (int i = 0; i < 4; ++i) cls[i] = (m.x >> (8 * i)) & 255, cls[4 + i] = (m.y >> (8 * i)) & 255;
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) cls[i] = mrow[col[i]];
    }
}

// the background of the eight slots of output row `row`: resized4's image; on the byte route a slot past the frame takes the last one inside
template <int BG, int MODE, bool VEC>
__device__ __forceinline__ void egress_background(const IngestSrc& s, int row, int x0, int w, float sy, float sx, float (&bg)[8][3]) {
    float a[4][3], b[4][3];
    resized4<BG == 2, MODE>(s, row, x0, w, sy, sx, a);
    resized4<BG == 2, MODE>(s, row, (VEC || x0 + 4 < w) ? x0 + 4 : x0, w, sy, sx, b);  // a group wholly past the frame is replaced below
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

// o = (A * colour + (255 - A) * under + 127) / 255 in int32, all terms >= 0
__device__ __forceinline__ int blend255(int A, int colour, int under) { return (int)((unsigned)(A * colour + (255 - A) * under + 127) / 255u); }

// one pixel: the palette entry e over the background value (BG != 0), or the colour alone
template <int BG>
__device__ __forceinline__ void egress_blend(uint32_t e, const float (&bg)[3], int (&o)[3]) {
    const int A = (int)(e >> 24);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int colour = (int)((e >> (8 * c)) & 255);
        o[c] = BG ? blend255(A, colour, (int)bg[c]) : colour;
    }
}

// a thread's two rows (row[0], row[1]) by eight slots of finished RGB leave as RGB24, or as Y rows and the four chroma quads of row
// pair py.  Byte route: a slot past the frame holds the value of the last one inside it and is stored at that one's address.
template <bool YUV_OUT, bool VEC>
__device__ __forceinline__ void egress_store(const EgressOut& o, const int (&px)[2][8][3], const int (&row)[2], const int (&col)[8], int x0, int py, int w) {
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

}  // namespace fs
