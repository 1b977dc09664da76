// The decoded source frame of frame ingest (ingest_ops.hip) and of the overlay background of frame egress (egress_ops.hip): one
// description of a uint8 RGB24 / NV12 / I420 frame, its integer YUV -> RGB conversion (our definition, include/floodseg_test.h) and the
// uint8 image the network sees -- the half-pixel bilinear resize of interp.h, un-contracted, rounded half to even and clamped to
// [0, 255].  Both kernels take that image from resized4 below, so they agree on it bit for bit.  Compile every user with
// -ffp-contract=off (csrc/Makefile).
#pragma once
#include "common.h"
#include "interp.h"

namespace fs {

struct IngestSrc {
    const uint8_t* p0;  // RGB24: the interleaved frame; YUV: the Y plane
    const uint8_t* pu;  // YUV: the first U sample
    const uint8_t* pv;  // YUV: the first V sample
    int H, W;
    int cw, cstep;  // chroma samples per row; bytes from one sample of a chroma plane to the next (2: NV12, 1: I420)
    int yoff, ymul, rv, gu, gv, bu;  // c = ymul (Y - yoff); R = (c + rv e + 128) >> 8, G = (c - gu d - gv e + 128) >> 8, B = (c + bu d + 128) >> 8
    int whole_dwords;  // W % 4 == 0 and p0 4-byte aligned: four pixels of a row start on a dword
};

// rows of the conversion table of include/floodseg_test.h, index matrix * 2 + full_range: ymul, yoff, rv, gu, gv, bu
constexpr int YUV_COEF[4][6] = {{298, 16, 409, 100, 208, 516}, {256, 0, 359, 88, 183, 454}, {298, 16, 459, 55, 136, 541}, {256, 0, 403, 48, 120, 475}};

// format 0: RGB24 [H][W][3] in `frame`; 1: NV12 (u = the interleaved UV plane); 2: I420 (u, v planes); arguments validated by the caller
inline IngestSrc make_ingest_src(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int H, int W) {
    IngestSrc s{};
    s.p0 = frame;
    s.H = H;
    s.W = W;
    s.whole_dwords = W % 4 == 0 && reinterpret_cast<uintptr_t>(frame) % 4 == 0;
    if (format != 0) {
        const int* k = YUV_COEF[matrix * 2 + full_range];
        s.ymul = k[0], s.yoff = k[1], s.rv = k[2], s.gu = k[3], s.gv = k[4], s.bu = k[5];
        s.cw = cdiv(W, 2);
        s.cstep = format == 1 ? 2 : 1;
        s.pu = u;
        s.pv = format == 1 ? u + 1 : v;
    }
    return s;
}

__device__ __forceinline__ float clip_u8(int v) { return (float)min(max(v, 0), 255); }

__device__ __forceinline__ void yuv_to_rgb(const IngestSrc& s, int y, int u, int v, float (&c)[3]) {
    const int l = s.ymul * (y - s.yoff) + 128, d = u - 128, e = v - 128;
    c[0] = clip_u8((l + s.rv * e) >> 8);
    c[1] = clip_u8((l - s.gu * d - s.gv * e) >> 8);
    c[2] = clip_u8((l + s.bu * d) >> 8);
}

// the RGB value of source pixel (y, x), both inside the frame
template <bool YUV>
__device__ __forceinline__ void fetch(const IngestSrc& s, int y, int x, float (&c)[3]) {
    const size_t p = (size_t)y * s.W + x;
    if (!YUV) {
        c[0] = (float)s.p0[3 * p];
        c[1] = (float)s.p0[3 * p + 1];
        c[2] = (float)s.p0[3 * p + 2];
    } else {
        const size_t q = ((size_t)(y >> 1) * s.cw + (x >> 1)) * s.cstep;
        yuv_to_rgb(s, s.p0[p], s.pu[q], s.pv[q], c);
    }
}

// source pixels (y, x0 .. x0 + 3), x0 a multiple of 4 inside the frame; columns past the frame repeat the last one
template <bool YUV>
__device__ __forceinline__ void fetch4(const IngestSrc& s, int y, int x0, float (&c)[4][3]) {
    if (s.whole_dwords) {
        const size_t p = (size_t)y * s.W + x0;
        if (!YUV) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(s.p0 + 3 * p);
            const uint32_t a = q[0], b = q[1], d = q[2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            c[0][0] = (float)(a & 255), c[0][1] = (float)((a >> 8) & 255), c[0][2] = (float)((a >> 16) & 255);
            c[1][0] = (float)(a >> 24), c[1][1] = (float)(b & 255), c[1][2] = (float)((b >> 8) & 255);
            c[2][0] = (float)((b >> 16) & 255), c[2][1] = (float)(b >> 24), c[2][2] = (float)(d & 255);
            c[3][0] = (float)((d >> 8) & 255), c[3][1] = (float)((d >> 16) & 255), c[3][2] = (float)(d >> 24);
        } else {
            const uint32_t yy = *reinterpret_cast<const uint32_t*>(s.p0 + p);
            const size_t q = ((size_t)(y >> 1) * s.cw + (x0 >> 1)) * s.cstep;  // W % 4 == 0: the second chroma sample exists
            const int u0 = s.pu[q], v0 = s.pv[q], u1 = s.pu[q + s.cstep], v1 = s.pv[q + s.cstep];
            yuv_to_rgb(s, yy & 255, u0, v0, c[0]);
            yuv_to_rgb(s, (yy >> 8) & 255, u0, v0, c[1]);
            yuv_to_rgb(s, (yy >> 16) & 255, u1, v1, c[2]);
            yuv_to_rgb(s, yy >> 24, u1, v1, c[3]);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) fetch<YUV>(s, y, min(x0 + i, s.W - 1), c[i]);
}

// Pixels (oy, x0 .. x0 + 3) of the frame resized to h x w (oy < h, x0 < w, x0 a multiple of 4), as the uint8 image cv2.resize stores:
// integer values 0..255 held in floats.  Columns past w repeat the last one.  MODE 0: both axes resampled; 1: W == w, rows resampled
// (the horizontal scale is exactly 1, the column coordinate is the integer itself with weights (1, 0), and 1 * a + 0 * b == a for the
// finite non-negative taps, so the east taps are not loaded); 2: H == h and W == w, the pixel is its own value.
template <bool YUV, int MODE>
__device__ __forceinline__ void resized4(const IngestSrc& s, int oy, int x0, int w, float sy, float sx, float (&v)[4][3]) {
    if (MODE == 2) {
        fetch4<YUV>(s, oy, x0, v);
        return;
    }
    const LinCoord cy = lin_coord(oy, s.H, sy, 0);
    if (MODE == 1) {
        float a[4][3], b[4][3];
        fetch4<YUV>(s, cy.i0, x0, a);
        fetch4<YUV>(s, cy.i1, x0, b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[i][c] = __fadd_rn(__fmul_rn(cy.w0, a[i][c]), __fmul_rn(cy.w1, b[i][c]));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const LinCoord cx = lin_coord(min(x0 + i, w - 1), s.W, sx, 0);
            float t00[3], t01[3], t10[3], t11[3];
            fetch<YUV>(s, cy.i0, cx.i0, t00);
            fetch<YUV>(s, cy.i0, cx.i1, t01);
            fetch<YUV>(s, cy.i1, cx.i0, t10);
            fetch<YUV>(s, cy.i1, cx.i1, t11);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[i][c] = bilerp(t00[c], t01[c], t10[c], t11[c], cy, cx);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[i][c] = fminf(fmaxf(rintf(v[i][c]), 0.f), 255.f);  // .round_().clamp_(0, 255): the stored uint8 image
}

// The one-pixel form: pixel (oy, ox) of the same resized image (oy < h, ox < w), for a gather that wants single pixels at unrelated
// places (ortho_ops.hip).  The same operations in the same order as resized4 on that column, so the two agree bit for bit; MODE as there.
template <bool YUV, int MODE>
__device__ __forceinline__ void resized1(const IngestSrc& s, int oy, int ox, float sy, float sx, float (&v)[3]) {
    if (MODE == 2) {
        // The rounding line below leaves a whole number in [0, 255] as it is, and MODE 2 still runs it: returning here lets the compiler
        // pack a caller's clip(x >> 8) bytes straight from the integers with v_ashr_pk_u8_i32, and the dword a YUV caller then stored
        // had bits of the shifted operand ORed into its third byte on gfx950 (tests/test_gpu_ortho.py, the identity-resize YUV cases).
        fetch<YUV>(s, oy, ox, v);
    } else if (MODE == 1) {
        const LinCoord cy = lin_coord(oy, s.H, sy, 0);
        float a[3], b[3];
        fetch<YUV>(s, cy.i0, ox, a);
        fetch<YUV>(s, cy.i1, ox, b);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __fadd_rn(__fmul_rn(cy.w0, a[c]), __fmul_rn(cy.w1, b[c]));
    } else {
        const LinCoord cy = lin_coord(oy, s.H, sy, 0), cx = lin_coord(ox, s.W, sx, 0);
        float t00[3], t01[3], t10[3], t11[3];
        fetch<YUV>(s, cy.i0, cx.i0, t00);
        fetch<YUV>(s, cy.i0, cx.i1, t01);
        fetch<YUV>(s, cy.i1, cx.i0, t10);
        fetch<YUV>(s, cy.i1, cx.i1, t11);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = bilerp(t00[c], t01[c], t10[c], t11[c], cy, cx);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(rintf(v[c]), 0.f), 255.f);
}

}  // namespace fs
