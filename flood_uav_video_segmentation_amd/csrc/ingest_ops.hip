// Frame ingest: one decoded uint8 frame -> the network's normalised NCHW fp32 input, one launch (the transform_predict chain of the
// reference, flow/base.py:426-431 -> flow/transform.py:26-106: ToTensor, Resize = cv2.INTER_LINEAR on the uint8 image, Normalize).
// Per output pixel: uint8 taps -> (YUV input: integer conversion to RGB, our definition, include/floodseg_test.h) -> half-pixel
// bilinear resize in the operation order of resize_bilinear_nchw_kernel (lin_coord / bilerp, align_corners = 0, un-contracted) ->
// round half to even, clamp to [0, 255] (the uint8 image cv2.resize stores) -> (x - mean[c]) / std[c] with a true division.
// Nothing in between reaches HBM.
//
// Bandwidth-bound (a 1080 x 1920 RGB frame: 6.2 MB read, 24.7 MB written).  A thread owns four neighbouring output pixels of one row
// and all three channels: three 16-byte stores, one per plane, where the output allows it.  Every tap is loaded from a clamped
// address, unconditionally.  Two shortcuts that change no bit: when the widths are equal the horizontal scale is exactly 1, the
// column coordinate is the integer itself with weights (1, 0), and 1 * a + 0 * b == a for the finite non-negative taps, so the east
// taps are not loaded (1080 -> 1072 rows); when both sizes are equal the same holds for the rows and the pixel is its own value (the
// reference's cv2.resize to the same size is a copy).  The source description and the path up to the stored uint8 image live in
// ingest_src.h, shared with the overlay background of egress_ops.hip.
#include "common.h"
#include "ingest_src.h"
#include "interp.h"
#include "kernels.h"

namespace fs {
namespace {

// MODE 0: both axes resampled; 1: W == w, rows resampled; 2: H == h and W == w
template <bool YUV, int MODE>
__global__ __launch_bounds__(256) void frame_prepare_kernel(IngestSrc s, int h, int w, int ngroups, float sy, float sx, const float* __restrict__ mean,
                                                            const float* __restrict__ std, float* __restrict__ out, int vec_out) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)h * (unsigned)ngroups) return;
    const int oy = (int)(idx / (unsigned)ngroups), x0 = (int)(idx - (unsigned)oy * (unsigned)ngroups) * 4;
    float v[4][3];
    resized4<YUV, MODE>(s, oy, x0, w, sy, sx, v);
    const size_t plane = (size_t)h * w, at = (size_t)oy * w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = mean[c], sd = std[c];
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __fdiv_rn(__fadd_rn(v[i][c], -m), sd);
        float* dst = out + c * plane + at;
        if (vec_out) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < w) dst[i] = o[i];
        }
    }
}

template <bool YUV>
void launch_mode(const IngestSrc& s, int h, int w, const float* mean, const float* std, float* out, hipStream_t st) {
    const int ngroups = cdiv(w, 4);
    const int vec_out = w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const dim3 grid((unsigned)cdiv64((int64_t)h * ngroups, 256));
    const float sy = resize_scale(s.H, h, 0), sx = resize_scale(s.W, w, 0);
    if (s.H == h && s.W == w)
        frame_prepare_kernel<YUV, 2><<<grid, 256, 0, st>>>(s, h, w, ngroups, sy, sx, mean, std, out, vec_out);
    else if (s.W == w)
        frame_prepare_kernel<YUV, 1><<<grid, 256, 0, st>>>(s, h, w, ngroups, sy, sx, mean, std, out, vec_out);
    else
        frame_prepare_kernel<YUV, 0><<<grid, 256, 0, st>>>(s, h, w, ngroups, sy, sx, mean, std, out, vec_out);
}

}  // namespace

int launch_frame_prepare(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int H, int W,
                         const float* mean, const float* std, float* out, int h, int w, hipStream_t st) {
    const IngestSrc s = make_ingest_src(frame, u, v, format, matrix, full_range, H, W);
    if (format == 0)
        launch_mode<false>(s, h, w, mean, std, out, st);
    else
        launch_mode<true>(s, h, w, mean, std, out, st);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
