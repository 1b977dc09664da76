// The orthophoto under the flood-extent mosaic (include/floodseg_test.h: ortho_accumulate, ortho_compose).  OUR DEFINITION
// -- the reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.  The rules -- which frame pixel lies under a
// canvas pixel, a frame's rank there, when it replaces the stored one, what compose draws -- are ortho_defs.h's and mosaic_defs.h's
// (__host__ __device__, also run on the CPU by the tests); the image sampled is ingest_src.h's (resized1: the uint8 image the network
// saw, bit for bit what compose_frame draws under that frame's mask); the blend is egress_px.h's.  This file is the launches:
//   ortho_accumulate  one frame per call; one workgroup per 64 x 16 canvas tile as in mosaic_accumulate.  The pose row is read at a
//                     uniform address (it lands in scalar registers); a tile the frame cannot touch returns having read nothing else.
//                     A thread owns its canvas pixels: it reads the rank word (8 B), and only where the frame's rank is strictly
//                     smaller does it fetch the taps, convert, and store rank (8 B) and pixel (4 B).  No atomics; the result is the
//                     minimum over frames, so it depends neither on the order of the calls nor on a repeated call.
//   ortho_compose     one pass over the canvas, 64 x 16 tiles, a thread per four pixels of a row; the palette in LDS as stage_palette
//                     packs it, the class tile with a one-pixel apron in LDS when an edge line is asked for.  Four pixels leave as
//                     three dwords where CW % 4 == 0 and the planes are aligned, as bytes otherwise.
// Every loop bound follows from the arguments; nothing is allocated or synchronised on the host.  Compile with -ffp-contract=off
// (csrc/Makefile): the resize must round as ingest's and egress's do.
#include "egress_px.h"
#include "ingest_src.h"
#include "kernels.h"
#include "map_checks.h"
#include "ortho_defs.h"

namespace fs {

namespace {

constexpr int TILE_W = 64, TILE_H = 16, THREADS = 256;
constexpr int ROWS_PER_STEP = THREADS / TILE_W;  // accumulate: a thread owns column tid & 63 of rows tid >> 6, + 4, + 8, + 12
constexpr int GROUP = 4;                         // compose: a thread owns four pixels of one row: 16 threads a row, 16 rows

// ------------------------------------------------------------------ ortho_accumulate
template <bool YUV, int MODE>
__global__ __launch_bounds__(THREADS) void ortho_accumulate_kernel(IngestSrc s, const long long* __restrict__ pose_row, uint32_t ordinal, int H, int W,
                                                                   int mode, int CH, int CW, int ox, int oy, float sy, float sx,
                                                                   unsigned long long* __restrict__ rank, uint32_t* __restrict__ rgba) {
    const int tid = threadIdx.x, X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * TILE_H;
    const int X1 = min(X0 + TILE_W, CW), Y1 = min(Y0 + TILE_H, CH);
    int64_t pose[mos::POSE_WORDS];  // the same address in every thread: scalar loads
#pragma unroll
    for (int i = 0; i < mos::POSE_WORDS; ++i) pose[i] = pose_row[i];
    if (!mos::pose_votes(pose) || !mos::touches(pose + 6, X0, Y0, X1, Y1, ox, oy, H, W)) return;  // uniform: nothing else is read or written
    const int X = X0 + (tid & (TILE_W - 1));
    if (X >= CW) return;
    for (int Y = Y0 + tid / TILE_W; Y < Y1; Y += ROWS_PER_STEP) {
        int x, y;
        uint64_t mine;
        if (!orth::candidate(pose + 6, X, Y, ox, oy, H, W, mode, ordinal, &x, &y, &mine)) continue;
        const size_t cell = (size_t)Y * CW + X;
        if (!orth::replaces(mine, rank[cell])) continue;  // a loser has read 8 bytes
        float v[3];
        resized1<YUV, MODE>(s, y, x, sy, sx, v);  // (x, y) lies inside the resized image: candidate tested it
        rank[cell] = mine;
        rgba[cell] = orth::pack_rgba((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]);
    }
}

template <bool YUV>
void accumulate_mode(const IngestSrc& s, const long long* pose, uint32_t ordinal, int H, int W, int mode, int CH, int CW, int ox, int oy,
                     unsigned long long* rank, uint32_t* rgba, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(CW, TILE_W), (unsigned)cdiv(CH, TILE_H));
    const float sy = resize_scale(s.H, H, 0), sx = resize_scale(s.W, W, 0);  // as egress_ops.hip takes them
    if (s.H == H && s.W == W)
        ortho_accumulate_kernel<YUV, 2><<<grid, THREADS, 0, st>>>(s, pose, ordinal, H, W, mode, CH, CW, ox, oy, sy, sx, rank, rgba);
    else if (s.W == W)
        ortho_accumulate_kernel<YUV, 1><<<grid, THREADS, 0, st>>>(s, pose, ordinal, H, W, mode, CH, CW, ox, oy, sy, sx, rank, rgba);
    else
        ortho_accumulate_kernel<YUV, 0><<<grid, THREADS, 0, st>>>(s, pose, ordinal, H, W, mode, CH, CW, ox, oy, sy, sx, rank, rgba);
}

// ------------------------------------------------------------------ ortho_compose
// WIDE: CW % 4 == 0 and rgba, cls and out aligned so that a thread's four pixels are one uint4 of rgba, one dword of cls and three
// dwords of out.  EDGE: edge_set != 0 (and cls given): the class tile with its apron goes through LDS.
template <bool WIDE, bool EDGE>
__global__ __launch_bounds__(THREADS) void ortho_compose_kernel(const uint32_t* __restrict__ rgba, const uint8_t* __restrict__ cls,
                                                                const uint8_t* __restrict__ palette, int K, uint32_t edge_set, uint32_t fill, int CH, int CW,
                                                                uint8_t* __restrict__ out) {
    __shared__ uint32_t pal[256];
    __shared__ uint8_t tile[EDGE ? TILE_H + 2 : 1][EDGE ? TILE_W + 2 : 1];
    const int tid = threadIdx.x, X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * TILE_H;
    if (cls) stage_palette(pal, palette, K);
    if (EDGE) {
        for (int i = tid; i < (TILE_H + 2) * (TILE_W + 2); i += THREADS) {
            const int ty = i / (TILE_W + 2), tx = i - ty * (TILE_W + 2);
            const int Y = Y0 + ty - 1, X = X0 + tx - 1;
            tile[ty][tx] = (Y >= 0 && Y < CH && X >= 0 && X < CW) ? cls[(size_t)Y * CW + X] : (uint8_t)orth::UNSEEN;  // outside the canvas: no edge
        }
    }
    __syncthreads();
    const int ty = tid / (TILE_W / GROUP), tx = (tid % (TILE_W / GROUP)) * GROUP;
    const int Y = Y0 + ty, X = X0 + tx;
    if (Y >= CH || X >= CW) return;
    const size_t cell = (size_t)Y * CW + X;
    uint32_t px[GROUP], k[GROUP];
    if (WIDE) {
        const uint4 q = *reinterpret_cast<const uint4*>(rgba + cell);
        px[0] = q.x, px[1] = q.y, px[2] = q.z, px[3] = q.w;
        const uint32_t c = cls ? *reinterpret_cast<const uint32_t*>(cls + cell) : 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < GROUP; ++i) k[i] = (c >> (8 * i)) & 255u;
    } else {
#pragma unroll
        for (int i = 0; i < GROUP; ++i) {
            const bool in = X + i < CW;
            px[i] = in ? rgba[cell + i] : 0u;
            k[i] = (in && cls) ? cls[cell + i] : orth::UNSEEN;
        }
    }
    uint32_t o[GROUP][3];
#pragma unroll
    for (int i = 0; i < GROUP; ++i) {
        const uint32_t under = orth::under_rgb(px[i], fill);
        uint32_t A = 0u, e = 0u;
        if (cls && orth::takes_colour(k[i], K)) {  // k < K <= 256: inside pal[], which is staged only with a class plane (K = 256 takes 255 too)
            e = pal[k[i]];
            A = e >> 24;
            if (EDGE && orth::on_edge(k[i], edge_set, tile[ty][tx + i + 1], tile[ty + 2][tx + i + 1], tile[ty + 1][tx + i], tile[ty + 1][tx + i + 2])) A = 255u;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[i][c] = (uint32_t)blend255((int)A, (int)((e >> (8 * c)) & 255u), (int)((under >> (8 * c)) & 255u));
    }
    uint8_t* dst = out + cell * 3;
    if (WIDE) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        d[0] = pack4(o[0][0], o[0][1], o[0][2], o[1][0]);
        d[1] = pack4(o[1][1], o[1][2], o[2][0], o[2][1]);
        d[2] = pack4(o[2][2], o[3][0], o[3][1], o[3][2]);
    } else {
#pragma unroll
        for (int i = 0; i < GROUP; ++i)
            if (X + i < CW) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[3 * i + c] = (uint8_t)o[i][c];
            }
    }
}

}  // namespace

int launch_ortho_accumulate(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW,
                            const long long* pose, uint32_t ordinal, int H, int W, int mode, int CH, int CW, int ox, int oy, unsigned long long* rank,
                            uint32_t* rgba, hipStream_t s) {
    FS_REQUIRE(frame && pose && rank && rgba, "ortho_accumulate: null pointer");
    FS_TRY(check_frame_source("ortho_accumulate", u, v, format, matrix, full_range, FH, FW));
    FS_TRY(check_mask_on_canvas("ortho_accumulate", 1, H, W, CH, CW, ox, oy));
    FS_REQUIRE(mode == orth::MODE_CENTRE || mode == orth::MODE_LATEST, "ortho_accumulate: mode must be 0 (centre) or 1 (latest), got mode=%d", mode);
    FS_REQUIRE(ordinal != orth::ORDINAL_NONE, "ortho_accumulate: ordinal=%u is reserved", ordinal);
    FS_REQUIRE(aligned(pose, 8), "ortho_accumulate: pose is not aligned to 8 bytes");
    FS_REQUIRE(aligned(rank, 8), "ortho_accumulate: rank is not aligned to 8 bytes");
    FS_REQUIRE(aligned(rgba, 4), "ortho_accumulate: rgba is not aligned to 4 bytes");
    const IngestSrc src = make_ingest_src(frame, u, v, format, matrix, full_range, FH, FW);
    if (format == 0)
        accumulate_mode<false>(src, pose, ordinal, H, W, mode, CH, CW, ox, oy, rank, rgba, s);
    else
        accumulate_mode<true>(src, pose, ordinal, H, W, mode, CH, CW, ox, oy, rank, rgba, s);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_ortho_compose(const uint32_t* rgba, const uint8_t* cls, const uint8_t* palette, int K, uint32_t edge_set, uint32_t fill, int CH, int CW,
                         uint8_t* out, hipStream_t s) {
    FS_REQUIRE(rgba && out, "ortho_compose: null pointer");
    FS_REQUIRE(!cls || palette, "ortho_compose: null pointer (a class plane without a palette)");
    FS_TRY(check_sides("ortho_compose", "the canvas", 1, CH, CW));
    FS_REQUIRE(K >= 1 && K <= 256, "ortho_compose: palette must hold 1..256 classes, got %d", K);
    const int edge_bits = K < 32 ? K : 32;
    FS_REQUIRE(edge_bits == 32 || (edge_set >> edge_bits) == 0u, "ortho_compose: edge_set=0x%x names a class at or above %d", edge_set, edge_bits);
    FS_REQUIRE(fill < (1u << 24), "ortho_compose: fill=0x%x is not r | g << 8 | b << 16", fill);
    FS_REQUIRE(aligned(rgba, 4), "ortho_compose: rgba is not aligned to 4 bytes");
    const dim3 grid((unsigned)cdiv(CW, TILE_W), (unsigned)cdiv(CH, TILE_H));
    const bool wide = CW % 4 == 0 && aligned(rgba, 16) && aligned(out, 4) && (!cls || aligned(cls, 4));
    const bool edge = cls && edge_set != 0u;
    if (wide && edge)
        ortho_compose_kernel<true, true><<<grid, THREADS, 0, s>>>(rgba, cls, palette, K, edge_set, fill, CH, CW, out);
    else if (wide)
        ortho_compose_kernel<true, false><<<grid, THREADS, 0, s>>>(rgba, cls, palette, K, edge_set, fill, CH, CW, out);
    else if (edge)
        ortho_compose_kernel<false, true><<<grid, THREADS, 0, s>>>(rgba, cls, palette, K, edge_set, fill, CH, CW, out);
    else
        ortho_compose_kernel<false, false><<<grid, THREADS, 0, s>>>(rgba, cls, palette, K, edge_set, fill, CH, CW, out);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
