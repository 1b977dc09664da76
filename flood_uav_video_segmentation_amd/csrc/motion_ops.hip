// Block motion estimation on decoded frames: full-search integer SAD over 16x16 blocks (our definition -- the reference reads the
// encoder's vectors with mvextractor, dataset/flow/extract_motion_vectors.py:47-108; this produces the table that step hands to
// the grid producer, flow_ops.hip::mv_to_grids).  Integer arithmetic only: the result is defined bit for bit (tests/motion_ref.py).
//
// One workgroup (4 waves) owns up to 8 neighbouring blocks of one block row.  It stages the reference strip those blocks can reach
// ((16 + 2R) rows x (128 + 2R' + 4) bytes, R' = R rounded up to 4; pixels outside the frame as zeros that no valid candidate reads)
// and the current blocks into LDS as luma -- an RGB frame is reduced while it is staged, so there is no luma pre-pass and no scratch.
// A wave then searches one block at a time: the current block sits in 64 SGPRs, a lane takes one dy and FOUR neighbouring dx
// (v_qsad_pk_u16_u8: four 4-byte SADs of a sliding 8-byte window per instruction, 16-bit accumulators -- a whole block's SAD is at
// most 256 * 255 = 65280), reading five aligned dwords of a strip row per current row.  The strip's row pitch is an odd number of
// dwords, so lanes of neighbouring dy fall on different banks.  The winner is the minimum of a 64-bit key (cost, |dx| + |dy|, dy, dx)
// over the lanes (__shfl_xor); waves do not share a block, so nothing crosses waves.
// (v_mqsad_u32_u8 would give 32-bit sums, but it is the MASKED form: it leaves out the bytes where the current pixel is 0.)
//
// block_match_modes (the same search, MODES = true) also decides, per block, whether the winner explains the block at all (intra: its
// SAD exceeds the block's own deviation from its mean) and, per frame pair, whether so many blocks are intra that the pair is a scene
// cut; both are expressed as VOID ROWS, vectors that are not there, which mv_owner_kernel (flow_ops.hip) skips.
#include "kernels.h"

namespace fs {
namespace {

constexpr int MB = 16;   // block edge
constexpr int NB = 8;    // blocks per workgroup
constexpr int MAX_R = 32;
constexpr int MAX_PITCH4 = (NB * MB + 2 * MAX_R + 4) / 4;  // dwords per strip row at R = 32
constexpr int MAX_ROWS = MB + 2 * MAX_R;

__device__ inline uint32_t luma_u8(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// luma of pixels (y, x .. x + 3) as the four bytes of a dword, x a multiple of 4; pixels outside the frame give 0.
// whole_dwords: W % 4 == 0 and a 4-byte aligned frame, so the four pixels are inside or outside together and start on a dword.
template <bool RGB>
__device__ inline uint32_t load_luma4(const uint8_t* __restrict__ f, int y, int x, int H, int W, bool whole_dwords) {
    if (y < 0 || y >= H || x + 3 < 0 || x >= W) return 0;
    if (whole_dwords) {
        const size_t p = (size_t)y * W + x;
        if (!RGB) return *reinterpret_cast<const uint32_t*>(f + p);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(f + 3 * p);
        const uint32_t a = q[0], b = q[1], c = q[2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        return luma_u8(a & 255, (a >> 8) & 255, (a >> 16) & 255) | luma_u8(a >> 24, b & 255, (b >> 8) & 255) << 8 |
               luma_u8((b >> 16) & 255, b >> 24, c & 255) << 16 | luma_u8((c >> 8) & 255, (c >> 16) & 255, c >> 24) << 24;
    }
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int xi = x + i;
        if (xi < 0 || xi >= W) continue;
        const size_t p = (size_t)y * W + xi;
        const uint32_t px = RGB ? luma_u8(f[3 * p], f[3 * p + 1], f[3 * p + 2]) : f[p];
        v |= px << (8 * i);
    }
    return v;
}

__device__ inline unsigned long long pack64(uint32_t lo, uint32_t hi) { return (unsigned long long)hi << 32 | lo; }

// sum over the wave of a value every lane holds (the butterfly of the key minimum below); every lane gets the total
__device__ inline uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// MODES adds the inter / intra decision of block_match_modes (include/floodseg_test.h): the block's activity from the 64 dwords of the
// current block that the wave already staged, one dword per lane (v_sad_u8 against 0 for the sum, against the replicated mean for the
// deviation, a wave sum each), and a void row in place of the winner's when sad > activity + intra_bias.  Without MODES none of that
// exists and intra_bias / activity are unused: the <RGB, false> instantiations are block_match's kernel and nothing more.
template <bool RGB, bool MODES>
__global__ __launch_bounds__(256) void block_match_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ ref, int H, int W, int R,
                                                          int lambda, int wb, int nwg_x, int whole_dwords, int* __restrict__ mv,
                                                          int* __restrict__ cost, int intra_bias, int* __restrict__ activity) {
    __shared__ uint32_t s_ref[MAX_ROWS * MAX_PITCH4];
    __shared__ uint32_t s_cur[NB * MB * MB / 4];  // [block][row][4]
    const int by = blockIdx.x / nwg_x, bx0 = (blockIdx.x - by * nwg_x) * NB;
    const int nb = min(NB, wb - bx0);
    const int Rp = (R + 3) & ~3;
    const int pitch4 = (NB * MB + 2 * Rp + 4) / 4;  // odd
    const int rows = MB + 2 * R;
    const int y0 = by * MB - R, x0 = bx0 * MB - Rp;
    for (int i = threadIdx.x; i < rows * pitch4; i += 256) {
        const int r = i / pitch4, c = i - r * pitch4;
        s_ref[i] = load_luma4<RGB>(ref, y0 + r, x0 + 4 * c, H, W, whole_dwords);
    }
    for (int i = threadIdx.x; i < nb * (MB * MB / 4); i += 256)
        s_cur[i] = load_luma4<RGB>(cur, by * MB + ((i >> 2) & 15), (bx0 + (i >> 6)) * MB + 4 * (i & 3), H, W, whole_dwords);
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ng = (Rp + R) / 4 + 1;  // groups of four dx, the first at -Rp: the last one reaches R
    const int ntask = (2 * R + 1) * ng;
    const int dy_lo = max(-R, -by * MB), dy_hi = min(R, H - MB - by * MB);
    for (int b = wave; b < nb; b += 4) {
        const int bx = bx0 + b;
        const int dx_lo = max(-R, -bx * MB), dx_hi = min(R, W - MB - bx * MB);
        uint32_t c[MB][4];  // the current block: wave-uniform, lives in SGPRs
#pragma unroll
        for (int i = 0; i < MB * 4; ++i) c[i >> 2][i & 3] = __builtin_amdgcn_readfirstlane(s_cur[b * (MB * MB / 4) + i]);
        unsigned long long best = ~0ull;
        for (int t0 = 0; t0 < ntask; t0 += 64) {
            const int t = t0 + lane;
            const bool live = t < ntask;
            const int dyi = live ? t / ng : 0, g = live ? t - dyi * ng : 0;
            const uint32_t* p = s_ref + dyi * pitch4 + b * (MB / 4) + g;
            unsigned long long acc = 0;  // four 16-bit sums: dx = -Rp + 4 g + (0, 1, 2, 3)
#pragma unroll
            for (int row = 0; row < MB; ++row) {
                const uint32_t r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3], r4 = p[4];
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r0, r1), c[row][0], acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r1, r2), c[row][1], acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r2, r3), c[row][2], acc);
                acc = __builtin_amdgcn_qsad_pk_u16_u8(pack64(r3, r4), c[row][3], acc);
                p += pitch4;
            }
            const int dy = dyi - R;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int dx = -Rp + 4 * g + i;
                const uint32_t mag = (uint32_t)(abs(dx) + abs(dy));
                const uint32_t cst = (uint32_t)(acc >> (16 * i)) & 0xffffu;
                // cost < 2^17 | |dx| + |dy| <= 64 | dy + 32 | dx + 32: the order of the definition
                const unsigned long long key =
                    (unsigned long long)(cst + (uint32_t)lambda * mag) << 21 | (unsigned long long)(mag << 14 | (uint32_t)(dy + 32) << 7 | (uint32_t)(dx + 32));
                const bool ok = live && dx >= dx_lo && dx <= dx_hi && dy >= dy_lo && dy <= dy_hi;
                best = ok && key < best ? key : best;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        const int dx = (int)(best & 127) - 32, dy = (int)((best >> 7) & 127) - 32;
        const int dst_x = bx * MB + MB / 2, dst_y = by * MB + MB / 2;
        const size_t blk = (size_t)by * wb + bx;
        // (source, w, h, src_x, src_y, dst_x, dst_y): one lane per field
        int v = lane == 0 ? -1 : lane < 3 ? MB : lane == 3 ? dst_x + dx : lane == 4 ? dst_y + dy : lane == 5 ? dst_x : dst_y;
        if (MODES) {
            const uint32_t px = s_cur[b * (MB * MB / 4) + lane];  // four pixels of the block per lane
            const uint32_t mean = (wave_sum(__builtin_amdgcn_sad_u8(px, 0u, 0u)) + 128u) >> 8;  // <= 255
            const int act = (int)wave_sum(__builtin_amdgcn_sad_u8(px, mean * 0x01010101u, 0u));
            const int sad = (int)(best >> 21) - lambda * (int)((best >> 14) & 127);
            if (sad > act + intra_bias) v = lane == 0 ? -1 : lane < 3 ? MB : -MB;  // the void row: no vector was sent for this block
            if (lane == 8 && activity) activity[blk] = act;
        }
        if (lane < 7) mv[blk * 7 + lane] = v;
        if (lane == 7 && cost) cost[blk] = (int)(best >> 21);
    }
}

// The finishing pass of block_match_modes, ONE workgroup: the cut rule needs the pair's intra count before any row is final, so it runs
// behind the search on the stream.  It counts the void rows the search wrote (src_x = -16 is no winner's: a candidate window lies
// inside the frame, so a winner's src_x is >= 8) -- a sum of per-thread integer counts, no atomic and nothing to clear beforehand --
// then, on a cut, makes every row void, and writes stats.  8040 rows at 1080p: 8 rows per thread.
constexpr int FIN_THREADS = 1024;
__global__ __launch_bounds__(FIN_THREADS) void block_match_finish_kernel(int* __restrict__ mv, int blocks, int cut_permille, int* __restrict__ stats) {
    __shared__ int s_part[FIN_THREADS / 64];
    int n = 0;
    for (int i = threadIdx.x; i < blocks; i += FIN_THREADS) n += mv[(size_t)i * 7 + 3] == -MB;
    n = (int)wave_sum((uint32_t)n);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = n;
    __syncthreads();
    int intra = 0;
#pragma unroll
    for (int i = 0; i < FIN_THREADS / 64; ++i) intra += s_part[i];
    const bool is_cut = (long long)intra * 1000 > (long long)cut_permille * blocks;
    if (is_cut)
        for (long long i = threadIdx.x; i < (long long)blocks * 7; i += FIN_THREADS) {
            const int f = (int)(i % 7);
            mv[i] = f == 0 ? -1 : f < 3 ? MB : -MB;
        }
    if (stats && threadIdx.x < 4) stats[threadIdx.x] = threadIdx.x == 0 ? blocks : threadIdx.x == 1 ? intra : threadIdx.x == 2 ? (int)is_cut : 0;
}

// window_weights (include/floodseg_test.h): the per-frame blend weights of one window from the cut flags of its n frame pairs.  ONE
// workgroup of one wave: lane j - 1 reads pair j's flag, the wave's ballot is the set of cut pairs, and lane f writes frame f's row --
// both outputs whole, no atomic, nothing read on the host.  The no-cut row is the expression the fusion kernels evaluate themselves.
struct WindowStats {
    const int* pair[WINDOW_MAX_FRAMES];  // pair[j - 1]: the stats of (j-1 -> j), or nullptr
};
__global__ __launch_bounds__(64) void window_weights_kernel(WindowStats st, int n, float* __restrict__ weights, int* __restrict__ source) {
    const int f = threadIdx.x;
    const bool cut = f < n && st.pair[f] != nullptr && st.pair[f][2] != 0;  // lane f holds pair j = f + 1
    const unsigned long long cuts = __ballot(cut);                          // bit j - 1 <=> pair j is a cut
    if (f >= n) return;
    float wa, wb;
    int src;
    if (cuts == 0) {
        wa = (float)((double)(n - f) / (double)n);
        wb = (float)((double)f / (double)n);
        src = 0;
    } else {
        const int first = __ffsll((long long)cuts), last = 64 - __clzll((long long)cuts);  // smallest and largest cut pair j (1-based)
        const bool prev = f < first || (f < last && 2 * f <= n);
        wa = prev ? 1.f : 0.f;
        wb = prev ? 0.f : 1.f;
        src = f < first ? 1 : f >= last ? 2 : 3;
    }
    weights[2 * f] = wa;
    weights[2 * f + 1] = wb;
    source[f] = src;
}

}  // namespace

int launch_window_weights(const int* const* stats, int n, float* weights, int* source, hipStream_t s) {
    static_assert(WINDOW_MAX_FRAMES == 64, "window_weights_kernel keeps the cut pairs of a window in one 64-lane ballot");
    WindowStats st{};
    for (int j = 0; j < n; ++j) st.pair[j] = stats ? stats[j] : nullptr;
    window_weights_kernel<<<1, 64, 0, s>>>(st, n, weights, source);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_block_match(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int R, int lambda, int* mv, int* cost, hipStream_t s) {
    const int hb = H / MB, wb = W / MB, nwg_x = cdiv(wb, NB);
    const int whole = W % 4 == 0 && (reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(ref)) % 4 == 0;
    const dim3 grid((unsigned)(hb * nwg_x));
    if (channels == 3)
        block_match_kernel<true, false><<<grid, 256, 0, s>>>(cur, ref, H, W, R, lambda, wb, nwg_x, whole, mv, cost, 0, nullptr);
    else
        block_match_kernel<false, false><<<grid, 256, 0, s>>>(cur, ref, H, W, R, lambda, wb, nwg_x, whole, mv, cost, 0, nullptr);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_block_match_modes(const uint8_t* cur, const uint8_t* ref, int H, int W, int channels, int R, int lambda, int intra_bias, int cut_permille,
                             int* mv, int* cost, int* activity, int* stats, hipStream_t s) {
    const int hb = H / MB, wb = W / MB, nwg_x = cdiv(wb, NB);
    const int whole = W % 4 == 0 && (reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(ref)) % 4 == 0;
    const dim3 grid((unsigned)(hb * nwg_x));
    if (channels == 3)
        block_match_kernel<true, true><<<grid, 256, 0, s>>>(cur, ref, H, W, R, lambda, wb, nwg_x, whole, mv, cost, intra_bias, activity);
    else
        block_match_kernel<false, true><<<grid, 256, 0, s>>>(cur, ref, H, W, R, lambda, wb, nwg_x, whole, mv, cost, intra_bias, activity);
    FS_HIP(hipGetLastError());
    // cut_permille 1000 can never cut: without stats to fill there is nothing left to decide
    if (cut_permille < 1000 || stats) {
        block_match_finish_kernel<<<1, FIN_THREADS, 0, s>>>(mv, hb * wb, cut_permille, stats);
        FS_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace fs
