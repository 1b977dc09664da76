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
//
// guide_vectors (further down; rules: guide_defs.h) passes over a finished table with global_motion's camera model: void rows take the
// camera's vector, vectors that disagree with it are replaced -- in evidence mode only if the camera's window explains the block no
// worse, measured with the luma and the wave sum of this file.
#include "kernels.h"
#include "guide_defs.h"

namespace fs {
namespace {

constexpr int MB = 16;   // block edge
constexpr int NB = 8;    // blocks per workgroup
constexpr int MAX_R = 32;
constexpr int MAX_PITCH4 = (NB * MB + 2 * MAX_R + 4) / 4;  // dwords per strip row at R = 32
constexpr int MAX_ROWS = MB + 2 * MAX_R;

__device__ inline uint32_t luma_u8(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// luma of pixels (y, x .. x + 3) as the four bytes of a dword; pixels outside the frame give 0.
// whole_dwords: W % 4 == 0, a 4-byte aligned frame AND x a multiple of 4, so the four pixels are inside or outside together and start
// on a dword (the search's staging; the guide kernel's cur block).  Without it x is ANY column and the pixels are read byte by byte:
// guide_vectors_kernel reads the guide's window of ref that way, at x + pdx.
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

// guide_vectors (include/floodseg_test.h; the rules: guide_defs.h): the table of a frame pair guided by global_motion's camera model.
// One wave per block, four blocks per workgroup; blockIdx.y is the pair.  Every lane computes the same prediction, class and decision
// from the row (one word per lane, broadcast) and the pair's model row, so every branch is wave-uniform.  Only with EVIDENCE, and only
// the wave whose row is an outlier with an available guide, touches the frames: four pixels of a block row per lane -- cur through
// load_luma4's dword path where the frame allows, the guide's window of ref at whatever byte it starts on -- v_sad_u8 and one wave
// sum.  The <*, false> instantiation holds no frame code.  out may be mv: a row is read and written by its own wave alone, read
// first.  The counts go through an LDS tally per workgroup and leave with one 64-bit atomic per non-zero cell.
template <bool RGB, bool EVIDENCE>
__global__ __launch_bounds__(256) void guide_vectors_kernel(const int* mv, const long long* __restrict__ model, int blocks, int wb, int FH, int FW,
                                                            int fill_void, long long outlier_q20, const uint8_t* __restrict__ cur,
                                                            const uint8_t* __restrict__ ref, int whole_dwords, const int* __restrict__ cost, int penalty,
                                                            int guide_bias, int* out, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t s_tally[guide::COUNT_WORDS];
    if (threadIdx.x < guide::COUNT_WORDS) s_tally[threadIdx.x] = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int f = blockIdx.y, i = (int)blockIdx.x * 4 + wave;
    if (i < blocks) {
        const int by = i / wb, bx = i - by * wb;
        const int cx = bx * MB + MB / 2, cy = by * MB + MB / 2;
        const size_t blk = (size_t)f * blocks + i;
        const int mine = lane < guide::ROW_WORDS ? mv[blk * guide::ROW_WORDS + lane] : 0;
        int32_t r[guide::ROW_WORDS];
#pragma unroll
        for (int k = 0; k < guide::ROW_WORDS; ++k) r[k] = __shfl(mine, k, 64);
        int64_t M[mos::MODEL_WORDS];
#pragma unroll
        for (int k = 0; k < mos::MODEL_WORDS; ++k) M[k] = model[(size_t)f * mos::MODEL_WORDS + k];
        const bool guided = guide::pair_guides(M);  // status and bounds before any product
        int64_t gx = 0, gy = 0, pdx = 0, pdy = 0;
        bool avail = false;
        if (guided) {
            guide::predict(M, cx, cy, &gx, &gy, &pdx, &pdy);
            avail = guide::available(pdx, pdy, cx, cy, FH, FW);
        }
        int dx, dy;
        const int cls = guide::classify(r, cx, cy, &dx, &dy);
        const bool outlier = guided && cls == guide::ROW_VECTOR && guide::is_outlier(dx, dy, gx, gy, outlier_q20);
        bool ask;
        int decision = guide::decide(cls, outlier, guided, avail, fill_void, &ask);
        if (EVIDENCE && ask) {  // available: |pdx|, |pdy| <= 32 and the window lies inside the frame
            const size_t frame = (size_t)f * FH * FW * (RGB ? 3 : 1);
            const int y = cy - MB / 2 + (lane >> 2), x = cx - MB / 2 + 4 * (lane & 3);
            const uint32_t a = load_luma4<RGB>(cur + frame, y, x, FH, FW, whole_dwords != 0);
            const uint32_t b = load_luma4<RGB>(ref + frame, y + (int)pdy, x + (int)pdx, FH, FW, false);
            const int64_t cost_g = guide::guide_cost((int64_t)wave_sum(__builtin_amdgcn_sad_u8(a, b, 0u)), penalty, pdx, pdy);
            if (!guide::evidence_replaces(cost_g, cost[blk], guide_bias)) decision = guide::KEEP;
        }
        if (lane < guide::ROW_WORDS) out[blk * guide::ROW_WORDS + lane] = guide::out_word(decision, lane, mine, cx, cy, pdx, pdy);
        if (lane == 0) {
            atomicAdd(&s_tally[guide::C_BLOCKS], 1u);
            if (cls == guide::ROW_VOID) atomicAdd(&s_tally[guide::C_VOID], 1u);
            if (cls == guide::ROW_FOREIGN) atomicAdd(&s_tally[guide::C_FOREIGN], 1u);
            if (outlier) atomicAdd(&s_tally[guide::C_OUTLIERS], 1u);
            if (decision == guide::FILL) atomicAdd(&s_tally[guide::C_FILLED], 1u);
            if (decision == guide::REPLACE) atomicAdd(&s_tally[guide::C_REPLACED], 1u);
            if (decision == guide::DROP) atomicAdd(&s_tally[guide::C_DROPPED], 1u);
            if (decision == guide::KEEP) atomicAdd(&s_tally[guide::C_KEPT], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < guide::COUNT_WORDS && s_tally[threadIdx.x] != 0u)
        atomicAdd(counts + (size_t)f * guide::COUNT_WORDS + threadIdx.x, (unsigned long long)s_tally[threadIdx.x]);
}

// counts is cleared by a kernel, not a memset node: n * 8 <= 512 words, one thread each
__global__ __launch_bounds__(512) void guide_clear_kernel(unsigned long long* __restrict__ counts, int words) {
    if ((int)threadIdx.x < words) counts[threadIdx.x] = 0ull;
}

bool aligned_to(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

int launch_guide_vectors(const int32_t* mv, const long long* model, int n, int FH, int FW, int fill_void, long long outlier_q20, const uint8_t* cur,
                         const uint8_t* ref, int channels, const int32_t* cost, int penalty, int guide_bias, int32_t* out, long long* counts, hipStream_t s) {
    static_assert(mos::MAX_FRAMES * guide::COUNT_WORDS <= 512, "guide_clear_kernel clears counts with one workgroup of 512");
    FS_REQUIRE(mv && model && out && counts, "guide_vectors: null pointer (mv %p, model %p, out %p, counts %p)", (const void*)mv, (const void*)model,
               (void*)out, (void*)counts);
    FS_REQUIRE(n >= 1 && n <= mos::MAX_FRAMES, "guide_vectors: n must be 1..%d, got %d", mos::MAX_FRAMES, n);
    FS_REQUIRE(FH >= guide::MIN_SIDE && FH <= mos::MAX_SIDE && FW >= guide::MIN_SIDE && FW <= mos::MAX_SIDE,
               "guide_vectors: the frame must be %d..%d pixels a side, got %dx%d", guide::MIN_SIDE, mos::MAX_SIDE, FH, FW);
    FS_REQUIRE(outlier_q20 >= -1 && outlier_q20 <= guide::MAX_OUTLIER_Q20, "guide_vectors: outlier_q20 must be -1 (off) or 0..%lld, got %lld",
               (long long)guide::MAX_OUTLIER_Q20, outlier_q20);
    FS_REQUIRE(penalty >= 0 && penalty <= guide::MAX_PENALTY, "guide_vectors: penalty must be 0..%d, got %d", guide::MAX_PENALTY, penalty);
    FS_REQUIRE(guide_bias >= 0 && guide_bias <= guide::MAX_BIAS, "guide_vectors: guide_bias must be 0..%d, got %d", guide::MAX_BIAS, guide_bias);
    const bool evidence = cur && ref && cost;
    FS_REQUIRE(evidence || (!cur && !ref && !cost), "guide_vectors: cur, ref and cost come together or not at all (cur %p, ref %p, cost %p)",
               (const void*)cur, (const void*)ref, (const void*)cost);
    FS_REQUIRE(channels == 1 || channels == 3, "guide_vectors: channels must be 1 (luma) or 3 (RGB), got %d", channels);
    FS_REQUIRE(aligned_to(mv, 4) && aligned_to(out, 4) && aligned_to(cost, 4), "guide_vectors: mv, out or cost is not aligned to 4 bytes");
    FS_REQUIRE(aligned_to(model, 8) && aligned_to(counts, 8), "guide_vectors: model or counts is not aligned to 8 bytes");
    const int wb = FW / MB, blocks = (FH / MB) * wb;
    guide_clear_kernel<<<1, 512, 0, s>>>(reinterpret_cast<unsigned long long*>(counts), n * guide::COUNT_WORDS);
    FS_HIP(hipGetLastError());
    const dim3 grid((unsigned)cdiv(blocks, 4), (unsigned)n);
    const int whole = FW % 4 == 0 && aligned_to(cur, 4);
    unsigned long long* tally = reinterpret_cast<unsigned long long*>(counts);
    if (!evidence)
        guide_vectors_kernel<false, false><<<grid, 256, 0, s>>>(mv, model, blocks, wb, FH, FW, fill_void, outlier_q20, nullptr, nullptr, 0, nullptr, 0, 0, out, tally);
    else if (channels == 3)
        guide_vectors_kernel<true, true><<<grid, 256, 0, s>>>(mv, model, blocks, wb, FH, FW, fill_void, outlier_q20, cur, ref, whole, cost, penalty, guide_bias, out, tally);
    else
        guide_vectors_kernel<false, true><<<grid, 256, 0, s>>>(mv, model, blocks, wb, FH, FW, fill_void, outlier_q20, cur, ref, whole, cost, penalty, guide_bias, out, tally);
    FS_HIP(hipGetLastError());
    return 0;
}

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
