// Region identity across frames (include/floodseg_test.h: region_links, region_links_mc, region_tracks).  OUR
// DEFINITION -- the reference emits hard masks only.  Opt-in passes behind region_table: nothing on the shipped routes calls them.
//   region_links    index planes + tables of consecutive frames -> per row its best-overlapping row of the other frame, both ways
//   region_links_mc the same with the frame before gathered at every pixel's SOURCE under the block matcher's vectors
//   region_tracks   the links -> a track id per region: continued from the frame before, or born
// Integers throughout, and every result is a function of the inputs alone: the pair counts are integer sums, the best partner is an
// integer maximum, and whether the pair table overflows depends on the number of distinct pairs only (track_defs.h, probe_slot).
// The packing, the probe sequence and the continue / born rule are track_defs.h's (__host__ __device__, also run on the CPU by the
// tests).  Every loop has a static bound, stated at the loop; nothing waits on another workgroup, allocates or synchronises.
#include "kernels.h"
#include "track_defs.h"

#include <algorithm>

namespace fs {

namespace {

// the workspace of one frame pair, in 8-byte words: keys [max_pairs], best_back [R], best_fwd [R], one word of two 32-bit figures
// (pairs stored, overflow), then the 32-bit pair counts [max_pairs] (max_pairs is even)
struct PairSpace {
    unsigned long long *keys, *best_back, *best_fwd;
    unsigned *flags, *count;
};
__host__ __device__ inline size_t pair_words(int R, unsigned max_pairs) { return (size_t)max_pairs + 2 * (size_t)R + 1 + max_pairs / 2; }
__device__ __forceinline__ PairSpace pair_space(unsigned long long* ws, int f, int R, unsigned max_pairs) {
    unsigned long long* p = ws + (size_t)f * pair_words(R, max_pairs);
    PairSpace s;
    s.keys = p;
    s.best_back = p + max_pairs;
    s.best_fwd = s.best_back + R;
    s.flags = reinterpret_cast<unsigned*>(s.best_fwd + R);
    s.count = s.flags + 2;
    return s;
}

__global__ __launch_bounds__(256) void track_zero_kernel(unsigned long long* __restrict__ p, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) p[i] = 0ull;
}

__device__ __forceinline__ int rows_of(const long long* counts, int R) {  // rows written, as far as memory safety allows
    const long long c = counts[1];
    return (int)(c < 0 ? 0 : (c > R ? R : c));
}

// ------------------------------------------------------------------ pass 0 (region_links_mc): one packed shift per block
// What the compensated overlap pass needs on top of the in-place one's arguments; empty for the in-place instantiation.
template <bool MC>
struct Motion {};
template <>
struct Motion<true> {
    const unsigned* shifts;  // [n][hb * wb]: trk::mc_row_shift of every table row, behind the pair tables in the workspace
    const int* pair_stats;   // [n][4], block_match_modes' stats, or nullptr
    int FH, FW, hb, wb;      // the decoded frame and its blocks
};

// One table row per thread, grid = (blocks / 256, frames): 28 bytes in, 4 bytes out, so that the overlap pass reads one cache-resident
// dword per pixel (the same one for 16 neighbours) and not a row.  A cut pair's flag word is set here, after the zeroing: the overlap
// pass skips that pair and the unpack pass writes it like an overflowing one.
__global__ __launch_bounds__(256) void track_shift_kernel(const int* __restrict__ mv, const int* __restrict__ pair_stats, const int* prev_index, int H, int W,
                                                          int FH, int FW, int blocks, int R, unsigned max_pairs, unsigned long long* ws,
                                                          unsigned* __restrict__ shifts) {
    const int f = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k < blocks) shifts[(size_t)f * blocks + k] = trk::mc_row_shift(mv + ((size_t)f * blocks + k) * trk::MC_VECTOR_INTS, H, W, FH, FW);
    if (k == 0 && pair_stats && (f || prev_index)) {
        const unsigned cut = trk::cut_flag(pair_stats + 4 * (size_t)f);
        if (cut) pair_space(ws, f, R, max_pairs).flags[1] = cut;
    }
}

// ------------------------------------------------------------------ pass 1: the overlap of every (a, b) pair
// grid = (256-pixel row pieces, rows, frames), as region_accumulate_kernel: a wave is 64 consecutive pixels of one row.  Runs of equal
// (a, b) inside the wave are found with a ballot, and the run's first lane inserts the pair and adds the run's length: one insertion
// per run, not per pixel.  Frame 0 without a frame before it does nothing (the whole workgroup leaves before any cross-lane op).
// MC: a is gathered at the pixel's source (track_defs.h: the block column is the thread's own, the block row the row's; the packed shift
// of the block comes from pass 0), -1 where the source lies outside the mask; runs of equal (a, b) are runs whatever the sources.  A
// cut pair does nothing.
template <bool MC>
__global__ __launch_bounds__(256) void track_overlap_kernel(const int* __restrict__ index, const long long* __restrict__ table,
                                                            const long long* __restrict__ counts, const int* __restrict__ prev_index,
                                                            const long long* __restrict__ prev_table, const long long* __restrict__ prev_counts,
                                                            int H, int W, int R, unsigned max_pairs, unsigned long long* ws, Motion<MC> mo) {
    const int f = blockIdx.z;
    const size_t HW = (size_t)H * W;
    if (f == 0 && !prev_index) return;
    if constexpr (MC) {
        if (mo.pair_stats && trk::cut_flag(mo.pair_stats + 4 * (size_t)f)) return;
    }
    const int* ia = f ? index + (size_t)(f - 1) * HW : prev_index;
    const long long* ta = f ? table + (size_t)(f - 1) * R * 10 : prev_table;
    const int rows_a = rows_of(f ? counts + 2 * (size_t)(f - 1) : prev_counts, R);
    const int* ib = index + (size_t)f * HW;
    const long long* tb = table + (size_t)f * R * 10;
    const int rows_b = rows_of(counts + 2 * (size_t)f, R);
    const PairSpace sp = pair_space(ws, f, R, max_pairs);
    const int x = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = x < W;
    const int xc = min(x, W - 1);
    int bx = 0;
    const unsigned* shifts = nullptr;
    if constexpr (MC) {
        bx = trk::mc_block(xc, W, mo.FW);
        shifts = mo.shifts + (size_t)f * mo.hb * mo.wb;
    }
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const size_t i = (size_t)y * W + xc;
        int a;
        if constexpr (MC) {
            const int by = trk::mc_block(y, H, mo.FH);
            const unsigned shift = by < mo.hb && bx < mo.wb ? shifts[(size_t)by * mo.wb + bx] : 0u;  // the remainder strip: no shift
            int ys, xs;
            a = trk::mc_source(y, xc, shift, H, W, &ys, &xs) ? ia[(size_t)ys * W + xs] : -1;
        } else {
            a = ia[i];
        }
        const int b = ib[i];
        const bool ok = valid && a >= 0 && a < rows_a && b >= 0 && b < rows_b;  // background and rows past the cap take no part
        const int ka = ok ? a : -1, kb = ok ? b : -1;
        const int pa = __shfl_up(ka, 1), pb = __shfl_up(kb, 1);
        const unsigned long long heads = __ballot(lane == 0 || pa != ka || pb != kb);
        const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const int end = above ? __ffsll((long long)above) - 1 : 64;  // the run of a head lane is [lane, end)
        if (((heads >> lane) & 1ull) && ok && ta[(size_t)a * 10] == tb[(size_t)b * 10]) {  // the same class: column 0 of both rows
            const unsigned long long key = trk::pack_key(a, b);
            bool stored = false;
            for (unsigned p = 0; p < max_pairs && !stored; ++p) {  // bounded: max_pairs probes visit every slot once
                const unsigned slot = trk::probe_slot(key, p, max_pairs);
                unsigned long long cur = __hip_atomic_load(&sp.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == 0ull) {
                    cur = atomicCAS(&sp.keys[slot], 0ull, key);
                    if (cur == 0ull) cur = key;
                }
                if (cur == key) {
                    atomicAdd(&sp.count[slot], (unsigned)(end - lane));
                    stored = true;
                }
            }
            if (!stored) atomicOr(&sp.flags[1], 1u);  // every slot holds another pair
        }
    }
}

// ------------------------------------------------------------------ pass 2: per row the best partner; one slot per thread
__global__ __launch_bounds__(256) void track_best_kernel(const int* __restrict__ prev_index, int R, unsigned max_pairs, unsigned long long* ws) {
    const int f = blockIdx.y;
    if (f == 0 && !prev_index) return;
    const PairSpace sp = pair_space(ws, f, R, max_pairs);
    const unsigned slot = blockIdx.x * 256 + threadIdx.x;  // < max_pairs: the grid is max_pairs / 256 workgroups, or one of max_pairs threads
    const unsigned long long key = slot < max_pairs ? sp.keys[slot] : 0ull;
    if (key) {
        const int a = trk::key_a(key), b = trk::key_b(key);  // < R: only such pairs were inserted
        const unsigned c = sp.count[slot];
        atomicMax(&sp.best_back[b], trk::pack_best(c, a));
        atomicMax(&sp.best_fwd[a], trk::pack_best(c, b));
    }
    const int stored = __syncthreads_count(key != 0ull);
    if (threadIdx.x == 0 && stored) atomicAdd(&sp.flags[0], (unsigned)stored);
}

// ------------------------------------------------------------------ pass 3: the packed cells become back / fwd; one row per thread
__global__ __launch_bounds__(256) void track_unpack_kernel(int R, unsigned max_pairs, int min_overlap, unsigned long long* ws, int* __restrict__ back,
                                                           int* __restrict__ fwd, long long* __restrict__ link_counts) {
    const int f = blockIdx.y;
    const PairSpace sp = pair_space(ws, f, R, max_pairs);
    const unsigned word = sp.flags[1];
    const bool overflow = word != 0u;  // the pair table overflowed, or (region_links_mc) the pair is a cut: no links either way
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) {
        link_counts[2 * (size_t)f] = sp.flags[0];
        link_counts[2 * (size_t)f + 1] = trk::link_flags(word);
    }
    if (r >= R) return;
    const size_t at = ((size_t)f * R + r) * 2;
    trk::unpack_link(sp.best_back[r], min_overlap, overflow, &back[at], &back[at + 1]);
    trk::unpack_link(sp.best_fwd[r], min_overlap, overflow, &fwd[at], &fwd[at + 1]);
}

// ------------------------------------------------------------------ pass 4: track ids
// The rows at and behind counts[f][1] are (-1, -1, -1, 0): one row per thread, any number of workgroups.  The ids kernel never touches
// these rows, so the two launches write disjoint rows.
__global__ __launch_bounds__(256) void track_fill_kernel(const long long* __restrict__ counts, int R, long long* __restrict__ tracks) {
    const int f = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R || r < rows_of(counts + 2 * (size_t)f, R)) return;
    long long* row = tracks + ((size_t)f * R + r) * 4;
    row[0] = row[1] = row[2] = -1;
    row[3] = 0;
}

// ONE workgroup walks the frames in order: frame f needs frame f - 1's ids, so the frames are a chain.  Inside a frame the rows that
// exist go in pieces of 1024: the continue / born decision, an exclusive scan of the born flags (a ballot per wave, the 16 wave totals
// through LDS) on top of the running count, then the ids.  Both loops are bounded: n frames, ceil(rows / 1024) <= ceil(R / 1024)
// pieces.  tracks is read (frame f - 1) and written (frame f) by this one workgroup; the barrier at the end of a frame orders the two.
__global__ __launch_bounds__(trk::TRACK_BLOCK) void track_ids_kernel(const int* __restrict__ back, const int* __restrict__ fwd,
                                                                     const long long* __restrict__ counts, const long long* prev_tracks, int n, int R,
                                                                     long long* state, long long* tracks) {
    __shared__ int wave_total[trk::TRACK_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long next = state[0];
    for (int f = 0; f < n; ++f) {
        const long long* pt = f ? tracks + (size_t)(f - 1) * R * 4 : prev_tracks;
        const int* bk = back + (size_t)f * R * 2;
        const int* fw = fwd + (size_t)f * R * 2;
        const int rows = rows_of(counts + 2 * (size_t)f, R);
        long long* out = tracks + (size_t)f * R * 4;
        for (int base = 0; base < rows; base += trk::TRACK_BLOCK) {  // rows <= R; the same for every thread
            const int r = base + tid;
            const bool has = r < rows;
            bool cont = false;
            int a = -1, ov = 0;
            long long pid = -1, ppar = -1;
            if (has) {
                a = bk[2 * (size_t)r];
                ov = bk[2 * (size_t)r + 1];
                if (a < 0 || a >= R) {  // a link the caller made up: no row before it
                    a = -1;
                    ov = 0;
                }
                if (a >= 0) {
                    if (pt) {
                        pid = pt[4 * (size_t)a];
                        ppar = pt[4 * (size_t)a + 1];
                    }
                    cont = trk::continues(a, fw[2 * (size_t)a], r, pid);
                }
            }
            const bool born = has && !cont;
            const unsigned long long bits = __ballot(born);
            if (lane == 0) wave_total[wave] = __popcll(bits);
            __syncthreads();
            int before = __popcll(bits & ((1ull << lane) - 1ull)), all = 0;
            for (int v = 0; v < trk::TRACK_BLOCK / 64; ++v) {
                const int t = wave_total[v];
                if (v < wave) before += t;
                all += t;
            }
            __syncthreads();
            if (has) {
                long long* row = out + 4 * (size_t)r;
                row[0] = cont ? pid : next + before;
                row[1] = cont ? ppar : pid;  // a continued region keeps its track's parent; a born one names its best predecessor's track
                row[2] = a;
                row[3] = ov;
            }
            next += all;
        }
        __syncthreads();
    }
    if (tid == 0) state[0] = next;
}

int track_sizes(const char* what, int n, int max_regions) {
    FS_REQUIRE(n >= 1 && n <= 65535, "%s: 1..65535 frames, got n=%d", what, n);
    FS_REQUIRE(max_regions >= 1 && max_regions <= 65536, "%s: max_regions=%d out of range (1..65536)", what, max_regions);
    return 0;
}

// what both link ops refuse, in region_links' order; `what` names the op in the message
int links_checks(const char* what, const void* index, const void* table, const void* counts, const void* prev_index, const void* prev_table,
                 const void* prev_counts, int n, int H, int W, int max_regions, int max_pairs, int min_overlap, const void* back, const void* fwd,
                 const void* link_counts, const void* workspace) {
    FS_REQUIRE(index && table && counts && back && fwd && link_counts && workspace, "%s: null pointer", what);
    FS_REQUIRE(H >= 1 && W >= 1, "%s: sizes must be >= 1, got %dx%d", what, H, W);
    if (int rc = track_sizes(what, n, max_regions)) return rc;
    FS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 1, "%s: a frame of 2^31 - 1 pixels or more (%dx%d)", what, H, W);
    FS_REQUIRE(max_pairs >= trk::MIN_PAIRS && max_pairs <= trk::MAX_PAIRS && (max_pairs & (max_pairs - 1)) == 0,
               "%s: max_pairs=%d must be a power of two in %d..%d", what, max_pairs, trk::MIN_PAIRS, trk::MAX_PAIRS);
    FS_REQUIRE(min_overlap >= 1, "%s: min_overlap=%d must be >= 1", what, min_overlap);
    const int given = (prev_index != nullptr) + (prev_table != nullptr) + (prev_counts != nullptr);
    FS_REQUIRE(given == 0 || given == 3, "%s: the previous frame is given in part (prev_index, prev_table and prev_counts go together)", what);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: the workspace is not aligned to 8 bytes", what);
    return 0;
}

// the launches both link ops share: everything but the overlap pass (and region_links_mc's pass 0 in front of it)
void launch_zero(unsigned long long* ws, int n, int max_regions, int max_pairs, hipStream_t s) {
    const size_t words = (size_t)n * pair_words(max_regions, (unsigned)max_pairs);
    hipLaunchKernelGGL(track_zero_kernel, dim3((unsigned)std::min<size_t>((words + 255) / 256, 1u << 20)), dim3(256), 0, s, ws, words);
}
void launch_best_unpack(const int* prev_index, int n, int max_regions, int max_pairs, int min_overlap, unsigned long long* ws, int* back, int* fwd,
                        long long* link_counts, hipStream_t s) {
    hipLaunchKernelGGL(track_best_kernel, dim3((unsigned)cdiv(max_pairs, 256), (unsigned)n), dim3(256), 0, s, prev_index, max_regions, (unsigned)max_pairs, ws);
    hipLaunchKernelGGL(track_unpack_kernel, dim3((unsigned)cdiv(max_regions, 256), (unsigned)n), dim3(256), 0, s, max_regions, (unsigned)max_pairs,
                       min_overlap, ws, back, fwd, link_counts);
}

}  // namespace

int launch_region_links(const int* index, const long long* table, const long long* counts, const int* prev_index, const long long* prev_table,
                        const long long* prev_counts, int n, int H, int W, int max_regions, int max_pairs, int min_overlap, int* back, int* fwd,
                        long long* link_counts, void* workspace, hipStream_t s) {
    if (int rc = links_checks("region_links", index, table, counts, prev_index, prev_table, prev_counts, n, H, W, max_regions, max_pairs, min_overlap, back,
                              fwd, link_counts, workspace))
        return rc;
    unsigned long long* ws = static_cast<unsigned long long*>(workspace);
    launch_zero(ws, n, max_regions, max_pairs, s);
    hipLaunchKernelGGL(track_overlap_kernel<false>, dim3((unsigned)cdiv(W, 256), (unsigned)std::min(H, 65535), (unsigned)n), dim3(256), 0, s, index, table,
                       counts, prev_index, prev_table, prev_counts, H, W, max_regions, (unsigned)max_pairs, ws, Motion<false>{});
    launch_best_unpack(prev_index, n, max_regions, max_pairs, min_overlap, ws, back, fwd, link_counts, s);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_region_links_mc(const int* index, const long long* table, const long long* counts, const int* prev_index, const long long* prev_table,
                           const long long* prev_counts, const int* mv, const int* pair_stats, int n, int H, int W, int frame_h, int frame_w,
                           int max_regions, int max_pairs, int min_overlap, int* back, int* fwd, long long* link_counts, void* workspace, hipStream_t s) {
    if (int rc = links_checks("region_links_mc", index, table, counts, prev_index, prev_table, prev_counts, n, H, W, max_regions, max_pairs, min_overlap,
                              back, fwd, link_counts, workspace))
        return rc;
    FS_REQUIRE(mv, "region_links_mc: null pointer (mv)");
    FS_REQUIRE(frame_h >= trk::MC_BLOCK && frame_w >= trk::MC_BLOCK, "region_links_mc: the decoded frame must hold a block of %d, got frame %dx%d",
               trk::MC_BLOCK, frame_h, frame_w);
    FS_REQUIRE((int64_t)frame_h * frame_w < ((int64_t)1 << 31), "region_links_mc: a decoded frame of 2^31 pixels or more (%dx%d)", frame_h, frame_w);
    // the packed shifts are 16-bit: |shift| <= 1024 * mask / frame + 1/2 must stay below 2^15 (track_defs.h)
    FS_REQUIRE(H <= (int64_t)trk::MC_MAX_SCALE * frame_h && W <= (int64_t)trk::MC_MAX_SCALE * frame_w,
               "region_links_mc: the mask (%dx%d) may be at most %d times the decoded frame (%dx%d) along an axis", H, W, trk::MC_MAX_SCALE, frame_h,
               frame_w);
    unsigned long long* ws = static_cast<unsigned long long*>(workspace);
    Motion<true> mo;
    mo.FH = frame_h, mo.FW = frame_w, mo.hb = frame_h / trk::MC_BLOCK, mo.wb = frame_w / trk::MC_BLOCK;
    const int blocks = mo.hb * mo.wb;  // < 2^23
    unsigned* shifts = reinterpret_cast<unsigned*>(ws + (size_t)n * pair_words(max_regions, (unsigned)max_pairs));
    mo.shifts = shifts, mo.pair_stats = pair_stats;
    launch_zero(ws, n, max_regions, max_pairs, s);
    hipLaunchKernelGGL(track_shift_kernel, dim3((unsigned)cdiv(blocks, 256), (unsigned)n), dim3(256), 0, s, mv, pair_stats, prev_index, H, W, frame_h, frame_w,
                       blocks, max_regions, (unsigned)max_pairs, ws, shifts);
    hipLaunchKernelGGL(track_overlap_kernel<true>, dim3((unsigned)cdiv(W, 256), (unsigned)std::min(H, 65535), (unsigned)n), dim3(256), 0, s, index, table,
                       counts, prev_index, prev_table, prev_counts, H, W, max_regions, (unsigned)max_pairs, ws, mo);
    launch_best_unpack(prev_index, n, max_regions, max_pairs, min_overlap, ws, back, fwd, link_counts, s);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_region_tracks(const int* back, const int* fwd, const long long* counts, const long long* prev_tracks, int n, int max_regions,
                         long long* state, long long* tracks, hipStream_t s) {
    FS_REQUIRE(back && fwd && counts && state && tracks, "region_tracks: null pointer");
    if (int rc = track_sizes("region_tracks", n, max_regions)) return rc;
    hipLaunchKernelGGL(track_fill_kernel, dim3((unsigned)cdiv(max_regions, 256), (unsigned)n), dim3(256), 0, s, counts, max_regions, tracks);
    hipLaunchKernelGGL(track_ids_kernel, dim3(1), dim3(trk::TRACK_BLOCK), 0, s, back, fwd, counts, prev_tracks, n, max_regions, state, tracks);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
