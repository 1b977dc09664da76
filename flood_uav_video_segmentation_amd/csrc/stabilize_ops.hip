// Temporal mask stabiliser (include/floodseg_test.h: mask_stabilize).  OUR DEFINITION -- the reference measures the
// flicker of its masks (flow/base.py:280-295) and does nothing about it.  An opt-in pass in front of the despeckle: nothing on the
// shipped routes calls it.  Integers throughout; the per-pixel transition is stabilize_defs.h's (__host__ __device__, also run on the
// CPU by the tests), the pixel -> block -> shift -> source rule is track_defs.h's, shared with region_links_mc.
//   in place      a pixel's history does not depend on any other pixel: ONE launch walks all n frames with the state words in
//                 registers, loaded and stored once (8 B per pixel and call, not per frame)
//   compensated   the prior word is gathered at the pixel's source, another pixel's word of the frame before: one launch per frame,
//                 ping-pong between the caller's plane and a second one in the workspace; one small launch packs the shifts first
// A thread owns four consecutive pixels of the flat [H * W] plane, so its state words are one aligned 16-byte access whatever W is; the
// byte planes (mask, confidence, out) of a frame start at f * H * W and are read and written as one dword only where that address is
// a multiple of 4, byte by byte otherwise; the last thread of a plane whose size is no multiple of 4 goes word by word.
// Counters: events are summed per thread, per wave (shuffles) and per workgroup (LDS), then ONE 64-bit atomic per counter, frame and
// workgroup, on a grid of at most GRID_PER_CU workgroups of THREADS per compute unit (same-address atomics serialise: with four times
// as many workgroups of 256 both pixel kernels took twice as long).  Integer sums: the order does not matter.
#include "kernels.h"
#include "stabilize_defs.h"
#include "track_defs.h"

#include <algorithm>

namespace fs {

namespace {

constexpr int THREADS = 1024;         // per workgroup of the two pixel kernels: 16 waves share one set of global atomics
constexpr int GRID_PER_CU = 2;        // workgroups per compute unit: the 32 waves a CU holds
constexpr int WINDOW_FRAMES = 2048;   // frames per in-place launch: their counters are 32 KiB of LDS

// four bytes of a byte plane at p as one dword (byte j in bits 8j..): one load where `wide`, else the first cnt bytes one by one
__device__ __forceinline__ uint32_t load4(const uint8_t* p, bool wide, int cnt) {
    if (wide) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < cnt) v |= (uint32_t)p[j] << (8 * j);
    return v;
}
// The narrow path stores four bytes in a straight line, none behind a branch of its own: a byte past the count (cnt >= 1) is stored as
// byte 0 once more, the same value to the same address by the same thread.
__device__ __forceinline__ void store4(uint8_t* p, uint32_t v, bool wide, int cnt) {
    if (wide) {
        *reinterpret_cast<uint32_t*>(p) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = j < cnt ? j : 0;
        p[k] = (uint8_t)(v >> (8 * k));
    }
}
__device__ __forceinline__ bool dword_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

__device__ __forceinline__ void load_words(const uint32_t* p, int cnt, uint32_t s[4]) {
    if (cnt == 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = j < cnt ? p[j] : 0u;
}
__device__ __forceinline__ void store_words(uint32_t* p, int cnt, const uint32_t s[4]) {
    if (cnt == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(s[0], s[1], s[2], s[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // straight-line as in store4: a word past the count repeats word 0
        const bool own = j < cnt;
        p[own ? j : 0] = own ? s[j] : s[0];
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the four pixels of a thread through one frame: s[] updated, the emitted bytes returned, the events' byte sums in *events
template <bool CONF>
__device__ __forceinline__ uint32_t quad_step(uint32_t s[4], uint32_t m, uint32_t cf, int cnt, int K, int P, int T, uint32_t* events) {
    uint32_t o4 = 0, ev = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
            int out;
            uint32_t e;
            const int conf = CONF ? (int)((cf >> (8 * j)) & 0xffu) : -1;
            s[j] = stb::step(s[j], (int)((m >> (8 * j)) & 0xffu), K, P, stb::trusted(conf, T), &out, &e);
            o4 |= (uint32_t)out << (8 * j);
            ev += e;
        }
    }
    *events = ev;
    return o4;
}

// the counts of an in-place call, cleared on the stream in front of its one launch (the compensated route clears them in its pass 0)
__global__ __launch_bounds__(256) void stabilize_clear_kernel(unsigned long long* __restrict__ counts, int words) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < words) counts[i] = 0ull;
}

// ------------------------------------------------------------------ in place: all frames of the call in one launch
// grid = at most GRID_PER_CU x CUs workgroups, each striding over the plane's quads; lds = n x 4 counters (n <= WINDOW_FRAMES).
template <bool CONF>
__global__ __launch_bounds__(THREADS) void stabilize_window_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ conf,
                                                               const int* __restrict__ pair_stats, int n, unsigned HW, int K, int P, int T, int has_state,
                                                               uint32_t* state, uint8_t* __restrict__ out, unsigned long long* counts) {
    extern __shared__ unsigned wg_counts[];  // [n][4] = (held, switched, seeded, trusted)
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 4 * n; i += THREADS) wg_counts[i] = 0u;
    __syncthreads();
    const unsigned quads = (HW + 3u) / 4u;  // HW < 2^31 - 1
    for (unsigned base = blockIdx.x * (unsigned)THREADS; base < quads; base += gridDim.x * (unsigned)THREADS) {  // uniform in the workgroup: the shuffles below are whole
        const unsigned q = base + tid;
        const bool active = q < quads;
        const unsigned p0 = active ? 4u * q : 0u;
        const int cnt = active ? (int)min(4u, HW - p0) : 0;
        uint32_t s[4] = {0u, 0u, 0u, 0u};
        if (has_state && active) load_words(state + p0, cnt, s);
        for (int f = 0; f < n; ++f) {
            const size_t at = (size_t)f * HW + p0;
            uint32_t ev = 0;
            if (active) {
                if (pair_stats && pair_stats[4 * (size_t)f + 2] != 0) s[0] = s[1] = s[2] = s[3] = 0u;  // a scene cut: no prior
                const uint32_t m = load4(mask + at, cnt == 4 && dword_aligned(mask + at), cnt);
                const uint32_t cf = CONF ? load4(conf + at, cnt == 4 && dword_aligned(conf + at), cnt) : 0u;
                const uint32_t o4 = quad_step<CONF>(s, m, cf, cnt, K, P, T, &ev);
                store4(out + at, o4, cnt == 4 && dword_aligned(out + at), cnt);
            }
            // bytes -> 16-bit fields: a wave's sum is at most 256 per counter
            const uint32_t a = wave_sum(ev & 0x00ff00ffu), b = wave_sum((ev >> 8) & 0x00ff00ffu);  // held | seeded << 16, switched | trusted << 16
            if (lane == 0) {
                unsigned* c = wg_counts + 4 * f;
                if (a & 0xffffu) atomicAdd(c + 0, a & 0xffffu);
                if (b & 0xffffu) atomicAdd(c + 1, b & 0xffffu);
                if (a >> 16) atomicAdd(c + 2, a >> 16);
                if (b >> 16) atomicAdd(c + 3, b >> 16);
            }
        }
        if (active) store_words(state + p0, cnt, s);
    }
    __syncthreads();
    for (int i = tid; i < 4 * n; i += THREADS)
        if (wg_counts[i]) atomicAdd(counts + i, (unsigned long long)wg_counts[i]);
}

// ------------------------------------------------------------------ compensated, pass 0: one packed shift per block and frame
// table[f] = (flag, shift of block 0, 1, ...): flag 1 = the frame has no prior at all (a cut, or frame 0 without a state).  The
// frame's four counters are cleared here as well: the frame launches only add to them.
__global__ __launch_bounds__(256) void stabilize_shift_kernel(const int* __restrict__ mv, const int* __restrict__ pair_stats, int has_state, int H, int W,
                                                              int FH, int FW, int blocks, unsigned* __restrict__ table,
                                                              unsigned long long* __restrict__ counts) {
    const int f = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    unsigned* row = table + (size_t)f * (blocks + 1);
    if (k < blocks) row[1 + k] = trk::mc_row_shift(mv + ((size_t)f * blocks + k) * trk::MC_VECTOR_INTS, H, W, FH, FW);
    if (k == 0) row[0] = ((f == 0 && !has_state) || (pair_stats && pair_stats[4 * (size_t)f + 2] != 0)) ? 1u : 0u;
    if (k < 4) counts[4 * (size_t)f + k] = 0ull;
}

// ------------------------------------------------------------------ compensated, pass 1..n: one frame, prior gathered at the source
template <bool CONF>
__global__ __launch_bounds__(THREADS) void stabilize_frame_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ conf,
                                                              const unsigned* __restrict__ row, int H, int W, int FH, int FW, int hb, int wb, int K, int P,
                                                              int T, const uint32_t* __restrict__ prev, uint32_t* __restrict__ next,
                                                              uint8_t* __restrict__ out, unsigned long long* counts) {
    __shared__ unsigned wg_counts[4];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 4) wg_counts[tid] = 0u;
    __syncthreads();
    const unsigned HW = (unsigned)H * (unsigned)W, quads = (HW + 3u) / 4u;
    const bool no_prior = row[0] != 0u;
    const unsigned* shifts = row + 1;
    const bool wide_m = dword_aligned(mask), wide_c = CONF && dword_aligned(conf), wide_o = dword_aligned(out);  // p0 is a multiple of 4
    uint32_t held = 0, switched = 0, seeded = 0, trusted = 0;
    for (unsigned q = blockIdx.x * (unsigned)THREADS + tid; q < quads; q += gridDim.x * (unsigned)THREADS) {
        const unsigned p0 = 4u * q;
        const int cnt = (int)min(4u, HW - p0);
        uint32_t s[4] = {0u, 0u, 0u, 0u};
        if (!no_prior) {
            int y = (int)(p0 / (unsigned)W), x = (int)(p0 % (unsigned)W);
            int by = trk::mc_block(y, H, FH);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < cnt) {
                    const int bx = trk::mc_block(x, W, FW);
                    const unsigned shift = by < hb && bx < wb ? shifts[(size_t)by * wb + bx] : 0u;  // the remainder strip: no shift
                    int ys, xs;
                    if (trk::mc_source(y, x, shift, H, W, &ys, &xs)) s[j] = prev[(size_t)ys * W + xs];
                    if (++x == W) {  // the quad runs on into the next row
                        x = 0;
                        ++y;
                        by = trk::mc_block(min(y, H - 1), H, FH);
                    }
                }
            }
        }
        uint32_t ev;
        const uint32_t m = load4(mask + p0, cnt == 4 && wide_m, cnt);
        const uint32_t cf = CONF ? load4(conf + p0, cnt == 4 && wide_c, cnt) : 0u;
        const uint32_t o4 = quad_step<CONF>(s, m, cf, cnt, K, P, T, &ev);
        store4(out + p0, o4, cnt == 4 && wide_o, cnt);
        store_words(next + p0, cnt, s);
        held += ev & 0xffu, switched += (ev >> 8) & 0xffu, seeded += (ev >> 16) & 0xffu, trusted += ev >> 24;
    }
    held = wave_sum(held), switched = wave_sum(switched), seeded = wave_sum(seeded), trusted = wave_sum(trusted);  // every lane is here
    if (lane == 0) {
        if (held) atomicAdd(wg_counts + 0, held);
        if (switched) atomicAdd(wg_counts + 1, switched);
        if (seeded) atomicAdd(wg_counts + 2, seeded);
        if (trusted) atomicAdd(wg_counts + 3, trusted);
    }
    __syncthreads();
    if (tid < 4 && wg_counts[tid]) atomicAdd(counts + tid, (unsigned long long)wg_counts[tid]);
}

unsigned grid_for(unsigned quads) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    return std::max(1u, std::min((quads + THREADS - 1u) / THREADS, (unsigned)(GRID_PER_CU * cus)));
}

}  // namespace

int launch_mask_stabilize(const uint8_t* mask, const uint8_t* conf, const int* mv, const int* pair_stats, int n, int H, int W, int frame_h, int frame_w,
                          int K, int persist, int trust, int has_state, uint32_t* state, uint8_t* out, long long* counts, void* workspace, hipStream_t s) {
    FS_REQUIRE(mask && out && state && counts, "mask_stabilize: null pointer");
    FS_REQUIRE(n >= 1, "mask_stabilize: at least one frame, got n=%d", n);
    FS_REQUIRE(H >= 1 && W >= 1, "mask_stabilize: sizes must be >= 1, got %dx%d", H, W);
    FS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 1, "mask_stabilize: a frame of 2^31 - 1 pixels or more (%dx%d)", H, W);
    FS_REQUIRE(K >= 1 && K <= stb::MAX_CLASSES, "mask_stabilize: classes=%d out of range (1..%d)", K, stb::MAX_CLASSES);
    FS_REQUIRE(persist >= 1 && persist <= stb::MAX_PERSIST, "mask_stabilize: persist=%d out of range (1..%d)", persist, stb::MAX_PERSIST);
    FS_REQUIRE(trust >= 0 && trust <= stb::TRUST_OFF, "mask_stabilize: trust=%d out of range (0..%d)", trust, stb::TRUST_OFF);
    FS_REQUIRE(has_state == 0 || has_state == 1, "mask_stabilize: has_state must be 0 or 1, got %d", has_state);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(state) % 16 == 0, "mask_stabilize: the state plane is not aligned to 16 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(counts) % 8 == 0, "mask_stabilize: counts is not aligned to 8 bytes");
    const unsigned HW = (unsigned)H * (unsigned)W, quads = (HW + 3u) / 4u;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (!mv) {
        const unsigned grid = grid_for(quads);
        for (int c0 = 0; c0 < n; c0 += 1 << 20)  // 4 n words, at most 2^22 a launch
            hipLaunchKernelGGL(stabilize_clear_kernel, dim3((unsigned)cdiv(4 * std::min(n - c0, 1 << 20), 256)), dim3(256), 0, s, cnt + 4 * (size_t)c0,
                               4 * std::min(n - c0, 1 << 20));
        for (int f0 = 0; f0 < n; f0 += WINDOW_FRAMES) {  // one launch up to WINDOW_FRAMES frames; a longer call is chained here
            const int take = std::min(n - f0, WINDOW_FRAMES);
            const size_t at = (size_t)f0 * HW;
            const int* stats = pair_stats ? pair_stats + 4 * (size_t)f0 : nullptr;
            auto kernel = conf ? stabilize_window_kernel<true> : stabilize_window_kernel<false>;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), (size_t)take * 4 * sizeof(unsigned), s, mask + at, conf ? conf + at : nullptr, stats, take, HW, K,
                               persist, trust, f0 ? 1 : has_state, state, out + at, cnt + 4 * (size_t)f0);
        }
        FS_HIP(hipGetLastError());
        return 0;
    }
    FS_REQUIRE(workspace, "mask_stabilize: mv needs the workspace");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mask_stabilize: the workspace is not aligned to 16 bytes");
    FS_REQUIRE(n <= 65535, "mask_stabilize: at most 65535 frames per compensated call, got n=%d", n);
    FS_REQUIRE(frame_h >= trk::MC_BLOCK && frame_w >= trk::MC_BLOCK, "mask_stabilize: mv needs the decoded frame's size, at least a block of %d, got frame %dx%d",
               trk::MC_BLOCK, frame_h, frame_w);
    FS_REQUIRE((int64_t)frame_h * frame_w < ((int64_t)1 << 31), "mask_stabilize: a decoded frame of 2^31 pixels or more (%dx%d)", frame_h, frame_w);
    FS_REQUIRE(H <= (int64_t)trk::MC_MAX_SCALE * frame_h && W <= (int64_t)trk::MC_MAX_SCALE * frame_w,
               "mask_stabilize: the mask (%dx%d) may be at most %d times the decoded frame (%dx%d) along an axis", H, W, trk::MC_MAX_SCALE, frame_h, frame_w);
    const int hb = frame_h / trk::MC_BLOCK, wb = frame_w / trk::MC_BLOCK, blocks = hb * wb;  // < 2^23
    uint32_t* second = static_cast<uint32_t*>(workspace);
    unsigned* table = second + ((size_t)HW + 3) / 4 * 4;
    const unsigned grid = grid_for(quads);
    hipLaunchKernelGGL(stabilize_shift_kernel, dim3((unsigned)cdiv(blocks, 256), (unsigned)n), dim3(256), 0, s, mv, pair_stats, has_state, H, W, frame_h, frame_w,
                       blocks, table, cnt);
    // Frame f writes the caller's plane when n - 1 - f is even, so the last frame always does.  Frame 0 must not read the plane it
    // writes (the gather reads other pixels' words): for odd n the caller's prior state is copied to the second plane first.
    const bool odd = (n & 1) != 0;
    if (odd && has_state) FS_HIP(hipMemcpyAsync(second, state, (size_t)HW * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    for (int f = 0; f < n; ++f) {
        const bool to_caller = ((n - 1 - f) & 1) == 0;
        const uint32_t* prev = to_caller ? second : state;
        uint32_t* next = to_caller ? state : second;
        const size_t at = (size_t)f * HW;
        auto kernel = conf ? stabilize_frame_kernel<true> : stabilize_frame_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), 0, s, mask + at, conf ? conf + at : nullptr, table + (size_t)f * (blocks + 1), H, W, frame_h, frame_w, hb,
                           wb, K, persist, trust, prev, next, out + at, cnt + 4 * (size_t)f);
    }
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
