// Integer helpers of the region tracking (track_ops.hip; definitions: include/floodseg_test.h, region_links / region_tracks; DESIGN
// §3.12).  Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these functions, and a host program
// (tests/test_tracks_cpu.py builds tests/tracks_host_check.cpp) runs serial versions of the four passes through the very same
// functions, so the packing, the probe sequence and the continue / born rule are checked on the CPU.
#ifndef FS_TRACK_DEFS_H_
#define FS_TRACK_DEFS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_TRK_HD __host__ __device__ __forceinline__
#else
#define FS_TRK_HD inline
#endif

namespace fs {
namespace trk {

constexpr int MIN_PAIRS = 16, MAX_PAIRS = 1 << 20;  // the pair table's size: a power of two in this range
constexpr int TRACK_BLOCK = 1024;                   // rows per piece of the track-id scan: one workgroup

// ---- the pair table.  A slot's key is 0 while it is empty; the key of the pair (row a of the frame before, row b of this frame),
// 0 <= a, b < 65536, has bit 63 set, so no pair packs to 0.
FS_TRK_HD uint64_t pack_key(int a, int b) { return (1ull << 63) | ((uint64_t)(uint32_t)a << 32) | (uint64_t)(uint32_t)b; }
FS_TRK_HD int key_a(uint64_t key) { return (int)((key >> 32) & 0x7fffffffu); }
FS_TRK_HD int key_b(uint64_t key) { return (int)(key & 0xffffffffu); }

// The probe sequence of a key: probe i = 0 .. max_pairs - 1 visits slot (hash + i) mod max_pairs, so the max_pairs probes visit EVERY
// slot once.  An insertion therefore fails only when all max_pairs slots hold other keys: whether a frame pair overflows depends on
// its number of distinct pairs alone, never on the hash or on the order of the insertions.
FS_TRK_HD uint32_t probe_slot(uint64_t key, uint32_t i, uint32_t max_pairs) {
    const uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32);
    return (h + i) & (max_pairs - 1u);
}

// ---- the best partner of a row: the maximum of overlap << 32 | (0xffffffff - other row) over the row's pairs.  The larger overlap
// wins, and among equal overlaps the inverted row makes the LOWEST other row the maximum.  0 = no pair (a stored pair has overlap >= 1).
FS_TRK_HD uint64_t pack_best(uint32_t overlap, int other) { return ((uint64_t)overlap << 32) | (uint64_t)(0xffffffffu - (uint32_t)other); }
FS_TRK_HD int best_overlap(uint64_t best) { return (int)(best >> 32); }  // < 2^31: a frame has fewer pixels
FS_TRK_HD int best_row(uint64_t best) { return (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu)); }

// One (row, overlap) link from a packed best value: the partner, unless the frame pair overflowed or its best overlap is below
// min_overlap (>= 1, so the empty value 0 never qualifies): then (-1, 0).
FS_TRK_HD void unpack_link(uint64_t best, int min_overlap, bool overflow, int* row, int* overlap) {
    const bool ok = !overflow && best_overlap(best) >= min_overlap;
    *row = ok ? best_row(best) : -1;
    *overlap = ok ? best_overlap(best) : 0;
}

// ---- the continue / born rule.  Row b of this frame, whose back link names row a of the frame before, CONTINUES a's track exactly
// when a >= 0, a's forward link names b, and a has a track (prev_id >= 0; -1: no track table for the frame before, or no such row).
FS_TRK_HD bool continues(int a, int fwd_of_a, int b, long long prev_id) { return a >= 0 && fwd_of_a == b && prev_id >= 0; }

}  // namespace trk
}  // namespace fs
#endif  // FS_TRACK_DEFS_H_
