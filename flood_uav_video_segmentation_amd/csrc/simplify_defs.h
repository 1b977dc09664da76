// Integer definitions of the outline simplification (simplify_ops.hip; definitions: include/floodseg_test.h, outline_simplify; DESIGN
// §3.14).  Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these functions, and a host program
// (tests/test_simplify_cpu.py builds tests/simplify_host_check.cpp) runs every test case round by round through the very same
// functions, so the distance key, the test, the round-1 rule and the split rule are checked on the CPU.
#ifndef FS_SIMPLIFY_DEFS_H_
#define FS_SIMPLIFY_DEFS_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_SMP_HD __host__ __device__ __forceinline__
#else
#define FS_SMP_HD inline
#endif

namespace fs {
namespace smp {

constexpr int CHUNK = 1024;  // vertices per workgroup of the scan passes
constexpr int MAX_CONTOURS = 1 << 20, MIN_VERTICES = 4, MAX_VERTICES = 1 << 22;
constexpr int MAX_COORD = 16384, MAX_TOL_Q = 1 << 20, MAX_ROUNDS = 256;
constexpr int ROUND_SLOTS = MAX_ROUNDS + 2;  // rounds 0 .. max_rounds, one spare
// the header of a frame's workspace, in 32-bit words: rows, vertices under the rows, unconverged, flags, kept vertices, three spare;
// then per round "some segment was open" and "some segment split"
constexpr int HDR_ROWS = 0, HDR_END = 1, HDR_UNCONVERGED = 2, HDR_FLAGS = 3, HDR_KEPT = 4, HDR_OPEN = 8, HDR_SPLIT = HDR_OPEN + ROUND_SLOTS;
constexpr int HDR_INTS = HDR_SPLIT + ROUND_SLOTS;  // 524
// the flags of a frame
constexpr int FLAG_UNCONVERGED = 1, FLAG_INPUT_OVERFLOW = 2, FLAG_INPUT_TRUNCATED = 4, FLAG_INCONSISTENT = 8;

// FS_OUTLINE_SIMPLIFY_WORKSPACE_BYTES / 8 per frame (C = max_contours, V = max_vertices): the segment cells, the keys and the two
// parities of maxima [V] 64-bit each; the two parities of smallest indices, the rows and the output rows [V] 32-bit each; the chunk
// sums; the contours' ends [C]; the header.
FS_SMP_HD size_t chunks(int V) { return ((size_t)V + CHUNK - 1) / CHUNK; }
FS_SMP_HD size_t frame_words(int C, int V) { return 6 * (size_t)V + (chunks(V) + 1) / 2 + ((size_t)C + 1) / 2 + HDR_INTS / 2; }

FS_SMP_HD int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
FS_SMP_HD int clamp_coord(int v) { return clamp_int(v, 0, MAX_COORD); }

// ---- the distance key of vertex p against the segment a -> b: q with q / L = the squared distance from p to the SEGMENT, L = |b - a|^2
// (L = 0: q = |p - a|^2).  Coordinates <= 2^14, so L <= 2^29 and q <= 2^58.
FS_SMP_HD int64_t seg_key(int ax, int ay, int bx, int by, int px, int py, int64_t* length2) {
    const int64_t ux = bx - ax, uy = by - ay, wx = px - ax, wy = py - ay;
    const int64_t L = ux * ux + uy * uy, t = ux * wx + uy * wy;
    *length2 = L;
    if (L == 0) return wx * wx + wy * wy;
    if (t <= 0) return (wx * wx + wy * wy) * L;
    if (t >= L) {
        const int64_t zx = px - bx, zy = py - by;
        return (zx * zx + zy * zy) * L;
    }
    const int64_t cross = ux * wy - uy * wx;
    return cross * cross;
}
// Does the farthest vertex of a segment examined in `round` split it?  Round 0 (the whole ring from its anchor) always; round 1 whenever
// the vertex is off the segment, whatever the tolerance -- so no ring degenerates; from round 2 on beyond the tolerance: 16 q > tol_q L.
FS_SMP_HD bool splits(int round, int64_t q, int64_t L, int tol_q) {
    if (round == 0) return true;
    if (round == 1) return q > 0;
    return 16 * q > (int64_t)tol_q * L;
}

// ---- a vertex's cell: the open segment (l, r) it is an interior vertex of, l < j < r <= m in the contour's own numbering (index m is
// vertex 0 again), or KEPT / DROPPED in the place of l.
constexpr int KEPT = -1, DROPPED = -2;
FS_SMP_HD uint64_t pack_seg(int l, int r) { return (uint64_t)(uint32_t)l << 32 | (uint32_t)r; }
FS_SMP_HD int seg_l(uint64_t cell) { return (int)(uint32_t)(cell >> 32); }
FS_SMP_HD int seg_r(uint64_t cell) { return (int)(uint32_t)cell; }
// The cell of interior vertex j of (l, r) once the segment's farthest vertex s is known: a segment that does not split drops its
// interior; one that does keeps s, and every other vertex moves to the half it lies in.
FS_SMP_HD uint64_t split_seg(int l, int r, int j, bool split, int s) {
    if (!split) return pack_seg(DROPPED, 0);
    if (j == s) return pack_seg(KEPT, 0);
    return j < s ? pack_seg(l, s) : pack_seg(s, r);
}

}  // namespace smp
}  // namespace fs
#endif  // FS_SIMPLIFY_DEFS_H_
