// Integer definitions of the region outlines (outline_ops.hip; definitions: include/floodseg_test.h, region_outlines).
// Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these functions, and a host program
// (tests/test_outlines_cpu.py builds tests/outlines_host_check.cpp) walks every contour of every test case through the very same
// functions, so the slot packing, the corner of a slot, the successor rule and the anchor rule are checked on the CPU.
#ifndef FS_OUTLINE_DEFS_H_
#define FS_OUTLINE_DEFS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_OTL_HD __host__ __device__ __forceinline__
#else
#define FS_OTL_HD inline
#endif

namespace fs {
namespace otl {

constexpr int CHUNK = 1024;                                 // pixels (4096 slots), and nodes, per workgroup of the counting / ranking passes
constexpr int MAX_CONTOURS = 1 << 20, MIN_VERTICES = 4, MAX_VERTICES = 1 << 22;
constexpr int64_t MAX_PIXELS = (int64_t)1 << 29;            // H * W below this: a slot id 4 * pixel + d fits 31 bits

// ---- slots.  The crack d of pixel (x, y): 0 top heading east, 1 right heading south, 2 bottom heading west, 3 left heading north;
// the pixel is on the crack's right.
FS_OTL_HD int pack_slot(int x, int y, int d, int W) { return 4 * (y * W + x) + d; }
FS_OTL_HD void unpack_slot(int slot, int W, int* x, int* y, int* d) {
    const int p = slot >> 2;
    *d = slot & 3;
    *y = p / W;
    *x = p - *y * W;
}
FS_OTL_HD int dir_x(int d) { return (d == 0) - (d == 2); }
FS_OTL_HD int dir_y(int d) { return (d == 1) - (d == 3); }
// the start corner of a crack: top (x, y), right (x + 1, y), bottom (x + 1, y + 1), left (x, y + 1)
FS_OTL_HD void start_corner(int x, int y, int d, int* X, int* Y) {
    *X = x + (d == 1 || d == 2);
    *Y = y + (d >= 2);
}

// A pixel's row as the outlines see it: rows outside 0 .. R - 1 (background, regions past the cap, a caller's garbage) own no cracks.
FS_OTL_HD int row_or_none(int v, int R) { return v >= 0 && v < R ? v : -1; }

// The index plane of one frame; at() answers -1 outside the frame.
struct Plane {
    const int32_t* index;
    int H, W, R;
    FS_OTL_HD int at(int x, int y) const { return x >= 0 && y >= 0 && x < W && y < H ? row_or_none(index[(int64_t)y * W + x], R) : -1; }
};

// ---- the 3 x 3 neighbourhood of a pixel of row r >= 0 as 8 bits, bit set = that neighbour holds r too:
// 0 N, 1 NE, 2 E, 3 SE, 4 S, 5 SW, 6 W, 7 NW.
FS_OTL_HD unsigned same_bits(const Plane& p, int x, int y, int r) {
    return (unsigned)(p.at(x, y - 1) == r) | (unsigned)(p.at(x + 1, y - 1) == r) << 1 | (unsigned)(p.at(x + 1, y) == r) << 2 |
           (unsigned)(p.at(x + 1, y + 1) == r) << 3 | (unsigned)(p.at(x, y + 1) == r) << 4 | (unsigned)(p.at(x - 1, y + 1) == r) << 5 |
           (unsigned)(p.at(x - 1, y) == r) << 6 | (unsigned)(p.at(x - 1, y - 1) == r) << 7;
}
// Edge d is a crack when the neighbour across it (bit 2 d) is not of the row.
FS_OTL_HD unsigned crack_bits(unsigned same) {
    return (~same & 1u) | (~same >> 1 & 2u) | (~same >> 2 & 4u) | (~same >> 3 & 8u);
}
// The predecessor of crack d runs straight into it exactly when the pixel behind (against d: bit 2 (d + 3) mod 4) is of the row and the
// pixel beside that one, across the line of the crack (the next bit), is not.  Every other crack is a RUN START.  The rule needs no
// connectivity: at a saddle both predecessors turn.
FS_OTL_HD unsigned start_bits(unsigned same) {
    unsigned out = 0;
    for (int d = 0; d < 4; ++d) {
        const int behind = 2 * ((d + 3) & 3);
        const bool crack = !(same >> (2 * d) & 1u), straight = (same >> behind & 1u) && !(same >> (behind + 1) & 1u);
        out |= (unsigned)(crack && !straight) << d;
    }
    return out;
}

// ---- the successor rule.  Crack (x, y, d) of row r ends at corner V.  A is the pixel ahead, B the pixel ahead on the left (diagonal
// across V); the pixel on the left is not r (that is the crack).  B and A of r: left turn onto B.  A only: straight on, onto A.
// Neither: right turn, the next edge of the same pixel.  B only is the SADDLE: left at connectivity 8, right at 4.
FS_OTL_HD int successor(const Plane& p, int r, int x, int y, int d, int connectivity) {
    const int left = (d + 3) & 3;
    const int ax = x + dir_x(d), ay = y + dir_y(d), bx = ax + dir_x(left), by = ay + dir_y(left);
    const bool a = p.at(ax, ay) == r, b = p.at(bx, by) == r;
    if (b && (a || connectivity == 8)) return pack_slot(bx, by, left, p.W);
    if (a) return pack_slot(ax, ay, d, p.W);
    return pack_slot(x, y, (d + 1) & 3, p.W);
}

// The run start that follows run start `slot`: straight on while the successor keeps the direction.  A straight run stays inside the
// frame and moves one pixel per crack, so it has at most max(H, W) cracks: the loop's bound follows from the arguments alone.
FS_OTL_HD int next_run_start(const Plane& p, int slot, int connectivity) {
    int x, y, d;
    unpack_slot(slot, p.W, &x, &y, &d);
    const int r = p.at(x, y);
    const int bound = p.H > p.W ? p.H : p.W;
    int cur = slot;
    for (int k = 0; k < bound; ++k) {
        cur = successor(p, r, x, y, d, connectivity);
        if ((cur & 3) != d) break;
        x += dir_x(d);
        y += dir_y(d);
    }
    return cur;
}

// ---- the anchor rule.  A node is a run start; nodes are numbered in ascending slot order, so the smallest node of a contour is its
// anchor.  A ranking cell packs (smallest node seen, steps back to it): the minimum of two cells is the cell of the smaller node, and
// of the nearer one when both name the same node (a window that wraps its contour).
FS_OTL_HD uint64_t pack_rank(uint32_t node, uint32_t steps) { return (uint64_t)node << 32 | steps; }
FS_OTL_HD uint32_t rank_node(uint64_t cell) { return (uint32_t)(cell >> 32); }
FS_OTL_HD uint32_t rank_steps(uint64_t cell) { return (uint32_t)cell; }
// One round of pointer jumping: `mine` covers the 2^k nodes that end at a node, `far` the 2^k nodes that end 2^k nodes before it.
FS_OTL_HD uint64_t join_rank(uint64_t mine, uint64_t far, uint32_t window) {
    const uint64_t moved = pack_rank(rank_node(far), rank_steps(far) + window);
    return moved < mine ? moved : mine;
}
// rounds after which every window holds its whole contour: the smallest k with 2^k >= max_vertices
FS_OTL_HD int rank_rounds(int max_vertices) {
    int k = 0;
    while (k < 31 && ((int64_t)1 << k) < max_vertices) ++k;
    return k;
}

}  // namespace otl
}  // namespace fs
#endif  // FS_OUTLINE_DEFS_H_
