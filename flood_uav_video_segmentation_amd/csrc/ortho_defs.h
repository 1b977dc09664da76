// The rules of the orthophoto under the flood-extent mosaic (ortho_ops.hip; definitions: include/floodseg_test.h, ortho_accumulate and
// ortho_compose).  Plain __host__ __device__ C++ with nothing of HIP in it, in the style of mosaic_defs.h: the kernels call
// these functions, and a host program (tests/test_ortho_cpu.py builds tests/ortho_host_check.cpp) runs them on the CPU.  Which frame
// pixel lies under a canvas pixel is mosaic_defs.h's business (pose_votes, anchor_coord, source_pixel, touches), used unchanged: an
// orthophoto pixel and the mosaic's vote at that canvas pixel come from the same mask pixel of the same frame.
#ifndef FS_ORTHO_DEFS_H_
#define FS_ORTHO_DEFS_H_

#include "mosaic_defs.h"

namespace fs {
namespace orth {

enum Mode { MODE_CENTRE = 0, MODE_LATEST = 1 };
constexpr uint64_t RANK_EMPTY = ~(uint64_t)0;   // a canvas pixel no frame has won: every rank of a frame is smaller
constexpr uint32_t ORDINAL_NONE = 0xFFFFFFFFu;  // refused as an ordinal: with it a latest-mode rank could not beat RANK_EMPTY's high word
constexpr uint32_t UNSEEN = 255u;               // mosaic_resolve's class of a canvas pixel without votes

// ---- the rank of frame pixel (x, y), 0 <= x < W, 0 <= y < H, of the frame with this ordinal.  The smaller rank owns the canvas pixel.
// centre: the squared distance of the pixel's centre from the optical axis, in half pixels: |2x + 1 - W| <= W - 1 < 2^14 (W <= 16384),
// so each square is below 2^28 and the key below 2^29 -- it fits the high word with room to spare, and the int products cannot
// overflow.  Ties go to the earlier frame through the low word.
FS_MOS_HD uint32_t centre_key(int x, int y, int H, int W) {
    const int dx = 2 * x + 1 - W, dy = 2 * y + 1 - H;
    return (uint32_t)(dx * dx) + (uint32_t)(dy * dy);
}
FS_MOS_HD uint64_t frame_rank(int mode, int x, int y, int H, int W, uint32_t ordinal) {
    const uint32_t key = mode == MODE_LATEST ? 0xFFFFFFFFu - ordinal : centre_key(x, y, H, W);
    return ((uint64_t)key << 32) | ordinal;
}
FS_MOS_HD uint32_t rank_ordinal(uint64_t rank) { return (uint32_t)rank; }
FS_MOS_HD bool replaces(uint64_t rank, uint64_t stored) { return rank < stored; }  // strictly: a second identical call changes nothing

// ---- one frame at canvas pixel (X, Y): false = the frame has no pixel there; otherwise the frame pixel and its rank.  The caller has
// tested pose_votes(pose) (the products below rely on its bounds; mosaic_defs.h derives them).
FS_MOS_HD bool candidate(const int64_t* from_anchor, int X, int Y, int ox, int oy, int H, int W, int mode, uint32_t ordinal, int* x, int* y, uint64_t* rank) {
    int64_t sx, sy;
    mos::source_pixel(from_anchor, mos::anchor_coord(X, ox), mos::anchor_coord(Y, oy), &sx, &sy);
    if (sx < 0 || sx >= W || sy < 0 || sy >= H) return false;
    *x = (int)sx, *y = (int)sy;
    *rank = frame_rank(mode, *x, *y, H, W, ordinal);
    return true;
}

FS_MOS_HD uint32_t pack_rgba(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16) | (0xFFu << 24); }  // alpha 255: seen

// ---- compose.  under: the orthophoto's pixel, or the fill colour (r | g << 8 | b << 16) where no frame has been
FS_MOS_HD uint32_t under_rgb(uint32_t rgba, uint32_t fill) { return ((rgba >> 24) != 0u ? rgba : fill) & 0xFFFFFFu; }
// a class takes its palette colour only below K: 255 is "never seen" here, not class 0 as in compose_frame
FS_MOS_HD bool takes_colour(uint32_t k, int K) { return k < (uint32_t)K; }
FS_MOS_HD bool in_edge_set(uint32_t k, uint32_t edge_set) { return k < 32u && ((edge_set >> k) & 1u) != 0u; }
// the one-pixel line along the INSIDE of class k's boundary: a 4-neighbour of another seen class.  A neighbour outside the canvas is
// handed in as UNSEEN; unseen ground makes no edge.
FS_MOS_HD bool differs(uint32_t k, uint32_t neighbour) { return neighbour != k && neighbour != UNSEEN; }
FS_MOS_HD bool on_edge(uint32_t k, uint32_t edge_set, uint32_t north, uint32_t south, uint32_t west, uint32_t east) {
    return in_edge_set(k, edge_set) && (differs(k, north) || differs(k, south) || differs(k, west) || differs(k, east));
}

}  // namespace orth
}  // namespace fs

#endif  // FS_ORTHO_DEFS_H_
