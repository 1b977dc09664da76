// Union-find primitives of the region labelling (region_ops.hip; definitions: include/floodseg_test.h, mask_regions).
// Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these functions one pixel per thread, and a host program
// (tests/test_regions_cpu.py builds one) calls the very same functions pixel by pixel, tile by tile, so the merge logic and the
// ends of its loops are checked on the CPU.
//
// A plane of int32 cells holds, per pixel, BIAS + the index of its parent.  The tile-local plane (LDS) uses BIAS 0 and local indices;
// the global plane uses BIAS 1 and frame-local pixel indices, 0 meaning background: a stored cell is then always a valid LABEL of some
// pixel of the same set, so the flatten pass can overwrite parents with final labels in place while other threads still walk them.
//
// THE INVARIANT: parent[i] <= i, with equality exactly at a root.  Every store keeps it: a cell is only ever lowered (min), and only
// to the index of a pixel of the same region.  The root of a finished set is therefore its smallest index: the anchor, the region's
// first pixel in raster order (the global index is raster order; inside a tile the local index is, too).
#ifndef FS_REGION_UF_H_
#define FS_REGION_UF_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_UF_HD __host__ __device__ __forceinline__
#else
#define FS_UF_HD inline
#endif

namespace fs {
namespace uf {

constexpr int TILE_H = 32, TILE_W = 64;  // one workgroup's tile; a wave covers one tile row

// Relaxed loads and mins at agent scope on the device, so that a find never spins on a stale L1 line and a min is one atomic; plain
// memory operations on the host, where one thread runs the passes in sequence.
FS_UF_HD int cell_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
FS_UF_HD void cell_store(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p = v;
#endif
}
FS_UF_HD int cell_min(int* p, int v) {  // returns the old value
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    const int old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

// The root of i.  Bounded: every step goes to a strictly smaller index (parent[i] < i off a root), so at most i steps.
template <int BIAS>
FS_UF_HD int find(const int* cells, int i) {
    for (;;) {  // measure: i, strictly decreasing, >= 0
        const int p = cell_load(cells + i) - BIAS;
        if (p >= i || p < 0) return i;  // p == i: a root.  p > i or p < 0 cannot happen; a root too, so that no plane, however wrong, keeps the
                                        // loop going or sends it outside the plane
        i = p;
    }
}

// Unite the sets of a and b: the larger root is hung under the smaller.  Bounded: a failed min (somebody else lowered the cell first)
// continues from the value it found there, which is strictly below the root it tried to lower, so a + b strictly decreases from one
// round to the next; each find inside is bounded as above.
template <int BIAS>
FS_UF_HD void unite(int* cells, int a, int b) {
    for (;;) {  // measure: a + b, strictly decreasing, >= 0
        a = find<BIAS>(cells, a);
        b = find<BIAS>(cells, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }            // a > b: hang a under b
        const int old = cell_min(cells + a, b + BIAS) - BIAS;   // old <= a (invariant)
        if (old >= a) return;                                     // a was still a root: linked
        a = old;                                                  // old < a: somebody linked a elsewhere; go on with that set and b
    }
}

// The class byte the labelling compares: ids >= K are background, 255 (K <= 255, so 255 is never a class)
FS_UF_HD int region_class(int id, int K) { return id < K ? id : 255; }

// ---- pass 1, one pixel of a tile: link (ly, lx) to its in-tile neighbours that come before it in raster order.
// cls = the tile's class bytes [TILE_H][TILE_W] (255 = background or outside the frame), parent = the tile's cells (BIAS 0).
FS_UF_HD void tile_link(const uint8_t* cls, int* parent, int ly, int lx, int conn8) {
    const int i = ly * TILE_W + lx;
    const int c = cls[i];
    if (c == 255) return;
    if (lx > 0 && cls[i - 1] == c) unite<0>(parent, i, i - 1);
    if (ly > 0) {
        if (cls[i - TILE_W] == c) unite<0>(parent, i, i - TILE_W);
        if (conn8) {
            if (lx > 0 && cls[i - TILE_W - 1] == c) unite<0>(parent, i, i - TILE_W - 1);
            if (lx < TILE_W - 1 && cls[i - TILE_W + 1] == c) unite<0>(parent, i, i - TILE_W + 1);
        }
    }
}

// pass 1, the cell written for tile pixel i of the tile at (ty0, tx0): the frame index of its local root, + 1; 0 for background
FS_UF_HD int tile_cell(const uint8_t* cls, const int* parent, int i, int ty0, int tx0, int W) {
    if (cls[i] == 255) return 0;
    const int r = find<0>(parent, i);
    return (ty0 + r / TILE_W) * W + tx0 + r % TILE_W + 1;
}

// ---- pass 2, the tile-border walk.  Border pixels of a frame are numbered t = 0 .. border_count - 1: first the pixels of every row
// that starts a tile row (y = TILE_H, 2 TILE_H, ...), then the pixels of every column that starts a tile column.
FS_UF_HD int border_rows(int H) { return (H - 1) / TILE_H; }
FS_UF_HD int border_cols(int W) { return (W - 1) / TILE_W; }
FS_UF_HD int64_t border_count(int H, int W) { return (int64_t)border_rows(H) * W + (int64_t)border_cols(W) * H; }

FS_UF_HD void border_pair(const uint8_t* mask, int* cells, int K, int W, int y, int x, int qy, int qx) {
    const int c = region_class(mask[(int64_t)y * W + x], K);
    if (c != 255 && region_class(mask[(int64_t)qy * W + qx], K) == c) unite<1>(cells, y * W + x, qy * W + qx);
}

// unite border pixel t with its neighbours across the tile edge.  Row pixels look up (and, at 8, up-left and up-right: these include
// both diagonal pairs at a tile corner); column pixels look left (and, at 8, up-left and down-left).  A pair met twice is united twice.
FS_UF_HD void border_walk(const uint8_t* mask, int* cells, int K, int H, int W, int conn8, int64_t t) {
    const int64_t nrow = (int64_t)border_rows(H) * W;
    if (t < nrow) {
        const int y = (int)(t / W + 1) * TILE_H, x = (int)(t % W);
        border_pair(mask, cells, K, W, y, x, y - 1, x);
        if (conn8) {
            if (x > 0) border_pair(mask, cells, K, W, y, x, y - 1, x - 1);
            if (x < W - 1) border_pair(mask, cells, K, W, y, x, y - 1, x + 1);
        }
    } else {
        const int64_t u = t - nrow;
        const int x = (int)(u / H + 1) * TILE_W, y = (int)(u % H);
        border_pair(mask, cells, K, W, y, x, y, x - 1);
        if (conn8) {
            if (y > 0) border_pair(mask, cells, K, W, y, x, y - 1, x - 1);
            if (y < H - 1) border_pair(mask, cells, K, W, y, x, y + 1, x - 1);
        }
    }
}

// ---- pass 3, one pixel: the cell becomes the canonical label, 1 + the root's index (a cell someone else already flattened is a
// valid parent cell as well: that of a pixel hung directly under its root).
FS_UF_HD void flatten(int* cells, int i) {
    if (cell_load(cells + i) == 0) return;
    cell_store(cells + i, find<1>(cells, i) + 1);
}

}  // namespace uf
}  // namespace fs
#endif  // FS_REGION_UF_H_
