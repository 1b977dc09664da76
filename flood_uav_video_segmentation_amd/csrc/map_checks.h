// The argument checks that the launchers of the map family share (mosaic_ops.hip, ortho_ops.hip, refine_ops.hip, relocate_ops.hip,
// merge_ops.hip).  Host code only.  A check takes the op's name, which leads every message, and returns through fs::fail: call it under
// FS_TRY, in the place where the op has always made that check -- the first refusal is part of an op's behaviour.
#ifndef FS_MAP_CHECKS_H_
#define FS_MAP_CHECKS_H_

#include "common.h"
#include "relocate_defs.h"

namespace fs {

inline bool side_ok(int v, int lo) { return v >= lo && v <= mos::MAX_SIDE; }
inline bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
inline bool origin_ok(int ox, int oy) { return ox >= -mos::MAX_SIDE && ox <= mos::MAX_SIDE && oy >= -mos::MAX_SIDE && oy <= mos::MAX_SIDE; }

// what: "the frame", "the mask", "the canvas", "canvas A", "the plane", ..; lo: its smallest side
inline int check_sides(const char* op, const char* what, int lo, int h, int w) {
    FS_REQUIRE(side_ok(h, lo) && side_ok(w, lo), "%s: %s must be %d..%d pixels a side, got %dx%d", op, what, lo, mos::MAX_SIDE, h, w);
    return 0;
}
// what: "the origin", "origin A", "origin B"
inline int check_origin(const char* op, const char* what, int ox, int oy) {
    FS_REQUIRE(origin_ok(ox, oy), "%s: %s must lie within %d pixels of the canvas corner, got (%d, %d)", op, what, mos::MAX_SIDE, ox, oy);
    return 0;
}
// a frame's mask (its smallest side: lo), the canvas and the canvas's origin
inline int check_mask_on_canvas(const char* op, int lo, int H, int W, int CH, int CW, int ox, int oy) {
    FS_TRY(check_sides(op, "the mask", lo, H, W));
    FS_TRY(check_sides(op, "the canvas", 1, CH, CW));
    return check_origin(op, "the origin", ox, oy);
}
// the two canvases of a merge op and their origins
inline int check_canvases(const char* op, int CH_a, int CW_a, int ox_a, int oy_a, int CH_b, int CW_b, int ox_b, int oy_b) {
    FS_TRY(check_sides(op, "canvas A", 1, CH_a, CW_a));
    FS_TRY(check_sides(op, "canvas B", 1, CH_b, CW_b));
    FS_TRY(check_origin(op, "origin A", ox_a, oy_a));
    return check_origin(op, "origin B", ox_b, oy_b);
}
inline int check_cell_edge(const char* op, int S) {
    FS_REQUIRE(relo::scale_ok(S), "%s: the cell edge must be 4, 8 or 16, got S=%d", op, S);
    return 0;
}
// what: "canvas", "canvas A"; after check_cell_edge
inline int check_has_cell(const char* op, const char* what, int CH, int CW, int S) {
    FS_REQUIRE(CH / S >= 1 && CW / S >= 1, "%s: a %dx%d %s has no cell of S=%d", op, CH, CW, what, S);
    return 0;
}
// a frame as ingest_src.h takes it: format, matrix, range, the chroma pointers, FH x FW
inline int check_frame_source(const char* op, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW) {
    FS_REQUIRE(format >= 0 && format <= 2, "%s: format must be 0 (RGB24), 1 (NV12) or 2 (I420), got %d", op, format);
    FS_REQUIRE(matrix == 0 || matrix == 1, "%s: matrix must be 0 (BT.601) or 1 (BT.709), got %d", op, matrix);
    FS_REQUIRE(full_range == 0 || full_range == 1, "%s: range must be 0 (limited) or 1 (full), got %d", op, full_range);
    FS_REQUIRE(format == 0 || (u && (format != 2 || v)), "%s: null chroma pointer for a YUV format", op);
    return check_sides(op, "the frame", 1, FH, FW);
}

}  // namespace fs

#endif  // FS_MAP_CHECKS_H_
