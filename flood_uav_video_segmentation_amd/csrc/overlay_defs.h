// Integer definitions of the region overlay's labels (overlay_ops.hip; definitions: include/floodseg_test.h, frame_compose_regions;
// DESIGN §3.15): the 5 x 7 digit font, which rows get a label, the text box and the ink test.  Plain __host__ __device__ C++ with nothing
// of HIP in it: the stamp kernel calls these functions, and a host program (tests/test_overlay_cpu.py builds
// tests/overlay_host_check.cpp) prints every label box and ink cell of a scene through the very same functions.
#ifndef FS_OVERLAY_DEFS_H_
#define FS_OVERLAY_DEFS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_OVL_HD __host__ __device__ __forceinline__
#else
#define FS_OVL_HD inline
#endif

namespace fs {
namespace ovl {

constexpr int MAX_REGIONS = 65536, MAX_FILL = 256, MAX_WIDTH = 4, MAX_SCALE = 4, MAX_DIGITS = 7;
constexpr int64_t ID_MODULUS = 10000000;  // a label prints id mod 10^7
constexpr int GLYPH_W = 5, GLYPH_H = 7, GLYPH_PITCH = 6;
constexpr int MARK_HALO = 1, MARK_INK = 2;  // the bits of the marks plane

// FONT[digit][row], rows top to bottom, bit 4 the leftmost column
constexpr uint8_t FONT[10][7] = {{0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},
                                 {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},
                                 {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
                                 {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},
                                 {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}};

// a digit's seven rows in one word: row v in bits 5 v .. 5 v + 4.  The ten words are compile-time constants picked by a switch, so the
// stamp kernel loads nothing per glyph (a loop over FONT's rows is seven dependent memory loads per digit on the device)
constexpr uint64_t pack_glyph(int digit) {
    uint64_t g = 0;
    for (int v = 0; v < GLYPH_H; ++v) g |= (uint64_t)FONT[digit][v] << (5 * v);
    return g;
}
FS_OVL_HD uint64_t glyph_bits(int digit) {
    constexpr uint64_t G0 = pack_glyph(0), G1 = pack_glyph(1), G2 = pack_glyph(2), G3 = pack_glyph(3), G4 = pack_glyph(4), G5 = pack_glyph(5),
                       G6 = pack_glyph(6), G7 = pack_glyph(7), G8 = pack_glyph(8), G9 = pack_glyph(9);
    switch (digit) {
        case 0: return G0;
        case 1: return G1;
        case 2: return G2;
        case 3: return G3;
        case 4: return G4;
        case 5: return G5;
        case 6: return G6;
        case 7: return G7;
        case 8: return G8;
        default: return G9;
    }
}

// a row as the overlay sees it: values outside 0 .. R - 1 (background, regions past the cap, a caller's garbage) are -1
FS_OVL_HD int row_or_none(int v, int R) { return v >= 0 && v < R ? v : -1; }

FS_OVL_HD int64_t floor_div(int64_t a, int64_t b) {  // b > 0
    const int64_t q = a / b;
    return q * b > a ? q - 1 : q;
}

struct Label {
    int nd;                     // digits, 0: the row gets no label
    int x0, y0, tw, th;         // the text box [x0, x0 + tw) x [y0, y0 + th); the halo rectangle is s wider on every side
    uint8_t digit[MAX_DIGITS];  // most significant first
};

// The label of row r (0 <= r < R) of a frame h x w at scale s (1..4).  live = min(counts[1], R); id = the row's id (tracks[r][0], or
// r); area, sum_x, sum_y = table columns 1, 6, 7.  Any int64 values are valid arguments: a label that is drawn lies inside the frame.
FS_OVL_HD Label make_label(int r, int64_t live, int64_t id, int64_t area, int64_t sum_x, int64_t sum_y, int64_t min_area, int h, int w, int s) {
    Label L{};
    if (r >= live || id < 0 || area < min_area || area < 1) return L;
    int64_t t = id % ID_MODULUS;
    int nd = 1;
    for (int64_t q = t / 10; q > 0; q /= 10) ++nd;
    const int tw = (GLYPH_PITCH * nd - 1) * s, th = GLYPH_H * s;
    if (w < tw + 2 * s || h < th + 2 * s) return L;
    for (int k = nd - 1; k >= 0; --k) L.digit[k] = (uint8_t)(t % 10), t /= 10;
    // the centroid, held to a range in which the sums below cannot overflow; the clamp to the frame makes the result the same
    const int64_t big = (int64_t)1 << 40;
    int64_t cx = floor_div(sum_x, area), cy = floor_div(sum_y, area);
    cx = cx < -big ? -big : cx > big ? big : cx;
    cy = cy < -big ? -big : cy > big ? big : cy;
    int64_t x0 = cx - tw / 2, y0 = cy - th / 2;
    x0 = x0 < s ? s : x0;
    y0 = y0 < s ? s : y0;
    x0 = x0 > w - tw - s ? w - tw - s : x0;
    y0 = y0 > h - th - s ? h - th - s : y0;
    L.nd = nd, L.x0 = (int)x0, L.y0 = (int)y0, L.tw = tw, L.th = th;
    return L;
}

// the marks of pixel (x, y) of the halo rectangle [x0 - s, x0 + tw + s) x [y0 - s, y0 + th + s) of a label whose glyphs are
// glyph[k] = glyph_bits(digit[k])
FS_OVL_HD int label_marks(const Label& L, const uint64_t* glyph, int s, int x, int y) {
    int bits = MARK_HALO;
    if (x >= L.x0 && x < L.x0 + L.tw && y >= L.y0 && y < L.y0 + L.th) {
        const int u = (x - L.x0) / s, v = (y - L.y0) / s;
        const int k = u / GLYPH_PITCH, col = u % GLYPH_PITCH;
        if (col < GLYPH_W && ((glyph[k] >> (5 * v + 4 - col)) & 1)) bits |= MARK_INK;
    }
    return bits;
}

}  // namespace ovl
}  // namespace fs

#endif  // FS_OVERLAY_DEFS_H_
