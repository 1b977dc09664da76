// Stand-alone host program for tests/test_overlay_cpu.py: csrc/overlay_defs.h compiled by the host compiler.  Reads scenes of region
// rows from a binary file and prints, for every row that gets a label, its text box and the ink cells of its halo rectangle, through
// the very functions the stamp kernel calls (make_label, glyph_bits, label_marks).
// File: int32 scenes; per scene int64 [6] = (h, w, scale, min_area, R, live), then R rows int64 [4] = (id, area, sum_x, sum_y).
// Output: "scene c", then per labelled row "r x0 y0 tw th text" and one line "ink" followed by x,y pairs in raster order; every pixel
// of the halo rectangle must carry the halo bit, and no pixel outside the text box may carry ink (checked here, exit status 2).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "overlay_defs.h"

int main(int argc, char** argv) {
    if (argc != 2) return 64;
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 65;
    int32_t scenes = 0;
    if (std::fread(&scenes, sizeof scenes, 1, fh) != 1) return 66;
    for (int c = 0; c < scenes; ++c) {
        int64_t head[6];
        if (std::fread(head, sizeof head, 1, fh) != 1) return 66;
        const int h = (int)head[0], w = (int)head[1], s = (int)head[2], R = (int)head[4];
        const int64_t min_area = head[3], live = head[5];
        std::vector<int64_t> rows((size_t)R * 4);
        if (R && std::fread(rows.data(), sizeof(int64_t), rows.size(), fh) != rows.size()) return 66;
        std::printf("scene %d\n", c);
        for (int r = 0; r < R; ++r) {
            const int64_t* t = &rows[(size_t)r * 4];
            const fs::ovl::Label L = fs::ovl::make_label(r, live < R ? live : R, t[0], t[1], t[2], t[3], min_area, h, w, s);
            if (L.nd == 0) continue;
            uint64_t glyph[fs::ovl::MAX_DIGITS] = {};
            std::printf("%d %d %d %d %d ", r, L.x0, L.y0, L.tw, L.th);
            for (int k = 0; k < L.nd; ++k) {
                glyph[k] = fs::ovl::glyph_bits(L.digit[k]);
                std::printf("%d", (int)L.digit[k]);
            }
            std::printf("\nink");
            if (L.x0 - s < 0 || L.y0 - s < 0 || L.x0 + L.tw + s > w || L.y0 + L.th + s > h) return 2;  // the rectangle lies inside the frame
            for (int y = L.y0 - s; y < L.y0 + L.th + s; ++y)
                for (int x = L.x0 - s; x < L.x0 + L.tw + s; ++x) {
                    const int bits = fs::ovl::label_marks(L, glyph, s, x, y);
                    if (!(bits & fs::ovl::MARK_HALO)) return 2;
                    const bool in_box = x >= L.x0 && x < L.x0 + L.tw && y >= L.y0 && y < L.y0 + L.th;
                    if ((bits & fs::ovl::MARK_INK) && !in_box) return 2;
                    if (bits & fs::ovl::MARK_INK) std::printf(" %d,%d", x, y);
                }
            std::printf("\n");
        }
    }
    std::fclose(fh);
    return 0;
}
