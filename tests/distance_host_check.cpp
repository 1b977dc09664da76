// The integer rules of csrc/distance_ops.hip (mask_distance) on the CPU, serially, through the same distance_defs.h functions the kernels
// call: the class-set test, the 64-row chunk words with their carries, the column tie rule, the row scan with its stop rule, the report.
// Built by tests/test_distance_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads the cases from the file named on
// the command line:
//   int32 entries;  per entry: int32 n, H, W, source_set, R, want_nearest;  uint8 mask [n][H][W]
// and prints, per entry, "case i", then one line "d2 nearest" per pixel (nearest as 0 without the plane).  Before the cases, the packing
// and the stop rule at their limits (the sanitizer watches them).
#include "distance_defs.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fs;

static int limits() {
    int bad = 0;
    const uint64_t far = dst::candidate(0, 32767, 32767u, 32767, 32768);  // the largest distance a frame can hold
    bad += dst::cand_d2(far) != 2147352578u || dst::cand_raster(far) != 32767u * 32768u + 32767u || far >= dst::NO_CANDIDATE;
    bad += dst::candidate(5, 3, dst::NO_ROW, 0, 8) != dst::NO_CANDIDATE;
    bad += dst::better(dst::pack(4, 9), dst::pack(4, 7)) != dst::pack(4, 7) || dst::better(dst::pack(3, 9), dst::pack(4, 7)) != dst::pack(3, 9);
    bad += dst::scan_stops(2, dst::pack(4, 0), 0, true) || !dst::scan_stops(3, dst::pack(4, 0), 0, true) || !dst::scan_stops(2, dst::pack(4, 0), 0, false);
    bad += dst::scan_stops(32767, dst::NO_CANDIDATE, 0, true) || !dst::scan_stops(8, dst::NO_CANDIDATE, 7, true) || dst::scan_stops(7, dst::NO_CANDIDATE, 7, true);
    bad += dst::column_pick(5, 3, 7) != 3 || dst::column_pick(5, 2, 7) != 7 || dst::column_pick(5, -1, 7) != 7 || dst::column_pick(5, 3, -1) != 3;
    bad += dst::column_pick(5, -1, -1) != -1 || dst::column_pick(5, 5, 5) != 5;
    const uint64_t ends = ((uint64_t)1 << 63) | 1u;
    bad += dst::chunk_up(ends, 128, 62) != 128 || dst::chunk_up(ends, 128, 63) != 191 || dst::chunk_down(ends, 128, 1) != 191 || dst::chunk_down(ends, 128, 0) != 128;
    bad += dst::chunk_up(0, 0, 63) != -1 || dst::chunk_down(0, 0, 0) != -1 || dst::chunk_down((uint64_t)1, 0, 1) != -1;
    bad += dst::in_set(32, 1u) || dst::in_set(33, 2u) || dst::in_set(255, 0xFFFFFFFFu) || !dst::in_set(31, 0x80000000u) || dst::in_set(1, 1u);
    uint32_t d2;
    int32_t q;
    dst::report(dst::pack(50, 11), 7, &d2, &q);
    bad += d2 != dst::NONE || q != -1;
    dst::report(dst::pack(49, 11), 7, &d2, &q);
    bad += d2 != 49u || q != 11;
    dst::report(far, 0, &d2, &q);
    bad += d2 != 2147352578u || q != 1073741823;
    const int thr[3] = {0, 2, 32767};
    bad += dst::first_bin(0, thr, 3) != 0 || dst::first_bin(4, thr, 3) != 1 || dst::first_bin(5, thr, 3) != 2 || dst::first_bin(1073676290u, thr, 3) != 3;
    bad += dst::first_bin(dst::NONE, thr, 3) != 3;
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (int bad = limits()) {
        std::fprintf(stderr, "limits: %d wrong\n", bad);
        return 1;
    }
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    int32_t entries = 0;
    if (std::fread(&entries, 4, 1, fh) != 1) return 2;
    for (int i = 0; i < entries; ++i) {
        int32_t head[6];
        if (std::fread(head, 4, 6, fh) != 6) return 2;
        const int n = head[0], H = head[1], W = head[2], R = head[4];
        const uint32_t set = (uint32_t)head[3];
        const bool want_nearest = head[5] != 0;
        std::vector<uint8_t> mask((size_t)n * H * W);
        if (std::fread(mask.data(), 1, mask.size(), fh) != mask.size()) return 2;
        const int chunks = (H + dst::CHUNK - 1) / dst::CHUNK;
        std::printf("case %d\n", i);
        for (int f = 0; f < n; ++f) {
            const uint8_t* m = mask.data() + (size_t)f * H * W;
            // the column pass, as the two column kernels run it: the chunk words, their first and last rows, the carries, the pick
            std::vector<uint64_t> bits((size_t)chunks * W, 0);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (dst::in_set(m[(size_t)y * W + x], set)) bits[(size_t)(y / dst::CHUNK) * W + x] |= (uint64_t)1 << (y % dst::CHUNK);
            std::vector<uint16_t> rows((size_t)H * W);
            for (int c = 0; c < chunks; ++c)
                for (int x = 0; x < W; ++x) {
                    int above = -1, below = -1;
                    for (int k = c - 1; k >= 0 && above < 0; --k) above = dst::chunk_up(bits[(size_t)k * W + x], k * dst::CHUNK, 63);
                    for (int k = c + 1; k < chunks && below < 0; ++k) below = dst::chunk_down(bits[(size_t)k * W + x], k * dst::CHUNK, 0);
                    const int y0 = c * dst::CHUNK;
                    for (int r = 0; r < dst::CHUNK && y0 + r < H; ++r) {
                        int up = dst::chunk_up(bits[(size_t)c * W + x], y0, r), down = dst::chunk_down(bits[(size_t)c * W + x], y0, r);
                        if (up < 0) up = above;
                        if (down < 0) down = below;
                        const int pick = dst::column_pick(y0 + r, up, down);
                        rows[(size_t)(y0 + r) * W + x] = pick < 0 ? (uint16_t)dst::NO_ROW : (uint16_t)pick;
                    }
                }
            // the row pass
            for (int y = 0; y < H; ++y) {
                const uint16_t* row = rows.data() + (size_t)y * W;
                for (int x = 0; x < W; ++x) {
                    uint32_t d2;
                    int32_t q;
                    dst::report(dst::scan_row(row, y, x, W, H, R, want_nearest), R, &d2, &q);
                    std::printf("%u %d\n", d2, want_nearest ? q : 0);
                }
            }
        }
    }
    std::fclose(fh);
    return 0;
}
