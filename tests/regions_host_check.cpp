// The labelling passes of csrc/region_ops.hip on the CPU: the same region_uf.h functions the kernels call one pixel per thread, called
// here pixel by pixel and tile by tile, in the kernels' order and once more in the reverse order (the result must not depend on it).
// Built by tests/test_regions_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads the cases and the labels it
// has to reproduce from the file named on the command line:
//   int32 entries;  per entry: int32 n, H, W, K, connectivity;  uint8 mask [n][H][W];  int32 labels [n][H][W]
#include "region_uf.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fs;

static void label(const uint8_t* mask, int H, int W, int K, int conn8, bool reverse, int* cells) {
    const int tiles_x = (W + uf::TILE_W - 1) / uf::TILE_W, tiles_y = (H + uf::TILE_H - 1) / uf::TILE_H, T = uf::TILE_H * uf::TILE_W;
    std::vector<uint8_t> cls(T);
    std::vector<int> parent(T);
    for (int tile = 0; tile < tiles_x * tiles_y; ++tile) {  // pass 1: region_tile_kernel, one workgroup after the other
        const int ty0 = tile / tiles_x * uf::TILE_H, tx0 = tile % tiles_x * uf::TILE_W;
        for (int i = 0; i < T; ++i) {
            const int y = ty0 + i / uf::TILE_W, x = tx0 + i % uf::TILE_W;
            cls[i] = (y < H && x < W) ? (uint8_t)uf::region_class(mask[(size_t)y * W + x], K) : (uint8_t)255;
            parent[i] = i;
        }
        for (int j = 0; j < T; ++j) {
            const int i = reverse ? T - 1 - j : j;
            uf::tile_link(cls.data(), parent.data(), i / uf::TILE_W, i % uf::TILE_W, conn8);
        }
        for (int i = 0; i < T; ++i) {
            const int y = ty0 + i / uf::TILE_W, x = tx0 + i % uf::TILE_W;
            if (y < H && x < W) cells[(size_t)y * W + x] = uf::tile_cell(cls.data(), parent.data(), i, ty0, tx0, W);
        }
    }
    const int64_t border = uf::border_count(H, W);  // pass 2: region_border_kernel
    for (int64_t j = 0; j < border; ++j) uf::border_walk(mask, cells, K, H, W, conn8, reverse ? border - 1 - j : j);
    for (int j = 0; j < H * W; ++j) uf::flatten(cells, reverse ? H * W - 1 - j : j);  // pass 3: region_flatten_kernel
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    int entries = 0, bad = 0;
    if (std::fread(&entries, 4, 1, fh) != 1) return 2;
    for (int e = 0; e < entries; ++e) {
        int head[5];
        if (std::fread(head, 4, 5, fh) != 5) return 2;
        const int n = head[0], H = head[1], W = head[2], K = head[3], conn8 = head[4] == 8;
        const size_t HW = (size_t)H * W;
        std::vector<uint8_t> mask(n * HW);
        std::vector<int> want(n * HW), cells(HW);
        if (std::fread(mask.data(), 1, n * HW, fh) != n * HW || std::fread(want.data(), 4, n * HW, fh) != n * HW) return 2;
        for (int f = 0; f < n; ++f)
            for (int reverse = 0; reverse < 2; ++reverse) {
                cells.assign(HW, -7);
                label(mask.data() + f * HW, H, W, K, conn8, reverse != 0, cells.data());
                size_t wrong = 0;
                for (size_t i = 0; i < HW; ++i) wrong += cells[i] != want[f * HW + i];
                if (wrong) {
                    std::printf("entry %d (%d x %d x %d, K %d, connectivity %d) frame %d reverse %d: %zu labels differ\n", e, n, H, W, K, head[4], f, reverse, wrong);
                    ++bad;
                }
            }
    }
    std::fclose(fh);
    std::printf("%d entries, %d mismatching runs\n", entries, bad);
    return bad ? 1 : 0;
}
