// The rules of csrc/ortho_ops.hip on the CPU, serially, through the same ortho_defs.h (and mosaic_defs.h) functions the kernels call.
// Built by tests/test_ortho_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on the
// command line, one per line, and prints one line of integers per command:
//   key x y H W                                        -> centre_key
//   rank mode x y H W ordinal                          -> rank ordinal-of-rank
//   replaces rank stored                               -> 0 | 1
//   cand from[6] X Y ox oy H W mode ordinal            -> ok x y rank (zeros when there is no pixel)
//   gather CH CW ox oy H W mode frames, then per frame pose[16] ordinal
//                                                      -> CH x CW ranks, then CH x CW winning frame pixels y W + x (-1: empty): the
//                                                         kernel's steps, tile by tile with the tile test, one frame after the other
//   pack r g b                                         -> rgba
//   under rgba fill                                    -> rgb
//   takes k K                                          -> 0 | 1
//   edge k edge_set north south west east              -> 0 | 1
#include "ortho_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fs;

static FILE* in;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "ortho_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
static unsigned long long uword() {
    unsigned long long v = 0;
    if (fscanf(in, "%llu", &v) != 1) {
        fprintf(stderr, "ortho_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
static void words(int64_t* out, int count) {
    for (int i = 0; i < count; ++i) out[i] = word();
}

static void gather() {
    const int CH = (int)word(), CW = (int)word(), ox = (int)word(), oy = (int)word(), H = (int)word(), W = (int)word(), mode = (int)word(), frames = (int)word();
    std::vector<uint64_t> rank((size_t)CH * CW, orth::RANK_EMPTY);
    std::vector<long long> pixel((size_t)CH * CW, -1);
    for (int f = 0; f < frames; ++f) {
        int64_t pose[mos::POSE_WORDS];
        words(pose, mos::POSE_WORDS);
        const uint32_t ordinal = (uint32_t)uword();
        if (!mos::pose_votes(pose)) continue;
        for (int Y0 = 0; Y0 < CH; Y0 += 16)
            for (int X0 = 0; X0 < CW; X0 += 64) {
                const int X1 = X0 + 64 < CW ? X0 + 64 : CW, Y1 = Y0 + 16 < CH ? Y0 + 16 : CH;
                if (!mos::touches(pose + 6, X0, Y0, X1, Y1, ox, oy, H, W)) continue;
                for (int Y = Y0; Y < Y1; ++Y)
                    for (int X = X0; X < X1; ++X) {
                        int x, y;
                        uint64_t mine;
                        if (!orth::candidate(pose + 6, X, Y, ox, oy, H, W, mode, ordinal, &x, &y, &mine)) continue;
                        const size_t cell = (size_t)Y * CW + X;
                        if (!orth::replaces(mine, rank[cell])) continue;
                        rank[cell] = mine, pixel[cell] = (long long)y * W + x;
                    }
            }
    }
    for (size_t i = 0; i < rank.size(); ++i) printf("%s%llu", i ? " " : "", (unsigned long long)rank[i]);
    for (size_t i = 0; i < pixel.size(); ++i) printf(" %lld", pixel[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: ortho_host_check COMMANDS\n");
        return 2;
    }
    char op[16];
    while (fscanf(in, "%15s", op) == 1) {
        if (!strcmp(op, "key")) {
            const int x = (int)word(), y = (int)word(), H = (int)word(), W = (int)word();
            printf("%u\n", orth::centre_key(x, y, H, W));
        } else if (!strcmp(op, "rank")) {
            const int mode = (int)word(), x = (int)word(), y = (int)word(), H = (int)word(), W = (int)word();
            const uint64_t r = orth::frame_rank(mode, x, y, H, W, (uint32_t)uword());
            printf("%llu %u\n", (unsigned long long)r, orth::rank_ordinal(r));
        } else if (!strcmp(op, "replaces")) {
            const uint64_t a = uword(), b = uword();
            printf("%d\n", orth::replaces(a, b) ? 1 : 0);
        } else if (!strcmp(op, "cand")) {
            int64_t from[6];
            words(from, 6);
            const int X = (int)word(), Y = (int)word(), ox = (int)word(), oy = (int)word(), H = (int)word(), W = (int)word(), mode = (int)word();
            const uint32_t ordinal = (uint32_t)uword();
            int x = 0, y = 0;
            uint64_t r = 0;
            const bool ok = orth::candidate(from, X, Y, ox, oy, H, W, mode, ordinal, &x, &y, &r);
            printf("%d %d %d %llu\n", ok ? 1 : 0, ok ? x : 0, ok ? y : 0, ok ? (unsigned long long)r : 0ull);
        } else if (!strcmp(op, "gather")) {
            gather();
        } else if (!strcmp(op, "pack")) {
            const uint32_t r = (uint32_t)word(), g = (uint32_t)word(), b = (uint32_t)word();
            printf("%u\n", orth::pack_rgba(r, g, b));
        } else if (!strcmp(op, "under")) {
            const uint32_t rgba = (uint32_t)uword(), fill = (uint32_t)uword();
            printf("%u\n", orth::under_rgb(rgba, fill));
        } else if (!strcmp(op, "takes")) {
            const uint32_t k = (uint32_t)word();
            printf("%d\n", orth::takes_colour(k, (int)word()) ? 1 : 0);
        } else if (!strcmp(op, "edge")) {
            const uint32_t k = (uint32_t)word(), set = (uint32_t)uword(), n = (uint32_t)word(), s = (uint32_t)word(), w = (uint32_t)word(), e = (uint32_t)word();
            printf("%d\n", orth::on_edge(k, set, n, s, w, e) ? 1 : 0);
        } else {
            fprintf(stderr, "ortho_host_check: unknown command %s\n", op);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
