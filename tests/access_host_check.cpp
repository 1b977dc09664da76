// The rules of csrc/access_ops.hip on the CPU, serially, through the same access_defs.h functions the kernels call.  Built by
// tests/test_access_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on the command
// line and prints one line of integers per command.  Planes and staged tiles are exactly as large as they say: a read outside one is
// the sanitizer's to find.
//   field H W connectivity max_cost want_origin rounds terminal_set cost[32], then mask [H W], seeds [H W]
//                                                              -> converged valued, then d [H W], origin [H W]
// The frame is relaxed as the kernels relax it: tile by tile of TILE x TILE pixels with a ring of one pixel staged beside it (NO_KEY and
// kind 0 outside the frame), gathers from the staged copy until a sweep lowers nothing or SWEEPS sweeps are done, the lowered keys written
// back, and the neighbour tiles whose ring holds a lowered pixel marked for the next round; a tile that is not marked is skipped.  The
// tiles of a round run one after the other here, which is one of the orders the GPU may produce.
#include "access_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fs;

static FILE* in;
constexpr int TILE = 32, LW = TILE + 2, SWEEPS = 4 * TILE;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "access_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}

struct Staged {
    std::vector<uint64_t> key;
    std::vector<uint32_t> kind;
    int x0, y0;  // the frame pixel of staged (1, 1)
    uint64_t keys(int x, int y) const { return key.at((size_t)(y - y0 + 1) * LW + (x - x0 + 1)); }
    uint32_t kinds(int x, int y) const { return kind.at((size_t)(y - y0 + 1) * LW + (x - x0 + 1)); }
};

static void field() {
    const int H = (int)word(), W = (int)word(), conn = (int)word();
    const uint32_t max_cost = (uint32_t)word();
    const bool want_origin = word() != 0;
    const int rounds = (int)word();
    const uint32_t terminal_set = (uint32_t)word();
    uint8_t cost[acc::MAX_CLASSES];
    for (auto& c : cost) c = (uint8_t)word();
    std::vector<uint8_t> mask((size_t)H * W), seeds((size_t)H * W);
    for (auto& v : mask) v = (uint8_t)word();
    for (auto& v : seeds) v = (uint8_t)word();
    if (H < 1 || W < 1 || H > acc::MAX_SIDE || W > acc::MAX_SIDE || (conn != 4 && conn != 8) || max_cost > acc::MAX_COST || rounds < 1 || rounds > acc::MAX_ROUNDS)
        exit(3);
    const uint32_t bound = acc::bound_of(max_cost);
    std::vector<uint64_t> keys((size_t)H * W);
    for (int i = 0; i < H * W; ++i) keys[i] = acc::seed_key(acc::kind_of(mask[i], cost, terminal_set), seeds[i], (uint32_t)i, want_origin);
    const int tx = (W + TILE - 1) / TILE, ty = (H + TILE - 1) / TILE;
    std::vector<uint8_t> dirty((size_t)tx * ty, 1), next((size_t)tx * ty, 0);
    for (int round = 0; round < rounds; ++round) {
        for (int by = 0; by < ty; ++by)
            for (int bx = 0; bx < tx; ++bx) {
                if (!dirty[(size_t)by * tx + bx]) continue;
                dirty[(size_t)by * tx + bx] = 0;
                Staged st{std::vector<uint64_t>((size_t)LW * LW), std::vector<uint32_t>((size_t)LW * LW), bx * TILE, by * TILE};
                for (int i = 0; i < LW * LW; ++i) {
                    const int gx = st.x0 + i % LW - 1, gy = st.y0 + i / LW - 1;
                    const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
                    st.key[i] = inside ? keys[(size_t)gy * W + gx] : acc::NO_KEY;
                    st.kind[i] = inside ? acc::kind_of(mask[(size_t)gy * W + gx], cost, terminal_set) : 0u;
                }
                const std::vector<uint64_t> was = st.key;
                bool changed = true;
                for (int sweep = 0; sweep < SWEEPS && changed; ++sweep) {
                    std::vector<uint64_t> best((size_t)TILE * TILE);
                    for (int ly = 0; ly < TILE; ++ly)
                        for (int lx = 0; lx < TILE; ++lx)
                            best[(size_t)ly * TILE + lx] = acc::gather([&](int x, int y) { return st.keys(x, y); }, [&](int x, int y) { return st.kinds(x, y); },
                                                                       st.x0 + lx, st.y0 + ly, conn, bound);
                    changed = false;
                    for (int ly = 0; ly < TILE; ++ly)
                        for (int lx = 0; lx < TILE; ++lx) {
                            uint64_t& cell = st.key[(size_t)(ly + 1) * LW + lx + 1];
                            if (best[(size_t)ly * TILE + lx] < cell) cell = best[(size_t)ly * TILE + lx], changed = true;
                        }
                }
                if (changed) next[(size_t)by * tx + bx] = 1;
                for (int ly = 0; ly < TILE; ++ly)
                    for (int lx = 0; lx < TILE; ++lx) {
                        const size_t li = (size_t)(ly + 1) * LW + lx + 1;
                        if (!(st.key[li] < was[li])) continue;
                        if (st.x0 + lx >= W || st.y0 + ly >= H) exit(4);  // only a pixel inside the frame is ever lowered
                        keys[(size_t)(st.y0 + ly) * W + st.x0 + lx] = st.key[li];
                        for (int k = 0; k < acc::MOVES; ++k) {
                            const int dx = acc::move_dx(k), dy = acc::move_dy(k), nx = bx + dx, ny = by + dy;
                            const bool edge_x = dx == 0 || (dx < 0 ? lx == 0 : lx == TILE - 1), edge_y = dy == 0 || (dy < 0 ? ly == 0 : ly == TILE - 1);
                            if (edge_x && edge_y && nx >= 0 && nx < tx && ny >= 0 && ny < ty) next[(size_t)ny * tx + nx] = 1;
                        }
                    }
            }
        dirty.swap(next);
        std::fill(next.begin(), next.end(), 0);
    }
    int converged = 1;
    long long valued = 0;
    for (auto v : dirty) converged &= !v;
    for (auto k : keys) valued += k != acc::NO_KEY;
    printf("%d %lld", converged, valued);
    for (auto k : keys) printf(" %u", acc::key_cost(k));
    for (auto k : keys) printf(" %d", k == acc::NO_KEY ? -1 : (want_origin ? acc::key_origin(k) : 0));
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: access_host_check COMMANDS.txt\n");
        return 2;
    }
    char cmd[32];
    while (fscanf(in, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "field")) field();
        else {
            fprintf(stderr, "access_host_check: unknown command %s\n", cmd);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
