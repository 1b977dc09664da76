// The integer rules of the dry-route cost field and its tabulation (access_ops.hip; definitions: include/floodseg_test.h, mask_access
// and region_access).  Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these functions, and a
// host program (tests/test_access_cpu.py builds tests/access_host_check.cpp) runs them on the CPU.
#ifndef FS_ACCESS_DEFS_H_
#define FS_ACCESS_DEFS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_ACC_HD __host__ __device__ __forceinline__
#else
#define FS_ACC_HD inline
#endif

namespace fs {
namespace acc {

constexpr int MAX_SIDE = 32768;                      // H, W: the range of mask_distance
constexpr int MAX_CLASSES = 32;                      // the cost table and the bits of terminal_set; ids at or above it are barriers
constexpr uint32_t NONE = 0xFFFFFFFFu;               // FS_ACCESS_NONE
constexpr uint32_t MAX_COST = 0x7FFFF000u;           // the largest R: 2^31 - 4096, so that a value plus one move stays below 2^31
constexpr int MAX_ROUNDS = 65535;
constexpr int STEP_ORTHO = 5, STEP_DIAG = 7;         // a move costs step * (cost[from] + cost[to])
constexpr uint32_t MAX_MOVE = STEP_DIAG * 2u * 255u; // 3570

// ---- THE MOVE TABLE, in the order every tie between neighbours is broken in (access_route): the four orthogonal moves, then the
// four diagonal ones.  Move k goes FROM p + (DX[k], DY[k]) TO p when p gathers, and from p to p + (DX[k], DY[k]) when a route is read.
constexpr int MOVES = 8;
FS_ACC_HD int move_dx(int k) { return k == 0 ? -1 : k == 1 ? 1 : k < 4 ? 0 : (k & 1) ? 1 : -1; }      // W E N S NW NE SW SE
FS_ACC_HD int move_dy(int k) { return k < 2 ? 0 : k == 2 ? -1 : k == 3 ? 1 : k < 6 ? -1 : 1; }
FS_ACC_HD int move_step(int k) { return k < 4 ? STEP_ORTHO : STEP_DIAG; }
FS_ACC_HD int move_count(int connectivity) { return connectivity == 8 ? 8 : 4; }

// ---- what a mask id is: its walking cost in the low byte (0: barrier), bit 8 set where it is terminal.  A terminal class without a
// cost is a barrier like any other.
constexpr uint32_t TERMINAL = 0x100u;
FS_ACC_HD uint32_t kind_of(int id, const uint8_t* cost, uint32_t terminal_set) {
    if (id < 0 || id >= MAX_CLASSES || cost[id] == 0) return 0u;
    return (uint32_t)cost[id] | (((terminal_set >> id) & 1u) ? TERMINAL : 0u);
}
FS_ACC_HD bool passable(uint32_t kind) { return kind != 0u && (kind & TERMINAL) == 0u; }
FS_ACC_HD bool enterable(uint32_t kind) { return kind != 0u; }  // passable or terminal
FS_ACC_HD uint32_t cost_of(uint32_t kind) { return kind & 0xFFu; }

// ---- THE ALLOWED-MOVE TEST: the cost of move k from a pixel of kind `from` to one of kind `to`, 0 where the move is not allowed.
// side_a and side_b are the kinds of the two pixels orthogonally between them; they are looked at for a diagonal move only.
FS_ACC_HD uint32_t move_cost(int k, uint32_t from, uint32_t to, uint32_t side_a, uint32_t side_b) {
    if (!passable(from) || !enterable(to)) return 0u;
    if (k >= 4 && !(passable(side_a) && passable(side_b))) return 0u;  // no corner cutting
    return (uint32_t)move_step(k) * (cost_of(from) + cost_of(to));
}

// ---- THE KEY: the cost in the high dword, the origin's raster index in the low one, so that the smaller 64-bit word is the cheaper
// route and, at equal cost, the one from the seed with the smaller raster index.  NO_KEY is larger than every key; its halves are
// FS_ACCESS_NONE and -1.
constexpr uint64_t NO_KEY = ~(uint64_t)0;
FS_ACC_HD uint64_t make_key(uint32_t d, uint32_t origin) { return ((uint64_t)d << 32) | origin; }
FS_ACC_HD uint32_t key_cost(uint64_t key) { return (uint32_t)(key >> 32); }
FS_ACC_HD int32_t key_origin(uint64_t key) { return (int32_t)(uint32_t)key; }

// the largest cost that is reported: R, or MAX_COST for R = 0
FS_ACC_HD uint32_t bound_of(uint32_t max_cost) { return max_cost == 0u ? MAX_COST : max_cost; }

// what the neighbour's key offers across a move of cost w (0: not allowed): NO_KEY without an offer or beyond the bound.  A key that
// is not NO_KEY carries a cost <= MAX_COST, so the sum stays below 2^31.
FS_ACC_HD uint64_t offer(uint64_t neighbour, uint32_t w, uint32_t bound) {
    if (w == 0u || neighbour == NO_KEY) return NO_KEY;
    const uint32_t d = key_cost(neighbour);
    if (d > bound || w > bound - d) return NO_KEY;
    return neighbour + ((uint64_t)w << 32);
}
FS_ACC_HD uint64_t better(uint64_t a, uint64_t b) { return b < a ? b : a; }

// a pixel's key before the first round: its own raster index at cost 0 where it is a seed that counts
FS_ACC_HD uint64_t seed_key(uint32_t kind, int seed, uint32_t raster, bool want_origin) {
    return seed != 0 && passable(kind) ? make_key(0u, want_origin ? raster : 0u) : NO_KEY;
}
// a pixel's key as the planes of an earlier call hold it (resume); a plane's word is taken as it is and never used as an index
FS_ACC_HD uint64_t plane_key(uint32_t d, int32_t origin, bool want_origin) {
    return d == NONE || d > MAX_COST ? NO_KEY : make_key(d, want_origin ? (uint32_t)origin : 0u);
}

// ---- ONE GATHER of pixel (x, y): the best of its own key and its neighbours' offers.  `keys` and `kinds` answer for every pixel of
// the frame and for the ring of one pixel around it (NO_KEY and 0 there).
template <class Keys, class Kinds>
FS_ACC_HD uint64_t gather(const Keys& keys, const Kinds& kinds, int x, int y, int connectivity, uint32_t bound) {
    uint64_t best = keys(x, y);
    const uint32_t to = kinds(x, y);
    if (!enterable(to)) return best;
    for (int k = 0; k < move_count(connectivity); ++k) {
        const int dx = move_dx(k), dy = move_dy(k);
        const uint32_t w = move_cost(k, kinds(x + dx, y + dy), to, kinds(x + dx, y), kinds(x, y + dy));
        best = better(best, offer(keys(x + dx, y + dy), w, bound));
    }
    return best;
}

}  // namespace acc
}  // namespace fs
#endif  // FS_ACCESS_DEFS_H_
