// The per-pixel transition of csrc/stabilize_ops.hip (mask_stabilize, the in-place route) on the CPU, serially, through the same
// stabilize_defs.h functions the kernels call.  Built by tests/test_stabilize_cpu.py with -fsanitize=address,undefined as a stand-alone
// program; reads the cases from the file named on the command line:
//   int32 entries;  per entry: int32 n, HW, K, P, T, has_conf, has_state;  uint8 mask [n][HW];  has_conf: uint8 conf [n][HW];
//   has_state: uint32 state [HW]
// and prints, per entry, "case i", then per frame "frame f" and one line "out state" per pixel (the state in hex), then
// "counts held switched seeded trusted".  Before the cases, the packing at its limits (the sanitizer watches it).
#include "stabilize_defs.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fs;

template <class T>
static bool read_all(FILE* fh, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), fh) == v.size(); }

static int limits() {
    int bad = 0, out;
    uint32_t ev;
    const uint32_t top = stb::pack(255, 255, 255);
    bad += top != 0x80ffffffu || stb::emitted(top) != 255 || stb::candidate(top) != 255 || stb::run(top) != 255 || !stb::valid(top) || stb::valid(0u);
    bad += stb::step(stb::pack(0, 1, 255), 1, 2, 255, false, &out, &ev) != stb::pack(1, 1, 0) || ev != stb::EV_SWITCHED;  // the cap reaches P = 255
    bad += stb::step(stb::pack(0, 1, 254), 1, 2, 255, false, &out, &ev) != stb::pack(1, 1, 0);
    bad += stb::step(stb::pack(0, 1, 253), 1, 2, 255, false, &out, &ev) != stb::pack(0, 1, 254) || out != 0 || ev != stb::EV_HELD;
    bad += stb::trusted(-1, 0) || !stb::trusted(0, 0) || stb::trusted(255, 256) || !stb::trusted(200, 200) || stb::trusted(199, 200);
    bad += 4 * stb::EV_HELD + 4 * stb::EV_SWITCHED + 4 * stb::EV_SEEDED + 4 * stb::EV_TRUSTED != 0x04040404u;  // four pixels: no carry
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
        int32_t h[7];
        if (std::fread(h, 4, 7, fh) != 7) return 2;
        const int n = h[0], HW = h[1], K = h[2], P = h[3], T = h[4], has_conf = h[5], has_state = h[6];
        std::vector<uint8_t> mask((size_t)n * HW), conf(has_conf ? (size_t)n * HW : 0);
        std::vector<uint32_t> state(has_state ? HW : 0);
        if (!read_all(fh, mask) || !read_all(fh, conf) || !read_all(fh, state)) return 2;
        state.resize(HW, 0u);
        std::printf("case %d\n", i);
        for (int f = 0; f < n; ++f) {
            long long held = 0, switched = 0, seeded = 0, trusted = 0;
            std::printf("frame %d\n", f);
            for (int p = 0; p < HW; ++p) {
                int out;
                uint32_t ev;
                const size_t at = (size_t)f * HW + p;
                state[p] = stb::step(state[p], mask[at], K, P, stb::trusted(has_conf ? conf[at] : -1, T), &out, &ev);
                std::printf("%d %x\n", out, state[p]);
                held += ev & 0xffu, switched += (ev >> 8) & 0xffu, seeded += (ev >> 16) & 0xffu, trusted += ev >> 24;
            }
            std::printf("counts %lld %lld %lld %lld\n", held, switched, seeded, trusted);
        }
    }
    std::fclose(fh);
    return 0;
}
