// The rules of csrc/refine_ops.hip on the CPU, serially, through the same refine_defs.h functions the kernels call.  Built by
// tests/test_refine_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on the command
// line, one per line, and prints one line of integers per command:
//   usable pose[16]                                     -> 0 | 1
//   pixel to[6] x y ox oy                               -> X Y
//   old rank ordinal min_age                            -> 0 | 1
//   luma r g b                                          -> luma
//   view H W CH CW ox oy ordinal min_age pose[16], then CH x CW rank words, then CH x CW rgba words
//                                                       -> H x W view bytes, then H x W valid bytes: map_view's steps, pixel by pixel
//   gate H W rows, then H x W valid bytes, then rows x 7 table words
//                                                       -> rows x 7 words: the gated table
//   step H W CH CW ox oy model[16] state[32] pose[16]   -> out[8] state[32] pose[16]
#include "refine_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fs;

static FILE* in;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "refine_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
static unsigned long long uword() {
    unsigned long long v = 0;
    if (fscanf(in, "%llu", &v) != 1) {
        fprintf(stderr, "refine_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
static void words(int64_t* out, int count) {
    for (int i = 0; i < count; ++i) out[i] = word();
}

static void view() {
    const int H = (int)word(), W = (int)word(), CH = (int)word(), CW = (int)word(), ox = (int)word(), oy = (int)word();
    const uint32_t ordinal = (uint32_t)uword();
    const int min_age = (int)word();
    int64_t pose[mos::POSE_WORDS];
    words(pose, mos::POSE_WORDS);
    std::vector<uint64_t> rank((size_t)CH * CW);
    std::vector<uint32_t> rgba((size_t)CH * CW);
    for (auto& v : rank) v = uword();
    for (auto& v : rgba) v = (uint32_t)uword();
    std::vector<int> seen((size_t)H * W, 0), valid((size_t)H * W, 0);
    const bool usable = refn::view_usable(pose);
    for (int y = 0; y < H && usable; ++y)
        for (int x = 0; x < W; ++x) {
            int64_t X, Y;
            refn::canvas_pixel(pose, x, y, ox, oy, &X, &Y);
            if (!refn::in_canvas(X, Y, CH, CW)) continue;
            const size_t cell = (size_t)Y * CW + (size_t)X;
            if (!refn::seen(rgba[cell])) continue;
            if (min_age > 0 && !refn::old_enough(rank[cell], ordinal, min_age)) continue;
            seen[(size_t)y * W + x] = (int)refn::luma_of(rgba[cell]), valid[(size_t)y * W + x] = 1;
        }
    for (size_t i = 0; i < seen.size(); ++i) printf("%s%d", i ? " " : "", seen[i]);
    for (size_t i = 0; i < valid.size(); ++i) printf(" %d", valid[i]);
    printf("\n");
}

static void gate() {
    const int H = (int)word(), W = (int)word(), rows = (int)word();
    std::vector<uint8_t> valid((size_t)H * W);  // exactly the plane: a read outside it is the sanitizer's to find
    for (auto& v : valid) v = (uint8_t)word();
    for (int r = 0; r < rows; ++r) {
        int32_t row[refn::ROW_WORDS];
        for (int i = 0; i < refn::ROW_WORDS; ++i) row[i] = (int32_t)word();
        if (!refn::gate_keeps(row, valid.data(), H, W)) refn::void_row(row);
        for (int i = 0; i < refn::ROW_WORDS; ++i) printf("%s%d", r || i ? " " : "", row[i]);
    }
    printf("\n");
}

static void step() {
    const int H = (int)word(), W = (int)word(), CH = (int)word(), CW = (int)word(), ox = (int)word(), oy = (int)word();
    int64_t model[mos::MODEL_WORDS], state[mos::STATE_WORDS], pose[mos::POSE_WORDS], out[refn::OUT_WORDS];
    words(model, mos::MODEL_WORDS);
    words(state, mos::STATE_WORDS);
    words(pose, mos::POSE_WORDS);
    refn::refine_step(model, state, pose, out, H, W, CH, CW, ox, oy);
    for (int i = 0; i < refn::OUT_WORDS; ++i) printf("%s%lld", i ? " " : "", (long long)out[i]);
    for (int i = 0; i < mos::STATE_WORDS; ++i) printf(" %lld", (long long)state[i]);
    for (int i = 0; i < mos::POSE_WORDS; ++i) printf(" %lld", (long long)pose[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: refine_host_check COMMANDS\n");
        return 2;
    }
    char op[16];
    while (fscanf(in, "%15s", op) == 1) {
        if (!strcmp(op, "usable")) {
            int64_t pose[mos::POSE_WORDS];
            words(pose, mos::POSE_WORDS);
            printf("%d\n", refn::view_usable(pose) ? 1 : 0);
        } else if (!strcmp(op, "pixel")) {
            int64_t to[6], X, Y;
            words(to, 6);
            const int x = (int)word(), y = (int)word(), ox = (int)word(), oy = (int)word();
            refn::canvas_pixel(to, x, y, ox, oy, &X, &Y);
            printf("%lld %lld\n", (long long)X, (long long)Y);
        } else if (!strcmp(op, "old")) {
            const uint64_t rank = uword();
            const uint32_t ordinal = (uint32_t)uword();
            printf("%d\n", refn::old_enough(rank, ordinal, (int)word()) ? 1 : 0);
        } else if (!strcmp(op, "luma")) {
            const uint32_t r = (uint32_t)word(), g = (uint32_t)word(), b = (uint32_t)word();
            printf("%u\n", refn::luma(r, g, b));
        } else if (!strcmp(op, "view")) {
            view();
        } else if (!strcmp(op, "gate")) {
            gate();
        } else if (!strcmp(op, "step")) {
            step();
        } else {
            fprintf(stderr, "refine_host_check: unknown command %s\n", op);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
