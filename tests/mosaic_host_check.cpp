// The rules of csrc/mosaic_ops.hip on the CPU, serially, through the same mosaic_defs.h functions the kernels call.  Built by
// tests/test_mosaic_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on the command
// line, one per line, and prints one line of integers per command:
//   rshr v                                            -> rshr(v)
//   compose a[6] b[6]                                 -> c[6]
//   key count bin                                     -> key count dx dy
//   tol tol_q20 rounds r                              -> T
//   solve s[12]                                       -> ok model[6]
//   finish model[6] FH FW H W                         -> ok fwd[6] inv[6]
//   motion FH FW H W rounds tol_q20 min exclude has_mask rows, then rows x 7 table words, then H x W mask bytes (has_mask)
//                                                     -> the model row [16]: the kernel's steps, one row after the other
//   pose state[32] model[16] H W CH CW ox oy bridge   -> pose[16] state[32]
//   pixel from[6] X Y ox oy                           -> x y
//   touch from[6] X0 Y0 X1 Y1 ox oy H W               -> 0 | 1
//   vote v more                                       -> v'
//   conf most total                                   -> c
#include "mosaic_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fs;

static FILE* in;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "mosaic_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
static void words(int64_t* out, int count) {
    for (int i = 0; i < count; ++i) out[i] = word();
}
static void print(const int64_t* v, int count) {
    for (int i = 0; i < count; ++i) printf("%s%lld", i ? " " : "", (long long)v[i]);
    printf("\n");
}

static bool usable(const int32_t* row, const std::vector<uint8_t>& mask, bool has_mask, uint32_t exclude, int FH, int FW, int H, int W, int* p, int* q, int* dx,
                   int* dy) {
    if (!mos::row_vector(row, FH, FW, dx, dy)) return false;
    if (has_mask && mos::excluded(mask[(size_t)mos::centre_y(row[6], H, FH) * W + mos::centre_x(row[5], W, FW)], exclude)) return false;
    *p = mos::block_p(row[5], FW / 16), *q = mos::block_q(row[6], FH / 16);
    return true;
}

static void motion() {
    const int FH = (int)word(), FW = (int)word(), H = (int)word(), W = (int)word(), rounds = (int)word();
    const int64_t tol = word();
    const int min_inliers = (int)word();
    const uint32_t exclude = (uint32_t)word();
    const bool has_mask = word() != 0;
    const int rows = (int)word();
    std::vector<int32_t> table((size_t)rows * 7);
    for (auto& v : table) v = (int32_t)word();
    std::vector<uint8_t> mask(has_mask ? (size_t)H * W : 0);
    for (auto& v : mask) v = (uint8_t)word();
    std::vector<uint32_t> hist(mos::HIST_BINS, 0u);
    int64_t usable_rows = 0;
    int p, q, dx, dy;
    for (int i = 0; i < rows; ++i)
        if (usable(&table[(size_t)i * 7], mask, has_mask, exclude, FH, FW, H, W, &p, &q, &dx, &dy)) ++hist[mos::hist_bin(dx, dy)], ++usable_rows;
    uint64_t best = 0;
    for (int b = 0; b < mos::HIST_BINS; ++b) {
        const uint64_t k = mos::mode_key(hist[b], b);
        best = k > best ? k : best;
    }
    int64_t model[6] = {(int64_t)mos::key_dx(best) * mos::ONE, 0, 0, (int64_t)mos::key_dy(best) * mos::ONE, 0, 0};
    int64_t inliers = mos::key_count(best);
    int status = usable_rows < min_inliers ? mos::MODEL_FEW : mos::MODEL_OK, done = 0;
    for (int r = 0; r < rounds && status == mos::MODEL_OK; ++r) {
        const int64_t T = mos::round_tolerance(tol, rounds, r);
        int64_t s[mos::SUMS] = {0};
        for (int i = 0; i < rows; ++i)
            if (usable(&table[(size_t)i * 7], mask, has_mask, exclude, FH, FW, H, W, &p, &q, &dx, &dy) && mos::is_inlier(model, p, q, dx, dy, T))
                mos::add_row(s, p, q, dx, dy);
        int64_t next[6];
        const int stop = s[0] < min_inliers ? 1 : !mos::gm_solve(s, next) ? 2 : 0;
        if (stop) {
            if (r == 0) status = stop == 1 ? mos::MODEL_FEW : mos::MODEL_DEGENERATE;
            break;
        }
        memcpy(model, next, sizeof(model));
        inliers = s[0], done = r + 1;
    }
    int64_t fwd[6], inv[6], row[mos::MODEL_WORDS];
    if (status == mos::MODEL_OK && !mos::gm_finish(model, FH, FW, H, W, fwd, inv)) status = mos::MODEL_DEGENERATE;
    if (status != mos::MODEL_OK) mos::identity(fwd), mos::identity(inv);
    mos::write_model(row, fwd, inv, status, usable_rows, inliers, done);
    print(row, mos::MODEL_WORDS);
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: mosaic_host_check COMMANDS\n");
        return 2;
    }
    char op[16];
    while (fscanf(in, "%15s", op) == 1) {
        int64_t a[32], b[16], c[48];
        if (!strcmp(op, "rshr")) {
            c[0] = mos::rshr(word());
            print(c, 1);
        } else if (!strcmp(op, "compose")) {
            words(a, 6), words(b, 6);
            mos::compose(a, b, c);
            print(c, 6);
            mos::compose(a, b, a);  // in place gives the same
            if (memcmp(a, c, 6 * sizeof(int64_t))) return 3;
        } else if (!strcmp(op, "key")) {
            const uint32_t count = (uint32_t)word();
            const int bin = (int)word();
            const uint64_t k = mos::mode_key(count, bin);
            c[0] = (int64_t)k, c[1] = mos::key_count(k), c[2] = mos::key_dx(k), c[3] = mos::key_dy(k);
            print(c, 4);
            if (mos::hist_bin((int)c[2], (int)c[3]) != bin) return 3;
        } else if (!strcmp(op, "tol")) {
            const int64_t tol = word();
            const int rounds = (int)word(), r = (int)word();
            c[0] = mos::round_tolerance(tol, rounds, r);
            print(c, 1);
        } else if (!strcmp(op, "solve")) {
            words(a, 12);
            for (int i = 0; i < 6; ++i) c[1 + i] = 0;
            c[0] = mos::gm_solve(a, c + 1) ? 1 : 0;
            print(c, 7);
        } else if (!strcmp(op, "finish")) {
            words(a, 6);
            const int FH = (int)word(), FW = (int)word(), H = (int)word(), W = (int)word();
            c[0] = mos::gm_finish(a, FH, FW, H, W, c + 1, c + 7) ? 1 : 0;
            print(c, 13);
        } else if (!strcmp(op, "motion")) {
            motion();
        } else if (!strcmp(op, "pose")) {
            words(a, 32), words(b, 16);
            const int H = (int)word(), W = (int)word(), CH = (int)word(), CW = (int)word(), ox = (int)word(), oy = (int)word(), bridge = (int)word();
            mos::pose_step(b, a, c, H, W, CH, CW, ox, oy, bridge);
            memcpy(c + 16, a, 32 * sizeof(int64_t));
            print(c, 48);
        } else if (!strcmp(op, "pixel")) {
            words(a, 6);
            const int X = (int)word(), Y = (int)word(), ox = (int)word(), oy = (int)word();
            mos::source_pixel(a, mos::anchor_coord(X, ox), mos::anchor_coord(Y, oy), c, c + 1);
            print(c, 2);
        } else if (!strcmp(op, "touch")) {
            words(a, 6);
            const int X0 = (int)word(), Y0 = (int)word(), X1 = (int)word(), Y1 = (int)word(), ox = (int)word(), oy = (int)word(), H = (int)word(), W = (int)word();
            c[0] = mos::touches(a, X0, Y0, X1, Y1, ox, oy, H, W) ? 1 : 0;
            print(c, 1);
        } else if (!strcmp(op, "vote")) {
            const uint16_t v = (uint16_t)word();
            c[0] = mos::vote_add(v, (uint32_t)word());
            print(c, 1);
        } else if (!strcmp(op, "conf")) {
            const uint32_t most = (uint32_t)word();
            c[0] = mos::vote_confidence(most, (uint32_t)word());
            print(c, 1);
        } else {
            fprintf(stderr, "mosaic_host_check: unknown command %s\n", op);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
