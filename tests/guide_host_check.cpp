// The rules of guide_vectors (csrc/motion_ops.hip) on the CPU, serially, through the same guide_defs.h functions the kernel calls.  Built
// by tests/test_guide_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on the
// command line, one per line, and prints one line of integers per command:
//   predict model[16] cx cy                      -> guides gx gy pdx pdy          (zeros behind guides = 0: no product is formed)
//   avail pdx pdy cx cy FH FW                    -> 0 | 1
//   class row[7] cx cy                           -> class dx dy
//   outlier dx dy gx gy outlier_q20              -> 0 | 1
//   evidence sad penalty pdx pdy cost bias       -> cost_g replaces
//   row FH FW fill_void outlier_q20 has_evidence sad penalty cost bias model[16] cx cy row[7]
//                                                -> decision class outlier out[7]: the kernel's steps for one block, in its order
#include "guide_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace fs;

static FILE* in;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "guide_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
static void words(int64_t* out, int count) {
    for (int i = 0; i < count; ++i) out[i] = word();
}
static void row_words(int32_t* out) {
    for (int i = 0; i < guide::ROW_WORDS; ++i) out[i] = (int32_t)word();
}

static void predict() {
    int64_t M[mos::MODEL_WORDS];
    words(M, mos::MODEL_WORDS);
    const int cx = (int)word(), cy = (int)word();
    int64_t gx = 0, gy = 0, pdx = 0, pdy = 0;
    const bool guides = guide::pair_guides(M);
    if (guides) guide::predict(M, cx, cy, &gx, &gy, &pdx, &pdy);
    printf("%d %lld %lld %lld %lld\n", (int)guides, (long long)gx, (long long)gy, (long long)pdx, (long long)pdy);
}

static void row() {
    const int FH = (int)word(), FW = (int)word(), fill_void = (int)word();
    const int64_t outlier_q20 = word();
    const int has_evidence = (int)word();
    const int64_t sad = word();
    const int penalty = (int)word();
    const int32_t cost = (int32_t)word();
    const int bias = (int)word();
    int64_t M[mos::MODEL_WORDS];
    words(M, mos::MODEL_WORDS);
    const int cx = (int)word(), cy = (int)word();
    int32_t r[guide::ROW_WORDS];
    row_words(r);
    const bool guided = guide::pair_guides(M);
    int64_t gx = 0, gy = 0, pdx = 0, pdy = 0;
    bool avail = false;
    if (guided) {
        guide::predict(M, cx, cy, &gx, &gy, &pdx, &pdy);
        avail = guide::available(pdx, pdy, cx, cy, FH, FW);
    }
    int dx, dy;
    const int cls = guide::classify(r, cx, cy, &dx, &dy);
    const bool outlier = guided && cls == guide::ROW_VECTOR && guide::is_outlier(dx, dy, gx, gy, outlier_q20);
    bool ask;
    int decision = guide::decide(cls, outlier, guided, avail, fill_void, &ask);
    if (has_evidence && ask && !guide::evidence_replaces(guide::guide_cost(sad, penalty, pdx, pdy), cost, bias)) decision = guide::KEEP;
    printf("%d %d %d", decision, cls, (int)outlier);
    for (int i = 0; i < guide::ROW_WORDS; ++i) printf(" %d", (int)guide::out_word(decision, i, r[i], cx, cy, pdx, pdy));
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: guide_host_check COMMANDS.txt\n");
        return 2;
    }
    char cmd[32];
    while (fscanf(in, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "predict")) {
            predict();
        } else if (!strcmp(cmd, "avail")) {
            const int64_t pdx = word(), pdy = word();
            const int cx = (int)word(), cy = (int)word(), FH = (int)word(), FW = (int)word();
            printf("%d\n", (int)guide::available(pdx, pdy, cx, cy, FH, FW));
        } else if (!strcmp(cmd, "class")) {
            int32_t r[guide::ROW_WORDS];
            row_words(r);
            const int cx = (int)word(), cy = (int)word();
            int dx, dy;
            const int cls = guide::classify(r, cx, cy, &dx, &dy);
            printf("%d %d %d\n", cls, dx, dy);
        } else if (!strcmp(cmd, "outlier")) {
            const int dx = (int)word(), dy = (int)word();
            const int64_t gx = word(), gy = word(), oq = word();
            printf("%d\n", (int)guide::is_outlier(dx, dy, gx, gy, oq));
        } else if (!strcmp(cmd, "evidence")) {
            const int64_t sad = word();
            const int penalty = (int)word();
            const int64_t pdx = word(), pdy = word();
            const int32_t cost = (int32_t)word();
            const int bias = (int)word();
            const int64_t cost_g = guide::guide_cost(sad, penalty, pdx, pdy);
            printf("%lld %d\n", (long long)cost_g, (int)guide::evidence_replaces(cost_g, cost, bias));
        } else if (!strcmp(cmd, "row")) {
            row();
        } else {
            fprintf(stderr, "guide_host_check: unknown command %s\n", cmd);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
