// The rules of csrc/relocate_ops.hip on the CPU, serially, through the same relocate_defs.h functions the kernels call.  Built by
// tests/test_relocate_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on the
// command line and prints one line of integers per command:
//   coarse CH CW S, then CH x CW rgba words              -> ch x cw lumas, then ch x cw validity bytes
//   geometry H W CH CW ox oy S state[32]                 -> geom[8] (nt still 0)
//   patch H W CH CW ox oy S state[32], then H x W lumas  -> geom[8], then (status 0 only) tw x th lumas and tw x th validity bytes
//   locate ch cw permille exclude geom[8], then ch x cw cl, ch x cw cv and (a usable geom only) tw x th tl, tw x th tv
//                                                        -> found[16]
//   better sad n u v sad n u v                           -> 0 | 1
//   step H W CH CW ox oy S max_mean ratio found[16] state[32]        -> cand_state[32] cand_pose[16]
//   commit S cand_state[32] cand_pose[16] correct_out[8] state[32] pose[16] found[16]   -> out[8] state[32] pose[16]
#include "relocate_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fs;

static FILE* in;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "relocate_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
static void words(int64_t* out, int count) {
    for (int i = 0; i < count; ++i) out[i] = word();
}
static void print(const int64_t* v, int count, bool first) {
    for (int i = 0; i < count; ++i) printf("%s%lld", first && i == 0 ? "" : " ", (long long)v[i]);
}

static void coarse() {
    const int CH = (int)word(), CW = (int)word(), S = (int)word();
    std::vector<uint32_t> rgba((size_t)CH * CW);  // exactly the canvas: a read outside it is the sanitizer's to find
    for (auto& v : rgba) v = (uint32_t)word();
    const int ch = CH / S, cw = CW / S;
    std::vector<uint8_t> cl((size_t)ch * cw), cv((size_t)ch * cw);
    for (int y = 0; y < ch; ++y)
        for (int x = 0; x < cw; ++x) relo::coarse_cell(rgba.data(), CW, x, y, S, &cl[(size_t)y * cw + x], &cv[(size_t)y * cw + x]);
    for (size_t i = 0; i < cl.size(); ++i) printf("%s%d", i ? " " : "", cl[i]);
    for (size_t i = 0; i < cv.size(); ++i) printf(" %d", cv[i]);
    printf("\n");
}

static void patch(bool cells) {
    const int H = (int)word(), W = (int)word(), CH = (int)word(), CW = (int)word(), ox = (int)word(), oy = (int)word(), S = (int)word();
    int64_t state[mos::STATE_WORDS], geom[relo::GEOM_WORDS];
    words(state, mos::STATE_WORDS);
    std::vector<uint8_t> luma(cells ? (size_t)H * W : 0);
    for (auto& v : luma) v = (uint8_t)word();
    const int status = relo::patch_geometry(state, H, W, CH, CW, ox, oy, S, geom);
    if (!cells || status != relo::PATCH_OK) {
        print(geom, relo::GEOM_WORDS, true);
        printf("\n");
        return;
    }
    const int tw = (int)geom[3], th = (int)geom[4];
    std::vector<int> tl((size_t)tw * th), tv((size_t)tw * th);
    for (int j = 0; j < th; ++j)
        for (int i = 0; i < tw; ++i) {
            uint32_t sum = 0;
            bool all = true;
            for (int p = 0; p < S * S; ++p) {
                int x, y;
                if (!relo::patch_source(state, (geom[1] + i) * S + p % S, (geom[2] + j) * S + p / S, ox, oy, H, W, &x, &y)) {
                    all = false;
                    continue;
                }
                sum += luma[(size_t)y * W + x];
            }
            tl[(size_t)j * tw + i] = all ? (int)relo::cell_mean(sum, S) : 0, tv[(size_t)j * tw + i] = all ? 1 : 0;
            geom[5] += all ? 1 : 0;
        }
    print(geom, relo::GEOM_WORDS, true);
    for (int v : tl) printf(" %d", v);
    for (int v : tv) printf(" %d", v);
    printf("\n");
}

static void locate() {
    const int ch = (int)word(), cw = (int)word(), permille = (int)word(), exclude = (int)word();
    int64_t geom[relo::GEOM_WORDS], found[relo::FOUND_WORDS];
    words(geom, relo::GEOM_WORDS);
    std::vector<uint8_t> cl((size_t)ch * cw), cv((size_t)ch * cw);
    for (auto& v : cl) v = (uint8_t)word();
    for (auto& v : cv) v = (uint8_t)word();
    if (!relo::geom_ok(geom, ch, cw)) {
        relo::write_found(found, relo::FOUND_BAD_GEOM, relo::no_score(), relo::no_score(), 0, 0, 0);
        print(found, relo::FOUND_WORDS, true);
        printf("\n");
        return;
    }
    const int tw = (int)geom[3], th = (int)geom[4];
    std::vector<uint8_t> tl((size_t)tw * th), tv((size_t)tw * th);
    for (auto& v : tl) v = (uint8_t)word();
    for (auto& v : tv) v = (uint8_t)word();
    std::vector<relo::Score> scores;
    for (int av = 0; av + th <= ch; ++av)
        for (int au = 0; au + tw <= cw; ++au) {
            relo::Score s{0, 0, au - geom[1], av - geom[2]};
            relo::score_placement(cl.data(), cv.data(), cw, tl.data(), tv.data(), tw, th, au, av, &s.sad, &s.n);
            scores.push_back(s);
        }
    relo::Score best = relo::no_score(), second = relo::no_score();
    int64_t count = 0;
    for (const auto& s : scores)
        if (relo::eligible(s.n, geom[5], permille)) {
            count += 1;
            if (relo::better(s, best)) best = s;
        }
    if (best.n != 0)
        for (const auto& s : scores)
            if (relo::eligible(s.n, geom[5], permille) && relo::outside(s, best, exclude) && relo::better(s, second)) second = s;
    relo::write_found(found, best.n != 0 ? relo::FOUND : relo::FOUND_NONE, best, second, (int64_t)scores.size(), count, geom[5]);
    print(found, relo::FOUND_WORDS, true);
    printf("\n");
}

static void step() {
    const int H = (int)word(), W = (int)word(), CH = (int)word(), CW = (int)word(), ox = (int)word(), oy = (int)word(), S = (int)word();
    const int max_mean = (int)word(), ratio = (int)word();
    int64_t found[relo::FOUND_WORDS], state[mos::STATE_WORDS], cs[mos::STATE_WORDS], cp[mos::POSE_WORDS];
    words(found, relo::FOUND_WORDS);
    words(state, mos::STATE_WORDS);
    relo::relocate_step(found, state, cs, cp, max_mean, ratio, H, W, CH, CW, ox, oy, S);
    print(cs, mos::STATE_WORDS, true);
    print(cp, mos::POSE_WORDS, false);
    printf("\n");
}

static void commit() {
    const int S = (int)word();
    int64_t cs[mos::STATE_WORDS], cp[mos::POSE_WORDS], co[refn::OUT_WORDS], state[mos::STATE_WORDS], pose[mos::POSE_WORDS], found[relo::FOUND_WORDS], out[relo::OUT_WORDS];
    words(cs, mos::STATE_WORDS);
    words(cp, mos::POSE_WORDS);
    words(co, refn::OUT_WORDS);
    words(state, mos::STATE_WORDS);
    words(pose, mos::POSE_WORDS);
    words(found, relo::FOUND_WORDS);
    relo::commit_step(cs, cp, co, state, pose, found, S, out);
    print(out, relo::OUT_WORDS, true);
    print(state, mos::STATE_WORDS, false);
    print(pose, mos::POSE_WORDS, false);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: relocate_host_check COMMANDS\n");
        return 2;
    }
    char op[16];
    while (fscanf(in, "%15s", op) == 1) {
        if (!strcmp(op, "coarse")) {
            coarse();
        } else if (!strcmp(op, "geometry")) {
            patch(false);
        } else if (!strcmp(op, "patch")) {
            patch(true);
        } else if (!strcmp(op, "locate")) {
            locate();
        } else if (!strcmp(op, "better")) {
            int64_t v[8];
            words(v, 8);
            printf("%d\n", relo::better(relo::Score{v[0], v[1], v[2], v[3]}, relo::Score{v[4], v[5], v[6], v[7]}) ? 1 : 0);
        } else if (!strcmp(op, "step")) {
            step();
        } else if (!strcmp(op, "commit")) {
            commit();
        } else {
            fprintf(stderr, "relocate_host_check: unknown command %s\n", op);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
