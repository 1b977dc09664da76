// The rules of csrc/merge_ops.hip on the CPU, serially, through the same merge_defs.h functions the kernels call.  Built by
// tests/test_merge_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on the command
// line and prints one line of integers per command.  Canvases are exactly as large as they say: a read outside one is the sanitizer's
// to find.  Rank words travel as two 32-bit halves (high, low).
//   view CHa CWa oxa oya CHb CWb oxb oyb Y0 X0 WH WW link[16], then rgba_a, rgba_b            -> cur, view, valid_a, valid_b
//   gate H W, then (H/16)(W/16) rows of 7, valid_a, valid_b                                 -> the gated table
//   correct Y0 X0 oxa oya model[16] link[16]                                                -> link[16] out[8]
//   merge K CHa CWa oxa oya CHb CWb oxb oyb offset mode ortho link[16], then votes_a, votes_b and (ortho) rank_a, rgba_a, rank_b, rgba_b
//                                                                                           -> counts[8], votes_a and (ortho) rank_a, rgba_a
//   geometry y0 x0 y1 x1 oxb oyb CHa CWa oxa oya S link[16]                                 -> geom[8] (nt still 0)
//   patch CHb CWb y0 x0 y1 x1 oxb oyb CHa CWa oxa oya S link[16], then rgba_b               -> geom[8], then (status 0 only) tl, tv
//   place S max_mean ratio found[16] link[16]                                               -> cand[16] out[8]
#include "merge_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fs;

static FILE* in;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "merge_host_check: a command is short of arguments\n");
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
template <class T>
static void read_plane(std::vector<T>& v) {
    for (auto& x : v) x = (T)word();
}
static void read_ranks(std::vector<uint64_t>& v) {
    for (auto& x : v) {
        const uint64_t hi = (uint64_t)word(), lo = (uint64_t)word();
        x = (hi << 32) | lo;
    }
}

static void view() {
    const int CHa = (int)word(), CWa = (int)word(), oxa = (int)word(), oya = (int)word(), CHb = (int)word(), CWb = (int)word(), oxb = (int)word(), oyb = (int)word();
    const int Y0 = (int)word(), X0 = (int)word(), WH = (int)word(), WW = (int)word();
    int64_t link[mrg::LINK_WORDS], g[6] = {0, 0, 0, 0, 0, 0};
    words(link, mrg::LINK_WORDS);
    std::vector<uint32_t> a((size_t)CHa * CWa), b((size_t)CHb * CWb);
    read_plane(a), read_plane(b);
    if (!mrg::window_ok(Y0, X0, WH, WW, CHa, CWa)) exit(3);
    const bool usable = mrg::link_views(link);
    if (usable) mrg::gather_affine(link, oxb, oyb, g);
    std::vector<uint32_t> out[4];
    for (auto& p : out) p.resize((size_t)WH * WW);
    for (int j = 0; j < WH; ++j)
        for (int i = 0; i < WW; ++i) {
            int bx = 0, by = 0;
            const bool has_b = usable && mrg::b_pixel(g, X0 + i, Y0 + j, oxa, oya, CHb, CWb, &bx, &by);
            const size_t at = (size_t)j * WW + i;
            mrg::view_pixel(a[(size_t)(Y0 + j) * CWa + X0 + i], has_b, has_b ? b[(size_t)by * CWb + bx] : 0u, &out[0][at], &out[2][at], &out[1][at], &out[3][at]);
        }
    bool first = true;
    for (auto& p : out)
        for (auto v : p) printf("%s%u", first ? "" : " ", v), first = false;
    printf("\n");
}

static void gate() {
    const int H = (int)word(), W = (int)word(), blocks = (H / 16) * (W / 16);
    std::vector<int32_t> table((size_t)blocks * refn::ROW_WORDS);
    read_plane(table);
    std::vector<uint8_t> va((size_t)H * W), vb((size_t)H * W);
    read_plane(va), read_plane(vb);
    for (int r = 0; r < blocks; ++r)
        if (!mrg::merge_gate_keeps(&table[(size_t)r * refn::ROW_WORDS], r, va.data(), vb.data(), H, W)) refn::void_row(&table[(size_t)r * refn::ROW_WORDS]);
    for (size_t i = 0; i < table.size(); ++i) printf("%s%d", i ? " " : "", table[i]);
    printf("\n");
}

static void correct() {
    const int Y0 = (int)word(), X0 = (int)word(), oxa = (int)word(), oya = (int)word();
    int64_t model[mos::MODEL_WORDS], link[mrg::LINK_WORDS], out[mrg::OUT_WORDS];
    words(model, mos::MODEL_WORDS), words(link, mrg::LINK_WORDS);
    mrg::correct_step(model, link, X0, Y0, oxa, oya, out);
    print(link, mrg::LINK_WORDS, true), print(out, mrg::OUT_WORDS, false);
    printf("\n");
}

static void merge() {
    const int K = (int)word(), CHa = (int)word(), CWa = (int)word(), oxa = (int)word(), oya = (int)word(), CHb = (int)word(), CWb = (int)word(), oxb = (int)word(),
              oyb = (int)word();
    const uint32_t offset = (uint32_t)word();
    const int mode = (int)word(), ortho = (int)word();
    int64_t link[mrg::LINK_WORDS], g[6], counts[mrg::COUNT_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    words(link, mrg::LINK_WORDS);
    const size_t pa = (size_t)CHa * CWa, pb = (size_t)CHb * CWb;
    std::vector<uint16_t> va(K * pa), vb(K * pb);
    read_plane(va), read_plane(vb);
    std::vector<uint64_t> ra(ortho ? pa : 0), rb(ortho ? pb : 0);
    std::vector<uint32_t> ca(ortho ? pa : 0), cb(ortho ? pb : 0);
    read_ranks(ra), read_plane(ca), read_ranks(rb), read_plane(cb);
    counts[0] = link[12];
    if (mrg::link_merges(link)) {
        mrg::gather_affine(link, oxb, oyb, g);
        for (int Y0 = 0; Y0 < CHa; Y0 += 16)          // tile by tile as the kernel walks: a tile b_reaches refuses must hold no pixel of B
            for (int X0 = 0; X0 < CWa; X0 += 64) {
                const int X1 = X0 + 64 < CWa ? X0 + 64 : CWa, Y1 = Y0 + 16 < CHa ? Y0 + 16 : CHa;
                const bool reach = mrg::b_reaches(g, X0, Y0, X1, Y1, oxa, oya, CHb, CWb);
                for (int Y = Y0; Y < Y1; ++Y)
                    for (int X = X0; X < X1; ++X) {
                        int bx, by;
                        if (!mrg::b_pixel(g, X, Y, oxa, oya, CHb, CWb, &bx, &by)) continue;
                        if (!reach) exit(4);
                        const size_t cell_a = (size_t)Y * CWa + X, cell_b = (size_t)by * CWb + bx;
                        counts[1] += 1;
                        bool any = false;
                        for (int k = 0; k < K; ++k) {
                            const uint32_t more = vb[k * pb + cell_b];
                            if (!more) continue;
                            va[k * pa + cell_a] = mos::vote_add(va[k * pa + cell_a], more);
                            any = true, counts[3] += more;
                        }
                        counts[2] += any ? 1 : 0;
                        uint64_t mine;
                        if (ortho && mrg::shifted_rank(rb[cell_b], offset, mode, &mine) && orth::replaces(mine, ra[cell_a]))
                            ra[cell_a] = mine, ca[cell_a] = cb[cell_b], counts[4] += 1;
                    }
            }
    }
    print(counts, mrg::COUNT_WORDS, true);
    for (auto v : va) printf(" %u", v);
    for (auto v : ra) printf(" %llu %llu", (unsigned long long)(v >> 32), (unsigned long long)(v & 0xFFFFFFFFull));
    for (auto v : ca) printf(" %u", v);
    printf("\n");
}

static void patch(bool cells) {
    const int CHb = cells ? (int)word() : 0, CWb = cells ? (int)word() : 0;
    const int y0 = (int)word(), x0 = (int)word(), y1 = (int)word(), x1 = (int)word(), oxb = (int)word(), oyb = (int)word(), CHa = (int)word(), CWa = (int)word(),
              oxa = (int)word(), oya = (int)word(), S = (int)word();
    int64_t link[mrg::LINK_WORDS], geom[relo::GEOM_WORDS], g[6];
    words(link, mrg::LINK_WORDS);
    std::vector<uint32_t> b((size_t)CHb * CWb);
    read_plane(b);
    const int status = mrg::box_geometry(link, y0, x0, y1, x1, oxb, oyb, CHa, CWa, oxa, oya, S, geom);
    if (!cells || status != relo::PATCH_OK) {
        print(geom, relo::GEOM_WORDS, true);
        printf("\n");
        return;
    }
    if (!mrg::box_ok(y0, x0, y1, x1, CHb, CWb)) exit(3);
    mrg::gather_affine(link, oxb, oyb, g);
    const int tw = (int)geom[3], th = (int)geom[4];
    std::vector<int> tl((size_t)tw * th), tv((size_t)tw * th);
    for (int j = 0; j < th; ++j)
        for (int i = 0; i < tw; ++i) {
            uint32_t sum = 0;
            bool all = true;
            for (int p = 0; p < S * S; ++p) {
                uint32_t luma;
                if (!mrg::patch_pixel(g, (geom[1] + i) * S + p % S, (geom[2] + j) * S + p / S, oxa, oya, b.data(), CHb, CWb, &luma)) {
                    all = false;
                    continue;
                }
                sum += luma;
            }
            tl[(size_t)j * tw + i] = all ? (int)relo::cell_mean(sum, S) : 0, tv[(size_t)j * tw + i] = all ? 1 : 0;
            geom[5] += all ? 1 : 0;
        }
    print(geom, relo::GEOM_WORDS, true);
    for (auto v : tl) printf(" %d", v);
    for (auto v : tv) printf(" %d", v);
    printf("\n");
}

static void place() {
    const int S = (int)word(), max_mean = (int)word(), ratio = (int)word();
    int64_t found[relo::FOUND_WORDS], link[mrg::LINK_WORDS], cand[mrg::LINK_WORDS], out[mrg::OUT_WORDS];
    words(found, relo::FOUND_WORDS), words(link, mrg::LINK_WORDS);
    mrg::place_step(found, link, max_mean, ratio, S, cand, out);
    print(cand, mrg::LINK_WORDS, true), print(out, mrg::OUT_WORDS, false);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: merge_host_check COMMANDS.txt\n");
        return 2;
    }
    char cmd[32];
    while (fscanf(in, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "view")) view();
        else if (!strcmp(cmd, "gate")) gate();
        else if (!strcmp(cmd, "correct")) correct();
        else if (!strcmp(cmd, "merge")) merge();
        else if (!strcmp(cmd, "geometry")) patch(false);
        else if (!strcmp(cmd, "patch")) patch(true);
        else if (!strcmp(cmd, "place")) place();
        else {
            fprintf(stderr, "merge_host_check: unknown command %s\n", cmd);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
