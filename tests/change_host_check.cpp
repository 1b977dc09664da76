// The rules of csrc/change_ops.hip on the CPU, serially, through the same change_defs.h (and merge_defs.h) functions the kernels call.
// Built by tests/test_change_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads commands from the file named on
// the command line and prints one line of integers per command.  Canvases, planes and staged windows are exactly as large as they say:
// a read outside one is the sanitizer's to find.
//   change K CHa CWa oxa oya CHb CWb oxb oyb min_votes min_conf r watch_set link[16], then votes_a, votes_b
//                                                              -> counts[8], transitions[2 K K], change, cls_a, cls_b
// The planes are walked tile by tile as the kernels walk them: the classes first (a tile that b_reaches refuses must hold no pixel of
// B: exit 4), then the codes from sets staged for the tile plus its apron, clipped at the canvas edge, ORed along the rows in place and
// then along the columns, with a tally per tile (no cell above the tile's 1024 pixels: exit 5).
#include "change_defs.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fs;

static FILE* in;

static long long word() {
    long long v = 0;
    if (fscanf(in, "%lld", &v) != 1) {
        fprintf(stderr, "change_host_check: a command is short of arguments\n");
        exit(2);
    }
    return v;
}
template <class T>
static void read_plane(std::vector<T>& v) {
    for (auto& x : v) x = (T)word();
}

// one plane's sets for the tile at (X0, Y0): after it, sets[y * PW + x] for x < TILE_W is the OR over the window's row y
static std::vector<uint32_t> row_sets(const std::vector<uint8_t>& plane, int CH, int CW, int X0, int Y0, int r) {
    const int PW = chg::TILE_W + 2 * r, PH = chg::TILE_H + 2 * r;
    std::vector<uint32_t> sets((size_t)PW * PH), span((size_t)chg::TILE_W * PH);
    for (int i = 0; i < PW * PH; ++i) sets[i] = chg::staged_bit(plane.data(), CH, CW, X0 - r + i % PW, Y0 - r + i / PW);
    for (int y = 0; y < PH; ++y)
        for (int x = 0; x < chg::TILE_W; ++x) span[(size_t)y * chg::TILE_W + x] = chg::span_or(&sets[(size_t)y * PW + x], 1, r);
    for (int y = 0; y < PH; ++y)
        for (int x = 0; x < chg::TILE_W; ++x) sets[(size_t)y * PW + x] = span[(size_t)y * chg::TILE_W + x];
    return sets;
}

static void change() {
    const int K = (int)word(), CHa = (int)word(), CWa = (int)word(), oxa = (int)word(), oya = (int)word(), CHb = (int)word(), CWb = (int)word(), oxb = (int)word(),
              oyb = (int)word(), min_votes = (int)word(), min_conf = (int)word(), r = (int)word();
    const uint32_t watch_set = (uint32_t)word();
    int64_t link[mrg::LINK_WORDS], g[6] = {0, 0, 0, 0, 0, 0};
    for (auto& v : link) v = word();
    const size_t pa = (size_t)CHa * CWa, pb = (size_t)CHb * CWb;
    std::vector<uint16_t> va(K * pa), vb(K * pb);
    read_plane(va), read_plane(vb);
    if (K < 1 || K > mos::MAX_CLASSES || !chg::thresholds_ok(min_votes, min_conf, r) || !chg::watch_ok(watch_set, K)) exit(3);
    std::vector<uint8_t> cls_a(pa), cls_b(pa), change(pa);
    std::vector<int64_t> counts(chg::COUNT_WORDS, 0), transitions((size_t)2 * K * K, 0);
    counts[0] = link[12];
    const bool merges = mrg::link_merges(link);
    if (merges) mrg::gather_affine(link, oxb, oyb, g);
    for (int Y0 = 0; Y0 < CHa; Y0 += chg::TILE_H)
        for (int X0 = 0; X0 < CWa; X0 += chg::TILE_W) {
            const int X1 = X0 + chg::TILE_W < CWa ? X0 + chg::TILE_W : CWa, Y1 = Y0 + chg::TILE_H < CHa ? Y0 + chg::TILE_H : CHa;
            const bool reach = merges && mrg::b_reaches(g, X0, Y0, X1, Y1, oxa, oya, CHb, CWb);
            for (int Y = Y0; Y < Y1; ++Y)
                for (int X = X0; X < X1; ++X) {
                    chg::Winner wa = chg::no_votes(), wb = chg::no_votes();
                    int bx = 0, by = 0;
                    const bool has_b = merges && mrg::b_pixel(g, X, Y, oxa, oya, CHb, CWb, &bx, &by);
                    if (has_b && !reach) exit(4);
                    for (int k = 0; k < K; ++k) {
                        chg::take_votes(&wa, k, va[k * pa + (size_t)Y * CWa + X]);
                        if (has_b) chg::take_votes(&wb, k, vb[k * pb + (size_t)by * CWb + bx]);
                    }
                    cls_a[(size_t)Y * CWa + X] = chg::decided_class(wa, min_votes, min_conf);
                    cls_b[(size_t)Y * CWa + X] = has_b ? chg::decided_class(wb, min_votes, min_conf) : chg::NONE;
                }
        }
    for (int Y0 = 0; Y0 < CHa; Y0 += chg::TILE_H)
        for (int X0 = 0; X0 < CWa; X0 += chg::TILE_W) {
            const int X1 = X0 + chg::TILE_W < CWa ? X0 + chg::TILE_W : CWa, Y1 = Y0 + chg::TILE_H < CHa ? Y0 + chg::TILE_H : CHa;
            const int PW = chg::TILE_W + 2 * r;
            const bool reach = merges && mrg::b_reaches(g, X0, Y0, X1, Y1, oxa, oya, CHb, CWb);
            const std::vector<uint32_t> sets_a = row_sets(cls_a, CHa, CWa, X0, Y0, r), sets_b = row_sets(cls_b, CHa, CWa, X0, Y0, r);
            std::vector<uint32_t> tally((size_t)chg::tally_cells(K), 0u);
            for (int Y = Y0; Y < Y1; ++Y)
                for (int X = X0; X < X1; ++X) {
                    const size_t cell = (size_t)Y * CWa + X;
                    const int tx = X - X0, ty = Y - Y0;
                    int bx, by;
                    tally[1] += reach && mrg::b_pixel(g, X, Y, oxa, oya, CHb, CWb, &bx, &by) ? 1u : 0u;
                    const uint32_t win_a = chg::span_or(&sets_a[(size_t)ty * PW + tx], PW, r), win_b = chg::span_or(&sets_b[(size_t)ty * PW + tx], PW, r);
                    const int code = chg::change_code(cls_a[cell], cls_b[cell], win_a, win_b, watch_set);
                    change[cell] = (uint8_t)code;
                    if (code == chg::NOT_COMPARABLE) continue;
                    tally[2] += 1u, tally[2 + code] += 1u;
                    tally[chg::HEAD + chg::transition_cell(0, cls_a[cell], cls_b[cell], K)] += 1u;
                    if (code >= chg::CHANGED_OTHER) tally[chg::HEAD + chg::transition_cell(1, cls_a[cell], cls_b[cell], K)] += 1u;
                }
            for (size_t i = 1; i < tally.size(); ++i) {
                if (tally[i] > (uint32_t)(chg::TILE_W * chg::TILE_H)) exit(5);
                (i < (size_t)chg::HEAD ? counts[i] : transitions[i - chg::HEAD]) += tally[i];
            }
        }
    bool first = true;
    for (auto v : counts) printf("%s%lld", first ? "" : " ", (long long)v), first = false;
    for (auto v : transitions) printf(" %lld", (long long)v);
    for (auto v : change) printf(" %u", v);
    for (auto v : cls_a) printf(" %u", v);
    for (auto v : cls_b) printf(" %u", v);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: change_host_check COMMANDS.txt\n");
        return 2;
    }
    char cmd[32];
    while (fscanf(in, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "change")) change();
        else {
            fprintf(stderr, "change_host_check: unknown command %s\n", cmd);
            return 2;
        }
    }
    fclose(in);
    return 0;
}
