// csrc/ground_defs.h on the CPU (tests/test_ground_cpu.py builds this with -fsanitize=address,undefined -ffp-contract=off and compares
// every line with tests/ground_ref.py).  It walks the canvas and the raster tile by tile as csrc/ground_ops.hip does: the all-unseen
// test first, then the tile's (TW + 1) x (TH + 1) corners staged once, then the pixels from the staged array; a raster tile whose four
// corners map beyond one side of the canvas box is filled without looking at its pixels.
//   usage: ground_host_check COMMANDS.txt        one command per line, numbers separated by blanks, doubles as C99 hex floats
//     check    CH CW ox oy  m*9                                   -> check_forward's code and the orientation
//     checkinv GH GW gsd e0 ntop  m*9                             -> check_inverse's code
//     area     CH CW ox oy K R  m*9  cls*(CH*CW)  [index*(CH*CW) when R > 0]   -> K class sums, R region sums, 4 counts
//     points   n ox oy  m*9  (x y)*n                              -> (E N)*n
//     rectify  CH CW ox oy GH GW gsd e0 ntop fill rgbfill  m*9  cls*(CH*CW)  rgba*(CH*CW)   -> the plane raster, then the rgb words
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ground_defs.h"

using namespace fs;

namespace {

constexpr int TW = 64, TH = 16;

double number(std::istringstream& in) {
    std::string word;
    in >> word;
    return strtod(word.c_str(), nullptr);
}
long long integer(std::istringstream& in) {
    long long v = 0;
    in >> v;
    return v;
}
void model(std::istringstream& in, double* m) {
    for (int k = 0; k < 9; ++k) m[k] = number(in);
}

void do_area(std::istringstream& in) {
    const int CH = (int)integer(in), CW = (int)integer(in), ox = (int)integer(in), oy = (int)integer(in), K = (int)integer(in), R = (int)integer(in);
    double m[9];
    model(in, m);
    std::vector<uint8_t> cls((size_t)CH * CW);
    for (auto& c : cls) c = (uint8_t)integer(in);
    std::vector<int32_t> index(R > 0 ? (size_t)CH * CW : 0);
    for (auto& i : index) i = (int32_t)integer(in);
    const int orient = gnd::orientation(m);
    std::vector<int64_t> klass(K, 0), region(R, 0);
    int64_t counts[4] = {0, 0, 0, 0};
    for (int Y0 = 0; Y0 < CH; Y0 += TH)
        for (int X0 = 0; X0 < CW; X0 += TW) {
            bool any = false;
            for (int y = Y0; y < Y0 + TH && y < CH; ++y)
                for (int x = X0; x < X0 + TW && x < CW; ++x) any = any || cls[(size_t)y * CW + x] != gnd::UNSEEN;
            if (!any) continue;
            std::vector<int64_t> ce((TW + 1) * (TH + 1)), cn((TW + 1) * (TH + 1));  // exactly the kernel's LDS arrays: a wrong index is the sanitizer's
            for (int cy = 0; cy <= TH; ++cy)
                for (int cx = 0; cx <= TW; ++cx)
                    if (X0 + cx <= CW && Y0 + cy <= CH) gnd::corner(m, X0 + cx - ox, Y0 + cy - oy, &ce[cy * (TW + 1) + cx], &cn[cy * (TW + 1) + cx]);
            for (int ly = 0; ly < TH && Y0 + ly < CH; ++ly)
                for (int lx = 0; lx < TW && X0 + lx < CW; ++lx) {
                    const size_t at = (size_t)(Y0 + ly) * CW + X0 + lx;
                    const int c = cls[at];
                    if (c == (int)gnd::UNSEEN) continue;
                    if (c >= K) {
                        ++counts[2];
                        continue;
                    }
                    const int q = ly * (TW + 1) + lx;
                    const int64_t a =
                        gnd::area2(ce.at(q), cn.at(q), ce.at(q + 1), cn.at(q + 1), ce.at(q + TW + 2), cn.at(q + TW + 2), ce.at(q + TW + 1), cn.at(q + TW + 1)) * orient;
                    if (gnd::folded(a)) {
                        ++counts[1];
                        continue;
                    }
                    ++counts[0];
                    klass[c] += a;
                    if (R > 0 && index[at] >= 0 && index[at] < R) region[index[at]] += a;
                }
        }
    for (int64_t v : klass) printf("%" PRId64 " ", v);
    for (int64_t v : region) printf("%" PRId64 " ", v);
    printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", counts[0], counts[1], counts[2], counts[3]);
}

void do_points(std::istringstream& in) {
    const int n = (int)integer(in), ox = (int)integer(in), oy = (int)integer(in);
    double m[9];
    model(in, m);
    for (int p = 0; p < n; ++p) {
        const long long x = integer(in), y = integer(in);
        int64_t e = gnd::NO_POINT, nn = gnd::NO_POINT;
        if (x >= -(1 << 20) && x <= (1 << 20) && y >= -(1 << 20) && y <= (1 << 20))
            if (!gnd::corner_checked(m, (int)x - ox, (int)y - oy, &e, &nn)) e = nn = gnd::NO_POINT;
        printf("%" PRId64 " %" PRId64 "%s", e, nn, p + 1 < n ? " " : "");
    }
    printf("\n");
}

void do_rectify(std::istringstream& in) {
    const int CH = (int)integer(in), CW = (int)integer(in), ox = (int)integer(in), oy = (int)integer(in), GH = (int)integer(in), GW = (int)integer(in);
    const int gsd = (int)integer(in);
    const int64_t e0 = integer(in), ntop = integer(in);
    const int fill = (int)integer(in);
    const uint32_t rgb_fill = (uint32_t)integer(in);
    double inv[9];
    model(in, inv);
    std::vector<uint8_t> cls((size_t)CH * CW);
    for (auto& c : cls) c = (uint8_t)integer(in);
    std::vector<uint32_t> rgba((size_t)CH * CW);
    for (auto& w : rgba) w = (uint32_t)integer(in);
    std::vector<uint8_t> plane((size_t)GH * GW);
    std::vector<uint32_t> rgb((size_t)GH * GW);
    const auto tap = [&](int tx, int ty) -> uint32_t { return tx >= 0 && tx < CW && ty >= 0 && ty < CH ? rgba.at((size_t)ty * CW + tx) : 0u; };
    int skipped = 0;
    for (int V0 = 0; V0 < GH; V0 += TH)
        for (int U0 = 0; U0 < GW; U0 += TW) {
            double cx[4], cy[4];
            for (int k = 0; k < 4; ++k) {
                const int cu = (k == 1 || k == 2) ? (U0 + TW < GW ? U0 + TW : GW) : U0, cv = k >= 2 ? (V0 + TH < GH ? V0 + TH : GH) : V0;
                const double du = (double)cu * (double)gsd, dv = (double)cv * (double)gsd;
                const double eg = (double)e0 + du, ng = (double)ntop - dv;
                gnd::project(inv, eg, ng, &cx[k], &cy[k]);
            }
            const bool empty = gnd::tile_outside(cx, cy, ox, oy, CH, CW);
            skipped += empty;
            for (int v = V0; v < V0 + TH && v < GH; ++v)
                for (int u = U0; u < U0 + TW && u < GW; ++u) {
                    const size_t at = (size_t)v * GW + u;
                    plane[at] = (uint8_t)fill, rgb[at] = rgb_fill & 0xFFFFFFu;
                    if (empty) continue;
                    double eg, ng, x, y;
                    gnd::raster_ground(u, v, gsd, e0, ntop, &eg, &ng);
                    if (!gnd::ground_to_anchor(inv, eg, ng, &x, &y)) continue;
                    int X, Y;
                    if (gnd::nearest_pixel(x, y, ox, oy, CH, CW, &X, &Y)) plane[at] = cls.at((size_t)Y * CW + X);
                    rgb[at] = gnd::rectify_colour(tap, x, y, ox, oy, rgb_fill);
                }
        }
    printf("%d", skipped);
    for (uint8_t v : plane) printf(" %u", (unsigned)v);
    for (uint32_t v : rgb) printf(" %u", (unsigned)v);
    printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: ground_host_check COMMANDS.txt\n");
        return 2;
    }
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "check") {
            const int CH = (int)integer(in), CW = (int)integer(in), ox = (int)integer(in), oy = (int)integer(in);
            double m[9];
            model(in, m);
            printf("%d %d\n", gnd::check_forward(m, CH, CW, ox, oy), gnd::orientation(m));
        } else if (cmd == "checkinv") {
            const int GH = (int)integer(in), GW = (int)integer(in), gsd = (int)integer(in);
            const int64_t e0 = integer(in), ntop = integer(in);
            double m[9];
            model(in, m);
            printf("%d\n", gnd::check_inverse(m, GH, GW, gsd, e0, ntop));
        } else if (cmd == "area") {
            do_area(in);
        } else if (cmd == "points") {
            do_points(in);
        } else if (cmd == "rectify") {
            do_rectify(in);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
