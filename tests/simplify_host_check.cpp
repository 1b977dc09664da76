// Stand-alone host program (tests/test_simplify_cpu.py builds it with -fsanitize=address,undefined): the outline simplification through
// csrc/simplify_defs.h on the CPU, in ROUND form as the kernels run it.  Every vertex holds a cell (split_seg / pack_seg); per round
// every open vertex takes the split the round before decided (splits), measures its key (seg_key) into its segment's slot -- the
// segment's left vertex, two buffers by the round's parity -- and the smallest index among the largest keys is picked; what is open
// after the last round is kept.  Prints per frame "frame F rows kept rounds flags" and per row "F row first kept area2 flags".
//   file: int32 cases; per case int32 (n, C, V, tol_q, max_rounds), contours int64 [n][C][6], vertices int32 [n][V][2], counts int64 [n][4]
//   Only frames that region_outlines made are given: the rows are consistent (the validity rules are the numpy definition's to test).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "simplify_defs.h"

using namespace fs;

template <typename T>
static bool read_all(FILE* fh, T* out, size_t count) { return fread(out, sizeof(T), count, fh) == count; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int32_t cases = 0;
    if (!read_all(fh, &cases, 1)) return 2;
    for (int c = 0; c < cases; ++c) {
        int32_t head[5];
        if (!read_all(fh, head, 5)) return 2;
        const int n = head[0], C = head[1], V = head[2], tol_q = head[3], K = head[4];
        std::vector<int64_t> contours((size_t)n * C * 6), counts((size_t)n * 4);
        std::vector<int32_t> vertices((size_t)n * V * 2);
        if (!read_all(fh, contours.data(), contours.size()) || !read_all(fh, vertices.data(), vertices.size()) || !read_all(fh, counts.data(), counts.size()))
            return 2;
        if (smp::frame_words(C, V) * 8 * (size_t)n == 0) return 2;
        printf("case %d\n", c);
        for (int f = 0; f < n; ++f) {
            const int rows = (int)counts[4 * f + 1];
            if (counts[4 * f + 3] & 1) {
                printf("frame %d 0 0 0 %d\n", f, smp::FLAG_INPUT_OVERFLOW);
                continue;
            }
            const int64_t* table = contours.data() + (size_t)f * C * 6;
            const int32_t* vert = vertices.data() + (size_t)f * V * 2;
            const int end = rows ? (int)(table[(rows - 1) * 6 + 1] + table[(rows - 1) * 6 + 2]) : 0;
            std::vector<int> row(end), off(end), len(end);
            for (int r = 0; r < rows; ++r)
                for (int j = 0; j < (int)table[r * 6 + 2]; ++j) {
                    const int i = (int)table[r * 6 + 1] + j;
                    row[i] = r;
                    off[i] = (int)table[r * 6 + 1];
                    len[i] = (int)table[r * 6 + 2];
                }
            auto X = [&](int i, int j) { return smp::clamp_coord(vert[2 * (off[i] + (j >= len[i] ? 0 : j))]); };
            auto Y = [&](int i, int j) { return smp::clamp_coord(vert[2 * (off[i] + (j >= len[i] ? 0 : j)) + 1]); };
            std::vector<uint64_t> seg(end), key(end), qmax[2] = {std::vector<uint64_t>(end, 0), std::vector<uint64_t>(end, 0)};
            std::vector<int> imin[2] = {std::vector<int>(end, INT_MAX), std::vector<int>(end, INT_MAX)};
            for (int i = 0; i < end; ++i) seg[i] = i == off[i] ? smp::pack_seg(smp::KEPT, 0) : smp::pack_seg(0, len[i]);
            int deepest = 0;
            // the cell of open vertex i after the split of `round`
            auto apply = [&](int i, int round) {
                const int l = smp::seg_l(seg[i]), r = smp::seg_r(seg[i]), j = i - off[i], par = round & 1;
                const int64_t ux = X(i, r) - X(i, l), uy = Y(i, r) - Y(i, l);
                const int s = imin[par][off[i] + l];
                const bool split = smp::splits(round, (int64_t)qmax[par][off[i] + l], ux * ux + uy * uy, tol_q);
                if (split && (s <= l || s >= r)) {
                    printf("case %d frame %d: vertex %d of (%d, %d) is told to split at %d\n", c, f, j, l, r, s);
                    exit(1);
                }
                if (split && j == s && round > deepest) deepest = round;
                return smp::split_seg(l, r, j, split, s);
            };
            for (int k = 0; k <= K; ++k) {
                const int par = k & 1;
                for (int i = 0; i < end; ++i) {  // launch A
                    if (smp::seg_l(seg[i]) < 0) continue;
                    if (k > 0) seg[i] = apply(i, k - 1);
                    if (smp::seg_l(seg[i]) < 0) continue;
                    const int l = smp::seg_l(seg[i]), r = smp::seg_r(seg[i]), j = i - off[i];
                    if (!(0 <= l && l < j && j < r && r <= len[i])) {
                        printf("case %d frame %d: vertex %d is not inside its segment (%d, %d)\n", c, f, j, l, r);
                        return 1;
                    }
                    int64_t L;
                    key[i] = (uint64_t)smp::seg_key(X(i, l), Y(i, l), X(i, r), Y(i, r), X(i, j), Y(i, j), &L);
                    if (key[i] > qmax[par][off[i] + l]) qmax[par][off[i] + l] = key[i];
                }
                for (int i = 0; i < end; ++i) {  // launch B
                    if (smp::seg_l(seg[i]) >= 0) {
                        const int slot = off[i] + smp::seg_l(seg[i]);
                        if (key[i] == qmax[par][slot] && i - off[i] < imin[par][slot]) imin[par][slot] = i - off[i];
                    }
                    qmax[par ^ 1][i] = 0;
                    imin[par ^ 1][i] = INT_MAX;
                }
            }
            std::vector<int> unconverged(rows, 0);
            int any = 0;
            for (int i = 0; i < end; ++i) {  // the closing pass
                if (smp::seg_l(seg[i]) < 0) continue;
                seg[i] = apply(i, K);
                if (smp::seg_l(seg[i]) >= 0) {
                    seg[i] = smp::pack_seg(smp::KEPT, 0);
                    unconverged[row[i]] = any = 1;
                }
            }
            int kept = 0;
            for (int i = 0; i < end; ++i) kept += smp::seg_l(seg[i]) == smp::KEPT;
            printf("frame %d %d %d %d %d\n", f, rows, kept, deepest, any | (counts[4 * f] > rows ? smp::FLAG_INPUT_TRUNCATED : 0));
            int at = 0;
            for (int r = 0; r < rows; ++r) {
                const int o = (int)table[r * 6 + 1], m = (int)table[r * 6 + 2];
                std::vector<int> ring;
                for (int j = 0; j < m; ++j)
                    if (smp::seg_l(seg[o + j]) == smp::KEPT) ring.push_back(j);
                long long area2 = 0;
                for (size_t k = 0; k < ring.size(); ++k) {
                    const int a = ring[k], b = ring[(k + 1) % ring.size()];
                    area2 += (long long)X(o, a) * Y(o, b) - (long long)X(o, b) * Y(o, a);
                }
                printf("%d %d %d %d %lld %d\n", f, r, at, (int)ring.size(), area2, unconverged[r]);
                at += (int)ring.size();
            }
        }
    }
    fclose(fh);
    return 0;
}
