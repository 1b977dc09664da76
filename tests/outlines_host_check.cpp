// Stand-alone host program (tests/test_outlines_cpu.py builds it with -fsanitize=address,undefined): the region outlines through
// csrc/outline_defs.h on the CPU.  For every case of the input file it lists the run starts in slot order (same_bits / start_bits),
// links each to the next one (next_run_start + a bisection of the list), ranks the cycles by the pointer jumping the kernels do
// (pack_rank / join_rank, rank_rounds(max_vertices) rounds with two buffers), cross-checks every contour by walking it crack by crack
// with successor(), and prints the contour table: one line "frame contour region offset vertices cracks area2 anchor" per contour.
//   file: int32 cases; per case int32 (n, H, W, R, connectivity, max_vertices) and the index planes int32 [n][H][W]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "outline_defs.h"

using namespace fs;

static bool read_ints(FILE* fh, int32_t* out, size_t count) { return fread(out, sizeof(int32_t), count, fh) == count; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    int32_t cases = 0;
    if (!read_ints(fh, &cases, 1)) return 2;
    for (int c = 0; c < cases; ++c) {
        int32_t head[6];
        if (!read_ints(fh, head, 6)) return 2;
        const int n = head[0], H = head[1], W = head[2], R = head[3], conn = head[4], V = head[5];
        std::vector<int32_t> planes((size_t)n * H * W);
        if (!read_ints(fh, planes.data(), planes.size())) return 2;
        printf("case %d\n", c);
        for (int f = 0; f < n; ++f) {
            const otl::Plane p = {planes.data() + (size_t)f * H * W, H, W, R};
            std::vector<int> slot;
            for (int i = 0; i < H * W; ++i) {
                const int y = i / W, x = i - y * W, r = p.at(x, y);
                if (r < 0) continue;
                const unsigned starts = otl::start_bits(otl::same_bits(p, x, y, r));
                for (int d = 0; d < 4; ++d)
                    if (starts >> d & 1u) slot.push_back(otl::pack_slot(x, y, d, W));
            }
            const int m = (int)slot.size();
            if (m > V) {
                printf("%d overflow %d\n", f, m);
                continue;
            }
            std::vector<int> next(m), jump(m), jump2(m);
            std::vector<uint64_t> val(m), val2(m);
            for (int i = 0; i < m; ++i) {
                const int target = otl::next_run_start(p, slot[i], conn);
                int lo = 0, hi = m - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (slot[mid] < target) lo = mid + 1;
                    else hi = mid;
                }
                if (slot[lo] != target) {
                    printf("case %d frame %d: the walk from slot %d ends on %d, which is no run start\n", c, f, slot[i], target);
                    return 1;
                }
                next[i] = lo;
                jump[lo] = i;
                val[i] = otl::pack_rank((uint32_t)i, 0u);
            }
            for (int k = 0; k < otl::rank_rounds(V); ++k) {
                for (int i = 0; i < m; ++i) {
                    val2[i] = otl::join_rank(val[i], val[jump[i]], 1u << k);
                    jump2[i] = jump[jump[i]];
                }
                val.swap(val2);
                jump.swap(jump2);
            }
            int contour = 0, offset = 0;
            for (int a = 0; a < m; ++a) {
                if ((int)otl::rank_node(val[a]) != a) continue;
                // the contour of anchor a, node by node: every node names a, and its steps count up from 0
                int count = 0;
                long long area2 = 0, cracks = 0;
                int i = a;
                do {
                    if ((int)otl::rank_node(val[i]) != a || (int)otl::rank_steps(val[i]) != count) {
                        printf("case %d frame %d: node %d ranks (%u, %u), expected (%d, %d)\n", c, f, i, otl::rank_node(val[i]), otl::rank_steps(val[i]), a, count);
                        return 1;
                    }
                    int x, y, d, x0, y0, x1, y1;
                    otl::unpack_slot(slot[i], W, &x, &y, &d);
                    otl::start_corner(x, y, d, &x0, &y0);
                    otl::unpack_slot(slot[next[i]], W, &x, &y, &d);
                    otl::start_corner(x, y, d, &x1, &y1);
                    area2 += (long long)x0 * y1 - (long long)x1 * y0;
                    cracks += abs(x1 - x0) + abs(y1 - y0);
                    ++count;
                    i = next[i];
                } while (i != a && count <= m);
                // the same contour crack by crack
                long long walked = 0;
                int x, y, d, cur = slot[a];
                otl::unpack_slot(cur, W, &x, &y, &d);
                const int r = p.at(x, y);
                do {
                    otl::unpack_slot(cur, W, &x, &y, &d);
                    cur = otl::successor(p, r, x, y, d, conn);
                    ++walked;
                } while (cur != slot[a] && walked <= 4ll * H * W);
                if (walked != cracks) {
                    printf("case %d frame %d: contour of slot %d has %lld cracks by runs, %lld by the walk\n", c, f, slot[a], cracks, walked);
                    return 1;
                }
                printf("%d %d %d %d %d %lld %lld %d\n", f, contour, r, offset, count, cracks, area2, slot[a]);
                ++contour;
                offset += count;
            }
        }
    }
    fclose(fh);
    return 0;
}
