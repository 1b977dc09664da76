// The compensated overlap pass of csrc/track_ops.hip (region_links_mc) on the CPU, serially, through the same track_defs.h functions the
// kernels call: pass 0 packs one shift per block, pass 1 gathers the previous plane at every pixel's source and counts the pairs (one
// insertion per pixel here, in raster order and once more in reverse), passes 2 and 3 pick and unpack.  Built by
// tests/test_tracks_mc_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads the cases and what it has to reproduce
// from the file named on the command line:
//   int32 entries;  per entry: int32 n, H, W, R, max_pairs, min_overlap, FH, FW, has_stats;  int32 index [n][H][W];
//   int64 table [n][R][10];  int64 counts [n][2];  int32 mv [n][FH/16 * FW/16][7];  has_stats: int32 stats [n][4];
//   int32 back [n][R][2];  int32 fwd [n][R][2];  int64 link_counts [n][2]
// Frame 0 has no frame before it.  Before the cases, the arithmetic at the limits the launcher admits (the sanitizer watches it).
#include "track_defs.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fs;

template <class T>
static bool read_all(FILE* fh, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), fh) == v.size(); }

static int rows_of(const int64_t* counts, int R) { return (int)(counts[1] < 0 ? 0 : (counts[1] > R ? R : counts[1])); }

static int limits() {
    int bad = 0;
    const int big = 2147483646, top = (1 << 27) - 1;  // the tallest mask (one column), the tallest frame (16 columns)
    bad += trk::mc_block(big - 1, big, top) != (int)(((2 * (__int128)(big - 1) + 1) * top) / (2 * (__int128)big) / 16);
    bad += trk::mc_block(big - 1, big, 16) != 0 || trk::mc_block(0, 1, 16) != 0 || trk::mc_block(0, 1, top) != top / 2 / 16;
    bad += trk::mc_block(495, 496, 16) != 0 || trk::mc_block(49, 50, 50) != 3 || trk::mc_block(47, 50, 50) != 2;
    for (int v : {-1024, -1, 0, 1, 1024}) {
        const int s = trk::mc_scale(v, 31 * 16, 16);  // the largest admitted scale: |shift| <= 31744
        bad += s != 31 * v || trk::mc_shift_x(trk::mc_pack_shift(-s, s)) != s || trk::mc_shift_y(trk::mc_pack_shift(-s, s)) != -s;
    }
    bad += trk::mc_scale(1, 1, 2) != 1 || trk::mc_scale(-1, 1, 2) != -1 || trk::mc_scale(1, 1, 3) != 0 || trk::mc_scale(3, 37, 48) != 2;
    int ys, xs;
    bad += trk::mc_source(big - 1, 0, trk::mc_pack_shift(31744, 0), big, 1, &ys, &xs) || !trk::mc_source(5, 5, trk::mc_pack_shift(-5, -5), 6, 6, &ys, &xs) ||
           ys != 0 || xs != 0 || trk::mc_source(5, 5, trk::mc_pack_shift(-6, 0), 6, 6, &ys, &xs) || trk::mc_source(5, 5, trk::mc_pack_shift(0, 1), 6, 6, &ys, &xs);
    const int32_t lo = INT32_MIN, hi = INT32_MAX;
    const int32_t rows[6][7] = {{0, 0, 0, hi, hi, 0, 0}, {0, 0, 0, lo, 5, hi, 5}, {0, 0, 0, 5, 5, -1, 5}, {0, 0, 0, 1033, 9, 9, 9}, {0, 0, 0, 1034, 9, 9, 9},
                                {-1, 16, 16, -16, -16, -16, -16}};
    const uint32_t want[6] = {0u, 0u, 0u, trk::mc_pack_shift(0, 1024), 0u, 0u};
    for (int j = 0; j < 6; ++j) bad += trk::mc_row_shift(rows[j], 64, 64, 64, 64) != want[j];
    const int32_t cut[4] = {9, 9, 1, 0}, plain[4] = {9, 9, 0, 0};
    bad += trk::cut_flag(cut) != 2u || trk::cut_flag(plain) != 0u || trk::link_flags(1u) != 1 || trk::link_flags(2u) != 2 || trk::link_flags(0u) != 0;
    return bad;
}

// passes 0 to 3 for the frame pair (f - 1, f)
static void links(const int* ia, const int64_t* ta, int rows_a, const int* ib, const int64_t* tb, int rows_b, const int32_t* mv, const int32_t* stats, int H,
                  int W, int FH, int FW, int R, uint32_t max_pairs, int min_overlap, bool reverse, int* back, int* fwd, int64_t* link_counts) {
    const int hb = FH / trk::MC_BLOCK, wb = FW / trk::MC_BLOCK;
    const size_t HW = (size_t)H * W;
    std::vector<uint64_t> keys(max_pairs, 0), best_back(R, 0), best_fwd(R, 0);
    std::vector<uint32_t> count(max_pairs, 0), shifts((size_t)hb * wb);
    unsigned word = 0;
    for (int k = 0; k < hb * wb; ++k) shifts[k] = trk::mc_row_shift(mv + (size_t)k * trk::MC_VECTOR_INTS, H, W, FH, FW);  // pass 0
    if (stats) word = trk::cut_flag(stats);
    for (size_t j = 0; j < HW && !word; ++j) {  // pass 1; a cut pair skips it
        const size_t i = reverse ? HW - 1 - j : j;
        const int y = (int)(i / W), x = (int)(i % W);
        const int by = trk::mc_block(y, H, FH), bx = trk::mc_block(x, W, FW);
        const uint32_t shift = by < hb && bx < wb ? shifts[(size_t)by * wb + bx] : 0u;
        int ys, xs;
        const int a = trk::mc_source(y, x, shift, H, W, &ys, &xs) ? ia[(size_t)ys * W + xs] : -1, b = ib[i];
        if (!(a >= 0 && a < rows_a && b >= 0 && b < rows_b) || ta[(size_t)a * 10] != tb[(size_t)b * 10]) continue;
        const uint64_t key = trk::pack_key(a, b);
        bool stored = false;
        for (uint32_t p = 0; p < max_pairs && !stored; ++p) {
            const uint32_t slot = trk::probe_slot(key, p, max_pairs);
            if (keys[slot] == 0) keys[slot] = key;
            if (keys[slot] == key) {
                ++count[slot];
                stored = true;
            }
        }
        if (!stored) word |= trk::FLAG_OVERFLOW;
    }
    int64_t pairs = 0;
    for (uint32_t s = 0; s < max_pairs; ++s) {  // pass 2
        if (!keys[s]) continue;
        ++pairs;
        const int a = trk::key_a(keys[s]), b = trk::key_b(keys[s]);
        const uint64_t vb = trk::pack_best(count[s], a), vf = trk::pack_best(count[s], b);
        if (vb > best_back[b]) best_back[b] = vb;
        if (vf > best_fwd[a]) best_fwd[a] = vf;
    }
    for (int r = 0; r < R; ++r) {  // pass 3
        trk::unpack_link(best_back[r], min_overlap, word != 0, &back[2 * r], &back[2 * r + 1]);
        trk::unpack_link(best_fwd[r], min_overlap, word != 0, &fwd[2 * r], &fwd[2 * r + 1]);
    }
    link_counts[0] = pairs;
    link_counts[1] = trk::link_flags(word);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (int wrong = limits()) {
        std::printf("%d checks at the limits fail\n", wrong);
        return 1;
    }
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    int entries = 0, bad = 0;
    if (std::fread(&entries, 4, 1, fh) != 1) return 2;
    for (int e = 0; e < entries; ++e) {
        int head[9];
        if (std::fread(head, 4, 9, fh) != 9) return 2;
        const int n = head[0], H = head[1], W = head[2], R = head[3], min_overlap = head[5], FH = head[6], FW = head[7];
        const uint32_t max_pairs = (uint32_t)head[4];
        const size_t HW = (size_t)H * W, nR = (size_t)n * R, blocks = (size_t)(FH / 16) * (FW / 16);
        std::vector<int> index(n * HW), mv(n * blocks * 7), stats(head[8] ? n * 4 : 0), want_back(nR * 2), want_fwd(nR * 2), back(nR * 2), fwd(nR * 2);
        std::vector<int64_t> table(nR * 10), counts(n * 2), want_lc(n * 2), lc(n * 2);
        if (!read_all(fh, index) || !read_all(fh, table) || !read_all(fh, counts) || !read_all(fh, mv) || !read_all(fh, stats) || !read_all(fh, want_back) ||
            !read_all(fh, want_fwd) || !read_all(fh, want_lc))
            return 2;
        for (int reverse = 0; reverse < 2; ++reverse) {
            for (int f = 0; f < n; ++f) {
                int *bk = &back[(size_t)f * R * 2], *fw = &fwd[(size_t)f * R * 2];
                if (f == 0) {  // nothing before it: an empty table gives (-1, 0) throughout
                    for (int r = 0; r < R; ++r) {
                        trk::unpack_link(0, min_overlap, false, &bk[2 * r], &bk[2 * r + 1]);
                        trk::unpack_link(0, min_overlap, false, &fw[2 * r], &fw[2 * r + 1]);
                    }
                    lc[0] = lc[1] = 0;
                    continue;
                }
                links(&index[(f - 1) * HW], &table[(size_t)(f - 1) * R * 10], rows_of(&counts[2 * (f - 1)], R), &index[f * HW], &table[(size_t)f * R * 10],
                      rows_of(&counts[2 * f], R), &mv[f * blocks * 7], head[8] ? &stats[4 * f] : nullptr, H, W, FH, FW, R, max_pairs, min_overlap, reverse != 0,
                      bk, fw, &lc[2 * f]);
            }
            if (!(back == want_back && fwd == want_fwd && lc == want_lc)) {
                std::printf("entry %d (%d x %d x %d on %d x %d, R %d, max_pairs %u) reverse %d: differs (back %d fwd %d counts %d)\n", e, n, H, W, FH, FW, R,
                            max_pairs, reverse, back == want_back, fwd == want_fwd, lc == want_lc);
                ++bad;
            }
        }
    }
    std::fclose(fh);
    std::printf("%d entries, %d mismatching runs\n", entries, bad);
    return bad ? 1 : 0;
}
