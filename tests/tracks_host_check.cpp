// The four passes of csrc/track_ops.hip on the CPU, serially, through the same track_defs.h functions the kernels call: the pair table
// (one insertion per pixel here, in raster order and once more in reverse: the result must not depend on it), the best pick, the
// unpacking and the track ids.  Built by tests/test_tracks_cpu.py with -fsanitize=address,undefined as a stand-alone program; reads the
// cases and what it has to reproduce from the file named on the command line:
//   int32 entries;  per entry: int32 n, H, W, R, max_pairs, min_overlap;  int32 index [n][H][W];  int64 table [n][R][10];
//   int64 counts [n][2];  int32 back [n][R][2];  int32 fwd [n][R][2];  int64 link_counts [n][2];  int64 tracks [n][R][4];  int64 state [2]
// Frame 0 has no frame before it and the ids start at 0.
#include "track_defs.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fs;

template <class T>
static bool read_all(FILE* fh, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), fh) == v.size(); }

static int rows_of(const int64_t* counts, int R) { return (int)(counts[1] < 0 ? 0 : (counts[1] > R ? R : counts[1])); }

// passes 1 to 3 for the frame pair (f - 1, f)
static void links(const int* ia, const int64_t* ta, int rows_a, const int* ib, const int64_t* tb, int rows_b, size_t HW, int R, uint32_t max_pairs,
                  int min_overlap, bool reverse, int* back, int* fwd, int64_t* link_counts) {
    std::vector<uint64_t> keys(max_pairs, 0), best_back(R, 0), best_fwd(R, 0);
    std::vector<uint32_t> count(max_pairs, 0);
    bool overflow = false;
    for (size_t j = 0; j < HW; ++j) {  // pass 1
        const size_t i = reverse ? HW - 1 - j : j;
        const int a = ia[i], b = ib[i];
        if (!(a >= 0 && a < rows_a && b >= 0 && b < rows_b) || ta[(size_t)a * 10] != tb[(size_t)b * 10]) continue;
        const uint64_t key = trk::pack_key(a, b);
        if (trk::key_a(key) != a || trk::key_b(key) != b || key == 0) std::abort();
        bool stored = false;
        for (uint32_t p = 0; p < max_pairs && !stored; ++p) {
            const uint32_t slot = trk::probe_slot(key, p, max_pairs);
            if (keys[slot] == 0) keys[slot] = key;
            if (keys[slot] == key) {
                ++count[slot];
                stored = true;
            }
        }
        overflow |= !stored;
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
        trk::unpack_link(best_back[r], min_overlap, overflow, &back[2 * r], &back[2 * r + 1]);
        trk::unpack_link(best_fwd[r], min_overlap, overflow, &fwd[2 * r], &fwd[2 * r + 1]);
    }
    link_counts[0] = pairs;
    link_counts[1] = overflow;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    int entries = 0, bad = 0;
    if (std::fread(&entries, 4, 1, fh) != 1) return 2;
    for (int e = 0; e < entries; ++e) {
        int head[6];
        if (std::fread(head, 4, 6, fh) != 6) return 2;
        const int n = head[0], H = head[1], W = head[2], R = head[3], min_overlap = head[5];
        const uint32_t max_pairs = (uint32_t)head[4];
        const size_t HW = (size_t)H * W, nR = (size_t)n * R;
        std::vector<int> index(n * HW), want_back(nR * 2), want_fwd(nR * 2), back(nR * 2), fwd(nR * 2);
        std::vector<int64_t> table(nR * 10), counts(n * 2), want_lc(n * 2), want_tracks(nR * 4), want_state(2), lc(n * 2), tracks(nR * 4);
        if (!read_all(fh, index) || !read_all(fh, table) || !read_all(fh, counts) || !read_all(fh, want_back) || !read_all(fh, want_fwd) ||
            !read_all(fh, want_lc) || !read_all(fh, want_tracks) || !read_all(fh, want_state))
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
                      rows_of(&counts[2 * f], R), HW, R, max_pairs, min_overlap, reverse != 0, bk, fw, &lc[2 * f]);
            }
            int64_t next = 0;  // pass 4
            for (int f = 0; f < n; ++f) {
                const int64_t* pt = f ? &tracks[(size_t)(f - 1) * R * 4] : nullptr;
                const int *bk = &back[(size_t)f * R * 2], *fw = &fwd[(size_t)f * R * 2];
                const int rows = rows_of(&counts[2 * f], R);
                for (int r = 0; r < R; ++r) {
                    int64_t* row = &tracks[((size_t)f * R + r) * 4];
                    if (r >= rows) {
                        row[0] = row[1] = row[2] = -1;
                        row[3] = 0;
                        continue;
                    }
                    int a = bk[2 * r], ov = bk[2 * r + 1];
                    if (a < 0 || a >= R) a = -1, ov = 0;
                    const int64_t pid = a >= 0 && pt ? pt[4 * a] : -1, ppar = a >= 0 && pt ? pt[4 * a + 1] : -1;
                    const bool cont = a >= 0 && trk::continues(a, fw[2 * a], r, pid);
                    row[0] = cont ? pid : next++;
                    row[1] = cont ? ppar : pid;
                    row[2] = a;
                    row[3] = ov;
                }
            }
            const bool same = back == want_back && fwd == want_fwd && lc == want_lc && tracks == want_tracks && next == want_state[0];
            if (!same) {
                std::printf("entry %d (%d x %d x %d, R %d, max_pairs %u, min_overlap %d) reverse %d: differs (back %d fwd %d counts %d tracks %d state %d)\n",
                            e, n, H, W, R, max_pairs, min_overlap, reverse, back == want_back, fwd == want_fwd, lc == want_lc, tracks == want_tracks,
                            next == want_state[0]);
                ++bad;
            }
        }
    }
    std::fclose(fh);
    std::printf("%d entries, %d mismatching runs\n", entries, bad);
    return bad ? 1 : 0;
}
