// Region overlay of frame egress (definition: include/floodseg_test.h, frame_compose_regions): frame_compose's picture
// plus three optional layers drawn from region_table's index plane and region_tracks' rows -- a fill colour per track id, an outline
// of T pixels inside every region, and the id as a 5 x 7 digit label at the region's centroid.  Integers throughout; every output byte
// is a function of the inputs alone.  Two passes on the stream, nothing read back:
//
// STAMP (labels only).  The marks plane (one byte per pixel, the caller's workspace) is zeroed, then one workgroup per table row works
// out that row's label (overlay_defs.h) and ORs bit 0 (halo) / bit 1 (ink) of every pixel of its halo rectangle into the plane with a
// 32-bit atomicOr on the aligned dword that holds the byte.  OR commutes, so overlapping labels give the same plane in any order of
// arrival.  Every loop is bounded by the rectangle (at most 172 x 36 pixels, 25 trips of 256 threads); rows without a label leave at
// once; no thread waits for another.
//
// COMPOSE.  frame_compose_kernel's work per thread -- two rows by eight columns through the shared pieces of egress_px.h, so the base
// picture, the RGB -> YUV conversion and both store routes are the same code -- with the layers in between.  A workgroup owns a tile
// of 32 rows x 128 columns (16 x 16 threads) and stages the tile's index values with a T-pixel apron in LDS once: (32 + 2T) x
// (128 + 2T) dwords read from HBM / L2 per 4096 pixels (1.08 x the plane at T = 1, 1.33 x at T = 4) instead of (2T + 1)^2 loads per
// pixel.  Cells outside the frame hold NONE, "not a neighbour"; values outside 0 .. R - 1 are stored as -1.  The window test is
// separable: a thread reads the 10 x 16 cells around its 2 x 8 pixels as forty 16-byte LDS reads, folds each column's rows into "all
// r", "mixed" or "none" per output row, and then tests the 2T + 1 column summaries around each pixel: 160 cells and ~1000 integer
// operations per thread whatever T, against 81 x 16 cells.  The loops are unrolled to the largest width and predicated by wave-uniform
// comparisons with T, so every register index is a constant (no scratch).  Layers that are off are uniform branches around their
// loads; with all three off the launcher hands the call to launch_frame_compose itself.
// The slots of a thread past the frame (byte route) and the partner of an odd last row take the finished value of the last pixel
// inside, as in frame_compose_kernel, so that no store sits behind a branch of its own (tests/test_isa_guards.py).
#include "common.h"
#include "egress_px.h"
#include "ingest_src.h"
#include "interp.h"
#include "kernels.h"
#include "overlay_defs.h"

namespace fs {
namespace {

constexpr int TILE_W = 128, TILE_H = 32, APRON = ovl::MAX_WIDTH;
constexpr int TILE_LD = TILE_W + 2 * APRON, TILE_ROWS = TILE_H + 2 * APRON;  // 136 x 40 dwords = 21760 B
constexpr int NONE = -2, MIXED = -3;  // a cell outside the frame; a column whose rows disagree
static_assert(TILE_LD % 4 == 0, "a thread reads its cells as aligned 16-byte words");
static_assert(TILE_W == 128 && TILE_ROWS % 2 == 0 && TILE_ROWS * 2 * APRON <= 2 * 256, "the staging: 256 threads = 2 rows of 128 columns; the apron in two trips");

struct OverlayLayers {
    const int32_t* index;     // [h][w]
    const long long* tracks;  // [R][4] or NULL: the id of a row is the row
    const uint8_t* fill;      // [P][3]
    const uint8_t* outline;   // [K][4] or NULL
    const uint8_t* marks;     // [h][w] bytes, written by the stamp pass
    int R, P, T;              // T = 0 when no outline is drawn
    uint32_t two32_mod_p;     // 2^32 mod P
    int labels;               // 0 | 1
    uint32_t halo, ink;       // R | G << 8 | B << 16 (| A << 24)
};

__global__ __launch_bounds__(256) void stamp_labels_kernel(const long long* __restrict__ table, const long long* __restrict__ counts,
                                                           const long long* __restrict__ tracks, int R, long long min_area, int h, int w, int s,
                                                           uint32_t* __restrict__ marks) {
    __shared__ ovl::Label lab;
    __shared__ uint64_t glyph[ovl::MAX_DIGITS];
    const int r = (int)blockIdx.x;
    if (threadIdx.x == 0) {
        const long long live = counts[1] < R ? counts[1] : R;
        const long long* t = table + (size_t)r * 10;
        lab = ovl::make_label(r, live, tracks ? tracks[(size_t)r * 4] : r, t[1], t[6], t[7], min_area, h, w, s);
        for (int k = 0; k < lab.nd; ++k) glyph[k] = ovl::glyph_bits(lab.digit[k]);
    }
    __syncthreads();
    const ovl::Label& L = lab;
    if (L.nd == 0) return;
    const int rx0 = L.x0 - s, ry0 = L.y0 - s, rw = L.tw + 2 * s, n = rw * (L.th + 2 * s);  // inside the frame: make_label clamps the box
    for (int i = (int)threadIdx.x; i < n; i += 256) {
        const int dy = i / rw, x = rx0 + (i - dy * rw), y = ry0 + dy;
        const uint32_t bits = (uint32_t)ovl::label_marks(L, glyph, s, x, y);
        const size_t a = (size_t)y * w + x;
        atomicOr(marks + (a >> 2), bits << (8 * (a & 3)));
    }
}

__device__ __forceinline__ int fold(int a, int v) { return v == NONE ? a : a == NONE ? v : a == v ? a : MIXED; }

// BG, MODE, YUV_OUT, VEC: frame_compose_kernel's.  Grid: (ceil(w / 128), ceil(h / 32)).
template <int BG, int MODE, bool YUV_OUT, bool VEC>
__global__ __launch_bounds__(256) void frame_compose_regions_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ palette, int K, IngestSrc s,
                                                                    EgressOut o, OverlayLayers L, int h, int w, int npairs, float sy, float sx) {
    __shared__ uint32_t pal[256];   // the class palette per mask value, as frame_compose_kernel's
    __shared__ uint32_t opal[256];  // the outline colours per mask value (A = 0: none)
    __shared__ uint32_t fpal[256];  // the fill colours per id mod P
    __shared__ __attribute__((aligned(16))) int tile[TILE_ROWS * TILE_LD];
    const int tx0 = (int)blockIdx.x * TILE_W, ty0 = (int)blockIdx.y * TILE_H, T = L.T;
    const bool need_index = L.P > 0 || T > 0;
    stage_palette(pal, palette, K);
    if (T > 0) stage_palette(opal, L.outline, K);
    if ((int)threadIdx.x < L.P) {
        const uint8_t* p = L.fill + 3 * threadIdx.x;
        fpal[threadIdx.x] = pack4(p[0], p[1], p[2], 0);
    }
    if (need_index) {
        // Every load of the staging is issued before the first value is used: a loop of load -> LDS store trips pays one memory
        // latency per trip (measured: ~1 us a trip, 16 to 22 trips -- the whole kernel's time).  The centre: thread -> column tid & 127,
        // rows (tid >> 7) + 2 k, 512 contiguous bytes a row; then the 2 T apron columns, <= 320 cells.  Addresses are clamped into the
        // frame and the last row / cell is repeated (the same value into the same LDS cell) instead of branching.
        const int nrows = TILE_H + 2 * T, cx = (int)threadIdx.x & (TILE_W - 1), gx = tx0 + cx;
        int v[TILE_ROWS / 2];
#pragma unroll
        for (int k = 0; k < TILE_ROWS / 2; ++k) {
            const int ry = min(((int)threadIdx.x >> 7) + 2 * k, nrows - 1), gy = ty0 - T + ry;
            const int raw = L.index[(size_t)min(max(gy, 0), h - 1) * w + min(gx, w - 1)];
            v[k] = gy >= 0 && gy < h && gx < w ? ovl::row_or_none(raw, L.R) : NONE;
        }
        int a[2], acell[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            a[k] = NONE, acell[k] = 0;
            if (T > 0) {  // wave-uniform
                const int i = min((int)threadIdx.x + 256 * k, nrows * 2 * T - 1), ry = i / (2 * T), j = i - ry * 2 * T;
                const int col = j < T ? j - T : TILE_W + j - T, gy = ty0 - T + ry, ax = tx0 + col;
                const int raw = L.index[(size_t)min(max(gy, 0), h - 1) * w + min(max(ax, 0), w - 1)];
                a[k] = gy >= 0 && gy < h && ax >= 0 && ax < w ? ovl::row_or_none(raw, L.R) : NONE;
                acell[k] = (APRON - T + ry) * TILE_LD + APRON + col;
            }
        }
#pragma unroll
        for (int k = 0; k < TILE_ROWS / 2; ++k) {
            const int ry = min(((int)threadIdx.x >> 7) + 2 * k, nrows - 1);
            tile[(APRON - T + ry) * TILE_LD + APRON + cx] = v[k];
        }
        if (T > 0) {
#pragma unroll
            for (int k = 0; k < 2; ++k) tile[acell[k]] = a[k];
        }
    }
    __syncthreads();
    const int lgx = (int)threadIdx.x & 15, lpy = (int)threadIdx.x >> 4;
    const int x0 = tx0 + 8 * lgx, py = (ty0 >> 1) + lpy;
    if (x0 >= w || py >= npairs) return;
    const int row[2] = {2 * py, min(2 * py + 1, h - 1)};  // an odd last row is its own partner
    int col[8];                                            // the column each of the eight slots stands for
#pragma unroll
    for (int i = 0; i < 8; ++i) col[i] = VEC ? x0 + i : min(x0 + i, w - 1);

    // the rows of the thread's own pixels, and per pixel whether some in-frame cell of its window holds another row
    int rr[2][8];
    unsigned edge[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) rr[i][k] = -1;
    if (need_index) {
        const int* base = tile + (2 * lpy) * TILE_LD + 8 * lgx;  // the cell of row 2 py - 4, column x0 - 4
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int4 a = *reinterpret_cast<const int4*>(base + (APRON + i) * TILE_LD + APRON);
            const int4 b = *reinterpret_cast<const int4*>(base + (APRON + i) * TILE_LD + APRON + 4);
            rr[i][0] = a.x, rr[i][1] = a.y, rr[i][2] = a.z, rr[i][3] = a.w, rr[i][4] = b.x, rr[i][5] = b.y, rr[i][6] = b.z, rr[i][7] = b.w;
        }
        if (T > 0) {
            int cs[2][16];  // per output row and window column: the column's rows folded
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int i = 0; i < 2; ++i) cs[i][4 * q] = cs[i][4 * q + 1] = cs[i][4 * q + 2] = cs[i][4 * q + 3] = NONE;
#pragma unroll
                for (int d = 0; d < 2 * APRON + 2; ++d) {
                    if (d < APRON - T || d > APRON + 1 + T) continue;  // wave-uniform
                    const int4 v = *reinterpret_cast<const int4*>(base + d * TILE_LD + 4 * q);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int dist = d - APRON - i < 0 ? APRON + i - d : d - APRON - i;
                        if (dist > T) continue;
                        cs[i][4 * q] = fold(cs[i][4 * q], v.x), cs[i][4 * q + 1] = fold(cs[i][4 * q + 1], v.y);
                        cs[i][4 * q + 2] = fold(cs[i][4 * q + 2], v.z), cs[i][4 * q + 3] = fold(cs[i][4 * q + 3], v.w);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    bool e = false;
#pragma unroll
                    for (int dx = -APRON; dx <= APRON; ++dx) {
                        const int c = cs[i][k + APRON + dx];
                        e = e || ((dx < 0 ? -dx : dx) <= T && c != NONE && c != rr[i][k]);
                    }
                    edge[i] |= (e && rr[i][k] >= 0 ? 1u : 0u) << k;
                }
        }
    }

    int px[2][8][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t cls[8];
        egress_classes<VEC>(mask + (size_t)row[r] * w, x0, col, cls);
        float bg[8][3];
        if (BG) egress_background<BG, MODE, VEC>(s, row[r], x0, w, sy, sx, bg);
        uint32_t mk[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) mk[i] = 0;
        if (L.labels) {
            const uint8_t* mrow = L.marks + (size_t)row[r] * w;
            if (VEC) {  // w % 8 == 0 and a 4-byte aligned plane: two dwords
                const uint32_t a = *reinterpret_cast<const uint32_t*>(mrow + x0), b = *reinterpret_cast<const uint32_t*>(mrow + x0 + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) mk[i] = (a >> (8 * i)) & 255, mk[4 + i] = (b >> (8 * i)) & 255;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) mk[i] = mrow[col[i]];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t e = pal[cls[i]];
            const int rw = rr[r][i];
            if (L.P > 0 && rw >= 0) {
                const long long id = L.tracks ? L.tracks[(size_t)rw * 4] : (long long)rw;
                if (id >= 0) {
                    const uint32_t hi = (uint32_t)((unsigned long long)id >> 32), lo = (uint32_t)id, P = (uint32_t)L.P;
                    e = (e & 0xFF000000u) | fpal[((hi % P) * L.two32_mod_p + lo % P) % P];  // id mod P in 32-bit steps (P <= 256)
                }
            }
            egress_blend<BG>(e, bg[i], px[r][i]);
            if ((edge[r] >> i) & 1) {
                const uint32_t oc = opal[cls[i]];
                const int OA = (int)(oc >> 24);  // 0: this class draws no outline, and the blend below is the identity
#pragma unroll
                for (int c = 0; c < 3; ++c) px[r][i][c] = blend255(OA, (int)((oc >> (8 * c)) & 255), px[r][i][c]);
            }
            if (mk[i] & ovl::MARK_INK) {
#pragma unroll
                for (int c = 0; c < 3; ++c) px[r][i][c] = (int)((L.ink >> (8 * c)) & 255);
            } else if (mk[i] & ovl::MARK_HALO) {
#pragma unroll
                for (int c = 0; c < 3; ++c) px[r][i][c] = blend255((int)(L.halo >> 24), (int)((L.halo >> (8 * c)) & 255), px[r][i][c]);
            }
        }
        if (!VEC) {  // a slot past the frame: the last pixel inside, layers included
#pragma unroll
            for (int i = 1; i < 8; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) px[r][i][c] = x0 + i < w ? px[r][i][c] : px[r][i - 1][c];
        }
    }
    if (2 * py + 1 >= h) {  // the odd last row's partner is the row itself (its cells of the tile lie outside the frame)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[1][i][c] = px[0][i][c];
    }
    egress_store<YUV_OUT, VEC>(o, px, row, col, x0, py, w);
}

template <int BG, int MODE>
void launch_out(const uint8_t* mask, const uint8_t* palette, int K, const IngestSrc& s, const EgressOut& o, const OverlayLayers& L, int h, int w, bool yuv_out,
                bool vec, hipStream_t st) {
    const int npairs = cdiv(h, 2);
    const dim3 grid((unsigned)cdiv(w, TILE_W), (unsigned)cdiv(h, TILE_H));
    const float sy = BG ? resize_scale(s.H, h, 0) : 1.f, sx = BG ? resize_scale(s.W, w, 0) : 1.f;
    if (yuv_out && vec)
        frame_compose_regions_kernel<BG, MODE, true, true><<<grid, 256, 0, st>>>(mask, palette, K, s, o, L, h, w, npairs, sy, sx);
    else if (yuv_out)
        frame_compose_regions_kernel<BG, MODE, true, false><<<grid, 256, 0, st>>>(mask, palette, K, s, o, L, h, w, npairs, sy, sx);
    else if (vec)
        frame_compose_regions_kernel<BG, MODE, false, true><<<grid, 256, 0, st>>>(mask, palette, K, s, o, L, h, w, npairs, sy, sx);
    else
        frame_compose_regions_kernel<BG, MODE, false, false><<<grid, 256, 0, st>>>(mask, palette, K, s, o, L, h, w, npairs, sy, sx);
}

template <int BG>
void launch_mode(const uint8_t* mask, const uint8_t* palette, int K, const IngestSrc& s, const EgressOut& o, const OverlayLayers& L, int h, int w, bool yuv_out,
                 bool vec, hipStream_t st) {
    if (s.H == h && s.W == w)
        launch_out<BG, 2>(mask, palette, K, s, o, L, h, w, yuv_out, vec, st);
    else if (s.W == w)
        launch_out<BG, 1>(mask, palette, K, s, o, L, h, w, yuv_out, vec, st);
    else
        launch_out<BG, 0>(mask, palette, K, s, o, L, h, w, yuv_out, vec, st);
}

}  // namespace

// arguments validated by the caller (api_test.hip)
int launch_frame_compose_regions(const uint8_t* mask, int h, int w, const uint8_t* palette, int K, const uint8_t* frame, const uint8_t* u, const uint8_t* v,
                                 int format, int matrix, int full_range, int H, int W, uint8_t* out, uint8_t* out_u, uint8_t* out_v, int out_format,
                                 int out_matrix, int out_full_range, const int32_t* index, const long long* table, const long long* counts,
                                 const long long* tracks, int max_regions, const uint8_t* fill_palette, int P, const uint8_t* outline, int outline_width,
                                 int label_scale, long long label_min_area, uint32_t halo_rgba, uint32_t ink_rgb, void* workspace, hipStream_t st) {
    const int T = outline ? outline_width : 0;
    if (P == 0 && T == 0 && label_scale == 0)  // no layer: frame_compose's picture from frame_compose's kernel
        return launch_frame_compose(mask, h, w, palette, K, frame, u, v, format, matrix, full_range, H, W, out, out_u, out_v, out_format, out_matrix,
                                    out_full_range, st);
    if (label_scale > 0) {
        FS_HIP(hipMemsetAsync(workspace, 0, ((size_t)h * w + 3) / 4 * 4, st));
        stamp_labels_kernel<<<max_regions, 256, 0, st>>>(table, counts, tracks, max_regions, label_min_area, h, w, label_scale,
                                                         static_cast<uint32_t*>(workspace));
        FS_HIP(hipGetLastError());
    }
    OverlayLayers L{};
    L.index = index, L.tracks = tracks, L.fill = fill_palette, L.outline = outline, L.marks = static_cast<const uint8_t*>(workspace);
    L.R = max_regions, L.P = P, L.T = T;
    L.two32_mod_p = P > 0 ? (uint32_t)(((uint64_t)1 << 32) % (uint64_t)P) : 0;
    L.labels = label_scale > 0, L.halo = halo_rgba, L.ink = ink_rgb;
    bool vec;
    const EgressOut o = make_egress_out(mask, w, out, out_u, out_v, out_format, out_matrix, out_full_range, &vec);
    if (!frame) {
        launch_out<0, 2>(mask, palette, K, IngestSrc{}, o, L, h, w, out_format != 0, vec, st);
    } else {
        const IngestSrc s = make_ingest_src(frame, u, v, format, matrix, full_range, H, W);
        if (format == 0)
            launch_mode<1>(mask, palette, K, s, o, L, h, w, out_format != 0, vec, st);
        else
            launch_mode<2>(mask, palette, K, s, o, L, h, w, out_format != 0, vec, st);
    }
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
