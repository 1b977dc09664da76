// Georeferencing the flood mosaic on the GPU (include/floodseg_test.h: ground_area, ground_rectify, ground_points).  OUR
// DEFINITION -- the reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.  The projection of a lattice corner,
// the shoelace area of a pixel, the bounds, the sampling rules of the rectified raster and the empty-tile test are ground_defs.h's
// (__host__ __device__, also run on the CPU by the tests); this file is built with -ffp-contract=off so that they round here as there.
//   ground_area     two launches: clear the outputs; one workgroup of 256 per 64 x 16 canvas tile.  It reads its bytes first and
//                   returns if they are all 255.  Otherwise it projects the tile's 65 x 17 lattice corners ONCE into LDS (one division
//                   pair per corner, not four per pixel), every thread takes the shoelace of its four pixels from LDS, the class sums
//                   go through an int64 LDS histogram (one LDS atomic per wave row of one class) flushed with one 64-bit atomic per
//                   non-zero cell, and the region sums are merged per run of equal rows in the wave before they touch memory.
//   ground_rectify  one launch, one owner per raster pixel, no atomics: 64 x 16 raster tiles; a tile whose four corners map beyond one
//                   side of the canvas box writes fill and returns; otherwise one projection per pixel serves every plane and the colour.
//   ground_points   one launch: ground_defs.h's corner per point.
// Every loop bound follows from the arguments or is a constant; no thread waits for another workgroup; the sums are integers, so the
// order does not matter.
#include "kernels.h"
#include "ground_defs.h"

#include <algorithm>

namespace fs {

namespace {

constexpr int TW = 64, TH = 16;        // the tile of both kernels: a wave owns a row of it
constexpr int THREADS = 256;           // four waves; a thread owns the pixels (tid % 64, tid / 64 + 4 k), k = 0..3
constexpr int OWN = TH / (THREADS / 64);  // 4
constexpr int CORNERS = (TW + 1) * (TH + 1);
constexpr int CELLS = 256 + 3;         // the class sums (K <= 255), then the three counts

struct Model9 {
    double m[9];
};
struct PlaneSet {
    const uint8_t* in[gnd::MAX_PLANES];
    uint8_t* out[gnd::MAX_PLANES];
    int n;
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ------------------------------------------------------------------ ground_area 1: the outputs start at zero
__global__ __launch_bounds__(256) void ground_clear_kernel(unsigned long long* __restrict__ class_area2, int K, unsigned long long* __restrict__ region_area2,
                                                           int max_regions, unsigned long long* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < K) class_area2[i] = 0ull;
    if (i < max_regions) region_area2[i] = 0ull;
    if (i < 4) counts[i] = 0ull;
}

__device__ __forceinline__ void region_flush(unsigned long long* region_area2, int lane, int r, unsigned long long sum) {
    if (lane == 0 && r >= 0 && sum != 0ull) atomicAdd(region_area2 + r, sum);
}

// ------------------------------------------------------------------ ground_area 2: one canvas tile per workgroup
__global__ __launch_bounds__(THREADS) void ground_area_kernel(const uint8_t* __restrict__ cls, const int* __restrict__ index, Model9 fwd, int orient, int CH,
                                                              int CW, int ox, int oy, int K, int max_regions, unsigned long long* class_area2,
                                                              unsigned long long* region_area2, unsigned long long* counts) {
    __shared__ long long ce[CORNERS], cn[CORNERS];
    __shared__ unsigned long long cells[CELLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH, X = X0 + lane;
    for (int i = tid; i < CELLS; i += THREADS) cells[i] = 0ull;
    int id[OWN];
    int any = 0;
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int Y = Y0 + wave + 4 * k;
        id[k] = X < CW && Y < CH ? (int)cls[(size_t)Y * CW + X] : (int)gnd::UNSEEN;
        any |= id[k] != (int)gnd::UNSEEN;
    }
    if (!__syncthreads_or(any)) return;  // nothing but unseen ground: the tile has cost its bytes
    for (int q = tid; q < CORNERS; q += THREADS) {
        const int cy = q / (TW + 1), cx = q - cy * (TW + 1);
        if (X0 + cx <= CW && Y0 + cy <= CH) {  // lattice points of the canvas only: the bounds were checked for those
            int64_t e, n;
            gnd::corner(fwd.m, X0 + cx - ox, Y0 + cy - oy, &e, &n);
            ce[q] = e, cn[q] = n;
        }
    }
    __syncthreads();
    unsigned n_summed = 0, n_folded = 0, n_over = 0;  // lane 0's are the wave's
    int run_row = -1;
    unsigned long long run_sum = 0ull;
#pragma unroll
    for (int k = 0; k < OWN; ++k) {  // uniform in the wave: the ballots and shuffles below are whole
        const int ly = wave + 4 * k, Y = Y0 + ly;
        const bool in = X < CW && Y < CH;
        const int c = id[k];
        long long a = 0;
        bool summed = false, fold = false;
        if (in && c < K) {
            const int q = ly * (TW + 1) + lane;
            a = gnd::area2(ce[q], cn[q], ce[q + 1], cn[q + 1], ce[q + TW + 2], cn[q + TW + 2], ce[q + TW + 1], cn[q + TW + 1]) * orient;
            fold = gnd::folded(a);
            summed = !fold;
        }
        const unsigned long long take = __ballot(summed);
        n_summed += (unsigned)__popcll(take);
        n_folded += (unsigned)__popcll(__ballot(fold));
        n_over += (unsigned)__popcll(__ballot(in && c >= K && c != (int)gnd::UNSEEN));
        if (take) {
            // the class sums: one LDS atomic per wave where its summed pixels are of one class, one per pixel otherwise
            const int lead = __ffsll((long long)take) - 1, cell = __shfl(c, lead);
            if (__ballot(summed && c != cell) == 0ull) {
                const unsigned long long sum = wave_sum64(summed ? (unsigned long long)a : 0ull);
                if (lane == lead) atomicAdd(cells + cell, sum);
            } else if (summed) {
                atomicAdd(cells + c, (unsigned long long)a);
            }
        }
        if (index) {
            int r = -1;
            if (summed) {
                const int i = index[(size_t)Y * CW + X];
                if (i >= 0 && i < max_regions) r = i;  // an index read from memory is checked before use
            }
            unsigned long long todo = __ballot(r >= 0);
            while (todo) {  // at most 64 turns: every turn takes at least the leading lane out
                const int lead = __ffsll((long long)todo) - 1, r0 = __shfl(r, lead);
                const bool own = r == r0;
                const unsigned long long sum = wave_sum64(own ? (unsigned long long)a : 0ull);
                if (r0 == run_row) {
                    run_sum += sum;
                } else {
                    region_flush(region_area2, lane, run_row, run_sum);
                    run_row = r0, run_sum = sum;
                }
                todo &= ~__ballot(own);
            }
        }
    }
    region_flush(region_area2, lane, run_row, run_sum);
    if (lane == 0) {
        if (n_summed) atomicAdd(cells + 256, (unsigned long long)n_summed);
        if (n_folded) atomicAdd(cells + 257, (unsigned long long)n_folded);
        if (n_over) atomicAdd(cells + 258, (unsigned long long)n_over);
    }
    __syncthreads();
    for (int i = tid; i < CELLS; i += THREADS) {
        const unsigned long long v = cells[i];
        if (!v) continue;
        if (i < 256) {
            if (i < K) atomicAdd(class_area2 + i, v);
        } else {
            atomicAdd(counts + (i - 256), v);
        }
    }
}

// ------------------------------------------------------------------ ground_rectify: one raster tile per workgroup
__global__ __launch_bounds__(THREADS) void ground_rectify_kernel(PlaneSet planes, const uint32_t* __restrict__ rgba, uint8_t* __restrict__ rgb_out, Model9 inv,
                                                                 int CH, int CW, int ox, int oy, int GH, int GW, int gsd_mm, long long e0_mm,
                                                                 long long ntop_mm, int fill, uint32_t rgb_fill) {
    __shared__ double cx[4], cy[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int U0 = blockIdx.x * TW, V0 = blockIdx.y * TH, u = U0 + lane;
    if (tid < 4) {  // the tile's four lattice corners, clipped to the raster: multiples of a millimetre below 2^53, exact
        const int cu = (tid == 1 || tid == 2) ? min(U0 + TW, GW) : U0, cv = tid >= 2 ? min(V0 + TH, GH) : V0;
        const double du = (double)cu * (double)gsd_mm, dv = (double)cv * (double)gsd_mm;
        const double eg = (double)e0_mm + du, ng = (double)ntop_mm - dv;
        gnd::project(inv.m, eg, ng, &cx[tid], &cy[tid]);
    }
    __syncthreads();
    const bool empty = gnd::tile_outside(cx, cy, ox, oy, CH, CW);
    if (u >= GW) return;
#pragma unroll 1  // rolled: unrolled, the rows' stores each end up behind a wait of their own (tests/test_isa_guards.py)
    for (int k = 0; k < OWN; ++k) {
        const int v = V0 + wave + 4 * k;
        if (v >= GH) continue;
        const size_t at = (size_t)v * GW + u;
        int X = 0, Y = 0;
        double x = 0.0, y = 0.0;
        bool on = false, placed = false;
        if (!empty) {
            double eg, ng;
            gnd::raster_ground(u, v, gsd_mm, e0_mm, ntop_mm, &eg, &ng);
            placed = gnd::ground_to_anchor(inv.m, eg, ng, &x, &y);
            on = placed && gnd::nearest_pixel(x, y, ox, oy, CH, CW, &X, &Y);
        }
        const size_t from = (size_t)Y * CW + X;
        for (int p = 0; p < planes.n; ++p) planes.out[p][at] = on ? planes.in[p][from] : (uint8_t)fill;
        if (rgb_out) {
            uint32_t c = rgb_fill & 0xFFFFFFu;
            if (placed) {
                const auto tap = [&](int tx, int ty) -> uint32_t { return tx >= 0 && tx < CW && ty >= 0 && ty < CH ? rgba[(size_t)ty * CW + tx] : 0u; };
                c = gnd::rectify_colour(tap, x, y, ox, oy, rgb_fill);
            }
            rgb_out[at * 3] = (uint8_t)c, rgb_out[at * 3 + 1] = (uint8_t)(c >> 8), rgb_out[at * 3 + 2] = (uint8_t)(c >> 16);
        }
    }
}

// ------------------------------------------------------------------ ground_points: the corner rule per point
__global__ __launch_bounds__(256) void ground_points_kernel(const int* __restrict__ points, int n, Model9 fwd, int ox, int oy, long long* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int x = points[2 * (size_t)p], y = points[2 * (size_t)p + 1];
    int64_t e = gnd::NO_POINT, nn = gnd::NO_POINT;
    if (x >= -(1 << 20) && x <= (1 << 20) && y >= -(1 << 20) && y <= (1 << 20)) {  // x - ox cannot overflow
        if (!gnd::corner_checked(fwd.m, x - ox, y - oy, &e, &nn)) e = nn = gnd::NO_POINT;
    }
    out[2 * (size_t)p] = e, out[2 * (size_t)p + 1] = nn;
}

const char* refusal_word(int r) {
    switch (r) {
        case gnd::NOT_FINITE: return "a model value is not finite";
        case gnd::DENOMINATOR: return "the denominator is not positive at a corner (the horizon crosses the map)";
        case gnd::RATIO: return "the corner denominators differ by more than a factor of 4";
        case gnd::RANGE: return "a canvas corner lies 2^31 mm or more from the ground origin";
        case gnd::STEP: return "one pixel's corner differences may reach 2^30 mm";
        case gnd::AREA: return "the canvas covers 2^61 mm^2 or more";
        case gnd::ORIENTATION: return "the model's determinant is zero";
    }
    return "ok";
}

int check_model(const char* op, const char* which, int r, const double* m) {
    FS_REQUIRE(r == gnd::OK, "%s: the %s model is refused: %s (model = %.17g %.17g %.17g / %.17g %.17g %.17g / %.17g %.17g %.17g)", op, which, refusal_word(r),
               m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]);
    return 0;
}

int check_canvas(const char* op, int CH, int CW, int ox, int oy) {
    FS_REQUIRE(CH >= 1 && CW >= 1 && CH <= gnd::MAX_SIDE && CW <= gnd::MAX_SIDE, "%s: the canvas must be 1..%d pixels a side, got %dx%d", op, gnd::MAX_SIDE, CH, CW);
    FS_REQUIRE(ox >= -gnd::MAX_ORIGIN && ox <= gnd::MAX_ORIGIN && oy >= -gnd::MAX_ORIGIN && oy <= gnd::MAX_ORIGIN,
               "%s: the origin must lie within %d pixels of the canvas corner, got ox=%d oy=%d", op, gnd::MAX_ORIGIN, ox, oy);
    return 0;
}

Model9 model_of(const double* m) {
    Model9 r;
    for (int k = 0; k < 9; ++k) r.m[k] = m[k];
    return r;
}

}  // namespace

int launch_ground_area(const uint8_t* cls, int CH, int CW, int ox, int oy, const double* forward, int K, const int32_t* index, int max_regions,
                       long long* class_area2, long long* region_area2, long long* counts, hipStream_t s) {
    FS_REQUIRE(cls && forward && class_area2 && counts, "ground_area: null pointer");
    FS_TRY(check_canvas("ground_area", CH, CW, ox, oy));
    FS_REQUIRE(K >= 1 && K <= 255, "ground_area: classes=%d out of range (1..255)", K);
    FS_REQUIRE(max_regions >= 0 && max_regions <= gnd::MAX_REGIONS, "ground_area: max_regions=%d out of range (0..%d)", max_regions, gnd::MAX_REGIONS);
    FS_REQUIRE((index != nullptr) == (max_regions > 0) && (region_area2 != nullptr) == (max_regions > 0),
               "ground_area: index and region_area2 go with max_regions >= 1, and only with it (max_regions=%d)", max_regions);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(index) % 4 == 0, "ground_area: index is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(class_area2) % 8 == 0 && reinterpret_cast<uintptr_t>(region_area2) % 8 == 0 && reinterpret_cast<uintptr_t>(counts) % 8 == 0,
               "ground_area: class_area2, region_area2 or counts is not aligned to 8 bytes");
    FS_TRY(check_model("ground_area", "forward", gnd::check_forward(forward, CH, CW, ox, oy), forward));
    unsigned long long* class_u = reinterpret_cast<unsigned long long*>(class_area2);
    unsigned long long* region_u = reinterpret_cast<unsigned long long*>(region_area2);
    unsigned long long* counts_u = reinterpret_cast<unsigned long long*>(counts);
    hipLaunchKernelGGL(ground_clear_kernel, dim3((unsigned)cdiv(std::max(std::max(K, max_regions), 4), 256)), dim3(256), 0, s, class_u, K, region_u, max_regions,
                       counts_u);
    hipLaunchKernelGGL(ground_area_kernel, dim3((unsigned)cdiv(CW, TW), (unsigned)cdiv(CH, TH)), dim3(THREADS), 0, s, cls, index, model_of(forward),
                       gnd::orientation(forward), CH, CW, ox, oy, K, max_regions, class_u, region_u, counts_u);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_ground_rectify(const double* inverse, int CH, int CW, int ox, int oy, int GH, int GW, int gsd_mm, long long e0_mm, long long ntop_mm, int nplanes,
                          const uint8_t* const* planes, uint8_t* const* outs, const uint32_t* rgba, uint8_t* rgb_out, int fill, uint32_t rgb_fill, hipStream_t s) {
    FS_REQUIRE(inverse, "ground_rectify: null pointer");
    FS_TRY(check_canvas("ground_rectify", CH, CW, ox, oy));
    FS_REQUIRE(GH >= 1 && GW >= 1 && GH <= gnd::MAX_SIDE && GW <= gnd::MAX_SIDE, "ground_rectify: the raster must be 1..%d pixels a side, got %dx%d", gnd::MAX_SIDE,
               GH, GW);
    FS_REQUIRE(gsd_mm >= 1 && gsd_mm <= gnd::MAX_GSD_MM, "ground_rectify: gsd_mm=%d out of range (1..%d)", gsd_mm, gnd::MAX_GSD_MM);
    const long long far = (long long)1 << 40;  // top_left_mm: the raster's far corner then stays below 2^41, exact in a double by far
    FS_REQUIRE(e0_mm > -far && e0_mm < far && ntop_mm > -far && ntop_mm < far, "ground_rectify: top_left_mm must lie within 2^40 mm of the ground origin, got (%lld, %lld)",
               e0_mm, ntop_mm);
    FS_REQUIRE(nplanes >= 0 && nplanes <= gnd::MAX_PLANES, "ground_rectify: %d planes (0..%d)", nplanes, gnd::MAX_PLANES);
    FS_REQUIRE(nplanes == 0 || (planes && outs), "ground_rectify: null pointer");
    FS_REQUIRE((rgba != nullptr) == (rgb_out != nullptr), "ground_rectify: rgba and its raster go together");
    FS_REQUIRE(nplanes > 0 || rgba, "ground_rectify: nothing to rectify (no plane and no rgba)");
    FS_REQUIRE(fill >= 0 && fill <= 255, "ground_rectify: fill=%d out of range (0..255)", fill);
    FS_REQUIRE(rgb_fill <= 0xFFFFFFu, "ground_rectify: rgb_fill=0x%x is no r | g << 8 | b << 16", rgb_fill);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(rgba) % 4 == 0, "ground_rectify: rgba is not aligned to 4 bytes");
    PlaneSet set = {};
    set.n = nplanes;
    for (int p = 0; p < nplanes; ++p) {  // the caller's host arrays
        FS_REQUIRE(planes[p] && outs[p], "ground_rectify: plane %d is null", p);
        set.in[p] = planes[p], set.out[p] = outs[p];
    }
    FS_TRY(check_model("ground_rectify", "inverse", gnd::check_inverse(inverse, GH, GW, gsd_mm, e0_mm, ntop_mm), inverse));
    hipLaunchKernelGGL(ground_rectify_kernel, dim3((unsigned)cdiv(GW, TW), (unsigned)cdiv(GH, TH)), dim3(THREADS), 0, s, set, rgba, rgb_out, model_of(inverse), CH,
                       CW, ox, oy, GH, GW, gsd_mm, e0_mm, ntop_mm, fill, rgb_fill);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_ground_points(const int32_t* points, int n, const double* forward, int ox, int oy, long long* out, hipStream_t s) {
    FS_REQUIRE(points && forward && out, "ground_points: null pointer");
    FS_REQUIRE(n >= 1 && n <= (1 << 28), "ground_points: n=%d out of range (1..2^28)", n);
    FS_REQUIRE(ox >= -gnd::MAX_ORIGIN && ox <= gnd::MAX_ORIGIN && oy >= -gnd::MAX_ORIGIN && oy <= gnd::MAX_ORIGIN,
               "ground_points: the origin must lie within %d pixels of the canvas corner, got ox=%d oy=%d", gnd::MAX_ORIGIN, ox, oy);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(points) % 4 == 0, "ground_points: points is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(out) % 8 == 0, "ground_points: out is not aligned to 8 bytes");
    FS_TRY(check_model("ground_points", "forward", !gnd::finite9(forward) ? gnd::NOT_FINITE : gnd::orientation(forward) == 0 ? gnd::ORIENTATION : gnd::OK, forward));
    hipLaunchKernelGGL(ground_points_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, points, n, model_of(forward), ox, oy, out);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
