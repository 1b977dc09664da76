// The two launches of a patch of coarse cells, once, for map_patch (relocate_ops.hip: the pixels are the frame's through resized1) and
// merge_patch (merge_ops.hip: the pixels are canvas B's through patch_pixel); DESIGN §3.22, §3.23.  Device code: the rules are
// relocate_defs.h's.  What differs between the two ops is a small SOURCE type that each file defines next to its launcher:
//   a Box     `row` (the state or the link, ROW_WORDS int64 at a uniform address), S, and
//             int geometry(const int64_t* row, int64_t* geom)                         patch_geometry or box_geometry on the loaded row
//   a Patch   a Box, and bool luma(const int64_t* row, int64_t X, int64_t Y, uint32_t* l)   the luma under canvas pixel (X, Y), or false
// Cells: a wave per patch cell, four cells a workgroup; every wave derives the geometry from the row (scalar loads), a lane takes the
// pixels lane, lane + 64, .. of the cell's S^2, one ballot says whether any was missing and wave_sum adds the lumas.  Finish: one
// workgroup counts the valid cells and writes geom.
#ifndef FS_PATCH_KERNELS_H_
#define FS_PATCH_KERNELS_H_

#include "kernels.h"
#include "relocate_defs.h"

namespace fs {

constexpr int WAVE = 64, PATCH_THREADS = 256;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

template <class Patch>
__global__ __launch_bounds__(PATCH_THREADS) void patch_cells_kernel(Patch src, uint8_t* __restrict__ tl, uint8_t* __restrict__ tv) {
    int64_t row[Patch::ROW_WORDS], geom[relo::GEOM_WORDS];  // the same address in every thread: scalar loads
#pragma unroll
    for (int i = 0; i < Patch::ROW_WORDS; ++i) row[i] = src.row[i];
    if (src.geometry(row, geom) != relo::PATCH_OK) return;  // uniform
    const int S = src.S, tw = (int)geom[3], th = (int)geom[4], lane = threadIdx.x & (WAVE - 1);
    const int cell = blockIdx.x * (PATCH_THREADS / WAVE) + threadIdx.x / WAVE;  // wave-uniform
    if (cell >= tw * th) return;
    const int j = cell / tw, i = cell - j * tw;
    const int64_t X0 = (geom[1] + i) * S, Y0 = (geom[2] + j) * S;
    uint32_t sum = 0;
    bool ok = true;
    for (int p = lane; p < S * S; p += WAVE) {
        uint32_t l;
        if (!src.luma(row, X0 + p % S, Y0 + p / S, &l)) {
            ok = false;
            continue;
        }
        sum += l;
    }
    const bool all = __ballot(!ok) == 0ull;
    sum = wave_sum(sum);
    if (lane == 0) tl[cell] = all ? (uint8_t)relo::cell_mean(sum, S) : (uint8_t)0, tv[cell] = all ? 1 : 0;
}

template <class Box>
__global__ __launch_bounds__(PATCH_THREADS) void patch_finish_kernel(Box src, const uint8_t* __restrict__ tv, long long* __restrict__ geom_out) {
    __shared__ uint32_t part[PATCH_THREADS / WAVE];
    int64_t row[Box::ROW_WORDS], geom[relo::GEOM_WORDS];
#pragma unroll
    for (int i = 0; i < Box::ROW_WORDS; ++i) row[i] = src.row[i];
    const bool ok = src.geometry(row, geom) == relo::PATCH_OK;  // uniform
    uint32_t count = 0;
    if (ok)
        for (int c = threadIdx.x; c < (int)(geom[3] * geom[4]); c += PATCH_THREADS) count += tv[c] == 1 ? 1u : 0u;
    count = wave_sum(count);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        geom[5] = ok ? (int64_t)(part[0] + part[1] + part[2] + part[3]) : 0;
        for (int i = 0; i < relo::GEOM_WORDS; ++i) geom_out[i] = geom[i];
    }
}

// CH, CW: the canvas the patch is placed on.  A patch that passes has no more cells than its coarse canvas, and at most 65536.
template <class Patch>
void launch_patch_cells(const Patch& src, int CH, int CW, uint8_t* tl, uint8_t* tv, hipStream_t st) {
    const int64_t cells = (int64_t)(CH / src.S) * (CW / src.S);
    const dim3 grid((unsigned)cdiv64(cells < relo::MAX_PATCH_CELLS ? cells : relo::MAX_PATCH_CELLS, PATCH_THREADS / WAVE));
    patch_cells_kernel<Patch><<<grid, PATCH_THREADS, 0, st>>>(src, tl, tv);
}

}  // namespace fs

#endif  // FS_PATCH_KERNELS_H_
