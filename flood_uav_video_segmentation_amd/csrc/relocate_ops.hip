// Relocalisation of a lost pose chain against the orthophoto (include/floodseg_test.h: map_coarse, map_patch, map_locate, pose_relocate,
// relocate_commit).  OUR DEFINITION -- the reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.
// The rules -- a coarse cell, the patch's geometry, the order of placements, when a placement is accepted, what is committed -- are
// relocate_defs.h's on top of refine_defs.h (__host__ __device__, also run on the CPU by the tests); the image is ingest_src.h's
// resized1, the one map_view calls cur.  This file is the launches:
//   map_coarse       a thread per cell: S rows of S canvas words; adjacent lanes read adjacent 4 S bytes of a canvas row.
//   map_patch        patch_kernels.h's two launches (cells, finish), which merge_patch shares, on FramePatch below: the geometry is
//                    patch_geometry's on the state row, a pixel is gathered through source_pixel as ortho_accumulate does.
//   map_locate       two launches.  SCORES (the hot one): a workgroup owns 64 x 4 placements, a wave one row of 64 shifts.  The patch goes
//                    through LDS in chunks of 64 x 8 cells, the coarse canvas under the tile as a strip of 128 x 11 cells, both as bytes
//                    with the validity widened to 0x00 / 0xFF.  A lane's window is unaligned by its shift: it reads the aligned dwords
//                    (lane l reads dword l / 4 + k: 32 lanes touch 8 or 9 consecutive banks, equal addresses broadcast) and shifts the
//                    pair with v_alignbyte; the patch dwords are the same address in every lane (broadcast).  Per four cells: one AND of
//                    the two validity dwords, two ANDs, one v_sad_u8 and one popcount of the same mask.  v_mqsad_u32_u8 masks on a ZERO
//                    reference byte (motion_ops.hip), which a valid luma of 0 would trip: it does not fit.  Every placement's (sad, n)
//                    goes to the score plane; no atomics, no thread waits for another workgroup.  BEST: one workgroup folds the plane with
//                    relo::better, a total order, so the order of the fold does not matter; then again for the runner-up.
//   pose_relocate    one wave, lane 0 runs relo::relocate_step.       relocate_commit: one wave, lane 0 runs relo::commit_step; the
//                    decision to copy is taken on the device.
// Every loop bound follows from the arguments or from a geometry that geom_ok / patch_geometry bounded first; nothing is allocated,
// synchronised or read back on the host.  Compile with -ffp-contract=off (csrc/Makefile): the resize must round as ingest's does.
#include "egress_px.h"
#include "ingest_src.h"
#include "kernels.h"
#include "map_checks.h"
#include "patch_kernels.h"

namespace fs {

namespace {

constexpr int THREADS = 256;
constexpr int PU = 64, PV = 4;               // scores: the placements of a workgroup
constexpr int TC = 64, TR = 8;               // scores: a chunk of the patch
constexpr int SW = TC + PU, SR = TR + PV - 1;  // scores: the strip of the coarse canvas under a chunk for every placement of the tile

// ------------------------------------------------------------------ map_coarse
__global__ __launch_bounds__(THREADS) void map_coarse_kernel(const uint32_t* __restrict__ rgba, int CW, int ch, int cw, int S, uint8_t* __restrict__ cl,
                                                             uint8_t* __restrict__ cv) {
    const int cx = blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1)), cy = blockIdx.y * (THREADS / WAVE) + threadIdx.x / WAVE;
    if (cx >= cw || cy >= ch) return;
    uint8_t l, v;
    relo::coarse_cell(rgba, CW, cx, cy, S, &l, &v);
    cl[(size_t)cy * cw + cx] = l, cv[(size_t)cy * cw + cx] = v;
}

// ------------------------------------------------------------------ map_patch: patch_kernels.h's two launches on the frame
struct FrameBox {  // the patch of a lost chain's frame: the state row and patch_geometry's arguments
    static constexpr int ROW_WORDS = mos::STATE_WORDS;
    const long long* row;
    int H, W, CH, CW, ox, oy, S;
    __device__ int geometry(const int64_t* state, int64_t* geom) const { return relo::patch_geometry(state, H, W, CH, CW, ox, oy, S, geom); }
};
template <bool YUV, int MODE>
struct FramePatch : FrameBox {  // its pixels: the frame resized to the mask's size, as ortho_accumulate gathers it
    IngestSrc s;
    float sy, sx;
    __device__ bool luma(const int64_t* state, int64_t X, int64_t Y, uint32_t* l) const {
        int x, y;
        if (!relo::patch_source(state, X, Y, ox, oy, H, W, &x, &y)) return false;
        float v[3];
        resized1<YUV, MODE>(s, y, x, sy, sx, v);
        *l = refn::luma((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]);
        return true;
    }
};

template <bool YUV>
void patch_mode(const IngestSrc& s, const FrameBox& box, uint8_t* tl, uint8_t* tv, hipStream_t st) {
    const float sy = resize_scale(s.H, box.H, 0), sx = resize_scale(s.W, box.W, 0);  // as refine_ops.hip and ortho_ops.hip take them
    if (s.H == box.H && s.W == box.W)
        launch_patch_cells(FramePatch<YUV, 2>{box, s, sy, sx}, box.CH, box.CW, tl, tv, st);
    else if (s.W == box.W)
        launch_patch_cells(FramePatch<YUV, 1>{box, s, sy, sx}, box.CH, box.CW, tl, tv, st);
    else
        launch_patch_cells(FramePatch<YUV, 0>{box, s, sy, sx}, box.CH, box.CW, tl, tv, st);
}

// ------------------------------------------------------------------ map_locate: the score plane
__global__ __launch_bounds__(THREADS) void locate_scores_kernel(const uint8_t* __restrict__ cl, const uint8_t* __restrict__ cv, int ch, int cw,
                                                                const uint8_t* __restrict__ tl, const uint8_t* __restrict__ tv,
                                                                const long long* __restrict__ geom_row, uint2* __restrict__ scores) {
    __shared__ uint32_t s_cl[SR][SW / 4], s_cm[SR][SW / 4], s_tl[TR][TC / 4], s_tm[TR][TC / 4];
    int64_t geom[relo::GEOM_WORDS];
#pragma unroll
    for (int i = 0; i < relo::GEOM_WORDS; ++i) geom[i] = geom_row[i];
    if (!relo::geom_ok(geom, ch, cw)) return;  // uniform
    const int tw = (int)geom[3], th = (int)geom[4], npu = cw - tw + 1, npv = ch - th + 1;
    const int au0 = blockIdx.x * PU, av0 = blockIdx.y * PV;
    if (au0 >= npu || av0 >= npv) return;  // uniform: the grid is sized for the smallest patch
    const int tid = threadIdx.x, ul = tid & (PU - 1), vl = tid / PU;
    const int base = ul >> 2;
    const uint32_t shift = (uint32_t)(ul & 3);
    uint8_t* const b_cl = reinterpret_cast<uint8_t*>(&s_cl[0][0]);
    uint8_t* const b_cm = reinterpret_cast<uint8_t*>(&s_cm[0][0]);
    uint8_t* const b_tl = reinterpret_cast<uint8_t*>(&s_tl[0][0]);
    uint8_t* const b_tm = reinterpret_cast<uint8_t*>(&s_tm[0][0]);
    uint32_t sad = 0, bits = 0;
    for (int j0 = 0; j0 < th; j0 += TR) {
        for (int i0 = 0; i0 < tw; i0 += TC) {
            __syncthreads();  // the chunk before this one has been read
            for (int idx = tid; idx < SR * SW; idx += THREADS) {
                const int r = idx / SW, c = idx - r * SW;
                const int Y = av0 + j0 + r, X = au0 + i0 + c;
                const bool in = Y < ch && X < cw;  // outside the coarse canvas: not valid
                const size_t at = in ? (size_t)Y * cw + X : 0;
                b_cl[idx] = in ? cl[at] : (uint8_t)0;
                b_cm[idx] = (in && cv[at] == 1) ? (uint8_t)0xFF : (uint8_t)0;
            }
            for (int idx = tid; idx < TR * TC; idx += THREADS) {
                const int r = idx / TC, c = idx - r * TC;
                const int j = j0 + r, i = i0 + c;
                const bool in = j < th && i < tw;  // outside the patch: not valid
                const size_t at = in ? (size_t)j * tw + i : 0;
                b_tl[idx] = in ? tl[at] : (uint8_t)0;
                b_tm[idx] = (in && tv[at] == 1) ? (uint8_t)0xFF : (uint8_t)0;
            }
            __syncthreads();
            const int rows = min(TR, th - j0);  // uniform.  Columns past the patch are staged as not valid: all TC / 4 groups run, unrolled
            for (int r = 0; r < rows; ++r) {
                const uint32_t* const row_l = s_cl[r + vl];
                const uint32_t* const row_m = s_cm[r + vl];
                uint32_t lo_l = row_l[base], lo_m = row_m[base];
#pragma unroll
                for (int k = 0; k < TC / 4; ++k) {
                    const uint32_t hi_l = row_l[base + k + 1], hi_m = row_m[base + k + 1];  // base + k + 1 <= 15 + 15 + 1 < SW / 4
                    const uint32_t c = __builtin_amdgcn_alignbyte(hi_l, lo_l, shift);
                    const uint32_t m = __builtin_amdgcn_alignbyte(hi_m, lo_m, shift) & s_tm[r][k];
                    sad = __builtin_amdgcn_sad_u8(c & m, s_tl[r][k] & m, sad);
                    bits += (uint32_t)__popc(m);
                    lo_l = hi_l, lo_m = hi_m;
                }
            }
        }
    }
    const int au = au0 + ul, av = av0 + vl;
    if (au < npu && av < npv) scores[(size_t)av * cw + au] = make_uint2(sad, bits >> 3);  // sad <= 255 x 65536 < 2^24, bits <= 2^19
}

// ------------------------------------------------------------------ map_locate: the best placement and the runner-up
constexpr int FOLD_THREADS = 1024;  // one workgroup: the plane is read twice, so its width is what hides the loads' latency

__device__ relo::Score fold(relo::Score mine, relo::Score* all) {  // every thread gets the block's best
    __syncthreads();
    all[threadIdx.x] = mine;
    __syncthreads();
    for (int half = FOLD_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half && relo::better(all[threadIdx.x + half], all[threadIdx.x])) all[threadIdx.x] = all[threadIdx.x + half];
        __syncthreads();
    }
    return all[0];
}

__global__ __launch_bounds__(FOLD_THREADS) void locate_best_kernel(const uint2* __restrict__ scores, int ch, int cw, const long long* __restrict__ geom_row,
                                                              int permille, int exclude, long long* __restrict__ found_out) {
    __shared__ relo::Score all[FOLD_THREADS];
    __shared__ uint32_t part[FOLD_THREADS / WAVE];
    int64_t geom[relo::GEOM_WORDS], found[relo::FOUND_WORDS];
#pragma unroll
    for (int i = 0; i < relo::GEOM_WORDS; ++i) geom[i] = geom_row[i];
    if (!relo::geom_ok(geom, ch, cw)) {  // uniform
        if (threadIdx.x == 0) {
            relo::write_found(found, relo::FOUND_BAD_GEOM, relo::no_score(), relo::no_score(), 0, 0, 0);
            for (int i = 0; i < relo::FOUND_WORDS; ++i) found_out[i] = found[i];
        }
        return;
    }
    const int tw = (int)geom[3], th = (int)geom[4], npu = cw - tw + 1, npv = ch - th + 1, total = npu * npv;  // at most 2^24
    const int64_t nt = geom[5];
    relo::Score best = relo::no_score();
    uint32_t count = 0;
    for (int p = threadIdx.x; p < total; p += FOLD_THREADS) {
        const int av = p / npu, au = p - av * npu;
        const uint2 s = scores[(size_t)av * cw + au];
        const relo::Score here{(int64_t)s.x, (int64_t)s.y, au - geom[1], av - geom[2]};
        if (!relo::eligible(here.n, nt, permille)) continue;
        count += 1;
        if (relo::better(here, best)) best = here;
    }
    best = fold(best, all);
    count = wave_sum(count);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = count;
    relo::Score second = relo::no_score();
    if (best.n != 0)
        for (int p = threadIdx.x; p < total; p += FOLD_THREADS) {
            const int av = p / npu, au = p - av * npu;
            const uint2 s = scores[(size_t)av * cw + au];
            const relo::Score here{(int64_t)s.x, (int64_t)s.y, au - geom[1], av - geom[2]};
            if (relo::eligible(here.n, nt, permille) && relo::outside(here, best, exclude) && relo::better(here, second)) second = here;
        }
    second = fold(second, all);  // its barriers also publish part[]
    if (threadIdx.x == 0) {
        int64_t fit = 0;
        for (int w = 0; w < FOLD_THREADS / WAVE; ++w) fit += part[w];
        relo::write_found(found, best.n != 0 ? relo::FOUND : relo::FOUND_NONE, best, second, total, fit, nt);
        for (int i = 0; i < relo::FOUND_WORDS; ++i) found_out[i] = found[i];
    }
}

// ------------------------------------------------------------------ pose_relocate and relocate_commit: lane 0 runs the header's step
__global__ __launch_bounds__(WAVE) void pose_relocate_kernel(const long long* __restrict__ found_row, const long long* __restrict__ state_row,
                                                             long long* __restrict__ cand_state, long long* __restrict__ cand_pose, int max_mean,
                                                             int ratio_permille, int H, int W, int CH, int CW, int ox, int oy, int S) {
    if (threadIdx.x != 0) return;
    int64_t found[relo::FOUND_WORDS], state[mos::STATE_WORDS], cs[mos::STATE_WORDS], cp[mos::POSE_WORDS];
    for (int i = 0; i < relo::FOUND_WORDS; ++i) found[i] = found_row[i];
    for (int i = 0; i < mos::STATE_WORDS; ++i) state[i] = state_row[i];
    relo::relocate_step(found, state, cs, cp, max_mean, ratio_permille, H, W, CH, CW, ox, oy, S);
    for (int i = 0; i < mos::STATE_WORDS; ++i) cand_state[i] = cs[i];
    for (int i = 0; i < mos::POSE_WORDS; ++i) cand_pose[i] = cp[i];
}

__global__ __launch_bounds__(WAVE) void relocate_commit_kernel(const long long* __restrict__ cand_state, const long long* __restrict__ cand_pose,
                                                               const long long* __restrict__ correct_out, long long* __restrict__ state,
                                                               long long* __restrict__ pose, const long long* __restrict__ found_row, int S,
                                                               long long* __restrict__ out_row) {
    if (threadIdx.x != 0) return;
    int64_t cs[mos::STATE_WORDS], cp[mos::POSE_WORDS], co[refn::OUT_WORDS], st[mos::STATE_WORDS], p[mos::POSE_WORDS], found[relo::FOUND_WORDS], out[relo::OUT_WORDS];
    for (int i = 0; i < mos::STATE_WORDS; ++i) cs[i] = cand_state[i], st[i] = state[i];
    for (int i = 0; i < mos::POSE_WORDS; ++i) cp[i] = cand_pose[i], p[i] = pose[i];
    for (int i = 0; i < refn::OUT_WORDS; ++i) co[i] = correct_out[i];
    for (int i = 0; i < relo::FOUND_WORDS; ++i) found[i] = found_row[i];
    if (relo::commit_step(cs, cp, co, st, p, found, S, out) == relo::RELOCATED) {  // the copy happens here, on the device
        for (int i = 0; i < relo::COMMIT_STATE_WORDS; ++i) state[i] = st[i];
        for (int i = 0; i < relo::COMMIT_POSE_WORDS; ++i) pose[i] = p[i];
    }
    for (int i = 0; i < relo::OUT_WORDS; ++i) out_row[i] = out[i];
}

}  // namespace

int launch_map_coarse(const uint32_t* rgba, int CH, int CW, int S, uint8_t* cl, uint8_t* cv, hipStream_t s) {
    FS_REQUIRE(rgba && cl && cv, "map_coarse: null pointer");
    FS_TRY(check_sides("map_coarse", "the canvas", 1, CH, CW));
    FS_TRY(check_cell_edge("map_coarse", S));
    FS_TRY(check_has_cell("map_coarse", "canvas", CH, CW, S));
    FS_REQUIRE(aligned(rgba, 4), "map_coarse: rgba is not aligned to 4 bytes");
    const int ch = CH / S, cw = CW / S;
    map_coarse_kernel<<<dim3((unsigned)cdiv(cw, WAVE), (unsigned)cdiv(ch, THREADS / WAVE)), THREADS, 0, s>>>(rgba, CW, ch, cw, S, cl, cv);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_map_patch(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const long long* state, int H,
                     int W, int CH, int CW, int ox, int oy, int S, uint8_t* tl, uint8_t* tv, long long* geom, hipStream_t s) {
    FS_REQUIRE(frame && state && tl && tv && geom, "map_patch: null pointer");
    FS_TRY(check_frame_source("map_patch", u, v, format, matrix, full_range, FH, FW));
    FS_TRY(check_mask_on_canvas("map_patch", 1, H, W, CH, CW, ox, oy));
    FS_TRY(check_cell_edge("map_patch", S));
    FS_TRY(check_has_cell("map_patch", "canvas", CH, CW, S));
    FS_REQUIRE(aligned(state, 8) && aligned(geom, 8), "map_patch: state or geom is not aligned to 8 bytes");
    const IngestSrc src = make_ingest_src(frame, u, v, format, matrix, full_range, FH, FW);
    const FrameBox box = {state, H, W, CH, CW, ox, oy, S};
    if (format == 0)
        patch_mode<false>(src, box, tl, tv, s);
    else
        patch_mode<true>(src, box, tl, tv, s);
    FS_HIP(hipGetLastError());
    patch_finish_kernel<<<1, PATCH_THREADS, 0, s>>>(box, tv, geom);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_map_locate(const uint8_t* cl, const uint8_t* cv, int ch, int cw, const uint8_t* tl, const uint8_t* tv, const long long* geom, int min_overlap_permille,
                      int exclude, uint32_t* scores, long long* found, hipStream_t s) {
    FS_REQUIRE(cl && cv && tl && tv && geom && scores && found, "map_locate: null pointer");
    FS_REQUIRE(ch >= 1 && ch <= mos::MAX_SIDE / 4 && cw >= 1 && cw <= mos::MAX_SIDE / 4, "map_locate: the coarse canvas must be 1..%d cells a side, got %dx%d",
               mos::MAX_SIDE / 4, ch, cw);
    FS_REQUIRE(min_overlap_permille >= 1 && min_overlap_permille <= 1000, "map_locate: min_overlap_permille must be 1..1000, got %d", min_overlap_permille);
    FS_REQUIRE(exclude >= 0 && exclude <= relo::MAX_EXCLUDE, "map_locate: exclude must be 0..%d cells, got %d", relo::MAX_EXCLUDE, exclude);
    FS_REQUIRE(aligned(geom, 8) && aligned(found, 8) && aligned(scores, 8), "map_locate: geom, found or scores is not aligned to 8 bytes");
    locate_scores_kernel<<<dim3((unsigned)cdiv(cw, PU), (unsigned)cdiv(ch, PV)), THREADS, 0, s>>>(cl, cv, ch, cw, tl, tv, geom, reinterpret_cast<uint2*>(scores));
    FS_HIP(hipGetLastError());
    locate_best_kernel<<<1, FOLD_THREADS, 0, s>>>(reinterpret_cast<const uint2*>(scores), ch, cw, geom, min_overlap_permille, exclude, found);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_pose_relocate(const long long* found, const long long* state, long long* cand_state, long long* cand_pose, int max_mean, int ratio_permille, int H, int W,
                         int CH, int CW, int ox, int oy, int S, hipStream_t s) {
    FS_REQUIRE(found && state && cand_state && cand_pose, "pose_relocate: null pointer");
    FS_REQUIRE(max_mean >= 0 && max_mean <= 255, "pose_relocate: max_mean must be 0..255, got %d", max_mean);
    FS_REQUIRE(ratio_permille >= 1 && ratio_permille <= 1000, "pose_relocate: ratio_permille must be 1..1000, got %d", ratio_permille);
    FS_TRY(check_mask_on_canvas("pose_relocate", 1, H, W, CH, CW, ox, oy));
    FS_TRY(check_cell_edge("pose_relocate", S));
    FS_REQUIRE(aligned(found, 8) && aligned(state, 8) && aligned(cand_state, 8) && aligned(cand_pose, 8),
               "pose_relocate: found, state, cand_state or cand_pose is not aligned to 8 bytes");
    FS_REQUIRE(state != cand_state, "pose_relocate: cand_state is the state itself");
    pose_relocate_kernel<<<1, WAVE, 0, s>>>(found, state, cand_state, cand_pose, max_mean, ratio_permille, H, W, CH, CW, ox, oy, S);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_relocate_commit(const long long* cand_state, const long long* cand_pose, const long long* correct_out, long long* state, long long* pose,
                           const long long* found, int S, long long* out, hipStream_t s) {
    FS_REQUIRE(cand_state && cand_pose && correct_out && state && pose && found && out, "relocate_commit: null pointer");
    FS_TRY(check_cell_edge("relocate_commit", S));
    FS_REQUIRE(aligned(cand_state, 8) && aligned(cand_pose, 8) && aligned(correct_out, 8) && aligned(state, 8) && aligned(pose, 8) && aligned(found, 8) &&
                   aligned(out, 8),
               "relocate_commit: a row is not aligned to 8 bytes");
    relocate_commit_kernel<<<1, WAVE, 0, s>>>(cand_state, cand_pose, correct_out, state, pose, found, S, out);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
