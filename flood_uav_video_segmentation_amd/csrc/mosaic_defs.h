// The rules of the flood-extent mosaic (mosaic_ops.hip; definitions: include/floodseg_test.h, global_motion, pose_chain,
// mosaic_accumulate and mosaic_resolve).  Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these
// functions, and a host program (tests/test_mosaic_cpu.py builds tests/mosaic_host_check.cpp) runs them on the CPU.  The two functions
// that work in float64, gm_solve and gm_finish, write every operation out one per statement: the object that holds them is built with
// -ffp-contract=off, so the device rounds each product and each sum exactly as the host build of this header does.
#ifndef FS_MOSAIC_DEFS_H_
#define FS_MOSAIC_DEFS_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_MOS_HD __host__ __device__ __forceinline__
#else
#define FS_MOS_HD inline
#endif

namespace fs {
namespace mos {

constexpr int FRAC = 20;                       // FS_POSE_FRAC: poses and pair models are Q20
constexpr int64_t ONE = (int64_t)1 << FRAC;
constexpr int MAX_FRAMES = 64;                 // n of one call
constexpr int MAX_SIDE = 16384;                // FH, FW, H, W, CH, CW
constexpr int MAX_CLASSES = 32;                // K, and the bits of exclude_set
constexpr int MAX_VECTOR = 32;                 // |dx|, |dy| of a usable row: the matcher's largest search
constexpr int HIST_SIDE = 2 * MAX_VECTOR + 1;  // 65
constexpr int HIST_BINS = HIST_SIDE * HIST_SIDE;
constexpr int MAX_ROUNDS = 8;
constexpr int64_t MAX_TOL_Q20 = 64 * ((int64_t)1 << 20);  // tol_q20 of the call, and the cap of every round's tolerance
constexpr int MODEL_WORDS = 16, POSE_WORDS = 16, STATE_WORDS = 32;
constexpr int SUMS = 12;                       // N, Sp, Sq, Spp, Spq, Sqq, Sdx, Spdx, Sqdx, Sdy, Spdy, Sqdy
enum ModelStatus { MODEL_OK = 0, MODEL_CUT = 1, MODEL_FEW = 2, MODEL_DEGENERATE = 3 };
enum PoseStatus { POSE_OK = 0, POSE_BRIDGED = 1, POSE_LOST = 2 };
enum Phase { PHASE_FRESH = 0, PHASE_TRACKING = 1, PHASE_LOST = 2 };

// ---- THE BOUNDS, and why every product below stays inside 63 bits.
//   a pair model that the chain accepts (pair_in_bounds):     |linear entry| <= 2 ONE = 2^21,   |translation| < 2^16 ONE = 2^36
//   a pose of a frame that is not lost (pose_in_bounds):      |linear entry| <  16 ONE = 2^24  (both directions),
//                                                             |to_anchor translation|   < 2^14 ONE = 2^34,
//                                                             |from_anchor translation| < 2^20 ONE = 2^40
// global_motion's plausible models have forward entries within 1.25 and inverse entries within 1.5 (the determinant is at least
// 0.75^2 - 0.25^2 = 0.5, and g11 / (g00 g11 - c) <= 1 / (0.75 - 0.0625 / 0.75) = 1.5), so the first line refuses nothing it wrote unless
// the camera moved 65536 mask pixels in one frame.  The from_anchor translation is about -(from_anchor's linear part) x (to_anchor's
// translation), at most 2 x 16 x 2^14 = 2^19 pixels: its bound is a net under the rounding of a long chain, not a limit of its own.
//   compose(to_anchor, fwd):    linear 2^24 x 2^21 = 2^45, two of them 2^46;  translation 2^24 x 2^36 = 2^60, two 2^61, + 2^34 < 2^62
//   compose(inv, from_anchor):  linear 2^21 x 2^24 = 2^45, two 2^46;          translation 2^21 x 2^40 = 2^61, two 2^62, + 2^36 < 2^63
//   a canvas pixel:             |X - ox| <= 2^15 (X < 2^14, |ox| <= 2^14), so |AX| = |(2 (X - ox) + 1) << 19| < 2^36;
//                               2^24 x 2^36 = 2^60, two 2^61, + 2^19 and the translation 2^40 < 2^62
//   a rectangle's corner (corner_box, the widest caller): linear entry < 2^24 x (|corner| <= 2^15 whole pixels) = 2^39, two 2^40,
//                               + a translation below 2^41 < 2^42; a caller's origin (|ox| ONE <= 2^34) on top stays below 2^43
// The rounding sums of gm_solve: |p|, |q| < 2^10 and at most 2^20 rows, so every sum is below 2^40 and exact in float64.
constexpr int64_t PAIR_LINEAR_MAX = 2 * ONE;
constexpr int64_t PAIR_SHIFT_LIMIT = ((int64_t)1 << 16) * ONE;
constexpr int64_t POSE_LINEAR_LIMIT = 16 * ONE;
constexpr int64_t POSE_SHIFT_LIMIT = ((int64_t)1 << 14) * ONE;   // to_anchor's: the definition's bound
constexpr int64_t POSE_BACK_SHIFT_LIMIT = ((int64_t)1 << 20) * ONE;
constexpr int64_t PLAUSIBLE = ONE / 4;                           // |m00 - 1|, |m11 - 1|, |m01|, |m10| of a pair
constexpr double PARAM_LIMIT = 1048576.0;                        // a fitted parameter of 2^20 pixels or more is no fit

FS_MOS_HD int64_t rshr(int64_t v) { return (v + ((int64_t)1 << (FRAC - 1))) >> FRAC; }  // arithmetic shift: floor(v / ONE + 1/2)
FS_MOS_HD int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

// ---- affines: (m00, m01, m02, m10, m11, m12), x' = m00 x + m01 y + m02
FS_MOS_HD void identity(int64_t* m) {
    m[0] = ONE, m[1] = 0, m[2] = 0, m[3] = 0, m[4] = ONE, m[5] = 0;
}
// c = a o b (b first).  c may be a or b.
FS_MOS_HD void compose(const int64_t* a, const int64_t* b, int64_t* c) {
    const int64_t c0 = rshr(a[0] * b[0] + a[1] * b[3]), c1 = rshr(a[0] * b[1] + a[1] * b[4]), c2 = rshr(a[0] * b[2] + a[1] * b[5]) + a[2];
    const int64_t c3 = rshr(a[3] * b[0] + a[4] * b[3]), c4 = rshr(a[3] * b[1] + a[4] * b[4]), c5 = rshr(a[3] * b[2] + a[4] * b[5]) + a[5];
    c[0] = c0, c[1] = c1, c[2] = c2, c[3] = c3, c[4] = c4, c[5] = c5;
}
FS_MOS_HD bool linear_within(const int64_t* m, int64_t bound) {  // |entry| <= bound
    return iabs64(m[0]) <= bound && iabs64(m[1]) <= bound && iabs64(m[3]) <= bound && iabs64(m[4]) <= bound;
}
FS_MOS_HD bool shift_below(const int64_t* m, int64_t limit) {  // |translation| < limit
    return iabs64(m[2]) < limit && iabs64(m[5]) < limit;
}
FS_MOS_HD bool pair_in_bounds(const int64_t* fwd, const int64_t* inv) {
    return linear_within(fwd, PAIR_LINEAR_MAX) && linear_within(inv, PAIR_LINEAR_MAX) && shift_below(fwd, PAIR_SHIFT_LIMIT) && shift_below(inv, PAIR_SHIFT_LIMIT);
}
FS_MOS_HD bool pose_in_bounds(const int64_t* to_anchor, const int64_t* from_anchor) {
    return linear_within(to_anchor, POSE_LINEAR_LIMIT - 1) && linear_within(from_anchor, POSE_LINEAR_LIMIT - 1) && shift_below(to_anchor, POSE_SHIFT_LIMIT) &&
           shift_below(from_anchor, POSE_BACK_SHIFT_LIMIT);
}

// ---- THE BOX RULE: the bounding box, in Q20, of the four corners of the whole-pixel rectangle [x0, x1] x [y0, y1] under affine m.  A
// whole pixel times a Q20 entry needs no rounding, so the box is exact; the affine image of the rectangle lies inside it.  Adding a whole
// origin (ox ONE) to a minimum or a maximum is exact too, so origins stay with the callers.  Products: see THE BOUNDS above; every caller
// says in one line why its operands are inside them.  A corner's coordinate m0 x + m1 y + m2 is a term in x plus a term in y, so its
// extremes over the four corners are the sums of the terms' extremes: the corners' own eight products, and no corner is enumerated.
FS_MOS_HD void corner_box(const int64_t* m, int64_t x0, int64_t y0, int64_t x1, int64_t y1, int64_t* lo_x, int64_t* hi_x, int64_t* lo_y, int64_t* hi_y) {
    const int64_t ax0 = m[0] * x0, ax1 = m[0] * x1, ay0 = m[1] * y0, ay1 = m[1] * y1, bx0 = m[3] * x0, bx1 = m[3] * x1, by0 = m[4] * y0, by1 = m[4] * y1;
    *lo_x = (ax0 < ax1 ? ax0 : ax1) + (ay0 < ay1 ? ay0 : ay1) + m[2], *hi_x = (ax0 < ax1 ? ax1 : ax0) + (ay0 < ay1 ? ay1 : ay0) + m[2];
    *lo_y = (bx0 < bx1 ? bx0 : bx1) + (by0 < by1 ? by0 : by1) + m[5], *hi_y = (bx0 < bx1 ? bx1 : bx0) + (by0 < by1 ? by1 : by0) + m[5];
}

// ---- a table row.  Usable: not void, the block centre inside the frame (the matcher writes no other), |dx|, |dy| <= 32; the mask test is
// the caller's (it needs the plane).  The differences are taken in 64 bits: a row is device memory and may hold anything.
FS_MOS_HD bool row_vector(const int32_t* row, int FH, int FW, int* dx, int* dy) {
    const int64_t sx = row[3], sy = row[4], tx = row[5], ty = row[6];
    if (sx < 0 || tx < 0 || ty < 0 || tx >= FW || ty >= FH) return false;
    const int64_t ex = sx - tx, ey = sy - ty;
    if (ex < -MAX_VECTOR || ex > MAX_VECTOR || ey < -MAX_VECTOR || ey > MAX_VECTOR) return false;
    *dx = (int)ex, *dy = (int)ey;
    return true;
}
// the mask pixel under the block centre (floor divisions; the products are below 2^28)
FS_MOS_HD int centre_x(int dst_x, int W, int FW) { const int x = (int)((int64_t)dst_x * W / FW); return x < W - 1 ? x : W - 1; }
FS_MOS_HD int centre_y(int dst_y, int H, int FH) { const int y = (int)((int64_t)dst_y * H / FH); return y < H - 1 ? y : H - 1; }
FS_MOS_HD bool excluded(int cls, uint32_t exclude_set) { return cls < MAX_CLASSES && ((exclude_set >> cls) & 1u) != 0u; }
// block coordinates in units of 8 pixels about the centre of the block grid
FS_MOS_HD int block_p(int dst_x, int wb) { return 2 * (dst_x >> 4) + 1 - wb; }
FS_MOS_HD int block_q(int dst_y, int hb) { return 2 * (dst_y >> 4) + 1 - hb; }

// ---- the histogram's mode as the LARGEST key: the count, then the smallest |dx| + |dy|, then the smallest dy, then the smallest dx
FS_MOS_HD int hist_bin(int dx, int dy) { return (dy + MAX_VECTOR) * HIST_SIDE + (dx + MAX_VECTOR); }
FS_MOS_HD uint64_t mode_key(uint32_t count, int bin) {
    const int dy = bin / HIST_SIDE - MAX_VECTOR, dx = bin % HIST_SIDE - MAX_VECTOR;
    const int mag = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    return ((uint64_t)count << 32) | ((uint64_t)(2 * MAX_VECTOR - mag) << 16) | ((uint64_t)(MAX_VECTOR - dy) << 8) | (uint64_t)(MAX_VECTOR - dx);
}
FS_MOS_HD uint32_t key_count(uint64_t key) { return (uint32_t)(key >> 32); }
FS_MOS_HD int key_dx(uint64_t key) { return MAX_VECTOR - (int)(key & 0xffu); }
FS_MOS_HD int key_dy(uint64_t key) { return MAX_VECTOR - (int)((key >> 8) & 0xffu); }

// ---- a round: tolerance, inlier test, the row's share of the twelve sums
FS_MOS_HD int64_t round_tolerance(int64_t tol_q20, int rounds, int r) {
    const int64_t cap = MAX_TOL_Q20, wide = tol_q20 << (rounds - 1 - r);  // tol_q20 <= 2^26 and a shift of 0..7: below 2^34
    return wide < cap ? wide : cap;
}
// model = (a0, a1, a2, b0, b1, b2): |a| < 2^40 (gm_solve), |p|, |q| < 2^10: every term is below 2^50
FS_MOS_HD bool is_inlier(const int64_t* model, int p, int q, int dx, int dy, int64_t T) {
    const int64_t px = model[0] + model[1] * p + model[2] * q, py = model[3] + model[4] * p + model[5] * q;
    return iabs64((int64_t)dx * ONE - px) <= T && iabs64((int64_t)dy * ONE - py) <= T;
}
FS_MOS_HD void add_row(int64_t* s, int p, int q, int dx, int dy) {
    s[0] += 1, s[1] += p, s[2] += q, s[3] += (int64_t)p * p, s[4] += (int64_t)p * q, s[5] += (int64_t)q * q;
    s[6] += dx, s[7] += (int64_t)p * dx, s[8] += (int64_t)q * dx, s[9] += dy, s[10] += (int64_t)p * dy, s[11] += (int64_t)q * dy;
}

// ---- the least-squares model of one round from the twelve sums: the 3 x 3 normal equations by Cramer's rule in float64, in THIS order
// of operations, no fused multiply-add; each parameter rounded to Q20 to nearest, ties to even.  false: the determinant came out as 0,
// or a parameter is not a finite number below 2^20 pixels (degenerate either way); model is then untouched.
FS_MOS_HD bool q20_of(double v, int64_t* out) {
    if (!(v > -PARAM_LIMIT && v < PARAM_LIMIT)) return false;  // a NaN fails both comparisons
    const double scaled = v * 1048576.0;                        // exact: a power of two
    *out = (int64_t)llrint(scaled);
    return true;
}
FS_MOS_HD bool gm_solve(const int64_t* s, int64_t* model) {
    const double m00 = (double)s[0], m01 = (double)s[1], m02 = (double)s[2], m11 = (double)s[3], m12 = (double)s[4], m22 = (double)s[5];
    double t0, t1;
    t0 = m11 * m22, t1 = m12 * m12;
    const double c00 = t0 - t1;
    t0 = m01 * m22, t1 = m12 * m02;
    const double c01 = t0 - t1;
    t0 = m01 * m12, t1 = m11 * m02;
    const double c02 = t0 - t1;
    t0 = m00 * m22, t1 = m02 * m02;
    const double c11 = t0 - t1;
    t0 = m00 * m12, t1 = m01 * m02;
    const double c12 = t0 - t1;
    t0 = m00 * m11, t1 = m01 * m01;
    const double c22 = t0 - t1;
    t0 = m00 * c00, t1 = m01 * c01;
    double det = t0 - t1;
    t0 = m02 * c02;
    det = det + t0;
    if (det == 0.0) return false;
    int64_t out[6];
    for (int k = 0; k < 2; ++k) {
        const double r0 = (double)s[6 + 3 * k], r1 = (double)s[7 + 3 * k], r2 = (double)s[8 + 3 * k];
        double u;
        t0 = c00 * r0, t1 = c01 * r1;
        u = t0 - t1;
        t0 = c02 * r2;
        u = u + t0;
        const double v0 = u / det;
        t0 = c11 * r1, t1 = c01 * r0;
        u = t0 - t1;
        t0 = c12 * r2;
        u = u - t0;
        const double v1 = u / det;
        t0 = c02 * r0, t1 = c12 * r1;
        u = t0 - t1;
        t0 = c22 * r2;
        u = u + t0;
        const double v2 = u / det;
        if (!q20_of(v0, out + 3 * k) || !q20_of(v1, out + 3 * k + 1) || !q20_of(v2, out + 3 * k + 2)) return false;
    }
    for (int i = 0; i < 6; ++i) model[i] = out[i];
    return true;
}

// ---- the pair model in mask pixels.  In frame pixels x_prev = x + a0 + a1 (x - 8 wb) / 8 + a2 (y - 8 hb) / 8 (y alike); scaled to mask
// pixels, rounded ONCE to Q20; the inverse from the QUANTISED forward model, rounded once.  false: implausible (or out of the chain's
// bounds); fwd and inv are then the identity.
FS_MOS_HD bool gm_finish(const int64_t* model, int FH, int FW, int H, int W, int64_t* fwd, int64_t* inv) {
    identity(fwd);
    identity(inv);
    const double one = 1048576.0;
    const double a0 = (double)model[0] / one, a1 = (double)model[1] / one, a2 = (double)model[2] / one;
    const double b0 = (double)model[3] / one, b1 = (double)model[4] / one, b2 = (double)model[5] / one;
    const double wb = (double)(FW / 16), hb = (double)(FH / 16);
    const double dW = (double)W, dH = (double)H, dFW = (double)FW, dFH = (double)FH;
    const double sx = dW / dFW, sy = dH / dFH;
    double t0, t1;
    t0 = dW * dFH, t1 = dFW * dH;
    const double kxy = t0 / t1;  // (W FH) / (FW H)
    t0 = dH * dFW, t1 = dFH * dW;
    const double kyx = t0 / t1;  // (H FW) / (FH W)
    double f[6];
    t0 = a1 / 8.0;
    f[0] = 1.0 + t0;
    t0 = a2 / 8.0;
    f[1] = t0 * kxy;
    t0 = a1 * wb, t1 = a2 * hb;
    t0 = a0 - t0;
    t0 = t0 - t1;
    f[2] = t0 * sx;
    t0 = b1 / 8.0;
    f[3] = t0 * kyx;
    t0 = b2 / 8.0;
    f[4] = 1.0 + t0;
    t0 = b1 * wb, t1 = b2 * hb;
    t0 = b0 - t0;
    t0 = t0 - t1;
    f[5] = t0 * sy;
    int64_t m[6], w[6];
    for (int i = 0; i < 6; ++i)
        if (!q20_of(f[i], m + i)) return false;
    if (iabs64(m[0] - ONE) > PLAUSIBLE || iabs64(m[4] - ONE) > PLAUSIBLE || iabs64(m[1]) > PLAUSIBLE || iabs64(m[3]) > PLAUSIBLE) return false;
    const double g00 = (double)m[0] / one, g01 = (double)m[1] / one, g02 = (double)m[2] / one;
    const double g10 = (double)m[3] / one, g11 = (double)m[4] / one, g12 = (double)m[5] / one;
    t0 = g00 * g11, t1 = g01 * g10;
    const double det = t0 - t1;  // at least 0.5
    const double i00 = g11 / det, i11 = g00 / det;
    t0 = g01 / det;
    const double i01 = -t0;
    t0 = g10 / det;
    const double i10 = -t0;
    t0 = i00 * g02, t1 = i01 * g12;
    t0 = t0 + t1;
    const double i02 = -t0;
    t0 = i10 * g02, t1 = i11 * g12;
    t0 = t0 + t1;
    const double i12 = -t0;
    if (!q20_of(i00, w) || !q20_of(i01, w + 1) || !q20_of(i02, w + 2) || !q20_of(i10, w + 3) || !q20_of(i11, w + 4) || !q20_of(i12, w + 5)) return false;
    if (!pair_in_bounds(m, w)) return false;
    for (int i = 0; i < 6; ++i) fwd[i] = m[i], inv[i] = w[i];
    return true;
}

// ---- one row of `model`: forward (6), inverse (6), status, usable rows, inliers, rounds completed
FS_MOS_HD void write_model(int64_t* row, const int64_t* fwd, const int64_t* inv, int status, int64_t usable, int64_t inliers, int rounds_done) {
    for (int i = 0; i < 6; ++i) row[i] = fwd[i], row[6 + i] = inv[i];
    row[12] = status, row[13] = usable, row[14] = inliers, row[15] = rounds_done;
}

// ---- the pose chain: one frame.  state: to_anchor (6), from_anchor (6), last_fwd (6), last_inv (6), phase, frames seen, frames lost, the
// current bridge run, 4 spare words (zero).  Everything read from `model` and `state` is tested before use: a status that is none of
// 0..3 counts as 3, an ok model out of the pair bounds counts as 3, a phase that is none of 0..2 counts as lost.
// frame_clipped: a corner outside the canvas [0, CW] x [0, CH] is an edge of the corners' box outside it; pose_in_bounds held to_anchor.
FS_MOS_HD bool frame_clipped(const int64_t* to_anchor, int H, int W, int CH, int CW, int ox, int oy) {
    int64_t lo_x, hi_x, lo_y, hi_y;
    corner_box(to_anchor, 0, 0, W, H, &lo_x, &hi_x, &lo_y, &hi_y);
    return lo_x + (int64_t)ox * ONE < 0 || lo_y + (int64_t)oy * ONE < 0 || hi_x + (int64_t)ox * ONE > (int64_t)CW * ONE || hi_y + (int64_t)oy * ONE > (int64_t)CH * ONE;
}
FS_MOS_HD void pose_step(const int64_t* model, int64_t* state, int64_t* pose, int H, int W, int CH, int CW, int ox, int oy, int max_bridge) {
    int64_t* to_anchor = state;
    int64_t* from_anchor = state + 6;
    int64_t* last_fwd = state + 12;
    int64_t* last_inv = state + 18;
    const int64_t phase = state[24];
    int status = POSE_OK;
    int64_t inliers = 0, usable = 0;
    if (phase == PHASE_FRESH) {  // the anchor: its own model row relates it to a frame outside the mosaic
        identity(to_anchor), identity(from_anchor), identity(last_fwd), identity(last_inv);
        state[24] = PHASE_TRACKING, state[27] = 0;
    } else if (phase != PHASE_TRACKING) {
        status = POSE_LOST;
    } else {
        int st = model[12] == MODEL_OK ? MODEL_OK : model[12] == MODEL_CUT ? MODEL_CUT : MODEL_DEGENERATE;
        if (st == MODEL_OK && !pair_in_bounds(model, model + 6)) st = MODEL_DEGENERATE;
        inliers = model[14], usable = model[13];
        if (st == MODEL_OK) {
            for (int i = 0; i < 6; ++i) last_fwd[i] = model[i], last_inv[i] = model[6 + i];
            state[27] = 0;
        } else if (st == MODEL_CUT || state[27] < 0 || state[27] >= max_bridge || !pair_in_bounds(last_fwd, last_inv)) {
            status = POSE_LOST;
        } else {
            status = POSE_BRIDGED;
            state[27] += 1;
        }
        if (status != POSE_LOST) {
            int64_t to_next[6] = {0, 0, 0, 0, 0, 0}, from_next[6] = {0, 0, 0, 0, 0, 0};
            bool ok = pose_in_bounds(to_anchor, from_anchor);  // the state is device memory too
            if (ok) {
                compose(to_anchor, last_fwd, to_next);
                compose(last_inv, from_anchor, from_next);
                ok = pose_in_bounds(to_next, from_next);
            }
            if (ok) {
                for (int i = 0; i < 6; ++i) to_anchor[i] = to_next[i], from_anchor[i] = from_next[i];
            } else {
                status = POSE_LOST;
            }
        }
        if (status == POSE_LOST) state[24] = PHASE_LOST;
    }
    state[25] += 1;
    if (status == POSE_LOST) {
        state[26] += 1;
        identity(pose), identity(pose + 6);
        pose[12] = POSE_LOST, pose[13] = 0;
    } else {
        for (int i = 0; i < 6; ++i) pose[i] = to_anchor[i], pose[6 + i] = from_anchor[i];
        pose[12] = status, pose[13] = frame_clipped(to_anchor, H, W, CH, CW, ox, oy) ? 1 : 0;
    }
    pose[14] = inliers, pose[15] = usable;
}

// ---- the gather: the frame pixel under the centre of canvas pixel (X, Y) with the anchor's corner at (ox, oy)
FS_MOS_HD bool pose_votes(const int64_t* pose) {  // a row of `poses` is device memory: status and bounds are tested before use
    return (pose[12] == POSE_OK || pose[12] == POSE_BRIDGED) && linear_within(pose + 6, POSE_LINEAR_LIMIT - 1) && shift_below(pose + 6, POSE_BACK_SHIFT_LIMIT);
}
FS_MOS_HD int64_t anchor_coord(int X, int ox) { return (2 * ((int64_t)X - ox) + 1) * (ONE / 2); }  // (2 (X - ox) + 1) << 19, negative values included
FS_MOS_HD void source_pixel(const int64_t* from_anchor, int64_t AX, int64_t AY, int64_t* x, int64_t* y) {
    *x = (rshr(from_anchor[0] * AX + from_anchor[1] * AY) + from_anchor[2]) >> FRAC;
    *y = (rshr(from_anchor[3] * AX + from_anchor[4] * AY) + from_anchor[5]) >> FRAC;
}
// can frame `from_anchor` touch the canvas rectangle [X0, X1) x [Y0, Y1)?  Its image lies inside corner_box's box (|X - ox| <= 2^15, a
// translation below 2^41); a pixel's rounded source lies within one Q20 unit of its centre's exact image: one whole pixel is allowed for.
FS_MOS_HD bool touches(const int64_t* from_anchor, int X0, int Y0, int X1, int Y1, int ox, int oy, int H, int W) {
    int64_t lo_x, hi_x, lo_y, hi_y;
    corner_box(from_anchor, (int64_t)X0 - ox, (int64_t)Y0 - oy, (int64_t)X1 - ox, (int64_t)Y1 - oy, &lo_x, &hi_x, &lo_y, &hi_y);
    return hi_x >= -ONE && lo_x <= (int64_t)(W + 1) * ONE && hi_y >= -ONE && lo_y <= (int64_t)(H + 1) * ONE;
}
FS_MOS_HD uint16_t vote_add(uint16_t v, uint32_t more) {  // `more` single votes, each saturating at 65535
    const uint32_t s = (uint32_t)v + more;
    return (uint16_t)(s > 65535u ? 65535u : s);
}

// ---- resolve: one canvas pixel's K counts -> class (lowest id on a tie; 255: none), confidence, total
FS_MOS_HD uint8_t vote_confidence(uint32_t most, uint32_t total) { return total == 0u ? (uint8_t)0 : (uint8_t)((255u * most + total / 2u) / total); }

}  // namespace mos
}  // namespace fs

#endif  // FS_MOSAIC_DEFS_H_
